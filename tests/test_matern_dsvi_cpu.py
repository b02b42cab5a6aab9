"""Host-side checks of the Matern DSVI layers (no GPU): the `nu=` keyword of models.dgps, which kernels a
VariationalStrategy accepts, the argument checks of nsgp_i8_matern_build_f32 (negative return = index of the offending
argument in its signature, 0 for empty sizes, both before any launch) and the argument errors of the projection entry
points and of the layer nodes."""
import ctypes

import pytest
import torch

NUS = (0.5, 1.5, 2.5)


def _kernels(model):
    return model.layers[0].covar_module.base_kernel, model.last_layer.covar_module.base_kernel


def test_deepgp_nu_keyword_forms():
    import models.dgps as m
    from nsgp.gp.kernels import MaternKernel, RBFKernel
    for nu in NUS:
        h, l_ = _kernels(m.DeepGP(1, (100, 3), num_inducing=8, nu=nu))
        assert isinstance(h, MaternKernel) and isinstance(l_, MaternKernel) and h.nu == nu and l_.nu == nu
    h, l_ = _kernels(m.DeepGP(1, (100, 3), num_inducing=8, nu=(None, 2.5)))
    assert type(h) is RBFKernel and isinstance(l_, MaternKernel) and l_.nu == 2.5
    h, l_ = _kernels(m.DeepGP(2, (100, 3), num_inducing=8, nu=[0.5, None], tie_layers=False))
    assert isinstance(h, MaternKernel) and h.nu == 0.5 and type(l_) is RBFKernel
    model = m.DeepGP(2, (100, 3), num_inducing=8, nu=(1.5, 0.5), tie_layers=False)
    assert [lay.covar_module.base_kernel.nu for lay in model.layers] == [1.5, 1.5]
    assert [lay.variational_strategy.nu for lay in list(model.layers) + [model.last_layer]] == [1.5, 1.5, 0.5]
    layer = m.DeepGPHiddenLayer(3, 2, 8, 'linear', nu=1.5)
    assert layer.variational_strategy.nu == 1.5 and m.DeepGPHiddenLayer(3, 2, 8).variational_strategy.nu is None


@pytest.mark.parametrize('bad', [2.0, 0, '1.5', (1.5,), (1.5, 2.0), (0.5, 1.5, 2.5), [2.5, 3.5]])
def test_deepgp_bad_nu_raises_the_matern_kernels_error(bad):
    import models.dgps as m
    with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
        m.DeepGP(1, (100, 3), num_inducing=8, nu=bad)
    with pytest.raises(TypeError):
        m.DeepGP(1, (100, 3), 8, True, 'cholesky', None, 1.5)             # keyword-only


@pytest.mark.parametrize('variational', ['cholesky', 'mean_field'])
def test_nu_none_is_todays_model_and_matern_keeps_its_parameter_names_and_shapes(variational):
    import models.dgps as m
    from nsgp.gp.kernels import RBFKernel
    torch.manual_seed(0)
    ref = m.DeepGP(1, (100, 3), num_inducing=8, variational=variational)
    torch.manual_seed(0)
    same = m.DeepGP(1, (100, 3), num_inducing=8, variational=variational, nu=None)
    assert all(type(k) is RBFKernel for k in _kernels(same))
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in same.state_dict().items()]
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), same.state_dict().values()))
    torch.manual_seed(0)
    mat = m.DeepGP(1, (100, 3), num_inducing=8, variational=variational, nu=1.5)
    assert [(k, tuple(v.shape)) for k, v in ref.state_dict().items()] == [(k, tuple(v.shape)) for k, v in mat.state_dict().items()]
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), mat.state_dict().values()))     # same draws
    assert all(s.nu is None for s in (ref.layers[0].variational_strategy, ref.last_layer.variational_strategy))


def test_variational_strategy_takes_rbf_and_matern_and_refuses_the_rest():
    import models.dgps as m
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, RBFKernel, ScaleKernel
    layer = m.DeepGPHiddenLayer(2, None, 6, nu=2.5)
    vs = layer.variational_strategy
    Z, ls, os_ = vs.whiten_group()
    assert Z.shape == (1, 6, 2) and ls.shape == (1, 2) and os_.shape == (1,) and len(vs.whiten_group()) == 3
    assert len(vs._flat_params()) == 5 and vs.nu == 2.5
    for bad in (ScaleKernel(PeriodicKernel()), ScaleKernel(RBFKernel() * PeriodicKernel()), MaternKernel(nu=1.5), RBFKernel()):
        layer.covar_module = bad
        with pytest.raises(NotImplementedError, match='ScaleKernel\\(RBFKernel\\) and, in the layers of a deep GP'):
            vs.whiten_group()
        with pytest.raises(NotImplementedError):
            vs.nu


def test_matern_is_taken_by_deep_gp_layers_only():
    """A stand-alone ApproximateGP keeps refusing ScaleKernel(MaternKernel), as tests/test_gpu_matern.py pins it; the same
    strategy and kernel inside a DeepGPLayer are accepted."""
    import nsgp.gp as gpytorch
    from nsgp.gp.kernels import MaternKernel, ScaleKernel
    from nsgp.gp.models import ApproximateGP, DeepGPLayer
    from nsgp.gp.variational import CholeskyVariationalDistribution, VariationalStrategy

    def make(base, *extra):
        class Layer(base):
            def __init__(self, z):
                vd = CholeskyVariationalDistribution(z.shape[-2])
                super().__init__(VariationalStrategy(self, z, vd, learn_inducing_locations=True), *extra)
                self.mean_module = gpytorch.means.ConstantMean()
                self.covar_module = ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=2))
        return Layer(torch.randn(6, 2))
    with pytest.raises(NotImplementedError, match='in a Layer'):
        make(ApproximateGP).variational_strategy.whiten_group()
    with pytest.raises(NotImplementedError):
        make(ApproximateGP).variational_strategy.nu
    vs = make(DeepGPLayer, 2, None).variational_strategy
    assert vs.nu == 2.5 and len(vs.whiten_group()) == 3


def test_i8_matern_build_argument_checks_return_before_any_launch():
    from nsgp import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    #     Z  x  sx ls os batch M   n   D  nu2 planes Kd kscale Kzx_f32 stream
    ok = [b, b, 0, b, b, 1, 128, 64, 2, 3, 4, b, b, None, None]
    call = lambda i=None, v=None: lib.nsgp_i8_matern_build_f32(*[v if k == i else a for k, a in enumerate(ok)])   # noqa: E731
    assert call(0, None) == -1 and call(1, None) == -2 and call(2, -1) == -3 and call(3, None) == -4 and call(4, None) == -5
    assert call(5, -1) == -6 and call(5, 65536) == -6
    assert call(6, -1) == -7 and call(6, 4097) == -7
    assert call(7, -1) == -8
    assert call(8, 0) == -9 and call(8, 5) == -9
    for nu2 in (0, 2, 4, 6, -1, 7):
        assert call(9, nu2) == -10
    assert call(10, 3) == -11 and call(10, 6) == -11
    assert call(11, None) == -12 and call(12, None) == -13
    # empty sizes: 0, no launch (there is no GPU here), for every nu and both plane counts
    for nu2 in (1, 3, 5):
        for planes in (4, 5):
            for i in (5, 6, 7):
                args = [0 if k == i else a for k, a in enumerate(ok)]
                args[9], args[10] = nu2, planes
                assert lib.nsgp_i8_matern_build_f32(*args) == 0
    # a bad argument wins over an empty size
    args = list(ok)
    args[7], args[9] = 0, 2
    assert lib.nsgp_i8_matern_build_f32(*args) == -10
    # the RBF entry keeps its codes
    okr = [b, b, 0, b, b, 1, 128, 64, 2, 4, b, b, None, None]
    assert lib.nsgp_i8_rbf_build_f32(*[3 if k == 9 else a for k, a in enumerate(okr)]) == -10
    assert lib.nsgp_i8_rbf_build_f32(*[None if k == 11 else a for k, a in enumerate(okr)]) == -11
    assert lib.nsgp_i8_rbf_build_f32(*[0 if k == 7 else a for k, a in enumerate(okr)]) == 0


def test_kernel_nu_is_an_int8_only_argument_of_the_projections():
    from nsgp import ops
    b, M, n, D = 1, 8, 16, 2
    W, Lq = torch.eye(M).expand(b, M, M), torch.eye(M).expand(b, M, M)
    m, s2m1, os_ = torch.zeros(b, M), torch.zeros(b, M), torch.ones(b)
    kin = (torch.zeros(b, M, D), torch.zeros(n, D), torch.ones(b, D), os_)
    W64 = W.double()
    with pytest.raises(ops.BackendError, match="'kzx_fused' projection evaluates Kzx in an RBF-only path"):
        ops.svgp_project(W, None, Lq, m, os_, W64f=W64, kernel_inputs=kin, kernel_nu=1.5)
    with pytest.raises(ops.BackendError, match="'bf16' projection evaluates Kzx in an RBF-only path"):
        ops.svgp_project_bf16(W, None, Lq, m, os_, W64f=W64, kernel_inputs=kin, kernel_nu=1.5)
    for first in ('kzx_fused', 'bf16'):
        with pytest.raises(ops.BackendError, match=f"'{first}' projection evaluates Kzx in an RBF-only path"):
            ops.svgp_project_diag(first, W, s2m1, m, os_, kernel_inputs=kin, W64f=W64, kernel_nu=2.5)
    with pytest.raises(ops.BackendError, match='needs the int8 product'):
        ops.svgp_project(W, torch.zeros(b, M, n), Lq, m, os_, kernel_nu=0.5)
    with pytest.raises(ops.BackendError, match='needs the int8 product'):
        ops.svgp_project_diag('f64acc', W, s2m1, m, os_, Kzx=torch.zeros(b, M, n), W64f=W64, kernel_nu=0.5)
    # a bad nu on the int8 path is matern_build's error; all of these come before the device checks (CPU tensors here)
    with pytest.raises(ops.BackendError, match='nu must be one of'):
        ops.svgp_project(W, None, Lq, m, os_, W64f=W64, i8_inputs=kin, kernel_nu=2.0)
    with pytest.raises(ops.BackendError, match='nu must be one of'):
        ops.svgp_project_diag('i8', W, s2m1, m, os_, kernel_inputs=kin, W64f=W64, kernel_nu=3)
    # without kernel_nu the same calls reach the device check, as they always have
    with pytest.raises(ops.BackendError, match='CUDA'):
        ops.svgp_project(W, None, Lq, m, os_, W64f=W64, kernel_inputs=kin)


@pytest.mark.parametrize('mean_field', [False, True])
def test_bf16_all_refuses_a_matern_layer(mean_field):
    from nsgp import svgp
    from nsgp.gp import settings
    b, M, n, D = 1, 8, 16, 2
    x, Z, ls, os_, m = torch.zeros(n, D), torch.zeros(b, M, D), torch.ones(b, D), torch.ones(b), torch.zeros(b, M)
    q = dict(s2=torch.ones(b, M)) if mean_field else dict(Lq=torch.eye(M).expand(b, M, M))
    W = torch.eye(M).expand(b, M, M).contiguous()
    with settings.forward_precision('bf16_all'):
        with pytest.raises(NotImplementedError, match="bf16_all"):
            svgp.svgp_marginal(x, Z, ls, os_, m, W64=W, nu=1.5, **q)
    with pytest.raises(ValueError, match='nu must be None'):
        svgp.svgp_marginal(x, Z, ls, os_, m, W64=W, nu=2.0, **q)
    with pytest.raises(ValueError, match='one entry per group'):
        svgp.whiten([(Z, ls, os_)], nu=[1.5, None])
    with pytest.raises(ValueError, match='nu must be None'):
        svgp.whiten([(Z, ls, os_)], nu=[1.0])


def test_select_projection_and_the_plan_do_not_know_the_radial_function():
    import inspect
    from nsgp import ops, svgp
    assert list(inspect.signature(svgp.select_projection).parameters) == [
        'dtype', 'M', 'D', 'n', 'kzx_f64', 'has_w64', 'fusable', 'forward_precision', 'whiten_matmul_f64', 'whiten_matmul_i8',
        'fuse_kzx', 'hidden_var_f64', 'diag_q']
    assert list(inspect.signature(ops.svgp_projection_plan.__wrapped__).parameters) == [
        'M', 'n', 'batch', 'dtype', 'first', 'second', 'i8_planes']
    # a Matern layer is never `fusable`: with the defaults it takes the int8 product, four planes / five when it feeds the next
    assert svgp.select_projection(torch.float32, 1024, 2, 4096, False, True, False, 'f32', True, True, True, 'auto')[:3] == \
        ('i8', 'f32', 4)
    assert svgp.select_projection(torch.float32, 1024, 2, 4096, True, True, False, 'f32', True, True, True, 'auto')[:3] == \
        ('i8', 'f64acc_t', 5)
