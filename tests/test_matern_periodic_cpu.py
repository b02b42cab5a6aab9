"""MaternKernel * PeriodicKernel (the temporal kernel with a roughness parameter) without a GPU: the float64 restatement
the GPU tests compare against, the C ABI of the fused build, and the host logic that routes the kernel pair, the ops and the
spatio-temporal models to it.

`matern_periodic_ref` restates (imported by tests/test_gpu_matern_periodic.py), with delta = x1 - x2, u_d = delta_d / l_d,
s = sum_d u_d^2, r = |delta|, theta = pi r / p:

    k = os kappa_nu(s) E,   E = exp(-2 sin^2(theta) / l_p),
    kappa_1/2 = e^-d,  kappa_3/2 = (1 + sqrt3 d) e^-sqrt3 d,  kappa_5/2 = (1 + sqrt5 d + 5/3 s) e^-sqrt5 d,

with d = clamp_min(s, 1e-30).sqrt() (and r likewise), so that autograd takes the derivative at zero distance as 0, the
device kernel's convention."""
import ctypes
import math

import pytest
import torch

F64 = torch.float64
NUS = (0.5, 1.5, 2.5)


def matern_periodic_ref(x1, x2, ls_env, ls_per, period, os_, nu):
    """x1:(n1,D) or (b,n1,D), x2 likewise, ls_env:(b,D), ls_per, period:(b,), os_:(b,) or None -> (b,n1,n2)."""
    delta = x1.unsqueeze(-2) - x2.unsqueeze(-3)
    u = delta / ls_env[:, None, None, :]
    s = (u * u).sum(-1)
    d = s.clamp_min(1e-30).sqrt()
    if nu == 0.5:
        kap = torch.exp(-d)
    elif nu == 1.5:
        a = math.sqrt(3.0)
        kap = (1 + a * d) * torch.exp(-a * d)
    elif nu == 2.5:
        a = math.sqrt(5.0)
        kap = (1 + a * d + (5.0 / 3.0) * s) * torch.exp(-a * d)
    else:
        raise ValueError(nu)
    r = (delta * delta).sum(-1).clamp_min(1e-30).sqrt()
    theta = math.pi * r / period[:, None, None]
    k = kap * torch.exp(-2.0 * torch.sin(theta).pow(2) / ls_per[:, None, None])
    k = k + torch.zeros(ls_per.shape[0], 1, 1, dtype=k.dtype)              # (b, n1, n2) also for shared x
    return k if os_ is None else os_[:, None, None] * k


def _scalar_entry(x1, x2, le, lp, p, os_, nu):
    """One entry and its closed-form derivatives, written from the formulae (plain Python floats).
    Returns k, dk/dx1 (list), dk/dle (list), dk/dlp, dk/dp, dk/dos."""
    D = len(x1)
    delta = [a - b for a, b in zip(x1, x2)]
    u = [dl / l for dl, l in zip(delta, le)]
    s = sum(v * v for v in u)
    d = math.sqrt(s)
    r = math.sqrt(sum(v * v for v in delta))
    if nu == 0.5:
        kap = math.exp(-d)
        phi = 0.0 if d == 0.0 else -math.exp(-d) / d
    elif nu == 1.5:
        a = math.sqrt(3.0)
        kap = (1 + a * d) * math.exp(-a * d)
        phi = -3.0 * math.exp(-a * d)
    else:
        a = math.sqrt(5.0)
        kap = (1 + a * d + 5.0 / 3.0 * s) * math.exp(-a * d)
        phi = -5.0 / 3.0 * (1 + a * d) * math.exp(-a * d)
    th = math.pi * r / p
    sn, cs = math.sin(th), math.cos(th)
    E = math.exp(-2.0 * sn * sn / lp)
    k = os_ * kap * E
    c = 4.0 / lp * sn * cs * math.pi
    gx = [os_ * E * phi * u[i] / le[i] - (k * (c / p) * delta[i] / r if r > 0 else 0.0) for i in range(D)]
    gle = [-os_ * E * phi * u[i] * u[i] / le[i] for i in range(D)]
    return k, gx, gle, k * 2.0 * sn * sn / (lp * lp), k * c * r / (p * p), kap * E


@pytest.mark.parametrize('nu', NUS)
def test_restatement_matches_the_scalar_formulae_and_their_closed_form_gradients(nu):
    g = torch.Generator().manual_seed(11)
    D = 2
    x1 = torch.randn(4, D, generator=g, dtype=F64)
    x2 = torch.cat([torch.randn(3, D, generator=g, dtype=F64), x1[1:2], 30.0 + x1[:1]])      # a zero and a far distance
    le = torch.rand(1, D, generator=g, dtype=F64) + 0.6
    lp, pe, os_ = torch.tensor([0.9], dtype=F64), torch.tensor([1.3], dtype=F64), torch.tensor([1.7], dtype=F64)
    leaves = [t.clone().requires_grad_() for t in (x1, x2, le, lp, pe, os_)]
    K = matern_periodic_ref(*leaves, nu)
    assert K.shape == (1, 4, 5)
    for i in range(4):
        for j in range(5):
            for t in leaves:
                t.grad = None
            K[0, i, j].backward(retain_graph=True)
            k, gx, gle, glp, gp, gos = _scalar_entry(x1[i].tolist(), x2[j].tolist(), le[0].tolist(), 0.9, 1.3, 1.7, nu)
            close = lambda got, want: abs(float(got) - want) <= 1e-13 + 1e-11 * abs(want)   # noqa: E731
            assert close(K[0, i, j], k), (i, j)
            a1, a2, ale, alp, ape, aos = (t.grad for t in leaves)
            for dd in range(D):
                assert close(a1[i, dd], gx[dd]) and close(a2[j, dd], -gx[dd]), (i, j, dd)
                assert close(ale[0, dd], gle[dd]), (i, j, dd)
            assert close(alp[0], glp) and close(ape[0], gp) and close(aos[0], gos), (i, j)
    # zero distance: k = os, and nothing but d/d os is non-zero, for every nu
    for t in leaves:
        t.grad = None
    K[0, 1, 3].backward()
    assert abs(float(K[0, 1, 3]) - 1.7) < 1e-14                      # the clamp: d = 1e-15, not 0
    assert all(float(t.grad.abs().max()) < 1e-25 for t in leaves[:5]) and abs(float(leaves[5].grad) - 1.0) < 1e-14


def test_header_declares_and_library_exports_the_matern_periodic_entry_points():
    import nsgp
    names = nsgp.declared_symbols()
    want = [f'nsgp_matern_periodic_build_{d}_{s}' for d in ('fwd', 'bwd') for s in ('f32', 'f64')]
    for name in want:
        assert name in names, name
    assert 'nsgp_matern_periodic_build_bwd_workspace' not in names           # the rbf_periodic query serves both
    lib = nsgp.load_library()
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for name in want:
        assert hasattr(raw, name), name
    assert lib.nsgp_abi_version() == 2


def test_matern_periodic_entry_points_validate_their_arguments_on_the_host():
    """Bad arguments return the negative 1-based index of the offending one in this entry point's own signature before
    any launch; empty problems return 0 without a launch.  Safe without a GPU: no call below reaches the device."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    #         x1 x2 ls_env ls_per period os batch n1 n2 D sx1 sx2 nu2 diag_add K ldk sK stream
    fwd_ok = [b, b, b, b, b, b, 1, 4, 4, 2, 0, 0, 5, 0.0, b, 4, 16, None]
    #         x1 x2 ls_env ls_per period os batch n1 n2 D sx1 sx2 nu2 G ldg sG g_x1 g_x2 g_le g_lp g_pe g_os ws ws_bytes stream
    bwd_ok = [b, b, b, b, b, b, 1, 4, 4, 2, 0, 0, 3, b, 4, 16, b, b, b, b, b, b, b, 512, None]
    for sfx in ('f32', 'f64'):
        fwd = getattr(lib, f'nsgp_matern_periodic_build_fwd_{sfx}')
        bwd = getattr(lib, f'nsgp_matern_periodic_build_bwd_{sfx}')
        bad_f = lambda i, v: fwd(*[v if k == i else a for k, a in enumerate(fwd_ok)])      # noqa: E731
        bad_b = lambda i, v: bwd(*[v if k == i else a for k, a in enumerate(bwd_ok)])      # noqa: E731
        for bad in (bad_f, bad_b):
            assert bad(0, None) == -1 and bad(1, None) == -2
            assert bad(2, None) == -3                                    # ls_env is required here
            assert bad(3, None) == -4 and bad(4, None) == -5
            assert bad(6, -1) == -7 and bad(7, -1) == -8 and bad(8, -1) == -9
            assert bad(9, 0) == -10 and bad(9, 9) == -10 and bad(9, -3) == -10
            for nu2 in (0, 2, 4, 6, -1, 7, 25):
                assert bad(12, nu2) == -13, nu2
        assert bad_f(14, None) == -15 and bad_f(15, 3) == -16
        assert bad_b(13, None) == -14 and bad_b(14, 3) == -15
        # os == NULL means 1: not an error (nothing to do, so no launch)
        assert fwd(*[None if k == 5 else (0 if k == 7 else a) for k, a in enumerate(fwd_ok)]) == 0
        # empty problems: no launch, success
        assert bad_f(6, 0) == 0 and bad_f(7, 0) == 0 and bad_f(8, 0) == 0
        assert bad_b(6, 0) == 0 and bad_b(7, 0) == 0 and bad_b(8, 0) == 0


def test_product_kernel_recognises_the_matern_periodic_pair():
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, RBFKernel
    for nu in NUS:
        m, p = MaternKernel(nu=nu, active_dims=(0)), PeriodicKernel(active_dims=(0))
        for prod in (m * p, p * m):
            assert prod.fuses_outputscale
            env, per = prod._rbf_periodic()
            assert env is m and per is p
    assert (MaternKernel(nu=1.5) * PeriodicKernel()).fuses_outputscale                  # no active_dims on either
    assert not (MaternKernel(nu=1.5, active_dims=(0)) * PeriodicKernel(active_dims=(1))).fuses_outputscale
    assert not (MaternKernel(nu=1.5, active_dims=(0)) * PeriodicKernel()).fuses_outputscale
    assert not (MaternKernel(nu=1.5) * PeriodicKernel() * RBFKernel()).fuses_outputscale
    # the RBF pair still resolves to the RBF envelope
    r, p = RBFKernel(active_dims=(0)), PeriodicKernel(active_dims=(0))
    for prod in (r * p, p * r):
        env, per = prod._rbf_periodic()
        assert env is r and per is p and prod.fuses_outputscale


def test_ops_fail_loudly_on_cpu_tensors_and_on_other_nu():
    from nsgp import ops, BackendError
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, ScaleKernel
    x = torch.randn(5, 1)
    le, lp, pe, os_ = torch.ones(1, 1), torch.ones(1), torch.ones(1), torch.ones(1)
    for nu in NUS:
        with pytest.raises(BackendError):
            ops.matern_periodic_build(x, x, le, lp, pe, os_, nu)
        with pytest.raises(BackendError):
            ops.matern_periodic_kernel(x, x, le, lp, pe, os_, nu)
        with pytest.raises(BackendError):
            ops.matern_periodic_build_bwd(x, x, le, lp, pe, os_, nu, torch.ones(1, 5, 5))
        with pytest.raises(BackendError):
            ScaleKernel(MaternKernel(nu=nu) * PeriodicKernel())(x).evaluate()
    for call in (lambda: ops.matern_periodic_kernel(x, x, le, lp, pe, os_, 1.0),
                 lambda: ops.matern_periodic_build(x, x, le, lp, pe, os_, 1.0),
                 lambda: ops.matern_periodic_build_bwd(x, x, le, lp, pe, os_, 2.0, torch.ones(1, 5, 5))):
        with pytest.raises(RuntimeError, match='nu must be one of'):
            call()
    with pytest.raises(BackendError, match='ls_env is required'):
        ops.matern_periodic_build(x, x, None, lp, pe, os_, 1.5)
    import inspect
    sig = inspect.signature(ops.matern_periodic_kernel)
    assert list(sig.parameters) == ['x1', 'x2', 'ls_env', 'ls_per', 'period', 'os_', 'nu', 'diag_add']
    assert sig.parameters['os_'].default is None and sig.parameters['nu'].default == 2.5
    assert sig.parameters['diag_add'].default == 0.0


def _st_models(temporal_nu):
    import nsgp.gp as gpytorch
    from models.gibbs_kernels import LogNormalPriorProcess
    from models.spatio_temporal_models import SparseSpatioTemporal_Nonstationary, SpatioTemporal_Stationary
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(12, 3, generator=g), torch.randn(12, generator=g)
    z = x[::3].clone()
    kw = {} if temporal_nu == 'absent' else dict(temporal_nu=temporal_nu)
    stat = SpatioTemporal_Stationary(x, y, gpytorch.likelihoods.GaussianLikelihood(), **kw)
    prior = LogNormalPriorProcess(input_dim=2, active_dims=(0, 1))
    sparse = SparseSpatioTemporal_Nonstationary(x, y, gpytorch.likelihoods.GaussianLikelihood(), prior, z, num_dim=2, **kw)
    return stat, sparse


def test_models_take_temporal_nu_and_keep_their_state_dict_keys():
    from models.spatio_temporal_models import _temporal_kernel
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, RBFKernel
    absent, none, rough = _st_models('absent'), _st_models(None), _st_models(1.5)
    for a, n, r in zip(absent, none, rough):
        assert list(a.state_dict()) == list(n.state_dict())
        assert set(n.state_dict()) == set(r.state_dict())
        for (ka, va), (kn, vn) in zip(a.state_dict().items(), n.state_dict().items()):
            assert va.shape == vn.shape and va.dtype == vn.dtype, ka
        for k, v in n.state_dict().items():
            assert r.state_dict()[k].shape == v.shape, k
    for m in none:
        tk = m.temporal_covar_module
        tk = getattr(tk, 'base_kernel') if not hasattr(tk, 'raw_outputscale') else tk
        assert type(tk.base_kernel.kernels[0]) is RBFKernel
    for m in rough:
        tk = m.temporal_covar_module
        tk = getattr(tk, 'base_kernel') if not hasattr(tk, 'raw_outputscale') else tk
        env, per = tk.base_kernel.kernels
        assert type(env) is MaternKernel and env.nu == 1.5 and type(per) is PeriodicKernel
        assert tk.base_kernel.fuses_outputscale
    for bad in (1.0, 2.0, 0.0):
        with pytest.raises(RuntimeError):
            _st_models(bad)
        with pytest.raises(RuntimeError):
            _temporal_kernel(bad)
    k = _temporal_kernel()
    assert type(k.base_kernel.kernels[0]) is RBFKernel and float(k.outputscale) > 7
    assert float(_temporal_kernel(0.5).outputscale) > 7
