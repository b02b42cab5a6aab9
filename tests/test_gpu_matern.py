"""MaternKernel (nu = 1/2, 3/2, 5/2) on the MI355X: the batched Matern-ARD build and its backward (csrc/pairwise.hip,
MaternOp) against the float64 restatement of tests/test_matern_cpu.py, and the model paths built on it (exact GP,
inducing-point kernel, composition, the reference's matrix-variate prior demo) against the oracle on in-test matrices.
Tolerances are those of the existing tests of the same kernel family or model path, named at each assert."""
import math
import os

import pytest
import torch

from conftest import measured
from test_matern_cpu import matern_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NUS = (0.5, 1.5, 2.5)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _tol(dt):
    """test_gpu_kernels._tol: the forward builds."""
    return dict(rtol=1e-11, atol=1e-12) if dt == F64 else dict(rtol=2e-5, atol=2e-6)


def _gtol(dt):
    """test_gpu_kernels.test_rbf_fwd_bwd: the backward."""
    return dict(rtol=1e-9, atol=1e-10) if dt == F64 else dict(rtol=2e-3, atol=2e-3)


# (batch, n1, n2, D, x layout): 'flat' = both (n,D); 'mixed' = x1 (b,n1,D), x2 shared (n2,D); 'batched' = both (b,n,D)
CASES = [(1, 316, 78, 2, 'flat'), (1, 1, 1, 1, 'flat'), (1, 5, 700, 3, 'flat'), (1, 130, 257, 5, 'flat'),
         (1, 64, 64, 1, 'flat'), (1, 100, 90, 8, 'flat'), (2, 130, 300, 3, 'mixed'), (2, 130, 300, 3, 'batched')]


def _inputs(b, n1, n2, D, layout, seed):
    g = _g(seed)
    x1 = torch.randn(*((b,) if layout != 'flat' else ()), n1, D, generator=g, dtype=F64)
    x2 = torch.randn(*((b,) if layout == 'batched' else ()), n2, D, generator=g, dtype=F64)
    ls = torch.rand(b, D, generator=g, dtype=F64) + 0.5
    os_ = torch.rand(b, generator=g, dtype=F64) + 0.5
    G = torch.randn(b, n1, n2, generator=g, dtype=F64)
    return x1, x2, ls, os_, G


# ------------------------------------------------------------------------------------------ 1, 2: forward, backward
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('case', CASES, ids=[f'{c[0]}x{c[1]}x{c[2]}xD{c[3]}-{c[4]}' for c in CASES])
def test_matern_fwd_bwd_match_the_restatement(ops, dt, nu, case):
    b, n1, n2, D, layout = case
    x1, x2, ls, os_, G = _inputs(b, n1, n2, D, layout, seed=n1 + 7 * n2 + D)
    x1, x2, ls, os_, G = [t.to(dt).double() for t in (x1, x2, ls, os_, G)]       # the restatement sees the same inputs
    diag_add = 0.0123
    ins = [t.clone().requires_grad_() for t in (x1, x2, ls, os_)]
    ref = matern_ref(*ins, nu) + diag_add * torch.eye(n1, n2, dtype=F64)
    (ref * G).sum().backward()
    cu = [t.to(dt).cuda().requires_grad_() for t in (x1, x2, ls, os_)]
    got = ops.matern_kernel(cu[0], cu[1], cu[2], cu[3], nu, diag_add)
    assert got.shape == (b, n1, n2) and got.dtype == dt
    assert measured(f'matern nu={nu} {dt} fwd {case}', got, ref, **_tol(dt))
    (got * G.to(dt).cuda()).sum().backward()
    for name, a, r in zip(('x1', 'x2', 'ls', 'os'), cu, ins):
        assert a.grad.shape == r.grad.shape
        assert measured(f'matern nu={nu} {dt} grad {name} {case}', a.grad, r.grad, **_gtol(dt))


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_matern_kxx_gradient_takes_zero_at_zero_distance(ops, dt, nu):
    """K(x, x) with a gradient on x: the diagonal (d = 0) contributes nothing -- for nu = 1/2 by the convention of the
    kernel, for 3/2 and 5/2 by the limit; autograd of the restatement (clamp_min) does the same."""
    g = _g(41)
    n, D = 150, 2
    x = torch.randn(n, D, generator=g, dtype=F64).to(dt).double()
    ls = (torch.rand(1, D, generator=g, dtype=F64) + 0.5).to(dt).double()
    os_ = torch.tensor([0.8], dtype=F64).to(dt).double()
    G = torch.randn(1, n, n, generator=g, dtype=F64).to(dt).double()
    xr = x.clone().requires_grad_()
    (matern_ref(xr, xr, ls, os_, nu) * G).sum().backward()
    xc = x.to(dt).cuda().requires_grad_()
    K = ops.matern_kernel(xc, xc, ls.to(dt).cuda(), os_.to(dt).cuda(), nu)
    (K * G.to(dt).cuda()).sum().backward()
    assert bool(torch.isfinite(xc.grad).all())
    assert measured(f'matern nu={nu} {dt} K(x,x) grad x', xc.grad, xr.grad, **_gtol(dt))


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('b,n,D', [(1, 70, 2), (3, 257, 3), (2, 1024, 2)])
def test_matern_backward_symmetric_mode_sums_both_sides(ops, dt, nu, b, n, D):
    """As test_rbf_backward_symmetric_mode_sums_both_sides: one buffer for both x gradients receives g_x1 + g_x2."""
    g = _g(11 + n)
    x = torch.randn(b, n, D, generator=g, dtype=F64).to(dt).cuda()
    ls = (torch.rand(b, D, generator=g, dtype=F64) + 0.5).to(dt).cuda()
    os_ = (torch.rand(b, generator=g, dtype=F64) + 0.5).to(dt).cuda()
    G = torch.randn(b, n, n, generator=g, dtype=F64).to(dt).cuda()
    g1, g2, gls, gos = ops.matern_build_bwd(x, x, ls, os_, nu, G)
    s1, s2, sls, sos = ops.matern_build_bwd(x, x, ls, os_, nu, G, sym=True)
    assert s1 is s2
    tol = dict(rtol=1e-11, atol=1e-11) if dt == F64 else dict(rtol=2e-5, atol=2e-5)
    assert torch.allclose(s1, g1 + g2, **tol)
    assert torch.equal(sls, gls) and torch.equal(sos, gos)


# ------------------------------------------------------------------------------------------ 3: range and NaN
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_matern_distance_range_far_tail_and_nan(ops, dt, nu):
    """As test_gibbs_and_rbf_exponent_range: points on a line whose distances span 1e-3 to 1e3 lengthscales agree with
    the restatement (its tolerances) without NaNs, an entry 1e6 lengthscales away is exactly 0, and a NaN coordinate
    poisons exactly its row and column."""
    n, D = 96, 2
    t = torch.cat([torch.zeros(1, dtype=F64), torch.logspace(-3, 3, n - 1, dtype=F64)])
    x = torch.stack([t, 0.5 * t], -1).to(dt)
    ls = torch.ones(1, D, dtype=dt)
    os_ = torch.ones(1, dtype=dt)
    K = ops.matern_build(x.cuda(), x.cuda(), ls.cuda(), os_.cuda(), nu).cpu().double()[0]
    ref = matern_ref(x.double(), x.double(), ls.double(), os_.double(), nu)[0]
    assert torch.isfinite(K).all()
    tol = dict(rtol=1e-11, atol=1e-300) if dt == F64 else dict(rtol=3e-5, atol=1e-37)
    assert measured(f'matern nu={nu} {dt} distance range', K, ref, **tol)
    far = torch.tensor([[0.0, 0.0], [1e6, 0.0], [0.0, -1e6], [7e5, 7e5]], dtype=dt).cuda()
    Kf = ops.matern_build(far, far, ls.cuda(), os_.cuda(), nu).cpu()[0]
    assert torch.equal(torch.diagonal(Kf), torch.ones(4, dtype=dt))
    off = Kf[~torch.eye(4, dtype=torch.bool)]
    assert not torch.isnan(off).any() and bool((off == 0).all()), Kf
    xn = x.clone()
    xn[7, 0] = float('nan')
    Kn = ops.matern_build(xn.cuda(), xn.cuda(), ls.cuda(), os_.cuda(), nu).cpu()[0]
    assert torch.isnan(Kn[7]).all() and torch.isnan(Kn[:, 7]).all()
    keep = [i for i in range(n) if i != 7]
    assert torch.isfinite(Kn[keep][:, keep]).all()


# ------------------------------------------------------------------------------------------ 4: full size
@pytest.mark.parametrize('dt', [F32, F64])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n', [4096, 16384])
def test_matern_full_size_properties(ops, dt, nu, n):
    g = _g(5 + n)
    x = torch.randn(n, 2, generator=g, dtype=F64).to(dt)
    ls = torch.tensor([[0.5, 0.7]], dtype=dt)
    os_ = torch.tensor([0.8], dtype=dt)
    xc, lsc, osc = x.cuda(), ls.cuda(), os_.cuda()
    K = ops.matern_build(xc, xc, lsc, osc, nu)[0]
    eps = torch.finfo(dt).eps
    dg = torch.diagonal(K)
    assert float((dg - osc).abs().max()) <= 16 * eps * float(os_), float((dg - osc).abs().max())
    asym = float(((K - K.T).abs() - eps * K.abs()).max())
    assert asym <= 0.0, asym                                          # symmetric to 1 ulp
    idx = torch.randint(0, n, (2, 4096), generator=_g(17))
    samp = K[idx[0].cuda(), idx[1].cuda()]
    ref = matern_ref(x.double()[idx[0]].unsqueeze(1), x.double()[idx[1]].unsqueeze(1), ls.double(), os_.double(), nu)
    assert measured(f'matern nu={nu} {dt} N={n} sampled entries', samp, ref.reshape(-1), **_tol(dt))
    del K, dg
    G = torch.randn(n, n, generator=_g(3), dtype=dt).cuda() if n <= 4096 else \
        torch.randn(n, n, dtype=dt, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3))
    first = ops.matern_build_bwd(xc, xc, lsc, osc, nu, G)
    second = ops.matern_build_bwd(xc, xc, lsc, osc, nu, G)
    for a, b in zip(first, second):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------ 5: exact GP
def _uib_whitened(data_dir, dtype):
    import utils.dataprep as dp
    data = dp.download_data(os.path.join(data_dir, 'uib_spatial.csv')).to(dtype)
    x, y, *_ = dp.whitening_transform(data)
    return dp.train_test_split(x, y, 0.8)


def _exact_model(data, dtype, base):
    """test_seard_exact_gp_matches_oracle_and_sklearn_path's set-up around another base kernel."""
    import nsgp.gp as gpytorch
    import models.dgps as m
    trx, try_, tex, tey = data
    likelihood = gpytorch.likelihoods.GaussianLikelihood()
    kernel = gpytorch.kernels.ScaleKernel(base)
    model = m.ExactGPModel(trx, try_, likelihood, kernel).to(dtype).cuda()
    model.likelihood.noise = 0.05
    kernel.outputscale = 0.644
    kernel.base_kernel.lengthscale = torch.tensor([[0.7, 0.9]])
    model.mean_module.constant.data.fill_(0.1)
    return model, likelihood


RAW = ('likelihood.noise_covar.raw_noise', 'mean_module.constant', 'covar_module.raw_outputscale',
       'covar_module.base_kernel.raw_lengthscale')


def _mll_and_grads(model, likelihood):
    import nsgp.gp as gpytorch
    model.train()
    likelihood.train()
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    val = mll(model(model.train_inputs[0]), model.train_targets)
    val.backward()
    params = dict(model.named_parameters())
    assert set(params) == set(RAW), sorted(params)
    return val, {k: params[k].grad.detach().cpu().double().reshape(-1) for k in RAW}


def _raw_cpu(model):
    params = dict(model.named_parameters())
    return {k: params[k].detach().cpu().double().clone().requires_grad_() for k in RAW}


def _hyper(raw):
    sp = torch.nn.functional.softplus
    return (sp(raw[RAW[0]]).reshape(()) + 1e-4, raw[RAW[1]].reshape(()), sp(raw[RAW[2]]).reshape(1),
            sp(raw[RAW[3]]).reshape(1, -1))


def _rel(g32, g64):
    a = torch.cat([g32[k] for k in RAW])
    b = torch.cat([g64[k] for k in RAW])
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize('nu', NUS)
def test_matern_exact_gp_matches_oracle(data_dir, ops, nu):
    import nsgp.gp as gpytorch
    from oracle import exact
    from oracle import kernels as OK
    out = {}
    for dtype in (F64, F32):
        data = _uib_whitened(data_dir, dtype)
        trx, try_, tex, tey = data
        model, likelihood = _exact_model(data, dtype, gpytorch.kernels.MaternKernel(nu=nu, ard_num_dims=2))
        val, grads = _mll_and_grads(model, likelihood)
        raw = _raw_cpu(model)
        noise, c, os_, ls = _hyper(raw)
        xd, yd, xs = trx.double(), try_.double(), tex.double()
        n = len(xd)
        K = matern_ref(xd, xd, ls, os_, nu)[0] + noise * torch.eye(n, dtype=F64)
        ref = exact.mvn_log_prob(yd, c.expand(n), K) / n
        ref.backward()
        rel_mll = abs(float(val) - float(ref)) / abs(float(ref))
        print(f'[measured] matern nu={nu} {dtype} exact-GP MLL rel err {rel_mll:.3g}')
        assert rel_mll < (1e-6 if dtype == F64 else 2e-4)
        ref_grads = {k: raw[k].grad.reshape(-1) for k in RAW}
        if dtype == F64:
            for k in RAW:
                assert measured(f'matern nu={nu} exact-GP grad {k}', grads[k], ref_grads[k], rtol=1e-5, atol=1e-8)
        # RBF-ARD model at the same hyper-parameters and dtype: the accepted float32 gradient error
        rmodel, rlik = _exact_model(data, dtype, gpytorch.kernels.RBFKernel(ard_num_dims=2))
        _, rgrads = _mll_and_grads(rmodel, rlik)
        out[dtype] = (grads, rgrads)
        # posterior
        model.eval()
        likelihood.eval()
        with torch.no_grad():
            pred = likelihood(model(tex.cuda()))
        with torch.no_grad():
            K_sx = matern_ref(xs, xd, ls, os_, nu)[0]
            K_ss = matern_ref(xs, xs, ls, os_, nu)[0]
            L = torch.linalg.cholesky(K)
            alpha = torch.cholesky_solve((yd - c).unsqueeze(-1), L).squeeze(-1)
            m_ref = c + K_sx @ alpha
            V = torch.linalg.solve_triangular(L, K_sx.T, upper=False)
            v_ref = torch.diagonal(K_ss) - (V * V).sum(0) + noise
        rel = float((pred.loc.cpu().double() - m_ref).norm() / m_ref.norm())
        print(f'[measured] matern nu={nu} {dtype} posterior mean rel err {rel:.3g}')
        assert rel < (1e-6 if dtype == F64 else 1e-4), rel
        v = torch.diagonal(pred.covariance_matrix).cpu().double()
        assert measured(f'matern nu={nu} {dtype} predictive variance', v, v_ref,
                        rtol=1e-7 if dtype == F64 else 2e-3, atol=1e-9 if dtype == F64 else 1e-5)
        # five Adam steps lower the loss
        model.train()
        likelihood.train()
        mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        losses = []
        for _ in range(5):
            opt.zero_grad()
            loss = -mll(model(model.train_inputs[0]), model.train_targets)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0], losses
    rel_m = _rel(out[F32][0], out[F64][0])
    rel_r = _rel(out[F32][1], out[F64][1])
    print(f'[measured] nu={nu} float32 gradient |g32 - g64| / |g64|: matern {rel_m:.3g}, rbf {rel_r:.3g} '
          f'(bound 3x rbf = {3 * rel_r:.3g})')
    assert rel_m <= 3 * rel_r, (rel_m, rel_r)


# ------------------------------------------------------------------------------------------ 6: inducing-point kernel
def test_matern_inducing_point_kernel_matches_oracle(data_dir, ops):
    import nsgp.gp as gpytorch
    from sklearn.cluster import KMeans
    from oracle import sparse
    nu = 1.5
    trx, try_, tex, tey = _uib_whitened(data_dir, F64)
    z = torch.tensor(KMeans(60, n_init=2, random_state=0).fit(trx.numpy()).cluster_centers_).double()

    class SparseGP(gpytorch.models.ExactGP):
        def __init__(self, train_x, train_y, likelihood, z):
            super().__init__(train_x, train_y, likelihood)
            self.mean_module = gpytorch.means.ZeroMean()
            base = gpytorch.kernels.ScaleKernel(gpytorch.kernels.MaternKernel(nu=nu, ard_num_dims=2))
            self.covar_module = gpytorch.kernels.InducingPointKernel(base, inducing_points=z, likelihood=likelihood)

        def forward(self, x):
            return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    likelihood = gpytorch.likelihoods.GaussianLikelihood()
    model = SparseGP(trx, try_, likelihood, z).double().cuda()
    likelihood.noise = 0.05
    model.covar_module.base_kernel.outputscale = 0.644
    model.covar_module.base_kernel.base_kernel.lengthscale = torch.tensor([[0.7, 0.9]])
    model.train()
    likelihood.train()
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    val = mll(model(model.train_inputs[0]), model.train_targets)
    val.backward()
    sp = torch.nn.functional.softplus
    noise = float(sp(likelihood.noise_covar.raw_noise.detach().cpu()) + 1e-4)
    os_ = sp(model.covar_module.base_kernel.raw_outputscale.detach().cpu()).reshape(1)
    ls = sp(model.covar_module.base_kernel.base_kernel.raw_lengthscale.detach().cpu()).reshape(1, 2)
    zo = z.clone().requires_grad_()
    xd, yd, xs = trx.double(), try_.double(), tex.double()
    K = lambda a, b: matern_ref(a, b, ls, os_, nu)[0]                     # noqa: E731
    ref = sparse.ipk_mll(K(zo, zo), K(xd, zo), os_.expand(len(xd)), yd, noise)
    ref.backward()
    rel = abs(float(val) - float(ref)) / abs(float(ref))
    print(f'[measured] matern IPK objective rel err {rel:.3g}')
    assert rel < 1e-7
    assert measured('matern IPK inducing-point grad', model.covar_module.inducing_points.grad, zo.grad,
                    rtol=1e-5, atol=1e-8)
    model.eval()
    likelihood.eval()
    with torch.no_grad():
        pred = likelihood(model(tex.cuda()))
        m_ref, c_ref = sparse.ipk_predict(K(z, z), K(xd, z), os_.expand(len(xd)), K(xs, z), os_.expand(len(xs)), yd,
                                          noise)
    rel = float((pred.loc.cpu() - m_ref).norm() / m_ref.norm())
    print(f'[measured] matern IPK posterior mean rel err {rel:.3g}')
    assert rel < 1e-7, rel
    assert measured('matern IPK predictive variance', torch.diagonal(pred.covariance_matrix), torch.diagonal(c_ref),
                    rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------------------------------ 7: composition
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_matern_composes_through_the_generic_kernel_code(ops, dt, nu):
    import nsgp.gp as gpytorch
    from oracle import kernels as OK
    K_ = gpytorch.kernels
    g = _g(77)
    x1 = torch.randn(120, 3, generator=g, dtype=F64).to(dt)
    x2 = torch.randn(90, 3, generator=g, dtype=F64).to(dt)
    a, b = x1.double(), x2.double()
    one = torch.ones(1, dtype=F64)
    # ScaleKernel(Matern) + ScaleKernel(RBF)
    km = K_.ScaleKernel(K_.MaternKernel(nu=nu, ard_num_dims=3))
    kr = K_.ScaleKernel(K_.RBFKernel(ard_num_dims=3))
    km.outputscale, kr.outputscale = 0.7, 1.3
    km.base_kernel.lengthscale = torch.tensor([[0.6, 0.9, 1.2]])
    kr.base_kernel.lengthscale = torch.tensor([[1.1, 0.5, 0.8]])
    ks = (km + kr).to(dt).cuda()
    got = ks(x1.cuda(), x2.cuda()).evaluate()
    val = lambda t: t.detach().cpu().double()                             # noqa: E731  (as set, in dt)
    ref = matern_ref(a, b, val(km.base_kernel.lengthscale).reshape(1, 3), val(km.outputscale).reshape(1), nu)[0] + \
        OK.rbf_ard(a, b, val(kr.base_kernel.lengthscale), val(kr.outputscale))
    assert measured(f'matern nu={nu} {dt} Scale(Matern) + Scale(RBF)', got, ref, **_tol(dt))
    # MaternKernel(active_dims=[0, 1]) * PeriodicKernel(active_dims=[2])
    m = K_.MaternKernel(nu=nu, ard_num_dims=2, active_dims=[0, 1])
    p = K_.PeriodicKernel(active_dims=[2])
    m.lengthscale = torch.tensor([[0.8, 1.1]])
    p.lengthscale = torch.tensor([[0.9]])
    p.period_length = torch.tensor([[1.7]])
    kp = (m * p).to(dt).cuda()
    got = kp(x1.cuda(), x2.cuda()).evaluate()
    ref = matern_ref(a[:, :2], b[:, :2], val(m.lengthscale).reshape(1, 2), one, nu)[0] * \
        OK.periodic(a[:, 2:], b[:, 2:], val(p.lengthscale).reshape(()), val(p.period_length).reshape(()))
    assert measured(f'matern nu={nu} {dt} Matern[0,1] * Periodic[2]', got, ref, **_tol(dt))
    # batch_shape = (3,): shared and batched inputs
    kb = K_.ScaleKernel(K_.MaternKernel(nu=nu, ard_num_dims=2, batch_shape=torch.Size([3])),
                        batch_shape=torch.Size([3]))
    kb.outputscale = torch.tensor([0.5, 1.0, 1.5])
    kb.base_kernel.lengthscale = torch.tensor([[[0.6, 0.9]], [[1.0, 0.7]], [[1.4, 1.2]]])
    kb = kb.to(dt).cuda()
    lsb = kb.base_kernel.lengthscale.detach().cpu().double().reshape(3, 2)
    osb = kb.outputscale.detach().cpu().double()
    got = kb(x1[:, :2].cuda(), x2[:, :2].cuda()).evaluate()
    assert got.shape == (3, 120, 90)
    assert measured(f'matern nu={nu} {dt} batch (3,) shared x', got, matern_ref(a[:, :2], b[:, :2], lsb, osb, nu),
                    **_tol(dt))
    xb1 = torch.randn(3, 50, 2, generator=g, dtype=F64).to(dt)
    xb2 = torch.randn(3, 40, 2, generator=g, dtype=F64).to(dt)
    got = kb(xb1.cuda(), xb2.cuda()).evaluate()
    assert got.shape == (3, 50, 40)
    assert measured(f'matern nu={nu} {dt} batch (3,) batched x', got,
                    matern_ref(xb1.double(), xb2.double(), lsb, osb, nu), **_tol(dt))


# ------------------------------------------------------------------------------------------ 8: the reference demo
def test_matern_matrix_variate_prior_demo(ops):
    """models/latent_priors.py:101-123 of the reference, float64 (kappa of the 900 x 900 row covariance ~ 1.9e6)."""
    import numpy as np
    from nsgp.gp.kernels import MaternKernel
    from models.latent_priors import MatrixVariateNormalPrior
    num_grid = 30
    X = np.linspace(-2, 2, num_grid)
    X_grid = np.meshgrid(X, X)
    X = torch.tensor(np.vstack((X_grid[0].flatten(), X_grid[1].flatten())).T, dtype=F64)
    kern = MaternKernel(nu=2.5, ard_num_dims=2).double().cuda()
    row_covar = kern(X.cuda()).evaluate()
    assert row_covar.shape == (900, 900)
    ls = kern.lengthscale.detach().cpu().reshape(1, 2)
    ref = matern_ref(X, X, ls, torch.ones(1, dtype=F64), 2.5)[0]
    assert measured('matern demo row covariance', row_covar, ref, **_tol(F64))
    loc = torch.zeros(900, 2, dtype=F64).cuda()
    col_covar = torch.eye(2, dtype=F64).cuda()
    prior = MatrixVariateNormalPrior(loc, row_covariance_matrix=row_covar, column_covariance_matrix=col_covar)
    s = prior.sample_n(1)
    assert s.shape == (900, 2) and bool(torch.isfinite(s).all())
    lp = prior.log_prob(s)
    assert bool(torch.isfinite(lp).all())


# ------------------------------------------------------------------------------------------ 9: guard
def test_variational_strategy_still_refuses_a_matern_kernel(ops):
    import nsgp.gp as gpytorch
    from nsgp.gp.variational import VariationalStrategy, CholeskyVariationalDistribution

    class Layer(gpytorch.models.ApproximateGP):
        def __init__(self, z):
            vd = CholeskyVariationalDistribution(z.shape[-2])
            super().__init__(VariationalStrategy(self, z, vd, learn_inducing_locations=True))
            self.mean_module = gpytorch.means.ConstantMean()
            self.covar_module = gpytorch.kernels.ScaleKernel(gpytorch.kernels.MaternKernel(nu=2.5, ard_num_dims=2))

        def forward(self, x):
            return gpytorch.distributions.MultivariateNormal(self.mean_module(x), self.covar_module(x))

    z = torch.randn(16, 2, generator=_g(9))
    layer = Layer(z).cuda()
    with pytest.raises(NotImplementedError):
        layer(torch.randn(32, 2, generator=_g(10)).cuda())
