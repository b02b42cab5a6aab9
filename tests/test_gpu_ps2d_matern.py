"""MultivariateGibbsKernel(nu = 1/2, 3/2, 5/2) on the MI355X: the Paciorek-Schervish build with the Matern radial function
and its backward (csrc/pairwise.hip, PsRadialOp) against the float64 restatement of tests/test_ps2d_matern_cpu.py, and the
kernel classes built on it against the oracle, which reaches its kernel through the attribute oracle.kernels.ps2d and so
serves unchanged with that attribute pointed at the restatement.  Tolerances are those of the existing tests of the same
code (test_gpu_matern._tol for the forward, test_ps2d_fwd_bwd's for the gradients) or of the same model path
(test_gpu_models), named at each assert, with the float32 ones of the forward and backward tightened to ~3x the error
measured (_ftol, _btol; the measured values: profiles/ps2d_matern/errors.txt); inputs are rounded to the dtype before the
restatement sees them."""
import math

import pytest
import torch

from conftest import measured
from test_gpu_matern import _tol
from test_ps2d_matern_cpu import ps2d_matern_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
NUS = (0.5, 1.5, 2.5)
DMAT = [[0.7, 0.1], [-0.2, 0.9]]


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _ftol(dt):
    """The forward: test_gpu_matern._tol.  Float32: see FTOL32 below."""
    return _tol(dt) if dt == F64 else FTOL32


def _btol(dt):
    """The Sigma-gradients: test_ps2d_fwd_bwd's.  Float32: see BTOL32 below."""
    return dict(rtol=1e-9, atol=1e-10) if dt == F64 else BTOL32


# float32 bounds, ~3x the worst error this kernel showed on the MI355X under the starting bounds (the project's rule):
# forward, test_gpu_matern._tol (rtol 2e-5, atol 2e-6): worst diff / (atol + rtol |ref|) = 0.047 ((130, 129), nu = 5/2;
# 0.046 in the 1000 x 3850 case); gradients, test_ps2d_fwd_bwd's rtol = atol = 3e-3: worst 0.00096 (sigma2 of the 1000 x 3850 case, sums
# of 1000 terms; 0.0005 elsewhere)
FTOL32 = dict(rtol=3e-6, atol=3e-7)
BTOL32 = dict(rtol=9e-6, atol=9e-6)


def _inputs(n1, n2, dt, seed):
    """x ~ U[0, 1]^2, Sigma = ps_sigma(H, D) with H ~ N(0, 1) and the unsymmetric D of test_ps2d_fwd_bwd (determinants
    >= 1.2, a1 != a2), G ~ N(0, 1), all rounded to dt and returned in float64."""
    from oracle import kernels as K
    g = _g(seed)
    x1 = torch.rand(n1, 2, generator=g, dtype=F64)
    x2 = torch.rand(n2, 2, generator=g, dtype=F64)
    H1, H2 = torch.randn(n1, 2, generator=g, dtype=F64), torch.randn(n2, 2, generator=g, dtype=F64)
    Dm = torch.tensor(DMAT, dtype=F64)
    G = torch.randn(n1, n2, generator=g, dtype=F64)
    return [t.to(dt).double() for t in (x1, x2, K.ps_sigma(H1, Dm), K.ps_sigma(H2, Dm), G)]


_REF = {}


def _reference(n1, n2, dt, nu, jitter, seed):
    """(inputs, K, g_s1, g_s2) of the restatement, computed once per case and left unchanged."""
    key = (n1, n2, dt, nu, jitter, seed)
    if key not in _REF:
        x1, x2, s1, s2, G = _inputs(n1, n2, dt, seed)
        r1, r2 = s1.clone().requires_grad_(), s2.clone().requires_grad_()
        ref = ps2d_matern_ref(x1, x2, r1, r2, jitter, nu)
        (ref * G).sum().backward()
        _REF[key] = ((x1, x2, s1, s2, G), ref.detach(), r1.grad, r2.grad)
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1: forward and gradients
# the forward tile's 64 x 256 (float32) / 64 x 128 (float64) edges and the backward's 64 x 256 ones; (1000, 3850) is the
# smallest ragged shape whose backward takes the 64-row kernel (16 x 16 = 256 workgroups)
SHAPES = [(1, 1), (63, 255), (64, 256), (65, 257), (130, 129), (5, 700)]
BIG = (1000, 3850)
CASES = ([(s, nu, dt, 1e-5) for s in SHAPES for nu in NUS for dt in (F64, F32)] +
         [((65, 257), nu, dt, 0.0) for nu in NUS for dt in (F64, F32)] +
         [(BIG, 1.5, F64, 1e-5), (BIG, 1.5, F32, 1e-5)])


@pytest.mark.parametrize('shape,nu,dt,jitter', CASES,
                         ids=[f'{s[0]}x{s[1]}-nu{nu}-{str(dt)[6:]}-jit{j:g}' for s, nu, dt, j in CASES])
def test_ps2d_matern_fwd_bwd_match_the_restatement(ops, shape, nu, dt, jitter):
    n1, n2 = shape
    (x1, x2, s1, s2, G), ref, g1, g2 = _reference(n1, n2, dt, nu, jitter, seed=n1 + 7 * n2)
    assert float(torch.det(s1).min()) >= 1.2 and float((s1[:, 0, 1] - s1[:, 1, 0]).abs().min()) > 0
    if shape == BIG:
        assert ops.pairwise_bwd_plan(1, n1, n2).rows == 64
    else:
        assert ops.pairwise_bwd_plan(1, n1, n2).rows == 16
    c1, c2 = s1.to(dt).cuda().requires_grad_(), s2.to(dt).cuda().requires_grad_()
    got = ops.ps2d_kernel(x1.to(dt).cuda(), x2.to(dt).cuda(), c1, c2, jitter, nu=nu)
    assert got.shape == (n1, n2) and got.dtype == dt
    assert measured(f'ps2d-matern nu={nu} {dt} jit={jitter:g} fwd {shape}', got, ref, **_ftol(dt))
    (got * G.to(dt).cuda()).sum().backward()
    for name, a, r in (('sigma1', c1, g1), ('sigma2', c2, g2)):
        assert a.grad.shape == r.shape
        assert measured(f'ps2d-matern nu={nu} {dt} jit={jitter:g} grad {name} {shape}', a.grad, r, **_btol(dt))


# ------------------------------------------------------------------------------------------ 2: K(x, x)
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n', [70, 257])
def test_ps2d_matern_kxx_one_tensor_in_both_roles(ops, dt, nu, n):
    """K(x, x) with ONE tensor as sigma1 and sigma2: autograd sums both roles; the diagonal is 1; the diagonal entries
    (zero distance, equal Sigma) contribute exactly nothing to the Sigma-gradient -- for nu = 1/2 by the phi(0) = 0
    convention -- so another diagonal of G leaves it bit-equal."""
    x, _, s, _, G = _inputs(n, n, dt, seed=41 + n)
    sr = s.clone().requires_grad_()
    ref = ps2d_matern_ref(x, x, sr, sr, 1e-5, nu)
    (ref * G).sum().backward()
    xc, sc, Gc = x.to(dt).cuda(), s.to(dt).cuda().requires_grad_(), G.to(dt).cuda()
    K = ops.ps2d_kernel(xc, xc, sc, sc, 1e-5, nu=nu)
    assert measured(f'ps2d-matern nu={nu} {dt} K(x,x) n={n}', K, ref, **_ftol(dt))
    assert measured(f'ps2d-matern nu={nu} {dt} K(x,x) diagonal n={n}', torch.diagonal(K), torch.ones(n, dtype=F64),
                    **_ftol(dt))
    (K * Gc).sum().backward()
    assert bool(torch.isfinite(sc.grad).all())
    assert measured(f'ps2d-matern nu={nu} {dt} K(x,x) grad sigma n={n}', sc.grad, sr.grad, **_btol(dt))
    # the diagonal contributes nothing
    G2 = Gc + torch.diag(torch.randn(n, generator=_g(5), dtype=F64).to(dt).cuda())
    assert not torch.equal(G2, Gc)
    sd = sc.detach()
    a = ops.ps2d_build_bwd(xc, xc, sd, sd, 1e-5, Gc, nu=nu)
    b = ops.ps2d_build_bwd(xc, xc, sd, sd, 1e-5, G2, nu=nu)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(a[0] + a[1], sc.grad)


# ------------------------------------------------------------------------------------------ 3: coincident points
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_ps2d_matern_coincident_points_across_two_tensors(ops, dt, nu):
    """x2[:5] = x1[:5] with different Sigma on the two sides: zero distance without equal operands.  Values and gradients
    are finite and match (nu = 1/2: the derivative at zero distance is taken as 0 on both sides)."""
    n1, n2 = 40, 33
    x1, x2, s1, s2, G = _inputs(n1, n2, dt, seed=77)
    x2 = x2.clone()
    x2[:5] = x1[:5]
    r1, r2 = s1.clone().requires_grad_(), s2.clone().requires_grad_()
    ref = ps2d_matern_ref(x1, x2, r1, r2, 1e-5, nu)
    (ref * G).sum().backward()
    c1, c2 = s1.to(dt).cuda().requires_grad_(), s2.to(dt).cuda().requires_grad_()
    got = ops.ps2d_kernel(x1.to(dt).cuda(), x2.to(dt).cuda(), c1, c2, 1e-5, nu=nu)
    (got * G.to(dt).cuda()).sum().backward()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(c1.grad).all()) and bool(torch.isfinite(c2.grad).all())
    assert measured(f'ps2d-matern nu={nu} {dt} coincident fwd', got, ref, **_ftol(dt))
    assert measured(f'ps2d-matern nu={nu} {dt} coincident grad sigma1', c1.grad, r1.grad, **_btol(dt))
    assert measured(f'ps2d-matern nu={nu} {dt} coincident grad sigma2', c2.grad, r2.grad, **_btol(dt))
    # the coincident entries alone (G zero elsewhere)
    Gz = torch.zeros_like(G)
    Gz[:5, :5] = torch.diag(torch.diagonal(G[:5, :5]))
    r1.grad, r2.grad = None, None
    (ps2d_matern_ref(x1, x2, r1, r2, 1e-5, nu) * Gz).sum().backward()
    g1, g2 = ops.ps2d_build_bwd(x1.to(dt).cuda(), x2.to(dt).cuda(), c1.detach(), c2.detach(), 1e-5, Gz.to(dt).cuda(), nu=nu)
    assert measured(f'ps2d-matern nu={nu} {dt} coincident entries only, grad sigma1', g1, r1.grad, **_btol(dt))
    assert measured(f'ps2d-matern nu={nu} {dt} coincident entries only, grad sigma2', g2, r2.grad, **_btol(dt))


# ------------------------------------------------------------------------------------------ 4: diagonal limit
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_ps2d_matern_with_diagonal_sigma_is_the_gibbs_matern_build(ops, dt, nu):
    """Sigma = diag(2 ell^2), jitter = 0: GibbsKernel(nu)'s own device build."""
    n1, n2 = 130, 257
    g = _g(23)
    x1 = torch.randn(n1, 2, generator=g, dtype=F64).to(dt).cuda()
    x2 = torch.randn(n2, 2, generator=g, dtype=F64).to(dt).cuda()
    e1 = (torch.rand(2, n1, generator=g, dtype=F64) + 0.5).to(dt).cuda()
    e2 = (torch.rand(2, n2, generator=g, dtype=F64) + 0.5).to(dt).cuda()
    got = ops.ps2d_build(x1, x2, torch.diag_embed(2 * e1.T ** 2), torch.diag_embed(2 * e2.T ** 2), 0.0, nu=nu)
    ref = ops.gibbs_kernel(x1, x2, e1, e2, nu=nu)
    assert measured(f'ps2d-matern nu={nu} {dt} diagonal limit vs gibbs_kernel', got, ref, **_ftol(dt))


# ------------------------------------------------------------------------------------------ 5: edge values
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_ps2d_matern_negative_quadratic_form_gives_the_prefactor(ops, dt, nu):
    """Sigma negative definite (unsymmetric, det Sigma > 0 and det A > 0, so the prefactor P is real): Q < 0 for every
    pair of distinct points.  The op evaluates kappa at s = 0, so k = P exactly -- the value at zero distance, which
    does not depend on x -- and the distance term of the gradient is dropped."""
    n1, n2 = 9, 7
    g = _g(91)
    x1 = torch.rand(n1, 2, generator=g, dtype=F64).to(dt)
    x2 = torch.rand(n2, 2, generator=g, dtype=F64).to(dt)
    base = torch.tensor([[-1.5, 0.3], [0.2, -1.1]], dtype=F64)
    s1 = (base + 0.1 * torch.rand(n1, 2, 2, generator=g, dtype=F64)).to(dt)
    s2 = (base + 0.1 * torch.rand(n2, 2, 2, generator=g, dtype=F64)).to(dt)
    A = 0.5 * (s1.double()[:, None] + s2.double()[None, :])
    assert float(torch.det(s1.double()).min()) > 0 and float(torch.det(s2.double()).min()) > 0
    assert float(torch.det(A).min()) > 0
    d = (x1.double()[:, None, :] - x2.double()[None, :, :])
    Q = (d.unsqueeze(-2) @ torch.inverse(A + 1e-5 * torch.eye(2, dtype=F64)) @ d.unsqueeze(-1)).reshape(n1, n2)
    assert float(Q.max()) < 0
    x1c, x2c, s1c, s2c = x1.cuda(), x2.cuda(), s1.cuda(), s2.cuda()
    K = ops.ps2d_build(x1c, x2c, s1c, s2c, 1e-5, nu=nu)
    zero = torch.zeros_like(x1c), torch.zeros_like(x2c)
    P = ops.ps2d_build(*zero, s1c, s2c, 1e-5, nu=nu)
    assert torch.equal(K, P)
    Pref = ps2d_matern_ref(torch.zeros(n1, 2, dtype=F64), torch.zeros(n2, 2, dtype=F64), s1.double(), s2.double(), 1e-5, nu)
    assert measured(f'ps2d-matern nu={nu} {dt} Q < 0: k = P', K, Pref, **_ftol(dt))
    G = torch.randn(n1, n2, generator=g, dtype=F64).to(dt).cuda()
    for a, b in zip(ops.ps2d_build_bwd(x1c, x2c, s1c, s2c, 1e-5, G, nu=nu),
                    ops.ps2d_build_bwd(*zero, s1c, s2c, 1e-5, G, nu=nu)):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('nu', NUS)
def test_ps2d_matern_nan_poisons_its_row_or_column_only(ops, dt, nu):
    n1, n2 = 70, 130
    x1, x2, s1, s2, _ = _inputs(n1, n2, dt, seed=19)
    x1, x2, s1, s2 = [t.to(dt).cuda() for t in (x1, x2, s1, s2)]
    rows = [i for i in range(n1) if i != 7]
    cols = [j for j in range(n2) if j != 66]
    xn, sn = x1.clone(), s1.clone()
    xn[7, 1] = float('nan')
    sn[7, 0, 1] = float('nan')
    for what, xa, sa in (('x1', xn, s1), ('sigma1', x1, sn)):
        K = ops.ps2d_build(xa, x2, sa, s2, 1e-5, nu=nu)
        assert bool(torch.isnan(K[7]).all()), what
        assert bool(torch.isfinite(K[rows]).all()), what
    xn, sn = x2.clone(), s2.clone()
    xn[66, 0] = float('nan')
    sn[66, 1, 1] = float('nan')
    for what, xa, sa in (('x2', xn, s2), ('sigma2', x2, sn)):
        K = ops.ps2d_build(x1, xa, s1, sa, 1e-5, nu=nu)
        assert bool(torch.isnan(K[:, 66]).all()), what
        assert bool(torch.isfinite(K[:, cols]).all()), what


# ------------------------------------------------------------------------------------------ 6: nu = None
@pytest.mark.parametrize('dt', [F64, F32])
def test_nu_none_is_the_ps2d_kernel_of_before(ops, dt):
    n1, n2 = 130, 300
    x1, x2, s1, s2, G = _inputs(n1, n2, dt, seed=61)
    x1c, x2c, Gc = x1.to(dt).cuda(), x2.to(dt).cuda(), G.to(dt).cuda()
    out = []
    for kw in ({}, {'nu': None}):
        c1, c2 = s1.to(dt).cuda().requires_grad_(), s2.to(dt).cuda().requires_grad_()
        K = ops.ps2d_kernel(x1c, x2c, c1, c2, 1e-5, **kw)
        (K * Gc).sum().backward()
        out.append((K.detach(), c1.grad, c2.grad))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    # ... which is the library's squared-exponential entry point, and not the Matern kernel
    from oracle import kernels as OK
    assert measured(f'ps2d nu=None {dt} vs oracle.kernels.ps2d', out[0][0], OK.ps2d(x1, x2, s1, s2, 1e-5), **_tol(dt))
    assert not torch.equal(out[0][0], ops.ps2d_kernel(x1c, x2c, c1.detach(), c2.detach(), 1e-5, nu=2.5))
    assert torch.equal(ops.ps2d_build(x1c, x2c, c1.detach(), c2.detach(), nu=None),
                       ops.ps2d_build(x1c, x2c, c1.detach(), c2.detach()))
    for u, v in zip(ops.ps2d_build_bwd(x1c, x2c, c1.detach(), c2.detach(), 1e-5, Gc, nu=None),
                    ops.ps2d_build_bwd(x1c, x2c, c1.detach(), c2.detach(), 1e-5, Gc)):
        assert torch.equal(u, v)


# ------------------------------------------------------------------------------------------ 7: the kernel classes
def _oracle_with(monkeypatch, nu):
    """Point the oracle's Paciorek-Schervish kernel at the restatement for nu (undone by monkeypatch after the test)."""
    import oracle.kernels
    monkeypatch.setattr(oracle.kernels, 'ps2d',
                        lambda x1, x2, s1, s2, jitter=1e-5: ps2d_matern_ref(x1, x2, s1, s2, jitter, nu))


def test_multivariate_gibbs_kernels_with_nu_match_the_oracle(data_dir, ops, monkeypatch):
    """test_multivariate_gibbs_kernels_match_oracle (its scenario and bounds) with nu = 3/2 on the dense kernel and
    nu = 1/2 on the sparse one; both classes store nu and default to None."""
    from models.multivariate_gibbs_kernel import MultivariateGibbsKernel
    from models.sparse_multivariate_gibbs_kernel import SparseMultivariateGibbsKernel
    from oracle import psgibbs
    from test_gpu_models import KN_TOL, KSX_TOL, _uib_spatial
    xtr, ytr, xte, yte = _uib_spatial(data_dir)
    x, xs = xtr[:200].float().cuda(), xte[:50].float().cuda()
    assert MultivariateGibbsKernel(x, 2).nu is None
    assert SparseMultivariateGibbsKernel(x[:40].clone(), 2, x[:40].clone()).nu is None
    for nu in NUS:
        assert MultivariateGibbsKernel(x, 2, nu=nu).nu == nu
        assert SparseMultivariateGibbsKernel(x[:40].clone(), 2, x[:40].clone(), nu=nu).nu == nu
    assert not any(key == 'nu' or key.endswith('.nu') for key in MultivariateGibbsKernel(x, 2, nu=1.5).state_dict())

    _oracle_with(monkeypatch, 1.5)
    torch.manual_seed(0)
    k = MultivariateGibbsKernel(x, 2, nu=1.5)
    ls = torch.full((1, 2), math.log(2.0), dtype=F64)            # softplus(0): `lengthscale=` kwarg is swallowed
    col = 5.0 * torch.eye(2, dtype=F64)
    H, Dm = k.H.detach().cpu().double(), k.D.detach().cpu().double()
    xd, xsd = x.cpu().double(), xs.cpu().double()
    Kxx = k(x).evaluate()
    ref = psgibbs.mv_gibbs_forward(xd, xd, xd, H, Dm, ls, col)
    assert measured('PS nu=1.5 Kxx', Kxx, ref, rtol=2e-4, atol=2e-5)
    Ksx = k(xs, x).evaluate()
    ref_sx = psgibbs.mv_gibbs_forward(xsd, xd, xd, H, Dm, ls, col)
    assert measured('PS nu=1.5 cross-covariance', Ksx, ref_sx, rtol=KSX_TOL, atol=KSX_TOL)
    # it is the Matern kernel: the squared-exponential one is far outside the bound
    S = psgibbs.kernels.ps_sigma(H, Dm)
    rbf = ps2d_matern_ref(xd, xd, S, S, 1e-5, None, radial=lambda s, nu: torch.exp(-0.5 * s))
    assert not measured('PS nu=1.5 Kxx vs the squared-exponential kernel', Kxx, rbf, rtol=2e-4, atol=2e-5)
    # gradient reaches D only (H is detached inside the kernel, reference :85,98)
    Kxx.sum().backward()
    assert k.D.grad is not None and float(k.D.grad.abs().max()) > 0
    assert k.H.grad is None or float(k.H.grad.abs().max()) == 0.0
    # sparse variant: H at M inducing locations
    _oracle_with(monkeypatch, 0.5)
    Z = x[:40].clone()
    ks = SparseMultivariateGibbsKernel(Z, 2, Z.clone(), nu=0.5)
    Kn = ks(x).evaluate()
    refn = psgibbs.mv_gibbs_forward(xd, xd, Z.cpu().double(), ks.H.detach().cpu().double(),
                                    ks.D.detach().cpu().double(), ls, torch.eye(2, dtype=F64), row_os=math.log(2.0))
    assert measured('sparse PS nu=0.5 Knn', Kn, refn, rtol=KN_TOL, atol=KN_TOL)
    Kn.sum().backward()
    assert ks.D.grad is not None and float(ks.D.grad.abs().max()) > 0
    assert ks.H.grad is None or float(ks.H.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 8: an exact GP
def test_exact_gp_over_the_multivariate_gibbs_kernel_with_nu(data_dir, ops):
    """ExactGPModel(ScaleKernel(MultivariateGibbsKernel(x[:200], 2, nu = 3/2))) in float64: the marginal log likelihood and
    its gradient with respect to D against a float64 torch restatement (the restatement kernel through ps_sigma(H, D), a
    Cholesky, an MVN log-prob), under the bounds of test_diagonal_exact_gp_objective_gradient_and_predict (1e-7 relative;
    rtol 1e-6, atol 1e-9).  The prior on H adds log p(H) to the objective, a term without D: it is taken from the model."""
    import nsgp.gp as gpytorch
    import models.dgps as m
    from models.multivariate_gibbs_kernel import MultivariateGibbsKernel
    from oracle import exact, kernels as OK
    from test_gpu_models import _uib_spatial
    xtr, ytr, _, _ = _uib_spatial(data_dir)
    x, y = xtr[:200], ytr[:200]
    torch.manual_seed(0)
    base = MultivariateGibbsKernel(x.float().cuda(), 2, nu=1.5)      # built in float32 as everywhere; .double() below
    likelihood = gpytorch.likelihoods.GaussianLikelihood()
    kernel = gpytorch.kernels.ScaleKernel(base)
    model = m.ExactGPModel(x, y, likelihood, kernel).double().cuda()
    model.likelihood.noise = 0.05
    kernel.outputscale = 0.644
    model.mean_module.constant.data.fill_(0.1)
    with torch.no_grad():
        base.D.copy_(torch.tensor(DMAT, dtype=F64))
    assert base.D.dtype == F64 and base.H.dtype == F64
    model.train()
    likelihood.train()
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(likelihood, model)
    val = mll(model(model.train_inputs[0]), model.train_targets)
    val.backward()
    log_prior = float(base.prior_H.log_prob(base.H.detach()).sum()) / 200

    Dr = torch.tensor(DMAT, dtype=F64, requires_grad=True)
    S = OK.ps_sigma(base.H.detach().cpu(), Dr)
    cov = 0.644 * ps2d_matern_ref(x, x, S, S, 1e-5, 1.5) + 0.05 * torch.eye(200, dtype=F64)
    ref = exact.mvn_log_prob(y, torch.full((200,), 0.1, dtype=F64), cov) / 200
    ref.backward()
    rel = abs(float(val) - log_prior - float(ref)) / abs(float(ref))
    print(f'[measured] ExactGP over MultivariateGibbsKernel nu=1.5: MLL {float(val) - log_prior:.9f} (restatement '
          f'{float(ref):.9f}, log p(H) / n = {log_prior:.6g}), rel err {rel:.3g}')
    assert rel < 1e-7
    assert measured('ExactGP over MultivariateGibbsKernel nu=1.5 grad D', base.D.grad, Dr.grad, rtol=1e-6, atol=1e-9)
