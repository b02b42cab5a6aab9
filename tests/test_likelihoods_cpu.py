"""BernoulliLikelihood (probit) and StudentTLikelihood without a GPU: the class surface, the torch-op path of expected_log_prob /
log_marginal against a float64 restatement written here, the 20-node rule and the closed-form predictive moments against
adaptive quadrature, the data-parallel objective's shares, and the host-side argument checks of the Gauss-Hermite entry point.

The restatement (gh_ell_ref, gh_log_marginal_ref) uses numpy's hermgauss, torch.special.log_ndtr, torch.lgamma and torch.log1p
and never the classes under test; tests/test_gpu_likelihoods.py imports it as the reference of the HIP kernel."""
import ctypes
import math

import numpy as np
import pytest
import torch

F32, F64 = torch.float32, torch.float64
BERNOULLI, STUDENT_T = 0, 1


# ------------------------------------------------------------------------------------------ the restatement
def _rule(Q, dt=F64):
    t, w = np.polynomial.hermite.hermgauss(Q)
    return torch.from_numpy(t).to(dt), torch.from_numpy(w).to(dt)


def student_t_normaliser(nu):
    return torch.lgamma(0.5 * (nu + 1.0)) - torch.lgamma(0.5 * nu) - 0.5 * torch.log(nu * math.pi)


def log_density_ref(kind, y, f, params=None, normaliser=True):
    """log p(y | f), broadcasting; params = (nu, s2) tensors for Student-t.  normaliser=False: the part the kernels evaluate."""
    if kind == BERNOULLI:
        return torch.special.log_ndtr((2.0 * y - 1.0) * f)
    nu, s2 = params
    lp = -0.5 * (nu + 1.0) * torch.log1p((y - f) ** 2 / (nu * s2)) - 0.5 * torch.log(s2)
    return lp + student_t_normaliser(nu) if normaliser else lp


def _nodes_values(kind, y, mu, v, params, Q, normaliser):
    t, w = _rule(Q, mu.dtype)
    f = mu.unsqueeze(-1) + torch.sqrt(2.0 * v).unsqueeze(-1) * t
    return log_density_ref(kind, y.unsqueeze(-1), f, params, normaliser), w


def gh_ell_ref(kind, y, mu, v, params=None, Q=20, normaliser=True):
    """pi^-1/2 sum_k w_k log p(y | mu + sqrt(2 v) t_k) per point, in mu's dtype; differentiable."""
    lp, w = _nodes_values(kind, y, mu, v, params, Q, normaliser)
    return (lp * w).sum(-1) / math.sqrt(math.pi)


def gh_log_marginal_ref(kind, y, mu, v, params=None, Q=20, normaliser=True):
    """log(pi^-1/2 sum_k w_k p(y | mu + sqrt(2 v) t_k)) per point as a log-sum-exp."""
    lp, w = _nodes_values(kind, y, mu, v, params, Q, normaliser)
    keep = w > 0
    return torch.logsumexp(lp[..., keep] + torch.log(w[keep]), dim=-1) - 0.5 * math.log(math.pi)


def point_inputs(kind, S, n, seed, dt=F64):
    """mu uniform in [-6, 6], v log-uniform in [1e-4, 9]; Bernoulli y in {0, 1}, Student-t y ~ 3 N(0, 1).  Float64 draws,
    rounded to dt (so that both dtypes see the same numbers up to that rounding)."""
    g = torch.Generator().manual_seed(seed)
    mu = 12.0 * torch.rand(S, n, generator=g, dtype=F64) - 6.0
    v = torch.exp(math.log(1e-4) + (math.log(9.0) - math.log(1e-4)) * torch.rand(S, n, generator=g, dtype=F64))
    if kind == BERNOULLI:
        y = (torch.rand(n, generator=g, dtype=F64) < 0.5).to(F64)
    else:
        y = 3.0 * torch.randn(n, generator=g, dtype=F64)
    return y.to(dt), mu.to(dt), v.to(dt)


STUDENT_PARAMS = (2.7, 0.6)


def _params64(kind):
    return None if kind == BERNOULLI else tuple(torch.tensor(p, dtype=F64) for p in STUDENT_PARAMS)


class _Dist:
    def __init__(self, mean, variance):
        self.mean, self.variance = mean, variance
        self.event_shape = mean.shape[-1:]


def _likelihood(kind, dt):
    from nsgp.gp.likelihoods import BernoulliLikelihood, StudentTLikelihood
    if kind == BERNOULLI:
        return BernoulliLikelihood().to(dt)
    lik = StudentTLikelihood().to(dt)
    lik.deg_free, lik.noise = (torch.tensor(p, dtype=F64) for p in STUDENT_PARAMS)      # (a Python float would pass through float32)
    return lik


# ------------------------------------------------------------------------------------------ surface
def test_class_surface():
    from nsgp.gp import settings
    from nsgp.gp.likelihoods import BernoulliLikelihood, StudentTLikelihood, _OneDimensionalLikelihood
    b, s = BernoulliLikelihood(), StudentTLikelihood()
    assert isinstance(b, _OneDimensionalLikelihood) and isinstance(s, _OneDimensionalLikelihood)
    assert sorted(b.state_dict()) == ['quadrature.locations', 'quadrature.weights'] and not list(b.parameters())
    assert sorted(s.state_dict()) == ['quadrature.locations', 'quadrature.weights', 'raw_deg_free', 'raw_noise']
    assert b.quadrature.locations.shape == (20,) and b.quadrature.weights.dtype == torch.get_default_dtype()
    assert float(s.raw_deg_free.detach()) == 0.0 and float(s.raw_noise.detach()) == 0.0
    assert abs(float(s.deg_free.detach()) - 2.6931) < 1e-4 and abs(float(s.noise.detach()) - 0.6931) < 1e-4
    s.deg_free, s.noise = 5.25, 0.125
    assert abs(float(s.deg_free.detach()) - 5.25) < 1e-5 and abs(float(s.noise.detach()) - 0.125) < 1e-6
    s.initialize(deg_free=3.0, noise=2.0)
    assert abs(float(s.deg_free.detach()) - 3.0) < 1e-5 and abs(float(s.noise.detach()) - 2.0) < 1e-5
    assert StudentTLikelihood(batch_shape=torch.Size([3])).raw_deg_free.shape == (3, 1)
    # buffers follow the module; a dtype change refills them from the float64 rule
    t64, w64 = _rule(20)
    d = BernoulliLikelihood().double()
    assert torch.equal(d.quadrature.locations, t64) and torch.equal(d.quadrature.weights, w64)
    assert torch.equal(b.quadrature.locations, t64.float())
    for Q in (1, 5, 64):
        with settings.num_gauss_hermite_locs(Q):
            assert StudentTLikelihood().quadrature.weights.shape == (Q,)
    assert settings.num_gauss_hermite_locs.value() == 20
    for Q in (0, 65, -1, 2.5):
        with settings.num_gauss_hermite_locs(Q), pytest.raises(ValueError):
            BernoulliLikelihood()
    # forward(function_samples) gives the torch.distributions object
    f = torch.tensor([-1.0, 0.0, 2.0])
    assert torch.allclose(b(f).probs, torch.special.ndtr(f))
    st = s(f)
    assert isinstance(st, torch.distributions.StudentT) and torch.allclose(st.loc, f) and bool(((st.scale - 2.0 ** 0.5).abs() < 1e-5).all())


def test_deep_gp_takes_a_likelihood_and_keeps_the_gaussian_default():
    import models.dgps as m
    from nsgp.gp.likelihoods import GaussianLikelihood, StudentTLikelihood
    assert isinstance(m.DeepGP(1, (50, 2), num_inducing=4).likelihood, GaussianLikelihood)
    lik = StudentTLikelihood()
    model = m.DeepGP(1, (50, 2), num_inducing=4, likelihood=lik)
    assert model.likelihood is lik and 'likelihood.raw_deg_free' in model.state_dict()


# ------------------------------------------------------------------------------------------ the torch-op path
@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
def test_cpu_path_matches_the_restatement_in_float64(kind):
    y, mu, v = point_inputs(kind, 3, 257, 11 + kind)
    lik = _likelihood(kind, F64)
    ell = lik.expected_log_prob(y, _Dist(mu, v))
    lm = lik.log_marginal(y, _Dist(mu, v))
    p = None if kind == BERNOULLI else (lik.deg_free.detach(), lik.noise.detach())
    assert ell.shape == (3, 257) and lm.shape == (3, 257)
    torch.testing.assert_close(ell, gh_ell_ref(kind, y, mu, v, p), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(lm, gh_log_marginal_ref(kind, y, mu, v, p), rtol=1e-12, atol=0.0)
    # one point, no sample dimension
    torch.testing.assert_close(lik.expected_log_prob(y[:1], _Dist(mu[0, :1], v[0, :1])), gh_ell_ref(kind, y[:1], mu[0, :1], v[0, :1], p),
                               rtol=1e-12, atol=0.0)


@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
def test_cpu_path_matches_the_restatement_in_float32(kind):
    """Bound: 4 x the float32 restatement's own distance from the float64 one on these inputs, 3e-7 of max(|ref|, 1)."""
    y, mu, v = point_inputs(kind, 3, 257, 11 + kind, F32)
    lik = _likelihood(kind, F32)
    p32 = None if kind == BERNOULLI else (lik.deg_free.detach(), lik.noise.detach())
    p64 = None if p32 is None else tuple(t.double() for t in p32)
    for name, fn, ref_fn in (('expected_log_prob', lik.expected_log_prob, gh_ell_ref), ('log_marginal', lik.log_marginal, gh_log_marginal_ref)):
        got = fn(y, _Dist(mu, v)).detach()
        ref = ref_fn(kind, y.double(), mu.double(), v.double(), p64)
        own = ref_fn(kind, y, mu, v, p32)
        scale = ref.abs().clamp_min(1.0)
        print(f'[measured] {name} kind {kind} float32: class {float(((got - ref).abs() / scale).max()):.3g}, '
              f'restatement {float(((own - ref).abs() / scale).max()):.3g} of max(|ref|, 1)')
        assert got.dtype == F32 and bool(((got.double() - ref).abs() <= 4 * 3e-7 * scale).all())


def test_student_t_gradients_reach_the_raw_parameters_on_the_cpu():
    y, mu, v = point_inputs(STUDENT_T, 2, 33, 5)
    lik = _likelihood(STUDENT_T, F64)
    mu.requires_grad_()
    lik.expected_log_prob(y, _Dist(mu, v)).sum().backward()
    nu, s2 = (torch.tensor(p, dtype=F64, requires_grad=True) for p in STUDENT_PARAMS)
    mu2 = mu.detach().clone().requires_grad_()
    gh_ell_ref(STUDENT_T, y, mu2, v, (nu, s2)).sum().backward()
    torch.testing.assert_close(mu.grad, mu2.grad, rtol=1e-11, atol=1e-13)
    # d/d raw = d/d constrained * sigmoid(raw) (softplus)
    torch.testing.assert_close(lik.raw_deg_free.grad.reshape(()), nu.grad * torch.sigmoid(lik.raw_deg_free.detach()).reshape(()),
                               rtol=1e-10, atol=0.0)
    torch.testing.assert_close(lik.raw_noise.grad.reshape(()), s2.grad * torch.sigmoid(lik.raw_noise.detach()).reshape(()),
                               rtol=1e-10, atol=0.0)


# ------------------------------------------------------------------------------------------ against exact integrals
GRID = [(mu, v) for mu in (-3.0, 0.0, 0.7, 3.0) for v in (1e-4, 0.05, 0.5)]


def _expect(g, mu, v):
    """E_{N(f | mu, v)} g(f) by adaptive quadrature over mu +- 12 standard deviations (the rest is below 1e-30)."""
    from scipy.integrate import quad
    sd = math.sqrt(v)
    val, _ = quad(lambda f: g(f) * math.exp(-0.5 * ((f - mu) / sd) ** 2) / (sd * math.sqrt(2 * math.pi)), mu - 12 * sd, mu + 12 * sd,
                  epsabs=1e-13, epsrel=1e-13, limit=400, points=[mu])
    return val


def _scalar_log_density(kind, y):
    from scipy.special import log_ndtr, gammaln
    if kind == BERNOULLI:
        return lambda f: float(log_ndtr((2 * y - 1) * f))
    nu, s2 = STUDENT_PARAMS
    c = gammaln((nu + 1) / 2) - gammaln(nu / 2) - 0.5 * math.log(nu * math.pi * s2)
    return lambda f: c - (nu + 1) / 2 * math.log1p((y - f) ** 2 / (nu * s2))


@pytest.mark.parametrize('kind,y', [(BERNOULLI, 1.0), (BERNOULLI, 0.0), (STUDENT_T, 0.7)])
def test_expected_log_prob_against_adaptive_quadrature(kind, y):
    """The 20-node rule itself is within 4.8e-7 of the exact integral on this grid; bound 1e-6 absolute."""
    lik = _likelihood(kind, F64)
    mu = torch.tensor([g[0] for g in GRID], dtype=F64)
    v = torch.tensor([g[1] for g in GRID], dtype=F64)
    got = lik.expected_log_prob(torch.full_like(mu, y), _Dist(mu, v))
    want = torch.tensor([_expect(_scalar_log_density(kind, y), m, s) for m, s in GRID], dtype=F64)
    print(f'[measured] expected_log_prob kind {kind} y {y} vs adaptive quadrature: max |diff| {float((got - want).abs().max()):.3g}')
    assert float((got - want).abs().max()) < 1e-6


def test_predictive_moments_against_adaptive_quadrature():
    """Closed forms: Bernoulli p = Phi(mu / sqrt(1 + v)), p (1 - p); Student-t mu, v + noise nu / (nu - 2).  Tolerance 1e-9."""
    from scipy.integrate import quad
    from scipy.special import ndtr
    from scipy import stats
    mu = torch.tensor([g[0] for g in GRID], dtype=F64)
    v = torch.tensor([g[1] for g in GRID], dtype=F64)
    # a leading sample dimension is carried through unchanged
    dist = _Dist(mu.expand(2, -1), v.expand(2, -1))
    b = _likelihood(BERNOULLI, F64)(dist)
    p = torch.tensor([_expect(lambda f: float(ndtr(f)), m, s) for m, s in GRID], dtype=F64)
    assert b.mean.shape == (2, len(GRID)) and b.variance.shape == (2, len(GRID))
    assert float((b.mean - p).abs().max()) < 1e-9 and float((b.variance - p * (1 - p)).abs().max()) < 1e-9
    lik = _likelihood(STUDENT_T, F64)
    s = lik(dist)
    nu, s2 = STUDENT_PARAMS
    sd = math.sqrt(s2)
    var_t, _ = quad(lambda r: r * r * stats.t.pdf(r / sd, nu) / sd, -np.inf, np.inf, epsabs=1e-13, epsrel=1e-13, limit=500)
    e1 = torch.tensor([_expect(lambda f: f, m, q) for m, q in GRID], dtype=F64)             # E y = E f
    e2 = torch.tensor([_expect(lambda f: f * f + var_t, m, q) for m, q in GRID], dtype=F64)  # E y^2 = E [f^2 + var(y | f)]
    assert s.mean.shape == (2, len(GRID))
    assert float((s.mean - e1).abs().max()) < 1e-9 and float((s.variance - (e2 - e1 ** 2)).abs().max()) < 1e-9


# ------------------------------------------------------------------------------------------ data-parallel shares
class _Strategy:
    def __init__(self, kl):
        self.kl = kl

    def kl_divergence(self):
        return self.kl


def test_data_parallel_shares_sum_to_the_one_process_objective():
    """dp_objective(..., world=2) on the two halves of a CPU batch sums to DeepApproximateMLL(VariationalELBO(StudentTLikelihood,
    ...)) of the whole batch: q(f) and the KL from the float64 oracle, the likelihood's torch-op path.  float64, rtol 1e-12."""
    from nsgp.dist import dp_objective
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.gp.module import Module
    from oracle import svgp
    g = torch.Generator().manual_seed(3)
    B, S, M, D, N = 64, 3, 10, 2, 1000
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64)  # noqa: E731

    def layer(b, linear):
        p = dict(Z=r(b, M, D) if b else r(M, D), lengthscale=torch.rand((b, 1, D) if b else (1, D), generator=g, dtype=F64) + 0.7,
                 outputscale=torch.rand((b,) if b else (), generator=g, dtype=F64) + 0.5, m=0.3 * (r(b, M) if b else r(M)),
                 Lq=torch.tril(0.1 * (r(b, M, M) if b else r(M, M))) + torch.eye(M, dtype=F64))
        p['mean'] = ('linear', r(D, 1), r(1)) if linear else ('constant', r(1))
        return p
    hidden, last = layer(2, True), layer(0, False)
    x, y = r(B, D), 3.0 * r(B)
    mean, var = svgp.dgp_forward(x, hidden, last, 1, [r(S, B, 2)], S)
    kl = svgp.kl_whitened(hidden) + svgp.kl_whitened(last)
    model = Module()
    model.variational_strategy = _Strategy(kl)
    lik = _likelihood(STUDENT_T, F64)
    mll = DeepApproximateMLL(VariationalELBO(lik, model, N))
    whole = mll(_Dist(mean, var), y)
    h = B // 2
    shares = [dp_objective(mll, _Dist(mean[:, sl], var[:, sl]), y[sl], B, 2) for sl in (slice(0, h), slice(h, B))]
    torch.testing.assert_close(shares[0] + shares[1], whole, rtol=1e-12, atol=0.0)
    ref = (gh_ell_ref(STUDENT_T, y, mean, var, _params64(STUDENT_T)).sum(-1) / B - kl / N).mean(0)
    torch.testing.assert_close(whole, ref, rtol=1e-12, atol=0.0)
    neg = [dp_objective(mll, _Dist(mean[:, sl], var[:, sl]), y[sl], B, 2, negate=True) for sl in (slice(0, h), slice(h, B))]
    torch.testing.assert_close(neg[0] + neg[1], -whole, rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------ the C entry points' checks
@pytest.mark.parametrize('sfx', ['f32', 'f64'])
def test_gauss_hermite_entry_points_validate_their_arguments_on_the_host(sfx):
    """A bad argument is answered with minus its position before any launch (safe without a GPU), as tests/test_abi.py has it
    for the other entry points."""
    import nsgp
    lib = nsgp.load_library()
    assert lib.nsgp_abi_version() == 2                                          # nothing removed or re-signed
    buf = (ctypes.c_double * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    name = f'nsgp_gh_log_marginal_{sfx}'
    assert name in nsgp.declared_symbols()
    ok = [1, b, b, b, b, b, b, 20, 3, 100, b, None]     # (kind, y, mu, v, params, nodes, weights, Q, S, n, out, stream)
    bad = lambda i, val: getattr(lib, name)(*[val if k == i - 1 else a for k, a in enumerate(ok)])  # noqa: E731
    assert bad(1, 2) == -1 and bad(1, -1) == -1                                 # kind
    assert bad(2, None) == -2 and bad(3, None) == -3 and bad(4, None) == -4
    assert bad(5, None) == -5                                                   # Student-t without (nu, s2)
    assert getattr(lib, name)(*[0] + ok[1:]) == -5                              # Bernoulli with params
    assert bad(6, None) == -6 and bad(7, None) == -7
    assert bad(8, 0) == -8 and bad(8, 65) == -8 and bad(8, -3) == -8            # Q
    assert bad(9, -1) == -9 and bad(9, 65536) == -9                             # S
    assert bad(10, -1) == -10 and bad(10, 2 ** 40) == -10                       # n: S n lanes must fit the grid
    assert bad(11, None) == -11
    assert bad(9, 0) == 0 and bad(10, 0) == 0                                   # nothing to launch


def test_ops_refuse_cpu_tensors():
    from nsgp import BackendError, ops
    y, mu, v = point_inputs(BERNOULLI, 2, 5, 0)
    t, w = _rule(20)
    with pytest.raises(BackendError):
        ops.gh_log_marginal(0, y, mu, v, None, t, w)
