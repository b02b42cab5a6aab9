"""BernoulliLikelihood / StudentTLikelihood on the GPU: the Gauss-Hermite log-marginal kernel (csrc/svgp.hip: gh_term,
gh_point_lse behind nsgp_gh_log_marginal) against the float64 restatement of tests/test_likelihoods_cpu.py (hermgauss,
log_ndtr, lgamma, log1p), the ELBO (torch ops on the device) and `predict` of models built on it against the oracle's q(f)
and KL plus that restatement, the example's Student-t run, and the launches of a Gaussian step.  Tolerances are the project's
own for the same kind of quantity, imported where they have a name and quoted where they do not."""
import pytest
import torch

from conftest import measured
from test_gpu_dgp import DSVI_GRAD_TOL, _FixedEps
from test_gpu_matern import _tol
from test_likelihoods_cpu import BERNOULLI, STUDENT_T, STUDENT_PARAMS, _rule, gh_ell_ref, gh_log_marginal_ref, point_inputs

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
sp = torch.nn.functional.softplus


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dev(t, dt):
    return None if t is None else t.to(dt).cuda()


def _params(kind, dt):
    """(nu, s2) as the device sees them (rounded to dt), in float64 on the host; None for Bernoulli."""
    return None if kind == BERNOULLI else torch.tensor(STUDENT_PARAMS, dtype=F64).to(dt).double()


def _case(kind, S, n, seed, dt):
    """Inputs rounded to dt, held in float64: mu in [-6, 6], v in [1e-4, 9], so the nodes reach z ~ -29."""
    y, mu, v = (t.double() for t in point_inputs(kind, S, n, seed, dt))
    p = _params(kind, dt)
    return y, mu, v, p, (None if p is None else tuple(p))


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
@pytest.mark.parametrize('S,n', [(4096, 1), (3, 257), (1, 1), (2, 65537)])
def test_log_marginal_matches_the_restatement(S, n, kind, dt):
    """Per-point values at test_gpu_matern._tol (the project's tolerance for transcendental element kernels): rows of one
    point, a ragged last block, one point, and rows longer than 2^16; the class on CUDA tensors (normaliser included) too."""
    from nsgp import ops
    from nsgp.gp.likelihoods import BernoulliLikelihood, StudentTLikelihood
    y64, mu64, v64, p64, par = _case(kind, S, n, 300 + n, dt)
    t, w = _rule(20)
    y, mu, v, p = _dev(y64, dt), _dev(mu64, dt), _dev(v64, dt), _dev(p64, dt)
    lm = ops.gh_log_marginal(kind, y, mu, v, p, _dev(t, dt), _dev(w, dt))
    assert lm.shape == (S, n) and bool(torch.isfinite(lm).all())
    ref = gh_log_marginal_ref(kind, y64, mu64, v64, par, normaliser=False)
    assert kind == STUDENT_T or S * n < 1000 or float(ref.min()) < -10.0         # log Phi's lower tail IS in the inputs
    assert measured(f'gh log marginal kind {kind} {dt} ({S},{n})', lm, ref, **_tol(dt))
    lik = (BernoulliLikelihood() if kind == BERNOULLI else StudentTLikelihood()).to(dt).cuda()
    if kind == STUDENT_T:
        lik.deg_free, lik.noise = p64[0], p64[1]
        par = (lik.deg_free.detach().cpu().double().reshape(()), lik.noise.detach().cpu().double().reshape(()))

    class D:
        mean, variance = mu, v
    with torch.no_grad():
        got = lik.log_marginal(y, D)
    assert got.shape == (S, n)
    assert measured(f'likelihood.log_marginal kind {kind} {dt}', got, gh_log_marginal_ref(kind, y64, mu64, v64, par), **_tol(dt))


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
@pytest.mark.parametrize('Q', [1, 5, 20, 64])
def test_node_counts(Q, kind, dt):
    from nsgp import ops
    y64, mu64, v64, p64, par = _case(kind, 3, 257, 900 + Q, dt)
    t, w = _rule(Q)
    lm = ops.gh_log_marginal(kind, _dev(y64, dt), _dev(mu64, dt), _dev(v64, dt), _dev(p64, dt), _dev(t, dt), _dev(w, dt))
    ref = gh_log_marginal_ref(kind, y64, mu64, v64, par, Q=Q, normaliser=False)
    assert measured(f'gh log marginal Q{Q} kind {kind} {dt}', lm, ref, **_tol(dt))


def test_bad_operands_are_an_error_not_a_launch():
    from nsgp import BackendError, ops
    y, mu, v = (t.cuda() for t in point_inputs(BERNOULLI, 2, 5, 0, F32))
    t, w = (x.float().cuda() for x in _rule(65))
    t20, w20 = t[:20].contiguous(), w[:20].contiguous()
    with pytest.raises(BackendError):
        ops.gh_log_marginal(BERNOULLI, y, mu, v, None, t, w)                     # more than 64 nodes
    with pytest.raises(BackendError):
        ops.gh_log_marginal(STUDENT_T, y, mu, v, None, t20, w20)                 # Student-t needs its two parameters
    with pytest.raises(BackendError):
        ops.gh_log_marginal(BERNOULLI, y, mu, v, torch.ones(2, device='cuda'), t20, w20)
    with pytest.raises(BackendError):
        ops.gh_log_marginal(BERNOULLI, y[:4], mu, v, None, t20, w20)
    with pytest.raises(BackendError):
        ops.gh_log_marginal(2, y, mu, v, None, t20, w20)
    torch.cuda.synchronize()


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
def test_a_nan_stays_in_its_point(kind, dt):
    from nsgp import ops
    S, n = 3, 257
    y, mu, v = (_dev(t, dt) for t in point_inputs(kind, S, n, 55, dt))
    p = _dev(_params(kind, dt), dt)
    t, w = _dev(_rule(20)[0], dt), _dev(_rule(20)[1], dt)
    clean = ops.gh_log_marginal(kind, y, mu, v, p, t, w)
    mu[1, 256] = float('nan')
    v[2, 0] = float('nan')
    y[7] = float('nan')                                                         # a target: its whole column
    out = ops.gh_log_marginal(kind, y, mu, v, p, t, w)
    bad = torch.zeros(S, n, dtype=torch.bool, device='cuda')
    bad[1, 256] = bad[2, 0] = True
    bad[:, 7] = True
    assert torch.equal(torch.isnan(out), bad) and torch.equal(out[~bad], clean[~bad])


# ------------------------------------------------------------------------------------------ models
def _build(kind, dt, seed, D=2, M=33, variational='cholesky'):
    """test_gpu_dgp._build (parameters moved off their trivial initialisation) with a non-Gaussian likelihood."""
    import models.dgps as m
    from nsgp.gp.likelihoods import BernoulliLikelihood, StudentTLikelihood
    torch.manual_seed(seed)
    lik = BernoulliLikelihood() if kind == BERNOULLI else StudentTLikelihood()
    model = m.DeepGP(1, (1000, D), num_inducing=M, variational=variational, likelihood=lik).to(dt).cuda()
    g = _g(seed + 1)
    with torch.no_grad():
        for mod in (model.layers[0], model.last_layer):
            vd = mod.variational_strategy._variational_distribution
            vd.variational_mean.copy_(0.3 * torch.randn(vd.variational_mean.shape, generator=g))
            if hasattr(vd, '_variational_stddev'):
                vd._variational_stddev.copy_(0.5 + torch.rand(vd._variational_stddev.shape, generator=g))
            else:
                vd.chol_variational_covar.copy_(torch.tril(0.1 * torch.randn(vd.chol_variational_covar.shape, generator=g))
                                                + torch.eye(M))
            mod.variational_strategy.variational_params_initialized.fill_(1)
            mod.covar_module.base_kernel.raw_lengthscale.add_(0.3 * torch.randn(
                mod.covar_module.base_kernel.raw_lengthscale.shape, generator=g).cuda())
        if kind == STUDENT_T:
            lik.raw_deg_free.fill_(0.4)
            lik.raw_noise.fill_(-0.7)
    return model


def _oracle_layers(model):
    """Float64 CPU leaves of every raw parameter, the oracle's layer dicts built on them (a mean-field layer's Lq is
    diag_embed(s)) and the likelihood's (nu, s2): (hidden, last, par, leaves, params)."""
    leaves, params = {}, {}

    def leaf(name, p):
        params[name] = p
        leaves[name] = p.detach().cpu().double().clone().requires_grad_()
        return leaves[name]

    def layer(prefix, mod, linear):
        vs = mod.variational_strategy
        vd = vs._variational_distribution
        d = dict(Z=leaf(prefix + 'Z', vs.inducing_points),
                 lengthscale=sp(leaf(prefix + 'raw_ls', mod.covar_module.base_kernel.raw_lengthscale)),
                 outputscale=sp(leaf(prefix + 'raw_os', mod.covar_module.raw_outputscale)),
                 m=leaf(prefix + 'm', vd.variational_mean))
        if hasattr(vd, '_variational_stddev'):
            d['Lq'] = torch.diag_embed(leaf(prefix + 'raw_stddev', vd._variational_stddev).abs().clamp_min(1e-8))
        else:
            d['Lq'] = leaf(prefix + 'Lq', vd.chol_variational_covar)
        if linear:
            d['mean'] = ('linear', leaf(prefix + 'w', mod.mean_module.weights), leaf(prefix + 'b', mod.mean_module.bias))
        else:
            d['mean'] = ('constant', leaf(prefix + 'c', mod.mean_module.constant))
        return d
    hidden, last = layer('h.', model.layers[0], True), layer('l.', model.last_layer, False)
    lik = model.likelihood
    par = None
    if hasattr(lik, 'raw_deg_free'):
        par = (sp(leaf('raw_deg_free', lik.raw_deg_free)).reshape(()) + 2.0, sp(leaf('raw_noise', lik.raw_noise)).reshape(()))
    return hidden, last, par, leaves, params


def _targets(kind, B, g):
    return (torch.rand(B, generator=g) < 0.4).float() if kind == BERNOULLI else 2.0 * torch.randn(B, generator=g)


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('variational', ['cholesky', 'mean_field'])
@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
def test_model_objective_and_gradients_match_oracle(kind, variational, dt):
    """-DeepApproximateMLL(VariationalELBO) of DeepGP(1, (N, 2), num_inducing=33, likelihood=L) at B = 65, S = 3 and the
    gradient of every parameter, the likelihood's own included, against autograd of the oracle's q(f) and KL plus the
    restatement; bounds of test_gpu_dgp.test_dsvi_elbo_and_gradients_match_oracle (value 2e-6 relative + 1e-7, gradients
    DSVI_GRAD_TOL max-norm relative).  These likelihoods have no fused objective: fused_dsvi_objective answers None and the
    ELBO term is expected_log_prob in torch ops on the device."""
    from oracle import svgp
    from nsgp.gp import mlls, settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    B, S, N, D = 65, 3, 5000, 2
    model = _build(kind, dt, 40 + kind, variational=variational)
    g = _g(8)
    x, y = torch.randn(B, D, generator=g), _targets(kind, B, g)
    eps = [torch.randn(S, B, 2, generator=g)]
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, N))
    xd, yd = x.to(dt).cuda(), y.to(dt).cuda()
    model.train()
    with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        out = model(xd)
        assert mlls.fused_dsvi_objective(mll.base_mll, out, yd, 1.0, 1.0) is None
        ell = model.likelihood.expected_log_prob(yd, out)
        assert ell.shape == (S, B) and ell.is_cuda and ell.dtype == dt
        loss = -mll(out, yd)
        loss.backward()
    hidden, last, par, leaves, params = _oracle_layers(model)
    mean, var = svgp.dgp_forward(x.to(dt).double(), hidden, last, 1, [e.to(dt).double() for e in eps], S)
    ell_ref = gh_ell_ref(kind, y.double(), mean, var, par)
    ref = -(ell_ref.sum(-1) / B - (svgp.kl_whitened(hidden) + svgp.kl_whitened(last)) / N).mean(0)
    ref.backward()
    tol = dict(rtol=1e-9, atol=1e-10) if dt == F64 else dict(rtol=2e-3, atol=2e-4)     # float32: test_gpu_dgp's predict bound
    assert measured(f'gh expected_log_prob on the device kind {kind} {variational} {dt}', ell, ell_ref, **tol)
    got, ref = float(loss.detach()), float(ref.detach())
    print(f'[measured] gh model loss kind {kind} {variational} {dt}: rel err {abs(got - ref) / abs(ref):.3g}')
    assert abs(got - ref) < 2e-6 * abs(ref) + 1e-7
    assert set(params) == set(leaves) and (kind == BERNOULLI or {'raw_deg_free', 'raw_noise'} <= set(params))
    errs = {}
    for name, p in params.items():
        have, want = p.grad.detach().cpu().double(), leaves[name].grad
        if name.endswith('Lq'):
            want = torch.tril(want)
        errs[name] = float((have - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    print(f'[measured] gh model grads kind {kind} {variational} {dt}:', {k: '%.3g' % e for k, e in errs.items()})
    for name, err in errs.items():
        assert err < DSVI_GRAD_TOL, (name, err)


@pytest.mark.parametrize('kind', [BERNOULLI, STUDENT_T])
def test_predict_gives_the_closed_form_moments_of_the_oracles_q_f(kind):
    """predict on a two-batch loader: (S, N) outputs, finite, equal to the closed-form moments and the restated log marginal
    applied to the oracle's q(f); bounds of test_gpu_dgp.test_predict_matches_oracle_and_full_covariance_is_consistent."""
    from oracle import svgp
    from nsgp import ops
    from nsgp.gp import settings
    model = _build(kind, F32, 60 + kind)
    g = _g(9)
    n, S = 39, 4
    xs = [torch.randn(n, 2, generator=g) for _ in range(2)]
    ys = [_targets(kind, n, g) for _ in range(2)]
    eps = [torch.randn(S, n, 2, generator=g)]
    model.eval()
    calls = []
    orig = ops._lib.call
    ops._lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
            preds, mus, variances, lls = model.predict([(x.cuda(), y.cuda()) for x, y in zip(xs, ys)])
    finally:
        ops._lib.call = orig
    assert calls.count('nsgp_gh_log_marginal_f32') == 2                          # the kernel, once per batch
    assert mus.shape == (S, 2 * n) and variances.shape == (S, 2 * n) and lls.shape == (S, 2 * n)
    assert preds.mean.shape == (S, n) and all(bool(torch.isfinite(t).all()) for t in (mus, variances, lls))
    hidden, last, par, _, _ = _oracle_layers(model)
    m_ref, v_ref, ll_ref = [], [], []
    with torch.no_grad():
        for x, y in zip(xs, ys):
            mean, var = svgp.dgp_forward(x.double(), hidden, last, 1, [e.double() for e in eps], S)
            if kind == BERNOULLI:
                p = torch.special.ndtr(mean / (1.0 + var).sqrt())
                m_ref.append(p)
                v_ref.append(p * (1.0 - p))
            else:
                m_ref.append(mean)
                v_ref.append(var + par[1] * par[0] / (par[0] - 2.0))
            ll_ref.append(gh_log_marginal_ref(kind, y.double(), mean, var, par))
    tol = dict(rtol=2e-3, atol=2e-4)
    assert measured(f'gh predict mean kind {kind}', mus, torch.cat(m_ref, -1), **tol)
    assert measured(f'gh predict variance kind {kind}', variances, torch.cat(v_ref, -1), **tol)
    assert measured(f'gh predict lls kind {kind}', lls, torch.cat(ll_ref, -1), rtol=5e-3, atol=5e-3)


def test_spatial_example_trains_with_the_student_t_likelihood(tmp_path):
    """examples/deepgp_spatial.py --likelihood student_t on the bundled uib_spatial.csv, a short run: the loss falls from its
    first epoch's, the metrics are finite and the prediction frame has the reference's columns."""
    import importlib.util
    import os
    import types
    import utils.dataprep as dp
    from utils.config import DATASET_DIR
    ex = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples')
    import sys
    sys.path.insert(0, ex)
    try:
        spec = importlib.util.spec_from_file_location('deepgp_spatial', os.path.join(ex, 'deepgp_spatial.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ex)
    dataset = dp.download_data(str(DATASET_DIR / 'uib_spatial.csv'))
    base = dict(layers=1, inducing=32, batch=315, lr=0.01, samples=3, verbose=False, likelihood='student_t')
    first = mod.run_split(dataset, 0, types.SimpleNamespace(epochs=1, out=None, **base), torch.device('cuda', 0))
    rm, nl, loss, frame = mod.run_split(dataset, 0, types.SimpleNamespace(epochs=40, out=str(tmp_path / 'p.csv'), **base),
                                        torch.device('cuda', 0))
    print(f'[measured] student-t example: RMSE {rm:.4f} NLPD {nl:.4f} loss {first[2]:.4f} -> {loss:.4f}')
    assert all(map(lambda t: t == t and abs(t) < 1e6, (rm, nl, loss))) and loss < first[2]
    assert list(frame.columns) == ['pred', 'std', 'lat', 'lon'] and bool(frame.notna().all().all())


# ------------------------------------------------------------------------------------------ Gaussian models are untouched
@pytest.mark.parametrize('variational,node,entries', [
    ('cholesky', 'DsviObjectiveFnBackward', ['nsgp_dsvi_objective_fwd_f32', 'nsgp_dsvi_objective_bwd_f32']),
    ('mean_field', 'KlMeanFieldTotalFnBackward',
     ['nsgp_gauss_ell_total_fwd_f32', 'nsgp_kl_meanfield_total_acc_fwd_f32', 'nsgp_kl_meanfield_total_acc_fwd_f32',
      'nsgp_kl_meanfield_total_bwd_f32', 'nsgp_kl_meanfield_total_bwd_f32', 'nsgp_gauss_ell_total_bwd_f32'])])
def test_a_gaussian_step_launches_what_it_did(variational, node, entries):
    """The objective of a Gaussian DeepGP step goes through the entry points it always went through (the fused pair for
    Cholesky layers, the Gaussian head of the chain for mean-field ones), in the same order, and DeepGP's default likelihood
    is the Gaussian one."""
    import models.dgps as m
    from nsgp import ops
    from nsgp.gp import settings
    from nsgp.gp.likelihoods import GaussianLikelihood
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    torch.manual_seed(5)
    model = m.DeepGP(1, (1000, 2), num_inducing=33, variational=variational).cuda()
    assert isinstance(model.likelihood, GaussianLikelihood)
    g = _g(6)
    x, y = torch.randn(65, 2, generator=g).cuda(), torch.randn(65, generator=g).cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 1000))
    model.train()
    calls = []
    orig = ops._lib.call
    ops._lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        with settings.num_likelihood_samples(3):
            loss = mll(model(x), y)
            loss.backward()
    finally:
        ops._lib.call = orig
    assert type(loss.grad_fn).__name__ == node
    objective = [c for c in calls if any(k in c for k in ('gauss_ell', 'kl_', 'dsvi_objective', 'nsgp_gh_'))]
    assert objective == entries, objective
