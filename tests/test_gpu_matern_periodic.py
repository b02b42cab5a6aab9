"""MaternKernel * PeriodicKernel on the MI355X: the fused build and its backward (csrc/pairwise.hip, RadialPeriodicOp)
against the float64 restatement of tests/test_matern_periodic_cpu.py, and the kernel classes and the spatio-temporal
model built on it.

Tolerances start from the ceilings the project applies to this family (test_rbf_periodic_build_forward_backward: float64
1e-10 / 1e-11 on values and 1e-8 on gradients, float32 2e-4 / 2e-5 on values and 5e-3 with sqrt(n1 n2) scaling on
gradients; the exact-GP test from test_stationary_spatiotemporal_exact_gp_matches_oracle) and are tightened to about three
times the worst case measured on MI355X where that is far below the ceiling; every check
prints its worst |diff| / (atol + rtol |ref|) under -s.  The measured table is profiles/matern_periodic/errors.txt."""
import math

import pytest
import torch

from conftest import measured
from test_matern_periodic_cpu import matern_periodic_ref

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
    """values: ceilings 1e-10 / 1e-11 and 2e-4 / 2e-5; measured worst 4.3e-5 and 1.0e-2 of them"""
    return dict(rtol=1.5e-14, atol=1.5e-15) if dt == F64 else dict(rtol=6e-6, atol=6e-7)


def _gtol(dt, n1, n2):
    """gradients: ceilings 1e-8 and 5e-3 (a sum of n1 n2 terms, so the float32 absolute part grows with sqrt(n1 n2));
    measured worst 4.3e-6 and 8.7e-4 of them"""
    if dt == F64:
        return dict(rtol=1.5e-13, atol=1.5e-13)
    return dict(rtol=1.5e-5, atol=1.5e-5 * max(1.0, math.sqrt(n1 * n2) / 10))


# (batch, n1, n2, D, batched x).  Forward tile: 64 rows x 256 (float32) / 128 (float64) columns; backward tile: 16 or 64
# rows x 256 columns.  D = 3 takes the generic-dimension instance; (64, 65, 257, 1) is the smallest shape on the 64-row
# backward: batch * ceil(n1 / 64) * ceil(n2 / 256) = 256.
CASES = [(1, 1, 1, 1, False), (1, 63, 255, 1, False), (1, 64, 256, 1, False), (1, 65, 257, 1, False),
         (2, 65, 130, 1, True), (3, 100, 257, 2, False), (1, 5, 700, 3, False), (64, 65, 257, 1, False)]
IDS = [f'{c[0]}x{c[1]}x{c[2]}xD{c[3]}' + ('-batched' if c[4] else '') for c in CASES]
NAMES = ('x1', 'x2', 'ls_env', 'ls_per', 'period', 'os')


def _inputs(case, dt, seed):
    """float64 tensors holding values of type dt: x1, x2 (two points of x1 repeated in x2: zero distances), ls_env, ls_per,
    period, os, G."""
    b, n1, n2, D, batched = case
    g = _g(seed)
    lead = (b,) if batched else ()
    x1 = torch.randn(*lead, n1, D, generator=g, dtype=F64)
    x2 = torch.randn(*lead, n2, D, generator=g, dtype=F64)
    k = min(2, n1, n2)
    x2[..., n2 - k:, :] = x1[..., :k, :]
    le = torch.rand(b, D, generator=g, dtype=F64) + 0.6
    lp = torch.rand(b, generator=g, dtype=F64) + 0.5
    pe = torch.rand(b, generator=g, dtype=F64) + 0.8
    os_ = torch.rand(b, generator=g, dtype=F64) + 0.5
    G = torch.randn(b, n1, n2, generator=g, dtype=F64)
    return [t.to(dt).double() for t in (x1, x2, le, lp, pe, os_, G)]


def test_the_cases_reach_both_backward_tile_heights(ops):
    rows = {c[:3]: ops.pairwise_bwd_plan(*c[:3]).rows for c in CASES}
    assert rows[(1, 65, 257)] == 16 and rows[(64, 65, 257)] == 64 and set(rows.values()) == {16, 64}
    assert ops.pairwise_bwd_plan(63, 65, 257).rows == 16                     # one batch entry fewer: still the 16-row kernel


# ------------------------------------------------------------------------------------------ forward and six gradients
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_forward_and_all_gradients_match_the_restatement(ops, dt, nu, case):
    b, n1, n2, D, _ = case
    *ins, G = _inputs(case, dt, seed=17 + n1 + 7 * n2 + D)
    diag_add = 0.0123
    leaves = [t.clone().requires_grad_() for t in ins]
    ref = matern_periodic_ref(*leaves, nu) + diag_add * torch.eye(n1, n2, dtype=F64)
    (ref * G).sum().backward()
    cu = [t.to(dt).cuda().requires_grad_() for t in ins]
    got = ops.matern_periodic_kernel(*cu, nu, diag_add)
    assert got.shape == (b, n1, n2) and got.dtype == dt
    ok = measured(f'matern_periodic nu={nu} {dt} fwd {case}', got, ref, **_tol(dt))
    (got * G.to(dt).cuda()).sum().backward()
    for name, a, r in zip(NAMES, cu, leaves):
        assert a.grad.shape == r.grad.shape, name
        ok = measured(f'matern_periodic nu={nu} {dt} grad {name} {case}', a.grad, r.grad, **_gtol(dt, n1, n2)) and ok
    assert ok


@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('case', [CASES[3], CASES[5]], ids=[IDS[3], IDS[5]])
def test_without_outputscale_and_with_input_gradients_off(ops, dt, nu, case):
    """os_ = None is an outputscale of 1; an x that needs no gradient gets none and leaves every other gradient bit-equal
    (the same launch with one output pointer absent)."""
    b, n1, n2, D, _ = case
    *ins, G = _inputs(case, dt, seed=5 + n1)
    ins = ins[:5]
    leaves = [t.clone().requires_grad_() for t in ins]
    ref = matern_periodic_ref(*leaves, None, nu)
    (ref * G).sum().backward()
    Gc = G.to(dt).cuda()

    def run(need_x1, need_x2):
        cu = [t.to(dt).cuda() for t in ins]
        for i, t in enumerate(cu):
            t.requires_grad_(i >= 2 or (need_x1 if i == 0 else need_x2))
        K = ops.matern_periodic_kernel(*cu, None, nu)
        (K * Gc).sum().backward()
        return K, [t.grad for t in cu]
    K, full = run(True, True)
    ok = measured(f'matern_periodic nu={nu} {dt} no-os fwd {case}', K, ref, **_tol(dt))
    for name, a, r in zip(NAMES, full, leaves):
        ok = measured(f'matern_periodic nu={nu} {dt} no-os grad {name} {case}', a, r.grad, **_gtol(dt, n1, n2)) and ok
    assert ok
    for need in ((False, True), (True, False), (False, False)):
        K2, part = run(*need)
        assert torch.equal(K2, K)
        for i, (a, f) in enumerate(zip(part, full)):
            if i < 2 and not need[i]:
                assert a is None
            else:
                assert torch.equal(a, f), (need, NAMES[i])


def test_the_matern_path_of_the_node_refuses_a_second_derivative(ops):
    g = _g(2)
    x = torch.randn(20, 1, generator=g, dtype=F64).cuda().requires_grad_()
    one = torch.ones(1, dtype=F64, device='cuda')
    out = ops.matern_periodic_kernel(x, x, one.reshape(1, 1), one, one, one, 1.5)
    (gx,) = torch.autograd.grad((out * out).sum(), x, create_graph=True)
    assert bool(torch.isfinite(gx).all())
    with pytest.raises(RuntimeError, match='once_differentiable'):
        gx.sum().backward()


def test_shape_errors_name_the_op_and_its_argument(ops):
    x = torch.zeros(5, 2, dtype=F64, device='cuda')
    one = torch.ones(1, dtype=F64, device='cuda')
    with pytest.raises(ops.BackendError, match='matern_periodic_build: ls_env must be'):
        ops.matern_periodic_build(x, x, torch.ones(1, 3, dtype=F64, device='cuda'), one, one, one, 1.5)
    with pytest.raises(ops.BackendError, match='matern_periodic_build: os must be'):
        ops.matern_periodic_build(x, x, one.expand(1, 2), one, one, torch.ones(2, dtype=F64, device='cuda'), 1.5)
    with pytest.raises(ops.BackendError, match='rbf_periodic_build: ls_rbf must be'):
        ops.rbf_periodic_build(x, x, torch.ones(1, 3, dtype=F64, device='cuda'), one, one, one)


# ------------------------------------------------------------------------------------------ K(x, x)
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n,D', [(70, 1), (257, 2)])
def test_kxx_diagonal_is_the_outputscale_and_adds_no_gradient(ops, dt, nu, n, D):
    """One tensor in both roles: the diagonal is os + diag_add to a few ulp, nothing is NaN, and the diagonal of G does
    not reach the x, ls_env, ls_per and period gradients (bit for bit; nu = 1/2 by the kernel's convention)."""
    g = _g(41 + n)
    x = torch.randn(n, D, generator=g, dtype=F64).to(dt).double()
    le = (torch.rand(1, D, generator=g, dtype=F64) + 0.6).to(dt).double()
    lp, pe, os_ = [torch.tensor([v], dtype=F64).to(dt).double() for v in (0.9, 1.3, 1.7)]
    G = torch.randn(1, n, n, generator=g, dtype=F64).to(dt).double()
    diag_add = 0.25
    xr, *pr = [t.clone().requires_grad_() for t in (x, le, lp, pe, os_)]
    ref = matern_periodic_ref(xr, xr, *pr, nu) + diag_add * torch.eye(n, dtype=F64)
    (ref * G).sum().backward()

    def run(Gm):
        xc, *pc = [t.to(dt).cuda().requires_grad_() for t in (x, le, lp, pe, os_)]
        K = ops.matern_periodic_kernel(xc, xc, *pc, nu, diag_add)
        (K * Gm.to(dt).cuda()).sum().backward()
        return K.detach(), [t.grad for t in (xc, *pc)]
    K, grads = run(G)
    assert bool(torch.isfinite(K).all()) and all(bool(torch.isfinite(t).all()) for t in grads)
    want = (os_.to(dt) + torch.tensor(diag_add, dtype=dt)).item()
    ulp = abs(want) * torch.finfo(dt).eps
    worst = float((torch.diagonal(K[0]).double().cpu() - want).abs().max())
    print(f'[measured] matern_periodic nu={nu} {dt} K(x,x) n={n}: diagonal off os + diag_add by {worst / ulp:.3g} ulp')
    assert worst <= 4 * ulp
    ok = measured(f'matern_periodic nu={nu} {dt} K(x,x) n={n} fwd', K, ref, **_tol(dt))
    for name, a, r in zip(('x', 'ls_env', 'ls_per', 'period', 'os'), grads, (xr, *pr)):
        ok = measured(f'matern_periodic nu={nu} {dt} K(x,x) n={n} grad {name}', a, r.grad, **_gtol(dt, n, n)) and ok
    assert ok
    G2 = G.clone()
    torch.diagonal(G2[0]).copy_(torch.randn(n, generator=g, dtype=F64) * 100.0)
    _, grads2 = run(G2)
    for name, a, c in zip(('x', 'ls_env', 'ls_per', 'period'), grads, grads2):
        assert torch.equal(a, c), name
    assert not torch.equal(grads[4], grads2[4])                               # the outputscale does see the diagonal


# ------------------------------------------------------------------------------------------ periodicity
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
def test_periodic_in_the_period_and_the_envelope_alone_without_the_periodic_factor(ops, dt, nu):
    """D = 1.  k(x, x + m p) for m = 1, 2, 3 is the envelope at that distance times os (the periodic factor is 1 there),
    and with ls_per at 1e30 (float64) / 1e20 (float32) the whole build is ops.matern_build."""
    g = _g(9)
    n = 130
    x = torch.randn(n, 1, generator=g, dtype=F64).to(dt).cuda()
    le = torch.tensor([[2.3]], dtype=dt).cuda()
    lp, pe, os_ = [torch.tensor([v], dtype=dt).cuda() for v in (0.7, 1.25, 1.9)]      # 1.25 m: exact in both types
    one = torch.ones(1, dtype=dt).cuda()
    ok = True
    for m in (1, 2, 3):
        xs = x + m * pe
        got = torch.diagonal(ops.matern_periodic_build(x, xs, le, lp, pe, os_, nu)[0])
        want = torch.diagonal(ops.matern_build(x, xs, le, one, nu)[0]) * os_
        ok = measured(f'matern_periodic nu={nu} {dt} k(x, x + {m} p)', got, want, **_tol(dt)) and ok
    huge = torch.tensor([1e30 if dt == F64 else 1e20], dtype=dt).cuda()
    x2 = torch.randn(257, 1, generator=g, dtype=F64).to(dt).cuda()
    got = ops.matern_periodic_build(x, x2, le, huge, pe, os_, nu)
    want = ops.matern_build(x, x2, le, os_, nu)
    ok = measured(f'matern_periodic nu={nu} {dt} ls_per huge vs matern_build', got, want, **_tol(dt)) and ok
    assert ok


# ------------------------------------------------------------------------------------------ range, far tail, NaN
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
def test_distance_range_far_tail_and_nan(ops, dt, nu):
    """Points on a line whose distances span 1e-4 to 1e4 envelope lengthscales and up to 50 periods agree with the
    restatement relatively (as test_matern_distance_range_far_tail_and_nan: rtol alone; ceilings: the family's 1e-10 in
    float64, and in float32 that test's 3e-5 plus the rounding of theta = pi r / p, |d log E / d theta| theta eps <=
    4 * 50 pi * 2^-23 / ls_per = 7.5e-5; measured worst 1.1e-3 and 0.12 of them); an entry 1e6 lengthscales away is exactly 0; a NaN coordinate poisons exactly its row and column."""
    n = 96
    t = torch.cat([torch.zeros(1, dtype=F64), torch.logspace(-4, 4, n - 1, dtype=F64)])
    x = t.reshape(n, 1).to(dt)
    le, lp, pe, os_ = [torch.tensor(v, dtype=dt) for v in ([[1.0]], [1.0], [200.0], [1.0])]
    assert float((x.max() - x.min()) / pe) == 50.0
    dev = lambda *ts: [a.cuda() for a in ts]                                        # noqa: E731
    K = ops.matern_periodic_build(*dev(x, x, le, lp, pe, os_), nu).cpu()[0]
    ref = matern_periodic_ref(*[a.double() for a in (x, x, le, lp, pe, os_)], nu)[0]
    assert bool(torch.isfinite(K).all())
    tol = dict(rtol=4e-13, atol=1e-300) if dt == F64 else dict(rtol=4e-5, atol=1e-37)    # ceilings 1e-10, 1.1e-4
    assert measured(f'matern_periodic nu={nu} {dt} distance range', K, ref, **tol)
    assert bool((K[0, -8:] == 0).all())                                        # the far tail of this very line
    far = torch.tensor([[0.0], [1e6], [-1e6], [7e5]], dtype=dt)
    Kf = ops.matern_periodic_build(*dev(far, far, le, lp, pe, os_), nu).cpu()[0]
    assert torch.equal(torch.diagonal(Kf), torch.ones(4, dtype=dt))
    off = Kf[~torch.eye(4, dtype=torch.bool)]
    assert not torch.isnan(off).any() and bool((off == 0).all()), Kf
    xn = x.clone()
    xn[7, 0] = float('nan')
    Kn = ops.matern_periodic_build(*dev(xn, xn, le, lp, pe, os_), nu).cpu()[0]
    bad = torch.zeros(n, n, dtype=torch.bool)
    bad[7, :] = True
    bad[:, 7] = True
    assert bool(torch.isnan(Kn[bad]).all()) and torch.equal(Kn[~bad], K[~bad])
    # and in the backward: the NaN row reaches x1[7] only, the NaN column x2[7] only
    G = torch.ones(1, n, n, dtype=dt).cuda()
    g1, g2, *_ = ops.matern_periodic_build_bwd(*dev(xn, x, le, lp, pe, os_), nu, G)
    keep = torch.arange(n) != 7
    assert bool(torch.isnan(g1[0, 7]).all()) and bool(torch.isfinite(g1[0, keep]).all())
    g1, g2, *_ = ops.matern_periodic_build_bwd(*dev(x, xn, le, lp, pe, os_), nu, G)
    assert bool(torch.isnan(g2[0, 7]).all()) and bool(torch.isfinite(g2[0, keep]).all())


# ------------------------------------------------------------------------------------------ kernel classes
@pytest.mark.parametrize('dt', [F64, F32], ids=['f64', 'f32'])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('order', ['matern_first', 'periodic_first'])
def test_scale_of_matern_times_periodic_is_one_fused_launch(ops, monkeypatch, dt, nu, order):
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, ScaleKernel
    g = _g(23)
    x = torch.randn(131, 3, generator=g, dtype=F64).to(dt).cuda()
    x2 = torch.randn(131, 3, generator=g, dtype=F64).to(dt).cuda()
    env, per = MaternKernel(nu=nu, active_dims=(0)), PeriodicKernel(active_dims=(0))
    kern = ScaleKernel(env * per if order == 'matern_first' else per * env, active_dims=0).to(dt).cuda()
    with torch.no_grad():
        env.raw_lengthscale.fill_(0.8)
        per.raw_lengthscale.fill_(0.3)
        per.raw_period_length.fill_(0.6)
        kern.raw_outputscale.fill_(0.4)
    calls = {'fused': 0, 'matern': 0}
    fused, plain = ops.matern_periodic_kernel, ops.matern_kernel

    def count(key, fn):
        def wrapped(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapped
    monkeypatch.setattr(ops, 'matern_periodic_kernel', count('fused', fused))
    monkeypatch.setattr(ops, 'matern_kernel', count('matern', plain))
    with torch.no_grad():
        K = kern(x, x2).evaluate()
    assert calls == {'fused': 1, 'matern': 0}
    t1, t2 = x[:, :1].contiguous(), x2[:, :1].contiguous()
    one = torch.ones(1, dtype=dt, device='cuda')
    with torch.no_grad():
        le, lp, pe = env.lengthscale.reshape(1, 1), per.lengthscale.reshape(1), per.period_length.reshape(1)
        want = ops.matern_build(t1, t2, le, one, nu)[0] * ops.rbf_periodic_build(t1, t2, None, lp, pe, None)[0] * \
            kern.outputscale
        ok = measured(f'ScaleKernel(Matern * Periodic) nu={nu} {dt} {order} vs separate builds', K, want, **_tol(dt))
        d = kern(x, x2, diag=True)
        assert d.shape == (131,)
        ok = measured(f'ScaleKernel(Matern * Periodic) nu={nu} {dt} {order} diag=True', d, torch.diagonal(K), **_tol(dt)) and ok
        # PeriodicKernel's own diag branch with the envelope handed in
        d2 = per.forward(t1, t2, diag=True, _outputscale=kern.outputscale, _rbf=env)
        ok = measured(f'PeriodicKernel.forward(diag, _rbf=Matern) nu={nu} {dt}', d2, torch.diagonal(K), **_tol(dt)) and ok
    assert ok and calls == {'fused': 1, 'matern': 0}                          # the diag paths are elementwise torch


def test_default_temporal_kernel_is_the_rbf_periodic_launch_it_was(ops):
    from models.spatio_temporal_models import _temporal_kernel
    g = _g(4)
    x = torch.randn(215, 3, generator=g, dtype=F64).cuda()
    kern = _temporal_kernel().double().cuda()
    with torch.no_grad():
        K = kern(x).evaluate()
        env, per = kern.base_kernel.kernels
        t = x[:, :1]
        direct = ops.rbf_periodic_kernel(t, t, env.lengthscale.reshape(1, 1), per.lengthscale.reshape(1),
                                         per.period_length.reshape(1), kern.outputscale.reshape(1))[0]
    assert torch.equal(K, direct)


# ------------------------------------------------------------------------------------------ model
def test_stationary_spatiotemporal_exact_gp_with_a_matern_temporal_envelope():
    """SpatioTemporal_Stationary(temporal_nu=1.5), float64, on the 215-point uib subset (172 train): MLL, every parameter
    gradient and the predictive mean and variance at the 43 held-out points against a dense float64 torch GP built from
    the restatement plus the oracle's rbf_ard (bounds: test_stationary_spatiotemporal_exact_gp_matches_oracle)."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nsgp.gp as gpytorch
    from models.spatio_temporal_models import SpatioTemporal_Stationary
    from oracle import kernels
    from oracle.exact import mvn_log_prob
    from test_gpu_spatiotemporal import _model_params, _uib_subset
    nu = 1.5
    xtr, ytr, xte, yte = _uib_subset()
    assert xtr.shape == (172, 3) and xte.shape == (43, 3)
    lik = gpytorch.likelihoods.GaussianLikelihood()
    model = SpatioTemporal_Stationary(xtr, ytr, lik, temporal_nu=nu).double().cuda()
    g = _g(5)
    with torch.no_grad():
        for p_ in model.parameters():
            p_.add_(0.3 * torch.randn(p_.shape, generator=g, dtype=F64).to(p_))
    model.train(); lik.train()
    mll = gpytorch.mlls.ExactMarginalLogLikelihood(lik, model)
    val = mll(model(model.train_inputs[0]), model.train_targets)
    val.backward()
    raw, leaves, p, noise = _model_params(model)

    def kern(a, b):
        one = lambda v: v.reshape(1)                                                # noqa: E731
        kt = matern_periodic_ref(a[:, 0:1], b[:, 0:1], p['ls_t'].reshape(1, 1), one(p['ls_p']), one(p['period']),
                                 one(p['os_t']), nu)[0]
        return kt + p['os_s'] * kernels.rbf_ard(a[:, 1:3], b[:, 1:3], p['ls_s'].reshape(1, 2))
    n = xtr.shape[0]
    ref = mvn_log_prob(ytr, torch.zeros_like(ytr), kern(xtr, xtr) + noise * torch.eye(n, dtype=F64)) / n
    ref.backward()
    # ceilings 1e-9 / 1e-10 (MLL), 1e-6 / 1e-8 (gradients), 1e-7 / 1e-8 (predictions); measured worst 1.2e-3, 2.8e-6 and
    # 1.8e-5 of them
    ratio = abs(float(val) - float(ref)) / (4e-12 * abs(float(ref)) + 4e-13)
    print(f'[measured] SpatioTemporal_Stationary(temporal_nu=1.5) MLL {float(val):.12g} vs {float(ref):.12g}: '
          f'worst diff/(atol + rtol|ref|) = {ratio:.3g} at rtol 4e-12 atol 4e-13')
    ok = ratio < 1.0
    for k, v in raw.items():
        ok = measured(f'SpatioTemporal_Stationary(temporal_nu=1.5) grad {k}', v.grad.reshape(-1), leaves[k].grad.reshape(-1),
                      rtol=1e-11, atol=1e-13) and ok
    model.eval(); lik.eval()
    with torch.no_grad():
        pred = lik(model(xte.cuda()))
        Kxx = kern(xtr, xtr) + noise * torch.eye(n, dtype=F64)
        Ksx = kern(xte, xtr)
        m_ref = Ksx @ torch.linalg.solve(Kxx, ytr)
        v_ref = torch.diagonal(kern(xte, xte) - Ksx @ torch.linalg.solve(Kxx, Ksx.T)) + noise
        ok = measured('SpatioTemporal_Stationary(temporal_nu=1.5) predictive mean', pred.loc, m_ref, rtol=6e-12, atol=6e-13) and ok
        ok = measured('SpatioTemporal_Stationary(temporal_nu=1.5) predictive variance',
                      torch.diagonal(pred.covariance_matrix), v_ref, rtol=6e-12, atol=6e-13) and ok
    assert ok
