"""Every row of the tables of tests/test_svgp_reduction_cases_cpu.py on the GPU: the SVGP / DSVI reductions of csrc/svgp.hip
and the small kernels of csrc/misc.hip at every loop and launch boundary.

How a result is judged is stated (and its preconditions asserted) in that file: `torch.equal` against the float64 reference
on integer data wherever every term is a product or sum of the inputs; the worst-case bound (N + c) u sum |t_i| (`red_tol`)
with spiked inputs where a term holds a log, a division or a square root; c u |pieces| element-wise, c counted beside the
assert; bit-equality between the paths of the fused Adam.  Achieved error / bound is printed through conftest.measured (run
with -s).  Whatever the C ABI writes lies inside a sentinel-filled buffer whose guards must survive the call.
"""
import ctypes
import math

import pytest
import torch

from conftest import measured
from test_svgp_reduction_cases_cpu import (
    ADAM_CASES, ADAM_STEPS, C_GAUSS, C_KL, COLSTATS_CASES, DTYPES, FIN_BASE_ADD, FIN_BATCH, FIN_D, FINALIZE_RUNS, GAUSS_CASES,
    KL_CASES, MISC_N, OBJ_CASES, OBJ_MAX_GROUPS, PLAIN_ROWDOT_CASES, ROWDOT_CASES, SAMPLE_CASES, U, colstats_inputs,
    colstats_reference, finalize_inputs, finalize_reference, gauss_blocks, gauss_inputs, gauss_terms, gen, kl_blocks,
    kl_grad_reference, kl_inputs, kl_reference, kl_terms_count, normal32, obj_inputs, obj_reference, obj_terms_count, red_tol,
    rowdot_inputs, rowdot_reference, sample_inputs, sample_reference)

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
PAD = 64                                                  # guard elements on either side (a multiple of 16 bytes)
BOTH = ['f32', 'f64']


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def dev(t, dt, off=0):
    """float64 CPU tensor -> the case's dtype on the device, unchanged in value; off: start that many elements into a larger
    buffer (a pointer that is not 16-byte aligned)."""
    td = t.to(DTYPES[dt] if isinstance(dt, str) else dt).contiguous()
    assert torch.equal(torch.nan_to_num(td.double()), torch.nan_to_num(t.double())), 'input is not a number of the dtype'
    if not off:
        return td.cuda()
    buf = torch.zeros(td.numel() + off + 3, dtype=td.dtype, device='cuda')
    view = buf[off:off + td.numel()].view(td.shape)
    view.copy_(td)
    assert view.data_ptr() % 16 != 0
    return view


class Guard:
    """Outputs and workspaces as windows of sentinel-filled buffers."""

    def __init__(self):
        self.items = []

    def out(self, shape, dtype, off=0, init=None):
        numel = math.prod(shape)
        buf = torch.full((numel + 2 * PAD + off,), SENTINEL, dtype=dtype, device='cuda')
        view = buf[PAD + off:PAD + off + numel].view(shape)
        if init is not None:
            view.copy_(init)
        self.items.append((buf, PAD + off, numel))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for k, (buf, lo, numel) in enumerate(self.items):
            assert bool((buf[:lo] == SENTINEL).all()) and bool((buf[lo + numel:] == SENTINEL).all()), \
                f'{what}: output {k} was written outside its {numel} elements'


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def within(name, got, ref, tol):
    """|got - ref| <= tol, element-wise (tol: a number or a tensor); prints the worst |got - ref| / tol.  Where the bound is 0
    the value must be equal."""
    got = got.detach().double().cpu().reshape(-1)
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
    tol = torch.as_tensor(tol, dtype=torch.float64).reshape(-1).expand_as(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    zero = tol == 0
    if bool(zero.any()) and not torch.equal(got[zero], ref[zero]):
        return False
    ratio = torch.where(zero, torch.zeros_like(ref), (got - ref) / torch.where(zero, torch.ones_like(tol), tol))
    return measured(name, ratio, torch.zeros_like(ratio), 0.0, 1.0)


def same(got, want):
    return torch.equal(got.detach().double().cpu().reshape(want.shape), want)


def _cid(c):
    return getattr(c, 'name', None) or '-'.join(str(f) for f in c)


# ---------------------------------------------------------------------------------------------------------------------------
# Gaussian expected log-likelihood
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_run(ops, P, dt, form, need_noise):
    y, mu, v = dev(P['y'], dt), dev(P['mu'], dt).requires_grad_(), dev(P['v'], dt).requires_grad_()
    noise = torch.tensor([P['noise']], dtype=DTYPES[dt], device='cuda', requires_grad=need_noise)
    if form == 'vec':
        out = ops.GaussEllFn.apply(y, mu, v, noise, P['scale'])
        out.backward(dev(P['gout'], dt))
        go = P['gout'].unsqueeze(1)
    else:
        out = ops.GaussEllTotalFn.apply(y, mu, v, noise, P['scale'])
        (out * P['up']).backward()
        go = torch.full((mu.shape[0], 1), P['up'], dtype=torch.float64)
    return out, mu.grad, v.grad, noise.grad, go


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', GAUSS_CASES, ids=_cid)
def test_gauss_ell_value_and_gradients_within_the_summation_bound(ops, case, dt):
    n, S = case
    P = gauss_inputs(case, 'bound')
    t, a, gt, ga = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
    sc, u, tag = P['scale'], U[dt], f'gauss {n}x{S} {dt}'
    for form, need_noise in (('vec', True), ('total', True), ('vec', False), ('total', False)):
        out, gmu, gv, gn, go = _gauss_run(ops, P, dt, form, need_noise)
        if form == 'vec':                                 # S sums of n terms
            assert within(f'{tag} vec', out, sc * t.sum(1), red_tol(n, C_GAUSS, dt, abs(sc) * a.sum(1)))
        else:                                             # one sum of S n terms
            assert within(f'{tag} total', out, sc * t.sum(), red_tol(S * n, C_GAUSS, dt, abs(sc) * float(a.sum())))
        ref_mu = go * sc * (P['y'] - P['mu']) / P['noise']
        ref_v = (-0.5 * go * sc / P['noise']).expand(S, n)
        # gmu = (gout scale) (y - mu) (1 / s2): 5 roundings; gv = -1/2 (gout scale) (1 / s2): 3 roundings
        assert within(f'{tag} {form} gmu', gmu, ref_mu, 5 * u * ref_mu.abs())
        assert within(f'{tag} {form} gv', gv, ref_v, 3 * u * ref_v.abs())
        if need_noise:                                    # scale sum_s gout_s sum_i 1/2 (e / s2^2 - 1 / s2): <= C_GAUSS roundings
            assert within(f'{tag} {form} gnoise', gn, sc * (go * gt).sum(),
                          red_tol(S * n, C_GAUSS, dt, abs(sc) * float((go.abs() * ga).sum())))
        else:
            assert gn is None


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', GAUSS_CASES, ids=_cid)
def test_gauss_ell_gradients_are_exact_on_integer_data_with_unit_noise(ops, case, dt):
    """noise = 1: the noise gradient's terms are 1/2 (e - 1) gout, and gmu, gv are products of the inputs."""
    n, S = case
    P = gauss_inputs(case, 'int')
    _, _, gt, _ = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
    for form in ('vec', 'total'):
        _, gmu, gv, gn, go = _gauss_run(ops, P, dt, form, True)
        assert same(gn, P['scale'] * (go * gt).sum().reshape(1)), (form, float(gn), float(P['scale'] * (go * gt).sum()))
        assert same(gmu, go * P['scale'] * (P['y'] - P['mu']))
        assert same(gv, (-0.5 * go * P['scale']).expand(S, n).contiguous())


# ---------------------------------------------------------------------------------------------------------------------------
# whitened KL
# ---------------------------------------------------------------------------------------------------------------------------
def _kl_grads_ok(tag, m, L, P, go, dt, c_m, c_l):
    """gm within c_m u |ref|, gLq within c_l u |go| (|l| + |1 / l|) below and on the diagonal, exactly 0 above it."""
    M = P['m'].shape[1]
    rm, rl, mag = kl_grad_reference(P['m'], P['L'], go)
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    gL = L.grad.detach().cpu().double().reshape(rl.shape)
    assert torch.equal(gL[:, upper], torch.zeros_like(gL[:, upper])), f'{tag}: gLq is not exactly 0 above the diagonal'
    ok = within(f'{tag} gm', m.grad, rm, c_m * U[dt] * rm.abs())
    return within(f'{tag} gLq', gL[:, ~upper], rl[:, ~upper], c_l * U[dt] * mag[:, ~upper]) and ok


def _kl_leaves(P, dt):
    return dev(P['m'], dt).requires_grad_(), dev(P['L_given'], dt).requires_grad_()


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', KL_CASES, ids=_cid)
def test_kl_value_and_gradients_within_the_summation_bound(ops, case, dt):
    M, batch = case
    P = kl_inputs(case, 'bound')
    ref, ab = kl_reference(P['m'], P['L'])
    N, tag = kl_terms_count(M), f'kl {M}x{batch} {dt}'
    m, L = _kl_leaves(P, dt)
    assert within(f'{tag} per batch', ops.kl_whitened(m.detach(), L.detach()), ref, red_tol(N, C_KL, dt, ab))
    out = ops.KlWhitenedFn.apply(m, L)
    assert within(f'{tag} sum', out, ref.sum(), red_tol(batch * N, C_KL, dt, float(ab.sum())))
    (out * P['up']).backward()
    # kernel with gout = 1, then torch's * g: gm 1 rounding, gLq 1 / l, l - 1 / l, * g: 3
    assert _kl_grads_ok(f'{tag} sum', m, L, P, P['up'], dt, 1, 3)
    for addin in (None, P['addin']):
        m, L = _kl_leaves(P, dt)
        ad = None if addin is None else torch.tensor(addin, dtype=DTYPES[dt], device='cuda', requires_grad=True)
        out = ops.KlWhitenedTotalFn.apply(m, L, P['scale'], ad)
        want = P['scale'] * ref.sum() + (addin or 0.0)
        assert within(f'{tag} total addin={addin}', out, want,
                      red_tol(batch * N, C_KL, dt, abs(P['scale']) * float(ab.sum()) + abs(addin or 0.0)))
        (out * P['up']).backward()
        # gout = scale * g on the device (1 rounding), then gm: * m (2 in all); gLq: 1 / l, l - 1 / l, * gout (4 in all)
        assert _kl_grads_ok(f'{tag} total', m, L, P, P['scale'] * P['up'], dt, 2, 4)
        if ad is not None:
            assert float(ad.grad) == P['up']


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', KL_CASES, ids=_cid)
def test_kl_is_exact_on_integer_data_with_unit_diagonal(ops, case, dt):
    """Every diagonal entry +-1: log |l| = 0 and l - 1 / l = 0 exactly, everything else is sums of products of the inputs."""
    M, batch = case
    P = kl_inputs(case, 'int')
    ref, _ = kl_reference(P['m'], P['L'])
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    m, L = _kl_leaves(P, dt)
    assert same(ops.kl_whitened(m.detach(), L.detach()), ref)
    out = ops.KlWhitenedFn.apply(m, L)
    assert same(out, ref.sum())
    (out * P['up']).backward()
    rm, rl, _ = kl_grad_reference(P['m'], P['L'], P['up'])
    assert same(m.grad, rm) and same(torch.nan_to_num(L.grad, nan=7.0), rl)
    for addin in (None, P['addin']):
        m, L = _kl_leaves(P, dt)
        ad = None if addin is None else torch.tensor(addin, dtype=DTYPES[dt], device='cuda')
        out = ops.KlWhitenedTotalFn.apply(m, L, P['scale'], ad)
        assert same(out, P['scale'] * ref.sum() + (addin or 0.0)), (float(out), float(P['scale'] * ref.sum() + (addin or 0.0)))
        (out * P['up']).backward()
        rm, rl, _ = kl_grad_reference(P['m'], P['L'], P['scale'] * P['up'])
        assert same(m.grad, rm) and same(torch.nan_to_num(L.grad, nan=7.0), rl)
        assert bool((L.grad[:, upper] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# fused DSVI objective against the float64 closed form
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', OBJ_CASES, ids=_cid)
def test_dsvi_objective_matches_the_closed_form(ops, case, dt):
    P = obj_inputs(case)
    val, ab, _ = obj_reference(P)
    u, tag, S, n, M = U[dt], f'objective {case.name} {dt}', case.S, case.n, case.M
    y, mu, v = dev(P['y'], dt), dev(P['mu'], dt).requires_grad_(), dev(P['v'], dt).requires_grad_()
    noise = torch.tensor([P['noise']], dtype=DTYPES[dt], device='cuda', requires_grad=case.noise_grad)
    leaves = []
    for (m, _, Lg), b in zip(P['groups'], case.batches):
        if case.squeeze and b == 1:
            m, Lg = m[0], Lg[0]                           # handed over as (M,) / (M, M)
        leaves += [dev(m, dt).requires_grad_(), dev(Lg, dt).requires_grad_()]
    out = ops.DsviObjectiveFn.apply(y, mu, v, noise, P['ell_scale'], P['kl_scale'], *leaves)
    assert out.shape == ()
    assert within(f'{tag} value', out, val, red_tol(obj_terms_count(case), C_GAUSS + C_KL, dt, ab))
    (out * case.up).backward()
    _, _, gt, ga = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
    ce = case.up * P['ell_scale']
    ref_mu, ref_v = ce * (P['y'] - P['mu']) / P['noise'], torch.full((S, n), -0.5 * ce / P['noise'], dtype=torch.float64)
    # gmu = (up ell_scale) (y - mu) (1 / s2): 5 roundings; gv = -1/2 (up ell_scale) (1 / s2): 3
    assert within(f'{tag} gmu', mu.grad, ref_mu, 5 * u * ref_mu.abs())
    assert within(f'{tag} gv', v.grad, ref_v, 3 * u * ref_v.abs())
    if case.noise_grad:
        assert within(f'{tag} gnoise', noise.grad, ce * gt.sum(), red_tol(S * n, C_GAUSS, dt, abs(ce) * float(ga.sum())))
    else:
        assert noise.grad is None
    for k, (m, L, _) in enumerate(P['groups']):
        lm, lL = leaves[2 * k], leaves[2 * k + 1]
        assert lm.grad.shape == lm.shape and lL.grad.shape == lL.shape
        # go = up kl_scale (1 rounding); gm = go m (2 in all); gLq = go (l - 1 / l) (4 in all)
        assert _kl_grads_ok(f'{tag} group {k}', lm, lL, dict(m=m, L=L), case.up * P['kl_scale'], dt, 2, 4)


def test_dsvi_objective_rejects_more_groups_than_the_kernel_holds(ops):
    from nsgp._lib import BackendError
    y, mu = torch.zeros(4, device='cuda'), torch.zeros(1, 4, device='cuda')
    v, noise = torch.ones(1, 4, device='cuda'), torch.ones(1, device='cuda')
    mL = []
    for _ in range(OBJ_MAX_GROUPS + 1):
        mL += [torch.zeros(2, device='cuda'), torch.eye(2, device='cuda')]
    assert float(ops.DsviObjectiveFn.apply(y, mu, v, noise, 1.0, 1.0, *mL[:2 * OBJ_MAX_GROUPS])) < 0.0
    with pytest.raises(BackendError):
        ops.DsviObjectiveFn.apply(y, mu, v, noise, 1.0, 1.0, *mL)


# ---------------------------------------------------------------------------------------------------------------------------
# the reductions through the C ABI: exactly-sized workspaces and outputs between guards
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', BOTH)
def test_reductions_stay_inside_their_workspaces_and_outputs(ops, dt):
    """The likelihood (total form: S nblk partials, one more for the backward) and the KL (batch nblk partials) at their
    largest rows, with a workspace of exactly the size the entry point checks for; same bits as through nsgp.ops."""
    from nsgp import _lib
    tdt, es = DTYPES[dt], 4 if dt == 'f32' else 8
    case = GAUSS_CASES[-1]
    n, S = case
    P = gauss_inputs(case, 'bound')
    want, gmu_w, gv_w, gn_w, _ = _gauss_run(ops, P, dt, 'total', True)
    y, mu, v = dev(P['y'], dt), dev(P['mu'], dt), dev(P['v'], dt)
    noise, up = torch.tensor([P['noise']], dtype=tdt, device='cuda'), torch.tensor([P['up']], dtype=tdt, device='cuda')
    G = Guard()
    nparts = S * gauss_blocks(n)
    out, ws = G.out((1,), tdt), G.out((nparts,), tdt)
    _lib.call(f'nsgp_gauss_ell_total_fwd_{dt}', _p(y), _p(mu), _p(v), _p(noise), S, n, P['scale'], _p(out), _p(ws), nparts * es,
              ops._stream())
    gmu, gv, gn, ws2 = G.out((S, n), tdt), G.out((S, n), tdt), G.out((1,), tdt), G.out((nparts + 1,), tdt)
    _lib.call(f'nsgp_gauss_ell_total_bwd_{dt}', _p(y), _p(mu), _p(v), _p(noise), S, n, P['scale'], _p(up), _p(gmu), _p(gv),
              _p(gn), _p(ws2), (nparts + 1) * es, ops._stream())
    G.check('gauss_ell_total')
    assert torch.equal(out.reshape(()), want.detach()) and torch.equal(gmu, gmu_w) and torch.equal(gv, gv_w)
    assert torch.equal(gn, gn_w)
    assert getattr(_lib.load(), f'nsgp_gauss_ell_total_fwd_{dt}')(_p(y), _p(mu), _p(v), _p(noise), S, n, P['scale'], _p(out),
                                                                  _p(ws), nparts * es - 1, ops._stream()) == -9

    case = KL_CASES[-1]
    M, batch = case
    P = kl_inputs(case, 'bound')
    m, L = dev(P['m'], dt), dev(P['L_given'], dt)
    ad, up = torch.tensor([P['addin']], dtype=tdt, device='cuda'), torch.tensor([P['up']], dtype=tdt, device='cuda')
    want = ops.KlWhitenedTotalFn.apply(m, L, P['scale'], ad)
    G = Guard()
    nparts = batch * kl_blocks(M)
    out, ws = G.out((1,), tdt), G.out((nparts,), tdt)
    _lib.call(f'nsgp_kl_whitened_total_acc_fwd_{dt}', _p(m), _p(L), batch, M, P['scale'], _p(ad), _p(out), _p(ws), nparts * es,
              ops._stream())
    gm, gL = G.out((batch, M), tdt), G.out((batch, M, M), tdt)
    _lib.call(f'nsgp_kl_whitened_total_bwd_{dt}', _p(m), _p(L), batch, M, P['scale'], _p(up), _p(gm), _p(gL), ops._stream())
    G.check('kl_whitened_total')
    assert torch.equal(out.reshape(()), want)
    rm, rl, mag = kl_grad_reference(P['m'], P['L'], P['scale'] * P['up'])
    assert within(f'kl abi {dt} gm', gm, rm, 2 * U[dt] * rm.abs()) and within(f'kl abi {dt} gLq', gL, rl, 4 * U[dt] * mag)


# ---------------------------------------------------------------------------------------------------------------------------
# rowdot_affine and rowdot through the C ABI (exact)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', ROWDOT_CASES, ids=_cid)
def test_rowdot_affine_is_exact_and_writes_nothing_else(ops, case, dt):
    from nsgp import _lib
    n, batch, M, D, shared, drop, off = case
    P = rowdot_inputs(n, batch, M, D, 'affine')
    R = rowdot_reference(P, shared)
    A, g = dev(P['A'], dt, int(off == 'A')), dev(P['g'], dt, int(off == 'g'))
    gv, x = dev(P['gv'], dt, int(off == 'gv')), dev(P['x'], dt)
    tdt, nb = DTYPES[dt], 1 if shared else batch
    G = Guard()
    got = dict(out=G.out((batch, M), tdt), out_gv=G.out((batch,), tdt), out_1=G.out((nb,), tdt), out_x=G.out((nb, D), tdt))
    _lib.call(f'nsgp_rowdot_affine_{dt}', _p(A), _p(g), None if drop == 'gv' else _p(gv), None if drop == 'out_x' else _p(x),
              n * D, D, shared, batch, M, n, _p(got['out']), _p(got['out_gv']), None if drop == 'out_x' else _p(got['out_x']),
              None if drop == 'out_1' else _p(got['out_1']), ops._stream())
    G.check(_cid(case))
    for name, want in R.items():
        if name == ('out_gv' if drop == 'gv' else drop):
            assert bool((got[name] == SENTINEL).all()), f'{name} is absent and was written'
        else:
            assert same(got[name], want), (name, got[name].cpu(), want)


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('n,off', PLAIN_ROWDOT_CASES, ids=lambda v: str(v))
def test_rowdot_is_exact_and_writes_nothing_else(ops, n, off, dt):
    from nsgp import _lib
    P = rowdot_inputs(n, 2, 3, 1, 'plain')
    A, g = dev(P['A'], dt, int(off == 'A')), dev(P['g'], dt, int(off == 'g'))
    G = Guard()
    out = G.out((2, 3), DTYPES[dt])
    _lib.call(f'nsgp_rowdot_{dt}', _p(A), _p(g), 2, 3, n, _p(out), ops._stream())
    G.check(f'rowdot {n} {off}')
    assert same(out, rowdot_reference(P, 0)['out'])


# ---------------------------------------------------------------------------------------------------------------------------
# colstats, colstats_bwd and the three finalize forms through the C ABI (exact)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', COLSTATS_CASES, ids=_cid)
def test_colstats_and_backward_are_exact_and_write_nothing_else(ops, case, dt):
    from nsgp import _lib
    M, n, b = case
    P = colstats_inputs(case)
    R = colstats_reference(P)
    D = {k: dev(t, dt) for k, t in P.items()}
    tdt = DTYPES[dt]
    G = Guard()
    got = dict(mean=G.out((b, n), tdt), var=G.out((b, n), tdt), Abar=G.out((b, M, n), tdt), C2=G.out((b, M, n), tdt),
               mbar=G.out((b, M), tdt))
    _lib.call(f'nsgp_svgp_colstats_{dt}', _p(D['A']), _p(D['C']), _p(D['m']), _p(D['base']), b, M, n, _p(got['mean']),
              _p(got['var']), ops._stream())
    _lib.call(f'nsgp_svgp_colstats_bwd_{dt}', _p(D['A']), _p(D['C']), _p(D['m']), _p(D['gmean']), _p(D['gvar']), b, M, n,
              _p(got['Abar']), _p(got['C2']), _p(got['mbar']), ops._stream())
    G.check(_cid(case))
    for name, want in R.items():
        assert same(got[name], want), name


@pytest.mark.parametrize('case,dt', FINALIZE_RUNS, ids=lambda v: v if isinstance(v, str) else _cid(v))
def test_colstats_finalize_forms_are_exact_and_write_nothing_else(ops, case, dt):
    from nsgp import _lib
    b, D, n, tiles = FIN_BATCH, FIN_D, case.n, case.tiles
    P = finalize_inputs(case)
    want_mean, want_var = finalize_reference(case, P)
    tdt = DTYPES[dt]
    pdt = torch.float64 if case.form == 'p64' else tdt
    parts = [dev(P[k], pdt) for k in ('pdot', 'psqA', 'psqC')]
    base, x = dev(P['base'], dt), dev(P['x'], dt)
    w = None if P['w'] is None else dev(P['w'], dt)
    c = None if P['c'] is None else dev(P['c'], dt)
    G = Guard()
    mean, var = G.out((b, n), tdt), G.out((b, n), tdt)
    if case.form == 'plain':
        _lib.call(f'nsgp_svgp_colstats_finalize_{dt}', *[_p(t) for t in parts], _p(base), b, tiles, n, _p(mean), _p(var),
                  ops._stream())
    else:
        name = 'nsgp_svgp_colstats_finalize_affine_' + ('p64_f32' if case.form == 'p64' else dt)
        _lib.call(name, *[_p(t) for t in parts], _p(base), FIN_BASE_ADD, b, tiles, n, _p(x), n * D, D, _p(w),
                  0 if case.shared else D, _p(c), 0 if case.shared else 1, _p(mean), _p(var), ops._stream())
    G.check(_cid(case))
    assert same(mean, want_mean), (mean.cpu(), want_mean)
    assert same(var, want_var), (var.cpu(), want_var)


# ---------------------------------------------------------------------------------------------------------------------------
# layer sampling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('case', SAMPLE_CASES, ids=_cid)
def test_sampling_forward_and_backward(ops, case, dt):
    from nsgp import _lib
    S, n, b, ns = case
    P = sample_inputs(case)
    R = sample_reference(P, ns)
    D = {k: dev(t, dt) for k, t in P.items()}
    tdt, u, tag = DTYPES[dt], U[dt], f'sample {_cid(case)} {dt}'
    G = Guard()
    h, gmean, gvar = G.out((S, n, b), tdt), G.out((b, ns, n), tdt), G.out((b, ns, n), tdt)
    _lib.call(f'nsgp_dgp_sample_fwd_{dt}', _p(D['mean']), _p(D['var']), _p(D['eps']), S, ns, n, b, _p(h), ops._stream())
    _lib.call(f'nsgp_dgp_sample_bwd_{dt}', _p(D['var']), _p(D['eps']), _p(D['gh']), S, ns, n, b, _p(gmean), _p(gvar),
              ops._stream())
    G.check(tag)
    # h = mean + sqrt(var) eps: sqrt, product, sum: 3 roundings of at most |mean| + |sqrt(var) eps|
    assert within(f'{tag} h', h, R['h'], 3 * u * R['h_mag'])
    assert same(gmean, R['gmean'])                        # sums of the integer gh
    # gvar = sum_s gh eps (1/2 / sqrt(var)): sqrt, quotient, two products per term; S terms (ns = 1) or one
    assert within(f'{tag} gvar', gvar, R['gvar'], red_tol(S if ns == 1 else 1, 4, dt, R['gvar_abs']))


# ---------------------------------------------------------------------------------------------------------------------------
# fused Adam: the vector and the scalar branch, the host and the device step count
# ---------------------------------------------------------------------------------------------------------------------------
ADAM_HP = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8)


def _adam_run(ops, n, align, grad_scale, device_step, data):
    """ADAM_STEPS steps on buffers between guards; returns (p, m, v) on the CPU."""
    from nsgp import _lib
    offs = dict(aligned=(0, 0, 0, 0), all_off=(1, 1, 1, 1), g_off=(0, 1, 0, 0))[align]
    G = Guard()
    p = G.out((n,), torch.float32, offs[0], data['p0'])
    g = G.out((n,), torch.float32, offs[1])
    m = G.out((n,), torch.float32, offs[2], torch.zeros(n))
    v = G.out((n,), torch.float32, offs[3], torch.zeros(n))
    assert [t.data_ptr() % 16 != 0 for t in (p, g, m, v)] == [bool(o) for o in offs]
    for step in range(1, ADAM_STEPS + 1):
        g.copy_(data['g'][step - 1])
        sd = torch.tensor([step], dtype=torch.int64, device='cuda') if device_step else None
        # with a device-side count the host count is 0: bias corrections taken from it would be those of step 1
        _lib.call('nsgp_adam_step_f32', _p(p), _p(g), _p(m), _p(v), n, ADAM_HP['lr'], ADAM_HP['b1'], ADAM_HP['b2'],
                  ADAM_HP['eps'], 0 if device_step else step, _p(sd), grad_scale, ops._stream())
    G.check(f'adam {n} {align}')
    return p.cpu(), m.cpu(), v.cpu()


@pytest.mark.parametrize('case', ADAM_CASES, ids=_cid)
def test_adam_paths_agree_bit_for_bit_and_match_the_oracle(ops, case):
    from oracle import svgp
    n, align, gs = case
    g = gen(f'adam-{n}')
    data = dict(p0=normal32((n,), g).float(), g=[normal32((n,), g).float() for _ in range(ADAM_STEPS)])
    base = _adam_run(ops, n, 'aligned', gs, False, data)
    for device_step in (False, True):
        got = _adam_run(ops, n, align, gs, device_step, data)
        for name, a, b in zip('pmv', got, base):
            assert torch.equal(a, b), f'{name} differs from the aligned host-step run (device_step={device_step}): ' \
                f'{int((a != b).sum())} of {n}, first at {int((a != b).nonzero()[0])}'
    want, state = [data['p0'].double()], {}
    for step in range(ADAM_STEPS):
        want = svgp.adam_step(want, [data['g'][step].double() * gs], state, lr=ADAM_HP['lr'], betas=(ADAM_HP['b1'], ADAM_HP['b2']),
                              eps=ADAM_HP['eps'])
    assert measured(f'adam {_cid(case)} vs oracle', base[0], want[0], 1e-5, 1e-6)     # test_fused_adam_matches_oracle's


# ---------------------------------------------------------------------------------------------------------------------------
# cast, phi_sym, scale_diag with leading dimensions beyond the row length
# ---------------------------------------------------------------------------------------------------------------------------
def _windows(n, ld, sP, batch):
    """Index (batch, n, n) of the matrices inside a flat buffer of batch * sP elements."""
    b = torch.arange(batch).reshape(-1, 1, 1) * sP
    return b + torch.arange(n).reshape(1, -1, 1) * ld + torch.arange(n).reshape(1, 1, -1)


@pytest.mark.parametrize('n', MISC_N)
@pytest.mark.parametrize('src', BOTH)
def test_cast_with_padded_rows_writes_only_the_columns(ops, n, src):
    from nsgp import _lib
    dst = 'f64' if src == 'f32' else 'f32'
    rows, lds, ldd = 3, n + 3, n + 5
    g = gen(f'cast-{n}-{src}')
    val = torch.randn(rows, n, generator=g, dtype=DTYPES[src])
    S = torch.full((rows, lds), float('nan'), dtype=DTYPES[src])
    S[:, :n] = val
    G = Guard()
    out, Sd = G.out((rows, ldd), DTYPES[dst]), S.cuda()
    _lib.call(f'nsgp_cast_{src}_to_{dst}', _p(Sd), lds, _p(out), ldd, rows, n, ops._stream())
    G.check(f'cast {n}')
    assert torch.equal(out[:, :n].cpu(), val.to(DTYPES[dst]))                          # round to nearest even, as torch
    assert bool((out[:, n:] == SENTINEL).all())


@pytest.mark.parametrize('dt', BOTH)
@pytest.mark.parametrize('n', MISC_N)
def test_phi_sym_and_scale_diag_with_padded_rows_and_batch_gaps(ops, n, dt):
    from nsgp import _lib
    tdt, batch, ld = DTYPES[dt], 2, n + 3
    sP = n * ld + 7
    idx = _windows(n, ld, sP, batch)
    g = gen(f'phi-{n}-{dt}')
    vals = torch.randn(batch, n, n, generator=g, dtype=tdt)
    lower = torch.tril(torch.ones(n, n, dtype=torch.bool))
    P = torch.full((batch * sP,), float('nan'), dtype=tdt)
    P[idx[:, lower]] = vals[:, lower]                    # the strict upper triangle and all padding stay NaN: never read
    G = Guard()
    S, Pd = G.out((batch * sP,), tdt), P.cuda()
    _lib.call(f'nsgp_chol_bwd_phi_sym_{dt}', _p(Pd), _p(S), n, ld, sP, batch, ops._stream())
    G.check(f'phi_sym {n}')
    want = torch.full((batch * sP,), SENTINEL, dtype=tdt)
    sym = torch.where(lower, vals, vals.transpose(1, 2))
    want[idx] = sym
    assert torch.equal(S.cpu(), want)

    Q0 = torch.full((batch * sP,), SENTINEL, dtype=tdt)
    Q0[idx] = vals
    G = Guard()
    Q = G.out((batch * sP,), tdt, 0, Q0)
    _lib.call(f'nsgp_scale_diag_{dt}', _p(Q), n, ld, sP, batch, 1.5, ops._stream())
    G.check(f'scale_diag {n}')
    eye = torch.eye(n, dtype=torch.bool)
    Q0[idx[:, eye]] = vals[:, eye] * 1.5                  # one correctly rounded product
    assert torch.equal(Q.cpu(), Q0)
