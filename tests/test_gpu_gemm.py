"""Every row of GEMM_CASES (tests/test_gemm_plan_cpu.py) on the GPU, exactly.

Exact pass: operands hold small integers (A in -3..4, B in -3..4 from a different stream, C0 in -8..8), so the float64
product of the same operands, masked to the declared triangles, is THE answer for float32 and float64 alike, whatever the
summation order, split or tile (the bound is stated and asserted in test_gemm_plan_cpu.py): `torch.equal`, no tolerance.  A
GEMM bug is a dropped, doubled or misplaced term or tile, not a rounding error.  The triangle an operand flag declares zero
holds NaN, the parent buffer around an operand view holds NaN, C holds NaN where beta == 0.

Every row runs twice: through ops.gemm, and through the C ABI with C a window (ldc = N + 3 or N + 4, guard rows, guard
between batch elements) of a sentinel-filled buffer and a guarded split-K workspace; nothing outside the M x N windows and
the workspace proper may change.

What the header promises for C_LOWER: beta == 0 without C_NOFILL: the strict upper triangle is exactly 0; with C_NOFILL it is
unspecified (only the lower triangle is compared); beta != 0: the strict upper triangle keeps C0, bit for bit.

Rounding pass: one row per plan key on seeded normal data against the float64 product of the rounded operands, held
elementwise to |got - ref| <= (K + ksplit + 4) u (|alpha| |op(A)| |op(B)| + |beta| |C0|), u = eps / 2: the standard bound of a
sum of K products in any order, plus the slab additions and the alpha / beta step.  It follows from the arithmetic, it is not
measured; the achieved ratio is printed (run with -s)."""
import ctypes
import zlib

import pytest
import torch

from test_gemm_plan_cpu import (AL, AU, BL, BU, CL, NF, HD, DTYPES, GEMM_CASES, build_operands, plan_key, stored_shapes)

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
WS_GUARD = 4096


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _tri_zero_mask(rows, cols, lower):
    """True where a matrix declared lower (upper) triangular is declared zero."""
    r = torch.arange(rows).unsqueeze(1)
    c = torch.arange(cols).unsqueeze(0)
    return (c > r) if lower else (c < r)


def _draw(shape, gen, dt, kind, lo, hi):
    if kind == 'int':
        return torch.randint(lo, hi + 1, shape, generator=gen).to(dt)
    return torch.randn(shape, generator=gen, dtype=dt)


def _problem(case, kind):
    """Clean operands (CPU, the row's dtype), the operands as handed to the kernel (NaN in the declared-zero triangles) and
    C0.  Returns dict with opA, opB (float64, masked to zero: (lead, M, K), (lead, K, N)), fill(), C0."""
    dt = DTYPES[case.dt]
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    sa, sb = stored_shapes(case)
    dense = {'A': _draw(sa, gen, dt, kind, -3, 4), 'B': _draw(sb, gen, dt, kind, -3, 4)}
    for which, spec in (('A', case.va), ('B', case.vb)):
        if ':' in spec:                                   # one matrix for the whole batch
            dense[which] = dense[which][:1].expand_as(dense[which]).contiguous()
    opA = dense['A'].transpose(-1, -2) if case.ta else dense['A']
    opB = dense['B'].transpose(-1, -2) if case.tb else dense['B']
    zA = zB = None
    if case.flags & (AL | AU):
        zA = _tri_zero_mask(case.M, case.K, bool(case.flags & AL))
    if case.flags & (BL | BU):                            # B_LOWER: op(B)(k, n) == 0 for n > k
        zB = _tri_zero_mask(case.K, case.N, bool(case.flags & BL))
    nan = float('nan')
    given = {}
    for which, op, z, t in (('A', opA, zA, case.ta), ('B', opB, zB, case.tb)):
        g = op.clone()
        if z is not None:
            g = torch.where(z, torch.full_like(g, nan), g)
        given[which] = (g.transpose(-1, -2) if t else g).contiguous()
    clean = lambda op, z: (op if z is None else torch.where(z, torch.zeros_like(op), op)).double()   # noqa: E731
    lead = (case.nb,) if case.nb else ()
    C0 = _draw(lead + (case.M, case.N), gen, dt, kind, -8, 8) if case.beta != 0 else \
        torch.full(lead + (case.M, case.N), nan, dtype=dt)
    return dict(opA=clean(opA, zA), opB=clean(opB, zB), C0=C0,
                fill=lambda shape, which: given[which].cuda())


def _expected(case, P, need_mag=False):
    """(expected float64 output, comparison mask, elementwise magnitude |alpha||A||B| + |beta||C0| for the rounding bound)."""
    prod = P['opA'] @ P['opB']
    mag = abs(case.alpha) * (P['opA'].abs() @ P['opB'].abs()) if need_mag else torch.zeros_like(prod)
    val = case.alpha * prod
    if case.flags & HD:
        d = torch.diagonal(val, dim1=-2, dim2=-1)
        d.mul_(0.5)
    if case.beta != 0:
        val = val + case.beta * P['C0'].double()
        mag = mag + abs(case.beta) * P['C0'].double().abs()
    mask = torch.ones(val.shape, dtype=torch.bool)
    if case.flags & CL:
        up = _tri_zero_mask(case.M, case.N, True).expand_as(val)
        if case.beta != 0:
            val = torch.where(up, P['C0'].double(), val)         # the strict upper triangle keeps C0
        elif case.flags & NF:
            mask = ~up                                           # unspecified
            val = torch.where(up, torch.zeros_like(val), val)
        else:
            val = torch.where(up, torch.zeros_like(val), val)    # exactly zero
        mag = torch.where(up, torch.zeros_like(mag), mag)
    return val, mask, mag


def _first_wrong(got, want, mask):
    bad = ((got != want) & mask).nonzero()
    i = tuple(int(x) for x in bad[0])
    return f'{len(bad)} wrong elements, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}'


def _run_ops(case, ops, P):
    A, B = build_operands(case, 'cuda', P['fill'])
    out = P['C0'].cuda()
    got = ops.gemm(A, B, case.ta, case.tb, alpha=case.alpha, beta=case.beta, out=out, flags=case.flags)
    assert got is out
    return out.cpu().double(), tuple(ops.gemm_plan(A, B, case.ta, case.tb, case.flags))[:9]


def _run_abi(case, ops, P):
    """The same launch through the C ABI: C a window of a sentinel-filled buffer, the workspace followed by a guard."""
    from nsgp import _lib
    A, B = build_operands(case, 'cuda', P['fill'])
    _, _, Av, M, K, sam, sak, sba, Bv, N, sbk, sbn, sbb, nb = ops._gemm_operands(A, B, case.ta, case.tb, None)
    dt = DTYPES[case.dt]
    wide = zlib.crc32(case.name.encode()) & 1
    ldc, c0 = (N + 4, 1) if wide else (N + 3, 0)
    buf = torch.full((nb, M + 5, ldc), SENTINEL, dtype=dt, device='cuda')
    win = buf[:, 2:M + 2, c0:c0 + N]
    win.copy_(P['C0'].cuda().reshape(nb, M, N))
    before = buf.clone()
    lib = _lib.load()
    es = buf.element_size()
    wsb = lib.nsgp_gemm_workspace(M, N, K, nb, 1, es, case.flags)
    ws = torch.full((wsb + WS_GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    _lib.call(f'nsgp_gemm_{case.dt}', M, N, K, float(case.alpha), ops._p(Av), sam, sak, sba, 0, ops._p(Bv), sbk, sbn, sbb, 0,
              float(case.beta), ctypes.c_void_p(win.data_ptr()), ldc, (M + 5) * ldc, 0, nb, 1, int(case.flags),
              ops._p(ws) if wsb else None, wsb, ops._stream())
    torch.cuda.synchronize()
    got = win.cpu().double().reshape(P['C0'].shape)
    assert bool((ws[wsb:] == 0xA5).all()), f'{case.name}: the launch wrote past its {wsb}-byte workspace'
    buf[:, 2:M + 2, c0:c0 + N] = 0
    before[:, 2:M + 2, c0:c0 + N] = 0
    assert torch.equal(buf.view(torch.int32 if es == 4 else torch.int64), before.view(torch.int32 if es == 4 else torch.int64)), \
        f'{case.name}: the launch wrote outside its M x N windows (ldc {ldc})'
    return got


ONE_LEVEL = [c for c in GEMM_CASES if c.nb2 == 1]
TWO_LEVEL = [c for c in GEMM_CASES if c.nb2 > 1]


@pytest.mark.parametrize('case', ONE_LEVEL, ids=lambda c: c.name)
def test_gemm_case_is_exact_and_writes_nothing_else(ops, case):
    P = _problem(case, 'int')
    want, mask, _ = _expected(case, P)
    got, plan = _run_ops(case, ops, P)
    assert plan == case.plan, (case.name, plan)
    assert torch.equal(got[mask], want[mask]), f'{case.name} plan {plan} (ops.gemm): ' + _first_wrong(got, want, mask)
    got = _run_abi(case, ops, P)
    assert torch.equal(got[mask], want[mask]), f'{case.name} plan {plan} (C ABI, ldc > N): ' + _first_wrong(got, want, mask)


@pytest.mark.parametrize('case', TWO_LEVEL, ids=lambda c: c.name)
@pytest.mark.parametrize('zero', ['none', 'a2', 'b1'])
def test_gemm_two_level_batch_of_diagonal_blocks_is_exact(ops, case, zero):
    """The launches of nsgp_trtri: batch x pairs blocks (s x s) on the diagonal of batch (n x n) matrices, n = 2 s pairs,
    every operand and C a window (ld = n, level-2 stride 2 s (n + 1)).  zero: `a2` A's pair stride is 0 (every pair reads
    the first pair's block), `b1` B's matrix stride is 0."""
    from nsgp import _lib
    dt = DTYPES[case.dt]
    s, nb1, nb2 = case.M, case.nb, case.nb2
    assert case.M == case.N == case.K and not case.ta and not case.tb
    n = 2 * s * nb2
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    nan = float('nan')
    Ap = torch.full((nb1, n, n), nan, dtype=dt)
    Bp = torch.full((nb1, n, n), nan, dtype=dt)
    Cp = torch.full((nb1, n, n), SENTINEL, dtype=dt)
    ao = (s, s) if case.flags & AL else (s, 0)           # where the blocks sit inside a pair's 2s x 2s diagonal block
    bo = (0, 0) if case.flags & BL else (s, 0)
    co = (s, 0)
    zA = _tri_zero_mask(s, s, True) if case.flags & AL else None
    zB = _tri_zero_mask(s, s, True) if case.flags & BL else None
    want = {}
    blocks = {}
    for b in range(nb1):
        for p in range(nb2):
            a = torch.randint(-3, 5, (s, s), generator=gen).to(dt)
            bb = torch.randint(-3, 5, (s, s), generator=gen).to(dt)
            blocks[b, p] = (a, bb)
            o = 2 * s * p
            Ap[b, o + ao[0]:o + ao[0] + s, o + ao[1]:o + ao[1] + s] = a if zA is None else torch.where(zA, torch.full_like(a, nan), a)
            Bp[b, o + bo[0]:o + bo[0] + s, o + bo[1]:o + bo[1] + s] = bb if zB is None else torch.where(zB, torch.full_like(bb, nan), bb)
    for b in range(nb1):
        for p in range(nb2):
            a = blocks[b, 0 if zero == 'a2' else p][0].double()
            bb = blocks[0 if zero == 'b1' else b, p][1].double()
            if zA is not None:
                a = torch.where(zA, torch.zeros_like(a), a)
            if zB is not None:
                bb = torch.where(zB, torch.zeros_like(bb), bb)
            want[b, p] = case.alpha * (a @ bb)
    Ad, Bd, Cd = Ap.cuda(), Bp.cuda(), Cp.cuda()
    es = Ad.element_size()
    off = lambda o: (o[0] * n + o[1]) * es                # noqa: E731
    l2 = 2 * s * (n + 1)
    _lib.call(f'nsgp_gemm_{case.dt}', s, s, s, float(case.alpha),
              ctypes.c_void_p(Ad.data_ptr() + off(ao)), n, 1, n * n, 0 if zero == 'a2' else l2,
              ctypes.c_void_p(Bd.data_ptr() + off(bo)), n, 1, 0 if zero == 'b1' else n * n, l2,
              0.0, ctypes.c_void_p(Cd.data_ptr() + off(co)), n, n * n, l2, nb1, nb2, int(case.flags), None, 0, ops._stream())
    torch.cuda.synchronize()
    got = Cd.cpu()
    for (b, p), w in want.items():
        o = 2 * s * p
        g = got[b, o + co[0]:o + co[0] + s, o + co[1]:o + co[1] + s].double()
        assert torch.equal(g, w), f'{case.name} block {(b, p)}: ' + _first_wrong(g, w, torch.ones_like(w, dtype=torch.bool))
        got[b, o + co[0]:o + co[0] + s, o + co[1]:o + co[1] + s] = SENTINEL
    assert bool((got == SENTINEL).all()), f'{case.name}: wrote outside the blocks'


def _one_row_per_plan_key():
    seen = {}
    for c in ONE_LEVEL:
        seen.setdefault(plan_key(c.dt, c.plan), c)
    return list(seen.values())


@pytest.mark.parametrize('case', _one_row_per_plan_key(), ids=lambda c: c.name)
def test_gemm_rounding_stays_within_the_bound_of_the_arithmetic(ops, case):
    P = _problem(case, 'normal')
    want, mask, mag = _expected(case, P, need_mag=True)
    got, plan = _run_ops(case, ops, P)
    u = torch.finfo(DTYPES[case.dt]).eps / 2
    bound = (case.K + plan[2] + 4) * u * mag
    diff = (got - want).abs()
    assert bool(torch.isfinite(got[mask]).all())
    ratio = float((diff[mask] / bound[mask].clamp_min(1e-300)).max())
    print(f'[measured] gemm rounding {case.name} key {plan_key(case.dt, plan)}: max|diff| {float(diff[mask].max()):.3g}, '
          f'worst diff/bound = {ratio:.3g} at (K + ksplit + 4) u = {(case.K + plan[2] + 4) * u:.3g}')
    assert bool((diff[mask] <= bound[mask]).all()), ratio


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_gemm_empty_inner_and_outer_dimensions(ops, dt):
    """K = 0: C = beta C0 (beta == 0: zeros, whatever C held), no operand is read.  M or N = 0: nothing happens."""
    from nsgp import _lib
    tdt = DTYPES[dt]
    for M, N in ((70, 130), (128, 128)):
        C0 = torch.randint(-8, 9, (M, N)).to(tdt)
        out = torch.full((M, N), float('nan'), dtype=tdt, device='cuda')
        ops.gemm(torch.empty(M, 0, dtype=tdt, device='cuda'), torch.empty(0, N, dtype=tdt, device='cuda'), out=out)
        assert torch.equal(out.cpu(), torch.zeros(M, N, dtype=tdt))
        out = C0.cuda()
        ops.gemm(torch.empty(M, 0, dtype=tdt, device='cuda'), torch.empty(0, N, dtype=tdt, device='cuda'), alpha=-2.0,
                 beta=-2.0, out=out)
        assert torch.equal(out.cpu(), -2.0 * C0)
    guard = torch.full((64,), SENTINEL, dtype=tdt, device='cuda')
    for M, N in ((0, 5), (5, 0)):
        assert getattr(_lib.load(), f'nsgp_gemm_{dt}')(M, N, 4, 1.0, ops._p(guard), 4, 1, 0, 0, ops._p(guard), N, 1, 0, 0, 0.0,
                                                        ops._p(guard), max(N, 1), 0, 0, 1, 1, 0, None, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((guard == SENTINEL).all())


@pytest.mark.parametrize('dt', ['f32', 'f64'])
def test_gemm_error_codes_leave_c_untouched(ops, dt):
    """Every argument check of gemm_impl returns before anything is launched (read off csrc/gemm.hip: the checks precede the
    first memset / kernel launch), so C must be bit-identical afterwards."""
    from nsgp import _lib
    tdt = DTYPES[dt]
    fn = getattr(_lib.load(), f'nsgp_gemm_{dt}')
    a = torch.ones(64, 4096, dtype=tdt, device='cuda')
    b = torch.ones(4096, 64, dtype=tdt, device='cuda')
    c = torch.full((64, 64), SENTINEL, dtype=tdt, device='cuda')
    ws = torch.zeros(1024, dtype=torch.uint8, device='cuda')
    ok = dict(M=64, N=64, K=16, A=ops._p(a), B=ops._p(b), C=ops._p(c), ldc=64, nb1=1, nb2=1, flags=0, ws=None, wsb=0)

    def call(**kw):
        k = dict(ok, **kw)
        return fn(k['M'], k['N'], k['K'], 1.0, k['A'], 4096, 1, 0, 0, k['B'], 64, 1, 0, 0, 0.0, k['C'], k['ldc'], 0, 0,
                  k['nb1'], k['nb2'], k['flags'], k['ws'], k['wsb'], ops._stream())
    assert call(M=-1) == -1 and call(N=-1) == -2 and call(K=-1) == -3
    assert call(nb1=0) == -20 and call(nb2=0) == -20
    assert call(A=None) == -5 and call(B=None) == -10 and call(C=None) == -16 and call(ldc=63) == -17
    assert call(flags=AL | AU) == -22 and call(flags=BL | BU) == -22
    need = _lib.load().nsgp_gemm_workspace(64, 64, 4096, 1, 1, a.element_size(), 0)
    assert need > 1024
    assert call(K=4096) == -23 and call(K=4096, ws=ops._p(ws), wsb=1024) == -23
    assert call(nb1=70000) == -24
    torch.cuda.synchronize()
    assert bool((c == SENTINEL).all())
