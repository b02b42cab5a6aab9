"""Every fused SVGP product of csrc/gemm.hip on the GPU, exactly: the rows of tests/fused_gemm_cases.py through the C entry
points (as tools/record_gemm_hashes.py calls them).

`int` rows: small-integer operands (ranges asserted in tests/test_fused_gemm_cases_cpu.py), so the float64 formula of
include/nsgp.h, section K6, is the answer for float32 and float64 alike: `torch.equal`.  The partial buffers are compared
PER TILE ROW -- part[b, t, j], t < T -- never as a sum over t: their layout is a contract.  `grid` rows (the
float64-accumulating entry points): Y must be the exact product rounded once to float32, bit for bit; each partial is held
elementwise to (rows in the tile + 2) u sum_rows |v|^2 (|v| |rv| for part_dot), u = 2^-53, plus one float32 rounding for
float32 partials -- the bound of a sum of that many products, not a measurement; a float64 partial formed from the rounded
Y misses it by eight orders of magnitude.  `kzx` rows: Y is the exact product of W with the float32 operand the RBF build
returns, each partial is held per tile row to the bound of the arithmetic, and Y and both partial buffers are bit-equal to
nsgp_svgp_tri_gemm_colstats_f64acc on that operand.

Every row: the strict upper triangle of L / W / Lq holds NaN; every output lies inside a sentinel-filled parent with 16
guard words either side, partial buffers have two tile rows more than the launch fills wherever the entry point takes
`part_rows`, and everything the header does not say is written must keep its bits; outputs start as NaN (the Lqbar of
lqbar_acc from an integer C0, whose strict upper triangle must keep its bits; that of lqbar must be exactly 0)."""
import ctypes

import pytest
import torch

import fused_gemm_cases as FC
import gemm_bits_cases as GB

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
GUARD = 16
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _bits(t):
    return t.view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


class Guarded:
    """An output of `shape` inside a sentinel-filled parent, GUARD words either side.  `init` (CPU tensor or None: NaN) fills
    rows [:rows] of dimension 1 -- what the launch is to write; further rows keep the sentinel."""

    def __init__(self, shape, dtype, rows=None, init=None):
        numel = 1
        for s in shape:
            numel *= s
        self.parent = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=dtype, device='cuda')
        self.view = self.parent[GUARD:GUARD + numel].view(shape)
        self.rows = shape[1] if rows is None else rows
        self.view[:, :self.rows] = NAN if init is None else init.cuda()
        self.before = self.parent.clone()

    def ptr(self):
        return ctypes.c_void_p(self.view.data_ptr())

    def written(self):
        return self.view[:, :self.rows].cpu()

    def check_untouched(self, what):
        """Everything but rows [:rows] of the view keeps its bits."""
        after = self.parent.clone()
        n = self.view.numel()
        after[GUARD:GUARD + n].view(self.view.shape)[:, :self.rows] = 0
        b = self.before.clone()
        b[GUARD:GUARD + n].view(self.view.shape)[:, :self.rows] = 0
        assert torch.equal(_bits(after), _bits(b)), f'{what}: written outside what the header says'


def _offset_view(t, elems):
    """t on the GPU as a view `elems` elements into a parent one element larger (a misaligned base pointer)."""
    parent = torch.full((t.numel() + 1,), NAN, dtype=t.dtype, device='cuda')
    v = parent[elems:elems + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def _first_wrong(got, want):
    bad = (got != want).nonzero()
    i = tuple(int(x) for x in bad[0])
    return f'{len(bad)} wrong elements, first at {i}: got {float(got[i])!r}, want {float(want[i])!r}'


def _assert_equal(c, name, got, want, skip=None):
    """got == want exactly (float64 comparison of exactly converted values); `skip`: a mask of elements held elsewhere."""
    got, want = got.double(), want.double()
    if skip is not None:
        got, want = torch.where(skip, torch.zeros_like(got), got), torch.where(skip, torch.zeros_like(want), want)
    assert torch.equal(got, want), f'{FC.case_id(c)} tile {c.tile} whole {c.whole}: {name}: ' + _first_wrong(got, want)


def run(c, d, ops):
    """One call of the row's entry point on the operands `d` -> {name: Guarded}; every guard checked."""
    from nsgp import _lib
    lib = _lib.load()
    b, M, n, st = c.batch, c.M, c.n, ops._stream()
    opt = dict(c.opt)
    dt = FC.F64 if c.dt == 'f64' else FC.F32
    p = ops._p
    dev = lambda name: d[name].cuda()                                                        # noqa: E731
    out = {}
    if c.family in ('colstats', 'colstats_t', 'colstats_rows'):
        T = int(lib.nsgp_svgp_colstats_tiles(M, n, b, FC.es(c)))
        rows = T + FC.EXTRA_ROWS if c.family == 'colstats_rows' else T
        out = dict(Y=Guarded((b, M, n), dt), p0=Guarded((b, rows, n), dt, T), p1=Guarded((b, rows, n), dt, T))
        L, X, rv = dev('L'), dev('X'), dev('rv')
        p0 = None if opt.get('p0') == 'null' else out['p0'].ptr()
        if c.family == 'colstats_rows':
            _lib.call(f'nsgp_svgp_tri_gemm_colstats_rows_{c.dt}', p(L), 0, p(X), p(rv), b, M, n, out['Y'].ptr(), p0,
                      out['p1'].ptr(), rows, st)
        else:
            _lib.call(f'nsgp_svgp_tri_gemm_colstats_{c.dt}', p(L), int(c.family == 'colstats_t'), p(X), p(rv), b, M, n,
                      out['Y'].ptr(), p0, out['p1'].ptr(), st)
    elif c.family == 'abar':
        out = dict(Abar=Guarded((b, M, n), dt))
        args = [dev(k) for k in ('Lq', 'C', 'A', 'm', 'gm', 'gv')]
        _lib.call(f'nsgp_svgp_abar_{c.dt}', *[p(t) for t in args], b, M, n, out['Abar'].ptr(), st)
    elif c.family in ('lqbar', 'lqbar_acc'):
        acc = c.family == 'lqbar_acc'
        wsb = int(lib.nsgp_svgp_lqbar_workspace(b, M, n, FC.es(c)))
        assert int(wsb > 0) == c.split and wsb % FC.es(c) == 0
        out = dict(Lqbar=Guarded((b, M, M), dt, init=d['C0'] if acc else None))
        if wsb:
            out['ws'] = Guarded((1, wsb // FC.es(c)), dt)
        A, C = dev('A'), dev('C')
        gv = _offset_view(d['gv'], 1) if opt.get('mis') == 'gvar' else dev('gv')
        beta = (GB.LQ_BETA,) if acc else ()
        _lib.call(f'nsgp_svgp_{c.family}_{c.dt}', p(A), p(C), p(gv), b, M, n, *beta, out['Lqbar'].ptr(),
                  out['ws'].ptr() if wsb else None, wsb, st)
    else:
        T = int(lib.nsgp_svgp_f64acc_tiles_for(M, n, b))
        rows = T + FC.EXTRA_ROWS
        pdt = FC.part_dtype(c)
        out = dict(Y=Guarded((b, M, n), FC.F32), p1=Guarded((b, rows, n), pdt, T))
        W = _offset_view(d['W'], 1) if opt.get('mis') == 'W' else dev('W')
        rv = dev('rv')
        if c.family == 'kzx':
            out['p0'] = Guarded((b, rows, n), pdt, T)
            Z, x, ls, os_ = d['Zd'], d['xd'], d['lsd'], d['osd']
            _lib.call('nsgp_svgp_kzx_gemm_colstats_f64acc', p(W), p(Z), p(x), n * opt['D'] if opt['xb'] else 0, p(ls), p(os_),
                      opt['D'], p(rv), b, M, n, out['Y'].ptr(), out['p0'].ptr(), out['p1'].ptr(), rows, st)
        else:
            X = _offset_view(d['X'], 1) if opt.get('mis') == 'X' else dev('X')
            if c.family == 'f64acc_t':
                _lib.call('nsgp_svgp_tri_gemm_colstats_f64acc_t', p(W), p(X), b, M, n, out['Y'].ptr(), out['p1'].ptr(), rows, st)
            else:
                out['p0'] = Guarded((b, rows, n), pdt, T)
                p0 = None if opt.get('p0') == 'null' else out['p0'].ptr()
                _lib.call('nsgp_svgp_tri_gemm_colstats_' + c.family, p(W), p(X), p(rv), b, M, n, out['Y'].ptr(), p0,
                          out['p1'].ptr(), rows, st)
    torch.cuda.synchronize()
    for name, gbuf in out.items():
        if name == 'ws':                                 # the workspace proper is the launch's own; its guards are not
            gbuf.check_untouched(f'{FC.case_id(c)} workspace')
        else:
            gbuf.check_untouched(f'{FC.case_id(c)} {name}')
    if opt.get('p0') == 'null':                          # not passed: nothing of it may have been written either
        assert torch.equal(_bits(out['p0'].parent), _bits(out['p0'].before))
        del out['p0']
    return out


def _check_int(c, d, out, ref, nan_col=None):
    """Exact comparison of an `int` row.  nan_col: X[last b, 0, j*] was NaN -- column j* of the last batch element is NaN in
    every row of Y and every tile row of the partials, and NOTHING else differs from the reference."""
    for name in ('Y', 'p0', 'p1', 'Abar', 'Lqbar'):
        if name not in out:
            continue
        got, want = out[name].written(), ref[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        skip = None
        if nan_col is not None:
            skip = torch.zeros(want.shape, dtype=torch.bool)
            skip[-1, :, nan_col] = True
            assert bool(torch.isnan(got[skip]).all()), f'{FC.case_id(c)}: {name}[last b, :, {nan_col}] is not NaN everywhere'
        _assert_equal(c, name, got, want, skip)
    if c.family == 'lqbar':
        up = torch.ones(c.M, c.M, dtype=torch.bool).triu(1)
        assert bool((out['Lqbar'].written()[:, up] == 0).all()), 'strict upper triangle of Lqbar not zero'
    if c.family == 'lqbar_acc':
        up = torch.ones(c.M, c.M, dtype=torch.bool).triu(1)
        assert torch.equal(_bits(out['Lqbar'].written()[:, up]), _bits(d['C0'][:, up])), 'strict upper triangle of Lqbar changed'


INT_CASES = [c for c in FC.CASES if c.kind == 'int']
GRID_CASES = [c for c in FC.CASES if c.kind == 'grid']
KZX_CASES = [c for c in FC.CASES if c.kind == 'kzx']


@pytest.mark.parametrize('case', INT_CASES, ids=FC.case_id)
def test_fused_product_is_exact_per_tile_row_and_writes_nothing_else(ops, case):
    d = FC.build(case)
    out = run(case, d, ops)
    _check_int(case, d, out, FC.reference(case, d))


@pytest.mark.parametrize('case,col', FC.NAN_CASES, ids=lambda v: FC.case_id(v) if isinstance(v, FC.Case) else f'j{v}')
def test_one_nan_column_stays_in_its_column(ops, case, col):
    """Any mixing of columns in the shuffle or LDS reduction of the epilogue spreads the NaN."""
    d = FC.build(case)
    ref = FC.reference(case, d)                          # of the clean operands: what every other element must still be
    d['X'] = d['X'].clone()
    d['X'][-1, 0, col] = NAN
    out = run(case, d, ops)
    _check_int(case, d, out, ref, nan_col=col)


@pytest.mark.parametrize('case', GRID_CASES, ids=FC.case_id)
def test_f64acc_rounds_y_once_and_sums_unrounded_partials(ops, case):
    d = FC.build(case)
    ref = FC.grid_reference(case, d)
    out = run(case, d, ops)
    Y = out['Y'].written()
    assert Y.dtype == torch.float32
    _assert_equal(case, 'Y (the exact product rounded once)', Y, ref['Y'].float())
    p32 = FC.part_dtype(case) == FC.F32
    for name in ('p0', 'p1'):
        if name not in out:
            continue
        hi, lo, mag = ref[name]
        got = out[name].written()
        assert got.dtype == FC.part_dtype(case) and got.shape == hi.shape
        assert bool(torch.isfinite(got).all())
        diff = ((got.double() - hi) - lo).abs()
        bound = (ref['rows'] + 2) * 2.0 ** -53 * mag + (2.0 ** -24 * hi.abs() if p32 else 0.0)
        ratio = float((diff / bound.clamp_min(1e-300)).max())
        print(f'[measured] {FC.case_id(case)} {name}: worst |got - exact| / bound = {ratio:.3g} '
              f'(max diff {float(diff.max()):.3g}, {"float32" if p32 else "float64"} partials)')
        bad = (diff > bound).nonzero()
        assert len(bad) == 0, f'{FC.case_id(case)} {name}: {len(bad)} beyond the bound, first at {tuple(bad[0].tolist())}, ratio {ratio:.3g}'


@pytest.mark.parametrize('case', KZX_CASES, ids=FC.case_id)
def test_generated_operand_product_is_exact_and_equals_the_materialised_one(ops, case):
    from nsgp import _lib
    d = FC.build(case)
    klo, khi, units = FC.kzx_range(case, d)
    assert units < 2.0 ** 53
    for k in ('Z', 'x', 'ls', 'os'):
        d[k + 'd'] = d[k].cuda()
    K32 = ops.rbf_build(d['Zd'], d['xd'], d['lsd'], d['osd'])
    assert K32.dtype == torch.float32 and K32.shape == (case.batch, case.M, case.n)
    assert klo <= float(K32.min()) and float(K32.max()) <= khi, (klo, float(K32.min()), float(K32.max()), khi)
    out = run(case, d, ops)
    # exact in float64 by the range just asserted (fused_gemm_cases.kzx_range), rounded once
    V = d['clean_L'] @ K32.cpu().double()
    _assert_equal(case, 'Y (W @ K32 rounded once)', out['Y'].written(), V.float())
    # placement, independently of the launch compared with below: each float32 partial per tile row against the float64 sums
    # of the exact v -- (rows + 2) u sum |v|^2 for the kernel's float64 sum, as much again for the host's, one float32 rounding
    h = case.tile[0]
    rows = torch.tensor([min(h, case.M - t * h) for t in range(case.trows)], dtype=torch.float64)[None, :, None]
    rvd = d['rv'].double()[:, :, None]
    sq = FC.tile_sums(V * V, h)
    for name, ref, mag in (('p0', FC.tile_sums(V * rvd, h), FC.tile_sums(V.abs() * rvd.abs(), h)), ('p1', sq, sq)):
        diff = (out[name].written().double() - ref).abs()
        bound = 2 * (rows + 2) * 2.0 ** -53 * mag + 2.0 ** -24 * ref.abs()
        bad = (~(diff <= bound)).nonzero()
        assert len(bad) == 0, f'{FC.case_id(case)} {name}: {len(bad)} beyond the bound, first at {tuple(bad[0].tolist())}'
    b, M, n, T = case.batch, case.M, case.n, case.trows
    Y, p0, p1 = (torch.full(s, NAN, dtype=torch.float32, device='cuda') for s in ((b, M, n), (b, T, n), (b, T, n)))
    W, rv = d['W'].cuda(), d['rv'].cuda()
    _lib.call('nsgp_svgp_tri_gemm_colstats_f64acc', ops._p(W), ops._p(K32), ops._p(rv), b, M, n, ops._p(Y), ops._p(p0), ops._p(p1),
              T, ops._stream())
    torch.cuda.synchronize()
    for name, mine, theirs in (('Y', out['Y'], Y), ('part_dot', out['p0'], p0), ('part_sq', out['p1'], p1)):
        assert bool(torch.isfinite(theirs).all())
        assert torch.equal(_bits(mine.written()), _bits(theirs.cpu())), f'{FC.case_id(case)}: {name} differs from the materialised product'
