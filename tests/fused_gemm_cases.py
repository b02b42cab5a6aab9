"""The exact tests of the fused SVGP products of csrc/gemm.hip: case table, seeded builders and float64 references, shared
by tests/test_fused_gemm_cases_cpu.py (no GPU) and tests/test_gpu_fused_gemm.py.  Nothing here touches a GPU.

Every row states where its launch lands -- tile, `whole`, the two vector-load flags, split along K, tile rows -- and the path
tags it is there for; the CPU test asks the library's host queries whether that is so.  The families and their entry
points are those of tests/gemm_bits_cases.py (FAMILIES), and every row of its CASES has a row here with the same launch
shape, so the bit pin and the exact tests hold the same launches.

Data kinds
    int   every operand holds small integers from a seeded torch.randint, the ranges chosen per row (`int_ranges`) so that
          every output and every partial sum, in any order, is an integer below 2^24 (float32 storage) or 2^53: the float64
          formula of include/nsgp.h, section K6, is then THE answer, bit for bit (`int_bounds` computes what the CPU test
          asserts: a condition on the inputs, not a tolerance).
    grid  (float64-accumulating families) W integers in -3..4, a float32 X = k 2^-20 with |k| < 2^23, a float64 X64 =
          k 2^-40 with |k| < 2^40 (not float32 numbers): every partial sum of W X is a multiple of the grid below 2^53 units,
          the float64 host product is exact in any order, and Y must be its single rounding to float32.  The partials are
          sums of squares of 34- to 50-bit values; `grid_reference` returns them exactly (integer arithmetic) as a
          double-double, with the bound of the arithmetic.
    kzx   the generated operand: inputs confined so that every float32 value the RBF build can return lies in
          [klo, khi] (`kzx_range`), all of them multiples of 2^(floor(log2 klo) - 23); with |W| <= 4 and M terms every partial
          sum is below 4 M khi, and the float64 host product W @ K32.double() is exact while 4 M khi / 2^(floor(log2 klo) - 23)
          < 2^53.
The strict upper triangle of every stored triangular operand (L, W, Lq -- also under trans = 1) holds NaN."""
import collections
import math
import zlib

import numpy as np
import torch

import gemm_bits_cases as GB

Case = collections.namedtuple('Case', 'family dt kind batch M n tile whole vec split trows tags opt')

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
EXTRA_ROWS = 2                          # part_rows = tile rows + this wherever the entry point takes part_rows
PART_ROWS_FAMILIES = ('colstats_rows',) + GB.F64ACC_FAMILIES + ('kzx',)
P64_FAMILIES = ('f64acc_b64', 'f64acc_t')
B64_FAMILIES = ('f64acc_b64', 'f64acc_b64p32')
GRID32, GRID64 = 20, 40                 # X = k 2^-GRID
TAGS = ('vecA_off', 'vecB_off', 'vec_not_whole', 'misaligned_W', 'misaligned_X', 'ks_vec', 'ks_unaligned_batch',
        'ks_unaligned_base', 'tile_rows_1', 'tile_rows_2', 'tile_rows_3', 'tile_rows_4', 'part_rows_extra', 'p0_null',
        'batch_perm_on', 'batch_perm_off', 'trans', 'split', 'unsplit', 'whole', 'ragged', 'tiles_512', 'per_gp_x')


def _c(family, dt, kind, shape, tile, whole, vec, split, trows, tags, **opt):
    tags = set(tags) | {'whole' if whole else 'ragged'}
    if family in PART_ROWS_FAMILIES:
        tags.add('part_rows_extra')
    if family in ('colstats_t', 'f64acc_t'):
        tags.add('trans')
    if family in ('lqbar', 'lqbar_acc'):
        tags.add('split' if split else 'unsplit')
    if opt.get('p0') == 'null':
        tags.add('p0_null')
    if opt.get('xb'):
        tags.add('per_gp_x')
    return Case(family, dt, kind, shape[0], shape[1], shape[2], tuple(tile), int(whole), tuple(vec), int(split), int(trows),
                tuple(sorted(tags)), tuple(sorted(opt.items())))


# ---- the projections gemm_impl launches: Y = op(L) X (K = M).  (batch, M, n) -> tile, whole, (vecA, vecB), tile rows, tags.
# vecA: M % 4 == 0; vecB: n % 4 == 0 (and M n % 4 == 0); whole: both, and M, n, K multiples of the tile.
PROJ_SMALL = [
    ((1, 1, 1), (64, 64), 0, (0, 0), 1, ('vecA_off', 'vecB_off', 'tile_rows_1')),
    ((1, 64, 64), (64, 64), 1, (1, 1), 1, ('tile_rows_1',)),
    ((1, 65, 63), (64, 64), 0, (0, 0), 2, ('vecA_off', 'vecB_off', 'tile_rows_2')),
    ((1, 130, 64), (64, 64), 0, (0, 1), 3, ('vecA_off', 'tile_rows_3')),
    ((1, 128, 66), (64, 64), 0, (1, 0), 2, ('vecB_off', 'tile_rows_2')),
    ((3, 129, 4), (64, 64), 0, (0, 1), 3, ('vecA_off', 'batch_perm_on', 'tile_rows_3')),
    # the rows of the bit pin
    ((2, 128, 192), (64, 64), 1, (1, 1), 2, ('batch_perm_on', 'tile_rows_2')),
    ((2, 63, 65), (64, 64), 0, (0, 0), 1, ('vecA_off', 'vecB_off', 'batch_perm_on', 'tile_rows_1')),
    ((1, 130, 700), (64, 64), 0, (0, 1), 3, ('vecA_off', 'tile_rows_3')),
]
# float32 only: the 128 x 64 and 128 x 128 tiles exist from n = 16320 / 32832 on (M = 256); the pinned shapes are kept
PROJ_WIDE = [
    ((1, 256, 16384), (128, 64), 1, (1, 1), 2, ('tile_rows_2',)),
    ((1, 250, 16400), (128, 64), 0, (0, 1), 2, ('vecA_off', 'tile_rows_2')),
    ((1, 256, 38400), (128, 128), 1, (1, 1), 2, ('tile_rows_2',)),
    ((1, 250, 38500), (128, 128), 0, (0, 1), 2, ('vecA_off', 'tile_rows_2')),
]
ROWS_SHAPES = ((1, 1, 1), (1, 64, 64), (1, 65, 63), (1, 130, 64), (1, 128, 66), (3, 129, 4), (1, 130, 700))

# ---- Lqbar = tril(A diag(2 gvar) C^T) (M x M, K = n).  -> tile, whole, vec (A and C alike), split, tags.
# The k-scaled loader takes its vector path only where gvar + bb n is aligned to 4 elements.
LQ_SMALL = [
    ((2, 64, 1), (64, 64), 0, 0, 0, ('ks_unaligned_batch', 'batch_perm_on', 'vecA_off', 'vecB_off')),
    ((2, 64, 31), (64, 64), 0, 0, 0, ('ks_unaligned_batch', 'batch_perm_on', 'vecA_off', 'vecB_off')),
    ((2, 65, 33), (64, 64), 0, 0, 0, ('ks_unaligned_batch', 'batch_perm_on', 'vecA_off', 'vecB_off')),
    ((2, 130, 67), (64, 64), 0, 0, 0, ('ks_unaligned_batch', 'batch_perm_on', 'vecA_off', 'vecB_off')),
    ((2, 64, 64), (64, 64), 1, 1, 0, ('ks_vec', 'batch_perm_on')),
]
LQ_BASE = ((1, 128, 64), (64, 64), 1, 1, 0, ('ks_unaligned_base',))         # gvar passed at element offset 1
LQ_PIN_F32 = [
    ((1, 192, 300), (64, 64), 0, 1, 0, ('ks_vec',)),
    ((1, 192, 4096), (64, 64), 1, 1, 1, ('ks_vec',)),
    ((2, 256, 16384), (128, 128), 1, 1, 1, ('ks_vec', 'batch_perm_off')),
    ((1, 200, 1000), (64, 64), 0, 1, 1, ('ks_vec',)),
    ((1, 2944, 256), (128, 128), 1, 1, 0, ('ks_vec',)),
]
LQ_PIN_F64 = [r for r in LQ_PIN_F32 if r[1] == (64, 64)]
LQ_PIN_ACC = [LQ_PIN_F32[1], LQ_PIN_F32[0]]

# ---- the float64-accumulating projections (64 columns per tile).  -> tile rows' height, whole, (vecA, vecB), tile rows, tags.
# 64-row tiles while ceil(M / 128) ceil(n / 64) batch < 512; vecA: M % 4 == 0 and W 32-byte aligned; vecB: n % 4 == 0 and X
# 16-byte (X64: 32-byte) aligned; batch_perm: batch > 1 and tile rows x tile columns x batch <= 512.
F64ACC = [
    ((1, 1, 1), 64, 0, (0, 0), 1, ('vecA_off', 'vecB_off', 'tile_rows_1'), None),
    ((2, 63, 65), 64, 0, (0, 0), 1, ('vecA_off', 'vecB_off', 'batch_perm_on', 'tile_rows_1'), None),
    ((1, 132, 64), 64, 0, (1, 1), 3, ('vec_not_whole', 'tile_rows_3'), None),
    ((1, 130, 64), 64, 0, (0, 1), 3, ('vecA_off', 'tile_rows_3'), None),
    ((1, 128, 66), 64, 0, (1, 0), 2, ('vecB_off', 'tile_rows_2'), None),
    ((1, 64, 64), 64, 1, (1, 1), 1, ('tile_rows_1',), None),
    ((1, 128, 64), 64, 1, (1, 1), 2, ('tile_rows_2',), None),
    ((1, 192, 64), 64, 1, (1, 1), 3, ('tile_rows_3',), None),
    ((1, 256, 64), 64, 1, (1, 1), 4, ('tile_rows_4',), None),
    ((2, 256, 512), 64, 1, (1, 1), 4, ('batch_perm_on', 'tile_rows_4'), None),
    ((2, 256, 512), 64, 0, (0, 1), 4, ('misaligned_W', 'vecA_off', 'batch_perm_on', 'tile_rows_4'), 'W'),
    ((2, 256, 512), 64, 0, (1, 0), 4, ('misaligned_X', 'vecB_off', 'batch_perm_on', 'tile_rows_4'), 'X'),
    ((4, 256, 4096), 128, 1, (1, 1), 2, ('tiles_512', 'batch_perm_on', 'tile_rows_2'), None),
    ((4, 250, 4100), 128, 0, (0, 1), 2, ('vecA_off', 'batch_perm_off', 'tile_rows_2'), None),
    # the rows of the bit pin ((2, 256, 512) is above)
    ((1, 200, 333), 64, 0, (1, 0), 4, ('vecB_off', 'tile_rows_4'), None),
    ((1, 256, 16384), 128, 1, (1, 1), 2, ('tiles_512', 'tile_rows_2'), None),
    ((2, 250, 8200), 128, 0, (0, 1), 2, ('vecA_off', 'batch_perm_off', 'tile_rows_2'), None),
]
# generated B operand (whole tiles only): (batch, M, n), tile rows' height, tile rows, D, per-GP inputs
KZX = [((1, 64, 64), 64, 1, 1, 0), ((2, 64, 128), 64, 1, 2, 1), ((1, 192, 64), 64, 3, 4, 0),
       ((2, 256, 512), 64, 4, 3, 0), ((1, 256, 16384), 128, 2, 1, 0), ((1, 256, 16384), 128, 2, 4, 0), ((3, 128, 128), 64, 2, 4, 1)]

CASES = []
for _fam in ('colstats', 'colstats_t', 'abar'):
    CASES += [_c(_fam, 'f32', 'int', s, t, w, v, 0, r, tg) for s, t, w, v, r, tg in PROJ_SMALL + PROJ_WIDE]
    CASES += [_c(_fam, 'f64', 'int', s, t, w, v, 0, r, tg) for s, t, w, v, r, tg in PROJ_SMALL]
CASES += [_c('colstats_rows', dt, 'int', s, t, w, v, 0, r, tg) for dt in ('f32', 'f64') for s, t, w, v, r, tg in PROJ_SMALL
          if s in ROWS_SHAPES]
for _fam in ('lqbar', 'lqbar_acc'):
    for _dt in ('f32', 'f64'):
        _pin = LQ_PIN_ACC if _fam == 'lqbar_acc' else (LQ_PIN_F32 if _dt == 'f32' else LQ_PIN_F64)
        CASES += [_c(_fam, _dt, 'int', s, t, w, (v, v), sp, -(-s[1] // t[0]), tg) for s, t, w, v, sp, tg in LQ_SMALL + _pin]
        CASES += [_c(_fam, _dt, 'int', s, t, w, (v, v), sp, -(-s[1] // t[0]), tg, mis='gvar') for s, t, w, v, sp, tg in [LQ_BASE]]
for _fam in GB.F64ACC_FAMILIES:
    for _kind in ('int', 'grid'):
        CASES += [_c(_fam, 'f64acc', _kind, s, (h, 64), w, v, 0, r, tg, **({'mis': m} if m else {}))
                  for s, h, w, v, r, tg, m in F64ACC]
CASES += [_c('kzx', 'f64acc', 'kzx', s, (h, 64), 1, (1, 1), 0, r,
             (('batch_perm_on',) if s[0] > 1 else ()) + (('tiles_512',) if s[2] == 16384 else ()), D=D, xb=xb)
          for s, h, r, D, xb in KZX]
# part_dot == NULL: one row per column-statistics family that accepts it (Y and part_sq still right, nothing else written)
_P0 = {('colstats', 'f32', (1, 65, 63)), ('colstats_t', 'f64', (1, 65, 63)), ('colstats_rows', 'f32', (1, 130, 64)),
       ('f64acc', 'f64acc', (2, 63, 65)), ('f64acc_b64', 'f64acc', (1, 132, 64)), ('f64acc_b64p32', 'f64acc', (1, 128, 66))}
CASES += [_c(c.family, c.dt, c.kind, (c.batch, c.M, c.n), c.tile, c.whole, c.vec, c.split, c.trows, c.tags, p0='null')
          for c in CASES if c.kind == 'int' and (c.family, c.dt, (c.batch, c.M, c.n)) in _P0]


def case_id(c):
    tail = ''.join(f'|{k}={v}' for k, v in c.opt)
    return f'{c.family}|{c.dt}|{c.kind}|b{c.batch}M{c.M}n{c.n}{tail}'


def find(family, dt, kind, shape, **opt):
    want = tuple(sorted(opt.items()))
    hit = [c for c in CASES if (c.family, c.dt, c.kind, (c.batch, c.M, c.n), c.opt) == (family, dt, kind, tuple(shape), want)]
    assert len(hit) == 1, (family, dt, kind, shape, opt)
    return hit[0]


# One NaN column: X[last b, 0, j*] = NaN, j* inside a column tile (row, j*)
NAN_CASES = [(find('colstats', 'f32', 'int', (1, 130, 700)), 64 * 3 + 21),
             (find('f64acc', 'f64acc', 'int', (2, 256, 512)), 64 * 5 + 37),
             (find('f64acc_b64', 'f64acc', 'int', (1, 200, 333)), 64 * 2 + 11)]


def seed(c):
    return zlib.crc32(case_id(c).encode())


def es(c):
    return 8 if c.dt == 'f64' else 4


def storage_limit(c, what):
    """Largest magnitude below which every integer is a number of the format `what` (Y, part, out) is stored and summed in."""
    if c.dt == 'f64':
        return 2.0 ** 53
    if c.dt == 'f64acc' and what == 'part' and c.family in P64_FAMILIES:
        return 2.0 ** 53
    return 2.0 ** 24


def part_dtype(c):
    return F64 if (c.dt == 'f64' or c.family in P64_FAMILIES) else F32


def int_ranges(c):
    """(l, x): the triangular operand is drawn from -l..l (float64 storage: -3..4), the others from -x..x, by the row's M
    and storage.  M <= 64: the worst case 64 (2 3 64)^2 = 9.4e6 fits float32; M <= 256 relies on the draw (4.1e6 reached
    for a 128-row tile) and is asserted on the data, like every row."""
    if c.dt == 'f64':
        return None, None                  # -3..4, as tests/test_gpu_gemm.py
    if c.family in ('lqbar', 'lqbar_acc'):
        return 2, 2                        # gvar: -2..2 without 0, whatever the storage
    return (2, 3) if c.M <= 64 else (1, 2)


def _ints(g, shape, amp, dtype):
    lo, hi = (-3, 5) if amp is None else (-amp, amp + 1)
    return torch.randint(lo, hi, shape, generator=g).to(dtype)


def _tri(g, shape, amp, dtype):
    """A drawn square operand with no zero on its diagonal (a 1 x 1 product is then not trivially 0)."""
    t = _ints(g, shape, amp, dtype)
    dg = torch.diagonal(t, dim1=-2, dim2=-1)
    dg[dg == 0] = 1
    return t


def _nonzero(g, shape, amp, dtype):
    """Integers of -amp..amp without 0: a dropped term of a scaled sum always shows."""
    t = torch.randint(1, amp + 1, shape, generator=g) * (2 * torch.randint(0, 2, shape, generator=g) - 1)
    return t.to(dtype)


def tril_nan(t):
    """The lower triangle of t (batch, M, M) with NaN above it: the entry points read the lower triangle only."""
    return torch.where(torch.ones(t.shape[-2:], dtype=torch.bool).triu(1), torch.full_like(t, NAN), t)


def build(c):
    """Seeded operands of a row, on the CPU, in the dtypes the entry point takes (dict).  Triangular operands are given with
    NaN in the strict upper triangle; `clean_*` are their float64 lower triangles."""
    g = torch.Generator().manual_seed(seed(c))
    b, M, n = c.batch, c.M, c.n
    dt = F64 if c.dt == 'f64' else F32
    d = {}
    if c.family in ('colstats', 'colstats_t', 'colstats_rows'):
        l, x = int_ranges(c)
        L = _tri(g, (b, M, M), l, dt)
        d.update(L=tril_nan(L), clean_L=torch.tril(L).double(), X=_ints(g, (b, M, n), x, dt), rv=_ints(g, (b, M), x, dt))
    elif c.family == 'abar':
        l, x = int_ranges(c)
        Lq = _tri(g, (b, M, M), l, dt)
        d.update(Lq=tril_nan(Lq), clean_L=torch.tril(Lq).double(), C=_ints(g, (b, M, n), x, dt), A=_ints(g, (b, M, n), 8, dt),
                 m=_ints(g, (b, M), 2, dt), gm=_ints(g, (b, n), 2, dt), gv=_ints(g, (b, n), 2, dt))
    elif c.family in ('lqbar', 'lqbar_acc'):
        l, x = int_ranges(c)
        d.update(A=_ints(g, (b, M, n), l, dt), C=_ints(g, (b, M, n), x, dt), gv=_nonzero(g, (b, n), 2, dt))
        if c.family == 'lqbar_acc':        # even, so that beta C0 (beta = -1/2) is an integer
            d['C0'] = 2 * _ints(g, (b, M, M), 8, dt)
    elif c.family in GB.F64ACC_FAMILIES:
        b64 = c.family in B64_FAMILIES
        if c.kind == 'int':
            l, x = int_ranges(c)
            W = _tri(g, (b, M, M), l, F64)
            X = _ints(g, (b, M, n), x, F64 if b64 else F32)
            rv = _ints(g, (b, M), x, F32)
        else:
            W = _tri(g, (b, M, M), None, F64)
            if b64:
                X = torch.randint(-2 ** GRID64 + 1, 2 ** GRID64, (b, M, n), generator=g).double() * 2.0 ** -GRID64
            else:
                X = (torch.randint(-2 ** 23 + 1, 2 ** 23, (b, M, n), generator=g).double() * 2.0 ** -GRID32).float()
            rv = _ints(g, (b, M), 2, F32)
        d.update(W=tril_nan(W), clean_L=torch.tril(W), X=X, rv=rv)
    else:                                  # kzx
        D, xb = dict(c.opt)['D'], dict(c.opt)['xb']
        W = _tri(g, (b, M, M), None, F64)
        d.update(W=tril_nan(W), clean_L=torch.tril(W), rv=_ints(g, (b, M), 2, F32),
                 Z=torch.rand(b, M, D, generator=g) - 0.5, x=torch.rand(*((b, n, D) if xb else (n, D)), generator=g) - 0.5,
                 ls=0.6 + torch.rand(b, D, generator=g), os=0.5 + torch.rand(b, generator=g))
    return d


def op_l(c, d):
    """op(L) of the row's product, float64 (batch, M, M)."""
    L = d['clean_L']
    return L.transpose(-1, -2) if c.family in ('colstats_t', 'f64acc_t') else L


# ---- float64 references (include/nsgp.h, section K6) -------------------------------------------------------------------
def tile_sums(V, h):
    """(batch, M, n) -> (batch, ceil(M / h), n): the sum over the rows of each tile row of height h."""
    b, M, n = V.shape
    T = -(-M // h)
    P = torch.zeros(b, T * h, n, dtype=V.dtype)
    P[:, :M] = V
    return P.view(b, T, h, n).sum(2)


def ref_colstats(opL, X, rv, h):
    """Y = op(L) X;  part_dot[b,t,j] = sum_{k in tile row t} Y[b,k,j] rv[b,k];  part_sq[b,t,j] = sum Y[b,k,j]^2."""
    Y = opL @ X.double()
    return Y, (tile_sums(Y * rv.double()[:, :, None], h) if rv is not None else None), tile_sums(Y * Y, h)


def ref_abar(Lq, C, A, m, gm, gv):
    """Abar = 2 (Lq C) diag(gvar) + m gmean^T - 2 A diag(gvar)."""
    f = lambda t: t.double()                                                                # noqa: E731
    return 2 * (Lq @ f(C)) * f(gv)[:, None, :] + f(m)[:, :, None] * f(gm)[:, None, :] - 2 * f(A) * f(gv)[:, None, :]


def ref_lqbar(A, C, gv, beta=0.0, C0=None):
    """Lqbar = tril(A diag(2 gvar) C^T) (+ beta C0 on the lower triangle; the strict upper triangle is 0, or keeps C0)."""
    P = torch.tril((A.double() * (2 * gv.double())[:, None, :]) @ C.double().transpose(-1, -2))
    if C0 is None:
        return P
    up = torch.ones(P.shape[-2:], dtype=torch.bool).triu(1)
    return torch.where(up, C0.double(), P + beta * C0.double())


def reference(c, d):
    """The expected outputs of an `int` row (dict of float64 tensors)."""
    if c.family in ('colstats', 'colstats_t', 'colstats_rows') or c.family in GB.F64ACC_FAMILIES:
        rv = None if c.family == 'f64acc_t' else d['rv']
        Y, p0, p1 = ref_colstats(op_l(c, d), d['X'], rv, c.tile[0])
        return dict(Y=Y, p0=p0, p1=p1)
    if c.family == 'abar':
        return dict(Abar=ref_abar(d['clean_L'], d['C'], d['A'], d['m'], d['gm'], d['gv']))
    if c.family == 'lqbar':
        return dict(Lqbar=ref_lqbar(d['A'], d['C'], d['gv']))
    return dict(Lqbar=ref_lqbar(d['A'], d['C'], d['gv'], GB.LQ_BETA, d['C0']))


def int_bounds(c, d):
    """{quantity: (largest magnitude any partial sum of it can reach, in any order; the limit of its storage)} of an `int`
    row, from |op(L)| |X|: a condition on the inputs."""
    if c.family in ('colstats', 'colstats_t', 'colstats_rows') or c.family in GB.F64ACC_FAMILIES:
        V = op_l(c, d).abs() @ d['X'].double().abs()
        out = {'Y': (float(V.max()), storage_limit(c, 'Y')),
               'part_sq': (float(tile_sums(V * V, c.tile[0]).max()), storage_limit(c, 'part'))}
        if c.family != 'f64acc_t':
            out['part_dot'] = (float(tile_sums(V * d['rv'].double().abs()[:, :, None], c.tile[0]).max()), storage_limit(c, 'part'))
        return out
    if c.family == 'abar':
        f = lambda t: t.double().abs()                                                      # noqa: E731
        V = 2 * ((d['clean_L'].abs() @ f(d['C'])) + f(d['A'])) * f(d['gv'])[:, None, :] + f(d['m'])[:, :, None] * f(d['gm'])[:, None, :]
        return {'Abar': (float(V.max()), storage_limit(c, 'out'))}
    V = (d['A'].double().abs() * (2 * d['gv'].double().abs())[:, None, :]) @ d['C'].double().abs().transpose(-1, -2)
    if c.family == 'lqbar_acc':
        V = V + abs(GB.LQ_BETA) * d['C0'].double().abs()
    return {'Lqbar': (float(V.max()), storage_limit(c, 'out'))}


# ---- grid kind --------------------------------------------------------------------------------------------------------
def grid_bits(c):
    return GRID64 if c.family in B64_FAMILIES else GRID32


def grid_condition(c, d):
    """(largest partial sum of |op(W)| |X| in grid units, X on the grid and within its range, X64 not float32 numbers)."""
    gb = grid_bits(c)
    K = d['X'].double() * 2.0 ** gb
    on_grid = bool((K == K.round()).all()) and float(K.abs().max()) < 2.0 ** (gb if gb == GRID64 else 23)
    not_f32 = bool((d['X'].float().double() != d['X'].double()).any()) if gb == GRID64 else None
    return float((op_l(c, d).abs() @ K.abs()).max()), on_grid, not_f32


def _exact_pair(E, scale):
    """Object array of Python integers (units of 2^-scale) -> (hi, lo) float64 arrays with hi + lo == E 2^-scale to 2^-106."""
    hi = np.frompyfunc(float, 1, 1)(E).astype(np.float64)
    lo = np.frompyfunc(lambda e, h: float(e - int(h)), 2, 1)(E, hi).astype(np.float64)
    return torch.from_numpy(hi * 2.0 ** -scale), torch.from_numpy(lo * 2.0 ** -scale)


def grid_reference(c, d):
    """Y (float64, exact: every partial sum is a multiple of the grid below 2^53 units) and, per partial buffer, the exact
    sum as a double-double (hi, lo) with the magnitude sum sum_rows |v|^2 (|v| |rv|) and the rows of each tile row.
    The squares do not fit float64: v = (hi 2^25 + lo) 2^-g with integer hi, lo, summed in int64 and combined as integers."""
    gb, h = grid_bits(c), c.tile[0]
    V = op_l(c, d) @ d['X'].double()
    k = (V * 2.0 ** gb).to(torch.int64)
    assert bool((k.double() * 2.0 ** -gb == V).all())
    hi, lo = k >> 25, k & (2 ** 25 - 1)
    obj = lambda t: t.numpy().astype(object)                                                # noqa: E731
    sq = obj(tile_sums(hi * hi, h)) * 2 ** 50 + obj(tile_sums(hi * lo, h)) * 2 ** 26 + obj(tile_sums(lo * lo, h))
    sq_hi, sq_lo = _exact_pair(sq, 2 * gb)
    out = dict(Y=V, p1=(sq_hi, sq_lo, sq_hi))
    if c.family != 'f64acc_t':
        r = d['rv'].to(torch.int64)[:, :, None]
        out['p0'] = _exact_pair(obj(tile_sums(k * r, h)), gb) + (tile_sums(k.abs() * r.abs(), h).double() * 2.0 ** -gb,)
    rows = torch.tensor([min(h, c.M - t * h) for t in range(-(-c.M // h))], dtype=F64)
    out['rows'] = rows[None, :, None]
    return out


# ---- kzx --------------------------------------------------------------------------------------------------------------
def kzx_range(c, d):
    """(klo, khi, units): every float32 value of os exp(-1/2 |(z - x) / ls|^2) on the row's inputs lies in [klo, khi] (the
    float64 extremes widened by 2^-10, a thousand times the error of a float32 evaluation); such values are multiples of
    2^(floor(log2 klo) - 23), and units = 4 M khi in that unit bounds every partial sum of W K32 with |W| <= 4."""
    Z, x, ls = d['Z'].double(), d['x'].double(), d['ls'].double()
    if x.dim() == 2:
        x = x.expand(c.batch, c.n, x.shape[-1])
    d2 = (((Z[:, :, None, :] - x[:, None, :, :]) / ls[:, None, None, :]) ** 2).sum(-1)
    klo = float((d['os'].double()[:, None, None] * torch.exp(-0.5 * d2)).min()) * (1 - 2.0 ** -10)
    khi = float(d['os'].max()) * (1 + 2.0 ** -10)
    return klo, khi, 4 * c.M * khi / 2.0 ** (math.floor(math.log2(klo)) - 23)
