"""The fused-product cases of the GEMM bit pin (csrc/gemm.hip), shared by tools/record_gemm_hashes.py,
tests/test_gemm_bits_cases_cpu.py and tests/test_gpu_gemm_bits.py.  The plain products of the pin are the rows of
GEMM_CASES (tests/test_gemm_plan_cpu.py) on seeded normal operands; this table adds the variants no exact test holds:
fused epilogues (column statistics, the A-adjoint), the k-scaled loader with a lower-only, split output, and the
float64-accumulating projections (float32 / float64 / generated B operand).

One row per (entry-point family x tile x whole / ragged) that exists.  Every row states the tile and the `whole` value
(and, for the lqbar rows, whether the launch is split along K) it was chosen for; tests/test_gemm_bits_cases_cpu.py checks
them against the library's host-side queries.  In every row the triangular operand has M = K, so the tile rows of one
launch have K ranges of different lengths and between them run every stretch of the K loops: masked and unmasked staging,
waves with and without MFMA work, diagonal blocks at either end, a ragged last K-tile, odd and even tile counts in the
paired loops, the generic head and tail.
"""
import collections
import zlib

# family: the entry point(s), see FAMILIES.  tile = (rows, columns).  opt: family-specific ((key, value), ...).
Case = collections.namedtuple('Case', 'family dt batch M n tile whole opt')

FAMILIES = {
    # gemm_impl launches: nsgp_gemm_plan answers for (M, N, K, flags, modes) below
    'colstats': 'nsgp_svgp_tri_gemm_colstats_{dt} (trans = 0)',
    'colstats_t': 'nsgp_svgp_tri_gemm_colstats_{dt} (trans = 1)',
    'colstats_rows': 'nsgp_svgp_tri_gemm_colstats_rows_{dt} (part_rows above the tile rows)',
    'abar': 'nsgp_svgp_abar_{dt}',
    'lqbar': 'nsgp_svgp_lqbar_{dt}',
    'lqbar_acc': 'nsgp_svgp_lqbar_acc_{dt} (beta != 0)',
    # tri_gemm_colstats_f64acc_impl launches: nsgp_svgp_f64acc_tiles_for / nsgp_svgp_kzx_gemm_supported answer
    'f64acc': 'nsgp_svgp_tri_gemm_colstats_f64acc',
    'f64acc_b64': 'nsgp_svgp_tri_gemm_colstats_f64acc_b64',
    'f64acc_b64p32': 'nsgp_svgp_tri_gemm_colstats_f64acc_b64p32',
    'f64acc_t': 'nsgp_svgp_tri_gemm_colstats_f64acc_t',
    'kzx': 'nsgp_svgp_kzx_gemm_colstats_f64acc',
}
GEMM_IMPL_FAMILIES = ('colstats', 'colstats_t', 'colstats_rows', 'abar', 'lqbar', 'lqbar_acc')
F64ACC_FAMILIES = ('f64acc', 'f64acc_b64', 'f64acc_b64p32', 'f64acc_t')

AL, AU, CL, NS = 1, 2, 16, 32           # NSGP_GEMM_* of include/nsgp.h
LQ_BETA = -0.5                          # beta of the lqbar_acc rows
EXTRA_ROWS = 2                          # colstats_rows: part_rows = the launch's tile rows + this


def _c(family, dt, shape, tile, whole, **opt):
    return Case(family, dt, shape[0], shape[1], shape[2], tuple(tile), int(whole), tuple(sorted(opt.items())))


# (batch, M, n) -> (tile, whole) of the projections A = W X (flags A_LOWER / A_UPPER | NO_SPLITK, K = M)
PROJ_F32 = [((2, 128, 192), (64, 64), 1), ((2, 63, 65), (64, 64), 0), ((1, 130, 700), (64, 64), 0),
            ((1, 256, 16384), (128, 64), 1), ((1, 250, 16400), (128, 64), 0),
            ((1, 256, 38400), (128, 128), 1), ((1, 250, 38500), (128, 128), 0)]
PROJ_F64 = PROJ_F32[:3]
# (batch, M, n) -> (tile, whole, split) of Lqbar = tril(A diag(2 v) C^T) (M x M output, K = n, flag C_LOWER)
LQBAR_F32 = [((1, 192, 300), (64, 64), 0, 0), ((1, 192, 4096), (64, 64), 1, 1), ((2, 256, 16384), (128, 128), 1, 1),
             ((1, 200, 1000), (64, 64), 0, 1), ((1, 2944, 256), (128, 128), 1, 0)]
LQBAR_F64 = [r for r in LQBAR_F32 if r[1] == (64, 64)]
LQBAR_ACC = [((1, 192, 4096), (64, 64), 1, 1), ((1, 192, 300), (64, 64), 0, 0)]
# (batch, M, n) -> (tile rows, whole) of the float64-accumulating projection (64 columns per tile)
F64ACC = [((2, 256, 512), 64, 1), ((1, 200, 333), 64, 0), ((1, 256, 16384), 128, 1), ((2, 250, 8200), 128, 0)]
# generated B operand (whole tiles only): (batch, M, n), tile rows, D, per-GP inputs
KZX = [((2, 256, 512), 64, 3, 0), ((1, 256, 16384), 128, 1, 0), ((1, 256, 16384), 128, 4, 0), ((3, 128, 128), 64, 4, 1)]

CASES = []
for _fam in ('colstats', 'colstats_t', 'abar'):
    CASES += [_c(_fam, 'f32', s, t, w) for s, t, w in PROJ_F32]
    CASES += [_c(_fam, 'f64', s, t, w) for s, t, w in PROJ_F64]
CASES += [_c('colstats_rows', dt, (1, 130, 700), (64, 64), 0) for dt in ('f32', 'f64')]
CASES += [_c('lqbar', 'f32', s, t, w, split=sp) for s, t, w, sp in LQBAR_F32]
CASES += [_c('lqbar', 'f64', s, t, w, split=sp) for s, t, w, sp in LQBAR_F64]
CASES += [_c('lqbar_acc', dt, s, t, w, split=sp) for dt in ('f32', 'f64') for s, t, w, sp in LQBAR_ACC]
for _fam in F64ACC_FAMILIES:
    CASES += [_c(_fam, 'f64acc', s, (r, 64), w) for s, r, w in F64ACC]
CASES += [_c('kzx', 'f64acc', s, (r, 64), 1, D=D, xb=xb) for s, r, D, xb in KZX]


def case_id(c):
    tail = ''.join(f'|{k}={v}' for k, v in c.opt)
    return f'{c.family}|{c.dt}|b{c.batch}M{c.M}n{c.n}{tail}'


def seed(c):
    return zlib.crc32(case_id(c).encode())


def gemm_query(c):
    """(M, N, K, flags, mode_a, mode_b) of the nsgp_gemm_plan query that plans a gemm_impl row (operands contiguous and
    aligned: vector loads wherever the unit-stride extent is a multiple of 4)."""
    if c.family in ('lqbar', 'lqbar_acc'):
        return c.M, c.M, c.n, CL, 0, 0
    if c.family == 'colstats_t':
        return c.M, c.n, c.M, AU | NS, 1, 1
    return c.M, c.n, c.M, AL | NS, 0, 1


def gemm_vec(c):
    """(vec_a, vec_b) of that query, by gemm_impl's rule (unit stride, the other strides multiples of 4)."""
    if c.family in ('lqbar', 'lqbar_acc'):
        v = int(c.n % 4 == 0 and (c.M * c.n) % 4 == 0)
        return v, v
    return int(c.M % 4 == 0), int(c.n % 4 == 0 and (c.M * c.n) % 4 == 0)
