"""Case table of the split-K reduce (csrc/gemm.hip: splitk_reduce_kernel, splitk_reduce_vec_kernel), shared by
tools/record_splitk_reduce_hashes.py, tests/test_gpu_splitk_reduce_bits.py and tests/test_splitk_reduce_cases_cpu.py.

A row is a square product C (M x M) = alpha A B + beta C through nsgp_gemm_f32 / nsgp_gemm_f64 itself, on a C with its own
leading dimension and batch strides:
    M        64, 100, 128, 132, 192: one 64-tile, groups cut by the matrix edge of a tile, more than one block of the reduce;
             102: N % 4 != 0, which no other size gives (100 and 132 are multiples of 4) -- the scalar kernel at ldc == N
    ldpad    ldc = N + ldpad: 0, or 1 (unaligned rows: the scalar kernel)
    K        512, 2304, 4096: 2, 9 and 16 K-slices; 2048 (8 slices: the unroll width of the vector kernel itself) and 64 (one
             slice: no reduce at all) in the extra rows at the end
    batch    '1'; '2x1' and '1x2': two matrices on the first or the second batch level, BATCH_GAP elements apart beyond
             M * ldc (not contiguous; the gap keeps 16-byte alignment, so these rows stay on the vector kernel)
    flags    none, C_LOWER, C_LOWER | C_HALFDIAG, C_LOWER | C_NOFILL
    alpha    1, -1;  beta 0, 0.5;  float32 and float64
The core is the full product of (M, ldpad, flags, dtype), twice; K, batch, alpha and beta of a row are drawn from its name
(crc32), so the table is the same everywhere; the CPU companion asserts what the draw has to cover.
"""
import itertools
import zlib
from collections import namedtuple

CL, NF, HD = 16, 64, 128            # NSGP_GEMM_C_LOWER, C_NOFILL, C_HALFDIAG (include/nsgp.h)
SIZES = (64, 100, 102, 128, 132, 192)
KS = (512, 2304, 4096)
BATCHES = ('1', '2x1', '1x2')
FLAGS = (0, CL, CL | HD, CL | NF)
ALPHAS = (1.0, -1.0)
BETAS = (0.0, 0.5)
DTS = ('f32', 'f64')
BATCH_GAP = 8                       # elements between two matrices of a batch, beyond M * ldc
GUARD_WORDS = 8                     # guard elements in front of and behind C
UNROLL = 8                          # REDUCE_UNROLL of csrc/gemm.hip

Case = namedtuple('Case', 'dt M K ldpad batch flags alpha beta')


def case_id(c):
    return f'{c.dt}|M{c.M}|K{c.K}|ld+{c.ldpad}|b{c.batch}|fl{c.flags}|a{c.alpha:g}|b{c.beta:g}'


def _draw(key, values, salt):
    return values[zlib.crc32(f'{salt}|{key}'.encode()) % len(values)]


def _cases():
    out = []
    for rep in (0, 1):
        for M, ldpad, flags, dt in itertools.product(SIZES, (0, 1), FLAGS, DTS):
            key = f'{rep}|{M}|{ldpad}|{flags}|{dt}'
            out.append(Case(dt, M, _draw(key, KS, 'K'), ldpad, _draw(key, BATCHES, 'batch'), flags, _draw(key, ALPHAS, 'alpha'),
                            _draw(key, BETAS, 'beta')))
    for dt, flags, ldpad in itertools.product(DTS, (0, CL), (0, 1)):      # exactly the unroll width
        out.append(Case(dt, 128, 2048, ldpad, '1', flags, 1.0, 0.0))
    for dt in DTS:                                                        # one slice: no reduce
        out.append(Case(dt, 128, 64, 0, '1', CL, 1.0, 0.0))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


CASES = _cases()


def batch_levels(c):
    """(nb1, nb2)"""
    return {'1': (1, 1), '2x1': (2, 1), '1x2': (1, 2)}[c.batch]


def layout(c, ldpad=None, gap=BATCH_GAP):
    """(ldc, stride between the matrices of the batch, elements of the whole buffer with its guards) of C -- or, with another
    ldpad / gap, of the float64 copy"""
    ldc = c.M + (c.ldpad if ldpad is None else ldpad)
    nb = 2 if c.batch != '1' else 1
    stride = c.M * ldc + gap
    return ldc, stride, 2 * GUARD_WORDS + nb * stride


def vector_path(c):
    """reduce_vec_ok of csrc/gemm.hip for this row (bases are 16-byte aligned by construction, the row is square)."""
    ldc, stride, _ = layout(c)
    return c.M % 4 == 0 and ldc % 4 == 0 and (c.batch == '1' or stride % 4 == 0)


def zero_filled_upper(c):
    """The reduce writes zeros into the strict upper triangle."""
    return bool(c.flags & CL) and c.beta == 0.0
