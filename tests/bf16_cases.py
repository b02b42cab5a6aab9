"""The case tables of the exact tests of csrc/gemm_bf16.hip, their seeded input builders and float64 references.  No GPU here.

Four tables, one per entry point:

* `PROJ_CASES` (nsgp_svgp_tri_gemm_colstats_bf16): the smallest shapes at which the two-deep register / LDS pipeline of
  `bf16_proj_kernel` runs every K-tile count nt = 1 .. 7 in BOTH triangle modes.  `proj_path` repeats the host's and the
  kernel's arithmetic (tiles_m, tiles_n, per row tile kbeg, kend, nt) and names what a case reaches;
  tests/test_bf16_cases_cpu.py asserts that the table reaches all of it.  Per row tile of M (lower | upper):
      M =   8: 1 | 1          M = 200: 2,4 | 4,2          M = 328: 2,4,6 | 6,4,2
      M =  72: 2 | 2          M = 264: 2,4,5 | 5,3,1      M = 392: 2,4,6,7 | 7,5,3,1
      M = 136: 2,3 | 3,1      (264 is the only one with nt = 5 in the lower mode: 256 < kend <= 320 needs 256 < M <= 320)
  and M = 128, 256 for whole tiles.
* `CAST_CASES` (nsgp_cast_sq_bf16_f32 / _f64), `TCAST_CASES` (nsgp_transpose_cast_bf16), `RBF_CASES` (nsgp_rbf_build_t_bf16).

Data of a projection case:
  'small'  integers in [-2, 2]: every float32 partial sum of Y and of the column statistics is an integer below 2^24, so the
           kernel's float32 results equal the float64 reference BIT FOR BIT in any summation order;
  'wide'   integers in [-16, 16]: Y is still exact (|sum| <= 256 * 392 < 2^24) and many |Y| exceed 256, where odd integers
           are ties of the bf16 grid -- the transposed bf16 copy then checks round-to-nearest-even; the statistics round;
  'real'   Gaussian operands rounded to bf16.
The triangle's zeros are really in the operands' memory (the kernel's contract: it skips K ranges, it does not mask).
"""
import collections
import functools

BM, BN, BK = 128, 128, 64                 # the tile of bf16_proj_kernel (csrc/gemm_bf16.hip)
LOWER, UPPER = 1, 2

ProjCase = collections.namedtuple('ProjCase', 'tri batch M n rowvec yt data')
CastCase = collections.namedtuple('CastCase', 'dt n batch transpose tril')
TCastCase = collections.namedtuple('TCastCase', 'batch M n')
RbfCase = collections.namedtuple('RbfCase', 'batch M n D shared_x')


def _proj_table():
    out = []
    for tri in (LOWER, UPPER):
        # every nt, every ragged / whole form of M, the n values spread over them
        for M, n in ((8, 1), (72, 127), (136, 129), (200, 128), (264, 200), (328, 129), (392, 200), (128, 128), (256, 127)):
            batch = 3 if (tri, M) in ((LOWER, 136), (UPPER, 200)) else 1
            out.append(ProjCase(tri, batch, M, n, True, True, 'small'))
        out += [ProjCase(tri, 1, M, n, True, True, 'wide') for M, n in ((136, 200), (264, 127), (392, 129))]
        out.append(ProjCase(tri, 1, 392, 200, True, True, 'real'))
    # the optional operands (product 2 of the layer runs with neither)
    out += [ProjCase(LOWER, 1, 136, 129, False, True, 'small'), ProjCase(UPPER, 1, 264, 1, False, True, 'small'),
            ProjCase(LOWER, 1, 264, 127, True, False, 'small'), ProjCase(UPPER, 1, 136, 200, True, False, 'small'),
            ProjCase(UPPER, 1, 392, 129, False, False, 'small')]
    return out


PROJ_CASES = _proj_table()

CAST_CASES = [CastCase(dt, n, 1 + 2 * ((i + f + (dt == 'f64')) % 2), f >> 1, f & 1)
              for dt in ('f32', 'f64') for i, n in enumerate((1, 7, 16, 17, 200)) for f in range(4)]

TCAST_CASES = [TCastCase(*c) for c in ((1, 1, 1), (2, 31, 33), (1, 32, 32), (2, 33, 31), (3, 65, 40), (1, 64, 64), (1, 40, 65),
                                       (1, 200, 129))]

RBF_CASES = [RbfCase(*c) for c in ((1, 1, 1, 1, True), (2, 7, 33, 3, False), (1, 8, 65, 8, True), (3, 13, 33, 1, False),
                                   (2, 8, 1, 3, True), (1, 13, 65, 8, True), (2, 7, 65, 8, False), (2, 200, 1, 1, False),
                                   (1, 200, 33, 3, True), (2, 200, 65, 8, False), (3, 200, 33, 8, True))]


def case_id(c):
    if isinstance(c, ProjCase):
        return (f'{"lower" if c.tri == LOWER else "upper"}|b{c.batch}|M{c.M}|n{c.n}|{c.data}'
                + ('' if c.rowvec else '|norv') + ('' if c.yt else '|noyt'))
    if isinstance(c, CastCase):
        return f'{c.dt}|n{c.n}|b{c.batch}' + ('|T' if c.transpose else '') + ('|tril' if c.tril else '')
    if isinstance(c, TCastCase):
        return f'b{c.batch}|M{c.M}|n{c.n}'
    return f'b{c.batch}|M{c.M}|n{c.n}|D{c.D}|' + ('sharedx' if c.shared_x else 'batchx')


def _cdiv(a, b):
    return -(-a // b)


def proj_tiles(c):
    """(tiles_m, tiles_n, [(kbeg, kend, nt) of every 128-row tile]) as the host and `bf16_proj_kernel` compute them."""
    tiles_m, tiles_n = _cdiv(c.M, BM), _cdiv(c.n, BN)
    rows = []
    for bm in range(tiles_m):
        m0, kbeg, kend = bm * BM, 0, c.M
        if c.tri == LOWER:
            kend = min(m0 + BM, c.M)
        if c.tri == UPPER:
            kbeg = m0 // BK * BK
        rows.append((kbeg, kend, _cdiv(kend - kbeg, BK)))
    return tiles_m, tiles_n, rows


PROJ_TAGS = {'nt1', 'nt2', 'nt3', 'nt4', 'nt5', 'nt6', 'nt_ge7', 'k_tail_chunk', 'ragged_row_tile', 'whole_tiles',
             'ragged_col_tile', 'one_col_tile_narrow', 'several_col_tiles', 'batched', 'lower', 'upper', 'no_rowvec', 'no_yt',
             'with_yt'}
NT_TAGS = ('nt1', 'nt2', 'nt3', 'nt4', 'nt5', 'nt6', 'nt_ge7')


def proj_path(c):
    """What of the kernel a projection case reaches."""
    tiles_m, tiles_n, rows = proj_tiles(c)
    tags = {'nt_ge7' if nt >= 7 else f'nt{nt}' for _, _, nt in rows}
    tags.add('lower' if c.tri == LOWER else 'upper')
    if c.M % BK:
        tags.add('k_tail_chunk')                  # the last K-tile has 16-byte chunks past K: read as zeros
    tags.add('ragged_row_tile' if c.M % BM else 'whole_tiles')
    if c.n % BN:
        tags.add('ragged_col_tile')
    if c.n < BN:
        tags.add('one_col_tile_narrow')
    if tiles_n > 1:
        tags.add('several_col_tiles')
    if c.batch > 1:
        tags.add('batched')
    if not c.rowvec:
        tags.add('no_rowvec')
    tags.add('with_yt' if c.yt else 'no_yt')
    return tags


# ------------------------------------------------------------------------------------------------ projection: inputs, reference

def _seed(c):
    return 1000003 * c.tri + 7919 * c.M + 31 * c.n + c.batch + 101 * ('small', 'wide', 'real').index(c.data)


@functools.lru_cache(maxsize=None)
def proj_inputs(c):
    """(P (batch, M, M) bf16 with the other triangle zero, Qt (batch, n, M) bf16, rowvec (batch, M) float32) on the host.
    The operands do not depend on the rowvec / yt switches of the case; rowvec is returned also where the case passes NULL."""
    import torch
    g = torch.Generator().manual_seed(_seed(c))
    if c.data == 'real':
        P = torch.randn(c.batch, c.M, c.M, generator=g)
        Qt = torch.randn(c.batch, c.n, c.M, generator=g)
        rv = torch.randn(c.batch, c.M, generator=g)
    else:
        a = 2 if c.data == 'small' else 16
        P = torch.randint(-a, a + 1, (c.batch, c.M, c.M), generator=g).float()
        Qt = torch.randint(-a, a + 1, (c.batch, c.n, c.M), generator=g).float()
        rv = torch.randint(-a, a + 1, (c.batch, c.M), generator=g).float()
    P = torch.tril(P) if c.tri == LOWER else torch.triu(P)
    return P.to(torch.bfloat16), Qt.to(torch.bfloat16), rv


def tile_row_sums(t, M):
    """(batch, M, n) -> (batch, ceil(M / 128), n): the sums over the rows of each 128-row tile (float64 in, float64 out)."""
    import torch
    b, _, n = t.shape
    T = _cdiv(M, BM)
    pad = torch.zeros(b, T * BM, n, dtype=t.dtype)
    pad[:, :M] = t
    return pad.reshape(b, T, BM, n).sum(2)


def proj_reference_from(P, Qt, rv, M):
    """The float64 results of the bf16 operands, and the sums of absolute terms that bound any float32 evaluation order:
    Y, absY = |P| |Qt|^T; part_dot, abs_dot = tile-row sums of Y rv, |Y| |rv|; part_sq = tile-row sums of Y^2."""
    Pd, Qd, rd = P.double(), Qt.double(), rv.double().unsqueeze(-1)
    Y = Pd @ Qd.transpose(-1, -2)
    absY = Pd.abs() @ Qd.abs().transpose(-1, -2)
    return dict(Y=Y, absY=absY, part_dot=tile_row_sums(Y * rd, M), abs_dot=tile_row_sums((Y * rd).abs(), M),
                part_sq=tile_row_sums(Y * Y, M))


@functools.lru_cache(maxsize=None)
def proj_reference(c):
    P, Qt, rv = proj_inputs(c)
    return proj_reference_from(P, Qt, rv, c.M)


def summed_range(c):
    """(M,) float64: the K range `bf16_proj_kernel` sums for each output row (kend - kbeg of its row tile)."""
    import torch
    _, _, rows = proj_tiles(c)
    return torch.tensor([rows[m // BM][1] - rows[m // BM][0] for m in range(c.M)], dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ casts: inputs, reference

def planted_values(dt):
    """Values every cast input carries: ties of the bf16 grid in both directions (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6),
    signed zeros and infinities, 3.4e38 (finite in float32, above the largest bf16: -> inf), a float32 subnormal and a NaN.
    float64 adds 1 + 2^-8 + 2^-40 (through float32 it is the tie, -> 1; rounded directly it would be 1 + 2^-7) and
    magnitudes outside float32."""
    v = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0, -0.0, float('inf'), -float('inf'), 3.4e38, -3.4e38,
         1e-40, float('nan')]
    if dt == 'f64':
        v += [1.0 + 2.0 ** -8 + 2.0 ** -40, 1e300, -1e-300]
    return v


def plant(t, dt, start=0):
    """Write the planted values over a contiguous tensor's flat elements 0, 5, 10, ... in place: all of them where they
    fit, else as many as fit, beginning with value number `start` (so that the tiny cases differ in what they carry)."""
    vals = planted_values(dt)
    vals = vals[start % len(vals):] + vals[:start % len(vals)]
    flat = t.reshape(-1)
    for i, v in enumerate(vals[:(flat.numel() + 4) // 5]):
        flat[5 * i] = v
    return t


def _torch_dt(dt):
    import torch
    return torch.float32 if dt == 'f32' else torch.float64


@functools.lru_cache(maxsize=None)
def cast_input(c):
    """(batch, n, n) source of a cast case; with tril a NaN sits above the diagonal (the kernel must not read it)."""
    import torch
    g = torch.Generator().manual_seed(977 * c.n + 13 * c.batch + 2 * c.transpose + c.tril + 5 * (c.dt == 'f64'))
    src = plant(torch.randn(c.batch, c.n, c.n, generator=g, dtype=_torch_dt(c.dt)), c.dt,
                3 * (2 * c.transpose + c.tril) + 5 * (c.dt == 'f64'))
    if c.tril and c.n > 1:
        src[:, 0, c.n - 1] = float('nan')
    return src


def cast_reference(c):
    """dst = op(src) -> float32 -> bf16 (the kernel converts `(__bf16)(float)v`), op = tril, then transpose."""
    import torch
    t = cast_input(c)
    if c.tril:
        t = torch.tril(t)
    if c.transpose:
        t = t.transpose(-1, -2)
    return t.contiguous().to(torch.float32).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def tcast_input(c):
    import torch
    g = torch.Generator().manual_seed(3571 * c.M + 17 * c.n + c.batch)
    return plant(torch.randn(c.batch, c.M, c.n, generator=g), 'f32', c.batch + c.M)


def tcast_reference(c):
    import torch
    return tcast_input(c).transpose(-1, -2).contiguous().to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------ RBF build: inputs, reference

RBF_DELTA = 2.0 ** -15       # relative error allowed to the kernel's float32 evaluation of os exp(-s / 2), derived in rbf_inputs
RBF_MAX_S = 20.0


@functools.lru_cache(maxsize=None)
def rbf_inputs(c):
    """z (batch, M, D), x (n, D) or (batch, n, D), ls (batch, D) in [0.8, 1.6], os (batch,) in [0.5, 1.5], float32.
    With s = sum_d ((x_d - z_d) / ls_d)^2 <= 20 nothing is subnormal (v >= 0.5 e^-10) and the float32 evaluation carries
    about 13 roundings in s -- |d(s / 2)| <= 10 * 13 * 2^-24 ~ 8e-6 -- plus the exp2 path: below RBF_DELTA relative."""
    import torch
    g = torch.Generator().manual_seed(4001 * c.M + 97 * c.n + 7 * c.D + c.batch + 1000 * c.shared_x)
    z = 0.5 * torch.randn(c.batch, c.M, c.D, generator=g)
    x = 0.5 * torch.randn((c.n, c.D) if c.shared_x else (c.batch, c.n, c.D), generator=g)
    ls = 0.8 + 0.8 * torch.rand(c.batch, c.D, generator=g)
    os_ = 0.5 + torch.rand(c.batch, generator=g)
    return z, x, ls, os_


@functools.lru_cache(maxsize=None)
def rbf_reference(c):
    """(s, v) in float64 from the float32 inputs, in the kernel's layout (batch, n, M): v = os exp(-s / 2)."""
    import torch
    z, x, ls, os_ = (t.double() for t in rbf_inputs(c))
    xb = x if x.dim() == 3 else x.unsqueeze(0).expand(c.batch, c.n, c.D)
    s = (((xb.unsqueeze(2) - z.unsqueeze(1)) / ls.reshape(c.batch, 1, 1, c.D)) ** 2).sum(-1)
    return s, os_.reshape(c.batch, 1, 1) * torch.exp(-0.5 * s)


def rbf_restated_f32(c):
    """The kernel's arithmetic restated in float32 on the host (reciprocal lengthscale, sum in d order, exp)."""
    import torch
    z, x, ls, os_ = rbf_inputs(c)
    xb = x if x.dim() == 3 else x.unsqueeze(0).expand(c.batch, c.n, c.D)
    il = (1.0 / ls).reshape(c.batch, 1, 1, c.D)
    s = torch.zeros(c.batch, c.n, c.M)
    for d in range(c.D):
        t = (xb[:, :, None, d] - z[:, None, :, d]) * il[..., d]
        s = s + t * t
    return os_.reshape(c.batch, 1, 1) * torch.exp(-0.5 * s)


def bf16_neighbours(v):
    """For positive normal float64 v: (lo, hi, mid) with lo <= v < hi consecutive bf16 numbers, all exact in float64."""
    import torch
    _, ex = torch.frexp(v)                                   # v = m 2^ex, m in [0.5, 1): bf16 spacing 2^(ex - 8)
    ulp = torch.ldexp(torch.ones_like(v), ex - 8)
    lo = torch.floor(v / ulp) * ulp
    return lo, lo + ulp, lo + 0.5 * ulp


def rbf_verdict(c, got):
    """got: the kernel's (batch, n, M) output as float64.  Returns (neighbour, nearest, decided): per element, whether got
    is one of v's two bf16 neighbours; whether it is the nearer one; whether v is farther than RBF_DELTA v from the midpoint
    (where the nearer one is required)."""
    _, v = rbf_reference(c)
    lo, hi, mid = bf16_neighbours(v)
    neighbour = (got == lo) | (got == hi)
    nearest = got == (lo + (hi - lo) * (v > mid))
    decided = (v - mid).abs() > RBF_DELTA * v
    return neighbour, nearest, decided
