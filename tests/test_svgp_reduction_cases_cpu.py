"""Case tables, input builders and float64 references for the SVGP / DSVI reductions (csrc/svgp.hip) and the small kernels
of csrc/misc.hip, with the host-side checks of the tables (no GPU).  tests/test_gpu_svgp_reductions.py imports everything
from here and runs every row on the GPU.

The tables exist to hit the loop and launch boundaries of the kernels.  `gauss_blocks` and `kl_blocks` restate the two grid
formulas of csrc/svgp.hip; the `test_*_table_*` tests below assert that every boundary is present, so deleting a boundary
row fails here, without a GPU.

How a result is judged (three methods, strongest first):

* exact -- inputs are small integers and every scale a power of two, so every partial sum, in any order, is a multiple of a
  power of two q of magnitude below 2^24 q: exact in float32 and float64, and the float64 reference IS the answer
  (`torch.equal`).  `test_exact_cases_stay_below_2_to_24` asserts sum |term| / q < 2^24 from the reference alone.
* bound -- where a term holds a log, a division or a square root.  A reduction of N terms, each evaluated with at most c
  roundings, in any summation order satisfies |got - ref| <= (N + c) u sum_i |t_i|  (u = 2^-24 / 2^-53; Higham, Accuracy and
  Stability of Numerical Algorithms, section 4.2: N - 1 additions at most on the path of any term, plus the c roundings of the
  term itself, first order in u).  sum |t_i| is taken over the elementary pieces of the reference (`*_abs` below), so
  cancellation inside a term does not shrink it.  `red_tol` is that bound; c is stated where it is used.  With N = 1 this
  is the element-wise bound c u |t|, which is why c cannot be left out.
  Such a bound cannot show one dropped element among 66 000 float32 terms, so the inputs carry SPIKES: one large value at
  the first and last element and on both sides of the boundaries the case is about.  `test_spikes_are_visible` asserts, from
  the reference alone, that removing any single probed term moves the float64 reference by more than 4x the tolerance the
  GPU test uses.  It is a condition on the inputs: `spike` solves it for the spike value.
* bit-equality between two paths that run the same arithmetic (fused Adam).

All builders return float64 CPU tensors whose values are exactly representable in float32, so both dtypes see the same
numbers.  Builders are deterministic (seeded by the case).
"""
import collections
import math
import zlib

import pytest
import torch

DTYPES = {'f32': torch.float32, 'f64': torch.float64}
U = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
EXACT_LIMIT = 2.0 ** 24
L2PI = math.log(2.0 * math.pi)


def cdiv(a, b):
    return -(-a // b)


def gauss_blocks(n):
    """csrc/svgp.hip gauss_blocks: blocks per sample row of the likelihood partial sums; each strides by nblk * 256."""
    return min(max(cdiv(n, 1024), 1), 64)


def kl_blocks(M):
    """csrc/svgp.hip kl_blocks: blocks per batch element of the KL partial sums; rows stride by nblk, columns by 256."""
    return min(max(cdiv(M * M, 1024), 1), 256)


def kl_diag_blocks(tot):
    """csrc/svgp.hip kl_diag_blocks: blocks of the mean-field KL's partial sums over all batch * M elements; each strides by
    nblk * 256."""
    return min(cdiv(tot, 1024), 256)


def rowdot_chunks(n, dt):
    """rowdot_affine_kernel: chunks of 256 lanes x 16 bytes per row."""
    return cdiv(n, 256 * (4 if dt == 'f32' else 2))


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).double()


def normal32(shape, g, scale=1.0):
    return (scale * torch.randn(tuple(shape), generator=g, dtype=torch.float32)).double()


def uniform32(shape, g, lo, hi):
    return (lo + (hi - lo) * torch.rand(tuple(shape), generator=g, dtype=torch.float32)).float().double()


def red_tol(n_terms, c, dt, abs_sum):
    """(N + c) u sum |t_i|: see the module docstring."""
    return (n_terms + c) * U[dt] * abs_sum


def spike(n_terms, c, base_abs, k, unit=1.0, even=False):
    """Power of two V such that a term of magnitude unit * V, present k times next to terms of absolute sum base_abs, is more
    than 4 x red_tol(float32) of the whole sum: unit V > a (base_abs + k unit V), a = 4 (N + c) u, i.e. V above
    a base_abs / ((1 - a k) unit); the next power of two but one is taken.  even: an even exponent (the caller takes the root)."""
    a = 4.0 * (n_terms + c) * U['f32']
    assert a * k < 1.0, f'{k} probes are too many for {n_terms} float32 terms'
    e = max(math.ceil(math.log2(a * max(base_abs, 1.0) / (1.0 - a * k) / unit)) + 1, 4)
    return 2.0 ** (e + (e % 2 if even else 0))


# ---------------------------------------------------------------------------------------------------------------------------
# Gaussian expected log-likelihood
# ---------------------------------------------------------------------------------------------------------------------------
GaussCase = collections.namedtuple('GaussCase', 'n S')
GAUSS_N = (1, 255, 256, 257, 1024, 1025, 65536, 65537, 66563)
# GAUSS_CASES_BEGIN
GAUSS_CASES = [GaussCase(n, S) for n in GAUSS_N for S in (1, 5)]
# GAUSS_CASES_END
GAUSS_GOUT = (1.0, 1.5, 1.25, 1.75, 1.125)               # per-sample upstream gradient of the vector form
GAUSS_UP = -1.5                                          # scalar upstream gradient of the total form
# roundings of one term -1/2 ((y - mu)^2 + v) / s2 + log s2 + log 2pi) as the kernel evaluates it: y - mu, d d, + v, 1 / s2,
# e is2, log (2 ulp), + ls2, the constant log 2pi, + l2pi; then the block's partial times gout, the total times scale
C_GAUSS = 12


def gauss_terms(y, mu, v, s2):
    """(term, |pieces| of the term, noise-gradient term, |pieces| of it), each (S, n), float64."""
    e = (y - mu) ** 2 + v
    ls2 = math.log(s2)
    return (-0.5 * (e / s2 + ls2 + L2PI), 0.5 * (e / s2 + abs(ls2) + L2PI),
            0.5 * (e / s2 ** 2 - 1.0 / s2), 0.5 * (e / s2 ** 2 + 1.0 / s2))


def gauss_probes(n, S):
    """(s, i) of the spikes: first and last element, both sides of the two largest of the boundaries 256 (one block's lanes),
    1024 (one block's share), nblk * 256 (the grid stride) and 65536 (the cap of 64 blocks) below n, the corners of the last
    sample row, and both sides of partial 255 | 256 of the `total` reduction where S * nblk > 256."""
    nblk = gauss_blocks(n)
    cols = {0, n - 1}
    for B in sorted(b for b in {256, 1024, nblk * 256, 65536} if b < n)[-2:]:
        cols |= {B - 1, B}
    probes = {(0, c) for c in cols} | {(S - 1, 0), (S - 1, n - 1)}
    if S * nblk > 256:
        probes |= {(p // nblk, (p % nblk) * 256) for p in (255, 256)}
    return sorted(probes)


def gauss_inputs(case, mode):
    """mode 'bound': seeded normal data, noise 0.6875, spikes in v.  mode 'int': integers, noise 1 (log s2 = 0, 1 / s2 = 1):
    the noise gradient's terms 1/2 (e - 1) gout and the element-wise gradients are exact."""
    n, S = case
    g = gen(f'gauss-{n}-{S}-{mode}')
    if mode == 'int':
        return dict(y=ints((n,), g, -2, 2), mu=ints((S, n), g, -2, 2), v=ints((S, n), g, 0, 3), noise=1.0, scale=0.5,
                    gout=ints((S,), g, 1, 2), up=2.0, probes=[])
    y, mu, v = normal32((n,), g), normal32((S, n), g), uniform32((S, n), g, 0.5, 1.5)
    noise, scale = 0.6875, -0.375
    probes = gauss_probes(n, S)
    V = spike(S * n, C_GAUSS, float(gauss_terms(y, mu, v, noise)[1].sum()), len(probes), 0.5 / noise)
    for s, i in probes:
        v[s, i] = V
    return dict(y=y, mu=mu, v=v, noise=noise, scale=scale, gout=torch.tensor(GAUSS_GOUT[:S], dtype=torch.float64),
                up=GAUSS_UP, probes=probes)


# ---------------------------------------------------------------------------------------------------------------------------
# whitened KL
# ---------------------------------------------------------------------------------------------------------------------------
KlCase = collections.namedtuple('KlCase', 'M batch')
KL_M = (1, 2, 31, 32, 33, 256, 257, 512, 513, 520)
# KL_CASES_BEGIN
KL_CASES = [KlCase(M, b) for M in KL_M for b in (1, 3)]
# KL_CASES_END
KL_SCALE, KL_UP = -0.25, 1.5
# roundings of the pieces l^2, m^2, -2 log |l| (log: 2 ulp, times 2 exact) and of the tail 1/2 s, scale, + const, + addin
C_KL = 8


def kl_terms_count(M):
    return M * (M + 1) // 2 + 2 * M + 1                   # l_ij^2 (j <= i), m_i^2, log |l_ii|, the constant -M / 2


def kl_reference(m, L):
    """m:(b, M), L:(b, M, M) with zeros above the diagonal -> (KL_b:(b,), sum of |pieces| per b)."""
    M = m.shape[1]
    ld = torch.diagonal(L, dim1=-2, dim2=-1).abs().log()
    sq = (L ** 2).sum((1, 2)) + (m ** 2).sum(1)
    return 0.5 * (sq - 2.0 * ld.sum(1) - M), 0.5 * (sq + 2.0 * ld.abs().sum(1) + M)


def kl_grad_reference(m, L, go):
    """(gm, gLq, element-wise magnitude of gLq's pieces |go| (|l| + |1/l| on the diagonal))."""
    eye = torch.eye(L.shape[-1], dtype=torch.bool)
    inv = torch.where(eye, 1.0 / torch.where(eye, L, torch.ones_like(L)), torch.zeros_like(L))
    return go * m, go * (L - inv), abs(go) * (L.abs() + inv.abs())


def kl_probes(M, batch):
    """(b, i, j) of the spikes: the corners of the triangle, both sides of column 255 | 256 (second trip of the j loop),
    rows nblk - 1 | nblk (a block's second row), the last element of the last batch entry, and both sides of partial
    255 | 256 of the `total` reduction where batch * nblk > 256."""
    nblk = kl_blocks(M)
    p = {(0, 0, 0), (0, M - 1, M - 1), (batch - 1, M - 1, M - 1)}
    p |= {(0, M - 1, 255), (0, M - 1, 256)} if M > 256 else {(0, M - 1, 0)}
    if nblk < M:
        p |= {(0, nblk - 1, 0), (0, nblk, 0)}
    if batch * nblk > 256:
        p |= {(0, 255, 0), (1, 0, 0)}
    return sorted(p)


def kl_inputs(case, mode):
    """L: clean lower factor; L_given: the same with NaN in the strict upper triangle (never read).  mode 'int': integer
    entries, diagonal +-1 (log |l| = 0 exactly).  mode 'bound': normal entries, diagonal magnitudes in [0.5, 1.5] with random
    signs, spikes."""
    M, batch = case
    g = gen(f'kl-{M}-{batch}-{mode}')
    sign = 2.0 * torch.randint(0, 2, (batch, M), generator=g).double() - 1.0
    if M > 1:
        sign[:, 0], sign[:, 1] = -1.0, 1.0
    else:
        sign[0, 0] = -1.0
    if mode == 'int':
        m, L, diag, probes = ints((batch, M), g), torch.tril(ints((batch, M, M), g), -1), sign, []
        scale, addin, up = 0.5, 3.0, 2.0
    else:
        m, L = normal32((batch, M), g), torch.tril(normal32((batch, M, M), g, 0.3), -1)
        diag = sign * uniform32((batch, M), g, 0.5, 1.5)
        scale, addin, up = KL_SCALE, 0.40625, KL_UP
        probes = kl_probes(M, batch)
    L = L + torch.diag_embed(diag)
    if probes:
        base = float(kl_reference(m, L)[1].sum())
        V = math.sqrt(spike(batch * kl_terms_count(M), C_KL, base, len(probes), 0.5, even=True))
        for b, i, j in probes:
            L[b, i, j] = -V if i == j and sign[b, i] < 0 else V
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    L_given = torch.where(upper, torch.full_like(L, float('nan')), L)
    return dict(m=m, L=L, L_given=L_given, scale=scale, addin=addin, up=up, probes=probes)


# ---------------------------------------------------------------------------------------------------------------------------
# mean-field KL (bit record only: tests/test_gpu_meanfield.py holds its values to the oracle)
# ---------------------------------------------------------------------------------------------------------------------------
MfKlCase = collections.namedtuple('MfKlCase', 'batch M')
# MF_KL_CASES_BEGIN
MF_KL_CASES = [MfKlCase(b, M) for b, M in ((1, 1), (1, 255), (1, 257), (1, 1024), (1, 1025), (3, 342), (2, 131073))]
# MF_KL_CASES_END
# value and gradients as tests/test_gpu_meanfield.py::test_mean_field_kl_matches_oracle_and_accumulates judges them
MF_KL_TOL = {'f32': dict(rtol=2e-5, atol=1e-6), 'f64': dict(rtol=1e-12, atol=1e-13)}


def mf_kl_inputs(case):
    """m normal, variances s2 uniform in [0.25, 2.25]; scale, addin and upstream gradient of the whitened KL's total form."""
    g = gen(f'mfkl-{case.batch}-{case.M}')
    return dict(m=normal32(case, g), s2=uniform32(case, g, 0.25, 2.25), scale=KL_SCALE, addin=0.40625, up=KL_UP)


def mf_kl_reference(P):
    """(sum_b KL(N(m_b, diag(s2_b)) || N(0, I)), gm, gs2 for a unit upstream factor), float64."""
    m, s2 = P['m'], P['s2']
    return float(0.5 * ((s2 - 1.0) - s2.log() + m * m).sum()), m, 0.5 * (1.0 - 1.0 / s2)


# ---------------------------------------------------------------------------------------------------------------------------
# fused DSVI objective
# ---------------------------------------------------------------------------------------------------------------------------
# squeeze: groups of batch 1 are handed over as (M,) / (M, M).  up: the upstream gradient of the scalar.
ObjCase = collections.namedtuple('ObjCase', 'name n S M batches squeeze noise_grad up')
# OBJ_CASES_BEGIN
OBJ_CASES = [
    ObjCase('g0-n1025', 1025, 2, 0, (), False, True, 0.5),
    ObjCase('g1-M1-n1', 1, 1, 1, (1,), True, False, -2.0),
    ObjCase('g3-M33-ragged-blocks', 1025, 3, 33, (1, 3, 2), True, True, 0.75),
    ObjCase('g8-M33-n65537', 65537, 2, 33, (1, 2, 1, 3, 1, 1, 2, 1), False, False, 1.5),
    ObjCase('g2-M257', 1025, 5, 257, (2, 1), False, True, -0.5),
]
# OBJ_CASES_END
OBJ_MAX_GROUPS = 8
OBJ_NOISE, OBJ_ELL_SCALE, OBJ_KL_SCALE = 0.5, -0.125, 0.5


def obj_terms_count(case):
    return case.S * case.n + sum(case.batches) * (kl_terms_count(case.M) if case.batches else 0)


def obj_inputs(case):
    """Likelihood operands and one (m, L, L_given) per group; spikes at the first and last likelihood element and at the first
    element of the first group and the last of the last."""
    g = gen('obj-' + case.name)
    n, S, M = case.n, case.S, case.M
    y, mu, v = normal32((n,), g), normal32((S, n), g), uniform32((S, n), g, 0.5, 1.5)
    groups = []
    for b in case.batches:
        sign = 2.0 * torch.randint(0, 2, (b, M), generator=g).double() - 1.0
        L = torch.tril(normal32((b, M, M), g, 0.3), -1) + torch.diag_embed(sign * uniform32((b, M), g, 0.5, 1.5))
        groups.append([normal32((b, M), g), L])
    base = abs(OBJ_ELL_SCALE) * float(gauss_terms(y, mu, v, OBJ_NOISE)[1].sum()) \
        + abs(OBJ_KL_SCALE) * sum(float(kl_reference(m, L)[1].sum()) for m, L in groups)
    ell_probes = sorted({(0, 0), (S - 1, n - 1)})
    kl_pr = sorted({(0, 0, 0, 0), (len(groups) - 1, case.batches[-1] - 1, M - 1, M - 1)}) if groups else []
    X = spike(obj_terms_count(case), C_GAUSS + C_KL, base, len(ell_probes) + len(kl_pr), 1.0, even=True)
    for s, i in ell_probes:                              # term |ell_scale| V / (2 noise) = X
        v[s, i] = X * 2.0 * OBJ_NOISE / abs(OBJ_ELL_SCALE)
    for gi, b, i, j in kl_pr:                            # term |kl_scale| l^2 / 2 = X
        groups[gi][1][b, i, j] = math.sqrt(X * 2.0 / abs(OBJ_KL_SCALE))
    upper = torch.triu(torch.ones(M, M, dtype=torch.bool), 1)
    groups = [(m, L, torch.where(upper, torch.full_like(L, float('nan')), L)) for m, L in groups]
    return dict(y=y, mu=mu, v=v, noise=OBJ_NOISE, ell_scale=OBJ_ELL_SCALE, kl_scale=OBJ_KL_SCALE, groups=groups,
                ell_probes=ell_probes, kl_probes=kl_pr)


def obj_reference(P):
    """(value, sum of |pieces|, (S, n) scaled likelihood terms, per group (b,) scaled KL) of the closed form."""
    t, a, _, _ = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
    val, ab = P['ell_scale'] * t.sum(), abs(P['ell_scale']) * a.sum()
    for m, L, _ in P['groups']:
        k, ka = kl_reference(m, L)
        val, ab = val + P['kl_scale'] * k.sum(), ab + abs(P['kl_scale']) * ka.sum()
    return float(val), float(ab), P['ell_scale'] * t


# ---------------------------------------------------------------------------------------------------------------------------
# the objective's bit record (tools/record_objective_hashes.py, tests/test_gpu_objective_bits.py)
# ---------------------------------------------------------------------------------------------------------------------------
# (kind, row of the kind's table, dtype): every row above that feeds an entry point of the DSVI objective, in both dtypes
OBJECTIVE_BITS_CASES = [(kind, c, dt) for kind, table in (('gauss', GAUSS_CASES), ('kl', KL_CASES), ('obj', OBJ_CASES),
                                                          ('mfkl', MF_KL_CASES)) for c in table for dt in DTYPES]


def objective_bits_id(run):
    kind, c, dt = run
    return '-'.join([kind] + ([c.name] if kind == 'obj' else [str(f) for f in c]) + [dt])


# ---------------------------------------------------------------------------------------------------------------------------
# rowdot / rowdot_affine (exact)
# ---------------------------------------------------------------------------------------------------------------------------
# drop: which of gv / out_1 / out_x is absent.  off: which operand starts one element into its buffer.
RowdotCase = collections.namedtuple('RowdotCase', 'n batch M D shared drop off')
ROWDOT_N = (4, 1000, 2052, 3076, 7168, 7172, 7176, 9220)
ROWDOT_ODD_N = (769, 1793, 2051)


def _rows_for(n):
    return rowdot_chunks(n, 'f64') + 1                    # every i % nch and one wrap, for both dtypes


def _rowdot_cases():
    rows = []
    for k, n in enumerate(ROWDOT_N + ROWDOT_ODD_N):
        for shared in (0, 1):
            rows.append(RowdotCase(n, 2, _rows_for(n), (1, 3)[(k + shared) % 2], shared, None, None))
    for drop in ('gv', 'out_1', 'out_x'):
        for n, shared in ((1000, 0), (2051, 1), (7176, 0)):
            rows.append(RowdotCase(n, 2, _rows_for(n), 3, shared, drop, None))
    for off in ('A', 'g', 'gv'):
        for n in (1000, 7176, 9220):
            rows.append(RowdotCase(n, 2, _rows_for(n), 3, 0, None, off))
    return rows


# ROWDOT_CASES_BEGIN
ROWDOT_CASES = _rowdot_cases()
PLAIN_ROWDOT_CASES = [(n, off) for n in ROWDOT_N + ROWDOT_ODD_N for off in (None, 'A', 'g')]
# ROWDOT_CASES_END


def rowdot_inputs(n, batch, M, D, tag):
    g = gen(f'rowdot-{n}-{batch}-{M}-{D}-{tag}')
    return dict(A=ints((batch, M, n), g), g=ints((batch, n), g), gv=ints((batch, n), g), x=ints((batch, n, D), g))


def rowdot_real_inputs(n, batch, M, D, tag):
    """The same operands with seeded normal values: a changed summation order shows in the bits (the layer's bit record)."""
    g = gen(f'rowdot-real-{n}-{batch}-{M}-{D}-{tag}')
    return dict(A=normal32((batch, M, n), g), g=normal32((batch, n), g), gv=normal32((batch, n), g),
                x=normal32((batch, n, D), g))


def rowdot_reference(P, shared):
    """out:(b, M), out_gv:(b,), out_1:(nb,), out_x:(nb, D) with nb = 1 when the mean parameters are shared."""
    out = torch.einsum('bmn,bn->bm', P['A'], P['g'])
    o1, ox = P['g'].sum(1), torch.einsum('bnd,bn->bd', P['x'], P['g'])
    if shared:
        o1, ox = o1.sum(0, keepdim=True), ox.sum(0, keepdim=True)
    return dict(out=out, out_gv=P['gv'].sum(1), out_1=o1, out_x=ox)


# ---------------------------------------------------------------------------------------------------------------------------
# colstats, colstats_bwd, the three finalize forms (exact)
# ---------------------------------------------------------------------------------------------------------------------------
ColstatsCase = collections.namedtuple('ColstatsCase', 'M n batch')
# COLSTATS_CASES_BEGIN
COLSTATS_CASES = [ColstatsCase(M, n, 2) for M in (1, 2, 3, 4, 5, 7, 100) for n in (1, 63, 64, 65, 333)]
# COLSTATS_CASES_END


def colstats_inputs(case):
    M, n, b = case
    g = gen(f'colstats-{M}-{n}-{b}')
    return dict(A=ints((b, M, n), g), C=ints((b, M, n), g), m=ints((b, M), g), base=ints((b,), g, 0, 8),
                gmean=ints((b, n), g), gvar=ints((b, n), g))


def colstats_real_inputs(case):
    M, n, b = case
    g = gen(f'colstats-real-{M}-{n}-{b}')
    return dict(A=normal32((b, M, n), g), C=normal32((b, M, n), g), m=normal32((b, M), g), base=uniform32((b,), g, 0.5, 2.0),
                gmean=normal32((b, n), g), gvar=normal32((b, n), g))


def colstats_reference(P):
    A, C, m = P['A'], P['C'], P['m']
    g1, g2 = P['gmean'].unsqueeze(1), 2.0 * P['gvar'].unsqueeze(1)
    return dict(mean=torch.einsum('bmn,bm->bn', A, m), var=P['base'].unsqueeze(1) + (C * C - A * A).sum(1),
                Abar=m.unsqueeze(2) * g1 - g2 * A, C2=g2 * C, mbar=torch.einsum('bmn,bn->bm', A, P['gmean']))


# form: 'plain' (nsgp_svgp_colstats_finalize), 'affine' (..._finalize_affine), 'p64' (..._finalize_affine_p64_f32)
FinalizeCase = collections.namedtuple('FinalizeCase', 'form tiles n has_w has_c shared')
FIN_TILES, FIN_N = (1, 2, 7), (1, 255, 256, 257)
_FIN_COMBOS = ((1, 1, 0), (1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1))
P64_BIG = 2.0 ** 25


def _finalize_cases():
    rows = []
    for k, (tiles, n) in enumerate((t, n) for t in FIN_TILES for n in FIN_N):
        rows.append(FinalizeCase('plain', tiles, n, 0, 0, 0))
        rows.append(FinalizeCase('affine', tiles, n, *_FIN_COMBOS[k % len(_FIN_COMBOS)]))
        rows.append(FinalizeCase('p64', tiles, n, 1, 1, k % 2))
    return rows


# FINALIZE_CASES_BEGIN
FINALIZE_CASES = _finalize_cases()
# FINALIZE_CASES_END
FIN_BATCH, FIN_D, FIN_BASE_ADD = 2, 3, 0.25


def finalize_inputs(case):
    """Partials (b, tiles, n), base (b,), x (b, n, D), w (nb, D), c (nb,), nb = 1 when shared.  p64: the float64 partials
    carry 2^25 + 1/2 against -2^25, so their sums are not float32 numbers until the last step: rounding a partial, the
    running sum, or the sum before c is added, to float32 loses the 1/2 (float32 numbers are 4 apart there)."""
    b, D = FIN_BATCH, FIN_D
    g = gen('finalize-' + '-'.join(str(f) for f in case))
    P = dict(pdot=ints((b, case.tiles, case.n), g), psqA=ints((b, case.tiles, case.n), g, 0, 8),
             psqC=ints((b, case.tiles, case.n), g, 0, 8), base=ints((b,), g, 0, 8), x=ints((b, case.n, D), g))
    nb = 1 if case.shared else b
    P['w'] = ints((nb, D), g) if case.has_w else None
    P['c'] = ints((nb,), g) if case.has_c else None
    if case.form == 'p64':
        P['pdot'][:, 0] += P64_BIG + 0.5
        P['c'] = 4.0 * P['c'] - P64_BIG                  # (a float32 number: they are 2 apart below 2^25, 4 above)
        P['psqC'][:, 0] += P64_BIG + 0.5
        P['psqA'][:, -1] += P64_BIG
    return P


def finalize_real_inputs(case):
    """The same operands with seeded real values.  p64: the float64 partials are products of two float32 numbers, so they
    are no float32 numbers themselves."""
    b, D = FIN_BATCH, FIN_D
    g = gen('finalize-real-' + '-'.join(str(f) for f in case))
    shape = (b, case.tiles, case.n)
    P = dict(pdot=normal32(shape, g), psqA=uniform32(shape, g, 0.0, 4.0), psqC=uniform32(shape, g, 0.0, 4.0),
             base=uniform32((b,), g, 0.5, 2.0), x=normal32((b, case.n, D), g))
    nb = 1 if case.shared else b
    P['w'] = normal32((nb, D), g) if case.has_w else None
    P['c'] = normal32((nb,), g) if case.has_c else None
    if case.form == 'p64':
        for k in ('pdot', 'psqA', 'psqC'):
            P[k] = P[k] * uniform32(shape, g, 0.5, 1.5)
    return P


def finalize_reference(case, P):
    mean = P['pdot'].sum(1)
    if P['w'] is not None:
        mean = mean + torch.einsum('bnd,bd->bn', P['x'], P['w'].expand(FIN_BATCH, -1))
    if P['c'] is not None:
        mean = mean + P['c'].expand(FIN_BATCH).unsqueeze(1)
    base_add = 0.0 if case.form == 'plain' else FIN_BASE_ADD
    return mean, (P['base'].unsqueeze(1) + base_add) + (P['psqC'].sum(1) - P['psqA'].sum(1))


# ---------------------------------------------------------------------------------------------------------------------------
# sampling, Adam, cast / phi_sym / scale_diag
# ---------------------------------------------------------------------------------------------------------------------------
SampleCase = collections.namedtuple('SampleCase', 'S n b ns')
# SAMPLE_CASES_BEGIN
SAMPLE_CASES = sorted({SampleCase(S, n, b, ns) for S, n, b in ((1, 1, 1), (4, 77, 2), (3, 256, 1), (2, 257, 3))
                       for ns in (1, S)})
# SAMPLE_CASES_END


def sample_inputs(case):
    S, n, b, ns = case
    g = gen(f'sample-{S}-{n}-{b}-{ns}')
    return dict(mean=normal32((b, ns, n), g), var=uniform32((b, ns, n), g, 0.25, 4.0), eps=normal32((S, n, b), g),
                gh=ints((S, n, b), g))


def sample_reference(P, ns):
    """h, gmean (exact on the integer gh), gvar and the sum of |terms| of gvar."""
    mean, var = P['mean'].permute(1, 2, 0), P['var'].permute(1, 2, 0)          # (ns, n, b), broadcast over S if ns == 1
    h = mean + var.sqrt() * P['eps']
    t = P['gh'] * P['eps'] * (0.5 / var.sqrt())
    red = (lambda q: q.sum(0, keepdim=True)) if ns == 1 else (lambda q: q)
    back = lambda q: q.permute(2, 0, 1).contiguous()                           # noqa: E731
    return dict(h=h, h_mag=mean.abs() + (var.sqrt() * P['eps']).abs(), gmean=back(red(P['gh'])), gvar=back(red(t)),
                gvar_abs=back(red(t.abs())))


def sample_real_inputs(case):
    """sample_inputs with a seeded normal upstream gradient (the layer's bit record)."""
    P = sample_inputs(case)
    P['gh'] = normal32(P['gh'].shape, gen('sample-real-' + '-'.join(str(f) for f in case)))
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# mean-field column statistics: diag_colsq, colstats_finalize_diag, diag_bwd (bit record only: tests/test_gpu_meanfield.py
# holds their values to the oracle)
# ---------------------------------------------------------------------------------------------------------------------------
# csrc/svgp.hip: rows of A per partial of diag_colsq, columns of A per workgroup of diag_bwd, bytes per lane of the vector forms
DIAG_ROWS, DIAG_BWD_COLS, VEC_LANE_BYTES = 32, 4096, 16
DIAG_BATCH = 2
DIAG_M = (1, 31, 32, 33, 65)
DIAG_N = (1, 5, 512, 516, 1024, 1028, 4096, 4100, 8195)
DIAG_OFFS = (None, 'A', 'gmean')
# off: the operand that starts one element into its buffer ('gmean': the backward pass alone leaves its vector kernel).
# extra: tile rows of diag_colsq's partial buffer beyond nsgp_svgp_diag_tiles(M) (they must come out as zeros).
DiagCase = collections.namedtuple('DiagCase', 'M n off extra')
DiagFinCase = collections.namedtuple('DiagFinCase', 'tiles qtiles n has_w has_c shared')


def diag_tiles(M):
    """csrc/svgp.hip nsgp_svgp_diag_tiles."""
    return cdiv(M, DIAG_ROWS)


def diag_vec(dt):
    """Elements per lane of the vector forms."""
    return VEC_LANE_BYTES // (4 if dt == 'f32' else 8)


def diag_groups(n, dt, vec):
    """diag_colsq_kernel: column groups of 256 lanes (grid.x)."""
    return cdiv(n, 256 * (diag_vec(dt) if vec else 1))


def diag_form(case, dt):
    """The launch form a row reaches: 'vec', 'scalar-n' (n no multiple of the lane's elements), 'scalar-A' (A misaligned:
    both passes), 'scalar-g' (gmean misaligned: the backward pass only)."""
    if case.n % diag_vec(dt):
        return 'scalar-n'
    return {None: 'vec', 'A': 'scalar-A', 'gmean': 'scalar-g'}[case.off]


def _diag_cases():
    """Every n with every operand offset, every M with every launch form (at n = 516: the vector kernels in both dtypes,
    n = 8195: the scalar ones), M and the extra tile row rotating; not the cross product."""
    rows = {DiagCase(DIAG_M[(k + j) % len(DIAG_M)], n, off, (k + j) % 2)
            for k, n in enumerate(DIAG_N) for j, off in enumerate(DIAG_OFFS)}
    rows |= {DiagCase(M, n, off, (i + j + q + 1) % 2)
             for i, M in enumerate(DIAG_M) for q, n in enumerate((516, 8195)) for j, off in enumerate(DIAG_OFFS)}
    return sorted(rows, key=lambda c: (c.n, c.M, str(c.off), c.extra))


# DIAG_CASES_BEGIN
DIAG_CASES = _diag_cases()
DIAG_FIN_CASES = [DiagFinCase(t, q, FIN_N[(i + k) % len(FIN_N)], *combo)
                  for i, (t, q) in enumerate((t, q) for t in (1, 7) for q in (1, 3)) for k, combo in enumerate(_FIN_COMBOS)]
# DIAG_CASES_END


def diag_inputs(case):
    """A (b, M, n), s2m1 = s^2 - 1 of both signs, m, and the upstream gradients of mean and var."""
    b, g = DIAG_BATCH, gen('diag-' + '-'.join(str(f) for f in case))
    return dict(A=normal32((b, case.M, case.n), g), s2m1=uniform32((b, case.M), g, -0.75, 1.25), m=normal32((b, case.M), g),
                gmean=normal32((b, case.n), g), gvar=normal32((b, case.n), g))


def diag_fin_inputs(case):
    """finalize_inputs' operands with seeded real values; pq: the float64 partials of diag_colsq, of both signs and no
    float32 numbers."""
    b, D = FIN_BATCH, FIN_D
    g = gen('diagfin-' + '-'.join(str(f) for f in case))
    P = dict(pdot=normal32((b, case.tiles, case.n), g),
             pq=normal32((b, case.qtiles, case.n), g) * uniform32((b, case.qtiles, case.n), g, 0.5, 1.5),
             base=uniform32((b,), g, 0.5, 2.0), x=normal32((b, case.n, D), g))
    nb = 1 if case.shared else b
    P['w'] = normal32((nb, D), g) if case.has_w else None
    P['c'] = normal32((nb,), g) if case.has_c else None
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# the layer reductions' bit record (tools/record_layer_reduction_hashes.py, tests/test_gpu_layer_reduction_bits.py)
# ---------------------------------------------------------------------------------------------------------------------------
# the float64 layer has no float64-partials form
FINALIZE_RUNS = [(c, dt) for c in FINALIZE_CASES for dt in DTYPES if not (c.form == 'p64' and dt == 'f64')]
# (kind, row of the kind's table, dtype): every row above that feeds an entry point of the layer half of csrc/svgp.hip
LAYER_BITS_CASES = [(kind, c, dt) for kind, table in (('rowdot_affine', ROWDOT_CASES), ('rowdot', PLAIN_ROWDOT_CASES),
                                                      ('colstats', COLSTATS_CASES), ('sample', SAMPLE_CASES),
                                                      ('diag', DIAG_CASES), ('diag_fin', DIAG_FIN_CASES))
                    for c in table for dt in DTYPES] + [('finalize', c, dt) for c, dt in FINALIZE_RUNS]


def layer_bits_id(run):
    kind, c, dt = run
    return '-'.join([kind] + [str(f) for f in c] + [dt])


# align: 'aligned' all four buffers 16-byte aligned, 'all_off' all start one element in, 'g_off' only the gradient
AdamCase = collections.namedtuple('AdamCase', 'n align grad_scale')
ADAM_N = (1, 3, 4, 5, 1023, 1024, 1025, 10001)
# ADAM_CASES_BEGIN
ADAM_CASES = [AdamCase(n, al, (1.0, 0.25)[(k + j) % 2]) for k, n in enumerate(ADAM_N)
              for j, al in enumerate(('aligned', 'all_off', 'g_off'))]
# ADAM_CASES_END
ADAM_STEPS = 3

MISC_N = (1, 16, 17, 257)


# ---------------------------------------------------------------------------------------------------------------------------
# the host-side checks of the tables
# ---------------------------------------------------------------------------------------------------------------------------
def test_gauss_table_hits_every_grid_boundary():
    ns = {c.n for c in GAUSS_CASES}
    assert ns >= set(GAUSS_N)
    for n in GAUSS_N:
        assert {c.S for c in GAUSS_CASES if c.n == n} >= {1, 5}, n
    blocks = {gauss_blocks(n) for n in ns}
    assert {1, 2, 64} <= blocks                                        # one block, two blocks, the cap
    for edge in (256, 1024, 65536):                                    # both sides of every threshold
        assert {edge - 1, edge, edge + 1} & ns >= {edge, edge + 1}, edge
    assert 255 in ns and 1 in ns
    # the cap is reached from both sides and passed by a ragged remainder (a trip that only some lanes take)
    assert any(cdiv(n, 1024) > 64 and n % 1024 not in (0, 1) for n in ns)
    # `total`: more than 256 partials (second trip of reduce_final_kernel)
    assert any(c.S * gauss_blocks(c.n) > 256 for c in GAUSS_CASES)
    assert any(c.S * gauss_blocks(c.n) <= 256 and c.S > 1 for c in GAUSS_CASES)
    assert len(GAUSS_GOUT) >= 5 and len(set(GAUSS_GOUT)) == len(GAUSS_GOUT) and GAUSS_UP != 1.0


def test_kl_table_hits_every_grid_boundary():
    Ms = {c.M for c in KL_CASES}
    assert Ms >= set(KL_M)
    for M in KL_M:
        assert {c.batch for c in KL_CASES if c.M == M} >= {1, 3}, M
    assert 1 in Ms and 2 in Ms
    assert any(kl_blocks(M) == 1 and M > 1 for M in Ms)                # one block walks several rows
    assert {31, 32, 33} <= Ms and kl_blocks(32) == 1 and kl_blocks(33) == 2
    assert {256, 257} <= Ms                                            # second trip of the j loop
    assert {512, 513} <= Ms and kl_blocks(512) == 256                  # the cap, reached ...
    assert any(M * M > 256 * 1024 and kl_blocks(M) < M for M in Ms)    # ... and passed: a block takes a second row
    assert any(M > 513 for M in Ms)
    assert any(c.batch * kl_blocks(c.M) > 256 for c in KL_CASES)       # `total`: more than 256 partials
    for c in KL_CASES:
        P = kl_inputs(c, 'bound')
        d = torch.diagonal(P['L'], dim1=-2, dim2=-1)
        assert bool((d < 0).any()), c
        up = torch.triu(torch.ones(c.M, c.M, dtype=torch.bool), 1)
        assert bool(torch.isnan(P['L_given'][:, up]).all()) and not bool(torch.isnan(P['L_given'][:, ~up]).any())
        Pi = kl_inputs(c, 'int')
        assert bool((torch.diagonal(Pi['L'], dim1=-2, dim2=-1).abs() == 1).all())


def test_objective_table_hits_every_boundary():
    ng = {len(c.batches) for c in OBJ_CASES}
    assert ng >= {0, 1, 3, OBJ_MAX_GROUPS}
    assert {c.M for c in OBJ_CASES if c.batches} >= {1, 33, 257}
    assert {c.n for c in OBJ_CASES} >= {1, 1025, 65537}
    assert {c.noise_grad for c in OBJ_CASES} == {True, False}
    assert all(c.up != 1.0 for c in OBJ_CASES)
    # a group whose element count is no multiple of 256 is followed by another group (a partial block, then a clean start)
    assert any(len(c.batches) >= 3 and all((b * c.M * c.M) % 256 for b in c.batches[:-1]) for c in OBJ_CASES)
    assert any(c.batches == (1, 3, 2) and c.M == 33 for c in OBJ_CASES)
    # both layouts of a group
    assert any(c.squeeze and 1 in c.batches for c in OBJ_CASES)
    assert any((not c.squeeze and 1 in c.batches) or max(c.batches, default=0) > 1 for c in OBJ_CASES)
    assert len({c.name for c in OBJ_CASES}) == len(OBJ_CASES)


def test_mean_field_kl_table_hits_every_boundary():
    tots = {c.batch * c.M for c in MF_KL_CASES}
    assert {(c.batch, c.M) for c in MF_KL_CASES} >= {(1, 1), (1, 255), (1, 257), (1, 1024), (1, 1025), (3, 342), (2, 131073)}
    assert 1 in tots and {255, 257} <= tots                            # one lane, both sides of a block's 256 lanes
    assert {1024, 1025} <= tots and kl_diag_blocks(1024) == 1 and kl_diag_blocks(1025) == 2      # a block's share
    assert any(c.batch > 1 and c.batch * c.M > 1024 and (c.batch * c.M) % 256 for c in MF_KL_CASES)   # batched, ragged
    assert any(cdiv(t, 1024) > 256 and t % 1024 for t in tots)         # past the cap of 256 blocks: a ragged second trip
    for c in MF_KL_CASES:
        P = mf_kl_inputs(c)
        assert P['m'].shape == tuple(c) and float(P['s2'].min()) >= 0.25 and float(P['s2'].max()) <= 2.25


def test_objective_bit_record_holds_exactly_the_tables_rows():
    import json
    import os
    ids = [objective_bits_id(r) for r in OBJECTIVE_BITS_CASES]
    assert len(set(ids)) == len(ids) == 2 * (len(GAUSS_CASES) + len(KL_CASES) + len(OBJ_CASES) + len(MF_KL_CASES))
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'objective_hashes.json')) as f:
        record = json.load(f)['cases']
    assert sorted(record) == sorted(ids)
    assert all(record[k] and all(len(h) == 64 for h in record[k].values()) for k in ids)


def test_rowdot_table_hits_every_loop_boundary():
    ns = {c.n for c in ROWDOT_CASES}
    assert ns >= set(ROWDOT_N) | set(ROWDOT_ODD_N)
    for dt, V in (('f32', 4), ('f64', 2)):
        nch = {n: rowdot_chunks(n, dt) for n in ns if n % V == 0}
        assert any(v == 1 for v in nch.values())
        assert any(v == 7 for v in nch.values()) and any(8 <= v < 16 for v in nch.values())  # last below / first in the
        assert any(v > 8 and v % 8 for v in nch.values())                                  # unrolled loop, plus a tail
        assert any(v == 8 for v in nch.values()) or dt == 'f64'                            # (f64: 14, 15 and 19 chunks)
        assert any(v >= 8 and n % (256 * V) for n, v in nch.items())                       # ragged last chunk
        for c in ROWDOT_CASES:
            if c.n % V == 0:
                assert c.M > rowdot_chunks(c.n, dt), c                                     # every rotated start and a wrap
    # the weight gradient's eight pairs in flight (n > 1792) and below; strided_sum4 four-deep aligned (n >= 4 * 256 * V)
    assert any(c.n > 1792 + 2048 for c in ROWDOT_CASES) and any(c.n <= 1792 for c in ROWDOT_CASES)
    # odd n with batch 2: the second batch element is unaligned; 769 / 1793 are one past the unaligned four-deep loop's
    # entry (j + 768 < n) and its second trip, 2051 has a ragged one-deep tail
    assert all(c.batch == 2 for c in ROWDOT_CASES)
    assert {n for n in ns if n % 2} >= {769, 1793, 2051}
    for n in ns:
        rows = [c for c in ROWDOT_CASES if c.n == n and c.drop is None and c.off is None]
        assert {c.shared for c in rows} == {0, 1}, n
    assert {c.D for c in ROWDOT_CASES} >= {1, 3}
    assert {c.drop for c in ROWDOT_CASES} == {None, 'gv', 'out_1', 'out_x'}
    assert {c.off for c in ROWDOT_CASES} >= {None, 'A', 'g'}
    # an offset operand at a size that would otherwise take the vector path, beyond the eight-chunk threshold too
    assert any(c.off == 'A' and c.n % 4 == 0 and rowdot_chunks(c.n, 'f32') >= 8 for c in ROWDOT_CASES)
    assert any(c.off == 'g' and c.n % 4 == 0 and c.n > 4 * 1024 for c in ROWDOT_CASES)
    # each absent output / offset operand at one chunk, at the eight-chunk loop (7176) and (offsets) at the unrolled loop plus
    # tail, where the unaligned strided_sum4 takes its four-deep loop more than once (9220); an absent output also at an odd n
    for drop in ('gv', 'out_1', 'out_x'):
        assert {c.n for c in ROWDOT_CASES if c.drop == drop} >= {1000, 2051, 7176}, drop
    for off in ('A', 'g', 'gv'):
        assert {c.n for c in ROWDOT_CASES if c.off == off} >= {1000, 7176, 9220}, off
    assert {n for n, _ in PLAIN_ROWDOT_CASES} >= set(ROWDOT_N) and {o for _, o in PLAIN_ROWDOT_CASES} == {None, 'A', 'g'}
    for n in ROWDOT_N:
        assert {o for m, o in PLAIN_ROWDOT_CASES if m == n} == {None, 'A', 'g'}, n


def test_colstats_and_finalize_tables_hit_every_boundary():
    assert {c.M for c in COLSTATS_CASES} >= {1, 2, 3, 4, 5, 7, 100}
    for M in (1, 2, 3, 4, 5, 7, 100):
        assert {c.n for c in COLSTATS_CASES if c.M == M} >= {1, 63, 64, 65, 333}, M
    assert all(c.batch == 2 for c in COLSTATS_CASES)
    # kq = ceil(M / 4): waves left without a row
    assert any(3 * cdiv(c.M, 4) >= c.M for c in COLSTATS_CASES) and any(cdiv(c.M, 4) >= c.M for c in COLSTATS_CASES)
    for form in ('plain', 'affine', 'p64'):
        rows = [c for c in FINALIZE_CASES if c.form == form]
        assert {(c.tiles, c.n) for c in rows} >= {(t, n) for t in FIN_TILES for n in FIN_N}, form
    aff = [c for c in FINALIZE_CASES if c.form == 'affine']
    assert {c.has_w for c in aff} == {0, 1} and {c.has_c for c in aff} == {0, 1}
    assert {(c.has_w, c.has_c) for c in aff} >= {(1, 1), (0, 0), (1, 0), (0, 1)}
    assert {c.shared for c in aff if c.has_w or c.has_c} == {0, 1}
    p64 = [c for c in FINALIZE_CASES if c.form == 'p64']
    assert {c.shared for c in p64} == {0, 1}
    for c in p64:                                         # no partial sum survives an early downcast
        P = finalize_inputs(c)
        for name in ('pdot', 'psqC'):
            s = P[name].sum(1)
            assert bool((s.float().double() != s).all()), (c, name)
            assert bool((P[name][:, 0].float().double() != P[name][:, 0]).all()), (c, name)
        mean, var = finalize_reference(c, P)
        assert bool((mean.float().double() == mean).all()) and bool((var.float().double() == var).all())
        # the sum before c is added is no float32 number either
        pre = mean - P['c'].expand(FIN_BATCH).unsqueeze(1)
        assert bool((pre.float().double() != pre).all()), c


def test_diag_table_hits_every_boundary():
    assert {c.M for c in DIAG_CASES} == set(DIAG_M) and {c.n for c in DIAG_CASES} == set(DIAG_N)
    assert {diag_tiles(M) for M in DIAG_M} >= {1, 2, 3} and {DIAG_ROWS - 1, DIAG_ROWS, DIAG_ROWS + 1, 1} <= set(DIAG_M)
    assert any(M > 2 * DIAG_ROWS and M % DIAG_ROWS for M in DIAG_M)                     # a ragged third tile
    forms = ('vec', 'scalar-n', 'scalar-A', 'scalar-g')
    for dt in DTYPES:
        V = diag_vec(dt)
        assert V == {'f32': 4, 'f64': 2}[dt]
        vec_n = {c.n for c in DIAG_CASES if diag_form(c, dt) == 'vec'}
        # one column group filled to its last lane, and one lane of the next
        assert {256 * V, 256 * V + 4} <= vec_n, dt
        assert diag_groups(256 * V, dt, True) == 1 and diag_groups(256 * V + 4, dt, True) == 2
        # one chunk of the backward pass filled, one vector of the next; an odd n in its third chunk
        assert {DIAG_BWD_COLS, DIAG_BWD_COLS + 4} <= vec_n and any(n % 2 and n > 2 * DIAG_BWD_COLS for n in DIAG_N)
        scalar_n = {c.n for c in DIAG_CASES if diag_form(c, dt) == 'scalar-n'}
        assert {1, 5, 8195} <= scalar_n and all(n % V for n in scalar_n)
        assert any(diag_groups(n, dt, False) > 1 for n in scalar_n)
        for M in DIAG_M:                                  # every M with every launch form
            assert {diag_form(c, dt) for c in DIAG_CASES if c.M == M} == set(forms), (M, dt)
        for form in forms:                                # the extra tile row with every launch form
            assert {c.extra for c in DIAG_CASES if diag_form(c, dt) == form} == {0, 1}, (form, dt)
        for n in DIAG_N:                                  # every n with every launch form it can reach
            want = {'scalar-n'} if n % V else set(forms) - {'scalar-n'}
            assert {diag_form(c, dt) for c in DIAG_CASES if c.n == n} == want, (n, dt)
    for n in DIAG_N:
        assert {c.off for c in DIAG_CASES if c.n == n} == set(DIAG_OFFS), n
    assert len(DIAG_CASES) < len(DIAG_M) * len(DIAG_N) * len(DIAG_OFFS)                 # not the cross product
    assert {(c.tiles, c.qtiles) for c in DIAG_FIN_CASES} == {(1, 1), (1, 3), (7, 1), (7, 3)}
    for tq in ((1, 1), (1, 3), (7, 1), (7, 3)):
        assert {(c.has_w, c.has_c, c.shared) for c in DIAG_FIN_CASES if (c.tiles, c.qtiles) == tq} == set(_FIN_COMBOS), tq
    assert {c.n for c in DIAG_FIN_CASES} >= set(FIN_N)
    for c in DIAG_CASES[:3] + DIAG_CASES[-1:]:
        P = diag_inputs(c)
        assert P['A'].shape == (DIAG_BATCH, c.M, c.n) and bool((P['s2m1'] < 0).any() or c.M == 1)
        assert float(P['s2m1'].min()) >= -0.75 and float(P['s2m1'].max()) <= 1.25


def test_layer_bit_record_holds_exactly_the_tables_rows():
    import json
    import os
    ids = [layer_bits_id(r) for r in LAYER_BITS_CASES]
    assert len(set(ids)) == len(ids) == 2 * (len(ROWDOT_CASES) + len(PLAIN_ROWDOT_CASES) + len(COLSTATS_CASES)
                                             + len(SAMPLE_CASES) + len(DIAG_CASES) + len(DIAG_FIN_CASES)) + len(FINALIZE_RUNS)
    assert len(FINALIZE_RUNS) == 2 * len(FINALIZE_CASES) - sum(c.form == 'p64' for c in FINALIZE_CASES)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'layer_reduction_hashes.json')) as f:
        record = json.load(f)['cases']
    assert sorted(record) == sorted(ids)
    assert all(record[k] and all(len(h) == 64 for h in record[k].values()) for k in ids)


def test_sample_adam_and_misc_tables():
    assert {(c.S, c.n, c.b) for c in SAMPLE_CASES} >= {(1, 1, 1), (4, 77, 2), (3, 256, 1), (2, 257, 3)}
    for S, n, b in ((4, 77, 2), (3, 256, 1), (2, 257, 3)):
        assert {c.ns for c in SAMPLE_CASES if (c.S, c.n, c.b) == (S, n, b)} == {1, S}
    assert {c.n for c in ADAM_CASES} >= set(ADAM_N)
    for n in ADAM_N:
        assert {c.align for c in ADAM_CASES if c.n == n} == {'aligned', 'all_off', 'g_off'}, n
    assert {c.grad_scale for c in ADAM_CASES} == {1.0, 0.25}
    for al in ('aligned', 'all_off', 'g_off'):
        assert {c.grad_scale for c in ADAM_CASES if c.align == al} == {1.0, 0.25}, al
    assert ADAM_STEPS == 3
    assert set(MISC_N) >= {1, 16, 17, 257}


def _below_limit(abs_value, q, what, limit=EXACT_LIMIT):
    """Every partial sum is a multiple of q of magnitude at most abs_value: exact while abs_value / q < 2^24."""
    worst = float(torch.as_tensor(abs_value).abs().max()) / q
    assert worst < limit, f'{what}: sum |term| / q = {worst:.4g} is not below {limit:g}'


def test_exact_cases_stay_below_2_to_24():
    ab = lambda P: {k: (v.abs() if torch.is_tensor(v) else v) for k, v in P.items()}       # noqa: E731
    for c in ROWDOT_CASES:
        P = rowdot_inputs(c.n, c.batch, c.M, c.D, 'affine')
        for name, val in rowdot_reference(ab(P), c.shared).items():
            _below_limit(val, 1.0, (c, name))
    for n, off in PLAIN_ROWDOT_CASES:
        _below_limit(rowdot_reference(ab(rowdot_inputs(n, 2, 3, 1, 'plain')), 0)['out'], 1.0, (n, off))
    for c in COLSTATS_CASES:
        A = ab(colstats_inputs(c))
        R = colstats_reference(A)
        # var and Abar subtract: the same expressions with + bound them
        _below_limit(A['base'].unsqueeze(1) + (A['C'] ** 2 + A['A'] ** 2).sum(1), 1.0, (c, 'var'))
        _below_limit(A['m'].unsqueeze(2) * A['gmean'].unsqueeze(1) + 2.0 * A['gvar'].unsqueeze(1) * A['A'], 1.0, (c, 'Abar'))
        for name in ('mean', 'C2', 'mbar'):
            _below_limit(R[name], 1.0, (c, name))
    for c in FINALIZE_CASES:
        P = ab(finalize_inputs(c))
        mean = P['pdot'].sum(1) + (torch.einsum('bnd,bd->bn', P['x'], P['w'].expand(FIN_BATCH, -1)) if c.has_w else 0.0) \
            + (P['c'].expand(FIN_BATCH).unsqueeze(1) if c.has_c else 0.0)
        var = P['base'].unsqueeze(1) + FIN_BASE_ADD + P['psqC'].sum(1) + P['psqA'].sum(1)
        # p64 sums in float64 (exact below 2^53) and only its RESULT must be a float32 number, asserted with the table above
        limit = 2.0 ** 53 if c.form == 'p64' else EXACT_LIMIT
        _below_limit(mean, 0.5, (c, 'mean'), limit)
        _below_limit(var, 0.25, (c, 'var'), limit)
    for c in SAMPLE_CASES:
        _below_limit(sample_reference(ab(sample_inputs(c)), c.ns)['gmean'], 1.0, (c, 'gmean'))
    for c in KL_CASES:                                    # forward with every diagonal entry +-1: multiples of 1/2 (1/4 scaled)
        P = kl_inputs(c, 'int')
        _, a = kl_reference(P['m'], P['L'])
        _below_limit(a.sum() + abs(P['addin']), 0.25, (c, 'kl'))
    for c in GAUSS_CASES:                                 # noise gradient at noise = 1: terms 1/2 (e - 1) times an integer
        P = gauss_inputs(c, 'int')                        # gout (vector form) or upstream gradient (total form); the power-
        _, _, _, ga = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])     # of-two scale multiplies the finished sum
        _below_limit((ga * P['gout'].unsqueeze(1)).sum(), 0.5, (c, 'gnoise'))
        _below_limit(ga.sum() * abs(P['up']), 0.5, (c, 'gnoise total'))


def test_spikes_are_visible():
    """Removing any one probed term moves the float64 reference by more than 4x the loosest tolerance the GPU test applies
    to a sum that holds it (the `total` forms, float32)."""
    for c in GAUSS_CASES:
        P = gauss_inputs(c, 'bound')
        t, a, _, _ = gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
        tol = red_tol(c.S * c.n, C_GAUSS, 'f32', abs(P['scale']) * float(a.sum()))
        assert P['probes'] == gauss_probes(c.n, c.S) and (0, 0) in P['probes'] and (c.S - 1, c.n - 1) in P['probes']
        for s, i in P['probes']:
            assert abs(P['scale'] * float(t[s, i])) > 4.0 * tol, (c, s, i)
            row_tol = red_tol(c.n, C_GAUSS, 'f32', abs(P['scale']) * float(a[s].sum()))
            assert abs(P['scale'] * float(t[s, i])) > 4.0 * row_tol, (c, s, i)
    for c in KL_CASES:
        P = kl_inputs(c, 'bound')
        _, a = kl_reference(P['m'], P['L'])
        tol = red_tol(c.batch * kl_terms_count(c.M), C_KL, 'f32', abs(P['scale']) * float(a.sum()))
        assert P['probes'] == kl_probes(c.M, c.batch)
        for b, i, j in P['probes']:
            moved = 0.5 * float(P['L'][b, i, j]) ** 2                   # the term l_ij^2 / 2 of KL_b
            assert abs(P['scale']) * moved > 4.0 * tol, (c, b, i, j)
            assert moved > 4.0 * red_tol(kl_terms_count(c.M), C_KL, 'f32', float(a[b])), (c, b, i, j)
    for c in OBJ_CASES:
        P = obj_inputs(c)
        _, ab, t = obj_reference(P)
        tol = red_tol(obj_terms_count(c), C_GAUSS + C_KL, 'f32', ab)
        assert (0, 0) in P['ell_probes'] and (c.S - 1, c.n - 1) in P['ell_probes']
        for s, i in P['ell_probes']:
            assert abs(float(t[s, i])) > 4.0 * tol, (c.name, s, i)
        assert bool(P['kl_probes']) == bool(c.batches)
        for gi, b, i, j in P['kl_probes']:
            assert abs(P['kl_scale']) * 0.5 * float(P['groups'][gi][1][b, i, j]) ** 2 > 4.0 * tol, (c.name, gi, b, i, j)


def test_builder_values_are_float32_numbers():
    """Both dtypes must see the same inputs: everything a builder returns survives a round trip through float32."""
    def check(P, what):
        for k, v in P.items():
            if torch.is_tensor(v):
                w = v[~torch.isnan(v)]
                assert torch.equal(w.float().double(), w), (what, k)
            elif isinstance(v, float):
                assert float(torch.tensor(v, dtype=torch.float32)) == v, (what, k)
    for c in GAUSS_CASES[:4] + GAUSS_CASES[-2:]:
        check(gauss_inputs(c, 'bound'), c)
    for c in KL_CASES[:6] + KL_CASES[-1:]:
        check(kl_inputs(c, 'bound'), c)
    for c in OBJ_CASES:
        P = obj_inputs(c)
        check(P, c.name)
        for m, L, Lg in P['groups']:
            check(dict(m=m, L=L, Lg=Lg), c.name)
    for c in SAMPLE_CASES:
        check(sample_inputs(c), c)
        check(sample_real_inputs(c), c)
    check(rowdot_real_inputs(1000, 2, 3, 3, 'affine'), 'rowdot')
    check(colstats_real_inputs(COLSTATS_CASES[-1]), 'colstats')
    check(diag_inputs(DIAG_CASES[0]), 'diag')
