"""The case table of the Cholesky / triangular-inverse bit pin (csrc/potrf.hip) and its seeded input builder.  No GPU here.

`CASES` is THE list tools/record_potrf_hashes.py records and tests/test_gpu_potrf_bits.py recomputes: the smallest shapes
that reach every launch path of `potrf_impl`, `potrf_inv_impl` and `trtri_impl`.  `potrf_path`, `inv_path` and `trtri_path`
repeat the hosts' arithmetic (nslab, ntile, tm > tn, pre, tail, outer panels, nprow, npupd) and name the branches a case
reaches; tests/test_potrf_bits_cases_cpu.py asserts that the table reaches all of them, so a case cannot be dropped quietly.

Inputs: `A A^T / n + 0.5 I` in float64 from `torch.Generator().manual_seed(...)`, cast to the case's dtype -- the builder of
tests/test_gpu_kernels.py::_spd, with the Gaussian factor rounded to multiples of 2^-10 first.  Every product and partial
sum of A A^T is then an integer multiple of 2^-20 below 2^53 of them (|a| < 8, n < 2^13), so the host's float64 product is
exact in any summation order and the input BITS do not depend on which BLAS, or which CPU, builds them.
"""
import collections
import functools

NB = 64
DTYPES = ('f64', 'f32')
GUARD_LD, GUARD_BATCH = 8, 40         # strided cases: ld = n + 8, batch stride = ld * n + 40

# op: 'potrf' | 'trtri' | 'potrf_trtri' | 'potrf_trtri_w32';  env: the switches set around the call;
# bad: ((matrix, minor), ...) -- A[matrix][minor - 1][minor - 1] = -5, so that info[matrix] == minor;
# strided: '' | 'A' (potrf's matrix) | 'X' (the fused call's inverse, and its float32 copy): padded strides, guards checked.
Case = collections.namedtuple('Case', 'op dt n batch env bad strided')


def case_id(c):
    s = f'{c.op}|{c.dt}|n{c.n}b{c.batch}'
    s += ''.join(f'|{k[len("NSGP_POTRF_"):]}={v}' for k, v in c.env)
    s += ''.join(f'|bad{b}@{m}' for b, m in c.bad)
    return s + (f'|ld{c.strided}' if c.strided else '')


def _C(op, dt, n, batch=1, env=(), bad=(), strided=''):
    return Case(op, dt, n, batch, tuple(env), tuple(bad), strided)


def _table():
    out = []
    for dt in DTYPES:
        # ---- potrf
        out += [_C('potrf', dt, n) for n in (1, 7, 63, 64, 65, 128, 130, 192, 200, 320, 448, 2112, 2149)]
        out += [_C('potrf', dt, n, 3) for n in (200, 320)]
        out += [_C('potrf', dt, 2112, env=[('NSGP_POTRF_NB2', '4')])]
        out += [_C('potrf', dt, 200, 2, strided='A')]
        out += [_C('potrf', dt, 200, bad=[(0, m)]) for m in (6, 151, 195)]
        out += [_C('potrf', dt, 200, 3, bad=[(1, 151)])]
        # ---- potrf_trtri
        fused = [_C('potrf_trtri', dt, n, b) for n in (64, 128, 192, 256, 320) for b in (1, 2)]
        fused += [_C('potrf_trtri', dt, 1024, 3), _C('potrf_trtri', dt, 2048), _C('potrf_trtri', dt, 200),
                  _C('potrf_trtri', dt, 2112), _C('potrf_trtri', dt, 192, env=[('NSGP_POTRF_INV', '0')]),
                  _C('potrf_trtri', dt, 192, 2, strided='X')]
        out += fused
        if dt == 'f64':
            out += [c._replace(op='potrf_trtri_w32') for c in fused]
        # ---- trtri
        out += [_C('trtri', dt, n) for n in (1, 63, 64, 65, 130, 200, 1100)]
    return out


CASES = _table()


@functools.lru_cache(maxsize=None)        # shared by the cases of one (n, batch): under 200 MB for the whole table
def _spd64(n, batch):
    import torch
    g = torch.Generator().manual_seed(7919 * n + batch)
    A = torch.randn((batch, n, n), generator=g, dtype=torch.float64)
    A = torch.round(A * 1024.0) / 1024.0                    # see the module docstring: the product below is exact
    return A @ A.transpose(-1, -2) / n + 0.5 * torch.eye(n, dtype=torch.float64)


def make_input(c):
    """The case's (batch, n, n) matrices on the host, in its dtype, bad pivots planted."""
    import torch
    A = _spd64(c.n, c.batch).to(torch.float64 if c.dt == 'f64' else torch.float32).clone()
    for b, m in c.bad:
        A[b, m - 1, m - 1] = -5.0
    return A


def _cdiv(a, b):
    return -(-a // b)


def potrf_launches(n, nb2=None):
    """The launches of potrf_impl, in order: ('step', j0, pre, below, nslab, wcols, tm, tn, ntile), ('tail', j0, pre),
    ('gemm', rest, kw)."""
    nb2m = nb2 if nb2 else (32 if n <= 4096 else 16)
    NB2 = nb2m * NB if n > 2048 else n
    out = []
    for J0 in range(0, n, NB2):
        Jend = min(J0 + NB2, n)
        for j0 in range(J0, Jend, NB):
            nb = min(n - j0, NB)
            pre = int(j0 > J0)
            if nb < NB:
                out.append(('tail', j0, pre))
                break
            below = n - j0 - nb
            nslab = _cdiv(below, NB) if below > 0 else 1
            wcols = Jend - (j0 + nb) if pre else 0
            tm = tn = ntile = 0
            if below > 0 and wcols > 0:
                tm, tn = _cdiv(below, NB), _cdiv(wcols, NB)
                ntile = tn * (tn + 1) // 2 + (tm - tn) * tn
            out.append(('step', j0, pre, below, nslab, wcols, tm, tn, ntile))
        if Jend < n:
            out.append(('gemm', n - Jend, Jend - J0))
    return out


def potrf_path(c):
    """Branches of potrf_impl and its kernels that a 'potrf' case reaches."""
    nb2 = dict(c.env).get('NSGP_POTRF_NB2')
    ls = potrf_launches(c.n, int(nb2) if nb2 else None)
    steps = [l for l in ls if l[0] == 'step']
    tails = [l for l in ls if l[0] == 'tail']
    gemm = any(l[0] == 'gemm' for l in ls)
    tags = set()
    if not steps:
        tags.add('tail_only')
    for _, j0, pre, below, nslab, wcols, tm, tn, ntile in steps:
        tags.add('panel_pre' if pre else 'panel_first')
        if below == 0:
            tags.add('panel_pre_no_slab' if pre else 'panel_rows0')
        if below % NB:
            tags.add('ragged_slab')
        if nslab > 1:
            tags.add('several_slabs')
        if ntile:
            tags.add('update_tiles')
            tags.add('ragged_update_tile' if wcols % NB else 'full_update_tile')
            if tn >= 3:
                tags.add('triangle_tn_ge_3')
            if tm > tn:
                tags.add('update_rows_below_triangle')
            if c.batch > 1:
                tags.add('batched_update_tiles')
        if gemm and j0 > 0 and not pre:
            tags.add('lone_panel_after_gemm')
    for _, j0, pre in tails:
        if steps:
            tags.add('tail_pre' if pre else 'tail_no_pre')
        if gemm and pre:
            tags.add('tail_pre_after_gemm')
    if gemm:
        tags.add('outer_panel_gemm')
    if c.strided:
        tags.add('strided_A')
    for b, m in c.bad:
        j0 = (m - 1) // NB * NB
        tags.add('bad_in_tail' if c.n - j0 < NB else ('bad_in_panel0' if j0 == 0 else 'bad_in_later_panel'))
        if c.batch > 1 and 0 < b < c.batch - 1:
            tags.add('bad_in_middle_of_batch')
    return tags


def inv_launches(n):
    """The launches of potrf_inv_impl: (j0, pre, nslab, nprow, nsyrk, npupd, tn)."""
    out = []
    for j0 in range(0, n, NB):
        pre = int(j0 > 0)
        below = n - j0 - NB
        nslab = below // NB if below > 0 else 1
        nprow = j0 // NB + 1
        nsyrk = npupd = tn = 0
        if pre and below > 0:
            tn = below // NB
            nsyrk, npupd = tn * (tn + 1) // 2, tn * (j0 // NB)
        out.append((j0, pre, nslab, nprow, nsyrk, npupd, tn))
    return out


def inv_path(c):
    """Branches of potrf_trtri_impl that a 'potrf_trtri' / 'potrf_trtri_w32' case reaches."""
    tags = set()
    if c.n % NB or c.n > 2048 or dict(c.env).get('NSGP_POTRF_INV') == '0':
        tags.add('fallback_switch' if c.env else ('fallback_ragged' if c.n % NB else 'fallback_large'))
        return tags
    ls = inv_launches(c.n)
    if len(ls) == 1:
        tags.add('single_panel')
    for j0, pre, nslab, nprow, nsyrk, npupd, tn in ls:
        tags.add('chunk_diag')
        if nprow >= 2:
            tags.add('chunk_first_touched')
        if nprow >= 3:
            tags.add('chunk_already_updated')
        if nsyrk:
            tags.add('syrk_tiles')
        if npupd:
            tags.add('pupd_first_touched')
            if j0 // NB >= 2:
                tags.add('pupd_accumulates')
            if tn >= 2:
                tags.add('pupd_two_row_blocks')
    if c.batch > 1:
        tags.add('batched')
    if (c.n, c.batch) == (1024, 3):
        tags.add('headline_chain')
    if c.n == 2048:
        tags.add('largest_one_level')
    if c.strided:
        tags.add('strided_X')
    return tags


def trtri_path(c):
    """Branches of trtri_impl that a 'trtri' case reaches."""
    n, tags, s = c.n, set(), NB
    tags.add('ragged_diag_block' if n % NB else 'full_diag_blocks')
    if n <= NB:
        tags.add('diag_only')
    while s < n:
        full = n // (2 * s)
        rem = n - full * 2 * s
        if full:
            tags.add('full_pairs')
        if rem > s:
            tags.add('rem_gt_s_after_full_pairs' if full else 'rem_gt_s')
        if s > NB:
            tags.add('second_level')
        s *= 2
    return tags


def path(c):
    return {'potrf': potrf_path, 'trtri': trtri_path}.get(c.op, inv_path)(c)
