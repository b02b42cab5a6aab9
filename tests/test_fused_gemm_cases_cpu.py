"""The case table of the exact fused-GEMM tests (tests/fused_gemm_cases.py), checked on the host (no GPU):
every row lands on the tile, `whole` value, vector flags, split and tile rows it states and reaches the paths it is tagged
for -- asked of the library's own host queries (nsgp_gemm_plan, nsgp_svgp_colstats_tiles, nsgp_svgp_f64acc_tiles_for,
nsgp_svgp_kzx_gemm_supported, nsgp_svgp_lqbar_workspace); the table holds every (family, dtype, tile, whole) combination
and every launch of the bit pin, and every tag; the exactness conditions of the `int`, `grid` and `kzx` kinds hold on the
built data; every reference function agrees with a loop written from the formula.  A planner change that moves a row fails
here and is answered by adding the shape that reaches the path it left."""
import ctypes

import pytest
import torch

import fused_gemm_cases as FC
import gemm_bits_cases as GB
from test_gemm_bits_cases_cpu import COMBINATIONS

ALIGNED = 4096                          # only a pointer's alignment is looked at


def _lib():
    import nsgp
    return nsgp.load_library()


def _plan(lib, c):
    M, N, K, flags, ma, mb = GB.gemm_query(c)
    buf = (ctypes.c_int32 * 11)()
    assert lib.nsgp_gemm_plan(M, N, K, c.batch, 1, FC.es(c), flags, c.vec[0], c.vec[1], ma, mb,
                              ctypes.cast(buf, ctypes.c_void_p)) == 0
    return tuple(buf)


def _vec_rule(c):
    """(vecA, vecB) by the rules of gemm_impl / tri_gemm_colstats_f64acc_impl, from the shape and the row's misalignment."""
    mis = dict(c.opt).get('mis')
    if c.family in ('lqbar', 'lqbar_acc'):
        v = int(c.n % 4 == 0)
        return v, v
    if c.family == 'kzx':
        return int(c.M % 4 == 0), 1
    return int(c.M % 4 == 0 and mis != 'W'), int(c.n % 4 == 0 and mis != 'X')


def row_problems(lib, c):
    """Reasons why a row does not land where it states (empty: it does)."""
    why = []
    tags = set(c.tags)
    opt = dict(c.opt)
    say = lambda cond, text: None if cond else why.append(text)                              # noqa: E731
    say(tags <= set(FC.TAGS), f'unknown tags {tags - set(FC.TAGS)}')
    say(c.vec == _vec_rule(c), f'vector flags {c.vec} != {_vec_rule(c)}')
    say(('vecA_off' in tags) == (not c.vec[0]) and ('vecB_off' in tags) == (not c.vec[1]), 'vec*_off tags')
    say(('whole' in tags) == bool(c.whole) and ('ragged' in tags) == (not c.whole), 'whole / ragged tags')
    say(('misaligned_W' in tags) == (opt.get('mis') == 'W') and ('misaligned_X' in tags) == (opt.get('mis') == 'X'), 'misaligned tags')
    say(('ks_unaligned_base' in tags) == (opt.get('mis') == 'gvar'), 'ks_unaligned_base tag')
    say(('p0_null' in tags) == (opt.get('p0') == 'null'), 'p0_null tag')
    say(('part_rows_extra' in tags) == (c.family in FC.PART_ROWS_FAMILIES) and FC.EXTRA_ROWS > 0, 'part_rows_extra tag')
    say(('trans' in tags) == (c.family in ('colstats_t', 'f64acc_t')), 'trans tag')
    say(('per_gp_x' in tags) == bool(opt.get('xb')), 'per_gp_x tag')
    for k in (1, 2, 3, 4):
        say(f'tile_rows_{k}' not in tags or c.trows == k, f'tile_rows_{k} tag on a row with {c.trows} tile rows')
    say((c.batch > 1) == bool(tags & {'batch_perm_on', 'batch_perm_off'}) and not tags >= {'batch_perm_on', 'batch_perm_off'},
        'batch_perm tags')
    if c.family in GB.GEMM_IMPL_FAMILIES:
        p = _plan(lib, c)
        say((p[0], p[1]) == c.tile and p[4] == c.whole, f'plan {p}')
        say(c.batch == 1 or (p[6] == 1) == ('batch_perm_on' in tags), f'batch_perm {p[6]}')
        if c.family in ('lqbar', 'lqbar_acc'):
            wsb = lib.nsgp_svgp_lqbar_workspace(c.batch, c.M, c.n, FC.es(c))
            say(int(p[2] > 1) == c.split == int(wsb > 0), f'split: plan {p[2]}, workspace {wsb}')
            say(wsb == (p[2] * c.batch * c.M * c.M * FC.es(c) if p[2] > 1 else 0), f'workspace {wsb}')
            say(c.trows == -(-c.M // c.tile[0]), 'tile rows')
            # the k-scaled loader's vector path: gvar + bb n aligned to 4 elements
            base = 1 if opt.get('mis') == 'gvar' else 0
            al = [(base + bb * c.n) % 4 == 0 for bb in range(c.batch)]
            say(('ks_vec' in tags) == all(al), 'ks_vec tag')
            say(('ks_unaligned_batch' in tags) == (al[0] and not all(al)), 'ks_unaligned_batch tag')
            say(('ks_unaligned_base' in tags) == (not al[0]), 'ks_unaligned_base rule')
        else:
            say(p[2] == 1 and c.split == 0, 'a projection is never split')
            T = lib.nsgp_svgp_colstats_tiles(c.M, c.n, c.batch, FC.es(c))
            say(T == c.trows == -(-c.M // c.tile[0]), f'tile rows {T}')
    else:
        T = lib.nsgp_svgp_f64acc_tiles_for(c.M, c.n, c.batch)
        say(T == c.trows == -(-c.M // c.tile[0]) and c.tile[1] == 64 and c.split == 0, f'tile rows {T}')
        big = -(-c.M // 128) * -(-c.n // 64) * c.batch
        say((c.tile[0] == 128) == (big >= 512), 'tile height')
        say(('tiles_512' in tags) == (big == 512), 'tiles_512 tag')
        say(c.batch == 1 or (T * -(-c.n // 64) * c.batch <= 512) == ('batch_perm_on' in tags), 'batch_perm rule')
        say(('vec_not_whole' in tags) == (c.vec == (1, 1) and not c.whole), 'vec_not_whole tag')
        D = opt.get('D', 1)
        w_ptr = ctypes.c_void_p(ALIGNED + (8 if opt.get('mis') == 'W' else 0))
        sup = lib.nsgp_svgp_kzx_gemm_supported(w_ptr, c.M, c.n, c.batch, D)        # whole but for the B operand's own flag
        say(sup == int(bool(c.whole) or opt.get('mis') == 'X'), f'kzx_gemm_supported {sup}')
        say(c.whole == int(sup and c.vec[1]), 'whole')
    return why


def table_problems(cases):
    """Reasons why a table does not cover what it must (empty: it does)."""
    why = []
    have = {(c.family, c.dt, c.tile, c.whole) for c in cases}
    why += [f'no row for {k}' for k in COMBINATIONS if k not in have]
    launches = {(c.family, c.dt, c.batch, c.M, c.n, tuple((k, v) for k, v in c.opt if k in ('D', 'xb'))) for c in cases}
    for p in GB.CASES:                                   # the pin's launches (its `split` is a statement, not an input)
        key = (p.family, p.dt, p.batch, p.M, p.n, tuple((k, v) for k, v in p.opt if k in ('D', 'xb')))
        if key not in launches:
            why.append(f'no row for the pinned launch {GB.case_id(p)}')
    carried = {t for c in cases for t in c.tags}
    why += [f'no row carries the tag {t}' for t in FC.TAGS if t not in carried]
    for fam in ('lqbar', 'lqbar_acc'):
        for dt in ('f32', 'f64'):
            got = {t for c in cases if (c.family, c.dt) == (fam, dt) for t in c.tags}
            why += [f'{fam} {dt}: no {t} row' for t in ('ks_vec', 'ks_unaligned_batch', 'ks_unaligned_base', 'split', 'unsplit')
                    if t not in got]
    for fam in GB.F64ACC_FAMILIES:
        for kind in ('int', 'grid'):
            got = {t for c in cases if (c.family, c.kind) == (fam, kind) for t in c.tags}
            why += [f'{fam} {kind}: no {t} row' for t in ('misaligned_W', 'misaligned_X', 'vec_not_whole', 'vecA_off', 'vecB_off',
                                                          'tiles_512', 'batch_perm_on', 'batch_perm_off', 'tile_rows_1',
                                                          'tile_rows_2', 'tile_rows_3', 'tile_rows_4') if t not in got]
    for fam in ('colstats', 'colstats_t', 'colstats_rows', 'abar'):
        for dt in ('f32', 'f64'):
            got = {t for c in cases if (c.family, c.dt) == (fam, dt) for t in c.tags}
            why += [f'{fam} {dt}: no {t} row' for t in ('vecA_off', 'vecB_off', 'whole', 'tile_rows_1', 'tile_rows_3') if t not in got]
    p0 = {c.family for c in cases if 'p0_null' in c.tags}
    why += [f'no part_dot == NULL row for {f}' for f in ('colstats', 'colstats_t', 'colstats_rows', 'f64acc', 'f64acc_b64',
                                                         'f64acc_b64p32') if f not in p0]
    return why


def test_the_table_covers_every_combination_pinned_launch_and_tag():
    ids = [FC.case_id(c) for c in FC.CASES]
    assert len(set(ids)) == len(ids)
    assert table_problems(FC.CASES) == []
    assert {c.kind for c in FC.CASES if c.family in GB.F64ACC_FAMILIES} == {'int', 'grid'}
    assert {dict(c.opt)['D'] for c in FC.CASES if c.family == 'kzx'} >= {1, 2, 3, 4}
    for c, j in FC.NAN_CASES:                            # j* strictly inside a column tile
        assert 0 < j % c.tile[1] < c.tile[1] - 1 and j < c.n and c.kind == 'int'
    fams = [(c.family, c.dt, c.whole, c.tile[0]) for c, _ in FC.NAN_CASES]
    assert fams == [('colstats', 'f32', 0, 64), ('f64acc', 'f64acc', 1, 64), ('f64acc_b64', 'f64acc', 0, 64)]


@pytest.mark.parametrize('tag', FC.TAGS)
def test_removing_the_rows_that_carry_a_tag_fails_the_table_check(tag):
    left = [c for c in FC.CASES if tag not in c.tags]
    assert len(left) < len(FC.CASES)
    assert table_problems(left) != []


def test_removing_any_single_row_that_alone_carries_a_tag_fails_the_table_check():
    for fam_kind in {(c.family, c.dt, c.kind) for c in FC.CASES}:
        group = [c for c in FC.CASES if (c.family, c.dt, c.kind) == fam_kind]
        for t in FC.TAGS:
            sole = [c for c in group if t in c.tags]
            if len(sole) == 1 and t in ('misaligned_W', 'misaligned_X', 'ks_unaligned_base', 'tiles_512', 'vec_not_whole', 'p0_null'):
                assert table_problems([c for c in FC.CASES if c is not sole[0]]) != [], (fam_kind, t)


@pytest.mark.parametrize('case', FC.CASES, ids=FC.case_id)
def test_every_row_lands_where_it_states(case):
    assert row_problems(_lib(), case) == []


def test_a_misstated_row_is_noticed():
    lib = _lib()
    c = FC.find('f64acc', 'f64acc', 'int', (2, 256, 512), mis='W')
    assert row_problems(lib, c._replace(whole=1)) and row_problems(lib, c._replace(vec=(1, 1)))
    c = FC.find('lqbar', 'f32', 'int', (2, 65, 33))
    assert row_problems(lib, c._replace(tags=tuple(t for t in c.tags if t != 'ks_unaligned_batch')))
    c = FC.find('colstats', 'f32', 'int', (1, 256, 16384))
    assert row_problems(lib, c._replace(tile=(64, 64))) and row_problems(lib, c._replace(trows=4))


def test_the_wide_rows_are_needed_for_their_tiles():
    """The float32 128 x 64 and 128 x 128 tiles are not reachable at a fraction of the pinned widths."""
    lib = _lib()
    for c in FC.CASES:
        if c.family == 'colstats' and c.tile[0] == 128:
            half = c._replace(n=c.n // 2 // 4 * 4)
            assert (_plan(lib, half)[0], _plan(lib, half)[1]) != c.tile


# ---- exactness conditions on the built data ----------------------------------------------------------------------------
@pytest.mark.parametrize('case', [c for c in FC.CASES if c.kind == 'int'], ids=FC.case_id)
def test_int_rows_keep_every_partial_sum_an_exact_integer(case):
    d = FC.build(case)
    for name, t in d.items():
        if name not in ('L', 'Lq', 'W'):
            assert bool((t == t.round()).all()), name
    for name in ('L', 'Lq', 'W'):                        # the ignored triangle holds NaN, also under trans = 1
        if name in d:
            up = torch.ones(case.M, case.M, dtype=torch.bool).triu(1)
            assert bool(torch.isnan(d[name][:, up]).all()) and bool((d[name][:, ~up] == d['clean_L'][:, ~up]).all())
    dg = torch.diagonal(d['clean_L'], dim1=-2, dim2=-1) if 'clean_L' in d else torch.ones(1)
    assert bool((dg != 0).all())                         # a 1 x 1 product is not trivially 0
    if case.family in ('lqbar', 'lqbar_acc'):            # no term of the scaled sum can drop out unnoticed
        assert bool((d['gv'] != 0).all())
    bounds = FC.int_bounds(case, d)
    assert bounds
    for name, (reached, limit) in bounds.items():
        assert reached < limit, (name, reached, limit)
    if case.family == 'lqbar_acc':
        assert bool((GB.LQ_BETA * d['C0'] == (GB.LQ_BETA * d['C0']).round()).all()) and GB.LQ_BETA == -0.5


@pytest.mark.parametrize('case', [c for c in FC.CASES if c.kind == 'grid'], ids=FC.case_id)
def test_grid_rows_make_the_float64_host_product_exact(case):
    d = FC.build(case)
    units, on_grid, not_f32 = FC.grid_condition(case, d)
    assert on_grid and units < 2.0 ** 53
    assert not_f32 in (None, True)
    assert (d['X'].dtype == torch.float64) == (case.family in FC.B64_FAMILIES)
    assert bool((d['clean_L'] == d['clean_L'].round()).all()) and float(d['clean_L'].min()) >= -3 and float(d['clean_L'].max()) <= 4
    # the bound of the partials' test needs |v| |rv| exact: rv holds small integers
    assert bool((d['rv'] == d['rv'].round()).all()) and float(d['rv'].abs().max()) <= 2


@pytest.mark.parametrize('case', [c for c in FC.CASES if c.kind == 'kzx'], ids=FC.case_id)
def test_kzx_rows_make_the_float64_host_product_exact(case):
    d = FC.build(case)
    klo, khi, units = FC.kzx_range(case, d)
    assert 0 < klo < khi and units < 2.0 ** 53
    assert float(d['clean_L'].abs().max()) <= 4 and bool((d['clean_L'] == d['clean_L'].round()).all())


# ---- the reference functions against loops written from the formulas of include/nsgp.h ---------------------------------
def test_reference_functions_agree_with_naive_loops():
    g = torch.Generator().manual_seed(5)
    b, M, n, h = 2, 5, 3, 2
    r = lambda *s: torch.randint(-3, 4, s, generator=g).double()                             # noqa: E731
    L, X, rv = torch.tril(r(b, M, M)), r(b, M, n), r(b, M)
    for trans in (0, 1):
        Y, p0, p1 = FC.ref_colstats(L.transpose(-1, -2) if trans else L, X, rv, h)
        T = -(-M // h)
        assert p0.shape == p1.shape == (b, T, n)
        for bb in range(b):
            for j in range(n):
                col = [sum((L[bb, k, i] if trans else L[bb, i, k]) * X[bb, k, j] for k in range(M)) for i in range(M)]
                for i in range(M):
                    assert Y[bb, i, j] == col[i]
                for t in range(T):
                    rows = range(t * h, min(M, (t + 1) * h))
                    assert p0[bb, t, j] == sum(col[i] * rv[bb, i] for i in rows)
                    assert p1[bb, t, j] == sum(col[i] ** 2 for i in rows)
    C, A, m, gm, gv, C0 = r(b, M, n), r(b, M, n), r(b, M), r(b, n), r(b, n), 2 * r(b, M, M)
    ab = FC.ref_abar(L, C, A, m, gm, gv)
    lq = FC.ref_lqbar(A, C, gv)
    lqa = FC.ref_lqbar(A, C, gv, -0.5, C0)
    for bb in range(b):
        for k in range(M):
            for j in range(n):
                lc = sum(L[bb, k, i] * C[bb, i, j] for i in range(M))
                assert ab[bb, k, j] == 2 * lc * gv[bb, j] + m[bb, k] * gm[bb, j] - 2 * gv[bb, j] * A[bb, k, j]
            for l in range(M):
                s = sum(A[bb, k, j] * 2 * gv[bb, j] * C[bb, l, j] for j in range(n))
                assert lq[bb, k, l] == (s if l <= k else 0)
                assert lqa[bb, k, l] == (s - 0.5 * C0[bb, k, l] if l <= k else C0[bb, k, l])


def test_grid_reference_is_the_exact_sum():
    """On a tiny grid row the double-double partials equal sums formed with Python integers, and hi is their rounding."""
    from fractions import Fraction
    c = FC.find('f64acc_b64', 'f64acc', 'grid', (2, 63, 65))
    d = FC.build(c)
    ref = FC.grid_reference(c, d)
    V, h = ref['Y'], c.tile[0]
    for bb, t, j in ((0, 0, 0), (1, 0, 64), (1, 0, 17)):
        rows = range(t * h, min(c.M, (t + 1) * h))
        sq = sum(Fraction(float(V[bb, i, j])) ** 2 for i in rows)
        dot = sum(Fraction(float(V[bb, i, j])) * Fraction(float(d['rv'][bb, i])) for i in rows)
        for name, want in (('p1', sq), ('p0', dot)):
            hi, lo, mag = ref[name]
            assert Fraction(float(hi[bb, t, j])) + Fraction(float(lo[bb, t, j])) == want or \
                abs(Fraction(float(hi[bb, t, j])) + Fraction(float(lo[bb, t, j])) - want) <= abs(want) * Fraction(1, 2 ** 100)
            assert float(hi[bb, t, j]) == float(want)
        assert float(ref['p1'][2][bb, t, j]) == float(sq)
        assert Fraction(float(ref['p0'][2][bb, t, j])) == sum(abs(Fraction(float(V[bb, i, j])) * Fraction(float(d['rv'][bb, i]))) for i in rows)
    assert ref['rows'].flatten().tolist() == [63.0]
