"""The case tables of the exact bf16 tests (tests/bf16_cases.py), checked on the host (no GPU): the projection table holds
every case it was specified with and reaches every K-tile count of `bf16_proj_kernel`'s pipeline in both triangle modes;
the conditions under which tests/test_gpu_bf16_kernels.py may ask for BIT equality (every float32 partial sum an integer
below 2^24) hold, computed from the float64 reference alone; the RBF inputs keep the share of elements whose bf16 rounding
the float32 evaluation error could move small.  Dropping a case fails `test_the_projection_table_holds_every_specified_case`;
a kernel or host change that moves a case off its branch fails `test_the_projection_table_reaches_every_branch`."""
import pytest
import torch

import bf16_cases as BC

TWO24 = float(2 ** 24)


def _specified():
    """The projection cases as specified, written out independently of the table's own construction."""
    ids = []
    for tri in ('lower', 'upper'):
        for M, n in ((8, 1), (72, 127), (136, 129), (200, 128), (264, 200), (328, 129), (392, 200), (128, 128), (256, 127)):
            b = 3 if (tri, M) in (('lower', 136), ('upper', 200)) else 1
            ids.append(f'{tri}|b{b}|M{M}|n{n}|small')
        ids += [f'{tri}|b1|M136|n200|wide', f'{tri}|b1|M264|n127|wide', f'{tri}|b1|M392|n129|wide', f'{tri}|b1|M392|n200|real']
    ids += ['lower|b1|M136|n129|small|norv', 'upper|b1|M264|n1|small|norv', 'lower|b1|M264|n127|small|noyt',
            'upper|b1|M136|n200|small|noyt', 'upper|b1|M392|n129|small|norv|noyt']
    return ids


def test_the_projection_table_holds_every_specified_case():
    got = [BC.case_id(c) for c in BC.PROJ_CASES]
    assert len(set(got)) == len(got) == len(set(BC.PROJ_CASES))
    assert sorted(got) == sorted(_specified())
    assert len(got) <= 40 and all(c.M <= 392 and c.n <= 200 for c in BC.PROJ_CASES)


def test_the_projection_table_reaches_every_branch():
    reached = set().union(*(BC.proj_path(c) for c in BC.PROJ_CASES))
    assert BC.PROJ_TAGS - reached == set() and reached - BC.PROJ_TAGS == set()
    for mode in ('lower', 'upper'):
        paths = [BC.proj_path(c) for c in BC.PROJ_CASES]
        for tag in BC.NT_TAGS:
            assert any({tag, mode} <= p for p in paths), (tag, mode)
        # ... and every K-tile count with exact data, where a wrong tile cannot hide in a tolerance
        exact = set().union(*(BC.proj_path(c) for c in BC.PROJ_CASES if c.data == 'small' and mode in BC.proj_path(c)))
        assert set(BC.NT_TAGS) <= exact, (mode, exact)
    for sw in ('no_rowvec', 'no_yt'):                       # the optional operands are left out in either mode
        assert {c.tri for c in BC.PROJ_CASES if sw in BC.proj_path(c)} == {BC.LOWER, BC.UPPER}
    assert {c.data for c in BC.PROJ_CASES} == {'small', 'wide', 'real'}
    assert sum(c.batch == 3 for c in BC.PROJ_CASES) == 2
    assert {c.n for c in BC.PROJ_CASES} == {1, 127, 128, 129, 200}


def test_each_shape_lands_where_it_was_chosen_for():
    nts = lambda tri, M: [r[2] for r in BC.proj_tiles(BC.ProjCase(tri, 1, M, 128, True, True, 'small'))[2]]
    want = {8: ([1], [1]), 72: ([2], [2]), 136: ([2, 3], [3, 1]), 200: ([2, 4], [4, 2]), 264: ([2, 4, 5], [5, 3, 1]),
            328: ([2, 4, 6], [6, 4, 2]), 392: ([2, 4, 6, 7], [7, 5, 3, 1]), 128: ([2], [2]), 256: ([2, 4], [4, 2])}
    for M, (lo, up) in want.items():
        assert nts(BC.LOWER, M) == lo and nts(BC.UPPER, M) == up, M
    # the K ranges themselves, at the shape with the most row tiles
    assert BC.proj_tiles(BC.ProjCase(BC.LOWER, 1, 392, 1, True, True, 'small'))[2] == \
        [(0, 128, 2), (0, 256, 4), (0, 384, 6), (0, 392, 7)]
    assert BC.proj_tiles(BC.ProjCase(BC.UPPER, 1, 392, 1, True, True, 'small'))[2] == \
        [(0, 392, 7), (128, 392, 5), (256, 392, 3), (384, 392, 1)]


@pytest.mark.parametrize('case', BC.PROJ_CASES, ids=BC.case_id)
def test_projection_operands_keep_the_kernels_contract(case):
    P, Qt, rv = BC.proj_inputs(case)
    assert P.dtype == Qt.dtype == torch.bfloat16 and rv.dtype == torch.float32
    assert P.shape == (case.batch, case.M, case.M) and Qt.shape == (case.batch, case.n, case.M)
    other = torch.triu(P.float(), 1) if case.tri == BC.LOWER else torch.tril(P.float(), -1)
    assert not bool(other.any())                            # the triangle's zeros are in memory
    assert bool(torch.diagonal(P.float(), dim1=-2, dim2=-1).any())
    if case.data != 'real':
        a = 2 if case.data == 'small' else 16
        for t in (P.float(), Qt.float(), rv):
            assert bool((t == t.round()).all()) and float(t.abs().max()) == a


@pytest.mark.parametrize('case', [c for c in BC.PROJ_CASES if c.data != 'real'], ids=BC.case_id)
def test_exactness_conditions_of_the_integer_data(case):
    ref = BC.proj_reference(case)
    Y = ref['Y']
    assert bool((Y == Y.round()).all())
    assert float(ref['absY'].max()) < TWO24                 # every partial sum of every element of Y, in any order
    if case.data == 'small':
        # the statistics: every partial sum over the 128 rows of a tile is an integer below 2^24 (and so is each Y^2)
        assert float(ref['abs_dot'].max()) < TWO24 and float(ref['part_sq'].max()) < TWO24
        assert float(Y.abs().max()) < 4096.0
    else:
        # ties of the bf16 grid in both directions: odd integers in [257, 511] (spacing 2); the even neighbour's last
        # mantissa bit decides whether nearest-even rounds down (y % 4 == 1) or up (y % 4 == 3)
        a = Y.abs()
        ties = a[(a >= 257) & (a <= 511) & (a % 2 == 1)]
        assert int((ties % 4 == 1).sum()) >= 10 and int((ties % 4 == 3).sum()) >= 10
        assert float((a > 256).double().mean()) > 0.25
        back = Y.float().to(torch.bfloat16).double()
        assert bool((back != Y).any())                      # the bf16 copy does round


def test_planted_values_round_as_the_cast_test_assumes():
    """The host conversion the cast tests compare with: float64 -> float32 -> bf16, nearest-even."""
    bits = lambda v, dt: int(torch.tensor([v], dtype=dt).to(torch.float32).to(torch.bfloat16).view(torch.int16)[0]) & 0xFFFF
    for dt in (torch.float32, torch.float64):
        assert bits(1.0 + 2.0 ** -8, dt) == 0x3F80 and bits(1.0 + 3 * 2.0 ** -8, dt) == 0x3F82
        assert bits(-(1.0 + 2.0 ** -8), dt) == 0xBF80
        assert bits(0.0, dt) == 0x0000 and bits(-0.0, dt) == 0x8000
        assert bits(float('inf'), dt) == 0x7F80 and bits(-float('inf'), dt) == 0xFF80
        assert bits(3.4e38, dt) == 0x7F80 and bits(-3.4e38, dt) == 0xFF80
        assert bits(1e-40, dt) == 0x0001
    assert bits(1.0 + 2.0 ** -8 + 2.0 ** -40, torch.float64) == 0x3F80       # directly it would be 0x3F81
    assert bits(1e300, torch.float64) == 0x7F80 and bits(-1e-300, torch.float64) == 0x8000


def test_cast_and_transpose_tables_cover_their_dimensions():
    for dt in ('f32', 'f64'):
        rows = [c for c in BC.CAST_CASES if c.dt == dt]
        assert {c.n for c in rows} == {1, 7, 16, 17, 200} and {c.batch for c in rows} == {1, 3}
        for n in (1, 7, 16, 17, 200):
            assert {(c.transpose, c.tril) for c in rows if c.n == n} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert any(c.batch * c.n * c.n > 256 and (c.batch * c.n * c.n) % 256 for c in rows)       # a ragged last block
    assert len(set(BC.CAST_CASES)) == len(BC.CAST_CASES)
    for c in BC.CAST_CASES:
        src, ref = BC.cast_input(c), BC.cast_reference(c)
        assert bool(src.isnan().any()) or src.numel() < 5 * len(BC.planted_values(c.dt))
        if c.tril and c.n > 1:                              # the NaN above the diagonal comes out as zero
            assert bool(src[:, 0, c.n - 1].isnan().all())
            out = ref[:, c.n - 1, 0] if c.transpose else ref[:, 0, c.n - 1]
            assert bool((out.view(torch.int16) == 0).all())
    for dim in ('M', 'n'):                                  # the 32 x 32 LDS tile: below, at and above 32 and 64
        v = {getattr(c, dim) for c in BC.TCAST_CASES}
        assert {1, 31, 32, 33, 64, 65} <= v and max(v) > 128
    assert any(c.batch > 1 for c in BC.TCAST_CASES)


def test_rbf_table_covers_its_dimensions():
    assert {c.M for c in BC.RBF_CASES} == {1, 7, 8, 13, 200} and {c.D for c in BC.RBF_CASES} == {1, 3, 8}
    assert {c.n for c in BC.RBF_CASES} == {1, 33, 65}
    for vec in (True, False):                               # 16-byte stores (M % 8 == 0) and element stores
        rows = [c for c in BC.RBF_CASES if (c.M % 8 == 0) == vec]
        assert {c.shared_x for c in rows} == {True, False} and any(c.batch > 1 for c in rows)
        assert any(c.D == 8 for c in rows)
    assert any(c.batch > 1 and not c.shared_x and c.n > 1 for c in BC.RBF_CASES)


@pytest.mark.parametrize('case', BC.RBF_CASES, ids=BC.case_id)
def test_rbf_inputs_keep_the_midpoint_condition(case):
    s, v = BC.rbf_reference(case)
    assert v.shape == (case.batch, case.n, case.M)
    assert float(s.max()) <= BC.RBF_MAX_S
    assert float(v.min()) > 2.0 ** -126 * 256               # nothing near the subnormals of bf16
    lo, hi, mid = BC.bf16_neighbours(v)
    assert bool((lo <= v).all()) and bool((v < hi).all())
    assert bool((lo.float().to(torch.bfloat16).double() == lo).all()) and bool((hi.float().to(torch.bfloat16).double() == hi).all())
    # the float32 restatement of the kernel's arithmetic stays inside delta (measured: 1.4e-6 at worst)
    dev = float(((BC.rbf_restated_f32(case).double() - v).abs() / v).max())
    assert dev < BC.RBF_DELTA / 8, dev
    # ... and its verdict is the one the GPU test asks of the kernel
    got = BC.rbf_restated_f32(case).to(torch.bfloat16).double()
    neighbour, nearest, decided = BC.rbf_verdict(case, got)
    assert bool(neighbour.all()) and bool(nearest[decided].all())
    if v.numel() >= 1000:
        assert float((~decided).double().mean()) < 0.03


def test_rbf_midpoint_zone_is_small_over_the_table():
    und = sum(int((~BC.rbf_verdict(c, BC.rbf_reference(c)[1])[2]).sum()) for c in BC.RBF_CASES)
    tot = sum(c.batch * c.n * c.M for c in BC.RBF_CASES)
    assert und / tot < 0.03, und / tot
