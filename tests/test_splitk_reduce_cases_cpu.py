"""What the case table of the split-K reduce (tests/splitk_reduce_cases.py) has to reach, asked of the table itself and of
the library's planner (nsgp_gemm_plan: host-side, no GPU): both reduce kernels, the groups the diagonal cuts, the zero-filled
strict upper part, every flag, size, K, batch form, alpha, beta and dtype on either kernel, and K-slice counts below, at and
above the vector kernel's unroll width as well as a row that is not split at all."""
import importlib.util
import os

import splitk_reduce_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _recorder():
    spec = importlib.util.spec_from_file_location('record_splitk_reduce_hashes',
                                                  os.path.join(ROOT, 'tools', 'record_splitk_reduce_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
KSPLIT = {c: REC.ksplit(c) for c in SC.CASES}
SPLIT = [c for c in SC.CASES if KSPLIT[c] > 1]


def test_rows_are_unique_and_name_themselves():
    assert len({SC.case_id(c) for c in SC.CASES}) == len(SC.CASES) == len(set(SC.CASES))


def test_every_value_of_every_dimension_reaches_both_kernels():
    for vec in (True, False):
        rows = [c for c in SPLIT if SC.vector_path(c) == vec]
        sizes = {c.M for c in rows}
        assert sizes == (set(SC.SIZES) - {102} if vec else set(SC.SIZES)), (vec, sizes)
        for field, values in (('K', SC.KS), ('batch', SC.BATCHES), ('flags', SC.FLAGS), ('alpha', SC.ALPHAS),
                              ('beta', SC.BETAS), ('dt', SC.DTS)):
            assert {getattr(c, field) for c in rows} >= set(values), (vec, field)
        for dt in SC.DTS:                                     # every flag in either arithmetic
            assert {c.flags for c in rows if c.dt == dt} == set(SC.FLAGS), (vec, dt)


def test_scalar_kernel_is_reached_by_each_of_its_reasons():
    assert any(c.M % 4 != 0 and c.ldpad == 0 for c in SPLIT)                  # N % 4 != 0 alone
    assert any(c.M % 4 == 0 and c.ldpad == 1 for c in SPLIT)                  # unaligned rows alone
    assert all(SC.vector_path(c) for c in SPLIT if c.M % 4 == 0 and c.ldpad == 0)   # the batch gap keeps the alignment


def test_diagonal_cut_groups_and_zero_filled_upper_part():
    for dt in SC.DTS:
        vec = [c for c in SPLIT if SC.vector_path(c) and c.dt == dt]
        lower = [c for c in vec if c.flags & SC.CL]           # every row of a lower output has a group the diagonal cuts
        assert lower
        assert any(SC.zero_filled_upper(c) and c.M // 4 > 1 for c in lower)       # the store-only index range
        assert any(not SC.zero_filled_upper(c) for c in lower)                    # ... and rows without it (beta != 0)
        assert any(c.flags & SC.HD and c.beta != 0 for c in lower) and any(c.flags & SC.HD and c.beta == 0 for c in lower)
        assert any(SC.zero_filled_upper(c) and c.batch != '1' for c in lower)
        # sizes whose last tile is cut by the matrix edge, and more than one block of the reduce (> 256 groups)
        assert {100, 132} <= {c.M for c in lower} and any(c.M * (c.M // 4) > 256 for c in vec)


def test_k_slices_below_at_and_above_the_unroll_width():
    for vec in (True, False):
        for dt in SC.DTS:
            ks = {KSPLIT[c] for c in SC.CASES if SC.vector_path(c) == vec and c.dt == dt}
            assert any(1 < k < SC.UNROLL for k in ks) and SC.UNROLL in ks and any(k > SC.UNROLL for k in ks), (vec, dt, ks)
            assert any(k > SC.UNROLL and k % SC.UNROLL for k in ks) and any(k > SC.UNROLL and k % SC.UNROLL == 0 for k in ks)
    assert {KSPLIT[c] for c in SC.CASES if c.K in SC.KS} == {2, 9, 16}
    for dt in SC.DTS:
        assert any(KSPLIT[c] == 1 for c in SC.CASES if c.dt == dt)                # no reduce: out64 is refused there


def test_layouts_keep_what_the_vector_kernel_needs_and_guards_exist():
    for c in SC.CASES:
        ldc, stride, total = SC.layout(c)
        assert ldc >= c.M and stride > c.M * ldc and total > 2 * SC.GUARD_WORDS
        assert (SC.GUARD_WORDS * 4) % 16 == 0                  # C starts 16-byte aligned in a float32 buffer (32 in float64)
        nb1, nb2 = SC.batch_levels(c)
        assert nb1 * nb2 == (1 if c.batch == '1' else 2)
