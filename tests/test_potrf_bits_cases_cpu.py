"""The case table of the potrf bit pin (tests/potrf_bits_cases.py), checked on the host (no GPU): it holds every case the
pin was specified with, every case has a line in the record, and -- with each case's path derived from n, batch and the
switches by the arithmetic of `potrf_impl`, `potrf_inv_impl` and `trtri_impl` (csrc/potrf.hip) -- the table reaches every
branch listed here for both dtypes.  Dropping a case fails `test_the_table_holds_every_specified_case`; a host change that
moves a case off its branch fails `test_the_table_reaches_every_branch` and is answered by adding the shape that reaches it."""
import json
import os

import pytest

import potrf_bits_cases as PB

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'potrf_hashes.json')

POTRF_BRANCHES = {
    'tail_only', 'panel_first', 'panel_rows0', 'panel_pre', 'panel_pre_no_slab', 'tail_pre', 'ragged_slab', 'several_slabs',
    'update_tiles', 'full_update_tile', 'ragged_update_tile', 'triangle_tn_ge_3', 'update_rows_below_triangle',
    'batched_update_tiles', 'outer_panel_gemm', 'lone_panel_after_gemm', 'tail_pre_after_gemm', 'strided_A',
    'bad_in_panel0', 'bad_in_later_panel', 'bad_in_tail', 'bad_in_middle_of_batch'}
INV_BRANCHES = {
    'single_panel', 'chunk_diag', 'chunk_first_touched', 'chunk_already_updated', 'syrk_tiles', 'pupd_first_touched',
    'pupd_accumulates', 'pupd_two_row_blocks', 'batched', 'headline_chain', 'largest_one_level', 'fallback_ragged',
    'fallback_large', 'fallback_switch', 'strided_X'}
TRTRI_BRANCHES = {'diag_only', 'full_diag_blocks', 'ragged_diag_block', 'full_pairs', 'rem_gt_s', 'rem_gt_s_after_full_pairs',
                  'second_level'}


def _specified():
    """The cases as the pin was specified, written out independently of the table's own construction."""
    ids = []
    for dt in ('f64', 'f32'):
        ids += [f'potrf|{dt}|n{n}b1' for n in (1, 7, 63, 64, 65, 128, 130, 192, 200, 320, 448, 2112, 2149)]
        ids += [f'potrf|{dt}|n200b3', f'potrf|{dt}|n320b3', f'potrf|{dt}|n2112b1|NB2=4', f'potrf|{dt}|n200b2|ldA']
        ids += [f'potrf|{dt}|n200b1|bad0@{m}' for m in (6, 151, 195)] + [f'potrf|{dt}|n200b3|bad1@151']
        ops = ('potrf_trtri', 'potrf_trtri_w32') if dt == 'f64' else ('potrf_trtri',)
        for op in ops:
            ids += [f'{op}|{dt}|n{n}b{b}' for n in (64, 128, 192, 256, 320) for b in (1, 2)]
            ids += [f'{op}|{dt}|n1024b3', f'{op}|{dt}|n2048b1', f'{op}|{dt}|n200b1', f'{op}|{dt}|n2112b1',
                    f'{op}|{dt}|n192b1|INV=0', f'{op}|{dt}|n192b2|ldX']
        ids += [f'trtri|{dt}|n{n}b1' for n in (1, 63, 64, 65, 130, 200, 1100)]
    return ids


def test_the_table_holds_every_specified_case():
    got = [PB.case_id(c) for c in PB.CASES]
    assert len(set(got)) == len(got)
    assert sorted(got) == sorted(_specified())


def test_the_record_has_a_line_for_every_case():
    with open(RECORD) as f:
        rec = json.load(f)['cases']
    assert sorted(rec) == sorted(PB.case_id(c) for c in PB.CASES)
    assert all(v and all(len(h) == 64 for h in v.values()) for v in rec.values())


@pytest.mark.parametrize('dt', PB.DTYPES)
def test_the_table_reaches_every_branch(dt):
    reached = {'potrf': set(), 'inv': set(), 'trtri': set()}
    for c in PB.CASES:
        if c.dt == dt:
            reached['potrf' if c.op == 'potrf' else 'trtri' if c.op == 'trtri' else 'inv'] |= PB.path(c)
    assert POTRF_BRANCHES - reached['potrf'] == set()
    assert INV_BRANCHES - reached['inv'] == set()
    assert TRTRI_BRANCHES - reached['trtri'] == set()
    if dt == 'f64':         # the float32 copy is written on the fused path and cast on every fallback
        w32 = set().union(*(PB.path(c) for c in PB.CASES if c.op == 'potrf_trtri_w32'))
        assert INV_BRANCHES - w32 == set()


def test_each_specified_shape_lands_where_it_was_chosen_for():
    """The reason each shape is in the table, checked against the hosts' arithmetic."""
    P = lambda n, batch=1, **kw: PB.potrf_path(PB.Case('potrf', 'f64', n, batch, tuple(kw.get('env', ())), (), ''))
    for n in (1, 7, 63):
        assert P(n) == {'tail_only'}
    assert P(64) == {'panel_first', 'panel_rows0'}
    assert 'tail_pre' in P(65) and 'update_tiles' not in P(65)
    assert 'panel_pre_no_slab' in P(128) and 'update_tiles' not in P(128)
    assert 'ragged_update_tile' in P(130)
    assert 'full_update_tile' in P(192) and 'update_tiles' not in P(128)
    assert {'ragged_slab', 'tail_pre'} <= P(200)
    assert 'triangle_tn_ge_3' in P(320) and 'triangle_tn_ge_3' in P(448) and 'triangle_tn_ge_3' not in P(200)
    assert 'batched_update_tiles' in P(200, 3) and 'batched_update_tiles' in P(320, 3)
    assert {'outer_panel_gemm', 'lone_panel_after_gemm'} <= P(2112) and 'tail_pre_after_gemm' not in P(2112)
    assert {'outer_panel_gemm', 'tail_pre_after_gemm'} <= P(2149)
    # tm > tn: one level (n <= 2048) never has it; a 256-column outer panel puts up to 29 full tile rows under a triangle of 2
    assert 'update_rows_below_triangle' not in P(2048) and 'update_rows_below_triangle' not in P(448)
    assert 'update_rows_below_triangle' in P(2112, env=[('NSGP_POTRF_NB2', '4')])
    assert max(l[6] - l[7] for l in PB.potrf_launches(2112, 4) if l[0] == 'step') == 29
    I = lambda n, batch=1: PB.inv_path(PB.Case('potrf_trtri', 'f64', n, batch, (), (), ''))
    assert 'chunk_already_updated' in I(192) and 'chunk_already_updated' not in I(128)
    assert 'pupd_two_row_blocks' in I(256) and 'pupd_two_row_blocks' not in I(192)
    assert I(200) == {'fallback_ragged'} and I(2112) == {'fallback_large'}
    T = lambda n: PB.trtri_path(PB.Case('trtri', 'f64', n, 1, (), (), ''))
    assert 'rem_gt_s_after_full_pairs' in T(1100) and 'second_level' in T(1100)
