"""The case table of the GEMM bit pin (tests/gemm_bits_cases.py), checked on the host (no GPU): every fused row lands on
the tile and `whole` value it states -- asked of the library's own planners: `nsgp_gemm_plan` for the families gemm_impl
launches (it plans fused launches with the same make_plan; float64 never takes 128-row tiles, fused or not),
`nsgp_svgp_f64acc_tiles_for` / `nsgp_svgp_kzx_gemm_supported` for the float64-accumulating families -- the table holds
every combination the pin was specified with, and the record has a line for every case and no other.  A planner change that
moves a row fails here and is answered by adding the shape that reaches the combination it left, never by dropping it."""
import ctypes
import json
import os

import pytest

import gemm_bits_cases as GB
from test_gemm_plan_cpu import GEMM_CASES

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_hashes.json')


def _specified():
    """The fused cases as the pin was specified, written out independently of the table's own construction."""
    ids = []
    small = ['b2M128n192', 'b2M63n65', 'b1M130n700']
    wide = ['b1M256n16384', 'b1M250n16400', 'b1M256n38400', 'b1M250n38500']
    for fam in ('colstats', 'colstats_t', 'abar'):
        ids += [f'{fam}|f32|{s}' for s in small + wide] + [f'{fam}|f64|{s}' for s in small]
    ids += [f'colstats_rows|{dt}|b1M130n700' for dt in ('f32', 'f64')]
    for dt in ('f32', 'f64'):
        ids += [f'lqbar|{dt}|b1M192n300|split=0', f'lqbar|{dt}|b1M192n4096|split=1', f'lqbar|{dt}|b1M200n1000|split=1']
        ids += [f'lqbar_acc|{dt}|b1M192n4096|split=1', f'lqbar_acc|{dt}|b1M192n300|split=0']
    ids += ['lqbar|f32|b2M256n16384|split=1', 'lqbar|f32|b1M2944n256|split=0']
    for fam in ('f64acc', 'f64acc_b64', 'f64acc_b64p32', 'f64acc_t'):
        ids += [f'{fam}|f64acc|{s}' for s in ('b2M256n512', 'b1M200n333', 'b1M256n16384', 'b2M250n8200')]
    ids += ['kzx|f64acc|b2M256n512|D=3|xb=0', 'kzx|f64acc|b1M256n16384|D=1|xb=0', 'kzx|f64acc|b1M256n16384|D=4|xb=0',
            'kzx|f64acc|b3M128n128|D=4|xb=1']
    return ids


# (family group, dtype, tile, whole) combinations that exist and must each have a row
COMBINATIONS = (
    [(fam, 'f32', t, w) for fam in ('colstats', 'colstats_t', 'abar') for t in ((64, 64), (128, 64), (128, 128)) for w in (0, 1)] +
    [(fam, 'f64', (64, 64), w) for fam in ('colstats', 'colstats_t', 'abar') for w in (0, 1)] +
    [(fam, 'f64acc', (r, 64), w) for fam in GB.F64ACC_FAMILIES for r in (64, 128) for w in (0, 1)] +
    [('kzx', 'f64acc', (r, 64), 1) for r in (64, 128)])


def test_the_table_holds_every_specified_case():
    got = [GB.case_id(c) for c in GB.CASES]
    assert len(set(got)) == len(got)
    assert sorted(got) == sorted(_specified())
    have = {(c.family, c.dt, c.tile, c.whole) for c in GB.CASES}
    assert [k for k in COMBINATIONS if k not in have] == []
    lq = {(c.dt, c.tile, dict(c.opt)['split'], c.whole) for c in GB.CASES if c.family == 'lqbar'}
    for dt in ('f32', 'f64'):          # unsplit / split 64-tiles, a ragged split, and float32's 128-tiles split and unsplit
        assert {(dt, (64, 64), 0, 0), (dt, (64, 64), 1, 1), (dt, (64, 64), 1, 0)} <= lq
    assert {('f32', (128, 128), 1, 1), ('f32', (128, 128), 0, 1)} <= lq
    acc = {(c.dt, dict(c.opt)['split']) for c in GB.CASES if c.family == 'lqbar_acc'}
    assert acc == {(dt, s) for dt in ('f32', 'f64') for s in (0, 1)} and GB.LQ_BETA != 0
    assert any(dict(c.opt)['xb'] for c in GB.CASES if c.family == 'kzx')
    assert {dict(c.opt)['D'] for c in GB.CASES if c.family == 'kzx'} >= {1, 3, 4}


@pytest.mark.parametrize('case', GB.CASES, ids=GB.case_id)
def test_every_fused_row_lands_on_the_tile_it_states(case):
    import nsgp
    lib = nsgp.load_library()
    if case.family in GB.GEMM_IMPL_FAMILIES:
        M, N, K, flags, ma, mb = GB.gemm_query(case)
        va, vb = GB.gemm_vec(case)
        buf = (ctypes.c_int32 * 11)()
        assert lib.nsgp_gemm_plan(M, N, K, case.batch, 1, 4 if case.dt == 'f32' else 8, flags, va, vb, ma, mb,
                                  ctypes.cast(buf, ctypes.c_void_p)) == 0
        assert (buf[0], buf[1]) == case.tile and buf[4] == case.whole, tuple(buf)
        if case.family in ('lqbar', 'lqbar_acc'):
            assert int(buf[2] > 1) == dict(case.opt)['split'], tuple(buf)
            # the lower triangle of the unsplit 128-tile row has at least 256 tiles (what makes the planner take 128-tiles)
            if case.tile == (128, 128) and not dict(case.opt)['split']:
                assert buf[7] >= 256
        else:
            assert buf[2] == 1
            tiles = lib.nsgp_svgp_colstats_tiles(case.M, case.n, case.batch, 4 if case.dt == 'f32' else 8)
            assert tiles == -(-case.M // case.tile[0])
    else:
        rows = lib.nsgp_svgp_f64acc_tiles_for(case.M, case.n, case.batch)
        assert rows == -(-case.M // case.tile[0]) and rows != -(-case.M // (192 - case.tile[0]))
        aligned = ctypes.c_void_p(4096)                  # only the pointer's alignment is looked at
        D = dict(case.opt).get('D', 1)
        assert lib.nsgp_svgp_kzx_gemm_supported(aligned, case.M, case.n, case.batch, D) == case.whole


def test_the_record_has_a_line_for_every_case_and_no_other():
    with open(RECORD) as f:
        rec = json.load(f)['cases']
    want = ['plain|' + c.name for c in GEMM_CASES] + [GB.case_id(c) for c in GB.CASES]
    assert sorted(rec) == sorted(want)
    assert all(v and all(len(h) == 64 for h in v.values()) for v in rec.values())
