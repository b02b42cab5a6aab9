"""The int8 projection kernel's schedule (csrc/gemm_i8.hip: how the K-block stages are filled and waited for, when the
epilogue's operands are fetched) must not move one output bit: the product is exact integer accumulation and one rounding.  Every case of
tools/record_i8_projection_hashes.py -- row counts of one to four K-blocks (fewer than, equal to and more than the ring's
depth), an almost empty second row tile, odd and even numbers of row tiles, the headline's 1024 rows; partial and whole
column tiles; 4 and 5 Kzx planes; 1 and 2 GPs; with and without the row vector; float32 and float64 partials -- is held to
the sha256 digests of A and of both partials planes recorded on the commit before the pipeline changed
(tests/golden/i8_projection_hashes.json: per shape, the digest of its 16 variants' digests for each of the three arrays),
and A to the float64 product so that the record is of right answers."""
import importlib.util
import json
import os

import pytest
import torch

from conftest import measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'i8_projection_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_i8_projection_hashes',
                                                  os.path.join(ROOT, 'tools', 'record_i8_projection_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
_ROWS = sorted({M for M, _ in REC.SHAPES})
_cache = {}


def _run(M):
    """Digests and value-check results of every case with M rows, computed once and shared by the two tests."""
    if M not in _cache:
        values = []

        def check(t, planes, A):
            # the bound of tests/test_gpu_i8.py::test_i8_projection_shapes_and_digit_scale_edges, for 4 and 5 planes alike,
            # per GP: a few 1e-8 of the product scale max sum|W||K| (35-bit W digits, dropped digit pairs), the float32
            # rounding of A, and the Kzx digits' own floor 2^-(7 planes - 1) |os| max_m sum_k |W[m][k]|
            A_ref, Kzx = REC.float64_product(t)
            W64, os_ = t['W64'].cpu(), t['os'].cpu()
            for i in range(A_ref.shape[0]):
                scale = float((W64[i].abs() @ Kzx[i].abs()).max())
                amax = float(A_ref[i].abs().max())
                kfloor = 2.0 ** -(7 * planes - 1) * abs(float(os_[i])) * float(W64[i].abs().sum(-1).max())
                name = f'i8 pipeline M{M} n{A_ref.shape[2]} planes {planes} GP {i} of {A_ref.shape[0]}'
                ok = bool(torch.isfinite(A[i]).all()) and measured(name, A[i], A_ref[i], rtol=0.0,
                                                                   atol=2e-8 * scale + 1.2e-7 * amax + kfloor)
                values.append((name, ok))
        digests = REC.record([s for s in REC.SHAPES if s[0] == M], on_product=check)
        _cache[M] = (digests, values)
    return _cache[M]


def test_record_holds_every_case():
    with open(RECORD) as f:
        rec = json.load(f)['shapes']
    assert sorted(rec) == sorted(f'{M},{n}' for M, n in REC.SHAPES)
    assert all(len(v) == 3 and all(len(h) == 64 for h in v) for v in rec.values())


@pytest.mark.parametrize('M', _ROWS)
def test_i8_projection_is_bit_identical_to_the_record(M):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    with open(RECORD) as f:
        rec = json.load(f)['shapes']
    digests, _ = _run(M)
    assert sorted(digests) == sorted(REC.case_key(*c) for c in REC.CASES if c[0] == M)       # every variant was run
    folded = REC.fold(digests)
    diff = {k: [name for name, a, b in zip(('A', 'part_dot', 'part_sq'), v, rec[k]) if a != b]
            for k, v in folded.items() if v != rec[k]}
    assert not diff, f'{len(diff)} of {len(folded)} shapes differ from the record: {diff}'


@pytest.mark.parametrize('M', _ROWS)
def test_i8_projection_matches_the_float64_product(M):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    _, values = _run(M)
    assert len(values) == 3 * 2 * len([s for s in REC.SHAPES if s[0] == M])     # (1 + 2 GPs) x 2 plane counts per shape
    bad = [name for name, ok in values if not ok]
    assert not bad, bad
