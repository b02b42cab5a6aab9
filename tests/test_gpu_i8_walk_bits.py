"""A workgroup of the int8 projection (csrc/gemm_i8.hip, i8_proj_kernel) walks consecutive column tiles of its tile row and
issues the next tile's first stage before the current tile's epilogue.  Per tile nothing may change: every shape of
tests/i8_walk_cases.py -- one to nine column tiles, whole and ragged last tile, full and short walks, one to three tile rows,
4 and 5 Kzx planes, 1 and 2 GPs, with and without the row vector, float32 and float64 partials -- is held to the sha256
digests of A and of both partials planes, guard words included, recorded on the commit before the walk
(tests/golden/i8_walk_hashes.json, written by tools/record_i8_walk_hashes.py, which refuses wrong results).  Here too A is
held to the float64 product, the partials to the column sums of A, the guard words to their value, and a NaN digit-scale
slot in the last K-block that the tiles of two full walks read has to reach exactly their columns of that tile row."""
import importlib.util
import json
import os

import pytest
import torch

import i8_walk_cases as WC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'i8_walk_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_i8_walk_hashes', os.path.join(ROOT, 'tools', 'record_i8_walk_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['shapes']


def test_record_holds_every_shape(record):
    assert sorted(record) == sorted([f'{M},{n}' for M, n in WC.SHAPES] + ['nan'])
    assert all(len(v) == 3 and all(len(h) == 64 for h in v) for v in record.values())


@pytest.mark.parametrize('M', WC.ROWS)
def test_walked_projection_is_bit_identical_to_the_record_and_right(M, record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    shapes = [s for s in WC.SHAPES if s[0] == M]
    digests, wrong = REC.record(shapes, checked=True)
    assert len(digests) == len(shapes) * len(WC.VARIANTS)
    assert not wrong, wrong                                   # guard words, the float64 product, the column sums
    folded = REC.fold(digests, shapes)
    diff = {k: [name for name, a, b in zip(('A', 'part_dot', 'part_sq'), v, record[k]) if a != b]
            for k, v in folded.items() if v != record[k]}
    assert not diff, f'{len(diff)} of {len(folded)} shapes differ from the record: {diff}'


def test_nan_digit_scale_slot_reaches_exactly_the_tiles_that_read_it(record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    digests, why = REC.nan_case()
    assert not why, why
    assert digests == record['nan']
