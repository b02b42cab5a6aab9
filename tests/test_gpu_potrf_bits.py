"""csrc/potrf.hip may be restructured, never re-rounded: every element of L, of the inverse and of its float32 copy keeps
its arithmetic and the order of that arithmetic (the panel workgroups and the inverse's row-block workgroups factor the same
diagonal block and rely on agreeing bit for bit).  Every case of tests/potrf_bits_cases.py -- each launch path of potrf,
of the fused factor-and-inverse and of trtri, padded strides with guard words, bad pivots in the first panel, a later panel,
the tail and the middle of a batch -- is held to the sha256 digests of its outputs recorded on the commit before the file
was restructured (tests/golden/potrf_hashes.json, written by tools/record_potrf_hashes.py, which refuses to record results
that miss test_potrf_and_trtri's tolerances against float64 LAPACK: the record is of right answers)."""
import importlib.util
import json
import os

import pytest
import torch

import potrf_bits_cases as PB

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'potrf_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_potrf_hashes', os.path.join(ROOT, 'tools', 'record_potrf_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case', PB.CASES, ids=PB.case_id)
def test_potrf_outputs_are_bit_identical_to_the_record(case, record, monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    digests, out = REC.run_case(case)
    assert out.get('guards', True), 'a guard word next to the output was overwritten'
    ref = record[PB.case_id(case)]
    diff = sorted(name for name in set(ref) | set(digests) if ref.get(name) != digests.get(name))
    assert not diff, f'{PB.case_id(case)}: {diff} differ from the record'
