"""csrc/gemm.hip may be restructured, never re-rounded: every output element keeps its sequence of MFMA accumulations over
the K-tiles and its epilogue arithmetic.  Every row of GEMM_CASES (tests/test_gemm_plan_cpu.py) on seeded normal operands
-- the exact tests of those rows use integers and do not see a change of summation order -- and every fused row of
tests/gemm_bits_cases.py (column statistics, the A-adjoint, the k-scaled split lower-only product, the float64-accumulating
projections with a float32, float64 or generated B operand) is held to the sha256 digests of its outputs recorded on the
commit before the file was restructured (tests/golden/gemm_hashes.json, written by tools/record_gemm_hashes.py, which
refuses to record results that miss the tolerances of the existing tests against the float64 dense formulas: the record
is of right answers)."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'gemm_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_gemm_hashes', os.path.join(ROOT, 'tools', 'record_gemm_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case', REC.all_cases(), ids=REC.case_id)
def test_gemm_outputs_are_bit_identical_to_the_record(case, record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    digests, _ = REC.run_case(case)
    ref = record[REC.case_id(case)]
    diff = sorted(name for name in set(ref) | set(digests) if ref.get(name) != digests.get(name))
    assert not diff, f'{REC.case_id(case)}: {diff} differ from the record'
