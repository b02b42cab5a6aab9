"""The DSVI objective's kernels (csrc/svgp.hip: Gaussian expected log-likelihood, whitened and mean-field KL, their adjoints,
in the per-term, one-scalar and fused forms) may be restructured, never re-rounded: every reduction keeps its order and every
term its arithmetic.  Every row of the gauss, KL, objective and mean-field KL tables of
tests/test_svgp_reduction_cases_cpu.py, in both dtypes, is held to the sha256 digests of its outputs recorded on the commit
before the terms were gathered into shared device functions (tests/golden/objective_hashes.json, written by
tools/record_objective_hashes.py, which refuses to record results that miss the tolerances of test_gpu_svgp_reductions.py
and test_gpu_meanfield.py against float64, or that touched a guard word: the record is of right answers)."""
import importlib.util
import json
import os

import pytest
import torch

from test_svgp_reduction_cases_cpu import OBJECTIVE_BITS_CASES, objective_bits_id

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'objective_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_objective_hashes', os.path.join(ROOT, 'tools', 'record_objective_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('run', OBJECTIVE_BITS_CASES, ids=objective_bits_id)
def test_objective_outputs_are_bit_identical_to_the_record(run, record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    digests, out = REC.run_case(run)
    assert out['guards'], 'a guard word next to an output or a workspace was overwritten'
    ref = record[objective_bits_id(run)]
    diff = sorted(name for name in set(ref) | set(digests) if ref.get(name) != digests.get(name))
    assert not diff, f'{objective_bits_id(run)}: {diff} differ from the record'
