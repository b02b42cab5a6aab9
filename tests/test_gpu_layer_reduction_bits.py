"""The SVGP layer's reductions (the layer half of csrc/svgp.hip: column statistics and their finalize forms, the row dots of
the adjoint, sampling, the mean-field diag_* kernels) may be restructured, never re-rounded: every reduction keeps its order
and every term its arithmetic.  Every row of the rowdot, colstats, finalize, sample and DIAG tables of
tests/test_svgp_reduction_cases_cpu.py, on seeded real values and in both dtypes, is held to the sha256 digests of its outputs
recorded on the commit before the pieces were gathered into shared device functions
(tests/golden/layer_reduction_hashes.json, written by tools/record_layer_reduction_hashes.py, which refuses to record
results that miss `red_tol` against float64 or that touched a guard word: the record is of right answers)."""
import importlib.util
import json
import os

import pytest
import torch

from test_svgp_reduction_cases_cpu import LAYER_BITS_CASES, layer_bits_id

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'layer_reduction_hashes.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_layer_reduction_hashes',
                                                  os.path.join(ROOT, 'tools', 'record_layer_reduction_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('run', LAYER_BITS_CASES, ids=layer_bits_id)
def test_layer_reduction_outputs_are_bit_identical_to_the_record(run, record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    digests, out = REC.run_case(run)
    assert out['guards'], 'a guard word next to an output or a workspace was overwritten'
    ref = record[layer_bits_id(run)]
    diff = sorted(name for name in set(ref) | set(digests) if ref.get(name) != digests.get(name))
    assert not diff, f'{layer_bits_id(run)}: {diff} differ from the record'
