"""The SVGP forward projection launches what it launched before its host code was reorganised.

tests/golden/projection_launches.json: entry point and every non-pointer argument of every launch of one forward call, per
case (direct calls of ops.svgp_project / svgp_project_bf16 in all their forms, and svgp.svgp_marginal under every combination
of the settings that select an arithmetic), recorded by tools/record_projection_launches.py at commit b04fea4.  The replay
must give the recorded list exactly: same kernels, same order, same sizes, tile rows and flags, same null pointers."""
import json

import pytest
import torch

from test_projection_plan import RECORD, recorder

pytestmark = pytest.mark.gpu


def test_replay_gives_the_recorded_launches():
    R = recorder()
    with open(RECORD) as f:
        want = R.unpack(json.load(f))
    got, _ = R.record()
    assert sorted(got) == sorted(want)
    bad = [k for k in want if json.loads(json.dumps(got[k])) != want[k]]
    assert not bad, f'{len(bad)} of {len(want)} cases differ, e.g. {bad[0]}: {got[bad[0]]} != {want[bad[0]]}'


def _operands(b=2, M=64, n=96, D=2):
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).cuda()                       # noqa: E731
    W64 = torch.tril(r(b, M, M)).double()
    return dict(W=W64.float(), W64=W64, Kzx=r(b, M, n), Lq=torch.tril(r(b, M, M)), m=r(b, M), os=r(b).abs() + 1,
                Z=r(b, M, D), x=r(n, D), ls=r(b, D).abs() + 1)


@pytest.mark.parametrize('which', ['ls', 'os', 'x', 'Z'])
def test_malformed_kernel_inputs_are_an_error_not_a_launch(which):
    """(Z, x, ls, os) with one tensor of the wrong shape: BackendError from every entry point that takes the tuple
    (svgp_project_bf16 used to hand it to its kernels unchecked)."""
    from nsgp import BackendError, ops
    t = _operands()
    kin = dict(Z=t['Z'], x=t['x'], ls=t['ls'], os=t['os'])
    kin[which] = {'ls': t['ls'][:, :1], 'os': t['os'][:1], 'x': t['x'][:, :1], 'Z': t['Z'][:1]}[which].contiguous()
    kin = (kin['Z'], kin['x'], kin['ls'], kin['os'])
    a = (t['W'], t['Kzx'], t['Lq'], t['m'], t['os'])
    nok = (t['W'], None, t['Lq'], t['m'], t['os'])
    with pytest.raises(BackendError):
        ops.svgp_project_bf16(*a, kernel_inputs=kin)
    with pytest.raises(BackendError):
        ops.svgp_project_bf16(*nok, W64f=t['W64'], i8_inputs=kin)
    with pytest.raises(BackendError):
        ops.svgp_project(*nok, W64f=t['W64'], i8_inputs=kin)
    with pytest.raises(BackendError):
        ops.svgp_project(*nok, W64f=t['W64'], kernel_inputs=kin)
    torch.cuda.synchronize()


def test_kernel_inputs_of_another_size_than_kzx_are_an_error():
    from nsgp import BackendError, ops
    t = _operands()
    with pytest.raises(BackendError, match='shapes'):
        ops.svgp_project_bf16(t['W'], t['Kzx'], t['Lq'], t['m'], t['os'],
                              kernel_inputs=(t['Z'], t['x'][:-8].contiguous(), t['ls'], t['os']))
