"""The split-K reduce of csrc/gemm.hip may be made faster, never re-rounded: per element it stays
`s = 0; s += slab[0]; ...; s += slab[ks - 1]; s *= alpha; (halved diagonal) s *= 0.5; (beta != 0) s += beta * c`, on the
vector kernel and on the scalar one, and it writes exactly the elements it wrote before.  Every row of
tests/splitk_reduce_cases.py is held to the sha256 digest of its whole guarded output buffer recorded on the commit before
the vector kernel existed (tests/golden/splitk_reduce_hashes.json, written by tools/record_splitk_reduce_hashes.py, which
refuses results that miss the summation bound against the float64 product or touch a guard word).

The float64 copy of a float32 product (nsgp_gemm_f32_out64): bit-equal to the widened float32 result on every element the
reduce writes, guard words everywhere else, refused where the product is not split; and at the layer level the float64 Wbar
buffer and the Kzz adjoint of the whitening chain are bit-equal with the copy coming from the reduce or from the cast."""
import ctypes
import importlib.util
import json
import os

import pytest
import torch

import splitk_reduce_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'splitk_reduce_hashes.json')
OUT64_UNSPLIT = -64            # NSGP_GEMM_OUT64_UNSPLIT (include/nsgp.h)


def _recorder():
    spec = importlib.util.spec_from_file_location('record_splitk_reduce_hashes',
                                                  os.path.join(ROOT, 'tools', 'record_splitk_reduce_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()
F32_CASES = [c for c in SC.CASES if c.dt == 'f32']


@pytest.fixture(scope='module')
def record():
    with open(RECORD) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('case', SC.CASES, ids=SC.case_id)
def test_split_products_are_bit_identical_to_the_record(case, record):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    digests, extras = REC.run_case(case)
    why = REC.check(case, extras)                             # guard words, the zeros, the float64 reference
    assert not why, f'{SC.case_id(case)}: {why}'
    assert digests == record[SC.case_id(case)], f'{SC.case_id(case)}: differs from the record'


@pytest.mark.parametrize('case', F32_CASES, ids=SC.case_id)
def test_float64_copy_is_the_widened_result_and_nothing_else(case):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import _lib
    lib = _lib.load()
    A, B, C0 = REC.operands(case)
    _, _, total = SC.layout(case)
    idx = REC.matrix_index(case)
    buf = torch.full((total,), REC.GUARD, dtype=torch.float32)
    buf[idx.reshape(-1)] = C0.reshape(-1)
    # the copy has a layout of its own: another row padding (odd on every other row of the table: element-wise stores) and gap
    pad64, gap64 = (2, 6) if F32_CASES.index(case) % 2 == 0 else (3, 5)
    ld64, stride64, total64 = SC.layout(case, pad64, gap64)
    idx64 = REC.matrix_index(case, pad64, gap64)
    buf, Ad, Bd = buf.cuda(), A.cuda(), B.cuda()
    buf64 = torch.full((total64,), REC.GUARD, dtype=torch.float64, device='cuda')
    args, ws = REC.gemm_args(case, Ad, Bd, buf)
    nb1, nb2 = SC.batch_levels(case)
    s1, s2 = (stride64, 0) if nb2 == 1 else (0, stride64)
    tail = (ctypes.c_void_p(buf64.data_ptr() + SC.GUARD_WORDS * 8), ld64, s1, s2)
    rc = lib.nsgp_gemm_f32_out64(*args, *tail)
    torch.cuda.synchronize()
    if REC.ksplit(case) == 1:
        assert rc == OUT64_UNSPLIT
        assert bool((buf64 == REC.GUARD).all()) and bool((buf.cpu()[idx].isnan()).all())      # nothing was launched
        return
    assert rc == 0
    assert REC.sha(buf) == REC.run_case(case)[0]['C']                                          # C as without the copy
    got, got64 = buf.cpu()[idx], buf64.cpu()
    r, col = torch.arange(case.M).view(-1, 1), torch.arange(case.M).view(1, -1)
    written = torch.ones(got.shape, dtype=torch.bool)
    if case.flags & SC.CL and not SC.zero_filled_upper(case):
        written = (col <= r).expand_as(got).clone()
    assert torch.equal(got64[idx64][written].view(torch.int64), got.double()[written].view(torch.int64))
    keep = torch.ones(total64, dtype=torch.bool)
    keep[idx64[written]] = False
    assert bool((got64[keep] == REC.GUARD).all()), 'the copy was written where the reduce does not write C'
    # bad arguments of the copy are named like the others'
    assert lib.nsgp_gemm_f32_out64(*args, None, ld64, s1, s2) == -26
    assert lib.nsgp_gemm_f32_out64(*args, tail[0], case.M - 1, s1, s2) == -27


def _layer_backward(fused):
    """One backward pass of a two-group whitening chain (hidden layer of two GPs, last layer of one; M = 128, n = 1024) under
    float32 layers: the float64 Wbar the Cholesky adjoint reads, the Kzz adjoint it returns, the casts to float64 it ran."""
    from nsgp import ops, svgp
    g = torch.Generator().manual_seed(20)
    M, n, D = 128, 1024, 2
    leaves, groups = [], []
    for b in (2, 1):
        Z = torch.randn(b, M, D, generator=g).cuda().requires_grad_()
        ls = (0.7 + 0.3 * torch.rand(b, D, generator=g)).cuda().requires_grad_()
        os_ = (0.8 + 0.4 * torch.rand(b, generator=g)).cuda().requires_grad_()
        m = (0.3 * torch.randn(b, M, generator=g)).cuda().requires_grad_()
        Lq = (torch.eye(M) + 0.05 * torch.tril(torch.randn(b, M, M, generator=g))).cuda().requires_grad_()
        groups.append((Z, ls, os_))
        leaves.append((m, Lq))
    x = torch.randn(n, D, generator=g).cuda()
    wm, wv = torch.randn(n, generator=g).cuda(), torch.rand(n, generator=g).cuda()
    seen = dict(wbar=None, kbar=None, casts=0)
    gemm, cast = ops.gemm, ops.cast

    def spy_gemm(A, B, *a, **kw):
        out = gemm(A, B, *a, **kw)
        fl = kw.get('flags', 0)
        if fl & ops.GEMM_C_HALFDIAG:
            seen['wbar'] = A.clone()                          # Phi = tril(Wbar W^T): its first operand
        if kw.get('alpha') == -1.0:
            seen['kbar'] = out.clone()
        return out

    def spy_cast(t, dtype, out=None):
        seen['casts'] += int(dtype == torch.float64 and out is not None)
        return cast(t, dtype, out=out)

    old = svgp._FUSE_WBAR64
    svgp._FUSE_WBAR64, ops.gemm, ops.cast = fused, spy_gemm, spy_cast
    try:
        Ws, _, passed, W64s = svgp.whiten(groups, passthrough=True, out_dtype=torch.float32, with_f64=True)
        loss = 0.0
        for (m, Lq), W, (Z, ls, os_), W64 in zip(leaves, Ws, passed, W64s):
            mean, var, _ = svgp.svgp_marginal(x, Z, ls, os_, m, Lq, W64=W, W64f=W64)
            loss = loss + (mean * wm).sum() + (var * wv).sum()
        loss.backward()
        torch.cuda.synchronize()
    finally:
        svgp._FUSE_WBAR64, ops.gemm, ops.cast = old, gemm, cast
    grads = [t.grad.clone() for grp in groups for t in grp]
    return seen, grads


def test_whitening_adjoint_is_bit_equal_with_the_copy_from_the_reduce_or_from_the_cast():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops
    plan = ops.gemm_plan(torch.empty(2, 128, 1024), torch.empty(2, 128, 1024), tb=True, flags=ops.GEMM_C_LOWER)
    assert plan.ksplit > 1                                    # the Wbar products of this shape are split: the copy is the reduce's
    on, g_on = _layer_backward(True)
    off, g_off = _layer_backward(False)
    assert on['wbar'] is not None and on['wbar'].dtype == torch.float64 and tuple(on['wbar'].shape) == (3, 128, 128)
    assert off['casts'] == 2 and on['casts'] == 0             # one cast launch per layer, none with the reduce's copy
    assert torch.equal(on['wbar'].view(torch.int64), off['wbar'].view(torch.int64))
    assert bool((torch.triu(on['wbar'], 1) == 0).all()) and bool(torch.isfinite(on['wbar']).all())
    assert torch.equal(on['kbar'].view(torch.int64), off['kbar'].view(torch.int64))
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)
