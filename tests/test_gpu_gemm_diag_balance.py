"""The float32 GEMM wave schedule on the GPU: block maps and per-block MFMA masks (csrc/gemm.hip, gemm_wave_sched), exactly.

Operands are small integers with NO zero inside the support (values in {1, 2, 3}, signs mixed, row r of the left operand
scaled by a small factor that differs between the 32-row blocks of a tile), the ignored triangles hold large finite junk,
and the output sits between guard words.  Every product, partial sum and final value is then an integer (or a half-integer)
below 2^24, so float32 holds it exactly whatever the summation order, and the result must EQUAL the float64 dense formula: a
block that is wrongly skipped, run on the wrong K-tiles or stored at another block's rows changes it.

Shapes are the smallest that reach each path (asserted through nsgp_gemm_plan): 128 x 128 single-pass with two and three tile
rows (plain, masked and diagonal stretches), 128 x 64, lower-only outputs split and unsplit, and a ragged neighbour of each
(interior workgroups of the variant with bounds code).
"""
import ctypes
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

AL, AU, CL, NS = 1, 2, 16, 32
JUNK = 3.0e30
GUARD = -7.0e7
PAD = 64                                  # guard words on either side of the output (a multiple of 4: alignment is kept)

# (batch, M, n): projections  A_tri (M x M) @ X (M x n)
PROJ = [((1, 256, 38400), (128, 128), 1), ((1, 384, 38400), (128, 128), 1), ((1, 250, 38500), (128, 128), 0),
        ((1, 256, 16384), (128, 64), 1), ((1, 250, 16400), (128, 64), 0)]
# (batch, M, n): lower-only products  tril(A (M x n) @ C (M x n)^T)
LOWER = [((2, 256, 16384), 1, 1), ((2, 250, 16400), 0, 1), ((1, 2944, 256), 1, 0), ((1, 2940, 250), 0, 0),
         ((1, 384, 16384), 1, 1), ((1, 380, 16400), 0, 1)]
# (the float64 copy comes out of the split-K reduce only: no unsplit gemm_out64 case)
LOWER_CASES = [(f, *c) for f in ('gemm', 'gemm_out64', 'lqbar', 'lqbar_acc') for c in LOWER if f != 'gemm_out64' or c[2]]


def _ints(gen, *shape):
    """+-{1, 2, 3} on the device, seeded"""
    v = torch.randint(1, 4, shape, generator=gen, device='cuda').float()
    return torch.where(torch.rand(shape, generator=gen, device='cuda') < 0.5, -v, v)


def _gen(*key):
    return torch.Generator(device='cuda').manual_seed(zlib.crc32(repr(key).encode()))


def _guarded(shape, fill=float('nan')):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), GUARD, dtype=torch.float32, device='cuda')
    out = buf[PAD:PAD + n].view(*shape)
    out.fill_(fill)
    return buf, out


def _guards_intact(buf):
    return bool((buf[:PAD] == GUARD).all() and (buf[-PAD:] == GUARD).all())


def _plan(M, N, K, batch, flags, va, vb, ma, mb):
    import nsgp
    buf = (ctypes.c_int32 * 11)()
    assert nsgp.load_library().nsgp_gemm_plan(M, N, K, batch, 1, 4, flags, va, vb, ma, mb, ctypes.cast(buf, ctypes.c_void_p)) == 0
    return tuple(buf)


def _tri_operand(gen, b, M, factor):
    """Lower-triangular integers, row r scaled by factor(r); the strict upper triangle is junk on the device copy."""
    L = torch.tril(_ints(gen, b, M, M) * factor(torch.arange(M, device='cuda')).float()[None, :, None])
    Ld = L.clone()
    Ld[:, torch.triu(torch.ones(M, M, dtype=torch.bool, device='cuda'), 1)] = JUNK
    return L, Ld


def _block_factor(mod):
    return lambda r: 1 + r % mod


@pytest.mark.parametrize('shape,tile,whole', PROJ, ids=lambda v: str(v).replace(' ', ''))
@pytest.mark.parametrize('family', ['gemm_lower', 'gemm_upper', 'colstats', 'colstats_t', 'abar'])
def test_projection(family, shape, tile, whole):
    from nsgp import _lib, ops
    b, M, n = shape
    gen = _gen(family, shape)
    trans = family in ('gemm_upper', 'colstats_t')
    stats = family.startswith('colstats')
    # column statistics: sum_r Y[r, c]^2 over a tile's 128 rows has to stay below 2^24 as well -- factors 1 and 2 per block
    L, Ld = _tri_operand(gen, b, M, (lambda r: 1 + (r // 32) % 2) if stats else _block_factor(128))
    Xd = _ints(gen, b, M, n)
    op = (L.transpose(-1, -2) if trans else L).double()
    Yref = op @ Xd.double()
    assert float(Yref.abs().max()) < 2 ** 24
    flags = (AU if trans else AL) | (0 if family.startswith('gemm') else NS)
    vec_b = int(n % 4 == 0)
    plan = _plan(M, n, M, b, flags, int(M % 4 == 0), vec_b, int(trans), 1)
    assert plan[:2] == tile and plan[2] == 1 and plan[4] == whole, plan
    buf, Y = _guarded((b, M, n))
    st = ops._stream()
    if family.startswith('gemm'):
        ops.gemm(Ld, Xd, ta=trans, flags=flags, out=Y)
    elif stats:
        rvd = _ints(gen, b, M)
        T = int(_lib.load().nsgp_svgp_colstats_tiles(M, n, b, 4))
        assert T == -(-M // 128)
        pbuf0, p0 = _guarded((b, T, n))
        pbuf1, p1 = _guarded((b, T, n))
        _lib.call('nsgp_svgp_tri_gemm_colstats_f32', ops._p(Ld), int(trans), ops._p(Xd), ops._p(rvd), b, M, n, ops._p(Y),
                  ops._p(p0), ops._p(p1), st)
        pad = T * 128 - M
        Yp = torch.nn.functional.pad(Yref, (0, 0, 0, pad)).view(b, T, 128, n)
        rvp = torch.nn.functional.pad(rvd.double(), (0, pad)).view(b, T, 128, 1)
        r0, r1 = (Yp * rvp).sum(2), (Yp * Yp).sum(2)
        assert float((Yp * rvp).abs().sum(2).max()) < 2 ** 24 and float(r1.max()) < 2 ** 24      # exact in any order
        assert torch.equal(p0.double(), r0) and torch.equal(p1.double(), r1)
        assert _guards_intact(pbuf0) and _guards_intact(pbuf1)
    else:
        C, A = Xd, _ints(gen, b, M, n)
        m, gm, gv = _ints(gen, b, M), _ints(gen, b, n), _ints(gen, b, n)
        _lib.call('nsgp_svgp_abar_f32', ops._p(Ld), ops._p(C), ops._p(A), ops._p(m), ops._p(gm), ops._p(gv), b, M, n, ops._p(Y), st)
        d = lambda t: t.double()                                                          # noqa: E731
        Yref = 2 * Yref * d(gv)[:, None, :] + d(m)[:, :, None] * d(gm)[:, None, :] - 2 * d(A) * d(gv)[:, None, :]
        assert float(Yref.abs().max()) < 2 ** 24
    torch.cuda.synchronize()
    assert torch.equal(Y.double(), Yref), (Y.double() - Yref).abs().max()
    assert _guards_intact(buf)


@pytest.mark.parametrize('family,shape,whole,split', LOWER_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_lower_only_output(family, shape, whole, split):
    from nsgp import _lib, ops
    b, M, n = shape
    gen = _gen(family, shape)
    # |A| <= 3 * 27, |C| <= 3, |2 gv| <= 4, n <= 16400: every partial sum below 2^24
    Ad = _ints(gen, b, M, n) * _block_factor(27)(torch.arange(M, device='cuda')).float()[None, :, None]
    Cd = _ints(gen, b, M, n)
    v = int(n % 4 == 0)
    plan = _plan(M, M, n, b, CL, v, v, 0, 0)
    assert plan[:2] == (128, 128) and int(plan[2] > 1) == split and plan[4] == whole, plan
    lower = torch.tril(torch.ones(M, M, dtype=torch.bool, device='cuda'))
    buf, out = _guarded((b, M, M))
    if family.startswith('gemm'):
        ref = torch.tril(Ad.double() @ Cd.double().transpose(-1, -2))
        assert float(ref.abs().max()) < 2 ** 24
        if family == 'gemm_out64':
            o64 = torch.full((b, M, M), float('nan'), dtype=torch.float64, device='cuda')
            ops.gemm(Ad, Cd, tb=True, flags=CL, out=out, out64=o64)
            assert torch.equal(o64, ref)
        else:
            ops.gemm(Ad, Cd, tb=True, flags=CL, out=out)
    else:
        gv = _ints(gen, b, n).clamp(-2, 2)
        ref = torch.tril(torch.einsum('bkj,bj,blj->bkl', Ad.double(), 2 * gv.double(), Cd.double()))
        assert float(torch.einsum('bkj,bj,blj->bkl', Ad.double().abs(), 2 * gv.double().abs(), Cd.double().abs()).max()) < 2 ** 24
        wsb = int(_lib.load().nsgp_svgp_lqbar_workspace(b, M, n, 4))
        assert int(wsb > 0) == split
        ws = ops._ws(wsb, 'cuda')
        beta = ()
        if family == 'lqbar_acc':
            L0 = _ints(gen, b, M, M)
            out.copy_(L0)
            beta = (-0.5,)
            ref = torch.where(lower, ref - 0.5 * L0.double(), L0.double())     # the strict upper triangle keeps what it held
        _lib.call(f'nsgp_svgp_{family}_f32', ops._p(Ad), ops._p(Cd), ops._p(gv), b, M, n, *beta, ops._p(out), ops._p(ws), wsb,
                  ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(out.double(), ref), (out.double() - ref).abs().max()
    assert _guards_intact(buf)
