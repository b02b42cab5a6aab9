"""GPU parity of the mean-field variational family q(u) = N(m, diag(s^2)) against the float64 CPU oracle, which needs no
change: a layer dict with Lq = diag_embed(s), s = raw.abs().clamp_min(1e-8) a float64 leaf expression, IS the mean-field
layer.  Raw kernels against the dense formulas, the layer node, every first-product arithmetic, the KL nodes, the DSVI
objective end to end (all mean-field and mixed with a Cholesky layer), predict / full covariance, determinism, graph
capture and the non-positive-definite case.  Tolerances are those of the existing test of the same quantity for the
Cholesky layer, named at each assert."""
import os

import pytest
import torch

from conftest import measured
from test_gpu_dgp import DSVI_GRAD_TOL, _FixedEps
from test_gpu_i8 import I8_LAYER_GRAD_TOL, I8_LAYER_VALUE_TOL
from test_gpu_svgp import F32_GRAD_TOL, F32_VALUE_TOL

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
sp = torch.nn.functional.softplus


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _raw_stddev(shape, g):
    """Mixed signs, one entry at 1e-12: the clamp at 1e-8 is active there and the gradient is exactly zero."""
    raw = (0.5 + torch.rand(shape, generator=g, dtype=F64)) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    raw.reshape(-1)[raw.numel() // 2] = 1e-12
    return raw


def _s(raw):
    return raw.abs().clamp_min(1e-8)


def _rel(a, r):
    return float((a.detach().cpu().double() - r.detach()).abs().max() / (r.detach().abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------ 1: raw kernels
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('b,M,n', [(1, 1, 1), (2, 63, 65), (1, 33, 257), (1, 130, 700), (3, 256, 1000), (1, 1024, 4096)])
def test_mean_field_projection_ops_match_dense_formulas(dt, b, M, n):
    """svgp_project_diag / svgp_project_diag_bwd (diag_colsq, colstats_finalize_diag, diag_bwd behind SVGPMeanFieldLayerFn)
    against the dense float64 formulas, at the tile edges of test_fused_projection_ops_match_dense_formulas plus one."""
    from nsgp import ops
    g = _g(2000 + M + n)
    W = torch.tril(torch.randn(b, M, M, generator=g, dtype=F64)) / max(M, 1) ** 0.5
    K = torch.randn(b, M, n, generator=g, dtype=F64)
    m = torch.randn(b, M, generator=g, dtype=F64)
    base = torch.rand(b, generator=g, dtype=F64) + 0.5
    gm = torch.randn(b, n, generator=g, dtype=F64)
    gv = torch.randn(b, n, generator=g, dtype=F64)
    raw = _raw_stddev((b, M), g).requires_grad_()
    s2 = _s(raw) ** 2
    dev = lambda t: t.detach().to(dt).cuda()  # noqa: E731
    junk = torch.triu(torch.full((M, M), 7.0, dtype=F64), 1)              # the strict upper triangle of W is no operand
    s2m1 = dev(s2) - 1.0
    A, mean, var = ops.svgp_project_diag('f32', dev(W + junk), s2m1, dev(m), dev(base), Kzx=dev(K))
    A_ref = W @ K
    mean_ref = torch.einsum('bkj,bk->bj', A_ref, m)
    var_ref = base[:, None] + torch.einsum('bk,bkj->bj', s2.detach() - 1.0, A_ref ** 2)
    # tolerances of test_fused_projection_ops_match_dense_formulas
    tol = dict(rtol=1e-10, atol=1e-10) if dt == F64 else dict(rtol=2e-4, atol=2e-4 * max(1.0, M ** 0.5))
    assert measured(f'mean-field A {dt} b{b} M{M} n{n}', A, A_ref, **tol)
    assert measured(f'mean-field mean {dt} b{b} M{M} n{n}', mean, mean_ref, **tol)
    assert measured(f'mean-field var {dt} b{b} M{M} n{n}', var, var_ref, **tol)
    if dt == F32:
        # the same variance through the Cholesky layer's column statistics on C = s o A (two separately rounded sums)
        s = dev(_s(raw))
        _, var_c = ops.svgp_colstats(A, s.unsqueeze(-1) * A, dev(m), dev(base))
        A_ = A.cpu().double()                                             # both evaluated at the device's own A and s^2 - 1
        var_own = base[:, None].float().double() + torch.einsum('bk,bkj->bj', s2m1.cpu().double(), A_ ** 2)
        e_diag = float((var.cpu().double() - var_own).abs().max())
        e_chol = float((var_c.cpu().double() - var_own).abs().max())
        print(f'[measured] mean-field var error b{b} M{M} n{n}: one float64 sum {e_diag:.3g}, svgp_colstats on C = s o A {e_chol:.3g}')
        assert e_diag <= e_chol
    Abar, mbar, tbar, basebar, wbar, cbar = ops.svgp_project_diag_bwd(dev(m), s2m1, A, dev(gm), dev(gv))
    assert wbar is None and cbar is None
    A_ = A.cpu().double()                                                 # adjoints evaluated at the device's own A
    s2m1_ = s2m1.cpu().double()
    Abar_ref = m[:, :, None] * gm[:, None, :] + 2 * s2m1_[:, :, None] * A_ * gv[:, None, :]
    mbar_ref = torch.einsum('bkj,bj->bk', A_, gm)
    tbar_ref = torch.einsum('bkj,bj->bk', A_ ** 2, gv)
    tolb = dict(rtol=1e-9, atol=1e-9) if dt == F64 else dict(rtol=5e-4, atol=5e-4 * max(1.0, (n * 1.0) ** 0.5))
    assert measured('mean-field Abar', Abar, Abar_ref, **(tol if dt == F64 else tolb))
    assert measured('mean-field mbar', mbar, mbar_ref, **tolb)
    assert measured('mean-field s2bar', tbar, tbar_ref, **tolb)
    assert measured('mean-field basebar', basebar, gv.sum(-1), **tolb)
    # the raw parameter: plain autograd through s^2 = clamp(|raw|)^2 -- exactly zero where the clamp is active
    raw_dev = raw.detach().to(dt).cuda().requires_grad_()
    (raw_dev.abs().clamp_min(1e-8) ** 2 * tbar).sum().backward()
    (s2 * tbar_ref).sum().backward()
    assert measured('mean-field raw stddev grad', raw_dev.grad, raw.grad, **tolb)
    assert float(raw_dev.grad.reshape(-1)[raw.numel() // 2]) == 0.0 and float(raw.grad.reshape(-1)[raw.numel() // 2]) == 0.0


@pytest.mark.parametrize('dt', [F64, F32])
def test_mean_field_projection_with_an_affine_prior_mean(dt):
    """The affine prior mean through colstats_finalize_diag and its gradients through the rowdot launch that reads no row of
    A (tolerances of test_affine_prior_mean_is_folded_into_the_projection)."""
    from nsgp import ops
    b, M, n, D = 2, 40, 333, 3
    g = _g(77)
    W = torch.tril(torch.randn(b, M, M, generator=g, dtype=F64)) / M ** 0.5
    K, m = torch.randn(b, M, n, generator=g, dtype=F64), torch.randn(b, M, generator=g, dtype=F64)
    base = torch.rand(b, generator=g, dtype=F64) + 0.5
    x, w, c = torch.randn(n, D, generator=g, dtype=F64), torch.randn(1, D, generator=g, dtype=F64), torch.randn(1, generator=g, dtype=F64)
    gm, gv = torch.randn(b, n, generator=g, dtype=F64), torch.randn(b, n, generator=g, dtype=F64)
    s2m1 = _s(_raw_stddev((b, M), g)) ** 2 - 1.0
    dev = lambda t: t.to(dt).cuda()  # noqa: E731
    aff = (dev(x), dev(w), dev(c))
    A, mean, var = ops.svgp_project_diag('f32', dev(W), dev(s2m1), dev(m), dev(base), base_add=1e-4, affine=aff, Kzx=dev(K))
    A_ref = W @ K
    tol = dict(rtol=1e-10, atol=1e-10) if dt == F64 else dict(rtol=2e-4, atol=2e-4 * M ** 0.5)
    assert measured('mean-field affine mean', mean, torch.einsum('bkj,bk->bj', A_ref, m) + (x @ w[0])[None] + c, **tol)
    assert measured('mean-field affine var', var, base[:, None] + 1e-4 + torch.einsum('bk,bkj->bj', s2m1, A_ref ** 2), **tol)
    _, mbar, _, basebar, wbar, cbar = ops.svgp_project_diag_bwd(dev(m), dev(s2m1), A, dev(gm), dev(gv), affine=aff)
    tolb = dict(rtol=1e-9, atol=1e-9) if dt == F64 else dict(rtol=5e-4, atol=5e-4 * n ** 0.5)
    assert measured('mean-field affine mbar', mbar, torch.einsum('bkj,bj->bk', A.cpu().double(), gm), **tolb)
    assert measured('mean-field affine basebar', basebar, gv.sum(-1), **tolb)
    assert wbar.shape == (1, D) and cbar.shape == (1,)
    assert measured('mean-field affine wbar', wbar, torch.einsum('nd,bn->d', x, gm)[None], **tolb)
    assert measured('mean-field affine cbar', cbar, gm.sum().reshape(1), **tolb)


# ------------------------------------------------------------------------------------------ 2, 3: the layer
def _layer_params(b, M, D, n, seed, batched_x, spread=1.0):
    """test_gpu_svgp._params with a raw stddev in place of Lq; `spread` scales Z and x (see SPREAD)."""
    g = _g(seed)
    Z = spread * torch.randn(b, M, D, generator=g, dtype=F64)
    ls = torch.rand(b, D, generator=g, dtype=F64) + 0.7
    os_ = torch.rand(b, generator=g, dtype=F64) + 0.5
    m = 0.3 * torch.randn(b, M, generator=g, dtype=F64)
    raw = _raw_stddev((b, M), g)
    x = spread * torch.randn((b, n, D) if batched_x else (n, D), generator=g, dtype=F64)
    gm = torch.randn(b, n, generator=g, dtype=F64)
    gv = torch.randn(b, n, generator=g, dtype=F64)
    return (x, Z, ls, os_, m, raw), gm, gv


_ORACLE = {}


def _layer_oracle(b, M, D, n, seed, batched_x, jitter=1e-4, spread=1.0):
    """mean, var and the gradients of (x, Z, ls, os, m, raw_stddev) from the oracle; computed once per case and shared."""
    key = (b, M, D, n, seed, batched_x, jitter, spread)
    if key not in _ORACLE:
        from oracle import svgp
        leaves, gm, gv = _layer_params(b, M, D, n, seed, batched_x, spread)
        ins = [t.clone().requires_grad_() for t in leaves]
        xo, Zo, lso, oso, mo, rawo = ins
        xin = xo if xo.dim() == 3 else xo.unsqueeze(0).expand(b, *xo.shape)
        p = dict(Z=Zo, lengthscale=lso.unsqueeze(-2), outputscale=oso, m=mo, Lq=torch.diag_embed(_s(rawo)),
                 mean=('constant', torch.zeros(b, 1, dtype=F64)))
        mean, var = svgp.svgp_marginal(xin, p, jitter=jitter)
        ((mean * gm).sum() + (var * gv).sum()).backward()
        _ORACLE[key] = (mean.detach(), var.detach(), [t.grad for t in ins])
    return _ORACLE[key]


def _layer_device(b, M, D, n, seed, batched_x, dt, kzx_f64=False, spread=1.0):
    from nsgp.svgp import svgp_marginal
    leaves, gm, gv = _layer_params(b, M, D, n, seed, batched_x, spread)
    cu = [t.to(dt).cuda().requires_grad_() for t in leaves]
    x, Z, ls, os_, m, raw = cu
    mean, var, info = svgp_marginal(x, Z, ls, os_, m, s2=raw.abs().clamp_min(1e-8) ** 2, jitter=1e-4, kzx_f64=kzx_f64)
    ((mean * gm.to(dt).cuda()).sum() + (var * gv.to(dt).cuda()).sum()).backward()
    return mean.detach(), var.detach(), [t.grad for t in cu], info


NAMES = ('x', 'Z', 'ls', 'os', 'm', 'raw_stddev')


@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('b,M,D,n,batched_x', [(2, 50, 3, 315, False), (1, 130, 2, 400, True), (2, 64, 2, 96, True)])
def test_mean_field_layer_matches_oracle(dt, b, M, D, n, batched_x):
    """test_svgp_layer_matches_oracle with q(u) = N(m, diag(s^2)): its shapes, its tolerances."""
    mean_r, var_r, grads_r = _layer_oracle(b, M, D, n, 40 + M, batched_x)
    mean, var, grads, info = _layer_device(b, M, D, n, 40 + M, batched_x, dt)
    assert info.cpu().tolist() == [0] * b
    tol = dict(rtol=1e-9, atol=1e-10) if dt == F64 else F32_VALUE_TOL
    assert measured(f'mean-field layer mean {dt} b{b} M{M}', mean, mean_r, **tol)
    assert measured(f'mean-field layer var {dt} b{b} M{M}', var, var_r, **tol)
    for name, got, ref in zip(NAMES, grads, grads_r):
        err = _rel(got, ref)
        print(f'[measured] mean-field layer grad {name} {dt} b{b} M{M}: max-norm rel err {err:.3g}')
        assert err < (1e-7 if dt == F64 else F32_GRAD_TOL), (name, err)
    k = (b * M) // 2
    assert float(grads[5].reshape(-1)[k]) == 0.0 and float(grads_r[5].reshape(-1)[k]) == 0.0      # the clamped entry


# Inputs of the arithmetic cases: Z and x drawn 3x wider than test_gpu_svgp.py's N(0, 1).  F32_VALUE_TOL (atol 3e-5) is stated
# there for well-conditioned small layers, and one of the arithmetics here -- whiten_matmul_f64 off -- accumulates A = W Kzx in
# float32, whose error on the mean has the scale u sum_k |m_k| (|W||Kzx|)_kj, u = 2^-24.  With unit spread that scale is
# 1.5e-4 / 3.6e-4 / 2.1e-4 at the three shapes below (kappa(Kzz) 4e5 - 7e5, |W||Kzx| up to 400): no float32 accumulation can be
# held to 3e-5 there, whatever the kernel (measured: 4.2e-5 and 8.6e-5).  At spread 3 it is 1.9e-5 / 8.6e-6 / 7.0e-6 (kappa
# 1e4 - 1e5), inside the bound, so the bound tests the kernels and not the conditioning.  Computed from the inputs alone, in
# float64 on the host; every arithmetic gets the same inputs.
SPREAD = 3.0
SMALL = [(2, 64, 96, 2), (1, 130, 333, 3)]
ARITH = [
    # id, settings, kzx_f64, shapes (b, M, n, D), 'i8' / 'f32': whose tolerances hold
    ('i8', dict(whiten_matmul_i8=True), False, SMALL, 'i8'),
    ('f64acc', dict(whiten_matmul_i8=False), False, SMALL, 'f32'),
    ('f32', dict(whiten_matmul_i8=False, whiten_matmul_f64=False), False, SMALL, 'f32'),
    ('kzx_fused', dict(fuse_kzx=True), False, SMALL + [(1, 128, 128, 2)], 'f32'),
    ('i8 5 planes', dict(whiten_matmul_i8=True), True, SMALL, 'i8'),
    ('f64acc_b64', dict(whiten_matmul_i8=False), True, SMALL, 'f32'),
    ('bf16', dict(forward_precision='bf16'), False, [(2, 64, 96, 2), (1, 128, 128, 2)], 'i8'),
]
ARITH_CASES = [(a[0], a[1], a[2], shp, a[4]) for a in ARITH for shp in a[3]]


@pytest.mark.parametrize('name,flags,kzx_f64,shape,tols', ARITH_CASES, ids=[f'{c[0]}-{c[3]}' for c in ARITH_CASES])
def test_mean_field_layer_in_every_first_product_arithmetic(name, flags, kzx_f64, shape, tols):
    """The float32 layer with A = W Kzx in every arithmetic select_projection can name, against the oracle at the tolerance
    the existing test of that arithmetic applies to the Cholesky layer: test_gpu_i8.py's I8_LAYER_VALUE_TOL / I8_LAYER_GRAD_TOL
    (max-norm relative) for the int8 product, test_gpu_svgp.py's F32_VALUE_TOL / F32_GRAD_TOL for the others; the
    generated-Kzx product also equals the materialised one bit for bit, as in test_gpu_svgp.py.

    The inputs are those SPREAD describes."""
    import contextlib
    from nsgp import svgp
    from nsgp.gp import settings
    b, M, n, D = shape
    with contextlib.ExitStack() as st:
        for k, v in flags.items():
            st.enter_context(getattr(settings, k)(v))
        seen = []
        orig = svgp.ops.svgp_project_diag
        svgp.ops.svgp_project_diag = lambda first, *a, **kw: (seen.append((first, kw.get('i8_planes'))), orig(first, *a, **kw))[1]
        try:
            mean, var, grads, info = _layer_device(b, M, D, n, 300 + M, False, F32, kzx_f64=kzx_f64, spread=SPREAD)
        finally:
            svgp.ops.svgp_project_diag = orig
    want = {'i8 5 planes': 'i8', 'bf16': 'i8'}.get(name, name)
    if name == 'kzx_fused' and (M, n) != (128, 128):
        assert seen[0][0] in ('kzx_fused', 'i8'), seen                    # not whole tiles: the layer keeps the int8 product
        want = seen[0][0]
    assert seen[0][0] == want and (want != 'i8' or seen[0][1] == (5 if kzx_f64 else 4)), (name, seen)
    assert info.cpu().tolist() == [0] * b
    mean_r, var_r, grads_r = _layer_oracle(b, M, D, n, 300 + M, False, spread=SPREAD)
    errs = {nm: _rel(got, ref) for nm, got, ref in zip(NAMES, grads, grads_r)}
    print(f'[measured] mean-field layer {name} b{b} M{M} n{n} grads:', {k: '%.3g' % v for k, v in errs.items()})
    if want == 'i8':
        ev, em = _rel(var, var_r), _rel(mean, mean_r)
        print(f'[measured] mean-field layer {name} b{b} M{M} n{n}: mean {em:.3g} var {ev:.3g} (max-norm relative)')
        assert em < I8_LAYER_VALUE_TOL and ev < I8_LAYER_VALUE_TOL, (name, em, ev)
        assert max(errs.values()) < I8_LAYER_GRAD_TOL, (name, errs)
    else:
        ok_mean = measured(f'mean-field layer {name} mean b{b} M{M} n{n}', mean, mean_r, **F32_VALUE_TOL)
        ok_var = measured(f'mean-field layer {name} var b{b} M{M} n{n}', var, var_r, **F32_VALUE_TOL)
        assert ok_mean and ok_var, (name, shape)
        assert max(errs.values()) < F32_GRAD_TOL, (name, errs)
    if want == 'kzx_fused':             # test_layer_with_generated_kzx_matches_the_materialised_layer: bit for bit
        with settings.fuse_kzx(False), settings.whiten_matmul_i8(False):
            mat = _layer_device(b, M, D, n, 300 + M, False, F32, spread=SPREAD)
        for a, c in zip([mean, var] + grads, [mat[0], mat[1]] + mat[2]):
            assert torch.equal(a, c)


def test_mean_field_layer_mean_is_the_cholesky_layers_mean_bit_for_bit():
    """The mean A^T m (+ prior mean) keeps coming from the first product's partials exactly as in the Cholesky layer: same
    inputs, same bits, in the default and in the plain float32 arithmetic."""
    from nsgp.gp import settings
    from nsgp.svgp import svgp_marginal
    for b, M, n, D in SMALL:
        (x, Z, ls, os_, m, raw), _, _ = _layer_params(b, M, D, n, 300 + M, False, SPREAD)
        x, Z, ls, os_, m, raw = (t.float().cuda() for t in (x, Z, ls, os_, m, raw))
        for f64 in (True, False):
            with settings.whiten_matmul_f64(f64):
                mean_d, _, _ = svgp_marginal(x, Z, ls, os_, m, s2=raw.abs().clamp_min(1e-8) ** 2)
                mean_c, _, _ = svgp_marginal(x, Z, ls, os_, m, torch.diag_embed(raw.abs().clamp_min(1e-8)))
            assert torch.equal(mean_d, mean_c), (b, M, n, D, f64)


def test_mean_field_layer_under_bf16_is_the_f32_layer_and_bf16_all_is_finite():
    """forward_precision('bf16') moves C = Lq^T A to the bf16 cores; a mean-field layer has no C, so its result is that of
    'f32' bit for bit.  'bf16_all' (A on the bf16 cores) is a throughput mode whose existing test asks for finite results
    (test_bf16_forward_at_the_cfg5_shape_states_its_error) and bounds A by 2e-2 of its size at kernel level."""
    from nsgp.gp import settings
    for b, M, n, D in [(2, 64, 96, 2), (1, 128, 128, 2)]:
        res = {}
        for fp in ('f32', 'bf16', 'bf16_all'):
            with settings.forward_precision(fp):
                res[fp] = _layer_device(b, M, D, n, 300 + M, False, F32, spread=SPREAD)
        for a, c in zip([res['f32'][0], res['f32'][1]] + res['f32'][2], [res['bf16'][0], res['bf16'][1]] + res['bf16'][2]):
            assert torch.equal(a, c)
        mean_r, var_r, _ = _layer_oracle(b, M, D, n, 300 + M, False, spread=SPREAD)
        mean, var, grads, _ = res['bf16_all']
        print(f'[measured] mean-field layer bf16_all b{b} M{M}: mean {_rel(mean, mean_r):.3g} var {_rel(var, var_r):.3g}')
        assert all(bool(torch.isfinite(t).all()) for t in [mean, var] + grads)


# ------------------------------------------------------------------------------------------ 4: KL
@pytest.mark.parametrize('dt', [F64, F32])
@pytest.mark.parametrize('b', [1, 3])
@pytest.mark.parametrize('M', [1, 63, 257, 1024])
def test_mean_field_kl_matches_oracle_and_accumulates(dt, b, M):
    """KlMeanFieldFn / KlMeanFieldTotalFn against oracle.svgp.kl_whitened (value and gradients); tolerance of
    test_fused_dsvi_objective_equals_the_chain_of_per_term_kernels -- float32: the terms (s2 - 1) - log s2 + m^2 are
    non-negative and each good to a few ulp, so a sum of b M <= 3072 of them is good to ~1e-6 relative, and a gradient
    (1 - 1 / s2) / 2 to an absolute 1e-7; float64: 1e-12.  Adding into a running scalar adds exactly that scalar."""
    from nsgp import ops
    from oracle import svgp
    g = _g(500 + M + b)
    m = torch.randn(b, M, generator=g, dtype=F64).requires_grad_()
    raw = _raw_stddev((b, M), g)
    raw.reshape(-1)[raw.numel() // 2] = -0.3                              # (log of the clamped 1e-16 variance is not the point here)
    raw.requires_grad_()
    ref = svgp.kl_whitened(dict(m=m, Lq=torch.diag_embed(_s(raw))))
    (1.7 * ref).backward()
    md, rd = m.detach().to(dt).cuda().requires_grad_(), raw.detach().to(dt).cuda().requires_grad_()
    kl = ops.KlMeanFieldFn.apply(md, rd.abs().clamp_min(1e-8) ** 2)
    (1.7 * kl).backward()
    tol = dict(rtol=2e-5, atol=1e-6) if dt == F32 else dict(rtol=1e-12, atol=1e-13)
    assert kl.shape == () and measured(f'mean-field KL {dt} b{b} M{M}', kl, ref, **tol)
    assert measured('mean-field KL grad m', md.grad, m.grad, **tol)
    assert measured('mean-field KL grad raw stddev', rd.grad, raw.grad, **tol)
    # scaled, added into a running device scalar, upstream gradient on the device
    m2, r2 = md.detach().clone().requires_grad_(), rd.detach().clone().requires_grad_()
    run = torch.tensor(3.25, dtype=dt, device='cuda', requires_grad=True)
    s2 = r2.abs().clamp_min(1e-8) ** 2
    alone = ops.KlMeanFieldTotalFn.apply(m2, s2, -0.011)
    tot = ops.KlMeanFieldTotalFn.apply(m2, s2, -0.011, run)
    assert torch.equal(tot.detach(), run.detach() + alone.detach())
    assert measured('mean-field KL total', alone, -0.011 * ref, **tol)
    (2.0 * tot).backward()
    assert float(run.grad) == 2.0
    assert measured('mean-field KL total grad m', m2.grad, -0.011 * 2.0 / 1.7 * m.grad, **tol)
    assert measured('mean-field KL total grad raw stddev', r2.grad, -0.011 * 2.0 / 1.7 * raw.grad, **tol)


# ------------------------------------------------------------------------------------------ 5: end to end
def _build(num_layers, D, M, seed, hidden='mean_field', last='mean_field'):
    """test_gpu_dgp._build with a choice of variational family per layer."""
    import models.dgps as m
    torch.manual_seed(seed)
    model = m.DeepGP(num_layers, (1000, D), num_inducing=M, variational=last)
    if hidden != last:
        layer = m.DeepGPHiddenLayer(D, m.num_output_dims, M, 'linear', variational=hidden)
        model.layers = torch.nn.ModuleList([layer for _ in range(num_layers)])
    model = model.cuda()
    g = _g(seed + 1)
    with torch.no_grad():
        for mod in (model.layers[0], model.last_layer):
            vd = mod.variational_strategy._variational_distribution
            vd.variational_mean.copy_(0.3 * torch.randn(vd.variational_mean.shape, generator=g))
            if hasattr(vd, '_variational_stddev'):
                vd._variational_stddev.copy_(_raw_stddev(vd._variational_stddev.shape, g))
            else:
                vd.chol_variational_covar.copy_(torch.tril(0.1 * torch.randn(vd.chol_variational_covar.shape, generator=g))
                                                + torch.eye(M))
            mod.variational_strategy.variational_params_initialized.fill_(1)
            mod.covar_module.base_kernel.raw_lengthscale.add_(0.3 * torch.randn(
                mod.covar_module.base_kernel.raw_lengthscale.shape, generator=g).cuda())
    return model


def _oracle_layers(model):
    """Float64 CPU leaves of the raw parameters and the oracle's layer dicts; a mean-field layer's Lq is diag_embed(s)."""
    leaves = {}

    def leaf(name, t):
        leaves[name] = t.detach().cpu().double().clone().requires_grad_()
        return leaves[name]

    def layer(prefix, mod, linear):
        vs = mod.variational_strategy
        vd = vs._variational_distribution
        p = dict(Z=leaf(prefix + 'Z', vs.inducing_points),
                 lengthscale=sp(leaf(prefix + 'raw_ls', mod.covar_module.base_kernel.raw_lengthscale)),
                 outputscale=sp(leaf(prefix + 'raw_os', mod.covar_module.raw_outputscale)),
                 m=leaf(prefix + 'm', vd.variational_mean))
        if hasattr(vd, '_variational_stddev'):
            p['Lq'] = torch.diag_embed(_s(leaf(prefix + 'raw_stddev', vd._variational_stddev)))
        else:
            p['Lq'] = leaf(prefix + 'Lq', vd.chol_variational_covar)
        if linear:
            p['mean'] = ('linear', leaf(prefix + 'w', mod.mean_module.weights), leaf(prefix + 'b', mod.mean_module.bias))
        else:
            p['mean'] = ('constant', leaf(prefix + 'c', mod.mean_module.constant))
        return p
    hidden = layer('h.', model.layers[0], True)
    last = layer('l.', model.last_layer, False)
    noise = sp(leaf('raw_noise', model.likelihood.noise_covar.raw_noise)) + 1e-4
    return hidden, last, noise, leaves


def _model_params(model):
    out = {'raw_noise': model.likelihood.noise_covar.raw_noise}
    for prefix, mod in (('h.', model.layers[0]), ('l.', model.last_layer)):
        vs = mod.variational_strategy
        vd = vs._variational_distribution
        out.update({prefix + 'Z': vs.inducing_points, prefix + 'raw_ls': mod.covar_module.base_kernel.raw_lengthscale,
                    prefix + 'raw_os': mod.covar_module.raw_outputscale, prefix + 'm': vd.variational_mean})
        if hasattr(vd, '_variational_stddev'):
            out[prefix + 'raw_stddev'] = vd._variational_stddev
        else:
            out[prefix + 'Lq'] = vd.chol_variational_covar
    out.update({'h.w': model.layers[0].mean_module.weights, 'h.b': model.layers[0].mean_module.bias,
                'l.c': model.last_layer.mean_module.constant})
    return out


@pytest.mark.parametrize('hidden,last', [('mean_field', 'mean_field'), ('mean_field', 'cholesky')])
@pytest.mark.parametrize('num_layers,D,M,B,S', [(1, 3, 40, 315, 3), (2, 2, 64, 128, 4), (1, 2, 130, 200, 10)])
def test_mean_field_dsvi_elbo_and_gradients_match_oracle(num_layers, D, M, B, S, hidden, last):
    """test_dsvi_elbo_and_gradients_match_oracle (its shapes and bounds) for the mean-field model and for a mixed one
    (hidden mean-field, last Cholesky): both take the chain of per-term kernels in fused_dsvi_objective."""
    from oracle import svgp
    from nsgp.gp import mlls, settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    model = _build(num_layers, D, M, 100 + M, hidden, last)
    sd = model.state_dict()
    assert any('_variational_stddev' in k for k in sd) and (last == 'cholesky') == any('chol_variational_covar' in k for k in sd)
    g = _g(7)
    x = torch.randn(B, D, generator=g)
    y = torch.randn(B, generator=g)
    eps = [torch.randn(S, B, 2, generator=g) for _ in range(num_layers)]
    N = 5000
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, N))
    model.train()
    with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        out = model(x.cuda())
        assert mlls.fused_dsvi_objective(mll.base_mll, out, y.cuda(), 1.0, 1.0) is not None       # the chain, not None
        elbo = mll(out, y.cuda())
        assert out.mean.shape == (S, B) and out.variance.shape == (S, B)
        elbo.backward()
    hid, las, noise, leaves = _oracle_layers(model)
    ref = svgp.dsvi_elbo(x.double(), y.double(), hid, las, num_layers, [e.double() for e in eps], S, noise, N)
    ref.backward()
    elbo, ref = elbo.detach(), ref.detach()
    print('[measured] mean-field dsvi elbo rel err %.3g' % (abs(float(elbo) - float(ref)) / abs(float(ref))))
    assert abs(float(elbo) - float(ref)) < 2e-6 * abs(float(ref)) + 1e-7      # the bound of test_dsvi_elbo_and_gradients_match_oracle
    errs = {}
    params = _model_params(model)
    assert set(params) == set(leaves)
    for name, p in params.items():
        got, want = p.grad.detach().cpu().double(), leaves[name].grad
        if name.endswith('Lq'):
            want = torch.tril(want)
        errs[name] = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    print('[measured] mean-field dsvi max grad rel err', (num_layers, D, M, B, S, hidden, last), {k: '%.3g' % v for k, v in errs.items()})
    for name, err in errs.items():
        assert err < DSVI_GRAD_TOL, (name, err)                               # per-parameter max-norm relative error


def test_mean_field_model_trains_on_the_uib_spatial_batch(data_dir):
    import utils.dataprep as dp
    import models.dgps as m
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FusedAdam
    data = dp.download_data(os.path.join(data_dir, 'uib_spatial.csv')).float()
    x, y, *_ = dp.whitening_transform(data)
    trx, try_, _, _ = dp.train_test_split(x, y, 0.8)
    assert trx.shape[0] == 315
    trx, try_ = trx.cuda(), try_.cuda()
    torch.manual_seed(3)
    model = m.DeepGP(1, trx.shape, num_inducing=64, variational='mean_field').cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, trx.shape[0]))
    opt = FusedAdam(model.parameters(), lr=0.01, grads_as_views=False)
    eps = [torch.randn(3, 315, 2, generator=_g(4))]
    model.train()
    losses = []
    for _ in range(5):
        with settings.num_likelihood_samples(3), settings.eps_provider(_FixedEps(eps)):
            opt.zero_grad()
            loss = -mll(model(trx), try_)
            loss.backward()
            opt.step()
        losses.append(float(loss))
    print('[measured] mean-field uib_spatial losses', ['%.5f' % v for v in losses])
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]


# ------------------------------------------------------------------------------------------ 6: predict
def test_mean_field_predict_matches_oracle_and_full_covariance_is_consistent():
    """test_predict_matches_oracle_and_full_covariance_is_consistent, its bounds, for the mean-field model."""
    from oracle import svgp
    from nsgp.gp import settings
    model = _build(1, 2, 48, 321)
    g = _g(9)
    n, S = 78, 4
    x, y = torch.randn(n, 2, generator=g), torch.randn(n, generator=g)
    eps = [torch.randn(S, n, 2, generator=g)]
    model.eval()
    with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        preds, mus, variances, lls = model.predict([(x.cuda(), y.cuda())])
        cov = preds.covariance_matrix
    hidden, last, noise, _ = _oracle_layers(model)
    with torch.no_grad():
        m_ref, v_ref, ll_ref = svgp.dgp_predict(x.double(), y.double(), hidden, last, 1, [e.double() for e in eps], S, noise)
        _, cov_f = svgp.dgp_forward(x.double(), hidden, last, 1, [e.double() for e in eps], S, full_cov_last=True)
    tol = dict(rtol=2e-3, atol=2e-4)
    assert measured('mean-field predict mean', mus, m_ref, **tol)
    assert measured('mean-field predict variance', variances, v_ref, **tol)
    assert measured('mean-field predict lls', lls, ll_ref, rtol=5e-3, atol=5e-3)
    cov_ref = cov_f + float(noise) * torch.eye(n, dtype=F64)
    assert measured('mean-field full covariance', cov, cov_ref, rtol=5e-3, atol=5e-4)
    assert measured('mean-field full covariance diagonal', torch.diagonal(cov, dim1=-1, dim2=-2), v_ref, **tol)


# ------------------------------------------------------------------------------------------ 7: determinism, capture
def _training_setup(M=64, B=256, S=4):
    import models.dgps as m
    from nsgp.dist import PhiloxEps
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FusedAdam
    torch.manual_seed(11)
    model = m.DeepGP(1, (5000, 3), num_inducing=M, variational='mean_field').cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 5000))
    opt = FusedAdam(model.parameters(), lr=0.01, capturable=True, grads_as_views=False)
    g = _g(12)
    x, y = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    eps = PhiloxEps(173, row0=0, step_dev=opt.step_dev)
    model.train()
    return model, mll, opt, x, y, eps, S


def test_mean_field_step_is_bitwise_reproducible_and_capturable():
    """test_timed_step_is_bitwise_reproducible's step (forward + ELBO + backward + FusedAdam, Philox noise keyed by the device
    step counter) with the mean-field model: two eager runs from one state are bit-identical, and three graph-replayed steps
    equal three eager steps bit for bit -- the bound of that test."""
    from nsgp.dist import dp_objective
    from nsgp.gp import settings
    from nsgp.gp.module import transform_cache
    from nsgp.graph import GraphedCallable
    model, mll, opt, x, y, eps, S = _training_setup()
    one = torch.ones((), device='cuda')

    def whole_step():
        eps.start_step(0, row0=0)
        opt.zero_grad()
        with transform_cache():
            out = model(x)
            loss = dp_objective(mll, out, y, x.shape[0], 1, negate=True)
        loss.backward(gradient=one)
        opt.bucket.gather_grads()
        opt.step(gather=False)
        return loss.detach()

    bufs = (opt.bucket.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_dev)

    def restore(s):
        with torch.no_grad():
            for dst, src in zip(bufs, s):
                dst.copy_(src)
        opt.steps = 0

    def run(step, k):
        restore(s0)
        losses = [step().clone() for _ in range(k)]
        torch.cuda.synchronize()
        return dict(loss=torch.stack(losses), grad=opt.bucket.flat_g.clone(), param=opt.bucket.flat_p.clone(),
                    exp_avg_sq=opt.exp_avg_sq.clone())

    with settings.num_likelihood_samples(S), settings.eps_provider(eps):
        with torch.no_grad():
            model(x)                                        # the first call draws the variational-mean initialisation
        for _ in range(2):
            whole_step()
        s0 = [t.detach().clone() for t in bufs]
        s0[3].zero_()
        res = {'eager 1': run(whole_step, 1), 'eager 2': run(whole_step, 1), 'eager x3': run(whole_step, 3)}
        graphed = GraphedCallable(whole_step)
        res['replay x3'] = run(graphed, 3)
    assert bool(torch.isfinite(res['eager x3']['loss']).all()) and float(res['eager x3']['grad'].abs().max()) > 0
    for a, b in (('eager 1', 'eager 2'), ('eager x3', 'replay x3')):
        eq = {k: bool(torch.equal(res[a][k], res[b][k])) for k in res[a]}
        print(f'[measured] mean-field determinism {a} vs {b}: bitwise equal {eq}')
        assert all(eq.values()), ((a, b), eq)
    assert not torch.equal(res['eager 1']['param'], res['eager x3']['param'])


# ------------------------------------------------------------------------------------------ 8: non-PD Kzz
@pytest.mark.parametrize('i8', [True, False])
@pytest.mark.parametrize('fp', ['f32', 'bf16', 'bf16_all'])
def test_non_positive_definite_kzz_gives_nan_marginals_of_a_mean_field_layer(fp, i8):
    """The mean-field twin of test_non_positive_definite_kzz_gives_nan_marginals: the NaNs of the failed Cholesky reach the
    mean and the variance on every forward path, and nothing faults."""
    from nsgp.gp import settings
    from nsgp.svgp import svgp_marginal
    M, n = 72, 200
    Z = torch.randn(1, M, 2, dtype=F32, generator=_g(5)).cuda()
    x = torch.randn(n, 2, dtype=F32, generator=_g(6)).cuda()
    ls = torch.ones(1, 2, device='cuda')
    os_ = -torch.ones(1, device='cuda')
    m = torch.randn(1, M, generator=_g(7)).cuda()
    s2 = (0.5 + torch.rand(1, M, generator=_g(8))).cuda()
    with settings.whiten_matmul_i8(i8), settings.forward_precision(fp):
        mean, var, info = svgp_marginal(x, Z, ls, os_, m, s2=s2, jitter=0.0)
    assert int(info[0]) == 1
    assert not torch.isfinite(mean).any() and not torch.isfinite(var).any(), (fp, i8, int(torch.isfinite(mean).sum()),
                                                                            int(torch.isfinite(var).sum()))
