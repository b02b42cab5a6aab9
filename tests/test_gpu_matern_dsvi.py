"""GPU parity of the Matern DSVI layers (nu = 1/2, 3/2, 5/2) against the float64 CPU oracle.  The oracle is the unmodified
oracle/svgp.py; its kernel, oracle.kernels.rbf_ard, is substituted by the float64 Matern restatement of
tests/matern_dsvi_cases.py.  The int8 plane build and product at the shape edges, coincident points, non-finite inputs; the
layer node in every arithmetic; the mixed whitening chain; the model (ELBO, gradients, predict, full covariance); graph
capture.  Every bound is the one the project states for the same arithmetic on the RBF kernel, named at each assert."""
import contextlib
import math

import pytest
import torch

from conftest import measured
from matern_dsvi_cases import NUS, matern_ard, patch_oracle_kernel
from test_gpu_dgp import DSVI_GRAD_TOL, _FixedEps
from test_gpu_i8 import _ULP_BELOW, I8_LAYER_GRAD_TOL, I8_LAYER_VALUE_TOL
from test_gpu_meanfield import _model_params, _oracle_layers, _raw_stddev, _rel
from test_gpu_svgp import F32_GRAD_TOL, F32_VALUE_TOL

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _cuda(t):
    return t.cuda()


# ------------------------------------------------------------------------------------------ 1: plane build and product
def _kzx64(Z, x, ls, os_, nu):
    b, n, D = Z.shape[0], x.shape[-2], Z.shape[-1]
    xd = x.double() if x.dim() == 3 else x.double().unsqueeze(0).expand(b, n, D)
    return matern_ard(Z.double(), xd, ls.double().unsqueeze(-2), os_.double(), nu)


def _case(b, M, n, D, seed, nu, shared_x=True, os_=None, ls=None, jitter=1e-4):
    """test_gpu_i8._case with the Matern kernel: random inputs of b GPs, W64 = chol(|os| kappa_nu(Z, Z) + jitter I)^-1 in
    float64 from the float32 inputs (an INPUT of the product), and the float64 Kzx."""
    g = _g(seed)
    Z = torch.randn(b, M, D, generator=g)
    x = torch.randn((n, D) if shared_x else (b, n, D), generator=g)
    ls_ = torch.rand(b, D, generator=g) + 0.6
    os_d = torch.rand(b, generator=g) + 0.5
    ls = ls_ if ls is None else torch.as_tensor(ls, dtype=F32).reshape(b, -1).expand(b, D).contiguous()
    os_ = os_d if os_ is None else torch.as_tensor(os_, dtype=F32).reshape(b)
    m = torch.randn(b, M, generator=g)
    Kzz = matern_ard(Z.double(), Z.double(), ls.double().unsqueeze(-2), os_.double().abs(), nu) + jitter * torch.eye(M, dtype=F64)
    W64 = torch.linalg.solve_triangular(torch.linalg.cholesky(Kzz), torch.eye(M, dtype=F64).expand(b, M, M), upper=False)
    return Z, x, ls, os_, m, W64


_EDGES = {
    # name: (b, M, n, D, shared_x, os, ls) -- the rows of test_gpu_i8._EDGE_CASES that concern the build, D = 1..4
    'M1': (2, 1, 100, 2, True, None, None),
    'M31': (2, 31, 200, 3, True, None, None),
    'M33': (1, 33, 65, 3, False, None, None),
    'M129': (3, 129, 63, 2, False, None, None),
    'n1': (2, 200, 1, 3, False, None, None),
    'n63': (2, 160, 63, 2, True, None, None),
    'n65': (3, 100, 65, 1, False, None, None),
    'n257': (2, 40, 257, 4, True, None, None),                        # one column into the second 256-column workgroup
    'n257_batched': (2, 33, 257, 1, False, None, None),
    'os_pow2': (3, 160, 130, 2, True, (2.0, _ULP_BELOW(2.0), -0.75), None),
    'os_pow2_small': (3, 96, 64, 3, False, (0.25, _ULP_BELOW(0.25), -2.0), None),
    'ls_tiny': (3, 150, 100, 2, True, None, (2e-3, 1e-3, 5e-3)),
}


@pytest.mark.parametrize('planes', [4, 5])
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('name', list(_EDGES))
def test_matern_plane_build_and_product_at_the_shape_and_scale_edges(name, nu, planes):
    """ops.svgp_project(..., i8_inputs, kernel_nu): the float32 Kzx the build writes along against the float64 restatement (the
    bound of test_plane_build_kernel_also_writes_the_float32_kzx_the_backward_reads: 1.2e-7 max|ref|), and A, mean, var
    against the float64 product, each GP against ITS OWN product, with the bound forms of
    test_i8_projection_matches_the_float64_product (plus the digit floor of its edge-case twin, which is what holds where
    Kzx is far below os)."""
    from nsgp import ops
    b, M, n, D, shared_x, os_v, ls_v = _EDGES[name]
    Z, x, ls, os_, m, W64 = _case(b, M, n, D, 11 + M + n, nu, shared_x, os_=os_v, ls=ls_v)
    if name == 'ls_tiny':                   # a few columns ON inducing points, so that not all of Kzx is zero
        x[:3] = Z[0, :3]
    Kzx = _kzx64(Z, x, ls, os_, nu)
    A_ref = W64 @ Kzx
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=_g(5))) + 0.3 * torch.eye(M)
    kout = []
    A, C, mean, var = ops.svgp_project(_cuda(W64).float(), None, _cuda(Lq), _cuda(m), _cuda(os_), base_add=1e-4, W64f=_cuda(W64),
                                       i8_inputs=(_cuda(Z), _cuda(x), _cuda(ls), _cuda(os_)), i8_planes=planes, kernel_nu=nu,
                                       i8_kzx_out=kout)
    K32 = kout[0].cpu()
    assert K32.shape == (b, M, n) and torch.isfinite(K32).all()
    kerr = float((K32.double() - Kzx.float().double()).abs().max())
    print(f'[measured] matern nu {nu} {name} planes {planes}: float32 Kzx max err {kerr:.3g}, max|ref| {float(Kzx.abs().max()):.3g}')
    assert kerr <= 1.2e-7 * float(Kzx.abs().max())
    if name == 'ls_tiny':                   # hundreds of lengthscales away: exactly 0, never NaN; the coincident columns: os
        d = ((Z.double().unsqueeze(2) - x.double().reshape(1, 1, n, D)) / ls.double().reshape(b, 1, 1, D)).pow(2).sum(-1).sqrt()
        far = d > 200.0                     # kappa < (1 + 448 + 66667) e^-200 ~ 1e-82: below every float32 and every digit
        assert int(far.sum()) > 0.5 * far.numel() and bool((K32[far] == 0.0).all())
        assert bool((Kzx[d > 800.0] == 0.0).all()) and bool((d > 800.0).any())      # the float64 tail itself ends in 0
        assert torch.equal(K32[0, :3, :3].diagonal(), os_[0].expand(3))
    A, mean, var = A.cpu().double(), mean.cpu().double(), var.cpu().double()
    assert torch.isfinite(A).all() and torch.isfinite(mean).all() and torch.isfinite(var).all()
    mean_ref = (A_ref * m.double().unsqueeze(-1)).sum(1)
    C_ref = torch.tril(Lq).double().transpose(-1, -2) @ A
    var_ref = os_.double().reshape(b, 1) + 1e-4 + (C_ref ** 2).sum(1) - (A ** 2).sum(1)
    assert float((C.cpu().double() - C_ref).abs().max()) < 2e-5 * float(C_ref.abs().max()) + 1e-30
    for i in range(b):
        scale = float((W64[i].abs() @ Kzx[i].abs()).max())
        amax = float(A_ref[i].abs().max())
        kfloor = 2.0 ** -(7 * planes - 1) * abs(float(os_[i])) * float(W64[i].abs().sum(-1).max())
        assert measured(f'matern nu {nu} {name} planes {planes} GP {i} A (scale {scale:.3g}, max|A| {amax:.3g})', A[i], A_ref[i],
                        rtol=0.0, atol=2e-8 * scale + 1.2e-7 * amax + kfloor)
        assert measured(f'matern nu {nu} {name} planes {planes} GP {i} mean', mean[i], mean_ref[i], rtol=0.0,
                        atol=3e-8 * scale * math.sqrt(M) + 3e-7 * float(mean_ref[i].abs().max()) + kfloor * float(m[i].abs().sum()))
        assert measured(f'matern nu {nu} {name} planes {planes} GP {i} var', var[i], var_ref[i], rtol=2e-5,
                        atol=2e-5 * float(os_.abs().max()))


@pytest.mark.parametrize('planes', [4, 5])
@pytest.mark.parametrize('nu', NUS)
def test_matern_kzx_at_coincident_points_is_the_output_scale_exactly(nu, planes):
    """Columns of x that ARE rows of Z: s = 0, kappa = 1 (where poly e could round one ulp above 1 the digit cutter must
    still give digits in [-64, 64]), so those entries of the float32 Kzx equal float32(os) bit for bit -- at os on a power
    of two, one ulp below one, and negative -- and A stays within the product's bound."""
    from nsgp import ops
    b, M, n, D = 3, 70, 130, 3
    os_v = (2.0, _ULP_BELOW(2.0), -_ULP_BELOW(0.5))
    Z, x, ls, os_, m, W64 = _case(b, M, n, D, 77, nu, shared_x=False, os_=os_v)
    rows = torch.tensor([0, 31, 32, 33, 69])
    cols = torch.tensor([0, 63, 64, 65, 129])
    for i in range(b):
        x[i, cols] = Z[i, rows]
    x[:, 100] = Z[:, 5] * (1.0 + 2.0 ** -20)                # nearly coincident: kappa just below 1
    Kzx = _kzx64(Z, x, ls, os_, nu)
    kout = []
    A, _, mean, var = ops.svgp_project(_cuda(W64).float(), None, _cuda(torch.eye(M).expand(b, M, M)), _cuda(m), _cuda(os_),
                                       base_add=1e-4, W64f=_cuda(W64), i8_inputs=(_cuda(Z), _cuda(x), _cuda(ls), _cuda(os_)),
                                       i8_planes=planes, kernel_nu=nu, i8_kzx_out=kout)
    K32 = kout[0].cpu()
    for i in range(b):
        assert torch.equal(K32[i, rows, cols], os_[i].expand(len(rows))), (nu, planes, i, K32[i, rows, cols], os_[i])
    assert bool((K32.abs() <= os_.abs().reshape(b, 1, 1)).all())
    A_ref = W64 @ Kzx
    for i in range(b):
        scale = float((W64[i].abs() @ Kzx[i].abs()).max())
        assert measured(f'matern nu {nu} coincident planes {planes} GP {i} A', A[i], A_ref[i], rtol=0.0,
                        atol=2e-8 * scale + 1.2e-7 * float(A_ref[i].abs().max()))
    assert torch.isfinite(mean).all() and torch.isfinite(var).all()


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('poison', ['x_row', 'Z_row', 'ls', 'os_nan', 'os_inf', 'W_rows'])
def test_matern_i8_projection_propagates_non_finite_inputs(poison, nu):
    """The contract and the assertions of test_i8_projection_propagates_non_finite_inputs with the Matern plane build: every
    output entry whose float64 reference is NaN / +-Inf is not finite, the other GPs of the launch are bit-identical to a
    clean run."""
    from nsgp import ops
    b, M, n, D = 3, 200, 300, 3
    Z, x, ls, os_, m, W64 = _case(b, M, n, D, 21, nu, shared_x=False)
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=_g(6))) + 0.3 * torch.eye(M)

    def run(Z, x, ls, os_, W64):
        out = ops.svgp_project(_cuda(W64).float(), None, _cuda(Lq), _cuda(m), _cuda(os_), base_add=1e-4, W64f=_cuda(W64),
                               i8_inputs=(_cuda(Z), _cuda(x), _cuda(ls), _cuda(os_)), kernel_nu=nu)
        return [t.cpu() for t in out]
    clean = run(Z, x, ls, os_, W64)
    Zp, xp, lsp, osp, Wp = Z.clone(), x.clone(), ls.clone(), os_.clone(), W64.clone()
    nan = float('nan')
    if poison == 'x_row':
        xp[1, 77, 0] = nan
    elif poison == 'Z_row':
        Zp[1, 150, 2] = nan
    elif poison == 'ls':
        lsp[1, 1] = nan
    elif poison == 'os_nan':
        osp[1] = nan
    elif poison == 'os_inf':
        osp[1] = float('inf')
    else:
        Wp[1, 120:] = nan
    A, C, mean, var = run(Zp, xp, lsp, osp, Wp)
    K1 = _kzx64(Zp[1:2], xp[1:2], lsp[1:2], osp[1:2], nu)[0]
    Wl = torch.tril(Wp[1])
    fin = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)                   # noqa: E731
    A1 = fin(Wl) @ fin(K1)
    reach = (torch.tril(torch.ones(M, M, dtype=F64)) @ (~torch.isfinite(K1)).double()) > 0
    A1[reach | (~torch.isfinite(Wl)).any(1, keepdim=True)] = float('nan')
    mean1 = A1.T @ m[1].double()
    var1 = osp[1].double() + 1e-4 + ((torch.tril(Lq[1]).double().T @ A1) ** 2).sum(0) - (A1 ** 2).sum(0)
    bad_A, bad_mean, bad_var = ~torch.isfinite(A1), ~torch.isfinite(mean1), ~torch.isfinite(var1)
    assert bad_mean.any()                               # (the case does poison the output)
    assert not torch.isfinite(A[1][bad_A]).any()
    assert not torch.isfinite(mean[1][bad_mean]).any()
    assert not torch.isfinite(var[1][bad_var]).any()
    for i in (0, 2):                                    # the clean GPs of the same launches: bit for bit
        for got, ref in zip((A, C, mean, var), clean):
            assert torch.equal(got[i], ref[i]), (poison, i)


# ------------------------------------------------------------------------------------------ 2: the layer against the oracle
LAYER = dict(b=2, M=160, n=130, D=2, seed=41)
_ORACLE = {}


def _layer_inputs(spread):
    """The recipe of test_i8_layer_values_and_gradients_match_the_oracle at b = 2, M = 160, n = 130, D = 2; `spread` widens x and
    Z (test_gpu_meanfield.SPREAD: where A = W Kzx accumulates in float32 the value bound holds for the kernels only on
    better-conditioned inputs)."""
    b, M, n, D = LAYER['b'], LAYER['M'], LAYER['n'], LAYER['D']
    g = _g(LAYER['seed'])
    x = spread * torch.randn(n, D, generator=g)
    Z = spread * 1.5 * torch.randn(b, M, D, generator=g)
    ls = torch.rand(b, D, generator=g) * 0.3 + 0.8
    os_ = torch.rand(b, generator=g) + 0.5
    m = torch.randn(b, M, generator=g)
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=g)) + 0.5 * torch.eye(M)
    s2 = (0.5 + torch.rand(b, M, generator=g)) ** 2
    gm, gv = torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)
    return (x, Z, ls, os_, m), Lq, s2, gm, gv


def _layer_oracle(monkeypatch, nu, mean_field, spread):
    """Values and gradients of (x, Z, ls, os, m, Lq | s2) from oracle.svgp.svgp_marginal in float64 on the float32 inputs;
    computed once per case and shared."""
    key = (nu, mean_field, spread)
    if key not in _ORACLE:
        from oracle import svgp as OS
        patch_oracle_kernel(monkeypatch, nu)
        b, M, n, D = LAYER['b'], LAYER['M'], LAYER['n'], LAYER['D']
        common, Lq, s2, gm, gv = _layer_inputs(spread)
        leaves = [t.double().requires_grad_() for t in (*common, s2 if mean_field else Lq)]
        xr, Zr, lsr, osr, mr, qr = leaves
        p = dict(Z=Zr, lengthscale=lsr.unsqueeze(-2), outputscale=osr, m=mr, Lq=torch.diag_embed(qr.sqrt()) if mean_field else qr,
                 mean=('constant', torch.zeros(b, 1, dtype=F64)))
        mean_r, var_r = OS.svgp_marginal(xr.unsqueeze(0).expand(b, n, D), p)
        ((mean_r * gm.double()).sum() + (var_r * gv.double()).sum()).backward()
        grads = [torch.tril(t.grad) if (i == 5 and not mean_field) else t.grad for i, t in enumerate(leaves)]
        assert all(torch.isfinite(t).all() for t in grads)
        _ORACLE[key] = (mean_r.detach(), var_r.detach(), grads)
    return _ORACLE[key]


ARITH = [
    # id, settings, kzx_f64, dtype, spread, expected first product, whose bounds
    ('i8', {}, False, F32, 1.0, 'i8', 'i8'),
    ('i8 5 planes', {}, True, F32, 1.0, 'i8', 'i8'),
    ('f64acc', dict(whiten_matmul_i8=False), False, F32, 1.0, 'f64acc', 'f32'),
    ('f64acc_b64', dict(whiten_matmul_i8=False), True, F32, 1.0, 'f64acc_b64', 'f32'),
    ('f32', dict(whiten_matmul_f64=False), False, F32, 3.0, 'f32', 'f32'),
    ('bf16', dict(forward_precision='bf16'), False, F32, 1.0, 'i8', 'i8'),
    ('float64', {}, False, F64, 1.0, 'f32', 'f64'),
]
NAMES = ('x', 'Z', 'ls', 'os', 'm', 'q')


@pytest.mark.parametrize('arith', ARITH, ids=[a[0].replace(' ', '_') for a in ARITH])
@pytest.mark.parametrize('mean_field', [False, True], ids=['cholesky', 'mean_field'])
@pytest.mark.parametrize('nu', NUS)
def test_matern_layer_matches_the_oracle_in_every_arithmetic(monkeypatch, nu, mean_field, arith):
    """svgp_marginal(..., nu) against torch.autograd of the oracle in float64: mean, variance and the gradients of x, Z, ls, os,
    m and Lq / s2.  Bounds: test_gpu_i8.py's I8_LAYER_VALUE_TOL / I8_LAYER_GRAD_TOL (max-norm relative) where A is the int8
    product, test_gpu_svgp.py's F32_VALUE_TOL / F32_GRAD_TOL for the other float32 arithmetics (with test_gpu_meanfield.py's
    input spread where A accumulates in float32), that file's float64 bounds for the float64 layer."""
    from nsgp import svgp
    from nsgp.gp import settings
    name, flags, kzx_f64, dt, spread, want, tols = arith
    mean_r, var_r, grads_r = _layer_oracle(monkeypatch, nu, mean_field, spread)
    common, Lq, s2, gm, gv = _layer_inputs(spread)
    leaves = [t.to(dt).cuda().requires_grad_() for t in (*common, s2 if mean_field else Lq)]
    seen = []
    entry = 'svgp_project_diag' if mean_field else 'svgp_project_bf16' if name == 'bf16' else 'svgp_project'
    orig = getattr(svgp.ops, entry)

    def spy(*a, **kw):
        first = a[0] if mean_field else 'i8' if kw.get('i8_inputs') is not None else 'f64acc_b64' if kw.get('Kzx64') is not None \
            else 'kzx_fused' if kw.get('kernel_inputs') is not None else 'f64acc' if kw.get('W64f') is not None else 'f32'
        seen.append((first, kw.get('i8_planes'), kw.get('kernel_nu')))
        return orig(*a, **kw)
    monkeypatch.setattr(svgp.ops, entry, spy)
    with contextlib.ExitStack() as st:
        for k, v in flags.items():
            st.enter_context(getattr(settings, k)(v))
        q = dict(s2=leaves[5]) if mean_field else dict(Lq=leaves[5])
        mean, var, info = svgp.svgp_marginal(*leaves[:5], kzx_f64=kzx_f64, nu=nu, **q)
        ((mean * gm.to(dt).cuda()).sum() + (var * gv.to(dt).cuda()).sum()).backward()
    assert info.cpu().tolist() == [0] * LAYER['b']
    assert seen[0][0] == want, (name, seen)
    if want == 'i8':
        assert seen[0][2] == nu and (name == 'bf16' or seen[0][1] == (5 if kzx_f64 else 4)), (name, seen)
    errs = {nm: _rel(t.grad, r) for nm, t, r in zip(NAMES, leaves, grads_r)}
    em, ev = _rel(mean, mean_r), _rel(var, var_r)
    print(f'[measured] matern layer nu {nu} {"mean-field" if mean_field else "cholesky"} {name}: mean {em:.3g} var {ev:.3g} grads',
          {k: '%.3g' % v for k, v in errs.items()})
    if name == 'bf16' and not mean_field:
        # C = Lq^T A on bf16 operands: the variance and the gradients carry bf16's error whatever the kernel (measured 2.8e-3
        # on the variance; tests/test_gpu_bf16.py holds that product).  What sees the kernel is A, hence the mean.
        assert em < I8_LAYER_VALUE_TOL, (name, em)
        assert all(torch.isfinite(t.grad).all() for t in leaves) and ev < 5e-2, (name, ev)
    elif tols == 'i8':
        assert em < I8_LAYER_VALUE_TOL and ev < I8_LAYER_VALUE_TOL, (name, em, ev)
        assert max(errs.values()) < I8_LAYER_GRAD_TOL, (name, errs)
    else:
        tol = dict(rtol=1e-9, atol=1e-10) if tols == 'f64' else F32_VALUE_TOL
        ok_mean = measured(f'matern layer nu {nu} {name} mean', mean, mean_r, **tol)
        ok_var = measured(f'matern layer nu {nu} {name} var', var, var_r, **tol)
        assert ok_mean and ok_var, (name, nu, mean_field)
        assert max(errs.values()) < (1e-7 if tols == 'f64' else F32_GRAD_TOL), (name, errs)


# ------------------------------------------------------------------------------------------ 3: the whitening chain
def test_rbf_and_matern_groups_share_one_whitening_chain(monkeypatch):
    """whiten([(RBF group), (Matern group)], nu=[None, 1.5]) equals the two groups whitened separately, W and info bit for
    bit, and its gradients are the float64 oracle's (chol(Kzz + jitter I)^-1 by torch autograd; the float64 bound of
    test_gpu_svgp.py: 1e-7 max-norm relative)."""
    from nsgp import svgp
    from oracle import kernels
    g = _g(3)
    M = 64
    mk = lambda b, D: (torch.randn(b, M, D, generator=g, dtype=F64), torch.rand(b, D, generator=g, dtype=F64) + 0.7,   # noqa: E731
                       torch.rand(b, generator=g, dtype=F64) + 0.5)
    groups = [mk(2, 3), mk(1, 2)]
    nus = [None, 1.5]
    Gs = [torch.randn(2, M, M, generator=g, dtype=F64), torch.randn(1, M, M, generator=g, dtype=F64)]
    for dt in (F64, F32):
        dev = [tuple(t.to(dt).cuda().requires_grad_() for t in grp) for grp in groups]
        Ws, info = svgp.whiten(dev, nu=nus, out_dtype=dt)
        sum((W.double() * G.cuda()).sum() for W, G in zip(Ws, Gs)).backward()
        off = 0
        for gi, (grp, nu) in enumerate(zip(groups, nus)):
            alone = tuple(t.to(dt).cuda() for t in grp)
            (W1,), info1 = svgp.whiten([alone], nu=[nu], out_dtype=dt)
            assert torch.equal(Ws[gi], W1) and torch.equal(info[off:off + grp[0].shape[0]], info1), (dt, gi)
            off += grp[0].shape[0]
        assert info.cpu().tolist() == [0, 0, 0]
        if dt == F32:
            continue
        for gi, (grp, nu, G) in enumerate(zip(groups, nus, Gs)):
            Z, ls, os_ = (t.clone().requires_grad_() for t in grp)
            K = (kernels.rbf_ard(Z, Z, ls.unsqueeze(-2), os_) if nu is None else matern_ard(Z, Z, ls.unsqueeze(-2), os_, nu)) \
                + 1e-4 * torch.eye(M, dtype=F64)
            W = torch.linalg.solve_triangular(torch.linalg.cholesky(K), torch.eye(M, dtype=F64).expand_as(K), upper=False)
            assert measured(f'whiten group {gi} (nu {nu}) W', Ws[gi], W, rtol=0.0, atol=1e-9 * float(W.abs().max()))
            (W * G).sum().backward()
            for nm, got, ref in zip(('Z', 'ls', 'os'), dev[gi], (Z, ls, os_)):
                err = _rel(got.grad, ref.grad)
                print(f'[measured] mixed whitening chain group {gi} (nu {nu}) grad {nm}: {err:.3g}')
                assert err < 1e-7, (gi, nm, err)


# ------------------------------------------------------------------------------------------ 4: the model
def _build(nu, variational, seed, M=64, D=2):
    """test_gpu_meanfield._build for DeepGP(2, ..., nu=nu): away from the trivial initialisation."""
    import models.dgps as m
    torch.manual_seed(seed)
    model = m.DeepGP(2, (1000, D), num_inducing=M, variational=variational, nu=nu).cuda()
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


MODELS = [(1.5, 'cholesky'), ((None, 2.5), 'cholesky'), (1.5, 'mean_field'), (0.5, 'cholesky')]


@pytest.mark.parametrize('nu,variational', MODELS, ids=[f'{n}-{v}' for n, v in MODELS])
def test_matern_deepgp_elbo_gradients_predict_and_full_covariance_match_the_oracle(monkeypatch, nu, variational):
    """DeepGP(2, shape, num_inducing=64, nu=...) at a batch of 96, S = 3, as tests/test_gpu_dgp.py holds the RBF model: the
    ELBO (2e-6 relative) and every parameter gradient (DSVI_GRAD_TOL) against oracle.svgp.dsvi_elbo, predict against
    dgp_predict and the dense predictive covariance against the oracle's full_cov=True (the bounds of
    test_predict_matches_oracle_and_full_covariance_is_consistent)."""
    from oracle import svgp
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    B, S, D, N = 96, 3, 2, 5000
    model = _build(nu, variational, 164)
    nu_h, nu_l = nu if isinstance(nu, tuple) else (nu, nu)
    assert model.layers[0] is model.layers[1] and model.layers[0].variational_strategy.nu == nu_h \
        and model.last_layer.variational_strategy.nu == nu_l
    g = _g(7)
    x, y = torch.randn(B, D, generator=g), torch.randn(B, generator=g)
    eps = [torch.randn(S, B, 2, generator=g) for _ in range(2)]
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, N))
    model.train()
    with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        out = model(x.cuda())
        elbo = mll(out, y.cuda())
        assert out.mean.shape == (S, B) and out.variance.shape == (S, B)
        elbo.backward()
    hid, las, noise, leaves = _oracle_layers(model)
    patch_oracle_kernel(monkeypatch, None, {id(hid['lengthscale']): nu_h, id(las['lengthscale']): nu_l})
    ref = svgp.dsvi_elbo(x.double(), y.double(), hid, las, 2, [e.double() for e in eps], S, noise, N)
    ref.backward()
    elbo, ref = elbo.detach(), ref.detach()
    print('[measured] matern dsvi nu %s %s elbo rel err %.3g' % (nu, variational, abs(float(elbo) - float(ref)) / abs(float(ref))))
    assert abs(float(elbo) - float(ref)) < 2e-6 * abs(float(ref)) + 1e-7      # the bound of test_dsvi_elbo_and_gradients_match_oracle
    params = _model_params(model)
    assert set(params) == set(leaves)
    errs = {}
    for name, p in params.items():
        got, want = p.grad.detach().cpu().double(), leaves[name].grad
        if name.endswith('Lq'):
            want = torch.tril(want)
        errs[name] = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-12)
    print('[measured] matern dsvi max grad rel err', (nu, variational), {k: '%.3g' % v for k, v in errs.items()})
    for name, err in errs.items():
        assert err < DSVI_GRAD_TOL, (name, err)                               # per-parameter max-norm relative error
    # predict and the dense covariance
    model.eval()
    with settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        preds, mus, variances, lls = model.predict([(x.cuda(), y.cuda())])
        cov = preds.covariance_matrix
    with torch.no_grad():
        m_ref, v_ref, ll_ref = svgp.dgp_predict(x.double(), y.double(), hid, las, 2, [e.double() for e in eps], S, noise)
        _, cov_f = svgp.dgp_forward(x.double(), hid, las, 2, [e.double() for e in eps], S, full_cov_last=True)
    tol = dict(rtol=2e-3, atol=2e-4)
    assert measured('matern predict mean', mus, m_ref, **tol)
    assert measured('matern predict variance', variances, v_ref, **tol)
    assert measured('matern predict lls', lls, ll_ref, rtol=5e-3, atol=5e-3)
    cov_ref = cov_f + float(noise) * torch.eye(B, dtype=F64)
    assert measured('matern full covariance', cov, cov_ref, rtol=5e-3, atol=5e-4)
    assert measured('matern full covariance diagonal', torch.diagonal(cov, dim1=-1, dim2=-2), v_ref, **tol)


# ------------------------------------------------------------------------------------------ 5: graph capture
def test_matern_training_step_replays_from_a_graph_bit_for_bit():
    """One Matern training step (forward + ELBO + backward + FusedAdam, Philox noise keyed by the device step counter)
    captured with nsgp.graph.GraphedCallable and replayed: loss, gradients, parameters and the second moments equal the eager
    steps' bit for bit, as test_mean_field_step_is_bitwise_reproducible_and_capturable holds the mean-field model."""
    import models.dgps as m
    from nsgp.dist import PhiloxEps, dp_objective
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.gp.module import transform_cache
    from nsgp.graph import GraphedCallable
    from nsgp.optim import FusedAdam
    M, B, S = 64, 256, 4
    torch.manual_seed(11)
    model = m.DeepGP(1, (5000, 3), num_inducing=M, nu=1.5).cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 5000))
    opt = FusedAdam(model.parameters(), lr=0.01, capturable=True, grads_as_views=False)
    g = _g(12)
    x, y = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    eps = PhiloxEps(173, row0=0, step_dev=opt.step_dev)
    model.train()
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

    def run(step, k):
        with torch.no_grad():
            for dst, src in zip(bufs, s0):
                dst.copy_(src)
        opt.steps = 0
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
        eager = run(whole_step, 3)
        replay = run(GraphedCallable(whole_step), 3)
    assert bool(torch.isfinite(eager['loss']).all()) and float(eager['grad'].abs().max()) > 0
    assert float(eager['loss'][0]) != float(eager['loss'][2])
    eq = {k: bool(torch.equal(eager[k], replay[k])) for k in eager}
    print(f'[measured] matern step eager x3 vs replay x3: bitwise equal {eq}')
    assert all(eq.values()), eq
