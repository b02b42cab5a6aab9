"""The int8 digit-plane projection A = W Kzx (csrc/gemm_i8.hip; settings.whiten_matmul_i8): exact int32 accumulation of 14
plane products of the float64 W and of Kzx evaluated in float64, against the float64 product formed on the host --
gpytorch's float64 triangular solve behind models/dgps.py:44-51."""
import math

import pytest
import torch

from conftest import measured

pytestmark = pytest.mark.gpu
F64 = torch.float64
I8_LAYER_VALUE_TOL = 1.5e-5     # measured 4.8e-6 (mean), 1.2e-6 (variance) on MI355X
I8_LAYER_GRAD_TOL = 3e-3         # measured 1.0e-3 (os: the whitening adjoint through the float32 W), 2e-4 for x, Z, ls


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _case(b, M, n, D, seed, shared_x=True, os_=None, ls=None, jitter=1e-4):
    """Random inputs of b GPs; `os_` / `ls` (per GP) replace the drawn ones, the draws stay the same.  W64 = chol(Kzz)^-1 of
    the float32 inputs' Kzz + jitter I, formed in float64 (W64 is an INPUT of the product: its own error does not matter)."""
    g = torch.Generator().manual_seed(seed)
    Z = torch.randn(b, M, D, generator=g)
    x = torch.randn((n, D) if shared_x else (b, n, D), generator=g)
    ls_ = torch.rand(b, D, generator=g) + 0.6
    os_d = torch.rand(b, generator=g) + 0.5
    ls = ls_ if ls is None else torch.as_tensor(ls, dtype=torch.float32).reshape(b, -1).expand(b, D).contiguous()
    os_ = os_d if os_ is None else torch.as_tensor(os_, dtype=torch.float32).reshape(b)
    m = torch.randn(b, M, generator=g)
    Zd, lsd, osd = Z.double(), ls.double(), os_.double()
    xd = x.double() if x.dim() == 3 else x.double().unsqueeze(0).expand(b, n, D)
    # (|os|: a negative output scale only flips the sign of Kzx here; W stays that of a positive definite Kzz)
    Kzz = osd.abs().reshape(b, 1, 1) * torch.exp(-0.5 * (((Zd.unsqueeze(2) - Zd.unsqueeze(1)) / lsd.reshape(b, 1, 1, D)) ** 2)
                                                  .sum(-1)) + jitter * torch.eye(M, dtype=F64)
    W64 = torch.linalg.solve_triangular(torch.linalg.cholesky(Kzz), torch.eye(M, dtype=F64).expand(b, M, M), upper=False)
    Kzx = osd.reshape(b, 1, 1) * torch.exp(-0.5 * (((Zd.unsqueeze(2) - xd.unsqueeze(1)) / lsd.reshape(b, 1, 1, D)) ** 2).sum(-1))
    return Z, x, ls, os_, m, W64, Kzx


@pytest.mark.parametrize('b,M,n,D,shared_x', [(1, 1024, 4096, 2, True), (2, 1024, 1000, 3, True), (3, 200, 333, 3, False),
                                               (1, 96, 50, 1, True), (2, 128, 64, 4, True)])
def test_i8_projection_matches_the_float64_product(b, M, n, D, shared_x):
    _need_gpu()
    from nsgp import ops
    Z, x, ls, os_, m, W64, Kzx = _case(b, M, n, D, 7 + M + n, shared_x)
    A_ref = W64 @ Kzx
    c = lambda t: t.cuda()
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=torch.Generator().manual_seed(1))) + 0.3 * torch.eye(M)
    A, C, mean, var = ops.svgp_project(c(W64).float(), None, c(Lq), c(m), c(os_), base_add=1e-4, W64f=c(W64),
                                       i8_inputs=(c(Z), c(x), c(ls), c(os_)))
    print('kappa-free scale: max|W| %.3g, max sum|W||K| %.3g, max|A| %.3g' % (
        float(W64.abs().max()), float((W64.abs() @ Kzx.abs()).max()), float(A_ref.abs().max())))
    # 35-bit W digits, 28-bit K digits, pairs with a + b >= 5 dropped: a few 1e-7 of the PRODUCT SCALE sum|W||K|, which at
    # kappa ~ 1e6 is ~1e2 x max|A|; measured 9.5e-7 of max|A| at the headline shape
    scale = float((W64.abs() @ Kzx.abs()).max())
    assert measured(f'i8 A b{b} M{M} n{n} D{D}', A, A_ref, rtol=0.0, atol=2e-8 * scale + 1.2e-7 * float(A_ref.abs().max()))
    mean_ref = (A_ref * m.double().unsqueeze(-1)).sum(1)
    assert measured('i8 mean', mean, mean_ref, rtol=0.0, atol=3e-8 * scale * math.sqrt(M) + 3e-7 * float(mean_ref.abs().max()))
    # the second projection and the variance follow from the kernel's own A (float32 path here)
    C_ref = torch.tril(Lq).double().transpose(-1, -2) @ A.cpu().double()
    assert float((C.cpu().double() - C_ref).abs().max() / C_ref.abs().max()) < 2e-5
    var_ref = os_.double().reshape(b, 1) + 1e-4 + (C_ref ** 2).sum(1) - (A.cpu().double() ** 2).sum(1)
    assert measured('i8 var', var, var_ref, rtol=2e-5, atol=2e-5 * float(os_.max()))


def test_i8_projection_with_float64_second_projection_and_partials():
    """Layers that feed the next layer (settings.hidden_var_f64): C = Lq^T A on the float64-accumulating kernel and float64
    partials -- the variance carries no cancellation loss."""
    _need_gpu()
    from nsgp import ops
    b, M, n, D = 2, 1024, 4096, 3
    Z, x, ls, os_, m, W64, Kzx = _case(b, M, n, D, 99)
    c = lambda t: t.cuda()
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=torch.Generator().manual_seed(2))) + 0.1 * torch.eye(M)
    A, C, mean, var = ops.svgp_project(c(W64).float(), None, c(Lq), c(m), c(os_), base_add=1e-4, W64f=c(W64),
                                       i8_inputs=(c(Z), c(x), c(ls), c(os_)), Lq64=c(Lq).double(), i8_planes=5)
    A_ref = W64 @ Kzx
    # five Kzx planes (35 bits below os): what is left is W's own 35-bit digits and the dropped pairs a + b >= 5 -- measured
    # 3.7e-7 of max|A| here (4 planes: 1.3e-6)
    assert measured('i8 (5 planes) A', A, A_ref, rtol=0.0, atol=8e-7 * float(A_ref.abs().max()))
    C_ref = torch.tril(Lq).double().transpose(-1, -2) @ A.cpu().double()
    var_ref = os_.double().reshape(b, 1) + 1e-4 + (C_ref ** 2).sum(1) - (A_ref ** 2).sum(1)
    scale = float((W64.abs() @ Kzx.abs()).max())
    assert measured('i8+f64 C', C, C_ref, rtol=0.0, atol=2e-7 * float(C_ref.abs().max()))
    assert measured(f'i8+f64 var (min var / os = {float((var_ref / os_.double().reshape(b, 1)).min()):.2g})', var, var_ref,
                    rtol=3e-7, atol=1e-7 * scale)


def test_model_level_switch_and_backward():
    """settings.whiten_matmul_i8 on / off through the layer: same values to float32 accuracy, gradients alike."""
    _need_gpu()
    from nsgp.gp import settings
    from nsgp.svgp import svgp_marginal
    g = torch.Generator().manual_seed(3)
    b, M, n, D = 2, 256, 500, 3
    mk = lambda *s: torch.randn(*s, generator=g).cuda()
    x, Z = mk(n, D), mk(b, M, D)
    ls, os_ = (torch.rand(b, D, generator=g) + 0.7).cuda(), (torch.rand(b, generator=g) + 0.5).cuda()
    m = mk(b, M)
    Lq = (torch.tril(0.1 * torch.randn(b, M, M, generator=g)) + torch.eye(M)).cuda()
    gm, gv = mk(b, n), mk(b, n)
    res = {}
    for on in (True, False):
        leaves = [t.clone().requires_grad_() for t in (Z, ls, os_, m, Lq)]
        with settings.whiten_matmul_i8(on):
            mean, var, _ = svgp_marginal(x, *leaves)
        ((mean * gm).sum() + (var * gv).sum()).backward()
        res[on] = (mean.detach(), var.detach(), [t.grad for t in leaves])
    # (the float64-accumulating path multiplies a float32-ROUNDED Kzx: its own error, ~4e-5 here, dominates the difference)
    assert measured('mean i8 vs f64acc', res[True][0], res[False][0], rtol=0.0, atol=2e-4 * float(res[False][0].abs().max()))
    assert measured('var i8 vs f64acc', res[True][1], res[False][1], rtol=0.0, atol=2e-4 * float(res[False][1].abs().max()))
    for a, r in zip(res[True][2], res[False][2]):
        assert float((a - r).abs().max()) < 2e-3 * float(r.abs().max()) + 1e-6


def test_plane_build_kernel_also_writes_the_float32_kzx_the_backward_reads():
    """nsgp_i8_rbf_build_f32(..., Kzx_f32): the float32 Kzx rounded from the float64 values the digits are cut from -- equal to
    the float64 oracle kernel rounded to float32, to one float32 ulp (the kernel's own exp is good to ~1 ulp of float64).  The
    layer keeps it for its backward pass (Wbar = tril(Abar Kzx^T)) instead of launching a float32 build there; the gradients of
    that path are held to the float64 oracle by test_i8_layer_values_and_gradients_match_the_oracle below."""
    import torch
    from nsgp import _lib, ops
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    g = torch.Generator().manual_seed(4)
    b, M, n, D = 2, 200, 333, 3
    Z, x = torch.randn(b, M, D, generator=g), torch.randn(n, D, generator=g)
    ls, os_ = torch.rand(b, D, generator=g) + 0.6, torch.rand(b, generator=g) + 0.5
    lib = _lib.load()
    dZ, dx, dls, dos = Z.cuda(), x.cuda(), ls.cuda(), os_.cuda()
    Kd = torch.empty(int(lib.nsgp_i8_k_planes_bytes(b, M, n, 4)), dtype=torch.uint8, device='cuda')
    ksc = torch.empty(int(lib.nsgp_i8_kscale_count(b, M, n)), dtype=torch.float64, device='cuda')
    K32 = torch.full((b, M, n), float('nan'), device='cuda')
    _lib.call('nsgp_i8_rbf_build_f32', ops._p(dZ), ops._p(dx), 0, ops._p(dls), ops._p(dos), b, M, n, D, 4, ops._p(Kd), ops._p(ksc),
              ops._p(K32), ops._stream())
    d2 = (((Z.double().unsqueeze(2) - x.double().unsqueeze(0).unsqueeze(1)) / ls.double().reshape(b, 1, 1, D)) ** 2).sum(-1)
    ref = (os_.double().reshape(b, 1, 1) * torch.exp(-0.5 * d2)).float()
    assert torch.isfinite(K32).all()
    assert float((K32.cpu() - ref).abs().max()) <= 1.2e-7 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------- shapes and edges
_ULP_BELOW = lambda v: float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(0.0)))   # noqa: E731
_EDGE_CASES = {
    # name: (b, M, n, D, shared_x, os, ls, jitter)
    'M1': (2, 1, 100, 2, True, None, None, 1e-4),                     # one row: a single, mostly padded k-block
    'M31': (2, 31, 200, 3, True, None, None, 1e-4),                   # below one 32-deep k-block
    'M33': (1, 33, 65, 3, False, None, None, 1e-4),                   # one row past it
    'M129': (3, 129, 63, 2, False, None, None, 1e-4),                 # one row into the second 128-row tile
    'M4096': (2, 4096, 300, 4, True, None, None, 1e-9),               # the nsgp_i8_supported limit, kappa(Kzz) ~ 1e12
    'n1': (2, 200, 1, 3, False, None, None, 1e-4),
    'n63': (2, 160, 63, 2, True, None, None, 1e-4),
    'n65': (3, 100, 65, 1, False, None, None, 1e-4),
    # the digit scale (frexp of os): exactly 2^k (leading digit 32), one float32 ulp below (leading digit 64), negative
    'os_pow2': (3, 160, 130, 2, True, (2.0, _ULP_BELOW(2.0), -0.75), None, 1e-4),
    'os_pow2_small': (3, 96, 64, 3, False, (0.25, _ULP_BELOW(0.25), -2.0), None, 1e-4),
    # Kzx underflows to 0 almost everywhere / Kzx ~ os everywhere (leading digit 64 just below a power of two)
    'ls_tiny': (3, 150, 100, 2, True, None, (2e-3, 1e-3, 5e-3), 1e-4),
    'ls_huge': (3, 150, 100, 2, True, (_ULP_BELOW(1.0), 1.0, -_ULP_BELOW(0.5)), (1e4, 3e3, 1e5), 1e-4),
}


@pytest.mark.parametrize('planes', [4, 5])
@pytest.mark.parametrize('name', list(_EDGE_CASES))
def test_i8_projection_shapes_and_digit_scale_edges(name, planes):
    """Shapes the int8 kernels accept but the headline never runs (one k-block or less, partial tiles, one column, the M =
    4096 limit), the digit scale at and just below a power of two and negative, Kzx underflowing / saturating -- each GP
    of a launch against ITS OWN float64 product W64 @ Kzx (a scale or a plane stride that crossed a batch boundary would
    show up in the other GPs), both Kzx plane counts."""
    _need_gpu()
    from nsgp import ops
    b, M, n, D, shared_x, os_v, ls_v, jitter = _EDGE_CASES[name]
    Z, x, ls, os_, m, W64, Kzx = _case(b, M, n, D, 11 + M + n, shared_x, os_=os_v, ls=ls_v, jitter=jitter)
    if name == 'ls_tiny':                   # a few columns ON inducing points, so that not all of Kzx is zero
        x[:3] = Z[0, :3]
        xd = x.double().unsqueeze(0).expand(b, n, D)
        Kzx = os_.double().reshape(b, 1, 1) * torch.exp(-0.5 * (((Z.double().unsqueeze(2) - xd.unsqueeze(1))
                                                               / ls.double().reshape(b, 1, 1, D)) ** 2).sum(-1))
    A_ref = W64 @ Kzx
    c = lambda t: t.cuda()                                                                    # noqa: E731
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=torch.Generator().manual_seed(5))) + 0.3 * torch.eye(M)
    A, C, mean, var = ops.svgp_project(c(W64).float(), None, c(Lq), c(m), c(os_), base_add=1e-4, W64f=c(W64),
                                       i8_inputs=(c(Z), c(x), c(ls), c(os_)), i8_planes=planes)
    A, mean = A.cpu().double(), mean.cpu().double()
    assert torch.isfinite(A).all() and torch.isfinite(mean).all() and torch.isfinite(var).all()
    mean_ref = (A_ref * m.double().unsqueeze(-1)).sum(1)
    if M == 4096:
        ev = torch.linalg.eigvalsh(W64[0].T @ W64[0])                 # (L L^T)^-1 = W^T W: kappa(Kzz + jitter I)
        print(f'[{name}] kappa(Kzz + {jitter:g} I) of GP 0: {float(ev[-1] / ev[0]):.3g}')
    for i in range(b):
        # the bound form of test_i8_projection_matches_the_float64_product: a few 1e-8 of the product scale max sum|W||K|
        # (35-bit W digits, dropped pairs) plus the float32 rounding of A, plus the Kzx digits' own floor: entries are cut
        # to a unit of 2^-(7 planes - 1) of the digit scale 2^e >= |os|, so |dK| <= 2^-(7 planes - 1) |os| wherever Kzx
        # itself is far below os (ls -> 0), |dA| <= that times max_m sum_k |W[m][k]|
        scale = float((W64[i].abs() @ Kzx[i].abs()).max())
        amax = float(A_ref[i].abs().max())
        kfloor = 2.0 ** -(7 * planes - 1) * abs(float(os_[i])) * float(W64[i].abs().sum(-1).max())
        assert measured(f'i8 edge {name} planes {planes} GP {i} A (scale {scale:.3g}, max|A| {amax:.3g})', A[i], A_ref[i],
                        rtol=0.0, atol=2e-8 * scale + 1.2e-7 * amax + kfloor)
        assert measured(f'i8 edge {name} planes {planes} GP {i} mean', mean[i], mean_ref[i], rtol=0.0,
                        atol=3e-8 * scale * math.sqrt(M) + 3e-7 * float(mean_ref[i].abs().max())
                        + kfloor * float(m[i].abs().sum()))


# ---------------------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize('poison', ['x_row', 'Z_row', 'ls', 'os_nan', 'os_inf', 'W_rows'])
def test_i8_projection_propagates_non_finite_inputs(poison):
    """Contract: every output entry whose float64 reference is NaN / +-Inf is not finite (the whole affected GP may be),
    and the other GPs of the launch are bit-identical to a clean run.  GP 1 of 3 is poisoned: a NaN in one row of its x
    (per-GP x), in one inducing point, in one lengthscale, a NaN / Inf output scale, or NaN rows of W (what the whitening
    chain leaves for a Kzz that is not positive definite)."""
    _need_gpu()
    from nsgp import ops
    b, M, n, D = 3, 200, 300, 3
    Z, x, ls, os_, m, W64, Kzx = _case(b, M, n, D, 21, shared_x=False)
    c = lambda t: t.cuda()                                                                    # noqa: E731
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=torch.Generator().manual_seed(6))) + 0.3 * torch.eye(M)

    def run(Z, x, ls, os_, W64):
        out = ops.svgp_project(c(W64).float(), None, c(Lq), c(m), c(os_), base_add=1e-4, W64f=c(W64),
                               i8_inputs=(c(Z), c(x), c(ls), c(os_)))
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
    # float64 reference of the poisoned GP
    xd = xp[1].double()
    K1 = osp[1].double() * torch.exp(-0.5 * (((Zp[1].double().unsqueeze(1) - xd.unsqueeze(0)) / lsp[1].double()) ** 2).sum(-1))
    # A = W Kzx with W lower triangular (the reference's triangular solve): entry (m, j) is non-finite iff W[m, k] or Kzx[k, j]
    # is for some k <= m -- a plain W @ Kzx would also spread a NaN row of Kzx through the zeros above W's diagonal
    Wl = torch.tril(Wp[1])
    fin = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)                   # noqa: E731
    A1 = fin(Wl) @ fin(K1)
    reach = (torch.tril(torch.ones(M, M, dtype=F64)) @ (~torch.isfinite(K1)).double()) > 0
    A1[reach | (~torch.isfinite(Wl)).any(1, keepdim=True)] = float('nan')
    mean1 = A1.T @ m[1].double()
    var1 = osp[1].double() + 1e-4 + ((torch.tril(Lq[1]).double().T @ A1) ** 2).sum(0) - (A1 ** 2).sum(0)
    bad_A, bad_mean, bad_var = ~torch.isfinite(A1), ~torch.isfinite(mean1), ~torch.isfinite(var1)
    print(f'[measured] non-finite {poison}: reference non-finite entries A {int(bad_A.sum())}, mean {int(bad_mean.sum())}, '
          f'var {int(bad_var.sum())}; kernel non-finite A {int((~torch.isfinite(A[1])).sum())}, '
          f'mean {int((~torch.isfinite(mean[1])).sum())}, var {int((~torch.isfinite(var[1])).sum())}')
    assert bad_mean.any()                               # (the case does poison the output)
    assert not torch.isfinite(A[1][bad_A]).any()
    assert not torch.isfinite(mean[1][bad_mean]).any()
    assert not torch.isfinite(var[1][bad_var]).any()
    for i in (0, 2):                                    # the clean GPs of the same launches: bit for bit
        for got, ref in zip((A, C, mean, var), clean):
            assert torch.equal(got[i], ref[i]), (poison, i)


def test_nan_in_a_hidden_layer_reaches_the_elbo():
    """2-layer DeepGP, int8 projection in both layers: a NaN inducing point of the hidden layer leaves NaN rows in its W
    (the whitening chain) and a NaN row in its Kzx; the ELBO reaches them only through the int8 product (the KL term
    does not depend on Z), whose digit cutters must not turn them into finite digits."""
    _need_gpu()
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from test_gpu_dgp import _FixedEps, _build
    B, S, M, D = 128, 3, 64, 3
    model, _ = _build(1, D, M, 31)
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 1000))
    g = torch.Generator().manual_seed(32)
    x, y = torch.randn(B, D, generator=g).cuda(), torch.randn(B, generator=g).cuda()
    eps = [torch.randn(S, B, 2, generator=g)]
    model.train()
    with settings.whiten_matmul_i8(True), settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        elbo = mll(model(x), y)
        assert bool(torch.isfinite(elbo))
        with torch.no_grad():
            model.layers[0].variational_strategy.inducing_points[0, 5, 1] = float('nan')
        hid = model.layers[0](x)
        assert torch.isnan(hid.mean[..., 0]).all()
        elbo = mll(model(x), y)
    assert bool(torch.isnan(elbo)), float(elbo)


# ---------------------------------------------------------------------------------------------------- layer gradients
def test_i8_layer_values_and_gradients_match_the_oracle():
    """svgp_marginal with the int8 projection at the headline layer size (M = 1024, n = 4096, kappa(Kzz) ~ 1e6) against
    torch.autograd of oracle.svgp.svgp_marginal in float64: mean, variance and the gradients of x, Z, ls, os, m, Lq
    (per-tensor max-norm relative error).  The backward of this path reads the float32 Kzx the plane build wrote along
    (rounded from the float64 values) and the float32 rounding of W64."""
    _need_gpu()
    from nsgp.gp import settings
    from nsgp.svgp import svgp_marginal
    from oracle import svgp as OS
    g = torch.Generator().manual_seed(41)
    b, M, n, D = 2, 1024, 4096, 3
    x = torch.randn(n, D, generator=g)
    Z = 1.5 * torch.randn(b, M, D, generator=g)
    ls = torch.rand(b, D, generator=g) * 0.3 + 0.8
    os_ = torch.rand(b, generator=g) + 0.5
    m = torch.randn(b, M, generator=g)
    Lq = torch.tril(0.05 * torch.randn(b, M, M, generator=g)) + 0.5 * torch.eye(M)
    gm, gv = torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)
    leaves = [t.cuda().requires_grad_() for t in (x, Z, ls, os_, m, Lq)]
    with settings.whiten_matmul_i8(True):
        mean, var, _ = svgp_marginal(*leaves)
    ((mean * gm.cuda()).sum() + (var * gv.cuda()).sum()).backward()
    ref_leaves = [t.double().requires_grad_() for t in (x, Z, ls, os_, m, Lq)]
    xr, Zr, lsr, osr, mr, Lqr = ref_leaves
    p = dict(Z=Zr, lengthscale=lsr.unsqueeze(-2), outputscale=osr, m=mr, Lq=Lqr,
             mean=('constant', torch.zeros(b, 1, dtype=F64)))
    mean_r, var_r = OS.svgp_marginal(xr.unsqueeze(0).expand(b, n, D), p)
    ((mean_r * gm.double()).sum() + (var_r * gv.double()).sum()).backward()
    with torch.no_grad():
        from oracle import kernels
        Kzz = kernels.rbf_ard(Zr, Zr, lsr.unsqueeze(-2), osr) + 1e-4 * torch.eye(M, dtype=F64)
        ev = torch.linalg.eigvalsh(Kzz)
        print('kappa(Kzz + 1e-4 I):', ['%.3g' % float(k) for k in ev[:, -1] / ev[:, 0]])
    rel = lambda a, r: float((a.detach().cpu().double() - r.detach()).abs().max() / r.detach().abs().max())   # noqa: E731
    errs = {'mean': rel(mean, mean_r), 'var': rel(var, var_r)}
    for name, a, r in zip(('x', 'Z', 'ls', 'os', 'm', 'Lq'), leaves, ref_leaves):
        errs['grad ' + name] = rel(a.grad, torch.tril(r.grad) if name == 'Lq' else r.grad)
    print('[measured] i8 layer vs float64 oracle (max-norm relative):', {k: '%.3g' % v for k, v in errs.items()})
    assert errs['mean'] < I8_LAYER_VALUE_TOL and errs['var'] < I8_LAYER_VALUE_TOL, errs
    assert max(v for k, v in errs.items() if k.startswith('grad')) < I8_LAYER_GRAD_TOL, errs
