"""Whitened SVGP layer marginals as fused autograd nodes with hand-derived backward passes.

What gpytorch's VariationalStrategy.forward does per layer (driven by
models/dgps.py:48-51 through DeepGPLayer.__call__):

    Kzz = K(Z,Z) + jitter I ; L = chol(Kzz.double()) ; A = L^-1 Kzx (double, cast back)
    mean = A^T m (+ mu(x), added by the caller) ; var = kxx + 1e-4 + colsum(A o ((Lq Lq^T - I) A))

MI355X formulation (same math, no per-sample redundancy, everything on the matrix cores):
    W   = chol(Kzz)^-1              float64 potrf + trtri  -- parameter-only work, done ONCE per step
                                    for every layer of the model in one batched chain (WhitenFn)
    A   = W Kzx                     f32 MFMA GEMM, lower-triangular W skips half the K-tiles
    C   = Lq^T A                    f32 MFMA GEMM, upper-triangular operand
    var = base + colsum(C o C) - colsum(A o A)      reduced in the two GEMMs' epilogues (A, C not re-read)
The backward is 4 more (M x M x n) GEMMs per layer (SVGPLayerFn; the elementwise parts of Abar / Lqbar are
folded into a GEMM epilogue and an operand loader) + one batched M^3 Cholesky adjoint
(WhitenFn); every identity is checked against torch autograd of the oracle in tests/test_gpu_svgp.py.
"""
import weakref

import torch
from torch.autograd.function import once_differentiable

from . import ops
from .ops import GEMM_A_LOWER, GEMM_A_UPPER, GEMM_B_LOWER, GEMM_B_UPPER, GEMM_C_LOWER, GEMM_C_NOFILL, GEMM_C_HALFDIAG

VAR_JITTER = 1e-4          # data_data_covar.add_jitter(1e-4) in VariationalStrategy.forward

# The whitening adjoint wants the layers' float32 Wbar = tril(Abar Kzx^T) widened into one batched float64 buffer.  The
# split-K reduce of that product holds every element in a register, so it writes the float64 copy itself (ops.gemm, out64)
# and WhitenFn.backward's cast launch per layer goes.  The tests switch this off to compare both paths bit for bit.
_FUSE_WBAR64 = True


class _WbarSlots:
    """The batched float64 Wbar of one whitening chain, shared by WhitenFn.backward and the backward passes of the float32
    layers that consume its W.  A layer finds the chain through the float64 W it was handed (a view of the chain's batched
    result: its address names chain and group), writes its group's block and notes which gradient tensor the block
    mirrors; WhitenFn.backward skips the cast for a group whose incoming gradient is that very tensor, unmodified."""
    _by_w64 = weakref.WeakValueDictionary()           # address of a group's float64 W -> the chain's slots

    def __init__(self, W64, sizes):
        self.shape, self.device, self.sizes = tuple(W64.shape), W64.device, list(sizes)
        self.offs, self.buf, self.sent, off = {}, None, {}, 0
        for gi, b in enumerate(self.sizes):
            self.offs[W64[off:off + b].data_ptr()] = gi
            _WbarSlots._by_w64[W64[off:off + b].data_ptr()] = self
            off += b

    @staticmethod
    def find(W64f, W):
        """(slots, group) for a float32 layer on the float32 W of a chain, with that chain's float64 W64f; else None."""
        if W64f is None or W64f.dtype != torch.float64 or W.dtype != torch.float32:
            return None
        slots = _WbarSlots._by_w64.get(W64f.data_ptr())
        if slots is None or W64f.data_ptr() not in slots.offs:
            return None
        gi = slots.offs[W64f.data_ptr()]
        ok = tuple(W64f.shape) == (slots.sizes[gi], *slots.shape[1:]) and W64f.is_contiguous() and W64f.device == slots.device
        return (slots, gi) if ok else None

    def block(self, gi):
        if self.buf is None:
            self.buf = torch.empty(self.shape, dtype=torch.float64, device=self.device)
        off = sum(self.sizes[:gi])
        return self.buf[off:off + self.sizes[gi]]

    def mirrors(self, gi, g):
        return self.buf is not None and self.sent.get(gi) == (g.data_ptr(), g._version, tuple(g.shape))


def _wbar_product(slot, Abar, Kzx):
    """Wbar = tril(Abar Kzx^T); with a slot (see _WbarSlots) its float64 copy lands in the whitening chain's buffer."""
    if slot is None or not _FUSE_WBAR64 or Abar.dtype != torch.float32:
        return ops.gemm(Abar, Kzx, tb=True, flags=GEMM_C_LOWER)
    slots, gi = slot
    Wbar = ops.gemm(Abar, Kzx, tb=True, flags=GEMM_C_LOWER, out64=slots.block(gi))
    slots.sent[gi] = (Wbar.data_ptr(), Wbar._version, tuple(Wbar.shape))
    return Wbar


def _kernel_build(nu, x1, x2, ls, os_, **kw):
    """ops.rbf_build (nu None) or ops.matern_build: the stationary ARD kernel of a layer, chosen by its nu."""
    return ops.rbf_build(x1, x2, ls, os_, **kw) if nu is None else ops.matern_build(x1, x2, ls, os_, nu, **kw)


def _kernel_build_bwd(nu, x1, x2, ls, os_, G, **kw):
    """The backward of _kernel_build: ops.rbf_build_bwd or ops.matern_build_bwd."""
    return ops.rbf_build_bwd(x1, x2, ls, os_, G, **kw) if nu is None else ops.matern_build_bwd(x1, x2, ls, os_, nu, G, **kw)


def _check_nu(nu, what):
    if nu is not None and nu not in ops.MATERN_NU:
        raise ValueError(f'{what}: nu must be None (RBF) or one of {ops.MATERN_NU}, got {nu!r}')
    return None if nu is None else float(nu)


class WhitenFn(torch.autograd.Function):
    """W[g] = chol(os_g kappa_g(Z_g, Z_g; ls_g) + jitter I)^-1 in float64 for a list of GP groups; kappa_g is RBF, or Matern
    where the group's entry of `nu` is not None.

    inputs: jitter, chol_bwd_f64, out_dtype, nu (None or one entry per group), then (Z_i:(b_i,M,D_i), ls_i:(b_i,D_i),
    os_i:(b_i,)) per group, all with
    the same M.  Outputs: W64_i:(b_i, M, M) float64 per group, info:(sum b_i,), then the parameters again
    (Z_i, ls_i, os_i pass-throughs).  A layer that takes its kernel parameters from the pass-throughs sends its Kzx-path
    gradients back through this node, where they join the Kzz-path gradients in one multi-tensor add instead of six
    accumulation launches of the autograd engine.  The Gram matrices are built
    per group (the input dimension differs between layers), then ONE batched potrf + trtri chain
    factors them all; the adjoint  Kbar = -1/2 W^T (Phi(B) + Phi(B)^T) W,  B = tril(Wbar) W^T  is three
    batched MFMA GEMMs.
    """

    @staticmethod
    def forward(ctx, jitter, chol_bwd_f64, out_dtype, nu, *params):
        groups = [params[i:i + 3] for i in range(0, len(params), 3)]
        nu = tuple(nu) if nu is not None else (None,) * len(groups)
        z64, off = [], 0
        M = groups[0][0].shape[-2]
        K = torch.empty((sum(g[0].shape[0] for g in groups), M, M), dtype=torch.float64, device=groups[0][0].device)
        # float64 copies of all (small) parameters with ONE multi-tensor copy instead of a cast launch per tensor
        flat = [t for g in groups for t in g]
        if all(t.dtype == torch.float64 for t in flat):
            f64 = list(flat)
        else:
            f64 = [torch.empty(t.shape, dtype=torch.float64, device=t.device) for t in flat]
            torch._foreach_copy_(f64, [t.detach() for t in flat])
        for gi, (Z, ls, os_) in enumerate(groups):          # Gram matrices straight into the batched buffer
            Zd, lsd, osd = f64[3 * gi:3 * gi + 3]
            z64.append((Zd, lsd, osd))
            _kernel_build(nu[gi], Zd, Zd, lsd, osd, diag_add=jitter, out=K[off:off + Z.shape[0]])
            off += Z.shape[0]
        # K is consumed; the factor itself is never needed.  A float32 model also gets its float32 W from the same launches
        if out_dtype == torch.float32:
            W64, info, W32 = ops.potrf_trtri_(K, want_f32=True)
        else:
            (W64, info), W32 = ops.potrf_trtri_(K), None
        ctx.save_for_backward(W64, *[t for g in z64 for t in g])
        ctx.sizes = [g[0].shape[0] for g in groups]
        ctx.dtypes = [g[0].dtype for g in groups]
        ctx.chol_bwd_f64 = chol_bwd_f64
        ctx.nu = nu
        # float32 layers on a float64 chain: their Wbar products fill the adjoint's float64 buffer themselves
        ctx.wbar_slots = _WbarSlots(W64, ctx.sizes) if (out_dtype == torch.float32 and W64.dtype == torch.float64) else None
        ctx.mark_non_differentiable(info)
        ctx.set_materialize_grads(False)         # no zero-fill launches for outputs nobody differentiated
        # the layers consume W in their own dtype: ONE cast of the batched result here instead of one per layer
        Wout = W64 if out_dtype in (None, torch.float64) else (W32 if W32 is not None else ops.cast(W64, out_dtype))
        outs, outs64, off = [], [], 0
        for b in ctx.sizes:                      # one output per group (views of the batched result)
            outs.append(Wout[off:off + b])
            outs64.append(W64[off:off + b].detach() if Wout is not W64 else Wout[off:off + b].detach())
            off += b
        # the float64 W rides along (non-differentiable): a float32 layer accumulates A = W Kzx in float64 with it
        ctx.mark_non_differentiable(*outs64)
        return (*outs, info, *[t.view_as(t) for t in flat], *outs64)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        W64, *flat = ctx.saved_tensors
        ng = len(ctx.sizes)
        gpass = gouts[ng + 1:ng + 1 + 3 * ng]                # gradients that came in through the pass-throughs
        if ng == 1 and gouts[0] is not None and gouts[0].dtype == W64.dtype:
            Wbar = gouts[0]
        else:                                    # float64 batched Wbar: cast + placement in one multi-tensor copy
            slots = ctx.wbar_slots
            Wbar = slots.buf if (slots is not None and slots.buf is not None) else torch.empty_like(W64)
            dst, src, off = [], [], 0
            for gi, b in enumerate(ctx.sizes):
                if gouts[gi] is None:
                    Wbar[off:off + b].zero_()
                elif slots is not None and slots.mirrors(gi, gouts[gi]):
                    pass                                 # written by the layer's split-K reduce (_wbar_product)
                else:
                    dst.append(Wbar[off:off + b])
                    src.append(gouts[gi])
                off += b
            if dst and all(g.dtype == torch.float32 and g.is_cuda for g in src) and Wbar.dtype == torch.float64:
                for d_, s_ in zip(dst, src):             # one cast launch per layer: the multi-tensor copy of three 1024^2
                    ops.cast(s_, torch.float64, out=d_)  # matrices took 27 us (few, large tensors), these take 5 + 8
            elif dst:
                torch._foreach_copy_(dst, src)
            if slots is not None:
                slots.sent.clear()
        if ctx.chol_bwd_f64:
            Wb, Wc = Wbar.contiguous(), W64
        else:
            Wb, Wc = ops.cast(Wbar.contiguous(), torch.float32), ops.cast(W64, torch.float32)
        # Kbar = -1/2 W^T (Phi + Phi^T) W with Phi = tril(Wbar W^T), diagonal halved.  The kernel backward below sums the
        # row and the column side of its input (sym=True), i.e. it sees Kbar + Kbar^T only, so G = -W^T Phi W stands in for
        # Kbar (G + G^T = 2 Kbar): every product keeps its triangular structure -- lower triangle of a lower x upper
        # product, lower x lower (lower result), upper x lower -- 2/3 of a dense M^3 product in total instead of 4/3.
        # The strict upper triangles of Phi and Phi W are never written and never read (LOWER operand flags mask them).
        Phi = ops.gemm(Wb, Wc, tb=True, flags=GEMM_A_LOWER | GEMM_B_UPPER | GEMM_C_LOWER | GEMM_C_NOFILL | GEMM_C_HALFDIAG)
        T = ops.gemm(Phi, Wc, flags=GEMM_A_LOWER | GEMM_B_LOWER | GEMM_C_LOWER | GEMM_C_NOFILL)
        Kbar = ops.gemm(Wc, T, ta=True, alpha=-1.0, flags=GEMM_A_UPPER | GEMM_B_LOWER)
        grads, off = [None, None], 0
        for gi, b in enumerate(ctx.sizes):
            Zd, lsd, osd = flat[3 * gi:3 * gi + 3]
            Kb = Kbar[off:off + b]
            off += b
            if Kb.dtype != torch.float64:
                Zk, lsk, osk = Zd.float(), lsd.float(), osd.float()
            else:
                Zk, lsk, osk = Zd, lsd, osd
            gZ, _, gls, gos = _kernel_build_bwd(ctx.nu[gi], Zk, Zk, lsk, osk, Kb.contiguous(), sym=True)  # both sides summed
            grads += [gZ, gls, gos]
        # back to the parameters' dtypes with ONE multi-tensor copy
        outs = [g if g.dtype == ctx.dtypes[i // 3] else torch.empty(g.shape, dtype=ctx.dtypes[i // 3], device=g.device)
                for i, g in enumerate(grads[2:])]
        src = [g for g, o in zip(grads[2:], outs) if o is not g]
        dst = [o for g, o in zip(grads[2:], outs) if o is not g]
        if dst:
            torch._foreach_copy_(dst, src)
        extra = [(o, g) for o, g in zip(outs, gpass) if g is not None]
        if extra:
            torch._foreach_add_([o for o, _ in extra], [g.reshape(o.shape) for o, g in extra])
        return (None, None, None, None, *outs)


def whiten(groups, jitter=1e-4, chol_bwd_f64=True, passthrough=False, out_dtype=None, with_f64=False, nu=None):
    """groups: list of (Z:(b,M,D), ls:(b,D), os:(b,)).  Returns (list of W:(b,M,M) per group -- float64 unless
    `out_dtype` asks for the layers' dtype --, info); with
    passthrough=True also the list of (Z, ls, os) pass-through triples a layer should build its Kzx from (WhitenFn);
    with_f64=True appends the list of float64 W per group (non-differentiable companions of the float32 W: the forward
    projection of a float32 layer accumulates in float64 with them, settings.whiten_matmul_f64).
    nu: None (every group RBF) or one entry per group, None | 0.5 | 1.5 | 2.5 -- RBF and Matern groups share the chain."""
    flat = [t for g in groups for t in g]
    if nu is not None:
        if len(nu) != len(groups):
            raise ValueError(f'whiten: nu needs one entry per group ({len(groups)}), got {len(nu)}')
        nu = tuple(_check_nu(v, 'whiten') for v in nu)
        nu = nu if any(v is not None for v in nu) else None
    res = WhitenFn.apply(float(jitter), bool(chol_bwd_f64), out_dtype, nu, *flat)
    ng = len(groups)
    Ws, info, rest, W64s = res[:ng], res[ng], res[ng + 1:ng + 1 + 3 * ng], res[ng + 1 + 3 * ng:]
    from .gp import settings
    if settings.check_variational_cholesky.on():
        bad = info.nonzero()
        if bad.numel():                                   # host sync: debugging aid only
            from .gp.utils.cholesky import NotPSDError
            b = int(bad[0, 0])
            raise NotPSDError(f'Kzz + {jitter:g} I of GP {b} (of {info.numel()} in the whitening chain) is not positive '
                              f'definite: leading minor {int(info[b])} failed')
    out = [list(Ws), info]
    if passthrough:
        out.append([tuple(rest[3 * i:3 * i + 3]) for i in range(ng)])
    if with_f64:
        out.append(list(W64s))
    return tuple(out)


def select_projection(dtype, M, D, n, kzx_f64, has_w64, fusable, forward_precision, whiten_matmul_f64, whiten_matmul_i8,
                      fuse_kzx, hidden_var_f64, diag_q=False):
    """Which arithmetic a layer's forward projection runs in, from sizes and the settings' values only: (first, second) in
    ops.svgp_projection_plan's names, the int8 product's Kzx planes, whether it takes the float64 W.  kzx_f64: the layer
    feeds the next one (settings.hidden_kzx_f64); has_w64: the float64 W of the whitening chain is at hand; fusable: the
    generated-Kzx kernel supports the shape.
    A = W Kzx of a float32 layer with the float64 W (kept under whiten_matmul_f64, and by 'bf16_all' regardless):
     * fuse_kzx (wins over int8): Kzx never materialised in the forward pass, its tiles are generated inside the loader of
       the float64-accumulating product (whole tiles); the backward builds it once for Wbar = tril(Abar Kzx^T);
     * the exact int8 digit-plane product (whiten_matmul_i8; M <= 4096, D <= 4; wins over a float64 Kzx): four Kzx planes /
       14 plane products (1e-6 of max|A|), five / 19 for a layer that feeds the next one (A to float32 rounding);
     * int8 off: the float64-accumulating product on the float32 Kzx (round 2) -- on a float64 Kzx, which the forward then
       builds, for a layer that feeds the next one ('f64acc_b64').
    C = Lq^T A: float32, except for a layer that feeds the next one and sees at most 8192 points -- the first hidden layer
    of a deep GP (hidden_var_f64) -- where it accumulates in float64 on a float64 copy of Lq ('f64acc_t') with float64
    column-statistic partials: the variance os + colsum(C^2 - A^2) cancels to << os once q(u) has trained and reaches the
    next layer's inputs through sqrt(var) eps.  Measured after 1000 Adam steps at the headline shape (max-norm, vs the
    float64 oracle; tests/test_gpu_headline_precision.py): output mean 4.4e-6 with it, 5.2e-5 without (the reference's own
    float32 arithmetic: 4.5e-4); +0.12 ms on a 4.34 ms step.
    'bf16' (BASELINE configs[4]; float32 layers, M % 8 == 0, else as 'f32'): C on the bf16 cores; 'bf16_all' also A.
    diag_q: q(u) is mean-field (SVGPMeanFieldLayerFn).  There is no C, so its rules do not apply and `second` is 'diag';
    `first` and the planes are chosen as above."""
    fp = forward_precision
    w64 = dtype == torch.float32 and has_w64 and (whiten_matmul_f64 or fp == 'bf16_all')
    fuse = fp == 'f32' and fuse_kzx and w64 and fusable
    i8 = fp in ('f32', 'bf16') and not fuse and w64 and whiten_matmul_i8 and D <= 4 and M <= 4096
    can64 = kzx_f64 and fp == 'f32' and w64 and not fuse
    var64 = can64 and ((n <= 8192) if hidden_var_f64 == 'auto' else bool(hidden_var_f64))
    bf16 = dtype == torch.float32 and fp in ('bf16', 'bf16_all') and M % 8 == 0
    first = 'bf16' if (bf16 and fp == 'bf16_all') else 'kzx_fused' if fuse else 'i8' if i8 else \
        'f64acc_b64' if can64 else 'f64acc' if w64 else 'f32'
    second = 'diag' if diag_q else 'bf16' if bf16 else 'f64acc_t' if var64 else 'f32'
    return first, second, 5 if (kzx_f64 and not bf16) else 4, bool(w64)


def _forward_precision_for(nu):
    """forward_precision('bf16_all') writes Kxz with the RBF-only bf16 build and exists to time BASELINE configs[4]: a
    Matern layer under it is an error, not a quiet downgrade that would falsify the timing."""
    from .gp import settings
    if nu is not None and settings.forward_precision.value() == 'bf16_all':
        raise NotImplementedError("forward_precision('bf16_all') times the RBF-only bf16 Kxz build: a Matern layer "
                                  f"(nu={nu}) takes 'f32' or 'bf16'")


class SVGPLayerFn(torch.autograd.Function):
    """(x, Z, ls, os, m, Lq, W64, mean_w, mean_c) -> (mean:(b,n), var:(b,n))

    x:(n,D) shared by the b output GPs, or (b,n,D);  Z:(b,M,D)  ls:(b,D)  os:(b,)  m:(b,M)  Lq:(b,M,M)
    (only the lower triangle of Lq is used, like CholeskyVariationalDistribution.forward);
    W64:(b,M,M) = chol(Kzz)^-1 from WhitenFn (float64, or already in x's dtype).  The dependence of Kzz on (Z, ls, os) flows
    through W64's gradient; this node differentiates the Kzx path.
    mean_w:(D,) or (b,D) and mean_c:(1,) or (b,) are the weights / constant of an affine prior mean function
    (gpytorch LinearMean / ConstantMean, models/dgps.py:40-43); either may be None.  The prior mean is added in the
    kernel that assembles the column statistics and its gradients come out of the `rowdot` launch of the backward,
    so the mean module costs no launches of its own.
    """

    @staticmethod
    def forward(ctx, x, Z, ls, os_, m, Lq, W64, mean_w, mean_c, W64f=None, kzx_f64=False, nu=None):
        from .gp import settings
        _forward_precision_for(nu)
        W = W64 if W64.dtype == x.dtype else ops.cast(W64, x.dtype)
        if W64f is None and W64.dtype == torch.float64 and x.dtype == torch.float32:
            W64f = W64
        first, second, planes, w64 = select_projection(
            x.dtype, Z.shape[-2], Z.shape[-1], x.shape[-2], kzx_f64, W64f is not None,
            nu is None and settings.fuse_kzx.on() and ops.svgp_kzx_fusable(W64f, Z, x, x.shape[-2]),
            settings.forward_precision.value(),
            settings.whiten_matmul_f64.on(), settings.whiten_matmul_i8.on(), settings.fuse_kzx.on(), settings.hidden_var_f64.value())
        W64f = W64f if w64 else None
        affine = None if (mean_w is None and mean_c is None) else (x, mean_w, mean_c)
        Kzx = Kzx64 = Lq64 = None
        if first == 'f64acc_b64':
            src = [x.detach(), Z.detach(), ls.detach(), os_.detach()] + ([Lq.detach()] if second == 'f64acc_t' else [])
            dst = [torch.empty(t.shape, dtype=torch.float64, device=t.device) for t in src]
            torch._foreach_copy_(dst, src)
            Kzx64 = _kernel_build(nu, dst[1], dst[0], dst[2], dst[3])
            Lq64 = dst[4] if len(dst) == 5 else None
        elif second == 'f64acc_t':
            Lq64 = ops.cast(Lq.detach(), torch.float64)
        elif first in ('f32', 'f64acc', 'bf16'):       # ('bf16' builds its own bf16 Kxz; it takes this one's shape)
            Kzx = _kernel_build(nu, Z, x, ls, os_)       # (b,M,n)
        # int8 path: the plane-build kernel also writes the float32 Kzx the BACKWARD needs (Wbar = tril(Abar Kzx^T)) when there
        # is going to be one -- its own build launch (28 us at the headline's last layer) disappears
        kin = (Z, x, ls, os_)
        i8 = dict(i8_inputs=kin, i8_kzx_out=[] if any(ctx.needs_input_grad) else None, kernel_nu=nu) if first == 'i8' else {}
        if second == 'bf16':
            A, C, mean, var = ops.svgp_project_bf16(W, Kzx, Lq, m, os_, base_add=VAR_JITTER, affine=affine, W64f=W64f,
                                                    kernel_inputs=kin if first == 'bf16' else None, **i8)
        else:
            A, C, mean, var = ops.svgp_project(W, Kzx, Lq, m, os_, base_add=VAR_JITTER, affine=affine, W64f=W64f,
                                               kernel_inputs=kin if first == 'kzx_fused' else None, Kzx64=Kzx64,
                                               Lq64=Lq64, i8_planes=planes, **i8)                    # 2 GEMMs
        if i8.get('i8_kzx_out'):
            Kzx = i8['i8_kzx_out'][0]
        ctx.save_for_backward(x, Z, ls, os_, m, Lq, W, Kzx, A, C, mean_w, mean_c)
        ctx.w_dtype = W64.dtype
        ctx.nu = nu
        ctx.wbar_slot = _WbarSlots.find(W64f, W64)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        x, Z, ls, os_, m, Lq, W, Kzx, A, C, mean_w, mean_c = ctx.saved_tensors
        if Kzx is None:                                  # fused / float64-Kzx forward: built here, once, for the Wbar product
            Kzx = _kernel_build(ctx.nu, Z, x, ls, os_)
        gmean = gmean.contiguous()
        affine = None if (mean_w is None and mean_c is None) else (x, mean_w, mean_c)
        Abar, Lqbar, mbar, basebar, wbar, cbar = ops.svgp_project_bwd(Lq, m, A, C, gmean, gvar.contiguous(),
                                                                      affine=affine)
        Kzxbar = ops.gemm(W, Abar, ta=True, flags=GEMM_A_UPPER)                  # W^T Abar
        Wbar = _wbar_product(ctx.wbar_slot, Abar, Kzx)                           # tril(Abar Kzx^T)
        need_x = ctx.needs_input_grad[0]
        gZ, gx, gls, gos = _kernel_build_bwd(ctx.nu, Z, x, ls, os_, Kzxbar, need_x1=True, need_x2=need_x)
        gos = gos + basebar
        if need_x:
            if mean_w is not None:                       # d(prior mean)/dx = w  (deeper layers of a tied stack only)
                gx = gx + gmean.unsqueeze(-1) * mean_w.reshape(-1, 1, x.shape[-1])
            if x.dim() == 2:
                gx = gx[0] if gx.shape[0] == 1 else gx.sum(0)
        return (gx if need_x else None, gZ, gls.reshape(ls.shape), gos.reshape(os_.shape), mbar, Lqbar,
                Wbar if Wbar.dtype == ctx.w_dtype else ops.cast(Wbar, ctx.w_dtype),
                None if mean_w is None else wbar.reshape(mean_w.shape),
                None if mean_c is None else cbar.reshape(mean_c.shape), None, None, None)


class SVGPMeanFieldLayerFn(torch.autograd.Function):
    """(x, Z, ls, os, m, s2, W64, mean_w, mean_c) -> (mean:(b,n), var:(b,n)) for a mean-field q(u) = N(m, diag(s2)).

    SVGPLayerFn with s2:(b,M), the variances of q(u), in place of Lq.  S = diag(s2) leaves ONE (M x M x n) product in the
    forward pass (A = W Kzx, in whichever arithmetic select_projection names) and two in the backward:
        var_j = os + 1e-4 + sum_k (s2_k - 1) A_kj^2             one pass over A, summed in float64
        Abar  = m gmean^T + 2 diag(s2 - 1) A diag(gvar),  s2bar_k = sum_j A_kj^2 gvar_j,  mbar = A gmean     one pass over A
        Kzxbar = W^T Abar,  Wbar = tril(Abar Kzx^T)             as in SVGPLayerFn
    The Kzx handling is SVGPLayerFn's: the int8 build writes the float32 Kzx the backward needs, the generated-Kzx and
    float64-Kzx forward passes leave it to the backward to build."""

    @staticmethod
    def forward(ctx, x, Z, ls, os_, m, s2, W64, mean_w, mean_c, W64f=None, kzx_f64=False, nu=None):
        from .gp import settings
        _forward_precision_for(nu)
        W = W64 if W64.dtype == x.dtype else ops.cast(W64, x.dtype)
        if W64f is None and W64.dtype == torch.float64 and x.dtype == torch.float32:
            W64f = W64
        first, _, planes, w64 = select_projection(
            x.dtype, Z.shape[-2], Z.shape[-1], x.shape[-2], kzx_f64, W64f is not None,
            nu is None and settings.fuse_kzx.on() and ops.svgp_kzx_fusable(W64f, Z, x, x.shape[-2]),
            settings.forward_precision.value(),
            settings.whiten_matmul_f64.on(), settings.whiten_matmul_i8.on(), settings.fuse_kzx.on(), settings.hidden_var_f64.value(),
            diag_q=True)
        W64f = W64f if w64 else None
        affine = None if (mean_w is None and mean_c is None) else (x, mean_w, mean_c)
        Kzx = Kzx64 = None
        if first == 'f64acc_b64':
            src = [x.detach(), Z.detach(), ls.detach(), os_.detach()]
            dst = [torch.empty(t.shape, dtype=torch.float64, device=t.device) for t in src]
            torch._foreach_copy_(dst, src)
            Kzx64 = _kernel_build(nu, dst[1], dst[0], dst[2], dst[3])
        elif first in ('f32', 'f64acc'):
            Kzx = _kernel_build(nu, Z, x, ls, os_)       # (b,M,n)
        kzx_out = [] if (first == 'i8' and any(ctx.needs_input_grad)) else None
        s2m1 = s2.detach() - 1.0
        A, mean, var = ops.svgp_project_diag(first, W, s2m1, m, os_, base_add=VAR_JITTER, affine=affine, Kzx=Kzx, Kzx64=Kzx64,
                                             kernel_inputs=(Z, x, ls, os_) if first in ('kzx_fused', 'i8', 'bf16') else None,
                                             W64f=W64f, i8_planes=planes, i8_kzx_out=kzx_out,
                                             kernel_nu=nu if first == 'i8' else None)
        if kzx_out:
            Kzx = kzx_out[0]
        ctx.save_for_backward(x, Z, ls, os_, m, s2m1, W, Kzx, A, mean_w, mean_c)
        ctx.w_dtype = W64.dtype
        ctx.nu = nu
        ctx.wbar_slot = _WbarSlots.find(W64f, W64)
        return mean, var

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        x, Z, ls, os_, m, s2m1, W, Kzx, A, mean_w, mean_c = ctx.saved_tensors
        if Kzx is None:                                  # built here, once, for the Wbar product
            Kzx = _kernel_build(ctx.nu, Z, x, ls, os_)
        gmean = gmean.contiguous()
        affine = None if (mean_w is None and mean_c is None) else (x, mean_w, mean_c)
        Abar, mbar, s2bar, basebar, wbar, cbar = ops.svgp_project_diag_bwd(m, s2m1, A, gmean, gvar.contiguous(), affine=affine)
        Kzxbar = ops.gemm(W, Abar, ta=True, flags=GEMM_A_UPPER)                  # W^T Abar
        Wbar = _wbar_product(ctx.wbar_slot, Abar, Kzx)                           # tril(Abar Kzx^T)
        need_x = ctx.needs_input_grad[0]
        gZ, gx, gls, gos = _kernel_build_bwd(ctx.nu, Z, x, ls, os_, Kzxbar, need_x1=True, need_x2=need_x)
        gos = gos + basebar
        if need_x:
            if mean_w is not None:                       # d(prior mean)/dx = w  (deeper layers of a tied stack only)
                gx = gx + gmean.unsqueeze(-1) * mean_w.reshape(-1, 1, x.shape[-1])
            if x.dim() == 2:
                gx = gx[0] if gx.shape[0] == 1 else gx.sum(0)
        return (gx if need_x else None, gZ, gls.reshape(ls.shape), gos.reshape(os_.shape), mbar, s2bar,
                Wbar if Wbar.dtype == ctx.w_dtype else ops.cast(Wbar, ctx.w_dtype),
                None if mean_w is None else wbar.reshape(mean_w.shape),
                None if mean_c is None else cbar.reshape(mean_c.shape), None, None, None)


def svgp_marginal(x, Z, ls, os_, m, Lq=None, jitter=1e-4, chol_bwd_f64=True, W64=None, mean_w=None, mean_c=None, W64f=None,
                  kzx_f64=False, s2=None, nu=None):
    """mean and variance of q(f) at x for b whitened SVGPs; the mean excludes the prior mean function unless its
    affine parameters are passed (mean_w: LinearMean weights (D,) / (b,D), mean_c: constant or bias (1,) / (b,)).
    q(u) = N(m, Lq Lq^T), or mean-field N(m, diag(s2)) when s2:(b,M) is given in place of Lq.
    nu: None for the RBF kernel, or 0.5 | 1.5 | 2.5 for Matern (with W64 given, the nu that chain was whitened with).
    Returns (mean, var, info); pass W64 (from `whiten`) to share one factorisation chain across layers."""
    nu = _check_nu(nu, 'svgp_marginal')
    if (Lq is None) == (s2 is None):
        raise ValueError('svgp_marginal: exactly one of Lq (Cholesky q(u)) and s2 (mean-field q(u)) expected')
    info = None
    if W64 is None:
        (W64,), info, ((Z, ls, os_),), (W64f,) = whiten([(Z, ls, os_)], jitter, chol_bwd_f64, passthrough=True,
                                                        out_dtype=x.dtype, with_f64=True, nu=[nu])
    if s2 is not None:
        mean, var = SVGPMeanFieldLayerFn.apply(x, Z, ls, os_, m, s2, W64, mean_w, mean_c, W64f, kzx_f64, nu)
    else:
        mean, var = SVGPLayerFn.apply(x, Z, ls, os_, m, Lq, W64, mean_w, mean_c, W64f, kzx_f64, nu)
    return mean, var, info
