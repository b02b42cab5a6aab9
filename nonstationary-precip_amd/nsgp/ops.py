"""Device ops: thin, checked wrappers over the C ABI (include/nsgp.h) + torch.autograd.Functions.

Every function here requires CUDA (ROCm) tensors and runs a hand-written gfx950 kernel on torch's
current stream; torch only owns memory, streams and the autograd graph edges.  There is no CPU or
eager fallback: a CPU tensor or a missing library raises `BackendError`.

Raw ops (no autograd) are lower-case functions returning new tensors; autograd entry points are the
`*Fn` classes and the lower-case convenience wrappers at the bottom (`gibbs_kernel`, `rbf_kernel`,
`matern_kernel`, `ps2d_kernel`, `matmul`, `chol_inv`, ...).
"""
import ctypes
import functools
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import BackendError

GEMM_A_LOWER, GEMM_A_UPPER, GEMM_B_LOWER, GEMM_B_UPPER, GEMM_C_LOWER, GEMM_NO_SPLITK, GEMM_C_NOFILL = 1, 2, 4, 8, 16, 32, 64
GEMM_C_HALFDIAG = 128


# --------------------------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sfx(t):
    if t.dtype == torch.float32:
        return 'f32'
    if t.dtype == torch.float64:
        return 'f64'
    raise BackendError(f'nsgp kernels compute in float32/float64, got {t.dtype}')


def _chk(*ts):
    """All tensors on the same CUDA device, same floating dtype."""
    first = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise BackendError('nsgp ops need CUDA (ROCm) tensors: the HIP backend is the only backend '
                               '(no CPU fallback).  Move the model/data to the GPU.')
        if first is None:
            first = t
        elif t.dtype != first.dtype or t.device != first.device:
            raise BackendError(f'mixed dtype/device: {t.dtype}/{t.device} vs {first.dtype}/{first.device}')
    _sfx(first)
    if first.device.index != torch.cuda.current_device():
        # every wrapper launches on torch.cuda.current_stream() of the CURRENT device: device-1 pointers on device 0's
        # stream would be a GPU memory fault, not an error code
        raise BackendError(f'tensors live on {first.device} but the current device is cuda:{torch.cuda.current_device()}: '
                           'call torch.cuda.set_device(...) (one process per GPU) or wrap the call in torch.cuda.device(...)')
    return first


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


# --------------------------------------------------------------------------------------------
# Gradient sinks: where a large parameter's gradient should be WRITTEN (the flat gradient bucket of nsgp.optim.FlatBucket)
# instead of being handed to autograd in a fresh buffer and copied there afterwards.  A backward kernel that produces the
# gradient of a registered parameter asks `grad_sink(t)` (t: the parameter as the node received it -- same storage):
#   * (view, False): nothing is in place yet -> write the gradient into `view` and RETURN `view` as the gradient (autograd's
#     AccumulateGrad adopts it as p.grad: the bucket is filled without a copy);
#   * (view, True):  the view already holds a term of this gradient (the KL term, an earlier application of a tied layer,
#     or -- gradient accumulation over several backward passes -- p.grad itself) -> ACCUMULATE into `view` and return
#     None for that input.
# "Already holds a term" cannot be read off p.grad inside one backward pass (the engine sums the incoming gradients of a leaf
# in its input buffer and sets p.grad only after the LAST of them), so a sink remembers the autograd graph task that wrote
# it first; across passes p.grad decides, so any way of clearing gradients is safe.
# --------------------------------------------------------------------------------------------
_grad_sinks = {}
_grad_sinks_on = True


class grad_sinks:
    """Context manager / switch: `with ops.grad_sinks(False): ...` makes every backward pass inside hand its gradients
    over in fresh buffers, as plain torch does.  Needed when gradients are taken with `torch.autograd.grad` (or kept across
    `zero_grad()`): a sink's gradient IS a view of the optimiser's flat gradient bucket, so the next backward pass would
    overwrite a tensor the caller still holds.  (Inside an ordinary `loss.backward()` the view becomes `p.grad` and the
    aliasing is the point: the bucket is filled without a copy.)"""

    def __init__(self, enabled):
        self.enabled, self.prev = bool(enabled), None

    def __enter__(self):
        global _grad_sinks_on
        self.prev, _grad_sinks_on = _grad_sinks_on, self.enabled
        return self

    def __exit__(self, *exc):
        global _grad_sinks_on
        _grad_sinks_on = self.prev
        return False


class _GradSink:
    def __init__(self, param, flat_g, off):
        import weakref
        self.param = weakref.ref(param)
        self.flat_g, self.off, self.numel, self.shape = flat_g, int(off), param.numel(), tuple(param.shape)
        self.task = None                                  # id of the backward pass (graph task) that wrote first

    def view(self):
        return self.flat_g[self.off:self.off + self.numel].view(self.shape)


def register_grad_sink(param, flat_g, off):
    _grad_sinks[param.data_ptr()] = _GradSink(param, flat_g, off)


def unregister_grad_sinks(flat_g):
    for k in [k for k, v in _grad_sinks.items() if v.flat_g is flat_g]:
        del _grad_sinks[k]


def grad_sink(t):
    """(view shaped like t, accumulate) for a tensor that IS a registered parameter (same storage, same number of
    elements, contiguous) inside a backward pass, else None."""
    s = _grad_sinks.get(t.data_ptr()) if _grad_sinks_on else None
    if s is None:
        return None
    task = torch._C._current_graph_task_id()
    p = s.param()
    if task < 0 or p is None or p.data_ptr() != t.data_ptr() or t.numel() != s.numel or not t.is_contiguous() \
            or t.dtype != s.flat_g.dtype or t.device != s.flat_g.device:
        return None
    v = s.view()
    if p.grad is not None:
        if p.grad.data_ptr() != v.data_ptr():
            return None                               # something else owns p.grad: the ordinary path accumulates into it
        s.task = task
        return v.view(t.shape), True                  # an earlier pass (or stage) left its gradient in the view
    if s.task == task:
        return v.view(t.shape), True                  # an earlier node of THIS pass wrote the view
    s.task = task
    return v.view(t.shape), False


def _scalar_dev(v, like):
    """Host number or tensor -> 1-element device tensor of like's dtype (no sync)."""
    if torch.is_tensor(v):
        return v.detach().reshape(1).to(device=like.device, dtype=like.dtype)
    return torch.full((1,), float(v), dtype=like.dtype, device=like.device)


# --------------------------------------------------------------------------------------------
# K1 Gibbs, K1' its Matern form
# --------------------------------------------------------------------------------------------
MATERN_NU = (0.5, 1.5, 2.5)


def _gibbs_args(x1, x2, ell1, ell2):
    ref = _chk(x1, x2, ell1, ell2)
    if x1.dim() != 2 or x2.dim() != 2 or ell1.dim() != 2 or ell2.dim() != 2:
        raise BackendError('gibbs_build: x:(n,D), ell:(D,n) expected')
    n1, D = x1.shape
    n2 = x2.shape[0]
    if x2.shape[1] != D or ell1.shape != (D, n1) or ell2.shape != (D, n2):
        raise BackendError(f'gibbs_build: shape mismatch x1{tuple(x1.shape)} x2{tuple(x2.shape)} '
                           f'ell1{tuple(ell1.shape)} ell2{tuple(ell2.shape)}')
    return ref, n1, n2, D


def _out_matrix(out, shape, ref):
    """Validate a caller-provided contiguous output buffer (or allocate one)."""
    if out is None:
        return torch.empty(shape, dtype=ref.dtype, device=ref.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != ref.dtype or out.device != ref.device \
            or not out.is_contiguous():
        raise BackendError(f'out: contiguous {tuple(shape)} {ref.dtype} tensor on {ref.device} expected')
    return out


def _gibbs_entry(nu):
    """(library stem, the scalars its entry points take after D) of the Gibbs build: nu = None is the squared-exponential
    kernel, nu in {0.5, 1.5, 2.5} its Matern form (K1', nu2 = 2 nu).  Any other value raises as gpytorch's MaternKernel."""
    if nu is None:
        return 'gibbs', ()
    if nu not in MATERN_NU:
        raise RuntimeError('nu expected to be 0.5, 1.5, or 2.5')
    return 'gibbs_matern', (int(2 * nu),)


def gibbs_build(x1, x2, ell1, ell2, outputscale=None, diag_add=None, out=None, nu=None):
    """K = os * Gibbs(x1,x2; ell1,ell2) (+ diag_add on the diagonal).  models/gibbs_kernels.py:154-162.
    nu in {0.5, 1.5, 2.5}: the non-stationary Matern kernel os * P * Matern_nu(sqrt(2 sum_d delta_d^2 / s_d)) with the
    same prefactor P (include/nsgp.h, K1')."""
    stem, extra = _gibbs_entry(nu)
    ref, n1, n2, D = _gibbs_args(x1, x2, ell1, ell2)
    x1, x2, ell1, ell2 = _c(x1), _c(x2), _c(ell1), _c(ell2)
    os_ = None if outputscale is None else _scalar_dev(outputscale, ref)
    da = None if diag_add is None else _scalar_dev(diag_add, ref)
    K = _out_matrix(out, (n1, n2), ref)
    _lib.call(f'nsgp_{stem}_build_fwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ell1), _p(ell2), n1, n2, D, *extra,
              _p(os_), _p(da), _p(K), n2, _stream())
    return K


def gibbs_build_bwd(x1, x2, ell1, ell2, outputscale, G, need_x=False, need_os=True, nu=None):
    stem, extra = _gibbs_entry(nu)
    ref, n1, n2, D = _gibbs_args(x1, x2, ell1, ell2)
    _chk(ref, G)
    if G.shape != (n1, n2):
        raise BackendError('gibbs_build_bwd: G shape')
    x1, x2, ell1, ell2, G = _c(x1), _c(x2), _c(ell1), _c(ell2), _c(G)
    os_ = None if outputscale is None else _scalar_dev(outputscale, ref)
    g_l1, g_l2 = torch.empty_like(ell1), torch.empty_like(ell2)
    g_x1 = torch.empty_like(x1) if need_x else None
    g_x2 = torch.empty_like(x2) if need_x else None
    g_os = torch.empty(1, dtype=ref.dtype, device=ref.device) if need_os else None
    lib = _lib.load()
    wsb = lib.nsgp_gibbs_build_bwd_workspace(n1, n2, D, ref.element_size())
    ws = _ws(wsb, ref.device)
    _lib.call(f'nsgp_{stem}_build_bwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ell1), _p(ell2), n1, n2, D, *extra, _p(os_),
              _p(G), n2, _p(g_l1), _p(g_l2), _p(g_x1), _p(g_x2), _p(g_os), _p(ws), ws.numel(), _stream())
    return g_l1, g_l2, g_x1, g_x2, g_os


# --------------------------------------------------------------------------------------------
# K2 RBF-ARD (batched)
# --------------------------------------------------------------------------------------------
def _shared_or_batched(x, batch, D, what):
    """x:(n,D) shared by the batch or (batch,n,D) -> (contiguous x, n, its batch stride in elements: 0 when shared)."""
    if x.dim() == 2:
        if x.shape[1] != D:
            raise BackendError(f'{what}: x last dim != D')
        return _c(x), x.shape[0], 0
    if x.dim() == 3 and x.shape[0] == batch and x.shape[2] == D:
        x = _c(x)
        return x, x.shape[1], x.shape[1] * D
    raise BackendError(f'{what}: x shape {tuple(x.shape)} vs batch {batch}, D {D}')


def _rbf_args(x1, x2, ls, os_, what):
    ref = _chk(x1, x2, ls, os_)
    if ls.dim() == 1:
        ls = ls.unsqueeze(0)
    os_ = os_.reshape(-1)
    batch, D = ls.shape
    if os_.shape[0] != batch:
        raise BackendError(f'{what}: os must be (batch,)')
    x1, n1, sx1 = _shared_or_batched(x1, batch, D, what)
    x2, n2, sx2 = _shared_or_batched(x2, batch, D, what)
    return ref, x1, x2, _c(ls), _c(os_), batch, n1, n2, D, sx1, sx2


# The stationary ARD family K[b] = os[b] * kappa(|(x1-x2)/ls[b]|) shares its argument rules, allocation and call shape;
# a member is its library stem (nsgp_<stem>_build_fwd/_bwd_*) plus the extra scalar arguments its entry points take
# after sx2 (Matern: nu2).
def _ard_build(stem, extra, x1, x2, ls, os_, diag_add, out):
    ref, x1, x2, ls, os_, batch, n1, n2, D, sx1, sx2 = _rbf_args(x1, x2, ls, os_, f'{stem}_build')
    K = _out_matrix(out, (batch, n1, n2), ref)
    _lib.call(f'nsgp_{stem}_build_fwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls), _p(os_), batch, n1, n2, D, sx1, sx2, *extra,
              float(diag_add), _p(K), n2, n1 * n2, _stream())
    return K


def _ard_build_bwd(stem, extra, x1, x2, ls, os_, G, need_x1, need_x2, sym):
    what = f'{stem}_build_bwd'
    ref, x1, x2, ls, os_, batch, n1, n2, D, sx1, sx2 = _rbf_args(x1, x2, ls, os_, what)
    _chk(ref, G)
    G = _c(G).reshape(batch, n1, n2)
    g_x1 = torch.empty((batch, n1, D), dtype=ref.dtype, device=ref.device) if need_x1 else None
    g_x2 = torch.empty((batch, n2, D), dtype=ref.dtype, device=ref.device) if need_x2 else None
    if sym:
        if n1 != n2 or sx1 != sx2 or not (need_x1 and need_x2):
            raise BackendError(f'{what}: sym needs x1 and x2 of one shape and both gradients')
        g_x2 = g_x1
    g_ls = torch.empty((batch, D), dtype=ref.dtype, device=ref.device)
    g_os = torch.empty((batch,), dtype=ref.dtype, device=ref.device)
    workspace = getattr(_lib.load(), f'nsgp_{stem}_build_bwd_workspace')
    ws = _ws(workspace(batch, n1, n2, D, ref.element_size()), ref.device)
    _lib.call(f'nsgp_{stem}_build_bwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls), _p(os_), batch, n1, n2, D, sx1, sx2, *extra,
              _p(G), n2, n1 * n2, _p(g_x1), _p(g_x2), _p(g_ls), _p(g_os), _p(ws), ws.numel(), _stream())
    return g_x1, g_x2, g_ls, g_os


def rbf_build(x1, x2, ls, os_, diag_add=0.0, out=None):
    """K[b] = os[b] * exp(-0.5 |(x1-x2)/ls[b]|^2) (+diag_add I).  x:(n,D) shared or (batch,n,D)."""
    return _ard_build('rbf', (), x1, x2, ls, os_, diag_add, out)


def rbf_build_bwd(x1, x2, ls, os_, G, need_x1=True, need_x2=True, sym=False):
    """Returns g_x1:(batch,n1,D) g_x2:(batch,n2,D) (per-batch, caller sums if x was shared) g_ls, g_os.
    sym=True (x1 is x2, the Kzz case): ONE buffer receives the sum of the row- and column-side gradients and is
    returned for both."""
    return _ard_build_bwd('rbf', (), x1, x2, ls, os_, G, need_x1, need_x2, sym)


# --------------------------------------------------------------------------------------------
# K2'' Matern-ARD (batched), nu in {1/2, 3/2, 5/2}
# --------------------------------------------------------------------------------------------
def _nu2(nu):
    if nu not in MATERN_NU:
        raise BackendError(f'matern_build: nu must be one of {MATERN_NU}, got {nu}')
    return int(2 * nu)


def matern_build(x1, x2, ls, os_, nu, diag_add=0.0, out=None):
    """K[b] = os[b] * Matern_nu(|(x1-x2)/ls[b]|) (+diag_add I).  Arguments and batching as rbf_build."""
    return _ard_build('matern', (_nu2(nu),), x1, x2, ls, os_, diag_add, out)


def matern_build_bwd(x1, x2, ls, os_, nu, G, need_x1=True, need_x2=True, sym=False):
    """As rbf_build_bwd: g_x1:(batch,n1,D) g_x2:(batch,n2,D) per batch, g_ls:(batch,D), g_os:(batch,); sym=True sums
    both sides into one buffer.  For nu = 1/2 the derivative at zero distance is taken as 0."""
    return _ard_build_bwd('matern', (_nu2(nu),), x1, x2, ls, os_, G, need_x1, need_x2, sym)


# --------------------------------------------------------------------------------------------
# K2' RBF-ARD x Periodic (one launch)
# --------------------------------------------------------------------------------------------
def _rbfper_args(x1, x2, ls_rbf, ls_per, period, os_, what='rbf_periodic_build', env='ls_rbf'):
    """The periodic family's argument rules; `what` and `env` name the op and its envelope lengthscale in the errors."""
    ref = _chk(x1, x2, ls_rbf, ls_per, period, os_)
    ls_per, period = _c(ls_per.reshape(-1)), _c(period.reshape(-1))
    batch = ls_per.shape[0]
    if period.shape[0] != batch:
        raise BackendError(f'{what}: ls_per and period must be (batch,)')
    D = x1.shape[-1]
    if ls_rbf is not None:
        ls_rbf = _c(ls_rbf.reshape(batch, -1))
        if ls_rbf.shape[1] != D:
            raise BackendError(f'{what}: {env} must be (batch, D)')
    if os_ is not None:
        os_ = _c(os_.reshape(-1))
        if os_.shape[0] != batch:
            raise BackendError(f'{what}: os must be (batch,)')
    x1, n1, sx1 = _shared_or_batched(x1, batch, D, what)
    x2, n2, sx2 = _shared_or_batched(x2, batch, D, what)
    return ref, x1, x2, ls_rbf, ls_per, period, os_, batch, n1, n2, D, sx1, sx2


def rbf_periodic_build(x1, x2, ls_rbf, ls_per, period, os_, diag_add=0.0):
    """K[b] = os[b] RBF-ARD(x; ls_rbf[b]) Periodic(x; ls_per[b], period[b]); ls_rbf / os_ may be None."""
    ref, x1, x2, ls_rbf, ls_per, period, os_, batch, n1, n2, D, sx1, sx2 = _rbfper_args(x1, x2, ls_rbf, ls_per,
                                                                                       period, os_)
    K = torch.empty((batch, n1, n2), dtype=ref.dtype, device=ref.device)
    _lib.call(f'nsgp_rbf_periodic_build_fwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls_rbf), _p(ls_per), _p(period), _p(os_),
              batch, n1, n2, D, sx1, sx2, float(diag_add), _p(K), n2, n1 * n2, _stream())
    return K


def rbf_periodic_build_bwd(x1, x2, ls_rbf, ls_per, period, os_, G, need_x1=True, need_x2=True):
    ref, x1, x2, ls_rbf, ls_per, period, os_, batch, n1, n2, D, sx1, sx2 = _rbfper_args(x1, x2, ls_rbf, ls_per,
                                                                                       period, os_)
    _chk(ref, G)
    G = _c(G).reshape(batch, n1, n2)
    new = lambda *shp: torch.empty(shp, dtype=ref.dtype, device=ref.device)
    g_x1 = new(batch, n1, D) if need_x1 else None
    g_x2 = new(batch, n2, D) if need_x2 else None
    g_lr = new(batch, D) if ls_rbf is not None else None
    g_lp, g_pe = new(batch), new(batch)
    g_os = new(batch)
    lib = _lib.load()
    ws = _ws(lib.nsgp_rbf_periodic_build_bwd_workspace(batch, n1, n2, D, ref.element_size()), ref.device)
    _lib.call(f'nsgp_rbf_periodic_build_bwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls_rbf), _p(ls_per), _p(period), _p(os_),
              batch, n1, n2, D, sx1, sx2, _p(G), n2, n1 * n2, _p(g_x1), _p(g_x2), _p(g_lr), _p(g_lp), _p(g_pe), _p(g_os),
              _p(ws), ws.numel(), _stream())
    return g_x1, g_x2, g_lr, g_lp, g_pe, g_os


# --------------------------------------------------------------------------------------------
# K2''' Matern-ARD x Periodic (one launch), nu in {1/2, 3/2, 5/2}: the rbf_periodic argument rules, the envelope required
# --------------------------------------------------------------------------------------------
def _matper_args(x1, x2, ls_env, ls_per, period, os_, nu):
    nu2 = _nu2(nu)
    if ls_env is None:
        raise BackendError('matern_periodic_build: ls_env is required (the plain PeriodicKernel is rbf_periodic_build)')
    return (*_rbfper_args(x1, x2, ls_env, ls_per, period, os_, 'matern_periodic_build', 'ls_env'), nu2)


def matern_periodic_build(x1, x2, ls_env, ls_per, period, os_, nu, diag_add=0.0):
    """K[b] = os[b] Matern_nu-ARD(x; ls_env[b]) Periodic(x; ls_per[b], period[b]) (+diag_add I); os_ may be None."""
    ref, x1, x2, ls_env, ls_per, period, os_, batch, n1, n2, D, sx1, sx2, nu2 = _matper_args(x1, x2, ls_env, ls_per,
                                                                                            period, os_, nu)
    K = torch.empty((batch, n1, n2), dtype=ref.dtype, device=ref.device)
    _lib.call(f'nsgp_matern_periodic_build_fwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls_env), _p(ls_per), _p(period), _p(os_),
              batch, n1, n2, D, sx1, sx2, nu2, float(diag_add), _p(K), n2, n1 * n2, _stream())
    return K


def matern_periodic_build_bwd(x1, x2, ls_env, ls_per, period, os_, nu, G, need_x1=True, need_x2=True):
    """As rbf_periodic_build_bwd: g_x1:(batch,n1,D) g_x2:(batch,n2,D) per batch (None when not needed), g_ls_env:(batch,D),
    g_ls_per, g_period, g_os:(batch,).  For nu = 1/2 the derivative at zero distance is taken as 0."""
    ref, x1, x2, ls_env, ls_per, period, os_, batch, n1, n2, D, sx1, sx2, nu2 = _matper_args(x1, x2, ls_env, ls_per,
                                                                                            period, os_, nu)
    _chk(ref, G)
    G = _c(G).reshape(batch, n1, n2)
    new = lambda *shp: torch.empty(shp, dtype=ref.dtype, device=ref.device)
    g_x1 = new(batch, n1, D) if need_x1 else None
    g_x2 = new(batch, n2, D) if need_x2 else None
    g_le, g_lp, g_pe, g_os = new(batch, D), new(batch), new(batch), new(batch)
    # the periodic family's accumulator layout: one workspace query for both members
    ws = _ws(_lib.load().nsgp_rbf_periodic_build_bwd_workspace(batch, n1, n2, D, ref.element_size()), ref.device)
    _lib.call(f'nsgp_matern_periodic_build_bwd_{_sfx(ref)}', _p(x1), _p(x2), _p(ls_env), _p(ls_per), _p(period), _p(os_),
              batch, n1, n2, D, sx1, sx2, nu2, _p(G), n2, n1 * n2, _p(g_x1), _p(g_x2), _p(g_le), _p(g_lp), _p(g_pe),
              _p(g_os), _p(ws), ws.numel(), _stream())
    return g_x1, g_x2, g_le, g_lp, g_pe, g_os


# --------------------------------------------------------------------------------------------
# K3 Paciorek-Schervish (D = 2)
# --------------------------------------------------------------------------------------------
def _ps_args(x1, x2, s1, s2):
    ref = _chk(x1, x2, s1, s2)
    n1, n2 = x1.shape[0], x2.shape[0]
    if x1.shape != (n1, 2) or x2.shape != (n2, 2) or s1.shape != (n1, 2, 2) or s2.shape != (n2, 2, 2):
        raise BackendError('ps2d_build: x:(n,2), sigma:(n,2,2) expected')
    return ref, n1, n2


def _ps_entry(nu):
    """(library stem, the scalars its entry points take after n2) of the Paciorek-Schervish build: nu = None is the
    squared-exponential kernel, nu in {0.5, 1.5, 2.5} its Matern form (K3', nu2 = 2 nu).  Any other value raises as
    _gibbs_entry."""
    if nu is None:
        return 'ps2d', ()
    if nu not in MATERN_NU:
        raise RuntimeError('nu expected to be 0.5, 1.5, or 2.5')
    return 'ps2d_matern', (int(2 * nu),)


def ps2d_build(x1, x2, s1, s2, jitter=1e-5, nu=None):
    """K = |S1|^(1/4) |S2|^(1/4) |A|^(-1/2) exp(-Q), A = (S1 + S2) / 2, Q = d^T (A + jitter I)^-1 d.
    nu in {0.5, 1.5, 2.5}: Matern_nu(sqrt(2 Q)) in place of exp(-Q) (include/nsgp.h, K3')."""
    stem, extra = _ps_entry(nu)
    ref, n1, n2 = _ps_args(x1, x2, s1, s2)
    x1, x2, s1, s2 = _c(x1), _c(x2), _c(s1), _c(s2)
    K = torch.empty((n1, n2), dtype=ref.dtype, device=ref.device)
    _lib.call(f'nsgp_{stem}_build_fwd_{_sfx(ref)}', _p(x1), _p(x2), _p(s1), _p(s2), n1, n2, *extra, float(jitter), _p(K),
              n2, _stream())
    return K


def ps2d_build_bwd(x1, x2, s1, s2, jitter, G, nu=None):
    stem, extra = _ps_entry(nu)
    ref, n1, n2 = _ps_args(x1, x2, s1, s2)
    _chk(ref, G)
    x1, x2, s1, s2, G = _c(x1), _c(x2), _c(s1), _c(s2), _c(G)
    g1, g2 = torch.empty_like(s1), torch.empty_like(s2)
    lib = _lib.load()
    ws = _ws(lib.nsgp_ps2d_build_bwd_workspace(n1, n2, ref.element_size()), ref.device)
    _lib.call(f'nsgp_{stem}_build_bwd_{_sfx(ref)}', _p(x1), _p(x2), _p(s1), _p(s2), n1, n2, *extra, float(jitter), _p(G),
              n2, _p(g1), _p(g2), _p(ws), ws.numel(), _stream())
    return g1, g2


class PairwiseBwdPlan(NamedTuple):
    """The launch every *_build_bwd makes (include/nsgp.h, nsgp_pairwise_bwd_plan)."""
    rows: int
    nti: int
    ntj: int


def pairwise_bwd_plan(batch, n1, n2):
    """The backward launch of a (batch, n1, n2) build (batch = 1 for Gibbs and ps2d), as a PairwiseBwdPlan.  Host-side only:
    nothing is launched and no GPU is needed."""
    rows = ctypes.c_int(0)
    nti, ntj = ctypes.c_int64(0), ctypes.c_int64(0)
    ref = lambda v: ctypes.cast(ctypes.byref(v), ctypes.c_void_p)  # noqa: E731
    _lib.call('nsgp_pairwise_bwd_plan', int(batch), int(n1), int(n2), ref(rows), ref(nti), ref(ntj))
    return PairwiseBwdPlan(rows.value, nti.value, ntj.value)


# --------------------------------------------------------------------------------------------
# KM Lloyd's k-means (include/nsgp.h, KM; nsgp.cluster drives the loop).  Raw ops, no autograd.
# --------------------------------------------------------------------------------------------
def _kmeans_x(x, c, what):
    """(x as the kernel reads it, ldx, n, D): any 2-D x with unit column stride and row stride >= D goes in without a copy."""
    ref = _chk(x, c)
    if x.dim() != 2 or c.dim() != 2 or c.shape[1] != x.shape[1] or c.shape[0] < 1:
        raise BackendError(f'{what}: x:(n,D), centres:(M>=1,D) expected, got {tuple(x.shape)} and {tuple(c.shape)}')
    n, D = x.shape
    if (D > 1 and x.stride(1) != 1) or (n > 1 and x.stride(0) < D):
        x = x.contiguous()
    return ref, x, max(x.stride(0), D), n, D


def _kmeans_vec(t, n, dtype, ref, name):
    if t.shape != (n,) or t.dtype != dtype or t.device != ref.device or not t.is_contiguous():
        raise BackendError(f'{name}: contiguous ({n},) {dtype} tensor on {ref.device} expected')
    return t


def kmeans_assign(x, c, labels=None, d2=None):
    """(labels int32 (n,), d2 (n,)): the nearest of the M centres c:(M,D) of every point of x:(n,D) and the squared distance
    to it (FMA chain on differences; strict <, so the lowest index wins a tie; a NaN point keeps label 0 and d2 = +inf).
    `labels` / `d2`: buffers to write into."""
    ref, x, ldx, n, D = _kmeans_x(x, c, 'kmeans_assign')
    c = _c(c)
    labels = torch.empty(n, dtype=torch.int32, device=ref.device) if labels is None \
        else _kmeans_vec(labels, n, torch.int32, ref, 'labels')
    d2 = torch.empty(n, dtype=ref.dtype, device=ref.device) if d2 is None else _kmeans_vec(d2, n, ref.dtype, ref, 'd2')
    _lib.call(f'nsgp_kmeans_assign_{_sfx(ref)}', _p(x), ldx, n, D, _p(c), c.shape[0], _p(labels), _p(d2), _stream())
    return labels, d2


def kmeans_update(x, labels, d2, c_old):
    """(c_new (M,D), counts int32 (M,), stats float64 (2,) = [sum d2, sum_k |c_new_k - c_old_k|^2]): the mean of every
    cluster's points, float64 sums in an order fixed by (n, D, M), one division; an empty cluster keeps c_old bit for bit."""
    ref, x, ldx, n, D = _kmeans_x(x, c_old, 'kmeans_update')
    _chk(ref, d2)
    c_old = _c(c_old)
    M = c_old.shape[0]
    _kmeans_vec(labels, n, torch.int32, ref, 'labels')
    _kmeans_vec(d2, n, ref.dtype, ref, 'd2')
    c_new = torch.empty_like(c_old)
    counts = torch.empty(M, dtype=torch.int32, device=ref.device)
    stats = torch.empty(2, dtype=torch.float64, device=ref.device)
    ws = _ws(_lib.load().nsgp_kmeans_update_workspace(n, D, M), ref.device)
    _lib.call(f'nsgp_kmeans_update_{_sfx(ref)}', _p(x), ldx, n, D, _p(labels), _p(d2), _p(c_old), M, _p(c_new), _p(counts),
              _p(stats), _p(ws), _stream())
    return c_new, counts, stats


# --------------------------------------------------------------------------------------------
# MFMA GEMM
# --------------------------------------------------------------------------------------------
def _mat_view(t, trans):
    """Return (tensor, rows, cols, row_stride, col_stride, batch, batch_stride) of op(t) without copying
    when one of the two trailing strides is 1; otherwise make it contiguous."""
    if t.dim() not in (2, 3):
        raise BackendError('gemm: operands must be 2-D or 3-D (batched)')
    sr, sc = t.stride(-2), t.stride(-1)
    ok = (sr == 1 or sc == 1) and (t.dim() == 2 or t.shape[0] == 1 or t.stride(0) >= 0)
    if t.shape[-1] == 1 and sr != 1:
        sc = 1
    if t.shape[-2] == 1 and sc != 1:
        sr = 1
    if not ok or not (sr == 1 or sc == 1):
        t = t.contiguous()
        sr, sc = t.stride(-2), t.stride(-1)
    r, c = t.shape[-2], t.shape[-1]
    if trans:
        r, c, sr, sc = c, r, sc, sr
    nb = t.shape[0] if t.dim() == 3 else 1
    sb = t.stride(0) if t.dim() == 3 else 0
    return t, r, c, sr, sc, nb, sb


_gemm_timer = None


def set_gemm_timer(timer):
    """bench.py hook: `timer(fn, flops, dtype)` must call fn() (the launch) and may bracket it with HIP events.
    flops = algorithmic 2*M*N*K per batch element, halved for a triangular operand / lower-only output."""
    global _gemm_timer
    _gemm_timer = timer


class GemmPlan(NamedTuple):
    """The launch nsgp_gemm_* makes for a product (include/nsgp.h, nsgp_gemm_plan): the fields of its `out` array."""
    tile_m: int
    tile_n: int
    ksplit: int
    kper: int
    whole: int
    xcd_chunk: int
    batch_perm: int
    grid_x: int
    grid_y: int
    mode_a: int
    mode_b: int


def _gemm_operands(A, B, ta, tb, out):
    """Views, sizes, strides and the output of gemm(); shared with gemm_plan so that both see the same operands."""
    ref = A
    A, M, K, sam, sak, nba, sba = _mat_view(A, ta)
    B, K2, N, sbk, sbn, nbb, sbb = _mat_view(B, tb)
    if K != K2:
        raise BackendError(f'gemm: inner dims {K} vs {K2}')
    nb = max(nba, nbb)
    if nba not in (1, nb) or nbb not in (1, nb):
        raise BackendError('gemm: batch mismatch')
    if nba == 1:
        sba = 0
    if nbb == 1:
        sbb = 0
    batched = A.dim() == 3 or B.dim() == 3
    shape = (nb, M, N) if batched else (M, N)
    if out is not None and (tuple(out.shape) != shape or not out.is_contiguous()):
        raise BackendError(f'gemm: out must be contiguous {shape}, got {tuple(out.shape)}')
    return ref, shape, A, M, K, sam, sak, sba, B, N, sbk, sbn, sbb, nb


def gemm_plan(A, B, ta=False, tb=False, flags=0, out=None):
    """The plan `gemm(A, B, ta, tb, flags=flags, out=out)` launches, as a GemmPlan.  Host-side only: nothing is launched and
    no GPU is needed (CPU tensors of the same layout give the plan of their device twins as far as their base pointers are
    aligned alike).  mode_* / vec_* are derived from the operand views the way gemm_impl (csrc/gemm.hip) derives them."""
    _sfx(A)
    ref, shape, A, M, K, sam, sak, sba, B, N, sbk, sbn, sbb, nb = _gemm_operands(A, B, ta, tb, out)
    es = ref.element_size()

    def mode_vec(t, s_other, s_k, s_batch):            # s_k: stride along k; s_other: along m (A) or n (B)
        mode = 0 if s_k == 1 else (1 if s_other == 1 else 0)
        unit, other = (s_k, s_other) if mode == 0 else (s_other, s_k)
        return mode, int(unit == 1 and other % 4 == 0 and s_batch % 4 == 0 and t.data_ptr() % (4 * es) == 0)
    mode_a, vec_a = mode_vec(A, sam, sak, sba)
    mode_b, vec_b = mode_vec(B, sbn, sbk, sbb)
    buf = (ctypes.c_int32 * len(GemmPlan._fields))()
    _lib.call('nsgp_gemm_plan', M, N, K, nb, 1, es, int(flags), vec_a, vec_b, mode_a, mode_b,
              ctypes.cast(buf, ctypes.c_void_p))
    return GemmPlan(*buf)


class GemmWaveSchedule(NamedTuple):
    """One wave's walk through the K loop of a float32 gemm_kernel workgroup (include/nsgp.h, nsgp_gemm_wave_schedule)."""
    tm: int
    tn: int
    row_blocks: tuple      # 32-row block of the tile per MFMA tile row
    col_blocks: tuple      # 32-column block of the tile per MFMA tile column
    lo: tuple              # per MFMA tile x = i * tn + j: it has work in the K-tiles [lo[x], hi[x])
    hi: tuple
    nt: int
    h0: int
    h1: int
    p0: int
    p1: int
    kbeg: int              # after the triangular clip; K-tiles are counted from it
    masks: int             # bit m: MFMA mask m exists as a loop copy
    segments: tuple        # stretches of the hot range: (first K-tile, end, mask run, bare staging)
    tiles: tuple           # per K-tile: (mask needed, mask run, staging masks diagonal blocks, times run)


_SCHED_HEAD, _SCHED_SEGS = 24, 16   # NSGP_GEMM_SCHED_HEAD, NSGP_GEMM_SCHED_SEGS (include/nsgp.h)


def gemm_wave_schedule(tile_m, tile_n, flags, bm, bn, wave, kbeg, kend, epi=0, ksc=0, edge=False, interior=True):
    """Host-side only (no GPU): the schedule gemm_kernel<float, tile_m, tile_n, ...> gives wave `wave` of tile (bm, bn) on the
    K-slice [kbeg, kend), computed by the functions the kernel runs.  edge: the variant with bounds code (ragged or unaligned
    launch); interior (edge only): the workgroup's tile lies inside M and N on vector-loadable operands."""
    depth = 32 if tile_m == 128 else 16
    cap = _SCHED_HEAD + 4 * _SCHED_SEGS + 4 * ((kend - kbeg + depth - 1) // depth + 2)
    buf = (ctypes.c_int32 * cap)()
    _lib.call('nsgp_gemm_wave_schedule', int(tile_m), int(tile_n), int(epi), int(ksc), int(bool(edge)), int(flags),
              int(bool(interior)), int(bm), int(bn), int(wave), int(kbeg), int(kend), ctypes.cast(buf, ctypes.c_void_p), cap)
    o = list(buf)
    tm, tn, nt, nseg = o[0], o[1], o[14], o[20]
    if nseg > _SCHED_SEGS:
        raise BackendError(f'gemm_wave_schedule: {nseg} stretches')
    s0, t0 = _SCHED_HEAD, _SCHED_HEAD + 4 * _SCHED_SEGS
    return GemmWaveSchedule(tm, tn, tuple(o[2:2 + tm]), tuple(o[4:4 + tn]), tuple(o[6:6 + tm * tn]), tuple(o[10:10 + tm * tn]),
                            nt, o[15], o[16], o[17], o[18], o[19], o[21],
                            tuple(tuple(o[s0 + 4 * i:s0 + 4 * i + 4]) for i in range(nseg)),
                            tuple(tuple(o[t0 + 4 * t:t0 + 4 * t + 4]) for t in range(nt)))


GEMM_OUT64_UNSPLIT = -64   # NSGP_GEMM_OUT64_UNSPLIT (include/nsgp.h)


def gemm(A, B, ta=False, tb=False, alpha=1.0, beta=0.0, out=None, flags=0, out64=None):
    """out = alpha * op(A) @ op(B) + beta * out on the matrix cores.  2-D or batched 3-D operands
    (a 2-D operand broadcasts against a 3-D one).
    out64 (float32 product): a contiguous float64 tensor of out's shape that receives a widened copy of every element the
    call writes to out -- from the split-K reduce where the product is split (nsgp_gemm_f32_out64), by a cast launch of the
    whole of out where it is not."""
    ref = _chk(A, B, out)
    ref, shape, A, M, K, sam, sak, sba, B, N, sbk, sbn, sbb, nb = _gemm_operands(A, B, ta, tb, out)
    if out is None:
        if beta != 0.0:
            raise BackendError('gemm: beta != 0 needs out')
        out = torch.empty(shape, dtype=ref.dtype, device=ref.device)
    if out64 is not None and (ref.dtype != torch.float32 or out64.dtype != torch.float64 or tuple(out64.shape) != shape
                              or not out64.is_contiguous() or out64.device != ref.device):
        raise BackendError(f'gemm: out64 must be a contiguous float64 {shape} beside a float32 product')
    lib = _lib.load()
    wsb = 0 if (flags & GEMM_NO_SPLITK) else lib.nsgp_gemm_workspace(M, N, K, nb, 1, ref.element_size(), int(flags))
    ws = _ws(wsb, ref.device) if wsb else None
    def launch():
        args = (M, N, K, float(alpha), _p(A), sam, sak, sba, 0, _p(B), sbk, sbn, sbb, 0,
                float(beta), _p(out), N, M * N, 0, nb, 1, int(flags), _p(ws), ws.numel() if ws is not None else 0,
                _stream())
        if out64 is not None:
            rc = lib.nsgp_gemm_f32_out64(*args, _p(out64), N, M * N, 0)
            if rc == 0:
                return
            if rc != GEMM_OUT64_UNSPLIT:
                raise BackendError('nsgp_gemm_f32_out64 failed: ' + (f'argument {-rc} invalid' if rc < 0 else f'hipError {rc}'))
        _lib.call(f'nsgp_gemm_{_sfx(ref)}', *args)
        if out64 is not None:
            cast(out, torch.float64, out=out64)
    if _gemm_timer is not None:
        tri = flags & (GEMM_A_LOWER | GEMM_A_UPPER | GEMM_B_LOWER | GEMM_B_UPPER | GEMM_C_LOWER)
        _gemm_timer(launch, 2.0 * M * N * K * nb * (0.5 if tri else 1.0), ref.dtype)
    else:
        launch()
    return out


# --------------------------------------------------------------------------------------------
# K4 / K5 Cholesky, triangular inverse
# --------------------------------------------------------------------------------------------
def potrf(A, check=False, overwrite=False):
    """Lower Cholesky factor of a (batched) SPD matrix; returns (L, info) with info an int32 device
    tensor (LAPACK convention).  `check=True` syncs and raises on failure; `overwrite=True` factors a
    contiguous input in place."""
    ref = _chk(A)
    if A.dim() not in (2, 3) or A.shape[-1] != A.shape[-2]:
        raise BackendError('potrf: square (batched) matrix expected')
    L = A if (overwrite and A.is_contiguous()) else A.contiguous().clone()
    n = L.shape[-1]
    batch = L.shape[0] if L.dim() == 3 else 1
    info = (torch.empty if n > 0 else torch.zeros)(batch, dtype=torch.int32, device=ref.device)   # set by the first panel
    lib = _lib.load()
    ws = _ws(lib.nsgp_potrf_workspace(n, batch, ref.element_size()), ref.device)
    _lib.call(f'nsgp_potrf_{_sfx(ref)}', _p(L), n, n, n * n, batch, _p(info), _p(ws), ws.numel(), _stream())
    if check:
        bad = int(info.max().item())
        if bad:
            raise BackendError(f'potrf: leading minor {bad} is not positive definite')
    return L, info


def trtri(L):
    """X = L^-1 for a (batched) lower-triangular L (strict upper of L ignored, of X zero)."""
    ref = _chk(L)
    if L.dim() not in (2, 3) or L.shape[-1] != L.shape[-2]:
        raise BackendError('trtri: square (batched) matrix expected')
    L = _c(L)
    n = L.shape[-1]
    batch = L.shape[0] if L.dim() == 3 else 1
    X = torch.empty_like(L)
    lib = _lib.load()
    ws = _ws(lib.nsgp_trtri_workspace(n, batch, ref.element_size()), ref.device)
    _lib.call(f'nsgp_trtri_{_sfx(ref)}', _p(L), n, n, n * n, _p(X), n, n * n, batch, _p(ws), ws.numel(), _stream())
    return X


def potrf_trtri_(A, want_f32=False):
    """(X, info) with X = chol(A)^-1 (lower triangular) for a contiguous (batched) SPD matrix that is CONSUMED: on return A
    holds intermediate data, not a factor.  One chain of launches without the factor's write-back pass.
    want_f32=True (float64 A): returns (X, info, X32) with a float32 copy of X -- written by the same launches when the
    in-launch inverse runs, by a cast otherwise."""
    ref = _chk(A)
    if A.dim() not in (2, 3) or A.shape[-1] != A.shape[-2] or not A.is_contiguous():
        raise BackendError('potrf_trtri_: contiguous square (batched) matrix expected')
    n = A.shape[-1]
    batch = A.shape[0] if A.dim() == 3 else 1
    X = torch.empty_like(A)
    info = (torch.empty if n > 0 else torch.zeros)(batch, dtype=torch.int32, device=ref.device)
    lib = _lib.load()
    ws = _ws(lib.nsgp_potrf_workspace(n, batch, ref.element_size()) + lib.nsgp_trtri_workspace(n, batch, ref.element_size()),
             ref.device)
    if want_f32 and ref.dtype == torch.float64:
        import ctypes
        X32 = torch.empty(A.shape, dtype=torch.float32, device=ref.device)
        wrote = ctypes.c_int(0)
        _lib.call('nsgp_potrf_trtri_f64_w32', _p(A), n, n, n * n, batch, _p(info), _p(X), n, n * n, _p(X32),
                  ctypes.addressof(wrote), _p(ws), ws.numel(), _stream())
        if not wrote.value:
            X32 = cast(X, torch.float32)
        return X, info, X32
    _lib.call(f'nsgp_potrf_trtri_{_sfx(ref)}', _p(A), n, n, n * n, batch, _p(info), _p(X), n, n * n, _p(ws), ws.numel(),
              _stream())
    if want_f32:
        return X, info, (X if ref.dtype == torch.float32 else cast(X, torch.float32))
    return X, info


def chol_bwd_phi_sym(P):
    ref = _chk(P)
    P = _c(P)
    n = P.shape[-1]
    batch = P.shape[0] if P.dim() == 3 else 1
    S = torch.empty_like(P)
    _lib.call(f'nsgp_chol_bwd_phi_sym_{_sfx(ref)}', _p(P), _p(S), n, n, n * n, batch, _stream())
    return S


def scale_diag_(P, factor):
    """P[..., i, i] *= factor in place (batch of square matrices)."""
    ref = _chk(P)
    if not P.is_contiguous():
        raise BackendError('scale_diag_: contiguous matrices expected')
    n = P.shape[-1]
    batch = P.shape[0] if P.dim() == 3 else 1
    _lib.call(f'nsgp_scale_diag_{_sfx(ref)}', _p(P), n, n, n * n, batch, float(factor), _stream())
    return P


def cast(t, dtype, out=None):
    """float32 <-> float64 copy on the current stream (row-major, any leading shape).  `out`: a contiguous tensor of the
    target dtype and the same number of elements to write into (e.g. a slice of a batched buffer) instead of a new one."""
    _chk(t)
    if t.dtype == dtype and out is None:
        return t
    t = _c(t)
    if out is None:
        out = torch.empty(t.shape, dtype=dtype, device=t.device)
    elif out.dtype != dtype or out.numel() != t.numel() or not out.is_contiguous() or out.device != t.device or t.dtype == dtype:
        raise BackendError('cast(out=...): contiguous tensor of the target dtype with as many elements, on the same device')
    cols = t.shape[-1] if t.dim() else 1
    rows = t.numel() // max(cols, 1)
    name = 'nsgp_cast_f64_to_f32' if dtype == torch.float32 else 'nsgp_cast_f32_to_f64'
    _lib.call(name, _p(t), cols, _p(out), cols, rows, cols, _stream())
    return out


# --------------------------------------------------------------------------------------------
# K6 / K7 raw ops
# --------------------------------------------------------------------------------------------
def svgp_colstats(A, C, m, base):
    ref = _chk(A, C, m, base)
    A, C, m, base = _c(A), _c(C), _c(m), _c(base.reshape(-1))
    batch, M, n = A.shape
    if C.shape != A.shape or m.shape != (batch, M) or base.shape != (batch,):
        raise BackendError('svgp_colstats: shapes')
    mean = torch.empty((batch, n), dtype=ref.dtype, device=ref.device)
    var = torch.empty_like(mean)
    _lib.call(f'nsgp_svgp_colstats_{_sfx(ref)}', _p(A), _p(C), _p(m), _p(base), batch, M, n, _p(mean), _p(var),
              _stream())
    return mean, var


def svgp_colstats_bwd(A, C, m, gmean, gvar):
    ref = _chk(A, C, m, gmean, gvar)
    A, C, m, gmean, gvar = _c(A), _c(C), _c(m), _c(gmean), _c(gvar)
    batch, M, n = A.shape
    if gmean.shape != (batch, n) or gvar.shape != (batch, n):
        raise BackendError('svgp_colstats_bwd: shapes')
    Abar, C2 = torch.empty_like(A), torch.empty_like(C)
    mbar = torch.empty_like(m)
    _lib.call(f'nsgp_svgp_colstats_bwd_{_sfx(ref)}', _p(A), _p(C), _p(m), _p(gmean), _p(gvar), batch, M, n,
              _p(Abar), _p(C2), _p(mbar), _stream())
    return Abar, C2, mbar


def _timed(launch, flops, dtype):
    if _gemm_timer is not None:
        _gemm_timer(launch, flops, dtype)
    else:
        launch()


def _affine_args(affine, batch, n, ref):
    """(x, w, c) of an affine prior mean -> pointer / stride arguments of the *_affine entry points (all null for None).
    x:(n,D) shared by the batch or (batch,n,D); w:(D,) shared or (batch,D) or None; c:(1,) shared or (batch,) or None."""
    if affine is None:
        return None, 0, 0, None, 0, None, 0
    x, w, c = affine
    x = _c(x)
    D = x.shape[-1]
    if x.shape[-2] != n or (x.dim() == 3 and x.shape[0] != batch) or x.dim() not in (2, 3):
        raise BackendError('affine prior mean: x shape')
    sxb = n * D if x.dim() == 3 else 0
    swb = scb = 0
    if w is not None:
        w = _c(w.reshape(-1, D))
        if w.shape[0] not in (1, batch):
            raise BackendError('affine prior mean: weights shape')
        swb = D if (w.shape[0] == batch and batch > 1) else 0
    if c is not None:
        c = _c(c.reshape(-1))
        if c.shape[0] not in (1, batch):
            raise BackendError('affine prior mean: constant shape')
        scb = 1 if (c.shape[0] == batch and batch > 1) else 0
    _chk(ref, x, *[t for t in (w, c) if t is not None])
    return x, sxb, D, w, swb, c, scb


def _affine_grad_outputs(affine, swb, scb, w, c, batch, D, ref):
    """(shared, wbar, cbar) of `_affine_args`' operands: shared = 1 when the mean parameters are shared by the batch (their
    gradients are then summed over it); wbar / cbar are empty, in the shapes of w / c (None where w / c is None)."""
    shared = int(affine is not None and swb == 0 and scb == 0)
    if w is not None and c is not None and batch > 1 and (swb == 0) != (scb == 0):
        raise BackendError('affine prior mean: weights and constant must both be shared or both be per batch')
    nb = 1 if shared else batch
    wbar = None if w is None else torch.empty((nb, D), dtype=ref.dtype, device=ref.device)
    cbar = None if c is None else torch.empty(nb, dtype=ref.dtype, device=ref.device)
    return shared, wbar, cbar


def _w64_operand(W64f, ref, dims, what):
    """The float64 W of a float32 layer, checked against the layer's (batch, M) and device, contiguous."""
    if ref.dtype != torch.float32 or W64f.dtype != torch.float64 or W64f.shape != (*dims, dims[1]) or W64f.device != ref.device:
        raise BackendError(f'{what}: W64f must be the float64 (b,M,M) W of a float32 layer')
    return _c(W64f)


def _kernel_inputs_args(t, ref, what):
    """(Z, x, ls, os) of a stationary ARD kernel (RBF; Matern on the int8 path, `kernel_nu`) whose Kzx a projection evaluates
    itself -> the four tensors contiguous (os flat) and (b, M, n), checked: ref's device and dtype, Z:(b,M,D), x:(n,D) or
    (b,n,D), ls:(b,D), os:(b,)."""
    if not isinstance(t, (tuple, list)) or len(t) != 4 or not all(isinstance(v, torch.Tensor) for v in t):
        raise BackendError(f'{what}: (Z, x, ls, os) expected')
    _chk(ref, *t)
    kZ, kx, kls, kos = _c(t[0]), _c(t[1]), _c(t[2]), _c(t[3].reshape(-1))
    b, D = kZ.shape[0], kZ.shape[-1]
    if kZ.dim() != 3 or kx.dim() not in (2, 3) or kx.shape[-1] != D or (kx.dim() == 3 and kx.shape[0] != b) \
            or kls.shape != (b, D) or kos.shape != (b,):
        raise BackendError(f'{what}: (Z, x, ls, os) shapes')
    return (kZ, kx, kls, kos), (b, kZ.shape[1], kx.shape[-2])


def svgp_kzx_fusable(W64f, Z, x, n):
    """True when A = W Kzx can run with Kzx generated inside the GEMM loader (nsgp_svgp_kzx_gemm_colstats_f64acc):
    float32 layer with its float64 W, D <= 4, whole tiles."""
    if W64f is None or W64f.dtype != torch.float64 or Z.dtype != torch.float32 or not W64f.is_contiguous():
        return False
    batch, M, D = Z.shape
    return bool(_lib.load().nsgp_svgp_kzx_gemm_supported(_p(W64f), M, n, batch, D))


def _project_a_i8(W64f, kZ, kx, kls, kos, m, A, part_dot, part_sq, T, p64, planes, flops, kzx_out=None, nu=None):
    """A = W Kzx as the exact int8 digit-plane product (csrc/gemm_i8.hip): digit planes of W and of Kzx (evaluated in
    float64 from Z, x, ls, os -- RBF, or Matern with nu in MATERN_NU), then the product with its column-statistic partials
    (T tile rows per batch element).
    kzx_out: a list that receives the float32 Kzx (b, M, n) the plane-build kernel writes along (for the backward pass)."""
    lib = _lib.load()
    batch, M, D = kZ.shape
    n = kx.shape[-2]
    dev, st = A.device, _stream()
    Wd = torch.empty(int(lib.nsgp_i8_w_planes_bytes(batch, M)), dtype=torch.uint8, device=dev)
    Kd = torch.empty(int(lib.nsgp_i8_k_planes_bytes(batch, M, n, planes)), dtype=torch.uint8, device=dev)
    wsc = torch.empty((batch, M), dtype=torch.float64, device=dev)
    ksc = torch.empty((int(lib.nsgp_i8_kscale_count(batch, M, n)),), dtype=torch.float64, device=dev)
    K32 = torch.empty((batch, M, n), dtype=torch.float32, device=dev) if kzx_out is not None else None
    _lib.call('nsgp_i8_slice_w_f64', _p(W64f), batch, M, _p(Wd), _p(wsc), st)
    if nu is None:
        _lib.call('nsgp_i8_rbf_build_f32', _p(kZ), _p(kx), n * D if kx.dim() == 3 else 0, _p(kls), _p(kos), batch, M, n, D,
                  planes, _p(Kd), _p(ksc), _p(K32), st)
    else:
        _lib.call('nsgp_i8_matern_build_f32', _p(kZ), _p(kx), n * D if kx.dim() == 3 else 0, _p(kls), _p(kos), batch, M, n, D,
                  _nu2(nu), planes, _p(Kd), _p(ksc), _p(K32), st)
    if kzx_out is not None:
        kzx_out.append(K32)
    _timed(lambda: _lib.call('nsgp_svgp_tri_gemm_colstats_i8', _p(Wd), _p(wsc), _p(Kd), _p(ksc), planes, _p(m), batch, M, n,
                             _p(A), _p(part_dot), _p(part_sq), T, 1 if p64 else 0, st), flops, 'i8')


class ProjectionPlan(NamedTuple):
    """What one forward projection launches and how its column-statistic partials are laid out (`svgp_projection_plan`)."""
    first: str                  # arithmetic of A = W Kzx: 'f32' | 'f64acc' | 'f64acc_b64' | 'kzx_fused' | 'i8' | 'bf16'
    second: str                 # arithmetic of C = Lq^T A: 'f32' | 'f64acc_t' | 'bf16'; 'diag': mean-field q(u), no C
    planes: int                 # Kzx digit planes of the int8 product (4 or 5), else 0
    p1: str                     # entry points: product 1, product 2, and the reduction of the partials to mean and var
    p2: str
    fin: str
    T1: int                     # tile rows product 1 writes (planes 0 and 1 of the partials), product 2 writes (plane 2),
    T2: int                     # and T of the partials buffer (3, batch, T, n)
    T: int
    part_dtype: torch.dtype
    zero: bool                  # the buffer starts zero-filled
    scratch: bool               # product 2 writes a compact (batch, T2, n) buffer that is then copied into plane 2


@functools.lru_cache(maxsize=None)
def svgp_projection_plan(M, n, batch, dtype, first, second, i8_planes=4):
    """The plan of a forward projection, from sizes only (host-side planner queries of the library; no tensor, no GPU).
    Every kernel lays its partials out by its own tile height -- e.g. M = 1024, n = 4032, b = 1: 8 tile rows in the float32
    plan, 16 in the float64-accumulating kernel (64-row tiles when its 128-row grid is under one round of the chip) -- so
    the buffer has T = max(T1, T2) rows and is ZERO-FILLED EXACTLY WHEN SOME ROW OF SOME PLANE IS WRITTEN BY NO KERNEL
    (T1 < T or T2 < T): finalize sums all T rows of all three planes, and no error code reports an uninitialised one.
    'f64acc_t' (C accumulated in float64, float64 partials) follows a first product that can write float64 partials.
    second = 'diag' (mean-field q(u) = N(m, diag(s^2)), every `first`): there is no second product.  p2 is the pass over A
    that writes the float64 partials of q_j = sum_k (s_k^2 - 1) A_kj^2 -- T2 rows of a (batch, T2, n) buffer of their own --
    and the partials buffer (2, batch, T, n) holds product 1's two planes only (T = T1: no row is left unwritten)."""
    f32 = dtype == torch.float32
    if second == 'diag':
        if first not in ('f32', 'f64acc', 'f64acc_b64', 'kzx_fused', 'i8', 'bf16') or (not f32 and (dtype, first) != (torch.float64, 'f32')) \
                or (first == 'bf16' and M % 8):
            raise BackendError(f'svgp_projection_plan: no {first} / diag projection of a {dtype} layer with M = {M}')
        lib, sfx, pre = _lib.load(), 'f32' if f32 else 'f64', 'nsgp_svgp_tri_gemm_colstats_'
        T1 = int(lib.nsgp_svgp_colstats_tiles(M, n, batch, 4 if f32 else 8) if first == 'f32' else lib.nsgp_i8_tiles(M)
                 if first == 'i8' else lib.nsgp_svgp_bf16_tiles(M) if first == 'bf16' else lib.nsgp_svgp_f64acc_tiles_for(M, n, batch))
        p1 = {'f32': pre + sfx, 'f64acc_b64': pre + 'f64acc_b64p32', 'kzx_fused': 'nsgp_svgp_kzx_gemm_colstats_f64acc'}.get(first, pre + first)
        return ProjectionPlan(first, second, (5 if i8_planes == 5 else 4) if first == 'i8' else 0, p1, 'nsgp_svgp_diag_colsq_' + sfx,
                              'nsgp_svgp_colstats_finalize_diag_' + sfx, T1, int(lib.nsgp_svgp_diag_tiles(M)), T1, dtype, False, False)
    if (not f32 and (dtype, first, second) != (torch.float64, 'f32', 'f32')) or (second == 'bf16' and M % 8) \
            or first not in ('f32', 'f64acc', 'f64acc_b64', 'kzx_fused', 'i8', 'bf16') or (first == 'bf16' and second != 'bf16') \
            or second not in ('f32', 'f64acc_t', 'bf16') or (second == 'f64acc_t' and first not in ('f64acc_b64', 'i8')):
        raise BackendError(f'svgp_projection_plan: no {first} / {second} projection of a {dtype} layer with M = {M}')
    lib, sfx, pre = _lib.load(), 'f32' if f32 else 'f64', 'nsgp_svgp_tri_gemm_colstats_'
    Tf = int(lib.nsgp_svgp_colstats_tiles(M, n, batch, 4 if f32 else 8))
    T1, T2 = (int(Tf if a == 'f32' else lib.nsgp_i8_tiles(M) if a == 'i8' else lib.nsgp_svgp_bf16_tiles(M) if a == 'bf16'
                  else lib.nsgp_svgp_f64acc_tiles_for(M, n, batch)) for a in (first, second))
    T, p64 = max(T1, T2), second == 'f64acc_t'
    # the plain float32 / float64 kernel lays its partials out with its own Tf rows; its *_rows twin takes the row count
    p1 = {'f32': pre + ('' if T == Tf else 'rows_') + sfx, 'f64acc_b64': pre + ('f64acc_b64' if p64 else 'f64acc_b64p32'),
          'kzx_fused': 'nsgp_svgp_kzx_gemm_colstats_f64acc'}.get(first, pre + first)
    # int8 with float64 partials has always been zero-filled, also where both kernels report the same tile rows (the
    # headline's first layer: 8 and 8) and the rule does not ask for it: kept, the launch sequence stays what it was
    zero = T1 < T or T2 < T or (first == 'i8' and p64)
    return ProjectionPlan(first, second, (5 if i8_planes == 5 else 4) if first == 'i8' else 0, p1,
                          pre + ('rows_' + sfx if second == 'f32' else second),
                          'nsgp_svgp_colstats_finalize_affine_' + ('p64_f32' if p64 else sfx), T1, T2, T,
                          torch.float64 if p64 else dtype, zero,
                          second == 'bf16' and T2 != T)       # the bf16 kernel writes its partials with its own row count


def _kernel_nu_arg(kernel_nu, first, what):
    """kernel_nu of a projection that evaluates Kzx itself: None (RBF), or a Matern nu -- which only the int8 plane build
    has; the generated-Kzx loader and the bf16 Kxz build are RBF-only paths."""
    if kernel_nu is None:
        return None
    if first != 'i8':
        raise BackendError(f'{what}: kernel_nu={kernel_nu} needs the int8 product (i8_inputs)' + (
            f'; the {first!r} projection evaluates Kzx in an RBF-only path' if first in ('kzx_fused', 'bf16') else ''))
    _nu2(kernel_nu)
    return float(kernel_nu)


def _run_projection(plan, dims, W, B, kin, Lq, m, base, base_add, affine, kzx_out=None, nu=None):
    """Allocate A, C, the partials, mean and var and launch what `plan` says: product 1 (W: its triangular operand in the
    precision the plan's arithmetic reads, B: the Kzx it reads or None, kin: the checked (Z, x, ls, os) it evaluates Kzx
    from or None), the bf16 cast / transpose, product 2 (Lq likewise) and finalize.  Returns A, C, mean, var."""
    (batch, M, n), dt, dev, st, T = dims, m.dtype, m.device, _stream(), plan.T
    flops = 1.0 * M * M * n * batch                      # 2 M M n / 2 (triangular operand)
    diag = plan.second == 'diag'                         # mean-field q(u): Lq is s^2 - 1 (batch, M), there is no C
    A = torch.empty((batch, M, n), dtype=dt, device=dev)
    C = None if diag else torch.empty_like(A)
    part = (torch.zeros if plan.zero else torch.empty)((2 if diag else 3, batch, max(T, 1), n), dtype=plan.part_dtype, device=dev)
    p0, p1 = _p(part[0]), _p(part[1])
    if kin is not None:
        kZ, kx, kls, kos = kin
        D = kZ.shape[-1]
        sx = n * D if kx.dim() == 3 else 0
    if plan.second == 'bf16':
        Ub = torch.empty((batch, M, M), dtype=torch.bfloat16, device=dev)
        AT = torch.empty((batch, n, M), dtype=torch.bfloat16, device=dev)
        _lib.call('nsgp_cast_sq_bf16_f32', _p(Lq), _p(Ub), M, batch, 1, 1, st)          # tril(Lq)^T
    if plan.first == 'f32':
        rows = (T,) if plan.p1.startswith('nsgp_svgp_tri_gemm_colstats_rows') else ()
        _timed(lambda: _lib.call(plan.p1, _p(W), 0, _p(B), _p(m), batch, M, n, _p(A), p0, p1, *rows, st), flops, dt)
    elif plan.first in ('f64acc', 'f64acc_b64'):
        _timed(lambda: _lib.call(plan.p1, _p(W), _p(B), _p(m), batch, M, n, _p(A), p0, p1, T, st), flops, 'f64acc')
    elif plan.first == 'kzx_fused':
        _timed(lambda: _lib.call(plan.p1, _p(W), _p(kZ), _p(kx), sx, _p(kls), _p(kos), D, _p(m), batch, M, n, _p(A), p0, p1,
                                 T, st), flops, 'f64acc')
    elif plan.first == 'i8':
        _project_a_i8(W, kZ, kx, kls, kos, m, A, part[0], part[1], T, plan.part_dtype != dt, plan.planes, flops,
                      kzx_out=kzx_out, nu=nu)
    else:                                                # bf16: bf16 copies of W and of Kxz, written by the build kernel
        Wb = torch.empty((batch, M, M), dtype=torch.bfloat16, device=dev)
        Kxz = torch.empty((batch, n, M), dtype=torch.bfloat16, device=dev)
        _lib.call('nsgp_cast_sq_bf16_f64' if W.dtype == torch.float64 else 'nsgp_cast_sq_bf16_f32', _p(W), _p(Wb), M, batch,
                  0, 1, st)
        _lib.call('nsgp_rbf_build_t_bf16', _p(kZ), _p(kx), _p(kls), _p(kos), batch, M, n, D, sx, _p(Kxz), st)
        _timed(lambda: _lib.call(plan.p1, _p(Wb), 1, _p(Kxz), _p(m), batch, M, n, _p(A), None if diag else _p(AT), p0, p1, st),
               flops, 'bf16')
    if diag:
        mean, var = torch.empty((batch, n), dtype=dt, device=dev), torch.empty((batch, n), dtype=dt, device=dev)
        x, sxb, Da, w, swb, c, scb = _affine_args(affine, batch, n, m)
        pq = torch.empty((batch, max(plan.T2, 1), n), dtype=torch.float64, device=dev)
        _lib.call(plan.p2, _p(A), _p(Lq), batch, M, n, _p(pq), plan.T2, st)
        _lib.call(plan.fin, p0, T, _p(pq), plan.T2, _p(base), float(base_add), batch, n, _p(x), sxb, Da, _p(w), swb, _p(c), scb,
                  _p(mean), _p(var), st)
        return A, None, mean, var
    if plan.second == 'f32':
        _timed(lambda: _lib.call(plan.p2, _p(Lq), 1, _p(A), None, batch, M, n, _p(C), None, _p(part[2]), T, st), flops, dt)
    elif plan.second == 'f64acc_t':                      # C = Lq^T A accumulated in float64 (layers that feed the next layer)
        _timed(lambda: _lib.call(plan.p2, _p(Lq), _p(A), batch, M, n, _p(C), _p(part[2]), T, st), flops, 'f64acc')
    else:
        if plan.first != 'bf16':                         # (the bf16 first product writes the bf16 A^T along)
            _lib.call('nsgp_transpose_cast_bf16', _p(A), _p(AT), batch, M, n, st)
        p2 = torch.empty((batch, plan.T2, n), dtype=dt, device=dev) if plan.scratch else part[2]
        _timed(lambda: _lib.call(plan.p2, _p(Ub), 2, _p(AT), None, batch, M, n, _p(C), None, None, _p(p2), st), flops, 'bf16')
        if plan.scratch:
            part[2, :, :plan.T2].copy_(p2)
    mean, var = torch.empty((batch, n), dtype=dt, device=dev), torch.empty((batch, n), dtype=dt, device=dev)
    x, sxb, Da, w, swb, c, scb = _affine_args(affine, batch, n, m)
    _lib.call(plan.fin, _p(part[0]), _p(part[1]), _p(part[2]), _p(base), float(base_add), batch, T, n, _p(x), sxb, Da,
              _p(w), swb, _p(c), scb, _p(mean), _p(var), st)
    return A, C, mean, var


def svgp_project(W, Kzx, Lq, m, base, base_add=0.0, affine=None, W64f=None, kernel_inputs=None, Kzx64=None, Lq64=None,
                 i8_inputs=None, i8_planes=4, i8_kzx_out=None, kernel_nu=None):
    """Fused K6 forward: A = W Kzx, C = Lq^T A (triangular MFMA GEMMs) with the column statistics reduced in
    the GEMM epilogues.  W, Lq:(b,M,M) lower; Kzx:(b,M,n); m:(b,M); base:(b,).
    Returns A, C, mean = A^T m (+ the affine prior mean x w + c, `affine` = (x, w, c)), var = base + base_add +
    colsum(C^2 - A^2).
    W64f: the float64 W of a float32 layer -- A is then accumulated in float64 on the float32 Kzx and rounded once
    (nsgp_svgp_tri_gemm_colstats_f64acc: the reference's float64 solve); W itself (float32) is only used by the backward.
    kernel_inputs=(Z, x, ls, os) with Kzx=None (and W64f, `svgp_kzx_fusable`): Kzx is never materialised, its tiles are
    generated inside the loader of the first product from Z:(b,M,D), x:(n,D) or (b,n,D), ls:(b,D), os:(b,).
    Kzx64 (float64 (b,M,n), with W64f, instead of Kzx): the same product on a float64 Kzx.  i8_inputs=(Z, x, ls, os) (with
    W64f, instead of Kzx): A on the int8 matrix cores (csrc/gemm_i8.hip), exact int32 accumulation of the digit-plane
    products of the float64 W and of Kzx evaluated in float64 -- 14 with four Kzx planes, 19 with five (`i8_planes`).
    Lq64 (with Kzx64 or i8_inputs): the float64 Lq -- C is accumulated in float64 too, with float64 partials.
    kernel_nu (with i8_inputs only): the kernel of (Z, x, ls, os) is Matern with that nu instead of RBF."""
    i8, b64 = i8_inputs is not None, Kzx64 is not None
    kernel_nu = _kernel_nu_arg(kernel_nu, 'i8' if i8 else 'kzx_fused' if kernel_inputs is not None else 'dense', 'svgp_project')
    if i8 and (Kzx is not None or b64 or kernel_inputs is not None or W64f is None):
        raise BackendError('svgp_project: i8_inputs=(Z, x, ls, os) comes with W64f and without Kzx / Kzx64 / kernel_inputs')
    ref = _chk(W, Kzx, Lq, m, base)
    if b64 and (Kzx is not None or W64f is None or Kzx64.dtype != torch.float64 or Kzx64.dim() != 3 or Kzx64.device != ref.device):
        raise BackendError('svgp_project: Kzx64 (float64 (b,M,n) on the layer device, with W64f, instead of Kzx) expected')
    fused = Kzx is None and not b64 and not i8
    if fused and (kernel_inputs is None or W64f is None):
        raise BackendError('svgp_project: Kzx=None needs kernel_inputs and W64f')
    kin = B = None
    if i8 or fused:
        kin, (batch, M, n) = _kernel_inputs_args(i8_inputs if i8 else kernel_inputs, ref, 'svgp_project')
        if i8 and (ref.dtype != torch.float32 or kin[0].shape[2] > 4 or not _lib.load().nsgp_i8_supported(M)):
            raise BackendError('svgp_project: i8_inputs shapes (float32 layer, D <= 4, M <= 4096)')
    else:
        B = _c(Kzx64 if b64 else Kzx)
        batch, M, n = B.shape
    W, Lq, m, base = _c(W), _c(Lq), _c(m), _c(base.reshape(-1))
    if W.shape != (batch, M, M) or Lq.shape != (batch, M, M) or m.shape != (batch, M) or base.shape != (batch,):
        raise BackendError('svgp_project: shapes')
    if W64f is not None:
        W = _w64_operand(W64f, ref, (batch, M), 'svgp_project')
    if Lq64 is not None:
        if W64f is None or not (b64 or i8) or Lq64.dtype != torch.float64 or Lq64.shape != (batch, M, M) or Lq64.device != ref.device:
            raise BackendError('svgp_project: Lq64 must be the float64 (b,M,M) copy of Lq (with W64f and Kzx64 / i8_inputs)')
        Lq = _c(Lq64)
    first = 'i8' if i8 else 'f64acc_b64' if b64 else 'kzx_fused' if fused else 'f64acc' if W64f is not None else 'f32'
    plan = svgp_projection_plan(M, n, batch, ref.dtype, first, 'f32' if Lq64 is None else 'f64acc_t', i8_planes)
    return _run_projection(plan, (batch, M, n), W, B, kin, Lq, m, base, base_add, affine, i8_kzx_out, kernel_nu)


def svgp_project_bf16(W, Kzx, Lq, m, base, base_add=0.0, affine=None, W64f=None, kernel_inputs=None, i8_inputs=None,
                      i8_kzx_out=None, kernel_nu=None):
    """BASELINE configs[4]'s "bf16 forward": the forward projections of a float32 SVGP layer with bf16 matrix-core products
    (bf16 operands, float32 accumulation, float32 A / C; csrc/gemm_bf16.hip), column statistics in the epilogues.

    kernel_inputs=None (settings.forward_precision('bf16')): A = W Kzx runs as in `svgp_project` (float32, float64
        accumulation with W64f, int8 with W64f and i8_inputs, Kzx then optional) -- its terms |W||Kzx| ~ 1e2 cancel to O(1),
        which bf16 operands cannot carry (measured at M = 2048: 160 % error on the layer outputs) -- and C = Lq^T A, whose
        operands are O(1), runs on the bf16 cores from a bf16 transposed copy of A.
    kernel_inputs=(Z, x, ls, os) (forward_precision('bf16_all')): BOTH products in bf16, Kxz written in bf16 by the build
        kernel (nsgp_rbf_build_t_bf16) -- configs[4] to the letter; a throughput figure, not a usable numerical mode.
    kernel_nu (with i8_inputs only): the kernel of (Z, x, ls, os) is Matern with that nu; the bf16 Kxz build is RBF-only.
    Returns A, C, mean, var (float32).  M must be a multiple of 8."""
    kernel_nu = _kernel_nu_arg(kernel_nu, 'bf16' if kernel_inputs is not None else 'i8' if i8_inputs is not None else 'dense',
                               'svgp_project_bf16')
    ref = _chk(Lq, m, base, Kzx)
    if ref.dtype != torch.float32:
        raise BackendError('svgp_project_bf16: float32 layers only')
    if Kzx is None and (i8_inputs is None or W64f is None or kernel_inputs is not None):
        raise BackendError('svgp_project_bf16: Kzx=None needs i8_inputs and W64f (mode bf16)')
    first = 'bf16' if kernel_inputs is not None else 'f32' if W64f is None else 'f64acc' if i8_inputs is None else 'i8'
    kernel_nu = _kernel_nu_arg(kernel_nu, first, 'svgp_project_bf16')      # (i8_inputs without W64f: not the int8 product)
    kin = dims = None
    if first in ('bf16', 'i8'):
        kin, dims = _kernel_inputs_args(kernel_inputs if first == 'bf16' else i8_inputs, ref, 'svgp_project_bf16')
    if Kzx is not None:
        Kzx, kdims = _c(Kzx), dims
        dims = tuple(Kzx.shape)
    batch, M, n = dims
    if M % 8 != 0:
        raise BackendError('svgp_project_bf16: M must be a multiple of 8')
    Lq, m, base = _c(Lq), _c(m), _c(base.reshape(-1))
    if Lq.shape != (batch, M, M) or m.shape != (batch, M) or base.shape != (batch,) \
            or (Kzx is not None and kdims not in (None, dims)):          # (Z, x, ls, os) of another size than Kzx
        raise BackendError('svgp_project_bf16: shapes')
    plan = svgp_projection_plan(M, n, batch, ref.dtype, first, 'bf16')
    return _run_projection(plan, (batch, M, n), _c(W if W64f is None else W64f), Kzx, kin, Lq, m, base, base_add, affine,
                           i8_kzx_out, kernel_nu)


def svgp_project_bwd(Lq, m, A, C, gmean, gvar, affine=None):
    """Adjoints of svgp_project w.r.t. A (total, through C as well), Lq and m:
    Abar = 2 (Lq C) diag(gvar) + m gmean^T - 2 A diag(gvar);  Lqbar = tril(A diag(2 gvar) C^T);  mbar = A gmean.
    Also returns basebar = rowsum(gvar):(b,) and, with `affine` = (x, w, c) as in svgp_project, the gradients
    (wbar, cbar) of the affine prior mean in the shapes of w / c (None where w / c is None)."""
    ref = _chk(Lq, m, A, C, gmean, gvar)
    Lq, m, A, C, gmean, gvar = _c(Lq), _c(m), _c(A), _c(C), _c(gmean), _c(gvar)
    batch, M, n = A.shape
    if C.shape != A.shape or Lq.shape != (batch, M, M) or m.shape != (batch, M) or gmean.shape != (batch, n) \
            or gvar.shape != (batch, n):
        raise BackendError('svgp_project_bwd: shapes')
    lib = _lib.load()
    sfx, st = _sfx(ref), _stream()
    Abar = torch.empty_like(A)
    sink = grad_sink(Lq)                     # the optimiser's gradient bucket, when Lq is a registered parameter
    Lqbar, lq_beta = (torch.empty_like(Lq), 0.0) if sink is None else (sink[0], 1.0 if sink[1] else 0.0)
    mbar = torch.empty_like(m)
    flops = 1.0 * M * M * n * batch
    basebar = torch.empty(batch, dtype=ref.dtype, device=ref.device)
    x, sxb, D, w, swb, c, scb = _affine_args(affine, batch, n, ref)
    shared, wbar, cbar = _affine_grad_outputs(affine, swb, scb, w, c, batch, D, ref)
    _lib.call(f'nsgp_rowdot_affine_{sfx}', _p(A), _p(gmean), _p(gvar), _p(x) if wbar is not None else None, sxb, D,
              shared, batch, M, n, _p(mbar), _p(basebar), _p(wbar), _p(cbar), st)
    _timed(lambda: _lib.call(f'nsgp_svgp_abar_{sfx}', _p(Lq), _p(C), _p(A), _p(m), _p(gmean), _p(gvar), batch, M, n,
                             _p(Abar), st), flops, ref.dtype)
    wsb = lib.nsgp_svgp_lqbar_workspace(batch, M, n, ref.element_size())
    ws = _ws(wsb, ref.device) if wsb else None
    _timed(lambda: _lib.call(f'nsgp_svgp_lqbar_acc_{sfx}', _p(A), _p(C), _p(gvar), batch, M, n, lq_beta, _p(Lqbar), _p(ws),
                             ws.numel() if ws is not None else 0, st), flops, ref.dtype)
    # accumulated onto a gradient that is already p.grad: nothing to hand to autograd for Lq
    return Abar, (None if lq_beta else Lqbar), mbar, basebar, wbar, cbar


def svgp_project_diag(first, W, s2m1, m, base, base_add=0.0, affine=None, Kzx=None, Kzx64=None, kernel_inputs=None,
                      W64f=None, i8_planes=4, i8_kzx_out=None, kernel_nu=None):
    """Forward projection of a layer with a mean-field q(u) = N(m, diag(s^2)): A = W Kzx in the arithmetic `first` names
    (svgp_projection_plan; the operands of `svgp_project` / `svgp_project_bf16`: Kzx for 'f32' / 'f64acc', Kzx64 for
    'f64acc_b64', kernel_inputs = (Z, x, ls, os) for 'kzx_fused' / 'i8' / 'bf16', W64f wherever the float64 W is read),
    then ONE pass over A instead of the second product.  s2m1:(b,M) = s^2 - 1.  kernel_nu (first == 'i8' only): the kernel
    of kernel_inputs is Matern with that nu; 'kzx_fused' and 'bf16' evaluate Kzx in RBF-only paths.
    Returns A, mean = A^T m (+ the affine prior mean), var = base + base_add + sum_k s2m1_k A_kj^2, summed in float64."""
    kernel_nu = _kernel_nu_arg(kernel_nu, first, 'svgp_project_diag')
    ref = _chk(W, s2m1, m, base, Kzx)
    needs_w64 = first in ('f64acc', 'f64acc_b64', 'kzx_fused', 'i8')
    if first not in ('f32', 'bf16') and not needs_w64:
        raise BackendError(f'svgp_project_diag: unknown first product {first!r}')
    if (needs_w64 and W64f is None) or (first in ('f32', 'f64acc')) != (Kzx is not None) \
            or (first == 'f64acc_b64') != (Kzx64 is not None) or (first in ('kzx_fused', 'i8', 'bf16')) != (kernel_inputs is not None):
        raise BackendError(f'svgp_project_diag: operands of a {first!r} first product')
    kin = B = None
    if kernel_inputs is not None:
        kin, (batch, M, n) = _kernel_inputs_args(kernel_inputs, ref, 'svgp_project_diag')
        if first == 'i8' and (ref.dtype != torch.float32 or kin[0].shape[2] > 4 or not _lib.load().nsgp_i8_supported(M)):
            raise BackendError('svgp_project_diag: int8 product shapes (float32 layer, D <= 4, M <= 4096)')
    else:
        B = _c(Kzx64 if Kzx64 is not None else Kzx)
        if B.dim() != 3 or B.device != ref.device or B.dtype != (torch.float64 if Kzx64 is not None else ref.dtype):
            raise BackendError('svgp_project_diag: Kzx / Kzx64 must be (b,M,n) on the layer device')
        batch, M, n = B.shape
    W, s2m1, m, base = _c(W), _c(s2m1), _c(m), _c(base.reshape(-1))
    if W.shape != (batch, M, M) or s2m1.shape != (batch, M) or m.shape != (batch, M) or base.shape != (batch,):
        raise BackendError('svgp_project_diag: shapes')
    if W64f is not None:
        W = _w64_operand(W64f, ref, (batch, M), 'svgp_project_diag')
    plan = svgp_projection_plan(M, n, batch, ref.dtype, first, 'diag', i8_planes)
    if first == 'kzx_fused' and not svgp_kzx_fusable(W, kin[0], kin[1], n):
        raise BackendError('svgp_project_diag: the generated-Kzx product needs whole tiles (svgp_kzx_fusable)')
    A, _, mean, var = _run_projection(plan, (batch, M, n), W, B, kin, s2m1, m, base, base_add, affine, i8_kzx_out, kernel_nu)
    return A, mean, var


def svgp_project_diag_bwd(m, s2m1, A, gmean, gvar, affine=None):
    """Adjoints of svgp_project_diag: Abar = m gmean^T + 2 diag(s2m1) A diag(gvar) (the total adjoint of A), mbar = A gmean,
    tbar = rowsum(A^2 diag(gvar)) (the gradient of s^2), from ONE pass over A; basebar = rowsum(gvar):(b,) and the gradients
    (wbar, cbar) of the affine prior mean come from the rowdot launch, which reads no row of A here."""
    ref = _chk(m, s2m1, A, gmean, gvar)
    m, s2m1, A, gmean, gvar = _c(m), _c(s2m1), _c(A), _c(gmean), _c(gvar)
    batch, M, n = A.shape
    if m.shape != (batch, M) or s2m1.shape != (batch, M) or gmean.shape != (batch, n) or gvar.shape != (batch, n):
        raise BackendError('svgp_project_diag_bwd: shapes')
    sfx, st = _sfx(ref), _stream()
    if A.numel() == 0:
        raise BackendError('svgp_project_diag_bwd: empty A')
    Abar, mbar, tbar = torch.empty_like(A), torch.empty_like(m), torch.empty_like(m)
    basebar = torch.empty(batch, dtype=ref.dtype, device=ref.device)
    x, sxb, D, w, swb, c, scb = _affine_args(affine, batch, n, ref)
    shared, wbar, cbar = _affine_grad_outputs(affine, swb, scb, w, c, batch, D, ref)
    ws = _ws(_lib.load().nsgp_svgp_diag_bwd_workspace(batch, M, n), ref.device)
    _lib.call(f'nsgp_svgp_diag_bwd_{sfx}', _p(A), _p(m), _p(s2m1), _p(gmean), _p(gvar), batch, M, n, _p(Abar), _p(mbar),
              _p(tbar), _p(ws), ws.numel(), st)
    # the rows past M of rowdot_affine only (M = 0: basebar, wbar, cbar)
    _lib.call(f'nsgp_rowdot_affine_{sfx}', _p(A), _p(gmean), _p(gvar), _p(x) if wbar is not None else None, sxb, D,
              shared, batch, 0, n, _p(mbar), _p(basebar), _p(wbar), _p(cbar), st)
    return Abar, mbar, tbar, basebar, wbar, cbar


def _kl_meanfield_args(m, s2, what):
    ref = _chk(m, s2)
    m2, s2 = _c(m), _c(s2)
    if m2.dim() == 1:
        m2, s2 = m2.unsqueeze(0), s2.unsqueeze(0)
    if m2.dim() != 2 or s2.shape != m2.shape or m2.numel() == 0:
        raise BackendError(f'{what}: m, s2 must be (b,M) or (M,), not empty')
    return ref, m2, s2


def kl_meanfield_total(m, s2, scale=1.0, addin=None):
    """1-element tensor  addin + scale * sum_b KL(N(m_b, diag(s2_b)) || N(0, I));  m, s2:(b,M) or (M,)."""
    ref, m2, s2 = _kl_meanfield_args(m, s2, 'kl_meanfield_total')
    out = torch.empty(1, dtype=ref.dtype, device=ref.device)
    ws = _red_ws(ref)
    _lib.call(f'nsgp_kl_meanfield_total_acc_fwd_{_sfx(ref)}', _p(m2), _p(s2), m2.shape[0], m2.shape[1], float(scale),
              _addin_arg(ref, addin, 'kl_meanfield_total'), _p(out), _p(ws), ws.numel(), _stream())
    return out


def kl_meanfield_total_bwd(m, s2, scale, gout):
    """(gm, gs2) of kl_meanfield_total for the upstream gradient gout (a 1-element device tensor), in m's / s2's shapes."""
    ref, m2, s22 = _kl_meanfield_args(m, s2, 'kl_meanfield_total_bwd')
    _chk(ref, gout)
    gm, gs2 = torch.empty_like(m2), torch.empty_like(s22)
    _lib.call(f'nsgp_kl_meanfield_total_bwd_{_sfx(ref)}', _p(m2), _p(s22), m2.shape[0], m2.shape[1], float(scale),
              _p(_c(gout).reshape(1)), _p(gm), _p(gs2), _stream())
    return gm.reshape(m.shape), gs2.reshape(s2.shape)


def dgp_sample(mean, var, eps):
    """h[s,i,c] = mean[c,s',i] + sqrt(var[c,s',i]) eps[s,i,c]; mean/var:(b,ns,n) ns in {1,S}; eps:(S,n,b)."""
    ref = _chk(mean, var, eps)
    mean, var, eps = _c(mean), _c(var), _c(eps)
    S, n, b = eps.shape
    ns = mean.shape[1]
    if mean.shape != (b, ns, n) or var.shape != mean.shape or ns not in (1, S):
        raise BackendError('dgp_sample: shapes')
    h = torch.empty_like(eps)
    _lib.call(f'nsgp_dgp_sample_fwd_{_sfx(ref)}', _p(mean), _p(var), _p(eps), S, ns, n, b, _p(h), _stream())
    return h


def dgp_sample_bwd(var, eps, gh):
    ref = _chk(var, eps, gh)
    var, eps, gh = _c(var), _c(eps), _c(gh)
    S, n, b = eps.shape
    ns = var.shape[1]
    gmean, gvar = torch.empty_like(var), torch.empty_like(var)
    _lib.call(f'nsgp_dgp_sample_bwd_{_sfx(ref)}', _p(var), _p(eps), _p(gh), S, ns, n, b, _p(gmean), _p(gvar),
              _stream())
    return gmean, gvar


def _red_ws(ref):
    return _ws(_lib.load().nsgp_reduce_workspace(0, ref.element_size()), ref.device)


def _gauss_args(y, mu, v, noise, what):
    ref = _chk(y, mu, v, noise)
    y, mu, v = _c(y), _c(mu), _c(v)
    if mu.dim() != 2 or y.shape != (mu.shape[1],) or v.shape != mu.shape:
        raise BackendError(f'{what}: shapes')
    return ref, y, mu, v, noise.reshape(1)


def gauss_ell(y, mu, v, noise, scale, _form=''):
    """out[s] = scale * sum_i E_q log N(y_i | f_si, noise);  mu, v:(S,n)  y:(n,)  noise: 1-element tensor."""
    ref, y, mu, v, noise = _gauss_args(y, mu, v, noise, f'gauss_ell{_form}')
    S, n = mu.shape
    out = torch.empty(1 if _form else S, dtype=ref.dtype, device=ref.device)
    ws = _red_ws(ref)
    _lib.call(f'nsgp_gauss_ell{_form}_fwd_{_sfx(ref)}', _p(y), _p(mu), _p(v), _p(noise), S, n, float(scale), _p(out), _p(ws),
              ws.numel(), _stream())
    return out


def gauss_ell_bwd(y, mu, v, noise, scale, gout, need_noise=True, _form=''):
    """(gmu, gv, gnoise or None) of gauss_ell for the upstream gradient gout:(S,), a device tensor."""
    ref, y, mu, v, noise = _gauss_args(y, mu, v, noise, f'gauss_ell{_form}_bwd')
    _chk(ref, gout)
    S, n = mu.shape
    if gout.numel() != (1 if _form else S):
        raise BackendError(f'gauss_ell{_form}_bwd: gout must have {"1 element" if _form else "S elements"}')
    gmu, gv = torch.empty_like(mu), torch.empty_like(mu)
    gn = torch.empty(1, dtype=ref.dtype, device=ref.device) if need_noise else None
    ws = _red_ws(ref)
    _lib.call(f'nsgp_gauss_ell{_form}_bwd_{_sfx(ref)}', _p(y), _p(mu), _p(v), _p(noise), S, n, float(scale),
              _p(_c(gout).reshape(-1)), _p(gmu), _p(gv), _p(gn), _p(ws), ws.numel(), _stream())
    return gmu, gv, gn


def gauss_ell_total(y, mu, v, noise, scale):
    """1-element tensor  scale * sum_s sum_i E_q log N(y_i | f_si, noise): gauss_ell and the sum over s as ONE reduction."""
    return gauss_ell(y, mu, v, noise, scale, _form='_total')


def gauss_ell_total_bwd(y, mu, v, noise, scale, gout, need_noise=True):
    """(gmu, gv, gnoise or None) of gauss_ell_total for the upstream gradient gout (a 1-element device tensor)."""
    return gauss_ell_bwd(y, mu, v, noise, scale, gout, need_noise, _form='_total')


GH_BERNOULLI, GH_STUDENT_T = 0, 1
GH_MAX_NODES = 64


def _gh_args(kind, y, mu, v, params, nodes, weights, what):
    """Checked operands of the Gauss-Hermite entry points: y:(n,) mu, v:(S,n); params None (Bernoulli) or the two elements
    (nu, s2) (Student-t); nodes, weights:(Q,) with 1 <= Q <= 64."""
    if kind not in (GH_BERNOULLI, GH_STUDENT_T):
        raise BackendError(f'{what}: kind must be 0 (Bernoulli) or 1 (Student-t), got {kind!r}')
    ref = _chk(y, mu, v, params, nodes, weights)
    y, mu, v, nodes, weights = _c(y), _c(mu), _c(v), _c(nodes), _c(weights)
    if mu.dim() != 2 or y.shape != (mu.shape[1],) or v.shape != mu.shape:
        raise BackendError(f'{what}: shapes')
    if nodes.dim() != 1 or weights.shape != nodes.shape or not 1 <= nodes.numel() <= GH_MAX_NODES:
        raise BackendError(f'{what}: nodes, weights must be (Q,) with 1 <= Q <= {GH_MAX_NODES}, got {tuple(nodes.shape)}, '
                           f'{tuple(weights.shape)}')
    if (kind == GH_STUDENT_T) != (params is not None) or (params is not None and params.numel() != 2):
        raise BackendError(f'{what}: params is (nu, s2) for Student-t and None for Bernoulli')
    return ref, y, mu, v, (None if params is None else _c(params).reshape(2)), nodes, weights


def gh_log_marginal(kind, y, mu, v, params, nodes, weights):
    """out[s,i] = log(pi^-1/2 sum_k w_k p(y_i | mu_si + sqrt(2 v_si) t_k)), a log-sum-exp per point: nsgp_gh_log_marginal."""
    ref, y, mu, v, params, nodes, weights = _gh_args(kind, y, mu, v, params, nodes, weights, 'gh_log_marginal')
    S, n = mu.shape
    out = torch.empty_like(mu)
    _lib.call(f'nsgp_gh_log_marginal_{_sfx(ref)}', int(kind), _p(y), _p(mu), _p(v), _p(params), _p(nodes), _p(weights),
              nodes.numel(), S, n, _p(out), _stream())
    return out


def _kl_whitened_args(m, Lq, what):
    ref = _chk(m, Lq)
    m2, L2 = _c(m), _c(Lq)
    if m2.dim() == 1:
        m2, L2 = m2.unsqueeze(0), L2.unsqueeze(0)
    if m2.dim() != 2 or L2.shape != (*m2.shape, m2.shape[1]):
        raise BackendError(f'{what}: m, Lq must be (b,M), (b,M,M) or (M,), (M,M)')
    return ref, m2, L2


def _grad_out(t):
    """Where the FIRST kernel to write t's gradient writes it: the optimiser's gradient bucket when t is a registered
    parameter whose range nothing has written yet (see grad_sink), else a fresh buffer."""
    sink = grad_sink(t)
    return sink[0] if (sink is not None and not sink[1]) else torch.empty_like(t)


def kl_whitened(m, Lq):
    """out[b] = KL(N(m_b, Lq_b Lq_b^T) || N(0, I));  m, Lq:(b,M), (b,M,M) or (M,), (M,M)."""
    ref, m, Lq = _kl_whitened_args(m, Lq, 'kl_whitened')
    out = torch.empty(m.shape[0], dtype=ref.dtype, device=ref.device)
    ws = _red_ws(ref)
    _lib.call(f'nsgp_kl_whitened_fwd_{_sfx(ref)}', _p(m), _p(Lq), *m.shape, _p(out), _p(ws), ws.numel(), _stream())
    return out


def kl_whitened_bwd(m, Lq, gout):
    ref, m2, L2 = _kl_whitened_args(m, Lq, 'kl_whitened_bwd')
    gm, gL = torch.empty_like(m2), torch.empty_like(L2)
    _lib.call(f'nsgp_kl_whitened_bwd_{_sfx(ref)}', _p(m2), _p(L2), *m2.shape, float(gout), _p(gm), _p(gL), _stream())
    return gm.reshape(m.shape), gL.reshape(Lq.shape)


def _addin_arg(ref, addin, what):
    if addin is None:
        return None
    _chk(ref, addin)
    if addin.numel() != 1:
        raise BackendError(f'{what}: addin must be a scalar')
    return _p(_c(addin).reshape(1))


def kl_whitened_total(m, Lq, scale=1.0, addin=None):
    """1-element tensor  addin + scale * sum_b KL(N(m_b, Lq_b Lq_b^T) || N(0, I))  (addin: optional scalar tensor, so the
    terms of an objective chain without separate additions)."""
    ref, m2, L2 = _kl_whitened_args(m, Lq, 'kl_whitened_total')
    if m2.shape[0] == 0:
        raise BackendError('kl_whitened_total: empty batch')
    out = torch.empty(1, dtype=ref.dtype, device=ref.device)
    ws = _red_ws(ref)
    _lib.call(f'nsgp_kl_whitened_total_acc_fwd_{_sfx(ref)}', _p(m2), _p(L2), *m2.shape, float(scale),
              _addin_arg(ref, addin, 'kl_whitened_total'), _p(out), _p(ws), ws.numel(), _stream())
    return out


def kl_whitened_total_bwd(m, Lq, scale, gout):
    """(gm, gLq) of kl_whitened_total for the upstream gradient gout (a 1-element device tensor), in m's / Lq's shapes."""
    ref, m2, L2 = _kl_whitened_args(m, Lq, 'kl_whitened_total_bwd')
    _chk(ref, gout)
    gm, gL = torch.empty_like(m2), _grad_out(L2)
    _lib.call(f'nsgp_kl_whitened_total_bwd_{_sfx(ref)}', _p(m2), _p(L2), *m2.shape, float(scale), _p(_c(gout).reshape(1)),
              _p(gm), _p(gL), _stream())
    return gm.reshape(m.shape), gL.reshape(Lq.shape)


def philox_normal(seed, stream_id, row0, S, n, b, dtype=torch.float32, device='cuda', step_dev=None):
    """eps:(S,n,b) standard normals keyed by (seed, stream_id, global row, sample, column).  `step_dev`
    (1-element int64 device tensor) replaces the high word of stream_id on the device (graph replays)."""
    eps = torch.empty((S, n, b), dtype=dtype, device=device)
    if not eps.is_cuda:
        raise BackendError('philox_normal: CUDA device required')
    with torch.cuda.device(eps.device):
        _lib.call(f'nsgp_philox_normal_{_sfx(eps)}', ctypes.c_uint64(seed), ctypes.c_uint64(stream_id),
                  _p(step_dev), row0, S, n, b, _p(eps), _stream())
    return eps


def adam_step_(p, g, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0, step_dev=None):
    _chk(p, g, exp_avg, exp_avg_sq)
    if p.dtype != torch.float32 or not all(t.is_contiguous() for t in (p, g, exp_avg, exp_avg_sq)):
        raise BackendError('adam_step_: contiguous float32 flat buffers expected')
    _lib.call('nsgp_adam_step_f32', _p(p), _p(g), _p(exp_avg), _p(exp_avg_sq), p.numel(), float(lr), float(beta1),
              float(beta2), float(eps), int(step), _p(step_dev), float(grad_scale), _stream())
    return p


# --------------------------------------------------------------------------------------------
# autograd Functions
# --------------------------------------------------------------------------------------------
class GibbsKernelFn(torch.autograd.Function):
    """K = os * Gibbs(x1,x2;ell1,ell2) + diag_add*I  (GibbsKernel.forward under GibbsSafeScaleKernel,
    models/gibbs_kernels.py:135-168).  Pass the same tensor as ell1 and ell2 for K_xx: autograd then
    sums both roles.  nu = None: the squared-exponential kernel; 0.5, 1.5, 2.5: its Matern form."""

    @staticmethod
    def forward(ctx, x1, x2, ell1, ell2, outputscale, diag_add, nu=None):
        # a host-number outputscale (gibbs_build takes one) is no variable: it stays in ctx and has no gradient
        os_t = torch.is_tensor(outputscale)
        ctx.save_for_backward(x1, x2, ell1, ell2, outputscale if os_t else None)
        ctx.os_host = None if os_t else outputscale
        ctx.nu = nu
        ctx.has_diag = diag_add is not None
        ctx.diag_shape = diag_add.shape if torch.is_tensor(diag_add) else None
        return gibbs_build(x1, x2, ell1, ell2, outputscale, diag_add, nu=nu)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x1, x2, ell1, ell2, outputscale = ctx.saved_tensors
        need_x = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        os_ = outputscale if outputscale is not None else ctx.os_host
        g_l1, g_l2, g_x1, g_x2, g_os = gibbs_build_bwd(x1, x2, ell1, ell2, os_, G, need_x=need_x, nu=ctx.nu)
        g_diag = None
        if ctx.has_diag and ctx.needs_input_grad[5]:
            g_diag = torch.diagonal(G).sum().reshape(ctx.diag_shape if ctx.diag_shape is not None else ())
        g_osr = None
        if outputscale is not None and ctx.needs_input_grad[4]:
            g_osr = g_os.reshape(outputscale.shape)
        return (g_x1 if ctx.needs_input_grad[0] else None, g_x2 if ctx.needs_input_grad[1] else None,
                g_l1 if ctx.needs_input_grad[2] else None, g_l2 if ctx.needs_input_grad[3] else None,
                g_osr, g_diag, None)


def _sum_shared(g_x, x, needed):
    """Per-batch input gradient (batch,n,D) -> gradient of x: summed over the batch when x:(n,D) was shared."""
    if not needed:
        return None
    return g_x.sum(0) if x.dim() == 2 else g_x


def _ard_fn_backward(ctx, build_bwd, extra, G):
    """backward of the stationary ARD Functions (saved: x1, x2, ls, os_): the gradients of those four inputs."""
    x1, x2, ls, os_ = ctx.saved_tensors
    n1g, n2g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    g_x1, g_x2, g_ls, g_os = build_bwd(x1, x2, ls, os_, *extra, G, need_x1=n1g, need_x2=n2g)
    return _sum_shared(g_x1, x1, n1g), _sum_shared(g_x2, x2, n2g), g_ls.reshape(ls.shape), g_os.reshape(os_.shape)


class RbfKernelFn(torch.autograd.Function):
    """K[b] = os[b] RBF-ARD(x1, x2; ls[b]) + diag_add I   (gpytorch ScaleKernel(RBFKernel))."""

    @staticmethod
    def forward(ctx, x1, x2, ls, os_, diag_add):
        ctx.save_for_backward(x1, x2, ls, os_)
        return rbf_build(x1, x2, ls, os_, diag_add)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        return (*_ard_fn_backward(ctx, rbf_build_bwd, (), G), None)


class MaternKernelFn(torch.autograd.Function):
    """K[b] = os[b] Matern_nu-ARD(x1, x2; ls[b]) + diag_add I   (gpytorch ScaleKernel(MaternKernel(nu)))."""

    @staticmethod
    def forward(ctx, x1, x2, ls, os_, nu, diag_add):
        ctx.save_for_backward(x1, x2, ls, os_)
        ctx.nu = nu
        return matern_build(x1, x2, ls, os_, nu, diag_add)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        return (*_ard_fn_backward(ctx, matern_build_bwd, (ctx.nu,), G), None, None)


class RbfPeriodicKernelFn(torch.autograd.Function):
    """K[b] = os[b] RBF-ARD(x; ls_rbf[b]) Periodic(x; ls_per[b], period[b]) + diag_add I; ls_rbf / os may be None
    (gpytorch ScaleKernel(RBFKernel * PeriodicKernel), models/spatio_temporal_models.py:22,42).
    nu = None: that kernel; 0.5, 1.5, 2.5: the Matern envelope in place of the RBF one (ls_rbf is then its lengthscale and
    required) -- one node for the periodic family, as GibbsKernelFn and Ps2dKernelFn are for theirs."""

    @staticmethod
    def forward(ctx, x1, x2, ls_rbf, ls_per, period, os_, diag_add, nu=None):
        ctx.save_for_backward(x1, x2, ls_per, period, *([ls_rbf] if ls_rbf is not None else []),
                              *([os_] if os_ is not None else []))
        ctx.has = (ls_rbf is not None, os_ is not None)
        ctx.nu = nu
        if nu is not None:
            return matern_periodic_build(x1, x2, ls_rbf, ls_per, period, os_, nu, diag_add)
        return rbf_periodic_build(x1, x2, ls_rbf, ls_per, period, os_, diag_add)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x1, x2, ls_per, period, *rest = ctx.saved_tensors
        ls_rbf = rest.pop(0) if ctx.has[0] else None
        os_ = rest.pop(0) if ctx.has[1] else None
        n1g, n2g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if ctx.nu is not None:
            g_x1, g_x2, g_lr, g_lp, g_pe, g_os = matern_periodic_build_bwd(x1, x2, ls_rbf, ls_per, period, os_, ctx.nu, G,
                                                                           n1g, n2g)
        else:
            g_x1, g_x2, g_lr, g_lp, g_pe, g_os = rbf_periodic_build_bwd(x1, x2, ls_rbf, ls_per, period, os_, G, n1g, n2g)
        return (_sum_shared(g_x1, x1, n1g), _sum_shared(g_x2, x2, n2g),
                g_lr.reshape(ls_rbf.shape) if ls_rbf is not None else None, g_lp.reshape(ls_per.shape),
                g_pe.reshape(period.shape), g_os.reshape(os_.shape) if os_ is not None else None, None, None)


class Ps2dKernelFn(torch.autograd.Function):
    """Paciorek-Schervish kernel for per-point 2x2 matrices (models/multivariate_gibbs_kernel.py:98-150).
    nu = None: the squared-exponential kernel; 0.5, 1.5, 2.5: its Matern form.  x1 and x2 get no gradient."""

    @staticmethod
    def forward(ctx, x1, x2, s1, s2, jitter, nu=None):
        ctx.save_for_backward(x1, x2, s1, s2)
        ctx.jitter = jitter
        ctx.nu = nu
        return ps2d_build(x1, x2, s1, s2, jitter, nu=nu)

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x1, x2, s1, s2 = ctx.saved_tensors
        g1, g2 = ps2d_build_bwd(x1, x2, s1, s2, ctx.jitter, G, nu=ctx.nu)
        return (None, None, g1 if ctx.needs_input_grad[2] else None, g2 if ctx.needs_input_grad[3] else None, None,
                None)


def _tri_flags(ta, tb, a_lower, b_lower, out_lower):
    f = 0
    if a_lower:
        f |= GEMM_A_UPPER if ta else GEMM_A_LOWER
    if b_lower:
        f |= GEMM_B_UPPER if tb else GEMM_B_LOWER
    if out_lower:
        f |= GEMM_C_LOWER
    return f


class MatmulFn(torch.autograd.Function):
    """C = op(A) op(B) with optional lower-triangular structure of the *stored* A / B / C.
    Differentiable to any order (backward recurses through `matmul`)."""

    @staticmethod
    def forward(ctx, A, B, ta, tb, a_lower, b_lower, out_lower):
        ctx.save_for_backward(A, B)
        ctx.cfg = (ta, tb, a_lower, b_lower, out_lower)
        return gemm(A, B, ta, tb, flags=_tri_flags(ta, tb, a_lower, b_lower, out_lower))

    @staticmethod
    def backward(ctx, G):
        A, B = ctx.saved_tensors
        ta, tb, a_lower, b_lower, out_lower = ctx.cfg
        gA = gB = None
        if ctx.needs_input_grad[0]:
            if not ta:
                gA = matmul(G, B, False, not tb, out_lower, b_lower, a_lower)
            else:
                gA = matmul(B, G, tb, True, b_lower, out_lower, a_lower)
            if A.dim() == 2 and gA.dim() == 3:
                gA = gA.sum(0)
            elif A.dim() == 3 and A.shape[0] == 1 and gA.shape[0] > 1:      # batch 1 broadcast against batch nb
                gA = gA.sum(0, keepdim=True)
        if ctx.needs_input_grad[1]:
            if not tb:
                gB = matmul(A, G, not ta, False, a_lower, out_lower, b_lower)
            else:
                gB = matmul(G, A, True, ta, out_lower, a_lower, b_lower)
            if B.dim() == 2 and gB.dim() == 3:
                gB = gB.sum(0)
            elif B.dim() == 3 and B.shape[0] == 1 and gB.shape[0] > 1:
                gB = gB.sum(0, keepdim=True)
        return gA, gB, None, None, None, None, None


def matmul(A, B, ta=False, tb=False, a_lower=False, b_lower=False, out_lower=False):
    return MatmulFn.apply(A, B, ta, tb, a_lower, b_lower, out_lower)


class CholInvFn(torch.autograd.Function):
    """W = chol(K)^-1 (lower), so that K^-1 = W^T W and log|K| = -2 sum log diag W.

    Replaces psd_safe_cholesky + triangular_solve(eye, .) (models/gibbs_kernels.py:197-208) and the
    Cholesky factor / inv_matmul of gpytorch's VariationalStrategy and ExactMarginalLogLikelihood.
    Backward:  Kbar = -W^T sym(Phi(tril(Wbar) W^T)) W  with sym(Phi(B)) = (Phi(B) + Phi(B)^T)/2.
    """

    @staticmethod
    def forward(ctx, K):
        L, info = potrf(K)
        W = trtri(L)
        ctx.save_for_backward(W)
        ctx.mark_non_differentiable(info)
        return W, info

    @staticmethod
    @once_differentiable
    def backward(ctx, Wbar, _):
        (W,) = ctx.saved_tensors
        Bm = gemm(Wbar, W, False, True, flags=GEMM_A_LOWER | GEMM_B_UPPER)      # tril(Wbar) W^T
        S = chol_bwd_phi_sym(Bm)                                                 # Phi + Phi^T
        T = gemm(S, W, False, False, flags=GEMM_B_LOWER)
        return gemm(W, T, True, False, alpha=-0.5, flags=GEMM_A_UPPER)


def chol_inv(K):
    """Returns (W, info): W lower with K^-1 = W^T W; info int32 per matrix (0 = ok)."""
    return CholInvFn.apply(K)


def gibbs_kernel(x1, x2, ell1, ell2, outputscale=None, diag_add=None, nu=None):
    return GibbsKernelFn.apply(x1, x2, ell1, ell2, outputscale, diag_add, nu)


def rbf_kernel(x1, x2, ls, os_, diag_add=0.0):
    """Batched: returns (batch, n1, n2); ls:(batch,D) os:(batch,)."""
    return RbfKernelFn.apply(x1, x2, ls, os_, diag_add)


def matern_kernel(x1, x2, ls, os_, nu, diag_add=0.0):
    """Batched: returns (batch, n1, n2); ls:(batch,D) os:(batch,), nu in {0.5, 1.5, 2.5}."""
    return MaternKernelFn.apply(x1, x2, ls, os_, nu, diag_add)


def rbf_periodic_kernel(x1, x2, ls_rbf, ls_per, period, os_=None, diag_add=0.0):
    """Batched (batch, n1, n2): os * RBF-ARD(ls_rbf) * Periodic(ls_per, period); ls_rbf / os_ None = factor absent."""
    return RbfPeriodicKernelFn.apply(x1, x2, ls_rbf, ls_per, period, os_, diag_add)


def matern_periodic_kernel(x1, x2, ls_env, ls_per, period, os_=None, nu=2.5, diag_add=0.0):
    """Batched (batch, n1, n2): os * Matern_nu-ARD(ls_env) * Periodic(ls_per, period), nu in {0.5, 1.5, 2.5}; os_ None = 1."""
    _nu2(nu)
    return RbfPeriodicKernelFn.apply(x1, x2, ls_env, ls_per, period, os_, diag_add, nu)


def ps2d_kernel(x1, x2, s1, s2, jitter=1e-5, nu=None):
    return Ps2dKernelFn.apply(x1, x2, s1, s2, jitter, nu)


class GaussEllFn(torch.autograd.Function):
    """(S,) vector: scale * sum_i E_q log N(y_i | f_si, noise)   (GaussianLikelihood.expected_log_prob
    summed over the minibatch, per likelihood sample)."""

    @staticmethod
    def forward(ctx, y, mu, v, noise, scale):
        ctx.save_for_backward(y, mu, v, noise)
        ctx.scale = scale
        return gauss_ell(y, mu, v, noise, scale)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, mu, v, noise = ctx.saved_tensors
        gmu, gv, gn = gauss_ell_bwd(y, mu, v, noise, ctx.scale, g, need_noise=ctx.needs_input_grad[3])
        return None, gmu, gv, gn.reshape(noise.shape) if gn is not None else None, None


class KlWhitenedFn(torch.autograd.Function):
    """sum_b KL(N(m_b, Lq_b Lq_b^T) || N(0, I))   (whitened VariationalStrategy.kl_divergence)."""

    @staticmethod
    def forward(ctx, m, Lq):
        ctx.save_for_backward(m, Lq)
        return kl_whitened(m, Lq).sum()

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        m, Lq = ctx.saved_tensors
        gm, gL = kl_whitened_bwd(m, Lq, 1.0)
        return gm * g, gL * g


class GaussEllTotalFn(torch.autograd.Function):
    """Scalar  scale * sum_s sum_i E_q log N(y_i | f_si, noise): the (S,) vector of GaussEllFn followed by a
    mean / scaling, as ONE reduction; its backward reads the upstream gradient on the device."""

    @staticmethod
    def forward(ctx, y, mu, v, noise, scale):
        ctx.save_for_backward(y, mu, v, noise)
        ctx.scale = float(scale)
        return gauss_ell_total(y, mu, v, noise, scale).reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        y, mu, v, noise = ctx.saved_tensors
        gmu, gv, gn = gauss_ell_total_bwd(y, mu, v, noise, ctx.scale, g, need_noise=ctx.needs_input_grad[3])
        return None, gmu, gv, gn.reshape(noise.shape) if gn is not None else None, None


class KlWhitenedTotalFn(torch.autograd.Function):
    """Scalar  addin + scale * sum_b KL(N(m_b, Lq_b Lq_b^T) || N(0, I))  (kl_whitened_total); backward reads the upstream
    gradient on the device and is the first writer of Lq's range of the gradient bucket (see grad_sink)."""

    @staticmethod
    def forward(ctx, m, Lq, scale, addin=None):
        out = kl_whitened_total(m, Lq, scale, addin)
        ctx.save_for_backward(m, Lq)
        ctx.scale, ctx.has_addin = float(scale), addin is not None
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        m, Lq = ctx.saved_tensors
        gm, gL = kl_whitened_total_bwd(m, Lq, ctx.scale, g)
        return gm, gL, None, (g if ctx.has_addin else None)


class KlMeanFieldTotalFn(torch.autograd.Function):
    """Scalar  addin + scale * sum_b KL(N(m_b, diag(s2_b)) || N(0, I))  -- KlWhitenedTotalFn for a mean-field q(u);
    m, s2:(b,M) or (M,), s2 the variances.  backward reads the upstream gradient on the device.  With scale 1 and no addin
    it is the whitened VariationalStrategy.kl_divergence of a mean-field q(u)."""

    @staticmethod
    def forward(ctx, m, s2, scale=1.0, addin=None):
        out = kl_meanfield_total(m, s2, scale, addin)
        ctx.save_for_backward(m, s2)
        ctx.scale, ctx.has_addin = float(scale), addin is not None
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        m, s2 = ctx.saved_tensors
        gm, gs2 = kl_meanfield_total_bwd(m, s2, ctx.scale, g)
        return gm, gs2, None, (g if ctx.has_addin else None)


KlMeanFieldFn = KlMeanFieldTotalFn                       # apply(m, s2): the name tests/test_gpu_meanfield.py knows


class DsviObjectiveFn(torch.autograd.Function):
    """Scalar  ell_scale * sum_s sum_i E_q log N(y_i | f_si, noise) + kl_scale * sum_g sum_b KL(N(m_gb, Lq_gb Lq_gb^T) || N(0, I))
    for a list of variational groups (m_g:(b_g,M) or (M,), Lq_g:(b_g,M,M) or (M,M); one per layer, all of the same M):
    nsgp_dsvi_objective_{fwd,bwd} -- two launches forward, two backward, whatever the number of layers (the chain of
    GaussEllTotalFn + one KlWhitenedTotalFn per layer it replaces: 2 + 2 per layer forward, 3 + 1 per layer backward).
    apply(y, mu, v, noise, ell_scale, kl_scale, m_0, Lq_0, m_1, Lq_1, ...)"""

    @staticmethod
    def _arrays(ms, Ls):
        ng = len(ms)
        pm = (ctypes.c_void_p * ng)(*[t.data_ptr() for t in ms])
        pL = (ctypes.c_void_p * ng)(*[t.data_ptr() for t in Ls])
        nb = (ctypes.c_int64 * ng)(*[t.shape[0] for t in ms])
        return ng, pm, pL, nb

    @staticmethod
    def forward(ctx, y, mu, v, noise, ell_scale, kl_scale, *mL):
        ref = _chk(y, mu, v, noise, *mL)
        y, mu, v = _c(y), _c(mu), _c(v)
        S, n = mu.shape
        if y.shape != (n,) or v.shape != mu.shape or len(mL) % 2 or len(mL) > 16:
            raise BackendError('dsvi_objective: shapes')
        groups = [_kl_whitened_args(m, Lq, 'dsvi_objective')[1:] for m, Lq in zip(mL[0::2], mL[1::2])]
        ms, Ls = [m2 for m2, _ in groups], [L2 for _, L2 in groups]
        M = ms[0].shape[1] if ms else 0
        if any(m2.shape[1] != M for m2 in ms):
            raise BackendError('dsvi_objective: every group must be (b,M) / (b,M,M) with one M')
        out = torch.empty(1, dtype=ref.dtype, device=ref.device)
        lib = _lib.load()
        ws = _ws(lib.nsgp_dsvi_objective_workspace(S, n, M, sum(m2.shape[0] for m2 in ms), ref.element_size()), ref.device)
        ng, pm, pL, nb = DsviObjectiveFn._arrays(ms, Ls)
        _lib.call(f'nsgp_dsvi_objective_fwd_{_sfx(ref)}', _p(y), _p(mu), _p(v), _p(noise.reshape(1)), S, n, float(ell_scale), ng,
                  pm, pL, nb, M, float(kl_scale), _p(out), _p(ws), ws.numel(), _stream())
        ctx.save_for_backward(y, mu, v, noise, *ms, *Ls)
        ctx.cfg = (float(ell_scale), float(kl_scale), len(ms), [(m.shape, Lq.shape) for m, Lq in zip(mL[0::2], mL[1::2])])
        return out.reshape(())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ell_scale, kl_scale, ng, shapes = ctx.cfg
        y, mu, v, noise, *rest = ctx.saved_tensors
        ms, Ls = rest[:ng], rest[ng:]
        S, n = mu.shape
        M = ms[0].shape[1] if ms else 0
        gmu, gv = torch.empty_like(mu), torch.empty_like(mu)
        need_noise = ctx.needs_input_grad[3]
        gn = torch.empty(1, dtype=mu.dtype, device=mu.device) if need_noise else None
        gms, gLs = [torch.empty_like(m2) for m2 in ms], [_grad_out(L2) for L2 in Ls]
        lib = _lib.load()
        ws = _ws(lib.nsgp_dsvi_objective_workspace(S, n, 0, 0, mu.element_size()), mu.device)
        _, pm, pL, nb = DsviObjectiveFn._arrays(ms, Ls)
        pgm = (ctypes.c_void_p * ng)(*[t.data_ptr() for t in gms])
        pgL = (ctypes.c_void_p * ng)(*[t.data_ptr() for t in gLs])
        _lib.call(f'nsgp_dsvi_objective_bwd_{_sfx(mu)}', _p(y), _p(mu), _p(v), _p(noise.reshape(1)), S, n, ell_scale, ng, pm, pL,
                  nb, M, kl_scale, _p(_c(g).reshape(1)), _p(gmu), _p(gv), _p(gn), pgm, pgL, _p(ws), ws.numel(), _stream())
        grads = []
        for gm, gL, (sm, sL) in zip(gms, gLs, shapes):
            grads += [gm.reshape(sm), gL.reshape(sL)]
        return (None, gmu, gv, gn.reshape(noise.shape) if gn is not None else None, None, None, *grads)


class DgpSampleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mean, var, eps):
        ctx.save_for_backward(var, eps)
        return dgp_sample(mean, var, eps)

    @staticmethod
    @once_differentiable
    def backward(ctx, gh):
        var, eps = ctx.saved_tensors
        gm, gv = dgp_sample_bwd(var, eps, gh)
        return gm, gv, None
