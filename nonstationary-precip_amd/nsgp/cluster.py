"""k-means inducing points on the device: Lloyd's algorithm over `ops.kmeans_assign` / `ops.kmeans_update` (csrc/kmeans.hip).

`kmeans_inducing_points(n_inducing, X)` has the call shape of the helper the reference picks its inducing points with
(pm.gp.util.kmeans_inducing_points at experiments/spatial_exp.py:153: whiten, scipy.cluster.vq.kmeans from distinct
observations, un-whiten).  This is set-up code: one scalar comes back to the host per iteration.  Results are deterministic:
equal inputs and seed give equal bits.
"""
from typing import NamedTuple

import torch

from . import ops
from ._lib import BackendError


class KMeansResult(NamedTuple):
    centers: torch.Tensor      # (M, D), dtype and device of x
    labels: torch.Tensor       # (n,) int32: the nearest returned centre of every point
    inertia: float             # sum of squared distances to it (in whitened units when whiten=True)
    n_iter: int                # Lloyd iterations (assign + update) of the returned restart
    counts: torch.Tensor       # (M,) int32: points per returned centre


def _check(x, M, init, n_init, max_iter, tol):
    if not torch.is_tensor(x) or x.dim() != 2 or not x.is_floating_point():
        raise ValueError('kmeans: x must be a floating-point (n, D) tensor')
    n, D = x.shape
    if n < 1 or D < 1:
        raise ValueError(f'kmeans: x is empty: {tuple(x.shape)}')
    if int(M) != M or M < 1:
        raise ValueError(f'kmeans: M must be an integer >= 1, got {M!r}')
    if n_init < 1 or max_iter < 1 or not tol >= 0:
        raise ValueError(f'kmeans: n_init >= 1, max_iter >= 1 and tol >= 0 expected, got {n_init}, {max_iter}, {tol}')
    if isinstance(init, str):
        if init != 'random':
            raise ValueError(f"kmeans: init must be 'random' or an (M, D) tensor, got {init!r}")
        if M > n:
            raise ValueError(f'kmeans: M = {M} distinct observations asked of n = {n} points')
    else:
        if not torch.is_tensor(init) or tuple(init.shape) != (M, D) or init.dtype != x.dtype:
            raise ValueError(f'kmeans: init must be an ({M}, {D}) {x.dtype} tensor')
        if not bool(torch.isfinite(init).all()):
            raise ValueError('kmeans: init has non-finite entries')
    if not bool(torch.isfinite(x).all()):
        raise ValueError('kmeans: x has non-finite entries')


def _lloyd(x, c, max_iter, thresh):
    """(centres, labels, counts, inertia, n_iter) from the initial centres c."""
    labels = d2 = None
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        labels, d2 = ops.kmeans_assign(x, c, labels, d2)
        c, _, stats = ops.kmeans_update(x, labels, d2, c)
        if float(stats[1]) <= thresh:                     # the one read-back of the iteration
            break
    labels, d2 = ops.kmeans_assign(x, c, labels, d2)      # labels, counts and inertia of the RETURNED centres
    # A whole update pass for two small results (its centres are dropped): the counts and the inertia then come from the
    # kernels' own fixed summation order, so they are deterministic and are the figures a further iteration would see.
    _, counts, stats = ops.kmeans_update(x, labels, d2, c)
    return c, labels, counts, float(stats[0]), n_iter


def kmeans(x, M, *, init='random', n_init=1, max_iter=100, tol=1e-4, seed=0, whiten=False):
    """Lloyd's k-means of the rows of x:(n, D) (CUDA, float32 or float64) into M clusters -> KMeansResult.

    init      'random': the rows torch.randperm(n, generator=<CPU generator seeded with seed + restart>)[:M] of x (distinct
              observations), or an (M, D) tensor of x's dtype.
    loop      assign, then update; stops when sum_k |c_new_k - c_old_k|^2 <= tol * mean_d var(x_d) (scikit-learn's rule; tol=0
              stops only at a fixed point) or after max_iter iterations; one more assign then makes labels, counts and inertia
              those of the returned centres.  An empty cluster keeps its centre (it is not relocated).
    n_init    restarts of a 'random' init; the lowest inertia is kept, the first on a tie.
    whiten    cluster x / std(x, 0) (a zero deviation counts as 1) and multiply the centres back.
    Raises ValueError for a bad argument or non-finite data, BackendError for CPU tensors."""
    _check(x, M, init, n_init, max_iter, tol)
    if not x.is_cuda or (torch.is_tensor(init) and not init.is_cuda):
        raise BackendError('kmeans needs CUDA (ROCm) tensors: the HIP backend is the only backend (no CPU fallback).')
    M = int(M)
    x = x.detach()
    scale = None
    if whiten:
        scale = x.std(0, unbiased=False)
        scale = torch.where(scale == 0, torch.ones_like(scale), scale)
        x = x / scale
    thresh = float(tol) * float(x.double().var(0, unbiased=False).mean())
    best = None
    for restart in range(1 if torch.is_tensor(init) else int(n_init)):
        if torch.is_tensor(init):
            c = init.detach() / scale if whiten else init.detach().clone()
        else:
            g = torch.Generator().manual_seed(int(seed) + restart)
            c = x[torch.randperm(x.shape[0], generator=g)[:M].to(x.device)]
        run = _lloyd(x, c.contiguous(), int(max_iter), thresh)
        if best is None or run[3] < best[3]:
            best = run
    c, labels, counts, inertia, n_iter = best
    return KMeansResult(c * scale if whiten else c, labels, inertia, n_iter, counts)


def kmeans_inducing_points(n_inducing, X, *, seed=0, **kw):
    """The (n_inducing, D) k-means centres of X, whitened as the reference's helper does (experiments/spatial_exp.py:153).
    A tensor stays a tensor on its device; anything array-like is clustered on the current GPU in float64 and comes back
    as a float64 numpy array.  Further keywords go to `kmeans`."""
    kw.setdefault('whiten', True)
    if torch.is_tensor(X):
        return kmeans(X, n_inducing, seed=seed, **kw).centers
    import numpy as np
    if not torch.cuda.is_available():
        raise BackendError('kmeans_inducing_points needs a GPU: the HIP backend is the only backend (no CPU fallback).')
    x = torch.as_tensor(np.asarray(X, dtype=np.float64)).cuda()
    return kmeans(x, n_inducing, seed=seed, **kw).centers.cpu().numpy()
