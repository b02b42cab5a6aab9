"""Case table, input builders and the float64 restatement of Lloyd's k-means (csrc/kmeans.hip, nsgp/cluster.py).
tests/test_kmeans_cases_cpu.py checks the table and the restatement without a GPU; tests/test_gpu_kmeans.py runs every row
on the device.

`lloyd_ref` is numpy float64: squared distances as sums of squared differences in dimension order, `argmin` (the lowest
index on a tie), `bincount` means, an empty cluster keeps its centre, the stop rule shift^2 <= tol * mean_d var(x_d), and one
final assign, so that labels, counts and inertia belong to the returned centres.

Rows.  Every row runs with integer data (coordinates and centres in -4 .. 4, so points and centres repeat and distances tie;
every distance and every sum is exact in both types) and with real data (standard normal points; the centres are
observations where M <= n).  The sizes come from the kernels' own edges:
  assign   512 points per workgroup (2 per lane), centres in LDS tiles of KM_TILE = 256;
  update   points staged 512 at a time, 256 x 4 clusters per workgroup (M = 1025 needs a second group), partials summed in
           8 runs of chunks (10 chunks: runs of 2), chunks of 2 stages beyond n = 2^19 (the two BIG rows: a last chunk whose
           second stage holds one point, and one whose second stage is empty).
"""
from typing import NamedTuple

import numpy as np

KM_TILE = 256            # centres per LDS tile of the assign kernel
KM_STAGE = 512           # points per LDS block of the update kernel
EPS = {'f32': 2.0 ** -23, 'f64': 2.0 ** -52}
NP_DT = {'f32': np.float32, 'f64': np.float64}


class Case(NamedTuple):
    dtn: str
    D: int
    n: int
    M: int
    strided: bool = False

    @property
    def name(self):
        return f'{self.dtn}-D{self.D}-n{self.n}-M{self.M}' + ('-strided' if self.strided else '')


_SHAPES = [  # (D, n, M, strided)
    (1, 1, 1, False), (2, 1, 2, False), (3, 63, 63, False), (5, 64, 64, False), (1, 65, 65, False), (2, 257, 2, False),
    (3, 257, 300, False), (5, 1000, 513, False), (2, 1000, 257, True), (3, 63, 1, True), (5, 65, 300, True),
    (1, 257, 64, True), (2, 513, 64, False), (1, 512, 65, False), (2, 511, 1025, False), (3, 4700, 3, False),
]
_BIG = [Case('f32', 1, (1 << 19) + 513, 2), Case('f64', 2, (1 << 19) + 100, 3)]
CASES = [Case(dtn, *s) for dtn in ('f32', 'f64') for s in _SHAPES] + _BIG


def update_chunks(n):
    """(stages, chunks) of the update's plan: a chunk is 512 * clamp(ceil(n / 2^19), 1, 8) points."""
    stages = min(max(-(-n // (1 << 19)), 1), 8)
    return stages, -(-n // (stages * KM_STAGE))


def workspace_bytes(n, D, M):
    chunks = update_chunks(n)[1]
    return 8 * (chunks * (2 * D + 1) * M + chunks + M)


def _rng(case, tag):
    import zlib
    return np.random.default_rng(zlib.crc32(f'{case.name}/{tag}'.encode()))


def integer_inputs(case):
    """(x, c) in the row's type: integers in -4 .. 4; centre 1 repeats centre 0 and point 1 repeats point 0 where they exist."""
    g = _rng(case, 'int')
    x = g.integers(-4, 5, (case.n, case.D)).astype(NP_DT[case.dtn])
    c = g.integers(-4, 5, (case.M, case.D)).astype(NP_DT[case.dtn])
    if case.M > 1:
        c[1] = c[0]
    if case.n > 1:
        x[1] = x[0]
    return x, c


def real_inputs(case):
    """(x, c) in the row's type: standard normal points; the centres are the first M observations in a shuffled order, or
    normal draws of their own where M > n."""
    g = _rng(case, 'real')
    x = g.standard_normal((case.n, case.D)).astype(NP_DT[case.dtn])
    if case.M <= case.n:
        c = x[g.permutation(case.n)[:case.M]].copy()
    else:
        c = g.standard_normal((case.M, case.D)).astype(NP_DT[case.dtn])
    return x, c


def sq_dists(x, c):
    """(n, M) float64: sum_d (x_d - c_d)^2 added in dimension order."""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    s = np.zeros((x.shape[0], c.shape[0]))
    for d in range(x.shape[1]):
        df = x[:, d, None] - c[None, :, d]
        s = s + df * df
    return s


def assign_ref(x, c):
    """(labels int32, d2 float64): argmin takes the lowest index on a tie."""
    s = sq_dists(x, c)
    if s.shape[0] == 0:
        return np.zeros(0, np.int32), np.zeros(0)
    lab = s.argmin(1)
    return lab.astype(np.int32), s[np.arange(s.shape[0]), lab]


def update_ref(x, labels, c_old):
    """(c_new float64, counts int32): bincount means, one division; an empty cluster keeps its centre."""
    x, c_old = np.asarray(x, np.float64), np.asarray(c_old, np.float64)
    M = c_old.shape[0]
    counts = np.bincount(labels, minlength=M)
    c_new = c_old.copy()
    full = counts > 0
    for d in range(x.shape[1]):
        sums = np.bincount(labels, weights=x[:, d], minlength=M)
        c_new[full, d] = sums[full] / counts[full]
    return c_new, counts.astype(np.int32)


def exact_means(x, labels, c_old):
    """`update_ref` with every cluster sum taken exactly (math.fsum) and rounded once before the division: the float64
    mean that the 1-ulp check of the update holds the device to (a plain float64 sum of k terms is itself several ulps of
    the mean away from it where the terms cancel)."""
    import math
    x, c_new = np.asarray(x, np.float64), np.array(c_old, np.float64)
    order = np.argsort(labels, kind='stable')
    lab = np.asarray(labels)[order]
    starts = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]]) if len(lab) else np.zeros(0, int)
    ends = np.r_[starts[1:], len(lab)]
    for s, e in zip(starts, ends):
        k = lab[s]
        if 0 <= k < c_new.shape[0]:
            for d in range(x.shape[1]):
                c_new[k, d] = math.fsum(x[order[s:e], d]) / (e - s)
    return c_new


def sum_in_kernel_order(v):
    """The float64 sum of v in the order of the update's one-workgroup reduction (include/nsgp.h, KM): thread t of 256 adds
    items t, t + 256, ... in order; a xor butterfly over each wave's 64 lanes (offsets 32 .. 1); the four waves in order."""
    v = np.asarray(v, np.float64)
    a = np.zeros(256)
    for i in range(0, len(v), 256):
        seg = v[i:i + 256]
        a[:len(seg)] = a[:len(seg)] + seg
    w = a.reshape(4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def shift2_in_kernel_order(c_new, c_old):
    """sum_k |c_new_k - c_old_k|^2 as the device adds it: per cluster the rounded squares in d order, then the clusters by
    `sum_in_kernel_order`.  c_new, c_old: the values as stored (the row's type)."""
    df = np.asarray(c_new, np.float64) - np.asarray(c_old, np.float64)
    s = np.zeros(df.shape[0])
    for d in range(df.shape[1]):
        s = s + df[:, d] * df[:, d]
    return sum_in_kernel_order(s)


class LloydRef(NamedTuple):
    centers: np.ndarray
    labels: np.ndarray
    inertia: float
    n_iter: int
    counts: np.ndarray


def lloyd_ref(x, init, max_iter=100, tol=1e-4):
    x = np.asarray(x, np.float64)
    c = np.array(init, np.float64)
    thresh = tol * x.var(0).mean()
    n_iter = 0
    for n_iter in range(1, max_iter + 1):
        labels, _ = assign_ref(x, c)
        c_new, _ = update_ref(x, labels, c)
        shift2 = float(((c_new - c) ** 2).sum())
        c = c_new
        if shift2 <= thresh:
            break
    labels, d2 = assign_ref(x, c)
    return LloydRef(c, labels, float(d2.sum()), n_iter, np.bincount(labels, minlength=c.shape[0]).astype(np.int32))


# Gaussian problems of the float64 comparisons (scikit-learn on the host, kmeans() on the device): (n, M, D).  None of them
# meets an empty cluster (asserted in test_kmeans_cases_cpu.py): scikit-learn relocates an empty cluster, Lloyd here does not.
GAUSS = [(2000, 7, 2), (5000, 64, 3), (1000, 65, 1)]


def gauss_problem(n, M, D):
    """(x, init) float64: standard normal points and M distinct observations."""
    g = np.random.default_rng(1000 * n + 10 * M + D)
    x = g.standard_normal((n, D))
    return x, x[g.permutation(n)[:M]].copy()
