"""k-means on the device: event-timed assign and update launches, a whole kmeans(), and two baselines in the same process.

    python tools/kmeans_bench.py [--shape 100000,1024,2 1000000,2048,2 1000000,2048,3] [--dtype f32 f64] [--reps 20]
                                 [--cdist-gib 4] [--sklearn-pairs 2e8]

Per (n, M, D, dtype), one JSON line each:
  assign / update   median ms of `--reps` launches of ops.kmeans_assign / ops.kmeans_update (three kernels), each between its
                    own pair of events, after `--warmup` untimed ones;
  cdist_argmin      the same timing of torch.cdist(x, c).argmin(1) on the same card -- what a user without the kernels would
                    write.  Skipped, and reported as skipped, where the n x M distance matrix exceeds `--cdist-gib`;
  kmeans            wall-clock seconds of nsgp.kmeans(x, M, init=init, max_iter=50, tol=0) ending in a synchronise (the
                    second of two calls), with its iteration count and inertia;
  sklearn           wall-clock seconds of KMeans(M, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=50).fit on the
                    host (the threads the environment allows), as context.  Run where n M <= `--sklearn-pairs`, skipped and
                    reported as skipped beyond (0 = never, inf = always).
x is standard normal from a seed; init is M distinct observations (the rows nsgp.kmeans would draw with seed 0).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', nargs='+', default=['100000,1024,2', '1000000,2048,2', '1000000,2048,3'])
    ap.add_argument('--dtype', nargs='+', default=['f32', 'f64'], choices=['f32', 'f64'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cdist-gib', type=float, default=4.0)
    ap.add_argument('--sklearn-pairs', type=float, default=2e8)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nonstationary-precip_amd'))
    import nsgp
    from nsgp import ops
    torch.cuda.set_device(0)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts), min(ts), max(ts)

    def emit(**kw):
        print(json.dumps(kw), flush=True)

    for shape in args.shape:
        n, M, D = (int(v) for v in shape.split(','))
        for dts in args.dtype:
            dt = torch.float32 if dts == 'f32' else torch.float64
            x = torch.randn(n, D, generator=torch.Generator().manual_seed(n + M + D), dtype=torch.float64).to(dt).cuda()
            init = x[torch.randperm(n, generator=torch.Generator().manual_seed(0))[:M].cuda()].contiguous()
            tag = dict(n=n, M=M, D=D, dtype=dts)
            labels, d2 = ops.kmeans_assign(x, init)
            med, lo, hi = timed(lambda: ops.kmeans_assign(x, init, labels, d2))
            emit(what='assign', ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), reps=args.reps,
                 gpairs_per_s=round(n * M / med / 1e6, 1), **tag)
            assign_ms = med
            med, lo, hi = timed(lambda: ops.kmeans_update(x, labels, d2, init))
            emit(what='update', ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), reps=args.reps, **tag)
            gib = n * M * x.element_size() / 2.0 ** 30
            if gib <= args.cdist_gib:
                ref = torch.cdist(x, init).argmin(1)
                agree = float((ref == labels).double().mean())
                med, lo, hi = timed(lambda: torch.cdist(x, init).argmin(1))
                emit(what='cdist_argmin', ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4), reps=args.reps,
                     labels_agree=round(agree, 6), assign_speedup=round(med / assign_ms, 2), **tag)
                del ref
            else:
                emit(what='cdist_argmin', skipped=f'distance matrix {gib:.1f} GiB > {args.cdist_gib:g} GiB', **tag)
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = nsgp.kmeans(x, M, init=init, max_iter=50, tol=0.0)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
            emit(what='kmeans', seconds=round(wall, 4), n_iter=res.n_iter, inertia=res.inertia, **tag)
            if n * M <= args.sklearn_pairs:
                from sklearn.cluster import KMeans
                xh, ih = x.cpu().numpy(), init.cpu().numpy()
                t0 = time.perf_counter()
                sk = KMeans(M, init=ih, n_init=1, algorithm='lloyd', tol=0, max_iter=50).fit(xh)
                emit(what='sklearn', seconds=round(time.perf_counter() - t0, 3), n_iter=int(sk.n_iter_),
                     inertia=float(sk.inertia_), threads=os.environ.get('OMP_NUM_THREADS'), **tag)
            else:
                emit(what='sklearn', skipped=f'n M = {n * M:.3g} > {args.sklearn_pairs:g}', **tag)
            del x, init, labels, d2


if __name__ == '__main__':
    main()
