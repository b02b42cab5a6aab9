"""The Paciorek-Schervish builds (ops.ps2d_build / ops.ps2d_build_bwd) with nu = None (the squared-exponential kernel) and
nu = 1/2, 3/2, 5/2, forward and backward, at n1 x n2 = 5676 x 512 (BASELINE configs[2]: all rows against M = 512 inducing
points) and 4096 x 4096, float32 and float64.

    rocprofv3 --kernel-trace --stats -d OUT -o ps2d -- python tools/ps2d_matern_bench.py        kernel times (one run)
    python tools/ps2d_matern_bench.py --events                                                  event-timed calls

Every case launches its forward and its backward `--reps` times after `--warmup` untimed ones.  In the profiler's kernel
trace the kernels are told apart by their functor (PsOp / PsRadialOp<MaternRadial<nu2>>) and type, and the two shapes by
the grid: `--summarise OUT/ps2d_kernel_trace.csv` (no GPU needed) prints, per kernel and grid, the number of dispatches
and the median / min / max duration in microseconds.  With --events one JSON line per case: the median ms of the
event-timed call (allocation and host side included) and, for the forward, TB/s over the algorithmic bytes
s (n1 n2 + 6 (n1 + n2)).
"""
import argparse
import json
import os
import statistics
import sys

import torch

SHAPES = {'cfg2': (5676, 512), 'square': (4096, 4096)}


def summarise(path):
    """Per (kernel, grid) of a rocprofv3 kernel trace: dispatches, median / min / max duration in microseconds."""
    import csv
    import re
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r['Kernel_Name']
        if 'pairwise_' not in name and 'reduce_all_kernel' not in name:
            continue
        # "void (anonymous namespace)::kernel<T, Op>(arguments)" -> "kernel<T, Op>"
        name = re.sub(r'^void ', '', name.replace('(anonymous namespace)::', '')).split('(')[0]
        grid = 'x'.join(r[f'Grid_Size_{a}'] for a in 'XYZ')
        rows.setdefault((name, grid), []).append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    print('kernel,grid,dispatches,median_us,min_us,max_us')
    for (name, grid), ts in sorted(rows.items()):
        print(f'"{name}",{grid},{len(ts)},{statistics.median(ts):.2f},{min(ts):.2f},{max(ts):.2f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', nargs='+', default=list(SHAPES), choices=list(SHAPES))
    ap.add_argument('--dtype', nargs='+', default=['f32', 'f64'], choices=['f32', 'f64'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--events', action='store_true')
    ap.add_argument('--summarise', metavar='KERNEL_TRACE_CSV')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nonstationary-precip_amd'))
    from nsgp import ops
    from models.multivariate_gibbs_kernel import _sigma
    torch.cuda.set_device(0)
    Dm = torch.tensor([[0.7, 0.1], [-0.2, 0.9]], dtype=torch.float64)
    for shape in args.shape:
        n1, n2 = SHAPES[shape]
        for dts in args.dtype:
            dt = torch.float32 if dts == 'f32' else torch.float64
            g = torch.Generator().manual_seed(n1 + n2)
            x1 = torch.rand(n1, 2, generator=g, dtype=torch.float64).to(dt).cuda()
            x2 = torch.rand(n2, 2, generator=g, dtype=torch.float64).to(dt).cuda()
            s1 = _sigma(torch.randn(n1, 2, generator=g, dtype=torch.float64), Dm).to(dt).cuda()
            s2 = _sigma(torch.randn(n2, 2, generator=g, dtype=torch.float64), Dm).to(dt).cuda()
            G = torch.randn(n1, n2, generator=g, dtype=torch.float64).to(dt).cuda()
            for nu in (None, 0.5, 1.5, 2.5):
                for name, fn in (('fwd', lambda: ops.ps2d_build(x1, x2, s1, s2, 1e-5, nu=nu)),
                                 ('bwd', lambda: ops.ps2d_build_bwd(x1, x2, s1, s2, 1e-5, G, nu=nu))):
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
                    if args.events:
                        ms = statistics.median(ts)
                        row = {'kernel': 'ps2d' if nu is None else f'ps2d_matern{nu}', 'pass': name, 'dtype': dts,
                               'n1': n1, 'n2': n2, 'ms': round(ms, 4), 'reps': args.reps}
                        if name == 'fwd':
                            nbytes = x1.element_size() * (n1 * n2 + 6 * (n1 + n2))
                            row['tbps'] = round(nbytes / (ms * 1e-3) / 1e12, 3)
                        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
