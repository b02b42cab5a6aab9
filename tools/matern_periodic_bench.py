"""Event-timed ScaleKernel(MaternKernel(nu) * PeriodicKernel()) at D = 1: the fused launch against the generic product path.

    python tools/matern_periodic_bench.py [--n 4096 5676] [--dtype f32 f64] [--nu 0.5 1.5 2.5] [--runs 7] [--reps 20]

Both variants evaluate the SAME kernel object.  `fused` is what ProductKernel does with the pair now: one launch of
ops.matern_periodic_kernel with the outputscale folded in (forward), one tile pass backward.  `generic` is what it did
before the pair was recognised (ProductKernel._rbf_periodic answering None): the Matern build, the periodic build, a torch
multiply and a torch outputscale multiply forward; two tile backward passes plus the torch products backward.
Passes: `fwd` (the dense matrix under no_grad) and `fwdbwd` (the matrix, then K.backward(G) into the four parameters).

The two variants alternate: `--runs` runs of each in one process, a run being `--warmup` untimed and `--reps` timed
evaluations, each between its own pair of events, reported as the median ms.  One JSON line per (case, variant, run), then
one summary line per case with the median over runs of each variant and the generic variant's min-max spread.
"""
import argparse
import json
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', nargs='+', type=int, default=[4096, 5676])
    ap.add_argument('--dtype', nargs='+', default=['f32', 'f64'], choices=['f32', 'f64'])
    ap.add_argument('--nu', nargs='+', type=float, default=[0.5, 1.5, 2.5])
    ap.add_argument('--passes', nargs='+', default=['fwd', 'fwdbwd'], choices=['fwd', 'fwdbwd'])
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nonstationary-precip_amd'))
    from nsgp.gp.kernels import MaternKernel, PeriodicKernel, ProductKernel, ScaleKernel
    torch.cuda.set_device(0)
    recognise = ProductKernel._rbf_periodic

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
        return statistics.median(ts)

    for dts in args.dtype:
        dt = torch.float32 if dts == 'f32' else torch.float64
        for n in args.n:
            g = torch.Generator().manual_seed(n)
            x = (3.0 * torch.randn(n, 1, generator=g, dtype=torch.float64)).to(dt).cuda()
            G = torch.randn(n, n, dtype=dt, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
            for nu in args.nu:
                kern = ScaleKernel(MaternKernel(nu=nu) * PeriodicKernel()).to(dt).cuda()
                params = list(kern.parameters())

                def fwd():
                    with torch.no_grad():
                        return kern(x).evaluate()

                def fwdbwd():
                    for p in params:
                        p.grad = None
                    kern(x).evaluate().backward(G)
                for ps in args.passes:
                    fn = fwd if ps == 'fwd' else fwdbwd
                    ms = {'fused': [], 'generic': []}
                    for run in range(args.runs):
                        for variant in ('generic', 'fused'):
                            ProductKernel._rbf_periodic = recognise if variant == 'fused' else (lambda self: None)
                            try:
                                t = timed(fn)
                            finally:
                                ProductKernel._rbf_periodic = recognise
                            ms[variant].append(t)
                            print(json.dumps({'kernel': f'matern{nu}_periodic', 'variant': variant, 'pass': ps, 'dtype': dts,
                                              'n': n, 'run': run, 'ms': round(t, 4), 'reps': args.reps}), flush=True)
                    fu, ge = statistics.median(ms['fused']), statistics.median(ms['generic'])
                    print(json.dumps({'summary': f'matern{nu}_periodic', 'pass': ps, 'dtype': dts, 'n': n,
                                      'fused_ms': round(fu, 4), 'generic_ms': round(ge, 4),
                                      'generic_min_ms': round(min(ms['generic']), 4),
                                      'generic_max_ms': round(max(ms['generic']), 4),
                                      'fused_min_ms': round(min(ms['fused']), 4), 'fused_max_ms': round(max(ms['fused']), 4),
                                      'speedup': round(ge / fu, 3), 'runs': args.runs}), flush=True)
            del G


if __name__ == '__main__':
    main()
