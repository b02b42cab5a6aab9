"""Event-timed pairwise builds at N = 4096 and 16384, D = 2, batch 1: one JSON line per case.

    python tools/matern_bench.py [--tree PATH] [--kernels matern gibbs gibbs_matern rbf] [--n 4096 16384] [--dtype f32 f64]

Cases: `matern` (nu = 1/2, 3/2, 5/2), `gibbs` (ops.gibbs_build with an outputscale), `gibbs_matern` (the same call with
nu = 1/2, 3/2, 5/2: the non-stationary Matern kernel) and `rbf`, each as the forward build alone (`fwd`) and as forward +
backward (`fwdbwd`, the backward of K(x, x) with every gradient).  --tree imports nsgp from another checkout of this
repository (e.g. a parent commit's, for a baseline; name only the kernels that checkout has).

Each case: `--warmup` untimed launches, then `--reps` timed launches, each between its own pair of events; the line
reports the median ms.  TB/s uses the algorithmic bytes of csrc/pairwise.hip's header, s (n1 n2 + 2 D (n1 + n2)) for
the forward; the forward + backward counts the n^2 matrix twice (K written, G read): s (2 n1 n2 + 4 D (n1 + n2)).
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--kernels', nargs='+', default=['matern', 'gibbs', 'gibbs_matern', 'rbf'],
                    choices=['matern', 'gibbs', 'gibbs_matern', 'rbf'])
    ap.add_argument('--n', nargs='+', type=int, default=[4096, 16384])
    ap.add_argument('--dtype', nargs='+', default=['f32', 'f64'], choices=['f32', 'f64'])
    ap.add_argument('--passes', nargs='+', default=['fwd', 'fwdbwd'], choices=['fwd', 'fwdbwd'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--tag', default='')
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.tree), 'nonstationary-precip_amd'))
    from nsgp import ops
    torch.cuda.set_device(0)
    D = 2
    for dts in args.dtype:
        dt = torch.float32 if dts == 'f32' else torch.float64
        s = torch.tensor([], dtype=dt).element_size()
        for n in args.n:
            g = torch.Generator().manual_seed(n)
            x = torch.randn(n, D, generator=g, dtype=torch.float64).to(dt).cuda()
            ell = torch.exp(0.3 * torch.randn(D, n, generator=g, dtype=torch.float64) + math.log(0.3)).to(dt).cuda()
            ls = torch.tensor([[0.5, 0.7]], dtype=dt, device='cuda')
            os_ = torch.tensor([0.8], dtype=dt, device='cuda')
            K = torch.empty(1, n, n, dtype=dt, device='cuda')
            G = torch.randn(n, n, dtype=dt, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
            cases = []
            for k in args.kernels:
                if k == 'matern':
                    for nu in (0.5, 1.5, 2.5):
                        cases.append((f'matern{nu}',
                                      lambda nu=nu: ops.matern_build(x, x, ls, os_, nu, out=K),
                                      lambda nu=nu: ops.matern_build_bwd(x, x, ls, os_, nu, G)))
                elif k == 'gibbs':
                    cases.append(('gibbs', lambda: ops.gibbs_build(x, x, ell, ell, outputscale=os_, out=K[0]),
                                  lambda: ops.gibbs_build_bwd(x, x, ell, ell, os_, G, need_x=True)))
                elif k == 'gibbs_matern':
                    for nu in (0.5, 1.5, 2.5):
                        cases.append((f'gibbs_matern{nu}',
                                      lambda nu=nu: ops.gibbs_build(x, x, ell, ell, outputscale=os_, out=K[0], nu=nu),
                                      lambda nu=nu: ops.gibbs_build_bwd(x, x, ell, ell, os_, G, need_x=True, nu=nu)))
                else:
                    cases.append(('rbf', lambda: ops.rbf_build(x, x, ls, os_, out=K),
                                  lambda: ops.rbf_build_bwd(x, x, ls, os_, G)))
            for name, fwd, bwd in cases:
                for p in args.passes:
                    fn = fwd if p == 'fwd' else (lambda fwd=fwd, bwd=bwd: (fwd(), bwd()))
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
                    ms = statistics.median(ts)
                    nbytes = s * ((1 if p == 'fwd' else 2) * n * n + (2 if p == 'fwd' else 4) * D * (n + n))
                    print(json.dumps({'tag': args.tag, 'kernel': name, 'pass': p, 'dtype': dts, 'n': n, 'ms': round(ms, 4),
                                      'tbps': round(nbytes / (ms * 1e-3) / 1e12, 3), 'reps': args.reps}), flush=True)
            del K, G


if __name__ == '__main__':
    main()
