"""Step time of the headline DSVI model with RBF layers and with Matern layers, measured in one process, alternating.

The headline shape of bench.py: 2-layer deep GP (one hidden layer of two GPs + the last layer), M = 1024 inducing points,
S = 10 samples, minibatch 4096, float32, default settings; the step is bench.py's one-GPU step (forward + objective +
backward + FusedAdam, Philox noise keyed by the device step counter) replayed as a hipGraph.  A sample is the wall time
of a run of steps that lasts at least `--seconds`, between two device synchronisations, divided by the number of steps;
the samples of the models are taken in turn (rbf, 0.5, 1.5, 2.5, rbf, ...), and the median, the extremes and
(max - min) / median of each model's samples are reported as one JSON line.

    python tools/matern_dsvi_step_time.py                       # nu=None and every nu of this tree
    python tools/matern_dsvi_step_time.py --nus rbf --root /path/to/another/checkout
        the RBF model of another checkout (built there), e.g. the parent commit: same code path of this script
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/matern_dsvi_step_time.py --nus 1.5 --profile-steps 20
        eager steps only, no timing: the per-kernel times come from the trace
"""
import argparse
import json
import os
import statistics
import sys
import time

M_INDUCING, S_SAMPLES, BATCH, N_DATA, SEED = 1024, 10, 4096, 100_000, 173      # bench.py's headline constants


def parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   help='checkout whose package is timed (default: this one)')
    p.add_argument('--nus', default='rbf,0.5,1.5,2.5', help="comma-separated: 'rbf' (nu=None) and / or values of nu")
    p.add_argument('--samples', type=int, default=7)
    p.add_argument('--seconds', type=float, default=1.0, help='least duration of one sample')
    p.add_argument('--warmup', type=int, default=30, help='replayed steps before the first sample')
    p.add_argument('--profile-steps', type=int, default=0, help='run this many eager steps and exit (for a kernel trace)')
    return p


def build(name, device):
    import torch
    import models.dgps as dgps
    from nsgp.dist import PhiloxEps
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FusedAdam
    torch.manual_seed(SEED)
    kw = {} if name == 'rbf' else dict(nu=float(name))                         # (a checkout without the keyword)
    model = dgps.DeepGP(1, (N_DATA, 3), num_inducing=M_INDUCING, **kw).to(device)
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, N_DATA))
    opt = FusedAdam(model.parameters(), lr=0.01, capturable=True, grads_as_views=False)
    eps = PhiloxEps(SEED, row0=0, step_dev=opt.step_dev)
    model.train()
    return model, mll, opt, eps


def make_step(model, mll, opt, eps, x, y):
    import torch
    from nsgp.dist import dp_objective
    from nsgp.gp.module import transform_cache
    one = torch.ones((), device=x.device)

    def step():
        eps.start_step(0, row0=0)
        opt.zero_grad()
        with transform_cache():
            loss = dp_objective(mll, model(x), y, BATCH, 1, negate=True)
        loss.backward(gradient=one)
        opt.bucket.gather_grads()
        opt.step(gather=False)
        return loss.detach()
    return step


def main(argv=None):
    args = parser().parse_args(argv)
    args.root = os.path.abspath(args.root)
    for p in (os.path.join(args.root, 'nonstationary-precip_amd'), args.root):
        sys.path.insert(0, p)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('matern_dsvi_step_time: needs a GPU (there is no CPU path to time)')
    from nsgp.gp import settings
    from nsgp.graph import GraphedCallable
    dev = torch.device('cuda', torch.cuda.current_device())
    g = torch.Generator().manual_seed(SEED)
    x, y = torch.randn(BATCH, 3, generator=g).to(dev), torch.randn(BATCH, generator=g).to(dev)
    names = [n for n in args.nus.split(',') if n]
    out = {'shape': dict(M=M_INDUCING, S=S_SAMPLES, batch=BATCH, layers=2, dtype='float32'), 'root': args.root, 'models': {}}
    with settings.num_likelihood_samples(S_SAMPLES):
        steps, info, alive = {}, {}, []
        for name in names:
            model, mll, opt, eps = build(name, dev)
            step = make_step(model, mll, opt, eps, x, y)
            # a captured graph holds raw pointers into the model's and the optimiser's buffers and no reference to them:
            # they must outlive every replay (the next capture empties the allocator's cache of anything freed)
            alive.append((model, mll, opt, eps, step))
            with settings.eps_provider(eps):
                with torch.no_grad():
                    model(x)                                # draws the variational-mean initialisation (a host read)
                if args.profile_steps:
                    for _ in range(args.profile_steps):
                        step()
                    torch.cuda.synchronize()
                    continue
                graphed = GraphedCallable(step)
                for _ in range(args.warmup):
                    loss = graphed()
                torch.cuda.synchronize()
            steps[name] = graphed
            info[name] = dict(loss_after_warmup=float(loss))
        if args.profile_steps:
            return 0
        count = {}                                          # how many steps fill a sample
        for name in names:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                steps[name]()
            torch.cuda.synchronize()
            count[name] = max(20, int(args.seconds / ((time.perf_counter() - t0) / 20)) + 1)
        samples = {name: [] for name in names}
        for _ in range(args.samples):
            for name in names:                              # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(count[name]):
                    steps[name]()
                torch.cuda.synchronize()
                samples[name].append((time.perf_counter() - t0) / count[name] * 1e3)
    for name in names:
        s = samples[name]
        med = statistics.median(s)
        out['models'][name] = dict(info[name], ms_per_step_median=round(med, 4), ms_per_step_min=round(min(s), 4),
                                   ms_per_step_max=round(max(s), 4), spread_rel=round((max(s) - min(s)) / med, 4),
                                   steps_per_sample=count[name], samples=[round(v, 4) for v in s])
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
