"""The timed step is deterministic: bench.py's one-GPU step (forward + ELBO + backward + FusedAdam, Philox noise keyed by
the device step counter) run twice from the same state gives the same loss, flat gradient bucket and updated parameters
bit for bit -- eagerly, as hipGraph replays, and eager against replay.  The kernels are written without atomics (one
writer per output element, fixed reduction orders), so any difference is a bug."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timed_step_is_bitwise_reproducible():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from nsgp.dist import PhiloxEps, dp_objective
    from nsgp.gp import settings
    from nsgp.gp.module import transform_cache
    from nsgp.graph import GraphedCallable
    dev = torch.device('cuda', torch.cuda.current_device())
    x_all, y_all = bench.synthetic_grid()
    rows = torch.randperm(bench.N_DATA, generator=torch.Generator().manual_seed(bench.SEED))[:bench.BATCH]
    x_in, y_in = x_all[rows].to(dev), y_all[rows].to(dev)             # static buffers, as in bench.py
    model, mll, opt = bench.build(dev, 1)
    eps = PhiloxEps(bench.SEED, row0=0, step_dev=opt.step_dev)
    one = torch.ones((), device=dev)
    model.train()

    def whole_step():                                   # bench.py: fwd_bwd() + adam_step() at one GPU
        eps.start_step(0, row0=0)
        opt.zero_grad()
        with transform_cache():
            out = model(x_in)
            loss = dp_objective(mll, out, y_in, bench.BATCH, 1, negate=True)
        loss.backward(gradient=one)
        opt.bucket.gather_grads()
        opt.step(gather=False)
        return loss.detach()

    def state():
        return [t.detach().clone() for t in (opt.bucket.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_dev)]

    def restore(s):
        with torch.no_grad():
            for dst, src in zip((opt.bucket.flat_p, opt.exp_avg, opt.exp_avg_sq, opt.step_dev), s):
                dst.copy_(src)
        opt.steps = 0

    def outputs(loss):
        torch.cuda.synchronize()
        return dict(loss=loss.detach().clone().reshape(1), grad=opt.bucket.flat_g.detach().clone(),
                    param=opt.bucket.flat_p.detach().clone(), exp_avg_sq=opt.exp_avg_sq.detach().clone())

    def same(a, b):
        return {k: bool(torch.equal(a[k], b[k])) for k in a}

    with settings.num_likelihood_samples(bench.S_SAMPLES), settings.eps_provider(eps), settings.whiten_matmul_f64(True):
        with torch.no_grad():
            model(x_in)                                 # the first call draws the variational-mean init (bench.py does too)
        for _ in range(3):                              # a few real steps: the state is that of a model in training
            whole_step()
        s0 = state()
        s0[3].zero_()                                   # step counter 0 (the eps of every run below are the same)
        res = {}
        for k in ('eager 1', 'eager 2'):
            restore(s0)
            res[k] = outputs(whole_step())
        assert bool(torch.isfinite(res['eager 1']['loss']).all())
        g = GraphedCallable(whole_step)                 # (warm-up and capture run real steps: undone by restore)
        for k in ('replay 1', 'replay 2'):
            restore(s0)
            res[k] = outputs(g())
    pairs = {('eager 1', 'eager 2'): same(res['eager 1'], res['eager 2']),
             ('replay 1', 'replay 2'): same(res['replay 1'], res['replay 2']),
             ('eager 1', 'replay 1'): same(res['eager 1'], res['replay 1'])}
    for (a, b), eq in pairs.items():
        d = {k: float((res[a][k].double() - res[b][k].double()).abs().max()) for k in eq}
        print(f'[measured] determinism {a} vs {b}: bitwise equal {eq}; max|diff| {d}')
    for (a, b), eq in pairs.items():
        assert all(eq.values()), ((a, b), eq)
