"""Data-parallel DSVI on the GPU product path: two ranks (gloo rendezvous, both on cuda:0 -- RCCL itself needs one
GPU per rank and is exercised by the driver's multi-GPU run) train a small DeepGP with the sharded minibatch, the
Philox noise keyed by global row, the flat-bucket all-reduce and the fused Adam step; the result must equal the
single-process run on the full minibatch (float32 round-off only).  This is the exactness claim of nsgp/dist.py,
end to end through the HIP kernels."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _run(rank, world, port, out_path, steps, staged=False):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'nonstationary-precip_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.cuda.set_device(0)
    if world > 1:
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group('gloo', rank=rank, world_size=world)
    import models.dgps as m
    from nsgp.dist import DataParallel, PhiloxEps, dp_objective, shard_bounds
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FusedAdam
    torch.manual_seed(11)
    N, D, M, S, B = 2000, 3, 48, 4, 256
    model = m.DeepGP(1, (N, D), num_inducing=M).cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, N))
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, D, generator=g).cuda()
    y = torch.randn(B, generator=g).cuda()
    lo, hi = shard_bounds(B, world, rank)
    model.train()
    plan, stage_of = None, None
    if staged:
        # staged backward (nsgp/stages.py): per-stage asynchronous all-reduces of contiguous bucket ranges
        from nsgp.stages import BackwardStages
        plan = BackwardStages()
        with settings.num_likelihood_samples(S), settings.eps_provider(PhiloxEps(173, row0=lo)), \
                settings.backward_stages(plan):
            probe = -dp_objective(mll, model(x[lo:hi]), y[lo:hi], B, world)
        stage_of = plan.final_stage_of(probe, [p for p in model.parameters() if p.requires_grad])
        assert plan.num_stages == 4                       # loss + last layer | hidden layer | whitening chain | softplus
    opt = FusedAdam(model.parameters(), lr=0.01, capturable=True, grads_as_views=False, stage_of=stage_of)
    if staged:
        names = {id(p): n for n, p in model.named_parameters()}
        by_stage = {}
        for p, k in zip(opt.bucket.params, opt.bucket.stage_index):
            by_stage.setdefault(k, []).append(names[id(p)])
        assert any('last_layer' in n and 'chol_variational_covar' in n for n in by_stage[0]), by_stage
        assert all('last_layer' not in n or 'variational' not in n for n in by_stage[1]), by_stage
        assert any('chol_variational_covar' in n for n in by_stage[1]), by_stage
        assert all('inducing_points' in n for n in by_stage[2]), by_stage
        assert all('raw_' in n for n in by_stage[3]), by_stage
        segs = sorted(opt.bucket.segments.values())
        assert segs[0][0] == 0 and segs[-1][1] == opt.bucket.numel
        assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))           # contiguous, disjoint, complete
    dp = DataParallel(opt.bucket)
    dp.broadcast_params()
    eps = PhiloxEps(173, row0=lo, step_dev=opt.step_dev)
    losses = []
    with settings.num_likelihood_samples(S), settings.eps_provider(eps):
        for _ in range(steps):
            eps.start_step(0, row0=lo)
            opt.zero_grad()
            if staged:
                with settings.backward_stages(plan):
                    loss = -dp_objective(mll, model(x[lo:hi]), y[lo:hi], B, world)
                plan.backward(loss, after_stage=dp.allreduce_stage)
                dp.wait_stages()
            else:
                loss = -dp_objective(mll, model(x[lo:hi]), y[lo:hi], B, world)
                loss.backward()
                dp.allreduce_grads()
            opt.step(gather=False)
            t = loss.detach().clone().reshape(1)
            if world > 1:
                dist.all_reduce(t)
            losses.append(float(t))
    if rank == 0:
        # parameters by NAME: the staged run lays the bucket out in a different order
        torch.save({'p': torch.cat([p.detach().reshape(-1).cpu() for _, p in sorted(model.named_parameters())]),
                    'losses': torch.tensor(losses)}, out_path)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_rank_data_parallel_training_equals_single_process(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    steps = 4
    one, two = str(tmp_path / 'one.pt'), str(tmp_path / 'two.pt')
    mp.spawn(_run, args=(1, 0, one, steps), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), two, steps), nprocs=2, join=True)
    a = torch.load(one, weights_only=True)
    b = torch.load(two, weights_only=True)
    # the ranks' objectives sum to the single-GPU loss at every step ...
    assert torch.allclose(a['losses'], b['losses'], rtol=2e-5, atol=1e-6), (a['losses'], b['losses'])
    # ... and after 4 Adam steps the parameters agree to float32 round-off (Adam's 1/sqrt(v) amplifies tiny
    # gradient differences on near-zero-gradient entries, hence the absolute tolerance of 0.2 * lr)
    assert a['losses'][-1] < a['losses'][0]
    assert float((a['p'] - b['p']).abs().max()) < 2e-3
    assert float((a['p'] - b['p']).abs().mean()) < 2e-5


def test_staged_backward_with_overlapped_exchange_equals_single_process(tmp_path):
    """The staged backward (graph cut between the layers, the whitening chain and the packed softplus; every stage's
    gradients exchanged asynchronously as one contiguous range of the bucket) trains to the same parameters as the plain
    single-process step: one rank staged == one rank plain (no node runs twice, nothing is dropped), and two staged ranks
    == one rank."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    steps = 4
    one, st1, st2 = str(tmp_path / 'one.pt'), str(tmp_path / 'st1.pt'), str(tmp_path / 'st2.pt')
    mp.spawn(_run, args=(1, 0, one, steps), nprocs=1, join=True)
    mp.spawn(_run, args=(1, 0, st1, steps, True), nprocs=1, join=True)
    mp.spawn(_run, args=(2, _free_port(), st2, steps, True), nprocs=2, join=True)
    a = torch.load(one, weights_only=True)
    for path in (st1, st2):
        b = torch.load(path, weights_only=True)
        assert torch.allclose(a['losses'], b['losses'], rtol=2e-5, atol=1e-6), (a['losses'], b['losses'])
        assert float((a['p'] - b['p']).abs().max()) < 2e-3
        assert float((a['p'] - b['p']).abs().mean()) < 2e-5


def _bench_line(nproc, extra, port, full=True):
    """Run bench.py the way the driver launches it (torch.distributed.run for N > 1) and return its JSON line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, NSGP_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0')
    common = ['--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-build-chol'] + (['--full'] if full else []) + extra
    if nproc == 1:
        cmd = [sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1'] + common
    else:
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(root, 'bench.py'),
               '--gpus', str(nproc)] + common
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, out.stdout[-2000:]                     # rank 0 prints ONE line
    return json.loads(lines[0])


def test_bench_two_rank_control_flow_matches_one_rank():
    """The N > 1 control flow of bench.py itself -- two hipGraph replays (forward + backward, Adam) around the eager
    gradient all-reduce, barrier + max-over-ranks timing, rank-0 JSON -- with two ranks on this one GPU over gloo
    (RCCL needs a GPU per rank; the driver runs that).  Strong scaling (the default) splits ONE 4096-row
    minibatch, so the summed objective after the same number of steps must equal the single-rank run's."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    one = _bench_line(1, [], 0)
    two = _bench_line(2, [], _free_port())
    assert one['n_gpus'] == 1 and two['n_gpus'] == 2
    assert one['scaling'] == 'strong' and two['scaling'] == 'strong'
    assert two['config']['global_batch'] == 4096 and two['config']['per_gpu_batch'] == 2048
    for r in (one, two):
        assert r['metric'] == 'dsvi_elbo_steps_per_sec' and r['unit'] == 'steps/s' and r['steps'] == 3
        assert r['value'] == pytest.approx(r['iterations_per_sec'])        # strong: value IS iterations/s
        assert r['rows_per_sec'] == pytest.approx(4096 * r['iterations_per_sec'], rel=1e-3)
        assert 'roofline' in r and r['roofline']['bound'] == 'mfma'
    assert two['final_loss'] == pytest.approx(one['final_loss'], rel=2e-4)
    # N > 1 runs the staged backward by default: three exchange groups (last layer | hidden layer | the rest)
    ex = two['gradient_exchange']
    assert ex['exchange_groups'] == 3 and ex['backward_stages'] == 4
    assert sum(ex['group_bytes']) > 12_000_000                              # the whole 12.6 MB bucket
    assert ex['group_bytes'][0] > 4_000_000 and ex['group_bytes'][1] > 8_000_000 and ex['group_bytes'][2] < 100_000
    flat = _bench_line(2, ['--no-overlap'], _free_port())                   # one all-reduce after the backward pass
    assert flat['final_loss'] == pytest.approx(one['final_loss'], rel=2e-4)
    st = _bench_line(1, ['--staged'], 0)                                    # the staging itself, priced at N = 1
    assert st['final_loss'] == pytest.approx(one['final_loss'], rel=2e-4)
    weak = _bench_line(2, ['--scaling', 'weak'], _free_port())
    assert weak['scaling'] == 'weak' and weak['config']['global_batch'] == 8192
    assert weak['value'] == pytest.approx(2 * weak['iterations_per_sec'], rel=1e-3)


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """A plain bench.py run times the steps and prints the headline fields only (the roofline re-run is --full's);
    --dump-outputs writes the last timed step's loss, parameters and gradients, the same in a plain and a --full run
    (seeded inputs; the dump is taken before the --full re-run moves the parameters)."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import numpy as np
    plain = _bench_line(1, ['--dump-outputs', str(tmp_path / 'plain')], 0, full=False)
    full = _bench_line(1, ['--dump-outputs', str(tmp_path / 'full')], 0)
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in plain
    assert plain['steps'] == 3 and plain['ms_per_step'] == pytest.approx(1e3 / plain['value'], rel=1e-2)
    assert 'roofline' not in plain and 'roofline' in full
    names = sorted(os.listdir(tmp_path / 'plain'))
    assert names == sorted(os.listdir(tmp_path / 'full'))
    assert 'loss.npy' in names and any(n.startswith('param.') for n in names) and any(n.startswith('grad.') for n in names)
    assert sum(os.path.getsize(tmp_path / 'plain' / n) for n in names) <= 64 << 20
    loss = np.load(tmp_path / 'plain' / 'loss.npy')
    assert loss.dtype == np.float64 and float(loss[0]) == pytest.approx(plain['final_loss'], rel=1e-5)
    for n in names:
        a, b = np.load(tmp_path / 'plain' / n), np.load(tmp_path / 'full' / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6, err_msg=n)


def test_gradient_sinks_fill_the_bucket_without_a_copy_and_match_plain_autograd():
    """FlatBucket(grads_as_views=False) registers its large parameters as gradient sinks: the KL term's and the layers'
    Lq gradients are written / accumulated straight into the bucket range (no gather copy), in whatever order the engine
    runs them, for tied layers, across two backward passes without zero_grad, and after gradients were cleared by hand.
    Reference: the same model with an ordinary torch optimiser layout (no bucket)."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, 'nonstationary-precip_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import models.dgps as m
    from nsgp.dist import PhiloxEps
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FlatBucket

    def build(layers):
        torch.manual_seed(3)
        m.num_output_dims = 3 if layers > 1 else 2         # a tied hidden layer maps 3 -> 3 (module-level knob, as upstream)
        model = m.DeepGP(layers, (600, 3), num_inducing=256).cuda()        # 256 x 256 factors: above the sink threshold
        mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 600))
        model.train()
        return model, mll

    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(192, 3, generator=g).cuda(), torch.randn(192, generator=g).cuda()

    def grads(model, mll, passes, bucket=None, clear_by_hand=False):
        out = None
        for rep in range(2):                              # second repetition: after gradients were cleared
            if bucket is not None and not clear_by_hand:
                bucket.zero_grad()
            else:
                for p in model.parameters():
                    p.grad = None
            for _ in range(passes):
                with settings.num_likelihood_samples(3), settings.eps_provider(PhiloxEps(5)):
                    loss = -mll(model(x), y)
                loss.backward()
            if bucket is not None:
                bucket.gather_grads()
                out = {n: bucket.flat_g[off:off + k].view(p.shape).clone()
                       for (n, p), (off, k) in zip([(names[id(q)], q) for q in bucket.params], bucket.offsets)}
            else:
                out = {n: p.grad.clone() for n, p in model.named_parameters()}
        return out

    for layers in (1, 2):                                  # 2: the tied hidden layer is applied twice
        for passes in (1, 2):
            for by_hand in (False, True):
                ref_model, ref_mll = build(layers)
                ref = grads(ref_model, ref_mll, passes)
                model, mll = build(layers)
                names = {id(p): n for n, p in model.named_parameters()}
                bucket = FlatBucket(model.parameters(), grads_as_views=False)
                got = grads(model, mll, passes, bucket, clear_by_hand=by_hand)
                big = [n for n, p in model.named_parameters() if p.numel() >= (1 << 16)]
                assert big
                for n in big:                              # adopted: p.grad lives in the bucket, nothing was copied
                    p = dict(model.named_parameters())[n]
                    idx = [i for i, q in enumerate(bucket.params) if q is p][0]
                    assert p.grad is not None and p.grad.data_ptr() == bucket.grad_views[idx].data_ptr()
                for n in ref:
                    assert torch.allclose(got[n], ref[n], rtol=2e-5, atol=1e-6), (layers, passes, by_hand, n)
                del bucket
    m.num_output_dims = 2


def test_autograd_grad_results_stay_distinct_with_the_sinks_switched_off():
    """a gradient sink hands autograd a view of the optimiser's bucket.  Under `ops.grad_sinks(False)` two
    `torch.autograd.grad` calls return independent tensors (plain-torch behaviour); with the sinks on (the default, meant
    for loss.backward()) the two results alias the same bucket range -- documented on FlatBucket."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import models.dgps as m
    from nsgp import ops
    from nsgp.dist import PhiloxEps
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    from nsgp.optim import FlatBucket
    torch.manual_seed(3)
    m.num_output_dims = 2
    model = m.DeepGP(1, (600, 3), num_inducing=256).cuda()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, 600))
    model.train()
    bucket = FlatBucket(model.parameters(), grads_as_views=False)
    Lq = model.last_layer.variational_strategy._variational_distribution.chol_variational_covar
    assert Lq.numel() >= (1 << 16)
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(192, 3, generator=g).cuda(), torch.randn(192, generator=g).cuda()

    def grad_of(scale):
        with settings.num_likelihood_samples(3), settings.eps_provider(PhiloxEps(5)):
            loss = -scale * mll(model(x), y)
        return torch.autograd.grad(loss, [Lq])[0]
    with ops.grad_sinks(False):
        g1 = grad_of(1.0)
        keep = g1.clone()
        g2 = grad_of(2.0)
    assert g1.data_ptr() != g2.data_ptr()
    assert torch.equal(g1, keep)                                   # the first result did not change under the second
    assert torch.allclose(g2, 2.0 * g1, rtol=1e-5, atol=1e-7)
    base, end = bucket.flat_g.data_ptr(), bucket.flat_g.data_ptr() + bucket.flat_g.numel() * 4
    assert not (base <= g1.data_ptr() < end) and not (base <= g2.data_ptr() < end)
    a1 = grad_of(1.0)                                               # sinks on: the gradient lives in the bucket
    assert base <= a1.data_ptr() < end
    del bucket


def test_bench_staged_capture_failure_on_one_rank_is_decided_collectively():
    """VERDICT r2 item 8 / ADVICE r2: if capturing the staged step fails (here: simulated on rank 1 only), BOTH ranks fall
    back to eager launches -- the decision is an all-reduce(MIN) of a capture-ok flag -- the JSON line carries the flag and
    the run ends at the same loss as the graph-replayed run."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    ok = _bench_line(2, [], _free_port())
    os.environ['NSGP_BENCH_FAIL_CAPTURE'] = '1'
    try:
        bad = _bench_line(2, [], _free_port())
    finally:
        del os.environ['NSGP_BENCH_FAIL_CAPTURE']
    assert 'hipgraph_capture_failed_ran_eagerly' not in ok['gradient_exchange'] and ok['config']['hipgraph'] is True
    assert 'hipgraph_capture_failed_ran_eagerly' in bad['gradient_exchange'] and bad['config']['hipgraph'] is False
    assert bad['final_loss'] == pytest.approx(ok['final_loss'], rel=2e-4)
