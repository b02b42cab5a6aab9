"""the north-star tolerance (posterior mean within 1e-4 relative error) asserted AT the headline
shape -- BASELINE configs[3]: 2-layer DSVI DeepGP, M = 1024 inducing points, minibatch B = 4096, S = 10 likelihood
samples, D = 3 -- after a few Adam steps from bench.py's own initialisation (so kappa(Kzz) is that of a model in
training, not of the random init; 25 and 1000 steps), float32 HIP path against the float64 CPU oracle (models/dgps.py:44-51,92-98
through gpytorch's whitened VariationalStrategy.forward).

Error measure: max-norm relative error  max_i |got_i - ref_i| / max_i |ref_i|  per layer output (means AND
variances) and relative error of the ELBO.  kappa(Kzz + jitter I) is printed for each GP."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _maxrel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.fixture(scope='module')
def trained():
    """train_steps -> (model, mll) after that many Adam steps from bench.py's initialisation; each count trains once per
    module (the forward and the gradient tests share the 1000-step model)."""
    _need_gpu()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    from nsgp.gp import settings
    cache = {}

    def get(train_steps):
        if train_steps not in cache:
            M, B, S, N = bench.M_INDUCING, bench.BATCH, bench.S_SAMPLES, bench.N_DATA
            assert (M, B, S) == (1024, 4096, 10)
            dev = torch.device('cuda', torch.cuda.current_device())
            x_all, y_all = bench.synthetic_grid()
            model, mll, opt = bench.build(dev, 1)
            perm = torch.randperm(N, generator=torch.Generator().manual_seed(bench.SEED))
            model.train()
            with settings.num_likelihood_samples(S):
                for k in range(train_steps):                         # Adam steps (lr 0.01) on fresh minibatches
                    rows = perm[(k % (N // B)) * B:(k % (N // B) + 1) * B]
                    opt.zero_grad()
                    loss = -mll(model(x_all[rows].to(dev)), y_all[rows].to(dev))
                    loss.backward()
                    opt.step()
            assert bool(torch.isfinite(loss))
            cache[train_steps] = (model, mll)
        return cache[train_steps]
    return get


def _minibatch(seed=5):
    import bench
    g = torch.Generator().manual_seed(seed)
    x_all, y_all = bench.synthetic_grid()
    rows = torch.randperm(bench.N_DATA, generator=g)[:bench.BATCH]                # a fresh minibatch
    return x_all[rows], y_all[rows], [torch.randn(bench.S_SAMPLES, bench.BATCH, 2, generator=g)]


def _kappas(hidden, last, M):
    from oracle import kernels
    kap = []
    with torch.no_grad():
        for p in (hidden, last):
            Kzz = kernels.rbf_ard(p['Z'].detach(), p['Z'].detach(), p['lengthscale'].detach(), p['outputscale'].detach())
            Kzz = Kzz + 1e-4 * torch.eye(M, dtype=F64)
            ev = torch.linalg.eigvalsh(Kzz)
            kap += [float(k_) for k_ in (ev[..., -1] / ev[..., 0]).reshape(-1)]
    return kap


@pytest.mark.parametrize('train_steps', [25, 1000])
def test_posterior_mean_within_1e4_at_the_headline_shape(train_steps, trained):
    """train_steps = 25: a model early in training; 1000: kappa(Kzz) has moved with the inducing points / lengthscales
    (the bound must hold along the training trajectory, not only near the initialisation)."""
    import bench
    from nsgp.gp import settings
    from oracle import kernels, svgp
    from test_gpu_dgp import _FixedEps, _oracle_layers
    M, B, S, N = bench.M_INDUCING, bench.BATCH, bench.S_SAMPLES, bench.N_DATA
    dev = torch.device('cuda', torch.cuda.current_device())
    model, mll = trained(train_steps)
    xb, yb, eps = _minibatch()
    model.eval()                       # eval: no variational-mean init noise; same marginals as train mode
    with torch.no_grad(), settings.num_likelihood_samples(S), settings.eps_provider(_FixedEps(eps)):
        hid = model.layers[0](xb.to(dev))                           # MultitaskMVN over (n, 2)
        h_mean, h_var = hid.mean, hid.variance
        out = model(xb.to(dev))
        o_mean, o_var = out.mean, out.variance                      # (S, B)
        model.train()
        elbo = mll(model(xb.to(dev)), yb.to(dev))
    with torch.no_grad():
        hidden, last, noise, _ = _oracle_layers(model)
        det = lambda p: {k: (v.detach() if torch.is_tensor(v) else tuple(t.detach() if torch.is_tensor(t) else t for t in v))
                         for k, v in p.items()}
        hidden, last, noise = det(hidden), det(last), noise.detach()
        xd = xb.double()
        xin = xd.unsqueeze(-3).expand(2, B, 3)
        hm_ref, hv_ref = svgp.svgp_marginal(xin, hidden)            # (2, B)
        om_ref, ov_ref = svgp.dgp_forward(xd, hidden, last, 1, [e.double() for e in eps], S)
        elbo_ref = svgp.dsvi_elbo(xd, yb.double(), hidden, last, 1, [e.double() for e in eps], S, noise, N)
        kap = []
        for p in (hidden, last):
            Kzz = kernels.rbf_ard(p['Z'], p['Z'], p['lengthscale'], p['outputscale'])
            Kzz = Kzz + 1e-4 * torch.eye(M, dtype=F64)
            ev = torch.linalg.eigvalsh(Kzz)
            kap += [float(k_) for k_ in (ev[..., -1] / ev[..., 0]).reshape(-1)]
    errs = dict(hidden_mean=_maxrel(h_mean.transpose(-1, -2), hm_ref), hidden_var=_maxrel(h_var.transpose(-1, -2), hv_ref),
                out_mean=_maxrel(o_mean, om_ref), out_var=_maxrel(o_var, ov_ref),
                elbo=abs(float(elbo) - float(elbo_ref)) / abs(float(elbo_ref)))
    print(f'after {train_steps} Adam steps: kappa(Kzz + 1e-4 I) [hidden 0, hidden 1, last]:', ['%.3g' % k_ for k_ in kap])
    print('max-norm relative errors (f32 HIP vs f64 oracle):', {k: '%.3g' % v for k, v in errs.items()})
    assert errs['hidden_mean'] <= 1e-4, errs                        # the north-star bound, per layer
    assert errs['out_mean'] <= 1e-4, errs
    assert errs['hidden_var'] <= 1e-4 and errs['out_var'] <= 1e-4, errs
    assert errs['elbo'] <= 1e-4, errs


# per-parameter max-norm relative gradient error, ~3x the worst measured on MI355X over 25 / 1000 Adam steps: int8 projection
# on 2.0e-4 / 1.8e-4, off (float64-accumulated product of the float32 Kzx) 2.1e-4 / 6.8e-4 -- the int8 path is the more
# accurate one (its Kzx digits come from a float64 evaluation); the worst entries are the last layer's Z gradients
HEADLINE_GRAD_TOL = {True: 6e-4, False: 2e-3}


@pytest.fixture(scope='module')
def oracle_grads():
    """train_steps -> (ELBO, {parameter: gradient}) of torch.autograd through oracle.svgp.dsvi_elbo in float64 on the host, at
    the trained model's parameters, the _minibatch() inputs and its fixed eps (once per count: the int8 on / off cases share
    it)."""
    cache = {}

    def get(train_steps, model):
        if train_steps not in cache:
            import bench
            from oracle import svgp
            from test_gpu_dgp import _oracle_layers
            xb, yb, eps = _minibatch()
            hidden, last, noise, leaves = _oracle_layers(model)
            # per-point zero offsets on the hidden layer's bias: their gradients are the summands of the bias gradient
            # (a sum over the B points that cancels as training converges, see the test)
            kind, w, bias = hidden['mean']
            delta = torch.zeros(bias.shape[0], xb.shape[0], dtype=F64, requires_grad=True)
            hidden['mean'] = (kind, w, bias + delta)
            ref = svgp.dsvi_elbo(xb.double(), yb.double(), hidden, last, 1, [e.double() for e in eps], bench.S_SAMPLES, noise,
                                 bench.N_DATA)
            ref.backward()
            grads = {k: v.grad for k, v in leaves.items()}
            grads['h.b summands'] = delta.grad.abs().sum(-1).reshape(grads['h.b'].shape)
            cache[train_steps] = (float(ref), grads, _kappas(hidden, last, bench.M_INDUCING))
        return cache[train_steps]
    return get


@pytest.mark.parametrize('i8', [True, False])
@pytest.mark.parametrize('train_steps', [25, 1000])
def test_gradients_match_the_oracle_at_the_headline_shape(train_steps, i8, trained, oracle_grads):
    """The backward of the timed step (about two thirds of its flops, the Cholesky adjoint at kappa(Kzz) ~ 1e6 among them)
    at the shape bench.py times: one forward + backward of the trained model at M = 1024, B = 4096, S = 10 with fixed eps,
    every parameter gradient against torch.autograd of the float64 oracle (per-parameter max-norm relative error, the
    measure of test_gpu_dgp.py::test_dsvi_elbo_and_gradients_match_oracle), with the int8 projection on and off."""
    import bench
    from nsgp.gp import settings
    from test_gpu_dgp import _FixedEps, _model_params
    dev = torch.device('cuda', torch.cuda.current_device())
    model, mll = trained(train_steps)
    xb, yb, eps = _minibatch()
    model.train()
    model.zero_grad(set_to_none=True)
    with settings.num_likelihood_samples(bench.S_SAMPLES), settings.eps_provider(_FixedEps(eps)), settings.whiten_matmul_i8(i8):
        elbo = mll(model(xb.to(dev)), yb.to(dev))
        elbo.backward()
    elbo_ref, grads_ref, kap = oracle_grads(train_steps, model)
    errs = {}
    for name, p in _model_params(model).items():
        got, want = p.grad.detach().cpu().double(), grads_ref[name]
        if name.endswith('Lq'):
            want = torch.tril(want)
        if name == 'h.b':
            # the hidden layer's bias gradient is a sum over the B points that cancels as training converges (after
            # 1000 steps it fell to ~1e-3 of its summands, and its plain relative error to 2e-3 / 2e-2 with the int8 product
            # on / off): measured against the size of the terms it sums, sum_i |dELBO / dmean_i|
            errs['h.b plain'] = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
            errs[name] = float(((got - want).abs() / grads_ref['h.b summands']).max())
            continue
        errs[name] = float((got - want).abs().max()) / (float(want.abs().max()) + 1e-30)
    model.zero_grad(set_to_none=True)
    worst = max((k for k in errs if k != 'h.b plain'), key=errs.get)
    print(f'after {train_steps} Adam steps: kappa(Kzz + 1e-4 I) [hidden 0, hidden 1, last]:', ['%.3g' % k_ for k_ in kap])
    print(f'[measured] headline grads i8={i8} steps={train_steps}: worst {errs[worst]:.3g} ({worst}); elbo rel err '
          f'{abs(float(elbo) - elbo_ref) / abs(elbo_ref):.3g};', {k: '%.2g' % v for k, v in errs.items()})
    assert errs[worst] < HEADLINE_GRAD_TOL[i8], errs
