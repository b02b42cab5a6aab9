"""DSVI deep GP on the MI355X engine -- drop-in for models/dgps.py of the reference.

Same surface (reference file:line):
  num_output_dims                                   models/dgps.py:13
  DeepGPHiddenLayer(input_dims, output_dims, num_inducing=250, mean_type='constant')   :15-70
  DeepGP(num_layers, train_x_shape)  with .layers / .last_layer / .likelihood / .forward / .predict(loader)   :72-111
  ExactGPModel(train_x, train_y, likelihood, kernel)                                    :113-122
Reference quirks kept: the hidden layers are ONE tied layer object repeated
num_layers times, and predict() returns only the last batch's distribution.  Additions (keyword-only,
defaults reproduce the reference): DeepGP(..., num_inducing=250, tie_layers=True, variational='cholesky');
variational='mean_field' gives every layer a MeanFieldVariationalDistribution; likelihood=None keeps GaussianLikelihood(),
an instance (BernoulliLikelihood(), StudentTLikelihood()) is used as given; nu=None keeps ScaleKernel(RBFKernel) layers,
nu=0.5 | 1.5 | 2.5 gives every layer ScaleKernel(MaternKernel(nu)), a pair (hidden, last) mixes (either entry may be None).
"""
import torch

import nsgp.gp as gpytorch
from nsgp.gp import settings
from nsgp.gp.distributions import MultivariateNormal, MultitaskMultivariateNormal
from nsgp.gp.kernels import MaternKernel, RBFKernel, ScaleKernel
from nsgp.gp.likelihoods import GaussianLikelihood
from nsgp.gp.means import ConstantMean, LinearMean
from nsgp.gp.models import DeepGPLayer, DeepGP as _DeepGPBase, ExactGP
from nsgp.gp.variational import CholeskyVariationalDistribution, MeanFieldVariationalDistribution, VariationalStrategy

num_output_dims = 2
VARIATIONAL_DISTRIBUTIONS = {'cholesky': CholeskyVariationalDistribution, 'mean_field': MeanFieldVariationalDistribution}


class DeepGPHiddenLayer(DeepGPLayer):
    """One whitened SVGP layer: Z ~ randn, q(u) = N(m, Lq Lq^T) -- or N(m, diag(s^2)) with variational='mean_field' --,
    ScaleKernel(RBF-ARD), or ScaleKernel(Matern-ARD) with nu = 0.5 | 1.5 | 2.5."""

    def __init__(self, input_dims, output_dims, num_inducing=250, mean_type='constant', variational='cholesky', nu=None):
        if variational not in VARIATIONAL_DISTRIBUTIONS:
            raise ValueError(f'variational must be one of {sorted(VARIATIONAL_DISTRIBUTIONS)}, got {variational!r}')
        batch_shape = torch.Size([]) if output_dims is None else torch.Size([output_dims])
        Z = torch.randn(*batch_shape, num_inducing, input_dims)
        q_u = VARIATIONAL_DISTRIBUTIONS[variational](num_inducing_points=num_inducing, batch_shape=batch_shape)
        strategy = VariationalStrategy(self, Z, q_u, learn_inducing_locations=True)
        super().__init__(strategy, input_dims, output_dims)
        self.mean_module = ConstantMean(batch_shape=batch_shape) if mean_type == 'constant' \
            else LinearMean(input_dims)
        base = RBFKernel(batch_shape=batch_shape, ard_num_dims=input_dims) if nu is None \
            else MaternKernel(nu=nu, batch_shape=batch_shape, ard_num_dims=input_dims)
        self.covar_module = ScaleKernel(base, batch_shape=batch_shape, ard_num_dims=None)

    def forward(self, x):
        """Prior at x (what gpytorch's VariationalStrategy evaluates at [Z; x])."""
        return MultivariateNormal(self.mean_module(x), self.covar_module(x))

    def __call__(self, x, *other_inputs, **kwargs):
        """Concatenation skip connections, as in the reference (unused by DeepGP.forward)."""
        if len(other_inputs):
            if isinstance(x, MultitaskMultivariateNormal):
                x = x.rsample()
            S = settings.num_likelihood_samples.value()
            x = torch.cat([x] + [inp.unsqueeze(0).expand(S, *inp.shape) for inp in other_inputs], dim=-1)
        return super().__call__(x, are_samples=bool(len(other_inputs)))


class DeepGP(_DeepGPBase):
    def __init__(self, num_layers, train_x_shape, *, num_inducing=250, tie_layers=True, variational='cholesky',
                 likelihood=None, nu=None):
        nu = tuple(nu) if isinstance(nu, list) else nu       # (anything else unexpected: MaternKernel's RuntimeError)
        nu_hidden, nu_last = nu if isinstance(nu, tuple) and len(nu) == 2 else (nu, nu)
        hidden = DeepGPHiddenLayer(input_dims=train_x_shape[-1], output_dims=num_output_dims,
                                   num_inducing=num_inducing, mean_type='linear', variational=variational, nu=nu_hidden)
        last = DeepGPHiddenLayer(input_dims=hidden.output_dims, output_dims=None,
                                 num_inducing=num_inducing, mean_type='constant', variational=variational, nu=nu_last)
        super().__init__()
        if tie_layers:
            stack = [hidden for _ in range(num_layers)]
        else:
            stack = [hidden] + [DeepGPHiddenLayer(hidden.output_dims, num_output_dims, num_inducing, 'linear',
                                                  variational=variational, nu=nu_hidden)
                                for _ in range(num_layers - 1)]
        self.layers = torch.nn.ModuleList(stack)
        self.last_layer = last
        self.likelihood = GaussianLikelihood() if likelihood is None else likelihood

    def forward(self, inputs):
        rep = inputs
        for layer in self.layers:
            rep = layer(rep)
        return self.last_layer(rep)

    def initialize_inducing_points(self, x, *, seed=0, **kmeans_kw):
        """Replace the Z ~ randn start (a reference quirk, kept as the default) by k-means: the first layer's Z becomes the
        centres `nsgp.cluster.kmeans(x, num_inducing, seed=seed, **kmeans_kw)` of the inputs x:(n, D), shared by its output
        dimensions; every later distinct layer, the last included, gets those centres pushed through the mean modules of the
        layers before it (a tied hidden layer is set once and applied num_layers times).  Nothing else changes.  Returns
        the KMeansResult."""
        from nsgp.cluster import kmeans
        first = self.layers[0].variational_strategy.inducing_points
        res = kmeans(x, first.shape[-2], seed=seed, **kmeans_kw)
        rep, done = res.centers.to(first.dtype), set()
        with torch.no_grad():
            for layer in list(self.layers) + [self.last_layer]:
                if id(layer) not in done:
                    done.add(id(layer))
                    Z = layer.variational_strategy.inducing_points
                    Z.copy_(rep.expand_as(Z))
                if layer is not self.last_layer:
                    m = layer.mean_module(rep)                          # (M,), or (output_dims, M) for a batched mean
                    rep = m.unsqueeze(-1).expand(-1, layer.output_dims) if m.dim() == 1 else m.transpose(-1, -2)
        return res

    def predict(self, test_loader):
        """Returns (predictive of the LAST batch, means (S,N), variances (S,N), per-point log marginals (S,N)):
        the tuple of the reference's DeepGP.predict (:100-111).  Each batch is propagated twice, once for the
        noisy predictive and once for the log marginal of its targets, exactly like the reference."""
        parts = {'mean': [], 'variance': [], 'll': []}
        last_predictive = None
        with torch.no_grad():
            for xb, yb in test_loader:
                last_predictive = self.likelihood(self(xb))
                parts['mean'].append(last_predictive.mean)
                parts['variance'].append(last_predictive.variance)
                parts['ll'].append(self.likelihood.log_marginal(yb, self(xb)))
        joined = {k: torch.cat(v, dim=-1) for k, v in parts.items()}
        return last_predictive, joined['mean'], joined['variance'], joined['ll']


class ExactGPModel(ExactGP):
    """Constant-mean exact GP over a caller-supplied kernel (SE-ARD baselines)."""

    def __init__(self, train_x, train_y, likelihood, kernel):
        super().__init__(train_x, train_y, likelihood)
        self.mean_module = ConstantMean()
        self.covar_module = kernel

    def forward(self, x):
        return MultivariateNormal(self.mean_module(x), self.covar_module(x))
