"""GaussianLikelihood [gpytorch.likelihoods recalled, SURVEY A.1/A.5]: noise = softplus(raw_noise) + 1e-4
(raw init 0 -> 0.6932), state-dict key `noise_covar.raw_noise`; `likelihood(dist)` adds noise * I,
expected_log_prob / log_marginal as used by VariationalELBO and models/dgps.py:109."""
import math

import numpy.polynomial.hermite
import torch

from .. import ops
from . import settings
from .constraints import GreaterThan, Positive
from .distributions import MultivariateNormal, MultitaskMultivariateNormal
from .lazy import LazyTensor, DiagLazyTensor, lazify
from .module import Module


class Likelihood(Module):
    pass


class HomoskedasticNoise(Module):
    def __init__(self, noise_prior=None, noise_constraint=None, batch_shape=torch.Size()):
        super().__init__()
        self.register_parameter('raw_noise', torch.nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.register_constraint('raw_noise', noise_constraint or GreaterThan(1e-4))
        if noise_prior is not None:
            self.register_prior('noise_prior', noise_prior, lambda m: m.noise)

    @property
    def noise(self):
        return self._get_constrained('raw_noise')

    @noise.setter
    def noise(self, value):
        self._set_constrained('raw_noise', value)


class GaussianLikelihood(Likelihood):
    def __init__(self, noise_prior=None, noise_constraint=None, batch_shape=torch.Size(), **kwargs):
        super().__init__()
        self.noise_covar = HomoskedasticNoise(noise_prior, noise_constraint, batch_shape)

    @property
    def noise(self):
        return self.noise_covar.noise

    @noise.setter
    def noise(self, value):
        self.noise_covar.noise = value

    @property
    def raw_noise(self):
        return self.noise_covar.raw_noise

    def _shaped_noise_covar(self, shape, *params, **kwargs):
        n = shape[-1]
        return DiagLazyTensor(self.noise.expand(*shape[:-1], n) if len(shape) > 1 else self.noise.expand(n))

    def forward(self, function_samples, *params, **kwargs):
        return torch.distributions.Normal(function_samples, self.noise.sqrt())

    def marginal(self, function_dist, *params, **kwargs):
        mean = function_dist.mean
        noise = self.noise
        if isinstance(function_dist, MultitaskMultivariateNormal):
            return MultitaskMultivariateNormal(mean, None, _var=function_dist.variance + noise,
                                               _tsn=function_dist._tsn)
        if getattr(function_dist, '_diag_only', False):
            return function_dist._with_noise(noise)
        covar = function_dist.lazy_covariance_matrix
        return function_dist.__class__(mean, covar.add_diag(noise.reshape(-1)[:1] if noise.numel() == 1 else noise))

    def __call__(self, input, *params, **kwargs):
        if torch.is_tensor(input):
            return self.forward(input, *params, **kwargs)
        return self.marginal(input, *params, **kwargs)

    def expected_log_prob(self, target, input, *params, **kwargs):
        """-1/2 [((y - mu)^2 + v)/noise + log noise + log 2 pi]  per point (shape of input.mean)."""
        mean, variance = input.mean, input.variance
        noise = self.noise
        res = ((target - mean) ** 2 + variance) / noise + noise.log() + math.log(2 * math.pi)
        return res.mul(-0.5)

    def log_marginal(self, observations, function_dist, *params, **kwargs):
        """Normal(mu, sqrt(clamp_min(v + noise, 1e-8))).log_prob(y)  (models/dgps.py:109)."""
        mean, variance = function_dist.mean, function_dist.variance
        v = (variance + self.noise).clamp_min(1e-8)
        return -0.5 * ((observations - mean) ** 2 / v + v.log() + math.log(2 * math.pi))


class GaussHermiteQuadrature1D(torch.nn.Module):
    """The Q-node Gauss-Hermite rule of numpy.polynomial.hermite.hermgauss as persistent buffers `locations`, `weights`:
    int exp(-t^2) g(t) dt ~ sum_k w_k g(t_k).  Computed in float64, stored in the default dtype; `.cuda()` moves the
    buffers and `.double()` / `.float()` refill them from the float64 rule, so no host-to-device copy happens inside a
    (captured) training step.  Q = settings.num_gauss_hermite_locs unless given, 1 <= Q <= 64.
    Being persistent, the buffers are part of the state dict: `load_state_dict` puts the checkpoint's values back, so a
    float32 checkpoint loaded into a `.double()` model carries float32-rounded nodes (1e-7 relative on the sums) until the
    next dtype change.  Callers that hand in a q(f) of another dtype than the module's get the buffers cast to it, with the
    rounding of the narrower of the two types."""
    MAX_LOCS = 64

    def __init__(self, num_locs=None):
        super().__init__()
        Q = settings.num_gauss_hermite_locs.value() if num_locs is None else num_locs
        if isinstance(Q, bool) or not isinstance(Q, int) or not 1 <= Q <= self.MAX_LOCS:
            raise ValueError(f'the number of Gauss-Hermite locations must be an integer in 1..{self.MAX_LOCS}, got {Q!r}')
        self.num_locs = Q
        t, w = self._rule()
        dt = torch.get_default_dtype()
        self.register_buffer('locations', t.to(dt))
        self.register_buffer('weights', w.to(dt))

    def _rule(self):
        t, w = numpy.polynomial.hermite.hermgauss(self.num_locs)
        return torch.from_numpy(t), torch.from_numpy(w)

    def _apply(self, fn, *args, **kwargs):
        before = self.locations.dtype
        super()._apply(fn, *args, **kwargs)
        if self.locations.dtype != before:                # a float32 copy widened to float64 would keep float32's rounding
            t, w = self._rule()
            self.locations, self.weights = t.to(self.locations), w.to(self.weights)
        return self

    def forward(self, log_prob, mean, variance):
        """pi^-1/2 sum_k w_k g(mu + sqrt(2 v) t_k) for g given as a function of tensors with a trailing node dimension."""
        t, w = self.locations.to(mean.dtype), self.weights.to(mean.dtype)
        f = mean.unsqueeze(-1) + (2.0 * variance).sqrt().unsqueeze(-1) * t
        return (log_prob(f) * w).sum(-1) / math.sqrt(math.pi)


class PredictiveMoments:
    """What `likelihood(q(f))` of a _OneDimensionalLikelihood returns: the predictive `.mean` and `.variance` of y."""

    def __init__(self, mean, variance):
        self.mean, self.variance = mean, variance

    @property
    def stddev(self):
        return self.variance.sqrt()


class _OneDimensionalLikelihood(Likelihood):
    """A likelihood p(y_i | f_i) of one latent value per observation [gpytorch.likelihoods._OneDimensionalLikelihood
    recalled]: expectations under q(f_i) = N(mu_i, v_i) by Gauss-Hermite quadrature with the rule in `self.quadrature`,
      expected_log_prob(y, q(f)) = pi^-1/2 sum_k w_k log p(y | mu + sqrt(2 v) t_k)            per point,
      log_marginal(y, q(f))      = log(pi^-1/2 sum_k w_k p(y | mu + sqrt(2 v) t_k))           per point (a log-sum-exp).
    expected_log_prob is plain torch ops on any device (VariationalELBO's generic path); log_marginal of CUDA tensors with a
    1-D target runs the HIP kernel nsgp_gh_log_marginal (ops.gh_log_marginal); CPU tensors go through torch ops, and so does
    a call that asks for gradients (the kernel has no backward), has a target of more dimensions or a batch of parameter sets.

    A deliberate difference from gpytorch: `likelihood(q(f))` / `marginal` returns the predictive mean and variance of y in
    CLOSED FORM (PredictiveMoments), deterministic, where gpytorch returns a distribution over likelihood samples.  The
    leading sample dimension of q(f) is carried through unchanged.

    Subclasses give `_log_prob(y, f)` (broadcasting torch ops), `forward(function_samples)`, `_moments(mu, v)`, and for the
    kernels `_gh_kind`, `_gh_params()` (None or the tensor the kernel reads) and `_gh_constant()` (None or the f-independent
    part of log p the kernel leaves out, a 1-element tensor)."""
    _gh_kind = None

    def __init__(self):
        super().__init__()
        self.quadrature = GaussHermiteQuadrature1D()

    def _log_prob(self, y, f):
        raise NotImplementedError

    def _moments(self, mean, variance):
        raise NotImplementedError

    def _gh_params(self):
        return None

    def _gh_constant(self):
        return None

    def _gh_rule(self, ref):
        """(locations, weights) as the kernels take them: on ref's device, in ref's dtype (no copy when they already are)."""
        q = self.quadrature
        return q.locations.to(device=ref.device, dtype=ref.dtype), q.weights.to(device=ref.device, dtype=ref.dtype)

    def _gh_ready(self):
        """May the HIP kernels evaluate this likelihood: a kind they know and one (not a batch of) parameter set."""
        return self._gh_kind is not None

    def expected_log_prob(self, target, input, *params, **kwargs):
        mean, variance = input.mean, input.variance
        y = target.unsqueeze(-1)
        return self.quadrature(lambda f: self._log_prob(y, f), mean, variance)

    def log_marginal(self, observations, function_dist, *params, **kwargs):
        mean, variance = function_dist.mean, function_dist.variance
        if mean.is_cuda and observations.dim() == 1 and mean.dim() in (1, 2) and self._gh_ready() \
                and not (torch.is_grad_enabled() and (mean.requires_grad or variance.requires_grad)):
            t, w = self._gh_rule(mean)
            p = self._gh_params()
            out = ops.gh_log_marginal(self._gh_kind, observations, mean.reshape(-1, mean.shape[-1]),
                                      variance.reshape(-1, mean.shape[-1]), None if p is None else p.detach(), t, w)
            c = self._gh_constant()
            return (out if c is None else out + c.detach().reshape(())).reshape(mean.shape)
        q = self.quadrature
        t, w = q.locations.to(mean.dtype), q.weights.to(mean.dtype)
        f = mean.unsqueeze(-1) + (2.0 * variance).sqrt().unsqueeze(-1) * t
        lp = self._log_prob(observations.unsqueeze(-1), f)
        keep = w > 0                                       # (a weight that underflowed in float32 has no logarithm)
        return torch.logsumexp(lp[..., keep] + w[keep].log(), dim=-1) - 0.5 * math.log(math.pi)

    def marginal(self, function_dist, *params, **kwargs):
        return PredictiveMoments(*self._moments(function_dist.mean, function_dist.variance))

    def __call__(self, input, *params, **kwargs):
        if torch.is_tensor(input):
            return self.forward(input, *params, **kwargs)
        return self.marginal(input, *params, **kwargs)


class BernoulliLikelihood(_OneDimensionalLikelihood):
    """p(y = 1 | f) = Phi(f) (probit link), targets 0 / 1 as floats: log p = log Phi((2 y - 1) f).  No parameters.
    Predictive mean Phi(mu / sqrt(1 + v)), variance p (1 - p)."""
    _gh_kind = ops.GH_BERNOULLI

    def _log_prob(self, y, f):
        return torch.special.log_ndtr((2.0 * y - 1.0) * f)

    def forward(self, function_samples, *params, **kwargs):
        return torch.distributions.Bernoulli(probs=torch.special.ndtr(function_samples))

    def _moments(self, mean, variance):
        p = torch.special.ndtr(mean / (1.0 + variance).sqrt())
        return p, p * (1.0 - p)


class StudentTLikelihood(_OneDimensionalLikelihood):
    """p(y | f) = Student-t with `deg_free` = nu degrees of freedom, location f and scale sqrt(`noise`).
    raw_deg_free: init 0 under GreaterThan(2) (nu = 2.6931); raw_noise: init 0 under Positive (noise = 0.6931).
    Predictive mean mu, variance v + noise nu / (nu - 2).  The HIP kernels take one parameter set (batch_shape ());
    a batch of them is evaluated with torch ops."""
    _gh_kind = ops.GH_STUDENT_T

    def __init__(self, batch_shape=torch.Size(), deg_free_prior=None, deg_free_constraint=None, noise_prior=None,
                 noise_constraint=None):
        super().__init__()
        self.register_parameter('raw_deg_free', torch.nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.register_parameter('raw_noise', torch.nn.Parameter(torch.zeros(*batch_shape, 1)))
        self.register_constraint('raw_deg_free', deg_free_constraint or GreaterThan(2))
        self.register_constraint('raw_noise', noise_constraint or Positive())
        if deg_free_prior is not None:
            self.register_prior('deg_free_prior', deg_free_prior, lambda m: m.deg_free)
        if noise_prior is not None:
            self.register_prior('noise_prior', noise_prior, lambda m: m.noise)

    @property
    def deg_free(self):
        return self._get_constrained('raw_deg_free')

    @deg_free.setter
    def deg_free(self, value):
        self._set_constrained('raw_deg_free', value)

    @property
    def noise(self):
        return self._get_constrained('raw_noise')

    @noise.setter
    def noise(self, value):
        self._set_constrained('raw_noise', value)

    def _normaliser(self, nu):
        return torch.lgamma(0.5 * (nu + 1.0)) - torch.lgamma(0.5 * nu) - 0.5 * torch.log(nu * math.pi)

    def _log_prob(self, y, f):
        nu, s2 = self.deg_free.unsqueeze(-1), self.noise.unsqueeze(-1)           # (..., 1, 1) against (..., n, Q)
        return self._normaliser(nu) - 0.5 * (nu + 1.0) * torch.log1p((y - f) ** 2 / (nu * s2)) - 0.5 * torch.log(s2)

    def _gh_ready(self):
        return self.raw_deg_free.numel() == 1 and self.raw_noise.numel() == 1

    def _gh_params(self):
        return torch.cat([self.deg_free.reshape(-1), self.noise.reshape(-1)])

    def _gh_constant(self):
        return self._normaliser(self.deg_free.reshape(-1))

    def forward(self, function_samples, *params, **kwargs):
        return torch.distributions.StudentT(df=self.deg_free, loc=function_samples, scale=self.noise.sqrt())

    def _moments(self, mean, variance):
        nu = self.deg_free
        return mean, variance + self.noise * nu / (nu - 2.0)
