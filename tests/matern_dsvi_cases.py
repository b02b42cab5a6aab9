"""Shared by tests/test_gpu_matern_dsvi.py: the float64 Matern restatement that stands in for oracle.kernels.rbf_ard, so
that the unmodified oracle/svgp.py is the reference of a Matern layer and of a deep GP that mixes RBF and Matern layers."""
import math

import torch

NUS = (0.5, 1.5, 2.5)


def matern_radial(s, nu):
    """kappa_nu of the squared scaled distance s.  The distance is s.clamp_min(1e-30).sqrt(), as MaternKernel._radial takes it:
    a plain sqrt has an infinite derivative at s = 0 and autograd returns NaN on the diagonal of Kzz."""
    d = s.clamp_min(1e-30).sqrt()
    a = math.sqrt(2.0 * nu)
    poly = 1.0 if nu == 0.5 else 1.0 + a * d if nu == 1.5 else 1.0 + a * d + (5.0 / 3.0) * s
    return poly * torch.exp(-a * d)


def matern_ard(x1, x2, lengthscale, outputscale, nu):
    """oracle.kernels.rbf_ard's signature and broadcasting with the Matern radial function."""
    a, b = x1 / lengthscale, x2 / lengthscale
    k = matern_radial((a.unsqueeze(-2) - b.unsqueeze(-3)).pow(2).sum(-1), nu)
    if outputscale is not None:
        os_ = torch.as_tensor(outputscale, dtype=k.dtype)
        k = k * os_.reshape(*os_.shape, 1, 1) if os_.dim() else k * os_
    return k


def patch_oracle_kernel(monkeypatch, nu, by_lengthscale=None):
    """monkeypatch oracle.kernels.rbf_ard (what oracle/svgp.py reaches the kernel through) with the Matern restatement.
    nu: the smoothness of every call (None: the oracle's own RBF); by_lengthscale: {id(lengthscale tensor): nu or None},
    for a model whose layers differ -- oracle.svgp hands a layer's `lengthscale` entry to the kernel as it is."""
    from oracle import kernels
    rbf = kernels.rbf_ard

    def kernel(x1, x2, lengthscale, outputscale=None):
        v = nu if by_lengthscale is None else by_lengthscale[id(lengthscale)]
        return rbf(x1, x2, lengthscale, outputscale) if v is None else matern_ard(x1, x2, lengthscale, outputscale, v)
    monkeypatch.setattr(kernels, 'rbf_ard', kernel)
