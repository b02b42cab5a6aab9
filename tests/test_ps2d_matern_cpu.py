"""MultivariateGibbsKernel(nu = 1/2, 3/2, 5/2), the Paciorek-Schervish kernel with a full 2x2 Sigma(x) and the Matern radial
function, without a GPU: the C ABI declares and exports its entry points, they validate their arguments on the host, the
ops and the kernel classes refuse a bad `nu`, and the float64 restatement the GPU tests compare against reduces to the
oracle's squared-exponential kernel and to the diagonal non-stationary Matern kernel, and is positive definite.

`ps2d_matern_ref` is the float64 restatement (imported by tests/test_gpu_ps2d_matern.py): oracle.kernels.ps2d with exp(-q)
replaced by kappa_nu of s = 2 q,
    k = |S1|^(1/4) |S2|^(1/4) |A|^(-1/2) kappa_nu(d),   A = (S1 + S2) / 2,   d^2 = s = 2 delta^T (A + jitter I)^-1 delta,
kappa_nu the Matern closed forms of tests/test_gibbs_matern_cpu.py, with d = clamp_min(s, 1e-30).sqrt() as there, so that
autograd takes the derivative at d = 0 as 0, the device kernel's convention."""
import ctypes
import math

import pytest
import torch

from test_gibbs_matern_cpu import gibbs_matern_ref

F64 = torch.float64
NUS = (0.5, 1.5, 2.5)


def matern_radial(s, nu):
    """kappa_nu at the squared distance s."""
    d = s.clamp_min(1e-30).sqrt()
    if nu == 0.5:
        return torch.exp(-d)
    if nu == 1.5:
        a = math.sqrt(3.0)
        return (1 + a * d) * torch.exp(-a * d)
    if nu == 2.5:
        a = math.sqrt(5.0)
        return (1 + a * d + (5.0 / 3.0) * s) * torch.exp(-a * d)
    raise ValueError(nu)


def ps2d_matern_ref(x1, x2, sig1, sig2, jitter, nu, radial=matern_radial):
    """x1:(n1,2) x2:(n2,2), sig1:(n1,2,2) sig2:(n2,2,2) -> (n1,n2): the op sequence of oracle.kernels.ps2d (jitter in the
    inverse only, no symmetry assumed) up to the quadratic form q, then prefactor * radial(2 q, nu)."""
    n1, n2 = x1.shape[0], x2.shape[0]
    Si = sig1.unsqueeze(1).expand(n1, n2, 2, 2)
    Sj = sig2.unsqueeze(0).expand(n1, n2, 2, 2)
    det_product = torch.det(sig1).pow(0.25).unsqueeze(1) * torch.det(sig2).pow(0.25).unsqueeze(0)
    avg = (Si + Sj) / 2
    prefactor = det_product * torch.det(avg).pow(-0.5)
    inv = torch.inverse(avg + jitter * torch.eye(2, dtype=avg.dtype))
    diff = x1.unsqueeze(-2) - x2.unsqueeze(-3)
    q = (diff.unsqueeze(-2) @ inv @ diff.unsqueeze(-1)).reshape(n1, n2)
    return prefactor * radial(2 * q, nu)


NAMES = [f'nsgp_ps2d_matern_build_{p}_{s}' for p in ('fwd', 'bwd') for s in ('f32', 'f64')]


# ------------------------------------------------------------------------------------------ 1: header and exports
def test_header_declares_and_library_exports_the_ps2d_matern_entry_points():
    import nsgp
    names = nsgp.declared_symbols()
    for name in NAMES:
        assert name in names, name
    lib = nsgp.load_library()
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert lib.nsgp_abi_version() == 2


def test_ps2d_matern_backward_shares_the_ps2d_workspace_query():
    """No workspace query of its own: the accumulator counts are the Paciorek-Schervish kernel's."""
    import nsgp
    assert not [n for n in nsgp.declared_symbols() if 'ps2d_matern' in n and 'workspace' in n]
    assert nsgp.load_library().nsgp_ps2d_build_bwd_workspace(300, 500, 8) > 0


# ------------------------------------------------------------------------------------------ 2: argument checks
def test_ps2d_matern_entry_points_validate_their_arguments_on_the_host():
    """Bad arguments return the negative 1-based index of the offending one before any launch (nsgp_ps2d_build_*'s checks
    with nu2 as argument 7 and every later index one up); empty problems return 0 without a launch.  Safe without a GPU:
    no call below reaches the device."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    #       x1 x2 s1 s2 n1 n2 nu2 jit K ldk stream
    fwd_ok = [b, b, b, b, 4, 4, 5, 1e-5, b, 4, None]
    #       x1 x2 s1 s2 n1 n2 nu2 jit G ldg g_s1 g_s2 ws ws_bytes stream
    bwd_ok = [b, b, b, b, 4, 4, 3, 1e-5, b, 4, b, b, b, 512, None]
    for sfx in ('f32', 'f64'):
        fwd = getattr(lib, f'nsgp_ps2d_matern_build_fwd_{sfx}')
        bwd = getattr(lib, f'nsgp_ps2d_matern_build_bwd_{sfx}')
        bad_f = lambda i, v: fwd(*[v if k == i else a for k, a in enumerate(fwd_ok)])       # noqa: E731
        bad_b = lambda i, v: bwd(*[v if k == i else a for k, a in enumerate(bwd_ok)])       # noqa: E731
        for bad in (bad_f, bad_b):
            assert bad(0, None) == -1 and bad(1, None) == -2 and bad(2, None) == -3 and bad(3, None) == -4
            assert bad(4, -1) == -5 and bad(5, -1) == -6
            for nu2 in (0, 2, 4, 6, -1, 7, 25):
                assert bad(6, nu2) == -7, nu2
            # K / G and its leading dimension
            assert bad(8, None) == -9 and bad(9, 3) == -10
        # the first bad argument is the one reported
        assert fwd(None, None, b, b, 4, 4, 2, 1e-5, None, 1, None) == -1
        assert fwd(b, b, b, None, -1, 4, 2, 1e-5, None, 1, None) == -4
        assert fwd(b, b, b, b, 4, 4, 2, 1e-5, None, 1, None) == -7
        assert bwd(b, b, b, b, 4, -2, 2, 1e-5, None, 1, None, None, None, 0, None) == -6
        assert bwd(b, b, b, b, 4, 4, 2, 1e-5, None, 1, None, None, None, 0, None) == -7
        assert bwd(b, b, b, b, 4, 4, 1, 1e-5, None, 1, None, None, None, 0, None) == -9
        # empty problems: no launch, success (also with no matrix at all)
        assert bad_f(4, 0) == 0 and bad_f(5, 0) == 0
        assert bad_b(4, 0) == 0 and bad_b(5, 0) == 0
        assert fwd(b, b, b, b, 0, 4, 1, 0.0, None, 4, None) == 0
        assert bwd(b, b, b, b, 4, 0, 1, 0.0, None, 0, None, None, None, 0, None) == 0


# ------------------------------------------------------------------------------------------ 3: the restatement
def _points(n1, n2, seed, hi=1.0):
    """x ~ U[0, hi]^2 and Sigma = ps_sigma(H, D), H ~ N(0, 1), D unsymmetric: the recipe of test_ps2d_fwd_bwd."""
    from oracle import kernels as K
    g = torch.Generator().manual_seed(seed)
    x1 = hi * torch.rand(n1, 2, generator=g, dtype=F64)
    x2 = hi * torch.rand(n2, 2, generator=g, dtype=F64)
    H1, H2 = torch.randn(n1, 2, generator=g, dtype=F64), torch.randn(n2, 2, generator=g, dtype=F64)
    Dm = torch.tensor([[0.7, 0.1], [-0.2, 0.9]], dtype=F64)
    return x1, x2, K.ps_sigma(H1, Dm), K.ps_sigma(H2, Dm)


@pytest.mark.parametrize('jitter', [1e-5, 0.0])
def test_restatement_with_the_squared_exponential_radial_is_the_oracle_kernel(jitter):
    from oracle import kernels as K
    x1, x2, s1, s2 = _points(31, 45, seed=3)
    x2 = torch.cat([x2, x1[:4]])                                                 # includes zero distances
    s2 = torch.cat([s2, s1[:4]])
    got = ps2d_matern_ref(x1, x2, s1, s2, jitter, None, radial=lambda s, nu: torch.exp(-0.5 * s))
    ref = K.ps2d(x1, x2, s1, s2, jitter)
    assert float(((got - ref).abs() / ref.abs()).max()) < 1e-15
    # and with a Matern radial it is another kernel
    assert float((ps2d_matern_ref(x1, x2, s1, s2, jitter, 1.5) - ref).abs().max()) > 1e-3


@pytest.mark.parametrize('nu', NUS)
def test_restatement_has_the_diagonal_limit(nu):
    """Sigma = diag(2 ell^2), jitter = 0: the non-stationary Matern kernel of GibbsKernel(nu)."""
    g = torch.Generator().manual_seed(17)
    x1 = torch.randn(57, 2, generator=g, dtype=F64)
    x2 = torch.cat([torch.randn(40, 2, generator=g, dtype=F64), x1[:5]])          # includes zero distances
    e1 = torch.rand(2, 57, generator=g, dtype=F64) + 0.3
    e2 = torch.rand(2, 45, generator=g, dtype=F64) + 0.3
    got = ps2d_matern_ref(x1, x2, torch.diag_embed(2 * e1.T ** 2), torch.diag_embed(2 * e2.T ** 2), 0.0, nu)
    ref = gibbs_matern_ref(x1, x2, e1, e2, None, nu)
    assert float((got - ref).abs().max()) < 1e-14


@pytest.mark.parametrize('nu', NUS)
def test_restatement_gram_matrix_is_positive_definite(nu):
    x, _, s, _ = _points(40, 1, seed=29, hi=2.0)
    K = ps2d_matern_ref(x, x, s, s, 1e-5, nu)
    assert float((torch.diagonal(K) - 1).abs().max()) < 1e-14
    lo = float(torch.linalg.eigvalsh(0.5 * (K + K.T))[0])
    print(f'[measured] ps2d-matern restatement nu={nu} min eigenvalue {lo:.3g}')
    assert lo > 0


# ------------------------------------------------------------------------------------------ 4: ops and kernel classes
def test_ops_reject_a_bad_nu_and_cpu_tensors():
    from nsgp import ops, BackendError
    x, s = torch.randn(5, 2), torch.eye(2).expand(5, 2, 2).contiguous()
    G = torch.ones(5, 5)
    for nu in (2.0, 0, 3.5, 1):
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.ps2d_build(x, x, s, s, nu=nu)
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.ps2d_build_bwd(x, x, s, s, 1e-5, G, nu=nu)
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.ps2d_kernel(x, x, s, s, nu=nu)
    for nu in (None,) + NUS:
        with pytest.raises(BackendError):
            ops.ps2d_build(x, x, s, s, nu=nu)
        with pytest.raises(BackendError):
            ops.ps2d_build_bwd(x, x, s, s, 1e-5, G, nu=nu)
        with pytest.raises(BackendError):
            ops.ps2d_kernel(x, x, s, s, 1e-5, nu=nu)


def test_kernel_classes_refuse_a_bad_nu():
    """Before anything is built (the row kernel of the prior on H needs the device: that nu is stored and defaults to None
    is checked in tests/test_gpu_ps2d_matern.py)."""
    from models.multivariate_gibbs_kernel import MultivariateGibbsKernel
    from models.sparse_multivariate_gibbs_kernel import SparseMultivariateGibbsKernel
    x = torch.randn(6, 2)
    for nu in (2.0, 0.0, 3.5, 1.0, '1.5'):
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            MultivariateGibbsKernel(x, 2, nu=nu)
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            SparseMultivariateGibbsKernel(x, 2, x.clone(), nu=nu)
    with pytest.raises(TypeError):
        MultivariateGibbsKernel(x, 2, 1.5)                                       # keyword-only
    with pytest.raises(TypeError):
        SparseMultivariateGibbsKernel(x, 2, x.clone(), 1.5)
