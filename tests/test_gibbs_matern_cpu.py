"""GibbsKernel(nu = 1/2, 3/2, 5/2), the non-stationary Matern kernel, without a GPU: the C ABI declares and exports its
entry points, they validate their arguments on the host, the kernel and model classes store and forward `nu`, and the
float64 restatement the GPU tests compare against has the stationary limit and is positive definite.

`gibbs_matern_ref` is the float64 restatement (imported by tests/test_gpu_gibbs_matern.py) of Paciorek & Schervish (2006)
with Sigma(x) = diag ell(x)^2:
    k = os * prod_d sqrt(2 l1_d l2_d / s_d) * kappa_nu(d),   s_d = l1_d^2 + l2_d^2,   d^2 = 2 sum_d (x1_d - x2_d)^2 / s_d,
kappa_nu the Matern closed forms of tests/test_matern_cpu.py, with d = clamp_min(d^2, 1e-30).sqrt() as in `matern_ref`, so
that autograd takes the derivative at d = 0 as 0, the device kernel's convention."""
import ctypes
import math

import pytest
import torch

from test_matern_cpu import matern_ref

F64 = torch.float64
NUS = (0.5, 1.5, 2.5)


def gibbs_matern_ref(x1, x2, ell1, ell2, os_, nu):
    """x1:(n1,D) x2:(n2,D), ell1:(D,n1) ell2:(D,n2), os_: scalar (tensor or float) or None -> (n1,n2); leading batch
    dimensions as oracle.kernels.gibbs, whose signature this has without os_ and nu."""
    sq = ell1.unsqueeze(-1) ** 2 + ell2.unsqueeze(-2) ** 2                      # (D,n1,n2)
    pre = torch.sqrt(2 * ell1.unsqueeze(-1) * ell2.unsqueeze(-2) / sq).prod(-3)
    diff = x1.unsqueeze(-2) - x2.unsqueeze(-3)                                  # (n1,n2,D)
    s = 2 * (diff ** 2 / sq.movedim(-3, -1)).sum(-1)
    d = s.clamp_min(1e-30).sqrt()
    if nu == 0.5:
        k = torch.exp(-d)
    elif nu == 1.5:
        a = math.sqrt(3.0)
        k = (1 + a * d) * torch.exp(-a * d)
    elif nu == 2.5:
        a = math.sqrt(5.0)
        k = (1 + a * d + (5.0 / 3.0) * s) * torch.exp(-a * d)
    else:
        raise ValueError(nu)
    k = pre * k
    return k if os_ is None else os_ * k


NAMES = [f'nsgp_gibbs_matern_build_{p}_{s}' for p in ('fwd', 'bwd') for s in ('f32', 'f64')]


def test_header_declares_and_library_exports_the_gibbs_matern_entry_points():
    import nsgp
    names = nsgp.declared_symbols()
    for name in NAMES:
        assert name in names, name
    lib = nsgp.load_library()
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
    assert lib.nsgp_abi_version() == 2


def test_gibbs_matern_entry_points_validate_their_arguments_on_the_host():
    """Bad arguments return the negative 1-based index of the offending one before any launch; empty problems return 0
    without a launch.  Safe without a GPU: no call below reaches the device."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    b = ctypes.cast(buf, ctypes.c_void_p)
    #       x1 x2 l1 l2 n1 n2 D nu2 os diag_add K ldk stream
    fwd_ok = [b, b, b, b, 4, 4, 2, 5, b, b, b, 4, None]
    #       x1 x2 l1 l2 n1 n2 D nu2 os G ldg g_l1 g_l2 g_x1 g_x2 g_os ws ws_bytes stream
    bwd_ok = [b, b, b, b, 4, 4, 2, 3, b, b, 4, b, b, b, b, b, b, 512, None]
    for sfx in ('f32', 'f64'):
        fwd = getattr(lib, f'nsgp_gibbs_matern_build_fwd_{sfx}')
        bwd = getattr(lib, f'nsgp_gibbs_matern_build_bwd_{sfx}')
        bad_f = lambda i, v: fwd(*[v if k == i else a for k, a in enumerate(fwd_ok)])       # noqa: E731
        bad_b = lambda i, v: bwd(*[v if k == i else a for k, a in enumerate(bwd_ok)])       # noqa: E731
        for bad in (bad_f, bad_b):
            assert bad(0, None) == -1 and bad(1, None) == -2 and bad(2, None) == -3 and bad(3, None) == -4
            assert bad(4, -1) == -5 and bad(5, -1) == -6
            assert bad(6, 0) == -7 and bad(6, 9) == -7 and bad(6, -3) == -7
            for nu2 in (0, 2, 4, 6, -1, 7, 25):
                assert bad(7, nu2) == -8, nu2
        assert bad_f(10, None) == -11 and bad_f(11, 3) == -12
        assert bad_b(9, None) == -10 and bad_b(10, 3) == -11
        # the first bad argument is the one reported
        assert fwd(None, None, b, b, 4, 4, 0, 2, b, b, None, 1, None) == -1
        assert fwd(b, b, b, b, 4, 4, 2, 2, b, b, None, 1, None) == -8
        # empty problems: no launch, success (also with no matrix at all)
        assert bad_f(4, 0) == 0 and bad_f(5, 0) == 0
        assert bad_b(4, 0) == 0 and bad_b(5, 0) == 0
        assert fwd(b, b, b, b, 0, 4, 2, 1, None, None, None, 4, None) == 0
        assert bwd(b, b, b, b, 4, 0, 2, 1, None, None, 0, None, None, None, None, None, None, 0, None) == 0


def test_gibbs_matern_backward_shares_the_gibbs_workspace_query():
    """No workspace query of its own: the accumulator counts are the Gibbs kernel's."""
    import nsgp
    assert not [n for n in nsgp.declared_symbols() if 'gibbs_matern' in n and 'workspace' in n]
    assert nsgp.load_library().nsgp_gibbs_build_bwd_workspace(300, 500, 3, 8) > 0


def test_gibbs_kernel_and_models_store_and_forward_nu(monkeypatch):
    import nsgp.gp as gpytorch
    from nsgp import ops
    from models.gibbs_kernels import GibbsKernel, LogNormalPriorProcess
    from models.nonstationary_models import DiagonalExactGP, DiagonalSparseGP
    from models.spatio_temporal_models import SparseSpatioTemporal_Nonstationary
    assert GibbsKernel().nu is None
    for nu in NUS:
        assert GibbsKernel(nu=nu, ard_num_dims=2).nu == nu
    for nu in (2.0, 0.0, 3.5, 1.0, '1.5'):
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            GibbsKernel(nu=nu)
    assert not any(k == 'nu' or k.endswith('.nu') for k in GibbsKernel(nu=1.5).state_dict())

    # the one launch site hands nu on, for K(x, x), K(x, z) and the fused scalars alike
    seen = []

    def record(x1, x2, ell1, ell2, outputscale=None, diag_add=None, **kw):
        seen.append(kw)
        return torch.zeros(x1.shape[-2], x2.shape[-2], dtype=x1.dtype)
    monkeypatch.setattr(ops, 'gibbs_kernel', record)
    x, z = torch.randn(6, 2), torch.randn(4, 2)
    e, ez = torch.ones(2, 6), torch.ones(2, 4)
    for nu in (None, 1.5):
        k = GibbsKernel(nu=nu, ard_num_dims=2)
        del seen[:]
        k.forward(x, x, ell1=e)
        k.forward(x, z, ell1=e, ell2=ez, _outputscale=torch.ones(()), _diag_add=torch.ones(()))
        assert seen == [{'nu': nu}, {'nu': nu}]

    g = torch.Generator().manual_seed(0)
    xtr, ytr = torch.randn(12, 2, generator=g), torch.randn(12, generator=g)
    zz = xtr[::3].clone()
    lik = gpytorch.likelihoods.GaussianLikelihood
    base = {
        DiagonalExactGP: lambda m: m.covar_module.base_kernel,
        DiagonalSparseGP: lambda m: m.covar_module.base_kernel.base_kernel,
    }
    for cls, get in base.items():
        extra = (zz,) if cls is DiagonalSparseGP else ()
        prior = LogNormalPriorProcess(input_dim=2)
        assert get(cls(xtr, ytr, lik(), prior, *extra, num_dim=2)).nu is None
        assert get(cls(xtr, ytr, lik(), prior, *extra, 2, nu=1.5)).nu == 1.5
        with pytest.raises(TypeError):
            cls(xtr, ytr, lik(), prior, *extra, 2, 1.5)                     # keyword-only
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            cls(xtr, ytr, lik(), prior, *extra, num_dim=2, nu=2.0)
    xst, zst = torch.randn(12, 3, generator=g), torch.randn(4, 2, generator=g)
    prior = LogNormalPriorProcess(input_dim=2, active_dims=(0, 1))
    st = lambda **kw: SparseSpatioTemporal_Nonstationary(xst, ytr, lik(), prior, zst.clone(), num_dim=2, **kw)  # noqa: E731
    assert st().spatial_covar_module.base_kernel.base_kernel.nu is None
    assert st(nu=2.5).spatial_covar_module.base_kernel.base_kernel.nu == 2.5
    with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
        st(nu=3.0)


def test_ops_reject_a_bad_nu_and_cpu_tensors():
    from nsgp import ops, BackendError
    x, e = torch.randn(5, 2), torch.ones(2, 5)
    G = torch.ones(5, 5)
    for nu in (2.0, 0, 3.5, 1):
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.gibbs_build(x, x, e, e, nu=nu)
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.gibbs_build_bwd(x, x, e, e, None, G, nu=nu)
        with pytest.raises(RuntimeError, match='nu expected to be 0.5, 1.5, or 2.5'):
            ops.gibbs_kernel(x, x, e, e, nu=nu)
    for nu in (None,) + NUS:
        with pytest.raises(BackendError):
            ops.gibbs_build(x, x, e, e, nu=nu)
        with pytest.raises(BackendError):
            ops.gibbs_build_bwd(x, x, e, e, None, G, nu=nu)
        with pytest.raises(BackendError):
            ops.gibbs_kernel(x, x, e, e, 0.5, 0.1, nu=nu)


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('D', [1, 2, 3])
def test_restatement_has_the_stationary_limit(nu, D):
    """ell1 = ell2 = const: os * Matern_nu-ARD(ell)."""
    g = torch.Generator().manual_seed(7 + D)
    x1 = torch.randn(57, D, generator=g, dtype=F64)
    x2 = torch.cat([torch.randn(40, D, generator=g, dtype=F64), x1[:5]])          # includes zero distances
    ls = torch.rand(1, D, generator=g, dtype=F64) + 0.3
    got = gibbs_matern_ref(x1, x2, ls.T.expand(D, 57), ls.T.expand(D, 45), 0.7, nu)
    ref = matern_ref(x1, x2, ls, torch.tensor([0.7], dtype=F64), nu)[0]
    assert float((got - ref).abs().max()) < 1e-14


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('D', [1, 2, 3])
def test_restatement_gram_matrix_is_positive_definite(nu, D):
    g = torch.Generator().manual_seed(11 * D)
    n = 300
    x = torch.randn(n, D, generator=g, dtype=F64)
    ell = torch.exp(0.8 * torch.randn(D, n, generator=g, dtype=F64))
    K = gibbs_matern_ref(x, x, ell, ell, None, nu)
    assert float((K - K.T).abs().max()) == 0.0
    assert float((torch.diagonal(K) - 1).abs().max()) < 1e-14
    lo = float(torch.linalg.eigvalsh(K)[0])
    print(f'[measured] nu={nu} D={D} min eigenvalue {lo:.3g}')
    assert lo > 0
