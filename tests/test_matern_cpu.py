"""MaternKernel (nu = 1/2, 3/2, 5/2) without a GPU: the C ABI declares and exports the batched Matern-ARD entry points,
they validate their arguments on the host, the gpytorch-facing kernel class has gpytorch's construction semantics, and
the float64 restatement the GPU tests compare against agrees with scikit-learn's Matern kernel.

`matern_ref` is the float64 restatement of the closed forms (imported by tests/test_gpu_matern.py):
    nu = 1/2: e^-d,  nu = 3/2: (1 + sqrt3 d) e^-sqrt3 d,  nu = 5/2: (1 + sqrt5 d + 5/3 d^2) e^-sqrt5 d,
with d = clamp_min(s, 1e-30).sqrt(), s = |(x1 - x2) / ls|^2, so that autograd takes the derivative at d = 0 as 0, the
device kernel's convention."""
import ctypes
import math

import numpy as np
import pytest
import torch

F64 = torch.float64
NUS = (0.5, 1.5, 2.5)


def matern_ref(x1, x2, ls, os_, nu):
    """os[b] * k_nu(|(x1 - x2) / ls[b]|): x1:(n1,D) or (b,n1,D), x2 likewise, ls:(b,D), os:(b,) -> (b,n1,n2)."""
    u = (x1.unsqueeze(-2) - x2.unsqueeze(-3)) / ls[:, None, None, :]
    s = (u * u).sum(-1)
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
    return os_[:, None, None] * k


def test_header_declares_and_library_exports_the_matern_entry_points():
    import nsgp
    names = nsgp.declared_symbols()
    want = ['nsgp_matern_build_fwd_f32', 'nsgp_matern_build_fwd_f64', 'nsgp_matern_build_bwd_f32',
            'nsgp_matern_build_bwd_f64', 'nsgp_matern_build_bwd_workspace']
    for name in want:
        assert name in names, name
    lib = nsgp.load_library()
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for name in want:
        assert hasattr(raw, name), name
    assert lib.nsgp_abi_version() == 2
    # host-only size query: the RBF workspace layout (same accumulator counts)
    assert lib.nsgp_matern_build_bwd_workspace(2, 300, 500, 3, 8) == lib.nsgp_rbf_build_bwd_workspace(2, 300, 500, 3, 8)


def test_matern_entry_points_validate_their_arguments_on_the_host():
    """Bad arguments return the negative 1-based index of the offending one before any launch; empty problems return 0
    without a launch.  Safe without a GPU: no call below reaches the device."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    P = lambda o: ctypes.cast(o, ctypes.c_void_p)
    b = P(buf)
    #       x1 x2 ls os batch n1 n2 D sx1 sx2 nu2 diag_add K ldk sK stream
    fwd_ok = [b, b, b, b, 1, 4, 4, 2, 0, 0, 5, 0.0, b, 4, 16, None]
    #       x1 x2 ls os batch n1 n2 D sx1 sx2 nu2 G ldg sG g_x1 g_x2 g_ls g_os ws ws_bytes stream
    bwd_ok = [b, b, b, b, 1, 4, 4, 2, 0, 0, 3, b, 4, 16, b, b, b, b, b, 512, None]
    for sfx in ('f32', 'f64'):
        fwd = getattr(lib, f'nsgp_matern_build_fwd_{sfx}')
        bwd = getattr(lib, f'nsgp_matern_build_bwd_{sfx}')
        bad_f = lambda i, v: fwd(*[v if k == i else a for k, a in enumerate(fwd_ok)])
        bad_b = lambda i, v: bwd(*[v if k == i else a for k, a in enumerate(bwd_ok)])
        for bad in (bad_f, bad_b):
            assert bad(0, None) == -1 and bad(1, None) == -2 and bad(2, None) == -3 and bad(3, None) == -4
            assert bad(4, -1) == -5 and bad(5, -1) == -6 and bad(6, -1) == -7
            assert bad(7, 0) == -8 and bad(7, 9) == -8 and bad(7, -3) == -8
            for nu2 in (0, 2, 4, 6, -1, 7, 25):
                assert bad(10, nu2) == -11, nu2
        assert bad_f(12, None) == -13 and bad_f(13, 3) == -14
        assert bad_b(11, None) == -12 and bad_b(12, 3) == -13
        # empty problems: no launch, success
        assert bad_f(4, 0) == 0 and bad_f(5, 0) == 0 and bad_f(6, 0) == 0
        assert bad_b(4, 0) == 0 and bad_b(5, 0) == 0 and bad_b(6, 0) == 0


def test_rbf_entry_points_validate_their_arguments_on_the_host():
    """The RBF entry points share their argument checks with the Matern ones; their return codes are the negative
    1-based index in their OWN signature (no nu2, so K / ldk / G / ldg sit one place earlier).  Safe without a GPU: no
    call below reaches the device."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    P = lambda o: ctypes.cast(o, ctypes.c_void_p)
    b = P(buf)
    #       x1 x2 ls os batch n1 n2 D sx1 sx2 diag_add K ldk sK stream
    fwd_ok = [b, b, b, b, 1, 4, 4, 2, 0, 0, 0.0, b, 4, 16, None]
    #       x1 x2 ls os batch n1 n2 D sx1 sx2 G ldg sG g_x1 g_x2 g_ls g_os ws ws_bytes stream
    bwd_ok = [b, b, b, b, 1, 4, 4, 2, 0, 0, b, 4, 16, b, b, b, b, b, 512, None]
    for sfx in ('f32', 'f64'):
        fwd = getattr(lib, f'nsgp_rbf_build_fwd_{sfx}')
        bwd = getattr(lib, f'nsgp_rbf_build_bwd_{sfx}')
        bad_f = lambda i, v: fwd(*[v if k == i else a for k, a in enumerate(fwd_ok)])
        bad_b = lambda i, v: bwd(*[v if k == i else a for k, a in enumerate(bwd_ok)])
        for bad in (bad_f, bad_b):
            assert bad(0, None) == -1 and bad(1, None) == -2 and bad(2, None) == -3 and bad(3, None) == -4
            assert bad(4, -1) == -5 and bad(5, -1) == -6 and bad(6, -1) == -7
            assert bad(7, 0) == -8 and bad(7, 9) == -8 and bad(7, -3) == -8
        assert bad_f(11, None) == -12 and bad_f(12, 3) == -13
        assert bad_b(10, None) == -11 and bad_b(11, 3) == -12
        # empty problems: no launch, success
        assert bad_f(4, 0) == 0 and bad_f(5, 0) == 0 and bad_f(6, 0) == 0
        assert bad_b(4, 0) == 0 and bad_b(5, 0) == 0 and bad_b(6, 0) == 0


def test_matern_kernel_construction_follows_gpytorch():
    from nsgp.gp.kernels import MaternKernel, ScaleKernel
    for nu in (2.0, 0.0, 3.5, 1.0):
        with pytest.raises(RuntimeError):
            MaternKernel(nu=nu)
    k = MaternKernel(nu=1.5, ard_num_dims=2)
    assert k.raw_lengthscale.shape == (1, 2)
    assert k.nu == 1.5 and k.has_lengthscale and k.is_stationary and k.fuses_outputscale
    assert MaternKernel().nu == 2.5
    assert MaternKernel(nu=0.5, batch_shape=torch.Size([3])).raw_lengthscale.shape == (3, 1, 1)
    keys = set(k.state_dict())
    assert 'raw_lengthscale' in keys and not any('nu' == s or s.endswith('.nu') for s in keys)
    assert set(ScaleKernel(MaternKernel(nu=0.5)).state_dict()) >= {'raw_outputscale', 'base_kernel.raw_lengthscale'}
    # positive constraint (softplus of the zero initialisation)
    assert torch.allclose(k.lengthscale.detach(), torch.full((1, 2), math.log(2.0)))


@pytest.mark.parametrize('nu', NUS)
def test_restatement_matches_sklearn(nu):
    from sklearn.gaussian_process import kernels
    g = torch.Generator().manual_seed(31)
    x1 = torch.randn(57, 3, generator=g, dtype=F64)
    x2 = torch.cat([torch.randn(40, 3, generator=g, dtype=F64), x1[:5]])          # includes zero distances
    ls = torch.rand(1, 3, generator=g, dtype=F64) + 0.3
    ref = matern_ref(x1, x2, ls, torch.ones(1, dtype=F64), nu)[0]
    sk = kernels.Matern(length_scale=ls[0].numpy(), nu=nu)(x1.numpy(), x2.numpy())
    assert np.abs(ref.numpy() - sk).max() < 1e-14


def test_cpu_tensors_raise_backend_error():
    from nsgp import ops, BackendError
    from nsgp.gp.kernels import MaternKernel, ScaleKernel
    x = torch.randn(5, 2)
    ls = torch.ones(1, 2)
    os_ = torch.ones(1)
    for nu in NUS:
        with pytest.raises(BackendError):
            ops.matern_build(x, x, ls, os_, nu)
        with pytest.raises(BackendError):
            ops.matern_kernel(x, x, ls, os_, nu)
        with pytest.raises(BackendError):
            ops.matern_build_bwd(x, x, ls, os_, nu, torch.ones(1, 5, 5))
        with pytest.raises(BackendError):
            ScaleKernel(MaternKernel(nu=nu, ard_num_dims=2))(x).evaluate()
    with pytest.raises(BackendError):
        ops.matern_build(x, x, ls, os_, 2.0)
