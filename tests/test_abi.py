"""CPU-side checks of the drop-in boundary: the shared object loads and exports every symbol that
include/nsgp.h declares (no compute calls here -- there is no GPU in the build container)."""
import ctypes
import os
import re

import pytest
import torch


def test_header_declares_the_hot_path_entry_points():
    from nsgp import declared_symbols
    names = declared_symbols()
    for stem in ('gibbs_build_fwd', 'gibbs_build_bwd', 'rbf_build_fwd', 'rbf_build_bwd', 'ps2d_build_fwd',
                 'ps2d_build_bwd', 'gemm', 'potrf', 'trtri', 'svgp_colstats', 'svgp_colstats_bwd',
                 'dgp_sample_fwd', 'dgp_sample_bwd', 'gauss_ell_fwd', 'gauss_ell_bwd', 'kl_whitened_fwd',
                 'kl_whitened_bwd', 'philox_normal'):
        for sfx in ('f32', 'f64'):
            assert f'nsgp_{stem}_{sfx}' in names, (stem, sfx)
    assert 'nsgp_adam_step_f32' in names and 'nsgp_abi_version' in names
    assert 'nsgp_gemm_plan' in names and 'nsgp_pairwise_bwd_plan' in names          # host-side launch queries


def test_library_loads_and_exports_every_declared_symbol():
    import nsgp
    assert os.path.exists(nsgp.LIB_PATH), 'run `python __graft_entry__.py` (build) first'
    lib = nsgp.load_library()                     # raises BackendError on any missing symbol
    assert lib.nsgp_abi_version() == 2            # 2: the uncalled nsgp_kl_whitened_total_fwd_* left the ABI
    assert not [n for n in nsgp.declared_symbols() if n.startswith('nsgp_kl_whitened_total_fwd')]
    assert lib.nsgp_build_arch() == b'gfx950'
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for name in nsgp.declared_symbols():
        assert hasattr(raw, name), name
    # host-only size queries are safe without a GPU
    assert lib.nsgp_potrf_workspace(1024, 3, 8) == 3 * 16 * 64 * 64 * 8
    assert lib.nsgp_gemm_workspace(1024, 40960, 1024, 1, 1, 4, 0) == 0
    assert lib.nsgp_gemm_workspace(1024, 1024, 40960, 1, 1, 4, 16) > 0
    from nsgp import ops
    assert tuple(ops.pairwise_bwd_plan(2, 1024, 1024)) == (16, 64, 4) and tuple(ops.pairwise_bwd_plan(1, 4096, 4096)) == (64, 64, 16)


def test_no_signature_in_the_header_uses_torch_or_cxx_types():
    from nsgp import _lib
    text = _lib._strip_comments(open(_lib.HEADER).read())
    assert 'at::' not in text and 'torch' not in text and 'std::' not in text and 'template' not in text
    assert re.search(r'extern\s+"C"', text)


def test_product_fails_loudly_without_a_gpu_or_on_cpu_tensors():
    from nsgp import ops, BackendError
    x = torch.randn(5, 2)
    e = torch.ones(2, 5)
    with pytest.raises(BackendError):
        ops.gibbs_build(x, x, e, e)
    with pytest.raises(BackendError):
        ops.gemm(x, x, tb=True)
    with pytest.raises(BackendError):
        ops.potrf(torch.eye(4))


def test_product_never_imports_the_oracle():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nonstationary-precip_amd')
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, re.M), os.path.join(dp, f)


def test_potrf_trtri_rejects_bad_arguments_with_error_codes_not_faults():
    """nsgp_potrf_trtri_* validate their pointers and leading dimensions before any launch, like nsgp_potrf /
    nsgp_trtri (a negative return = index of the bad argument).  The checks run on the host: safe without a GPU."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 16)()
    info = (ctypes.c_int32 * 1)()
    ws = (ctypes.c_char * 65536)()
    P = lambda o: ctypes.cast(o, ctypes.c_void_p)
    ok = dict(A=P(buf), n=2, lda=2, sA=4, batch=1, info=P(info), X=P(buf), ldx=2, sX=4)

    def call(name, **kw):
        a = dict(ok, **kw)
        extra = (None, None) if name.endswith('w32') else ()
        return getattr(lib, name)(a['A'], a['n'], a['lda'], a['sA'], a['batch'], a['info'], a['X'], a['ldx'], a['sX'], *extra,
                                  P(ws), 65536, None)
    for name in ('nsgp_potrf_trtri_f32', 'nsgp_potrf_trtri_f64', 'nsgp_potrf_trtri_f64_w32'):
        assert call(name, A=None) == -1
        assert call(name, n=-1) == -2
        assert call(name, lda=1) == -3
        assert call(name, batch=-1) == -5
        assert call(name, batch=70000) == -5
        assert call(name, info=None) == -6
        assert call(name, X=None) == -7
        assert call(name, ldx=1) == -8
        assert call(name, n=0) == 0 and call(name, batch=0) == 0


def test_round3_entry_points_validate_their_arguments_on_the_host():
    """The int8 projection entry points, their planner queries and the matrix-core rate probe reject bad arguments with the
    index of the offending one before any launch (safe without a GPU), and the planner queries answer from sizes alone."""
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_double * 64)()
    P = lambda o: ctypes.cast(o, ctypes.c_void_p)
    b = P(buf)
    # planner queries (csrc/gemm_i8.hip: 128-row tiles, 64-column tiles, 32-deep k-blocks, 16-byte pieces)
    assert lib.nsgp_i8_supported(1024) == 1 and lib.nsgp_i8_supported(4096) == 1 and lib.nsgp_i8_supported(4097) == 0
    assert lib.nsgp_i8_tiles(1024) == 8 and lib.nsgp_i8_tiles(1000) == 8 and lib.nsgp_i8_tiles(0) == 0
    assert lib.nsgp_i8_w_planes_bytes(2, 1024) == 2 * 5 * 32 * 2 * 1024 * 16
    assert lib.nsgp_i8_k_planes_bytes(1, 1024, 4096, 4) == 4 * 32 * 2 * 4096 * 16
    assert lib.nsgp_i8_k_planes_bytes(1, 1024, 4096, 3) == 0                     # only 4 or 5 planes exist
    # one digit-scale slot per build workgroup (32-deep k-block x 256 columns of the 64-padded n)
    assert lib.nsgp_i8_kscale_count(2, 1024, 4096) == 2 * 32 * 16 and lib.nsgp_i8_kscale_count(1, 33, 65) == 2 * 1
    assert lib.nsgp_i8_kscale_count(1, 1024, 0) == 0
    # slicing W
    assert lib.nsgp_i8_slice_w_f64(None, 1, 128, b, b, None) == -1
    assert lib.nsgp_i8_slice_w_f64(b, -1, 128, b, b, None) == -2
    assert lib.nsgp_i8_slice_w_f64(b, 1, 5000, b, b, None) == -3
    assert lib.nsgp_i8_slice_w_f64(b, 1, 128, None, b, None) == -4
    assert lib.nsgp_i8_slice_w_f64(b, 1, 128, b, None, None) == -5
    assert lib.nsgp_i8_slice_w_f64(b, 0, 128, b, b, None) == 0
    # the product
    ok = [b, b, b, b, 4, None, 1, 128, 64, b, None, b, 1, 0, None]
    bad = lambda i, v: lib.nsgp_svgp_tri_gemm_colstats_i8(*[v if k == i else a for k, a in enumerate(ok)])
    assert bad(0, None) == -1 and bad(1, None) == -2 and bad(2, None) == -3 and bad(3, None) == -4
    assert bad(4, 3) == -5 and bad(4, 6) == -5
    assert bad(6, -1) == -6 and bad(7, 5000) == -7 and bad(8, -1) == -8 and bad(9, None) == -9 and bad(11, None) == -11
    assert bad(12, 0) == -12                                                      # fewer partial rows than tile rows
    assert bad(8, 0) == 0 and bad(6, 0) == 0
    # the rate probe
    assert lib.nsgp_mfma_rate_probe(3, 256, 16, b, b, None) == -1
    assert lib.nsgp_mfma_rate_probe(0, 0, 16, b, b, None) == -2
    assert lib.nsgp_mfma_rate_probe(0, 256, 15, b, b, None) == -3                # iterations: a multiple of 16
    assert lib.nsgp_mfma_rate_probe(0, 256, 16, None, b, None) == -4
    assert lib.nsgp_mfma_rate_probe(0, 256, 16, b, None, None) == -5
