"""Host-side checks of the mean-field variational family (no GPU): the class surface of MeanFieldVariationalDistribution,
the `variational=` keyword of models.dgps, the plan of a projection without a second product, and the argument checks of
the new entry points (negative return = index of the offending argument, before any launch)."""
import ctypes

import pytest
import torch

F32, F64 = torch.float32, torch.float64


def test_class_is_exported_with_gpytorch_parameter_names_shapes_and_initial_values():
    import nsgp.gp as gpytorch
    from nsgp.gp.lazy import DiagLazyTensor
    from nsgp.gp.variational import MeanFieldVariationalDistribution, _VariationalDistribution
    assert gpytorch.variational.MeanFieldVariationalDistribution is MeanFieldVariationalDistribution
    assert issubclass(MeanFieldVariationalDistribution, _VariationalDistribution)
    for batch_shape in ((), (2,)):
        q = MeanFieldVariationalDistribution(7, batch_shape=torch.Size(batch_shape))
        params = dict(q.named_parameters())
        assert sorted(params) == ['_variational_stddev', 'variational_mean']
        assert tuple(params['variational_mean'].shape) == (*batch_shape, 7)
        assert tuple(params['_variational_stddev'].shape) == (*batch_shape, 7)
        assert torch.equal(params['variational_mean'], torch.zeros(*batch_shape, 7))
        assert torch.equal(params['_variational_stddev'], torch.ones(*batch_shape, 7))
        assert q.mean_init_std == 1e-3 and q.num_inducing_points == 7 and q.batch_shape == torch.Size(batch_shape)
        dist = q()
        assert isinstance(dist.lazy_covariance_matrix, DiagLazyTensor)
        assert torch.equal(dist.mean, torch.zeros(*batch_shape, 7))
        assert torch.equal(dist.lazy_covariance_matrix.evaluate(), torch.eye(7).expand(*batch_shape, 7, 7))
        # initialisation: mean ~ N(0, mean_init_std^2), stddev <- 1
        with torch.no_grad():
            q._variational_stddev.fill_(3.0)
        torch.manual_seed(0)
        q.initialize_variational_distribution()
        assert torch.equal(q._variational_stddev, torch.ones(*batch_shape, 7))
        assert 0.0 < float(q.variational_mean.detach().abs().max()) < 6e-3


def test_state_dict_round_trips_and_the_sign_of_the_raw_stddev_does_not_matter():
    from nsgp.gp.variational import MeanFieldVariationalDistribution
    g = torch.Generator().manual_seed(3)
    a = MeanFieldVariationalDistribution(5, batch_shape=torch.Size([2]))
    raw = torch.randn(2, 5, generator=g)
    raw[0, 1] = 1e-12
    with torch.no_grad():
        a.variational_mean.copy_(torch.randn(2, 5, generator=g))
        a._variational_stddev.copy_(raw)
    sd = a.state_dict()
    assert sorted(sd) == ['_variational_stddev', 'variational_mean']
    b = MeanFieldVariationalDistribution(5, batch_shape=torch.Size([2]))
    b.load_state_dict(sd)
    assert torch.equal(b._variational_stddev, raw) and torch.equal(b.variational_mean, a.variational_mean)
    cov = a().lazy_covariance_matrix.evaluate()
    with torch.no_grad():
        b._variational_stddev.copy_(raw.abs())
    assert torch.equal(b().lazy_covariance_matrix.evaluate(), cov)
    assert torch.equal(torch.diagonal(cov, dim1=-1, dim2=-2), raw.abs().clamp_min(1e-8) ** 2)
    assert float(a.variational_stddev[0, 1].detach()) == pytest.approx(1e-8)
    # where the clamp is active the raw parameter gets a zero gradient, elsewhere sign(raw) * upstream
    a.variational_stddev.sum().backward()
    want = torch.sign(raw)
    want[0, 1] = 0.0
    assert torch.equal(a._variational_stddev.grad, want)


def test_models_dgps_variational_keyword():
    import models.dgps as m
    pre = 'variational_strategy._variational_distribution.'
    torch.manual_seed(0)
    model = m.DeepGP(1, (100, 3), num_inducing=16, variational='mean_field')
    sd = model.state_dict()
    assert not any('chol_variational_covar' in k for k in sd)
    assert tuple(sd['layers.0.' + pre + '_variational_stddev'].shape) == (2, 16)
    assert tuple(sd['layers.0.' + pre + 'variational_mean'].shape) == (2, 16)
    assert tuple(sd['last_layer.' + pre + '_variational_stddev'].shape) == (16,)
    assert tuple(sd['last_layer.' + pre + 'variational_mean'].shape) == (16,)
    untied = m.DeepGP(2, (100, 2), num_inducing=8, tie_layers=False, variational='mean_field')
    assert not any('chol_variational_covar' in k for k in untied.state_dict()) and len({id(l) for l in untied.layers}) == 2
    # the default is what it was: the keys and shapes tests/test_host_cpu.py expects
    torch.manual_seed(0)
    sd = m.DeepGP(1, (1000, 3)).state_dict()
    want = {
        'layers.0.variational_strategy.inducing_points': (2, 250, 3),
        'layers.0.' + pre + 'variational_mean': (2, 250), 'layers.0.' + pre + 'chol_variational_covar': (2, 250, 250),
        'layers.0.mean_module.weights': (3, 1), 'layers.0.mean_module.bias': (1,),
        'layers.0.covar_module.raw_outputscale': (2,), 'layers.0.covar_module.base_kernel.raw_lengthscale': (2, 1, 3),
        'last_layer.variational_strategy.inducing_points': (250, 2),
        'last_layer.' + pre + 'variational_mean': (250,), 'last_layer.' + pre + 'chol_variational_covar': (250, 250),
        'last_layer.mean_module.constant': (1,), 'last_layer.covar_module.raw_outputscale': (),
        'last_layer.covar_module.base_kernel.raw_lengthscale': (1, 2), 'likelihood.noise_covar.raw_noise': (1,),
    }
    for k, shp in want.items():
        assert k in sd and tuple(sd[k].shape) == shp, k
    assert not any('_variational_stddev' in k for k in sd)
    assert set(m.DeepGP(1, (1000, 3), variational='cholesky').state_dict()) == set(sd)
    for bad in ('meanfield', 'natural', None):
        with pytest.raises(ValueError):
            m.DeepGP(1, (100, 3), num_inducing=4, variational=bad)
        with pytest.raises(ValueError):
            m.DeepGPHiddenLayer(3, 2, num_inducing=4, variational=bad)


def test_plan_of_a_projection_without_a_second_product():
    from nsgp import BackendError, _lib, ops
    lib = _lib.load()
    pre = 'nsgp_svgp_tri_gemm_colstats_'
    p1 = {'f32': pre + 'f32', 'f64acc': pre + 'f64acc', 'f64acc_b64': pre + 'f64acc_b64p32', 'i8': pre + 'i8',
          'kzx_fused': 'nsgp_svgp_kzx_gemm_colstats_f64acc', 'bf16': pre + 'bf16'}
    for M, n, b in ((1, 1, 1), (63, 65, 2), (1024, 4096, 1)):
        for first in p1:
            if first == 'bf16' and M % 8:
                with pytest.raises(BackendError):
                    ops.svgp_projection_plan(M, n, b, F32, first, 'diag')
                continue
            p = ops.svgp_projection_plan(M, n, b, F32, first, 'diag', 5)
            T1 = {'f32': lib.nsgp_svgp_colstats_tiles(M, n, b, 4), 'i8': lib.nsgp_i8_tiles(M),
                  'bf16': lib.nsgp_svgp_bf16_tiles(M)}.get(first, lib.nsgp_svgp_f64acc_tiles_for(M, n, b))
            assert p == ops.ProjectionPlan(first, 'diag', 5 if first == 'i8' else 0, p1[first], 'nsgp_svgp_diag_colsq_f32',
                                           'nsgp_svgp_colstats_finalize_diag_f32', T1, (M + 31) // 32, T1, F32, False, False)
            assert p.T1 >= 1 and p.T2 >= 1
        p = ops.svgp_projection_plan(M, n, b, F64, 'f32', 'diag')
        assert (p.p1, p.p2, p.fin, p.part_dtype, p.zero) == (pre + 'f64', 'nsgp_svgp_diag_colsq_f64',
                                                              'nsgp_svgp_colstats_finalize_diag_f64', F64, False)
        assert p.T == p.T1 == lib.nsgp_svgp_colstats_tiles(M, n, b, 8) and p.T2 == (M + 31) // 32
        for first in ('f64acc', 'i8', 'bf16', 'kzx_fused', 'f64acc_b64'):        # float64 layers: the plain product only
            with pytest.raises(BackendError):
                ops.svgp_projection_plan(M, n, b, F64, first, 'diag')
    with pytest.raises(BackendError):
        ops.svgp_projection_plan(64, 64, 1, F32, 'f64acc_t', 'diag')
    assert lib.nsgp_svgp_diag_tiles(0) == 0 and lib.nsgp_svgp_diag_tiles(32) == 1 and lib.nsgp_svgp_diag_tiles(33) == 2


def test_existing_plan_rows_are_what_they_were():
    """Literal copies of what svgp_projection_plan returned before 'diag' existed."""
    from nsgp import ops
    P, pre, fin = ops.ProjectionPlan, 'nsgp_svgp_tri_gemm_colstats_', 'nsgp_svgp_colstats_finalize_affine_'
    assert ops.svgp_projection_plan(1024, 4096, 2, F32, 'i8', 'f64acc_t', 5) == \
        P('i8', 'f64acc_t', 5, pre + 'i8', pre + 'f64acc_t', fin + 'p64_f32', 8, 8, 8, F64, True, False)
    assert ops.svgp_projection_plan(1024, 40960, 1, F32, 'i8', 'f32', 4) == \
        P('i8', 'f32', 4, pre + 'i8', pre + 'rows_f32', fin + 'f32', 8, 8, 8, F32, False, False)
    assert ops.svgp_projection_plan(1024, 4032, 1, F32, 'f64acc', 'f32') == \
        P('f64acc', 'f32', 0, pre + 'f64acc', pre + 'rows_f32', fin + 'f32', 16, 8, 16, F32, True, False)
    assert ops.svgp_projection_plan(63, 65, 2, F64, 'f32', 'f32') == \
        P('f32', 'f32', 0, pre + 'f64', pre + 'rows_f64', fin + 'f64', 1, 1, 1, F64, False, False)
    assert ops.svgp_projection_plan(1024, 4096, 1, F32, 'bf16', 'bf16') == \
        P('bf16', 'bf16', 0, pre + 'bf16', pre + 'bf16', fin + 'f32', 8, 8, 8, F32, False, False)
    assert ops.svgp_projection_plan(1024, 4096, 1, F32, 'f64acc_b64', 'f64acc_t') == \
        P('f64acc_b64', 'f64acc_t', 0, pre + 'f64acc_b64', pre + 'f64acc_t', fin + 'p64_f32', 8, 8, 8, F64, False, False)


def test_selection_with_a_diagonal_q_keeps_the_first_product_and_the_planes():
    from nsgp.svgp import select_projection
    base = dict(dtype=F32, M=1024, D=2, n=4096, kzx_f64=True, has_w64=True, fusable=True, forward_precision='f32',
                whiten_matmul_f64=True, whiten_matmul_i8=True, fuse_kzx=False, hidden_var_f64='auto')
    for over in ({}, dict(n=40960, kzx_f64=False), dict(fuse_kzx=True), dict(whiten_matmul_i8=False), dict(D=5),
                 dict(forward_precision='bf16'), dict(forward_precision='bf16_all', whiten_matmul_f64=False),
                 dict(forward_precision='bf16', M=252), dict(whiten_matmul_f64=False), dict(dtype=F64)):
        chol = select_projection(**{**base, **over})
        diag = select_projection(**{**base, **over}, diag_q=True)
        assert diag == (chol[0], 'diag', chol[2], chol[3]), over
        assert select_projection(**{**base, **over}, diag_q=False) == chol


def _P(o):
    return ctypes.cast(o, ctypes.c_void_p)


def test_new_entry_points_are_exported_and_validate_their_arguments_on_the_host():
    import nsgp
    lib = nsgp.load_library()
    assert lib.nsgp_abi_version() == 2
    names = nsgp.declared_symbols()
    for stem in ('svgp_diag_colsq', 'svgp_colstats_finalize_diag', 'svgp_diag_bwd', 'kl_meanfield_total_acc_fwd',
                 'kl_meanfield_total_bwd'):
        for sfx in ('f32', 'f64'):
            assert f'nsgp_{stem}_{sfx}' in names and hasattr(ctypes.CDLL(nsgp.LIB_PATH), f'nsgp_{stem}_{sfx}'), (stem, sfx)
    assert 'nsgp_svgp_diag_tiles' in names and 'nsgp_svgp_diag_bwd_workspace' in names
    buf = (ctypes.c_double * 4096)()
    b = _P(buf)

    def check(name, ok, bad, zero):
        """ok: a valid argument list; bad: {position: (value, code)}; zero: positions whose 0 means an empty problem."""
        fn = getattr(lib, name)
        for i, (v, code) in bad.items():
            for val, c in (zip(v, code) if isinstance(v, tuple) else ((v, code),)):
                assert fn(*[val if k == i else a for k, a in enumerate(ok)]) == c, (name, i, val)
        for i in zero:
            assert fn(*[0 if k == i else a for k, a in enumerate(ok)]) == 0, (name, i)

    for sfx in ('f32', 'f64'):
        # (A, s2m1, batch, M, n, part_q, T, stream): T = ceil(40 / 32) = 2 partial rows at least
        check(f'nsgp_svgp_diag_colsq_{sfx}', [b, b, 1, 40, 8, b, 2, None],
              {0: (None, -1), 1: (None, -2), 2: ((-1, 70000), (-3, -3)), 3: (-1, -4), 4: (-1, -5), 5: (None, -6),
               6: ((1, -1), (-7, -7))}, (2, 3, 4))
        # (part_dot, tiles, part_q, qtiles, base, base_add, batch, n, x, sxb, D, w, swb, c, scb, mean, var, stream)
        check(f'nsgp_svgp_colstats_finalize_diag_{sfx}', [b, 1, b, 2, b, 1e-4, 1, 8, b, 0, 2, b, 0, b, 0, b, b, None],
              {0: (None, -1), 1: (-1, -2), 2: (None, -3), 3: (-1, -4), 4: (None, -5), 6: (-1, -7), 7: (-1, -8), 8: (None, -9),
               9: (-1, -10), 10: ((-1, 0, 99), (-11, -11, -11)), 12: (-1, -13), 14: (-1, -15), 15: (None, -16), 16: (None, -17)},
              (6, 7))
        # (A, m, s2m1, gmean, gvar, batch, M, n, Abar, mbar, tbar, ws, ws_bytes, stream)
        need = lib.nsgp_svgp_diag_bwd_workspace(1, 40, 5000)
        assert need == 1 * 40 * 2 * 2 * 8 and lib.nsgp_svgp_diag_bwd_workspace(2, 3, 4096) == 2 * 3 * 1 * 2 * 8
        assert lib.nsgp_svgp_diag_bwd_workspace(0, 40, 8) == 0 and lib.nsgp_svgp_diag_bwd_workspace(1, 40, 0) == 0
        check(f'nsgp_svgp_diag_bwd_{sfx}', [b, b, b, b, b, 1, 40, 5000, b, b, b, b, need, None],
              {0: (None, -1), 1: (None, -2), 2: (None, -3), 3: (None, -4), 4: (None, -5), 5: ((-1, 70000), (-6, -6)),
               6: (-1, -7), 7: (-1, -8), 8: (None, -9), 9: (None, -10), 10: (None, -11), 11: (None, -12),
               12: (need - 1, -13)}, (5, 6, 7))
        # (m, s2, batch, M, scale, addin, out, ws, wsb, stream)
        check(f'nsgp_kl_meanfield_total_acc_fwd_{sfx}', [b, b, 2, 40, 1.0, None, b, b, 65536, None],
              {0: (None, -1), 1: (None, -2), 2: (-1, -3), 3: (-1, -4), 6: (None, -7), 7: (None, -8), 8: (3, -9)}, (2, 3))
        # (m, s2, batch, M, scale, gout, gm, gs2, stream)
        check(f'nsgp_kl_meanfield_total_bwd_{sfx}', [b, b, 2, 40, 1.0, b, b, b, None],
              {0: (None, -1), 1: (None, -2), 2: (-1, -3), 3: (-1, -4), 5: (None, -6), 6: (None, -7), 7: (None, -8)}, (2, 3))


def test_mean_field_ops_fail_loudly_on_cpu_tensors():
    from nsgp import BackendError, ops
    m, s2 = torch.zeros(2, 4), torch.ones(2, 4)
    with pytest.raises(BackendError):
        ops.kl_meanfield_total(m, s2)
    with pytest.raises(BackendError):
        ops.svgp_project_diag('f32', torch.eye(4).expand(2, 4, 4), s2 - 1, m, torch.ones(2), Kzx=torch.zeros(2, 4, 3))
    with pytest.raises(ValueError):
        from nsgp.svgp import svgp_marginal
        svgp_marginal(torch.zeros(3, 1), torch.zeros(2, 4, 1), torch.ones(2, 1), torch.ones(2), m)
