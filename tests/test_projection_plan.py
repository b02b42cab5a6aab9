"""The pure planners of the SVGP forward projection against the launch record of the commit before they existed.

tests/golden/projection_launches.json was written by tools/record_projection_launches.py on an MI355X at commit b04fea4,
when the choice of arithmetic and the partials layout were still inline branches of SVGPLayerFn.forward, ops.svgp_project
and ops.svgp_project_bf16.  For every recorded case, nsgp.svgp.select_projection and nsgp.ops.svgp_projection_plan -- sizes
and settings in, no tensor, no GPU -- must name the same entry points, the same tile rows T, the same partials dtype (the
finalize entry point) and the same compact-scratch case.  tests/test_gpu_projection_launches.py replays the record."""
import importlib.util
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, 'tests', 'golden', 'projection_launches.json')

# direct-call form of the recorder -> (layer dtype, first product, second product, int8 Kzx planes)
FORMS = {'f32': ('f32', 'f32', 4), 'f64': ('f32', 'f32', 4), 'w64': ('f64acc', 'f32', 4), 'k64': ('f64acc_b64', 'f32', 4),
         'k64_lq64': ('f64acc_b64', 'f64acc_t', 4), 'kin': ('kzx_fused', 'f32', 4), 'i8p4': ('i8', 'f32', 4),
         'i8p5': ('i8', 'f32', 5), 'i8p4_lq64': ('i8', 'f64acc_t', 4), 'i8p5_lq64': ('i8', 'f64acc_t', 5),
         'bf16': ('f32', 'bf16', 4), 'bf16_w64': ('f64acc', 'bf16', 4), 'bf16_i8': ('i8', 'bf16', 4),
         'bf16_kin': ('bf16', 'bf16', 4), 'bf16_kin_w64': ('bf16', 'bf16', 4)}
PRODUCTS = ('nsgp_svgp_tri_gemm_colstats', 'nsgp_svgp_kzx_gemm_colstats')


def recorder():
    spec = importlib.util.spec_from_file_location('record_projection_launches',
                                                  os.path.join(ROOT, 'tools', 'record_projection_launches.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def recorded():
    with open(RECORD) as f:
        return recorder().unpack(json.load(f))


def expected(key, lib):
    """(dtype, first, second, planes, builds) of a recorded case, from its id alone; builds: the rbf_build launches the
    forward makes for the projection (layer cases)."""
    from nsgp import svgp
    kind, shape, what, tail = key.split('|')
    b, M, n, D = (int(v) for v in shape.split(','))
    if kind == 'd':
        first, second, planes = FORMS[what]
        return (b, M, n), torch.float64 if what == 'f64' else torch.float32, first, second, planes, None
    fp, w64, i8, fuse, _hkzx, hvar = what.split(',')
    fusable = bool(int(fuse)) and bool(lib.nsgp_svgp_kzx_gemm_supported(None, M, n, b, D))
    first, second, planes, _ = svgp.select_projection(
        torch.float32, M, D, n, tail[1] == '1', True, fusable, fp, bool(int(w64)), bool(int(i8)), bool(int(fuse)),
        hvar if hvar == 'auto' else bool(int(hvar)))
    builds = ['nsgp_rbf_build_fwd_f64'] if first == 'f64acc_b64' else \
        ['nsgp_rbf_build_fwd_f32'] if first in ('f32', 'f64acc', 'bf16') else []
    return (b, M, n), torch.float32, first, second, planes, builds


def test_planners_reproduce_every_recorded_case():
    from nsgp import _lib, ops
    lib = _lib.load()
    cases = recorded()
    assert len(cases) > 4000
    bad = []
    for key, launches in cases.items():
        (b, M, n), dtype, first, second, planes, builds = expected(key, lib)
        plan = ops.svgp_projection_plan(M, n, b, dtype, first, second, planes)
        names = [r[0] for r in launches]
        fin = launches[-1]
        got = dict(products=[r for r in names if r.startswith(PRODUCTS)], fin=fin[0], T=fin[7],
                   p64=fin[0].endswith('_p64_f32'))
        want = dict(products=[plan.p1, plan.p2], fin=plan.fin, T=plan.T,
                    p64=plan.part_dtype == torch.float64 and dtype == torch.float32)
        for r in launches:                                   # every launch that takes the row count takes T
            if r[0].endswith(('_f64acc', '_f64acc_b64', '_f64acc_b64p32', '_f64acc_t', '_rows_f32', '_rows_f64')):
                got.setdefault('rows', set()).add(r[-2])
            if r[0].endswith('_colstats_i8'):
                got.setdefault('rows', set()).add(r[-3])
                got['i8'] = (r[5], r[-2])
                want['i8'] = (plan.planes, int(want['p64']))
        if 'rows' in got:
            want['rows'] = {plan.T}
        if second == 'bf16':                                 # the bf16 kernel's own tile rows; compact scratch iff fewer than T
            got['scratch'] = fin[7] != lib.nsgp_svgp_bf16_tiles(M)
            want['scratch'] = plan.scratch
            assert plan.T2 == lib.nsgp_svgp_bf16_tiles(M)
        if builds is not None:
            got['builds'] = [r for r in names if r.startswith('nsgp_rbf_build_fwd')]
            want['builds'] = builds
            got['lq64'] = any(r[0] == 'nsgp_cast_f32_to_f64' and r[2] == M for r in launches) or second != 'f64acc_t' \
                or first == 'f64acc_b64'
            want['lq64'] = True
        if got != want:
            bad.append((key, got, want))
    assert not bad, f'{len(bad)} of {len(cases)} cases differ, e.g. {bad[:3]}'


def test_zero_fill_rule_and_the_recorded_shapes_cover_every_layout_condition():
    """Zero-filled exactly when some row of some plane is written by no kernel -- plus int8 with float64 partials, always."""
    from nsgp import _lib, ops
    lib = _lib.load()
    seen = set()
    for b, M, n, D in recorder().SHAPES:
        for first, second, planes in set(FORMS.values()):
            if (second == 'bf16' and M % 8) or (first == 'i8' and D > 4):
                continue
            p = ops.svgp_projection_plan(M, n, b, torch.float32, first, second, planes)
            assert p.T == max(p.T1, p.T2) and p.T1 >= 1 and p.T2 >= 1
            rule = p.T1 < p.T or p.T2 < p.T
            assert p.zero == (rule or (first == 'i8' and second == 'f64acc_t'))
            assert p.scratch == (second == 'bf16' and p.T2 < p.T)
            assert not p.scratch or p.zero                   # the widened plane's other rows are zeros
            if first in ('f64acc', 'kzx_fused') and second == 'f32' and rule:
                seen.add('f64acc rows != float32 plan')
            if p.scratch:
                seen.add('bf16 rows < product 1')
            if first == 'i8' and second == 'f64acc_t':
                seen.add('i8, float64 partials, ' + ('rule zero-fills' if rule else 'kept zero-fill'))
    assert seen == {'f64acc rows != float32 plan', 'bf16 rows < product 1', 'i8, float64 partials, rule zero-fills',
                    'i8, float64 partials, kept zero-fill'}
    # the shape ops.py names: 8 tile rows in the float32 plan, 16 in the float64-accumulating kernel
    assert (lib.nsgp_svgp_colstats_tiles(1024, 4032, 1, 4), lib.nsgp_svgp_f64acc_tiles_for(1024, 4032, 1)) == (8, 16)


def test_plan_rejects_combinations_no_kernel_runs():
    from nsgp import BackendError, ops
    for dtype, first, second in ((torch.float64, 'f64acc', 'f32'), (torch.float32, 'f64acc', 'f64acc_t'),
                                 (torch.float32, 'bf16', 'f32'), (torch.float32, 'f32', 'bf16_all'),
                                 (torch.float16, 'f32', 'f32')):
        with pytest.raises(BackendError):
            ops.svgp_projection_plan(256, 512, 1, dtype, first, second)
    with pytest.raises(BackendError):
        ops.svgp_projection_plan(252, 512, 1, torch.float32, 'f32', 'bf16')      # bf16 needs M % 8 == 0


def test_malformed_kernel_inputs_raise_before_any_tensor_is_touched():
    from nsgp import BackendError, ops
    z = torch.zeros(1, 8, 2)
    for t in (None, (z, z, z), [z, z, z, None], 'Zxlo'):
        with pytest.raises(BackendError, match='expected'):
            ops._kernel_inputs_args(t, z, 'test')


def test_selection_precedence():
    from nsgp.svgp import select_projection
    f32 = torch.float32
    sel = lambda **k: select_projection(**{**dict(dtype=f32, M=1024, D=2, n=4096, kzx_f64=True, has_w64=True, fusable=True,  # noqa: E731
                                                  forward_precision='f32', whiten_matmul_f64=True, whiten_matmul_i8=True,
                                                  fuse_kzx=False, hidden_var_f64='auto'), **k})
    assert sel() == ('i8', 'f64acc_t', 5, True)                                  # the headline's first layer
    assert sel(n=40960, kzx_f64=False) == ('i8', 'f32', 4, True)                 # ... and its last
    assert sel(fuse_kzx=True)[:2] == ('kzx_fused', 'f32')                        # fuse wins over int8
    assert sel(whiten_matmul_i8=False)[:2] == ('f64acc_b64', 'f64acc_t')         # int8 wins over hidden_kzx_f64
    assert sel(D=5)[:2] == ('f64acc_b64', 'f64acc_t') and sel(M=4104)[0] == 'f64acc_b64'
    assert sel(n=8200)[1] == 'f32' and sel(n=8200, hidden_var_f64=True)[1] == 'f64acc_t'
    assert sel(forward_precision='bf16_all', whiten_matmul_f64=False) == ('bf16', 'bf16', 4, True)   # keeps the float64 W
    assert sel(forward_precision='bf16') == ('i8', 'bf16', 4, True)
    assert sel(forward_precision='bf16', M=252) == ('i8', 'f32', 5, True)        # M % 8: falls back to svgp_project
    assert sel(forward_precision='bf16_all', M=252, whiten_matmul_f64=False) == ('f64acc', 'f32', 5, True)
    assert sel(whiten_matmul_f64=False) == ('f32', 'f32', 5, False) and sel(dtype=torch.float64)[:2] == ('f32', 'f32')
