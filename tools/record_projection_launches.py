"""Record what the SVGP forward projection launches: entry-point names and every non-pointer argument.

    python tools/record_projection_launches.py --out tests/golden/projection_launches.json
    python tools/record_projection_launches.py --dump DIR       # + sha256 of the raw bytes of A, C, mean, var per case

The forward projection is host code that picks kernels, tile-row counts and a partials layout from sizes and settings
(nsgp/ops.py, nsgp/svgp.py).  This tool wraps `nsgp._lib.call` for the duration of one forward call and writes, per case,
the list of launches: the entry point, each integer / float argument, and for each pointer argument only whether it is
null ('p' / '0').  It drives the public surface only -- ops.svgp_project, ops.svgp_project_bf16, svgp.svgp_marginal and
the settings -- so the same file records any commit; tests/test_gpu_projection_launches.py replays the committed record
on the code under test and tests/test_projection_plan.py checks the pure planners against it without a GPU.

File layout (names and integers only): `launches` is the table of distinct launch lists, `cases` maps a case id to its
row in that table.  Case ids:
    direct  'd|b,M,n,D|<form>|<a0|a1>'                      form: DIRECT_FORMS, a1 = with an affine prior mean
    layer   'l|b,M,n,D|fp,w64,i8,fuse,hkzx,hvar|k<0|1>g<0|1>'   the settings, kzx_f64, gradients required

--dump: outputs come from seeded inputs; before each case a NaN-filled block a few times the size of the partials is
allocated and freed, so a partials buffer that should have been zero-filled and was not reads NaN instead of whatever zeros
the allocator left by chance.  The arrays of the large shapes add up to many GB, so the dump holds the sha256 of each
array's raw bytes; two dumps agree bit for bit (NaNs included) exactly when their digests do (`--compare A B`).
"""
import argparse
import contextlib
import ctypes
import hashlib
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

# (batch, M, n, D) and the tile rows the planner queries give (float32 plan / f64acc / int8 / bf16), which
# tests/test_projection_plan.py asserts so that every layout condition keeps a case:
SHAPES = [
    (1, 1024, 4096, 2),     # headline first layer, 8/8/8/8: nothing to zero but for int8 + Lq64 (kept, see ops)
    (1, 1024, 40960, 2),    # headline last layer: n > 8192 turns hidden_var_f64 'auto' off
    (1, 1024, 4032, 2),     # 8/16/8/8: f64acc rows != float32 plan's; int8 + Lq64 leaves float64 rows unwritten
    (3, 1000, 4000, 3),     # batch 3, M not a multiple of 128, n not one of 64: generated Kzx unsupported
    (3, 256, 512, 2),       # batch 3, 4/4/2/2: bf16 rows fewer than product 1's (compact scratch, then widened)
    (2, 252, 320, 2),       # M % 8 != 0: the bf16 modes fall back to svgp_project
    (1, 256, 384, 5),       # D = 5: int8 and generated Kzx unavailable
]
DIRECT_FORMS = ['f32', 'f64', 'w64', 'k64', 'k64_lq64', 'kin', 'i8p4', 'i8p5', 'i8p4_lq64', 'i8p5_lq64',
                'bf16', 'bf16_w64', 'bf16_i8', 'bf16_kin', 'bf16_kin_w64']
LAYER_SETTINGS = list(itertools.product(('f32', 'bf16', 'bf16_all'), (0, 1), (0, 1), (0, 1), (0, 1), ('auto', 1, 0)))


def shape_key(shape):
    return ','.join(str(v) for v in shape)


def layer_key(shape, s, kzx_f64, grad):
    return f"l|{shape_key(shape)}|{','.join(str(v) for v in s)}|k{int(kzx_f64)}g{int(grad)}"


def direct_key(shape, form, affine):
    return f'd|{shape_key(shape)}|{form}|a{int(affine)}'


def direct_available(shape, form):
    """Forms a shape cannot run (they raise by contract) are not cases."""
    b, M, n, D = shape
    if form.startswith('bf16') and M % 8:
        return False
    if 'i8' in form and (D > 4 or M > 4096):
        return False
    if form == 'kin':
        from nsgp import _lib
        return bool(_lib.load().nsgp_svgp_kzx_gemm_supported(None, M, n, b, D))
    return True


@contextlib.contextmanager
def recording(log):
    from nsgp import _lib
    real = _lib.call

    def call(name, *args):
        argtypes = _lib.PROTOTYPES[name][1]
        row = [name]
        for ty, a in zip(argtypes, args):
            if ty is ctypes.c_void_p:
                row.append('0' if (a is None or not getattr(a, 'value', a)) else 'p')
            else:
                row.append(a)
        log.append(row)
        return real(name, *args)
    _lib.call = call
    try:
        yield log
    finally:
        _lib.call = real


@contextlib.contextmanager
def layer_settings(s):
    from nsgp.gp import settings
    fp, w64, i8, fuse, hkzx, hvar = s
    with settings.forward_precision(fp), settings.whiten_matmul_f64(bool(w64)), settings.whiten_matmul_i8(bool(i8)), \
            settings.fuse_kzx(bool(fuse)), settings.hidden_kzx_f64(bool(hkzx)), \
            settings.hidden_var_f64(hvar if hvar == 'auto' else bool(hvar)):
        yield


def make_inputs(shape, seed=173):
    """Seeded operands of one shape: a real whitening factor (W = chol(Kzz)^-1), a unit-diagonal-ish Lq."""
    import torch
    from nsgp import ops, svgp
    b, M, n, D = shape
    g = torch.Generator().manual_seed(seed + 7 * M + n + D + b)
    r = lambda *s: torch.randn(*s, generator=g)                     # noqa: E731
    t = dict(Z=r(b, M, D), x=r(n, D), ls=0.7 + 0.3 * torch.rand(b, D, generator=g), os=0.8 + 0.4 * torch.rand(b, generator=g),
             m=r(b, M), Lq=torch.tril(0.05 * r(b, M, M)) + torch.eye(M), w=0.3 * r(b, D), c=0.1 * r(b))
    t = {k: v.cuda() for k, v in t.items()}
    with torch.no_grad():
        (W,), _, (W64,) = svgp.whiten([(t['Z'], t['ls'], t['os'])], out_dtype=torch.float32, with_f64=True)
        t['W'], t['W64'] = W.contiguous(), W64.contiguous()
        t['Kzx'] = ops.rbf_build(t['Z'], t['x'], t['ls'], t['os'])
        for k in ('Z', 'x', 'ls', 'os', 'm', 'Lq', 'w', 'c'):
            t[k + '64'] = t[k].double()
        t['Kzx64'] = ops.rbf_build(t['Z64'], t['x64'], t['ls64'], t['os64'])
    return t


def run_direct(t, form, affine):
    from nsgp import ops
    kin = (t['Z'], t['x'], t['ls'], t['os'])
    if form == 'f64':
        aff = (t['x64'], t['w64'], t['c64']) if affine else None
        return ops.svgp_project(t['W64'], t['Kzx64'], t['Lq64'], t['m64'], t['os64'], base_add=1e-4, affine=aff)
    aff = (t['x'], t['w'], t['c']) if affine else None
    a = (t['W'], t['Kzx'], t['Lq'], t['m'], t['os'])
    nok = (t['W'], None, t['Lq'], t['m'], t['os'])
    kw = dict(base_add=1e-4, affine=aff)
    if form == 'f32':
        return ops.svgp_project(*a, **kw)
    if form == 'w64':
        return ops.svgp_project(*a, W64f=t['W64'], **kw)
    if form in ('k64', 'k64_lq64'):
        return ops.svgp_project(*nok, W64f=t['W64'], Kzx64=t['Kzx64'], Lq64=t['Lq64'] if 'lq64' in form else None, **kw)
    if form == 'kin':
        return ops.svgp_project(*nok, W64f=t['W64'], kernel_inputs=kin, **kw)
    if form.startswith('i8p'):
        return ops.svgp_project(*nok, W64f=t['W64'], i8_inputs=kin, i8_planes=int(form[3]),
                                Lq64=t['Lq64'] if 'lq64' in form else None, **kw)
    if form == 'bf16':
        return ops.svgp_project_bf16(*a, **kw)
    if form == 'bf16_w64':
        return ops.svgp_project_bf16(*a, W64f=t['W64'], **kw)
    if form == 'bf16_i8':
        return ops.svgp_project_bf16(*nok, W64f=t['W64'], i8_inputs=kin, **kw)
    if form == 'bf16_kin':
        return ops.svgp_project_bf16(*a, kernel_inputs=kin, **kw)
    if form == 'bf16_kin_w64':
        return ops.svgp_project_bf16(*a, W64f=t['W64'], kernel_inputs=kin, **kw)
    raise ValueError(form)


def run_layer(t, kzx_f64, grad):
    """One SVGPLayerFn.forward under the settings in force, on a precomputed whitening factor (its launches are not the
    projection's).  Returns (mean, var)."""
    import torch
    from nsgp import svgp
    leaves = [t[k].detach().clone().requires_grad_(grad) for k in ('Z', 'ls', 'os', 'm', 'Lq', 'w', 'c')]
    Z, ls, os_, m, Lq, w, c = leaves
    with torch.set_grad_enabled(grad):
        mean, var, _ = svgp.svgp_marginal(t['x'], Z, ls, os_, m, Lq, W64=t['W'], W64f=t['W64'], mean_w=w, mean_c=c,
                                          kzx_f64=kzx_f64)
    return mean, var


def poison(shape):
    """Allocate and free NaN-filled blocks a few times the size of the largest partials buffer of this shape, in both of the
    caching allocator's pools, so that the next torch.empty of a partials buffer is carved out of NaNs."""
    import torch
    b, M, n, D = shape
    part = 3 * b * ((M + 63) // 64) * n * 8
    torch.cuda.empty_cache()
    blocks = [torch.full((4 * part // 4,), float('nan'), device='cuda')]
    if part <= 2 ** 20:
        blocks.append(torch.full((2 ** 20 // 4,), float('nan'), device='cuda'))
    del blocks


def digest(*arrays):
    return [hashlib.sha256(a.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for a in arrays]


def cases(shapes=SHAPES):
    """(key, shape, runner(t) -> outputs) for every case, in a fixed order."""
    for shape in shapes:
        for form in DIRECT_FORMS:
            if direct_available(shape, form):
                for affine in (False, True):
                    yield direct_key(shape, form, affine), shape, (lambda t, f=form, a=affine: run_direct(t, f, a)), None
        for s in LAYER_SETTINGS:
            for kzx_f64 in (False, True):
                for grad in (False, True):
                    yield (layer_key(shape, s, kzx_f64, grad), shape,
                           (lambda t, k=kzx_f64, g=grad: run_layer(t, k, g)), s)


def record(shapes=SHAPES, dump=False, only=None):
    """{case id: launch list} (and {case id: digests} with dump) for every case, or for the ids in `only`."""
    import torch
    launches, digests, inputs = {}, {}, {}
    for key, shape, run, s in cases(shapes):
        if only is not None and key not in only:
            continue
        if shape not in inputs:
            inputs.clear()
            inputs[shape] = make_inputs(shape)
            print(f'shape {shape} ...', file=sys.stderr, flush=True)
        if dump:
            poison(shape)
        log = []
        with layer_settings(s) if s is not None else contextlib.nullcontext():
            with recording(log):
                out = run(inputs[shape])
        launches[key] = log
        if dump:
            digests[key] = digest(*out)
        del out
    torch.cuda.synchronize()
    return launches, digests


_KG = ('k0g0', 'k0g1', 'k1g0', 'k1g1')


def pack(launches):
    """Distinct launch lists once; the four (kzx_f64, gradients) variants of a layer case share one entry."""
    table, index, out = [], {}, {}
    for key, log in launches.items():
        k = json.dumps(log)
        if k not in index:
            index[k] = len(table)
            table.append(log)
        if key.startswith('l|'):
            head, kg = key.rsplit('|', 1)
            out.setdefault(head, [None] * 4)[_KG.index(kg)] = index[k]
        else:
            out[key] = index[k]
    return {'shapes': [list(s) for s in SHAPES], 'launches': table, 'cases': out}


def unpack(doc):
    """{case id: launch list} of a packed record."""
    out = {}
    for key, i in doc['cases'].items():
        if isinstance(i, list):
            out.update({f'{key}|{kg}': doc['launches'][j] for kg, j in zip(_KG, i) if j is not None})
        else:
            out[key] = doc['launches'][i]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='write the launch record (JSON) here')
    ap.add_argument('--dump', metavar='DIR', help='write DIR/outputs.json: sha256 of the raw bytes of each output per case')
    ap.add_argument('--compare', nargs=2, metavar=('A', 'B'), help='compare two --dump directories (and their launch records)')
    a = ap.parse_args()
    if a.compare:
        bad = 0
        for name in ('outputs.json', 'launches.json'):
            x, y = (json.load(open(os.path.join(d, name))) for d in a.compare)
            if name == 'launches.json':
                x, y = unpack(x), unpack(y)
            diff = sorted(k for k in set(x) | set(y) if x.get(k) != y.get(k))
            print(f'{name}: {len(x)} / {len(y)} cases, {len(diff)} differ' + ''.join(f'\n  {k}' for k in diff[:20]))
            bad += len(diff)
        sys.exit(1 if bad else 0)
    launches, digests = record(dump=bool(a.dump))
    doc = pack(launches)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(doc, f, separators=(',', ':'))
            f.write('\n')
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        with open(os.path.join(a.dump, 'launches.json'), 'w') as f:
            json.dump(doc, f, separators=(',', ':'))
        with open(os.path.join(a.dump, 'outputs.json'), 'w') as f:
            json.dump(digests, f, indent=0)
    print(f'{len(launches)} cases, {len(doc["launches"])} distinct launch lists')


if __name__ == '__main__':
    main()
