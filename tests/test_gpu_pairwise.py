"""Every row of tests/test_pairwise_cases_cpu.py on the GPU: the forward and backward pairwise builds of csrc/pairwise.hip
against float64, at every tile edge, launch path and stride.

Guards.  Every output (and K) is a window of a sentinel-filled buffer and so is the workspace (the bytes *_workspace()
reports, between two guards); nothing outside the windows may change.  Every input array is followed by NaN, and the padding
of G (ldg - n2 and between batch entries) holds NaN; no output may become NaN.

Forward.  One master build per (family, dtype, D, batching) -- the largest problem, K a window with aligned ld, batch stride
and base, i.e. the vector store path -- is held to the float64 oracle at the existing forward tolerances.  Every other forward
row (shape x layout) must torch.equal the matching slice of its master: an entry's arithmetic depends neither on its tile,
nor on ld, nor on the store path (vector or scalar).  The contiguous layout runs through nsgp.ops, the windows through the
C ABI.

Backward.  Every output element is held to |err| <= ((N + c) u + eps_fwd) sum |t| (test_pairwise_cases_cpu's docstring);
the achieved worst ratio is printed per row (run with -s).  Same-buffer rows are compared with the reference of g1 + g2.  Rows
the wrappers can express also run through nsgp.ops and must give the C ABI's bits."""
import ctypes
import itertools
import math

import pytest
import torch

import test_pairwise_cases_cpu as C
from test_pairwise_cases_cpu import BWD_CASES, DTYPES, FAMILIES, fam_kind

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
PAD = 8
WS_GUARD = 4096
NAN = float('nan')


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _ptr(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def dev_in(t):
    """A CPU array on the device, followed by NaN."""
    if t is None:
        return None
    flat = torch.full((t.numel() + PAD,), NAN, dtype=t.dtype, device='cuda')
    flat[:t.numel()] = t.reshape(-1).cuda()
    return flat[:t.numel()].view(t.shape)


def dev_inputs(p):
    return {k: dev_in(v) for k, v in p.items()}


class Window:
    """A (batch, rows, cols) window with strides (sb, ld, 1) at element `off` of a sentinel-filled (or NaN-filled) buffer."""

    def __init__(self, dt, batch, rows, cols, ld, sb, off=0, fill=SENTINEL):
        self.fill = fill
        self.buf = torch.full((off + max(batch, 1) * max(sb, rows * ld) + PAD,), fill, dtype=dt, device='cuda')
        self.view = torch.as_strided(self.buf, (batch, rows, cols), (sb, ld, 1), off)
        self.off = off

    @property
    def ptr(self):
        return _ptr(self.buf, self.off)

    def take(self):
        """The window's contents; the window is then refilled and the WHOLE buffer must be the fill value again."""
        got = self.view.clone()
        self.view.fill_(self.fill)
        return got, bool((self.buf == self.fill).all())


def _sx(x, n, D):
    return 0 if x.dim() == 2 else n * D


def _nu2(fam):
    return int(2 * FAMILIES[fam]['nu'])


def fwd_call(fam, dtn, D, batch, pd, n1, n2, K, ldk, sK, diag):
    """(symbol, [(argument name, value)]) of the family's forward entry point.  diag: the diag_add value, or for Gibbs a
    device scalar / None."""
    kind, S = fam_kind(fam), None
    if kind == 'gibbs':
        a = [('x1', _ptr(pd['x1'])), ('x2', _ptr(pd['x2'])), ('l1', _ptr(pd['l1'])), ('l2', _ptr(pd['l2'])), ('n1', n1),
             ('n2', n2), ('D', D), ('os', _ptr(pd.get('os'))), ('diag_add', _ptr(diag) if torch.is_tensor(diag) else None),
             ('K', K), ('ldk', ldk), ('stream', S)]
    elif kind == 'ard':
        a = [('x1', _ptr(pd['x1'])), ('x2', _ptr(pd['x2'])), ('ls', _ptr(pd['ls'])), ('os', _ptr(pd['os'])), ('batch', batch),
             ('n1', n1), ('n2', n2), ('D', D), ('sx1', _sx(pd['x1'], n1, D)), ('sx2', _sx(pd['x2'], n2, D))]
        if 'nu' in FAMILIES[fam]:
            a.append(('nu2', _nu2(fam)))
        a += [('diag_add', float(diag)), ('K', K), ('ldk', ldk), ('sK', sK), ('stream', S)]
    elif kind == 'rbf_periodic':
        a = [('x1', _ptr(pd['x1'])), ('x2', _ptr(pd['x2'])), ('lsr', _ptr(pd['lsr'])), ('lsp', _ptr(pd['lsp'])),
             ('per', _ptr(pd['per'])), ('os', _ptr(pd['os'])), ('batch', batch), ('n1', n1), ('n2', n2), ('D', D),
             ('sx1', _sx(pd['x1'], n1, D)), ('sx2', _sx(pd['x2'], n2, D)), ('diag_add', float(diag)), ('K', K), ('ldk', ldk),
             ('sK', sK), ('stream', S)]
    else:
        a = [('x1', _ptr(pd['x1'])), ('x2', _ptr(pd['x2'])), ('s1', _ptr(pd['s1'])), ('s2', _ptr(pd['s2'])), ('n1', n1),
             ('n2', n2), ('jitter', _jit(dtn)), ('K', K), ('ldk', ldk), ('stream', S)]
    return f'nsgp_{FAMILIES[fam]["stem"]}_build_fwd_{dtn}', a


def bwd_call(fam, dtn, D, batch, pd, n1, n2, G, ldg, sG, outs, ws, wsb):
    """(symbol, [(argument name, value)]) of the family's backward entry point; outs: {output name: pointer or None}."""
    sym, a = fwd_call(fam, dtn, D, batch, pd, n1, n2, None, 0, 0, 0.0)
    cut = {'gibbs': 'diag_add', 'ard': 'diag_add', 'rbf_periodic': 'diag_add', 'ps2d': 'K'}[fam_kind(fam)]
    a = a[:[k for k, _ in a].index(cut)]
    a += [('G', G), ('ldg', ldg)]
    if FAMILIES[fam]['batched']:
        a.append(('sG', sG))
    a += [('g_' + name, outs.get(name)) for name in C.outputs_of(fam, None)]
    a += [('ws', ws), ('ws_bytes', wsb), ('stream', None)]
    return sym.replace('_fwd_', '_bwd_'), a


def _jit(dtn):
    return float(torch.tensor(C.PS_JITTER, dtype=DTYPES[dtn]))


def _invoke(call):
    from nsgp import _lib
    sym, a = call
    return getattr(_lib.load(), sym)(*[v for _, v in a])


def ws_bytes(fam, dtn, D, batch, n1, n2):
    from nsgp import _lib
    lib, es = _lib.load(), 4 if dtn == 'f32' else 8
    kind = fam_kind(fam)
    if kind == 'gibbs':
        return lib.nsgp_gibbs_build_bwd_workspace(n1, n2, D, es)
    if kind == 'ps2d':
        return lib.nsgp_ps2d_build_bwd_workspace(n1, n2, es)
    return getattr(lib, f'nsgp_{FAMILIES[fam]["stem"]}_build_bwd_workspace')(batch, n1, n2, D, es)


# --------------------------------------------------------------------------------------------
# forward
# --------------------------------------------------------------------------------------------
def _fwd_diag(fam, da_on):
    return 0.0 if fam == 'ps2d' or not da_on else C.DIAG_ADD


def run_fwd_abi(fam, dtn, D, batch, pd, n1, n2, ldk, sK, off, diag, what):
    dt = DTYPES[dtn]
    win = Window(dt, batch, n1, n2, ldk, sK, off)
    if fam_kind(fam) == 'gibbs':
        diag = torch.full((1,), diag, dtype=dt, device='cuda') if diag else None
    rc = _invoke(fwd_call(fam, dtn, D, batch, pd, n1, n2, win.ptr, ldk, sK, diag))
    assert rc == 0, (what, rc)
    got, clean = win.take()
    assert clean, f'{what}: the build wrote outside its window (ldk {ldk}, sK {sK}, offset {off})'
    return got


def run_fwd_ops(ops, fam, dtn, pd, diag):
    kind, f = fam_kind(fam), FAMILIES[fam]
    if kind == 'gibbs':
        return ops.gibbs_build(pd['x1'], pd['x2'], pd['l1'], pd['l2'], outputscale=pd.get('os'),
                               diag_add=diag if diag else None)[None]
    if kind == 'ard':
        if 'nu' in f:
            return ops.matern_build(pd['x1'], pd['x2'], pd['ls'], pd['os'], f['nu'], diag_add=diag)
        return ops.rbf_build(pd['x1'], pd['x2'], pd['ls'], pd['os'], diag_add=diag)
    if kind == 'rbf_periodic':
        return ops.rbf_periodic_build(pd['x1'], pd['x2'], pd['lsr'], pd['lsp'], pd['per'], pd['os'], diag_add=diag)
    return ops.ps2d_build(pd['x1'], pd['x2'], pd['s1'], pd['s2'], jitter=_jit(dtn))[None]


@pytest.mark.parametrize('m', C.fwd_masters(), ids=lambda m: f'{m[0]}-{m[1]}-D{m[2]}-b{m[3]}-{"shared" if m[4] else "batched"}'
                         + ('' if m[5] else '-nodiag'))
def test_forward_master_matches_float64_and_every_row_equals_its_slice(ops, m):
    from conftest import measured
    fam, dtn, D, batch, shared, da_on = m
    n1m, n2m = C.FWD_N1_MAX, C.fwd_n2_max(dtn)
    p = C.make_inputs(fam, dtn, D, batch, n1m, n2m, shared)
    if fam == 'gibbs' and not da_on:
        p['os'] = None
    diag = _fwd_diag(fam, da_on)
    ref = C.ref_forward(fam, C._f64(p), diag, jitter=_jit(dtn))
    cpt = C.CPT[dtn]
    ldm = -(-n2m // cpt) * cpt + cpt
    master = run_fwd_abi(fam, dtn, D, batch, dev_inputs(p), n1m, n2m, ldm, (n1m + 1) * ldm, 0, diag, 'master')
    rtol, atol = C.fwd_tol(fam, dtn)
    assert measured(f'pairwise fwd {fam} {dtn} D={D} b={batch}', master, ref, rtol=rtol, atol=atol)
    wrong = []
    for n1, n2 in C.fwd_shapes(dtn):
        pd = dev_inputs(C.slice_inputs(fam, p, n1, n2))
        want = master[:, :n1, :n2]
        for layout in C.FWD_LAYOUTS:
            if layout == 'sk_odd' and not FAMILIES[fam]['batched']:
                continue
            if layout == 'contig':
                got = run_fwd_ops(ops, fam, dtn, pd, diag)
            else:
                ldk, sK, off = C.fwd_layout(layout, dtn, n1, n2)
                got = run_fwd_abi(fam, dtn, D, batch, pd, n1, n2, ldk, sK, off, diag, f'{n1}x{n2} {layout}')
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                wrong.append((n1, n2, layout, len(bad), bad[0].tolist()))
    assert not wrong, f'{len(wrong)} rows differ from their master slice; (n1, n2, layout, entries, first): {wrong[:8]}'


# --------------------------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------------------------
def out_shapes(fam, D, batch, n1, n2):
    kind = fam_kind(fam)
    if kind == 'gibbs':
        return {'l1': (D, n1), 'l2': (D, n2), 'x1': (n1, D), 'x2': (n2, D), 'os': (1,)}
    if kind == 'ard':
        return {'x1': (batch, n1, D), 'x2': (batch, n2, D), 'ls': (batch, D), 'os': (batch,)}
    if kind == 'rbf_periodic':
        return {'x1': (batch, n1, D), 'x2': (batch, n2, D), 'lsr': (batch, D), 'lsp': (batch,), 'per': (batch,), 'os': (batch,)}
    return {'s1': (n1, 4), 's2': (n2, 4)}


def standard(fam, name, t):
    """An output as stored -> the reference's layout: row / col (batch, n, K), glob (batch, K)."""
    kind = fam_kind(fam)
    if kind == 'gibbs':
        return t.T[None] if name in ('l1', 'l2') else t[None] if name in ('x1', 'x2') else t.reshape(1, 1)
    if kind == 'ps2d':
        return t[None]
    return t if t.dim() >= 2 else t[:, None]


TWIN = {'x2': 'x1', 'l2': 'l1', 's2': 's1'}


def run_bwd_abi(case, pd, Gwin, names, what):
    """One backward launch through the C ABI, the outputs in `names` non-NULL (same-buffer rows: the column-side twin shares the
    row-side buffer).  Returns {name: output as stored (device)}."""
    fam, dtn, dt = case.fam, case.dtn, DTYPES[case.dtn]
    shapes = out_shapes(fam, case.D, case.batch, case.n1, case.n2)
    wins = {}
    for name in names:
        if case.sym and name in TWIN:
            continue
        if fam_kind(fam) == 'rbf_periodic' and name == 'lsr' and pd['lsr'] is None:
            continue
        wins[name] = Window(dt, 1, 1, math.prod(shapes[name]), math.prod(shapes[name]), math.prod(shapes[name]), off=PAD)
    outs = {name: w.ptr for name, w in wins.items()}
    if case.sym:
        outs.update({b: outs[a] for b, a in TWIN.items() if a in outs and b in names})
    wsb = ws_bytes(fam, dtn, case.D, case.batch, case.n1, case.n2)
    ws = torch.full((WS_GUARD + wsb + WS_GUARD,), 0xA5, dtype=torch.uint8, device='cuda')     # guard | workspace | guard
    rc = _invoke(bwd_call(fam, dtn, case.D, case.batch, pd, case.n1, case.n2, Gwin.ptr, Gwin.view.stride(1),
                          Gwin.view.stride(0), outs, _ptr(ws, WS_GUARD), wsb))
    assert rc == 0, (what, rc)
    assert bool((ws[:WS_GUARD] == 0xA5).all()), f'{what}: the launch wrote in front of its workspace'
    assert bool((ws[WS_GUARD + wsb:] == 0xA5).all()), f'{what}: the launch wrote past its {wsb}-byte workspace'
    got = {}
    for name, w in wins.items():
        g, clean = w.take()
        assert clean, f'{what}: wrote outside the window of g_{name}'
        assert not bool(torch.isnan(g).any()), f'{what}: NaN in g_{name}'
        got[name] = g.reshape(shapes[name])
    return got


def run_bwd_ops(ops, case, pd, G):
    fam, f, kind = case.fam, FAMILIES[case.fam], fam_kind(case.fam)
    if kind == 'gibbs':
        r = ops.gibbs_build_bwd(pd['x1'], pd['x2'], pd['l1'], pd['l2'], pd['os'], G[0], need_x=True, need_os=True)
        return dict(zip(('l1', 'l2', 'x1', 'x2', 'os'), r))
    if kind == 'ard':
        if 'nu' in f:
            r = ops.matern_build_bwd(pd['x1'], pd['x2'], pd['ls'], pd['os'], f['nu'], G, sym=case.sym)
        else:
            r = ops.rbf_build_bwd(pd['x1'], pd['x2'], pd['ls'], pd['os'], G, sym=case.sym)
        r = dict(zip(('x1', 'x2', 'ls', 'os'), r))
        if case.sym:
            assert r['x2'] is r['x1']
            del r['x2']
        return r
    if kind == 'rbf_periodic':
        r = dict(zip(('x1', 'x2', 'lsr', 'lsp', 'per', 'os'),
                     ops.rbf_periodic_build_bwd(pd['x1'], pd['x2'], pd['lsr'], pd['lsp'], pd['per'], pd['os'], G)))
        return {k: v for k, v in r.items() if v is not None}
    return dict(zip(('s1', 's2'), ops.ps2d_build_bwd(pd['x1'], pd['x2'], pd['s1'], pd['s2'], _jit(case.dtn), G[0])))


def _g_window(case, G):
    ldg = case.n2 + case.ldg
    win = Window(DTYPES[case.dtn], case.batch, case.n1, case.n2, ldg, case.n1 * ldg + case.sg, fill=NAN)
    win.view.copy_(G.cuda())
    return win


@pytest.mark.parametrize('case', BWD_CASES, ids=lambda c: c.name)
def test_backward_row_is_within_its_rounding_bound_and_writes_nothing_else(ops, case):
    p, G = C.bwd_problem(case)
    ref = C.bwd_reference(case, p, G)
    pd = dev_inputs(p)
    Gwin = _g_window(case, G)
    names = C.outputs_of(case.fam, p)
    got = run_bwd_abi(case, pd, Gwin, names, case.name)
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    worst = 0.0
    for name, (val, bound) in ref.items():
        g = standard(case.fam, name, got[name]).double().cpu()
        assert g.shape == val.shape, (name, g.shape, val.shape)
        ratio = (g - val).abs() / bound.clamp_min(1e-300)
        r = float(ratio.max())
        worst = max(worst, r)
        assert r <= 1.0, f'{case.name} g_{name}: |err| / bound = {r:.3g} at {tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])}'
    print(f'[measured] pairwise bwd {case.name} plan {case.plan}: worst |err| / bound = {worst:.3g}')
    # the wrapper's launch of the same row: the same bits
    wrapper_can = not case.ldg and not case.sg and not (case.sym and fam_kind(case.fam) != 'ard')
    if wrapper_can:
        via_ops = run_bwd_ops(ops, case, pd, Gwin.view)
        for name, g in got.items():
            assert torch.equal(via_ops[name].reshape(g.shape), g), f'{case.name}: nsgp.ops and the C ABI differ in g_{name}'
    if case.nulls:
        for k in range(len(names)):
            for sub in itertools.combinations(names, k):
                part = run_bwd_abi(case, pd, Gwin, list(sub), f'{case.name} outputs {sub}')
                for name, g in part.items():
                    assert torch.equal(g, got[name]), f'{case.name}: g_{name} with outputs {sub} differs from the all-outputs run'


# --------------------------------------------------------------------------------------------
# error codes and empty problems
# --------------------------------------------------------------------------------------------
BAD = {   # kind -> direction -> [(argument, bad value, return code)]
    'gibbs': {'fwd': [('x1', None, -1), ('x2', None, -2), ('l1', None, -3), ('l2', None, -4), ('n1', -1, -5), ('n2', -1, -6),
                      ('D', 0, -7), ('D', 9, -7), ('K', None, -10), ('ldk', 'short', -11)],
              'bwd': [('x1', None, -1), ('x2', None, -2), ('l1', None, -3), ('l2', None, -4), ('n1', -1, -5), ('n2', -1, -6),
                      ('D', 0, -7), ('D', 9, -7), ('G', None, -9), ('ldg', 'short', -10), ('ws', None, -100),
                      ('ws_bytes', 'short', -100)]},
    'rbf': {'fwd': [('x1', None, -1), ('x2', None, -2), ('ls', None, -3), ('os', None, -4), ('batch', -1, -5), ('n1', -1, -6),
                    ('n2', -1, -7), ('D', 0, -8), ('D', 9, -8), ('K', None, -12), ('ldk', 'short', -13)],
            'bwd': [('x1', None, -1), ('x2', None, -2), ('ls', None, -3), ('os', None, -4), ('batch', -1, -5), ('n1', -1, -6),
                    ('n2', -1, -7), ('D', 0, -8), ('D', 9, -8), ('G', None, -11), ('ldg', 'short', -12), ('ws', None, -100),
                    ('ws_bytes', 'short', -100)]},
    'matern': {'fwd': [('x1', None, -1), ('x2', None, -2), ('ls', None, -3), ('os', None, -4), ('batch', -1, -5),
                       ('n1', -1, -6), ('n2', -1, -7), ('D', 0, -8), ('D', 9, -8), ('nu2', 2, -11), ('K', None, -13),
                       ('ldk', 'short', -14)],
               'bwd': [('x1', None, -1), ('x2', None, -2), ('ls', None, -3), ('os', None, -4), ('batch', -1, -5),
                       ('n1', -1, -6), ('n2', -1, -7), ('D', 0, -8), ('D', 9, -8), ('nu2', 4, -11), ('G', None, -12),
                       ('ldg', 'short', -13), ('ws', None, -100), ('ws_bytes', 'short', -100)]},
    'rbf_periodic': {'fwd': [('x1', None, -1), ('x2', None, -2), ('lsp', None, -4), ('per', None, -5), ('batch', -1, -7),
                             ('n1', -1, -8), ('n2', -1, -9), ('D', 0, -10), ('D', 9, -10), ('K', None, -14),
                             ('ldk', 'short', -15)],
                     'bwd': [('x1', None, -1), ('x2', None, -2), ('lsp', None, -4), ('per', None, -5), ('batch', -1, -7),
                             ('n1', -1, -8), ('n2', -1, -9), ('D', 0, -10), ('D', 9, -10), ('G', None, -13),
                             ('ldg', 'short', -14), ('ws', None, -100), ('ws_bytes', 'short', -100)]},
    'ps2d': {'fwd': [('x1', None, -1), ('x2', None, -2), ('s1', None, -3), ('s2', None, -4), ('n1', -1, -5), ('n2', -1, -6),
                     ('K', None, -8), ('ldk', 'short', -9)],
             'bwd': [('x1', None, -1), ('x2', None, -2), ('s1', None, -3), ('s2', None, -4), ('n1', -1, -5), ('n2', -1, -6),
                     ('G', None, -8), ('ldg', 'short', -9), ('ws', None, -100), ('ws_bytes', 'short', -100)]},
}
EMPTY = [('n1', 0), ('n2', 0), ('batch', 0)]


@pytest.mark.parametrize('fam', ['gibbs', 'rbf', 'matern32', 'rbfper', 'ps2d'])
@pytest.mark.parametrize('dtn', list(DTYPES))
def test_bad_arguments_and_empty_problems_leave_every_buffer_untouched(ops, fam, dtn):
    dt = DTYPES[dtn]
    D, batch, n1, n2 = 2, 2 if FAMILIES[fam]['batched'] else 1, 9, 7
    pd = dev_inputs(C.make_inputs(fam, dtn, D, batch, n1, n2, False if FAMILIES[fam]['batched'] else True))
    shapes = out_shapes(fam, D, batch, n1, n2)
    Kwin = Window(dt, batch, n1, n2, n2, n1 * n2, off=PAD)
    Gwin = Window(dt, batch, n1, n2, n2, n1 * n2, off=PAD, fill=1.0)
    wins = {name: Window(dt, 1, 1, math.prod(s), math.prod(s), math.prod(s), off=PAD) for name, s in shapes.items()}
    wsb = ws_bytes(fam, dtn, D, batch, n1, n2)
    ws = torch.full((WS_GUARD + wsb + WS_GUARD,), 0xA5, dtype=torch.uint8, device='cuda')     # guard | workspace | guard
    diag = torch.full((1,), 0.5, dtype=dt, device='cuda') if fam == 'gibbs' else 0.5
    calls = {'fwd': fwd_call(fam, dtn, D, batch, pd, n1, n2, Kwin.ptr, n2, n1 * n2, diag),
             'bwd': bwd_call(fam, dtn, D, batch, pd, n1, n2, Gwin.ptr, n2, n1 * n2, {k: w.ptr for k, w in wins.items()},
                             _ptr(ws, WS_GUARD), wsb)}
    stem = FAMILIES[fam]['stem']
    short = {'ldk': n2 - 1, 'ldg': n2 - 1, 'ws_bytes': 8}
    for direction, (sym, args) in calls.items():
        names = [k for k, _ in args]
        trials = [(a, short.get(a, v) if v == 'short' else v, rc) for a, v, rc in BAD[stem][direction]]
        trials += [(a, v, 0) for a, v in EMPTY if a in names]
        for arg, val, want in trials:
            rc = _invoke((sym, [(k, val if k == arg else v) for k, v in args]))
            assert rc == want, (sym, arg, val, rc, want)
    torch.cuda.synchronize()
    for name, w in list(wins.items()) + [('K', Kwin)]:
        assert bool((w.buf == SENTINEL).all()), f'{fam} {dtn}: a rejected or empty call wrote to {name}'
    assert bool((ws == 0xA5).all()), f'{fam} {dtn}: a rejected or empty call wrote to the workspace'
