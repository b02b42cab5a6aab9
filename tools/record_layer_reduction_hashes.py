"""Record sha256 digests of what the SVGP layer's reductions (the layer half of csrc/svgp.hip) write.

    python tools/record_layer_reduction_hashes.py --out tests/golden/layer_reduction_hashes.json
    python tools/record_layer_reduction_hashes.py --compare tests/golden/layer_reduction_hashes.json

The column statistics, their finalize forms, the row dots of the adjoint, sampling and the mean-field `diag_*` kernels are
fixed-order reductions and element-wise passes, so a change of the file's structure can and must leave every output bit where
it was.  tests/test_gpu_svgp_reductions.py holds them on small-integer data, which is exact in any summation order; this
tool runs the same tables (and DIAG_CASES) of tests/test_svgp_reduction_cases_cpu.py on seeded REAL values.  It drives the C
entry points directly (ctypes; NSGP_LIB selects the library, so the same file runs against the library of the commit to be
preserved and against the one under test), in both dtypes, and takes the sha256 of the raw bytes of every output:
    rowdot_affine   rowdot_affine                                       out, out_gv, out_1, out_x (an absent one stays NaN)
    rowdot          rowdot                                              out
    colstats        svgp_colstats, svgp_colstats_bwd                    mean, var, Abar, C2, mbar
    finalize        colstats_finalize / _affine / _affine_p64_f32       mean, var
    sample          dgp_sample_fwd / _bwd                               h, gmean, gvar
    diag            svgp_diag_colsq, svgp_diag_bwd                      part_q (not where gmean alone is offset), Abar, mbar, tbar
    diag_fin        colstats_finalize_diag                              mean, var
Every output and workspace is a window of exactly the size the entry point needs, filled with NaN, inside a buffer of guard
words: an element a kernel should have written and did not shows in the digest, and one it should not have written shows in
the guards.

--out runs every case TWICE and refuses to write unless both runs agree, no guard word moved and every value is within the
bound of tests/test_svgp_reduction_cases_cpu.py of the float64 reference: `red_tol`, (N + c) u sum |t_i| with the sum of the
absolute terms taken in float64, for a sum of N terms, and c u |pieces| for an element-wise output (c is counted beside each
use).  The record is of right answers.  tests/test_gpu_layer_reduction_bits.py recomputes the digests on the code under test
and requires equality case by case.
"""
import argparse
import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_svgp_reduction_cases_cpu as RC      # noqa: E402

GUARD = -7.0
PAD = 64                                                  # guard elements on either side (a multiple of 16 bytes)
CASES, case_id = RC.LAYER_BITS_CASES, RC.layer_bits_id


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Buffers:
    """Outputs and workspaces: NaN windows inside guard words."""

    def __init__(self, dtype):
        self.dtype, self.items = dtype, []

    def new(self, *shape, dtype=None):
        import torch
        numel = math.prod(shape)
        buf = torch.full((numel + 2 * PAD,), GUARD, dtype=dtype or self.dtype, device='cuda')
        buf[PAD:PAD + numel] = float('nan')
        self.items.append((buf, numel))
        return buf[PAD:PAD + numel].view(shape)

    def guards_intact(self):
        return all(bool((b[:PAD] == GUARD).all()) and bool((b[PAD + n:] == GUARD).all()) for b, n in self.items)


def inputs(run):
    """The case's operands: float64 CPU tensors, seeded by the case."""
    kind, c, dt = run
    if kind == 'rowdot_affine':
        return RC.rowdot_real_inputs(c.n, c.batch, c.M, c.D, 'affine')
    if kind == 'rowdot':
        return RC.rowdot_real_inputs(c[0], 2, 3, 1, 'plain')
    return {'colstats': RC.colstats_real_inputs, 'finalize': RC.finalize_real_inputs, 'sample': RC.sample_real_inputs,
            'diag': RC.diag_inputs, 'diag_fin': RC.diag_fin_inputs}[kind](c)


def run_case(run):
    """One pass over the case's entry points -> (digests {output name: sha256}, outputs {name: tensor, 'guards': bool})."""
    import torch
    from nsgp import _lib, ops
    kind, c, dt = run
    tdt, f64 = RC.DTYPES[dt], torch.float64
    B, st, p = Buffers(tdt), ops._stream(), ops._p
    P = inputs(run)

    def dev(t, off=0, dtype=tdt):
        if t is None:
            return None
        td = t.to(dtype).contiguous()
        if not off:
            return td.cuda()
        buf = torch.zeros(td.numel() + off + 3, dtype=dtype, device='cuda')
        view = buf[off:off + td.numel()].view(td.shape)
        view.copy_(td)
        assert view.data_ptr() % 16 != 0
        return view

    def call(name, *args):
        _lib.call(f'nsgp_{name}', *args)

    out = {}
    if kind == 'rowdot_affine':
        n, batch, M, D, shared, drop, off = c
        A, g, gv, x = dev(P['A'], int(off == 'A')), dev(P['g'], int(off == 'g')), dev(P['gv'], int(off == 'gv')), dev(P['x'])
        nb = 1 if shared else batch
        out = dict(out=B.new(batch, M), out_gv=B.new(batch), out_1=B.new(nb), out_x=B.new(nb, D))
        call(f'rowdot_affine_{dt}', p(A), p(g), None if drop == 'gv' else p(gv), None if drop == 'out_x' else p(x), n * D, D,
             shared, batch, M, n, p(out['out']), p(out['out_gv']), None if drop == 'out_x' else p(out['out_x']),
             None if drop == 'out_1' else p(out['out_1']), st)
    elif kind == 'rowdot':
        n, off = c
        A, g = dev(P['A'], int(off == 'A')), dev(P['g'], int(off == 'g'))
        out = dict(out=B.new(2, 3))
        call(f'rowdot_{dt}', p(A), p(g), 2, 3, n, p(out['out']), st)
    elif kind == 'colstats':
        M, n, b = c
        D = {k: dev(t) for k, t in P.items()}
        out = dict(mean=B.new(b, n), var=B.new(b, n), Abar=B.new(b, M, n), C2=B.new(b, M, n), mbar=B.new(b, M))
        call(f'svgp_colstats_{dt}', p(D['A']), p(D['C']), p(D['m']), p(D['base']), b, M, n, p(out['mean']), p(out['var']), st)
        call(f'svgp_colstats_bwd_{dt}', p(D['A']), p(D['C']), p(D['m']), p(D['gmean']), p(D['gvar']), b, M, n, p(out['Abar']),
             p(out['C2']), p(out['mbar']), st)
    elif kind == 'finalize':
        b, D, n = RC.FIN_BATCH, RC.FIN_D, c.n
        parts = [dev(P[k], dtype=f64 if c.form == 'p64' else tdt) for k in ('pdot', 'psqA', 'psqC')]
        base, x, w, cc = dev(P['base']), dev(P['x']), dev(P['w']), dev(P['c'])
        out = dict(mean=B.new(b, n), var=B.new(b, n))
        if c.form == 'plain':
            call(f'svgp_colstats_finalize_{dt}', *[p(t) for t in parts], p(base), b, c.tiles, n, p(out['mean']), p(out['var']), st)
        else:
            call('svgp_colstats_finalize_affine_' + ('p64_f32' if c.form == 'p64' else dt), *[p(t) for t in parts], p(base),
                 RC.FIN_BASE_ADD, b, c.tiles, n, p(x), n * D, D, p(w), 0 if c.shared else D, p(cc), 0 if c.shared else 1,
                 p(out['mean']), p(out['var']), st)
    elif kind == 'sample':
        S, n, b, ns = c
        D = {k: dev(t) for k, t in P.items()}
        out = dict(h=B.new(S, n, b), gmean=B.new(b, ns, n), gvar=B.new(b, ns, n))
        call(f'dgp_sample_fwd_{dt}', p(D['mean']), p(D['var']), p(D['eps']), S, ns, n, b, p(out['h']), st)
        call(f'dgp_sample_bwd_{dt}', p(D['var']), p(D['eps']), p(D['gh']), S, ns, n, b, p(out['gmean']), p(out['gvar']), st)
    elif kind == 'diag':
        b, M, n = RC.DIAG_BATCH, c.M, c.n
        lib = _lib.load()
        A, s2m1, m = dev(P['A'], int(c.off == 'A')), dev(P['s2m1']), dev(P['m'])
        gmean, gvar = dev(P['gmean'], int(c.off == 'gmean')), dev(P['gvar'])
        T = int(lib.nsgp_svgp_diag_tiles(M)) + c.extra
        assert T == RC.diag_tiles(M) + c.extra
        if c.off != 'gmean':                              # (the forward pass reads no gmean)
            out['part_q'] = B.new(b, T, n, dtype=f64)
            call(f'svgp_diag_colsq_{dt}', p(A), p(s2m1), b, M, n, p(out['part_q']), T, st)
        wsb = int(lib.nsgp_svgp_diag_bwd_workspace(b, M, n))
        assert wsb == b * M * RC.cdiv(n, RC.DIAG_BWD_COLS) * 16
        ws = B.new(wsb // 8, dtype=f64)
        out.update(Abar=B.new(b, M, n), mbar=B.new(b, M), tbar=B.new(b, M))
        call(f'svgp_diag_bwd_{dt}', p(A), p(m), p(s2m1), p(gmean), p(gvar), b, M, n, p(out['Abar']), p(out['mbar']),
             p(out['tbar']), p(ws), wsb, st)
    else:
        b, D, n = RC.FIN_BATCH, RC.FIN_D, c.n
        pdot, pq, base, x, w, cc = dev(P['pdot']), dev(P['pq'], dtype=f64), dev(P['base']), dev(P['x']), dev(P['w']), dev(P['c'])
        out = dict(mean=B.new(b, n), var=B.new(b, n))
        call(f'svgp_colstats_finalize_diag_{dt}', p(pdot), c.tiles, p(pq), c.qtiles, p(base), RC.FIN_BASE_ADD, b, n, p(x),
             n * D, D, p(w), 0 if c.shared else D, p(cc), 0 if c.shared else 1, p(out['mean']), p(out['var']), st)
    torch.cuda.synchronize()
    dig = {k: sha(t) for k, t in out.items()}
    out['guards'] = B.guards_intact()
    return dig, out


def check(run, out):
    """Reasons why the case's results are not right answers (empty: they are).  Every bound is `red_tol` on the sum of the
    absolute terms of the float64 reference, or c u |pieces| element-wise (red_tol with N = 0)."""
    import torch
    kind, c, dt = run
    why = [] if out['guards'] else ['a guard word was overwritten']
    P = inputs(run)
    ab = {k: (v.abs() if torch.is_tensor(v) else v) for k, v in P.items()}

    def within(name, ref, tol, absent=False):
        got = out[name].double().cpu().reshape(-1)
        if absent:
            if not bool(torch.isnan(got).all()):
                why.append(f'{name} is absent and was written')
            return
        ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
        tol = torch.as_tensor(tol, dtype=torch.float64).reshape(-1).expand_as(ref)
        if got.shape != ref.shape or not bool(((got - ref).abs() <= tol).all()):      # (a NaN fails the comparison)
            why.append(f'{name}: off by {float((got - ref).abs().max()):.3g}, bound {float(tol.max()):.3g}')

    def affine_mean(Q, b):
        """sum_d x w + c of the finalize forms, on Q = P or its absolute values."""
        mu = torch.zeros(b, Q['x'].shape[1], dtype=torch.float64)
        if Q['w'] is not None:
            mu = mu + torch.einsum('bnd,bd->bn', Q['x'], Q['w'].expand(b, -1))
        if Q['c'] is not None:
            mu = mu + Q['c'].expand(b).unsqueeze(1)
        return mu

    if kind in ('rowdot_affine', 'rowdot'):
        if kind == 'rowdot':
            n, batch, D, shared, drop = c[0], 2, 1, 0, None
        else:
            n, batch, D, shared, drop = c.n, c.batch, c.D, c.shared, c.drop
        R, Ra = RC.rowdot_reference(P, shared), RC.rowdot_reference(ab, shared)
        nsum = n * (batch if shared else 1)
        # a product and n - 1 additions per row (c = 1); the plain sums hold no product
        within('out', R['out'], RC.red_tol(n, 1, dt, Ra['out']))
        if kind == 'rowdot_affine':
            within('out_gv', R['out_gv'], RC.red_tol(n, 0, dt, Ra['out_gv']), drop == 'gv')
            within('out_1', R['out_1'], RC.red_tol(nsum, 0, dt, Ra['out_1']), drop == 'out_1')
            within('out_x', R['out_x'], RC.red_tol(nsum, 1, dt, Ra['out_x']), drop == 'out_x')
    elif kind == 'colstats':
        M, n, b = c
        R = RC.colstats_reference(P)
        g2 = 2.0 * ab['gvar'].unsqueeze(1)
        within('mean', R['mean'], RC.red_tol(M, 1, dt, torch.einsum('bmn,bm->bn', ab['A'], ab['m'])))
        # base and 2 M squares, each one rounding
        within('var', R['var'], RC.red_tol(2 * M + 1, 1, dt, ab['base'].unsqueeze(1) + (P['C'] ** 2 + P['A'] ** 2).sum(1)))
        # Abar = m g1 - (2 gv) a: two products and the difference; C2 = (2 gv) c: one product
        within('Abar', R['Abar'], RC.red_tol(0, 3, dt, ab['m'].unsqueeze(2) * ab['gmean'].unsqueeze(1) + g2 * ab['A']))
        within('C2', R['C2'], RC.red_tol(0, 1, dt, g2 * ab['C']))
        within('mbar', R['mbar'], RC.red_tol(n, 1, dt, torch.einsum('bmn,bn->bm', ab['A'], ab['gmean'])))
    elif kind == 'finalize':
        mean, var = RC.finalize_reference(c, P)
        base_add = 0.0 if c.form == 'plain' else RC.FIN_BASE_ADD
        D = RC.FIN_D if c.has_w else 0
        # mean: tiles partials, D products, c; var: base, base_add, 2 tiles partials; p64 rounds its float64 sum once more
        within('mean', mean, RC.red_tol(c.tiles + D + 1, 2, dt, ab['pdot'].sum(1) + affine_mean(ab, RC.FIN_BATCH)))
        within('var', var, RC.red_tol(2 * c.tiles + 2, 1, dt, ab['base'].unsqueeze(1) + base_add + ab['psqC'].sum(1) + ab['psqA'].sum(1)))
    elif kind == 'sample':
        S, n, b, ns = c
        R = RC.sample_reference(P, ns)
        Ra = RC.sample_reference(dict(P, gh=ab['gh'], eps=ab['eps']), ns)
        # as tests/test_gpu_svgp_reductions.py::test_sampling_forward_and_backward; gmean is a sum of S terms or a copy
        within('h', R['h'], RC.red_tol(0, 3, dt, R['h_mag']))
        within('gmean', R['gmean'], RC.red_tol(S if ns == 1 else 1, 0, dt, Ra['gmean']))
        within('gvar', R['gvar'], RC.red_tol(S if ns == 1 else 1, 4, dt, R['gvar_abs']))
    elif kind == 'diag':
        b, M, n = RC.DIAG_BATCH, c.M, c.n
        A, s, m, g1, g2 = P['A'], P['s2m1'].unsqueeze(2), P['m'].unsqueeze(2), P['gmean'].unsqueeze(1), P['gvar'].unsqueeze(1)
        if 'part_q' in out:
            T = RC.diag_tiles(M) + c.extra
            term = torch.zeros(b, T * RC.DIAG_ROWS, n, dtype=torch.float64)
            term[:, :M] = s * A * A
            tiles = term.reshape(b, T, RC.DIAG_ROWS, n)
            # float64 whatever A's type: (s a) a + acc, two roundings a term; a tile row past M is exactly 0
            within('part_q', tiles.sum(2), RC.red_tol(RC.DIAG_ROWS, 2, 'f64', tiles.abs().sum(2)))
        # Abar = m g1 + (2 s) (a g2): three products and the sum
        within('Abar', m * g1 + 2.0 * s * A * g2, RC.red_tol(0, 4, dt, (m * g1).abs() + (2.0 * s * A * g2).abs()))
        # mbar, tbar: n terms of one / two products, and the rounding of the float64 total to the layer's type
        within('mbar', (A * g1).sum(2), RC.red_tol(n, 2, dt, (A * g1).abs().sum(2)))
        within('tbar', (A * A * g2).sum(2), RC.red_tol(n, 3, dt, (A * A * g2).abs().sum(2)))
    else:
        b = RC.FIN_BATCH
        D = RC.FIN_D if c.has_w else 0
        within('mean', P['pdot'].sum(1) + affine_mean(P, b), RC.red_tol(c.tiles + D + 1, 1, dt, ab['pdot'].sum(1) + affine_mean(ab, b)))
        # base, base_add and qtiles partials in float64, rounded once to the layer's type
        within('var', (P['base'].unsqueeze(1) + RC.FIN_BASE_ADD) + P['pq'].sum(1),
               RC.red_tol(c.qtiles + 2, 1, dt, ab['base'].unsqueeze(1) + RC.FIN_BASE_ADD + ab['pq'].sum(1)))
    return why


def record(cases=CASES, checked=False):
    """({case id: digests}, {case id: reasons} of the cases whose results failed `check`)."""
    digests, wrong = {}, {}
    for run in cases:
        dig, out = run_case(run)
        digests[case_id(run)] = dig
        if checked or not out['guards']:
            why = check(run, out) if checked else ['a guard word was overwritten']
            if why:
                wrong[case_id(run)] = why
    return digests, wrong


def write_record(path, digests):
    with open(path, 'w') as f:
        f.write('{"cases": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in digests.items()) + '\n}}\n')


def differing(ref, got):
    return {k: sorted(name for name in set(ref.get(k, {})) | set(got.get(k, {})) if ref.get(k, {}).get(name) != got.get(k, {}).get(name))
            for k in sorted(set(ref) | set(got)) if ref.get(k) != got.get(k)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='write the digests (JSON) here')
    ap.add_argument('--compare', metavar='FILE', help='recompute and compare with a record; exit status 1 if any case differs')
    a = ap.parse_args()
    got, wrong = record(checked=bool(a.out))
    print(f'{len(got)} cases, {sum(len(v) for v in got.values())} digests')
    if a.out:
        again, _ = record()
        unstable = differing(got, again)
        for k, v in list(wrong.items()) + list(unstable.items()):
            print(f'  {k}: {v}')
        if wrong or unstable:
            print(f'NOT written: {len(wrong)} cases with wrong results, {len(unstable)} that differ between two runs')
            sys.exit(2)
        write_record(a.out, got)
        print(f'two runs agree, every result within tolerance, no guard word moved: wrote {a.out}')
    if a.compare:
        with open(a.compare) as f:
            ref = json.load(f)['cases']
        diff = differing(ref, got)
        print(f'{len(diff)} of {len(ref)} recorded cases differ' + ''.join(f'\n  {k}: {v}' for k, v in diff.items()))
        sys.exit(1 if diff or wrong else 0)


if __name__ == '__main__':
    main()
