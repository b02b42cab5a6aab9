"""Record sha256 digests of what the DSVI objective's entry points (csrc/svgp.hip) write.

    python tools/record_objective_hashes.py --out tests/golden/objective_hashes.json
    python tools/record_objective_hashes.py --compare tests/golden/objective_hashes.json

The objective's terms are fixed-order reductions and element-wise adjoints, so a change of the file's structure can and must
leave every output bit where it was.  This tool drives the C entry points directly (ctypes; NSGP_LIB selects the library, so
the same file runs against the library of the commit to be preserved and against the one under test) on the seeded
'bound'-mode inputs of tests/test_svgp_reduction_cases_cpu.py, in both dtypes, and takes the sha256 of the raw bytes of
every output:
    gauss   gauss_ell_fwd / _bwd with GAUSS_GOUT              vec_out, vec_gmu, vec_gv, vec_gnoise
            gauss_ell_total_fwd / _bwd with GAUSS_UP          total_out, total_gmu, total_gv, total_gnoise
    kl      kl_whitened_fwd / _bwd                            out, gm, gLq
            kl_whitened_total_acc_fwd without / with addin    total_out, total_out_addin
            kl_whitened_total_bwd                             total_gm, total_gLq
    obj     dsvi_objective_fwd / _bwd                         out, gmu, gv, gnoise (where the case asks), gm<g>, gLq<g>
    mfkl    kl_meanfield_total_acc_fwd without / with addin   out, out_addin
            kl_meanfield_total_bwd                            gm, gs2
The KL inputs are the cases' L_given (NaN above the diagonal: never read).  Every output and workspace is a window of
exactly the size the entry point needs, filled with NaN, inside a buffer of guard words: an element a kernel should have
written and did not shows in the digest, and one it should not have written shows in the guards.

--out runs every case TWICE and refuses to write unless both runs agree, every value meets the tolerance the GPU tests
apply to it (tests/test_gpu_svgp_reductions.py: `red_tol` and the element-wise bounds against the float64 reference;
mean-field KL: the tolerance of tests/test_gpu_meanfield.py::test_mean_field_kl_matches_oracle_and_accumulates) and no guard
word moved: the record is of right answers.  tests/test_gpu_objective_bits.py recomputes the digests on the code under
test and requires equality case by case.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_svgp_reduction_cases_cpu as RC      # noqa: E402

GUARD = -7.0
PAD = 64                                                  # guard elements on either side (a multiple of 16 bytes)
CASES, case_id = RC.OBJECTIVE_BITS_CASES, RC.objective_bits_id


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class Buffers:
    """Outputs and workspaces: NaN windows inside guard words."""

    def __init__(self, dtype):
        self.dtype, self.items = dtype, []

    def new(self, *shape):
        import math
        import torch
        numel = math.prod(shape)
        buf = torch.full((numel + 2 * PAD,), GUARD, dtype=self.dtype, device='cuda')
        buf[PAD:PAD + numel] = float('nan')
        self.items.append((buf, numel))
        return buf[PAD:PAD + numel].view(shape)

    def guards_intact(self):
        return all(bool((b[:PAD] == GUARD).all()) and bool((b[PAD + n:] == GUARD).all()) for b, n in self.items)


def run_case(run):
    """One pass over the case's entry points -> (digests {output name: sha256}, outputs {name: tensor, 'guards': bool})."""
    import torch
    from nsgp import _lib, ops
    kind, c, dt = run
    tdt, es = RC.DTYPES[dt], 4 if dt == 'f32' else 8
    B, st, p = Buffers(tdt), ops._stream(), ops._p
    dev = lambda t: torch.as_tensor(t, dtype=torch.float64).to(tdt).contiguous().cuda()       # noqa: E731
    one = lambda x: torch.tensor([x], dtype=tdt, device='cuda')                               # noqa: E731
    out = {}

    def call(name, *args):
        _lib.call(f'nsgp_{name}_{dt}', *args)

    if kind == 'gauss':
        n, S = c
        P = RC.gauss_inputs(c, 'bound')
        y, mu, v, noise = dev(P['y']), dev(P['mu']), dev(P['v']), one(P['noise'])
        nparts = S * RC.gauss_blocks(n)
        for form, sfx, gout, nout in (('vec', '', dev(P['gout']), S), ('total', '_total', one(P['up']), 1)):
            o, ws = B.new(nout), B.new(nparts)
            call(f'gauss_ell{sfx}_fwd', p(y), p(mu), p(v), p(noise), S, n, P['scale'], p(o), p(ws), nparts * es, st)
            gmu, gv, gn, ws2 = B.new(S, n), B.new(S, n), B.new(1), B.new(nparts + 1)
            call(f'gauss_ell{sfx}_bwd', p(y), p(mu), p(v), p(noise), S, n, P['scale'], p(gout), p(gmu), p(gv), p(gn), p(ws2),
                 (nparts + 1) * es, st)
            out.update({f'{form}_out': o, f'{form}_gmu': gmu, f'{form}_gv': gv, f'{form}_gnoise': gn})
    elif kind == 'kl':
        M, batch = c
        P = RC.kl_inputs(c, 'bound')
        m, L, nparts = dev(P['m']), dev(P['L_given']), batch * RC.kl_blocks(M)
        o, ws, gm, gL = B.new(batch), B.new(nparts), B.new(batch, M), B.new(batch, M, M)
        call('kl_whitened_fwd', p(m), p(L), batch, M, p(o), p(ws), nparts * es, st)
        call('kl_whitened_bwd', p(m), p(L), batch, M, P['up'], p(gm), p(gL), st)
        out.update(out=o, gm=gm, gLq=gL)
        for name, addin in (('total_out', None), ('total_out_addin', one(P['addin']))):
            o, ws = B.new(1), B.new(nparts)
            call('kl_whitened_total_acc_fwd', p(m), p(L), batch, M, P['scale'], p(addin), p(o), p(ws), nparts * es, st)
            out[name] = o
        gm, gL = B.new(batch, M), B.new(batch, M, M)
        call('kl_whitened_total_bwd', p(m), p(L), batch, M, P['scale'], p(one(P['up'])), p(gm), p(gL), st)
        out.update(total_gm=gm, total_gLq=gL)
    elif kind == 'obj':
        P = RC.obj_inputs(c)
        n, S, M, ng = c.n, c.S, c.M, len(c.batches)
        y, mu, v, noise = dev(P['y']), dev(P['mu']), dev(P['v']), one(P['noise'])
        ms, Ls = [dev(m) for m, _, _ in P['groups']], [dev(Lg) for _, _, Lg in P['groups']]
        ptrs = lambda ts: (ctypes.c_void_p * ng)(*[t.data_ptr() for t in ts])                 # noqa: E731
        nb = (ctypes.c_int64 * ng)(*c.batches)
        lib = _lib.load()
        wsb = int(lib.nsgp_dsvi_objective_workspace(S, n, M, sum(c.batches), es))
        o, ws = B.new(1), B.new(wsb // es)
        call('dsvi_objective_fwd', p(y), p(mu), p(v), p(noise), S, n, P['ell_scale'], ng, ptrs(ms), ptrs(Ls), nb, M,
             P['kl_scale'], p(o), p(ws), wsb, st)
        wsb = int(lib.nsgp_dsvi_objective_workspace(S, n, 0, 0, es))
        gmu, gv, gn, ws2 = B.new(S, n), B.new(S, n), (B.new(1) if c.noise_grad else None), B.new(wsb // es)
        gms, gLs = [B.new(*m.shape) for m in ms], [B.new(*L.shape) for L in Ls]
        call('dsvi_objective_bwd', p(y), p(mu), p(v), p(noise), S, n, P['ell_scale'], ng, ptrs(ms), ptrs(Ls), nb, M,
             P['kl_scale'], p(one(c.up)), p(gmu), p(gv), p(gn), ptrs(gms), ptrs(gLs), p(ws2), wsb, st)
        out.update(out=o, gmu=gmu, gv=gv)
        if c.noise_grad:
            out['gnoise'] = gn
        for g in range(ng):
            out.update({f'gm{g}': gms[g], f'gLq{g}': gLs[g]})
    else:
        batch, M = c
        P = RC.mf_kl_inputs(c)
        m, s2, nparts = dev(P['m']), dev(P['s2']), RC.kl_diag_blocks(batch * M)
        for name, addin in (('out', None), ('out_addin', one(P['addin']))):
            o, ws = B.new(1), B.new(nparts)
            call('kl_meanfield_total_acc_fwd', p(m), p(s2), batch, M, P['scale'], p(addin), p(o), p(ws), nparts * es, st)
            out[name] = o
        gm, gs2 = B.new(batch, M), B.new(batch, M)
        call('kl_meanfield_total_bwd', p(m), p(s2), batch, M, P['scale'], p(one(P['up'])), p(gm), p(gs2), st)
        out.update(gm=gm, gs2=gs2)
    torch.cuda.synchronize()
    dig = {k: sha(t) for k, t in out.items()}
    out['guards'] = B.guards_intact()
    return dig, out


def check(run, out):
    """Reasons why the case's results are not right answers (empty: they are): the bounds of tests/test_gpu_svgp_reductions.py
    and, for the mean-field KL, of tests/test_gpu_meanfield.py."""
    import torch
    kind, c, dt = run
    u, why = RC.U[dt], []
    if not out['guards']:
        why.append('a guard word was overwritten')

    def within(name, ref, tol):
        got = out[name].double().cpu().reshape(-1)
        ref = torch.as_tensor(ref, dtype=torch.float64).reshape(-1)
        tol = torch.as_tensor(tol, dtype=torch.float64).reshape(-1).expand_as(ref)
        if got.shape != ref.shape or not bool(((got - ref).abs() <= tol).all()):      # (a NaN fails the comparison)
            why.append(f'{name}: off by {float((got - ref).abs().max()):.3g}, bound {float(tol.max()):.3g}')

    def kl_grads(tag, m, L, go, c_m, c_l):
        rm, rl, mag = RC.kl_grad_reference(m, L, go)
        upper = torch.triu(torch.ones(L.shape[-1], L.shape[-1], dtype=torch.bool), 1)
        mag = torch.where(upper, torch.zeros_like(mag), mag)                          # exactly 0 above the diagonal
        within(f'{tag}gm', rm, c_m * u * rm.abs())
        within(f'{tag}gLq', rl, c_l * u * mag)

    if kind == 'gauss':
        n, S = c
        P = RC.gauss_inputs(c, 'bound')
        t, a, gt, ga = RC.gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
        sc = P['scale']
        within('vec_out', sc * t.sum(1), RC.red_tol(n, RC.C_GAUSS, dt, abs(sc) * a.sum(1)))
        within('total_out', sc * t.sum(), RC.red_tol(S * n, RC.C_GAUSS, dt, abs(sc) * float(a.sum())))
        for form, go in (('vec', P['gout'].unsqueeze(1)), ('total', torch.full((S, 1), P['up'], dtype=torch.float64))):
            ref_mu, ref_v = go * sc * (P['y'] - P['mu']) / P['noise'], (-0.5 * go * sc / P['noise']).expand(S, n)
            within(f'{form}_gmu', ref_mu, 5 * u * ref_mu.abs())
            within(f'{form}_gv', ref_v, 3 * u * ref_v.abs())
            within(f'{form}_gnoise', sc * (go * gt).sum(), RC.red_tol(S * n, RC.C_GAUSS, dt, abs(sc) * float((go.abs() * ga).sum())))
    elif kind == 'kl':
        M, batch = c
        P = RC.kl_inputs(c, 'bound')
        ref, ab = RC.kl_reference(P['m'], P['L'])
        N = RC.kl_terms_count(M)
        within('out', ref, RC.red_tol(N, RC.C_KL, dt, ab))
        kl_grads('', P['m'], P['L'], P['up'], 1, 3)
        for name, addin in (('total_out', 0.0), ('total_out_addin', P['addin'])):
            within(name, P['scale'] * ref.sum() + addin,
                   RC.red_tol(batch * N, RC.C_KL, dt, abs(P['scale']) * float(ab.sum()) + abs(addin)))
        kl_grads('total_', P['m'], P['L'], P['scale'] * P['up'], 2, 4)
    elif kind == 'obj':
        P = RC.obj_inputs(c)
        val, ab, _ = RC.obj_reference(P)
        S, n = c.S, c.n
        within('out', val, RC.red_tol(RC.obj_terms_count(c), RC.C_GAUSS + RC.C_KL, dt, ab))
        _, _, gt, ga = RC.gauss_terms(P['y'], P['mu'], P['v'], P['noise'])
        ce = c.up * P['ell_scale']
        ref_mu = ce * (P['y'] - P['mu']) / P['noise']
        ref_v = torch.full((S, n), -0.5 * ce / P['noise'], dtype=torch.float64)
        within('gmu', ref_mu, 5 * u * ref_mu.abs())
        within('gv', ref_v, 3 * u * ref_v.abs())
        if c.noise_grad:
            within('gnoise', ce * gt.sum(), RC.red_tol(S * n, RC.C_GAUSS, dt, abs(ce) * float(ga.sum())))
        for g, (m, L, _) in enumerate(P['groups']):
            rm, rl, mag = RC.kl_grad_reference(m, L, c.up * P['kl_scale'])
            upper = torch.triu(torch.ones(c.M, c.M, dtype=torch.bool), 1)
            within(f'gm{g}', rm, 2 * u * rm.abs())
            within(f'gLq{g}', rl, 4 * u * torch.where(upper, torch.zeros_like(mag), mag))
    else:
        P = RC.mf_kl_inputs(c)
        kl, rm, rs = RC.mf_kl_reference(P)
        tol = RC.MF_KL_TOL[dt]
        bound = lambda ref: tol['atol'] + tol['rtol'] * torch.as_tensor(ref, dtype=torch.float64).abs()     # noqa: E731
        for name, ref in (('out', P['scale'] * kl), ('out_addin', P['addin'] + P['scale'] * kl),
                          ('gm', P['scale'] * P['up'] * rm), ('gs2', P['scale'] * P['up'] * rs)):
            within(name, ref, bound(ref))
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
