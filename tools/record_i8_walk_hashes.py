"""Record sha256 digests of what the int8 projection (csrc/gemm_i8.hip, nsgp_svgp_tri_gemm_colstats_i8) writes on the shapes
of tests/i8_walk_cases.py: one to nine column tiles, whole and ragged, one to three tile rows.

    python tools/record_i8_walk_hashes.py --out tests/golden/i8_walk_hashes.json
    python tools/record_i8_walk_hashes.py --compare tests/golden/i8_walk_hashes.json

Inputs, digit planes and the float64 reference are those of tools/record_i8_projection_hashes.py.  Here every output (A and
both partials planes) lies inside a buffer of guard words -- in front, behind, and as one more partials row than the kernel
has tile rows -- and the digest is of the whole buffer.  The record holds, per shape 'M,n', the digest of its 16 variants'
digests for each of the three buffers, and the same three for NAN_CASE under 'nan'.

--out runs every case TWICE and refuses to write unless both runs agree, no guard word moved, A meets the bound of
tests/test_gpu_i8_pipeline.py against the float64 product and the partials are the column sums of that A: the record is of
right answers.  Run it on the commit whose output is to be preserved; tests/test_gpu_i8_walk_bits.py recomputes everything
on the code under test.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import i8_walk_cases as WC                # noqa: E402


def _pipeline_recorder():
    spec = importlib.util.spec_from_file_location('record_i8_projection_hashes',
                                                  os.path.join(ROOT, 'tools', 'record_i8_projection_hashes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


PR = _pipeline_recorder()


def product(t, built, planes, rv, p64):
    """One launch of the product into guarded buffers: ((bufA, bufp0, bufp1), (A, p0, p1) views of the written parts)."""
    import ctypes
    import torch
    from nsgp import _lib, ops
    Wd, wsc, Kd, ksc = built
    batch, M, _ = t['Z'].shape
    n = t['x'].shape[0]
    T = int(_lib.load().nsgp_i8_tiles(M))
    rows = T + WC.EXTRA_ROWS
    G = WC.GUARD_WORDS
    pd = torch.float64 if p64 else torch.float32
    nan = float('nan')

    def guarded(shape, dtype):
        numel = 1
        for s in shape:
            numel *= s
        buf = torch.full((numel + 2 * G,), WC.GUARD, dtype=dtype, device='cuda')
        view = buf[G:G + numel].view(shape)
        return buf, view

    bufA, A = guarded((batch, M, n), torch.float32)
    buf0, p0 = guarded((batch, rows, n), pd)
    buf1, p1 = guarded((batch, rows, n), pd)
    A.fill_(nan)
    p0[:, :T].fill_(nan)
    p1[:, :T].fill_(nan)
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())          # noqa: E731
    _lib.call('nsgp_svgp_tri_gemm_colstats_i8', ops._p(Wd), ops._p(wsc), ops._p(Kd), ops._p(ksc), planes,
              ops._p(t['rv']) if rv else None, batch, M, n, ptr(A), ptr(p0), ptr(p1), rows, 1 if p64 else 0, ops._stream())
    return (bufA, buf0, buf1), (A, p0, p1)


def guards_intact(bufs, views, T):
    G = WC.GUARD_WORDS
    ok = all(bool((b[:G] == WC.GUARD).all()) and bool((b[-G:] == WC.GUARD).all()) for b in bufs)
    return ok and all(bool((p[:, T:] == WC.GUARD).all()) for p in views[1:])


def check_values(t, planes, rv, views, finite=None):
    """Reasons why (A, p0, p1) are not right answers (empty: they are).  finite: mask of the entries of A that must be
    finite and are compared (NAN_CASE); the others must be NaN."""
    import torch
    A, p0, p1 = (v.cpu() for v in views)
    A_ref, Kzx = PR.float64_product(t)
    W64, os_ = t['W64'].cpu(), t['os'].cpu()
    T = -(-A.shape[1] // WC.BM)
    why = []
    for i in range(A.shape[0]):
        scale = float((W64[i].abs() @ Kzx[i].abs()).max())
        amax = float(A_ref[i].abs().max())
        kfloor = 2.0 ** -(7 * planes - 1) * abs(float(os_[i])) * float(W64[i].abs().sum(-1).max())
        atol = 2e-8 * scale + 1.2e-7 * amax + kfloor       # the bound of tests/test_gpu_i8_pipeline.py
        m = torch.ones_like(A[i], dtype=torch.bool) if finite is None else finite[i]
        if not bool(torch.isfinite(A[i][m]).all()) or not bool(torch.isnan(A[i][~m]).all()):
            why.append(f'GP {i}: A is not finite exactly where it has to be')
            continue
        if float((A[i].double() - A_ref[i])[m].abs().max()) > atol:
            why.append(f'GP {i}: A beyond {atol:.3g} of the float64 product')
    if finite is None:
        # the partials are sums over a tile row's rows of the unrounded float64 values, rounded once per tile row to their
        # type: against sums of the float32 A that is T roundings of A (2^-24 each) and, for float32 partials, T more
        Ad = A.double()
        u = 2.0 ** -24
        sq, sq_mag = (Ad ** 2).sum(1), (Ad ** 2).sum(1)
        if not bool(((p1[:, :T].double().sum(1) - sq).abs() <= 8 * u * sq_mag + 1e-300).all()):
            why.append('part_sq is not the column sum of A^2')
        if rv:
            r = t['rv'].cpu().double()
            dot, mag = torch.einsum('bkj,bk->bj', Ad, r), torch.einsum('bkj,bk->bj', Ad.abs(), r.abs())
            if not bool(((p0[:, :T].double().sum(1) - dot).abs() <= 8 * u * mag + 1e-300).all()):
                why.append('part_dot is not the column sum of A rv')
    return why


def digest(bufs):
    return [hashlib.sha256(b.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for b in bufs]


def record(shapes=None, checked=False):
    """({case id: [sha256 of the A, part_dot and part_sq buffers]}, {case id: reasons})."""
    import torch
    from nsgp import _lib
    out, wrong = {}, {}
    for M, n in (WC.SHAPES if shapes is None else shapes):
        T = int(_lib.load().nsgp_i8_tiles(M))
        for batch in (1, 2):
            t = PR.make_inputs(M, n, batch)
            for planes in (4, 5):
                built = PR.build_planes(t, planes)
                for rv in (0, 1):
                    for p64 in (0, 1):
                        bufs, views = product(t, built, planes, rv, p64)
                        key = PR.case_key(M, n, planes, batch, rv, p64)
                        out[key] = digest(bufs)
                        why = [] if guards_intact(bufs, views, T) else ['a guard word was written']
                        if checked and p64 == 0:           # (A is the same for both partial types)
                            why += check_values(t, planes, rv, views)
                        if why:
                            wrong[key] = why
    torch.cuda.synchronize()
    return out, wrong


def nan_case():
    """NAN_CASE: (digests, reasons).  Rows of the second tile row, columns of the poisoned slot: NaN; all else as ever."""
    import torch
    from nsgp import _lib
    c = WC.NAN_CASE
    t = PR.make_inputs(c['M'], c['n'], c['batch'])
    Wd, wsc, Kd, ksc = PR.build_planes(t, c['planes'])
    gx = -(-(-(-c['n'] // WC.BN) * WC.BN) // WC.SLOT_COLS)
    KB = -(-c['M'] // WC.BK)
    assert ksc.numel() == c['batch'] * KB * gx
    ksc.view(c['batch'], KB, gx)[0, c['kb'], c['slot']] = float('nan')
    bufs, views = product(t, (Wd, wsc, Kd, ksc), c['planes'], c['rv'], c['p64'])
    T = int(_lib.load().nsgp_i8_tiles(c['M']))
    finite = torch.ones((c['batch'], c['M'], c['n']), dtype=torch.bool)
    finite[:, WC.BM * (c['kb'] * WC.BK // WC.BM):, c['slot'] * WC.SLOT_COLS:(c['slot'] + 1) * WC.SLOT_COLS] = False
    why = [] if guards_intact(bufs, views, T) else ['a guard word was written']
    why += check_values(t, c['planes'], c['rv'], views, finite=finite)
    torch.cuda.synchronize()
    return digest(bufs), why


def fold(per_case, shapes=None):
    return {f'{M},{n}': [hashlib.sha256(''.join(per_case[PR.case_key(M, n, *v)][i] for v in WC.VARIANTS).encode()).hexdigest()
                         for i in range(3)] for M, n in (WC.SHAPES if shapes is None else shapes)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='write the digests (JSON) here')
    ap.add_argument('--compare', metavar='FILE', help='recompute and compare with a record; exit status 1 if any case differs')
    a = ap.parse_args()
    got, wrong = record(checked=bool(a.out))
    nan_dig, nan_why = nan_case()
    folded = dict(fold(got), nan=nan_dig)
    print(f'{len(got)} cases, {len(folded)} record lines')
    if a.out:
        again, _ = record()
        unstable = sorted(k for k in got if got[k] != again[k]) + (['nan'] if nan_case()[0] != nan_dig else [])
        if nan_why:
            wrong['nan'] = nan_why
        for k, v in wrong.items():
            print(f'  {k}: {v}')
        if wrong or unstable:
            print(f'NOT written: {len(wrong)} cases with wrong results, {len(unstable)} that differ between two runs: {unstable}')
            sys.exit(2)
        with open(a.out, 'w') as f:
            f.write('{"shapes": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in folded.items()) + '\n}}\n')
        print(f'two runs agree, every result right: wrote {a.out}')
    if a.compare:
        with open(a.compare) as f:
            ref = json.load(f)['shapes']
        diff = sorted(k for k in set(ref) | set(folded) if ref.get(k) != folded.get(k))
        print(f'{len(diff)} of {len(ref)} recorded lines differ' + ''.join(f'\n  {k}' for k in diff[:20]))
        sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
