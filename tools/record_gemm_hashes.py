"""Record sha256 digests of what the GEMM entry points (csrc/gemm.hip) write.

    python tools/record_gemm_hashes.py --out tests/golden/gemm_hashes.json
    python tools/record_gemm_hashes.py --compare tests/golden/gemm_hashes.json

Every product of the SVGP layer and the trailing updates of potrf / trtri run through the one gemm_kernel template; each
output element is a fixed sequence of MFMA accumulations over the K-tiles followed by a fixed epilogue, so a change of the
file's structure can and must leave every output bit where it was.  The exact tests of the plain products use integer
operands and do not see a change of summation order; this tool pins the bits on seeded standard-normal operands:
    plain products     every row of GEMM_CASES (tests/test_gemm_plan_cpu.py): same shapes, layouts, flags, alpha and beta,
                       through ops.gemm; the digest is of C (of tril(C) where the header leaves the strict upper
                       triangle unspecified).  The two-level batch rows go through nsgp_gemm_* itself on CONTIGUOUS
                       (nb x nb2, M, K) operands, not on the diagonal-block windows (ld = n, level-2 stride 2 s (n + 1))
                       that nsgp_trtri passes and tests/test_gpu_gemm.py builds: same plan, same kernel, both vector-loadable
    fused products     every row of tests/gemm_bits_cases.py, through the C entry point: Y and both partial buffers of the
                       column-statistics products (unwritten rows hold a guard value), Abar, Lqbar
Operands the entry point declares triangular carry junk in the other triangle.  Output buffers start as NaN.

--out runs every case TWICE and refuses to write unless both runs agree and every result meets the tolerance the existing
test of its entry point uses against the float64 dense formula: the elementwise rounding bound of
tests/test_gpu_gemm.py (plain), the tolerances of test_fused_projection_ops_match_dense_formulas (colstats, abar, lqbar),
of test_float64_kzx_projection_of_layers_that_feed_the_next_layer (f64acc: 1.2e-7 / 2e-7 of the largest value) and the
bit equality with the materialised operand of test_projection_with_generated_kzx_equals_the_materialised_one (kzx): the
record is of right answers.  Run it on the commit whose output is to be preserved (NSGP_LIB selects the library);
tests/test_gpu_gemm_bits.py recomputes the digests on the code under test and requires equality case by case.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import gemm_bits_cases as GB              # noqa: E402
import test_gemm_plan_cpu as GP           # noqa: E402

GUARD = -7.0
JUNK = 7.0


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def all_cases():
    return list(GP.GEMM_CASES) + list(GB.CASES)


def case_id(c):
    return 'plain|' + c.name if isinstance(c, GP.Case) else GB.case_id(c)


# ---- plain products ---------------------------------------------------------------------------------------------------
def _tri_zero(rows, cols, lower):
    import torch
    r, c = torch.arange(rows).unsqueeze(1), torch.arange(cols).unsqueeze(0)
    return (c > r) if lower else (c < r)


def _run_plain(case):
    """A row of GEMM_CASES on normal operands: NaN where an operand flag declares a zero triangle, NaN around the views."""
    import torch
    from nsgp import _lib, ops
    dt = GP.DTYPES[case.dt]
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    two_level = case.nb2 > 1
    sa, sb = GP.stored_shapes(case)
    if two_level:
        sa, sb = (case.nb * case.nb2,) + sa[1:], (case.nb * case.nb2,) + sb[1:]
    dense = {'A': torch.randn(sa, generator=gen, dtype=dt), 'B': torch.randn(sb, generator=gen, dtype=dt)}
    for which, spec in (('A', case.va), ('B', case.vb)):
        if ':' in spec:                                   # one matrix for the whole batch
            dense[which] = dense[which][:1].expand_as(dense[which]).contiguous()
    opA = dense['A'].transpose(-1, -2) if case.ta else dense['A']
    opB = dense['B'].transpose(-1, -2) if case.tb else dense['B']
    zA = _tri_zero(case.M, case.K, bool(case.flags & GP.AL)) if case.flags & (GP.AL | GP.AU) else None
    zB = _tri_zero(case.K, case.N, bool(case.flags & GP.BL)) if case.flags & (GP.BL | GP.BU) else None
    nan = float('nan')
    given = {}
    for which, op, z, t in (('A', opA, zA, case.ta), ('B', opB, zB, case.tb)):
        g = op if z is None else torch.where(z, torch.full_like(op, nan), op)
        given[which] = (g.transpose(-1, -2) if t else g).contiguous()
    lead = tuple(sa[:-2])
    C0 = torch.randn(lead + (case.M, case.N), generator=gen, dtype=dt) if case.beta != 0 else \
        torch.full(lead + (case.M, case.N), nan, dtype=dt)
    out = C0.cuda()
    if two_level:
        A, B = given['A'].cuda(), given['B'].cuda()
        M, N, K = case.M, case.N, case.K
        _lib.call(f'nsgp_gemm_{case.dt}', M, N, K, float(case.alpha), ops._p(A), K, 1, case.nb2 * M * K, M * K, ops._p(B), N, 1,
                  case.nb2 * K * N, K * N, float(case.beta), ops._p(out), N, case.nb2 * M * N, M * N, case.nb, case.nb2,
                  int(case.flags), None, 0, ops._stream())
    else:
        A, B = GP.build_operands(case, 'cuda', lambda shape, which: given[which].cuda())
        ops.gemm(A, B, case.ta, case.tb, alpha=case.alpha, beta=case.beta, out=out, flags=case.flags)
    unspecified = bool(case.flags & GP.CL) and bool(case.flags & GP.NF) and case.beta == 0
    dig = {'C': sha(torch.tril(out) if unspecified else out)}
    clean = lambda op, z: (op if z is None else torch.where(z, torch.zeros_like(op), op)).double()   # noqa: E731
    return dig, dict(kind='plain', out=out, opA=clean(opA, zA), opB=clean(opB, zB), C0=C0, unspecified=unspecified)


def _check_plain(case, x):
    import torch
    from nsgp import _lib
    A, B, C0 = x['opA'], x['opB'], x['C0'].double()
    val, mag = case.alpha * (A @ B), abs(case.alpha) * (A.abs() @ B.abs())
    if case.flags & GP.HD:
        torch.diagonal(val, dim1=-2, dim2=-1).mul_(0.5)
    if case.beta != 0:
        val, mag = val + case.beta * C0, mag + abs(case.beta) * C0.abs()
    mask = torch.ones(val.shape, dtype=torch.bool)
    if case.flags & GP.CL:
        up = _tri_zero(case.M, case.N, True).expand_as(val)
        val = torch.where(up, C0 if case.beta != 0 else torch.zeros_like(val), val)
        mag = torch.where(up, torch.zeros_like(mag), mag)
        if x['unspecified']:
            mask = ~up
    buf = (ctypes.c_int32 * 11)()
    nb = max(case.nb, 1)
    _lib.load().nsgp_gemm_plan(case.M, case.N, case.K, nb, case.nb2, 4 if case.dt == 'f32' else 8, case.flags, 1, 1, 0, 1,
                               ctypes.cast(buf, ctypes.c_void_p))
    u = torch.finfo(GP.DTYPES[case.dt]).eps / 2
    bound = (case.K + buf[2] + 4) * u * mag             # the rounding bound of tests/test_gpu_gemm.py (ksplit by shape alone)
    got = x['out'].cpu().double()
    if not bool(torch.isfinite(got[mask]).all()):
        return ['non-finite output']
    bad = ((got - val).abs() > bound) & mask
    return [f'{int(bad.sum())} elements beyond the rounding bound'] if bool(bad.any()) else []


# ---- fused products ---------------------------------------------------------------------------------------------------
def _tril_junk(t):
    """The lower triangle of t (batch, M, M) with junk above it: the entry points must read the lower triangle only."""
    import torch
    return torch.tril(t) + torch.triu(torch.full_like(t, JUNK), 1)


def _close(name, got, ref, rtol, atol):
    import torch
    got = got.cpu().double()
    if torch.allclose(got, ref, rtol=rtol, atol=atol):
        return []
    return [f'{name} off by {float((got - ref).abs().max()):.3g} (rtol {rtol:g}, atol {atol:g})']


def _run_fused(c):
    import torch
    from nsgp import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(GB.seed(c))
    b, M, n, st, nan = c.batch, c.M, c.n, ops._stream(), float('nan')
    opt = dict(c.opt)
    F32, F64 = torch.float32, torch.float64
    dt = F64 if c.dt == 'f64' else F32
    es = 8 if c.dt == 'f64' else 4
    rn = lambda *shape, dtype=dt: torch.randn(*shape, generator=g, dtype=dtype)           # noqa: E731
    dev = lambda t: t.cuda()                                                              # noqa: E731
    empty = lambda *shape, dtype=dt, fill=nan: torch.full(shape, fill, dtype=dtype, device='cuda')   # noqa: E731
    x = dict(kind=c.family)
    if c.family in ('colstats', 'colstats_t', 'colstats_rows'):
        trans = int(c.family == 'colstats_t')
        L, X, rv = rn(b, M, M) / M ** 0.5, rn(b, M, n), rn(b, M)
        T = int(lib.nsgp_svgp_colstats_tiles(M, n, b, es))
        rows = T + GB.EXTRA_ROWS if c.family == 'colstats_rows' else T
        Y, p0, p1 = empty(b, M, n), empty(b, rows, n, fill=GUARD), empty(b, rows, n, fill=GUARD)
        Ld, Xd, rvd = dev(_tril_junk(L)), dev(X), dev(rv)
        if c.family == 'colstats_rows':
            _lib.call(f'nsgp_svgp_tri_gemm_colstats_rows_{c.dt}', ops._p(Ld), 0, ops._p(Xd), ops._p(rvd), b, M, n, ops._p(Y),
                      ops._p(p0), ops._p(p1), rows, st)
        else:
            _lib.call(f'nsgp_svgp_tri_gemm_colstats_{c.dt}', ops._p(Ld), trans, ops._p(Xd), ops._p(rvd), b, M, n, ops._p(Y),
                      ops._p(p0), ops._p(p1), st)
        W = torch.tril(L).double()
        x.update(Y=Y, p0=p0, p1=p1, T=T, Yref=(W.transpose(-1, -2) if trans else W) @ X.double(), rv=rv.double())
        return {'Y': sha(Y), 'part_dot': sha(p0), 'part_sq': sha(p1)}, x
    if c.family == 'abar':
        Lq = torch.tril(0.3 * rn(b, M, M)) + torch.eye(M, dtype=dt)
        C, A, m, gm, gv = rn(b, M, n), rn(b, M, n), rn(b, M), rn(b, n), rn(b, n)
        Abar = empty(b, M, n)
        args = [dev(t) for t in (_tril_junk(Lq), C, A, m, gm, gv)]
        _lib.call(f'nsgp_svgp_abar_{c.dt}', *[ops._p(t) for t in args], b, M, n, ops._p(Abar), st)
        d = lambda t: t.double()                                                          # noqa: E731
        ref = 2 * (torch.tril(d(Lq)) @ d(C)) * d(gv)[:, None, :] + d(m)[:, :, None] * d(gm)[:, None, :] - 2 * d(A) * d(gv)[:, None, :]
        x.update(Abar=Abar, ref=ref)
        return {'Abar': sha(Abar)}, x
    if c.family in ('lqbar', 'lqbar_acc'):
        A, C, gv = rn(b, M, n), rn(b, M, n), rn(b, n)
        acc = c.family == 'lqbar_acc'
        L0 = rn(b, M, M) if acc else torch.full((b, M, M), nan, dtype=dt)
        out = dev(L0)
        wsb = int(lib.nsgp_svgp_lqbar_workspace(b, M, n, es))
        ws = ops._ws(wsb, 'cuda')
        Ad, Cd, gd = dev(A), dev(C), dev(gv)
        beta = (GB.LQ_BETA,) if acc else ()
        _lib.call(f'nsgp_svgp_{c.family}_{c.dt}', ops._p(Ad), ops._p(Cd), ops._p(gd), b, M, n, *beta, ops._p(out), ops._p(ws),
                  wsb, st)
        ref = torch.tril(torch.einsum('bkj,bj,blj->bkl', A.double(), 2 * gv.double(), C.double()))
        if acc:                                          # the strict upper triangle keeps what it held
            ref = torch.where(_tri_zero(M, M, True), L0.double(), ref + GB.LQ_BETA * L0.double())
        x.update(Lqbar=out, ref=ref, split=int(wsb > 0))
        return {'Lqbar': sha(out)}, x
    # float64 accumulation on float32 data
    W = rn(b, M, M, dtype=F64) / M ** 0.5
    rv = rn(b, M, dtype=F32)
    Wd, rvd = dev(_tril_junk(W)), dev(rv)
    T = int(lib.nsgp_svgp_f64acc_tiles_for(M, n, b))
    Y = empty(b, M, n, dtype=F32)
    Wl = torch.tril(W)
    if c.family == 'kzx':
        D, xb = opt['D'], opt['xb']
        Z, xs = rn(b, M, D, dtype=F32), 1.3 * rn(*((b, n, D) if xb else (n, D)), dtype=F32)
        ls = 0.6 + torch.rand(b, D, generator=g)
        os_ = 0.5 + torch.rand(b, generator=g)
        Zd, xd, lsd, osd = dev(Z), dev(xs), dev(ls), dev(os_)
        p0, p1 = empty(b, T, n, dtype=F32, fill=GUARD), empty(b, T, n, dtype=F32, fill=GUARD)
        _lib.call('nsgp_svgp_kzx_gemm_colstats_f64acc', ops._p(Wd), ops._p(Zd), ops._p(xd), n * D if xb else 0, ops._p(lsd),
                  ops._p(osd), D, ops._p(rvd), b, M, n, ops._p(Y), ops._p(p0), ops._p(p1), T, st)
        x.update(Y=Y, p0=p0, p1=p1, W=Wd, rvd=rvd, T=T, kin=(Zd, xd, lsd, osd))
        return {'Y': sha(Y), 'part_dot': sha(p0), 'part_sq': sha(p1)}, x
    b64 = c.family in ('f64acc_b64', 'f64acc_b64p32')
    p64 = c.family in ('f64acc_b64', 'f64acc_t')
    X = rn(b, M, n, dtype=F64 if b64 else F32)
    Xd = dev(X)
    pdt = F64 if p64 else F32
    p0, p1 = empty(b, T, n, dtype=pdt, fill=GUARD), empty(b, T, n, dtype=pdt, fill=GUARD)
    if c.family == 'f64acc_t':
        _lib.call('nsgp_svgp_tri_gemm_colstats_f64acc_t', ops._p(Wd), ops._p(Xd), b, M, n, ops._p(Y), ops._p(p1), T, st)
        dig = {'Y': sha(Y), 'part_sq': sha(p1)}
        p0 = None
    else:
        _lib.call('nsgp_svgp_tri_gemm_colstats_' + c.family, ops._p(Wd), ops._p(Xd), ops._p(rvd), b, M, n, ops._p(Y), ops._p(p0),
                  ops._p(p1), T, st)
        dig = {'Y': sha(Y), 'part_dot': sha(p0), 'part_sq': sha(p1)}
    x.update(Y=Y, p0=p0, p1=p1, p64=p64, T=T, rv=rv.double(),
             Yref=(Wl.transpose(-1, -2) if c.family == 'f64acc_t' else Wl) @ X.double())
    return dig, x


def _check_fused(c, x):
    import torch
    from nsgp import _lib, ops
    f64 = c.dt == 'f64'
    M, n = c.M, c.n
    why = []
    if c.family in ('colstats', 'colstats_t', 'colstats_rows'):
        tol = dict(rtol=1e-10, atol=1e-10) if f64 else dict(rtol=2e-4, atol=2e-4 * max(1.0, M ** 0.5))
        T, ref = x['T'], x['Yref']
        why += _close('Y', x['Y'], ref, **tol)
        why += _close('sum part_dot', x['p0'][:, :T].sum(1), torch.einsum('bkj,bk->bj', ref, x['rv']), **tol)
        why += _close('sum part_sq', x['p1'][:, :T].sum(1), (ref ** 2).sum(1), **tol)
        if not bool((x['p0'][:, T:] == GUARD).all() and (x['p1'][:, T:] == GUARD).all()):
            why.append('a partial row past the tile rows was written')
    elif c.family == 'abar':
        tol = dict(rtol=1e-10, atol=1e-10) if f64 else dict(rtol=5e-4, atol=5e-4 * max(1.0, n ** 0.5))
        why += _close('Abar', x['Abar'], x['ref'], **tol)
    elif c.family in ('lqbar', 'lqbar_acc'):
        tol = dict(rtol=1e-9, atol=1e-9) if f64 else dict(rtol=5e-4, atol=5e-4 * max(1.0, n ** 0.5))
        why += _close('Lqbar', x['Lqbar'], x['ref'], **tol)
        if c.family == 'lqbar' and not bool((torch.triu(x['Lqbar'], 1) == 0).all()):
            why.append('strict upper triangle of Lqbar not zero')
        if x['split'] != dict(c.opt)['split']:
            why.append(f'split {x["split"]} is not what the row states')
    elif c.family == 'kzx':
        Zd, xd, lsd, osd = x['kin']
        K = ops.rbf_build(Zd, xd, lsd, osd)
        Y, p0, p1 = torch.empty_like(x['Y']), torch.empty_like(x['p0']), torch.empty_like(x['p1'])
        _lib.call('nsgp_svgp_tri_gemm_colstats_f64acc', ops._p(x['W']), ops._p(K), ops._p(x['rvd']), c.batch, M, n, ops._p(Y),
                  ops._p(p0), ops._p(p1), x['T'], ops._stream())
        for name, a, b_ in (('Y', x['Y'], Y), ('part_dot', x['p0'], p0), ('part_sq', x['p1'], p1)):
            if not torch.equal(a, b_):
                why.append(f'{name} differs from the product on the materialised operand')
        ref = torch.tril(x['W']).cpu() @ K.cpu().double()
        why += _close('Y', x['Y'], ref, rtol=0.0, atol=1.2e-7 * float(ref.abs().max()))
    else:
        ref = x['Yref']
        why += _close('Y', x['Y'], ref, rtol=0.0, atol=1.2e-7 * float(ref.abs().max()))
        sq = (ref ** 2).sum(1)
        dot = torch.einsum('bkj,bk->bj', ref, x['rv'])
        if x['p64']:
            tol = lambda r: dict(rtol=2e-7, atol=2e-7 * float(r.abs().max()))      # noqa: E731
        else:
            tol = lambda r: dict(rtol=2e-4, atol=2e-4 * max(1.0, M ** 0.5))        # noqa: E731
        why += _close('sum part_sq', x['p1'].sum(1), sq, **tol(sq))
        if x['p0'] is not None:
            why += _close('sum part_dot', x['p0'].sum(1), dot, **tol(dot))
    return why


def run_case(c):
    """One call of the case's entry point -> (digests {output name: sha256}, extras for `check`)."""
    return _run_plain(c) if isinstance(c, GP.Case) else _run_fused(c)


def check(c, extras):
    """Reasons why the case's results are not right answers (empty: they are)."""
    return _check_plain(c, extras) if isinstance(c, GP.Case) else _check_fused(c, extras)


def record(cases=None, checked=False):
    """({case id: digests}, {case id: reasons} of the cases whose results failed `check`)."""
    import torch
    digests, wrong = {}, {}
    for i, c in enumerate(all_cases() if cases is None else cases):
        if i % 50 == 0:
            print(f'  case {i}: {case_id(c)}', file=sys.stderr, flush=True)
        dig, extras = run_case(c)
        digests[case_id(c)] = dig
        if checked:
            why = check(c, extras)
            if why:
                wrong[case_id(c)] = why
    torch.cuda.synchronize()
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
    print(f'{len(got)} cases')
    if a.out:
        again, _ = record()
        unstable = differing(got, again)
        for k, v in list(wrong.items()) + list(unstable.items()):
            print(f'  {k}: {v}')
        if wrong or unstable:
            print(f'NOT written: {len(wrong)} cases with wrong results, {len(unstable)} that differ between two runs')
            sys.exit(2)
        write_record(a.out, got)
        print(f'two runs agree, every result within tolerance: wrote {a.out}')
    if a.compare:
        with open(a.compare) as f:
            ref = json.load(f)['cases']
        diff = differing(ref, got)
        print(f'{len(diff)} of {len(ref)} recorded cases differ' + ''.join(f'\n  {k}: {v}' for k, v in diff.items()))
        sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
