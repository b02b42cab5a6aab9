"""Record sha256 digests of what the Cholesky / triangular-inverse entry points (csrc/potrf.hip) write.

    python tools/record_potrf_hashes.py --out tests/golden/potrf_hashes.json
    python tools/record_potrf_hashes.py --compare tests/golden/potrf_hashes.json

potrf.hip promises fixed arithmetic in a fixed order per element (the panel workgroups and the inverse's row-block
workgroups factor the same diagonal block and must agree bit for bit), so a change of its structure can and must leave
every output bit where it was.  This tool drives the C entry points directly on the seeded inputs of
tests/potrf_bits_cases.py and takes, per case, the sha256 of the raw bytes of every output:
    potrf              L (the whole matrix, zeroed upper triangle included) and info
    trtri              X (the whole matrix); its input is the library's own factor of the case's matrix
    potrf_trtri        tril(X), triu(X, 1), info -- and X32, wrote32 for the _f64_w32 entry (X32 is the cast of X where the
                       library reports wrote32 = 0, as nsgp.ops.potrf_trtri_ does)
A matrix that fails on purpose contributes through info only; its healthy neighbours are digested one by one.  Strided
cases digest the whole padded buffer, guard words included, and the guards are checked separately.  Output buffers start
as NaN (guards as -7), so an entry the kernels should have written and did not shows in the digest.

--out runs every case TWICE and refuses to write unless both runs agree and every healthy result meets the tolerances of
tests/test_gpu_kernels.py::test_potrf_and_trtri against torch.linalg.cholesky in float64 (L: rtol 1e-10 / atol 1e-11 in
float64, 2e-3 / 2e-4 in float32; X L = I to 1e-9 / 2e-3), info holds what the case planted, and no guard word moved: the
record is of right answers.  Run it on the commit whose output is to be preserved (NSGP_LIB selects the library);
tests/test_gpu_potrf_bits.py recomputes the digests on the code under test and requires equality case by case.
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

import potrf_bits_cases as PB      # noqa: E402

GUARD = -7.0


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


@contextlib.contextmanager
def switches(env):
    """The case's switches in the environment for the duration of the call (the library reads them per call)."""
    old = {k: os.environ.get(k) for k, _ in env}
    os.environ.update(dict(env))
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _buffer(batch, n, dtype, padded, fill):
    """(flat buffer, its (batch, n, n) view, ld, batch stride): contiguous, or padded with guard words around every row and
    matrix.  The view starts as `fill`."""
    import torch
    ld = n + (PB.GUARD_LD if padded else 0)
    s = ld * n + (PB.GUARD_BATCH if padded else 0)
    buf = torch.full((batch * s,), GUARD, dtype=dtype, device='cuda')
    view = buf.as_strided((batch, n, n), (s, ld, 1))
    view.fill_(fill)
    return buf, view, ld, s


def _guards_intact(buf, view):
    import torch
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided(view.shape, view.stride()).fill_(False)
    return bool((buf[mask] == GUARD).all())


def run_case(c):
    """One call of the case's entry point -> (digests {output name: sha256}, outputs {name: tensor} for `check`)."""
    import torch
    from nsgp import _lib, ops
    lib = _lib.load()
    dtype = torch.float64 if c.dt == 'f64' else torch.float32
    sfx, es, n, batch = c.dt, (8 if c.dt == 'f64' else 4), c.n, c.batch
    nan = float('nan')
    A0 = PB.make_input(c)
    Abuf, A, lda, sA = _buffer(batch, n, dtype, c.strided == 'A', 0.0)
    A.copy_(A0)
    info = torch.full((batch,), -99, dtype=torch.int32, device='cuda')
    w1 = int(lib.nsgp_potrf_workspace(n, batch, es))
    w2 = int(lib.nsgp_trtri_workspace(n, batch, es))
    st = ops._stream()
    healthy = [b for b in range(batch) if b not in dict(c.bad)]
    out = {'A0': A0, 'healthy': healthy}
    with switches(c.env):
        if c.op in ('potrf', 'trtri'):
            ws = ops._ws(w1, 'cuda')
            _lib.call(f'nsgp_potrf_{sfx}', ops._p(Abuf), n, lda, sA, batch, ops._p(info), ops._p(ws), ws.numel(), st)
            out.update(L=A, info=info, guards=_guards_intact(Abuf, A))
            if c.op == 'potrf':
                dig = {'info': sha(info)}
                if not c.bad:
                    dig['L'] = sha(Abuf)
                else:
                    dig.update({f'L{b}': sha(A[b]) for b in healthy})
                return dig, out
            Xbuf, X, ldx, sX = _buffer(batch, n, dtype, False, nan)
            ws = ops._ws(w2, 'cuda')
            _lib.call(f'nsgp_trtri_{sfx}', ops._p(Abuf), n, lda, sA, ops._p(Xbuf), ldx, sX, batch, ops._p(ws), ws.numel(), st)
            out.update(X=X)
            return {'X': sha(Xbuf)}, out
        padded = c.strided == 'X'
        Xbuf, X, ldx, sX = _buffer(batch, n, dtype, padded, nan)
        ws = ops._ws(w1 + w2, 'cuda')
        if c.op == 'potrf_trtri':
            _lib.call(f'nsgp_potrf_trtri_{sfx}', ops._p(Abuf), n, lda, sA, batch, ops._p(info), ops._p(Xbuf), ldx, sX,
                      ops._p(ws), ws.numel(), st)
            guards, extra = _guards_intact(Xbuf, X), {}
        else:
            X32buf, X32, _, _ = _buffer(batch, n, torch.float32, padded, nan)
            wrote = ctypes.c_int(-1)
            _lib.call('nsgp_potrf_trtri_f64_w32', ops._p(Abuf), n, lda, sA, batch, ops._p(info), ops._p(Xbuf), ldx, sX,
                      ops._p(X32buf), ctypes.addressof(wrote), ops._p(ws), ws.numel(), st)
            guards = _guards_intact(Xbuf, X) and _guards_intact(X32buf, X32)
            if not wrote.value:
                X32 = ops.cast(X, torch.float32)
            extra = {'X32': sha(X32), 'wrote32': hashlib.sha256(str(wrote.value).encode()).hexdigest()}
            out.update(X32=X32, wrote32=wrote.value)
    out.update(X=X, info=info, guards=guards)
    dig = {'trilX': sha(torch.tril(X)), 'triuX': sha(torch.triu(X, 1)), 'info': sha(info)}
    if padded:
        dig['Xbuf'] = sha(Xbuf)
    dig.update(extra)
    return dig, out


def check(c, out):
    """Reasons why the case's results are not right answers (empty: they are)."""
    import torch
    why = []
    f64 = c.dt == 'f64'
    want_info = [dict(c.bad).get(b, 0) for b in range(c.batch)]
    if 'info' in out and out['info'].cpu().tolist() != want_info:
        why.append(f'info {out["info"].cpu().tolist()} != {want_info}')
    if not out.get('guards', True):
        why.append('a guard word was overwritten')
    eye = torch.eye(c.n, dtype=torch.float64)
    for b in out['healthy']:
        ref = torch.linalg.cholesky(out['A0'][b].double())
        if c.op in ('potrf', 'trtri'):
            L = out['L'][b].cpu().double()
            if not torch.equal(torch.triu(L, 1), torch.zeros_like(L)):
                why.append(f'matrix {b}: strict upper triangle of L not zero')
            tol = dict(rtol=1e-10, atol=1e-11) if f64 else dict(rtol=2e-3, atol=2e-4)
            if not torch.allclose(L, ref, **tol):
                why.append(f'matrix {b}: L off by {float((L - ref).abs().max()):.3g}')
        else:
            L = ref
        if c.op != 'potrf':
            X = out['X'][b].cpu().double()
            if c.op == 'trtri' and not torch.equal(torch.triu(X, 1), torch.zeros_like(X)):
                why.append(f'matrix {b}: strict upper triangle of X not zero')
            res = float((torch.tril(X) @ L - eye).abs().max())
            if not res <= (1e-9 if f64 else 2e-3):
                why.append(f'matrix {b}: |X L - I| = {res:.3g}')
        if c.op == 'potrf_trtri_w32' and not torch.equal(torch.tril(out['X32'][b]).cpu(), torch.tril(out['X'][b]).float().cpu()):
            why.append(f'matrix {b}: X32 is not X rounded once')
    return why


def record(cases=PB.CASES, checked=False):
    """({case id: digests}, {case id: reasons} of the cases whose results failed `check`)."""
    import torch
    digests, wrong = {}, {}
    for c in cases:
        dig, out = run_case(c)
        digests[PB.case_id(c)] = dig
        if checked:
            why = check(c, out)
            if why:
                wrong[PB.case_id(c)] = why
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
