"""Record sha256 digests of what a split-K product writes through the reduce kernels of csrc/gemm.hip.

    python tools/record_splitk_reduce_hashes.py --out tests/golden/splitk_reduce_hashes.json
    python tools/record_splitk_reduce_hashes.py --compare tests/golden/splitk_reduce_hashes.json

Each row of tests/splitk_reduce_cases.py is one call of nsgp_gemm_f32 / nsgp_gemm_f64 on seeded standard-normal operands,
with C inside a buffer of guard words: in front, behind, in the padding of every row (ldc > N) and between the matrices of
a batch.  C itself starts as NaN (beta == 0) or as seeded normal values.  The digest is of the WHOLE buffer, so it pins the
sums' bits, the zeros of a C_LOWER output and every element the call has to leave alone.

--out runs every case TWICE and refuses to write unless both runs agree, every guard word is intact and every value meets
the worst-case summation bound of tests/test_gpu_gemm.py against the float64 product of the same operands: the record is of
right answers.  Run it on the commit whose output is to be preserved; tests/test_gpu_splitk_reduce_bits.py recomputes the
digests on the code under test and requires equality case by case.
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

import splitk_reduce_cases as SC          # noqa: E402

GUARD = -7.0


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def ksplit(c):
    """The K-slices the planner gives the row (nsgp_gemm_plan: by shape alone, no GPU)."""
    from nsgp import _lib
    nb1, nb2 = SC.batch_levels(c)
    buf = (ctypes.c_int32 * 11)()
    assert _lib.load().nsgp_gemm_plan(c.M, c.M, c.K, nb1, nb2, 4 if c.dt == 'f32' else 8, c.flags, 1, 1, 0, 1,
                                      ctypes.cast(buf, ctypes.c_void_p)) == 0
    return int(buf[2])


def matrix_index(c, ldpad=None, gap=SC.BATCH_GAP):
    """Flat positions of the (nb, M, N) elements of C in its guarded buffer (layout of splitk_reduce_cases)."""
    import torch
    ldc, stride, _ = SC.layout(c, ldpad, gap)
    nb = 2 if c.batch != '1' else 1
    b, r, col = torch.arange(nb).view(-1, 1, 1), torch.arange(c.M).view(1, -1, 1), torch.arange(c.M).view(1, 1, -1)
    return SC.GUARD_WORDS + b * stride + r * ldc + col


def operands(c):
    """Seeded operands of the row on the host: A (nb, M, K), B (nb, K, N), the initial C (nb, M, N)."""
    import torch
    dt = torch.float32 if c.dt == 'f32' else torch.float64
    gen = torch.Generator().manual_seed(zlib.crc32(SC.case_id(c).encode()))
    nb = 2 if c.batch != '1' else 1
    A = torch.randn((nb, c.M, c.K), generator=gen, dtype=dt)
    B = torch.randn((nb, c.K, c.M), generator=gen, dtype=dt)
    C0 = torch.randn((nb, c.M, c.M), generator=gen, dtype=dt) if c.beta != 0 else torch.full((nb, c.M, c.M), float('nan'), dtype=dt)
    return A, B, C0


def gemm_args(c, A, B, buf):
    """The arguments of nsgp_gemm_f32 / nsgp_gemm_f64 for the row, C inside `buf`; also returns the workspace (keep it)."""
    from nsgp import _lib, ops
    M, K = c.M, c.K
    nb1, nb2 = SC.batch_levels(c)
    ldc, stride, _ = SC.layout(c)
    es = buf.element_size()
    wsb = int(_lib.load().nsgp_gemm_workspace(M, M, K, nb1, nb2, es, c.flags))
    ws = ops._ws(wsb, buf.device)
    s1, s2 = (stride, 0) if nb2 == 1 else (0, stride)
    a1, a2 = (M * K, 0) if nb2 == 1 else (0, M * K)
    Cp = ctypes.c_void_p(buf.data_ptr() + SC.GUARD_WORDS * es)
    return (M, M, K, float(c.alpha), ops._p(A), K, 1, a1, a2, ops._p(B), M, 1, a1, a2, float(c.beta), Cp, ldc, s1, s2,
            nb1, nb2, int(c.flags), ops._p(ws), wsb, ops._stream()), ws


def run_case(c):
    """One call of the row's entry point -> (digests, extras for `check`)."""
    import torch
    from nsgp import _lib
    A, B, C0 = operands(c)
    _, _, total = SC.layout(c)
    buf = torch.full((total,), GUARD, dtype=C0.dtype)
    idx = matrix_index(c)
    buf[idx.reshape(-1)] = C0.reshape(-1)
    buf, Ad, Bd = buf.cuda(), A.cuda(), B.cuda()
    args, ws = gemm_args(c, Ad, Bd, buf)
    _lib.call(f'nsgp_gemm_{c.dt}', *args)
    torch.cuda.synchronize()
    return {'C': sha(buf)}, dict(buf=buf, A=A, B=B, C0=C0, idx=idx)


def check(c, x):
    """Reasons why the row's result is not a right answer (empty: it is)."""
    import torch
    why = []
    got_all = x['buf'].cpu()
    keep = torch.ones(got_all.numel(), dtype=torch.bool)
    keep[x['idx'].reshape(-1)] = False
    if not bool((got_all[keep] == GUARD).all()):
        why.append('a guard word around C was written')
    got = got_all[x['idx']].double()
    A, B, C0 = x['A'].double(), x['B'].double(), x['C0'].double()
    val, mag = c.alpha * (A @ B), abs(c.alpha) * (A.abs() @ B.abs())
    if c.flags & SC.HD:
        torch.diagonal(val, dim1=-2, dim2=-1).mul_(0.5)
    if c.beta != 0:
        val, mag = val + c.beta * C0, mag + abs(c.beta) * C0.abs()
    ks = ksplit(c)
    r, col = torch.arange(c.M).view(-1, 1), torch.arange(c.M).view(1, -1)
    up = (col > r).expand_as(val)
    lower = bool(c.flags & SC.CL)
    if lower:
        if c.beta != 0 or (ks == 1 and c.flags & SC.NF):       # left as it was (unsplit NOFILL: untouched, NaN here)
            same = got[up].view(torch.int64) == C0[up].view(torch.int64)
            if not bool(same.all()):
                why.append('the strict upper triangle was touched')
        elif not bool((got[up] == 0).all()):
            why.append('the strict upper triangle is not zero')
    mask = ~up if lower else torch.ones_like(up)
    u = torch.finfo(x['buf'].dtype).eps / 2
    bound = (c.K + ks + 4) * u * mag                           # the rounding bound of tests/test_gpu_gemm.py
    if not bool(torch.isfinite(got[mask]).all()):
        return why + ['non-finite output']
    bad = ((got - val).abs() > bound) & mask
    if bool(bad.any()):
        why.append(f'{int(bad.sum())} elements beyond the rounding bound')
    return why


def record(checked=False):
    import torch
    digests, wrong = {}, {}
    for c in SC.CASES:
        dig, extras = run_case(c)
        digests[SC.case_id(c)] = dig
        if checked:
            why = check(c, extras)
            if why:
                wrong[SC.case_id(c)] = why
    torch.cuda.synchronize()
    return digests, wrong


def write_record(path, digests):
    with open(path, 'w') as f:
        f.write('{"cases": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in digests.items()) + '\n}}\n')


def differing(ref, got):
    return sorted(k for k in set(ref) | set(got) if ref.get(k) != got.get(k))


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
        for k, v in wrong.items():
            print(f'  {k}: {v}')
        if wrong or unstable:
            print(f'NOT written: {len(wrong)} cases with wrong results, {len(unstable)} that differ between two runs: {unstable}')
            sys.exit(2)
        write_record(a.out, got)
        print(f'two runs agree, every result within tolerance: wrote {a.out}')
    if a.compare:
        with open(a.compare) as f:
            ref = json.load(f)['cases']
        diff = differing(ref, got)
        print(f'{len(diff)} of {len(ref)} recorded cases differ' + ''.join(f'\n  {k}' for k in diff))
        sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
