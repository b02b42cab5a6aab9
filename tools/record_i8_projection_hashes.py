"""Record sha256 digests of what the int8 projection kernel (csrc/gemm_i8.hip, nsgp_svgp_tri_gemm_colstats_i8) writes.

    python tools/record_i8_projection_hashes.py --out tests/golden/i8_projection_hashes.json
    python tools/record_i8_projection_hashes.py --compare tests/golden/i8_projection_hashes.json

The int8 product is exact -- int32 level sums, one float64 Horner, one rounding -- so a change of its schedule (how the
K-blocks are staged, how many are in flight, when the epilogue's operands are fetched) can leave every output bit where it
was.  This tool drives the three C entry points directly (digit planes of W, digit planes of Kzx, the product) on seeded
inputs and takes, per case, the sha256 of the raw bytes of A and of the two column-statistic partials planes.  The record
holds one line per shape 'M,n': three digests (A, part_dot, part_sq), each the sha256 of that array's 16 per-variant
digests joined in `VARIANTS` order (`fold`), so every case is in it and the file stays a few KB.  Run it on the commit
whose output is to be preserved; tests/test_gpu_i8_pipeline.py recomputes the digests on the code under test and requires
equality for every shape, and holds A to the float64 product so that the record itself is of right answers.

Cases (`CASES`): the row counts at which a ring of K-block stages can go wrong -- one, two, three, four K-blocks of 32
(fewer than, equal to, one more than the ring's depth: the ring wraps within one tile at M = 128), a second row tile that
is almost all padding (129), odd and even numbers of row tiles (160, 256, 384), the headline's 1024 -- times partial and
whole column tiles, both Kzx plane counts, one and two GPs per launch, with and without the row vector of the first
column statistic, float32 and float64 partials.  Case id: 'M,n|p<planes>b<batch>r<0|1>f<32|64>'.

Inputs are drawn on the host from a seeded generator; W is the float64 inverse Cholesky factor of the float32 inputs' RBF
Kzz + 1e-4 I from the library's own whitening chain (nsgp.svgp.whiten: deterministic on a given GPU, which a host LAPACK
across machines is not), so |W| spans decades as it does in a layer.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'nonstationary-precip_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 3
SMALL_M = (1, 31, 32, 33, 64, 96, 128, 129, 160, 256, 384)
SMALL_N = (1, 63, 64, 65, 127, 128, 129, 200)
SHAPES = [(M, n) for M in SMALL_M for n in SMALL_N] + [(1024, 512)]
VARIANTS = [(planes, batch, rv, p64) for planes in (4, 5) for batch in (1, 2) for rv in (0, 1) for p64 in (0, 1)]
CASES = [(M, n) + v for M, n in SHAPES for v in VARIANTS]


def case_key(M, n, planes, batch, rv, p64):
    return f'{M},{n}|p{planes}b{batch}r{rv}f{64 if p64 else 32}'


def make_inputs(M, n, batch):
    """Seeded float32 inputs of `batch` GPs (on the GPU) and the float64 whitening factor W of their Kzz + 1e-4 I."""
    import torch
    from nsgp import svgp
    g = torch.Generator().manual_seed(1000003 * M + 1009 * n + batch)
    t = dict(Z=torch.randn(batch, M, D, generator=g), x=torch.randn(n, D, generator=g),
             ls=torch.rand(batch, D, generator=g) + 0.6, os=torch.rand(batch, generator=g) + 0.5,
             rv=torch.randn(batch, M, generator=g))
    t = {k: v.cuda() for k, v in t.items()}
    with torch.no_grad():
        _, _, (W64,) = svgp.whiten([(t['Z'], t['ls'], t['os'])], out_dtype=torch.float32, with_f64=True)
    t['W64'] = W64.detach().contiguous()
    return t


def build_planes(t, planes):
    """Digit planes and scales of W and of Kzx: (Wd, wsc, Kd, ksc)."""
    import torch
    from nsgp import _lib, ops
    lib = _lib.load()
    batch, M, _ = t['Z'].shape
    n = t['x'].shape[0]
    Wd = torch.empty(int(lib.nsgp_i8_w_planes_bytes(batch, M)), dtype=torch.uint8, device='cuda')
    Kd = torch.empty(int(lib.nsgp_i8_k_planes_bytes(batch, M, n, planes)), dtype=torch.uint8, device='cuda')
    wsc = torch.empty((batch, M), dtype=torch.float64, device='cuda')
    ksc = torch.empty((int(lib.nsgp_i8_kscale_count(batch, M, n)),), dtype=torch.float64, device='cuda')
    st = ops._stream()
    _lib.call('nsgp_i8_slice_w_f64', ops._p(t['W64']), batch, M, ops._p(Wd), ops._p(wsc), st)
    _lib.call('nsgp_i8_rbf_build_f32', ops._p(t['Z']), ops._p(t['x']), 0, ops._p(t['ls']), ops._p(t['os']), batch, M, n, D,
              planes, ops._p(Kd), ops._p(ksc), None, st)
    return Wd, wsc, Kd, ksc


def product(t, built, planes, rv, p64):
    """One launch of the product: (A, part_dot, part_sq).  The outputs start as NaN, so an entry the kernel should have
    written and did not shows in the digest whatever the allocator handed out."""
    import torch
    from nsgp import _lib, ops
    Wd, wsc, Kd, ksc = built
    batch, M, _ = t['Z'].shape
    n = t['x'].shape[0]
    T = int(_lib.load().nsgp_i8_tiles(M))
    nan = float('nan')
    A = torch.full((batch, M, n), nan, dtype=torch.float32, device='cuda')
    pd = torch.float64 if p64 else torch.float32
    p0, p1 = (torch.full((batch, T, n), nan, dtype=pd, device='cuda') for _ in range(2))
    _lib.call('nsgp_svgp_tri_gemm_colstats_i8', ops._p(Wd), ops._p(wsc), ops._p(Kd), ops._p(ksc), planes,
              ops._p(t['rv']) if rv else None, batch, M, n, ops._p(A), ops._p(p0), ops._p(p1), T, 1 if p64 else 0, ops._stream())
    return A, p0, p1


def digest(*arrays):
    return [hashlib.sha256(a.detach().contiguous().cpu().numpy().tobytes()).hexdigest() for a in arrays]


def fold(per_case):
    """{'M,n': [digest of the A digests, of the part_dot digests, of the part_sq digests]} over the 16 variants of each shape
    in `VARIANTS` order, from record()'s {case id: [sha256 of A, of part_dot, of part_sq]}.  A missing case is a KeyError."""
    return {f'{M},{n}': [hashlib.sha256(''.join(per_case[case_key(M, n, *v)][i] for v in VARIANTS).encode()).hexdigest()
                         for i in range(3)]
            for M, n in sorted({tuple(int(x) for x in k.split('|')[0].split(',')) for k in per_case})}


def write_record(path, folded):
    with open(path, 'w') as f:
        f.write('{"shapes": {\n' + ',\n'.join(f'{json.dumps(k)}: {json.dumps(v)}' for k, v in folded.items()) + '\n}}\n')


def float64_product(t):
    """W @ Kzx on the host in float64, Kzx evaluated in float64 from the float32 inputs: (A_ref, Kzx), both (batch, M, n)."""
    import torch
    Z, x, ls, os_ = (t[k].cpu().double() for k in ('Z', 'x', 'ls', 'os'))
    b = Z.shape[0]
    d2 = (((Z.unsqueeze(2) - x.unsqueeze(0).unsqueeze(1)) / ls.reshape(b, 1, 1, D)) ** 2).sum(-1)
    Kzx = os_.reshape(b, 1, 1) * torch.exp(-0.5 * d2)
    return t['W64'].cpu() @ Kzx, Kzx


def record(shapes=SHAPES, on_product=None):
    """{case id: [sha256 of A, of part_dot, of part_sq]} for every case of `shapes`.  on_product(t, planes, A) is called once
    per (shape, batch, planes) with the inputs and the product of the first variant."""
    import torch
    out = {}
    for M, n in shapes:
        for batch in (1, 2):
            t = make_inputs(M, n, batch)
            for planes in (4, 5):
                built = build_planes(t, planes)
                first = True
                for rv in (0, 1):
                    for p64 in (0, 1):
                        A, p0, p1 = product(t, built, planes, rv, p64)
                        out[case_key(M, n, planes, batch, rv, p64)] = digest(A, p0, p1)
                        if first and on_product is not None:
                            on_product(t, planes, A)
                        first = False
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', help='write the digests (JSON) here')
    ap.add_argument('--compare', metavar='FILE', help='recompute and compare with a record; exit status 1 if any case differs')
    a = ap.parse_args()
    got = record()
    assert sorted(got) == sorted(case_key(*c) for c in CASES)
    folded = fold(got)
    if a.out:
        write_record(a.out, folded)
    print(f'{len(got)} cases, {len(folded)} shapes')
    if a.compare:
        with open(a.compare) as f:
            ref = json.load(f)['shapes']
        diff = sorted(k for k in set(ref) | set(folded) if ref.get(k) != folded.get(k))
        print(f'{len(diff)} of {len(ref)} recorded shapes differ' + ''.join(f'\n  {k}' for k in diff[:20]))
        sys.exit(1 if diff else 0)


if __name__ == '__main__':
    main()
