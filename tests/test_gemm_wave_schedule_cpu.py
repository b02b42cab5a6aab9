"""The wave schedule of the float32 GEMM K loops, checked on the host (no GPU) through nsgp_gemm_wave_schedule -- the query
answers with the functions gemm_kernel itself runs (csrc/gemm.hip: gemm_krange, gemm_hot_range, gemm_wave_sched,
gemm_next_seg, gemm_pick_mask), so what is asserted here is what the kernel does.

A 128-row tile is 2 x 2 waves; a wave runs TM x TN MFMA tiles of 32 x 32 and decides per K-tile which of them to issue.  For
every tile shape, flag combination the library launches, tile, wave and K-slice below:

  (a) every (32 x 32 block, K-tile) that holds an element of both operands' supports and of the output's kept triangle is run;
  (b) nothing is run that the previous schedule did not run.  That rule is written down here (`parent_run`): a wave owned the
      row blocks {2r, 2r + 1} and the column blocks {2c, 2c + 1}, and ran all of its MFMA tiles or none -- in the hot loop by
      the K range [lo, hi) of its 64 rows / columns, in the one-tile-ahead loop by `tile_mask != 0`, always in the k-scaled loop;
  (c) every wave runs every K-tile exactly once, the stretches tile [h0, h1) in order, every mask run exists as a loop copy,
      and bare staging is used only where the staged tile meets no diagonal block (the invariant that keeps the workgroup's
      barriers matched: it cannot be debugged on the device);
  (d) the longest wave of a workgroup is no longer than under the previous rule;
  (e) the column-statistics epilogue (epi 1) keeps the identity row map (its partial sums run over "this wave's rows").
No case is skipped: every enumerated workgroup is checked for all five.
"""
import numpy as np
import pytest

from nsgp import ops

AL, AU, BL, BU, CL = ops.GEMM_A_LOWER, ops.GEMM_A_UPPER, ops.GEMM_B_LOWER, ops.GEMM_B_UPPER, ops.GEMM_C_LOWER
MT, BK = 32, 32
SIZES = (128, 160, 256, 384, 1024)
TILES = ((128, 128), (128, 64))
# (flags, epi, ksc, split): what gemm_impl and the fused entry points launch on 128-row float32 tiles
LAUNCHES = (
    (AL, 0, 0, False), (AU, 0, 0, False), (BL, 0, 0, False), (BU, 0, 0, False),
    (CL, 0, 0, False), (CL, 0, 0, True), (AL | BU | CL, 0, 0, False), (AL | BU | CL, 0, 0, True),
    (AL, 1, 0, False), (AU, 1, 0, False),            # column statistics, both transposes
    (AL, 2, 0, False),                               # A-adjoint
    (CL, 0, 1, False), (CL, 0, 1, True),             # k-scaled loader (Lqbar)
)


def k_slices(K, split):
    if not split:
        return [(0, K)]
    kper = max(BK, -(-(-(-K // 4)) // BK) * BK)
    n = -(-K // kper)
    return [(s * kper, min((s + 1) * kper, K)) for s in sorted({0, n // 2, n - 1})]


def clip(flags, m0, n0, bm, bn, kb, ke):
    if flags & AL:
        ke = min(ke, m0 + bm)
    if flags & AU:
        kb = max(kb, m0 // BK * BK)
    if flags & BL:
        kb = max(kb, n0 // BK * BK)
    if flags & BU:
        ke = min(ke, n0 + bn)
    if (flags & CL) and n0 > m0 + bm - 1:
        ke = kb
    return kb, ke, (-(-(ke - kb) // BK) if ke > kb else 0)


def hot_range(flags, m0, n0, bm, bn, kb, ke, nt, roll, interior):
    def regular(t):
        k0 = kb + t * BK
        if k0 + BK > ke:
            return False
        if not roll:
            if flags & (AL | AU) and k0 < m0 + bm and k0 + BK > m0:
                return False
            if flags & (BL | BU) and k0 < n0 + bn and k0 + BK > n0:
                return False
        return True
    r0 = r1 = 0
    if interior:
        while r0 < nt and not regular(r0):
            r0 += 1
        r1 = r0
        while r1 < nt and regular(r1):
            r1 += 1
    if r0 > 0:                 # float32: no hot range unless it starts at the first K-tile (every tile goes one-tile-ahead)
        r0 = r1 = 0
    return r0, max(r1 - 1, r0)


def needed(flags, m0, n0, nbr, nbc, kb, ke, nt):
    """need[rb, cb, t]: rows r, columns c and k of the block / K-tile with A(r, k), B(k, c) in their supports and C(r, c) kept.
    Difference constraints x - y <= w on (zero, r, c, k): feasible iff no negative cycle (Floyd-Warshall, vectorised)."""
    rb, cb, t = np.meshgrid(np.arange(nbr), np.arange(nbc), np.arange(nt), indexing='ij')
    big = 1 << 40
    d = np.full((4, 4) + rb.shape, big, dtype=np.int64)
    for i in range(4):
        d[i, i] = 0
    Z, R, C, Kk = 0, 1, 2, 3

    def le(x, y, w):                       # x - y <= w
        d[y, x] = np.minimum(d[y, x], w)
    r_lo, c_lo, k_lo = m0 + rb * MT, n0 + cb * MT, kb + t * BK
    k_hi = np.minimum(k_lo + BK, ke) - 1
    le(R, Z, r_lo + MT - 1); le(Z, R, -r_lo)
    le(C, Z, c_lo + MT - 1); le(Z, C, -c_lo)
    le(Kk, Z, k_hi); le(Z, Kk, -k_lo)
    zero = np.zeros_like(rb)
    if flags & AL:
        le(Kk, R, zero)                    # k <= r
    if flags & AU:
        le(R, Kk, zero)                    # k >= r
    if flags & BL:
        le(C, Kk, zero)                    # B(k, n) == 0 for n > k
    if flags & BU:
        le(Kk, C, zero)                    # B(k, n) == 0 for n < k
    if flags & CL:
        le(C, R, zero)                     # n <= m
    for m in range(4):
        for i in range(4):
            for j in range(4):
                d[i, j] = np.minimum(d[i, j], d[i, m] + d[m, j])
    return np.all([d[i, i] >= 0 for i in range(4)], axis=0)


def parent_run(flags, ksc, m0, n0, bm, bn, kb, ke, nt, h0, h1, wr, wc):
    """run[rb, cb, t] of one wave under the previous schedule (identity block map, all MFMA tiles of the wave or none)."""
    wm, wn = bm // 2, bn // 2
    tm, tn = wm // MT, wn // MT
    wm0, wn0 = wr * wm, wc * wn
    run = np.zeros((bm // MT, bn // MT, nt), dtype=bool)
    cmask = [(i, j) for i in range(tm) for j in range(tn)
             if not (flags & CL) or n0 + wn0 + j * MT <= m0 + wm0 + (i + 1) * MT - 1]

    def tile_mask(k0):
        mk = set(cmask)
        for i in range(tm):
            r0 = m0 + wm0 + i * MT
            if (flags & AL and not k0 < r0 + MT) or (flags & AU and not k0 + BK > r0):
                mk -= {(i, j) for j in range(tn)}
        for j in range(tn):
            c0 = n0 + wn0 + j * MT
            if (flags & BU and not k0 < c0 + MT) or (flags & BL and not k0 + BK > c0):
                mk -= {(i, j) for i in range(tm)}
        return mk
    lo, hi = h0, h1
    R0, C0 = m0 + wm0, n0 + wn0
    if flags & AL:
        hi = min(hi, max(-(-(R0 + wm - kb) // BK), 0))
    if flags & AU:
        lo = max(lo, (R0 - kb) // BK if R0 > kb else 0)
    if flags & BU:
        hi = min(hi, max(-(-(C0 + wn - kb) // BK), 0))
    if flags & BL:
        lo = max(lo, (C0 - kb) // BK if C0 > kb else 0)
    if not cmask:
        lo = hi = h0
    lo = min(lo, h1)
    hi = max(hi, lo)
    for t in range(nt):
        if h0 <= t < h1:
            on = True if ksc else lo <= t < hi
        else:
            on = bool(tile_mask(kb + t * BK))
        if on:
            run[wr * tm:(wr + 1) * tm, wc * tn:(wc + 1) * tn, t] = True
    return run


def check_workgroup(M, bm, bn, flags, epi, ksc, kslice, tile, edge=False, interior=True):
    tm_, tn_ = tile
    m0, n0 = tm_ * bm, tn_ * bn
    kb, ke, nt = clip(flags, m0, n0, bm, bn, *kslice)
    h0, h1 = hot_range(flags, m0, n0, bm, bn, kb, ke, nt, not ksc, interior)
    nbr, nbc = bm // MT, bn // MT
    need = needed(flags, m0, n0, nbr, nbc, kb, ke, nt)
    new = np.zeros((nbr, nbc, nt), dtype=bool)
    old = np.zeros_like(new)
    new_len, old_len, rows_seen, cols_seen = [], [], [], []
    triA, triB = flags & (AL | AU), flags & (BL | BU)
    for wave in range(4):
        wr, wc = wave >> 1, wave & 1
        s = ops.gemm_wave_schedule(bm, bn, flags, tm_, tn_, wave, kslice[0], kslice[1], epi=epi, ksc=ksc, edge=edge, interior=interior)
        where = (M, bm, bn, flags, epi, ksc, kslice, tile, wave, s)
        assert (s.nt, s.h0, s.h1, s.kbeg) == (nt, h0, h1, kb if nt else s.kbeg), where
        assert s.tm == bm // 2 // MT and s.tn == bn // 2 // MT, where
        if epi == 1 or edge or (bm, bn) != (128, 128):                                    # (e); and the whole-wave variants
            assert s.row_blocks == tuple(wr * s.tm + i for i in range(s.tm)), where
        if edge or (bm, bn) != (128, 128):                   # whole-wave schedule: all of the wave's MFMA tiles or none
            assert s.col_blocks == tuple(wc * s.tn + j for j in range(s.tn)), where
            assert s.masks == 1 | (1 << ((1 << (s.tm * s.tn)) - 1)) and len(set(zip(s.lo, s.hi))) == 1, where
        rows_seen += s.row_blocks
        cols_seen += s.col_blocks
        # (c) every K-tile once; the stretches tile [h0, h1); legal (mask, staging) pairs
        assert all(rec[3] == 1 for rec in s.tiles), where
        at = h0
        for tb, te, mk, plain in s.segments:
            assert tb == at and te > tb, where
            at = te
            assert (s.masks >> mk) & 1, where
            assert all(s.tiles[t][1] == mk and s.tiles[t][2] == (not plain) for t in range(tb, te)), where
        assert at == (h1 if h1 > h0 else h0), where
        mine = np.zeros_like(new)
        for t, (want, ran, masked, _) in enumerate(s.tiles):
            assert (s.masks >> ran) & 1 and (want & ~ran) == 0, where
            assert want == sum(1 << x for x in range(s.tm * s.tn) if s.lo[x] <= t < s.hi[x]), where
            if not masked:                               # bare staging of tile t + 1: it meets no diagonal block
                k0 = kb + (t + 1) * BK
                assert h0 <= t < h1, where
                assert not (triA and k0 < m0 + bm and k0 + BK > m0), where
                assert not (triB and k0 < n0 + bn and k0 + BK > n0), where
            for x in range(s.tm * s.tn):
                if (ran >> x) & 1:
                    mine[s.row_blocks[x // s.tn], s.col_blocks[x % s.tn], t] = True
        assert not (new & mine).any(), where             # no block belongs to two waves
        new |= mine
        new_len.append(int(mine.sum()))
        prun = parent_run(flags, ksc, m0, n0, bm, bn, kb, ke, nt, h0, h1, wr, wc)
        old |= prun
        old_len.append(int(prun.sum()))
    assert sorted(rows_seen) == sorted(2 * list(range(nbr))), (M, bm, bn, flags, epi, tile, rows_seen)
    assert sorted(cols_seen) == sorted(2 * list(range(nbc))), (M, bm, bn, flags, epi, tile, cols_seen)
    here = (M, bm, bn, flags, epi, ksc, kslice, tile)
    assert not (need & ~new).any(), ('(a) a needed block is not run', here, np.argwhere(need & ~new)[:4])
    assert not (new & ~old).any(), ('(b) runs what the previous schedule did not', here, np.argwhere(new & ~old)[:4])
    assert max(new_len) <= max(old_len), ('(d) longest wave', here, new_len, old_len)
    return sum(new_len), sum(old_len), int(need.sum())


def tiles_of(M, bm, bn, flags):
    return [(i, j) for i in range(-(-M // bm)) for j in range(-(-M // bn)) if not (flags & CL) or j * bn <= i * bm + bm - 1]


@pytest.mark.parametrize('bm,bn', TILES)
@pytest.mark.parametrize('M', SIZES)
def test_wave_schedule(M, bm, bn):
    for flags, epi, ksc, split in LAUNCHES:
        for kslice in k_slices(M, split):
            for tile in tiles_of(M, bm, bn, flags):
                check_workgroup(M, bm, bn, flags, epi, ksc, kslice, tile)


@pytest.mark.parametrize('bm,bn', TILES)
def test_wave_schedule_with_bounds_code(bm, bn):
    """The variant with bounds code (ragged or unaligned launches) keeps the whole-wave schedule; its workgroups outside the
    interior run every K-tile through the one-tile-ahead loop.  Same assertions, interior and not, split and not."""
    for flags, epi, ksc, split in LAUNCHES:
        for kslice in k_slices(384, split):
            for tile in tiles_of(384, bm, bn, flags):
                for interior in (True, False):
                    check_workgroup(384, bm, bn, flags, epi, ksc, kslice, tile, edge=True, interior=interior)


def test_issue_counts_m1024():
    """The block x K-tile totals of the three families at M = 1024 (128 x 128 tiles), previous -> now, as worked out by hand."""
    def total(flags, ksc, kslice):
        new = old = 0
        for tile in tiles_of(1024, 128, 128, flags):
            n, o, _ = check_workgroup(1024, 128, 128, flags, 0, ksc, kslice, tile)
            new, old = new + n, old + o
        return old, new
    # single pass, triangular A: 544 -> 528 (row block x K-tile) per column of 32, times 32 such columns
    assert total(AL, 0, (0, 1024)) == (544 * 32, 528 * 32)
    # lower-only outputs, a slice of three K-tiles (two in the hot loop, the last one-tile-ahead): per K-tile 28 full tiles x 16
    # blocks + 8 diagonal tiles x 12 -> 10; the bare hot loop of the k-scaled loader ran 16 on a diagonal tile
    full, now = 28 * 16, 28 * 16 + 8 * 10
    assert total(CL, 0, (0, 96)) == (3 * (full + 8 * 12), 3 * now)
    assert total(CL, 1, (0, 96)) == (2 * (full + 8 * 16) + (full + 8 * 12), 3 * now)


def test_bad_arguments():
    import ctypes
    import nsgp
    lib = nsgp.load_library()
    buf = (ctypes.c_int32 * 512)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    ok = [128, 128, 0, 0, 0, AL, 1, 0, 0, 0, 0, 256, out, 512]
    assert lib.nsgp_gemm_wave_schedule(*ok) == 0
    for i, v, rc in ((0, 96, -1), (2, 3, -3), (3, 2, -4), (4, 2, -5), (5, AL | AU, -6), (6, 0, -7), (9, 4, -10), (11, -1, -12),
                     (13, 8, -14), (13, 24 + 64 + 4, -14)):
        args = list(ok)
        args[i] = v
        assert lib.nsgp_gemm_wave_schedule(*args) == rc, (i, v)
