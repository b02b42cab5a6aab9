"""Case table of the int8 projection's column-tile walk (csrc/gemm_i8.hip, i8_proj_kernel), shared by
tools/record_i8_walk_hashes.py, tests/test_gpu_i8_walk_bits.py and tests/test_i8_walk_cases_cpu.py.

A workgroup walks WALK consecutive 64-column tiles of one 128-row tile row (with four Kzx planes; one tile with five).  The
shapes are the column-tile counts at which a walk can go wrong -- 1 (a row of one tile: a short walk and nothing else), 2
(one full walk), 3 and 5 (a short walk after full ones), 4, 9 -- each with a whole last tile (n = 64 t) and a ragged one
(n = 64 t - 7), times 128 rows (one tile row, four K-blocks), 192 (a second tile row of padding and six K-blocks) and 384
(three tile rows); every shape in the 16 variants of the pipeline record: 4 and 5 planes, 1 and 2 GPs, without and with the
row vector, float32 and float64 partials.  NAN_CASE puts a NaN into the digit-scale slot of the last K-block the second tile
row reads, for the columns 256..511 -- both tiles of the walks (4, 5) and (6, 7), none of the others."""
TILE_COUNTS = (1, 2, 3, 4, 5, 9)
ROWS = (128, 192, 384)
WALK = 2
BN, BM, BK, SLOT_COLS = 64, 128, 32, 256
SHAPES = [(M, n) for M in ROWS for t in TILE_COUNTS for n in (BN * t, BN * t - 7)]
VARIANTS = [(planes, batch, rv, p64) for planes in (4, 5) for batch in (1, 2) for rv in (0, 1) for p64 in (0, 1)]
NAN_CASE = dict(M=192, n=BN * 9 - 7, planes=4, batch=1, rv=1, p64=0, kb=5, slot=1)
GUARD = -7.0
GUARD_WORDS = 16            # in front of and behind every output
EXTRA_ROWS = 1              # partial rows beyond the tile rows: never written


def walks(n):
    """Tiles per walk along a row of the launch, in order."""
    t = -(-n // BN)
    return [min(WALK, t - i) for i in range(0, t, WALK)]
