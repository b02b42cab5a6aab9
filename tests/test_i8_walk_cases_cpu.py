"""What the case table of the int8 projection's column-tile walk (tests/i8_walk_cases.py) has to reach: full walks, short
walks, a row of one tile, ragged last tiles, padded tile rows, and a NaN digit-scale slot in the last K-block that a tile of
a full walk reads."""
import i8_walk_cases as WC


def test_walk_forms():
    forms = {n: WC.walks(n) for _, n in WC.SHAPES}
    assert any(w == [1] for w in forms.values())                                   # a one-tile row
    assert any(w == [WC.WALK] for w in forms.values())                             # exactly one full walk
    assert any(len(w) > 1 and w[-1] < WC.WALK for w in forms.values())             # a short walk after full ones
    assert any(len(w) > 1 and w[-1] == WC.WALK for w in forms.values())            # full walks only, several
    assert any(len(w) > 2 and w[-1] < WC.WALK for w in forms.values())             # several full walks, then a short one
    assert {sum(w) for w in forms.values()} == set(WC.TILE_COUNTS)
    for t in WC.TILE_COUNTS:                                                       # whole and ragged last tile of every count
        assert {n % WC.BN for _, n in WC.SHAPES if -(-n // WC.BN) == t} == {0, WC.BN - 7}


def test_rows_and_variants():
    assert {M for M, _ in WC.SHAPES} == {128, 192, 384}
    assert any(M % WC.BM for M, _ in WC.SHAPES)                                    # padded rows
    assert len(WC.VARIANTS) == 16 and len(set(WC.VARIANTS)) == 16
    for i, values in enumerate(((4, 5), (1, 2), (0, 1), (0, 1))):
        assert {v[i] for v in WC.VARIANTS} == set(values)


def test_nan_slot_sits_in_the_last_k_block_of_a_walked_tile():
    c = WC.NAN_CASE
    assert (c['M'], c['n']) in WC.SHAPES and c['planes'] == 4                      # the walked instantiation
    KB = -(-c['M'] // WC.BK)
    last_row_tile = -(-c['M'] // WC.BM) - 1
    assert c['kb'] == min((last_row_tile + 1) * WC.BM // WC.BK, KB) - 1            # the last K-block that tile row reads
    assert c['kb'] >= WC.BM // WC.BK                                               # ... and no K-block of the first tile row
    tiles = range(c['slot'] * WC.SLOT_COLS // WC.BN, min((c['slot'] + 1) * WC.SLOT_COLS, c['n'] + WC.BN - 1) // WC.BN)
    assert all(WC.walks(c['n'])[t // WC.WALK] == WC.WALK for t in tiles)           # first and second tiles of full walks
    assert {t % WC.WALK for t in tiles} == set(range(WC.WALK))
    assert 0 < min(tiles) and max(tiles) < -(-c['n'] // WC.BN) - 1                 # finite tiles on either side
