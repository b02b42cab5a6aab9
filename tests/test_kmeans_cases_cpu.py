"""k-means without a GPU: the case table of tests/kmeans_cases.py, its float64 restatement against scikit-learn, the C ABI
(declared, exported, arguments checked on the host, workspace sizes) and the host-side errors of the Python surface."""
import ctypes

import numpy as np
import pytest
import torch

import kmeans_cases as KC

SYMBOLS = ('nsgp_kmeans_assign_f32', 'nsgp_kmeans_assign_f64', 'nsgp_kmeans_update_f32', 'nsgp_kmeans_update_f64',
           'nsgp_kmeans_update_workspace')


def test_table_is_well_formed_and_reaches_every_required_class():
    assert len({c.name for c in KC.CASES}) == len(KC.CASES)
    for c in KC.CASES:
        assert c.dtn in ('f32', 'f64') and 1 <= c.D <= 8 and c.n >= 1 and c.M >= 1, c.name
        for x, cen in (KC.integer_inputs(c), KC.real_inputs(c)):
            assert x.shape == (c.n, c.D) and cen.shape == (c.M, c.D) and x.dtype == cen.dtype == KC.NP_DT[c.dtn], c.name
            assert np.isfinite(x).all() and np.isfinite(cen).all()
    for dtn in ('f32', 'f64'):
        rows = [c for c in KC.CASES if c.dtn == dtn]
        assert {c.D for c in rows} >= {1, 2, 3, 5}                      # every specialised dimension and the generic kernel
        assert {c.n for c in rows} >= {1, 63, 64, 65, 257, 1000}
        assert {c.M for c in rows} >= {1, 2, 63, 64, 65, 300}
        assert any(c.M > KC.KM_TILE for c in rows) and any(c.M > 2 * KC.KM_TILE for c in rows)   # a second and a third tile
        assert any(c.M > 1024 for c in rows)                            # a second cluster group of the update
        assert any(c.strided for c in rows) and {c.D for c in rows if c.strided} >= {1, 2, 3, 5}
        assert {511, 512, 513} <= {c.n for c in rows}                   # the 512-point workgroup / LDS block edge
        assert any(KC.update_chunks(c.n)[1] > 8 for c in rows)          # runs of more than one chunk
        assert any(KC.update_chunks(c.n)[0] == 2 for c in rows)         # a second stage
    big = [c for c in KC.CASES if KC.update_chunks(c.n)[0] == 2]
    tails = {c.n % (2 * KC.KM_STAGE) for c in big}
    assert any(t > KC.KM_STAGE for t in tails) and any(0 < t <= KC.KM_STAGE for t in tails)


def test_integer_rows_have_ties_and_empty_clusters_and_exact_arithmetic():
    ties = empties = 0
    for c in KC.CASES:
        if c.n > 5000:
            continue
        x, cen = KC.integer_inputs(c)
        s = KC.sq_dists(x, cen)
        assert (s == np.round(s)).all() and s.max() < 2 ** 20            # exact in float32 too
        ties += int(((s == s.min(1, keepdims=True)).sum(1) > 1).any())
        lab, _ = KC.assign_ref(x, cen)
        if c.M > 1:
            assert (lab != 1).all(), c.name                                # centre 1 repeats centre 0: the lowest index wins
        empties += int((np.bincount(lab, minlength=c.M) == 0).any())
    assert ties >= 20 and empties >= 20


def test_restatement_pieces_agree_with_each_other():
    g = np.random.default_rng(5)
    v = g.standard_normal(1000)
    assert abs(KC.sum_in_kernel_order(v) - v.sum()) < 1e-12 and KC.sum_in_kernel_order(np.arange(700.0)) == 244650.0
    assert KC.sum_in_kernel_order(np.zeros(0)) == 0.0
    x = g.standard_normal((500, 3))
    lab = g.integers(0, 7, 500).astype(np.int32)
    lab[lab == 4] = 5                                                      # cluster 4 is empty
    c_old = g.standard_normal((7, 3))
    a, counts = KC.update_ref(x, lab, c_old)
    b = KC.exact_means(x, lab, c_old)
    assert np.abs(a - b).max() < 1e-14 and (a[4] == c_old[4]).all() and (b[4] == c_old[4]).all() and counts[4] == 0
    assert counts.sum() == 500
    assert abs(KC.shift2_in_kernel_order(a, c_old) - ((a - c_old) ** 2).sum()) < 1e-12
    assert KC.workspace_bytes(1000, 2, 300) == 8 * (2 * 5 * 300 + 2 + 300)
    assert KC.update_chunks(1 << 19) == (1, 1024) and KC.update_chunks((1 << 19) + 1) == (2, 513)
    assert KC.update_chunks(5_000_000) == (8, 1221) and KC.update_chunks(0) == (1, 0)


@pytest.mark.parametrize('n,M,D', KC.GAUSS)
def test_lloyd_ref_matches_scikit_learn(n, M, D):
    """The same iteration count, identical labels, centres within 1e-12, from the same init with tol = 0."""
    from sklearn.cluster import KMeans
    x, init = KC.gauss_problem(n, M, D)
    ref = KC.lloyd_ref(x, init, max_iter=300, tol=0.0)
    assert ref.counts.min() > 0 and ref.counts.sum() == n                  # no empty cluster: scikit-learn would relocate it
    sk = KMeans(M, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(x)
    worst = float(np.abs(sk.cluster_centers_ - ref.centers).max())
    print(f'[measured] {n, M, D}: {ref.n_iter} iterations (scikit-learn {sk.n_iter_}), centres differ by {worst:.3g}')
    assert sk.n_iter_ == ref.n_iter
    assert (sk.labels_ == ref.labels).all()
    assert worst <= 1e-12
    assert abs(sk.inertia_ - ref.inertia) <= 1e-12 * ref.inertia


def test_header_declares_the_kmeans_entry_points():
    from nsgp import declared_symbols
    names = declared_symbols()
    for s in SYMBOLS:
        assert s in names, s


def test_library_exports_the_kmeans_entry_points():
    import nsgp
    lib = nsgp.load_library()
    raw = ctypes.CDLL(nsgp.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), s
    assert lib.nsgp_abi_version() == 2                                     # nothing left the ABI


def _ptr():
    buf = (ctypes.c_double * 64)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entry_points_reject_bad_arguments_before_any_launch():
    """A negative return is the position of the bad argument; the checks run on the host, so this is safe without a GPU.  No
    call here has all its arguments valid, except assign with n = 0, which launches nothing."""
    import nsgp
    lib = nsgp.load_library()
    keep, b = _ptr()
    for sfx in ('f32', 'f64'):
        fn = getattr(lib, f'nsgp_kmeans_assign_{sfx}')
        ok = [b, 2, 5, 2, b, 3, b, b, None]                                # x ldx n D c M labels d2 stream
        bad = lambda i, v: fn(*[v if k == i else a for k, a in enumerate(ok)])   # noqa: E731
        assert bad(0, None) == -1 and bad(1, 1) == -2 and bad(2, -1) == -3 and bad(2, 1 << 31) == -3     # counts are int32
        assert bad(3, 0) == -4 and bad(3, 9) == -4 and bad(4, None) == -5 and bad(5, 0) == -6 and bad(5, -3) == -6
        assert bad(5, (1 << 24) + 1) == -6                                 # NSGP_KMEANS_MAX_M: the update's grid rows
        assert bad(6, None) == -7 and bad(7, None) == -8
        assert bad(2, 0) == 0                                              # nothing to do, nothing launched
        fn = getattr(lib, f'nsgp_kmeans_update_{sfx}')
        ok = [b, 2, 5, 2, b, b, b, 3, b, b, b, b, None]                    # x ldx n D labels d2 c_old M c_new counts stats ws stream
        bad = lambda i, v: fn(*[v if k == i else a for k, a in enumerate(ok)])   # noqa: E731
        assert bad(0, None) == -1 and bad(1, 1) == -2 and bad(2, -1) == -3 and bad(3, 0) == -4 and bad(3, 9) == -4
        assert bad(4, None) == -5 and bad(5, None) == -6 and bad(6, None) == -7 and bad(7, 0) == -8
        assert bad(7, (1 << 24) + 1) == -8 and bad(2, 1 << 31) == -3
        assert bad(8, None) == -9 and bad(9, None) == -10 and bad(10, None) == -11 and bad(11, None) == -12
    del keep


def test_update_workspace_values():
    import nsgp
    ws = nsgp.load_library().nsgp_kmeans_update_workspace
    assert ws(1000, 2, 300) == 8 * (2 * 5 * 300 + 2 + 300) == 26416
    assert ws(0, 2, 5) == 8 * 5                                            # no chunk: only the per-cluster shifts
    assert ws(512, 1, 1) == 8 * (3 + 1 + 1) and ws(513, 1, 1) == 8 * (2 * 3 + 2 + 1)
    assert ws(1 << 19, 3, 4) == 8 * (1024 * 7 * 4 + 1024 + 4)              # one stage up to 2^19 points
    assert ws((1 << 19) + 1, 3, 4) == 8 * (513 * 7 * 4 + 513 + 4)          # two stages beyond
    assert ws(5_000_000, 8, 2048) == 8 * (1221 * 17 * 2048 + 1221 + 2048)  # eight stages at most
    assert ws(-1, 2, 5) == 0 and ws(10, 0, 5) == 0 and ws(10, 9, 5) == 0 and ws(10, 2, 0) == 0
    assert ws(1 << 31, 2, 5) == 0 and ws(10, 2, (1 << 24) + 1) == 0 and ws(10, 2, 1 << 24) == 8 * (5 * (1 << 24) + 1 + (1 << 24))
    for c in KC.CASES:
        assert ws(c.n, c.D, c.M) == KC.workspace_bytes(c.n, c.D, c.M), c.name


def test_ops_and_kmeans_raise_backend_error_on_cpu_tensors():
    import nsgp
    from nsgp import ops, BackendError
    x, c = torch.randn(20, 2), torch.randn(3, 2)
    with pytest.raises(BackendError):
        ops.kmeans_assign(x, c)
    with pytest.raises(BackendError):
        ops.kmeans_update(x, torch.zeros(20, dtype=torch.int32), torch.zeros(20), c)
    with pytest.raises(BackendError):
        nsgp.kmeans(x, 3)
    with pytest.raises(BackendError):
        nsgp.kmeans(x, 3, init=c)
    with pytest.raises(BackendError):
        nsgp.kmeans_inducing_points(3, x)
    assert nsgp.cluster.kmeans is nsgp.kmeans and nsgp.KMeansResult._fields == ('centers', 'labels', 'inertia', 'n_iter', 'counts')


def test_kmeans_value_errors():
    """Checked at entry, before the device is needed."""
    import nsgp
    x = torch.randn(10, 2)
    bad = [dict(M=0), dict(M=-1), dict(M=11),                              # M > n with init='random'
           dict(M=3, init=torch.randn(3, 3)), dict(M=3, init=torch.randn(4, 2)), dict(M=3, init=torch.randn(6)),
           dict(M=3, init=torch.randn(3, 2, dtype=torch.float64)),         # dtype of x expected
           dict(M=3, init='k-means++'), dict(M=3, init=torch.full((3, 2), float('nan'))),
           dict(M=3, init=torch.tensor([[0.0, 1.0], [2.0, float('inf')], [0.0, 0.0]])),
           dict(M=3, n_init=0), dict(M=3, max_iter=0), dict(M=3, tol=-1.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            nsgp.kmeans(x, kw.pop('M'), **kw)
    for v in (float('nan'), float('inf'), -float('inf')):
        y = x.clone()
        y[7, 1] = v
        with pytest.raises(ValueError):
            nsgp.kmeans(y, 3)
        with pytest.raises(ValueError):
            nsgp.kmeans_inducing_points(3, y)
    with pytest.raises(ValueError):
        nsgp.kmeans(torch.randn(10), 3)
    with pytest.raises(ValueError):
        nsgp.kmeans(torch.randn(0, 2), 1, init=torch.randn(1, 2))
    with pytest.raises(nsgp.BackendError):                                 # M > n is fine with an explicit init
        nsgp.kmeans(x, 11, init=torch.randn(11, 2))
