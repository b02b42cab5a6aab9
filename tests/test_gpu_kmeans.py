"""k-means on the MI355X (csrc/kmeans.hip, nsgp/cluster.py, DeepGP.initialize_inducing_points) against the float64
restatement of tests/kmeans_cases.py.  Every row of the table runs with integer data (exact arithmetic: bit-equal results,
ties and empty clusters included) and with real data (bounds from the arithmetic: 2 (D + 2) eps for a distance chain, 1 ulp for
a mean, n 2^-52 for the float64 scalars).  Run with -s for the measured figures next to their bounds."""
import functools
import math

import numpy as np
import pytest
import torch

import kmeans_cases as KC

pytestmark = pytest.mark.gpu

TORCH_DT = {'f32': torch.float32, 'f64': torch.float64}
IDS = [c.name for c in KC.CASES]


@pytest.fixture(scope='module')
def ops():
    """No skip here: the `gpu` mark selects these tests, and a device that fails to initialise must fail them."""
    from nsgp import ops as _ops
    return _ops


def _dev_x(x, strided):
    """x on the device; strided: a window of a wider buffer (leading dimension D + 3, base one element in)."""
    t = torch.from_numpy(x).cuda()
    if not strided:
        return t
    wide = torch.full((x.shape[0], x.shape[1] + 3), 7.0, dtype=t.dtype, device=t.device)
    wide[:, 1:1 + x.shape[1]] = t
    win = wide[:, 1:1 + x.shape[1]]
    assert not win.is_contiguous() or x.shape[0] == 1
    return win


@functools.lru_cache(maxsize=None)
def _integer_problem(case):
    x, c = KC.integer_inputs(case)
    lab, d2 = KC.assign_ref(x, c)
    return x, c, lab, d2


@functools.lru_cache(maxsize=None)
def _real_problem(case):
    x, c = KC.real_inputs(case)
    s = KC.sq_dists(x, c)                                 # float64, from the inputs already rounded to the row's type
    return x, c, s


def _chain_bound(case):
    return 2 * (case.D + 2) * KC.EPS[case.dtn]            # worst case of the FMA chain of D terms, relative


# --------------------------------------------------------------------------------------------
# assign
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', KC.CASES, ids=IDS)
def test_assign_integer_rows_are_bit_equal(ops, case):
    x, c, lab, d2 = _integer_problem(case)
    got_lab, got_d2 = ops.kmeans_assign(_dev_x(x, case.strided), torch.from_numpy(c).cuda())
    assert got_lab.dtype == torch.int32 and got_d2.dtype == TORCH_DT[case.dtn]
    assert np.array_equal(got_lab.cpu().numpy(), lab)
    assert np.array_equal(got_d2.cpu().numpy(), d2.astype(KC.NP_DT[case.dtn]))


@pytest.mark.parametrize('case', KC.CASES, ids=IDS)
def test_assign_real_rows_choose_an_optimal_centre_to_rounding(ops, case):
    x, c, s = _real_problem(case)
    xd = _dev_x(x, case.strided)
    lab, d2 = ops.kmeans_assign(xd, torch.from_numpy(c).cuda())
    lab, d2 = lab.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    assert lab.min() >= 0 and lab.max() < case.M
    chosen, best, b = s[np.arange(case.n), lab], s.min(1), _chain_bound(case)
    tiny = np.finfo(np.float64).tiny
    print(f'[measured] {case.name}: chosen/min - 1 <= {float((chosen / np.maximum(best, tiny)).max() - 1):.3g}, '
          f'|d2 - ref|/ref <= {float((np.abs(d2 - chosen) / np.maximum(chosen, tiny)).max()):.3g}, bound {b:.3g}')
    assert (chosen <= best * (1 + b)).all()               # no point excluded
    assert (np.abs(d2 - chosen) <= b * chosen).all()
    if case.strided:                                      # the bits of the contiguous copy
        lab2, d22 = ops.kmeans_assign(xd.contiguous(), torch.from_numpy(c).cuda())
        assert np.array_equal(lab2.cpu().numpy(), lab) and np.array_equal(d22.cpu().numpy().astype(np.float64), d2)


@pytest.mark.parametrize('dtn,D', [('f32', 2), ('f64', 2), ('f32', 5), ('f64', 1), ('f64', 5), ('f32', 3)])
def test_assign_nan_point_and_nan_centre(ops, dtn, D):
    """A NaN point gets (label 0, d2 = +inf) and a NaN centre is never chosen, first centre or not; every other point's
    result is what it is without them (integer data: bit-equal to the restatement without that centre)."""
    case = KC.Case(dtn, D, 600, 300)
    x, c = KC.integer_inputs(case)
    inf = float('inf')
    for bad_centre in (0, 7, 299):
        xn, cn = x.copy(), c.copy()
        xn[[0, 17, 511, 512, 599], D - 1] = np.nan                         # first and last lane item, both sides of a workgroup
        cn[bad_centre, 0] = np.nan
        keep = np.array([k for k in range(case.M) if k != bad_centre])
        lab_ref, d2_ref = KC.assign_ref(x, c[keep])
        lab, d2 = ops.kmeans_assign(torch.from_numpy(xn).cuda(), torch.from_numpy(cn).cuda())
        lab, d2 = lab.cpu().numpy(), d2.cpu().numpy()
        bad = np.isnan(xn).any(1)
        assert (lab[bad] == 0).all() and (d2[bad] == inf).all()
        assert np.array_equal(lab[~bad], keep[lab_ref][~bad]) and np.array_equal(d2[~bad], d2_ref[~bad].astype(d2.dtype))
        assert (lab[~bad] != bad_centre).all()


# --------------------------------------------------------------------------------------------
# update
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', KC.CASES, ids=IDS)
def test_update_integer_rows_are_bit_equal(ops, case):
    """Exact sums and one division: c_new, counts and inertia equal the restatement's bits, shift^2 the restatement added in
    the kernel's stated order; an empty cluster returns c_old's bits with count 0."""
    x, c, lab, d2 = _integer_problem(case)
    T = KC.NP_DT[case.dtn]
    c_ref, counts_ref = KC.update_ref(x, lab, c)
    c_ref = c_ref.astype(T)
    c_new, counts, stats = ops.kmeans_update(_dev_x(x, case.strided), torch.from_numpy(lab).cuda(),
                                             torch.from_numpy(d2.astype(T)).cuda(), torch.from_numpy(c).cuda())
    c_new, counts, stats = c_new.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy()
    assert counts.dtype == np.int32 and stats.dtype == np.float64 and c_new.dtype == T
    assert np.array_equal(counts, counts_ref) and counts.sum() == case.n
    assert np.array_equal(c_new.view(np.uint8), c_ref.view(np.uint8))
    empty = counts == 0
    assert np.array_equal(c_new[empty].view(np.uint8), c[empty].view(np.uint8))
    assert stats[0] == d2.sum()
    assert stats[1] == KC.shift2_in_kernel_order(c_ref, c)


@pytest.mark.parametrize('case', KC.CASES, ids=IDS)
def test_update_real_rows_means_within_one_ulp(ops, case):
    """The reference's labels fed in: centres within 1 ulp of the row's type of the float64 mean, inertia and shift^2 within
    n 2^-52 relative (shift^2 of the centres the device returned); a strided x gives the bits of its contiguous copy."""
    x, c, s = _real_problem(case)
    T = KC.NP_DT[case.dtn]
    lab = s.argmin(1).astype(np.int32)
    d2 = s[np.arange(case.n), lab].astype(T)
    xd, args = _dev_x(x, case.strided), (torch.from_numpy(lab).cuda(), torch.from_numpy(d2).cuda(), torch.from_numpy(c).cuda())
    c_new_t, counts_t, stats_t = ops.kmeans_update(xd, *args)
    c_new, counts, stats = c_new_t.cpu().numpy(), counts_t.cpu().numpy(), stats_t.cpu().numpy()
    ref = KC.exact_means(x, lab, c)
    ulp = np.spacing(np.abs(ref).astype(T)).astype(np.float64)
    err = np.abs(c_new.astype(np.float64) - ref)
    inertia = math.fsum(d2.astype(np.float64))
    df = c_new.astype(np.float64) - c.astype(np.float64)
    shift2 = math.fsum((df * df).ravel())
    rel = lambda a, b: abs(a - b) / b if b else abs(a)                     # noqa: E731
    print(f'[measured] {case.name}: |c_new - mean| <= {float((err / ulp).max()):.3g} ulp, inertia rel {rel(stats[0], inertia):.3g}, '
          f'shift2 rel {rel(stats[1], shift2):.3g}, bound {case.n * 2.0 ** -52:.3g}')
    assert np.array_equal(counts, np.bincount(lab, minlength=case.M))
    assert (err <= ulp).all()
    empty = counts == 0
    assert np.array_equal(c_new[empty].view(np.uint8), c[empty].view(np.uint8))
    assert abs(stats[0] - inertia) <= case.n * 2.0 ** -52 * inertia
    assert abs(stats[1] - shift2) <= case.n * 2.0 ** -52 * shift2
    if case.strided:
        c2, n2, s2 = ops.kmeans_update(xd.contiguous(), *args)
        assert torch.equal(c2, c_new_t) and torch.equal(n2, counts_t) and torch.equal(s2, stats_t)


# --------------------------------------------------------------------------------------------
# determinism
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [KC.Case('f32', 2, 1000, 257), KC.Case('f64', 5, 4700, 65)], ids=lambda c: c.name)
def test_two_runs_give_equal_bits(ops, case):
    import nsgp
    x, c, _ = _real_problem(case)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()

    def step():
        lab, d2 = ops.kmeans_assign(xd, cd)
        return (lab, d2) + tuple(ops.kmeans_update(xd, lab, d2, cd))
    for a, b in zip(step(), step()):
        assert torch.equal(a, b)
    r1, r2 = (nsgp.kmeans(xd, case.M, n_init=2, seed=11, max_iter=20) for _ in range(2))
    assert torch.equal(r1.centers, r2.centers) and torch.equal(r1.labels, r2.labels) and torch.equal(r1.counts, r2.counts)
    assert r1.inertia == r2.inertia and r1.n_iter == r2.n_iter


# --------------------------------------------------------------------------------------------
# kmeans()
# --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gauss_ref(n, M, D):
    x, init = KC.gauss_problem(n, M, D)
    return x, init, KC.lloyd_ref(x, init, max_iter=300, tol=0.0)


@pytest.mark.parametrize('n,M,D', KC.GAUSS)
def test_kmeans_float64_follows_the_restatement(ops, n, M, D):
    """Same init, tol = 0: the same iteration count, equal labels and counts, centres at 1e-12 (in float64 a label flipped by
    rounding needs a relative gap below 1e-13)."""
    import nsgp
    x, init, ref = _gauss_ref(n, M, D)
    res = nsgp.kmeans(torch.from_numpy(x).cuda(), M, init=torch.from_numpy(init).cuda(), tol=0.0, max_iter=300)
    worst = float(np.abs(res.centers.cpu().numpy() - ref.centers).max())
    print(f'[measured] {n, M, D}: {res.n_iter} iterations (restatement {ref.n_iter}), centres differ by {worst:.3g}')
    assert res.n_iter == ref.n_iter
    assert np.array_equal(res.labels.cpu().numpy(), ref.labels) and np.array_equal(res.counts.cpu().numpy(), ref.counts)
    assert worst <= 1e-12
    assert abs(res.inertia - ref.inertia) <= 1e-12 * ref.inertia
    assert res.centers.dtype == torch.float64 and res.labels.dtype == torch.int32 and res.counts.dtype == torch.int32


def test_kmeans_stops_by_scikit_learns_rule(ops):
    """tol > 0: the restatement's iteration count with the same threshold tol * mean_d var(x_d); max_iter caps it."""
    import nsgp
    x, init, _ = _gauss_ref(2000, 7, 2)
    ref = KC.lloyd_ref(x, init, max_iter=300, tol=1e-4)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(init).cuda()
    res = nsgp.kmeans(xd, 7, init=cd)
    assert res.n_iter == ref.n_iter < 45 and np.array_equal(res.labels.cpu().numpy(), ref.labels)
    assert nsgp.kmeans(xd, 7, init=cd, max_iter=3).n_iter == 3


def _blobs(D):
    """Blobs 3 units apart on a grid, points within 0.5 of their centre in every coordinate, uneven sizes; float32."""
    g = np.random.default_rng(40 + D)
    grid = np.stack(np.meshgrid(*[np.arange(3) * 3.0] * D, indexing='ij'), -1).reshape(-1, D)
    sizes = g.integers(5, 40, len(grid))
    blob = np.repeat(np.arange(len(grid)), sizes)
    x = (grid[blob] + g.uniform(-0.5, 0.5, (len(blob), D))).astype(np.float32)
    perm = g.permutation(len(blob))
    return x[perm], blob[perm].astype(np.int32), len(grid)


@pytest.mark.parametrize('D', [2, 3])
def test_kmeans_float32_converges_to_the_blob_means(ops, D):
    import nsgp
    x, blob, M = _blobs(D)
    init = np.stack([x[np.flatnonzero(blob == k)[0]] for k in range(M)])     # one observation per blob
    res = nsgp.kmeans(torch.from_numpy(x).cuda(), M, init=torch.from_numpy(init).cuda(), tol=0.0)
    assert np.array_equal(res.labels.cpu().numpy(), blob) and res.n_iter == 2
    means = KC.exact_means(x, blob, init)
    err = np.abs(res.centers.cpu().numpy().astype(np.float64) - means) / np.spacing(np.abs(means).astype(np.float32))
    print(f'[measured] blobs D={D}: centres within {float(err.max()):.3g} ulp of the means')
    assert (err <= 1.0).all()
    assert np.array_equal(res.counts.cpu().numpy(), np.bincount(blob, minlength=M))


def test_kmeans_float32_random_init_properties(ops):
    import nsgp
    n, M, D, eps = 3000, 20, 2, KC.EPS['f32']
    x = np.random.default_rng(77).standard_normal((n, D)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    # Lloyd never increases the inertia: recomputed in float64 from the centres of every iteration
    g = torch.Generator().manual_seed(5)
    c = xd[torch.randperm(n, generator=g)[:M].cuda()]
    prev = math.inf
    for it in range(15):
        lab, d2 = ops.kmeans_assign(xd, c)
        c, _, _ = ops.kmeans_update(xd, lab, d2, c)
        now = float(KC.sq_dists(x, c.cpu().numpy()).min(1).sum())
        assert now <= prev * (1 + n * eps), (it, now, prev)
        prev = now
    one = nsgp.kmeans(xd, M, seed=5, tol=0.0, max_iter=15)
    assert torch.equal(one.centers, c)                                      # the loop above is the loop kmeans() runs
    # the best of three restarts is the one returned, the first on a tie
    res = nsgp.kmeans(xd, M, n_init=3, seed=5)
    singles = [nsgp.kmeans(xd, M, n_init=1, seed=5 + r) for r in range(3)]
    k = int(np.argmin([s.inertia for s in singles]))
    assert res.inertia == singles[k].inertia and torch.equal(res.centers, singles[k].centers) and res.n_iter == singles[k].n_iter
    assert int(res.counts.sum()) == n and np.array_equal(res.counts.cpu().numpy(), np.bincount(res.labels.cpu().numpy(), minlength=M))
    # the returned labels are optimal for the returned centres, to the rounding of the chain
    s = KC.sq_dists(x, res.centers.cpu().numpy())
    chosen = s[np.arange(n), res.labels.cpu().numpy()]
    assert (chosen <= s.min(1) * (1 + 2 * (D + 2) * eps)).all()
    assert abs(res.inertia - chosen.sum()) <= n * eps * chosen.sum()


# --------------------------------------------------------------------------------------------
# kmeans_inducing_points, DeepGP.initialize_inducing_points
# --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', [torch.float32, torch.float64])
def test_kmeans_inducing_points(ops, dt):
    import nsgp
    g = np.random.default_rng(3)
    X = g.standard_normal((800, 3)) * np.array([1.0, 30.0, 0.01]) + np.array([5.0, -100.0, 0.0])
    X[:, 2] = 0.25                                                          # a constant column: its deviation counts as 1
    xt = torch.from_numpy(X).to(dt).cuda()
    Z = nsgp.kmeans_inducing_points(32, xt, seed=2)
    assert torch.is_tensor(Z) and Z.device == xt.device and Z.dtype == dt and Z.shape == (32, 3)
    assert (Z >= xt.min(0).values).all() and (Z <= xt.max(0).values).all()   # inside the bounding box
    std = xt.std(0, unbiased=False)
    std = torch.where(std == 0, torch.ones_like(std), std)
    assert float(std[2]) == 1.0
    assert torch.equal(Z, nsgp.kmeans(xt / std, 32, seed=2).centers * std)
    assert torch.equal(Z, nsgp.kmeans(xt, 32, seed=2, whiten=True).centers)
    assert not torch.equal(Z, nsgp.kmeans_inducing_points(32, xt, seed=3))
    if dt == torch.float64:                                                 # array-like in, float64 numpy out
        for arr in (X, X.tolist(), X.astype(np.float32)):
            Zn = nsgp.kmeans_inducing_points(32, arr, seed=2)
            assert isinstance(Zn, np.ndarray) and Zn.dtype == np.float64 and Zn.shape == (32, 3)
            assert (Zn >= np.asarray(arr).min(0)).all() and (Zn <= np.asarray(arr).max(0)).all()
        assert np.array_equal(nsgp.kmeans_inducing_points(32, X, seed=2), Z.cpu().numpy())


@pytest.mark.parametrize('tied', [True, False])
def test_deepgp_initialize_inducing_points(ops, tied):
    import nsgp
    import models.dgps as dgps
    from nsgp.gp import settings
    from nsgp.gp.mlls import DeepApproximateMLL, VariationalELBO
    torch.manual_seed(9)
    g = torch.Generator().manual_seed(9)
    n, M = 300, 16
    x, y = torch.randn(n, 2, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    model = dgps.DeepGP(2, (n, 2), num_inducing=M, tie_layers=tied).cuda()
    assert (model.layers[0] is model.layers[1]) == tied
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    res = model.initialize_inducing_points(x, seed=4)
    centres = nsgp.kmeans(x, M, seed=4).centers
    assert torch.equal(res.centers, centres)
    rep, seen = centres, set()
    names = {id(m): name for name, m in model.named_modules()}
    for layer in list(model.layers) + [model.last_layer]:
        Z = layer.variational_strategy.inducing_points
        if id(layer) not in seen:
            seen.add(id(layer))
            assert torch.equal(Z.detach(), rep.expand_as(Z)), names[id(layer)]
        if layer is not model.last_layer:
            m = layer.mean_module(rep).detach()
            assert m.shape == (M,)
            rep = torch.stack([m, m], -1)                                   # both output dimensions share the linear mean
    assert model.last_layer.variational_strategy.inducing_points.shape == (M, 2)
    after = model.state_dict()
    changed = {k for k in after if not torch.equal(after[k], before[k])}
    assert changed == {k for k in after if k.endswith('variational_strategy.inducing_points')}
    assert len(changed) == 3                                                # a tied layer is listed under both of its places
    model.train()
    mll = DeepApproximateMLL(VariationalELBO(model.likelihood, model, n))
    with settings.num_likelihood_samples(3):
        elbo = mll(model(x), y)
    (-elbo).backward()
    assert math.isfinite(float(elbo.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
