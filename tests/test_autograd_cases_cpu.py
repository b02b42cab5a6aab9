"""The case tables of the autograd-node tests (tests/autograd_cases.py), checked on the host (no GPU): every table reaches
every tag of its node's host branching, and loses one when the case named for it is dropped; the MatmulFn builder's
integer-exactness condition holds for every row; the whitening rows stay under the kappa cap; and each float64 reference
agrees with torch.autograd.gradcheck, or with torch autograd of an independently written dense formula, on small inputs."""
import math

import pytest
import torch

import autograd_cases as AC

F64 = torch.float64

# node -> (cases, path, required tags, id, the case whose removal loses a tag, that tag)
TABLES = {
    'matmul': (AC.MATMUL_CASES, AC.matmul_path, AC.MATMUL_TAGS, AC.matmul_id, 'f64|nt|abo|2x2|small|Gcontig', 'f64/cross_nt_abo'),
    'chol_inv': (AC.CHOL_CASES, AC.chol_path, AC.CHOL_TAGS, AC.chol_id, 'f32|n65|b3|Wbar_trans', 'f32/n65_batched_Wbar_trans'),
    'mvn': (AC.MVN_CASES, AC.mvn_path, AC.MVN_TAGS, AC.mvn_id, 'f32|n200|batch2x2|d_bcast', 'f32/n200_rank2_d_bcast'),
    'lowrank': (AC.LOWRANK_CASES, AC.lowrank_path, AC.LOWRANK_TAGS, AC.lowrank_id, 'f64|n65|k64|batch3|d_bcast',
                'f64/n65_k64_batched_d_bcast'),
    'whiten': (AC.WHITEN_CASES, AC.whiten_path, AC.WHITEN_TAGS, AC.whiten_id, 'M130|three_mid_unused|bwd32|pass|pf32|outf32',
               'cell_M130|three_mid_unused|bwd32|pass|pf32|outf32'),
    'wrap': (AC.WRAP_CASES, AC.wrap_path, AC.WRAP_TAGS, AC.wrap_id, 'rbf|shared_x2|Gexpand', 'rbf:shared_x2'),
    'layer': (AC.LAYER_CASES, AC.layer_path, AC.LAYER_TAGS, AC.layer_id, 'chol|f32|no_i8_var32|A|x_shared_grad|mean_wc|kzx_f64',
              'chol/f32:f64acc_b64+f32/4'),
}


def _reached(cases, path):
    return set().union(*(path(c) for c in cases))


@pytest.mark.parametrize('node', sorted(TABLES))
def test_the_table_reaches_every_tag_and_has_no_duplicate(node):
    cases, path, tags, cid, _, _ = TABLES[node]
    ids = [cid(c) for c in cases]
    assert len(set(ids)) == len(ids)
    assert tags - _reached(cases, path) == set()
    assert _reached(cases, path) - tags == set(), 'a tag the required set does not know: add it there'


@pytest.mark.parametrize('node', sorted(TABLES))
def test_dropping_the_named_case_loses_a_tag(node):
    cases, path, tags, cid, named, tag = TABLES[node]
    assert named in [cid(c) for c in cases]
    assert tag in tags - _reached([c for c in cases if cid(c) != named], path)


def test_matmul_rows_are_legal_exact_integers_and_the_references_are_integers():
    for c in AC.MATMUL_CASES:
        assert AC.matmul_legal(c) and max(AC.matmul_dims(c)) <= 130, AC.matmul_id(c)
        d = AC.matmul_build(c)                         # asserts: integers in -2..2, exact in the dtype, bound < 2^24
        for k in 'ABGH':
            st = d[k + '_st']
            low = {'A': 'a', 'B': 'b', 'G': 'o', 'H': 'a'}[k] in c.lower and not (k == 'G' and c.layout == 'expand')
            assert bool(torch.isnan(st).any()) == (low and st.shape[-1] > 1), (AC.matmul_id(c), k)
            if low:
                assert bool(torch.isnan(torch.triu(st, 1)[..., 0, 1:]).all()) and not bool(torch.isnan(torch.tril(st)).any())
        ref = AC.matmul_reference(c, d)                # asserts: every entry an integer within matmul_int_bound
        assert (ref['gG2'] is None) == (c.layout == 'expand')
        assert float(ref['gA'].abs().max()) > 0 and float(ref['gB2'].abs().max()) > 0


def test_matmul_table_holds_what_it_was_specified_with():
    """Written out independently of the table's construction."""
    C = AC.MATMUL_CASES
    for dt in ('f64', 'f32'):
        sub = [c for c in C if c.dt == dt]
        assert {(c.ta, c.tb, c.lower) for c in sub if c.form == '2x2' and c.size == 'small' and c.layout == 'contig'} == \
            {(ta, tb, lo) for ta in (False, True) for tb in (False, True) for lo in ('', 'a', 'b', 'o', 'ab', 'ao', 'bo', 'abo')}
        assert {c.form for c in sub} == {'2x2', '3x3', '2x3', '3x2', '1x3', '3x1', 'vec'}
        for form in ('3x3', '2x3', '3x2', '1x3', '3x1', 'vec'):
            assert {(c.ta, c.tb) for c in sub if c.form == form} == set(AC.TT), form
        assert {(c.ta, c.tb) for c in sub if c.size == 'ragged'} == set(AC.TT)
        assert {c.layout for c in sub} == {'contig', 'trans', 'expand'}
        assert any(c.lower == 'abo' and not c.ta and c.tb and c.form == '3x3' for c in sub)     # lazy.py: L L^T, both lower
    assert AC.matmul_dims(AC._mm('f64', 0, 0, '')) == (70, 55, 90)
    assert AC.matmul_dims(AC._mm('f64', 0, 0, '', size='ragged')) == (130, 65, 129)
    assert AC.matmul_shapes(AC._mm('f64', 1, 0, 'a', 'vec')) == ((70, 70), (70, 1), (70, 1))
    assert AC.matmul_shapes(AC._mm('f64', 0, 1, '', '1x3')) == ((1, 70, 90), (3, 55, 90), (3, 70, 55))


def test_matmul_path_follows_the_backward_calls():
    P = lambda *a, **k: {t[4:] for t in AC.matmul_path(AC._mm('f64', *a, **k))}        # noqa: E731
    assert {'gA_not_ta', 'gB_not_tb', 'out_lower@a', 'b_lower@b', 'a_lower@out', 'a_lower@a', 'out_lower@b', 'b_lower@out'} <= P(0, 0, 'abo')
    assert {'gA_ta', 'gB_tb', 'b_lower@a', 'out_lower@b', 'out_lower@a', 'a_lower@b'} <= P(1, 1, 'abo')
    assert 'sum0_A' in P(0, 0, '', '2x3') and 'batch1_B' in P(0, 0, '', '3x1') and 'sum0_A' not in P(0, 0, '', '3x3')
    assert '2:out_lower@out' in P(0, 0, 'o') and 'out_lower@out' not in P(0, 0, 'o')


def test_matmul_reference_is_the_gradient_gradcheck_accepts():
    """The formula the reference differentiates, at a small size with real-valued inputs: first and second order."""
    g = torch.Generator().manual_seed(3)
    for ta, tb, lower in ((False, True, 'abo'), (True, False, 'ao'), (True, True, 'b')):
        A, B = (torch.randn(5, 5, generator=g, dtype=F64, requires_grad=True) for _ in range(2))

        def f(A, B):
            Ae, Be = (torch.tril(A) if 'a' in lower else A), (torch.tril(B) if 'b' in lower else B)
            C = (Ae.mT if ta else Ae) @ (Be.mT if tb else Be)
            return torch.tril(C) if 'o' in lower else C
        assert torch.autograd.gradcheck(f, (A, B)) and torch.autograd.gradgradcheck(f, (A, B))


def test_cholesky_references_agree_with_gradcheck_and_definition():
    for c in (AC.CholCase('f64', 7, 0, 'contig'), AC.CholCase('f64', 7, 3, 'contig')):
        d, ref = AC.chol_build(c), AC.chol_reference(c)
        K = d['K'].double()
        assert torch.allclose(ref['W'].mT @ ref['W'], torch.linalg.inv(K), rtol=1e-12, atol=1e-12)       # K^-1 = W^T W
        assert float(torch.triu(ref['W'], 1).abs().max()) == 0.0

        def f(K):                                       # symmetrised input: the gradient a symmetric K has
            Ks = 0.5 * (K + K.mT)
            L = torch.linalg.cholesky(Ks)
            return torch.linalg.solve_triangular(L, torch.eye(c.n, dtype=F64).expand_as(L), upper=False)
        Kg = K.clone().requires_grad_()
        assert torch.autograd.gradcheck(f, (Kg,))
        (gK,) = torch.autograd.grad((f(Kg) * torch.tril(d['Wbar'].double())).sum(), Kg)
        assert torch.allclose(gK, ref['gK'], rtol=1e-11, atol=1e-12)


def test_log_prob_references_agree_with_torch_distributions():
    from torch.distributions import LowRankMultivariateNormal, MultivariateNormal
    for c in (AC.MvnCase('f64', 65, (3,), 'bcast'), AC.MvnCase('f64', 1, (2, 2), 'full'), AC.MvnCase('f32', 65, (), 'full')):
        d = AC.mvn_build(c)
        ref = AC.mvn_reference(c, d)
        K, dv = d['K'].double().requires_grad_(), d['d'].double().requires_grad_()
        lp = MultivariateNormal(torch.zeros(c.n, dtype=F64), covariance_matrix=K).log_prob(dv)
        gK, gd = torch.autograd.grad((lp * d['g'].double()).sum(), (K, dv))
        assert torch.allclose(lp, ref['lp'], rtol=1e-12, atol=1e-12)
        assert torch.allclose(0.5 * (gK + gK.mT), ref['gK'], rtol=1e-10, atol=1e-12) and torch.allclose(gd, ref['gd'], rtol=1e-10, atol=1e-12)
        assert ref['gd'].shape == d['d'].shape and ref['lp'].shape == c.bshape
    for c in (AC.LowrankCase('f64', 65, 8, (3,), 'bcast'), AC.LowrankCase('f64', 65, 64, (), 'full')):
        d = AC.lowrank_build(c)
        ref = AC.lowrank_reference(c, d)
        t = {k: d[k].double().requires_grad_() for k in ('root', 'diag', 'd')}
        lp = LowRankMultivariateNormal(torch.zeros(c.n, dtype=F64), t['root'], t['diag']).log_prob(t['d'])
        grads = torch.autograd.grad((lp * d['g'].double()).sum(), list(t.values()))
        assert torch.allclose(lp, ref['lp'], rtol=1e-11, atol=1e-11)
        for got, k in zip(grads, ('groot', 'gdiag', 'gd')):
            assert torch.allclose(got, ref[k], rtol=1e-9, atol=1e-11), k


def test_whitening_rows_stay_under_the_kappa_cap():
    seen = set()
    for c in AC.WHITEN_CASES:
        k = AC.whiten_kappa(c)
        if (c.M, c.groups, c.pdt) not in seen:
            seen.add((c.M, c.groups, c.pdt))
            print(f'[kappa] whiten M{c.M}|{c.groups}|p{c.pdt}: ' + ', '.join(f'{r["kappa"]:.3g}' for r in AC.whiten_reference(c)))
        assert 1.0 <= k < AC.KAPPA_CAP
    for c in AC.LAYER_CASES:
        assert AC.layer_reference(c)['kappa'] < AC.KAPPA_CAP


def test_whitening_reference_agrees_with_gradcheck_and_with_the_oracle_kernel():
    from oracle import kernels as OK
    c = AC.WhitenCase(64, 'two', True, True, 'f64', None)
    data, ref = AC.whiten_build(c), AC.whiten_reference(c)
    for grp, r in zip(data, ref):
        Z, ls, os_ = grp['Z'].double(), grp['ls'].double(), grp['os'].double()
        K = OK.rbf_ard(Z, Z, ls.unsqueeze(-2), os_) + AC.WHITEN_JITTER * torch.eye(c.M, dtype=F64)
        assert torch.allclose(r['W'].mT @ r['W'] @ K, torch.eye(c.M, dtype=F64).expand_as(K), rtol=0, atol=1e-9)
    Z = data[1]['Z'].double()[:, :6].clone().requires_grad_()
    ls, os_ = data[1]['ls'].double().clone().requires_grad_(), data[1]['os'].double().clone().requires_grad_()
    f = lambda Z, ls, os_: torch.linalg.solve_triangular(torch.linalg.cholesky(AC._kzz(Z, ls, os_, 1e-4)),        # noqa: E731
                                                         torch.eye(6, dtype=F64).expand(Z.shape[0], 6, 6), upper=False)
    assert torch.autograd.gradcheck(f, (Z, ls, os_))
    # the pass-through route adds exactly its coefficients
    with_p, without = AC.whiten_reference(c), AC.whiten_reference(c._replace(passthrough=False))
    for a, b_, grp in zip(with_p, without, data):
        for k, cf in zip(('gZ', 'gls', 'gos'), grp['coef']):
            assert torch.allclose(a[k] - b_[k], cf.double(), rtol=0, atol=1e-9)


def test_wrapper_formulas_agree_with_the_oracle_and_torch_distributions():
    from oracle import kernels as OK
    g = AC.wrap_inputs('gibbs')
    assert torch.allclose(AC.gibbs_dense(g['x1'], g['x2'], g['ell1'], g['ell2']), OK.gibbs(g['x1'], g['x2'], g['ell1'], g['ell2']),
                          rtol=1e-13, atol=1e-14)
    K = AC.gibbs_dense(g['x1'], g['x2'], g['ell1'], g['ell2'], 0.644, 0.011)
    assert torch.allclose(K, 0.644 * OK.gibbs(g['x1'], g['x2'], g['ell1'], g['ell2']) + 0.011 * torch.eye(AC.WRAP_N, dtype=F64))
    r = AC.wrap_inputs('rbf')
    assert torch.allclose(AC.rbf_dense(r['x1'][0], r['x2'], r['ls'], r['os']),
                          OK.rbf_ard(r['x1'][0], r['x2'], r['ls'].unsqueeze(-2), r['os']), rtol=1e-13, atol=1e-14)
    k = AC.wrap_inputs('kl_whitened')
    q = torch.distributions.MultivariateNormal(k['m'], scale_tril=torch.tril(k['Lq']))
    p = torch.distributions.MultivariateNormal(torch.zeros_like(k['m']), torch.eye(k['m'].numel(), dtype=F64))
    assert torch.allclose(AC.kl_whitened_dense(k['m'], k['Lq']), torch.distributions.kl_divergence(q, p), rtol=1e-11)
    e = AC.wrap_inputs('gauss_ell')
    gh_x, gh_w = (torch.from_numpy(a) for a in __import__('numpy').polynomial.hermite.hermgauss(40))
    f = e['mu'].unsqueeze(-1) + torch.sqrt(2 * e['v']).unsqueeze(-1) * gh_x
    logp = torch.distributions.Normal(f, math.sqrt(float(e['noise']))).log_prob(e['y'].reshape(1, -1, 1))
    quad = 0.5 * ((logp * gh_w).sum(-1) / math.sqrt(math.pi)).sum(-1)
    assert torch.allclose(AC.gauss_ell_dense(e['y'], e['mu'], e['v'], e['noise'], 0.5), quad, rtol=1e-10)
    for layout in AC.MM_LAYOUTS:
        G = AC.with_layout(g['G'], layout)
        assert G.shape == g['G'].shape and {'contig': G.is_contiguous(), 'trans': G.stride(-2) == 1,
                                            'expand': G.stride() == (0, 0)}[layout]


def test_layer_reference_agrees_with_the_oracle_and_the_table_with_select_projection():
    from oracle import svgp as OS
    for c in (AC.LayerCase('chol', 'f64', 'default', 'A', 'per_gp', True, 'none', False),
              AC.LayerCase('chol', 'f64', 'default', 'A', 'shared', False, 'none', False)):
        d, ref = AC.layer_build(c), AC.layer_reference(c)
        b, M, n, D = AC.LAYER_SHAPES[c.shape]
        xin = d['x'] if d['x'].dim() == 3 else d['x'].unsqueeze(0).expand(b, n, D)
        p = dict(Z=d['Z'], lengthscale=d['ls'].unsqueeze(-2), outputscale=d['os'], m=d['m'], Lq=d['Lq'],
                 mean=('constant', torch.zeros(b, 1, dtype=F64)))
        mean, var = OS.svgp_marginal(xin, p, jitter=AC.LAYER_JITTER)
        assert torch.allclose(mean, ref['mean'], rtol=1e-9, atol=1e-10) and torch.allclose(var, ref['var'], rtol=1e-9, atol=1e-10)
    # the mean-field variance is the Cholesky one at Lq = diag(sqrt(s2)); the affine mean adds x w + c
    c = AC.LayerCase('diag', 'f64', 'default', 'A', 'shared', True, 'wc', True)
    d, ref = AC.layer_build(c), AC.layer_reference(c)
    b, M, n, D = AC.LAYER_SHAPES[c.shape]
    p = dict(Z=d['Z'], lengthscale=d['ls'].unsqueeze(-2), outputscale=d['os'], m=d['m'], Lq=torch.diag_embed(d['s2'].sqrt()),
             mean=('constant', torch.zeros(b, 1, dtype=F64)))
    mean, var = OS.svgp_marginal(d['x'].unsqueeze(0).expand(b, n, D), p, jitter=AC.LAYER_JITTER)
    assert torch.allclose(var, ref['var'], rtol=1e-9, atol=1e-10)
    assert torch.allclose(mean + (d['x'] @ d['mean_w']).unsqueeze(0) + d['mean_c'], ref['mean'], rtol=1e-9, atol=1e-10)
    # the restated selection is the product's (host arithmetic only; the fused form needs whole tiles)
    from nsgp.svgp import select_projection
    for c in AC.LAYER_CASES:
        s = dict(forward_precision='f32', whiten_matmul_f64=True, whiten_matmul_i8=True, fuse_kzx=False, hidden_var_f64='auto')
        s.update(AC.LAYER_CFG[c.cfg])
        b, M, n, D = AC.LAYER_SHAPES[c.shape]
        fusable = s['fuse_kzx'] and c.dt == 'f32' and M % 128 == 0 and n % 128 == 0
        got = select_projection(AC.DT[c.dt], M, D, n, c.kzx_f64, True, fusable, s['forward_precision'], s['whiten_matmul_f64'],
                                s['whiten_matmul_i8'], s['fuse_kzx'], s['hidden_var_f64'], diag_q=c.q == 'diag')
        assert got[:3] == AC.layer_select(c), AC.layer_id(c)


@pytest.mark.parametrize('node', ['chol_inv', 'mvn', 'lowrank', 'whiten_bwd32'])
def test_no_measured_float32_error_grows_faster_than_n_kappa_u(node):
    """The per-size figures of AC.F32_MEASURED cover every size of the node's table, and from the smallest size on none of
    them grows faster than n kappa_2 (kappa: the largest among the float32 rows of that size).  They grow far slower, which
    is why the bounds are per size and not a constant times n kappa u."""
    kappa = AC.f32_kappa_by_size(node)
    for (nd, quantity), by_n in AC.F32_MEASURED.items():
        if nd != node:
            continue
        assert sorted(by_n) == sorted(kappa)
        n0 = min(by_n)
        for n, err in by_n.items():
            growth, allowed = err / by_n[n0], n * kappa[n] / (n0 * kappa[n0])
            print(f'[growth] {node} {quantity} n {n}: error x{growth:.3g} from n {n0}, n kappa x{allowed:.3g}')
            assert growth <= allowed * (1 + 1e-12)
