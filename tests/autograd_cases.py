"""Case tables, seeded builders and float64 references for the tests of the autograd nodes (nsgp/ops.py MatmulFn,
CholInvFn and the kernel / loss wrappers, nsgp/gp/distributions.py MvnLogProbFn and _lowrank_diag_log_prob, nsgp/svgp.py
WhitenFn, SVGPLayerFn and SVGPMeanFieldLayerFn), shared by tests/test_autograd_cases_cpu.py (no GPU) and
tests/test_gpu_autograd_nodes.py.  Nothing here touches a GPU or imports nsgp.ops: every reference is plain torch on the CPU in float64, differentiated by torch autograd.

The nodes are host code: they choose which backward product runs, with which triangular flags, on which operand order, and
what happens to the result (`sum(0)`, `reshape`, `None`).  `*_path(case)` restates that branching and returns the tags a
case reaches; the CPU test asserts that each table reaches every tag, so that a case cannot be dropped quietly.

MatmulFn   Data are integers in -2..2 held in the case's dtype and the inner dimension is at most 130, so every product of
           the forward, the first and the second backward pass is an integer far below 2^24 (`matmul_int_bound`): the
           float64 reference is THE answer in float32 and float64, whatever the summation order or the split along K, and
           the GPU test compares with torch.equal.  The strict upper triangle of every operand declared lower holds NaN
           in storage, and so does the incoming gradient of an `out_lower` product.
Cholesky   Inputs from potrf_bits_cases._spd64 (exact, independent of the BLAS that builds them).
Whitening  Z on a jittered lattice so that kappa_2(Kzz + jitter I) stays below KAPPA_CAP; `whiten_kappa` measures it.
"""
import collections
import functools
import itertools
import math
import zlib

import torch

import potrf_bits_cases as PB

F32, F64 = torch.float32, torch.float64
NAN = float('nan')
DT = {'f64': F64, 'f32': F32}
LOG2PI = math.log(2 * math.pi)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


def _nan_above(t):
    """t with NaN in the strict upper triangle of its trailing square."""
    n = t.shape[-1]
    mask = torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    return t.masked_fill(mask, NAN)


# ================================================================================================================
# MatmulFn
# ================================================================================================================
MatmulCase = collections.namedtuple('MatmulCase', 'dt ta tb lower form size layout')
MM_BATCH = 3
MM_SIZES = {'small': (70, 55, 90), 'ragged': (130, 65, 129)}          # (M, N, K)
MM_FORMS = ('2x2', '3x3', '2x3', '3x2', '1x3', '3x1', 'vec')          # operand ranks / batch sizes; vec: 2-D x (K,1)
MM_LAYOUTS = ('contig', 'trans', 'expand')                             # of the incoming gradient G
MM_FLAGS = {'a': 'a_lower', 'b': 'b_lower', 'o': 'out_lower'}
MM_SUBSETS = ('', 'a', 'b', 'o', 'ab', 'ao', 'bo', 'abo')
TT = ((False, False), (False, True), (True, False), (True, True))


def matmul_id(c):
    return f'{c.dt}|{"t" if c.ta else "n"}{"t" if c.tb else "n"}|{c.lower or "-"}|{c.form}|{c.size}|G{c.layout}'


def _mm(dt, ta, tb, lower='', form='2x2', size='small', layout='contig'):
    return MatmulCase(dt, bool(ta), bool(tb), lower, form, size, layout)


def _matmul_table():
    out = []
    for dt in ('f64', 'f32'):
        # every (ta, tb) with every subset of the structure flags
        out += [_mm(dt, ta, tb, lo) for ta, tb in TT for lo in MM_SUBSETS]
        # two tile rows with a ragged edge
        out += [_mm(dt, ta, tb, lo, size='ragged') for ta, tb in TT for lo in ('', 'abo')]
        # operand forms: the flags ride on the mixed transposes, and on the plain batched product
        for form in MM_FORMS[1:]:
            full = 'a' if form == 'vec' else 'abo'
            out += [_mm(dt, ta, tb, full if ta != tb else '', form) for ta, tb in TT]
        out += [_mm(dt, False, False, 'abo', '3x3'), _mm(dt, True, True, 'abo', '2x3'), _mm(dt, False, False, 'abo', '3x1'),
                _mm(dt, True, True, 'a', 'vec'), _mm(dt, False, False, 'abo', '1x3', 'ragged')]
        # layouts of the incoming gradient
        for layout in MM_LAYOUTS[1:]:
            out += [_mm(dt, ta, tb, 'o' if ta == tb else 'abo', layout=layout) for ta, tb in TT]
            out += [_mm(dt, False, True, '', '2x3', layout=layout), _mm(dt, True, False, 'ab', '3x2', 'ragged', layout)]
    return out


def matmul_dims(c):
    """(M, N, K) of the case: the size's, with the dimensions a structure flag ties made equal (first of M, N, K wins)."""
    M, N, K = MM_SIZES[c.size]
    if c.form == 'vec':
        N = 1
    base = {'M': M, 'N': N, 'K': K}
    rep = {k: k for k in base}
    for f in c.lower:
        p, q = {'a': ('M', 'K'), 'b': ('K', 'N'), 'o': ('M', 'N')}[f]
        rp, rq = rep[p], rep[q]
        for k in rep:
            if rep[k] in (rp, rq):
                rep[k] = min(rp, rq, key='MNK'.index)
    return tuple(base[rep[k]] for k in 'MNK')


def matmul_shapes(c):
    """Stored shapes of A, B and the shape of C."""
    M, N, K = matmul_dims(c)
    a = (K, M) if c.ta else (M, K)
    b = (N, K) if c.tb else (K, N)
    ba, bb = {'2x2': (None, None), '3x3': (3, 3), '2x3': (None, 3), '3x2': (3, None), '1x3': (1, 3), '3x1': (3, 1),
              'vec': (None, None)}[c.form]
    a = a if ba is None else (ba, *a)
    b = b if bb is None else (bb, *b)
    nb = max(ba or 0, bb or 0)
    return a, b, ((nb, M, N) if nb else (M, N))


def matmul_legal(c):
    M, N, K = matmul_dims(c)
    return ('a' not in c.lower or M == K) and ('b' not in c.lower or K == N) and ('o' not in c.lower or M == N)


def matmul_int_bound(c):
    """Largest magnitude any entry, or any partial sum in any order, of the forward, first-backward and second-backward
    products can reach: (largest inner or batch-summed dimension) x 2 x 2 x batch."""
    M, N, K = matmul_dims(c)
    return max(M, N, K) * 4 * MM_BATCH


def matmul_build(c):
    """dict of CPU tensors.  A, B, G, H: float64, clean (zero where the structure says so) -- the reference's inputs.
    A_st, B_st, G_st, H_st: the case's dtype as STORED for the device: NaN above the diagonal of every operand declared
    lower, of G for an out_lower product, and of H (the weight of gA in the second-order loss) for a lower A.
    G is all ones for the 'expand' layout (the gradient .sum() sends)."""
    assert matmul_legal(c), matmul_id(c)
    g = _gen('matmul', matmul_id(c)[4:])                # the same integers in both dtypes
    sa, sb, sc = matmul_shapes(c)
    A, B, H = _ints(sa, g), _ints(sb, g), _ints(sa, g)
    G = torch.ones(sc, dtype=F64) if c.layout == 'expand' else _ints(sc, g)
    out = {}
    low_g = 'o' in c.lower and c.layout != 'expand'
    for name, t, low in (('A', A, 'a' in c.lower), ('B', B, 'b' in c.lower), ('G', G, low_g), ('H', H, 'a' in c.lower)):
        out[name] = torch.tril(t) if low else t
        out[name + '_st'] = (_nan_above(t) if low else t).to(DT[c.dt])
        clean = torch.nan_to_num(out[name + '_st'].double(), nan=0.0)
        assert torch.equal(clean, out[name]) and float(out[name].abs().max()) <= 2, 'integers in -2..2, exact in the dtype'
    assert matmul_int_bound(c) < 2 ** 24
    return out


def matmul_reference(c, d):
    """float64 torch autograd of C = [tril] op(tril? A) op(tril? B): dict C, gA, gB, and the second order gB2, gG2 =
    d/dB, d/dG of sum(gA o H) (gG2 None for the 'expand' layout, whose G is not an input)."""
    A, B = d['A'].clone().requires_grad_(), d['B'].clone().requires_grad_()
    G = d['G'].clone().requires_grad_(c.layout != 'expand')
    Ae = torch.tril(A) if 'a' in c.lower else A
    Be = torch.tril(B) if 'b' in c.lower else B
    C = (Ae.mT if c.ta else Ae) @ (Be.mT if c.tb else Be)
    if 'o' in c.lower:
        C = torch.tril(C)
    gA, gB = torch.autograd.grad(C, (A, B), torch.tril(G) if 'o' in c.lower else G, create_graph=True)
    wrt = (B, G) if G.requires_grad else (B,)
    second = torch.autograd.grad((gA * d['H']).sum(), wrt)
    ref = dict(C=C.detach(), gA=gA.detach(), gB=gB.detach(), gB2=second[0], gG2=second[1] if len(second) == 2 else None)
    bound = matmul_int_bound(c)
    for k, v in ref.items():
        assert v is None or (torch.equal(v, v.round()) and float(v.abs().max()) <= bound), (matmul_id(c), k)
    return ref


def _mm_backward_calls(ta, tb, la, lb, lo):
    """MatmulFn.backward restated: [(branch, (ta, tb, a_lower, b_lower, out_lower) of the recursive matmul, what its two
    operands are)], flags carried as the NAME of the flag of the original product they come from (or None)."""
    ga = ('gA_not_ta', (False, not tb, lo, lb, la), ('G', 'B')) if not ta else ('gA_ta', (tb, True, lb, lo, la), ('B', 'G'))
    gb = ('gB_not_tb', (not ta, False, la, lo, lb), ('A', 'G')) if not tb else ('gB_tb', (True, ta, lo, la, lb), ('G', 'A'))
    return ga, gb


def matmul_path(c):
    lab = {f: (MM_FLAGS[f] if f in c.lower else None) for f in 'abo'}
    tags = {f'G_{c.layout}', f'form_{c.form}', f'size_{c.size}'}
    if (c.form, c.size, c.layout) == ('2x2', 'small', 'contig'):          # the full cross of transposes and structure flags
        tags.add(f'cross_{"t" if c.ta else "n"}{"t" if c.tb else "n"}_{c.lower or "-"}')
    first = _mm_backward_calls(c.ta, c.tb, lab['a'], lab['b'], lab['o'])

    def slots(cfg, pre):
        return {f'{pre}{flag}@{slot}' for flag, slot in zip(cfg[2:], ('a', 'b', 'out')) if flag}
    for branch, cfg, _ in first:
        tags |= {branch} | slots(cfg, '')
    # second order: the backward of gA's product, with respect to both of its operands (B and G)
    tags.add('second_order')
    for branch, cfg, _ in _mm_backward_calls(*first[0][1]):
        tags |= {'2:' + branch} | slots(cfg, '2:')
    ra, rb = {'2x3': ('sum0', None), '3x2': (None, 'sum0'), '1x3': ('batch1', None), '3x1': (None, 'batch1')}.get(c.form, (None, None))
    if ra:
        tags.add(f'{ra}_A')
    if rb:
        tags.add(f'{rb}_B')
    return {f'{c.dt}/{t}' for t in tags}


MATMUL_TAGS = {f'{dt}/{t}' for dt in DT for t in (
    ['gA_ta', 'gA_not_ta', 'gB_tb', 'gB_not_tb', '2:gA_ta', '2:gA_not_ta', '2:gB_tb', '2:gB_not_tb', 'second_order',
     'sum0_A', 'sum0_B', 'batch1_A', 'batch1_B'] +
    [f'{flag}@{slot}' for flag in MM_FLAGS.values() for slot in ('a', 'b', 'out') if (flag, slot) != ('out_lower', 'out')] +
    # (first order never puts out_lower on an output; second order does.  gA's product has a_lower on its output, so its own
    #  backward never puts a_lower on an output, nor b_lower on a first operand)
    [f'2:{flag}@{slot}' for flag in MM_FLAGS.values() for slot in ('a', 'b', 'out')
     if (flag, slot) not in (('a_lower', 'out'), ('b_lower', 'a'))] +
    [f'G_{x}' for x in MM_LAYOUTS] + [f'form_{x}' for x in MM_FORMS] + [f'size_{x}' for x in MM_SIZES] +
    [f'cross_{tt}_{lo or "-"}' for tt in ('nn', 'nt', 'tn', 'tt') for lo in MM_SUBSETS])}
MATMUL_CASES = _matmul_table()


# ================================================================================================================
# CholInvFn
# ================================================================================================================
CholCase = collections.namedtuple('CholCase', 'dt n batch layout')      # batch 0: a 2-D input; layout of Wbar
CHOL_NS = (1, 7, 64, 65, 130, 200)
CHOL_CASES = [CholCase(dt, n, b, lay) for dt in ('f64', 'f32') for n in CHOL_NS for b in (0, 3) for lay in ('contig', 'trans')]


def chol_id(c):
    return f'{c.dt}|n{c.n}|b{c.batch}|Wbar_{c.layout}'


def chol_path(c):
    return {f'{c.dt}/n{c.n}_{"batched" if c.batch else "unbatched"}_Wbar_{c.layout}'}


CHOL_TAGS = {f'{dt}/n{n}_{f}_Wbar_{lay}' for dt in DT for n in CHOL_NS for f in ('batched', 'unbatched') for lay in ('contig', 'trans')}


def chol_build(c):
    """K in the case's dtype (2-D when batch == 0) and a full Wbar: float32-representable normals, garbage above the
    diagonal included (only tril(Wbar) reaches W)."""
    K = PB._spd64(c.n, max(c.batch, 1)).to(DT[c.dt])
    K = K if c.batch else K[0]
    Wbar = torch.randn(K.shape, generator=_gen('chol', c.n, c.batch), dtype=F32).to(DT[c.dt])
    return dict(K=K.clone(), Wbar=Wbar)


@functools.lru_cache(maxsize=None)
def _chol_reference(dt, n, batch):
    d = chol_build(CholCase(dt, n, batch, 'contig'))
    K = d['K'].double().requires_grad_()
    L = torch.linalg.cholesky(K)
    W = torch.linalg.solve_triangular(L, torch.eye(n, dtype=F64), upper=False)
    (gK,) = torch.autograd.grad((W * torch.tril(d['Wbar'].double())).sum(), K)
    kappa = float(torch.linalg.cond(K.detach()).max())
    return dict(W=W.detach(), gK=0.5 * (gK + gK.mT), kappa=kappa)


def chol_reference(c):
    """W = chol(K)^-1, the symmetric gradient of sum(W o tril(Wbar)) and kappa_2(K), float64, of the case's own (rounded)
    input.  Shared by the two layouts of Wbar; treat as read-only."""
    return _chol_reference(c.dt, c.n, c.batch)


# ================================================================================================================
# MvnLogProbFn and _lowrank_diag_log_prob
# ================================================================================================================
MvnCase = collections.namedtuple('MvnCase', 'dt n bshape dform')        # dform: 'full' | 'bcast' (d of shape (n,))
MVN_NS = (1, 65, 200)
MVN_BSHAPES = ((), (3,), (2, 2))
MVN_CASES = [MvnCase(dt, n, bs, df) for dt in ('f64', 'f32') for n in MVN_NS for bs in MVN_BSHAPES
             for df in (('full',) if bs == () else ('full', 'bcast'))]

# The low-rank form multiplies through ops.matmul, which takes 2-D and 3-D operands: batch shapes () and (3,).
LowrankCase = collections.namedtuple('LowrankCase', 'dt n k bshape dform')
LOWRANK_KS = (1, 8, 64)
LOWRANK_CASES = [LowrankCase(dt, n, k, bs, df) for dt in ('f64', 'f32') for n in MVN_NS for k in LOWRANK_KS if k <= n
                 for bs in MVN_BSHAPES[:2] for df in (('full',) if bs == () else ('full', 'bcast'))]


def mvn_id(c):
    return f'{c.dt}|n{c.n}|batch{"x".join(map(str, c.bshape)) or "-"}|d_{c.dform}'


def lowrank_id(c):
    return f'{c.dt}|n{c.n}|k{c.k}|batch{"x".join(map(str, c.bshape)) or "-"}|d_{c.dform}'


def mvn_path(c):
    """MvnLogProbFn restated: K.reshape(-1, n, n); d.expand(batch, n) copies when d is (n,) under a batch; gd goes through
    sum_to_size exactly then."""
    tags = {f'batch_rank{len(c.bshape)}', f'n{c.n}', 'd_expand' if (c.dform == 'bcast') else 'd_as_is',
            'gd_sum_to_size' if c.dform == 'bcast' else 'gd_as_is', f'n{c.n}_rank{len(c.bshape)}_d_{c.dform}'}
    return {f'{c.dt}/{t}' for t in tags}


MVN_TAGS = {f'{dt}/{t}' for dt in DT for t in ['batch_rank0', 'batch_rank1', 'batch_rank2', 'd_expand', 'd_as_is',
                                                'gd_sum_to_size', 'gd_as_is'] + [f'n{n}' for n in MVN_NS] +
            [f'n{n}_rank{r}_d_{df}' for n in MVN_NS for r in (0, 1, 2) for df in ('full', 'bcast') if (r, df) != (0, 'bcast')]}


def lowrank_path(c):
    """_lowrank_diag_log_prob restated: three ops.matmul products (R^T R, R^T d, W v with a_lower) and ops.chol_inv of the
    k x k system, batched or not; a (n,) d under a batch broadcasts in the elementwise ops before the products."""
    form = 'batched' if c.bshape else 'unbatched'
    tags = {form, f'k{c.k}', f'n{c.n}', f'd_{c.dform}', f'n{c.n}_k{c.k}_{form}_d_{c.dform}'}
    return {f'{c.dt}/{t}' for t in tags}


LOWRANK_TAGS = {f'{dt}/{t}' for dt in DT for t in ['batched', 'unbatched', 'd_full', 'd_bcast'] + [f'k{k}' for k in LOWRANK_KS] +
                [f'n{n}' for n in MVN_NS] +
                [f'n{n}_k{k}_{f}_d_{df}' for n in MVN_NS for k in LOWRANK_KS if k <= n
                 for f, df in (('unbatched', 'full'), ('batched', 'full'), ('batched', 'bcast'))]}


def mvn_build(c):
    """K:(*bshape, n, n) SPD, d:(*bshape, n) or (n,), the upstream gradient g:(*bshape), in the case's dtype."""
    nb = max(1, math.prod(c.bshape))
    K = PB._spd64(c.n, nb).to(DT[c.dt]).reshape(*c.bshape, c.n, c.n).clone()
    g = _gen('mvn', c.n, c.bshape, c.dform)
    dshape = (c.n,) if c.dform == 'bcast' else (*c.bshape, c.n)
    d = torch.randn(dshape, generator=g, dtype=F32).to(DT[c.dt])
    up = (torch.rand(c.bshape, generator=g, dtype=F32) + 0.5).to(DT[c.dt])
    return dict(K=K, d=d, g=up)


def _dense_log_prob(K, d):
    n = K.shape[-1]
    db = d.expand(*K.shape[:-2], n)
    quad = (db * torch.linalg.solve(K, db.unsqueeze(-1)).squeeze(-1)).sum(-1)
    return -0.5 * (quad + torch.linalg.slogdet(K)[1] + n * LOG2PI)


def mvn_reference(c, data):
    """The float64 dense formula log N(d | 0, K) and its torch-autograd gradients under the upstream gradient g."""
    K, d = data['K'].double().requires_grad_(), data['d'].double().requires_grad_()
    lp = _dense_log_prob(K, d)
    gK, gd = torch.autograd.grad((lp * data['g'].double()).sum(), (K, d))
    return dict(lp=lp.detach(), gK=gK, gd=gd, kappa=float(torch.linalg.cond(K.detach()).max()))


def lowrank_build(c):
    """root:(*bshape, n, k), diag:(*bshape, n) > 0, d:(*bshape, n) or (n,), upstream g:(*bshape)."""
    g = _gen('lowrank', c.n, c.k, c.bshape, c.dform)
    root = torch.randn((*c.bshape, c.n, c.k), generator=g, dtype=F32) / math.sqrt(c.k)
    diag = torch.rand((*c.bshape, c.n), generator=g, dtype=F32) + 0.5
    d = torch.randn((c.n,) if c.dform == 'bcast' else (*c.bshape, c.n), generator=g, dtype=F32)
    up = torch.rand(c.bshape, generator=g, dtype=F32) + 0.5
    return {k: v.to(DT[c.dt]) for k, v in dict(root=root, diag=diag, d=d, g=up).items()}


def lowrank_reference(c, data):
    """The float64 DENSE formula on K = R R^T + diag(D) (not the Woodbury identity the product uses)."""
    root, diag, d = (data[k].double().requires_grad_() for k in ('root', 'diag', 'd'))
    K = root @ root.mT + torch.diag_embed(diag)
    lp = _dense_log_prob(K, d)
    groot, gdiag, gd = torch.autograd.grad((lp * data['g'].double()).sum(), (root, diag, d))
    return dict(lp=lp.detach(), groot=groot, gdiag=gdiag, gd=gd, kappa=float(torch.linalg.cond(K.detach()).max()))


# ================================================================================================================
# WhitenFn (through svgp.whiten)
# ================================================================================================================
WhitenCase = collections.namedtuple('WhitenCase', 'M groups chol_bwd_f64 passthrough pdt out_dtype')
KAPPA_CAP = 1e6
WHITEN_JITTER = 1e-4
WHITEN_MS = (64, 130)
# groups: name -> [(b, D, used by the loss)]
WHITEN_GROUPS = {'one': [(2, 2, True)], 'two': [(2, 3, True), (1, 2, True)], 'three_mid_unused': [(1, 2, True), (2, 3, False), (1, 1, True)]}
WHITEN_CASES = [WhitenCase(M, gr, cb, pt, pdt, od) for M in WHITEN_MS for gr in WHITEN_GROUPS for cb in (True, False)
                for pt in (False, True) for pdt in ('f64', 'f32') for od in (None, 'f32')]


def whiten_id(c):
    return (f'M{c.M}|{c.groups}|bwd{"64" if c.chol_bwd_f64 else "32"}|{"pass" if c.passthrough else "nopass"}|p{c.pdt}|'
            f'out{c.out_dtype or "64"}')


def whiten_path(c):
    """WhitenFn restated.  forward: parameters already float64 or copied; W32 from the factorisation's own launches when the
    layers want float32.  backward: the single-group shortcut takes the incoming gradient as Wbar when its dtype is W64's;
    otherwise the groups are placed in a batched buffer -- zero_() for a group nobody differentiated, a cast launch per
    float32 gradient, a multi-tensor copy for float64 ones --; the adjoint runs in float64 or float32; gradients return to
    the parameters' dtype; pass-through gradients are added."""
    groups = WHITEN_GROUPS[c.groups]
    tags = {f'M{c.M}', 'params_f64' if c.pdt == 'f64' else 'params_copied', 'out_f32' if c.out_dtype else 'out_f64',
            'adjoint_f64' if c.chol_bwd_f64 else 'adjoint_f32', f'groups_{len(groups)}'}
    if len(groups) == 1 and c.out_dtype is None:
        tags.add('wbar_is_gout')
    else:
        tags.add('wbar_batched')
        tags |= {'wbar_cast_f32' if c.out_dtype else 'wbar_foreach_copy'}
        if not all(u for _, _, u in groups):
            tags.add('wbar_zero_unused')
    if len({D for _, D, _ in groups}) > 1:
        tags.add('mixed_D')
    tags.add('grads_back_to_f32' if c.pdt == 'f32' else 'grads_stay_f64')
    tags.add('passthrough_added' if c.passthrough else 'no_passthrough')
    tags.add('cell_' + whiten_id(c))                                    # the table is the full cross of its six switches
    if c.passthrough and not all(u for _, _, u in groups):
        tags.add('unused_group_gets_passthrough_only')
    return tags


WHITEN_TAGS = {'M64', 'M130', 'params_f64', 'params_copied', 'out_f32', 'out_f64', 'adjoint_f64', 'adjoint_f32', 'groups_1',
               'groups_2', 'groups_3', 'wbar_is_gout', 'wbar_batched', 'wbar_cast_f32', 'wbar_foreach_copy', 'wbar_zero_unused',
               'mixed_D', 'grads_back_to_f32', 'grads_stay_f64', 'passthrough_added', 'no_passthrough',
               'unused_group_gets_passthrough_only'}
WHITEN_TAGS |= {f'cell_M{M}|{gr}|bwd{bw}|{pt}|p{pdt}|out{od}' for M in (64, 130) for gr in ('one', 'two', 'three_mid_unused')
                for bw in ('64', '32') for pt in ('pass', 'nopass') for pdt in ('f64', 'f32') for od in ('64', 'f32')}


@functools.lru_cache(maxsize=None)
def _whiten_inputs(M, groups, pdt):
    """Per group: Z on a lattice of spacing 1 jittered by +-0.2 (no two inducing points closer than 0.6, which is what
    keeps kappa down), ls in [0.7, 1.0], os in [0.5, 1.5]; Wbar (full, float32-representable) and the coefficients of
    the pass-through loss.  All rounded to float32 first, so that float32 and float64 parameters hold the same numbers."""
    out = []
    for gi, (b, D, used) in enumerate(WHITEN_GROUPS[groups]):
        g = _gen('whiten', M, groups, gi)
        side = math.ceil(M ** (1.0 / D))
        lattice = torch.tensor(list(itertools.product(range(side), repeat=D)), dtype=F32)
        Z = torch.stack([lattice[torch.randperm(len(lattice), generator=g)[:M]] for _ in range(b)])
        Z = Z + 0.4 * (torch.rand(Z.shape, generator=g) - 0.5)
        ls = 0.7 + 0.3 * torch.rand(b, D, generator=g)
        os_ = 0.5 + torch.rand(b, generator=g)
        Wbar = torch.randn(b, M, M, generator=g)
        coef = tuple(torch.randn(t.shape, generator=g) for t in (Z, ls, os_))
        out.append(dict(Z=Z.to(DT[pdt]), ls=ls.to(DT[pdt]), os=os_.to(DT[pdt]), Wbar=Wbar, coef=coef, used=used))
    return out


def whiten_build(c):
    return _whiten_inputs(c.M, c.groups, c.pdt)


def _kzz(Z, ls, os_, jitter):
    z = Z / ls.unsqueeze(-2)
    d2 = (z.unsqueeze(-2) - z.unsqueeze(-3)).pow(2).sum(-1)
    return os_[:, None, None] * torch.exp(-0.5 * d2) + jitter * torch.eye(Z.shape[-2], dtype=Z.dtype)


@functools.lru_cache(maxsize=None)
def _whiten_reference(M, groups, pdt, passthrough):
    out = []
    for grp in _whiten_inputs(M, groups, pdt):
        Z, ls, os_ = (grp[k].double().requires_grad_() for k in ('Z', 'ls', 'os'))
        K = _kzz(Z, ls, os_, WHITEN_JITTER)
        W = torch.linalg.solve_triangular(torch.linalg.cholesky(K), torch.eye(M, dtype=F64).expand_as(K), upper=False)
        loss = (W * torch.tril(grp['Wbar'].double())).sum() if grp['used'] else W.sum() * 0.0
        if passthrough:
            loss = loss + sum((p * cf.double()).sum() for p, cf in zip((Z, ls, os_), grp['coef']))
        gZ, gls, gos = torch.autograd.grad(loss, (Z, ls, os_))
        out.append(dict(W=W.detach(), gZ=gZ, gls=gls, gos=gos, kappa=float(torch.linalg.cond(K.detach()).max())))
    return out


def whiten_reference(c):
    """Per group: W = inv(cholesky(os RBF(Z, Z; ls) + jitter I)) in float64, the torch-autograd gradients of
    sum_used sum(W o tril(Wbar)) [+ sum_all sum(coef o (Z, ls, os)) with passthrough], and kappa_2 of the Gram matrix."""
    return _whiten_reference(c.M, c.groups, c.pdt, c.passthrough)


def whiten_kappa(c):
    return max(r['kappa'] for r in whiten_reference(c))


# ================================================================================================================
# Wrapper contracts of the kernel and loss nodes (values and kernel gradients are held elsewhere: only what the
# torch.autograd.Function wrappers add -- needs_input_grad, layouts of G, host scalars, shared inputs, 1-D forms)
# ================================================================================================================
WrapCase = collections.namedtuple('WrapCase', 'node variant')
WRAP_N, WRAP_D, WRAP_BATCH = 33, 2, 3
GIBBS_OS = ('float', 'tensor', 'none')
GIBBS_DIAG = ('none', 'float', 'tensor')
WRAP_CASES = (
    [WrapCase('gibbs', f'os_{o}|diag_{d}|G{lay}') for (o, d), lay in zip(itertools.product(GIBBS_OS, GIBBS_DIAG),
                                                                       itertools.cycle(MM_LAYOUTS))] +
    [WrapCase(node, 'subsets') for node in ('gibbs', 'rbf', 'matern', 'rbf_periodic', 'ps2d')] +
    [WrapCase('rbf', f'{v}|G{lay}') for v, lay in (('shared_x1', 'trans'), ('shared_x2', 'expand'), ('shared_both', 'contig'))] +
    [WrapCase('kl_whitened', 'm_1d'), WrapCase('kl_whitened_total', 'm_1d'), WrapCase('kl_whitened_total', 'm_1d|addin'),
     WrapCase('gauss_ell', 'noise_fixed'), WrapCase('gauss_ell_total', 'noise_fixed')])
# the tensor inputs of each kernel node, in apply() order, whose every needs_input_grad subset the 'subsets' rows run
WRAP_TENSOR_INPUTS = {'gibbs': ('x1', 'x2', 'ell1', 'ell2', 'outputscale', 'diag_add'), 'rbf': ('x1', 'x2', 'ls', 'os'),
                      'matern': ('x1', 'x2', 'ls', 'os'), 'rbf_periodic': ('x1', 'x2', 'ls_rbf', 'ls_per', 'period', 'os'),
                      'ps2d': ('s1', 's2')}


def wrap_id(c):
    return f'{c.node}|{c.variant}'


def wrap_path(c):
    """What the wrapper of the row's node does beyond calling its kernels."""
    v = c.variant.split('|')
    tags = {f'{c.node}:{t}' for t in v if not t.startswith('G')} | {f'G_{t[1:]}' for t in v if t.startswith('G')}
    if c.node == 'gibbs' and v[0].startswith('os_'):
        tags |= {'gibbs:os_in_ctx' if v[0] == 'os_float' else 'gibbs:os_saved',
                 'gibbs:g_diag' if v[1] == 'diag_tensor' else 'gibbs:no_g_diag'}
    if c.node == 'rbf' and v[0].startswith('shared'):
        tags.add('sum_shared')
    if c.node.startswith(('kl', 'gauss')):
        tags.add('upstream_g_not_one')
    return tags


WRAP_TAGS = ({f'gibbs:os_{o}' for o in GIBBS_OS} | {f'gibbs:diag_{d}' for d in GIBBS_DIAG} |
             {'gibbs:os_in_ctx', 'gibbs:os_saved', 'gibbs:g_diag', 'gibbs:no_g_diag', 'sum_shared', 'upstream_g_not_one'} |
             {f'{n}:subsets' for n in WRAP_TENSOR_INPUTS} | {f'G_{x}' for x in MM_LAYOUTS} |
             {'rbf:shared_x1', 'rbf:shared_x2', 'rbf:shared_both', 'kl_whitened:m_1d', 'kl_whitened_total:m_1d',
              'kl_whitened_total:addin', 'gauss_ell:noise_fixed', 'gauss_ell_total:noise_fixed'})


def wrap_inputs(node):
    """float64 CPU inputs of a node's rows, by name."""
    g = _gen('wrap', node)
    n, D, b = WRAP_N, WRAP_D, WRAP_BATCH
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)             # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g, dtype=F64)              # noqa: E731
    if node == 'gibbs':
        return dict(x1=rn(n, D), x2=rn(n, D), ell1=0.5 + ru(D, n), ell2=0.5 + ru(D, n), outputscale=torch.tensor(0.644, dtype=F64),
                    diag_add=torch.tensor(0.011, dtype=F64), G=rn(n, n))
    if node in ('rbf', 'matern'):
        return dict(x1=rn(b, n, D), x2=rn(b, n + 4, D), ls=0.7 + ru(b, D), os=0.5 + ru(b), G=rn(b, n, n + 4))
    if node == 'rbf_periodic':
        return dict(x1=rn(b, n, D), x2=rn(b, n + 4, D), ls_rbf=0.7 + ru(b, D), ls_per=0.7 + ru(b), period=1.0 + ru(b),
                    os=0.5 + ru(b), G=rn(b, n, n + 4))
    if node == 'ps2d':
        def spd(k):
            a = rn(k, 2, 2)
            return a @ a.mT + 0.5 * torch.eye(2, dtype=F64)
        return dict(x1=rn(n, 2), x2=rn(n + 4, 2), s1=spd(n), s2=spd(n + 4), G=rn(n, n + 4))
    if node.startswith('kl'):
        M = 65
        return dict(m=0.3 * rn(M), Lq=torch.tril(0.1 * rn(M, M)) + torch.eye(M, dtype=F64), addin=rn(()), g=torch.tensor(1.7, dtype=F64))
    if node.startswith('gauss'):
        S = 3
        return dict(y=rn(n), mu=rn(S, n), v=0.2 + ru(S, n), noise=torch.tensor([0.37], dtype=F64), g=0.5 + ru(S))
    raise KeyError(node)


def gibbs_dense(x1, x2, ell1, ell2, outputscale=None, diag_add=None):
    """os prod_d sqrt(2 l1 l2 / (l1^2 + l2^2)) exp(-sum_d (x1 - x2)^2 / (l1^2 + l2^2)) + diag_add I;  ell:(D,n)."""
    s = ell1.unsqueeze(-1) ** 2 + ell2.unsqueeze(-2) ** 2                              # (D, n1, n2)
    pre = torch.sqrt(2 * ell1.unsqueeze(-1) * ell2.unsqueeze(-2) / s).prod(0)
    diff2 = (x1.T.unsqueeze(-1) - x2.T.unsqueeze(-2)) ** 2
    K = pre * torch.exp(-(diff2 / s).sum(0))
    if outputscale is not None:
        K = K * outputscale
    if diag_add is not None:
        K = K + diag_add * torch.eye(K.shape[0], dtype=K.dtype)
    return K


def rbf_dense(x1, x2, ls, os_):
    """os[b] exp(-0.5 |(x1 - x2) / ls[b]|^2); x shared (n,D) or per batch (b,n,D)."""
    a, c = x1 / ls.unsqueeze(-2), x2 / ls.unsqueeze(-2)
    return os_[:, None, None] * torch.exp(-0.5 * (a.unsqueeze(-2) - c.unsqueeze(-3)).pow(2).sum(-1))


def kl_whitened_dense(m, Lq):
    """KL(N(m, L L^T) || N(0, I)) with L = tril(Lq)."""
    L = torch.tril(Lq)
    return 0.5 * ((m * m).sum() + (L * L).sum() - m.numel() - 2.0 * torch.log(torch.diagonal(L)).sum())


def gauss_ell_dense(y, mu, v, noise, scale):
    """(S,): scale sum_i E_{N(mu, v)} log N(y_i | f, noise)."""
    return scale * (-0.5 * torch.log(2 * math.pi * noise) - ((y - mu) ** 2 + v) / (2 * noise)).sum(-1)


def with_layout(G, layout):
    """A tensor of G's values (ones for 'expand') whose strides are the layout's."""
    if layout == 'trans':
        return G.mT.contiguous().mT
    if layout == 'expand':
        return torch.ones((), dtype=G.dtype, device=G.device).expand(G.shape)
    return G.contiguous()


# ================================================================================================================
# float32 forms of the Cholesky nodes: no constant existed.  Largest max|got - ref| / max|ref| measured on an MI355X
# against the float64 reference of the SAME float32 inputs, per node, quantity and size (the case that set it, its kappa_2);
# a row's bound is F32_BOUND_FACTOR times the figure of its own size.  The errors turned out NOT to follow n kappa u:
# from n = 1 to n = 200 they grow 5 to 30-fold (values of the log-densities not at all) while n kappa grows 1800-fold, so
# a bound scaled by n kappa u would be loose by orders of magnitude at every size but the smallest
# (tests/test_autograd_cases_cpu.py checks that no figure grows FASTER than n kappa u from the smallest size on).
# ================================================================================================================
F32_BOUND_FACTOR = 3.0
F32_MEASURED = {
    ('chol_inv', 'value'): {1: 2.3e-8,      # f32|n1|b0 W, kappa 1
                            7: 1.44e-7,     # f32|n7|b3 W, kappa 7.6
                            64: 3.19e-7,    # f32|n64|b3 W, kappa 8.7
                            65: 3.52e-7,    # f32|n65|b3 W, kappa 8.6
                            130: 4.65e-7,   # f32|n130|b3 W, kappa 8.7
                            200: 6.49e-7},  # f32|n200|b0 W, kappa 9.1
    ('chol_inv', 'grad'): {1: 1.1e-7,       # f32|n1|b3 gK, kappa 1
                           7: 2.01e-7,      # f32|n7|b0 gK, kappa 7.0
                           64: 6.52e-7,     # f32|n64|b3 gK, kappa 8.7
                           65: 8.43e-7,     # f32|n65|b3 gK, kappa 8.6
                           130: 9.19e-7,    # f32|n130|b0 gK, kappa 8.3
                           200: 1.2e-6},    # f32|n200|b3 gK, kappa 9.0
    ('mvn', 'value'): {1: 8.52e-8,          # f32|n1|batch2x2|d_full lp, kappa 1
                       65: 8.22e-8,         # f32|n65|batch2x2|d_bcast lp, kappa 8.9
                       200: 7.78e-8},       # f32|n200|batch3|d_bcast lp, kappa 9.0
    ('mvn', 'grad'): {1: 5.52e-7,           # f32|n1|batch2x2|d_bcast gK, kappa 1
                      65: 9.85e-7,          # f32|n65|batch2x2|d_bcast gK, kappa 8.9
                      200: 2.31e-6},        # f32|n200|batch3|d_bcast gK, kappa 9.0
    ('lowrank', 'value'): {1: 1.23e-7,      # f32|n1|k1|batch3|d_full lp, kappa 1
                           65: 9.13e-8,     # f32|n65|k1|batch3|d_bcast lp, kappa 161
                           200: 6.93e-8},   # f32|n200|k64|batch3|d_bcast lp, kappa 15
    ('lowrank', 'grad'): {1: 6.84e-7,       # f32|n1|k1|batch3|d_full gd, kappa 1
                          65: 1.14e-6,      # f32|n65|k64|batch3|d_bcast groot, kappa 7.2
                          200: 9.44e-7},    # f32|n200|k64|batch-|d_full groot, kappa 16
    # chol_bwd_f64=False: the whitening adjoint's three products and the kernel backward in float32, by M
    ('whiten_bwd32', 'grad'): {64: 3.16e-5,     # M64|three_mid_unused|bwd32|pass|pf64|out64 gos[2]: its group's kappa 26
                               130: 1.57e-5},   # M130|two|bwd32|pass|pf64|out64 gos[1]: its group's kappa 281
}


def f32_bound(node, quantity, n):
    return F32_BOUND_FACTOR * F32_MEASURED[(node, quantity)][n]


def f32_kappa_by_size(node):
    """{n: largest kappa_2 among the node's float32 rows of that size} -- what the growth check sets the figures against."""
    out = collections.defaultdict(float)
    if node == 'chol_inv':
        for c in CHOL_CASES:
            out[c.n] = max(out[c.n], chol_reference(c)['kappa'])
    elif node == 'mvn':
        for c in MVN_CASES:
            out[c.n] = max(out[c.n], mvn_reference(c, mvn_build(c))['kappa'])
    elif node == 'lowrank':
        for c in LOWRANK_CASES:
            out[c.n] = max(out[c.n], lowrank_reference(c, lowrank_build(c))['kappa'])
    else:
        for c in WHITEN_CASES:
            out[c.M] = max(out[c.M], whiten_kappa(c))
    return dict(out)


# ================================================================================================================
# SVGPLayerFn and SVGPMeanFieldLayerFn (through svgp.svgp_marginal, the entry the models use)
# ================================================================================================================
LayerCase = collections.namedtuple('LayerCase', 'q dt cfg shape x_mode x_grad mean kzx_f64')    # q: 'chol' | 'diag'
# cfg -> the settings context managers (nsgp.gp.settings) entered around the call, by name
LAYER_CFG = {
    'default': {},                                                         # int8 digit planes (4; 5 for kzx_f64)
    'no_i8': {'whiten_matmul_i8': False},                                  # f64acc; kzx_f64: f64acc_b64 + f64acc_t
    'no_i8_var32': {'whiten_matmul_i8': False, 'hidden_var_f64': False},   # kzx_f64: f64acc_b64 + f32
    'no_w64': {'whiten_matmul_f64': False},                                # f32
    'fused': {'fuse_kzx': True},                                           # kzx_fused
    'bf16': {'forward_precision': 'bf16'},                                 # i8 + bf16
    'bf16_no_i8': {'forward_precision': 'bf16', 'whiten_matmul_i8': False},  # f64acc + bf16
    'bf16_all': {'forward_precision': 'bf16_all'},                         # bf16 + bf16
}
LAYER_SHAPES = {'A': (2, 64, 96, 2), 'B': (1, 130, 333, 3), 'T': (2, 128, 128, 3)}      # (b, M, n, D); T: whole tiles
# (x shared by the GPs or one per GP, x requires grad, affine prior mean, the layer feeds the next one)
LAYER_VARIANTS = (('shared', False, 'none', False), ('per_gp', True, 'w', False), ('shared', True, 'none', False),
                  ('per_gp', False, 'c', False), ('shared', True, 'wc', True))
LAYER_JITTER = 1e-4
LAYER_VAR_JITTER = 1e-4


def _layer_table():
    out = []
    V = LAYER_VARIANTS
    for q in ('chol', 'diag'):
        for cfg in ('default', 'no_i8', 'no_w64'):
            out += [LayerCase(q, 'f32', cfg, s, *v) for s in ('A', 'B') for v in V]
        out += [LayerCase(q, 'f32', 'no_i8_var32', 'A', *V[4])]
        out += [LayerCase(q, 'f32', 'fused', 'T', *v) for v in V]
        out += [LayerCase(q, 'f32', cfg, 'A', *v) for cfg in ('bf16', 'bf16_no_i8', 'bf16_all') for v in V]
        out += [LayerCase(q, 'f64', 'default', s, *v) for s in ('A', 'B') for v in V]
    return out


LAYER_CASES = _layer_table()


def layer_id(c):
    return (f'{c.q}|{c.dt}|{c.cfg}|{c.shape}|x_{c.x_mode}{"_grad" if c.x_grad else ""}|mean_{c.mean}' +
            ('|kzx_f64' if c.kzx_f64 else ''))


def layer_select(c):
    """nsgp.svgp.select_projection restated for the case: (first, second, int8 Kzx planes).  svgp_marginal runs its own
    whitening chain, so a float32 layer always has the float64 W at hand."""
    s = dict(forward_precision='f32', whiten_matmul_f64=True, whiten_matmul_i8=True, fuse_kzx=False, hidden_var_f64='auto')
    s.update(LAYER_CFG[c.cfg])
    b, M, n, D = LAYER_SHAPES[c.shape]
    fp, f32 = s['forward_precision'], c.dt == 'f32'
    w64 = f32 and (s['whiten_matmul_f64'] or fp == 'bf16_all')
    fuse = fp == 'f32' and s['fuse_kzx'] and w64 and D <= 4 and M % 128 == 0 and n % 128 == 0      # whole tiles
    i8 = fp in ('f32', 'bf16') and not fuse and w64 and s['whiten_matmul_i8'] and D <= 4 and M <= 4096
    can64 = c.kzx_f64 and fp == 'f32' and w64 and not fuse
    var64 = can64 and ((n <= 8192) if s['hidden_var_f64'] == 'auto' else bool(s['hidden_var_f64']))
    bf16 = f32 and fp in ('bf16', 'bf16_all') and M % 8 == 0
    first = 'bf16' if (bf16 and fp == 'bf16_all') else 'kzx_fused' if fuse else 'i8' if i8 else \
        'f64acc_b64' if can64 else 'f64acc' if w64 else 'f32'
    second = 'diag' if c.q == 'diag' else 'bf16' if bf16 else 'f64acc_t' if var64 else 'f32'
    return first, second, 5 if (c.kzx_f64 and not bf16) else 4


def layer_path(c):
    """The layer nodes restated: the projection pair, where the backward's Kzx comes from, and what happens to gx."""
    first, second, planes = layer_select(c)
    b = LAYER_SHAPES[c.shape][0]
    tags = {f'{c.dt}:first_{first}', f'second_{second}', f'shape_{c.shape}', 'mean_' + c.mean}
    if first == 'i8':
        tags |= {f'i8_planes_{planes}', 'kzx_from_i8_build'}
    elif first in ('kzx_fused', 'f64acc_b64') or (c.q == 'chol' and second == 'f64acc_t') or (c.q == 'diag' and first == 'bf16'):
        tags.add('kzx_built_in_backward')
    else:
        tags.add('kzx_saved')
    if c.x_grad:
        tags.add('gx_sum0' if (c.x_mode == 'shared' and b > 1) else 'gx_index0' if c.x_mode == 'shared' else 'gx_per_gp')
        tags.add('gx_mean_w_term' if 'w' in c.mean else 'gx_no_mean_w')
    else:
        tags.add('gx_none')
    if c.kzx_f64:
        tags.add('kzx_f64')
    tags.add(f'{c.dt}:{first}+{second}/{LAYER_VARIANTS.index(tuple(c[4:]))}')      # every pair with every variant
    if c.shape == 'B':
        tags.add(f'{c.dt}:{first}+{second}/{LAYER_VARIANTS.index(tuple(c[4:]))}@B')
    if c.kzx_f64 and second in ('bf16', 'diag') and LAYER_CFG[c.cfg].get('forward_precision', 'f32') != 'f32':
        tags.add('kzx_f64_dropped_under_bf16')                           # no float64 Kzx / variance, four int8 planes
    return {f'{c.q}/{t}' for t in tags}


LAYER_TAGS = {f'{q}/{t}' for q in ('chol', 'diag') for t in (
    ['f32:first_' + f for f in ('f32', 'f64acc', 'i8', 'kzx_fused', 'f64acc_b64', 'bf16')] + ['f64:first_f32'] +
    ['i8_planes_4', 'i8_planes_5', 'kzx_from_i8_build', 'kzx_built_in_backward', 'kzx_saved', 'gx_sum0', 'gx_index0', 'gx_per_gp',
     'gx_mean_w_term', 'gx_no_mean_w', 'gx_none', 'kzx_f64', 'mean_none', 'mean_w', 'mean_c', 'mean_wc',
     'shape_A', 'shape_B', 'shape_T'])}
LAYER_TAGS |= {'chol/second_' + s for s in ('f32', 'f64acc_t', 'bf16')} | {'diag/second_diag'}
# (first, second of the Cholesky node) -> the variants (indices into LAYER_VARIANTS) it is run with; 4 is the kzx_f64 one
_LAYER_PAIRS = {('f32:i8', 'f32'): (0, 1, 2, 3), ('f32:i8', 'f64acc_t'): (4,), ('f32:f64acc', 'f32'): (0, 1, 2, 3), ('f32:f64acc_b64', 'f64acc_t'): (4,),
                ('f32:f64acc_b64', 'f32'): (4,), ('f32:f32', 'f32'): (0, 1, 2, 3, 4), ('f32:kzx_fused', 'f32'): (0, 1, 2, 3, 4),
                ('f32:i8', 'bf16'): (0, 1, 2, 3, 4), ('f32:f64acc', 'bf16'): (0, 1, 2, 3, 4), ('f32:bf16', 'bf16'): (0, 1, 2, 3, 4),
                ('f64:f32', 'f32'): (0, 1, 2, 3, 4)}
LAYER_TAGS |= {f'chol/{f}+{s}/{v}' for (f, s), vs in _LAYER_PAIRS.items() for v in vs}
LAYER_TAGS |= {f'diag/{f}+diag/{v}' for f in {f for f, _ in _LAYER_PAIRS}
               for v in sorted(set().union(*(vs for (f2, _), vs in _LAYER_PAIRS.items() if f2 == f)))}
# the ragged shape B runs every variant of the configurations whose kernels take ragged tiles (default, no_i8, no_w64, float64)
_LAYER_PAIRS_B = {('f32:i8', 'f32'): (0, 1, 2, 3), ('f32:i8', 'f64acc_t'): (4,), ('f32:f64acc', 'f32'): (0, 1, 2, 3),
                  ('f32:f64acc_b64', 'f64acc_t'): (4,), ('f32:f32', 'f32'): (0, 1, 2, 3, 4), ('f64:f32', 'f32'): (0, 1, 2, 3, 4)}
LAYER_TAGS |= {f'chol/{f}+{s}/{v}@B' for (f, s), vs in _LAYER_PAIRS_B.items() for v in vs}
LAYER_TAGS |= {f'diag/{f}+diag/{v}@B' for (f, _), vs in _LAYER_PAIRS_B.items() for v in vs}
LAYER_TAGS |= {'chol/kzx_f64_dropped_under_bf16', 'diag/kzx_f64_dropped_under_bf16'}


@functools.lru_cache(maxsize=None)
def _layer_inputs(q, shape, x_mode, mean):
    """float32-representable inputs (held in float64): Z on the jittered lattice of the whitening cases, x uniform over the
    lattice's box, q(u) near the prior, the weights gm, gv of the loss sum(mean o gm) + sum(var o gv)."""
    b, M, n, D = LAYER_SHAPES[shape]
    g = _gen('layer', shape, x_mode, mean)
    side = math.ceil(M ** (1.0 / D))
    lattice = torch.tensor(list(itertools.product(range(side), repeat=D)), dtype=F32)
    Z = torch.stack([lattice[torch.randperm(len(lattice), generator=g)[:M]] for _ in range(b)])
    Z = Z + 0.4 * (torch.rand(Z.shape, generator=g) - 0.5)
    d = dict(Z=Z, ls=0.7 + 0.3 * torch.rand(b, D, generator=g), os=0.5 + torch.rand(b, generator=g),
             x=(side - 1) * torch.rand((n, D) if x_mode == 'shared' else (b, n, D), generator=g),
             m=0.3 * torch.randn(b, M, generator=g), gm=torch.randn(b, n, generator=g), gv=torch.randn(b, n, generator=g))
    if q == 'chol':
        d['Lq'] = torch.tril(0.1 * torch.randn(b, M, M, generator=g)) + torch.eye(M)
    else:
        d['s2'] = 0.5 + torch.rand(b, M, generator=g)
    if 'w' in mean:
        d['mean_w'] = torch.randn((D,) if x_mode == 'shared' else (b, D), generator=g)
    if 'c' in mean:
        d['mean_c'] = torch.randn((1,) if x_mode == 'shared' else (b,), generator=g)
    return {k: v.double() for k, v in d.items()}


def layer_build(c):
    return _layer_inputs(c.q, c.shape, c.x_mode, c.mean)


LAYER_LEAVES = ('x', 'Z', 'ls', 'os', 'm', 'Lq', 's2', 'mean_w', 'mean_c')


@functools.lru_cache(maxsize=None)
def _layer_reference(q, shape, x_mode, mean):
    d = _layer_inputs(q, shape, x_mode, mean)
    b, M, n, D = LAYER_SHAPES[shape]
    t = {k: d[k].clone().requires_grad_() for k in LAYER_LEAVES if k in d}
    xb = t['x'] if x_mode == 'per_gp' else t['x'].unsqueeze(0).expand(b, n, D)
    K = _kzz(t['Z'], t['ls'], t['os'], LAYER_JITTER)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(K), rbf_dense(t['Z'], xb, t['ls'], t['os']), upper=False)
    mu = torch.einsum('bkj,bk->bj', A, t['m'])
    if 'mean_w' in t:
        mu = mu + (xb * t['mean_w'].reshape(-1, 1, D)).sum(-1)
    if 'mean_c' in t:
        mu = mu + t['mean_c'].reshape(-1, 1)
    base = t['os'].unsqueeze(-1) + LAYER_VAR_JITTER
    if q == 'chol':
        C = torch.tril(t['Lq']).mT @ A
        var = base + (C * C).sum(1) - (A * A).sum(1)
    else:
        var = base + ((t['s2'] - 1.0).unsqueeze(-1) * A * A).sum(1)
    grads = torch.autograd.grad((mu * d['gm']).sum() + (var * d['gv']).sum(), list(t.values()))
    return dict(mean=mu.detach(), var=var.detach(), kappa=float(torch.linalg.cond(K.detach()).max()),
                grads=dict(zip(t.keys(), grads)))


def layer_reference(c):
    """The whitened SVGP marginals by the dense float64 formulas (Cholesky of Kzz + jitter I, a triangular solve) and the
    torch-autograd gradients of sum(mean o gm) + sum(var o gv) with respect to every input; shared, read-only."""
    return _layer_reference(c.q, c.shape, c.x_mode, c.mean)
