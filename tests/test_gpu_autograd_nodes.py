"""The torch.autograd.Function nodes (nsgp/ops.py, nsgp/gp/distributions.py, nsgp/svgp.py) against float64 torch autograd
of the dense formulas (tests/autograd_cases.py): every backward product, structure flag, operand order, reduction and
`None` the nodes choose on the host.  MatmulFn is compared bit for bit on integer data, first and second order; the
Cholesky nodes within the constants the suite already holds in float64, and within 3x the error measured at each size
(AC.F32_MEASURED) where it held none.  Run with -s for the achieved errors, the file's wall time and its slowest ids."""
import itertools
import time

import pytest
import torch

import autograd_cases as AC
from conftest import measured
from test_gpu_svgp import F32_GRAD_TOL, F32_VALUE_TOL

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64

# float64 Cholesky nodes: the constants of tests/test_gpu_kernels.py::test_chol_inv_autograd
CHOL64_VALUE = dict(rtol=1e-9, atol=1e-10)
CHOL64_GRAD = dict(rtol=1e-8, atol=1e-9)
# a float64 gradient handed back in float32 parameters is rounded once more: 2^-24 relative on top of CHOL64_GRAD
CHOL64_GRAD_TO_F32 = dict(rtol=1e-8 + 2.0 ** -24, atol=1e-9)
W64_TO_F32 = dict(rtol=2.0 ** -24 + 1e-9, atol=1e-10)     # the float32 copy of a float64 W: one rounding
# The float32 forms of these nodes had no constant: a row's bound is 3x the largest max-norm relative error measured on an
# MI355X among the rows of its own size, against the float64 reference of the same float32 inputs -- the tables
# AC.F32_MEASURED, with the case that set each figure and its kappa (AC.f32_bound).
# wrapper rows (float64 kernels, n = 33): a float64 kernel gradient is a sum of at most 3 x 37 terms of size <= max|ref|
WRAP64 = dict(rtol=1e-9, atol=1e-11)
# the same float64 kernel with another needs_input_grad subset may sum in another order: n u, far below this
SUBSET64 = dict(rtol=1e-10, atol=1e-12)

# layer nodes: the constants of tests/test_gpu_svgp.py (float64: its rtol 1e-9 / atol 1e-10 on the marginals and 1e-7
# max-norm relative on the gradients; float32: F32_VALUE_TOL, F32_GRAD_TOL)
LAYER64_VALUE = dict(rtol=1e-9, atol=1e-10)
LAYER64_GRAD = 1e-7
# C = Lq^T A on the bf16 cores: the mean is the float32 path's; tests/test_gpu_bf16.py bounds what the variance moves by 5e-2
BF16_VAR_TOL = 5e-2
# gradients of a float32 backward on the bf16 forward's C, and everything of 'bf16_all' (A on the bf16 cores too, which
# test_gpu_bf16.py only requires to be finite): no constant existed -- max-norm relative errors measured on an MI355X over
# the rows of each (first, second) pair, with the row that set the figure; the bound is 3x.
BF16_MEASURED = {
    ('i8', 'bf16'): dict(grad=0.0137),          # chol|f32|bf16|A|x_per_gp_grad|mean_w g_ls, kappa 856 (variance: 0.0094)
    ('f64acc', 'bf16'): dict(grad=0.0137),      # chol|f32|bf16_no_i8|A|x_per_gp_grad|mean_w g_ls, kappa 856
    # chol|f32|bf16_all|A: x_shared|mean_none mean (kappa 146), x_per_gp_grad|mean_w var and g_ls (kappa 856)
    ('bf16', 'bf16'): dict(mean=0.00929, var=0.0116, grad=0.0169),
    # diag|f32|bf16_all|A: x_shared|mean_none mean (kappa 146), x_per_gp|mean_c var (kappa 185), x_per_gp_grad|mean_w g_m (kappa 856)
    ('bf16', 'diag'): dict(mean=0.00929, var=0.00439, grad=0.0151),
}

_TIMES = {}
_T0 = []


@pytest.fixture(autouse=True)
def _timed(request):
    t = time.perf_counter()
    if not _T0:
        _T0.append(t)
    yield
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    _TIMES[request.node.name] = time.perf_counter() - t


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nsgp import ops as _ops
    return _ops


def _maxnorm(name, got, ref, bound):
    """max|got - ref| / max|ref| against a bound; prints both."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    err = float((got - ref).abs().max()) / (float(ref.abs().max()) + 1e-300)
    print(f'[measured] {name}: max-norm rel err {err:.3g} (bound {bound:.3g})')
    return err <= bound


def _finite(*ts):
    return all(t is None or bool(torch.isfinite(t).all()) for t in ts)


# ---------------------------------------------------------------------------------------------------------------- MatmulFn
@pytest.mark.parametrize('c', AC.MATMUL_CASES, ids=AC.matmul_id)
def test_matmul_node_is_exact_to_second_order(ops, c):
    d = AC.matmul_build(c)
    ref = AC.matmul_reference(c, d)
    A, B = d['A_st'].cuda().requires_grad_(), d['B_st'].cuda().requires_grad_()
    flags = dict(a_lower='a' in c.lower, b_lower='b' in c.lower, out_lower='o' in c.lower)
    C = ops.matmul(A, B, c.ta, c.tb, **flags)
    if c.layout == 'expand':                                # the stride-0 gradient .sum() sends
        Gleaf = None
        gA, gB = torch.autograd.grad(C.sum(), (A, B), create_graph=True)
    else:
        if c.layout == 'trans':
            Gleaf = d['G_st'].mT.contiguous().cuda().requires_grad_()
            G = Gleaf.mT
        else:
            Gleaf = G = d['G_st'].cuda().requires_grad_()
        assert G.is_contiguous() == (c.layout == 'contig') or 1 in G.shape[-2:]
        gA, gB = torch.autograd.grad(C, (A, B), grad_outputs=G, create_graph=True)
    assert gA.shape == A.shape and gB.shape == B.shape
    second = torch.autograd.grad((gA * d['H_st'].cuda()).sum(), (B,) if Gleaf is None else (B, Gleaf))
    gB2 = second[0]
    gG2 = None if Gleaf is None else (second[1].mT if c.layout == 'trans' else second[1])
    got = dict(C=C, gA=gA, gB=gB, gB2=gB2, gG2=gG2)
    assert _finite(*got.values()), [k for k, v in got.items() if not _finite(v)]
    for k, v in got.items():
        if v is not None:
            assert v.dtype == AC.DT[c.dt] and v.shape == ref[k].shape, k
            assert torch.equal(v.detach().cpu().double(), ref[k]), (k, float((v.detach().cpu().double() - ref[k]).abs().max()))
    # the gradient of an operand stored lower is exactly zero above its diagonal
    for low, gs in (('a', (gA,)), ('b', (gB, gB2)), ('o', (gG2,))):
        for t in gs:
            if low in c.lower and t is not None:
                assert float(torch.triu(t.detach(), 1).abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------- CholInvFn
@pytest.mark.parametrize('c', AC.CHOL_CASES, ids=AC.chol_id)
def test_chol_inv_node(ops, c):
    d, ref = AC.chol_build(c), AC.chol_reference(c)
    K = d['K'].cuda().requires_grad_()
    W, info = ops.chol_inv(K)
    assert not info.requires_grad and info.cpu().tolist() == [0] * max(c.batch, 1)
    Wbar = AC.with_layout(d['Wbar'].cuda(), c.layout)
    (gK,) = torch.autograd.grad(W, K, grad_outputs=Wbar)
    Wr, gr = ref['W'], ref['gK']
    assert gK.shape == K.shape and float(torch.triu(W.detach(), 1).abs().max() if c.n > 1 else 0.0) == 0.0
    name = f'chol_inv {AC.chol_id(c)} kappa {ref["kappa"]:.3g}'
    if c.dt == 'f64':
        ok = [measured(name + ' W', W, Wr, **CHOL64_VALUE), measured(name + ' gK', gK, gr, **CHOL64_GRAD)]
    else:
        ok = [_maxnorm(name + ' W', W, Wr, AC.f32_bound('chol_inv', 'value', c.n)),
              _maxnorm(name + ' gK', gK, gr, AC.f32_bound('chol_inv', 'grad', c.n))]
    assert all(ok), ok


# ------------------------------------------------------------------------------------------- MvnLogProbFn and the low rank
@pytest.mark.parametrize('c', AC.MVN_CASES, ids=AC.mvn_id)
def test_mvn_log_prob_node(ops, c):
    from nsgp.gp.distributions import MvnLogProbFn
    d = AC.mvn_build(c)
    ref = AC.mvn_reference(c, d)
    K, dv = d['K'].cuda().requires_grad_(), d['d'].cuda().requires_grad_()
    lp, info = MvnLogProbFn.apply(K, dv)
    assert lp.shape == c.bshape and not info.requires_grad and int(info.abs().max()) == 0
    gK, gd = torch.autograd.grad(lp, (K, dv), grad_outputs=d['g'].cuda())
    assert gK.shape == K.shape and gd.shape == dv.shape
    name = f'mvn {AC.mvn_id(c)} kappa {ref["kappa"]:.3g}'
    if c.dt == 'f64':
        ok = [measured(name + ' lp', lp, ref['lp'], **CHOL64_VALUE), measured(name + ' gK', gK, ref['gK'], **CHOL64_GRAD),
              measured(name + ' gd', gd, ref['gd'], **CHOL64_GRAD)]
    else:
        gb = AC.f32_bound('mvn', 'grad', c.n)
        ok = [_maxnorm(name + ' lp', lp, ref['lp'], AC.f32_bound('mvn', 'value', c.n)), _maxnorm(name + ' gK', gK, ref['gK'], gb),
              _maxnorm(name + ' gd', gd, ref['gd'], gb)]
    assert all(ok), ok


@pytest.mark.parametrize('c', AC.LOWRANK_CASES, ids=AC.lowrank_id)
def test_lowrank_diag_log_prob(ops, c):
    from nsgp.gp.distributions import _lowrank_diag_log_prob
    d = AC.lowrank_build(c)
    ref = AC.lowrank_reference(c, d)
    root, diag, dv = (d[k].cuda().requires_grad_() for k in ('root', 'diag', 'd'))
    lp = _lowrank_diag_log_prob(root, diag, dv)
    assert lp.shape == c.bshape
    grads = torch.autograd.grad(lp, (root, diag, dv), grad_outputs=d['g'].cuda())
    name = f'lowrank {AC.lowrank_id(c)} kappa {ref["kappa"]:.3g}'
    if c.dt == 'f64':
        ok = [measured(name + ' lp', lp, ref['lp'], **CHOL64_VALUE)]
    else:
        ok = [_maxnorm(name + ' lp', lp, ref['lp'], AC.f32_bound('lowrank', 'value', c.n))]
    for what, got, leaf in zip(('groot', 'gdiag', 'gd'), grads, (root, diag, dv)):
        assert got.shape == leaf.shape
        if c.dt == 'f64':
            ok.append(measured(f'{name} {what}', got, ref[what], **CHOL64_GRAD))
        else:
            ok.append(_maxnorm(f'{name} {what}', got, ref[what], AC.f32_bound('lowrank', 'grad', c.n)))
    assert all(ok), ok


# ---------------------------------------------------------------------------------------------------------------- WhitenFn
def _whiten_run(ops, c, data, bucket):
    """One forward + backward of the case.  bucket=True: the parameters live in a FlatBucket whose gradients autograd hands
    over (the optimiser's arrangement) and the gradients are read from p.grad after loss.backward(); bucket=False: plain
    leaves, torch.autograd.grad inside ops.grad_sinks(False).  Returns (Ws, info, [gradient or None per parameter])."""
    from nsgp import svgp
    from nsgp.optim import FlatBucket
    params = [torch.nn.Parameter(g[k].cuda()) for g in data for k in ('Z', 'ls', 'os')]
    fb = FlatBucket(params, grads_as_views=False) if bucket else None
    groups = [tuple(params[3 * i:3 * i + 3]) for i in range(len(data))]
    res = svgp.whiten(groups, jitter=AC.WHITEN_JITTER, chol_bwd_f64=c.chol_bwd_f64, passthrough=c.passthrough,
                      out_dtype=AC.DT[c.out_dtype] if c.out_dtype else None)
    Ws, info = res[0], res[1]
    losses = [(W * g['Wbar'].to(W.dtype).cuda()).sum() for W, g in zip(Ws, data) if g['used']]
    if c.passthrough:
        for trip, g in zip(res[2], data):
            losses += [(p * cf.to(p.dtype).cuda()).sum() for p, cf in zip(trip, g['coef'])]
    # whatever the backward allocates next is likely to reuse this block: a group nobody differentiated must not read it
    junk = torch.full((sum(g['Z'].shape[0] for g in data), c.M, c.M), AC.NAN, dtype=F64, device='cuda')
    del junk
    if bucket:
        torch.autograd.backward(losses)
        grads = [p.grad for p in params]
    else:
        with ops.grad_sinks(False):
            grads = list(torch.autograd.grad(losses, params, allow_unused=True))
    del fb
    return Ws, info, grads


@pytest.mark.parametrize('c', AC.WHITEN_CASES, ids=AC.whiten_id)
def test_whiten_node(ops, c):
    data, ref = AC.whiten_build(c), AC.whiten_reference(c)
    kappa = AC.whiten_kappa(c)
    assert kappa < AC.KAPPA_CAP
    Ws, info, grads = _whiten_run(ops, c, data, bucket=False)
    _, _, grads_b = _whiten_run(ops, c, data, bucket=True)
    assert not info.requires_grad and info.cpu().tolist() == [0] * sum(g['Z'].shape[0] for g in data)
    name = f'whiten {AC.whiten_id(c)} kappa {kappa:.3g}'
    kzz_only = AC.whiten_reference(c._replace(passthrough=False))          # the Kzz route alone
    ok = []
    for gi, (W, g, r) in enumerate(zip(Ws, data, ref)):
        assert W.dtype == (F32 if c.out_dtype else F64)
        ok.append(measured(f'{name} W[{gi}]', W, r['W'], **(W64_TO_F32 if c.out_dtype else CHOL64_VALUE)))
        got = grads[3 * gi:3 * gi + 3]
        if not g['used']:
            # exactly the gradient of the pass-throughs the loss used, or nothing
            for t, cf in zip(got, g['coef']):
                if c.passthrough:
                    assert torch.equal(t.cpu(), cf.to(t.dtype))
                else:
                    assert t is None or float(t.abs().max()) == 0.0
            continue
        for what, t, leaf in zip(('gZ', 'gls', 'gos'), got, (g['Z'], g['ls'], g['os'])):
            assert t.shape == leaf.shape and t.dtype == leaf.dtype
            if not c.chol_bwd_f64:
                ok.append(_maxnorm(f'{name} {what}[{gi}] (group kappa {r["kappa"]:.3g})', t, r[what],
                                   AC.f32_bound('whiten_bwd32', 'grad', c.M)))
            elif c.pdt == 'f64':
                ok.append(measured(f'{name} {what}[{gi}]', t, r[what], **CHOL64_GRAD))
            elif not c.passthrough:
                ok.append(measured(f'{name} {what}[{gi}]', t, r[what], **CHOL64_GRAD_TO_F32))
            else:
                # float32 sum of two float32 routes: the Kzz route is rounded to float32, then the sum is: 2^-24 of each
                allowed = 1e-9 + 1e-8 * r[what].abs() + 2.0 ** -24 * (kzz_only[gi][what].abs() + r[what].abs())
                ratio = float(((t.detach().double().cpu() - r[what]).abs() / allowed).max())
                print(f'[measured] {name} {what}[{gi}]: worst diff / (CHOL64_GRAD + 2^-24 (|Kzz route| + |sum|)) = {ratio:.3g}')
                ok.append(ratio < 1.0)
    assert all(ok), ok
    # the optimiser's bucket changes where gradients land, never their bits
    for a, b in zip(grads, grads_b):
        assert (a is None and (b is None or float(b.abs().max()) == 0.0)) or torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ layer nodes
def _layer_settings(cfg):
    import contextlib
    from nsgp.gp import settings
    stack = contextlib.ExitStack()
    for name, value in AC.LAYER_CFG[cfg].items():
        stack.enter_context(getattr(settings, name)(value))
    return stack


def _rel(name, got, ref):
    err = float((got.detach().double().cpu() - ref).abs().max()) / (float(ref.abs().max()) + 1e-30)
    print(f'[measured] {name}: max-norm rel err {err:.3g}')
    return err


@pytest.mark.parametrize('c', AC.LAYER_CASES, ids=AC.layer_id)
def test_svgp_layer_nodes(ops, c):
    from nsgp import svgp
    from nsgp.gp import settings
    d, ref = AC.layer_build(c), AC.layer_reference(c)
    b, M, n, D = AC.LAYER_SHAPES[c.shape]
    dt = AC.DT[c.dt]
    leaves = {k: d[k].to(dt).cuda().requires_grad_(k != 'x' or c.x_grad) for k in AC.LAYER_LEAVES if k in d}
    first, second, planes = AC.layer_select(c)
    with _layer_settings(c.cfg):
        # the settings alone put the node on the pair the row is there for
        w64f = torch.empty(b, M, M, dtype=F64, device='cuda') if c.dt == 'f32' else None
        fusable = settings.fuse_kzx.on() and ops.svgp_kzx_fusable(w64f, leaves['Z'], leaves['x'], n)
        sel = svgp.select_projection(dt, M, D, n, c.kzx_f64, True, fusable, settings.forward_precision.value(),
                                     settings.whiten_matmul_f64.on(), settings.whiten_matmul_i8.on(), settings.fuse_kzx.on(),
                                     settings.hidden_var_f64.value(), diag_q=c.q == 'diag')
        assert sel[:3] == (first, second, planes), (sel, first, second, planes)
        mean, var, info = svgp.svgp_marginal(leaves['x'], leaves['Z'], leaves['ls'], leaves['os'], leaves['m'],
                                             Lq=leaves.get('Lq'), s2=leaves.get('s2'), jitter=AC.LAYER_JITTER,
                                             mean_w=leaves.get('mean_w'), mean_c=leaves.get('mean_c'), kzx_f64=c.kzx_f64)
        ((mean * d['gm'].to(dt).cuda()).sum() + (var * d['gv'].to(dt).cuda()).sum()).backward()
    assert not info.requires_grad and info.cpu().tolist() == [0] * b
    name = f'layer {AC.layer_id(c)} ({first}, {second}) kappa {ref["kappa"]:.3g}'
    bf16_first, bf16_second = first == 'bf16', second == 'bf16' or first == 'bf16'
    ok = []
    if c.dt == 'f64':
        ok += [measured(name + ' mean', mean, ref['mean'], **LAYER64_VALUE), measured(name + ' var', var, ref['var'], **LAYER64_VALUE)]
    elif bf16_first:                       # 'bf16_all': both projections carry bf16 operands
        ok += [_finite(mean, var), _rel(name + ' mean', mean, ref['mean']) <= 3 * BF16_MEASURED[first, second]['mean'],
               _rel(name + ' var', var, ref['var']) <= 3 * BF16_MEASURED[first, second]['var']]
    else:
        ok.append(measured(name + ' mean', mean, ref['mean'], **F32_VALUE_TOL))
        if bf16_second:
            ok.append(_rel(name + ' var', var, ref['var']) < BF16_VAR_TOL)
        else:
            ok.append(measured(name + ' var', var, ref['var'], **F32_VALUE_TOL))
    for k, leaf in leaves.items():
        if k == 'x' and not c.x_grad:
            assert leaf.grad is None
            continue
        g, r = leaf.grad, ref['grads'][k]
        assert g is not None and g.shape == leaf.shape and g.dtype == dt, k
        r = torch.tril(r) if k == 'Lq' else r
        err = _rel(f'{name} g_{k}', g, r)
        if bf16_second:
            ok.append(_finite(g) and err <= 3 * BF16_MEASURED[first, second]['grad'])
        else:
            ok.append(err < (LAYER64_GRAD if c.dt == 'f64' else F32_GRAD_TOL))
    assert all(ok), ok


# ------------------------------------------------------------------------------------------------------- wrapper contracts
def _kernel_call(ops, node, t, **over):
    a = dict(t, **over)
    if node == 'gibbs':
        return ops.gibbs_kernel(a['x1'], a['x2'], a['ell1'], a['ell2'], a['outputscale'], a['diag_add'])
    if node == 'rbf':
        return ops.rbf_kernel(a['x1'], a['x2'], a['ls'], a['os'])
    if node == 'matern':
        return ops.matern_kernel(a['x1'], a['x2'], a['ls'], a['os'], 1.5)
    if node == 'rbf_periodic':
        return ops.rbf_periodic_kernel(a['x1'], a['x2'], a['ls_rbf'], a['ls_per'], a['period'], a['os'])
    return ops.ps2d_kernel(a['x1'], a['x2'], a['s1'], a['s2'])


def _wrap_subsets(ops, node):
    """Every needs_input_grad subset of the node's tensor inputs: the subset's gradients are the all-on run's, the others None."""
    names = AC.WRAP_TENSOR_INPUTS[node]
    inp = {k: v.cuda() for k, v in AC.wrap_inputs(node).items()}
    G = inp.pop('G')

    def run(subset):
        t = {k: (v.clone().requires_grad_(k in subset) if k in names else v) for k, v in inp.items()}
        _kernel_call(ops, node, t).backward(G)
        return {k: t[k].grad for k in names}
    full = run(names)
    assert all(v is not None and v.shape == inp[k].shape for k, v in full.items())
    for r in range(1, len(names)):
        for subset in itertools.combinations(names, r):
            got = run(subset)
            for k in names:
                if k in subset:
                    assert measured(f'{node} {"+".join(subset)}: {k}', got[k], full[k], **SUBSET64), (subset, k)
                else:
                    assert got[k] is None, (subset, k)


def _wrap_gibbs(ops, variant):
    o, dg, lay = variant.split('|')
    inp = AC.wrap_inputs('gibbs')
    leaves = {k: v.clone().requires_grad_() for k, v in inp.items() if k != 'G'}
    dev = {k: v.detach().cuda().requires_grad_() for k, v in leaves.items()}
    pick = lambda src, key, mode: None if mode.endswith('none') else (float(inp[key]) if mode.endswith('float') else src[key])  # noqa: E731
    Kr = AC.gibbs_dense(leaves['x1'], leaves['x2'], leaves['ell1'], leaves['ell2'], pick(leaves, 'outputscale', o),
                        pick(leaves, 'diag_add', dg))
    K = ops.gibbs_kernel(dev['x1'], dev['x2'], dev['ell1'], dev['ell2'], pick(dev, 'outputscale', o), pick(dev, 'diag_add', dg))
    assert measured(f'gibbs {variant} K', K, Kr, **WRAP64)
    Gr = AC.with_layout(inp['G'], lay[1:])
    Kr.backward(Gr)
    K.backward(AC.with_layout(inp['G'].cuda(), lay[1:]))
    for k in leaves:
        used = not ((k == 'outputscale' and o != 'os_tensor') or (k == 'diag_add' and dg != 'diag_tensor'))
        if used:
            assert dev[k].grad.shape == leaves[k].shape
            assert measured(f'gibbs {variant} g_{k}', dev[k].grad, leaves[k].grad, **WRAP64)
        else:
            assert dev[k].grad is None


def _wrap_rbf_shared(ops, variant):
    which, lay = variant.split('|')
    inp = AC.wrap_inputs('rbf')
    if which in ('shared_x1', 'shared_both'):
        inp['x1'] = inp['x1'][0]
    if which in ('shared_x2', 'shared_both'):
        inp['x2'] = inp['x2'][0]
    leaves = {k: v.clone().requires_grad_() for k, v in inp.items() if k != 'G'}
    dev = {k: v.detach().cuda().requires_grad_() for k, v in leaves.items()}
    Kr = AC.rbf_dense(leaves['x1'], leaves['x2'], leaves['ls'], leaves['os'])
    K = ops.rbf_kernel(dev['x1'], dev['x2'], dev['ls'], dev['os'])
    assert measured(f'rbf {variant} K', K, Kr, **WRAP64)
    Kr.backward(AC.with_layout(inp['G'], lay[1:]))
    K.backward(AC.with_layout(inp['G'].cuda(), lay[1:]))
    for k in leaves:
        assert dev[k].grad.shape == leaves[k].shape
        assert measured(f'rbf {variant} g_{k}', dev[k].grad, leaves[k].grad, **WRAP64)


def _wrap_loss(ops, node, variant):
    inp = AC.wrap_inputs(node)
    g = inp['g']
    if node.startswith('kl'):
        leaves = {k: inp[k].clone().requires_grad_() for k in ('m', 'Lq') + (('addin',) if 'addin' in variant else ())}
        dev = {k: v.detach().cuda().requires_grad_() for k, v in leaves.items()}
        ref = AC.kl_whitened_dense(leaves['m'], leaves['Lq']) * (0.25 if 'total' in node else 1.0)
        if node == 'kl_whitened':
            out = ops.KlWhitenedFn.apply(dev['m'], dev['Lq'])
        else:
            out = ops.KlWhitenedTotalFn.apply(dev['m'], dev['Lq'], 0.25, dev.get('addin'))
            ref = ref + (leaves['addin'] if 'addin' in leaves else 0.0)
        assert out.shape == ()
    else:
        leaves = {k: inp[k].clone().requires_grad_() for k in ('mu', 'v')}
        dev = {k: v.detach().cuda().requires_grad_() for k, v in leaves.items()}
        noise = inp['noise'].cuda()                                        # requires_grad False: no gradient asked for
        ref = AC.gauss_ell_dense(inp['y'], leaves['mu'], leaves['v'], inp['noise'], 0.5)
        fn = ops.GaussEllTotalFn if 'total' in node else ops.GaussEllFn
        out = fn.apply(inp['y'].cuda(), dev['mu'], dev['v'], noise, 0.5)
        if 'total' in node:
            ref, g = ref.sum(), torch.tensor(1.7, dtype=F64)
        assert out.shape == ref.shape
    assert measured(f'{node} {variant} value', out, ref, **WRAP64)
    (ref * g).sum().backward()                                              # a non-unit upstream gradient
    (out * g.cuda()).sum().backward()
    if not node.startswith('kl'):
        assert noise.grad is None
    for k in leaves:
        assert dev[k].grad.shape == leaves[k].shape
        assert measured(f'{node} {variant} g_{k}', dev[k].grad, leaves[k].grad, **WRAP64)


@pytest.mark.parametrize('c', AC.WRAP_CASES, ids=AC.wrap_id)
def test_wrapper_contract(ops, c):
    if c.variant == 'subsets':
        _wrap_subsets(ops, c.node)
    elif c.node == 'gibbs':
        _wrap_gibbs(ops, c.variant)
    elif c.node == 'rbf':
        _wrap_rbf_shared(ops, c.variant)
    else:
        _wrap_loss(ops, c.node, c.variant)


# ------------------------------------------------------------------------------- the nodes' own reductions, called directly
@pytest.mark.parametrize('what', ['matmul_2x3', 'matmul_3x2', 'matmul_1x3', 'matmul_3x1', 'mvn_d_bcast', 'rbf_shared_x1',
                                  'rbf_shared_x2', 'matern_shared_x1', 'rbf_periodic_shared_x2'])
def test_backward_itself_returns_gradients_in_the_inputs_shapes(ops, what):
    """autograd's engine sums a gradient that is merely broadcastable to its input, so a node that forgets its own
    `sum(0)` / `sum_to_size` still passes every test that goes through .backward().  The static backward is called here
    directly, on the node's own ctx (the output's grad_fn), and must hand back the inputs' shapes itself."""
    from nsgp.gp.distributions import MvnLogProbFn
    if what.startswith('matmul'):
        c = AC._mm('f64', False, True, '', what[7:])
        d = AC.matmul_build(c)
        A, B = d['A_st'].cuda().requires_grad_(), d['B_st'].cuda().requires_grad_()
        C = ops.matmul(A, B, c.ta, c.tb)
        gA, gB = ops.MatmulFn.backward(C.grad_fn, d['G_st'].cuda())[:2]
        ref = AC.matmul_reference(c, d)
        assert gA.shape == A.shape and gB.shape == B.shape
        assert torch.equal(gA.cpu(), ref['gA']) and torch.equal(gB.cpu(), ref['gB'])
    elif what == 'mvn_d_bcast':
        c = AC.MvnCase('f64', 65, (3,), 'bcast')
        d = AC.mvn_build(c)
        K, dv = d['K'].cuda().requires_grad_(), d['d'].cuda().requires_grad_()
        lp, _ = MvnLogProbFn.apply(K, dv)
        gK, gd = MvnLogProbFn.backward(lp.grad_fn, d['g'].cuda(), None)
        assert gK.shape == K.shape and gd.shape == dv.shape
        assert measured('mvn direct gd', gd, AC.mvn_reference(c, d)['gd'], **CHOL64_GRAD)
    else:
        node, which = what.rsplit('_shared_', 1)
        inp = {k: v.cuda() for k, v in AC.wrap_inputs(node).items()}
        inp[which] = inp[which][0]
        G = inp.pop('G')
        t = {k: v.clone().requires_grad_() for k, v in inp.items()}
        K = _kernel_call(ops, node, t)
        fn = {'rbf': ops.RbfKernelFn, 'matern': ops.MaternKernelFn, 'rbf_periodic': ops.RbfPeriodicKernelFn}[node]
        grads = fn.backward(K.grad_fn, G)
        assert grads[0].shape == t['x1'].shape and grads[1].shape == t['x2'].shape
        # and the shared input's gradient is the SUM of the per-GP ones: the same node on a per-GP copy of that input
        tb = dict(t, **{which: inp[which].expand(AC.WRAP_BATCH, *inp[which].shape).contiguous().requires_grad_()})
        Kb = _kernel_call(ops, node, tb)                                      # (kept alive: its grad_fn owns the saved tensors)
        per_gp = fn.backward(Kb.grad_fn, G)[0 if which == 'x1' else 1]
        assert per_gp.shape == tb[which].shape
        assert measured(f'{what} direct g_{which}', grads[0 if which == 'x1' else 1], per_gp.sum(0), **SUBSET64)


# ------------------------------------------------------------------------------------------------------- double backward
def _once_nodes(ops):
    """name -> callable returning (output the loss squares, an input that requires grad) for every node but MatmulFn."""
    from nsgp import svgp
    from nsgp.gp.distributions import MvnLogProbFn
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64).cuda()          # noqa: E731
    ru = lambda *s: (0.5 + torch.rand(*s, generator=g, dtype=F64)).cuda()   # noqa: E731
    n, D, b, M, S = 20, 2, 2, 16, 3
    spd = AC.PB._spd64(M, 1)[0].cuda()
    Lq = (torch.tril(0.1 * rn(b, M, M)) + torch.eye(M, dtype=F64, device='cuda'))
    x = rn(n, D).requires_grad_()
    ell = ru(D, n)
    Z, ls, os_, m = rn(b, M, D), ru(b, D), ru(b), rn(b, M)
    y, mu, v, noise = rn(n), rn(S, n).requires_grad_(), ru(S, n), ru(1)
    sig = torch.eye(2, dtype=F64, device='cuda').expand(n, 2, 2).contiguous().requires_grad_()
    Kin = spd.clone().requires_grad_()
    Zg = Z.clone().requires_grad_()
    mg = m.clone().requires_grad_()
    mean = rn(b, 1, n).requires_grad_()
    return {
        'CholInvFn': lambda: (ops.chol_inv(Kin)[0], Kin),
        'MvnLogProbFn': lambda: (MvnLogProbFn.apply(Kin, rn(M))[0], Kin),
        'WhitenFn': lambda: (svgp.whiten([(Zg, ls, os_)])[0][0], Zg),
        'GibbsKernelFn': lambda: (ops.gibbs_kernel(x, x, ell, ell), x),
        'RbfKernelFn': lambda: (ops.rbf_kernel(x, x, ls, os_), x),
        'MaternKernelFn': lambda: (ops.matern_kernel(x, x, ls, os_, 2.5), x),
        'RbfPeriodicKernelFn': lambda: (ops.rbf_periodic_kernel(x, x, ls, ru(b), ru(b), os_), x),
        'Ps2dKernelFn': lambda: (ops.ps2d_kernel(x.detach(), x.detach(), sig, sig), sig),
        'GaussEllFn': lambda: (ops.GaussEllFn.apply(y, mu, v, noise, 1.0), mu),
        'GaussEllTotalFn': lambda: (ops.GaussEllTotalFn.apply(y, mu, v, noise, 1.0), mu),
        'KlWhitenedFn': lambda: (ops.KlWhitenedFn.apply(mg, Lq), mg),
        'KlWhitenedTotalFn': lambda: (ops.KlWhitenedTotalFn.apply(mg, Lq, 1.0), mg),
        'KlMeanFieldTotalFn': lambda: (ops.KlMeanFieldTotalFn.apply(mg, ru(b, M)), mg),
        'DsviObjectiveFn': lambda: (ops.DsviObjectiveFn.apply(y, mu, v, noise, 1.0, 1.0, mg, Lq), mu),
        'DgpSampleFn': lambda: (ops.DgpSampleFn.apply(mean, ru(b, 1, n), rn(S, n, b)), mean),
        'SVGPLayerFn': lambda: (svgp.svgp_marginal(x, Z, ls, os_, mg, Lq)[0], mg),
        'SVGPMeanFieldLayerFn': lambda: (svgp.svgp_marginal(x, Z, ls, os_, mg, s2=ru(b, M))[0], mg),
    }


ONCE_NODES = ('CholInvFn', 'MvnLogProbFn', 'WhitenFn', 'GibbsKernelFn', 'RbfKernelFn', 'MaternKernelFn', 'RbfPeriodicKernelFn',
              'Ps2dKernelFn', 'GaussEllFn', 'GaussEllTotalFn', 'KlWhitenedFn', 'KlWhitenedTotalFn', 'KlMeanFieldTotalFn',
              'DsviObjectiveFn', 'DgpSampleFn', 'SVGPLayerFn', 'SVGPMeanFieldLayerFn')


@pytest.mark.parametrize('node', ONCE_NODES)
def test_nodes_other_than_matmul_refuse_a_second_derivative(ops, node):
    """Their backward passes are raw library calls: a second derivative through them would be silently wrong (the gradient
    would depend on the inputs through the upstream gradient only), so it must raise."""
    out, leaf = _once_nodes(ops)[node]()
    (g,) = torch.autograd.grad((out * out).sum(), leaf, create_graph=True)     # upstream gradient 2 out requires grad
    assert _finite(g)
    with pytest.raises(RuntimeError, match='once_differentiable'):
        g.sum().backward()


def test_every_node_of_the_package_is_covered():
    """A new torch.autograd.Function must join the double-backward table (or be differentiable twice, like MatmulFn)."""
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nsgp.gp.distributions as dist
    from nsgp import ops as o, svgp
    found = {name for mod in (o, svgp, dist) for name, v in vars(mod).items()
             if isinstance(v, type) and issubclass(v, torch.autograd.Function) and v.__module__ == mod.__name__}
    assert found - {'KlMeanFieldFn'} == set(ONCE_NODES) | {'MatmulFn'}


def test_zz_wall_time_and_slowest_ids():
    """Last in the file: its wall time and slowest ids (printed under -s)."""
    wall = time.perf_counter() - _T0[0]
    slow = sorted(_TIMES.items(), key=lambda kv: -kv[1])[:8]
    print(f'[timing] test_gpu_autograd_nodes.py: {len(_TIMES)} tests, wall {wall:.2f} s; slowest: ' +
          ', '.join(f'{k} {v * 1e3:.0f} ms' for k, v in slow))
