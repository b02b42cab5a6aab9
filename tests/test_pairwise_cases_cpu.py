"""Case tables, input builders and float64 references for the pairwise builds (csrc/pairwise.hip), and the checks of the
tables themselves that need no GPU.  tests/test_gpu_pairwise.py runs every row on the device.

Families: gibbs, rbf, matern12 / matern32 / matern52, rbf_periodic (with and without ls_rbf, with and without os), ps2d; each
in float32 and float64.

References.  `ref_forward` is oracle.kernels / test_matern_cpu.matern_ref evaluated in float64 on the inputs already rounded
to the row's dtype.  `ref_terms` gives, per output, the PER-TERM tensor t[b, i, j, k] = G[b, i, j] dk[b, i, j] / dtheta_k in
closed form (float64): a row-side output is its sum over j, a column-side output its sum over i, a global output its sum over
both, and sum |t| is the scale of the rounding bound of that output.  test_terms_sum_to_autograd_of_the_oracle holds the sums
to autograd of the oracle, including the Matern nu = 1/2 zero-at-zero convention and the periodic r = 0 branch.

Inputs.  Points lie on a jittered Kronecker lattice in a box of about one lengthscale (`side`), so every kernel value is
>= 0.05 of the output scale.  x1 fills the lower 0.4 of the box in every coordinate and x2 the upper 0.4: every coordinate
difference is 0.2 .. 1 box sides, bounded below, so no term is negligible and none is the difference of two nearly equal
quotients (the ARD functor divides by the lengthscale before it subtracts).  The bound below takes sum |t| as the scale of a
term's own rounding error, which holds only where a term is not itself a cancelling sum, so the builders keep the three
brackets that could cancel away from zero:
  Gibbs   l1 in [1, 1.15], l2 in [1.5, 1.7], box side <= 0.5: in 1/(2l) - l/s + 2 l delta^2/s^2 the first two parts give
          +-(l2^2 - l1^2)/(2 l s), of size >= 0.087, and the third is <= 0.056.
  ps2d    S1 = [[~1.05, +0.25], [+0.25, ~1.05]], S2 = [[~1.5, -0.25], [-0.25, ~1.5]], box side 0.2: 1/4 (S^-T - A^-T) keeps its
          sign entry by entry and the quadratic part 1/2 (B^-T d)(B^-1 d)^T stays below half of it.
  periodic  period >= 4 > 2 |x1 - x2|: sin and cos of pi r / period are both positive, so the periodic and the RBF part of
          d/dx have one sign.
Where l1 ~ l2 the Gibbs bracket cancels to a small fraction of its parts, and an output that is a single term (n2 = 1) then
carries a rounding error far above any multiple of u |t|: sum |t| is not the scale of such a term's error, so these rows do
not run that regime (the existing Gibbs tests, at their own tolerances, do).
|G| is in [0.5, 1.5] with random signs.  PROBED positions -- first and last row and column of the matrix and of the first and
last tile edge in each direction -- carry a spike of `spike(fam, n1, n2)` >= 64, sized so that one missing probed term moves every
output it feeds by more than 4x that output's bound (asserted here, from the reference alone).  The guarantee covers the
crossings of probed rows and probed columns only: inside a probed row or column sum |t| is dominated by its spikes, so a
missing UNSPIKED term there lies inside the bound; the unprobed rows and columns, which carry no spike, catch such a term
where it is one of few.  One same-buffer row per family has x2 = x1 (`same`): its diagonal terms are zero by construction
(zero distance), which is what that row is for, and its margin is asserted off the diagonal.

Backward bound (per output element):  |err| <= ((N + c) u + eps_fwd) sum |t|.
  u        unit roundoff of the dtype.
  c        roundings in one term, counted from the functor's grad (`TERM_ROUNDINGS`).
  eps_fwd  the forward relative tolerance of that family and dtype (`fwd_tol`): the element-wise exp / rsqrt / sincos.
  N        additions on the longest path from a term to the output under the row's plan (`path_adds`):
             row item     4 (a lane's four columns, serial) + 6 (wave tree) + ceil(ntj / 8) (its chain in pass 2) + 7 (the
                          eight chains, serial) + 1 (the division by the lengthscale, where there is one)
             column item  rows / 4 (a wave's rows, serial) + 3 (four waves through LDS, serial) + ceil(nti / 8) + 7 + 1
             global       rows (a lane's rows / 4 x 4 entries, serial) + 9 (block tree: 6 + 3) + ceil(nti ntj / 256) (the
                          stride-256 loop of pass 2) + 9 + 1
             same-buffer  the longer of the row and the column path with BOTH chain lengths: a row block's chain adds
             summing      ceil(ntj / 8) row-side and then ceil(nti / 8) column-side partials.
"""
import math
import zlib
from typing import NamedTuple

import pytest
import torch

from oracle import kernels as OK
from test_matern_cpu import matern_ref

F32, F64 = torch.float32, torch.float64
DTYPES = {'f32': F32, 'f64': F64}
CPT = {'f32': 4, 'f64': 2}                       # columns per thread of the forward kernel; the tile is 64 x 64 CPT
UNIT = {'f32': 2.0 ** -24, 'f64': 2.0 ** -53}
FWD_TI, BWD_TJ = 64, 256
DIAG_ADD = 0.375
PS_JITTER = 0.01

FAMILIES = {
    #  stem: library entry points nsgp_<stem>_build_*; dims: the D values run; spec: the D values with their own functor
    'gibbs': dict(stem='gibbs', batched=False, dims=(1, 2, 3, 4, 8), spec=(1, 2, 3)),
    'rbf': dict(stem='rbf', batched=True, dims=(1, 2, 3, 4, 8), spec=(1, 2, 3)),
    'matern12': dict(stem='matern', nu=0.5, batched=True, dims=(1, 2, 3, 4, 8), spec=(1, 2, 3)),
    'matern32': dict(stem='matern', nu=1.5, batched=True, dims=(1, 2, 3, 4, 8), spec=(1, 2, 3)),
    'matern52': dict(stem='matern', nu=2.5, batched=True, dims=(1, 2, 3, 4, 8), spec=(1, 2, 3)),
    'rbfper': dict(stem='rbf_periodic', lsr=True, os=True, batched=True, dims=(1, 2, 3, 8), spec=(1, 2)),
    'rbfper_nolsr': dict(stem='rbf_periodic', lsr=False, os=True, batched=True, dims=(1, 2, 3, 8), spec=(1, 2)),
    'rbfper_noos': dict(stem='rbf_periodic', lsr=True, os=False, batched=True, dims=(1, 2, 3, 8), spec=(1, 2)),
    'per_plain': dict(stem='rbf_periodic', lsr=False, os=False, batched=True, dims=(1, 2, 3, 8), spec=(1, 2)),
    'ps2d': dict(stem='ps2d', batched=False, dims=(2,), spec=(2,)),
}
# roundings in one term of the functor's grad, from the operands as loaded to the value added to the accumulator (an upper
# count: every multiply, add, divide and reciprocal is one, a fused multiply-add is counted as two)
TERM_ROUNDINGS = {
    'gibbs': lambda D: 22 + 4 * D,        # base(): 4 per further dimension, 6 around rsqrt / exp; per d: s 3, inv 1, df 1, q 3,
                                          # bracket 7, w 2, product 1
    'ard': lambda D: 10 + 2 * D,          # point / ls 2, df 1, sq 2 per dimension, radial polynomial <= 5, w 2, w df df 2
    'rbf_periodic': lambda D: 30 + 6 * D,   # base(): 2 + 4 per dimension, sqrt, u 2, exponent 6; w 2, dsdu 4, period 3, dr 2, gx 4
    'ps2d': lambda D: 60,                 # determinants 3 x 3, quad 9, k 5, B^-1 d 8, shared term 4, dr 2, sum 3, product 1
}


def fam_kind(fam):
    stem = FAMILIES[fam]['stem']
    return 'ard' if stem in ('rbf', 'matern') else stem


def fwd_tol(fam, dtn):
    """(rtol, atol) of the existing forward tests: test_gpu_kernels._tol, and test_gpu_spatiotemporal's for the periodic
    builds."""
    if fam_kind(fam) == 'rbf_periodic':
        return (2e-4, 2e-5) if dtn == 'f32' else (1e-10, 1e-11)
    return (2e-5, 2e-6) if dtn == 'f32' else (1e-11, 1e-12)


# --------------------------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------------------------
_ALPHA = [math.sqrt(p) % 1.0 for p in (2, 3, 5, 7, 11, 13, 17, 19)]


def side(fam, D):
    """Box side: |x1 - x2|^2 <= D side^2 <= 3.24, about one lengthscale, every kernel value >= 0.05.  Gibbs and ps2d take a
    smaller box, so that the bracket of their lengthscale / matrix terms keeps its sign (module docstring)."""
    return 0.2 if fam == 'ps2d' else min(1.8 / math.sqrt(D), 0.5) if fam == 'gibbs' else 1.8 / math.sqrt(D)


def _lattice(n, D, s, lo, phase, gen, dt):
    """n points of a jittered Kronecker lattice in [lo, lo + 0.4] x side per coordinate."""
    i = torch.arange(1, n + 1, dtype=F64).unsqueeze(1)
    base = torch.remainder(i * torch.tensor(_ALPHA[:D], dtype=F64) + phase, 1.0)
    jit = torch.rand(n, D, generator=gen, dtype=F64) * 0.01
    return (s * (lo + 0.39 * base + jit)).to(dt)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32('/'.join(str(k) for k in key).encode()))


def make_inputs(fam, dtn, D, batch, n1, n2, shared):
    """The row's inputs in its own dtype (CPU).  Point i of a set depends on i alone (and the family, dtype, D, batch entry),
    never on n: a prefix of a larger problem's inputs is the smaller problem's inputs."""
    dt, f = DTYPES[dtn], FAMILIES[fam]
    g = _gen(fam, dtn, D)
    s = side(fam, D)
    u = lambda *shape: torch.rand(*shape, generator=g, dtype=F64)       # noqa: E731
    p = {}
    if f['batched']:
        for name, n, lo, ph in (('x1', n1, 0.0, 0.0), ('x2', n2, 0.6, 0.37)):
            xs = [_lattice(n, D, s, lo, ph + 0.13 * b, _gen(fam, dtn, D, name, b), dt) for b in range(1 if shared else batch)]
            p[name] = xs[0] if shared else torch.stack(xs)
    else:
        p['x1'] = _lattice(n1, D, s, 0.0, 0.0, _gen(fam, dtn, D, 'x1'), dt)
        p['x2'] = _lattice(n2, D, s, 0.6, 0.37, _gen(fam, dtn, D, 'x2'), dt)
    kind = fam_kind(fam)
    if kind == 'gibbs':
        for name, n, lo, w in (('l1', n1, 1.0, 0.15), ('l2', n2, 1.5, 0.2)):
            gl = _gen(fam, dtn, D, name)
            p[name] = (lo + w * torch.rand(n, D, generator=gl, dtype=F64)).T.contiguous().to(dt)       # (D, n) dim-major
        p['os'] = torch.tensor([1.3], dtype=dt)
    elif kind == 'ard':
        p['ls'] = (1.0 + 0.5 * u(256, 8))[:batch, :D].contiguous().to(dt)
        p['os'] = (0.7 + 0.6 * u(256))[:batch].contiguous().to(dt)
    elif kind == 'rbf_periodic':
        p['lsr'] = (1.0 + 0.5 * u(256, 8))[:batch, :D].contiguous().to(dt) if f['lsr'] else None
        p['lsp'] = (2.0 + 0.5 * u(256))[:batch].contiguous().to(dt)
        p['per'] = (4.0 + 0.5 * u(256))[:batch].contiguous().to(dt)
        os_ = (0.7 + 0.6 * u(256))[:batch].contiguous().to(dt)
        p['os'] = os_ if f['os'] else None
    else:
        for name, n, lo, sg in (('s1', n1, 1.0, 1.0), ('s2', n2, 1.45, -1.0)):
            r = torch.rand(n, 4, generator=_gen(fam, dtn, name), dtype=F64)
            off, asym = sg * (0.23 + 0.04 * r[:, 1]), 0.04 * (r[:, 2] - 0.5)
            p[name] = torch.stack([lo + 0.1 * r[:, 0], off + asym, off - asym, lo + 0.1 * r[:, 3]], -1).reshape(n, 2, 2).to(dt)
    return p


def slice_inputs(fam, p, n1, n2):
    """The (n1, n2) problem inside a larger problem's inputs."""
    q = dict(p)
    for name, n in (('x1', n1), ('x2', n2)):
        q[name] = p[name][..., :n, :].contiguous()
    for name, n in (('l1', n1), ('l2', n2)):
        if name in p:
            q[name] = p[name][:, :n].contiguous()
    for name, n in (('s1', n1), ('s2', n2)):
        if name in p:
            q[name] = p[name][:n].contiguous()
    return q


def spike(fam, n1, n2):
    """Factor on G at a probed position: 64, or the power of two above n1 n2 / 512 (periodic builds, whose float32 forward
    tolerance is ten times the others': n1 n2 / 51.2), so that one probed term stays above 4x the float32 bound of a global
    output (a sum of n1 n2 terms).  The float64 twin of a row takes the same factor."""
    scale = fwd_tol(fam, 'f32')[0] / 2e-5
    return float(max(64, 2 ** math.ceil(math.log2(max(scale * n1 * n2 / 512.0, 1.0)))))


def edge_indices(n, tile):
    """First and last index, and both sides of the first and of the last tile edge inside [0, n)."""
    last = ((n - 1) // tile) * tile
    return sorted({i for i in (0, n - 1, tile - 1, tile, last - 1, last) if 0 <= i < n})


def probed(n1, n2, rows):
    return [(i, j) for i in edge_indices(n1, rows) for j in edge_indices(n2, BWD_TJ)]


def make_G(fam, dtn, batch, n1, n2, rows):
    dt = DTYPES[dtn]
    g = _gen(fam, dtn, 'G', batch, n1, n2)
    G = (0.5 + torch.rand(batch, n1, n2, generator=g, dtype=F64)) * \
        (torch.randint(0, 2, (batch, n1, n2), generator=g).double() * 2 - 1)
    ii = torch.tensor(edge_indices(n1, rows))
    jj = torch.tensor(edge_indices(n2, BWD_TJ))
    G[:, ii[:, None], jj[None, :]] *= spike(fam, n1, n2)
    return G.to(dt)


# --------------------------------------------------------------------------------------------
# float64 references
# --------------------------------------------------------------------------------------------
def _f64(p):
    return {k: (None if v is None else v.double()) for k, v in p.items()}


def ref_forward(fam, p, diag_add=0.0, jitter=PS_JITTER):
    """(batch, n1, n2) float64 from the oracle; p: float64 inputs."""
    f, kind = FAMILIES[fam], fam_kind(fam)
    if kind == 'gibbs':
        K = OK.gibbs(p['x1'], p['x2'], p['l1'], p['l2'])[None]
        if p.get('os') is not None:
            K = K * p['os']
    elif kind == 'ard':
        if 'nu' in f:
            K = matern_ref(p['x1'], p['x2'], p['ls'], p['os'], f['nu'])
        else:
            K = OK.rbf_ard(p['x1'], p['x2'], p['ls'][:, None, :], p['os'])
    elif kind == 'rbf_periodic':
        K = OK.periodic(p['x1'], p['x2'], p['lsp'][:, None, None], p['per'][:, None, None])
        if p['lsr'] is not None:
            K = K * OK.rbf_ard(p['x1'], p['x2'], p['lsr'][:, None, :])
        if p['os'] is not None:
            K = K * p['os'][:, None, None]
    else:
        K = OK.ps2d(p['x1'], p['x2'], p['s1'], p['s2'], jitter)[None]
    if diag_add:
        K = K + diag_add * torch.eye(K.shape[-2], K.shape[-1], dtype=F64)
    return K


def _delta(p):
    x1, x2 = p['x1'], p['x2']
    x1 = x1 if x1.dim() == 3 else x1[None]
    x2 = x2 if x2.dim() == 3 else x2[None]
    return x1[:, :, None, :] - x2[:, None, :, :]                      # (b or 1, n1, n2, D)


def ref_terms(fam, p, G, jitter=PS_JITTER):
    """{output: (kind, t)}: kind in row / col / glob, t:(batch, n1, n2, K) float64 with t[b,i,j,k] = G[b,i,j] dk[b,i,j]/dtheta_k.
    p: float64 inputs, G:(batch, n1, n2) float64."""
    f, kind = FAMILIES[fam], fam_kind(fam)
    df = _delta(p)
    if kind == 'gibbs':
        a = p['l1'].T[None, :, None, :]                               # (1, n1, 1, D)
        b = p['l2'].T[None, None, :, :]
        s = a * a + b * b
        os_ = p['os'] if p.get('os') is not None else torch.ones(1, dtype=F64)
        k0 = torch.sqrt(2 * a * b / s).prod(-1) * torch.exp(-(df * df / s).sum(-1))
        w = (G * k0 * os_)[..., None]
        q = df * df / (s * s)
        gx = 2 * w * df / s
        return {'l1': ('row', w * (0.5 / a - a / s + 2 * a * q)), 'l2': ('col', w * (0.5 / b - b / s + 2 * b * q)),
                'x1': ('row', -gx), 'x2': ('col', gx), 'os': ('glob', (G * k0)[..., None])}
    if kind == 'ard':
        ls = p['ls'][:, None, None, :]
        uu = df / ls
        s = (uu * uu).sum(-1)
        d = s.sqrt()
        nu = f.get('nu')
        if nu is None:
            kap = torch.exp(-0.5 * s)
            phi = -kap
        elif nu == 0.5:
            kap = torch.exp(-d)
            phi = torch.where(d > 0, -kap / torch.where(d > 0, d, torch.ones_like(d)), torch.zeros_like(d))
        elif nu == 1.5:
            a = math.sqrt(3.0)
            kap, phi = (1 + a * d) * torch.exp(-a * d), -3.0 * torch.exp(-a * d)
        else:
            a = math.sqrt(5.0)
            kap, phi = (1 + a * d + 5.0 / 3.0 * s) * torch.exp(-a * d), -5.0 / 3.0 * (1 + a * d) * torch.exp(-a * d)
        w = (G * p['os'][:, None, None] * phi)[..., None]
        gx = w * uu / ls
        return {'x1': ('row', gx), 'x2': ('col', -gx), 'ls': ('glob', -w * uu * uu / ls), 'os': ('glob', (G * kap)[..., None])}
    if kind == 'rbf_periodic':
        lp, pe = p['lsp'][:, None, None], p['per'][:, None, None]
        r = (df * df).sum(-1).sqrt()
        sn, cs = torch.sin(math.pi * r / pe), torch.cos(math.pi * r / pe)
        expo = -2 * sn * sn / lp
        if p['lsr'] is not None:
            lr = p['lsr'][:, None, None, :]
            expo = expo - 0.5 * (df * df / (lr * lr)).sum(-1)
        k0 = torch.exp(expo).expand(G.shape)
        w = G * k0 * (p['os'][:, None, None] if p['os'] is not None else 1.0)
        dsdu = 4 * sn * cs * math.pi / lp
        dr = torch.where(r > 0, dsdu / pe / torch.where(r > 0, r, torch.ones_like(r)), torch.zeros_like(r))
        gx = -dr[..., None] * df
        out = {}
        if p['lsr'] is not None:
            gx = gx - df / (lr * lr)
            out['lsr'] = ('glob', w[..., None] * df * df / (lr * lr * lr))
        gx = w[..., None] * gx
        out.update({'x1': ('row', gx), 'x2': ('col', -gx), 'lsp': ('glob', (w * 2 * sn * sn / (lp * lp))[..., None]),
                    'per': ('glob', (w * dsdu * r / (pe * pe))[..., None])})
        out['os'] = ('glob', (G * k0)[..., None])                      # os == NULL means 1: g_os is still d/d os there
        return out
    # Paciorek-Schervish: k = |S1|^1/4 |S2|^1/4 |A|^-1/2 exp(-d^T B^-1 d), A = (S1 + S2) / 2, B = A + jitter I, so
    #   d log k / dS1 = 1/4 S1^-T - 1/4 A^-T + 1/2 (B^-T d)(B^-1 d)^T     (-d^T d(B^-1) d = d^T B^-1 dB B^-1 d, dB/dS1 = 1/2)
    # with the 2 x 2 inverses written out (M^-1 = adj(M) / det M), elementwise
    s1 = p['s1'].reshape(-1, 4)[None, :, None, :]                      # (1, n1, 1, 4)
    s2 = p['s2'].reshape(-1, 4)[None, None, :, :]
    det = lambda m: m[..., 0] * m[..., 3] - m[..., 1] * m[..., 2]      # noqa: E731
    inv_t = lambda m: torch.stack([m[..., 3], -m[..., 2], -m[..., 1], m[..., 0]], -1) / det(m)[..., None]   # noqa: E731
    A = 0.5 * (s1 + s2)
    B = A + jitter * torch.tensor([1.0, 0.0, 0.0, 1.0], dtype=F64)
    d0, d1 = df[..., 0], df[..., 1]
    dB = det(B)
    z0, z1 = (B[..., 3] * d0 - B[..., 1] * d1) / dB, (-B[..., 2] * d0 + B[..., 0] * d1) / dB        # B^-1 d
    v0, v1 = (B[..., 3] * d0 - B[..., 2] * d1) / dB, (-B[..., 1] * d0 + B[..., 0] * d1) / dB        # B^-T d
    k = det(s1).pow(0.25) * det(s2).pow(0.25) * det(A).pow(-0.5) * torch.exp(-(d0 * z0 + d1 * z1))
    w = (G * k)[..., None]
    shared = -0.25 * inv_t(A) + 0.5 * torch.stack([v0 * z0, v0 * z1, v1 * z0, v1 * z1], -1)
    return {'s1': ('row', w * (shared + 0.25 * inv_t(s1))), 's2': ('col', w * (shared + 0.25 * inv_t(s2)))}


_AXES = {'row': (2,), 'col': (1,), 'glob': (1, 2)}


def reduce_terms(terms, sym=False):
    """{output: (value, sum |t|)} float64: row (b, n1, K), col (b, n2, K), glob (b, K).  sym: the same-buffer summing mode --
    every row output also receives its column twin ('x1' <- 'x2', 'l1' <- 'l2', 's1' <- 's2'), which is not written."""
    out = {}
    for name, (kind, t) in terms.items():
        out[name] = (t.sum(_AXES[kind]), t.abs().sum(_AXES[kind]))
    if sym:
        for a, b in (('x1', 'x2'), ('l1', 'l2'), ('s1', 's2')):
            if a in out:
                out[a] = (out[a][0] + out[b][0], out[a][1] + out[b][1])
                del out[b]
    return out


def path_adds(kind, rows, nti, ntj, sym=False):
    """N of the bound: additions on the longest path from a term to an output of this kind (module docstring)."""
    c8 = lambda t: -(-t // 8)                                           # noqa: E731
    row = 4 + 6 + c8(ntj) + 7 + 1
    col = rows // 4 + 3 + c8(nti) + 7 + 1
    if sym:
        return max(4 + 6, rows // 4 + 3) + c8(ntj) + c8(nti) + 7 + 1
    return {'row': row, 'col': col, 'glob': rows + 9 + -(-(nti * ntj) // 256) + 9 + 1}[kind]


def bound_factor(fam, dtn, D, kind, plan, sym=False):
    """(N + c) u + eps_fwd."""
    return (path_adds(kind, *plan, sym=sym) + TERM_ROUNDINGS[fam_kind(fam)](D)) * UNIT[dtn] + fwd_tol(fam, dtn)[0]


# --------------------------------------------------------------------------------------------
# forward table
# --------------------------------------------------------------------------------------------
FWD_N1 = (1, 3, 4, 5, 63, 64, 65, 129)
FWD_LAYOUTS = ('contig', 'ld_odd', 'sk_odd', 'base1')
FWD_BATCHING = ((1, True), (3, True), (3, False))                    # (batch, x shared by the batch)
FWD_N1_MAX = 321


def fwd_n2(dtn):
    c = CPT[dtn]
    w = 64 * c
    return (1, c - 1, c, c + 1, w - 1, w, w + 1, 2 * w + 1)


def fwd_n2_max(dtn):
    return max(2 * 64 * CPT[dtn] + 1, 321)


def fwd_shapes(dtn):
    """(n1, n2): the full cross of the tile-edge sizes (both rectangular orientations), and shapes beyond 256 rows whose
    diagonal leaves a 64-row tile inside a column tile and ends inside one."""
    return [(a, b) for a in FWD_N1 for b in fwd_n2(dtn)] + [(300, 300), (321, 321), (321, 65), (65, 321), (257, 258)]


def fwd_layout(layout, dtn, n1, n2):
    """(ldk, batch stride, element offset of K in a buffer aligned to 16 bytes) of a layout class.
    contig: the wrapper's; ld_odd: ldk % CPT != 0; sk_odd: ldk aligned, batch stride % CPT != 0; base1: both aligned, the base
    pointer one element past an aligned address."""
    c = CPT[dtn]
    up = -(-n2 // c) * c
    if layout == 'contig':
        return n2, n1 * n2, 0
    if layout == 'ld_odd':
        return up + c + 1, n1 * (up + c + 1) + 2 * c, 0
    if layout == 'sk_odd':
        return up + c, n1 * (up + c) + c + 1, 0
    return up + c, (n1 + 1) * (up + c), 1


def fwd_masters():
    """One master build per (family, dtype, D, batch, shared, diag_add device scalar or NULL): the largest problem, K a window
    with aligned ld, batch stride and base (the vector store path).  Every forward row is a prefix of its master."""
    out = []
    for fam, f in FAMILIES.items():
        for dtn in DTYPES:
            for D in f['dims']:
                if f['batched']:
                    out += [(fam, dtn, D, b, sh, True) for b, sh in FWD_BATCHING]
                else:
                    out += [(fam, dtn, D, 1, True, True)]
                    if fam == 'gibbs':
                        out += [(fam, dtn, D, 1, True, False)]          # diag_add NULL (and outputscale NULL)
    return out


# --------------------------------------------------------------------------------------------
# backward table
# --------------------------------------------------------------------------------------------
class Bwd(NamedTuple):
    fam: str
    dtn: str
    D: int
    batch: int
    n1: int
    n2: int
    plan: tuple            # (rows per workgroup, nti, ntj), pinned: what nsgp_pairwise_bwd_plan must answer
    shared: bool = False   # x shared by the batch
    ldg: int = 0           # padding of G's rows (elements)
    sg: int = 0            # padding between G's batch entries (elements)
    sym: bool = False      # same-buffer summing mode
    nulls: bool = False    # also run every NULL / non-NULL combination of the outputs
    same: bool = False     # x2 = x1: the diagonal has distance 0 (Matern nu = 1/2 zero-at-zero, periodic r = 0 branch)

    @property
    def name(self):
        tags = ''.join(t for t, on in (('-shared', self.shared), (f'-ldg{self.ldg}', self.ldg), (f'-sg{self.sg}', self.sg),
                                       ('-sym', self.sym), ('-nulls', self.nulls), ('-same', self.same)) if on)
        return f'{self.fam}-{self.dtn}-D{self.D}-b{self.batch}-{self.n1}x{self.n2}{tags}'


def _plan(batch, n1, n2):
    """The table's own statement of the plan (the library's is compared with it row by row)."""
    wgs = batch * -(-n1 // 64) * -(-n2 // 256)
    rows = 64 if wgs >= 256 else 16
    return (rows, -(-n1 // rows), -(-n2 // 256))


# shapes on the 16-row path: (n1, n2).  Row tails n1 mod 16 in {1, 3, 4, 5, 15, 0}, column tails n2 mod 256 in {1, 63, 64, 65,
# 255, 0}; 2305 columns: 10 row-item partials; 145 rows: 10 column-item partials; (4097, 1): 257 global partials
S16 = [(17, 1), (19, 63), (20, 64), (21, 65), (31, 255), (32, 256), (33, 257), (3, 2305), (145, 321), (4097, 1)]
# on the 64-row path, batched: (batch, n1, n2) with batch ceil(n1/64) ceil(n2/256) >= 256.  Row tails n1 mod 64 in {1, 3, 4, 5, 63, 0}
S64_BATCHED = [(128, 65, 1), (128, 67, 63), (256, 4, 64), (256, 5, 65), (256, 63, 2), (256, 1, 255), (256, 64, 3),
               (256, 2, 256)]
# both sides of the threshold at the smallest sizes that reach it: 258 and 252 workgroups
THRESH_BATCHED = [(43, 129, 257), (42, 129, 257)]
# unbatched (Gibbs, ps2d): 256, 256, 256 and 252 workgroups
THRESH_UNBATCHED = [(1, 65281), (16321, 1), (4033, 769), (4032, 769)]
# on the 64-row path, unbatched: row tails with one column, column tails with one row
S64_UNBATCHED = [(16323, 1), (16324, 1), (16325, 1), (16383, 1), (16384, 1),
                 (1, 65343), (1, 65344), (1, 65345), (1, 65535), (1, 65536)]


def _bwd_cases():
    rows = []

    def add(fam, dtn, D, batch, n1, n2, **kw):
        rows.append(Bwd(fam, dtn, D, batch, n1, n2, _plan(batch, n1, n2), **kw))
    for fam, f in FAMILIES.items():
        dims = f['dims']
        for dtn in DTYPES:
            if f['batched']:
                # the 16-row shapes, D cycling through every value of the family, batch 1 / 2 / 3, x shared or not
                for k, (n1, n2) in enumerate(S16):
                    add(fam, dtn, dims[k % len(dims)], 1 + k % 3, n1, n2, shared=k % 2 == 1)
                for k, (b, n1, n2) in enumerate(S64_BATCHED):
                    add(fam, dtn, dims[(k + 1) % len(dims)], b, n1, n2, shared=k % 2 == 0)
                for b, n1, n2 in THRESH_BATCHED:
                    add(fam, dtn, 1, b, n1, n2)
                add(fam, dtn, 2, 2, 37, 300, ldg=3, sg=5)
                add(fam, dtn, dims[-1], 2, 129, 129, sym=True)               # 16-row path, generic functor; 9 column-side
                #                                                              partials per item: all 8 chains add some
                add(fam, dtn, 1, 256, 65, 65, sym=True)                      # 64-row path: 2 x 1 x 256 workgroups
                add(fam, dtn, 2, 2, 21, 65, nulls=True)
                add(fam, dtn, 2, 2, 77, 77, sym=True, same=True)
            else:
                for k, (n1, n2) in enumerate(S16):
                    add(fam, dtn, dims[k % len(dims)], 1, n1, n2)
                for k, (n1, n2) in enumerate(S64_UNBATCHED):
                    add(fam, dtn, dims[(k + 1) % len(dims)], 1, n1, n2)
                for n1, n2 in THRESH_UNBATCHED:
                    add(fam, dtn, dims[min(1, len(dims) - 1)], 1, n1, n2)
                add(fam, dtn, dims[min(1, len(dims) - 1)], 1, 37, 300, ldg=3)
                add(fam, dtn, dims[-1], 1, 129, 129, sym=True)
                add(fam, dtn, dims[0], 1, 1985, 1985, sym=True)              # 64-row path: 32 x 8 workgroups, 1985 = 31 * 64 + 1
                add(fam, dtn, 2, 1, 21, 65, nulls=True)
                add(fam, dtn, 2, 1, 77, 77, sym=True, same=True)
    return rows


BWD_CASES = _bwd_cases()


def outputs_of(fam, p):
    """Output names of the family's backward in ABI order (those the inputs make available)."""
    kind = fam_kind(fam)
    if kind == 'gibbs':
        return ['l1', 'l2', 'x1', 'x2', 'os']
    if kind == 'ard':
        return ['x1', 'x2', 'ls', 'os']
    if kind == 'rbf_periodic':
        return ['x1', 'x2', 'lsr', 'lsp', 'per', 'os']
    return ['s1', 's2']


def bwd_problem(case):
    """(inputs in the row's dtype, G in the row's dtype) of a backward row."""
    p = make_inputs(case.fam, case.dtn, case.D, case.batch, case.n1, case.n2, case.shared or not FAMILIES[case.fam]['batched'])
    if case.same:                                                     # the Kzz case: one point set on both sides
        # the probed points are PLACED, evenly across the set's part of the box: between two of them every coordinate differs
        # by >= 0.05 box sides, so that a probed off-diagonal term is not small by an accident of the lattice
        idx = sorted(set(edge_indices(case.n1, case.plan[0])) | set(edge_indices(case.n2, BWD_TJ)))
        d = torch.arange(case.D, dtype=F64)
        for r, i in enumerate(idx):
            p['x1'][..., i, :] = (side(case.fam, case.D) * (0.02 + 0.36 * r / max(len(idx) - 1, 1) + 0.004 * d)).to(p['x1'].dtype)
        p['x2'] = p['x1'].clone()
    return p, make_G(case.fam, case.dtn, case.batch, case.n1, case.n2, case.plan[0])


def bwd_reference(case, p, G):
    """{output: (value, bound)} float64 for the row: bound = ((N + c) u + eps_fwd) sum |t|."""
    red = reduce_terms(ref_terms(case.fam, _f64(p), G.double()), sym=case.sym)
    kinds = {'l1': 'row', 'x1': 'row', 's1': 'row', 'l2': 'col', 'x2': 'col', 's2': 'col'}
    return {name: (val, bound_factor(case.fam, case.dtn, case.D, kinds.get(name, 'glob'), case.plan,
                                     sym=case.sym and name in ('l1', 'x1', 's1')) * mag)
            for name, (val, mag) in red.items()}


# --------------------------------------------------------------------------------------------
# checks of the tables (no GPU)
# --------------------------------------------------------------------------------------------
def bwd_classes(c):
    """The boundary classes a backward row hits.  Tail and chain classes are kept apart for the batched entry points and the
    unbatched ones (Gibbs, ps2d: no batch stride, grid z = 1) and for the two kernels (16 or 64 rows per workgroup)."""
    rows, nti, ntj = c.plan
    f = FAMILIES[c.fam]
    path = ('batched' if f['batched'] else 'unbatched', f'r{rows}')
    nr = {'gibbs': 2, 'ard': 1, 'rbf_periodic': 1, 'ps2d': 2}[fam_kind(c.fam)] * (c.D if c.D in f['spec'] else 8)
    out = {path + ('row-tail', c.n1 % rows), path + ('col-tail', c.n2 % BWD_TJ),
           (c.fam, c.dtn, 'D', c.D), (c.fam, c.dtn, path[1])}
    out.add((path[0], 'workgroups', c.batch * -(-c.n1 // 64) * -(-c.n2 // 256)))
    if ntj > 8:
        out.add(path + ('row-chain-wrap',))
    if nti > 8:
        out.add(path + ('col-chain-wrap',))
    if nti * ntj > 256:
        out.add(path + ('glob-loop-wrap',))
    if (c.n1 * nr) % 32 or (c.n2 * nr) % 32:
        out.add(path + ('items-not-32',))
    if c.ldg:
        out.add((c.fam, c.dtn, 'ldg'))
    if c.sg:
        out.add((c.fam, c.dtn, 'sG'))
    if c.sym:
        out.add((c.fam, c.dtn, 'sym', path[1]))
        if nti >= 8:
            out.add((c.fam, c.dtn, 'sym-all-chains'))
    if c.nulls:
        out.add((c.fam, c.dtn, 'nulls'))
    if c.same:
        out.add((c.fam, c.dtn, 'zero-distance'))
    return out


def bwd_required():
    req = set()
    for kind in ('batched', 'unbatched'):
        for rows in (16, 64):
            path = (kind, f'r{rows}')
            req |= {path + ('row-tail', t) for t in (1, 3, 4, 5, rows - 1, 0)}
            req |= {path + ('col-tail', t) for t in (1, 63, 64, 65, 255, 0)}
            req.add(path + ('items-not-32',))
        req |= {(kind, 'r16', 'row-chain-wrap'), (kind, 'r16', 'col-chain-wrap'), (kind, 'r16', 'glob-loop-wrap')}
    req |= {('unbatched', 'r64', 'row-chain-wrap'), ('unbatched', 'r64', 'col-chain-wrap'),
            ('batched', 'workgroups', 258), ('batched', 'workgroups', 252),
            ('unbatched', 'workgroups', 256), ('unbatched', 'workgroups', 252)}
    for fam, f in FAMILIES.items():
        for dtn in DTYPES:
            req |= {(fam, dtn, 'D', D) for D in f['dims']}
            req |= {(fam, dtn, 'r16'), (fam, dtn, 'r64'), (fam, dtn, 'ldg'), (fam, dtn, 'sym', 'r16'), (fam, dtn, 'sym', 'r64'),
                    (fam, dtn, 'nulls'), (fam, dtn, 'sym-all-chains'), (fam, dtn, 'zero-distance')}
            if f['batched']:
                req.add((fam, dtn, 'sG'))
    return req


def test_every_family_runs_two_generic_dimensions_and_every_specialised_one():
    for fam, f in FAMILIES.items():
        if fam == 'ps2d':
            continue
        assert set(f['spec']) <= set(f['dims']), fam
        assert len(set(f['dims']) - set(f['spec'])) >= 2, fam
    assert FAMILIES['rbfper']['spec'] == (1, 2) and 3 in FAMILIES['rbfper']['dims']


def test_backward_table_hits_every_boundary_class():
    """Closure over (path, row-tail class, column-tail class, chain-wrap flags, D class, layout class): every required class
    is hit by a row.  Deleting (4097, 1) from S16 leaves ('batched', 'r16', 'glob-loop-wrap') uncovered; deleting (3, 2305)
    leaves (*, 'r16', 'row-chain-wrap'), deleting (256, 63, 2) from S64_BATCHED leaves ('batched', 'r64', 'row-tail', 63)."""
    covered = set()
    for c in BWD_CASES:
        covered |= bwd_classes(c)
    missing = bwd_required() - covered
    assert not missing, sorted(missing, key=str)
    # the named threshold rows are in the table for every family they apply to
    shapes = {(c.fam, c.dtn, c.batch, c.n1, c.n2) for c in BWD_CASES}
    for fam, f in FAMILIES.items():
        for dtn in DTYPES:
            want = [(b, n1, n2) for b, n1, n2 in THRESH_BATCHED] if f['batched'] else [(1, n1, n2) for n1, n2 in THRESH_UNBATCHED]
            for s in want:
                assert (fam, dtn) + s in shapes, (fam, dtn, s)
    assert len({c.name for c in BWD_CASES}) == len(BWD_CASES)


def test_forward_table_hits_every_boundary_class():
    for dtn in DTYPES:
        c, w = CPT[dtn], 64 * CPT[dtn]
        shapes = fwd_shapes(dtn)
        assert {b for _, b in shapes} >= {1, c - 1, c, c + 1, w - 1, w, w + 1, 2 * w + 1}
        assert {a for a, _ in shapes} >= {1, 3, 4, 5, 63, 64, 65, 129}
        assert any(a > b for a, b in shapes) and any(a < b for a, b in shapes)
        # beyond 256: the diagonal leaves a row tile inside a column tile, and the matrix ends inside a tile
        assert any(a > 256 and b > 256 and a % FWD_TI and b % w for a, b in shapes)
        assert all(a <= FWD_N1_MAX and b <= fwd_n2_max(dtn) for a, b in shapes)
        for a, b in shapes:
            ld, sk, off = fwd_layout('contig', dtn, a, b)
            assert (ld, sk, off) == (b, a * b, 0)
            ld, sk, off = fwd_layout('ld_odd', dtn, a, b)
            assert ld >= b and ld % c != 0 and sk >= a * ld
            ld, sk, off = fwd_layout('sk_odd', dtn, a, b)
            assert ld >= b and ld % c == 0 and sk % c != 0 and sk >= a * ld
            ld, sk, off = fwd_layout('base1', dtn, a, b)
            assert ld >= b and ld % c == 0 and sk % c == 0 and off == 1 and sk >= a * ld
    masters = fwd_masters()
    for fam, f in FAMILIES.items():
        for dtn in DTYPES:
            mine = [m for m in masters if m[0] == fam and m[1] == dtn]
            assert {m[2] for m in mine} == set(f['dims'])
            if f['batched']:
                assert {(m[3], m[4]) for m in mine} == set(FWD_BATCHING)
    assert {m[5] for m in masters if m[0] == 'gibbs'} == {True, False}


def _load_lib():
    import nsgp
    return nsgp.load_library()


def test_plan_query_matches_every_row_and_validates_its_arguments():
    from nsgp import ops, BackendError
    _load_lib()
    for c in BWD_CASES:
        assert tuple(ops.pairwise_bwd_plan(c.batch, c.n1, c.n2)) == c.plan, c.name
    # the named boundary rows, written out (not through _plan)
    literal = {(43, 129, 257): (64, 3, 2), (42, 129, 257): (16, 9, 2), (1, 1, 65281): (64, 1, 256), (1, 16321, 1): (64, 256, 1),
               (1, 4033, 769): (64, 64, 4), (1, 4032, 769): (16, 252, 4), (1, 4097, 1): (16, 257, 1), (1, 3, 2305): (16, 1, 10),
               (1, 145, 321): (16, 10, 2), (2, 129, 129): (16, 9, 1), (256, 65, 65): (64, 2, 1), (1, 1985, 1985): (64, 32, 8)}
    in_table = {(c.batch, c.n1, c.n2): c.plan for c in BWD_CASES}
    for shape, plan in literal.items():
        assert in_table[shape] == plan and tuple(ops.pairwise_bwd_plan(*shape)) == plan, shape
    assert tuple(ops.pairwise_bwd_plan(2, 1024, 1024)) == (16, 64, 4)           # 128 workgroups of 64 rows: the DSVI Kzz adjoint
    assert tuple(ops.pairwise_bwd_plan(1, 4096, 4096)) == (64, 64, 16)
    assert tuple(ops.pairwise_bwd_plan(0, 5, 5)) == tuple(ops.pairwise_bwd_plan(1, 0, 5)) == (0, 0, 0)
    for bad in ((-1, 1, 1), (1, -1, 1), (1, 1, -1)):
        with pytest.raises(BackendError):
            ops.pairwise_bwd_plan(*bad)
    import ctypes
    lib = _load_lib()
    r, a, b = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
    P = lambda v: ctypes.cast(ctypes.byref(v), ctypes.c_void_p)         # noqa: E731
    assert lib.nsgp_pairwise_bwd_plan(1, 1, 1, None, P(a), P(b)) == -4
    assert lib.nsgp_pairwise_bwd_plan(1, 1, 1, P(r), None, P(b)) == -5
    assert lib.nsgp_pairwise_bwd_plan(1, 1, 1, P(r), P(a), None) == -6


def test_workspace_queries_follow_the_plan():
    """bwd_ws_elems and the launch take the plan from one helper: the reported bytes are the plan's partial counts with the
    generic functor's accumulator counts (NR, NC, NG), plus the 256 bytes of slack."""
    lib = _load_lib()
    for batch, n1, n2 in ((1, 17, 1), (2, 1024, 1024), (43, 129, 257), (42, 129, 257), (1, 4033, 769), (1, 4032, 769)):
        rows, nti, ntj = _plan(batch, n1, n2)
        elems = lambda nr, nc, ng: batch * (ntj * n1 * nr + nti * n2 * nc + nti * ntj * ng)    # noqa: E731
        for es in (4, 8):
            assert lib.nsgp_rbf_build_bwd_workspace(batch, n1, n2, 2, es) == elems(8, 8, 9) * es + 256
            assert lib.nsgp_matern_build_bwd_workspace(batch, n1, n2, 2, es) == elems(8, 8, 9) * es + 256
            assert lib.nsgp_rbf_periodic_build_bwd_workspace(batch, n1, n2, 2, es) == elems(8, 8, 11) * es + 256
            if batch == 1:
                assert lib.nsgp_gibbs_build_bwd_workspace(n1, n2, 2, es) == elems(16, 16, 1) * es + 256
                assert lib.nsgp_ps2d_build_bwd_workspace(n1, n2, es) == elems(4, 4, 1) * es + 256


AUTOGRAD_CASES = [(fam, D, shared) for fam, f in FAMILIES.items() for D in (f['dims'][0], f['dims'][-1])
                  for shared in ((False, True) if f['batched'] else (True,))]


@pytest.mark.parametrize('fam,D,shared', AUTOGRAD_CASES, ids=lambda v: str(v))
def test_terms_sum_to_autograd_of_the_oracle(fam, D, shared):
    """sum of the per-term tensors == autograd of the oracle, to 1e-12 of sum |t| (the scale of every bound here)."""
    batch = 2 if FAMILIES[fam]['batched'] else 1
    n1, n2 = 23, 19
    p = _f64(make_inputs(fam, 'f64', D, batch, n1, n2, shared))
    G = make_G(fam, 'f64', batch, n1, n2, 16).double()
    _check_against_autograd(fam, p, G, shared)


@pytest.mark.parametrize('fam', ['matern12', 'matern32', 'matern52', 'rbf', 'rbfper', 'per_plain', 'gibbs', 'ps2d'])
def test_terms_at_zero_distance_follow_the_oracle(fam):
    """x1 == x2: the diagonal has distance 0 -- Matern nu = 1/2 takes the derivative there as 0, the periodic factor's r = 0
    branch adds nothing."""
    batch = 2 if FAMILIES[fam]['batched'] else 1
    n = 13
    p = _f64(make_inputs(fam, 'f64', 2, batch, n, n, True))
    p['x2'] = p['x1'].clone()
    G = make_G(fam, 'f64', batch, n, n, 16).double()
    terms = ref_terms(fam, p, G)
    if fam == 'matern12':
        i = torch.arange(n)
        assert float(terms['x1'][1][:, i, i].abs().max()) == 0.0 and float(terms['ls'][1][:, i, i].abs().max()) == 0.0
    _check_against_autograd(fam, p, G, True)


def _check_against_autograd(fam, p, G, shared):
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items() if v is not None}
    q = dict(p, **leaves)
    (ref_forward(fam, q) * G).sum().backward()
    red = reduce_terms(ref_terms(fam, p, G))
    for name, (val, mag) in red.items():
        if name not in leaves:                                        # os of a periodic build without an output scale
            continue
        g = leaves[name].grad
        if name in ('l1', 'l2'):
            g = g.T[None]                                             # (D, n) -> (1, n, D)
        elif name in ('s1', 's2'):
            g = g.reshape(1, -1, 4)
        elif name in ('x1', 'x2') and g.dim() == 2:
            g, val, mag = g[None], val.sum(0, keepdim=True), mag.sum(0, keepdim=True)   # shared x: summed over the batch
        elif name in ('os', 'lsp', 'per') and fam != 'gibbs':
            g = g[:, None]
        elif fam == 'gibbs' and name == 'os':
            g = g[None]
        assert g.shape == val.shape, (name, g.shape, val.shape)
        err = float(((g - val).abs() / mag.clamp_min(1e-300)).max())
        assert err < 1e-12, (fam, name, err)


def test_kernel_values_stay_above_a_twentieth():
    """No term is negligible: every kernel value of every family is >= 0.05 of its output scale, at every D."""
    for fam, f in FAMILIES.items():
        for D in f['dims']:
            p = _f64(make_inputs(fam, 'f32', D, 3 if f['batched'] else 1, 200, 150, False if f['batched'] else True))
            K = ref_forward(fam, p)
            scale = p['os'].reshape(-1, 1, 1) if p.get('os') is not None else 1.0
            assert float((K / scale).min()) >= 0.05, (fam, D, float((K / scale).min()))


@pytest.mark.parametrize('case', BWD_CASES, ids=lambda c: c.name)
def test_a_missing_probed_term_moves_every_output_it_feeds_by_four_bounds(case):
    """For every probed position: removing that term changes the reference of its row item, its column item and the globals by
    more than 4x that output's bound."""
    p, G = bwd_problem(case)
    terms = ref_terms(case.fam, _f64(p), G.double())
    ref = bwd_reference(case, p, G)
    twin = {'x2': 'x1', 'l2': 'l1', 's2': 's1'}
    worst = math.inf
    ii = torch.tensor(edge_indices(case.n1, case.plan[0]))
    jj = torch.tensor(edge_indices(case.n2, BWD_TJ))
    for name, (kind, t) in terms.items():
        tt = t[:, ii[:, None], jj[None, :]].abs()                       # (b, |ii|, |jj|, K): the probed terms
        if case.same:                                                   # x2 = x1: a diagonal term is zero by construction
            tt = torch.where((ii[:, None] == jj[None, :])[None, :, :, None], torch.full_like(tt, math.inf), tt)
        bound = ref[twin[name] if case.sym and name in twin else name][1]
        if kind == 'row':
            b = bound[:, ii][:, :, None, :]
        elif kind == 'col':                                             # same-buffer mode: item j of the one buffer
            b = bound[:, jj][:, None, :, :]
        else:
            b = bound[:, None, None, :]
        worst = min(worst, float((tt / b).min()))
    assert worst > 4.0, (case.name, worst)
