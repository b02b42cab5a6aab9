"""Every kernel of csrc/gemm_bf16.hip against a float64 reference of the same operation, BIT FOR BIT wherever the operation is
exact (tables, input builders and references: tests/bf16_cases.py; their conditions: tests/test_bf16_cases_cpu.py).

* the casts and the transpose-cast are exact operations: dst equals the host's float -> bf16 (nearest-even, float64 through
  float32) on every element, ties, signed zeros, infinities, overflow, subnormals included (NaN compared with isnan);
* the MFMA projection on integer data whose partial sums stay below 2^24 is exact in any order: Y, its bf16 transposed copy
  YT and both column-statistic partials equal the float64 reference bit for bit, at every K-tile count 1 .. 7 of the
  two-deep pipeline in both triangle modes; on wider integers YT checks nearest-even and the partials a derived summation
  bound; on Gaussian data Y is held to the summation bound of its own operands;
* the bf16 RBF build returns, per element, the nearer bf16 neighbour of os exp(-s / 2) evaluated in float64, unless that
  value is within 2^-15 relative of the midpoint (then either neighbour).

Every output lives in a buffer with 64 guard words on either side and starts as a sentinel, so a store outside the layout
and an element never written both show."""
import ctypes

import pytest
import torch

import bf16_cases as BC
from conftest import measured

pytestmark = pytest.mark.gpu

GUARD = 64                                        # elements on either side of every output
GUARD_BITS = {torch.int32: 0x5A5A5A5A, torch.int16: 0x5A5A}
SENTINEL = {torch.int32: 0x4B4B4B4B, torch.int16: 0x4B4B}        # 1.33e7 in either format: no result of these tests
U = 2.0 ** -24                                    # unit roundoff of float32
GEMM = 'nsgp_svgp_tri_gemm_colstats_bf16'


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Out:
    """An output buffer of `numel` float32 / bf16 elements between guards, pre-filled with the sentinel."""

    def __init__(self, numel, dtype):
        self.dtype, self.numel = dtype, numel
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.buf = torch.full((numel + 2 * GUARD,), SENTINEL[self.bits], dtype=self.bits, device='cuda')
        self.buf[:GUARD] = GUARD_BITS[self.bits]
        self.buf[GUARD + numel:] = GUARD_BITS[self.bits]

    def ptr(self, offset=0):
        return ctypes.c_void_p(self.buf.data_ptr() + (GUARD + offset) * self.buf.element_size())

    def get(self, *shape):
        """The payload on the host, in the output's dtype; asserts the guards first."""
        h = self.buf.cpu()
        g = GUARD_BITS[self.bits]
        assert bool((h[:GUARD] == g).all()) and bool((h[GUARD + self.numel:] == g).all()), 'a guard word was overwritten'
        return h[GUARD:GUARD + self.numel].view(self.dtype).reshape(*shape)

    def untouched(self):
        h = self.buf.cpu()
        return bool((h[:GUARD] == GUARD_BITS[self.bits]).all()) and bool((h[GUARD + self.numel:] == GUARD_BITS[self.bits]).all()) \
            and bool((h[GUARD:GUARD + self.numel] == SENTINEL[self.bits]).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.dtype == torch.bfloat16 else torch.int64)


def _same_bits(got, ref):
    return got.shape == ref.shape and torch.equal(_bits(got), _bits(ref))


def _same_bits_or_nan(got, ref):
    nan = ref.float().isnan()
    return got.shape == ref.shape and bool(got.float().isnan()[nan].all()) and torch.equal(_bits(got)[~nan], _bits(ref)[~nan])


# ------------------------------------------------------------------------------------------------ casts

@pytest.mark.parametrize('case', BC.CAST_CASES, ids=BC.case_id)
def test_square_cast_is_the_hosts_nearest_even_cast_through_float32(case):
    """dst = op(src) -> float32 -> bf16 bit for bit.  The float64 rows found the kernel rounding ONCE (1 + 2^-8 + 2^-40 came
    out as 0x3F81): the compiler had folded `(__bf16)(float)v` into a single conversion of the double."""
    _need_gpu()
    from nsgp import _lib
    src = BC.cast_input(case)
    dst, dev = Out(src.numel(), torch.bfloat16), src.cuda()
    _lib.call('nsgp_cast_sq_bf16_' + case.dt, _p(dev), dst.ptr(), case.n, case.batch, case.transpose, case.tril, _stream())
    torch.cuda.synchronize()
    assert _same_bits_or_nan(dst.get(case.batch, case.n, case.n), BC.cast_reference(case))


@pytest.mark.parametrize('case', BC.TCAST_CASES, ids=BC.case_id)
def test_transpose_cast_is_the_hosts_cast_of_the_transpose(case):
    _need_gpu()
    from nsgp import _lib
    src = BC.tcast_input(case)
    dst, dev = Out(src.numel(), torch.bfloat16), src.cuda()
    _lib.call('nsgp_transpose_cast_bf16', _p(dev), dst.ptr(), case.batch, case.M, case.n, _stream())
    torch.cuda.synchronize()
    assert _same_bits_or_nan(dst.get(case.batch, case.n, case.M), BC.tcast_reference(case))


# ------------------------------------------------------------------------------------------------ projection

def _run_proj(tri, P, Qt, rv, yt=True):
    """One launch on host operands P (b, M, M) bf16, Qt (b, n, M) bf16, rv (b, M) float32 or None.  Returns the guarded
    outputs (Y, YT or None, part_dot, part_sq); part_dot is always passed (it must stay untouched without rv)."""
    from nsgp import _lib
    b, M, n = P.shape[0], P.shape[1], Qt.shape[1]
    T = -(-M // BC.BM)
    assert int(_lib.load().nsgp_svgp_bf16_tiles(M)) == T
    Y, YT = Out(b * M * n, torch.float32), Out(b * n * M, torch.bfloat16) if yt else None
    pd, ps = Out(b * T * n, torch.float32), Out(b * T * n, torch.float32)
    Pd, Qd, rd = P.cuda(), Qt.cuda(), None if rv is None else rv.cuda()
    _lib.call(GEMM, _p(Pd), tri, _p(Qd), None if rd is None else _p(rd), b, M, n, Y.ptr(), YT.ptr() if yt else None, pd.ptr(),
              ps.ptr(), _stream())
    torch.cuda.synchronize()
    return Y, YT, pd, ps


def _check_copy_and_partials(Yg, YT, pd, ps, rv, M, exact):
    """What holds for any data, against the kernel's OWN Y: YT is its transpose-cast, the partials are the tile-row sums of
    Y rv and Y^2 -- bit for bit where `exact`, else within 136 u sum|terms| (the 128 + 8 additions a column's reduction
    can at most chain, each correctly rounded)."""
    b, _, n = Yg.shape
    T = -(-M // BC.BM)
    if YT is not None:
        assert _same_bits(YT.get(b, n, M), Yg.transpose(-1, -2).contiguous().to(torch.bfloat16))
    Yd = Yg.double()
    sq = BC.tile_row_sums(Yd * Yd, M)
    got_sq = ps.get(b, T, n)
    if rv is None:
        assert pd.untouched()
    else:
        rd = rv.double().unsqueeze(-1)
        dot, adot = BC.tile_row_sums(Yd * rd, M), BC.tile_row_sums((Yd * rd).abs(), M)
        got_dot = pd.get(b, T, n)
    if exact:
        assert _same_bits(got_sq, sq.float()) and bool((sq.float().double() == sq).all())
        assert rv is None or (_same_bits(got_dot, dot.float()) and bool((dot.float().double() == dot).all()))
    else:
        assert bool(((got_sq.double() - sq).abs() <= 136 * U * sq).all())
        assert rv is None or bool(((got_dot.double() - dot).abs() <= 136 * U * adot).all())


@pytest.mark.parametrize('case', BC.PROJ_CASES, ids=BC.case_id)
def test_projection_against_float64_at_every_pipeline_edge(case):
    """Y, YT and the partials of one launch (see the module docstring).  The rows without rowvec found the kernel writing
    zeros into a part_dot it was handed all the same; it now leaves it alone."""
    _need_gpu()
    P, Qt, rv = BC.proj_inputs(case)
    ref = BC.proj_reference(case)
    Y, YT, pd, ps = _run_proj(case.tri, P, Qt, rv if case.rowvec else None, case.yt)
    Yg = Y.get(case.batch, case.M, case.n)
    if case.data == 'real':
        # float32 accumulation of exact products: (K + 8) additions in the worst chain, twice that for the MFMA's own order
        bound = 2 * (BC.summed_range(case).reshape(1, -1, 1) + 8) * U * ref['absY']
        ok = measured(f'bf16 projection Y {BC.case_id(case)} / summation bound', Yg.double() / bound, ref['Y'] / bound, 0.0, 1.0)
        assert ok and bool(torch.isfinite(Yg).all())
    else:
        assert _same_bits(Yg, ref['Y'].float())
    _check_copy_and_partials(Yg, YT, pd, ps, rv if case.rowvec else None, case.M, exact=case.data == 'small')
    if case.data == 'small':                                   # ... and the partials against the reference's own
        T = -(-case.M // BC.BM)
        assert _same_bits(ps.get(case.batch, T, case.n), ref['part_sq'].float())
        assert not case.rowvec or _same_bits(pd.get(case.batch, T, case.n), ref['part_dot'].float())


@pytest.mark.parametrize('tri', [BC.LOWER, BC.UPPER])
def test_projection_nan_stays_in_its_row_or_column(tri):
    _need_gpu()
    case = BC.ProjCase(tri, 1, 136, 129, True, True, 'small')
    P, Qt, rv = BC.proj_inputs(case)
    ref = BC.proj_reference(case)['Y'].float()
    for r in (5, 130):                                         # a NaN on the diagonal of P (inside either triangle): row r of Y
        Pn = P.clone()
        Pn[0, r, r] = float('nan')
        Y, YT, _, _ = _run_proj(tri, Pn, Qt, rv)
        Yg, YTg = Y.get(1, 136, 129), YT.get(1, 129, 136)
        rows = torch.arange(136) != r
        assert bool(Yg[0, r].isnan().all()) and _same_bits(Yg[:, rows], ref[:, rows])
        assert bool(YTg[0, :, r].float().isnan().all()) and _same_bits(YTg[:, :, rows], ref[:, rows].transpose(-1, -2).to(torch.bfloat16))
    for col, k in ((3, 70), (128, 130)):                       # a NaN in row `col` of Qt: column `col` of Y, nothing else
        Qn = Qt.clone()
        Qn[0, col, k] = float('nan')
        Y, _, _, _ = _run_proj(tri, P, Qn, rv)
        Yg = Y.get(1, 136, 129)
        cols = torch.arange(129) != col
        assert _same_bits(Yg[:, :, cols], ref[:, :, cols])
        hit = P[0, :, k].float() != 0                          # rows whose P really multiplies it
        assert bool(hit.any()) and bool(Yg[0, hit, col].isnan().all())


def test_projection_argument_checks_launch_nothing():
    _need_gpu()
    from nsgp import _lib
    fn = getattr(_lib.load(), GEMM)
    M, n = 16, 8
    P = torch.ones(M * M + 8, dtype=torch.bfloat16, device='cuda')
    Qt = torch.ones(n * M + 8, dtype=torch.bfloat16, device='cuda')
    rv = torch.ones(M, device='cuda')
    Y, YT = Out(M * n, torch.float32), Out(n * M + 8, torch.bfloat16)
    pd, ps = Out(n, torch.float32), Out(n, torch.float32)
    st = _stream()
    one = P.element_size()

    def rc(P_=_p(P), tri=1, Qt_=_p(Qt), batch=1, M_=M, n_=n, Y_=Y.ptr(), YT_=YT.ptr(), ps_=ps.ptr()):
        return fn(P_, tri, Qt_, _p(rv), batch, M_, n_, Y_, YT_, pd.ptr(), ps_, st)

    assert rc(tri=0) == -2 and rc(tri=3) == -2
    assert rc(M_=12) == -6
    assert rc(P_=ctypes.c_void_p(P.data_ptr() + one)) == -1 and rc(Qt_=ctypes.c_void_p(Qt.data_ptr() + one)) == -1
    assert rc(YT_=YT.ptr(1)) == -9
    assert rc(Y_=None) == -8 and rc(ps_=None) == -11
    assert rc(batch=0) == 0 and rc(M_=0) == 0 and rc(n_=0) == 0
    assert rc(batch=65536) == -24
    torch.cuda.synchronize()
    assert Y.untouched() and YT.untouched() and pd.untouched() and ps.untouched()
    assert rc() == 0                                           # and the same buffers are accepted as they stand
    torch.cuda.synchronize()
    assert bool((Y.get(M, n) == float(M)).all())               # operands of ones (the kernel masks nothing): Y = M everywhere


@pytest.mark.parametrize('tri', [BC.LOWER, BC.UPPER])
def test_chain_second_product_reads_the_first_ones_transposed_copy(tri):
    """Product 2 fed with the YT product 1 wrote, and with the transpose-cast of product 1's Y: the same bits."""
    _need_gpu()
    from nsgp import _lib
    b, M, n = 2, 136, 129
    P, Qt, rv = BC.proj_inputs(BC.ProjCase(tri, b, M, n, True, True, 'real'))
    P2, _, _ = BC.proj_inputs(BC.ProjCase(3 - tri, b, M, n, False, False, 'real'))
    Y, YT, _, _ = _run_proj(tri, P, Qt, rv)
    Yg, YTg = Y.get(b, M, n), YT.get(b, n, M)
    AT = Out(b * n * M, torch.bfloat16)
    Yd = Yg.cuda()
    _lib.call('nsgp_transpose_cast_bf16', _p(Yd), AT.ptr(), b, M, n, _stream())
    torch.cuda.synchronize()
    ATg = AT.get(b, n, M)
    assert _same_bits(ATg, YTg) and bool(torch.isfinite(Yg).all())
    C1, _, pd1, ps1 = _run_proj(3 - tri, P2, YTg, None, yt=False)
    C2, _, pd2, ps2 = _run_proj(3 - tri, P2, ATg, None, yt=False)
    assert _same_bits(C1.get(b, M, n), C2.get(b, M, n)) and _same_bits(ps1.get(b, 2, n), ps2.get(b, 2, n))
    assert pd1.untouched() and pd2.untouched()
    ref = P2.double() @ YTg.double().transpose(-1, -2)
    bound = 2 * (136 + 8) * U * (P2.double().abs() @ YTg.double().abs().transpose(-1, -2))
    assert measured(f'bf16 chain C (tri {3 - tri}) / summation bound', C1.get(b, M, n).double() / bound, ref / bound, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ RBF build

@pytest.mark.parametrize('case', BC.RBF_CASES, ids=BC.case_id)
def test_rbf_build_rounds_the_float64_value_to_the_nearer_bf16(case):
    """Per element: one of the two bf16 neighbours of v = os exp(-s / 2) (float64 from the float32 inputs), and the nearer
    one unless v is within RBF_DELTA v = 2^-15 v of their midpoint -- the derived bound of the kernel's float32 evaluation
    (tests/bf16_cases.py::rbf_inputs).  No share of elements is exempt."""
    _need_gpu()
    from nsgp import _lib
    z, x, ls, os_ = (t.cuda() for t in BC.rbf_inputs(case))
    out = Out(case.batch * case.n * case.M, torch.bfloat16)
    sxb = 0 if case.shared_x else case.n * case.D
    _lib.call('nsgp_rbf_build_t_bf16', _p(z), _p(x), _p(ls), _p(os_), case.batch, case.M, case.n,
              case.D, sxb, out.ptr(), _stream())
    torch.cuda.synchronize()
    got = out.get(case.batch, case.n, case.M).double()
    s, v = BC.rbf_reference(case)
    assert float(s.max()) <= BC.RBF_MAX_S
    neighbour, nearest, decided = BC.rbf_verdict(case, got)
    print(f'[measured] rbf bf16 {BC.case_id(case)}: {int((~neighbour).sum())} not a neighbour, '
          f'{int((~nearest & decided).sum())} decided but not nearest, {int((~nearest & ~decided).sum())} of '
          f'{int((~decided).sum())} in the midpoint zone took the farther one, of {v.numel()}')
    assert bool(neighbour.all())
    assert bool(nearest[decided].all())


def test_rbf_build_argument_checks_launch_nothing():
    _need_gpu()
    from nsgp import _lib
    fn = _lib.load().nsgp_rbf_build_t_bf16
    case = BC.RbfCase(1, 8, 1, 1, True)
    z, x, ls, os_ = (t.cuda() for t in BC.rbf_inputs(case))
    out = Out(8, torch.bfloat16)
    for D in (0, 9):
        assert fn(_p(z), _p(x), _p(ls), _p(os_), 1, 8, 1, D, 0, out.ptr(), _stream()) == -8
    torch.cuda.synchronize()
    assert out.untouched()
