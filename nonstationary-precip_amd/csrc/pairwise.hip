// pairwise.hip -- kernel-matrix builds K[i,j] = k(row_i, col_j) and their backward reductions.
//
//   K1 Gibbs (models/gibbs_kernels.py:154-162), K1' its Matern form (GibbsRadialOp), K2 batched RBF-ARD (gpytorch ScaleKernel(RBF),
//   models/dgps.py:44-46), K3 Paciorek-Schervish D=2 (models/multivariate_gibbs_kernel.py:98-150), K3' its Matern form
//   (PsRadialOp).
//
// Layout: a functor per kernel family (GibbsOp, ArdOp, RbfPeriodicOp, PsOp) is plugged into ONE forward tile kernel and
// ONE backward tile kernel; dispatch_dim is the one place where the runtime D picks the specialised or generic functor.
// The stationary ARD family os * kappa(|(x1 - x2) / ls|) is ONE functor, ArdOp<T, D, Radial>: RBF and Matern differ only
// in the Radial policy.  To add a radial function: one policy struct (eval + negated, see radial.h), one extern "C"
// forward/backward pair over ard_check / ard_fwd / ard_bwd, one ops.py wrapper pair over _ard_build / _ard_build_bwd, one
// _StationaryArdKernel subclass in nsgp/gp/kernels.py.
//
// Forward: HBM-write bound.  One 256-thread workgroup owns a 64 x (64*CPT) tile; a lane owns CPT
// consecutive columns (16 B) so every wave store is one contiguous 1 KiB line group; the column
// operands live in registers for the whole tile and the row operands are computed once per tile and
// broadcast-read from LDS.
// Algorithmic bytes per build: s*(n1*n2 + 2*D*(n1+n2)).
// Measured at N = 16384 (tools/probes/): a torch fill_ writes 6.85 TB/s; this kernel with the arithmetic stubbed out
// reaches 5.8 TB/s (float32) / 6.2 TB/s (float64), and the real Gibbs build 5.7 / 5.0 TB/s -- float32 sits on the
// skeleton's ceiling, float64 still pays ~43 VALU instructions per entry (custom exp and rsqrt in common.h).
// Tried without gain: v_pk_* arithmetic on column pairs, non-temporal stores, 16 x (256*CPT) tiles with the four waves
// side by side (-12 %), an XCD-contiguous tile order.
//
// Backward: one pass over G (dLoss/dK).  A workgroup owns a 64 x 256 tile: wave w walks rows
// w, w+4, ..; a lane covers 4 columns 64 apart (coalesced G reads).  Row-side gradients are
// wave-reduced once per row (amortised over 256 columns), column-side gradients stay in
// registers and are combined across the 4 waves through LDS.  Tile partials go to a workspace and
// a second tiny kernel sums them: deterministic, no atomics.
#include "common.h"
#include "radial.h"

#include <type_traits>

namespace {

template <typename T> struct Cpt;
template <> struct Cpt<float> { static constexpr int v = 4; };
template <> struct Cpt<double> { static constexpr int v = 2; };

template <int D> struct DimMax { static constexpr int v = D ? D : NSGP_MAX_DIM; };

// ------------------------------------------------------------------------------------------
// functors
// ------------------------------------------------------------------------------------------
template <typename T, int D> struct GibbsOp {
    static constexpr int DM = DimMax<D>::v;
    static constexpr int NR = 2 * DM, NC = 2 * DM, NG = 1;
    const T *x1, *x2, *l1, *l2;
    int64_t n1, n2;
    int Drt;
    const T* osp;                          // device scalar or nullptr (= 1)
    __device__ __forceinline__ T os() const { return osp ? osp[0] : T(1); }
    // per-point operands: x, l, q = l^2 and h = sqrt(prod_d sqrt(2) l_d), so that
    //   k = prod_d sqrt(2 l1 l2 / s_d) * exp(-sum_d delta_d^2 / s_d),   s_d = q1_d + q2_d
    //     = h1 h2 rsqrt(S) * exp(-(sum_d delta_d^2 prod_{e != d} s_e) / S),   S = prod_d s_d
    // costs ONE rsqrt and ONE exp per matrix entry (the per-point sqrt is amortised over a tile).
    struct P { T x[DM]; T l[DM]; T q[DM]; T h; };
    __device__ __forceinline__ P point(const T* x, const T* l, int64_t n, int64_t i) const {
        P p;
        T hp = T(1);
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            const bool on = D || d < Drt;
            p.x[d] = on ? x[i * Drt + d] : T(0);
            p.l[d] = on ? l[(int64_t)d * n + i] : T(1);
            p.q[d] = p.l[d] * p.l[d];
            if (on) hp *= T(1.4142135623730951) * p.l[d];
        }
        p.h = t_fsqrt(hp);
        return p;
    }
    __device__ __forceinline__ P row(int64_t, int64_t i) const { return point(x1, l1, n1, i); }
    __device__ __forceinline__ P col(int64_t, int64_t j) const { return point(x2, l2, n2, j); }
    // unscaled kernel value
    __device__ __forceinline__ T base(const P& r, const P& c) const {
        T S = r.q[0] + c.q[0];
        T num = (r.x[0] - c.x[0]) * (r.x[0] - c.x[0]);
#pragma unroll
        for (int d = 1; d < DM; ++d) {
            if (D || d < Drt) {
                const T s = r.q[d] + c.q[d];
                const T df = r.x[d] - c.x[d];
                num = num * s + df * df * S;               // sum_d delta_d^2 prod_{e != d} s_e, built incrementally
                S *= s;
            }
        }
        const T rs = t_rsqrt(S);
        return r.h * c.h * rs * t_fexp(-num * rs * rs);
    }
    __device__ __forceinline__ T eval(int64_t, const P& r, const P& c) const { return os() * base(r, c); }
    // forward-build variants: the output scale is folded into the column operand once per thread
    __device__ __forceinline__ P fcol(int64_t b, int64_t j) const { P p = col(b, j); p.h *= os(); return p; }
    __device__ __forceinline__ T feval(int64_t, const P& r, const P& c) const { return base(r, c); }
    // accumulate g * d k / d(param) into row / col / global accumulators
    __device__ __forceinline__ void grad(int64_t, const P& r, const P& c, T g, T* ra, T* ca, T* ga) const {
        const T kb = base(r, c);
        ga[0] += g * kb;
        const T w = g * kb * os();
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < Drt) {
                const T a = r.l[d], b = c.l[d];
                const T s = a * a + b * b;
                const T inv = T(1) / s;
                const T df = r.x[d] - c.x[d];
                const T q = df * df * inv * inv;          // delta^2 / s^2
                ra[d] += w * (T(0.5) / a - a * inv + T(2) * a * q);
                ca[d] += w * (T(0.5) / b - b * inv + T(2) * b * q);
                const T gx = T(2) * w * df * inv;
                ra[DM + d] -= gx;
                ca[DM + d] += gx;
            }
        }
    }
};

// K2 / K2'' batched stationary ARD kernels  k = os[b] * kappa(s),  s = |u|^2,  u = (x1 - x2) / ls[b]:  ONE functor; the
// radial function kappa is the `Radial` policy of radial.h (RbfRadial, MaternRadial<NU2>).
template <typename T, int D, typename Radial> struct ArdOp {
    static constexpr int DM = DimMax<D>::v;
    static constexpr int NR = DM, NC = DM, NG = DM + 1;
    const T *x1, *x2, *ls, *os;           // ls:(batch,D) os:(batch)
    int64_t n1, n2, sx1, sx2;
    int Drt;
    struct P { T x[DM]; };                // pre-divided by the lengthscale
    __device__ __forceinline__ P point(const T* x, int64_t sx, int64_t b, int64_t i) const {
        P p;
#pragma unroll
        for (int d = 0; d < DM; ++d)
            p.x[d] = (D || d < Drt) ? x[b * sx + i * Drt + d] / ls[b * Drt + d] : T(0);
        return p;
    }
    __device__ __forceinline__ P row(int64_t b, int64_t i) const { return point(x1, sx1, b, i); }
    __device__ __forceinline__ P col(int64_t b, int64_t j) const { return point(x2, sx2, b, j); }
    __device__ __forceinline__ T sq(const P& r, const P& c) const {
        T s = T(0);
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            const T df = r.x[d] - c.x[d];
            s = t_fma(df, df, s);                    // explicit: gemm.hip's generated-Kzx loader repeats this sum bit for bit
        }
        return s;
    }
    __device__ __forceinline__ T eval(int64_t b, const P& r, const P& c) const { return os[b] * Radial::eval(sq(r, c)); }
    __device__ __forceinline__ P fcol(int64_t b, int64_t j) const { return col(b, j); }
    __device__ __forceinline__ T feval(int64_t b, const P& r, const P& c) const { return eval(b, r, c); }
    // row/col accumulators are in units of d/d(x/ls) ("scaled x"); pass 2 divides by ls.
    __device__ __forceinline__ void grad(int64_t b, const P& r, const P& c, T g, T* ra, T* ca, T* ga) const {
        T q;
        const T kb = Radial::eval(sq(r, c), &q);
        ga[DM] += g * kb;
        const T w = g * q * os[b];
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            const T df = r.x[d] - c.x[d];
            if constexpr (Radial::negated) {
                ra[d] -= w * df;
                ca[d] += w * df;
                ga[d] += w * df * df;         // * 1/ls applied in pass 2
            } else {
                ra[d] += w * df;
                ca[d] -= w * df;
                ga[d] -= w * df * df;
            }
        }
    }
};

// K1' non-stationary Matern (Paciorek & Schervish 2006 with Sigma(x) = diag l(x)^2):  k = os * P * kappa(s), the Gibbs
// prefactor P = prod_d sqrt(2 l1 l2 / s_d) = h1 h2 rsqrt(S) times the stationary radial function at the squared distance
// s = 2 sum_d delta_d^2 / s_d = 2 num / S (GibbsOp::base's variables; kappa = e^{-s/2} is GibbsOp itself).  A sibling of
// GibbsOp, not a respelling of it: the per-point operands (P, point, row, col, fcol) and the accumulator layout are
// inherited, so the launchers, the OutDesc wiring, the workspace size and the symmetric mode are GibbsOp's, and GibbsOp's
// own code -- whose float32 bits depend on its spelling under -ffp-contract=fast -- is not touched.
// Per entry: one rsqrt, one distance (matern_dist) and one exp (matern_poly_exp).
// With phi = (d kappa / d d) / d as the policy returns it, q_d = delta_d^2 / s_d^2 and a = l1_d (b = l2_d alike):
//   dk/da    = os P [kappa (1/(2a) - a / s_d) - 2 phi a q_d]
//   dk/dx1_d = 2 os P phi delta_d / s_d = -dk/dx2_d            dk/dos = P kappa
template <typename T, int D, typename Radial> struct GibbsRadialOp : GibbsOp<T, D> {
    using G = GibbsOp<T, D>;
    using P = typename G::P;
    static constexpr int DM = G::DM;
    // the prefactor h1 h2 rsqrt(S) (returned) and the squared distance s.  BWD: s_d from l, not from the stored q -- the
    // backward keeps four column operands per lane, and with q live as well the generic float64 instance spilled
    // (364 B of scratch per lane; the per-dimension reciprocals of grad below were the rest)
    static __device__ __forceinline__ T lsq(T a, T b) { return t_fma(a, a, b * b); }      // s_d, one spelling
    template <bool BWD = false> __device__ __forceinline__ T pre(const P& r, const P& c, T& s) const {
        T S = BWD ? lsq(r.l[0], c.l[0]) : r.q[0] + c.q[0];
        T num = (r.x[0] - c.x[0]) * (r.x[0] - c.x[0]);
#pragma unroll
        for (int d = 1; d < DM; ++d) {
            if (D || d < this->Drt) {
                const T sd = BWD ? lsq(r.l[d], c.l[d]) : r.q[d] + c.q[d];
                const T df = r.x[d] - c.x[d];
                // explicit: left to -ffp-contract the compiler fused this sum for two of a lane's four float32 columns
                // and not for the other two (nu = 5/2, D = 2), and K(x, x) was symmetric to several ulp only
                num = t_fma(df * df, S, num * sd);
                S *= sd;
            }
        }
        const T rs = t_rsqrt(S);
        s = T(2) * num * rs * rs;
        return r.h * c.h * rs;
    }
    __device__ __forceinline__ T base(const P& r, const P& c) const {
        T s;
        const T p = pre(r, c, s);
        return p * Radial::eval(s);
    }
    __device__ __forceinline__ T eval(int64_t, const P& r, const P& c) const { return this->os() * base(r, c); }
    __device__ __forceinline__ T feval(int64_t, const P& r, const P& c) const { return base(r, c); }
    __device__ __forceinline__ void grad(int64_t, const P& r, const P& c, T g, T* ra, T* ca, T* ga) const {
        T s, q;
        const T p = this->template pre<true>(r, c, s);
        const T kap = Radial::eval(s, &q);
        ga[0] += g * (p * kap);
        const T w = g * p * this->os();
        const T wk = w * kap, wq = w * q;             // wq = w phi, or -w phi for a negated policy
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < this->Drt) {
                // one division per dimension: u = 1 / (2 a b s_d) gives 1 / s_d = 2 a b u, and
                // 1/(2a) - a / s_d = -b t,  1/(2b) - b / s_d = a t  with  t = (a - b)(a + b) u
                const T a = r.l[d], b = c.l[d];
                const T sd = lsq(a, b);
                const T ab2 = T(2) * a * b;
                const T u = T(1) / (ab2 * sd);
                const T inv = ab2 * u;
                const T t = wk * ((a - b) * (a + b) * u);
                const T df = r.x[d] - c.x[d];
                const T gx = T(2) * wq * df * inv;                   // 2 w (+-phi) delta / s_d
                const T qd = gx * df * inv;                          // 2 w (+-phi) delta^2 / s_d^2
                if constexpr (Radial::negated) {
                    ra[d] += a * qd - b * t;
                    ca[d] += b * qd + a * t;
                    ra[DM + d] -= gx;
                    ca[DM + d] += gx;
                } else {
                    ra[d] -= a * qd + b * t;
                    ca[d] += a * t - b * qd;
                    ra[DM + d] += gx;
                    ca[DM + d] -= gx;
                }
            }
        }
    }
};

// K2' batched  os * RBF-ARD(x; ls_r) * Periodic(x; ls_p, period):
//   k = os * exp(-1/2 sum_d ((x_d - x'_d)/ls_r,d)^2) * exp(-2 sin^2(pi |x - x'| / period) / ls_p)
// (gpytorch PeriodicKernel < 1.9 as recalled in SURVEY A.2/A.7: Euclidean distance of x / period, division by
// the lengthscale, not its square).  One launch builds ScaleKernel(RBFKernel * PeriodicKernel) of
// models/spatio_temporal_models.py:22,42 and experiments/temporal_exp.py:39; ls_r == nullptr drops the RBF
// factor (plain PeriodicKernel), os == nullptr means 1.
template <typename T, int D> struct RbfPeriodicOp {
    static constexpr int DM = DimMax<D>::v;
    static constexpr int NR = DM, NC = DM, NG = DM + 3;        // globals: ls_r[D], ls_p, period, os
    const T *x1, *x2, *lsr, *lsp, *per, *os;
    int64_t n1, n2, sx1, sx2;
    int Drt;
    struct P { T x[DM]; };
    __device__ __forceinline__ P point(const T* x, int64_t sx, int64_t b, int64_t i) const {
        P p;
#pragma unroll
        for (int d = 0; d < DM; ++d) p.x[d] = (D || d < Drt) ? x[b * sx + i * Drt + d] : T(0);
        return p;
    }
    __device__ __forceinline__ P row(int64_t b, int64_t i) const { return point(x1, sx1, b, i); }
    __device__ __forceinline__ P col(int64_t b, int64_t j) const { return point(x2, sx2, b, j); }
    // exponent pieces: q = sum_d (delta_d / ls_r,d)^2, r = |delta|, (s, c) = sincos(pi r / period)
    __device__ __forceinline__ T base(int64_t b, const P& r, const P& c, T& rr, T& sn, T& cs) const {
        T q = T(0), r2 = T(0);
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < Drt) {
                const T df = r.x[d] - c.x[d];
                r2 += df * df;
                if (lsr) { const T il = T(1) / lsr[b * Drt + d]; q += df * df * il * il; }
            }
        }
        rr = t_sqrt(r2);
        const T u = T(3.14159265358979323846) * rr / per[b];
        sn = sin(u); cs = cos(u);
        return t_exp(T(-0.5) * q - T(2) * sn * sn / lsp[b]);
    }
    __device__ __forceinline__ T eval(int64_t b, const P& r, const P& c) const {
        T rr, sn, cs;
        const T k = base(b, r, c, rr, sn, cs);
        return os ? os[b] * k : k;
    }
    __device__ __forceinline__ P fcol(int64_t b, int64_t j) const { return col(b, j); }
    __device__ __forceinline__ T feval(int64_t b, const P& r, const P& c) const { return eval(b, r, c); }
    __device__ __forceinline__ void grad(int64_t b, const P& r, const P& c, T g, T* ra, T* ca, T* ga) const {
        T rr, sn, cs;
        const T kb = base(b, r, c, rr, sn, cs);
        ga[DM + 2] += g * kb;                                              // d/d os
        const T w = g * kb * (os ? os[b] : T(1));
        const T ilp = T(1) / lsp[b], ip = T(1) / per[b];
        ga[DM] += w * T(2) * sn * sn * ilp * ilp;                          // d/d ls_p
        const T dsdu = T(4) * ilp * sn * cs * T(3.14159265358979323846);   // -(d exponent / d u), u = pi r / period
        ga[DM + 1] += w * dsdu * rr * ip * ip;                             // d/d period  (du/dp = -pi r / p^2)
        const T dr = rr > T(0) ? dsdu * ip / rr : T(0);                    // -(d exponent / d r) / r
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < Drt) {
                const T df = r.x[d] - c.x[d];
                T gx = -dr * df;                                           // d exponent / d x1_d (periodic part)
                if (lsr) {
                    const T il = T(1) / lsr[b * Drt + d];
                    gx -= df * il * il;
                    ga[d] += w * df * df * il * il * il;                   // d/d ls_r,d
                }
                ra[d] += w * gx;
                ca[d] -= w * gx;
            }
        }
    }
};

// K2''' batched  os * kappa(s) * Periodic(x; ls_p, period),  s = sum_d (delta_d / ls_e,d)^2:  the temporal kernel with a
// radial envelope from radial.h in place of the squared exponential,
//   k = os kappa(s) E,   E = exp(-2 sin^2(theta) / ls_p),   theta = pi |delta| / period.
// A sibling of RbfPeriodicOp as GibbsRadialOp is of GibbsOp: the members, the per-point operands (P, point, row, col,
// fcol) and the accumulator layout (NR / NC / NG: ls_e[D], ls_p, period, os) are inherited, so the launchers, the OutDesc
// wiring (rbfper_launch_bwd), the workspace size and the one-buffer symmetric mode are RbfPeriodicOp's, and
// RbfPeriodicOp's own code is not touched.  `lsr` is the envelope lengthscale and is required (the entry points check).
// E is RbfPeriodicOp's spelling (library sin / cos / exp, division by ls_p); kappa, its range, far tail (0 * E with
// E <= 1, never inf * 0), NaN behaviour and phi(0) = 0 for nu = 1/2 are the policy's.  The two sums are explicit fmas:
// forward and backward see one s and one r per entry, whatever -ffp-contract makes of the neighbouring code.
// With phi = (d kappa / d d) / d as the policy returns it, u_d = delta_d / ls_e,d and c = (4 / ls_p) sin cos pi:
//   dk/dx1_d = os E phi u_d / ls_e,d - k (c / period) delta_d / r = -dk/dx2_d        (second term 0 at r = 0)
//   dk/dls_e,d = -os E phi u_d^2 / ls_e,d    dk/dls_p = k 2 sin^2 / ls_p^2    dk/dperiod = k c r / period^2    dk/dos = kappa E
// An entry with delta = 0 (the diagonal of K(x, x)) has u = 0, r = 0 and sin = 0: every term but dk/dos is exactly 0.
template <typename T, int D, typename Radial> struct RadialPeriodicOp : RbfPeriodicOp<T, D> {
    using B = RbfPeriodicOp<T, D>;
    using P = typename B::P;
    static constexpr int DM = B::DM;
    // the periodic factor E (returned) and the pieces of one entry: s, r = |delta|, (sn, cs) = sincos(theta)
    __device__ __forceinline__ T base(int64_t b, const P& r, const P& c, T& s, T& rr, T& sn, T& cs) const {
        T q = T(0), r2 = T(0);
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < this->Drt) {
                const T df = r.x[d] - c.x[d];
                const T u = df * (T(1) / this->lsr[b * this->Drt + d]);
                r2 = t_fma(df, df, r2);
                q = t_fma(u, u, q);
            }
        }
        s = q;
        rr = t_sqrt(r2);
        const T th = T(3.14159265358979323846) * rr / this->per[b];
        sn = sin(th); cs = cos(th);
        return t_exp(T(-2) * sn * sn / this->lsp[b]);
    }
    __device__ __forceinline__ T eval(int64_t b, const P& r, const P& c) const {
        T s, rr, sn, cs;
        const T e = base(b, r, c, s, rr, sn, cs);
        const T k = Radial::eval(s) * e;
        return this->os ? this->os[b] * k : k;
    }
    __device__ __forceinline__ T feval(int64_t b, const P& r, const P& c) const { return eval(b, r, c); }
    __device__ __forceinline__ void grad(int64_t b, const P& r, const P& c, T g, T* ra, T* ca, T* ga) const {
        T s, rr, sn, cs, q;
        const T e = base(b, r, c, s, rr, sn, cs);
        const T kap = Radial::eval(s, &q);
        ga[DM + 2] += g * (kap * e);                                       // d/d os
        const T we = g * e * (this->os ? this->os[b] : T(1));
        const T w = we * kap, wq = we * q;                                 // g k;  g os E phi (-phi for a negated policy)
        const T ilp = T(1) / this->lsp[b], ip = T(1) / this->per[b];
        ga[DM] += w * T(2) * sn * sn * ilp * ilp;                          // d/d ls_p
        const T dsdu = T(4) * ilp * sn * cs * T(3.14159265358979323846);   // c: -(d log E / d theta)
        ga[DM + 1] += w * dsdu * rr * ip * ip;                             // d/d period  (d theta / dp = -pi r / p^2)
        const T wr = rr > T(0) ? w * dsdu * ip / rr : T(0);                // g k (c / period) / r
#pragma unroll
        for (int d = 0; d < DM; ++d) {
            if (D || d < this->Drt) {
                const T df = r.x[d] - c.x[d];
                const T il = T(1) / this->lsr[b * this->Drt + d];
                const T u = df * il;
                const T gu = wq * u * il;                                  // g os E (+-phi) u_d / ls_e,d
                if constexpr (Radial::negated) {
                    const T gx = -gu - wr * df;
                    ra[d] += gx; ca[d] -= gx;
                    ga[d] += gu * u;                                       // d/d ls_e,d
                } else {
                    const T gx = gu - wr * df;
                    ra[d] += gx; ca[d] -= gx;
                    ga[d] -= gu * u;
                }
            }
        }
    }
};

template <typename T> struct PsOp {
    static constexpr int NR = 4, NC = 4, NG = 1;      // NG unused (kept 1 for array sizing)
    const T *x1, *x2, *s1, *s2;
    T jit;
    struct P { T x[2]; T s[4]; T q;  /* det^(1/4) */ };
    __device__ __forceinline__ P load(const T* x, const T* s, int64_t i) const {
        P p;
        p.x[0] = x[2 * i]; p.x[1] = x[2 * i + 1];
#pragma unroll
        for (int k = 0; k < 4; ++k) p.s[k] = s[4 * i + k];
        const T det = p.s[0] * p.s[3] - p.s[1] * p.s[2];
        p.q = t_sqrt(t_sqrt(det));
        return p;
    }
    __device__ __forceinline__ P row(int64_t, int64_t i) const { return load(x1, s1, i); }
    __device__ __forceinline__ P col(int64_t, int64_t j) const { return load(x2, s2, j); }
    __device__ __forceinline__ P fcol(int64_t b, int64_t j) const { return col(b, j); }
    __device__ __forceinline__ T feval(int64_t b, const P& r, const P& c) const { return eval(b, r, c); }
    __device__ __forceinline__ T eval(int64_t, const P& r, const P& c) const {
        const T a0 = T(0.5) * (r.s[0] + c.s[0]), a1 = T(0.5) * (r.s[1] + c.s[1]);
        const T a2 = T(0.5) * (r.s[2] + c.s[2]), a3 = T(0.5) * (r.s[3] + c.s[3]);
        const T detA = a0 * a3 - a1 * a2;
        const T b0 = a0 + jit, b3 = a3 + jit;
        const T detB = b0 * b3 - a1 * a2;
        const T d0 = r.x[0] - c.x[0], d1 = r.x[1] - c.x[1];
        const T quad = (b3 * d0 * d0 - (a1 + a2) * d0 * d1 + b0 * d1 * d1) / detB;
        return r.q * c.q / t_sqrt(detA) * t_exp(-quad);
    }
    __device__ __forceinline__ void grad(int64_t, const P& r, const P& c, T g, T* ra, T* ca, T*) const {
        const T a0 = T(0.5) * (r.s[0] + c.s[0]), a1 = T(0.5) * (r.s[1] + c.s[1]);
        const T a2 = T(0.5) * (r.s[2] + c.s[2]), a3 = T(0.5) * (r.s[3] + c.s[3]);
        const T detA = a0 * a3 - a1 * a2;
        const T b0 = a0 + jit, b3 = a3 + jit;
        const T detB = b0 * b3 - a1 * a2;
        const T d0 = r.x[0] - c.x[0], d1 = r.x[1] - c.x[1];
        const T quad = (b3 * d0 * d0 - (a1 + a2) * d0 * d1 + b0 * d1 * d1) / detB;
        const T k = r.q * c.q / t_sqrt(detA) * t_exp(-quad);
        const T w = g * k;
        // B^-1 d  and  B^-T d
        const T iB = T(1) / detB;
        const T v0 = (b3 * d0 - a1 * d1) * iB, v1 = (-a2 * d0 + b0 * d1) * iB;     // B^-1 d
        const T u0 = (b3 * d0 - a2 * d1) * iB, u1 = (-a1 * d0 + b0 * d1) * iB;     // B^-T d
        // shared term: -1/4 A^-T + 1/2 u v^T
        const T iA = T(0.25) / detA;
        const T sh0 = -iA * a3 + T(0.5) * u0 * v0;
        const T sh1 = iA * a2 + T(0.5) * u0 * v1;
        const T sh2 = iA * a1 + T(0.5) * u1 * v0;
        const T sh3 = -iA * a0 + T(0.5) * u1 * v1;
        const T dr = T(0.25) / (r.s[0] * r.s[3] - r.s[1] * r.s[2]);
        const T dc = T(0.25) / (c.s[0] * c.s[3] - c.s[1] * c.s[2]);
        ra[0] += w * (sh0 + dr * r.s[3]); ra[1] += w * (sh1 - dr * r.s[2]);
        ra[2] += w * (sh2 - dr * r.s[1]); ra[3] += w * (sh3 + dr * r.s[0]);
        ca[0] += w * (sh0 + dc * c.s[3]); ca[1] += w * (sh1 - dc * c.s[2]);
        ca[2] += w * (sh2 - dc * c.s[1]); ca[3] += w * (sh3 + dc * c.s[0]);
    }
};

// K3' Paciorek & Schervish (2006) with a full per-point 2x2 Sigma(x) and the Matern radial function:  k = P * kappa(s),
// PsOp's prefactor P = |S1|^(1/4) |S2|^(1/4) |A|^(-1/2) times the stationary radial function at the squared distance
// s = 2 Q, Q = delta^T B^-1 delta, A = (S1 + S2) / 2, B = A + jit I (kappa = e^{-s/2} = e^{-Q} is PsOp itself; the Matern
// argument is d = sqrt(2 Q), P&S's 2 sqrt(nu Q) = sqrt(2 nu) d).  A sibling of PsOp as GibbsRadialOp is of GibbsOp: the
// per-point operands (P, load, row, col, fcol) and the accumulator layout are inherited, so the launchers, the OutDesc
// wiring and the workspace size are PsOp's, and PsOp's own code is not touched.  Sigma is not assumed symmetric, the
// jitter enters the inverse only, and Q < 0 (a Sigma that is not positive definite) is evaluated as Q = 0: k = P, and the
// distance term of the gradient is dropped; a NaN stays NaN (the test is false for it).
// Per entry: one reciprocal (det B), one rsqrt (det A), one distance (matern_dist) and one exp (matern_poly_exp).
// With phi = (d kappa / d d) / d as the policy returns it, u = B^-T delta, v = B^-1 delta:
//   dk/dS1 = P [kappa (S1^-T - A^-T) / 4 - phi u v^T / 2],   S2 alike with S2^-T.
template <typename T, typename Radial> struct PsRadialOp : PsOp<T> {
    using P = typename PsOp<T>::P;
    static_assert(!Radial::negated, "the policy writes phi");
    // P (returned), s and the 2x2 pieces of one entry: ONE statement for eval and grad
    struct Pieces { T a[4]; T b0, b3, d0, d1, iB, detA; bool neg; };
    static __device__ __forceinline__ T det2(T m0, T m1, T m2, T m3) { return t_fma(m0, m3, -(m1 * m2)); }
    __device__ __forceinline__ T pre(const P& r, const P& c, T& s, Pieces& e) const {
#pragma unroll
        for (int k = 0; k < 4; ++k) e.a[k] = T(0.5) * (r.s[k] + c.s[k]);
        e.b0 = e.a[0] + this->jit; e.b3 = e.a[3] + this->jit;
        e.iB = t_rcp(det2(e.b0, e.a[1], e.a[2], e.b3));
        e.d0 = r.x[0] - c.x[0]; e.d1 = r.x[1] - c.x[1];
        const T s2 = T(2) * (e.b3 * e.d0 * e.d0 - (e.a[1] + e.a[2]) * e.d0 * e.d1 + e.b0 * e.d1 * e.d1) * e.iB;
        e.neg = s2 < T(0);
        s = e.neg ? T(0) : s2;
        e.detA = det2(e.a[0], e.a[1], e.a[2], e.a[3]);
        return r.q * c.q * t_rsqrt(e.detA);
    }
    __device__ __forceinline__ T eval(int64_t, const P& r, const P& c) const {
        T s;
        Pieces e;
        const T p = pre(r, c, s, e);
        return p * Radial::eval(s);
    }
    __device__ __forceinline__ T feval(int64_t b, const P& r, const P& c) const { return eval(b, r, c); }
    // 1 / (4 det) of det A, det S1 and det S2: ONE spelling (see prod_diff).  float: v_rcp_f32, one instruction; double: from
    // rsqrt(det), since a float64 division costs twice t_rsqrt.  det < 0 has no prefactor (NaN) either way.
    static __device__ __forceinline__ T quarter_inv(T det) {
        if constexpr (sizeof(T) == 4) return T(0.25) * t_rcp(det);
        const T rs = t_rsqrt(det);
        return T(0.25) * rs * rs;
    }
    // m n - p q with both products rounded, never fused: exactly 0 for (m, n) == (p, q), so that an entry with delta = 0
    // and S1 == S2 bit for bit (the diagonal of K(x, x)) adds exactly nothing to the gradient
    static __device__ __forceinline__ T prod_diff(T m, T n, T p, T q) {
#pragma clang fp contract(off)
        const T mn = m * n, pq = p * q;
        return mn - pq;
    }
    __device__ __forceinline__ void grad(int64_t, const P& r, const P& c, T g, T* ra, T* ca, T*) const {
        T s, q;
        Pieces e;
        const T p = pre(r, c, s, e);
        const T kap = Radial::eval(s, &q);
        const T w = g * p;
        const T wk = w * kap;
        const T h = e.neg ? T(0) : T(-0.5) * w * q;                                  // -1/2 g P phi
        const T v0 = (e.b3 * e.d0 - e.a[1] * e.d1) * e.iB, v1 = (e.b0 * e.d1 - e.a[2] * e.d0) * e.iB;      // B^-1 delta
        const T u0 = (e.b3 * e.d0 - e.a[2] * e.d1) * e.iB, u1 = (e.b0 * e.d1 - e.a[1] * e.d0) * e.iB;      // B^-T delta
        const T hu0 = h * u0, hu1 = h * u1;
        const T t0 = hu0 * v0, t1 = hu0 * v1, t2 = hu1 * v0, t3 = hu1 * v1;
        const T iA = quarter_inv(e.detA);
        const T dr = quarter_inv(det2(r.s[0], r.s[1], r.s[2], r.s[3]));
        const T dc = quarter_inv(det2(c.s[0], c.s[1], c.s[2], c.s[3]));
        ra[0] += wk * prod_diff(dr, r.s[3], iA, e.a[3]) + t0; ra[1] += wk * prod_diff(iA, e.a[2], dr, r.s[2]) + t1;
        ra[2] += wk * prod_diff(iA, e.a[1], dr, r.s[1]) + t2; ra[3] += wk * prod_diff(dr, r.s[0], iA, e.a[0]) + t3;
        ca[0] += wk * prod_diff(dc, c.s[3], iA, e.a[3]) + t0; ca[1] += wk * prod_diff(iA, e.a[2], dc, c.s[2]) + t1;
        ca[2] += wk * prod_diff(iA, e.a[1], dc, c.s[1]) + t2; ca[3] += wk * prod_diff(dc, c.s[0], iA, e.a[0]) + t3;
    }
};

// ------------------------------------------------------------------------------------------
// forward tile kernel
// ------------------------------------------------------------------------------------------
constexpr int FWD_TI = 64;

template <typename T, typename Op>
__global__ __launch_bounds__(256) void pairwise_fwd_kernel(Op op, int64_t n1, int64_t n2, T diag_add_v,
                                                           const T* __restrict__ diag_add_p,
                                                           T* __restrict__ K, int64_t ldk, int64_t sK, int vec_ok) {
    constexpr int CPT = Cpt<T>::v;
    __shared__ typename Op::P rows_s[FWD_TI];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.z;
    const int64_t jb = (int64_t)blockIdx.x * 64 * CPT;
    const int64_t j0 = jb + (int64_t)lane * CPT;
    const int64_t i0 = (int64_t)blockIdx.y * FWD_TI;
    // column operands first (clamped indices, so every thread may load): their global-load latency overlaps the row
    // operands' -- a tile is short (N = 4096: 1024 workgroups, all resident at once, ~20 us), two dependent
    // latencies in front of the first store were a tenth of the launch
    typename Op::P cols[CPT];
#pragma unroll
    for (int c = 0; c < CPT; ++c) cols[c] = op.fcol(b, j0 + c < n2 ? j0 + c : n2 - 1);
    const T diag_add = diag_add_p ? diag_add_p[0] : diag_add_v;
    // row operands of the tile: computed once (one thread per row), then broadcast-read from LDS
    if (threadIdx.x < FWD_TI && i0 + threadIdx.x < n1) rows_s[threadIdx.x] = op.row(b, i0 + threadIdx.x);
    __syncthreads();
    if (j0 >= n2) return;
    T* Kb = K + b * sK;
    const bool full = vec_ok && (j0 + CPT <= n2);
    const int rmax = (int)(n1 - i0 < FWD_TI ? n1 - i0 : FWD_TI);
    // only tiles that cross the diagonal test for it (block-uniform)
    const bool on_diag = i0 < jb + 64 * CPT && jb < i0 + FWD_TI;
    auto entry = [&](int r, T (&v)[CPT]) {
        const typename Op::P rp = rows_s[r];
#pragma unroll
        for (int c = 0; c < CPT; ++c) v[c] = op.feval(b, rp, cols[c]);
        if (on_diag) {
#pragma unroll
            for (int c = 0; c < CPT; ++c) if (i0 + r == j0 + c) v[c] += diag_add;
        }
    };
    if (full) {
#pragma unroll 2
        for (int r = w; r < rmax; r += 4) {
            T v[CPT];
            entry(r, v);
            T* dst = Kb + (i0 + r) * ldk + j0;
            if constexpr (CPT == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            else *reinterpret_cast<double2*>(dst) = make_double2(v[0], v[1]);
        }
    } else {
        for (int r = w; r < rmax; r += 4) {
            T v[CPT];
            entry(r, v);
            T* dst = Kb + (i0 + r) * ldk + j0;
#pragma unroll
            for (int c = 0; c < CPT; ++c) if (j0 + c < n2) dst[c] = v[c];
        }
    }
}

template <typename T, typename Op>
int launch_fwd(const Op& op, int64_t batch, int64_t n1, int64_t n2, T diag_add, const T* diag_add_p, T* K,
               int64_t ldk, int64_t sK, void* stream) {
    if (n1 == 0 || n2 == 0 || batch == 0) return 0;
    constexpr int CPT = Cpt<T>::v;
    const int vec_ok = (ldk % CPT == 0) && (sK % CPT == 0) && ((uintptr_t)K % (CPT * sizeof(T)) == 0);
    dim3 grid((unsigned)cdiv64(n2, 64 * CPT), (unsigned)cdiv64(n1, FWD_TI), (unsigned)batch);
    hipLaunchKernelGGL((pairwise_fwd_kernel<T, Op>), grid, dim3(256), 0, (hipStream_t)stream, op, n1, n2,
                       diag_add, diag_add_p, K, ldk, sK, vec_ok);
    return nsgp_launch_status();
}

// ------------------------------------------------------------------------------------------
// backward tile kernel (pass 1) and partial reduction (pass 2)
// ------------------------------------------------------------------------------------------
constexpr int BWD_TI = 64, BWD_TJ = 256;
// Rows per backward workgroup: 64, or 16 when the 64-row grid would leave most of the 256 CUs idle (e.g. the float64
// Kzz adjoint of the DSVI step: 1024 x 1024 x 2 GPs = 128 workgroups of 64 x 256 entries took 28 us, latency-bound).
static inline int bwd_rows(int64_t batch, int64_t n1, int64_t n2) {
    return batch * cdiv64(n1, BWD_TI) * cdiv64(n2, BWD_TJ) < 256 ? 16 : BWD_TI;
}
// The backward launch of a (batch, n1, n2) problem: the ONE place launch_bwd, bwd_ws_elems and nsgp_pairwise_bwd_plan take
// it from.  Grid (ntj, nti, batch); the workspace holds ntj row-side, nti column-side and nti * ntj global partials.
struct BwdPlan { int rows; int64_t nti, ntj; };
static inline BwdPlan bwd_plan(int64_t batch, int64_t n1, int64_t n2) {
    const int rows = bwd_rows(batch, n1, n2);
    return {rows, cdiv64(n1, rows), cdiv64(n2, BWD_TJ)};
}

template <typename T, typename Op, int TI>
__global__ __launch_bounds__(256) void pairwise_bwd_kernel(Op op, int64_t n1, int64_t n2,
                                                           const T* __restrict__ G, int64_t ldg, int64_t sG,
                                                           T* __restrict__ P1, T* __restrict__ P2,
                                                           T* __restrict__ PG) {
    constexpr int NR = Op::NR, NC = Op::NC, NG = Op::NG;
    __shared__ T lds[256 * NC];
    __shared__ T lds_g[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.z;
    const int64_t tj = blockIdx.x, ti = blockIdx.y;
    const int64_t ntj = gridDim.x, nti = gridDim.y;
    const int64_t j0 = tj * BWD_TJ, i0 = ti * TI;
    const T* Gb = G + b * sG;

    typename Op::P cols[4];
    bool cok[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t j = j0 + c * 64 + lane;
        cok[c] = j < n2;
        cols[c] = op.col(b, cok[c] ? j : n2 - 1);
    }
    T ca[4][NC];
    T ga[NG];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < NC; ++k) ca[c][k] = T(0);
#pragma unroll
    for (int k = 0; k < NG; ++k) ga[k] = T(0);

    for (int r = w; r < TI; r += 4) {
        const int64_t i = i0 + r;
        if (i >= n1) break;                         // wave-uniform
        const typename Op::P rp = op.row(b, i);
        T ra[NR];
#pragma unroll
        for (int k = 0; k < NR; ++k) ra[k] = T(0);
        T gv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) gv[c] = cok[c] ? Gb[i * ldg + j0 + c * 64 + lane] : T(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) op.grad(b, rp, cols[c], gv[c], ra, ca[c], ga);
#pragma unroll
        for (int k = 0; k < NR; ++k) ra[k] = wave_sum(ra[k]);
        if (lane == 0) {
            T* dst = P1 + ((b * ntj + tj) * n1 + i) * NR;
#pragma unroll
            for (int k = 0; k < NR; ++k) dst[k] = ra[k];
        }
    }
    // column side: combine the 4 waves through LDS, one chunk of 64 columns at a time
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        for (int ww = 0; ww < 4; ++ww) {
            if (w == ww) {
#pragma unroll
                for (int k = 0; k < NC; ++k) {
                    T* p = &lds[(c * 64 + lane) * NC + k];
                    *p = (ww == 0) ? ca[c][k] : (*p + ca[c][k]);
                }
            }
            __syncthreads();
        }
    }
    {
        const int64_t j = j0 + threadIdx.x;
        if (j < n2) {
            T* dst = P2 + ((b * nti + ti) * n2 + j) * NC;
#pragma unroll
            for (int k = 0; k < NC; ++k) dst[k] = lds[threadIdx.x * NC + k];
        }
    }
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const T s = block_sum_256(ga[k], lds_g);
        if (threadIdx.x == 0) PG[((b * nti + ti) * ntj + tj) * NG + k] = s;
    }
}

// out descriptor for pass 2: value k of item i goes to ptr[k][b*bstride[k] + i*stride[k]] * scale
template <typename T> struct OutDesc {
    T* ptr[2 * NSGP_MAX_DIM];
    int64_t stride[2 * NSGP_MAX_DIM];
    int64_t bstride[2 * NSGP_MAX_DIM];
    const T* div[2 * NSGP_MAX_DIM];       // optional per-batch divisor array (RBF: lengthscale), index b*divstride+divoff
    int64_t divstride[2 * NSGP_MAX_DIM];
    int64_t divoff[2 * NSGP_MAX_DIM];
    int nval;
};

// out[item] = sum_t P[t][item]: a workgroup is 32 consecutive items x 8 partial-sum chains (the tile partials of an
// item are `ntiles` strided loads; one serial chain of 160 dependent-latency loads took 40 us at n2 = 40960), combined
// through LDS in a fixed order (deterministic).
template <typename T>
__device__ __forceinline__ void reduce_items_body(const T* __restrict__ P, int64_t ntiles, int64_t n,
                                                  const OutDesc<T>& od, int64_t blk, int64_t b, T (*lds)[33],
                                                  const T* __restrict__ Pb = nullptr, int64_t ntb = 0) {
    const int ix = threadIdx.x & 31, cy = threadIdx.x >> 5;
    const int64_t idx = blk * 32 + ix;
    const int64_t tot = n * od.nval;
    T s = T(0);
    if (idx < tot) {
        const T* p = P + b * ntiles * tot + idx;
        for (int64_t t = cy; t < ntiles; t += 8) s += p[t * tot];
        if (Pb) {                                         // symmetric case: the other side's partials of the same item
            const T* q = Pb + b * ntb * tot + idx;
            for (int64_t t = cy; t < ntb; t += 8) s += q[t * tot];
        }
    }
    lds[cy][ix] = s;
    __syncthreads();
    if (cy != 0 || idx >= tot) return;
    const int64_t i = idx / od.nval;
    const int k = (int)(idx % od.nval);
    if (!od.ptr[k]) return;
#pragma unroll
    for (int c = 1; c < 8; ++c) s += lds[c][ix];
    if (od.div[k]) s /= od.div[k][b * od.divstride[k] + od.divoff[k]];
    od.ptr[k][b * od.bstride[k] + i * od.stride[k]] = s;
}

// ONE launch for the three reductions behind a backward tile pass (workgroups [0, nblk1): row items, [nblk1, nblk1 +
// nblk2): column items, the last one: the global values of this batch entry, summing `nparts` partials of `nval` values).
template <typename T>
__global__ __launch_bounds__(256) void reduce_all_kernel(const T* __restrict__ P1, int64_t ntj, int64_t n1,
                                                         OutDesc<T> rows, const T* __restrict__ P2, int64_t nti,
                                                         int64_t n2, OutDesc<T> cols, const T* __restrict__ PG,
                                                         int64_t nparts, OutDesc<T> globs, int64_t nblk1,
                                                         int64_t nblk2) {
    __shared__ T lds[8][33];
    const int64_t b = blockIdx.z, blk = blockIdx.x;
    if (blk < nblk1) { reduce_items_body<T>(P1, ntj, n1, rows, blk, b, lds, nblk2 == 0 ? P2 : nullptr, nti); return; }
    if (blk < nblk1 + nblk2) { reduce_items_body<T>(P2, nti, n2, cols, blk - nblk1, b, lds); return; }
    T* l4 = &lds[0][0];
    for (int k = 0; k < globs.nval; ++k) {
        T s = T(0);
        for (int64_t t = threadIdx.x; t < nparts; t += 256) s += PG[(b * nparts + t) * globs.nval + k];
        s = block_sum_256(s, l4);
        if (threadIdx.x == 0 && globs.ptr[k]) {
            if (globs.div[k]) s /= globs.div[k][b * globs.divstride[k] + globs.divoff[k]];
            globs.ptr[k][b * globs.bstride[k]] = s;
        }
        __syncthreads();
    }
}

template <typename Op> size_t bwd_ws_elems(int64_t batch, int64_t n1, int64_t n2) {
    const BwdPlan p = bwd_plan(batch, n1, n2);
    return (size_t)(batch * (p.ntj * n1 * Op::NR + p.nti * n2 * Op::NC + p.nti * p.ntj * Op::NG));
}

template <typename T, typename Op>
int launch_bwd(const Op& op, int64_t batch, int64_t n1, int64_t n2, const T* G, int64_t ldg, int64_t sG,
               const OutDesc<T>& rows, const OutDesc<T>& cols, const OutDesc<T>& globs,
               void* ws, size_t ws_bytes, void* stream) {
    if (n1 == 0 || n2 == 0 || batch == 0) return 0;
    const BwdPlan plan = bwd_plan(batch, n1, n2);
    const int ti_rows = plan.rows;
    const int64_t ntj = plan.ntj, nti = plan.nti;
    if (ws_bytes < bwd_ws_elems<Op>(batch, n1, n2) * sizeof(T) || !ws) return -100;
    T* P1 = (T*)ws;
    T* P2 = P1 + batch * ntj * n1 * Op::NR;
    T* PG = P2 + batch * nti * n2 * Op::NC;
    hipStream_t st = (hipStream_t)stream;
    if (ti_rows == 16)
        hipLaunchKernelGGL((pairwise_bwd_kernel<T, Op, 16>), dim3((unsigned)ntj, (unsigned)nti, (unsigned)batch),
                           dim3(256), 0, st, op, n1, n2, G, ldg, sG, P1, P2, PG);
    else
        hipLaunchKernelGGL((pairwise_bwd_kernel<T, Op, BWD_TI>), dim3((unsigned)ntj, (unsigned)nti, (unsigned)batch),
                           dim3(256), 0, st, op, n1, n2, G, ldg, sG, P1, P2, PG);
    // x1 == x2 with ONE gradient buffer for both sides (rows and cols describe the same outputs): the row-side blocks
    // add the column-side partials of their item and no column-side blocks run
    bool sym = n1 == n2 && Op::NR == Op::NC;
    bool any = false;
    for (int k = 0; sym && k < Op::NR; ++k) {
        sym = rows.ptr[k] == cols.ptr[k] && rows.stride[k] == cols.stride[k] && rows.bstride[k] == cols.bstride[k];
        any = any || rows.ptr[k] != nullptr;
    }
    sym = sym && any;
    const int64_t nblk1 = cdiv64(n1 * Op::NR, 32), nblk2 = sym ? 0 : cdiv64(n2 * Op::NC, 32);
    hipLaunchKernelGGL((reduce_all_kernel<T>), dim3((unsigned)(nblk1 + nblk2 + (globs.nval > 0 ? 1 : 0)), 1, (unsigned)batch),
                       dim3(256), 0, st, (const T*)P1, ntj, n1, rows, (const T*)(sym || nblk2 ? P2 : nullptr), nti, n2, cols,
                       (const T*)PG, nti * ntj, globs, nblk1, nblk2);
    return nsgp_launch_status();
}

template <typename T> OutDesc<T> empty_desc(int nval) {
    OutDesc<T> d;
    for (int k = 0; k < 2 * NSGP_MAX_DIM; ++k) {
        d.ptr[k] = nullptr; d.stride[k] = 0; d.bstride[k] = 0; d.div[k] = nullptr; d.divstride[k] = 0; d.divoff[k] = 0;
    }
    d.nval = nval;
    return d;
}

// ------------------------------------------------------------------------------------------
// typed entry points
// ------------------------------------------------------------------------------------------
// dispatch_dim (common.h) is the one dispatch on the runtime dimension.
template <typename T>
int gibbs_fwd(const T* x1, const T* x2, const T* l1, const T* l2, int64_t n1, int64_t n2, int D, const T* os,
              const T* diag_add, T* K, int64_t ldk, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!l1) return -3; if (!l2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (D < 1 || D > NSGP_MAX_DIM) return -7;
    if (!K && n1 * n2 > 0) return -10; if (ldk < n2) return -11;
    return dispatch_dim<1, 2, 3>(D, [&](auto d) {
        GibbsOp<T, decltype(d)::value> op{x1, x2, l1, l2, n1, n2, D, os};
        return launch_fwd<T>(op, 1, n1, n2, T(0), diag_add, K, ldk, 0, stream);
    });
}

// The backward launch of the Gibbs family (GibbsOp, GibbsRadialOp): one accumulator layout, so one output wiring.
template <typename T, typename Op>
int gibbs_launch_bwd(const Op& op, const T* G, int64_t ldg, T* g_l1, T* g_l2, T* g_x1, T* g_x2, T* g_os, void* ws,
                     size_t wsb, void* stream) {
    constexpr int DM = Op::DM;
    const int D = op.Drt;
    const int64_t n1 = op.n1, n2 = op.n2;
    OutDesc<T> rows = empty_desc<T>(Op::NR), cols = empty_desc<T>(Op::NC), globs = empty_desc<T>(Op::NG);
    for (int d = 0; d < D; ++d) {
        if (g_l1) { rows.ptr[d] = g_l1 + (int64_t)d * n1; rows.stride[d] = 1; }
        if (g_x1) { rows.ptr[DM + d] = g_x1 + d; rows.stride[DM + d] = D; }
        if (g_l2) { cols.ptr[d] = g_l2 + (int64_t)d * n2; cols.stride[d] = 1; }
        if (g_x2) { cols.ptr[DM + d] = g_x2 + d; cols.stride[DM + d] = D; }
    }
    globs.ptr[0] = g_os;
    return launch_bwd<T>(op, 1, n1, n2, G, ldg, 0, rows, cols, globs, ws, wsb, stream);
}

template <typename T>
int gibbs_bwd(const T* x1, const T* x2, const T* l1, const T* l2, int64_t n1, int64_t n2, int D, const T* os, const T* G,
              int64_t ldg, T* g_l1, T* g_l2, T* g_x1, T* g_x2, T* g_os, void* ws, size_t wsb, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!l1) return -3; if (!l2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (D < 1 || D > NSGP_MAX_DIM) return -7;
    if (!G && n1 * n2 > 0) return -9; if (ldg < n2) return -10;
    return dispatch_dim<1, 2, 3>(D, [&](auto dim) {
        GibbsOp<T, decltype(dim)::value> op{x1, x2, l1, l2, n1, n2, D, os};
        return gibbs_launch_bwd<T>(op, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb, stream);
    });
}

// Stationary ARD family (RBF, Matern): the inputs every entry point of the family takes, in signature order.
template <typename T> struct ArdIn {
    const T *x1, *x2, *ls, *os;
    int64_t batch, n1, n2;
    int D;
    int64_t sx1, sx2;
};

// The family's argument check: 0, or the negative 1-based index of the first bad argument in the entry point's OWN
// signature (C ABI).  The entry point's extra scalars (Matern: nu2) follow sx2 as arguments 11..10 + extra; `mat` is K
// or G, which without extras is argument `mat_arg`, and `ld` its leading dimension, the argument after it.
template <typename T>
int ard_check(const ArdIn<T>& a, int extra, bool extra_ok, const T* mat, int64_t ld, int mat_arg) {
    if (!a.x1) return -1; if (!a.x2) return -2; if (!a.ls) return -3; if (!a.os) return -4;
    if (a.batch < 0) return -5; if (a.n1 < 0) return -6; if (a.n2 < 0) return -7;
    if (a.D < 1 || a.D > NSGP_MAX_DIM) return -8;
    if (!extra_ok) return -11;
    if (!mat && a.batch * a.n1 * a.n2 > 0) return -(mat_arg + extra);
    if (ld < a.n2) return -(mat_arg + extra + 1);
    return 0;
}
constexpr int ARD_FWD_K = 12, ARD_BWD_G = 11;

template <typename T, typename Radial>
int ard_fwd(const ArdIn<T>& a, T diag_add, T* K, int64_t ldk, int64_t sK, void* stream) {
    return dispatch_dim<1, 2, 3>(a.D, [&](auto d) {
        ArdOp<T, decltype(d)::value, Radial> op{a.x1, a.x2, a.ls, a.os, a.n1, a.n2, a.sx1, a.sx2, a.D};
        return launch_fwd<T>(op, a.batch, a.n1, a.n2, diag_add, (const T*)nullptr, K, ldk, sK, stream);
    });
}

template <typename T, typename Radial>
int ard_bwd(const ArdIn<T>& a, const T* G, int64_t ldg, int64_t sG, T* g_x1, T* g_x2, T* g_ls, T* g_os, void* ws,
            size_t wsb, void* stream) {
    return dispatch_dim<1, 2, 3>(a.D, [&](auto dim) {
        using Op = ArdOp<T, decltype(dim)::value, Radial>;
        Op op{a.x1, a.x2, a.ls, a.os, a.n1, a.n2, a.sx1, a.sx2, a.D};
        constexpr int DM = Op::DM;
        const int D = a.D;
        OutDesc<T> rows = empty_desc<T>(Op::NR), cols = empty_desc<T>(Op::NC), globs = empty_desc<T>(Op::NG);
        for (int d = 0; d < D; ++d) {
            if (g_x1) { rows.ptr[d] = g_x1 + d; rows.stride[d] = D; rows.bstride[d] = a.n1 * D;
                        rows.div[d] = a.ls; rows.divstride[d] = D; rows.divoff[d] = d; }
            if (g_x2) { cols.ptr[d] = g_x2 + d; cols.stride[d] = D; cols.bstride[d] = a.n2 * D;
                        cols.div[d] = a.ls; cols.divstride[d] = D; cols.divoff[d] = d; }
            if (g_ls) { globs.ptr[d] = g_ls + d; globs.bstride[d] = D;
                        globs.div[d] = a.ls; globs.divstride[d] = D; globs.divoff[d] = d; }
        }
        if (g_os) { globs.ptr[DM] = g_os; globs.bstride[DM] = 1; }
        return launch_bwd<T>(op, a.batch, a.n1, a.n2, G, ldg, sG, rows, cols, globs, ws, wsb, stream);
    });
}

template <typename T>
int rbf_fwd(const T* x1, const T* x2, const T* ls, const T* os, int64_t batch, int64_t n1, int64_t n2, int D,
            int64_t sx1, int64_t sx2, T diag_add, T* K, int64_t ldk, int64_t sK, void* stream) {
    const ArdIn<T> a{x1, x2, ls, os, batch, n1, n2, D, sx1, sx2};
    if (const int bad = ard_check(a, 0, true, (const T*)K, ldk, ARD_FWD_K)) return bad;
    return ard_fwd<T, RbfRadial>(a, diag_add, K, ldk, sK, stream);
}

template <typename T>
int rbf_bwd(const T* x1, const T* x2, const T* ls, const T* os, int64_t batch, int64_t n1, int64_t n2, int D,
            int64_t sx1, int64_t sx2, const T* G, int64_t ldg, int64_t sG, T* g_x1, T* g_x2, T* g_ls, T* g_os,
            void* ws, size_t wsb, void* stream) {
    const ArdIn<T> a{x1, x2, ls, os, batch, n1, n2, D, sx1, sx2};
    if (const int bad = ard_check(a, 0, true, G, ldg, ARD_BWD_G)) return bad;
    return ard_bwd<T, RbfRadial>(a, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws, wsb, stream);
}

// nu2 = 2 nu (checked by the caller) -> f(MaternRadial<nu2>{})
static inline bool matern_nu2_ok(int nu2) { return nu2 == 1 || nu2 == 3 || nu2 == 5; }
template <typename F> int dispatch_nu2(int nu2, F&& f) {
    return nu2 == 1 ? f(MaternRadial<1>{}) : nu2 == 3 ? f(MaternRadial<3>{}) : f(MaternRadial<5>{});
}

template <typename T>
int matern_fwd(const T* x1, const T* x2, const T* ls, const T* os, int64_t batch, int64_t n1, int64_t n2, int D,
               int64_t sx1, int64_t sx2, int nu2, T diag_add, T* K, int64_t ldk, int64_t sK, void* stream) {
    const ArdIn<T> a{x1, x2, ls, os, batch, n1, n2, D, sx1, sx2};
    if (const int bad = ard_check(a, 1, matern_nu2_ok(nu2), (const T*)K, ldk, ARD_FWD_K)) return bad;
    return dispatch_nu2(nu2, [&](auto radial) {
        return ard_fwd<T, decltype(radial)>(a, diag_add, K, ldk, sK, stream);
    });
}

template <typename T>
int matern_bwd(const T* x1, const T* x2, const T* ls, const T* os, int64_t batch, int64_t n1, int64_t n2, int D,
               int64_t sx1, int64_t sx2, int nu2, const T* G, int64_t ldg, int64_t sG, T* g_x1, T* g_x2, T* g_ls,
               T* g_os, void* ws, size_t wsb, void* stream) {
    const ArdIn<T> a{x1, x2, ls, os, batch, n1, n2, D, sx1, sx2};
    if (const int bad = ard_check(a, 1, matern_nu2_ok(nu2), G, ldg, ARD_BWD_G)) return bad;
    return dispatch_nu2(nu2, [&](auto radial) {
        return ard_bwd<T, decltype(radial)>(a, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws, wsb, stream);
    });
}

// K1': the Gibbs signatures with nu2 after D (so every later argument's index is one up)
template <typename T>
int gibbs_matern_fwd(const T* x1, const T* x2, const T* l1, const T* l2, int64_t n1, int64_t n2, int D, int nu2,
                     const T* os, const T* diag_add, T* K, int64_t ldk, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!l1) return -3; if (!l2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (D < 1 || D > NSGP_MAX_DIM) return -7;
    if (!matern_nu2_ok(nu2)) return -8;
    if (!K && n1 * n2 > 0) return -11; if (ldk < n2) return -12;
    return dispatch_nu2(nu2, [&](auto radial) {
        return dispatch_dim<1, 2, 3>(D, [&](auto d) {
            GibbsRadialOp<T, decltype(d)::value, decltype(radial)> op{{x1, x2, l1, l2, n1, n2, D, os}};
            return launch_fwd<T>(op, 1, n1, n2, T(0), diag_add, K, ldk, 0, stream);
        });
    });
}

template <typename T>
int gibbs_matern_bwd(const T* x1, const T* x2, const T* l1, const T* l2, int64_t n1, int64_t n2, int D, int nu2,
                     const T* os, const T* G, int64_t ldg, T* g_l1, T* g_l2, T* g_x1, T* g_x2, T* g_os, void* ws,
                     size_t wsb, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!l1) return -3; if (!l2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (D < 1 || D > NSGP_MAX_DIM) return -7;
    if (!matern_nu2_ok(nu2)) return -8;
    if (!G && n1 * n2 > 0) return -10; if (ldg < n2) return -11;
    return dispatch_nu2(nu2, [&](auto radial) {
        return dispatch_dim<1, 2, 3>(D, [&](auto dim) {
            GibbsRadialOp<T, decltype(dim)::value, decltype(radial)> op{{x1, x2, l1, l2, n1, n2, D, os}};
            return gibbs_launch_bwd<T>(op, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb, stream);
        });
    });
}

template <typename T>
int ps_fwd(const T* x1, const T* x2, const T* s1, const T* s2, int64_t n1, int64_t n2, T jit, T* K, int64_t ldk,
           void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!s1) return -3; if (!s2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (!K && n1 * n2 > 0) return -8; if (ldk < n2) return -9;
    PsOp<T> op{x1, x2, s1, s2, jit};
    return launch_fwd<T>(op, 1, n1, n2, T(0), (const T*)nullptr, K, ldk, 0, stream);
}

// The backward launch of the Paciorek-Schervish family (PsOp, PsRadialOp): one accumulator layout, so one output wiring.
template <typename T, typename Op>
int ps_launch_bwd(const Op& op, int64_t n1, int64_t n2, const T* G, int64_t ldg, T* g_s1, T* g_s2, void* ws, size_t wsb,
                  void* stream) {
    OutDesc<T> rows = empty_desc<T>(4), cols = empty_desc<T>(4), globs = empty_desc<T>(0);
    for (int k = 0; k < 4; ++k) {
        if (g_s1) { rows.ptr[k] = g_s1 + k; rows.stride[k] = 4; }
        if (g_s2) { cols.ptr[k] = g_s2 + k; cols.stride[k] = 4; }
    }
    return launch_bwd<T>(op, 1, n1, n2, G, ldg, 0, rows, cols, globs, ws, wsb, stream);
}

template <typename T>
int ps_bwd(const T* x1, const T* x2, const T* s1, const T* s2, int64_t n1, int64_t n2, T jit, const T* G,
           int64_t ldg, T* g_s1, T* g_s2, void* ws, size_t wsb, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!s1) return -3; if (!s2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (!G && n1 * n2 > 0) return -8; if (ldg < n2) return -9;
    PsOp<T> op{x1, x2, s1, s2, jit};
    return ps_launch_bwd<T>(op, n1, n2, G, ldg, g_s1, g_s2, ws, wsb, stream);
}

// K3': the Paciorek-Schervish signatures with nu2 after n2 (so every later argument's index is one up)
template <typename T>
int ps_matern_fwd(const T* x1, const T* x2, const T* s1, const T* s2, int64_t n1, int64_t n2, int nu2, T jit, T* K,
                  int64_t ldk, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!s1) return -3; if (!s2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (!matern_nu2_ok(nu2)) return -7;
    if (!K && n1 * n2 > 0) return -9; if (ldk < n2) return -10;
    return dispatch_nu2(nu2, [&](auto radial) {
        PsRadialOp<T, decltype(radial)> op{{x1, x2, s1, s2, jit}};
        return launch_fwd<T>(op, 1, n1, n2, T(0), (const T*)nullptr, K, ldk, 0, stream);
    });
}

template <typename T>
int ps_matern_bwd(const T* x1, const T* x2, const T* s1, const T* s2, int64_t n1, int64_t n2, int nu2, T jit,
                  const T* G, int64_t ldg, T* g_s1, T* g_s2, void* ws, size_t wsb, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!s1) return -3; if (!s2) return -4;
    if (n1 < 0) return -5; if (n2 < 0) return -6; if (!matern_nu2_ok(nu2)) return -7;
    if (!G && n1 * n2 > 0) return -9; if (ldg < n2) return -10;
    return dispatch_nu2(nu2, [&](auto radial) {
        PsRadialOp<T, decltype(radial)> op{{x1, x2, s1, s2, jit}};
        return ps_launch_bwd<T>(op, n1, n2, G, ldg, g_s1, g_s2, ws, wsb, stream);
    });
}

template <typename T>
int rbfper_fwd(const T* x1, const T* x2, const T* lsr, const T* lsp, const T* per, const T* os, int64_t batch,
               int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, T diag_add, T* K, int64_t ldk, int64_t sK,
               void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!lsp) return -4; if (!per) return -5;
    if (batch < 0) return -7; if (n1 < 0) return -8; if (n2 < 0) return -9; if (D < 1 || D > NSGP_MAX_DIM) return -10;
    if (!K && batch * n1 * n2 > 0) return -14; if (ldk < n2) return -15;
    return dispatch_dim<1, 2>(D, [&](auto d) {
        RbfPeriodicOp<T, decltype(d)::value> op{x1, x2, lsr, lsp, per, os, n1, n2, sx1, sx2, D};
        return launch_fwd<T>(op, batch, n1, n2, diag_add, (const T*)nullptr, K, ldk, sK, stream);
    });
}
// The backward launch of the periodic family (RbfPeriodicOp, RadialPeriodicOp): one accumulator layout, so one output wiring.
template <typename T, typename Op>
int rbfper_launch_bwd(const Op& op, int64_t batch, const T* G, int64_t ldg, int64_t sG, T* g_x1, T* g_x2, T* g_lsr,
                      T* g_lsp, T* g_per, T* g_os, void* ws, size_t wsb, void* stream) {
    constexpr int DM = Op::DM;
    const int D = op.Drt;
    const int64_t n1 = op.n1, n2 = op.n2;
    OutDesc<T> rows = empty_desc<T>(Op::NR), cols = empty_desc<T>(Op::NC), globs = empty_desc<T>(Op::NG);
    for (int d = 0; d < D; ++d) {
        if (g_x1) { rows.ptr[d] = g_x1 + d; rows.stride[d] = D; rows.bstride[d] = n1 * D; }
        if (g_x2) { cols.ptr[d] = g_x2 + d; cols.stride[d] = D; cols.bstride[d] = n2 * D; }
        if (g_lsr && op.lsr) { globs.ptr[d] = g_lsr + d; globs.bstride[d] = D; }
    }
    if (g_lsp) { globs.ptr[DM] = g_lsp; globs.bstride[DM] = 1; }
    if (g_per) { globs.ptr[DM + 1] = g_per; globs.bstride[DM + 1] = 1; }
    if (g_os) { globs.ptr[DM + 2] = g_os; globs.bstride[DM + 2] = 1; }
    return launch_bwd<T>(op, batch, n1, n2, G, ldg, sG, rows, cols, globs, ws, wsb, stream);
}

template <typename T>
int rbfper_bwd(const T* x1, const T* x2, const T* lsr, const T* lsp, const T* per, const T* os, int64_t batch,
               int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, const T* G, int64_t ldg, int64_t sG, T* g_x1,
               T* g_x2, T* g_lsr, T* g_lsp, T* g_per, T* g_os, void* ws, size_t wsb, void* stream) {
    if (!x1) return -1; if (!x2) return -2; if (!lsp) return -4; if (!per) return -5;
    if (batch < 0) return -7; if (n1 < 0) return -8; if (n2 < 0) return -9; if (D < 1 || D > NSGP_MAX_DIM) return -10;
    if (!G && batch * n1 * n2 > 0) return -13; if (ldg < n2) return -14;
    return dispatch_dim<1, 2>(D, [&](auto dim) {
        RbfPeriodicOp<T, decltype(dim)::value> op{x1, x2, lsr, lsp, per, os, n1, n2, sx1, sx2, D};
        return rbfper_launch_bwd<T>(op, batch, G, ldg, sG, g_x1, g_x2, g_lsr, g_lsp, g_per, g_os, ws, wsb, stream);
    });
}

// K2''': the rbf_periodic signatures with the envelope lengthscale required and nu2 after sx2 (so every later argument's
// index is one up)
template <typename T>
int matper_check(const T* x1, const T* x2, const T* lse, const T* lsp, const T* per, int64_t batch, int64_t n1,
                 int64_t n2, int D, int nu2) {
    if (!x1) return -1; if (!x2) return -2; if (!lse) return -3; if (!lsp) return -4; if (!per) return -5;
    if (batch < 0) return -7; if (n1 < 0) return -8; if (n2 < 0) return -9; if (D < 1 || D > NSGP_MAX_DIM) return -10;
    if (!matern_nu2_ok(nu2)) return -13;
    return 0;
}
template <typename T>
int matper_fwd(const T* x1, const T* x2, const T* lse, const T* lsp, const T* per, const T* os, int64_t batch,
               int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, T diag_add, T* K, int64_t ldk,
               int64_t sK, void* stream) {
    if (const int bad = matper_check(x1, x2, lse, lsp, per, batch, n1, n2, D, nu2)) return bad;
    if (!K && batch * n1 * n2 > 0) return -15; if (ldk < n2) return -16;
    return dispatch_nu2(nu2, [&](auto radial) {
        return dispatch_dim<1, 2>(D, [&](auto d) {
            RadialPeriodicOp<T, decltype(d)::value, decltype(radial)> op{{x1, x2, lse, lsp, per, os, n1, n2, sx1, sx2, D}};
            return launch_fwd<T>(op, batch, n1, n2, diag_add, (const T*)nullptr, K, ldk, sK, stream);
        });
    });
}
template <typename T>
int matper_bwd(const T* x1, const T* x2, const T* lse, const T* lsp, const T* per, const T* os, int64_t batch,
               int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, const T* G, int64_t ldg, int64_t sG,
               T* g_x1, T* g_x2, T* g_lse, T* g_lsp, T* g_per, T* g_os, void* ws, size_t wsb, void* stream) {
    if (const int bad = matper_check(x1, x2, lse, lsp, per, batch, n1, n2, D, nu2)) return bad;
    if (!G && batch * n1 * n2 > 0) return -14; if (ldg < n2) return -15;
    return dispatch_nu2(nu2, [&](auto radial) {
        return dispatch_dim<1, 2>(D, [&](auto dim) {
            RadialPeriodicOp<T, decltype(dim)::value, decltype(radial)> op{{x1, x2, lse, lsp, per, os, n1, n2, sx1, sx2, D}};
            return rbfper_launch_bwd<T>(op, batch, G, ldg, sG, g_x1, g_x2, g_lse, g_lsp, g_per, g_os, ws, wsb, stream);
        });
    });
}

}  // namespace

extern "C" {

int nsgp_pairwise_bwd_plan(int64_t batch, int64_t n1, int64_t n2, int* rows_per_wg, int64_t* nti, int64_t* ntj) {
    if (batch < 0) return -1; if (n1 < 0) return -2; if (n2 < 0) return -3;
    if (!rows_per_wg) return -4; if (!nti) return -5; if (!ntj) return -6;
    *rows_per_wg = 0; *nti = 0; *ntj = 0;
    if (batch == 0 || n1 == 0 || n2 == 0) return 0;          // nothing is launched
    const BwdPlan p = bwd_plan(batch, n1, n2);
    *rows_per_wg = p.rows; *nti = p.nti; *ntj = p.ntj;
    return 0;
}

int nsgp_gibbs_build_fwd_f32(const float* x1, const float* x2, const float* l1, const float* l2, int64_t n1,
                             int64_t n2, int D, const float* os, const float* diag_add, float* K, int64_t ldk,
                             void* stream) {
    return gibbs_fwd<float>(x1, x2, l1, l2, n1, n2, D, os, diag_add, K, ldk, stream);
}
int nsgp_gibbs_build_fwd_f64(const double* x1, const double* x2, const double* l1, const double* l2, int64_t n1,
                             int64_t n2, int D, const double* os, const double* diag_add, double* K, int64_t ldk,
                             void* stream) {
    return gibbs_fwd<double>(x1, x2, l1, l2, n1, n2, D, os, diag_add, K, ldk, stream);
}
size_t nsgp_gibbs_build_bwd_workspace(int64_t n1, int64_t n2, int D, int elem_size) {
    (void)D;                                    // sized for the generic (NSGP_MAX_DIM) functor
    return bwd_ws_elems<GibbsOp<double, 0>>(1, n1, n2) * (size_t)elem_size + 256;
}
int nsgp_gibbs_build_bwd_f32(const float* x1, const float* x2, const float* l1, const float* l2, int64_t n1,
                             int64_t n2, int D, const float* os, const float* G, int64_t ldg, float* g_l1, float* g_l2,
                             float* g_x1, float* g_x2, float* g_os, void* ws, size_t wsb, void* stream) {
    return gibbs_bwd<float>(x1, x2, l1, l2, n1, n2, D, os, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb, stream);
}
int nsgp_gibbs_build_bwd_f64(const double* x1, const double* x2, const double* l1, const double* l2, int64_t n1,
                             int64_t n2, int D, const double* os, const double* G, int64_t ldg, double* g_l1,
                             double* g_l2, double* g_x1, double* g_x2, double* g_os, void* ws, size_t wsb,
                             void* stream) {
    return gibbs_bwd<double>(x1, x2, l1, l2, n1, n2, D, os, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb, stream);
}

int nsgp_gibbs_matern_build_fwd_f32(const float* x1, const float* x2, const float* l1, const float* l2, int64_t n1,
                                    int64_t n2, int D, int nu2, const float* os, const float* diag_add, float* K,
                                    int64_t ldk, void* stream) {
    return gibbs_matern_fwd<float>(x1, x2, l1, l2, n1, n2, D, nu2, os, diag_add, K, ldk, stream);
}
int nsgp_gibbs_matern_build_fwd_f64(const double* x1, const double* x2, const double* l1, const double* l2, int64_t n1,
                                    int64_t n2, int D, int nu2, const double* os, const double* diag_add, double* K,
                                    int64_t ldk, void* stream) {
    return gibbs_matern_fwd<double>(x1, x2, l1, l2, n1, n2, D, nu2, os, diag_add, K, ldk, stream);
}
int nsgp_gibbs_matern_build_bwd_f32(const float* x1, const float* x2, const float* l1, const float* l2, int64_t n1,
                                    int64_t n2, int D, int nu2, const float* os, const float* G, int64_t ldg,
                                    float* g_l1, float* g_l2, float* g_x1, float* g_x2, float* g_os, void* ws,
                                    size_t wsb, void* stream) {
    return gibbs_matern_bwd<float>(x1, x2, l1, l2, n1, n2, D, nu2, os, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb,
                                   stream);
}
int nsgp_gibbs_matern_build_bwd_f64(const double* x1, const double* x2, const double* l1, const double* l2, int64_t n1,
                                    int64_t n2, int D, int nu2, const double* os, const double* G, int64_t ldg,
                                    double* g_l1, double* g_l2, double* g_x1, double* g_x2, double* g_os, void* ws,
                                    size_t wsb, void* stream) {
    return gibbs_matern_bwd<double>(x1, x2, l1, l2, n1, n2, D, nu2, os, G, ldg, g_l1, g_l2, g_x1, g_x2, g_os, ws, wsb,
                                    stream);
}

int nsgp_rbf_build_fwd_f32(const float* x1, const float* x2, const float* ls, const float* os, int64_t batch,
                           int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, float diag_add, float* K,
                           int64_t ldk, int64_t sK, void* stream) {
    return rbf_fwd<float>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, diag_add, K, ldk, sK, stream);
}
int nsgp_rbf_build_fwd_f64(const double* x1, const double* x2, const double* ls, const double* os, int64_t batch,
                           int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, double diag_add, double* K,
                           int64_t ldk, int64_t sK, void* stream) {
    return rbf_fwd<double>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, diag_add, K, ldk, sK, stream);
}
size_t nsgp_rbf_build_bwd_workspace(int64_t batch, int64_t n1, int64_t n2, int D, int elem_size) {
    (void)D;
    return bwd_ws_elems<ArdOp<double, 0, RbfRadial>>(batch, n1, n2) * (size_t)elem_size + 256;
}
int nsgp_rbf_build_bwd_f32(const float* x1, const float* x2, const float* ls, const float* os, int64_t batch,
                           int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, const float* G, int64_t ldg,
                           int64_t sG, float* g_x1, float* g_x2, float* g_ls, float* g_os, void* ws, size_t wsb,
                           void* stream) {
    return rbf_bwd<float>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws, wsb, stream);
}
int nsgp_rbf_build_bwd_f64(const double* x1, const double* x2, const double* ls, const double* os, int64_t batch,
                           int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, const double* G, int64_t ldg,
                           int64_t sG, double* g_x1, double* g_x2, double* g_ls, double* g_os, void* ws,
                           size_t wsb, void* stream) {
    return rbf_bwd<double>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws, wsb, stream);
}

int nsgp_matern_build_fwd_f32(const float* x1, const float* x2, const float* ls, const float* os, int64_t batch,
                              int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, float diag_add, float* K,
                              int64_t ldk, int64_t sK, void* stream) {
    return matern_fwd<float>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, nu2, diag_add, K, ldk, sK, stream);
}
int nsgp_matern_build_fwd_f64(const double* x1, const double* x2, const double* ls, const double* os, int64_t batch,
                              int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, double diag_add,
                              double* K, int64_t ldk, int64_t sK, void* stream) {
    return matern_fwd<double>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, nu2, diag_add, K, ldk, sK, stream);
}
size_t nsgp_matern_build_bwd_workspace(int64_t batch, int64_t n1, int64_t n2, int D, int elem_size) {
    (void)D;                                    // sized for the generic (NSGP_MAX_DIM) functor, any radial function
    return bwd_ws_elems<ArdOp<double, 0, RbfRadial>>(batch, n1, n2) * (size_t)elem_size + 256;
}
int nsgp_matern_build_bwd_f32(const float* x1, const float* x2, const float* ls, const float* os, int64_t batch,
                              int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, const float* G,
                              int64_t ldg, int64_t sG, float* g_x1, float* g_x2, float* g_ls, float* g_os, void* ws,
                              size_t wsb, void* stream) {
    return matern_bwd<float>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, nu2, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws, wsb,
                             stream);
}
int nsgp_matern_build_bwd_f64(const double* x1, const double* x2, const double* ls, const double* os, int64_t batch,
                              int64_t n1, int64_t n2, int D, int64_t sx1, int64_t sx2, int nu2, const double* G,
                              int64_t ldg, int64_t sG, double* g_x1, double* g_x2, double* g_ls, double* g_os, void* ws,
                              size_t wsb, void* stream) {
    return matern_bwd<double>(x1, x2, ls, os, batch, n1, n2, D, sx1, sx2, nu2, G, ldg, sG, g_x1, g_x2, g_ls, g_os, ws,
                              wsb, stream);
}

int nsgp_ps2d_build_fwd_f32(const float* x1, const float* x2, const float* s1, const float* s2, int64_t n1,
                            int64_t n2, float jit, float* K, int64_t ldk, void* stream) {
    return ps_fwd<float>(x1, x2, s1, s2, n1, n2, jit, K, ldk, stream);
}
int nsgp_ps2d_build_fwd_f64(const double* x1, const double* x2, const double* s1, const double* s2, int64_t n1,
                            int64_t n2, double jit, double* K, int64_t ldk, void* stream) {
    return ps_fwd<double>(x1, x2, s1, s2, n1, n2, jit, K, ldk, stream);
}
size_t nsgp_ps2d_build_bwd_workspace(int64_t n1, int64_t n2, int elem_size) {
    return bwd_ws_elems<PsOp<double>>(1, n1, n2) * (size_t)elem_size + 256;
}
int nsgp_ps2d_build_bwd_f32(const float* x1, const float* x2, const float* s1, const float* s2, int64_t n1,
                            int64_t n2, float jit, const float* G, int64_t ldg, float* g_s1, float* g_s2, void* ws,
                            size_t wsb, void* stream) {
    return ps_bwd<float>(x1, x2, s1, s2, n1, n2, jit, G, ldg, g_s1, g_s2, ws, wsb, stream);
}
int nsgp_ps2d_build_bwd_f64(const double* x1, const double* x2, const double* s1, const double* s2, int64_t n1,
                            int64_t n2, double jit, const double* G, int64_t ldg, double* g_s1, double* g_s2,
                            void* ws, size_t wsb, void* stream) {
    return ps_bwd<double>(x1, x2, s1, s2, n1, n2, jit, G, ldg, g_s1, g_s2, ws, wsb, stream);
}

int nsgp_ps2d_matern_build_fwd_f32(const float* x1, const float* x2, const float* s1, const float* s2, int64_t n1,
                                   int64_t n2, int nu2, float jit, float* K, int64_t ldk, void* stream) {
    return ps_matern_fwd<float>(x1, x2, s1, s2, n1, n2, nu2, jit, K, ldk, stream);
}
int nsgp_ps2d_matern_build_fwd_f64(const double* x1, const double* x2, const double* s1, const double* s2, int64_t n1,
                                   int64_t n2, int nu2, double jit, double* K, int64_t ldk, void* stream) {
    return ps_matern_fwd<double>(x1, x2, s1, s2, n1, n2, nu2, jit, K, ldk, stream);
}
int nsgp_ps2d_matern_build_bwd_f32(const float* x1, const float* x2, const float* s1, const float* s2, int64_t n1,
                                   int64_t n2, int nu2, float jit, const float* G, int64_t ldg, float* g_s1,
                                   float* g_s2, void* ws, size_t wsb, void* stream) {
    return ps_matern_bwd<float>(x1, x2, s1, s2, n1, n2, nu2, jit, G, ldg, g_s1, g_s2, ws, wsb, stream);
}
int nsgp_ps2d_matern_build_bwd_f64(const double* x1, const double* x2, const double* s1, const double* s2, int64_t n1,
                                   int64_t n2, int nu2, double jit, const double* G, int64_t ldg, double* g_s1,
                                   double* g_s2, void* ws, size_t wsb, void* stream) {
    return ps_matern_bwd<double>(x1, x2, s1, s2, n1, n2, nu2, jit, G, ldg, g_s1, g_s2, ws, wsb, stream);
}

int nsgp_rbf_periodic_build_fwd_f32(const float* x1, const float* x2, const float* ls_rbf, const float* ls_per,
                                    const float* period, const float* os, int64_t batch, int64_t n1, int64_t n2, int D,
                                    int64_t sx1, int64_t sx2, float diag_add, float* K, int64_t ldk, int64_t sK,
                                    void* stream) {
    return rbfper_fwd<float>(x1, x2, ls_rbf, ls_per, period, os, batch, n1, n2, D, sx1, sx2, diag_add, K, ldk, sK, stream);
}
int nsgp_rbf_periodic_build_fwd_f64(const double* x1, const double* x2, const double* ls_rbf, const double* ls_per,
                                    const double* period, const double* os, int64_t batch, int64_t n1, int64_t n2,
                                    int D, int64_t sx1, int64_t sx2, double diag_add, double* K, int64_t ldk,
                                    int64_t sK, void* stream) {
    return rbfper_fwd<double>(x1, x2, ls_rbf, ls_per, period, os, batch, n1, n2, D, sx1, sx2, diag_add, K, ldk, sK, stream);
}
size_t nsgp_rbf_periodic_build_bwd_workspace(int64_t batch, int64_t n1, int64_t n2, int D, int elem_size) {
    (void)D;
    return bwd_ws_elems<RbfPeriodicOp<double, 0>>(batch, n1, n2) * (size_t)elem_size + 256;
}
int nsgp_rbf_periodic_build_bwd_f32(const float* x1, const float* x2, const float* ls_rbf, const float* ls_per,
                                    const float* period, const float* os, int64_t batch, int64_t n1, int64_t n2, int D,
                                    int64_t sx1, int64_t sx2, const float* G, int64_t ldg, int64_t sG, float* g_x1,
                                    float* g_x2, float* g_ls_rbf, float* g_ls_per, float* g_period, float* g_os,
                                    void* ws, size_t wsb, void* stream) {
    return rbfper_bwd<float>(x1, x2, ls_rbf, ls_per, period, os, batch, n1, n2, D, sx1, sx2, G, ldg, sG, g_x1, g_x2,
                             g_ls_rbf, g_ls_per, g_period, g_os, ws, wsb, stream);
}
int nsgp_rbf_periodic_build_bwd_f64(const double* x1, const double* x2, const double* ls_rbf, const double* ls_per,
                                    const double* period, const double* os, int64_t batch, int64_t n1, int64_t n2,
                                    int D, int64_t sx1, int64_t sx2, const double* G, int64_t ldg, int64_t sG,
                                    double* g_x1, double* g_x2, double* g_ls_rbf, double* g_ls_per, double* g_period,
                                    double* g_os, void* ws, size_t wsb, void* stream) {
    return rbfper_bwd<double>(x1, x2, ls_rbf, ls_per, period, os, batch, n1, n2, D, sx1, sx2, G, ldg, sG, g_x1, g_x2,
                              g_ls_rbf, g_ls_per, g_period, g_os, ws, wsb, stream);
}

int nsgp_matern_periodic_build_fwd_f32(const float* x1, const float* x2, const float* ls_env, const float* ls_per,
                                       const float* period, const float* os, int64_t batch, int64_t n1, int64_t n2,
                                       int D, int64_t sx1, int64_t sx2, int nu2, float diag_add, float* K, int64_t ldk,
                                       int64_t sK, void* stream) {
    return matper_fwd<float>(x1, x2, ls_env, ls_per, period, os, batch, n1, n2, D, sx1, sx2, nu2, diag_add, K, ldk, sK,
                             stream);
}
int nsgp_matern_periodic_build_fwd_f64(const double* x1, const double* x2, const double* ls_env, const double* ls_per,
                                       const double* period, const double* os, int64_t batch, int64_t n1, int64_t n2,
                                       int D, int64_t sx1, int64_t sx2, int nu2, double diag_add, double* K,
                                       int64_t ldk, int64_t sK, void* stream) {
    return matper_fwd<double>(x1, x2, ls_env, ls_per, period, os, batch, n1, n2, D, sx1, sx2, nu2, diag_add, K, ldk, sK,
                              stream);
}
int nsgp_matern_periodic_build_bwd_f32(const float* x1, const float* x2, const float* ls_env, const float* ls_per,
                                       const float* period, const float* os, int64_t batch, int64_t n1, int64_t n2,
                                       int D, int64_t sx1, int64_t sx2, int nu2, const float* G, int64_t ldg,
                                       int64_t sG, float* g_x1, float* g_x2, float* g_ls_env, float* g_ls_per,
                                       float* g_period, float* g_os, void* ws, size_t wsb, void* stream) {
    return matper_bwd<float>(x1, x2, ls_env, ls_per, period, os, batch, n1, n2, D, sx1, sx2, nu2, G, ldg, sG, g_x1, g_x2,
                             g_ls_env, g_ls_per, g_period, g_os, ws, wsb, stream);
}
int nsgp_matern_periodic_build_bwd_f64(const double* x1, const double* x2, const double* ls_env, const double* ls_per,
                                       const double* period, const double* os, int64_t batch, int64_t n1, int64_t n2,
                                       int D, int64_t sx1, int64_t sx2, int nu2, const double* G, int64_t ldg,
                                       int64_t sG, double* g_x1, double* g_x2, double* g_ls_env, double* g_ls_per,
                                       double* g_period, double* g_os, void* ws, size_t wsb, void* stream) {
    return matper_bwd<double>(x1, x2, ls_env, ls_per, period, os, batch, n1, n2, D, sx1, sx2, nu2, G, ldg, sG, g_x1,
                              g_x2, g_ls_env, g_ls_per, g_period, g_os, ws, wsb, stream);
}

}  // extern "C"
