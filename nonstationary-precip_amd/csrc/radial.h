// radial.h -- the radial functions kappa(s), s = |u|^2, of the stationary ARD kernels: ONE statement of each, shared by the
// tile kernels of pairwise.hip (ArdOp, GibbsRadialOp) and by the int8 projection's Kzx plane builder of gemm_i8.hip, so that
// the float64 Kzx the digit planes are cut from and ops.rbf_build / ops.matern_build in float64 are one function.
// (Moved here from pairwise.hip unchanged: every kernel of that file disassembles to the same instructions as before,
// profiles/matern_dsvi/isa_diff_pairwise.json.)
#pragma once
#include "common.h"

namespace {

// K2 / K2'' batched stationary ARD kernels  k = os[b] * kappa(s),  s = |u|^2,  u = (x1 - x2) / ls[b]:  ONE functor, the
// radial function kappa is the `Radial` policy (a template parameter only: no member, so the kernel-argument layout is
// the same for every radial function).  A policy is stateless and has one function
//     template <typename T> static T eval(T s, T* q = nullptr)
// that returns kappa(s) and, when q != nullptr (the backward), also writes q = phi or q = -phi, where
// phi = (d kappa / d d) / d <= 0 with d = sqrt(s), so that d kappa / d u_d = phi u_d.  `negated` says which: RBF writes
// -phi (which IS kappa: nothing is computed twice), Matern writes phi.  ArdOp::grad accumulates with the matching signs.
// Both spellings are the same mathematics, but not the same code: under -ffp-contract=fast the compiler picks which
// multiply-add pairs to fuse from the spelling (with Matern in the -phi spelling the float32 nu = 1/2 backward stopped
// fusing ga += g kappa and its g_os / g_x moved in the last bits), and RBF in the phi spelling costs the timed step up to
// 14 instructions per kernel.  So each policy keeps the sign under which its results were established.
struct RbfRadial {                        // kappa = exp(-s / 2), -phi = kappa
    static constexpr bool negated = true;
    template <typename T> static __device__ __forceinline__ T eval(T s, T* q = nullptr) {
        const T k = t_fexp(T(-0.5) * s);
        if (q) *q = k;
        return k;
    }
};

// Matern, nu = NU2 / 2 in {1/2, 3/2, 5/2} (a template parameter: uniform per launch, so each entry runs straight-line
// code with its constants folded; three instantiations per D and type).  d = sqrt(s), a = sqrt(2 nu):
//   nu = 1/2:  kappa = e^-d                          phi = -e^-d / d, 0 at d = 0
//   nu = 3/2:  kappa = (1 + a d) e^-ad               phi = -3 e^-ad
//   nu = 5/2:  kappa = (1 + a d + 5/3 s) e^-ad       phi = -5/3 (1 + a d) e^-ad
// d = 0 for nu = 1/2 is the symmetric subgradient (the limit of the other two): K(x, x)'s diagonal adds no gradient.
// A NaN coordinate stays NaN (the d == 0 test is false for NaN); far entries are 0 * finite, never inf * 0.
template <typename T> __device__ __forceinline__ T matern_dist(T s);
// v_sqrt_f32, 1 ulp
template <> __device__ __forceinline__ float matern_dist<float>(float s) { return t_fsqrt(s); }
// s * rsqrt(s) (t_rsqrt: 1 ulp in about 7 instructions, against ~17 for the library sqrt); s = 0 and s below the normal
// range give 0 (d < 1.5e-154 lengthscales), NaN stays NaN
template <> __device__ __forceinline__ double matern_dist<double>(double s) {
    return s < 2.2250738585072014e-308 ? 0.0 : s * t_rsqrt(s);
}
// k = poly e with e = e^{-a d}, d >= 0 (poly = 1 for nu = 1/2); returns k, writes e.
// float: a log2(e) is one constant (one rounding less in front of v_exp_f32).  v_exp_f32 returns no denormals, but
// poly e stays normal while e is not (poly reaches ~1e4 before k leaves the normal range): below 2^-64, e is formed as
// 2^64 e^{-ad} and the product rescaled by 2^-64, exactly.
// double: t_fexp gives the smallest denormal, not 0, below -745; exp(x) rounds to 0 there, so the far tail is 0.
template <int NU2> struct MaternA;
template <> struct MaternA<1> { static constexpr double a = 1.0, a_log2e = 1.4426950408889634; };
template <> struct MaternA<3> { static constexpr double a = 1.7320508075688772, a_log2e = 2.4988211106473432; };
template <> struct MaternA<5> { static constexpr double a = 2.23606797749979, a_log2e = 3.225964182229561; };
template <int NU2> __device__ __forceinline__ float matern_poly_exp(float d, float poly, float& e) {
    const float x = d * -(float)MaternA<NU2>::a_log2e;
    const bool lo = x < -64.0f;
    const float e2 = __builtin_amdgcn_exp2f(lo ? x + 64.0f : x);
    e = lo ? e2 * 0x1p-64f : e2;
    return lo ? (poly * e2) * 0x1p-64f : poly * e2;
}
template <int NU2> __device__ __forceinline__ double matern_poly_exp(double d, double poly, double& e) {
    const double x = d * -MaternA<NU2>::a;
    e = x < -745.1332191019412 ? 0.0 : t_fexp(x);              // NaN: false, t_fexp(NaN) = NaN
    return poly * e;
}

template <int NU2> struct MaternRadial {
    static_assert(NU2 == 1 || NU2 == 3 || NU2 == 5, "nu = 1/2, 3/2, 5/2");
    static constexpr bool negated = false;
    template <typename T> static __device__ __forceinline__ T eval(T s, T* q = nullptr) {
        constexpr T A = T(MaternA<NU2>::a);
        const T d = matern_dist(s);
        T e;
        if constexpr (NU2 == 1) {
            const T k = matern_poly_exp<NU2>(d, T(1), e);
            if (q) *q = d == T(0) ? T(0) : -e / d;
            return k;
        } else if constexpr (NU2 == 3) {
            const T k = matern_poly_exp<NU2>(d, t_fma(A, d, T(1)), e);
            if (q) *q = T(-3) * e;
            return k;
        } else {
            const T p1 = t_fma(A, d, T(1));
            const T k = matern_poly_exp<NU2>(d, t_fma(T(5.0 / 3.0), s, p1), e);
            if (q) *q = T(-5.0 / 3.0) * p1 * e;
            return k;
        }
    }
};

}  // namespace
