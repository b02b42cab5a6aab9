// gemm_i8.hip -- the whitened projection A = W Kzx of a float32 SVGP layer on the int8 matrix cores, to better than
// float32 accuracy (an error-free-transformation product in the manner of Ozaki's scheme).
//
// Why: A = L^-1 Kzx (gpytorch VariationalStrategy.forward behind /root/reference/models/dgps.py:44-51; SURVEY A.3: a float64
// triangular solve, cast back) cannot be accumulated in float32 -- at kappa(Kzz) ~ 1e6 the terms |W||Kzx| ~ 1e2 cancel to
// O(1) and float32 accumulation costs 2e-4 of the posterior mean -- so round 2 ran it on the float64 MFMA
// (v_mfma_f64_16x16x4_f64, 78.6 TFLOP/s peak, 47 achieved: the single largest kernel of a DSVI step).  gfx950's int8 MFMA
// (v_mfma_i32_32x32x32_i8) is 64x the float64 rate per multiply-add, and integer accumulation is EXACT.  So:
//
//   W[m][k]  = wsc[m] * sum_{a<5}  dW_a[m][k] 128^-a    dW_a in [-64, 64]  (wsc[m] = 2^e / 64 >= max_k |W[m][k]| / 64)
//   K[k][j]  = ksc    * sum_{b<SK} dK_b[k][j] 128^-b    dK_b in [-64, 64]  (ksc    = 2^e / 64 >= |os| / 64: |K| <= |os|)
//   A[m][j]  = wsc[m] ksc sum_{l<LEV} 128^-l  sum_{a+b=l} sum_k dW_a[m][k] dK_b[k][j]
//
// in two instantiations: SK = 4 planes of Kzx, LEV = 5 levels (14 digit-plane products) for a layer whose output feeds the
// likelihood, and SK = 5, LEV = 6 (19 products) for a layer whose output is the next layer's input (nsgp/svgp.py chooses).
// Each inner sum is an int32 (|.| <= 5 x 1024 x 64^2 < 2^25 for M <= 1024, < 2^27 at the M = 4096 limit nsgp_i8_supported
// admits), the level sums are combined by Horner's rule in float64 and rounded ONCE to float32.  What is dropped: W below
// 2^-35 of its row maximum, K below 2^-28 (2^-35 with five planes) of os -- K is evaluated in float64 from the float32
// inputs, the digits carry 4 (11) more bits than a float32 Kzx, so this also replaces settings.hidden_kzx_f64's float64 Kzx
// -- and the digit pairs with a + b >= LEV.
// Measured against the float64 product at the headline shape (kappa 8.5e5): 9.5e-7 of max|A| with 14 products, < 8e-7 (the
// float32 rounding of A itself) with 19 -- float64 accumulation of the float32 Kzx: 5.6e-6; float32 accumulation: 6.6e-5
// (tests/test_gpu_i8.py; the numpy emulation the plane counts were chosen with: tools/probes/ozaki_emulation.py).
//
// Layout.  Digit planes are stored the way the kernel stages them, so a K-step's operand block is one contiguous run:
//   Wd[b][a][kb][h][Mp][16]   int8, kb = k / 32, h = (k % 32) / 16, Mp = M rounded up to 128 (zero rows), zeros for k > m
//   Kd[b][s][kb][h][np][16]   int8, np = n rounded up to 64 (zero columns)
// One 256-thread workgroup = a 128 x 64 output tile, 4 waves of 64 x 32 (two 32 x 32 MFMA tiles), LEV int32 level
// accumulators per MFMA tile (the five-plane form sits at 255 VGPRs, no spills).  LDS holds two stages of
// (5 x 128 + SK x 64) x 32 bytes (28 / 30 KB), images [plane][h][row][16] so that an operand fragment is one
// conflict-free ds_read_b128 per lane; the stages are filled by LDS-DMA (global_load_lds_dwordx4: a K-step's block is one
// contiguous run in memory, so no registers are spent on staging; NSGP_I8_DMA=0 builds the register-staged form); the K
// planes of a K-step stay in registers while the W planes stream through; behind the stages, 1.5 KB for the row scales and
// the row vector of the tile's 128 rows, which the prologue fetches beside the first stage so that the epilogue reads no
// global memory, and 2 KB for the column-statistics reduction; two workgroups per CU (2 x 59.5 / 63.5 KB of the 160 KB LDS,
// 227 / 252 VGPRs, no scratch).  With four planes a workgroup walks two column tiles (i8_walk).
#include <cstdlib>
#include "common.h"
#include "radial.h"

namespace {

#ifndef NSGP_I8_DMA
#define NSGP_I8_DMA 1
#endif
constexpr int I8_BM = 128, I8_BN = 64, I8_BK = 32;
// column tiles a workgroup of i8_proj_kernel walks: two with four Kzx planes; one with five, whose six level accumulators
// leave no registers for a loop around the tile (it spills: 6 VGPRs at two tiles)
constexpr int i8_walk(int sk) { return sk == 4 ? 2 : 1; }
constexpr int I8_SW = 5;                                    // digit planes of W (K: 4 or 5, template SK; levels a + b < LEV)

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// ---- digit planes of W (one workgroup per row) ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void i8_slice_w_kernel(const double* __restrict__ W, int64_t M, int64_t Mp, int64_t KB,
                                                         signed char* __restrict__ Wd, double* __restrict__ wsc) {
    __shared__ double lds[4];
    const int64_t b = blockIdx.y, m = blockIdx.x;
    signed char* out = Wd + b * (int64_t)I8_SW * KB * 2 * Mp * 16;
    const int64_t plane = KB * 2 * Mp * 16;
    if (m >= M) {                                           // padding rows: zeros
        for (int64_t k = threadIdx.x; k < KB * 32; k += 256)
            for (int a = 0; a < I8_SW; ++a) out[a * plane + ((k >> 5) * 2 + ((k >> 4) & 1)) * Mp * 16 + m * 16 + (k & 15)] = 0;
        return;
    }
    const double* row = W + (b * M + m) * M;
    // NaN-propagating maximum (a plain v > mx skips NaN): a row with a NaN or an infinity -- W of a Kzz that is not positive
    // definite -- gets the scale NaN and zero digits, so the product's epilogue (v *= wsc ksc) makes that row of A NaN
    const auto nmax = [](double a, double c) { return (a > c || a != a) ? a : c; };
    double mx = 0.0;
    for (int64_t k = threadIdx.x; k <= m; k += 256) mx = nmax(fabs(row[k]), mx);
    // block max through LDS
    for (int off = 32; off > 0; off >>= 1) mx = nmax(__shfl_xor(mx, off, 64), mx);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = nmax(nmax(lds[0], lds[1]), nmax(lds[2], lds[3]));
    const bool fin = mx <= 1.7976931348623157e308;          // false for NaN and +inf
    int e = 0;
    (void)frexp(fin ? mx : 0.0, &e);                        // mx = f 2^e, f in [0.5, 1)  ->  2^e >= mx
    const double rs = (fin && mx > 0.0) ? ldexp(1.0, e) : 1.0;
    if (threadIdx.x == 0) wsc[b * M + m] = fin ? rs / 64.0 : __builtin_nan("");
    const double inv = 64.0 / rs;
    for (int64_t k = threadIdx.x; k < KB * 32; k += 256) {
        double t = (fin && k <= m && k < M) ? row[k] * inv : 0.0;
        const int64_t o = ((k >> 5) * 2 + ((k >> 4) & 1)) * Mp * 16 + m * 16 + (k & 15);
#pragma unroll
        for (int a = 0; a < I8_SW; ++a) {
            const double d = rint(t);
            out[a * plane + o] = (signed char)(int)d;
            t = (t - d) * 128.0;
        }
    }
}

// ---- digit planes of Kzx, evaluated in float64 from the float32 kernel inputs ------------------------------------
// One thread = one column j and one k-block of 32: K[k][j] = os kappa(s), s = sum_d ((z[k][d] - x[j][d]) / ls[d])^2, with
// the radial function kappa a policy: I8Rbf, exp(-s / 2) spelled as this kernel always spelled it (its digits are pinned
// bit for bit), or I8Matern<NU2>, which IS MaternRadial<NU2>::eval<double> of radial.h -- the function ops.matern_build
// evaluates in float64: 0 distance below the normal range of s, 0 beyond exponent -745.13, NaN stays NaN.  kappa <= 1
// up to one ulp (poly e may round above 1): |sc| <= 64 (1 - 2^-53) since 2^e > |os| strictly, so |t| < 64.5 and every
// digit stays in [-64, 64].
struct I8Rbf {
    static __device__ __forceinline__ double eval(double r2) { return t_fexp<double>(-0.5 * r2); }
};
template <int NU2> struct I8Matern {
    static __device__ __forceinline__ double eval(double s) { return MaternRadial<NU2>::template eval<double>(s); }
};
// Digit scale: every workgroup (256 columns x one k-block) writes its own slot ksc[b][kb][blockIdx.x] -- os's power of two / 64,
// or NaN when os or an ls is not finite or one of its entries came out NaN (a NaN z or x).  One writer per slot, so a NaN
// cannot be overwritten by another workgroup's finite value; the product folds the slots of the k-blocks a tile reads.
template <typename Radial, int D, int SK>
__global__ __launch_bounds__(256) void i8_kzx_build_kernel(const float* __restrict__ Z, const float* __restrict__ x, int64_t sx,
                                                           const float* __restrict__ ls, const float* __restrict__ os,
                                                           int64_t M, int64_t n, int64_t np, int64_t KB,
                                                           signed char* __restrict__ Kd, double* __restrict__ ksc,
                                                           float* __restrict__ Kf) {
    const int64_t b = blockIdx.z, kb = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    __shared__ double zs[32][D];
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    if (threadIdx.x < 32 * D) {
        const int kk = threadIdx.x / D, d = threadIdx.x % D;
        const int64_t k = kb * 32 + kk;
        zs[kk][d] = k < M ? (double)Z[(b * M + k) * D + d] / (double)ls[b * D + d] : 0.0;
    }
    __syncthreads();
    const double osd = (double)os[b];
    bool fin = fabs(osd) <= 1.7976931348623157e308;
#pragma unroll
    for (int d = 0; d < D; ++d) fin = fin && fabs((double)ls[b * D + d]) <= 1.7976931348623157e308;
    int e = 0;
    (void)frexp(fin ? osd : 0.0, &e);
    const double cs = ldexp(1.0, e);                        // >= |os|
    const double sc = fin ? osd * 64.0 / cs : 0.0;
    if (j < np) {
        double xs[D];
#pragma unroll
        for (int d = 0; d < D; ++d) xs[d] = j < n ? (double)x[b * sx + j * D + d] / (double)ls[b * D + d] : 0.0;
        signed char* out = Kd + b * (int64_t)SK * KB * 2 * np * 16;
        const int64_t plane = KB * 2 * np * 16;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int pk[SK][4] = {};
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int kk = h * 16 + q;
                double r2 = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) { const double df = zs[kk][d] - xs[d]; r2 = __builtin_fma(df, df, r2); }
                const bool in = j < n && kb * 32 + kk < M;
                const bool nan_e = in && r2 != r2;
                if (nan_e) bad = 1;
                const double ev = in ? Radial::eval(r2) : 0.0;
                const double evd = nan_e ? 0.0 : ev;          // (no NaN into the digit cutter's float -> int conversions)
                // the float32 Kzx the backward pass needs for Wbar = tril(Abar Kzx^T), rounded from the float64 value (the
                // forward pass itself never reads it): saves the backward's own build launch
                if (Kf && in) Kf[(b * M + kb * 32 + kk) * n + j] = (float)(osd * ev);
                // (the product stays free to fuse into the first plane's t - dg, as it always has: digits bit-identical)
                double t = sc * evd;
#pragma unroll
                for (int s = 0; s < SK; ++s) {
                    const double dg = rint(t);
                    pk[s][q >> 2] |= ((int)dg & 0xFF) << (8 * (q & 3));
                    t = (t - dg) * 128.0;
                }
            }
#pragma unroll
            for (int s = 0; s < SK; ++s) {
                v4i v = {pk[s][0], pk[s][1], pk[s][2], pk[s][3]};
                *reinterpret_cast<v4i*>(out + s * plane + (kb * 2 + h) * np * 16 + j * 16) = v;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0)
        ksc[(b * KB + kb) * gridDim.x + blockIdx.x] = (fin && !bad) ? cs / 64.0 : __builtin_nan("");
}

// ---- the product --------------------------------------------------------------------------------------------------
// P64: float64 column-statistic partials (layers whose variance also accumulates in float64, see nsgp.h)
template <int P64, int SK, int LEV>
__global__ __launch_bounds__(256, 2) void i8_proj_kernel(const signed char* __restrict__ Wd, const double* __restrict__ wsc,
                                                         const signed char* __restrict__ Kd, const double* __restrict__ ksc,
                                                         const float* __restrict__ rv, int64_t M, int64_t n, int64_t Mp,
                                                         int64_t np, int64_t KB, int tiles_n, float* __restrict__ Y,
                                                         void* __restrict__ p0, void* __restrict__ p1, int part_rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char i8_smem[];
    constexpr int A_STAGE = I8_SW * 2 * I8_BM * 16, B_STAGE = SK * 2 * I8_BN * 16;       // 20480 + 8192 bytes
    unsigned char* As = i8_smem;                            // [2][A_STAGE]
    unsigned char* Bs = i8_smem + 2 * A_STAGE;              // [2][B_STAGE]
    double* Ws = reinterpret_cast<double*>(i8_smem + 2 * (A_STAGE + B_STAGE));           // [128] wsc of the tile's rows
    float* Rs = reinterpret_cast<float*>(Ws + I8_BM);                                     // [128] rv of the tile's rows
    double* red = reinterpret_cast<double*>(Rs + I8_BM);    // [2 quantities][2 wave rows][64 columns] of the epilogue
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 32;
    const int64_t bb = blockIdx.y;
    const int tiles_m = (int)(Mp / I8_BM);
    // Anatomy of the two launches of a headline step (0.447 -> 0.374 ms once the epilogue stopped loading from global memory:
    // 356 -> 292 us for <0,4,5> at n = 40960, 91 -> 82 us for <1,5,6> at b = 2, n = 4096).  Switches that skipped the MFMAs /
    // the staging / both, measured on the loop before that change (0.441 ms): staging alone 0.345, MFMAs + fragment reads
    // alone 0.363, neither -- first-stage latency, barriers, the float64 Horner epilogue and the stores of 5120 + 1024 short
    // workgroups -- 0.187 ms, of which the epilogue's 64 serialised loads per workgroup (the row scale and the row vector
    // under the per-element bounds test: one branch, one load, one vmcnt(0) each) were the 0.07 ms now gone.  The K loop is
    // as it was: one K-block of prefetch, vmcnt(0) and a barrier per K-block, 28 KB into LDS per 112 MFMAs (2.6 GB per
    // launch, 7.4 TB/s).  Not built: a ring of three stages with counted waits (W alone fits three stages twice per CU, 2 x
    // 61.5 KB, if the Kzx fragments go straight to registers -- whose ordinary loads the compiler waits for with vmcnt(0)
    // while an LDS-DMA is in flight, so they would have to be issued and counted by hand).
    // Two column tiles per workgroup (below): 289.4 -> 279.4 us for <0,4,5>; four tiles: 293.2 (too few workgroups for the
    // tail); <.,5,6> spills under a tile loop and keeps one tile (profiles/splitk_reduce_i8_walk/).
    // (Tried and dropped: an XCD-grouped order -- workgroup 8 q + x, which the hardware places on XCD x, walking all row tiles of
    // column tiles x, x + 8, ... back to back so that a column tile's Kzx planes enter that L2 once: 0.441 -> 0.534 ms per
    // headline step, like the same experiment on the float32 GEMM.)
    // A workgroup walks up to TW consecutive column tiles of one tile row: same W blocks, same K range, and the first
    // stage and digit-scale slots of tile t + 1 are issued before the epilogue of tile t, so that only the first tile of a
    // walk pays the cold latency of its prologue in the open (the row scales and the row vector are the walk's).
    constexpr int TW = i8_walk(SK);
    const int walks_n = (tiles_n + TW - 1) / TW;
    const int bm = tiles_m - 1 - (int)blockIdx.x / walks_n;          // long K ranges first
    const int bn0 = ((int)blockIdx.x % walks_n) * TW;
    const int ntile = TW == 1 ? 1 : __builtin_amdgcn_readfirstlane(tiles_n - bn0 < TW ? tiles_n - bn0 : TW);
    const int64_t m0 = (int64_t)bm * I8_BM, n00 = (int64_t)bn0 * I8_BN;
    int nkb = (int)((m0 + I8_BM) / I8_BK);                  // lower triangular W: k < m0 + 128
    if (nkb > KB) nkb = (int)KB;
    const signed char* Wb = Wd + bb * (int64_t)I8_SW * KB * 2 * Mp * 16;
    const signed char* Kb = Kd + bb * (int64_t)SK * KB * 2 * np * 16;
    const int64_t wplane = KB * 2 * Mp * 16, kplane = KB * 2 * np * 16;

    // staging: piece q of A = (plane a, half h, row) = q / 256, (q % 256) / 128, q % 128; LDS offset 16 q.  5 per thread.
    // piece q of B = (plane s, half h, col) = q / 128, (q % 128) / 64, q % 64: SK x 128 pieces, NPB per thread (the last
    // one of 5 planes only for the first 128 threads).
    // The addresses are those of column tile t of the walk, worked out again from the thread index wherever a tile needs
    // them -- through a value the compiler cannot see through: pointers kept from one tile to the next would stay in
    // registers across the epilogue, which has none to spare.
    constexpr int NPB = (SK * 128 + 255) / 256;
    const signed char* ga[5];
    const signed char* gb[NPB];
    auto pieces = [&](int t) __attribute__((always_inline)) {
        int tv = tid;
        asm volatile("" : "+v"(tv));
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const int q = tv + 256 * j;
            const int a = q >> 8, h = (q >> 7) & 1, row = q & 127;
            ga[j] = Wb + a * wplane + (int64_t)h * Mp * 16 + (m0 + row) * 16;
        }
#pragma unroll
        for (int j = 0; j < NPB; ++j) {
            int q = tv + 256 * j;
            if (q >= SK * 128) q = SK * 128 - 1;                       // (clamped: loaded twice, stored once)
            const int s = q >> 7, h = (q >> 6) & 1, col = q & 63;
            gb[j] = Kb + s * kplane + (int64_t)h * np * 16 + (n00 + t * I8_BN + col) * 16;
        }
    };
    const int64_t astep = 2 * Mp * 16, bstep = 2 * np * 16;          // bytes per k-block
#if NSGP_I8_DMA
    // Staging by LDS-DMA (global_load_lds_dwordx4): the digit planes are stored in the order the LDS image wants them, so a
    // wave's 64 consecutive pieces are 1 KB of global memory -> 1 KB of LDS, no staging registers (the 5 level accumulators
    // and the operand fragments need all 256), no ds_write.  The LDS base of a wave's run is wave-uniform (M0).
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;
    auto dma = [&](int kb, int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(ga[j] + (int64_t)kb * astep),
                                             (lptr_t)(As + buf * A_STAGE + (wave * 64 + 256 * j) * 16), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            if (wave * 64 + 256 * j < SK * 128)
                __builtin_amdgcn_global_load_lds((gptr_t)(gb[j] + (int64_t)kb * bstep),
                                                 (lptr_t)(Bs + buf * B_STAGE + (wave * 64 + 256 * j) * 16), 16, 0, 0);
    };
#endif
    v4i ra[5], rb[NPB];
    auto gload = [&](int kb) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 5; ++j) ra[j] = *reinterpret_cast<const v4i*>(ga[j] + (int64_t)kb * astep);
#pragma unroll
        for (int j = 0; j < NPB; ++j) rb[j] = *reinterpret_cast<const v4i*>(gb[j] + (int64_t)kb * bstep);
    };
    auto sstore = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 5; ++j) *reinterpret_cast<v4i*>(As + buf * A_STAGE + (tid + 256 * j) * 16) = ra[j];
#pragma unroll
        for (int j = 0; j < NPB; ++j)
            if (tid + 256 * j < SK * 128) *reinterpret_cast<v4i*>(Bs + buf * B_STAGE + (tid + 256 * j) * 16) = rb[j];
    };

    // this wave's rows reach k < m0 + wm0 + 64: the upper wave row has nothing to do in the tile's last two k-blocks
    const int wave_nkb = __builtin_amdgcn_readfirstlane((int)((m0 + wm0 + 64 + I8_BK - 1) / I8_BK));
    const int half = lane >> 5, lr = lane & 31;
    // The epilogue's operands are fetched here, beside the first stage's cold load, not after the loop: the row scales and
    // the row vector of the tile's 128 rows go to LDS (zeros for rows >= M and for a null rv), the digit scale of Kzx is
    // folded by the barrier that publishes the first stage -- the build's slot of k-block 0 for these columns, NaN if the
    // slot of any k-block this tile reads is NaN.
    const int64_t gx = (np + 255) >> 8;
    const double* ksb = ksc + bb * KB * gx;
    const float* rvb = rv ? rv + bb * M : nullptr;
    // the first stage and the digit-scale slots of column tile t of the walk (clamped index, not a branch)
    auto stage0 = [&](int t) __attribute__((always_inline)) {
        pieces(t);
#if NSGP_I8_DMA
        dma(0, 0);
#else
        gload(0);
        sstore(0);
#endif
        return ksb[((n00 + t * I8_BN) >> 8) + (int64_t)(tid < nkb ? tid : nkb - 1) * gx];
    };
    double kslot = stage0(0);
    // (clamped indices, not branches: the three loads leave together and are waited for once, with the stage)
    const int64_t prow = m0 + (tid & (I8_BM - 1)), crow = prow < M ? prow : M - 1;
    const double wload = wsc[bb * M + crow];
    const float rload = rvb ? rvb[crow] : 0.0f;
    const double wrow = prow < M ? wload : 0.0;
    const float rrow = prow < M ? rload : 0.0f;
    if (tid < I8_BM) { Ws[tid] = wrow; Rs[tid] = rrow; }
#pragma unroll 1
    for (int t = 0; t < ntile; ++t) {
    const int bn = bn0 + t;
    const int64_t n0 = (int64_t)bn * I8_BN;
    const double* ks = ksb + (n0 >> 8);
    v16i acc[LEV][2];
#pragma unroll
    for (int l = 0; l < LEV; ++l)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[l][i][r] = 0;
#if NSGP_I8_DMA
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the tile's first stage: issued above, or before the last epilogue
#endif
    const double kscale = __syncthreads_or(kslot != kslot) ? __builtin_nan("") : ks[0];
    if (t > 0) pieces(t);                                  // (the first tile's are the prologue's)
    for (int kb = 0; kb < nkb; ++kb) {
        const int buf = kb & 1;
#if NSGP_I8_DMA
        if (kb + 1 < nkb) dma(kb + 1, buf ^ 1);           // (every wave left buffer buf ^ 1 behind the last barrier)
#else
        if (kb + 1 < nkb) gload(kb + 1);
#endif
        if (kb < wave_nkb) {
            // K's planes stay in registers for the whole k-block; W's planes pass through one at a time, the next one's
            // fragments read while the current one's MFMAs run
            v4i af[2][2], bf[SK];
#pragma unroll
            for (int s = 0; s < SK; ++s)
                bf[s] = *reinterpret_cast<const v4i*>(Bs + buf * B_STAGE + ((s * 2 + half) * I8_BN + wn0 + lr) * 16);
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[0][i] = *reinterpret_cast<const v4i*>(As + buf * A_STAGE + ((0 * 2 + half) * I8_BM + wm0 + 32 * i + lr) * 16);
#pragma unroll
            for (int a = 0; a < I8_SW; ++a) {
                if (a + 1 < I8_SW) {
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        af[(a + 1) & 1][i] = *reinterpret_cast<const v4i*>(
                            As + buf * A_STAGE + (((a + 1) * 2 + half) * I8_BM + wm0 + 32 * i + lr) * 16);
                }
#pragma unroll
                for (int s = 0; s < SK; ++s)
                    if (a + s < LEV) {
#pragma unroll
                        for (int i = 0; i < 2; ++i)
                            acc[a + s][i] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[a & 1][i], bf[s], acc[a + s][i], 0, 0, 0);
                    }
            }
        }
#if NSGP_I8_DMA
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's pieces of the next stage have landed ...
#else
        if (kb + 1 < nkb) sstore(buf ^ 1);
#endif
        __syncthreads();                                   // ... and so have everybody else's
    }

    // The next tile's first stage goes to buffer 0 now -- every wave is behind the loop's last barrier, and the epilogue's
    // scratch has LDS of its own -- and lands under the epilogue.
    if (t + 1 < ntile) kslot = stage0(t + 1);
    // epilogue: levels -> float64 -> one rounding to float32; column statistics from the float64 values.  No global load is
    // left in it: a load under the per-element `in` made the compiler branch around it and wait for it alone, 64 dependent
    // round trips per workgroup.
    double sdot = 0.0, ssq = 0.0;
    // (the tile row as a value the compiler cannot see through: it would otherwise compute the 32 row offsets of the stores
    // once per walk and keep them in registers across the K loop, which the accumulators need)
    int64_t m0e = m0;
    asm volatile("" : "+s"(m0e));
    int lanee = lane, tide = tid;
    asm volatile("" : "+v"(lanee), "+v"(tide));
    const int halfe = lanee >> 5, lre = lanee & 31;
    const int64_t col = n0 + wn0 + lre;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int lrow = wm0 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * halfe;
            const int64_t row = m0e + lrow;
            const double wr = Ws[lrow];
            const float rr = Rs[lrow];
            double v = (double)acc[LEV - 1][i][r];
#pragma unroll
            for (int l = LEV - 2; l >= 0; --l) v = __builtin_fma(v, 0.0078125, (double)acc[l][i][r]);
            const bool in = row < M && col < n;
            v *= (in ? wr : 0.0) * kscale;
            if (in) Y[(bb * M + row) * n + col] = (float)v;
            sdot += v * ((rvb && in) ? (double)rr : 0.0);
            ssq += v * v;
        }
    sdot += __shfl_xor(sdot, 32, 64);
    ssq += __shfl_xor(ssq, 32, 64);
    __syncthreads();                                        // (the last tile's sums have been read)
    if (lanee < 32) {
        red[(0 + (wave >> 1)) * I8_BN + wn0 + lanee] = sdot;
        red[(2 + (wave >> 1)) * I8_BN + wn0 + lanee] = ssq;
    }
    __syncthreads();
    if (tide < I8_BN && n0 + tide < n) {
        const int64_t o = (bb * part_rows + bm) * n + n0 + tide;
        const double d = red[tide] + red[I8_BN + tide], q = red[2 * I8_BN + tide] + red[3 * I8_BN + tide];
        if (P64) {
            if (p0) reinterpret_cast<double*>(p0)[o] = d;
            reinterpret_cast<double*>(p1)[o] = q;
        } else {
            if (p0) reinterpret_cast<float*>(p0)[o] = (float)d;
            reinterpret_cast<float*>(p1)[o] = (float)q;
        }
    }
    }   // column tiles of the walk
}

static inline int64_t i8_mp(int64_t M) { return cdiv64(M, I8_BM) * I8_BM; }
static inline int64_t i8_np(int64_t n) { return cdiv64(n, I8_BN) * I8_BN; }
static inline int64_t i8_kb(int64_t M) { return cdiv64(M, I8_BK); }

// the plane build of one radial function, arguments checked by the caller: D in 1..4, planes in {4, 5}, no empty size
template <typename Radial>
int i8_kzx_build_launch(const float* Z, const float* x, int64_t sx, const float* ls, const float* os, int64_t batch, int64_t M,
                        int64_t n, int D, int planes, void* Kd, double* kscale, float* Kzx_f32, void* stream) {
    const int64_t np = i8_np(n), KB = i8_kb(M);
    dim3 grid((unsigned)cdiv64(np, 256), (unsigned)KB, (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    signed char* kd = (signed char*)Kd;
#define NSGP_I8_BUILD(DD, SS) hipLaunchKernelGGL((i8_kzx_build_kernel<Radial, DD, SS>), grid, dim3(256), 0, st, Z, x, sx, ls, os, M, n, np, KB, kd, kscale, Kzx_f32)
    if (planes == 4) {
        switch (D) { case 1: NSGP_I8_BUILD(1, 4); break; case 2: NSGP_I8_BUILD(2, 4); break; case 3: NSGP_I8_BUILD(3, 4); break;
                     default: NSGP_I8_BUILD(4, 4); break; }
    } else {
        switch (D) { case 1: NSGP_I8_BUILD(1, 5); break; case 2: NSGP_I8_BUILD(2, 5); break; case 3: NSGP_I8_BUILD(3, 5); break;
                     default: NSGP_I8_BUILD(4, 5); break; }
    }
#undef NSGP_I8_BUILD
    return nsgp_launch_status();
}

}  // namespace

extern "C" {

int nsgp_i8_supported(int64_t M) { return (M >= 1 && M <= 4096) ? 1 : 0; }       // int32 level sums: 5 M 64^2 < 2^31
size_t nsgp_i8_w_planes_bytes(int64_t batch, int64_t M) {
    return (batch > 0 && M > 0) ? (size_t)(batch * I8_SW * i8_kb(M) * 2 * i8_mp(M) * 16) : 0;
}
size_t nsgp_i8_k_planes_bytes(int64_t batch, int64_t M, int64_t n, int planes) {
    return (batch > 0 && M > 0 && n > 0 && (planes == 4 || planes == 5)) ? (size_t)(batch * planes * i8_kb(M) * 2 * i8_np(n) * 16) : 0;
}
size_t nsgp_i8_tiles(int64_t M) { return M > 0 ? (size_t)cdiv64(M, I8_BM) : 0; }
size_t nsgp_i8_kscale_count(int64_t batch, int64_t M, int64_t n) {                // one slot per build workgroup
    return (batch > 0 && M > 0 && n > 0) ? (size_t)(batch * i8_kb(M) * cdiv64(i8_np(n), 256)) : 0;
}

int nsgp_i8_slice_w_f64(const double* W, int64_t batch, int64_t M, void* Wd, double* wscale, void* stream) {
    if (!W) return -1; if (batch < 0) return -2; if (M < 0 || !nsgp_i8_supported(M > 0 ? M : 1)) return -3;
    if (!Wd) return -4; if (!wscale) return -5;
    if (batch == 0 || M == 0) return 0;
    if (batch > 65535) return -2;
    hipLaunchKernelGGL(i8_slice_w_kernel, dim3((unsigned)i8_mp(M), (unsigned)batch), dim3(256), 0, (hipStream_t)stream, W, M,
                       i8_mp(M), i8_kb(M), (signed char*)Wd, wscale);
    return nsgp_launch_status();
}

int nsgp_i8_rbf_build_f32(const float* Z, const float* x, int64_t x_batch_stride, const float* ls, const float* os,
                          int64_t batch, int64_t M, int64_t n, int D, int planes, void* Kd, double* kscale, float* Kzx_f32,
                          void* stream) {
    if (planes != 4 && planes != 5) return -10;
    if (!Z) return -1; if (!x) return -2; if (x_batch_stride < 0) return -3; if (!ls) return -4; if (!os) return -5;
    if (batch < 0) return -6; if (M < 0 || !nsgp_i8_supported(M > 0 ? M : 1)) return -7; if (n < 0) return -8;
    if (D < 1 || D > 4) return -9; if (!Kd) return -10; if (!kscale) return -11;
    if (batch == 0 || M == 0 || n == 0) return 0;
    if (batch > 65535 || i8_kb(M) > 65535) return -6;
    return i8_kzx_build_launch<I8Rbf>(Z, x, x_batch_stride, ls, os, batch, M, n, D, planes, Kd, kscale, Kzx_f32, stream);
}

int nsgp_i8_matern_build_f32(const float* Z, const float* x, int64_t x_batch_stride, const float* ls, const float* os,
                             int64_t batch, int64_t M, int64_t n, int D, int nu2, int planes, void* Kd, double* kscale,
                             float* Kzx_f32, void* stream) {
    if (!Z) return -1; if (!x) return -2; if (x_batch_stride < 0) return -3; if (!ls) return -4; if (!os) return -5;
    if (batch < 0) return -6; if (M < 0 || !nsgp_i8_supported(M > 0 ? M : 1)) return -7; if (n < 0) return -8;
    if (D < 1 || D > 4) return -9; if (nu2 != 1 && nu2 != 3 && nu2 != 5) return -10;
    if (planes != 4 && planes != 5) return -11; if (!Kd) return -12; if (!kscale) return -13;
    if (batch == 0 || M == 0 || n == 0) return 0;
    if (batch > 65535 || i8_kb(M) > 65535) return -6;
    switch (nu2) {
        case 1: return i8_kzx_build_launch<I8Matern<1>>(Z, x, x_batch_stride, ls, os, batch, M, n, D, planes, Kd, kscale, Kzx_f32, stream);
        case 3: return i8_kzx_build_launch<I8Matern<3>>(Z, x, x_batch_stride, ls, os, batch, M, n, D, planes, Kd, kscale, Kzx_f32, stream);
        default: return i8_kzx_build_launch<I8Matern<5>>(Z, x, x_batch_stride, ls, os, batch, M, n, D, planes, Kd, kscale, Kzx_f32, stream);
    }
}

int nsgp_svgp_tri_gemm_colstats_i8(const void* Wd, const double* wscale, const void* Kd, const double* kscale,
                                   int planes, const float* rowvec, int64_t batch, int64_t M, int64_t n, float* Y,
                                   void* part_dot, void* part_sq, int64_t part_rows, int partials_f64, void* stream) {
    if (planes != 4 && planes != 5) return -5;
    if (!Wd) return -1; if (!wscale) return -2; if (!Kd) return -3; if (!kscale) return -4;
    if (batch < 0) return -6; if (M < 0 || !nsgp_i8_supported(M > 0 ? M : 1)) return -7; if (n < 0) return -8;
    if (!Y) return -9; if (!part_sq) return -11; if (part_rows < cdiv64(M > 0 ? M : 1, I8_BM)) return -12;
    if (batch == 0 || M == 0 || n == 0) return 0;
    const int64_t Mp = i8_mp(M), np = i8_np(n), KB = i8_kb(M);
    const int64_t tiles_n = np / I8_BN, tiles = (Mp / I8_BM) * cdiv64(tiles_n, i8_walk(planes));   // one workgroup per walk
    if (tiles > 2147483647LL || batch > 65535) return -8;
    const size_t lds = 2 * (size_t)(I8_SW * 2 * I8_BM * 16 + planes * 2 * I8_BN * 16) + I8_BM * (sizeof(double) + sizeof(float)) +
                       4 * I8_BN * sizeof(double);
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)tiles, (unsigned)batch);
#define NSGP_I8_PROJ(PP, SS) hipLaunchKernelGGL((i8_proj_kernel<PP, SS, (SS == 5 ? 6 : 5)>), grid, dim3(256), lds, st, (const signed char*)Wd, wscale, \
        (const signed char*)Kd, kscale, rowvec, M, n, Mp, np, KB, (int)tiles_n, Y, part_dot, part_sq, (int)part_rows)
    if (planes == 4) { if (partials_f64) NSGP_I8_PROJ(1, 4); else NSGP_I8_PROJ(0, 4); }
    else { if (partials_f64) NSGP_I8_PROJ(1, 5); else NSGP_I8_PROJ(0, 5); }
#undef NSGP_I8_PROJ
    return nsgp_launch_status();
}

}  // extern "C"
