// kmeans.hip -- Lloyd's k-means for the inducing points (include/nsgp.h, KM): the assign kernel and the three launches of
// the deterministic update.  gfx950 only; 256-thread workgroups (4 waves of 64).
//
// Conventions of pairwise.hip: dispatch_dim<1, 2, 3> picks the kernel with the dimension as a compile-time constant (inside a
// kernel D = DS ? DS : Drt, so guards and strides fold), or the generic one (DS = 0: NSGP_MAX_DIM register slots, runtime trip
// count, the unused slots hold zeros); distances are FMA
// chains on differences; no floating-point atomics anywhere; arguments are checked on the host before any HIP call.
//
// assign   Each lane keeps KM_P points' coordinates in registers (point = block base + p * 256 + thread).  The centres
//          stream through LDS in tiles of KM_TILE; inside a tile every lane reads the SAME centre (one broadcast LDS read,
//          conflict-free), so M is not bounded by the LDS and the VALU work -- D subtractions and FMAs, one compare, two
//          selects per pair -- stays in registers.
// update   Owner-computes, so nobody sorts and nobody adds to another thread's sum.  A chunk is `stages` blocks of KM_STAGE
//          points.  Workgroup (chunk, g) stages labels and coordinates in LDS block by block; thread t owns clusters
//          g * 256 KM_R + t + 256 j (j < KM_R) and walks the block in point order (all lanes read the same label: a
//          broadcast).  Its float64 sums (two-sum compensated: a high and a low part) and counts go to ws[chunk][row][k],
//          rows = D high parts, D low parts, the count, coalesced along k; group 0
//          also sums the chunk's d2.  km_finish_kernel sums a cluster's partials over chunks in chunk order (8 contiguous
//          runs of chunks, then the 8 in order), divides once and writes the centre and the cluster's shift; km_stats_kernel
//          adds the per-chunk inertias and per-cluster shifts in one workgroup.  About n M compares, as many as assign.
#include "common.h"

#define KM_THREADS 256
#define KM_P       2        // points per lane in assign
#define KM_TILE    256      // centres per LDS tile in assign
#define KM_STAGE   512      // points per LDS block in update
#define KM_R       4        // clusters per thread and pass in update
#define KM_PARTS   8        // runs of chunks per cluster in km_finish_kernel
#define KM_KPB     (KM_THREADS / KM_PARTS)   // clusters per workgroup there

template <typename T> __device__ __forceinline__ T km_inf();
template <> __device__ __forceinline__ float km_inf<float>() { return __builtin_huge_valf(); }
template <> __device__ __forceinline__ double km_inf<double>() { return __builtin_huge_val(); }

// (hi, lo) += v with the rounding error of hi + v kept in lo (Knuth's two-sum, exact for any magnitudes): the cluster sums
// carry about 106 bits, so the one rounding of hi + lo before the division is the only one a mean's numerator sees
__device__ __forceinline__ void km_add(double& hi, double& lo, double v) {
    const double s = hi + v, bp = s - hi;
    lo += (hi - (s - bp)) + (v - bp);
    hi = s;
}

template <typename T, int DS>
__global__ __launch_bounds__(KM_THREADS) void km_assign_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int Drt,
                                                               const T* __restrict__ c, int M,
                                                               int32_t* __restrict__ labels, T* __restrict__ d2) {
    constexpr int DM = DS ? DS : NSGP_MAX_DIM;
    const int D = DS ? DS : Drt;                        // a constant in the specialised instances: every `d < D` folds
    __shared__ T cs[KM_TILE * DM];                      // cs[k * D + d]
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * (KM_THREADS * KM_P) + tid;
    T xr[KM_P][DM], best[KM_P];
    int32_t lab[KM_P];
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
        const int64_t i = base + (int64_t)p * KM_THREADS;
#pragma unroll
        for (int d = 0; d < DM; ++d) xr[p][d] = (i < n && d < D) ? x[i * ldx + d] : T(0);
        best[p] = km_inf<T>();
        lab[p] = 0;
    }
    for (int m0 = 0; m0 < M; m0 += KM_TILE) {
        const int mt = min(KM_TILE, M - m0);
        __syncthreads();
        for (int idx = tid; idx < mt * D; idx += KM_THREADS) cs[idx] = c[(int64_t)m0 * D + idx];
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < mt; ++k) {
            T cd[DM];
#pragma unroll
            for (int d = 0; d < DM; ++d) cd[d] = d < D ? cs[k * D + d] : T(0);
#pragma unroll
            for (int p = 0; p < KM_P; ++p) {
                T s = T(0);
#pragma unroll
                for (int d = 0; d < DM; ++d)
                    if (d < D) {
                        const T df = xr[p][d] - cd[d];
                        s = t_fma(df, df, s);
                    }
                if (s < best[p]) {                      // strict: the lowest index wins a tie, a NaN never wins
                    best[p] = s;
                    lab[p] = m0 + k;
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
        const int64_t i = base + (int64_t)p * KM_THREADS;
        if (i < n) {
            labels[i] = lab[p];
            d2[i] = best[p];
        }
    }
}

template <typename T, int DS>
__global__ __launch_bounds__(KM_THREADS) void km_partial_kernel(const T* __restrict__ x, int64_t ldx, int64_t n, int Drt,
                                                                const int32_t* __restrict__ labels,
                                                                const T* __restrict__ d2, int M, int stages,
                                                                double* __restrict__ part, double* __restrict__ inert) {
    constexpr int DM = DS ? DS : NSGP_MAX_DIM;
    const int D = DS ? DS : Drt;
    __shared__ T xs[KM_STAGE * DM];                     // xs[i * DM + d], zero beyond D and beyond the last point
    __shared__ int32_t ls[KM_STAGE];                    // -1 beyond the last point
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int k0 = (int)blockIdx.y * (KM_THREADS * KM_R) + tid;
    double acc[KM_R][DM], low[KM_R][DM], ine = 0.0;
    int32_t cnt[KM_R];
#pragma unroll
    for (int j = 0; j < KM_R; ++j) {
        cnt[j] = 0;
#pragma unroll
        for (int d = 0; d < DM; ++d) acc[j][d] = low[j][d] = 0.0;
    }
    for (int st = 0; st < stages; ++st) {
        const int64_t p0 = (chunk * stages + st) * KM_STAGE;
        if (p0 >= n) break;                             // uniform over the workgroup
        const int npt = (int)min((int64_t)KM_STAGE, n - p0);
        __syncthreads();
        for (int i = tid; i < KM_STAGE; i += KM_THREADS) {
            const bool in = i < npt;
            ls[i] = in ? labels[p0 + i] : -1;
#pragma unroll
            for (int d = 0; d < DM; ++d) xs[i * DM + d] = (in && d < D) ? x[(p0 + i) * ldx + d] : T(0);
            if (in && blockIdx.y == 0) ine += (double)d2[p0 + i];
        }
        __syncthreads();
        for (int i = 0; i < npt; ++i) {
            const int r = ls[i] - k0;
#pragma unroll
            for (int j = 0; j < KM_R; ++j)
                if (r == j * KM_THREADS) {
                    ++cnt[j];
#pragma unroll
                    for (int d = 0; d < DM; ++d) km_add(acc[j][d], low[j][d], (double)xs[i * DM + d]);
                }
        }
    }
    double* out = part + chunk * (int64_t)(2 * D + 1) * M;    // rows: D high parts, D low parts, the count
#pragma unroll
    for (int j = 0; j < KM_R; ++j) {
        const int k = k0 + j * KM_THREADS;
        if (k < M) {
#pragma unroll
            for (int d = 0; d < DM; ++d)
                if (d < D) {
                    out[(int64_t)d * M + k] = acc[j][d];
                    out[(int64_t)(D + d) * M + k] = low[j][d];
                }
            out[(int64_t)2 * D * M + k] = (double)cnt[j];
        }
    }
    if (blockIdx.y == 0) {
        const double s = block_sum_256(ine, red);
        if (tid == 0) inert[chunk] = s;
    }
}

template <typename T, int DS>
__global__ __launch_bounds__(KM_THREADS) void km_finish_kernel(const double* __restrict__ part, int64_t nchunks, int Drt,
                                                               const T* __restrict__ c_old, int M, T* __restrict__ c_new,
                                                               int32_t* __restrict__ counts, double* __restrict__ shift) {
    constexpr int DM = DS ? DS : NSGP_MAX_DIM;
    const int D = DS ? DS : Drt;
    __shared__ double red[KM_PARTS][2 * DM + 1][KM_KPB];
    const int kl = threadIdx.x % KM_KPB, q = threadIdx.x / KM_KPB;
    const int k = (int)blockIdx.x * KM_KPB + kl;
    const int64_t per = (nchunks + KM_PARTS - 1) / KM_PARTS;
    const int64_t c0 = min(nchunks, q * per), c1 = min(nchunks, (q + 1) * per);
    double acc[DM], low[DM], num = 0.0;
#pragma unroll
    for (int d = 0; d < DM; ++d) acc[d] = low[d] = 0.0;
    if (k < M)
        for (int64_t ch = c0; ch < c1; ++ch) {
            const double* src = part + ch * (int64_t)(2 * D + 1) * M + k;
#pragma unroll
            for (int d = 0; d < DM; ++d)
                if (d < D) {
                    km_add(acc[d], low[d], src[(int64_t)d * M]);
                    low[d] += src[(int64_t)(D + d) * M];
                }
            num += src[(int64_t)2 * D * M];
        }
#pragma unroll
    for (int d = 0; d < DM; ++d) {
        red[q][d][kl] = acc[d];
        red[q][DM + d][kl] = low[d];
    }
    red[q][2 * DM][kl] = num;
    __syncthreads();
    if (q == 0 && k < M) {
#pragma clang fp contract(off)                          // the shift below: a rounded square, then a rounded sum, never an FMA
        double cnt = 0.0;
        for (int r = 0; r < KM_PARTS; ++r) cnt += red[r][2 * DM][kl];
        double sh = 0.0;
#pragma unroll
        for (int d = 0; d < DM; ++d)
            if (d < D) {
                const T old = c_old[(int64_t)k * D + d];
                T now = old;
                if (cnt > 0.0) {
                    double s = 0.0, e = 0.0;
                    for (int r = 0; r < KM_PARTS; ++r) {
                        km_add(s, e, red[r][d][kl]);
                        e += red[r][DM + d][kl];
                    }
                    now = (T)((s + e) / cnt);
                }
                c_new[(int64_t)k * D + d] = now;
                const double df = (double)now - (double)old;
                sh = sh + df * df;                      // not contracted (pragma above): the stated order of include/nsgp.h
            }
        counts[k] = (int32_t)cnt;
        shift[k] = sh;
    }
}

// one workgroup: stats[0] = sum of the per-chunk inertias, stats[1] = sum of the per-cluster shifts; thread t adds items
// t, t + 256, ... in order, then the fixed tree of block_sum_256
__global__ __launch_bounds__(KM_THREADS) void km_stats_kernel(const double* __restrict__ inert, int64_t nchunks,
                                                              const double* __restrict__ shift, int M,
                                                              double* __restrict__ stats) {
    __shared__ double red[4];
    double a = 0.0, b = 0.0;
    for (int64_t i = threadIdx.x; i < nchunks; i += KM_THREADS) a += inert[i];
    for (int k = threadIdx.x; k < M; k += KM_THREADS) b += shift[k];
    a = block_sum_256(a, red);
    b = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        stats[0] = a;
        stats[1] = b;
    }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
struct KmPlan { int stages; int64_t nchunks; };

static KmPlan km_plan(int64_t n) {
    const int64_t s = cdiv64(n, (int64_t)1 << 19);
    KmPlan p;
    p.stages = (int)(s < 1 ? 1 : s > 8 ? 8 : s);
    p.nchunks = cdiv64(n, (int64_t)p.stages * KM_STAGE);
    return p;
}

// the size bounds, stated once: counts are int32 (n <= 2^31 - 1), and the update's grid has ceil(M / 1024) <= 65535 rows
static bool km_n_ok(int64_t n) { return n >= 0 && n <= NSGP_KMEANS_MAX_N; }
static bool km_dim_ok(int D) { return D >= 1 && D <= NSGP_MAX_DIM; }
static bool km_m_ok(int M) { return M >= 1 && M <= NSGP_KMEANS_MAX_M; }

template <typename T>
int km_assign(const T* x, int64_t ldx, int64_t n, int D, const T* c, int M, int32_t* labels, T* d2, void* stream) {
    if (!x && n > 0) return -1;
    if (!km_dim_ok(D)) return -4;
    if (ldx < D) return -2;
    if (!km_n_ok(n)) return -3;
    if (!c) return -5; if (!km_m_ok(M)) return -6;
    if (!labels && n > 0) return -7; if (!d2 && n > 0) return -8;
    if (n == 0) return 0;
    const dim3 grid((unsigned)cdiv64(n, KM_THREADS * KM_P));
    return dispatch_dim<1, 2, 3>(D, [&](auto d) {
        hipLaunchKernelGGL((km_assign_kernel<T, decltype(d)::value>), grid, dim3(KM_THREADS), 0, (hipStream_t)stream, x, ldx,
                           n, D, c, M, labels, d2);
        return nsgp_launch_status();
    });
}

template <typename T>
int km_update(const T* x, int64_t ldx, int64_t n, int D, const int32_t* labels, const T* d2, const T* c_old, int M,
              T* c_new, int32_t* counts, double* stats, void* ws, void* stream) {
    if (!x && n > 0) return -1;
    if (!km_dim_ok(D)) return -4;
    if (ldx < D) return -2;
    if (!km_n_ok(n)) return -3;
    if (!labels && n > 0) return -5; if (!d2 && n > 0) return -6;
    if (!c_old) return -7; if (!km_m_ok(M)) return -8;
    if (!c_new) return -9; if (!counts) return -10; if (!stats) return -11; if (!ws) return -12;
    const KmPlan p = km_plan(n);
    double* part = (double*)ws;
    double* inert = part + p.nchunks * (int64_t)(2 * D + 1) * M;
    double* shift = inert + p.nchunks;
    const hipStream_t s = (hipStream_t)stream;
    return dispatch_dim<1, 2, 3>(D, [&](auto d) {
        constexpr int DS = decltype(d)::value;
        if (p.nchunks > 0) {
            const dim3 grid((unsigned)p.nchunks, (unsigned)cdiv64(M, KM_THREADS * KM_R));
            hipLaunchKernelGGL((km_partial_kernel<T, DS>), grid, dim3(KM_THREADS), 0, s, x, ldx, n, D, labels, d2, M,
                               p.stages, part, inert);
            if (int e = nsgp_launch_status()) return e;
        }
        hipLaunchKernelGGL((km_finish_kernel<T, DS>), dim3((unsigned)cdiv64(M, KM_KPB)), dim3(KM_THREADS), 0, s, part,
                           p.nchunks, D, c_old, M, c_new, counts, shift);
        if (int e = nsgp_launch_status()) return e;
        hipLaunchKernelGGL(km_stats_kernel, dim3(1), dim3(KM_THREADS), 0, s, inert, p.nchunks, shift, M, stats);
        return nsgp_launch_status();
    });
}

extern "C" {

int nsgp_kmeans_assign_f32(const float* x, int64_t ldx, int64_t n, int D, const float* c, int M, int32_t* labels,
                           float* d2, void* stream) {
    return km_assign<float>(x, ldx, n, D, c, M, labels, d2, stream);
}
int nsgp_kmeans_assign_f64(const double* x, int64_t ldx, int64_t n, int D, const double* c, int M, int32_t* labels,
                           double* d2, void* stream) {
    return km_assign<double>(x, ldx, n, D, c, M, labels, d2, stream);
}
size_t nsgp_kmeans_update_workspace(int64_t n, int D, int M) {
    if (!km_n_ok(n) || !km_dim_ok(D) || !km_m_ok(M)) return 0;
    const KmPlan p = km_plan(n);
    return sizeof(double) * (size_t)(p.nchunks * (int64_t)(2 * D + 1) * M + p.nchunks + M);
}
int nsgp_kmeans_update_f32(const float* x, int64_t ldx, int64_t n, int D, const int32_t* labels, const float* d2,
                           const float* c_old, int M, float* c_new, int32_t* counts, double* stats, void* ws,
                           void* stream) {
    return km_update<float>(x, ldx, n, D, labels, d2, c_old, M, c_new, counts, stats, ws, stream);
}
int nsgp_kmeans_update_f64(const double* x, int64_t ldx, int64_t n, int D, const int32_t* labels, const double* d2,
                           const double* c_old, int M, double* c_new, int32_t* counts, double* stats, void* ws,
                           void* stream) {
    return km_update<double>(x, ldx, n, D, labels, d2, c_old, M, c_new, counts, stats, ws, stream);
}

}  // extern "C"
