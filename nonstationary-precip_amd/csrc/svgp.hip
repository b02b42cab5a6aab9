// svgp.hip -- K6 SVGP epilogue / DeepGPLayer sampling and K7 ELBO reductions.
//
// gpytorch semantics restated (gpytorch itself is absent):
//   VariationalStrategy.forward : mean = A^T m + mu(x),  var = kxx + 1e-4 + colsum(A o ((S-I)A))
//                                 with S = Lq Lq^T  ->  colsum(C o C) - colsum(A o A), C = Lq^T A
//   DeepGPLayer.__call__        : h = mean + sqrt(var) * eps  (diagonal sampling)
//   GaussianLikelihood.expected_log_prob, VariationalELBO, DeepApproximateMLL, KL(q(u) || N(0,I))
// driven by models/dgps.py:48-51,92-98 and experiments/deepgp_spatial_bench.py:61,84-88.
// All of these are HBM-bound streaming passes over (M x n) or (S x n) data.
#include "common.h"

namespace {

// ---- pieces of the layer's reductions, each written once ("Layer reductions"); V = 16 / sizeof(T) elements per lane
template <typename T, int V> struct VecOf;
template <> struct VecOf<float, 4> { using type = float4; };
template <> struct VecOf<double, 2> { using type = double2; };

// V consecutive elements at p (V > 1: p is 16-byte aligned)
template <typename T, int V> __device__ __forceinline__ void ld_vec(const T* __restrict__ p, T (&v)[V]) {
    if constexpr (V == 1) {
        v[0] = p[0];
    } else {
        const typename VecOf<T, V>::type t = *reinterpret_cast<const typename VecOf<T, V>::type*>(p);
        v[0] = t.x; v[1] = t.y;
        if constexpr (V == 4) { v[2] = t.z; v[3] = t.w; }
    }
}
template <typename T, int V> __device__ __forceinline__ void st_vec(T* __restrict__ p, const T (&v)[V]) {
    if constexpr (V == 1) {
        p[0] = v[0];
    } else {
        typename VecOf<T, V>::type t;
        t.x = v[0]; t.y = v[1];
        if constexpr (V == 4) { t.z = v[2]; t.w = v[3]; }
        *reinterpret_cast<typename VecOf<T, V>::type*>(p) = t;
    }
}

// sum of the 16 / sizeof(T) products p[v] q[v], left to right (p, q 16-byte aligned)
template <typename T, int V = 16 / sizeof(T)> __device__ __forceinline__ T dot_vec(const T* p, const T* q) {
    T a[V], b[V];
    ld_vec<T, V>(p, a); ld_vec<T, V>(q, b);
    T s = a[0] * b[0];
    for (int v = 1; v < V; ++v) s += a[v] * b[v];
    return s;
}
// sum of the 16 / sizeof(T) elements at p, in pairs: (p0 + p1) + (p2 + p3)
template <typename T, int V = 16 / sizeof(T)> __device__ __forceinline__ T sum_vec(const T* p) {
    T a[V];
    ld_vec<T, V>(p, a);
    if constexpr (V == 4) return (a[0] + a[1]) + (a[2] + a[3]);
    else return a[0] + a[1];
}

// a row dot: may the 16-byte walk be taken; the scalar walk (one lane's share); block sum, thread 0 stores (lds: 4 elements)
template <typename T> __device__ __forceinline__ bool rowdot_vec_ok(const T* row, const T* gb, int64_t n) {
    return (n % (16 / sizeof(T)) == 0) && ((uintptr_t)row % 16 == 0) && ((uintptr_t)gb % 16 == 0);
}
template <typename T> __device__ __forceinline__ T rowdot_scalar(const T* row, const T* gb, int64_t n) {
    T acc = T(0);
    for (int64_t j = threadIdx.x; j < n; j += 256) acc += row[j] * gb[j];
    return acc;
}
template <typename T> __device__ __forceinline__ void block_sum_store(T acc, T* lds, T* out, int64_t at) {
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) out[at] = acc;
}

// s[k] = sum over the tile rows t of part[k][b, t, j]: K (batch, tiles, n) planes in ONE walk (K loads in flight per tile row)
template <typename TP, int K>
__device__ __forceinline__ void tile_sums(const TP* const (&part)[K], int64_t b, int64_t tiles, int64_t n, int64_t j, TP (&s)[K]) {
    for (int k = 0; k < K; ++k) s[k] = TP(0);
    for (int64_t t = 0; t < tiles; ++t)
        for (int k = 0; k < K; ++k) s[k] += part[k][(b * tiles + t) * n + j];
}
// the affine prior mean (gpytorch ConstantMean / LinearMean of models/dgps.py:40-43): sm += sum_d x[b,j,d] w[b,d], summed in TA
// from 0, then sm += c[b].  x / w / c batch strides may be 0 = shared; w or c may be null.
template <typename TA, typename T>
__device__ __forceinline__ void add_affine_mean(TA& sm, int64_t b, int64_t j, const T* x, int64_t sxb, int D, const T* w,
                                                int64_t swb, const T* c, int64_t scb) {
    if (w) {
        const T* xr = x + b * sxb + j * D;
        const T* wr = w + b * swb;
        TA mu = TA(0);
        for (int d = 0; d < D; ++d) mu += (TA)xr[d] * (TA)wr[d];
        sm += mu;
    }
    if (c) sm += (TA)c[b * scb];
}

// ---- colstats: mean[b,j] = sum_k A m ; var[b,j] = base[b] + sum_k (C^2 - A^2) ------------------
template <typename T>
__global__ __launch_bounds__(256) void colstats_kernel(const T* __restrict__ A, const T* __restrict__ C,
                                                       const T* __restrict__ m, const T* __restrict__ base,
                                                       int64_t M, int64_t n, T* __restrict__ mean,
                                                       T* __restrict__ var) {
    __shared__ T sm[4][64], sv[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t b = blockIdx.y, j = (int64_t)blockIdx.x * 64 + lane;
    const T* Ab = A + b * M * n;
    const T* Cb = C + b * M * n;
    const T* mb = m + b * M;
    T am = T(0), av = T(0);
    if (j < n) {
        const int64_t kq = (M + 3) / 4;
        const int64_t k0 = w * kq, k1 = (k0 + kq) < M ? (k0 + kq) : M;
        for (int64_t k = k0; k < k1; ++k) {
            const T a = Ab[k * n + j], c = Cb[k * n + j];
            am += a * mb[k];
            av += c * c - a * a;
        }
    }
    sm[w][lane] = am; sv[w][lane] = av;
    __syncthreads();
    if (w == 0 && j < n) {
        mean[b * n + j] = sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane];
        var[b * n + j] = base[b] + (sv[0][lane] + sv[1][lane] + sv[2][lane] + sv[3][lane]);
    }
}

// ---- colstats from the GEMM epilogues' per-tile-row partial sums ----------------------------------
// Optional affine prior mean added on the way out:  mean[b,j] += sum_d x[b,j,d] w[b,d] + c[b].
// TP: element type of the partial buffers (float64 partials of the float64-accumulating projections with a float32 layer)
template <typename T, typename TP = T>
__global__ void colstats_finalize_kernel(const TP* __restrict__ pdot, const TP* __restrict__ psqA,
                                         const TP* __restrict__ psqC, const T* __restrict__ base, T base_add,
                                         int64_t batch, int64_t tiles, int64_t n, const T* __restrict__ x,
                                         int64_t sxb, int D, const T* __restrict__ w, int64_t swb,
                                         const T* __restrict__ c, int64_t scb, T* __restrict__ mean,
                                         T* __restrict__ var) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int64_t b = idx / n, j = idx % n;
    TP s[3];                                             // dot, squares of A, squares of C
    tile_sums({pdot, psqA, psqC}, b, tiles, n, j, s);
    add_affine_mean(s[0], b, j, x, sxb, D, w, swb, c, scb);
    mean[idx] = (T)s[0];
    var[idx] = (T)(((TP)base[b] + (TP)base_add) + (s[2] - s[1]));
}

// ---- out[b][i] = sum_j A[b][i][j] * g[b][j]  (one workgroup per row; the m-gradient  A gmean) ------
template <typename T>
__global__ __launch_bounds__(256) void rowdot_kernel(const T* __restrict__ A, const T* __restrict__ g, int64_t M,
                                                     int64_t n, T* __restrict__ out) {
    __shared__ T lds[4];
    const int64_t b = blockIdx.y, i = blockIdx.x;
    const T* row = A + (b * M + i) * n;
    const T* gb = g + b * n;
    T acc = T(0);
    constexpr int V = 16 / sizeof(T);
    if (rowdot_vec_ok(row, gb, n))
        for (int64_t j = (int64_t)threadIdx.x * V; j < n; j += 256 * V) acc += dot_vec(row + j, gb + j);
    else
        acc = rowdot_scalar(row, gb, n);
    block_sum_store(acc, lds, out, b * M + i);
}

// ---- rowdot plus the reductions over the same columns that the layer's adjoint needs anyway:
//   rows i < M        : out[b,i]  = sum_j A[b,i,j] g[b,j]                      (mbar = A gmean)
//   row  M            : out_gv[b] = sum_j gv[b,j]                              (d/d outputscale through `base`)
//   row  M+1          : out_1     = sum_j g[b,j]                               (constant mean / bias gradient)
//   rows M+2 .. M+1+D : out_x[d]  = sum_j x[b,j,d] g[b,j]                      (linear-mean weight gradient)
// out_1 / out_x are per batch, or summed over the batch when the mean parameters are shared (`shared`).
// sum of q[0..n) by one 256-thread workgroup: 16-byte loads, four in flight per lane per trip (block-reduced; lds: 4 elements)
template <typename T> __device__ __forceinline__ T strided_sum4(const T* __restrict__ q, int64_t n, T* lds) {
    constexpr int V = 16 / sizeof(T);
    T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
    int64_t j = 0;
    if ((uintptr_t)q % 16 == 0) {
        const int64_t step = 256 * V;
        for (j = (int64_t)threadIdx.x * V; j + 3 * step + V <= n; j += 4 * step) {
            a0 += sum_vec(q + j); a1 += sum_vec(q + j + step); a2 += sum_vec(q + j + 2 * step); a3 += sum_vec(q + j + 3 * step);
        }
        for (; j + V <= n; j += step) a0 += sum_vec(q + j);
        // ragged end: elements [n - n % V, n) by the first lanes
        const int64_t tail0 = n - n % V;
        if ((int64_t)threadIdx.x < n - tail0) a1 += q[tail0 + threadIdx.x];
    } else {
        for (j = threadIdx.x; j + 768 < n; j += 1024) { a0 += q[j]; a1 += q[j + 256]; a2 += q[j + 512]; a3 += q[j + 768]; }
        for (; j < n; j += 256) a0 += q[j];
    }
    return block_sum_256((a0 + a1) + (a2 + a3), lds);
}

template <typename T>
__global__ __launch_bounds__(256) void rowdot_affine_kernel(const T* __restrict__ A, const T* __restrict__ g,
                                                            const T* __restrict__ gv, const T* __restrict__ x,
                                                            int64_t sxb, int D, int shared, int64_t batch, int64_t M,
                                                            int64_t n, T* __restrict__ out, T* __restrict__ out_gv,
                                                            T* __restrict__ out_x, T* __restrict__ out_1) {
    __shared__ T lds[4];
    const int64_t b = blockIdx.y, i = blockIdx.x;
    T acc = T(0);
    if (i < M) {
        const T* row = A + (b * M + i) * n;
        const T* gb = g + b * n;
        constexpr int V = 16 / sizeof(T);
        if (rowdot_vec_ok(row, gb, n)) {
            // Chunks of 256 lanes x 16 bytes, walked from a start that differs from row to row: rows are n elements apart
            // (160 KB at the headline's last layer, a multiple of the memory channels' interleave), so workgroups that all
            // begin at column 0 march through the SAME channel together.  Eight chunks in flight per lane.
            const int64_t nch = (n + 256 * V - 1) / (256 * V);
            const int64_t c0 = i % nch;
            T a1 = T(0), a2 = T(0), a3 = T(0);
            auto chunk = [&](int64_t t, T& dst) __attribute__((always_inline)) {
                int64_t c = c0 + t;
                if (c >= nch) c -= nch;
                const int64_t j = (c * 256 + threadIdx.x) * V;
                if (j < n) dst += dot_vec(row + j, gb + j);
            };
            int64_t t = 0;
            for (; t + 7 < nch; t += 8) {
                chunk(t, acc); chunk(t + 1, a1); chunk(t + 2, a2); chunk(t + 3, a3);
                chunk(t + 4, acc); chunk(t + 5, a1); chunk(t + 6, a2); chunk(t + 7, a3);
            }
            for (; t < nch; ++t) chunk(t, acc);
            acc = (acc + a1) + (a2 + a3);
        } else {
            acc = rowdot_scalar(row, gb, n);
        }
        block_sum_store(acc, lds, out, b * M + i);
        return;
    }
    const int e = (int)(i - M);
    if (e == 0) {
        if (!gv) return;
        // (the virtual rows are ONE workgroup each: with a dependent-latency loop of n / 256 scalar loads they, not the M
        // rows of A, set the launch's duration -- 87 of 100 us at n = 40960.  Four independent loads per lane per trip.)
        acc = strided_sum4(gv + b * n, n, lds);
        if (threadIdx.x == 0) out_gv[b] = acc;
        return;
    }
    if (e == 1 ? !out_1 : !out_x) return;
    if (shared && b != 0) return;
    const int64_t b1 = shared ? batch : b + 1;
    for (int64_t bb = b; bb < b1; ++bb) {
        const T* gb = g + bb * n;
        T a0 = T(0), a1 = T(0), a2 = T(0), a3 = T(0);
        int64_t j = threadIdx.x;
        if (e == 1) {
            acc += strided_sum4(gb, n, lds);             // (block-reduced already: every lane holds the sum)
            __syncthreads();
            continue;
        }
        const T* xc = x + bb * sxb + (e - 2);
        for (; j + 1792 < n; j += 2048) {                // eight (g, x) pairs in flight per lane
            T gq[8], xq[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { gq[u] = gb[j + 256 * u]; xq[u] = xc[(j + 256 * u) * D]; }
            a0 += xq[0] * gq[0] + xq[4] * gq[4]; a1 += xq[1] * gq[1] + xq[5] * gq[5];
            a2 += xq[2] * gq[2] + xq[6] * gq[6]; a3 += xq[3] * gq[3] + xq[7] * gq[7];
        }
        for (; j < n; j += 256) a0 += xc[j * D] * gb[j];
        acc += (a0 + a1) + (a2 + a3);
    }
    if (e != 1) acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) {
        if (e == 1) out_1[shared ? 0 : b] = acc;
        else out_x[(shared ? 0 : b) * D + (e - 2)] = acc;
    }
}

// ---- colstats backward: one block per (row k, batch b) ------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void colstats_bwd_kernel(const T* __restrict__ A, const T* __restrict__ C,
                                                           const T* __restrict__ m, const T* __restrict__ gmean,
                                                           const T* __restrict__ gvar, int64_t M, int64_t n,
                                                           T* __restrict__ Abar, T* __restrict__ C2,
                                                           T* __restrict__ mbar) {
    __shared__ T lds[4];
    const int64_t b = blockIdx.y, k = blockIdx.x;
    const int64_t off = (b * M + k) * n;
    const T mk = m[b * M + k];
    const T* gm = gmean + b * n;
    const T* gv = gvar + b * n;
    T acc = T(0);
    for (int64_t j = threadIdx.x; j < n; j += 256) {
        const T a = A[off + j], g1 = gm[j], g2 = T(2) * gv[j];
        acc += a * g1;
        Abar[off + j] = mk * g1 - g2 * a;
        C2[off + j] = g2 * C[off + j];
    }
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) mbar[b * M + k] = acc;
}

// ---- sampling ------------------------------------------------------------------------------------
template <typename T>
__global__ void sample_fwd_kernel(const T* __restrict__ mean, const T* __restrict__ var, const T* __restrict__ eps,
                                  int64_t S, int64_t ns, int64_t n, int64_t b, T* __restrict__ h) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= S * n * b) return;
    const int64_t c = idx % b, i = (idx / b) % n, s = idx / (b * n);
    const int64_t sp = ns == 1 ? 0 : s;
    const int64_t q = (c * ns + sp) * n + i;
    h[idx] = mean[q] + t_sqrt(var[q]) * eps[idx];
}

template <typename T>
__global__ void sample_bwd_kernel(const T* __restrict__ var, const T* __restrict__ eps, const T* __restrict__ gh,
                                  int64_t S, int64_t ns, int64_t n, int64_t b, T* __restrict__ gmean,
                                  T* __restrict__ gvar) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= b * ns * n) return;
    const int64_t i = q % n, sp = (q / n) % ns, c = q / (n * ns);
    const T hs = T(0.5) / t_sqrt(var[q]);
    T gm = T(0), gv = T(0);
    const int64_t s0 = ns == 1 ? 0 : sp, s1 = ns == 1 ? S : sp + 1;
    for (int64_t s = s0; s < s1; ++s) {
        const int64_t idx = (s * n + i) * b + c;
        const T g = gh[idx];
        gm += g;
        gv += g * eps[idx] * hs;
    }
    gmean[q] = gm;
    gvar[q] = gv;
}

// ---- the terms of the DSVI objective: every piece of arithmetic once -------------------------------------------------
// The kernels further down are schedulers: each works out which (sample | group, batch element, chunk) a block owns and
// calls a piece, so the per-term, the one-scalar and the fused entry points run the same text ("Objective
// terms").  A piece is inlined with the contraction mode of THIS place (the default), whatever its caller sets.

// sum of part[lo, hi) over one 256-thread workgroup (valid in thread 0; lds: 4 elements): second stage of every reduction
template <typename T>
__device__ __forceinline__ T part_sum(const T* __restrict__ part, int64_t lo, int64_t hi, T* lds) {
    T s = T(0);
    for (int64_t t = lo + threadIdx.x; t < hi; t += 256) s += part[t];
    return block_sum_256(s, lds);
}

// one point of the Gaussian expected log-likelihood, d = y - mu, e = d^2 + v:  -1/2 (e / s2 + log s2 + log 2pi), or (GN)
// its derivative with respect to the noise s2:  1/2 (e / s2^2 - 1 / s2)
template <typename T, bool GN> __device__ __forceinline__ T gauss_term(T d, T v, T is2, T ls2) {
    const T e = d * d + v;
    if constexpr (GN) return T(0.5) * (e * is2 * is2 - is2);
    else return T(-0.5) * (e * is2 + ls2 + T(1.8378770664093454835606594728112));
}

// this lane's sum of the term (gn: of its noise gradient) over points first, first + stride, ... < n of one sample row (mu,
// v: that row).  gn selects per point: a caller that passes a constant gets the plain loop, and gauss_ell_part_kernel, which
// passes its argument, keeps the select inside the loop -- and with it the un-contracted add it has always rounded with.
template <typename T>
__device__ __forceinline__ T gauss_row_sum(const T* __restrict__ y, const T* __restrict__ mu, const T* __restrict__ v,
                                           const T* __restrict__ noise, int64_t first, int64_t stride, int64_t n, bool gn) {
    const T s2 = noise[0];
    const T is2 = T(1) / s2, ls2 = t_log(s2);
    T acc = T(0);
    for (int64_t i = first; i < n; i += stride) {
        const T d = y[i] - mu[i];
        acc += gn ? gauss_term<T, true>(d, v[i], is2, ls2) : gauss_term<T, false>(d, v[i], is2, ls2);
    }
    return acc;
}

// gmu, gv at element idx of (S, n) for the upstream factor coef (upstream gradient times the term's scale)
template <typename T>
__device__ __forceinline__ void gauss_adjoint_at(int64_t idx, const T* __restrict__ y, const T* __restrict__ mu,
                                                 const T* __restrict__ noise, int64_t n, T coef, T* __restrict__ gmu,
                                                 T* __restrict__ gv) {
    const T is2 = T(1) / noise[0];
    gmu[idx] = coef * (y[idx % n] - mu[idx]) * is2;
    gv[idx] = T(-0.5) * coef * is2;
}

// ---- Gauss-Hermite log marginal: log int p(y | f) N(f | mu, v) df ~ log(pi^-1/2 sum_k w_k p(y | mu + sqrt(2 v) t_k)) for a
// likelihood of one latent value.  KIND 0: Bernoulli with a probit link, log p = log Phi((2 y - 1) f); KIND 1: Student-t with
// nu degrees of freedom, location f and scale sqrt(s2) -- its f-dependent part -(nu + 1)/2 log1p(r^2 / (nu s2)) - 1/2 log s2,
// r = y - f (the normaliser lgamma((nu + 1)/2) - lgamma(nu/2) - 1/2 log(nu pi) is the caller's).
constexpr int GH_MAX_Q = 64;
constexpr int GH_BERNOULLI = 0, GH_STUDENT_T = 1;

template <typename T> __device__ __forceinline__ T t_log1p(T x);
template <> __device__ __forceinline__ float t_log1p<float>(float x) { return log1pf(x); }
template <> __device__ __forceinline__ double t_log1p<double>(double x) { return log1p(x); }
template <typename T> __device__ __forceinline__ T t_erfc(T x);
template <> __device__ __forceinline__ float t_erfc<float>(float x) { return erfcf(x); }
template <> __device__ __forceinline__ double t_erfc<double>(double x) { return erfc(x); }
template <typename T> __device__ __forceinline__ T t_erfcx(T x);     // exp(x^2) erfc(x)
template <> __device__ __forceinline__ float t_erfcx<float>(float x) { return erfcxf(x); }
template <> __device__ __forceinline__ double t_erfcx<double>(double x) { return erfcx(x); }

// what a term needs of (nu, s2), worked out once per thread (Bernoulli: nothing)
template <typename T> struct GhParams { T ia, hnp1, hls2; };             // 1/(nu s2), (nu + 1)/2, 1/2 log s2
template <typename T, int KIND> __device__ __forceinline__ GhParams<T> gh_params(const T* __restrict__ params) {
    GhParams<T> P{};
    if constexpr (KIND == GH_STUDENT_T) {
        const T nu = params[0], s2 = params[1];
        P.ia = T(1) / (nu * s2); P.hnp1 = T(0.5) * (nu + T(1)); P.hls2 = T(0.5) * t_log(s2);
    }
    return P;
}

// nodes and weights (the weights times pi^-1/2) into the workgroup's LDS: every lane reads all Q of them per point
template <typename T>
__device__ __forceinline__ void gh_stage_rule(const T* __restrict__ nodes, const T* __restrict__ weights, int Q, T* sn, T* sw) {
    if ((int)threadIdx.x < Q) {
        sn[threadIdx.x] = nodes[threadIdx.x];
        sw[threadIdx.x] = weights[threadIdx.x] * T(0.56418958354775628694807945156077);
    }
    __syncthreads();
}

// log p(y | f) at one node.
// log Phi(z): z <= 0 through the scaled complementary error function, log(erfcx(-z / sqrt 2) / 2) - z^2 / 2, finite and
// accurate down to the z ~ -29 the nodes reach (erfc itself underflows near z = -13 in float32); z > 0 as
// log1p(-erfc(z / sqrt 2) / 2).  A NaN z fails `z <= 0` and leaves the second branch as a NaN.
template <typename T, int KIND>
__device__ __forceinline__ T gh_term(T y, T f, const GhParams<T>& P) {
    if constexpr (KIND == GH_BERNOULLI) {
        const T z = (T(2) * y - T(1)) * f;
        if (z <= T(0)) return t_log(T(0.5) * t_erfcx(-z * T(0.70710678118654752440084436210485))) - T(0.5) * z * z;
        return t_log1p(T(-0.5) * t_erfc(z * T(0.70710678118654752440084436210485)));
    } else {
        const T r = y - f;
        return -P.hnp1 * t_log1p(r * r * P.ia) - P.hls2;
    }
}

// the Q-node log marginal of one point as a running log-sum-exp (the largest log p so far is factored out: at z ~ -29
// every p underflows)
template <typename T, int KIND>
__device__ __forceinline__ T gh_point_lse(T y, T mu, T v, const GhParams<T>& P, const T* sn, const T* sw, int Q) {
    const T sd = t_sqrt(T(2) * v);
    T m = T(0), s = T(0);
    for (int k = 0; k < Q; ++k) {
        const T lp = gh_term<T, KIND>(y, mu + sd * sn[k], P);
        if (k == 0) { m = lp; s = sw[0]; }
        else if (lp > m) { s = s * t_exp(m - lp) + sw[k]; m = lp; }
        else s += sw[k] * t_exp(lp - m);                 // (a NaN lp lands here and makes s a NaN)
    }
    return m + t_log(s);
}

// this lane's share of  sum_{j <= i} l_ij^2 + sum_i (m_i^2 - 2 log |l_ii|)  (twice KL(N(m, L L^T) || N(0, I)), plus M) over
// rows xb, xb + nblk, ... of one (m, L); only the lower triangle is read (no 64-bit div/mod per element)
template <typename T>
__device__ __forceinline__ T kl_rows_sum(const T* __restrict__ m, const T* __restrict__ L, int64_t M, int64_t xb,
                                         int64_t nblk) {
    T acc = T(0);
    for (int64_t i = xb; i < M; i += nblk) {
        const T* row = L + i * M;
        for (int64_t j = threadIdx.x; j <= i; j += 256) {
            const T l = row[j];
            acc += l * l;
            if (j == i) acc += m[i] * m[i] - T(2) * t_log(l < T(0) ? -l : l);
        }
    }
    return acc;
}

// gLq at element idx of one (batch, M, M) group (zero above the diagonal), and gm beside each diagonal element, for the
// upstream factor go
template <typename T>
__device__ __forceinline__ void kl_adjoint_at(int64_t idx, const T* __restrict__ m, const T* __restrict__ Lq, int64_t M, T go,
                                              T* __restrict__ gm, T* __restrict__ gLq) {
    const int64_t e = idx % (M * M), b = idx / (M * M);
    const int64_t i = e / M, j = e % M;
    T g = T(0);
    if (j <= i) {
        const T l = Lq[idx];
        g = go * (i == j ? l - T(1) / l : l);
        if (i == j) gm[b * M + i] = go * m[b * M + i];
    }
    gLq[idx] = g;
}

// ---- per-term kernels --------------------------------------------------------------------------------------------------
// out[o] = scale * sum(part[o nparts .. (o + 1) nparts)) + add (+ add_dev[o])
template <typename T>
__global__ __launch_bounds__(256) void reduce_final_kernel(const T* __restrict__ part, int64_t nparts, int64_t nout,
                                                           T scale, T add, T* __restrict__ out,
                                                           const T* __restrict__ add_dev = nullptr) {
    __shared__ T lds[4];
    const int64_t o = blockIdx.x;
    if (o >= nout) return;
    const T s = part_sum(part, o * nparts, (o + 1) * nparts, lds);
    if (threadIdx.x == 0) out[o] = scale * s + add + (add_dev ? add_dev[o] : T(0));
}

// part[s * gridDim.x + blk] = (gout ? gout[s * gs] : 1) * sum over block blk's chunk of sample row s of the Gaussian term, or
// (want_gnoise) of its noise gradient                                                       (gs = 0: one shared gout)
template <typename T>
__global__ __launch_bounds__(256) void gauss_ell_part_kernel(const T* __restrict__ y, const T* __restrict__ mu,
                                                             const T* __restrict__ v, const T* __restrict__ noise,
                                                             const T* __restrict__ gout, int64_t gs, int64_t n,
                                                             int want_gnoise, T* __restrict__ part) {
    __shared__ T lds[4];
    const int64_t s = blockIdx.y;
    T acc = gauss_row_sum(y, mu + s * n, v + s * n, noise, (int64_t)blockIdx.x * 256 + threadIdx.x,
                          (int64_t)gridDim.x * 256, n, want_gnoise != 0);
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[s * gridDim.x + blockIdx.x] = gout ? gout[s * gs] * acc : acc;
}

template <typename T>
__global__ void gauss_ell_bwd_kernel(const T* __restrict__ y, const T* __restrict__ mu, const T* __restrict__ noise,
                                     const T* __restrict__ gout, int64_t gs, int64_t S, int64_t n, T scale,
                                     T* __restrict__ gmu, T* __restrict__ gv) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < S * n) gauss_adjoint_at(idx, y, mu, noise, n, gout[(idx / n) * gs] * scale, gmu, gv);
}

// out[s, i] = log(pi^-1/2 sum_k w_k p(y_i | mu_si + sqrt(2 v_si) t_k)), one lane per point
template <typename T, int KIND>
__global__ __launch_bounds__(256) void gh_log_marginal_kernel(const T* __restrict__ y, const T* __restrict__ mu,
                                                              const T* __restrict__ v, const T* __restrict__ params,
                                                              const T* __restrict__ nodes, const T* __restrict__ weights,
                                                              int Q, int64_t S, int64_t n, T* __restrict__ out) {
    __shared__ T sn[GH_MAX_Q], sw[GH_MAX_Q];
    gh_stage_rule(nodes, weights, Q, sn, sw);
    const GhParams<T> P = gh_params<T, KIND>(params);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx < S * n) out[idx] = gh_point_lse<T, KIND>(y[idx % n], mu[idx], v[idx], P, sn, sw, Q);
}

// part[b * gridDim.x + blk] = block blk's rows of batch element b
template <typename T>
__global__ __launch_bounds__(256) void kl_part_kernel(const T* __restrict__ m, const T* __restrict__ Lq, int64_t M,
                                                      T* __restrict__ part) {
    __shared__ T lds[4];
    const int64_t b = blockIdx.y;
    T acc = kl_rows_sum(m + b * M, Lq + b * M * M, M, (int64_t)blockIdx.x, (int64_t)gridDim.x);
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[b * gridDim.x + blockIdx.x] = acc;
}

template <typename T>
__global__ void kl_bwd_kernel(const T* __restrict__ m, const T* __restrict__ Lq, int64_t batch, int64_t M, T gout,
                              const T* __restrict__ gdev, T* __restrict__ gm, T* __restrict__ gLq) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * M * M) return;
    if (gdev) gout *= gdev[0];                          // upstream gradient read on the device (no host scalar)
    kl_adjoint_at(idx, m, Lq, M, gout, gm, gLq);
}

template <typename T>
int colstats_impl(const T* A, const T* C, const T* m, const T* base, int64_t batch, int64_t M, int64_t n, T* mean,
                  T* var, void* stream) {
    if (!A) return -1; if (!C) return -2; if (!m) return -3; if (!base) return -4;
    if (batch < 0) return -5; if (M < 0) return -6; if (n < 0) return -7; if (!mean) return -8; if (!var) return -9;
    if (batch == 0 || n == 0) return 0;
    hipLaunchKernelGGL((colstats_kernel<T>), dim3((unsigned)cdiv64(n, 64), (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, A, C, m, base, M, n, mean, var);
    return nsgp_launch_status();
}

template <typename T>
int colstats_bwd_impl(const T* A, const T* C, const T* m, const T* gmean, const T* gvar, int64_t batch, int64_t M,
                      int64_t n, T* Abar, T* C2, T* mbar, void* stream) {
    if (!A) return -1; if (!C) return -2; if (!m) return -3; if (!gmean) return -4; if (!gvar) return -5;
    if (batch < 0) return -6; if (M < 0) return -7; if (n < 0) return -8;
    if (!Abar) return -9; if (!C2) return -10; if (!mbar) return -11;
    if (batch == 0 || M == 0) return 0;
    hipLaunchKernelGGL((colstats_bwd_kernel<T>), dim3((unsigned)M, (unsigned)batch), dim3(256), 0, (hipStream_t)stream,
                       A, C, m, gmean, gvar, M, n, Abar, C2, mbar);
    return nsgp_launch_status();
}

template <typename T>
int sample_fwd_impl(const T* mean, const T* var, const T* eps, int64_t S, int64_t ns, int64_t n, int64_t b, T* h,
                    void* stream) {
    if (!mean) return -1; if (!var) return -2; if (!eps) return -3;
    if (S < 0) return -4; if (ns != 1 && ns != S) return -5; if (n < 0) return -6; if (b < 0) return -7; if (!h) return -8;
    const int64_t tot = S * n * b;
    if (tot == 0) return 0;
    hipLaunchKernelGGL((sample_fwd_kernel<T>), dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                       mean, var, eps, S, ns, n, b, h);
    return nsgp_launch_status();
}

template <typename T>
int sample_bwd_impl(const T* var, const T* eps, const T* gh, int64_t S, int64_t ns, int64_t n, int64_t b, T* gmean,
                    T* gvar, void* stream) {
    if (!var) return -1; if (!eps) return -2; if (!gh) return -3;
    if (S < 0) return -4; if (ns != 1 && ns != S) return -5; if (n < 0) return -6; if (b < 0) return -7;
    if (!gmean) return -8; if (!gvar) return -9;
    const int64_t tot = b * ns * n;
    if (tot == 0) return 0;
    hipLaunchKernelGGL((sample_bwd_kernel<T>), dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream,
                       var, eps, gh, S, ns, n, b, gmean, gvar);
    return nsgp_launch_status();
}

// blocks of partial sums: per sample row of the likelihood (each strides over the row by nblk * 256), per batch element of
// the whitened KL (rows stride by nblk), and over all tot = batch * M > 0 elements of the mean-field KL
static inline int64_t gauss_blocks(int64_t n) {
    int64_t nblk = cdiv64(n, 1024); if (nblk > 64) nblk = 64; if (nblk < 1) nblk = 1;
    return nblk;
}
static inline int64_t kl_blocks(int64_t M) {
    int64_t nblk = cdiv64(M * M, 1024); if (nblk > 256) nblk = 256; if (nblk < 1) nblk = 1;
    return nblk;
}
static inline int64_t kl_diag_blocks(int64_t tot) { return cdiv64(tot, 1024) > 256 ? 256 : cdiv64(tot, 1024); }

// `total`: out[0] = scale * sum over ALL samples and points (the caller folds 1/S into scale), one launch less
// downstream than an (S,) vector followed by a mean; the backward then takes ONE upstream gradient gout[0].
template <typename T>
int gauss_fwd_impl(const T* y, const T* mu, const T* v, const T* noise, int64_t S, int64_t n, T scale, T* out,
                   void* ws, size_t wsb, void* stream, bool total = false) {
    if (!y) return -1; if (!mu) return -2; if (!v) return -3; if (!noise) return -4;
    if (S < 0 || S > 65535) return -5; if (n < 0) return -6; if (!out) return -8;
    if (S == 0) return 0;
    const int64_t nblk = gauss_blocks(n);
    if (!ws || wsb < (size_t)(S * nblk) * sizeof(T)) return -9;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((gauss_ell_part_kernel<T>), dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, st, y, mu, v, noise,
                       (const T*)nullptr, (int64_t)0, n, 0, (T*)ws);
    const int64_t nout = total ? 1 : S;                  // one sum of all S nblk partials, or S sums of nblk
    hipLaunchKernelGGL((reduce_final_kernel<T>), dim3((unsigned)nout), dim3(256), 0, st, (const T*)ws, S * nblk / nout, nout,
                       scale, T(0), out);
    return nsgp_launch_status();
}

template <typename T>
int gauss_bwd_impl(const T* y, const T* mu, const T* v, const T* noise, int64_t S, int64_t n, T scale, const T* gout,
                   T* gmu, T* gv, T* gnoise, void* ws, size_t wsb, void* stream, bool total = false) {
    const int64_t gs = total ? 0 : 1;
    if (!y) return -1; if (!mu) return -2; if (!v) return -3; if (!noise) return -4;
    if (S < 0 || S > 65535) return -5; if (n < 0) return -6; if (!gout) return -8; if (!gmu) return -9;
    if (!gv) return -10;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tot = S * n;
    if (tot > 0)
        hipLaunchKernelGGL((gauss_ell_bwd_kernel<T>), dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, st, y, mu, noise,
                           gout, gs, S, n, scale, gmu, gv);
    if (gnoise) {
        const int64_t nblk = gauss_blocks(n);
        if (!ws || wsb < (size_t)(S * nblk + 1) * sizeof(T)) return -12;
        if (S > 0)
            hipLaunchKernelGGL((gauss_ell_part_kernel<T>), dim3((unsigned)nblk, (unsigned)S), dim3(256), 0, st, y, mu,
                               v, noise, gout, gs, n, 1, (T*)ws);
        hipLaunchKernelGGL((reduce_final_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)ws, S * nblk, (int64_t)1,
                           scale, T(0), gnoise);
    }
    return nsgp_launch_status();
}

// Gauss-Hermite log marginal of a likelihood `kind` with Q nodes: argument checks (minus the position) and the launch
static inline int gh_check(int kind, const void* y, const void* mu, const void* v, const void* params, const void* nodes,
                           const void* weights, int64_t Q, int64_t S, int64_t n) {
    if (kind != GH_BERNOULLI && kind != GH_STUDENT_T) return -1;
    if (!y) return -2; if (!mu) return -3; if (!v) return -4;
    if ((kind == GH_STUDENT_T) != (params != nullptr)) return -5;
    if (!nodes) return -6; if (!weights) return -7; if (Q < 1 || Q > GH_MAX_Q) return -8;
    if (S < 0 || S > 65535) return -9; if (n < 0) return -10;
    return 0;
}

template <typename T>
int gh_log_marginal_impl(int kind, const T* y, const T* mu, const T* v, const T* params, const T* nodes, const T* weights,
                         int64_t Q, int64_t S, int64_t n, T* out, void* stream) {
    if (const int rc = gh_check(kind, y, mu, v, params, nodes, weights, Q, S, n)) return rc;
    if (!out) return -11;
    if (S == 0 || n == 0) return 0;
    if (n > 2147483647LL * 256 / S) return -10;          // S n lanes in blocks of 256: the grid's x extent
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)cdiv64(S * n, 256));
    if (kind == GH_BERNOULLI)
        hipLaunchKernelGGL((gh_log_marginal_kernel<T, GH_BERNOULLI>), grid, dim3(256), 0, st, y, mu, v, params, nodes, weights,
                           (int)Q, S, n, out);
    else
        hipLaunchKernelGGL((gh_log_marginal_kernel<T, GH_STUDENT_T>), grid, dim3(256), 0, st, y, mu, v, params, nodes, weights,
                           (int)Q, S, n, out);
    return nsgp_launch_status();
}

template <typename T>
int kl_fwd_impl(const T* m, const T* Lq, int64_t batch, int64_t M, T* out, void* ws, size_t wsb, void* stream,
                bool total = false, T scale = T(1), const T* addin = nullptr) {
    if (!m) return -1; if (!Lq) return -2; if (batch < 0) return -3; if (M < 0) return -4; if (!out) return -5;
    if (batch == 0) return 0;
    const int64_t nblk = kl_blocks(M);
    if (!ws || wsb < (size_t)(batch * nblk) * sizeof(T)) return -6;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((kl_part_kernel<T>), dim3((unsigned)nblk, (unsigned)batch), dim3(256), 0, st, m, Lq, M, (T*)ws);
    const int64_t nout = total ? 1 : batch;              // total: out[0] = addin[0] + scale * sum_b KL_b; else scale is 1
    hipLaunchKernelGGL((reduce_final_kernel<T>), dim3((unsigned)nout), dim3(256), 0, st, (const T*)ws, batch * nblk / nout,
                       nout, T(0.5) * scale, T(-0.5) * T(M) * T(batch / nout) * scale, out, addin);
    return nsgp_launch_status();
}

template <typename T>
int kl_bwd_impl(const T* m, const T* Lq, int64_t batch, int64_t M, T gout, T* gm, T* gLq, void* stream,
                const T* gdev = nullptr) {
    if (!m) return -1; if (!Lq) return -2; if (batch < 0) return -3; if (M < 0) return -4; if (!gm) return -6;
    if (!gLq) return -7;
    const int64_t tot = batch * M * M;
    if (tot == 0) return 0;
    hipLaunchKernelGGL((kl_bwd_kernel<T>), dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream, m, Lq,
                       batch, M, gout, gdev, gm, gLq);
    return nsgp_launch_status();
}

// ---- the whole DSVI objective as ONE scalar: two launches forward, two backward -------------------------------------
// out = ell_scale * sum_s sum_i E_q log N(y_i | f_si, noise) + kl_scale * sum_groups sum_b KL(N(m_b, Lq_b Lq_b^T) || N(0, I))
// (the caller folds 1/(B S), 1/num_data and the sign into the two scales).  The chain of per-term reductions this replaces
// cost 6 launches forward and 5 backward for the 2-layer model, ~5 us each under graph replay.
constexpr int OBJ_MAX_GROUPS = 8;
template <typename T> struct ObjGroups {
    const T* m[OBJ_MAX_GROUPS];
    const T* Lq[OBJ_MAX_GROUPS];
    T* gm[OBJ_MAX_GROUPS];
    T* gLq[OBJ_MAX_GROUPS];
    int batch[OBJ_MAX_GROUPS];
    int blk0[OBJ_MAX_GROUPS + 1];        // first block of each group in the KL region of a grid
    int ng;
};

// the group g that block kb of a grid's KL region belongs to
template <typename T> __device__ __forceinline__ int obj_group_of(const ObjGroups<T>& G, int kb) {
    int g = 0;
    while (g + 1 < G.ng && kb >= G.blk0[g + 1]) ++g;
    return g;
}

// blocks [0, S nblk_e): likelihood partials (block (s, x) strides over row s, as gauss_ell_part_kernel's); then, per group
// and batch element, nblk_k blocks of KL partials (rows x, x + nblk_k, ... as kl_part_kernel's)
template <typename T>
__global__ __launch_bounds__(256) void dsvi_obj_part_kernel(const T* __restrict__ y, const T* __restrict__ mu,
                                                            const T* __restrict__ v, const T* __restrict__ noise, int64_t n,
                                                            int nblk_e, int n_ell, ObjGroups<T> G, int64_t M, int nblk_k,
                                                            T* __restrict__ part) {
    __shared__ T lds[4];
    const int b = (int)blockIdx.x;
    T acc;
    if (b < n_ell) {
        const int64_t s = b / nblk_e, xb = b % nblk_e;
        acc = gauss_row_sum(y, mu + s * n, v + s * n, noise, xb * 256 + threadIdx.x, (int64_t)nblk_e * 256, n, false);
    } else {
        const int kb = b - n_ell, g = obj_group_of(G, kb);
        const int rel = kb - G.blk0[g];
        const int64_t bi = rel / nblk_k, xb = rel % nblk_k;
        acc = kl_rows_sum(G.m[g] + bi * M, G.Lq[g] + bi * M * M, M, xb, (int64_t)nblk_k);
    }
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[b] = acc;
}

// out[0] = ell_scale * sum(part[0 .. n_ell)) + kl_scale * (1/2 sum(part[n_ell .. n_all)) - kl_half_const)
template <typename T>
__global__ __launch_bounds__(256) void dsvi_obj_final_kernel(const T* __restrict__ part, int n_ell, int n_all, T ell_scale,
                                                             T kl_scale, T kl_half_const, T* __restrict__ out) {
    __shared__ T lds[4];
    const T a = part_sum(part, (int64_t)0, (int64_t)n_ell, lds);
    __syncthreads();
    const T k = part_sum(part, (int64_t)n_ell, (int64_t)n_all, lds);
    if (threadIdx.x == 0) out[0] = ell_scale * a + kl_scale * (T(0.5) * k - kl_half_const);
}

// backward: blocks [0, nb_e): gmu / gv; then per group its gLq / gm elements; then (want_gn) S nblk_e blocks of
// noise-gradient partials.  gout[0] is the upstream gradient of the scalar, read on the device.
template <typename T>
__global__ __launch_bounds__(256) void dsvi_obj_bwd_kernel(const T* __restrict__ y, const T* __restrict__ mu,
                                                           const T* __restrict__ v, const T* __restrict__ noise, int64_t S,
                                                           int64_t n, T ell_scale, T kl_scale, const T* __restrict__ gout,
                                                           int nb_e, ObjGroups<T> G, int64_t M, int nb_kl, int nblk_e,
                                                           T* __restrict__ gmu, T* __restrict__ gv, T* __restrict__ part_gn) {
    __shared__ T lds[4];
    const int b = (int)blockIdx.x;
    const T up = gout[0];
    if (b < nb_e) {
        const int64_t idx = (int64_t)b * 256 + threadIdx.x;
        if (idx < S * n) gauss_adjoint_at(idx, y, mu, noise, n, up * ell_scale, gmu, gv);
        return;
    }
    if (b < nb_e + nb_kl) {
        const int kb = b - nb_e, g = obj_group_of(G, kb);
        const int64_t idx = (int64_t)(kb - G.blk0[g]) * 256 + threadIdx.x;
        if (idx < (int64_t)G.batch[g] * M * M) kl_adjoint_at(idx, G.m[g], G.Lq[g], M, up * kl_scale, G.gm[g], G.gLq[g]);
        return;
    }
    const int rb = b - nb_e - nb_kl;
    const int64_t s = rb / nblk_e, xb = rb % nblk_e;
    T acc = gauss_row_sum(y, mu + s * n, v + s * n, noise, xb * 256 + threadIdx.x, (int64_t)nblk_e * 256, n, true);
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part_gn[rb] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void dsvi_obj_gnoise_kernel(const T* __restrict__ part, int nparts, T ell_scale,
                                                              const T* __restrict__ gout, T* __restrict__ gnoise) {
    __shared__ T lds[4];
    const T a = part_sum(part, (int64_t)0, (int64_t)nparts, lds);
    if (threadIdx.x == 0) gnoise[0] = gout[0] * ell_scale * a;
}

template <typename T>
static int obj_groups(ObjGroups<T>& G, int ngroups, const void* const* m, const void* const* Lq, void* const* gm, void* const* gLq,
                      const int64_t* batch, int64_t per_batch_blocks_or_elems, bool elems, int64_t M) {
    G.ng = ngroups;
    int64_t off = 0;
    for (int g = 0; g < ngroups; ++g) {
        if (!m[g] || !Lq[g] || batch[g] < 1) return -1;
        G.m[g] = (const T*)m[g]; G.Lq[g] = (const T*)Lq[g];
        G.gm[g] = gm ? (T*)gm[g] : nullptr; G.gLq[g] = gLq ? (T*)gLq[g] : nullptr;
        if (gm && (!gm[g] || !gLq[g])) return -1;
        G.batch[g] = (int)batch[g];
        G.blk0[g] = (int)off;
        off += elems ? cdiv64(batch[g] * M * M, 256) : batch[g] * per_batch_blocks_or_elems;
        if (off > 2000000000LL) return -1;
    }
    G.blk0[ngroups] = (int)off;
    return 0;
}

template <typename T>
static int dsvi_obj_fwd_impl(const T* y, const T* mu, const T* v, const T* noise, int64_t S, int64_t n, T ell_scale,
                             int ngroups, const void* const* m, const void* const* Lq, const int64_t* batch, int64_t M,
                             T kl_scale, T* out, void* ws, size_t wsb, void* stream) {
    if (!y) return -1; if (!mu) return -2; if (!v) return -3; if (!noise) return -4;
    if (S < 1 || S > 65535) return -5; if (n < 1) return -6;
    if (ngroups < 0 || ngroups > OBJ_MAX_GROUPS) return -8; if (ngroups > 0 && (!m || !Lq || !batch)) return -9;
    if (M < 0) return -12; if (!out) return -14;
    const int64_t nblk_e = gauss_blocks(n), nblk_k = kl_blocks(M);
    ObjGroups<T> G{};
    if (obj_groups<T>(G, ngroups, m, Lq, nullptr, nullptr, batch, nblk_k, false, M)) return -9;
    const int64_t n_ell = S * nblk_e, n_all = n_ell + G.blk0[ngroups];
    if (!ws || wsb < (size_t)n_all * sizeof(T)) return -15;
    int64_t tot_b = 0;
    for (int g = 0; g < ngroups; ++g) tot_b += batch[g];
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((dsvi_obj_part_kernel<T>), dim3((unsigned)n_all), dim3(256), 0, st, y, mu, v, noise, n, (int)nblk_e,
                       (int)n_ell, G, M, (int)nblk_k, (T*)ws);
    hipLaunchKernelGGL((dsvi_obj_final_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)ws, (int)n_ell, (int)n_all, ell_scale,
                       kl_scale, T(0.5) * T(M) * T(tot_b), out);
    return nsgp_launch_status();
}

template <typename T>
static int dsvi_obj_bwd_impl(const T* y, const T* mu, const T* v, const T* noise, int64_t S, int64_t n, T ell_scale,
                             int ngroups, const void* const* m, const void* const* Lq, const int64_t* batch, int64_t M,
                             T kl_scale, const T* gout, T* gmu, T* gv, T* gnoise, void* const* gm, void* const* gLq, void* ws,
                             size_t wsb, void* stream) {
    if (!y) return -1; if (!mu) return -2; if (!v) return -3; if (!noise) return -4;
    if (S < 1 || S > 65535) return -5; if (n < 1) return -6;
    if (ngroups < 0 || ngroups > OBJ_MAX_GROUPS) return -8; if (ngroups > 0 && (!m || !Lq || !batch)) return -9;
    if (M < 0) return -12; if (!gout) return -14; if (!gmu) return -15; if (!gv) return -16;
    if (ngroups > 0 && (!gm || !gLq)) return -18;
    const int64_t nblk_e = gauss_blocks(n);
    ObjGroups<T> G{};
    if (obj_groups<T>(G, ngroups, m, Lq, gm, gLq, batch, 0, true, M)) return -9;
    const int64_t nb_e = cdiv64(S * n, 256), nb_kl = G.blk0[ngroups], nb_gn = gnoise ? S * nblk_e : 0;
    if (gnoise && (!ws || wsb < (size_t)nb_gn * sizeof(T))) return -20;
    if (nb_e + nb_kl + nb_gn > 2000000000LL) return -6;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((dsvi_obj_bwd_kernel<T>), dim3((unsigned)(nb_e + nb_kl + nb_gn)), dim3(256), 0, st, y, mu, v, noise, S, n,
                       ell_scale, kl_scale, gout, (int)nb_e, G, M, (int)nb_kl, (int)nblk_e, gmu, gv, (T*)ws);
    if (gnoise)
        hipLaunchKernelGGL((dsvi_obj_gnoise_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)ws, (int)nb_gn, ell_scale, gout,
                           gnoise);
    return nsgp_launch_status();
}

// ---- mean-field q(u) = N(m, diag(s^2)): column statistics, their adjoint and the KL term -------------------------------
// There is no C = Lq^T A: var_j = base + base_add + sum_k (s_k^2 - 1) A_kj^2 is one pass over A.  The sum is taken in
// float64 whatever A's type is (its terms have both signs once q(u) has trained) and meets base in float64.
constexpr int DIAG_ROWS = 32;            // rows of A per partial (nsgp_svgp_diag_tiles)
constexpr int DIAG_BWD_COLS = 4096;      // columns of A per workgroup of the backward pass

// part[b,t,j] = sum_{k in tile t} s2m1[b,k] A[b,k,j]^2.  grid (column groups, T, batch); a lane owns V columns, a
// workgroup DIAG_ROWS rows (tiles past the last row write zeros: every row of the buffer is written).
template <typename T, int V>
__global__ __launch_bounds__(256) void diag_colsq_kernel(const T* __restrict__ A, const T* __restrict__ s2m1, int64_t M,
                                                         int64_t n, double* __restrict__ part) {
    const int64_t b = blockIdx.z, t = blockIdx.y;
    const int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    if (j >= n) return;                                  // (V > 1: n % V == 0, so j + V <= n)
    const int64_t k0 = t * DIAG_ROWS, k1 = (k0 + DIAG_ROWS) < M ? (k0 + DIAG_ROWS) : M;
    const T* Ab = A + b * M * n + j;
    const T* sb = s2m1 + b * M;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
#pragma unroll 8
    for (int64_t k = k0; k < k1; ++k) {
        T a[V];
        ld_vec<T, V>(Ab + k * n, a);
        const double s = (double)sb[k];
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = __builtin_fma(s * (double)a[v], (double)a[v], acc[v]);
    }
    double* out = part + (b * gridDim.y + t) * n + j;
#pragma unroll
    for (int v = 0; v < V; ++v) out[v] = acc[v];
}

// mean as colstats_finalize_kernel (same order, same type); var = (base + base_add + sum_t part_q) in float64, rounded once
template <typename T>
__global__ void colstats_finalize_diag_kernel(const T* __restrict__ pdot, int64_t tiles, const double* __restrict__ pq,
                                              int64_t qtiles, const T* __restrict__ base, T base_add, int64_t batch,
                                              int64_t n, const T* __restrict__ x, int64_t sxb, int D,
                                              const T* __restrict__ w, int64_t swb, const T* __restrict__ c, int64_t scb,
                                              T* __restrict__ mean, T* __restrict__ var) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= batch * n) return;
    const int64_t b = idx / n, j = idx % n;
    T sm[1]; double q[1];
    tile_sums({pdot}, b, tiles, n, j, sm);
    tile_sums({pq}, b, qtiles, n, j, q);
    add_affine_mean(sm[0], b, j, x, sxb, D, w, swb, c, scb);
    mean[idx] = sm[0];
    var[idx] = (T)(((double)base[b] + (double)base_add) + q[0]);
}

// Abar = m gmean^T + 2 diag(s2m1) A diag(gvar), and the partial row sums of A gmean and A^2 gvar over DIAG_BWD_COLS columns:
// grid (M, column chunks, batch); part[((b M + k) chunks + c) 2 + {0, 1}] in float64
template <typename T, int V>
__global__ __launch_bounds__(256) void diag_bwd_kernel(const T* __restrict__ A, const T* __restrict__ m,
                                                       const T* __restrict__ s2m1, const T* __restrict__ gmean,
                                                       const T* __restrict__ gvar, int64_t M, int64_t n,
                                                       T* __restrict__ Abar, double* __restrict__ part) {
    __shared__ double lds[4];
    const int64_t k = blockIdx.x, c = blockIdx.y, b = blockIdx.z;
    const int64_t row = (b * M + k) * n;
    const T mk = m[b * M + k], s2 = T(2) * s2m1[b * M + k];
    const T* gm = gmean + b * n;
    const T* gv = gvar + b * n;
    const int64_t j0 = c * DIAG_BWD_COLS, j1 = (j0 + DIAG_BWD_COLS) < n ? (j0 + DIAG_BWD_COLS) : n;
    T am = T(0), at = T(0);
#pragma unroll 4
    for (int64_t j = j0 + (int64_t)threadIdx.x * V; j < j1; j += 256 * V) {
        T a[V], g1[V], g2[V], o[V];
        ld_vec<T, V>(A + row + j, a);
        ld_vec<T, V>(gm + j, g1);
        ld_vec<T, V>(gv + j, g2);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const T ag = a[v] * g2[v];
            o[v] = mk * g1[v] + s2 * ag;
            am += a[v] * g1[v];
            at += a[v] * ag;
        }
        st_vec<T, V>(Abar + row + j, o);
    }
    const double sm = block_sum_256((double)am, lds);
    const double st = block_sum_256((double)at, lds);
    if (threadIdx.x == 0) {
        double* p = part + ((b * M + k) * gridDim.y + c) * 2;
        p[0] = sm; p[1] = st;
    }
}

template <typename T>
__global__ void diag_bwd_final_kernel(const double* __restrict__ part, int64_t rows, int64_t chunks, T* __restrict__ mbar,
                                      T* __restrict__ tbar) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double sm = 0.0, st = 0.0;
    for (int64_t c = 0; c < chunks; ++c) { sm += part[(r * chunks + c) * 2]; st += part[(r * chunks + c) * 2 + 1]; }
    mbar[r] = (T)sm;
    tbar[r] = (T)st;
}

// part[blk] = sum over a strided share of the batch * M elements of (s2 - 1) - log s2 + m^2  (twice the KL)
template <typename T>
__global__ __launch_bounds__(256) void kl_diag_part_kernel(const T* __restrict__ m, const T* __restrict__ s2, int64_t tot,
                                                           T* __restrict__ part) {
    __shared__ T lds[4];
    T acc = T(0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (int64_t)gridDim.x * 256) {
        const T v = s2[i], mm = m[i];
        acc += ((v - T(1)) - t_log(v)) + mm * mm;
    }
    acc = block_sum_256(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// out[0] = (addin ? addin[0] : 0) + scale * sum(part): the scaled term is rounded on its own (no contraction into the
// addition), so that chaining onto a running scalar adds exactly the value the un-chained call returns
template <typename T>
__global__ __launch_bounds__(256) void kl_diag_final_kernel(const T* __restrict__ part, int64_t nparts, T scale,
                                                            const T* __restrict__ addin, T* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ T lds[4];
    const T s = part_sum(part, (int64_t)0, nparts, lds);
    if (threadIdx.x == 0) {
        const T r = scale * s;
        out[0] = addin ? addin[0] + r : r;
    }
}

template <typename T>
__global__ void kl_diag_bwd_kernel(const T* __restrict__ m, const T* __restrict__ s2, int64_t tot, T scale,
                                   const T* __restrict__ gout, T* __restrict__ gm, T* __restrict__ gs2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= tot) return;
    const T go = scale * gout[0];
    gm[i] = go * m[i];
    gs2[i] = T(0.5) * go * (T(1) - T(1) / s2[i]);
}

template <typename T> static bool vec_ok(const void* p) { return ((uintptr_t)p % 16) == 0; }

template <typename T>
static int diag_colsq_impl(const T* A, const T* s2m1, int64_t batch, int64_t M, int64_t n, double* part, int64_t Tq,
                           void* stream) {
    if (!A) return -1; if (!s2m1) return -2; if (batch < 0 || batch > 65535) return -3; if (M < 0) return -4;
    if (n < 0) return -5; if (!part) return -6; if (Tq < cdiv64(M, DIAG_ROWS) || Tq > 65535) return -7;
    if (batch == 0 || M == 0 || n == 0) return 0;
    constexpr int V = 16 / sizeof(T);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = n % V == 0 && vec_ok<T>(A);
    const int64_t groups = cdiv64(n, 256 * (vec ? V : 1));
    if (groups > 2147483647LL) return -5;
    const dim3 grid((unsigned)groups, (unsigned)Tq, (unsigned)batch);
    if (vec) hipLaunchKernelGGL((diag_colsq_kernel<T, V>), grid, dim3(256), 0, st, A, s2m1, M, n, part);
    else hipLaunchKernelGGL((diag_colsq_kernel<T, 1>), grid, dim3(256), 0, st, A, s2m1, M, n, part);
    return nsgp_launch_status();
}

// the argument checks that the finalize forms with an affine prior mean share (every form numbers them alike)
template <typename T>
static int affine_args_status(const T* x, int64_t sxb, int64_t D, const T* w, int64_t swb, int64_t scb, const T* mean,
                              const T* var) {
    if (w && !x) return -9; if (sxb < 0) return -10; if (D < 0 || D > NSGP_MAX_DIM || (w && D == 0)) return -11;
    if (swb < 0) return -13; if (scb < 0) return -15; if (!mean) return -16; if (!var) return -17;
    return 0;
}

template <typename T>
static int finalize_diag_impl(const T* part_dot, int64_t tiles, const double* part_q, int64_t qtiles, const T* base,
                              T base_add, int64_t batch, int64_t n, const T* x, int64_t sxb, int64_t D, const T* w,
                              int64_t swb, const T* c, int64_t scb, T* mean, T* var, void* stream) {
    if (!part_dot) return -1; if (tiles < 0) return -2; if (!part_q) return -3; if (qtiles < 0) return -4;
    if (!base) return -5; if (batch < 0) return -7; if (n < 0) return -8;
    if (const int rc = affine_args_status(x, sxb, D, w, swb, scb, mean, var)) return rc;
    if (batch * n == 0) return 0;
    if (cdiv64(batch * n, 256) > 2147483647LL) return -8;
    hipLaunchKernelGGL((colstats_finalize_diag_kernel<T>), dim3((unsigned)cdiv64(batch * n, 256)), dim3(256), 0,
                       (hipStream_t)stream, part_dot, tiles, part_q, qtiles, base, base_add, batch, n, x, sxb, (int)D, w,
                       swb, c, scb, mean, var);
    return nsgp_launch_status();
}

static inline size_t diag_bwd_ws(int64_t batch, int64_t M, int64_t n) {
    if (batch <= 0 || M <= 0 || n <= 0) return 0;
    return (size_t)(batch * M * cdiv64(n, DIAG_BWD_COLS)) * 2 * sizeof(double);
}

template <typename T>
static int diag_bwd_impl(const T* A, const T* m, const T* s2m1, const T* gmean, const T* gvar, int64_t batch, int64_t M,
                         int64_t n, T* Abar, T* mbar, T* tbar, void* ws, size_t wsb, void* stream) {
    if (!A) return -1; if (!m) return -2; if (!s2m1) return -3; if (!gmean) return -4; if (!gvar) return -5;
    if (batch < 0 || batch > 65535) return -6; if (M < 0 || M > 2147483647LL) return -7; if (n < 0) return -8;
    if (!Abar) return -9; if (!mbar) return -10; if (!tbar) return -11;
    if (batch == 0 || M == 0 || n == 0) return 0;
    const int64_t chunks = cdiv64(n, DIAG_BWD_COLS);
    if (chunks > 65535) return -8;
    if (!ws || ((uintptr_t)ws % 8) != 0) return -12; if (wsb < diag_bwd_ws(batch, M, n)) return -13;
    constexpr int V = 16 / sizeof(T);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)M, (unsigned)chunks, (unsigned)batch);
    if (n % V == 0 && vec_ok<T>(A) && vec_ok<T>(Abar) && vec_ok<T>(gmean) && vec_ok<T>(gvar))
        hipLaunchKernelGGL((diag_bwd_kernel<T, V>), grid, dim3(256), 0, st, A, m, s2m1, gmean, gvar, M, n, Abar, (double*)ws);
    else
        hipLaunchKernelGGL((diag_bwd_kernel<T, 1>), grid, dim3(256), 0, st, A, m, s2m1, gmean, gvar, M, n, Abar, (double*)ws);
    hipLaunchKernelGGL((diag_bwd_final_kernel<T>), dim3((unsigned)cdiv64(batch * M, 256)), dim3(256), 0, st,
                       (const double*)ws, batch * M, chunks, mbar, tbar);
    return nsgp_launch_status();
}

template <typename T>
static int kl_diag_fwd_impl(const T* m, const T* s2, int64_t batch, int64_t M, T scale, const T* addin, T* out, void* ws,
                            size_t wsb, void* stream) {
    if (!m) return -1; if (!s2) return -2; if (batch < 0) return -3; if (M < 0) return -4; if (!out) return -7;
    if (batch == 0 || M == 0) return 0;
    const int64_t nblk = kl_diag_blocks(batch * M);
    if (!ws) return -8; if (wsb < (size_t)nblk * sizeof(T)) return -9;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL((kl_diag_part_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, st, m, s2, batch * M, (T*)ws);
    hipLaunchKernelGGL((kl_diag_final_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)ws, nblk, T(0.5) * scale, addin, out);
    return nsgp_launch_status();
}

template <typename T>
static int kl_diag_bwd_impl(const T* m, const T* s2, int64_t batch, int64_t M, T scale, const T* gout, T* gm, T* gs2,
                            void* stream) {
    if (!m) return -1; if (!s2) return -2; if (batch < 0) return -3; if (M < 0) return -4; if (!gout) return -6;
    if (!gm) return -7; if (!gs2) return -8;
    const int64_t tot = batch * M;
    if (tot == 0) return 0;
    if (cdiv64(tot, 256) > 2147483647LL) return -4;
    hipLaunchKernelGGL((kl_diag_bwd_kernel<T>), dim3((unsigned)cdiv64(tot, 256)), dim3(256), 0, (hipStream_t)stream, m, s2,
                       tot, scale, gout, gm, gs2);
    return nsgp_launch_status();
}

}  // namespace

template <typename T, typename TP = T>
static int finalize_affine_impl(const TP* part_dot, const TP* part_sq_a, const TP* part_sq_c, const T* base, T base_add,
                                int64_t batch, int64_t tiles, int64_t n, const T* x, int64_t sxb, int64_t D, const T* w,
                                int64_t swb, const T* c, int64_t scb, T* mean, T* var, void* stream) {
    if (!part_dot) return -1; if (!part_sq_a) return -2; if (!part_sq_c) return -3; if (!base) return -4;
    if (batch < 0) return -6; if (tiles < 0) return -7; if (n < 0) return -8;
    if (const int rc = affine_args_status(x, sxb, D, w, swb, scb, mean, var)) return rc;
    if (batch * n == 0) return 0;
    hipLaunchKernelGGL((colstats_finalize_kernel<T, TP>), dim3((unsigned)cdiv64(batch * n, 256)), dim3(256), 0,
                       (hipStream_t)stream, part_dot, part_sq_a, part_sq_c, base, base_add, batch, tiles, n, x, sxb,
                       (int)D, w, swb, c, scb, mean, var);
    return nsgp_launch_status();
}

// the plain form: its own argument numbering, then the affine form without a prior mean
template <typename T>
static int finalize_plain_impl(const T* part_dot, const T* part_sq_a, const T* part_sq_c, const T* base, int64_t batch,
                               int64_t tiles, int64_t n, T* mean, T* var, void* stream) {
    if (!part_dot) return -1; if (!part_sq_a) return -2; if (!part_sq_c) return -3; if (!base) return -4;
    if (batch < 0) return -5; if (tiles < 0) return -6; if (n < 0) return -7; if (!mean) return -8; if (!var) return -9;
    return finalize_affine_impl<T, T>(part_dot, part_sq_a, part_sq_c, base, T(0), batch, tiles, n, nullptr, 0, 0, nullptr, 0,
                                      nullptr, 0, mean, var, stream);
}

template <typename T>
static int rowdot_impl(const T* A, const T* g, int64_t batch, int64_t M, int64_t n, T* out, void* stream) {
    if (!A) return -1; if (!g) return -2; if (batch < 0) return -3; if (M < 0) return -4; if (n < 0) return -5; if (!out) return -6;
    if (batch * M == 0) return 0;
    hipLaunchKernelGGL((rowdot_kernel<T>), dim3((unsigned)M, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, A, g, M, n, out);
    return nsgp_launch_status();
}

template <typename T>
static int rowdot_affine_impl(const T* A, const T* g, const T* gv, const T* x, int64_t sxb, int64_t D, int shared,
                              int64_t batch, int64_t M, int64_t n, T* out, T* out_gv, T* out_x, T* out_1,
                              void* stream) {
    if (!A) return -1; if (!g) return -2; if (sxb < 0) return -5; if (D < 0 || D > NSGP_MAX_DIM) return -6;
    if (batch < 0) return -8; if (M < 0) return -9; if (n < 0) return -10; if (!out) return -11;
    if (gv && !out_gv) return -12; if (out_x && (!x || D == 0)) return -13;
    if (batch == 0) return 0;
    const int64_t rows = M + 2 + (out_x ? D : 0);
    if (rows > 2147483647LL || batch > 65535) return -9;
    hipLaunchKernelGGL((rowdot_affine_kernel<T>), dim3((unsigned)rows, (unsigned)batch), dim3(256), 0,
                       (hipStream_t)stream, A, g, gv, x, sxb, (int)D, shared, batch, M, n, out, out_gv, out_x, out_1);
    return nsgp_launch_status();
}

extern "C" {

size_t nsgp_reduce_workspace(int64_t n_elems, int elem_size) {
    (void)n_elems;
    return (size_t)65536 * elem_size;       // covers RED_BLOCKS partials and 256 x batch(<=256) KL partials
}

int nsgp_svgp_colstats_f32(const float* A, const float* C, const float* m, const float* base, int64_t batch,
                           int64_t M, int64_t n, float* mean, float* var, void* stream) {
    return colstats_impl<float>(A, C, m, base, batch, M, n, mean, var, stream);
}
int nsgp_svgp_colstats_f64(const double* A, const double* C, const double* m, const double* base, int64_t batch,
                           int64_t M, int64_t n, double* mean, double* var, void* stream) {
    return colstats_impl<double>(A, C, m, base, batch, M, n, mean, var, stream);
}
int nsgp_svgp_colstats_bwd_f32(const float* A, const float* C, const float* m, const float* gmean,
                               const float* gvar, int64_t batch, int64_t M, int64_t n, float* Abar, float* C2,
                               float* mbar, void* stream) {
    return colstats_bwd_impl<float>(A, C, m, gmean, gvar, batch, M, n, Abar, C2, mbar, stream);
}
int nsgp_svgp_colstats_bwd_f64(const double* A, const double* C, const double* m, const double* gmean,
                               const double* gvar, int64_t batch, int64_t M, int64_t n, double* Abar, double* C2,
                               double* mbar, void* stream) {
    return colstats_bwd_impl<double>(A, C, m, gmean, gvar, batch, M, n, Abar, C2, mbar, stream);
}
int nsgp_dgp_sample_fwd_f32(const float* mean, const float* var, const float* eps, int64_t S, int64_t ns, int64_t n,
                            int64_t b, float* h, void* stream) {
    return sample_fwd_impl<float>(mean, var, eps, S, ns, n, b, h, stream);
}
int nsgp_dgp_sample_bwd_f32(const float* var, const float* eps, const float* gh, int64_t S, int64_t ns, int64_t n,
                            int64_t b, float* gmean, float* gvar, void* stream) {
    return sample_bwd_impl<float>(var, eps, gh, S, ns, n, b, gmean, gvar, stream);
}
int nsgp_dgp_sample_fwd_f64(const double* mean, const double* var, const double* eps, int64_t S, int64_t ns,
                            int64_t n, int64_t b, double* h, void* stream) {
    return sample_fwd_impl<double>(mean, var, eps, S, ns, n, b, h, stream);
}
int nsgp_dgp_sample_bwd_f64(const double* var, const double* eps, const double* gh, int64_t S, int64_t ns, int64_t n,
                            int64_t b, double* gmean, double* gvar, void* stream) {
    return sample_bwd_impl<double>(var, eps, gh, S, ns, n, b, gmean, gvar, stream);
}
int nsgp_gauss_ell_fwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S, int64_t n,
                           float scale, float* out, void* ws, size_t wsb, void* stream) {
    return gauss_fwd_impl<float>(y, mu, v, noise, S, n, scale, out, ws, wsb, stream);
}
int nsgp_gauss_ell_bwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S, int64_t n,
                           float scale, const float* gout, float* gmu, float* gv, float* gnoise, void* ws,
                           size_t wsb, void* stream) {
    return gauss_bwd_impl<float>(y, mu, v, noise, S, n, scale, gout, gmu, gv, gnoise, ws, wsb, stream);
}
int nsgp_gauss_ell_fwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S,
                           int64_t n, double scale, double* out, void* ws, size_t wsb, void* stream) {
    return gauss_fwd_impl<double>(y, mu, v, noise, S, n, scale, out, ws, wsb, stream);
}
int nsgp_gauss_ell_bwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S,
                           int64_t n, double scale, const double* gout, double* gmu, double* gv, double* gnoise,
                           void* ws, size_t wsb, void* stream) {
    return gauss_bwd_impl<double>(y, mu, v, noise, S, n, scale, gout, gmu, gv, gnoise, ws, wsb, stream);
}
int nsgp_kl_whitened_fwd_f32(const float* m, const float* Lq, int64_t batch, int64_t M, float* out, void* ws,
                             size_t wsb, void* stream) {
    return kl_fwd_impl<float>(m, Lq, batch, M, out, ws, wsb, stream);
}
int nsgp_kl_whitened_bwd_f32(const float* m, const float* Lq, int64_t batch, int64_t M, float gout, float* gm,
                             float* gLq, void* stream) {
    return kl_bwd_impl<float>(m, Lq, batch, M, gout, gm, gLq, stream);
}
int nsgp_kl_whitened_fwd_f64(const double* m, const double* Lq, int64_t batch, int64_t M, double* out, void* ws,
                             size_t wsb, void* stream) {
    return kl_fwd_impl<double>(m, Lq, batch, M, out, ws, wsb, stream);
}
int nsgp_kl_whitened_bwd_f64(const double* m, const double* Lq, int64_t batch, int64_t M, double gout, double* gm,
                             double* gLq, void* stream) {
    return kl_bwd_impl<double>(m, Lq, batch, M, gout, gm, gLq, stream);
}

int nsgp_svgp_colstats_finalize_f32(const float* part_dot, const float* part_sq_a, const float* part_sq_c,
                                    const float* base, int64_t batch, int64_t tiles, int64_t n, float* mean,
                                    float* var, void* stream) {
    return finalize_plain_impl<float>(part_dot, part_sq_a, part_sq_c, base, batch, tiles, n, mean, var, stream);
}
int nsgp_svgp_colstats_finalize_f64(const double* part_dot, const double* part_sq_a, const double* part_sq_c,
                                    const double* base, int64_t batch, int64_t tiles, int64_t n, double* mean,
                                    double* var, void* stream) {
    return finalize_plain_impl<double>(part_dot, part_sq_a, part_sq_c, base, batch, tiles, n, mean, var, stream);
}
int nsgp_svgp_colstats_finalize_affine_f32(const float* part_dot, const float* part_sq_a, const float* part_sq_c,
                                           const float* base, float base_add, int64_t batch, int64_t tiles, int64_t n,
                                           const float* x, int64_t x_batch_stride, int64_t D, const float* w,
                                           int64_t w_batch_stride, const float* c, int64_t c_batch_stride, float* mean,
                                           float* var, void* stream) {
    return finalize_affine_impl<float>(part_dot, part_sq_a, part_sq_c, base, base_add, batch, tiles, n, x, x_batch_stride,
                                       D, w, w_batch_stride, c, c_batch_stride, mean, var, stream);
}
int nsgp_svgp_colstats_finalize_affine_p64_f32(const double* part_dot, const double* part_sq_a, const double* part_sq_c,
                                               const float* base, float base_add, int64_t batch, int64_t tiles, int64_t n,
                                               const float* x, int64_t x_batch_stride, int64_t D, const float* w,
                                               int64_t w_batch_stride, const float* c, int64_t c_batch_stride, float* mean,
                                               float* var, void* stream) {
    return finalize_affine_impl<float, double>(part_dot, part_sq_a, part_sq_c, base, base_add, batch, tiles, n, x,
                                               x_batch_stride, D, w, w_batch_stride, c, c_batch_stride, mean, var, stream);
}
int nsgp_svgp_colstats_finalize_affine_f64(const double* part_dot, const double* part_sq_a, const double* part_sq_c,
                                           const double* base, double base_add, int64_t batch, int64_t tiles,
                                           int64_t n, const double* x, int64_t x_batch_stride, int64_t D,
                                           const double* w, int64_t w_batch_stride, const double* c,
                                           int64_t c_batch_stride, double* mean, double* var, void* stream) {
    return finalize_affine_impl<double>(part_dot, part_sq_a, part_sq_c, base, base_add, batch, tiles, n, x,
                                        x_batch_stride, D, w, w_batch_stride, c, c_batch_stride, mean, var, stream);
}
int nsgp_rowdot_affine_f32(const float* A, const float* g, const float* gv, const float* x, int64_t x_batch_stride,
                           int64_t D, int shared, int64_t batch, int64_t M, int64_t n, float* out, float* out_gv,
                           float* out_x, float* out_1, void* stream) {
    return rowdot_affine_impl<float>(A, g, gv, x, x_batch_stride, D, shared, batch, M, n, out, out_gv, out_x, out_1,
                                     stream);
}
int nsgp_rowdot_affine_f64(const double* A, const double* g, const double* gv, const double* x, int64_t x_batch_stride,
                           int64_t D, int shared, int64_t batch, int64_t M, int64_t n, double* out, double* out_gv,
                           double* out_x, double* out_1, void* stream) {
    return rowdot_affine_impl<double>(A, g, gv, x, x_batch_stride, D, shared, batch, M, n, out, out_gv, out_x, out_1,
                                      stream);
}
int nsgp_rowdot_f32(const float* A, const float* g, int64_t batch, int64_t M, int64_t n, float* out, void* stream) {
    return rowdot_impl<float>(A, g, batch, M, n, out, stream);
}
int nsgp_rowdot_f64(const double* A, const double* g, int64_t batch, int64_t M, int64_t n, double* out, void* stream) {
    return rowdot_impl<double>(A, g, batch, M, n, out, stream);
}

/* mean-field q(u): column statistics, their adjoint, KL (nsgp.svgp.SVGPMeanFieldLayerFn, nsgp.ops.KlMeanFieldTotalFn) */
size_t nsgp_svgp_diag_tiles(int64_t M) { return M > 0 ? (size_t)cdiv64(M, DIAG_ROWS) : 0; }
int nsgp_svgp_diag_colsq_f32(const float* A, const float* s2m1, int64_t batch, int64_t M, int64_t n, double* part_q,
                             int64_t T, void* stream) {
    return diag_colsq_impl<float>(A, s2m1, batch, M, n, part_q, T, stream);
}
int nsgp_svgp_diag_colsq_f64(const double* A, const double* s2m1, int64_t batch, int64_t M, int64_t n, double* part_q,
                             int64_t T, void* stream) {
    return diag_colsq_impl<double>(A, s2m1, batch, M, n, part_q, T, stream);
}
int nsgp_svgp_colstats_finalize_diag_f32(const float* part_dot, int64_t tiles, const double* part_q, int64_t qtiles,
                                         const float* base, float base_add, int64_t batch, int64_t n, const float* x,
                                         int64_t x_batch_stride, int64_t D, const float* w, int64_t w_batch_stride,
                                         const float* c, int64_t c_batch_stride, float* mean, float* var, void* stream) {
    return finalize_diag_impl<float>(part_dot, tiles, part_q, qtiles, base, base_add, batch, n, x, x_batch_stride, D, w,
                                     w_batch_stride, c, c_batch_stride, mean, var, stream);
}
int nsgp_svgp_colstats_finalize_diag_f64(const double* part_dot, int64_t tiles, const double* part_q, int64_t qtiles,
                                         const double* base, double base_add, int64_t batch, int64_t n, const double* x,
                                         int64_t x_batch_stride, int64_t D, const double* w, int64_t w_batch_stride,
                                         const double* c, int64_t c_batch_stride, double* mean, double* var, void* stream) {
    return finalize_diag_impl<double>(part_dot, tiles, part_q, qtiles, base, base_add, batch, n, x, x_batch_stride, D, w,
                                      w_batch_stride, c, c_batch_stride, mean, var, stream);
}
size_t nsgp_svgp_diag_bwd_workspace(int64_t batch, int64_t M, int64_t n) { return diag_bwd_ws(batch, M, n); }
int nsgp_svgp_diag_bwd_f32(const float* A, const float* m, const float* s2m1, const float* gmean, const float* gvar,
                           int64_t batch, int64_t M, int64_t n, float* Abar, float* mbar, float* tbar, void* ws,
                           size_t ws_bytes, void* stream) {
    return diag_bwd_impl<float>(A, m, s2m1, gmean, gvar, batch, M, n, Abar, mbar, tbar, ws, ws_bytes, stream);
}
int nsgp_svgp_diag_bwd_f64(const double* A, const double* m, const double* s2m1, const double* gmean, const double* gvar,
                           int64_t batch, int64_t M, int64_t n, double* Abar, double* mbar, double* tbar, void* ws,
                           size_t ws_bytes, void* stream) {
    return diag_bwd_impl<double>(A, m, s2m1, gmean, gvar, batch, M, n, Abar, mbar, tbar, ws, ws_bytes, stream);
}
int nsgp_kl_meanfield_total_acc_fwd_f32(const float* m, const float* s2, int64_t batch, int64_t M, float scale,
                                        const float* addin, float* out, void* ws, size_t wsb, void* stream) {
    return kl_diag_fwd_impl<float>(m, s2, batch, M, scale, addin, out, ws, wsb, stream);
}
int nsgp_kl_meanfield_total_acc_fwd_f64(const double* m, const double* s2, int64_t batch, int64_t M, double scale,
                                        const double* addin, double* out, void* ws, size_t wsb, void* stream) {
    return kl_diag_fwd_impl<double>(m, s2, batch, M, scale, addin, out, ws, wsb, stream);
}
int nsgp_kl_meanfield_total_bwd_f32(const float* m, const float* s2, int64_t batch, int64_t M, float scale,
                                    const float* gout, float* gm, float* gs2, void* stream) {
    return kl_diag_bwd_impl<float>(m, s2, batch, M, scale, gout, gm, gs2, stream);
}
int nsgp_kl_meanfield_total_bwd_f64(const double* m, const double* s2, int64_t batch, int64_t M, double scale,
                                    const double* gout, double* gm, double* gs2, void* stream) {
    return kl_diag_bwd_impl<double>(m, s2, batch, M, scale, gout, gm, gs2, stream);
}

/* scalar forms used by the fused ELBO tail (nsgp.ops.GaussEllTotalFn / KlWhitenedTotalFn) */
int nsgp_gauss_ell_total_fwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S,
                                 int64_t n, float scale, float* out, void* ws, size_t wsb, void* stream) {
    return gauss_fwd_impl<float>(y, mu, v, noise, S, n, scale, out, ws, wsb, stream, true);
}
int nsgp_gauss_ell_total_fwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S,
                                 int64_t n, double scale, double* out, void* ws, size_t wsb, void* stream) {
    return gauss_fwd_impl<double>(y, mu, v, noise, S, n, scale, out, ws, wsb, stream, true);
}
int nsgp_gauss_ell_total_bwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S,
                                 int64_t n, float scale, const float* gout, float* gmu, float* gv, float* gnoise,
                                 void* ws, size_t wsb, void* stream) {
    return gauss_bwd_impl<float>(y, mu, v, noise, S, n, scale, gout, gmu, gv, gnoise, ws, wsb, stream, true);
}
int nsgp_gauss_ell_total_bwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S,
                                 int64_t n, double scale, const double* gout, double* gmu, double* gv, double* gnoise,
                                 void* ws, size_t wsb, void* stream) {
    return gauss_bwd_impl<double>(y, mu, v, noise, S, n, scale, gout, gmu, gv, gnoise, ws, wsb, stream, true);
}
int nsgp_kl_whitened_total_acc_fwd_f32(const float* m, const float* Lq, int64_t batch, int64_t M, float scale,
                                       const float* addin, float* out, void* ws, size_t wsb, void* stream) {
    if (batch == 0) return addin ? -3 : 0;               // nothing would write out = addin
    return kl_fwd_impl<float>(m, Lq, batch, M, out, ws, wsb, stream, true, scale, addin);
}
int nsgp_kl_whitened_total_acc_fwd_f64(const double* m, const double* Lq, int64_t batch, int64_t M, double scale,
                                       const double* addin, double* out, void* ws, size_t wsb, void* stream) {
    if (batch == 0) return addin ? -3 : 0;
    return kl_fwd_impl<double>(m, Lq, batch, M, out, ws, wsb, stream, true, scale, addin);
}
int nsgp_kl_whitened_total_bwd_f32(const float* m, const float* Lq, int64_t batch, int64_t M, float scale,
                                   const float* gout, float* gm, float* gLq, void* stream) {
    if (!gout) return -6;
    return kl_bwd_impl<float>(m, Lq, batch, M, scale, gm, gLq, stream, gout);
}
int nsgp_kl_whitened_total_bwd_f64(const double* m, const double* Lq, int64_t batch, int64_t M, double scale,
                                   const double* gout, double* gm, double* gLq, void* stream) {
    if (!gout) return -6;
    return kl_bwd_impl<double>(m, Lq, batch, M, scale, gm, gLq, stream, gout);
}

/* Gauss-Hermite log marginal of a Bernoulli (kind 0) or Student-t (kind 1) likelihood (nsgp.ops.gh_log_marginal) */
int nsgp_gh_log_marginal_f32(int kind, const float* y, const float* mu, const float* v, const float* params,
                             const float* nodes, const float* weights, int64_t Q, int64_t S, int64_t n, float* out,
                             void* stream) {
    return gh_log_marginal_impl<float>(kind, y, mu, v, params, nodes, weights, Q, S, n, out, stream);
}
int nsgp_gh_log_marginal_f64(int kind, const double* y, const double* mu, const double* v, const double* params,
                             const double* nodes, const double* weights, int64_t Q, int64_t S, int64_t n, double* out,
                             void* stream) {
    return gh_log_marginal_impl<double>(kind, y, mu, v, params, nodes, weights, Q, S, n, out, stream);
}

size_t nsgp_dsvi_objective_workspace(int64_t S, int64_t n, int64_t M, int64_t total_batch, int elem_size) {
    if (S < 1 || n < 1) return 0;
    return (size_t)(S * gauss_blocks(n) + (M > 0 ? total_batch * kl_blocks(M) : 0)) * (size_t)elem_size;
}
int nsgp_dsvi_objective_fwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S, int64_t n,
                                float ell_scale, int ngroups, const void* const* m, const void* const* Lq,
                                const int64_t* batch, int64_t M, float kl_scale, float* out, void* ws, size_t wsb,
                                void* stream) {
    return dsvi_obj_fwd_impl<float>(y, mu, v, noise, S, n, ell_scale, ngroups, m, Lq, batch, M, kl_scale, out, ws, wsb, stream);
}
int nsgp_dsvi_objective_fwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S, int64_t n,
                                double ell_scale, int ngroups, const void* const* m, const void* const* Lq,
                                const int64_t* batch, int64_t M, double kl_scale, double* out, void* ws, size_t wsb,
                                void* stream) {
    return dsvi_obj_fwd_impl<double>(y, mu, v, noise, S, n, ell_scale, ngroups, m, Lq, batch, M, kl_scale, out, ws, wsb, stream);
}
int nsgp_dsvi_objective_bwd_f32(const float* y, const float* mu, const float* v, const float* noise, int64_t S, int64_t n,
                                float ell_scale, int ngroups, const void* const* m, const void* const* Lq,
                                const int64_t* batch, int64_t M, float kl_scale, const float* gout, float* gmu, float* gv,
                                float* gnoise, void* const* gm, void* const* gLq, void* ws, size_t wsb, void* stream) {
    return dsvi_obj_bwd_impl<float>(y, mu, v, noise, S, n, ell_scale, ngroups, m, Lq, batch, M, kl_scale, gout, gmu, gv, gnoise,
                                    gm, gLq, ws, wsb, stream);
}
int nsgp_dsvi_objective_bwd_f64(const double* y, const double* mu, const double* v, const double* noise, int64_t S, int64_t n,
                                double ell_scale, int ngroups, const void* const* m, const void* const* Lq,
                                const int64_t* batch, int64_t M, double kl_scale, const double* gout, double* gmu, double* gv,
                                double* gnoise, void* const* gm, void* const* gLq, void* ws, size_t wsb, void* stream) {
    return dsvi_obj_bwd_impl<double>(y, mu, v, noise, S, n, ell_scale, ngroups, m, Lq, batch, M, kl_scale, gout, gmu, gv, gnoise,
                                     gm, gLq, ws, wsb, stream);
}

}  // extern "C"
