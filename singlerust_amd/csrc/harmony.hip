// harmony.hip — Harmony batch integration of dense f64 points (the PCA scores a fit left in HBM, or points the caller
// supplies): srx_harmony_result / srx_harmony_points, the srx_harmony handle, and the two k-NN entries that read its
// corrected block.  The definition is in include/srx.h; all arithmetic is f64 and no kernel uses a floating-point atomic.
//
//   k_hm_cosine      (thread per cell) Zhat_i = X_i / |X_i|, the norm summed in coordinate order; finiteness of the input
//   k_hm_gather      the K start rows of Zhat -> Y
//   k_hm_blocks      q_i = H(1 + t, i) mod n_blocks
//   k_hm_assign<M>   one wave per cell, lane l owns clusters l, l + 64, ..: the K dot products against Y (in LDS when it
//                    fits, else read through the caches), then  M = kHard: the one-hot row of the spherical k-means;
//                    kSoft: the softmax row of R, with the ratio table of the cell's batch when a block is updated;
//                    kObjective: the cell's terms of the objective, summed per lane, one slot per wave
//   k_hm_tables      grouped sums T[k][b] of R over the cells of a chunk (and of one block q): thread k owns column k of a
//                    table in LDS and walks the chunk's cells in order; one partial table per chunk
//   k_hm_fold        the partial tables added in chunk order (runs of chunks, then the runs), and what the step does
//                    with the sum: set O and E, take a block's rows out and make the ratio table, add the new rows back,
//                    or store m for the correction
//   k_hm_gemm_t      partial[chunk] = R[rows]^T X[rows] (K x d) for a chunk of (optionally permuted) rows: 32 rows at a
//                    time in LDS, each thread up to 8 of the 16 x d outputs of its cluster tile, rows in order
//   k_hm_centroids   the partials added in chunk order, Y_k = s_k / |s_k| (kept when s_k = 0)
//   k_hm_ridge       the same sum per batch (S_kb), then w0_k and W_kb of the closed-form ridge correction
//   k_hm_correct     one wave per cell: Z_corr_i = Z_i - sum_k R_ik W[b_i][k]
// Every sum over cells is a chain over a contiguous chunk followed by chains over the chunks; chunk and run sizes depend on
// (n, d, K, B) alone, so the result is bit-identical from call to call.
#include "common.hpp"
#include "hash.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

struct srx_harmony {
    srx_ctx* ctx = nullptr;
    uint64_t n = 0;
    uint32_t d = 0, K = 0, B = 0;
    void* d_block = nullptr;             // one allocation: Z_corr | R | Y | O | E
    double *d_zc = nullptr, *d_r = nullptr, *d_y = nullptr, *d_o = nullptr, *d_e = nullptr;
    srx_harmony_info info{};
};

namespace srx {

int32_t knn_self_device(srx_ctx* ctx, const double* d_pts, uint64_t n, uint64_t d_full, size_t ld, const srx_knn_opts* opts,
                        uint32_t* indices_out, double* distances_out, srx_knn_info* info, const uint32_t** d_idx,
                        const double** d_dist, uint64_t* n_out);                                                   // knn.hip
int32_t graph_from_device_list(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k,
                               srx_graph** out);                                                                  // graph.hip
int32_t bbknn_device(srx_ctx* ctx, const double* d_pts, const double* h_pts, size_t ld, uint64_t n, uint64_t d_full, const uint32_t* batch,
                     uint32_t B, const srx_bbknn_opts* opts, uint32_t* indices_out, double* distances_out, srx_bbknn_info* info_out,
                     srx_graph** out);                                                                            // bbknn.hip

constexpr int kHmKT = 16;                // clusters per tile of k_hm_gemm_t
constexpr int kHmRows = 32;              // rows staged per step of k_hm_gemm_t
constexpr int kHmBT = 16;                // batches per pass of k_hm_tables (a 16 x 256 table of doubles in LDS)
constexpr size_t kHmYLds = 120 * 1024;   // Y goes to LDS up to this size (padded rows)
constexpr uint32_t kHmMaxBlocks = 65536;
enum { kHard = 0, kSoft = 1, kObjective = 2 };
enum { kFoldInit = 0, kFoldOut = 1, kFoldIn = 2, kFoldM = 3 };

__host__ __device__ __forceinline__ uint64_t hm_hash(uint64_t seed, uint64_t a, uint64_t i) {
    return mix64(seed + kGold64 * (1ull + (a << 32) + i));
}

__global__ void __launch_bounds__(256) k_hm_cosine(const double* __restrict__ x, size_t ld, uint64_t n, int d,
                                                   double* __restrict__ zh, int* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double* r = x + i * ld;
    double s = 0.0;
    bool nf = false;
    for (int c = 0; c < d; ++c) {
        const double v = r[c];
        nf |= !is_finite(v);
        s += v * v;
    }
    if (nf && bad) *bad = 1;
    const double nrm = sqrt(s);
    for (int c = 0; c < d; ++c) zh[i * d + c] = nrm > 0.0 ? r[c] / nrm : 0.0;
}

__global__ void k_hm_gather(const double* __restrict__ zh, const uint32_t* __restrict__ start, int d, double* __restrict__ y) {
    const int k = blockIdx.x, c = threadIdx.x;
    if (c < d) y[(size_t)k * d + c] = zh[(size_t)start[k] * d + c];
}

__global__ void __launch_bounds__(256) k_hm_blocks(uint64_t seed, uint64_t a, uint64_t n, uint32_t nb, uint32_t* __restrict__ q) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) q[i] = (uint32_t)(hm_hash(seed, a, i) % nb);
}

struct HmAssign {
    const double* zh;            // n x d
    const double* y;             // K x d
    const uint32_t* batch;
    const uint32_t* qarr;        // block of every cell (q >= 0)
    const double* ratio;         // B x K: theta log((E + 1) / (O + 1)), or null
    const double *o, *e;         // K x B (kObjective)
    double* r;                   // n x K
    double* part;                // one slot per wave (kObjective)
    uint64_t n;
    int d, K, B, dp, q;
    double sigma, theta;
};

template <int MODE, bool YLDS>
__global__ void __launch_bounds__(256) k_hm_assign(HmAssign a) {
    extern __shared__ __align__(16) double ys[];
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int d = a.d, K = a.K;
    if (YLDS) {
        for (int e = threadIdx.x; e < K * d; e += 256) ys[(e / d) * a.dp + e % d] = a.y[e];
        __syncthreads();
    }
    const double* yb = YLDS ? ys : a.y;
    const int ystr = YLDS ? a.dp : d;
    const int nj = (K + 63) >> 6;
    int ko[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) ko[j] = min(lane + 64 * j, K - 1) * ystr;
    const uint64_t n_groups = (a.n + 63) >> 6, stride = (uint64_t)gridDim.x * 4;
    double part = 0.0;
    for (uint64_t g = (uint64_t)blockIdx.x * 4 + wave; g < n_groups; g += stride) {
        const uint64_t i_lane = g * 64 + lane;
        const bool mine = i_lane < a.n && (a.q < 0 || a.qarr[i_lane] == (uint32_t)a.q);
        unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
        while (m) {
            const uint64_t i = g * 64 + (uint64_t)__builtin_ctzll(m);      // wave-uniform
            m &= m - 1;
            const double* z = a.zh + i * d;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int c = 0; c < d; ++c) {
                const double zc = z[c];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nj) acc[j] += zc * yb[ko[j] + c];
            }
            double* rrow = a.r + i * K;
            if (MODE == kHard) {
                double bv = -__builtin_inf();
                int bk = 0x7FFFFFFF;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = lane + 64 * j;
                    if (k < K && acc[j] > bv) { bv = acc[j]; bk = k; }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double ov = __shfl_xor(bv, off, 64);
                    const int ok = __shfl_xor(bk, off, 64);
                    if (ov > bv || (ov == bv && ok < bk)) { bv = ov; bk = ok; }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = lane + 64 * j;
                    if (k < K) rrow[k] = k == bk ? 1.0 : 0.0;
                }
            } else if (MODE == kSoft) {
                const uint32_t b = a.batch[i];
                double lg[4], mx = -__builtin_inf();
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = lane + 64 * j;
                    lg[j] = -__builtin_inf();
                    if (k < K) {
                        lg[j] = -(2.0 * (1.0 - acc[j])) / a.sigma;
                        if (a.ratio) lg[j] += a.ratio[(size_t)b * K + k];
                        mx = fmax(mx, lg[j]);
                    }
                }
                mx = wave_max(mx);
                double s = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    lg[j] = lane + 64 * j < K ? exp(lg[j] - mx) : 0.0;
                    s += lg[j];
                }
                s = wave_sum(s);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (lane + 64 * j < K) rrow[lane + 64 * j] = lg[j] / s;
            } else {
                const uint32_t b = a.batch[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = lane + 64 * j;
                    if (k < K) {
                        const double r = rrow[k], dist = 2.0 * (1.0 - acc[j]);
                        const size_t kb = (size_t)k * a.B + b;
                        double t = r * dist;
                        if (r > 0.0) t += a.sigma * (r * log(r));
                        t += a.sigma * a.theta * (r * log((a.o[kb] + 1.0) / (a.e[kb] + 1.0)));
                        part += t;
                    }
                }
            }
        }
    }
    if (MODE == kObjective) {
        part = wave_sum(part);
        if (lane == 0) a.part[(size_t)blockIdx.x * 4 + wave] = part;
    }
}

// part: n_chunks x K x B.  Chunk p holds the cells [p * per, (p + 1) * per); q < 0: every cell, else the cells of block q.
__global__ void __launch_bounds__(256) k_hm_tables(const double* __restrict__ r, uint64_t n, int K, int B, uint64_t per,
                                                   const uint32_t* __restrict__ batch, const uint32_t* __restrict__ qarr, int q,
                                                   double* __restrict__ part) {
    __shared__ double tab[kHmBT * 256];
    __shared__ uint32_t code[256];
    const int k = threadIdx.x;
    const uint64_t i0 = per * blockIdx.x, i1 = i0 + per < n ? i0 + per : n;
    double* out = part + (size_t)blockIdx.x * K * B;
    for (int b0 = 0; b0 < B; b0 += kHmBT) {
        for (int bb = 0; bb < kHmBT; ++bb) tab[bb * 256 + k] = 0.0;
        for (uint64_t c0 = i0; c0 < i1; c0 += 256) {
            __syncthreads();
            const uint64_t i = c0 + threadIdx.x;
            uint32_t cd = 0xFFFFFFFFu;
            if (i < i1 && (q < 0 || qarr[i] == (uint32_t)q)) {
                const uint32_t b = batch[i];
                if (b >= (uint32_t)b0 && b < (uint32_t)(b0 + kHmBT)) cd = b - (uint32_t)b0;
            }
            code[threadIdx.x] = cd;
            __syncthreads();
            const int cnt = (int)(i1 - c0 < 256 ? i1 - c0 : 256);
            if (k < K)
                for (int t = 0; t < cnt; ++t) {
                    const uint32_t bb = code[t];
                    if (bb != 0xFFFFFFFFu) tab[bb * 256 + k] += r[(c0 + t) * K + k];
                }
        }
        if (k < K)
            for (int bb = 0; bb < kHmBT && b0 + bb < B; ++bb) out[(size_t)k * B + b0 + bb] = tab[bb * 256 + k];
        __syncthreads();
    }
}

// grid K, 256 threads.  bp: B rounded up to a power of two.  The 256 / bp threads of batch b each add a run of consecutive
// chunks' partials of (k, b) in chunk order, then thread b adds the runs' sums in order.
__global__ void __launch_bounds__(256) k_hm_fold(const double* __restrict__ part, int n_chunks, int K, int B, int bp,
                                                 const double* __restrict__ pb, int mode, double theta, double* __restrict__ o,
                                                 double* __restrict__ e, double* __restrict__ ratio) {
    __shared__ double seg[256];
    __shared__ double sh[256];
    const int k = blockIdx.x, b = threadIdx.x;
    {
        const int bb = threadIdx.x & (bp - 1), s = threadIdx.x / bp, runs = 256 / bp;
        const int len = (n_chunks + runs - 1) / runs, p0 = s * len, p1 = p0 + len < n_chunks ? p0 + len : n_chunks;
        double t = 0.0;
        if (bb < B)
            for (int p = p0; p < p1; ++p) t += part[((size_t)p * K + k) * B + bb];
        seg[threadIdx.x] = t;
    }
    __syncthreads();
    double t = 0.0;
    if (b < B)
        for (int s = 0; s < 256 / bp; ++s) t += seg[s * bp + b];
    sh[b] = t;
    __syncthreads();
    if (b >= B) return;
    double rs = 0.0;
    for (int c = 0; c < B; ++c) rs += sh[c];
    const size_t kb = (size_t)k * B + b;
    if (mode == kFoldM) {
        o[kb] = t;
    } else if (mode == kFoldInit) {
        o[kb] = t;
        e[kb] = rs * pb[b];
    } else if (mode == kFoldOut) {
        const double ov = o[kb] - t, ev = e[kb] - rs * pb[b];
        o[kb] = ov;
        e[kb] = ev;
        ratio[(size_t)b * K + k] = theta * log((ev + 1.0) / (ov + 1.0));
    } else {
        o[kb] += t;
        e[kb] += rs * pb[b];
    }
}

// grid (n_chunks, ceil(K / 16)).  chunk c holds the rows perm[lo[c] .. lo[c + 1]) (perm null: the rows themselves, and
// lo null: lo[c] = c * per clipped to n).
__global__ void __launch_bounds__(256) k_hm_gemm_t(const double* __restrict__ r, int K, const double* __restrict__ x, size_t ld,
                                                   int d, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ lo,
                                                   uint64_t per, uint64_t n, double* __restrict__ part) {
    __shared__ double rs[kHmRows * kHmKT];
    __shared__ double xs[kHmRows * 128];
    const uint64_t s0 = lo ? lo[blockIdx.x] : per * blockIdx.x;
    const uint64_t s1 = lo ? lo[blockIdx.x + 1] : (s0 + per < n ? s0 + per : n);
    const int k0 = blockIdx.y * kHmKT;
    const int n_out = kHmKT * d;
    int ok[8], oc[8];
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int o = (int)threadIdx.x + 256 * j;
        ok[j] = o < n_out ? o / d : 0;
        oc[j] = o < n_out ? o % d : 0;
        acc[j] = 0.0;
    }
    for (uint64_t c0 = s0; c0 < s1; c0 += kHmRows) {
        __syncthreads();
        for (int e = threadIdx.x; e < kHmRows * kHmKT; e += 256) {
            const int rr = e / kHmKT, kq = e % kHmKT;
            double v = 0.0;
            if (c0 + rr < s1 && k0 + kq < K) {
                const uint64_t row = perm ? perm[c0 + rr] : c0 + rr;
                v = r[row * K + k0 + kq];
            }
            rs[e] = v;
        }
        for (int e = threadIdx.x; e < kHmRows * d; e += 256) {
            const int rr = e / d, c = e % d;
            double v = 0.0;
            if (c0 + rr < s1) {
                const uint64_t row = perm ? perm[c0 + rr] : c0 + rr;
                v = x[row * ld + c];
            }
            xs[e] = v;
        }
        __syncthreads();
        for (int rr = 0; rr < kHmRows; ++rr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += rs[rr * kHmKT + ok[j]] * xs[rr * d + oc[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int o = (int)threadIdx.x + 256 * j;
        if (o < n_out && k0 + ok[j] < K) part[((size_t)blockIdx.x * K + k0 + ok[j]) * d + oc[j]] = acc[j];
    }
}

// grid K, 128 threads
__global__ void __launch_bounds__(128) k_hm_centroids(const double* __restrict__ part, int n_chunks, int K, int d,
                                                      double* __restrict__ y) {
    __shared__ double sh[128];
    const int k = blockIdx.x, c = threadIdx.x;
    double s = 0.0;
    if (c < d)
        for (int p = 0; p < n_chunks; ++p) s += part[((size_t)p * K + k) * d + c];
    sh[c] = s;
    __syncthreads();
    if (c >= d) return;
    double n2 = 0.0;
    for (int t = 0; t < d; ++t) n2 += sh[t] * sh[t];
    const double nrm = sqrt(n2);
    if (nrm > 0.0) y[(size_t)k * d + c] = s / nrm;
}

// grid K, 128 threads.  cb: B + 1 offsets into the chunks (batch b owns chunks cb[b] .. cb[b + 1]); w: B x K x d.
__global__ void __launch_bounds__(128) k_hm_ridge(const double* __restrict__ part, const uint32_t* __restrict__ cb, int K, int B,
                                                  int d, const double* __restrict__ m, double lambda, double* __restrict__ w) {
    const int k = blockIdx.x, c = threadIdx.x;
    if (c >= d) return;
    double num = 0.0, s = 0.0;
    for (int b = 0; b < B; ++b) {
        double S = 0.0;
        for (uint32_t p = cb[b]; p < cb[b + 1]; ++p) S += part[((size_t)p * K + k) * d + c];
        w[((size_t)b * K + k) * d + c] = S;
        const double mk = m[(size_t)k * B + b], den = mk + lambda;
        num += lambda * S / den;
        s += lambda * mk / den;
    }
    const double w0 = s != 0.0 ? num / s : 0.0;
    for (int b = 0; b < B; ++b) {
        const size_t at = ((size_t)b * K + k) * d + c;
        const double mk = m[(size_t)k * B + b], den = mk + lambda;
        w[at] = s != 0.0 ? (w[at] - mk * w0) / den : 0.0;
    }
}

__global__ void __launch_bounds__(256) k_hm_correct(const double* __restrict__ z, size_t ld, const double* __restrict__ r,
                                                    const double* __restrict__ w, const uint32_t* __restrict__ batch, uint64_t n,
                                                    int K, int d, double* __restrict__ zc) {
    const uint64_t i = global_wave_id();
    if (i >= n) return;
    const int lane = lane_id();
    const double* wb = w + (size_t)batch[i] * K * d;
    const double* rrow = r + i * K;
    const int c0 = lane, c1 = lane + 64;
    double a0 = 0.0, a1 = 0.0;
    for (int k = 0; k < K; ++k) {
        const double rk = rrow[k];
        if (c0 < d) a0 += rk * wb[(size_t)k * d + c0];
        if (c1 < d) a1 += rk * wb[(size_t)k * d + c1];
    }
    if (c0 < d) zc[i * d + c0] = z[i * ld + c0] - a0;
    if (c1 < d) zc[i * d + c1] = z[i * ld + c1] - a1;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct HmOpts {
    double theta, sigma, lambda, eps_cluster, eps_harmony;
    uint64_t seed;
    int K, n_blocks, max_rounds, max_iters, init_iters, d;
};

// options, without anything that depends on n
static int32_t hm_opts(srx_ctx* ctx, const srx_harmony_opts* in, uint64_t d_full, HmOpts* o) {
    const srx_harmony_opts s = in ? *in : srx_harmony_opts{2.0, 0.1, 1.0, 1e-5, 1e-4, 0, 0, 0, 0, 0, 0, 0};
    if (!(is_finite(s.theta) && s.theta >= 0.0)) return fail(ctx, SRX_E_ARG, "harmony: theta must be finite and >= 0");
    if (!(is_finite(s.sigma) && s.sigma > 0.0)) return fail(ctx, SRX_E_ARG, "harmony: sigma must be finite and > 0");
    if (!(is_finite(s.lambda) && s.lambda > 0.0)) return fail(ctx, SRX_E_ARG, "harmony: lambda must be finite and > 0");
    if (!(is_finite(s.epsilon_cluster) && s.epsilon_cluster >= 0.0) || !(is_finite(s.epsilon_harmony) && s.epsilon_harmony >= 0.0))
        return fail(ctx, SRX_E_ARG, "harmony: epsilon_cluster and epsilon_harmony must be finite and >= 0");
    if (s.n_clusters < 0 || s.n_clusters > SRX_HARMONY_MAX_CLUSTERS)
        return fail(ctx, SRX_E_ARG, "harmony: n_clusters = %d outside 0..%d", s.n_clusters, SRX_HARMONY_MAX_CLUSTERS);
    if (s.n_blocks < 0 || (uint32_t)s.n_blocks > kHmMaxBlocks)
        return fail(ctx, SRX_E_ARG, "harmony: n_blocks = %d outside 0..%u", s.n_blocks, kHmMaxBlocks);
    if (s.max_rounds < 0 || s.max_rounds > SRX_HARMONY_MAX_ROUNDS)
        return fail(ctx, SRX_E_ARG, "harmony: max_rounds = %d outside 0..%d", s.max_rounds, SRX_HARMONY_MAX_ROUNDS);
    if (s.max_cluster_iters < 0 || s.max_cluster_iters > 65536)
        return fail(ctx, SRX_E_ARG, "harmony: max_cluster_iters = %d outside 0..65536", s.max_cluster_iters);
    if (s.init_iters < -1 || s.init_iters > 65536) return fail(ctx, SRX_E_ARG, "harmony: init_iters = %d outside -1..65536", s.init_iters);
    if (s.n_dims < 0 || (uint64_t)s.n_dims > d_full)
        return fail(ctx, SRX_E_ARG, "harmony: n_dims = %d but the points have %llu coordinates", s.n_dims, (unsigned long long)d_full);
    const uint64_t d = s.n_dims ? (uint64_t)s.n_dims : d_full;
    if (d < 1 || d > SRX_KNN_MAX_DIMS)
        return fail(ctx, SRX_E_ARG, "harmony: %llu coordinates outside 1..%d", (unsigned long long)d, SRX_KNN_MAX_DIMS);
    *o = HmOpts{s.theta, s.sigma, s.lambda, s.epsilon_cluster, s.epsilon_harmony, s.seed, s.n_clusters, s.n_blocks ? s.n_blocks : 20,
                s.max_rounds ? s.max_rounds : 10, s.max_cluster_iters ? s.max_cluster_iters : 20,
                s.init_iters < 0 ? 0 : (s.init_iters ? s.init_iters : 10), (int)d};
    return SRX_OK;
}

static int32_t hm_alloc(srx_ctx* ctx, uint64_t n, uint32_t d, uint32_t K, uint32_t B, srx_harmony** out) {
    srx_harmony* h = new srx_harmony;
    h->ctx = ctx;
    h->n = n;
    h->d = d;
    h->K = K;
    h->B = B;
    const size_t o_r = up256(n * d * 8), o_y = o_r + up256(n * K * 8), o_o = o_y + up256((size_t)K * d * 8),
                 o_e = o_o + up256((size_t)K * B * 8), total = o_e + up256((size_t)K * B * 8);
    hipError_t e = hipMalloc(&h->d_block, total + 256);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "harmony: %zu bytes: %s", total, hipGetErrorString(e));
    }
    char* p = (char*)h->d_block;
    h->d_zc = (double*)p;
    h->d_r = (double*)(p + o_r);
    h->d_y = (double*)(p + o_y);
    h->d_o = (double*)(p + o_o);
    h->d_e = (double*)(p + o_e);
    *out = h;
    return SRX_OK;
}

template <int MODE>
static int32_t hm_launch_assign(srx_ctx* ctx, const HmAssign& a, bool ylds, size_t lds, unsigned grid) {
    if (ylds) {
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_hm_assign<MODE, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_hm_assign<MODE, true>), dim3(grid), dim3(256), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((k_hm_assign<MODE, false>), dim3(grid), dim3(256), 0, ctx->stream, a);
    }
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// x: the points on the device, n x (>= o.d) with pitch ld.  batch: host labels.  n >= 1, K <= n.
static int32_t hm_run(srx_ctx* ctx, const double* x, size_t ld, uint64_t n, const uint32_t* batch, uint32_t B, const HmOpts& o,
                      srx_harmony* h) {
    hipStream_t st = ctx->stream;
    const int d = o.d, K = (int)h->K;
    // ---- host: batch sizes, the cells ordered by (batch, cell), the chunks of the correction, the start cells
    std::vector<uint64_t> nb(B, 0);
    for (uint64_t i = 0; i < n; ++i) nb[batch[i]]++;
    std::vector<double> pb(B);
    for (uint32_t b = 0; b < B; ++b) pb[b] = (double)nb[b] / (double)n;
    const uint64_t per_g = std::max<uint64_t>(256, ((n + 255) / 256 + kHmRows - 1) / kHmRows * kHmRows);   // rows per chunk of k_hm_gemm_t
    const int chunks_y = (int)((n + per_g - 1) / per_g);
    std::vector<uint32_t> perm(n), cb(B + 1, 0);
    std::vector<uint64_t> lo;
    {
        std::vector<uint64_t> off(B + 1, 0);
        for (uint32_t b = 0; b < B; ++b) off[b + 1] = off[b] + nb[b];
        std::vector<uint64_t> cur(off.begin(), off.end() - 1);
        for (uint64_t i = 0; i < n; ++i) perm[cur[batch[i]]++] = (uint32_t)i;
        for (uint32_t b = 0; b < B; ++b) {
            for (uint64_t s = off[b]; s < off[b + 1]; s += per_g) lo.push_back(s);
            cb[b + 1] = (uint32_t)lo.size();
        }
        lo.push_back(n);
        // a chunk ends where the next begins, and the last chunk of a batch where the batch ends: the same number
    }
    const int chunks_c = (int)lo.size() - 1;
    std::vector<uint32_t> start(K);
    {
        std::vector<std::pair<uint64_t, uint32_t>> key(n);
        for (uint64_t i = 0; i < n; ++i) key[i] = {hm_hash(o.seed, 0, i), (uint32_t)i};
        std::partial_sort(key.begin(), key.begin() + K, key.end());
        for (int k = 0; k < K; ++k) start[k] = key[k].second;
    }
    // chunks of the grouped tables: as many as keep the partial tables within 64 MiB, at most 2048
    const uint64_t kb = (uint64_t)K * B;
    const uint64_t max_t = std::min<uint64_t>(2048, std::max<uint64_t>(16, (8ull << 20) / kb));
    const int chunks_t = (int)std::max<uint64_t>(1, std::min<uint64_t>(max_t, (n + 511) / 512));
    const uint64_t per_t = (n + chunks_t - 1) / chunks_t;
    const int dp = d | 1;
    int bp = 1;
    while (bp < (int)B) bp <<= 1;
    const size_t y_lds = (size_t)K * dp * 8;
    const bool ylds = y_lds <= kHmYLds;
    const unsigned grid_a = (unsigned)std::min<uint64_t>(2048, ((n + 63) / 64 + 3) / 4);
    const unsigned grid_n = (unsigned)((n + 255) / 256);

    // ---- scratch
    double *d_zh, *d_part, *d_tpart, *d_ratio, *d_m, *d_w, *d_pb, *d_obj;
    uint32_t *d_batch, *d_q, *d_perm, *d_start, *d_cb;
    uint64_t* d_lo;
    int* d_bad;
    SRX_TRY(scratch(ctx, "harmony_zh", n * d * 8, (void**)&d_zh));
    SRX_TRY(scratch(ctx, "harmony_part", (size_t)std::max(chunks_y, chunks_c) * K * d * 8, (void**)&d_part));
    SRX_TRY(scratch(ctx, "harmony_tpart", (size_t)chunks_t * kb * 8, (void**)&d_tpart));
    SRX_TRY(scratch(ctx, "harmony_ratio", kb * 8, (void**)&d_ratio));
    SRX_TRY(scratch(ctx, "harmony_m", kb * 8, (void**)&d_m));
    SRX_TRY(scratch(ctx, "harmony_w", kb * d * 8, (void**)&d_w));
    SRX_TRY(scratch(ctx, "harmony_pb", (size_t)B * 8 + 8, (void**)&d_pb));
    SRX_TRY(scratch(ctx, "harmony_obj", (size_t)grid_a * 4 * 8, (void**)&d_obj));
    SRX_TRY(scratch(ctx, "harmony_batch", n * 4, (void**)&d_batch));
    SRX_TRY(scratch(ctx, "harmony_q", n * 4, (void**)&d_q));
    SRX_TRY(scratch(ctx, "harmony_perm", n * 4, (void**)&d_perm));
    SRX_TRY(scratch(ctx, "harmony_start", (size_t)K * 4, (void**)&d_start));
    SRX_TRY(scratch(ctx, "harmony_cb", (size_t)(B + 1) * 4, (void**)&d_cb));
    SRX_TRY(scratch(ctx, "harmony_lo", lo.size() * 8, (void**)&d_lo));
    d_bad = reinterpret_cast<int*>(d_pb + B);
    SRX_TRY(h2d(ctx, d_batch, batch, n * 4));
    SRX_TRY(h2d(ctx, d_perm, perm.data(), n * 4));
    SRX_TRY(h2d(ctx, d_start, start.data(), (size_t)K * 4));
    SRX_TRY(h2d(ctx, d_cb, cb.data(), (size_t)(B + 1) * 4));
    SRX_TRY(h2d(ctx, d_lo, lo.data(), lo.size() * 8));
    SRX_TRY(h2d(ctx, d_pb, pb.data(), (size_t)B * 8));

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());

    SRX_HIP(ctx, hipMemsetAsync(d_bad, 0, 4, st));
    hipLaunchKernelGGL(k_hm_cosine, dim3(grid_n), dim3(256), 0, st, x, ld, n, d, d_zh, d_bad);
    SRX_HIP(ctx, hipGetLastError());
    int bad = 0;
    SRX_TRY(d2h(ctx, &bad, d_bad, 4));
    if (bad) return fail(ctx, SRX_E_ARG, "harmony: the points hold NaN or Inf");

    HmAssign a{d_zh, h->d_y, d_batch, d_q, nullptr, h->d_o, h->d_e, h->d_r, d_obj, n, d, K, (int)B, dp, -1, o.sigma, o.theta};
    auto centroids = [&]() -> int32_t {       // Y = normalise(R^T Zhat)
        hipLaunchKernelGGL(k_hm_gemm_t, dim3(chunks_y, (K + kHmKT - 1) / kHmKT), dim3(256), 0, st, h->d_r, K, d_zh, (size_t)d, d,
                           (const uint32_t*)nullptr, (const uint64_t*)nullptr, per_g, n, d_part);
        hipLaunchKernelGGL(k_hm_centroids, dim3(K), dim3(128), 0, st, d_part, chunks_y, K, d, h->d_y);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    auto tables = [&](int q, int mode, double* o_out) -> int32_t {
        hipLaunchKernelGGL(k_hm_tables, dim3(chunks_t), dim3(256), 0, st, h->d_r, n, K, (int)B, per_t, d_batch, d_q, q, d_tpart);
        hipLaunchKernelGGL(k_hm_fold, dim3(K), dim3(256), 0, st, d_tpart, chunks_t, K, (int)B, bp, d_pb, mode, o.theta, o_out, h->d_e, d_ratio);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };

    // ---- start: K cells, spherical k-means, the first soft assignment
    hipLaunchKernelGGL(k_hm_gather, dim3(K), dim3(128), 0, st, d_zh, d_start, d, h->d_y);
    for (int it = 0; it < o.init_iters; ++it) {
        SRX_TRY(hm_launch_assign<kHard>(ctx, a, ylds, y_lds, grid_a));
        SRX_TRY(centroids());
    }
    SRX_TRY(hm_launch_assign<kSoft>(ctx, a, ylds, y_lds, grid_a));
    SRX_TRY(tables(-1, kFoldInit, h->d_o));

    srx_harmony_info& info = h->info;
    std::vector<double> obj_part((size_t)grid_a * 4);
    uint64_t t = 0;
    for (int r = 1; r <= o.max_rounds; ++r) {
        std::vector<double> objs;
        for (int j = 1; j <= o.max_iters; ++j) {
            SRX_TRY(centroids());
            hipLaunchKernelGGL(k_hm_blocks, dim3(grid_n), dim3(256), 0, st, o.seed, 1 + t, n, (uint32_t)o.n_blocks, d_q);
            for (int q = 0; q < o.n_blocks; ++q) {
                SRX_TRY(tables(q, kFoldOut, h->d_o));
                a.q = q;
                a.ratio = d_ratio;
                SRX_TRY(hm_launch_assign<kSoft>(ctx, a, ylds, y_lds, grid_a));
                SRX_TRY(tables(q, kFoldIn, h->d_o));
            }
            a.q = -1;
            a.ratio = nullptr;
            ++t;
            SRX_TRY(hm_launch_assign<kObjective>(ctx, a, ylds, y_lds, grid_a));
            SRX_TRY(d2h(ctx, obj_part.data(), d_obj, obj_part.size() * 8));
            double ov = 0.0;
            for (double p : obj_part) ov += p;
            objs.push_back(ov);
            if (j >= 6 && o.eps_cluster > 0.0) {
                const double old = objs[j - 6] + objs[j - 5] + objs[j - 4], nw = objs[j - 3] + objs[j - 2] + objs[j - 1];
                if ((old - nw) / fabs(old) < o.eps_cluster) break;
            }
        }
        info.round_iters[r - 1] = (uint32_t)objs.size();
        info.round_objective[r - 1] = objs.back();
        info.rounds = (uint32_t)r;
        // correction from the original points, then the cosine rows of the corrected ones
        SRX_TRY(tables(-1, kFoldM, d_m));
        hipLaunchKernelGGL(k_hm_gemm_t, dim3(chunks_c, (K + kHmKT - 1) / kHmKT), dim3(256), 0, st, h->d_r, K, x, ld, d, d_perm, d_lo,
                           (uint64_t)0, n, d_part);
        hipLaunchKernelGGL(k_hm_ridge, dim3(K), dim3(128), 0, st, d_part, d_cb, K, (int)B, d, d_m, o.lambda, d_w);
        hipLaunchKernelGGL(k_hm_correct, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, x, ld, h->d_r, d_w, d_batch, n, K, d, h->d_zc);
        hipLaunchKernelGGL(k_hm_cosine, dim3(grid_n), dim3(256), 0, st, h->d_zc, (size_t)d, n, d, d_zh, (int*)nullptr);
        SRX_HIP(ctx, hipGetLastError());
        if (r >= 2 && o.eps_harmony > 0.0) {
            const double hp = info.round_objective[r - 2], hr = info.round_objective[r - 1];
            if ((hp - hr) / fabs(hp) < o.eps_harmony) {
                info.converged = 1;
                break;
            }
        }
    }
    SRX_TRY(timer.stop(&info.ms));
    info.cluster_iters = t;
    return SRX_OK;
}

// everything after the points are on the device: the checks that need n, the handle, the run
static int32_t hm_device(srx_ctx* ctx, const double* x, size_t ld, uint64_t n, const uint32_t* batch, uint32_t n_batches,
                         const HmOpts& o_in, srx_harmony** out, srx_harmony_info* info_out) {
    HmOpts o = o_in;
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "harmony: more than 2^32 - 2 cells");
    if (n == 0) o.K = o.K ? o.K : 1;
    else if (o.K == 0) o.K = (int)std::max<uint64_t>(1, std::min<uint64_t>((n + 15) / 30, 100));
    if (n && (uint64_t)o.K > n) return fail(ctx, SRX_E_ARG, "harmony: n_clusters = %d but only %llu cells", o.K, (unsigned long long)n);
    for (uint64_t i = 0; i < n; ++i)
        if (batch[i] >= n_batches)
            return fail(ctx, SRX_E_ARG, "harmony: cell %llu has batch %u, not below n_batches = %u", (unsigned long long)i, batch[i], n_batches);
    srx_harmony* h = nullptr;
    SRX_TRY(hm_alloc(ctx, n, (uint32_t)o.d, (uint32_t)o.K, n_batches, &h));
    h->info.n = n;
    h->info.d = (uint32_t)o.d;
    h->info.n_batches = n_batches;
    h->info.n_clusters = (uint32_t)o.K;
    h->info.n_blocks = (uint32_t)o.n_blocks;
    if (n) {
        Range rg("harmony");
        const int32_t rc = hm_run(ctx, x, ld, n, batch, n_batches, o, h);
        if (rc != SRX_OK) {
            srx_harmony_free(h);
            return rc;
        }
    }
    if (info_out) *info_out = h->info;
    *out = h;
    return SRX_OK;
}

static int32_t hm_check_common(srx_ctx* ctx, const uint32_t* batch, uint32_t n_batches, uint64_t n, srx_harmony** out) {
    if (!out) return fail(ctx, SRX_E_ARG, "harmony: null output handle");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "harmony: rows are sharded; the integration needs all cells");
    if (n_batches < 1 || n_batches > SRX_HARMONY_MAX_BATCHES)
        return fail(ctx, SRX_E_ARG, "harmony: n_batches = %u outside 1..%d", n_batches, SRX_HARMONY_MAX_BATCHES);
    if (!batch && n) return fail(ctx, SRX_E_ARG, "harmony: null batch labels");
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_harmony_result(srx_mat* m, const uint32_t* batch, uint32_t n_batches, const srx_harmony_opts* opts, srx_harmony** out,
                           srx_harmony_info* info) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "no PCA result on this matrix");
    const uint64_t n = m->csc ? m->n_cols : m->n_rows;       // cells: the column axis of a CSC handle (as srx_knn_result)
    SRX_TRY(hm_check_common(ctx, batch, n_batches, n, out));
    HmOpts o;
    SRX_TRY(hm_opts(ctx, opts, m->pca.n_pc, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return hm_device(ctx, m->pca.d_scores, (size_t)scores_ld((int)m->pca.n_pc), n, batch, n_batches, o, out, info);
}

int32_t srx_harmony_points(srx_ctx* ctx, const double* points, uint64_t n, uint64_t d, const uint32_t* batch, uint32_t n_batches,
                           const srx_harmony_opts* opts, srx_harmony** out, srx_harmony_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    SRX_TRY(hm_check_common(ctx, batch, n_batches, n, out));
    if (!points && n) return fail(ctx, SRX_E_ARG, "harmony: null points");
    HmOpts o;
    SRX_TRY(hm_opts(ctx, opts, d, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    double* d_x = nullptr;
    if (n) {
        SRX_TRY(scratch(ctx, "harmony_in", n * d * 8, (void**)&d_x));
        SRX_TRY(h2d(ctx, d_x, points, n * d * 8));
    }
    return hm_device(ctx, d_x, (size_t)d, n, batch, n_batches, o, out, info);
}

int32_t srx_harmony_fetch(srx_harmony* h, int32_t which, double* out) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null harmony handle");
    srx_ctx* ctx = h->ctx;
    const double* src;
    size_t count;
    switch (which) {
        case SRX_HARMONY_CORRECTED: src = h->d_zc; count = h->n * h->d; break;
        case SRX_HARMONY_R: src = h->d_r; count = h->n * h->K; break;
        case SRX_HARMONY_CENTROIDS: src = h->d_y; count = (size_t)h->K * h->d; break;
        case SRX_HARMONY_OBSERVED: src = h->d_o; count = (size_t)h->K * h->B; break;
        case SRX_HARMONY_EXPECTED: src = h->d_e; count = (size_t)h->K * h->B; break;
        default: return fail(ctx, SRX_E_ARG, "srx_harmony_fetch: which = %d names no table", which);
    }
    if (h->n == 0) return SRX_OK;                    // an empty handle holds no table
    if (!out) return fail(ctx, SRX_E_ARG, "srx_harmony_fetch: null output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, out, src, count * 8);
}

int32_t srx_harmony_info_get(const srx_harmony* h, srx_harmony_info* info) {
    if (!h || !info) return fail(h ? h->ctx : nullptr, SRX_E_ARG, "null argument");
    *info = h->info;
    return SRX_OK;
}

int32_t srx_knn_harmony(srx_harmony* h, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out, srx_knn_info* info) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null harmony handle");
    srx_ctx* ctx = h->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return knn_self_device(ctx, h->d_zc, h->n, h->d, (size_t)h->d, opts, indices_out, distances_out, info, nullptr, nullptr, nullptr);
}

int32_t srx_neighbors_harmony(srx_harmony* h, const srx_knn_opts* opts, srx_knn_info* knn_info, srx_graph** out) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null harmony handle");
    srx_ctx* ctx = h->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "neighbors: null output handle");
    *out = nullptr;
    if (!opts) return fail(ctx, SRX_E_ARG, "neighbors: null options");
    if (opts->include_self) return fail(ctx, SRX_E_ARG, "neighbors: the graph is built from a list that excludes self (include_self = 0)");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t* d_idx = nullptr;
    const double* d_dist = nullptr;
    uint64_t n = 0;
    SRX_TRY(knn_self_device(ctx, h->d_zc, h->n, h->d, (size_t)h->d, opts, nullptr, nullptr, knn_info, &d_idx, &d_dist, &n));
    return graph_from_device_list(ctx, d_idx, d_dist, n, (uint32_t)opts->k, out);
}

int32_t srx_bbknn_harmony(srx_harmony* h, const uint32_t* batch, uint32_t n_batches, const srx_bbknn_opts* opts, srx_bbknn_info* info,
                          srx_graph** out) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null harmony handle");
    srx_ctx* ctx = h->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "bbknn: null output handle");
    *out = nullptr;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return bbknn_device(ctx, h->d_zc, nullptr, (size_t)h->d, h->n, h->d, batch, n_batches, opts, nullptr, nullptr, info, out);
}

void srx_harmony_free(srx_harmony* h) {
    if (!h) return;
    if (h->d_block) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        (void)hipFree(h->d_block);
    }
    delete h;
}

}  // extern "C"
