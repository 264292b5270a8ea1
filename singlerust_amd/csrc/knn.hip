// knn.hip — exact k-nearest-neighbour search over dense f64 points (the PCA scores a fit left in HBM, or points the
// caller supplies): srx_knn_result / srx_knn_points.
//
// N x N is never formed.  An f32 pass on the matrix cores PROPOSES K' = k + kKnnSlack candidates per query, f64 decides:
//
//   k_knn_colsum / _finish   column means of the reference in a fixed order (the centre c), finiteness of every point
//   k_knn_fragments          f32 copy of x - c in MFMA fragment order with |x - c|^2 as one more coordinate; max |x - c|^2.
//                            Behind knn_prepare, which knn_ivf.hip calls too (through an index array, for its list-major copy)
//   k_knn_candidates<K, RT>  s(q, r) = |r|^2 - 2 q.r on v_mfma_f32_32x32x2_f32 for a block of 128 queries against every
//                            reference tile; the K' smallest per query kept in LDS; out: their indices and the bound tau
//   k_knn_exact<false>       f64 distances (difference form) of the K' candidates, sorted by (distance, index), the first
//                            k written; the certificate below decides whether the row is proven
//   k_knn_exact<true>        the rows the certificate refused: the same f64 selection over ALL references
// What the inverted-file index shares with this file is in knn_internal.hpp, stated there once: the keys and their merge,
// the keep step of the f64 selection (knn_take), eps_row of the certificate (knn_certificate), and on the host the (K, RT)
// instance table with its dispatch, the dynamic LDS and the candidate counts K' and CAP.  The tile loop of k_knn_candidates
// is stated a second time in k_ivf_candidates (see the note there).
//
// Certificate.  With centred points q, r in f64 the pass approximates t(q, r) = |r|^2 - 2 q.r = dist^2 - |q|^2, which orders
// the references of one query exactly as the distance does.  What it computes is an f32 fmaf chain over K = padded d + 1
// products (the MFMA is bit-for-bit such a chain) on inputs rounded to f32, u = 2^-24:
//     chain of K products:            |fl(sum) - sum| <= gamma_K * sum|a_j b_j|,   gamma_K = K u / (1 - K u)
//     each coordinate rounded once:   |fl(q_j) fl(r_j) - q_j r_j| <= (2u + u^2) |q_j r_j|;  the factor -2 and the 1 are exact
//     the norm coordinate:            |fl(|r|^2) - |r|^2| <= u |r|^2
// so with sum|q_j r_j| <= |q| |r| (Cauchy-Schwarz) and |r| <= R = the largest reference norm
//     |s - t| <= (K + 3) u (1 + K u) (2 |q| R + R^2)  <  eps_row := 1.01 (K + 4) u (2 |q| R + R^2).
// The 1 % covers the second-order terms and every f64 rounding in q, R, the centring and the re-rank (all ~1e-16 relative).
// Products that underflow in f32 would add an absolute term; R is therefore required inside [2^-40, 2^60] and eps_row is
// +inf outside (every row then takes the f64 pass).  Every point the pass did not keep has s >= tau (kept-or-dropped is
// decided against a threshold that only falls), hence t >= tau - eps_row.  A row is proven when
//     t_k + eps_row < tau,      t_k = (k-th exact squared distance) - |q|^2:
// strictly, and by a margin of at least 0.01 eps_row, so no point left out can tie with the k-th one even in rounded f64.
#include "common.hpp"
#include "knn_internal.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>

namespace srx {

// ---- centre, finiteness ------------------------------------------------------------------------------------------------
// grid.x blocks of 256 threads; thread t owns column t % dpow (dpow = d rounded up to a power of two <= 256) and walks the rows
// of its block's range in order: the partial of (block, column) is one fixed-order sum.  part: gridDim.x x d.
__global__ void __launch_bounds__(256) k_knn_colsum(const double* __restrict__ x, uint64_t n, int d, size_t ld, int dpow,
                                                    double* __restrict__ part, int* __restrict__ bad) {
    __shared__ double sh[256];
    const int col = threadIdx.x % dpow, lane_row = threadIdx.x / dpow, rows_per_it = 256 / dpow;
    const uint64_t per = (n + gridDim.x - 1) / gridDim.x;
    const uint64_t r0 = per * blockIdx.x, r1 = r0 + per < n ? r0 + per : n;
    double s = 0.0;
    bool nf = false;
    if (col < d)
        for (uint64_t r = r0 + lane_row; r < r1; r += rows_per_it) {
            const double v = x[r * ld + col];
            nf |= !is_finite(v);
            s += v;
        }
    if (nf) *bad = 1;
    sh[threadIdx.x] = s;
    __syncthreads();
    if (part && threadIdx.x < d) {
        double t = 0.0;
        for (int g = 0; g < rows_per_it; ++g) t += sh[g * dpow + threadIdx.x];
        part[(size_t)blockIdx.x * d + threadIdx.x] = t;
    }
}
__global__ void k_knn_colsum_finish(const double* __restrict__ part, int n_part, int d, uint64_t n, double* __restrict__ centre,
                                    unsigned long long* __restrict__ rmax2_bits) {
    const int c = threadIdx.x;
    if (c < d) {
        double t = 0.0;
        for (int p = 0; p < n_part; ++p) t += part[(size_t)p * d + c];
        centre[c] = t / (double)n;
    }
    if (c == 0) *rmax2_bits = 0ull;
}

// ---- f32 copy in fragment order ----------------------------------------------------------------------------------------
// Points are grouped in blocks of 32; block b holds K floats per point as [s = kk / 2][h = kk & 1][i = point % 32], so that
// lane l of a wave reads word s * 64 + l for step s of v_mfma_f32_32x32x2_f32 (operand element [i = l & 31][k = l >> 5]):
// consecutive words, no bank conflict, and a reference tile is one contiguous piece of memory.  Position p is point ids[p]
// (ids null: p itself below n), and what each coordinate holds is stated at knn_prepare (knn_internal.hpp), the launcher
// both searches call.
__global__ void __launch_bounds__(256) k_knn_fragments(const double* __restrict__ x, size_t ld, const uint32_t* __restrict__ ids,
                                                       uint64_t n, uint64_t n_pad, int d, int K, const double* __restrict__ centre,
                                                       float* __restrict__ out, unsigned long long* __restrict__ rmax2_bits) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pad) return;
    const uint32_t src = ids ? ids[p] : (p < n ? (uint32_t)p : kKnnNone);
    const bool real = src != kKnnNone;
    float* o = out + (p >> 5) * (size_t)(32 * K) + (p & 31);
    double nrm = 0.0;
    for (int kk = 0; kk < d; ++kk) {
        const double v = real ? x[(size_t)src * ld + kk] - centre[kk] : 0.0;
        nrm += v * v;
        o[(kk >> 1) * 64 + (kk & 1) * 32] = (float)v;
    }
    o[(d >> 1) * 64 + (d & 1) * 32] = real ? (float)nrm : __builtin_inff();
    for (int kk = d + 1; kk < K; ++kk) o[(kk >> 1) * 64 + (kk & 1) * 32] = 0.f;
    // non-negative doubles order as their bit patterns: an order-free maximum
    if (rmax2_bits && real) atomicMax(rmax2_bits, (unsigned long long)__double_as_longlong(nrm));
}

int32_t knn_prepare(srx_ctx* ctx, const double* d_x, size_t ld, const uint32_t* d_ids, uint64_t n, uint64_t n_pad, int d, int K,
                    const double* d_centre, float* d_out, unsigned long long* d_rmax2_bits) {
    hipLaunchKernelGGL(k_knn_fragments, dim3(grid256(n_pad)), dim3(256), 0, ctx->stream, d_x, ld, d_ids, n, n_pad, d, K, d_centre,
                       d_out, d_rmax2_bits);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// ---- candidate pass (the keys of one query in LDS and their merge: knn_internal.hpp) -------------------------------------
// K: padded coordinates (even, > d); RT: references per tile.  Dynamic LDS: 2 tiles | keys 128 x CAP | cnt 128 | tau 128.
// self_skip: query i is reference i and may not list itself.
template <int K, int RT>
__global__ void __launch_bounds__(256) k_knn_candidates(const float* __restrict__ ref_t, uint64_t n_ref_pad,
                                                        const float* __restrict__ qry_t, uint64_t n_query, uint64_t n_query_pad,
                                                        int d, int KP, int CAP, int self_skip,
                                                        uint32_t* __restrict__ cand, float* __restrict__ tau_out) {
    constexpr int S = K / 2;                       // MFMA steps per 32 x 32 tile
    constexpr int TILE = RT * K;                   // floats
    constexpr int NV = (TILE / 4 + 255) / 256;     // float4 per thread and tile
    extern __shared__ __align__(16) unsigned char smem[];
    float* tiles = reinterpret_cast<float*>(smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + (size_t)2 * TILE * 4);
    int* cnt = reinterpret_cast<int*>(keys + (size_t)kKnnQB * CAP);
    float* tau_s = reinterpret_cast<float*>(cnt + kKnnQB);

    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int qs = wave * 32 + j;                  // this lane's query slot (two lanes share one)
    const uint64_t q_first = (uint64_t)blockIdx.x * kKnnQB + (uint64_t)wave * 32;
    const uint64_t q_idx = q_first + j;

    if (threadIdx.x < kKnnQB) {
        cnt[threadIdx.x] = 0;
        tau_s[threadIdx.x] = __builtin_inff();
    }
    // B operand: (-2 q, 1, 0..): element [k = 2s + h][column j]
    float qreg[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int kk = 2 * s + h;
        float v = 0.f;
        if (q_first < n_query_pad && kk < d) v = -2.f * qry_t[(q_first >> 5) * (size_t)(32 * K) + s * 64 + lane];
        qreg[s] = kk == d ? 1.f : v;
    }
    const uint64_t n_tiles = n_ref_pad / RT;
    const f32x4* g = reinterpret_cast<const f32x4*>(ref_t);
    f32x4 stage[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int w = v * 256 + (int)threadIdx.x;
        stage[v] = g[w < TILE / 4 ? w : 0];
        if (w < TILE / 4) reinterpret_cast<f32x4*>(tiles)[w] = stage[v];
    }
    __syncthreads();
    float tau = __builtin_inff();
    const int full = CAP - 32;                     // a 32-reference sub-tile adds at most 32 entries to a query

    for (uint64_t t = 0; t < n_tiles; ++t) {
        const bool more = t + 1 < n_tiles;
        if (more) {
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int w = v * 256 + (int)threadIdx.x;
                stage[v] = g[(t + 1) * (size_t)(TILE / 4) + (w < TILE / 4 ? w : 0)];
            }
        }
        const float* cur = tiles + (t & 1) * TILE;
#pragma unroll
        for (int sub = 0; sub < RT / 32; ++sub) {
            f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < S; ++s)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[(sub * S + s) * 64 + lane], qreg[s], acc, 0, 0, 0);
            // common path: nothing in the tile is below the query's bound — one minimum tree, one compare, one ballot
            float lo = acc[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) lo = fminf(lo, acc[r]);
            if (__builtin_amdgcn_ballot_w64(lo < tau) != 0ull) {
                const uint32_t base = (uint32_t)(t * RT) + sub * 32 + 4 * h;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t idx = base + (r & 3) + 8 * (r >> 2);     // C/D map: row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                    if (acc[r] < tau && !(self_skip && idx == (uint32_t)q_idx)) {
                        const int slot = atomicAdd(&cnt[qs], 1);
                        keys[(size_t)qs * CAP + slot] = ((unsigned long long)f32_key(acc[r]) << 32) | idx;
                    }
                }
                wave_lds_sync();
                unsigned long long need = __builtin_amdgcn_ballot_w64(h == 0 && cnt[qs] > full);
                while (need) {
                    const int jj = __builtin_ctzll(need);
                    need &= need - 1;
                    knn_merge(keys, cnt, tau_s, wave * 32 + jj, CAP, KP);
                }
                tau = tau_s[qs];
            }
        }
        if (more) {
            f32x4* nxt = reinterpret_cast<f32x4*>(tiles + ((t + 1) & 1) * TILE);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const int w = v * 256 + (int)threadIdx.x;
                if (w < TILE / 4) nxt[w] = stage[v];
            }
        }
        __syncthreads();
    }
    // sort what is left and hand out the KP lowest with the bound every dropped point respects
    wave_lds_sync();
    for (int jj = 0; jj < 32; ++jj) {
        const int s = wave * 32 + jj;
        const uint64_t q = q_first + jj;
        if (q >= n_query) break;
        knn_merge(keys, cnt, tau_s, s, CAP, KP);
        const int n = cnt[s];
        for (int c = lane; c < KP; c += 64) cand[q * KP + c] = c < n ? (uint32_t)keys[(size_t)s * CAP + c] : kKnnNone;
        if (lane == 0) tau_out[q] = tau_s[s];
    }
}

// ---- f64 selection (knn_dist2, knn_less, knn_take, knn_certificate: knn_internal.hpp) ----------------------------------
// One wave per query row.  ALL = false: the row's KP candidates; ALL = true: row rows[..] against every reference.
// The wave keeps at most k + 64 entries in LDS: 64 references at a time, those below the k-th kept one go through the keep
// step.  ALL = false also evaluates the certificate and lists the rows that fail it in `fail_rows` (count in fail_n).
template <bool ALL>
__global__ void __launch_bounds__(256) k_knn_exact(const double* __restrict__ ref, uint64_t n_ref, size_t ld_r,
                                                   const double* __restrict__ qry, uint64_t n_query, size_t ld_q, int d, int k,
                                                   int KP, int self_skip, const uint32_t* __restrict__ cand,
                                                   const float* __restrict__ tau, const double* __restrict__ centre,
                                                   const unsigned long long* __restrict__ rmax2_bits, int Kpad,
                                                   const uint32_t* __restrict__ rows, uint64_t n_rows,
                                                   uint32_t* __restrict__ idx_out, double* __restrict__ dist_out,
                                                   uint32_t* __restrict__ fail_rows, unsigned int* __restrict__ fail_n) {
    __shared__ double sd[4][128];
    __shared__ uint32_t si[4][128];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
    if (w >= (ALL ? n_rows : n_query)) return;
    const uint64_t q = ALL ? rows[w] : w;
    const double* qp = qry + q * ld_q;
    double* D = sd[wave];
    uint32_t* I = si[wave];
    int n = 0;                                    // kept entries, sorted, wave-uniform
    const uint64_t total = ALL ? n_ref : (uint64_t)KP;
    for (uint64_t c0 = 0; c0 < total; c0 += 64) {
        uint32_t idx = kKnnNone;
        if (c0 + lane < total) idx = ALL ? (uint32_t)(c0 + lane) : cand[q * KP + c0 + lane];
        bool ok = idx != kKnnNone && !(self_skip && idx == (uint32_t)q);
        double dd = 0.0;
        if (ok) {
            dd = knn_dist2(qp, ref + (size_t)idx * ld_r, d);
            if (n == k) ok = knn_less(dd, idx, D[k - 1], I[k - 1]);
        }
        n = knn_take(D, I, n, k, ok, dd, idx);
    }
    // (the caller guarantees k admissible references, and K' >= k candidates exist whenever that many references do)
    bool proven = true;
    if (!ALL) {
        const KnnBound b = knn_certificate(qp, centre, d, Kpad, rmax2_bits);
        proven = n == k && (D[k - 1] - b.qn) + b.eps_row < (double)tau[q];
        if (!proven && lane == 0) fail_rows[atomicAdd(fail_n, 1u)] = (uint32_t)q;
    }
    if (proven)
        for (int c = lane; c < k; c += 64) {
            if (idx_out) idx_out[q * k + c] = I[c];
            if (dist_out) dist_out[q * k + c] = sqrt(D[c]);
        }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
int32_t knn_exact_rows(srx_ctx* ctx, const KnnArgs& a, int k, int self_skip, const uint32_t* d_rows, uint64_t n_rows,
                       uint32_t* d_idx, double* d_dist) {
    if (n_rows == 0) return SRX_OK;
    hipLaunchKernelGGL(k_knn_exact<true>, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, ctx->stream, a.d_ref, a.n_ref, a.ld_r,
                       a.d_qry, a.n_query, a.ld_q, a.d, k, 0, self_skip, (const uint32_t*)nullptr, (const float*)nullptr,
                       (const double*)nullptr, (const unsigned long long*)nullptr, 0, d_rows, n_rows, d_idx, d_dist,
                       (uint32_t*)nullptr, (unsigned int*)nullptr);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

int32_t knn_device(srx_ctx* ctx, const KnnArgs& a, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out,
                   srx_knn_info* info) {
    const int k = opts->k, d = a.d;
    const uint64_t admissible = a.n_ref - ((a.self && !opts->include_self) ? 1 : 0);
    const int self_skip = a.self && !opts->include_self;
    const KnnCounts counts = knn_candidate_counts(k, admissible);
    const int KP = counts.KP, CAP = counts.CAP;
    const int K = knn_padded_width(d);
    const uint64_t n_ref_pad = (a.n_ref + kKnnPad - 1) / kKnnPad * kKnnPad, n_query_pad = (a.n_query + kKnnPad - 1) / kKnnPad * kKnnPad;
    const int n_part = (int)std::min<uint64_t>(1024, (a.n_ref + 255) / 256);
    int dpow = 1;
    while (dpow < d) dpow <<= 1;

    // one scratch block: centre d | rmax2 1 | partials n_part x d | flags | fail count, then the big arrays
    double* d_small;
    SRX_TRY(scratch(ctx, "knn_small", ((size_t)d + 2 + (size_t)n_part * d + 2) * 8, (void**)&d_small));
    double* d_centre = d_small;
    unsigned long long* d_rmax2 = reinterpret_cast<unsigned long long*>(d_small + d);
    double* d_part = d_small + d + 1;
    int* d_bad = reinterpret_cast<int*>(d_part + (size_t)n_part * d);
    unsigned int* d_fail_n = reinterpret_cast<unsigned int*>(d_bad) + 1;
    float *d_ref_t, *d_qry_t;
    SRX_TRY(scratch(ctx, "knn_ref_f32", n_ref_pad * (size_t)K * 4, (void**)&d_ref_t));
    d_qry_t = d_ref_t;
    if (!a.self) SRX_TRY(scratch(ctx, "knn_qry_f32", n_query_pad * (size_t)K * 4, (void**)&d_qry_t));
    uint32_t *d_cand, *d_fail, *d_idx;
    float* d_tau;
    double* d_dist;
    SRX_TRY(scratch(ctx, "knn_cand", a.n_query * (size_t)KP * 4, (void**)&d_cand));
    SRX_TRY(scratch(ctx, "knn_tau", a.n_query * 4, (void**)&d_tau));
    SRX_TRY(scratch(ctx, "knn_fail", a.n_query * 4, (void**)&d_fail));
    SRX_TRY(scratch(ctx, "knn_idx", a.n_query * (size_t)k * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "knn_dist", a.n_query * (size_t)k * 8, (void**)&d_dist));

    hipStream_t st = ctx->stream;
    unsigned int n_fail = 0;
    {
        ProfScope ps(ctx, SRX_K_KNN, (double)(a.n_ref + (a.self ? 0 : a.n_query)) * d * 8.0 + (double)a.n_query * k * 12.0);
        SRX_HIP(ctx, hipMemsetAsync(d_bad, 0, 8, st));
        hipLaunchKernelGGL(k_knn_colsum, dim3(n_part), dim3(256), 0, st, a.d_ref, a.n_ref, d, a.ld_r, dpow, d_part, d_bad);
        if (!a.self)
            hipLaunchKernelGGL(k_knn_colsum, dim3((unsigned)std::min<uint64_t>(1024, (a.n_query + 255) / 256)), dim3(256), 0, st,
                               a.d_qry, a.n_query, d, a.ld_q, dpow, (double*)nullptr, d_bad);
        hipLaunchKernelGGL(k_knn_colsum_finish, dim3(1), dim3(128), 0, st, d_part, n_part, d, a.n_ref, d_centre, d_rmax2);
        SRX_HIP(ctx, hipGetLastError());
        int bad = 0;
        SRX_TRY(d2h(ctx, &bad, d_bad, 4));
        if (bad) return fail(ctx, SRX_E_ARG, "knn: the points hold NaN or Inf");

        SRX_TRY(knn_prepare(ctx, a.d_ref, a.ld_r, nullptr, a.n_ref, n_ref_pad, d, K, d_centre, d_ref_t, d_rmax2));
        if (!a.self) SRX_TRY(knn_prepare(ctx, a.d_qry, a.ld_q, nullptr, a.n_query, n_query_pad, d, K, d_centre, d_qry_t, nullptr));
        SRX_TRY(knn_dispatch(K, [&](auto Kc, auto RTc) -> int32_t {
            constexpr int KK = decltype(Kc)::value, RT = decltype(RTc)::value;
            const size_t lds = knn_candidates_lds(KK, RT, CAP);
            SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_knn_candidates<KK, RT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            const unsigned grid = (unsigned)((a.n_query + kKnnQB - 1) / kKnnQB);
            hipLaunchKernelGGL((k_knn_candidates<KK, RT>), dim3(grid), dim3(256), lds, st, (const float*)d_ref_t, n_ref_pad,
                               (const float*)d_qry_t, a.n_query, n_query_pad, d, KP, CAP, self_skip, d_cand, d_tau);
            SRX_HIP(ctx, hipGetLastError());
            return SRX_OK;
        }));
        const unsigned wg = (unsigned)((a.n_query + 3) / 4);
        hipLaunchKernelGGL(k_knn_exact<false>, dim3(wg), dim3(256), 0, st, a.d_ref, a.n_ref, a.ld_r, a.d_qry, a.n_query, a.ld_q, d, k,
                           KP, self_skip, d_cand, d_tau, d_centre, d_rmax2, K, (const uint32_t*)nullptr, (uint64_t)0, d_idx, d_dist,
                           d_fail, d_fail_n);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(d2h(ctx, &n_fail, d_fail_n, 4));
        SRX_TRY(knn_exact_rows(ctx, a, k, self_skip, d_fail, n_fail, d_idx, d_dist));
    }
    if (indices_out) SRX_TRY(d2h(ctx, indices_out, d_idx, a.n_query * (size_t)k * 4));
    if (distances_out) SRX_TRY(d2h(ctx, distances_out, d_dist, a.n_query * (size_t)k * 8));
    SRX_HIP(ctx, hipStreamSynchronize(st));
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_ref = a.n_ref;
        info->n_query = a.n_query;
        info->d = (uint32_t)d;
        info->k = (uint32_t)k;
        info->n_candidates = (uint32_t)KP;
        info->rows_recomputed = n_fail;
        info->rows_certified = a.n_query - n_fail;
    }
    return SRX_OK;
}

// argument checks shared by both entry points; d_full: coordinates per point, d: those used
int32_t knn_check(srx_ctx* ctx, const srx_knn_opts* opts, uint64_t n_ref, uint64_t n_query, uint64_t d_full, bool self,
                  int* d_out) {
    if (!opts) return fail(ctx, SRX_E_ARG, "knn: null options");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "knn: rows are sharded; neighbours need all cells");
    if (opts->k < 1 || opts->k > kKnnMaxK) return fail(ctx, SRX_E_ARG, "knn: k = %d outside 1..%d", opts->k, kKnnMaxK);
    if (opts->n_dims < 0 || (uint64_t)opts->n_dims > d_full)
        return fail(ctx, SRX_E_ARG, "knn: n_dims = %d but the points have %llu coordinates", opts->n_dims, (unsigned long long)d_full);
    const uint64_t d = opts->n_dims ? (uint64_t)opts->n_dims : d_full;
    if (d < 1 || d > SRX_KNN_MAX_DIMS)
        return fail(ctx, SRX_E_ARG, "knn: %llu coordinates outside 1..%d", (unsigned long long)d, SRX_KNN_MAX_DIMS);
    if (n_ref >= 0xFFFFFFFFull || n_query >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "knn: more than 2^32 - 2 points");
    const uint64_t admissible = n_ref - ((self && !opts->include_self && n_ref) ? 1 : 0);
    if (n_query && (uint64_t)opts->k > admissible)
        return fail(ctx, SRX_E_ARG, "knn: k = %d but only %llu admissible reference points", opts->k, (unsigned long long)admissible);
    *d_out = (int)d;
    return SRX_OK;
}

// srx_knn_result with the list left on the device (graph.hip builds the neighbour graph from it): *d_idx / *d_dist are the
// "knn_idx" / "knn_dist" scratch slots, n x opts->k row-major, valid until the next k-NN call on this context.
int32_t knn_result_resident(srx_mat* m, const srx_knn_opts* opts, srx_knn_info* info, const uint32_t** d_idx,
                            const double** d_dist, uint64_t* n_out) {
    *n_out = 0;
    SRX_TRY(srx_knn_result(m, opts, nullptr, nullptr, info));
    srx_ctx* ctx = m->ctx;
    const uint64_t n = m->csc ? m->n_cols : m->n_rows;
    if (n == 0) return SRX_OK;
    SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)d_idx));
    SRX_TRY(scratch(ctx, "knn_dist", 0, (void**)d_dist));
    *n_out = n;
    return SRX_OK;
}

// The self search over n points that already lie on the device (harmony.hip: the corrected block of an srx_harmony), through
// the same checks and the same KnnArgs as srx_knn_result.  d_idx / d_dist non-null: the list is also left on the device as
// knn_result_resident leaves it (*n_out = 0 for n == 0).
int32_t knn_self_device(srx_ctx* ctx, const double* d_pts, uint64_t n, uint64_t d_full, size_t ld, const srx_knn_opts* opts,
                        uint32_t* indices_out, double* distances_out, srx_knn_info* info, const uint32_t** d_idx,
                        const double** d_dist, uint64_t* n_out) {
    if (n_out) *n_out = 0;
    int d = 0;
    SRX_TRY(knn_check(ctx, opts, n, n, d_full, true, &d));
    if (info) memset(info, 0, sizeof *info);
    if (n == 0) return SRX_OK;
    Range rg("knn");
    KnnArgs a{d_pts, d_pts, n, n, ld, ld, d, true};
    SRX_TRY(knn_device(ctx, a, opts, indices_out, distances_out, info));
    if (d_idx) {
        SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)d_idx));
        SRX_TRY(scratch(ctx, "knn_dist", 0, (void**)d_dist));
        *n_out = n;
    }
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_knn_result(srx_mat* m, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out, srx_knn_info* info) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "no PCA result on this matrix");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = m->csc ? m->n_cols : m->n_rows;      // cells: the column axis of a CSC handle (as srx_result_fetch)
    int d = 0;
    SRX_TRY(knn_check(ctx, opts, n, n, m->pca.n_pc, true, &d));
    if (info) memset(info, 0, sizeof *info);
    if (n == 0) return SRX_OK;
    Range rg("knn");
    const size_t ld = (size_t)scores_ld((int)m->pca.n_pc);
    KnnArgs a{m->pca.d_scores, m->pca.d_scores, n, n, ld, ld, d, true};
    return knn_device(ctx, a, opts, indices_out, distances_out, info);
}

int32_t srx_knn_points(srx_ctx* ctx, const double* ref, uint64_t n_ref, const double* query, uint64_t n_query, uint64_t d,
                       const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out, srx_knn_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (!ref && n_ref) return fail(ctx, SRX_E_ARG, "knn: null reference points");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const bool self = query == nullptr;
    if (self) n_query = n_ref;
    int du = 0;
    SRX_TRY(knn_check(ctx, opts, n_ref, n_query, d, self, &du));
    if (info) memset(info, 0, sizeof *info);
    if (n_query == 0) return SRX_OK;
    Range rg("knn");
    double *d_ref, *d_qry;
    SRX_TRY(scratch(ctx, "knn_ref_f64", n_ref * d * 8, (void**)&d_ref));
    SRX_TRY(h2d(ctx, d_ref, ref, n_ref * d * 8));
    d_qry = d_ref;
    if (!self) {
        SRX_TRY(scratch(ctx, "knn_qry_f64", n_query * d * 8, (void**)&d_qry));
        SRX_TRY(h2d(ctx, d_qry, query, n_query * d * 8));
    }
    KnnArgs a{d_ref, d_qry, n_ref, n_query, (size_t)d, (size_t)d, du, self};
    return knn_device(ctx, a, opts, indices_out, distances_out, info);
}

}  // extern "C"
