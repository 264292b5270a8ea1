// graph.hip — the weighted neighbour graph of a k-NN list (what scanpy's pp.neighbors stores as obsp["distances"] and
// obsp["connectivities"]): srx_neighbors_result / srx_neighbors_from_knn and the srx_graph handle.
//
// Definition (include/srx.h has it in full).  Row i of a self-excluding k-NN list holds k distinct neighbours j != i with
// distances d_ij >= 0; T = log2(k + 1).
//     rho_i    the smallest strictly positive distance of the row (none: rho = sigma = 0, every weight 1)
//     c_i      neighbours with d_ij <= rho_i;   S_i(s) = c_i + sum over {d_ij > rho_i} exp(-(d_ij - rho_i) / s)
//     sigma*_i the root of S_i(s) = T when c_i < T, else 0 ("no root")
//     sigma_i  max(sigma*_i, 1e-3 * sum_j d_ij / (k + 1))               ("clamped" when the floor is the larger)
//     a_ij     1 when d_ij <= rho_i, else exp(-(d_ij - rho_i) / sigma_i)
//     C        A + A^T - A o A^T, exact zeros not stored;   D[i, j] = d_ij on the k-NN edges
// This is umap-learn's fuzzy_simplicial_set (local_connectivity 1, set_op_mix_ratio 1) for rows that do not list the cell
// itself, hence k + 1 where scanpy has n_neighbors.
//
// Kernels, one wave per row unless said otherwise (k <= 64: lane p holds entry p of the row):
//   k_graph_rows      checks the list (index range, self, duplicates, distances), puts the row in column order (rank by
//                     counting across the lanes: this IS the row of D, and everything after it depends on the row as a SET),
//                     rho, c, the root by bracketing and bisection in f64 (graph_root.hpp: every sum a fixed-order butterfly),
//                     the floor, the directed weights
//   k_graph_reverse   binary search of i in row j for every edge i -> j: the reverse weight b (0 when absent), the value
//                     (a + b) - a b of the pair, whether it is stored; an edge whose reverse is absent is an IN-ONLY entry
//                     of row j and is counted there (one global atomic per such edge)
//   k_graph_rowlen    (thread per row) row length of C = stored out-edges + in-only entries; rows whose in-only list is long
//   scan_exclusive    (scan.hip) twice: the offsets of the in-only lists and the indptr of C
//   k_graph_scatter   (thread per edge) in-only entries to their row through an atomic cursor, in arbitrary order
//   k_graph_order     in-only list of a row with at most kShort entries: rank by counting in LDS, written back in place
//   k_graph_order_long  one workgroup per longer list (a hub: thousands to n - 1 entries): the sources are distinct, so a
//                     bitmap of kBits source numbers at a time with prefix popcounts gives every entry its rank
//   k_graph_merge     the row of C: out-edges (sorted, <= 64) and in-only entries (sorted, disjoint from them) each find
//                     their place by a binary search in the other list
// Whatever order the atomics ran in, every stored row is sorted by column and every value depends only on its pair: the
// result is bit-identical from call to call, and C[i, j] and C[j, i] are the same bits (fma(-a, b, a + b) is symmetric).
#include "common.hpp"
#include "graph_handle.hpp"
#include "graph_root.hpp"
#include "pca_internal.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cmath>

namespace srx {

int32_t knn_result_resident(srx_mat* m, const srx_knn_opts* opts, srx_knn_info* info, const uint32_t** d_idx,
                            const double** d_dist, uint64_t* n_out);      // knn.hip

constexpr int kGraphMaxK = 64;
constexpr int kShort = kInShort;         // in-only lists up to here are ordered by one wave in LDS
constexpr int kBits = 1 << 17;           // source numbers per pass of the long-list ordering (16 KiB bitmap + 16 KiB prefix)

__device__ __forceinline__ unsigned long long below(int p) { return p >= 64 ? ~0ull : (1ull << p) - 1ull; }
// (a + b) - a b in one rounding of the product: symmetric in a and b, 0 < result <= 1 for a, b in [0, 1] not both 0
__device__ __forceinline__ double fuzzy_union(double a, double b) { return fma(-a, b, a + b); }
// the value of a pair from its two directed weights (an absent direction is 0): symmetric in a and b for either rule
__device__ __forceinline__ double pair_value(PairRule r, double a, double b) { return r.mean ? (a + b) / r.denom : fuzzy_union(a, b); }

__global__ void __launch_bounds__(256) k_graph_rows(const uint32_t* __restrict__ idx_in, const double* __restrict__ dist_in,
                                                    uint64_t n, int k, uint64_t* __restrict__ dptr, uint32_t* __restrict__ dind,
                                                    double* __restrict__ ddat, double* __restrict__ a_out,
                                                    double* __restrict__ rho_out, double* __restrict__ sigma_out,
                                                    unsigned long long* __restrict__ ctr, int* __restrict__ flag) {
    __shared__ uint32_t s_i[4][kWave];
    __shared__ double s_d[4][kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const bool act = lane < k;
    const size_t e = (size_t)row * k + lane;
    uint32_t ci = act ? idx_in[e] : 0xFFFFFFFFu;
    double cd = act ? dist_in[e] : 0.0;
    int bad = 0;
    if (act) {
        if (ci >= n) bad |= kBadRange;
        if (ci == row) bad |= kBadSelf;
        if (!(cd >= 0.0 && cd <= kDblMax)) bad |= kBadDist;
    }
    int rank = 0;
    for (int m = 0; m < k; ++m) {
        const uint32_t o = __shfl(ci, m, kWave);
        rank += o < ci;
        if (act && m != lane && o == ci) bad |= kBadDup;
    }
    if (bad) atomicOr(flag, bad);        // the host refuses the list; what follows stays inside the row and its loops are bounded
    // the row in column order
    s_i[wave][lane] = 0xFFFFFFFFu;
    s_d[wave][lane] = 0.0;
    wave_lds_sync();
    if (act) {
        s_i[wave][rank] = ci;
        s_d[wave][rank] = cd;
    }
    wave_lds_sync();
    ci = s_i[wave][lane];
    cd = s_d[wave][lane];

    const double inf = (double)__builtin_inff();
    double rho = wave_min(act && cd > 0.0 ? cd : inf);
    const bool all_zero = !(rho < inf);
    if (all_zero) rho = 0.0;
    const bool one = act && cd <= rho, far = act && !one;
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(one));
    const double T = log2((double)(k + 1));
    const double sum_d = wave_sum(act ? cd : 0.0);
    const double x = far ? cd - rho : 0.0;
    const bool has_root = !all_zero && (double)c < T;
    double sig = 0.0;
    if (has_root) {
        // S rises from c < T (s -> 0) to k > T (s -> inf; k = T only for k = 1, where c = 1 = T)
        sig = graph_root(one, far, x, T);
    }
    const double floor_ = 1e-3 * sum_d / (double)(k + 1);
    const bool clamped = !all_zero && floor_ > sig;
    const double sigma = all_zero ? 0.0 : (clamped ? floor_ : sig);
    if (act) {
        dind[e] = ci;
        ddat[e] = cd;
        a_out[e] = far ? exp(-x / sigma) : 1.0;
    }
    if (lane == 0) {
        rho_out[row] = rho;
        sigma_out[row] = sigma;
        dptr[row] = row * (uint64_t)k;
        if (row + 1 == n) dptr[n] = n * (uint64_t)k;
        unsigned long long* my = ctr + (size_t)(row & (kCtrSlots - 1)) * kCtrN;
        if (!has_root) atomicAdd(&my[kCtrNoRoot], 1ull);
        if (clamped) atomicAdd(&my[kCtrClamped], 1ull);
        if (all_zero) atomicAdd(&my[kCtrAllZero], 1ull);
    }
}

// first position in the ascending list p[0..m) whose entry is not below key
__device__ __forceinline__ int lower_bound_u32(const uint32_t* __restrict__ p, int m, uint32_t key) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// flags: bit 0 the out-edge's entry of C is stored, bit 1 the edge is an in-only entry of its target's row
__global__ void __launch_bounds__(256) k_graph_reverse(const uint32_t* __restrict__ dind, const double* __restrict__ a_in,
                                                       uint64_t n, int k, PairRule rule, double* __restrict__ cval,
                                                       unsigned char* __restrict__ flags, int64_t* __restrict__ cnt_out,
                                                       int64_t* __restrict__ indeg, unsigned long long* __restrict__ ctr) {
    const int lane = lane_id();
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const bool act = lane < k;
    const size_t e = (size_t)row * k + lane;
    bool found = false, kept = false;
    int dropped = 0;
    if (act) {
        const uint32_t j = dind[e];
        const double a = a_in[e];
        const uint32_t* rj = dind + (size_t)j * k;
        const int q = lower_bound_u32(rj, k, (uint32_t)row);
        found = q < k && rj[q] == (uint32_t)row;
        const double b = found ? a_in[(size_t)j * k + q] : 0.0;
        const double v = pair_value(rule, a, b);
        kept = v != 0.0;
        const bool in_only = !found && kept;
        if (in_only) atomicAdd((unsigned long long*)&indeg[j], 1ull);
        // a zero that has no reverse edge is a zero of row j as well, which nobody else sees
        if (!kept) dropped = found ? 1 : 2;
        cval[e] = v;
        flags[e] = (unsigned char)((kept ? 1 : 0) | (in_only ? 2 : 0));
    }
    const int n_kept = __builtin_popcountll(__builtin_amdgcn_ballot_w64(kept));
    const int n_found = __builtin_popcountll(__builtin_amdgcn_ballot_w64(found));
    const int n_drop = wave_sum(dropped);
    if (lane == 0) {
        cnt_out[row] = n_kept;
        unsigned long long* my = ctr + (size_t)(row & (kCtrSlots - 1)) * kCtrN;
        if (n_found) atomicAdd(&my[kCtrMutual], (unsigned long long)n_found);
        if (n_drop) atomicAdd(&my[kCtrDropped], (unsigned long long)n_drop);
    }
}

// small: [0] longest row of C, [1] number of long in-only lists
__global__ void __launch_bounds__(256) k_graph_rowlen(const int64_t* __restrict__ cnt_out, const int64_t* __restrict__ indeg,
                                                      uint64_t n, int64_t* __restrict__ len, uint32_t* __restrict__ long_rows,
                                                      unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    long long l = 0;
    if (i < n) {
        l = cnt_out[i] + indeg[i];
        len[i] = l;
        if (indeg[i] > kShort) long_rows[atomicAdd(&small[1], 1ull)] = (uint32_t)i;
    }
    l = wave_max(l);
    if (lane_id() == 0 && l > 0) atomicMax(&small[0], (unsigned long long)l);
}

__global__ void __launch_bounds__(256) k_graph_scatter(const uint32_t* __restrict__ dind, const double* __restrict__ a_in,
                                                       const unsigned char* __restrict__ flags, uint64_t n_edges, int k,
                                                       const int64_t* __restrict__ tptr, unsigned long long* __restrict__ cursor,
                                                       uint32_t* __restrict__ t_src, double* __restrict__ t_val) {
    const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges || !(flags[e] & 2)) return;
    const uint32_t j = dind[e];
    const unsigned long long q = (unsigned long long)tptr[j] + atomicAdd(&cursor[j], 1ull);
    t_src[q] = (uint32_t)(e / (uint64_t)k);
    t_val[q] = a_in[e];
}

__global__ void __launch_bounds__(256) k_graph_order(const int64_t* __restrict__ tptr, uint64_t n, uint32_t* __restrict__ t_src,
                                                     double* __restrict__ t_val) {
    __shared__ uint32_t s_s[4][kShort];
    __shared__ double s_v[4][kShort];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const int64_t lo = tptr[row];
    const int64_t m64 = tptr[row + 1] - lo;
    if (m64 < 2 || m64 > kShort) return;
    const int m = (int)m64;
    for (int t = lane; t < m; t += kWave) {
        s_s[wave][t] = t_src[lo + t];
        s_v[wave][t] = t_val[lo + t];
    }
    wave_lds_sync();
    for (int t = lane; t < m; t += kWave) {
        const uint32_t key = s_s[wave][t];
        int r = 0;
        for (int u = 0; u < m; ++u) r += s_s[wave][u] < key;       // sources of a list are distinct: ranks are a permutation
        t_src[lo + r] = key;
        t_val[lo + r] = s_v[wave][t];
    }
}

// One workgroup per long list; out: the ordered list at the same offsets of a second pair of arrays.
__global__ void __launch_bounds__(256) k_graph_order_long(const int64_t* __restrict__ tptr, const uint32_t* __restrict__ long_rows,
                                                          uint64_t n, const uint32_t* __restrict__ t_src,
                                                          const double* __restrict__ t_val, uint32_t* __restrict__ o_src,
                                                          double* __restrict__ o_val) {
    constexpr int W = kBits / 32, PER = W / 256;
    __shared__ uint32_t bits[W];
    __shared__ uint32_t pre[W];
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x;
    const uint32_t row = long_rows[blockIdx.x];
    const int64_t lo = tptr[row], hi = tptr[row + 1];
    uint32_t done = 0;
    for (uint64_t base = 0; base < n; base += kBits) {
        for (int w = tid; w < W; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int64_t p = lo + tid; p < hi; p += 256) {
            const uint64_t s = (uint64_t)t_src[p] - base;        // below base: wraps to a huge number
            if (s < (uint64_t)kBits) atomicOr(&bits[s >> 5], 1u << (s & 31));
        }
        __syncthreads();
        const uint32_t total = bitmap_prefix_fill<W, PER>(bits, pre, wtot);
        __syncthreads();
        if (total)
            for (int64_t p = lo + tid; p < hi; p += 256) {
                const uint32_t src = t_src[p];
                const uint64_t s = (uint64_t)src - base;
                if (s < (uint64_t)kBits) {
                    const uint32_t r = done + bitmap_rank(bits, pre, (uint32_t)s);
                    o_src[lo + r] = src;
                    o_val[lo + r] = t_val[p];
                }
            }
        done += total;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_graph_merge(const uint32_t* __restrict__ dind, const double* __restrict__ cval,
                                                     const unsigned char* __restrict__ flags, uint64_t n, int k, PairRule rule,
                                                     const int64_t* __restrict__ tptr, const uint32_t* __restrict__ t_src,
                                                     const double* __restrict__ t_val, const uint32_t* __restrict__ l_src,
                                                     const double* __restrict__ l_val, const uint64_t* __restrict__ cptr,
                                                     uint32_t* __restrict__ cind, double* __restrict__ cdat) {
    __shared__ uint32_t s_col[4][kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const bool act = lane < k;
    const size_t e = (size_t)row * k + lane;
    const uint32_t col = act ? dind[e] : 0xFFFFFFFFu;
    const bool kept = act && (flags[e] & 1);
    const unsigned long long keptmask = __builtin_amdgcn_ballot_w64(kept);
    s_col[wave][lane] = col;
    wave_lds_sync();
    const int64_t tlo = tptr[row];
    const int m = (int)(tptr[row + 1] - tlo);
    const uint32_t* ts = (m > kShort ? l_src : t_src) + tlo;
    const double* tv = (m > kShort ? l_val : t_val) + tlo;
    const uint64_t base = cptr[row];
    if (kept) {
        const uint64_t pos = (uint64_t)__builtin_popcountll(keptmask & below(lane)) + (uint64_t)lower_bound_u32(ts, m, col);
        cind[base + pos] = col;
        cdat[base + pos] = cval[e];
    }
    for (int q = lane; q < m; q += kWave) {
        const uint32_t j = ts[q];
        const int r = lower_bound_u32(s_col[wave], k, j);          // out-edges below j (j itself is not among them)
        const uint64_t pos = (uint64_t)q + (uint64_t)__builtin_popcountll(keptmask & below(r));
        cind[base + pos] = j;
        cdat[base + pos] = pair_value(rule, tv[q], 0.0);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------

int32_t graph_alloc(srx_ctx* ctx, uint64_t n, uint32_t k, srx_graph** out) {
    srx_graph* g = new srx_graph;
    g->ctx = ctx;
    g->n = n;
    g->k = k;
    g->info.n = n;
    g->info.k = k;
    const size_t nk = (size_t)n * k;
    const size_t o_ind = up256((n + 1) * 8), o_dat = o_ind + up256(nk * 4), o_a = o_dat + up256(nk * 8), o_rho = o_a + up256(nk * 8),
                 o_sig = o_rho + up256(n * 8), total = o_sig + up256(n * 8);
    hipError_t e = hipMalloc(&g->d_block, total);
    if (e != hipSuccess) {
        delete g;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "graph: %zu bytes: %s", total, hipGetErrorString(e));
    }
    char* p = (char*)g->d_block;
    g->d_dptr = (uint64_t*)p;
    g->d_dind = (uint32_t*)(p + o_ind);
    g->d_ddat = (double*)(p + o_dat);
    g->d_a = (double*)(p + o_a);
    g->d_rho = (double*)(p + o_rho);
    g->d_sigma = (double*)(p + o_sig);
    *out = g;
    return SRX_OK;
}

int32_t graph_alloc_c(srx_graph* g, uint64_t nnz) {
    const size_t o_ind = up256((g->n + 1) * 8), o_dat = o_ind + up256(nnz * 4), total = o_dat + up256(nnz * 8);
    hipError_t e = hipMalloc(&g->d_cblock, total);
    if (e != hipSuccess)
        return fail(g->ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "graph: %zu bytes: %s", total, hipGetErrorString(e));
    char* p = (char*)g->d_cblock;
    g->d_cptr = (uint64_t*)p;
    g->d_cind = (uint32_t*)(p + o_ind);
    g->d_cdat = (double*)(p + o_dat);
    return SRX_OK;
}

// d_idx / d_dist: the k-NN list on the device (n x k row-major).  n >= 1, 1 <= k <= 64.
static int32_t graph_build(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, srx_graph** out) {
    srx_graph* g = nullptr;
    SRX_TRY(graph_alloc(ctx, n, k, &g));
    auto bail = [&](int32_t rc) {
        srx_graph_free(g);
        return rc;
    };
#define G_TRY(expr)                          \
    do {                                     \
        int32_t rc_ = (expr);                \
        if (rc_ != SRX_OK) return bail(rc_); \
    } while (0)
#define G_HIP(expr)                                                                                               \
    do {                                                                                                          \
        hipError_t e_ = (expr);                                                                                   \
        if (e_ != hipSuccess)                                                                                     \
            return bail(fail(ctx, e_ == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "%s failed: %s", #expr, hipGetErrorString(e_))); \
    } while (0)
    const size_t nk = (size_t)n * k;
    hipStream_t st = ctx->stream;
    unsigned long long* d_small;
    G_TRY(scratch(ctx, "graph_small", kPairSmallWords * 8, (void**)&d_small));
    const unsigned wg_rows = (unsigned)((n + 3) / 4);
    uint64_t ctr[kPairSmallWords];
    uint64_t nnz = 0;
    {
        // algorithmic bytes: read the list, write D; C is added once its size is known
        ProfScope ps(ctx, SRX_K_GRAPH, (double)nk * 12.0 * 2.0 + (double)(n + 1) * 16.0);
        G_HIP(hipMemsetAsync(d_small, 0, kPairSmallWords * 8, st));
        hipLaunchKernelGGL(k_graph_rows, dim3(wg_rows), dim3(256), 0, st, d_idx, d_dist, n, (int)k, g->d_dptr, g->d_dind, g->d_ddat,
                           g->d_a, g->d_rho, g->d_sigma, d_small, pair_flag(d_small));
        G_HIP(hipGetLastError());
        G_TRY(list_flag_check(ctx, "neighbors", n, pair_flag(d_small)));
        G_TRY(pair_union_csr(ctx, PairRule{0, 1.0}, g->d_dind, g->d_a, n, k, d_small, ctr, &nnz,
                             [&](uint64_t cnt, uint64_t** ptr, uint32_t** ind, double** dat) {
                                 SRX_TRY(graph_alloc_c(g, cnt));
                                 *ptr = g->d_cptr;
                                 *ind = g->d_cind;
                                 *dat = g->d_cdat;
                                 return (int32_t)SRX_OK;
                             }));
        g->info.nnz_connectivities = nnz;
        if (ps.e0) ctx->prof[SRX_K_GRAPH].bytes += (double)nnz * 12.0;
    }
    G_HIP(hipStreamSynchronize(st));
#undef G_TRY
#undef G_HIP
    uint64_t sum[kCtrN] = {0, 0, 0, 0, 0};
    for (int s = 0; s < kCtrSlots; ++s)
        for (int c = 0; c < kCtrN; ++c) sum[c] += ctr[s * kCtrN + c];
    g->info.nnz_distances = nk;
    g->info.n_mutual = sum[kCtrMutual] / 2;
    g->info.rows_no_root = sum[kCtrNoRoot];
    g->info.rows_clamped = sum[kCtrClamped];
    g->info.rows_all_zero = sum[kCtrAllZero];
    g->info.entries_dropped = sum[kCtrDropped];
    g->info.max_row_nnz = ctr[kCtrSlots * kCtrN];
    *out = g;
    return SRX_OK;
}

int32_t list_flag_check(srx_ctx* ctx, const char* who, uint64_t n, const int* d_flag) {
    int flag = 0;
    SRX_TRY(d2h(ctx, &flag, d_flag, 4));
    if (flag & kBadRange) return fail(ctx, SRX_E_ARG, "%s: a neighbour index is not below n = %llu", who, (unsigned long long)n);
    if (flag & kBadSelf) return fail(ctx, SRX_E_ARG, "%s: a row names itself (the list must exclude self)", who);
    if (flag & kBadDup) return fail(ctx, SRX_E_ARG, "%s: a row names one neighbour twice", who);
    if (flag & kBadDist) return fail(ctx, SRX_E_ARG, "%s: a distance is negative, NaN or Inf", who);
    return SRX_OK;
}

int32_t in_lists_build(srx_ctx* ctx, const uint32_t* d_dind, const double* d_val, const unsigned char* d_flags, uint64_t n,
                       uint32_t k, int64_t* d_indeg, InLists* out) {
    const size_t nk = (size_t)n * k;
    hipStream_t st = ctx->stream;
    SRX_TRY(scratch(ctx, "graph_tptr", (n + 1) * 8, (void**)&out->tptr));
    SRX_TRY(scratch(ctx, "graph_tsrc", nk * 4, (void**)&out->tsrc));
    SRX_TRY(scratch(ctx, "graph_tval", nk * 8, (void**)&out->tval));
    out->lsrc = nullptr;
    out->lval = nullptr;
    SRX_TRY(scan_exclusive(ctx, d_indeg, n, out->tptr, nullptr));
    hipLaunchKernelGGL(k_graph_scatter, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, d_dind, d_val, d_flags, (uint64_t)nk, (int)k,
                       out->tptr, reinterpret_cast<unsigned long long*>(d_indeg + n), out->tsrc, out->tval);
    hipLaunchKernelGGL(k_graph_order, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, out->tptr, n, out->tsrc, out->tval);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

int32_t in_lists_order_long(srx_ctx* ctx, uint64_t n, uint32_t k, const uint32_t* d_long, uint64_t n_long, InLists* io) {
    if (!n_long) return SRX_OK;
    const size_t nk = (size_t)n * k;
    SRX_TRY(scratch(ctx, "graph_lsrc", nk * 4, (void**)&io->lsrc));
    SRX_TRY(scratch(ctx, "graph_lval", nk * 8, (void**)&io->lval));
    hipLaunchKernelGGL(k_graph_order_long, dim3((unsigned)n_long), dim3(256), 0, ctx->stream, io->tptr, d_long, n, io->tsrc, io->tval,
                       io->lsrc, io->lval);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// The symmetric pattern of a k-NN list and its transpose with one value per pair (graph_handle.hpp): k_graph_reverse to
// k_graph_merge.  d_small: the caller's zeroed block, whose row counters and flag it may have used already.
int32_t pair_union_csr(srx_ctx* ctx, PairRule rule, const uint32_t* d_dind, const double* d_a, uint64_t n, uint32_t k,
                       unsigned long long* d_small, uint64_t* ctr, uint64_t* nnz_out, const PairAlloc& alloc) {
    const size_t nk = (size_t)n * k;
    hipStream_t st = ctx->stream;
    unsigned long long* d_ctr = d_small;
    unsigned long long* d_two = d_small + (size_t)kCtrSlots * kCtrN;
    double* d_cval;
    unsigned char* d_flags;
    int64_t *d_cnt, *d_indeg, *d_len;
    uint32_t* d_long;
    SRX_TRY(scratch(ctx, "graph_cval", nk * 8, (void**)&d_cval));
    SRX_TRY(scratch(ctx, "graph_flags", nk, (void**)&d_flags));
    SRX_TRY(scratch(ctx, "graph_cnt", n * 8, (void**)&d_cnt));
    SRX_TRY(scratch(ctx, "graph_indeg", 2 * n * 8, (void**)&d_indeg));       // in-only counts | cursors
    SRX_TRY(scratch(ctx, "graph_len", n * 8, (void**)&d_len));
    SRX_TRY(scratch(ctx, "graph_long", (nk / kShort + 1) * 4, (void**)&d_long));     // lists longer than kShort: at most nk / kShort

    const unsigned wg_rows = (unsigned)((n + 3) / 4), wg_thr = (unsigned)((n + 255) / 256);
    SRX_HIP(ctx, hipMemsetAsync(d_indeg, 0, 2 * n * 8, st));
    hipLaunchKernelGGL(k_graph_reverse, dim3(wg_rows), dim3(256), 0, st, d_dind, d_a, n, (int)k, rule, d_cval, d_flags, d_cnt, d_indeg,
                       d_ctr);
    hipLaunchKernelGGL(k_graph_rowlen, dim3(wg_thr), dim3(256), 0, st, d_cnt, d_indeg, n, d_len, d_long, d_two);
    SRX_HIP(ctx, hipGetLastError());
    InLists in;
    SRX_TRY(in_lists_build(ctx, d_dind, d_a, d_flags, n, k, d_indeg, &in));
    SRX_TRY(d2h(ctx, ctr, d_small, (kPairSmallWords - 1) * 8));
    SRX_TRY(in_lists_order_long(ctx, n, k, d_long, ctr[kCtrSlots * kCtrN + 1], &in));
    int64_t* d_tptr = in.tptr;
    uint32_t *d_tsrc = in.tsrc, *d_lsrc = in.lsrc;
    double *d_tval = in.tval, *d_lval = in.lval;
    // the indptr goes to scratch first: its last entry sizes the allocation it then moves into
    int64_t* d_cptr_tmp;
    SRX_TRY(scratch(ctx, "graph_cptr", (n + 1) * 8, (void**)&d_cptr_tmp));
    SRX_TRY(scan_exclusive(ctx, d_len, n, d_cptr_tmp, nullptr));
    int64_t nnz = 0;
    SRX_TRY(d2h(ctx, &nnz, d_cptr_tmp + n, 8));
    uint64_t* cptr = nullptr;
    uint32_t* cind = nullptr;
    double* cdat = nullptr;
    SRX_TRY(alloc((uint64_t)nnz, &cptr, &cind, &cdat));
    SRX_HIP(ctx, hipMemcpyAsync(cptr, d_cptr_tmp, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_graph_merge, dim3(wg_rows), dim3(256), 0, st, d_dind, d_cval, d_flags, n, (int)k, rule, d_tptr, d_tsrc, d_tval,
                       d_lsrc, d_lval, cptr, cind, cdat);
    SRX_HIP(ctx, hipGetLastError());
    *nnz_out = (uint64_t)nnz;
    return SRX_OK;
}

// n == 0: both matrices empty, indptr = {0}
static int32_t graph_empty(srx_ctx* ctx, uint32_t k, srx_graph** out) {
    srx_graph* g = nullptr;
    SRX_TRY(graph_alloc(ctx, 0, k, &g));
    int32_t rc = graph_alloc_c(g, 0);
    if (rc == SRX_OK && (hipMemsetAsync(g->d_dptr, 0, 8, ctx->stream) != hipSuccess ||
                         hipMemsetAsync(g->d_cptr, 0, 8, ctx->stream) != hipSuccess))
        rc = fail(ctx, SRX_E_HIP, "graph: hipMemsetAsync failed");
    if (rc != SRX_OK) {
        srx_graph_free(g);
        return rc;
    }
    *out = g;
    return SRX_OK;
}

// The graph of a k-NN list that lies on the device (n x k row-major, no row names itself): what srx_neighbors_result does
// with the list of knn_result_resident, for the other holders of such a list (harmony.hip).
int32_t graph_from_device_list(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, srx_graph** out) {
    Range rg("graph");
    if (n == 0) return graph_empty(ctx, k, out);
    return graph_build(ctx, d_idx, d_dist, n, k, out);
}

int32_t keep_on_handle(srx_ctx* ctx, double** slot, bool resized, const double* d_src, size_t bytes) {
    if (*slot && resized) {
        SRX_HIP(ctx, hipFree(*slot));
        *slot = nullptr;
    }
    if (!*slot) SRX_HIP(ctx, hipMalloc((void**)slot, bytes));
    SRX_HIP(ctx, hipMemcpyAsync(*slot, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_neighbors_result(srx_mat* m, const srx_knn_opts* opts, srx_knn_info* knn_info, srx_graph** out) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "neighbors: null output handle");
    *out = nullptr;
    if (!opts) return fail(ctx, SRX_E_ARG, "neighbors: null options");
    if (opts->include_self) return fail(ctx, SRX_E_ARG, "neighbors: the graph is built from a list that excludes self (include_self = 0)");
    const uint32_t* d_idx = nullptr;
    const double* d_dist = nullptr;
    uint64_t n = 0;
    SRX_TRY(knn_result_resident(m, opts, knn_info, &d_idx, &d_dist, &n));
    Range rg("graph");
    if (n == 0) return graph_empty(ctx, (uint32_t)opts->k, out);
    return graph_build(ctx, d_idx, d_dist, n, (uint32_t)opts->k, out);
}

int32_t srx_neighbors_from_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                               srx_graph** out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (!out) return fail(ctx, SRX_E_ARG, "neighbors: null output handle");
    *out = nullptr;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "neighbors: rows are sharded; the graph needs all cells");
    if (k < 1 || k > (uint32_t)kGraphMaxK) return fail(ctx, SRX_E_ARG, "neighbors: k = %u outside 1..%d", k, kGraphMaxK);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return graph_empty(ctx, k, out);
    if (!indices || !distances) return fail(ctx, SRX_E_ARG, "neighbors: null k-NN list");
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "neighbors: more than 2^32 - 2 cells");
    if ((uint64_t)k > n - 1) return fail(ctx, SRX_E_ARG, "neighbors: k = %u but a cell has only %llu others", k, (unsigned long long)(n - 1));
    Range rg("graph");
    uint32_t* d_idx;
    double* d_dist;
    SRX_TRY(scratch(ctx, "graph_in_idx", n * k * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "graph_in_dist", n * k * 8, (void**)&d_dist));
    SRX_TRY(h2d(ctx, d_idx, indices, n * k * 4));
    SRX_TRY(h2d(ctx, d_dist, distances, n * k * 8));
    return graph_build(ctx, d_idx, d_dist, n, k, out);
}

int32_t srx_graph_info_get(const srx_graph* g, srx_graph_info* info) {
    if (!g || !info) return fail(g ? g->ctx : nullptr, SRX_E_ARG, "null argument");
    *info = g->info;
    return SRX_OK;
}

int32_t srx_graph_fetch(srx_graph* g, int32_t which, uint64_t* indptr, uint32_t* indices, double* data) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (which != SRX_GRAPH_DISTANCES && which != SRX_GRAPH_CONNECTIVITIES)
        return fail(ctx, SRX_E_ARG, "srx_graph_fetch: which = %d is neither distances nor connectivities", which);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const bool c = which == SRX_GRAPH_CONNECTIVITIES;
    const uint64_t nnz = c ? g->info.nnz_connectivities : g->info.nnz_distances;
    if (indptr) SRX_TRY(d2h(ctx, indptr, c ? g->d_cptr : g->d_dptr, (g->n + 1) * 8));
    if (indices) SRX_TRY(d2h(ctx, indices, c ? g->d_cind : g->d_dind, nnz * 4));
    if (data) SRX_TRY(d2h(ctx, data, c ? g->d_cdat : g->d_ddat, nnz * 8));
    return SRX_OK;
}

int32_t srx_graph_fetch_scales(srx_graph* g, double* rho, double* sigma) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (rho) SRX_TRY(d2h(ctx, rho, g->d_rho, g->n * 8));
    if (sigma) SRX_TRY(d2h(ctx, sigma, g->d_sigma, g->n * 8));
    return SRX_OK;
}

void srx_graph_free(srx_graph* g) {
    if (!g) return;
    if (g->d_block || g->d_cblock || g->d_labels || g->d_embed || g->d_dm_t || g->d_dm_evecs || g->d_layout) {
        (void)hipSetDevice(g->ctx->device);
        (void)hipStreamSynchronize(g->ctx->stream);
        if (g->d_block) (void)hipFree(g->d_block);
        if (g->d_cblock) (void)hipFree(g->d_cblock);
        if (g->d_labels) (void)hipFree(g->d_labels);
        if (g->d_embed) (void)hipFree(g->d_embed);
        if (g->d_dm_t) (void)hipFree(g->d_dm_t);
        if (g->d_dm_evecs) (void)hipFree(g->d_dm_evecs);
        if (g->d_layout) (void)hipFree(g->d_layout);
    }
    delete g;
}

}  // extern "C"
