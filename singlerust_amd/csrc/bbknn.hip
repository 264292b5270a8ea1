// bbknn.hip — batch-balanced neighbours (BBKNN) and the trimming of a graph's connectivities: srx_bbknn_result / srx_bbknn_points
// / srx_graph_trim here, srx_bbknn_harmony in harmony.hip through bbknn_device.  include/srx.h has the definition in full.
//
// The list.  The rows are sorted by batch (label_sort_count / label_sort_place: a stable counting sort, so a batch becomes
// the contiguous block [o_b, o_b + n_b) of places and keeps the order of its points), k_bb_gather copies the used coordinates
// into one block in that order, and every batch b is searched by knn_device over at most three DISJOINT query ranges:
//   places [0, o_b)            against block b, k_within           (queries of lower batches)
//   block b against itself     as a self graph, k_within - 1       (skipped when k_within = 1)
//   places [o_b + n_b, n)      against block b, k_within           (queries of higher batches)
// n n_b distance pairs per batch, n^2 over all (n^2 - sum n_b^2 with k_within = 1); no cell meets its own block twice.  One
// masked search of all points would have to keep k_within B candidates per row and batch-aware thresholds in the candidate
// pass; the ranges reuse the exact search as it is, certificate included.  The sort is stable, so the block-local index order is
// the order of the original indices and the search's tie rule is the definition's.
// k_bb_merge runs after each search, stream-ordered before the next one reuses the "knn_idx" / "knn_dist" slots: it copies the
// search's columns to the row's slot range of the n x K list, block-local reference indices mapped to point ids through the
// permutation, sorted query places back to their rows.  k_bb_sort_rows (a wave per row, lane p holds entry p, rank by counting
// as knn_take does) then orders each row by (distance, index).  graph_from_device_list builds the graph, unchanged.
//
// Trimming (trim_c).  Values are compared through u64 keys in the order of the doubles.
//   k_trim_mark    (thread per row) rows with L_i > trim are compacted into one list per selection route (one integer atomic per
//                  wave and route); every other row gets t_i = 0.  At the default trim almost no row is marked.
//   k_trim_select_wave   L_i <= kTrimWaveCap: a wave per row, the row's keys in registers
//   k_trim_select_block<true>   L_i <= kTrimBlockCap: a workgroup per row, the keys cached in LDS
//   k_trim_select_block<false>  beyond: a workgroup per row that reads the row from global memory every round
//                  All three are a radix select from the top byte down: a 256-bin histogram in LDS of the keys that match the
//                  prefix so far (integer atomics), then one wave walks the bins from 255 down to the one that holds the
//                  trim-th largest.  Eight rounds give the key itself: exact, whatever the order of the entries.
//   k_trim_filter<false>  (wave per row) counts the entries with c >= t_i and c >= t_j; scan_exclusive makes the indptr;
//   k_trim_filter<true>   writes them, in order, into the new C block (graph_alloc_c).
// The counters of srx_trim_info are integer sums and maxima.
#include "common.hpp"
#include "graph_handle.hpp"
#include "knn_internal.hpp"
#include "markers_internal.hpp"
#include "scan.hpp"

#include <algorithm>

namespace srx {

int32_t graph_from_device_list(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, srx_graph** out);   // graph.hip
int scores_ld(int n_pc);                                                                                                             // pca_solve.hip

constexpr int kBbMaxK = 64;
constexpr uint32_t kTrimWaveCap = 512;             // 8 keys per lane
constexpr uint32_t kTrimBlockCap = 4096;           // 32 KiB of keys in LDS
constexpr int kTrimPerLane = (int)(kTrimWaveCap / kWave);
// the small block of a trim: the three route counts | the longest row before and after | rows emptied
enum { kTrWave = 0, kTrShort, kTrLong, kTrMaxBefore, kTrMaxAfter, kTrEmptied, kTrWords };

__device__ __forceinline__ unsigned long long below_lane(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ void max_to(unsigned long long* p, unsigned long long v) {
    if (v > *(volatile unsigned long long*)p) atomicMax(p, v);
}

// ---- the list ----------------------------------------------------------------------------------------------------------------

// out[p * d + c] = pts[perm[p] * ld + c]: the used coordinates in sorted order
__global__ void __launch_bounds__(256) k_bb_gather(const double* __restrict__ pts, size_t ld, const uint32_t* __restrict__ perm, uint64_t n,
                                                   int d, double* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * (uint64_t)d) return;
    const uint64_t p = t / (uint64_t)d;
    const int c = (int)(t - p * (uint64_t)d);
    out[t] = pts[(size_t)perm[p] * ld + c];
}

// One search's columns (nq x ks, queries = the places from q0, references = the places from o_b) into columns [slot, slot + ks)
// of the list rows of the queries' points.
__global__ void __launch_bounds__(256) k_bb_merge(const uint32_t* __restrict__ kidx, const double* __restrict__ kdist, uint64_t nq, int ks,
                                                  const uint32_t* __restrict__ perm, uint64_t q0, uint64_t o_b, int slot, int K,
                                                  uint32_t* __restrict__ lidx, double* __restrict__ ldist) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nq * (uint64_t)ks) return;
    const uint64_t q = t / (uint64_t)ks;
    const int c = (int)(t - q * (uint64_t)ks);
    const size_t dst = (size_t)perm[q0 + q] * K + slot + c;
    lidx[dst] = perm[o_b + kidx[t]];
    ldist[dst] = kdist[t];
}

// A wave per row: lane p holds entry p, its rank is the number of entries before it in (distance, index) order.  The indices of
// a row are distinct, so the ranks are a permutation; every lane has read its entry before any lane writes (the shuffles).
__global__ void __launch_bounds__(256) k_bb_sort_rows(uint32_t* __restrict__ lidx, double* __restrict__ ldist, uint64_t n, int K) {
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    const bool act = lane < K;
    const size_t base = (size_t)row * K;
    const double dd = act ? ldist[base + lane] : 0.0;
    const uint32_t ii = act ? lidx[base + lane] : 0u;
    int r = 0;
    for (int m = 0; m < K; ++m) {
        const double dm = __shfl(dd, m, kWave);
        const uint32_t im = __shfl(ii, m, kWave);
        r += knn_less(dm, im, dd, ii);
    }
    if (act) {
        lidx[base + r] = ii;
        ldist[base + r] = dd;
    }
}

// ---- trimming ----------------------------------------------------------------------------------------------------------------

// f64 -> u64 with the same order (the stored values are positive; the map holds for every double that is no NaN)
__device__ __forceinline__ uint64_t trim_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double trim_val(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__global__ void __launch_bounds__(256) k_trim_mark(const uint64_t* __restrict__ cptr, uint64_t n, uint64_t trim, double* __restrict__ thr,
                                                   uint32_t* __restrict__ rows_wave, uint32_t* __restrict__ rows_short,
                                                   uint32_t* __restrict__ rows_long, unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = lane_id();
    unsigned long long L = 0;
    int route = -1;
    if (i < n) {
        L = cptr[i + 1] - cptr[i];
        thr[i] = 0.0;
        if (L > trim) route = L <= kTrimWaveCap ? kTrWave : L <= kTrimBlockCap ? kTrShort : kTrLong;
    }
    for (int r = kTrWave; r <= kTrLong; ++r) {
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(route == r);
        if (mask == 0ull) continue;                        // wave-uniform
        const int leader = __builtin_ctzll(mask);
        unsigned long long at = 0;
        if (lane == leader) at = atomicAdd(&small[r], (unsigned long long)__builtin_popcountll(mask));
        at = __shfl(at, leader, kWave);
        uint32_t* list = r == kTrWave ? rows_wave : r == kTrShort ? rows_short : rows_long;
        if (route == r) list[at + (unsigned long long)__builtin_popcountll(mask & below_lane(lane))] = (uint32_t)i;
    }
    const unsigned long long Lmax = wave_max(L);
    if (lane == 0 && Lmax) max_to(&small[kTrMaxBefore], Lmax);
}

// One FULL wave: hist (LDS, 256 bins, visible to the wave) counts the keys that match the prefix by their next byte, and at
// least krem >= 1 of them exist.  Lane l takes the bins 255 - 4 l downwards, so that the inclusive scan over the lanes counts
// from the top.  Returns the bin that holds the krem-th largest and lowers krem by the keys in the bins above it.
__device__ __forceinline__ uint32_t trim_pick(const uint32_t* hist, uint32_t& krem) {
    const int lane = lane_id();
    uint32_t c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = hist[255 - 4 * lane - j];
        s += c[j];
    }
    const uint32_t inc = wave_scan_inclusive(s);
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(inc >= krem);
    if (mask == 0ull) return 0u;                           // (fewer than krem keys: the contract excludes it)
    const int src = __builtin_ctzll(mask);
    uint32_t bin = 0, kr = 0, before = inc - s;
    if (lane == src) {
        bool found = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (!found && before + c[j] >= krem) {
                bin = (uint32_t)(255 - 4 * lane - j);
                kr = krem - before;
                found = true;
            }
            if (!found) before += c[j];
        }
    }
    krem = __shfl(kr, src, kWave);
    return __shfl(bin, src, kWave);
}

// rows[w]: a row with trim < L <= kTrimWaveCap
__global__ void __launch_bounds__(256) k_trim_select_wave(const uint64_t* __restrict__ cptr, const double* __restrict__ cdat,
                                                          const uint32_t* __restrict__ rows, uint64_t n_rows, uint32_t trim,
                                                          double* __restrict__ thr) {
    __shared__ uint32_t s_hist[4][256];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t w = global_wave_id();
    if (w >= n_rows) return;
    const uint32_t row = rows[w];
    const uint64_t lo = cptr[row];
    const uint32_t L = (uint32_t)(cptr[row + 1] - lo);
    uint64_t key[kTrimPerLane];
#pragma unroll
    for (int j = 0; j < kTrimPerLane; ++j) {
        const uint32_t e = (uint32_t)lane + 64u * j;
        key[j] = e < L ? trim_key(cdat[lo + e]) : 0ull;
    }
    uint32_t* hist = s_hist[wave];
    uint64_t prefix = 0;
    uint32_t krem = trim;
    for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) hist[lane * 4 + j] = 0u;
        wave_lds_sync();
        const uint64_t hi = shift == 56 ? 0ull : ~0ull << (shift + 8);
#pragma unroll
        for (int j = 0; j < kTrimPerLane; ++j) {
            const uint32_t e = (uint32_t)lane + 64u * j;
            if (e < L && (key[j] & hi) == prefix) atomicAdd(&hist[(uint32_t)(key[j] >> shift) & 255u], 1u);
        }
        wave_lds_sync();
        prefix |= (uint64_t)trim_pick(hist, krem) << shift;
        wave_lds_sync();
    }
    if (lane == 0) thr[row] = trim_val(prefix);
}

// rows[blockIdx.x]: a row with L > max(trim, kTrimWaveCap); CACHED: L <= kTrimBlockCap
template <bool CACHED>
__global__ void __launch_bounds__(256) k_trim_select_block(const uint64_t* __restrict__ cptr, const double* __restrict__ cdat,
                                                           const uint32_t* __restrict__ rows, uint32_t trim, double* __restrict__ thr) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint64_t s_keys[CACHED ? kTrimBlockCap : 1];
    __shared__ uint32_t s_pick[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t row = rows[blockIdx.x];
    const uint64_t lo = cptr[row];
    const uint64_t L = cptr[row + 1] - lo;
    if (CACHED)
        for (uint64_t i = tid; i < L; i += 256) s_keys[i] = trim_key(cdat[lo + i]);
    uint64_t prefix = 0;
    uint32_t krem = trim;
    for (int shift = 56; shift >= 0; shift -= 8) {
        s_hist[tid] = 0u;
        __syncthreads();
        const uint64_t hi = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (uint64_t i = tid; i < L; i += 256) {
            const uint64_t key = CACHED ? s_keys[i] : trim_key(cdat[lo + i]);
            if ((key & hi) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < (uint32_t)kWave) {
            uint32_t kr = krem;
            const uint32_t bin = trim_pick(s_hist, kr);
            if (tid == 0) {
                s_pick[0] = bin;
                s_pick[1] = kr;
            }
        }
        __syncthreads();               // the next round's writes of s_hist and s_pick follow this barrier and the next two
        prefix |= (uint64_t)s_pick[0] << shift;
        krem = s_pick[1];
    }
    if (tid == 0) thr[row] = trim_val(prefix);
}

// A wave per row: the entries with c >= t_i and c >= t_j, counted (len) or written in order from optr[row]
template <bool FILL>
__global__ void __launch_bounds__(256) k_trim_filter(const uint64_t* __restrict__ cptr, const uint32_t* __restrict__ cind,
                                                     const double* __restrict__ cdat, const double* __restrict__ thr, uint64_t n,
                                                     int64_t* __restrict__ len, const uint64_t* __restrict__ optr,
                                                     uint32_t* __restrict__ oind, double* __restrict__ odat,
                                                     unsigned long long* __restrict__ small) {
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const int lane = lane_id();
    const uint64_t lo = cptr[row], hi = cptr[row + 1];
    const double ti = thr[row];
    uint64_t kept = 0;
    uint64_t obase = 0;
    if constexpr (FILL) obase = optr[row];
    for (uint64_t e0 = lo; e0 < hi; e0 += 64) {
        const uint64_t e = e0 + lane;
        bool keep = false;
        uint32_t j = 0;
        double c = 0.0;
        if (e < hi) {
            j = cind[e];
            c = cdat[e];
            keep = c >= ti && c >= thr[j];
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
        if constexpr (FILL) {
            if (keep) {
                const uint64_t pos = obase + kept + (uint64_t)__builtin_popcountll(mask & below_lane(lane));
                oind[pos] = j;
                odat[pos] = c;
            }
        }
        kept += (uint64_t)__builtin_popcountll(mask);
    }
    if constexpr (!FILL) {
        if (lane == 0) {
            len[row] = (int64_t)kept;
            if (kept) max_to(&small[kTrMaxAfter], kept);
            else if (hi > lo) atomicAdd(&small[kTrEmptied], 1ull);
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------

// The trimmed form of c (n >= 1 rows) into a C block allocated on dst (dst->n == c.n, dst->d_cblock null on entry); trim >= 1.
// Sets dst's nnz_connectivities and max_row_nnz.  On an error the caller frees dst.
static int32_t trim_c(srx_ctx* ctx, SymCsr c, uint64_t trim, srx_graph* dst, srx_trim_info* info) {
    const uint64_t n = c.n;
    hipStream_t st = ctx->stream;
    unsigned long long* d_small;
    double* d_thr;
    uint32_t* d_rows;
    int64_t *d_len, *d_cptr_tmp;
    SRX_TRY(scratch(ctx, "trim_small", kTrWords * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "trim_thr", n * 8, (void**)&d_thr));
    SRX_TRY(scratch(ctx, "trim_rows", 3 * n * 4, (void**)&d_rows));
    SRX_TRY(scratch(ctx, "trim_len", n * 8, (void**)&d_len));
    SRX_TRY(scratch(ctx, "trim_cptr", (n + 1) * 8, (void**)&d_cptr_tmp));
    uint32_t *d_rw = d_rows, *d_rs = d_rows + n, *d_rl = d_rows + 2 * n;
    memset(info, 0, sizeof *info);
    info->trim = trim;
    info->wave_capacity = kTrimWaveCap;
    info->short_capacity = kTrimBlockCap;
    info->nnz_before = c.nnz;

    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, kTrWords * 8, st));
    hipLaunchKernelGGL(k_trim_mark, dim3(grid256(n)), dim3(256), 0, st, c.ptr, n, trim, d_thr, d_rw, d_rs, d_rl, d_small);
    SRX_HIP(ctx, hipGetLastError());
    unsigned long long sm[kTrWords];
    SRX_TRY(d2h(ctx, sm, d_small, sizeof sm));
    // a marked row has trim < L < 2^32: the rank fits 32 bits
    const uint32_t t32 = (uint32_t)std::min<uint64_t>(trim, 0xFFFFFFFFull);
    if (sm[kTrWave])
        hipLaunchKernelGGL(k_trim_select_wave, dim3((unsigned)((sm[kTrWave] + 3) / 4)), dim3(256), 0, st, c.ptr, c.w, (const uint32_t*)d_rw,
                           (uint64_t)sm[kTrWave], t32, d_thr);
    if (sm[kTrShort])
        hipLaunchKernelGGL(k_trim_select_block<true>, dim3((unsigned)sm[kTrShort]), dim3(256), 0, st, c.ptr, c.w, (const uint32_t*)d_rs, t32,
                           d_thr);
    if (sm[kTrLong])
        hipLaunchKernelGGL(k_trim_select_block<false>, dim3((unsigned)sm[kTrLong]), dim3(256), 0, st, c.ptr, c.w, (const uint32_t*)d_rl, t32,
                           d_thr);
    const unsigned wg_rows = (unsigned)((n + 3) / 4);
    hipLaunchKernelGGL(k_trim_filter<false>, dim3(wg_rows), dim3(256), 0, st, c.ptr, c.ind, c.w, (const double*)d_thr, n, d_len,
                       (const uint64_t*)nullptr, (uint32_t*)nullptr, (double*)nullptr, d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(scan_exclusive(ctx, d_len, n, d_cptr_tmp, nullptr));
    int64_t nnz = 0;
    SRX_TRY(d2h(ctx, &nnz, d_cptr_tmp + n, 8));
    SRX_TRY(graph_alloc_c(dst, (uint64_t)nnz));
    SRX_HIP(ctx, hipMemcpyAsync(dst->d_cptr, d_cptr_tmp, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_trim_filter<true>, dim3(wg_rows), dim3(256), 0, st, c.ptr, c.ind, c.w, (const double*)d_thr, n, (int64_t*)nullptr,
                       (const uint64_t*)dst->d_cptr, dst->d_cind, dst->d_cdat, d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(d2h(ctx, sm, d_small, sizeof sm));
    info->rows_wave = sm[kTrWave];
    info->rows_short = sm[kTrShort];
    info->rows_long = sm[kTrLong];
    info->rows_over_trim = sm[kTrWave] + sm[kTrShort] + sm[kTrLong];
    info->nnz_after = (uint64_t)nnz;
    info->entries_trimmed = c.nnz - (uint64_t)nnz;
    info->max_row_nnz_before = sm[kTrMaxBefore];
    info->max_row_nnz_after = sm[kTrMaxAfter];
    info->rows_emptied = sm[kTrEmptied];
    dst->info.nnz_connectivities = (uint64_t)nnz;
    dst->info.max_row_nnz = sm[kTrMaxAfter];
    return SRX_OK;
}

// The C block of g replaced by its trimmed form.  A graph without a row over trim keeps its block: every threshold is 0.
static int32_t trim_in_place(srx_ctx* ctx, srx_graph* g, uint64_t trim, srx_trim_info* info) {
    if (g->info.max_row_nnz <= trim) {
        memset(info, 0, sizeof *info);
        info->trim = trim;
        info->wave_capacity = kTrimWaveCap;
        info->short_capacity = kTrimBlockCap;
        info->nnz_before = info->nnz_after = g->info.nnz_connectivities;
        info->max_row_nnz_before = info->max_row_nnz_after = g->info.max_row_nnz;
        return SRX_OK;
    }
    const SymCsr c = connectivities(g);
    void* old = g->d_cblock;
    g->d_cblock = nullptr;
    const int32_t rc = trim_c(ctx, c, trim, g, info);
    if (rc != SRX_OK) {
        if (g->d_cblock) (void)hipFree(g->d_cblock);
        g->d_cblock = old;               // the caller frees the handle
        return rc;
    }
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    SRX_HIP(ctx, hipFree(old));
    return SRX_OK;
}

static const srx_bbknn_opts kBbDefaults = {0, 0, -1};

// The whole of BBKNN on n points with pitch ld (doubles) and d_full coordinates; batch: n host labels.  The points lie on the
// device at d_pts, or on the host at h_pts (d_pts null): those are uploaded once the arguments have passed.
int32_t bbknn_device(srx_ctx* ctx, const double* d_pts, const double* h_pts, size_t ld, uint64_t n, uint64_t d_full, const uint32_t* batch, uint32_t B,
                     const srx_bbknn_opts* opts, uint32_t* indices_out, double* distances_out, srx_bbknn_info* info_out,
                     srx_graph** out) {
    if (out) *out = nullptr;
    const srx_bbknn_opts* o = opts ? opts : &kBbDefaults;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "bbknn: rows are sharded; neighbours need all cells");
    const int64_t kw = o->neighbors_within_batch == 0 ? 3 : o->neighbors_within_batch;
    if (kw < 1) return fail(ctx, SRX_E_ARG, "bbknn: neighbors_within_batch = %d is below 1", o->neighbors_within_batch);
    if (B < 1 || B > (uint32_t)kBbMaxK + 1) return fail(ctx, SRX_E_ARG, "bbknn: n_batches = %u is outside 1 .. %d", B, kBbMaxK + 1);
    const int64_t K64 = kw * (int64_t)B - 1;
    if (K64 < 1 || K64 > kBbMaxK)
        return fail(ctx, SRX_E_ARG,
                    "bbknn: K = neighbors_within_batch * n_batches - 1 = %lld is outside 1 .. %d, the limit of every list consumer "
                    "(3 neighbours per batch allow 21 batches)",
                    (long long)K64, kBbMaxK);
    const int K = (int)K64, k_within = (int)kw;
    if (n && !batch && B != 1) return fail(ctx, SRX_E_ARG, "bbknn: null batch labels with n_batches = %u", B);
    srx_knn_opts ko{k_within, o->n_dims, 0, 0};
    int d = 0;
    SRX_TRY(knn_check(ctx, &ko, n, 0, d_full, false, &d));       // d, n_dims, n < 2^32 - 1
    srx_bbknn_info info;
    memset(&info, 0, sizeof info);
    info.n = n;
    info.n_batches = B;
    info.neighbors_within_batch = (uint32_t)k_within;
    info.k = (uint32_t)K;
    info.d = (uint32_t)d;
    const uint64_t trim = o->trim < 0 ? (uint64_t)(10 * kw * (int64_t)B) : (uint64_t)o->trim;
    info.trim.trim = trim;
    info.trim.wave_capacity = kTrimWaveCap;
    info.trim.short_capacity = kTrimBlockCap;
    if (n == 0) {
        if (out) SRX_TRY(graph_from_device_list(ctx, nullptr, nullptr, 0, (uint32_t)K, out));
        if (info_out) *info_out = info;
        return SRX_OK;
    }
    Range rg("bbknn");
    hipStream_t st = ctx->stream;
    if (!d_pts) {
        double* up;
        SRX_TRY(scratch(ctx, "bbknn_pts", n * ld * 8, (void**)&up));
        SRX_TRY(h2d(ctx, up, h_pts, n * ld * 8));
        d_pts = up;
    }
    StreamTimer t_all(ctx, st);
    SRX_TRY(t_all.start());

    // rows by batch
    uint32_t* d_labels;
    if (batch) SRX_TRY(host_labels(ctx, n, batch, B, "bbknn", &d_labels));
    else {
        SRX_TRY(scratch(ctx, "mk_labels", n * 4, (void**)&d_labels));
        SRX_HIP(ctx, hipMemsetAsync(d_labels, 0, n * 4, st));
    }
    unsigned long long* d_small;
    uint64_t* d_sizes;
    double* d_sorted;
    uint32_t *d_lidx, *d_kidx;
    double *d_ldist, *d_kdist;
    SRX_TRY(scratch(ctx, "mk_small", MK_WORDS * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "bbknn_sizes", (size_t)B * 8, (void**)&d_sizes));
    SRX_TRY(scratch(ctx, "bbknn_sorted", n * (size_t)d * 8, (void**)&d_sorted));
    SRX_TRY(scratch(ctx, "bbknn_idx", n * (size_t)K * 4, (void**)&d_lidx));
    SRX_TRY(scratch(ctx, "bbknn_dist", n * (size_t)K * 8, (void**)&d_ldist));
    // the two slots the searches write, at their largest size: no search below re-allocates them under a merge
    SRX_TRY(scratch(ctx, "knn_idx", n * (size_t)k_within * 4, (void**)&d_kidx));
    SRX_TRY(scratch(ctx, "knn_dist", n * (size_t)k_within * 8, (void**)&d_kdist));
    std::vector<uint64_t> sizes(B);
    LabelSort sort;
    {
        StreamTimer t(ctx, st);
        SRX_TRY(t.start());
        SRX_HIP(ctx, hipMemsetAsync(d_small, 0, MK_WORDS * 8, st));
        SRX_TRY(label_sort_count(ctx, d_labels, n, B, d_small, d_sizes, &sort));
        unsigned long long small[MK_WORDS];
        SRX_TRY(d2h(ctx, small, d_small, sizeof small));
        if (small[MK_FLAGS] & kMkBadLabel) return fail(ctx, SRX_E_ARG, "bbknn: a batch label is not below n_batches = %u", B);
        SRX_TRY(d2h(ctx, sizes.data(), d_sizes, (size_t)B * 8));
        info.min_batch_cells = *std::min_element(sizes.begin(), sizes.end());
        info.max_batch_cells = *std::max_element(sizes.begin(), sizes.end());
        for (uint32_t b = 0; b < B; ++b)
            if (sizes[b] < (uint64_t)k_within)
                return fail(ctx, SRX_E_ARG, "bbknn: batch %u has %llu points, fewer than neighbors_within_batch = %d", b,
                            (unsigned long long)sizes[b], k_within);
        SRX_TRY(label_sort_place(ctx, d_labels, sort));
        hipLaunchKernelGGL(k_bb_gather, dim3(grid256(n * (uint64_t)d)), dim3(256), 0, st, d_pts, ld, (const uint32_t*)sort.d_perm, n, d,
                           d_sorted);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(t.stop(&info.ms_sort));
    }
    const uint32_t* d_perm = sort.d_perm;

    // the searches, each followed by its merge
    uint64_t o_b = 0;
    for (uint32_t b = 0; b < B; ++b) {
        const uint64_t n_b = sizes[b];
        struct Part {
            uint64_t q0, nq;
            int ks, slot;
            bool self;
        };
        const Part parts[3] = {{0, o_b, k_within, (int)b * k_within - 1, false},
                               {o_b, k_within > 1 ? n_b : 0, k_within - 1, (int)b * k_within, true},
                               {o_b + n_b, n - o_b - n_b, k_within, (int)b * k_within, false}};
        for (const Part& p : parts) {
            if (p.nq == 0) continue;
            srx_knn_opts so{p.ks, 0, 0, 0};
            srx_knn_info ki;
            KnnArgs a{d_sorted + o_b * (size_t)d, d_sorted + p.q0 * (size_t)d, n_b, p.nq, (size_t)d, (size_t)d, d, p.self};
            double ms = 0.0;
            {
                StreamTimer t(ctx, st);
                SRX_TRY(t.start());
                SRX_TRY(knn_device(ctx, a, &so, nullptr, nullptr, &ki));
                SRX_TRY(t.stop(&ms));
            }
            info.ms_search += ms;
            info.n_searches++;
            info.pairs_searched += p.nq * n_b;
            info.rows_certified += ki.rows_certified;
            info.rows_recomputed += ki.rows_recomputed;
            {
                StreamTimer t(ctx, st);
                SRX_TRY(t.start());
                hipLaunchKernelGGL(k_bb_merge, dim3(grid256(p.nq * (uint64_t)p.ks)), dim3(256), 0, st, (const uint32_t*)d_kidx,
                                   (const double*)d_kdist, p.nq, p.ks, d_perm, p.q0, o_b, p.slot, K, d_lidx, d_ldist);
                SRX_HIP(ctx, hipGetLastError());
                SRX_TRY(t.stop(&ms));
            }
            info.ms_merge += ms;
        }
        o_b += n_b;
    }
    {
        double ms = 0.0;
        StreamTimer t(ctx, st);
        SRX_TRY(t.start());
        hipLaunchKernelGGL(k_bb_sort_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_lidx, d_ldist, n, K);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(t.stop(&ms));
        info.ms_merge += ms;
    }
    if (indices_out) SRX_TRY(d2h(ctx, indices_out, d_lidx, n * (size_t)K * 4));
    if (distances_out) SRX_TRY(d2h(ctx, distances_out, d_ldist, n * (size_t)K * 8));

    srx_graph* g = nullptr;
    if (out) {
        {
            StreamTimer t(ctx, st);
            SRX_TRY(t.start());
            SRX_TRY(graph_from_device_list(ctx, d_lidx, d_ldist, n, (uint32_t)K, &g));
            const int32_t rc = t.stop(&info.ms_graph);
            if (rc != SRX_OK) {
                srx_graph_free(g);
                return rc;
            }
        }
        if (trim) {
            StreamTimer t(ctx, st);
            int32_t rc = t.start();
            if (rc == SRX_OK) rc = trim_in_place(ctx, g, trim, &info.trim);
            if (rc == SRX_OK) rc = t.stop(&info.ms_trim);
            if (rc != SRX_OK) {
                srx_graph_free(g);
                return rc;
            }
        } else {
            info.trim.nnz_before = info.trim.nnz_after = g->info.nnz_connectivities;
            info.trim.max_row_nnz_before = info.trim.max_row_nnz_after = g->info.max_row_nnz;
        }
    }
    const int32_t rc = t_all.stop(&info.ms);
    if (rc != SRX_OK) {
        srx_graph_free(g);
        return rc;
    }
    if (out) *out = g;
    if (info_out) *info_out = info;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_bbknn_result(srx_mat* m, const uint32_t* batch, uint32_t n_batches, const srx_bbknn_opts* opts, srx_bbknn_info* info,
                         srx_graph** out) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "bbknn: null output handle");
    *out = nullptr;
    if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "no PCA result on this matrix");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = m->csc ? m->n_cols : m->n_rows;      // cells: the column axis of a CSC handle (as srx_knn_result)
    return bbknn_device(ctx, m->pca.d_scores, nullptr, (size_t)scores_ld((int)m->pca.n_pc), n, m->pca.n_pc, batch, n_batches, opts, nullptr, nullptr,
                        info, out);
}

int32_t srx_bbknn_points(srx_ctx* ctx, const double* points, uint64_t n, uint64_t d, const uint32_t* batch, uint32_t n_batches,
                         const srx_bbknn_opts* opts, uint32_t* indices_out, double* distances_out, srx_bbknn_info* info,
                         srx_graph** out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (out) *out = nullptr;
    if (!points && n) return fail(ctx, SRX_E_ARG, "bbknn: null points");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return bbknn_device(ctx, nullptr, points, (size_t)d, n, d, batch, n_batches, opts, indices_out, distances_out, info, out);
}

int32_t srx_graph_trim(srx_graph* g, int64_t trim, srx_trim_info* info_out, srx_graph** out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "trim: null graph");
    srx_ctx* ctx = g->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "trim: null output handle");
    *out = nullptr;
    if (trim < 1) return fail(ctx, SRX_E_ARG, "trim: trim = %lld is below 1", (long long)trim);
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "trim: rows are sharded; the graph needs all cells");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("trim");
    hipStream_t st = ctx->stream;
    const uint64_t n = g->n;
    const size_t nk = (size_t)n * g->k;
    srx_graph* t = nullptr;
    SRX_TRY(graph_alloc(ctx, n, g->k, &t));
    t->info = g->info;
    srx_trim_info info;
    int32_t rc = SRX_OK;
    auto copy = [&](void* dst, const void* src, size_t bytes) {
        if (rc == SRX_OK && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) != hipSuccess)
            rc = fail(ctx, SRX_E_HIP, "trim: hipMemcpyAsync failed");
    };
    copy(t->d_dptr, g->d_dptr, (n + 1) * 8);
    copy(t->d_dind, g->d_dind, nk * 4);
    copy(t->d_ddat, g->d_ddat, nk * 8);
    copy(t->d_a, g->d_a, nk * 8);
    copy(t->d_rho, g->d_rho, n * 8);
    copy(t->d_sigma, g->d_sigma, n * 8);
    if (rc == SRX_OK) {
        if (n == 0) {
            memset(&info, 0, sizeof info);
            info.trim = (uint64_t)trim;
            info.wave_capacity = kTrimWaveCap;
            info.short_capacity = kTrimBlockCap;
            rc = graph_alloc_c(t, 0);
            if (rc == SRX_OK && hipMemsetAsync(t->d_cptr, 0, 8, st) != hipSuccess) rc = fail(ctx, SRX_E_HIP, "trim: hipMemsetAsync failed");
        } else {
            rc = trim_c(ctx, connectivities(g), (uint64_t)trim, t, &info);
        }
    }
    if (rc == SRX_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(ctx, SRX_E_HIP, "trim: hipStreamSynchronize failed");
    if (rc != SRX_OK) {
        srx_graph_free(t);
        return rc;
    }
    if (info_out) *info_out = info;
    *out = t;
    return SRX_OK;
}

}  // extern "C"
