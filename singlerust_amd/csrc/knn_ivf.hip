// knn_ivf.hip — approximate k-nearest-neighbour search through an inverted-file (IVF) index over dense f64 points:
// srx_knn_index_* and srx_neighbors_index.  include/srx.h defines the index and the search; this file computes them.
//
// Everything that compares a point with the centroids is the EXACT search of knn.hip on device pointers (knn_device): the
// assignment of a point is its k = 1 search among the centroids, the probe set of a query its k = n_probe search — with that
// file's certificate and its (distance, index) order.  What is new here:
//
//   k_ivf_sort_pass           one 8-bit digit of a stable counting sort of (key, value) pairs: per-block digit counts, then
//                             scan_exclusive over the (digit, block) table, then the scatter.  No atomics: a value's place
//                             is table + the counts of the waves before its own + its rank among the equal digits of its wave
//   k_ivf_offsets             list offsets from the sorted keys
//   k_ivf_segsum              one workgroup per segment of rows: a fixed-order f64 column sum or mean (centroid means over the
//                             sorted sample, the global centre, the inertia)
//   k_ivf_place               a member's place in the list-major f32 copy: every list padded to whole tiles, the original
//                             index beside it.  The copy itself is knn.hip's (knn_prepare through the index array: the same
//                             layout, global centre and norm coordinate, +inf norms at the padding)
//   k_ivf_candidates<K, RT>   THE HOT PATH: one workgroup per (list, block of <= 128 of the queries that probe it).  It is
//                             k_knn_candidates with the query fragments gathered through an index array, the reference tiles
//                             the list's own range of the copy, and K' = k + 8 candidates and a bound tau per (query, probe)
//   k_ivf_select<false>       one wave per query: the K' best of its n_probe x K' candidates by f32 score, their f64 re-rank
//                             (knn_take), knn.hip's certificate (knn_certificate) with tau = the minimum of the K'-th score
//                             and the row's pairs' bounds; lists the rows that fail and the rows that are short
//   k_ivf_select<true>        the rows that failed: the f64 selection over the members of their probed lists
// Rows whose probed lists hold fewer than k admissible points go through k_knn_exact<true> (knn_exact_rows).
//
// Certificate.  Every list is a subset of the references, centred by the same global centre c and bounded by the same
// R = max |r - c|, and a (query, probe) pair keeps or drops a point against a threshold that only falls: every point of a
// probed list that was not kept has s >= tau of its pair; the scores of all lists are one function of the same centred points,
// so the row keeps the K' lowest of its pairs' candidates and every one it drops has s >= the K'-th: tau = the minimum of both.  The proof in knn.hip's header then holds as
// written, for "the references" = the members of the probed lists.
//
// Candidate memory is n_query x n_probe x K' x 8 bytes (score and index); queries are processed in chunks so that it stays below kIvfCandBudget.
#include "common.hpp"
#include "hash.hpp"
#include "knn_internal.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>

struct srx_knn_index {
    srx_ctx* ctx = nullptr;
    uint64_t n_ref = 0, n_pad = 0;
    int d = 0, K = 0;
    uint32_t n_lists = 0;
    double* d_pts = nullptr;                 // n_ref x d, the index's own copy
    double* d_cent = nullptr;                // n_lists x d
    double* d_centre = nullptr;              // d doubles, then max |x - c|^2 as bits
    unsigned long long* d_rmax2 = nullptr;
    int64_t *d_off = nullptr, *d_poff = nullptr;      // n_lists + 1 each: members / padded positions
    uint32_t *d_members = nullptr, *d_pos = nullptr;  // n_ref each: list-major point indices; position of a point in the copy
    uint32_t* d_ids = nullptr;               // n_pad: original index of a position (kKnnNone: padding)
    float* d_ref_t = nullptr;                // n_pad x K
    std::vector<int64_t> h_off;
    srx_ivf_info info{};
};

namespace srx {

int32_t graph_from_device_list(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, srx_graph** out);   // graph.hip

constexpr size_t kIvfCandBudget = (size_t)1 << 30;      // bytes of candidates per chunk of queries
constexpr int kIvfSortItems = 4;                        // keys per thread and sort block (1024 per block)
constexpr uint64_t kIvfSumChunk = 2048;                 // rows per partial of a long fixed-order sum
constexpr int kIvfMaxProbe = 64;
constexpr uint32_t kIvfDefaultProbe = 20;                // profiles/knn_ivf.md: recall@15 0.965 at 1.3 M cells (16 gives 0.936)

// ---- stable counting sort, one 8-bit digit per pass --------------------------------------------------------------------
// lanes of this wave that are valid and hold the same digit
__device__ __forceinline__ unsigned long long ivf_match8(uint32_t digit, bool valid) {
    unsigned long long peers = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}
// Item (block, e, t) is key block * 1024 + e * 256 + t.  SCATTER = false: table[digit * nb + block] = the block's count of the
// digit.  SCATTER = true: `table` is the exclusive scan of that table; every pair goes to its place.  vals_in null: 0, 1, 2, ...
template <bool SCATTER>
__global__ void __launch_bounds__(256) k_ivf_sort_pass(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in,
                                                       uint64_t n, int shift, unsigned nb, int64_t* __restrict__ table,
                                                       uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ int cnt[kIvfSortItems * 4][256];
    for (int i = threadIdx.x; i < kIvfSortItems * 4 * 256; i += 256) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    uint32_t key[kIvfSortItems];
    int rank[kIvfSortItems];
#pragma unroll
    for (int e = 0; e < kIvfSortItems; ++e) {
        const uint64_t i = (uint64_t)blockIdx.x * (256 * kIvfSortItems) + e * 256 + threadIdx.x;
        const bool valid = i < n;
        key[e] = valid ? keys_in[i] : 0u;
        const uint32_t digit = (key[e] >> shift) & 255u;
        const unsigned long long peers = ivf_match8(digit, valid);
        const unsigned long long below = peers & ((1ull << lane) - 1ull);
        rank[e] = __builtin_popcountll(below);
        if (valid && below == 0ull) cnt[e * 4 + wave][digit] = __builtin_popcountll(peers);
    }
    __syncthreads();
    if (!SCATTER) {
        int s = 0;
        for (int r = 0; r < kIvfSortItems * 4; ++r) s += cnt[r][threadIdx.x];
        table[(size_t)threadIdx.x * nb + blockIdx.x] = s;
    } else {
#pragma unroll
        for (int e = 0; e < kIvfSortItems; ++e) {
            const uint64_t i = (uint64_t)blockIdx.x * (256 * kIvfSortItems) + e * 256 + threadIdx.x;
            if (i >= n) continue;
            const uint32_t digit = (key[e] >> shift) & 255u;
            int64_t pos = table[(size_t)digit * nb + blockIdx.x] + rank[e];
            for (int r = 0; r < e * 4 + wave; ++r) pos += cnt[r][digit];
            keys_out[pos] = key[e];
            vals_out[pos] = vals_in ? vals_in[i] : (uint32_t)i;
        }
    }
}

// off[c] = the first sorted position whose key is >= c, for c = 0 .. n_keys (thread p writes the c in (key[p - 1], key[p]])
__global__ void __launch_bounds__(256) k_ivf_offsets(const uint32_t* __restrict__ sorted, uint64_t n, uint32_t n_keys,
                                                     int64_t* __restrict__ off) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p > n) return;
    const uint32_t lo = p == 0 ? 0u : sorted[p - 1] + 1u, hi = p == n ? n_keys : sorted[p];
    for (uint32_t c = lo; c <= hi; ++c) off[c] = (int64_t)p;
}

// ---- fixed-order sums ----------------------------------------------------------------------------------------------------
// One workgroup per segment [lo, hi) of rows (off[seg] .. off[seg + 1], or chunk-sized pieces of 0 .. n when off is null); row
// p of the segment is x[idx ? idx[p] : p].  Thread t owns column t % dpow and adds the rows lo + t / dpow, + 256 / dpow, ... in
// that order; the 256 / dpow partial sums of a column are then added in order.  denom == 0: the sum; > 0: sum / denom;
// < 0: sum / (hi - lo), and an empty segment leaves its output as it is.
__global__ void __launch_bounds__(256) k_ivf_segsum(const double* __restrict__ x, size_t ld, int d, int dpow,
                                                    const uint32_t* __restrict__ idx, const int64_t* __restrict__ off,
                                                    uint64_t chunk, uint64_t n, double denom, double* __restrict__ out) {
    __shared__ double sh[256];
    const uint64_t seg = blockIdx.x;
    const uint64_t lo = off ? (uint64_t)off[seg] : seg * chunk;
    const uint64_t hi = off ? (uint64_t)off[seg + 1] : (lo + chunk < n ? lo + chunk : n);
    const int col = threadIdx.x % dpow, g = threadIdx.x / dpow, G = 256 / dpow;
    double s = 0.0;
    if (col < d)
        for (uint64_t p = lo + g; p < hi; p += G) s += x[(size_t)(idx ? idx[p] : p) * ld + col];
    sh[threadIdx.x] = s;
    __syncthreads();
    if ((int)threadIdx.x < d) {
        double t = 0.0;
        for (int gg = 0; gg < G; ++gg) t += sh[gg * dpow + threadIdx.x];
        if (denom < 0.0) {
            if (hi > lo) out[seg * d + threadIdx.x] = t / (double)(hi - lo);
        } else
            out[seg * d + threadIdx.x] = denom > 0.0 ? t / denom : t;
    }
}

// dense copy of rows (ids null: rows 0 .. n - 1) of a pitched array
__global__ void __launch_bounds__(256) k_ivf_gather(const double* __restrict__ x, size_t ld, const uint32_t* __restrict__ ids,
                                                    uint64_t n, int d, double* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * (uint64_t)d) return;
    const uint64_t r = i / d;
    const int c = (int)(i % d);
    out[i] = x[(size_t)(ids ? ids[r] : r) * ld + c];
}

// squared distance of every point to its assigned centroid
__global__ void __launch_bounds__(256) k_ivf_dist2(const double* __restrict__ x, const double* __restrict__ cent,
                                                   const uint32_t* __restrict__ assign, uint64_t n, int d, double* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = knn_dist2(x + i * d, cent + (size_t)assign[i] * d, d);
}

// ---- the list-major f32 copy ---------------------------------------------------------------------------------------------
// sorted position p (list lists[p], point members[p]) -> its place in the padded copy
__global__ void __launch_bounds__(256) k_ivf_place(const uint32_t* __restrict__ lists, const uint32_t* __restrict__ members,
                                                   uint64_t n, const int64_t* __restrict__ off, const int64_t* __restrict__ poff,
                                                   uint32_t* __restrict__ ids, uint32_t* __restrict__ pos) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t l = lists[p], m = members[p];
    const uint32_t q = (uint32_t)(poff[l] + ((int64_t)p - off[l]));
    ids[q] = m;
    pos[m] = q;
}

// ---- candidate pass, list-major ------------------------------------------------------------------------------------------
// items[w] = (list, first sorted pair, pairs <= 128, -).  pairs[]: the chunk's (query, probe slot) pairs sorted by list, as
// (query - q0) * n_probe + slot.  A query's fragment is read at position qpos[query] (qpos null: query) of qry_t.  Keys carry
// the position inside the list (ascending with the point index, as the members are); the self-skip and the output translate it
// through ids.  Dynamic LDS: 2 tiles | keys 128 x CAP | cnt 128 | tau 128.  Out: cand[pair x KP] as keys (ordered score bits
// << 32 | point index; ~0: none), tau_out[pair].
// The tile loop below (LDS carve-up, staging, MFMA chain, minimum tree and ballot, C/D row map, append, merge-on-full) is
// k_knn_candidates' loop, which is the case "every slot live, one list = all references".  Stated once as a forceinline
// template it compiled to the same loop instructions at the same occupancy, yet the searches at 1.3 M cells measured 0.2 to
// 0.5 % slower than the two copies (profiles/knn.md, profiles/knn_ivf.md), so the copies stay: a change to one is a change
// to both.
template <int K, int RT>
__global__ void __launch_bounds__(256) k_ivf_candidates(const float* __restrict__ ref_t, const uint32_t* __restrict__ ids,
                                                        const int64_t* __restrict__ poff, const float* __restrict__ qry_t,
                                                        const uint32_t* __restrict__ qpos, const uint32_t* __restrict__ pairs,
                                                        const uint4* __restrict__ items, uint64_t q0, int n_probe, int d, int KP,
                                                        int CAP, int self_skip, unsigned long long* __restrict__ cand,
                                                        float* __restrict__ tau_out) {
    constexpr int S = K / 2;
    constexpr int TILE = RT * K;
    constexpr int NV = (TILE / 4 + 255) / 256;
    extern __shared__ __align__(16) unsigned char smem[];
    float* tiles = reinterpret_cast<float*>(smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + (size_t)2 * TILE * 4);
    int* cnt = reinterpret_cast<int*>(keys + (size_t)kKnnQB * CAP);
    float* tau_s = reinterpret_cast<float*>(cnt + kKnnQB);

    const uint4 item = items[blockIdx.x];
    const uint32_t list = item.x, first = item.y;
    const int n_here = (int)item.z;
    const uint64_t p0 = (uint64_t)poff[list];
    const uint64_t n_tiles = ((uint64_t)poff[list + 1] - p0) / RT;

    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int qs = wave * 32 + j;                  // this lane's query slot (two lanes share one)
    const bool live = qs < n_here;
    const bool wave_live = wave * 32 < n_here;
    const uint32_t pair = live ? pairs[first + qs] : 0u;
    const uint32_t q_idx = (uint32_t)(q0 + pair / (uint32_t)n_probe);

    if (threadIdx.x < kKnnQB) {
        cnt[threadIdx.x] = 0;
        tau_s[threadIdx.x] = (int)threadIdx.x < n_here ? __builtin_inff() : -__builtin_inff();   // an unused slot keeps nothing
    }
    // B operand: (-2 q, 1, 0..): element [k = 2s + h][column j], gathered from the query's own fragment block
    float qreg[S];
    {
        const uint32_t qp = live ? (qpos ? qpos[q_idx] : q_idx) : 0u;
        const float* qf = qry_t + (size_t)(qp >> 5) * (32 * K) + (qp & 31) + h * 32;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int kk = 2 * s + h;
            float v = 0.f;
            if (live && kk < d) v = -2.f * qf[s * 64];
            qreg[s] = kk == d ? 1.f : v;
        }
    }
    const f32x4* g = reinterpret_cast<const f32x4*>(ref_t + p0 * (size_t)K);
    f32x4 stage[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const int w = v * 256 + (int)threadIdx.x;
        stage[v] = g[w < TILE / 4 ? w : 0];
        if (w < TILE / 4) reinterpret_cast<f32x4*>(tiles)[w] = stage[v];
    }
    __syncthreads();
    float tau = live ? __builtin_inff() : -__builtin_inff();
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
        if (wave_live) {
#pragma unroll
            for (int sub = 0; sub < RT / 32; ++sub) {
                f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < S; ++s)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[(sub * S + s) * 64 + lane], qreg[s], acc, 0, 0, 0);
                float lo = acc[0];
#pragma unroll
                for (int r = 1; r < 16; ++r) lo = fminf(lo, acc[r]);
                if (__builtin_amdgcn_ballot_w64(lo < tau) != 0ull) {
                    const uint32_t base = (uint32_t)(t * RT) + sub * 32 + 4 * h;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const uint32_t loc = base + (r & 3) + 8 * (r >> 2);     // C/D map: row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
                        if (acc[r] < tau && !(self_skip && ids[p0 + loc] == q_idx)) {
                            const int slot = atomicAdd(&cnt[qs], 1);
                            keys[(size_t)qs * CAP + slot] = ((unsigned long long)f32_key(acc[r]) << 32) | loc;
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
        if (s >= n_here) break;
        knn_merge(keys, cnt, tau_s, s, CAP, KP);
        const int n = cnt[s];
        const uint32_t pr = pairs[first + s];
        for (int c = lane; c < KP; c += 64) {
            const unsigned long long e = keys[(size_t)s * CAP + c];      // the score stays, the position becomes the point index
            cand[(size_t)pr * KP + c] = c < n ? ((e & 0xFFFFFFFF00000000ull) | ids[p0 + (uint32_t)e]) : ~0ull;
        }
        if (lane == 0) tau_out[pr] = tau_s[s];
    }
}

// ---- f64 selection ---------------------------------------------------------------------------------------------------------
// One wave per query row.  LISTS = false: row q0 + w of the chunk, over its n_probe x KP candidates; the certificate decides
// whether it is written, listed in fail_rows (count[0]) or — fewer than k admissible members in its probed lists — in
// short_rows (count[1]).  LISTS = true: row rows[w] over all members of its probed lists, always written.
template <bool LISTS>
__global__ void __launch_bounds__(256) k_ivf_select(const double* __restrict__ ref, const double* __restrict__ qry, size_t ld_q,
                                                    uint64_t q0, uint64_t n_rows, int d, int k, int KP, int n_probe, int self_skip,
                                                    const unsigned long long* __restrict__ cand, const float* __restrict__ tau,
                                                    const uint32_t* __restrict__ probe, const int64_t* __restrict__ off,
                                                    const uint32_t* __restrict__ members, const double* __restrict__ centre,
                                                    const unsigned long long* __restrict__ rmax2_bits, int Kpad,
                                                    const uint32_t* __restrict__ rows, uint32_t* __restrict__ idx_out,
                                                    double* __restrict__ dist_out, uint32_t* __restrict__ fail_rows,
                                                    uint32_t* __restrict__ short_rows, unsigned int* __restrict__ count) {
    __shared__ double sd[4][128];
    __shared__ uint32_t si[4][128];
    __shared__ unsigned long long sk[4][kKnnMaxK + kKnnSlack + 64];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
    if (w >= n_rows) return;
    const uint64_t q = LISTS ? rows[w] : q0 + w;
    const double* qp = qry + q * ld_q;
    const uint32_t* pr = probe + q * (size_t)n_probe;
    double* D = sd[wave];
    uint32_t* I = si[wave];
    unsigned long long* Kk = sk[wave];
    // LISTS = false, first: the KP lowest of the row's n_probe x KP keys, by (f32 score, point index).  The scores of all
    // lists are the same function of the same centred points, so they compare across lists; every key dropped here has a
    // score >= the KP-th kept one, which joins the pairs' bounds in the certificate below.
    int n_keys = 0, n_valid = 0;
    if (!LISTS) {
        const unsigned long long* src = cand + w * (size_t)n_probe * KP;
        const int total = n_probe * KP;
        for (int c0 = 0; c0 < total; c0 += 64) {
            const unsigned long long key = c0 + lane < total ? src[c0 + lane] : ~0ull;
            bool ok = key != ~0ull;
            n_valid += __builtin_popcountll(__builtin_amdgcn_ballot_w64(ok));
            if (ok && n_keys == KP) ok = key < Kk[KP - 1];
            const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
            if (m == 0ull) continue;
            if (ok) Kk[n_keys + __builtin_popcountll(m & ((1ull << lane) - 1ull))] = key;
            const int nk = n_keys + __builtin_popcountll(m);          // <= KP + 64 <= 136
            wave_lds_sync();
            unsigned long long e[3];
            int r[3] = {0, 0, 0};
#pragma unroll
            for (int t = 0; t < 3; ++t) e[t] = lane + 64 * t < nk ? Kk[lane + 64 * t] : ~0ull;
            for (int x = 0; x < nk; ++x) {
                const unsigned long long o = Kk[x];
#pragma unroll
                for (int t = 0; t < 3; ++t) r[t] += o < e[t];
            }
            wave_lds_sync();
#pragma unroll
            for (int t = 0; t < 3; ++t)
                if (lane + 64 * t < nk && r[t] < KP) Kk[r[t]] = e[t];     // keys are distinct (distinct points)
            n_keys = nk < KP ? nk : KP;
            wave_lds_sync();
        }
    }
    int n = 0;                                    // kept entries, sorted, wave-uniform
    const int n_seg = LISTS ? n_probe : 1;
    for (int sg = 0; sg < n_seg; ++sg) {
        const uint32_t* src = LISTS ? members + off[pr[sg]] : nullptr;
        const uint64_t total = LISTS ? (uint64_t)(off[pr[sg] + 1] - off[pr[sg]]) : (uint64_t)n_keys;
        for (uint64_t c0 = 0; c0 < total; c0 += 64) {
            const uint32_t idx = c0 + lane < total ? (LISTS ? src[c0 + lane] : (uint32_t)Kk[c0 + lane]) : kKnnNone;
            bool ok = idx != kKnnNone && !(self_skip && idx == (uint32_t)q);
            double dd = 0.0;
            if (ok) {
                dd = knn_dist2(qp, ref + (size_t)idx * d, d);
                if (n == k) ok = knn_less(dd, idx, D[k - 1], I[k - 1]);
            }
            n = knn_take(D, I, n, k, ok, dd, idx);
        }
    }
    bool write = true;
    if (!LISTS) {
        long long len = 0;
        float tq = __builtin_inff();
        if (lane < n_probe) {
            len = off[pr[lane] + 1] - off[pr[lane]];
            tq = tau[w * (size_t)n_probe + lane];
        }
        const long long avail = wave_sum(len) - (self_skip ? 1 : 0);      // (in the self form a point's own list is probed)
        float tau_min = wave_min(tq);
        if (n_valid > KP) tau_min = fminf(tau_min, key_f32((uint32_t)(Kk[KP - 1] >> 32)));
        const KnnBound b = knn_certificate(qp, centre, d, Kpad, rmax2_bits);
        const bool is_short = avail < (long long)k;
        write = !is_short && n == k && (D[k - 1] - b.qn) + b.eps_row < (double)tau_min;
        if (!write && lane == 0) {
            if (is_short) short_rows[atomicAdd(count + 1, 1u)] = (uint32_t)q;
            else fail_rows[atomicAdd(count, 1u)] = (uint32_t)q;
        }
    }
    if (write)
        for (int c = lane; c < k; c += 64) {
            idx_out[q * k + c] = I[c];
            dist_out[q * k + c] = sqrt(D[c]);
        }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// Stable sort of n pairs (d_keys[i] < n_keys, i) by key: *keys_out / *vals_out are scratch slots, valid until the next sort.
static int32_t ivf_sort(srx_ctx* ctx, const uint32_t* d_keys, uint64_t n, uint32_t n_keys, uint32_t** keys_out, uint32_t** vals_out) {
    const unsigned nb = (unsigned)((at_least_one(n) + 256 * kIvfSortItems - 1) / (256 * kIvfSortItems));
    uint32_t* buf;
    int64_t* tab;
    SRX_TRY(scratch(ctx, "ivf_sort_buf", 4 * up256(at_least_one(n) * 4), (void**)&buf));
    SRX_TRY(scratch(ctx, "ivf_sort_tab", (2 * (size_t)256 * nb + 1) * 8, (void**)&tab));
    const size_t stride = up256(at_least_one(n) * 4) / 4;
    uint32_t *k_buf[2] = {buf, buf + stride}, *v_buf[2] = {buf + 2 * stride, buf + 3 * stride};
    int passes = 1;
    while (passes < 4 && ((uint64_t)1 << (8 * passes)) < (uint64_t)n_keys) ++passes;
    const uint32_t *kin = d_keys, *vin = nullptr;
    for (int p = 0; p < passes; ++p) {
        hipLaunchKernelGGL(k_ivf_sort_pass<false>, dim3(nb), dim3(256), 0, ctx->stream, kin, vin, n, 8 * p, nb, tab, (uint32_t*)nullptr,
                           (uint32_t*)nullptr);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(scan_exclusive(ctx, tab, (uint64_t)256 * nb, tab + (size_t)256 * nb, nullptr));
        hipLaunchKernelGGL(k_ivf_sort_pass<true>, dim3(nb), dim3(256), 0, ctx->stream, kin, vin, n, 8 * p, nb, tab + (size_t)256 * nb,
                           k_buf[p & 1], v_buf[p & 1]);
        SRX_HIP(ctx, hipGetLastError());
        kin = k_buf[p & 1];
        vin = v_buf[p & 1];
    }
    *keys_out = const_cast<uint32_t*>(kin);
    *vals_out = const_cast<uint32_t*>(vin);
    return SRX_OK;
}

static int pow2_at_least(int d) {
    int p = 1;
    while (p < d) p <<= 1;
    return p;
}
// out[0 .. d) = the column sums of x (n x d, pitch ld) over denom (0: the plain sum), in the fixed order of k_ivf_segsum twice
static int32_t ivf_colsum(srx_ctx* ctx, const double* x, size_t ld, uint64_t n, int d, double denom, double* out) {
    const uint64_t n_part = (n + kIvfSumChunk - 1) / kIvfSumChunk;
    double* part;
    SRX_TRY(scratch(ctx, "ivf_part", at_least_one(n_part) * d * 8, (void**)&part));
    const int dpow = pow2_at_least(d);
    hipLaunchKernelGGL(k_ivf_segsum, dim3((unsigned)n_part), dim3(256), 0, ctx->stream, x, ld, d, dpow, (const uint32_t*)nullptr,
                       (const int64_t*)nullptr, kIvfSumChunk, n, 0.0, part);
    hipLaunchKernelGGL(k_ivf_segsum, dim3(1), dim3(256), 0, ctx->stream, (const double*)part, (size_t)d, d, dpow, (const uint32_t*)nullptr,
                       (const int64_t*)nullptr, n_part, n_part, denom, out);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

static void ivf_release(srx_knn_index* ix) {
    if (!ix) return;
    if (ix->ctx) (void)hipSetDevice(ix->ctx->device);
    for (void* p : {(void*)ix->d_pts, (void*)ix->d_cent, (void*)ix->d_centre, (void*)ix->d_off, (void*)ix->d_poff, (void*)ix->d_members,
                    (void*)ix->d_pos, (void*)ix->d_ids, (void*)ix->d_ref_t})
        if (p) (void)hipFree(p);
    delete ix;
}

// the training sample: the n_train points with the smallest (mix(mix(seed) ^ i), i), in that order
static std::vector<uint32_t> ivf_sample(uint64_t n_ref, uint64_t n_train, uint64_t seed) {
    std::vector<std::pair<uint64_t, uint32_t>> h(n_ref);
    const uint64_t s = splitmix64(seed);
    for (uint64_t i = 0; i < n_ref; ++i) h[i] = {splitmix64(s ^ i), (uint32_t)i};
    std::partial_sort(h.begin(), h.begin() + n_train, h.end());
    std::vector<uint32_t> ids(n_train);
    for (uint64_t i = 0; i < n_train; ++i) ids[i] = h[i].second;
    return ids;
}

// Lloyd iterations on the hashed sample; ix->d_cent holds the result
static int32_t ivf_train(srx_knn_index* ix, const srx_ivf_opts& o, uint64_t n_train) {
    srx_ctx* ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const int d = ix->d;
    const uint32_t L = ix->n_lists;
    const std::vector<uint32_t> ids = ivf_sample(ix->n_ref, n_train, o.seed);
    uint32_t* d_sid;
    double* d_sample;
    SRX_TRY(scratch(ctx, "ivf_sample_ids", n_train * 4, (void**)&d_sid));
    SRX_TRY(scratch(ctx, "ivf_sample", n_train * (size_t)d * 8, (void**)&d_sample));
    SRX_TRY(h2d(ctx, d_sid, ids.data(), n_train * 4));
    {
        ProfScope ps(ctx, SRX_K_KNN, (double)n_train * d * 16.0);
        hipLaunchKernelGGL(k_ivf_gather, dim3(grid256(n_train * d)), dim3(256), 0, st, (const double*)ix->d_pts, (size_t)d,
                           (const uint32_t*)d_sid, n_train, d, d_sample);
        SRX_HIP(ctx, hipGetLastError());
        SRX_HIP(ctx, hipMemcpyAsync(ix->d_cent, d_sample, (size_t)L * d * 8, hipMemcpyDeviceToDevice, st));      // the start
    }
    const srx_knn_opts one{1, 0, 0, 0};
    for (int it = 0; it < o.train_iters; ++it) {
        KnnArgs a{ix->d_cent, d_sample, L, n_train, (size_t)d, (size_t)d, d, false};
        SRX_TRY(knn_device(ctx, a, &one, nullptr, nullptr, nullptr));
        uint32_t *d_assign, *d_keys, *d_vals;
        int64_t* d_toff;
        SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)&d_assign));
        SRX_TRY(scratch(ctx, "ivf_toff", ((size_t)L + 1) * 8, (void**)&d_toff));
        ProfScope ps(ctx, SRX_K_KNN, (double)n_train * d * 8.0);
        SRX_TRY(ivf_sort(ctx, d_assign, n_train, L, &d_keys, &d_vals));
        hipLaunchKernelGGL(k_ivf_offsets, dim3(grid256(n_train + 1)), dim3(256), 0, st, (const uint32_t*)d_keys, n_train, L, d_toff);
        hipLaunchKernelGGL(k_ivf_segsum, dim3(L), dim3(256), 0, st, (const double*)d_sample, (size_t)d, d, pow2_at_least(d),
                           (const uint32_t*)d_vals, (const int64_t*)d_toff, (uint64_t)0, n_train, -1.0, ix->d_cent);
        SRX_HIP(ctx, hipGetLastError());
    }
    return SRX_OK;
}

// The index over n_ref points at d_src (device, pitch ld, the first d coordinates); h_cent: supplied centroids or null.
static int32_t ivf_build(srx_ctx* ctx, const double* d_src, size_t ld, uint64_t n_ref, int d, const srx_ivf_opts& o,
                         const double* h_cent, srx_knn_index** out) {
    hipStream_t st = ctx->stream;
    uint32_t L = (uint32_t)o.n_lists;
    if (L == 0) L = (uint32_t)std::min<double>((double)n_ref, std::max(1.0, std::round(4.0 * std::sqrt((double)n_ref))));
    uint64_t n_train = 0;
    if (!h_cent) {
        const uint64_t want = o.max_train_points ? o.max_train_points : (uint64_t)64 * L;
        n_train = std::min<uint64_t>(n_ref, std::max<uint64_t>(want, L));
    }
    srx_knn_index* ix = new srx_knn_index;
    struct Guard {
        srx_knn_index* p;
        ~Guard() { ivf_release(p); }
    } guard{ix};
    ix->ctx = ctx;
    ix->n_ref = n_ref;
    ix->d = d;
    ix->K = knn_padded_width(d);
    ix->n_lists = L;
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_pts, n_ref * (size_t)d * 8));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_cent, (size_t)L * d * 8));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_centre, ((size_t)d + 1) * 8));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_off, ((size_t)L + 1) * 8));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_poff, ((size_t)L + 1) * 8));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_members, n_ref * 4));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_pos, n_ref * 4));
    ix->d_rmax2 = reinterpret_cast<unsigned long long*>(ix->d_centre + d);
    hipLaunchKernelGGL(k_ivf_gather, dim3(grid256(n_ref * d)), dim3(256), 0, st, d_src, ld, (const uint32_t*)nullptr, n_ref, d, ix->d_pts);
    SRX_HIP(ctx, hipGetLastError());

    StreamTimer t_train(ctx, st), t_assign(ctx, st);
    double ms_train = 0.0, ms_assign = 0.0;
    if (h_cent) SRX_TRY(h2d(ctx, ix->d_cent, h_cent, (size_t)L * d * 8));
    else {
        SRX_TRY(t_train.start());
        SRX_TRY(ivf_train(ix, o, n_train));
        SRX_TRY(t_train.stop(&ms_train));
    }

    // assignment (also where NaN / Inf in the points or the centroids is refused), lists, inertia
    SRX_TRY(t_assign.start());
    const srx_knn_opts one{1, 0, 0, 0};
    KnnArgs a{ix->d_cent, ix->d_pts, L, n_ref, (size_t)d, (size_t)d, d, false};
    SRX_TRY(knn_device(ctx, a, &one, nullptr, nullptr, nullptr));
    uint32_t *d_assign, *d_keys, *d_vals;
    double* d_d2;
    SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)&d_assign));
    SRX_TRY(scratch(ctx, "ivf_d2", (n_ref + 1) * 8, (void**)&d_d2));
    double inertia = 0.0;
    {
        ProfScope ps(ctx, SRX_K_KNN, (double)n_ref * d * 8.0 * 3.0);
        hipLaunchKernelGGL(k_ivf_dist2, dim3(grid256(n_ref)), dim3(256), 0, st, (const double*)ix->d_pts, (const double*)ix->d_cent,
                           (const uint32_t*)d_assign, n_ref, d, d_d2);
        SRX_TRY(ivf_colsum(ctx, d_d2, 1, n_ref, 1, 0.0, d_d2 + n_ref));
        SRX_TRY(ivf_sort(ctx, d_assign, n_ref, L, &d_keys, &d_vals));
        hipLaunchKernelGGL(k_ivf_offsets, dim3(grid256(n_ref + 1)), dim3(256), 0, st, (const uint32_t*)d_keys, n_ref, L, ix->d_off);
        SRX_HIP(ctx, hipGetLastError());
        SRX_HIP(ctx, hipMemcpyAsync(ix->d_members, d_vals, n_ref * 4, hipMemcpyDeviceToDevice, st));
    }
    SRX_TRY(d2h(ctx, &inertia, d_d2 + n_ref, 8));
    ix->h_off.resize((size_t)L + 1);
    SRX_TRY(d2h(ctx, ix->h_off.data(), ix->d_off, ((size_t)L + 1) * 8));

    // every list padded to whole tiles; the f32 copy with the global centre
    std::vector<int64_t> h_poff((size_t)L + 1, 0);
    uint64_t min_list = n_ref, max_list = 0, empty = 0;
    for (uint32_t l = 0; l < L; ++l) {
        const uint64_t len = (uint64_t)(ix->h_off[l + 1] - ix->h_off[l]);
        h_poff[l + 1] = h_poff[l] + (int64_t)((len + kKnnPad - 1) / kKnnPad * kKnnPad);
        min_list = std::min(min_list, len);
        max_list = std::max(max_list, len);
        empty += len == 0;
    }
    ix->n_pad = (uint64_t)h_poff[L];
    if (ix->n_pad >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "knn index: the padded lists hold more than 2^32 - 2 positions");
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_ids, ix->n_pad * 4));
    SRX_HIP(ctx, hipMalloc((void**)&ix->d_ref_t, ix->n_pad * (size_t)ix->K * 4));
    SRX_TRY(h2d(ctx, ix->d_poff, h_poff.data(), ((size_t)L + 1) * 8));
    {
        ProfScope ps(ctx, SRX_K_KNN, (double)n_ref * d * 12.0);
        SRX_HIP(ctx, hipMemsetAsync(ix->d_ids, 0xFF, ix->n_pad * 4, st));
        SRX_HIP(ctx, hipMemsetAsync(ix->d_rmax2, 0, 8, st));
        hipLaunchKernelGGL(k_ivf_place, dim3(grid256(n_ref)), dim3(256), 0, st, (const uint32_t*)d_keys, (const uint32_t*)ix->d_members,
                           n_ref, (const int64_t*)ix->d_off, (const int64_t*)ix->d_poff, ix->d_ids, ix->d_pos);
        SRX_TRY(ivf_colsum(ctx, ix->d_pts, (size_t)d, n_ref, d, (double)n_ref, ix->d_centre));
        SRX_TRY(knn_prepare(ctx, ix->d_pts, (size_t)d, ix->d_ids, n_ref, ix->n_pad, d, ix->K, ix->d_centre, ix->d_ref_t, ix->d_rmax2));
    }
    SRX_TRY(t_assign.stop(&ms_assign));

    srx_ivf_info& info = ix->info;
    memset(&info, 0, sizeof info);
    info.n_ref = n_ref;
    info.n_train = n_train;
    info.d = (uint32_t)d;
    info.n_lists = L;
    info.train_iters = h_cent ? 0u : (uint32_t)o.train_iters;
    info.min_list = min_list;
    info.max_list = max_list;
    info.empty_lists = empty;
    info.inertia = inertia;
    info.ms_train = ms_train;
    info.ms_assign = ms_assign;
    guard.p = nullptr;
    *out = ix;
    return SRX_OK;
}

static int32_t ivf_opts_check(srx_ctx* ctx, const srx_ivf_opts* opts, uint64_t n_ref, uint64_t d, srx_ivf_opts* o) {
    *o = opts ? *opts : srx_ivf_opts{0, 10, 0, 0};
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "knn index: rows are sharded; the index needs all cells");
    if (d < 1 || d > SRX_KNN_MAX_DIMS)
        return fail(ctx, SRX_E_ARG, "knn index: %llu coordinates outside 1..%d", (unsigned long long)d, SRX_KNN_MAX_DIMS);
    if (n_ref < 1 || n_ref >= 0xFFFFFFFFull)
        return fail(ctx, SRX_E_ARG, "knn index: %llu points outside 1..2^32 - 2", (unsigned long long)n_ref);
    if (o->n_lists < 0 || (uint64_t)o->n_lists > n_ref)
        return fail(ctx, SRX_E_ARG, "knn index: n_lists = %d outside 0..%llu", o->n_lists, (unsigned long long)n_ref);
    if (o->train_iters < 0 || o->train_iters > 1000) return fail(ctx, SRX_E_ARG, "knn index: train_iters = %d outside 0..1000", o->train_iters);
    return SRX_OK;
}

// The search of n_query rows at d_qry (device, pitch ld_q; the index's own points for the self form).  The list is left in the
// "knn_idx" / "knn_dist" scratch slots, as knn_device leaves it.
static int32_t ivf_search_device(srx_knn_index* ix, const double* d_qry, size_t ld_q, uint64_t n_query, bool self, int k,
                                 int include_self, int n_probe, srx_ivf_search_info* info) {
    srx_ctx* ctx = ix->ctx;
    hipStream_t st = ctx->stream;
    const int d = ix->d, K = ix->K;
    const uint32_t L = ix->n_lists;
    const int self_skip = self && !include_self;
    const uint64_t admissible = ix->n_ref - (self_skip ? 1 : 0);
    const KnnCounts counts = knn_candidate_counts(k, admissible);
    const int KP = counts.KP, CAP = counts.CAP;

    // probe sets: the exact n_probe nearest centroids of every query
    const srx_knn_opts po{n_probe, 0, 0, 0};
    KnnArgs pa{ix->d_cent, d_qry, L, n_query, (size_t)d, ld_q, d, false};
    SRX_TRY(knn_device(ctx, pa, &po, nullptr, nullptr, nullptr));
    uint32_t *d_knn, *d_probe, *d_idx, *d_fail, *d_short;
    double* d_dist;
    unsigned int* d_count;
    int64_t* d_qoff;
    SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)&d_knn));
    SRX_TRY(scratch(ctx, "ivf_probe", n_query * (size_t)n_probe * 4, (void**)&d_probe));
    SRX_HIP(ctx, hipMemcpyAsync(d_probe, d_knn, n_query * (size_t)n_probe * 4, hipMemcpyDeviceToDevice, st));
    SRX_HIP(ctx, hipStreamSynchronize(st));                      // (the slot may be replaced by a larger one below)
    SRX_TRY(scratch(ctx, "knn_idx", n_query * (size_t)k * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "knn_dist", n_query * (size_t)k * 8, (void**)&d_dist));
    SRX_TRY(scratch(ctx, "ivf_rows", (2 * n_query + 2) * 4, (void**)&d_fail));
    d_short = d_fail + n_query;
    d_count = reinterpret_cast<unsigned int*>(d_short + n_query);
    SRX_TRY(scratch(ctx, "ivf_qoff", ((size_t)L + 1) * 8, (void**)&d_qoff));

    // query fragments: the index's own copy through the positions for the self form, else a copy in query order
    const float* d_qry_t = ix->d_ref_t;
    const uint32_t* d_qpos = ix->d_pos;
    if (!self) {
        const uint64_t nq_pad = (n_query + 31) / 32 * 32;
        float* t;
        SRX_TRY(scratch(ctx, "ivf_qry_f32", nq_pad * (size_t)K * 4, (void**)&t));
        ProfScope ps(ctx, SRX_K_KNN, (double)n_query * d * 12.0);
        SRX_TRY(knn_prepare(ctx, d_qry, ld_q, nullptr, n_query, nq_pad, d, K, ix->d_centre, t, nullptr));
        d_qry_t = t;
        d_qpos = nullptr;
    }

    const uint64_t rows_per_chunk = std::max<uint64_t>(1, kIvfCandBudget / ((size_t)n_probe * KP * 8));
    uint64_t n_fail_all = 0, n_short_all = 0, scanned = 0;
    std::vector<int64_t> h_qoff((size_t)L + 1);
    std::vector<uint4> h_items;
    KnnArgs full{ix->d_pts, d_qry, ix->n_ref, n_query, (size_t)d, ld_q, d, self};
    for (uint64_t q0 = 0; q0 < n_query; q0 += rows_per_chunk) {
        const uint64_t nq = std::min(rows_per_chunk, n_query - q0), n_pairs = nq * n_probe;
        unsigned long long* d_cand;
        uint32_t *d_keys, *d_pairs;
        float* d_tau;
        uint4* d_items;
        SRX_TRY(scratch(ctx, "ivf_cand", n_pairs * (size_t)KP * 8, (void**)&d_cand));
        SRX_TRY(scratch(ctx, "ivf_tau", n_pairs * 4, (void**)&d_tau));
        {
            // (query, probe) pairs by list; a list with no member writes nothing: its pairs keep "none" and tau = +inf
            ProfScope ps(ctx, SRX_K_KNN, (double)n_pairs * 16.0);
            SRX_TRY(ivf_sort(ctx, d_probe + q0 * n_probe, n_pairs, L, &d_keys, &d_pairs));
            hipLaunchKernelGGL(k_ivf_offsets, dim3(grid256(n_pairs + 1)), dim3(256), 0, st, (const uint32_t*)d_keys, n_pairs, L, d_qoff);
            SRX_HIP(ctx, hipGetLastError());
            SRX_HIP(ctx, hipMemsetAsync(d_cand, 0xFF, n_pairs * (size_t)KP * 8, st));
            SRX_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)d_tau, 0x7F800000, n_pairs, st));
            SRX_HIP(ctx, hipMemsetAsync(d_count, 0, 8, st));
        }
        SRX_TRY(d2h(ctx, h_qoff.data(), d_qoff, ((size_t)L + 1) * 8));
        h_items.clear();
        for (uint32_t l = 0; l < L; ++l) {
            const uint64_t nql = (uint64_t)(h_qoff[l + 1] - h_qoff[l]), len = (uint64_t)(ix->h_off[l + 1] - ix->h_off[l]);
            scanned += nql * len;
            if (!len) continue;
            for (uint64_t b = 0; b < nql; b += kKnnQB)
                h_items.push_back(make_uint4(l, (uint32_t)(h_qoff[l] + b), (uint32_t)std::min<uint64_t>(kKnnQB, nql - b), 0u));
        }
        SRX_TRY(scratch(ctx, "ivf_items", at_least_one(h_items.size()) * sizeof(uint4), (void**)&d_items));
        SRX_TRY(h2d(ctx, d_items, h_items.data(), h_items.size() * sizeof(uint4)));
        unsigned int h_count[2] = {0, 0};
        {
            ProfScope ps(ctx, SRX_K_KNN, (double)nq * d * 8.0 + (double)nq * k * 12.0);
            const unsigned n_items = (unsigned)h_items.size();
            if (n_items) {
                SRX_TRY(knn_dispatch(K, [&](auto Kc, auto RTc) -> int32_t {
                    constexpr int KK = decltype(Kc)::value, RT = decltype(RTc)::value;
                    const size_t lds = knn_candidates_lds(KK, RT, CAP);
                    SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_ivf_candidates<KK, RT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     (int)lds));
                    hipLaunchKernelGGL((k_ivf_candidates<KK, RT>), dim3(n_items), dim3(256), lds, st, (const float*)ix->d_ref_t,
                                       (const uint32_t*)ix->d_ids, (const int64_t*)ix->d_poff, d_qry_t, d_qpos, (const uint32_t*)d_pairs,
                                       (const uint4*)d_items, q0, n_probe, d, KP, CAP, self_skip, d_cand, d_tau);
                    SRX_HIP(ctx, hipGetLastError());
                    return SRX_OK;
                }));
            }
            hipLaunchKernelGGL(k_ivf_select<false>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, (const double*)ix->d_pts, d_qry, ld_q,
                               q0, nq, d, k, KP, n_probe, self_skip, (const unsigned long long*)d_cand, (const float*)d_tau,
                               (const uint32_t*)d_probe, (const int64_t*)ix->d_off, (const uint32_t*)ix->d_members,
                               (const double*)ix->d_centre, (const unsigned long long*)ix->d_rmax2, K, (const uint32_t*)nullptr, d_idx,
                               d_dist, d_fail, d_short, d_count);
            SRX_HIP(ctx, hipGetLastError());
            SRX_TRY(d2h(ctx, h_count, d_count, 8));
            if (h_count[0]) {
                hipLaunchKernelGGL(k_ivf_select<true>, dim3((h_count[0] + 3) / 4), dim3(256), 0, st, (const double*)ix->d_pts, d_qry, ld_q,
                                   (uint64_t)0, (uint64_t)h_count[0], d, k, KP, n_probe, self_skip, (const unsigned long long*)nullptr,
                                   (const float*)nullptr, (const uint32_t*)d_probe, (const int64_t*)ix->d_off,
                                   (const uint32_t*)ix->d_members, (const double*)nullptr, (const unsigned long long*)nullptr, K,
                                   (const uint32_t*)d_fail, d_idx, d_dist, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                   (unsigned int*)nullptr);
                SRX_HIP(ctx, hipGetLastError());
            }
            SRX_TRY(knn_exact_rows(ctx, full, k, self_skip, d_short, h_count[1], d_idx, d_dist));
        }
        SRX_HIP(ctx, hipStreamSynchronize(st));                  // (the next chunk reuses the row lists and the counters)
        n_fail_all += h_count[0];
        n_short_all += h_count[1];
    }
    if (info) {
        memset(info, 0, sizeof *info);
        info->n_query = n_query;
        info->k = (uint32_t)k;
        info->n_probe = (uint32_t)n_probe;
        info->n_candidates = (uint32_t)KP;
        info->rows_rescanned = n_fail_all;
        info->rows_exhaustive = n_short_all;
        info->rows_certified = n_query - n_fail_all - n_short_all;
        info->pairs = n_query * (uint64_t)n_probe;
        info->points_scanned = scanned;
    }
    return SRX_OK;
}

// checks of a search; *n_probe_out: the resolved probe count, *self / *n_query as the search will run
static int32_t ivf_search_check(srx_knn_index* ix, bool self, uint64_t n_query, const srx_knn_opts* opts, int32_t n_probe,
                                int* n_probe_out) {
    srx_ctx* ctx = ix->ctx;
    int du = 0;
    SRX_TRY(knn_check(ctx, opts, ix->n_ref, n_query, (uint64_t)ix->d, self, &du));
    if (du != ix->d) return fail(ctx, SRX_E_ARG, "knn index: n_dims = %d but the index was built over %d coordinates", opts->n_dims, ix->d);
    if (n_probe < 0 || n_probe > kIvfMaxProbe || (uint32_t)n_probe > ix->n_lists)
        return fail(ctx, SRX_E_ARG, "knn index: n_probe = %d outside 0..%d or above the %u lists", n_probe, kIvfMaxProbe, ix->n_lists);
    *n_probe_out = n_probe ? n_probe : (int)std::min<uint32_t>(kIvfDefaultProbe, ix->n_lists);
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_knn_index_points(srx_ctx* ctx, const double* ref, uint64_t n_ref, uint64_t d, const srx_ivf_opts* opts,
                             const double* centroids, srx_knn_index** out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (!out) return fail(ctx, SRX_E_ARG, "knn index: null output handle");
    *out = nullptr;
    srx_ivf_opts o;
    SRX_TRY(ivf_opts_check(ctx, opts, n_ref, d, &o));
    if (!ref) return fail(ctx, SRX_E_ARG, "knn index: null reference points");
    if (centroids) {
        if (o.n_lists == 0) return fail(ctx, SRX_E_ARG, "knn index: supplied centroids need n_lists");
        for (uint64_t i = 0; i < (uint64_t)o.n_lists * d; ++i)
            if (!is_finite(centroids[i])) return fail(ctx, SRX_E_ARG, "knn index: the centroids hold NaN or Inf");
    }
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("knn_index");
    double* d_up;
    SRX_TRY(scratch(ctx, "ivf_up_f64", n_ref * d * 8, (void**)&d_up));
    SRX_TRY(h2d(ctx, d_up, ref, n_ref * d * 8));
    return ivf_build(ctx, d_up, (size_t)d, n_ref, (int)d, o, centroids, out);
}

int32_t srx_knn_index_result(srx_mat* m, int32_t n_dims, const srx_ivf_opts* opts, srx_knn_index** out) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "knn index: null output handle");
    *out = nullptr;
    if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "no PCA result on this matrix");
    if (n_dims < 0 || (uint32_t)n_dims > m->pca.n_pc)
        return fail(ctx, SRX_E_ARG, "knn index: n_dims = %d but the scores have %u coordinates", n_dims, m->pca.n_pc);
    const uint64_t n = m->csc ? m->n_cols : m->n_rows, d = n_dims ? (uint64_t)n_dims : m->pca.n_pc;
    srx_ivf_opts o;
    SRX_TRY(ivf_opts_check(ctx, opts, n, d, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("knn_index");
    return ivf_build(ctx, m->pca.d_scores, (size_t)scores_ld((int)m->pca.n_pc), n, (int)d, o, nullptr, out);
}

int32_t srx_knn_index_info_get(const srx_knn_index* ix, srx_ivf_info* info) {
    if (!ix || !info) return fail(ix ? ix->ctx : nullptr, SRX_E_ARG, "knn index: null handle or info");
    *info = ix->info;
    return SRX_OK;
}

int32_t srx_knn_index_fetch(srx_knn_index* ix, double* centroids, uint64_t* list_offsets, uint32_t* list_members) {
    if (!ix) return fail(nullptr, SRX_E_ARG, "null knn index");
    srx_ctx* ctx = ix->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (centroids) SRX_TRY(d2h(ctx, centroids, ix->d_cent, (size_t)ix->n_lists * ix->d * 8));
    if (list_offsets)
        for (size_t l = 0; l <= ix->n_lists; ++l) list_offsets[l] = (uint64_t)ix->h_off[l];
    if (list_members) SRX_TRY(d2h(ctx, list_members, ix->d_members, ix->n_ref * 4));
    return SRX_OK;
}

int32_t srx_knn_index_search(srx_knn_index* ix, const double* query, uint64_t n_query, const srx_knn_opts* opts, int32_t n_probe,
                             uint32_t* indices_out, double* distances_out, srx_ivf_search_info* info) {
    if (!ix) return fail(nullptr, SRX_E_ARG, "null knn index");
    srx_ctx* ctx = ix->ctx;
    const bool self = query == nullptr;
    if (self) n_query = ix->n_ref;
    int np = 0;
    SRX_TRY(ivf_search_check(ix, self, n_query, opts, n_probe, &np));
    if (info) memset(info, 0, sizeof *info);
    if (n_query == 0) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("knn_index_search");
    const double* d_qry = ix->d_pts;
    if (!self) {
        double* q;
        SRX_TRY(scratch(ctx, "ivf_qry_f64", n_query * (size_t)ix->d * 8, (void**)&q));
        SRX_TRY(h2d(ctx, q, query, n_query * (size_t)ix->d * 8));
        d_qry = q;
    }
    srx_ivf_search_info si;
    SRX_TRY(ivf_search_device(ix, d_qry, (size_t)ix->d, n_query, self, opts->k, opts->include_self, np, &si));
    uint32_t* d_idx;
    double* d_dist;
    SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "knn_dist", 0, (void**)&d_dist));
    if (indices_out) SRX_TRY(d2h(ctx, indices_out, d_idx, n_query * (size_t)opts->k * 4));
    if (distances_out) SRX_TRY(d2h(ctx, distances_out, d_dist, n_query * (size_t)opts->k * 8));
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (info) *info = si;
    return SRX_OK;
}

int32_t srx_neighbors_index(srx_knn_index* ix, const srx_knn_opts* opts, int32_t n_probe, srx_ivf_search_info* info, srx_graph** out) {
    if (!ix) return fail(nullptr, SRX_E_ARG, "null knn index");
    srx_ctx* ctx = ix->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "neighbors: null output handle");
    *out = nullptr;
    if (!opts) return fail(ctx, SRX_E_ARG, "neighbors: null options");
    if (opts->include_self) return fail(ctx, SRX_E_ARG, "neighbors: the graph is built from a list that excludes self (include_self = 0)");
    int np = 0;
    SRX_TRY(ivf_search_check(ix, true, ix->n_ref, opts, n_probe, &np));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_ivf_search_info si;
    {
        Range rg("knn_index_search");
        SRX_TRY(ivf_search_device(ix, ix->d_pts, (size_t)ix->d, ix->n_ref, true, opts->k, 0, np, &si));
    }
    if (info) *info = si;
    uint32_t* d_idx;
    double* d_dist;
    SRX_TRY(scratch(ctx, "knn_idx", 0, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "knn_dist", 0, (void**)&d_dist));
    return graph_from_device_list(ctx, d_idx, d_dist, ix->n_ref, (uint32_t)opts->k, out);
}

void srx_knn_index_free(srx_knn_index* ix) { ivf_release(ix); }

}  // extern "C"
