// gene_sets.hip — per cell, the sums of the stored values over gene lists (srx_gene_list_sums), the control genes of a gene-set
// score (srx_score_genes_controls: host code alone) and the score built on the two (srx_score_genes).  include/srx.h has the
// definition; this file has one walk kernel, one finishing kernel for the score, and the host logic.
//
// The walk.  A wave walks its row's column indices alone (2 bytes per entry through the 16-bit mirror) and tests each against a 1-bit
// "in any list of this walk" bitmap in LDS (G / 8 bytes).  The hits of a 1024-entry chunk are first COMPACTED into a queue of the
// wave in LDS (ballot + lane rank), then drained 64 at a time: lane q loads the value and the gene's 64-bit membership mask (a
// G x 8 B table, L2-resident) of hit q and adds round(x 2^scale) into the accumulators of its wave, 64 lists x (i64 sum, u32
// count) in LDS, with integer LDS atomics.  The first form took the dependent value and mask loads inside the loop over the
// chunk's 16 steps; a cell-cycle input lists its ~1000 control genes per set, so 7 % of the entries are hits, every step of
// every row had one, and the 16 load latencies of a chunk ran one after another: 2.75 ms at c3 against 0.80 ms for the row sums
// (profiles/score_genes.md).  After a row, lane t converts list t: SUM = f64(S) 2^-scale, one coalesced store per row and output.
#include "markers_internal.hpp"
#include "hash.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <type_traits>
#include <vector>

// the f64 finishing arithmetic is evaluated as srx.h writes it, every operation rounded once
#pragma clang fp contract(off)

namespace srx {

constexpr int kGsWaves = 4;                    // waves per workgroup of the walk: a row per wave
constexpr int kGsWidth = 64;                   // lists per walk: the bits of a membership mask
constexpr int kGsUnroll = 16;                  // 64-entry chunks of a row in flight per wave (as k_rowcount: a ~840-entry row is one round trip)
constexpr size_t kGsBitsLds = 65536;           // the bitmap goes to LDS up to this many bytes (524288 genes), else it is read in place
constexpr int kGsChunk = kGsUnroll * kWave;   // entries of a row per round: the capacity of a wave's hit queue
constexpr size_t kGsAccLds = (size_t)kGsWaves * kGsWidth * (sizeof(long long) + sizeof(uint32_t));

// a queued hit: its place in the chunk above its gene, in 32 bits where the gene has 16
template <typename I> struct GsHit;
template <> struct GsHit<uint16_t> { using T = uint32_t; static constexpr int kShift = 16; };
template <> struct GsHit<int32_t> { using T = unsigned long long; static constexpr int kShift = 32; };
template <typename I> constexpr size_t gs_queue_lds() { return (size_t)kGsWaves * kGsChunk * sizeof(typename GsHit<I>::T); }

// rows of the matrix, one per wave at a time.  `n_here` lists of this walk are columns col0 .. of the n_lists-wide outputs.
// LDS: the sums (u64), the hit queues, the counts (u32), then the bitmap where it is staged.
template <typename I, typename V, bool LDS>
__global__ __launch_bounds__(kGsWaves * kWave) void k_gs_walk(const int64_t* __restrict__ indptr, const I* __restrict__ idx,
                                                              const V* __restrict__ vals, const uint32_t* __restrict__ g_bits, int n_words,
                                                              const unsigned long long* __restrict__ mask, uint64_t n_rows, double fx,
                                                              double inv_fx, int n_here, uint64_t n_lists, uint64_t col0,
                                                              double* __restrict__ sum_out, uint32_t* __restrict__ cnt_out) {
    using E = typename GsHit<I>::T;
    constexpr int kShift = GsHit<I>::kShift;
    extern __shared__ double lds_raw[];
    unsigned long long* s_sum = reinterpret_cast<unsigned long long*>(lds_raw);
    E* s_queue = reinterpret_cast<E*>(s_sum + kGsWaves * kGsWidth);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_queue + kGsWaves * kGsChunk);
    const uint32_t* bits = g_bits;
    const int lane = lane_id();
    const int wave_in = (int)(threadIdx.x / kWave);
    unsigned long long* my_sum = s_sum + wave_in * kGsWidth;
    uint32_t* my_cnt = s_cnt + wave_in * kGsWidth;
    E* my_queue = s_queue + wave_in * kGsChunk;
    my_sum[lane] = 0;
    my_cnt[lane] = 0;
    if constexpr (LDS) {
        uint32_t* s_bits = s_cnt + kGsWaves * kGsWidth;
        for (int e = threadIdx.x; e < n_words; e += blockDim.x) s_bits[e] = g_bits[e];
        bits = s_bits;
    }
    __syncthreads();
    const uint64_t wave = global_wave_id();
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) / kWave;
    const unsigned long long below = (1ull << lane) - 1ull;          // the lanes before this one
    // (Requesting the next chunk's indices between the queueing and the drain, so that both sets of loads are in flight together,
    //  was built and measured: 1.97 ms at c3 against 1.39 ms for this form.  Not kept.)
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const int64_t lo = indptr[r], hi = indptr[r + 1];
        for (int64_t base = lo; base < hi; base += kGsChunk) {
            int32_t g[kGsUnroll];
#pragma unroll
            for (int u = 0; u < kGsUnroll; ++u) {
                const int64_t p = base + u * kWave + lane;
                g[u] = p < hi ? (int32_t)idx[p] : -1;
            }
            // the hits of the chunk, queued in the order of the row (at most kGsChunk of them)
            uint32_t n_hit = 0;
#pragma unroll
            for (int u = 0; u < kGsUnroll; ++u) {
                const bool hit = g[u] >= 0 && ((bits[g[u] >> 5] >> (g[u] & 31)) & 1u);
                const unsigned long long who = __ballot(hit);
                if (hit) my_queue[n_hit + (uint32_t)__popcll(who & below)] = ((E)(uint32_t)(u * kWave + lane) << kShift) | (E)(uint32_t)g[u];
                n_hit += (uint32_t)__popcll(who);
            }
            wave_lds_sync();
            // 64 hits at a time: the value as round(x 2^scale), ties to even, into every list that holds the gene
            for (uint32_t q = lane; q < n_hit; q += kWave) {
                const E e = my_queue[q];
                const uint32_t gene = (uint32_t)(e & (((E)1 << kShift) - 1)), at = (uint32_t)(e >> kShift);
                unsigned long long mk = mask[gene];
                const double x = (double)vals[base + at];
                const unsigned long long fixed = (unsigned long long)(long long)__builtin_rint(x * fx);
                while (mk) {
                    const int t = __ffsll((long long)mk) - 1;
                    mk &= mk - 1;
                    atomicAdd(&my_sum[t], fixed);
                    atomicAdd(&my_cnt[t], 1u);
                }
            }
            wave_lds_sync();
        }
        const unsigned long long s = my_sum[lane];
        const uint32_t c = my_cnt[lane];
        my_sum[lane] = 0;
        my_cnt[lane] = 0;
        if (lane < n_here) {
            if (sum_out) sum_out[r * n_lists + col0 + lane] = (double)(long long)s * inv_fx;
            if (cnt_out) cnt_out[r * n_lists + col0 + lane] = c;
        }
        wave_lds_sync();
    }
}

// score[i][s] = SUM_set / |set| - SUM_ctrl / |ctrl| from the n_rows x 2 n_sets sums (the sets, then their controls)
__global__ __launch_bounds__(256) void k_gs_score(const double* __restrict__ sums, const double* __restrict__ size, uint64_t n_rows,
                                                  uint64_t n_sets, double* __restrict__ score) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_rows * n_sets) return;
    const uint64_t i = e / n_sets, s = e % n_sets;
    const double a = sums[i * 2 * n_sets + s] / size[s];
    const double b = sums[i * 2 * n_sets + n_sets + s] / size[n_sets + s];
    score[e] = a - b;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
namespace {

// refusals 1.(3)-(6) of srx.h; sets the device
int32_t gs_check_handle(srx_mat* m, const char* who) {
    srx_ctx* ctx = m->ctx;
    if (m->csc) return fail(ctx, SRX_E_ARG, "%s walks cells: convert the CSC matrix with srx_matrix_to_csr", who);
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: a context with more than one rank (the sharded form is out of scope)", who);
    if (ctx->pool_on > 0) return fail(ctx, SRX_E_ARG, "%s: a backed session is open on this context (the out-of-core form is out of scope)", who);
    if (m->n_rows >= (1ull << 32)) return fail(ctx, SRX_E_ARG, "%s: 2^32 rows or more", who);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return SRX_OK;
}

// a list of lists: ptr starts at 0 and never decreases, no list is empty, every gene is below n_genes and distinct within its
// list.  `what` names the lists in the messages ("list", "set").
int32_t gs_check_lists(srx_ctx* ctx, const char* who, const char* what, const uint64_t* ptr, const uint64_t* genes, uint64_t n, uint64_t n_genes,
                       uint64_t* longest) {
    if (ptr[0] != 0) return fail(ctx, SRX_E_ARG, "%s: %s_ptr[0] = %llu (it starts at 0)", who, what, (unsigned long long)ptr[0]);
    for (uint64_t t = 0; t < n; ++t) {
        if (ptr[t + 1] < ptr[t]) return fail(ctx, SRX_E_ARG, "%s: %s_ptr decreases at %s %llu", who, what, what, (unsigned long long)t);
        if (ptr[t + 1] == ptr[t]) return fail(ctx, SRX_E_ARG, "%s: %s %llu is empty", who, what, (unsigned long long)t);
    }
    std::vector<uint64_t> sorted;
    *longest = 0;
    for (uint64_t t = 0; t < n; ++t) {
        sorted.assign(genes + ptr[t], genes + ptr[t + 1]);
        std::sort(sorted.begin(), sorted.end());
        if (sorted.back() >= n_genes)
            return fail(ctx, SRX_E_ARG, "%s: gene index %llu of %s %llu is not below %llu", who, (unsigned long long)sorted.back(), what,
                        (unsigned long long)t, (unsigned long long)n_genes);
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end())
            return fail(ctx, SRX_E_ARG, "%s: gene %llu is repeated in %s %llu", who, (unsigned long long)*dup, what, (unsigned long long)t);
        *longest = std::max<uint64_t>(*longest, sorted.size());
    }
    return SRX_OK;
}

// max_abs over all stored values; SRX_E_NAN for a NaN or Inf
int32_t gs_value_scan(srx_mat* m, const char* who, double* max_abs) {
    srx_ctx* ctx = m->ctx;
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "gs_small", VS_WORDS * 8, (void**)&d_small));
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, VS_WORDS * 8, ctx->stream));
    value_scan(m, d_small);
    SRX_HIP(ctx, hipGetLastError());
    unsigned long long small[VS_WORDS];
    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    if (small[VS_FLAGS] & kValNonFinite) return fail(ctx, SRX_E_NAN, "%s: a stored value is NaN or Inf", who);
    memcpy(max_abs, &small[VS_MAXABS], 8);
    return SRX_OK;
}

int gs_scale_log2(double max_abs, uint64_t longest) {
    int L = 0;
    while ((1ull << L) < at_least_one(longest)) ++L;
    return 62 - fx_exponent(max_abs) - L;
}

// the walks of the checked lists: d_sum / d_cnt (n_rows x n_lists on the device; either may be null) are written in full
int32_t gs_walks(srx_mat* m, const uint64_t* list_ptr, const uint64_t* list_genes, uint64_t n_lists, int scale_log2, double* d_sum,
                 uint32_t* d_cnt, uint32_t* n_walks) {
    srx_ctx* ctx = m->ctx;
    const uint64_t N = m->n_rows, G = m->n_cols;
    *n_walks = (uint32_t)((n_lists + kGsWidth - 1) / kGsWidth);
    if (N == 0) return SRX_OK;
    const int n_words = (int)((G + 31) / 32);
    const bool in_lds = (size_t)n_words * 4 <= kGsBitsLds;
    const size_t lds = kGsAccLds + (m->d_idx16 ? gs_queue_lds<uint16_t>() : gs_queue_lds<int32_t>()) + (in_lds ? (size_t)n_words * 4 : 0);
    const double fx = std::ldexp(1.0, scale_log2), inv_fx = std::ldexp(1.0, -scale_log2);
    unsigned long long* d_mask;
    uint32_t* d_bits;
    SRX_TRY(scratch(ctx, "gs_mask", at_least_one(G) * 8, (void**)&d_mask));
    SRX_TRY(scratch(ctx, "gs_bits", (size_t)at_least_one(n_words) * 4, (void**)&d_bits));
    std::vector<unsigned long long> mask(at_least_one(G));
    std::vector<uint32_t> bits(at_least_one(n_words));
    // a wave per row; eight workgroups per CU where the LDS allows it
    const uint64_t want = (N + kGsWaves - 1) / kGsWaves;
    const uint64_t per_cu = std::max<uint64_t>(1, std::min<uint64_t>(8, (160 * 1024) / lds));
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->n_cus * per_cu));
    for (uint32_t w = 0; w < *n_walks; ++w) {
        const uint64_t t0 = (uint64_t)w * kGsWidth, t1 = std::min<uint64_t>(t0 + kGsWidth, n_lists);
        std::fill(mask.begin(), mask.end(), 0ull);
        std::fill(bits.begin(), bits.end(), 0u);
        for (uint64_t t = t0; t < t1; ++t)
            for (uint64_t e = list_ptr[t]; e < list_ptr[t + 1]; ++e) {
                const uint64_t g = list_genes[e];
                mask[g] |= 1ull << (t - t0);
                bits[g >> 5] |= 1u << (g & 31);
            }
        SRX_TRY(h2d(ctx, d_mask, mask.data(), G * 8));
        SRX_TRY(h2d(ctx, d_bits, bits.data(), (size_t)n_words * 4));
        auto launch = [&](auto kern, const auto* idxp, const auto* valp) -> int32_t {
            SRX_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(kGsWaves * kWave), lds, ctx->stream, (const int64_t*)m->d_indptr, idxp, valp,
                               (const uint32_t*)d_bits, n_words, (const unsigned long long*)d_mask, N, fx, inv_fx, (int)(t1 - t0), n_lists, t0,
                               d_sum, d_cnt);
            SRX_HIP(ctx, hipGetLastError());
            return SRX_OK;
        };
        auto by_val = [&](const auto* idxp) -> int32_t {
            using I = std::remove_cv_t<std::remove_pointer_t<decltype(idxp)>>;
            if (is_f32(m)) return in_lds ? launch(k_gs_walk<I, float, true>, idxp, (const float*)m->d_values)
                                         : launch(k_gs_walk<I, float, false>, idxp, (const float*)m->d_values);
            return in_lds ? launch(k_gs_walk<I, double, true>, idxp, (const double*)m->d_values)
                          : launch(k_gs_walk<I, double, false>, idxp, (const double*)m->d_values);
        };
        SRX_TRY(m->d_idx16 ? by_val((const uint16_t*)m->d_idx16) : by_val((const int32_t*)m->d_indices));
    }
    return SRX_OK;
}

struct GsOpts {
    uint64_t ctrl_size, n_bins, seed;
    bool as_ref;
    explicit GsOpts(const srx_score_genes_opts* o)
        : ctrl_size(o && o->ctrl_size ? o->ctrl_size : 50), n_bins(o && o->n_bins ? o->n_bins : 25), seed(o ? o->seed : 0),
          as_ref(!o || o->ctrl_as_ref != 0) {}
};

// srx.h 2., refusals (2) to (8): the control lists into ctrl_ptr / ctrl, the cuts into `cut` (UINT32_MAX outside the pool)
int32_t gs_controls(srx_ctx* ctx, const char* who, const double* mean, uint64_t G, const uint64_t* pool, uint64_t n_pool, const uint64_t* set_ptr,
                    const uint64_t* set_genes, uint64_t n_sets, const GsOpts& o, std::vector<uint64_t>& ctrl_ptr, std::vector<uint64_t>& ctrl,
                    std::vector<uint32_t>& cut, uint64_t* n_items_out, uint64_t* longest_set) {
    if (o.n_bins < 2) return fail(ctx, SRX_E_ARG, "%s: n_bins = %llu (at least 2)", who, (unsigned long long)o.n_bins);
    std::vector<uint64_t> P;          // the pool in ascending gene order
    cut.assign(at_least_one(G), UINT32_MAX);
    if (pool == nullptr) {
        P.resize(G);
        std::iota(P.begin(), P.end(), 0ull);
    } else {
        P.assign(pool, pool + n_pool);
        std::sort(P.begin(), P.end());
        if (!P.empty() && P.back() >= G)
            return fail(ctx, SRX_E_ARG, "%s: pool gene %llu is not below %llu", who, (unsigned long long)P.back(), (unsigned long long)G);
        const auto dup = std::adjacent_find(P.begin(), P.end());
        if (dup != P.end()) return fail(ctx, SRX_E_ARG, "%s: gene %llu is repeated in the pool", who, (unsigned long long)*dup);
    }
    const uint64_t np = P.size();
    const uint64_t n_items = (uint64_t)std::nearbyint((double)np / (double)(o.n_bins - 1));      // ties to even: np.round
    if (n_items == 0)
        return fail(ctx, SRX_E_ARG, "%s: n_items = rint(%llu / %llu) = 0 (fewer pool genes than half a bin)", who, (unsigned long long)np,
                    (unsigned long long)(o.n_bins - 1));
    for (uint64_t j : P)
        if (!is_finite(mean[j])) return fail(ctx, SRX_E_ARG, "%s: the mean of gene %llu is not finite", who, (unsigned long long)j);
    // rank(method="min"): 1 + the number of pool genes with a strictly smaller mean
    std::vector<uint64_t> by_mean(P);
    std::stable_sort(by_mean.begin(), by_mean.end(), [&](uint64_t a, uint64_t b) { return mean[a] < mean[b]; });
    uint32_t max_cut = 0;
    for (uint64_t a = 0, first = 0; a < np; ++a) {
        if (mean[by_mean[a]] != mean[by_mean[first]]) first = a;
        const uint32_t c = (uint32_t)((first + 1) / n_items);
        cut[by_mean[a]] = c;
        max_cut = std::max(max_cut, c);
    }
    // the genes of every cut in ascending gene order
    std::vector<std::vector<uint64_t>> bin((size_t)max_cut + 1);
    for (uint64_t j : P) bin[cut[j]].push_back(j);

    SRX_TRY(gs_check_lists(ctx, who, "set", set_ptr, set_genes, n_sets, G, longest_set));
    for (uint64_t e = 0; e < set_ptr[n_sets]; ++e)
        if (cut[set_genes[e]] == UINT32_MAX) return fail(ctx, SRX_E_ARG, "%s: gene %llu of a set is not in the pool", who, (unsigned long long)set_genes[e]);
    auto key = [&](uint64_t j) { return mix64(o.seed + kGold64 * (j + 1)); };
    ctrl_ptr.assign(1, 0);
    ctrl.clear();
    std::vector<uint64_t> own, cuts, cand, picked;
    for (uint64_t s = 0; s < n_sets; ++s) {
        own.assign(set_genes + set_ptr[s], set_genes + set_ptr[s + 1]);
        std::sort(own.begin(), own.end());
        cuts.clear();
        for (uint64_t j : own) cuts.push_back(cut[j]);
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        picked.clear();
        for (uint64_t c : cuts) {
            cand.clear();
            for (uint64_t j : bin[c])
                if (o.as_ref || !std::binary_search(own.begin(), own.end(), j)) cand.push_back(j);
            if (cand.size() > o.ctrl_size) {
                std::sort(cand.begin(), cand.end(), [&](uint64_t a, uint64_t b) {
                    const uint64_t ka = key(a), kb = key(b);
                    return ka != kb ? ka < kb : a < b;
                });
                cand.resize(o.ctrl_size);
            }
            for (uint64_t j : cand)
                if (!std::binary_search(own.begin(), own.end(), j)) picked.push_back(j);
        }
        std::sort(picked.begin(), picked.end());          // the cuts are disjoint: no gene twice
        if (picked.empty()) return fail(ctx, SRX_E_ARG, "%s: the control list of set %llu is empty", who, (unsigned long long)s);
        ctrl.insert(ctrl.end(), picked.begin(), picked.end());
        ctrl_ptr.push_back(ctrl.size());
    }
    *n_items_out = n_items;
    return SRX_OK;
}

}  // namespace
}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_gene_list_sums(srx_mat* m, const uint64_t* list_ptr, const uint64_t* list_genes, uint64_t n_lists, double* sum_out,
                           uint32_t* cnt_out, srx_gene_list_info* info) {
    const char* who = "gene_list_sums";
    if (!m || !list_ptr || !list_genes) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "%s: a null matrix or list array", who);
    srx_ctx* ctx = m->ctx;
    if (!sum_out && !cnt_out) return fail(ctx, SRX_E_ARG, "%s: no output (sum_out and cnt_out are both NULL)", who);
    if (n_lists < 1 || n_lists > SRX_GENE_LISTS_MAX)
        return fail(ctx, SRX_E_ARG, "%s: n_lists = %llu is outside 1 .. %d", who, (unsigned long long)n_lists, SRX_GENE_LISTS_MAX);
    SRX_TRY(gs_check_handle(m, who));
    uint64_t longest = 0;
    SRX_TRY(gs_check_lists(ctx, who, "list", list_ptr, list_genes, n_lists, m->n_cols, &longest));
    Range rg("gene_list_sums");
    srx_gene_list_info I{};
    I.n_rows = m->n_rows; I.n_cols = m->n_cols; I.n_lists = n_lists; I.longest_list = longest;
    StreamTimer timer(ctx, ctx->stream);
    SRX_TRY(timer.start());
    SRX_TRY(gs_value_scan(m, who, &I.max_abs));
    SRX_TRY(timer.stop(&I.ms_scan));
    I.sum_scale_log2 = gs_scale_log2(I.max_abs, longest);
    const uint64_t cells = at_least_one(m->n_rows * n_lists);
    double* d_sum = nullptr;
    uint32_t* d_cnt = nullptr;
    if (sum_out) SRX_TRY(scratch(ctx, "gs_sum", cells * 8, (void**)&d_sum));
    if (cnt_out) SRX_TRY(scratch(ctx, "gs_cnt", cells * 4, (void**)&d_cnt));
    StreamTimer walk(ctx, ctx->stream);
    SRX_TRY(walk.start());
    SRX_TRY(gs_walks(m, list_ptr, list_genes, n_lists, I.sum_scale_log2, d_sum, d_cnt, &I.n_walks));
    SRX_TRY(walk.stop(&I.ms_walk));
    if (sum_out) SRX_TRY(d2h(ctx, sum_out, d_sum, m->n_rows * n_lists * 8));
    if (cnt_out) SRX_TRY(d2h(ctx, cnt_out, d_cnt, m->n_rows * n_lists * 4));
    if (info) *info = I;
    return SRX_OK;
}

int32_t srx_score_genes_controls(const double* gene_mean, uint64_t n_genes, const uint64_t* pool, uint64_t n_pool, const uint64_t* set_ptr,
                                 const uint64_t* set_genes, uint64_t n_sets, const srx_score_genes_opts* opts, uint64_t* ctrl_ptr_out,
                                 uint64_t* ctrl_genes_out, uint64_t capacity, uint32_t* cut_out) {
    const char* who = "score_genes_controls";
    if (!gene_mean || !set_ptr || !set_genes || !ctrl_ptr_out || !ctrl_genes_out || (!pool && n_pool))
        return fail(nullptr, SRX_E_ARG, "%s: a null array", who);
    if (n_sets == 0) return fail(nullptr, SRX_E_ARG, "%s: no set", who);
    std::vector<uint64_t> ctrl_ptr, ctrl;
    std::vector<uint32_t> cut;
    uint64_t n_items = 0, longest = 0;
    SRX_TRY(gs_controls(nullptr, who, gene_mean, n_genes, pool, n_pool, set_ptr, set_genes, n_sets, GsOpts(opts), ctrl_ptr, ctrl, cut, &n_items,
                        &longest));
    if (ctrl.size() > capacity)
        return fail(nullptr, SRX_E_ARG, "%s: the control lists hold %llu genes, capacity is %llu", who, (unsigned long long)ctrl.size(),
                    (unsigned long long)capacity);
    memcpy(ctrl_ptr_out, ctrl_ptr.data(), ctrl_ptr.size() * 8);
    memcpy(ctrl_genes_out, ctrl.data(), ctrl.size() * 8);
    if (cut_out) memcpy(cut_out, cut.data(), n_genes * 4);
    return SRX_OK;
}

int32_t srx_score_genes(srx_mat* m, const uint64_t* set_ptr, const uint64_t* set_genes, uint64_t n_sets, const uint64_t* pool, uint64_t n_pool,
                        const srx_score_genes_opts* opts, double* score_out, uint64_t* ctrl_ptr_out, uint64_t* ctrl_genes_out, uint64_t capacity,
                        srx_score_genes_info* info) {
    const char* who = "score_genes";
    if (!m || !set_ptr || !set_genes) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "%s: a null matrix or set array", who);
    srx_ctx* ctx = m->ctx;
    if (!score_out || (!pool && n_pool) || (!ctrl_ptr_out != !ctrl_genes_out))
        return fail(ctx, SRX_E_ARG, "%s: a null array (score_out; pool with n_pool > 0; one control output without the other)", who);
    if (n_sets < 1 || n_sets > SRX_GENE_LISTS_MAX / 2)
        return fail(ctx, SRX_E_ARG, "%s: n_sets = %llu is outside 1 .. %d", who, (unsigned long long)n_sets, SRX_GENE_LISTS_MAX / 2);
    SRX_TRY(gs_check_handle(m, who));
    Range rg("score_genes");
    const uint64_t N = m->n_rows, G = m->n_cols;
    srx_score_genes_info I{};
    I.n_rows = N; I.n_cols = G; I.n_sets = n_sets;

    // -- the values (SRX_E_NAN) and the gene means
    StreamTimer t_mean(ctx, ctx->stream);
    SRX_TRY(t_mean.start());
    SRX_TRY(gs_value_scan(m, who, &I.max_abs));
    std::vector<double> mean(at_least_one(G));
    SRX_TRY(srx_compute_sum(m, SRX_COLUMN, mean.data()));
    for (uint64_t j = 0; j < G; ++j) mean[j] = mean[j] / (double)N;
    SRX_TRY(t_mean.stop(&I.ms_mean));

    // -- the control genes
    StreamTimer t_ctrl(ctx, ctx->stream);
    SRX_TRY(t_ctrl.start());
    std::vector<uint64_t> ctrl_ptr, ctrl;
    std::vector<uint32_t> cut;
    uint64_t longest = 0;
    SRX_TRY(gs_controls(ctx, who, mean.data(), G, pool, n_pool, set_ptr, set_genes, n_sets, GsOpts(opts), ctrl_ptr, ctrl, cut, &I.n_items, &longest));
    if (ctrl_genes_out && ctrl.size() > capacity)
        return fail(ctx, SRX_E_ARG, "%s: the control lists hold %llu genes, capacity is %llu", who, (unsigned long long)ctrl.size(),
                    (unsigned long long)capacity);
    SRX_TRY(t_ctrl.stop(&I.ms_ctrl));
    I.n_pool = pool ? n_pool : G;
    I.n_ctrl_total = ctrl.size();

    // -- 2 n_sets lists: the sets, then their controls
    const uint64_t n_lists = 2 * n_sets, n_set_genes = set_ptr[n_sets];
    std::vector<uint64_t> list_ptr(n_lists + 1), list_genes(set_genes, set_genes + n_set_genes);
    list_genes.insert(list_genes.end(), ctrl.begin(), ctrl.end());
    std::vector<double> size(n_lists);
    for (uint64_t s = 0; s <= n_sets; ++s) list_ptr[s] = set_ptr[s];
    for (uint64_t s = 1; s <= n_sets; ++s) list_ptr[n_sets + s] = n_set_genes + ctrl_ptr[s];
    for (uint64_t t = 0; t < n_lists; ++t) {
        size[t] = (double)(list_ptr[t + 1] - list_ptr[t]);
        longest = std::max(longest, list_ptr[t + 1] - list_ptr[t]);
    }
    I.longest_list = longest;
    I.sum_scale_log2 = gs_scale_log2(I.max_abs, longest);
    double *d_sum, *d_size, *d_score;
    SRX_TRY(scratch(ctx, "gs_sum", at_least_one(N * n_lists) * 8, (void**)&d_sum));
    SRX_TRY(scratch(ctx, "gs_size", n_lists * 8, (void**)&d_size));
    SRX_TRY(scratch(ctx, "gs_score", at_least_one(N * n_sets) * 8, (void**)&d_score));
    StreamTimer t_walk(ctx, ctx->stream);
    SRX_TRY(t_walk.start());
    SRX_TRY(gs_walks(m, list_ptr.data(), list_genes.data(), n_lists, I.sum_scale_log2, d_sum, nullptr, &I.n_walks));
    SRX_TRY(h2d(ctx, d_size, size.data(), n_lists * 8));
    if (N) {
        hipLaunchKernelGGL(k_gs_score, dim3(grid256(N * n_sets)), dim3(256), 0, ctx->stream, (const double*)d_sum, (const double*)d_size, N, n_sets,
                           d_score);
        SRX_HIP(ctx, hipGetLastError());
    }
    SRX_TRY(t_walk.stop(&I.ms_walk));
    SRX_TRY(d2h(ctx, score_out, d_score, N * n_sets * 8));
    if (ctrl_genes_out) {
        memcpy(ctrl_ptr_out, ctrl_ptr.data(), ctrl_ptr.size() * 8);
        memcpy(ctrl_genes_out, ctrl.data(), ctrl.size() * 8);
    }
    if (info) *info = I;
    return SRX_OK;
}

}  // extern "C"
