// select.hip — FeatureSelection::HighlyVariable(n) and explicit lists: the ranking of the per-gene variances on the device
// (variances, candidates from a sampled threshold, ranks by counting, then ONE workgroup that makes the selection bitmask, the
// selected genes in selection order and the PCA's centring / scaling vectors), the host ranking outside its envelope, and
// srx_select_hvg.  Reads the global moments genes.hip leaves on the matrix (d_cnt / d_sum / d_sq, n_rows_global).
#include "pca_internal.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cmath>

// csr.rs:179-185 and pca/mod.rs:87-91 are evaluated in the reference's operation order (no FMA contraction)
#pragma clang fp contract(off)

namespace srx {


// dim_red/mod.rs:135-140.  Rust's sort_by is stable; comparator b.partial_cmp(a) = descending.
static int32_t select_hvg_host(srx_ctx* ctx, const std::vector<double>& var, uint64_t n, std::vector<uint64_t>& out) {
    for (double v : var)
        if (v != v) return fail(ctx, SRX_E_NAN, "%s", kNanVarianceMsg);
    // stable descending order == the strict total order (variance desc, gene index asc), so a
    // partial sort of the first n under that order gives exactly the stable sort's prefix
    std::vector<uint64_t> order(var.size());
    for (uint64_t j = 0; j < order.size(); ++j) order[j] = j;
    uint64_t take = n < order.size() ? n : order.size();
    auto before = [&](uint64_t a, uint64_t b) { return var[a] > var[b] || (var[a] == var[b] && a < b); };
    std::nth_element(order.begin(), order.begin() + (take ? take - 1 : 0), order.end(), before);
    std::sort(order.begin(), order.begin() + take, before);
    out.assign(order.begin(), order.begin() + take);
    return SRX_OK;
}

// ---- FeatureSelection::HighlyVariable(n) on the device (the pipeline's route: no host round trip) ----
// Same semantics as select_hvg_host / dim_red/mod.rs:135-140: nz-only population variance in the reference's
// operation order (csr.rs:179-185: no FMA contraction — this file's operators under the pragma), stable descending order
// (ties keep the ascending gene index), NaN -> status bit 1 (the reference panics).
__global__ void k_gene_var(const uint64_t* __restrict__ cnt, const double* __restrict__ sum, const double* __restrict__ sq,
                           uint64_t G, double* __restrict__ var, uint32_t* __restrict__ rank, uint32_t rank_init) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    double v = 0.0;
    if (cnt[j] > 0) {
        const double c = (double)(uint32_t)cnt[j];
        // plain operators: the pragma above covers them.  (The runtime's __dmul_rn / __dsub_rn are operators of a header read
        // before the pragma: their results stayed contractable, and sq / c - mean * mean was ONE v_fma_f64.)
        const double mean = sum[j] / c;
        const double mm = mean * mean;
        v = sq[j] / c - mm;
    }
    var[j] = v;
    rank[j] = rank_init;          // (candidate route: 0xffffffff = not a candidate; full ranking: the partial ranks start at 0)
}

// rank of every gene under (variance desc, index asc) by counting.  Block (x, y): genes 256 x .. 256 x + 255
// against the comparison slice y (kRankTile variances staged in LDS, read as broadcast b128 pairs); a tile
// wholly before the block's genes wins ties (>=), wholly after loses them (>), only the tile holding the
// block's own genes needs the index compare.  Partial ranks are summed with integer atomics (exact, any order).
constexpr int kRankTile = 2048;
// one (block of 256 genes, comparison tile) pair of the full ranking; `tile`: kRankTile doubles of LDS; all 256 threads
__device__ __forceinline__ void full_rank_pair(const double* __restrict__ var, uint32_t G, uint32_t* __restrict__ rank_out, uint32_t bx,
                                               uint32_t by, double* tile) {
    const uint32_t j = bx * 256 + threadIdx.x;
    const uint32_t base = by * kRankTile;
    for (uint32_t e = threadIdx.x; e < kRankTile; e += 256) tile[e] = base + e < G ? var[base + e] : -INFINITY;
    __syncthreads();
    if (j < G) {
        const double mine = var[j];
        const uint32_t j_lo = bx * 256, j_hi = j_lo + 255;
        uint32_t rank = 0;
        if (base + kRankTile - 1 < j_lo) {                       // every gene of the tile precedes every gene of the block
#pragma unroll 8
            for (int e = 0; e < kRankTile; ++e) rank += tile[e] >= mine ? 1u : 0u;
        } else if (base > j_hi) {
#pragma unroll 8
            for (int e = 0; e < kRankTile; ++e) rank += tile[e] > mine ? 1u : 0u;
        } else {
#pragma unroll 4
            for (int e = 0; e < kRankTile; ++e) {
                const double o = tile[e];
                rank += (o > mine || (o == mine && base + e < j)) ? 1u : 0u;
            }
        }
        atomicAdd(&rank_out[j], rank);
    }
    __syncthreads();                                             // (the tile is re-filled by the caller's next pair)
}
__global__ __launch_bounds__(256) void k_hvg_rank(const double* __restrict__ var, uint32_t G, uint32_t* __restrict__ rank_out) {
    __shared__ double tile[kRankTile];
    full_rank_pair(var, G, rank_out, blockIdx.x, blockIdx.y, tile);
}

// ---- the same ranks for the genes that can be selected only --------------------------------------------------------------
// HighlyVariable(n) needs the ranks below n.  A threshold taken from a SAMPLE of the variances (512 of them, the sample
// quantile n / G pushed down by four standard deviations of a sample quantile) leaves ~n + 10 % of G candidates; they are
// ranked among themselves, every gene below the threshold keeps rank 0xffffffff.  If the sample misled (fewer than n
// candidates: probability ~3e-5 per call; more than `cap`, the size the candidate kernel is launched for; NaN variances)
// the full ranking runs instead — decided on the device.
// O(M^2) instead of O(G^2) comparisons: 173 -> ~25 us at 28k genes, n = 2000.
constexpr int kRankSample = 512;
constexpr int kSelThreads = 1024;
// One workgroup: the threshold from the sample, the candidate list (gene ids in any order: the ranks are a strict total order),
// rank_out[candidate] = 0, and the decision: `counter` = number of candidates M if n <= M <= cap, else 0xffffffff with
// rank_out zeroed for EVERY gene — the full ranking takes over in k_rank_selected.  (Round 5: threshold, gather, the fallback's
// reset and its early-exit launch were four kernels of 5-17 us each on the step's critical path.)
__global__ __launch_bounds__(kSelThreads) void k_hvg_candidates(const double* __restrict__ var, uint32_t G, uint32_t n, uint32_t cap,
                                                                uint32_t* __restrict__ counter, uint32_t* __restrict__ cand,
                                                                uint32_t* __restrict__ rank_out,
                                                                int force_miss /* test switch: a threshold nothing reaches */) {
    __shared__ double sv[kRankSample];
    __shared__ double s_thr;
    __shared__ uint32_t s_cnt;
    const uint32_t S = G < (uint32_t)kRankSample ? G : (uint32_t)kRankSample;
    const uint32_t t = threadIdx.x, lane = t & 63;
    if (t < (uint32_t)kRankSample) sv[t] = t < S ? var[(uint64_t)t * G / S] : -INFINITY;
    if (t == 0) {
        s_thr = force_miss ? INFINITY : -INFINITY;      // every gene a candidate unless a sample element says otherwise
        s_cnt = 0u;
    }
    __syncthreads();
    if (!force_miss && S == (uint32_t)kRankSample) {          // (uniform)
        const double q = (double)n / (double)G;
        const double kq = (q + 4.0 * sqrt(q * (1.0 - q) / (double)S)) * (double)S + 1.0;
        // the sample in descending order (bitonic network in LDS, 256 compare-exchanges per step: ranking every element against
        // every other one took 17 us of one workgroup); equal values may stand in any order — the threshold is a VALUE
        for (uint32_t size = 2; size <= (uint32_t)kRankSample; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                if (t < (uint32_t)kRankSample / 2) {
                    const uint32_t lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const double a = sv[lo], b = sv[hi];
                    if (desc ? a < b : a > b) {
                        sv[lo] = b;
                        sv[hi] = a;
                    }
                }
                __syncthreads();
            }
        if (t == 0 && kq < (double)(S - 1)) s_thr = sv[(uint32_t)kq];       // (NaN variances in the sample: whatever stands there — the status word reports them)
    }
    __syncthreads();
    const double thr = s_thr;
    constexpr int kAhead = 8;                 // variances of eight rounds in flight (a round per load was 0.5 us of latency each)
    for (uint32_t base = 0; base < G; base += kSelThreads * kAhead) {
        double v[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            const uint32_t j = base + a * kSelThreads + t;
            v[a] = j < G ? var[j] : -INFINITY;
        }
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            const uint32_t j = base + a * kSelThreads + t;
            const bool in = j < G && v[a] >= thr;
            const unsigned long long m = __ballot(in);
            uint32_t at = 0;
            if (lane == 0 && m) at = atomicAdd(&s_cnt, (uint32_t)__popcll(m));
            at = __shfl(at, 0, 64);
            if (in) {
                cand[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = j;
                rank_out[j] = 0u;
            }
        }
    }
    __syncthreads();
    const uint32_t M = s_cnt;
    const bool ok = M >= n && M <= cap;
    if (!ok)
        for (uint32_t j = t; j < G; j += kSelThreads) rank_out[j] = 0u;          // the full ranking's partial sums start from zero
    if (t == 0) *counter = ok ? M : 0xffffffffu;
}
// rank_out[gene] for every candidate: candidates above it under (variance desc, index asc).  Pair (x, y): candidates 256 x ..
// against the y-th tile of kCandTile of the candidate list; partial ranks are summed with integer atomics.  Where the
// candidates cannot be used (`counter` = 0xffffffff: fewer than n, more than the list the launch was sized for, NaN variances)
// the same workgroups walk the pairs of the FULL ranking instead.
constexpr int kCandTile = 128;      // (512: 44 us per launch at c3 — each thread walks a whole tile; 128: four times the workgroups, a quarter of the walk)
__global__ __launch_bounds__(256) void k_rank_selected(const double* __restrict__ var, uint32_t G, const uint32_t* __restrict__ counter,
                                                       const uint32_t* __restrict__ cand, uint32_t* __restrict__ rank_out) {
    __shared__ double tile[kRankTile];
    const uint32_t M = *counter;
    if (M == 0xffffffffu) {
        const uint32_t gb = (G + 255) / 256, gy = (G + kRankTile - 1) / kRankTile;
        for (uint32_t p = blockIdx.y * gridDim.x + blockIdx.x; p < gb * gy; p += gridDim.x * gridDim.y)
            full_rank_pair(var, G, rank_out, p % gb, p / gb, tile);
        return;
    }
    double* tv = tile;
    uint32_t* ti = reinterpret_cast<uint32_t*>(tile + kCandTile);
    const uint32_t base = blockIdx.y * kCandTile;
    if (blockIdx.x * 256 >= M || base >= M) return;           // (uniform)
    for (uint32_t e = threadIdx.x; e < kCandTile; e += 256) {
        const uint32_t g = base + e < M ? cand[base + e] : 0xffffffffu;
        ti[e] = g;
        tv[e] = g != 0xffffffffu ? var[g] : -INFINITY;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const uint32_t gi = cand[i];
    const double mine = var[gi];
    uint32_t rank = 0;
#pragma unroll 4
    for (int e = 0; e < kCandTile; ++e) {
        const double o = tv[e];
        rank += (o > mine || (o == mine && ti[e] < gi)) ? 1u : 0u;
    }
    if (rank) atomicAdd(&rank_out[gi], rank);
}

// One workgroup: selection bitmask + per-word prefix counts (what the compaction kernels read), the selected genes in
// selection order, and the per-slot (ascending gene order) centring / scaling vectors of the PCA from the all-cells moments
// (pca/mod.rs:87-91: mean = sum/N, var = sumsq/N - mean^2, ddof 0); trace = sum_s dinv_s^2 ss_s, summed in a fixed tree.
// `rank`: per gene its place in the selection, 0xffffffff for none — the HighlyVariable(n) ranking or the positions in an
// explicit list (select_list).  `gene_var` null: no NaN test (an explicit list: the reference only panics on NaN when it
// sorts); `sum` null: no vectors.  LDS: the bits and prefix counts are made in LDS (n_words <= 2048: G <= 65536), else in
// place in global memory.
constexpr int kSelLdsWords = 2048;
template <bool LDS>
__global__ __launch_bounds__(1024) void k_sel_finish(const uint32_t* __restrict__ rank, const double* __restrict__ gene_var,
                                                     const double* __restrict__ sum,
                                                     const double* __restrict__ sq, uint32_t G, uint32_t take, int n_words,
                                                     double n_cells, int center, int scale, int32_t* __restrict__ sel_rank,
                                                     int* __restrict__ status, uint32_t* __restrict__ bits,
                                                     uint32_t* __restrict__ prefix, double* __restrict__ mu,
                                                     double* __restrict__ sd, double* __restrict__ dinv,
                                                     double* __restrict__ trace) {
    __shared__ uint32_t s_bits[LDS ? kSelLdsWords : 1], s_pre[LDS ? kSelLdsWords : 1], s_wave[16];
    __shared__ double s_tr[1024];
    __shared__ int s_nan;
    uint32_t* const wbits = LDS ? s_bits : bits;
    uint32_t* const wpre = LDS ? s_pre : prefix;
    const int t = threadIdx.x, lane = t & 63;
    if (t == 0) s_nan = 0;
    __syncthreads();
    // the gene of rank r < take goes to sel_rank[r] and into the mask (two words per thread); a NaN variance anywhere is the
    // status word's bit 0 (the reference panics there: select_hvg_host)
    bool nan = false;
    constexpr int kAhead = 8;                 // (the loads of eight rounds in flight)
    for (uint32_t base = 0; base < (uint32_t)n_words * 32; base += 1024 * kAhead) {       // (a wave: 64 consecutive genes = two mask words)
        uint32_t rk[kAhead];
        double v[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            const uint32_t g = base + a * 1024 + t;
            rk[a] = g < G ? rank[g] : 0xffffffffu;
            v[a] = g < G && gene_var ? gene_var[g] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < kAhead; ++a) {
            const uint32_t g = base + a * 1024 + t;
            nan |= v[a] != v[a];
            const bool in = rk[a] < take;      // (a gene behind G: 0xffffffff, never below `take`)
            if (in) sel_rank[rk[a]] = (int32_t)g;
            const unsigned long long m = __ballot(in);
            if (lane == 0 && (g >> 5) < (uint32_t)n_words) wbits[g >> 5] = (uint32_t)m;
            if (lane == 32 && (g >> 5) < (uint32_t)n_words) wbits[g >> 5] = (uint32_t)(m >> 32);
        }
    }
    if (nan) s_nan = 1;
    __syncthreads();
    // exclusive scan of the popcounts, 2048 words per round: per-thread pair, wave scan, wave totals
    uint32_t carry = 0;
    for (int w0 = 0; w0 < n_words; w0 += 2 * 1024) {
        const int w = w0 + 2 * t;
        uint32_t b[2] = {0u, 0u};
        if (w < n_words) b[0] = wbits[w];
        if (w + 1 < n_words) b[1] = wbits[w + 1];
        const uint32_t c0 = (uint32_t)__popc(b[0]), c1 = (uint32_t)__popc(b[1]);
        uint32_t round_total;
        const uint32_t excl = carry + block_scan_exclusive<16>(c0 + c1, s_wave, round_total);
        if (w < n_words) wpre[w] = excl;
        if (w + 1 < n_words) wpre[w + 1] = excl + c0;
        carry += round_total;
        __syncthreads();
    }
    // never more than `take` selected genes, whatever the flags say (a ranking broken by NaN variances can flag more): the
    // passes over the matrix test the bit alone and the compacted columns must stay below `take`
    for (int w = t; w < n_words; w += 1024) {
        uint32_t b_ = wbits[w];
        const uint32_t e = wpre[w], room = e < take ? take - e : 0u;
        while ((uint32_t)__popc(b_) > room) b_ &= ~(1u << (31 - __clz((int)b_)));
        wbits[w] = b_;
    }
    __syncthreads();
    if constexpr (LDS)
        for (int w = t; w < n_words; w += 1024) {
            bits[w] = s_bits[w];
            prefix[w] = s_pre[w];
        }
    double tr = 0.0;
    for (uint32_t g = t; sum && g < G; g += 1024) {
        const uint32_t w = wbits[g >> 5];
        if (!((w >> (g & 31)) & 1u)) continue;
        const uint32_t s = bitmap_rank_word(w, wpre, g);
        const double mean = sum[g] / n_cells;
        double var = sq[g] / n_cells - mean * mean;
        if (var < 0) var = 0;
        const double std_ = sqrt(var);
        mu[s] = (center || scale) ? mean : 0.0;          // pca/mod.rs:85-119: stored only if center || scale
        sd[s] = scale ? std_ : 1.0;
        const double di = (scale && std_ > 0) ? 1.0 / std_ : 1.0;      // zero-variance column: std treated as 1
        dinv[s] = di;
        double ss = center ? (sq[g] - n_cells * mean * mean) : sq[g];
        if (ss < 0) ss = 0;
        tr += di * di * ss;
    }
    s_tr[t] = tr;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if (t < half) s_tr[t] += s_tr[t + half];
        __syncthreads();
    }
    if (t == 0) {
        if (sum) *trace = s_tr[0];                      // (`sum` null: no vectors — the trace is one of them)
        *status = s_nan;
    }
}

// The buffers of a selection of `take` of G genes (context scratch, read by the PCA that follows: a backed session keeps them
// from its selection to its solve), and the per-gene rank table k_sel_finish reads.
static int32_t sel_buffers(srx_ctx* ctx, uint64_t G, uint64_t take, SelDev& out, uint32_t** d_rank) {
    const int n_words = (int)((G + 31) / 32);
    double* d_f;
    SRX_TRY(scratch(ctx, "hvg_rankv", at_least_one(G) * sizeof(uint32_t), (void**)d_rank));
    SRX_TRY(scratch(ctx, "hvg_rank", at_least_one(take) * sizeof(int32_t), (void**)&out.d_sel_rank));
    SRX_TRY(scratch(ctx, "pca_selbits", at_least_one(2 * n_words) * sizeof(uint32_t), (void**)&out.d_bits));
    SRX_TRY(scratch(ctx, "hvg_f", (3 * at_least_one(take) + 8) * sizeof(double), (void**)&d_f));
    SRX_TRY(scratch(ctx, "hvg_status", 256, (void**)&out.d_status));
    out.d_mu = d_f;
    out.d_sd = d_f + take;
    out.d_dinv = d_f + 2 * take;
    out.d_trace = d_f + 3 * take;
    out.k = (int)take;
    out.n_words = n_words;
    return SRX_OK;
}

// `d_prefix`: the n_words prefix counts (the pipeline keeps them behind the bits: out.d_bits + out.n_words)
static int32_t launch_sel_finish(srx_ctx* ctx, const uint32_t* d_rank, const double* d_var, const double* d_sum, const double* d_sq, uint64_t G,
                                 double n_cells, int center, int scale, const SelDev& out, uint32_t* d_prefix) {
    auto kern = out.n_words <= kSelLdsWords ? k_sel_finish<true> : k_sel_finish<false>;
    hipLaunchKernelGGL(kern, dim3(1), dim3(1024), 0, ctx->stream, d_rank, d_var, d_sum, d_sq, (uint32_t)G, (uint32_t)out.k, out.n_words,
                       n_cells, center, scale, out.d_sel_rank, out.d_status, out.d_bits, d_prefix, out.d_mu, out.d_sd, out.d_dinv,
                       out.d_trace);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// the device ranking's envelope: G <= 65536 (the fallback rank kernel is O(G^2)) and take <= kDevSelMaxK (what it is tested in)
bool hvg_on_device(uint64_t n, uint64_t n_cols) {
    return n > 0 && std::min(n, n_cols) <= kDevSelMaxK && n_cols <= 65536;
}

// The work buffers of the device ranking beside the SelDev: G variances, the G-entry rank table, the candidate list (G entries)
// and its counter word, the prefix counts.
struct SelWork {
    double* d_var = nullptr;
    uint32_t *d_rank = nullptr, *d_cand = nullptr, *d_counter = nullptr, *d_prefix = nullptr;
};
enum { kRouteAuto = 0, kRouteFull = 1, kRouteMiss = 2 };      // (srx_select_args.route)
// Device-side HighlyVariable(n) on device pointers: the four launches: variances; threshold + candidate list + the decision;
// the ranks; mask, vectors, status.  `take` = min(n, G); `route`: kRouteFull ranks every gene, kRouteMiss gives
// k_hvg_candidates a threshold nothing reaches (the device-side fallback).  d_cand / d_counter are read on the candidate route only.
static int32_t hvg_launches(srx_ctx* ctx, const uint64_t* d_cnt, const double* d_sum, const double* d_sq, uint64_t G, uint64_t take,
                            double n_cells, int center, int scale, int route, const SelWork& w, const SelDev& out) {
    const unsigned gb = (unsigned)at_least_one((G + 255) / 256);
    const unsigned gy = (unsigned)at_least_one((G + kRankTile - 1) / kRankTile);
    const bool all = route == kRouteFull || take == 0 || G < (uint64_t)kRankSample;
    hipLaunchKernelGGL(k_gene_var, dim3(gb), dim3(256), 0, ctx->stream, d_cnt, d_sum, d_sq, G, w.d_var, w.d_rank, all ? 0u : 0xffffffffu);
    if (all) {
        hipLaunchKernelGGL(k_hvg_rank, dim3(gb, gy), dim3(256), 0, ctx->stream, w.d_var, (uint32_t)G, w.d_rank);
    } else {
        const uint32_t cap = (uint32_t)std::min<uint64_t>(G, std::max<uint64_t>(4 * take, 4096));
        hipLaunchKernelGGL(k_hvg_candidates, dim3(1), dim3(kSelThreads), 0, ctx->stream, w.d_var, (uint32_t)G, (uint32_t)take, cap, w.d_counter,
                           w.d_cand, w.d_rank, route == kRouteMiss ? 1 : 0);
        hipLaunchKernelGGL(k_rank_selected, dim3((cap + 255) / 256, (cap + kCandTile - 1) / kCandTile), dim3(256), 0, ctx->stream, w.d_var,
                           (uint32_t)G, w.d_counter, w.d_cand, w.d_rank);
    }
    return launch_sel_finish(ctx, w.d_rank, w.d_var, d_sum, d_sq, G, n_cells, center, scale, out, w.d_prefix);
}

// Device-side HighlyVariable(n): fills the scratch buffers named in sel_buffers; nothing is read back.
int32_t select_hvg_device(srx_mat* m, uint64_t n, int center, int scale, SelDev& out) {
    srx_ctx* ctx = m->ctx;
    const uint64_t G = m->n_cols;
    const uint64_t take = n < G ? n : G;
    SelWork w;
    SRX_TRY(scratch(ctx, "hvg_var", at_least_one(G) * sizeof(double), (void**)&w.d_var));
    SRX_TRY(sel_buffers(ctx, G, take, out, &w.d_rank));
    w.d_prefix = out.d_bits + out.n_words;
    static const bool full_rank = getenv("SRX_HVG_FULL_RANK") != nullptr;       // A/B switch: rank every gene
    static const int force_miss = getenv("SRX_HVG_FORCE_MISS") ? 1 : 0;         // exercises the device-side fallback
    // every buffer is asked for before the first launch: where scratch() grows one (hipFree + hipMalloc, which wait for the
    // device), it does so ahead of k_gene_var, not between it and k_hvg_candidates
    if (!(full_rank || take == 0 || G < (uint64_t)kRankSample)) {
        SRX_TRY(scratch(ctx, "hvg_cand", (at_least_one(G) + 8) * sizeof(uint32_t), (void**)&w.d_cand));
        w.d_counter = w.d_cand + G + 4;
    }
    return hvg_launches(ctx, m->d_cnt, m->d_sum, m->d_sq, G, take, (double)m->n_rows_global, center, scale,
                        full_rank ? kRouteFull : force_miss ? kRouteMiss : kRouteAuto, w, out);
}

// The ranking alone, for any key array (pearson.hip): d_rank[j] += the number of genes before j under (key desc, index asc);
// the caller has zeroed d_rank.  The full ranking: a key array has no sampled threshold to trust.
int32_t rank_keys_device(srx_ctx* ctx, const double* d_key, uint64_t G, uint32_t* d_rank) {
    if (G == 0) return SRX_OK;
    hipLaunchKernelGGL(k_hvg_rank, dim3((unsigned)((G + 255) / 256), (unsigned)((G + kRankTile - 1) / kRankTile)), dim3(256), 0, ctx->stream,
                       d_key, (uint32_t)G, d_rank);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// The first `take` of a full ranking: d_sel[rank] = gene for every gene with rank < take
__global__ __launch_bounds__(256) void k_pick_top(const uint32_t* __restrict__ rank, uint64_t G, uint32_t take, uint64_t* __restrict__ sel) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < G && rank[j] < take) sel[rank[j]] = j;
}
int32_t pick_top(srx_ctx* ctx, const uint32_t* d_rank, uint64_t G, uint64_t take, uint64_t* d_sel) {
    hipLaunchKernelGGL(k_pick_top, dim3(grid256(G)), dim3(256), 0, ctx->stream, d_rank, G, (uint32_t)take, d_sel);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// An explicit list: its rank table is the position of every gene in the list, so that the selection comes out in the
// caller's order (1.2 MB to upload at 300 000 columns).  Needs the global moments of `m` where `vectors`.
static int32_t list_rank_table(srx_ctx* ctx, const uint64_t* genes, uint64_t k, uint64_t G, std::vector<uint32_t>& rank) {
    rank.assign(G, 0xffffffffu);
    for (uint64_t s = 0; s < k; ++s) {
        const uint64_t g = genes ? genes[s] : s;
        if (g >= G) return fail(ctx, SRX_E_BOUNDS, "selected feature index %llu out of bounds (n_vars = %llu)",
                                (unsigned long long)g, (unsigned long long)G);
        if (rank[g] != 0xffffffffu) return fail(ctx, SRX_E_ARG, "selected feature index %llu appears twice", (unsigned long long)g);
        rank[g] = (uint32_t)s;
    }
    return SRX_OK;
}
int32_t select_list(srx_mat* m, const uint64_t* genes, uint64_t k, int center, int scale, SelDev& out, bool vectors) {
    srx_ctx* ctx = m->ctx;
    const uint64_t G = m->n_cols;
    std::vector<uint32_t> rank;
    SRX_TRY(list_rank_table(ctx, genes, k, G, rank));
    uint32_t* d_rank;
    SRX_TRY(sel_buffers(ctx, G, k, out, &d_rank));
    SRX_TRY(h2d(ctx, d_rank, rank.data(), G * sizeof(uint32_t)));
    return launch_sel_finish(ctx, d_rank, nullptr, vectors ? m->d_sum : nullptr, m->d_sq, G, (double)m->n_rows_global, center, scale, out,
                             out.d_bits + out.n_words);
}

int32_t hvg_list_host(srx_mat* m, uint64_t n, std::vector<uint64_t>& out) {
    std::vector<double> var;
    if (m->csc) {                                // compute_variance(Column) of a CSC matrix: csc.rs:164-177 (NaN for an empty gene)
        var.resize(m->n_rows);
        SRX_TRY(row_stat(m, 1, var.data(), nullptr));
    } else {
        SRX_TRY(gene_variances(m, var));
    }
    return select_hvg_host(m->ctx, var, n, out);
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_select_hvg(srx_mat* m, uint64_t n, uint64_t* idx_out, uint64_t* n_out) {
    if (!m || !n_out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    std::vector<uint64_t> sel;
    SRX_TRY(hvg_list_host(m, n, sel));
    if (idx_out) memcpy(idx_out, sel.data(), sel.size() * sizeof(uint64_t));
    *n_out = sel.size();
    return SRX_OK;
}

// Kernel-level entry point of the selection (test and diagnostics: no stability promise): hvg_launches / select_list's table and
// k_sel_finish on host arrays, in fresh device buffers of exactly the stated sizes, each followed by kSelTail sentinel elements
// that must come back untouched.
namespace {
constexpr size_t kSelTail = 8;
constexpr unsigned char kSelSentinelByte = 0xa5;
struct SelBufs {                                   // the device buffers of one call, freed when it returns
    std::vector<void*> p;
    ~SelBufs() {
        for (void* q : p) (void)hipFree(q);
    }
};
// `n` elements of `elem` bytes from `host` (null: sentinel bytes there too) + the tail
int32_t sel_up(srx_ctx* ctx, SelBufs& bufs, const void* host, size_t n, size_t elem, void** dev) {
    SRX_HIP(ctx, hipMalloc(dev, (n + kSelTail) * elem));
    bufs.p.push_back(*dev);
    std::vector<unsigned char> h((n + kSelTail) * elem, kSelSentinelByte);
    if (host) memcpy(h.data(), host, n * elem);
    return h2d(ctx, *dev, h.data(), h.size());
}
int32_t sel_down(srx_ctx* ctx, void* host, const void* dev, size_t n, size_t elem, int bit, int32_t* touched) {
    std::vector<unsigned char> h((n + kSelTail) * elem);
    SRX_TRY(d2h(ctx, h.data(), dev, h.size()));
    if (host) memcpy(host, h.data(), n * elem);
    for (size_t e = n * elem; e < h.size(); ++e)
        if (h[e] != kSelSentinelByte) *touched |= 1 << bit;
    return SRX_OK;
}
}  // namespace

int32_t srx_select_op(srx_ctx* ctx, srx_select_args* a) {
    if (!ctx || !a) return fail(ctx, SRX_E_ARG, "srx_select_op: null argument");
    const bool list = a->op == SRX_SEL_LIST;
    if (a->op != SRX_SEL_HVG && !list) return fail(ctx, SRX_E_ARG, "srx_select_op: unknown op %d", a->op);
    const bool vectors = !(list && (a->flags & SRX_SEL_NO_VECTORS));
    const uint64_t G = a->G;
    if (G == 0 || a->take == 0) return fail(ctx, SRX_E_ARG, "srx_select_op: G and take must be >= 1");
    if (!a->rank || !a->sel_rank || !a->bits || !a->prefix || (vectors && (!a->sum || !a->sq || !a->mu || !a->sd || !a->dinv)))
        return fail(ctx, SRX_E_ARG, "srx_select_op: null array");
    std::vector<uint32_t> table;
    if (list) {
        if (!a->genes) return fail(ctx, SRX_E_ARG, "srx_select_op: null gene list");
        // a matrix has fewer than 2^31 columns (upload_on): the rank table, n_words and the kernel's G are sized by that
        if (G >= (1ull << 31)) return fail(ctx, SRX_E_ARG, "srx_select_op: G %llu exceeds int32 device indices", (unsigned long long)G);
        SRX_TRY(list_rank_table(ctx, a->genes, a->take, G, table));
    } else {
        if (!a->cnt || !a->var) return fail(ctx, SRX_E_ARG, "srx_select_op: null array");
        if (a->route < kRouteAuto || a->route > kRouteMiss) return fail(ctx, SRX_E_ARG, "srx_select_op: route must be 0, 1 or 2");
        if (!hvg_on_device(a->take, G))
            return fail(ctx, SRX_E_ARG, "srx_select_op: outside the device ranking's envelope (G <= 65536, min(take, G) <= %llu)",
                        (unsigned long long)kDevSelMaxK);
    }
    SRX_HIP(ctx, hipSetDevice(ctx->device));

    const uint64_t k = std::min<uint64_t>(a->take, G);
    const int n_words = (int)((G + 31) / 32);
    SelBufs bufs;
    uint64_t* d_cnt = nullptr;
    double *d_sum = nullptr, *d_sq = nullptr;
    SelWork w;
    SelDev out;
    out.k = (int)k;
    out.n_words = n_words;
    uint32_t unused = (uint32_t)SRX_SEL_COUNTER_UNUSED;
    if (a->cnt) SRX_TRY(sel_up(ctx, bufs, a->cnt, G, 8, (void**)&d_cnt));
    if (a->sum && vectors) SRX_TRY(sel_up(ctx, bufs, a->sum, G, 8, (void**)&d_sum));
    if (a->sq && vectors) SRX_TRY(sel_up(ctx, bufs, a->sq, G, 8, (void**)&d_sq));
    SRX_TRY(sel_up(ctx, bufs, a->var, G, 8, (void**)&w.d_var));
    SRX_TRY(sel_up(ctx, bufs, list ? table.data() : a->rank, G, 4, (void**)&w.d_rank));
    SRX_TRY(sel_up(ctx, bufs, nullptr, G, 4, (void**)&w.d_cand));
    SRX_TRY(sel_up(ctx, bufs, &unused, 1, 4, (void**)&w.d_counter));
    SRX_TRY(sel_up(ctx, bufs, a->sel_rank, k, 4, (void**)&out.d_sel_rank));
    SRX_TRY(sel_up(ctx, bufs, a->bits, n_words, 4, (void**)&out.d_bits));
    SRX_TRY(sel_up(ctx, bufs, a->prefix, n_words, 4, (void**)&w.d_prefix));
    SRX_TRY(sel_up(ctx, bufs, a->mu, k, 8, (void**)&out.d_mu));
    SRX_TRY(sel_up(ctx, bufs, a->sd, k, 8, (void**)&out.d_sd));
    SRX_TRY(sel_up(ctx, bufs, a->dinv, k, 8, (void**)&out.d_dinv));
    SRX_TRY(sel_up(ctx, bufs, &a->trace, 1, 8, (void**)&out.d_trace));
    SRX_TRY(sel_up(ctx, bufs, &a->status, 1, 4, (void**)&out.d_status));

    if (list)
        SRX_TRY(launch_sel_finish(ctx, w.d_rank, nullptr, d_sum, d_sq, G, (double)a->n_cells, a->center, a->scale, out, w.d_prefix));
    else
        SRX_TRY(hvg_launches(ctx, d_cnt, d_sum, d_sq, G, k, (double)a->n_cells, a->center, a->scale, a->route, w, out));
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));

    int32_t touched = 0;
    if (d_cnt) SRX_TRY(sel_down(ctx, nullptr, d_cnt, G, 8, 0, &touched));
    if (d_sum) SRX_TRY(sel_down(ctx, nullptr, d_sum, G, 8, 1, &touched));
    if (d_sq) SRX_TRY(sel_down(ctx, nullptr, d_sq, G, 8, 2, &touched));
    SRX_TRY(sel_down(ctx, list ? nullptr : a->var, w.d_var, G, 8, 3, &touched));
    SRX_TRY(sel_down(ctx, a->rank, w.d_rank, G, 4, 4, &touched));
    SRX_TRY(sel_down(ctx, nullptr, w.d_cand, G, 4, 5, &touched));
    SRX_TRY(sel_down(ctx, &a->counter, w.d_counter, 1, 4, 6, &touched));
    SRX_TRY(sel_down(ctx, a->sel_rank, out.d_sel_rank, k, 4, 7, &touched));
    SRX_TRY(sel_down(ctx, a->bits, out.d_bits, n_words, 4, 8, &touched));
    SRX_TRY(sel_down(ctx, a->prefix, w.d_prefix, n_words, 4, 9, &touched));
    SRX_TRY(sel_down(ctx, a->mu, out.d_mu, k, 8, 10, &touched));
    SRX_TRY(sel_down(ctx, a->sd, out.d_sd, k, 8, 11, &touched));
    SRX_TRY(sel_down(ctx, a->dinv, out.d_dinv, k, 8, 12, &touched));
    SRX_TRY(sel_down(ctx, &a->trace, out.d_trace, 1, 8, 13, &touched));
    SRX_TRY(sel_down(ctx, &a->status, out.d_status, 1, 4, 14, &touched));
    a->tail_touched = touched;
    return SRX_OK;
}

}  // extern "C"
