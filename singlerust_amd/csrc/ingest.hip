// ingest.hip — new cells on a fitted data set: srx_umap_transform_knn / srx_umap_transform_graph (the cells placed in the
// fitted UMAP, nothing refitted) and srx_knn_vote / srx_knn_vote_graph (their labels from their neighbours' labels).  The
// projection of the cells and the search for their neighbours are pca.hip's and knn.hip's.
//
// Definition (include/srx.h has it in full): umap-learn's UMAP.transform restated.  Per query row the membership weights of
// its kq reference neighbours (the graph section's scale with rho = 0 and the nearest entry left out of the row sum), the
// start at their weighted mean, then srx_umap's epochs with the reference positions held fixed: only the query moves, it
// reads fixed positions, so query rows do not interact.  Hence no double buffer and no launch per epoch: the lanes that own
// a query keep its position in registers through all the epochs of a launch.  A launch holds at most
// SRX_UMAP_TRANSFORM_CHUNK epochs, so that none runs long whatever n_epochs is; the launches follow each other on the
// context's stream and hand on the positions alone, which makes the result the same bits for every chunk length.
//
// Kernels:
//   k_ingest_rows<DIM>    one wave per query row, lane p holds entry p (kq <= 64): checks the list into a flag word (index
//                         range, duplicates, distances), puts the row in column order (rank by counting across the lanes,
//                         through LDS), finds the nearest entry, solves sigma (graph_root.hpp: the statement k_graph_rows
//                         solves its rows with), writes the weights, sigma and the start (fixed-order butterflies)
//   (k_umap_wmax, k_umap_active of umap.hip: w_max and entries_active over the n_query x kq weights)
//   k_ingest_epochs<DIM>  SRX_UMAP_GROUP lanes per query; a lane holds (j, r_e) of its up to 8 entries and the position in
//                         registers and runs the epochs [t0, t1) in a loop: which of its entries the schedule samples (a
//                         bit mask), per sampled entry the attraction and the R hashed targets (um_term of
//                         umap_internal.hpp, the body k_umap_epoch uses), group_sum, every lane of the group applies the
//                         same delta.  No LDS, barrier or atomic in the loop; the position is stored once, the sample
//                         counter is a per-block integer sum added with an integer atomic.
//   k_ingest_vote         one wave per row: a lane counts the occurrences of its entry's label along the row by shuffles,
//                         the wave takes the maximum of (count, -label)
// x^y is ocml's pow(double, double); no -ffast-math, FMA contraction off (umap_internal.hpp).
#include "common.hpp"
#include "graph_handle.hpp"
#include "graph_root.hpp"
#include "hash.hpp"
#include "scan.hpp"

#include <cmath>

#include "umap_internal.hpp"         // FMA contraction is off from here on

namespace srx {

constexpr int kIngestMaxK = 64;
constexpr int kIngestPerLane = kIngestMaxK / kUmGroup;      // entries of a row that one lane of its group holds, at the most
enum { kBadLabel = 16 };                                    // beside kBadRange .. kBadDist of graph_handle.hpp
// the small block (8-byte words): the UM_ words of umap_internal.hpp | the row counters in kCtrSlots slots | the flag
enum { IG_NOROOT = 0, IG_CLAMPED, IG_ALLZERO, IG_NEAREST, IG_N };
constexpr size_t kIgCtr = UM_WORDS, kIgFlag = kIgCtr + (size_t)kCtrSlots * IG_N, kIgWords = kIgFlag + 1;

template <int DIM>
__global__ void __launch_bounds__(256) k_ingest_rows(const uint32_t* __restrict__ idx_in, const double* __restrict__ dist_in,
                                                     uint64_t nq, int kq, uint64_t n_ref, const double* __restrict__ yref,
                                                     uint32_t* __restrict__ cols, double* __restrict__ w_out,
                                                     double* __restrict__ sigma_out, double* __restrict__ y0,
                                                     unsigned long long* __restrict__ ctr, int* __restrict__ flag) {
    __shared__ uint32_t s_i[4][kWave];
    __shared__ double s_d[4][kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = global_wave_id();
    if (row >= nq) return;
    const bool act = lane < kq;
    const size_t e = (size_t)row * kq + lane;
    uint32_t ci = act ? idx_in[e] : 0xFFFFFFFFu;
    double cd = act ? dist_in[e] : 0.0;
    int bad = 0;
    if (act) {
        if (ci >= n_ref) bad |= kBadRange;
        if (!(cd >= 0.0 && cd <= kDblMax)) bad |= kBadDist;
    }
    int rank = 0;
    for (int m = 0; m < kq; ++m) {
        const uint32_t o = __shfl(ci, m, kWave);
        rank += o < ci;
        if (act && m != lane && o == ci) bad |= kBadDup;
    }
    if (bad) atomicOr(flag, bad);        // the host refuses the list; what follows stays inside the row, its loops are bounded
    // the row in column order: lane s holds slot s
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

    // the nearest entry by (distance, index) stays out of the row sum
    const double inf = (double)__builtin_inff();
    const double dmin = wave_min(act ? cd : inf);
    const uint32_t imin = wave_min(act && cd == dmin ? ci : 0xFFFFFFFFu);
    const bool nearest = act && cd == dmin && ci == imin;
    const bool all_zero = !(wave_max(act ? cd : 0.0) > 0.0);
    const bool in_sum = act && !nearest;
    const bool far = in_sum && cd > 0.0, one = in_sum && !far;
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(one));
    const double T = log2((double)kq);
    const double sum_d = wave_sum(act ? cd : 0.0);
    const double x = far ? cd : 0.0;
    const bool has_root = !all_zero && (double)c < T;
    double sig = 0.0;
    // S rises from c < T (s -> 0) to kq - 1 > T (s -> inf; kq >= 3)
    if (has_root) sig = graph_root(one, far, x, T);
    const double floor_ = 1e-3 * sum_d / (double)kq;
    const bool clamped = !all_zero && floor_ > sig;
    const double sigma = all_zero ? 0.0 : (clamped ? floor_ : sig);
    const double w = act ? (cd > 0.0 ? exp(-cd / sigma) : 1.0) : 0.0;

    // the start: the weighted mean of the neighbours' positions (a refused index is not followed)
    const double W = wave_sum(w);
    double yr[DIM], ys[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) yr[d] = 0.0;
    if (act && ci < n_ref) um_load<DIM>(yref, ci, yr);
    const bool from_nearest = W == 0.0;
    const double f = w / W;
#pragma unroll
    for (int d = 0; d < DIM; ++d) ys[d] = wave_sum(from_nearest ? (nearest ? yr[d] : 0.0) : (act ? f * yr[d] : 0.0));

    if (act) {
        cols[e] = ci;
        w_out[e] = w;
    }
    if (lane == 0) {
        sigma_out[row] = sigma;
#pragma unroll
        for (int d = 0; d < DIM; ++d) y0[row * DIM + d] = ys[d];
        unsigned long long* my = ctr + (size_t)(row & (kCtrSlots - 1)) * IG_N;
        if (!has_root) atomicAdd(&my[IG_NOROOT], 1ull);
        if (clamped) atomicAdd(&my[IG_CLAMPED], 1ull);
        if (all_zero) atomicAdd(&my[IG_ALLZERO], 1ull);
        if (from_nearest) atomicAdd(&my[IG_NEAREST], 1ull);
    }
}

// Epochs t0 .. t1 - 1 of the `epochs`-epoch schedule on the positions at yq (read once, written once).  cols / w: the rows in
// slot order (every column < n_ref: the list has passed its check); small: the run's block (w_max read, the samples added).
template <int DIM>
__global__ void __launch_bounds__(256) k_ingest_epochs(const uint32_t* __restrict__ cols, const double* __restrict__ w, uint64_t nq,
                                                       int kq, const double* __restrict__ yref, uint64_t n_ref, double* __restrict__ yq,
                                                       uint32_t t0, uint32_t t1, double alpha0, double epochs, UmParams p,
                                                       unsigned long long* __restrict__ small) {
    constexpr int G = kUmGroup, PER = kIngestPerLane;
    __shared__ unsigned long long s_wave[4];
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = row < nq;
    const uint64_t nnz = nq * (uint64_t)kq, base = row * (uint64_t)kq + sub;
    double yi[DIM];
    uint32_t j[PER];
    double r[PER];                       // r_e; 0 for a slot the row does not have: floor(t * 0) never rises, it is never sampled
#pragma unroll
    for (int c = 0; c < DIM; ++c) yi[c] = 0.0;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        j[q] = 0;
        r[q] = 0.0;
    }
    if (live) {
        um_load<DIM>(yq, row, yi);
        const double wmax = __longlong_as_double((long long)small[UM_WMAX]);
#pragma unroll
        for (int q = 0; q < PER; ++q)
            if (sub + q * G < kq) {
                j[q] = cols[base + q * G];
                r[q] = w[base + q * G] / wmax;
            }
    }
    const double att = -2.0 * p.a * p.b, rep = 2.0 * p.gamma * p.b;
    unsigned long long n_samp = 0;
    // every lane of the block runs every epoch (a lane without a row samples nothing): the butterflies read all of them
    for (uint32_t t = t0; t < t1; ++t) {
        const double tf = (double)t, tp = (double)(t - 1);
        const double alpha = alpha0 * (1.0 - tp / epochs);
        unsigned mask = 0;
#pragma unroll
        for (int q = 0; q < PER; ++q) mask |= floor(tf * r[q]) > floor(tp * r[q]) ? 1u << q : 0u;
        n_samp += (unsigned)__builtin_popcount(mask);
        double acc[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
        // this lane's sampled entries in ascending order; the lanes of a wave walk theirs independently
        while (mask) {
            const int q = __builtin_ctz(mask);
            mask &= mask - 1;
            uint32_t jq = j[0];
#pragma unroll
            for (int u = 1; u < PER; ++u) jq = q == u ? j[u] : jq;
            // s = -1: the attraction along the entry; s = 0 .. rate - 1: its negative samples
            const uint64_t first = ((uint64_t)t * nnz + (base + (uint64_t)(q * G))) * (uint64_t)p.rate + 1;
            for (int s = -1; s < p.rate; ++s) {
                uint64_t o = jq;
                if (s >= 0) {
                    const uint64_t z = mix64(p.seed + kGold64 * (first + (uint64_t)s));
                    o = ((z >> 32) * n_ref) >> 32;                  // < n_ref < 2^32
                }
                um_term<DIM>(yi, yref, o, p, s < 0, s < 0 ? att : rep, alpha, acc);
            }
        }
#pragma unroll
        for (int c = 0; c < DIM; ++c) yi[c] = yi[c] + group_sum<G>(acc[c]);
    }
    if (live && sub == 0) {
        if constexpr (DIM == 2) {
            reinterpret_cast<double2*>(yq)[row] = make_double2(yi[0], yi[1]);
        } else {
#pragma unroll
            for (int c = 0; c < DIM; ++c) yq[row * DIM + c] = yi[c];
        }
    }
    n_samp = block_sum_thread0<4>(n_samp, s_wave);
    if (n_samp) atomicAdd(&small[UM_SAMPLES], n_samp);
}

// labels: n_ref u32 on the device; n_groups: what a label must stay below
__global__ void __launch_bounds__(256) k_ingest_vote(const uint32_t* __restrict__ idx_in, uint64_t nq, int k, uint64_t n_ref,
                                                     const uint32_t* __restrict__ labels, uint32_t n_groups,
                                                     uint32_t* __restrict__ label_out, uint32_t* __restrict__ count_out,
                                                     int* __restrict__ flag) {
    const int lane = lane_id();
    const uint64_t row = global_wave_id();
    if (row >= nq) return;
    const bool act = lane < k;
    const uint32_t ci = act ? idx_in[(size_t)row * k + lane] : 0xFFFFFFFFu;
    const bool ok = act && ci < n_ref;
    const uint32_t lab = ok ? labels[ci] : 0xFFFFFFFFu;
    int bad = 0;
    if (act && !ok) bad |= kBadRange;
    if (ok && lab >= n_groups) bad |= kBadLabel;
    uint32_t cnt = 0;
    for (int m = 0; m < k; ++m) {
        const uint32_t oi = __shfl(ci, m, kWave), ol = __shfl(lab, m, kWave);
        cnt += ol == lab;
        if (act && m != lane && oi == ci) bad |= kBadDup;
    }
    if (bad) atomicOr(flag, bad);
    // the most frequent label, ties to the lowest: the largest (count, ~label)
    const unsigned long long best = wave_max(act ? ((unsigned long long)cnt << 32) | (0xFFFFFFFFu - lab) : 0ull);
    if (lane == 0) {
        label_out[row] = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
        count_out[row] = (uint32_t)(best >> 32);
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int32_t ingest_flag_check(srx_ctx* ctx, const char* who, uint64_t n_ref, const int* d_flag) {
    int flag = 0;
    SRX_TRY(d2h(ctx, &flag, d_flag, 4));
    if (flag & kBadRange) return fail(ctx, SRX_E_ARG, "%s: a neighbour index is not below n_ref = %llu", who, (unsigned long long)n_ref);
    if (flag & kBadDup) return fail(ctx, SRX_E_ARG, "%s: a row names one reference twice", who);
    if (flag & kBadDist) return fail(ctx, SRX_E_ARG, "%s: a distance is negative, NaN or Inf", who);
    if (flag & kBadLabel) return fail(ctx, SRX_E_ARG, "%s: a reference label is not below n_groups", who);
    return SRX_OK;
}

struct IgOpts {
    srx_umap_transform_opts o;
    uint32_t epochs, run, chunk;
};

static int32_t ig_opts(srx_ctx* ctx, const srx_umap_transform_opts* in, uint64_t nq, IgOpts* out) {
    srx_umap_transform_opts o = in ? *in : srx_umap_transform_opts{0.0, 0.0, 0.5, 1.0, 1.0, 0.25, 0, 0, 0, 5, 0};
    if (o.negative_sample_rate < 0 || o.negative_sample_rate > 32)
        return fail(ctx, SRX_E_ARG, "umap_transform: negative_sample_rate = %d outside 0..32", o.negative_sample_rate);
    if (o.a == 0.0 && o.b == 0.0) SRX_TRY(umap_fit_curve(ctx, o.spread, o.min_dist, &o.a, &o.b));
    if (!is_pos_finite(o.a) || !is_pos_finite(o.b))
        return fail(ctx, SRX_E_ARG, "umap_transform: a and b must be positive finite numbers (or both 0: fitted)");
    if (!is_pos_finite(o.gamma)) return fail(ctx, SRX_E_ARG, "umap_transform: gamma must be a positive finite number");
    if (!is_pos_finite(o.alpha0)) return fail(ctx, SRX_E_ARG, "umap_transform: alpha0 must be a positive finite number");
    if (o.n_epochs < 0 || o.n_epochs > SRX_UMAP_MAX_EPOCHS)
        return fail(ctx, SRX_E_ARG, "umap_transform: n_epochs = %d outside 0..%d", o.n_epochs, SRX_UMAP_MAX_EPOCHS);
    if (o.n_epochs == 0) o.n_epochs = nq <= 10000 ? 100 : 30;
    if (o.stop_after < 0 || o.stop_after > o.n_epochs)
        return fail(ctx, SRX_E_ARG, "umap_transform: stop_after = %d outside 0..n_epochs = %d", o.stop_after, o.n_epochs);
    if (o.chunk_epochs < 0 || o.chunk_epochs > SRX_UMAP_TRANSFORM_CHUNK)
        return fail(ctx, SRX_E_ARG, "umap_transform: chunk_epochs = %d outside 0..%d", o.chunk_epochs, SRX_UMAP_TRANSFORM_CHUNK);
    out->o = o;
    out->epochs = (uint32_t)o.n_epochs;
    out->run = (uint32_t)(o.stop_after ? o.stop_after : o.n_epochs);
    out->chunk = (uint32_t)(o.chunk_epochs ? o.chunk_epochs : SRX_UMAP_TRANSFORM_CHUNK);
    return SRX_OK;
}

// what both lists must satisfy before anything is queued; lo: the smallest row length of the caller
static int32_t ig_check_list(srx_ctx* ctx, const char* who, const uint32_t* indices, uint64_t nq, uint32_t k, uint32_t lo, uint64_t n_ref) {
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: rows are sharded; the fitted data set lives on one rank", who);
    if (k < lo || k > (uint32_t)kIngestMaxK) return fail(ctx, SRX_E_ARG, "%s: k = %u outside %u..%d", who, k, lo, kIngestMaxK);
    if ((uint64_t)k > n_ref) return fail(ctx, SRX_E_ARG, "%s: k = %u but there are only %llu reference points", who, k, (unsigned long long)n_ref);
    if (n_ref >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "%s: 2^32 - 1 reference points or more", who);
    if (nq && !indices) return fail(ctx, SRX_E_ARG, "%s: null k-NN list", who);
    return SRX_OK;
}

// d_yref: n_ref x dim f64 on the device, finite.  Everything else from host pointers.
static int32_t transform_run(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t nq, uint32_t kq, const double* d_yref,
                             uint64_t n_ref, uint32_t dim, const IgOpts& u, srx_umap_transform_out* out, srx_umap_transform_info* info) {
    srx_umap_transform_info li{};
    li.n_query = nq;
    li.n_ref = n_ref;
    li.kq = kq;
    li.dim = dim;
    li.n_epochs = u.epochs;
    li.a = u.o.a;
    li.b = u.o.b;
    if (nq == 0) {
        if (info) *info = li;
        return SRX_OK;
    }
    Range rg("umap_transform");
    hipStream_t st = ctx->stream;
    const size_t nk = (size_t)nq * kq;
    uint32_t *d_idx, *d_cols;
    double *d_dist, *d_w, *d_sigma, *d_y;
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "ingest_idx", nk * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "ingest_dist", nk * 8, (void**)&d_dist));
    SRX_TRY(scratch(ctx, "ingest_cols", nk * 4, (void**)&d_cols));
    SRX_TRY(scratch(ctx, "ingest_w", nk * 8, (void**)&d_w));
    SRX_TRY(scratch(ctx, "ingest_sigma", nq * 8, (void**)&d_sigma));
    SRX_TRY(scratch(ctx, "ingest_y", nq * dim * 8, (void**)&d_y));
    SRX_TRY(scratch(ctx, "ingest_small", kIgWords * 8, (void**)&d_small));
    SRX_TRY(h2d(ctx, d_idx, indices, nk * 4));
    SRX_TRY(h2d(ctx, d_dist, distances, nk * 8));
    int* d_flag = reinterpret_cast<int*>(d_small + kIgFlag);

    {
        StreamTimer timer(ctx, st);
        SRX_TRY(timer.start());
        SRX_HIP(ctx, hipMemsetAsync(d_small, 0, kIgWords * 8, st));
        const unsigned wg_rows = (unsigned)((nq + 3) / 4);
        if (dim == 2)
            hipLaunchKernelGGL(k_ingest_rows<2>, dim3(wg_rows), dim3(256), 0, st, d_idx, d_dist, nq, (int)kq, n_ref, d_yref, d_cols, d_w, d_sigma,
                               d_y, d_small + kIgCtr, d_flag);
        else
            hipLaunchKernelGGL(k_ingest_rows<3>, dim3(wg_rows), dim3(256), 0, st, d_idx, d_dist, nq, (int)kq, n_ref, d_yref, d_cols, d_w, d_sigma,
                               d_y, d_small + kIgCtr, d_flag);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(timer.stop(&li.membership_ms));
    }
    SRX_TRY(ingest_flag_check(ctx, "umap_transform", n_ref, d_flag));
    // the list is sound: from here on results may be written
    if (out) {
        if (out->start) SRX_TRY(d2h(ctx, out->start, d_y, nq * dim * 8));
        if (out->weights) SRX_TRY(d2h(ctx, out->weights, d_w, nk * 8));
        if (out->columns) SRX_TRY(d2h(ctx, out->columns, d_cols, nk * 4));
        if (out->sigma) SRX_TRY(d2h(ctx, out->sigma, d_sigma, nq * 8));
    }
    double ms = 0.0;
    {
        StreamTimer timer(ctx, st);
        SRX_TRY(timer.start());
        umap_wmax_active(ctx, d_w, nk, (double)u.epochs, d_small);
        const UmParams p{u.o.a, u.o.b, u.o.gamma, u.o.seed, u.o.negative_sample_rate};
        const unsigned blocks = grid256(nq * (uint64_t)kUmGroup);
        for (uint32_t t0 = 1; t0 <= u.run; t0 += u.chunk) {
            const uint32_t t1 = t0 + u.chunk <= u.run ? t0 + u.chunk : u.run + 1;
            if (dim == 2)
                hipLaunchKernelGGL(k_ingest_epochs<2>, dim3(blocks), dim3(256), 0, st, d_cols, d_w, nq, (int)kq, d_yref, n_ref, d_y, t0, t1,
                                   u.o.alpha0, (double)u.epochs, p, d_small);
            else
                hipLaunchKernelGGL(k_ingest_epochs<3>, dim3(blocks), dim3(256), 0, st, d_cols, d_w, nq, (int)kq, d_yref, n_ref, d_y, t0, t1,
                                   u.o.alpha0, (double)u.epochs, p, d_small);
        }
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(timer.stop(&ms));
    }
    uint64_t h[kIgWords];
    SRX_TRY(d2h(ctx, h, d_small, sizeof h));
    uint64_t sum[IG_N] = {0, 0, 0, 0};
    for (int s = 0; s < kCtrSlots; ++s)
        for (int c = 0; c < IG_N; ++c) sum[c] += h[kIgCtr + (size_t)s * IG_N + c];
    li.rows_no_root = sum[IG_NOROOT];
    li.rows_clamped = sum[IG_CLAMPED];
    li.rows_all_zero = sum[IG_ALLZERO];
    li.rows_start_nearest = sum[IG_NEAREST];
    li.entries_active = h[UM_ACTIVE];
    li.samples = h[UM_SAMPLES];
    li.negatives = h[UM_SAMPLES] * (uint64_t)u.o.negative_sample_rate;
    li.epochs_run = u.run;
    memcpy(&li.w_max, &h[UM_WMAX], 8);
    li.ms = li.membership_ms + ms;
    if (out && out->embedding) SRX_TRY(d2h(ctx, out->embedding, d_y, nq * dim * 8));
    if (info) *info = li;
    return SRX_OK;
}

// d_labels: n_ref u32 on the device
static int32_t vote_run(srx_ctx* ctx, const char* who, const uint32_t* indices, uint64_t nq, uint32_t k, const uint32_t* d_labels, uint64_t n_ref,
                        uint32_t n_groups, uint32_t* labels_out, uint32_t* counts_out) {
    if (nq == 0) return SRX_OK;
    Range rg("knn_vote");
    hipStream_t st = ctx->stream;
    uint32_t *d_idx, *d_out;
    int* d_flag;
    SRX_TRY(scratch(ctx, "ingest_idx", nq * k * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "ingest_vote", 2 * nq * 4, (void**)&d_out));
    SRX_TRY(scratch(ctx, "ingest_small", kIgWords * 8, (void**)&d_flag));
    SRX_TRY(h2d(ctx, d_idx, indices, nq * k * 4));
    SRX_HIP(ctx, hipMemsetAsync(d_flag, 0, 4, st));
    hipLaunchKernelGGL(k_ingest_vote, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, d_idx, nq, (int)k, n_ref, d_labels, n_groups, d_out,
                       d_out + nq, d_flag);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(ingest_flag_check(ctx, who, n_ref, d_flag));
    if (labels_out) SRX_TRY(d2h(ctx, labels_out, d_out, nq * 4));
    if (counts_out) SRX_TRY(d2h(ctx, counts_out, d_out + nq, nq * 4));
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_umap_transform_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n_query, uint32_t kq,
                               const double* ref_embedding, uint64_t n_ref, uint32_t dim, const srx_umap_transform_opts* opts,
                               srx_umap_transform_out* out, srx_umap_transform_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    SRX_TRY(ig_check_list(ctx, "umap_transform", indices, n_query, kq, 3, n_ref));
    if (dim != 2 && dim != 3) return fail(ctx, SRX_E_ARG, "umap_transform: dim = %u is not 2 or 3", dim);
    if (n_query && !distances) return fail(ctx, SRX_E_ARG, "umap_transform: null distances");
    if (!ref_embedding) return fail(ctx, SRX_E_ARG, "umap_transform: null reference positions");
    IgOpts u;
    SRX_TRY(ig_opts(ctx, opts, n_query, &u));
    for (uint64_t c = 0; c < n_ref * dim; ++c)
        if (!is_finite(ref_embedding[c])) return fail(ctx, SRX_E_ARG, "umap_transform: the reference positions hold a NaN or Inf");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    double* d_yref = nullptr;
    if (n_query) {
        SRX_TRY(scratch(ctx, "ingest_yref", n_ref * dim * 8, (void**)&d_yref));
        SRX_TRY(h2d(ctx, d_yref, ref_embedding, n_ref * dim * 8));
    }
    return transform_run(ctx, indices, distances, n_query, kq, d_yref, n_ref, dim, u, out, info);
}

int32_t srx_umap_transform_graph(srx_graph* g, const uint32_t* indices, const double* distances, uint64_t n_query, uint32_t kq,
                                 uint32_t dim, const srx_umap_transform_opts* opts, srx_umap_transform_out* out,
                                 srx_umap_transform_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->embed_valid) return fail(ctx, SRX_E_ARG, "umap_transform: no srx_umap has run on this graph: there is no embedding to map onto");
    if (dim != 2 && dim != 3) return fail(ctx, SRX_E_ARG, "umap_transform: dim = %u is not 2 or 3", dim);
    if (dim != g->embed_dim) return fail(ctx, SRX_E_ARG, "umap_transform: dim = %u, but the resident embedding has %u components", dim, g->embed_dim);
    SRX_TRY(ig_check_list(ctx, "umap_transform", indices, n_query, kq, 3, g->n));
    if (n_query && !distances) return fail(ctx, SRX_E_ARG, "umap_transform: null distances");
    IgOpts u;
    SRX_TRY(ig_opts(ctx, opts, n_query, &u));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    // the embedding is srx_umap's own result: finite (its start is checked, every term of a step is clipped)
    return transform_run(ctx, indices, distances, n_query, kq, g->d_embed, g->n, g->embed_dim, u, out, info);
}

int32_t srx_knn_vote(srx_ctx* ctx, const uint32_t* indices, uint64_t n_query, uint32_t k, const uint32_t* ref_labels, uint64_t n_ref,
                     uint32_t n_groups, uint32_t* labels_out, uint32_t* counts_out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    SRX_TRY(ig_check_list(ctx, "knn_vote", indices, n_query, k, 1, n_ref));
    if (!ref_labels) return fail(ctx, SRX_E_ARG, "knn_vote: null reference labels");
    for (uint64_t i = 0; i < n_ref; ++i)
        if (ref_labels[i] >= n_groups)
            return fail(ctx, SRX_E_ARG, "knn_vote: the label %u of reference %llu is not below n_groups = %u", ref_labels[i], (unsigned long long)i,
                        n_groups);
    if (n_query == 0) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* d_labels;
    SRX_TRY(scratch(ctx, "ingest_labels", n_ref * 4, (void**)&d_labels));
    SRX_TRY(h2d(ctx, d_labels, ref_labels, n_ref * 4));
    return vote_run(ctx, "knn_vote", indices, n_query, k, d_labels, n_ref, n_groups, labels_out, counts_out);
}

int32_t srx_knn_vote_graph(srx_graph* g, const uint32_t* indices, uint64_t n_query, uint32_t k, uint32_t* labels_out, uint32_t* counts_out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->labels_valid) return fail(ctx, SRX_E_ARG, "knn_vote: no srx_louvain has run on this graph: there are no labels to vote with");
    SRX_TRY(ig_check_list(ctx, "knn_vote", indices, n_query, k, 1, g->n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    // the labels are srx_louvain's own: every one is below n
    return vote_run(ctx, "knn_vote", indices, n_query, k, g->d_labels, g->n, 0xFFFFFFFFu, labels_out, counts_out);
}

}  // extern "C"
