// doublets.hip — doublet detection (Scrublet, restated in include/srx.h): synthetic doublets as sums of CSR row pairs, their
// projection onto the fitted PCA beside the observed scores, the exact k-NN search over both, the likelihood scores of every
// neighbour list and the host threshold.  The srx_doublets handle owns the point block, the list, the parents and the scores;
// the synthetic matrix lives only between the simulation and the projection.
//
//   k_doublet_parents   p(s, c) of the hashed parents, one thread per parent
//   k_doublet_count     matches between the two parents of a synthetic row by binary search of the shorter parent's columns in
//                       the longer: the union holds len_a + len_b - matches entries
//   k_doublet_fill<VT>  the sorted union-add.  a_i with lower bound lb in B and match flag m_i = (B[lb] == a_i) goes to
//                       i + lb - (matches before i); an unmatched b_j with lower bound la in A goes to j + la - (matches among
//                       B[0 .. j)), which is the number of matches among A[0 .. la) because matched pairs keep their order.  The
//                       running match counts are prefix sums along each side (scan.hpp).  No atomics: every output position is
//                       computed on its own, so the matrix is the same bits from call to call.
//   k_doublet_scores    one thread per row of the list: k_d and the formulas of section 4 in f64
//   k_doublet_call      predicted and z of the observed rows for a threshold, and the two counts the rates are made of (integer
//                       atomics, one per workgroup)
//
// Both passes give a workgroup of four waves four consecutive synthetic rows.  A row whose parents hold at most
// SRX_DOUBLET_WAVE_ROW entries together is walked by one wave, 64 entries per round, so four rows are in flight per workgroup and
// no barrier is paid; after that the whole workgroup strides over each longer row of its four, 256 entries per round with the
// block scan's two barriers.  Where the switch-over lies: a wave's round costs one dependent binary search (about log2 of the other
// parent's length cached loads); rows of equal length finish together in wave mode, so the workgroup form only pays for a row that
// would keep one wave walking while its three neighbours idle.  8192 entries are 128 rounds of one wave against 32 of the
// workgroup: a single-cell row of typical depth (a few thousand genes at most, c3: 1 650) stays in wave mode, the rare very deep
// cell does not hold its workgroup for hundreds of rounds.  The constant was chosen by this reasoning, not by a sweep.
#include "scan.hpp"
#include "hash.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

struct srx_doublets {
    srx_ctx* ctx = nullptr;
    uint64_t n = 0, n_sim = 0;
    uint32_t k_adj = 0, d = 0;
    size_t ld = 0;                       // doubles per row of the point block: scores_ld() of the fit's components
    double r = 0.0;
    void* d_block = nullptr;             // one allocation: points | Ld | se | z | parents | list | predicted | counts
    double *d_pts = nullptr, *d_ld = nullptr, *d_se = nullptr, *d_z = nullptr;
    uint64_t* d_parents = nullptr;
    uint32_t* d_knn = nullptr;
    uint8_t* d_pred = nullptr;
    unsigned long long* d_counts = nullptr;
    std::vector<double> sim_scores;      // host copy of Ld[n ..): what the threshold reads
    double auto_threshold = 0.0;
    int32_t auto_found = 0;
    uint32_t auto_rounds = 0;
    srx_doublet_info info{};
};

namespace srx {

int32_t knn_self_device(srx_ctx* ctx, const double* d_pts, uint64_t n, uint64_t d_full, size_t ld, const srx_knn_opts* opts,
                        uint32_t* indices_out, double* distances_out, srx_knn_info* info, const uint32_t** d_idx,
                        const double** d_dist, uint64_t* n_out);                                                   // knn.hip

constexpr int kDbWaves = 4;                       // waves, and synthetic rows, per workgroup
constexpr int kDbBlock = kDbWaves * kWave;
constexpr int kDbWaveRow = SRX_DOUBLET_WAVE_ROW;

__global__ __launch_bounds__(256) void k_doublet_parents(uint64_t seed, uint64_t n, uint64_t count, uint64_t* __restrict__ parents) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;           // t = 2 s + c
    if (t >= count) return;
    parents[t] = ((mix64(seed + kGold64 * (1ull + t)) >> 32) * n) >> 32;
}

// first position of a[0 .. n) that is not below key
__device__ __forceinline__ int doublet_lower_bound(const int32_t* __restrict__ a, int n, int32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the two parent rows of synthetic row s
struct DoubletRow {
    int64_t a0, b0;
    int la, lb;
};
__device__ __forceinline__ DoubletRow doublet_row(const int64_t* __restrict__ indptr, const uint64_t* __restrict__ parents, uint64_t s) {
    const uint64_t pa = parents[2 * s], pb = parents[2 * s + 1];
    DoubletRow r;
    r.a0 = indptr[pa];
    r.la = (int)(indptr[pa + 1] - r.a0);
    r.b0 = indptr[pb];
    r.lb = (int)(indptr[pb + 1] - r.b0);
    return r;
}

// matches of S[first, first + step, ..) in Lg
__device__ __forceinline__ int doublet_matches(const int32_t* __restrict__ S, int ls, const int32_t* __restrict__ Lg, int ll, int first,
                                               int step) {
    int m = 0;
    for (int i = first; i < ls; i += step) {
        const int32_t c = S[i];
        const int p = doublet_lower_bound(Lg, ll, c);
        m += (p < ll && Lg[p] == c) ? 1 : 0;
    }
    return m;
}

__global__ __launch_bounds__(kDbBlock) void k_doublet_count(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                            const uint64_t* __restrict__ parents, uint64_t n_sim,
                                                            int64_t* __restrict__ cnt) {
    __shared__ int s_w[kDbWaves];
    const int wave = threadIdx.x / kWave, lane = lane_id();
    const uint64_t s0 = (uint64_t)blockIdx.x * kDbWaves;
    {   // a wave per short row
        const uint64_t s = s0 + wave;
        if (s < n_sim) {
            const DoubletRow r = doublet_row(indptr, parents, s);
            if (r.la + r.lb <= kDbWaveRow) {
                const bool a_short = r.la <= r.lb;
                const int32_t* S = idx + (a_short ? r.a0 : r.b0);
                const int32_t* Lg = idx + (a_short ? r.b0 : r.a0);
                const int m = wave_sum(doublet_matches(S, a_short ? r.la : r.lb, Lg, a_short ? r.lb : r.la, lane, kWave));
                if (lane == 0) cnt[s] = (int64_t)(r.la + r.lb - m);
            }
        }
    }
    for (int w = 0; w < kDbWaves; ++w) {   // the workgroup over each long row (the test is the same in every thread)
        const uint64_t s = s0 + w;
        if (s >= n_sim) break;
        const DoubletRow r = doublet_row(indptr, parents, s);
        if (r.la + r.lb <= kDbWaveRow) continue;
        const bool a_short = r.la <= r.lb;
        const int32_t* S = idx + (a_short ? r.a0 : r.b0);
        const int32_t* Lg = idx + (a_short ? r.b0 : r.a0);
        const int m = block_sum<kDbWaves>(doublet_matches(S, a_short ? r.la : r.lb, Lg, a_short ? r.lb : r.la, (int)threadIdx.x, kDbBlock), s_w);
        if (threadIdx.x == 0) cnt[s] = (int64_t)(r.la + r.lb - m);
    }
}

// One side of a synthetic row: the entries X[0 .. lx) (values xv) against the other parent Y[0 .. ly) (values yv), by a wave
// (BLOCK false: all 64 lanes, 64 entries per round) or by the workgroup (BLOCK true: every thread, 256 per round).  A_SIDE: a
// matched entry is written with the sum of both values, in the order a + b; else a matched entry is skipped (the other side
// writes it).  `len` = the row's length in the output: a position beyond it (the input was not canonical) is not written.
template <typename VT, bool BLOCK, bool A_SIDE>
__device__ __forceinline__ void doublet_side(const int32_t* __restrict__ X, const VT* __restrict__ xv, int lx, const int32_t* __restrict__ Y,
                                             const VT* __restrict__ yv, int ly, int32_t* __restrict__ out_idx, VT* __restrict__ out_val,
                                             int len, int* s_w) {
    constexpr int STEP = BLOCK ? kDbBlock : kWave;
    const int t = BLOCK ? (int)threadIdx.x : lane_id();
    int run = 0;                                   // matches in the rounds before this one
    for (int i0 = 0; i0 < lx; i0 += STEP) {
        const int i = i0 + t;
        const bool in = i < lx;
        int32_t c = 0;
        int p = 0, m = 0;
        if (in) {
            c = X[i];
            p = doublet_lower_bound(Y, ly, c);
            m = (p < ly && Y[p] == c) ? 1 : 0;
        }
        int before, total;
        if (BLOCK) {
            before = block_scan_exclusive<kDbWaves>(m, s_w, total);
        } else {
            const int inc = wave_scan_inclusive(m);
            before = inc - m;
            total = __shfl(inc, kWave - 1, kWave);
        }
        const int pos = i + p - (run + before);
        if (in && (A_SIDE || !m) && pos < len) {
            out_idx[pos] = c;
            out_val[pos] = (A_SIDE && m) ? (VT)(xv[i] + yv[p]) : xv[i];
        }
        run += total;
        if (BLOCK) __syncthreads();                // the next round writes s_w again
    }
}

template <typename VT>
__global__ __launch_bounds__(kDbBlock) void k_doublet_fill(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                           const VT* __restrict__ vals, const uint64_t* __restrict__ parents,
                                                           uint64_t n_sim, const int64_t* __restrict__ out_ptr,
                                                           int32_t* __restrict__ out_idx, VT* __restrict__ out_val) {
    __shared__ int s_w[kDbWaves];
    const int wave = threadIdx.x / kWave;
    const uint64_t s0 = (uint64_t)blockIdx.x * kDbWaves;
    {
        const uint64_t s = s0 + wave;
        if (s < n_sim) {
            const DoubletRow r = doublet_row(indptr, parents, s);
            if (r.la + r.lb <= kDbWaveRow) {
                const int64_t o = out_ptr[s];
                const int len = (int)(out_ptr[s + 1] - o);
                doublet_side<VT, false, true>(idx + r.a0, vals + r.a0, r.la, idx + r.b0, vals + r.b0, r.lb, out_idx + o, out_val + o, len, s_w);
                doublet_side<VT, false, false>(idx + r.b0, vals + r.b0, r.lb, idx + r.a0, vals + r.a0, r.la, out_idx + o, out_val + o, len, s_w);
            }
        }
    }
    for (int w = 0; w < kDbWaves; ++w) {
        const uint64_t s = s0 + w;
        if (s >= n_sim) break;
        const DoubletRow r = doublet_row(indptr, parents, s);
        if (r.la + r.lb <= kDbWaveRow) continue;
        const int64_t o = out_ptr[s];
        const int len = (int)(out_ptr[s + 1] - o);
        doublet_side<VT, true, true>(idx + r.a0, vals + r.a0, r.la, idx + r.b0, vals + r.b0, r.lb, out_idx + o, out_val + o, len, s_w);
        doublet_side<VT, true, false>(idx + r.b0, vals + r.b0, r.lb, idx + r.a0, vals + r.a0, r.la, out_idx + o, out_val + o, len, s_w);
    }
}

__global__ __launch_bounds__(256) void k_doublet_scores(const uint32_t* __restrict__ knn, uint64_t n_tot, uint64_t n_obs, int k_adj,
                                                        double rho, double se_rho, double r, double* __restrict__ score,
                                                        double* __restrict__ se) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tot) return;
    const uint32_t* row = knn + i * (uint64_t)k_adj;
    int kd = 0;
    for (int j = 0; j < k_adj; ++j) kd += row[j] >= n_obs ? 1 : 0;
    const double q = (double)(kd + 1) / (double)(k_adj + 2);
    const double D = 1.0 - rho - q * (1.0 - rho - rho / r);
    const double Ld = q * rho / r / D;
    const double se_q = sqrt(q * (1.0 - q) / (double)(k_adj + 3));
    const double t1 = se_q / q * (1.0 - rho), t2 = se_rho / rho * (1.0 - q);
    const double se_Ld = q * rho / r / (D * D) * sqrt(t1 * t1 + t2 * t2);
    if (score) score[i] = Ld;
    if (se) se[i] = se_Ld;
}

__global__ __launch_bounds__(256) void k_doublet_call(const double* __restrict__ score, const double* __restrict__ se, uint64_t n_obs,
                                                      uint64_t n_tot, double t, uint8_t* __restrict__ pred, double* __restrict__ z,
                                                      unsigned long long* __restrict__ counts /* observed, simulated above t */) {
    __shared__ int s_w[256 / kWave];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    int obs = 0, sim = 0;
    if (i < n_obs) {
        const double v = score[i];
        obs = v > t ? 1 : 0;
        pred[i] = (uint8_t)obs;
        z[i] = (v - t) / se[i];
    } else if (i < n_tot) {
        sim = score[i] > t ? 1 : 0;
    }
    const int packed = block_sum<256 / kWave>(obs + (sim << 16), s_w);        // (at most 256 of each)
    if (threadIdx.x == 0 && packed) {
        if (packed & 0xFFFF) atomicAdd(&counts[0], (unsigned long long)(packed & 0xFFFF));
        if (packed >> 16) atomicAdd(&counts[1], (unsigned long long)(packed >> 16));
    }
}

// round to nearest, halves away from zero (x >= 0)
static uint64_t round_half_up(double x) { return (uint64_t)floor(x + 0.5); }

// Section 1 on the device.  d_parents: room for 2 n_sim on the device, filled here (from `parents`, checked, or by the hash).
static int32_t simulate_device(srx_mat* counts, uint64_t n_sim, uint64_t seed, const uint64_t* parents, uint64_t* d_parents,
                               srx_mat** out) {
    srx_ctx* ctx = counts->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = counts->n_rows;
    *out = nullptr;
    const int32_t dtype = is_f32(counts) ? SRX_F32 : SRX_F64;
    srx_mat* t = nullptr;
    if (n_sim == 0) {
        SRX_TRY(srx_matrix_alloc(ctx, 0, counts->n_cols, 0, dtype, counts->store, &t));
        const hipError_t e = hipMemsetAsync(t->d_indptr, 0, sizeof(int64_t), st);
        if (e != hipSuccess) {
            srx_matrix_free(t);
            return fail(ctx, SRX_E_HIP, "doublets: %s", hipGetErrorString(e));
        }
        t->store_auto = counts->store_auto;
        *out = t;
        return SRX_OK;
    }
    if (parents) {
        for (uint64_t i = 0; i < 2 * n_sim; ++i)
            if (parents[i] >= n)
                return fail(ctx, SRX_E_BOUNDS, "doublets: parent %llu of synthetic row %llu is %llu, not below %llu cells",
                            (unsigned long long)(i & 1), (unsigned long long)(i >> 1), (unsigned long long)parents[i], (unsigned long long)n);
        SRX_TRY(h2d(ctx, d_parents, parents, 2 * n_sim * sizeof(uint64_t)));
    } else {
        hipLaunchKernelGGL(k_doublet_parents, dim3(grid256(2 * n_sim)), dim3(256), 0, st, seed, n, 2 * n_sim, d_parents);
    }
    int64_t *d_cnt, *d_ptr, *d_total = nullptr;
    SRX_TRY(scratch(ctx, "doublet_cnt", n_sim * sizeof(int64_t), (void**)&d_cnt));
    SRX_TRY(scratch(ctx, "doublet_ptr", (n_sim + 1) * sizeof(int64_t), (void**)&d_ptr));
    const unsigned grid = (unsigned)((n_sim + kDbWaves - 1) / kDbWaves);
    hipLaunchKernelGGL(k_doublet_count, dim3(grid), dim3(kDbBlock), 0, st, (const int64_t*)counts->d_indptr, (const int32_t*)counts->d_indices,
                       (const uint64_t*)d_parents, n_sim, d_cnt);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(scan_exclusive(ctx, d_cnt, n_sim, d_ptr, &d_total));
    int64_t nnz = 0;
    SRX_TRY(d2h(ctx, &nnz, d_total, sizeof(int64_t)));
    SRX_TRY(srx_matrix_alloc(ctx, n_sim, counts->n_cols, (uint64_t)nnz, dtype, counts->store, &t));
    t->store_auto = counts->store_auto;          // as srx_matrix_clone: f32 storage of an AUTO matrix still widens at normalize_total
    hipError_t e = hipMemcpyAsync(t->d_indptr, d_ptr, (n_sim + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) {
        if (is_f32(counts))
            hipLaunchKernelGGL((k_doublet_fill<float>), dim3(grid), dim3(kDbBlock), 0, st, (const int64_t*)counts->d_indptr,
                               (const int32_t*)counts->d_indices, (const float*)counts->d_values, (const uint64_t*)d_parents, n_sim,
                               (const int64_t*)t->d_indptr, t->d_indices, (float*)t->d_values);
        else
            hipLaunchKernelGGL((k_doublet_fill<double>), dim3(grid), dim3(kDbBlock), 0, st, (const int64_t*)counts->d_indptr,
                               (const int32_t*)counts->d_indices, (const double*)counts->d_values, (const uint64_t*)d_parents, n_sim,
                               (const int64_t*)t->d_indptr, t->d_indices, (double*)t->d_values);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);         // the scratch offsets may be regrown by the next call
    if (e != hipSuccess) {
        srx_matrix_free(t);
        return fail(ctx, SRX_E_HIP, "doublets: the simulation failed: %s", hipGetErrorString(e));
    }
    *out = t;
    return SRX_OK;
}

static int32_t simulate_check(srx_mat* counts, uint64_t n_sim) {
    srx_ctx* ctx = counts->ctx;
    if (counts->csc) return fail(ctx, SRX_E_ARG, "doublets: counts are in CSC storage; convert with srx_matrix_to_csr");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "doublets: rows are sharded; the simulation draws parents from all cells");
    if (counts->n_rows == 0) return fail(ctx, SRX_E_ARG, "doublets: no cells");
    if (counts->n_rows + n_sim >= (1ull << 32) || n_sim >= (1ull << 32))
        return fail(ctx, SRX_E_ARG, "doublets: %llu cells and %llu synthetic rows exceed 2^32 - 1 points", (unsigned long long)counts->n_rows,
                    (unsigned long long)n_sim);
    return SRX_OK;
}

static int32_t rates_check(srx_ctx* ctx, double rho, double se_rho) {
    if (!(rho > 0.0 && rho < 1.0)) return fail(ctx, SRX_E_ARG, "doublets: expected_rate = %g outside (0, 1)", rho);
    if (!(se_rho >= 0.0) || !is_finite(se_rho)) return fail(ctx, SRX_E_ARG, "doublets: stdev_rate = %g is negative or not finite", se_rho);
    return SRX_OK;
}

// Section 5's automatic threshold
static void threshold_minimum(const double* x, uint64_t n, double* thr, int32_t* found, uint32_t* rounds) {
    *thr = NAN;
    *found = 0;
    *rounds = 0;
    if (n < 2) return;
    double mn = x[0], mx = x[0];
    for (uint64_t i = 0; i < n; ++i) {
        if (!is_finite(x[i])) return;
        mn = x[i] < mn ? x[i] : mn;
        mx = x[i] > mx ? x[i] : mx;
    }
    if (!(mx > mn)) return;
    const double w = mx - mn;
    constexpr int B = 256;
    std::vector<double> s(B, 0.0), nx(B);
    for (uint64_t i = 0; i < n; ++i) {
        const double b = floor((x[i] - mn) / w * 256.0);
        s[b >= 255.0 ? 255 : (int)b] += 1.0;
    }
    int mx_at[2] = {0, 0}, n_max = 0;
    uint32_t r = 0;
    do {
        for (int i = 0; i < B; ++i) nx[i] = (s[i ? i - 1 : 0] + s[i] + s[i < B - 1 ? i + 1 : B - 1]) / 3.0;
        s.swap(nx);
        ++r;
        n_max = 0;
        bool rising = true;
        for (int i = 0; i + 1 < B; ++i) {
            if (rising) {
                if (s[i + 1] < s[i]) {
                    if (n_max < 2) mx_at[n_max] = i;
                    ++n_max;
                    rising = false;
                }
            } else if (s[i + 1] > s[i]) {
                rising = true;
            }
        }
    } while (n_max >= 3 && r < SRX_DOUBLET_MAX_ROUNDS);
    *rounds = r;
    if (n_max != 2 || r >= SRX_DOUBLET_MAX_ROUNDS) return;
    int b = mx_at[0];
    for (int i = mx_at[0]; i <= mx_at[1]; ++i)
        if (s[i] < s[b]) b = i;
    *thr = mn + (b + 0.5) * w / 256.0;
    *found = 1;
}

// predicted, z and the rates of the handle for threshold t (0 = the automatic one)
static int32_t call_device(srx_doublets* h, double threshold) {
    srx_ctx* ctx = h->ctx;
    srx_doublet_info& info = h->info;
    const bool given = threshold > 0.0;
    const double t = given ? threshold : h->auto_threshold;
    info.threshold = t;
    info.threshold_found = given ? 0u : (uint32_t)h->auto_found;
    info.smooth_rounds = given ? 0u : h->auto_rounds;
    const uint64_t n_tot = h->n + h->n_sim;
    SRX_HIP(ctx, hipMemsetAsync(h->d_counts, 0, 2 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_doublet_call, dim3(grid256(n_tot)), dim3(256), 0, ctx->stream, (const double*)h->d_ld, (const double*)h->d_se, h->n,
                       n_tot, t, h->d_pred, h->d_z, h->d_counts);
    SRX_HIP(ctx, hipGetLastError());
    unsigned long long c[2] = {0, 0};
    SRX_TRY(d2h(ctx, c, h->d_counts, sizeof c));
    info.n_predicted = c[0];
    if (t == t) {
        info.detected_rate = (double)c[0] / (double)h->n;
        info.detectable_fraction = (double)c[1] / (double)h->n_sim;
        info.overall_rate = info.detected_rate / info.detectable_fraction;
    } else {
        info.detected_rate = info.detectable_fraction = info.overall_rate = NAN;
    }
    return SRX_OK;
}

struct DoubletOpts {
    double sim_ratio = 2.0, rho = 0.05, se_rho = 0.02, target_sum = 0.0, threshold = 0.0;
    uint64_t seed = 0;
    int k = 0, n_dims = 0, transform = 0;
};

static int32_t doublets_run(srx_mat* fitted, srx_mat* counts, const DoubletOpts& o, srx_doublets* h) {
    srx_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    srx_doublet_info& info = h->info;
    const uint64_t n = h->n, n_sim = h->n_sim, n_tot = n + n_sim;
    const uint64_t n_pc = fitted->pca.n_pc;
    StreamTimer t_sim(ctx, st), t_proj(ctx, st), t_knn(ctx, st), t_score(ctx, st);       // (a timer is started once)

    // 1. the synthetic matrix
    srx_mat* sim = nullptr;
    SRX_TRY(t_sim.start());
    SRX_TRY(simulate_device(counts, n_sim, o.seed, nullptr, h->d_parents, &sim));
    int32_t rc = t_sim.stop(&info.ms_simulate);
    info.nnz_sim = sim->nnz;

    // 2. the point block: the fit's scores as they lie, then the synthetic rows' scores written behind them
    srx_pca_model* model = nullptr;
    if (rc == SRX_OK) rc = t_proj.start();
    if (rc == SRX_OK) {
        hipError_t e = hipMemsetAsync(h->d_pts + n * h->ld, 0, n_sim * h->ld * sizeof(double), st);
        if (e == hipSuccess) e = hipMemcpyAsync(h->d_pts, fitted->pca.d_scores, n * h->ld * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) rc = fail(ctx, SRX_E_HIP, "doublets: copy of the fitted scores failed: %s", hipGetErrorString(e));
    }
    if (rc == SRX_OK) rc = srx_pca_model_from_result(fitted, &model);
    if (rc == SRX_OK) rc = pca_transform_device(model, sim, o.target_sum, o.transform, h->d_pts + n * h->ld, h->ld);
    if (rc == SRX_OK) rc = t_proj.stop(&info.ms_project);
    srx_pca_model_free(model);
    srx_matrix_free(sim);
    SRX_TRY(rc);

    // 3. neighbours of every point among all points
    srx_knn_opts ko{(int32_t)h->k_adj, (int32_t)h->d, 0, 0};
    srx_knn_info ki;
    const uint32_t* d_idx = nullptr;
    const double* d_dist = nullptr;
    uint64_t n_out = 0;
    SRX_TRY(t_knn.start());
    SRX_TRY(knn_self_device(ctx, h->d_pts, n_tot, n_pc, h->ld, &ko, nullptr, nullptr, &ki, &d_idx, &d_dist, &n_out));
    SRX_HIP(ctx, hipMemcpyAsync(h->d_knn, d_idx, n_tot * (size_t)h->k_adj * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    SRX_TRY(t_knn.stop(&info.ms_knn));
    info.rows_certified = ki.rows_certified;
    info.rows_recomputed = ki.rows_recomputed;

    // 4. scores; 5. the simulated ones go to the host for the threshold
    SRX_TRY(t_score.start());
    hipLaunchKernelGGL(k_doublet_scores, dim3(grid256(n_tot)), dim3(256), 0, st, (const uint32_t*)h->d_knn, n_tot, n, (int)h->k_adj, o.rho,
                       o.se_rho, h->r, h->d_ld, h->d_se);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_score.stop(&info.ms_score));
    h->sim_scores.resize(n_sim);
    SRX_TRY(d2h(ctx, h->sim_scores.data(), h->d_ld + n, n_sim * sizeof(double)));
    threshold_minimum(h->sim_scores.data(), n_sim, &h->auto_threshold, &h->auto_found, &h->auto_rounds);
    return call_device(h, o.threshold);
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_doublets_simulate(srx_mat* counts, uint64_t n_sim, uint64_t seed, const uint64_t* parents, srx_mat** out,
                              uint64_t* parents_out) {
    if (!counts || !out) return fail(counts ? counts->ctx : nullptr, SRX_E_ARG, "doublets: null argument");
    srx_ctx* ctx = counts->ctx;
    SRX_TRY(simulate_check(counts, n_sim));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t* d_parents;
    SRX_TRY(scratch(ctx, "doublet_parents", at_least_one(2 * n_sim) * sizeof(uint64_t), (void**)&d_parents));
    srx_mat* t = nullptr;
    SRX_TRY(simulate_device(counts, n_sim, seed, parents, d_parents, &t));
    if (parents_out && n_sim) {
        const int32_t rc = d2h(ctx, parents_out, d_parents, 2 * n_sim * sizeof(uint64_t));
        if (rc != SRX_OK) {
            srx_matrix_free(t);
            return rc;
        }
    }
    *out = t;
    return SRX_OK;
}

int32_t srx_doublet_scores_knn(srx_ctx* ctx, const uint32_t* indices, uint64_t n_obs, uint64_t n_sim, uint32_t k_adj,
                               double expected_rate, double stdev_rate, double* score_out, double* se_out) {
    if (!ctx || !indices) return fail(ctx, SRX_E_ARG, "doublets: null argument");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "doublets: a context with more than one rank");
    if (k_adj == 0 || k_adj >= (1u << 30)) return fail(ctx, SRX_E_ARG, "doublets: k_adj = %u", k_adj);
    if (n_obs == 0) return fail(ctx, SRX_E_ARG, "doublets: no observed rows");
    if (n_obs + n_sim >= (1ull << 32) || n_sim >= (1ull << 32)) return fail(ctx, SRX_E_ARG, "doublets: more than 2^32 - 1 rows");
    SRX_TRY(rates_check(ctx, expected_rate, stdev_rate));
    const uint64_t n_tot = n_obs + n_sim;
    for (uint64_t e = 0; e < n_tot * k_adj; ++e)
        if (indices[e] >= n_tot)
            return fail(ctx, SRX_E_ARG, "doublets: neighbour %llu of row %llu is %u, not below %llu rows", (unsigned long long)(e % k_adj),
                        (unsigned long long)(e / k_adj), indices[e], (unsigned long long)n_tot);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* d_idx;
    double* d_out;
    SRX_TRY(scratch(ctx, "doublet_list", n_tot * k_adj * sizeof(uint32_t), (void**)&d_idx));
    SRX_TRY(scratch(ctx, "doublet_list_scores", 2 * n_tot * sizeof(double), (void**)&d_out));
    SRX_TRY(h2d(ctx, d_idx, indices, n_tot * k_adj * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_doublet_scores, dim3(grid256(n_tot)), dim3(256), 0, ctx->stream, (const uint32_t*)d_idx, n_tot, n_obs, (int)k_adj,
                       expected_rate, stdev_rate, (double)n_sim / (double)n_obs, d_out, d_out + n_tot);
    SRX_HIP(ctx, hipGetLastError());
    if (score_out) SRX_TRY(d2h(ctx, score_out, d_out, n_tot * sizeof(double)));
    if (se_out) SRX_TRY(d2h(ctx, se_out, d_out + n_tot, n_tot * sizeof(double)));
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SRX_OK;
}

int32_t srx_doublets_threshold(const double* sim_scores, uint64_t n, double* threshold_out, int32_t* found_out, uint32_t* rounds_out) {
    if (!sim_scores && n) return fail(nullptr, SRX_E_ARG, "doublets: null scores");
    double thr;
    int32_t found;
    uint32_t rounds;
    threshold_minimum(sim_scores, n, &thr, &found, &rounds);
    if (threshold_out) *threshold_out = thr;
    if (found_out) *found_out = found;
    if (rounds_out) *rounds_out = rounds;
    return SRX_OK;
}

int32_t srx_doublets_result(srx_mat* fitted, srx_mat* counts, const srx_doublet_opts* opts, srx_doublets** out, srx_doublet_info* info) {
    if (!fitted || !counts || !out) return fail(fitted ? fitted->ctx : counts ? counts->ctx : nullptr, SRX_E_ARG, "doublets: null argument");
    srx_ctx* ctx = counts->ctx;
    if (fitted->ctx != ctx) return fail(ctx, SRX_E_ARG, "doublets: fitted and counts live on different contexts");
    DoubletOpts o;
    if (opts) {
        if (opts->sim_ratio < 0.0 || !is_finite(opts->sim_ratio)) return fail(ctx, SRX_E_ARG, "doublets: sim_ratio = %g", opts->sim_ratio);
        if (opts->threshold < 0.0 || opts->threshold != opts->threshold) return fail(ctx, SRX_E_ARG, "doublets: threshold = %g", opts->threshold);
        if (opts->k < 0) return fail(ctx, SRX_E_ARG, "doublets: k = %d", opts->k);
        if (opts->n_dims < 0) return fail(ctx, SRX_E_ARG, "doublets: n_dims = %d", opts->n_dims);
        if (opts->transform & ~(SRX_BACKED_NORMALIZE | SRX_BACKED_LOG1P)) return fail(ctx, SRX_E_ARG, "doublets: bad transform bits %d", opts->transform);
        if (opts->sim_ratio != 0.0) o.sim_ratio = opts->sim_ratio;
        if (opts->expected_rate != 0.0) o.rho = opts->expected_rate;
        if (opts->stdev_rate != 0.0) o.se_rho = opts->stdev_rate;
        o.target_sum = opts->target_sum;
        o.threshold = opts->threshold;
        o.seed = opts->seed;
        o.k = opts->k;
        o.n_dims = opts->n_dims;
        o.transform = opts->transform;
    }
    SRX_TRY(rates_check(ctx, o.rho, o.se_rho));
    if (!fitted->pca.valid || !fitted->pca.d_small) return fail(ctx, SRX_E_ARG, "doublets: no PCA result on the fitted matrix");
    if (fitted->pca.residual == kResidualRegress)
        return fail(ctx, SRX_E_ARG, "doublets: the fitted result is a PCA of regressed, scaled and clipped values (srx_pca_regress); the "
                                    "simulated cells are projected by srx_pca_transform, which has no covariates to regress out of them");
    if (fitted->pca.residual)
        return fail(ctx, SRX_E_ARG, "doublets: the fitted result is a PCA of Pearson residuals (srx_pca_pearson); the simulated cells are "
                                    "projected by srx_pca_transform, which has no residual model");
    if (counts->csc) return fail(ctx, SRX_E_ARG, "doublets: counts are in CSC storage; convert with srx_matrix_to_csr");
    const uint64_t n = counts->n_rows;
    const uint64_t fit_cells = fitted->csc ? fitted->n_cols : fitted->n_rows, fit_genes = fitted->csc ? fitted->n_rows : fitted->n_cols;
    if (fit_cells != n || fit_genes != counts->n_cols)
        return fail(ctx, SRX_E_ARG, "doublets: fitted is %llu x %llu but counts are %llu x %llu", (unsigned long long)fit_cells,
                    (unsigned long long)fit_genes, (unsigned long long)n, (unsigned long long)counts->n_cols);
    if (o.sim_ratio * (double)n >= 4294967296.0) return fail(ctx, SRX_E_ARG, "doublets: sim_ratio = %g of %llu cells", o.sim_ratio, (unsigned long long)n);
    const uint64_t n_sim = round_half_up(o.sim_ratio * (double)n);
    SRX_TRY(simulate_check(counts, n_sim));
    if (n_sim == 0) return fail(ctx, SRX_E_ARG, "doublets: sim_ratio = %g of %llu cells gives no synthetic row", o.sim_ratio, (unsigned long long)n);
    const uint64_t n_tot = n + n_sim, n_pc = fitted->pca.n_pc;
    const double r = (double)n_sim / (double)n;
    const uint64_t k = o.k ? (uint64_t)o.k : round_half_up(0.5 * sqrt((double)n));
    const uint64_t k_adj = round_half_up((double)k * (1.0 + r));
    if (k_adj < 1 || k_adj > SRX_DOUBLET_MAX_K)
        return fail(ctx, SRX_E_ARG, "doublets: k = %llu with %g synthetic rows per cell searches %llu neighbours, outside 1..%d; choose k or a smaller sim_ratio",
                    (unsigned long long)k, r, (unsigned long long)k_adj, SRX_DOUBLET_MAX_K);
    if (k_adj > n_tot - 1)
        return fail(ctx, SRX_E_ARG, "doublets: %llu neighbours but only %llu other points", (unsigned long long)k_adj, (unsigned long long)(n_tot - 1));
    if ((uint64_t)o.n_dims > n_pc) return fail(ctx, SRX_E_ARG, "doublets: n_dims = %d but the fit has %llu components", o.n_dims, (unsigned long long)n_pc);
    const uint64_t d = o.n_dims ? (uint64_t)o.n_dims : n_pc;
    if (d < 1 || d > SRX_KNN_MAX_DIMS) return fail(ctx, SRX_E_ARG, "doublets: %llu coordinates outside 1..%d", (unsigned long long)d, SRX_KNN_MAX_DIMS);
    SRX_HIP(ctx, hipSetDevice(ctx->device));

    auto* h = new srx_doublets;
    h->ctx = ctx;
    h->n = n;
    h->n_sim = n_sim;
    h->k_adj = (uint32_t)k_adj;
    h->d = (uint32_t)d;
    h->ld = (size_t)scores_ld((int)n_pc);
    h->r = r;
    const size_t b_pts = up256(n_tot * h->ld * 8), b_tot = up256(n_tot * 8), b_obs = up256(n * 8), b_par = up256(2 * n_sim * 8),
                 b_knn = up256(n_tot * k_adj * 4), b_pred = up256(n);
    const size_t bytes = b_pts + 2 * b_tot + b_obs + b_par + b_knn + b_pred + 256;
    const hipError_t e = hipMalloc(&h->d_block, bytes);
    if (e != hipSuccess) {
        delete h;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "doublets: hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    char* p = static_cast<char*>(h->d_block);
    h->d_pts = reinterpret_cast<double*>(p);
    h->d_ld = reinterpret_cast<double*>(p += b_pts);
    h->d_se = reinterpret_cast<double*>(p += b_tot);
    h->d_z = reinterpret_cast<double*>(p += b_tot);
    h->d_parents = reinterpret_cast<uint64_t*>(p += b_obs);
    h->d_knn = reinterpret_cast<uint32_t*>(p += b_par);
    h->d_pred = reinterpret_cast<uint8_t*>(p += b_knn);
    h->d_counts = reinterpret_cast<unsigned long long*>(p += b_pred);
    h->info.n_obs = n;
    h->info.n_sim = n_sim;
    h->info.k = (uint32_t)k;
    h->info.k_adj = (uint32_t)k_adj;
    h->info.d = (uint32_t)d;
    int32_t rc;
    {
        Range rg("doublets");
        rc = doublets_run(fitted, counts, o, h);
    }
    if (rc != SRX_OK) {
        srx_doublets_free(h);
        return rc;
    }
    if (info) *info = h->info;
    *out = h;
    return SRX_OK;
}

int32_t srx_doublets_call(srx_doublets* h, double threshold, srx_doublet_info* info) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null doublets handle");
    srx_ctx* ctx = h->ctx;
    if (threshold < 0.0 || threshold != threshold) return fail(ctx, SRX_E_ARG, "doublets: threshold = %g", threshold);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    SRX_TRY(call_device(h, threshold));
    if (info) *info = h->info;
    return SRX_OK;
}

int32_t srx_doublets_fetch(srx_doublets* h, int32_t which, void* out) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null doublets handle");
    srx_ctx* ctx = h->ctx;
    if (which < SRX_DOUBLETS_SCORES_OBS || which > SRX_DOUBLETS_KNN) return fail(ctx, SRX_E_ARG, "srx_doublets_fetch: which = %d names no table", which);
    if (!out) return fail(ctx, SRX_E_ARG, "srx_doublets_fetch: null output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n = h->n, n_sim = h->n_sim, n_tot = n + n_sim;
    switch (which) {
        case SRX_DOUBLETS_SCORES_OBS: return d2h(ctx, out, h->d_ld, n * 8);
        case SRX_DOUBLETS_SCORES_SIM: return d2h(ctx, out, h->d_ld + n, n_sim * 8);
        case SRX_DOUBLETS_SE_OBS: return d2h(ctx, out, h->d_se, n * 8);
        case SRX_DOUBLETS_SE_SIM: return d2h(ctx, out, h->d_se + n, n_sim * 8);
        case SRX_DOUBLETS_Z: return d2h(ctx, out, h->d_z, n * 8);
        case SRX_DOUBLETS_PREDICTED: return d2h(ctx, out, h->d_pred, n);
        case SRX_DOUBLETS_POINTS: return d2h_rows(ctx, out, h->d_pts, n_tot, (size_t)h->d * 8, h->ld * 8);
        case SRX_DOUBLETS_PARENTS: return d2h(ctx, out, h->d_parents, 2 * n_sim * 8);
        default: return d2h(ctx, out, h->d_knn, n_tot * (size_t)h->k_adj * 4);
    }
}

int32_t srx_doublets_info_get(const srx_doublets* h, srx_doublet_info* info) {
    if (!h || !info) return fail(h ? h->ctx : nullptr, SRX_E_ARG, "null argument");
    *info = h->info;
    return SRX_OK;
}

void srx_doublets_free(srx_doublets* h) {
    if (!h) return;
    if (h->d_block) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        (void)hipFree(h->d_block);
    }
    delete h;
}

}  // extern "C"
