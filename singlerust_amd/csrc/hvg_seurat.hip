// hvg_seurat.hip — highly variable genes as scanpy's flavor = "seurat_v3" chooses them, on the RAW counts, with batches
// (srx.h: srx_select_hvg_seurat_v3, srx_loess_direct, srx_clipped_group_moments).
//
// Per batch: the moments of every gene (markers.hip's walk over label-sorted rows: the batch is the group), a direct loess fit
// of log10(var) on log10(mean) over the genes that vary, a clip per (batch, gene) from the fitted variance, the moments of
// the clipped values (the same walk once more, with the clip table read beside the values) and the normalised variance.
// Then ranks per batch (select.hip's rank_keys_device), the median rank over the batches and the final order.
// Every floating-point sum has one fixed order (a fit's moments: lanes counted from the first weighted point, one butterfly);
// the sums over the stored entries are 64-bit fixed point with integer atomics.  No floating-point atomics.
#include "markers_internal.hpp"
#include "pca_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// srx.h states the order of every operation
#pragma clang fp contract(off)

namespace srx {

constexpr int kSvLoessThreads = 256;                       // four fit points per workgroup, a wave each
constexpr int kSvLoessWaves = kSvLoessThreads / kWave;
constexpr double kSvRankTol = 0x1p-33;                     // the degree rule of srx.h

__device__ __forceinline__ double sv_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double sv_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double sv_add(double a, double b) { return a + b; }
__device__ __forceinline__ double sv_div(double a, double b) { return a / b; }

// ---- step 1: mean, var of every (batch, gene); the trend's abscissa and ordinate; the sort key of the abscissa ------------------
// key = -x for a gene that varies (rank_keys_device orders by key descending, index ascending: x ascending), -inf otherwise,
// so that the m genes that vary take the places 0 .. m - 1.  m is counted with integer atomics, one per wave and batch.
__global__ __launch_bounds__(256) void k_sv_stats(const long long* __restrict__ S, const long long* __restrict__ Q,
                                                  const uint64_t* __restrict__ sizes, uint32_t n_batches, uint64_t G, double inv_sum,
                                                  double inv_sq, double* __restrict__ mean, double* __restrict__ var,
                                                  double* __restrict__ lx, double* __restrict__ ly, double* __restrict__ key,
                                                  uint32_t* __restrict__ m_of) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < (uint64_t)n_batches * G;
    bool varies = false;
    uint32_t b = 0;
    if (in) {
        b = (uint32_t)(i / G);
        const double n = (double)sizes[b];
        const double s = sv_mul((double)S[i], inv_sum), q = sv_mul((double)Q[i], inv_sq);
        const double mu = sv_div(s, n);
        const double v = sv_mul(sv_sub(sv_div(q, n), sv_mul(mu, mu)), sv_div(n, sv_sub(n, 1.0)));
        varies = v > 0.0;
        mean[i] = mu;
        var[i] = v;
        const double x = varies ? log10(mu) : 0.0;
        lx[i] = x;
        ly[i] = varies ? log10(v) : 0.0;
        key[i] = varies ? -x : -INFINITY;
    }
    // one atomic per wave and batch (a wave straddles batches where G is no multiple of 64): the lanes of the first batch
    // that still has one are counted by a ballot, its first lane adds
    unsigned long long left = __ballot(varies);
    while (left) {
        const int first = __ffsll((long long)left) - 1;
        const uint32_t bf = __shfl(b, first, kWave);
        const unsigned long long same = __ballot(varies && b == bf);
        if (lane_id() == first) atomicAdd(&m_of[bf], (uint32_t)__popcll(same));
        left &= ~same;
    }
}

// the genes that vary, in the order of their abscissa: place p of batch b holds (x, y, gene)
__global__ __launch_bounds__(256) void k_sv_scatter(const double* __restrict__ lx, const double* __restrict__ ly,
                                                    const double* __restrict__ key, const uint32_t* __restrict__ rank, uint32_t n_batches,
                                                    uint64_t G, double* __restrict__ xs, double* __restrict__ ys,
                                                    uint32_t* __restrict__ gene_of) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_batches * G || !(key[i] > -INFINITY)) return;
    const uint64_t row = i / G * G;
    const uint64_t at = row + rank[i];                 // rank < m <= G for a gene that varies
    xs[at] = lx[i];
    ys[at] = ly[i];
    gene_of[at] = (uint32_t)(i - row);
}

// ---- step 2: the direct loess fit, a wave per fit point, every batch in one launch --------------------------------------------
// xs ascending.  The q nearest points of place p are a window [s, s + q) that holds p; h = min over s of
// max(x_p - x[s], x[s + q - 1] - x_p): the first term falls with s, the second rises, so the minimum lies where they cross
// (a binary search).  The weighted points (distance < h; h == 0: distance == 0) are again one run [a, b), found by two more
// searches; both depend on the VALUE x_p alone, so tied fit points walk the same run in the same lane assignment.
__global__ __launch_bounds__(kSvLoessThreads) void k_sv_loess(const double* __restrict__ xs, const double* __restrict__ ys,
                                                               const uint32_t* __restrict__ gene_of, const uint32_t* __restrict__ m_of,
                                                               uint64_t stride, double span, double* __restrict__ fitted) {
    const uint32_t b = blockIdx.y;
    const uint32_t m = m_of[b];
    const uint32_t p = blockIdx.x * kSvLoessWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    if (p >= m) return;                         // (a whole wave; the kernel has no workgroup barrier)
    const double* x = xs + (uint64_t)b * stride;
    const double* y = ys + (uint64_t)b * stride;
    const int lane = lane_id();
    const double xp = x[p];
    // q = min(m, max(1, floor(span m + 1e-5)))
    double qd = floor(sv_add(sv_mul(span, (double)m), 1e-5));
    qd = qd < 1.0 ? 1.0 : qd;
    const uint32_t q = qd >= (double)m ? m : (uint32_t)qd;
    // the windows that hold p: s in [s_lo, s_hi]
    const uint32_t s_lo = p + 1 >= q ? p + 1 - q : 0u, s_hi = p < m - q ? p : m - q;
    // the first s with x[s + q - 1] - x_p >= x_p - x[s], or s_hi where none is
    uint32_t lo = s_lo, hi = s_hi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sv_sub(x[mid + q - 1], xp) >= sv_sub(xp, x[mid])) hi = mid; else lo = mid + 1;
    }
    auto reach = [&](uint32_t s) {
        const double l = sv_sub(xp, x[s]), r = sv_sub(x[s + q - 1], xp);
        return l > r ? l : r;
    };
    double h = reach(lo);
    if (lo > s_lo) {
        const double h2 = reach(lo - 1);
        h = h2 < h ? h2 : h;
    }
    // the run of weighted points: [a, e).  Left of p the distance x_p - x[i] falls with i, right of p it rises.
    uint32_t a, e;
    {
        uint32_t l0 = 0, l1 = p;                       // the first i <= p with a weight
        while (l0 < l1) {
            const uint32_t mid = l0 + ((l1 - l0) >> 1);
            const double d = sv_sub(xp, x[mid]);
            if (h > 0.0 ? d < h : d == 0.0) l1 = mid; else l0 = mid + 1;
        }
        a = l0;
        uint32_t r0 = p + 1, r1 = m;                   // the first i > p without one
        while (r0 < r1) {
            const uint32_t mid = r0 + ((r1 - r0) >> 1);
            const double d = sv_sub(x[mid], xp);
            if (h > 0.0 ? d < h : d == 0.0) r0 = mid + 1; else r1 = mid;
        }
        e = r0;
    }
    // the eight moments: lane l takes the points a + l, a + l + 64, .. in that order
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
    for (uint32_t i = a + (uint32_t)lane; i < e; i += kWave) {
        double t = 0.0, w = 1.0;
        if (h > 0.0) {
            t = sv_div(sv_sub(x[i], xp), h);
            const double u = fabs(t);
            const double c = sv_sub(1.0, sv_mul(sv_mul(u, u), u));
            w = sv_mul(sv_mul(c, c), c);
        }
        const double yi = y[i];
        const double wt = sv_mul(w, t), wt2 = sv_mul(wt, t);
        m0 = sv_add(m0, w);
        m1 = sv_add(m1, wt);
        m2 = sv_add(m2, wt2);
        m3 = sv_add(m3, sv_mul(wt2, t));
        m4 = sv_add(m4, sv_mul(sv_mul(wt2, t), t));
        b0 = sv_add(b0, sv_mul(w, yi));
        b1 = sv_add(b1, sv_mul(wt, yi));
        b2 = sv_add(b2, sv_mul(wt2, yi));
    }
    m0 = wave_sum(m0); m1 = wave_sum(m1); m2 = wave_sum(m2); m3 = wave_sum(m3); m4 = wave_sum(m4);
    b0 = wave_sum(b0); b1 = wave_sum(b1); b2 = wave_sum(b2);
    if (lane != 0) return;
    // the intercept of the weighted least-squares fit by Cramer's rule, at the degree the moments support (srx.h)
    const double c00 = sv_sub(sv_mul(m2, m4), sv_mul(m3, m3));
    const double c01 = sv_sub(sv_mul(m1, m4), sv_mul(m2, m3));
    const double c02 = sv_sub(sv_mul(m1, m3), sv_mul(m2, m2));
    const double det = sv_add(sv_sub(sv_mul(m0, c00), sv_mul(m1, c01)), sv_mul(m2, c02));
    const double d2 = sv_sub(sv_mul(m0, m2), sv_mul(m1, m1));
    double fit;
    if (det > sv_mul(kSvRankTol, sv_mul(sv_mul(m0, m2), m4))) {
        const double n01 = sv_sub(sv_mul(b1, m4), sv_mul(b2, m3));
        const double n02 = sv_sub(sv_mul(b1, m3), sv_mul(b2, m2));
        fit = sv_div(sv_add(sv_sub(sv_mul(b0, c00), sv_mul(m1, n01)), sv_mul(m2, n02)), det);
    } else if (d2 > sv_mul(kSvRankTol, sv_mul(m0, m2))) {
        fit = sv_div(sv_sub(sv_mul(b0, m2), sv_mul(b1, m1)), d2);
    } else {
        fit = sv_div(b0, m0);
    }
    fitted[(uint64_t)b * stride + gene_of[(uint64_t)b * stride + p]] = fit;
}

// ---- step 3: the clip of every (batch, gene), and after the clipped walk the normalised variance --------------------------------
__global__ __launch_bounds__(256) void k_sv_clip(const double* __restrict__ mean, const double* __restrict__ fitted,
                                                 const uint64_t* __restrict__ sizes, uint32_t n_batches, uint64_t G,
                                                 double* __restrict__ reg_var, double* __restrict__ clip) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_batches * G) return;
    const double n = (double)sizes[i / G];
    const double rv = pow(10.0, fitted[i]);          // the one operation of the method that is not correctly rounded: kept as a table
    reg_var[i] = rv;
    clip[i] = sv_add(sv_mul(sqrt(rv), sqrt(n)), mean[i]);
}
__global__ __launch_bounds__(256) void k_sv_nv(const double* __restrict__ mean, const double* __restrict__ reg_var,
                                               const long long* __restrict__ Sc, const long long* __restrict__ Qc,
                                               const uint64_t* __restrict__ sizes, uint32_t n_batches, uint64_t G, double inv_sum,
                                               double inv_sq, double* __restrict__ clip_sum, double* __restrict__ clip_sumsq,
                                               double* __restrict__ nv, uint32_t* __restrict__ rank) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_batches * G) return;
    const double n = (double)sizes[i / G];
    const double sc = sv_mul((double)Sc[i], inv_sum), qc = sv_mul((double)Qc[i], inv_sq);
    const double mu = mean[i];
    const double num = sv_sub(sv_add(sv_mul(n, sv_mul(mu, mu)), qc), sv_mul(sv_mul(2.0, sc), mu));
    clip_sum[i] = sc;
    clip_sumsq[i] = qc;
    nv[i] = sv_div(num, sv_mul(sv_sub(n, 1.0), reg_var[i]));
    rank[i] = 0u;                               // rank_keys_device adds to it
}

// ---- steps 4 and 5: per gene over the batches -----------------------------------------------------------------------------------
// The k-th smallest of the ranks below n_top by bisection on the value (ranks are integers below G): count(v) = the number of
// batches with rank <= v.  key: the final order as one integer-valued f64 for rank_keys_device (descending, index ascending).
__device__ __forceinline__ uint32_t sv_kth(const uint32_t* __restrict__ rank, uint32_t n_batches, uint64_t G, uint64_t j, uint32_t n_top,
                                           uint32_t k) {
    uint32_t lo = 0, hi = n_top - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        uint32_t c = 0;
        for (uint32_t b = 0; b < n_batches; ++b) c += rank[(uint64_t)b * G + j] <= mid ? 1u : 0u;
        if (c >= k + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__global__ __launch_bounds__(256) void k_sv_combine(const uint32_t* __restrict__ rank, const double* __restrict__ nv,
                                                    const long long* __restrict__ totS, const long long* __restrict__ totQ,
                                                    uint32_t n_batches, uint64_t G, uint64_t n_cells, uint32_t n_top, int paper,
                                                    double inv_sum, double inv_sq, double* __restrict__ means,
                                                    double* __restrict__ variances, double* __restrict__ vnorm,
                                                    double* __restrict__ median, uint32_t* __restrict__ nbatches,
                                                    double* __restrict__ key, uint32_t* __restrict__ final_rank) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    uint32_t nb = 0;
    double sum = 0.0;
    for (uint32_t b = 0; b < n_batches; ++b) {
        nb += rank[(uint64_t)b * G + j] < n_top ? 1u : 0u;
        sum = sv_add(sum, nv[(uint64_t)b * G + j]);
    }
    double med2 = 0.0;                          // 2 x median: an integer
    if (nb) {
        const uint32_t hi_k = sv_kth(rank, n_batches, G, j, n_top, nb / 2);
        const uint32_t lo_k = (nb & 1u) ? hi_k : sv_kth(rank, n_batches, G, j, n_top, nb / 2 - 1);
        med2 = sv_add((double)lo_k, (double)hi_k);
    }
    const double n = (double)n_cells;
    const double mu = sv_div(sv_mul((double)totS[j], inv_sum), n);
    means[j] = mu;
    variances[j] = sv_mul(sv_sub(sv_div(sv_mul((double)totQ[j], inv_sq), n), sv_mul(mu, mu)), sv_div(n, sv_sub(n, 1.0)));
    vnorm[j] = sv_div(sum, (double)n_batches);
    median[j] = nb ? sv_mul(med2, 0.5) : NAN;
    nbatches[j] = nb;
    // 2 median < 2^33 and nbatches <= 4096: both keys are integers below 2^47, exact in f64
    double k = -INFINITY;
    if (nb) k = paper ? sv_sub(sv_mul((double)nb, 0x1p34), med2) : -sv_add(sv_mul(med2, (double)(n_batches + 1)), (double)(n_batches - nb));
    key[j] = k;
    final_rank[j] = 0u;
}
// f64(fixed-point integer) x 2^-scale, a whole table
__global__ __launch_bounds__(256) void k_sv_unfix(const long long* __restrict__ in, uint64_t n, double inv, double* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sv_mul((double)in[i], inv);
}
// fitted values back in the caller's order (srx_loess_direct)
__global__ __launch_bounds__(256) void k_sv_negate(const double* __restrict__ x, uint64_t n, double* __restrict__ key, uint32_t* __restrict__ rank) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        key[i] = -x[i];
        rank[i] = 0u;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
struct DevBlock {
    srx_ctx* ctx;
    void* p = nullptr;
    ~DevBlock() {
        if (p) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(p);
        }
    }
};
struct MkHolder {
    srx_markers* mk = nullptr;
    ~MkHolder() { mk_free(mk); }
};

static int32_t sv_alloc(srx_ctx* ctx, DevBlock& blk, size_t bytes, const char* who) {
    hipError_t e = dev_malloc(ctx, &blk.p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        blk.p = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "%s: the tables (%zu bytes) do not fit: %s", who, bytes, hipGetErrorString(e));
    }
    return SRX_OK;
}

static bool sv_span_ok(double span) { return span > 0.0 && span <= 1.0; }

// the sort of every batch's abscissae, the scatter and the fits: lx, ly, key are n_batches x G; fitted has been zeroed
static int32_t sv_loess(srx_ctx* ctx, const double* d_lx, const double* d_ly, const double* d_key, const uint32_t* d_m, uint32_t n_batches,
                        uint64_t G, double span, uint32_t* d_rank, double* d_xs, double* d_ys, uint32_t* d_gene, double* d_fitted) {
    hipStream_t st = ctx->stream;
    const uint64_t cells = (uint64_t)n_batches * G;
    for (uint32_t b = 0; b < n_batches; ++b) SRX_TRY(rank_keys_device(ctx, d_key + (uint64_t)b * G, G, d_rank + (uint64_t)b * G));
    hipLaunchKernelGGL(k_sv_scatter, dim3(grid256(cells)), dim3(256), 0, st, d_lx, d_ly, d_key, (const uint32_t*)d_rank, n_batches, G, d_xs, d_ys,
                       d_gene);
    SRX_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_sv_loess, dim3((unsigned)((G + kSvLoessWaves - 1) / kSvLoessWaves), n_batches), dim3(kSvLoessThreads), 0, st,
                       (const double*)d_xs, (const double*)d_ys, (const uint32_t*)d_gene, d_m, G, span, d_fitted);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

static int32_t sv_begin(srx_mat* m, const char* who) {
    SRX_TRY(markers_check(m, who));
    srx_ctx* ctx = m->ctx;
    if (ctx->pool_on > 0) return fail(ctx, SRX_E_ARG, "%s: a backed session is open on this context (the out-of-core form is out of scope)", who);
    if (m->n_cols >= 0xffffffffull) return fail(ctx, SRX_E_ARG, "%s: %llu genes", who, (unsigned long long)m->n_cols);
    return SRX_OK;
}

static int32_t sv_refuse_negative(srx_mat* m, const char* who) {
    srx_ctx* ctx = m->ctx;
    if (!m->nnz) return SRX_OK;
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "seurat_bad", 256, (void**)&d_small));
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, 256, ctx->stream));
    value_scan(m, d_small);
    SRX_HIP(ctx, hipGetLastError());
    unsigned long long flags = 0;
    SRX_TRY(d2h(ctx, &flags, d_small + VS_FLAGS, sizeof flags));
    if (flags & kValNegative) return fail(ctx, SRX_E_ARG, "%s: the matrix holds a negative value (raw counts are expected)", who);
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_loess_direct(srx_ctx* ctx, const double* x, const double* y, uint64_t m, double span, double* fitted_out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "srx_loess_direct: null context");
    if (m && (!x || !y || !fitted_out)) return fail(ctx, SRX_E_ARG, "srx_loess_direct: null argument");
    if (!sv_span_ok(span)) return fail(ctx, SRX_E_ARG, "srx_loess_direct: span = %g is outside (0, 1]", span);
    if (m >= 0xffffffffull) return fail(ctx, SRX_E_ARG, "srx_loess_direct: %llu points", (unsigned long long)m);
    for (uint64_t i = 0; i < m; ++i)
        if (!is_finite(x[i]) || !is_finite(y[i])) return fail(ctx, SRX_E_NAN, "srx_loess_direct: point %llu is NaN or Inf", (unsigned long long)i);
    if (!m) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    DevBlock blk{ctx};
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
    const size_t ox = carve(m * 8), oy = carve(m * 8), ok = carve(m * 8), oxs = carve(m * 8), oys = carve(m * 8), of = carve(m * 8),
                 orank = carve(m * 4), og = carve(m * 4), om = carve(4);
    SRX_TRY(sv_alloc(ctx, blk, off, "srx_loess_direct"));
    char* base = (char*)blk.p;
    double *d_x = (double*)(base + ox), *d_y = (double*)(base + oy), *d_key = (double*)(base + ok), *d_xs = (double*)(base + oxs),
           *d_ys = (double*)(base + oys), *d_fit = (double*)(base + of);
    uint32_t *d_rank = (uint32_t*)(base + orank), *d_gene = (uint32_t*)(base + og), *d_m = (uint32_t*)(base + om);
    SRX_TRY(h2d(ctx, d_x, x, m * 8));
    SRX_TRY(h2d(ctx, d_y, y, m * 8));
    const uint32_t m32 = (uint32_t)m;
    SRX_TRY(h2d(ctx, d_m, &m32, 4));
    SRX_HIP(ctx, hipMemsetAsync(d_fit, 0, m * 8, ctx->stream));
    hipLaunchKernelGGL(k_sv_negate, dim3(grid256(m)), dim3(256), 0, ctx->stream, (const double*)d_x, m, d_key, d_rank);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(sv_loess(ctx, d_x, d_y, d_key, d_m, 1, m, span, d_rank, d_xs, d_ys, d_gene, d_fit));
    std::vector<double> fit(m);
    SRX_TRY(d2h(ctx, fit.data(), d_fit, m * 8));
    memcpy(fitted_out, fit.data(), m * 8);
    return SRX_OK;
}

int32_t srx_clipped_group_moments(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const double* clip, double* sum_out,
                                  double* sumsq_out, srx_markers_info* info) {
    SRX_TRY(sv_begin(m, "srx_clipped_group_moments"));
    srx_ctx* ctx = m->ctx;
    if (!clip) return fail(ctx, SRX_E_ARG, "srx_clipped_group_moments: null clip table");
    if (n_groups < 1 || n_groups > SRX_GROUPS_MAX)
        return fail(ctx, SRX_E_ARG, "srx_clipped_group_moments: n_groups = %u is outside 1 .. %d", n_groups, SRX_GROUPS_MAX);
    const uint64_t G = m->n_cols, cells = (uint64_t)n_groups * G;
    for (uint64_t i = 0; i < cells; ++i)
        if (!(clip[i] >= 0.0)) return fail(ctx, SRX_E_ARG, "srx_clipped_group_moments: clip[%llu] = %g (negative or NaN)", (unsigned long long)i, clip[i]);
    uint32_t* d_labels;
    SRX_TRY(markers_host_labels(m, labels, n_groups, "srx_clipped_group_moments", &d_labels));
    MkHolder hold;
    MkPlan plan;
    SRX_TRY(markers_moments(m, d_labels, n_groups, false, &hold.mk, &plan));
    std::vector<double> sum, sumsq;
    if (cells) {
        DevBlock blk{ctx};
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
        const size_t oc = carve(cells * 8), oS = carve(cells * 8), oQ = carve(cells * 8), oo = carve(cells * 8);
        SRX_TRY(sv_alloc(ctx, blk, off, "srx_clipped_group_moments"));
        char* base = (char*)blk.p;
        double *d_clip = (double*)(base + oc), *d_out = (double*)(base + oo);
        long long *d_S = (long long*)(base + oS), *d_Q = (long long*)(base + oQ);
        SRX_TRY(h2d(ctx, d_clip, clip, cells * 8));
        SRX_HIP(ctx, hipMemsetAsync(d_S, 0, oo - oS, ctx->stream));
        SRX_TRY(markers_clipped_walk(m, plan, d_clip, (unsigned long long*)d_S, (unsigned long long*)d_Q));
        const double inv_sum = std::ldexp(1.0, -hold.mk->info.sum_scale_log2), inv_sq = std::ldexp(1.0, -hold.mk->info.sq_scale_log2);
        auto fetch = [&](const long long* d_in, double inv, std::vector<double>& out) -> int32_t {
            out.resize(cells);
            hipLaunchKernelGGL(k_sv_unfix, dim3(grid256(cells)), dim3(256), 0, ctx->stream, d_in, cells, inv, d_out);
            SRX_HIP(ctx, hipGetLastError());
            return d2h(ctx, out.data(), d_out, cells * 8);
        };
        if (sum_out) SRX_TRY(fetch(d_S, inv_sum, sum));
        if (sumsq_out) SRX_TRY(fetch(d_Q, inv_sq, sumsq));
    }
    if (!sum.empty()) memcpy(sum_out, sum.data(), cells * 8);
    if (!sumsq.empty()) memcpy(sumsq_out, sumsq.data(), cells * 8);
    if (info) *info = hold.mk->info;
    return SRX_OK;
}

int32_t srx_select_hvg_seurat_v3(srx_mat* m, uint64_t n_top, const uint32_t* batch, uint32_t n_batches, const srx_seurat_v3_opts* opts,
                                 uint64_t* idx_out, uint64_t* n_out, srx_seurat_v3_tables* tables, srx_seurat_v3_info* info_out) {
    const char* who = "srx_select_hvg_seurat_v3";
    if (!m || !idx_out || !n_out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "%s: null argument", who);
    SRX_TRY(sv_begin(m, who));
    srx_ctx* ctx = m->ctx;
    if (n_top == 0) return fail(ctx, SRX_E_ARG, "%s: n_top = 0", who);
    const double span = opts && opts->span != 0.0 ? opts->span : 0.3;
    if (!sv_span_ok(span)) return fail(ctx, SRX_E_ARG, "%s: span = %g is outside (0, 1]", who, span);
    if (n_batches < 1 || n_batches > SRX_GROUPS_MAX) return fail(ctx, SRX_E_ARG, "%s: n_batches = %u is outside 1 .. %d", who, n_batches, SRX_GROUPS_MAX);
    const int paper = opts && opts->paper_order != 0;
    const uint64_t N = m->n_rows, G = m->n_cols, cells = (uint64_t)n_batches * G;
    const uint32_t top = (uint32_t)std::min<uint64_t>(n_top, at_least_one(G));
    hipStream_t st = ctx->stream;

    SRX_TRY(sv_refuse_negative(m, who));
    std::vector<uint32_t> one;
    if (!batch) {
        if (n_batches != 1) return fail(ctx, SRX_E_ARG, "%s: null batch labels with n_batches = %u", who, n_batches);
        one.assign(at_least_one(N), 0u);
    }
    uint32_t* d_labels;
    SRX_TRY(markers_host_labels(m, batch ? batch : one.data(), n_batches, who, &d_labels));

    srx_seurat_v3_info info;
    memset(&info, 0, sizeof info);
    StreamTimer t_mom(ctx, st), t_loess(ctx, st), t_clip(ctx, st), t_rank(ctx, st);

    // -- step 1
    SRX_TRY(t_mom.start());
    MkHolder hold;
    MkPlan plan;
    SRX_TRY(markers_moments(m, d_labels, n_batches, false, &hold.mk, &plan));
    const srx_markers* mk = hold.mk;
    uint64_t smallest = ~0ull;
    for (uint32_t b = 0; b < n_batches; ++b) {
        if (plan.sizes[b] < 2) return fail(ctx, SRX_E_ARG, "%s: batch %u has %llu cells; a variance needs 2", who, b, (unsigned long long)plan.sizes[b]);
        smallest = std::min(smallest, plan.sizes[b]);
    }
    info.n_cells = N;
    info.n_genes = G;
    info.n_batches = n_batches;
    info.sum_scale_log2 = mk->info.sum_scale_log2;
    info.sq_scale_log2 = mk->info.sq_scale_log2;
    info.max_abs = mk->info.max_abs;
    info.min_batch_cells = smallest;
    info.span = span;
    const double inv_sum = std::ldexp(1.0, -info.sum_scale_log2), inv_sq = std::ldexp(1.0, -info.sq_scale_log2);

    DevBlock blk{ctx};
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
    const size_t c8 = at_least_one(cells) * 8, c4 = at_least_one(cells) * 4, g8 = at_least_one(G) * 8, g4 = at_least_one(G) * 4;
    const size_t o_mean = carve(c8), o_var = carve(c8), o_lx = carve(c8), o_ly = carve(c8), o_key = carve(c8), o_xs = carve(c8),
                 o_ys = carve(c8), o_fit = carve(c8), o_rv = carve(c8), o_clip = carve(c8), o_Sc = carve(c8), o_Qc = carve(c8), o_cs = carve(c8),
                 o_cq = carve(c8), o_nv = carve(c8), o_rank = carve(c4), o_gene = carve(c4), o_m = carve((size_t)n_batches * 4),
                 o_means = carve(g8), o_vars = carve(g8), o_vn = carve(g8), o_med = carve(g8), o_fkey = carve(g8), o_nb = carve(g4),
                 o_frank = carve(g4), o_sel = carve((size_t)top * 8);
    SRX_TRY(sv_alloc(ctx, blk, off, who));
    char* base = (char*)blk.p;
    auto f64 = [&](size_t o) { return (double*)(base + o); };
    auto u32 = [&](size_t o) { return (uint32_t*)(base + o); };
    long long *d_Sc = (long long*)(base + o_Sc), *d_Qc = (long long*)(base + o_Qc);
    uint64_t* d_sel = (uint64_t*)(base + o_sel);
    SRX_HIP(ctx, hipMemsetAsync(blk.p, 0, off, st));
    hipLaunchKernelGGL(k_sv_stats, dim3(grid256(cells)), dim3(256), 0, st, (const long long*)mk->d_S, (const long long*)mk->d_Q,
                       (const uint64_t*)mk->d_sizes, n_batches, G, inv_sum, inv_sq, f64(o_mean), f64(o_var), f64(o_lx), f64(o_ly), f64(o_key),
                       u32(o_m));
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_mom.stop(&info.ms_moments));

    // -- step 2
    SRX_TRY(t_loess.start());
    if (G)
        SRX_TRY(sv_loess(ctx, f64(o_lx), f64(o_ly), f64(o_key), u32(o_m), n_batches, G, span, u32(o_rank), f64(o_xs), f64(o_ys), u32(o_gene),
                         f64(o_fit)));
    SRX_TRY(t_loess.stop(&info.ms_loess));

    // -- step 3
    SRX_TRY(t_clip.start());
    hipLaunchKernelGGL(k_sv_clip, dim3(grid256(cells)), dim3(256), 0, st, (const double*)f64(o_mean), (const double*)f64(o_fit),
                       (const uint64_t*)mk->d_sizes, n_batches, G, f64(o_rv), f64(o_clip));
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(markers_clipped_walk(m, plan, f64(o_clip), (unsigned long long*)d_Sc, (unsigned long long*)d_Qc));
    hipLaunchKernelGGL(k_sv_nv, dim3(grid256(cells)), dim3(256), 0, st, (const double*)f64(o_mean), (const double*)f64(o_rv),
                       (const long long*)d_Sc, (const long long*)d_Qc, (const uint64_t*)mk->d_sizes, n_batches, G, inv_sum, inv_sq, f64(o_cs),
                       f64(o_cq), f64(o_nv), u32(o_rank));
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_clip.stop(&info.ms_clip));

    // -- steps 4 and 5
    SRX_TRY(t_rank.start());
    for (uint32_t b = 0; b < n_batches; ++b) SRX_TRY(rank_keys_device(ctx, f64(o_nv) + (uint64_t)b * G, G, u32(o_rank) + (uint64_t)b * G));
    const uint64_t take = std::min<uint64_t>(n_top, G);
    if (G) {
        hipLaunchKernelGGL(k_sv_combine, dim3(grid256(G)), dim3(256), 0, st, (const uint32_t*)u32(o_rank), (const double*)f64(o_nv),
                           (const long long*)mk->d_totS, (const long long*)mk->d_totQ, n_batches, G, N, top, paper, inv_sum, inv_sq,
                           f64(o_means), f64(o_vars), f64(o_vn), f64(o_med), u32(o_nb), f64(o_fkey), u32(o_frank));
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(rank_keys_device(ctx, f64(o_fkey), G, u32(o_frank)));
        SRX_TRY(pick_top(ctx, u32(o_frank), G, take, d_sel));
    }
    SRX_TRY(t_rank.stop(&info.ms_rank));

    // everything comes to host buffers of this call first: nothing of the caller's is written before the last copy has succeeded
    struct Out { void* dst; size_t off; size_t bytes; std::vector<char> buf; };
    std::vector<Out> outs;
    auto want = [&](void* dst, size_t o, size_t bytes) { if (dst && bytes) outs.push_back(Out{dst, o, bytes, {}}); };
    want(idx_out, o_sel, take * 8);
    if (tables) {
        want(tables->means, o_means, G * 8); want(tables->variances, o_vars, G * 8); want(tables->variances_norm, o_vn, G * 8);
        want(tables->median, o_med, G * 8); want(tables->nbatches, o_nb, G * 4);
        want(tables->mean, o_mean, cells * 8); want(tables->var, o_var, cells * 8); want(tables->fitted, o_fit, cells * 8);
        want(tables->reg_var, o_rv, cells * 8); want(tables->clip, o_clip, cells * 8); want(tables->clip_sum, o_cs, cells * 8); want(tables->clip_sumsq, o_cq, cells * 8);
        want(tables->nv, o_nv, cells * 8); want(tables->rank, o_rank, cells * 4);
    }
    for (Out& o : outs) {
        o.buf.resize(o.bytes);
        SRX_TRY(d2h(ctx, o.buf.data(), base + o.off, o.bytes));
    }
    for (Out& o : outs) memcpy(o.dst, o.buf.data(), o.bytes);
    *n_out = take;
    if (info_out) *info_out = info;
    return SRX_OK;
}

}  // extern "C"
