// umap.hip — the UMAP layout of a symmetric weighted graph on the device: srx_umap (the connectivities of an srx_graph, read
// where they lie), srx_umap_csr (any symmetric CSR), srx_graph_embedding_fetch and the host-only curve fit srx_umap_fit_ab.
//
// Definition (include/srx.h has it in full): umap-learn's optimize_layout_euclidean restated as a synchronous, vertex-owned
// iteration.  Epoch t reads Y^{t-1} only and writes Y^t: positions are double-buffered, one launch per epoch, back to back on
// the context's stream with no host synchronisation between them.  Which entries act in an epoch is a stateless function of
// (t, w_e / w_max); the negative samples are a hash of (seed, t, e, p).  Nothing is added across vertices, so there is no
// floating-point atomic anywhere: the result is the same bits from call to call.
//
// Kernels:
//   (srx_umap_csr: k_symcsr_check of symcsr.hip validates the input)
//   k_umap_wmax          w_max by integer max of the bit patterns (positive doubles order as their bits do)
//   k_umap_active        the entries with floor(E w_e / w_max) > 0
//   k_umap_init_random   the hashed start
//   k_umap_absmax        max |x| over the first dim columns of a row-major array, as bits: the PCA start's scale and the
//                        NaN / Inf check of every start (a NaN's bits lie above Inf's)
//   k_umap_init_pca      scores[:, :dim] * (10 / max)
//   k_umap_epoch<DIM>    SRX_UMAP_GROUP lanes per vertex: lane s walks the entries lo + s, lo + s + G, ... of the row, skips on
//                        its own to the next one the schedule samples, gathers y_j and the R hashed targets, sums its terms in
//                        f64 in that order; group_sum (scan.hpp) adds the lanes; lane 0 writes y_i once.  Rows longer than G
//                        loop.  The counters are per-block integer sums added with integer atomics.
// The two terms of an epoch (um_term) and the small block are in umap_internal.hpp, shared with the transform of ingest.hip.
// x^y is ocml's pow(double, double); the file is built without -ffast-math and with FMA contraction off, so that every
// operation of the definition is rounded once, as numpy rounds it.
#include "common.hpp"
#include "graph_handle.hpp"
#include "hash.hpp"
#include "pca_internal.hpp"
#include "scan.hpp"
#include "symcsr.hpp"

#include <cmath>

#include "umap_internal.hpp"         // UmParams, um_load, um_term, the small block; FMA contraction is off from here on

namespace srx {

constexpr unsigned long long kUmInfBits = 0x7FF0000000000000ull;

__global__ void __launch_bounds__(256) k_umap_wmax(const double* __restrict__ w, uint64_t nnz, unsigned long long* __restrict__ small) {
    __shared__ unsigned long long s_wave[4];
    unsigned long long m = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(w[e]);
        m = b > m ? b : m;
    }
    m = block_max<4>(m, s_wave);
    if (threadIdx.x == 0 && m) atomicMax(&small[UM_WMAX], m);
}

__global__ void __launch_bounds__(256) k_umap_active(const double* __restrict__ w, uint64_t nnz, double epochs,
                                                     unsigned long long* __restrict__ small) {
    __shared__ unsigned long long s_wave[4];
    const double wmax = __longlong_as_double((long long)small[UM_WMAX]);
    unsigned long long c = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * 256)
        c += floor(epochs * (w[e] / wmax)) > 0.0;
    c = block_sum<4>(c, s_wave);
    if (threadIdx.x == 0 && c) atomicAdd(&small[UM_ACTIVE], c);
}

__global__ void __launch_bounds__(256) k_umap_init_random(double* __restrict__ y, uint64_t count, uint64_t seed) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= count) return;
    y[c] = -10.0 + 20.0 * unit53(mix64(seed + kGold64 * (c + 1)));
}

// x: rows x ld row-major; the first dim columns
__global__ void __launch_bounds__(256) k_umap_absmax(const double* __restrict__ x, uint64_t rows, int dim, uint64_t ld,
                                                     unsigned long long* __restrict__ dst) {
    __shared__ unsigned long long s_wave[4];
    unsigned long long m = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < rows * (uint64_t)dim; c += (uint64_t)gridDim.x * 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(x[(c / dim) * ld + (c % dim)]));
        m = b > m ? b : m;
    }
    m = block_max<4>(m, s_wave);
    if (threadIdx.x == 0 && m) atomicMax(dst, m);
}

__global__ void __launch_bounds__(256) k_umap_init_pca(const double* __restrict__ scores, uint64_t rows, int dim, uint64_t ld,
                                                       const unsigned long long* __restrict__ small, double* __restrict__ y) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= rows * (uint64_t)dim) return;
    const double s = 10.0 / __longlong_as_double((long long)small[UM_PCAMAX]);
    y[c] = scores[(c / dim) * ld + (c % dim)] * s;
}

template <int DIM>
__global__ void __launch_bounds__(256) k_umap_epoch(SymCsr g, const double* __restrict__ yin, double* __restrict__ yout, uint32_t t,
                                                    double alpha, UmParams p, unsigned long long* __restrict__ small) {
    constexpr int G = kUmGroup;
    __shared__ unsigned long long s_wave[4];
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = row < g.n;
    double acc[DIM], yi[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = yi[c] = 0.0;
    unsigned long long n_samp = 0, n_skip = 0;
    if (live) {
        um_load<DIM>(yin, row, yi);
        const double wmax = __longlong_as_double((long long)small[UM_WMAX]);
        const double tf = (double)t, tp = (double)(t - 1);
        const double att = -2.0 * p.a * p.b, rep = 2.0 * p.gamma * p.b, alpha2 = 2.0 * alpha;
        const uint64_t lo = g.ptr[row], hi = g.ptr[row + 1];
        for (uint64_t e = lo + sub;; e += G) {
            // on to this lane's next sampled entry: the lanes of a wave skip independently, so none waits through another's misses
            for (; e < hi; e += G) {
                const double r = g.w[e] / wmax;
                if (floor(tf * r) > floor(tp * r)) break;
            }
            if (e >= hi) break;
            ++n_samp;
            // s = -1: the attraction along the entry; s = 0 .. rate - 1: its negative samples
            const uint32_t j = g.ind[e];
            const uint64_t first = ((uint64_t)t * g.nnz + e) * (uint64_t)p.rate + 1;
            for (int s = -1; s < p.rate; ++s) {
                uint64_t o = j;
                if (s >= 0) {
                    const uint64_t z = mix64(p.seed + kGold64 * (first + (uint64_t)s));
                    o = ((z >> 32) * g.n) >> 32;                    // < n < 2^32
                    if (o == row) {
                        ++n_skip;
                        continue;
                    }
                }
                um_term<DIM>(yi, yin, o, p, s < 0, s < 0 ? att : rep, s < 0 ? alpha2 : alpha, acc);
            }
        }
    }
    // every lane of the block is here: the butterflies read all of them
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = group_sum<G>(acc[c]);
    if (live && sub == 0) {
        if constexpr (DIM == 2) {
            reinterpret_cast<double2*>(yout)[row] = make_double2(yi[0] + acc[0], yi[1] + acc[1]);
        } else {
#pragma unroll
            for (int c = 0; c < DIM; ++c) yout[row * DIM + c] = yi[c] + acc[c];
        }
    }
    // the counters: the block's sums in thread 0, one integer atomic each; the barrier frees s_wave for the second sum
    n_samp = block_sum_thread0<4>(n_samp, s_wave);
    if (n_samp) atomicAdd(&small[UM_SAMPLES], n_samp);
    __syncthreads();
    n_skip = block_sum_thread0<4>(n_skip, s_wave);
    if (n_skip) atomicAdd(&small[UM_SKIPPED], n_skip);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static unsigned um_stride_grid(uint64_t items) {              // grid-stride kernels: at most 8 blocks per CU of the 256
    const uint64_t b = (at_least_one(items) + 255) / 256;
    return (unsigned)(b < 2048 ? b : 2048);
}

// the curve of the residuals: y(x) on the grid
static double um_target(double x, double spread, double min_dist) { return x < min_dist ? 1.0 : exp(-(x - min_dist) / spread); }

static int32_t um_fit_ab(double spread, double min_dist, double* a_out, double* b_out) {
    constexpr int N = 300;
    double xs[N], ys[N], lx[N];
    for (int i = 0; i < N; ++i) {
        xs[i] = 3.0 * spread * (double)i / (double)(N - 1);
        ys[i] = um_target(xs[i], spread, min_dist);
        lx[i] = i ? log(xs[i]) : 0.0;
    }
    // residuals r_i = f_i - y_i with f = 1 / (1 + a x^(2b)); df/da = -x^(2b) f^2, df/db = -2 a x^(2b) ln(x) f^2 (both 0 at x = 0)
    auto eval = [&](double a, double b, long double* jtj, long double* jtr) {
        long double rss = 0.0L, s00 = 0.0L, s01 = 0.0L, s11 = 0.0L, g0 = 0.0L, g1 = 0.0L;
        for (int i = 0; i < N; ++i) {
            const double xp = i ? pow(xs[i], 2.0 * b) : 0.0;
            const double f = 1.0 / (1.0 + a * xp);
            const double r = f - ys[i];
            rss += (long double)r * r;
            if (jtj) {
                const double da = -xp * f * f, db = -2.0 * a * xp * lx[i] * f * f;
                s00 += (long double)da * da;
                s01 += (long double)da * db;
                s11 += (long double)db * db;
                g0 += (long double)da * r;
                g1 += (long double)db * r;
            }
        }
        if (jtj) {
            jtj[0] = s00;
            jtj[1] = s01;
            jtj[2] = s11;
            jtr[0] = g0;
            jtr[1] = g1;
        }
        return rss;
    };
    double a = 1.0, b = 1.0, lambda = 1e-3;
    long double jtj[3], jtr[2];
    long double rss = eval(a, b, jtj, jtr);
    for (int it = 0, quiet = 0; it < 500 && quiet < 3; ++it) {
        // (J^T J + lambda diag(J^T J)) step = -J^T r
        const long double m00 = jtj[0] * (1.0L + lambda), m11 = jtj[2] * (1.0L + lambda), m01 = jtj[1];
        const long double det = m00 * m11 - m01 * m01;
        if (!(det > 0.0L)) {
            lambda *= 10.0;
            if (lambda > 1e12) break;
            continue;
        }
        const double sa = (double)((-jtr[0] * m11 + jtr[1] * m01) / det), sb = (double)((-jtr[1] * m00 + jtr[0] * m01) / det);
        const double na = a + sa, nb = b + sb;
        const long double nrss = (na > 0.0 && nb > 0.0) ? eval(na, nb, nullptr, nullptr) : rss + 1.0L;
        if (nrss <= rss) {
            const bool tiny = fabs(sa) <= 1e-15 * fabs(a) && fabs(sb) <= 1e-15 * fabs(b);
            quiet = (tiny || nrss == rss) ? quiet + 1 : 0;
            a = na;
            b = nb;
            rss = eval(a, b, jtj, jtr);
            lambda = lambda > 1e-12 ? lambda * 0.1 : lambda;
        } else {
            lambda *= 10.0;
            if (lambda > 1e12) break;
        }
    }
    *a_out = a;
    *b_out = b;
    return SRX_OK;
}

static int32_t um_check_curve(srx_ctx* ctx, double spread, double min_dist) {
    if (!is_pos_finite(spread)) return fail(ctx, SRX_E_ARG, "umap: spread must be a positive finite number");
    if (!(min_dist >= 0.0 && min_dist <= spread)) return fail(ctx, SRX_E_ARG, "umap: min_dist must lie in 0 .. spread");
    return SRX_OK;
}

void umap_wmax_active(srx_ctx* ctx, const double* d_w, uint64_t nnz, double epochs, unsigned long long* d_small) {
    hipLaunchKernelGGL(k_umap_wmax, dim3(um_stride_grid(nnz)), dim3(256), 0, ctx->stream, d_w, nnz, d_small);
    hipLaunchKernelGGL(k_umap_active, dim3(um_stride_grid(nnz)), dim3(256), 0, ctx->stream, d_w, nnz, epochs, d_small);
}

int32_t umap_fit_curve(srx_ctx* ctx, double spread, double min_dist, double* a, double* b) {
    SRX_TRY(um_check_curve(ctx, spread, min_dist));
    return um_fit_ab(spread, min_dist, a, b);
}

struct UmOpts {
    srx_umap_opts o;
    uint32_t epochs, run;
};

static int32_t um_opts(srx_ctx* ctx, const srx_umap_opts* in, uint64_t n, UmOpts* out) {
    srx_umap_opts o = in ? *in : srx_umap_opts{0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 0, 0, 0, 2, 5, SRX_UMAP_INIT_PCA, 0};
    if (o.n_components != 2 && o.n_components != 3) return fail(ctx, SRX_E_ARG, "umap: n_components = %d is not 2 or 3", o.n_components);
    if (o.negative_sample_rate < 0 || o.negative_sample_rate > 32)
        return fail(ctx, SRX_E_ARG, "umap: negative_sample_rate = %d outside 0..32", o.negative_sample_rate);
    SRX_TRY(um_check_curve(ctx, o.spread, o.min_dist));
    if (o.a == 0.0 && o.b == 0.0) SRX_TRY(um_fit_ab(o.spread, o.min_dist, &o.a, &o.b));
    if (!is_pos_finite(o.a) || !is_pos_finite(o.b)) return fail(ctx, SRX_E_ARG, "umap: a and b must be positive finite numbers (or both 0: fitted)");
    if (!is_pos_finite(o.gamma)) return fail(ctx, SRX_E_ARG, "umap: gamma must be a positive finite number");
    if (!is_pos_finite(o.alpha0)) return fail(ctx, SRX_E_ARG, "umap: alpha0 must be a positive finite number");
    if (o.n_epochs < 0 || o.n_epochs > SRX_UMAP_MAX_EPOCHS)
        return fail(ctx, SRX_E_ARG, "umap: n_epochs = %d outside 0..%d", o.n_epochs, SRX_UMAP_MAX_EPOCHS);
    if (o.n_epochs == 0) o.n_epochs = n <= 10000 ? 500 : 200;
    if (o.stop_after < 0 || o.stop_after > o.n_epochs)
        return fail(ctx, SRX_E_ARG, "umap: stop_after = %d outside 0..n_epochs = %d", o.stop_after, o.n_epochs);
    if (o.init != SRX_UMAP_INIT_GIVEN && o.init != SRX_UMAP_INIT_RANDOM && o.init != SRX_UMAP_INIT_PCA)
        return fail(ctx, SRX_E_ARG, "umap: unknown start %d", o.init);
    out->o = o;
    out->epochs = (uint32_t)o.n_epochs;
    out->run = (uint32_t)(o.stop_after ? o.stop_after : o.n_epochs);
    return SRX_OK;
}

// the start's arguments, checked before anything is queued
static int32_t um_check_start(srx_ctx* ctx, const UmOpts& u, srx_mat* m, const double* init, uint64_t n) {
    if (u.o.init == SRX_UMAP_INIT_GIVEN) {
        if (!init && n) return fail(ctx, SRX_E_ARG, "umap: SRX_UMAP_INIT_GIVEN needs start positions");
    } else if (u.o.init == SRX_UMAP_INIT_PCA) {
        if (!m) return fail(ctx, SRX_E_ARG, "umap: the PCA start needs the matrix handle that holds the scores");
        if (m->ctx != ctx) return fail(ctx, SRX_E_ARG, "umap: the matrix and the graph belong to different contexts");
        if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "umap: no PCA result on this matrix");
        if ((int)m->pca.n_pc < u.o.n_components)
            return fail(ctx, SRX_E_ARG, "umap: the PCA result has %u components, the start needs %d", m->pca.n_pc, u.o.n_components);
        const uint64_t cells = m->csc ? m->n_cols : m->n_rows;
        if (cells != n) return fail(ctx, SRX_E_ARG, "umap: the matrix has %llu cells, the graph %llu", (unsigned long long)cells, (unsigned long long)n);
    }
    return SRX_OK;
}

// The run (n >= 1).  The result is left in *d_result (one of the two scratch position buffers).
static int32_t umap_run(srx_ctx* ctx, const SymCsr& g, const UmOpts& u, srx_mat* m, const double* init, double** d_result,
                        srx_umap_info* info) {
    hipStream_t st = ctx->stream;
    const int dim = u.o.n_components;
    const uint64_t count = g.n * (uint64_t)dim;
    double *d_y0, *d_y1;
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "umap_y0", count * 8, (void**)&d_y0));
    SRX_TRY(scratch(ctx, "umap_y1", count * 8, (void**)&d_y1));
    SRX_TRY(scratch(ctx, "umap_small", UM_WORDS * 8, (void**)&d_small));
    if (u.o.init == SRX_UMAP_INIT_GIVEN) SRX_TRY(h2d(ctx, d_y0, init, count * 8));

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, UM_WORDS * 8, st));
    if (u.o.init == SRX_UMAP_INIT_RANDOM) {
        hipLaunchKernelGGL(k_umap_init_random, dim3(grid256(count)), dim3(256), 0, st, d_y0, count, u.o.seed);
    } else if (u.o.init == SRX_UMAP_INIT_PCA) {
        const uint64_t ld = (uint64_t)scores_ld((int)m->pca.n_pc);
        hipLaunchKernelGGL(k_umap_absmax, dim3(um_stride_grid(count)), dim3(256), 0, st, m->pca.d_scores, g.n, dim, ld, d_small + UM_PCAMAX);
        hipLaunchKernelGGL(k_umap_init_pca, dim3(grid256(count)), dim3(256), 0, st, m->pca.d_scores, g.n, dim, ld, d_small, d_y0);
    }
    hipLaunchKernelGGL(k_umap_absmax, dim3(um_stride_grid(count)), dim3(256), 0, st, d_y0, g.n, dim, (uint64_t)dim, d_small + UM_ABSMAX);
    if (g.nnz) umap_wmax_active(ctx, g.w, g.nnz, (double)u.epochs, d_small);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t h[UM_WORDS];
    SRX_TRY(d2h(ctx, h, d_small, sizeof h));
    if (h[UM_ABSMAX] >= kUmInfBits) {
        if (u.o.init == SRX_UMAP_INIT_PCA && (h[UM_PCAMAX] == 0 || h[UM_PCAMAX] >= kUmInfBits))
            return fail(ctx, SRX_E_ARG, "umap: the PCA start is not usable (the scores are all zero, or hold a NaN or Inf)");
        return fail(ctx, SRX_E_ARG, "umap: the start positions hold a NaN or Inf");
    }
    double* cur = d_y0;
    double* nxt = d_y1;
    uint32_t ran = 0;
    if (g.nnz) {
        const UmParams p{u.o.a, u.o.b, u.o.gamma, u.o.seed, u.o.negative_sample_rate};
        const unsigned blocks = grid256(g.n * (uint64_t)kUmGroup);
        for (uint32_t t = 1; t <= u.run; ++t) {
            const double alpha = u.o.alpha0 * (1.0 - (double)(t - 1) / (double)u.epochs);
            if (dim == 2) hipLaunchKernelGGL(k_umap_epoch<2>, dim3(blocks), dim3(256), 0, st, g, cur, nxt, t, alpha, p, d_small);
            else hipLaunchKernelGGL(k_umap_epoch<3>, dim3(blocks), dim3(256), 0, st, g, cur, nxt, t, alpha, p, d_small);
            std::swap(cur, nxt);
        }
        ran = u.run;
        SRX_HIP(ctx, hipGetLastError());
    }
    SRX_TRY(timer.stop(&info->ms));
    SRX_TRY(d2h(ctx, h, d_small, sizeof h));
    info->n = g.n;
    info->nnz = g.nnz;
    info->entries_active = h[UM_ACTIVE];
    info->samples = h[UM_SAMPLES];
    info->negatives_skipped = h[UM_SKIPPED];
    info->negatives = h[UM_SAMPLES] * (uint64_t)u.o.negative_sample_rate - h[UM_SKIPPED];
    info->epochs_run = ran;
    memcpy(&info->w_max, &h[UM_WMAX], 8);
    *d_result = cur;
    return SRX_OK;
}

static void um_info_start(srx_umap_info* li, const UmOpts& u, uint64_t n) {
    *li = srx_umap_info{};
    li->n = n;
    li->n_epochs = u.epochs;
    li->dim = (uint32_t)u.o.n_components;
    li->a = u.o.a;
    li->b = u.o.b;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_umap(srx_graph* g, srx_mat* m, const srx_umap_opts* opts, const double* init, double* embedding_out, srx_umap_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "umap: rows are sharded; the layout needs the whole graph");
    UmOpts u;
    SRX_TRY(um_opts(ctx, opts, g->n, &u));
    SRX_TRY(um_check_start(ctx, u, m, init, g->n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_umap_info li;
    um_info_start(&li, u, g->n);
    const uint32_t dim = (uint32_t)u.o.n_components;
    if (g->n) {
        Range rg("umap");
        double* d_res = nullptr;
        SRX_TRY(umap_run(ctx, connectivities(g), u, m, init, &d_res, &li));
        const size_t bytes = (size_t)g->n * dim * 8;
        g->embed_valid = false;
        SRX_TRY(keep_on_handle(ctx, &g->d_embed, g->embed_dim != dim, d_res, bytes));
        if (embedding_out) SRX_TRY(d2h(ctx, embedding_out, g->d_embed, bytes));
    }
    g->embed_dim = dim;
    g->embed_valid = true;
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_umap_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                     const srx_umap_opts* opts, const double* init, double* embedding_out, srx_umap_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "umap: rows are sharded; the layout needs the whole graph");
    UmOpts u;
    SRX_TRY(um_opts(ctx, opts, n, &u));
    if (u.o.init == SRX_UMAP_INIT_PCA) return fail(ctx, SRX_E_ARG, "umap: the PCA start needs a matrix handle; srx_umap_csr has none");
    SRX_TRY(um_check_start(ctx, u, nullptr, init, n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_umap_info li;
    um_info_start(&li, u, n);
    if (n == 0) {
        if (info) *info = li;
        return SRX_OK;
    }
    Range rg("umap");
    SymCsr in;
    SRX_TRY(symcsr_to_device(ctx, "umap", indptr, indices, weights, n, &in));
    double* d_res = nullptr;
    SRX_TRY(umap_run(ctx, in, u, nullptr, init, &d_res, &li));
    if (embedding_out) SRX_TRY(d2h(ctx, embedding_out, d_res, (size_t)n * u.o.n_components * 8));
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_graph_embedding_fetch(srx_graph* g, double* out, uint32_t* dim_out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->embed_valid) return fail(ctx, SRX_E_ARG, "srx_graph_embedding_fetch: no srx_umap has run on this graph");
    if (dim_out) *dim_out = g->embed_dim;
    if (!g->n || !out) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, out, g->d_embed, (size_t)g->n * g->embed_dim * 8);
}

int32_t srx_umap_fit_ab(double spread, double min_dist, double* a, double* b) {
    if (!a || !b) return fail(nullptr, SRX_E_ARG, "umap: null output");
    SRX_TRY(um_check_curve(nullptr, spread, min_dist));
    return um_fit_ab(spread, min_dist, a, b);
}

}  // extern "C"
