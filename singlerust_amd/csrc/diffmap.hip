// diffmap.hip — diffusion maps and pseudotime of a symmetric weighted graph on the device: srx_diffmap (the connectivities of
// an srx_graph, read where they lie), srx_diffmap_csr (any symmetric CSR), srx_graph_diffmap_fetch,
// srx_graph_transitions_fetch, srx_dpt and srx_dpt_from.
//
// Definition (include/srx.h has it in full): the symmetric transition operator T of scanpy's compute_transitions, its
// n_comps algebraically largest eigenpairs, and DPT's distance from a root without branchings.
//
// Solver: a thick-restart Lanczos iteration with full reorthogonalisation (classical Gram-Schmidt applied twice) on a
// resident column-major basis V (leading dimension ld = n rounded up to 16, the padding rows stay zero).  alpha and beta
// stay on the device (DmCtl); the host reads them once per restart, solves the projected problem (an arrowhead plus a
// tridiagonal tail, at most 129 x 129) with a cyclic Jacobi of its own, and uploads the coefficients of the vectors it
// keeps.  A breakdown (beta <= 2^-40) sets DmCtl::stop on the device: every kernel queued behind it returns at once, the
// host sees the flag at the read it makes anyway and continues with a fresh hashed vector orthogonalised against the basis.
// A single-vector Krylov space holds one vector per eigenspace, so a repeated eigenvalue (one per component of a
// disconnected graph, the cosine pairs of a ring) is not found by the first run except through rounding.  Therefore the
// converged block is LOCKED (the leading columns of V, part of every Gram-Schmidt pass) and the same iteration runs in its
// complement from a fresh vector until the complement's largest Ritz pair has converged: above the smallest locked value
// it replaces that one and the check repeats, at or below it the block is complete.
//
// Nothing is added across workgroups with floating-point atomics: dot products leave one partial per (workgroup, column)
// in fixed slots and k_dm_reduce adds the slots in a fixed order, so the whole result is bit-identical from call to call.
//
// Kernels:
//   (srx_diffmap_csr: k_symcsr_check of symcsr.hip validates the input)
//   k_dm_rowsum        q_i or z_i: SRX_DIFFMAP_GROUP lanes per row, lane s adds the entries lo + s, lo + s + G, ..., butterfly
//   k_dm_kernel        K_ij = C_ij / (q_i q_j) and z_i in the same walk
//   k_dm_transitions   T_ij = K_ij / (sqrt(z_i) sqrt(z_j)), in place
//   k_dm_matvec        y = T x, row-owned as above; x is gathered (L2)
//   k_dm_hashvec       the start vector and every fresh vector
//   k_dm_dots          h = V_j^T w: a workgroup owns 1024 rows, its waves share the columns, 16-byte loads
//   k_dm_reduce        the slots of a column (or of the norm) added in a fixed order; also records alpha
//   k_dm_update        w -= V_j h, optionally leaving the partial sums of |w|^2
//   k_dm_append        beta = |w|, w /= beta (or the breakdown flag)
//   k_dm_ritz          V S for a chunk of 8 columns of S
//   k_dm_sign          the index of the component of largest magnitude (lowest index on ties) -> +-1
//   k_dm_emit          the row-major, sorted, signed block
//   k_dm_dpt, k_dm_dpt_scale   the distance from the root, its finite maximum (integer max of bit patterns), the quotient
// The file is built without -ffast-math and with FMA contraction off: every operation of the definition is rounded once.
// SRX_DIFFMAP_GROUP is a build-time constant (include/srx.h; -DSRX_DIFFMAP_GROUP=4|16|32 builds the alternatives that
// profiles/diffmap.md compares): there is no run-time switch.
#include "common.hpp"
#include "graph_handle.hpp"
#include "hash.hpp"
#include "scan.hpp"
#include "symcsr.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace srx {

constexpr int kDmGroup = SRX_DIFFMAP_GROUP;
constexpr int kDmRows = 1024;                // rows a workgroup of the tall-skinny kernels owns
constexpr int kDmMaxNcv = SRX_DIFFMAP_MAX_NCV, kDmMaxComps = SRX_DIFFMAP_MAX_COMPS;
constexpr int kDmMaxCols = kDmMaxNcv + kDmMaxComps + 1;
constexpr double kDmBreak = 0x1p-40;         // beta at or below this is a breakdown (|T| = 1)
constexpr unsigned long long kDmInfBits = 0x7FF0000000000000ull;
constexpr int kDmDummy = kDmMaxNcv + 2;      // the alpha / beta slot of steps nobody reads

struct DmCtl {
    unsigned long long stop;                 // 0, or 1 + the step whose beta was a breakdown
    unsigned long long dpt_max;              // bits of the largest finite distance
    double alpha[kDmMaxNcv + 3], beta[kDmMaxNcv + 3];
};

// ---- the operator ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_dm_rowsum(const uint64_t* __restrict__ ptr, const double* __restrict__ w, uint64_t n,
                                                   double* __restrict__ out) {
    constexpr int G = kDmGroup;
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    double acc = 0.0;
    if (row < n) {
        const uint64_t lo = ptr[row], hi = ptr[row + 1];
        for (uint64_t e = lo + sub; e < hi; e += G) acc += w[e];
    }
    acc = group_sum<G>(acc);
    if (row < n && sub == 0) out[row] = acc;
}

__global__ void __launch_bounds__(256) k_dm_kernel(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ ind,
                                                   const double* __restrict__ c, const double* __restrict__ q, uint64_t n,
                                                   double* __restrict__ kdat, double* __restrict__ z) {
    constexpr int G = kDmGroup;
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    double acc = 0.0;
    if (row < n) {
        const uint64_t lo = ptr[row], hi = ptr[row + 1];
        const double qi = q[row];
        for (uint64_t e = lo + sub; e < hi; e += G) {
            const double k = c[e] / (qi * q[ind[e]]);
            kdat[e] = k;
            acc += k;
        }
    }
    acc = group_sum<G>(acc);
    if (row < n && sub == 0) z[row] = acc;
}

__global__ void __launch_bounds__(256) k_dm_transitions(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ ind,
                                                        const double* __restrict__ z, uint64_t n, double* __restrict__ t) {
    constexpr int G = kDmGroup;
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    if (row >= n) return;
    const uint64_t lo = ptr[row], hi = ptr[row + 1];
    const double si = sqrt(z[row]);
    for (uint64_t e = lo + sub; e < hi; e += G) t[e] = t[e] / (si * sqrt(z[ind[e]]));
}

__global__ void __launch_bounds__(256) k_dm_matvec(SymCsr g, const double* __restrict__ x, double* __restrict__ y,
                                                   const DmCtl* __restrict__ ctl) {
    constexpr int G = kDmGroup;
    if (ctl->stop) return;
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    double acc = 0.0;
    if (row < g.n) {
        const uint64_t lo = g.ptr[row], hi = g.ptr[row + 1];
        for (uint64_t e = lo + sub; e < hi; e += G) acc += g.w[e] * x[g.ind[e]];
    }
    // every lane of the block is here: the butterfly reads all of them
    acc = group_sum<G>(acc);
    if (row < g.n && sub == 0) y[row] = acc;
}

// ---- the basis ---------------------------------------------------------------------------------------------------------
// v[i] = mix(seed + gold * (serial * n + i + 1)) as a number in [-0.5, 0.5); the padding rows are zeroed
__global__ void __launch_bounds__(256) k_dm_hashvec(double* __restrict__ v, uint64_t n, uint64_t ld, uint64_t seed, uint64_t serial,
                                                    const DmCtl* __restrict__ ctl) {
    if (ctl->stop) return;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ld) return;
    const uint64_t z = mix64(seed + kGold64 * (serial * n + i + 1));
    v[i] = i < n ? unit53(z) - 0.5 : 0.0;
}

// slots[block * stride + c] = sum over the block's rows of V[c * ld + i] * w[i], c < ncols.  Wave v of the block takes the
// columns v, v + 4, ...; lane l the rows base + 2 l + 128 t (t = 0..7), two at a time.
__global__ void __launch_bounds__(256) k_dm_dots(const double* __restrict__ V, const double* __restrict__ w, uint64_t ld, int ncols,
                                                 double* __restrict__ slots, int stride, const DmCtl* __restrict__ ctl) {
    if (ctl->stop) return;
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t base = (uint64_t)blockIdx.x * kDmRows + 2 * (uint64_t)lane;
    double2 wv[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint64_t r = base + 128 * (uint64_t)t;
        wv[t] = r < ld ? *reinterpret_cast<const double2*>(w + r) : make_double2(0.0, 0.0);
    }
    for (int c = wave; c < ncols; c += 4) {
        const double* col = V + (uint64_t)c * ld;
        double acc = 0.0;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint64_t r = base + 128 * (uint64_t)t;
            if (r < ld) {
                const double2 x = *reinterpret_cast<const double2*>(col + r);
                acc += x.x * wv[t].x;
                acc += x.y * wv[t].y;
            }
        }
        acc = wave_sum(acc);
        if (lane == 0) slots[(uint64_t)blockIdx.x * stride + c] = acc;
    }
}

// out[c] = the slots of column c added in a fixed order (block c of the grid).  alpha >= 0: the last column's coefficient
// is the step's alpha, set by the first Gram-Schmidt pass and added to by the second.
__global__ void __launch_bounds__(256) k_dm_reduce(const double* __restrict__ slots, unsigned nblk, int stride, double* __restrict__ out,
                                                   int alpha, int second, DmCtl* __restrict__ ctl) {
    __shared__ double s_wave[4];
    if (ctl->stop) return;
    const int c = blockIdx.x;
    double s = 0.0;
    for (unsigned b = threadIdx.x; b < nblk; b += 256) s += slots[(uint64_t)b * stride + c];
    s = block_sum<4>(s, s_wave);
    if (threadIdx.x == 0) {
        out[c] = s;
        if (alpha >= 0 && c == (int)gridDim.x - 1) ctl->alpha[alpha] = second ? ctl->alpha[alpha] + s : s;
    }
}

// w -= sum_c V[:, c] h[c] (c ascending); nslots: the block's sum of the new w[i]^2
__global__ void __launch_bounds__(256) k_dm_update(const double* __restrict__ V, double* __restrict__ w, uint64_t ld, int ncols,
                                                   const double* __restrict__ h, double* __restrict__ nslots, const DmCtl* __restrict__ ctl) {
    __shared__ double s_h[kDmMaxCols];
    __shared__ double s_wave[4];
    if (ctl->stop) return;
    for (int c = threadIdx.x; c < ncols; c += 256) s_h[c] = h[c];
    __syncthreads();
    double sq = 0.0;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint64_t r = (uint64_t)blockIdx.x * kDmRows + 512 * (uint64_t)half + 2 * (uint64_t)threadIdx.x;
        if (r < ld) {
            double2 acc = make_double2(0.0, 0.0);
            for (int c = 0; c < ncols; ++c) {
                const double2 x = *reinterpret_cast<const double2*>(V + (uint64_t)c * ld + r);
                acc.x += x.x * s_h[c];
                acc.y += x.y * s_h[c];
            }
            double2 v = *reinterpret_cast<double2*>(w + r);
            v.x -= acc.x;
            v.y -= acc.y;
            *reinterpret_cast<double2*>(w + r) = v;
            sq += v.x * v.x;
            sq += v.y * v.y;
        }
    }
    if (nslots) {
        sq = block_sum<4>(sq, s_wave);
        if (threadIdx.x == 0) nslots[blockIdx.x] = sq;
    }
}

// beta = sqrt(the norm slots added in a fixed order), the same bits in every block; w /= beta, or the breakdown flag
__global__ void __launch_bounds__(256) k_dm_append(double* __restrict__ w, uint64_t ld, const double* __restrict__ nslots, unsigned nblk,
                                                   int step, DmCtl* __restrict__ ctl) {
    __shared__ double s_wave[4];
    if (ctl->stop) return;
    double s = 0.0;
    for (unsigned b = threadIdx.x; b < nblk; b += 256) s += nslots[b];
    const double beta = sqrt(block_sum<4>(s, s_wave));
    if (!(beta > kDmBreak)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            ctl->beta[step] = 0.0;
            ctl->stop = (unsigned long long)step + 1;
        }
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) ctl->beta[step] = beta;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint64_t r = (uint64_t)blockIdx.x * kDmRows + 512 * (uint64_t)half + 2 * (uint64_t)threadIdx.x;
        if (r < ld) {
            double2 v = *reinterpret_cast<double2*>(w + r);
            v.x /= beta;
            v.y /= beta;
            *reinterpret_cast<double2*>(w + r) = v;
        }
    }
}

// Z[:, c0 + c] = sum_j V[:, j] S[j * ks + c0 + c] for c < 8 (blockIdx.y = c0 / 8), j ascending
__global__ void __launch_bounds__(256) k_dm_ritz(const double* __restrict__ V, uint64_t ld, int m, const double* __restrict__ S, int ks,
                                                 double* __restrict__ Z) {
    __shared__ double s_s[kDmMaxNcv * 8];
    const int c0 = blockIdx.y * 8, cw = min(8, ks - c0);
    for (int t = threadIdx.x; t < m * 8; t += 256) s_s[t] = (t & 7) < cw ? S[(uint64_t)(t >> 3) * ks + c0 + (t & 7)] : 0.0;
    __syncthreads();
    const uint64_t r = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (r >= ld) return;
    double2 acc[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[c] = make_double2(0.0, 0.0);
    for (int j = 0; j < m; ++j) {
        const double2 x = *reinterpret_cast<const double2*>(V + (uint64_t)j * ld + r);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c].x += x.x * s_s[j * 8 + c];
            acc[c].y += x.y * s_s[j * 8 + c];
        }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c)
        if (c < cw) *reinterpret_cast<double2*>(Z + (uint64_t)(c0 + c) * ld + r) = acc[c];
}

// sign[c] = +1 or -1 so that the component of largest magnitude of column c (lowest index on ties) becomes positive
__global__ void __launch_bounds__(256) k_dm_sign(const double* __restrict__ V, uint64_t n, uint64_t ld, double* __restrict__ sign) {
    __shared__ unsigned long long s_bits[256];
    __shared__ uint64_t s_idx[256];
    const double* col = V + (uint64_t)blockIdx.x * ld;
    unsigned long long best = 0;
    uint64_t at = ~0ull;
    for (uint64_t i = threadIdx.x; i < n; i += 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(col[i]));
        if (at == ~0ull || b > best) {
            best = b;
            at = i;
        }
    }
    s_bits[threadIdx.x] = best;
    s_idx[threadIdx.x] = at;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            const unsigned long long ob = s_bits[threadIdx.x + off];
            const uint64_t oi = s_idx[threadIdx.x + off];
            const uint64_t mi = s_idx[threadIdx.x];
            if (oi != ~0ull && (mi == ~0ull || ob > s_bits[threadIdx.x] || (ob == s_bits[threadIdx.x] && oi < mi))) {
                s_bits[threadIdx.x] = ob;
                s_idx[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) sign[blockIdx.x] = col[s_idx[0]] < 0.0 ? -1.0 : 1.0;
}

// out[i * m + l] = sign[perm[l]] * V[perm[l] * ld + i]
__global__ void __launch_bounds__(256) k_dm_emit(const double* __restrict__ V, uint64_t n, uint64_t ld, int m, const int* __restrict__ perm,
                                                 const double* __restrict__ sign, double* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * (uint64_t)m) return;
    const uint64_t i = t / m;
    const int c = perm[t % m];
    out[t] = sign[c] * V[(uint64_t)c * ld + i];
}

// ---- pseudotime --------------------------------------------------------------------------------------------------------
// d[i] = sqrt(sum_l (w[l] * (E[root, l] - E[i, l]))^2), l ascending; the largest finite d as bits into ctl->dpt_max
__global__ void __launch_bounds__(256) k_dm_dpt(const double* __restrict__ E, uint64_t n, int m, const double* __restrict__ w, uint64_t root,
                                                double* __restrict__ d, DmCtl* __restrict__ ctl) {
    __shared__ double s_w[kDmMaxComps], s_r[kDmMaxComps];
    __shared__ unsigned long long s_max[4];
    if (threadIdx.x < (unsigned)m) {
        s_w[threadIdx.x] = w[threadIdx.x];
        s_r[threadIdx.x] = E[root * m + threadIdx.x];
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long bits = 0;
    if (i < n) {
        double s = 0.0;
        for (int l = 0; l < m; ++l) {
            const double t = s_w[l] * (s_r[l] - E[i * m + l]);
            s = l ? s + t * t : t * t;
        }
        const double v = sqrt(s);
        d[i] = v;
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        bits = b < kDmInfBits ? b : 0;           // a NaN's bits lie above Inf's; v >= 0 or NaN
    }
    bits = block_max<4>(bits, s_max);
    if (threadIdx.x == 0 && bits) atomicMax(&ctl->dpt_max, bits);      // an integer max: the same whatever the order
}

__global__ void __launch_bounds__(256) k_dm_dpt_scale(double* __restrict__ d, uint64_t n, const DmCtl* __restrict__ ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double mx = __longlong_as_double((long long)ctl->dpt_max);
    d[i] = mx > 0.0 ? d[i] / mx : 0.0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct DmOpts {
    double tol;
    uint64_t seed;
    int n_comps, ncv, max_matvecs, density;
};

static int32_t dm_opts(srx_ctx* ctx, const srx_diffmap_opts* in, uint64_t n, DmOpts* out) {
    const srx_diffmap_opts o = in ? *in : srx_diffmap_opts{0.0, 0, 0, 0, 0, 1};
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "diffmap: rows are sharded; the solve needs the whole graph");
    if (o.n_comps < 0 || o.n_comps > kDmMaxComps) return fail(ctx, SRX_E_ARG, "diffmap: n_comps = %d outside 1..%d (0: 15)", o.n_comps, kDmMaxComps);
    if (!(o.tol >= 0.0)) return fail(ctx, SRX_E_ARG, "diffmap: tol must be >= 0 (0: 1e-10)");
    if (o.max_matvecs < 0) return fail(ctx, SRX_E_ARG, "diffmap: max_matvecs = %d is negative (0: 10000)", o.max_matvecs);
    if (n < 2) return fail(ctx, SRX_E_ARG, "diffmap: n = %llu; at least 2 vertices are needed", (unsigned long long)n);
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "diffmap: more than 2^32 - 2 vertices");
    int nc = o.n_comps ? o.n_comps : 15;
    if (o.ncv && (o.ncv < nc + 2 || o.ncv > kDmMaxNcv))
        return fail(ctx, SRX_E_ARG, "diffmap: ncv = %d outside n_comps + 2 = %d .. %d (0: max(2 n_comps + 1, 20))", o.ncv, nc + 2, kDmMaxNcv);
    if ((uint64_t)nc > n - 1) nc = (int)(n - 1);
    int ncv = o.ncv ? o.ncv : std::max(2 * nc + 1, 20);
    if ((uint64_t)ncv > n) ncv = (int)n;
    out->tol = o.tol > 0.0 ? o.tol : 1e-10;
    out->seed = o.seed;
    out->n_comps = nc;
    out->ncv = ncv;
    out->max_matvecs = o.max_matvecs ? o.max_matvecs : 10000;
    out->density = o.density_normalize != 0;
    return SRX_OK;
}

// Eigen-decomposition of the symmetric m x m matrix A (row-major, destroyed) by cyclic Jacobi: theta descending (equal values
// in the order of their columns), S[j * m + i] = component j of eigenvector i.  Plain loops in a fixed order: deterministic.
static void dm_jacobi(int m, std::vector<double>& A, std::vector<double>& theta, std::vector<double>& S) {
    std::vector<double> U((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) U[(size_t)i * m + i] = 1.0;
    for (int sweep = 0; sweep < 100; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < m - 1; ++p)
            for (int q = p + 1; q < m; ++q) {
                const double apq = A[(size_t)p * m + q];
                if (apq == 0.0) continue;
                const double app = A[(size_t)p * m + p], aqq = A[(size_t)q * m + q];
                if (fabs(apq) <= 0x1p-70 * std::max(fabs(app), fabs(aqq)) || fabs(apq) < 1e-300) {
                    A[(size_t)p * m + q] = A[(size_t)q * m + p] = 0.0;
                    continue;
                }
                rotated = true;
                const double th = (aqq - app) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < m; ++k) {          // columns p, q
                    const double akp = A[(size_t)k * m + p], akq = A[(size_t)k * m + q];
                    A[(size_t)k * m + p] = c * akp - s * akq;
                    A[(size_t)k * m + q] = s * akp + c * akq;
                }
                for (int k = 0; k < m; ++k) {          // rows p, q
                    const double apk = A[(size_t)p * m + k], aqk = A[(size_t)q * m + k];
                    A[(size_t)p * m + k] = c * apk - s * aqk;
                    A[(size_t)q * m + k] = s * apk + c * aqk;
                }
                A[(size_t)p * m + q] = A[(size_t)q * m + p] = 0.0;
                for (int k = 0; k < m; ++k) {
                    const double ukp = U[(size_t)k * m + p], ukq = U[(size_t)k * m + q];
                    U[(size_t)k * m + p] = c * ukp - s * ukq;
                    U[(size_t)k * m + q] = s * ukp + c * ukq;
                }
            }
        if (!rotated) break;
    }
    std::vector<int> order(m);
    for (int i = 0; i < m; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return A[(size_t)a * m + a] > A[(size_t)b * m + b]; });
    theta.resize(m);
    S.assign((size_t)m * m, 0.0);
    for (int i = 0; i < m; ++i) {
        theta[i] = A[(size_t)order[i] * m + order[i]];
        for (int j = 0; j < m; ++j) S[(size_t)j * m + i] = U[(size_t)j * m + order[i]];
    }
}

// One solve: the buffers, the counters and the launches every phase shares.
struct DmRun {
    srx_ctx* ctx;
    hipStream_t st;
    SymCsr g;
    uint64_t n, ld, seed, serial = 0;
    unsigned nblk;                     // workgroups of the tall-skinny kernels = norm slots
    int cap;                           // columns of V = the stride of the dot slots
    int ncv;
    double *V, *Z, *slots, *nslots, *h, *S;
    DmCtl* ctl;
    double tol_in;
    int max_matvecs, matvecs = 0, restarts = 0, breakdowns = 0;
    double last_est = INFINITY;
    std::vector<double> al, be;

    double* col(int c) const { return V + (uint64_t)c * ld; }

    void matvec(const double* x, double* y) const {
        hipLaunchKernelGGL(k_dm_matvec, dim3(grid256(n * (uint64_t)kDmGroup)), dim3(256), 0, st, g, x, y, ctl);
    }
    // w (a column of n rows, leading dimension ld) made orthogonal to the columns [0, ncols) of B by classical Gram-Schmidt,
    // twice; the partial sums of |w|^2 are left in nslots.  alpha >= 0: the coefficient of the last column is that step's alpha.
    void orth(const double* B, int ncols, double* w, int alpha) const {
        for (int pass = 0; pass < 2 && ncols; ++pass) {
            hipLaunchKernelGGL(k_dm_dots, dim3(nblk), dim3(256), 0, st, B, w, ld, ncols, slots, cap, ctl);
            hipLaunchKernelGGL(k_dm_reduce, dim3(ncols), dim3(256), 0, st, slots, nblk, cap, h, alpha, pass, ctl);
            hipLaunchKernelGGL(k_dm_update, dim3(nblk), dim3(256), 0, st, B, w, ld, ncols, h, pass ? nslots : nullptr, ctl);
        }
        if (!ncols) hipLaunchKernelGGL(k_dm_update, dim3(nblk), dim3(256), 0, st, B, w, ld, 0, h, nslots, ctl);
    }
    void append(double* w, int step) const { hipLaunchKernelGGL(k_dm_append, dim3(nblk), dim3(256), 0, st, w, ld, nslots, nblk, step, ctl); }
    // column c <- a fresh hashed unit vector orthogonal to the columns before it
    void fresh(int c) {
        hipLaunchKernelGGL(k_dm_hashvec, dim3(grid256(ld)), dim3(256), 0, st, col(c), n, ld, seed, serial++, ctl);
        orth(V, c, col(c), -1);
        append(col(c), kDmDummy);
    }
    int32_t read_ctl(DmCtl* hc) const {
        SRX_HIP(ctx, hipGetLastError());
        return d2h(ctx, hc, ctl, sizeof(DmCtl));
    }
    // Z[:, 0..ks) = V[:, L .. L + m) S[:, 0..ks) (S: m x m from dm_jacobi), then copied over the columns L .. L + ks of V
    int32_t ritz(int L, int m, const std::vector<double>& Sm, int ks) {
        std::vector<double> pack((size_t)m * ks);
        for (int j = 0; j < m; ++j)
            for (int c = 0; c < ks; ++c) pack[(size_t)j * ks + c] = Sm[(size_t)j * m + c];
        SRX_TRY(h2d(ctx, S, pack.data(), pack.size() * 8));
        hipLaunchKernelGGL(k_dm_ritz, dim3(grid256(ld / 2), (ks + 7) / 8), dim3(256), 0, st, col(L), ld, m, S, ks, Z);
        SRX_HIP(ctx, hipMemcpyAsync(col(L), Z, (size_t)ks * ld * 8, hipMemcpyDeviceToDevice, st));
        return SRX_OK;
    }

    // The `want` largest eigenpairs of T in the complement of the columns [0, L) of V by thick-restart Lanczos; on SRX_OK
    // the vectors are the columns L .. L + want of V and theta holds the Ritz values, descending.
    int32_t solve(int L, int want, std::vector<double>* theta_out) {
        const int m = (int)std::min<uint64_t>((uint64_t)ncv, n - (uint64_t)L);
        al.assign(m + 1, 0.0);
        be.assign(m + 1, 0.0);
        std::vector<double> theta_k, s_k, theta, Sm;
        DmCtl hc;
        fresh(L);
        int k = 0;
        for (;;) {
            int j = k;
            bool exhausted = false;
            while (j < m) {
                const int left = max_matvecs - matvecs;
                if (left <= 0) break;
                const int jend = std::min(m, j + left);
                for (int s = j; s < jend; ++s) {
                    matvec(col(L + s), col(L + s + 1));
                    orth(V, L + s + 1, col(L + s + 1), s);
                    append(col(L + s + 1), s);
                }
                SRX_TRY(read_ctl(&hc));
                if (hc.stop && (hc.stop - 1 < (unsigned long long)j || hc.stop - 1 >= (unsigned long long)jend))
                    return fail(ctx, SRX_E_NOCONV, "diffmap: a fresh vector had no component outside the basis");
                const int done = hc.stop ? (int)hc.stop - 1 : jend - 1;      // the last step whose alpha and beta are valid
                for (int s = j; s <= done; ++s) {
                    al[s] = hc.alpha[s];
                    be[s] = hc.beta[s];
                }
                matvecs += done - j + 1;
                j = done + 1;
                if (hc.stop) {
                    ++breakdowns;
                    SRX_HIP(ctx, hipMemsetAsync(&ctl->stop, 0, 8, st));
                    if ((uint64_t)L + (uint64_t)j >= n) {                    // the basis spans the whole complement
                        exhausted = true;
                        break;
                    }
                    fresh(L + j);
                }
            }
            const int me = j;                                                // columns of the projected problem
            if (me <= k || me < want) {                                      // the budget ended before anything new
                return fail(ctx, SRX_E_NOCONV, "diffmap: max_matvecs = %d reached after %d restarts", max_matvecs, restarts);
            }
            std::vector<double> H((size_t)me * me, 0.0);
            for (int i = 0; i < k; ++i) {
                H[(size_t)i * me + i] = theta_k[i];
                if (k < me) H[(size_t)i * me + k] = H[(size_t)k * me + i] = s_k[i];
            }
            for (int s = k; s < me; ++s) {
                H[(size_t)s * me + s] = al[s];
                if (s + 1 < me) H[(size_t)s * me + s + 1] = H[(size_t)(s + 1) * me + s] = be[s];
            }
            const double beta_last = exhausted ? 0.0 : be[me - 1];
            dm_jacobi(me, H, theta, Sm);
            double est = 0.0;
            for (int i = 0; i < want; ++i) est = std::max(est, fabs(beta_last * Sm[(size_t)(me - 1) * me + i]));
            last_est = est;
            if (est <= tol_in) {
                SRX_TRY(ritz(L, me, Sm, want));
                theta_out->assign(theta.begin(), theta.begin() + want);
                return SRX_OK;
            }
            if (matvecs >= max_matvecs)
                return fail(ctx, SRX_E_NOCONV, "diffmap: max_matvecs = %d reached after %d restarts (residual estimate %.3e, tol %.3e)",
                            max_matvecs, restarts, est, tol_in);
            // thick restart: keep k Ritz vectors and the residual direction
            k = std::max(1, std::min(want + (me - want) / 2, me - 1));
            theta_k.assign(theta.begin(), theta.begin() + k);
            s_k.resize(k);
            for (int i = 0; i < k; ++i) s_k[i] = beta_last * Sm[(size_t)(me - 1) * me + i];
            SRX_TRY(ritz(L, me, Sm, k));
            SRX_HIP(ctx, hipMemcpyAsync(col(L + k), col(L + me), ld * 8, hipMemcpyDeviceToDevice, st));
            ++restarts;
        }
    }
};

struct DmResult {
    double* d_evecs = nullptr;         // n x n_comps row-major, in scratch
    std::vector<double> evals;
};

// T from the graph c (C, or the copy of it): the two normalisation passes.  t: nnz doubles; q, z: n doubles of scratch.
static void dm_transitions(hipStream_t st, const SymCsr& c, bool density, double* q, double* z, double* t) {
    const unsigned blocks = grid256(c.n * (uint64_t)kDmGroup);
    if (density) {
        hipLaunchKernelGGL(k_dm_rowsum, dim3(blocks), dim3(256), 0, st, c.ptr, c.w, c.n, q);
        hipLaunchKernelGGL(k_dm_kernel, dim3(blocks), dim3(256), 0, st, c.ptr, c.ind, c.w, q, c.n, t, z);
    } else {
        (void)hipMemcpyAsync(t, c.w, c.nnz * 8, hipMemcpyDeviceToDevice, st);
        hipLaunchKernelGGL(k_dm_rowsum, dim3(blocks), dim3(256), 0, st, c.ptr, t, c.n, z);
    }
    hipLaunchKernelGGL(k_dm_transitions, dim3(blocks), dim3(256), 0, st, c.ptr, c.ind, z, c.n, t);
}

// The whole solve on a T that lies on the device.  SRX_E_NOCONV leaves info's counters filled.
static int32_t dm_run(srx_ctx* ctx, const SymCsr& g, const DmOpts& o, DmResult* res, srx_diffmap_info* info) {
    hipStream_t st = ctx->stream;
    const uint64_t n = g.n;
    const int nc = o.n_comps;
    DmRun r;
    r.ctx = ctx;
    r.st = st;
    r.g = g;
    r.n = n;
    r.ld = (n + 15) & ~15ull;
    r.seed = o.seed;
    r.nblk = (unsigned)((r.ld + kDmRows - 1) / kDmRows);
    r.cap = nc + o.ncv + 1;
    r.ncv = o.ncv;
    r.tol_in = o.tol / (2.0 + sqrt((double)nc));
    r.max_matvecs = o.max_matvecs;
    double *d_small, *d_out;
    int* d_perm;
    SRX_TRY(scratch(ctx, "dm_V", (size_t)r.cap * r.ld * 8, (void**)&r.V));
    SRX_TRY(scratch(ctx, "dm_Z", (size_t)o.ncv * r.ld * 8, (void**)&r.Z));
    SRX_TRY(scratch(ctx, "dm_slots", (size_t)r.nblk * (r.cap + 1) * 8, (void**)&r.slots));
    SRX_TRY(scratch(ctx, "dm_S", (size_t)kDmMaxNcv * kDmMaxNcv * 8, (void**)&r.S));
    // h (cap), lambda (64), res2 (64), sign (64), gram (64 x 64)
    SRX_TRY(scratch(ctx, "dm_small", (size_t)(kDmMaxCols + 3 * kDmMaxComps + kDmMaxComps * kDmMaxComps) * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "dm_perm", kDmMaxComps * 4, (void**)&d_perm));
    SRX_TRY(scratch(ctx, "dm_ctl", sizeof(DmCtl), (void**)&r.ctl));
    SRX_TRY(scratch(ctx, "dm_out", (size_t)n * nc * 8, (void**)&d_out));
    r.nslots = r.slots + (size_t)r.nblk * r.cap;
    r.h = d_small;
    double *d_lam = d_small + kDmMaxCols, *d_res2 = d_lam + kDmMaxComps, *d_sign = d_res2 + kDmMaxComps, *d_gram = d_sign + kDmMaxComps;

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(r.ctl, 0, sizeof(DmCtl), st));
    // only the padding rows of V need zeros: every column is written (rows < n by k_dm_matvec, all ld rows by the others)
    // before it is read, and Z is written whole by k_dm_ritz
    if (r.ld > n) SRX_HIP(ctx, hipMemset2DAsync(r.V + n, r.ld * 8, 0, (r.ld - n) * 8, (size_t)r.cap, st));

    auto finish_info = [&](double max_res, double max_ortho) -> int32_t {
        SRX_TRY(timer.stop(&info->ms));
        info->n = n;
        info->nnz = g.nnz;
        info->n_comps = (uint32_t)nc;
        info->ncv = (uint32_t)o.ncv;
        info->matvecs = (uint32_t)r.matvecs;
        info->restarts = (uint32_t)r.restarts;
        info->breakdowns = (uint32_t)r.breakdowns;
        info->max_residual = max_res;
        info->max_ortho = max_ortho;
        return SRX_OK;
    };

    // phase 1: the block; phase 2: the complement's largest pair, until it does not displace a member of the block
    std::vector<double> lam, top;
    int32_t rc = r.solve(0, nc, &lam);
    while (rc == SRX_OK) {
        rc = r.solve(nc, 1, &top);
        if (rc != SRX_OK) break;
        const int low = (int)(std::min_element(lam.begin(), lam.end()) - lam.begin());
        if (!(top[0] > lam[low] + o.tol)) break;
        SRX_HIP(ctx, hipMemcpyAsync(r.col(low), r.col(nc), r.ld * 8, hipMemcpyDeviceToDevice, st));
        lam[low] = top[0];
    }
    if (rc != SRX_OK) {
        const std::string msg = ctx->err;
        SRX_TRY(finish_info(r.last_est, 0.0));
        return rc == SRX_E_NOCONV ? fail(ctx, rc, "%s", msg.c_str()) : rc;
    }

    // the block re-orthonormalised once, column by column
    for (int l = 0; l < nc; ++l) {
        r.orth(r.V, l, r.col(l), -1);
        r.append(r.col(l), kDmDummy);
    }
    // lambda_l = v_l . T v_l, the residual T v_l - lambda_l v_l (in column nc), and V^T V
    for (int l = 0; l < nc; ++l) {
        double* tv = r.col(nc);
        r.matvec(r.col(l), tv);
        hipLaunchKernelGGL(k_dm_dots, dim3(r.nblk), dim3(256), 0, st, r.col(l), tv, r.ld, 1, r.slots, r.cap, r.ctl);
        hipLaunchKernelGGL(k_dm_reduce, dim3(1), dim3(256), 0, st, r.slots, r.nblk, r.cap, d_lam + l, -1, 0, r.ctl);
        hipLaunchKernelGGL(k_dm_update, dim3(r.nblk), dim3(256), 0, st, r.col(l), tv, r.ld, 1, d_lam + l, r.nslots, r.ctl);
        hipLaunchKernelGGL(k_dm_reduce, dim3(1), dim3(256), 0, st, r.nslots, r.nblk, 1, d_res2 + l, -1, 0, r.ctl);
        hipLaunchKernelGGL(k_dm_dots, dim3(r.nblk), dim3(256), 0, st, r.V, r.col(l), r.ld, l + 1, r.slots, r.cap, r.ctl);
        hipLaunchKernelGGL(k_dm_reduce, dim3(l + 1), dim3(256), 0, st, r.slots, r.nblk, r.cap, d_gram + (size_t)l * kDmMaxComps, -1, 0, r.ctl);
    }
    hipLaunchKernelGGL(k_dm_sign, dim3(nc), dim3(256), 0, st, r.V, n, r.ld, d_sign);
    SRX_HIP(ctx, hipGetLastError());
    std::vector<double> small((size_t)3 * kDmMaxComps + (size_t)kDmMaxComps * kDmMaxComps);
    SRX_TRY(d2h(ctx, small.data(), d_lam, small.size() * 8));
    DmCtl hc;
    SRX_TRY(r.read_ctl(&hc));
    if (hc.stop) {
        SRX_TRY(finish_info(r.last_est, 0.0));
        return fail(ctx, SRX_E_NOCONV, "diffmap: a vector of the block vanished in the final orthonormalisation");
    }
    double max_res = 0.0, max_ortho = 0.0;
    for (int l = 0; l < nc; ++l) {
        const double rr = sqrt(small[kDmMaxComps + l]);
        max_res = rr > max_res || rr != rr ? rr : max_res;
        for (int c = 0; c <= l; ++c) {
            const double d = fabs(small[(size_t)3 * kDmMaxComps + (size_t)l * kDmMaxComps + c] - (c == l ? 1.0 : 0.0));
            max_ortho = d > max_ortho || d != d ? d : max_ortho;
        }
    }
    std::vector<int> perm(nc);
    for (int l = 0; l < nc; ++l) perm[l] = l;
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return small[a] > small[b]; });
    res->evals.resize(nc);
    for (int l = 0; l < nc; ++l) res->evals[l] = small[perm[l]];
    SRX_TRY(h2d(ctx, d_perm, perm.data(), (size_t)nc * 4));
    hipLaunchKernelGGL(k_dm_emit, dim3(grid256(n * (uint64_t)nc)), dim3(256), 0, st, r.V, n, r.ld, nc, d_perm, d_sign, d_out);
    SRX_HIP(ctx, hipGetLastError());
    res->d_evecs = d_out;
    SRX_TRY(finish_info(max_res, max_ortho));
    if (!(max_res <= o.tol))
        return fail(ctx, SRX_E_NOCONV, "diffmap: the residual %.3e of the returned block exceeds tol = %.3e", max_res, o.tol);
    return SRX_OK;
}

// pseudotime from eigenpairs on the device (E: n x m row-major); the result is written to the host
static int32_t dm_dpt(srx_ctx* ctx, const double* d_E, const double* evals, uint64_t n, int m, uint64_t root, double cap, double* out) {
    hipStream_t st = ctx->stream;
    double w[kDmMaxComps];
    for (int l = 0; l < m; ++l) w[l] = evals[l] < cap ? evals[l] / (1.0 - evals[l]) : 1.0;
    double *d_w, *d_d;
    DmCtl* ctl;
    SRX_TRY(scratch(ctx, "dm_dpt_w", kDmMaxComps * 8, (void**)&d_w));
    SRX_TRY(scratch(ctx, "dm_dpt_d", n * 8, (void**)&d_d));
    SRX_TRY(scratch(ctx, "dm_ctl", sizeof(DmCtl), (void**)&ctl));
    SRX_TRY(h2d(ctx, d_w, w, (size_t)m * 8));
    SRX_HIP(ctx, hipMemsetAsync(&ctl->dpt_max, 0, 8, st));
    hipLaunchKernelGGL(k_dm_dpt, dim3(grid256(n)), dim3(256), 0, st, d_E, n, m, d_w, root, d_d, ctl);
    hipLaunchKernelGGL(k_dm_dpt_scale, dim3(grid256(n)), dim3(256), 0, st, d_d, n, ctl);
    SRX_HIP(ctx, hipGetLastError());
    return d2h(ctx, out, d_d, n * 8);
}

static int32_t dm_check_dpt(srx_ctx* ctx, uint64_t n, uint64_t root, double* cap) {
    if (root >= n) return fail(ctx, SRX_E_ARG, "dpt: root = %llu is not below n = %llu", (unsigned long long)root, (unsigned long long)n);
    if (*cap == 0.0) *cap = 0.9994;
    if (!(*cap > 0.0 && *cap <= 1.0)) return fail(ctx, SRX_E_ARG, "dpt: cap must lie in (0, 1] (0: 0.9994)");
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_diffmap(srx_graph* g, const srx_diffmap_opts* opts, double* evals_out, double* evecs_out, srx_diffmap_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    DmOpts o;
    SRX_TRY(dm_opts(ctx, opts, g->n, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("diffmap");
    const SymCsr c = connectivities(g);
    const uint64_t n = c.n, nnz = c.nnz;
    double *d_q, *d_z;
    SRX_TRY(scratch(ctx, "dm_q", n * 8, (void**)&d_q));
    SRX_TRY(scratch(ctx, "dm_z", n * 8, (void**)&d_z));
    g->dm_valid = g->dm_t_valid = false;
    if (!g->d_dm_t) SRX_HIP(ctx, hipMalloc((void**)&g->d_dm_t, at_least_one(nnz) * 8));
    dm_transitions(ctx->stream, c, o.density, d_q, d_z, g->d_dm_t);
    SRX_HIP(ctx, hipGetLastError());
    g->dm_t_valid = true;
    srx_diffmap_info li{};
    DmResult res;
    const int32_t rc = dm_run(ctx, SymCsr{c.ptr, c.ind, g->d_dm_t, n, nnz}, o, &res, &li);
    if (rc != SRX_OK) {
        if (rc == SRX_E_NOCONV && info) *info = li;
        return rc;
    }
    const size_t bytes = (size_t)n * o.n_comps * 8;
    SRX_TRY(keep_on_handle(ctx, &g->d_dm_evecs, g->dm_n_comps != (uint32_t)o.n_comps, res.d_evecs, bytes));
    if (evecs_out) SRX_TRY(d2h(ctx, evecs_out, g->d_dm_evecs, bytes));
    else SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    g->dm_evals = res.evals;
    g->dm_n_comps = (uint32_t)o.n_comps;
    g->dm_valid = true;
    if (evals_out) memcpy(evals_out, res.evals.data(), (size_t)o.n_comps * 8);
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_diffmap_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                        const srx_diffmap_opts* opts, double* evals_out, double* evecs_out, srx_diffmap_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    DmOpts o;
    SRX_TRY(dm_opts(ctx, opts, n, &o));
    if (!indptr) return fail(ctx, SRX_E_ARG, "diffmap: null indptr");
    for (uint64_t i = 0; i < n; ++i)
        if (indptr[i + 1] == indptr[i])
            return fail(ctx, SRX_E_ARG, "diffmap: row %llu has no entries (its density q is 0)", (unsigned long long)i);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("diffmap");
    SymCsr in;
    SRX_TRY(symcsr_to_device(ctx, "diffmap", indptr, indices, weights, n, &in));
    double *d_q, *d_z, *d_t;
    SRX_TRY(scratch(ctx, "dm_q", n * 8, (void**)&d_q));
    SRX_TRY(scratch(ctx, "dm_z", n * 8, (void**)&d_z));
    SRX_TRY(scratch(ctx, "dm_t", at_least_one(in.nnz) * 8, (void**)&d_t));
    dm_transitions(ctx->stream, in, o.density, d_q, d_z, d_t);
    SRX_HIP(ctx, hipGetLastError());
    srx_diffmap_info li{};
    DmResult res;
    const int32_t rc = dm_run(ctx, SymCsr{in.ptr, in.ind, d_t, n, in.nnz}, o, &res, &li);
    if (rc != SRX_OK) {
        if (rc == SRX_E_NOCONV && info) *info = li;
        return rc;
    }
    if (evecs_out) SRX_TRY(d2h(ctx, evecs_out, res.d_evecs, (size_t)n * o.n_comps * 8));
    if (evals_out) memcpy(evals_out, res.evals.data(), (size_t)o.n_comps * 8);
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_graph_diffmap_fetch(srx_graph* g, double* evals, double* evecs, uint32_t* n_comps_out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->dm_valid) return fail(ctx, SRX_E_ARG, "srx_graph_diffmap_fetch: no srx_diffmap has succeeded on this graph");
    if (n_comps_out) *n_comps_out = g->dm_n_comps;
    if (evals) memcpy(evals, g->dm_evals.data(), (size_t)g->dm_n_comps * 8);
    if (!evecs) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, evecs, g->d_dm_evecs, (size_t)g->n * g->dm_n_comps * 8);
}

int32_t srx_graph_transitions_fetch(srx_graph* g, double* data) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->dm_t_valid) return fail(ctx, SRX_E_ARG, "srx_graph_transitions_fetch: no srx_diffmap has run on this graph");
    if (!data || !g->info.nnz_connectivities) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, data, g->d_dm_t, (size_t)g->info.nnz_connectivities * 8);
}

int32_t srx_dpt(srx_graph* g, uint64_t root, double cap, double* pseudotime_out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "dpt: rows are sharded; the pseudotime needs the whole graph");
    if (!g->dm_valid) return fail(ctx, SRX_E_ARG, "dpt: no srx_diffmap has succeeded on this graph");
    SRX_TRY(dm_check_dpt(ctx, g->n, root, &cap));
    if (!pseudotime_out) return fail(ctx, SRX_E_ARG, "dpt: null output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return dm_dpt(ctx, g->d_dm_evecs, g->dm_evals.data(), g->n, (int)g->dm_n_comps, root, cap, pseudotime_out);
}

int32_t srx_dpt_from(srx_ctx* ctx, const double* evals, const double* evecs, uint64_t n, uint32_t m, uint64_t root, double cap,
                     double* pseudotime_out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "dpt: rows are sharded; the pseudotime needs the whole graph");
    if (m < 1 || m > (uint32_t)kDmMaxComps) return fail(ctx, SRX_E_ARG, "dpt: m = %u outside 1..%d", m, kDmMaxComps);
    SRX_TRY(dm_check_dpt(ctx, n, root, &cap));
    if (!evals || !evecs || !pseudotime_out) return fail(ctx, SRX_E_ARG, "dpt: null eigenvalues, eigenvectors or output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    double* d_E;
    SRX_TRY(scratch(ctx, "dm_dpt_E", (size_t)n * m * 8, (void**)&d_E));
    SRX_TRY(h2d(ctx, d_E, evecs, (size_t)n * m * 8));
    return dm_dpt(ctx, d_E, evals, n, (int)m, root, cap, pseudotime_out);
}

}  // extern "C"
