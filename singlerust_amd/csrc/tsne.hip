// tsne.hip — t-SNE in two dimensions on the device: the perplexity affinities of a k-NN list (srx_tsne_affinities_knn /
// _graph), the forces at a given layout (srx_tsne_forces) and the layout itself (srx_tsne_run), on the srx_tsne handle.
//
// Definition (include/srx.h has it in full).  Row i of the list gets p_{j|i} = exp(-beta_i (D_j - m_i)) / sum with beta_i the
// root of the row's entropy at log(perplexity); P = (p + p^T) / (2 n) on the union pattern, which graph.hip builds
// (pair_union_csr: the same kernels that build the connectivities).  An iteration reads Y^{t-1} only: the repulsion is a walk
// over a uniform pyramid of integer cell sums, the attraction a sum over the row of P, and the vertex's owner applies gains,
// momentum and the step.  Nothing floating-point is added with an atomic, every order of summation is fixed by the cells of
// the points, so the result is the same bits from call to call.
//
// Kernels:
//   k_tsne_rows         one wave per row (lane p holds entry p): the list's checks, the row in column order, m, c, the root of
//                       the entropy by bracketing and bisection (every sum a butterfly), p and beta
//   (k_graph_reverse .. k_graph_merge of graph.hip: the union pattern and P)
//   k_tsne_init_random, k_tsne_absmax, k_tsne_init_pca     the starts and their NaN / Inf check
//   k_tsne_bounds       min and max per coordinate as integer maxima of order-preserving keys
//   k_tsne_quant        side, lo, the quantised coordinates, the finest cell of every point; counts and u64 coordinate sums
//                       into the finest level with integer atomics
//   k_tsne_up           one wave per 64 consecutive cells (a 8 x 8 block in Morton order): up to three levels upward by
//                       integer butterflies
//   k_tsne_cells        (count, SX, SY) -> (m, com) of every cell of every level
//   scan_exclusive      (scan.hip) the first point of every finest cell
//   k_tsne_scatter      the points to their cell through an atomic cursor, in arbitrary order
//   k_tsne_rank         every point finds its place among its cell's members by counting the smaller indices: the order is
//                       (cell, index) whichever atomic won; the positions are copied into that order
//   k_tsne_walk         one point per lane in that order, so that a wave's lanes walk nearly the same cells; stackless
//                       (level, code) walk, the top kLdsLevels levels of the pyramid staged in LDS; rep, z, the workgroup's z
//   k_tsne_sum          the workgroup sums (Z, KL) added by one workgroup in a fixed order
//   k_tsne_step         SRX_TSNE_GROUP lanes per vertex: the attraction over the row of P, then gains, velocity, position
//   k_tsne_kl           the same walk over P for sum_e P_e ((log P_e - log q_e) + log Z)
// The file is built without -ffast-math and with FMA contraction off: every operation of the definition is rounded once.
#include "common.hpp"
#include "graph_handle.hpp"
#include "hash.hpp"
#include "pca_internal.hpp"
#include "pyramid.hpp"
#include "scan.hpp"

#include <cmath>

#pragma clang fp contract(off)

struct srx_tsne {
    srx_ctx* ctx = nullptr;
    uint64_t n = 0;
    uint32_t k = 0;
    // one allocation, sized once nnz is known: P (indptr, indices, data), beta
    void* d_block = nullptr;
    uint64_t* d_ptr = nullptr;
    uint32_t* d_ind = nullptr;
    double *d_dat = nullptr, *d_beta = nullptr;
    srx_tsne_info info{};
    // the embedding of the last srx_tsne_run: n x 2 f64
    double* d_embed = nullptr;
    bool embed_valid = false;
};

namespace srx {

constexpr int kTsGroup = SRX_TSNE_GROUP;
constexpr int kTsMaxLevels = SRX_TSNE_MAX_LEVELS;
constexpr int kLdsLevels = 5;                              // levels 1..5: 1364 cells x 24 B = 32 KiB, four workgroups a CU
constexpr int kLdsCells = ((1 << (2 * (kLdsLevels + 1))) - 4) / 3;
// the root is accepted at |H - log u| <= 9e-10: the header promises 1e-9 to a reader who evaluates H with another exp and log
constexpr double kTsRootTol = 9e-10;
constexpr unsigned long long kTsInfBits = 0x7FF0000000000000ull;
// the small block (8-byte words) behind the bounds of pyramid.hpp; the first TS_ZEROED are cleared before every pyramid
enum { TS_ACC = TS_BOUNDS_WORDS, TS_EXACT, TS_PAIRS, TS_ZEROED, TS_SIDE = TS_ZEROED, TS_LO0, TS_LO1, TS_Z,
       TS_KL, TS_ABSMAX, TS_PCAMAX, TS_WORDS = 16 };

// ---- affinities ------------------------------------------------------------------------------------------------------------------
// the entropy of the lane's row at beta: x = D - m (0 on the lanes behind the row), every lane holds the same bits
__device__ __forceinline__ double ts_entropy(bool act, double x, double beta, double* e_out, double* s_out) {
    const double e = act ? exp(-(beta * x)) : 0.0;
    const double S = wave_sum(e);
    const double W = wave_sum(x * e);
    *e_out = e;
    *s_out = S;
    return log(S) + beta * W / S;
}

__global__ void __launch_bounds__(256) k_tsne_rows(const uint32_t* __restrict__ idx_in, const double* __restrict__ dist_in, uint64_t n,
                                                   int k, double u, uint32_t* __restrict__ dind, double* __restrict__ p_out,
                                                   double* __restrict__ beta_out, unsigned long long* __restrict__ ctr,
                                                   int* __restrict__ flag) {
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
    rank = rank < kWave ? rank : kWave - 1;
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
    const double D = cd * cd;
    const double dmin = wave_min(act ? D : inf);
    const bool tie = act && D == dmin;
    const int c = __builtin_popcountll(__builtin_amdgcn_ballot_w64(tie));
    const double x = act ? D - dmin : 0.0;
    const double logu = log(u);
    const bool has_root = (double)c < u;
    double p = tie ? 1.0 / (double)c : 0.0, beta = inf;
    if (has_root) {
        // H falls from log k > log u (beta -> 0) to log c < log u (beta -> inf): bracket by factors of two from 1, then halve
        double ev, S;
        double lo = 1.0, hi = 1.0;
        double H = ts_entropy(act, x, 1.0, &ev, &S);
        beta = 1.0;
        if (!(fabs(H - logu) <= kTsRootTol)) {
            if (H > logu) {
                for (int it = 0; it < 2200; ++it) {
                    hi = lo * 2.0;
                    if (!(hi <= kDblMax)) {
                        hi = kDblMax;
                        break;
                    }
                    if (ts_entropy(act, x, hi, &ev, &S) <= logu) break;
                    lo = hi;
                }
            } else {
                for (int it = 0; it < 2200; ++it) {
                    lo = hi * 0.5;
                    if (lo == 0.0 || ts_entropy(act, x, lo, &ev, &S) > logu) break;
                    hi = lo;
                }
            }
            beta = hi;
            for (int it = 0; it < 128; ++it) {
                const double mid = lo + 0.5 * (hi - lo);
                if (!(mid > lo && mid < hi)) break;
                H = ts_entropy(act, x, mid, &ev, &S);
                beta = mid;
                if (fabs(H - logu) <= kTsRootTol) break;
                if (H > logu) lo = mid;
                else hi = mid;
            }
        }
        ts_entropy(act, x, beta, &ev, &S);
        p = ev / S;
    }
    if (act) {
        dind[e] = ci;
        p_out[e] = p;
    }
    if (lane == 0) {
        beta_out[row] = beta;
        if (!has_root) atomicAdd(&ctr[(size_t)(row & (kCtrSlots - 1)) * kCtrN + kCtrNoRoot], 1ull);
    }
}

// ---- starts ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsne_init_random(double* __restrict__ y, uint64_t count, uint64_t seed) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= count) return;
    y[c] = (unit53(mix64(seed + kGold64 * (c + 1))) - 0.5) * 2e-4;
}

// max |x| over the first two columns of rows x ld, as bits (a NaN's bits lie above Inf's)
__global__ void __launch_bounds__(256) k_tsne_absmax(const double* __restrict__ x, uint64_t rows, uint64_t ld,
                                                     unsigned long long* __restrict__ dst) {
    __shared__ unsigned long long s_wave[4];
    unsigned long long m = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x; c < rows * 2; c += (uint64_t)gridDim.x * 256) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(x[(c >> 1) * ld + (c & 1)]));
        m = b > m ? b : m;
    }
    m = block_max<4>(m, s_wave);
    if (threadIdx.x == 0 && m) atomicMax(dst, m);
}

__global__ void __launch_bounds__(256) k_tsne_init_pca(const double* __restrict__ scores, uint64_t rows, uint64_t ld,
                                                       const unsigned long long* __restrict__ small, double* __restrict__ y) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= rows * 2) return;
    const double s = 1e-4 / __longlong_as_double((long long)small[TS_PCAMAX]);
    y[c] = scores[(c >> 1) * ld + (c & 1)] * s;
}

// ---- the pyramid -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_tsne_bounds(const double* __restrict__ y, uint64_t n, unsigned long long* __restrict__ small) {
    __shared__ unsigned long long s_wave[4];
    unsigned long long k[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const double2 p = ts_load(y, i);
        const unsigned long long a = order_key(p.x), b = order_key(p.y);
        k[0] = a > k[0] ? a : k[0];
        k[1] = ~a > k[1] ? ~a : k[1];
        k[2] = b > k[2] ? b : k[2];
        k[3] = ~b > k[3] ? ~b : k[3];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const unsigned long long m = block_max<4>(k[c], s_wave);
        if (threadIdx.x == 0 && m) atomicMax(&small[TS_MAX0 + c], m);
    }
}

__global__ void __launch_bounds__(256) k_tsne_quant(const double* __restrict__ y, uint64_t n, int L, unsigned long long* __restrict__ small,
                                                    unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ sx,
                                                    unsigned long long* __restrict__ sy, uint32_t* __restrict__ code_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const TsGeom g = ts_geom(small);
    if (i == 0) {
        small[TS_SIDE] = (unsigned long long)__double_as_longlong(g.side);
        small[TS_LO0] = (unsigned long long)__double_as_longlong(g.lo0);
        small[TS_LO1] = (unsigned long long)__double_as_longlong(g.lo1);
    }
    if (i >= n) return;
    const double2 p = ts_load(y, i);
    const uint32_t u0 = ts_quant(p.x, g.lo0, g.side), u1 = ts_quant(p.y, g.lo1, g.side);
    const uint32_t code = spread_bits(u0 >> (32 - L)) | (spread_bits(u1 >> (32 - L)) << 1);
    code_out[i] = code;
    const size_t c = (size_t)level_off(L) + code;
    atomicAdd(&cnt[c], 1ull);
    atomicAdd(&sx[c], (unsigned long long)u0);
    atomicAdd(&sy[c], (unsigned long long)u1);
}

// levels src - 1 .. src - nlev from level src: the children of a cell are four consecutive codes
__global__ void __launch_bounds__(256) k_tsne_up(unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ sx,
                                                 unsigned long long* __restrict__ sy, int src, int nlev) {
    const uint64_t first = global_wave_id() * kWave;
    const uint64_t cells = 1ull << (2 * src);
    if (first >= cells) return;                      // wave-uniform
    const int lane = lane_id();
    const uint64_t code = first + lane;
    const bool valid = code < cells;
    const size_t at = (size_t)level_off(src) + code;
    unsigned long long c = valid ? cnt[at] : 0ull, x = valid ? sx[at] : 0ull, y = valid ? sy[at] : 0ull;
    for (int s = 1; s <= nlev; ++s) {
        for (int h = 2 * s - 2; h < 2 * s; ++h) {
            c += __shfl_xor(c, 1 << h, kWave);
            x += __shfl_xor(x, 1 << h, kWave);
            y += __shfl_xor(y, 1 << h, kWave);
        }
        if (valid && (lane & ((1 << (2 * s)) - 1)) == 0) {
            const size_t to = (size_t)level_off(src - s) + (code >> (2 * s));
            cnt[to] = c;
            sx[to] = x;
            sy[to] = y;
        }
    }
}

__global__ void __launch_bounds__(256) k_tsne_cells(const unsigned long long* __restrict__ cnt, const unsigned long long* __restrict__ sx,
                                                    const unsigned long long* __restrict__ sy, uint32_t total,
                                                    const unsigned long long* __restrict__ small, double* __restrict__ cx,
                                                    double* __restrict__ cy, double* __restrict__ cm) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= total) return;
    const unsigned long long m = cnt[c];
    cm[c] = (double)m;
    if (!m) return;
    const double unit = __longlong_as_double((long long)small[TS_SIDE]) * 0x1p-32;
    cx[c] = __longlong_as_double((long long)small[TS_LO0]) + ((double)sx[c] / (double)m) * unit;
    cy[c] = __longlong_as_double((long long)small[TS_LO1]) + ((double)sy[c] / (double)m) * unit;
}

__global__ void __launch_bounds__(256) k_tsne_scatter(const uint32_t* __restrict__ code, uint64_t n, const int64_t* __restrict__ start,
                                                      uint32_t* __restrict__ cursor, uint32_t* __restrict__ tmp) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = code[i];
    tmp[start[c] + (int64_t)atomicAdd(&cursor[c], 1u)] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_tsne_rank(const uint32_t* __restrict__ code, uint64_t n, const int64_t* __restrict__ start,
                                                   const uint32_t* __restrict__ tmp, const double* __restrict__ y,
                                                   uint32_t* __restrict__ order, double* __restrict__ ys) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = code[i];
    const int64_t lo = start[c], hi = start[c + 1];
    int64_t r = 0;
    for (int64_t q = lo; q < hi; ++q) r += tmp[q] < (uint32_t)i;       // the members are distinct: the ranks are a permutation
    order[lo + r] = (uint32_t)i;
    reinterpret_cast<double2*>(ys)[lo + r] = ts_load(y, i);           // the positions in that order: the walk reads them in a row
}

__global__ void __launch_bounds__(256) k_tsne_walk(const double* __restrict__ ys, const uint32_t* __restrict__ order, uint64_t n, int L,
                                                   double theta2, const double* __restrict__ cx, const double* __restrict__ cy,
                                                   const double* __restrict__ cm, const int64_t* __restrict__ start,
                                                   unsigned long long* __restrict__ small, double* __restrict__ rep,
                                                   double* __restrict__ z, double* __restrict__ zpart) {
    __shared__ double s_cx[kLdsCells], s_cy[kLdsCells], s_cm[kLdsCells];
    __shared__ double s_wave[4];
    __shared__ unsigned long long s_ctr[4];
    const int Ls = L < kLdsLevels ? L : kLdsLevels;
    const int staged = (int)level_off(Ls + 1);
    for (int t = threadIdx.x; t < staged; t += 256) {
        const double m = cm[t];
        s_cm[t] = m;
        s_cx[t] = m > 0.0 ? cx[t] : 0.0;
        s_cy[t] = m > 0.0 ? cy[t] : 0.0;
    }
    __syncthreads();
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < n;
    unsigned long long n_acc = 0, n_exact = 0, n_pairs = 0;
    double r0 = 0.0, r1 = 0.0, zi = 0.0;
    if (live) {
        const double2 yi = ts_load(ys, t);
        const double side = __longlong_as_double((long long)small[TS_SIDE]);
        int l = 1;
        uint32_t code = 0;
        while (l > 0) {
            const uint32_t at = level_off(l) + code;
            double m, px = 0.0, py = 0.0;
            if (l <= Ls) {
                m = s_cm[at];
                px = s_cx[at];
                py = s_cy[at];
            } else {
                m = cm[at];
                if (m > 0.0) {
                    px = cx[at];
                    py = cy[at];
                }
            }
            if (m > 0.0) {
                const double d0 = yi.x - px, d1 = yi.y - py;
                const double d2 = d0 * d0 + d1 * d1;
                const double sl = side * __longlong_as_double((long long)(1023 - l) << 52);
                if (sl * sl < theta2 * d2) {
                    const double q = 1.0 / (1.0 + d2);
                    const double mqq = m * q * q;
                    r0 += mqq * d0;
                    r1 += mqq * d1;
                    zi += m * q;
                    ++n_acc;
                } else if (l == L) {
                    ++n_exact;
                    const int64_t lo = start[code], hi = start[code + 1];
                    for (int64_t s = lo; s < hi; ++s) {               // ascending index: the sorted order within a cell
                        if (s == (int64_t)t) continue;
                        const double2 yj = ts_load(ys, s);
                        const double e0 = yi.x - yj.x, e1 = yi.y - yj.y;
                        const double q = 1.0 / (1.0 + (e0 * e0 + e1 * e1));
                        const double qq = q * q;
                        r0 += qq * e0;
                        r1 += qq * e1;
                        zi += q;
                        ++n_pairs;
                    }
                } else {
                    ++l;
                    code <<= 2;
                    continue;
                }
            }
            // on to the next cell: the next sibling, or the parent's once the four children are done
            ++code;
            while ((code & 3u) == 0u && l > 0) {
                code >>= 2;
                --l;
            }
        }
        const uint32_t i = order[t];
        reinterpret_cast<double2*>(rep)[i] = make_double2(r0, r1);
        z[i] = zi;
    }
    const double zb = block_sum<4>(zi, s_wave);
    if (threadIdx.x == 0) zpart[blockIdx.x] = zb;
    n_acc = block_sum_thread0<4>(n_acc, s_ctr);
    if (n_acc) atomicAdd(&small[TS_ACC], n_acc);
    __syncthreads();
    n_exact = block_sum_thread0<4>(n_exact, s_ctr);
    if (n_exact) atomicAdd(&small[TS_EXACT], n_exact);
    __syncthreads();
    n_pairs = block_sum_thread0<4>(n_pairs, s_ctr);
    if (n_pairs) atomicAdd(&small[TS_PAIRS], n_pairs);
}

// dst = the sum of part[0 .. nb) by ONE workgroup: thread t chains part[t], part[t + 256], ..., then the workgroup sum
__global__ void __launch_bounds__(256) k_tsne_sum(const double* __restrict__ part, uint64_t nb, double* __restrict__ dst) {
    __shared__ double s_wave[4];
    double s = 0.0;
    for (uint64_t b = threadIdx.x; b < nb; b += 256) s += part[b];
    s = block_sum<4>(s, s_wave);
    if (threadIdx.x == 0) *dst = s;
}

// ---- attraction and the update ---------------------------------------------------------------------------------------------------
struct TsStep {
    double alpha, mu, eta;
    int first;                      // iteration 1: gain 1 and vel 0 without reading them
};

// attr_out: the diagnostic (the attraction alone is written); else the iteration (yout, gain and vel are written)
__global__ void __launch_bounds__(256) k_tsne_step(SymCsr g, const double* __restrict__ yin, double* __restrict__ yout,
                                                   const double* __restrict__ rep, const unsigned long long* __restrict__ small,
                                                   TsStep p, double* __restrict__ gain, double* __restrict__ vel,
                                                   double* __restrict__ attr_out) {
    constexpr int G = kTsGroup;
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = row < g.n;
    double a0 = 0.0, a1 = 0.0;
    double2 yi = make_double2(0.0, 0.0);
    if (live) {
        yi = ts_load(yin, row);
        const uint64_t lo = g.ptr[row], hi = g.ptr[row + 1];
        for (uint64_t e = lo + sub; e < hi; e += G) {
            const double2 yj = ts_load(yin, g.ind[e]);
            const double d0 = yi.x - yj.x, d1 = yi.y - yj.y;
            const double q = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
            const double w = g.w[e] * q;
            a0 += w * d0;
            a1 += w * d1;
        }
    }
    // every lane of the block is here: the butterflies read all of them
    a0 = group_sum<G>(a0);
    a1 = group_sum<G>(a1);
    if (!live || sub != 0) return;
    if (attr_out) {
        reinterpret_cast<double2*>(attr_out)[row] = make_double2(a0, a1);
        return;
    }
    const double Z = __longlong_as_double((long long)small[TS_Z]);
    const double2 r = ts_load(rep, row);
    const double2 gn = p.first ? make_double2(1.0, 1.0) : ts_load(gain, row), v = p.first ? make_double2(0.0, 0.0) : ts_load(vel, row);
    const double at[2] = {a0, a1}, rp[2] = {r.x, r.y}, g_in[2] = {gn.x, gn.y}, v_in[2] = {v.x, v.y}, y_in[2] = {yi.x, yi.y};
    double g_out[2], v_out[2], y_out[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double grad = 4.0 * (p.alpha * at[c] - rp[c] / Z);
        double gg = ((grad > 0.0) != (v_in[c] > 0.0)) ? g_in[c] + 0.2 : g_in[c] * 0.8;
        gg = gg > 0.01 ? gg : 0.01;
        v_out[c] = p.mu * v_in[c] - (p.eta * gg) * grad;
        g_out[c] = gg;
        y_out[c] = y_in[c] + v_out[c];
    }
    reinterpret_cast<double2*>(gain)[row] = make_double2(g_out[0], g_out[1]);
    reinterpret_cast<double2*>(vel)[row] = make_double2(v_out[0], v_out[1]);
    reinterpret_cast<double2*>(yout)[row] = make_double2(y_out[0], y_out[1]);
}

__global__ void __launch_bounds__(256) k_tsne_kl(SymCsr g, const double* __restrict__ y, const unsigned long long* __restrict__ small,
                                                 double* __restrict__ part) {
    constexpr int G = kTsGroup;
    __shared__ double s_wave[4];
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    double acc = 0.0;
    if (row < g.n) {
        const double logZ = log(__longlong_as_double((long long)small[TS_Z]));
        const double2 yi = ts_load(y, row);
        const uint64_t lo = g.ptr[row], hi = g.ptr[row + 1];
        for (uint64_t e = lo + sub; e < hi; e += G) {
            const double2 yj = ts_load(y, g.ind[e]);
            const double d0 = yi.x - yj.x, d1 = yi.y - yj.y;
            const double q = 1.0 / (1.0 + (d0 * d0 + d1 * d1));
            const double w = g.w[e];
            acc += w * ((log(w) - log(q)) + logZ);
        }
    }
    acc = group_sum<G>(acc);
    const double b = block_sum<4>(sub == 0 ? acc : 0.0, s_wave);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static unsigned ts_stride_grid(uint64_t items) {              // grid-stride kernels: at most 8 blocks per CU of the 256
    const uint64_t b = (at_least_one(items) + 255) / 256;
    return (unsigned)(b < 2048 ? b : 2048);
}

int pyramid_levels(uint64_t n, int levels) {
    if (levels) return levels;
    int L = 1;
    while (L < kTsMaxLevels && (1ull << (2 * (L + 1))) < n) ++L;
    return L;
}

void pyramid_bounds(srx_ctx* ctx, const double* d_y, uint64_t n, unsigned long long* d_small) {
    hipLaunchKernelGGL(k_tsne_bounds, dim3(ts_stride_grid(n)), dim3(256), 0, ctx->stream, d_y, n, d_small);
}

void pyramid_up(srx_ctx* ctx, unsigned long long* d_a, unsigned long long* d_b, unsigned long long* d_c, int L) {
    for (int src = L; src > 1;) {
        const int nlev = src - 1 < 3 ? src - 1 : 3;
        const uint64_t waves = ((1ull << (2 * src)) + kWave - 1) / kWave;
        hipLaunchKernelGGL(k_tsne_up, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, ctx->stream, d_a, d_b, d_c, src, nlev);
        src -= nlev;
    }
}

void pyramid_absmax(srx_ctx* ctx, const double* d_x, uint64_t rows, uint64_t ld, unsigned long long* d_dst) {
    hipLaunchKernelGGL(k_tsne_absmax, dim3(ts_stride_grid(rows * 2)), dim3(256), 0, ctx->stream, d_x, rows, ld, d_dst);
}

static SymCsr ts_csr(const srx_tsne* h) { return SymCsr{h->d_ptr, h->d_ind, h->d_dat, h->n, h->info.nnz}; }

static int32_t ts_alloc(srx_tsne* h, uint64_t nnz) {
    const size_t o_ind = up256((h->n + 1) * 8), o_dat = o_ind + up256(nnz * 4), o_beta = o_dat + up256(nnz * 8),
                 total = o_beta + up256(h->n * 8);
    hipError_t e = hipMalloc(&h->d_block, total);
    if (e != hipSuccess)
        return fail(h->ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "tsne: %zu bytes: %s", total, hipGetErrorString(e));
    char* p = (char*)h->d_block;
    h->d_ptr = (uint64_t*)p;
    h->d_ind = (uint32_t*)(p + o_ind);
    h->d_dat = (double*)(p + o_dat);
    h->d_beta = (double*)(p + o_beta);
    return SRX_OK;
}

static srx_tsne* ts_new(srx_ctx* ctx, uint64_t n, uint32_t k, double u) {
    srx_tsne* h = new srx_tsne;
    h->ctx = ctx;
    h->n = n;
    h->k = k;
    h->info.n = n;
    h->info.k = k;
    h->info.perplexity = u;
    return h;
}

// n <= 1: no pairs; indptr = zeros
static int32_t ts_empty(srx_ctx* ctx, uint64_t n, uint32_t k, double u, srx_tsne** out) {
    srx_tsne* h = ts_new(ctx, n, k, u);
    int32_t rc = ts_alloc(h, 0);
    if (rc == SRX_OK && hipMemsetAsync(h->d_block, 0, up256((n + 1) * 8) + up256(n * 8), ctx->stream) != hipSuccess)
        rc = fail(ctx, SRX_E_HIP, "tsne: hipMemsetAsync failed");
    if (rc == SRX_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(ctx, SRX_E_HIP, "tsne: hipStreamSynchronize failed");
    if (rc != SRX_OK) {
        srx_tsne_free(h);
        return rc;
    }
    *out = h;
    return SRX_OK;
}

// perplexity as given -> the one used; k is in range
static int32_t ts_perplexity(srx_ctx* ctx, uint32_t k, double* u) {
    if (*u == 0.0) {
        const double d = (double)k / 3.0;
        *u = d < 30.0 ? d : 30.0;
        if (!(*u > 1.0)) return fail(ctx, SRX_E_ARG, "tsne: the default perplexity min(30, k / 3) = %g is not above 1 (k = %u)", *u, k);
    }
    if (!(*u > 1.0 && *u < (double)k)) return fail(ctx, SRX_E_ARG, "tsne: perplexity = %g outside (1, k = %u)", *u, k);
    return SRX_OK;
}

// d_idx / d_dist: the list on the device (n x k row-major); n >= 2, 2 <= k <= 64, 1 < u < k
static int32_t ts_build(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, double u, srx_tsne** out) {
    Range rg("tsne_affinities");
    srx_tsne* h = ts_new(ctx, n, k, u);
    auto run = [&]() -> int32_t {
        const size_t nk = (size_t)n * k;
        hipStream_t st = ctx->stream;
        unsigned long long* d_small;
        uint32_t* d_dind;
        double *d_p, *d_beta;
        SRX_TRY(scratch(ctx, "graph_small", kPairSmallWords * 8, (void**)&d_small));
        SRX_TRY(scratch(ctx, "tsne_dind", nk * 4, (void**)&d_dind));
        SRX_TRY(scratch(ctx, "tsne_p", nk * 8, (void**)&d_p));
        SRX_TRY(scratch(ctx, "tsne_beta", n * 8, (void**)&d_beta));
        SRX_HIP(ctx, hipMemsetAsync(d_small, 0, kPairSmallWords * 8, st));
        hipLaunchKernelGGL(k_tsne_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, d_idx, d_dist, n, (int)k, u, d_dind, d_p, d_beta,
                           d_small, pair_flag(d_small));
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(list_flag_check(ctx, "tsne", n, pair_flag(d_small)));
        uint64_t ctr[kPairSmallWords], nnz = 0;
        SRX_TRY(pair_union_csr(ctx, PairRule{1, (double)(2 * n)}, d_dind, d_p, n, k, d_small, ctr, &nnz,
                               [&](uint64_t cnt, uint64_t** ptr, uint32_t** ind, double** dat) {
                                   SRX_TRY(ts_alloc(h, cnt));
                                   *ptr = h->d_ptr;
                                   *ind = h->d_ind;
                                   *dat = h->d_dat;
                                   return (int32_t)SRX_OK;
                               }));
        SRX_HIP(ctx, hipMemcpyAsync(h->d_beta, d_beta, n * 8, hipMemcpyDeviceToDevice, st));
        SRX_HIP(ctx, hipStreamSynchronize(st));
        uint64_t sum[kCtrN] = {0, 0, 0, 0, 0};
        for (int s = 0; s < kCtrSlots; ++s)
            for (int c = 0; c < kCtrN; ++c) sum[c] += ctr[s * kCtrN + c];
        h->info.nnz = nnz;
        h->info.n_mutual = sum[kCtrMutual] / 2;
        h->info.rows_no_root = sum[kCtrNoRoot];
        h->info.entries_dropped = sum[kCtrDropped];
        return SRX_OK;
    };
    const int32_t rc = run();
    if (rc != SRX_OK) {
        srx_tsne_free(h);
        return rc;
    }
    *out = h;
    return SRX_OK;
}

// the buffers of a force evaluation at n points and L levels
struct TsWork {
    int L = 0;
    uint32_t total = 0, finest = 0;        // cells of all levels, of level L
    unsigned long long *d_small = nullptr, *d_cnt = nullptr, *d_sx = nullptr, *d_sy = nullptr;
    uint32_t *d_cursor = nullptr, *d_code = nullptr, *d_tmp = nullptr, *d_order = nullptr;
    size_t zero_bytes = 0;                  // d_cnt .. d_cursor are one block, cleared together
    double *d_cx = nullptr, *d_cy = nullptr, *d_cm = nullptr, *d_rep = nullptr, *d_z = nullptr, *d_part = nullptr, *d_ys = nullptr;
    int64_t* d_start = nullptr;
};

static int32_t ts_work(srx_ctx* ctx, uint64_t n, int L, TsWork* w) {
    w->L = L;
    w->total = level_off(L + 1);
    w->finest = 1u << (2 * L);
    const size_t ints = up256((size_t)w->total * 8);
    w->zero_bytes = 3 * ints + up256((size_t)w->finest * 4);
    char* p;
    SRX_TRY(scratch(ctx, "tsne_pyramid", w->zero_bytes, (void**)&p));
    w->d_cnt = (unsigned long long*)p;
    w->d_sx = (unsigned long long*)(p + ints);
    w->d_sy = (unsigned long long*)(p + 2 * ints);
    w->d_cursor = (uint32_t*)(p + 3 * ints);
    SRX_TRY(scratch(ctx, "tsne_com", 3 * ints, (void**)&p));
    w->d_cx = (double*)p;
    w->d_cy = (double*)(p + ints);
    w->d_cm = (double*)(p + 2 * ints);
    SRX_TRY(scratch(ctx, "tsne_small", TS_WORDS * 8, (void**)&w->d_small));
    SRX_TRY(scratch(ctx, "tsne_start", ((size_t)w->finest + 1) * 8, (void**)&w->d_start));
    const size_t n1 = at_least_one(n);
    SRX_TRY(scratch(ctx, "tsne_code", 3 * up256(n1 * 4), (void**)&p));
    w->d_code = (uint32_t*)p;
    w->d_tmp = (uint32_t*)(p + up256(n1 * 4));
    w->d_order = (uint32_t*)(p + 2 * up256(n1 * 4));
    SRX_TRY(scratch(ctx, "tsne_rep", n1 * 16, (void**)&w->d_rep));
    SRX_TRY(scratch(ctx, "tsne_z", n1 * 8, (void**)&w->d_z));
    SRX_TRY(scratch(ctx, "tsne_ys", n1 * 16, (void**)&w->d_ys));
    SRX_TRY(scratch(ctx, "tsne_part", (size_t)grid256(n * (uint64_t)kTsGroup) * 8, (void**)&w->d_part));
    return SRX_OK;
}

// rep, z and Z (small[TS_Z]) at d_y, queued on the context's stream; n >= 1
static int32_t ts_repulsion(srx_ctx* ctx, const TsWork& w, const double* d_y, uint64_t n, double theta) {
    hipStream_t st = ctx->stream;
    const unsigned pts = grid256(n);
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, TS_ZEROED * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(w.d_cnt, 0, w.zero_bytes, st));
    pyramid_bounds(ctx, d_y, n, w.d_small);
    hipLaunchKernelGGL(k_tsne_quant, dim3(pts), dim3(256), 0, st, d_y, n, w.L, w.d_small, w.d_cnt, w.d_sx, w.d_sy, w.d_code);
    pyramid_up(ctx, w.d_cnt, w.d_sx, w.d_sy, w.L);
    hipLaunchKernelGGL(k_tsne_cells, dim3(grid256(w.total)), dim3(256), 0, st, w.d_cnt, w.d_sx, w.d_sy, w.total, w.d_small, w.d_cx, w.d_cy,
                       w.d_cm);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(scan_exclusive(ctx, reinterpret_cast<const int64_t*>(w.d_cnt + level_off(w.L)), w.finest, w.d_start, nullptr));
    hipLaunchKernelGGL(k_tsne_scatter, dim3(pts), dim3(256), 0, st, w.d_code, n, w.d_start, w.d_cursor, w.d_tmp);
    hipLaunchKernelGGL(k_tsne_rank, dim3(pts), dim3(256), 0, st, w.d_code, n, w.d_start, w.d_tmp, d_y, w.d_order, w.d_ys);
    hipLaunchKernelGGL(k_tsne_walk, dim3(pts), dim3(256), 0, st, w.d_ys, w.d_order, n, w.L, theta * theta, w.d_cx, w.d_cy, w.d_cm, w.d_start,
                       w.d_small, w.d_rep, w.d_z, w.d_part);
    hipLaunchKernelGGL(k_tsne_sum, dim3(1), dim3(256), 0, st, w.d_part, (uint64_t)pts, reinterpret_cast<double*>(w.d_small + TS_Z));
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

struct TsOpts {
    srx_tsne_opts o;
    uint32_t iters, run;
    int L;
    double eta;
};

static int32_t ts_check_theta_levels(srx_ctx* ctx, double theta, int32_t levels) {
    if (!(theta >= 0.0 && theta <= kDblMax)) return fail(ctx, SRX_E_ARG, "tsne: theta must be a finite number >= 0");
    if (levels < 0 || levels > kTsMaxLevels) return fail(ctx, SRX_E_ARG, "tsne: levels = %d outside 0..%d", levels, kTsMaxLevels);
    return SRX_OK;
}

static int32_t ts_opts(srx_ctx* ctx, const srx_tsne_opts* in, uint64_t n, TsOpts* out) {
    srx_tsne_opts o = in ? *in : srx_tsne_opts{0.5, 0.0, 0.0, 0, 0, 250, 0, 0, SRX_TSNE_INIT_PCA, 0};
    SRX_TRY(ts_check_theta_levels(ctx, o.theta, o.levels));
    if (!(o.exaggeration >= 0.0 && o.exaggeration <= kDblMax)) return fail(ctx, SRX_E_ARG, "tsne: exaggeration must be a finite number >= 0 (0: 12)");
    if (!(o.learning_rate >= 0.0 && o.learning_rate <= kDblMax))
        return fail(ctx, SRX_E_ARG, "tsne: learning_rate must be a finite number >= 0 (0: max(n / 48, 50))");
    if (o.n_iter < 0 || o.n_iter > SRX_TSNE_MAX_ITERS) return fail(ctx, SRX_E_ARG, "tsne: n_iter = %d outside 0..%d", o.n_iter, SRX_TSNE_MAX_ITERS);
    if (o.exaggeration_iters < 0 || o.exaggeration_iters > SRX_TSNE_MAX_ITERS)
        return fail(ctx, SRX_E_ARG, "tsne: exaggeration_iters = %d outside 0..%d", o.exaggeration_iters, SRX_TSNE_MAX_ITERS);
    if (o.n_iter == 0) o.n_iter = 1000;
    if (o.stop_after < 0 || o.stop_after > o.n_iter)
        return fail(ctx, SRX_E_ARG, "tsne: stop_after = %d outside 0..n_iter = %d", o.stop_after, o.n_iter);
    if (o.init != SRX_TSNE_INIT_GIVEN && o.init != SRX_TSNE_INIT_RANDOM && o.init != SRX_TSNE_INIT_PCA)
        return fail(ctx, SRX_E_ARG, "tsne: unknown start %d", o.init);
    if (o.exaggeration == 0.0) o.exaggeration = 12.0;
    out->o = o;
    out->iters = (uint32_t)o.n_iter;
    out->run = (uint32_t)(o.stop_after ? o.stop_after : o.n_iter);
    out->L = pyramid_levels(n, o.levels);
    const double au = (double)n / 48.0;
    out->eta = o.learning_rate != 0.0 ? o.learning_rate : (au > 50.0 ? au : 50.0);
    return SRX_OK;
}

// the start's arguments, checked before anything is queued
static int32_t ts_check_start(srx_ctx* ctx, const TsOpts& u, srx_mat* m, const double* init, uint64_t n) {
    if (u.o.init == SRX_TSNE_INIT_GIVEN) {
        if (!init && n) return fail(ctx, SRX_E_ARG, "tsne: SRX_TSNE_INIT_GIVEN needs start positions");
    } else if (u.o.init == SRX_TSNE_INIT_PCA) {
        if (!m) return fail(ctx, SRX_E_ARG, "tsne: the PCA start needs the matrix handle that holds the scores");
        if (m->ctx != ctx) return fail(ctx, SRX_E_ARG, "tsne: the matrix and the affinities belong to different contexts");
        if (!m->pca.valid) return fail(ctx, SRX_E_ARG, "tsne: no PCA result on this matrix");
        if (m->pca.n_pc < 2) return fail(ctx, SRX_E_ARG, "tsne: the PCA result has %u components, the start needs 2", m->pca.n_pc);
        const uint64_t cells = m->csc ? m->n_cols : m->n_rows;
        if (cells != n) return fail(ctx, SRX_E_ARG, "tsne: the matrix has %llu cells, the affinities %llu", (unsigned long long)cells, (unsigned long long)n);
    }
    return SRX_OK;
}

// The run (n >= 1).  The result is left in *d_result (one of the two scratch position buffers).
static int32_t tsne_run(srx_tsne* h, const TsOpts& u, srx_mat* m, const double* init, double** d_result, srx_tsne_run_info* info) {
    srx_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = h->n, count = n * 2;
    TsWork w;
    SRX_TRY(ts_work(ctx, n, u.L, &w));
    double *d_y0, *d_y1, *d_gain, *d_vel;
    SRX_TRY(scratch(ctx, "tsne_y0", count * 8, (void**)&d_y0));
    SRX_TRY(scratch(ctx, "tsne_y1", count * 8, (void**)&d_y1));
    SRX_TRY(scratch(ctx, "tsne_gain", count * 8, (void**)&d_gain));
    SRX_TRY(scratch(ctx, "tsne_vel", count * 8, (void**)&d_vel));
    if (u.o.init == SRX_TSNE_INIT_GIVEN) SRX_TRY(h2d(ctx, d_y0, init, count * 8));

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, TS_WORDS * 8, st));
    if (u.o.init == SRX_TSNE_INIT_RANDOM) {
        hipLaunchKernelGGL(k_tsne_init_random, dim3(grid256(count)), dim3(256), 0, st, d_y0, count, u.o.seed);
    } else if (u.o.init == SRX_TSNE_INIT_PCA) {
        const uint64_t ld = (uint64_t)scores_ld((int)m->pca.n_pc);
        pyramid_absmax(ctx, m->pca.d_scores, n, ld, w.d_small + TS_PCAMAX);
        hipLaunchKernelGGL(k_tsne_init_pca, dim3(grid256(count)), dim3(256), 0, st, m->pca.d_scores, n, ld, w.d_small, d_y0);
    }
    pyramid_absmax(ctx, d_y0, n, 2, w.d_small + TS_ABSMAX);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t hs[TS_WORDS];
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (hs[TS_ABSMAX] >= kTsInfBits) {
        if (u.o.init == SRX_TSNE_INIT_PCA && (hs[TS_PCAMAX] == 0 || hs[TS_PCAMAX] >= kTsInfBits))
            return fail(ctx, SRX_E_ARG, "tsne: the PCA start is not usable (the scores are all zero, or hold a NaN or Inf)");
        return fail(ctx, SRX_E_ARG, "tsne: the start positions hold a NaN or Inf");
    }
    double* cur = d_y0;
    double* nxt = d_y1;
    uint32_t ran = 0;
    if (h->info.nnz) {
        const SymCsr g = ts_csr(h);
        const unsigned blocks = grid256(n * (uint64_t)kTsGroup);
        for (uint32_t t = 1; t <= u.run; ++t) {
            const bool early = t <= (uint32_t)u.o.exaggeration_iters;
            const TsStep p{early ? u.o.exaggeration : 1.0, early ? 0.5 : 0.8, u.eta, t == 1};
            SRX_TRY(ts_repulsion(ctx, w, cur, n, u.o.theta));
            hipLaunchKernelGGL(k_tsne_step, dim3(blocks), dim3(256), 0, st, g, cur, nxt, w.d_rep, w.d_small, p, d_gain, d_vel,
                               (double*)nullptr);
            std::swap(cur, nxt);
        }
        ran = u.run;
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
        info->cells_accepted = hs[TS_ACC];
        info->cells_exact = hs[TS_EXACT];
        info->pairs_exact = hs[TS_PAIRS];
        // the pass over the final Y: Z, then the divergence
        SRX_TRY(ts_repulsion(ctx, w, cur, n, u.o.theta));
        hipLaunchKernelGGL(k_tsne_kl, dim3(blocks), dim3(256), 0, st, g, cur, w.d_small, w.d_part);
        hipLaunchKernelGGL(k_tsne_sum, dim3(1), dim3(256), 0, st, w.d_part, (uint64_t)blocks, reinterpret_cast<double*>(w.d_small + TS_KL));
        SRX_HIP(ctx, hipGetLastError());
    }
    SRX_TRY(timer.stop(&info->ms));
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    info->iters_run = ran;
    if (ran) {
        memcpy(&info->Z, &hs[TS_Z], 8);
        memcpy(&info->kl, &hs[TS_KL], 8);
        memcpy(&info->side, &hs[TS_SIDE], 8);
    }
    *d_result = cur;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_tsne_affinities_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                                double perplexity, srx_tsne** out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (!out) return fail(ctx, SRX_E_ARG, "tsne: null output handle");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "tsne: rows are sharded; the affinities need all cells");
    if (k < 2 || k > (uint32_t)SRX_TSNE_MAX_K) return fail(ctx, SRX_E_ARG, "tsne: k = %u outside 2..%d", k, SRX_TSNE_MAX_K);
    SRX_TRY(ts_perplexity(ctx, k, &perplexity));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (n <= 1) return ts_empty(ctx, n, k, perplexity, out);
    if (!indices || !distances) return fail(ctx, SRX_E_ARG, "tsne: null k-NN list");
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "tsne: more than 2^32 - 2 cells");
    if ((uint64_t)k > n - 1) return fail(ctx, SRX_E_ARG, "tsne: k = %u but a cell has only %llu others", k, (unsigned long long)(n - 1));
    uint32_t* d_idx;
    double* d_dist;
    SRX_TRY(scratch(ctx, "graph_in_idx", n * k * 4, (void**)&d_idx));
    SRX_TRY(scratch(ctx, "graph_in_dist", n * k * 8, (void**)&d_dist));
    SRX_TRY(h2d(ctx, d_idx, indices, n * k * 4));
    SRX_TRY(h2d(ctx, d_dist, distances, n * k * 8));
    return ts_build(ctx, d_idx, d_dist, n, k, perplexity, out);
}

int32_t srx_tsne_affinities_graph(srx_graph* g, double perplexity, srx_tsne** out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "tsne: null output handle");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "tsne: rows are sharded; the affinities need all cells");
    if (g->k < 2 || g->k > (uint32_t)SRX_TSNE_MAX_K) return fail(ctx, SRX_E_ARG, "tsne: k = %u outside 2..%d", g->k, SRX_TSNE_MAX_K);
    SRX_TRY(ts_perplexity(ctx, g->k, &perplexity));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (g->n <= 1) return ts_empty(ctx, g->n, g->k, perplexity, out);
    return ts_build(ctx, g->d_dind, g->d_ddat, g->n, g->k, perplexity, out);
}

int32_t srx_tsne_info_get(const srx_tsne* h, srx_tsne_info* info) {
    if (!h || !info) return fail(h ? h->ctx : nullptr, SRX_E_ARG, "null argument");
    *info = h->info;
    return SRX_OK;
}

int32_t srx_tsne_fetch_affinities(srx_tsne* h, uint64_t* indptr, uint32_t* indices, double* data, double* beta) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null tsne handle");
    srx_ctx* ctx = h->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (indptr) SRX_TRY(d2h(ctx, indptr, h->d_ptr, (h->n + 1) * 8));
    if (indices && h->info.nnz) SRX_TRY(d2h(ctx, indices, h->d_ind, h->info.nnz * 4));
    if (data && h->info.nnz) SRX_TRY(d2h(ctx, data, h->d_dat, h->info.nnz * 8));
    if (beta && h->n) SRX_TRY(d2h(ctx, beta, h->d_beta, h->n * 8));
    return SRX_OK;
}

int32_t srx_tsne_forces(srx_tsne* h, const double* Y, double theta, int32_t levels, double* attr_out, double* rep_out, double* z_out,
                        srx_tsne_force_info* info) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null tsne handle");
    srx_ctx* ctx = h->ctx;
    SRX_TRY(ts_check_theta_levels(ctx, theta, levels));
    const uint64_t n = h->n;
    srx_tsne_force_info fi{};
    fi.levels = (uint32_t)pyramid_levels(n, levels);
    if (n == 0) {
        if (info) *info = fi;
        return SRX_OK;
    }
    if (!Y) return fail(ctx, SRX_E_ARG, "tsne: null positions");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    Range rg("tsne_forces");
    TsWork w;
    SRX_TRY(ts_work(ctx, n, (int)fi.levels, &w));
    double *d_y, *d_attr;
    SRX_TRY(scratch(ctx, "tsne_y0", n * 16, (void**)&d_y));
    SRX_TRY(scratch(ctx, "tsne_y1", n * 16, (void**)&d_attr));
    SRX_TRY(h2d(ctx, d_y, Y, n * 16));
    hipStream_t st = ctx->stream;
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, TS_WORDS * 8, st));
    pyramid_absmax(ctx, d_y, n, 2, w.d_small + TS_ABSMAX);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t hs[TS_WORDS];
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (hs[TS_ABSMAX] >= kTsInfBits) return fail(ctx, SRX_E_ARG, "tsne: the positions hold a NaN or Inf");
    SRX_TRY(ts_repulsion(ctx, w, d_y, n, theta));
    hipLaunchKernelGGL(k_tsne_step, dim3(grid256(n * (uint64_t)kTsGroup)), dim3(256), 0, st, ts_csr(h), d_y, (double*)nullptr, w.d_rep,
                       w.d_small, TsStep{1.0, 0.0, 0.0, 1}, (double*)nullptr, (double*)nullptr, d_attr);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (attr_out) SRX_TRY(d2h(ctx, attr_out, d_attr, n * 16));
    if (rep_out) SRX_TRY(d2h(ctx, rep_out, w.d_rep, n * 16));
    if (z_out) SRX_TRY(d2h(ctx, z_out, w.d_z, n * 8));
    memcpy(&fi.side, &hs[TS_SIDE], 8);
    memcpy(&fi.lo[0], &hs[TS_LO0], 8);
    memcpy(&fi.lo[1], &hs[TS_LO1], 8);
    fi.cells_accepted = hs[TS_ACC];
    fi.cells_exact = hs[TS_EXACT];
    fi.pairs_exact = hs[TS_PAIRS];
    if (info) *info = fi;
    return SRX_OK;
}

int32_t srx_tsne_run(srx_tsne* h, srx_mat* m, const srx_tsne_opts* opts, const double* init, double* embedding_out,
                     srx_tsne_run_info* info) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null tsne handle");
    srx_ctx* ctx = h->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "tsne: rows are sharded; the layout needs all cells");
    TsOpts u;
    SRX_TRY(ts_opts(ctx, opts, h->n, &u));
    SRX_TRY(ts_check_start(ctx, u, m, init, h->n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_tsne_run_info li{};
    li.n = h->n;
    li.nnz = h->info.nnz;
    li.n_iter = u.iters;
    li.levels = (uint32_t)u.L;
    li.eta = u.eta;
    if (h->n) {
        Range rg("tsne");
        double* d_res = nullptr;
        SRX_TRY(tsne_run(h, u, m, init, &d_res, &li));
        h->embed_valid = false;
        SRX_TRY(keep_on_handle(ctx, &h->d_embed, false, d_res, (size_t)h->n * 16));
        if (embedding_out) SRX_TRY(d2h(ctx, embedding_out, h->d_embed, (size_t)h->n * 16));
    }
    h->embed_valid = true;
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_tsne_embedding_fetch(srx_tsne* h, double* out) {
    if (!h) return fail(nullptr, SRX_E_ARG, "null tsne handle");
    srx_ctx* ctx = h->ctx;
    if (!h->embed_valid) return fail(ctx, SRX_E_ARG, "srx_tsne_embedding_fetch: no srx_tsne_run has run on this handle");
    if (!h->n || !out) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, out, h->d_embed, (size_t)h->n * 16);
}

void srx_tsne_free(srx_tsne* h) {
    if (!h) return;
    if (h->d_block || h->d_embed) {
        (void)hipSetDevice(h->ctx->device);
        (void)hipStreamSynchronize(h->ctx->stream);
        if (h->d_block) (void)hipFree(h->d_block);
        if (h->d_embed) (void)hipFree(h->d_embed);
    }
    delete h;
}

}  // extern "C"
