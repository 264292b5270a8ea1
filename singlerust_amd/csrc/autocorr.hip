// autocorr.hip — Moran's I and Geary's C per gene on a neighbour graph (srx_autocorr, srx_autocorr_csr; srx_autocorr_from_tables
// is the host arithmetic alone).  The definition is in include/srx.h; the design and the LDS budget are in DESIGN.md
// ("Spatial autocorrelation").
//
// The statistics need five per-gene sums.  Four of them (S, Q, A, B) are sums over the stored entries of the matrix with a
// per-row factor, the grouped-moments walk of markers.hip without the labels.  The fifth, P = sum over the edges (i, j > i) of
// w_ij x_i x_j, JOINS two sparse rows per edge: the kernel pattern of this file.  A workgroup owns one gene tile of the matrix
// and a block of rows; per row i it scatters the row's tile segment into a dense LDS table T[gene] = x_ig, its waves take the
// row's neighbours j > i one each, stream row j's tile segment, look T up and add the fixed-point term to a 64-bit LDS
// accumulator per gene, and the row's segment is walked once more to clear T.  T and the accumulator are 16 B per gene: what
// a gene tile of the matrix is sized for, so the cached tile cuts and the 16-bit index mirror serve as they are, and the other
// four tables take two launches of their own at 16 B per gene each instead of narrowing the walk's tile to a fifth.
//
// Kernels:
//   k_ac_wmax          the largest weight (integer max of the bit patterns: the weights are positive)
//   k_ac_degrees       wave per row of the graph: dq_i, and W, S1 and max dq over the grid
//   k_ac_s2            S2 from the dq_i
//   k_ac_moments<W>    workgroup = (gene tile, row block), wave per row: {S, Q}, or with W {A, B}
//   k_ac_walk          workgroup = (gene tile, row block): P
#include "graph_handle.hpp"
#include "markers_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

// srx.h states every product as rounded once: no FMA contraction in the code below
#pragma clang fp contract(off)

namespace srx {

constexpr int kAcThreads = 1024;          // one workgroup per CU: T and the accumulators fill the LDS
constexpr int kAcWaves = kAcThreads / kWave;
constexpr uint64_t kAcMinRows = 16;       // rows_per_block = max(kAcMinRows, ceil(N / max(1, kAcBlocks / n_tiles)))
constexpr uint64_t kAcBlocks = 4096;      // ... many short blocks: the rows at the top of the triangle hold most of the edges

// d_small: value_scan's two words, then these
enum { AC_WMAX = VS_WORDS, AC_W, AC_S1, AC_MAXDQ, AC_S2, AC_WORDS };

__device__ __forceinline__ double ac_mul(double a, double b) { return a * b; }
__device__ __forceinline__ long long ac_fix(double v, double fx) { return (long long)__builtin_rint(ac_mul(v, fx)); }

__global__ __launch_bounds__(256) void k_ac_wmax(const double* __restrict__ w, uint64_t nnz, unsigned long long* __restrict__ small) {
    unsigned long long mx = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(w[e]);
        mx = b > mx ? b : mx;
    }
    mx = wave_max(mx);
    if (lane_id() == 0 && mx) atomicMax(&small[AC_WMAX], mx);
}

// a wave takes the rows wave, wave + waves of the grid, ...; its sums join the grid's once
__global__ __launch_bounds__(256) void k_ac_degrees(const uint64_t* __restrict__ ptr, const double* __restrict__ w, uint64_t n, double fx_w,
                                                    double fx_1, long long* __restrict__ dq, unsigned long long* __restrict__ small) {
    const int lane = lane_id();
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
    long long tot_w = 0, tot_1 = 0, max_dq = 0;
    for (uint64_t row = global_wave_id(); row < n; row += waves) {
        const uint64_t lo = ptr[row], hi = ptr[row + 1];
        long long a = 0, b = 0;
        for (uint64_t e = lo + lane; e < hi; e += kWave) {
            const double v = w[e];
            a += ac_fix(v, fx_w);
            b += ac_fix(ac_mul(v, v), fx_1);
        }
        a = wave_sum(a);
        tot_1 += b;
        tot_w += lane == 0 ? a : 0;
        max_dq = a > max_dq ? a : max_dq;
        if (lane == 0) dq[row] = a;
    }
    tot_w = wave_sum(tot_w);
    tot_1 = wave_sum(tot_1);
    if (lane == 0) {
        if (tot_w) atomicAdd(&small[AC_W], (unsigned long long)tot_w);
        if (tot_1) atomicAdd(&small[AC_S1], (unsigned long long)tot_1);
        if (max_dq) atomicMax(&small[AC_MAXDQ], (unsigned long long)max_dq);
    }
}

__global__ __launch_bounds__(256) void k_ac_s2(const long long* __restrict__ dq, uint64_t n, double inv_w, double fx_2,
                                               unsigned long long* __restrict__ small) {
    long long t = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double d = ac_mul((double)dq[i], inv_w);
        t += ac_fix(ac_mul(d, d), fx_2);
    }
    t = wave_sum(t);
    if (lane_id() == 0 && t) atomicAdd(&small[AC_S2], (unsigned long long)t);
}

// {S, Q} (WEIGHTED false: fx_a = 2^s_S, fx_b = 2^s_Q) or {A, B} (fx_a = 2^s_A, fx_b = 2^s_B) of the rows [r0, r1) of the block
// within one gene tile: the accumulators side by side per gene in LDS, flushed by global integer atomics for the touched genes.
template <typename T, typename I, bool WEIGHTED>
__global__ __launch_bounds__(kAcThreads) void k_ac_moments(const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp,
                                                           const I* __restrict__ idx, const T* __restrict__ vals, uint64_t n_rows,
                                                           uint64_t n_cols, int n_tiles, int tile_genes, uint64_t rows_per_block,
                                                           const long long* __restrict__ dq, double inv_w, double fx_a, double fx_b,
                                                           unsigned long long* __restrict__ out_a, unsigned long long* __restrict__ out_b) {
    extern __shared__ double lds[];
    unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(lds);
    for (int g = threadIdx.x; g < 2 * tile_genes; g += kAcThreads) s_acc[g] = 0ull;
    __syncthreads();
    const int tile = blockIdx.x % n_tiles;
    const uint64_t r0 = (uint64_t)(blockIdx.x / n_tiles) * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int32_t gbase = tile * tile_genes;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    for (uint64_t r = r0 + wave; r < r1; r += kAcWaves) {
        int64_t lo, hi;
        seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
        const double d = WEIGHTED ? ac_mul((double)dq[r], inv_w) : 1.0;
        for (int64_t e = lo + lane; e < hi; e += kWave) {
            const int32_t g0 = (int32_t)idx[e] - gbase;
            const double x = (double)vals[e];
            const double xx = ac_mul(x, x);
            const long long ia = WEIGHTED ? ac_fix(ac_mul(d, x), fx_a) : ac_fix(x, fx_a);
            const long long ib = WEIGHTED ? ac_fix(ac_mul(d, xx), fx_b) : ac_fix(xx, fx_b);
            __hip_atomic_fetch_add(&s_acc[2 * g0], (unsigned long long)ia, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_add(&s_acc[2 * g0 + 1], (unsigned long long)ib, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < tile_genes; g += kAcThreads) {
        const uint64_t gene = (uint64_t)gbase + g;
        if (gene >= n_cols) continue;
        if (s_acc[2 * g]) atomicAdd(&out_a[gene], s_acc[2 * g]);
        if (s_acc[2 * g + 1]) atomicAdd(&out_b[gene], s_acc[2 * g + 1]);
    }
}

// P of the rows [r0, r1) of the block within one gene tile.  LDS: T (tile_genes f64: x_ig of the row in hand, +0 elsewhere),
// then the accumulators (tile_genes u64).  Every condition around a barrier is uniform over the workgroup: it depends on the
// row alone.  An entry of row j meets T == 0 where row i stores nothing, or stores a zero of either sign: its term would be
// rint(+-0) = 0, so it is skipped.  The rows of the graph are strictly ascending (the caller's check), so the neighbours
// above i are the tail of the row from the first index > i.
// One workgroup fills the LDS of its CU, so nothing else hides the latency of a row's chain of dependent loads (its cuts and
// graph offsets -> its entries and neighbours -> the neighbours' cuts -> their entries): the kernel keeps the next rows'
// loads in flight itself (profiles/autocorr.md).  The cuts and offsets of row i + 2 and the entries and the first 64
// neighbours of row i + 1 are requested before row i is walked; a thread keeps its entry of the row in registers for the
// scatter and the clear (segments beyond 1024 entries and rows beyond 64 neighbours take the plain loads); the first
// neighbour above i is a ballot over the lanes' neighbours, and a wave reads its neighbour's index from a lane, not from
// memory; a lane takes 4 consecutive entries of a neighbour's segment from the 4-entry boundary at or before its start, two
// such chunks in flight (the arrays of a matrix are padded by 16 entries; entries outside the segment are masked).
struct AcRow {                 // wave-uniform: what is known of a row before its entries are read
    int64_t lo, hi;            // its segment in the tile
    uint64_t a, cend;          // its row of the graph
};
struct AcEntries {             // per thread: entry lo + threadIdx.x of the segment (g < 0: none), neighbour a + lane (none: ~0)
    int32_t g;
    double x;
    uint32_t nb;
};
template <typename T, typename I>
__global__ __launch_bounds__(kAcThreads) void k_ac_walk(const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp,
                                                        const I* __restrict__ idx, const T* __restrict__ vals, uint64_t n_rows,
                                                        uint64_t n_cols, int n_tiles, int tile_genes, uint64_t rows_per_block,
                                                        const uint64_t* __restrict__ cptr, const uint32_t* __restrict__ cind,
                                                        const double* __restrict__ cw, double fx_p,
                                                        unsigned long long* __restrict__ out_p) {
    extern __shared__ double lds[];
    double* s_t = lds;
    unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(lds + tile_genes);
    for (int g = threadIdx.x; g < tile_genes; g += kAcThreads) {
        s_t[g] = 0.0;
        s_acc[g] = 0ull;
    }
    __syncthreads();
    const int tile = blockIdx.x % n_tiles;
    const uint64_t r0 = (uint64_t)(blockIdx.x / n_tiles) * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int32_t gbase = tile * tile_genes;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    auto load_row = [&](uint64_t r) {
        AcRow p{0, 0, 0, 0};
        if (r < r1) {
            seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, p.lo, p.hi);
            p.a = cptr[r];
            p.cend = cptr[r + 1];
        }
        return p;
    };
    auto load_entries = [&](const AcRow& p) {
        AcEntries e{-1, 0.0, 0xffffffffu};
        const int64_t at = p.lo + threadIdx.x;
        if (at < p.hi) {
            e.g = (int32_t)idx[at] - gbase;
            e.x = (double)vals[at];
        }
        if (p.a + lane < p.cend) e.nb = cind[p.a + lane];
        return e;
    };
    struct Chunk {
        int32_t g[4];
        T v[4];
    };
    auto load_chunk = [&](int64_t e0, Chunk& c) {
        if constexpr (sizeof(I) == 4) {
            const int4 g4 = *reinterpret_cast<const int4*>(idx + e0);
            c.g[0] = g4.x; c.g[1] = g4.y; c.g[2] = g4.z; c.g[3] = g4.w;
        } else {
            const uint2 g2 = *reinterpret_cast<const uint2*>(idx + e0);
            c.g[0] = (int)(g2.x & 0xffffu); c.g[1] = (int)(g2.x >> 16);
            c.g[2] = (int)(g2.y & 0xffffu); c.g[3] = (int)(g2.y >> 16);
        }
        if constexpr (sizeof(T) == 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(vals + e0);
            c.v[0] = t4.x; c.v[1] = t4.y; c.v[2] = t4.z; c.v[3] = t4.w;
        } else {
            const double2 a2 = *reinterpret_cast<const double2*>(vals + e0);
            const double2 b2 = *reinterpret_cast<const double2*>(vals + e0 + 2);
            c.v[0] = a2.x; c.v[1] = a2.y; c.v[2] = b2.x; c.v[3] = b2.y;
        }
    };
    auto add_chunk = [&](int64_t e0, int64_t lo, int64_t hi, double w, const Chunk& c) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e0 + k >= lo && e0 + k < hi) {
                const int32_t g0 = c.g[k] - gbase;
                const double xi = s_t[g0];
                if (xi != 0.0) {
                    const long long ip = ac_fix(ac_mul(w, ac_mul(xi, (double)c.v[k])), fx_p);
                    __hip_atomic_fetch_add(&s_acc[g0], (unsigned long long)ip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    };
    AcRow cur = load_row(r0), nxt = load_row(r0 + 1);
    AcEntries ce = load_entries(cur);
    for (uint64_t i = r0; i < r1; ++i) {
        const AcRow nn = load_row(i + 2);
        const AcEntries ne = load_entries(nxt);
        // the first neighbour above i: a lane without a neighbour holds ~0, above every row number
        uint64_t first;
        if (cur.cend - cur.a <= (uint64_t)kWave) {
            first = cur.a + (uint64_t)__popcll(__ballot(ce.nb <= (uint32_t)i));
        } else {
            uint64_t a = cur.a, b = cur.cend;
            while (a < b) {
                const uint64_t mid = a + ((b - a) >> 1);
                if (cind[mid] <= (uint32_t)i) a = mid + 1;
                else b = mid;
            }
            first = a;
        }
        if (cur.hi > cur.lo && first < cur.cend) {            // the row stores something in this tile and has a neighbour above it
            if (ce.g >= 0) s_t[ce.g] = ce.x;
            for (int64_t e = cur.lo + kAcThreads + threadIdx.x; e < cur.hi; e += kAcThreads) s_t[(int32_t)idx[e] - gbase] = (double)vals[e];
            __syncthreads();
            for (uint64_t q = first + wave; q < cur.cend; q += kAcWaves) {
                const uint64_t off = q - cur.a;
                const uint64_t j = off < (uint64_t)kWave ? (uint32_t)__builtin_amdgcn_readlane((int)ce.nb, __builtin_amdgcn_readfirstlane((int)off))
                                                         : cind[q];
                const double w = cw[q];
                int64_t jlo, jhi;
                seg_bounds(indptr, tp, n_rows, n_tiles, tile, j, jlo, jhi);
                const int64_t b0 = jlo & ~(int64_t)3;
                for (int64_t e0 = b0 + 4 * lane; e0 < jhi; e0 += 8 * kWave) {
                    const int64_t e1 = e0 + 4 * kWave;
                    Chunk c0, c1;
                    load_chunk(e0, c0);
                    load_chunk(e1 < jhi ? e1 : b0, c1);
                    add_chunk(e0, jlo, jhi, w, c0);
                    if (e1 < jhi) add_chunk(e1, jlo, jhi, w, c1);
                }
            }
            __syncthreads();
            if (ce.g >= 0) s_t[ce.g] = 0.0;
            for (int64_t e = cur.lo + kAcThreads + threadIdx.x; e < cur.hi; e += kAcThreads) s_t[(int32_t)idx[e] - gbase] = 0.0;
            __syncthreads();
        }
        cur = nxt;
        nxt = nn;
        ce = ne;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < tile_genes; g += kAcThreads) {
        const uint64_t gene = (uint64_t)gbase + g;
        if (gene < n_cols && s_acc[g]) atomicAdd(&out_p[gene], s_acc[g]);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static int ceil_log2(uint64_t v) {
    int L = 0;
    while ((1ull << L) < at_least_one(v)) ++L;
    return L;
}

struct AcGraphSums {
    long long W = 0, S1 = 0, S2 = 0;
    int s_w = 0, s_1 = 0, s_2 = 0;
};

// The eight scales of srx.h from info's n, nnz, max_abs, max_weight and max_degree (0 while it is not known: the scales that
// need it are then provisional).  Refuses maxima beyond the range in which every product of the definition stays finite.
constexpr double kAcMaxFactor = 5.78960446186580977e76;        // 2^255
static int32_t ac_scales(srx_ctx* ctx, const char* who, srx_autocorr_info* info) {
    if (info->n < 2 || info->n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "%s: N = %llu is outside 2 .. 2^32 - 2", who, (unsigned long long)info->n);
    if (!info->nnz) return fail(ctx, SRX_E_ARG, "%s: the graph has no stored entries (W = 0)", who);
    if (!(info->max_abs >= 0.0 && info->max_abs < kAcMaxFactor))
        return fail(ctx, SRX_E_ARG, "%s: max |x| = %g is not below 2^255: x x and its products with the weights would leave the f64 range", who, info->max_abs);
    if (!(info->max_weight >= 0.0 && info->max_weight < kAcMaxFactor) || !(info->max_degree >= 0.0 && info->max_degree < kAcMaxFactor))
        return fail(ctx, SRX_E_ARG, "%s: the largest weight %g or row sum %g is not below 2^255", who, info->max_weight, info->max_degree);
    const int e_x = fx_exponent(info->max_abs), e_w = fx_exponent(info->max_weight), e_d = fx_exponent(info->max_degree);
    const int L_N = ceil_log2(info->n), L_E = ceil_log2(info->nnz);
    info->s_sum = 62 - e_x - L_N;
    info->s_sumsq = 62 - 2 * e_x - L_N;
    info->s_dsum = 62 - e_d - e_x - L_N;
    info->s_dsumsq = 62 - e_d - 2 * e_x - L_N;
    info->s_cross = 62 - e_w - 2 * e_x - L_E;
    info->s_w = 62 - e_w - L_E;
    info->s_1 = 62 - 2 * e_w - L_E;
    info->s_2 = 62 - 2 * e_d - L_N;
    return SRX_OK;
}

// The statistics of srx.h from the five tables, in the order stated there.
static void ac_finish(const long long* S, const long long* Q, const long long* A, const long long* B, const long long* P, uint64_t G,
                      srx_autocorr_out* out, srx_autocorr_info* info) {
    typedef long double ld;
    const ld N = (ld)info->n;
    const ld W = std::ldexp((ld)info->w_int, -info->s_w);
    const ld s1 = std::ldexp((ld)info->s1_int, 1 - info->s_1), s2 = std::ldexp((ld)info->s2_int, 2 - info->s_2);
    const ld e_i = (ld)-1 / (N - 1);
    const ld var_i = (N * N * s1 - N * s2 + 3 * (W * W)) / ((N * N - 1) * (W * W)) - e_i * e_i;
    const ld var_c = ((2 * s1 + s2) * (N - 1) - 4 * (W * W)) / (2 * (N + 1) * (W * W));
    info->w = (double)W;
    info->s1 = (double)s1;
    info->s2 = (double)s2;
    info->e_i = (double)e_i;
    info->var_i = (double)var_i;
    info->e_c = 1.0;
    info->var_c = (double)var_c;
    const ld sd_i = var_i > 0 ? sqrtl(var_i) : 0, sd_c = var_c > 0 ? sqrtl(var_c) : 0;
    const int sh = 2 * info->s_sum - info->s_sumsq;          // 62 - L_N: 30 .. 61 for 2 <= N < 2^32
    const double nan = std::nan("");
    uint64_t constant = 0;
    for (uint64_t g = 0; g < G; ++g) {
        if (out) {
            if (out->sum) out->sum[g] = std::ldexp((double)S[g], -info->s_sum);
            if (out->sumsq) out->sumsq[g] = std::ldexp((double)Q[g], -info->s_sumsq);
            if (out->dsum) out->dsum[g] = std::ldexp((double)A[g], -info->s_dsum);
            if (out->dsumsq) out->dsumsq[g] = std::ldexp((double)B[g], -info->s_dsumsq);
            if (out->cross) out->cross[g] = std::ldexp((double)P[g], -info->s_cross);
        }
        const __int128 a = (__int128)info->n * (__int128)Q[g];                   // below 2^94
        const unsigned __int128 b = (unsigned __int128)((__int128)S[g] * (__int128)S[g]);      // at most 2^124
        const __int128 D = a - (__int128)(b >> sh);
        const uint64_t r = (uint64_t)(b & (((unsigned __int128)1 << sh) - 1));
        double vi = nan, vc = nan, zi = nan, zc = nan;
        if (D >= 1) {
            const ld den = std::ldexp(std::ldexp((ld)D, sh) - (ld)r, -2 * info->s_sum) / N;
            const ld Sg = std::ldexp((ld)S[g], -info->s_sum), Ag = std::ldexp((ld)A[g], -info->s_dsum);
            const ld Bg = std::ldexp((ld)B[g], -info->s_dsumsq), Pg = std::ldexp((ld)P[g], -info->s_cross);
            const ld t1 = 2 * Pg, t2 = (2 * (Sg * Ag)) / N, t3 = (((Sg * Sg) * W) / N) / N;
            const ld num_i = (t1 - t2) + t3;
            const ld I = ((N * num_i) / W) / den;
            const ld num_c = Bg - 2 * Pg;
            const ld Cc = (((N - 1) * num_c) / W) / den;
            vi = (double)I;
            vc = (double)Cc;
            if (var_i > 0) zi = (double)((I - e_i) / sd_i);
            if (var_c > 0) zc = (double)((Cc - 1) / sd_c);
        } else {
            ++constant;
        }
        if (out) {
            if (out->morans_i) out->morans_i[g] = vi;
            if (out->gearys_c) out->gearys_c[g] = vc;
            if (out->z_i) out->z_i[g] = zi;
            if (out->z_c) out->z_c[g] = zc;
        }
    }
    info->genes_constant = constant;
}

static uint64_t ac_rows_per_block(uint64_t n_rows, int n_tiles, const srx_autocorr_opts* opts) {
    if (opts && opts->rows_per_block) return opts->rows_per_block;
    const uint64_t want = std::max<uint64_t>(1, kAcBlocks / (uint64_t)std::max(n_tiles, 1));
    return std::max<uint64_t>(kAcMinRows, (n_rows + want - 1) / want);
}

// the refusals that need no pass over the data; sets the device
static int32_t ac_check(srx_mat* m, uint64_t n, const char* who) {
    if (!m) return fail(nullptr, SRX_E_ARG, "%s: null matrix", who);
    srx_ctx* ctx = m->ctx;
    if (m->csc) return fail(ctx, SRX_E_ARG, "%s walks cells: convert the CSC matrix with srx_matrix_to_csr", who);
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: rows are sharded; the graph of the cells lives on one rank", who);
    if (m->n_rows >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "%s: 2^32 - 1 rows or more", who);
    if (n != m->n_rows)
        return fail(ctx, SRX_E_ARG, "%s: the graph has %llu cells, the matrix %llu rows", who, (unsigned long long)n, (unsigned long long)m->n_rows);
    if (n < 2) return fail(ctx, SRX_E_ARG, "%s: N = %llu; the statistics need at least 2 cells", who, (unsigned long long)n);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return SRX_OK;
}

// c: a checked symmetric graph on the device (n = the matrix's rows, nnz > 0)
static int32_t ac_run(srx_mat* m, const SymCsr& c, const char* who, const srx_autocorr_opts* opts, srx_autocorr_out* out,
                      srx_autocorr_info* info_out) {
    srx_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t N = m->n_rows, G = m->n_cols;
    if (!c.nnz) return fail(ctx, SRX_E_ARG, "%s: the graph has no stored entries (W = 0)", who);
    Range rg("autocorr");
    SRX_TRY(ensure_tiles(m));                     // pattern-only: tile cuts and the 16-bit index mirror (cached on the handle)
    srx_autocorr_info info{};
    info.n = N; info.n_genes = G; info.nnz = c.nnz;

    unsigned long long* d_small;
    long long* d_dq;
    unsigned long long* d_tab;
    const uint64_t Gp = at_least_one(G);
    SRX_TRY(scratch(ctx, "ac_small", AC_WORDS * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "ac_dq", N * 8, (void**)&d_dq));
    {
        const int32_t rc = scratch(ctx, "ac_tables", 5 * Gp * 8, (void**)&d_tab);
        if (rc != SRX_OK) {
            (void)hipGetLastError();
            return fail(ctx, rc, "%s: the 5 x %llu tables (%llu bytes) do not fit", who, (unsigned long long)G, (unsigned long long)(5 * Gp * 8));
        }
    }
    unsigned long long *d_S = d_tab, *d_Q = d_tab + Gp, *d_A = d_tab + 2 * Gp, *d_B = d_tab + 3 * Gp, *d_P = d_tab + 4 * Gp;
    StreamTimer t_graph(ctx, st), t_mom(ctx, st), t_walk(ctx, st);          // the three parts; within them a timer per kernel
    StreamTimer t_wmax(ctx, st), t_deg(ctx, st), t_s2(ctx, st), t_sq(ctx, st), t_ab(ctx, st);

    // -- the graph sums; max |x| and non-finite values
    SRX_TRY(t_graph.start());
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, AC_WORDS * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(d_tab, 0, 5 * Gp * 8, st));
    value_scan(m, d_small);
    const unsigned grid_e = (unsigned)std::min<uint64_t>((c.nnz + 255) / 256, (uint64_t)ctx->n_cus * 8);
    const unsigned grid_n = (unsigned)std::min<uint64_t>((N + 255) / 256, (uint64_t)ctx->n_cus * 8);
    SRX_TRY(t_wmax.start());
    hipLaunchKernelGGL(k_ac_wmax, dim3(grid_e), dim3(256), 0, st, c.w, c.nnz, d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_wmax.stop(&info.ms_wmax));
    unsigned long long small[AC_WORDS];
    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    if (small[VS_FLAGS] & kValNonFinite) return fail(ctx, SRX_E_NAN, "%s: a stored value is NaN or Inf", who);
    memcpy(&info.max_abs, &small[VS_MAXABS], 8);
    memcpy(&info.max_weight, &small[AC_WMAX], 8);
    SRX_TRY(ac_scales(ctx, who, &info));                  // those that need no degree; the rest once max d is known
    const double inv_w = std::ldexp(1.0, -info.s_w);
    SRX_TRY(t_deg.start());
    hipLaunchKernelGGL(k_ac_degrees, dim3((unsigned)std::min<uint64_t>((N + 3) / 4, (uint64_t)ctx->n_cus * 8)), dim3(256), 0, st, c.ptr, c.w, N,
                       std::ldexp(1.0, info.s_w), std::ldexp(1.0, info.s_1), d_dq, d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_deg.stop(&info.ms_degrees));
    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    info.w_int = (int64_t)small[AC_W];
    info.s1_int = (int64_t)small[AC_S1];
    info.max_degree = (double)(long long)small[AC_MAXDQ] * inv_w;
    SRX_TRY(ac_scales(ctx, who, &info));
    SRX_TRY(t_s2.start());
    hipLaunchKernelGGL(k_ac_s2, dim3(grid_n), dim3(256), 0, st, (const long long*)d_dq, N, inv_w, std::ldexp(1.0, info.s_2), d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(t_s2.stop(&info.ms_s2));
    SRX_TRY(t_graph.stop(&info.ms_graph));

    // -- the four tables over the rows, then the walk over the edges
    const uint64_t rpb = ac_rows_per_block(N, m->n_tiles, opts);
    const uint64_t n_blocks = (N + rpb - 1) / rpb;
    const dim3 grid((unsigned)(n_blocks * (uint64_t)m->n_tiles));
    const size_t lds = (size_t)m->tile_genes * 16;
    if (n_blocks * (uint64_t)m->n_tiles > 0x7fffffffull) return fail(ctx, SRX_E_ARG, "%s: rows_per_block = %llu makes too many workgroups", who, (unsigned long long)rpb);
    auto moments = [&](auto kern, const auto* idxp, const auto* valp, double fa, double fb, unsigned long long* oa, unsigned long long* ob) -> int32_t {
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, grid, dim3(kAcThreads), lds, st, (const int64_t*)m->d_indptr, (const int64_t*)m->d_tile_ptr, idxp, valp, N, G,
                           m->n_tiles, m->tile_genes, rpb, (const long long*)d_dq, inv_w, fa, fb, oa, ob);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    auto walk = [&](auto kern, const auto* idxp, const auto* valp) -> int32_t {
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, grid, dim3(kAcThreads), lds, st, (const int64_t*)m->d_indptr, (const int64_t*)m->d_tile_ptr, idxp, valp, N, G,
                           m->n_tiles, m->tile_genes, rpb, c.ptr, c.ind, c.w, std::ldexp(1.0, info.s_cross), d_P);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    auto all = [&](const auto* idxp, const auto* valp) -> int32_t {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(valp)>>;
        using I = std::remove_cv_t<std::remove_pointer_t<decltype(idxp)>>;
        SRX_TRY(t_mom.start());
        SRX_TRY(t_sq.start());
        SRX_TRY(moments(k_ac_moments<T, I, false>, idxp, valp, std::ldexp(1.0, info.s_sum), std::ldexp(1.0, info.s_sumsq), d_S, d_Q));
        SRX_TRY(t_sq.stop(&info.ms_sum_sumsq));
        SRX_TRY(t_ab.start());
        SRX_TRY(moments(k_ac_moments<T, I, true>, idxp, valp, std::ldexp(1.0, info.s_dsum), std::ldexp(1.0, info.s_dsumsq), d_A, d_B));
        SRX_TRY(t_ab.stop(&info.ms_dsum_dsumsq));
        SRX_TRY(t_mom.stop(&info.ms_moments));
        SRX_TRY(t_walk.start());
        SRX_TRY(walk(k_ac_walk<T, I>, idxp, valp));
        return t_walk.stop(&info.ms_walk);
    };
    auto by_idx = [&](const auto* valp) -> int32_t {
        return m->d_idx16 ? all((const uint16_t*)m->d_idx16, valp) : all((const int32_t*)m->d_indices, valp);
    };
    if (m->nnz && G) SRX_TRY(is_f32(m) ? by_idx((const float*)m->d_values) : by_idx((const double*)m->d_values));
    info.ms = info.ms_graph + info.ms_moments + info.ms_walk;

    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    info.s2_int = (int64_t)small[AC_S2];
    std::vector<long long> tab(5 * Gp);
    SRX_TRY(d2h(ctx, tab.data(), d_tab, 5 * Gp * 8));
    const long long *S = tab.data(), *Q = S + Gp, *A = S + 2 * Gp, *B = S + 3 * Gp, *P = S + 4 * Gp;
    if (out) {
        if (out->sum_int) std::copy(S, S + G, (long long*)out->sum_int);
        if (out->sumsq_int) std::copy(Q, Q + G, (long long*)out->sumsq_int);
        if (out->dsum_int) std::copy(A, A + G, (long long*)out->dsum_int);
        if (out->dsumsq_int) std::copy(B, B + G, (long long*)out->dsumsq_int);
        if (out->cross_int) std::copy(P, P + G, (long long*)out->cross_int);
    }
    ac_finish(S, Q, A, B, P, G, out, &info);
    if (info_out) *info_out = info;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_autocorr(srx_mat* m, srx_graph* g, const srx_autocorr_opts* opts, srx_autocorr_out* out, srx_autocorr_info* info) {
    if (!m) return fail(nullptr, SRX_E_ARG, "srx_autocorr: null matrix");
    if (!g) return fail(m->ctx, SRX_E_ARG, "srx_autocorr: null graph");
    if (g->ctx != m->ctx) return fail(m->ctx, SRX_E_ARG, "srx_autocorr: the matrix and the graph belong to different contexts");
    SRX_TRY(ac_check(m, g->n, "srx_autocorr"));
    return ac_run(m, connectivities(g), "srx_autocorr", opts, out, info);
}

int32_t srx_autocorr_csr(srx_mat* m, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                         const srx_autocorr_opts* opts, srx_autocorr_out* out, srx_autocorr_info* info) {
    SRX_TRY(ac_check(m, n, "srx_autocorr_csr"));
    SymCsr c;
    SRX_TRY(symcsr_to_device(m->ctx, "srx_autocorr_csr", indptr, indices, weights, n, &c));
    return ac_run(m, c, "srx_autocorr_csr", opts, out, info);
}

int32_t srx_autocorr_from_tables(const int64_t* sum_int, const int64_t* sumsq_int, const int64_t* dsum_int, const int64_t* dsumsq_int,
                                 const int64_t* cross_int, uint64_t n_genes, srx_autocorr_info* info, srx_autocorr_out* out) {
    if (!info) return fail(nullptr, SRX_E_ARG, "srx_autocorr_from_tables: null info");
    if (n_genes && (!sum_int || !sumsq_int || !dsum_int || !dsumsq_int || !cross_int))
        return fail(nullptr, SRX_E_ARG, "srx_autocorr_from_tables: null table");
    if (info->n < 2 || info->n >= 0xFFFFFFFFull)
        return fail(nullptr, SRX_E_ARG, "srx_autocorr_from_tables: N = %llu is outside 2 .. 2^32 - 2", (unsigned long long)info->n);
    if (info->w_int <= 0) return fail(nullptr, SRX_E_ARG, "srx_autocorr_from_tables: w_int is not positive (W = 0)");
    const int sh = 2 * info->s_sum - info->s_sumsq;
    if (sh < 0 || sh > 62) return fail(nullptr, SRX_E_ARG, "srx_autocorr_from_tables: 2 s_sum - s_sumsq = %d is outside 0 .. 62", sh);
    info->n_genes = n_genes;
    ac_finish((const long long*)sum_int, (const long long*)sumsq_int, (const long long*)dsum_int, (const long long*)dsumsq_int,
              (const long long*)cross_int, n_genes, out, info);
    return SRX_OK;
}

int32_t srx_autocorr_scales(srx_autocorr_info* info) {
    if (!info) return fail(nullptr, SRX_E_ARG, "srx_autocorr_scales: null info");
    return ac_scales(nullptr, "srx_autocorr_scales", info);
}

}  // extern "C"
