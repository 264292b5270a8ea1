// markers.hip — marker genes per group: per-(group, gene) moments of the stored values, Welch's t statistic of every group
// against the rest, and the ranking of every group's genes (srx_group_moments, srx_rank_genes_groups[_graph], srx_markers_*).
// The definition is in include/srx.h; the design and the LDS budget are in DESIGN.md ("Marker genes").
//
// A (group, gene) accumulator table does not fit the LDS (n_groups x 10000 genes x 16 B), so the accumulators stay per gene
// and the ROWS are sorted instead: a stable counting sort of the rows by label gives a permutation in which every group is one
// run; a workgroup takes one (gene tile, block of at most rows_per_block permuted rows of ONE group), walks those rows' tile
// segments through the permutation (the matrix's cached tile cuts and its 16-bit index mirror: no new pattern structure) and
// adds its tile to the group's row of the tables.  Every sum is a 64-bit fixed-point integer, in LDS and in the tables, so
// the flush is a global integer atomic per TOUCHED gene: order-free like the LDS adds, and a sparse group writes little.
// (Per-block partials summed by a reduce kernel, the per-gene pass's arrangement, would cost blocks x G x 16 B with at least
// one block per group and tile: 1.8 GB at 4096 groups x 28k genes, read back once more.)
// The counts take a pass of their own over the indices alone (as k_gene_count): 10000 genes x (16 + 4) B exceed the LDS.
#include "graph_handle.hpp"
#include "markers_internal.hpp"
#include "scan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

// the statistics are evaluated in the order srx.h states them, every operation rounded once: no FMA contraction.  The pragma
// covers the code BELOW it only.  The runtime's __dmul_rn / __dsub_rn / __dadd_rn are plain operators in a header read before
// it, so their results stay contractable and `__dsub_rn(a, __dmul_rn(b, b))` becomes one v_fma_f64; the statistics therefore
// use the operators of this file (mk_mul, mk_sub, mk_add below), which the pragma does cover.
#pragma clang fp contract(off)

namespace srx {

constexpr int kMkThreads = 1024;          // one workgroup per CU: its accumulators fill the LDS
constexpr int kMkSortRows = 1024;         // rows per workgroup of the counting sort
constexpr uint64_t kMkMinRows = 64;       // rows_per_block = max(kMkMinRows, ceil(N / max(1, kMkBlocks / n_tiles)))
constexpr uint64_t kMkBlocks = 1024;      // ... four workgroups per CU of the 256 when one group holds every row

inline uint64_t mk_rows_per_block(uint64_t n_rows, int n_tiles) {
    const uint64_t want = std::max<uint64_t>(1, kMkBlocks / (uint64_t)std::max(n_tiles, 1));
    return std::max<uint64_t>(kMkMinRows, (n_rows + want - 1) / want);
}

// one f64 operation, rounded to nearest even, that never joins a neighbour in an FMA (compiled under the pragma above);
// f64 division and square root are correctly rounded as the compiler expands them
__device__ __forceinline__ double mk_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double mk_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double mk_add(double a, double b) { return a + b; }
__device__ __forceinline__ double mk_div(double a, double b) { return a / b; }

__global__ __launch_bounds__(256) void k_mk_label_max(const uint32_t* __restrict__ labels, uint64_t n, unsigned long long* __restrict__ small) {
    unsigned long long mx = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) mx = labels[i] > mx ? labels[i] : mx;
    mx = wave_max(mx);
    if (lane_id() == 0 && mx) atomicMax(&small[MK_MAXLABEL], mx);
}

// ---- the stable counting sort of the rows by label -------------------------------------------------------------------------
// Workgroup b takes the rows b * kMkSortRows ..: the histogram of their labels goes to table[g * n_blk + b] (group-major, so
// that ONE exclusive scan of the table gives every (group, workgroup) its first place in the permutation), and every row
// learns how many rows of its label precede it in the workgroup.  A label >= n_groups raises the flag and is not counted.
__global__ __launch_bounds__(kMkSortRows) void k_mk_label_count(const uint32_t* __restrict__ labels, uint64_t n, uint32_t n_groups,
                                                                uint64_t n_blk, int64_t* __restrict__ table, uint16_t* __restrict__ rank,
                                                                unsigned long long* __restrict__ small) {
    __shared__ uint32_t s_hist[SRX_GROUPS_MAX];
    __shared__ uint32_t s_lab[kMkSortRows];
    for (uint32_t g = threadIdx.x; g < n_groups; g += kMkSortRows) s_hist[g] = 0u;
    const uint64_t r = (uint64_t)blockIdx.x * kMkSortRows + threadIdx.x;
    uint32_t lab = 0xffffffffu;
    if (r < n) {
        lab = labels[r];
        if (lab >= n_groups) {
            atomicOr(&small[MK_FLAGS], kMkBadLabel);
            lab = 0xffffffffu;
        }
    }
    s_lab[threadIdx.x] = lab;
    __syncthreads();
    if (lab != 0xffffffffu) {
        atomicAdd(&s_hist[lab], 1u);
        uint32_t before = 0;
        for (uint32_t t = 0; t < threadIdx.x; ++t) before += s_lab[t] == lab ? 1u : 0u;
        rank[r] = (uint16_t)before;
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < n_groups; g += kMkSortRows) table[(uint64_t)g * n_blk + blockIdx.x] = (int64_t)s_hist[g];
}
// perm[first place of (label, workgroup) + rank in the workgroup] = row: within a group the rows keep their order
__global__ __launch_bounds__(kMkSortRows) void k_mk_place(const uint32_t* __restrict__ labels, const uint16_t* __restrict__ rank,
                                                          const int64_t* __restrict__ first, uint64_t n, uint64_t n_blk,
                                                          uint32_t* __restrict__ perm) {
    const uint64_t r = (uint64_t)blockIdx.x * kMkSortRows + threadIdx.x;
    if (r >= n) return;
    perm[first[(uint64_t)labels[r] * n_blk + blockIdx.x] + rank[r]] = (uint32_t)r;
}
__global__ void k_mk_sizes(const int64_t* __restrict__ first, uint32_t n_groups, uint64_t n_blk, uint64_t* __restrict__ sizes) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n_groups) sizes[g] = (uint64_t)(first[(uint64_t)(g + 1) * n_blk] - first[(uint64_t)g * n_blk]);
}

// ---- the walk: one workgroup = (gene tile, block of permuted rows of one group) -------------------------------------------
// COUNT: 32-bit counters per gene of the tile, the indices alone are read; else {S, Q} side by side per gene, 64-bit fixed
// point.  A wave takes two rows at a time; a lane takes 4 consecutive entries from the 4-entry boundary at or before the
// segment start (one 8- or 16-byte load of the indices, 16 or 2 x 16 bytes of values; entries outside [lo, hi) are masked —
// the arrays of a matrix are padded by 16 entries).
// CLIP (hvg_seurat.hip's second pass): min(x, clip[group][gene]) takes the place of x; the group's clip row is read where it lies
// (the accumulators fill the LDS, and the blocks of one group and tile share the row's slice in L2).
template <typename T, typename I, bool COUNT, bool CLIP = false>
__global__ __launch_bounds__(kMkThreads) void k_mk_walk(const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp,
                                                        const I* __restrict__ idx, const T* __restrict__ vals, uint64_t n_rows,
                                                        uint64_t n_cols, int n_tiles, int tile_genes,
                                                        const uint32_t* __restrict__ perm, const MkBlock* __restrict__ blocks,
                                                        double fx_sum, double fx_sq, unsigned long long* __restrict__ out_S,
                                                        unsigned long long* __restrict__ out_Q, uint32_t* __restrict__ out_C,
                                                        const double* __restrict__ clip) {
    extern __shared__ double lds[];
    unsigned long long* s_acc = reinterpret_cast<unsigned long long*>(lds);
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(lds);
    if constexpr (COUNT) {
        for (int g = threadIdx.x; g < tile_genes; g += kMkThreads) s_cnt[g] = 0u;
    } else {
        for (int g = threadIdx.x; g < 2 * tile_genes; g += kMkThreads) s_acc[g] = 0ull;
        // CLIP: one more word behind the accumulators, in the dynamic region (a static variable would shift its base)
        if constexpr (CLIP) {
            if (threadIdx.x == 0) s_acc[2 * tile_genes] = ~0ull;
        }
    }
    __syncthreads();
    const int tile = blockIdx.x % n_tiles;
    const MkBlock blk = blocks[blockIdx.x / n_tiles];
    const int32_t gbase = tile * tile_genes;
    // CLIP: the smallest clip of the group's row within this tile.  A value below it is below its own gene's clip too and skips
    // the gather from the table (8 bytes from a line of its own per entry: the walk is then bound by the gather rate, not by
    // bandwidth); min(x, clip) is the same bits either way.  Non-negative doubles order as their bit patterns.
    const double* const clip_row = CLIP ? clip + (uint64_t)blk.group * n_cols : nullptr;
    double clip_min = 0.0;
    if constexpr (CLIP) {
        unsigned long long* const s_clip_min = s_acc + 2 * tile_genes;       // (set to ~0 before the barrier above)
        unsigned long long mn = ~0ull;
        for (int g = threadIdx.x; g < tile_genes; g += kMkThreads) {
            const uint64_t gene = (uint64_t)gbase + g;
            if (gene < n_cols) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(clip_row[gene]);
                mn = b < mn ? b : mn;
            }
        }
        mn = wave_min(mn);
        if (lane_id() == 0) atomicMin(s_clip_min, mn);
        __syncthreads();
        clip_min = __longlong_as_double((long long)*s_clip_min);
    }
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    constexpr int kWaves = kMkThreads / kWave;
    constexpr int kR = 2;
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
        if constexpr (!COUNT) {
            if constexpr (sizeof(T) == 4) {
                const float4 t4 = *reinterpret_cast<const float4*>(vals + e0);
                c.v[0] = t4.x; c.v[1] = t4.y; c.v[2] = t4.z; c.v[3] = t4.w;
            } else {
                const double2 a2 = *reinterpret_cast<const double2*>(vals + e0);
                const double2 b2 = *reinterpret_cast<const double2*>(vals + e0 + 2);
                c.v[0] = a2.x; c.v[1] = a2.y; c.v[2] = b2.x; c.v[3] = b2.y;
            }
        }
    };
    auto add_chunk = [&](int64_t e0, int64_t lo, int64_t hi, const Chunk& c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (e0 + j >= lo && e0 + j < hi) {
                const int32_t g0 = c.g[j] - gbase;
                if constexpr (COUNT) {
                    __hip_atomic_fetch_add(&s_cnt[g0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    // round-to-nearest-even integers of x 2^s and (x x) 2^q: |.| < 2^62 by the choice of the scales (srx.h)
                    double x = (double)c.v[j];
                    if constexpr (CLIP) {
                        if (!(x < clip_min)) {
                            const double cl = clip_row[c.g[j]];
                            x = x < cl ? x : cl;
                        }
                    }
                    const long long is = (long long)__builtin_rint(mk_mul(x, fx_sum));
                    const long long iq = (long long)__builtin_rint(mk_mul(mk_mul(x, x), fx_sq));
                    __hip_atomic_fetch_add(&s_acc[2 * g0], (unsigned long long)is, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(&s_acc[2 * g0 + 1], (unsigned long long)iq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    };
    for (uint64_t p = (uint64_t)blk.p0 + wave; p < blk.p1; p += (uint64_t)kWaves * kR) {
        int64_t lo[kR], hi[kR];
        Chunk c[kR];
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const uint64_t pq = p + (uint64_t)q * kWaves;
            lo[q] = hi[q] = 0;
            if (pq < blk.p1) seg_bounds(indptr, tp, n_rows, n_tiles, tile, (uint64_t)perm[pq], lo[q], hi[q]);
        }
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const int64_t b0 = lo[q] & ~(int64_t)3, e0 = b0 + 4 * lane;
            load_chunk(e0 < hi[q] ? e0 : b0, c[q]);
        }
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const int64_t b0 = lo[q] & ~(int64_t)3, e0 = b0 + 4 * lane;
            if (e0 < hi[q]) add_chunk(e0, lo[q], hi[q], c[q]);
            for (int64_t e = e0 + 4 * kWave; e < hi[q]; e += 4 * kWave) {      // segments longer than 256 entries
                Chunk cc;
                load_chunk(e, cc);
                add_chunk(e, lo[q], hi[q], cc);
            }
        }
    }
    __syncthreads();
    // the tile joins the group's row of the tables: integer atomics (any order gives the same bits), touched genes only
    const uint64_t row = (uint64_t)blk.group * n_cols;
    for (int g = threadIdx.x; g < tile_genes; g += kMkThreads) {
        const uint64_t gene = (uint64_t)gbase + g;
        if (gene >= n_cols) continue;
        if constexpr (COUNT) {
            if (s_cnt[g]) atomicAdd(&out_C[row + gene], s_cnt[g]);
        } else {
            if (s_acc[2 * g]) atomicAdd(&out_S[row + gene], s_acc[2 * g]);
            if (s_acc[2 * g + 1]) atomicAdd(&out_Q[row + gene], s_acc[2 * g + 1]);
        }
    }
}

// totals over the groups, per gene (integers)
__global__ __launch_bounds__(256) void k_mk_totals(const long long* __restrict__ S, const long long* __restrict__ Q,
                                                   const uint32_t* __restrict__ Cn, uint32_t n_groups, uint64_t G,
                                                   long long* __restrict__ totS, long long* __restrict__ totQ, uint32_t* __restrict__ totC) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    long long s = 0, q = 0;
    uint32_t c = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        s += S[(uint64_t)g * G + j];
        q += Q[(uint64_t)g * G + j];
        c += Cn[(uint64_t)g * G + j];
    }
    totS[j] = s;
    totQ[j] = q;
    totC[j] = c;
}

// ---- the statistics of srx.h for one (group, gene), in the stated order -----------------------------------------------------
struct MkTables {
    const long long *S, *Q, *totS, *totQ;
    const uint32_t *C, *totC;
    const uint64_t* sizes;
    uint64_t G, N;
    double inv_sum, inv_sq;        // 2^-sum_scale_log2, 2^-sq_scale_log2
    int logged;
};
struct MkStat {
    double sum, sumsq, mean, var, mean_rest, var_rest, score, lfc, pct, pct_rest;
};
__device__ __forceinline__ void mk_side(double S, double Q, double c, uint64_t n, bool degenerate, double& mean, double& var, double& pct) {
    mean = var = pct = 0.0;
    if (n == 0) return;
    const double nd = (double)n;
    mean = mk_div(S, nd);
    pct = mk_div(c, nd);
    if (degenerate) return;
    const double v = mk_mul(mk_sub(mk_div(Q, nd), mk_mul(mean, mean)), mk_div(nd, mk_sub(nd, 1.0)));
    var = v > 0.0 ? v : 0.0;
}
__device__ __forceinline__ MkStat mk_stat(const MkTables& t, uint32_t g, uint64_t j) {
    const uint64_t at = (uint64_t)g * t.G + j;
    const long long S = t.S[at], Q = t.Q[at];
    const uint32_t c = t.C[at];
    const uint64_t ng = t.sizes[g], nr = t.N - ng;
    const bool degenerate = ng < 2 || nr < 2;
    MkStat o;
    o.sum = mk_mul((double)S, t.inv_sum);
    o.sumsq = mk_mul((double)Q, t.inv_sq);
    mk_side(o.sum, o.sumsq, (double)c, ng, degenerate, o.mean, o.var, o.pct);
    mk_side(mk_mul((double)(t.totS[j] - S), t.inv_sum), mk_mul((double)(t.totQ[j] - Q), t.inv_sq), (double)(t.totC[j] - c), nr,
            degenerate, o.mean_rest, o.var_rest, o.pct_rest);
    o.score = 0.0;
    if (!degenerate) {
        const double d = mk_add(mk_div(o.var, (double)ng), mk_div(o.var_rest, (double)nr));
        if (d > 0.0) o.score = mk_div(mk_sub(o.mean, o.mean_rest), __dsqrt_rn(d));
    }
    const double a = t.logged ? expm1(o.mean) : o.mean, b = t.logged ? expm1(o.mean_rest) : o.mean_rest;
    o.lfc = log2(mk_div(mk_add(a, 1e-9), mk_add(b, 1e-9)));
    return o;
}
// one table, groups g0 .. g0 + n_g - 1 (u64 for SRX_MARKERS_CNT, f64 otherwise)
__global__ __launch_bounds__(256) void k_mk_table(MkTables t, int which, uint32_t g0, uint32_t n_g, void* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_g * t.G) return;
    const uint32_t g = g0 + (uint32_t)(i / t.G);
    const uint64_t j = i % t.G;
    if (which == SRX_MARKERS_CNT) {
        reinterpret_cast<uint64_t*>(out)[i] = (uint64_t)t.C[(uint64_t)g * t.G + j];
        return;
    }
    const MkStat s = mk_stat(t, g, j);
    double v = 0.0;
    switch (which) {
        case SRX_MARKERS_SUM: v = s.sum; break;
        case SRX_MARKERS_SUMSQ: v = s.sumsq; break;
        case SRX_MARKERS_MEAN: v = s.mean; break;
        case SRX_MARKERS_VAR: v = s.var; break;
        case SRX_MARKERS_MEAN_REST: v = s.mean_rest; break;
        case SRX_MARKERS_VAR_REST: v = s.var_rest; break;
        case SRX_MARKERS_SCORE: v = s.score; break;
        case SRX_MARKERS_LFC: v = s.lfc; break;
        case SRX_MARKERS_PCT: v = s.pct; break;
        default: v = s.pct_rest; break;
    }
    reinterpret_cast<double*>(out)[i] = v;
}

// ---- ranking: the place of every gene of a group under (score desc, index asc) by counting, as select.hip's k_hvg_rank with a
// group dimension.  Block (x, y): genes 256 x .. of group g0 + y against ALL genes of the group, kMkRankTile scores staged in
// LDS at a time; a gene whose place is below n_top writes itself there.  `score`: the groups g0 .. of this launch, n_g x G.
constexpr int kMkRankTile = 2048;
__global__ __launch_bounds__(256) void k_mk_rank(const double* __restrict__ score, uint32_t G, uint32_t g0, uint32_t n_top,
                                                 uint32_t* __restrict__ top_gene, double* __restrict__ top_score) {
    __shared__ double tile[kMkRankTile];
    const double* sc = score + (uint64_t)blockIdx.y * G;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    const double mine = j < G ? sc[j] : 0.0;
    uint32_t rank = 0;
    for (uint32_t base = 0; base < G; base += kMkRankTile) {
        for (uint32_t e = threadIdx.x; e < kMkRankTile; e += 256) tile[e] = base + e < G ? sc[base + e] : -INFINITY;
        __syncthreads();
        if (base + kMkRankTile - 1 < blockIdx.x * 256) {             // every gene of the tile precedes the block's: ties are theirs
#pragma unroll 8
            for (int e = 0; e < kMkRankTile; ++e) rank += tile[e] >= mine ? 1u : 0u;
        } else if (base > blockIdx.x * 256 + 255) {
#pragma unroll 8
            for (int e = 0; e < kMkRankTile; ++e) rank += tile[e] > mine ? 1u : 0u;
        } else {
#pragma unroll 4
            for (int e = 0; e < kMkRankTile; ++e) {
                const double o = tile[e];
                rank += (o > mine || (o == mine && base + e < j)) ? 1u : 0u;
            }
        }
        __syncthreads();
    }
    if (j < G && rank < n_top) {
        const uint64_t at = (uint64_t)(g0 + blockIdx.y) * n_top + rank;
        top_gene[at] = j;
        top_score[at] = mine;
    }
}
__global__ __launch_bounds__(256) void k_mk_top_lfc(MkTables t, uint32_t n_groups, uint32_t n_top, const uint32_t* __restrict__ top_gene,
                                                    double* __restrict__ top_lfc) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_groups * n_top) return;
    top_lfc[i] = mk_stat(t, (uint32_t)(i / n_top), top_gene[i]).lfc;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static MkTables mk_tables(const srx_markers* mk) {
    MkTables t;
    t.S = mk->d_S; t.Q = mk->d_Q; t.totS = mk->d_totS; t.totQ = mk->d_totQ;
    t.C = mk->d_C; t.totC = mk->d_totC;
    t.sizes = mk->d_sizes;
    t.G = mk->n_cols; t.N = mk->n_rows;
    t.inv_sum = std::ldexp(1.0, -mk->info.sum_scale_log2);
    t.inv_sq = std::ldexp(1.0, -mk->info.sq_scale_log2);
    t.logged = mk->logged;
    return t;
}

void mk_free(srx_markers* mk) {
    if (!mk) return;
    if (mk->d_block) {
        (void)hipSetDevice(mk->ctx->device);
        (void)hipStreamSynchronize(mk->ctx->stream);
        (void)hipFree(mk->d_block);
    }
    if (mk->d_wx) {
        (void)hipSetDevice(mk->ctx->device);
        (void)hipStreamSynchronize(mk->ctx->stream);
        (void)hipFree(mk->d_wx);
    }
    delete mk;
}

struct MkEvents {
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~MkEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// the tables stay below this many bytes per launch of k_mk_table / k_mk_rank (scratch "mk_table")
constexpr uint64_t kMkChunkBytes = 64ull << 20;
static uint32_t mk_chunk_groups(const srx_markers* mk) {
    const uint64_t per = at_least_one(mk->n_cols) * 8;
    return (uint32_t)std::min<uint64_t>(mk->n_groups, std::max<uint64_t>(1, kMkChunkBytes / per));
}

#include "wilcoxon.inl"

// ---- the counting sort as the walks over label-sorted rows call it (markers_internal.hpp) -----------------------------------
int32_t label_sort_count(srx_ctx* ctx, const uint32_t* d_labels, uint64_t N, uint32_t n_groups, unsigned long long* d_small, uint64_t* d_sizes,
                         LabelSort* s) {
    hipStream_t st = ctx->stream;
    const uint64_t n_blk = at_least_one((N + kMkSortRows - 1) / kMkSortRows);
    const uint64_t n_tab = (uint64_t)n_groups * n_blk;
    int64_t *d_table, *d_first;
    uint16_t* d_rank;
    uint32_t* d_perm;
    SRX_TRY(scratch(ctx, "mk_table_cnt", n_tab * 8, (void**)&d_table));
    SRX_TRY(scratch(ctx, "mk_table_first", (n_tab + 1) * 8, (void**)&d_first));
    SRX_TRY(scratch(ctx, "mk_rank", at_least_one(N) * 2, (void**)&d_rank));
    SRX_TRY(scratch(ctx, "mk_perm", at_least_one(N) * 4, (void**)&d_perm));
    hipLaunchKernelGGL(k_mk_label_count, dim3((unsigned)n_blk), dim3(kMkSortRows), 0, st, d_labels, N, n_groups, n_blk, d_table, d_rank, d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(scan_exclusive(ctx, d_table, n_tab, d_first, nullptr));
    hipLaunchKernelGGL(k_mk_sizes, dim3((n_groups + 255) / 256), dim3(256), 0, st, (const int64_t*)d_first, n_groups, n_blk, d_sizes);
    SRX_HIP(ctx, hipGetLastError());
    *s = LabelSort{d_perm, d_first, d_rank, N, n_blk};
    return SRX_OK;
}
int32_t label_sort_place(srx_ctx* ctx, const uint32_t* d_labels, const LabelSort& s) {
    if (s.n) hipLaunchKernelGGL(k_mk_place, dim3((unsigned)s.n_blk), dim3(kMkSortRows), 0, ctx->stream, d_labels, (const uint16_t*)s.d_rank,
                                (const int64_t*)s.d_first, s.n, s.n_blk, s.d_perm);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}
std::vector<MkBlock> label_blocks(const std::vector<uint64_t>& sizes, uint64_t rows_per_block) {
    std::vector<MkBlock> blocks;
    uint64_t at = 0;
    for (uint32_t g = 0; g < (uint32_t)sizes.size(); ++g) {
        for (uint64_t p = 0; p < sizes[g]; p += rows_per_block)
            blocks.push_back(MkBlock{(uint32_t)(at + p), (uint32_t)(at + std::min(p + rows_per_block, sizes[g])), g, 0u});
        at += sizes[g];
    }
    return blocks;
}

// The walk's launches: every (gene tile, block) pair, by value storage and index form.  d_clip null: S, Q and, unless d_C is
// null, the counts C (a second launch over the indices alone); else the clipped sums alone.
static int32_t mk_walk(srx_mat* m, const uint32_t* d_perm, const MkBlock* d_blocks, size_t n_blocks, double fx_sum, double fx_sq,
                       const double* d_clip, unsigned long long* d_S, unsigned long long* d_Q, uint32_t* d_C) {
    srx_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const dim3 grid((unsigned)(n_blocks * (size_t)m->n_tiles));
    auto launch = [&](auto kern, size_t lds, const auto* idxp, const auto* valp) -> int32_t {
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, grid, dim3(kMkThreads), lds, st, (const int64_t*)m->d_indptr, (const int64_t*)m->d_tile_ptr, idxp, valp, m->n_rows,
                           m->n_cols, m->n_tiles, m->tile_genes, d_perm, d_blocks, fx_sum, fx_sq, d_S, d_Q, d_C, d_clip);
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    auto both = [&](const auto* idxp, const auto* valp) -> int32_t {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(valp)>>;
        using I = std::remove_cv_t<std::remove_pointer_t<decltype(idxp)>>;
        if (d_clip) return launch(k_mk_walk<T, I, false, true>, (size_t)m->tile_genes * 16 + 16, idxp, valp);      // (+ the smallest clip)
        SRX_TRY(launch(k_mk_walk<T, I, false>, (size_t)m->tile_genes * 16, idxp, valp));
        if (!d_C) return SRX_OK;                   // (a caller that reads no counts: hvg_seurat.hip)
        return launch(k_mk_walk<float, I, true>, (size_t)m->tile_genes * 4, idxp, (const float*)nullptr);      // (the indices alone)
    };
    auto by_idx = [&](const auto* valp) -> int32_t {
        return m->d_idx16 ? both((const uint16_t*)m->d_idx16, valp) : both((const int32_t*)m->d_indices, valp);
    };
    return is_f32(m) ? by_idx((const float*)m->d_values) : by_idx((const double*)m->d_values);
}

// The whole call.  d_labels: n_rows u32 on the device (n_groups known: every label is validated against it).  want_rank false:
// the moments alone (srx_group_moments).  wx: the rank-sum route (its scores are ranked in place of Welch's t).
static int32_t markers_run(srx_mat* m, const uint32_t* d_labels, uint32_t n_groups, const srx_rank_genes_opts* opts, bool want_rank,
                           srx_markers** out, const WxOpts* wx = nullptr, MkPlan* plan = nullptr, bool want_counts = true) {
    srx_ctx* ctx = m->ctx;
    const uint64_t N = m->n_rows, G = m->n_cols;
    uint32_t n_top = 0;
    int logged = 1;
    if (want_rank) {
        const int32_t nt = opts ? opts->n_top : 0;
        if (nt < 0 || (uint64_t)nt > G) return fail(ctx, SRX_E_ARG, "rank_genes_groups: n_top = %d is outside 0 .. n_cols = %llu", nt, (unsigned long long)G);
        n_top = nt ? (uint32_t)nt : (uint32_t)std::min<uint64_t>(100, G);
        logged = !opts || opts->logged != 0;
    }
    Range rg("markers");
    SRX_TRY(ensure_tiles(m));                     // pattern-only: tile cuts and the 16-bit index mirror (cached on the handle)
    MkEvents ev;
    for (hipEvent_t& e : ev.e) SRX_HIP(ctx, hipEventCreate(&e));
    hipStream_t st = ctx->stream;

    srx_markers* mk = new srx_markers();
    struct Guard {
        srx_markers* p;
        ~Guard() { mk_free(p); }
    } guard{mk};
    mk->ctx = ctx;
    mk->n_rows = N; mk->n_cols = G; mk->n_groups = n_groups; mk->n_top = n_top; mk->logged = logged;
    {
        const uint64_t cells = (uint64_t)n_groups * at_least_one(G), tops = (uint64_t)n_groups * at_least_one(n_top);
        size_t off = 0;
        auto carve = [&](size_t bytes) { const size_t at = off; off += up256(bytes); return at; };
        const size_t oS = carve(cells * 8), oQ = carve(cells * 8), otS = carve(at_least_one(G) * 8), otQ = carve(at_least_one(G) * 8),
                     osz = carve((size_t)n_groups * 8), ots = carve(tops * 8), otl = carve(tops * 8), oC = carve(cells * 4),
                     otC = carve(at_least_one(G) * 4), otg = carve(tops * 4);
        hipError_t e = dev_malloc(ctx, &mk->d_block, off);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            mk->d_block = nullptr;
            return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "markers: the %u x %llu tables (%zu bytes) do not fit: %s", n_groups,
                        (unsigned long long)G, off, hipGetErrorString(e));
        }
        char* b = (char*)mk->d_block;
        mk->d_S = (long long*)(b + oS); mk->d_Q = (long long*)(b + oQ);
        mk->d_totS = (long long*)(b + otS); mk->d_totQ = (long long*)(b + otQ);
        mk->d_sizes = (uint64_t*)(b + osz);
        mk->d_top_score = (double*)(b + ots); mk->d_top_lfc = (double*)(b + otl);
        mk->d_C = (uint32_t*)(b + oC); mk->d_totC = (uint32_t*)(b + otC); mk->d_top_gene = (uint32_t*)(b + otg);
        SRX_HIP(ctx, hipMemsetAsync(mk->d_block, 0, off, st));
    }

    // -- stage 1: max |x| and non-finite values; labels validated, counted and sorted
    SRX_HIP(ctx, hipEventRecord(ev.e[0], st));
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "mk_small", MK_WORDS * 8, (void**)&d_small));
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, MK_WORDS * 8, st));
    value_scan(m, d_small);
    LabelSort sort;
    SRX_TRY(label_sort_count(ctx, d_labels, N, n_groups, d_small, mk->d_sizes, &sort));
    unsigned long long small[MK_WORDS];
    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    if (small[MK_FLAGS] & kMkBadLabel) return fail(ctx, SRX_E_ARG, "markers: a label is not below n_groups = %u", n_groups);
    if (small[MK_FLAGS] & kValNonFinite) return fail(ctx, SRX_E_NAN, "markers: a stored value is NaN or Inf");
    std::vector<uint64_t> sizes(n_groups);
    SRX_TRY(d2h(ctx, sizes.data(), mk->d_sizes, (size_t)n_groups * 8));
    SRX_TRY(label_sort_place(ctx, d_labels, sort));
    const uint32_t* d_perm = sort.d_perm;

    // the scales (srx.h): e from max_abs, no lower than -30; L = ceil(log2(max(N, 1)))
    double max_abs;
    memcpy(&max_abs, &small[MK_MAXABS], 8);
    const int e = fx_exponent(max_abs);
    int L = 0;
    while ((1ull << L) < at_least_one(N)) ++L;
    srx_markers_info& info = mk->info;
    info.n_rows = N; info.n_cols = G; info.n_groups = n_groups; info.n_top = n_top;
    info.sum_scale_log2 = 62 - e - L;
    info.sq_scale_log2 = 62 - 2 * e - L;
    info.max_abs = max_abs;
    for (uint64_t s : sizes) info.groups_degenerate += (wx ? (s == 0 || N - s == 0) : (s < 2 || N - s < 2)) ? 1u : 0u;

    // the blocks: at most rows_per_block consecutive places of ONE group each
    const uint64_t rpb = mk_rows_per_block(N, m->n_tiles);
    const std::vector<MkBlock> blocks = label_blocks(sizes, rpb);
    SRX_HIP(ctx, hipEventRecord(ev.e[1], st));

    // -- stage 2: the grouped moments and counts, the totals
    MkBlock* d_blocks = nullptr;
    const double fx_sum = std::ldexp(1.0, info.sum_scale_log2), fx_sq = std::ldexp(1.0, info.sq_scale_log2);
    if (!blocks.empty() && m->nnz && G) {
        SRX_TRY(scratch(ctx, "mk_blocks", blocks.size() * sizeof(MkBlock), (void**)&d_blocks));
        SRX_TRY(h2d(ctx, d_blocks, blocks.data(), blocks.size() * sizeof(MkBlock)));
        SRX_TRY(mk_walk(m, d_perm, d_blocks, blocks.size(), fx_sum, fx_sq, nullptr, (unsigned long long*)mk->d_S, (unsigned long long*)mk->d_Q,
                        want_counts ? mk->d_C : nullptr));
    }
    if (plan) {
        plan->d_perm = d_perm;
        plan->d_blocks = d_blocks;
        plan->n_blocks = d_blocks ? blocks.size() : 0;
        plan->fx_sum = fx_sum;
        plan->fx_sq = fx_sq;
        plan->sizes = sizes;
    }
    if (G) hipLaunchKernelGGL(k_mk_totals, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, st, (const long long*)mk->d_S, (const long long*)mk->d_Q,
                              (const uint32_t*)mk->d_C, n_groups, G, mk->d_totS, mk->d_totQ, mk->d_totC);
    SRX_HIP(ctx, hipGetLastError());
    SRX_HIP(ctx, hipEventRecord(ev.e[2], st));
    if (wx) {
        mk->wilcoxon = true;
        SRX_TRY(wilcoxon_run(m, d_labels, mk, *wx));
        SRX_HIP(ctx, hipEventRecord(ev.e[5], st));        // (the three stages keep their own times: winfo)
    }
    hipEvent_t ev_stat = wx ? ev.e[5] : ev.e[2];

    // -- stages 3 and 4: the scores of a chunk of groups, then their ranking
    float ms_stat = 0.f, ms_rank = 0.f;
    if (want_rank && G && n_top) {
        const MkTables t = mk_tables(mk);
        const uint32_t per = mk_chunk_groups(mk);
        double* d_score;
        SRX_TRY(scratch(ctx, "mk_table", (uint64_t)per * G * 8, (void**)&d_score));
        hipEvent_t a = ev.e[3], b = ev.e[4];
        for (uint32_t g0 = 0; g0 < n_groups; g0 += per) {
            const uint32_t ng = std::min(per, n_groups - g0);
            const uint64_t cells = (uint64_t)ng * G;
            if (wx) hipLaunchKernelGGL(k_wx_table, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, wx_tables(mk), (int)SRX_MARKERS_SCORE, g0, ng, (void*)d_score);
            else hipLaunchKernelGGL(k_mk_table, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, t, (int)SRX_MARKERS_SCORE, g0, ng, (void*)d_score);
            SRX_HIP(ctx, hipGetLastError());
            if (n_groups <= per) SRX_HIP(ctx, hipEventRecord(a, st));
            hipLaunchKernelGGL(k_mk_rank, dim3((unsigned)((G + 255) / 256), ng), dim3(256), 0, st, (const double*)d_score, (uint32_t)G, g0, n_top,
                               mk->d_top_gene, mk->d_top_score);
            SRX_HIP(ctx, hipGetLastError());
        }
        const uint64_t tops = (uint64_t)n_groups * n_top;
        hipLaunchKernelGGL(k_mk_top_lfc, dim3((unsigned)((tops + 255) / 256)), dim3(256), 0, st, t, n_groups, n_top, (const uint32_t*)mk->d_top_gene,
                           mk->d_top_lfc);
        SRX_HIP(ctx, hipGetLastError());
        SRX_HIP(ctx, hipEventRecord(b, st));
        SRX_HIP(ctx, hipEventSynchronize(b));
        if (n_groups <= per) {                    // (several chunks interleave the two stages: their sum is reported as ranking)
            SRX_HIP(ctx, hipEventElapsedTime(&ms_stat, ev_stat, a));
            SRX_HIP(ctx, hipEventElapsedTime(&ms_rank, a, b));
        } else {
            SRX_HIP(ctx, hipEventElapsedTime(&ms_rank, ev_stat, b));
        }
    }
    SRX_HIP(ctx, hipEventSynchronize(ev.e[2]));
    float ms_prep = 0.f, ms_mom = 0.f;
    SRX_HIP(ctx, hipEventElapsedTime(&ms_prep, ev.e[0], ev.e[1]));
    SRX_HIP(ctx, hipEventElapsedTime(&ms_mom, ev.e[1], ev.e[2]));
    info.ms = (double)ms_prep + (double)ms_mom + (double)ms_stat + (double)ms_rank;
    if (wx) info.ms += mk->winfo.ms_stage + mk->winfo.ms_sort + mk->winfo.ms_ranks;
    if (getenv("SRX_MARKERS_TRACE"))
        fprintf(stderr, "srx markers: groups %u blocks %zu prepare %.3f moments %.3f statistics %.3f ranking %.3f ms\n", n_groups, blocks.size(),
                ms_prep, ms_mom, ms_stat, ms_rank);
    if (wx && getenv("SRX_MARKERS_TRACE"))
        fprintf(stderr, "srx markers: wilcoxon chunks %u stage %.3f sort %.3f ranks %.3f ms (short %llu long %llu segments)\n", mk->winfo.n_chunks,
                mk->winfo.ms_stage, mk->winfo.ms_sort, mk->winfo.ms_ranks, (unsigned long long)mk->winfo.segments_short,
                (unsigned long long)mk->winfo.segments_long);
    guard.p = nullptr;
    *out = mk;
    return SRX_OK;
}

// one table to the host, a chunk of groups at a time through the scratch buffer
static int32_t markers_fetch_table(srx_markers* mk, int32_t which, void* out) {
    srx_ctx* ctx = mk->ctx;
    const uint64_t G = mk->n_cols;
    if (!G) return SRX_OK;
    const MkTables t = mk_tables(mk);
    const uint32_t per = mk_chunk_groups(mk);
    void* d_tab;
    SRX_TRY(scratch(ctx, "mk_table", (uint64_t)per * G * 8, &d_tab));
    for (uint32_t g0 = 0; g0 < mk->n_groups; g0 += per) {
        const uint32_t ng = std::min(per, mk->n_groups - g0);
        const uint64_t cells = (uint64_t)ng * G;
        if (mk->wilcoxon && (which == SRX_MARKERS_SCORE || which == SRX_MARKERS_RANKSUM2))
            hipLaunchKernelGGL(k_wx_table, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, wx_tables(mk), (int)which, g0, ng, d_tab);
        else hipLaunchKernelGGL(k_mk_table, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream, t, (int)which, g0, ng, d_tab);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(d2h(ctx, (char*)out + (uint64_t)g0 * G * 8, d_tab, cells * 8));
    }
    return SRX_OK;
}

int32_t markers_moments(srx_mat* m, const uint32_t* d_labels, uint32_t n_groups, bool want_counts, srx_markers** out, MkPlan* plan) {
    return markers_run(m, d_labels, n_groups, nullptr, false, out, nullptr, plan, want_counts);
}

int32_t markers_clipped_walk(srx_mat* m, const MkPlan& plan, const double* d_clip, unsigned long long* d_S, unsigned long long* d_Q) {
    if (!plan.n_blocks) return SRX_OK;
    return mk_walk(m, plan.d_perm, plan.d_blocks, plan.n_blocks, plan.fx_sum, plan.fx_sq, d_clip, d_S, d_Q, nullptr);
}

int32_t markers_check(srx_mat* m, const char* what) {
    if (!m) return fail(nullptr, SRX_E_ARG, "%s: null matrix", what);
    srx_ctx* ctx = m->ctx;
    if (m->csc) return fail(ctx, SRX_E_ARG, "%s walks cells: convert the CSC matrix with srx_matrix_to_csr", what);
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "%s: rows are sharded; the labels of a clustering live on one rank", what);
    if (m->n_rows >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "%s: 2^32 - 1 rows or more", what);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return SRX_OK;
}

int32_t host_labels(srx_ctx* ctx, uint64_t n, const uint32_t* labels, uint32_t n_groups, const char* what, uint32_t** d_labels) {
    if (n_groups < 1 || n_groups > SRX_GROUPS_MAX) return fail(ctx, SRX_E_ARG, "%s: n_groups = %u is outside 1 .. %d", what, n_groups, SRX_GROUPS_MAX);
    if (n && !labels) return fail(ctx, SRX_E_ARG, "%s: null labels", what);
    SRX_TRY(scratch(ctx, "mk_labels", at_least_one(n) * 4, (void**)d_labels));
    return h2d(ctx, *d_labels, labels, n * 4);
}
int32_t markers_host_labels(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const char* what, uint32_t** d_labels) {
    return host_labels(m->ctx, m->n_rows, labels, n_groups, what, d_labels);
}

int32_t label_max(srx_ctx* ctx, const uint32_t* d_labels, uint64_t n, uint64_t* mx_out) {
    unsigned long long* d_small;
    SRX_TRY(scratch(ctx, "mk_small", MK_WORDS * 8, (void**)&d_small));
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, MK_WORDS * 8, ctx->stream));
    const unsigned grid = (unsigned)std::min<uint64_t>((at_least_one(n) + 255) / 256, (uint64_t)ctx->n_cus * 4);
    hipLaunchKernelGGL(k_mk_label_max, dim3(grid), dim3(256), 0, ctx->stream, d_labels, n, d_small);
    SRX_HIP(ctx, hipGetLastError());
    unsigned long long mx = 0;
    SRX_TRY(d2h(ctx, &mx, d_small + MK_MAXLABEL, 8));
    *mx_out = mx;
    return SRX_OK;
}

// the labels the last srx_louvain left on g: the handle checked against m, n_groups = the largest label + 1
static int32_t markers_graph_labels(srx_mat* m, srx_graph* g, const char* what, uint32_t* n_groups) {
    srx_ctx* ctx = m->ctx;
    if (!g) return fail(ctx, SRX_E_ARG, "%s: null graph", what);
    if (g->ctx != ctx) return fail(ctx, SRX_E_ARG, "%s: the matrix and the graph belong to different contexts", what);
    if (!g->labels_valid) return fail(ctx, SRX_E_ARG, "%s: no srx_louvain has run on this graph", what);
    if (g->n != m->n_rows)
        return fail(ctx, SRX_E_ARG, "%s: the graph has %llu cells, the matrix %llu rows", what, (unsigned long long)g->n, (unsigned long long)m->n_rows);
    if (!g->n) return fail(ctx, SRX_E_ARG, "%s: no cells, hence no groups", what);
    uint64_t mx = 0;
    SRX_TRY(label_max(ctx, g->d_labels, g->n, &mx));
    if (mx >= SRX_GROUPS_MAX) return fail(ctx, SRX_E_ARG, "%s: %llu communities, more than %d groups", what, (unsigned long long)(mx + 1), SRX_GROUPS_MAX);
    *n_groups = (uint32_t)mx + 1;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_group_moments(srx_mat* m, const uint32_t* labels, uint32_t n_groups, uint64_t* n_cells_out, uint64_t* cnt_out, double* sum_out,
                          double* sumsq_out) {
    SRX_TRY(markers_check(m, "srx_group_moments"));
    uint32_t* d_labels;
    SRX_TRY(markers_host_labels(m, labels, n_groups, "srx_group_moments", &d_labels));
    srx_markers* mk = nullptr;
    SRX_TRY(markers_run(m, d_labels, n_groups, nullptr, false, &mk));
    int32_t rc = SRX_OK;
    if (n_cells_out) rc = d2h(m->ctx, n_cells_out, mk->d_sizes, (size_t)n_groups * 8);
    if (rc == SRX_OK && cnt_out) rc = markers_fetch_table(mk, SRX_MARKERS_CNT, cnt_out);
    if (rc == SRX_OK && sum_out) rc = markers_fetch_table(mk, SRX_MARKERS_SUM, sum_out);
    if (rc == SRX_OK && sumsq_out) rc = markers_fetch_table(mk, SRX_MARKERS_SUMSQ, sumsq_out);
    mk_free(mk);
    return rc;
}

int32_t srx_rank_genes_groups(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const srx_rank_genes_opts* opts, srx_markers** out) {
    SRX_TRY(markers_check(m, "srx_rank_genes_groups"));
    if (!out) return fail(m->ctx, SRX_E_ARG, "srx_rank_genes_groups: null output");
    uint32_t* d_labels;
    SRX_TRY(markers_host_labels(m, labels, n_groups, "srx_rank_genes_groups", &d_labels));
    return markers_run(m, d_labels, n_groups, opts, true, out);
}

int32_t srx_rank_genes_groups_graph(srx_mat* m, srx_graph* g, const srx_rank_genes_opts* opts, srx_markers** out) {
    SRX_TRY(markers_check(m, "srx_rank_genes_groups_graph"));
    if (!out) return fail(m->ctx, SRX_E_ARG, "srx_rank_genes_groups_graph: null output");
    uint32_t n_groups = 0;
    SRX_TRY(markers_graph_labels(m, g, "srx_rank_genes_groups_graph", &n_groups));
    return markers_run(m, g->d_labels, n_groups, opts, true, out);
}

// the rank-sum route's own refusals and options: N below 2^31 (the doubled rank sums stay below 2^63), with the tie term N at
// most 2^21 (N^3 - N fits 64 bits)
static int32_t wilcoxon_begin(srx_mat* m, const srx_wilcoxon_opts* opts, const char* what, srx_rank_genes_opts* ro, WxOpts* wx) {
    ro->n_top = opts ? opts->n_top : 0;
    ro->logged = opts ? opts->logged : -1;
    wx->tie_correct = opts && opts->tie_correct;
    wx->scratch_bytes = opts ? opts->scratch_bytes : 0;
    if (m->n_rows >= (1ull << 31)) return fail(m->ctx, SRX_E_ARG, "%s: 2^31 rows or more: the doubled rank sums would pass 2^63", what);
    if (wx->tie_correct && m->n_rows > (1ull << 21))
        return fail(m->ctx, SRX_E_ARG, "%s: tie_correct with more than 2^21 rows (%llu): N^3 - N would pass 64 bits", what, (unsigned long long)m->n_rows);
    return SRX_OK;
}

int32_t srx_rank_genes_wilcoxon(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const srx_wilcoxon_opts* opts, srx_markers** out) {
    SRX_TRY(markers_check(m, "srx_rank_genes_wilcoxon"));
    if (!out) return fail(m->ctx, SRX_E_ARG, "srx_rank_genes_wilcoxon: null output");
    srx_rank_genes_opts ro;
    WxOpts wx;
    SRX_TRY(wilcoxon_begin(m, opts, "srx_rank_genes_wilcoxon", &ro, &wx));
    uint32_t* d_labels;
    SRX_TRY(markers_host_labels(m, labels, n_groups, "srx_rank_genes_wilcoxon", &d_labels));
    return markers_run(m, d_labels, n_groups, &ro, true, out, &wx);
}

int32_t srx_rank_genes_wilcoxon_graph(srx_mat* m, srx_graph* g, const srx_wilcoxon_opts* opts, srx_markers** out) {
    SRX_TRY(markers_check(m, "srx_rank_genes_wilcoxon_graph"));
    if (!out) return fail(m->ctx, SRX_E_ARG, "srx_rank_genes_wilcoxon_graph: null output");
    srx_rank_genes_opts ro;
    WxOpts wx;
    SRX_TRY(wilcoxon_begin(m, opts, "srx_rank_genes_wilcoxon_graph", &ro, &wx));
    uint32_t n_groups = 0;
    SRX_TRY(markers_graph_labels(m, g, "srx_rank_genes_wilcoxon_graph", &n_groups));
    return markers_run(m, g->d_labels, n_groups, &ro, true, out, &wx);
}

int32_t srx_markers_wilcoxon_info_get(const srx_markers* mk, srx_wilcoxon_info* info) {
    if (!mk || !info) return fail(mk ? mk->ctx : nullptr, SRX_E_ARG, "srx_markers_wilcoxon_info_get: null argument");
    if (!mk->wilcoxon) return fail(mk->ctx, SRX_E_ARG, "srx_markers_wilcoxon_info_get: this handle is a t-test's, not srx_rank_genes_wilcoxon's");
    *info = mk->winfo;
    return SRX_OK;
}

int32_t srx_markers_fetch_ties(srx_markers* mk, uint64_t* out) {
    if (!mk || !out) return fail(mk ? mk->ctx : nullptr, SRX_E_ARG, "srx_markers_fetch_ties: null argument");
    if (!mk->wilcoxon || !mk->winfo.tie_correct)
        return fail(mk->ctx, SRX_E_ARG, "srx_markers_fetch_ties: the tie terms exist on a handle of srx_rank_genes_wilcoxon made with tie_correct only");
    SRX_HIP(mk->ctx, hipSetDevice(mk->ctx->device));
    return d2h(mk->ctx, out, mk->d_T, (size_t)mk->n_cols * 8);
}

int32_t srx_markers_info_get(const srx_markers* mk, srx_markers_info* info) {
    if (!mk || !info) return fail(mk ? mk->ctx : nullptr, SRX_E_ARG, "srx_markers_info_get: null argument");
    *info = mk->info;
    return SRX_OK;
}

int32_t srx_markers_fetch_top(srx_markers* mk, uint32_t* genes_out, double* scores_out, double* lfc_out) {
    if (!mk) return fail(nullptr, SRX_E_ARG, "srx_markers_fetch_top: null handle");
    srx_ctx* ctx = mk->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n = (size_t)mk->n_groups * mk->n_top;
    if (genes_out) SRX_TRY(d2h(ctx, genes_out, mk->d_top_gene, n * 4));
    if (scores_out) SRX_TRY(d2h(ctx, scores_out, mk->d_top_score, n * 8));
    if (lfc_out) SRX_TRY(d2h(ctx, lfc_out, mk->d_top_lfc, n * 8));
    return SRX_OK;
}

int32_t srx_markers_fetch_table(srx_markers* mk, int32_t which, void* out) {
    if (!mk) return fail(nullptr, SRX_E_ARG, "srx_markers_fetch_table: null handle");
    srx_ctx* ctx = mk->ctx;
    if (which == SRX_MARKERS_RANKSUM2 && !mk->wilcoxon)
        return fail(ctx, SRX_E_ARG, "srx_markers_fetch_table: the rank sums belong to srx_rank_genes_wilcoxon; this handle is a t-test's");
    if (which < SRX_MARKERS_CNT || which > SRX_MARKERS_RANKSUM2) return fail(ctx, SRX_E_ARG, "srx_markers_fetch_table: no table %d", which);
    if (!out) return fail(ctx, SRX_E_ARG, "srx_markers_fetch_table: null output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return markers_fetch_table(mk, which, out);
}

int32_t srx_markers_fetch_sizes(srx_markers* mk, uint64_t* n_cells_out) {
    if (!mk || !n_cells_out) return fail(mk ? mk->ctx : nullptr, SRX_E_ARG, "srx_markers_fetch_sizes: null argument");
    SRX_HIP(mk->ctx, hipSetDevice(mk->ctx->device));
    return d2h(mk->ctx, n_cells_out, mk->d_sizes, (size_t)mk->n_groups * 8);
}

void srx_markers_free(srx_markers* mk) { mk_free(mk); }

}  // extern "C"
