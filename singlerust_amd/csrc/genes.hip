// genes.hip — per-gene (column-direction) passes over the row-major CSR: the gene-tile structures, the moments / count /
// min-max passes, the moments cache of a matrix, and the statistics entry points of the C ABI.  (The feature selection that
// reads the moments: select.hip.)
//
// Per-gene accumulation from a CSR is a scatter: global atomics (one per non-zero, 3.3e9
// for the 1.3M-cell config) are two orders of magnitude too slow, so the accumulators are
// privatised in LDS.  3 accumulators x G genes do not fit 160 KiB, hence GENE TILING: the
// gene axis is cut into tiles of <= 8000 genes (20 B of LDS each: u32 count + f64 sum + f64
// sum of squares); because column indices are sorted inside a row, a tile's entries are one
// contiguous segment of every row, found once per sparsity pattern (ensure_tiles) and
// cached on the matrix.  A 1024-thread workgroup (one per CU: it owns the
// whole LDS) takes one (gene tile, row block), walks the row segments one wave per row with
// coalesced loads of indices/values, accumulates with LDS atomics, and flushes its tile to
// a per-block partial buffer; a second tiny kernel sums the partials in fixed order.
//
// Algorithmic bytes: nnz*(4 + s_v) + (N+1)*8 + G*24.
#include "pca_internal.hpp"     // (GramPk: the records whose tile cuts k_tile_ptr also finds)
#include "log1p64.hpp"

#include <algorithm>
#include <cmath>

namespace srx {

constexpr int kMaxTileGenes = 10000;      // 10000 * 16 B (two 64-bit sums per gene) + the 2 KiB logarithm table <= 163840 B of LDS.
                                          // c3 (28k genes): 3 tiles of 9334 — a row's tile segment is ~280 entries instead of ~210 with
                                          // 4 tiles of 7000 (8000 * 20 B while the pass also counted): moments + store 3.09 -> see DESIGN;
                                          // the other way round, 5 / 6 tiles: 3.28 / 3.66 ms (round 4 A/B, SRX_EXP_TILE_GENES)
constexpr int kMomThreads = 1024;

// lower_bound of `bound` inside each row's sorted column list, for the interior tile cuts.  E: a column index (the gene tiles
// of X) or a record of the compacted matrix (the 256-column tiles of its tile-major view, retile).
__device__ __forceinline__ int32_t entry_column(int32_t c) { return c; }
template <typename T>
__device__ __forceinline__ int32_t entry_column(const GramPk<T>& e) { return e.j; }
template <typename E>
__global__ void k_tile_ptr(const int64_t* __restrict__ indptr, const E* __restrict__ idx,
                           uint64_t n_rows, int n_tiles, int tile_genes, int64_t* __restrict__ tp) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t total = (uint64_t)(n_tiles - 1) * n_rows;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        uint64_t t = i / n_rows + 1, r = i % n_rows;
        int32_t bound = (int32_t)(t * (uint64_t)tile_genes);
        int64_t lo = indptr[r], hi = indptr[r + 1];
        while (lo < hi) {
            int64_t mid = lo + ((hi - lo) >> 1);
            if (entry_column(idx[mid]) < bound) lo = mid + 1; else hi = mid;
        }
        tp[i] = lo;
    }
}

// The two value passes of the reference over the columns — scatter-add of x (csr.rs:94-100) and of x^2 (csr.rs:175-178) — in
// ONE walk; the third, the histogram of the indices (csr.rs:29-36), depends on the pattern only and is k_gene_count's.
// XF: the values are the RAW matrix and x = ln_1p(f64(v) * scale_row) is formed on the fly in f64 (RowXf, common.hpp):
// the moments of the normalised + log1p'd matrix to f64 accuracy whatever the storage type, before (and without) the
// in-place write-back.
// WB (with XF): the transformed value is also stored back in place, at the storage precision — every stored value belongs to
// exactly one (gene tile, row) segment, i.e. to one lane of one workgroup, so this pass IS the in-place normalise + log1p of
// the pipeline and nothing reads the raw matrix after it.
// (Round 3, measured and not kept: for COUNT DATA a per-segment value table — each lane makes ONE logarithm per group of row
//  segments, ln_1p(c * scale) for c = 1 .. 32, parked in the LDS the cached counts leave free; a value then costs an exactness
//  test and one ds_read_b64 instead of the ~30-instruction logarithm.  Bit-identical results, 16x fewer logarithms, and
//  3.64 ms against 3.18: the four dependent LDS reads of a chunk queue behind the other waves' atomics, and the arithmetic
//  they replace was what hid that latency.)
template <typename T, typename I, bool XF, bool WB = false>
__global__ __launch_bounds__(kMomThreads) void k_gene_moments(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp, const I* __restrict__ idx,
    std::conditional_t<WB, T, const T>* __restrict__ vals, uint64_t n_rows, uint64_t n_cols, int n_tiles, int tile_genes,
    uint64_t rows_per_block, const double* __restrict__ row_sum, double target, double fx_sum, double fx_sq,
    uint32_t* __restrict__ poison, double* __restrict__ part_sum, double* __restrict__ part_sq) {
    extern __shared__ double lds[];
    double* s_acc = lds;            // per gene {sum, sum of squares} side by side: one address computation per value, the second
                                    // atomic at the instruction's immediate offset
    // behind the accumulators (tile_genes * 16 B): the log1p table
    // (the table from global memory instead — 2 KB, L1-resident, one vector load per value — was tried: 5.7 ms against 3.5)
    const Log1pTabEntry* s_tab = reinterpret_cast<const Log1pTabEntry*>(reinterpret_cast<char*>(lds) + (size_t)tile_genes * 16);
    if constexpr (XF) stage_log1p_table(const_cast<Log1pTabEntry*>(s_tab));
    for (int g = threadIdx.x; g < 2 * tile_genes; g += kMomThreads) s_acc[g] = 0.0;
    __syncthreads();

    // The gene tiles of one row block run on the SAME XCD (consecutive workgroup ids go round the 8 XCDs): a row's tile segments
    // share their boundary cache lines — read by two tiles, and each tile's in-place stores cover only part of them — and
    // with the tiles on four different L2s every such line was fetched (and, written, merged) once per tile: 15.7 GB of HBM
    // traffic for 10.9 GB of data (profiles/r03_traffic_c3.json).
    int tile;
    uint64_t rb;
    {
        const uint64_t n_rb = gridDim.x / (unsigned)n_tiles;
        if (n_rb % 8 == 0) {
            const uint64_t slot = blockIdx.x / 8;
            tile = (int)(slot % (unsigned)n_tiles);
            rb = (slot / (unsigned)n_tiles) * 8 + blockIdx.x % 8;
        } else {
            tile = blockIdx.x % n_tiles;
            rb = blockIdx.x / n_tiles;
        }
    }
    const int32_t gbase = tile * tile_genes;
    const uint64_t r0 = rb * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);      // row bounds and scales are then scalars
    constexpr int kWaves = kMomThreads / kWave;

    // 4 consecutive entries per lane: one 16-byte (8-byte for 16-bit indices) load of the indices and one (f32) or two (f64) of
    // the values, from a 4-entry boundary; entries outside the segment are masked (the arrays are padded by 16 entries).
    // A row's segment in one of 3 gene tiles is ~280 entries, a wave step is 256 slots: one segment per step left the second
    // step of nearly every segment at 10 % fill behind a dependent load — and the pass is bound by the latency of its chains at
    // 4 waves per SIMD (60 VALU instructions per value, profiles/r04_pmc_gram.md).  So a wave works on BATCHES of kBR row segments laid end to end in one slot space
    // (slot = 4 entries of one segment; segment u owns the slots S[u] .. S[u + 1]): 4 segments = ~284 slots = 5 steps at 89 %
    // fill; a lane finds its segment with kBR - 1 compares against the (wave-uniform) prefix sums and selects the segment's
    // base, offset, length and scale.  kBS steps of loads are in flight all the time (a step of the current batch is evaluated, then
    // the same step of the next batch is fetched into the registers it freed); longer batches take their remaining steps with
    // plain loads.  (4 segments / 5 steps fill better, 89 %, and are slower: 2.88 against 2.82 ms.)
    constexpr int kBR = sizeof(T) == 4 ? 3 : 2;      // f64 values: half the batch (a chunk is 10 registers instead of 6)
    constexpr int kBS = sizeof(T) == 4 ? 4 : 3;
    struct Chunk {
        std::conditional_t<sizeof(I) == 4, int4, uint2> gi;       // the four column indices as loaded (16-bit ones stay packed)
        T v[4];
    };
    auto gene_of = [](const Chunk& c, int j) -> int {
        if constexpr (sizeof(I) == 4) return j == 0 ? c.gi.x : j == 1 ? c.gi.y : j == 2 ? c.gi.z : c.gi.w;
        else return (int)(((j < 2 ? c.gi.x : c.gi.y) >> (16 * (j & 1))) & 0xffffu);
    };
    auto load_chunk = [&](int64_t e0, Chunk& c) {
        if constexpr (sizeof(I) == 4) c.gi = *reinterpret_cast<const int4*>(idx + e0);
        else c.gi = *reinterpret_cast<const uint2*>(idx + e0);        // four 16-bit indices in one 8-byte load
        if constexpr (sizeof(T) == 4) {
            const float4 t4 = *reinterpret_cast<const float4*>(vals + e0);
            c.v[0] = t4.x; c.v[1] = t4.y; c.v[2] = t4.z; c.v[3] = t4.w;
        } else {
            const double2 a2 = *reinterpret_cast<const double2*>(vals + e0);
            const double2 b2 = *reinterpret_cast<const double2*>(vals + e0 + 2);
            c.v[0] = a2.x; c.v[1] = a2.y; c.v[2] = b2.x; c.v[3] = b2.y;
        }
    };
    // XF: the sums are kept in FIXED POINT (2^-sum_shift, 2^-sq_shift; 64-bit integer LDS atomics): integer addition is
    // associative, so the moments do not depend on the order the atomics land in — two genes with identical columns get
    // identical sums, as in the reference's sequential loops (HighlyVariable(n) breaks exact ties by gene index), and the
    // run is reproducible to the bit.  [Raw f32 values widened to f64 sum exactly anyway: the plain path keeps f64 adds.]
    // The magic constant's bit pattern is NOT subtracted per value: the accumulators sum bits(1.5 * 2^52 + x * 2^shift) =
    // bits(1.5 * 2^52) + round(x * 2^shift) in wrapping 64-bit arithmetic and k_moments_reduce takes count x bits(1.5 * 2^52)
    // off again (the per-gene counts are known).  Positions are tested as 32-bit offsets from the segment start.
    auto add_chunk = [&](int64_t e0, int rel /* position of the chunk's first entry in its segment: >= -3 */, unsigned len,
                         const Chunk& c, double scale) {
        // XF: the four logarithms first, as independent straight-line chains the compiler can interleave (the accumulators
        // leave room for 4 waves per SIMD: a wave has to bring its own instruction-level parallelism); the rare argument
        // classes are patched afterwards (entries outside the segment hold padding values: evaluated, never used)
        double y4[4] = {0.0, 0.0, 0.0, 0.0};
        if constexpr (XF) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double x = (double)c.v[j] * scale;
                if constexpr (sizeof(T) == 4) y4[j] = log1p_f64_moment_common(x, s_tab);
                else y4[j] = log1p_f64_fast(x, s_tab);
            }
            if constexpr (sizeof(T) == 4) {
                bool any_rare = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) any_rare |= log1p_f64_moment_is_rare((double)c.v[j] * scale);
                if (__builtin_expect(any_rare, 0)) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double x = (double)c.v[j] * scale;
                        if (log1p_f64_moment_is_rare(x)) y4[j] = log1p_f64_rare(x, s_tab);
                    }
                }
            }
        }
        if constexpr (XF && WB) {
            // the chunk's values go back as one 16-byte store (two for f64) when all four belong to the segment
            T o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (T)y4[j];
            if (rel >= 0 && (unsigned)(rel + 3) < len) {
                // non-temporal: nothing reads a stored value again in this pass (2.77 -> 2.73 ms; non-temporal LOADS cost 0.4 ms:
                // the boundary lines of a row's tile segments are shared by two workgroups through L2)
                if constexpr (sizeof(T) == 4) {
                    typedef float f4v __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(f4v{(float)o[0], (float)o[1], (float)o[2], (float)o[3]}, reinterpret_cast<f4v*>(vals + e0));
                } else {
                    typedef double d2v __attribute__((ext_vector_type(2)));
                    __builtin_nontemporal_store(d2v{(double)o[0], (double)o[1]}, reinterpret_cast<d2v*>(vals + e0));
                    __builtin_nontemporal_store(d2v{(double)o[2], (double)o[3]}, reinterpret_cast<d2v*>(vals + e0 + 2));
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((unsigned)(rel + j) < len) vals[e0 + j] = o[j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if ((unsigned)(rel + j) < len) {
                const int32_t g0 = gene_of(c, j) - gbase;
                double x0 = (double)c.v[j];
                if constexpr (XF) {
                    x0 = y4[j];
                    if (__builtin_expect(!(fabs(x0) < 64.0), 0)) {     // NaN, infinite, or outside the fixed-point range: the gene's moments are NaN
                        poison[(uint64_t)gbase + g0] = 1u;
                        continue;
                    }
                    // round-to-nearest integer of x * 2^shift through the 1.5 * 2^52 trick (|x * 2^shift| < 2^51)
                    const double kMagic = 6755399441055744.0;
                    const unsigned long long is = (unsigned long long)__double_as_longlong(__builtin_fma(x0, fx_sum, kMagic));
                    const unsigned long long iq = (unsigned long long)__double_as_longlong(__builtin_fma(x0 * x0, fx_sq, kMagic));
                    // (a poisoned value adds nothing while the reduction still takes its magic bits off: the gene's sums are
                    //  replaced by NaN anyway)
                    unsigned long long* a2 = reinterpret_cast<unsigned long long*>(s_acc) + 2 * g0;
                    __hip_atomic_fetch_add(a2, is, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_add(a2 + 1, iq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    continue;
                }
                __hip_atomic_fetch_add(&s_acc[2 * g0], x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&s_acc[2 * g0 + 1], x0 * x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    };
    // (all offsets of a row block fit 32 bits: block_geometry keeps rows_per_block x n_cols below 2^31)
    int64_t blk_lo, blk_hi_;
    seg_bounds(indptr, tp, n_rows, n_tiles, tile, r0 < n_rows ? r0 : 0, blk_lo, blk_hi_);
    const int64_t base = blk_lo & ~(int64_t)3;
    struct Batch {                   // wave-uniform but for `c`: five scalars per segment
        int eb[kBR];                 // (4-entry boundary at or before the segment start) - base - 4 S: entry of slot s = base + eb + 4 s
        int q[kBR];                  // 4 S + (segment start - its boundary): position of slot s's first entry in the segment = 4 s - q
        int len[kBR];                // segment length
        int S[kBR + 1];              // first slot of segment u; S[kBR] = slots of the batch
        double scale[kBR];
    };
    // slot `slot` of the batch -> its chunk's first entry, that entry's position in the segment, the segment's length / scale
    // (X_sel = X[0] + sum_u [slot >= S[u]] (X[u] - X[u - 1]) in wrapping 32-bit arithmetic — exact for integers and for the two
    //  halves of a double's bit pattern alike: the differences are wave-uniform (SALU), a lane pays one v_cndmask per segment
    //  boundary and word and one add; a chain of selects between SGPR values costs three VALU instructions per select, the
    //  constant bus taking one scalar operand per instruction)
    auto locate = [&](const Batch& g, int slot, int64_t& e0, int& rel, unsigned& len, double& scale) {
        const unsigned long long sc0 = (unsigned long long)__double_as_longlong(g.scale[0]);
        unsigned eb = (unsigned)g.eb[0], q = (unsigned)g.q[0], ln = (unsigned)g.len[0], slo = (unsigned)sc0, shi = (unsigned)(sc0 >> 32);
#pragma unroll
        for (int u = 1; u < kBR; ++u) {
            const bool in = slot >= g.S[u];
            const unsigned long long a = (unsigned long long)__double_as_longlong(g.scale[u]),
                                     b = (unsigned long long)__double_as_longlong(g.scale[u - 1]);
            eb += in ? (unsigned)g.eb[u] - (unsigned)g.eb[u - 1] : 0u;
            q += in ? (unsigned)g.q[u] - (unsigned)g.q[u - 1] : 0u;
            ln += in ? (unsigned)g.len[u] - (unsigned)g.len[u - 1] : 0u;
            slo += in ? (unsigned)a - (unsigned)b : 0u;
            shi += in ? (unsigned)(a >> 32) - (unsigned)(b >> 32) : 0u;
        }
        e0 = base + (int64_t)(int)(eb + 4u * (unsigned)slot);
        rel = (int)(4u * (unsigned)slot - q);
        len = ln;
        scale = __longlong_as_double((long long)(((unsigned long long)shi << 32) | slo));
    };
    auto describe = [&](Batch& g, uint64_t rbase) {
        int S = 0;
#pragma unroll
        for (int u = 0; u < kBR; ++u) {
            const uint64_t r = rbase + (uint64_t)u * kWaves;
            int64_t lo = base, hi = base;
            g.scale[u] = 1.0;
            if (r < r1) {
                seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
                if constexpr (XF) {
                    const double sr = row_sum[r];
                    g.scale[u] = sr == 0.0 ? 0.0 : target / sr;            // scale/mod.rs:9-15
                }
            }
            const int64_t b0 = lo & ~(int64_t)3;
            const int a = (int)(lo - b0);
            g.len[u] = (int)(hi - lo);
            g.S[u] = S;
            g.eb[u] = (int)(b0 - base) - 4 * S;
            g.q[u] = 4 * S + a;
            S += (a + g.len[u] + 3) >> 2;
        }
        g.S[kBR] = S;
    };
    // the load of step `st` of a batch: unconditional (slots past the batch read the first segment's first chunk again: a branch
    // around a load makes the compiler's wait for one step's data wait for every load issued since)
    auto issue = [&](const Batch& g, int st, Chunk& c) {
        const int slot = st * kWave + lane;
        int64_t e0;
        int rel;
        unsigned len;
        double sc;
        locate(g, slot < g.S[kBR] ? slot : 0, e0, rel, len, sc);
        load_chunk(e0, c);
    };
    auto step = [&](const Batch& g, int st, const Chunk& c) {
        int slot = st * kWave + lane;
        // (recomputed here, opaquely: left to itself the compiler keeps the located values of every prefetched step alive from
        //  `issue` on — spilled)
        asm volatile("" : "+v"(slot));
        if (slot < g.S[kBR]) {
            int64_t e0;
            int rel;
            unsigned len;
            double sc;
            locate(g, slot, e0, rel, len, sc);
            add_chunk(e0, rel, len, c, sc);
        }
    };
    {
        // ONE set of kBS chunk registers: step st of the current batch is evaluated, then step st of the NEXT batch is fetched into
        // the registers it has just freed — kBS steps of loads in flight all the time with half the registers two whole batches
        // took (which left the scheduler no room to overlap the logarithms of two steps)
        const uint64_t stride = (uint64_t)kWaves * kBR;
        Batch cur, nxt;
        Chunk c[kBS];
        uint64_t rbase = r0 + wave;
        describe(cur, rbase);
#pragma unroll
        for (int st = 0; st < kBS; ++st) issue(cur, st, c[st]);
        while (rbase < r1) {
            describe(nxt, rbase + stride);
#pragma unroll
            for (int st = 0; st < kBS; ++st) {
                if (st * kWave < cur.S[kBR]) step(cur, st, c[st]);          // (wave-uniform)
                issue(nxt, st, c[st]);
            }
            // batches longer than kBS steps (long rows): the rest, a step at a time
            for (int slot = kBS * kWave + lane; slot < cur.S[kBR]; slot += kWave) {
                int64_t e0;
                int rel;
                unsigned len;
                double sc;
                locate(cur, slot, e0, rel, len, sc);
                Chunk cc;
                load_chunk(e0, cc);
                add_chunk(e0, rel, len, cc, sc);
            }
            cur = nxt;
            rbase += stride;
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < tile_genes; g += kMomThreads) {
        uint64_t gene = (uint64_t)gbase + g;
        if (gene < n_cols) {
            part_sum[rb * n_cols + gene] = s_acc[2 * g];
            part_sq[rb * n_cols + gene] = s_acc[2 * g + 1];
        }
    }
}

// Per-gene non-zero counts of the stored pattern (csr.rs:24-36: the column histogram of the indices) — a property of the
// sparsity pattern alone: made once per pattern (srx_matrix_prepare, or the first pass that needs them), kept on the matrix,
// inherited by clones; the moments passes then carry no count atomic and no counters in LDS (16 B per gene: 3 gene tiles at
// 28k genes instead of 4).  Workgroup = (row block, gene tile) like the moments pass, 32-bit LDS counters, flushed with global
// partials `cnt[row block][gene]`.
template <typename I>
__global__ __launch_bounds__(kMomThreads) void k_gene_count(const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp,
                                                            const I* __restrict__ idx, uint64_t n_rows, uint64_t n_cols, int n_tiles,
                                                            int tile_genes, uint64_t rows_per_block, uint32_t* __restrict__ cnt) {
    extern __shared__ double lds[];
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(lds);
    for (int g = threadIdx.x; g < tile_genes; g += kMomThreads) s_cnt[g] = 0u;
    __syncthreads();
    const int tile = blockIdx.x % n_tiles;
    const uint64_t rb = blockIdx.x / n_tiles;
    const int32_t gbase = tile * tile_genes;
    const uint64_t r0 = rb * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    constexpr int kWaves = kMomThreads / kWave;
    // four row segments per step; a lane takes 4 consecutive entries from the 4-entry boundary at or before the segment start
    // (one 8-byte load of 16-bit indices, 16 bytes of 32-bit ones: 256 entries per wave instruction — one entry per lane and
    // load left this pass at 1.3-1.7 TB/s), two such chunks of every segment in flight, entries outside [lo, hi) masked
    // (the arrays are padded by 16 entries)
    constexpr int kU = 2, kR = 4;
    auto load4 = [&](int64_t e0, int32_t (&g)[4]) {
        if constexpr (sizeof(I) == 4) {
            const int4 g4 = *reinterpret_cast<const int4*>(idx + e0);
            g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
        } else {
            const uint2 g2 = *reinterpret_cast<const uint2*>(idx + e0);
            g[0] = (int)(g2.x & 0xffffu); g[1] = (int)(g2.x >> 16);
            g[2] = (int)(g2.y & 0xffffu); g[3] = (int)(g2.y >> 16);
        }
    };
    auto add4 = [&](int64_t e0, int64_t lo, int64_t hi, const int32_t (&g)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (e0 + j >= lo && e0 + j < hi)
                __hip_atomic_fetch_add(&s_cnt[g[j] - gbase], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    for (uint64_t rb4 = r0 + wave; rb4 < r1; rb4 += (uint64_t)kWaves * kR) {
        int64_t lo[kR], hi[kR];
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const uint64_t r = rb4 + (uint64_t)q * kWaves;
            lo[q] = hi[q] = 0;
            if (r < r1) seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo[q], hi[q]);
        }
        int32_t g[kR][kU][4];
#pragma unroll
        for (int q = 0; q < kR; ++q)
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t b0 = lo[q] & ~(int64_t)3, e0 = b0 + 4 * (u * kWave + lane);
                load4(e0 < hi[q] ? e0 : b0, g[q][u]);
            }
#pragma unroll
        for (int q = 0; q < kR; ++q) {
            const int64_t b0 = lo[q] & ~(int64_t)3;
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t e0 = b0 + 4 * (u * kWave + lane);
                if (e0 < hi[q]) add4(e0, lo[q], hi[q], g[q][u]);
            }
            // segments longer than kU x 256 entries: the rest, a chunk at a time
            for (int64_t e0 = b0 + 4 * (kU * kWave + lane); e0 < hi[q]; e0 += 4 * kWave) {
                int32_t gt[4];
                load4(e0, gt);
                add4(e0, lo[q], hi[q], gt);
            }
        }
    }
    __syncthreads();
    // per-row-block partials, summed by k_gene_count_reduce (global atomics into the 28k counters — 341 row blocks on every
    // address — took ~0.9 of this pass's 1.4 ms)
    for (int g = threadIdx.x; g < tile_genes; g += kMomThreads) {
        const uint64_t gene = (uint64_t)gbase + g;
        if (gene < n_cols) cnt[rb * n_cols + gene] = s_cnt[g];
    }
}
__global__ void k_gene_count_reduce(const uint32_t* __restrict__ part, uint64_t n_cols, uint64_t n_blocks, uint32_t* __restrict__ cnt) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_cols) return;
    uint32_t c = 0;
    for (uint64_t b = 0; b < n_blocks; ++b) c += part[b * n_cols + j];
    cnt[j] = c;
}

// Fixed-order sum of the per-row-block partials -> packed f64 [cnt | sum | sq | n_rows].
// `cnt`: this shard's per-gene non-zero counts (pattern-only, k_gene_count).
// Workgroup = 64 genes x kRedSlices slices of the row blocks (a thread per gene alone: 111 workgroups of one dependent walk over
// all 341 partials each, 45 us at c3 — a fixed cost of the step however few rows a rank holds).  The fixed-point partials are
// integers: the slices add in any order.
constexpr int kRedSlices = 8;
__global__ __launch_bounds__(64 * kRedSlices) void k_moments_reduce(
    const double* __restrict__ part_sum, const double* __restrict__ part_sq, uint64_t n_cols, uint64_t n_blocks, uint64_t n_rows,
    const uint32_t* __restrict__ cnt, double inv_fx_sum, double inv_fx_sq, const uint32_t* __restrict__ poison,
    double* __restrict__ packed) {
    __shared__ unsigned long long red[2][kRedSlices][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const uint64_t j = (uint64_t)blockIdx.x * 64 + lane;
    if (blockIdx.x == 0 && threadIdx.x == 0) packed[3 * n_cols] = (double)n_rows;
    const bool live = j < n_cols;
    double s = 0.0, q = 0.0;
    if (inv_fx_sum != 0.0) {                 // fixed-point partials (transformed values): exact integer sums
        unsigned long long is = 0, iq = 0;
        if (live) {
            // (four blocks' partials in flight per thread)
            uint64_t b = slice;
            for (; b + 3 * kRedSlices < n_blocks; b += 4 * kRedSlices) {
                unsigned long long xs[4], xq[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    xs[u] = (unsigned long long)__double_as_longlong(part_sum[(b + u * kRedSlices) * n_cols + j]);
                    xq[u] = (unsigned long long)__double_as_longlong(part_sq[(b + u * kRedSlices) * n_cols + j]);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    is += xs[u];
                    iq += xq[u];
                }
            }
            for (; b < n_blocks; b += kRedSlices) {
                is += (unsigned long long)__double_as_longlong(part_sum[b * n_cols + j]);
                iq += (unsigned long long)__double_as_longlong(part_sq[b * n_cols + j]);
            }
        }
        red[0][slice][lane] = is;
        red[1][slice][lane] = iq;
        __syncthreads();
        if (slice != 0 || !live) return;
#pragma unroll
        for (int u = 1; u < kRedSlices; ++u) {
            is += red[0][u][lane];
            iq += red[1][u][lane];
        }
        // every contribution carried the bit pattern of the 1.5 * 2^52 rounding constant along (k_gene_moments): off again
        const unsigned long long cn = (unsigned long long)cnt[j];
        const unsigned long long magic_bits = (unsigned long long)__double_as_longlong(6755399441055744.0);
        s = (double)(long long)(is - cn * magic_bits) * inv_fx_sum;
        q = (double)(long long)(iq - cn * magic_bits) * inv_fx_sq;
        if (poison[j]) s = q = __builtin_nan("");
    } else {
        // f64 partials of the raw values: ONE fixed order (the row blocks in sequence), by the first slice
        if (slice != 0 || !live) return;
        for (uint64_t b = 0; b < n_blocks; ++b) {
            s += part_sum[b * n_cols + j];
            q += part_sq[b * n_cols + j];
        }
    }
    packed[j] = (double)cnt[j];
    packed[n_cols + j] = s;
    packed[2 * n_cols + j] = q;
}

__global__ void k_moments_unpack(const double* __restrict__ packed, uint64_t n_cols, uint64_t* __restrict__ cnt,
                                 double* __restrict__ sum, double* __restrict__ sq) {
    uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_cols) return;
    cnt[j] = (uint64_t)packed[j];
    sum[j] = packed[n_cols + j];
    sq[j] = packed[2 * n_cols + j];
}

// ---- per-gene min / max (csr.rs:212-221) ------------------------------------------------------
// Order-preserving map double -> u64 so LDS integer atomics (ds_min_u64 / ds_max_u64) apply.
__device__ __host__ __forceinline__ uint64_t f64_key(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __host__ __forceinline__ double key_f64(uint64_t k) {
    uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

template <typename T>
__global__ __launch_bounds__(kMomThreads) void k_gene_minmax(
    const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp, const int32_t* __restrict__ idx,
    const T* __restrict__ vals, uint64_t n_rows, uint64_t n_cols, int n_tiles, int tile_genes,
    uint64_t rows_per_block, unsigned long long* __restrict__ g_min, unsigned long long* __restrict__ g_max) {
    extern __shared__ double lds[];
    unsigned long long* s_min = reinterpret_cast<unsigned long long*>(lds);
    unsigned long long* s_max = s_min + tile_genes;
    const unsigned long long kInf = f64_key(INFINITY), kNinf = f64_key(-INFINITY);
    for (int g = threadIdx.x; g < tile_genes; g += kMomThreads) { s_min[g] = kInf; s_max[g] = kNinf; }
    __syncthreads();
    const int tile = blockIdx.x % n_tiles;
    const uint64_t rb = blockIdx.x / n_tiles;
    const int32_t gbase = tile * tile_genes;
    const uint64_t r0 = rb * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);      // row bounds and scales are then scalars
    constexpr int kWaves = kMomThreads / kWave;
    for (uint64_t r = r0 + wave; r < r1; r += kWaves) {
        int64_t lo, hi;
        seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
        for (int64_t p = lo + lane; p < hi; p += kWave) {
            double x = (double)vals[p];
            if (x != x) continue;                      // f64::min/max ignore a NaN operand
            int32_t g = idx[p] - gbase;
            unsigned long long k = f64_key(x);
            atomicMin(&s_min[g], k);
            atomicMax(&s_max[g], k);
        }
    }
    __syncthreads();
    for (int g = threadIdx.x; g < tile_genes; g += kMomThreads) {
        uint64_t gene = (uint64_t)gbase + g;
        if (gene < n_cols) {
            if (s_min[g] != kInf) atomicMin(&g_min[gene], s_min[g]);
            if (s_max[g] != kNinf) atomicMax(&g_max[gene], s_max[g]);
        }
    }
}

__global__ void k_fill_u64(unsigned long long* p, uint64_t n, unsigned long long v) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// normalize_total(Column) on CSR: scale/mod.rs:141-173, values[j] *= scale[col].
template <typename T>
__global__ void k_col_scale(const int32_t* __restrict__ idx, T* __restrict__ vals, uint64_t nnz,
                            const double* __restrict__ sum, double target) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < nnz; i += stride) {
        double s = sum[idx[i]];
        double sc = s == 0.0 ? 0.0 : target / s;      // scale/mod.rs:93-99
        vals[i] = (T)((double)vals[i] * sc);
    }
}

static void tile_geometry(const srx_mat* m, int& n_tiles, int& tile_genes) {
    const uint64_t G = at_least_one(m->n_cols);
    n_tiles = (int)((G + kMaxTileGenes - 1) / kMaxTileGenes);
    tile_genes = (int)((G + n_tiles - 1) / n_tiles);
}

template <typename E>
int32_t launch_tile_ptr(srx_ctx* ctx, const int64_t* indptr, const E* idx, uint64_t n_rows, int n_tiles, int tile_genes,
                        int64_t* tp) {
    uint64_t total = (uint64_t)(n_tiles - 1) * n_rows;
    uint64_t g = (total + 255) / 256;
    if (g < 1) g = 1;
    if (g > 65535) g = 65535;
    hipLaunchKernelGGL(k_tile_ptr<E>, dim3((unsigned)g), dim3(256), 0, ctx->stream, indptr, idx, n_rows, n_tiles,
                       tile_genes, tp);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}
template int32_t launch_tile_ptr<int32_t>(srx_ctx*, const int64_t*, const int32_t*, uint64_t, int, int, int64_t*);
template int32_t launch_tile_ptr<GramPk<float>>(srx_ctx*, const int64_t*, const GramPk<float>*, uint64_t, int, int, int64_t*);
template int32_t launch_tile_ptr<GramPk<double>>(srx_ctx*, const int64_t*, const GramPk<double>*, uint64_t, int, int, int64_t*);

// Both pattern-only structures of a fresh CSR matrix in ONE walk over its 32-bit column indices: the 16-bit mirror (entries
// past nnz: 0, the arrays are padded for the vector walks) and the NB = n_tiles - 1 interior gene-tile cuts of every row.  A
// wave per row, 256 entries per step; a row is sorted by column, so the cut at `bound` is the row's start + the number of
// entries below it = the popcounts of the waves' `idx < bound` ballots (scalar instructions; no search, no second pass).
// k_tile_ptr's binary searches + a separate narrowing pass read the indices twice and moved 10.9 GB at c3 (2.3 ms of a cold
// step's 14.7); this moves 6.6.
// WIDEN: the other way round — the 16-bit mirror came over PCIe (upload_on: a quarter of the host's index bytes cross the
// link) and the 32-bit indices are made from it, with the same cuts.
// COUNT (round 6): the walk also makes the per-gene non-zero counts (csr.rs:24-36) — a 32-bit counter per gene in LDS (n_cols <= 38 000:
// 152 KB), one LDS atomic per entry, per-workgroup partials summed by k_gene_count_reduce — so that a handle leaves the upload / the
// generation with ALL its pattern-only structures and the first pipeline call on it pays no k_gene_count (0.54 + 0.12 ms at c3: VERDICT
// r5 item 5).  1024-thread workgroups then (the counters hold a CU to one workgroup).
template <int NB, bool WIDEN, bool COUNT = false>
__global__ __launch_bounds__(COUNT ? 1024 : 256) void k_narrow16_tiles(const int64_t* __restrict__ indptr, int32_t* idx,
                                                        uint64_t n_rows, int tile_genes, uint16_t* out,
                                                        int64_t* __restrict__ tp, uint32_t n_cols = 0, uint32_t* __restrict__ cnt_part = nullptr) {
    extern __shared__ uint32_t s_hist[];
    if constexpr (COUNT) {
        for (uint32_t g = threadIdx.x; g < n_cols; g += blockDim.x) s_hist[g] = 0u;
        __syncthreads();
    }
    const int lane = lane_id();
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x / kWave);
    constexpr int kU = 4;
    for (uint64_t r = global_wave_id(); r < n_rows; r += n_waves) {
        const int64_t lo = indptr[r], hi = indptr[r + 1];
        int cnt[NB > 0 ? NB : 1];
#pragma unroll
        for (int b = 0; b < NB; ++b) cnt[b] = 0;
        for (int64_t e0 = lo; e0 < hi; e0 += kU * kWave) {
            int32_t v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t e = e0 + u * kWave + lane;
                if constexpr (WIDEN) v[u] = e < hi ? (int32_t)out[e] : 0x7fffffff;
                else v[u] = e < hi ? idx[e] : 0x7fffffff;
            }
#pragma unroll
            for (int u = 0; u < kU; ++u) {
                const int64_t e = e0 + u * kWave + lane;
                if (e < hi) {
                    if constexpr (WIDEN) idx[e] = v[u];
                    else out[e] = (uint16_t)v[u];
                    if constexpr (COUNT) {
                        if ((uint32_t)v[u] < n_cols) __hip_atomic_fetch_add(&s_hist[v[u]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
#pragma unroll
                for (int b = 0; b < NB; ++b) cnt[b] += __popcll(__ballot(v[u] < (b + 1) * tile_genes));
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int b = 0; b < NB; ++b) tp[(uint64_t)b * n_rows + r] = lo + cnt[b];
        }
    }
    // (the 16 padding entries behind the last non-zero)
    if (blockIdx.x == 0 && threadIdx.x < 16) out[indptr[n_rows] + threadIdx.x] = (uint16_t)0;
    if constexpr (COUNT) {
        __syncthreads();
        for (uint32_t g = threadIdx.x; g < n_cols; g += blockDim.x) cnt_part[(uint64_t)blockIdx.x * n_cols + g] = s_hist[g];
    }
}

template <bool WIDEN>
static int32_t launch_narrow16_tiles(srx_mat* m, int nt, int tg, hipStream_t stream) {
    srx_ctx* ctx = m->ctx;
    // the counting form where a counter per gene fits the LDS and the counts are still owed
    const bool count = m->n_cols * 4 <= 155648 && !m->cnt_pat_valid && m->n_rows > 0 && m->nnz > 0;
    const unsigned g = count ? (unsigned)std::min<uint64_t>((m->n_rows + 15) / 16, (uint64_t)ctx->n_cus * 2)
                             : (unsigned)std::min<uint64_t>((m->n_rows + 3) / 4, (uint64_t)ctx->n_cus * 32);
    uint32_t* part = nullptr;
    if (count) {
        if (!m->d_cnt_pat) SRX_HIP(ctx, dev_malloc(ctx, (void**)&m->d_cnt_pat, m->n_cols * sizeof(uint32_t)));
        SRX_TRY(scratch(ctx, stream == ctx->stream ? "n16_part_cnt" : "n16_part_cnt_side", (size_t)g * m->n_cols * sizeof(uint32_t), (void**)&part));
    }
    auto go = [&](auto nb) -> int32_t {
        constexpr int NBv = decltype(nb)::value;
        if (count) {
            const size_t lds = m->n_cols * sizeof(uint32_t);
            SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_narrow16_tiles<NBv, WIDEN, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((k_narrow16_tiles<NBv, WIDEN, true>), dim3(g ? g : 1), dim3(1024), lds, stream, m->d_indptr, m->d_indices,
                               m->n_rows, tg, m->d_idx16, m->d_tile_ptr, (uint32_t)m->n_cols, part);
        } else {
            hipLaunchKernelGGL((k_narrow16_tiles<NBv, WIDEN, false>), dim3(g ? g : 1), dim3(256), 0, stream, m->d_indptr, m->d_indices,
                               m->n_rows, tg, m->d_idx16, m->d_tile_ptr, 0u, (uint32_t*)nullptr);
        }
        return SRX_OK;
    };
    int32_t rc;
    switch (nt - 1) {
        case 0: rc = go(std::integral_constant<int, 0>{}); break;
        case 1: rc = go(std::integral_constant<int, 1>{}); break;
        case 2: rc = go(std::integral_constant<int, 2>{}); break;
        case 3: rc = go(std::integral_constant<int, 3>{}); break;
        case 4: rc = go(std::integral_constant<int, 4>{}); break;
        case 5: rc = go(std::integral_constant<int, 5>{}); break;
        case 6: rc = go(std::integral_constant<int, 6>{}); break;
        case 7: rc = go(std::integral_constant<int, 7>{}); break;
        default: rc = go(std::integral_constant<int, 8>{}); break;
    }
    SRX_TRY(rc);
    if (count) {
        hipLaunchKernelGGL(k_gene_count_reduce, dim3((unsigned)((m->n_cols + 255) / 256)), dim3(256), 0, stream, (const uint32_t*)part, m->n_cols,
                           (uint64_t)g, m->d_cnt_pat);
        m->cnt_pat_valid = true;
    }
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// upload_on's second half for a matrix of at most 65536 columns: d_idx16 holds the column indices; d_indices and the tile cuts
// follow from it.  (m->d_indptr is in place; at most 7 tiles at 65536 columns.)
int32_t tiles_from_idx16(srx_mat* m, hipStream_t stream) {
    srx_ctx* ctx = m->ctx;
    int nt, tg;
    tile_geometry(m, nt, tg);
    if (nt > 9 || !m->d_idx16 || m->d_tile_ptr) return fail(ctx, SRX_E_ARG, "tiles_from_idx16: %d gene tiles", nt);
    if (m->n_rows == 0) return SRX_OK;
    if (nt > 1) SRX_HIP(ctx, dev_malloc(ctx, (void**)&m->d_tile_ptr, (size_t)(nt - 1) * m->n_rows * sizeof(int64_t)));
    SRX_TRY(launch_narrow16_tiles<true>(m, nt, tg, stream));
    m->n_tiles = nt;
    m->tile_genes = tg;
    return SRX_OK;
}

// The gene-tile geometry of a matrix and its pattern-only structures, once per pattern: up to 65536 columns the 16-bit mirror,
// the cuts and (up to 38000 columns) the per-gene counts in ONE walk, as the upload makes them; beyond, the cuts by binary
// search and no mirror.  A matrix without rows has nothing to walk (as in tiles_from_idx16: an upload of a shard without rows
// reaches here with its mirror and no geometry); the passes still read the cuts of row 0, so it gets one row of them.
int32_t ensure_tiles(srx_mat* m) {
    srx_ctx* ctx = m->ctx;
    if (m->n_tiles) return SRX_OK;
    int nt, tg;
    tile_geometry(m, nt, tg);
    if (nt > 1) SRX_HIP(ctx, dev_malloc(ctx, (void**)&m->d_tile_ptr, (size_t)(nt - 1) * at_least_one(m->n_rows) * sizeof(int64_t)));
    if (m->n_rows > 0 && m->n_cols <= 65536) {
        SRX_HIP(ctx, dev_malloc(ctx, (void**)&m->d_idx16, (m->nnz + 16) * sizeof(uint16_t)));
        SRX_TRY(launch_narrow16_tiles<false>(m, nt, tg, ctx->stream));
    } else if (m->n_rows > 0) {
        SRX_TRY(launch_tile_ptr(ctx, m->d_indptr, m->d_indices, m->n_rows, nt, tg, m->d_tile_ptr));
    }
    m->n_tiles = nt;
    m->tile_genes = tg;
    return SRX_OK;
}

static int32_t block_geometry(const srx_mat* m, uint64_t& n_blocks, uint64_t& rows_per_block) {
    // four workgroups per CU, one resident at a time (the accumulators fill the LDS): c3, XF + write-back pass, 1 / 2 / 4 / 8 / 16
    // per CU: 3.23 / 3.12 / 3.06 / 3.10 / 3.19 ms (shorter workgroups even out the CUs; more of them means more partial sums)
    uint64_t want = (uint64_t)(4 * m->ctx->n_cus) / (uint64_t)m->n_tiles;
    if (want < 1) want = 1;
    uint64_t by_rows = (m->n_rows + 63) / 64;   // at least ~64 rows per block
    if (by_rows < 1) by_rows = 1;
    n_blocks = want < by_rows ? want : by_rows;
    rows_per_block = (m->n_rows + n_blocks - 1) / n_blocks;
    if (rows_per_block < 1) rows_per_block = 1;
    // the moments pass addresses a row block's entries with 32-bit offsets from the block's first entry (a row holds at most
    // n_cols entries)
    const uint64_t cap = std::max<uint64_t>(1, 0x7fffffffull / std::max<uint64_t>(m->n_cols, 1));
    if (rows_per_block > cap) {
        rows_per_block = cap;
        n_blocks = (m->n_rows + rows_per_block - 1) / rows_per_block;
        // every block leaves a partial (sum, sumsq) pair per gene: a matrix so wide that the 32-bit cap asks for thousands of
        // blocks would make those buffers larger than the matrix — refused, not attempted
        if ((double)n_blocks * (double)std::max<uint64_t>(m->n_cols, 1) * 16.0 > 8.0 * 1024 * 1024 * 1024)
            return fail(m->ctx, SRX_E_ARG, "gene statistics: %llu columns x %llu row blocks exceed the partial-sum budget (matrix too wide)",
                        (unsigned long long)m->n_cols, (unsigned long long)n_blocks);
    }
    return SRX_OK;
}

// The storage x index-width dispatch of the per-gene passes: f(the values, typed by the storage) and f(the column indices:
// the 16-bit mirror where the matrix has one); a pass over both nests the two.
template <typename F>
static int32_t by_values(const srx_mat* m, F&& f) {
    return is_f32(m) ? f((float*)m->d_values) : f((double*)m->d_values);
}
template <typename F>
static int32_t by_indices(const srx_mat* m, F&& f) {
    return m->d_idx16 ? f((const uint16_t*)m->d_idx16) : f((const int32_t*)m->d_indices);
}

// This shard's (cnt, sum, sumsq) per gene and its row count, packed as 3G+1 doubles in a scratch buffer.
// `xf`: moments of the transformed values ln_1p(v * scale_row) formed on the fly from the raw matrix.
static int32_t local_moments(srx_mat* m, double** packed_out, RowXf xf = RowXf{}) {
    srx_ctx* ctx = m->ctx;
    SRX_TRY(ensure_tiles(m));
    const uint64_t G = m->n_cols;
    uint64_t nb, rpb;
    SRX_TRY(block_geometry(m, nb, rpb));
    double *p_sum, *p_sq, *packed;
    SRX_TRY(scratch(ctx, "mom_part_sum", nb * at_least_one(G) * sizeof(double), (void**)&p_sum));
    SRX_TRY(scratch(ctx, "mom_part_sq", nb * at_least_one(G) * sizeof(double), (void**)&p_sq));
    SRX_TRY(scratch(ctx, "mom_packed", (3 * G + 1) * sizeof(double), (void**)&packed));
    // the per-gene counts depend on the sparsity pattern only: counted once per pattern (here, or by srx_matrix_prepare), kept
    // on the matrix (clones inherit them)
    SRX_TRY(ensure_pattern_counts(m));
    const size_t lds = (size_t)m->tile_genes * 16 + (xf.row_sum ? (size_t)kLog1pTabBytes : 0);
    // s_i = 2 when the 16-bit index mirror exists (n_cols <= 65536), 4 otherwise
    const double bytes = (double)m->nnz * ((m->n_cols <= 65536 ? 2.0 : 4.0) + val_bytes(m)) + (double)(m->n_rows + 1) * 8.0 +
                         (double)G * 24.0 + (xf.row_sum ? (double)m->n_rows * 8.0 : 0.0) +
                         (xf.write_back ? (double)m->nnz * val_bytes(m) : 0.0);
    // fixed-point scales of the transformed sums: 62 bits hold n_rows values of magnitude < 2^6 (ln_1p(x) < 64, any
    // x < 6e27) resp. their squares
    double fx_sum = 0.0, fx_sq = 0.0;
    if (xf.row_sum) {
        int lg = 0;
        while ((1ull << lg) < at_least_one(m->n_rows)) ++lg;
        fx_sum = std::ldexp(1.0, std::min(62 - 6 - lg, 44));
        fx_sq = std::ldexp(1.0, std::min(62 - 12 - lg, 38));
    }
    uint32_t* d_poison = nullptr;
    if (xf.row_sum) {
        SRX_TRY(scratch(ctx, "mom_poison", at_least_one(G) * sizeof(uint32_t), (void**)&d_poison));
        SRX_HIP(ctx, hipMemsetAsync(d_poison, 0, at_least_one(G) * sizeof(uint32_t), ctx->stream));
    }
    {
        ProfScope ps(ctx, SRX_K_MOMENTS, bytes);
        dim3 grid((unsigned)(nb * m->n_tiles));
        auto launch = [&](auto kern, const auto* idxp, auto* valp) -> int32_t {
            SRX_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, grid, dim3(kMomThreads), lds, ctx->stream, m->d_indptr, m->d_tile_ptr, idxp, valp,
                               m->n_rows, G, m->n_tiles, m->tile_genes, rpb, xf.row_sum, xf.target, fx_sum, fx_sq, d_poison, p_sum, p_sq);
            return SRX_OK;
        };
        SRX_TRY(by_values(m, [&](auto* vals) {
            return by_indices(m, [&](const auto* idx) {
                using T = std::remove_pointer_t<decltype(vals)>;
                using I = std::remove_cv_t<std::remove_pointer_t<decltype(idx)>>;
                if (xf.row_sum && xf.write_back) return launch(k_gene_moments<T, I, true, true>, idx, vals);
                if (xf.row_sum) return launch(k_gene_moments<T, I, true>, idx, (const T*)vals);
                return launch(k_gene_moments<T, I, false>, idx, (const T*)vals);
            });
        }));
        hipLaunchKernelGGL(k_moments_reduce, dim3((unsigned)at_least_one((G + 63) / 64)), dim3(64 * kRedSlices), 0, ctx->stream, p_sum, p_sq, G, nb,
                           m->n_rows, (const uint32_t*)m->d_cnt_pat, fx_sum != 0.0 ? 1.0 / fx_sum : 0.0,
                           fx_sq != 0.0 ? 1.0 / fx_sq : 0.0, (const uint32_t*)d_poison, packed);
    }
    SRX_HIP(ctx, hipGetLastError());
    *packed_out = packed;
    return SRX_OK;
}

// The pattern-only per-gene counts (k_gene_count): one pass over the column indices, once per pattern — srx_matrix_prepare
// makes them ahead of time, so that clones inherit them.
int32_t ensure_pattern_counts(srx_mat* m) {
    if (m->cnt_pat_valid && m->d_cnt_pat) return SRX_OK;
    srx_ctx* ctx = m->ctx;
    SRX_TRY(ensure_tiles(m));
    const uint64_t G = m->n_cols;
    if (!m->d_cnt_pat) SRX_HIP(ctx, dev_malloc(ctx, (void**)&m->d_cnt_pat, at_least_one(G) * sizeof(uint32_t)));
    SRX_HIP(ctx, hipMemsetAsync(m->d_cnt_pat, 0, at_least_one(G) * sizeof(uint32_t), ctx->stream));
    if (m->n_rows && m->nnz) {
        uint64_t nb, rpb;
        SRX_TRY(block_geometry(m, nb, rpb));
        uint32_t* part;
        SRX_TRY(scratch(ctx, "mom_part_cnt", nb * G * sizeof(uint32_t), (void**)&part));
        const dim3 grid((unsigned)(nb * m->n_tiles));
        const size_t lds = (size_t)m->tile_genes * 4;
        ProfScope ps(ctx, SRX_K_MOMENTS, (double)m->nnz * (m->d_idx16 ? 2.0 : 4.0) + (double)(m->n_rows + 1) * 8.0 + (double)G * 4.0);
        by_indices(m, [&](const auto* idx) {
            using I = std::remove_cv_t<std::remove_pointer_t<decltype(idx)>>;
            hipLaunchKernelGGL(k_gene_count<I>, grid, dim3(kMomThreads), lds, ctx->stream, m->d_indptr, m->d_tile_ptr, idx, m->n_rows, G,
                               m->n_tiles, m->tile_genes, rpb, part);
            return SRX_OK;
        });
        hipLaunchKernelGGL(k_gene_count_reduce, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, ctx->stream, (const uint32_t*)part, G, nb,
                           m->d_cnt_pat);
        SRX_HIP(ctx, hipGetLastError());
    }
    m->cnt_pat_valid = true;
    return SRX_OK;
}

__global__ void k_add_f64(double* __restrict__ acc, const double* __restrict__ x, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] += x[i];
}

// Backed mode: the moments of one row tile ADDED to `d_acc` (3G+1 doubles; counts stay exact below 2^53).
int32_t moments_accumulate(srx_mat* m, double* d_acc, RowXf xf) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    double* packed;
    SRX_TRY(local_moments(m, &packed, xf));
    const uint64_t n = 3 * m->n_cols + 1;
    hipLaunchKernelGGL(k_add_f64, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_acc, packed, n);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

// ---- the moments cache of a matrix: d_cnt / d_sum / d_sq and n_rows_global, valid while moments_version == version ----
static int32_t alloc_moments(srx_mat* m) {
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t G = at_least_one(m->n_cols);
    if (!m->d_cnt) {
        SRX_HIP(ctx, hipMalloc((void**)&m->d_cnt, G * sizeof(uint64_t)));
        SRX_HIP(ctx, hipMalloc((void**)&m->d_sum, G * sizeof(double)));
        SRX_HIP(ctx, hipMalloc((void**)&m->d_sq, G * sizeof(double)));
    }
    return SRX_OK;
}

// The one route from this rank's packed totals (3G+1 doubles: cnt | sum | sq | rows) to the global moments of `m`: ONE
// all-reduce across the row shards, the unpack into d_cnt / d_sum / d_sq, and n_rows_global.  `n_is_local`: the packed row
// count is m->n_rows (a resident matrix), so a single-rank context needs no read-back for N; false: N always comes from the
// packed buffer (a backed accumulator's n_rows is not the global count).  Does not stamp moments_version.
static int32_t reduce_unpack_moments(srx_mat* m, double* d_packed, bool n_is_local) {
    srx_ctx* ctx = m->ctx;
    const uint64_t G = m->n_cols;
    SRX_TRY(allreduce_f64(ctx, d_packed, 3 * G + 1));
    hipLaunchKernelGGL(k_moments_unpack, dim3((unsigned)((G + 255) / 256 + 1)), dim3(256), 0, ctx->stream, d_packed, G,
                       m->d_cnt, m->d_sum, m->d_sq);
    SRX_HIP(ctx, hipGetLastError());
    if (n_is_local && !ctx->comm && !ctx->host_allreduce) {
        m->n_rows_global = m->n_rows;
    } else {
        double ng = 0.0;
        SRX_TRY(d2h(ctx, &ng, d_packed + 3 * G, sizeof(double)));
        m->n_rows_global = (uint64_t)ng;
    }
    return SRX_OK;
}

void moments_adopt(srx_mat* m) { m->moments_version = m->version; }
void moments_retire(srx_mat* m) { m->moments_version = 0; }       // (a version is never 0)

// All-reduces `d_packed` (3G+1 doubles, this rank's totals) and installs it as the global moments of `m`.
int32_t moments_install(srx_mat* m, double* d_packed) {
    SRX_TRY(alloc_moments(m));
    SRX_TRY(reduce_unpack_moments(m, d_packed, false));
    moments_adopt(m);
    return SRX_OK;
}

int32_t ensure_moments(srx_mat* m) {
    if (m->moments_version == m->version) return SRX_OK;
    SRX_TRY(alloc_moments(m));
    double* packed;
    SRX_TRY(local_moments(m, &packed));
    SRX_TRY(reduce_unpack_moments(m, packed, true));
    moments_adopt(m);
    return SRX_OK;
}

// Moments of the transformed values y = ln_1p(v * scale_row), computed from the RAW matrix (pipeline).  With xf.write_back
// the pass stores y in place, and from the moment its kernel is in the stream X is booked as normalised + log1p'd (`stored`
// true) — whatever fails behind it (all-reduce, read-back), the caller must not transform X a second time: the bookkeeping of
// normalize_total + log1p (scale/mod.rs:74-83 -> F64, transform/mod.rs:43-55) belongs to that moment.  The moments are those
// of the f64 transform, not of the values as stored: the caller adopts them for the solve that follows and retires them after.
int32_t ensure_moments_xf(srx_mat* m, RowXf xf, bool* stored) {
    *stored = false;
    SRX_TRY(alloc_moments(m));
    double* packed;
    SRX_TRY(local_moments(m, &packed, xf));
    if (xf.write_back) {
        m->dtype = SRX_F64;
        touch(m);
        *stored = true;
    }
    return reduce_unpack_moments(m, packed, true);
}

// The global per-column moments of the STORED matrix (for a CSC matrix: per cell) on the host; null destinations are skipped.
static int32_t fetch_moments(srx_mat* m, uint64_t* cnt, double* sum, double* sq) {
    SRX_TRY(ensure_moments(m));
    const uint64_t G = m->n_cols;
    if (cnt) SRX_TRY(d2h(m->ctx, cnt, m->d_cnt, G * sizeof(uint64_t)));
    if (sum) SRX_TRY(d2h(m->ctx, sum, m->d_sum, G * sizeof(double)));
    if (sq) SRX_TRY(d2h(m->ctx, sq, m->d_sq, G * sizeof(double)));
    return SRX_OK;
}

// csr.rs:179-185, evaluated in the reference's operation order (no FMA contraction).
#pragma clang fp contract(off)
void finalize_variance(const uint64_t* cnt, const double* sum, const double* sq, uint64_t G, double* out) {
    for (uint64_t j = 0; j < G; ++j) {
        out[j] = 0.0;
        if (cnt[j] > 0) {
            double c = (double)(uint32_t)cnt[j];
            double mean = sum[j] / c;
            out[j] = sq[j] / c - mean * mean;
        }
    }
}

int32_t gene_variances(srx_mat* m, std::vector<double>& var) {
    const uint64_t G = m->n_cols;
    std::vector<uint64_t> cnt(G);
    std::vector<double> sum(G), sq(G);
    SRX_TRY(fetch_moments(m, cnt.data(), sum.data(), sq.data()));
    var.resize(G);
    finalize_variance(cnt.data(), sum.data(), sq.data(), G, var.data());
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_gene_moments(srx_mat* m, uint64_t* cnt, double* sum, double* sumsq) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    if (m->csc) return fail(m->ctx, SRX_E_FORMAT, "srx_gene_moments walks cells: convert the CSC matrix with srx_matrix_to_csr");
    return fetch_moments(m, cnt, sum, sumsq);
}

int32_t srx_compute_number(srx_mat* m, int32_t direction, uint32_t* out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    direction = eff_dir(m, direction);           // CSC: csc.rs:15-35 is csr.rs:16-38 with the directions exchanged
    if (direction == SRX_ROW) return row_number(m, out);
    if (direction != SRX_COLUMN) return fail(m->ctx, SRX_E_ARG, "bad direction %d", direction);
    std::vector<uint64_t> cnt(m->n_cols);
    SRX_TRY(fetch_moments(m, cnt.data(), nullptr, nullptr));
    for (uint64_t j = 0; j < m->n_cols; ++j) out[j] = (uint32_t)cnt[j];   // reference counts in u32
    return SRX_OK;
}

int32_t srx_compute_sum(srx_mat* m, int32_t direction, double* out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    direction = eff_dir(m, direction);           // csc.rs:71-95
    if (direction == SRX_ROW) return row_stat(m, 0, out, nullptr);
    if (direction != SRX_COLUMN) return fail(m->ctx, SRX_E_ARG, "bad direction %d", direction);
    return fetch_moments(m, nullptr, out, nullptr);
}

int32_t srx_compute_variance(srx_mat* m, int32_t direction, double* out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    direction = eff_dir(m, direction);           // csc.rs:138-180: naive + guard on the scattered axis, two-pass on the major one
    if (direction == SRX_ROW) return row_stat(m, 1, out, nullptr);
    if (direction != SRX_COLUMN) return fail(m->ctx, SRX_E_ARG, "bad direction %d", direction);
    std::vector<double> var;
    SRX_TRY(gene_variances(m, var));
    memcpy(out, var.data(), var.size() * sizeof(double));
    return SRX_OK;
}

int32_t srx_compute_std_dev(srx_mat* m, int32_t direction, double* out) {
    SRX_TRY(srx_compute_variance(m, direction, out));
    uint64_t n = eff_dir(m, direction) == SRX_ROW ? m->n_rows : m->n_cols;
    for (uint64_t i = 0; i < n; ++i) out[i] = std::sqrt(out[i]);   // csr.rs:227
    return SRX_OK;
}

int32_t srx_compute_qc_variables(srx_mat* m, uint32_t* num_per_cell, uint32_t* num_per_gene, double* expr_per_gene,
                                 double* expr_per_cell, double* variance_per_gene, double* variance_per_cell,
                                 double* std_dev_per_cell, double* std_dev_per_gene) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (m->csc) {                                // stored rows are genes: exchange the roles of the outputs
        std::swap(num_per_cell, num_per_gene);
        std::swap(expr_per_cell, expr_per_gene);
        std::swap(variance_per_cell, variance_per_gene);
        std::swap(std_dev_per_cell, std_dev_per_gene);
    }
    // per cell: ONE row pass
    if (num_per_cell || expr_per_cell || variance_per_cell || std_dev_per_cell) {
        std::vector<double> var;
        double* vp = variance_per_cell;
        if (!vp && std_dev_per_cell) { var.resize(m->n_rows); vp = var.data(); }
        SRX_TRY(row_qc(m, num_per_cell, expr_per_cell, vp));
        if (std_dev_per_cell)
            for (uint64_t i = 0; i < m->n_rows; ++i) std_dev_per_cell[i] = std::sqrt(vp[i]);       // csr.rs:225-228
    }
    // per gene: ONE column pass (the cached moments)
    if (num_per_gene || expr_per_gene || variance_per_gene || std_dev_per_gene) {
        const uint64_t G = m->n_cols;
        std::vector<uint64_t> cnt(G);
        std::vector<double> sum(G), sq(G);
        SRX_TRY(fetch_moments(m, cnt.data(), sum.data(), sq.data()));
        if (num_per_gene) for (uint64_t j = 0; j < G; ++j) num_per_gene[j] = (uint32_t)cnt[j];
        if (expr_per_gene) memcpy(expr_per_gene, sum.data(), G * sizeof(double));
        if (variance_per_gene || std_dev_per_gene) {
            std::vector<double> var(G);
            finalize_variance(cnt.data(), sum.data(), sq.data(), G, var.data());
            if (variance_per_gene) memcpy(variance_per_gene, var.data(), G * sizeof(double));
            if (std_dev_per_gene) for (uint64_t j = 0; j < G; ++j) std_dev_per_gene[j] = std::sqrt(var[j]);
        }
    }
    return SRX_OK;
}

int32_t srx_compute_min_max(srx_mat* m, int32_t direction, double* mn, double* mx) {
    if (!m || !mn || !mx) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    direction = eff_dir(m, direction);           // csc.rs:186-212
    if (direction == SRX_ROW) return row_stat(m, 2, mn, mx);
    if (direction != SRX_COLUMN) return fail(ctx, SRX_E_ARG, "bad direction %d", direction);
    // per-gene extrema of a row shard are the shard's own (the path has sum all-reduces only): refuse rather than
    // return a different answer on every rank
    if (ctx->n_ranks > 1)
        return fail(ctx, SRX_E_ARG, "compute_min_max(Column) on a row-sharded context is shard-local: reduce the per-rank "
                                    "results on the host (min of mins, max of maxs) — rank %d of %d", ctx->rank, ctx->n_ranks);
    SRX_TRY(ensure_tiles(m));
    const uint64_t G = m->n_cols;
    unsigned long long* d;
    SRX_TRY(scratch(ctx, "minmax_keys", 2 * at_least_one(G) * sizeof(unsigned long long), (void**)&d));
    unsigned g1 = (unsigned)((G + 255) / 256 + 1);
    hipLaunchKernelGGL(k_fill_u64, dim3(g1), dim3(256), 0, ctx->stream, d, G, (unsigned long long)f64_key(INFINITY));
    hipLaunchKernelGGL(k_fill_u64, dim3(g1), dim3(256), 0, ctx->stream, d + G, G, (unsigned long long)f64_key(-INFINITY));
    uint64_t nb, rpb;
    SRX_TRY(block_geometry(m, nb, rpb));
    const size_t lds = (size_t)m->tile_genes * 16;
    dim3 grid((unsigned)(nb * m->n_tiles));
    SRX_TRY(by_values(m, [&](auto* vals) -> int32_t {
        using T = std::remove_pointer_t<decltype(vals)>;
        SRX_HIP(ctx, hipFuncSetAttribute((const void*)k_gene_minmax<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL((k_gene_minmax<T>), grid, dim3(kMomThreads), lds, ctx->stream, m->d_indptr, m->d_tile_ptr,
                           m->d_indices, (const T*)vals, m->n_rows, G, m->n_tiles, m->tile_genes, rpb, d, d + G);
        return SRX_OK;
    }));
    SRX_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> keys(2 * G);
    SRX_TRY(d2h(ctx, keys.data(), d, 2 * G * sizeof(unsigned long long)));
    for (uint64_t j = 0; j < G; ++j) { mn[j] = key_f64(keys[j]); mx[j] = key_f64(keys[G + j]); }
    return SRX_OK;
}

int32_t srx_normalize_total_inplace(srx_mat* m, double target_sum, int32_t direction) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    srx_ctx* ctx = m->ctx;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    direction = eff_dir(m, direction);           // scale_row_csc / scale_col_csc, scale/mod.rs:25-57,104-139
    SRX_TRY(promote_to_f64(m));                  // X becomes DynCsrMatrix::F64 (scale/mod.rs:74-83)
    if (direction == SRX_ROW) return launch_normalize(m, target_sum, true, false);
    if (direction != SRX_COLUMN) return fail(ctx, SRX_E_ARG, "bad direction %d", direction);
    SRX_TRY(ensure_moments(m));
    uint64_t g = (m->nnz + 255) / 256;
    if (g < 1) g = 1;
    if (g > 8192) g = 8192;
    by_values(m, [&](auto* vals) {
        using T = std::remove_pointer_t<decltype(vals)>;
        hipLaunchKernelGGL((k_col_scale<T>), dim3((unsigned)g), dim3(256), 0, ctx->stream, m->d_indices, vals, m->nnz, m->d_sum, target_sum);
        return SRX_OK;
    });
    SRX_HIP(ctx, hipGetLastError());
    m->dtype = SRX_F64;
    touch(m);
    return SRX_OK;
}

}  // extern "C"
