// wilcoxon.inl — the rank-sum route of markers.hip (srx_rank_genes_wilcoxon[_graph]): exact doubled rank sums per (group, gene)
// and the tie term per gene, in integers.  Included by markers.hip inside namespace srx, below its kernels; the definition is
// in include/srx.h, the design in DESIGN.md ("Marker genes: the rank-sum route").
//
// Per chunk of consecutive genes whose stored entries fit the staging buffer:
//   stage   the rows are walked through the gene tiles (as k_mk_walk, in row order) and every stored entry of the chunk's genes
//           goes to its gene's segment as (sortable key, 16-bit label); a workgroup counts its entries per gene in LDS, reserves
//           its share of every touched segment with ONE global atomic per gene and places the entries with LDS cursors.  The
//           order inside a segment is whatever the atomics gave: nothing below depends on it.
//   sort    a segment of 2 .. kWxLimit entries is sorted by one workgroup in LDS (bitonic; the host lists them); a longer one by a least-
//           significant-digit radix sort, 8 bits a pass, over tiles of kWxRadixTile entries that never leave their segment, so
//           that ONE device scan of the (segment, digit, tile) histogram table places every tile of every long segment.
//   ranks   one workgroup per gene walks the sorted segment, finds every entry's tie run (its ends looked up in the sorted
//           segment itself, so a run may cross any boundary of the sort and of this walk), splices in the zeros and adds the
//           doubled rank to the LDS accumulator of the entry's group.
// Keys are compared only; every sum is an integer.

constexpr int kWxThreads = 256;
constexpr uint32_t kWxLimit = 4096;          // the one-workgroup sort: 4096 x (8 + 2) B = 40 KiB of LDS at f64 keys, four workgroups a CU
constexpr uint32_t kWxRadixTile = 4096;      // entries per workgroup of a radix pass
constexpr uint32_t kWxRankTile = 1024;       // entries per round of the rank walk
constexpr uint64_t kWxDefaultScratch = 2ull << 30;

// the order-preserving unsigned image of a finite value; -0.0 and +0.0 share the image of +0.0
__device__ __forceinline__ uint32_t wx_key(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint64_t wx_key(double x) {
    uint64_t u = (uint64_t)__double_as_longlong(x);
    if ((u << 1) == 0ull) u = 0ull;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
template <typename K>
__device__ __forceinline__ constexpr K wx_zero_key() { return (K)1 << (sizeof(K) * 8 - 1); }

// first place in [lo, hi) of the ascending k whose key is not below / is above `key` (hi when there is none)
template <typename K>
__device__ __forceinline__ uint64_t wx_lower(const K* k, uint64_t lo, uint64_t hi, K key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename K>
__device__ __forceinline__ uint64_t wx_upper(const K* k, uint64_t lo, uint64_t hi, K key) {
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (k[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_wx_counts64(const uint32_t* __restrict__ cnt, uint32_t n, int64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (int64_t)cnt[i];
}

// ---- stage ------------------------------------------------------------------------------------------------------------------
// Workgroup = (gene tile t0 + x % n_t of the chunk, rows_per_block rows).  Genes j0 .. j1 - 1 are the chunk's; `off` (their
// exclusive scan) and `cursor` (zero on entry) are indexed by gene - j0.  A wave takes a row, a lane every 64th entry of it.
template <typename T, typename I, typename K>
__global__ __launch_bounds__(kWxThreads) void k_wx_stage(const int64_t* __restrict__ indptr, const int64_t* __restrict__ tp,
                                                         const I* __restrict__ idx, const T* __restrict__ vals,
                                                         const uint32_t* __restrict__ labels, uint64_t n_rows, int n_tiles, int tile_genes,
                                                         int t0, int n_t, uint32_t j0, uint32_t j1, uint64_t rows_per_block,
                                                         const int64_t* __restrict__ off, uint32_t* __restrict__ cursor,
                                                         K* __restrict__ keys, uint16_t* __restrict__ labs) {
    extern __shared__ uint32_t s_cur[];          // tile_genes
    const int tile = t0 + (int)(blockIdx.x % (unsigned)n_t);
    const uint64_t r0 = (uint64_t)(blockIdx.x / (unsigned)n_t) * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    const uint32_t gbase = (uint32_t)tile * (uint32_t)tile_genes;
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    constexpr int kWaves = kWxThreads / kWave;
    for (int g = threadIdx.x; g < tile_genes; g += kWxThreads) s_cur[g] = 0u;
    __syncthreads();
    for (uint64_t r = r0 + wave; r < r1; r += kWaves) {
        int64_t lo, hi;
        seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
        for (int64_t e = lo + lane; e < hi; e += kWave) {
            const uint32_t g = (uint32_t)idx[e];
            if (g >= j0 && g < j1) __hip_atomic_fetch_add(&s_cur[g - gbase], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    // the workgroup's share of every segment it touches: from here s_cur is the next free place of the gene's segment
    for (int g = threadIdx.x; g < tile_genes; g += kWxThreads) {
        const uint32_t c = s_cur[g];
        if (c) s_cur[g] = atomicAdd(&cursor[gbase + (uint32_t)g - j0], c);
    }
    __syncthreads();
    for (uint64_t r = r0 + wave; r < r1; r += kWaves) {
        int64_t lo, hi;
        seg_bounds(indptr, tp, n_rows, n_tiles, tile, r, lo, hi);
        const uint16_t lab = (uint16_t)labels[r];
        for (int64_t e = lo + lane; e < hi; e += kWave) {
            const uint32_t g = (uint32_t)idx[e];
            if (g >= j0 && g < j1) {
                const uint32_t p = __hip_atomic_fetch_add(&s_cur[g - gbase], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const int64_t at = off[g - j0] + (int64_t)p;
                keys[at] = wx_key(vals[e]);
                labs[at] = lab;
            }
        }
    }
}

// ---- sort: a segment of 2 .. kWxLimit entries, one workgroup, in LDS ----------------------------------------------------------
// Bitonic over the next power of two; the places behind the segment hold the all-ones key, above the image of every finite value.
// `list`: the chunk's genes (less j0) with 2 .. kWxLimit entries, one workgroup each.
template <typename K>
__global__ __launch_bounds__(kWxThreads) void k_wx_sort_short(K* __restrict__ keys, uint16_t* __restrict__ labs, const int64_t* __restrict__ off,
                                                              const uint32_t* __restrict__ list) {
    __shared__ K s_key[kWxLimit];
    __shared__ uint16_t s_lab[kWxLimit];
    const uint32_t jl = list[blockIdx.x];
    const int64_t base = off[jl];
    const uint64_t c64 = (uint64_t)(off[jl + 1] - base);
    if (c64 < 2 || c64 > kWxLimit) return;
    const uint32_t c = (uint32_t)c64;
    uint32_t P = 2;
    while (P < c) P <<= 1;
    for (uint32_t i = threadIdx.x; i < P; i += kWxThreads) {
        s_key[i] = i < c ? keys[base + i] : ~(K)0;
        s_lab[i] = i < c ? labs[base + i] : (uint16_t)0;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < (P >> 1); t += kWxThreads) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const K a = s_key[i], b = s_key[l];
                const bool up = (i & k) == 0;
                if ((a > b) == up && a != b) {
                    s_key[i] = b; s_key[l] = a;
                    const uint16_t x = s_lab[i];
                    s_lab[i] = s_lab[l]; s_lab[l] = x;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = threadIdx.x; i < c; i += kWxThreads) {
        keys[base + i] = s_key[i];
        labs[base + i] = s_lab[i];
    }
}

// ---- sort: the radix passes over the long segments --------------------------------------------------------------------------
// Tile b_local of a segment of nb tiles: its digit counts go to table[tbase + digit * nb + b_local], so the exclusive scan of the
// whole table, less its value at tbase, is the place of (digit, tile) inside the segment.
struct WxBlock {
    int64_t begin;         // first entry, in the staging arrays
    uint64_t tbase;        // the segment's first table entry
    uint32_t n, seg;       // entries; gene - j0
    uint32_t b_local, nb;
};
template <typename K>
__global__ __launch_bounds__(kWxThreads) void k_wx_radix_hist(const K* __restrict__ keys, const WxBlock* __restrict__ blocks, int shift,
                                                              int64_t* __restrict__ table) {
    __shared__ uint32_t s_hist[256];
    const WxBlock b = blocks[blockIdx.x];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < b.n; i += kWxThreads)
        __hip_atomic_fetch_add(&s_hist[(uint32_t)(keys[b.begin + i] >> shift) & 255u], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    table[b.tbase + (uint64_t)threadIdx.x * b.nb + b.b_local] = (int64_t)s_hist[threadIdx.x];
}
// The stable scatter: 256 entries a round, in order.  Within a wave the lanes of one digit are found by eight ballots; the
// lowest of them leaves their number for the waves behind it.
template <typename K>
__global__ __launch_bounds__(kWxThreads) void k_wx_radix_scatter(const K* __restrict__ keys_in, const uint16_t* __restrict__ labs_in,
                                                                 K* __restrict__ keys_out, uint16_t* __restrict__ labs_out,
                                                                 const WxBlock* __restrict__ blocks, int shift, const int64_t* __restrict__ first,
                                                                 const int64_t* __restrict__ off) {
    constexpr int kWaves = kWxThreads / kWave;
    __shared__ int64_t s_base[256];
    __shared__ uint32_t s_wc[kWaves][256];
    const WxBlock b = blocks[blockIdx.x];
    const int lane = lane_id();
    const int wave = threadIdx.x / kWave;
    s_base[threadIdx.x] = off[b.seg] + first[b.tbase + (uint64_t)threadIdx.x * b.nb + b.b_local] - first[b.tbase];
    for (int w = 0; w < kWaves; ++w) s_wc[w][threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t r0 = 0; r0 < b.n; r0 += kWxThreads) {
        const uint32_t i = r0 + threadIdx.x;
        const bool valid = i < b.n;
        K key = 0;
        uint16_t lab = 0;
        if (valid) {
            key = keys_in[b.begin + i];
            lab = labs_in[b.begin + i];
        }
        const uint32_t d = (uint32_t)(key >> shift) & 255u;
        unsigned long long mask = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool set = (d >> bit) & 1u;
            const unsigned long long bb = __ballot(set);
            mask &= set ? bb : ~bb;
        }
        const uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (valid && before == 0) s_wc[wave][d] = (uint32_t)__popcll(mask);
        __syncthreads();
        if (valid) {
            int64_t at = s_base[d] + before;
            for (int w = 0; w < wave; ++w) at += s_wc[w][d];
            keys_out[at] = key;
            labs_out[at] = lab;
        }
        __syncthreads();
        uint32_t sum = 0;
        for (int w = 0; w < kWaves; ++w) {
            sum += s_wc[w][threadIdx.x];
            s_wc[w][threadIdx.x] = 0u;
        }
        s_base[threadIdx.x] += sum;
        __syncthreads();
    }
}

// ---- ranks ------------------------------------------------------------------------------------------------------------------
// One workgroup per gene of the chunk.  The sorted segment holds `neg` keys below the zero key and `zst` stored zeros; with the
// n0 = N - c implicit zeros the column's order is  negatives | zst + n0 zeros | positives.  An entry whose tie run is [s, e) of
// the segment has b = s (+ n0 behind the zeros) smaller values and t = e - s (+ n0 among the zeros) ties: r2 = 2 b + t + 1.
// Inside a round of kWxRankTile entries the run's ends come from the round's keys in LDS; a run that starts at the round's
// first entry may have begun earlier (carried from the round before), one that reaches its last entry may go on (looked up in
// the segment).  C: the (group, gene) stored counts; a group's cells without a stored entry are zeros of rank r2_zero.
template <typename K>
__global__ __launch_bounds__(kWxThreads) void k_wx_ranks(const K* __restrict__ keys, const uint16_t* __restrict__ labs,
                                                         const int64_t* __restrict__ off, uint32_t j0, uint32_t n_groups, uint64_t N, uint64_t G,
                                                         const uint32_t* __restrict__ C, const uint64_t* __restrict__ sizes, int tie_correct,
                                                         unsigned long long* __restrict__ R2, unsigned long long* __restrict__ Tout) {
    extern __shared__ unsigned long long s_acc[];          // n_groups
    __shared__ K s_key[kWxRankTile];
    __shared__ unsigned long long s_T;
    const uint64_t j = (uint64_t)j0 + blockIdx.x;
    const int64_t base = off[blockIdx.x];
    const uint64_t c = (uint64_t)(off[blockIdx.x + 1] - base);
    const K* k = keys + base;
    const uint16_t* lb = labs + base;
    for (uint32_t g = threadIdx.x; g < n_groups; g += kWxThreads) s_acc[g] = 0ull;
    if (threadIdx.x == 0) s_T = 0ull;
    constexpr K Z = wx_zero_key<K>();
    // (every thread walks the same places: the loads are broadcasts)
    const uint64_t neg = wx_lower(k, (uint64_t)0, c, Z), zst = wx_upper(k, neg, c, Z) - neg, n0 = N - c;
    __syncthreads();
    uint64_t carry_start = 0;
    K carry_key = 0;
    bool has_carry = false;
    for (uint64_t a = 0; a < c; a += kWxRankTile) {
        const uint32_t n = (uint32_t)(c - a < kWxRankTile ? c - a : kWxRankTile);
        for (uint32_t i = threadIdx.x; i < n; i += kWxThreads) s_key[i] = k[a + i];
        __syncthreads();
        const K first_key = s_key[0], last_key = s_key[n - 1];
        const uint64_t first_start = (has_carry && carry_key == first_key) ? carry_start : a;
        uint64_t last_end = a + n;
        if (last_end < c && k[last_end] == last_key) last_end = wx_upper(k, last_end + 1, c, last_key);
        for (uint32_t i = threadIdx.x; i < n; i += kWxThreads) {
            const K key = s_key[i];
            const uint32_t lo = (uint32_t)wx_lower((const K*)s_key, (uint64_t)0, (uint64_t)i, key);
            const uint32_t hi = (uint32_t)wx_upper((const K*)s_key, (uint64_t)i + 1, (uint64_t)n, key);
            const uint64_t s = lo == 0 ? first_start : a + lo, e = hi == n ? last_end : a + hi;
            const uint64_t b = s + (key > Z ? n0 : 0ull), t = e - s + (key == Z ? n0 : 0ull);
            __hip_atomic_fetch_add(&s_acc[lb[a + i]], (unsigned long long)(2ull * b + t + 1ull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (tie_correct && a + i + 1 == e)                 // the run's last entry speaks for the run
                __hip_atomic_fetch_add(&s_T, (unsigned long long)(t * t * t - t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const uint32_t lo_last = (uint32_t)wx_lower((const K*)s_key, (uint64_t)0, (uint64_t)(n - 1), last_key);
        carry_start = lo_last == 0 ? first_start : a + lo_last;
        carry_key = last_key;
        has_carry = true;
        __syncthreads();
    }
    __syncthreads();
    const uint64_t r2_zero = 2ull * neg + zst + n0 + 1ull;
    for (uint32_t g = threadIdx.x; g < n_groups; g += kWxThreads) {
        const uint64_t at = (uint64_t)g * G + j;
        R2[at] = s_acc[g] + (sizes[g] - (uint64_t)C[at]) * r2_zero;
    }
    if (tie_correct && threadIdx.x == 0) Tout[j] = s_T + ((zst == 0 && n0 > 0) ? n0 * n0 * n0 - n0 : 0ull);
}

// ---- the score of srx.h for one (group, gene), in the stated order ------------------------------------------------------------
struct WxTables {
    const unsigned long long *R2, *T;
    const uint64_t* sizes;
    uint64_t G, N;
    int tie_correct;
};
__device__ __forceinline__ double wx_score(const WxTables& t, uint32_t g, uint64_t j) {
    const uint64_t ng = t.sizes[g], nr = t.N - ng;
    if (ng == 0 || nr == 0) return 0.0;
    const double num = mk_mul((double)(long long)(t.R2[(uint64_t)g * t.G + j] - ng * (t.N + 1)), 0.5);
    double tc = 1.0;
    if (t.tie_correct && t.N >= 2) tc = mk_sub(1.0, mk_div((double)t.T[j], (double)(t.N * t.N * t.N - t.N)));
    const double d = mk_mul(mk_div(mk_mul((double)(ng * nr), (double)(t.N + 1)), 12.0), tc);
    return d > 0.0 ? mk_div(num, __dsqrt_rn(d)) : 0.0;
}
// the score table (f64) or the doubled rank sums themselves (u64), groups g0 .. g0 + n_g - 1
__global__ __launch_bounds__(256) void k_wx_table(WxTables t, int which, uint32_t g0, uint32_t n_g, void* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)n_g * t.G) return;
    const uint32_t g = g0 + (uint32_t)(i / t.G);
    const uint64_t j = i % t.G;
    if (which == SRX_MARKERS_RANKSUM2) reinterpret_cast<unsigned long long*>(out)[i] = t.R2[(uint64_t)g * t.G + j];
    else reinterpret_cast<double*>(out)[i] = wx_score(t, g, j);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct WxOpts {
    int tie_correct = 0;
    uint64_t scratch_bytes = 0;
};
struct WxChunk {
    uint32_t j0, j1;
    uint64_t entries, n_blocks;
};
struct WxEvents {
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    ~WxEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};
// the large buffers of one call (staging, tile table and its scan, tile records): returned before the call ends, so that a
// context does not keep gigabytes after one call at atlas size (the named scratch buffers never shrink)
struct WxBuffers {
    srx_ctx* ctx;
    void* p = nullptr;
    ~WxBuffers() {
        if (!p) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
    }
};

static WxTables wx_tables(const srx_markers* mk) {
    WxTables t;
    t.R2 = (const unsigned long long*)mk->d_R2; t.T = (const unsigned long long*)mk->d_T;
    t.sizes = mk->d_sizes;
    t.G = mk->n_cols; t.N = mk->n_rows;
    t.tie_correct = mk->winfo.tie_correct;
    return t;
}

// Fills mk->d_R2 and mk->d_T; the grouped counts (d_C, d_totC) and the sizes are in place.  K: the key type of the storage.
template <typename T, typename K>
static int32_t wilcoxon_chunks(srx_mat* m, const uint32_t* d_labels, srx_markers* mk, const WxOpts& wx) {
    srx_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t N = m->n_rows, G = m->n_cols;
    srx_wilcoxon_info& wi = mk->winfo;
    // the per-gene stored counts: the totals of the grouped counts this call has just made (what the matrix's pattern
    // counts hold as well, without another pass over the indices)
    std::vector<uint32_t> cnt(G);
    SRX_TRY(d2h(ctx, cnt.data(), mk->d_totC, G * 4));
    const uint64_t eb = 2 * (sizeof(K) + 2);              // both sides of the radix ping-pong, key and label
    uint64_t longest = 0;
    for (uint32_t c : cnt) {
        longest = std::max<uint64_t>(longest, c);
        if (c > kWxLimit) wi.segments_long++;
        else if (c) wi.segments_short++;
    }
    uint64_t budget = wx.scratch_bytes ? wx.scratch_bytes : kWxDefaultScratch;
    budget = std::max(budget, at_least_one(longest) * eb);
    const uint64_t cap = budget / eb;
    std::vector<WxChunk> chunks;
    uint64_t max_entries = 0, max_genes = 0, max_blocks = 0;
    for (uint64_t j = 0; j < G;) {
        WxChunk ch{(uint32_t)j, (uint32_t)j, 0, 0};
        while (j < G && (ch.j1 == ch.j0 || ch.entries + cnt[j] <= cap)) {
            ch.entries += cnt[j];
            if (cnt[j] > kWxLimit) ch.n_blocks += (cnt[j] + kWxRadixTile - 1) / kWxRadixTile;
            ch.j1 = (uint32_t)++j;
        }
        max_entries = std::max(max_entries, ch.entries);
        max_genes = std::max<uint64_t>(max_genes, ch.j1 - ch.j0);
        max_blocks = std::max(max_blocks, ch.n_blocks);
        chunks.push_back(ch);
    }
    wi.n_chunks = (uint32_t)chunks.size();
    wi.scratch_bytes = max_entries * eb;
    wi.segment_limit = kWxLimit;

    const size_t n_pad = (size_t)((at_least_one(max_entries) + 127) & ~(uint64_t)127);
    int64_t *d_cnt64, *d_off;
    uint32_t *d_cursor, *d_short;
    SRX_TRY(scratch(ctx, "wx_cnt64", max_genes * 8, (void**)&d_cnt64));
    SRX_TRY(scratch(ctx, "wx_off", (max_genes + 1) * 8, (void**)&d_off));
    SRX_TRY(scratch(ctx, "wx_cursor", max_genes * 4, (void**)&d_cursor));
    SRX_TRY(scratch(ctx, "wx_short", max_genes * 4, (void**)&d_short));
    WxBuffers big{ctx};
    const size_t b_stage = n_pad * eb, b_tab = (size_t)max_blocks * 256 * 8, b_first = ((size_t)max_blocks * 256 + 32) * 8,
                 b_blocks = (size_t)max_blocks * sizeof(WxBlock);
    {
        const size_t bytes = b_stage + b_tab + b_first + b_blocks;
        hipError_t e = hipMalloc(&big.p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            big.p = nullptr;
            return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "wilcoxon: the staging of %llu entries (%zu bytes) does not fit: %s",
                        (unsigned long long)max_entries, bytes, hipGetErrorString(e));
        }
    }
    char* d_stage = (char*)big.p;
    int64_t* d_tab = (int64_t*)(d_stage + b_stage);
    int64_t* d_first = (int64_t*)(d_stage + b_stage + b_tab);
    WxBlock* d_blocks = (WxBlock*)(d_stage + b_stage + b_tab + b_first);
    K* keys[2] = {(K*)d_stage, (K*)d_stage + n_pad};
    uint16_t* labs[2] = {(uint16_t*)(keys[1] + n_pad), (uint16_t*)(keys[1] + n_pad) + n_pad};

    WxEvents ev;
    for (hipEvent_t& e : ev.e) SRX_HIP(ctx, hipEventCreate(&e));
    const size_t lds_stage = (size_t)m->tile_genes * 4, lds_rank = (size_t)mk->n_groups * 8;
    std::vector<WxBlock> blocks;
    std::vector<uint32_t> shorts;
    for (const WxChunk& ch : chunks) {
        const uint32_t nj = ch.j1 - ch.j0;
        shorts.clear();
        for (uint32_t j = ch.j0; j < ch.j1; ++j)
            if (cnt[j] >= 2 && cnt[j] <= kWxLimit) shorts.push_back(j - ch.j0);
        if (!shorts.empty()) SRX_TRY(h2d(ctx, d_short, shorts.data(), shorts.size() * 4));
        // the long segments' tiles (the host holds the counts, so it knows every segment's place as the scan below does)
        blocks.clear();
        if (ch.n_blocks) {
            uint64_t at = 0, tbase = 0;
            for (uint32_t j = ch.j0; j < ch.j1; ++j) {
                if (cnt[j] > kWxLimit) {
                    const uint32_t nb = (cnt[j] + kWxRadixTile - 1) / kWxRadixTile;
                    for (uint32_t b = 0; b < nb; ++b)
                        blocks.push_back(WxBlock{(int64_t)(at + (uint64_t)b * kWxRadixTile), tbase,
                                                 std::min<uint32_t>(kWxRadixTile, cnt[j] - b * kWxRadixTile), j - ch.j0, b, nb});
                    tbase += (uint64_t)nb * 256;
                }
                at += cnt[j];
            }
            SRX_TRY(h2d(ctx, d_blocks, blocks.data(), blocks.size() * sizeof(WxBlock)));
        }
        SRX_HIP(ctx, hipEventRecord(ev.e[0], st));
        hipLaunchKernelGGL(k_wx_counts64, dim3((nj + 255) / 256), dim3(256), 0, st, (const uint32_t*)(mk->d_totC + ch.j0), nj, d_cnt64);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(scan_exclusive(ctx, d_cnt64, nj, d_off, nullptr));
        if (ch.entries) {
            SRX_HIP(ctx, hipMemsetAsync(d_cursor, 0, (size_t)nj * 4, st));
            const int t0 = (int)(ch.j0 / (uint32_t)m->tile_genes), n_t = (int)((ch.j1 - 1) / (uint32_t)m->tile_genes) - t0 + 1;
            const uint64_t rpb = mk_rows_per_block(N, n_t);
            const dim3 grid((unsigned)(((N + rpb - 1) / rpb) * (uint64_t)n_t));
            auto launch = [&](const auto* idxp) {
                using I = std::remove_cv_t<std::remove_pointer_t<decltype(idxp)>>;
                hipLaunchKernelGGL((k_wx_stage<T, I, K>), grid, dim3(kWxThreads), lds_stage, st, (const int64_t*)m->d_indptr,
                                   (const int64_t*)m->d_tile_ptr, idxp, (const T*)m->d_values, d_labels, N, m->n_tiles, m->tile_genes, t0, n_t, ch.j0,
                                   ch.j1, rpb, (const int64_t*)d_off, d_cursor, keys[0], labs[0]);
            };
            if (m->d_idx16) launch((const uint16_t*)m->d_idx16);
            else launch((const int32_t*)m->d_indices);
            SRX_HIP(ctx, hipGetLastError());
        }
        SRX_HIP(ctx, hipEventRecord(ev.e[1], st));
        if (!shorts.empty()) {
            hipLaunchKernelGGL(k_wx_sort_short<K>, dim3((unsigned)shorts.size()), dim3(kWxThreads), 0, st, keys[0], labs[0], (const int64_t*)d_off,
                               (const uint32_t*)d_short);
            SRX_HIP(ctx, hipGetLastError());
        }
        if (!blocks.empty()) {
            const uint64_t n_tab = (uint64_t)blocks.size() * 256;
            int src = 0;
            for (int shift = 0; shift < (int)sizeof(K) * 8; shift += 8, src ^= 1) {      // an even number of passes: the result is in keys[0]
                hipLaunchKernelGGL(k_wx_radix_hist<K>, dim3((unsigned)blocks.size()), dim3(kWxThreads), 0, st, (const K*)keys[src],
                                   (const WxBlock*)d_blocks, shift, d_tab);
                SRX_TRY(scan_exclusive(ctx, d_tab, n_tab, d_first, nullptr));
                hipLaunchKernelGGL(k_wx_radix_scatter<K>, dim3((unsigned)blocks.size()), dim3(kWxThreads), 0, st, (const K*)keys[src],
                                   (const uint16_t*)labs[src], keys[src ^ 1], labs[src ^ 1], (const WxBlock*)d_blocks, shift,
                                   (const int64_t*)d_first, (const int64_t*)d_off);
                SRX_HIP(ctx, hipGetLastError());
            }
        }
        SRX_HIP(ctx, hipEventRecord(ev.e[2], st));
        hipLaunchKernelGGL(k_wx_ranks<K>, dim3(nj), dim3(kWxThreads), lds_rank, st, (const K*)keys[0], (const uint16_t*)labs[0], (const int64_t*)d_off,
                           ch.j0, mk->n_groups, N, G, (const uint32_t*)mk->d_C, (const uint64_t*)mk->d_sizes, wi.tie_correct,
                           (unsigned long long*)mk->d_R2, (unsigned long long*)mk->d_T);
        SRX_HIP(ctx, hipGetLastError());
        SRX_HIP(ctx, hipEventRecord(ev.e[3], st));
        SRX_HIP(ctx, hipEventSynchronize(ev.e[3]));
        float a = 0.f, b = 0.f, c = 0.f;
        SRX_HIP(ctx, hipEventElapsedTime(&a, ev.e[0], ev.e[1]));
        SRX_HIP(ctx, hipEventElapsedTime(&b, ev.e[1], ev.e[2]));
        SRX_HIP(ctx, hipEventElapsedTime(&c, ev.e[2], ev.e[3]));
        wi.ms_stage += a; wi.ms_sort += b; wi.ms_ranks += c;
    }
    return SRX_OK;
}

static int32_t wilcoxon_run(srx_mat* m, const uint32_t* d_labels, srx_markers* mk, const WxOpts& wx) {
    srx_ctx* ctx = m->ctx;
    const uint64_t G = mk->n_cols, cells = (uint64_t)mk->n_groups * at_least_one(G);
    const size_t bytes = (size_t)(cells + at_least_one(G)) * 8;
    hipError_t e = dev_malloc(ctx, &mk->d_wx, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        mk->d_wx = nullptr;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "wilcoxon: the %u x %llu rank sums (%zu bytes) do not fit: %s", mk->n_groups,
                    (unsigned long long)G, bytes, hipGetErrorString(e));
    }
    mk->d_R2 = (uint64_t*)mk->d_wx;
    mk->d_T = mk->d_R2 + cells;
    SRX_HIP(ctx, hipMemsetAsync(mk->d_wx, 0, bytes, ctx->stream));
    mk->winfo.tie_correct = wx.tie_correct ? 1 : 0;
    if (!G) return SRX_OK;
    return is_f32(m) ? wilcoxon_chunks<float, uint32_t>(m, d_labels, mk, wx) : wilcoxon_chunks<double, uint64_t>(m, d_labels, mk, wx);
}
