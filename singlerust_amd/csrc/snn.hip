// snn.hip — the shared-nearest-neighbour graph of a k-NN list (what Seurat's FindNeighbors, PhenoGraph and scran's buildSNNGraph
// cluster): srx_snn_from_knn / srx_snn_graph / srx_snn_min_shared.  include/srx.h has the definition in full.
//
// N(i) = knn(i), with i itself when include_self; K = |N(i)|; s_ij = |N(i) n N(j)|; a considered pair is stored when
// s_ij >= min_shared (which is J_ij = s / (2K - s) >= prune, J rising with s); the weight is J_ij or s_ij.
//
// With M(m) = {j : m in N(j)} = R(m), the reverse list of m, and m itself when include_self, row i of the result is the
// multiset union of M(m) over m in N(i) with i taken out: the multiplicity of j in it is s_ij.  c_i = sum |M(m)| is the row's
// candidate count.  Kernels:
//   k_snn_rows     (wave per row) checks the list as k_graph_rows does, puts the row in column order (this is the row of D),
//                  counts every target's in-degree (one integer atomic per edge)
//   k_graph_scatter / k_graph_order / k_graph_order_long  (graph.hip, through in_lists_build / in_lists_order_long) the reverse
//                  lists, ascending: every edge is flagged, the value array rides along unused
//   k_snn_cand     (thread per row) c_i; sorts the rows into three routes by it; finds the reverse lists that are long
//   k_snn_hash<64>   c_i <= kWaveCap: a wave per row.  The candidates are dealt to the lanes as ONE flat range (a binary search in
//                  the K list offsets finds a candidate's list), and go into an open-addressing table in LDS: u32 keys claimed
//                  by compare-and-swap, u8 counters (s <= K <= 65) added four to a word, bit 7 of a counter marks a pair joined
//                  by the list (SRX_SNN_PAIRS_KNN).  The table is sized to the row: the power of two from 2 c_i.
//   k_snn_hash<256>  c_i <= kBlockCap: the same by a workgroup per row
//   k_snn_window   beyond: a hub's neighbours, whose candidates run to K n.  A workgroup per row takes the index range in windows
//                  of kWin indices and counts in one u8 per index of the window.  The lists ascend, so each list's part of a
//                  window follows its part of the last one: a thread per list finds its end by bisection, and the parts are
//                  dealt to the threads as one flat range again.  The window is then read in index order
//   scan_exclusive (scan.hip) the row lengths of the count pass become the indptr
// Each route runs twice: the count pass leaves the number of stored entries per row (and the counters of srx_snn_info), the
// fill pass repeats the walk and writes.  The hash routes compact the kept slots in place and rank them by counting, so a
// row comes out ascending whatever order the table filled in; the window route meets the indices in order.  Every stored value
// depends on its pair's integer s alone: bit-identical from call to call, and both entries of a pair are the same bits.
#include "common.hpp"
#include "graph_handle.hpp"
#include "scan.hpp"

#include <algorithm>

namespace srx {

constexpr int kSnnMaxK = 64;
constexpr int kSnnLists = kSnnMaxK + 1;            // K at the most: k = 64 with self
constexpr uint32_t kWaveCap = 512, kWaveSlots = 1024;
constexpr uint32_t kBlockCap = 4096, kBlockSlots = 8192;
constexpr uint32_t kWin = 1u << 16;                // indices per window of the long route: 64 KiB of u8 counters
constexpr uint32_t kEmpty = 0xFFFFFFFFu;           // n < 2^32 - 1: no cell has this number
// the small block: kSnnSlots x {entries considered, rows empty} summed on the host | scalars | the list flag
constexpr int kSnnSlots = 64;
enum { kSmMaxShared = kSnnSlots * 2, kSmMaxRow, kSmMaxIndeg, kSmMaxCand, kSmSumCand, kSmWave, kSmMid, kSmLong, kSmRevLong, kSmFlag, kSmWords };

struct SnnArgs {
    const uint32_t* dind;      // D's indices: the list, rows ascending
    const int64_t* rptr;       // reverse lists: offsets, and the two arrays that hold them (in_list_src)
    const uint32_t *tsrc, *lsrc;
    uint64_t n;
    int k, self, pairs_knn, number;
    uint32_t min_shared;
    double two_k;              // (double)(2 K)
};

__device__ __forceinline__ unsigned long long below64(int p) { return p >= 64 ? ~0ull : (1ull << p) - 1ull; }
__device__ __forceinline__ void max_to(unsigned long long* p, unsigned long long v) {
    if (v > *(volatile unsigned long long*)p) atomicMax(p, v);       // most callers are below what is there already
}
// the stored weight of a pair from its shared count: integers until the one division
__device__ __forceinline__ double snn_value(const SnnArgs& a, uint32_t s) {
    return a.number ? (double)s : (double)s / (a.two_k - (double)s);
}

__global__ void __launch_bounds__(256) k_snn_rows(const uint32_t* __restrict__ idx_in, const double* __restrict__ dist_in, uint64_t n,
                                                  int k, uint64_t* __restrict__ dptr, uint32_t* __restrict__ dind,
                                                  double* __restrict__ ddat, int64_t* __restrict__ indeg, int* __restrict__ flag) {
    __shared__ uint32_t s_i[4][kWave];
    __shared__ double s_d[4][kWave];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const bool act = lane < k;
    const size_t e = (size_t)row * k + lane;
    uint32_t ci = act ? idx_in[e] : kEmpty;
    double cd = act && dist_in ? dist_in[e] : 0.0;
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
    if (bad) atomicOr(flag, bad);        // the host refuses the list before anything reads it as indices
    s_i[wave][lane] = kEmpty;            // (with duplicates some ranks stay unused: defined values all the same)
    s_d[wave][lane] = 0.0;
    wave_lds_sync();
    if (act) {
        s_i[wave][rank] = ci;
        s_d[wave][rank] = cd;
    }
    wave_lds_sync();
    if (act) {
        dind[e] = s_i[wave][lane];
        ddat[e] = s_d[wave][lane];
        if (ci < n) atomicAdd((unsigned long long*)&indeg[ci], 1ull);
    }
    if (lane == 0) {
        dptr[row] = row * (uint64_t)k;
        if (row + 1 == n) dptr[n] = n * (uint64_t)k;
    }
}

// cand[i] = c_i; the rows of the two workgroup routes and the long reverse lists are named in lists, in arbitrary order
__global__ void __launch_bounds__(256) k_snn_cand(const uint32_t* __restrict__ dind, const int64_t* __restrict__ indeg, uint64_t n, int k,
                                                  int self, uint64_t* __restrict__ cand, uint32_t* __restrict__ mid_rows,
                                                  uint32_t* __restrict__ long_rows, uint32_t* __restrict__ rev_long,
                                                  unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long c = 0, deg = 0;
    if (i < n) {
        deg = (unsigned long long)indeg[i];
        if (self) c = deg + 1;
        for (int q = 0; q < k; ++q) c += (unsigned long long)indeg[dind[i * k + q]] + (self ? 1ull : 0ull);
        cand[i] = c;
        if (c > kBlockCap) long_rows[atomicAdd(&small[kSmLong], 1ull)] = (uint32_t)i;
        else if (c > kWaveCap) mid_rows[atomicAdd(&small[kSmMid], 1ull)] = (uint32_t)i;
        if (deg > (unsigned long long)kInShort) rev_long[atomicAdd(&small[kSmRevLong], 1ull)] = (uint32_t)i;
    }
    const unsigned long long n_wave = wave_sum<unsigned long long>(i < n && c <= kWaveCap ? 1ull : 0ull);
    const unsigned long long c_sum = wave_sum(c), c_max = wave_max(c), d_max = wave_max(deg);
    if (lane_id() == 0) {
        if (n_wave) atomicAdd(&small[kSmWave], n_wave);
        if (c_sum) atomicAdd(&small[kSmSumCand], c_sum);
        max_to(&small[kSmMaxCand], c_max);
        max_to(&small[kSmMaxIndeg], d_max);
    }
}

// ---- what the three routes share: the lists of a row in LDS -----------------------------------------------------------------
struct RowLists {
    uint32_t mem[kSnnLists];               // N(i): the k neighbours, then i itself
    int64_t lo[kSnnLists];                 // where R(m) starts
    unsigned long long off[kSnnLists + 1]; // offsets of the lists M(m) in the row's flat candidate range
    unsigned long long own;                // |R(i)|
    int lists;                             // K
};
// By the first wave of a team, all 64 lanes active; the caller's barrier follows.
__device__ __forceinline__ void row_lists_load(const SnnArgs& a, uint32_t row, int lane, RowLists* L) {
    const bool act = lane < a.k;
    const uint32_t m = act ? a.dind[(size_t)row * a.k + lane] : 0u;
    const int64_t lo = act ? a.rptr[m] : 0;
    const unsigned long long len = act ? (unsigned long long)(a.rptr[m + 1] - lo) + (a.self ? 1ull : 0ull) : 0ull;
    const unsigned long long inc = wave_scan_inclusive(len);
    const unsigned long long tot = __shfl(inc, kWave - 1, kWave);
    if (act) {
        L->mem[lane] = m;
        L->lo[lane] = lo;
        L->off[lane + 1] = inc;
    }
    if (lane == 0) {
        const int64_t lo_i = a.rptr[row];
        const unsigned long long own = (unsigned long long)(a.rptr[row + 1] - lo_i);
        L->off[0] = 0;
        L->mem[a.k] = row;
        L->lo[a.k] = lo_i;
        L->off[a.k + 1] = tot + own + 1ull;      // read only with self
        L->own = own;
        L->lists = a.k + (a.self ? 1 : 0);
    }
}
// candidate t of the row's flat range
__device__ __forceinline__ uint32_t row_candidate(const SnnArgs& a, const RowLists* L, unsigned long long t) {
    int lo = 0, hi = L->lists;               // the list q with off[q] <= t < off[q + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (L->off[mid] <= t) lo = mid;
        else hi = mid;
    }
    const unsigned long long p = t - L->off[lo];
    if (a.self && p == 0) return L->mem[lo];
    const int64_t len = (int64_t)(L->off[lo + 1] - L->off[lo]) - a.self;
    return in_list_src(a.tsrc, a.lsrc, L->lo[lo], len)[p - (unsigned long long)a.self];
}

// ---- the hash routes ------------------------------------------------------------------------------------------------------------
template <int TEAM>
__device__ __forceinline__ void team_sync() {
    if constexpr (TEAM == kWave) wave_lds_sync();
    else __syncthreads();
}
__device__ __forceinline__ uint32_t tab_home(uint32_t j, int shift) { return (j * 0x9E3779B1u) >> shift; }
__device__ __forceinline__ void tab_add(uint32_t* keys, uint32_t* cnt, uint32_t mask, int shift, uint32_t j) {
    uint32_t s = tab_home(j, shift);
    for (;;) {                               // fewer keys than slots: an empty slot is always ahead
        const uint32_t old = atomicCAS(&keys[s], kEmpty, j);
        if (old == kEmpty || old == j) break;
        s = (s + 1) & mask;
    }
    atomicAdd(&cnt[s >> 2], 1u << ((s & 3) * 8));
}
__device__ __forceinline__ void tab_mark(const uint32_t* keys, uint32_t* cnt, uint32_t mask, int shift, uint32_t j) {
    uint32_t s = tab_home(j, shift);
    for (;;) {
        const uint32_t key = keys[s];
        if (key == j) {
            atomicOr(&cnt[s >> 2], 0x80u << ((s & 3) * 8));
            return;
        }
        if (key == kEmpty) return;           // shares nothing: not a considered pair
        s = (s + 1) & mask;
    }
}

// The counters of a row from the count pass: thread 0 of the team has the totals.
__device__ __forceinline__ void row_report(uint32_t row, unsigned long long kept, unsigned long long cons, unsigned long long smax,
                                           int64_t* len_out, unsigned long long* small) {
    len_out[row] = (int64_t)kept;
    unsigned long long* my = small + (size_t)(row & (kSnnSlots - 1)) * 2;
    if (cons) atomicAdd(&my[0], cons);
    if (!kept) atomicAdd(&my[1], 1ull);
    max_to(&small[kSmMaxShared], smax);
    max_to(&small[kSmMaxRow], kept);
}

template <int TEAM, uint32_t SLOTS, bool FILL>
__global__ void __launch_bounds__(256) k_snn_hash(SnnArgs a, const uint64_t* __restrict__ cand, const uint32_t* __restrict__ rows,
                                                  uint64_t n_rows, int64_t* __restrict__ len_out, const uint64_t* __restrict__ cptr,
                                                  uint32_t* __restrict__ cind, double* __restrict__ cdat,
                                                  unsigned long long* __restrict__ small) {
    constexpr int ROWS = 256 / TEAM;
    __shared__ uint32_t s_keys[ROWS][SLOTS];
    __shared__ uint32_t s_cnt[ROWS][SLOTS / 4];
    __shared__ RowLists s_lists[ROWS];
    __shared__ unsigned long long s_red[4];
    __shared__ uint32_t s_scan[4];
    const int team = TEAM == kWave ? (int)(threadIdx.x >> 6) : 0;
    const int tid = TEAM == kWave ? lane_id() : (int)threadIdx.x;
    // TEAM == 64: the rows in order, a row of another route is skipped (wave-uniform).  TEAM == 256: the rows named in `rows`.
    uint32_t row;
    if constexpr (TEAM == kWave) {
        const uint64_t r = global_wave_id();
        if (r >= n_rows || cand[r] > kWaveCap) return;
        row = (uint32_t)r;
    } else {
        row = rows[blockIdx.x];
    }
    uint32_t* keys = s_keys[team];
    uint32_t* cnt = s_cnt[team];
    unsigned char* cnt8 = reinterpret_cast<unsigned char*>(cnt);
    RowLists* L = &s_lists[team];
    if (tid < kWave) row_lists_load(a, row, tid, L);
    team_sync<TEAM>();
    const uint32_t c = (uint32_t)L->off[L->lists];          // <= the route's capacity: k_snn_cand sorted the rows by it
    uint32_t slots = 64;
    while (slots < 2 * c) slots <<= 1;                      // <= SLOTS, which is twice the capacity
    const uint32_t mask = slots - 1;
    const int shift = 32 - (31 - __builtin_clz(slots));
    for (uint32_t s = tid; s < slots; s += TEAM) keys[s] = kEmpty;
    for (uint32_t s = tid; s < slots / 4; s += TEAM) cnt[s] = 0u;
    team_sync<TEAM>();
    for (uint32_t t = tid; t < c; t += TEAM) {
        const uint32_t j = row_candidate(a, L, t);
        if (j != row) tab_add(keys, cnt, mask, shift, j);
    }
    team_sync<TEAM>();
    if (a.pairs_knn) {
        for (int q = tid; q < a.k; q += TEAM) tab_mark(keys, cnt, mask, shift, L->mem[q]);
        const uint32_t* own = in_list_src(a.tsrc, a.lsrc, L->lo[a.k], (int64_t)L->own);
        for (unsigned long long p = tid; p < L->own; p += TEAM) tab_mark(keys, cnt, mask, shift, own[p]);
        team_sync<TEAM>();
    }
    // the slots in chunks of TEAM: who is considered, who is kept; the fill pass moves the kept to the front of the table
    unsigned long long n_cons = 0, n_kept = 0, s_max = 0;
    uint32_t run = 0;
    for (uint32_t base = 0; base < slots; base += TEAM) {
        const uint32_t slot = base + tid;                   // slots is a multiple of 64, and of 256 when it exceeds 256
        const bool in = slot < slots;
        const uint32_t key = in ? keys[slot] : kEmpty;
        const uint32_t byte = in ? cnt8[slot] : 0u;
        const uint32_t s = byte & 0x7Fu;
        const bool cons = key != kEmpty && (!a.pairs_knn || (byte & 0x80u));
        const bool kept = cons && s >= a.min_shared;
        if (cons) {
            n_cons++;
            s_max = s > s_max ? s : s_max;
        }
        n_kept += kept;
        if constexpr (FILL) {
            uint32_t before, total;
            if constexpr (TEAM == kWave) {
                const unsigned long long m = __builtin_amdgcn_ballot_w64(kept);
                before = (uint32_t)__builtin_popcountll(m & below64(tid));
                total = (uint32_t)__builtin_popcountll(m);
                wave_lds_sync();
            } else {
                before = block_scan_exclusive<4, uint32_t>(kept ? 1u : 0u, s_scan, total);     // its barrier: every slot of the chunk is read
            }
            if (kept) {                                     // run + before <= slot: only slots already read are overwritten
                keys[run + before] = key;
                cnt8[run + before] = (unsigned char)s;
            }
            run += total;
            team_sync<TEAM>();
        }
    }
    if constexpr (FILL) {
        const uint64_t out = cptr[row];
        for (uint32_t t = tid; t < run; t += TEAM) {
            const uint32_t key = keys[t];
            uint32_t r = 0;
            for (uint32_t u = 0; u < run; ++u) r += keys[u] < key;         // the kept keys are distinct: the ranks are a permutation
            cind[out + r] = key;
            cdat[out + r] = snn_value(a, cnt8[t]);
        }
    } else {
        if constexpr (TEAM == kWave) {
            n_cons = wave_sum(n_cons);
            n_kept = wave_sum(n_kept);
            s_max = wave_max(s_max);
        } else {
            n_cons = block_sum<4>(n_cons, s_red);
            n_kept = block_sum<4>(n_kept, s_red);
            s_max = block_max<4>(s_max, s_red);
        }
        if (tid == 0) row_report(row, n_kept, n_cons, s_max, len_out, small);
    }
}

// ---- the long route: a workgroup per row, one u8 counter per index of a window ----------------------------------------------
// Thread t reads back the 256 consecutive indices from 256 t.  Their counters lie in the words t, 256 + t, 512 + t, ... (four
// indices to a word), so that the threads of a wave read consecutive words, not words 64 apart.
__device__ __forceinline__ uint32_t win_word(uint32_t d) { return (((d & 255u) >> 2) << 8) + (d >> 8); }
__device__ __forceinline__ uint32_t win_shift(uint32_t d) { return (d & 3u) * 8; }
template <bool FILL>
__global__ void __launch_bounds__(256) k_snn_window(SnnArgs a, const uint32_t* __restrict__ rows, int64_t* __restrict__ len_out,
                                                    const uint64_t* __restrict__ cptr, uint32_t* __restrict__ cind,
                                                    double* __restrict__ cdat, unsigned long long* __restrict__ small) {
    static_assert(kWin == 256 * 256, "win_word assumes 256 indices per thread");
    __shared__ uint32_t s_cnt[kWin / 4];
    __shared__ RowLists s_lists;
    __shared__ unsigned long long s_wstart[kSnnLists];     // per list: where its part of the window starts,
    __shared__ uint32_t s_wcnt[kSnnLists], s_woff[kSnnLists + 1];   // how long it is, and the parts' offsets
    __shared__ unsigned long long s_red[4];
    __shared__ uint32_t s_scan[4];
    const int tid = threadIdx.x;
    const uint32_t row = rows[blockIdx.x];
    RowLists* L = &s_lists;
    if (tid < kWave) row_lists_load(a, row, tid, L);
    __syncthreads();
    const uint32_t* own = in_list_src(a.tsrc, a.lsrc, L->lo[a.k], (int64_t)L->own);
    // thread q < K owns list q: the list itself and how far the windows before this one have taken it
    const int lists = L->lists;
    const uint32_t* my_list = nullptr;
    unsigned long long my_len = 0, my_cur = 0;
    if (tid < lists) {
        my_len = L->off[tid + 1] - L->off[tid] - (unsigned long long)a.self;
        my_list = in_list_src(a.tsrc, a.lsrc, L->lo[tid], (int64_t)my_len);
    }
    unsigned long long n_cons = 0, n_kept = 0, s_max = 0;
    uint64_t done = 0;
    for (uint64_t base = 0; base < a.n; base += kWin) {
        for (uint32_t w = tid; w < kWin / 4; w += 256) s_cnt[w] = 0u;
        // the lists ascend: what a list holds of this window starts where the last window ended
        if (tid < lists) {
            unsigned long long lo = my_cur, hi = my_len;
            while (lo < hi) {
                const unsigned long long mid = (lo + hi) >> 1;
                if ((uint64_t)my_list[mid] < base + kWin) lo = mid + 1;
                else hi = mid;
            }
            s_wstart[tid] = my_cur;
            s_wcnt[tid] = (uint32_t)(lo - my_cur);             // fewer than kWin: the entries of a list are distinct
            my_cur = lo;
        }
        __syncthreads();
        if (tid < kWave) {                                     // offsets of the lists' parts in the window's flat range
            const uint32_t inc = wave_scan_inclusive(tid < lists ? s_wcnt[tid] : 0u);
            s_woff[tid + 1] = inc;
            if (tid == 0) s_woff[0] = 0;
            const uint32_t tot = __shfl(inc, kWave - 1, kWave);
            if (tid == 0) s_woff[kSnnLists] = tot + (lists > kWave ? s_wcnt[kWave] : 0u);
        }
        if (a.self && tid < lists) {                           // m itself is a member of M(m)
            const uint32_t j = L->mem[tid];
            const uint64_t d = (uint64_t)j - base;             // below base: wraps to a huge number
            if (d < kWin && j != row) atomicAdd(&s_cnt[win_word((uint32_t)d)], 1u << win_shift((uint32_t)d));
        }
        __syncthreads();
        const uint32_t in_win = s_woff[lists];
        for (uint32_t t = tid; t < in_win; t += 256) {
            int lo = 0, hi = lists;                            // the list q with woff[q] <= t < woff[q + 1]
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_woff[mid] <= t) lo = mid;
                else hi = mid;
            }
            const int64_t len = (int64_t)(L->off[lo + 1] - L->off[lo]) - a.self;
            const uint32_t j = in_list_src(a.tsrc, a.lsrc, L->lo[lo], len)[s_wstart[lo] + (t - s_woff[lo])];
            const uint32_t d = (uint32_t)((uint64_t)j - base);     // inside the window by the search above
            if (j != row) atomicAdd(&s_cnt[win_word(d)], 1u << win_shift(d));
        }
        if (a.pairs_knn) {
            for (int q = tid; q < a.k; q += 256) {
                const uint64_t d = (uint64_t)L->mem[q] - base;
                if (d < kWin) atomicOr(&s_cnt[win_word((uint32_t)d)], 0x80u << win_shift((uint32_t)d));
            }
            for (unsigned long long p = tid; p < L->own; p += 256) {
                const uint64_t d = (uint64_t)own[p] - base;
                if (d < kWin) atomicOr(&s_cnt[win_word((uint32_t)d)], 0x80u << win_shift((uint32_t)d));
            }
        }
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t w = 0; w < 64; ++w) {
            const uint32_t word = s_cnt[w * 256 + tid];
            for (int b = 0; b < 4 && word; ++b) {
                const uint32_t byte = (word >> (8 * b)) & 0xFFu, s = byte & 0x7Fu;
                if (s > 0 && (!a.pairs_knn || (byte & 0x80u))) {
                    n_cons++;
                    s_max = s > s_max ? s : s_max;
                    mine += s >= a.min_shared;
                }
            }
        }
        n_kept += mine;
        if constexpr (FILL) {
            uint32_t total;
            uint64_t pos = cptr[row] + done + block_scan_exclusive<4, uint32_t>(mine, s_scan, total);
            for (uint32_t w = 0; w < 64 && mine; ++w) {
                const uint32_t word = s_cnt[w * 256 + tid];
                for (int b = 0; b < 4 && word; ++b) {
                    const uint32_t byte = (word >> (8 * b)) & 0xFFu, s = byte & 0x7Fu;
                    if (s >= a.min_shared && s > 0 && (!a.pairs_knn || (byte & 0x80u))) {
                        cind[pos] = (uint32_t)(base + (uint64_t)tid * 256 + w * 4 + b);
                        cdat[pos] = snn_value(a, s);
                        pos++;
                    }
                }
            }
            done += total;
        }
        __syncthreads();
    }
    if constexpr (!FILL) {
        n_cons = block_sum<4>(n_cons, s_red);
        n_kept = block_sum<4>(n_kept, s_red);
        s_max = block_max<4>(s_max, s_red);
        if (tid == 0) row_report(row, n_kept, n_cons, s_max, len_out, small);
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------

static const srx_snn_opts kSnnDefaults = {SRX_SNN_JACCARD, SRX_SNN_PAIRS_SHARED, 1, 0, 1.0 / 15.0};

static uint32_t min_shared_of(uint32_t K, double prune) {
    for (uint32_t s = 1; s <= K; ++s)
        if ((double)s / (double)(2 * K - s) >= prune) return s;
    return K + 1;
}

static int32_t snn_opts_check(srx_ctx* ctx, const srx_snn_opts* o) {
    if (!(o->prune >= 0.0 && o->prune <= 1.0)) return fail(ctx, SRX_E_ARG, "snn: prune = %g is not in [0, 1]", o->prune);
    if (o->weight != SRX_SNN_JACCARD && o->weight != SRX_SNN_NUMBER)
        return fail(ctx, SRX_E_ARG, "snn: weight = %d is neither jaccard nor number", o->weight);
    if (o->pairs != SRX_SNN_PAIRS_SHARED && o->pairs != SRX_SNN_PAIRS_KNN)
        return fail(ctx, SRX_E_ARG, "snn: pairs = %d is neither shared nor knn", o->pairs);
    return SRX_OK;
}

static void snn_info_start(srx_snn_info* info, uint64_t n, uint32_t k, const srx_snn_opts* o) {
    memset(info, 0, sizeof *info);
    info->n = n;
    info->k = k;
    info->set_size = k + (o->include_self ? 1u : 0u);
    info->min_shared = min_shared_of(info->set_size, o->prune);
    info->wave_capacity = kWaveCap;
    info->short_capacity = kBlockCap;
}

static int32_t snn_empty(srx_ctx* ctx, uint32_t k, srx_graph** out) {
    srx_graph* g = nullptr;
    SRX_TRY(graph_alloc(ctx, 0, k, &g));
    int32_t rc = graph_alloc_c(g, 0);
    if (rc == SRX_OK && (hipMemsetAsync(g->d_dptr, 0, 8, ctx->stream) != hipSuccess ||
                         hipMemsetAsync(g->d_cptr, 0, 8, ctx->stream) != hipSuccess))
        rc = fail(ctx, SRX_E_HIP, "snn: hipMemsetAsync failed");
    if (rc != SRX_OK) {
        srx_graph_free(g);
        return rc;
    }
    *out = g;
    return SRX_OK;
}

// d_idx / d_dist (may be null): the list on the device, n x k row-major.  n >= 1, 1 <= k <= 64, k <= n - 1, n < 2^32 - 1.
static int32_t snn_fill(srx_ctx* ctx, srx_graph* g, const uint32_t* d_idx, const double* d_dist, const srx_snn_opts* o,
                        srx_snn_info* info) {
    const uint64_t n = g->n;
    const uint32_t k = g->k;
    const size_t nk = (size_t)n * k;
    hipStream_t st = ctx->stream;
    unsigned long long* d_small;
    int64_t *d_indeg, *d_len, *d_cptr_tmp;
    uint64_t* d_cand;
    uint32_t *d_mid, *d_long, *d_rev_long;
    unsigned char* d_flags;
    SRX_TRY(scratch(ctx, "snn_small", kSmWords * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "snn_indeg", 2 * n * 8, (void**)&d_indeg));         // in-degrees | the scatter's cursors
    SRX_TRY(scratch(ctx, "snn_len", n * 8, (void**)&d_len));
    SRX_TRY(scratch(ctx, "snn_cptr", (n + 1) * 8, (void**)&d_cptr_tmp));
    SRX_TRY(scratch(ctx, "snn_cand", n * 8, (void**)&d_cand));
    SRX_TRY(scratch(ctx, "snn_mid", n * 4, (void**)&d_mid));
    SRX_TRY(scratch(ctx, "snn_long", n * 4, (void**)&d_long));
    SRX_TRY(scratch(ctx, "snn_rev_long", (nk / kInShort + 1) * 4, (void**)&d_rev_long));
    SRX_TRY(scratch(ctx, "snn_flags", nk, (void**)&d_flags));
    int* d_flag = reinterpret_cast<int*>(d_small + kSmFlag);
    const unsigned wg_rows = (unsigned)((n + 3) / 4), wg_thr = (unsigned)((n + 255) / 256);
    const int self = o->include_self ? 1 : 0;

    StreamTimer t_all(ctx, st), t_lists(ctx, st), t_count(ctx, st), t_fill(ctx, st);
    SRX_TRY(t_all.start());
    SRX_TRY(t_lists.start());
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, kSmWords * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(d_indeg, 0, 2 * n * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(g->d_a, 0, nk * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(g->d_rho, 0, n * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(g->d_sigma, 0, n * 8, st));
    hipLaunchKernelGGL(k_snn_rows, dim3(wg_rows), dim3(256), 0, st, d_idx, d_dist, n, (int)k, g->d_dptr, g->d_dind, g->d_ddat, d_indeg,
                       d_flag);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(list_flag_check(ctx, "snn", n, d_flag));
    // the reverse lists of ALL edges: every edge carries the in-list flag; the value array that rides along is D's data
    hipLaunchKernelGGL(k_snn_cand, dim3(wg_thr), dim3(256), 0, st, g->d_dind, d_indeg, n, (int)k, self, d_cand, d_mid, d_long, d_rev_long,
                       d_small);
    SRX_HIP(ctx, hipGetLastError());
    SRX_HIP(ctx, hipMemsetAsync(d_flags, 2, nk, st));
    InLists in;
    SRX_TRY(in_lists_build(ctx, g->d_dind, g->d_ddat, d_flags, n, k, d_indeg, &in));
    uint64_t sm[kSmWords];
    SRX_TRY(d2h(ctx, sm, d_small, kSmWords * 8));
    SRX_TRY(in_lists_order_long(ctx, n, k, d_rev_long, sm[kSmRevLong], &in));
    SRX_TRY(t_lists.stop(&info->ms_lists));
    const uint64_t n_mid = sm[kSmMid], n_long = sm[kSmLong];
    info->max_in_degree = sm[kSmMaxIndeg];
    info->max_candidates = sm[kSmMaxCand];
    info->sum_candidates = sm[kSmSumCand];
    info->rows_wave = sm[kSmWave];
    info->rows_long = n_long;

    SnnArgs a{g->d_dind, in.tptr, in.tsrc, in.lsrc, n, (int)k, self, o->pairs == SRX_SNN_PAIRS_KNN, o->weight == SRX_SNN_NUMBER,
              info->min_shared, (double)(2 * info->set_size)};
    auto pass = [&](bool fill) -> int32_t {
        uint64_t* cptr = g->d_cptr;
        uint32_t* cind = g->d_cind;
        double* cdat = g->d_cdat;
        if (fill) {
            hipLaunchKernelGGL((k_snn_hash<kWave, kWaveSlots, true>), dim3(wg_rows), dim3(256), 0, st, a, d_cand, nullptr, n, d_len, cptr, cind,
                               cdat, d_small);
            if (n_mid)
                hipLaunchKernelGGL((k_snn_hash<256, kBlockSlots, true>), dim3((unsigned)n_mid), dim3(256), 0, st, a, d_cand, d_mid, n_mid, d_len,
                                   cptr, cind, cdat, d_small);
            if (n_long)
                hipLaunchKernelGGL(k_snn_window<true>, dim3((unsigned)n_long), dim3(256), 0, st, a, d_long, d_len, cptr, cind, cdat, d_small);
        } else {
            hipLaunchKernelGGL((k_snn_hash<kWave, kWaveSlots, false>), dim3(wg_rows), dim3(256), 0, st, a, d_cand, nullptr, n, d_len, nullptr,
                               nullptr, nullptr, d_small);
            if (n_mid)
                hipLaunchKernelGGL((k_snn_hash<256, kBlockSlots, false>), dim3((unsigned)n_mid), dim3(256), 0, st, a, d_cand, d_mid, n_mid,
                                   d_len, nullptr, nullptr, nullptr, d_small);
            if (n_long)
                hipLaunchKernelGGL(k_snn_window<false>, dim3((unsigned)n_long), dim3(256), 0, st, a, d_long, d_len, nullptr, nullptr, nullptr,
                                   d_small);
        }
        SRX_HIP(ctx, hipGetLastError());
        return SRX_OK;
    };
    SRX_TRY(t_count.start());
    SRX_TRY(pass(false));
    SRX_TRY(scan_exclusive(ctx, d_len, n, d_cptr_tmp, nullptr));
    int64_t nnz = 0;
    SRX_TRY(d2h(ctx, &nnz, d_cptr_tmp + n, 8));
    SRX_TRY(t_count.stop(&info->ms_count));
    SRX_TRY(graph_alloc_c(g, (uint64_t)nnz));
    SRX_TRY(t_fill.start());
    SRX_HIP(ctx, hipMemcpyAsync(g->d_cptr, d_cptr_tmp, (n + 1) * 8, hipMemcpyDeviceToDevice, st));
    SRX_TRY(pass(true));
    SRX_TRY(d2h(ctx, sm, d_small, kSmWords * 8));
    SRX_TRY(t_fill.stop(&info->ms_fill));
    SRX_TRY(t_all.stop(&info->ms));
    uint64_t cons = 0, empty = 0;
    for (int s = 0; s < kSnnSlots; ++s) {
        cons += sm[s * 2];
        empty += sm[s * 2 + 1];
    }
    info->pairs_considered = cons / 2;
    info->rows_empty = empty;
    info->max_shared = (uint32_t)sm[kSmMaxShared];
    info->max_row_nnz = sm[kSmMaxRow];
    info->nnz = (uint64_t)nnz;
    info->pairs_kept = (uint64_t)nnz / 2;
    g->info.nnz_distances = nk;
    g->info.nnz_connectivities = (uint64_t)nnz;
    g->info.max_row_nnz = sm[kSmMaxRow];
    return SRX_OK;
}

static int32_t snn_build(srx_ctx* ctx, const uint32_t* d_idx, const double* d_dist, uint64_t n, uint32_t k, const srx_snn_opts* o,
                         srx_snn_info* info_out, srx_graph** out) {
    Range rg("snn");
    srx_snn_info info;
    snn_info_start(&info, n, k, o);
    srx_graph* g = nullptr;
    if (n == 0) SRX_TRY(snn_empty(ctx, k, &g));
    else {
        SRX_TRY(graph_alloc(ctx, n, k, &g));
        const int32_t rc = snn_fill(ctx, g, d_idx, d_dist, o, &info);
        if (rc != SRX_OK) {
            srx_graph_free(g);
            return rc;
        }
    }
    if (info_out) *info_out = info;
    *out = g;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_snn_min_shared(uint32_t k, int32_t include_self, double prune, uint32_t* out) {
    if (!out) return fail(nullptr, SRX_E_ARG, "snn_min_shared: null output");
    if (k < 1 || k > (uint32_t)kSnnMaxK) return fail(nullptr, SRX_E_ARG, "snn_min_shared: k = %u outside 1..%d", k, kSnnMaxK);
    if (!(prune >= 0.0 && prune <= 1.0)) return fail(nullptr, SRX_E_ARG, "snn_min_shared: prune = %g is not in [0, 1]", prune);
    *out = min_shared_of(k + (include_self ? 1u : 0u), prune);
    return SRX_OK;
}

int32_t srx_snn_from_knn(srx_ctx* ctx, const uint32_t* indices, const double* distances, uint64_t n, uint32_t k,
                         const srx_snn_opts* opts, srx_snn_info* info, srx_graph** out) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (!out) return fail(ctx, SRX_E_ARG, "snn: null output handle");
    *out = nullptr;
    const srx_snn_opts* o = opts ? opts : &kSnnDefaults;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "snn: rows are sharded; the graph needs all cells");
    if (k < 1 || k > (uint32_t)kSnnMaxK) return fail(ctx, SRX_E_ARG, "snn: k = %u outside 1..%d", k, kSnnMaxK);
    SRX_TRY(snn_opts_check(ctx, o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return snn_build(ctx, nullptr, nullptr, 0, k, o, info, out);
    if (!indices) return fail(ctx, SRX_E_ARG, "snn: null k-NN list");
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "snn: more than 2^32 - 2 cells");
    if ((uint64_t)k > n - 1) return fail(ctx, SRX_E_ARG, "snn: k = %u but a cell has only %llu others", k, (unsigned long long)(n - 1));
    uint32_t* d_idx;
    double* d_dist = nullptr;
    SRX_TRY(scratch(ctx, "snn_in_idx", n * k * 4, (void**)&d_idx));
    SRX_TRY(h2d(ctx, d_idx, indices, n * k * 4));
    if (distances) {
        SRX_TRY(scratch(ctx, "snn_in_dist", n * k * 8, (void**)&d_dist));
        SRX_TRY(h2d(ctx, d_dist, distances, n * k * 8));
    }
    return snn_build(ctx, d_idx, d_dist, n, k, o, info, out);
}

int32_t srx_snn_graph(srx_graph* g, const srx_snn_opts* opts, srx_snn_info* info, srx_graph** out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "snn: null graph");
    srx_ctx* ctx = g->ctx;
    if (!out) return fail(ctx, SRX_E_ARG, "snn: null output handle");
    *out = nullptr;
    const srx_snn_opts* o = opts ? opts : &kSnnDefaults;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "snn: rows are sharded; the graph needs all cells");
    SRX_TRY(snn_opts_check(ctx, o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    // the handle's D is a checked list in column order: the row kernel finds it as it is and copies it
    return snn_build(ctx, g->d_dind, g->d_ddat, g->n, g->k, o, info, out);
}

}  // extern "C"
