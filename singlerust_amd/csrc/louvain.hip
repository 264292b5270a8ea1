// louvain.hip — Louvain communities of a symmetric weighted graph on the device: srx_louvain (the connectivities of an
// srx_graph, read where they lie), srx_louvain_csr (any symmetric CSR) and srx_graph_labels_fetch.
//
// Definition (include/srx.h has it in full).  k_i = self_i + sum_j W_ij, 2m = sum_i k_i,
//     Q = sum_c [ in_c / 2m - gamma (tot_c / 2m)^2 ]
// A level starts from singletons and runs synchronous sweeps t = 0, 1, ...: in sweep t the vertices with (i + t) even
// evaluate, against the labelling and the tot_c of BEFORE the sweep,
//     g(c) = w_{i->c} - gamma k_i (tot_c - [c = c_i] k_i) / 2m
// for their own community and every community among their neighbours, and move to the best one only if it beats the own
// strictly (ties between targets: lowest id; a vertex alone in its community never joins a singleton with a lower id).
// Communities then become the vertices of the next level's graph.
//
// Determinism.  Everything that is summed by atomics is summed as 64-bit FIXED POINT: x -> rint(x * 2^S) with
// S = 60 - ceil(log2(2m)), so that 2m itself, the largest sum there is, stays below 2^61; integer addition does not depend
// on its order.  That holds tot_c (updated by the moved vertices only, +q(k_i) / -q(k_i): exact), the two sums of Q and
// the merged weights of a coarse graph.  The weights a long row sends to each community stay inside the row, at most
// max k_i: they are summed at the finer scale 2^(60 - ceil(log2(max k_i))) of the level.  Sums inside a short row are f64
// in a fixed order.  S is derived on the device from order-free quantities (max k_i by integer atomicMax, then 2m at a
// first, coarser scale), and every level's 2m is read back and checked against the range.
//
// Kernels:
//   (srx_louvain_csr: k_symcsr_check of symcsr.hip validates the input)
//   k_louvain_degree    thread per row: k_i in row order, singleton start, max k_i
//   k_louvain_scale     one thread: S from max k_i * n, then from 2m; 2m of the level
//   k_louvain_quant     q(k_i), tot of the singletons, their sum
//   k_louvain_classify / k_louvain_biglist   rows longer than a wave: their list and the offsets of their hash tables
//   k_louvain_move<G>   a row of at most G = 32 or 64 entries per G lanes: equal communities are combined by an all-pairs
//                       walk over the lanes (fixed order), gain in f64, arg max by butterfly
//   k_louvain_move_big  a workgroup per longer row, any length: an open-addressing table of 2^ceil(log2(2 L)) slots in a
//                       global workspace (a row of L entries meets at most L communities), fixed-point sums
//   k_louvain_apply     the moved vertices update tot and the community sizes; counts the moves
//   k_louvain_q_in / k_louvain_q_tot   the two sums of Q and the number of communities
//   k_louvain_flag / k_louvain_oldof / k_louvain_members   compact ids (flag + scan.hip's scan_exclusive) and the member list
//                       of each community
//   k_louvain_coarse<FILL>  a workgroup per coarse vertex walks its members' rows: a bitmap of kLvBits coarse ids at a time
//                       with prefix popcounts (scan.hpp's bitmap ranks) gives the row length, then every column its place,
//                       and the weights are added there in fixed point; self weight apart
//   k_louvain_unfix     fixed point -> f64 for the coarse weights
//   k_louvain_compose   cell -> community through a kept level
//   k_louvain_sizes / k_louvain_keys / k_louvain_bitonic / k_louvain_rank / k_louvain_relabel   final labels: communities
//                       ordered by (size descending, smallest member)
#include "common.hpp"
#include "graph_handle.hpp"
#include "scan.hpp"
#include "symcsr.hpp"

#include <cmath>

namespace srx {

constexpr int kLvBits = 1 << 17;         // coarse ids per pass of the aggregation (16 KiB bitmap + 16 KiB prefix)
constexpr int kLvSlots = 64;             // accumulators are spread over slots and summed in integers
constexpr uint32_t kLvEmpty = 0xFFFFFFFFu;
// the small block (8-byte words)
enum { LV_KMAX = 0, LV_MOVES, LV_NCOMM, LV_FLAG, LV_SHIFT, LV_SCALE, LV_INV, LV_TWOM, LV_WSCALE, LV_WINV, LV_ACC, LV_IN = LV_ACC + kLvSlots,
       LV_SQ = LV_IN + kLvSlots, LV_WORDS = LV_SQ + kLvSlots };

struct LvGraph : SymCsr {                // one level's graph; self == nullptr: no self weights (the input)
    const double* self;
};

__device__ __forceinline__ long long lv_fix(double x, double scale) { return __double2ll_rn(x * scale); }
__device__ __forceinline__ void lv_slot_add(unsigned long long* slots, long long v) {
    v = wave_sum(v);
    if (lane_id() == 0 && v) atomicAdd(&slots[(blockIdx.x * 4 + (threadIdx.x >> 6)) & (kLvSlots - 1)], (unsigned long long)v);
}

__global__ void __launch_bounds__(256) k_louvain_degree(LvGraph g, double* __restrict__ kdeg, uint32_t* __restrict__ comm,
                                                        uint32_t* __restrict__ size, unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    double s = 0.0;
    if (i < g.n) {
        if (g.self) s = g.self[i];
        for (uint64_t e = g.ptr[i]; e < g.ptr[i + 1]; ++e) s += g.w[e];
        kdeg[i] = s;
        comm[i] = (uint32_t)i;
        size[i] = 1u;
    }
    // non-negative doubles order as their bit patterns do
    const unsigned long long b = wave_max((unsigned long long)__double_as_longlong(s));
    if (lane_id() == 0 && b) atomicMax(&small[LV_KMAX], b);
}

// stage 0: a first scale from the bound n * max k_i >= 2m; stage 1: the scale of the run from 2m at the first scale;
// stage 2: 2m of this level at the scale of the run.  Each stage clears the slots it has read.
__global__ void k_louvain_scale(unsigned long long* __restrict__ small, uint64_t n, int stage) {
    if (threadIdx.x || blockIdx.x) return;
    double* sd = reinterpret_cast<double*>(small);
    long long total = 0;
    for (int s = 0; s < kLvSlots; ++s) {
        total += (long long)small[LV_ACC + s];
        small[LV_ACC + s] = 0ull;
    }
    if (stage == 2) {
        sd[LV_TWOM] = (double)total * sd[LV_INV];
        // the finer scale of sums that stay inside one row (at most max k_i < 2^e): 2^(60 - e)
        const double kmax = __longlong_as_double((long long)small[LV_KMAX]);
        int ek = 0;
        if (is_pos_finite(kmax)) (void)frexp(kmax, &ek);
        const int ws = 60 - ek > 1000 ? 1000 : 60 - ek < -1000 ? -1000 : 60 - ek;
        sd[LV_WSCALE] = ldexp(1.0, ws);
        sd[LV_WINV] = ldexp(1.0, -ws);
        return;
    }
    const double bound = stage == 0 ? __longlong_as_double((long long)small[LV_KMAX]) * (double)n : (double)total * sd[LV_INV];
    int e = 0;
    if (is_pos_finite(bound)) (void)frexp(bound, &e);        // bound < 2^e
    int shift = 60 - e;
    shift = shift > 1000 ? 1000 : shift < -1000 ? -1000 : shift;
    small[LV_SHIFT] = (unsigned long long)(long long)shift;
    sd[LV_SCALE] = ldexp(1.0, shift);
    sd[LV_INV] = ldexp(1.0, -shift);
    sd[LV_TWOM] = bound;
}

__global__ void __launch_bounds__(256) k_louvain_quant(const double* __restrict__ kdeg, uint64_t n, long long* __restrict__ kq,
                                                       unsigned long long* __restrict__ tot, unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const double scale = reinterpret_cast<const double*>(small)[LV_SCALE];
    long long q = 0;
    if (i < n) {
        q = lv_fix(kdeg[i], scale);
        if (kq) {
            kq[i] = q;
            tot[i] = (unsigned long long)q;
        }
    }
    lv_slot_add(small + LV_ACC, q);
}

__device__ __forceinline__ int64_t lv_hash_cap(uint64_t len) {      // a power of two >= 2 len
    int64_t c = 128;
    while ((uint64_t)c < 2 * len) c <<= 1;
    return c;
}

__global__ void __launch_bounds__(256) k_louvain_classify(const uint64_t* __restrict__ ptr, uint64_t n, int64_t* __restrict__ isbig,
                                                          int64_t* __restrict__ cap) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t len = ptr[i + 1] - ptr[i];
    isbig[i] = len > (uint64_t)kWave;
    cap[i] = len > (uint64_t)kWave ? lv_hash_cap(len) : 0;
}

__global__ void __launch_bounds__(256) k_louvain_biglist(const int64_t* __restrict__ isbig, const int64_t* __restrict__ bpos, uint64_t n,
                                                         uint32_t* __restrict__ big) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && isbig[i]) big[bpos[i]] = (uint32_t)i;
}

// g(c) of a vertex with degree ki: t = tot_c (less the vertex itself for its own community), as f64
__device__ __forceinline__ double lv_gain(double w_to, double gamma, double ki, double t, double twom) {
    return w_to - gamma * ki * t / twom;
}

// Rows of lo_len < L <= G entries, one per G lanes.  Every vertex of that class gets its entry of `next`.
template <int G>
__global__ void __launch_bounds__(256) k_louvain_move(LvGraph g, int lo_len, const double* __restrict__ kdeg, const long long* __restrict__ kq,
                                                      const uint32_t* __restrict__ comm, const unsigned long long* __restrict__ tot,
                                                      const uint32_t* __restrict__ size, uint32_t* __restrict__ next,
                                                      const unsigned long long* __restrict__ small, double gamma, int parity) {
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    if (row >= g.n) return;
    const uint64_t lo = g.ptr[row];
    const uint64_t len = g.ptr[row + 1] - lo;
    if (len > (uint64_t)G || (len <= (uint64_t)lo_len && !(lo_len == 0 && len == 0))) return;
    const uint32_t own = comm[row];
    if (len == 0 || ((row + (uint64_t)parity) & 1)) {
        if (sub == 0) next[row] = own;
        return;
    }
    const int L = (int)len;
    const bool act = sub < L;
    const uint32_t c = act ? comm[g.ind[lo + sub]] : kLvEmpty;
    const double ww = act ? g.w[lo + sub] : 0.0;
    double w_to = 0.0, w_own = 0.0;
    for (int m = 0; m < L; ++m) {
        const uint32_t oc = __shfl(c, m, G);
        const double ow = __shfl(ww, m, G);
        if (oc == c) w_to += ow;
        if (oc == own) w_own += ow;
    }
    const double* sd = reinterpret_cast<const double*>(small);
    const double inv = sd[LV_INV], twom = sd[LV_TWOM], ki = kdeg[row];
    const double g_own = lv_gain(w_own, gamma, ki, (double)((long long)tot[own] - kq[row]) * inv, twom);
    double best = -(double)__builtin_inff();
    uint32_t bc = kLvEmpty;
    if (act && c != own && !(size[own] == 1u && size[c] == 1u && c < own)) {
        best = lv_gain(w_to, gamma, ki, (double)(long long)tot[c] * inv, twom);
        bc = c;
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const double og = __shfl_xor(best, off, G);
        const uint32_t oc = __shfl_xor(bc, off, G);
        if (og > best || (og == best && oc < bc)) {
            best = og;
            bc = oc;
        }
    }
    if (sub == 0) next[row] = (bc != kLvEmpty && best > g_own) ? bc : own;
}

__device__ __forceinline__ uint64_t lv_hash(uint32_t c) { return ((uint64_t)c * 0x9E3779B97F4A7C15ull) >> 29; }

// One workgroup per row longer than a wave.  hoff[row] .. hoff[row + 1] is the row's table in the workspace.
__global__ void __launch_bounds__(256) k_louvain_move_big(LvGraph g, const uint32_t* __restrict__ big, const int64_t* __restrict__ hoff,
                                                          uint32_t* __restrict__ hkey, unsigned long long* __restrict__ hval,
                                                          const double* __restrict__ kdeg, const long long* __restrict__ kq,
                                                          const uint32_t* __restrict__ comm, const unsigned long long* __restrict__ tot,
                                                          const uint32_t* __restrict__ size, uint32_t* __restrict__ next,
                                                          const unsigned long long* __restrict__ small, double gamma, int parity) {
    __shared__ double s_g[4];
    __shared__ uint32_t s_c[4];
    __shared__ unsigned long long s_own;
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint32_t row = big[blockIdx.x];
    const uint32_t own = comm[row];
    if ((row + (uint32_t)parity) & 1u) {
        if (tid == 0) next[row] = own;
        return;
    }
    const uint64_t lo = g.ptr[row], len = g.ptr[row + 1] - lo;
    const uint64_t h0 = (uint64_t)hoff[row], cap = (uint64_t)hoff[row + 1] - h0, mask = cap - 1;
    uint32_t* keys = hkey + h0;
    unsigned long long* vals = hval + h0;
    const double* sd = reinterpret_cast<const double*>(small);
    const double wscale = sd[LV_WSCALE], winv = sd[LV_WINV], inv = sd[LV_INV], twom = sd[LV_TWOM];
    for (uint64_t t = tid; t < cap; t += 256) {
        keys[t] = kLvEmpty;
        vals[t] = 0ull;
    }
    if (tid == 0) s_own = 0ull;
    __threadfence();
    __syncthreads();
    for (uint64_t e = tid; e < len; e += 256) {
        const uint32_t c = comm[g.ind[lo + e]];
        const long long q = lv_fix(g.w[lo + e], wscale);
        uint64_t h = lv_hash(c) & mask;
        for (uint64_t probe = 0; probe < cap; ++probe) {           // at most len <= cap / 2 keys: a free slot is always met
            const uint32_t prev = atomicCAS(&keys[h], kLvEmpty, c);
            if (prev == kLvEmpty || prev == c) {
                atomicAdd(&vals[h], (unsigned long long)q);
                break;
            }
            h = (h + 1) & mask;
        }
    }
    __threadfence();
    __syncthreads();
    const double ki = kdeg[row];
    const uint32_t own_size = size[own];
    double best = -(double)__builtin_inff();
    uint32_t bc = kLvEmpty;
    for (uint64_t t = tid; t < cap; t += 256) {
        const uint32_t c = __hip_atomic_load(&keys[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == kLvEmpty) continue;
        const unsigned long long v = __hip_atomic_load(&vals[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c == own) {
            s_own = v;
            continue;
        }
        if (own_size == 1u && size[c] == 1u && c < own) continue;
        const double gc = lv_gain((double)(long long)v * winv, gamma, ki, (double)(long long)tot[c] * inv, twom);
        if (gc > best || (gc == best && c < bc)) {
            best = gc;
            bc = c;
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const double og = __shfl_xor(best, off, kWave);
        const uint32_t oc = __shfl_xor(bc, off, kWave);
        if (og > best || (og == best && oc < bc)) {
            best = og;
            bc = oc;
        }
    }
    if (lane == 0) {
        s_g[wave] = best;
        s_c[wave] = bc;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w)
            if (s_g[w] > best || (s_g[w] == best && s_c[w] < bc)) {
                best = s_g[w];
                bc = s_c[w];
            }
        const double g_own = lv_gain((double)(long long)s_own * winv, gamma, ki, (double)((long long)tot[own] - kq[row]) * inv, twom);
        next[row] = (bc != kLvEmpty && best > g_own) ? bc : own;
    }
}

__global__ void __launch_bounds__(256) k_louvain_apply(const uint32_t* __restrict__ comm, const uint32_t* __restrict__ next, uint64_t n,
                                                       const long long* __restrict__ kq, unsigned long long* __restrict__ tot,
                                                       uint32_t* __restrict__ size, unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        const uint32_t a = comm[i], b = next[i];
        moved = a != b;
        if (moved) {
            const long long q = kq[i];
            atomicAdd(&tot[b], (unsigned long long)q);
            atomicAdd(&tot[a], (unsigned long long)(-q));
            atomicAdd(&size[b], 1u);
            atomicSub(&size[a], 1u);
        }
    }
    const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(moved));
    if (lane_id() == 0 && cnt) atomicAdd(&small[LV_MOVES], (unsigned long long)cnt);
}

__global__ void __launch_bounds__(256) k_louvain_q_in(LvGraph g, const uint32_t* __restrict__ comm, unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const double scale = reinterpret_cast<const double*>(small)[LV_SCALE];
    long long q = 0;
    if (i < g.n) {
        const uint32_t c = comm[i];
        double s = g.self ? g.self[i] : 0.0;
        for (uint64_t e = g.ptr[i]; e < g.ptr[i + 1]; ++e)
            if (comm[g.ind[e]] == c) s += g.w[e];
        q = lv_fix(s, scale);
    }
    lv_slot_add(small + LV_IN, q);
}

// (tot_c / 2m)^2 <= 1 summed at the scale 2^61; the number of communities
__global__ void __launch_bounds__(256) k_louvain_q_tot(const unsigned long long* __restrict__ tot, const uint32_t* __restrict__ size,
                                                       uint64_t n, unsigned long long* __restrict__ small) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const double* sd = reinterpret_cast<const double*>(small);
    long long q = 0;
    const bool live = c < n && size[c] > 0u;
    if (live) {
        const double t = (double)(long long)tot[c] * sd[LV_INV] / sd[LV_TWOM];
        q = lv_fix(t * t, 2305843009213693952.0);
    }
    lv_slot_add(small + LV_SQ, q);
    const int cnt = __builtin_popcountll(__builtin_amdgcn_ballot_w64(live));
    if (lane_id() == 0 && cnt) atomicAdd(&small[LV_NCOMM], (unsigned long long)cnt);
}

__global__ void __launch_bounds__(256) k_louvain_flag(const uint32_t* __restrict__ size, uint64_t n, int64_t* __restrict__ flag,
                                                      int64_t* __restrict__ cnt) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    flag[c] = size[c] > 0u;
    cnt[c] = size[c];
}

__global__ void __launch_bounds__(256) k_louvain_oldof(const int64_t* __restrict__ flag, const int64_t* __restrict__ newid, uint64_t n,
                                                       uint32_t* __restrict__ oldof) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < n && flag[c]) oldof[newid[c]] = (uint32_t)c;
}

// the members of every community, in arbitrary order within it: what reads them is order-free
__global__ void __launch_bounds__(256) k_louvain_members(const uint32_t* __restrict__ comm, uint64_t n, const int64_t* __restrict__ mptr,
                                                         uint32_t* __restrict__ cursor, uint32_t* __restrict__ members) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = comm[i];
    members[(uint64_t)mptr[c] + atomicAdd(&cursor[c], 1u)] = (uint32_t)i;
}

// One workgroup per coarse vertex a.  !FILL: len[a] = distinct coarse neighbours, selfq[a] += the weight inside a (fixed
// point).  FILL: the columns of row a in ascending order and their weights (fixed point, into cacc at cptr[a]).
template <bool FILL>
__global__ void __launch_bounds__(256) k_louvain_coarse(LvGraph g, const uint32_t* __restrict__ comm, const int64_t* __restrict__ newid,
                                                        const uint32_t* __restrict__ oldof, const int64_t* __restrict__ mptr,
                                                        const uint32_t* __restrict__ members, uint64_t n_coarse,
                                                        const unsigned long long* __restrict__ small, int64_t* __restrict__ len,
                                                        unsigned long long* __restrict__ selfq, const int64_t* __restrict__ cptr,
                                                        uint32_t* __restrict__ cind, unsigned long long* __restrict__ cacc) {
    constexpr int W = kLvBits / 32, PER = W / 256;
    __shared__ uint32_t bits[W];
    __shared__ uint32_t pre[W];
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const uint32_t a = blockIdx.x;
    const uint32_t old = oldof[a];
    const int64_t mlo = mptr[old], mhi = mptr[old + 1];
    const double scale = reinterpret_cast<const double*>(small)[LV_SCALE];
    const uint64_t out0 = FILL ? (uint64_t)cptr[a] : 0;
    long long self_acc = 0;
    uint64_t done = 0;
    for (uint64_t base = 0; base < n_coarse; base += kLvBits) {
        for (int w = tid; w < W; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int64_t m = mlo + wave; m < mhi; m += 4) {
            const uint32_t i = members[m];
            const uint64_t lo = g.ptr[i], hi = g.ptr[i + 1];
            for (uint64_t e = lo + lane; e < hi; e += kWave) {
                const uint32_t b = (uint32_t)newid[comm[g.ind[e]]];
                if (b == a) {
                    if (!FILL && base == 0) self_acc += lv_fix(g.w[e], scale);
                } else {
                    const uint64_t s = (uint64_t)b - base;           // below base: wraps to a huge number
                    if (s < (uint64_t)kLvBits) atomicOr(&bits[s >> 5], 1u << (s & 31));
                }
            }
            if (!FILL && base == 0 && lane == 0 && g.self) self_acc += lv_fix(g.self[i], scale);
        }
        __syncthreads();
        const uint32_t total = bitmap_prefix_fill<W, PER>(bits, FILL ? pre : nullptr, wtot);      // (!FILL: the row's length alone)
        if (FILL && total) {
            for (int w = 0; w < PER; ++w) {                  // the columns of this thread's own words
                const int word = tid * PER + w;
                uint32_t run = pre[word], bw = bits[word];
                while (bw) {
                    const int bit = __ffs((int)bw) - 1;
                    bw &= bw - 1;
                    cind[out0 + done + run++] = (uint32_t)(base + (uint64_t)word * 32 + bit);
                }
            }
            __syncthreads();
            for (int64_t m = mlo + wave; m < mhi; m += 4) {
                const uint32_t i = members[m];
                const uint64_t lo = g.ptr[i], hi = g.ptr[i + 1];
                for (uint64_t e = lo + lane; e < hi; e += kWave) {
                    const uint32_t b = (uint32_t)newid[comm[g.ind[e]]];
                    const uint64_t s = (uint64_t)b - base;
                    if (b != a && s < (uint64_t)kLvBits) {
                        const uint32_t r = bitmap_rank(bits, pre, (uint32_t)s);
                        atomicAdd(&cacc[out0 + done + r], (unsigned long long)lv_fix(g.w[e], scale));
                    }
                }
            }
        }
        done += total;
        __syncthreads();
    }
    if (!FILL) {
        if (tid == 0) len[a] = (int64_t)done;
        self_acc = wave_sum(self_acc);
        if (lane == 0 && self_acc) atomicAdd(&selfq[a], (unsigned long long)self_acc);
    }
}

// in place: the 8 bytes of a fixed-point sum become the f64 it stands for
__global__ void __launch_bounds__(256) k_louvain_unfix(unsigned long long* __restrict__ acc, uint64_t count,
                                                       const unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double v = (double)(long long)acc[i] * reinterpret_cast<const double*>(small)[LV_INV];
    acc[i] = (unsigned long long)__double_as_longlong(v);
}

// cell -> the compact id of its community after this level; level_comm == nullptr: the identity (start)
__global__ void __launch_bounds__(256) k_louvain_compose(uint32_t* __restrict__ cell, uint64_t n_cells, const uint32_t* __restrict__ comm,
                                                         const int64_t* __restrict__ newid) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    cell[i] = comm ? (uint32_t)newid[comm[cell[i]]] : (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_louvain_sizes(const uint32_t* __restrict__ cell, uint64_t n_cells, uint32_t* __restrict__ csize,
                                                       uint32_t* __restrict__ cmin) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_cells) return;
    atomicAdd(&csize[cell[i]], 1u);
    atomicMin(&cmin[cell[i]], (uint32_t)i);
}

// ascending keys = size descending, then smallest member ascending; the padding sorts last
__global__ void __launch_bounds__(256) k_louvain_keys(const uint32_t* __restrict__ csize, const uint32_t* __restrict__ cmin, uint64_t n_comm,
                                                      uint64_t n_pad, unsigned long long* __restrict__ keys) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_pad) return;
    keys[c] = c < n_comm ? ((unsigned long long)(0xFFFFFFFFu - csize[c]) << 32) | cmin[c] : ~0ull;
}

__global__ void __launch_bounds__(256) k_louvain_bitonic(unsigned long long* __restrict__ keys, uint64_t n_pad, uint64_t j, uint64_t k) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t u = t ^ j;
    if (t >= n_pad || u <= t) return;
    const unsigned long long a = keys[t], b = keys[u];
    if ((a > b) == ((t & k) == 0)) {
        keys[t] = b;
        keys[u] = a;
    }
}

__global__ void __launch_bounds__(256) k_louvain_rank(const unsigned long long* __restrict__ keys, uint64_t n_comm,
                                                      const uint32_t* __restrict__ cell, uint32_t* __restrict__ rank) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p < n_comm) rank[cell[(uint32_t)keys[p]]] = (uint32_t)p;
}

__global__ void __launch_bounds__(256) k_louvain_relabel(const uint32_t* __restrict__ cell, uint64_t n_cells, const uint32_t* __restrict__ rank,
                                                         uint32_t* __restrict__ labels) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_cells) labels[i] = rank[cell[i]];
}

// ---- host side ---------------------------------------------------------------------------------------------------------
static int32_t lv_opts(srx_ctx* ctx, const srx_louvain_opts* in, srx_louvain_opts* o) {
    *o = in ? *in : srx_louvain_opts{1.0, 0.0, 0, 0};
    if (!is_pos_finite(o->resolution))
        return fail(ctx, SRX_E_ARG, "louvain: resolution must be a positive finite number");
    if (!(o->min_gain >= 0.0)) return fail(ctx, SRX_E_ARG, "louvain: min_gain must be >= 0");
    if (o->max_levels < 0 || o->max_levels > SRX_LOUVAIN_MAX_LEVELS)
        return fail(ctx, SRX_E_ARG, "louvain: max_levels = %d outside 0..%d", o->max_levels, SRX_LOUVAIN_MAX_LEVELS);
    if (o->max_sweeps < 0) return fail(ctx, SRX_E_ARG, "louvain: max_sweeps = %d is negative", o->max_sweeps);
    if (o->max_levels == 0) o->max_levels = SRX_LOUVAIN_MAX_LEVELS;
    if (o->max_sweeps == 0) o->max_sweeps = 200;
    return SRX_OK;
}

struct LvQ {
    double q;
    uint64_t n_comm;
};

// Q of the labelling `comm` with the totals `tot` on the level graph g; drains the stream
static int32_t lv_modularity(srx_ctx* ctx, const LvGraph& g, const uint32_t* d_comm, const unsigned long long* d_tot, const uint32_t* d_size,
                             unsigned long long* d_small, double gamma, LvQ* out) {
    hipStream_t st = ctx->stream;
    SRX_HIP(ctx, hipMemsetAsync(d_small + LV_IN, 0, 2 * kLvSlots * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(d_small + LV_NCOMM, 0, 8, st));
    hipLaunchKernelGGL(k_louvain_q_in, dim3(grid256(g.n)), dim3(256), 0, st, g, d_comm, d_small);
    hipLaunchKernelGGL(k_louvain_q_tot, dim3(grid256(g.n)), dim3(256), 0, st, d_tot, d_size, g.n, d_small);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t h[LV_WORDS];
    SRX_TRY(d2h(ctx, h, d_small, sizeof h));
    long long in = 0, sq = 0;
    for (int s = 0; s < kLvSlots; ++s) {
        in += (long long)h[LV_IN + s];
        sq += (long long)h[LV_SQ + s];
    }
    double inv, twom;
    memcpy(&inv, &h[LV_INV], 8);
    memcpy(&twom, &h[LV_TWOM], 8);
    out->q = (double)in * inv / twom - gamma * ((double)sq / 2305843009213693952.0);
    out->n_comm = h[LV_NCOMM];
    return SRX_OK;
}

// The run.  in: the input on the device (n >= 1); d_labels: n u32 on the device.
static int32_t louvain_run(srx_ctx* ctx, const SymCsr& in, const srx_louvain_opts& o, uint32_t* d_labels, srx_louvain_info* info) {
    hipStream_t st = ctx->stream;
    const uint64_t n = in.n;
    const double gamma = o.resolution;
    unsigned long long *d_small, *d_tot, *d_hval = nullptr;
    double* d_kdeg;
    long long* d_kq;
    uint32_t *d_size, *d_comm, *d_next, *d_cell, *d_big, *d_oldof, *d_members, *d_cursor, *d_hkey = nullptr;
    int64_t *d_i0, *d_i1, *d_s0, *d_s1;
    SRX_TRY(scratch(ctx, "louvain_small", LV_WORDS * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "louvain_kdeg", n * 8, (void**)&d_kdeg));
    SRX_TRY(scratch(ctx, "louvain_kq", n * 8, (void**)&d_kq));
    SRX_TRY(scratch(ctx, "louvain_tot", n * 8, (void**)&d_tot));
    SRX_TRY(scratch(ctx, "louvain_size", n * 4, (void**)&d_size));
    SRX_TRY(scratch(ctx, "louvain_comm", n * 4, (void**)&d_comm));
    SRX_TRY(scratch(ctx, "louvain_next", n * 4, (void**)&d_next));
    SRX_TRY(scratch(ctx, "louvain_cell", n * 4, (void**)&d_cell));
    SRX_TRY(scratch(ctx, "louvain_big", n * 4, (void**)&d_big));
    SRX_TRY(scratch(ctx, "louvain_oldof", n * 4, (void**)&d_oldof));
    SRX_TRY(scratch(ctx, "louvain_members", n * 4, (void**)&d_members));
    SRX_TRY(scratch(ctx, "louvain_cursor", n * 4, (void**)&d_cursor));
    SRX_TRY(scratch(ctx, "louvain_i0", n * 8, (void**)&d_i0));
    SRX_TRY(scratch(ctx, "louvain_i1", n * 8, (void**)&d_i1));
    SRX_TRY(scratch(ctx, "louvain_s0", (n + 1) * 8, (void**)&d_s0));
    SRX_TRY(scratch(ctx, "louvain_s1", (n + 1) * 8, (void**)&d_s1));

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());

    LvGraph g{in, nullptr};
    hipLaunchKernelGGL(k_louvain_compose, dim3(grid256(n)), dim3(256), 0, st, d_cell, n, (const uint32_t*)nullptr, (const int64_t*)nullptr);
    uint64_t n_comm = n;
    double q_prev = 0.0;
    bool have_q = false;
    uint64_t h[LV_WORDS];
    for (int level = 0; level < o.max_levels; ++level) {
        // singletons, degrees, the scale (first level) and 2m
        SRX_HIP(ctx, hipMemsetAsync(d_small, 0, (level == 0 ? LV_WORDS : LV_SHIFT) * 8, st));
        hipLaunchKernelGGL(k_louvain_degree, dim3(grid256(g.n)), dim3(256), 0, st, g, d_kdeg, d_comm, d_size, d_small);
        if (level == 0) {
            hipLaunchKernelGGL(k_louvain_scale, dim3(1), dim3(64), 0, st, d_small, g.n, 0);
            hipLaunchKernelGGL(k_louvain_quant, dim3(grid256(g.n)), dim3(256), 0, st, d_kdeg, g.n, (long long*)nullptr,
                               (unsigned long long*)nullptr, d_small);
            hipLaunchKernelGGL(k_louvain_scale, dim3(1), dim3(64), 0, st, d_small, g.n, 1);
        }
        hipLaunchKernelGGL(k_louvain_quant, dim3(grid256(g.n)), dim3(256), 0, st, d_kdeg, g.n, d_kq, d_tot, d_small);
        hipLaunchKernelGGL(k_louvain_scale, dim3(1), dim3(64), 0, st, d_small, g.n, 2);
        SRX_HIP(ctx, hipGetLastError());
        SRX_TRY(d2h(ctx, h, d_small, sizeof h));
        double twom, kmax, scale;
        memcpy(&twom, &h[LV_TWOM], 8);
        memcpy(&kmax, &h[LV_KMAX], 8);
        memcpy(&scale, &h[LV_SCALE], 8);
        if (!(kmax <= kDblMax)) return fail(ctx, SRX_E_ARG, "louvain: the weights of a row sum to Inf");
        if (twom == 0.0) break;                              // no edges: singletons, Q = 0
        // the asserted range of the fixed point: 2m, the largest sum there is, below 2^61
        if (!(twom * scale < 2305843009213693952.0))
            return fail(ctx, SRX_E_ARG, "louvain: total weight %g leaves the fixed-point range at level %d", twom, level);
        if (!have_q) {
            LvQ q0;
            SRX_TRY(lv_modularity(ctx, g, d_comm, d_tot, d_size, d_small, gamma, &q0));
            q_prev = q0.q;
            have_q = true;
        }
        // rows longer than a wave: their list and their tables
        hipLaunchKernelGGL(k_louvain_classify, dim3(grid256(g.n)), dim3(256), 0, st, g.ptr, g.n, d_i0, d_i1);
        SRX_TRY(scan_exclusive(ctx, d_i0, g.n, d_s0, nullptr));
        SRX_TRY(scan_exclusive(ctx, d_i1, g.n, d_s1, nullptr));
        hipLaunchKernelGGL(k_louvain_biglist, dim3(grid256(g.n)), dim3(256), 0, st, d_i0, d_s0, g.n, d_big);
        SRX_HIP(ctx, hipGetLastError());
        int64_t n_big = 0, n_slots = 0;
        SRX_TRY(d2h(ctx, &n_big, d_s0 + g.n, 8));
        SRX_TRY(d2h(ctx, &n_slots, d_s1 + g.n, 8));
        if (n_big) {
            SRX_TRY(scratch(ctx, "louvain_hkey", (size_t)n_slots * 4, (void**)&d_hkey));
            SRX_TRY(scratch(ctx, "louvain_hval", (size_t)n_slots * 8, (void**)&d_hval));
        }
        uint64_t sweeps = 0, moves = 0;
        int quiet = 0;
        for (int t = 0; t < o.max_sweeps && quiet < 2; ++t) {
            SRX_HIP(ctx, hipMemsetAsync(d_small + LV_MOVES, 0, 8, st));
            hipLaunchKernelGGL(k_louvain_move<32>, dim3(grid256(g.n * 32)), dim3(256), 0, st, g, 0, d_kdeg, d_kq, d_comm, d_tot, d_size,
                               d_next, d_small, gamma, t & 1);
            hipLaunchKernelGGL(k_louvain_move<64>, dim3(grid256(g.n * 64)), dim3(256), 0, st, g, 32, d_kdeg, d_kq, d_comm, d_tot, d_size,
                               d_next, d_small, gamma, t & 1);
            if (n_big)
                hipLaunchKernelGGL(k_louvain_move_big, dim3((unsigned)n_big), dim3(256), 0, st, g, d_big, d_s1, d_hkey, d_hval, d_kdeg, d_kq,
                                   d_comm, d_tot, d_size, d_next, d_small, gamma, t & 1);
            hipLaunchKernelGGL(k_louvain_apply, dim3(grid256(g.n)), dim3(256), 0, st, d_comm, d_next, g.n, d_kq, d_tot, d_size, d_small);
            SRX_HIP(ctx, hipGetLastError());
            uint64_t mv = 0;
            SRX_TRY(d2h(ctx, &mv, d_small + LV_MOVES, 8));
            std::swap(d_comm, d_next);
            ++sweeps;
            moves += mv;
            quiet = mv ? 0 : quiet + 1;
        }
        if (moves == 0) break;
        LvQ q;
        SRX_TRY(lv_modularity(ctx, g, d_comm, d_tot, d_size, d_small, gamma, &q));
        if (!(q.q > q_prev + o.min_gain)) break;              // the level is discarded
        // compact ids; the level is kept
        hipLaunchKernelGGL(k_louvain_flag, dim3(grid256(g.n)), dim3(256), 0, st, d_size, g.n, d_i0, d_i1);
        SRX_TRY(scan_exclusive(ctx, d_i0, g.n, d_s0, nullptr));          // newid
        hipLaunchKernelGGL(k_louvain_compose, dim3(grid256(n)), dim3(256), 0, st, d_cell, n, d_comm, d_s0);
        SRX_HIP(ctx, hipGetLastError());
        q_prev = q.q;
        n_comm = q.n_comm;
        info->level_communities[info->n_levels] = q.n_comm;
        info->level_modularity[info->n_levels] = q.q;
        info->n_levels++;
        info->sweeps += sweeps;
        info->moves += moves;
        if (level + 1 == o.max_levels || n_comm <= 1) break;
        // the next level's graph
        SRX_TRY(scan_exclusive(ctx, d_i1, g.n, d_s1, nullptr));          // member offsets by old id
        hipLaunchKernelGGL(k_louvain_oldof, dim3(grid256(g.n)), dim3(256), 0, st, d_i0, d_s0, g.n, d_oldof);
        SRX_HIP(ctx, hipMemsetAsync(d_cursor, 0, g.n * 4, st));
        hipLaunchKernelGGL(k_louvain_members, dim3(grid256(g.n)), dim3(256), 0, st, d_comm, g.n, d_s1, d_cursor, d_members);
        const char* set = (level & 1) ? "b" : "a";
        char name[4][32];
        snprintf(name[0], 32, "louvain_%s_ptr", set);
        snprintf(name[1], 32, "louvain_%s_ind", set);
        snprintf(name[2], 32, "louvain_%s_w", set);
        snprintf(name[3], 32, "louvain_%s_self", set);
        int64_t *d_len, *d_cptr;
        unsigned long long *d_selfq, *d_cacc;
        uint32_t* d_cind;
        SRX_TRY(scratch(ctx, "louvain_len", n_comm * 8, (void**)&d_len));
        SRX_TRY(scratch(ctx, name[0], (n_comm + 1) * 8, (void**)&d_cptr));
        SRX_TRY(scratch(ctx, name[3], n_comm * 8, (void**)&d_selfq));
        SRX_HIP(ctx, hipMemsetAsync(d_selfq, 0, n_comm * 8, st));
        hipLaunchKernelGGL(k_louvain_coarse<false>, dim3((unsigned)n_comm), dim3(256), 0, st, g, d_comm, d_s0, d_oldof, d_s1, d_members, n_comm,
                           d_small, d_len, d_selfq, (const int64_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr);
        SRX_TRY(scan_exclusive(ctx, d_len, n_comm, d_cptr, nullptr));
        int64_t nnz_c = 0;
        SRX_TRY(d2h(ctx, &nnz_c, d_cptr + n_comm, 8));
        SRX_TRY(scratch(ctx, name[1], at_least_one((uint64_t)nnz_c) * 4, (void**)&d_cind));
        SRX_TRY(scratch(ctx, name[2], at_least_one((uint64_t)nnz_c) * 8, (void**)&d_cacc));
        SRX_HIP(ctx, hipMemsetAsync(d_cacc, 0, at_least_one((uint64_t)nnz_c) * 8, st));
        hipLaunchKernelGGL(k_louvain_coarse<true>, dim3((unsigned)n_comm), dim3(256), 0, st, g, d_comm, d_s0, d_oldof, d_s1, d_members, n_comm,
                           d_small, (int64_t*)nullptr, (unsigned long long*)nullptr, d_cptr, d_cind, d_cacc);
        hipLaunchKernelGGL(k_louvain_unfix, dim3(grid256((uint64_t)nnz_c)), dim3(256), 0, st, d_cacc, (uint64_t)nnz_c, d_small);
        hipLaunchKernelGGL(k_louvain_unfix, dim3(grid256(n_comm)), dim3(256), 0, st, d_selfq, n_comm, d_small);
        SRX_HIP(ctx, hipGetLastError());
        g = LvGraph{SymCsr{reinterpret_cast<const uint64_t*>(d_cptr), d_cind, reinterpret_cast<const double*>(d_cacc), n_comm, (uint64_t)nnz_c},
                    reinterpret_cast<const double*>(d_selfq)};
    }
    // final labels: communities by (size descending, smallest member)
    uint64_t n_pad = 1;
    while (n_pad < n_comm) n_pad <<= 1;
    unsigned long long* d_keys;
    uint32_t *d_csize = d_size, *d_cmin = d_next, *d_rank = d_comm;      // the level's arrays are free now
    SRX_TRY(scratch(ctx, "louvain_keys", n_pad * 8, (void**)&d_keys));
    SRX_HIP(ctx, hipMemsetAsync(d_csize, 0, n_comm * 4, st));
    SRX_HIP(ctx, hipMemsetAsync(d_cmin, 0xFF, n_comm * 4, st));
    hipLaunchKernelGGL(k_louvain_sizes, dim3(grid256(n)), dim3(256), 0, st, d_cell, n, d_csize, d_cmin);
    hipLaunchKernelGGL(k_louvain_keys, dim3(grid256(n_pad)), dim3(256), 0, st, d_csize, d_cmin, n_comm, n_pad, d_keys);
    for (uint64_t k = 2; k <= n_pad; k <<= 1)
        for (uint64_t j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_louvain_bitonic, dim3(grid256(n_pad)), dim3(256), 0, st, d_keys, n_pad, j, k);
    hipLaunchKernelGGL(k_louvain_rank, dim3(grid256(n_comm)), dim3(256), 0, st, d_keys, n_comm, d_cell, d_rank);
    hipLaunchKernelGGL(k_louvain_relabel, dim3(grid256(n)), dim3(256), 0, st, d_cell, n, d_rank, d_labels);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(timer.stop(&info->ms));
    info->n = n;
    info->n_communities = n_comm;
    info->modularity = have_q ? q_prev : 0.0;
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_louvain(srx_graph* g, const srx_louvain_opts* opts, uint32_t* labels_out, srx_louvain_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    srx_louvain_opts o;
    SRX_TRY(lv_opts(ctx, opts, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_louvain_info li{};
    li.n = g->n;
    g->labels_valid = false;
    if (g->n) {
        Range rg("louvain");
        if (!g->d_labels) SRX_HIP(ctx, hipMalloc((void**)&g->d_labels, g->n * 4));
        SRX_TRY(louvain_run(ctx, connectivities(g), o, g->d_labels, &li));
        if (labels_out) SRX_TRY(d2h(ctx, labels_out, g->d_labels, g->n * 4));
    }
    g->labels_valid = true;
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_louvain_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                        const srx_louvain_opts* opts, uint32_t* labels_out, srx_louvain_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "louvain: rows are sharded; clustering needs the whole graph");
    srx_louvain_opts o;
    SRX_TRY(lv_opts(ctx, opts, &o));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_louvain_info li{};
    if (n == 0) {
        if (info) *info = li;
        return SRX_OK;
    }
    Range rg("louvain");
    SymCsr in;
    SRX_TRY(symcsr_to_device(ctx, "louvain", indptr, indices, weights, n, &in));
    uint32_t* d_labels;
    SRX_TRY(scratch(ctx, "louvain_labels", n * 4, (void**)&d_labels));
    SRX_TRY(louvain_run(ctx, in, o, d_labels, &li));
    if (labels_out) SRX_TRY(d2h(ctx, labels_out, d_labels, n * 4));
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_graph_labels_fetch(srx_graph* g, uint32_t* labels_out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->labels_valid) return fail(ctx, SRX_E_ARG, "srx_graph_labels_fetch: no srx_louvain has run on this graph");
    if (!g->n) return SRX_OK;
    if (!labels_out) return fail(ctx, SRX_E_ARG, "srx_graph_labels_fetch: null output");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, labels_out, g->d_labels, g->n * 4);
}

}  // extern "C"
