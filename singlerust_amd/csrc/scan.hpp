// scan.hpp — device-side prefix sums, lane-group and workgroup sums and bitmap ranks, stated once for every kernel that needs one (device code only;
// scan.hip has the device-wide scan_exclusive built on them).
#pragma once

#include "common.hpp"

namespace srx {

// Inclusive prefix sum of v over the wave's lanes.  ALL 64 LANES MUST BE ACTIVE (the shuffle reads lanes that sit out as
// garbage): call it from wave-uniform control flow and give the lanes behind the data a zero.
template <typename T>
__device__ __forceinline__ T wave_scan_inclusive(T v) {
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T o = __shfl_up(v, off, kWave);
        if (lane >= off) v += o;
    }
    return v;
}

// Exclusive prefix sum of v over the threads of a workgroup of WAVES full waves; `total` = the sum over all of them, in
// every thread.  `s_wave` (LDS) holds the wave totals: the ONE barrier in here lies between writing and reading them, so
// the CALLER owns the barrier between this call's reads and the next call's writes (a looped site ends its round with one).
template <int WAVES, typename T>
__device__ __forceinline__ T block_scan_exclusive(T v, T* s_wave, T& total) {
    const int wave = threadIdx.x / kWave;
    const T inc = wave_scan_inclusive(v);
    if (lane_id() == kWave - 1) s_wave[wave] = inc;
    __syncthreads();
    T before = 0;
    total = 0;
    for (int w = 0; w < WAVES; ++w) {
        const T t = s_wave[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + inc - v;
}

// Sum of v over each aligned group of G consecutive lanes (G a power of two <= 64), in every lane of the group: a butterfly
// of log2(G) steps whose shape depends on G alone, so a floating-point sum is the same bits from call to call.  ALL 64
// LANES MUST BE ACTIVE, as for the scan above.
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
    return v;
}

// Sum of v over the threads of a workgroup of WAVES full waves, in every thread: the butterfly of wave_sum, then the wave
// totals added in ascending wave order, left to right — ((s0 + s1) + s2) + s3 for four waves — so a floating-point sum is
// the same bits from call to call.  `s_wave` (LDS, WAVES entries): one barrier stands before its write (whoever still
// reads it from an earlier call is done), one after.  EVERY THREAD of the workgroup calls it.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum(T v, T* s_wave) {
    v = wave_sum(v);
    __syncthreads();
    if (lane_id() == 0) s_wave[threadIdx.x / kWave] = v;
    __syncthreads();
    T t = s_wave[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t += s_wave[w];
    return t;
}
// The same total in THREAD 0 ALONE, zero in every other thread: for a kernel whose thread 0 hands the sum on with an atomic
// and whose other threads have no use for it (k_umap_epoch: profiles/shared.md).  ONE barrier, between the write of
// `s_wave` and thread 0's reads: as for block_scan_exclusive, the CALLER owns the barrier between this call's reads and
// the next writes of `s_wave`.
template <int WAVES, typename T>
__device__ __forceinline__ T block_sum_thread0(T v, T* s_wave) {
    v = wave_sum(v);
    if (lane_id() == 0) s_wave[threadIdx.x / kWave] = v;
    __syncthreads();
    if (threadIdx.x != 0) return 0;
#pragma unroll
    for (int w = 1; w < WAVES; ++w) v += s_wave[w];
    return v;
}
// the same as block_sum for the maximum
template <int WAVES, typename T>
__device__ __forceinline__ T block_max(T v, T* s_wave) {
    v = wave_max(v);
    __syncthreads();
    if (lane_id() == 0) s_wave[threadIdx.x / kWave] = v;
    __syncthreads();
    T t = s_wave[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) t = s_wave[w] > t ? s_wave[w] : t;
    return t;
}

// ---- bitmap ranks: one bit per key in `bits`, pre[w] = set bits in the words before w; the place of key s among the set
// keys is pre[s / 32] + the set bits of its word below it.
// `word` = bits[s >> 5] as the caller has loaded it (to test the key's own bit first)
__device__ __forceinline__ uint32_t bitmap_rank_word(uint32_t word, const uint32_t* pre, uint32_t s) {
    return pre[s >> 5] + (uint32_t)__popc(word & ((1u << (s & 31)) - 1u));
}
__device__ __forceinline__ uint32_t bitmap_rank(const uint32_t* bits, const uint32_t* pre, uint32_t s) {
    return bitmap_rank_word(bits[s >> 5], pre, s);
}
// pre[0 .. W) from bits[0 .. W) by a workgroup of W / PER threads, thread t taking the PER consecutive words from t * PER;
// returns the number of set bits (`pre` null: that number alone).  The bits are visible to the workgroup on entry; barriers
// as block_scan_exclusive, and the caller's barrier also stands between these writes of `pre` and the other threads' reads.
template <int W, int PER>
__device__ __forceinline__ uint32_t bitmap_prefix_fill(const uint32_t* bits, uint32_t* pre, uint32_t* s_wave) {
    const int w0 = threadIdx.x * PER;
    uint32_t mine = 0;
    for (int w = 0; w < PER; ++w) mine += (uint32_t)__popc(bits[w0 + w]);
    uint32_t total;
    uint32_t run = block_scan_exclusive<W / PER / kWave>(mine, s_wave, total);
    for (int w = 0; pre && w < PER; ++w) {
        pre[w0 + w] = run;
        run += (uint32_t)__popc(bits[w0 + w]);
    }
    return total;
}

}  // namespace srx
