// knn_internal.hpp — what knn.hip (the exact search) and knn_ivf.hip (the inverted-file index) share: the constants of the
// candidate pass, the ordered f32 keys and the LDS merge of one query's entries, the f64 distance and its order, and the
// host entry points of the exact search on device pointers.  The certificate both files apply is stated in knn.hip's header.
#pragma once

#include "common.hpp"

namespace srx {

constexpr int kKnnSlack = 8;         // K' = k + 8 (profiles/knn.md: share of recomputed rows)
constexpr int kKnnMaxK = 64;
constexpr int kKnnQB = 128;          // queries of a workgroup: 4 waves x 32 columns of the 32x32 MFMA tile
constexpr int kKnnPad = 64;          // points are padded to whole reference tiles (the largest RT)
constexpr int kKnnCapMax = 120;      // kept + pending entries per query in LDS (two per lane in a merge)
constexpr uint32_t kKnnNone = 0xFFFFFFFFu;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// f32 -> u32 with the same order (negative scores occur: t = dist^2 - |q|^2)
__device__ __forceinline__ uint32_t f32_key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// One query's entries in LDS: u64 keys (ordered score bits << 32 | reference index), so (score, index) order is one compare.
// Merge of the n <= 120 entries of query slot `qs` by one wave: every lane ranks its (up to) two entries against all,
// the KP lowest go to their rank (sorted), the count falls to min(n, KP); returns the score that is now the bound.
__device__ __forceinline__ void knn_merge(unsigned long long* __restrict__ keys, int* __restrict__ cnt, float* __restrict__ tau,
                                          int qs, int CAP, int KP) {
    const int lane = lane_id();
    unsigned long long* e = keys + (size_t)qs * CAP;
    const int n = cnt[qs];
    const unsigned long long e0 = lane < n ? e[lane] : ~0ull, e1 = lane + 64 < n ? e[lane + 64] : ~0ull;
    int r0 = 0, r1 = 0;
    for (int m = 0; m < n; ++m) {
        const unsigned long long o = e[m];      // all lanes read the same word: a broadcast
        r0 += o < e0;
        r1 += o < e1;
    }
    wave_lds_sync();
    if (lane < n && r0 < KP) e[r0] = e0;         // keys are distinct (distinct indices): ranks are a permutation
    if (lane + 64 < n && r1 < KP) e[r1] = e1;
    if (n > KP) {
        if (lane < n && r0 == KP - 1) tau[qs] = key_f32((uint32_t)(e0 >> 32));
        if (lane + 64 < n && r1 == KP - 1) tau[qs] = key_f32((uint32_t)(e1 >> 32));
        if (lane == 0) cnt[qs] = KP;
    }
    wave_lds_sync();
}

// The reported squared distance: the differences of the ORIGINAL coordinates, summed in coordinate order.
__device__ __forceinline__ double knn_dist2(const double* __restrict__ a, const double* __restrict__ b, int d) {
    double s = 0.0;
    for (int c = 0; c < d; ++c) {
        const double t = a[c] - b[c];
        s += t * t;
    }
    return s;
}
__device__ __forceinline__ bool knn_less(double da, uint32_t ia, double db, uint32_t ib) { return da < db || (da == db && ia < ib); }

// padded coordinate count of the f32 copy: d + 1 (the norm) rounded up to the next instantiated width of the candidate pass
inline int knn_padded_width(int d) { return d < 8 ? 8 : d < 20 ? 20 : d < 36 ? 36 : d < 52 ? 52 : d < 68 ? 68 : 132; }

// ---- knn.hip: the exact search on device pointers ----------------------------------------------------------------------
struct KnnArgs {
    const double *d_ref, *d_qry;     // device, row-major with pitches ld_r / ld_q (doubles); d_qry == d_ref for a self graph
    uint64_t n_ref, n_query;
    size_t ld_r, ld_q;
    int d;
    bool self;
};
// The list goes to the "knn_idx" / "knn_dist" scratch slots (n_query x k row-major, valid until the next search on the context)
// and to the host pointers that are not null.
int32_t knn_device(srx_ctx* ctx, const KnnArgs& a, const srx_knn_opts* opts, uint32_t* indices_out, double* distances_out,
                   srx_knn_info* info);
// argument checks shared by the entry points; d_full: coordinates per point, *d_out: those used
int32_t knn_check(srx_ctx* ctx, const srx_knn_opts* opts, uint64_t n_ref, uint64_t n_query, uint64_t d_full, bool self, int* d_out);
// k_knn_exact<true>: the f64 selection over ALL references for the n_rows query rows listed in d_rows, written to their rows
// of d_idx / d_dist (n_query x k)
int32_t knn_exact_rows(srx_ctx* ctx, const KnnArgs& a, int k, int self_skip, const uint32_t* d_rows, uint64_t n_rows,
                       uint32_t* d_idx, double* d_dist);

}  // namespace srx
