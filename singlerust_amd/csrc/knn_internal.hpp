// knn_internal.hpp — what knn.hip (the exact search) and knn_ivf.hip (the inverted-file index) share, each stated once:
//   host    the constants and the (K, RT) instance table of the candidate pass with its dispatch, its dynamic LDS and its
//           candidate counts; the launcher of the f32 copy (the kernel is in knn.hip); the entry points of the exact search
//           on device pointers
//   device  the ordered f32 keys and the LDS merge of one query's entries; the f64 distance, its order and the keep step of
//           the f64 selection; the certificate's eps_row
// The certificate is derived in knn.hip's header.  The tile loops of the two candidate kernels (k_knn_candidates and
// k_ivf_candidates) are still two statements of one loop: see the note at k_ivf_candidates.
#pragma once

#include "common.hpp"

#include <algorithm>
#include <type_traits>
#include <utility>

namespace srx {

constexpr int kKnnSlack = 8;         // K' = k + 8 (profiles/knn.md: share of recomputed rows)
constexpr int kKnnMaxK = 64;
constexpr int kKnnQB = 128;          // queries of a workgroup: 4 waves x 32 columns of the 32x32 MFMA tile
constexpr int kKnnPad = 64;          // points are padded to whole reference tiles (the largest RT)
constexpr int kKnnCapMax = 120;      // kept + pending entries per query in LDS (two per lane in a merge)
constexpr uint32_t kKnnNone = 0xFFFFFFFFu;

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// ---- the instances of the candidate pass -------------------------------------------------------------------------------
// K: padded coordinates of the f32 copy (even, > d); RT: references per tile.  Both candidate kernels exist at these pairs.
struct KnnInstance {
    int K, RT;
};
constexpr KnnInstance kKnnInstances[] = {{8, 64}, {20, 64}, {36, 64}, {52, 64}, {68, 64}, {132, 32}};
constexpr size_t kKnnInstanceCount = sizeof kKnnInstances / sizeof kKnnInstances[0];

// padded coordinate count of the f32 copy: d + 1 (the norm) rounded up to the next instantiated width
inline int knn_padded_width(int d) {
    for (const KnnInstance& i : kKnnInstances)
        if (d < i.K) return i.K;
    return kKnnInstances[kKnnInstanceCount - 1].K;
}

// f(integral_constant K, integral_constant RT) of the instance of width K; a width with no instance is an error
template <class F, size_t... I>
int32_t knn_dispatch_at(int K, F&& f, std::index_sequence<I...>) {
    int32_t rc = SRX_E_ARG;
    (void)((K == kKnnInstances[I].K &&
            (rc = f(std::integral_constant<int, kKnnInstances[I].K>{}, std::integral_constant<int, kKnnInstances[I].RT>{}), true)) ||
           ...);
    return rc;
}
template <class F>
int32_t knn_dispatch(int K, F&& f) {
    return knn_dispatch_at(K, f, std::make_index_sequence<kKnnInstanceCount>{});
}

// dynamic LDS of a candidate kernel: 2 tiles | keys 128 x CAP | cnt 128 | tau 128
constexpr size_t knn_candidates_lds(int K, int RT, int CAP) {
    return (size_t)2 * RT * K * 4 + (size_t)kKnnQB * CAP * 8 + (size_t)kKnnQB * 8;
}

// KP = K': candidates kept per query (or per (query, probe) pair); CAP: entries a query slot holds between two merges
struct KnnCounts {
    int KP, CAP;
};
inline KnnCounts knn_candidate_counts(int k, uint64_t admissible) {
    const int KP = (int)std::min<uint64_t>((uint64_t)k + kKnnSlack, std::max<uint64_t>(admissible, 1));
    return {KP, std::min(2 * KP + 32, kKnnCapMax)};
}

// ---- one query's entries in LDS ------------------------------------------------------------------------------------------
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

// ---- the f64 selection -----------------------------------------------------------------------------------------------------
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

// The keep step of a wave that holds n <= k sorted entries (D, I: room for k + 64): the lanes with ok append (dd, idx), the
// n <= k + 64 <= 128 entries are ranked by (distance, index) and cut back to k.  Returns the new n (wave-uniform).
__device__ __forceinline__ int knn_take(double* __restrict__ D, uint32_t* __restrict__ I, int n, int k, bool ok, double dd,
                                        uint32_t idx) {
    const int lane = lane_id();
    const unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
    if (m == 0ull) return n;
    if (ok) {
        const int pos = n + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        D[pos] = dd;
        I[pos] = idx;
    }
    n += __builtin_popcountll(m);
    wave_lds_sync();
    const double d0 = lane < n ? D[lane] : 0.0, d1 = lane + 64 < n ? D[lane + 64] : 0.0;
    const uint32_t i0 = lane < n ? I[lane] : 0u, i1 = lane + 64 < n ? I[lane + 64] : 0u;
    int r0 = 0, r1 = 0;
    for (int e = 0; e < n; ++e) {
        const double de = D[e];
        const uint32_t ie = I[e];
        r0 += knn_less(de, ie, d0, i0);
        r1 += knn_less(de, ie, d1, i1);
    }
    wave_lds_sync();
    if (lane < n && r0 < k) { D[r0] = d0; I[r0] = i0; }
    if (lane + 64 < n && r1 < k) { D[r1] = d1; I[r1] = i1; }
    wave_lds_sync();
    return n < k ? n : k;
}

// ---- the certificate (knn.hip's header) ------------------------------------------------------------------------------------
constexpr double kKnnU = 5.9604644775390625e-08;              // u = 2^-24, the unit roundoff of f32
constexpr double kKnnRMin = 9.094947017729282e-13;            // 2^-40: below, products of the pass may underflow in f32
constexpr double kKnnRMax = 1.152921504606847e18;             // 2^60
struct KnnBound {
    double eps_row, qn;              // the bound on |s - t| of every reference of this query row; |q - c|^2
};
// eps_row of the query row at qp for a pass of width Kpad, +inf when R lies outside the guard.  A row with k exact distances
// is proven when (d_k^2 - qn) + eps_row < tau, tau the bound of everything the pass left out.
__device__ __forceinline__ KnnBound knn_certificate(const double* __restrict__ qp, const double* __restrict__ centre, int d, int Kpad,
                                                    const unsigned long long* __restrict__ rmax2_bits) {
    double qn = 0.0;
    for (int c = 0; c < d; ++c) {
        const double v = qp[c] - centre[c];
        qn += v * v;
    }
    const double R2 = __longlong_as_double((long long)*rmax2_bits), R = sqrt(R2);
    double eps = 1.01 * (double)(Kpad + 4) * kKnnU * (2.0 * sqrt(qn) * R + R2);
    if (!(R >= kKnnRMin && R <= kKnnRMax)) eps = (double)__builtin_inff();
    return {eps, qn};
}

// ---- knn.hip: the f32 copy and the exact search on device pointers -----------------------------------------------------
// The f32 copy of x - centre in MFMA fragment order (k_knn_fragments), n_pad positions of K floats into `out`.  Position p is point ids[p]
// (kKnnNone: padding); ids null: point p below n, padding above.  Coordinate kk < d: x - c; kk == d: |x - c|^2, +inf for a
// padding position (never below any threshold); above: 0.  rmax2_bits non-null: raised to the largest |x - c|^2 (as bits).
int32_t knn_prepare(srx_ctx* ctx, const double* d_x, size_t ld, const uint32_t* d_ids, uint64_t n, uint64_t n_pad, int d, int K,
                    const double* d_centre, float* d_out, unsigned long long* d_rmax2_bits);

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
