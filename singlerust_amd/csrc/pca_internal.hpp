// pca_internal.hpp — what the three translation units of the PCA path share (pca_form.hip: compaction + Gram formation;
// pca_solve.hip: the sparse products, the k x 64 subspace iteration and the solver driver; pca.hip: selection, the per-matrix
// driver, backed sessions and the C entry points).  Constants, the entry / record formats, small device helpers, the
// descriptors of the compacted matrix, and the functions that cross a translation-unit boundary.  Resolved (the options of a solve) is in pca_schedule.hpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <functional>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "pca_result.hpp"
#include "pca_schedule.hpp"

namespace srx {

constexpr int L = 64;               // panel width l
constexpr int kTThreads = 1024;     // transposed / Gram kernels: one workgroup per CU

// Tile-major view of the compacted matrix: the selected features are cut into tiles of KT compacted columns
constexpr int KT = 256;
// The widest device-side HighlyVariable(n) selection (and backed session): the envelope those routes are tested in
constexpr uint64_t kDevSelMaxK = 8192;

template <typename VT> struct GramPk;
template <> struct __attribute__((aligned(8))) GramPk<float> { int32_t j; float v; };
template <> struct __attribute__((aligned(16))) GramPk<double> { int32_t j; int32_t pad_; double v; };

constexpr int kGramWaves = 16;            // waves per Gram workgroup
constexpr int kGramUnroll = 8;            // suffix loads in flight per wave

// One unit of Gram work: entry (ja, va) times up to 64 consecutive entries of its row's suffix (the suffix starts at the
// entry itself — the diagonal product — and a suffix longer than a wave is cut into several records).
// pos: first suffix entry of this record, relative to its block's first entry; lenrb = lanes | rbase << 8, where
// rbase + jb is the index of G[ja][jb] among the owner's LDS accumulators (gram_row_base: may be negative, jb >= ja).
// (8-byte records — the entry's value fetched in the kernel instead of carried in the record, the piece index in the spare bits
//  of lenrb — were measured in round 3: the bucket pass gains 0.13 ms (0.93 -> 0.80) and the stripe kernel loses 0.45 with a
//  scalar load of the value (it shares lgkmcnt with the LDS atomics: waiting for it drains them) and 1.35 with a wave-uniform
//  vector load (one more L1 access per record).  The value stays in the record.)
template <typename VT> struct GramRec { uint32_t pos, lenrb; VT va; };
// records of a row with n kept entries: sum over suffix lengths L = 1 .. n of ceil(L / 64)
__host__ __device__ __forceinline__ uint64_t gram_row_records(uint64_t n) {
    const uint64_t q = n >> 6, r = n & 63;
    return 32 * q * (q + 1) + r * (q + 1);
}

__device__ __forceinline__ int gram_owner(int c, int sr_shift, int n_wg, int n_stripes) {
    const int s = c >> sr_shift;
    return s < n_wg ? s : n_stripes - 1 - s;
}

// accumulator layout of an owner: stripe A (rows a0 .. a0 + SR - 1, WA = k - a0 columns from a0), then stripe B (rows from
// b0 = the mirrored stripe, WB = k - b0 columns): the offset to which a column index jb >= ja is added
__device__ __forceinline__ int gram_row_base(int ja, int k, int sr_shift, int n_wg, int n_stripes) {
    const int s = ja >> sr_shift, SR = 1 << sr_shift;
    const int s0 = s << sr_shift;                       // first row of ja's stripe
    if (s < n_wg) return (ja - s0) * (k - s0) - s0;
    const int a0 = (n_stripes - 1 - s) << sr_shift;     // the owner's stripe A
    return SR * (k - a0) + (ja - s0) * (k - s0) - s0;
}

// index of (i, j), i <= j, in the packed upper triangle (row-major, row i holds columns i .. k - 1)
__host__ __device__ __forceinline__ size_t tri_index(int i, int j, int k) {
    return (size_t)i * (size_t)k - (size_t)i * (size_t)(i - 1) / 2 + (size_t)(j - i);
}

// ---- small vector helpers ------------------------------------------------------------------------
template <typename PT> struct Vec4;
template <> struct Vec4<float> {
    float4 v;
    __device__ __forceinline__ void load(const float* p) { v = *reinterpret_cast<const float4*>(p); }
    __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = v; }
    __device__ __forceinline__ float& operator[](int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }
};
template <> struct Vec4<double> {
    double2 a, b;
    __device__ __forceinline__ void load(const double* p) {
        a = *reinterpret_cast<const double2*>(p);
        b = *reinterpret_cast<const double2*>(p + 2);
    }
    __device__ __forceinline__ void store(double* p) const {
        *reinterpret_cast<double2*>(p) = a;
        *reinterpret_cast<double2*>(p + 2) = b;
    }
    __device__ __forceinline__ double& operator[](int i) { return i == 0 ? a.x : i == 1 ? a.y : i == 2 ? b.x : b.y; }
};

// DPP row rotate inside each 16-lane row (v_mov_b32_dpp row_ror:S) — no LDS traffic.
template <int S>
__device__ __forceinline__ int ror16(int x) {
    if constexpr (S == 0) return x;
    else return __builtin_amdgcn_update_dpp(0, x, 0x120 + S, 0xf, 0xf, false);
}
template <int S>
__device__ __forceinline__ float ror16(float x) {
    return __builtin_bit_cast(float, ror16<S>(__builtin_bit_cast(int, x)));
}
template <int S>
__device__ __forceinline__ double ror16(double x) {
    long long b = __builtin_bit_cast(long long, x);
    int lo = ror16<S>((int)(b & 0xffffffffll)), hi = ror16<S>((int)(b >> 32));
    return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ int64_t readlane64(int64_t x, int l) {
    int lo = __builtin_amdgcn_readlane((int)(x & 0xffffffffll), l);
    int hi = __builtin_amdgcn_readlane((int)(x >> 32), l);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}
__device__ __forceinline__ float readlane_v(float x, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
}
__device__ __forceinline__ double readlane_v(double x, int l) {
    return __builtin_bit_cast(double, readlane64(__builtin_bit_cast(long long, x), l));
}

// ---- compacted matrix: row-major records + the tile-major view of the matrix-free solver ------------
struct Tiled {
    uint64_t n_rows = 0, nnz = 0;
    int k = 0, nt = 0;         // nt = ceil(k / KT) tiles
    int64_t* tptr = nullptr;   // nt * n_rows + 1
    void* tpk = nullptr;       // GramPk<VT> records: (local column within the tile, value)
};
// How G's upper triangle is cut into stripes of SR rows and paired into workgroups (k_gram_stripes)
struct GramPlan {
    int k = 0, sr_shift = 0, n_stripes = 0, n_wg = 0;
    int n_z = 1;               // chunks: the grid is n_wg x n_z workgroups
    uint32_t rblk = 512;       // cells per bucket block
    uint32_t n_chunk = 0;      // consecutive row blocks per workgroup
    uint64_t n_rblk = 0;
    size_t lds_bytes = 0;
};
// X[:, sel] row by row: GramPk<VT> records (compacted column in [0, k), value), columns ascending within a row —
// what the Gram kernel walks (a suffix of a row is one contiguous run)
struct RowMajor {
    uint64_t n_rows = 0, nnz = 0;
    int k = 0;
    int64_t* ptr = nullptr;    // n_rows + 1
    void* pk = nullptr;
    uint32_t* perm = nullptr;  // rows ordered by their number of kept entries (forward SpMM), or null
    int64_t n_recs = -1;       // >= 0: the Gram kernel's record counts were made with the compaction (scratch pca_brtot / pca_brbase
                               // hold them): launch_gram starts at the bucket pass, one host wait less per step
};
// ---- select.hip (and, from genes.hip, the two things it needs beyond common.hpp) ---------------------
// FeatureSelection::HighlyVariable(n) ranked on the host (the CSC variance for a CSC matrix): the route of srx_select_hvg, and of
// the PCA drivers outside hvg_on_device's envelope, which pass the list on
int32_t hvg_list_host(srx_mat* m, uint64_t n, std::vector<uint64_t>& out);
// genes.hip: the nz-only population variance of every gene from the cached moments (csr.rs:179-185), on the host
int32_t gene_variances(srx_mat* m, std::vector<double>& var);
constexpr const char* kNanVarianceMsg = "NaN gene variance: called `Option::unwrap()` on a `None` value (partial_cmp)";
// The selection of a PCA on the device, made by k_sel_finish from a per-gene rank table (context scratch buffers)
struct SelDev {
    int k = 0, n_words = 0;
    int32_t* d_sel_rank = nullptr;   // the k selected gene ids in selection order (what select_features returns)
    uint32_t* d_bits = nullptr;      // n_words selection bits, then n_words prefix counts
    double *d_mu = nullptr, *d_sd = nullptr, *d_dinv = nullptr, *d_trace = nullptr;   // slot order (ascending gene)
    int* d_status = nullptr;         // bit 0: NaN variance (HighlyVariable(n) only)
};
// is FeatureSelection::HighlyVariable(n) ranked on the device (select_hvg_device)?  Else on the host, and passed on as a list
bool hvg_on_device(uint64_t n, uint64_t n_cols);
// needs the global moments of `m` (ensure_moments / moments_install: the callers have them for n_rows_global already)
int32_t select_hvg_device(srx_mat* m, uint64_t n, int center, int scale, SelDev& out);
// an explicit list (`genes`: k distinct features below n_cols in the caller's order; null: every feature, k = n_cols),
// validated; `vectors` false: the selection alone, the moments of `m` are not read
int32_t select_list(srx_mat* m, const uint64_t* genes, uint64_t k, int center, int scale, SelDev& out, bool vectors = true);
// the ranking alone, for any key array: d_rank[j] += the number of genes before j under (key desc, index asc); the caller has
// zeroed d_rank.  pick_top: d_sel[r] = the gene of rank r, for r < take
int32_t rank_keys_device(srx_ctx* ctx, const double* d_key, uint64_t G, uint32_t* d_rank);
int32_t pick_top(srx_ctx* ctx, const uint32_t* d_rank, uint64_t G, uint64_t take, uint64_t* d_sel);
// genes.hip.  E: int32_t column indices or GramPk<VT> records
template <typename E>
int32_t launch_tile_ptr(srx_ctx* ctx, const int64_t* indptr, const E* idx, uint64_t n_rows, int n_tiles, int tile_genes,
                        int64_t* tp);

// ---- pca_form.hip: the HVG-compacted matrix and G = A^T A --------------------------------------------
// (entries_per_cell, entry_bytes: the compacted matrix's mean row length and entry size — they size the stripe kernel's chunks; 0 where
//  only the blocks are wanted)
int32_t gram_plan(srx_ctx* ctx, int k, uint64_t n_rows, GramPlan& g, double entries_per_cell = 0.0, int entry_bytes = 0);
int grid_rows(const srx_ctx* ctx, uint64_t n_rows, int rows_per_block);
// `d_sel`: n_words selection bits followed by n_words prefix counts, on the device (the compacted column of a gene is its rank
// among the selected genes in ascending gene order).  Makes the row-major records, their row order (rm.perm) and, with
// `want_recs`, the Gram kernel's record counts.
int32_t compact_selection(srx_mat* m, const uint32_t* d_sel, int n_words, int k, RowMajor& rm, RowXf xf = RowXf{},
                          bool want_recs = false);
// the tile-major view of the records (the matrix-free solver)
int32_t retile(srx_mat* m, const RowMajor& rm, Tiled& t);
template <typename VT>
int32_t launch_gram(srx_ctx* ctx, const RowMajor& rm, double* Gp, bool* reduce = nullptr, bool zero_first = false);
inline size_t gram_packed_count(int k) { return (size_t)k * (size_t)(k + 1) / 2; }

// ---- pca_solve.hip: products, iteration, solver ------------------------------------------------------
int32_t build_row_order(srx_ctx* ctx, RowMajor& r);
int scores_ld(int n_pc);
// pca_model.inl: srx_pca_transform with feat == NULL, row r of the query written to d_out + r * ld on the device (doublets.hip)
int32_t pca_transform_device(srx_pca_model* p, srx_mat* q, double target_sum, int32_t transform, double* d_out, size_t ld);
void result_layout(uint64_t n_rows, int k, int n_pc, int dim, size_t& score_bytes, size_t& small_doubles,
                   PcaPlans* plans_out = nullptr);
int32_t ensure_result_capacity(srx_ctx* ctx, srx_pca_state& st, size_t need);
int32_t resolve_opts(srx_ctx* ctx, const srx_pca_opts* opts, int k, uint64_t Ng, bool f32, Resolved& o, int& l_act);
inline PcaResultLayout result_block(const srx_pca_state& st) { return PcaResultLayout(st.k, L, st.round_counts); }
// What the resident and the backed driver do with their compacted rows (`parts`: one for a resident matrix, one per row tile in
// backed mode, then `gram_packed` is the packed Gram matrix summed over the tiles; `t256p`: the 256-tiled view, matrix-free
// solver only): st.info, the solve at the precisions of (f32 storage, o.solver), and the small results moved from the context's
// scratch into the matrix's own result block (host copies: pca_materialize).  A solve that broke down before it had a block
// returns its code with st.valid false.
// A second source of the Gram solver (pearson_pca.hip): `parts` null, `gram_packed` the ready packed upper triangle of Z^T Z of a
// DENSE n_rows x k matrix in f64 that never exists as a whole, sel.d_mu its column means.  The round hands its panel to
// `write_scores`, which writes columns [col0, col0 + n_r) of the scores, Z P - 1 cvec^T, at the stride `ld`.
struct DenseSource {
    int k = 0;
    int route = kResidualPearson;    // what srx_pca_state::residual says of the result
    uint64_t n_rows = 0;
    std::function<int32_t(const double* panel, const double* cvec, int col0, int n_r, double* scores, int ld)> write_scores;
};
int32_t solve_and_stash(srx_ctx* ctx, bool f32, const RowMajor* parts, int n_parts, const Tiled* t256p, double* gram_packed,
                        const Resolved& o, const SelDev& sel, int l_act, uint64_t n_cells, uint64_t nnz_selected, srx_pca_state& st,
                        const DenseSource* dense = nullptr);

}  // namespace srx
