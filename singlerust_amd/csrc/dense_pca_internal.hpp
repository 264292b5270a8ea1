// dense_pca_internal.hpp — the PCA route over a dense n x k f64 matrix Z that exists only a chunk of cells at a time, as
// pearson_pca.hip (the clipped Pearson residuals) and regress.hip (regressed, scaled and clipped values) walk it.  The products,
// the slot table and the hand-off to the Gram solver live in dense_pca.hip, once; the two kernels that make a chunk are
// templates on the caller's element function and live here.
#pragma once

#include <functional>

#include "pca_internal.hpp"

namespace srx {

constexpr int kDenseTile = 64;      // a tile of Z^T Z; the row stride of a chunk is a whole number of tiles
constexpr int kDenseMaxK = 16384;   // the Gram solver's bound

// rows [row0, row0 + rows) of Z into `Z` at the stride ldz, columns >= k zero; launches on the context's stream
using DenseChunkFn = std::function<int32_t(uint64_t row0, uint64_t rows, double* Z)>;

struct DenseChunks {                // the chunk geometry
    uint64_t n = 0;                 // cells
    int k = 0;                      // columns of Z (slot order)
    uint32_t ldz = 0;               // k rounded up to whole tiles
    uint64_t chunk = 0, n_chunks = 0;
    double* d_Z = nullptr;          // chunk x ldz doubles (scratch "dense_chunk")
};

struct DenseSlots {                 // slot s of the solver and column s of Z: the listed genes in ascending order
    int k = 0;
    std::vector<int> slot_of_pos;   // caller's position -> slot
    int32_t* d_slot_of = nullptr;   // gene -> slot, -1 where the gene is not listed (scratch "dense_slot_of", G entries)
};

struct DenseSolved {                // what dense_pca_solve reports
    bool solved = false;            // the solver ran and returned the call's code: the fields below are set
    double ms_gram = 0.0, ms_solve = 0.0, ms_scores = 0.0;
    srx_pca_info pca{};
};

// `who`'s list: at most kDenseMaxK distinct indices below G
int32_t dense_check_list(srx_ctx* ctx, const char* who, const uint64_t* genes, uint64_t k, uint64_t G);
// the slot table of a checked list, on the host and the device
int32_t dense_slots_setup(srx_ctx* ctx, const uint64_t* genes, uint64_t k, uint64_t G, DenseSlots& s);
// ldz, the chunk size (chunk_cells; 0: what a quarter of the last-level cache holds) and the chunk buffer
int32_t dense_chunks_setup(srx_ctx* ctx, uint64_t n, uint64_t k, uint64_t chunk_cells, DenseChunks& g);
// *Gp (packed upper triangle) = Z^T Z and *colsum over all chunks in ascending order: the route's scratch buffers, zeroed here
int32_t dense_gram_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, double** Gp, double** colsum, double* ms);
// d2h of the packed triangle and the column sums, written in the caller's order (either output may be null)
int32_t dense_gram_fetch(srx_ctx* ctx, const DenseSlots& s, const double* Gp, const double* colsum, double* gram_out, double* colsum_out);
// The PCA of Z into m->pca for resolved options: the selection's buffers with `genes` in the caller's order, the Gram pass over
// make_gram's chunks, mu and the trace (`center`), the Gram solver with the score pass over make_scores' chunks as its writer.
// route: kResidual*; d_sd (k doubles on the device, or null: ones): what the result block reports as std.  Returns the
// solver's code with out.solved set, or an earlier failure with it clear.
int32_t dense_pca_solve(srx_mat* m, const Resolved& o, int l_act, const uint64_t* genes, const DenseChunks& g, const DenseChunkFn& make_gram,
                        const DenseChunkFn& make_scores, int route, int center, const double* d_sd, DenseSolved& out);

// ---- a chunk of Z: rows [row0, row0 + rows) x ldz columns, columns >= k zero --------------------------------------------------------
// Elem is the caller's element function, trivially copyable and passed by value:
//   __device__ double at(double x, uint64_t row, uint32_t slot, bool* clipped) const
// the entry of cell `row` and column `slot` for the stored value x (0: not stored), in the order srx.h states; it carries its
// own `fp contract(off)`, the kernels here do no arithmetic of their own.  Every pair gets the value of a zero entry
// (k_dense_fill), then the stored entries of the chunk's rows overwrite theirs (k_dense_stored).
// COUNT: cnt[0] += the pairs k_dense_fill found clipped (every pair as a zero entry), cnt[1] += the clipped stored entries,
// cnt[2] += those whose overwritten zero-entry value was counted in cnt[0].  Integers: exact in any order.
template <typename Elem, bool COUNT>
__global__ __launch_bounds__(256) void k_dense_fill(uint32_t k, uint32_t ldz, uint64_t row0, uint64_t rows, Elem el, double* __restrict__ Z,
                                                    unsigned long long* __restrict__ cnt) {
    const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= rows * ldz) return;
    const uint64_t i = o / ldz;
    const uint32_t c = (uint32_t)(o - i * ldz);
    bool cl = false;
    Z[o] = c < k ? el.at(0.0, row0 + i, c, &cl) : 0.0;
    if constexpr (COUNT) {
        const unsigned long long b = __ballot(cl);
        if (cl && lane_id() == __ffsll(b) - 1) atomicAdd(cnt, (unsigned long long)__popcll(b));
    }
}
// a wave per row
template <typename T, typename Elem, bool COUNT>
__global__ __launch_bounds__(256) void k_dense_stored(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                                      const T* __restrict__ vals, const int32_t* __restrict__ slot_of, uint32_t ldz,
                                                      uint64_t row0, uint64_t rows, Elem el, double* __restrict__ Z,
                                                      unsigned long long* __restrict__ cnt) {
    const uint64_t i = global_wave_id();
    if (i >= rows) return;
    const uint64_t r = row0 + i;
    const int64_t hi = indptr[r + 1];
    unsigned int n_new = 0, n_old = 0;
    for (int64_t e = indptr[r] + lane_id(); e < hi; e += kWave) {
        const int32_t s = slot_of[idx[e]];
        if (s < 0) continue;
        bool cl, cl0 = false;
        if constexpr (COUNT) (void)el.at(0.0, r, (uint32_t)s, &cl0);      // (first: 20 VGPRs; after the store the two evaluations share nothing, 30)
        Z[i * ldz + (uint32_t)s] = el.at((double)vals[e], r, (uint32_t)s, &cl);
        if constexpr (COUNT) {
            n_new += cl ? 1u : 0u;
            n_old += cl0 ? 1u : 0u;
        }
    }
    if constexpr (COUNT) {
        n_new = wave_sum(n_new);
        n_old = wave_sum(n_old);
        if (lane_id() == 0) {
            if (n_new) atomicAdd(cnt + 1, (unsigned long long)n_new);
            if (n_old) atomicAdd(cnt + 2, (unsigned long long)n_old);
        }
    }
}

// the two launches on the stream of m's context; `m` is a CSR handle of the cells' rows; cnt: COUNT only
template <typename Elem, bool COUNT>
int32_t dense_make_chunk(srx_mat* m, const DenseSlots& s, const DenseChunks& g, const Elem& el, uint64_t row0, uint64_t rows, double* Z,
                         unsigned long long* cnt = nullptr) {
    srx_ctx* ctx = m->ctx;
    hipLaunchKernelGGL((k_dense_fill<Elem, COUNT>), dim3((unsigned)((rows * g.ldz + 255) / 256)), dim3(256), 0, ctx->stream, (uint32_t)g.k, g.ldz,
                       row0, rows, el, Z, cnt);
    const unsigned grid = (unsigned)((rows + 3) / 4);
    if (is_f32(m))
        hipLaunchKernelGGL((k_dense_stored<float, Elem, COUNT>), dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices,
                           (const float*)m->d_values, (const int32_t*)s.d_slot_of, g.ldz, row0, rows, el, Z, cnt);
    else
        hipLaunchKernelGGL((k_dense_stored<double, Elem, COUNT>), dim3(grid), dim3(256), 0, ctx->stream, m->d_indptr, m->d_indices,
                           (const double*)m->d_values, (const int32_t*)s.d_slot_of, g.ldz, row0, rows, el, Z, cnt);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

}  // namespace srx
