// dense_pca_internal.hpp — the two products over a dense n x k f64 matrix Z that exists only a chunk of cells at a time, as
// pearson_pca.hip (the clipped Pearson residuals) and regress.hip (regressed, scaled and clipped values) share them.  The
// kernels (k_pp_syrk, k_pp_syrk_reduce, k_pp_colsum, k_pp_colsum_reduce, k_pp_finish, k_pp_scores) and the host loops live in
// pearson_pca.hip, once; a caller hands in what makes a chunk.
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
    double* d_Z = nullptr;          // chunk x ldz doubles (scratch "pp_chunk")
};

// `who`'s list: at most kDenseMaxK distinct indices below G
int32_t dense_check_list(srx_ctx* ctx, const char* who, const uint64_t* genes, uint64_t k, uint64_t G);
// ldz, the chunk size (chunk_cells; 0: what a quarter of the last-level cache holds) and the chunk buffer
int32_t dense_chunks_setup(srx_ctx* ctx, uint64_t n, uint64_t k, uint64_t chunk_cells, DenseChunks& g);
// Gp (packed upper triangle) = Z^T Z and colsum over all chunks in ascending order; both zeroed here
int32_t dense_gram_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, double* Gp, double* colsum, double* ms);
// columns [0, n_r) of S = Z P - 1 cvec^T, row i at out + i * ld; *ms_acc += the time of the pass
int32_t dense_score_pass(srx_ctx* ctx, const DenseChunks& g, const DenseChunkFn& make, const double* P, const double* cvec, int n_r,
                         double* out, int ld, double* ms_acc);
// the selection's vectors from the pass's results: mu = colsum / n (center) or 0, sd = dinv = 1, trace of G - n mu mu^T
int32_t dense_finish(srx_ctx* ctx, const double* Gp, const double* colsum, int k, uint64_t n, int center, const SelDev& sd);

}  // namespace srx
