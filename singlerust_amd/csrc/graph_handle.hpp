// graph_handle.hpp — the srx_graph handle of srx.h: built by graph.hip, read where it lies by the graph algorithms (louvain.hip,
// umap.hip, diffmap.hip).
#pragma once

#include "common.hpp"
#include "symcsr.hpp"

struct srx_graph {
    srx_ctx* ctx = nullptr;
    uint64_t n = 0;
    uint32_t k = 0;
    // one allocation: D (indptr, indices, data), the directed weights in D's order, rho, sigma
    void* d_block = nullptr;
    uint64_t* d_dptr = nullptr;
    uint32_t* d_dind = nullptr;
    double *d_ddat = nullptr, *d_a = nullptr, *d_rho = nullptr, *d_sigma = nullptr;
    // a second one, sized once nnz is known: C
    void* d_cblock = nullptr;
    uint64_t* d_cptr = nullptr;
    uint32_t* d_cind = nullptr;
    double* d_cdat = nullptr;
    srx_graph_info info{};
    // the labels of the last srx_louvain on this handle (louvain.hip): n u32, allocated by the first call
    uint32_t* d_labels = nullptr;
    bool labels_valid = false;
    // the embedding of the last srx_umap on this handle (umap.hip): n x embed_dim f64, row-major
    double* d_embed = nullptr;
    uint32_t embed_dim = 0;
    bool embed_valid = false;
    // the last srx_diffmap on this handle (diffmap.hip): T's data in C's order (nnz f64), the eigenvectors (n x dm_n_comps f64,
    // row-major) and the eigenvalues; dm_t_valid once T is built, dm_valid once a solve has succeeded
    double* d_dm_t = nullptr;
    double* d_dm_evecs = nullptr;
    std::vector<double> dm_evals;
    uint32_t dm_n_comps = 0;
    bool dm_t_valid = false, dm_valid = false;
};

namespace srx {
// C as the graph algorithms read it, where it lies
inline SymCsr connectivities(const srx_graph* g) { return SymCsr{g->d_cptr, g->d_cind, g->d_cdat, g->n, g->info.nnz_connectivities}; }
// A result kept with the handle (graph.hip): *slot (hipMalloc, freed first when `resized` says the array it holds has another
// size) <- the `bytes` at d_src, queued on the context's stream.  The caller owns the flag that says whether *slot is valid.
int32_t keep_on_handle(srx_ctx* ctx, double** slot, bool resized, const double* d_src, size_t bytes);
}  // namespace srx
