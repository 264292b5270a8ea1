// graph_handle.hpp — the srx_graph handle of srx.h: built by graph.hip, read where it lies by the graph algorithms (louvain.hip,
// umap.hip, diffmap.hip, tsne.hip, draw_graph.hip), and the union of a k-NN list with its transpose that graph.hip builds for C and tsne.hip for P.
#pragma once

#include "common.hpp"
#include "symcsr.hpp"

#include <functional>

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
    // the layout of the last srx_draw_graph on this handle (draw_graph.hip): n x 2 f64, row-major
    double* d_layout = nullptr;
    bool layout_valid = false;
};

namespace srx {
// C as the graph algorithms read it, where it lies
inline SymCsr connectivities(const srx_graph* g) { return SymCsr{g->d_cptr, g->d_cind, g->d_cdat, g->n, g->info.nnz_connectivities}; }
// A result kept with the handle (graph.hip): *slot (hipMalloc, freed first when `resized` says the array it holds has another
// size) <- the `bytes` at d_src, queued on the context's stream.  The caller owns the flag that says whether *slot is valid.
int32_t keep_on_handle(srx_ctx* ctx, double** slot, bool resized, const double* d_src, size_t bytes);

// A new handle with its D block allocated (indptr, indices, data, directed weights, rho, sigma: nothing filled in), and the C
// block of a handle once nnz is known (graph.hip).  A failed graph_alloc leaves *out alone; the caller frees g after the second.
int32_t graph_alloc(srx_ctx* ctx, uint64_t n, uint32_t k, srx_graph** out);
int32_t graph_alloc_c(srx_graph* g, uint64_t nnz);

// ---- the in-lists of a k-NN list (graph.hip): for every cell the sources of the flagged edges that point at it, ascending ----
// Lists of more than kInShort entries are ordered by a workgroup each (k_graph_order_long) into a second pair of arrays, at
// the same offsets; in_list_src picks the array that holds a list.
constexpr int kInShort = 512;
struct InLists {
    int64_t* tptr = nullptr;                 // n + 1 offsets
    uint32_t *tsrc = nullptr, *lsrc = nullptr;
    double *tval = nullptr, *lval = nullptr;
};
__host__ __device__ inline const uint32_t* in_list_src(const uint32_t* tsrc, const uint32_t* lsrc, int64_t lo, int64_t len) {
    return (len > kInShort ? lsrc : tsrc) + lo;
}
// d_indeg: 2 n words, the list lengths (counted by the caller) | n zeroed cursors.  Edge e of row e / k is listed at its
// target d_dind[e] when d_flags[e] & 2, with the value d_val[e].  Scans the lengths, scatters, orders the short lists.
int32_t in_lists_build(srx_ctx* ctx, const uint32_t* d_dind, const double* d_val, const unsigned char* d_flags, uint64_t n,
                       uint32_t k, int64_t* d_indeg, InLists* out);
// ... and the n_long lists named in d_long (the caller's row kernel found them), once the host knows n_long.
int32_t in_lists_order_long(srx_ctx* ctx, uint64_t n, uint32_t k, const uint32_t* d_long, uint64_t n_long, InLists* io);

// ---- the union of a k-NN list with its transpose (graph.hip) -------------------------------------------------------------------
// What a row kernel finds wrong with a list (OR-ed into a flag word), and the refusal that names it: `who` starts the message.
enum { kBadRange = 1, kBadSelf = 2, kBadDup = 4, kBadDist = 8 };
int32_t list_flag_check(srx_ctx* ctx, const char* who, uint64_t n, const int* d_flag);
// The small block of a build: counters spread over kCtrSlots slots (row & 63) of kCtrN words, summed on the host | the longest
// row, the number of long in-only lists | the flag.  The first three counters belong to the caller's row kernel.
constexpr int kCtrSlots = 64;
enum { kCtrNoRoot = 0, kCtrClamped, kCtrAllZero, kCtrMutual, kCtrDropped, kCtrN };
constexpr size_t kPairSmallWords = (size_t)kCtrSlots * kCtrN + 3;
inline int* pair_flag(unsigned long long* d_small) { return reinterpret_cast<int*>(d_small + kPairSmallWords - 1); }
// The value of a pair from its directed weights a and b (0 for an absent direction): the fuzzy union (a + b) - a b, or with
// `mean` the quotient (a + b) / denom.  Both are symmetric in a and b, so the two entries of a pair are the same bits.
struct PairRule {
    int mean;
    double denom;
};
// Where the result goes, once its size is known: (nnz, &indptr (n + 1), &indices, &data), all device pointers.
using PairAlloc = std::function<int32_t(uint64_t, uint64_t**, uint32_t**, double**)>;
// d_dind / d_a: the rows of the list in column order (n x k) and their directed weights.  Builds the CSR of every pair joined
// in either direction, rows ascending by column, pairs whose value is 0.0 dropped.  d_small: kPairSmallWords words the caller
// zeroed (its row kernel may have counted in them); ctr: the host copy, kPairSmallWords - 1 words (kCtrMutual counts both ends
// of a mutual pair, kCtrDropped every dropped entry of the symmetric matrix, word kCtrSlots * kCtrN is the longest row).
int32_t pair_union_csr(srx_ctx* ctx, PairRule rule, const uint32_t* d_dind, const double* d_a, uint64_t n, uint32_t k,
                       unsigned long long* d_small, uint64_t* ctr, uint64_t* nnz_out, const PairAlloc& alloc);
}  // namespace srx
