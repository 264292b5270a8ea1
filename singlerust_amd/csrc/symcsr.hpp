// symcsr.hpp — a symmetric weighted graph in CSR form as the device sees it, and the checked upload of a caller-supplied one
// (symcsr.hip).  Shared by the graph algorithms: louvain.hip, umap.hip, diffmap.hip.
#pragma once

#include "common.hpp"

namespace srx {

struct SymCsr {                          // n rows, nnz entries: row i is [ptr[i], ptr[i + 1]) of ind / w
    const uint64_t* ptr;
    const uint32_t* ind;
    const double* w;
    uint64_t n, nnz;
};

// The host CSR (n >= 1) checked and left in the context's scratch: the row offsets on the host (everything on the device
// indexes through them), the rest by k_symcsr_check.  `who` starts every message.  Drains the stream.
int32_t symcsr_to_device(srx_ctx* ctx, const char* who, const uint64_t* indptr, const uint32_t* indices, const double* weights,
                         uint64_t n, SymCsr* out);

}  // namespace srx
