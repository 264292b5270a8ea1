// symcsr.hip — the check of a caller-supplied symmetric CSR graph on the device and its upload, for the entry points that
// take one: srx_louvain_csr, srx_umap_csr, srx_diffmap_csr.
//
// Kernels:
//   k_symcsr_check      wave per row: index range, diagonal, order, weights, W_ij == W_ji
#include "symcsr.hpp"

namespace srx {

enum { kBadRange = 1, kBadDiag = 2, kBadOrder = 4, kBadWeight = 8, kBadSym = 16 };

// wave per row: index range, diagonal, order, weights, W_ij == W_ji by binary search; the findings are OR-ed into *flag
__global__ void __launch_bounds__(256) k_symcsr_check(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ ind,
                                                      const double* __restrict__ w, uint64_t n, unsigned long long* __restrict__ flag) {
    const int lane = lane_id();
    const uint64_t row = global_wave_id();
    if (row >= n) return;
    const uint64_t lo = ptr[row], hi = ptr[row + 1];
    int bad = 0;
    for (uint64_t e = lo + lane; e < hi; e += kWave) {
        const uint32_t j = ind[e];
        const double v = w[e];
        if (!is_pos_finite(v)) bad |= kBadWeight;
        if (e > lo && ind[e - 1] >= j) bad |= kBadOrder;
        if (j >= n) {
            bad |= kBadRange;
            continue;
        }
        if (j == row) {
            bad |= kBadDiag;
            continue;
        }
        // the entry (j, row): a binary search stays inside row j whatever its order
        uint64_t a = ptr[j], b = ptr[j + 1];
        const uint64_t end = b;
        while (a < b) {
            const uint64_t mid = a + ((b - a) >> 1);
            if (ind[mid] < (uint32_t)row) a = mid + 1;
            else b = mid;
        }
        if (!(a < end && ind[a] == (uint32_t)row && __double_as_longlong(w[a]) == __double_as_longlong(v))) bad |= kBadSym;
    }
    if (bad) atomicOr(flag, (unsigned long long)bad);
}

int32_t symcsr_to_device(srx_ctx* ctx, const char* who, const uint64_t* indptr, const uint32_t* indices, const double* weights,
                         uint64_t n, SymCsr* out) {
    if (!indptr) return fail(ctx, SRX_E_ARG, "%s: null indptr", who);
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "%s: more than 2^32 - 2 vertices", who);
    if (indptr[0] != 0) return fail(ctx, SRX_E_ARG, "%s: indptr[0] is not 0", who);
    for (uint64_t i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return fail(ctx, SRX_E_ARG, "%s: indptr decreases at row %llu", who, (unsigned long long)i);
    const uint64_t nnz = indptr[n];
    if (nnz && (!indices || !weights)) return fail(ctx, SRX_E_ARG, "%s: null indices or weights", who);
    uint64_t* d_ptr;
    uint32_t* d_ind;
    double* d_w;
    unsigned long long* d_flag;
    SRX_TRY(scratch(ctx, "symcsr_ptr", (n + 1) * 8, (void**)&d_ptr));
    SRX_TRY(scratch(ctx, "symcsr_ind", at_least_one(nnz) * 4, (void**)&d_ind));
    SRX_TRY(scratch(ctx, "symcsr_w", at_least_one(nnz) * 8, (void**)&d_w));
    SRX_TRY(scratch(ctx, "symcsr_flag", 8, (void**)&d_flag));
    *out = SymCsr{d_ptr, d_ind, d_w, n, nnz};
    SRX_TRY(h2d(ctx, d_ptr, indptr, (n + 1) * 8));
    if (nnz) {
        SRX_TRY(h2d(ctx, d_ind, indices, nnz * 4));
        SRX_TRY(h2d(ctx, d_w, weights, nnz * 8));
    }
    SRX_HIP(ctx, hipMemsetAsync(d_flag, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_symcsr_check, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, ctx->stream, out->ptr, out->ind, out->w, n, d_flag);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t flag = 0;
    SRX_TRY(d2h(ctx, &flag, d_flag, 8));
    if (flag & kBadRange) return fail(ctx, SRX_E_ARG, "%s: a column index is not below n = %llu", who, (unsigned long long)n);
    if (flag & kBadDiag) return fail(ctx, SRX_E_ARG, "%s: the graph has a diagonal entry", who);
    if (flag & kBadOrder) return fail(ctx, SRX_E_ARG, "%s: the columns of a row are not strictly ascending", who);
    if (flag & kBadWeight) return fail(ctx, SRX_E_ARG, "%s: a weight is <= 0, NaN or Inf", who);
    if (flag & kBadSym)
        return fail(ctx, SRX_E_ARG, "%s: the graph is not symmetric (W[i,j] and W[j,i] must both be stored, with the same bits)", who);
    return SRX_OK;
}

}  // namespace srx
