// umap_internal.hpp — what the two UMAP iterations share: umap.hip (the layout of a symmetric graph, every vertex moves, one
// launch per epoch) and ingest.hip (the transform of new points against fixed reference positions, many epochs per launch).
// The attraction and repulsion terms of include/srx.h are written once, here.  Everything from this header on is compiled
// with FMA contraction off, so that every operation of the definition is rounded once: include it last.
#pragma once

#include "common.hpp"

#pragma clang fp contract(off)

namespace srx {

constexpr int kUmGroup = SRX_UMAP_GROUP;
// the small block (8-byte words) of a run; k_umap_wmax and k_umap_active fill the first two
enum { UM_WMAX = 0, UM_ACTIVE, UM_SAMPLES, UM_SKIPPED, UM_ABSMAX, UM_PCAMAX, UM_WORDS = 8 };

struct UmParams {
    double a, b, gamma;
    uint64_t seed;
    int rate;
};

template <int DIM>
__device__ __forceinline__ void um_load(const double* __restrict__ y, uint64_t i, double (&p)[DIM]) {
    if constexpr (DIM == 2) {            // one 16-byte load
        const double2 v = reinterpret_cast<const double2*>(y)[i];
        p[0] = v.x;
        p[1] = v.y;
    } else {
#pragma unroll
        for (int c = 0; c < DIM; ++c) p[c] = y[i * DIM + c];
    }
}

// acc += scale * clip(q (y_i - y_o), -4, 4) with q from d2 = |y_i - y_o|^2; `attract`: the attraction of a sampled entry, else the
// repulsion from a negative sample (one body for both, so that pow is expanded once per exponent).  d2 == 0 adds nothing.
template <int DIM>
__device__ __forceinline__ void um_term(const double (&yi)[DIM], const double* __restrict__ y, uint64_t o, const UmParams& p, bool attract,
                                        double coef, double scale, double (&acc)[DIM]) {
    double yo[DIM], d[DIM];
    um_load<DIM>(y, o, yo);
    double d2 = 0.0;
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        d[c] = yi[c] - yo[c];
        d2 = c ? d2 + d[c] * d[c] : d[c] * d[c];
    }
    if (!(d2 > 0.0)) return;
    const double den = p.a * pow(d2, p.b) + 1.0;
    const double q = attract ? coef * pow(d2, p.b - 1.0) / den : coef / ((0.001 + d2) * den);
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
        const double g = fmin(fmax(q * d[c], -4.0), 4.0);
        acc[c] += scale * g;
    }
}

// ---- host side (umap.hip) ------------------------------------------------------------------------------------------------------
// k_umap_wmax and k_umap_active over the nnz weights at d_w, queued on the context's stream: d_small[UM_WMAX] (the bits of the
// largest weight) and d_small[UM_ACTIVE] (the entries with floor(epochs * w / w_max) > 0); the caller zeroed both.  nnz >= 1.
void umap_wmax_active(srx_ctx* ctx, const double* d_w, uint64_t nnz, double epochs, unsigned long long* d_small);
// a, b fitted to (spread, min_dist) as srx_umap_fit_ab fits them, with its refusals
int32_t umap_fit_curve(srx_ctx* ctx, double spread, double min_dist, double* a, double* b);

}  // namespace srx
