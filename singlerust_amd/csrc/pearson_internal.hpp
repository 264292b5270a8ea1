// pearson_internal.hpp — what pearson.hip (the residual variances, the selection, the block of residuals) and pearson_pca.hip
// (the PCA of the residuals) share: the arguments of a residual, the residual itself in the order srx.h states, and the
// preparation every call starts with (the value check, r, g, T).
#pragma once

#include "common.hpp"

// srx.h states the order of every operation of a residual: each translation unit that includes this file states
// `#pragma clang fp contract(off)` for its own code; pr_resid carries its own, so it does not depend on where it is included.

namespace srx {

struct PrArgs {
    double total;          // T
    double theta;          // the value in use (+inf: Poisson)
    double inv_theta;      // 1 / theta (0: Poisson), the dense form's factor
    double clip;           // the value in use (+inf: none)
    int poisson;
};

// z of srx.h for one pair, in the order written there.  T == 0 makes mu NaN, which fails the test like mu == 0.
__device__ __forceinline__ double pr_resid(double x, double r, double g, const PrArgs& a) {
#pragma clang fp contract(off)
    const double mu = (r * g) / a.total;
    if (!(mu > 0.0)) return 0.0;
    const double s = a.poisson ? sqrt(mu) : sqrt(mu + (mu * mu) / a.theta);
    const double z = (x - mu) / s;
    return fmin(fmax(z, -a.clip), a.clip);
}

struct PrPrep {
    uint64_t n = 0, G = 0;               // cells, genes of X
    const double* d_cell = nullptr;      // r_i
    const double* d_gene = nullptr;      // g_j
    double* d_gene_a = nullptr;          // g_j / T with the T of the WHOLE matrix (pr_prepare's): not the factor of a call that
                                         // replaces d_cell and a.total afterwards (pearson_pca.hip, totals = SELECTED)
    uint64_t n_expressed = 0, n_empty = 0;
    PrArgs a{};
};

// pearson.hip.  The refusals that need no pass over the matrix (a context with several ranks, an open backed session, theta,
// clip), and the values in use
int32_t pr_check_args(srx_mat* m, const srx_pearson_opts* opts, const char* who, PrArgs& a, uint64_t n_cells);
// Everything the calls share: the arguments, the value check, r, g, T and the counts.  One small read-back.
int32_t pr_prepare(srx_mat* m, const srx_pearson_opts* opts, const char* who, PrPrep& p);
void pr_info(const PrPrep& p, srx_pearson_info* info);
// T = sum r_i in the one fixed order of every call, and the number of cells with r_i == 0 (pearson.hip: k_pr_totals)
int32_t pr_totals(srx_ctx* ctx, const double* d_cell, uint64_t n, const double* d_gene, uint64_t G, double* total, uint64_t* n_empty);

}  // namespace srx
