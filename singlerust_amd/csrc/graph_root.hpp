// graph_root.hpp — the smooth-k-NN scale of one row of a k-NN list, stated once for the two row kernels that solve it (device
// code only): k_graph_rows of graph.hip (the rows of the fitted graph) and k_ingest_rows of ingest.hip (the rows of new cells
// against a fitted data set).  A wave owns the row; lane p holds entry p.
#pragma once

#include "common.hpp"

namespace srx {

// S(s) of the lane's row: `one` lanes count 1, `far` lanes exp(-x / s), the others nothing.  The butterfly adds in an
// order that does not depend on the lane, so every lane holds the same bits.
__device__ __forceinline__ double graph_S(bool one, bool far, double x, double s) {
    return wave_sum(one ? 1.0 : far ? exp(-x / s) : 0.0);
}

// The root of S(s) = T for a row whose `one` lanes number fewer than T and whose lanes number more (the caller has seen to
// both), in every lane: S rises from the count of `one` lanes (s -> 0) to the count of all lanes (s -> inf).  Bracket by
// factors of two from the largest x, then halve the bracket until it is one ulp wide or S is within 1e-13 of T; the upper
// end of the last bracket is the root.
__device__ __forceinline__ double graph_root(bool one, bool far, double x, double T) {
    double lo = wave_max(x), hi = lo;
    double S = graph_S(one, far, x, lo);
    if (S < T) {
        for (int it = 0; it < 2200; ++it) {
            hi = lo * 2.0;
            if (!(hi <= kDblMax) || graph_S(one, far, x, hi) >= T) break;
            lo = hi;
        }
    } else {
        for (int it = 0; it < 2200; ++it) {
            lo = hi * 0.5;
            if (lo == 0.0 || graph_S(one, far, x, lo) < T) break;
            hi = lo;
        }
    }
    for (int it = 0; it < 128; ++it) {
        const double mid = lo + 0.5 * (hi - lo);
        if (!(mid > lo && mid < hi)) break;
        S = graph_S(one, far, x, mid);
        if (fabs(S - T) <= 1e-13) {
            hi = mid;
            break;
        }
        if (S < T) lo = mid;
        else hi = mid;
    }
    return hi;
}

}  // namespace srx
