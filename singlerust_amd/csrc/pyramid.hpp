// pyramid.hpp — the geometry of the uniform pyramid of include/srx.h (t-SNE, section 3), shared by tsne.hip and draw_graph.hip:
// the first cell of a level, the order-preserving integer keys of the bounds reduction, side and lo from them, the quantised
// coordinate and the Morton spread.  The three passes both files queue unchanged (bounds, the levels above the finest, the
// NaN / Inf check of a start) are host functions defined in tsne.hip, next to their kernels.
#pragma once

#include "common.hpp"

namespace srx {

constexpr unsigned long long kSign = 0x8000000000000000ull;
// the first words of a pyramid's small block (8-byte words): the bounds as integer maxima, cleared before every pyramid
enum { TS_MAX0 = 0, TS_NMIN0, TS_MAX1, TS_NMIN1, TS_BOUNDS_WORDS };

// first cell of level l (1-based) in the concatenated levels, and their total up to L
__host__ __device__ __forceinline__ uint32_t level_off(int l) { return ((1u << (2 * l)) - 4u) / 3u; }

// a finite double as an integer that orders as the double does
__device__ __forceinline__ unsigned long long order_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b & kSign) ? ~b : (b | kSign);
}
__device__ __forceinline__ double order_val(unsigned long long key) {
    return __longlong_as_double((long long)((key & kSign) ? (key ^ kSign) : ~key));
}
__device__ __forceinline__ uint32_t spread_bits(uint32_t x) {      // bit b -> bit 2 b (16 bits in)
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}
__device__ __forceinline__ double2 ts_load(const double* __restrict__ y, uint64_t i) { return reinterpret_cast<const double2*>(y)[i]; }

struct TsGeom {
    double lo0, lo1, side;
};
__device__ __forceinline__ TsGeom ts_geom(const unsigned long long* __restrict__ small) {
    TsGeom g;
    g.lo0 = order_val(~small[TS_NMIN0]);
    g.lo1 = order_val(~small[TS_NMIN1]);
    const double e0 = order_val(small[TS_MAX0]) - g.lo0, e1 = order_val(small[TS_MAX1]) - g.lo1;
    const double ext = e0 > e1 ? e0 : e1;
    g.side = ext == 0.0 ? 1.0 : ext * (1.0 + 0x1p-20);
    return g;
}
__device__ __forceinline__ uint32_t ts_quant(double v, double lo, double side) {
    const double f = floor(((v - lo) / side) * 4294967296.0);
    return (uint32_t)(f < 4294967295.0 ? f : 4294967295.0);
}

// L of the options: `levels`, or from n
int pyramid_levels(uint64_t n, int levels);
// Queued on the context's stream (the caller checks hipGetLastError):
//   the bounds of y (n x 2) into small[TS_MAX0 .. TS_NMIN1], which the caller cleared;
//   levels L - 1 .. 1 of three u64 arrays of concatenated levels from their level L;
//   max |x| over the first two columns of rows x ld, as bits, into *dst (a NaN's bits lie above Inf's).
void pyramid_bounds(srx_ctx* ctx, const double* d_y, uint64_t n, unsigned long long* d_small);
void pyramid_up(srx_ctx* ctx, unsigned long long* d_a, unsigned long long* d_b, unsigned long long* d_c, int L);
void pyramid_absmax(srx_ctx* ctx, const double* d_x, uint64_t rows, uint64_t ld, unsigned long long* d_dst);

}  // namespace srx
