// draw_graph.hip — the ForceAtlas2 layout of a symmetric weighted graph in two dimensions on the device: srx_draw_graph (the
// connectivities of an srx_graph, read where they lie), srx_draw_graph_csr (any symmetric CSR), srx_graph_layout_fetch, the
// diagnostic srx_draw_graph_forces and the host-only speed rule srx_fa2_speed.
//
// Definition (include/srx.h has it in full).  An iteration reads Y^{t-1} only: the repulsion is a Barnes-Hut walk over t-SNE's
// uniform pyramid with integer masses (pyramid.hpp), the attraction a sum over the row of W, gravity a term of the vertex; the
// vertex's owner adds the three, one workgroup finishes swing and traction and one of its threads applies the speed rule, an
// apply kernel moves the points.  No host round trip inside an iteration, nothing floating-point is added with an atomic, every
// order of summation is fixed by the cells of the points: the result is the same bits from call to call.
//
// The walk is the one profiles/tsne.md asks for (k_tsne_walk: a thread per point, three dependent loads per cell, divergence):
//   one 32-byte record (com, mass, start | count) per cell, so one load serves a visit;
//   a wave owns 64 points that are consecutive in (finest cell, index) order and walks ONE depth-first path for them: the
//   record of the cell is a wave-uniform load, every lane takes its own accept decision, a ballot says whether any lane needs
//   the children, a lane that accepted is masked for the subtree (open_lvl below), so a lane adds its terms in exactly the
//   order of its own depth-first walk;
//   an opened finest cell is read by the wave together, 64 members at a time into LDS; every lane that opened it loops over
//   the tile.
// Levels 1 .. kFaLdsLevels = 4 of the records are staged in LDS: 340 cells x 32 B = 10.6 KiB, with the member tiles 17 KiB a
// workgroup, which leaves the occupancy to the registers (nine workgroups fit the 160 KiB of a CU).  Every wave visits most of
// these 340 cells; level 5 would add 32 KiB a workgroup, cap a CU at three workgroups and be copied by every workgroup for
// cells of which a wave visits a few (they stay in L2, read with a wave-uniform address).
//
// Kernels:
//   k_fa_mass           m_i = 1 + the row's length
//   k_fa_init_random    the hashed start
//   (k_tsne_bounds, k_tsne_up, k_tsne_absmax of tsne.hip through pyramid.hpp: the bounds, the upper levels, the NaN / Inf check)
//   k_fa_quant          side, lo, the finest cell of every point; member counts, masses and u64 mass-weighted coordinate sums
//                       into the finest level with integer atomics
//   scan_exclusive      (scan.hip) the first point of every finest cell
//   k_fa_cells          (M, SX, SY, start) -> the record of every cell of every level
//   k_fa_scatter, k_fa_rank   the points to their cell through an atomic cursor, then every point finds its place among its
//                       cell's members by counting the smaller indices (the order is (cell, index) whichever atomic won; the
//                       count is bounded by the exact loop the walk runs over the same members); (x, y, m, index) records
//   k_fa_walk           the wave-cooperative walk: rep, the four counters
//   k_fa_force          SRX_FA2_GROUP lanes per vertex: attraction over the row, gravity, F, swing and traction, the
//                       workgroup's mass-weighted sums of both
//   k_fa_speed          one workgroup: S, Tr, then thread 0 applies the speed rule (fa2_speed_rule, shared with the host)
//   k_fa_apply          y += F * factor
// The file is built without -ffast-math and with FMA contraction off: every operation of the definition is rounded once.
#include "common.hpp"
#include "graph_handle.hpp"
#include "hash.hpp"
#include "pyramid.hpp"
#include "scan.hpp"
#include "symcsr.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace srx {

constexpr int kFaGroup = SRX_FA2_GROUP;
constexpr int kFaLdsLevels = 4;
constexpr int kFaLdsCells = ((1 << (2 * (kFaLdsLevels + 1))) - 4) / 3;
constexpr unsigned long long kFaInfBits = 0x7FF0000000000000ull;
// the small block (8-byte words) behind the bounds of pyramid.hpp; the first FA_ZEROED are cleared before every pyramid
enum { FA_ACC = TS_BOUNDS_WORDS, FA_EXACT, FA_PAIRS, FA_COINC, FA_ZEROED, FA_SIDE = FA_ZEROED, FA_LO0, FA_LO1, FA_SPEED, FA_EFF,
       FA_SWING, FA_TRACT, FA_ABSMAX, FA_WORDS = 16 };

struct alignas(32) FaCell {         // a cell of the pyramid: m == 0 says empty; start and count at the finest level only
    double cx, cy, m;
    uint32_t start, count;
};
struct alignas(32) FaPoint {        // a point in (finest cell, index) order
    double x, y, m;
    uint32_t idx, pad_;
};

// Section 7's speed rule, stated once for the device's one thread and for srx_fa2_speed
__host__ __device__ inline void fa2_speed_rule(uint64_t n, double S, double Tr, double jtol, double* speed_io, double* eff_io) {
    double speed = *speed_io, eff = *eff_io;
    const double nn = (double)n;
    const double opt = 0.05 * sqrt(nn);
    const double a = sqrt(opt);
    double b = (opt * Tr) / (nn * nn);
    b = b < 10.0 ? b : 10.0;
    double jt = jtol * (a > b ? a : b);
    if (Tr > 0.0 && S / Tr > 2.0) {
        if (eff > 0.05) eff = eff * 0.5;
        jt = jt > jtol ? jt : jtol;
    }
    const double target = S == 0.0 ? (double)__builtin_inff() : ((jt * eff) * Tr) / S;
    if (S > jt * Tr) {
        if (eff > 0.05) eff = eff * 0.7;
    } else if (speed < 1000.0) {
        eff = eff * 1.3;
    }
    const double rise = target - speed, cap = 0.5 * speed;
    speed = speed + (rise < cap ? rise : cap);
    *speed_io = speed;
    *eff_io = eff;
}

__global__ void __launch_bounds__(256) k_fa_mass(const uint64_t* __restrict__ ptr, uint64_t n, uint32_t* __restrict__ mass) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) mass[i] = 1u + (uint32_t)(ptr[i + 1] - ptr[i]);
}

__global__ void __launch_bounds__(256) k_fa_init_random(double* __restrict__ y, uint64_t count, uint64_t seed) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= count) return;
    y[c] = unit53(mix64(seed + kGold64 * (c + 1)));
}

// ---- the pyramid -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_fa_quant(const double* __restrict__ y, const uint32_t* __restrict__ mass, uint64_t n, int L,
                                                  unsigned long long* __restrict__ small, long long* __restrict__ cnt,
                                                  unsigned long long* __restrict__ cm, unsigned long long* __restrict__ sx,
                                                  unsigned long long* __restrict__ sy, uint32_t* __restrict__ code_out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const TsGeom g = ts_geom(small);
    if (i == 0) {
        small[FA_SIDE] = (unsigned long long)__double_as_longlong(g.side);
        small[FA_LO0] = (unsigned long long)__double_as_longlong(g.lo0);
        small[FA_LO1] = (unsigned long long)__double_as_longlong(g.lo1);
    }
    if (i >= n) return;
    const double2 p = ts_load(y, i);
    const uint32_t u0 = ts_quant(p.x, g.lo0, g.side), u1 = ts_quant(p.y, g.lo1, g.side);
    const uint32_t code = spread_bits(u0 >> (32 - L)) | (spread_bits(u1 >> (32 - L)) << 1);
    code_out[i] = code;
    const unsigned long long m = mass[i];
    const size_t c = (size_t)level_off(L) + code;
    atomicAdd(reinterpret_cast<unsigned long long*>(&cnt[code]), 1ull);
    atomicAdd(&cm[c], m);
    atomicAdd(&sx[c], m * u0);                      // below 2^64: M_tot < 2^32
    atomicAdd(&sy[c], m * u1);
}

__global__ void __launch_bounds__(256) k_fa_cells(const unsigned long long* __restrict__ cm, const unsigned long long* __restrict__ sx,
                                                  const unsigned long long* __restrict__ sy, uint32_t total, int L,
                                                  const unsigned long long* __restrict__ small, const int64_t* __restrict__ start,
                                                  FaCell* __restrict__ cells) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= total) return;
    const unsigned long long m = cm[c];
    FaCell r{0.0, 0.0, (double)m, 0u, 0u};
    if (m) {
        const double unit = __longlong_as_double((long long)small[FA_SIDE]) * 0x1p-32;
        r.cx = __longlong_as_double((long long)small[FA_LO0]) + ((double)sx[c] / (double)m) * unit;
        r.cy = __longlong_as_double((long long)small[FA_LO1]) + ((double)sy[c] / (double)m) * unit;
        const uint32_t first = level_off(L);
        if (c >= first) {
            r.start = (uint32_t)start[c - first];
            r.count = (uint32_t)(start[c - first + 1] - start[c - first]);
        }
    }
    cells[c] = r;
}

__global__ void __launch_bounds__(256) k_fa_scatter(const uint32_t* __restrict__ code, uint64_t n, const int64_t* __restrict__ start,
                                                    uint32_t* __restrict__ cursor, uint32_t* __restrict__ tmp) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = code[i];
    tmp[start[c] + (int64_t)atomicAdd(&cursor[c], 1u)] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_fa_rank(const uint32_t* __restrict__ code, uint64_t n, const int64_t* __restrict__ start,
                                                 const uint32_t* __restrict__ tmp, const double* __restrict__ y,
                                                 const uint32_t* __restrict__ mass, FaPoint* __restrict__ pts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t c = code[i];
    const int64_t lo = start[c], hi = start[c + 1];
    int64_t r = 0;
    for (int64_t q = lo; q < hi; ++q) r += tmp[q] < (uint32_t)i;       // the members are distinct: the ranks are a permutation
    const double2 p = ts_load(y, i);
    pts[lo + r] = FaPoint{p.x, p.y, (double)mass[i], (uint32_t)i, 0u};
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------------
// open_lvl of a lane: the number of cells on the wave's current path, from level 1 down, that the lane itself opened.  At a
// cell of level l it is first cut to l - 1 (what it says about a sibling or a deeper branch the wave has left is stale); the
// lane then stands at this cell in its own walk exactly when open_lvl == l - 1.  A lane behind the data holds -1.
__global__ void __launch_bounds__(256) k_fa_walk(const FaPoint* __restrict__ pts, uint64_t n, int L, double theta2, double kr,
                                                 const FaCell* __restrict__ cells, unsigned long long* __restrict__ small,
                                                 double* __restrict__ rep) {
    __shared__ FaCell s_cell[kFaLdsCells];
    __shared__ double s_tx[4][kWave], s_ty[4][kWave], s_tm[4][kWave];
    __shared__ unsigned long long s_ctr[4];
    const int Ls = L < kFaLdsLevels ? L : kFaLdsLevels;
    const int staged = (int)level_off(Ls + 1);
    for (int t = threadIdx.x; t < staged; t += 256) s_cell[t] = cells[t];
    __syncthreads();
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const uint64_t first = ((uint64_t)blockIdx.x * 4 + (uint32_t)wave) * kWave;       // wave-uniform
    const uint64_t t = first + lane;
    const bool live = t < n;
    unsigned long long n_acc = 0, n_exact = 0, n_pairs = 0, n_coinc = 0;
    if (first < n) {
        const FaPoint me = live ? pts[t] : FaPoint{0.0, 0.0, 0.0, 0u, 0u};
        const double side = __longlong_as_double((long long)small[FA_SIDE]);
        double r0 = 0.0, r1 = 0.0;
        int open_lvl = live ? 0 : -1;
        int l = 1;
        uint32_t code = 0;
        while (l > 0) {
            const uint32_t at = level_off(l) + code;
            const FaCell c = l <= Ls ? s_cell[at] : cells[at];
            if (c.m > 0.0) {
                open_lvl = open_lvl < l - 1 ? open_lvl : l - 1;
                const bool here = open_lvl == l - 1;
                const double d0 = me.x - c.cx, d1 = me.y - c.cy;
                const double d2 = d0 * d0 + d1 * d1;
                const double sl = side * __longlong_as_double((long long)(1023 - l) << 52);
                const bool acc = sl * sl < theta2 * d2;
                if (here && acc) {
                    const double f = (kr * (me.m * c.m)) / d2;
                    r0 += f * d0;
                    r1 += f * d1;
                    ++n_acc;
                }
                const bool opens = here && !acc;
                if (__builtin_amdgcn_ballot_w64(opens)) {
                    if (l < L) {
                        if (opens) open_lvl = l;
                        ++l;
                        code <<= 2;
                        continue;
                    }
                    if (opens) ++n_exact;
                    for (uint32_t base = 0; base < c.count; base += kWave) {
                        const uint32_t left = c.count - base, cnt = left < (uint32_t)kWave ? left : (uint32_t)kWave;
                        const uint64_t s0 = (uint64_t)c.start + base;
                        wave_lds_sync();                                  // the tile before this one has been read
                        if ((uint32_t)lane < cnt && s0 + lane < n) {
                            const FaPoint p = pts[s0 + lane];
                            s_tx[wave][lane] = p.x;
                            s_ty[wave][lane] = p.y;
                            s_tm[wave][lane] = p.m;
                        }
                        wave_lds_sync();
                        if (opens) {
                            for (uint32_t j = 0; j < cnt; ++j) {          // ascending index: the sorted order within a cell
                                if (s0 + j == t) continue;
                                const double e0 = me.x - s_tx[wave][j], e1 = me.y - s_ty[wave][j];
                                const double e2 = e0 * e0 + e1 * e1;
                                ++n_pairs;
                                if (e2 > 0.0) {
                                    const double f = (kr * (me.m * s_tm[wave][j])) / e2;
                                    r0 += f * e0;
                                    r1 += f * e1;
                                } else {
                                    ++n_coinc;
                                }
                            }
                        }
                    }
                }
            }
            // on to the next cell: the next sibling, or the parent's once the four children are done
            ++code;
            while ((code & 3u) == 0u && l > 0) {
                code >>= 2;
                --l;
            }
        }
        if (live) reinterpret_cast<double2*>(rep)[me.idx] = make_double2(r0, r1);
    }
    n_acc = block_sum_thread0<4>(n_acc, s_ctr);
    if (n_acc) atomicAdd(&small[FA_ACC], n_acc);
    __syncthreads();
    n_exact = block_sum_thread0<4>(n_exact, s_ctr);
    if (n_exact) atomicAdd(&small[FA_EXACT], n_exact);
    __syncthreads();
    n_pairs = block_sum_thread0<4>(n_pairs, s_ctr);
    if (n_pairs) atomicAdd(&small[FA_PAIRS], n_pairs);
    __syncthreads();
    n_coinc = block_sum_thread0<4>(n_coinc, s_ctr);
    if (n_coinc) atomicAdd(&small[FA_COINC], n_coinc);
}

// ---- attraction, gravity, the sums, the step ---------------------------------------------------------------------------------------
struct FaForce {
    double gravity;
    int strong, linlog;
};

__device__ __forceinline__ double fa_norm(double a, double b) { return sqrt(a * a + b * b); }

// attr_out: the diagnostic (attr and grav alone are written); else the iteration (F, swing and the workgroup's sums)
__global__ void __launch_bounds__(256) k_fa_force(SymCsr g, const double* __restrict__ y, const uint32_t* __restrict__ mass,
                                                  const double* __restrict__ rep, FaForce p, const double* __restrict__ fprev,
                                                  double* __restrict__ fout, double* __restrict__ swing_out,
                                                  double* __restrict__ spart, double* __restrict__ tpart,
                                                  double* __restrict__ grav_out, double* __restrict__ attr_out) {
    constexpr int G = kFaGroup;
    __shared__ double s_wave[4];
    const uint64_t row = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int sub = threadIdx.x & (G - 1);
    const bool live = row < g.n;
    double a0 = 0.0, a1 = 0.0;
    double2 yi = make_double2(0.0, 0.0);
    if (live) {
        yi = ts_load(y, row);
        const uint64_t lo = g.ptr[row], hi = g.ptr[row + 1];
        for (uint64_t e = lo + sub; e < hi; e += G) {
            const double2 yj = ts_load(y, g.ind[e]);
            const double e0 = yi.x - yj.x, e1 = yi.y - yj.y;
            double f = g.w[e];
            if (p.linlog) {
                const double d = sqrt(e0 * e0 + e1 * e1);
                f = d > 0.0 ? f * (log1p(d) / d) : 0.0;
            }
            a0 += f * e0;
            a1 += f * e1;
        }
    }
    // every lane of the block is here: the butterflies read all of them
    a0 = -group_sum<G>(a0);
    a1 = -group_sum<G>(a1);
    const bool owner = live && sub == 0;
    double ms = 0.0, mt = 0.0;
    if (owner) {
        const double m = (double)mass[row];
        const double r = fa_norm(yi.x, yi.y);
        double g0 = 0.0, g1 = 0.0;
        if (r != 0.0) {
            const double c = p.strong ? p.gravity * m : (p.gravity * m) / r;
            g0 = -(c * yi.x);
            g1 = -(c * yi.y);
        }
        if (attr_out) {
            reinterpret_cast<double2*>(attr_out)[row] = make_double2(a0, a1);
            reinterpret_cast<double2*>(grav_out)[row] = make_double2(g0, g1);
        } else {
            const double2 rp = ts_load(rep, row), fp = ts_load(fprev, row);
            const double f0 = (rp.x + g0) + a0, f1 = (rp.y + g1) + a1;
            const double swing = fa_norm(fp.x - f0, fp.y - f1), tract = 0.5 * fa_norm(fp.x + f0, fp.y + f1);
            reinterpret_cast<double2*>(fout)[row] = make_double2(f0, f1);
            swing_out[row] = swing;
            ms = m * swing;
            mt = m * tract;
        }
    }
    if (attr_out) return;                            // the same for every thread of the launch
    ms = block_sum<4>(ms, s_wave);
    mt = block_sum<4>(mt, s_wave);
    if (threadIdx.x == 0) {
        spart[blockIdx.x] = ms;
        tpart[blockIdx.x] = mt;
    }
}

// S and Tr by ONE workgroup: thread u chains part[u], part[u + 256], ..., then the workgroup sum; thread 0 applies the rule
__global__ void __launch_bounds__(256) k_fa_speed(const double* __restrict__ spart, const double* __restrict__ tpart, uint64_t nb,
                                                  uint64_t n, double jtol, unsigned long long* __restrict__ small) {
    __shared__ double s_wave[4];
    double s = 0.0, t = 0.0;
    for (uint64_t b = threadIdx.x; b < nb; b += 256) {
        s += spart[b];
        t += tpart[b];
    }
    s = block_sum<4>(s, s_wave);
    t = block_sum<4>(t, s_wave);
    if (threadIdx.x != 0) return;
    double speed = __longlong_as_double((long long)small[FA_SPEED]), eff = __longlong_as_double((long long)small[FA_EFF]);
    fa2_speed_rule(n, s, t, jtol, &speed, &eff);
    small[FA_SPEED] = (unsigned long long)__double_as_longlong(speed);
    small[FA_EFF] = (unsigned long long)__double_as_longlong(eff);
    small[FA_SWING] = (unsigned long long)__double_as_longlong(s);
    small[FA_TRACT] = (unsigned long long)__double_as_longlong(t);
}

__global__ void __launch_bounds__(256) k_fa_apply(double* __restrict__ y, const double* __restrict__ f, const double* __restrict__ swing,
                                                  const uint32_t* __restrict__ mass, uint64_t n,
                                                  const unsigned long long* __restrict__ small) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double speed = __longlong_as_double((long long)small[FA_SPEED]);
    const double factor = speed / (1.0 + sqrt(speed * ((double)mass[i] * swing[i])));
    const double2 yi = ts_load(y, i), fi = ts_load(f, i);
    reinterpret_cast<double2*>(y)[i] = make_double2(yi.x + fi.x * factor, yi.y + fi.y * factor);
}

// ---- host side ---------------------------------------------------------------------------------------------------------
// the buffers of a force evaluation at n points and L levels
struct FaWork {
    int L = 0;
    uint32_t total = 0, finest = 0;        // cells of all levels, of level L
    unsigned long long *d_small = nullptr, *d_cm = nullptr, *d_sx = nullptr, *d_sy = nullptr;
    long long* d_cnt = nullptr;             // members of the finest cells
    uint32_t *d_cursor = nullptr, *d_code = nullptr, *d_tmp = nullptr, *d_mass = nullptr;
    size_t zero_bytes = 0;                  // d_cm .. d_cursor are one block, cleared together
    FaCell* d_cells = nullptr;
    FaPoint* d_pts = nullptr;
    int64_t* d_start = nullptr;
    double* d_rep = nullptr;
};

static int32_t fa_work(srx_ctx* ctx, uint64_t n, int L, FaWork* w) {
    w->L = L;
    w->total = level_off(L + 1);
    w->finest = 1u << (2 * L);
    const size_t ints = up256((size_t)w->total * 8), fin = up256((size_t)w->finest * 8);
    w->zero_bytes = 3 * ints + fin + up256((size_t)w->finest * 4);
    char* p;
    SRX_TRY(scratch(ctx, "fa2_pyramid", w->zero_bytes, (void**)&p));
    w->d_cm = (unsigned long long*)p;
    w->d_sx = (unsigned long long*)(p + ints);
    w->d_sy = (unsigned long long*)(p + 2 * ints);
    w->d_cnt = (long long*)(p + 3 * ints);
    w->d_cursor = (uint32_t*)(p + 3 * ints + fin);
    SRX_TRY(scratch(ctx, "fa2_cells", (size_t)w->total * sizeof(FaCell), (void**)&w->d_cells));
    SRX_TRY(scratch(ctx, "fa2_small", FA_WORDS * 8, (void**)&w->d_small));
    SRX_TRY(scratch(ctx, "fa2_start", ((size_t)w->finest + 1) * 8, (void**)&w->d_start));
    const size_t n1 = at_least_one(n);
    SRX_TRY(scratch(ctx, "fa2_code", 3 * up256(n1 * 4), (void**)&p));
    w->d_code = (uint32_t*)p;
    w->d_tmp = (uint32_t*)(p + up256(n1 * 4));
    w->d_mass = (uint32_t*)(p + 2 * up256(n1 * 4));
    SRX_TRY(scratch(ctx, "fa2_pts", n1 * sizeof(FaPoint), (void**)&w->d_pts));
    SRX_TRY(scratch(ctx, "fa2_rep", n1 * 16, (void**)&w->d_rep));
    return SRX_OK;
}

// rep at d_y, queued on the context's stream; n >= 1, the masses are in w.d_mass
static int32_t fa_repulsion(srx_ctx* ctx, const FaWork& w, const double* d_y, uint64_t n, double theta, double kr) {
    hipStream_t st = ctx->stream;
    const unsigned pts = grid256(n);
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, FA_ZEROED * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(w.d_cm, 0, w.zero_bytes, st));
    pyramid_bounds(ctx, d_y, n, w.d_small);
    hipLaunchKernelGGL(k_fa_quant, dim3(pts), dim3(256), 0, st, d_y, w.d_mass, n, w.L, w.d_small, w.d_cnt, w.d_cm, w.d_sx, w.d_sy, w.d_code);
    pyramid_up(ctx, w.d_cm, w.d_sx, w.d_sy, w.L);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(scan_exclusive(ctx, reinterpret_cast<const int64_t*>(w.d_cnt), w.finest, w.d_start, nullptr));
    hipLaunchKernelGGL(k_fa_cells, dim3(grid256(w.total)), dim3(256), 0, st, w.d_cm, w.d_sx, w.d_sy, w.total, w.L, w.d_small, w.d_start,
                       w.d_cells);
    hipLaunchKernelGGL(k_fa_scatter, dim3(pts), dim3(256), 0, st, w.d_code, n, w.d_start, w.d_cursor, w.d_tmp);
    hipLaunchKernelGGL(k_fa_rank, dim3(pts), dim3(256), 0, st, w.d_code, n, w.d_start, w.d_tmp, d_y, w.d_mass, w.d_pts);
    hipLaunchKernelGGL(k_fa_walk, dim3(pts), dim3(256), 0, st, w.d_pts, n, w.L, theta * theta, kr, w.d_cells, w.d_small, w.d_rep);
    SRX_HIP(ctx, hipGetLastError());
    return SRX_OK;
}

struct FaOpts {
    srx_fa2_opts o;
    uint32_t iters, run;
    int L;
};

static int32_t fa_check_param(srx_ctx* ctx, const char* name, double v) {
    if (!(v >= 0.0 && v <= kDblMax)) return fail(ctx, SRX_E_ARG, "draw_graph: %s must be a finite number >= 0", name);
    return SRX_OK;
}

static int32_t fa_opts(srx_ctx* ctx, const srx_fa2_opts* in, uint64_t n, FaOpts* out) {
    srx_fa2_opts o = in ? *in : srx_fa2_opts{1.2, 2.0, 1.0, 1.0, 0, 500, 0, 0, SRX_FA2_INIT_RANDOM, 0, 0};
    SRX_TRY(fa_check_param(ctx, "theta", o.theta));
    SRX_TRY(fa_check_param(ctx, "scaling_ratio", o.scaling_ratio));
    SRX_TRY(fa_check_param(ctx, "gravity", o.gravity));
    SRX_TRY(fa_check_param(ctx, "jitter_tolerance", o.jitter_tolerance));
    if (o.levels < 0 || o.levels > SRX_TSNE_MAX_LEVELS)
        return fail(ctx, SRX_E_ARG, "draw_graph: levels = %d outside 0..%d", o.levels, SRX_TSNE_MAX_LEVELS);
    if (o.n_iter < 0 || o.n_iter > SRX_FA2_MAX_ITERS) return fail(ctx, SRX_E_ARG, "draw_graph: n_iter = %d outside 0..%d", o.n_iter, SRX_FA2_MAX_ITERS);
    if (o.n_iter == 0) o.n_iter = 500;
    if (o.stop_after < 0 || o.stop_after > o.n_iter)
        return fail(ctx, SRX_E_ARG, "draw_graph: stop_after = %d outside 0..n_iter = %d", o.stop_after, o.n_iter);
    if (o.init != SRX_FA2_INIT_GIVEN && o.init != SRX_FA2_INIT_RANDOM) return fail(ctx, SRX_E_ARG, "draw_graph: unknown start %d", o.init);
    out->o = o;
    out->iters = (uint32_t)o.n_iter;
    out->run = (uint32_t)(o.stop_after ? o.stop_after : o.n_iter);
    out->L = pyramid_levels(n, o.levels);
    return SRX_OK;
}

static int32_t fa_check_mass(srx_ctx* ctx, uint64_t n, uint64_t nnz) {
    if (n >= (1ull << 32) || nnz >= (1ull << 32) || n + nnz >= (1ull << 32))
        return fail(ctx, SRX_E_ARG, "draw_graph: the total mass n + nnz = %llu is not below 2^32", (unsigned long long)(n + nnz));
    return SRX_OK;
}

static void fa_info_start(srx_fa2_info* li, const FaOpts& u, uint64_t n, uint64_t nnz) {
    *li = srx_fa2_info{};
    li->n = n;
    li->nnz = nnz;
    li->total_mass = n + nnz;
    li->n_iter = u.iters;
    li->levels = (uint32_t)u.L;
    li->speed = 1.0;
    li->speed_efficiency = 1.0;
}

static double bits_f64(uint64_t b) {
    double v;
    memcpy(&v, &b, 8);
    return v;
}

// The run (n >= 1) on a graph that is on the device.  The result is left in *d_result (a scratch buffer).
static int32_t fa_run(srx_ctx* ctx, const SymCsr& g, const FaOpts& u, const double* init, double** d_result, srx_fa2_info* info) {
    hipStream_t st = ctx->stream;
    const uint64_t n = g.n, count = n * 2;
    FaWork w;
    SRX_TRY(fa_work(ctx, n, u.L, &w));
    const unsigned blocks = grid256(n * (uint64_t)kFaGroup);
    double *d_y, *d_f0, *d_f1, *d_swing, *d_part;
    SRX_TRY(scratch(ctx, "fa2_y", count * 8, (void**)&d_y));
    SRX_TRY(scratch(ctx, "fa2_f0", count * 8, (void**)&d_f0));
    SRX_TRY(scratch(ctx, "fa2_f1", count * 8, (void**)&d_f1));
    SRX_TRY(scratch(ctx, "fa2_swing", n * 8, (void**)&d_swing));
    SRX_TRY(scratch(ctx, "fa2_part", (size_t)blocks * 16, (void**)&d_part));
    if (u.o.init == SRX_FA2_INIT_GIVEN) SRX_TRY(h2d(ctx, d_y, init, count * 8));

    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, FA_WORDS * 8, st));
    if (u.o.init == SRX_FA2_INIT_RANDOM)
        hipLaunchKernelGGL(k_fa_init_random, dim3(grid256(count)), dim3(256), 0, st, d_y, count, u.o.seed);
    pyramid_absmax(ctx, d_y, n, 2, w.d_small + FA_ABSMAX);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t hs[FA_WORDS];
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (hs[FA_ABSMAX] >= kFaInfBits) return fail(ctx, SRX_E_ARG, "draw_graph: the start positions hold a NaN or Inf");
    const double one = 1.0;
    memcpy(&hs[FA_SPEED], &one, 8);
    memcpy(&hs[FA_EFF], &one, 8);
    SRX_TRY(h2d(ctx, w.d_small, hs, sizeof hs));
    hipLaunchKernelGGL(k_fa_mass, dim3(grid256(n)), dim3(256), 0, st, g.ptr, n, w.d_mass);
    SRX_HIP(ctx, hipMemsetAsync(d_f0, 0, count * 8, st));                   // Fprev = 0
    double *fprev = d_f0, *fcur = d_f1;
    const FaForce fp{u.o.gravity, u.o.strong_gravity != 0, u.o.linlog != 0};
    for (uint32_t t = 1; t <= u.run; ++t) {
        SRX_TRY(fa_repulsion(ctx, w, d_y, n, u.o.theta, u.o.scaling_ratio));
        hipLaunchKernelGGL(k_fa_force, dim3(blocks), dim3(256), 0, st, g, d_y, w.d_mass, w.d_rep, fp, fprev, fcur, d_swing, d_part,
                           d_part + blocks, (double*)nullptr, (double*)nullptr);
        hipLaunchKernelGGL(k_fa_speed, dim3(1), dim3(256), 0, st, d_part, d_part + blocks, (uint64_t)blocks, n, u.o.jitter_tolerance,
                           w.d_small);
        hipLaunchKernelGGL(k_fa_apply, dim3(grid256(n)), dim3(256), 0, st, d_y, fcur, d_swing, w.d_mass, n, w.d_small);
        std::swap(fprev, fcur);
    }
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(timer.stop(&info->ms));
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    info->iters_run = u.run;
    if (u.run) {
        info->speed = bits_f64(hs[FA_SPEED]);
        info->speed_efficiency = bits_f64(hs[FA_EFF]);
        info->swing = bits_f64(hs[FA_SWING]);
        info->traction = bits_f64(hs[FA_TRACT]);
        info->side = bits_f64(hs[FA_SIDE]);
        info->cells_accepted = hs[FA_ACC];
        info->cells_exact = hs[FA_EXACT];
        info->pairs_exact = hs[FA_PAIRS];
        info->pairs_coincident = hs[FA_COINC];
    }
    *d_result = d_y;
    return SRX_OK;
}

static int32_t fa_check_start(srx_ctx* ctx, const FaOpts& u, const double* init, uint64_t n) {
    if (u.o.init == SRX_FA2_INIT_GIVEN && !init && n) return fail(ctx, SRX_E_ARG, "draw_graph: SRX_FA2_INIT_GIVEN needs start positions");
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_draw_graph(srx_graph* g, const srx_fa2_opts* opts, const double* init, double* layout_out, srx_fa2_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "draw_graph: rows are sharded; the layout needs the whole graph");
    FaOpts u;
    SRX_TRY(fa_opts(ctx, opts, g->n, &u));
    SRX_TRY(fa_check_start(ctx, u, init, g->n));
    const SymCsr c = connectivities(g);
    SRX_TRY(fa_check_mass(ctx, c.n, c.nnz));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_fa2_info li;
    fa_info_start(&li, u, c.n, c.nnz);
    if (g->n) {
        Range rg("draw_graph");
        double* d_res = nullptr;
        SRX_TRY(fa_run(ctx, c, u, init, &d_res, &li));
        g->layout_valid = false;
        SRX_TRY(keep_on_handle(ctx, &g->d_layout, false, d_res, (size_t)g->n * 16));
        if (layout_out) SRX_TRY(d2h(ctx, layout_out, g->d_layout, (size_t)g->n * 16));
    }
    g->layout_valid = true;
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_draw_graph_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                           const srx_fa2_opts* opts, const double* init, double* layout_out, srx_fa2_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "draw_graph: rows are sharded; the layout needs the whole graph");
    FaOpts u;
    SRX_TRY(fa_opts(ctx, opts, n, &u));
    SRX_TRY(fa_check_start(ctx, u, init, n));
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_fa2_info li;
    fa_info_start(&li, u, n, 0);
    if (n == 0) {
        if (info) *info = li;
        return SRX_OK;
    }
    if (!indptr) return fail(ctx, SRX_E_ARG, "draw_graph: null indptr");
    SRX_TRY(fa_check_mass(ctx, n, indptr[n]));              // before anything of that size is allocated or copied
    Range rg("draw_graph");
    SymCsr in;
    SRX_TRY(symcsr_to_device(ctx, "draw_graph", indptr, indices, weights, n, &in));
    fa_info_start(&li, u, in.n, in.nnz);
    double* d_res = nullptr;
    SRX_TRY(fa_run(ctx, in, u, init, &d_res, &li));
    if (layout_out) SRX_TRY(d2h(ctx, layout_out, d_res, (size_t)n * 16));
    if (info) *info = li;
    return SRX_OK;
}

int32_t srx_graph_layout_fetch(srx_graph* g, double* out) {
    if (!g) return fail(nullptr, SRX_E_ARG, "null graph");
    srx_ctx* ctx = g->ctx;
    if (!g->layout_valid) return fail(ctx, SRX_E_ARG, "srx_graph_layout_fetch: no srx_draw_graph has run on this graph");
    if (!g->n || !out) return SRX_OK;
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    return d2h(ctx, out, g->d_layout, (size_t)g->n * 16);
}

int32_t srx_draw_graph_forces(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, const double* weights, uint64_t n,
                              const double* Y, const srx_fa2_opts* opts, double* rep_out, double* grav_out, double* attr_out,
                              uint32_t* mass_out, srx_fa2_force_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "draw_graph: rows are sharded; the forces need the whole graph");
    FaOpts u;
    SRX_TRY(fa_opts(ctx, opts, n, &u));
    srx_fa2_force_info fi{};
    fi.levels = (uint32_t)u.L;
    if (n == 0) {
        if (info) *info = fi;
        return SRX_OK;
    }
    if (!Y) return fail(ctx, SRX_E_ARG, "draw_graph: null positions");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    if (!indptr) return fail(ctx, SRX_E_ARG, "draw_graph: null indptr");
    SRX_TRY(fa_check_mass(ctx, n, indptr[n]));
    Range rg("draw_graph_forces");
    SymCsr in;
    SRX_TRY(symcsr_to_device(ctx, "draw_graph", indptr, indices, weights, n, &in));
    fi.total_mass = in.n + in.nnz;
    FaWork w;
    SRX_TRY(fa_work(ctx, n, u.L, &w));
    double *d_y, *d_grav, *d_attr;
    SRX_TRY(scratch(ctx, "fa2_y", n * 16, (void**)&d_y));
    SRX_TRY(scratch(ctx, "fa2_f0", n * 16, (void**)&d_grav));
    SRX_TRY(scratch(ctx, "fa2_f1", n * 16, (void**)&d_attr));
    SRX_TRY(h2d(ctx, d_y, Y, n * 16));
    hipStream_t st = ctx->stream;
    SRX_HIP(ctx, hipMemsetAsync(w.d_small, 0, FA_WORDS * 8, st));
    pyramid_absmax(ctx, d_y, n, 2, w.d_small + FA_ABSMAX);
    SRX_HIP(ctx, hipGetLastError());
    uint64_t hs[FA_WORDS];
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (hs[FA_ABSMAX] >= kFaInfBits) return fail(ctx, SRX_E_ARG, "draw_graph: the positions hold a NaN or Inf");
    hipLaunchKernelGGL(k_fa_mass, dim3(grid256(n)), dim3(256), 0, st, in.ptr, n, w.d_mass);
    SRX_TRY(fa_repulsion(ctx, w, d_y, n, u.o.theta, u.o.scaling_ratio));
    hipLaunchKernelGGL(k_fa_force, dim3(grid256(n * (uint64_t)kFaGroup)), dim3(256), 0, st, in, d_y, w.d_mass, w.d_rep,
                       FaForce{u.o.gravity, u.o.strong_gravity != 0, u.o.linlog != 0}, (const double*)nullptr, (double*)nullptr,
                       (double*)nullptr, (double*)nullptr, (double*)nullptr, d_grav, d_attr);
    SRX_HIP(ctx, hipGetLastError());
    SRX_TRY(d2h(ctx, hs, w.d_small, sizeof hs));
    if (rep_out) SRX_TRY(d2h(ctx, rep_out, w.d_rep, n * 16));
    if (grav_out) SRX_TRY(d2h(ctx, grav_out, d_grav, n * 16));
    if (attr_out) SRX_TRY(d2h(ctx, attr_out, d_attr, n * 16));
    if (mass_out) SRX_TRY(d2h(ctx, mass_out, w.d_mass, n * 4));
    fi.side = bits_f64(hs[FA_SIDE]);
    fi.lo[0] = bits_f64(hs[FA_LO0]);
    fi.lo[1] = bits_f64(hs[FA_LO1]);
    fi.cells_accepted = hs[FA_ACC];
    fi.cells_exact = hs[FA_EXACT];
    fi.pairs_exact = hs[FA_PAIRS];
    fi.pairs_coincident = hs[FA_COINC];
    if (info) *info = fi;
    return SRX_OK;
}

int32_t srx_fa2_speed(uint64_t n, double S, double Tr, double jitter_tolerance, double* speed, double* eff) {
    if (!speed || !eff) return fail(nullptr, SRX_E_ARG, "fa2_speed: null output");
    if (n == 0) return fail(nullptr, SRX_E_ARG, "fa2_speed: n must be at least 1");
    if (!(S >= 0.0 && S <= kDblMax) || !(Tr >= 0.0 && Tr <= kDblMax)) return fail(nullptr, SRX_E_ARG, "fa2_speed: S and Tr must be finite numbers >= 0");
    if (!(jitter_tolerance >= 0.0 && jitter_tolerance <= kDblMax)) return fail(nullptr, SRX_E_ARG, "fa2_speed: jitter_tolerance must be a finite number >= 0");
    if (!(*speed >= 0.0) || !(*eff >= 0.0)) return fail(nullptr, SRX_E_ARG, "fa2_speed: speed and eff must be numbers >= 0");
    fa2_speed_rule(n, S, Tr, jitter_tolerance, speed, eff);
    return SRX_OK;
}

}  // extern "C"
