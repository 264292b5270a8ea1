// paga.hip — PAGA: the neighbour graph coarse-grained over the groups (srx_paga, srx_paga_csr, srx_paga_from_counts) and the
// start positions built on it (srx_paga_init_positions).  The definition is in include/srx.h; the design is in DESIGN.md
// ("PAGA").
//
// The device's part is ONE walk over the column indices of the pattern: E[label_i][label_j] += 1 per stored entry.  After a
// clustering a handful of (g, h) pairs take nearly every entry, so a global atomic per entry would queue them all on a few
// addresses.  Instead the ROWS are sorted by label (the counting sort of markers.hip), a workgroup takes kPagaRows sorted rows
// of ONE source group, counts the targets' labels in n_groups 32-bit LDS counters and adds its non-zero counters once to row
// g of the u64 table.  Everything after the walk is arithmetic on the n_groups x n_groups table, on the host, stated once
// (paga_finish) for the two device calls and srx_paga_from_counts.
//
// Kernels:
//   k_paga_check_indices   every column index below n (srx_paga_csr; the handle's D was checked when it was built)
//   k_paga_walk            workgroup = at most kPagaRows label-sorted rows of one group; a group of 2^w lanes per row
//   k_paga_init            one thread per coordinate of the start positions
#include "graph_handle.hpp"
#include "hash.hpp"
#include "markers_internal.hpp"

#include <algorithm>
#include <vector>

// srx.h states the start positions with every operation rounded once
#pragma clang fp contract(off)

namespace srx {

constexpr int kPagaThreads = 256;
constexpr uint64_t kPagaRows = 512;                 // rows per workgroup of the walk (tests/paga_ref.py states the same number)
constexpr uint64_t kPagaMaxRow = 1ull << 22;        // kPagaRows rows of fewer entries than this cannot wrap a 32-bit counter
constexpr unsigned long long kPagaBadIndex = kMkBadLabel << 1;
constexpr uint32_t kPagaNoNeighbour = 0xffffffffu;

__global__ __launch_bounds__(256) void k_paga_check_indices(const uint32_t* __restrict__ ind, uint64_t nnz, uint64_t n,
                                                            unsigned long long* __restrict__ small) {
    bool bad = false;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) bad |= ind[e] >= n;
    if (bad) atomicOr(&small[MK_FLAGS], kPagaBadIndex);
}

// Places [p0, p1) of the permutation, all of group b.group.  The walk is a chain of dependent loads (place -> row -> row
// offsets -> index -> label -> LDS add), so what it costs is latency, and the kernel is arranged to have many loads in flight
// (profiles/paga.md): first every thread fetches the offsets of two of the workgroup's rows into LDS, all at once; then the 256
// threads form groups of 2^wlog lanes (the host picks the power of two at or above the mean row length, 4 .. 64), a lane group
// takes kPagaUnroll rows per round and requests their indices together, then their labels together, then adds.  A k = 15 row
// keeps 15 of 16 lanes busy; what a row holds beyond the lane group's width follows in a plain loop.  (Counting the targets
// inside the row's own group in a register, instead of the one LDS word they all share, was measured and changed nothing.)
// The caller has checked every index against n and every label against n_groups: s_cnt has n_groups entries.
constexpr int kPagaUnroll = 4;
__global__ __launch_bounds__(kPagaThreads) void k_paga_walk(const uint64_t* __restrict__ ptr, const uint32_t* __restrict__ ind,
                                                            const uint32_t* __restrict__ labels, const uint32_t* __restrict__ perm,
                                                            const MkBlock* __restrict__ blocks, uint32_t n_groups, int wlog,
                                                            unsigned long long* __restrict__ E) {
    extern __shared__ uint32_t s_cnt[];
    __shared__ uint64_t s_lo[kPagaRows];
    __shared__ uint32_t s_len[kPagaRows];            // (below 2^22: the caller's check)
    const MkBlock b = blocks[blockIdx.x];
    const uint32_t rows = b.p1 - b.p0;               // (at most kPagaRows: label_blocks)
    for (uint32_t h = threadIdx.x; h < n_groups; h += kPagaThreads) s_cnt[h] = 0u;
    for (uint32_t r = threadIdx.x; r < rows; r += kPagaThreads) {
        const uint32_t row = perm[b.p0 + r];
        const uint64_t lo = ptr[row];
        s_lo[r] = lo;
        s_len[r] = (uint32_t)(ptr[(uint64_t)row + 1] - lo);
    }
    __syncthreads();
    const uint32_t width = 1u << wlog, sub = threadIdx.x & (width - 1u), per_round = (uint32_t)kPagaThreads >> wlog;
    for (uint32_t r0 = threadIdx.x >> wlog; r0 < rows; r0 += per_round * kPagaUnroll) {
        uint32_t j[kPagaUnroll], h[kPagaUnroll];
        bool on[kPagaUnroll];
#pragma unroll
        for (int u = 0; u < kPagaUnroll; ++u) {
            const uint32_t r = r0 + (uint32_t)u * per_round;
            on[u] = r < rows && sub < s_len[r];
            j[u] = on[u] ? ind[s_lo[r] + sub] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kPagaUnroll; ++u) h[u] = on[u] ? labels[j[u]] : 0u;
#pragma unroll
        for (int u = 0; u < kPagaUnroll; ++u)
            if (on[u]) atomicAdd(&s_cnt[h[u]], 1u);
        for (int u = 0; u < kPagaUnroll; ++u) {      // rows longer than the lane group
            const uint32_t r = r0 + (uint32_t)u * per_round;
            if (r >= rows) break;
            const uint64_t lo = s_lo[r];
            for (uint32_t e = sub + width; e < s_len[r]; e += width) atomicAdd(&s_cnt[labels[ind[lo + e]]], 1u);
        }
    }
    __syncthreads();
    unsigned long long* __restrict__ out = E + (uint64_t)b.group * n_groups;
    for (uint32_t h = threadIdx.x; h < n_groups; h += kPagaThreads) {
        const uint32_t c = s_cnt[h];
        if (c) atomicAdd(&out[h], (unsigned long long)c);
    }
}

// out[i][c], t = i * dim + c.  pos: n_groups x dim; nb[g]: the neighbour group of srx.h or kPagaNoNeighbour
__global__ __launch_bounds__(256) void k_paga_init(const uint32_t* __restrict__ labels, const double* __restrict__ pos,
                                                   const uint32_t* __restrict__ nb, uint64_t n, uint32_t n_groups, uint32_t dim,
                                                   uint64_t seed, double* __restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * dim) return;
    const uint64_t i = t / dim;
    const uint32_t c = (uint32_t)(t - i * dim), g = labels[i];
    if (g >= n_groups) return;                       // (refused by the caller before the launch)
    const double pg = pos[(uint64_t)g * dim + c];
    const uint32_t h = nb[g];
    if (h == kPagaNoNeighbour) {
        out[t] = pg;
        return;
    }
    const double dist = pg - pos[(uint64_t)h * dim + c];
    const double u = unit53(mix64(seed + kGold64 * (t + 1)));
    out[t] = (pg - 0.5 * dist) + (u - 0.5) * dist;
}

// ---- everything after the walk, on the host ------------------------------------------------------------------------------------
// E (G x G) and the sizes are consistent: no count in a row or column of an empty group.  Writes whatever of t is not null.
static void paga_finish(const uint64_t* E, const uint64_t* sizes, uint32_t G, srx_paga_tables* t, srx_paga_info* info, double ms) {
    const uint64_t GG = (uint64_t)G * G;
    srx_paga_info pi{};
    pi.n_groups = G;
    pi.ms = ms;
    std::vector<uint64_t> es(G, 0);
    for (uint32_t g = 0; g < G; ++g) {
        pi.n += sizes[g];
        pi.groups_empty += sizes[g] == 0 ? 1u : 0u;
        uint64_t s = 0;
        for (uint32_t h = 0; h < G; ++h) s += E[(uint64_t)g * G + h];
        es[g] = s;
        pi.nnz += s;
        pi.edges_inner += E[(uint64_t)g * G + g];
    }
    pi.edges_inter = pi.nnz - pi.edges_inner;
    double *conn = t ? t->connectivities : nullptr, *expd = t ? t->expected : nullptr, *tree = t ? t->tree : nullptr;
    if (conn) std::fill(conn, conn + GG, 0.0);
    if (expd) std::fill(expd, expd + GG, 0.0);
    if (tree) std::fill(tree, tree + GG, 0.0);
    struct Edge {
        double c;
        uint32_t g, h;
    };
    std::vector<Edge> edges;
    const double n1 = (double)(pi.n - 1);                  // (read only where V > 0, hence N >= 2)
    for (uint32_t g = 0; g < G; ++g)
        for (uint32_t h = g + 1; h < G; ++h) {
            const uint64_t v = E[(uint64_t)g * G + h] + E[(uint64_t)h * G + g];
            if (!v) continue;
            const unsigned __int128 num = (unsigned __int128)es[g] * sizes[h] + (unsigned __int128)es[h] * sizes[g];
            const double ex = (double)num / n1;
            const double r = (double)v / ex;
            const double c = r > 1.0 ? 1.0 : r;
            pi.pairs_connected++;
            pi.pairs_clipped += r > 1.0 ? 1u : 0u;
            if (expd) expd[(uint64_t)g * G + h] = expd[(uint64_t)h * G + g] = ex;
            if (conn) conn[(uint64_t)g * G + h] = conn[(uint64_t)h * G + g] = c;
            if (c > 0.0) edges.push_back(Edge{c, g, h});
        }
    // Kruskal: (conn descending, g ascending, h ascending); the edges were made in (g, h) order, so a stable sort by conn is that
    std::stable_sort(edges.begin(), edges.end(), [](const Edge& a, const Edge& b) { return a.c > b.c; });
    std::vector<uint32_t> root(G);
    for (uint32_t g = 0; g < G; ++g) root[g] = g;
    auto find = [&](uint32_t x) {
        while (root[x] != x) x = root[x] = root[root[x]];
        return x;
    };
    for (const Edge& e : edges) {
        const uint32_t a = find(e.g), b = find(e.h);
        if (a == b) continue;
        root[a > b ? a : b] = a > b ? b : a;
        pi.tree_edges++;
        if (tree) tree[(uint64_t)e.g * G + e.h] = e.c;
    }
    pi.components = G - pi.tree_edges;
    if (t) {
        if (t->sizes && t->sizes != sizes) std::copy(sizes, sizes + G, t->sizes);
        if (t->counts && t->counts != E) std::copy(E, E + GG, t->counts);
        if (t->out_edges) std::copy(es.begin(), es.end(), t->out_edges);
    }
    if (info) *info = pi;
}

static int32_t paga_groups_check(srx_ctx* ctx, const char* what, uint32_t n_groups) {
    if (n_groups < 1 || n_groups > SRX_GROUPS_MAX) return fail(ctx, SRX_E_ARG, "%s: n_groups = %u is outside 1 .. %d", what, n_groups, SRX_GROUPS_MAX);
    return SRX_OK;
}

// The device's part and the hand-off to paga_finish.  ptr / ind: the pattern on the device (n >= 1 rows, nnz entries, no row of
// kPagaMaxRow entries or more); check_ind: compare every index with n first.  d_labels: n u32 on the device, not yet checked.
static int32_t paga_run(srx_ctx* ctx, const uint64_t* d_ptr, const uint32_t* d_ind, uint64_t n, uint64_t nnz, bool check_ind,
                        const uint32_t* d_labels, uint32_t G, srx_paga_tables* t, srx_paga_info* info) {
    Range rg("paga");
    hipStream_t st = ctx->stream;
    const uint64_t GG = (uint64_t)G * G;
    unsigned long long *d_small, *d_E;
    uint64_t* d_sizes;
    SRX_TRY(scratch(ctx, "mk_small", MK_WORDS * 8, (void**)&d_small));
    SRX_TRY(scratch(ctx, "paga_sizes", (size_t)G * 8, (void**)&d_sizes));
    SRX_TRY(scratch(ctx, "paga_counts", GG * 8, (void**)&d_E));
    StreamTimer timer(ctx, st);
    SRX_TRY(timer.start());
    SRX_HIP(ctx, hipMemsetAsync(d_small, 0, MK_WORDS * 8, st));
    SRX_HIP(ctx, hipMemsetAsync(d_E, 0, GG * 8, st));
    LabelSort sort;
    SRX_TRY(label_sort_count(ctx, d_labels, n, G, d_small, d_sizes, &sort));
    if (check_ind && nnz) {
        const unsigned grid = (unsigned)std::min<uint64_t>((nnz + 255) / 256, (uint64_t)ctx->n_cus * 8);
        hipLaunchKernelGGL(k_paga_check_indices, dim3(grid), dim3(256), 0, st, d_ind, nnz, n, d_small);
        SRX_HIP(ctx, hipGetLastError());
    }
    unsigned long long small[MK_WORDS];
    SRX_TRY(d2h(ctx, small, d_small, sizeof small));
    if (small[MK_FLAGS] & kMkBadLabel) return fail(ctx, SRX_E_ARG, "paga: a label is not below n_groups = %u", G);
    if (small[MK_FLAGS] & kPagaBadIndex) return fail(ctx, SRX_E_ARG, "paga: a column index is not below n = %llu", (unsigned long long)n);
    std::vector<uint64_t> sizes(G);
    SRX_TRY(d2h(ctx, sizes.data(), d_sizes, (size_t)G * 8));
    SRX_TRY(label_sort_place(ctx, d_labels, sort));
    const std::vector<MkBlock> blocks = label_blocks(sizes, kPagaRows);
    if (nnz && !blocks.empty()) {
        MkBlock* d_blocks;
        SRX_TRY(scratch(ctx, "mk_blocks", blocks.size() * sizeof(MkBlock), (void**)&d_blocks));
        SRX_TRY(h2d(ctx, d_blocks, blocks.data(), blocks.size() * sizeof(MkBlock)));
        int wlog = 2;                                      // lanes per row: the power of two at or above the mean row length, 4 .. 64
        while (wlog < 6 && (n << wlog) < nnz) ++wlog;
        hipLaunchKernelGGL(k_paga_walk, dim3((unsigned)blocks.size()), dim3(kPagaThreads), (size_t)G * 4, st, d_ptr, d_ind, d_labels,
                           (const uint32_t*)sort.d_perm, (const MkBlock*)d_blocks, G, wlog, d_E);
        SRX_HIP(ctx, hipGetLastError());
    }
    double ms = 0.0;
    SRX_TRY(timer.stop(&ms));
    std::vector<uint64_t> own;
    uint64_t* E = t ? t->counts : nullptr;
    if (!E) {
        own.resize(GG);
        E = own.data();
    }
    SRX_TRY(d2h(ctx, E, d_E, GG * 8));
    paga_finish(E, sizes.data(), G, t, info, ms);
    return SRX_OK;
}

// n == 0: no device work
static void paga_empty(uint32_t G, srx_paga_tables* t, srx_paga_info* info) {
    const std::vector<uint64_t> E((uint64_t)G * G, 0), sizes(G, 0);
    paga_finish(E.data(), sizes.data(), G, t, info, 0.0);
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_paga(srx_graph* g, const uint32_t* labels, uint32_t n_groups, srx_paga_tables* t, srx_paga_info* info) {
    if (!g) return fail(nullptr, SRX_E_ARG, "paga: null graph");
    srx_ctx* ctx = g->ctx;
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "paga: rows are sharded; the labels of a clustering live on one rank");
    SRX_TRY(paga_groups_check(ctx, "paga", n_groups));
    if (!labels && !g->labels_valid) return fail(ctx, SRX_E_ARG, "paga: null labels, and no srx_louvain has run on this graph");
    if (g->n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "paga: 2^32 - 1 rows or more");
    if (!g->n) {
        paga_empty(n_groups, t, info);
        return SRX_OK;
    }
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* d_labels = g->d_labels;
    if (labels) SRX_TRY(host_labels(ctx, g->n, labels, n_groups, "paga", &d_labels));
    return paga_run(ctx, g->d_dptr, g->d_dind, g->n, g->info.nnz_distances, false, d_labels, n_groups, t, info);
}

int32_t srx_paga_csr(srx_ctx* ctx, const uint64_t* indptr, const uint32_t* indices, uint64_t n, const uint32_t* labels, uint32_t n_groups,
                     srx_paga_tables* t, srx_paga_info* info) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "paga: null ctx");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "paga: rows are sharded; the labels of a clustering live on one rank");
    SRX_TRY(paga_groups_check(ctx, "paga", n_groups));
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "paga: 2^32 - 1 rows or more");
    if (indptr && indptr[0] != 0) return fail(ctx, SRX_E_ARG, "paga: indptr[0] is not 0");
    if (!n) {
        paga_empty(n_groups, t, info);
        return SRX_OK;
    }
    if (!indptr) return fail(ctx, SRX_E_ARG, "paga: null indptr");
    if (!labels) return fail(ctx, SRX_E_ARG, "paga: null labels");
    for (uint64_t i = 0; i < n; ++i) {
        if (indptr[i + 1] < indptr[i]) return fail(ctx, SRX_E_ARG, "paga: indptr decreases at row %llu", (unsigned long long)i);
        if (indptr[i + 1] - indptr[i] >= kPagaMaxRow)
            return fail(ctx, SRX_E_ARG, "paga: row %llu holds 2^22 entries or more", (unsigned long long)i);
    }
    const uint64_t nnz = indptr[n];
    if (nnz && !indices) return fail(ctx, SRX_E_ARG, "paga: null indices");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t* d_ptr;
    uint32_t *d_ind, *d_labels;
    SRX_TRY(scratch(ctx, "paga_ptr", (n + 1) * 8, (void**)&d_ptr));
    SRX_TRY(scratch(ctx, "paga_ind", at_least_one(nnz) * 4, (void**)&d_ind));
    SRX_TRY(h2d(ctx, d_ptr, indptr, (n + 1) * 8));
    SRX_TRY(h2d(ctx, d_ind, indices, nnz * 4));
    SRX_TRY(host_labels(ctx, n, labels, n_groups, "paga", &d_labels));
    return paga_run(ctx, d_ptr, d_ind, n, nnz, true, d_labels, n_groups, t, info);
}

int32_t srx_paga_from_counts(const uint64_t* counts, const uint64_t* sizes, uint32_t n_groups, srx_paga_tables* t, srx_paga_info* info) {
    SRX_TRY(paga_groups_check(nullptr, "paga_from_counts", n_groups));
    if (!counts || !sizes) return fail(nullptr, SRX_E_ARG, "paga_from_counts: null counts or sizes");
    const uint64_t G = n_groups;
    for (uint64_t g = 0; g < G; ++g)
        for (uint64_t h = 0; h < G; ++h)
            if (counts[g * G + h] && (!sizes[g] || !sizes[h]))
                return fail(nullptr, SRX_E_ARG, "paga_from_counts: counts[%llu][%llu] is not 0, but group %llu is empty", (unsigned long long)g,
                            (unsigned long long)h, (unsigned long long)(sizes[g] ? h : g));
    paga_finish(counts, sizes, n_groups, t, info, 0.0);
    return SRX_OK;
}

int32_t srx_paga_init_positions(srx_graph* g, srx_ctx* ctx, const uint32_t* labels, uint64_t n, uint32_t n_groups,
                                const double* connectivities, const double* pos, uint32_t dim, uint64_t seed, double* out) {
    if (!ctx && g) ctx = g->ctx;
    if (!ctx) return fail(nullptr, SRX_E_ARG, "paga_init_positions: null graph and null ctx");
    if (g && g->ctx != ctx) return fail(ctx, SRX_E_ARG, "paga_init_positions: the graph belongs to another context");
    if (ctx->n_ranks > 1) return fail(ctx, SRX_E_ARG, "paga_init_positions: rows are sharded; the labels of a clustering live on one rank");
    SRX_TRY(paga_groups_check(ctx, "paga_init_positions", n_groups));
    if (dim != 2 && dim != 3) return fail(ctx, SRX_E_ARG, "paga_init_positions: dim = %u is neither 2 nor 3", dim);
    if (!connectivities || !pos) return fail(ctx, SRX_E_ARG, "paga_init_positions: null connectivities or pos");
    if (g && g->n != n) return fail(ctx, SRX_E_ARG, "paga_init_positions: n = %llu, but the graph has %llu cells", (unsigned long long)n, (unsigned long long)g->n);
    if (n >= 0xFFFFFFFFull) return fail(ctx, SRX_E_ARG, "paga_init_positions: 2^32 - 1 cells or more");
    if (!labels && !(g && g->labels_valid))
        return fail(ctx, SRX_E_ARG, "paga_init_positions: null labels, and no handle that holds those of an srx_louvain");
    if (n && !out) return fail(ctx, SRX_E_ARG, "paga_init_positions: null output");
    const uint64_t G = n_groups;
    for (uint64_t i = 0; i < G * dim; ++i)
        if (!is_finite(pos[i])) return fail(ctx, SRX_E_ARG, "paga_init_positions: pos holds a NaN or Inf");
    for (uint64_t i = 0; i < G * G; ++i)
        if (!is_finite(connectivities[i])) return fail(ctx, SRX_E_ARG, "paga_init_positions: connectivities holds a NaN or Inf");
    if (!n) return SRX_OK;
    std::vector<uint32_t> nb(G, kPagaNoNeighbour);
    for (uint64_t a = 0; a < G; ++a) {
        double best = 0.0;
        for (uint64_t b = 0; b < G; ++b)
            if (connectivities[a * G + b] > best) {
                best = connectivities[a * G + b];
                nb[a] = (uint32_t)b;
            }
    }
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t* d_labels = g ? g->d_labels : nullptr;
    if (labels) SRX_TRY(host_labels(ctx, n, labels, n_groups, "paga_init_positions", &d_labels));
    uint64_t mx = 0;
    SRX_TRY(label_max(ctx, d_labels, n, &mx));
    if (mx >= G) return fail(ctx, SRX_E_ARG, "paga_init_positions: a label is not below n_groups = %u", n_groups);
    double *d_pos, *d_out;
    uint32_t* d_nb;
    SRX_TRY(scratch(ctx, "paga_pos", G * dim * 8, (void**)&d_pos));
    SRX_TRY(scratch(ctx, "paga_nb", G * 4, (void**)&d_nb));
    SRX_TRY(scratch(ctx, "paga_init", n * dim * 8, (void**)&d_out));
    SRX_TRY(h2d(ctx, d_pos, pos, G * dim * 8));
    SRX_TRY(h2d(ctx, d_nb, nb.data(), G * 4));
    hipLaunchKernelGGL(k_paga_init, dim3(grid256(n * dim)), dim3(256), 0, ctx->stream, (const uint32_t*)d_labels, (const double*)d_pos,
                       (const uint32_t*)d_nb, n, n_groups, dim, seed, d_out);
    SRX_HIP(ctx, hipGetLastError());
    return d2h(ctx, out, d_out, n * dim * 8);
}

}  // extern "C"
