// markers_internal.hpp — what markers.hip (grouped moments, Welch's t, the rank sums) and hvg_seurat.hip (the Seurat v3 gene
// selection: the same grouped moments per batch, then a second walk with a per-(batch, gene) clip) share: the handle, the
// blocks of the walk over label-sorted rows, and the calls that run the walk.
#pragma once

#include "common.hpp"

#include <vector>

struct srx_markers {
    srx_ctx* ctx = nullptr;
    uint64_t n_rows = 0, n_cols = 0;
    uint32_t n_groups = 0, n_top = 0;
    int logged = 1;
    // one allocation: the fixed-point tables S, Q (n_groups x G i64), the counts C (n_groups x G u32), the totals over the
    // groups (G each), the group sizes, and the top lists (n_groups x n_top)
    void* d_block = nullptr;
    long long *d_S = nullptr, *d_Q = nullptr, *d_totS = nullptr, *d_totQ = nullptr;
    uint32_t *d_C = nullptr, *d_totC = nullptr;
    uint64_t* d_sizes = nullptr;
    uint32_t* d_top_gene = nullptr;
    double *d_top_score = nullptr, *d_top_lfc = nullptr;
    srx_markers_info info{};
    // the rank-sum route (wilcoxon.inl): an allocation of its own with the doubled rank sums R2 (n_groups x G u64) and the tie
    // terms T (G u64); null on a handle of the t-test
    bool wilcoxon = false;
    void* d_wx = nullptr;
    uint64_t *d_R2 = nullptr, *d_T = nullptr;
    srx_wilcoxon_info winfo{};
};

namespace srx {

// one workgroup of the walk: places [p0, p1) of the permutation, all of one group
struct MkBlock {
    uint32_t p0, p1;      // places of the permutation
    uint32_t group, pad_;
};

// What a second walk over the same label-sorted rows needs.  The device pointers are the context's scratch buffers "mk_perm"
// and "mk_blocks": valid until the next call that sorts rows by label on this context.
struct MkPlan {
    const uint32_t* d_perm = nullptr;
    const MkBlock* d_blocks = nullptr;
    size_t n_blocks = 0;
    double fx_sum = 0.0, fx_sq = 0.0;      // 2^sum_scale_log2, 2^sq_scale_log2
    std::vector<uint64_t> sizes;           // cells per group
};

// d_small: the few words the host reads back from the passes over the values (common.hpp: value_scan's two) and the labels
enum { MK_MAXABS = VS_MAXABS, MK_FLAGS = VS_FLAGS, MK_MAXLABEL = 2, MK_WORDS = 4 };
constexpr unsigned long long kMkBadLabel = kValOwnFlag;
// the e of srx.h's fixed-point scales: max_abs = f 2^e, 0.5 <= f < 1, so e is the smallest integer with max_abs < 2^e (0 for 0),
// taken no lower than -30
inline int fx_exponent(double max_abs) {
    int e = 0;
    (void)std::frexp(max_abs, &e);
    return e > -30 ? e : -30;
}

// ---- rows planned by label, for every walk over label-sorted rows (markers.hip's own, hvg_seurat.hip's through the plan above,
// paga.hip's over a graph's rows).  The stable counting sort comes in two halves, so that the caller reads d_small (MK_WORDS
// words it zeroed; a label >= n_groups raises kMkBadLabel in word MK_FLAGS) and the sizes between them: `count` queues the
// histograms, their scan and the group sizes (d_sizes: n_groups u64 on the device), `place` writes the permutation.  The
// buffers are the context's scratch ("mk_perm", ...): valid until the next sort on this context.
struct LabelSort {
    uint32_t* d_perm = nullptr;
    int64_t* d_first = nullptr;
    uint16_t* d_rank = nullptr;
    uint64_t n = 0, n_blk = 0;
};
int32_t label_sort_count(srx_ctx* ctx, const uint32_t* d_labels, uint64_t n, uint32_t n_groups, unsigned long long* d_small, uint64_t* d_sizes,
                         LabelSort* s);
int32_t label_sort_place(srx_ctx* ctx, const uint32_t* d_labels, const LabelSort& s);
// the workgroups of a walk: at most rows_per_block consecutive places of ONE group each, groups ascending
std::vector<MkBlock> label_blocks(const std::vector<uint64_t>& sizes, uint64_t rows_per_block);
// n_groups checked, n host labels uploaded into the scratch buffer "mk_labels" (not yet compared with n_groups: the sort does)
int32_t host_labels(srx_ctx* ctx, uint64_t n, const uint32_t* labels, uint32_t n_groups, const char* what, uint32_t** d_labels);
// the largest of n labels on the device (0 for none); drains the stream
int32_t label_max(srx_ctx* ctx, const uint32_t* d_labels, uint64_t n, uint64_t* mx);

void mk_free(srx_markers* mk);
// the refusals that need no pass over the matrix (NULL, CSC, several ranks, 2^32 - 1 rows or more); sets the device
int32_t markers_check(srx_mat* m, const char* what);
// n_groups checked, the labels uploaded into the scratch buffer "mk_labels"
int32_t markers_host_labels(srx_mat* m, const uint32_t* labels, uint32_t n_groups, const char* what, uint32_t** d_labels);
// the grouped moments alone (srx_group_moments' work): labels validated, rows sorted, S / Q and their totals filled; the
// counts C (a walk of their own over the indices) only with want_counts, else C and its totals stay 0
int32_t markers_moments(srx_mat* m, const uint32_t* d_labels, uint32_t n_groups, bool want_counts, srx_markers** out, MkPlan* plan);
// the walk of markers_moments once more with min(x, clip[group][gene]) in place of x: d_S, d_Q (n_groups x n_cols, zeroed by
// the caller) receive the fixed-point sums at the plan's scales; d_clip is n_groups x n_cols on the device
int32_t markers_clipped_walk(srx_mat* m, const MkPlan& plan, const double* d_clip, unsigned long long* d_S, unsigned long long* d_Q);

}  // namespace srx
