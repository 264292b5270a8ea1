// pca_model.inl — a fitted PCA applied to other cells: Pca::transform (src/shared/processing/pca/mod.rs:156-185), included by
// pca_solve.hip after the solver (run_pca, srx_spmm, srx_iterate_op).  A model folds V, mu, sd' and the flags once into what the forward product consumes: f64 panels
// P = D^-1 V (slices of 64 columns, model rows in the fit's selection order) and cvec = c mu^T P.  A transform builds the
// selection bits of the genes the query has, compacts the query (the raw-value XF form under normalise + log1p), gathers
// the panel rows into the compacted columns' order (ascending query gene) and runs the fit's forward kernel per slice.

struct srx_pca_model {
    srx_ctx* ctx = nullptr;
    uint64_t k = 0, n_pc = 0;
    int center = 1, scale = 1;
    int n_slices = 0;
    double* d_panel = nullptr;        // n_slices x k x 64 f64 (columns beyond n_pc zero), then n_slices x 64 cvec
    double* d_cvec = nullptr;
    int32_t* d_sel = nullptr;         // from a resident result: the fit's selection, fetched to `sel` when first needed
    bool has_sel = false;
    std::vector<uint64_t> sel;
};

namespace srx {

// The slot (ascending-gene row of the fit's result block) of every selection position: the rank of its gene among the
// selected ones (the genes are distinct).  k x k comparisons through LDS — a one-off of the model build.
constexpr int kSlotTile = 1024;
__global__ __launch_bounds__(256) void k_sel_slots(const int32_t* __restrict__ sel, int k, int32_t* __restrict__ slot) {
    __shared__ int32_t s[kSlotTile];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int32_t g = i < k ? sel[i] : 0;
    int n = 0;
    for (int j0 = 0; j0 < k; j0 += kSlotTile) {
        const int m = min(kSlotTile, k - j0);
        __syncthreads();
        for (int t = threadIdx.x; t < m; t += 256) s[t] = sel[j0 + t];
        __syncthreads();
        for (int t = 0; t < m; ++t) n += s[t] < g ? 1 : 0;
    }
    if (i < k) slot[i] = n;
}

// One 64-column slice per blockIdx.y: P[i, c] = (1 / sd'[r]) (V[r, p] sgn_p) for model row i (r = src_row[i], or i), component
// p = 64 slice + c (0 beyond n_pc), and per-block partial sums of mu^T P (k_cvec_reduce adds them in fixed order: no atomics).
// V[r, p] = V[r * ld_v + col_off[p]]; sgn_p = the sign of V[sgn_off[p]] (sgn_off < 0: +1) — the fit's result block keeps the
// Ritz vectors unsigned beside their signs, a caller's components come signed.  sd null: no scaling; mu null: no centring.
// (1 / sd') V sgn is the fit's own rounding of its panel, d V sgn: a model of a resident result reproduces the fit's scores.)
__global__ __launch_bounds__(1024) void k_model_panel(const double* __restrict__ V, uint64_t ld_v, const int64_t* __restrict__ col_off,
                                                      const int64_t* __restrict__ sgn_off, const int32_t* __restrict__ src_row,
                                                      const double* __restrict__ mu, const double* __restrict__ sd, int k, int n_pc,
                                                      double* __restrict__ panel, double* __restrict__ part /* [slices][blocks][64] */) {
    __shared__ double s_part[16][L];
    const int c = threadIdx.x & (L - 1), sl = threadIdx.x / L, slice = blockIdx.y;
    const int p = slice * L + c;
    const bool in = p < n_pc;
    const int64_t off = in ? col_off[p] : 0;
    double sg = 1.0;
    if (in && sgn_off[p] >= 0) sg = V[sgn_off[p]] < 0 ? -1.0 : 1.0;
    double* out = panel + (size_t)slice * k * L;
    double acc = 0.0;
    for (int i = blockIdx.x * 16 + sl; i < k; i += gridDim.x * 16) {
        const uint64_t r = src_row ? (uint64_t)src_row[i] : (uint64_t)i;
        const double s = sd ? sd[r] : 1.0;
        const double di = s > 0 ? 1.0 / s : 1.0;                 // zero-variance feature: sd treated as 1 (srx_pca)
        const double pv = in ? di * (V[r * ld_v + off] * sg) : 0.0;
        out[(size_t)i * L + c] = pv;
        if (mu) acc += mu[r] * pv;
    }
    s_part[sl][c] = acc;
    __syncthreads();
    if (sl == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += s_part[w][c];
        part[((size_t)slice * gridDim.x + blockIdx.x) * L + c] = t;
    }
}

// Per transform: the panel rows of the kp compacted columns (slot s <- model row row_of_slot[s]) at the product's precision, then
// the slice's cvec — every slice laid out as the fit's panel (kp x 64 | 64).
template <typename PT>
__global__ __launch_bounds__(256) void k_model_gather(const double* __restrict__ panel, const double* __restrict__ cvec, int k,
                                                      const int32_t* __restrict__ row_of_slot, int kp, PT* __restrict__ P) {
    const int slice = blockIdx.y;
    const size_t per = (size_t)kp * L + L;
    const double* src = panel + (size_t)slice * k * L;
    PT* dst = P + (size_t)slice * per;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < per; e += (size_t)gridDim.x * 256) {
        const size_t s = e / L;
        const int c = (int)(e % L);
        dst[e] = (PT)(s < (size_t)kp ? src[(size_t)row_of_slot[s] * L + c] : cvec[(size_t)slice * L + c]);
    }
}

// V -> the model's panels and constants (see k_model_panel for the arguments)
static int32_t model_build(srx_pca_model* p, const double* V, uint64_t ld_v, const std::vector<int64_t>& col_off,
                           const std::vector<int64_t>& sgn_off, const int32_t* src_row, const double* mu, const double* sd) {
    srx_ctx* ctx = p->ctx;
    const int k = (int)p->k, n_pc = (int)p->n_pc, ns = p->n_slices;
    int64_t* offs;
    double* part;
    SRX_TRY(scratch(ctx, "pcam_offs", 2 * (size_t)n_pc * sizeof(int64_t), (void**)&offs));
    SRX_TRY(scratch(ctx, "pcam_part", (size_t)ns * kPanelBlocks * L * sizeof(double), (void**)&part));
    SRX_TRY(h2d(ctx, offs, col_off.data(), (size_t)n_pc * sizeof(int64_t)));
    SRX_TRY(h2d(ctx, offs + n_pc, sgn_off.data(), (size_t)n_pc * sizeof(int64_t)));
    hipLaunchKernelGGL(k_model_panel, dim3(kPanelBlocks, (unsigned)ns), dim3(1024), 0, ctx->stream, V, ld_v, (const int64_t*)offs,
                       (const int64_t*)(offs + n_pc), src_row, p->center ? mu : nullptr, p->scale ? sd : nullptr, k, n_pc, p->d_panel,
                       part);
    for (int s = 0; s < ns; ++s)
        hipLaunchKernelGGL((k_cvec_reduce<double>), dim3(1), dim3(L), 0, ctx->stream, (const double*)(part + (size_t)s * kPanelBlocks * L),
                           kPanelBlocks, p->center, p->d_cvec + (size_t)s * L);
    SRX_HIP(ctx, hipGetLastError());
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the staging scratch may be regrown by the next call
    return SRX_OK;
}

static int32_t model_alloc(srx_ctx* ctx, uint64_t k, uint64_t n_pc, int center, int scale, bool dev_sel, srx_pca_model** out) {
    auto* p = new srx_pca_model;
    p->ctx = ctx;
    p->k = k;
    p->n_pc = n_pc;
    p->center = center ? 1 : 0;
    p->scale = scale ? 1 : 0;
    p->n_slices = (int)((n_pc + L - 1) / L);
    const size_t doubles = (size_t)p->n_slices * (k * L + L);
    const size_t bytes = doubles * 8 + (dev_sel ? k * sizeof(int32_t) : 0);
    const hipError_t e = hipMalloc((void**)&p->d_panel, bytes);
    if (e != hipSuccess) {
        delete p;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "srx_pca_model: hipMalloc of %zu bytes failed: %s", bytes,
                    hipGetErrorString(e));
    }
    p->d_cvec = p->d_panel + (size_t)p->n_slices * k * L;
    if (dev_sel) p->d_sel = reinterpret_cast<int32_t*>(p->d_cvec + (size_t)p->n_slices * L);
    *out = p;
    return SRX_OK;
}

// the model's own gene ids on the host (a resident result's are fetched once)
static int32_t model_sel(srx_pca_model* p) {
    if (!p->has_sel || !p->sel.empty()) return SRX_OK;
    std::vector<int32_t> s(p->k);
    SRX_TRY(d2h(p->ctx, s.data(), p->d_sel, p->k * sizeof(int32_t)));
    p->sel.assign(s.begin(), s.end());
    return SRX_OK;
}

// Where a transform leaves its scores: the dense host matrix `host` (n_rows x n_pc), or — `dev` non-null — rows of `ld`
// doubles on the device (the forward product writes them where they lie: no staging copy, no host round trip).
struct ScoreDest {
    double* host = nullptr;
    double* dev = nullptr;
    size_t ld = 0;
};

// Scores of the CSR matrix `m` (the query, or its transpose / transformed copy) into `dst`.
template <typename VT>
static int32_t model_scores(srx_pca_model* p, srx_mat* m, const std::vector<uint64_t>& genes /* ascending */,
                            const std::vector<int32_t>& row_of_slot, RowXf xf, ScoreDest dst) {
    using PT = VT;
    srx_ctx* ctx = p->ctx;
    const uint64_t N = m->n_rows;
    const int kp = (int)genes.size(), ns = p->n_slices, n_pc = (int)p->n_pc, ld = dst.dev ? (int)dst.ld : scores_ld(n_pc);
    double* scores = dst.dev;
    if (!scores) SRX_TRY(scratch(ctx, "pcat_scores", (N ? N : 1) * (size_t)ld * sizeof(double), (void**)&scores));
    if (kp == 0) {
        // no model gene is in the query: every row is -cvec (at the product's precision)
        std::vector<double> cv((size_t)ns * L);
        SRX_TRY(d2h(ctx, cv.data(), p->d_cvec, cv.size() * sizeof(double)));
        if (dst.dev) {
            std::vector<double> rows(N * (size_t)ld, 0.0);
            for (uint64_t r = 0; r < N; ++r)
                for (int j = 0; j < n_pc; ++j) rows[r * ld + j] = -(double)(PT)cv[j];
            return h2d(ctx, dst.dev, rows.data(), rows.size() * sizeof(double));
        }
        for (uint64_t r = 0; r < N; ++r)
            for (int j = 0; j < n_pc; ++j) dst.host[r * n_pc + j] = -(double)(PT)cv[j];
        return SRX_OK;
    }
    // selection bits of the present genes and their prefix counts (the compacted column of a gene is its rank among them)
    const int n_words = (int)((m->n_cols + 31) / 32);
    std::vector<uint32_t> bits(2 * (size_t)n_words, 0u);
    for (uint64_t g : genes) bits[g >> 5] |= 1u << (g & 31);
    for (int w = 0, run = 0; w < n_words; ++w) {
        bits[n_words + w] = (uint32_t)run;
        run += __builtin_popcount(bits[w]);
    }
    uint32_t* d_bits;
    int32_t* d_map;
    PT* P;
    SRX_TRY(scratch(ctx, "pcat_bits", bits.size() * sizeof(uint32_t), (void**)&d_bits));
    SRX_TRY(scratch(ctx, "pcat_map", (size_t)kp * sizeof(int32_t), (void**)&d_map));
    SRX_TRY(scratch(ctx, "pcat_P", (size_t)ns * ((size_t)kp * L + L) * sizeof(PT), (void**)&P));
    SRX_TRY(h2d(ctx, d_bits, bits.data(), bits.size() * sizeof(uint32_t)));
    SRX_TRY(h2d(ctx, d_map, row_of_slot.data(), (size_t)kp * sizeof(int32_t)));
    const size_t per = (size_t)kp * L + L;
    hipLaunchKernelGGL((k_model_gather<PT>), dim3((unsigned)std::min<size_t>((per + 255) / 256, 1024), (unsigned)ns), dim3(256), 0,
                       ctx->stream, (const double*)p->d_panel, (const double*)p->d_cvec, (int)p->k, (const int32_t*)d_map, kp, P);
    SRX_HIP(ctx, hipGetLastError());
    RowMajor rm;
    SRX_TRY(compact_selection(m, d_bits, n_words, kp, rm, xf));
    for (int s = 0; s < ns; ++s) {
        const PT* Ps = P + (size_t)s * per;
        SRX_TRY((launch_fwd_rows<VT, PT>(ctx, rm, Ps, Ps + (size_t)kp * L, std::min(L, n_pc - s * L), scores + (size_t)s * L,
                                         (PT*)nullptr, ld)));
    }
    if (dst.dev) return SRX_OK;
    return d2h_rows(ctx, dst.host, scores, N, (size_t)n_pc * 8, (size_t)ld * 8);
}

// The body of srx_pca_transform, for either destination.
static int32_t pca_transform_into(srx_pca_model* p, srx_mat* q, const uint64_t* feat, double target_sum, int32_t transform,
                                  ScoreDest dst) {
    if (!p || !q) return fail(p ? p->ctx : q ? q->ctx : nullptr, SRX_E_ARG, "srx_pca_transform: null model or query");
    srx_ctx* ctx = q->ctx;
    if (p->ctx != ctx) return fail(ctx, SRX_E_ARG, "srx_pca_transform: model and query live on different contexts");
    if (transform & ~(SRX_BACKED_NORMALIZE | SRX_BACKED_LOG1P)) return fail(ctx, SRX_E_ARG, "srx_pca_transform: bad transform bits %d", transform);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t k = p->k;
    const uint64_t n_cells = q->csc ? q->n_cols : q->n_rows, n_genes = q->csc ? q->n_rows : q->n_cols;
    if (!feat) {
        if (!p->has_sel) return fail(ctx, SRX_E_ARG, "srx_pca_transform: feat == NULL needs a model that knows its feature ids");
        SRX_TRY(model_sel(p));
    }
    const uint64_t* fm = feat ? feat : p->sel.data();
    // the present genes in ascending query order (the compacted columns' order) and the model row of each
    std::vector<std::pair<uint64_t, int32_t>> present;
    present.reserve(k);
    for (uint64_t i = 0; i < k; ++i) {
        if (fm[i] == UINT64_MAX) continue;
        if (fm[i] >= n_genes) return fail(ctx, SRX_E_BOUNDS, "srx_pca_transform: feat[%llu] = %llu out of bounds (%llu genes)",
                                          (unsigned long long)i, (unsigned long long)fm[i], (unsigned long long)n_genes);
        present.emplace_back(fm[i], (int32_t)i);
    }
    std::sort(present.begin(), present.end());
    for (size_t s = 1; s < present.size(); ++s)
        if (present[s].first == present[s - 1].first)
            return fail(ctx, SRX_E_ARG, "srx_pca_transform: query column %llu named twice in feat", (unsigned long long)present[s].first);
    if (!dst.host && !dst.dev && n_cells) return fail(ctx, SRX_E_ARG, "srx_pca_transform: null scores_out");
    if (n_cells == 0) return SRX_OK;
    std::vector<uint64_t> genes(present.size());
    std::vector<int32_t> row_of_slot(present.size());
    for (size_t s = 0; s < present.size(); ++s) {
        genes[s] = present[s].first;
        row_of_slot[s] = present[s].second;
    }
    // the matrix the compaction reads: the query itself, the CSR of a CSC query (device transpose, as srx_pca), or — one of the
    // two transform bits alone — a copy transformed in place by the separate calls; both bits are applied on the fly
    const bool do_norm = (transform & SRX_BACKED_NORMALIZE) != 0, do_log = (transform & SRX_BACKED_LOG1P) != 0;
    srx_mat* own = nullptr;
    int32_t rc = SRX_OK;
    if (q->csc) rc = transpose_device(q, &own);
    else if (do_norm != do_log) rc = srx_matrix_clone(q, &own);
    srx_mat* m = own ? own : q;
    RowXf xf;
    if (rc == SRX_OK && do_norm && do_log) {
        double* rs = nullptr;
        rc = scratch(ctx, "pcat_rowsum", (m->n_rows ? m->n_rows : 1) * sizeof(double), (void**)&rs);
        if (rc == SRX_OK) rc = launch_row_sums(m, rs);
        xf.row_sum = rs;
        xf.target = target_sum;
    } else if (rc == SRX_OK && do_norm) {
        rc = srx_normalize_total_inplace(m, target_sum, SRX_ROW);
    } else if (rc == SRX_OK && do_log) {
        rc = srx_log1p_inplace(m);
    }
    if (rc == SRX_OK) {
        Range r_("srx:pca_transform");
        rc = is_f32(m) ? model_scores<float>(p, m, genes, row_of_slot, xf, dst)
                       : model_scores<double>(p, m, genes, row_of_slot, xf, dst);
    }
    if (own) srx_matrix_free(own);
    return rc;
}

// srx_pca_transform with feat == NULL whose scores stay on the device: row r of the query goes to d_out + r * ld (ld >= n_pc
// doubles; the columns from n_pc on are left as they are).  Same checks, same arithmetic, same bits as the host entry point.
int32_t pca_transform_device(srx_pca_model* p, srx_mat* q, double target_sum, int32_t transform, double* d_out, size_t ld) {
    if (!d_out || !p || ld < p->n_pc) return fail(p ? p->ctx : nullptr, SRX_E_ARG, "pca_transform_device: no room for the scores");
    return pca_transform_into(p, q, nullptr, target_sum, transform, ScoreDest{nullptr, d_out, ld});
}

}  // namespace srx

extern "C" {

int32_t srx_pca_model_from_result(srx_mat* m, srx_pca_model** out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    srx_ctx* ctx = m->ctx;
    const srx_pca_state& st = m->pca;
    if (!st.valid || !st.d_small) return fail(ctx, SRX_E_ARG, "srx_pca_model_from_result: no PCA result on this matrix");
    if (st.residual == kResidualRegress)
        return fail(ctx, SRX_E_ARG, "srx_pca_model_from_result: the result is a PCA of regressed, scaled and clipped values (srx_pca_regress); "
                                    "srx_pca_transform has no covariates to regress out of new cells");
    if (st.residual)
        return fail(ctx, SRX_E_ARG, "srx_pca_model_from_result: the result is a PCA of Pearson residuals (srx_pca_pearson); "
                                    "srx_pca_transform would apply normalise / log1p arithmetic to a residual model");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t k = st.k, n_pc = st.n_pc;
    srx_pca_model* p = nullptr;
    SRX_TRY(model_alloc(ctx, k, n_pc, st.center, st.scale, true, &p));
    const PcaResultLayout lay = result_block(st);         // (rows of V in slot — ascending gene — order)
    const int32_t* d_sel_rank = reinterpret_cast<const int32_t*>(st.d_small + lay.sel_rank());
    std::vector<int64_t> col_off(n_pc), sgn_off(n_pc);
    for (uint64_t j = 0; j < n_pc; ++j) {
        col_off[j] = (int64_t)lay.col_offset(j);
        sgn_off[j] = (int64_t)lay.sgn_offset(j);
    }
    int32_t* slots;
    int32_t rc = scratch(ctx, "pcam_slots", k * sizeof(int32_t), (void**)&slots);
    if (rc == SRX_OK) {
        hipLaunchKernelGGL(k_sel_slots, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, ctx->stream, d_sel_rank, (int)k, slots);
        const hipError_t e = hipMemcpyAsync(p->d_sel, d_sel_rank, k * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream);
        rc = e == hipSuccess ? SRX_OK : fail(ctx, SRX_E_HIP, "srx_pca_model_from_result: copy of the selection failed");
    }
    if (rc == SRX_OK) rc = model_build(p, st.d_small, L, col_off, sgn_off, slots, st.d_small + lay.mu(), st.d_small + lay.sd());
    if (rc != SRX_OK) {
        srx_pca_model_free(p);
        return rc;
    }
    p->has_sel = true;
    *out = p;
    return SRX_OK;
}

int32_t srx_pca_model_create(srx_ctx* ctx, uint64_t k, uint64_t n_pc, const double* components, const double* mean,
                             const double* std_, const uint64_t* sel, int32_t center, int32_t scale, srx_pca_model** out) {
    if (!ctx || !components || !out) return fail(ctx, SRX_E_ARG, "null argument");
    if (k < 1 || n_pc < 1 || n_pc > k) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: need 1 <= n_pc <= k (k = %llu, n_pc = %llu)",
                                                   (unsigned long long)k, (unsigned long long)n_pc);
    if (k >= (1ull << 31)) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: k = %llu features", (unsigned long long)k);
    if (center && !mean) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: a centred model needs its mean");
    if (scale && !std_) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: a scaled model needs its std");
    for (uint64_t e = 0; e < k * n_pc; ++e)
        if (std::isnan(components[e])) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: NaN in components[%llu]", (unsigned long long)e);
    for (uint64_t i = 0; mean && i < k; ++i)
        if (std::isnan(mean[i])) return fail(ctx, SRX_E_ARG, "srx_pca_model_create: NaN in mean[%llu]", (unsigned long long)i);
    for (uint64_t i = 0; std_ && i < k; ++i)
        if (!std::isfinite(std_[i]) || std_[i] < 0)
            return fail(ctx, SRX_E_ARG, "srx_pca_model_create: std[%llu] = %g is negative or not finite", (unsigned long long)i, std_[i]);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_pca_model* p = nullptr;
    SRX_TRY(model_alloc(ctx, k, n_pc, center, scale, false, &p));
    // the host arrays staged in one scratch buffer: V | mu | sd
    double* stage;
    int32_t rc = scratch(ctx, "pcam_stage", (k * n_pc + 2 * k) * sizeof(double), (void**)&stage);
    if (rc == SRX_OK) rc = h2d(ctx, stage, components, k * n_pc * sizeof(double));
    if (rc == SRX_OK && mean) rc = h2d(ctx, stage + k * n_pc, mean, k * sizeof(double));
    if (rc == SRX_OK && std_) rc = h2d(ctx, stage + k * n_pc + k, std_, k * sizeof(double));
    std::vector<int64_t> col_off(n_pc), sgn_off(n_pc, -1);
    std::iota(col_off.begin(), col_off.end(), (int64_t)0);
    if (rc == SRX_OK) rc = model_build(p, stage, n_pc, col_off, sgn_off, nullptr, stage + k * n_pc, stage + k * n_pc + k);
    if (rc != SRX_OK) {
        srx_pca_model_free(p);
        return rc;
    }
    if (sel) {
        p->has_sel = true;
        p->sel.assign(sel, sel + k);
    }
    *out = p;
    return SRX_OK;
}

int32_t srx_pca_model_info(const srx_pca_model* p, uint64_t* k_out, uint64_t* n_pc_out, uint64_t* sel_out) {
    if (!p) return fail(nullptr, SRX_E_ARG, "null model");
    if (k_out) *k_out = p->k;
    if (n_pc_out) *n_pc_out = p->n_pc;
    if (sel_out) {
        if (!p->has_sel) return fail(p->ctx, SRX_E_ARG, "srx_pca_model_info: the model has no feature ids");
        auto* mp = const_cast<srx_pca_model*>(p);          // (the lazily fetched host copy of a resident result's selection)
        SRX_HIP(p->ctx, hipSetDevice(p->ctx->device));
        SRX_TRY(model_sel(mp));
        memcpy(sel_out, mp->sel.data(), p->k * sizeof(uint64_t));
    }
    return SRX_OK;
}

void srx_pca_model_free(srx_pca_model* p) {
    if (!p) return;
    if (p->d_panel) {
        (void)hipSetDevice(p->ctx->device);
        (void)hipStreamSynchronize(p->ctx->stream);
        (void)hipFree(p->d_panel);
    }
    delete p;
}

int32_t srx_pca_transform(srx_pca_model* p, srx_mat* q, const uint64_t* feat, double target_sum, int32_t transform,
                          double* scores_out) {
    return pca_transform_into(p, q, feat, target_sum, transform, ScoreDest{scores_out, nullptr, 0});
}

}  // extern "C"
