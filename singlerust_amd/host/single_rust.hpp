// single_rust.hpp — C++ host-side mirror of the reference's API for the hot path, over the C ABI
// of include/srx.h.
//
// The reference is Rust (src/lib.rs:5-15 re-exports `memory::{processing, statistics}`); this image
// has no Rust toolchain, so the host side above the C ABI is C++ (the reference is compiled code).
// Names, argument order and error behaviour follow the reference so that a test written against
// this header reads like the reference's own (`src/memory/processing/mod.rs:334-482`):
//
//   single_rust::IMAnnData adata = single_rust::IMAnnData::new_basic(x, obs_names, var_names);
//   single_rust::memory::processing::normalize_total_inplace(adata, 1e4, Direction::Row);
//   single_rust::memory::processing::log1p_transform_inplace(adata);
//   single_rust::memory::processing::dim_red::pca_inplace(adata, 50, {}, {}, {}, FeatureSelection::HighlyVariable(2000));
//   const Array2& x_pca = adata.obsm().at("X_pca");
//
// `anyhow::Result<T>` becomes "returns T or throws single_rust::Error" (message = srx_last_error).
// Header-only; link with -lsrx_hip.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/srx.h"

namespace single_rust {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

enum class Direction { Row = 0, Column = 1 };                   // src/shared/mod.rs:39-42

struct FeatureSelection {                                        // src/shared/mod.rs:17-23
    enum Kind { HighlyVariableColK, HighlyVariableK, RandomizedK, VarianceThresholdK, NoneK } kind = NoneK;
    std::string col;
    std::size_t n = 0;
    double threshold = 0.0;
    static FeatureSelection HighlyVariableCol(std::string c) { FeatureSelection f; f.kind = HighlyVariableColK; f.col = std::move(c); return f; }
    static FeatureSelection HighlyVariable(std::size_t n) { FeatureSelection f; f.kind = HighlyVariableK; f.n = n; return f; }
    static FeatureSelection Randomized(std::size_t n) { FeatureSelection f; f.kind = RandomizedK; f.n = n; return f; }
    static FeatureSelection VarianceThreshold(double t) { FeatureSelection f; f.kind = VarianceThresholdK; f.threshold = t; return f; }
    static FeatureSelection None() { return FeatureSelection(); }
};

struct FlexValue {                                               // src/shared/mod.rs:62-66
    srx_flex c{SRX_FLEX_NONE, 0, 0.0};
    static FlexValue Absolute(std::uint32_t v) { FlexValue f; f.c = srx_flex{SRX_FLEX_ABSOLUTE, v, 0.0}; return f; }
    static FlexValue Relative(double p) { FlexValue f; f.c = srx_flex{SRX_FLEX_RELATIVE, 0, p}; return f; }
    static FlexValue None() { return FlexValue(); }
};

// nalgebra_sparse::CsrMatrix<T> as the reference holds it (usize offsets/indices, typed values).
template <typename T>
struct CsrMatrix {
    std::size_t nrows = 0, ncols = 0;
    std::vector<std::uint64_t> row_offsets, col_indices;
    std::vector<T> values;
};
template <typename T>
struct CscMatrix {                                               // nalgebra_sparse::CscMatrix<T>
    std::size_t nrows = 0, ncols = 0;
    std::vector<std::uint64_t> col_offsets, row_indices;
    std::vector<T> values;
};
template <typename T> struct DTypeOf;
template <> struct DTypeOf<std::int8_t> { static constexpr int v = SRX_I8; };
template <> struct DTypeOf<std::int16_t> { static constexpr int v = SRX_I16; };
template <> struct DTypeOf<std::int32_t> { static constexpr int v = SRX_I32; };
template <> struct DTypeOf<std::uint8_t> { static constexpr int v = SRX_U8; };
template <> struct DTypeOf<std::uint16_t> { static constexpr int v = SRX_U16; };
template <> struct DTypeOf<std::uint32_t> { static constexpr int v = SRX_U32; };
template <> struct DTypeOf<float> { static constexpr int v = SRX_F32; };
template <> struct DTypeOf<double> { static constexpr int v = SRX_F64; };

struct Array2 {                                                  // ndarray::Array2<f64>, row-major
    std::size_t nrows = 0, ncols = 0;
    std::vector<double> data;
    double operator()(std::size_t r, std::size_t c) const { return data[r * ncols + c]; }
};

class Context {
public:
    explicit Context(int device_id = 0) {
        int rc = srx_ctx_create(device_id, &h_);
        if (rc != SRX_OK) throw Error(rc, srx_last_error(nullptr));
    }
    ~Context() { srx_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    srx_ctx* handle() const { return h_; }
    void check(int rc) const {
        if (rc != SRX_OK) throw Error(rc, srx_last_error(h_));
    }

private:
    srx_ctx* h_ = nullptr;
};

// anndata_memory::IMAnnData reduced to what the path touches: X (device-resident), names, obsm/varm.
class IMAnnData {
public:
    template <typename T>
    static IMAnnData new_basic(Context& ctx, const CsrMatrix<T>& x, std::vector<std::string> obs_names,
                               std::vector<std::string> var_names, int store = SRX_STORE_AUTO) {
        IMAnnData a(ctx);
        srx_csr h{x.nrows, x.ncols, x.values.size(), x.row_offsets.data(), x.col_indices.data(),
                  const_cast<T*>(x.values.data()), DTypeOf<T>::v};
        ctx.check(srx_matrix_upload(ctx.handle(), &h, store, &a.x_));
        a.row_offsets_ = x.row_offsets;
        a.col_indices_ = x.col_indices;
        a.obs_names_ = std::move(obs_names);
        a.var_names_ = std::move(var_names);
        return a;
    }
    // X as ArrayData::CscMatrix: same entry points, the reference's CSC arithmetic (helper/csc.rs, scale_*_csc)
    template <typename T>
    static IMAnnData new_basic(Context& ctx, const CscMatrix<T>& x, std::vector<std::string> obs_names,
                               std::vector<std::string> var_names, int store = SRX_STORE_AUTO) {
        IMAnnData a(ctx);
        srx_csr h{x.nrows, x.ncols, x.values.size(), x.col_offsets.data(), x.row_indices.data(),
                  const_cast<T*>(x.values.data()), DTypeOf<T>::v};
        ctx.check(srx_matrix_upload_csc(ctx.handle(), &h, store, &a.x_));
        a.row_offsets_ = x.col_offsets;
        a.col_indices_ = x.row_indices;
        a.obs_names_ = std::move(obs_names);
        a.var_names_ = std::move(var_names);
        return a;
    }
    bool x_is_csc() const {
        int32_t f = 0;
        ctx_->check(srx_matrix_format(x_, &f));
        return f == SRX_FORMAT_CSC;
    }
    IMAnnData(IMAnnData&& o) noexcept : ctx_(o.ctx_) { *this = std::move(o); }
    IMAnnData& operator=(IMAnnData&& o) noexcept {
        std::swap(x_, o.x_);
        row_offsets_ = std::move(o.row_offsets_);
        col_indices_ = std::move(o.col_indices_);
        obs_names_ = std::move(o.obs_names_);
        var_names_ = std::move(o.var_names_);
        obsm_ = std::move(o.obsm_);
        varm_ = std::move(o.varm_);
        var_bool_ = std::move(o.var_bool_);
        obs_cols_ = std::move(o.obs_cols_);
        var_cols_ = std::move(o.var_cols_);
        return *this;
    }
    ~IMAnnData() { srx_matrix_free(x_); }

    std::size_t n_obs() const { return info().n_rows; }
    std::size_t n_vars() const { return info().n_cols; }
    srx_mat* x() const { return x_; }
    Context& ctx() const { return *ctx_; }
    srx_mat_info info() const {
        srx_mat_info i{};
        ctx_->check(srx_matrix_info(x_, &i));
        return i;
    }
    // x().get_data(): the current values as the DynCsrMatrix variant X now is (F32 or F64)
    bool x_is_f64() const { return info().dtype != SRX_F32; }
    CsrMatrix<double> x_f64() const {
        CsrMatrix<double> m;
        auto i = info();
        m.nrows = i.n_rows;
        m.ncols = i.n_cols;
        m.row_offsets = row_offsets_;
        m.col_indices = col_indices_;
        m.values.resize(i.nnz);
        ctx_->check(srx_matrix_download_values(x_, m.values.data(), SRX_F64));
        return m;
    }
    IMAnnData deep_clone() const {                               // processing/mod.rs:315,330
        IMAnnData c(*ctx_);
        ctx_->check(srx_matrix_clone(x_, &c.x_));
        c.row_offsets_ = row_offsets_;
        c.col_indices_ = col_indices_;
        c.obs_names_ = obs_names_;
        c.var_names_ = var_names_;
        c.obsm_ = obsm_;
        c.varm_ = varm_;
        c.var_bool_ = var_bool_;
        c.obs_cols_ = obs_cols_;
        c.var_cols_ = var_cols_;
        return c;
    }
    // a matrix the library produced (filter / subset): the host copy of the pattern is downloaded
    static IMAnnData from_device(Context& ctx, srx_mat* x, std::vector<std::string> obs_names,
                                 std::vector<std::string> var_names) {
        IMAnnData a(ctx);
        a.x_ = x;
        auto i = a.info();
        a.row_offsets_.resize(i.n_rows + 1);
        a.col_indices_.resize(i.nnz);
        ctx.check(srx_matrix_download_pattern(x, a.row_offsets_.data(), a.col_indices_.data()));
        a.obs_names_ = std::move(obs_names);
        a.var_names_ = std::move(var_names);
        return a;
    }
    const std::vector<std::string>& obs_names() const { return obs_names_; }
    const std::vector<std::string>& var_names() const { return var_names_; }
    // numeric columns of the `obs` / `var` DataFrames (what qc_vars_inplace writes)
    std::map<std::string, std::vector<double>>& obs_columns() { return obs_cols_; }
    std::map<std::string, std::vector<double>>& var_columns() { return var_cols_; }
    // boolean columns of the `var` DataFrame (what FeatureSelection::HighlyVariableCol reads)
    std::map<std::string, std::vector<bool>>& var_bool() { return var_bool_; }
    const std::map<std::string, std::vector<bool>>& var_bool() const { return var_bool_; }
    std::map<std::string, Array2>& obsm() { return obsm_; }
    std::map<std::string, Array2>& varm() { return varm_; }

private:
    explicit IMAnnData(Context& ctx) : ctx_(&ctx) {}
    Context* ctx_;
    srx_mat* x_ = nullptr;
    std::vector<std::uint64_t> row_offsets_, col_indices_;
    std::vector<std::string> obs_names_, var_names_;
    std::map<std::string, Array2> obsm_, varm_;
    std::map<std::string, std::vector<bool>> var_bool_;
    std::map<std::string, std::vector<double>> obs_cols_, var_cols_;
};

namespace memory {

namespace statistics {                                           // src/memory/statistics/mod.rs:10-46
inline std::size_t len(const IMAnnData& a, Direction d) { return d == Direction::Row ? a.n_obs() : a.n_vars(); }
inline std::vector<std::uint32_t> compute_number(const IMAnnData& a, Direction d) {
    std::vector<std::uint32_t> v(len(a, d));
    a.ctx().check(srx_compute_number(a.x(), (int)d, v.data()));
    return v;
}
inline std::vector<double> compute_sum(const IMAnnData& a, Direction d) {
    std::vector<double> v(len(a, d));
    a.ctx().check(srx_compute_sum(a.x(), (int)d, v.data()));
    return v;
}
inline std::vector<double> compute_variance(const IMAnnData& a, Direction d) {
    std::vector<double> v(len(a, d));
    a.ctx().check(srx_compute_variance(a.x(), (int)d, v.data()));
    return v;
}
inline std::vector<double> compute_std_dev(const IMAnnData& a, Direction d) {
    std::vector<double> v(len(a, d));
    a.ctx().check(srx_compute_std_dev(a.x(), (int)d, v.data()));
    return v;
}
inline std::pair<std::vector<double>, std::vector<double>> compute_min_max(const IMAnnData& a, Direction d) {
    std::vector<double> mn(len(a, d)), mx(len(a, d));
    a.ctx().check(srx_compute_min_max(a.x(), (int)d, mn.data(), mx.data()));
    return {mn, mx};
}
// StatisticsContainer (src/memory/statistics/structs/mod.rs:1-10) and compute_qc_variables (mod.rs:48-72)
struct StatisticsContainer {
    std::vector<std::uint32_t> num_per_cell, num_per_gene;
    std::vector<double> expr_per_gene, expr_per_cell, variance_per_gene, variance_per_cell, std_dev_per_cell,
        std_dev_per_gene;
};
inline StatisticsContainer compute_qc_variables(const IMAnnData& a) {
    const std::size_t n = a.n_obs(), g = a.n_vars();
    StatisticsContainer c;
    c.num_per_cell.resize(n); c.num_per_gene.resize(g);
    c.expr_per_gene.resize(g); c.expr_per_cell.resize(n);
    c.variance_per_gene.resize(g); c.variance_per_cell.resize(n);
    c.std_dev_per_cell.resize(n); c.std_dev_per_gene.resize(g);
    a.ctx().check(srx_compute_qc_variables(a.x(), c.num_per_cell.data(), c.num_per_gene.data(), c.expr_per_gene.data(),
                                           c.expr_per_cell.data(), c.variance_per_gene.data(), c.variance_per_cell.data(),
                                           c.std_dev_per_cell.data(), c.std_dev_per_gene.data()));
    return c;
}
// qc_vars_inplace (src/memory/statistics/mod.rs:74-103): the eight vectors become columns of obs / var under the
// reference's names (counts are widened to f64: the mirror's DataFrames hold f64 columns)
inline void qc_vars_inplace(IMAnnData& a) {
    const StatisticsContainer d = compute_qc_variables(a);
    auto widen = [](const std::vector<std::uint32_t>& v) { return std::vector<double>(v.begin(), v.end()); };
    a.obs_columns()["num_genes_per_cell"] = widen(d.num_per_cell);
    a.obs_columns()["sum_expr_per_cell"] = d.expr_per_cell;
    a.obs_columns()["var_expr_per_cell"] = d.variance_per_cell;
    a.obs_columns()["std_dev_per_cell"] = d.std_dev_per_cell;
    a.var_columns()["num_cells_per_gene"] = widen(d.num_per_gene);
    a.var_columns()["sum_expr_per_gene"] = d.expr_per_gene;
    a.var_columns()["var_expr_per_gene"] = d.variance_per_gene;
    a.var_columns()["std_dev_per_gene"] = d.std_dev_per_gene;
}
}  // namespace statistics

namespace processing {                                           // src/memory/processing/mod.rs:303-332
inline void normalize_total_inplace(IMAnnData& a, double target_sum, Direction d) {
    a.ctx().check(srx_normalize_total_inplace(a.x(), target_sum, (int)d));
}
inline IMAnnData normalize_total(const IMAnnData& a, double target_sum, Direction d) {
    IMAnnData n = a.deep_clone();
    normalize_total_inplace(n, target_sum, d);
    return n;
}
inline void log1p_transform_inplace(IMAnnData& a) { a.ctx().check(srx_log1p_inplace(a.x())); }
inline IMAnnData log1p_transform(const IMAnnData& a) {
    IMAnnData n = a.deep_clone();
    log1p_transform_inplace(n);
    return n;
}

// filter_cells / filter_genes (processing/mod.rs:118-146, :271-299) and their in-place forms (:86-116, :245-269)
inline IMAnnData filter_impl(const IMAnnData& a, const FlexValue& lo, const FlexValue& hi, bool genes) {
    const std::size_t n = genes ? a.n_vars() : a.n_obs();
    std::vector<std::uint8_t> mask(n ? n : 1);
    srx_mat* out = nullptr;
    a.ctx().check(genes ? srx_filter_genes(a.x(), lo.c, hi.c, &out, mask.data())
                        : srx_filter_cells(a.x(), lo.c, hi.c, &out, mask.data()));
    std::vector<std::string> obs, var;
    for (std::size_t i = 0; i < a.obs_names().size(); ++i)
        if (genes || mask[i]) obs.push_back(a.obs_names()[i]);
    for (std::size_t j = 0; j < a.var_names().size(); ++j)
        if (!genes || mask[j]) var.push_back(a.var_names()[j]);
    return IMAnnData::from_device(a.ctx(), out, std::move(obs), std::move(var));
}
inline IMAnnData filter_cells(const IMAnnData& a, const FlexValue& lo, const FlexValue& hi) { return filter_impl(a, lo, hi, false); }
inline IMAnnData filter_genes(const IMAnnData& a, const FlexValue& lo, const FlexValue& hi) { return filter_impl(a, lo, hi, true); }
inline void filter_cells_inplace(IMAnnData& a, const FlexValue& lo, const FlexValue& hi) { a = filter_impl(a, lo, hi, false); }
inline void filter_genes_inplace(IMAnnData& a, const FlexValue& lo, const FlexValue& hi) { a = filter_impl(a, lo, hi, true); }

// Not in the reference: scanpy's highly_variable_genes(flavor = "pearson_residuals") on the RAW counts (srx.h states the
// definition).  The selected genes in rank order; var_bool()["highly_variable"] receives the mask that
// FeatureSelection::HighlyVariableCol("highly_variable") reads.  theta 0 = 100, clip 0 = sqrt(n_obs).
struct PearsonHvg {
    std::vector<std::uint64_t> selected;                          // rank order
    std::vector<double> residual_variances;                       // n_vars
    srx_pearson_info info{};
};
inline PearsonHvg highly_variable_genes_pearson(IMAnnData& a, std::size_t n_top_genes = 2000, double theta = 100.0, double clip = 0.0) {
    PearsonHvg r;
    const srx_pearson_opts opts{theta, clip};
    r.selected.resize(std::max<std::size_t>(std::min<std::size_t>(n_top_genes, a.n_vars()), 1));
    r.residual_variances.resize(std::max<std::size_t>(a.n_vars(), 1));
    std::uint64_t n_out = 0;
    a.ctx().check(srx_select_hvg_pearson(a.x(), n_top_genes, &opts, r.selected.data(), &n_out, r.residual_variances.data(), &r.info));
    r.selected.resize(n_out);
    r.residual_variances.resize(a.n_vars());
    std::vector<bool> mask(a.n_vars(), false);
    for (std::uint64_t g : r.selected) mask[g] = true;
    a.var_bool()["highly_variable"] = std::move(mask);
    return r;
}
// Not in the reference: scanpy's highly_variable_genes(flavor = "seurat_v3", batch_key = ..) on the RAW counts (srx.h states the
// definition: a direct loess surface).  `batch`: one code below n_batches per cell, or empty for one batch; paper_order: the
// order of "seurat_v3_paper".  The per-gene columns carry scanpy's names; var_bool()["highly_variable"] receives the mask.
struct SeuratV3Hvg {
    std::vector<std::uint64_t> selected;                          // rank order
    std::vector<double> means, variances, variances_norm, highly_variable_rank;      // n_vars each; the rank is NaN where no batch ranks the gene
    std::vector<std::uint32_t> highly_variable_nbatches;
    srx_seurat_v3_info info{};
};
inline SeuratV3Hvg highly_variable_genes_seurat_v3(IMAnnData& a, std::size_t n_top_genes = 2000, const std::vector<std::uint32_t>& batch = {},
                                                   std::uint32_t n_batches = 1, double span = 0.3, bool paper_order = false) {
    SeuratV3Hvg r;
    const std::size_t g = std::max<std::size_t>(a.n_vars(), 1);
    const srx_seurat_v3_opts opts{span, paper_order ? 1 : 0, 0};
    if (!batch.empty() && batch.size() != a.n_obs()) throw std::invalid_argument("highly_variable_genes_seurat_v3: one batch label per cell");
    r.selected.resize(std::max<std::size_t>(std::min<std::size_t>(n_top_genes, a.n_vars()), 1));
    r.means.resize(g); r.variances.resize(g); r.variances_norm.resize(g); r.highly_variable_rank.resize(g);
    r.highly_variable_nbatches.resize(g);
    srx_seurat_v3_tables t{};
    t.means = r.means.data(); t.variances = r.variances.data(); t.variances_norm = r.variances_norm.data();
    t.median = r.highly_variable_rank.data(); t.nbatches = r.highly_variable_nbatches.data();
    std::uint64_t n_out = 0;
    a.ctx().check(srx_select_hvg_seurat_v3(a.x(), n_top_genes, batch.empty() ? nullptr : batch.data(), batch.empty() ? 1u : n_batches, &opts,
                                           r.selected.data(), &n_out, &t, &r.info));
    r.selected.resize(n_out);
    for (auto* v : {&r.means, &r.variances, &r.variances_norm, &r.highly_variable_rank}) v->resize(a.n_vars());
    r.highly_variable_nbatches.resize(a.n_vars());
    std::vector<bool> mask(a.n_vars(), false);
    for (std::uint64_t j : r.selected) mask[j] = true;
    a.var_bool()["highly_variable"] = std::move(mask);
    return r;
}
// scanpy's normalize_pearson_residuals restricted to a gene list: n_obs x genes.size() clipped residuals, zeros included.
inline Array2 pearson_residuals(const IMAnnData& a, const std::vector<std::uint64_t>& genes, double theta = 100.0, double clip = 0.0) {
    const srx_pearson_opts opts{theta, clip};
    Array2 out;
    out.nrows = a.n_obs();
    out.ncols = genes.size();
    out.data.assign(std::max<std::size_t>(out.nrows * out.ncols, 1), 0.0);
    a.ctx().check(srx_pearson_residuals(a.x(), genes.data(), genes.size(), &opts, out.data.data(), nullptr));
    out.data.resize(out.nrows * out.ncols);
    return out;
}

// scanpy's normalize_pearson_residuals_pca on the RAW counts: PCA of the clipped residuals of `genes` (srx.h states the
// definition).  The scores stay resident as the handle's PCA result (neighbours, Harmony, ... read them there) and are stored as
// obsm["X_pca"]; selected_totals: the cell sums and the total over the listed genes (scanpy) instead of the whole matrix.
struct PearsonPca {
    Array2 scores, components;                                    // n_obs x n_pc, genes.size() x n_pc
    std::vector<double> explained_variance_ratio, mean;
    srx_pearson_pca_info info{};
};
inline PearsonPca pca_pearson_residuals(IMAnnData& a, const std::vector<std::uint64_t>& genes, int n_components = 50, double theta = 100.0,
                                        double clip = 0.0, bool selected_totals = true, bool center = true) {
    srx_pearson_pca_opts opts{};
    opts.pearson = srx_pearson_opts{theta, clip};
    opts.totals = selected_totals ? SRX_PEARSON_TOTALS_SELECTED : SRX_PEARSON_TOTALS_ALL;
    opts.center = center ? 1 : 0;
    opts.pca.n_components = n_components;
    opts.pca.center = -1;
    PearsonPca r;
    const std::size_t k = genes.size();
    const std::size_t n_pc = std::min<std::size_t>(n_components < 0 ? 2 : (std::size_t)n_components, k);
    r.scores.nrows = a.n_obs();
    r.scores.ncols = n_pc;
    r.components.nrows = k;
    r.components.ncols = n_pc;
    r.scores.data.assign(std::max<std::size_t>(a.n_obs() * n_pc, 1), 0.0);
    r.components.data.assign(std::max<std::size_t>(k * n_pc, 1), 0.0);
    r.explained_variance_ratio.assign(std::max<std::size_t>(n_pc, 1), 0.0);
    r.mean.assign(std::max<std::size_t>(k, 1), 0.0);
    a.ctx().check(srx_pca_pearson(a.x(), genes.data(), k, &opts, r.scores.data.data(), r.components.data.data(),
                                  r.explained_variance_ratio.data(), r.mean.data(), &r.info));
    r.scores.data.resize(a.n_obs() * n_pc);
    r.components.data.resize(k * n_pc);
    r.explained_variance_ratio.resize(n_pc);
    r.mean.resize(k);
    a.obsm()["X_pca"] = r.scores;
    return r;
}

// scanpy's regress_out -> scale(max_value) -> pca on the values as stored (after normalise + log1p): the covariates (n_obs x
// n_cov row-major; empty: plain scale + clip) regressed out of `genes`, the residuals scaled to unit variance and clipped, then
// their PCA (srx.h states the definition).  The scores stay resident as the handle's PCA result and are stored as obsm["X_pca"].
struct RegressPca {
    Array2 scores, components;                                    // n_obs x n_pc, genes.size() x n_pc
    std::vector<double> explained_variance_ratio, mean, std_;     // mean of the clipped values, the scale s
    srx_regress_info info{};
};
inline RegressPca pca_regress_scale(IMAnnData& a, const std::vector<std::uint64_t>& genes, const std::vector<double>& covariates,
                                    std::size_t n_cov, int n_components = 50, bool scale = true, double max_value = 10.0) {
    srx_regress_opts opts{};
    opts.scale = scale ? 1 : 0;
    opts.max_value = max_value;
    opts.pca.n_components = n_components;
    opts.pca.center = -1;
    RegressPca r;
    const std::size_t k = genes.size();
    const std::size_t n_pc = std::min<std::size_t>(n_components < 0 ? 2 : (std::size_t)n_components, k);
    if (covariates.size() != a.n_obs() * n_cov) throw std::invalid_argument("pca_regress_scale: covariates must hold n_obs x n_cov values");
    r.scores.nrows = a.n_obs();
    r.scores.ncols = n_pc;
    r.components.nrows = k;
    r.components.ncols = n_pc;
    r.scores.data.assign(std::max<std::size_t>(a.n_obs() * n_pc, 1), 0.0);
    r.components.data.assign(std::max<std::size_t>(k * n_pc, 1), 0.0);
    r.explained_variance_ratio.assign(std::max<std::size_t>(n_pc, 1), 0.0);
    r.mean.assign(std::max<std::size_t>(k, 1), 0.0);
    r.std_.assign(std::max<std::size_t>(k, 1), 0.0);
    a.ctx().check(srx_pca_regress(a.x(), genes.data(), k, n_cov ? covariates.data() : nullptr, n_cov, &opts, r.scores.data.data(),
                                  r.components.data.data(), r.explained_variance_ratio.data(), r.mean.data(), r.std_.data(), &r.info));
    r.scores.data.resize(a.n_obs() * n_pc);
    r.components.data.resize(k * n_pc);
    r.explained_variance_ratio.resize(n_pc);
    r.mean.resize(k);
    r.std_.resize(k);
    a.obsm()["X_pca"] = r.scores;
    return r;
}
// the regressed, scaled and clipped values themselves (n_obs x genes.size()): srx_regress_residuals
inline Array2 regress_out(const IMAnnData& a, const std::vector<std::uint64_t>& genes, const std::vector<double>& covariates,
                          std::size_t n_cov, bool scale = false, double max_value = 0.0) {
    srx_regress_opts opts{};
    opts.scale = scale ? 1 : 0;
    opts.max_value = max_value;
    if (covariates.size() != a.n_obs() * n_cov) throw std::invalid_argument("regress_out: covariates must hold n_obs x n_cov values");
    Array2 out;
    out.nrows = a.n_obs();
    out.ncols = genes.size();
    out.data.assign(std::max<std::size_t>(out.nrows * out.ncols, 1), 0.0);
    a.ctx().check(srx_regress_residuals(a.x(), genes.data(), genes.size(), n_cov ? covariates.data() : nullptr, n_cov, &opts,
                                        out.data.data(), nullptr));
    out.data.resize(out.nrows * out.ncols);
    return out;
}

// ---- sums over gene lists per cell, gene-set scores (srx.h states the definitions; scanpy's sc.tl.score_genes,
// score_genes_cell_cycle and the qc_vars of calculate_qc_metrics; the control genes of a bin are chosen by a hash, not by numpy's
// generator, and nothing is compared with scanpy)
struct GeneListSums {
    Array2 sum;                                // n_obs x n_lists
    std::vector<std::uint32_t> cnt;            // the same shape, row-major: stored entries, an explicit 0 included
    srx_gene_list_info info{};
};
inline std::pair<std::vector<std::uint64_t>, std::vector<std::uint64_t>> pack_lists(const std::vector<std::vector<std::uint64_t>>& lists) {
    std::vector<std::uint64_t> ptr(lists.size() + 1, 0), flat;
    for (std::size_t t = 0; t < lists.size(); ++t) {
        ptr[t + 1] = ptr[t] + lists[t].size();
        flat.insert(flat.end(), lists[t].begin(), lists[t].end());
    }
    if (flat.empty()) flat.push_back(0);
    return {ptr, flat};
}
inline GeneListSums gene_list_sums(const IMAnnData& a, const std::vector<std::vector<std::uint64_t>>& lists) {
    const auto packed = pack_lists(lists);
    GeneListSums r;
    r.sum.nrows = a.n_obs();
    r.sum.ncols = lists.size();
    r.sum.data.assign(std::max<std::size_t>(a.n_obs() * lists.size(), 1), 0.0);
    r.cnt.assign(std::max<std::size_t>(a.n_obs() * lists.size(), 1), 0u);
    a.ctx().check(srx_gene_list_sums(a.x(), packed.first.data(), packed.second.data(), lists.size(), r.sum.data.data(), r.cnt.data(), &r.info));
    r.sum.data.resize(a.n_obs() * lists.size());
    r.cnt.resize(a.n_obs() * lists.size());
    return r;
}
struct GeneScores {
    Array2 score;                                          // n_obs x n_sets
    std::vector<std::vector<std::uint64_t>> controls;      // per set, ascending
    srx_score_genes_info info{};
};
inline GeneScores score_genes(const IMAnnData& a, const std::vector<std::vector<std::uint64_t>>& sets, std::uint32_t ctrl_size = 50,
                              std::uint32_t n_bins = 25, const std::vector<std::uint64_t>* gene_pool = nullptr, std::uint64_t seed = 0,
                              bool ctrl_as_ref = true) {
    const auto packed = pack_lists(sets);
    srx_score_genes_opts opts{};
    opts.ctrl_size = ctrl_size;
    opts.n_bins = n_bins;
    opts.seed = seed;
    opts.ctrl_as_ref = ctrl_as_ref ? 1 : 0;
    // the bound of srx.h: per set ctrl_size * min(|set|, P / n_items + 1)
    const std::size_t P = gene_pool ? gene_pool->size() : a.n_vars(), size = ctrl_size ? ctrl_size : 50, bins = n_bins ? n_bins : 25;
    const std::size_t n_items = std::max<std::size_t>((std::size_t)std::nearbyint((double)P / (double)(std::max<std::size_t>(bins, 2) - 1)), 1);
    std::size_t capacity = 0;
    for (const auto& s : sets) capacity += size * std::min<std::size_t>(s.size(), P / n_items + 1);
    GeneScores r;
    r.score.nrows = a.n_obs();
    r.score.ncols = sets.size();
    r.score.data.assign(std::max<std::size_t>(a.n_obs() * sets.size(), 1), 0.0);
    std::vector<std::uint64_t> ctrl_ptr(sets.size() + 1, 0), ctrl(std::max<std::size_t>(capacity, 1), 0);
    a.ctx().check(srx_score_genes(a.x(), packed.first.data(), packed.second.data(), sets.size(), gene_pool ? gene_pool->data() : nullptr,
                                  gene_pool ? gene_pool->size() : 0, &opts, r.score.data.data(), ctrl_ptr.data(), ctrl.data(), ctrl.size(), &r.info));
    r.score.data.resize(a.n_obs() * sets.size());
    for (std::size_t s = 0; s < sets.size(); ++s) r.controls.emplace_back(ctrl.begin() + ctrl_ptr[s], ctrl.begin() + ctrl_ptr[s + 1]);
    return r;
}
struct CellCycle {
    std::vector<double> s_score, g2m_score;
    std::vector<std::string> phase;            // "S" by default, "G2M" where G2M > S, "G1" where both are < 0 (scanpy's rule and order)
};
inline CellCycle score_genes_cell_cycle(IMAnnData& a, const std::vector<std::uint64_t>& s_genes, const std::vector<std::uint64_t>& g2m_genes) {
    const GeneScores g = score_genes(a, {s_genes, g2m_genes}, (std::uint32_t)std::min(s_genes.size(), g2m_genes.size()));
    CellCycle r;
    for (std::size_t i = 0; i < a.n_obs(); ++i) {
        const double s = g.score.data[2 * i], m = g.score.data[2 * i + 1];
        r.s_score.push_back(s);
        r.g2m_score.push_back(m);
        r.phase.push_back(s < 0.0 && m < 0.0 ? "G1" : m > s ? "G2M" : "S");
    }
    a.obs_columns()["S_score"] = r.s_score;
    a.obs_columns()["G2M_score"] = r.g2m_score;
    return r;
}
// per subset k: total_counts_<k>, pct_counts_<k> = 100 * total / the cell's sum (0 / 0 stays NaN), n_genes_by_counts_<k> = the
// cell's STORED entries in the subset (an explicit 0 included: the one difference from scanpy's count of values > 0)
inline std::map<std::string, std::vector<double>> qc_gene_fractions(IMAnnData& a, const std::map<std::string, std::vector<std::uint64_t>>& subsets) {
    std::vector<std::vector<std::uint64_t>> lists;
    for (const auto& kv : subsets) lists.push_back(kv.second);
    const GeneListSums g = gene_list_sums(a, lists);
    const std::vector<double> total = statistics::compute_sum(a, Direction::Row);
    std::map<std::string, std::vector<double>> out;
    std::size_t t = 0;
    for (const auto& kv : subsets) {
        std::vector<double>&tc = out["total_counts_" + kv.first], &pc = out["pct_counts_" + kv.first], &ng = out["n_genes_by_counts_" + kv.first];
        for (std::size_t i = 0; i < a.n_obs(); ++i) {
            const double s = g.sum.data[i * lists.size() + t];
            tc.push_back(s);
            pc.push_back(100.0 * s / total[i]);
            ng.push_back((double)g.cnt[i * lists.size() + t]);
        }
        ++t;
    }
    for (const auto& kv : out) a.obs_columns()[kv.first] = kv.second;
    return out;
}

namespace dim_red {                                            // src/memory/processing/dim_red/mod.rs
inline std::vector<std::uint64_t> select_features(const IMAnnData& a, const FeatureSelection& fs) {   // :123-156
    switch (fs.kind) {
        case FeatureSelection::HighlyVariableK: {
            std::vector<std::uint64_t> idx(std::min<std::size_t>(fs.n, a.n_vars()));
            std::uint64_t n_out = 0;
            a.ctx().check(srx_select_hvg(a.x(), fs.n, idx.data(), &n_out));
            idx.resize(n_out);
            return idx;
        }
        case FeatureSelection::VarianceThresholdK: {
            auto var = statistics::compute_variance(a, Direction::Column);
            std::vector<std::uint64_t> idx;
            for (std::size_t i = 0; i < var.size(); ++i)
                if (var[i] > fs.threshold) idx.push_back(i);
            return idx;
        }
        case FeatureSelection::NoneK: {
            std::vector<std::uint64_t> idx(a.n_vars());
            for (std::size_t i = 0; i < idx.size(); ++i) idx[i] = i;
            return idx;
        }
        case FeatureSelection::HighlyVariableColK: {                       // :125-134: indices where the bool column is true
            auto it = a.var_bool().find(fs.col);
            if (it == a.var_bool().end()) throw Error(SRX_E_ARG, "Error accessing column '" + fs.col + "' : not found");
            std::vector<std::uint64_t> idx;
            for (std::size_t i = 0; i < it->second.size(); ++i)
                if (it->second[i]) idx.push_back(i);
            return idx;
        }
        case FeatureSelection::RandomizedK: {                              // :141-146: shuffle of 0..n_vars, first n (thread_rng)
            std::vector<std::uint64_t> idx(a.n_vars());
            for (std::size_t i = 0; i < idx.size(); ++i) idx[i] = i;
            std::random_device rd;
            std::mt19937_64 rng(rd());
            std::shuffle(idx.begin(), idx.end(), rng);
            idx.resize(std::min<std::size_t>(fs.n, idx.size()));
            return idx;
        }
    }
    throw Error(SRX_E_ARG, "unknown FeatureSelection");
}
// single_algebra's SVDImplementation markers (dim_red/mod.rs:12,24): accepted, as in the reference's signature, and
// ignored — the device solver has no SVD backend to choose.
struct FaerSVD {};
struct LapackSVD {};
// pca_inplace<S: SVDImplementation>(anndata, n_components, center, scale, n_threads, feature_selection, svd_mode)
// (:24-94), argument for argument.  Stores obsm["X_pca"] (:105-106) like attach_pca_results; returns the solver's info
// (the reference returns Ok(())).
template <typename S = FaerSVD>
inline srx_pca_info pca_inplace(IMAnnData& a, std::optional<std::size_t> n_components, std::optional<bool> center,
                                std::optional<bool> scale, std::optional<std::size_t> n_threads,
                                const FeatureSelection& fs, S /*svd_mode*/ = S{}) {
    auto sel = select_features(a, fs);
    srx_pca_opts o{};
    o.n_components = n_components ? (int)*n_components : -1;
    o.center = center ? (int)*center : -1;
    o.scale = scale ? (int)*scale : -1;
    o.n_threads = n_threads ? (int)*n_threads : -1;
    const std::size_t n_pc = std::min<std::size_t>(n_components.value_or(2), sel.size());    // :52
    Array2 scores;
    scores.nrows = a.n_obs();
    scores.ncols = n_pc;
    scores.data.resize(scores.nrows * n_pc);
    srx_pca_info info{};
    a.ctx().check(srx_pca(a.x(), sel.data(), sel.size(), &o, scores.data.data(), nullptr, nullptr, nullptr, nullptr,
                          &info));
    a.obsm()["X_pca"] = std::move(scores);
    return info;
}

// Pca after fit (src/shared/processing/pca/mod.rs:74): an owning wrapper of an srx_pca_model whose transform (:156-185)
// projects other cells into the fitted PC space on the device.
class PcaModel {
public:
    static constexpr std::uint64_t kAbsent = UINT64_MAX;     // feature-map entry of a model gene the query does not have
    // the model the last pca_inplace / pipeline on `a` left in HBM (a device-to-device copy: `a` may change afterwards)
    static PcaModel from_result(const IMAnnData& a) {
        PcaModel p(a.ctx());
        a.ctx().check(srx_pca_model_from_result(a.x(), &p.h_));
        return p;
    }
    // components k x n_pc row-major, mean / std k; sel (k feature ids, may be empty) for transform without a feature map
    static PcaModel from_parts(Context& ctx, std::size_t k, std::size_t n_pc, const std::vector<double>& components,
                               const std::vector<double>& mean, const std::vector<double>& std_,
                               const std::vector<std::uint64_t>& sel, bool center = true, bool scale = true) {
        if (components.size() != k * n_pc || (!mean.empty() && mean.size() != k) || (!std_.empty() && std_.size() != k) ||
            (!sel.empty() && sel.size() != k))
            throw Error(SRX_E_ARG, "PcaModel::from_parts: inconsistent sizes");
        PcaModel p(ctx);
        ctx.check(srx_pca_model_create(ctx.handle(), k, n_pc, components.data(), mean.empty() ? nullptr : mean.data(),
                                       std_.empty() ? nullptr : std_.data(), sel.empty() ? nullptr : sel.data(), center, scale,
                                       &p.h_));
        return p;
    }
    PcaModel(PcaModel&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    PcaModel& operator=(PcaModel&& o) noexcept {
        std::swap(ctx_, o.ctx_);
        std::swap(h_, o.h_);
        return *this;
    }
    PcaModel(const PcaModel&) = delete;
    PcaModel& operator=(const PcaModel&) = delete;
    ~PcaModel() { srx_pca_model_free(h_); }

    std::size_t k() const { return shape().first; }
    std::size_t n_pc() const { return shape().second; }
    // Pca::transform of the cells of `a`: feat = the query column of each model row (kAbsent where missing; empty = the
    // model's own feature ids); target_sum / log1p: normalize_total(Row) / ln_1p applied to the raw values on the fly
    Array2 transform(const IMAnnData& a, const std::vector<std::uint64_t>& feat = {}, std::optional<double> target_sum = {},
                     bool log1p = false) const {
        if (!feat.empty() && feat.size() != k()) throw Error(SRX_E_ARG, "PcaModel::transform: the feature map needs k entries");
        Array2 out;
        out.nrows = a.n_obs();
        out.ncols = n_pc();
        out.data.resize(out.nrows * out.ncols);
        const int bits = (target_sum ? SRX_BACKED_NORMALIZE : 0) | (log1p ? SRX_BACKED_LOG1P : 0);
        ctx_->check(srx_pca_transform(h_, a.x(), feat.empty() ? nullptr : feat.data(), target_sum.value_or(0.0), bits,
                                      out.data.empty() ? nullptr : out.data.data()));
        return out;
    }
    // the feature map from the model's gene names to the query's (var_names of the two objects)
    static std::vector<std::uint64_t> feature_map(const std::vector<std::string>& model_names,
                                                  const std::vector<std::string>& query_names) {
        std::map<std::string, std::uint64_t> where;
        for (std::size_t j = 0; j < query_names.size(); ++j) where.emplace(query_names[j], j);
        std::vector<std::uint64_t> f(model_names.size(), kAbsent);
        for (std::size_t i = 0; i < model_names.size(); ++i) {
            auto it = where.find(model_names[i]);
            if (it != where.end()) f[i] = it->second;
        }
        return f;
    }
    srx_pca_model* handle() const { return h_; }

private:
    explicit PcaModel(Context& ctx) : ctx_(&ctx) {}
    std::pair<std::size_t, std::size_t> shape() const {
        std::uint64_t k = 0, n = 0;
        ctx_->check(srx_pca_model_info(h_, &k, &n, nullptr));
        return {k, n};
    }
    Context* ctx_;
    srx_pca_model* h_ = nullptr;
};

// transform stored as obsm["X_pca"]
inline void pca_transform_inplace(IMAnnData& a, const PcaModel& model, const std::vector<std::uint64_t>& feat = {},
                                  std::optional<double> target_sum = {}, bool log1p = false) {
    a.obsm()["X_pca"] = model.transform(a, feat, target_sum, log1p);
}
}  // namespace dim_red

// Exact k-nearest-neighbour graph (Euclidean, f64; rows ascending by (distance, index)).  Not in the reference: the step
// that consumes obsm["X_pca"], in front of what its commented-out tsne (dim_red/mod.rs:159-227) would build.
struct KnnGraph {
    std::size_t n_query = 0, k = 0;
    std::vector<std::uint32_t> indices;      // n_query x k row-major
    std::vector<double> distances;
    srx_knn_info info{};
};
// self graph of the cells of `a` over the scores its last PCA left on the device (srx_knn_result)
inline KnnGraph neighbors(const IMAnnData& a, int n_neighbors = 15, int n_pcs = 0, bool include_self = false) {
    KnnGraph g;
    g.n_query = a.n_obs();
    g.k = n_neighbors > 0 ? static_cast<std::size_t>(n_neighbors) : 0;
    g.indices.resize(g.n_query * g.k);
    g.distances.resize(g.n_query * g.k);
    const srx_knn_opts o{n_neighbors, n_pcs, include_self ? 1 : 0, 0};
    a.ctx().check(srx_knn_result(a.x(), &o, g.indices.empty() ? nullptr : g.indices.data(),
                                 g.distances.empty() ? nullptr : g.distances.data(), &g.info));
    return g;
}
// neighbours of every query row among the reference rows (row-major n x d); an empty query: the self graph of ref
inline KnnGraph knn_points(Context& ctx, const std::vector<double>& ref, const std::vector<double>& query, std::size_t d,
                           int k = 15, bool include_self = false) {
    if (d == 0 || ref.size() % d || query.size() % d) throw Error(SRX_E_ARG, "knn_points: sizes are not multiples of d");
    KnnGraph g;
    const std::size_t n_ref = ref.size() / d;
    g.n_query = query.empty() ? n_ref : query.size() / d;
    g.k = k > 0 ? static_cast<std::size_t>(k) : 0;
    g.indices.resize(g.n_query * g.k);
    g.distances.resize(g.n_query * g.k);
    const srx_knn_opts o{k, 0, include_self ? 1 : 0, 0};
    ctx.check(srx_knn_points(ctx.handle(), ref.data(), n_ref, query.empty() ? nullptr : query.data(), g.n_query, d, &o,
                             g.indices.empty() ? nullptr : g.indices.data(),
                             g.distances.empty() ? nullptr : g.distances.data(), &g.info));
    return g;
}

// Approximate k-NN: an owning wrapper of an srx_knn_index (inverted-file index: centroids, lists, its own copy of the points).
// search() is exact within the n_probe nearest lists; n_probe == n_lists returns what knn_points returns.
class KnnIndex {
public:
    // over the scores the last PCA on `a` left on the device (srx_knn_index_result); trained centroids
    static KnnIndex of(const IMAnnData& a, int n_pcs = 0, const srx_ivf_opts& opts = srx_ivf_opts{0, 10, 0, 0}) {
        KnnIndex ix(a.ctx());
        a.ctx().check(srx_knn_index_result(a.x(), n_pcs, &opts, &ix.h_));
        return ix;
    }
    // over caller-supplied points (row-major n x d); centroids empty: trained, else opts.n_lists x d taken as they are
    static KnnIndex of_points(Context& ctx, const std::vector<double>& ref, std::size_t d, const std::vector<double>& centroids = {},
                              srx_ivf_opts opts = srx_ivf_opts{0, 10, 0, 0}) {
        if (d == 0 || ref.size() % d || centroids.size() % d) throw Error(SRX_E_ARG, "KnnIndex: sizes are not multiples of d");
        if (!centroids.empty()) opts.n_lists = static_cast<std::int32_t>(centroids.size() / d);
        KnnIndex ix(ctx);
        ctx.check(srx_knn_index_points(ctx.handle(), ref.data(), ref.size() / d, d, &opts,
                                       centroids.empty() ? nullptr : centroids.data(), &ix.h_));
        return ix;
    }
    KnnIndex(KnnIndex&& o) noexcept : ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    KnnIndex& operator=(KnnIndex&& o) noexcept {
        std::swap(ctx_, o.ctx_);
        std::swap(h_, o.h_);
        return *this;
    }
    KnnIndex(const KnnIndex&) = delete;
    KnnIndex& operator=(const KnnIndex&) = delete;
    ~KnnIndex() { srx_knn_index_free(h_); }

    srx_ivf_info info() const {
        srx_ivf_info i{};
        ctx_->check(srx_knn_index_info_get(h_, &i));
        return i;
    }
    // an empty query: the self form.  n_probe 0: min(20, n_lists).
    KnnGraph search(const std::vector<double>& query = {}, int k = 15, int n_probe = 0, bool include_self = false,
                    srx_ivf_search_info* sinfo = nullptr) const {
        const srx_ivf_info i = info();
        if (query.size() % i.d) throw Error(SRX_E_ARG, "KnnIndex::search: the query is not a multiple of d");
        KnnGraph g;
        g.n_query = query.empty() ? i.n_ref : query.size() / i.d;
        g.k = k > 0 ? static_cast<std::size_t>(k) : 0;
        g.indices.resize(g.n_query * g.k);
        g.distances.resize(g.n_query * g.k);
        const srx_knn_opts o{k, 0, include_self ? 1 : 0, 0};
        ctx_->check(srx_knn_index_search(h_, query.empty() ? nullptr : query.data(), g.n_query, &o, n_probe,
                                         g.indices.empty() ? nullptr : g.indices.data(),
                                         g.distances.empty() ? nullptr : g.distances.data(), sinfo));
        return g;
    }
    // (centroids n_lists x d, list offsets n_lists + 1, list members n_ref)
    void fetch(std::vector<double>& centroids, std::vector<std::uint64_t>& offsets, std::vector<std::uint32_t>& members) const {
        const srx_ivf_info i = info();
        centroids.resize(static_cast<std::size_t>(i.n_lists) * i.d);
        offsets.resize(static_cast<std::size_t>(i.n_lists) + 1);
        members.resize(i.n_ref);
        ctx_->check(srx_knn_index_fetch(h_, centroids.data(), offsets.data(), members.data()));
    }
    srx_knn_index* handle() const { return h_; }
    Context& ctx() const { return *ctx_; }

private:
    explicit KnnIndex(Context& ctx) : ctx_(&ctx) {}
    Context* ctx_;
    srx_knn_index* h_ = nullptr;
};

// The weighted neighbour graph (obsp["distances"], obsp["connectivities"]): an owning wrapper of an srx_graph.  Both matrices
// stay on the device as CSR for the consumers of the graph; csr() copies one to the host.
struct GraphCsr {
    std::vector<std::uint64_t> indptr;       // n + 1
    std::vector<std::uint32_t> indices;      // ascending within a row
    std::vector<double> data;
};
// eigenpairs of a diffusion map: evals descending, evecs n x n_comps row-major
struct Diffmap {
    std::uint64_t n = 0;
    std::uint32_t n_comps = 0;
    std::vector<double> evals, evecs;
};
// What PAGA gives uns["paga"]: the tables are n_groups x n_groups, row-major; `tree` holds its edges at g < h
struct Paga {
    std::uint32_t n_groups = 0;
    std::vector<std::uint64_t> sizes, out_edges, counts;
    std::vector<double> connectivities, expected, tree;
    srx_paga_info info{};
    explicit Paga(std::uint32_t G = 0)
        : n_groups(G), sizes(G), out_edges(G), counts(static_cast<std::size_t>(G) * G), connectivities(counts.size()),
          expected(counts.size()), tree(counts.size()) {}
    // the buffers as the C calls take them (the vectors must not be resized while it is in use)
    srx_paga_tables tables() {
        return srx_paga_tables{sizes.data(), out_edges.data(), counts.data(), connectivities.data(), expected.data(), tree.data()};
    }
};
// Moran's I and Geary's C per gene with their z-scores under normality, the five tables as f64 and as the integers themselves
// (srx_autocorr / srx_autocorr_csr); a constant gene has NaN statistics and is counted in info.genes_constant
struct Autocorr {
    std::vector<double> morans_i, gearys_c, z_i, z_c, sum, sumsq, dsum, dsumsq, cross;
    std::vector<std::int64_t> sum_int, sumsq_int, dsum_int, dsumsq_int, cross_int;
    srx_autocorr_info info{};
    explicit Autocorr(std::size_t G = 0)
        : morans_i(G), gearys_c(G), z_i(G), z_c(G), sum(G), sumsq(G), dsum(G), dsumsq(G), cross(G), sum_int(G), sumsq_int(G),
          dsum_int(G), dsumsq_int(G), cross_int(G) {}
    // the buffers as the C calls take them (the vectors must not be resized while it is in use)
    srx_autocorr_out out() {
        return srx_autocorr_out{morans_i.data(), gearys_c.data(), z_i.data(), z_c.data(), sum.data(), sumsq.data(), dsum.data(),
                                dsumsq.data(), cross.data(), sum_int.data(), sumsq_int.data(), dsum_int.data(), dsumsq_int.data(),
                                cross_int.data()};
    }
};
class Graph {
public:
    // k-NN over the scores the last PCA on `a` left on the device, then the graph of it (srx_neighbors_result)
    static Graph of(const IMAnnData& a, int n_neighbors = 15, int n_pcs = 0) {
        Graph g(a.ctx());
        const srx_knn_opts o{n_neighbors, n_pcs, 0, 0};
        a.ctx().check(srx_neighbors_result(a.x(), &o, &g.knn_info_, &g.h_));
        return g;
    }
    // the self search of an inverted-file index, then the graph of that list (srx_neighbors_index); knn_info() stays zero
    static Graph of_index(const KnnIndex& ix, int n_neighbors = 15, int n_probe = 0, srx_ivf_search_info* sinfo = nullptr) {
        Graph g(ix.ctx());
        const srx_knn_opts o{n_neighbors, 0, 0, 0};
        ix.ctx().check(srx_neighbors_index(ix.handle(), &o, n_probe, sinfo, &g.h_));
        return g;
    }
    // the graph of a k-NN list (n x k row-major; no row names itself): srx_neighbors_from_knn
    static Graph from_knn(Context& ctx, const std::vector<std::uint32_t>& indices, const std::vector<double>& distances,
                          std::size_t k) {
        if (k == 0 || indices.size() % k || indices.size() != distances.size())
            throw Error(SRX_E_ARG, "Graph::from_knn: indices and distances must both be n x k");
        Graph g(ctx);
        ctx.check(srx_neighbors_from_knn(ctx.handle(), indices.empty() ? nullptr : indices.data(),
                                         distances.empty() ? nullptr : distances.data(), indices.size() / k,
                                         static_cast<std::uint32_t>(k), &g.h_));
        return g;
    }
    // The shared-nearest-neighbour graph (Seurat's FindNeighbors, PhenoGraph): Jaccard index of the neighbour sets, pruned; an
    // ordinary Graph whose connectivities louvain(), umap(), paga() read.  Of a k-NN list (n x k row-major; `distances` may be
    // empty): srx_snn_from_knn.  opts null: Jaccard weights, every sharing pair, the cell in its own set, prune 1 / 15.
    static Graph snn_from_knn(Context& ctx, const std::vector<std::uint32_t>& indices, const std::vector<double>& distances,
                              std::size_t k, const srx_snn_opts* opts = nullptr, srx_snn_info* info = nullptr) {
        if (k == 0 || indices.size() % k || (!distances.empty() && indices.size() != distances.size()))
            throw Error(SRX_E_ARG, "Graph::snn_from_knn: indices must be n x k, distances too or empty");
        Graph g(ctx);
        ctx.check(srx_snn_from_knn(ctx.handle(), indices.empty() ? nullptr : indices.data(),
                                   distances.empty() ? nullptr : distances.data(), indices.size() / k,
                                   static_cast<std::uint32_t>(k), opts, info, &g.h_));
        return g;
    }
    // ... of the list this graph holds on the device, with no host round trip (srx_snn_graph): a new Graph, this one untouched
    Graph snn(const srx_snn_opts* opts = nullptr, srx_snn_info* info = nullptr) const {
        Graph g(*ctx_);
        ctx_->check(srx_snn_graph(h_, opts, info, &g.h_));
        return g;
    }
    // BBKNN (srx_bbknn_result): batch-balanced neighbours over the scores the last PCA on `a` left on the device, their graph,
    // trimmed as opts say (null: 3 neighbours per batch, all PCs, trim = 10 * 3 * n_batches).  `batch`: one label below
    // n_batches per cell.  The list has K = neighbors_within_batch * n_batches - 1 <= 64 entries per row.
    static Graph bbknn_of(const IMAnnData& a, const std::vector<std::uint32_t>& batch, std::uint32_t n_batches,
                          const srx_bbknn_opts* opts = nullptr, srx_bbknn_info* info = nullptr) {
        Graph g(a.ctx());
        a.ctx().check(srx_bbknn_result(a.x(), batch.empty() ? nullptr : batch.data(), n_batches, opts, info, &g.h_));
        return g;
    }
    // ... of caller-supplied points (n x d row-major): srx_bbknn_points; `indices` / `distances` (may be null) receive the n x K list
    static Graph bbknn_points(Context& ctx, const std::vector<double>& points, std::size_t d, const std::vector<std::uint32_t>& batch,
                              std::uint32_t n_batches, const srx_bbknn_opts* opts = nullptr, srx_bbknn_info* info = nullptr,
                              std::uint32_t* indices = nullptr, double* distances = nullptr) {
        if (d == 0 || points.size() % d || (n_batches != 1 && batch.size() != points.size() / d))
            throw Error(SRX_E_ARG, "Graph::bbknn_points: points must be n x d with one batch label per point");
        Graph g(ctx);
        ctx.check(srx_bbknn_points(ctx.handle(), points.empty() ? nullptr : points.data(), points.size() / d, d,
                                   batch.empty() ? nullptr : batch.data(), n_batches, opts, indices, distances, info, &g.h_));
        return g;
    }
    // BBKNN's trimming of the connectivities of any graph (srx_graph_trim): a new Graph, this one untouched
    Graph trim(std::int64_t trim, srx_trim_info* info = nullptr) const {
        Graph g(*ctx_);
        ctx_->check(srx_graph_trim(h_, trim, info, &g.h_));
        return g;
    }
    Graph(Graph&& o) noexcept : ctx_(o.ctx_), h_(o.h_), knn_info_(o.knn_info_) { o.h_ = nullptr; }
    Graph& operator=(Graph&& o) noexcept {
        std::swap(ctx_, o.ctx_);
        std::swap(h_, o.h_);
        std::swap(knn_info_, o.knn_info_);
        return *this;
    }
    Graph(const Graph&) = delete;
    Graph& operator=(const Graph&) = delete;
    ~Graph() { srx_graph_free(h_); }

    srx_graph_info info() const {
        srx_graph_info i{};
        ctx_->check(srx_graph_info_get(h_, &i));
        return i;
    }
    const srx_knn_info& knn_info() const { return knn_info_; }
    GraphCsr csr(int which) const {
        const srx_graph_info i = info();
        const std::uint64_t nnz = which == SRX_GRAPH_CONNECTIVITIES ? i.nnz_connectivities : i.nnz_distances;
        GraphCsr m;
        m.indptr.resize(i.n + 1);
        m.indices.resize(nnz);
        m.data.resize(nnz);
        ctx_->check(srx_graph_fetch(h_, which, m.indptr.data(), nnz ? m.indices.data() : nullptr, nnz ? m.data.data() : nullptr));
        return m;
    }
    GraphCsr distances() const { return csr(SRX_GRAPH_DISTANCES); }
    GraphCsr connectivities() const { return csr(SRX_GRAPH_CONNECTIVITIES); }
    // (rho, sigma), one per cell
    std::pair<std::vector<double>, std::vector<double>> scales() const {
        const std::uint64_t n = info().n;
        std::vector<double> rho(n), sigma(n);
        ctx_->check(srx_graph_fetch_scales(h_, n ? rho.data() : nullptr, n ? sigma.data() : nullptr));
        return {rho, sigma};
    }
    // Louvain communities of the connectivities, read where they lie (srx_louvain): one label per cell, communities
    // numbered by descending size; `info` (may be null) receives the call's srx_louvain_info
    std::vector<std::uint32_t> louvain(double resolution = 1.0, srx_louvain_info* info = nullptr, double min_gain = 0.0,
                                       int max_levels = 0, int max_sweeps = 0) const {
        const srx_louvain_opts o{resolution, min_gain, max_levels, max_sweeps};
        std::vector<std::uint32_t> labels(info_n());
        ctx_->check(srx_louvain(h_, &o, labels.empty() ? nullptr : labels.data(), info));
        return labels;
    }
    // the labels the last louvain() left on the device (srx_graph_labels_fetch)
    std::vector<std::uint32_t> labels() const {
        std::vector<std::uint32_t> labels(info_n());
        ctx_->check(srx_graph_labels_fetch(h_, labels.empty() ? nullptr : labels.data()));
        return labels;
    }
    // labels for new cells from the labels the last louvain() left on the device (srx_knn_vote_graph): `indices` is their k-NN
    // list among this graph's cells, n_query x k row-major; per new cell the most frequent label (ties to the lowest) and how
    // often it occurs
    std::pair<std::vector<std::uint32_t>, std::vector<std::uint32_t>> knn_vote(const std::vector<std::uint32_t>& indices,
                                                                               std::uint32_t k) const {
        if (!k || indices.size() % k) throw Error(SRX_E_ARG, "knn_vote: n_query x k indices expected");
        const std::size_t nq = indices.size() / k;
        std::vector<std::uint32_t> labels(nq), counts(nq);
        ctx_->check(srx_knn_vote_graph(h_, nq ? indices.data() : nullptr, nq, k, nq ? labels.data() : nullptr, nq ? counts.data() : nullptr));
        return {labels, counts};
    }
    // new cells placed in the embedding a srx_umap left on this handle, read where it lies (srx_umap_transform_graph): the
    // k-NN list as above with its distances, `dim` the embedding's; n_query x dim, row-major
    std::vector<double> umap_transform(const std::vector<std::uint32_t>& indices, const std::vector<double>& distances, std::uint32_t kq,
                                       std::uint32_t dim, const srx_umap_transform_opts* opts = nullptr,
                                       srx_umap_transform_info* info = nullptr) const {
        if (!kq || indices.size() % kq || distances.size() != indices.size())
            throw Error(SRX_E_ARG, "umap_transform: n_query x kq indices and distances expected");
        const std::size_t nq = indices.size() / kq;
        std::vector<double> emb(nq * dim);
        srx_umap_transform_out o{emb.empty() ? nullptr : emb.data(), nullptr, nullptr, nullptr, nullptr};
        ctx_->check(srx_umap_transform_graph(h_, nq ? indices.data() : nullptr, nq ? distances.data() : nullptr, nq, kq, dim, opts, &o, info));
        return emb;
    }
    // PAGA of the graph's D over the groups, read where it lies (srx_paga).  `labels` null: those the last louvain() left
    // on the device, n_groups = its n_communities or more; else one host label below n_groups per cell
    Paga paga(std::uint32_t n_groups, const std::vector<std::uint32_t>* labels = nullptr) const {
        if (labels && labels->size() != info_n()) throw Error(SRX_E_ARG, "paga: one label per cell expected");
        Paga p(n_groups);
        srx_paga_tables t = p.tables();
        ctx_->check(srx_paga(h_, labels && !labels->empty() ? labels->data() : nullptr, n_groups, &t, &p.info));
        return p;
    }
    // start positions for umap() from a PAGA result and a coarse layout `pos` (n_groups x dim, row-major): n x dim
    // (srx_paga_init_positions with the labels on the device)
    std::vector<double> paga_init_positions(const Paga& p, const std::vector<double>& pos, std::uint32_t dim, std::uint64_t seed = 0) const {
        if (pos.size() != static_cast<std::size_t>(p.n_groups) * dim) throw Error(SRX_E_ARG, "paga_init_positions: pos is n_groups x dim");
        std::vector<double> out(info_n() * dim);
        ctx_->check(srx_paga_init_positions(h_, nullptr, nullptr, info_n(), p.n_groups, p.connectivities.data(), pos.data(), dim, seed,
                                            out.empty() ? nullptr : out.data()));
        return out;
    }
    // ForceAtlas2 layout of the connectivities, read where they lie (srx_draw_graph): n x 2, row-major.  `opts` null: the
    // defaults (500 iterations from the hashed start); `init` (n x 2, e.g. paga_init_positions(p, pos, 2)) with
    // opts->init = SRX_FA2_INIT_GIVEN; `info` (may be null) receives the call's srx_fa2_info
    std::vector<double> draw_graph(const srx_fa2_opts* opts = nullptr, const std::vector<double>* init = nullptr,
                                   srx_fa2_info* info = nullptr) const {
        if (init && init->size() != info_n() * 2) throw Error(SRX_E_ARG, "draw_graph: the start is n x 2");
        std::vector<double> y(info_n() * 2);
        ctx_->check(srx_draw_graph(h_, opts, init && !init->empty() ? init->data() : nullptr, y.empty() ? nullptr : y.data(), info));
        return y;
    }
    // the layout the last draw_graph() left on the device (srx_graph_layout_fetch)
    std::vector<double> layout() const {
        std::vector<double> y(info_n() * 2);
        ctx_->check(srx_graph_layout_fetch(h_, y.empty() ? nullptr : y.data()));
        return y;
    }
    // Moran's I and Geary's C of every gene of `a` on the connectivities, read where they lie (srx_autocorr)
    Autocorr autocorr(const IMAnnData& a) const {
        Autocorr r(a.n_vars());
        srx_autocorr_out o = r.out();
        ctx_->check(srx_autocorr(a.x(), h_, nullptr, &o, &r.info));
        return r;
    }
    // Diffusion map of the connectivities, read where they lie (srx_diffmap): the n_comps algebraically largest eigenpairs of
    // the transition operator, descending; `opts` null: the defaults; `info` (may be null) receives the call's srx_diffmap_info
    Diffmap diffmap(const srx_diffmap_opts* opts = nullptr, srx_diffmap_info* info = nullptr) const {
        srx_diffmap_info li{};
        Diffmap d;
        d.n = info_n();
        const std::size_t room = opts && opts->n_comps > 0 ? static_cast<std::size_t>(opts->n_comps) : 15;
        d.evals.resize(room);
        d.evecs.resize(d.n * room);
        ctx_->check(srx_diffmap(h_, opts, d.evals.data(), d.evecs.data(), &li));
        d.n_comps = li.n_comps;
        d.evals.resize(d.n_comps);
        d.evecs.resize(d.n * d.n_comps);
        if (info) *info = li;
        return d;
    }
    // the values of the transition operator in the order of connectivities() (srx_graph_transitions_fetch)
    std::vector<double> transitions() const {
        std::vector<double> t(info().nnz_connectivities);
        ctx_->check(srx_graph_transitions_fetch(h_, t.empty() ? nullptr : t.data()));
        return t;
    }
    // pseudotime from `root` out of the eigenpairs the last diffmap() left on the device (srx_dpt; cap 0: 0.9994)
    std::vector<double> dpt(std::uint64_t root, double cap = 0.0) const {
        std::vector<double> p(info_n());
        ctx_->check(srx_dpt(h_, root, cap, p.data()));
        return p;
    }
    srx_graph* handle() const { return h_; }

private:
    explicit Graph(Context& ctx) : ctx_(&ctx) {}
    std::uint64_t info_n() const { return info().n; }
    Context* ctx_;
    srx_graph* h_ = nullptr;
    srx_knn_info knn_info_{};
};
// Louvain communities of any symmetric weighted graph (CSR, ascending columns, weights > 0, no diagonal): srx_louvain_csr
inline std::vector<std::uint32_t> louvain_csr(Context& ctx, const std::vector<std::uint64_t>& indptr,
                                              const std::vector<std::uint32_t>& indices, const std::vector<double>& weights,
                                              double resolution = 1.0, srx_louvain_info* info = nullptr) {
    if (indptr.empty() || indices.size() != weights.size() || indptr.back() != indices.size())
        throw Error(SRX_E_ARG, "louvain_csr: indptr (n + 1), indices and weights (indptr[n] each) expected");
    const srx_louvain_opts o{resolution, 0.0, 0, 0};
    std::vector<std::uint32_t> labels(indptr.size() - 1);
    ctx.check(srx_louvain_csr(ctx.handle(), indptr.data(), indices.empty() ? nullptr : indices.data(),
                              weights.empty() ? nullptr : weights.data(), labels.size(), &o, labels.empty() ? nullptr : labels.data(), info));
    return labels;
}
// ForceAtlas2 layout of any symmetric weighted graph (as for louvain_csr): srx_draw_graph_csr; n x 2, row-major
inline std::vector<double> draw_graph_csr(Context& ctx, const std::vector<std::uint64_t>& indptr, const std::vector<std::uint32_t>& indices,
                                          const std::vector<double>& weights, const srx_fa2_opts* opts = nullptr,
                                          const std::vector<double>* init = nullptr, srx_fa2_info* info = nullptr) {
    if (indptr.empty() || indices.size() != weights.size() || indptr.back() != indices.size())
        throw Error(SRX_E_ARG, "draw_graph_csr: indptr (n + 1), indices and weights (indptr[n] each) expected");
    const std::size_t n = indptr.size() - 1;
    if (init && init->size() != n * 2) throw Error(SRX_E_ARG, "draw_graph_csr: the start is n x 2");
    std::vector<double> y(n * 2);
    ctx.check(srx_draw_graph_csr(ctx.handle(), indptr.data(), indices.empty() ? nullptr : indices.data(),
                                 weights.empty() ? nullptr : weights.data(), n, opts, init && !init->empty() ? init->data() : nullptr,
                                 y.empty() ? nullptr : y.data(), info));
    return y;
}
// the speed rule of a ForceAtlas2 iteration on the host (srx_fa2_speed; no GPU): the new (speed, efficiency)
inline std::pair<double, double> fa2_speed(std::uint64_t n, double swing, double traction, double jitter_tolerance = 1.0, double speed = 1.0,
                                           double efficiency = 1.0) {
    const std::int32_t rc = srx_fa2_speed(n, swing, traction, jitter_tolerance, &speed, &efficiency);
    if (rc != SRX_OK) throw Error(rc, srx_last_error(nullptr));
    return {speed, efficiency};
}
// labels for new cells from host arrays (srx_knn_vote): their k-NN list among n_ref reference cells (n_query x k row-major)
// and one label below n_groups per reference cell; per new cell the most frequent label (ties to the lowest) and its count
inline std::pair<std::vector<std::uint32_t>, std::vector<std::uint32_t>> knn_vote(Context& ctx, const std::vector<std::uint32_t>& indices,
                                                                                  std::uint32_t k, const std::vector<std::uint32_t>& ref_labels,
                                                                                  std::uint32_t n_groups) {
    if (!k || indices.size() % k) throw Error(SRX_E_ARG, "knn_vote: n_query x k indices expected");
    const std::size_t nq = indices.size() / k;
    std::vector<std::uint32_t> labels(nq), counts(nq);
    ctx.check(srx_knn_vote(ctx.handle(), nq ? indices.data() : nullptr, nq, k, ref_labels.empty() ? nullptr : ref_labels.data(),
                           ref_labels.size(), n_groups, nq ? labels.data() : nullptr, nq ? counts.data() : nullptr));
    return {labels, counts};
}
// new cells placed in a fitted UMAP from host arrays (srx_umap_transform_knn): the k-NN list with its distances and the
// reference layout (n_ref x dim row-major, dim 2 or 3); n_query x dim, row-major
inline std::vector<double> umap_transform_knn(Context& ctx, const std::vector<std::uint32_t>& indices, const std::vector<double>& distances,
                                              std::uint32_t kq, const std::vector<double>& ref_embedding, std::uint32_t dim,
                                              const srx_umap_transform_opts* opts = nullptr, srx_umap_transform_info* info = nullptr) {
    if (!kq || indices.size() % kq || distances.size() != indices.size() || !dim || ref_embedding.size() % dim)
        throw Error(SRX_E_ARG, "umap_transform_knn: n_query x kq indices and distances and an n_ref x dim layout expected");
    const std::size_t nq = indices.size() / kq;
    std::vector<double> emb(nq * dim);
    srx_umap_transform_out o{emb.empty() ? nullptr : emb.data(), nullptr, nullptr, nullptr, nullptr};
    ctx.check(srx_umap_transform_knn(ctx.handle(), nq ? indices.data() : nullptr, nq ? distances.data() : nullptr, nq, kq,
                                     ref_embedding.empty() ? nullptr : ref_embedding.data(), ref_embedding.size() / dim, dim, opts, &o, info));
    return emb;
}
// the smallest shared count whose Jaccard index s / (2K - s) reaches `prune` (srx_snn_min_shared: host code, no GPU)
inline std::uint32_t snn_min_shared(std::uint32_t k, bool include_self = true, double prune = 1.0 / 15.0) {
    std::uint32_t s = 0;
    if (srx_snn_min_shared(k, include_self ? 1 : 0, prune, &s) != SRX_OK) throw Error(SRX_E_ARG, srx_last_error(nullptr));
    return s;
}
// PAGA of any directed pattern (CSR; every stored entry counts once) with one label below n_groups per row: srx_paga_csr
inline Paga paga_csr(Context& ctx, const std::vector<std::uint64_t>& indptr, const std::vector<std::uint32_t>& indices,
                     const std::vector<std::uint32_t>& labels, std::uint32_t n_groups) {
    if (indptr.empty() || indptr.back() != indices.size() || labels.size() != indptr.size() - 1)
        throw Error(SRX_E_ARG, "paga_csr: indptr (n + 1), indices (indptr[n]) and labels (n) expected");
    Paga p(n_groups);
    srx_paga_tables t = p.tables();
    ctx.check(srx_paga_csr(ctx.handle(), indptr.data(), indices.empty() ? nullptr : indices.data(), labels.size(),
                           labels.empty() ? nullptr : labels.data(), n_groups, &t, &p.info));
    return p;
}
// everything after the counts (host code in the library: no device): counts is n_groups x n_groups, row-major
inline Paga paga_from_counts(const std::vector<std::uint64_t>& counts, const std::vector<std::uint64_t>& sizes) {
    const std::uint32_t G = static_cast<std::uint32_t>(sizes.size());
    if (counts.size() != sizes.size() * sizes.size()) throw Error(SRX_E_ARG, "paga_from_counts: counts is n_groups x n_groups");
    Paga p(G);
    srx_paga_tables t = p.tables();
    const std::int32_t rc = srx_paga_from_counts(counts.data(), sizes.data(), G, &t, &p.info);
    if (rc != SRX_OK) throw Error(rc, srx_last_error(nullptr));
    return p;
}
// Moran's I and Geary's C on any symmetric weighted graph over the cells of `a` (CSR, ascending columns, weights > 0, no
// diagonal): srx_autocorr_csr
inline Autocorr autocorr_csr(const IMAnnData& a, const std::vector<std::uint64_t>& indptr, const std::vector<std::uint32_t>& indices,
                             const std::vector<double>& weights) {
    if (indptr.empty() || indices.size() != weights.size() || indptr.back() != indices.size())
        throw Error(SRX_E_ARG, "autocorr_csr: indptr (n + 1), indices and weights (indptr[n] each) expected");
    Autocorr r(a.n_vars());
    srx_autocorr_out o = r.out();
    a.ctx().check(srx_autocorr_csr(a.x(), indptr.data(), indices.empty() ? nullptr : indices.data(),
                                   weights.empty() ? nullptr : weights.data(), indptr.size() - 1, nullptr, &o, &r.info));
    return r;
}
// the eight fixed-point scales from info's n, nnz, max_abs, max_weight and max_degree (srx_autocorr_scales: host code)
inline srx_autocorr_info autocorr_scales(srx_autocorr_info info) {
    const std::int32_t rc = srx_autocorr_scales(&info);
    if (rc != SRX_OK) throw Error(rc, srx_last_error(nullptr));
    return info;
}
// the statistics from the five integer tables (host code in the library: no device); `info` carries n, the scales and the
// graph's integer sums
inline Autocorr autocorr_from_tables(const Autocorr& tables, const srx_autocorr_info& info) {
    Autocorr r = tables;
    r.info = info;
    srx_autocorr_out o = r.out();
    const std::int32_t rc = srx_autocorr_from_tables(tables.sum_int.data(), tables.sumsq_int.data(), tables.dsum_int.data(),
                                                     tables.dsumsq_int.data(), tables.cross_int.data(), tables.sum_int.size(), &r.info, &o);
    if (rc != SRX_OK) throw Error(rc, srx_last_error(nullptr));
    return r;
}
// Diffusion map of any symmetric weighted graph without empty rows (srx_diffmap_csr), and the pseudotime of such a result
inline Diffmap diffmap_csr(Context& ctx, const std::vector<std::uint64_t>& indptr, const std::vector<std::uint32_t>& indices,
                           const std::vector<double>& weights, const srx_diffmap_opts* opts = nullptr, srx_diffmap_info* info = nullptr) {
    if (indptr.empty() || indices.size() != weights.size() || indptr.back() != indices.size())
        throw Error(SRX_E_ARG, "diffmap_csr: indptr (n + 1), indices and weights (indptr[n] each) expected");
    srx_diffmap_info li{};
    Diffmap d;
    d.n = indptr.size() - 1;
    const std::size_t room = opts && opts->n_comps > 0 ? static_cast<std::size_t>(opts->n_comps) : 15;
    d.evals.resize(room);
    d.evecs.resize(d.n * room);
    ctx.check(srx_diffmap_csr(ctx.handle(), indptr.data(), indices.empty() ? nullptr : indices.data(),
                              weights.empty() ? nullptr : weights.data(), d.n, opts, d.evals.data(), d.evecs.data(), &li));
    d.n_comps = li.n_comps;
    d.evals.resize(d.n_comps);
    d.evecs.resize(d.n * d.n_comps);
    if (info) *info = li;
    return d;
}
inline std::vector<double> dpt_from(Context& ctx, const Diffmap& d, std::uint64_t root, double cap = 0.0) {
    std::vector<double> p(d.n);
    ctx.check(srx_dpt_from(ctx.handle(), d.evals.data(), d.evecs.data(), d.n, d.n_comps, root, cap, p.data()));
    return p;
}
}  // namespace processing
}  // namespace memory

// ---- single_rust::backed (src/backed/mod.rs): the matrix is not resident, it is visited as row chunks ----------
struct ComputationMode {                                          // src/shared/mod.rs:25-28
    enum Kind { ChunkedK, WholeK } kind = WholeK;
    std::size_t size = 0;
    static ComputationMode Chunked(std::size_t n) { ComputationMode m; m.kind = ChunkedK; m.size = n; return m; }
    static ComputationMode Whole() { return ComputationMode(); }
};

namespace backed {

// The CSR group of an h5ad `X` (indptr / indices / data) held by the caller: borrowed host arrays (a memory-mapped
// flat store, or the in-memory arrays).  `iter(chunk)` visits consecutive row ranges like ArrayElemOp::iter.
class BackedAnnData {
public:
    BackedAnnData(Context& ctx, std::size_t n_obs, std::size_t n_vars, const std::uint64_t* row_offsets,
                  const std::uint64_t* col_indices, const void* values, int dtype)
        : ctx_(&ctx), n_obs_(n_obs), n_vars_(n_vars), ip_(row_offsets), ix_(col_indices), v_(values), dtype_(dtype) {}
    template <typename T>
    static BackedAnnData of(Context& ctx, const CsrMatrix<T>& x) {
        return BackedAnnData(ctx, x.nrows, x.ncols, x.row_offsets.data(), x.col_indices.data(), x.values.data(), DTypeOf<T>::v);
    }
    std::size_t n_obs() const { return n_obs_; }
    std::size_t n_vars() const { return n_vars_; }
    Context& ctx() const { return *ctx_; }
    // rows [start, end) as an srx_csr tile: a window of the row offsets, nothing copied
    srx_csr tile(std::size_t start, std::size_t end) const {
        static const std::size_t width[] = {1, 2, 4, 1, 2, 4, 4, 8};      // SRX_I8 .. SRX_F64
        const std::uint64_t lo = ip_[start];
        return srx_csr{end - start, n_vars_, ip_[end] - lo, ip_ + start, ix_ + lo,
                       const_cast<char*>(static_cast<const char*>(v_)) + lo * width[dtype_], dtype_};
    }

private:
    Context* ctx_;
    std::size_t n_obs_, n_vars_;
    const std::uint64_t *ip_, *ix_;
    const void* v_;
    int dtype_;
};

class Session {                                                   // owning wrapper of an srx_backed
public:
    Session(Context& ctx, std::size_t n_cols, int store = SRX_STORE_AUTO) : ctx_(&ctx) {
        ctx.check(srx_backed_create(ctx.handle(), n_cols, store, &h_));
    }
    ~Session() { srx_backed_destroy(h_); }
    Session(const Session&) = delete;
    Session& operator=(const Session&) = delete;
    srx_backed* handle() const { return h_; }

private:
    Context* ctx_;
    srx_backed* h_ = nullptr;
};

namespace statistics {                                            // src/backed/statistics/mod.rs:5-45
namespace detail {
inline void sweep(const BackedAnnData& a, std::size_t size, Session& s, std::uint32_t* row_num, double* row_sum) {
    if (size == 0) throw Error(SRX_E_ARG, "ComputationMode::Chunked(0)");
    for (std::size_t start = 0; start < a.n_obs(); start += size) {
        const std::size_t end = std::min(start + size, a.n_obs());
        srx_csr t = a.tile(start, end);
        // every chunk writes at ITS rows (the reference's chunk helpers use the chunk-local index, csr.rs:57-62)
        a.ctx().check(srx_backed_stats_tile(s.handle(), &t, 0.0, 0, row_num ? row_num + start : nullptr,
                                            row_sum ? row_sum + start : nullptr));
    }
}
}  // namespace detail

inline std::vector<std::uint32_t> compute_number(const BackedAnnData& a, Direction d, const ComputationMode& mode) {
    const std::size_t chunk = mode.kind == ComputationMode::ChunkedK ? mode.size : std::max<std::size_t>(a.n_obs(), 1);
    Session s(a.ctx(), a.n_vars());
    std::vector<std::uint32_t> out(d == Direction::Row ? a.n_obs() : a.n_vars());
    detail::sweep(a, chunk, s, d == Direction::Row ? out.data() : nullptr, nullptr);
    if (d == Direction::Column) {
        std::vector<std::uint64_t> cnt(a.n_vars());
        a.ctx().check(srx_backed_moments(s.handle(), cnt.data(), nullptr, nullptr, nullptr));
        for (std::size_t j = 0; j < cnt.size(); ++j) out[j] = (std::uint32_t)cnt[j];
    }
    return out;
}

inline std::vector<double> compute_sum(const BackedAnnData& a, Direction d, const ComputationMode& mode) {
    const std::size_t chunk = mode.kind == ComputationMode::ChunkedK ? mode.size : std::max<std::size_t>(a.n_obs(), 1);
    Session s(a.ctx(), a.n_vars());
    std::vector<double> out(d == Direction::Row ? a.n_obs() : a.n_vars());
    detail::sweep(a, chunk, s, nullptr, d == Direction::Row ? out.data() : nullptr);
    if (d == Direction::Column) a.ctx().check(srx_backed_moments(s.handle(), nullptr, out.data(), nullptr, nullptr));
    return out;
}
}  // namespace statistics

namespace processing {
// The whole path over row chunks (the reference's backed::processing is empty; include/srx.h "backed mode").
struct PcaResult {
    Array2 x_pca;                      // n_obs x n_pc
    Array2 components;                 // k x n_pc, rows in selection order
    std::vector<double> explained_variance_ratio, mean, std_;
    std::vector<std::uint64_t> selected;
    srx_pca_info info{};
};
inline PcaResult pca_pipeline(const BackedAnnData& a, std::size_t chunk, double target_sum, std::size_t n_hvg,
                              int n_components, int store = SRX_STORE_AUTO) {
    if (chunk == 0) throw Error(SRX_E_ARG, "chunk size 0");
    Context& ctx = a.ctx();
    Session s(ctx, a.n_vars(), store);
    const int tf = SRX_BACKED_NORMALIZE | SRX_BACKED_LOG1P;
    for (std::size_t start = 0; start < a.n_obs(); start += chunk) {
        srx_csr t = a.tile(start, std::min(start + chunk, a.n_obs()));
        ctx.check(srx_backed_stats_tile(s.handle(), &t, target_sum, tf, nullptr, nullptr));
    }
    srx_pca_opts o{};
    o.n_components = n_components;
    o.center = o.scale = -1;
    std::uint64_t k = 0;
    ctx.check(srx_backed_select(s.handle(), n_hvg, nullptr, 0, &o, nullptr, &k));
    for (std::size_t start = 0; start < a.n_obs(); start += chunk) {
        srx_csr t = a.tile(start, std::min(start + chunk, a.n_obs()));
        ctx.check(srx_backed_gram_tile(s.handle(), &t, target_sum, tf));
    }
    PcaResult r;
    ctx.check(srx_backed_solve(s.handle(), &r.info));
    const std::size_t n_pc = r.info.n_pc;
    r.x_pca = Array2{a.n_obs(), n_pc, std::vector<double>(a.n_obs() * n_pc)};
    r.components = Array2{(std::size_t)k, n_pc, std::vector<double>(k * n_pc)};
    r.explained_variance_ratio.resize(n_pc);
    r.mean.resize(k);
    r.std_.resize(k);
    r.selected.resize(k);
    ctx.check(srx_backed_fetch(s.handle(), r.x_pca.data.data(), r.components.data.data(), r.explained_variance_ratio.data(),
                               r.mean.data(), r.std_.data(), r.selected.data()));
    return r;
}
}  // namespace processing
}  // namespace backed
}  // namespace single_rust
