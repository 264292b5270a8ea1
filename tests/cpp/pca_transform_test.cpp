// Pca::transform (src/shared/processing/pca/mod.rs:156-185) through the C++ host mirror: a PCA fitted on a matrix, then the
// fitted model applied to the same cells — from the resident result and from the host arrays, with and without a feature map
// — must give the fit's own scores (f32 storage: 1e-6, f64: 1e-12 of each component's largest score).
#include <cmath>
#include <cstdio>
#include <random>

#include "../../singlerust_amd/host/single_rust.hpp"

using namespace single_rust;
namespace proc = single_rust::memory::processing;
namespace dim_red = single_rust::memory::processing::dim_red;

static int failures = 0;
#define EXPECT(cond, ...)                                             \
    do {                                                              \
        if (!(cond)) {                                                \
            ++failures;                                               \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
        }                                                             \
    } while (0)

static CsrMatrix<double> counts(std::size_t nrows, std::size_t ncols, double density, unsigned seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::uniform_int_distribution<int> v(1, 30);
    CsrMatrix<double> m;
    m.nrows = nrows;
    m.ncols = ncols;
    m.row_offsets.push_back(0);
    for (std::size_t r = 0; r < nrows; ++r) {
        for (std::size_t c = 0; c < ncols; ++c)
            if (u(rng) < density) {
                m.col_indices.push_back(c);
                m.values.push_back((double)v(rng));
            }
        m.row_offsets.push_back(m.col_indices.size());
    }
    return m;
}

static std::vector<std::string> names(const char* p, std::size_t n) {
    std::vector<std::string> s;
    for (std::size_t i = 0; i < n; ++i) s.push_back(p + std::to_string(i));
    return s;
}

// max over components of max|got - want| / max|want|
static double comp_err(const Array2& got, const Array2& want) {
    double worst = 0.0;
    for (std::size_t c = 0; c < want.ncols; ++c) {
        double d = 0.0, m = 0.0;
        for (std::size_t r = 0; r < want.nrows; ++r) {
            d = std::max(d, std::fabs(got(r, c) - want(r, c)));
            m = std::max(m, std::fabs(want(r, c)));
        }
        worst = std::max(worst, m > 0 ? d / m : d);
    }
    return worst;
}

static void self_projection(Context& ctx, int store, double tol) {
    const std::size_t n = 600, g = 500, n_pc = 10, n_hvg = 200;
    IMAnnData a = IMAnnData::new_basic(ctx, counts(n, g, 0.1, 7 + store), names("obs", n), names("var", g), store);
    proc::normalize_total_inplace(a, 1e4, Direction::Row);
    proc::log1p_transform_inplace(a);
    dim_red::pca_inplace(a, n_pc, {}, {}, {}, FeatureSelection::HighlyVariable(n_hvg));
    const Array2 want = a.obsm().at("X_pca");

    auto m1 = dim_red::PcaModel::from_result(a);
    EXPECT(m1.k() == n_hvg && m1.n_pc() == n_pc, "model shape %zu x %zu", m1.k(), m1.n_pc());
    const Array2 s1 = m1.transform(a);
    EXPECT(s1.nrows == n && s1.ncols == n_pc, "scores shape %zu x %zu", s1.nrows, s1.ncols);
    EXPECT(comp_err(s1, want) <= tol, "store %d: model from the result: %.3g", store, comp_err(s1, want));

    std::vector<double> comps(n_hvg * n_pc), mean(n_hvg), sd(n_hvg);
    std::vector<std::uint64_t> sel(n_hvg);
    ctx.check(srx_result_fetch(a.x(), nullptr, comps.data(), nullptr, mean.data(), sd.data(), sel.data()));
    auto m2 = dim_red::PcaModel::from_parts(ctx, n_hvg, n_pc, comps, mean, sd, sel);
    const Array2 s2 = m2.transform(a);
    EXPECT(comp_err(s2, want) <= tol, "store %d: model from the host arrays: %.3g", store, comp_err(s2, want));
    // the same through a feature map made from gene names
    std::vector<std::string> model_names;
    for (auto s : sel) model_names.push_back(a.var_names()[s]);
    const auto feat = dim_red::PcaModel::feature_map(model_names, a.var_names());
    dim_red::pca_transform_inplace(a, m2, feat);
    EXPECT(comp_err(a.obsm().at("X_pca"), want) <= tol, "store %d: by names: %.3g", store, comp_err(a.obsm().at("X_pca"), want));
}

int main() {
    try {
        Context ctx(0);
        self_projection(ctx, SRX_STORE_F32, 1e-6);
        self_projection(ctx, SRX_STORE_F64, 1e-12);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 2;
    }
    if (failures) return 1;
    std::puts("pca transform: all checks passed");
    return 0;
}
