// The schedule of the PCA solver (singlerust_amd/csrc/pca_schedule.hpp, included alone): known answers for the filter degrees,
// the sweep counts and the plans; the header against a literal copy of the expressions the solver's host loop held inline
// before they were moved into it (parent_* below), over a grid, to the bit; the options and widths of a plan's rounds by hand.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../singlerust_amd/csrc/pca_schedule.hpp"

static int failures = 0;
static long long checks = 0;
#define EXPECT(cond)                                                              \
    do {                                                                          \
        ++checks;                                                                 \
        if (!(cond)) {                                                            \
            ++failures;                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
        }                                                                         \
    } while (0)

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the inline expressions of the host loop, copied literally ---------------------------------------
struct ParentDeg { int d, d2; double ta; };
static ParentDeg parent_degrees(double r, double o_tol, double ratio, double spread, int q_applied) {
    const double ta = ratio > 0 && ratio < 1 ? 2.0 / ratio - 1.0 : 1.0;
    int d = 3;
    if (ta > 1.0) d = (int)std::ceil(std::acosh(std::max(4.0 * r / o_tol, 1.0)) / std::acosh(ta) - 1e-9);
    if (d > q_applied) d = q_applied;
    if (d > 12) d = 12;
    {
        const double t1 = 2.0 * (spread > 1.0 ? spread : 1.0) - 1.0;
        const int d_safe = t1 > 1.0 + 1e-9 ? (int)std::floor(32.9 / std::acosh(t1)) : 12;
        if (d > d_safe) d = d_safe;
    }
    if (d < 2) d = 2;
    int d2 = 0;
    if (ta > 1.0) {
        const int d_need = (int)std::ceil(std::acosh(std::max(4.0 * r / o_tol, 1.0)) / std::acosh(ta) - 1e-9);
        if (d_need > d + 1) {
            const double t1 = 2.0 * (spread > 1.0 ? spread : 1.0) - 1.0;
            const int d_safe = t1 > 1.0 + 1e-9 ? (int)std::floor(32.9 / std::acosh(t1)) : 12;
            d2 = std::min(std::min(d_need - d, 12), std::min(d_safe, q_applied + d));
            if (d2 < 2) d2 = 0;
        }
    }
    return {d, d2, ta};
}
static void parent_rate(double r, double r_last, int sweeps_since, double& rate_meas) {
    if (r_last < INFINITY && sweeps_since > 0 && r < r_last) rate_meas = std::pow(r / r_last, 1.0 / sweeps_since);
}
static int parent_m(double r, double o_tol, double ratio, int o_power, double rate_meas, int iters, int o_max_iter) {
    double rate = rate_meas > 0.0 ? rate_meas : std::pow(ratio < 1.0 ? ratio : 1.0, (double)o_power);
    if (!(rate > 1e-8)) rate = 1e-8;
    if (rate > 0.9) rate = 0.9;
    int m = (int)std::ceil(std::log(o_tol / r) / std::log(rate) - 1e-9);
    if (m < 1) m = 1;
    if (m > 6) m = 6;
    if (iters + m > o_max_iter) m = o_max_iter - iters;
    return m;
}
static double parent_tol2(bool loose, double o_tol) {
    constexpr double loose_tol2 = 1e-6;
    const double exact_tol2 = std::max(1e-30, (o_tol * 1e-4) * (o_tol * 1e-4));
    return loose ? loose_tol2 : exact_tol2;
}

// ---- (b) known answers ------------------------------------------------------------------------------
static void known_answers() {
    struct { double r, tol, ratio, spread; int q, d, d2; } deg[] = {
        {1e-3, 1e-9, 0.5, 30, 7, 6, 4},      // the "6 at 30x" of the comment
        {1e-3, 1e-9, 0.5, 100, 7, 5, 5},
        {1.6e-3, 1e-7, 0.5, 3, 7, 7, 0},
        {1e-2, 1e-9, 0.97, 1.5, 7, 7, 12},
        {1e-2, 1e-9, 0.97, 1.5, 1, 2, 3},
        {1e-2, 1e-9, 1.0, 2, 7, 3, 0},       // ratio outside (0, 1)
        {1e-2, 1e-9, 0.0, 2, 7, 3, 0},       // ratio outside (0, 1)
        {2e-9, 1e-9, 0.5, 2, 7, 2, 0},
        {1e-3, 1e-9, 0.9, 1.0, 40, 12, 12},
        {1e-3, 1e-9, 0.5, 4.99, 40, 10, 0},
        {1e-3, 1e-9, 0.2, 1e6, 7, 2, 2},
    };
    for (const auto& c : deg) {
        const srx::ChebDegrees g = srx::cheb_degrees(c.r, c.tol, c.ratio, c.spread, c.q);
        EXPECT(g.d == c.d && g.d2 == c.d2);
        if (g.d != c.d || g.d2 != c.d2)
            std::fprintf(stderr, "  (%g, %g, %g, %g, %d): got (%d, %d), want (%d, %d)\n", c.r, c.tol, c.ratio, c.spread, c.q, g.d, g.d2, c.d, c.d2);
    }
    EXPECT(srx::plain_sweeps(1e-3, 1e-9, 0.5, 3, 0.0, 1, 200) == 6);
    EXPECT(srx::plain_sweeps(1e-3, 1e-9, 0.5, 1, 0.0, 598, 600) == 2);      // the budget
    EXPECT(srx::plain_sweeps(1e-3, 1e-9, 1.0, 1, 0.0, 1, 600) == 6);        // rate clamped to 0.9
    // by hand: rate = 0.5^3 = 0.125, ln(1e-3) / ln(0.125) = 6.908 / 2.079 = 3.32 -> 4
    EXPECT(srx::plain_sweeps(1e-6, 1e-9, 0.5, 3, 0.0, 1, 200) == 4);
    // by hand, a measured rate takes the ratio's place: ln(1e-3) / ln(0.05) = 6.908 / 2.996 = 2.31 -> 3
    EXPECT(srx::plain_sweeps(1e-6, 1e-9, 0.5, 3, 0.05, 1, 200) == 3);

    using V = std::vector<int>;
    const srx::PcaPlans bench = srx::pca_plans(1000, 50, 64);               // the benchmark's case: short budget and bail apply
    EXPECT(bench.a == V({50}) && bench.b == V({25, 25}));
    EXPECT(bench.have_b() && bench.a_is_short());
    EXPECT(bench.budget_a(200) == 40 && bench.budget_a(30) == 30 && bench.bail_a() == 0.93);
    EXPECT(&bench.safest() == &bench.b && bench.max_rounds() == 2);
    const srx::PcaPlans p100 = srx::pca_plans(1000, 100, 64);
    EXPECT(p100.a == V({48, 48, 4}) && p100.b == V({25, 25, 25, 25}));
    EXPECT(p100.have_b() && !p100.a_is_short() && p100.budget_a(200) == 200 && p100.bail_a() == 0.0);
    const srx::PcaPlans p70 = srx::pca_plans(70, 70, 64);
    EXPECT(p70.a == V({48, 22}) && p70.b == V({24, 46}));
    EXPECT(!p70.have_b() && &p70.safest() == &p70.a && p70.budget_a(200) == 200 && p70.bail_a() == 0.0);
    const srx::PcaPlans p64 = srx::pca_plans(64, 64, 64);
    EXPECT(p64.a == V({64}) && p64.b == V({64}) && !p64.have_b() && !p64.a_is_short());
    EXPECT(srx::pca_plans(1000, 56, 64).a == V({56}));
    EXPECT(srx::pca_plans(1000, 57, 64).a == V({48, 9}));
    EXPECT(srx::kPcaPerRound == 48 && srx::kPcaPerRoundSafe == 32);

    EXPECT(srx::wanted_pairs(true, 37, 5) == 37 && srx::wanted_pairs(false, 64, 50) == 54 && srx::wanted_pairs(false, 52, 50) == 52);
    EXPECT(srx::step_bails(true, 0.93, 0.94) && !srx::step_bails(false, 0.93, 0.94) && !srx::step_bails(true, 0.0, 0.94) &&
           !srx::step_bails(true, 0.93, 0.93));
    int q = 7, iters = 1;
    srx::count_filter(6, 4, 3, q, iters);                                   // 10 applications: ceil(10 / 3) = 4 sweeps
    EXPECT(q == 17 && iters == 5);
    srx::count_filter(7, 0, 1, q, iters);
    EXPECT(q == 24 && iters == 12);
    EXPECT(srx::jacobi_tol2(true, 1e-9) == 1e-6 && srx::jacobi_tol2(false, 1e-20) == 1e-30);
}

// ---- (c) the header against the inline expressions, over a grid ---------------------------------------
static void grid() {
    const double tols[] = {1e-5, 1e-7, 1e-9};
    const double ratios[] = {0, 0.1, 0.5, 0.9, 0.93, 0.97, 0.999, 1, 1.2};
    const double spreads[] = {0.5, 1, 1 + 1e-10, 3, 30, 100, 1e6};
    const int qs[] = {1, 2, 3, 7, 13, 40};
    const int powers[] = {1, 3};
    for (int e = 0; e <= 48; ++e) {                                         // r = 1e-12 .. 1, four per decade
        const double r = std::pow(10.0, -12.0 + 0.25 * e);
        for (double tol : tols) {
            for (bool loose : {false, true}) EXPECT(same_bits(srx::jacobi_tol2(loose, tol), parent_tol2(loose, tol)));
            for (double ratio : ratios) {
                for (double spread : spreads)
                    for (int q : qs) {
                        const ParentDeg p = parent_degrees(r, tol, ratio, spread, q);
                        const srx::ChebDegrees g = srx::cheb_degrees(r, tol, ratio, spread, q);
                        EXPECT(g.d == p.d && g.d2 == p.d2 && same_bits(g.ta, p.ta));
                    }
                for (int power : powers)
                    for (double rate_meas : {0.0, 1e-12, 0.05, 0.3, 0.95})
                        for (int iters : {1, 38, 198})
                            for (int max_iter : {40, 200, 600})
                                EXPECT(srx::plain_sweeps(r, tol, ratio, power, rate_meas, iters, max_iter) ==
                                       parent_m(r, tol, ratio, power, rate_meas, iters, max_iter));
            }
        }
        for (double r_last : {(double)INFINITY, r * 10, r * 1.0000001, r, r * 0.5})
            for (int since : {0, 1, 3, 6})
                for (double before : {0.0, 0.3}) {
                    double want = before, got = before;
                    parent_rate(r, r_last, since, want);
                    if (const double rm = srx::measured_rate(r, r_last, since); rm >= 0.0) got = rm;      // as the host loop does
                    EXPECT(same_bits(got, want));
                }
    }
}

// ---- (d) the rounds of a three-round plan, by hand ---------------------------------------------------
static void rounds() {
    srx::Resolved o{};
    o.n_pc = 100, o.center = 1, o.scale = 1, o.max_iter = 200, o.solver = 1, o.power = 3, o.warm = 2, o.tol = 1e-9, o.seed = 7;
    const std::vector<int> plan = {48, 48, 4};
    for (int r = 0; r < 3; ++r) {
        const srx::Resolved a = srx::round_options(o, plan[r], r, 40, 0.93, false);
        EXPECT(a.n_pc == plan[r] && a.max_iter == 40 && a.seed == 7u + (unsigned)r && a.bail_ratio == 0.93);
        EXPECT(!a.robust && a.power == 3 && a.warm == 2 && a.tol == 1e-9 && a.center == 1 && a.scale == 1 && a.solver == 1 && !a.direct);
        const srx::Resolved b = srx::round_options(o, plan[r], r, 200, 0.0, true);
        EXPECT(b.n_pc == plan[r] && b.seed == 7u + (unsigned)r && b.bail_ratio == 0.0);
        EXPECT(b.robust && b.power == 1 && b.warm == 6 && b.max_iter == 600);      // 2 x 3 applications up front, 200 x 3 in the budget
    }
    // widths: what is still in the operator, at most the block; a one-round plan keeps the width it was given
    EXPECT(srx::round_width(3, 64, 64, 1000, 0) == 64 && srx::round_width(3, 64, 64, 1000, 96) == 64);
    EXPECT(srx::round_width(3, 64, 64, 100, 0) == 64 && srx::round_width(3, 64, 64, 100, 48) == 52 && srx::round_width(3, 64, 64, 100, 96) == 4);
    EXPECT(srx::round_width(1, 37, 64, 1000, 0) == 37);
}

int main() {
    known_answers();
    grid();
    rounds();
    if (failures) {
        std::fprintf(stderr, "%d of %lld checks failed\n", failures, checks);
        return 1;
    }
    std::printf("all checks passed (%lld)\n", checks);
    return 0;
}
