// pca_schedule.hpp — every decision the host makes in a PCA solve (pca_solve.hip), as values: the plans of deflation rounds and
// their policy, the options of a round, and what one Rayleigh–Ritz step's read-back turns into (filter degrees, plain sweeps,
// tolerances, the bail).  Pure functions of the numbers the host holds at that point; tests/cpp/pca_schedule_test.cpp states
// them without a GPU.  Plain C++; the block width is an argument.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace srx {

struct Resolved {
    int n_pc, center, scale, max_iter, solver;
    double bail_ratio = 0.0; // > 0: give the round up after its first Ritz step when theta_l / theta_npc exceeds this (the
                             // caller has a plan with more guard columns per round)
    bool direct = false;     // k <= 64 with the explicit matrix: the block is the identity, one exact eigen-solve of C
    bool robust = false;     // last resort after a breakdown: CholeskyQR after every application of C, shifted
                             // CholeskyQR3, plain sweeps instead of Chebyshev filters
    int power = 1;           // applications of C per Rayleigh–Ritz step
    int warm = 0;            // leading sweeps of `power` applications + CholeskyQR WITHOUT a Rayleigh–Ritz step
    double tol;
    uint64_t seed;
};

// ---- plans --------------------------------------------------------------------------------------
// Components per deflation round when more than L - 8 are asked of a k > L problem (the block keeps 16 guard
// columns), and the number of rounds; the last round takes everything that is left once <= L dimensions remain.
constexpr int kPcaPerRound = 48;
constexpr int kPcaPerRoundSafe = 32;       // the fallback plan: >= 32 guard columns per round (c2, 1000 HVGs, 50 components:
                                           // 12 -> 19.6 ms, 16 -> 16.3, 24 -> 15.5, 32 -> 10.7)
// Components per round when at most `per` are asked of one round.
inline std::vector<int> plan_rounds(int k /* dimension of the operator's range */, int n_pc, int per, int L) {
    std::vector<int> counts;
    if (k <= L) {                            // the block spans the whole range: one exact round
        counts.push_back(n_pc);
        return counts;
    }
    int done = 0;
    while (done < n_pc) {
        const int take = (k - done <= L) ? n_pc - done : std::min(per, n_pc - done);
        counts.push_back(take);
        done += take;
    }
    return counts;
}

//   plan A: everything in one round up to 56 components (48 per round beyond) — two Ritz steps when the spectrum
//           decays across the block, the normal case;
//   plan B: rounds of <= 32 components with 32+ guard columns each.  Taken when plan A breaks down or stalls: a flat
//           tail (theta_64 / theta_50 -> 1) needs Chebyshev filters of high total degree, and with the dominant
//           eigenvalues still in the operator (theta_1 / theta_64 ~ 20-100) a degree-12 filter amplifies the leading
//           directions by T_12(t_1) ~ 1e20 over the guard columns — the block collapses onto them ("Cholesky pivot
//           <= 0").  Once a round has deflated the leading eigenpairs the remaining spectrum is narrow and the same
//           filters are harmless.
struct PcaPlans {
    std::vector<int> a, b;
    bool have_b() const { return b.size() > a.size(); }
    // One round for everything gets a short budget before the safe plan takes over; a plan A that already deflates
    // (n_pc > 56) keeps the full one.
    bool a_is_short() const { return have_b() && a.size() == 1; }
    int budget_a(int max_iter) const { return a_is_short() ? std::min(max_iter, 40) : max_iter; }
    // (a one-round plan A is also given up at once when its first Ritz step shows a flat tail, theta_64 / theta_npc >
    //  0.93: such a round needs a total filter degree of 45+ and plan B gets there sooner)
    double bail_a() const { return a_is_short() ? 0.93 : 0.0; }
    const std::vector<int>& safest() const { return have_b() ? b : a; }      // what robust mode runs
    size_t max_rounds() const { return std::max(a.size(), b.size()); }
};
inline PcaPlans pca_plans(int dim, int n_pc, int L) {
    const int n_b = (n_pc + kPcaPerRoundSafe - 1) / kPcaPerRoundSafe;
    return {plan_rounds(dim, n_pc, n_pc <= L - 8 ? n_pc : kPcaPerRound, L), plan_rounds(dim, n_pc, (n_pc + n_b - 1) / n_b, L)};
}

// The options of round r of a plan: its share of the components, its budget and seed, the caller's bail ratio.
inline Resolved round_options(const Resolved& o, int n_pc_r, int r, int budget, double bail, bool robust) {
    Resolved o_r = o;
    o_r.n_pc = n_pc_r;
    o_r.max_iter = budget;
    o_r.seed = o.seed + (uint64_t)r;
    o_r.bail_ratio = bail;
    if (robust) {                       // CholeskyQR after every application, the same number of applications up front
        o_r.robust = true;
        o_r.warm = o.warm * o.power;
        o_r.power = 1;
        o_r.max_iter = budget * o.power;
    }
    return o_r;
}
// The block width of a round that has `done` components behind it (dim - done: what is still in the operator).
inline int round_width(int rounds, int l_act, int L, int dim, int done) { return rounds == 1 ? l_act : std::min(L, dim - done); }

// ---- one Rayleigh–Ritz step ----------------------------------------------------------------------
// The eigen-solve's stopping tolerance (off-diagonal norm over the diagonal's, squared).
inline double jacobi_tol2(bool loose, double tol) {
    // the step after the warm-up only feeds the filter's bounds and the rotated start (any invertible U spans the same
    // block): off-diagonal norm 1e-3 of the diagonal is enough — the Ritz residual it reports, 1.63e-3 at c3, is the same
    // to three digits as with 1e-5 (1.62e-3), one Jacobi sweep less; at 1e-2 it reads 1.7e-2 and the filter takes a degree more
    constexpr double loose_tol2 = 1e-6;
    // an exact step: the off-diagonal norm the solver leaves behind shows up in the Ritz residuals as at most that norm
    // over theta_npc, i.e. sqrt(tol2) x (theta_1 / theta_npc) x a few — 1e-4 of the residual tolerance keeps it two
    // orders below what the step is judged on (tol 1e-7: 1e-22, one sweep of the quadratic tail less than 1e-30)
    return loose ? loose_tol2 : std::max(1e-30, (tol * 1e-4) * (tol * 1e-4));
}
// The pairs the eigen-solve must resolve (the guard columns' block need not be diagonal: jacobi.inl).
inline int wanted_pairs(bool direct, int l_act, int n_pc) { return direct ? l_act : std::min(l_act, n_pc + 4); }

// Is the round given up at its first Ritz step (flat tail: the caller has a plan with more guard columns)?
inline bool step_bails(bool first, double bail_ratio, double ratio) { return first && bail_ratio > 0.0 && ratio > bail_ratio; }

// The Chebyshev filter(s) behind a Ritz step with residual r and ratio = theta_l / theta_npc, spread = theta_1 / theta_l, on a
// block that has seen q_applied applications of C.  d2 > 0: a second filter behind the first one's CholeskyQR.
struct ChebDegrees { int d, d2; double ta; };
inline ChebDegrees cheb_degrees(double r, double tol, double ratio, double spread, int q_applied) {
    // degree: T_d(t_a) >= 4 r / tol with t_a = (2 theta_npc - b) / b = 2 / ratio - 1
    const double ta = ratio > 0 && ratio < 1 ? 2.0 / ratio - 1.0 : 1.0;
    const int d_need = ta > 1.0 ? (int)std::ceil(std::acosh(std::max(4.0 * r / tol, 1.0)) / std::acosh(ta) - 1e-9) : 3;
    int d = d_need;
    // The block captures eigenvector j up to an error ~ (b / lambda_j)^q after q applications of C, and a
    // degree-d filter multiplies that error (relative to the column's own component) by ~ (lambda_j / b)^d:
    // with d <= q the leading eigenvectors cannot swamp the other columns.  A degree-12 filter on a block
    // that had seen ONE application (SpMM solver, no warm-up) collapsed it ("block lost rank").
    if (d > q_applied) d = q_applied;
    if (d > 12) d = 12;                // T_12 of the largest t stays far inside f64; harder spectra take more rounds
    // The filter multiplies the component of every column along the leading eigenvector by T_d(t_1), t_1 =
    // 2 theta_1 / theta_l - 1, and the guard columns' own components by ~1: whatever rounding-level trace of v_1
    // a guard column carries (1e-16) must stay small against the column itself, or the block collapses onto the
    // leading directions and the next CholeskyQR finds a pivot <= 0.  T_d(t_1) <= 1e14 <=> d <= 32.9 / acosh(t_1):
    // no limit in practice when the block's spectrum spans less than 5x, 6 at 30x, 5 at 100x.
    const double t1 = 2.0 * (spread > 1.0 ? spread : 1.0) - 1.0;
    const int d_safe = t1 > 1.0 + 1e-9 ? (int)std::floor(32.9 / std::acosh(t1)) : 12;
    if (d > d_safe) d = d_safe;
    if (d < 2) d = 2;
    // the degree the tolerance asks for against the degree this filter may have: a second one behind it when one cannot do
    int d2 = 0;
    if (ta > 1.0 && d_need > d + 1) {
        d2 = std::min(std::min(d_need - d, 12), std::min(d_safe, q_applied + d));
        if (d2 < 2) d2 = 0;
    }
    return {d, d2, ta};
}
// What a filter step counts for: d - 1 (+ d2) applications in the filter(s) + the one of the Ritz step; `iters` in sweep
// equivalents (max_iter bounds applications of C).
inline void count_filter(int d, int d2, int power, int& q_applied, int& iters) {
    q_applied += d + d2;
    iters += (d + d2 + power - 1) / power;
}

// The rate of plain sweeps measured between two Ritz steps `sweeps_since` sweeps apart; negative: no measurement, the last
// one stands.
inline double measured_rate(double r, double r_last, int sweeps_since) {
    return r_last < INFINITY && sweeps_since > 0 && r < r_last ? std::pow(r / r_last, 1.0 / sweeps_since) : -1.0;
}
// Plain sweeps until the next Ritz step: as many as the rate (measured, else ratio^power) says the tolerance needs, 1..6,
// inside the budget.
inline int plain_sweeps(double r, double tol, double ratio, int power, double rate_meas, int iters, int max_iter) {
    double rate = rate_meas > 0.0 ? rate_meas : std::pow(ratio < 1.0 ? ratio : 1.0, (double)power);
    if (!(rate > 1e-8)) rate = 1e-8;
    if (rate > 0.9) rate = 0.9;
    int m = (int)std::ceil(std::log(tol / r) / std::log(rate) - 1e-9);
    if (m < 1) m = 1;
    if (m > 6) m = 6;
    if (iters + m > max_iter) m = max_iter - iters;
    return m;
}

}  // namespace srx
