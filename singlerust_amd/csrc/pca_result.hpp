// pca_result.hpp — the layout of the block of small results a PCA solve leaves in HBM (srx_pca_state::d_small, carved from the
// scores allocation): the one statement of it, for the solve that writes the block and for everything that reads it.  Plain C++.
#pragma once

#include <cstddef>
#include <utility>
#include <vector>

namespace srx {

// In doubles from the start of the block, w = the panel width (64), rows of V in slot (ascending gene) order:
//
//   rounds x [ V k*w | theta w | sgn w ] | mu k | sd k | trace 1 | pad 1 | sel_rank (int32) k
//
// One [V | theta | sgn] per deflation round (k_make_panel_mb writes it at the end of the round: the Ritz vectors unsigned, row
// stride w, beside their values and signs); the tail is k_sel_finish's vectors and the selection in rank order, whatever the
// selection was (stash_results).  Component p is column p - (first component of its round) of the round that resolved it.
struct PcaResultLayout {
    size_t k, w, rounds;
    std::vector<int> first;      // first component of every round, then n_pc (empty when built from a capacity)

    PcaResultLayout(size_t k_, size_t w_, const std::vector<int>& round_counts) : k(k_), w(w_), rounds(round_counts.size()), first(1, 0) {
        for (int n : round_counts) first.push_back(first.back() + n);
    }
    // sizing ahead of the solve: room for `round_capacity` rounds (no locate)
    PcaResultLayout(size_t k_, size_t w_, size_t round_capacity) : k(k_), w(w_), rounds(round_capacity) {}

    size_t round_block(size_t r) const { return r * (k * w + 2 * w); }
    size_t V(size_t r) const { return round_block(r); }
    size_t theta(size_t r) const { return V(r) + k * w; }
    size_t sgn(size_t r) const { return theta(r) + w; }
    size_t mu() const { return round_block(rounds); }
    size_t sd() const { return mu() + k; }
    size_t trace() const { return sd() + k; }
    size_t sel_rank() const { return trace() + 2; }             // k int32 entries, not doubles
    size_t total_doubles() const { return sel_rank() + (k + 1) / 2; }

    // (round, column within the round's 64) of component p
    std::pair<size_t, size_t> locate(size_t p) const {
        size_t r = 0;
        while (r + 1 < rounds && p >= (size_t)first[r + 1]) ++r;
        return {r, p - (size_t)first[r]};
    }
    // entry (row i, component p) of V is block[i * w + col_offset(p)]; the component's value and sign
    size_t col_offset(size_t p) const { return V(locate(p).first) + locate(p).second; }
    size_t theta_offset(size_t p) const { return theta(locate(p).first) + locate(p).second; }
    size_t sgn_offset(size_t p) const { return sgn(locate(p).first) + locate(p).second; }
};

}  // namespace srx
