// PcaResultLayout (singlerust_amd/csrc/pca_result.hpp, included alone) against a literal restatement of the result block:
//
//   rounds x [ V k*64 | theta 64 | sgn 64 ] | mu k | sd k | trace 1 | pad 1 | sel_rank (int32) k
//
// in doubles from the start of the block; component p is column p - (first component of its round) of the round that holds it.
#include <cstdio>
#include <vector>

#include "../../singlerust_amd/csrc/pca_result.hpp"

static int failures = 0;
#define EXPECT_EQ(a, b)                                                                                            \
    do {                                                                                                           \
        const unsigned long long a_ = (unsigned long long)(a), b_ = (unsigned long long)(b);                      \
        if (a_ != b_) {                                                                                            \
            ++failures;                                                                                            \
            std::fprintf(stderr, "FAIL %s:%d: %s = %llu, want %s = %llu\n", __FILE__, __LINE__, #a, a_, #b, b_);   \
        }                                                                                                          \
    } while (0)

static void check(std::size_t k, const std::vector<int>& counts) {
    const srx::PcaResultLayout lay(k, 64, counts);
    const std::size_t rounds = counts.size();
    std::vector<std::size_t> edges;                       // every region's begin, in the documented order, then the end
    for (std::size_t r = 0; r < rounds; ++r) {
        const std::size_t at = r * (k * 64 + 64 + 64);
        EXPECT_EQ(lay.round_block(r), at);
        EXPECT_EQ(lay.V(r), at);
        EXPECT_EQ(lay.theta(r), at + k * 64);
        EXPECT_EQ(lay.sgn(r), at + k * 64 + 64);
        edges.push_back(lay.V(r));
        edges.push_back(lay.theta(r));
        edges.push_back(lay.sgn(r));
    }
    const std::size_t tail = rounds * (k * 64 + 64 + 64);
    EXPECT_EQ(lay.mu(), tail);
    EXPECT_EQ(lay.sd(), tail + k);
    EXPECT_EQ(lay.trace(), tail + k + k);
    EXPECT_EQ(lay.sel_rank(), tail + k + k + 1 + 1);
    const std::size_t sel_doubles = k % 2 ? k / 2 + 1 : k / 2;      // k int32 entries, rounded up to whole doubles
    EXPECT_EQ(lay.total_doubles(), tail + k + k + 1 + 1 + sel_doubles);
    edges.push_back(lay.mu());
    edges.push_back(lay.sd());
    edges.push_back(lay.trace());
    edges.push_back(lay.trace() + 1);                     // pad
    edges.push_back(lay.sel_rank());
    edges.push_back(lay.total_doubles());
    // disjoint, in order, no gap: every region begins where the one before it ends
    std::vector<std::size_t> sizes;
    for (std::size_t r = 0; r < rounds; ++r) {
        sizes.push_back(k * 64);
        sizes.push_back(64);
        sizes.push_back(64);
    }
    for (std::size_t s : {k, k, (std::size_t)1, (std::size_t)1, sel_doubles}) sizes.push_back(s);
    EXPECT_EQ(edges.size(), sizes.size() + 1);
    EXPECT_EQ(edges[0], 0);
    for (std::size_t i = 0; i < sizes.size(); ++i) EXPECT_EQ(edges[i + 1], edges[i] + sizes[i]);
    // every component, the first and the last of every round among them
    std::size_t p = 0;
    for (std::size_t r = 0; r < rounds; ++r)
        for (std::size_t c = 0; c < (std::size_t)counts[r]; ++c, ++p) {
            EXPECT_EQ(lay.locate(p).first, r);
            EXPECT_EQ(lay.locate(p).second, c);
            EXPECT_EQ(lay.col_offset(p), r * (k * 64 + 128) + c);
            EXPECT_EQ(lay.theta_offset(p), r * (k * 64 + 128) + k * 64 + c);
            EXPECT_EQ(lay.sgn_offset(p), r * (k * 64 + 128) + k * 64 + 64 + c);
        }
    // sized ahead of the solve by a round capacity: the same block
    const srx::PcaResultLayout cap(k, 64, rounds);
    EXPECT_EQ(cap.total_doubles(), lay.total_doubles());
    EXPECT_EQ(cap.mu(), lay.mu());
    EXPECT_EQ(cap.sel_rank(), lay.sel_rank());
}

int main() {
    check(2000, {50});                  // one round
    check(2000, {48, 48, 4});           // plan A with deflation
    check(2000, {25, 25});              // plan B
    check(2000, {32, 32, 32, 4});
    check(17, {17});                    // k <= 64: the direct solve; odd k
    check(1001, {48, 2});               // odd k: the int32 tail rounds up
    check(2000, {1});                   // n_pc = 1
    check(2, {1});
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
