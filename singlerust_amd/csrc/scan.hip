// scan.hip — scan_exclusive: the device-wide exclusive scan of int64 counts that turns per-row counts into row pointers
// (HVG compaction, tile-major view, row filter, transpose, neighbour graph, Louvain aggregation).
// Three phases, 4096 elements per block: block sums, their scan by one workgroup, the scan inside every block.
#include "scan.hpp"

namespace srx {

constexpr int kScanItems = 4;
constexpr int kScanBlock = 1024;
__global__ __launch_bounds__(kScanBlock) void k_scan_block_sums(const int64_t* __restrict__ in, uint64_t n,
                                                                int64_t* __restrict__ block_sums) {
    __shared__ int64_t s_w[kScanBlock / kWave];
    uint64_t base = (uint64_t)blockIdx.x * kScanBlock * kScanItems;
    int64_t s = 0;
    for (int t = 0; t < kScanItems; ++t) {
        uint64_t i = base + (uint64_t)threadIdx.x * kScanItems + t;
        if (i < n) s += in[i];
    }
    s = wave_sum(s);
    if (lane_id() == 0) s_w[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t tot = 0;
        for (int w = 0; w < kScanBlock / kWave; ++w) tot += s_w[w];
        block_sums[blockIdx.x] = tot;
    }
}
// Exclusive scan of the block sums in place by ONE workgroup (nb is n/4096: a few thousand).
__global__ __launch_bounds__(kScanBlock) void k_scan_serial(int64_t* __restrict__ block_sums, uint64_t nb,
                                                            int64_t* __restrict__ total) {
    __shared__ int64_t s_w[kScanBlock / kWave];
    const uint64_t per = (nb + kScanBlock - 1) / kScanBlock;
    const uint64_t b0 = (uint64_t)threadIdx.x * per;
    const uint64_t b1 = b0 + per < nb ? b0 + per : nb;
    int64_t s = 0;
    for (uint64_t b = b0; b < b1; ++b) s += block_sums[b];
    int64_t all;
    int64_t acc = block_scan_exclusive<kScanBlock / kWave>(s, s_w, all);
    for (uint64_t b = b0; b < b1; ++b) {
        int64_t v = block_sums[b];
        block_sums[b] = acc;
        acc += v;
    }
    if (threadIdx.x == 0) *total = all;
}
__global__ __launch_bounds__(kScanBlock) void k_scan_apply(const int64_t* __restrict__ in, uint64_t n,
                                                           const int64_t* __restrict__ block_offs,
                                                           const int64_t* __restrict__ total,
                                                           int64_t* __restrict__ out /* n + 1 */) {
    __shared__ int64_t s_w[kScanBlock / kWave];
    uint64_t base = (uint64_t)blockIdx.x * kScanBlock * kScanItems;
    int64_t v[kScanItems];
    int64_t s = 0;
    for (int t = 0; t < kScanItems; ++t) {
        uint64_t i = base + (uint64_t)threadIdx.x * kScanItems + t;
        v[t] = i < n ? in[i] : 0;
        s += v[t];
    }
    int64_t block_total;       // (not used: block_offs has the sums of the blocks before this one)
    int64_t excl = block_offs[blockIdx.x] + block_scan_exclusive<kScanBlock / kWave>(s, s_w, block_total);
    for (int t = 0; t < kScanItems; ++t) {
        uint64_t i = base + (uint64_t)threadIdx.x * kScanItems + t;
        if (i < n) out[i] = excl;
        excl += v[t];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = *total;
}

// out[0..n] = exclusive scan of in[0..n), out[n] = total (also left in *total_dev).
int32_t scan_exclusive(srx_ctx* ctx, const int64_t* d_in, uint64_t n, int64_t* d_out, int64_t** total_dev) {
    const uint64_t per_block = (uint64_t)kScanBlock * kScanItems;
    const uint64_t nb = (n + per_block - 1) / per_block > 0 ? (n + per_block - 1) / per_block : 1;
    int64_t* d_bsum;
    SRX_TRY(scratch(ctx, "scan_bsum", (nb + 1) * sizeof(int64_t), (void**)&d_bsum));
    int64_t* d_total = d_bsum + nb;
    hipLaunchKernelGGL(k_scan_block_sums, dim3((unsigned)nb), dim3(kScanBlock), 0, ctx->stream, d_in, n, d_bsum);
    hipLaunchKernelGGL(k_scan_serial, dim3(1), dim3(kScanBlock), 0, ctx->stream, d_bsum, nb, d_total);
    hipLaunchKernelGGL(k_scan_apply, dim3((unsigned)nb), dim3(kScanBlock), 0, ctx->stream, d_in, n, d_bsum, d_total,
                       d_out);
    SRX_HIP(ctx, hipGetLastError());
    if (total_dev) *total_dev = d_total;
    return SRX_OK;
}

}  // namespace srx
