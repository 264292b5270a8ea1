// matrix.hip — the device-resident CSR of libsrx_hip.so: upload, alloc, clone, value storage, download, free.
//
// Device layout of X (SURVEY.md §8 "device layout"): int64 row offsets, int32 column
// indices, f32 or f64 values — the narrowing of the reference's usize indices
// (nalgebra_sparse::CsrMatrix) happens once, here.
#include "common.hpp"

#include <algorithm>

namespace srx {

// ---- upload kernels ------------------------------------------------------------------------------
template <typename S, typename D>
__global__ void k_convert_values(const S* __restrict__ src, D* __restrict__ dst, uint64_t n) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = (D)src[i];
}

// One wave per row: column indices strictly increasing inside the row (canonical CSR; the
// reference's CsrNonCanonical arm is todo!(), src/shared/statistics/mod.rs:11) and row
// offsets monotone.
__global__ void k_validate_rows(const int64_t* __restrict__ indptr, const int32_t* __restrict__ idx,
                                uint64_t n_rows, uint64_t nnz, int* __restrict__ flag) {
    uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / kWave;
    uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) / kWave;
    int lane = lane_id();
    bool bad = false;
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        int64_t lo = indptr[r], hi = indptr[r + 1];
        if (lo > hi || lo < 0 || (uint64_t)hi > nnz) { bad = true; continue; }
        for (int64_t p = lo + lane; p + 1 < hi; p += kWave) bad |= !(idx[p] < idx[p + 1]);
    }
    if (bad) atomicOr(flag, 2);
}

__global__ void k_rebase_indptr(int64_t* __restrict__ indptr, uint64_t n, int64_t base) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) indptr[i] -= base;
}

static int grid_for(uint64_t n, int block, int cap) {
    uint64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > (uint64_t)cap) g = cap;
    return (int)g;
}

template <typename S>
static int32_t convert_chunked(srx_ctx* ctx, hipStream_t stream, const char* tmp_tag, const void* host, void* d_dst,
                               uint64_t n, bool to_f32) {
    const uint64_t chunk = 32ull << 20;  // elements per staging chunk
    void* d_tmp;
    SRX_TRY(scratch(ctx, tmp_tag, (n < chunk ? n : chunk) * sizeof(S) + 16, &d_tmp));
    for (uint64_t off = 0; off < n; off += chunk) {
        uint64_t cnt = n - off < chunk ? n - off : chunk;
        SRX_HIP(ctx, hipMemcpy(d_tmp, (const S*)host + off, cnt * sizeof(S), hipMemcpyHostToDevice));
        int g = grid_for(cnt, 256, 4096);
        if (to_f32)
            hipLaunchKernelGGL((k_convert_values<S, float>), dim3(g), dim3(256), 0, stream,
                               (const S*)d_tmp, (float*)d_dst + off, cnt);
        else
            hipLaunchKernelGGL((k_convert_values<S, double>), dim3(g), dim3(256), 0, stream,
                               (const S*)d_tmp, (double*)d_dst + off, cnt);
        SRX_HIP(ctx, hipStreamSynchronize(stream));
    }
    return SRX_OK;
}

// f(T{}) with T the host type of `dtype`
template <typename F>
static int32_t by_dtype(srx_ctx* ctx, int32_t dtype, F&& f) {
    switch (dtype) {
        case SRX_I8:  return f(int8_t{});
        case SRX_I16: return f(int16_t{});
        case SRX_I32: return f(int32_t{});
        case SRX_U8:  return f(uint8_t{});
        case SRX_U16: return f(uint16_t{});
        case SRX_U32: return f(uint32_t{});
        case SRX_F32: return f(float{});
        case SRX_F64: return f(double{});
        default: return fail(ctx, SRX_E_DTYPE, "dtype %d is not supported for this operation", dtype);
    }
}

// ---- device buffers of a matrix ----------------------------------------------------------------------
// hipMalloc, or — while a backed session is open on the context — a recycled buffer of about the size (best fit among those
// at most a quarter larger; fresh buffers of 1 MiB and more get 3 % of headroom so that the next tile's slightly different
// size still fits).  The pool only holds what a session's tiles give back: it is capped (kPoolCapBytes, oldest buffers freed
// first), and when the device runs out of memory it is emptied and the allocation tried again.
constexpr size_t kPoolCapBytes = 24ull << 30;
static size_t pool_bytes(const srx_ctx* ctx) {
    size_t t = 0;
    for (auto& b : ctx->pool) t += b.second;
    return t;
}
hipError_t dev_malloc(srx_ctx* ctx, void** p, size_t bytes) {
    if (ctx->pool_on) {
        int best = -1;
        for (size_t i = 0; i < ctx->pool.size(); ++i) {
            const size_t cap = ctx->pool[i].second;
            if (cap >= bytes && cap <= bytes + bytes / 4 + (1u << 20) && (best < 0 || cap < ctx->pool[(size_t)best].second)) best = (int)i;
        }
        if (best >= 0) {
            *p = ctx->pool[(size_t)best].first;
            ctx->pool.erase(ctx->pool.begin() + best);
            return hipSuccess;
        }
    }
    const size_t want = (ctx->pool_on && bytes >= (1u << 20)) ? bytes + bytes / 32 + 65536 : bytes;
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess && !ctx->pool.empty()) {         // out of memory with recycled buffers parked: give them back, try again
        (void)hipGetLastError();
        pool_clear(ctx);
        e = hipMalloc(p, want);
    }
    return e;
}
static void dev_release(srx_mat* m, void* p) {
    if (!p) return;
    srx_ctx* ctx = m->ctx;
    size_t cap = 0;
    // recycled only while a session is open NOW (a matrix made during a session and freed after it frees its buffers)
    if (m->pooled && ctx && ctx->pool_on > 0 && hipMemPtrGetInfo(p, &cap) == hipSuccess && cap > 0) {
        ctx->pool.emplace_back(p, cap);
        while (ctx->pool.size() > 1 && pool_bytes(ctx) > kPoolCapBytes) {       // oldest first
            (void)hipFree(ctx->pool.front().first);
            ctx->pool.erase(ctx->pool.begin());
        }
    } else {
        (void)hipFree(p);
    }
}
void pool_clear(srx_ctx* ctx) {
    for (auto& b : ctx->pool) (void)hipFree(b.first);
    ctx->pool.clear();
}

static void free_mat_buffers(srx_mat* m) {
    if (!m) return;
    dev_release(m, m->d_indptr);
    dev_release(m, m->d_indices);
    dev_release(m, m->d_values);
    dev_release(m, m->d_tile_ptr);
    dev_release(m, m->d_idx16);
    dev_release(m, m->d_cnt);
    dev_release(m, m->d_cnt_pat);
    dev_release(m, m->d_sum);
    dev_release(m, m->d_sq);
    dev_release(m, m->d_row_sum);
    (void)hipFree(m->pca.d_scores);
}

static int32_t resolve_store(int32_t dtype, int32_t store) {
    if (store == SRX_STORE_F32 || store == SRX_STORE_F64) return store;
    switch (dtype) {
        case SRX_I32: case SRX_U32: case SRX_F64: return SRX_STORE_F64;
        default: return SRX_STORE_F32;
    }
}

// a buffer of its own (hipMalloc) holding a copy of the `bytes` at `src`, the copy queued on ctx->stream
template <typename T>
static hipError_t dup_buffer(srx_ctx* ctx, T** dst, const T* src, size_t bytes) {
    hipError_t e = hipMalloc((void**)dst, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(*dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream);
    return e;
}

// A change of m's value storage in two steps: a fresh buffer of `store` (nnz + 16 elements, hipMalloc, the padding not zeroed),
// and, once the caller has drained ctx->stream so that nothing reads the old values any more, the buffer made m's own.
static int32_t alloc_values(srx_mat* m, int32_t store, void** d_new) {
    SRX_HIP(m->ctx, hipMalloc(d_new, (m->nnz + 16) * (store == SRX_STORE_F32 ? sizeof(float) : sizeof(double))));
    return SRX_OK;
}
static void adopt_values(srx_mat* m, void* d_new, int32_t store) {
    (void)hipFree(m->d_values);
    m->d_values = d_new;
    m->store = store;
}

// Storage follows the reference's variant change: a matrix created with SRX_STORE_AUTO and held in f32 moves to f64 when
// an operation makes X a DynCsrMatrix::F64 (normalize_total on anything, log1p on a non-F32 matrix).  The values are
// widened exactly; everything derived from them stays valid.
int32_t promote_to_f64(srx_mat* m) {
    if (!m->store_auto || !is_f32(m)) return SRX_OK;
    srx_ctx* ctx = m->ctx;
    void* d_new = nullptr;
    SRX_TRY(alloc_values(m, SRX_STORE_F64, &d_new));
    const unsigned g = (unsigned)std::min<uint64_t>((m->nnz + 16 + 255) / 256, 65535);
    hipLaunchKernelGGL((k_convert_values<float, double>), dim3(g ? g : 1), dim3(256), 0, ctx->stream, (const float*)m->d_values,
                       (double*)d_new, m->nnz + 16);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(d_new);
        return fail(ctx, SRX_E_HIP, "promote_to_f64: conversion failed");
    }
    adopt_values(m, d_new, SRX_STORE_F64);
    return SRX_OK;
}

// H2D of a host CSR slice with the u64 -> i32 index narrowing, the value conversion and the canonical-CSR
// validation, every kernel on `stream`.  `h->indptr` may be a window of a larger row-offset array (a row tile of
// a backed matrix: indptr[0] != 0, indices / values pointing at the tile's first entry) — it is rebased on the
// device.  With a stream other than ctx->stream the staging buffers are separate ones, so a tile can be
// uploaded while the previous one is still being worked on.
int32_t upload_on(srx_ctx* ctx, const srx_csr* h, int32_t store, hipStream_t stream, srx_mat** out) {
    *out = nullptr;
    const bool side = stream != ctx->stream;
    const uint64_t base = h->indptr[0];
    if (h->indptr[h->n_rows] - base != h->nnz)
        return fail(ctx, SRX_E_FORMAT, "X is not a CSR matrix: row_offsets do not span nnz");
    // Every row offset is checked HERE, on the host, before anything on the device walks a row by them: the 16-bit upload path
    // (k_narrow16_tiles<WIDEN>) reads and writes indptr[r] .. indptr[r + 1] ahead of k_validate_rows, and a non-monotone or
    // out-of-range interior offset would send it outside the index arrays.  8 bytes per row: ~1 ms at 1.3M rows.
    {
        uint64_t bad = 0, prev = base;
        const uint64_t hi = base + h->nnz;
        for (uint64_t r = 1; r <= h->n_rows; ++r) {
            const uint64_t v = h->indptr[r];
            bad |= (uint64_t)(v < prev) | (uint64_t)(v > hi);
            prev = v;
        }
        if (bad) return fail(ctx, SRX_E_FORMAT, "X is not a CSR matrix: row_offsets are not monotone within [0, nnz]");
    }
    srx_mat* m = nullptr;
    SRX_TRY(srx_matrix_alloc(ctx, h->n_rows, h->n_cols, h->nnz, h->dtype, store, &m));
    bool direct_values = false;          // a DMA out of the caller's pinned values is in flight on ctx->direct_stream
    auto bail = [&](int32_t rc) {
        if (direct_values) (void)hipStreamSynchronize(ctx->direct_stream);
        srx_matrix_free(m);
        return rc;
    };
    hipError_t e = hipMemcpy(m->d_indptr, h->indptr, (h->n_rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(fail(ctx, SRX_E_HIP, "H2D indptr: %s", hipGetErrorString(e)));
    if (base)
        hipLaunchKernelGGL(k_rebase_indptr, dim3((unsigned)((h->n_rows + 256) / 256)), dim3(256), 0, stream, m->d_indptr,
                           h->n_rows + 1, (int64_t)base);

    int* d_flag;
    int32_t rc = scratch(ctx, side ? "flag_side" : "flag", 64, (void**)&d_flag);
    if (rc) return bail(rc);
    (void)hipMemsetAsync(d_flag, 0, sizeof(int), stream);

    // indices (u64 -> i32 on the way into the pinned staging buffers: 4 of the 8 bytes cross PCIe; with at most 65536 columns
    // u64 -> u16: 2 of the 8 — the 16-bit mirror the column passes walk arrives ready-made, and the 32-bit indices + the
    // gene-tile cuts of every row are made from it on the device, genes.hip) and, when the dtype is the storage type, the
    // values: the H2D workers, which also report a column index >= n_cols
    bool f32 = is_f32(m);
    const bool plain_values = (h->dtype == SRX_F32 && f32) || (h->dtype == SRX_F64 && !f32);
    if (h->nnz) {
        bool bad_col = false;
        // values the caller holds in PINNED memory (hipHostMalloc / hipHostRegister: a backed reader's tile buffers) need no
        // staging copy: one DMA straight out of them, under the workers' index narrowing
        if (plain_values && h->nnz * val_bytes(m) >= (8u << 20)) {
            // (first AND last byte: a registration that covers only a prefix of the array is not good enough; and if the copy
            //  cannot be queued all the same the values go through the staging workers like pageable ones — ADVICE r4)
            hipPointerAttribute_t at, at_end;
            const char* last = static_cast<const char*>(h->values) + h->nnz * val_bytes(m) - 1;
            if (hipPointerGetAttributes(&at, h->values) == hipSuccess && at.type == hipMemoryTypeHost &&
                hipPointerGetAttributes(&at_end, last) == hipSuccess && at_end.type == hipMemoryTypeHost) {
                if (!ctx->direct_stream) e = hipStreamCreateWithFlags(&ctx->direct_stream, hipStreamNonBlocking);
                if (e == hipSuccess)
                    e = hipMemcpyAsync(m->d_values, h->values, h->nnz * val_bytes(m), hipMemcpyHostToDevice, ctx->direct_stream);
                direct_values = e == hipSuccess;
                if (!direct_values) (void)hipGetLastError();
                e = hipSuccess;
            } else {
                (void)hipGetLastError();           // a plain pointer: not an error
            }
        }
        if (h->n_cols <= 65536) {
            e = dev_malloc(ctx, (void**)&m->d_idx16, (h->nnz + 16) * sizeof(uint16_t));
            if (e != hipSuccess) return bail(fail(ctx, SRX_E_HIP, "upload: %s", hipGetErrorString(e)));
            rc = parallel_h2d(ctx, h->indices, m->d_idx16, h->nnz, true, sizeof(uint16_t), h->n_cols, &bad_col);
            if (!rc && !bad_col) rc = tiles_from_idx16(m, stream);
        } else {
            rc = parallel_h2d(ctx, h->indices, m->d_indices, h->nnz, true, sizeof(int32_t), h->n_cols, &bad_col);
        }
        if (rc) return bail(rc);
        if (bad_col) return bail(fail(ctx, SRX_E_BOUNDS, "column index out of bounds (>= n_cols = %llu)",
                                      (unsigned long long)h->n_cols));
        bool staged_values = plain_values && !direct_values;
        if (direct_values) {
            e = hipStreamSynchronize(ctx->direct_stream);
            direct_values = false;
            if (e != hipSuccess) {                 // the DMA out of the caller's pages failed: the staging workers instead
                (void)hipGetLastError();
                staged_values = true;
            }
        }
        if (staged_values) {
            rc = parallel_h2d(ctx, h->values, m->d_values, h->nnz, false, val_bytes(m), 0, nullptr);
            if (rc) return bail(rc);
        }
    }
    if (!plain_values && h->nnz) {
        rc = by_dtype(ctx, h->dtype, [&](auto t) {
            return convert_chunked<decltype(t)>(ctx, stream, side ? "upload_tmp_side" : "upload_tmp", h->values, m->d_values, h->nnz, f32);
        });
        if (rc) return bail(rc);
    }
    // validate
    hipLaunchKernelGGL(k_validate_rows, dim3(grid_for(h->n_rows * kWave, 256, 8192)), dim3(256), 0, stream,
                       m->d_indptr, m->d_indices, h->n_rows, h->nnz, d_flag);
    int flag = 0;
    e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipMemcpy(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return bail(fail(ctx, SRX_E_HIP, "validate CSR: %s", hipGetErrorString(e)));
    if (flag & 2) return bail(fail(ctx, SRX_E_FORMAT, "X is not a canonical CSR matrix (unsorted/duplicate column indices)"));
    *out = m;
    return SRX_OK;
}

// ---- the one reduction over the stored values (common.hpp: value_scan): the largest finite |x| (the bit patterns of
// non-negative doubles order as integers), whether any value is NaN or Inf, whether any finite value is below zero
template <typename T>
__global__ __launch_bounds__(256) void k_value_scan(const T* __restrict__ vals, uint64_t nnz, unsigned long long* __restrict__ small) {
    unsigned long long mx = 0, flags = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const double v = (double)vals[i], a = fabs(v);
        if (a < INFINITY) {
            const unsigned long long b = (unsigned long long)__double_as_longlong(a);
            mx = b > mx ? b : mx;
            if (v < 0.0) flags |= kValNegative;
        } else {
            flags |= kValNonFinite;
        }
    }
    mx = wave_max(mx);
    flags = (__ballot((flags & kValNonFinite) != 0) ? kValNonFinite : 0ull) | (__ballot((flags & kValNegative) != 0) ? kValNegative : 0ull);
    // Both words only grow, so a wave that reads a value it cannot change skips its atomic: one atomic per wave on one
    // address is serialised (0.13 ms for the 16 workgroups per CU where every wave sent its maximum)
    if (lane_id() == 0) {
        if (mx > __hip_atomic_load(&small[VS_MAXABS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&small[VS_MAXABS], mx);
        if (flags & ~__hip_atomic_load(&small[VS_FLAGS], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(&small[VS_FLAGS], flags);
    }
}

void value_scan(srx_mat* m, unsigned long long* d_small) {
    if (!m->nnz) return;
    const unsigned grid = (unsigned)std::min<uint64_t>((m->nnz + 255) / 256, (uint64_t)m->ctx->n_cus * 16);
    if (is_f32(m)) hipLaunchKernelGGL(k_value_scan<float>, dim3(grid), dim3(256), 0, m->ctx->stream, (const float*)m->d_values, m->nnz, d_small);
    else hipLaunchKernelGGL(k_value_scan<double>, dim3(grid), dim3(256), 0, m->ctx->stream, (const double*)m->d_values, m->nnz, d_small);
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_matrix_alloc(srx_ctx* ctx, uint64_t n_rows, uint64_t n_cols, uint64_t nnz,
                         int32_t dtype, int32_t store, srx_mat** out) {
    if (!ctx || !out) return fail(ctx, SRX_E_ARG, "srx_matrix_alloc: null argument");
    *out = nullptr;
    if (dtype < SRX_I8 || dtype > SRX_F64)
        return fail(ctx, SRX_E_DTYPE, "dtype %d is not supported for this operation", dtype);
    if (n_cols >= (1ull << 31)) return fail(ctx, SRX_E_BOUNDS, "n_cols %llu exceeds int32 device indices",
                                            (unsigned long long)n_cols);
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    srx_mat* m = new srx_mat();
    m->ctx = ctx;
    m->n_rows = n_rows; m->n_cols = n_cols; m->nnz = nnz;
    m->dtype = dtype;
    m->store = resolve_store(dtype, store);
    m->store_auto = store == SRX_STORE_AUTO;
    m->n_rows_global = n_rows;
    m->pooled = ctx->pool_on > 0;
    hipError_t e;
    e = dev_malloc(ctx, (void**)&m->d_indptr, (n_rows + 1) * sizeof(int64_t));
    // +16 elements: the streaming kernels read 16-byte vectors that may run past a row's last entry
    if (e == hipSuccess) e = dev_malloc(ctx, (void**)&m->d_indices, (nnz + 16) * sizeof(int32_t));
    if (e == hipSuccess) e = dev_malloc(ctx, &m->d_values, (nnz + 16) * val_bytes(m));
    if (e == hipSuccess) e = hipMemsetAsync(m->d_indices + nnz, 0, 16 * sizeof(int32_t), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync((char*)m->d_values + nnz * val_bytes(m), 0, 16 * val_bytes(m), ctx->stream);
    if (e != hipSuccess) {
        free_mat_buffers(m);
        delete m;
        return fail(ctx, e == hipErrorOutOfMemory ? SRX_E_OOM : SRX_E_HIP, "hipMalloc for CSR failed: %s",
                    hipGetErrorString(e));
    }
    *out = m;
    return SRX_OK;
}

int32_t srx_matrix_upload(srx_ctx* ctx, const srx_csr* h, int32_t store, srx_mat** out) {
    if (!ctx || !h || !out) return fail(ctx, SRX_E_ARG, "srx_matrix_upload: null argument");
    *out = nullptr;
    if (!h->indptr || (h->nnz && (!h->indices || !h->values)))
        return fail(ctx, SRX_E_ARG, "srx_matrix_upload: null CSR slice");
    // (a whole matrix, not a window of one; that the offsets span nnz is upload_on's check)
    if (h->indptr[0] != 0) return fail(ctx, SRX_E_FORMAT, "X is not a CSR matrix: row_offsets do not span nnz");
    return upload_on(ctx, h, store, ctx->stream, out);
}

int32_t srx_matrix_device_ptrs(srx_mat* m, void** indptr, void** indices, void** values) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    if (indptr) *indptr = m->d_indptr;
    if (indices) *indices = m->d_indices;
    if (values) *values = m->d_values;
    touch(m);  // the caller may write through these pointers
    m->moments_version = 0;
    if (m->d_tile_ptr) { (void)hipFree(m->d_tile_ptr); m->d_tile_ptr = nullptr; }
    if (m->d_idx16) { (void)hipFree(m->d_idx16); m->d_idx16 = nullptr; }
    m->n_tiles = 0;
    m->cnt_pat_valid = false;
    return SRX_OK;
}

int32_t srx_matrix_info(const srx_mat* m, srx_mat_info* out) {
    if (!m || !out) return fail(nullptr, SRX_E_ARG, "null argument");
    out->n_rows = m->csc ? m->n_cols : m->n_rows;      // the shape of X, whatever the storage
    out->n_cols = m->csc ? m->n_rows : m->n_cols;
    out->nnz = m->nnz;
    out->dtype = m->dtype; out->store = m->store;
    out->row_offset = m->row_offset;
    out->n_rows_global = m->n_rows_global;
    return SRX_OK;
}

int32_t srx_matrix_set_shard(srx_mat* m, uint64_t row_offset) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    m->row_offset = row_offset;
    return SRX_OK;
}

int32_t srx_matrix_download_values(srx_mat* m, void* out, int32_t dtype_out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    srx_ctx* ctx = m->ctx;
    if (dtype_out != SRX_F32 && dtype_out != SRX_F64)
        return fail(ctx, SRX_E_DTYPE, "values can be fetched as F32 or F64 only");
    SRX_HIP(ctx, hipSetDevice(ctx->device));
    bool same = (dtype_out == SRX_F32) == is_f32(m);
    if (same) return d2h(ctx, out, m->d_values, m->nnz * val_bytes(m));
    void* d_tmp;
    size_t ob = dtype_out == SRX_F32 ? 4 : 8;
    SRX_TRY(scratch(ctx, "download_tmp", (m->nnz ? m->nnz : 1) * ob, &d_tmp));
    int g = grid_for(m->nnz, 256, 4096);
    if (is_f32(m))
        hipLaunchKernelGGL((k_convert_values<float, double>), dim3(g), dim3(256), 0, ctx->stream,
                           (const float*)m->d_values, (double*)d_tmp, m->nnz);
    else
        hipLaunchKernelGGL((k_convert_values<double, float>), dim3(g), dim3(256), 0, ctx->stream,
                           (const double*)m->d_values, (float*)d_tmp, m->nnz);
    return d2h(ctx, out, d_tmp, m->nnz * ob);
}

int32_t srx_matrix_clone(srx_mat* m, srx_mat** out) {
    if (!m || !out) return fail(m ? m->ctx : nullptr, SRX_E_ARG, "null argument");
    srx_ctx* ctx = m->ctx;
    srx_mat* c = nullptr;
    SRX_TRY(srx_matrix_alloc(ctx, m->n_rows, m->n_cols, m->nnz, m->dtype, m->store, &c));
    c->row_offset = m->row_offset;
    c->csc = m->csc;
    c->store_auto = m->store_auto;
    hipError_t e = hipMemcpyAsync(c->d_indptr, m->d_indptr, (m->n_rows + 1) * sizeof(int64_t),
                                  hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_indices, m->d_indices, m->nnz * sizeof(int32_t),
                                            hipMemcpyDeviceToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->d_values, m->d_values, m->nnz * val_bytes(m),
                                            hipMemcpyDeviceToDevice, ctx->stream);
    // pattern-only index structure (gene-tile cuts of every row) travels with the pattern
    if (e == hipSuccess && m->n_tiles > 0) {
        c->n_tiles = m->n_tiles;
        c->tile_genes = m->tile_genes;
        if (m->d_tile_ptr)
            e = dup_buffer(ctx, &c->d_tile_ptr, m->d_tile_ptr, (size_t)(m->n_tiles - 1) * (m->n_rows ? m->n_rows : 1) * sizeof(int64_t));
        if (e == hipSuccess && m->d_idx16) e = dup_buffer(ctx, &c->d_idx16, m->d_idx16, (m->nnz + 16) * sizeof(uint16_t));
    }
    if (e == hipSuccess && m->cnt_pat_valid && m->d_cnt_pat) {          // pattern-only per-gene counts
        e = dup_buffer(ctx, &c->d_cnt_pat, m->d_cnt_pat, (m->n_cols ? m->n_cols : 1) * sizeof(uint32_t));
        c->cnt_pat_valid = e == hipSuccess;
    }
    // a reserved result block (srx_matrix_reserve_results) is part of the handle's layout: the clone gets its own
    if (e == hipSuccess && m->pca.scores_cap > 0) {
        e = hipMalloc((void**)&c->pca.d_scores, m->pca.scores_cap);
        if (e == hipSuccess) c->pca.scores_cap = m->pca.scores_cap;
        // ... and so is the per-cell sum buffer of the pipeline's first pass (8 bytes per cell: a hipMalloc of it inside the
        // step showed as 0.25 ms outside every kernel)
        if (e == hipSuccess && !c->d_row_sum) e = hipMalloc((void**)&c->d_row_sum, (c->n_rows ? c->n_rows : 1) * sizeof(double));
    }
    if (e != hipSuccess) {
        srx_matrix_free(c);
        return fail(ctx, SRX_E_HIP, "clone D2D: %s", hipGetErrorString(e));
    }
    *out = c;
    return SRX_OK;
}

int32_t srx_matrix_prepare(srx_mat* m) {
    if (!m) return fail(nullptr, SRX_E_ARG, "null matrix");
    SRX_HIP(m->ctx, hipSetDevice(m->ctx->device));
    SRX_TRY(ensure_tiles(m));
    return m->csc ? SRX_OK : ensure_pattern_counts(m);
}

int32_t srx_matrix_copy_values(srx_mat* dst, const srx_mat* src) {
    if (!dst || !src) return fail(nullptr, SRX_E_ARG, "null argument");
    srx_ctx* ctx = dst->ctx;
    if (dst->nnz != src->nnz || dst->n_rows != src->n_rows)
        return fail(ctx, SRX_E_ARG, "copy_values: pattern mismatch");
    if (dst->store != src->store) {
        // a SRX_STORE_AUTO work copy that normalize_total / log1p / srx_pipeline promoted to f64 being restored from its
        // pristine f32 source (or the other way round): the value buffer follows the source's storage again
        if (!dst->store_auto) return fail(ctx, SRX_E_ARG, "copy_values: storage mismatch (explicit storage on the destination)");
        // (an allocation, a stream drain and a free per call: steady-state loops that restore a work copy every step should
        //  create it with an explicit SRX_STORE_F32 / SRX_STORE_F64 — then this branch is never taken)
        void* d_new = nullptr;
        SRX_TRY(alloc_values(dst, src->store, &d_new));
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        if (es != hipSuccess) {
            (void)hipFree(d_new);
            return fail(ctx, SRX_E_HIP, "copy_values: %s", hipGetErrorString(es));
        }
        adopt_values(dst, d_new, src->store);
        SRX_HIP(ctx, hipMemsetAsync((char*)dst->d_values + src->nnz * val_bytes(src), 0, 16 * val_bytes(src), ctx->stream));
    }
    SRX_HIP(ctx, hipMemcpyAsync(dst->d_values, src->d_values, src->nnz * val_bytes(src),
                                hipMemcpyDeviceToDevice, ctx->stream));
    dst->dtype = src->dtype;
    touch(dst);
    return SRX_OK;
}

void srx_matrix_free(srx_mat* m) {
    if (!m) return;
    if (m->ctx) {
        (void)hipSetDevice(m->ctx->device);
        (void)hipStreamSynchronize(m->ctx->stream);
    }
    free_mat_buffers(m);
    delete m;
}

}  // extern "C"
