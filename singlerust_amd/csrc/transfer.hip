// transfer.hip — host <-> device copies of libsrx_hip.so: the small staged ones on the context's stream and the transfer
// workers (several pinned double-buffer pipelines side by side) that move whole arrays.
#include "common.hpp"

#include <algorithm>
#include <atomic>
#include <thread>

namespace srx {

int32_t pinned(srx_ctx* ctx, size_t bytes, void** out) {
    if (ctx->pinned_bytes < bytes) {
        if (ctx->pinned) SRX_HIP(ctx, hipHostFree(ctx->pinned));
        ctx->pinned = nullptr;
        ctx->pinned_bytes = 0;
        size_t want = bytes < (1u << 20) ? (1u << 20) : bytes + bytes / 4;
        SRX_HIP(ctx, hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault));
        ctx->pinned_bytes = want;
    }
    *out = ctx->pinned;
    return SRX_OK;
}

static int32_t parallel_d2h(srx_ctx* ctx, void* dst, const void* src, size_t bytes);
static int32_t parallel_d2h_rows(srx_ctx* ctx, void* dst, const void* src, uint64_t rows, size_t width, size_t dev_pitch);

// Small/medium blocks go through the pinned staging buffer so the copy is a true async DMA
// ordered on the ctx stream; large blocks (values of the whole matrix, the score matrix) go through the
// transfer workers (several pinned double-buffer pipelines side by side).
int32_t d2h(srx_ctx* ctx, void* host, const void* dev, size_t bytes) {
    if (bytes == 0) return SRX_OK;
    if (bytes <= (64u << 20)) {
        void* p;
        SRX_TRY(pinned(ctx, bytes, &p));
        SRX_HIP(ctx, hipMemcpyAsync(p, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(host, p, bytes);
    } else {
        SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SRX_TRY(parallel_d2h(ctx, host, dev, bytes));
    }
    return SRX_OK;
}

// A small read-back the host waits for while the stream goes on.  Its own pinned slot (it used to stage through
// ctx->pinned, which any d2h() in between overwrites and any larger pinned() request frees) and a pending flag: one at a time.
constexpr size_t kSplitReadBytes = 256;
int32_t d2h_begin(srx_ctx* ctx, const void* dev, size_t bytes) {
    if (bytes > kSplitReadBytes) return fail(ctx, SRX_E_ARG, "d2h_begin: %zu bytes exceed the split read-back slot", bytes);
    if (ctx->d2h_pending) {              // (an error return between a begin and its end: the abandoned copy is waited out)
        SRX_HIP(ctx, hipEventSynchronize(ctx->d2h_ev));
        ctx->d2h_pending = false;
    }
    if (!ctx->pin_d2h) SRX_HIP(ctx, hipHostMalloc(&ctx->pin_d2h, kSplitReadBytes));
    if (!ctx->d2h_ev) SRX_HIP(ctx, hipEventCreateWithFlags(&ctx->d2h_ev, hipEventDisableTiming));
    SRX_HIP(ctx, hipMemcpyAsync(ctx->pin_d2h, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    SRX_HIP(ctx, hipEventRecord(ctx->d2h_ev, ctx->stream));
    ctx->d2h_pending = true;
    return SRX_OK;
}
int32_t d2h_end(srx_ctx* ctx, void* host, size_t bytes) {
    if (!ctx->d2h_pending) return fail(ctx, SRX_E_ARG, "d2h_end without d2h_begin");
    ctx->d2h_pending = false;
    SRX_HIP(ctx, hipEventSynchronize(ctx->d2h_ev));
    memcpy(host, ctx->pin_d2h, bytes);
    return SRX_OK;
}

// `rows` rows of `width` bytes, `dev_pitch` bytes apart on the device, to a dense host matrix
int32_t d2h_rows(srx_ctx* ctx, void* host, const void* dev, uint64_t rows, size_t width, size_t dev_pitch) {
    if (dev_pitch == width) return d2h(ctx, host, dev, rows * width);
    if (rows == 0 || width == 0) return SRX_OK;
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return parallel_d2h_rows(ctx, host, dev, rows, width, dev_pitch);
}

int32_t h2d(srx_ctx* ctx, void* dev, const void* host, size_t bytes) {
    if (bytes == 0) return SRX_OK;
    if (bytes <= (64u << 20)) {
        void* p;
        // the staging buffer may still feed an earlier async copy
        SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SRX_TRY(pinned(ctx, bytes, &p));
        memcpy(p, host, bytes);
        SRX_HIP(ctx, hipMemcpyAsync(dev, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
        SRX_TRY(parallel_h2d(ctx, host, dev, bytes, false, 1, 0, nullptr));
    }
    return SRX_OK;
}

// ---- the transfer workers ----------------------------------------------------------------------------------
// A pageable hipMemcpy moves ~26-31 GB/s on this box: one thread copies into the runtime's staging buffer while the
// DMA engine waits.  Here kUpWorkers (8; SRX_UP_WORKERS) threads each take a contiguous share of the array and run their own two-buffer
// pipeline (fill a pinned buffer — narrowing u64 indices to i32 and bounds-checking them on the way, so only half
// the index bytes cross PCIe — then hipMemcpyAsync on the worker's stream while the other buffer is being filled).
static const int kUpWorkers = [] {
    const char* e = getenv("SRX_UP_WORKERS");          // tuning switch
    const int v = e ? atoi(e) : 8;                   // 4: 40, 8: 55, 16: 39-50, 32: 33 GB/s of host data (400k x 20k matrix)
    return v < 1 ? 1 : v > 64 ? 64 : v;
}();
constexpr size_t kUpChunkBytes = 4u << 20;          // per staging buffer (pinned: workers x 2 x 4 MiB)

static int32_t ensure_up_workers(srx_ctx* ctx) {
    if (!ctx->up_workers.empty()) return SRX_OK;
    std::vector<srx_ctx::UpWorker> ws(kUpWorkers);
    for (auto& w : ws) {
        SRX_HIP(ctx, hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
        for (int b = 0; b < 2; ++b) {
            SRX_HIP(ctx, hipHostMalloc(&w.pin[b], kUpChunkBytes, hipHostMallocDefault));
            SRX_HIP(ctx, hipEventCreateWithFlags(&w.ev[b], hipEventDisableTiming));
        }
    }
    ctx->up_workers = std::move(ws);
    return SRX_OK;
}

// The frame of every worker transfer.  `n` units that move `per_chunk` to a staging buffer are split into contiguous shares
// (rounded up to `align` units, a power of two), one per worker, worker 0 on the calling thread; body(w, u0, u1) moves
// units [u0, u1) with worker w's stream, buffers and events and returns its first HIP error.  `dir` names the direction in the
// message of the first worker that failed.
template <typename Body>
static int32_t run_workers(srx_ctx* ctx, const char* dir, uint64_t n, uint64_t per_chunk, uint64_t align, Body&& body) {
    if (n == 0) return SRX_OK;
    SRX_TRY(ensure_up_workers(ctx));
    const int device = ctx->device;
    // small arrays: fewer workers (a share should be worth a thread)
    int nw = (int)std::min<uint64_t>(kUpWorkers, (n + per_chunk - 1) / per_chunk);
    if (nw < 1) nw = 1;
    const uint64_t share = ((n + nw - 1) / nw + align - 1) & ~(align - 1);
    std::vector<hipError_t> err(nw, hipSuccess);
    auto run = [&](int t) {
        hipError_t e = hipSetDevice(device);
        const uint64_t u0 = std::min<uint64_t>(n, (uint64_t)t * share), u1 = std::min<uint64_t>(n, u0 + share);
        if (e == hipSuccess) e = body(ctx->up_workers[t], u0, u1);
        err[t] = e;
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nw; ++t) th.emplace_back(run, t);
    run(0);
    for (auto& x : th) x.join();
    for (int t = 0; t < nw; ++t)
        if (err[t] != hipSuccess) return fail(ctx, SRX_E_HIP, "%s worker %d: %s", dir, t, hipGetErrorString(err[t]));
    return SRX_OK;
}

// u64 -> D on the way into a staging buffer; true if a value was >= n_cols
template <typename D>
static bool narrow_into(void* pin, const uint64_t* s, uint64_t cnt, uint64_t n_cols) {
    D* d = static_cast<D*>(pin);
    uint64_t over = 0;
    for (uint64_t i = 0; i < cnt; ++i) {
        const uint64_t v = s[i];
        over |= (uint64_t)(v >= n_cols);
        d[i] = (D)v;
    }
    return over != 0;
}

// `n` elements from host `src` to device `dst`.  narrow: src is u64[n], dst i32[n] (elem_bytes 4) or u16[n] (elem_bytes 2),
// values >= n_cols set *bad; otherwise a plain copy of n * elem_bytes bytes.
int32_t parallel_h2d(srx_ctx* ctx, const void* src, void* dst, uint64_t n, bool narrow, size_t elem_bytes, uint64_t n_cols,
                     bool* bad) {
    const uint64_t per_chunk = kUpChunkBytes / elem_bytes;
    std::atomic<bool> any_over{false};
    SRX_TRY(run_workers(ctx, "H2D", n, per_chunk, 16, [&](srx_ctx::UpWorker& w, uint64_t e0, uint64_t e1) {
        hipError_t e = hipSuccess;
        int buf = 0;
        bool used[2] = {false, false};
        bool over = false;
        for (uint64_t off = e0; off < e1 && e == hipSuccess; off += per_chunk, buf ^= 1) {
            const uint64_t cnt = std::min<uint64_t>(per_chunk, e1 - off);
            if (used[buf]) e = hipEventSynchronize(w.ev[buf]);          // the DMA out of this buffer has finished
            if (e != hipSuccess) break;
            if (narrow && elem_bytes == sizeof(uint16_t))
                over |= narrow_into<uint16_t>(w.pin[buf], static_cast<const uint64_t*>(src) + off, cnt, n_cols);
            else if (narrow)
                over |= narrow_into<int32_t>(w.pin[buf], static_cast<const uint64_t*>(src) + off, cnt, n_cols);
            else
                memcpy(w.pin[buf], static_cast<const char*>(src) + off * elem_bytes, cnt * elem_bytes);
            e = hipMemcpyAsync(static_cast<char*>(dst) + off * elem_bytes, w.pin[buf], cnt * elem_bytes, hipMemcpyHostToDevice,
                               w.stream);
            if (e == hipSuccess) e = hipEventRecord(w.ev[buf], w.stream);
            used[buf] = true;
        }
        if (e == hipSuccess) e = hipStreamSynchronize(w.stream);
        if (over) any_over = true;
        return e;
    }));
    if (bad && any_over) *bad = true;
    return SRX_OK;
}

// One worker's share of a D2H transfer, units [u0, u1) of `unit` bytes that lie dense in `dst`: issue(pin, off, cnt) queues the
// DMA of `cnt` units from unit `off` on into a staging buffer; chunk c is DMAed into buffer c & 1 while chunk c - 1 is copied
// out of the other one.
template <typename Issue>
static hipError_t d2h_share(srx_ctx::UpWorker& w, void* dst, uint64_t u0, uint64_t u1, uint64_t per_chunk, size_t unit,
                            Issue&& issue) {
    hipError_t e = hipSuccess;
    uint64_t prev_off = 0, prev_cnt = 0;
    int buf = 0;
    auto copy_out_prev = [&] {
        if (!prev_cnt || e != hipSuccess) return;
        e = hipEventSynchronize(w.ev[buf ^ 1]);
        if (e == hipSuccess) memcpy(static_cast<char*>(dst) + prev_off * unit, w.pin[buf ^ 1], prev_cnt * unit);
    };
    for (uint64_t off = u0; off < u1 && e == hipSuccess; off += per_chunk, buf ^= 1) {
        const uint64_t cnt = std::min<uint64_t>(per_chunk, u1 - off);
        e = issue(w.pin[buf], off, cnt);
        if (e == hipSuccess) e = hipEventRecord(w.ev[buf], w.stream);
        copy_out_prev();
        prev_off = off;
        prev_cnt = cnt;
    }
    copy_out_prev();
    return e;
}

// the same in the other direction: DMA into a pinned buffer, then a memcpy out of it while the next DMA runs
static int32_t parallel_d2h(srx_ctx* ctx, void* dst, const void* src, size_t bytes) {
    return run_workers(ctx, "D2H", bytes, kUpChunkBytes, 256, [&](srx_ctx::UpWorker& w, uint64_t b0, uint64_t b1) {
        return d2h_share(w, dst, b0, b1, kUpChunkBytes, 1, [&](void* pin, uint64_t off, uint64_t cnt) {
            return hipMemcpyAsync(pin, static_cast<const char*>(src) + off, cnt, hipMemcpyDeviceToHost, w.stream);
        });
    });
}

// ... and of `rows` rows of `width` bytes that lie `dev_pitch` bytes apart on the device (the score rows, padded to whole
// 128-byte pieces) into a dense host matrix: the workers take row ranges, the DMA engine does the strided read
// (hipMemcpy2DAsync into the dense pinned buffer), the memcpy out of the other buffer runs under it.
static int32_t parallel_d2h_rows(srx_ctx* ctx, void* dst, const void* src, uint64_t rows, size_t width, size_t dev_pitch) {
    if (rows == 0 || width == 0) return SRX_OK;
    if (width > kUpChunkBytes) return fail(ctx, SRX_E_ARG, "D2H: a row of %zu bytes exceeds the staging buffers", width);
    const uint64_t per_chunk = kUpChunkBytes / width;                   // rows per staging buffer
    return run_workers(ctx, "D2H", rows, per_chunk, 1, [&](srx_ctx::UpWorker& w, uint64_t r0, uint64_t r1) {
        return d2h_share(w, dst, r0, r1, per_chunk, width, [&](void* pin, uint64_t r, uint64_t cnt) {
            return hipMemcpy2DAsync(pin, width, static_cast<const char*>(src) + r * dev_pitch, dev_pitch, width, cnt,
                                    hipMemcpyDeviceToHost, w.stream);
        });
    });
}

// what this file owns in the context (srx_ctx_destroy, after the stream has been drained)
void transfer_destroy(srx_ctx* ctx) {
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    for (auto& uw : ctx->up_workers) {
        for (int b = 0; b < 2; ++b) {
            if (uw.pin[b]) (void)hipHostFree(uw.pin[b]);
            if (uw.ev[b]) (void)hipEventDestroy(uw.ev[b]);
        }
        if (uw.stream) (void)hipStreamDestroy(uw.stream);
    }
    if (ctx->direct_stream) (void)hipStreamDestroy(ctx->direct_stream);
    if (ctx->d2h_ev) (void)hipEventDestroy(ctx->d2h_ev);
    if (ctx->pin_d2h) (void)hipHostFree(ctx->pin_d2h);
}

}  // namespace srx
