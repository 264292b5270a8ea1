// ctx.hip — context, scratch memory, error and profiling plumbing of libsrx_hip.so.
#include "common.hpp"

#include <dlfcn.h>

namespace srx {

thread_local std::string g_tls_err;

int32_t scratch(srx_ctx* ctx, const char* name, size_t bytes, void** out) {
    auto& s = ctx->scratch[name];
    if (s.bytes < bytes) {
        if (s.p) SRX_HIP(ctx, hipFree(s.p));
        s.p = nullptr;
        s.bytes = 0;
        size_t want = bytes + bytes / 8 + 256;
        SRX_HIP(ctx, hipMalloc(&s.p, want));
        s.bytes = want;
    }
    *out = s.p;
    return SRX_OK;
}

// ---- roctx ---------------------------------------------------------------------------------------
namespace {
typedef int (*roctx_push_fn)(const char*);
typedef int (*roctx_pop_fn)(void);
struct Roctx {
    roctx_push_fn push = nullptr;
    roctx_pop_fn pop = nullptr;
    Roctx() {
        if (getenv("SRX_NO_ROCTX")) return;
        void* h = nullptr;
        for (const char* n : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (h) break;
        }
        if (!h) return;
        push = (roctx_push_fn)dlsym(h, "roctxRangePushA");
        pop = (roctx_pop_fn)dlsym(h, "roctxRangePop");
        if (!push || !pop) push = nullptr, pop = nullptr;
    }
};
Roctx& roctx() {
    static Roctx r;
    return r;
}
}  // namespace
Range::Range(const char* name) : on(false) {
    Roctx& r = roctx();
    if (r.push) {
        r.push(name);
        on = true;
    }
}
Range::~Range() {
    if (on) roctx().pop();
}

// ---- profiling -------------------------------------------------------------------------------
static hipEvent_t take_event(srx_ctx* ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

ProfScope::ProfScope(srx_ctx* c, int cls_, double alg_bytes, hipStream_t stream_, double aux_bytes) : ctx(c), cls(cls_), stream(stream_ ? stream_ : c->stream) {
    if (!(ctx->prof_mask & (1u << cls)) || ctx->capturing) return;      // no event nodes inside a captured graph
    e0 = take_event(ctx);
    e1 = take_event(ctx);
    if (!e0 || !e1) { e0 = e1 = nullptr; return; }
    ctx->prof[cls].bytes += alg_bytes;
    ctx->prof[cls].aux_bytes += aux_bytes;
    ctx->prof[cls].launches += 1;
    (void)hipEventRecord(e0, stream);
}
ProfScope::~ProfScope() {
    if (!e0) return;
    (void)hipEventRecord(e1, stream);
    ctx->prof[cls].pending.emplace_back(e0, e1);
}

int32_t StreamTimer::start() {
    SRX_HIP(ctx, hipEventCreate(&e0));
    SRX_HIP(ctx, hipEventCreate(&e1));
    SRX_HIP(ctx, hipEventRecord(e0, stream));
    started = true;
    return SRX_OK;
}
StreamTimer::~StreamTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
}
int32_t StreamTimer::stop(double* ms) {
    if (!started) return fail(ctx, SRX_E_HIP, "StreamTimer: stop() without start()");
    SRX_HIP(ctx, hipEventRecord(e1, stream));
    SRX_HIP(ctx, hipEventSynchronize(e1));
    float f = 0.f;
    SRX_HIP(ctx, hipEventElapsedTime(&f, e0, e1));
    *ms = (double)f;
    return SRX_OK;
}

static int32_t prof_drain(srx_ctx* ctx) {
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->comm_stream) SRX_HIP(ctx, hipStreamSynchronize(ctx->comm_stream));
    if (ctx->gram_stream) SRX_HIP(ctx, hipStreamSynchronize(ctx->gram_stream));
    for (int c = 0; c < SRX_K_COUNT_; ++c) {
        for (auto& pr : ctx->prof[c].pending) {
            float ms = 0.f;
            SRX_HIP(ctx, hipEventElapsedTime(&ms, pr.first, pr.second));
            ctx->prof[c].ms += ms;
            ctx->event_pool.push_back(pr.first);
            ctx->event_pool.push_back(pr.second);
        }
        ctx->prof[c].pending.clear();
    }
    return SRX_OK;
}

}  // namespace srx

using namespace srx;

extern "C" {

int32_t srx_abi_version(void) { return SRX_ABI_VERSION; }

int32_t srx_device_count(int32_t* n_out) {
    if (!n_out) return fail(nullptr, SRX_E_ARG, "srx_device_count: null output");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *n_out = 0;
        return fail(nullptr, SRX_E_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    *n_out = n;
    return SRX_OK;
}

int32_t srx_ctx_create(int32_t device_id, srx_ctx** out) {
    if (!out) return fail(nullptr, SRX_E_ARG, "srx_ctx_create: null output");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, SRX_E_HIP, "no HIP device available (%s); libsrx_hip has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, SRX_E_ARG, "device_id %d out of range [0,%d)", device_id, n);
    srx_ctx* ctx = new srx_ctx();
    ctx->device = device_id;
    hipDeviceProp_t prop;
    e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;                                  // nothing else is owned yet
        return fail(nullptr, SRX_E_HIP, "srx_ctx_create: %s", hipGetErrorString(e));
    }
    ctx->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = ctx;
    return SRX_OK;
}

void srx_ctx_destroy(srx_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    srx_comm_destroy(ctx);
    for (auto& kv : ctx->scratch) (void)hipFree(kv.second.p);
    pool_clear(ctx);
    for (int c = 0; c < SRX_K_COUNT_; ++c)
        for (auto& pr : ctx->prof[c].pending) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    for (auto& kv : ctx->graphs) (void)hipGraphExecDestroy(kv.second);
    if (ctx->pin_async) (void)hipHostFree(ctx->pin_async);
    transfer_destroy(ctx);
    if (ctx->d_gram_mode) (void)hipFree(ctx->d_gram_mode);
    for (auto e : ctx->async_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    if (ctx->comm_fork) (void)hipEventDestroy(ctx->comm_fork);
    if (ctx->comm_join) (void)hipEventDestroy(ctx->comm_join);
    if (ctx->gram_stream) (void)hipStreamDestroy(ctx->gram_stream);
    if (ctx->gram_fork) (void)hipEventDestroy(ctx->gram_fork);
    if (ctx->gram_join) (void)hipEventDestroy(ctx->gram_join);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int32_t srx_ctx_synchronize(srx_ctx* ctx) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    SRX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SRX_OK;
}

const char* srx_last_error(const srx_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    return g_tls_err.c_str();
}

int32_t srx_partition_rows(const uint64_t* indptr, uint64_t n_rows, int32_t n_ranks,
                           uint64_t* cut_out) {
    if (!indptr || !cut_out || n_ranks < 1) return fail(nullptr, SRX_E_ARG, "srx_partition_rows: bad args");
    // cut[r] = first row whose start offset reaches r/n_ranks of the non-zeros (binary search
    // on indptr): balances bytes walked per GPU, not row counts.
    uint64_t base = indptr[0], nnz = indptr[n_rows] - base;
    cut_out[0] = 0;
    for (int r = 1; r < n_ranks; ++r) {
        uint64_t target = base + (uint64_t)(((__uint128_t)nnz * (unsigned)r) / (unsigned)n_ranks);
        uint64_t lo = cut_out[r - 1], hi = n_rows;
        while (lo < hi) {
            uint64_t mid = lo + (hi - lo) / 2;
            if (indptr[mid] < target) lo = mid + 1; else hi = mid;
        }
        cut_out[r] = lo;
    }
    cut_out[n_ranks] = n_rows;
    return SRX_OK;
}

int32_t srx_prof_enable(srx_ctx* ctx, uint32_t class_mask) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    ctx->prof_mask = class_mask;
    return SRX_OK;
}

int32_t srx_prof_reset(srx_ctx* ctx) {
    if (!ctx) return fail(nullptr, SRX_E_ARG, "null ctx");
    SRX_TRY(prof_drain(ctx));
    for (int c = 0; c < SRX_K_COUNT_; ++c) {
        ctx->prof[c].ms = 0.0;
        ctx->prof[c].launches = 0;
        ctx->prof[c].bytes = 0.0;
        ctx->prof[c].aux_bytes = 0.0;
    }
    return SRX_OK;
}

int32_t srx_prof_get(srx_ctx* ctx, int32_t cls, double* total_ms, uint64_t* launches, double* bytes) {
    if (!ctx || cls < 0 || cls >= SRX_K_COUNT_) return fail(ctx, SRX_E_ARG, "bad kernel class");
    SRX_TRY(prof_drain(ctx));
    if (total_ms) *total_ms = ctx->prof[cls].ms;
    if (launches) *launches = ctx->prof[cls].launches;
    if (bytes) *bytes = ctx->prof[cls].bytes;
    return SRX_OK;
}

int32_t srx_prof_get_aux(srx_ctx* ctx, int32_t cls, double* aux_bytes) {
    if (!ctx || cls < 0 || cls >= SRX_K_COUNT_) return fail(ctx, SRX_E_ARG, "bad kernel class");
    if (aux_bytes) *aux_bytes = ctx->prof[cls].aux_bytes;
    return SRX_OK;
}

}  // extern "C"
