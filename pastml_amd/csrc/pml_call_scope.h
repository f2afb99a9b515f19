// What a C-ABI entry that owns device memory for the length of one call shares with the others: the scope of its scratch and
// events and of the copies to the caller, the rule for the columns of a chunk, the upload of the altered flags.
//
// THE RULE: a call's scratch and events live in one CallScope, which synchronises the stream before it frees.  Host buffers
// that the call's asynchronous copies read or write are declared BEFORE the scope, so that this synchronisation runs while
// they are alive -- on every path out of the function, an early PML_TRY / HIP_TRY return included.
//
// Nothing of HIP is included here: pml_host.h includes this header below the context, with the HIP runtime, fail, HIP_TRY and
// PML_TRY in sight; a host test supplies stand-ins for those names and a context of its own (tests/call_scope_driver.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

class CallScope {
    hipStream_t s_;
    bool events_on_;
    bool waited_ = false;   // finish() has run and nothing went through the scope since
    std::vector<void*> mem_;
    std::vector<hipEvent_t> ev_;
    struct Out {
        void* host;
        const void* dev;
        size_t bytes;
    };
    std::vector<Out> out_;   // what finish() copies to the caller, in the order it was asked for

public:
    CallScope(hipStream_t s, bool events_on) : s_(s), events_on_(events_on) {}
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
    // (reports nothing: the error that made the call return early is the one pml_last_error keeps)
    ~CallScope() {
        if (!waited_) (void)hipStreamSynchronize(s_);
        for (void* q : mem_) (void)hipFree(q);
        for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
    }

    // device memory for `count` elements (at least one: a count of 0 still gives a pointer of its own), freed with the scope
    template <typename T>
    int get(T** out, size_t count) {
        waited_ = false;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(1, count) * sizeof(T));
        if (e != hipSuccess) return fail(PML_ERR_HIP, "hipMalloc of %zu bytes failed: %s", count * sizeof(T), hipGetErrorString(e));
        mem_.push_back(q);
        *out = (T*)q;
        return PML_OK;
    }
    // ... filled from the host: the copy is queued on the scope's stream
    template <typename T>
    int put(T** out, const T* host, size_t count) {
        PML_TRY(get(out, count));
        if (count) HIP_TRY(hipMemcpyAsync(*out, host, count * sizeof(T), hipMemcpyHostToDevice, s_));
        return PML_OK;
    }

    // ... that the caller gets: finish() copies the `count` elements to `host`, so the size is written once.  A null `host`: the
    // output is not asked for -- *dev is null, nothing is allocated, nothing copied.  zeroed: the kernels add into it, the
    // hipMemsetAsync is queued here.  Leaving the scope without finish() copies nothing.
    template <typename T>
    int out(T** dev, T* host, size_t count, bool zeroed = false) {
        *dev = nullptr;
        if (host == nullptr) return PML_OK;
        PML_TRY(get(dev, count));
        if (zeroed) HIP_TRY(hipMemsetAsync(*dev, 0, count * sizeof(T), s_));
        out_.push_back(Out{host, *dev, count * sizeof(T)});
        return PML_OK;
    }

    // an event on the stream, if the scope keeps events; elapsed() reads the time between two of them after finish() -- 0
    // where none are kept
    int mark() {
        if (!events_on_) return PML_OK;
        waited_ = false;
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev_.push_back(e);
        HIP_TRY(hipEventRecord(e, s_));
        return PML_OK;
    }
    size_t n_marks() const { return ev_.size(); }
    int elapsed(size_t i, size_t j, float* ms) const {
        *ms = 0.f;
        if (events_on_) HIP_TRY(hipEventElapsedTime(ms, ev_[i], ev_[j]));
        return PML_OK;
    }

    // the one wait of the call (or of a chunk), behind the copies of out() -- each goes once: everything queued so far is done,
    // results and events may be read
    int finish() {
        std::vector<Out> outs;
        outs.swap(out_);
        // (a copy that fails leaves the wait to the end of the scope: the copies before it write host memory)
        for (const Out& o : outs) HIP_TRY(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, s_));
        waited_ = true;   // (a stream that fails to synchronise is not waited for again)
        HIP_TRY(hipStreamSynchronize(s_));
        return PML_OK;
    }
};

static inline size_t pow2_from(size_t n) {
    size_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// Columns of a chunk whose scratch takes per_col bytes per column: what half of the free memory holds, at most `cap`, at most
// the tunable where it is set (itself at least 1), at most n_cols.  0: not even one column fits.
static inline long long chunk_rule(size_t free_bytes, size_t per_col, long long cap, bool tuned, long long tunable, int n_cols) {
    long long chunk = (long long)std::min<size_t>(free_bytes / 2 / std::max<size_t>(1, per_col), (size_t)cap);
    if (tuned) chunk = std::min(chunk, std::max(1ll, tunable));
    return chunk < 1 ? 0 : std::min<long long>(chunk, n_cols);
}

// ... for the memory that the context's device has free now
static inline int columns_per_chunk(const pml_ctx* ctx, size_t per_col, long long cap, int tunable, int n_cols, const char* entry,
                                    long long* out) {
    HIP_TRY(hipSetDevice(ctx->device));
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *out = chunk_rule(free_b, per_col, cap, ctx->tune.on(tunable), ctx->tune.get(tunable, 1), n_cols);
    if (*out < 1) return fail(PML_ERR_HIP, "%s: %zu bytes of scratch per column do not fit the device", entry, per_col);
    return PML_OK;
}

// The altered flags of the nodes (caller's ids) as 0 / 1 in the library's numbering, on the device.  `host` is the caller's and
// declared before the scope (the rule above): the copy is only queued here.
static inline int upload_altered(const pml_ctx* ctx, CallScope& scope, const unsigned char* altered, std::vector<unsigned char>& host,
                                 unsigned char** d_alt) {
    const size_t N = (size_t)ctx->N;
    host.assign(N, 0);
    for (size_t i = 0; i < N; ++i) host[ctx->new_of_old.empty() ? i : (size_t)ctx->new_of_old[i]] = altered[i] ? 1 : 0;
    return scope.put(d_alt, (const unsigned char*)host.data(), N);
}
