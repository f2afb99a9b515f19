// Host-only check of pastml_amd/csrc/pml_call_scope.h: the scope of one call's scratch, events and copies to the caller, the
// rule for the columns of a chunk, the upload of the altered flags.  The HIP names the header uses are counting stand-ins here (a
// log of the calls in order, a table of the live allocations and their sizes, "the nth call of this kind fails"); device memory
// is host memory, so a copy that overruns its allocation is counted here and is a finding of a sanitizer build.
// Built and run by tests/test_call_scope_host.py; prints FAIL lines and exits 1, or one OK line.
#include "../include/pastml_hip.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <type_traits>
#include <vector>

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failures <= 40) {                     \
                printf("FAIL [%s] ", g_case.c_str());     \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

// ---- stand-ins for the HIP runtime --------------------------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorInjected = 7 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
typedef struct StreamTag* hipStream_t;
typedef struct EventTag { int id; }* hipEvent_t;

// (COPY: to the device; COPY_OUT: to the host)
enum Kind { MALLOC, FREE, COPY, COPY_OUT, MEMSET, SYNC, EV_CREATE, EV_RECORD, EV_ELAPSED, EV_DESTROY, SET_DEVICE, MEM_INFO, N_KINDS };
struct Call {
    Kind kind;
    const void *a, *b;   // pointer / event / stream arguments
    size_t n;            // bytes, or the device
};
struct Mock {
    std::vector<Call> log;
    std::set<void*> live, handed_out;
    std::map<const void*, size_t> bytes_of;   // of every allocation handed out
    std::set<hipEvent_t> live_events;
    int seen[N_KINDS] = {}, fail_at[N_KINDS];
    int bad_frees = 0, bad_event_uses = 0, overruns = 0;
    size_t free_bytes = 0;
    Mock() {
        for (int& f : fail_at) f = -1;
    }
    // logs the call; true if this one is to fail
    bool enter(Kind k, const void* a, const void* b, size_t n) {
        log.push_back(Call{k, a, b, n});
        return seen[k]++ == fail_at[k];
    }
    // `bytes` of "device" memory from p on: p is a live allocation that holds as many
    void touches(const void* p, size_t bytes) {
        const auto it = bytes_of.find(p);
        if (it == bytes_of.end() || !live.count(const_cast<void*>(p)) || bytes > it->second) ++overruns;
    }
    int count(Kind k) const { return seen[k]; }
    int first(Kind k) const {
        for (size_t i = 0; i < log.size(); ++i)
            if (log[i].kind == k) return (int)i;
        return -1;
    }
    int last(Kind k) const {
        for (size_t i = log.size(); i-- > 0;)
            if (log[i].kind == k) return (int)i;
        return -1;
    }
};
static Mock* g_mock = nullptr;

static hipError_t hipMalloc(void** p, size_t bytes) {
    if (g_mock->enter(MALLOC, nullptr, nullptr, bytes)) return hipErrorInjected;
    *p = malloc(bytes);
    g_mock->live.insert(*p);
    g_mock->handed_out.insert(*p);
    g_mock->bytes_of[*p] = bytes;
    return hipSuccess;
}
static hipError_t hipFree(void* p) {
    g_mock->enter(FREE, p, nullptr, 0);
    if (!g_mock->live.erase(p)) {
        ++g_mock->bad_frees;   // never handed out, or freed before
        return hipErrorInjected;
    }
    free(p);
    return hipSuccess;
}
static hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (g_mock->enter(kind == hipMemcpyDeviceToHost ? COPY_OUT : COPY, dst, s, bytes)) return hipErrorInjected;
    g_mock->touches(kind == hipMemcpyDeviceToHost ? src : dst, bytes);
    memcpy(dst, src, bytes);
    return hipSuccess;
}
static hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t s) {
    if (g_mock->enter(MEMSET, dst, s, bytes)) return hipErrorInjected;
    g_mock->touches(dst, bytes);
    memset(dst, value, bytes);
    return hipSuccess;
}
static hipError_t hipStreamSynchronize(hipStream_t s) { return g_mock->enter(SYNC, s, nullptr, 0) ? hipErrorInjected : hipSuccess; }
static hipError_t hipEventCreate(hipEvent_t* e) {
    if (g_mock->enter(EV_CREATE, nullptr, nullptr, 0)) return hipErrorInjected;
    *e = new EventTag{g_mock->count(EV_CREATE) - 1};
    g_mock->live_events.insert(*e);
    return hipSuccess;
}
static hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    if (!g_mock->live_events.count(e)) ++g_mock->bad_event_uses;
    return g_mock->enter(EV_RECORD, e, s, 0) ? hipErrorInjected : hipSuccess;
}
static hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
    if (!g_mock->live_events.count(a) || !g_mock->live_events.count(b)) ++g_mock->bad_event_uses;
    if (g_mock->enter(EV_ELAPSED, a, b, 0)) return hipErrorInjected;
    *ms = (float)(b->id - a->id);
    return hipSuccess;
}
static hipError_t hipEventDestroy(hipEvent_t e) {
    g_mock->enter(EV_DESTROY, e, nullptr, 0);
    if (!g_mock->live_events.erase(e)) {
        ++g_mock->bad_event_uses;
        return hipErrorInjected;
    }
    delete e;
    return hipSuccess;
}
static hipError_t hipSetDevice(int device) { return g_mock->enter(SET_DEVICE, nullptr, nullptr, (size_t)device) ? hipErrorInjected : hipSuccess; }
static hipError_t hipMemGetInfo(size_t* free_b, size_t* total_b) {
    if (g_mock->enter(MEM_INFO, nullptr, nullptr, 0)) return hipErrorInjected;
    *free_b = g_mock->free_bytes;
    *total_b = 2 * g_mock->free_bytes;
    return hipSuccess;
}
static const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "injected failure"; }

// ---- ... for the library's error reporting and the part of the context the header reads -----------------------------------
static char g_last_error[512];
__attribute__((format(printf, 2, 3))) static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                                            \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess)                                                                                    \
            return fail(PML_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)
#define PML_TRY(expr)                \
    do {                             \
        int _s = (expr);             \
        if (_s != PML_OK) return _s; \
    } while (0)

struct Tune {
    int which = -1;   // the one tunable that is set
    long long val = 0;
    bool on(int i) const { return i == which; }
    long long get(int i, long long dflt) const { return i == which ? val : dflt; }
};
struct pml_ctx {
    int device = 0;
    Tune tune;
    int N = 0;
    std::vector<int> new_of_old;
};

#include "../pastml_amd/csrc/pml_call_scope.h"

static_assert(!std::is_copy_constructible<CallScope>::value && !std::is_copy_assignable<CallScope>::value, "the scope cannot be copied");

static hipStream_t const STREAM = (hipStream_t)(uintptr_t)0x51;

// everything handed out came back exactly once, nothing else was freed, no event is left
static void check_clean(const Mock& m) {
    CHECK(m.live.empty(), "%zu allocations were never freed", m.live.size());
    CHECK(m.bad_frees == 0, "%d frees of pointers that were not live", m.bad_frees);
    CHECK(m.count(FREE) == (int)m.handed_out.size(), "%d frees of %zu allocations", m.count(FREE), m.handed_out.size());
    CHECK(m.live_events.empty(), "%zu events were never destroyed", m.live_events.size());
    CHECK(m.bad_event_uses == 0, "%d uses of events that were not live", m.bad_event_uses);
    CHECK(m.overruns == 0, "%d copies or fills outside a live allocation", m.overruns);
    if (m.count(FREE) > 0 && (m.count(COPY) > 0 || m.count(COPY_OUT) > 0 || m.count(MEMSET) > 0 || m.count(EV_RECORD) > 0))
        CHECK(m.first(SYNC) >= 0 && m.last(SYNC) < m.first(FREE), "a free at %d before the synchronisation at %d", m.first(FREE), m.last(SYNC));
    for (const Call& c : m.log)
        if (c.kind == SYNC || c.kind == COPY || c.kind == COPY_OUT || c.kind == MEMSET)
            CHECK((c.kind == SYNC ? c.a : c.b) == STREAM, "a call on another stream");
    // nothing queued is left unwaited for: a copy to the host that the scope freed under would write memory the caller reads
    if (m.last(COPY_OUT) >= 0) CHECK(m.last(SYNC) > m.last(COPY_OUT), "no synchronisation behind the copy out at %d", m.last(COPY_OUT));
}

// ---- 1, 2: six requests, the allocation of each failing in turn; a request of 0 elements -----------------------------------
static const size_t SIX_BYTES[6] = {40, 32, 0, 20, 24, 7};
static int six_requests(CallScope& sc, void** got) {
    static const double h1[4] = {1, 2, 3, 4};
    static const int h3[5] = {5, 6, 7, 8, 9};
    static const unsigned char h5[7] = {1, 0, 1, 0, 1, 0, 1};
    int* p0;
    double* p1;
    unsigned char *p2, *p5;
    int* p3;
    long long* p4;
    PML_TRY(sc.get(&p0, 10));
    got[0] = p0;
    PML_TRY(sc.put(&p1, h1, 4));
    got[1] = p1;
    PML_TRY(sc.get(&p2, 0));
    got[2] = p2;
    PML_TRY(sc.put(&p3, h3, 5));
    got[3] = p3;
    PML_TRY(sc.get(&p4, 3));
    got[4] = p4;
    PML_TRY(sc.put(&p5, h5, 7));
    got[5] = p5;
    CHECK(p1[3] == 4.0 && p3[4] == 9 && p5[6] == 1, "put did not copy");
    return PML_OK;
}

static void test_allocation_failures() {
    for (int bad = -1; bad < 6; ++bad) {
        g_case = "allocation " + std::to_string(bad) + " fails";
        Mock m;
        g_mock = &m;
        m.fail_at[MALLOC] = bad;
        void* got[6] = {};
        g_last_error[0] = 0;
        int status;
        {
            CallScope sc(STREAM, false);
            status = six_requests(sc, got);
            CHECK(m.count(FREE) == 0, "a free before the scope ended");
        }
        const int n_ok = bad < 0 ? 6 : bad;
        CHECK(status == (bad < 0 ? PML_OK : PML_ERR_HIP), "status %d", status);
        CHECK((int)m.handed_out.size() == n_ok, "%zu allocations, expected %d", m.handed_out.size(), n_ok);
        for (int i = 0; i < n_ok; ++i) {
            CHECK(got[i] != nullptr && m.handed_out.count(got[i]), "request %d got no pointer of the scope's", i);
            for (int j = 0; j < i; ++j) CHECK(got[i] != got[j], "requests %d and %d share a pointer", i, j);
        }
        if (bad >= 0) {
            const std::string want = "hipMalloc of " + std::to_string(SIX_BYTES[bad]) + " bytes failed: injected failure";
            CHECK(want == g_last_error, "message '%s', expected '%s'", g_last_error, want.c_str());
        }
        if (n_ok > 2) {   // (2) the request of 0 elements: a pointer of its own, one byte at least behind it
            size_t seen = 0;
            for (const Call& c : m.log)
                if (c.kind == MALLOC && seen++ == 2) CHECK(c.n >= 1, "the request of 0 elements asked hipMalloc for %zu bytes", c.n);
        }
        CHECK(m.count(EV_CREATE) == 0, "an event without events on");
        check_clean(m);
    }
}

// ---- 3, 4: events ----------------------------------------------------------------------------------------------------------
static int three_marks(CallScope& sc) {
    int* p;
    PML_TRY(sc.get(&p, 4));
    PML_TRY(sc.mark());
    PML_TRY(sc.mark());
    PML_TRY(sc.mark());
    return PML_OK;
}

static void test_events() {
    g_case = "events off";
    {
        Mock m;
        g_mock = &m;
        {
            CallScope sc(STREAM, false);
            CHECK(three_marks(sc) == PML_OK, "mark() failed");
            CHECK(sc.n_marks() == 0, "%zu marks", sc.n_marks());
            float ms = 5.f;
            CHECK(sc.finish() == PML_OK && sc.elapsed(0, 1, &ms) == PML_OK && ms == 0.f, "elapsed() without events gave %g", ms);
        }
        CHECK(m.count(EV_CREATE) + m.count(EV_RECORD) + m.count(EV_ELAPSED) + m.count(EV_DESTROY) == 0, "an event call");
        check_clean(m);
    }
    g_case = "events on";
    {
        Mock m;
        g_mock = &m;
        std::vector<hipEvent_t> made;
        {
            CallScope sc(STREAM, true);
            CHECK(three_marks(sc) == PML_OK, "mark() failed");
            CHECK(sc.n_marks() == 3, "%zu marks", sc.n_marks());
            for (const Call& c : m.log)
                if (c.kind == EV_RECORD) {
                    made.push_back((hipEvent_t)c.a);
                    CHECK(c.b == STREAM, "recorded on another stream");
                }
            CHECK(sc.finish() == PML_OK, "finish() failed");
            float ms = 0.f;
            CHECK(sc.elapsed(0, 2, &ms) == PML_OK && ms == 2.f, "elapsed(0, 2) gave %g", ms);
            CHECK(sc.elapsed(1, 2, &ms) == PML_OK && ms == 1.f, "elapsed(1, 2) gave %g", ms);
        }
        CHECK(m.count(EV_CREATE) == 3 && m.count(EV_RECORD) == 3 && m.count(EV_DESTROY) == 3, "creates %d records %d destroys %d",
              m.count(EV_CREATE), m.count(EV_RECORD), m.count(EV_DESTROY));
        CHECK(m.count(SYNC) == 1, "%d synchronisations", m.count(SYNC));
        CHECK(m.last(FREE) < m.first(EV_DESTROY), "an event destroyed before the last free");
        size_t seen = 0;
        for (const Call& c : m.log)
            if (c.kind == EV_ELAPSED) {
                CHECK(made.size() == 3 && c.a == made[seen] && c.b == made[2], "elapsed() handed over another pair");
                ++seen;
            }
        check_clean(m);
    }
    for (int which = 0; which < 2; ++which) {
        g_case = which ? "hipEventRecord fails" : "hipEventCreate fails";
        Mock m;
        g_mock = &m;
        m.fail_at[which ? EV_RECORD : EV_CREATE] = 1;
        {
            CallScope sc(STREAM, true);
            CHECK(three_marks(sc) == PML_ERR_HIP, "mark() did not fail");
        }
        CHECK(m.count(EV_DESTROY) == (which ? 2 : 1), "%d destroys", m.count(EV_DESTROY));
        check_clean(m);
    }
}

// ---- 5: finish() and the destructor ----------------------------------------------------------------------------------------
static void test_finish() {
    static const int host[3] = {1, 2, 3};
    int* p;
    g_case = "finish, end";
    {
        Mock m;
        g_mock = &m;
        {
            CallScope sc(STREAM, false);
            CHECK(sc.put(&p, host, 3) == PML_OK && sc.finish() == PML_OK, "failed");
        }
        CHECK(m.count(SYNC) == 1, "%d synchronisations", m.count(SYNC));
        check_clean(m);
    }
    g_case = "no finish";
    {
        Mock m;
        g_mock = &m;
        {
            CallScope sc(STREAM, false);
            CHECK(sc.put(&p, host, 3) == PML_OK, "failed");
        }
        CHECK(m.count(SYNC) == 1, "%d synchronisations", m.count(SYNC));
        check_clean(m);
    }
    g_case = "finish, put, end";
    {
        Mock m;
        g_mock = &m;
        {
            CallScope sc(STREAM, false);
            CHECK(sc.put(&p, host, 3) == PML_OK && sc.finish() == PML_OK && sc.put(&p, host, 2) == PML_OK, "failed");
        }
        CHECK(m.count(SYNC) == 2, "%d synchronisations", m.count(SYNC));
        check_clean(m);
    }
    g_case = "finish fails";
    {
        Mock m;
        g_mock = &m;
        m.fail_at[SYNC] = 0;
        int status;
        {
            CallScope sc(STREAM, false);
            CHECK(sc.put(&p, host, 3) == PML_OK, "failed");
            status = sc.finish();
        }
        CHECK(status == PML_ERR_HIP, "status %d", status);
        CHECK(strstr(g_last_error, "hipStreamSynchronize") != nullptr, "message '%s'", g_last_error);
        CHECK(m.count(FREE) == 1, "%d frees", m.count(FREE));
        check_clean(m);
    }
}

// ---- 5b: outputs -- device memory tied to its host destination, copied by finish() ----------------------------------------------
struct Outputs {
    int a[10];
    double b[4];         // not asked for in the calls below
    unsigned c[6];       // zeroed on the device, then added into
    unsigned short e;    // a request of 0 elements: nothing may be written here
    long long f[3];
    Outputs() { memset(this, 0x5a, sizeof(*this)); }
};
static const size_t OUT_BYTES[4] = {40, 24, 0, 24};

// the requests, then what the kernels would write; stop_after: the call returns early behind that many requests
static int four_outputs(CallScope& sc, Outputs& h, int stop_after = 4) {
    int* d_a;
    double* d_b = (double*)&h;
    unsigned* d_c;
    unsigned short* d_e;
    long long* d_f;
    PML_TRY(sc.out(&d_a, h.a, 10));
    PML_TRY(sc.out(&d_b, (double*)nullptr, 4));
    CHECK(d_b == nullptr, "an output that is not asked for got a pointer");
    if (stop_after == 1) return fail(PML_ERR_INVALID, "stopped");
    PML_TRY(sc.out(&d_c, h.c, 6, true));
    for (int i = 0; i < 6; ++i) CHECK(d_c[i] == 0, "a zeroed output holds %u", d_c[i]);
    PML_TRY(sc.out(&d_e, &h.e, 0));
    CHECK(d_e != nullptr, "a request of 0 elements got no pointer");
    if (stop_after == 3) return fail(PML_ERR_INVALID, "stopped");
    PML_TRY(sc.out(&d_f, h.f, 3));
    for (int i = 0; i < 10; ++i) d_a[i] = 100 + i;
    for (int i = 0; i < 6; ++i) d_c[i] += 7u * i;
    for (int i = 0; i < 3; ++i) d_f[i] = -1 - i;
    return PML_OK;
}

static bool untouched(const Outputs& h) {
    const Outputs fresh;
    return memcmp(&h, &fresh, sizeof(h)) == 0;
}

static void check_copied(const Outputs& h) {
    const Outputs fresh;
    for (int i = 0; i < 10; ++i) CHECK(h.a[i] == 100 + i, "a[%d] = %d", i, h.a[i]);
    for (int i = 0; i < 6; ++i) CHECK(h.c[i] == 7u * i, "c[%d] = %u", i, h.c[i]);
    for (int i = 0; i < 3; ++i) CHECK(h.f[i] == -1 - i, "f[%d] = %lld", i, h.f[i]);
    CHECK(memcmp(h.b, fresh.b, sizeof(h.b)) == 0 && h.e == fresh.e, "an output that was not asked for, or of 0 elements, was written");
}

static void test_outputs() {
    g_case = "outputs: order, sizes, one wait";
    {
        Mock m;
        g_mock = &m;
        Outputs h;   // (before the scope: the rule of the header)
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h) == PML_OK, "failed: %s", g_last_error);
            CHECK(m.count(COPY_OUT) == 0 && untouched(h), "a copy before finish()");
            CHECK(m.count(MEMSET) == 1 && m.log[m.first(MEMSET)].n == 24 && m.first(MEMSET) == m.first(MALLOC) + 2,
                  "the zeroed output was not cleared where it was asked for, in its own size");
            CHECK(sc.finish() == PML_OK, "finish() failed");
            check_copied(h);
        }
        CHECK(m.count(MALLOC) == 4, "%d allocations for four outputs that are asked for", m.count(MALLOC));
        const void* dst[4] = {h.a, h.c, &h.e, h.f};
        size_t seen = 0;
        for (const Call& c : m.log)
            if (c.kind == COPY_OUT && seen < 4) {
                CHECK(c.a == dst[seen] && c.n == OUT_BYTES[seen], "copy %zu goes to another output, or has %zu bytes", seen, c.n);
                ++seen;
            }
        CHECK(m.count(COPY_OUT) == 4, "%d copies out", m.count(COPY_OUT));
        CHECK(m.count(SYNC) == 1 && m.first(SYNC) > m.last(COPY_OUT), "%d synchronisations, the first at %d, the last copy at %d",
              m.count(SYNC), m.first(SYNC), m.last(COPY_OUT));
        check_clean(m);
    }
    g_case = "outputs: nothing is copied twice";
    {
        Mock m;
        g_mock = &m;
        Outputs h, h2;
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h) == PML_OK && sc.finish() == PML_OK, "failed");
            h.a[0] = -5;   // (the caller's from here on)
            CHECK(sc.finish() == PML_OK && m.count(COPY_OUT) == 4 && h.a[0] == -5, "a second finish() copied again");
            // a launcher that waits once per chunk: the next chunk's outputs go with the next wait, the first chunk's do not
            CHECK(four_outputs(sc, h2) == PML_OK && sc.finish() == PML_OK, "failed");
            CHECK(m.count(COPY_OUT) == 8 && h.a[0] == -5, "%d copies out behind two chunks", m.count(COPY_OUT));
            check_copied(h2);
        }
        CHECK(m.count(SYNC) == 3, "%d synchronisations", m.count(SYNC));
        check_clean(m);
    }
    for (int stop_after : {1, 3}) {
        g_case = "outputs: early exit behind request " + std::to_string(stop_after);
        Mock m;
        g_mock = &m;
        Outputs h;
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h, stop_after) == PML_ERR_INVALID, "did not stop");
        }
        CHECK(m.count(COPY_OUT) == 0 && untouched(h), "%d copies out on an early exit", m.count(COPY_OUT));
        CHECK(m.count(SYNC) == 1 && m.count(FREE) == stop_after, "synchronisations %d frees %d", m.count(SYNC), m.count(FREE));
        check_clean(m);
    }
    g_case = "outputs: an allocation fails";
    {
        Mock m;
        g_mock = &m;
        m.fail_at[MALLOC] = 1;
        Outputs h;
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h) == PML_ERR_HIP, "no error");
        }
        CHECK(m.count(COPY_OUT) == 0 && m.count(MEMSET) == 0 && untouched(h), "a copy or a fill behind a failed allocation");
        check_clean(m);
    }
    g_case = "outputs: the fill fails";
    {
        Mock m;
        g_mock = &m;
        m.fail_at[MEMSET] = 0;
        Outputs h;
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h) == PML_ERR_HIP && strstr(g_last_error, "hipMemsetAsync") != nullptr, "message '%s'", g_last_error);
        }
        CHECK(m.count(COPY_OUT) == 0 && m.count(FREE) == 2 && untouched(h), "copies %d frees %d", m.count(COPY_OUT), m.count(FREE));
        check_clean(m);
    }
    for (int bad = 0; bad < 8; ++bad) {
        const bool again = bad >= 4;   // the call goes on to a second finish(), or returns at once
        g_case = "outputs: copy " + std::to_string(bad % 4) + " fails" + (again ? ", finish again" : "");
        Mock m;
        g_mock = &m;
        m.fail_at[COPY_OUT] = bad % 4;
        Outputs h;
        int status;
        {
            CallScope sc(STREAM, false);
            CHECK(four_outputs(sc, h) == PML_OK, "failed");
            g_last_error[0] = 0;
            status = sc.finish();
            CHECK(m.count(SYNC) == 0, "a wait that reports nothing inside the failed finish()");
            if (again) CHECK(sc.finish() == PML_OK && m.count(COPY_OUT) == bad % 4 + 1, "the copies behind a failed one were tried later");
        }
        CHECK(status == PML_ERR_HIP && strstr(g_last_error, "hipMemcpyAsync") != nullptr, "status %d, message '%s'", status, g_last_error);
        CHECK(m.count(FREE) == 4 && m.count(SYNC) == 1, "frees %d synchronisations %d", m.count(FREE), m.count(SYNC));
        check_clean(m);   // (a wait behind the copies that went, before the frees)
    }
}

// ---- 6: the columns of a chunk.  Expected values by hand from
//         min(free / 2 / max(1, per_col), cap), then min(., max(1, tunable)) if set, an error below 1, then min(., n_cols) -------
static void test_chunk_rule() {
    const size_t GiB64 = 68719476736ull;
    const long long P = 65535, V = 1 << 20;   // the caps of the parsimony and of the vertical collapse
    struct Row {
        const char* name;
        size_t free_b, per_col;
        long long cap;
        bool tuned;
        long long tunable;
        int n_cols;
        long long expected;   // 0: does not fit
    };
    const Row rows[] = {
        {"memory to spare", GiB64, 1000, P, false, 0, 32, 32},
        {"memory to spare, wide cap", GiB64, 1000, V, false, 0, 32, 32},
        {"cap 65535 binds", GiB64, 1000, P, false, 0, 100000, 65535},           // 34 359 738 columns fit
        {"cap 2^20 binds", GiB64, 8, V, false, 0, 2000000, 1048576},            // 4 294 967 296 fit
        {"cap 2^20, not 65535", GiB64, 1000, V, false, 0, 100000, 100000},
        {"memory binds", 1000000, 1000, P, false, 0, 10000, 500},
        {"memory binds, odd sizes", 1000001, 333, V, false, 0, 10000, 1501},    // 500 000 / 333 = 1501.5
        {"tunable below the memory", 1000000, 1000, P, true, 5, 32, 5},
        {"tunable above the memory", 1000000, 1000, P, true, 700, 10000, 500},
        {"tunable above the columns", GiB64, 1000, V, true, 40, 32, 32},
        {"tunable 0", GiB64, 1000, P, true, 0, 32, 1},
        {"tunable negative", GiB64, 1000, V, true, -3, 32, 1},
        {"nothing per column", GiB64, 0, V, false, 0, 2000000, 1048576},
        {"nothing per column, little memory", 1000, 0, V, false, 0, 2000000, 500},
        {"one column fits exactly", 1000, 500, P, false, 0, 32, 1},
        {"no column fits", 1000, 501, P, false, 0, 32, 0},
        {"no column fits, tunable set", 1000, 501, V, true, 5, 32, 0},
        {"no memory", 0, 8, V, false, 0, 32, 0},
        {"one column", GiB64, 1000, P, false, 0, 1, 1},
        {"one column, tunable", GiB64, 1000, V, true, 7, 1, 1},
    };
    for (const Row& r : rows) {
        g_case = std::string("chunk rule: ") + r.name;
        const long long got = chunk_rule(r.free_b, r.per_col, r.cap, r.tuned, r.tunable, r.n_cols);
        CHECK(got == r.expected, "%lld columns, expected %lld", got, r.expected);
        // ... and through the function that asks the device
        Mock m;
        g_mock = &m;
        m.free_bytes = r.free_b;
        pml_ctx ctx;
        ctx.device = 3;
        if (r.tuned) {
            ctx.tune.which = 11;
            ctx.tune.val = r.tunable;
        }
        long long chunk = -1;
        g_last_error[0] = 0;
        const int status = columns_per_chunk(&ctx, r.per_col, r.cap, 11, r.n_cols, "pml_some_entry", &chunk);
        CHECK(m.count(SET_DEVICE) == 1 && m.log[0].kind == SET_DEVICE && m.log[0].n == 3, "the context's device was not selected first");
        if (r.expected > 0) {
            CHECK(status == PML_OK && chunk == r.expected, "status %d, %lld columns, expected %lld", status, chunk, r.expected);
        } else {
            const std::string want = "pml_some_entry: " + std::to_string(r.per_col) + " bytes of scratch per column do not fit the device";
            CHECK(status == PML_ERR_HIP && want == g_last_error, "status %d, message '%s'", status, g_last_error);
        }
    }
    g_case = "chunk rule: hipMemGetInfo fails";
    Mock m;
    g_mock = &m;
    m.fail_at[MEM_INFO] = 0;
    pml_ctx ctx;
    long long chunk = -1;
    CHECK(columns_per_chunk(&ctx, 8, V, 11, 32, "pml_some_entry", &chunk) == PML_ERR_HIP, "no error");
}

// ---- the power of two, the altered flags -----------------------------------------------------------------------------------
static void test_small_helpers() {
    g_case = "pow2_from";
    const size_t in[] = {0, 1, 2, 3, 4, 5, 8, 9, 1023, 1024, 1025, (size_t)1 << 30, ((size_t)1 << 30) + 1};
    const size_t out[] = {1, 1, 2, 4, 4, 8, 8, 16, 1024, 1024, 2048, (size_t)1 << 30, (size_t)1 << 31};
    for (size_t i = 0; i < sizeof(in) / sizeof(in[0]); ++i) CHECK(pow2_from(in[i]) == out[i], "pow2_from(%zu) = %zu", in[i], pow2_from(in[i]));

    const unsigned char altered[5] = {0, 7, 0, 1, 0};   // (any non-zero byte is a flag)
    for (int permuted = 0; permuted < 2; ++permuted) {
        g_case = permuted ? "upload_altered, renumbered" : "upload_altered";
        Mock m;
        g_mock = &m;
        pml_ctx ctx;
        ctx.N = 5;
        if (permuted) ctx.new_of_old = {4, 2, 0, 1, 3};
        const unsigned char expected[2][5] = {{0, 1, 0, 1, 0}, {0, 1, 1, 0, 0}};
        std::vector<unsigned char> host;
        {
            CallScope sc(STREAM, false);
            unsigned char* d_alt = nullptr;
            CHECK(upload_altered(&ctx, sc, altered, host, &d_alt) == PML_OK, "failed");
            CHECK(d_alt != nullptr && memcmp(d_alt, expected[permuted], 5) == 0, "other flags on the device");
            CHECK(m.count(SYNC) == 0, "upload_altered waits: the host vector is the caller's");
        }
        CHECK(m.count(MALLOC) == 1 && m.count(COPY) == 1 && m.count(SYNC) == 1, "mallocs %d copies %d synchronisations %d", m.count(MALLOC),
              m.count(COPY), m.count(SYNC));
        check_clean(m);
    }
}

int main() {
    test_allocation_failures();
    test_events();
    test_finish();
    test_outputs();
    test_chunk_rule();
    test_small_helpers();
    if (g_failures) {
        printf("%d checks failed\n", g_failures);
        return 1;
    }
    printf("OK: allocation failures, events, finish, outputs, chunk rule, helpers\n");
    return 0;
}
