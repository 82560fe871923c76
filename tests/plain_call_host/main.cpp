// The bookkeeping of PlainCall (libviso_amd/csrc/common.h, ctx.hip) and ctx_resolve without a device: ctx.hip itself is compiled into
// this program (host side only), and every hip* entry point and library function it uses is a stub here that writes a log line and
// fails on request.  The rule under test: an error return leaves nothing of the call queued -- the destructor waits for the stream,
// once, while it still holds the plain family's lock -- and every return with nothing queued, the success path included, waits for
// nothing.  tests/test_plain_call_cpu.py builds and runs it; it prints "plain_call_host ok" and returns 0, or says what it found.
#include "../../libviso_amd/csrc/ctx.hip"

#include <string>
#include <thread>

static std::vector<std::string> g_log;
static std::string g_fail;   // the stub of this name fails, once
static int g_failures = 0;

static bool fails(const char* name) {
    g_log.push_back(name);
    if (g_fail != name) return false;
    g_fail.clear();
    g_log.back() += " FAILED";
    return true;
}
// whether some thread holds the plain family's lock: asked from a thread that does not
static bool lock_held() {
    bool held = false;
    std::thread([&] { if (g_call_mu.try_lock()) g_call_mu.unlock(); else held = true; }).join();
    return held;
}

#define STUB(name, ...) extern "C" hipError_t name(__VA_ARGS__) { return fails(#name) ? hipErrorUnknown : hipSuccess; }
extern "C" hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
extern "C" hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "stub failure"; }
STUB(hipSetDevice, int)
extern "C" hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { static int streams[2]; static int n = 0; *s = (hipStream_t)&streams[n++ & 1]; return hipSuccess; }
STUB(hipStreamDestroy, hipStream_t)
extern "C" hipError_t hipStreamSynchronize(hipStream_t) {
    g_log.push_back(lock_held() ? "hipStreamSynchronize locked" : "hipStreamSynchronize UNLOCKED");
    return hipSuccess;
}
extern "C" hipError_t hipMalloc(void** p, size_t b) { if (fails("hipMalloc")) return hipErrorOutOfMemory; *p = malloc(b); return hipSuccess; }
extern "C" hipError_t hipHostMalloc(void** p, size_t b, unsigned) { if (fails("hipHostMalloc")) return hipErrorOutOfMemory; *p = malloc(b); return hipSuccess; }
extern "C" hipError_t hipFree(void* p) { free(p); return hipSuccess; }
extern "C" hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
STUB(hipMemsetAsync, void*, int, size_t, hipStream_t)
STUB(hipMemcpyAsync, void*, const void*, size_t, hipMemcpyKind, hipStream_t)
STUB(hipEventCreate, hipEvent_t*)
STUB(hipEventRecord, hipEvent_t, hipStream_t)
STUB(hipEventSynchronize, hipEvent_t)
extern "C" hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0; return hipSuccess; }

// the rest of the library that ctx.hip calls
void plain_cache_free(viso_ctx*) {}
int viso_batch_free(viso_batch*, bool) { return VISO_OK; }
const char* matcher_kernel_name(int) { return "stub"; }
int plain_signal_next(viso_ctx* c, PlainSignal* out) {
    if (fails("plain_signal_next")) return VISO_ERR_HIP;
    *out = PlainSignal{nullptr, nullptr, ++c->sig_seq};
    return VISO_OK;
}
int plain_signal_wait(viso_ctx*, hipStream_t, uint32_t) { return fails("plain_signal_wait") ? VISO_ERR_HIP : VISO_OK; }
int plain_blit(hipStream_t, const void*, void*, size_t, const int*, int, int, const PlainSignal*) { return fails("plain_blit") ? VISO_ERR_HIP : VISO_OK; }
int PlainStage::flush(hipStream_t) { return fails("flush") ? VISO_ERR_HIP : VISO_OK; }
static int launch() { return fails("launch") ? VISO_ERR_HIP : VISO_OK; }

// One call of the family's shape.  flush: its inputs go through the copy kernel and its results through fetch() (minimize, get_inliers,
// circle); otherwise its one kernel reads the pinned block and signals itself (collect, triangulate).
static int the_call(bool served, bool flush, size_t bytes) {
    PlainCall pc;
    VISO_TRY(pc.begin(VISO_PLAIN_MINIMIZE));
    if (served) return 1;
    VISO_TRY(pc.inputs(bytes));
    VISO_TRY(pc.result(bytes, flush));
    const int v = 7;
    pc.in.put(&v, 1);
    VISO_TRY(pc.sent(flush));
    PlainSignal sig;
    if (!flush) VISO_TRY(pc.signal(&sig));
    VISO_TRY(launch());
    pc.launched();
    if (flush) VISO_TRY(pc.fetch(1));
    VISO_TRY(pc.wait());
    pc.done();
    return VISO_OK;
}

// runs the call with `fail` failing and checks its return and the synchronises BEHIND the failure (all of them with fail == "")
static void expect(const char* what, bool served, bool flush, size_t bytes, const char* fail, int want_ret, int want_syncs) {
    g_log.clear();
    g_fail = fail;
    const int ret = the_call(served, flush, bytes);
    size_t from = 0;
    for (size_t i = 0; i < g_log.size(); ++i) if (g_log[i].find(" FAILED") != std::string::npos) from = i + 1;
    int syncs = 0, unlocked = 0;
    for (size_t i = from; i < g_log.size(); ++i) {
        if (g_log[i].rfind("hipStreamSynchronize", 0) == 0) ++syncs;
        if (g_log[i] == "hipStreamSynchronize UNLOCKED") ++unlocked;
    }
    const bool failed_as_asked = !*fail || (g_fail.empty() && from > 0);
    if (ret == want_ret && syncs == want_syncs && !unlocked && !lock_held() && failed_as_asked) return;
    ++g_failures;
    printf("FAILED %s: returned %d (expected %d), %d synchronises behind the failure (expected %d), %d of them without the lock, lock %s afterwards%s\n",
           what, ret, want_ret, syncs, want_syncs, unlocked, lock_held() ? "HELD" : "free", failed_as_asked ? "" : ", the stub never failed");
    for (const std::string& l : g_log) printf("    %s\n", l.c_str());
}

static void expect_text(const char* what, int ret, int want_ret, const char* want_text) {
    if (ret == want_ret && (!want_text || !strcmp(viso_last_error(), want_text))) return;
    ++g_failures;
    printf("FAILED %s: returned %d (expected %d), text \"%s\"\n", what, ret, want_ret, viso_last_error());
}

int main() {
    // ---- ctx_resolve -------------------------------------------------------------------------------------------------------------
    viso_ctx* dead = reinterpret_cast<viso_ctx*>(&g_failures);
    viso_ctx* c = nullptr;
    expect_text("a dead handle, named", ctx_resolve("viso_x", dead, &c), VISO_ERR_ARG, "viso_x: not a live context handle");
    expect_text("a dead handle, unnamed", ctx_resolve(nullptr, dead, &c), VISO_ERR_ARG, "not a live context handle");
    expect_text("the setter's text", viso_ctx_set_gn_split(dead, 1), VISO_ERR_ARG, "not a live context handle");
    expect_text("the check alone, null", ctx_resolve("viso_x", nullptr, nullptr), VISO_OK, nullptr);
    if (!g_log.empty()) { ++g_failures; printf("FAILED: the checks touched the device (%s)\n", g_log[0].c_str()); }
    expect_text("null is the default context", ctx_resolve("viso_x", nullptr, &c), VISO_OK, nullptr);
    if (c != viso_default_ctx() || !c) { ++g_failures; printf("FAILED: null did not resolve to the default context\n"); }
    viso_ctx* own = viso_ctx_create(0, nullptr);
    expect_text("a live handle", ctx_resolve("viso_x", own, &c), VISO_OK, nullptr);
    if (c != own) { ++g_failures; printf("FAILED: a live handle did not resolve to itself\n"); }
    viso_ctx_destroy(own);
    expect_text("a destroyed handle", ctx_resolve("viso_x", own, nullptr), VISO_ERR_ARG, "viso_x: not a live context handle");

    // ---- PlainCall ---------------------------------------------------------------------------------------------------------------
    // the first call allocates every block (ctx_scratch and ctx_pinned wait for the stream themselves when a block grows)
    expect("the first call", false, true, 64, "", VISO_OK, 4);
    for (int flush = 0; flush < 2; ++flush) {
        expect("success", false, flush, 64, "", VISO_OK, 0);
        expect("served", true, flush, 64, "", 1, 0);
        expect("the context's device cannot be set", false, flush, 64, "hipSetDevice", VISO_ERR_HIP, 0);
        expect("the launch failed", false, flush, 64, "launch", VISO_ERR_HIP, 1);
        expect("no signal", false, flush, 64, "plain_signal_next", VISO_ERR_HIP, 1);
        expect("the wait failed", false, flush, 64, "plain_signal_wait", VISO_ERR_HIP, 1);
    }
    expect("the flush failed", false, true, 64, "flush", VISO_ERR_HIP, 1);
    expect("the fetch failed", false, true, 64, "plain_blit", VISO_ERR_HIP, 1);
    // blocks that have to grow, and cannot: the inputs' pinned block, their device mirror, the result's mirror -- all before sent()
    expect("no pinned memory", false, true, 100000, "hipHostMalloc", VISO_ERR_HIP, 0);
    expect("no device memory", false, true, 200000, "hipMalloc", VISO_ERR_HIP, 0);
    expect("success behind the failures", false, true, 400000, "", VISO_OK, 4);   // the four blocks grow: their own waits, under the lock
    expect("success again", false, true, 400000, "", VISO_OK, 0);
    // the profile's events do not change any of it
    viso_plain_profile(1);
    expect("success, profiled", false, true, 64, "", VISO_OK, 0);
    expect("the launch failed, profiled", false, true, 64, "launch", VISO_ERR_HIP, 1);
    viso_plain_profile(0);
    viso_plain_times t;
    viso_plain_profile_get(VISO_PLAIN_MINIMIZE, &t);
    if (t.calls != 2) { ++g_failures; printf("FAILED: the profile counted %lld calls of 2\n", (long long)t.calls); }
    if (g_failures) return 1;
    printf("plain_call_host ok\n");
    return 0;
}
