// A simulated HIP runtime for running csrc/hgi_capi.hip on the CPU under ASan + UBSan (profiles/r16_host_routes.md).
//
// Memory: hipMalloc / hipHostMalloc hand out exact-size heap blocks (ASan's red zones guard both ends), filled with a
// nonzero poison byte; hipFree really frees.  Streams are FIFOs of operations (copies, memsets, launches, event records,
// event waits) run under one of four schedules (hostsim.h); a copy reads and writes when it EXECUTES, pageable host memory
// included.  hipStreamWaitEvent binds to the event's most recent record at the time of the call and is a no-op for an event
// that was never recorded (HIP's rule).
//
// 2-D copies, the rule this harness holds the library to: for a HOST-side operand every byte of [p, p + height * pitch)
// must lie inside the caller's array -- the rectangle profiles/r12_geometry_coverage.md section 6 found the runtime may
// pin and read as a whole; for a DEVICE-side operand (height - 1) * pitch + width.  This is the project's defensive
// contract, derived from one observed fault; it is NOT a measured property of ROCm.
#include "hostsim.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <map>
#include <set>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#endif

struct SimOp {
    int kind;      // 0 run, 1 record, 2 wait
    std::function<void()> fn;
    uint64_t rec;  // record id (kinds 1, 2)
    bool caller;   // touches pageable host memory
};

struct ihipStream_t {
    std::deque<SimOp> q;
};
struct ihipEvent_t {
    uint64_t last_rec = 0;   // 0: never recorded
};

namespace {

struct Block {
    size_t size;
    bool pinned;
};

sim::Schedule g_sched = sim::kEager;
uint64_t g_rng = 1;
uint8_t g_poison = 0xA5;
std::string g_label = "-";
std::map<uintptr_t, Block> g_blocks;
std::map<uintptr_t, size_t> g_callers;
std::set<ihipStream_t *> g_streams;
std::vector<char> g_rec_done(1, 1);
std::vector<ihipStream_t *> g_rec_stream(1, nullptr);
std::set<std::string> g_seen;
size_t g_findings = 0, g_allocs = 0;
sim::Census g_census = {};
ihipStream_t g_null;
volatile uint8_t g_sink;

uint64_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

ihipStream_t *S(hipStream_t s) { return s ? s : &g_null; }

template <class M>
typename M::const_iterator find_in(const M &m, const void *p)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    auto it = m.upper_bound(a);
    if (it == m.begin()) return m.end();
    --it;
    return it;
}

size_t block_size(const Block &b) { return b.size; }
size_t block_size(size_t b) { return b; }

// bytes from p to the end of the block that holds it; 0 if none does
template <class M>
size_t room(const M &m, const void *p)
{
    auto it = find_in(m, p);
    if (it == m.end()) return 0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), end = it->first + block_size(it->second);
    return a < end ? end - a : 0;
}

void touch(const void *p, size_t n)
{
    if (!n) return;
#if defined(__SANITIZE_ADDRESS__)
    if (!__asan_region_is_poisoned(const_cast<void *>(p), n)) return;
#endif
    const volatile uint8_t *q = static_cast<const volatile uint8_t *>(p);
    uint8_t acc = 0;
    for (size_t i = 0; i < n; ++i) acc ^= q[i];      // (ASan reports the first byte outside its allocation)
    g_sink = acc;
}

bool is_pinned(const void *p)
{
    auto it = find_in(g_blocks, p);
    return it != g_blocks.end() && room(g_blocks, p) && it->second.pinned;
}

// A host-side operand of `bytes` bytes: inside the caller's array, or a finding; then touched.
void host_operand(const void *p, size_t bytes, const char *what)
{
    if (!bytes) return;
    size_t r = room(g_callers, p);
    if (!r) r = room(g_blocks, p);
    if (r && bytes > r) {
        sim::finding("%s: the host range of %zu bytes leaves the array (%zu bytes from the pointer to its end) by %zu", what, bytes, r,
                     bytes - r);
        bytes = r;
    }
    touch(p, bytes);
}

bool step(ihipStream_t *s)
{
    if (s->q.empty()) return false;
    SimOp &h = s->q.front();
    if (h.kind == 2) {
        if (!g_rec_done[h.rec]) {
            ++g_census.waits_blocked;
            return false;
        }
        s->q.pop_front();
    } else if (h.kind == 1) {
        g_rec_done[h.rec] = 1;
        s->q.pop_front();
    } else {
        std::function<void()> fn = std::move(h.fn);
        s->q.pop_front();
        fn();
    }
    ++g_census.ops;
    return true;
}

std::vector<ihipStream_t *> all_streams()
{
    std::vector<ihipStream_t *> v(g_streams.begin(), g_streams.end());
    v.push_back(&g_null);
    return v;
}

bool random_step()
{
    std::vector<ihipStream_t *> v = all_streams(), ready;
    for (ihipStream_t *t : v)
        if (!t->q.empty() && !(t->q.front().kind == 2 && !g_rec_done[t->q.front().rec])) ready.push_back(t);
    if (ready.empty()) return false;
    return step(ready[rnd() % ready.size()]);
}

// Run until done() holds; `s` is the stream the blocking call waits for (nullptr: all of them).
void run_until(ihipStream_t *s, const std::function<bool()> &done)
{
    while (!done()) {
        bool progress = false;
        if (g_sched == sim::kRandom) {
            progress = random_step();
        } else if (g_sched == sim::kAwaitedFirst && s) {
            while (!done() && step(s)) progress = true;
            if (done()) return;
            for (ihipStream_t *t : all_streams())
                if (t != s && step(t)) {
                    progress = true;
                    break;
                }
        } else {
            for (ihipStream_t *t : all_streams())
                if (t != s)
                    while (step(t)) progress = true;
            if (s)
                while (!done() && step(s)) progress = true;
        }
        if (!progress && !done()) sim::die("deadlock: a blocking call waits for work no stream can run");
    }
}

void enqueue(hipStream_t hs, SimOp op)
{
    ihipStream_t *s = S(hs);
    if (hs && !g_streams.count(hs)) sim::die("operation queued on a stream that does not exist");
    s->q.push_back(std::move(op));
    size_t busy = 0;
    for (ihipStream_t *t : all_streams()) busy += !t->q.empty();
    if (busy > g_census.max_streams_busy) g_census.max_streams_busy = busy;
    if (g_sched == sim::kEager) {
        while (step(s)) {}
        if (!s->q.empty()) sim::die("eager schedule: a wait on a record that has not run");
    } else if (g_sched == sim::kRandom) {
        for (uint64_t k = rnd() % 3; k; --k) random_step();
    }
}

void copy_rows(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind, bool two_d, const char *what)
{
    if (!width || !height) return;
    const bool src_host = kind == hipMemcpyHostToDevice || kind == hipMemcpyHostToHost;
    const bool dst_host = kind == hipMemcpyDeviceToHost || kind == hipMemcpyHostToHost;
    const size_t sspan = (height - 1) * spitch + width, dspan = (height - 1) * dpitch + width;
    // (a 1-D copy comes here as one row: its range is its bytes on either side)
    if (src_host) host_operand(src, two_d ? height * spitch : width, what);
    else sim::dev_check(src, sspan, what);
    if (dst_host) host_operand(dst, two_d ? height * dpitch : width, what);
    else sim::dev_check(dst, dspan, what);
    for (size_t y = 0; y < height; ++y)
        memcpy(static_cast<uint8_t *>(dst) + y * dpitch, static_cast<const uint8_t *>(src) + y * spitch, width);
}

const char *kind_name(hipMemcpyKind k)
{
    return k == hipMemcpyHostToDevice ? "HostToDevice" : k == hipMemcpyDeviceToHost ? "DeviceToHost" : k == hipMemcpyDeviceToDevice ? "DeviceToDevice" : "other";
}

hipError_t queue_copy(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
                      hipStream_t stream, bool two_d, const char *api)
{
    if (kind == hipMemcpyDefault) sim::die("%s: hipMemcpyDefault is not modelled", api);
    if (height > 1 && (dpitch < width || spitch < width)) return hipErrorInvalidValue;
    const bool src_host = kind == hipMemcpyHostToDevice, dst_host = kind == hipMemcpyDeviceToHost;
    const bool caller = (src_host && !is_pinned(src)) || (dst_host && !is_pinned(dst));
    std::string what = std::string(api) + " " + kind_name(kind);
    ++g_census.copies;
    enqueue(stream, SimOp{0, [=]() { copy_rows(dst, dpitch, src, spitch, width, height, kind, two_d, what.c_str()); }, 0, caller});
    return hipSuccess;
}

void *new_block(size_t size, bool pinned)
{
    void *p = malloc(size ? size : 1);
    if (!p) sim::die("host allocation of %zu bytes failed", size);
    memset(p, g_poison, size);
    g_blocks[reinterpret_cast<uintptr_t>(p)] = Block{size, pinned};
    ++g_allocs;
    return p;
}

hipError_t free_block(void *p, bool pinned)
{
    if (!p) return hipSuccess;
    run_until(nullptr, [] { return sim::queued_ops() == 0; });   // (hipFree synchronizes the device)
    auto it = g_blocks.find(reinterpret_cast<uintptr_t>(p));
    if (it == g_blocks.end() || it->second.pinned != pinned) sim::die("free of a pointer that is no live block of this kind");
    g_blocks.erase(it);
    free(p);
    return hipSuccess;
}

}  // namespace

namespace sim {

void configure(Schedule s, uint64_t seed, uint8_t poison)
{
    if (queued_ops()) die("configure() with operations still queued");
    g_sched = s;
    g_rng = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    if (!g_rng) g_rng = 1;
    g_poison = poison;
}

void set_label(const char *label) { g_label = label; }
void caller_add(const void *p, size_t len) { g_callers[reinterpret_cast<uintptr_t>(p)] = len; }
void caller_clear() { g_callers.clear(); }

void launch(hipStream_t s, const char *, std::function<void()> fn)
{
    ++g_census.launches;
    enqueue(s, SimOp{0, std::move(fn), 0, false});
}

void dev_check(const void *p, size_t len, const char *what)
{
    if (!len) return;
    const size_t r = room(g_blocks, p);
    if (len > r) die("%s: %zu bytes at %p do not lie inside one device block (%zu bytes from the pointer to its end)", what, len, p, r);
}

void finding(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ++g_findings;
    // once per entry point and call site (the byte counts differ from case to case)
    std::string key = g_label + ": " + std::string(buf).substr(0, std::string(buf).find(':'));
    if (g_seen.insert(key).second) printf("FINDING %s: %s\n", g_label.c_str(), buf);
}

void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "hostsim: [%s] ", g_label.c_str());
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    fflush(stdout);
    abort();
}

size_t findings() { return g_findings; }
size_t alloc_count() { return g_allocs; }
size_t live_blocks() { return g_blocks.size(); }

size_t queued_ops()
{
    size_t n = g_null.q.size();
    for (ihipStream_t *t : g_streams) n += t->q.size();
    return n;
}

size_t queued_caller_ops()
{
    size_t n = 0;
    for (ihipStream_t *t : all_streams())
        for (const SimOp &o : t->q) n += o.caller;
    return n;
}

const Census &census() { return g_census; }

}  // namespace sim

extern "C" {

hipError_t hipGetDeviceCount(int *count)
{
    *count = 1;
    return hipSuccess;
}
hipError_t hipSetDevice(int device) { return device == 0 ? hipSuccess : hipErrorInvalidValue; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "simulated error"; }

hipError_t hipMalloc(void **ptr, size_t size)
{
    *ptr = new_block(size, false);
    return hipSuccess;
}
hipError_t hipFree(void *ptr) { return free_block(ptr, false); }
hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int)
{
    *ptr = new_block(size, true);
    return hipSuccess;
}
hipError_t hipHostFree(void *ptr) { return free_block(ptr, true); }

hipError_t hipHostRegister(void *ptr, size_t size, unsigned int)
{
    host_operand(ptr, size, "hipHostRegister");
    return hipSuccess;
}
hipError_t hipHostUnregister(void *) { return hipSuccess; }

hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int)
{
    *stream = new ihipStream_t();
    g_streams.insert(*stream);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream)
{
    ihipStream_t *s = S(stream);
    run_until(s, [s] { return s->q.empty(); });
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream)
{
    if (!g_streams.count(stream)) return hipErrorInvalidResourceHandle;
    hipStreamSynchronize(stream);
    g_streams.erase(stream);
    delete stream;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int)
{
    ++g_census.waits;
    if (!event->last_rec) return hipSuccess;   // never recorded: no-op
    enqueue(stream, SimOp{2, nullptr, event->last_rec, false});
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *status)
{
    *status = hipStreamCaptureStatusNone;
    return hipSuccess;
}

hipError_t hipEventCreate(hipEvent_t *event)
{
    *event = new ihipEvent_t();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned int) { return hipEventCreate(event); }
hipError_t hipEventDestroy(hipEvent_t event)
{
    delete event;   // (a queued wait holds the record's id, not the event)
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream)
{
    ++g_census.records;
    const uint64_t id = g_rec_done.size();
    g_rec_done.push_back(0);
    g_rec_stream.push_back(S(stream));
    event->last_rec = id;
    enqueue(stream, SimOp{1, nullptr, id, false});
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event)
{
    const uint64_t id = event->last_rec;
    if (!id) return hipSuccess;
    run_until(g_rec_stream[id], [id] { return g_rec_done[id] != 0; });
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t)
{
    *ms = 0.0f;
    return hipSuccess;
}

// The blocking copy: the streams of the library are non-blocking streams, which the null stream does not wait for, so nothing
// else has to run first.
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    ++g_census.copies;
    copy_rows(dst, bytes, src, bytes, bytes, 1, kind, false, "hipMemcpy");
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    return queue_copy(dst, bytes, src, bytes, bytes, 1, kind, stream, false, "hipMemcpyAsync");
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, hipMemcpyKind kind,
                            hipStream_t stream)
{
    return queue_copy(dst, dpitch, src, spitch, width, height, kind, stream, true, "hipMemcpy2DAsync");
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t stream)
{
    enqueue(stream, SimOp{0, [=]() {
                              sim::dev_check(dst, bytes, "hipMemsetAsync");
                              memset(dst, value, bytes);
                          },
                          0, false});
    return hipSuccess;
}

}  // extern "C"
