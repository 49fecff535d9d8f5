// Control interface of the simulated HIP runtime (hostsim.cpp): what the test program and the reference launches
// (sim_kernels.cpp) use beside the HIP calls themselves.  profiles/r16_host_routes.md says what is modelled and what is not.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>

namespace sim {

// Every one of these is a valid HIP execution of the same sequence of API calls.
enum Schedule {
    kEager = 0,         // each operation runs when it is queued
    kAwaitedLast = 1,   // at a blocking point every other stream first runs as far as its event waits allow
    kAwaitedFirst = 2,  // ... the awaited stream runs first, the others only as far as its waits need them
    kRandom = 3         // seeded: one operation at a time from a random runnable stream, at queueing and at blocking points
};

// A fresh run: schedule, seed (kRandom), the byte new device and pinned blocks are filled with.  Everything queued must have run.
void configure(Schedule s, uint64_t seed, uint8_t poison);
// the entry point under test, named in findings and aborts
void set_label(const char *label);

// caller memory of the case: exact-span arrays; copies are checked against them (and ASan guards their ends)
void caller_add(const void *p, size_t len);
void caller_clear();

// queue a launch on a stream; fn runs when the schedule executes it
void launch(hipStream_t s, const char *name, std::function<void()> fn);
// abort unless [p, p + len) lies inside ONE live device (or pinned) block
void dev_check(const void *p, size_t len, const char *what);

// a contract violation that does not stop the run: printed once per (label, text), counted
void finding(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
[[noreturn]] void die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

size_t findings();
size_t alloc_count();        // hipMalloc + hipHostMalloc calls so far
size_t live_blocks();
size_t queued_ops();         // operations queued on any stream
size_t queued_caller_ops();  // ... of them, copies that touch pageable host memory

struct Census {
    uint64_t ops, launches, copies, records, waits, waits_blocked, max_streams_busy;
};
const Census &census();

}  // namespace sim
