// fake_hip.h — test control of the CPU model of the HIP runtime in fake_hip.cpp: the 13 runtime calls that
// network-stack_amd/csrc/host_batch.cpp and csum_api.cpp make, modelled as an adversary (exact-size garbage-filled
// allocations, streams that run as late as the API allows, every device / range / lifetime rule checked and
// recorded). Used only by tests/cpp/test_host_batch.cpp and tests/cpp/cpu_launchers.cpp; nothing here touches a GPU.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

namespace fake {

// How queued stream work runs.
enum class Mode {
    kThreaded,  // a worker thread per stream drains its FIFO; hipStreamSynchronize waits for it
    kDeferred,  // nothing runs before its stream is synchronised; then in order, on the synchronising thread
};
// Streams must be idle. Streams made under one mode keep working under the other.
void set_mode(Mode m);
void set_device_count(int n);  // 1..4
constexpr int kCus = 256;      // hipDeviceAttributeMultiprocessorCount of every device

// ---- what the model saw ----
// Violations recorded since the last call, oldest first; clears them.
std::vector<std::string> take_violations();
void violation(const std::string& what);
uint64_t pending();            // operations queued on any stream and not yet complete
uint64_t ops_on_device(int d);  // copies and launches queued on streams of device d since reset_counters()
uint64_t live_blocks();        // hipMalloc / hipHostMalloc blocks not yet freed
void reset_counters();         // ops_on_device and calls()

// ---- fault injection: an error code out of the model, nothing more ----
enum class Fn { kMalloc, kHostMalloc, kMemcpyAsync, kStreamCreate, kSetDevice, kCount };
uint64_t calls(Fn f);  // calls of f since reset_counters()
// The k-th next call of f (k = 1: the next), from whichever thread, returns e and does nothing else. One fault is
// armed at a time; disarm() withdraws it.
void fail_nth(Fn f, uint64_t k, hipError_t e);
bool fault_fired();
void disarm();

// Joins the stream workers and frees the streams, so that LeakSanitizer's report is about the code under test.
// No runtime call may follow.
void shutdown();

// ---- for the launcher stand-ins (cpu_launchers.cpp) ----
// True when [p, p + bytes) lies inside one live device block of st's device; records a violation otherwise.
bool device_range(hipStream_t st, const void* p, uint64_t bytes, const char* what);
// Queue fn on st: checked for the issuing thread's device like a copy; `blocks` are device pointers the work refers
// to (null entries skipped), which must not be freed before it has run.
hipError_t enqueue(hipStream_t st, std::vector<const void*> blocks, std::function<void()> fn);

}  // namespace fake
