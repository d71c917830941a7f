// fake_hip.cpp — a CPU model of the 13 HIP runtime calls host_batch.cpp and csum_api.cpp make (fake_hip.h), for
// running the host batch driver under AddressSanitizer, UBSan and ThreadSanitizer without a GPU.
//
// The model gives the driver no more than the runtime's documentation does. Allocations are malloc of exactly the
// size asked, filled with garbage; a stream runs its work on a worker thread, or (Mode::kDeferred) not before it is
// synchronised; a queued copy holds pointers, not data. What the driver may not do is recorded as a violation:
// work on a stream from a thread whose current device is another, a range that leaves its block or lies on another
// device, pageable memory handed to an asynchronous copy, a block freed while queued work refers to it.
// Synchronisation is kept to what the runtime promises — a stream's own mutex orders enqueue, execution and
// synchronise; the block registry is read under a shared lock and the counters are relaxed atomics — so that
// ThreadSanitizer sees the driver's races and not this file's locks.
#include "fake_hip.h"

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <thread>

namespace {

struct Block {
    uintptr_t base;
    uint64_t size;
    int dev;
    bool host;
    std::atomic<int> refs{0};  // queued operations that refer to the block
};

struct Op {
    std::function<void()> fn;
    std::vector<Block*> refs;
};

}  // namespace

struct ihipStream_t {
    int dev = 0;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Op> q;
    uint64_t enq = 0, done = 0;
    bool stop = false, has_worker = false;
    std::thread worker;
};

namespace {

constexpr int kMaxDev = 4;
std::atomic<int> g_count{1};
std::atomic<int> g_mode{(int)fake::Mode::kThreaded};
thread_local int t_dev = 0;
thread_local hipError_t t_last = hipSuccess;

std::shared_mutex g_reg_mu;
std::map<uintptr_t, Block*> g_reg;

std::mutex g_streams_mu;
std::vector<ihipStream_t*> g_streams;

std::mutex g_viol_mu;
std::vector<std::string> g_viol;

std::atomic<uint64_t> g_ops[kMaxDev];
std::atomic<uint64_t> g_calls[(int)fake::Fn::kCount];

// the armed fault
std::atomic<int> g_fault_fn{-1};
std::atomic<int64_t> g_fault_left{0};
std::atomic<int> g_fault_err{0};
std::atomic<bool> g_fault_fired{false};

hipError_t fail(hipError_t e) {
    t_last = e;
    return e;
}

// hipSuccess, or the armed fault when this is the call it waits for.
hipError_t inject(fake::Fn f) {
    g_calls[(int)f].fetch_add(1, std::memory_order_relaxed);
    if (g_fault_fn.load(std::memory_order_relaxed) != (int)f) return hipSuccess;
    if (g_fault_left.fetch_sub(1, std::memory_order_relaxed) != 1) return hipSuccess;
    g_fault_fn.store(-1, std::memory_order_relaxed);
    g_fault_fired.store(true, std::memory_order_relaxed);
    return fail((hipError_t)g_fault_err.load(std::memory_order_relaxed));
}

// The live block that holds address p, or null. The registry lock is held shared by the caller.
Block* find_locked(const void* p) {
    const uintptr_t a = (uintptr_t)p;
    auto it = g_reg.upper_bound(a);
    if (it == g_reg.begin()) return nullptr;
    Block* b = (--it)->second;
    return a < b->base + std::max<uint64_t>(b->size, 1) ? b : nullptr;
}

bool inside(const Block* b, const void* p, uint64_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    return a >= b->base && bytes <= b->size && a - b->base <= b->size - bytes;
}

std::string hex(const void* p) {
    char s[32];
    std::snprintf(s, sizeof s, "%p", p);
    return s;
}

hipError_t alloc(void** out, size_t size, bool host) {
    if (!out) return fail(hipErrorInvalidValue);
    *out = nullptr;
    if (size == 0) return hipSuccess;
    void* p = std::malloc(size);  // exactly the size asked: the sanitizer's redzone sits at the true end
    if (!p) return fail(hipErrorOutOfMemory);
    std::memset(p, host ? 0x5A : 0xA5, size);  // nothing may lean on zeroed memory
    Block* b = new Block;
    b->base = (uintptr_t)p, b->size = size, b->dev = t_dev, b->host = host;
    std::unique_lock<std::shared_mutex> g(g_reg_mu);
    g_reg[b->base] = b;
    *out = p;
    return hipSuccess;
}

hipError_t release(void* p, bool host) {
    if (!p) return hipSuccess;
    Block* b = nullptr;
    {
        std::unique_lock<std::shared_mutex> g(g_reg_mu);
        auto it = g_reg.find((uintptr_t)p);
        if (it == g_reg.end() || it->second->host != host) {
            fake::violation(std::string(host ? "hipHostFree" : "hipFree") + " of " + hex(p) +
                            ", which is no live block of that kind");
            return fail(hipErrorInvalidValue);
        }
        b = it->second;
        g_reg.erase(it);
    }
    if (b->refs.load() > 0)
        fake::violation(std::string(host ? "hipHostFree" : "hipFree") + " of " + hex(p) +
                        " while queued work refers to it");
    std::free(p);
    delete b;
    return hipSuccess;
}

void run_op(Op& op) {
    op.fn();
    for (Block* b : op.refs) b->refs.fetch_sub(1);
}

void worker_loop(ihipStream_t* s) {
    std::unique_lock<std::mutex> l(s->mu);
    for (;;) {
        s->cv.wait(l, [&] { return s->stop || (!s->q.empty() && g_mode.load() == (int)fake::Mode::kThreaded); });
        if (s->stop) return;
        Op op = std::move(s->q.front());
        s->q.pop_front();
        l.unlock();
        run_op(op);
        l.lock();
        ++s->done;
        s->cv.notify_all();
    }
}

// Queue op on s. The issuing thread's device must be the stream's.
hipError_t push(ihipStream_t* s, Op op, const char* what) {
    if (!s) {
        fake::violation(std::string(what) + " on the null stream");
        return fail(hipErrorInvalidHandle);
    }
    if (t_dev != s->dev)
        fake::violation(std::string(what) + " on a stream of device " + std::to_string(s->dev) +
                        " from a thread whose device is " + std::to_string(t_dev));
    for (Block* b : op.refs) b->refs.fetch_add(1);
    g_ops[s->dev].fetch_add(1, std::memory_order_relaxed);
    std::lock_guard<std::mutex> l(s->mu);
    s->q.push_back(std::move(op));
    ++s->enq;
    if (g_mode.load() == (int)fake::Mode::kThreaded) {
        if (!s->has_worker) {
            s->has_worker = true;
            s->worker = std::thread(worker_loop, s);
        }
        s->cv.notify_all();
    }
    return hipSuccess;
}

}  // namespace

// ------------------------------------------------------------------ test control
namespace fake {

void set_mode(Mode m) { g_mode.store((int)m); }
void set_device_count(int n) { g_count.store(std::min(std::max(n, 1), kMaxDev)); }

void violation(const std::string& what) {
    std::lock_guard<std::mutex> g(g_viol_mu);
    g_viol.push_back(what);
}

std::vector<std::string> take_violations() {
    std::lock_guard<std::mutex> g(g_viol_mu);
    std::vector<std::string> v;
    v.swap(g_viol);
    return v;
}

uint64_t pending() {
    std::lock_guard<std::mutex> g(g_streams_mu);
    uint64_t n = 0;
    for (ihipStream_t* s : g_streams) {
        std::lock_guard<std::mutex> l(s->mu);
        n += s->enq - s->done;
    }
    return n;
}

uint64_t ops_on_device(int d) { return d >= 0 && d < kMaxDev ? g_ops[d].load() : 0; }

uint64_t live_blocks() {
    std::shared_lock<std::shared_mutex> g(g_reg_mu);
    return g_reg.size();
}

void reset_counters() {
    for (auto& c : g_ops) c.store(0);
    for (auto& c : g_calls) c.store(0);
}

uint64_t calls(Fn f) { return g_calls[(int)f].load(); }

void fail_nth(Fn f, uint64_t k, hipError_t e) {
    g_fault_fn.store(-1);
    g_fault_fired.store(false);
    g_fault_left.store((int64_t)k);
    g_fault_err.store((int)e);
    g_fault_fn.store((int)f);
}

bool fault_fired() { return g_fault_fired.load(); }
void disarm() { g_fault_fn.store(-1); }

void shutdown() {
    std::lock_guard<std::mutex> g(g_streams_mu);
    for (ihipStream_t* s : g_streams) {
        {
            std::lock_guard<std::mutex> l(s->mu);
            s->stop = true;
            s->cv.notify_all();
        }
        if (s->has_worker) s->worker.join();
        delete s;
    }
    g_streams.clear();
}

bool device_range(hipStream_t st, const void* p, uint64_t bytes, const char* what) {
    if (bytes == 0) return true;
    std::shared_lock<std::shared_mutex> g(g_reg_mu);
    const Block* b = find_locked(p);
    if (st && b && !b->host && b->dev == st->dev && inside(b, p, bytes)) return true;
    violation(std::string(what) + ": [" + hex(p) + ", +" + std::to_string(bytes) +
              ") is not inside one live block of " +
              (st ? "device " + std::to_string(st->dev) : std::string("a stream's device")));
    return false;
}

hipError_t enqueue(hipStream_t st, std::vector<const void*> blocks, std::function<void()> fn) {
    Op op;
    op.fn = std::move(fn);
    {
        std::shared_lock<std::shared_mutex> g(g_reg_mu);
        for (const void* p : blocks)
            if (p)
                if (Block* b = find_locked(p)) op.refs.push_back(b);
    }
    return push(st, std::move(op), "a launch");
}

}  // namespace fake

// ------------------------------------------------------------------ the 13 runtime calls
hipError_t hipGetDeviceCount(int* count) {
    if (!count) return fail(hipErrorInvalidValue);
    *count = g_count.load();
    return hipSuccess;
}

hipError_t hipSetDevice(int deviceId) {
    if (hipError_t e = inject(fake::Fn::kSetDevice)) return e;
    if (deviceId < 0 || deviceId >= g_count.load()) return fail(hipErrorInvalidDevice);
    t_dev = deviceId;
    return hipSuccess;
}

hipError_t hipGetDevice(int* deviceId) {
    if (!deviceId) return fail(hipErrorInvalidValue);
    *deviceId = t_dev;
    return hipSuccess;
}

hipError_t hipDeviceGetAttribute(int* pi, hipDeviceAttribute_t attr, int deviceId) {
    if (!pi || attr != hipDeviceAttributeMultiprocessorCount) return fail(hipErrorInvalidValue);
    if (deviceId < 0 || deviceId >= g_count.load()) return fail(hipErrorInvalidDevice);
    *pi = fake::kCus;
    return hipSuccess;
}

hipError_t hipGetLastError(void) {
    const hipError_t e = t_last;
    t_last = hipSuccess;
    return e;
}

hipError_t hipMalloc(void** ptr, size_t size) {
    if (hipError_t e = inject(fake::Fn::kMalloc)) return e;
    return alloc(ptr, size, false);
}

hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) {
    if (hipError_t e = inject(fake::Fn::kHostMalloc)) return e;
    return alloc(ptr, size, true);
}

hipError_t hipFree(void* ptr) { return release(ptr, false); }
hipError_t hipHostFree(void* ptr) { return release(ptr, true); }

hipError_t hipPointerGetAttributes(hipPointerAttribute_t* attributes, const void* ptr) {
    if (!attributes) return fail(hipErrorInvalidValue);
    std::shared_lock<std::shared_mutex> g(g_reg_mu);
    const Block* b = find_locked(ptr);
    if (!b) return fail(hipErrorInvalidValue);  // ordinary memory: the runtime knows nothing of it
    std::memset(attributes, 0, sizeof *attributes);
    attributes->type = b->host ? hipMemoryTypeHost : hipMemoryTypeDevice;
    attributes->device = b->dev;
    attributes->devicePointer = const_cast<void*>(ptr);
    attributes->hostPointer = b->host ? const_cast<void*>(ptr) : nullptr;
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int) {
    if (hipError_t e = inject(fake::Fn::kStreamCreate)) return e;
    if (!stream) return fail(hipErrorInvalidValue);
    ihipStream_t* s = new ihipStream_t;
    s->dev = t_dev;
    std::lock_guard<std::mutex> g(g_streams_mu);
    g_streams.push_back(s);
    *stream = s;
    return hipSuccess;
}

hipError_t hipStreamSynchronize(hipStream_t s) {
    if (!s) return fail(hipErrorInvalidHandle);
    std::unique_lock<std::mutex> l(s->mu);
    while (s->done != s->enq) {
        if (g_mode.load() == (int)fake::Mode::kDeferred && !s->q.empty()) {
            Op op = std::move(s->q.front());  // deferred work runs now, in order, on this thread
            s->q.pop_front();
            l.unlock();
            run_op(op);
            l.lock();
            ++s->done;
            s->cv.notify_all();
        } else {
            s->cv.wait(l);
        }
    }
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
    if (hipError_t e = inject(fake::Fn::kMemcpyAsync)) return e;
    if (bytes == 0) return hipSuccess;
    if (!s || (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToHost)) {
        fake::violation("hipMemcpyAsync on the null stream or of a kind the driver does not use");
        return fail(hipErrorInvalidValue);
    }
    const bool h2d = kind == hipMemcpyHostToDevice;
    const void* dptr = h2d ? dst : src;
    const void* hptr = h2d ? src : dst;
    Op op;
    {
        std::shared_lock<std::shared_mutex> g(g_reg_mu);
        Block* d = find_locked(dptr);
        Block* h = find_locked(hptr);
        std::string bad;
        if (!d || d->host || !inside(d, dptr, bytes))
            bad = "device side [" + hex(dptr) + ", +" + std::to_string(bytes) + ") is not inside one live device block";
        else if (d->dev != s->dev)
            bad = "device memory of device " + std::to_string(d->dev) + " on a stream of device " +
                  std::to_string(s->dev);
        else if (!h || !h->host)
            bad = "host side " + hex(hptr) + " is not pinned memory";
        else if (!inside(h, hptr, bytes))
            bad = "host side [" + hex(hptr) + ", +" + std::to_string(bytes) + ") leaves its pinned block";
        if (!bad.empty()) {
            fake::violation(std::string("hipMemcpyAsync ") + (h2d ? "H2D: " : "D2H: ") + bad);
            return fail(hipErrorInvalidValue);
        }
        op.refs = {d, h};
    }
    op.fn = [=] { std::memcpy(dst, src, bytes); };  // the pointers are captured, not the data
    return push(s, std::move(op), "hipMemcpyAsync");
}
