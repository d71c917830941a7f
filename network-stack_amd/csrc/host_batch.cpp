// host_batch.cpp — host-resident batches: shard over GPUs, pipeline per GPU.
//
// The reference's checksum input lives in transport buffers in host memory
// (transport/pipe/pipe.go:73-124 hands []byte slices between goroutines), so the
// end-to-end path is host → HBM → kernel → host. There is one pipeline and there are two jobs.
// run_shards gives each GPU contiguous shards (no collective: segments are independent) and each shard a host
// thread; run_chunks double-buffers the shard's chunks over two HIP streams, so chunk k+1's H2D copy overlaps
// chunk k's kernel and D2H. What a chunk copies and launches is the job's: CsumJob (fixed-stride and ragged
// checksums, the receive pass) or SenderJob (TCP images, datagrams, segmentation offload). Everything decided
// before the first copy — validation, shard bounds, chunk cuts, staging layout — is host_plan.h's. Caller memory
// that is already pinned (nsx_alloc_pinned) is DMA'd directly; pageable memory is bounced through pinned staging
// buffers (multi-threaded copy, stage_copy). Streams and buffers persist per device (DevCtx).
// NSX_HOST_EXACT_BUFFERS (never defined by the product build) makes every staging buffer exactly as large as was
// reserved, for tests/test_host_batch_cpp.py, which runs this file on a CPU model of HIP under sanitizers.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_tune.h"
#include "api_util.h"
#include "csum_kernels.h"
#include "host_plan.h"

namespace {

using nsx::Chunk;
using nsx::Cut;

// Pageable caller memory is bounced through pinned staging; one thread's memcpy (~10-25 GB/s) would
// then, not PCIe, set the end-to-end rate. Large copies are split over up to kCopyThreads threads
// (NSX_HOST_COPY_THREADS overrides; 1 = serial).
constexpr int kCopyThreads = 8;
constexpr uint64_t kCopySplitMin = 4ull << 20;

int copy_threads() {
    static const int n = [] {
        const char* e = std::getenv("NSX_HOST_COPY_THREADS");
        int v = e ? std::atoi(e) : 0;
        if (v < 1) v = std::min<int>(kCopyThreads, (int)std::max(1u, std::thread::hardware_concurrency()));
        return std::min(v, 64);
    }();
    return n;
}

void stage_copy(void* dst, const void* src, uint64_t bytes) {
    const int nt = bytes >= kCopySplitMin ? copy_threads() : 1;
    if (nt <= 1) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const uint64_t part = ((bytes + nt - 1) / nt + 4095) & ~4095ull;  // page-sized pieces
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) {
        const uint64_t lo = part * t;
        if (lo >= bytes) break;
        th.emplace_back([=] { std::memcpy((uint8_t*)dst + lo, (const uint8_t*)src + lo, std::min(part, bytes - lo)); });
    }
    std::memcpy(dst, src, std::min(part, bytes));
    for (auto& x : th) x.join();
}

bool is_pinned(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// A step's first HIP error goes back to run_chunks.
#define NSX_CHECK(expr) do { if (hipError_t e_ = (expr)) return e_; } while (0)

// Per-device resources reused across calls: the transport calls the host
// batch API once per received batch (tools/loopback.cpp), so stream creation,
// hipMalloc and hipHostMalloc (page registration) must not sit on every call —
// they cost milliseconds against a ~100 KB batch's tens of microseconds.
// Buffers only grow; nsx_host_cache_release() frees them. Calls on the same
// device serialise on the context's mutex (each call already fills the GPU's
// copy engines with its own double-buffered chunks).
template <bool kHost>
struct Grow {
    void* p = nullptr;
    uint64_t cap = 0;
    hipError_t ensure(uint64_t bytes) {
        if (bytes <= cap) return hipSuccess;
        release();
#ifdef NSX_HOST_EXACT_BUFFERS
        const uint64_t c = bytes;  // the sanitizer builds: a buffer reserved a byte short is a report
#else
        uint64_t c = 4096;
        while (c < bytes) c <<= 1;
#endif
        const hipError_t e = kHost ? hipHostMalloc(&p, c, hipHostMallocPortable) : hipMalloc(&p, c);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        cap = c;
        return hipSuccess;
    }
    void release() {
        if (p) (void)(kHost ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

// A device buffer and the pinned host buffer that stages it.
struct Staged {
    Grow<false> d;
    Grow<true> h;
    hipError_t ensure(uint64_t bytes) {
        NSX_CHECK(d.ensure(bytes));
        return h.ensure(bytes);
    }
    void release() { d.release(), h.release(); }
};

struct DevCtx {
    std::mutex mu;
    hipStream_t st[2] = {nullptr, nullptr};
    // per slot: data and out are staged only for pageable caller memory (their h sides grow on demand)
    Staged data[2], out[2], part[2], off[2];
    Staged fields[2], opts[2], raw[2];  // the sender job also stages header fields, options and raw sums
    void release() {
        for (int s = 0; s < 2; ++s) {
            data[s].release(), out[s].release(), part[s].release(), off[s].release();
            fields[s].release(), opts[s].release(), raw[s].release();
        }
    }
};

constexpr int kMaxDevices = 64;
constexpr int kMaxSlots = 8;  // nsx_tune.shards_per_device ≤ this
std::mutex g_ctx_mu;
DevCtx* g_ctx[kMaxDevices][kMaxSlots] = {};  // never destroyed: HIP may be torn down before static destructors run

DevCtx* dev_ctx(int dev, int slot) {
    if (dev < 0 || dev >= kMaxDevices || slot < 0 || slot >= kMaxSlots) return nullptr;
    std::lock_guard<std::mutex> g(g_ctx_mu);
    if (!g_ctx[dev][slot]) g_ctx[dev][slot] = new DevCtx;
    return g_ctx[dev][slot];
}

// What every job carries: the caller's tune and, set by run_shards, its shard.
struct Shard {
    const nsx_tune* tune = nullptr;
    uint64_t lo = 0, hi = 0;  // segment (or super-segment) range
    int dev = 0, slot = 0;    // slot: the shard's own DevCtx on the device (streams + staging)
    uint64_t budget() const { return tune && tune->chunk_bytes > 0 ? (uint64_t)tune->chunk_bytes : nsx::kChunkBytes; }
};

// The chunk pipeline of one shard. A job supplies plan() (its chunks; it also sizes its buffers there),
// reserve(ctx, s) (slot s's buffers), issue(ctx, s, chunk, cfg) (the chunk's H2D copies, launch and D2H copies on
// stream s) and finish(ctx, s, chunk) (the chunk's results, complete on the device, into caller memory).
template <class Job>
int run_chunks(Job& job) {
    const std::vector<Chunk> chunks = job.plan();
    const int nslots = chunks.size() > 1 ? 2 : 1;
    DevCtx* ctx = dev_ctx(job.dev, job.slot);
    if (!ctx) return NSX_EINVAL;
    std::lock_guard<std::mutex> hold(ctx->mu);
    hipStream_t* st = ctx->st;
    const auto pipeline = [&]() -> hipError_t {
        const Chunk* pending[2] = {nullptr, nullptr};
        NSX_CHECK(hipSetDevice(job.dev));
        const int cus = nsx::device_cus(job.dev);
        if (cus <= 0) return hipErrorNoDevice;
        const nsx::LaunchCfg cfg = nsx::launch_cfg(cus, job.tune);
        for (int s = 0; s < nslots; ++s) {
            if (!st[s]) NSX_CHECK(hipStreamCreateWithFlags(&st[s], hipStreamNonBlocking));
            NSX_CHECK(job.reserve(*ctx, s));
        }
        for (size_t k = 0; k < chunks.size(); ++k) {
            const int s = (int)(k % nslots);
            if (pending[s]) {  // slot reuse: finish chunk k-2
                NSX_CHECK(hipStreamSynchronize(st[s]));
                job.finish(*ctx, s, *pending[s]);
            }
            NSX_CHECK(job.issue(*ctx, s, chunks[k], cfg));
            pending[s] = &chunks[k];
        }
        for (int s = 0; s < nslots; ++s) {
            NSX_CHECK(hipStreamSynchronize(st[s]));
            if (pending[s]) job.finish(*ctx, s, *pending[s]);
        }
        return hipSuccess;
    };
    const hipError_t e = pipeline();
    if (e != hipSuccess)  // leave the streams idle for the next call
        for (int s = 0; s < 2; ++s)
            if (st[s]) (void)hipStreamSynchronize(st[s]);
    return nsx::map_err(e);
}

// Shards: num_gpus × shards_per_device contiguous ranges of the n segments, balanced by `offsets` (by count without);
// shard g runs on device g / shards_per_device in slot g % shards_per_device, one host thread per shard. `bytes`
// sizes an auto call (num_gpus <= 0); align64 starts every shard on a 64-frame mask word.
template <class Job>
int run_shards(const Job& proto, const uint64_t* offsets, uint64_t n, uint64_t bytes, bool align64, int num_gpus) {
    const int count = nsx::device_count();
    if (count <= 0) return NSX_ENODEV;
    if (num_gpus <= 0) num_gpus = nsx::auto_gpus(bytes, count);
    if (num_gpus > count) return NSX_ENODEV;
    const nsx_tune* tune = proto.tune;
    const int spd = (tune && tune->shards_per_device > 1) ? std::min(tune->shards_per_device, kMaxSlots) : 1;
    int caller_dev = 0;
    (void)hipGetDevice(&caller_dev);
    const int parts = (int)std::min<uint64_t>((uint64_t)num_gpus * spd, n);
    const std::vector<uint64_t> bounds = nsx::shard_bounds(offsets, n, parts, align64);
    std::vector<Job> jobs(parts, proto);
    std::vector<int> rc(parts, NSX_OK);
    for (int g = 0; g < parts; ++g)
        jobs[g].lo = bounds[g], jobs[g].hi = bounds[g + 1], jobs[g].dev = g / spd, jobs[g].slot = g % spd;
    const auto run = [&](int g) { rc[g] = run_chunks(jobs[g]); };
    std::vector<std::thread> th;
    for (int g = 1; g < parts; ++g)
        if (jobs[g].hi > jobs[g].lo) th.emplace_back(run, g);
    if (jobs[0].hi > jobs[0].lo) run(0);
    for (auto& t : th) t.join();
    (void)hipSetDevice(caller_dev);
    for (int r : rc)
        if (r != NSX_OK) return r;
    return NSX_OK;
}

// ---- the checksum job: fixed-stride and ragged raw sums, and the receive pass's validity mask ----
struct CsumJob : Shard {
    Cut mode = Cut::kFixed;
    const uint8_t* base = nullptr;
    uint64_t stride = 0;  // fixed stride
    uint32_t seg_len = 0;
    const uint64_t* offsets = nullptr;  // ragged and receive: absolute offsets into base
    const uint32_t* partial = nullptr;  // nullable
    uint16_t* out = nullptr;            // one raw sum per segment
    uint64_t* mask = nullptr;           // receive: one validity bit per frame (a chunk's c0 is a multiple of 64)
    int ipver = 0;                      // receive: 4 or 6
    // set by plan()
    uint64_t max_span = 0, max_segs = 0;
    bool in_pinned = false, out_pinned = false;

    bool rx() const { return mode == Cut::kRx; }
    uint64_t out_bytes(uint64_t cn) const { return rx() ? (cn + 63) / 64 * 8 : cn * sizeof(uint16_t); }
    uint8_t* out_host(uint64_t c0) const {
        return rx() ? reinterpret_cast<uint8_t*>(mask + c0 / 64) : reinterpret_cast<uint8_t*>(out + c0);
    }

    std::vector<Chunk> plan() {
        const std::vector<Chunk> chunks = nsx::plan_chunks(mode, offsets, stride, seg_len, lo, hi, budget());
        for (const Chunk& c : chunks) {
            max_span = std::max(max_span, c.byte_hi - c.byte_lo);
            max_segs = std::max(max_segs, c.c1 - c.c0);
        }
        in_pinned = is_pinned(base);
        out_pinned = is_pinned(out_host(lo));
        return chunks;
    }

    hipError_t reserve(DevCtx& ctx, int s) const {
        NSX_CHECK(ctx.data[s].d.ensure(std::max<uint64_t>(max_span, 16)));
        NSX_CHECK(ctx.out[s].d.ensure(std::max<uint64_t>(out_bytes(max_segs), 8)));
        if (partial) NSX_CHECK(ctx.part[s].ensure(max_segs * sizeof(uint32_t)));
        if (offsets) NSX_CHECK(ctx.off[s].ensure((max_segs + 1) * sizeof(uint64_t)));
        if (!in_pinned) NSX_CHECK(ctx.data[s].h.ensure(std::max<uint64_t>(max_span, 16)));
        if (!out_pinned) NSX_CHECK(ctx.out[s].h.ensure(std::max<uint64_t>(out_bytes(max_segs), 8)));
        return hipSuccess;
    }

    hipError_t issue(DevCtx& ctx, int s, const Chunk& c, const nsx::LaunchCfg& cfg) const {
        hipStream_t st = ctx.st[s];
        const uint64_t cn = c.c1 - c.c0, span = c.byte_hi - c.byte_lo;
        uint8_t* d_data = ctx.data[s].d.as<uint8_t>();
        uint16_t* d_out = ctx.out[s].d.as<uint16_t>();
        uint32_t* d_part = partial ? ctx.part[s].d.as<uint32_t>() : nullptr;
        const uint8_t* src = base + c.byte_lo;
        if (!in_pinned) {
            stage_copy(ctx.data[s].h.p, src, span);
            src = ctx.data[s].h.as<uint8_t>();
        }
        if (span) NSX_CHECK(hipMemcpyAsync(d_data, src, span, hipMemcpyHostToDevice, st));
        if (partial) {
            std::memcpy(ctx.part[s].h.p, partial + c.c0, cn * sizeof(uint32_t));
            NSX_CHECK(hipMemcpyAsync(d_part, ctx.part[s].h.p, cn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        if (offsets) {
            uint64_t* h_off = ctx.off[s].h.as<uint64_t>();
            uint64_t* d_off = ctx.off[s].d.as<uint64_t>();
            for (uint64_t i = 0; i <= cn; ++i) h_off[i] = offsets[c.c0 + i] - c.byte_lo;
            NSX_CHECK(hipMemcpyAsync(d_off, h_off, (cn + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            NSX_CHECK(rx() ? nsx::launch_rx_tcp(cfg, ipver, d_data, d_off, cn, reinterpret_cast<uint64_t*>(d_out),
                                                nullptr, nullptr, st)
                           : nsx::launch_ragged(cfg, d_data, d_off, cn, d_part, d_out, nullptr, st));
        } else {
            NSX_CHECK(nsx::launch_fixed(cfg, d_data, stride, seg_len, cn, d_part, d_out, st));
        }
        uint8_t* out_dst = out_pinned ? out_host(c.c0) : ctx.out[s].h.as<uint8_t>();
        return hipMemcpyAsync(out_dst, d_out, out_bytes(cn), hipMemcpyDeviceToHost, st);
    }

    void finish(DevCtx& ctx, int s, const Chunk& c) const {
        if (!out_pinned) std::memcpy(out_host(c.c0), ctx.out[s].h.p, out_bytes(c.c1 - c.c0));
    }
};

// ---- the sender job: the fused sender pass over host-resident segments ----
// A Go transport's send loop builds segments (tcp.go:98-128), stores ^sum at bytes 16-17 (tcp.go:110, :68-71) and
// writes the images into its pipe or socket buffers (transport/pipe/pipe.go:92-124): header fields, options and
// payloads start in host memory and the wire images end there. Per chunk: the fields (one pinned block of 256 B-
// aligned sub-arrays, host_plan.h's FieldSet), the rebased offsets (OffBlock), the option and payload spans and the
// partials go H2D, the build kernel runs, and the image span and raw sums come back; lead_data / lead_out keep the
// staged payload's and the image span's byte offsets mod 256. TCP images: ip null. Datagrams: the six nsx_ip_hdr_soa
// arrays ride in the field block behind the TCP fields. Segmentation offload (tso): shards and chunks are ranges of
// super-segments [c0, c1), whose fields (their mss a 15th array), options and payload are staged once each; the
// chunk's frames [frame_first[c0], frame_first[c1]) own its image span and raw sums, and the frame map goes along
// rebased — frame_first less frame_first[c0], frame_seg rebuilt from it as chunk-local indices.
struct SenderJob : Shard {
    const nsx_ip_hdr_soa* ip = nullptr;  // host arrays; null = TCP images only
    int ipver = 0;                       // 4 or 6 with ip
    nsx::FieldSet fields{};              // host arrays of the header fields (and the mss)
    const uint8_t* opts = nullptr;
    const uint64_t* opt_off = nullptr;  // nullable
    const uint8_t* data = nullptr;
    const uint64_t* data_off = nullptr;
    const uint32_t* partial = nullptr;  // nullable
    uint8_t* out = nullptr;
    const uint64_t* out_off = nullptr;  // per frame
    uint16_t* raw = nullptr;            // per frame, nullable
    bool gaps = false;  // some image slot is longer than its 4-padded image: the caller's bytes there are preserved
    bool tso = false;   // segmentation offload: every array above but out_off and raw is per super-segment
    const uint64_t* frame_first = nullptr;  // tso: n + 1
    const uint64_t* seg_out = nullptr;      // image offset of each segment's / super-segment's first frame (n + 1):
                                            // what shards and chunks are cut by; out_off itself without tso
    // set by plan()
    uint64_t max_out = 0, max_data = 0, max_opt = 0, max_segs = 0, max_frames = 0;
    bool in_pinned = false, out_pinned = false;

    // the frames of segments [c0, c1): the segments themselves without segmentation
    uint64_t frame_at(uint64_t c) const { return tso ? frame_first[c] : c; }

    std::vector<Chunk> plan() {
        const std::vector<Chunk> chunks = nsx::plan_sender_chunks(seg_out, data_off, lo, hi, budget());
        for (const Chunk& c : chunks) {
            max_out = std::max(max_out, c.byte_hi - c.byte_lo);
            max_data = std::max(max_data, data_off[c.c1] - data_off[c.c0]);
            if (opt_off) max_opt = std::max(max_opt, opt_off[c.c1] - opt_off[c.c0]);
            max_segs = std::max(max_segs, c.c1 - c.c0);
            max_frames = std::max(max_frames, frame_at(c.c1) - frame_at(c.c0));
        }
        in_pinned = is_pinned(data);
        out_pinned = is_pinned(out);
        return chunks;
    }

    hipError_t reserve(DevCtx& ctx, int s) const {
        uint64_t at[nsx::kAllFields];
        NSX_CHECK(ctx.data[s].d.ensure(512 + max_data + 16));
        NSX_CHECK(ctx.out[s].d.ensure(256 + max_out + 16));
        NSX_CHECK(ctx.fields[s].ensure(nsx::field_block(fields, max_segs, at)));
        NSX_CHECK(ctx.off[s].ensure(nsx::off_block(max_segs, max_frames, opt_off, tso).words * sizeof(uint64_t)));
        NSX_CHECK(ctx.raw[s].ensure(std::max<uint64_t>(max_frames * sizeof(uint16_t), 16)));
        if (partial) NSX_CHECK(ctx.part[s].ensure(max_segs * sizeof(uint32_t)));
        if (opt_off) NSX_CHECK(ctx.opts[s].ensure(max_opt + 16));
        if (!in_pinned) NSX_CHECK(ctx.data[s].h.ensure(max_data + 16));
        if (!out_pinned) NSX_CHECK(ctx.out[s].h.ensure(256 + max_out + 16));
        return hipSuccess;
    }

    // The chunk's offsets, rebased to the staged spans, into the slot's pinned offset block.
    void stage_offsets(uint64_t* ho, const nsx::OffBlock& ob, const Chunk& c, uint64_t lead_d, uint64_t lead_o) const {
        const uint64_t cn = c.c1 - c.c0, f0 = frame_at(c.c0), fn = frame_at(c.c1) - f0;
        for (uint64_t i = 0; i <= cn; ++i) {
            ho[i] = data_off[c.c0 + i] - data_off[c.c0] + lead_d;
            if (opt_off) ho[ob.at_opt + i] = opt_off[c.c0 + i] - opt_off[c.c0];
            if (tso) ho[ob.at_first + i] = frame_first[c.c0 + i] - f0;
        }
        for (uint64_t i = 0; i <= fn; ++i) ho[ob.at_out + i] = out_off[f0 + i] - c.byte_lo + lead_o;
        if (!tso) return;
        uint32_t* seg = reinterpret_cast<uint32_t*>(ho + ob.at_seg);
        for (uint64_t i = 0; i < cn; ++i)
            for (uint64_t f = frame_first[c.c0 + i]; f < frame_first[c.c0 + i + 1]; ++f) seg[f - f0] = (uint32_t)i;
    }

    hipError_t issue(DevCtx& ctx, int s, const Chunk& c, const nsx::LaunchCfg& cfg) const {
        hipStream_t st = ctx.st[s];
        const uint64_t cn = c.c1 - c.c0, span_o = c.byte_hi - c.byte_lo, fn = frame_at(c.c1) - frame_at(c.c0);
        const uint64_t d0 = data_off[c.c0], span_d = data_off[c.c1] - d0;
        const uint64_t lead_d = nsx::lead_data(d0), lead_o = nsx::lead_out(c.byte_lo);
        // header fields: the sub-arrays in one pinned block, one copy
        uint8_t* hf = ctx.fields[s].h.as<uint8_t>();
        uint64_t at[nsx::kAllFields];
        const uint64_t fbytes = nsx::field_block(fields, cn, at);
        for (int f = 0; f < fields.n; ++f)
            if (fields.src[f])
                std::memcpy(hf + at[f], (const uint8_t*)fields.src[f] + c.c0 * fields.esz[f], cn * fields.esz[f]);
        NSX_CHECK(hipMemcpyAsync(ctx.fields[s].d.p, hf, fbytes, hipMemcpyHostToDevice, st));
        nsx_tcp_hdr_soa d_tcp;
        nsx_ip_hdr_soa d_ip;
        const uint32_t* d_mss;
        nsx::field_block_soa(fields, at, ctx.fields[s].d.as<uint8_t>(), &d_tcp, &d_ip, &d_mss);
        // offsets
        const nsx::OffBlock ob = nsx::off_block(cn, fn, opt_off, tso);
        uint64_t* dofs = ctx.off[s].d.as<uint64_t>();
        stage_offsets(ctx.off[s].h.as<uint64_t>(), ob, c, lead_d, lead_o);
        NSX_CHECK(hipMemcpyAsync(dofs, ctx.off[s].h.p, ob.words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        const uint8_t* d_opts = nullptr;
        if (opt_off) {
            const uint64_t ospan = opt_off[c.c1] - opt_off[c.c0];
            if (ospan) {
                std::memcpy(ctx.opts[s].h.p, opts + opt_off[c.c0], ospan);
                NSX_CHECK(hipMemcpyAsync(ctx.opts[s].d.p, ctx.opts[s].h.p, ospan, hipMemcpyHostToDevice, st));
            }
            d_opts = ctx.opts[s].d.as<uint8_t>();
        }
        // payloads
        uint8_t* d_data = ctx.data[s].d.as<uint8_t>();
        const uint8_t* src = data + d0;
        if (!in_pinned && span_d) {
            stage_copy(ctx.data[s].h.p, src, span_d);
            src = ctx.data[s].h.as<uint8_t>();
        }
        if (span_d) NSX_CHECK(hipMemcpyAsync(d_data + lead_d, src, span_d, hipMemcpyHostToDevice, st));
        uint32_t* d_part = nullptr;
        if (partial) {
            std::memcpy(ctx.part[s].h.p, partial + c.c0, cn * sizeof(uint32_t));
            d_part = ctx.part[s].d.as<uint32_t>();
            NSX_CHECK(hipMemcpyAsync(d_part, ctx.part[s].h.p, cn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        }
        uint8_t* d_out = ctx.out[s].d.as<uint8_t>();
        uint8_t* out_dst = out_pinned ? out + c.byte_lo : ctx.out[s].h.as<uint8_t>() + lead_o;
        if (gaps && span_o) {  // the caller's bytes between images stay as they are
            if (!out_pinned) stage_copy(out_dst, out + c.byte_lo, span_o);
            NSX_CHECK(hipMemcpyAsync(d_out + lead_o, out_dst, span_o, hipMemcpyHostToDevice, st));
        }
        const nsx::IpHdrSoA ipd = nsx::to_soa(d_ip);
        const uint64_t* d_opt_off = opt_off ? dofs + ob.at_opt : nullptr;
        uint16_t* d_raw = raw ? ctx.raw[s].d.as<uint16_t>() : nullptr;
        if (tso) {
            const nsx::TsoMap map{d_mss, dofs + ob.at_first, reinterpret_cast<const uint32_t*>(dofs + ob.at_seg)};
            NSX_CHECK(nsx::launch_tso_build(cfg, ipver, ipd, map, nsx::to_soa(d_tcp), d_opts, d_opt_off, d_data, dofs,
                                            lead_d + span_d, fn, d_out, dofs + ob.at_out, d_raw, st));
        } else {
            NSX_CHECK(nsx::launch_tcp_build(cfg, ipver, ip ? &ipd : nullptr, nsx::to_soa(d_tcp), d_opts, d_opt_off,
                                            d_data, dofs, lead_d + span_d, d_part, cn, d_out, dofs + ob.at_out, d_raw,
                                            st));
        }
        if (span_o) NSX_CHECK(hipMemcpyAsync(out_dst, d_out + lead_o, span_o, hipMemcpyDeviceToHost, st));
        if (raw) NSX_CHECK(hipMemcpyAsync(ctx.raw[s].h.p, d_raw, fn * sizeof(uint16_t), hipMemcpyDeviceToHost, st));
        return hipSuccess;
    }

    void finish(DevCtx& ctx, int s, const Chunk& c) const {
        // the images back into pageable caller memory: the same multi-threaded copy as the payloads' way in (one
        // thread's memcpy held the pageable build at 31.7 GB/s of PCIe traffic against 54.3 pinned)
        if (!out_pinned)
            stage_copy(out + c.byte_lo, ctx.out[s].h.as<uint8_t>() + nsx::lead_out(c.byte_lo), c.byte_hi - c.byte_lo);
        if (raw)
            std::memcpy(raw + frame_at(c.c0), ctx.raw[s].h.p, (frame_at(c.c1) - frame_at(c.c0)) * sizeof(uint16_t));
    }
};

int csum_host(Cut mode, int ipver, const uint8_t* h_base, uint64_t stride, uint32_t seg_len, const uint64_t* h_offsets,
              uint64_t n, const uint32_t* h_partial, uint16_t* h_out, uint64_t* h_mask, int num_gpus,
              const nsx_tune* tune) {
    CsumJob j;
    j.tune = tune;
    j.mode = mode, j.ipver = ipver;
    j.base = h_base, j.stride = stride, j.seg_len = seg_len, j.offsets = h_offsets;
    j.partial = h_partial, j.out = h_out, j.mask = h_mask;
    const uint64_t bytes = h_offsets ? h_offsets[n] - h_offsets[0] : n * std::max<uint64_t>(stride, seg_len);
    return run_shards(j, h_offsets, n, bytes, mode == Cut::kRx, num_gpus);
}

// nsx_tcp_build_host (ip null), the transmit pass's host calls (ip + ipver) and the segmentation offload's (h_mss
// and the frame map; tso): everything the chunks rely on is checked here, before any copy, then the sharded job.
int sender_host(bool tso, const nsx_ip_hdr_soa* ip, int ipver, const nsx_tcp_hdr_soa* h_hdr, const uint8_t* h_opts,
                const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                const uint32_t* h_prefix_partial, const uint32_t* h_mss, uint64_t n, const uint64_t* h_frame_first,
                const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out, const uint64_t* h_out_off,
                uint16_t* h_raw, int num_gpus, const nsx_tune* tune) {
    if (n_frames == 0) return NSX_OK;
    if ((ip || tso) && !nsx::ip_hdr_ok(ip)) return NSX_EINVAL;
    if (!nsx::tcp_hdr_ok(h_hdr) || !h_data_off || !h_out || !h_out_off || (h_opt_off && !h_opts)) return NSX_EINVAL;
    if (tso && (n == 0 || n >= (1ull << 32) || !h_mss || !h_frame_first || !h_frame_seg)) return NSX_EINVAL;
    if (h_data_off[n] > h_data_off[0] && !h_data) return NSX_EINVAL;
    const uint32_t iph = !ip ? 0 : ipver == 4 ? 20 : 40;
    std::vector<uint64_t> seg_out;
    SenderJob j;
    if (tso) {
        if (nsx::tso_walk(h_opt_off, h_data_off, h_mss, n, h_frame_first, nullptr) != n_frames) return NSX_EINVAL;
        seg_out.resize(n + 1);
        if (!nsx::tso_layout_ok(iph, h_opt_off, h_data_off, h_mss, n, h_frame_seg, h_out_off, n_frames, seg_out.data(),
                                &j.gaps))
            return NSX_EINVAL;
    } else if (!nsx::sender_layout_ok(iph, h_opt_off, h_data_off, h_out_off, n, &j.gaps)) {
        return NSX_EINVAL;
    }
    j.tune = tune;
    j.ip = ip, j.ipver = ipver;
    j.fields = nsx::sender_fields(h_hdr, ip, ipver, tso ? h_mss : nullptr);
    j.opts = h_opts, j.opt_off = h_opt_off, j.data = h_data, j.data_off = h_data_off, j.partial = h_prefix_partial;
    j.out = h_out, j.out_off = h_out_off, j.raw = h_raw;
    j.tso = tso, j.frame_first = h_frame_first;
    j.seg_out = tso ? seg_out.data() : h_out_off;
    return run_shards(j, j.seg_out, n, j.seg_out[n] - j.seg_out[0], false, num_gpus);  // balanced by image bytes
}

// The ragged checksum (h_out) and the receive pass (h_mask): the same checks, then the job.
int ragged_host(Cut mode, int ipver, const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,
                const uint32_t* h_partial, uint16_t* h_out, uint64_t* h_mask, int num_gpus, const nsx_tune* tune) {
    const bool rx = mode == Cut::kRx;
    if (n == 0) return NSX_OK;
    if (!(rx ? (void*)h_mask : (void*)h_out) || !h_offsets || !h_base) return NSX_EINVAL;
    const nsx::LaunchCfg cfg = nsx::launch_cfg(1, tune);
    if (!(rx ? nsx::rx_tune_valid(cfg) : nsx::ragged_tune_valid(cfg))) return NSX_EINVAL;
    for (uint64_t i = 0; i < n; ++i)
        if (h_offsets[i + 1] < h_offsets[i]) return NSX_EINVAL;
    return csum_host(mode, ipver, h_base, 0, 0, h_offsets, n, h_partial, h_out, h_mask, num_gpus, tune);
}

}  // namespace

extern "C" {

int nsx_csum_fixed_host(const uint8_t* h_base, uint64_t stride, uint32_t seg_len, uint64_t n,
                        const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus) {
    return nsx_csum_fixed_host_tuned(h_base, stride, seg_len, n, h_prefix_partial, h_out, num_gpus, nullptr);
}

int nsx_csum_fixed_host_tuned(const uint8_t* h_base, uint64_t stride, uint32_t seg_len, uint64_t n,
                              const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus,
                              const nsx_tune* tune) {
    if (n == 0) return NSX_OK;
    if (!h_out || (seg_len && !h_base)) return NSX_EINVAL;
    return csum_host(Cut::kFixed, 0, h_base, stride, seg_len, nullptr, n, h_prefix_partial, h_out, nullptr, num_gpus,
                     tune);
}

int nsx_csum_ragged_host(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,
                         const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus) {
    return nsx_csum_ragged_host_tuned(h_base, h_offsets, n, h_prefix_partial, h_out, num_gpus, nullptr);
}

int nsx_csum_ragged_host_tuned(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,
                               const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus,
                               const nsx_tune* tune) {
    return ragged_host(Cut::kRagged, 0, h_base, h_offsets, n, h_prefix_partial, h_out, nullptr, num_gpus, tune);
}

int nsx_tcp_build_host(const nsx_tcp_hdr_soa* h_hdr, const uint8_t* h_opts, const uint64_t* h_opt_off,
                       const uint8_t* h_data, const uint64_t* h_data_off, const uint32_t* h_prefix_partial, uint64_t n,
                       uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_raw, int num_gpus) {
    return nsx_tcp_build_host_tuned(h_hdr, h_opts, h_opt_off, h_data, h_data_off, h_prefix_partial, n, h_out,
                                    h_out_off, h_raw, num_gpus, nullptr);
}

int nsx_tcp_build_host_tuned(const nsx_tcp_hdr_soa* h_hdr, const uint8_t* h_opts, const uint64_t* h_opt_off,
                             const uint8_t* h_data, const uint64_t* h_data_off, const uint32_t* h_prefix_partial,
                             uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_raw, int num_gpus,
                             const nsx_tune* tune) {
    return sender_host(false, nullptr, 0, h_hdr, h_opts, h_opt_off, h_data, h_data_off, h_prefix_partial, nullptr, n,
                       nullptr, nullptr, n, h_out, h_out_off, h_raw, num_gpus, tune);
}

// The receive pass, the transmit pass and segmentation offload from host memory, IPv4 and IPv6, each with its
// _tuned twin.
#define NSX_HOST_V(V)                                                                                               \
    int nsx_rx_ipv##V##_tcp_verify_host_tuned(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,         \
                                              uint64_t* h_mask, int num_gpus, const nsx_tune* tune) {               \
        return ragged_host(Cut::kRx, V, h_base, h_offsets, n, nullptr, nullptr, h_mask, num_gpus, tune);            \
    }                                                                                                               \
    int nsx_rx_ipv##V##_tcp_verify_host(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,               \
                                        uint64_t* h_mask, int num_gpus) {                                           \
        return ragged_host(Cut::kRx, V, h_base, h_offsets, n, nullptr, nullptr, h_mask, num_gpus, nullptr);         \
    }                                                                                                               \
    int nsx_tx_ipv##V##_tcp_build_host_tuned(                                                                       \
        const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts, const uint64_t* h_opt_off, \
        const uint8_t* h_data, const uint64_t* h_data_off, uint64_t n, uint8_t* h_out, const uint64_t* h_out_off,   \
        uint16_t* h_tcp_raw, int num_gpus, const nsx_tune* tune) {                                                  \
        if (n && !nsx::ip_hdr_ok(h_ip)) return NSX_EINVAL;                                                          \
        return sender_host(false, h_ip, V, h_tcp, h_opts, h_opt_off, h_data, h_data_off, nullptr, nullptr, n,       \
                           nullptr, nullptr, n, h_out, h_out_off, h_tcp_raw, num_gpus, tune);                       \
    }                                                                                                               \
    int nsx_tx_ipv##V##_tcp_build_host(                                                                             \
        const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts, const uint64_t* h_opt_off, \
        const uint8_t* h_data, const uint64_t* h_data_off, uint64_t n, uint8_t* h_out, const uint64_t* h_out_off,   \
        uint16_t* h_tcp_raw, int num_gpus) {                                                                        \
        return nsx_tx_ipv##V##_tcp_build_host_tuned(h_ip, h_tcp, h_opts, h_opt_off, h_data, h_data_off, n, h_out,   \
                                                    h_out_off, h_tcp_raw, num_gpus, nullptr);                       \
    }                                                                                                               \
    int nsx_tso_ipv##V##_tcp_build_host_tuned(                                                                      \
        const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts, const uint64_t* h_opt_off, \
        const uint8_t* h_data, const uint64_t* h_data_off, const uint32_t* h_mss, uint64_t n,                       \
        const uint64_t* h_frame_first, const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,              \
        const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus, const nsx_tune* tune) {                       \
        return sender_host(true, h_ip, V, h_tcp, h_opts, h_opt_off, h_data, h_data_off, nullptr, h_mss, n,          \
                           h_frame_first, h_frame_seg, n_frames, h_out, h_out_off, h_tcp_raw, num_gpus, tune);      \
    }                                                                                                               \
    int nsx_tso_ipv##V##_tcp_build_host(                                                                            \
        const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts, const uint64_t* h_opt_off, \
        const uint8_t* h_data, const uint64_t* h_data_off, const uint32_t* h_mss, uint64_t n,                       \
        const uint64_t* h_frame_first, const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,              \
        const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus) {                                             \
        return nsx_tso_ipv##V##_tcp_build_host_tuned(h_ip, h_tcp, h_opts, h_opt_off, h_data, h_data_off, h_mss, n,  \
                                                     h_frame_first, h_frame_seg, n_frames, h_out, h_out_off,        \
                                                     h_tcp_raw, num_gpus, nullptr);                                 \
    }
NSX_HOST_V(4)
NSX_HOST_V(6)
#undef NSX_HOST_V

int nsx_host_cache_release(void) {
    std::lock_guard<std::mutex> g(g_ctx_mu);
    int dev0 = 0;
    const bool restore = hipGetDevice(&dev0) == hipSuccess;
    for (int d = 0; d < kMaxDevices; ++d) {
        for (int s = 0; s < kMaxSlots; ++s) {
            if (!g_ctx[d][s]) continue;
            std::lock_guard<std::mutex> hold(g_ctx[d][s]->mu);
            if (hipSetDevice(d) != hipSuccess) {
                (void)hipGetLastError();
                continue;
            }
            g_ctx[d][s]->release();  // streams stay: they are cheap and reused
        }
    }
    if (restore) (void)hipSetDevice(dev0);
    return NSX_OK;
}

}  // extern "C"
