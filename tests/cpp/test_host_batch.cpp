// test_host_batch.cpp — the host batch driver (network-stack_amd/csrc/host_batch.cpp: shards, chunk pipeline,
// staging buffers, error paths) run on a CPU model of the HIP runtime (fake_hip.cpp) with CPU stand-ins for the
// kernels (cpu_launchers.cpp), built by tests/test_host_batch_cpp.py under AddressSanitizer + UBSan and under
// ThreadSanitizer with NSX_HOST_EXACT_BUFFERS, so that a staging buffer reserved a byte short, a host buffer reused
// before its stream was synchronised, work on the wrong device, a leak on an error path or a race between shard
// threads is a report, a recorded violation or a byte mismatch.
//
// Expected bytes: the same stand-in called once, synchronously, over the caller's whole arrays; the driver's output
// buffer must equal it byte for byte, the bytes a call must preserve included. argv[1] is tests/golden. Prints OK.
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_tune.h"
#include "cpu_launchers.h"
#include "fake_hip.h"

static std::string g_where;

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            std::printf("FAIL %s:%d: %s\n  in: %s\n", __FILE__, __LINE__, #cond, g_where.c_str()); \
            std::fflush(stdout);                                                                   \
            std::_Exit(1);                                                                         \
        }                                                                                          \
    } while (0)

static void where(const char* fmt, ...) {
    char s[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(s, sizeof s, fmt, ap);
    va_end(ap);
    g_where = s;
}

using U64 = std::vector<uint64_t>;
static std::mt19937_64 g_rng(0x1071);

static void fill_random(void* p, uint64_t n) {
    for (uint64_t i = 0; i < n; i += 8) {
        const uint64_t r = g_rng();
        std::memcpy(static_cast<uint8_t*>(p) + i, &r, std::min<uint64_t>(8, n - i));
    }
}
template <class T>
static std::vector<T> random_vec(uint64_t n) {
    std::vector<T> v(n);
    fill_random(v.data(), n * sizeof(T));
    return v;
}
static void fill_pattern(uint8_t* p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) p[i] = (uint8_t)(0xC3 ^ (i * 7));
}

// the sizes the GPU tests of the small-chunk paths use
static uint64_t pick_len() {
    static const uint64_t kLens[] = {0, 1, 63, 64, 1500, 1500, 1500, 9000, 64, 1};
    return kLens[g_rng() % 10];
}
static U64 pick_lens(uint64_t n) {
    U64 v(n);
    for (auto& x : v) x = pick_len();
    return v;
}
static U64 prefix(const U64& lens, uint64_t lead) {
    U64 off(lens.size() + 1, lead);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    return off;
}

// A caller's array: pinned (through the model's hipHostMalloc) or pageable, of exactly the bytes asked plus `mis`
// in front, so that the array starts `mis` bytes into its block and ends where the block ends.
class Bytes {
   public:
    Bytes(uint64_t n, bool pinned, uint64_t mis) : pinned_(pinned) {
        const uint64_t total = std::max<uint64_t>(n + mis, 1);
        if (pinned)
            CHECK(hipHostMalloc(&raw_, total, 0u) == hipSuccess);
        else
            raw_ = std::malloc(total);
        CHECK(raw_);
        p = static_cast<uint8_t*>(raw_) + mis;
    }
    Bytes(const Bytes&) = delete;
    Bytes& operator=(const Bytes&) = delete;
    ~Bytes() {
        if (pinned_)
            (void)hipHostFree(raw_);
        else
            std::free(raw_);
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }
    uint8_t* p = nullptr;

   private:
    void* raw_ = nullptr;
    bool pinned_;
};

static void same(const void* got, const void* want, uint64_t bytes, const char* what) {
    if (bytes == 0 || std::memcmp(got, want, bytes) == 0) return;
    const uint8_t *g = (const uint8_t*)got, *w = (const uint8_t*)want;
    uint64_t i = 0;
    while (g[i] == w[i]) ++i;
    std::printf("FAIL %s differ at byte %llu of %llu: got %02x, want %02x\n  in: %s\n", what, (unsigned long long)i,
                (unsigned long long)bytes, g[i], w[i], g_where.c_str());
    std::fflush(stdout);
    std::_Exit(1);
}

// ------------------------------------------------------------------ one call's dimensions
constexpr int kDevices = 3, kCallerDev = 1;

struct Cfg {
    fake::Mode mode = fake::Mode::kThreaded;
    int32_t budget = 0;  // nsx_tune.chunk_bytes
    bool in_pin = false, out_pin = false;
    int mis = 0;  // the caller's byte arrays start this far into their blocks
    int spd = 1, gpus = 1;
    std::string str() const {
        std::ostringstream s;
        s << (mode == fake::Mode::kThreaded ? "threaded" : "deferred") << " budget=" << budget << " in_pin=" << in_pin
          << " out_pin=" << out_pin << " mis=" << mis << " spd=" << spd << " gpus=" << gpus;
        return s.str();
    }
    nsx_tune tune() const {
        nsx_tune t{};
        t.chunk_bytes = budget, t.shards_per_device = spd;
        return t;
    }
};

static void begin_call(const Cfg& c) {
    fake::set_mode(c.mode);
    CHECK(hipSetDevice(kCallerDev) == hipSuccess);  // the caller is not on device 0: the call must put it back
    fake::reset_counters();
}

// What holds after every host call, failed ones included.
static void end_call(const Cfg& c, int rc, int want) {
    const std::vector<std::string> v = fake::take_violations();
    for (const std::string& s : v) std::printf("violation: %s\n", s.c_str());
    CHECK(v.empty());
    CHECK(fake::pending() == 0);  // every stream idle on return
    int dev = -1;
    CHECK(hipGetDevice(&dev) == hipSuccess && dev == kCallerDev);
    if (rc != want) std::printf("returned %d (%s), expected %d\n", rc, nsx_strerror(rc), want);
    CHECK(rc == want);
    CHECK(hipGetLastError() == hipSuccess);  // map_err leaves no error behind
    for (int d = std::max(c.gpus, 1); c.gpus > 0 && d < kDevices; ++d) CHECK(fake::ops_on_device(d) == 0);
}

// How a case's call is driven: plainly, or through a fault sweep. `prepare` pre-fills the outputs, `call` makes the
// host call, `verify` compares the outputs with the expected bytes.
using Fn0 = std::function<void()>;
using Call = std::function<int()>;
using Exec = std::function<void(const Cfg&, const Fn0& prepare, const Call& call, const Fn0& verify)>;

static void exec_plain(const Cfg& c, const Fn0& prepare, const Call& call, const Fn0& verify) {
    prepare();
    begin_call(c);
    const int rc = call();
    end_call(c, rc, NSX_OK);
    verify();
}
static Exec g_exec = exec_plain;
static uint64_t g_calls_made = 0, g_faults_fired = 0;

// Every k-th call of f in turn fails with e: the host call returns `want`, leaves the streams idle, the device
// restored and no violation, and the same call repeated without the fault gives the right bytes.
static Exec exec_fault(fake::Fn f, hipError_t e, int want, bool last_is_ignored) {
    return [=](const Cfg& c, const Fn0& prepare, const Call& call, const Fn0& verify) {
        (void)nsx_host_cache_release();  // so that the call allocates
        exec_plain(c, prepare, call, verify);
        uint64_t total = fake::calls(f);
        if (last_is_ignored) --total;  // run_shards' own restoring hipSetDevice, whose result nobody reads
        CHECK(total > 0);
        for (uint64_t k = 1; k <= total; ++k) {
            const std::string keep = g_where;
            where("%s | fault at call %llu of %llu", keep.c_str(), (unsigned long long)k, (unsigned long long)total);
            (void)nsx_host_cache_release();
            prepare();
            begin_call(c);
            fake::fail_nth(f, k, e);
            const int rc = call();
            CHECK(fake::fault_fired());
            fake::disarm();
            end_call(c, rc, want);
            exec_plain(c, prepare, call, verify);
            ++g_faults_fired;
            g_where = keep;
        }
    };
}

// ------------------------------------------------------------------ the checksum job
static void run_fixed(const Cfg& c, uint64_t stride, uint32_t seg_len, uint64_t n, bool with_partial) {
    where("fixed stride=%llu seg_len=%u n=%llu partial=%d | %s", (unsigned long long)stride, seg_len,
          (unsigned long long)n, with_partial, c.str().c_str());
    const uint64_t span = (n - 1) * stride + seg_len;
    Bytes base(span, c.in_pin, c.mis);
    fill_random(base.p, span);
    const std::vector<uint32_t> part = random_vec<uint32_t>(n);
    const uint32_t* partial = with_partial ? part.data() : nullptr;
    const uint64_t out_bytes = (n + 2) * 2;  // two entries behind the batch that the call must not touch
    Bytes out(out_bytes, c.out_pin, 2 * (c.mis & 1));
    std::vector<uint8_t> want(out_bytes);
    fill_pattern(want.data(), out_bytes);
    ref::fixed(nullptr, base.p, stride, seg_len, n, partial, reinterpret_cast<uint16_t*>(want.data()));
    const nsx_tune t = c.tune();
    g_exec(
        c, [&] { fill_pattern(out.p, out_bytes); },
        [&] { return nsx_csum_fixed_host_tuned(base.p, stride, seg_len, n, partial, out.as<uint16_t>(), c.gpus, &t); },
        [&] { same(out.p, want.data(), out_bytes, "fixed raw sums"); });
    ++g_calls_made;
}

static void run_ragged(const Cfg& c, const U64& lens, bool with_partial) {
    const uint64_t n = lens.size();
    where("ragged n=%llu partial=%d | %s", (unsigned long long)n, with_partial, c.str().c_str());
    const U64 off = prefix(lens, 3);
    Bytes base(off[n], c.in_pin, c.mis);
    fill_random(base.p, off[n]);
    const std::vector<uint32_t> part = random_vec<uint32_t>(n);
    const uint32_t* partial = with_partial ? part.data() : nullptr;
    const uint64_t out_bytes = (n + 2) * 2;
    Bytes out(out_bytes, c.out_pin, 2 * (c.mis & 1));
    std::vector<uint8_t> want(out_bytes);
    fill_pattern(want.data(), out_bytes);
    ref::ragged(nullptr, base.p, off.data(), n, partial, reinterpret_cast<uint16_t*>(want.data()), nullptr);
    const nsx_tune t = c.tune();
    g_exec(
        c, [&] { fill_pattern(out.p, out_bytes); },
        [&] { return nsx_csum_ragged_host_tuned(base.p, off.data(), n, partial, out.as<uint16_t>(), c.gpus, &t); },
        [&] { same(out.p, want.data(), out_bytes, "ragged raw sums"); });
    ++g_calls_made;
}

// ------------------------------------------------------------------ sender batches
struct TxBatch {
    int ipver;  // 0: TCP images
    uint64_t n;
    std::vector<uint16_t> sport, dport, window, urgent, ident;
    std::vector<uint32_t> seq, ack, flow, part;
    std::vector<uint8_t> offset, ctl, ttl, tclass, src, dst, opts, data;
    U64 opt_off, data_off;
    bool with_opts, null_optional;

    // lens: payload bytes per entry; null_optional: the arrays the ABI lets a caller leave out are left out
    TxBatch(int ipver_, const U64& lens, bool with_opts_, bool null_optional_)
        : ipver(ipver_), n(lens.size()), with_opts(with_opts_), null_optional(null_optional_) {
        sport = random_vec<uint16_t>(n), dport = random_vec<uint16_t>(n), window = random_vec<uint16_t>(n);
        urgent = random_vec<uint16_t>(n), ident = random_vec<uint16_t>(n);
        seq = random_vec<uint32_t>(n), ack = random_vec<uint32_t>(n), flow = random_vec<uint32_t>(n);
        part = random_vec<uint32_t>(n);
        offset = random_vec<uint8_t>(n), ctl = random_vec<uint8_t>(n), ttl = random_vec<uint8_t>(n);
        tclass = random_vec<uint8_t>(n);
        src = random_vec<uint8_t>(n * 16), dst = random_vec<uint8_t>(n * 16);
        static const uint64_t kOpt[] = {0, 1, 2, 3, 4, 10, 12, 40};  // every `remainder` of the reference's padding
        U64 olens(n);
        for (auto& x : olens) x = kOpt[g_rng() % 8];
        opt_off = prefix(olens, 1);  // the option bytes start at an odd address
        opts = random_vec<uint8_t>(opt_off[n] + 1);
        data_off = prefix(lens, 5);  // and the payloads off any alignment
        data = random_vec<uint8_t>(data_off[n]);
    }
    nsx_tcp_hdr_soa tcp() const {
        return {sport.data(), dport.data(), seq.data(),    ack.data(), null_optional ? nullptr : offset.data(),
                ctl.data(),   window.data(), urgent.data()};
    }
    nsx_ip_hdr_soa ip() const {
        if (null_optional) return {src.data(), dst.data(), nullptr, nullptr, nullptr, nullptr};
        return {src.data(), dst.data(), ident.data(), ttl.data(), tclass.data(), flow.data()};
    }
    const uint64_t* oo() const { return with_opts ? opt_off.data() : nullptr; }
    const uint8_t* ob() const { return with_opts ? opts.data() : nullptr; }
};

static nsx::TcpHdrSoA soa(const nsx_tcp_hdr_soa& h) {
    return {h.src_port, h.dst_port, h.seq_num, h.ack_num, h.offset, h.control, h.window, h.urgent_ptr};
}
static nsx::IpHdrSoA soa(const nsx_ip_hdr_soa& a) { return {a.src, a.dst, a.ident, a.ttl, a.tclass, a.flow}; }

// Slots longer than their padded image here and there: the bytes behind such an image are the caller's.
static void add_gaps(U64& out_off) {
    uint64_t extra = 0;
    for (size_t i = 1; i < out_off.size(); ++i) {
        extra += 4 * (i == 1 ? 1 : g_rng() % 3);
        out_off[i] += extra;
    }
}

// nsx_tcp_build_host (ipver 0) and nsx_tx_ipv4/6_tcp_build_host.
static void run_build(const Cfg& c, int ipver, const U64& lens, bool with_opts, bool with_partial, bool with_raw,
                      bool gaps, bool null_optional) {
    const uint64_t n = lens.size();
    where("build ipver=%d n=%llu opts=%d partial=%d raw=%d gaps=%d nulls=%d | %s", ipver, (unsigned long long)n,
          with_opts, with_partial, with_raw, gaps, null_optional, c.str().c_str());
    const TxBatch b(ipver, lens, with_opts, null_optional);
    Bytes data(b.data.size(), c.in_pin, c.mis);
    std::memcpy(data.p, b.data.data(), b.data.size());
    U64 out_off(n + 1);
    CHECK((ipver ? nsx_tx_layout_host(b.oo(), b.data_off.data(), n, ipver == 4 ? 20 : 40, out_off.data())
                 : nsx_tcp_layout_host(b.oo(), b.data_off.data(), n, out_off.data())) == NSX_OK);
    for (uint64_t i = 0; i < n; ++i)  // the stand-in's image length is the product's
        CHECK(out_off[i + 1] - out_off[i] ==
              (((ipver == 4 ? 20 : ipver == 6 ? 40 : 0) +
                nsx_tcp_wire_len(with_opts ? b.opt_off[i + 1] - b.opt_off[i] : 0, lens[i]) + 3) & ~3ull));
    if (gaps) add_gaps(out_off);
    const uint64_t out_bytes = out_off[n] + 5, raw_bytes = (n + 2) * 2;
    Bytes out(out_bytes, c.out_pin, c.mis), raw(raw_bytes, c.out_pin, 2 * (c.mis & 1));
    const nsx_tcp_hdr_soa tcp = b.tcp();
    const nsx_ip_hdr_soa ip = b.ip();
    const nsx::IpHdrSoA ips = soa(ip);
    const uint32_t* partial = with_partial && !ipver ? b.part.data() : nullptr;
    std::vector<uint8_t> want(out_bytes), want_raw(raw_bytes);
    fill_pattern(want.data(), out_bytes), fill_pattern(want_raw.data(), raw_bytes);
    ref::tcp_build(nullptr, ipver, ipver ? &ips : nullptr, soa(tcp), b.ob(), b.oo(), data.p, b.data_off.data(),
                   b.data_off[n], partial, n, want.data(), out_off.data(),
                   reinterpret_cast<uint16_t*>(want_raw.data()));
    uint16_t* rawp = with_raw ? raw.as<uint16_t>() : nullptr;
    const nsx_tune t = c.tune();
    g_exec(
        c, [&] { fill_pattern(out.p, out_bytes), fill_pattern(raw.p, raw_bytes); },
        [&] {
            if (ipver == 4)
                return nsx_tx_ipv4_tcp_build_host_tuned(&ip, &tcp, b.ob(), b.oo(), data.p, b.data_off.data(), n, out.p,
                                                        out_off.data(), rawp, c.gpus, &t);
            if (ipver == 6)
                return nsx_tx_ipv6_tcp_build_host_tuned(&ip, &tcp, b.ob(), b.oo(), data.p, b.data_off.data(), n, out.p,
                                                        out_off.data(), rawp, c.gpus, &t);
            return nsx_tcp_build_host_tuned(&tcp, b.ob(), b.oo(), data.p, b.data_off.data(), partial, n, out.p,
                                            out_off.data(), rawp, c.gpus, &t);
        },
        [&] {
            same(out.p, want.data(), out_bytes, "images");
            if (with_raw) same(raw.p, want_raw.data(), raw_bytes, "build raw sums");
        });
    ++g_calls_made;
}

// nsx_tso_ipv4/6_tcp_build_host over super-segments of `lens` payload bytes.
static void run_tso(const Cfg& c, int ipver, const U64& lens, bool with_opts, bool with_raw, bool gaps,
                    bool null_optional) {
    const uint64_t n = lens.size();
    where("tso ipver=%d n=%llu opts=%d raw=%d gaps=%d nulls=%d | %s", ipver, (unsigned long long)n, with_opts, with_raw,
          gaps, null_optional, c.str().c_str());
    const TxBatch b(ipver, lens, with_opts, null_optional);
    static const uint32_t kMss[] = {536, 1460, 9000, 100};
    std::vector<uint32_t> mss(n);
    for (auto& m : mss) m = kMss[g_rng() % 4];
    Bytes data(b.data.size(), c.in_pin, c.mis);
    std::memcpy(data.p, b.data.data(), b.data.size());
    U64 first(n + 1);
    CHECK(nsx_tso_count_host(b.data_off.data(), mss.data(), n, first.data()) == NSX_OK);
    const uint64_t nf = first[n];
    std::vector<uint32_t> seg(nf);
    U64 out_off(nf + 1);
    CHECK(nsx_tso_layout_host(b.oo(), b.data_off.data(), mss.data(), first.data(), n, ipver == 4 ? 20 : 40, seg.data(),
                              out_off.data()) == NSX_OK);
    if (gaps) add_gaps(out_off);
    const uint64_t out_bytes = out_off[nf] + 5, raw_bytes = (nf + 2) * 2;
    Bytes out(out_bytes, c.out_pin, c.mis), raw(raw_bytes, c.out_pin, 2 * (c.mis & 1));
    const nsx_tcp_hdr_soa tcp = b.tcp();
    const nsx_ip_hdr_soa ip = b.ip();
    std::vector<uint8_t> want(out_bytes), want_raw(raw_bytes);
    fill_pattern(want.data(), out_bytes), fill_pattern(want_raw.data(), raw_bytes);
    ref::tso_build(nullptr, ipver, soa(ip), nsx::TsoMap{mss.data(), first.data(), seg.data()}, soa(tcp), b.ob(), b.oo(),
                   data.p, b.data_off.data(), b.data_off[n], nf, want.data(), out_off.data(),
                   reinterpret_cast<uint16_t*>(want_raw.data()));
    uint16_t* rawp = with_raw ? raw.as<uint16_t>() : nullptr;
    const nsx_tune t = c.tune();
    g_exec(
        c, [&] { fill_pattern(out.p, out_bytes), fill_pattern(raw.p, raw_bytes); },
        [&] {
            return (ipver == 4 ? nsx_tso_ipv4_tcp_build_host_tuned : nsx_tso_ipv6_tcp_build_host_tuned)(
                &ip, &tcp, b.ob(), b.oo(), data.p, b.data_off.data(), mss.data(), n, first.data(), seg.data(), nf,
                out.p, out_off.data(), rawp, c.gpus, &t);
        },
        [&] {
            same(out.p, want.data(), out_bytes, "segmented frames");
            if (with_raw) same(raw.p, want_raw.data(), raw_bytes, "segmentation raw sums");
        });
    ++g_calls_made;
}

// ------------------------------------------------------------------ the receive pass
// n received frames packed back to back behind 3 bytes: datagrams the transmit stand-in built, most left whole,
// the others broken (a flipped bit, a byte cut off, a runt, nothing at all).
struct RxBatch {
    std::vector<uint8_t> buf;
    U64 off;
    uint64_t whole = 0;
};

static RxBatch make_rx(int ipver, uint64_t n) {
    static const uint64_t kPay[] = {0, 1, 63, 64, 200, 1500, 7, 20};
    U64 lens(n);
    for (auto& x : lens) x = kPay[g_rng() % 8];
    const TxBatch b(ipver, lens, true, false);
    U64 slot(n + 1);
    CHECK(nsx_tx_layout_host(b.oo(), b.data_off.data(), n, ipver == 4 ? 20 : 40, slot.data()) == NSX_OK);
    std::vector<uint8_t> built(slot[n]);
    const nsx_ip_hdr_soa ip = b.ip();
    const nsx::IpHdrSoA ips = soa(ip);
    ref::tcp_build(nullptr, ipver, &ips, soa(b.tcp()), b.ob(), b.oo(), b.data.data(), b.data_off.data(), b.data_off[n],
                   nullptr, n, built.data(), slot.data(), nullptr);
    RxBatch r;
    r.off.assign(1, 3);
    r.buf = random_vec<uint8_t>(3);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t len = (ipver == 4 ? 20 : 40) + nsx_tcp_wire_len(b.opt_off[i + 1] - b.opt_off[i], lens[i]);
        std::vector<uint8_t> f(built.begin() + slot[i], built.begin() + slot[i] + len);
        switch (g_rng() % 8) {
            // IPv6 bytes 1-3 and 7 (class, flow, hop limit) are under no checksum: a flip there breaks nothing
            case 0: f[ipver == 6 ? 8 + g_rng() % (len - 8) : g_rng() % len] ^= (uint8_t)(1u << (g_rng() % 8)); break;
            case 1: f.pop_back(); break;
            case 2: f.resize(g_rng() % 2 ? 0 : 7); break;
            default: ++r.whole;
        }
        r.buf.insert(r.buf.end(), f.begin(), f.end());
        r.off.push_back(r.buf.size());
    }
    return r;
}

static void run_rx(const Cfg& c, int ipver, const RxBatch& b) {
    const uint64_t n = b.off.size() - 1, words = (n + 63) / 64;
    where("rx ipv%d n=%llu | %s", ipver, (unsigned long long)n, c.str().c_str());
    Bytes base(b.buf.size(), c.in_pin, c.mis);
    std::memcpy(base.p, b.buf.data(), b.buf.size());
    const uint64_t mask_bytes = (words + 1) * 8;  // one word behind the mask that is not the call's
    Bytes mask(mask_bytes, c.out_pin, 8 * (c.mis & 1));
    std::vector<uint8_t> want(mask_bytes);
    fill_pattern(want.data(), mask_bytes);
    ref::rx_tcp(nullptr, ipver, base.p, b.off.data(), n, reinterpret_cast<uint64_t*>(want.data()));
    uint64_t bits = 0;
    for (uint64_t w = 0; w < words; ++w) bits += __builtin_popcountll(reinterpret_cast<uint64_t*>(want.data())[w]);
    CHECK(bits == b.whole);  // every frame the transmit stand-in built verifies, and no broken one does
    const nsx_tune t = c.tune();
    g_exec(
        c, [&] { fill_pattern(mask.p, mask_bytes); },
        [&] {
            return (ipver == 4 ? nsx_rx_ipv4_tcp_verify_host_tuned : nsx_rx_ipv6_tcp_verify_host_tuned)(
                base.p, b.off.data(), n, mask.as<uint64_t>(), c.gpus, &t);
        },
        [&] { same(mask.p, want.data(), mask_bytes, "validity mask"); });
    ++g_calls_made;
}

// ------------------------------------------------------------------ anchors: the stand-ins against product code
static std::vector<uint64_t> json_array(const std::string& text, const char* key) {
    const size_t at = text.find(std::string("\"") + key + "\": [");
    CHECK(at != std::string::npos);
    std::vector<uint64_t> v;
    const char* p = text.c_str() + text.find('[', at) + 1;
    while (*p && *p != ']') {
        char* end;
        v.push_back(std::strtoull(p, &end, 10));
        CHECK(end != p);
        p = end;
        while (*p == ',' || *p == ' ') ++p;
    }
    return v;
}

static std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) std::printf("cannot read %s\n", path.c_str());
    CHECK(bool(f));
    std::ostringstream s;
    s << f.rdbuf();
    return s.str();
}

static void test_anchors(const std::string& golden) {
    where("anchors");
    // raw sums against nsx_csum16, with and without a prefix
    for (uint64_t len : {0, 1, 2, 3, 63, 64, 1500, 9001}) {
        for (uint64_t plen : {0, 12, 40}) {
            const std::vector<uint8_t> seg = random_vec<uint8_t>(len + 1), pre = random_vec<uint8_t>(plen + 1);
            uint32_t partial = 0;
            for (uint64_t i = 0; i < plen; i += 2) partial += (uint32_t)pre[i] << 8 | pre[i + 1];
            uint16_t want = 0, got_fixed = 0, got_ragged = 0;
            CHECK(nsx_csum16(pre.data(), plen, seg.data(), len, &want) == NSX_OK);
            const uint64_t off[2] = {0, len};
            ref::fixed(nullptr, seg.data(), 0, (uint32_t)len, 1, plen ? &partial : nullptr, &got_fixed);
            ref::ragged(nullptr, seg.data(), off, 1, plen ? &partial : nullptr, &got_ragged, nullptr);
            CHECK(got_fixed == want && got_ragged == want);
        }
    }
    const std::vector<uint8_t> zeros(64, 0), ones(64, 0xFF);
    CHECK(ref::csum(0, zeros.data(), 64) == 0 && ref::csum(0, ones.data(), 64) == 0xFFFF);
    // the receive stand-in against the committed masks
    for (const char* name : {"rx", "rx6"}) {
        const std::string meta = slurp(golden + "/" + name + ".json"), blob = slurp(golden + "/" + name + ".bin");
        const U64 off = json_array(meta, "offsets"), want = json_array(meta, "mask");
        CHECK(off.size() > 64 && off.back() <= blob.size());
        const uint64_t n = off.size() - 1;
        CHECK(want.size() >= (n + 63) / 64);
        U64 got((n + 63) / 64, ~0ull);
        ref::rx_tcp(nullptr, name[2] ? 6 : 4, reinterpret_cast<const uint8_t*>(blob.data()), off.data(), n, got.data());
        for (size_t w = 0; w < got.size(); ++w) CHECK(got[w] == want[w]);
    }
    // an image is nsx_tcp_wire_len long, then zeros up to a multiple of 4, then nothing
    for (uint64_t olen = 0; olen <= 13; ++olen) {
        for (uint64_t dlen : {0, 1, 2, 7}) {
            const U64 lens{dlen};
            TxBatch b(0, lens, true, false);
            b.opt_off = {1, 1 + olen};
            b.opts = random_vec<uint8_t>(olen + 2);
            const uint64_t wire = nsx_tcp_wire_len(olen, dlen), out_off[2] = {0, 96};
            std::vector<uint8_t> out(96, 0xEE);
            uint16_t raw = 0;
            ref::tcp_build(nullptr, 0, nullptr, soa(b.tcp()), b.ob(), b.oo(), b.data.data(), b.data_off.data(),
                           b.data_off[1], nullptr, 1, out.data(), out_off, &raw);
            for (uint64_t k = wire; k < 96; ++k) CHECK(out[k] == (k < ((wire + 3) & ~3ull) ? 0 : 0xEE));
            if (dlen) CHECK(out[wire - 1] == b.data[b.data_off[1] - 1]);
            CHECK(ref::csum(0, out.data(), wire) == 0xFFFF);  // the stored field closes the sum (tcp.go:70)
            CHECK(raw == (uint16_t)~(out[16] << 8 | out[17]));
        }
    }
}

// ------------------------------------------------------------------ the cases
static const int32_t kBudgets[] = {1, 64, 4096, 0};
static const int kSpd[] = {1, 2, 3, 8};

// Both stream modes x the four chunk budgets x input and output pinned or pageable; shards per device, devices and
// the byte offset of the caller's arrays rotate through their values, from a different start for every `salt`.
static void for_dims(int salt, const std::function<void(const Cfg&)>& fn) {
    int i = salt;
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred})
        for (int32_t budget : kBudgets)
            for (int pin = 0; pin < 4; ++pin, ++i) {
                Cfg c;
                c.mode = mode, c.budget = budget, c.in_pin = pin & 1, c.out_pin = pin >> 1;
                c.spd = kSpd[i % 4], c.gpus = 1 + (i / 4 + i) % 3, c.mis = (i / 2 + salt) % 4;
                fn(c);
                (void)nsx_host_cache_release();  // each case's buffers are sized by that case alone
            }
}

static void test_all_entry_points() {
    int salt = 0;
    for (bool partial : {false, true}) {
        for_dims(salt++, [&](const Cfg& c) { run_fixed(c, 1503, 1500, 40, partial); });
        for_dims(salt++, [&](const Cfg& c) { run_fixed(c, 40, 64, 40, partial); });  // stride < seg_len: overlapping
        for_dims(salt++, [&](const Cfg& c) { run_fixed(c, 0, 1500, 40, partial); });  // every segment the first
        for_dims(salt++, [&](const Cfg& c) { run_fixed(c, 9, 0, 40, partial); });     // empty segments
        for_dims(salt++, [&](const Cfg& c) { run_ragged(c, pick_lens(40), partial); });
    }
    for (int ipver : {4, 6}) {
        std::vector<RxBatch> batches;
        for (uint64_t n : {1, 63, 64, 65, 128, 130, 257}) batches.push_back(make_rx(ipver, n));
        int k = 0;  // shard and chunk edges on and off 64-frame words; a pinned mask takes the shards' copies directly
        for_dims(salt++, [&](const Cfg& c) { run_rx(c, ipver, batches[k++ % 7]), run_rx(c, ipver, batches[k++ % 7]); });
    }
    for (int ipver : {0, 4, 6}) {
        for_dims(salt++, [&](const Cfg& c) { run_build(c, ipver, pick_lens(32), false, false, false, false, true); });
        for_dims(salt++, [&](const Cfg& c) { run_build(c, ipver, pick_lens(32), true, true, true, false, false); });
        for_dims(salt++, [&](const Cfg& c) { run_build(c, ipver, pick_lens(32), true, false, true, true, true); });
    }
    static const uint64_t kSuper[] = {0, 1, 1500, 9000, 20000, 64, 4000};
    const auto supers = [](uint64_t n) {
        U64 v(n);
        for (auto& x : v) x = kSuper[g_rng() % 7];
        return v;
    };
    for (int ipver : {4, 6}) {
        for_dims(salt++, [&](const Cfg& c) { run_tso(c, ipver, supers(9), false, true, false, true); });
        for_dims(salt++, [&](const Cfg& c) { run_tso(c, ipver, supers(9), true, true, true, false); });
        for_dims(salt++, [&](const Cfg& c) { run_tso(c, ipver, supers(9), true, false, false, false); });
    }
}

// One, two and three chunks exactly (one slot, two slots, the first slot used again), and more shards than segments.
static void test_chunk_counts() {
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred}) {
        for (uint64_t n : {1, 2, 3, 5}) {
            for (int pin = 0; pin < 4; ++pin) {
                Cfg c;
                c.mode = mode, c.budget = 1, c.in_pin = pin & 1, c.out_pin = pin >> 1, c.mis = pin;
                run_fixed(c, 1503, 1500, n, true);
                run_ragged(c, U64(n, 1500), true);
                run_build(c, 0, U64(n, 1500), true, true, true, pin & 1, false);
                run_build(c, 4, U64(n, 63), true, false, true, pin >> 1, false);
                run_tso(c, 6, U64(n, 4000), true, true, pin & 1, false);
                run_rx(c, 4, make_rx(4, 64 * n + 1));
                c.spd = 8, c.gpus = 3;  // 24 shards wanted
                run_fixed(c, 64, 64, n, false);
                run_ragged(c, U64(n, 63), false);
                run_tso(c, 4, U64(n, 1500), false, true, false, true);
                (void)nsx_host_cache_release();
            }
        }
    }
}

// Which devices a call uses: shard g on device g / shards_per_device, an auto call by the batch's bytes, and more
// devices than there are is NSX_ENODEV before anything is queued.
static void test_devices() {
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred}) {
        for (int spd : kSpd) {
            for (int gpus = 1; gpus <= kDevices; ++gpus) {
                Cfg c;
                c.mode = mode, c.budget = 4096, c.spd = spd, c.gpus = gpus;
                run_fixed(c, 1500, 1500, 96, true);  // sharded by count: every one of `gpus` devices has segments
                for (int d = 0; d < kDevices; ++d) CHECK((fake::ops_on_device(d) > 0) == (d < gpus));
                run_build(c, 4, U64(96, 64), false, false, true, false, false);
                for (int d = 0; d < kDevices; ++d) CHECK((fake::ops_on_device(d) > 0) == (d < gpus));
            }
        }
        Cfg c;
        c.mode = mode, c.gpus = 0;
        run_fixed(c, 0, 1500, 100000, false);  // 150 MB to the planner, 1.5 KB of memory: three 64 MiB shards
        for (int d = 0; d < kDevices; ++d) CHECK(fake::ops_on_device(d) > 0);
        run_fixed(c, 1500, 1500, 50, false);  // a small auto call stays on device 0
        CHECK(fake::ops_on_device(0) > 0 && fake::ops_on_device(1) == 0 && fake::ops_on_device(2) == 0);
        (void)nsx_host_cache_release();
    }
    where("num_gpus above the device count");
    std::vector<uint8_t> seg(64, 1);
    std::vector<uint16_t> out(4, 0xABCD);
    const U64 off{0, 16, 32, 48, 64};
    begin_call(Cfg{});
    CHECK(nsx_csum_fixed_host(seg.data(), 16, 16, 4, nullptr, out.data(), kDevices + 1) == NSX_ENODEV);
    CHECK(nsx_csum_ragged_host(seg.data(), off.data(), 4, nullptr, out.data(), kDevices + 1) == NSX_ENODEV);
    CHECK(fake::pending() == 0 && fake::take_violations().empty() && out[0] == 0xABCD);
    for (int d = 0; d < kDevices; ++d) CHECK(fake::ops_on_device(d) == 0);
    CHECK(fake::calls(fake::Fn::kMemcpyAsync) == 0 && fake::calls(fake::Fn::kMalloc) == 0);
    fake::set_device_count(1);  // and with one device, two
    CHECK(nsx_csum_fixed_host(seg.data(), 16, 16, 4, nullptr, out.data(), 2) == NSX_ENODEV);
    fake::set_device_count(kDevices);
}

// The buffers persist and only grow: small, large, small without a release in between.
static void test_buffer_reuse() {
    (void)nsx_host_cache_release();
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred}) {
        for (uint64_t n : {4, 90, 4, 31}) {
            Cfg c;
            c.mode = mode, c.budget = 4096, c.spd = 2;
            run_ragged(c, pick_lens(n), true);
            run_fixed(c, 100, 64, n, false);
            run_build(c, 6, pick_lens(n), true, false, true, true, false);
            run_tso(c, 4, U64(n / 4 + 1, 9000), true, true, false, false);
            run_rx(c, 6, make_rx(6, n * 3));
        }
    }
    (void)nsx_host_cache_release();
    CHECK(fake::live_blocks() == 0);
}

// NSX_HOST_COPY_THREADS=3: both directions of stage_copy split a 4 MiB + 4097 B span into uneven pieces.
static void test_threaded_copy() {
    const char* e = std::getenv("NSX_HOST_COPY_THREADS");
    where("NSX_HOST_COPY_THREADS must be 3 for this program");
    CHECK(e && std::atoi(e) == 3);
    const uint64_t big = (4ull << 20) + 4097;
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred}) {
        Cfg c;
        c.mode = mode, c.mis = 1;
        run_ragged(c, U64{big}, false);                                           // one segment, one input span
        run_build(c, 0, U64{big - 20}, false, true, true, false, false);          // one image of exactly `big` bytes
        run_build(c, 0, U64{7, big - 20, 64}, false, false, true, true, false);   // and among others, with gaps
        (void)nsx_host_cache_release();
    }
}

// Two application threads in host calls on the same device at once, and a third releasing the cache meanwhile.
static void test_concurrency() {
    for (fake::Mode mode : {fake::Mode::kThreaded, fake::Mode::kDeferred}) {
        fake::set_mode(mode);
        std::atomic<bool> stop{false};
        std::atomic<int> bad{0};
        const auto app = [&](int which) {
            std::mt19937_64 rng(which);
            if (hipSetDevice(kCallerDev) != hipSuccess) ++bad;
            for (int it = 0; it < 6; ++it) {
                const uint64_t n = 20 + rng() % 30, len = 1 + rng() % 1500;
                std::vector<uint8_t> base(n * len);
                for (uint64_t i = 0; i + 8 <= base.size(); i += 8) {
                    const uint64_t r = rng();
                    std::memcpy(base.data() + i, &r, 8);
                }
                std::vector<uint16_t> out(n), want(n);
                nsx_tune t{};
                t.chunk_bytes = 4096, t.shards_per_device = 1 + it % 2;
                ref::fixed(nullptr, base.data(), len, (uint32_t)len, n, nullptr, want.data());
                const int rc = nsx_csum_fixed_host_tuned(base.data(), len, (uint32_t)len, n, nullptr, out.data(),
                                                         1 + it % 2, &t);
                if (rc != NSX_OK || out != want) ++bad;
                int dev = -1;
                if (hipGetDevice(&dev) != hipSuccess || dev != kCallerDev) ++bad;
            }
        };
        std::thread a(app, 1), b(app, 2), r([&] {
            while (!stop.load()) {
                if (nsx_host_cache_release() != NSX_OK) ++bad;
                std::this_thread::yield();
            }
        });
        a.join(), b.join();
        stop.store(true);
        r.join();
        where("concurrent callers and cache release");
        CHECK(bad.load() == 0);
        const std::vector<std::string> v = fake::take_violations();
        for (const std::string& s : v) std::printf("violation: %s\n", s.c_str());
        CHECK(v.empty() && fake::pending() == 0);
    }
    (void)nsx_host_cache_release();
}

// A failing hipStreamCreateWithFlags. Streams are made once per device and shard slot and kept, so this runs before
// anything else has made one: the first stream of (device 0, slot 0); then, with that slot's streams in place, a
// stream of slots 1 / 2 in a 3-shard call; then the second stream of device 1 in a 2-device call.
static void test_stream_create_faults() {
    const auto once = [](const Cfg& c, uint64_t k, hipError_t e, int want) {
        g_exec = [=](const Cfg& cc, const Fn0& prepare, const Call& call, const Fn0& verify) {
            prepare();
            begin_call(cc);
            fake::fail_nth(fake::Fn::kStreamCreate, k, e);
            const int rc = call();
            CHECK(fake::fault_fired());
            fake::disarm();
            end_call(cc, rc, want);
            exec_plain(cc, prepare, call, verify);
            ++g_faults_fired;
        };
        run_ragged(c, U64(12, 1500), true);
        g_exec = exec_plain;
        (void)nsx_host_cache_release();
    };
    Cfg c;
    c.budget = 4096;
    c.mode = fake::Mode::kDeferred;
    once(c, 1, hipErrorOutOfMemory, NSX_ENOMEM);
    c.spd = 3;
    once(c, 2, hipErrorOutOfMemory, NSX_ENOMEM);
    c.spd = 1, c.gpus = 2, c.mode = fake::Mode::kThreaded;
    once(c, 2, hipErrorNoDevice, NSX_ENODEV);
}

// Every allocation of reserve() (device and pinned, slot 0 and slot 1), every copy of a multi-chunk pipeline and
// every shard's hipSetDevice fails in turn, in a single-shard call and in a 3-shard call where one shard is hit.
static void test_faults() {
    for (fake::Mode mode : {fake::Mode::kDeferred, fake::Mode::kThreaded}) {
        for (int spd : {1, 3}) {
            Cfg c;
            c.mode = mode, c.budget = 4096, c.spd = spd;
            const auto jobs = [&] {
                run_ragged(c, U64(4 * spd, 1500), true);                        // two chunks a shard, all staged
                run_tso(c, 4, U64(3 * spd, 4000), true, true, true, false);     // the sender job's reserve()
                c.in_pin = c.out_pin = true;
                run_build(c, 0, U64(4 * spd, 1500), true, true, true, false, false);
                c.in_pin = c.out_pin = false;
            };
            g_exec = exec_fault(fake::Fn::kMalloc, hipErrorOutOfMemory, NSX_ENOMEM, false);
            jobs();
            g_exec = exec_fault(fake::Fn::kHostMalloc, hipErrorOutOfMemory, NSX_ENOMEM, false);
            jobs();
            g_exec = exec_fault(fake::Fn::kMemcpyAsync, hipErrorUnknown, NSX_EIO, false);
            jobs();
            g_exec = exec_fault(fake::Fn::kSetDevice, hipErrorInvalidDevice, NSX_ENODEV, true);
            jobs();
            g_exec = exec_plain;
        }
    }
    (void)nsx_host_cache_release();
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    fake::set_device_count(kDevices);
    auto phase = [t0 =std::chrono::steady_clock::now()](const char* name, const Fn0& fn) mutable {
        fn();
        const auto t1 = std::chrono::steady_clock::now();
        std::printf("%-22s %6.2f s\n", name, std::chrono::duration<double>(t1 - t0).count());
        t0 = t1;
    };
    phase("anchors", [&] { test_anchors(argv[1]); });
    phase("stream create faults", test_stream_create_faults);
    phase("chunk counts", test_chunk_counts);
    phase("all entry points", test_all_entry_points);
    phase("devices", test_devices);
    phase("buffer reuse", test_buffer_reuse);
    phase("threaded copy", test_threaded_copy);
    phase("concurrency", test_concurrency);
    phase("faults", test_faults);
    (void)nsx_host_cache_release();
    where("the end");
    CHECK(fake::live_blocks() == 0);  // the cache is empty and every pinned array of the cases went back
    CHECK(hipSetDevice(0) == hipSuccess);
    fake::shutdown();
    std::printf("%llu host calls checked, %llu injected faults\nOK\n", (unsigned long long)g_calls_made,
                (unsigned long long)g_faults_fired);
    return 0;
}
