// cpu_launchers.cpp — CPU stand-ins for the launcher interface of network-stack_amd/csrc/csum_kernels.h, so that
// host_batch.cpp and csum_api.cpp link and run without a GPU (tests/cpp/test_host_batch.cpp).
//
// The five launchers the host batch driver calls queue, on the fake stream (fake_hip.h), a plain C++ restatement of
// the contract in include/nsx_csum.h — written from that header and from the numpy models tests/_tx.py, tests/_tso.py
// and tests/_rx.py. They are not the code under test; they are where a wrongly rebased chunk is caught: each asserts
// what the contract promises a kernel (non-decreasing offsets, data_off[n] <= data_bytes, 4-aligned image slots that
// hold their image, a frame map whose two arrays agree, whole mask words) and touches exactly the bytes the contract
// allows, so a buffer reserved a few bytes short is a sanitizer report. The rest of the interface exists only to
// link and reports hipErrorNotSupported.
#include "cpu_launchers.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fake_hip.h"

namespace {

using ull = unsigned long long;

[[noreturn]] void die(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stderr, "launcher contract broken: ");
    std::vfprintf(stderr, fmt, ap);
    std::fprintf(stderr, "\n");
    va_end(ap);
    std::fflush(nullptr);
    std::_Exit(3);
}

// [p, p + bytes) is device memory of st's device (no st: ordinary memory, the sanitizer's business).
void need(hipStream_t st, const void* p, uint64_t bytes, const char* what) {
    if (!st || bytes == 0) return;
    if (!p) die("%s: null with %llu bytes to touch", what, (ull)bytes);
    if (!fake::device_range(st, p, bytes, what)) die("%s leaves its device block (%llu bytes)", what, (ull)bytes);
}

void monotone(const uint64_t* off, uint64_t n, const char* what) {
    for (uint64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) die("%s decrease at %llu", what, (ull)i);
}

uint64_t add_words(uint64_t acc, const uint8_t* p, uint64_t len) {
    uint64_t i = 0;
    for (; i + 8 <= len; i += 8) {  // four big-endian words at a time
        uint64_t w;
        std::memcpy(&w, p + i, 8);
        w = __builtin_bswap64(w);
        acc += (w >> 48) + (w >> 32 & 0xFFFF) + (w >> 16 & 0xFFFF) + (w & 0xFFFF);
    }
    for (; i + 4 <= len; i += 4) {
        uint32_t w;
        std::memcpy(&w, p + i, 4);
        w = __builtin_bswap32(w);
        acc += (w >> 16) + (w & 0xFFFF);
    }
    for (; i + 2 <= len; i += 2) acc += (uint64_t)p[i] << 8 | p[i + 1];
    if (i < len) acc += (uint64_t)p[i] << 8;  // an odd total is zero-padded
    return acc;
}

uint16_t fold(uint64_t s) {
    while (s >> 16) s = (s & 0xFFFF) + (s >> 16);
    return (uint16_t)s;
}

void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 8), p[1] = (uint8_t)v; }
void put32(uint8_t* p, uint32_t v) { put16(p, v >> 16), put16(p + 2, v & 0xFFFF); }

// One frame of the sender / transmit pass.
struct Frame {
    int ipver;  // 0: the TCP image alone, over `partial`
    const uint8_t *src, *dst;
    uint16_t ident;
    uint8_t ttl, tclass;
    uint32_t flow;
    uint16_t sport, dport;
    uint32_t seq, ack;
    uint8_t byte12, ctl;
    uint16_t window, urgent;
    const uint8_t* opt;
    uint64_t olen;
    const uint8_t* pay;
    uint64_t dlen;
    uint32_t partial;
};

uint64_t wire_len(uint64_t olen, uint64_t dlen) { return 20 + olen + (olen ? (20 + olen) % 4 : 0) + dlen; }
uint32_t ip_len(int ipver) { return ipver == 4 ? 20 : ipver == 6 ? 40 : 0; }
bool fits_ip(int ipver, uint64_t wire) { return ipver == 4 ? wire <= 65515 : ipver == 6 ? wire <= 65535 : true; }

// Writes the frame and its zero padding at o (a 4-aligned slot of at least the padded length); the TCP raw sum.
uint16_t write_frame(const Frame& f, uint8_t* o) {
    const uint32_t iph = ip_len(f.ipver);
    const uint64_t wire = wire_len(f.olen, f.dlen), alen = f.ipver == 4 ? 4 : 16;
    uint64_t acc = f.partial;
    if (f.ipver == 4) {
        o[0] = 0x45, o[1] = 0;
        put16(o + 2, (uint32_t)(20 + wire));
        put16(o + 4, f.ident);
        o[6] = 0x40, o[7] = 0, o[8] = f.ttl, o[9] = 6;
        put16(o + 10, 0);
        std::memcpy(o + 12, f.src, 4);
        std::memcpy(o + 16, f.dst, 4);
        put16(o + 10, (uint16_t)~fold(add_words(0, o, 20)));
        acc = add_words(add_words(0, f.src, 4), f.dst, 4) + 6 + wire;
    } else if (f.ipver == 6) {
        put32(o, 6u << 28 | (uint32_t)f.tclass << 20 | (f.flow & 0xFFFFF));
        put16(o + 4, (uint32_t)wire);
        o[6] = 6, o[7] = f.ttl;
        std::memcpy(o + 8, f.src, 16);
        std::memcpy(o + 24, f.dst, 16);
        acc = add_words(add_words(0, f.src, alen), f.dst, alen) + (wire >> 16) + (wire & 0xFFFF) + 6;
    }
    uint8_t* t = o + iph;
    put16(t, f.sport), put16(t + 2, f.dport), put32(t + 4, f.seq), put32(t + 8, f.ack);
    t[12] = f.byte12, t[13] = f.ctl;
    put16(t + 14, f.window), put16(t + 16, 0), put16(t + 18, f.urgent);
    uint64_t at = 20;
    if (f.olen) {
        std::memcpy(t + at, f.opt, f.olen);
        at += f.olen;
        for (uint64_t k = (20 + f.olen) % 4; k; --k) t[at++] = 0;  // the reference's `remainder` padding
    }
    if (f.dlen) std::memcpy(t + at, f.pay, f.dlen);
    at += f.dlen;
    const uint16_t raw = fold(add_words(acc, t, wire));
    put16(t + 16, (uint16_t)~raw);
    for (uint64_t k = iph + wire; k & 3; ++k) o[k] = 0;  // up to 3 bytes after the frame
    return raw;
}

template <class T>
T at_or(const T* a, uint64_t i, T dflt) { return a ? a[i] : dflt; }

// A frame from entry `s` of the field arrays, with the options and the payload slice given.
Frame make_frame(int ipver, const nsx::IpHdrSoA* ip, const nsx::TcpHdrSoA& h, uint64_t s, const uint8_t* opt,
                 uint64_t olen, const uint8_t* pay, uint64_t dlen, uint32_t partial) {
    Frame f{};
    f.ipver = ipver;
    if (ipver) {
        const uint64_t alen = ipver == 4 ? 4 : 16;
        f.src = ip->src + s * alen, f.dst = ip->dst + s * alen;
        f.ident = at_or<uint16_t>(ip->ident, s, 0), f.ttl = at_or<uint8_t>(ip->ttl, s, 64);
        f.tclass = at_or<uint8_t>(ip->tclass, s, 0), f.flow = at_or<uint32_t>(ip->flow, s, 0);
    }
    f.sport = h.src_port[s], f.dport = h.dst_port[s], f.seq = h.seq[s], f.ack = h.ack[s];
    f.byte12 = h.offset ? h.offset[s] : (uint8_t)((20 + olen + 3) / 4);  // computeOffset
    f.ctl = h.ctl[s], f.window = h.window[s], f.urgent = h.urgent[s];
    f.opt = opt, f.olen = olen, f.pay = pay, f.dlen = dlen, f.partial = partial;
    return f;
}

void need_fields(hipStream_t st, int ipver, const nsx::IpHdrSoA* ip, const nsx::TcpHdrSoA& h, uint64_t n) {
    need(st, h.src_port, n * 2, "src_port"), need(st, h.dst_port, n * 2, "dst_port");
    need(st, h.seq, n * 4, "seq_num"), need(st, h.ack, n * 4, "ack_num");
    if (h.offset) need(st, h.offset, n, "offset");
    need(st, h.ctl, n, "control"), need(st, h.window, n * 2, "window"), need(st, h.urgent, n * 2, "urgent_ptr");
    if (!ipver) return;
    const uint64_t alen = ipver == 4 ? 4 : 16;
    need(st, ip->src, n * alen, "ip src"), need(st, ip->dst, n * alen, "ip dst");
    if (ip->ident) need(st, ip->ident, n * 2, "ident");
    if (ip->ttl) need(st, ip->ttl, n, "ttl");
    if (ip->tclass) need(st, ip->tclass, n, "tclass");
    if (ip->flow) need(st, ip->flow, n * 4, "flow");
}

// The slot [out_off[f], out_off[f + 1]) is 4-aligned and holds the padded frame.
void check_slot(const uint64_t* out_off, uint64_t f, uint64_t frame_len) {
    if (out_off[f] & 3) die("out_off[%llu] = %llu is not a multiple of 4", (ull)f, (ull)out_off[f]);
    if (out_off[f + 1] < out_off[f] || out_off[f + 1] - out_off[f] < ((frame_len + 3) & ~3ull))
        die("slot %llu [%llu, %llu) does not hold its %llu-byte image", (ull)f,
            (ull)out_off[f], (ull)out_off[f + 1], (ull)frame_len);
}

}  // namespace

namespace ref {

uint16_t csum(uint32_t partial, const uint8_t* p, uint64_t len) { return fold(add_words(partial, p, len)); }

void fixed(hipStream_t st, const uint8_t* base, uint64_t stride, uint32_t seg_len, uint64_t n, const uint32_t* partial,
           uint16_t* out) {
    if (n == 0) return;
    if (seg_len) need(st, base, (n - 1) * stride + seg_len, "fixed-stride segments");
    if (partial) need(st, partial, n * 4, "partials");
    need(st, out, n * 2, "raw sums");
    for (uint64_t i = 0; i < n; ++i)
        out[i] = csum(partial ? partial[i] : 0, seg_len ? base + i * stride : nullptr, seg_len);
}

void ragged(hipStream_t st, const uint8_t* base, const uint64_t* offsets, uint64_t n, const uint32_t* partial,
            uint16_t* out, uint8_t* ok) {
    if (n == 0) return;
    need(st, offsets, (n + 1) * 8, "ragged offsets");
    monotone(offsets, n, "ragged offsets");
    need(st, base + offsets[0], offsets[n] - offsets[0], "ragged segments");
    if (partial) need(st, partial, n * 4, "partials");
    if (out) need(st, out, n * 2, "raw sums");
    if (ok) need(st, ok, n, "verdicts");
    for (uint64_t i = 0; i < n; ++i) {
        const uint16_t raw = csum(partial ? partial[i] : 0, base + offsets[i], offsets[i + 1] - offsets[i]);
        if (out) out[i] = raw;
        if (ok) ok[i] = raw == 0xFFFF;
    }
}

static bool rx_valid4(const uint8_t* f, uint64_t len) {
    if (len < 20 || f[0] >> 4 != 4) return false;
    const uint64_t hl = (f[0] & 15) * 4u, total = (uint64_t)f[2] << 8 | f[3];
    if (hl < 20 || hl > len || total != len) return false;
    if ((f[6] & 0x3F) || f[7] || f[9] != 6 || len - hl < 20) return false;  // MF, fragment offset, protocol, TCP length
    if (fold(add_words(0, f, hl)) != 0xFFFF) return false;
    const uint64_t pseudo = add_words(0, f + 12, 8) + 6 + (len - hl);
    return fold(add_words(pseudo, f + hl, len - hl)) == 0xFFFF;
}

static bool rx_valid6(const uint8_t* f, uint64_t len) {
    if (len < 40 || f[0] >> 4 != 6) return false;
    const uint64_t pl = (uint64_t)f[4] << 8 | f[5];
    if (40 + pl != len || f[6] != 6 || pl < 20) return false;
    const uint64_t pseudo = add_words(0, f + 8, 32) + pl + 6;
    return fold(add_words(pseudo, f + 40, pl)) == 0xFFFF;
}

void rx_tcp(hipStream_t st, int ipver, const uint8_t* base, const uint64_t* offsets, uint64_t n, uint64_t* mask) {
    if (n == 0) return;
    if (ipver != 4 && ipver != 6) die("receive pass: ipver %d", ipver);
    need(st, offsets, (n + 1) * 8, "frame offsets");
    monotone(offsets, n, "frame offsets");
    need(st, base + offsets[0], offsets[n] - offsets[0], "frames");
    need(st, mask, (n + 63) / 64 * 8, "validity mask");  // whole words, and no more of them
    for (uint64_t w = 0; w < (n + 63) / 64; ++w) {
        uint64_t bits = 0;
        for (uint64_t i = w * 64; i < n && i < w * 64 + 64; ++i) {
            const uint8_t* f = base + offsets[i];
            const uint64_t len = offsets[i + 1] - offsets[i];
            if (ipver == 4 ? rx_valid4(f, len) : rx_valid6(f, len)) bits |= 1ull << (i % 64);
        }
        mask[w] = bits;  // bits past n are 0
    }
}

void tcp_build(hipStream_t st, int ipver, const nsx::IpHdrSoA* ip, const nsx::TcpHdrSoA& h, const uint8_t* opts,
               const uint64_t* opt_off, const uint8_t* data, const uint64_t* data_off, uint64_t data_bytes,
               const uint32_t* partial, uint64_t n, uint8_t* out, const uint64_t* out_off, uint16_t* raw) {
    if (n == 0) return;
    if (ipver != 0 && ipver != 4 && ipver != 6) die("build: ipver %d", ipver);
    if (ipver && !ip) die("build: datagrams without IP fields");
    need_fields(st, ipver, ip, h, n);
    need(st, data_off, (n + 1) * 8, "data_off"), need(st, out_off, (n + 1) * 8, "out_off");
    if (opt_off) need(st, opt_off, (n + 1) * 8, "opt_off");
    monotone(data_off, n, "data_off"), monotone(out_off, n, "out_off");
    if (opt_off) monotone(opt_off, n, "opt_off");
    if (data_off[n] > data_bytes) die("data_off[n] = %llu > data_bytes = %llu", (ull)data_off[n], (ull)data_bytes);
    need(st, data, data_bytes, "payload buffer");
    if (opt_off) need(st, opts + opt_off[0], opt_off[n] - opt_off[0], "options");
    if (partial) need(st, partial, n * 4, "partials");
    if (raw) need(st, raw, n * 2, "raw sums");
    need(st, out + out_off[0], out_off[n] - out_off[0], "image slots");
    const uint32_t iph = ip_len(ipver);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t olen = opt_off ? opt_off[i + 1] - opt_off[i] : 0, dlen = data_off[i + 1] - data_off[i];
        if (!fits_ip(ipver, wire_len(olen, dlen))) {  // not built: nothing written, raw 0
            if (raw) raw[i] = 0;
            continue;
        }
        check_slot(out_off, i, iph + wire_len(olen, dlen));
        const Frame f = make_frame(ipver, ip, h, i, olen ? opts + opt_off[i] : nullptr, olen,
                                   dlen ? data + data_off[i] : nullptr, dlen, !ipver && partial ? partial[i] : 0);
        const uint16_t r = write_frame(f, out + out_off[i]);
        if (raw) raw[i] = r;
    }
}

void tso_build(hipStream_t st, int ipver, const nsx::IpHdrSoA& ip, const nsx::TsoMap& tso, const nsx::TcpHdrSoA& h,
               const uint8_t* opts, const uint64_t* opt_off, const uint8_t* data, const uint64_t* data_off,
               uint64_t data_bytes, uint64_t n_frames, uint8_t* out, const uint64_t* out_off, uint16_t* raw) {
    if (n_frames == 0) return;
    if (ipver != 4 && ipver != 6) die("segmentation: ipver %d", ipver);
    need(st, tso.frame_seg, n_frames * 4, "frame_seg");
    const uint64_t n = (uint64_t)tso.frame_seg[n_frames - 1] + 1;  // the frame map says how many super-segments
    need(st, tso.frame_first, (n + 1) * 8, "frame_first"), need(st, tso.mss, n * 4, "mss");
    need_fields(st, ipver, &ip, h, n);
    need(st, data_off, (n + 1) * 8, "data_off"), need(st, out_off, (n_frames + 1) * 8, "out_off");
    if (opt_off) need(st, opt_off, (n + 1) * 8, "opt_off");
    monotone(data_off, n, "data_off"), monotone(out_off, n_frames, "out_off");
    if (opt_off) monotone(opt_off, n, "opt_off");
    if (data_off[n] > data_bytes) die("data_off[n] = %llu > data_bytes = %llu", (ull)data_off[n], (ull)data_bytes);
    need(st, data, data_bytes, "payload buffer");
    if (opt_off) need(st, opts + opt_off[0], opt_off[n] - opt_off[0], "options");
    if (raw) need(st, raw, n_frames * 2, "raw sums");
    need(st, out + out_off[0], out_off[n_frames] - out_off[0], "frame slots");
    // the two halves of the frame map agree with each other and with the payload lengths
    if (tso.frame_first[0] != 0 || tso.frame_first[n] != n_frames) die("frame_first does not span [0, n_frames]");
    for (uint64_t s = 0; s < n; ++s) {
        const uint64_t len = data_off[s + 1] - data_off[s];
        if (tso.mss[s] == 0) die("mss[%llu] = 0", (ull)s);
        const uint64_t cnt = len ? (len + tso.mss[s] - 1) / tso.mss[s] : 1;
        if (tso.frame_first[s + 1] - tso.frame_first[s] != cnt)
            die("frame_first[%llu..] is not the frame count", (ull)s);
    }
    for (uint64_t f = 0; f < n_frames; ++f) {
        const uint64_t s = tso.frame_seg[f];
        if (s >= n || f < tso.frame_first[s] || f >= tso.frame_first[s + 1])
            die("frame_seg[%llu] = %llu disagrees with frame_first", (ull)f, (ull)s);
    }
    const uint32_t iph = ip_len(ipver);
    for (uint64_t f = 0; f < n_frames; ++f) {
        const uint64_t s = tso.frame_seg[f], j = f - tso.frame_first[s];
        const uint64_t cnt = tso.frame_first[s + 1] - tso.frame_first[s], mss = tso.mss[s], end = data_off[s + 1];
        const uint64_t lo = std::min(data_off[s] + j * mss, end), hi = std::min(lo + mss, end);
        const uint64_t olen = opt_off ? opt_off[s + 1] - opt_off[s] : 0, dlen = hi - lo;
        if (!fits_ip(ipver, wire_len(olen, dlen))) {
            if (raw) raw[f] = 0;
            continue;
        }
        check_slot(out_off, f, iph + wire_len(olen, dlen));
        Frame fr = make_frame(ipver, &ip, h, s, olen ? opts + opt_off[s] : nullptr, olen, dlen ? data + lo : nullptr,
                              dlen, 0);
        fr.seq = (uint32_t)(fr.seq + j * mss);
        if (j != cnt - 1) fr.ctl &= (uint8_t)~0x09;  // FIN and PSH only on the last frame
        if (j != 0) fr.ctl &= (uint8_t)~0x80;        // CWR only on the first
        fr.ident = (uint16_t)(fr.ident + j);
        const uint16_t r = write_frame(fr, out + out_off[f]);
        if (raw) raw[f] = r;
    }
}

}  // namespace ref

// ------------------------------------------------------------------ the launcher interface
namespace nsx {

// The real ones live in the kernel file (which tune names a kernel shape) and are covered by the GPU tests.
bool rx_tune_valid(const LaunchCfg&) { return true; }
bool ragged_tune_valid(const LaunchCfg&) { return true; }

hipError_t launch_fixed(const LaunchCfg&, const void* d_base, uint64_t stride, uint32_t seg_len, uint64_t n,
                        const uint32_t* partial, uint16_t* out, hipStream_t st) {
    return fake::enqueue(st, {d_base, partial, out},
                         [=] { ref::fixed(st, (const uint8_t*)d_base, stride, seg_len, n, partial, out); });
}

hipError_t launch_ragged(const LaunchCfg&, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         const uint32_t* partial, uint16_t* out, uint8_t* ok, hipStream_t st) {
    return fake::enqueue(st, {d_base, d_offsets, partial, out, ok},
                         [=] { ref::ragged(st, (const uint8_t*)d_base, d_offsets, n, partial, out, ok); });
}

hipError_t launch_rx_tcp(const LaunchCfg&, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         uint64_t* mask, uint16_t* ip_raw, uint16_t* tcp_raw, hipStream_t st) {
    if (ip_raw || tcp_raw) return hipErrorNotSupported;  // the host driver asks for the mask alone
    return fake::enqueue(st, {d_base, d_offsets, mask},
                         [=] { ref::rx_tcp(st, ipver, (const uint8_t*)d_base, d_offsets, n, mask); });
}

hipError_t launch_tcp_build(const LaunchCfg&, int ipver, const IpHdrSoA* ip, const TcpHdrSoA& h, const uint8_t* opts,
                            const uint64_t* opt_off, const uint8_t* data, const uint64_t* data_off,
                            uint64_t data_bytes, const uint32_t* partial, uint64_t n, uint8_t* out,
                            const uint64_t* out_off, uint16_t* raw, hipStream_t st) {
    const bool has_ip = ip != nullptr;
    const IpHdrSoA ipv = has_ip ? *ip : IpHdrSoA{};  // the caller's struct may be gone when the stream runs this
    return fake::enqueue(st, {h.src_port, opts, opt_off, data, data_off, partial, out, out_off, raw}, [=] {
        ref::tcp_build(st, ipver, has_ip ? &ipv : nullptr, h, opts, opt_off, data, data_off, data_bytes, partial, n,
                       out, out_off, raw);
    });
}

hipError_t launch_tso_build(const LaunchCfg&, int ipver, const IpHdrSoA& ip, const TsoMap& tso, const TcpHdrSoA& h,
                            const uint8_t* opts, const uint64_t* opt_off, const uint8_t* data,
                            const uint64_t* data_off, uint64_t data_bytes, uint64_t n_frames, uint8_t* out,
                            const uint64_t* out_off, uint16_t* raw, hipStream_t st) {
    const std::vector<const void*> blocks{h.src_port, tso.mss, tso.frame_first, opts, opt_off, data, data_off,
                                          out,        out_off, raw};
    return fake::enqueue(st, blocks, [=] {
        ref::tso_build(st, ipver, ip, tso, h, opts, opt_off, data, data_off, data_bytes, n_frames, out, out_off, raw);
    });
}

// ---- the rest of the interface: present so that csum_api.cpp links ----
uint64_t fixed_launch_count(const LaunchCfg&, uintptr_t, uint64_t, uint32_t, uint64_t) { return 0; }
uint64_t ipv4_hdr_launch_count(const LaunchCfg&, uintptr_t, uint64_t, uint32_t, uint64_t) { return 0; }
hipError_t launch_pseudo_ipv4(const uint8_t*, const uint8_t*, const uint32_t*, uint8_t, uint64_t, uint32_t*, uint32_t,
                              hipStream_t) {
    return hipErrorNotSupported;
}
hipError_t launch_pseudo_ipv6(const uint8_t*, const uint8_t*, const uint32_t*, uint8_t, uint64_t, uint32_t*, uint32_t,
                              hipStream_t) {
    return hipErrorNotSupported;
}
hipError_t launch_verify_mask(const uint16_t*, uint64_t, uint64_t*, uint32_t, hipStream_t) {
    return hipErrorNotSupported;
}
uint64_t gro_work_bytes(uint64_t) { return 0; }
hipError_t launch_gro(const LaunchCfg&, int, const void*, const uint64_t*, uint64_t, const uint64_t*, const GroOut&,
                      void*, hipStream_t) {
    return hipErrorNotSupported;
}
hipError_t launch_gro_ordered(const LaunchCfg&, int, const void*, const uint64_t*, uint64_t, const uint64_t*,
                              const uint32_t*, const GroOut&, void*, hipStream_t) {
    return hipErrorNotSupported;
}
uint64_t gro_flow_work_bytes(uint64_t) { return 0; }
hipError_t launch_gro_flow(const LaunchCfg&, int, const void*, const uint64_t*, uint64_t, const uint64_t*, uint32_t*,
                           const GroOut&, void*, hipStream_t) {
    return hipErrorNotSupported;
}
hipError_t launch_tcp_parse(const LaunchCfg&, const void*, const uint64_t*, uint64_t, const TcpParsedSoA&,
                            hipStream_t) {
    return hipErrorNotSupported;
}
hipError_t launch_ipv4_hdr(const LaunchCfg&, uint8_t*, uint64_t, uint32_t, uint64_t, int, uint16_t*, uint64_t*,
                           hipStream_t) {
    return hipErrorNotSupported;
}
void deal_release(hipStream_t) {}
uint32_t deal_sets_in_use(int) { return 0; }
hipError_t launch_fill_splitmix64(void*, uint64_t, uint64_t, uint64_t, uint32_t, hipStream_t) {
    return hipErrorNotSupported;
}

}  // namespace nsx
