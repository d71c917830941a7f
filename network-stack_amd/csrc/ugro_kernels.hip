// ugro_kernels.hip — gfx950 kernels of UDP receive coalescing (nsx_ugro_ipv4_dev / nsx_ugro_ipv6_dev and the
// flow-keyed nsx_ugro_flow_ipv4_dev / nsx_ugro_flow_ipv6_dev, include/nsx_csum.h): the inverse of UDP segmentation
// offload. Runs of consecutive datagrams of one flow become super-datagrams in the SoA format nsx_udp_uso_*_build_dev
// takes. The pass structure is that of gro_kernels.hip, which stays as it is; UDP is the simpler case — no option
// block, no sequence numbers, the payload starts 8 bytes behind the IP header, a head writes nine fields.
//
// Five launches, none of which waits on another workgroup:
//   head   per frame: member, same(i, i-1), payload and header lengths → one meta dword in the workspace. A wave owns
//          63 consecutive frames plus the frame before them in lane 0, so every header is fetched by one lane and the
//          neighbour's fields come by ds_bpermute.
//   reduce per scan block: the number of heads and the payload bytes.
//   scan   one workgroup: exclusive prefix sums of the block sums; writes n_super and the closing offset.
//   apply  per scan block: frame_seg, each frame's payload destination, and at heads first_frame / data_off; the last
//          frame of each run goes to the workspace.
//   emit   the hot path. A wave takes a group of consecutive frames and copies each payload to its destination offset:
//          16-byte loads through a descriptor clamped to the frame, realigned by the (source − destination) byte
//          shift, 16-byte stores at destination-aligned addresses, byte / short / dword stores at the two ends (two
//          datagrams' payloads may meet inside one dword, so nothing is read back). The lane that owns a head frame
//          also writes the super-datagram's fields.
//
// head, apply and emit are templates on ORDERED, as in gro_kernels.hip: ORDERED serves nsx_ugro_flow_* — position p of
// the batch is frame order[p]; offsets and the valid bit go through the order, meta / wdst / wlast stay in position
// space, frame_seg is scattered to the frame and first_frame holds positions. The order comes from the key pass below
// (ugro_key_kernel: UDP membership, FNV-1a over the addresses and the ports) and the radix sort of
// gro_flow_kernels.hip (launch_flow_sort).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csum_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

// meta dword of a frame (0 for a non-member): payload bytes (<= 65527), bytes from the frame's start to its payload
// (IP header + 8 <= 68), same(i, i-1), member
constexpr uint32_t kPayMask = 0xFFFFu;
constexpr uint32_t kHdrShift = 20;
constexpr uint32_t kSame = 1u << 28, kMember = 1u << 29;
constexpr uint32_t kHeadFrames = 63;   // frames per wave of the head pass (lane 0 holds the frame before them)
constexpr uint32_t kEmitGroup = 16;    // frames per wave task of the emit pass
constexpr uint32_t kScanBlockDefault = 4096, kScanBlockMin = 16, kScanBlockMax = 65536;
constexpr uint32_t kNoFlow = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t m_pay(uint32_t m) { return m & kPayMask; }
__device__ __forceinline__ uint32_t m_hdr(uint32_t m) { return (m >> kHdrShift) & 127u; }

// join(i) from the meta dwords of frames i, i-1 and i-2 (0 where there is no such frame): the three-frame window
// of include/nsx_csum.h.
__device__ __forceinline__ bool ugro_join(uint32_t m0, uint32_t m1, uint32_t m2) {
    const uint32_t p0 = m_pay(m0), p1 = m_pay(m1), p2 = m_pay(m2);
    return (m0 & kSame) && p0 >= 1u && p0 <= p1 && !((m1 & kSame) && p1 < p2);
}

// Well-formed as the UDP receive verify defines, up to the UDP header (include/nsx_csum.h: version, lengths, protocol
// / Next Header 17, no fragment, room for the 8 header bytes), from the frame's length (capped) and its header dwords
// 0, 1 and 2 (h2: IPv4 only). iph = the IP header's bytes, P = the IP payload's. The UDP length and the checksum field
// are udp_member's.
template <bool V6>
__device__ __forceinline__ bool udp_wellformed(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t flen, uint32_t& iph,
                                               uint32_t& P) {
    bool ok;
    if constexpr (V6) {
        iph = 40u;
        ok = flen >= 48u && (h0 & 0xF0u) == 0x60u && 40u + bswap16(h1) == flen && ((h1 >> 16) & 0xFFu) == 17u;
    } else {
        iph = (h0 & 15u) * 4u;
        ok = flen >= 28u && (h0 & 0xF0u) == 0x40u && iph >= 20u && iph <= flen && bswap16(h0 >> 16) == flen &&
             (h1 & 0xFF3F0000u) == 0u && ((h2 >> 8) & 0xFFu) == 17u && flen - iph >= 8u;
    }
    P = flen - iph;
    return ok;
}

// u1 = UDP header bytes 4-7 (length, checksum). 8 <= U <= P as the verify has it, U == P (no padding) and a checksum
// field that is not 0.
__device__ __forceinline__ bool udp_member(uint32_t u1, uint32_t P) {
    const uint32_t U = bswap16(u1);
    return U >= 8u && U == P && (u1 >> 16) != 0u;
}

// ------------------------------------------------------------------------------------------------ head pass
template <bool V6, bool ORDERED>
__global__ __launch_bounds__(kBlock) void ugro_head_kernel(const uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           const uint64_t* __restrict__ valid,
                                                           const uint32_t* __restrict__ order,
                                                           uint32_t* __restrict__ meta) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint64_t first = wave * kHeadFrames;  // lane 1's frame
    if (first >= n) return;                     // wave-uniform
    const int64_t fi = (int64_t)first + lane - 1;
    const bool live = fi >= 0 && fi < (int64_t)n;
    const uint32_t p = live ? (uint32_t)fi : 0u;  // the position; i: the frame
    uint32_t i = p;
    if constexpr (ORDERED) i = live ? order[p] : 0u;
    const uint64_t o0 = live ? offsets[i] : 0u, o1 = live ? offsets[(uint64_t)i + 1] : 0u;
    // a frame longer than any length field can say is no member; the cap keeps the window arithmetic in 32 bits
    const uint32_t flen = live ? (uint32_t)min(o1 - o0, (uint64_t)0x20000u) : 0u;
    const bool vbit = live && ((valid[i >> 6] >> (i & 63u)) & 1u);
    const FrameWin F = frame_win(base + o0, vbit ? flen : 0u);  // a frame the mask rejects is not read at all

    constexpr int NK = V6 ? 10 : 4;  // IP words that must be equal
    uint32_t K[NK];
    uint32_t iph, P, ident = 0;
    const uint32_t h0 = F.at(0), h1 = F.at(4), h2 = V6 ? 0u : F.at(8);
    bool ok = udp_wellformed<V6>(h0, h1, h2, flen, iph, P) && vbit;
    if constexpr (V6) {
        K[0] = h0;         // version, class, flow
        K[1] = h1 >> 24;   // hop limit
#pragma unroll
        for (int k = 0; k < 8; ++k) K[2 + k] = F.at(8 + 4 * k);
    } else {
        ident = bswap16(h1);
        // IHL 5 is a condition of same(), not of membership: a frame with IP options is a singleton
        K[0] = (h0 & 0xFFFFu) | (h1 & 0xFFFF0000u);  // version / IHL, TOS, bytes 6-7
        K[1] = h2 & 0xFFu;                           // TTL
        K[2] = F.at(12);
        K[3] = F.at(16);
    }
    if (!ok) iph = 0u;
    // well-formed: iph + 8 <= flen, so the UDP header is inside the frame (and the window clamps)
    const uint32_t ports = ok ? F.at(iph) : 0u, u1 = ok ? F.at(iph + 4u) : 0u;
    const bool member = ok && udp_member(u1, P);
    const uint32_t pay = member ? P - 8u : 0u;

    // the frame before: lane - 1 (lane 0's own result is not used)
    const uint32_t src = (lane + 63u) & 63u;
    // (every ds_bpermute runs with the whole wave active: nothing below is skipped for a lane)
    const uint32_t pmember = bperm(member ? 1u : 0u, src);
    bool same = member && pmember != 0u;
#pragma unroll
    for (int k = 0; k < NK; ++k) same = (bperm(K[k], src) == K[k]) && same;
    if constexpr (!V6) {
        same = (((bperm(ident, src) + 1u) & 0xFFFFu) == ident) && same;
        same = same && iph == 20u;  // the previous frame's IHL is equal (K[0])
    }
    same = (bperm(ports, src) == ports) && same;

    if (live && lane >= 1u)
        meta[p] = member ? pay | ((iph + 8u) << kHdrShift) | (same ? kSame : 0u) | kMember : 0u;
}

// ------------------------------------------------------------------------------------------------ key pass
// One lane per frame: the head pass's membership test, then FNV-1a over the address dwords and the ports dword;
// 0xFFFFFFFF for a non-member. Writes the key and the identity index (the radix sort's input).
template <bool V6>
__global__ __launch_bounds__(kBlock) void ugro_key_kernel(const uint8_t* __restrict__ base,
                                                          const uint64_t* __restrict__ offsets, uint32_t n,
                                                          const uint64_t* __restrict__ valid,
                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n) return;
    const uint32_t i = (uint32_t)gi;
    uint32_t key = kNoFlow;
    if ((valid[i >> 6] >> (i & 63u)) & 1u) {  // a frame the mask rejects is not read at all
        const uint64_t o0 = offsets[i], o1 = offsets[(uint64_t)i + 1];
        const uint32_t flen = (uint32_t)min(o1 - o0, (uint64_t)0x20000u);  // as the head pass caps it
        const FrameWin F = frame_win(base + o0, flen);
        uint32_t iph, P;
        const uint32_t h0 = F.at(0), h1 = F.at(4), h2 = V6 ? 0u : F.at(8);
        if (udp_wellformed<V6>(h0, h1, h2, flen, iph, P) && udp_member(F.at(iph + 4u), P)) {
            uint32_t h = 0x811C9DC5u;
            constexpr uint32_t kAddr = V6 ? 8u : 12u, kAddrDwords = V6 ? 8u : 2u;
#pragma unroll
            for (uint32_t k = 0; k < kAddrDwords; ++k) h = (h ^ F.at(kAddr + 4u * k)) * 0x01000193u;
            key = (h ^ F.at(iph)) * 0x01000193u;
        }
    }
    keys[i] = key;
    idx[i] = i;
}

// ------------------------------------------------------------------------------------------------ scan
// Exclusive prefix sums over the 256 threads of a block, K values at once; total[] = the block's sums.
template <int K>
__device__ __forceinline__ void block_excl_scan(uint64_t (&v)[K], uint64_t (&total)[K], uint64_t (*lds)[K]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t incl[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint64_t x = v[k];
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint64_t y = __shfl_up((unsigned long long)x, d, 64);
            if (lane >= d) x += y;
        }
        incl[k] = x;
        if (lane == 63u) lds[w][k] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        uint64_t pre = 0, tot = 0;
        for (uint32_t j = 0; j < kWavesPerBlock; ++j) {
            const uint64_t s = lds[j][k];
            if (j < w) pre += s;
            tot += s;
        }
        total[k] = tot;
        v[k] = incl[k] - v[k] + pre;
    }
    __syncthreads();
}

struct UgroFrame {
    uint32_t m, head, last;  // meta; a head; the last frame of its run
};

__device__ __forceinline__ UgroFrame ugro_frame(const uint32_t* __restrict__ meta, uint32_t i, uint32_t n, bool live,
                                                bool want_last) {
    UgroFrame f{0u, 0u, 0u};
    if (!live) return f;
    const uint32_t m0 = meta[i], m1 = i >= 1u ? meta[i - 1u] : 0u, m2 = i >= 2u ? meta[i - 2u] : 0u;
    f.m = m0;
    f.head = (m0 & kMember) && !ugro_join(m0, m1, m2);
    if (want_last && (m0 & kMember)) f.last = i + 1u == n || !ugro_join(meta[i + 1u], m0, m1);
    return f;
}

// APPLY false: sums[2b..] = the block's (heads, payload bytes). APPLY true: sums holds the exclusive prefix of those
// over the blocks, and the per-frame and per-head outputs are written.
// ORDERED (with APPLY): i is a position; frame_seg is scattered to the frame order[i], all else stays by position.
template <bool APPLY, bool ORDERED>
__global__ __launch_bounds__(kBlock) void ugro_scan_block_kernel(const uint32_t* __restrict__ meta, uint32_t n,
                                                                 uint32_t per_block, uint64_t* __restrict__ sums,
                                                                 uint64_t* __restrict__ wdst,
                                                                 uint32_t* __restrict__ wlast,
                                                                 const uint32_t* __restrict__ order, UgroOut o) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(lo + per_block, (uint64_t)n);
    uint64_t carry[2] = {0, 0};
    if (APPLY) {
        carry[0] = sums[2u * blockIdx.x];
        carry[1] = sums[2u * blockIdx.x + 1u];
    }
    for (uint64_t t = lo; t < hi; t += kBlock) {  // block-uniform trip count
        const uint64_t fi = t + threadIdx.x;
        const bool live = fi < hi;
        const uint32_t i = (uint32_t)fi;
        const UgroFrame f = ugro_frame(meta, i, n, live, APPLY);
        uint64_t v[2] = {f.head, m_pay(f.m)}, tot[2];
        block_excl_scan<2>(v, tot, lds);
        if (APPLY && live) {
            const bool member = f.m & kMember;
            const uint32_t s = (uint32_t)(carry[0] + v[0]) + f.head - 1u;
            o.frame_seg[ORDERED ? order[i] : i] = member ? s : 0xFFFFFFFFu;
            wdst[i] = carry[1] + v[1];
            if (f.head) {
                o.first_frame[s] = i;
                o.data_off[s] = carry[1] + v[1];
            }
            if (f.last) wlast[s] = i;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) carry[k] += tot[k];
    }
    if (!APPLY && threadIdx.x == 0) {
        sums[2u * blockIdx.x] = carry[0];
        sums[2u * blockIdx.x + 1u] = carry[1];
    }
}

// One workgroup: sums (nb pairs) → their exclusive prefix in place; the totals close the outputs.
__global__ __launch_bounds__(kBlock) void ugro_scan_sums_kernel(uint64_t* __restrict__ sums, uint32_t nb, UgroOut o) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    uint64_t carry[2] = {0, 0};
    for (uint32_t t = 0; t < nb; t += kBlock) {
        const uint32_t b = t + threadIdx.x;
        const bool live = b < nb;
        uint64_t v[2], tot[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = live ? sums[2u * b + k] : 0u;
        block_excl_scan<2>(v, tot, lds);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (live) sums[2u * b + k] = carry[k] + v[k];
            carry[k] += tot[k];
        }
    }
    if (threadIdx.x == 0) {
        *o.n_super = carry[0];
        if (nb == 0) o.data_off[0] = 0;  // with frames, entry 0 belongs to the first head (or is the total)
        o.data_off[carry[0]] = carry[1];
    }
}

// ------------------------------------------------------------------------------------------------ emit + copy
// Bytes [lo, hi) of the 16-byte chunk x to q (16-aligned): whole dwords where the range covers them, else shorts
// and bytes; nothing outside the range is touched.
__device__ __forceinline__ void store_edge(uint8_t* q, u32x4 x, int32_t lo, int32_t hi) {
    const uint32_t d[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int32_t s = min(max(lo - 4 * k, 0), 4), e = min(max(hi - 4 * k, 0), 4);
        if (s >= e) continue;
        uint8_t* p = q + 4 * k;
        if (s == 0 && e == 4) {
            *reinterpret_cast<uint32_t*>(p) = d[k];
            continue;
        }
        if (s == 0 && e >= 2) {
            *reinterpret_cast<uint16_t*>(p) = (uint16_t)d[k];
        } else {
            if (s == 0) p[0] = (uint8_t)d[k];
            if (s <= 1 && e > 1) p[1] = (uint8_t)(d[k] >> 8);
        }
        if (s <= 2 && e == 4) {
            *reinterpret_cast<uint16_t*>(p + 2) = (uint16_t)(d[k] >> 16);
        } else {
            if (s <= 2 && e > 2) p[2] = (uint8_t)(d[k] >> 16);
            if (s <= 3 && e > 3) p[3] = (uint8_t)(d[k] >> 24);
        }
    }
}

typedef uint32_t a16x4 __attribute__((ext_vector_type(4)));  // 16-aligned: one global_store_dwordx4

// One datagram's payload copy, wave-uniform: destination chunk c is the 16 bytes at q0 + 16c (q0 16-aligned), of
// which bytes [a, end) from q0 belong to the payload; its source bytes start sh bytes into offset 16c of srs, a
// descriptor from the 4-aligned address at or below (payload − a) — at most 18 bytes below the payload, so at least
// 10 bytes into the frame, whose headers take 28 — to the dword holding the frame's last byte (a member has no
// padding: its payload ends with the frame). chunks == 0: no job.
struct CopyJob {
    __amdgpu_buffer_rsrc_t srs;
    uint8_t* q0;
    uint32_t a, end, sh, chunks;
};

// The next frame of the group, from k on, that has payload (k moves past it); chunks = 0 when there is none.
__device__ __forceinline__ CopyJob next_job(const uint8_t* __restrict__ base, uint8_t* data, uint32_t m, uint64_t off,
                                            uint64_t dst, uint32_t cnt, uint32_t& k) {
    CopyJob j{make_rsrc(base, 0), data, 0u, 0u, 0u, 0u};
    while (k < cnt) {
        const uint32_t mk = __builtin_amdgcn_readlane(m, k);
        const uint32_t L = m_pay(mk);
        if (L == 0u) {
            ++k;
            continue;
        }
        const uint8_t* sp = base + readlane64(off, k) + m_hdr(mk);  // the payload: it ends with the frame
        uint8_t* dp = data + readlane64(dst, k);
        ++k;
        j.a = (uint32_t)((uintptr_t)dp & 15u);
        j.q0 = dp - j.a;
        const uint8_t* s0 = sp - j.a;
        j.sh = (uint32_t)((uintptr_t)s0 & 3u);
        j.srs = make_rsrc(s0 - j.sh, ((uint64_t)(j.sh + j.a + L) + 3u) & ~3ull);
        j.end = j.a + L;
        j.chunks = (j.end + 15u) >> 4;
        break;
    }
    return j;
}

struct RowPair {
    u32x4 lo[2];
    uint32_t hi[2];
};

// Chunks c0 + lane and c0 + 64 + lane of job j: five source dwords each (the fifth only when the copy shifts).
__device__ __forceinline__ RowPair load_pair(const CopyJob& j, uint32_t c0, uint32_t lane) {
    RowPair p;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t c = c0 + r * kWave + lane;
        const bool on = c < j.chunks;
        p.lo[r] = bld16<true>(j.srs, on ? c * 16u : kOOB);
        p.hi[r] = __builtin_amdgcn_raw_buffer_load_b32(j.srs, on && j.sh ? c * 16u + 16u : kOOB, 0, 2);
    }
    return p;
}

__device__ __forceinline__ void store_pair(const CopyJob& j, uint32_t c0, uint32_t lane, const RowPair& p) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const uint32_t c = c0 + r * kWave + lane;
        if (c >= j.chunks) continue;
        const u32x4 x = j.sh ? realign(p.lo[r], p.hi[r], j.sh) : p.lo[r];
        const int32_t b0 = (int32_t)j.a - (int32_t)(c * 16u), b1 = (int32_t)j.end - (int32_t)(c * 16u);
        uint8_t* q = j.q0 + (uint64_t)c * 16u;
        if (b0 <= 0 && b1 >= 16) *reinterpret_cast<a16x4*>(q) = a16x4{x.x, x.y, x.z, x.w};
        else store_edge(q, x, max(b0, 0), min(b1, 16));
    }
}

// The nine fields of the super-datagram s whose first frame is at position i (one lane): src, dst, ident, ttl, tclass,
// flow, the two ports and gso — and frame_cnt from the run's last frame.
template <bool V6>
__device__ __forceinline__ void emit_head(const uint8_t* __restrict__ base, const uint32_t* __restrict__ wlast,
                                          const UgroOut& o, uint32_t i, uint32_t s, uint32_t m, uint64_t off) {
    const uint32_t hdr = m_hdr(m), pay = m_pay(m);
    const uint32_t iph = hdr - 8u;
    const FrameWin F = frame_win(base + off, hdr + pay);
    if constexpr (V6) {
        const uint32_t h0 = bswap32(F.at(0));
        uint32_t* sp = reinterpret_cast<uint32_t*>(o.src) + 4ull * s;  // 16-byte rows of a device allocation
        uint32_t* dp = reinterpret_cast<uint32_t*>(o.dst) + 4ull * s;
        const bool al = (((uintptr_t)o.src | (uintptr_t)o.dst) & 3u) == 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a = F.at(8 + 4 * k), b = F.at(24 + 4 * k);
            if (al) {
                sp[k] = a;
                dp[k] = b;
            } else {
                for (int j = 0; j < 4; ++j) {
                    o.src[16ull * s + 4 * k + j] = (uint8_t)(a >> (8 * j));
                    o.dst[16ull * s + 4 * k + j] = (uint8_t)(b >> (8 * j));
                }
            }
        }
        o.ident[s] = 0;
        o.ttl[s] = (uint8_t)(F.at(4) >> 24);
        o.tclass[s] = (uint8_t)(h0 >> 20);
        o.flow[s] = h0 & 0xFFFFFu;
    } else {
        const uint32_t h0 = F.at(0), a = F.at(12), b = F.at(16);
        for (int j = 0; j < 4; ++j) {
            o.src[4ull * s + j] = (uint8_t)(a >> (8 * j));
            o.dst[4ull * s + j] = (uint8_t)(b >> (8 * j));
        }
        o.ident[s] = (uint16_t)bswap16(F.at(4));
        o.ttl[s] = (uint8_t)F.at(8);
        o.tclass[s] = (uint8_t)(h0 >> 8);
        o.flow[s] = 0;
    }
    const uint32_t t0 = F.at(iph);
    o.src_port[s] = (uint16_t)bswap16(t0);
    o.dst_port[s] = (uint16_t)bswap16(t0 >> 16);
    o.gso[s] = max(pay, 1u);
    o.frame_cnt[s] = wlast[s] - i + 1u;
}

// ORDERED: lane j's frame is order[g0 + j]; its offset and its frame_seg entry go through the order, meta, wdst,
// wlast and first_frame are by position.
template <bool V6, bool ORDERED>
__global__ __launch_bounds__(kBlock) void ugro_emit_kernel(const uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           const uint32_t* __restrict__ meta,
                                                           const uint64_t* __restrict__ wdst,
                                                           const uint32_t* __restrict__ wlast,
                                                           const uint32_t* __restrict__ order, UgroOut o) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t groups = ((uint64_t)n + kEmitGroup - 1u) / kEmitGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += nwaves) {
        const uint32_t g0 = (uint32_t)(g * kEmitGroup), cnt = min(kEmitGroup, n - g0);
        // lane j < cnt: the frame at position g0 + j
        const bool own = lane < cnt;
        const uint32_t i = g0 + (own ? lane : 0u);
        const uint32_t m = own ? meta[i] : 0u;
        uint32_t f = i;  // the frame at position i
        if constexpr (ORDERED) f = own ? order[i] : 0u;
        const uint64_t off = own ? offsets[f] : 0u, dst = own ? wdst[i] : 0u;
        if (m & kMember) {
            const uint32_t s = o.frame_seg[f];
            if (o.first_frame[s] == i) emit_head<V6>(base, wlast, o, i, s, m, off);
        }
        // The group's payloads as one stream of row pairs (2 KiB of destination each), software-pipelined: the
        // loads of the next pair — of this frame, or the first of the next frame with a payload — are issued
        // before the current pair is stored. A pair past the group's end loads nothing (every offset out of range).
        uint32_t k = 0;
        CopyJob cur = next_job(base, o.data, m, off, dst, cnt, k);
        uint32_t c0 = 0;
        RowPair A = load_pair(cur, c0, lane);
        while (cur.chunks) {  // wave-uniform
            CopyJob nj = cur;
            uint32_t nc = c0 + 2u * kWave;
            if (nc >= cur.chunks) {
                nj = next_job(base, o.data, m, off, dst, cnt, k);
                nc = 0;
            }
            const RowPair B = load_pair(nj, nc, lane);
            store_pair(cur, c0, lane, A);
            cur = nj;
            c0 = nc;
            A = B;
        }
    }
}

uint32_t scan_block_frames(const LaunchCfg& c) {
    if (c.run_segs <= 0) return kScanBlockDefault;
    return std::min<uint32_t>(std::max<uint32_t>((uint32_t)c.run_segs, kScanBlockMin), kScanBlockMax);
}

struct UgroWork {
    uint64_t sums, wdst, meta, wlast, total;  // byte offsets from the workspace rounded up to 8
};

UgroWork ugro_layout(uint64_t n) {
    UgroWork w;
    const uint64_t nb_max = (n + kScanBlockMin - 1) / kScanBlockMin;  // the smallest scan block a tune can ask for
    w.sums = 0;
    w.wdst = w.sums + 16 * (nb_max + 1);
    w.meta = w.wdst + 8 * n;
    w.wlast = w.meta + 4 * n;
    w.total = w.wlast + 4 * n + 8;  // + the rounding of the caller's pointer
    return w;
}

// where the sort's scratch starts behind the passes' own (both rounded to 8)
uint64_t flow_sort_at(uint64_t n) { return (ugro_layout(n).total + 7u) & ~7ull; }

template <bool ORDERED>
hipError_t launch_ugro_passes(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets,
                              uint64_t n64, const uint64_t* valid, const uint32_t* order, const UgroOut& o, void* work,
                              hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (ugro_api.cpp)
    const UgroWork L = ugro_layout(n);
    uint8_t* w = reinterpret_cast<uint8_t*>(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    uint64_t* sums = reinterpret_cast<uint64_t*>(w + L.sums);
    uint64_t* wdst = reinterpret_cast<uint64_t*>(w + L.wdst);
    uint32_t* meta = reinterpret_cast<uint32_t*>(w + L.meta);
    uint32_t* wlast = reinterpret_cast<uint32_t*>(w + L.wlast);
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    const uint32_t per = scan_block_frames(c);
    const uint32_t nb = (uint32_t)(((uint64_t)n + per - 1) / per);
    if (n) {
        const uint64_t hw = ((uint64_t)n + kHeadFrames - 1) / kHeadFrames;
        const uint32_t hgrid = (uint32_t)((hw + kWavesPerBlock - 1) / kWavesPerBlock);
        if (ipver == 6)
            hipLaunchKernelGGL((ugro_head_kernel<true, ORDERED>), dim3(hgrid), dim3(kBlock), 0, st, base, d_offsets, n,
                               valid, order, meta);
        else
            hipLaunchKernelGGL((ugro_head_kernel<false, ORDERED>), dim3(hgrid), dim3(kBlock), 0, st, base, d_offsets,
                               n, valid, order, meta);
        // the reduce pass reads meta only: one instantiation serves both
        hipLaunchKernelGGL((ugro_scan_block_kernel<false, false>), dim3(nb), dim3(kBlock), 0, st, meta, n, per, sums,
                           wdst, wlast, order, o);
    }
    hipLaunchKernelGGL(ugro_scan_sums_kernel, dim3(1), dim3(kBlock), 0, st, sums, nb, o);
    if (n) {
        hipLaunchKernelGGL((ugro_scan_block_kernel<true, ORDERED>), dim3(nb), dim3(kBlock), 0, st, meta, n, per, sums,
                           wdst, wlast, order, o);
        const int bpc = c.blocks_per_cu >= 1 && c.blocks_per_cu <= 8 ? c.blocks_per_cu : 8;
        const uint64_t groups = ((uint64_t)n + kEmitGroup - 1) / kEmitGroup;
        const uint32_t egrid = (uint32_t)std::min<uint64_t>((groups + kWavesPerBlock - 1) / kWavesPerBlock,
                                                            (uint64_t)std::max(c.cus, 1) * bpc);
        if (ipver == 6)
            hipLaunchKernelGGL((ugro_emit_kernel<true, ORDERED>), dim3(egrid), dim3(kBlock), 0, st, base, d_offsets, n,
                               meta, wdst, wlast, order, o);
        else
            hipLaunchKernelGGL((ugro_emit_kernel<false, ORDERED>), dim3(egrid), dim3(kBlock), 0, st, base, d_offsets,
                               n, meta, wdst, wlast, order, o);
    }
    return hipGetLastError();
}

}  // namespace

uint64_t ugro_work_bytes(uint64_t n) { return ugro_layout(n).total; }

uint64_t ugro_flow_work_bytes(uint64_t n) { return flow_sort_at(n) + flow_sort_bytes(n) + 8; }

hipError_t launch_ugro(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                       const uint64_t* valid, const UgroOut& o, void* work, hipStream_t st) {
    return launch_ugro_passes<false>(c, ipver, d_base, d_offsets, n, valid, nullptr, o, work, st);
}

hipError_t launch_ugro_flow(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n64,
                            const uint64_t* valid, uint32_t* d_order, const UgroOut& o, void* work, hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (ugro_api.cpp)
    uint8_t* w = reinterpret_cast<uint8_t*>(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    if (n) {
        const FlowSortWork S = flow_sort_work(w + flow_sort_at(n), n);
        const uint8_t* base = static_cast<const uint8_t*>(d_base);
        const uint32_t kgrid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
        if (ipver == 6)
            hipLaunchKernelGGL(ugro_key_kernel<true>, dim3(kgrid), dim3(kBlock), 0, st, base, d_offsets, n, valid,
                               S.keys[0], S.idx[0]);
        else
            hipLaunchKernelGGL(ugro_key_kernel<false>, dim3(kgrid), dim3(kBlock), 0, st, base, d_offsets, n, valid,
                               S.keys[0], S.idx[0]);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = launch_flow_sort(c, n, S, d_order, st);
        if (e != hipSuccess) return e;
    }
    return launch_ugro_passes<true>(c, ipver, d_base, d_offsets, n64, valid, d_order, o, w, st);
}

}  // namespace nsx
