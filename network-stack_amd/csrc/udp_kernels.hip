// udp_kernels.hip — the gfx950 kernels of the UDP passes (include/nsx_csum.h nsx_udp_*): the fused transmit pass
// (nsx_udp_tx_*), its segmentation offload (nsx_udp_uso_*) and the receive verify (nsx_udp_rx_*). A kernel file of
// its own beside csum_kernels.hip, whose code objects it leaves as they are; the helpers that live only there
// (sad4, fold32, wave_sum, bswap16u) are copied, the shared ones come from kernel_util.h.
//
// The work is the TCP transmit pass's — copy and sum at HBM speed — in the same shape: wave64, a wave task = a group
// of consecutive frames whose metadata the lanes load once (lane j: frame g0 + j), 16 B per lane buffer loads
// through a descriptor clamped to the frame's own dwords, v_alignbyte for the source alignment, v_sad_u16
// accumulation with one wave reduction per frame, 1 KiB rows, the next frame's first two rows in flight while this
// one is summed and stored. UDP lets three things go:
//   * There are no options and the headers are 28 / 48 bytes, so the payload lands 4-aligned in the frame. The rows
//     are therefore laid over the PAYLOAD, not the frame: chunk c of a frame is payload bytes [16c, 16c + 16), read
//     from the payload's own aligned dwords and stored at frame byte H + 16c. No chunk straddles the header edge,
//     so no row needs per-dword clamped loads or a head mask; only the row holding the payload's end is masked.
//   * The headers never travel through the wave. The lane that loaded a frame's fields keeps its 7 / 12 header
//     dwords, receives the frame's folded payload sum (parked in lane k as the wave goes), adds its own partial —
//     pseudo-header + ports + length, summed in the big-endian domain in the metadata phase — and stores header,
//     checksum field and raw sum itself when the group is done: no v_readlane per header dword per frame, and no
//     held-back checksum dword.
//   * The IPv4 header is summed by its own lane and so never enters the wave's sum: the "header sums to 0xFFFF"
//     argument of tcp_build_kernel is not needed, the partial is the pseudo-header's outright.
// A built frame's raw sum is never 0: the partial holds the byte 17 and fold32 keeps a nonzero sum nonzero.
// A payload (receive: a datagram) of at most kLaneMax bytes does not go to the wave at all: the lane that holds its
// metadata copies and sums it, 64 frames at once, and the wave loop runs over the ballot of the longer ones.
//
// Receive: a wave task is one mask word — 64 consecutive frames — taken in steps of `step` frames (run_segs):
// lane j reads frame j's header through FrameWin (nothing outside the dwords that hold the frame's own bytes),
// decides well-formedness, sums the IPv4 header and the pseudo-header; the wave then sums the first U bytes of each
// well-formed datagram (SegWin's window: base rounded down to 4 bytes, the head and tail dwords masked, the total
// byte-swapped iff the datagram starts at an even address) and lane j gives the verdict. The split is static.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csum_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

// ---- copied from csum_kernels.hip (they live only there) ----
__device__ __forceinline__ uint32_t sad4(u32x4 v, uint32_t acc) {
    acc = __builtin_amdgcn_sad_u16(v.x, 0u, acc);
    acc = __builtin_amdgcn_sad_u16(v.y, 0u, acc);
    acc = __builtin_amdgcn_sad_u16(v.z, 0u, acc);
    acc = __builtin_amdgcn_sad_u16(v.w, 0u, acc);
    return acc;
}

__device__ __forceinline__ uint32_t fold32(uint32_t s) {
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

// Wave-wide sum of a per-lane value < 2^26: DPP row_ror inside each 16-lane row, then the 4 row totals.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x128, 0xF, 0xF, false);  // row_ror:8
    v += __builtin_amdgcn_update_dpp(0u, v, 0x124, 0xF, 0xF, false);  // row_ror:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x122, 0xF, 0xF, false);  // row_ror:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x121, 0xF, 0xF, false);  // row_ror:1
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

__device__ __forceinline__ uint32_t bswap16u(uint32_t v) { return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu); }
// ---- end of copies ----

// The two big-endian 16-bit words of a little-endian dword, added up.
__device__ __forceinline__ uint32_t be_words(uint32_t w) {
    const uint32_t b = bswap32(w);
    return (b >> 16) + (b & 0xFFFFu);
}

constexpr uint32_t kPre = 2;  // rows of the next frame in flight while this one is built
// Payloads / datagrams of at most this many bytes are not worth a wave each: the lane that holds the frame's
// metadata copies and sums (receive: sums) it itself, dword by dword over the frame's own aligned dwords, 64 frames
// at once; the wave then takes only the longer ones. The 64 lanes of a group read one contiguous span of the batch.
constexpr uint32_t kLaneMax = 256;

// Rows r0 .. r0 + kPre - 1 of one window: 4 + 1 dwords per lane and row.
struct Rows {
    u32x4 lo[kPre];
    uint32_t hi[kPre];
};

// sh: whether the fifth dword is needed (the window does not start on its first byte)
__device__ __forceinline__ void load_rows(__amdgpu_buffer_rsrc_t rs, uint32_t r0, uint32_t lane, bool sh, Rows& R) {
#pragma unroll
    for (uint32_t r = 0; r < kPre; ++r) {
        const uint32_t at = (r0 + r) * kRow + lane * 16u;
        R.lo[r] = bld16<false>(rs, at);
        R.hi[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, sh ? at + 16u : kOOB, 0, 0);
    }
}

// The descriptor over the aligned dwords that hold bytes [p, p + len) (none for len 0 or a dead frame), and p & 3.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t own_dwords(const uint8_t* p, uint32_t len, bool live, uint32_t& sh) {
    sh = (uint32_t)((uintptr_t)p & 3u);
    return make_rsrc(p - sh, live && len ? (uint64_t)((sh + len + 3u) & ~3u) : 0u);
}

struct UdpSoA {
    const uint16_t* src_port;
    const uint16_t* dst_port;
};

struct UsoArgs {
    const uint32_t* gso;          // per super-datagram: payload bytes per datagram (>= 1)
    const uint64_t* frame_first;  // per super-datagram: its first frame
    const uint32_t* frame_seg;    // per frame: its super-datagram
    uint64_t n_super;
};

// IPH 20 / 40: whole IPv4 / IPv6 datagrams carrying UDP. USO: the field and data_off arrays hold one entry per
// super-datagram, n / out_off / raw_out count frames; only the metadata phase differs (the frame's slice of its
// super-datagram's payload, clamped to that range whatever the frame map says, and ident + j).
template <int IPH, bool USO>
__global__ __launch_bounds__(kBlock) void udp_build_kernel(IpHdrSoA ip, UdpSoA udp, const uint8_t* __restrict__ data,
                                                           const uint64_t* __restrict__ data_off, uint64_t n,
                                                           uint32_t no_csum, uint8_t* __restrict__ out,
                                                           const uint64_t* __restrict__ out_off,
                                                           uint16_t* __restrict__ raw_out, uint32_t group,
                                                           UsoArgs uso) {
    static_assert(IPH == 20 || IPH == 40, "IPv4 or IPv6 datagrams");
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    constexpr uint32_t H = IPH + 8u;                       // payload position in the frame
    constexpr uint32_t kMaxPay = IPH == 20 ? 65507u : 65527u;
    constexpr int kA = IPH == 20 ? 1 : 4;                  // dwords per address
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t ngroups = (n + group - 1) / group;
    for (uint64_t g = (uint64_t)blockIdx.x * kWavesPerBlock + wave; g < ngroups;
         g += (uint64_t)gridDim.x * kWavesPerBlock) {
        const uint64_t g0 = g * group;
        const uint32_t cnt = (uint32_t)min((uint64_t)group, n - g0);
        // ---- per-lane metadata of frame g0 + lane (lanes past cnt repeat the last one and store nothing) ----
        const uint64_t fr = g0 + min(lane, cnt - 1u);
        uint64_t i = fr;
        uint64_t mdb, mde;
        uint32_t tj16 = 0;  // USO: the frame's index in its super-datagram, modulo 2^16 (the ident)
        if constexpr (USO) {
            i = min((uint64_t)uso.frame_seg[fr], uso.n_super - 1u);
            const uint64_t tj = fr - uso.frame_first[i];
            tj16 = (uint32_t)tj & 0xFFFFu;
            const uint64_t b = data_off[i], e = max(data_off[i + 1], b), gso = uso.gso[i];
            // the slice [b + j·gso, min(b + (j+1)·gso, e)) inside [b, e) whatever the frame map says: j is taken
            // as a 32-bit count first, so that j·gso cannot wrap 64 bits
            const uint64_t adv = min(tj, (uint64_t)0xFFFFFFFFu) * gso;
            mdb = adv >= e - b ? e : b + adv;
            mde = gso >= e - mdb ? e : mdb + gso;
        } else {
            mdb = data_off[i];
            mde = max(data_off[i + 1], mdb);
        }
        const uint64_t moo = out_off[fr];
        // the length from the 64-bit difference, classified before it is narrowed
        const uint64_t len64 = mde - mdb;
        const bool mskip = len64 > kMaxPay;  // does not fit the IP length field: not built, raw 0
        const uint32_t mlen = mskip ? 0u : (uint32_t)len64;
        const uint32_t ulen = 8u + mlen;
        const uint32_t sp = udp.src_port[i], dp = udp.dst_port[i];
        const uint32_t ttl = ip.ttl ? (uint32_t)ip.ttl[i] : 64u;
        const bool al = (((uintptr_t)ip.src | (uintptr_t)ip.dst) & 3u) == 0;  // wave-uniform
        uint32_t a[2 * kA];
#pragma unroll
        for (int w = 0; w < 2 * kA; ++w) {
            const uint8_t* q = (w < kA ? ip.src : ip.dst) + (uint64_t)(4 * kA) * i + 4 * (w % kA);
            a[w] = al ? *reinterpret_cast<const uint32_t*>(q)
                      : (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        }
        uint32_t as = 0;  // the addresses' big-endian words
#pragma unroll
        for (int w = 0; w < 2 * kA; ++w) as += be_words(a[w]);
        // pseudo-header (addresses, 17, UDP length) + UDP header (ports, length, field 0): < 2^21
        const uint32_t mpart = as + 17u + ulen + sp + dp + ulen;
        uint32_t I[IPH / 4];  // the IP header dwords as stored
        if constexpr (IPH == 20) {
            const uint32_t ident = ((ip.ident ? (uint32_t)ip.ident[i] : 0u) + tj16) & 0xFFFFu;
            I[0] = 0x45u | (bswap16u(20u + ulen) << 16);
            I[1] = bswap16u(ident) | (0x40u << 16);  // DF, fragment offset 0
            I[2] = ttl | (17u << 8);
            I[3] = a[0], I[4] = a[1];
            const uint32_t hs = be_words(I[0]) + be_words(I[1]) + be_words(I[2]) + as;
            I[2] |= bswap16u(~fold32(hs) & 0xFFFFu) << 16;  // RFC 791 §3.1
        } else {
            const uint32_t vtf = (6u << 28) | ((ip.tclass ? (uint32_t)ip.tclass[i] : 0u) << 20) |
                                 ((ip.flow ? ip.flow[i] : 0u) & 0xFFFFFu);
            I[0] = bswap32(vtf);
            I[1] = bswap16u(ulen) | (17u << 16) | (ttl << 24);
#pragma unroll
            for (int w = 0; w < 8; ++w) I[2 + w] = a[w];
        }
        // ---- small payloads: each lane copies and sums its own (kLaneMax: see above) ----
        uint32_t psum = 0;  // frame's payload sum, folded (LE halves): the lane's own, or parked in lane k by the wave
        const bool mine = lane < cnt && mlen != 0u && mlen <= kLaneMax;
        if (mine) {
            const uint8_t* p = data + mdb;
            const uint32_t sh = (uint32_t)((uintptr_t)p & 3u), wend = sh + mlen;  // window bytes [sh, wend)
            const uint32_t* w = reinterpret_cast<const uint32_t*>(p - sh);       // the payload's own aligned dwords
            uint32_t* o = reinterpret_cast<uint32_t*>(out + moo + H);
            uint32_t acc = 0, cur = w[0];
            for (uint32_t d = 0; 4u * d < mlen; ++d) {
                const uint32_t nxt = 4u * (d + 1u) < wend ? w[d + 1u] : 0u;
                uint32_t x = __builtin_amdgcn_alignbyte(nxt, cur, sh);
                if (4u * d + 4u > mlen) x &= (1u << (8u * (mlen - 4u * d))) - 1u;  // the last dword: zero padding
                acc = __builtin_amdgcn_sad_u16(x, 0u, acc);
                o[d] = x;
                cur = nxt;
            }
            psum = fold32(acc);
        }
        const uint32_t mwl = mine ? 0u : mlen;  // what is left to the wave
        // ---- the wave builds the other payloads one after another ----
        auto rs_of = [&](uint32_t k, uint32_t& sh) {
            return own_dwords(data + readlane64(mdb, k), __builtin_amdgcn_readlane(mwl, k), true, sh);
        };
        auto fetch = [&](uint32_t k, Rows& R) {
            uint32_t sh;
            const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
            load_rows(rs, 0, lane, sh != 0, R);
        };
        auto build = [&](uint32_t k, Rows& R) {
            const uint32_t len = __builtin_amdgcn_readlane(mwl, k);
            uint32_t sh;
            const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
            const uint32_t nb4 = (len + 3u) & ~3u, rows = (nb4 + kRow - 1u) / kRow;
            // the payload's slot: stores past its last dword are dropped (per-dword range check), so the tail
            // chunk needs no branch; the bytes between len and nb4 are the zero padding
            const __amdgpu_buffer_rsrc_t ors = make_rsrc(out + readlane64(moo, k) + H, nb4);
            uint32_t acc = 0;
            for (uint32_t r0 = 0; r0 < rows; r0 += kPre) {
                if (r0) load_rows(rs, r0, lane, sh != 0, R);
#pragma unroll
                for (uint32_t r = 0; r < kPre; ++r) {
                    const uint32_t pos = (r0 + r) * kRow + lane * 16u;
                    u32x4 x = sh ? realign(R.lo[r], R.hi[r], sh) : R.lo[r];
                    if ((r0 + r + 1u) * kRow > len)  // the row with the payload's end (and any row past it)
                        x = keep_bytes(x, 0, min(max((int32_t)len - (int32_t)pos, 0), 16));
                    acc = sad4(x, acc);
                    __builtin_amdgcn_raw_buffer_store_b128(v4u{x.x, x.y, x.z, x.w}, ors, pos, 0, 0);
                }
                acc = fold32(acc);
            }
            const uint32_t s = fold32(wave_sum(acc));
            psum = lane == k ? s : psum;
        };
        // over the frames that have something for the wave (lanes past cnt repeat frame cnt - 1: masked out), the
        // next one's first rows in flight while this one is built
        uint64_t todo = __ballot(mwl != 0u && lane < cnt);
        if (todo) {
            Rows A, B;
            uint32_t k = (uint32_t)__builtin_ctzll(todo);
            todo &= todo - 1u;
            fetch(k, A);
            for (;;) {
                const uint32_t k2 = todo ? (uint32_t)__builtin_ctzll(todo) : kWave;
                todo &= todo - 1u;
                if (k2 < kWave) fetch(k2, B);
                build(k, A);
                if (k2 == kWave) break;
                k = todo ? (uint32_t)__builtin_ctzll(todo) : kWave;
                todo &= todo - 1u;
                if (k < kWave) fetch(k, A);
                build(k2, B);
                if (k == kWave) break;
            }
        }
        // ---- each lane finishes its own frame: checksum, headers, raw ----
        // the payload starts at an even frame position and its chunks start on it: LE half = swapped BE word
        const uint32_t raw = mskip ? 0u : fold32(bswap16u(psum) + mpart);
        if (lane < cnt) {
            if (!mskip) {
                uint32_t field = ~raw & 0xFFFFu;
                field = field ? field : 0xFFFFu;  // RFC 768: a computed 0 is sent as all ones
                if (no_csum) field = 0u;
                const uint32_t U0 = bswap16u(sp) | (bswap16u(dp) << 16);
                const uint32_t U1 = bswap16u(ulen) | (bswap16u(field) << 16);
                uint32_t* o = reinterpret_cast<uint32_t*>(out + moo);  // 4-aligned (the layout rule)
#pragma unroll
                for (int d = 0; d < IPH / 4; ++d) o[d] = I[d];
                o[IPH / 4] = U0;
                o[IPH / 4 + 1] = U1;
            }
            if (raw_out) raw_out[fr] = (uint16_t)raw;
        }
    }
}

// ---- receive verify ----
template <bool V6>
__global__ __launch_bounds__(kBlock) void udp_rx_kernel(const uint8_t* __restrict__ base,
                                                        const uint64_t* __restrict__ offsets, uint64_t n,
                                                        uint64_t* __restrict__ mask, uint16_t* __restrict__ ip_raw,
                                                        uint16_t* __restrict__ udp_raw, uint32_t step) {
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t nwords = (n + 63u) / 64u;
    for (uint64_t w = (uint64_t)blockIdx.x * kWavesPerBlock + wave; w < nwords;
         w += (uint64_t)gridDim.x * kWavesPerBlock) {
        uint64_t bits = 0;  // wave-uniform: the mask word
        const uint32_t wcnt = (uint32_t)min((uint64_t)64u, n - w * 64u);
        for (uint32_t s0 = 0; s0 < wcnt; s0 += step) {
            const uint32_t cnt = min(step, wcnt - s0);
            const uint64_t f0 = w * 64u + s0;
            // ---- per-lane metadata of frame f0 + lane ----
            const bool live = lane < cnt;
            const uint64_t fr = f0 + min(lane, cnt - 1u);
            const uint64_t o0 = offsets[fr], o1 = offsets[fr + 1];
            // a frame longer than any length field can say is not well-formed
            const uint32_t flen = o1 > o0 ? (uint32_t)min(o1 - o0, (uint64_t)0x20000u) : 0u;
            const FrameWin F = frame_win(base + o0, flen);
            const uint32_t h0 = F.at(0), h1 = F.at(4);
            uint32_t iph, ipr = 0, part = 0;
            bool wf;
            if constexpr (V6) {
                iph = 40u;
                wf = flen >= 48u && (h0 & 0xF0u) == 0x60u && 40u + bswap16u(h1) == flen && ((h1 >> 16) & 0xFFu) == 17u;
#pragma unroll
                for (uint32_t d = 0; d < 8u; ++d) part += be_words(F.at(8u + 4u * d));
            } else {
                const uint32_t h2 = F.at(8);
                iph = (h0 & 15u) * 4u;
                const bool hdr = flen >= 20u && iph >= 20u && iph <= flen;
                wf = hdr && (h0 & 0xF0u) == 0x40u && bswap16u(h0 >> 16) == flen && (h1 & 0xFF3F0000u) == 0u &&
                     ((h2 >> 8) & 0xFFu) == 17u && flen - iph >= 8u;
                const uint32_t ad = be_words(F.at(12)) + be_words(F.at(16));
                part = ad;
                if (hdr) {  // the raw sum over the IHL*4 header bytes
                    uint32_t hs = be_words(h0) + be_words(h1) + be_words(h2) + ad;
                    for (uint32_t b = 20u; b < iph; b += 4u) hs += be_words(F.at(b));
                    ipr = fold32(hs);
                }
            }
            uint32_t U = 0, field = 0;
            if (wf) {  // the UDP header is the frame's own: iph + 8 <= flen
                const uint32_t u1 = F.at(iph + 4u);
                U = bswap16u(u1);
                field = u1 >> 16;
                wf = U >= 8u && U <= flen - iph;
            }
            wf = wf && live;
            // ---- small datagrams: each lane sums its own through the frame's window ----
            uint32_t psum = 0;  // the datagram's sum, folded, in the BE domain: the lane's own, or parked by the wave
            const bool mine = wf && U <= kLaneMax;
            if (mine) {
                const uint32_t wb = F.sh + iph, we = wb + U;  // the datagram's window bytes: all the frame's own
                uint32_t k = wb >> 2, acc = 0;
                const uint32_t kend = (we + 3u) >> 2;
                acc = __builtin_amdgcn_sad_u16(F.w[k] & keep_mask((int32_t)wb, (int32_t)we, (int32_t)(4u * k)), 0u, acc);
                for (++k; k + 4u < kend; k += 4u) acc = sad4(*reinterpret_cast<const u32x4*>(F.w + k), acc);
                for (; k < kend; ++k)
                    acc = __builtin_amdgcn_sad_u16(F.w[k] & keep_mask((int32_t)wb, (int32_t)we, (int32_t)(4u * k)), 0u, acc);
                psum = fold32(acc);
                if ((wb & 1u) == 0u) psum = bswap16u(psum);  // the datagram starts at an even address
            }
            const uint32_t mU = wf && !mine ? U : 0u;  // what is left to the wave
            part += 17u + U;
            const uint64_t mp = o0 + iph;  // the datagram's start in the batch
            // ---- the wave sums the first U bytes of the other well-formed datagrams ----
            auto rs_of = [&](uint32_t k, uint32_t& sh) {
                return own_dwords(base + readlane64(mp, k), __builtin_amdgcn_readlane(mU, k), true, sh);
            };
            auto fetch = [&](uint32_t k, Rows& R) {
                uint32_t sh;
                const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
                load_rows(rs, 0, lane, false, R);
            };
            auto sum = [&](uint32_t k, Rows& R) {
                const uint32_t len = __builtin_amdgcn_readlane(mU, k);
                uint32_t sh;
                const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
                const uint32_t end = sh + len, rows = (end + kRow - 1u) / kRow;  // window bytes [sh, end)
                uint32_t acc = 0;
                for (uint32_t r0 = 0; r0 < rows; r0 += kPre) {
                    if (r0) load_rows(rs, r0, lane, false, R);
#pragma unroll
                    for (uint32_t r = 0; r < kPre; ++r) {
                        const int32_t pos = (int32_t)((r0 + r) * kRow + lane * 16u);
                        u32x4 x = R.lo[r];
                        if (r0 + r == 0u || (r0 + r + 1u) * kRow > end)  // the rows with the window's edges
                            x = keep_bytes(x, min(max((int32_t)sh - pos, 0), 16), min(max((int32_t)end - pos, 0), 16));
                        acc = sad4(x, acc);
                    }
                    acc = fold32(acc);
                }
                uint32_t s = fold32(wave_sum(acc));
                if ((sh & 1u) == 0u) s = bswap16u(s);  // the datagram starts at an even address
                psum = lane == k ? s : psum;
            };
            uint64_t todo = __ballot(mU != 0u);  // wf holds only in live lanes
            if (todo) {
                Rows A, B;
                uint32_t k = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1u;
                fetch(k, A);
                for (;;) {
                    const uint32_t k2 = todo ? (uint32_t)__builtin_ctzll(todo) : kWave;
                    todo &= todo - 1u;
                    if (k2 < kWave) fetch(k2, B);
                    sum(k, A);
                    if (k2 == kWave) break;
                    k = todo ? (uint32_t)__builtin_ctzll(todo) : kWave;
                    todo &= todo - 1u;
                    if (k < kWave) fetch(k, A);
                    sum(k2, B);
                    if (k == kWave) break;
                }
            }
            // ---- verdicts ----
            const uint32_t raw = wf ? fold32(psum + part) : 0u;
            bool ok = wf && (raw == 0xFFFFu || (!V6 && field == 0u));
            if constexpr (V6) ok = ok && field != 0u;  // RFC 8200 §8.1: no zero checksum over IPv6
            else ok = ok && ipr == 0xFFFFu;
            bits |= __ballot(ok) << s0;
            if (live) {
                if (!V6 && ip_raw) ip_raw[fr] = (uint16_t)ipr;
                if (udp_raw) udp_raw[fr] = (uint16_t)raw;
            }
        }
        if (lane == 0) mask[w] = bits;
    }
}

uint32_t grid_of(const LaunchCfg& c, uint64_t wave_tasks, int default_bpc) {
    const int bpc = (c.blocks_per_cu >= 1 && c.blocks_per_cu <= 8) ? c.blocks_per_cu : default_bpc;
    const uint64_t want = (wave_tasks + kWavesPerBlock - 1) / kWavesPerBlock, most = (uint64_t)c.cus * bpc;
    return (uint32_t)std::max<uint64_t>(1, std::min(want, most));
}

// Frames per transmit wave task: about this many bytes, 16 at the most. Measured on 1M frames (IPv4, 4 blocks/CU):
// 1500 B frames 0.617 ms in groups of 4 against 0.653 / 0.678 / 0.707 / 0.732 for 8 / 16 / 32 / 64; 80 B frames 0.096 ms
// in groups of 16 against 0.304 / 0.161 / 0.114 / 0.195 for 4 / 8 / 32 / 64.
constexpr uint64_t kGroupBytes = 6144;

}  // namespace

hipError_t launch_udp_build(const LaunchCfg& c, int ipver, const IpHdrSoA& ip, const uint16_t* src_port,
                            const uint16_t* dst_port, const UdpUsoMap* uso, uint64_t n_super, const uint8_t* data,
                            const uint64_t* data_off, uint64_t data_bytes, uint64_t n_frames, uint32_t no_csum,
                            uint8_t* out, const uint64_t* out_off, uint16_t* raw, hipStream_t st) {
    if (!n_frames) return hipSuccess;
    // the group as the TCP transmit pass sizes it — up to 16 frames per wave task, fewer for long frames and for
    // batches that would leave waves idle — but at 4 blocks/CU: the kernels hold no more than 68 VGPRs, and the
    // wave's serial part per frame (the reduction, the descriptor set-up) hides behind the other waves' loads
    // (1500 B frames: 0.706 ms at 2 blocks/CU, 0.617 at 4, 0.643 at 8)
    const uint64_t waves = (uint64_t)c.cus * ((c.blocks_per_cu >= 1 && c.blocks_per_cu <= 8) ? c.blocks_per_cu : 4) *
                           kWavesPerBlock;
    const uint64_t frame = data_bytes / n_frames + (ipver == 4 ? 28 : 48);
    const uint64_t by_size = std::max<uint64_t>(1, (kGroupBytes + frame / 2) / frame);
    uint32_t group = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(16, by_size),
                                                  std::max<uint64_t>(1, (n_frames + waves - 1) / waves));
    if (c.run_segs >= 1 && c.run_segs <= 64) group = (uint32_t)c.run_segs;
    const uint32_t grid = grid_of(c, (n_frames + group - 1) / group, 4);
    const UdpSoA u{src_port, dst_port};
    const UsoArgs a = uso ? UsoArgs{uso->gso, uso->frame_first, uso->frame_seg, n_super} : UsoArgs{};
#define NSX_UDP_LAUNCH(IPH, USO)                                                                                    \
    hipLaunchKernelGGL((udp_build_kernel<IPH, USO>), dim3(grid), dim3(kBlock), 0, st, ip, u, data, data_off, n_frames, \
                       no_csum, out, out_off, raw, group, a)
    if (ipver == 4 && uso) NSX_UDP_LAUNCH(20, true);
    else if (ipver == 4) NSX_UDP_LAUNCH(20, false);
    else if (uso) NSX_UDP_LAUNCH(40, true);
    else NSX_UDP_LAUNCH(40, false);
#undef NSX_UDP_LAUNCH
    return hipGetLastError();
}

hipError_t launch_udp_rx(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         uint64_t* mask, uint16_t* ip_raw, uint16_t* udp_raw, hipStream_t st) {
    if (!n) return hipSuccess;
    // 8 blocks/CU and 16 frames per metadata step: 1M frames of 1500 B 0.294 ms against 0.337 for 4 blocks/CU and
    // whole-word steps, which 80 B frames prefer (0.035 ms against 0.041) — the bytes are in the long frames
    const uint32_t step = (c.run_segs >= 1 && c.run_segs <= 64) ? (uint32_t)c.run_segs : 16u;
    const uint32_t grid = grid_of(c, (n + 63) / 64, 8);
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    if (ipver == 6)
        hipLaunchKernelGGL(udp_rx_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, mask, nullptr,
                           udp_raw, step);
    else
        hipLaunchKernelGGL(udp_rx_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, mask, ip_raw,
                           udp_raw, step);
    return hipGetLastError();
}

}  // namespace nsx
