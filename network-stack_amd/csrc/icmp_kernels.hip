// icmp_kernels.hip — the gfx950 kernels of the ICMP family (include/nsx_csum.h nsx_icmp_*): error generation
// (nsx_icmp_err_*), its request helpers (nsx_icmp_req_*), the receive verify (nsx_icmp_rx_*) and the in-place echo
// reply (nsx_icmp_echo_reply_*). A kernel file of its own beside the seven others, whose code objects it leaves as
// they are: the shared helpers come from kernel_util.h, the ones that live in one of the other files only (sad4,
// fold32, wave_sum, the rows of udp_kernels.hip, block_excl_scan and store_edge of frag_kernels.hip, store_own of
// nat_kernels.hip) are restated here.
//
// Error generation is a filter, a scan and a fused copy-and-checksum:
//   plan    one lane per frame. The request word first: a zero request loads nothing else. Then the header dwords
//           through FrameWin, the status (NONE / BAD / QUIET, or eligible) and the message length into `meta`; the
//           block reduces (count, bytes) over its `per_block` frames (run_segs) into `sums`.
//   sums    one workgroup: the blocks' sums -> their exclusive prefix; *n_out and, when the cap does not bite, the
//           closing offset.
//   apply   the block scan again over `meta`: an eligible frame's rank and byte offset; rank < max_out is SENT
//           (src_frame, out_off), the others LIMITED; the frame of rank max_out closes out_off.
//   emit    the hot path. A wave takes 16 messages: lane j holds message j's metadata and header dwords, the wave
//           copies the quotes one after another, the next one's rows in flight while this one is summed and stored.
//           A quote is at most 548 / 1232 bytes: one row / one row pair of 16 bytes per lane. The chunks are laid
//           over the DESTINATION: the quote's first hb = -(slot + header) mod 16 bytes go with the header (lane j
//           stores header and head from registers: whole aligned dwords behind a byte / short start), the wave's
//           chunk c is quote bytes [hb + 16c, hb + 16c + 16) at a 16-aligned address, loaded through a descriptor
//           over the frame's own dwords from the one holding quote byte hb to the one holding byte q - 1 — nothing
//           below the frame, nothing past it — and realigned by the (source - destination) shift. The registers
//           that are stored are the registers that are summed (v_sad_u16, one wave reduction per message); the last
//           chunk is masked and stored by dword / short / byte. The sum is parked in lane j, which adds the ICMP
//           header's words (IPv6: and the pseudo-header's) and stores the 28 / 48 header bytes.
// Verify restates udp_rx_kernel: a wave per mask word, a lane per short frame, the wave per long one.
// Echo reply and the request helpers are one lane per frame, as nat_rewrite_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "icmp_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

constexpr uint32_t kStNone = 0, kStSent = 1, kStQuiet = 2, kStBad = 3, kStLimited = 4;  // NSX_ICMP_*
constexpr uint32_t kFragDf = 2;                                                        // NSX_FRAG_DF
constexpr uint32_t kGroup = 16;  // messages per wave task of the emit kernel
constexpr uint32_t kScanBlockDefault = 4096, kScanBlockMin = 16, kScanBlockMax = 65536;
constexpr uint32_t kLenCap = 0x20000u;  // a frame longer than any length field can say is malformed

// ---- restated from csum_kernels.hip / udp_kernels.hip (they live only there) ----
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

// The two big-endian 16-bit words of a little-endian dword, added up.
__device__ __forceinline__ uint32_t be_words(uint32_t w) {
    const uint32_t b = bswap32(w);
    return (b >> 16) + (b & 0xFFFFu);
}

// The descriptor over the aligned dwords that hold bytes [p, p + len) (none for len 0 or a dead frame), and p & 3.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t own_dwords(const uint8_t* p, uint32_t len, bool live, uint32_t& sh) {
    sh = (uint32_t)((uintptr_t)p & 3u);
    return make_rsrc(p - sh, live && len ? (uint64_t)((sh + len + 3u) & ~3u) : 0u);
}

// A frame's length as every pass here takes it: 0 for decreasing offsets, capped where no length field reaches.
__device__ __forceinline__ uint32_t frame_len(uint64_t o0, uint64_t o1) {
    return o1 > o0 ? (uint32_t)min(o1 - o0, (uint64_t)kLenCap) : 0u;
}

// ---- restated from frag_kernels.hip ----
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

// Exclusive scan of two values per thread over the block; total = the block's sums.
__device__ __forceinline__ void block_excl_scan(uint64_t (&v)[2], uint64_t (&total)[2], uint64_t (*lds)[2]) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t incl[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
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
    for (int k = 0; k < 2; ++k) {
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

// ---- restated from nat_kernels.hip ----
// RFC 1624 eqn. 3 as include/nsx_csum.h evaluates it: hc the field (big-endian value), acc the sum over the covered
// words of (~m & 0xFFFF) + m'.
__device__ __forceinline__ uint32_t csum_update(uint32_t hc, uint32_t acc) {
    const uint32_t x = (~hc & 0xFFFFu) + acc;
    const uint32_t fold = x ? 1u + (x - 1u) % 0xFFFFu : 0u;
    return ~fold & 0xFFFFu;
}
// (~m & 0xFFFF) + m' for the one word in the low halves of old and repl.
__device__ __forceinline__ uint32_t delta16(uint32_t old, uint32_t repl) {
    return (~bswap16(old) & 0xFFFFu) + bswap16(repl);
}

// The first nb bytes of the dwords v[0..K) (little-endian) to q[0, nb), q at any alignment, nb <= 4K and at least
// the bytes up to the next 4-byte boundary: those by a byte and / or a 16-bit store, then whole aligned dwords, then
// what is left by a 16-bit and / or a byte store. Every store is naturally aligned and covers bytes of [q, q + nb)
// only. (store_own of nat_kernels.hip with a run-time length: the emit pass's header-and-head run ends 16-aligned and
// has no tail; the echo reply's runs are whole dwords, nb = 4K.)
template <uint32_t K>
__device__ __forceinline__ void store_run(uint8_t* q, const uint32_t (&v)[K], uint32_t nb) {
    const uint32_t a = (uint32_t)((uintptr_t)q & 3u), head = (4u - a) & 3u;
    if (a & 1u) q[0] = (uint8_t)v[0];
    if (head & 2u) *reinterpret_cast<uint16_t*>(q + (a & 1u)) = (uint16_t)(v[0] >> (8u * (a & 1u)));
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t x = __builtin_amdgcn_alignbyte(j + 1 < K ? v[j + 1] : 0u, v[j], head);
        const int32_t left = (int32_t)nb - (int32_t)(head + 4u * j);  // bytes of the run from this aligned address on
        uint8_t* d = q + head + 4u * j;
        if (left >= 4) {
            *reinterpret_cast<uint32_t*>(d) = x;
        } else if (left > 0) {
            if (left & 2) *reinterpret_cast<uint16_t*>(d) = (uint16_t)x;
            if (left & 1) d[left & 2] = (uint8_t)(x >> (8 * (left & 2)));
        }
    }
}

// The 4·K bytes v[0..K) to q[0, 4K), all of them the frame's own.
template <uint32_t K>
__device__ __forceinline__ void store_own(uint8_t* q, const uint32_t (&v)[K]) {
    store_run(q, v, 4u * K);
}

// ------------------------------------------------------------------------------------------------ error plan
struct EmitCfg {
    uint32_t src[4];
    uint32_t ttl, ident0;
};

template <bool V6>
struct Msg {
    static constexpr uint32_t kHdr = V6 ? 48u : 28u;     // IP header + ICMP header
    static constexpr uint32_t kQuote = V6 ? 1232u : 548u;  // RFC 4443 §2.4(c): 1280 in all; RFC 1812 §4.3.2.3: 576
    static constexpr uint32_t kMinFrame = V6 ? 40u : 20u;
};

// The status of frame i's request r (nonzero) and, when it is eligible (kStSent here: the cap is applied later), the
// message's length. Reads nothing when the request is not an allowed one.
template <bool V6>
__device__ __forceinline__ uint32_t classify(const uint8_t* __restrict__ base, const uint64_t* __restrict__ offsets,
                                             uint32_t i, uint32_t r, uint32_t& mlen) {
    const uint32_t type = r & 0xFFu, code = (r >> 8) & 0xFFu;
    const bool allowed = V6 ? (type >= 1u && type <= 4u) : (type == 3u || type == 11u || type == 12u);
    mlen = 0;
    if ((r >> 16) || !allowed) return kStBad;
    const uint64_t o0 = offsets[i], o1 = offsets[(uint64_t)i + 1];
    const uint32_t flen = frame_len(o0, o1);
    if (flen < Msg<V6>::kMinFrame) return kStBad;
    const FrameWin F = frame_win(base + o0, flen);
    const uint32_t h0 = F.at(0), h1 = F.at(4);
    bool quiet;
    if constexpr (V6) {
        if ((h0 & 0xF0u) != 0x60u || 40u + bswap16(h1) != flen) return kStBad;
        const uint32_t s0 = F.at(8), s1 = F.at(12), s2 = F.at(16), s3 = F.at(20), d0 = F.at(24);
        // RFC 4443 §2.4(e): no error about an ICMPv6 error or a redirect, (e.3) about a multicast destination but for
        // Packet Too Big and the unrecognised-option Parameter Problem, (e.6) about a source that names no single node
        quiet = (s0 | s1 | s2 | s3) == 0u || (s0 & 0xFFu) == 0xFFu ||
                ((d0 & 0xFFu) == 0xFFu && !(type == 2u || (type == 4u && code == 2u)));
        if (((h1 >> 16) & 0xFFu) == 58u) {
            const uint32_t t = F.at(40) & 0xFFu;  // reads 0 when the frame ends at byte 40
            quiet = quiet || flen <= 40u || t < 128u || t == 137u;
        }
    } else {
        const uint32_t iph = (h0 & 15u) * 4u;
        if ((h0 & 0xF0u) != 0x40u || iph < 20u || iph > flen || bswap16(h0 >> 16) != flen) return kStBad;
        const uint32_t h2 = F.at(8), src = F.at(12), dst = F.at(16);
        // RFC 1122 §3.2.2 / RFC 1812 §4.3.2.7: no error about a non-initial fragment, a source that names no single
        // host, a multicast / class E destination, or an ICMP error
        quiet = (h1 & 0xFF1F0000u) != 0u || src == 0u || (src & 0xFFu) >= 224u || (dst & 0xFFu) >= 224u;
        if (((h2 >> 8) & 0xFFu) == 1u) {
            const uint32_t t = F.at(iph) & 0xFFu;
            constexpr uint32_t kQuery = 0x0007E701u;  // types 0, 8, 9, 10, 13-18
            quiet = quiet || iph >= flen || t >= 32u || !((kQuery >> t) & 1u);
        }
    }
    if (quiet) return kStQuiet;
    mlen = Msg<V6>::kHdr + min(flen, Msg<V6>::kQuote);
    return kStSent;
}

template <bool V6>
__global__ __launch_bounds__(kBlock) void icmp_plan_kernel(const uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           const uint32_t* __restrict__ req, uint32_t per_block,
                                                           uint32_t* __restrict__ meta, uint64_t* __restrict__ sums,
                                                           uint8_t* __restrict__ status) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(lo + per_block, (uint64_t)n);
    uint64_t carry[2] = {0, 0};
    for (uint64_t t = lo; t < hi; t += kBlock) {  // block-uniform trip count
        const uint64_t fi = t + threadIdx.x;
        uint32_t mlen = 0;
        if (fi < hi) {
            const uint32_t i = (uint32_t)fi, r = req[i];
            const uint32_t st = r ? classify<V6>(base, offsets, i, r, mlen) : kStNone;
            if (!mlen) status[i] = (uint8_t)st;  // an eligible frame's status is the apply pass's
            meta[i] = mlen;
        }
        uint64_t v[2] = {mlen != 0u, mlen}, tot[2];
        block_excl_scan(v, tot, lds);
        carry[0] += tot[0];
        carry[1] += tot[1];
    }
    if (threadIdx.x == 0) {
        sums[2u * blockIdx.x] = carry[0];
        sums[2u * blockIdx.x + 1u] = carry[1];
    }
}

// One workgroup: sums (nb pairs) -> their exclusive prefix in place; the totals close the outputs.
__global__ __launch_bounds__(kBlock) void icmp_scan_sums_kernel(uint64_t* __restrict__ sums, uint32_t nb,
                                                                uint64_t max_out, uint64_t* __restrict__ n_out,
                                                                uint64_t* __restrict__ out_off) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    uint64_t carry[2] = {0, 0};
    for (uint32_t t = 0; t < nb; t += kBlock) {
        const uint32_t b = t + threadIdx.x;
        const bool live = b < nb;
        uint64_t v[2], tot[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = live ? sums[2u * b + k] : 0u;
        block_excl_scan(v, tot, lds);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (live) sums[2u * b + k] = carry[k] + v[k];
            carry[k] += tot[k];
        }
    }
    if (threadIdx.x == 0) {
        *n_out = min(carry[0], max_out);
        // under the cap every eligible frame is sent and the bytes' total closes the offsets (none: entry 0); else
        // the frame of rank max_out does (icmp_apply_kernel)
        if (carry[0] <= max_out) out_off[carry[0]] = carry[1];
    }
}

__global__ __launch_bounds__(kBlock) void icmp_apply_kernel(uint32_t n, uint32_t per_block,
                                                            const uint32_t* __restrict__ meta,
                                                            const uint64_t* __restrict__ sums, uint64_t max_out,
                                                            uint8_t* __restrict__ status,
                                                            uint32_t* __restrict__ src_frame,
                                                            uint64_t* __restrict__ out_off) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(lo + per_block, (uint64_t)n);
    uint64_t carry[2] = {sums[2u * blockIdx.x], sums[2u * blockIdx.x + 1u]};
    for (uint64_t t = lo; t < hi; t += kBlock) {  // block-uniform trip count
        const uint64_t fi = t + threadIdx.x;
        const uint32_t mlen = fi < hi ? meta[(uint32_t)fi] : 0u;
        uint64_t v[2] = {mlen != 0u, mlen}, tot[2];
        block_excl_scan(v, tot, lds);
        if (mlen) {
            const uint64_t rank = carry[0] + v[0], at = carry[1] + v[1];
            if (rank < max_out) {
                status[fi] = (uint8_t)kStSent;
                src_frame[rank] = (uint32_t)fi;
                out_off[rank] = at;
            } else {
                status[fi] = (uint8_t)kStLimited;
                if (rank == max_out) out_off[rank] = at;  // the end of message max_out - 1
            }
        }
        carry[0] += tot[0];
        carry[1] += tot[1];
    }
}

// ------------------------------------------------------------------------------------------------ error emit
template <uint32_t NR>
struct QRows {
    u32x4 lo[NR];
    uint32_t hi[NR];
};

template <bool V6>
__global__ __launch_bounds__(kBlock) void icmp_emit_kernel(const uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           const uint32_t* __restrict__ req,
                                                           const uint32_t* __restrict__ arg, EmitCfg cfg,
                                                           const uint64_t* __restrict__ n_out_p, uint8_t* out,
                                                           const uint64_t* __restrict__ out_off,
                                                           const uint32_t* __restrict__ src_frame) {
    constexpr uint32_t H = Msg<V6>::kHdr, Q = Msg<V6>::kQuote;
    constexpr uint32_t NR = V6 ? 2u : 1u;  // 1 KiB rows that hold the longest quote
    constexpr uint32_t KH = H / 4u;        // header dwords
    static_assert(NR * kRow >= Q, "a quote fits the rows");
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const uint64_t n_out = min(*n_out_p, (uint64_t)n);
    const uint64_t ngroups = (n_out + kGroup - 1) / kGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWavesPerBlock + wave; g < ngroups;
         g += (uint64_t)gridDim.x * kWavesPerBlock) {
        const uint64_t s0 = g * kGroup;
        const uint32_t cnt = (uint32_t)min((uint64_t)kGroup, n_out - s0);
        // ---- per-lane metadata of message s0 + lane (lanes past cnt repeat the last one and store nothing) ----
        const uint64_t s = s0 + min(lane, cnt - 1u);
        const uint32_t f = min(src_frame[s], n - 1u);
        const uint64_t o0 = offsets[f], moo = out_off[s];
        const uint32_t flen = frame_len(o0, offsets[(uint64_t)f + 1]);
        const uint32_t q = min(flen, Q);
        // a message the plan pass made quotes a whole IP header; anything else is not built
        const bool mine = lane < cnt && flen >= Msg<V6>::kMinFrame;
        uint8_t* D = out + moo;
        const uint32_t hb = (16u - (uint32_t)((uintptr_t)(D + H) & 15u)) & 15u;  // quote bytes that go with the header
        const uint32_t mq = mine ? q : 0u;                                         // hb < 16 <= kMinFrame <= q
        // ---- the wave copies and sums quote bytes [hb, q) of one message after another ----
        auto rs_of = [&](uint32_t k, uint32_t& r) {
            const uint8_t* sp = base + readlane64(o0, k);
            const uint32_t sh = (uint32_t)((uintptr_t)sp & 3u), w0 = sh + __builtin_amdgcn_readlane(hb, k);
            r = w0 & 3u;
            // from the dword holding quote byte hb to the one holding byte q - 1: the frame's own
            return make_rsrc(sp - sh + (w0 & ~3u),
                             (uint64_t)(((sh + __builtin_amdgcn_readlane(mq, k) + 3u) & ~3u) - (w0 & ~3u)));
        };
        auto fetch = [&](uint32_t k, QRows<NR>& R) {
            uint32_t r;
            const __amdgpu_buffer_rsrc_t rs = rs_of(k, r);
#pragma unroll
            for (uint32_t j = 0; j < NR; ++j) {
                const uint32_t at = j * kRow + lane * 16u;
                R.lo[j] = bld16<true>(rs, at);
                R.hi[j] = __builtin_amdgcn_raw_buffer_load_b32(rs, r ? at + 16u : kOOB, 0, 2);
            }
        };
        uint32_t psum = 0;  // the message's sum over quote bytes [hb, q), folded, in the BE domain: parked in lane k
        auto build = [&](uint32_t k, const QRows<NR>& R) {
            uint32_t r;
            (void)rs_of(k, r);
            const uint32_t hbk = __builtin_amdgcn_readlane(hb, k);
            const int32_t left = (int32_t)(__builtin_amdgcn_readlane(mq, k) - hbk);  // bytes the wave copies
            uint8_t* q1 = out + readlane64(moo, k) + H + hbk;                        // 16-aligned
            uint32_t acc = 0;
#pragma unroll
            for (uint32_t j = 0; j < NR; ++j) {
                const uint32_t pos = j * kRow + lane * 16u;
                const int32_t rem = left - (int32_t)pos;
                u32x4 x = r ? realign(R.lo[j], R.hi[j], r) : R.lo[j];
                if (rem >= 16) {
                    *reinterpret_cast<a16x4*>(q1 + pos) = a16x4{x.x, x.y, x.z, x.w};
                } else {  // the chunk holding the quote's end, and every chunk past it
                    x = keep_bytes(x, 0, max(rem, 0));
                    if (rem > 0) store_edge(q1 + pos, x, 0, rem);
                }
                acc = sad4(x, acc);
            }
            uint32_t t = fold32(wave_sum(acc));
            if ((hbk & 1u) == 0u) t = bswap16(t);  // the chunks start at an even byte of the quote
            psum = lane == k ? t : psum;
        };
        uint64_t todo = __ballot(mq != 0u);
        if (todo) {
            QRows<NR> A, B;
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
        // ---- each lane finishes its own message: the head of the quote, both checksums, the header ----
        if (mine) {
            const FrameWin F = frame_win(base + o0, q);
            const uint32_t r = req[f] & 0xFFFFu, a = arg ? arg[f] : 0u;
            uint32_t v[KH + 4u];
            uint32_t sum = psum;
#pragma unroll
            for (uint32_t d = 0; d < 4u; ++d) {
                v[KH + d] = F.at(4u * d);
                sum += be_words(v[KH + d] & keep_mask(0, (int32_t)hb, (int32_t)(4u * d)));
            }
            v[KH - 2u] = r;  // type, code, checksum 0
            v[KH - 1u] = bswap32(a);
            sum += be_words(r) + be_words(v[KH - 1u]);
            if constexpr (V6) {
                v[0] = 0x60u;
                v[1] = bswap16(8u + q) | (58u << 16) | (cfg.ttl << 24);
#pragma unroll
                for (uint32_t d = 0; d < 4u; ++d) {
                    v[2u + d] = cfg.src[d];
                    v[6u + d] = F.at(8u + 4u * d);
                    sum += be_words(v[2u + d]) + be_words(v[6u + d]);
                }
                sum += 8u + q + 58u;  // RFC 8200 §8.1: the upper-layer length and the next header
            } else {
                v[0] = 0xC045u | (bswap16(28u + q) << 16);
                v[1] = bswap16((cfg.ident0 + (uint32_t)s) & 0xFFFFu);
                v[2] = cfg.ttl | (1u << 8);
                v[3] = cfg.src[0];
                v[4] = v[KH + 3u];  // the offending frame's src
                const uint32_t hs = be_words(v[0]) + be_words(v[1]) + be_words(v[2]) + be_words(v[3]) + be_words(v[4]);
                v[2] |= bswap16(~fold32(hs) & 0xFFFFu) << 16;  // RFC 791 §3.1
            }
            v[KH - 2u] |= bswap16(~fold32(sum) & 0xFFFFu) << 16;
            store_run(D, v, H + hb);
        }
    }
}

// ------------------------------------------------------------------------------------------------ request helpers
__global__ __launch_bounds__(kBlock) void icmp_req_frag_kernel(const uint8_t* __restrict__ status,
                                                               const uint32_t* __restrict__ mtu, uint32_t n,
                                                               uint32_t* __restrict__ req, uint32_t* __restrict__ arg) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n || status[gi] != kFragDf) return;
    req[gi] = 3u | (4u << 8);  // destination unreachable, fragmentation needed and DF set (RFC 1191)
    arg[gi] = mtu[gi] & 0xFFFFu;
}

template <bool V6>
__global__ __launch_bounds__(kBlock) void icmp_req_ttl_kernel(const uint8_t* __restrict__ base,
                                                              const uint64_t* __restrict__ offsets, uint32_t n,
                                                              const uint64_t* __restrict__ valid, uint32_t ttl_dec,
                                                              uint32_t* __restrict__ req, uint32_t* __restrict__ arg) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n) return;
    const uint32_t i = (uint32_t)gi;
    if (!((valid[i >> 6] >> (i & 63u)) & 1u)) return;  // a frame the mask rejects is not read at all
    const uint64_t o0 = offsets[i];
    const uint32_t flen = frame_len(o0, offsets[(uint64_t)i + 1]);
    if (flen < Msg<V6>::kMinFrame) return;
    const FrameWin F = frame_win(base + o0, flen);
    const uint32_t h0 = F.at(0);
    uint32_t t;
    if constexpr (V6) {
        if ((h0 & 0xF0u) != 0x60u) return;
        t = F.at(4) >> 24;
    } else {
        const uint32_t iph = (h0 & 15u) * 4u;
        if ((h0 & 0xF0u) != 0x40u || iph < 20u || iph > flen) return;
        t = F.at(8) & 0xFFu;
    }
    if (t > ttl_dec) return;
    req[i] = V6 ? 3u : 11u;  // time exceeded, code 0: hop limit / TTL exceeded in transit
    arg[i] = 0u;
}

// ------------------------------------------------------------------------------------------------ receive verify
constexpr uint32_t kPre = 2;  // rows of the next frame in flight while this one is summed
// Messages of at most this many bytes are summed by the lane that holds the frame's metadata (udp_kernels.hip).
constexpr uint32_t kLaneMax = 256;

struct Rows {
    u32x4 lo[kPre];
};

__device__ __forceinline__ void load_rows(__amdgpu_buffer_rsrc_t rs, uint32_t r0, uint32_t lane, Rows& R) {
#pragma unroll
    for (uint32_t r = 0; r < kPre; ++r) R.lo[r] = bld16<false>(rs, (r0 + r) * kRow + lane * 16u);
}

template <bool V6>
__global__ __launch_bounds__(kBlock) void icmp_rx_kernel(const uint8_t* __restrict__ base,
                                                         const uint64_t* __restrict__ offsets, uint64_t n,
                                                         uint64_t* __restrict__ mask, uint16_t* __restrict__ ip_raw,
                                                         uint16_t* __restrict__ icmp_raw, uint16_t* __restrict__ type,
                                                         uint32_t step) {
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
            const uint32_t flen = frame_len(o0, o1);
            const FrameWin F = frame_win(base + o0, flen);
            const uint32_t h0 = F.at(0), h1 = F.at(4);
            uint32_t iph, ipr = 0, part = 0;
            bool wf;
            if constexpr (V6) {
                iph = 40u;
                wf = flen >= 48u && (h0 & 0xF0u) == 0x60u && 40u + bswap16(h1) == flen && ((h1 >> 16) & 0xFFu) == 58u;
#pragma unroll
                for (uint32_t d = 0; d < 8u; ++d) part += be_words(F.at(8u + 4u * d));
                part += flen - 40u + 58u;  // RFC 8200 §8.1: the upper-layer length and the next header
            } else {
                const uint32_t h2 = F.at(8);
                iph = (h0 & 15u) * 4u;
                const bool hdr = flen >= 20u && iph >= 20u && iph <= flen;
                wf = hdr && (h0 & 0xF0u) == 0x40u && bswap16(h0 >> 16) == flen && (h1 & 0xFF3F0000u) == 0u &&
                     ((h2 >> 8) & 0xFFu) == 1u && flen - iph >= 8u;
                if (hdr) {  // the raw sum over the IHL*4 header bytes
                    uint32_t hs = be_words(h0) + be_words(h1) + be_words(h2) + be_words(F.at(12)) + be_words(F.at(16));
                    for (uint32_t b = 20u; b < iph; b += 4u) hs += be_words(F.at(b));
                    ipr = fold32(hs);
                }
            }
            wf = wf && live;
            const uint32_t U = wf ? flen - iph : 0u;            // the ICMP message: the frame's own, 8 bytes or more
            const uint32_t tc = wf ? bswap16(F.at(iph)) : 0u;  // type << 8 | code
            // ---- short messages: each lane sums its own through the frame's window ----
            uint32_t psum = 0;  // the message's sum, folded, in the BE domain: the lane's own, or parked by the wave
            const bool mine = wf && U <= kLaneMax;
            if (mine) {
                const uint32_t wb = F.sh + iph, we = wb + U;  // the message's window bytes: all the frame's own
                uint32_t k = wb >> 2, acc = 0;
                const uint32_t kend = (we + 3u) >> 2;
                acc = __builtin_amdgcn_sad_u16(F.w[k] & keep_mask((int32_t)wb, (int32_t)we, (int32_t)(4u * k)), 0u, acc);
                for (++k; k + 4u < kend; k += 4u) acc = sad4(*reinterpret_cast<const u32x4*>(F.w + k), acc);
                for (; k < kend; ++k)
                    acc = __builtin_amdgcn_sad_u16(F.w[k] & keep_mask((int32_t)wb, (int32_t)we, (int32_t)(4u * k)), 0u, acc);
                psum = fold32(acc);
                if ((wb & 1u) == 0u) psum = bswap16(psum);  // the message starts at an even address
            }
            const uint32_t mU = wf && !mine ? U : 0u;  // what is left to the wave
            const uint64_t mp = o0 + iph;              // the message's start in the batch
            // ---- the wave sums the other well-formed messages ----
            auto rs_of = [&](uint32_t k, uint32_t& sh) {
                return own_dwords(base + readlane64(mp, k), __builtin_amdgcn_readlane(mU, k), true, sh);
            };
            auto fetch = [&](uint32_t k, Rows& R) {
                uint32_t sh;
                const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
                load_rows(rs, 0, lane, R);
            };
            auto sum = [&](uint32_t k, Rows& R) {
                const uint32_t len = __builtin_amdgcn_readlane(mU, k);
                uint32_t sh;
                const __amdgpu_buffer_rsrc_t rs = rs_of(k, sh);
                const uint32_t end = sh + len, rows = (end + kRow - 1u) / kRow;  // window bytes [sh, end)
                uint32_t acc = 0;
                for (uint32_t r0 = 0; r0 < rows; r0 += kPre) {
                    if (r0) load_rows(rs, r0, lane, R);
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
                uint32_t t = fold32(wave_sum(acc));
                if ((sh & 1u) == 0u) t = bswap16(t);  // the message starts at an even address
                psum = lane == k ? t : psum;
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
            bool ok = wf && raw == 0xFFFFu;
            if constexpr (!V6) ok = ok && ipr == 0xFFFFu;
            bits |= __ballot(ok) << s0;
            if (live) {
                if (!V6 && ip_raw) ip_raw[fr] = (uint16_t)ipr;
                if (icmp_raw) icmp_raw[fr] = (uint16_t)raw;
                if (type) type[fr] = (uint16_t)(ok ? tc : 0xFFFFu);
            }
        }
        if (lane == 0) mask[w] = bits;
    }
}

// ------------------------------------------------------------------------------------------------ echo reply
template <bool V6>
__global__ __launch_bounds__(kBlock) void icmp_echo_kernel(uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           const uint64_t* __restrict__ valid, uint32_t ttl,
                                                           uint64_t* __restrict__ hit_mask) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = gi < n;
    const uint32_t i = (uint32_t)gi;
    bool hit = false;
    if (live && ((valid[i >> 6] >> (i & 63u)) & 1u)) {  // a frame the mask rejects is not read at all
        const uint64_t o0 = offsets[i];
        const uint32_t flen = frame_len(o0, offsets[(uint64_t)i + 1]);
        uint8_t* p = base + o0;
        const FrameWin F = frame_win(p, flen);
        const uint32_t h0 = F.at(0), h1 = F.at(4);
        // well-formed: iph + 8 <= flen, so every byte read or written below is the frame's own:
        // IPv4 [8, 20) and [iph, iph + 4), IPv6 [4, 44)
        if constexpr (V6) {
            const bool wf = flen >= 48u && (h0 & 0xF0u) == 0x60u && 40u + bswap16(h1) == flen &&
                            ((h1 >> 16) & 0xFFu) == 58u;
            const uint32_t t0 = F.at(40), d0 = F.at(24);
            if (wf && (t0 & 0xFFFFu) == 128u && (d0 & 0xFFu) != 0xFFu) {  // echo request, code 0, to a unicast address
                hit = true;
                uint32_t v[9];  // bytes 4-39: payload length, next header, hop limit; dst, src
                v[0] = (h1 & 0x00FFFFFFu) | (ttl << 24);
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    v[1u + k] = F.at(24u + 4u * k);
                    v[5u + k] = F.at(8u + 4u * k);
                }
                // the swap leaves the pseudo-header's sum as it was: the update is over ICMPv6 word 0 alone
                const uint32_t w0 = (t0 & 0xFF00u) | 129u;
                const uint32_t c = csum_update(bswap16(t0 >> 16), delta16(t0, w0));
                const uint32_t icmp[1] = {w0 | (bswap16(c) << 16)};
                store_own(p + 4, v);
                store_own(p + 40, icmp);
            }
        } else {
            const uint32_t h2 = F.at(8), iph = (h0 & 15u) * 4u;
            const bool wf = flen >= 20u && iph >= 20u && iph <= flen && (h0 & 0xF0u) == 0x40u &&
                            bswap16(h0 >> 16) == flen && (h1 & 0xFF3F0000u) == 0u && ((h2 >> 8) & 0xFFu) == 1u &&
                            flen - iph >= 8u;
            const uint32_t t0 = wf ? F.at(iph) : 0xFFu, src = F.at(12), dst = F.at(16);
            if (wf && (t0 & 0xFFFFu) == 8u && (dst & 0xFFu) < 224u) {  // echo request, code 0, to a unicast address
                hit = true;
                // bytes 8-11: TTL, protocol, header checksum — over the word at bytes 8-9 alone: the swap leaves the
                // address words' sum as it was
                const uint32_t w89 = (h2 & 0xFF00u) | ttl;
                const uint32_t hc = csum_update(bswap16(h2 >> 16), delta16(h2, w89));
                const uint32_t v[3] = {w89 | (bswap16(hc) << 16), dst, src};
                const uint32_t w0 = t0 & 0xFF00u;  // type 0
                const uint32_t c = csum_update(bswap16(t0 >> 16), delta16(t0, w0));
                const uint32_t icmp[1] = {w0 | (bswap16(c) << 16)};
                store_own(p + 8, v);
                store_own(p + iph, icmp);
            }
        }
    }
    const uint64_t word = __ballot(hit);  // lanes past n vote 0: bits past n stay clear
    if (live && (threadIdx.x & 63u) == 0u) hit_mask[i >> 6] = word;
}

uint32_t scan_block_frames(const LaunchCfg& c) {
    if (c.run_segs <= 0) return kScanBlockDefault;
    return std::min<uint32_t>(std::max<uint32_t>((uint32_t)c.run_segs, kScanBlockMin), kScanBlockMax);
}

uint32_t grid_of(const LaunchCfg& c, uint64_t wave_tasks, int default_bpc) {
    const int bpc = (c.blocks_per_cu >= 1 && c.blocks_per_cu <= 8) ? c.blocks_per_cu : default_bpc;
    const uint64_t want = (wave_tasks + kWavesPerBlock - 1) / kWavesPerBlock, most = (uint64_t)std::max(c.cus, 1) * bpc;
    return (uint32_t)std::max<uint64_t>(1, std::min(want, most));
}

uint32_t lane_grid(uint32_t n) { return (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock); }

}  // namespace

// sums: a pair per scan block, for the smallest scan block a tune can ask for; meta: a dword per frame; + the rounding
// of the caller's pointer
uint64_t icmp_err_work_bytes(uint64_t n) { return 16 * ((n + kScanBlockMin - 1) / kScanBlockMin + 1) + 4 * n + 8; }

hipError_t launch_icmp_err(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n64,
                           const uint32_t* req, const uint32_t* arg, const IcmpErrCfg& cfg, const IcmpErrOut& o,
                           void* work, hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (icmp_api.cpp)
    uint8_t* wb = reinterpret_cast<uint8_t*>(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    uint64_t* sums = reinterpret_cast<uint64_t*>(wb);
    uint32_t* meta = reinterpret_cast<uint32_t*>(wb + 16 * (((uint64_t)n + kScanBlockMin - 1) / kScanBlockMin + 1));
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    const uint32_t per = scan_block_frames(c);
    const uint32_t nb = (uint32_t)(((uint64_t)n + per - 1) / per);
    const bool v6 = ipver == 6;
    if (n) {
        if (v6)
            hipLaunchKernelGGL(icmp_plan_kernel<true>, dim3(nb), dim3(kBlock), 0, st, base, d_offsets, n, req, per, meta,
                               sums, o.status);
        else
            hipLaunchKernelGGL(icmp_plan_kernel<false>, dim3(nb), dim3(kBlock), 0, st, base, d_offsets, n, req, per,
                               meta, sums, o.status);
    }
    hipLaunchKernelGGL(icmp_scan_sums_kernel, dim3(1), dim3(kBlock), 0, st, sums, nb, cfg.max_out, o.n_out, o.out_off);
    if (n) {
        hipLaunchKernelGGL(icmp_apply_kernel, dim3(nb), dim3(kBlock), 0, st, n, per, meta, sums, cfg.max_out, o.status,
                           o.src_frame, o.out_off);
        const uint64_t most = std::min<uint64_t>(n, cfg.max_out);  // messages, at the most
        if (most) {
            const uint32_t grid = grid_of(c, (most + kGroup - 1) / kGroup, 8);
            const EmitCfg e{{cfg.src[0], cfg.src[1], cfg.src[2], cfg.src[3]}, cfg.ttl, cfg.ident0};
            if (v6)
                hipLaunchKernelGGL(icmp_emit_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, req,
                                   arg, e, o.n_out, o.out, o.out_off, o.src_frame);
            else
                hipLaunchKernelGGL(icmp_emit_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, req,
                                   arg, e, o.n_out, o.out, o.out_off, o.src_frame);
        }
    }
    return hipGetLastError();
}

hipError_t launch_icmp_req_frag(const uint8_t* status, const uint32_t* mtu, uint64_t n, uint32_t* req, uint32_t* arg,
                                hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(icmp_req_frag_kernel, dim3(lane_grid((uint32_t)n)), dim3(kBlock), 0, st, status, mtu,
                       (uint32_t)n, req, arg);
    return hipGetLastError();
}

hipError_t launch_icmp_req_ttl(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                               const uint64_t* valid, uint32_t ttl_dec, uint32_t* req, uint32_t* arg, hipStream_t st) {
    if (!n) return hipSuccess;
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    const uint32_t grid = lane_grid((uint32_t)n);
    if (ipver == 6)
        hipLaunchKernelGGL(icmp_req_ttl_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, (uint32_t)n,
                           valid, ttl_dec, req, arg);
    else
        hipLaunchKernelGGL(icmp_req_ttl_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, (uint32_t)n,
                           valid, ttl_dec, req, arg);
    return hipGetLastError();
}

hipError_t launch_icmp_rx(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                          uint64_t* mask, uint16_t* ip_raw, uint16_t* icmp_raw, uint16_t* type, hipStream_t st) {
    if (!n) return hipSuccess;
    // the shape of launch_udp_rx: 8 blocks/CU and 16 frames per metadata step
    const uint32_t step = (c.run_segs >= 1 && c.run_segs <= 64) ? (uint32_t)c.run_segs : 16u;
    const uint32_t grid = grid_of(c, (n + 63) / 64, 8);
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    if (ipver == 6)
        hipLaunchKernelGGL(icmp_rx_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, mask, nullptr,
                           icmp_raw, type, step);
    else
        hipLaunchKernelGGL(icmp_rx_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, mask, ip_raw,
                           icmp_raw, type, step);
    return hipGetLastError();
}

hipError_t launch_icmp_echo(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* valid,
                            uint32_t ttl, uint64_t* d_hit, hipStream_t st) {
    if (!n) return hipSuccess;
    uint8_t* base = static_cast<uint8_t*>(d_base);
    const uint32_t grid = lane_grid((uint32_t)n);
    if (ipver == 6)
        hipLaunchKernelGGL(icmp_echo_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, (uint32_t)n, valid,
                           ttl, d_hit);
    else
        hipLaunchKernelGGL(icmp_echo_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, (uint32_t)n,
                           valid, ttl, d_hit);
    return hipGetLastError();
}

}  // namespace nsx
