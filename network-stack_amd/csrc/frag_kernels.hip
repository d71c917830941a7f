// frag_kernels.hip — gfx950 kernels of IPv4 fragmentation (nsx_frag_ipv4_dev) and reassembly (nsx_reasm_ipv4_dev,
// include/nsx_csum.h). Both passes are copies with a header fix-up: the copy is that of the coalescing emit kernels
// (ugro_kernels.hip) — 16-byte loads through a descriptor clamped to the frame, realigned by the (source −
// destination) byte shift, 16-byte stores at destination-aligned addresses, byte / short / dword stores at the two
// ends — and the 20 header bytes of a fragment or a datagram are written by one lane from registers.
//
// Fragmentation, one launch: a wave takes 16 consecutive output slots. The lane that owns a slot reads its frame's
// offsets, mtu and header dwords, decides the frame's status (every slot of a frame reaches the same verdict), writes
// the slot's header bytes, and hands the wave one copy job: the piece of payload behind the header, or zeros.
//
// Reassembly, one serial chain of launches, none of which waits on another workgroup:
//   key     per frame: the member test, the fragment offset as the first sort key, the FNV-1a datagram key, is_frag.
//   sort    launch_flow_sort (gro_flow_kernels.hip) by offset, a regather of the datagram keys through that order,
//           and launch_flow_sort again: the order numpy.lexsort((arrival, offset, key)) gives.
//   head    per position: the frame's meta dword with cont(p). A wave owns 63 positions plus the one before them.
//   runs    reduce / scan / apply over !cont(p): every position's run number, every run's first position.
//   done    reduce / scan / apply over the runs' last positions: a run is complete iff its first frame has offset 0
//           and its last has MF clear; n_out, out_off, first_pos, frag_cnt, and per run its datagram and offset.
//   emit    a wave takes 16 positions: frame_seg, the payload copies (each fragment knows its destination), and at a
//           run's first position the datagram's header.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csum_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

constexpr uint32_t kGroup = 16;        // slots / positions per wave task of the copy kernels
constexpr uint32_t kHeadFrames = 63;   // positions per wave of the head pass (lane 0 holds the one before them)
constexpr uint32_t kScanBlockDefault = 4096, kScanBlockMin = 16, kScanBlockMax = 65536;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint64_t kLenCap = 1ull << 30;  // a frame or a slot this long is never copied (include/nsx_csum.h)
constexpr uint32_t kStPass = 0, kStCut = 1, kStDf = 2, kStBad = 3;

// RFC 1624's fold as the NAT comment of include/nsx_csum.h defines it: 0 for 0, else 1 + (x - 1) mod 0xFFFF
__device__ __forceinline__ uint32_t fold(uint32_t x) { return x ? 1u + (x - 1u) % 0xFFFFu : 0u; }

// ------------------------------------------------------------------------------------------------ the copy
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

// One copy, wave-uniform: destination chunk c is the 16 bytes at q0 + 16c (q0 16-aligned), of which bytes [a, end)
// from q0 are written; its source bytes start sh bytes into offset 16c of srs, a descriptor from the 4-aligned address
// at or below (source − a) — at most 18 bytes below the source, which lies 20 bytes or more into its frame — to the
// dword holding the source's last byte. A descriptor of no bytes makes the job a zero fill. chunks == 0: no job.
struct CopyJob {
    __amdgpu_buffer_rsrc_t srs;
    uint8_t* q0;
    uint32_t a, end, sh, chunks;
};

// What a lane asks of the wave: len bytes (< 2^30) from base + src to out + dst; zero: zeros instead.
struct Piece {
    uint64_t src, dst;
    uint32_t len, zero;
};

// The next lane of the group, from k on, that has a piece (k moves past it); chunks = 0 when there is none.
__device__ __forceinline__ CopyJob next_job(const uint8_t* __restrict__ base, uint8_t* out, const Piece& pc,
                                            uint32_t cnt, uint32_t& k) {
    CopyJob j{make_rsrc(base, 0), out, 0u, 0u, 0u, 0u};
    while (k < cnt) {
        const uint32_t L = __builtin_amdgcn_readlane(pc.len, k);
        if (L == 0u) {
            ++k;
            continue;
        }
        const bool zero = __builtin_amdgcn_readlane(pc.zero, k) != 0u;
        const uint8_t* sp = base + readlane64(pc.src, k);
        uint8_t* dp = out + readlane64(pc.dst, k);
        ++k;
        j.a = (uint32_t)((uintptr_t)dp & 15u);
        j.q0 = dp - j.a;
        if (!zero) {
            const uint8_t* s0 = sp - j.a;
            j.sh = (uint32_t)((uintptr_t)s0 & 3u);
            j.srs = make_rsrc(s0 - j.sh, ((uint64_t)(j.sh + j.a + L) + 3u) & ~3ull);
        }
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

// The group's pieces as one stream of row pairs (2 KiB of destination each), software-pipelined: the loads of the
// next pair — of this piece, or the first of the next lane that has one — are issued before the current pair is
// stored. A pair past the group's end loads nothing (every offset out of range).
__device__ __forceinline__ void copy_group(const uint8_t* __restrict__ base, uint8_t* out, const Piece& pc,
                                           uint32_t cnt, uint32_t lane) {
    uint32_t k = 0;
    CopyJob cur = next_job(base, out, pc, cnt, k);
    uint32_t c0 = 0;
    RowPair A = load_pair(cur, c0, lane);
    while (cur.chunks) {  // wave-uniform
        CopyJob nj = cur;
        uint32_t nc = c0 + 2u * kWave;
        if (nc >= cur.chunks) {
            nj = next_job(base, out, pc, cnt, k);
            nc = 0;
        }
        const RowPair B = load_pair(nj, nc, lane);
        store_pair(cur, c0, lane, A);
        cur = nj;
        c0 = nc;
        A = B;
    }
}

// nb header bytes (<= 20) of the dwords h[0..4] to p, at any alignment (one lane).
__device__ __forceinline__ void store_header(uint8_t* p, const uint32_t (&h)[5], uint32_t nb) {
    if (nb == 20u && ((uintptr_t)p & 3u) == 0u) {
#pragma unroll
        for (int k = 0; k < 5; ++k) reinterpret_cast<uint32_t*>(p)[k] = h[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (4u * k + b < nb) p[4 * k + b] = (uint8_t)(h[k] >> (8 * b));
}

// ------------------------------------------------------------------------------------------------ fragmentation
__global__ __launch_bounds__(kBlock) void frag_kernel(const uint8_t* __restrict__ base,
                                                      const uint64_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ mtu, uint64_t n,
                                                      const uint64_t* __restrict__ frag_first,
                                                      const uint32_t* __restrict__ frag_src, uint64_t n_frags,
                                                      uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off,
                                                      uint8_t* __restrict__ status) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t groups = (n_frags + kGroup - 1u) / kGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += nwaves) {
        const uint64_t t0 = g * kGroup;
        const uint32_t cnt = (uint32_t)min((uint64_t)kGroup, n_frags - t0);
        Piece pc{0u, 0u, 0u, 0u};
        if (lane < cnt) {
            const uint64_t t = t0 + lane;
            const uint64_t i = frag_src[t];
            const uint64_t d0 = out_off[t], d1 = out_off[t + 1];
            // a slot the map gives to no frame, or gives 2^30 bytes or more, is not written
            if (i < n && d1 >= d0 && d1 - d0 < kLenCap) {
                const uint64_t slot = d1 - d0, o0 = offsets[i], o1 = offsets[i + 1], j = t - frag_first[i];
                const uint64_t len = o1 >= o0 ? o1 - o0 : kLenCap;
                const uint32_t m = mtu[i];
                uint32_t st = kStBad;
                if (m < 28u) {
                    pc = Piece{0u, d0, (uint32_t)slot, 1u};  // no mtu at all: bad, the slot is zero
                } else if (len <= m && len < kLenCap) {
                    st = kStPass;
                    if (j == 0u && slot == len) {  // through as it stands: the first 20 bytes here, the rest a piece
                        const uint32_t nb = (uint32_t)min(len, (uint64_t)20u);
                        const FrameWin F = frame_win(base + o0, nb);
                        const uint32_t h[5] = {F.at(0), F.at(4), F.at(8), F.at(12), F.at(16)};
                        store_header(out + d0, h, nb);
                        pc = Piece{o0 + 20u, d0 + 20u, (uint32_t)len - nb, 0u};
                    }
                } else if (len < kLenCap) {
                    bool cut = false;
                    {  // len > m >= 28: the frame holds its 20 header bytes
                        const FrameWin F = frame_win(base + o0, 20u);
                        const uint32_t h0 = F.at(0), h1 = F.at(4), h2 = F.at(8);
                        const uint32_t f16 = bswap16(h1 >> 16), o = f16 & 0x1FFFu;  // bytes 6-7
                        const bool fits = (h0 & 0xFFu) == 0x45u && bswap16(h0 >> 16) == len &&
                                          (uint64_t)o * 8u + len - 20u <= 65535u;
                        st = !fits ? kStBad : (f16 & 0x4000u) ? kStDf : kStCut;
                        const uint32_t per = (m - 20u) & ~7u, pay = (uint32_t)len - 20u;  // fits: len <= 65535
                        if (st == kStCut && j < (pay + per - 1u) / per) {
                            const uint32_t at = (uint32_t)j * per, pl = min(per, pay - at);
                            const bool last = at + pl == pay;
                            if (slot == 20u + pl) {
                                cut = true;
                                // RFC 1624 eqn. 3 over words 1 (total length) and 3 (flags, offset)
                                const uint32_t m1 = (uint32_t)len, n1 = 20u + pl;
                                const uint32_t n3 = (f16 & 0xC000u) | (last ? f16 & 0x2000u : 0x2000u) | (o + at / 8u);
                                const uint32_t hc = bswap16(h2 >> 16);
                                const uint32_t nc = ~fold((~hc & 0xFFFFu) + (~m1 & 0xFFFFu) + n1 + (~f16 & 0xFFFFu) + n3) &
                                                    0xFFFFu;
                                const uint32_t h[5] = {(h0 & 0xFFFFu) | (bswap16(n1) << 16),
                                                       (h1 & 0xFFFFu) | (bswap16(n3) << 16),
                                                       (h2 & 0xFFFFu) | (bswap16(nc) << 16), F.at(12), F.at(16)};
                                store_header(out + d0, h, 20u);
                                pc = Piece{o0 + 20u + at, d0 + 20u, pl, 0u};
                            }
                        }
                    }
                    if (!cut && st != kStCut) pc = Piece{0u, d0, (uint32_t)slot, 1u};  // DF and bad: the slot is zero
                }
                if (j == 0u) status[i] = (uint8_t)st;
            }
        }
        copy_group(base, out, pc, cnt, lane);
    }
}

// ------------------------------------------------------------------------------------------------ reassembly
// meta dword of a position (0 for a non-member): payload bytes (<= 65515), fragment offset, MF, member, cont(p)
constexpr uint32_t kPayMask = 0xFFFFu, kOffShift = 16, kOffMask = 0x1FFFu;
constexpr uint32_t kMf = 1u << 29, kMember = 1u << 30, kCont = 1u << 31;

__device__ __forceinline__ uint32_t m_pay(uint32_t m) { return m & kPayMask; }
__device__ __forceinline__ uint32_t m_off(uint32_t m) { return (m >> kOffShift) & kOffMask; }

// The member test of include/nsx_csum.h over a frame of flen bytes (capped): the meta dword without cont, 0 for a
// non-member. Only the 20 header bytes are read, and none when the frame is shorter than 21.
__device__ __forceinline__ uint32_t reasm_member(const FrameWin& F, uint32_t flen, uint32_t (&h)[5]) {
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = 0u;
    if (flen < 21u) return 0u;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        h[k] = F.at(4u * k);
        sum += (h[k] & 0xFFFFu) + (h[k] >> 16);
    }
    sum = (sum & 0xFFFFu) + (sum >> 16);
    sum = (sum & 0xFFFFu) + (sum >> 16);  // byte order does not matter to an end-around-carry sum being 0xFFFF
    const uint32_t f16 = bswap16(h[1] >> 16), o = f16 & 0x1FFFu, mf = f16 & 0x2000u, pay = flen - 20u;
    const bool ok = (h[0] & 0xFFu) == 0x45u && bswap16(h[0] >> 16) == flen && sum == 0xFFFFu && (mf || o) &&
                    !(mf && (pay & 7u)) && o * 8u + pay <= 65515u;
    return ok ? pay | (o << kOffShift) | (mf ? kMf : 0u) | kMember : 0u;
}

// One lane per frame: the fragment offset (0 for a non-member) and the identity index as the first sort's input, the
// datagram key per frame, and the member bits.
__global__ __launch_bounds__(kBlock) void reasm_key_kernel(const uint8_t* __restrict__ base,
                                                           const uint64_t* __restrict__ offsets, uint32_t n,
                                                           uint32_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                           uint32_t* __restrict__ fkey, uint64_t* __restrict__ is_frag) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = gi < n;
    const uint32_t i = live ? (uint32_t)gi : 0u;
    uint32_t m = 0u, key = kNone;
    if (live) {
        const uint64_t o0 = offsets[i], o1 = offsets[(uint64_t)i + 1];
        // a frame longer than any length field can say is no member; the cap keeps the arithmetic in 32 bits
        const uint32_t flen = o1 >= o0 ? (uint32_t)min(o1 - o0, (uint64_t)0x20000u) : 0u;
        const FrameWin F = frame_win(base + o0, min(flen, 20u));
        uint32_t h[5];
        m = reasm_member(F, flen, h);
        if (m) {
            uint32_t k = (0x811C9DC5u ^ h[3]) * 0x01000193u;
            k = (k ^ h[4]) * 0x01000193u;
            key = (k ^ ((h[1] & 0xFFFFu) | ((h[2] & 0xFF00u) << 8))) * 0x01000193u;  // b4 | b5<<8 | b9<<16
        }
        keys[i] = m_off(m);
        idx[i] = i;
        fkey[i] = key;
    }
    const uint64_t bits = __ballot(m != 0u);  // a wave holds the 64 frames of one mask word
    if ((threadIdx.x & 63u) == 0u && live) is_frag[gi >> 6] = bits;
}

// The second sort's input: position p of the offset order holds frame order[p]; its key is that frame's.
__global__ __launch_bounds__(kBlock) void reasm_regather_kernel(const uint32_t* __restrict__ order, uint32_t n,
                                                                const uint32_t* __restrict__ fkey,
                                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ idx) {
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n) return;
    const uint32_t f = order[gi];
    keys[gi] = f < n ? fkey[f] : kNone;
    idx[gi] = f;
}

__global__ __launch_bounds__(kBlock) void reasm_head_kernel(const uint8_t* __restrict__ base,
                                                            const uint64_t* __restrict__ offsets, uint32_t n,
                                                            const uint32_t* __restrict__ order,
                                                            uint32_t* __restrict__ meta) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint64_t first = wave * kHeadFrames;  // lane 1's position
    if (first >= n) return;                     // wave-uniform
    const int64_t fi = (int64_t)first + lane - 1;
    bool live = fi >= 0 && fi < (int64_t)n;
    const uint32_t p = live ? (uint32_t)fi : 0u;
    const uint32_t i = live ? order[p] : 0u;
    live = live && i < n;
    const uint64_t o0 = live ? offsets[i] : 0u, o1 = live ? offsets[(uint64_t)i + 1] : 0u;
    const uint32_t flen = o1 >= o0 ? (uint32_t)min(o1 - o0, (uint64_t)0x20000u) : 0u;
    const FrameWin F = frame_win(base + o0, min(flen, 20u));
    uint32_t h[5];
    const uint32_t m = reasm_member(F, flen, h);
    // the position before: lane - 1 (lane 0's own result is not used); every ds_bpermute runs with the whole wave
    const uint32_t src = (lane + 63u) & 63u;
    const uint32_t pm = bperm(m, src);
    bool cont = m && pm && (pm & kMf) && m_off(m) * 8u == m_off(pm) * 8u + m_pay(pm);
    const uint32_t idp = (h[1] & 0xFFFFu) | ((h[2] & 0xFF00u) << 8);  // ident and protocol
    cont = (bperm(h[3], src) == h[3]) && cont;
    cont = (bperm(h[4], src) == h[4]) && cont;
    cont = (bperm(idp, src) == idp) && cont;
    if (fi >= 0 && fi < (int64_t)n && lane >= 1u) meta[p] = m | (cont ? kCont : 0u);
}

// Exclusive prefix sums over the 256 threads of a block, two values at once; total[] = the block's sums.
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

struct ReasmWorkPtrs {
    uint64_t* sums;      // per scan block: two sums
    uint64_t* run_dst;   // per run: its datagram's offset in out
    uint32_t* meta;      // per position
    uint32_t* wrun;      // per position: its run
    uint32_t* run_head;  // per run: its first position
    uint32_t* run_seg;   // per run: its datagram, or kNone
    uint32_t* fkey;      // per frame: the datagram key
};

struct ReasmOut {
    uint64_t* n_out;
    uint8_t* out;
    uint64_t* out_off;
    uint64_t* first_pos;
    uint32_t* frag_cnt;
    uint32_t* frame_seg;
};

// DONE false, the runs: a position that does not continue the one before starts a run (non-members are runs of one).
// DONE true, the complete runs, counted at their last positions, with their datagram bytes.
// APPLY false: sums[2b..] = the block's sums. APPLY true: sums holds their exclusive prefix over the blocks, and the
// per-position / per-run / per-datagram values are written.
template <bool DONE, bool APPLY>
__global__ __launch_bounds__(kBlock) void reasm_scan_block_kernel(uint32_t n, uint32_t per_block, ReasmWorkPtrs w,
                                                                  ReasmOut o) {
    __shared__ uint64_t lds[kWavesPerBlock][2];
    const uint64_t lo = (uint64_t)blockIdx.x * per_block, hi = min(lo + per_block, (uint64_t)n);
    uint64_t carry[2] = {0, 0};
    if (APPLY) {
        carry[0] = w.sums[2u * blockIdx.x];
        carry[1] = w.sums[2u * blockIdx.x + 1u];
    }
    for (uint64_t t = lo; t < hi; t += kBlock) {  // block-uniform trip count
        const uint64_t fi = t + threadIdx.x;
        const bool live = fi < hi;
        const uint32_t p = (uint32_t)fi;
        const uint32_t m = live ? w.meta[p] : 0u;
        uint64_t v[2] = {0, 0}, tot[2];
        uint32_t r = 0, head = 0;
        bool last = false;
        if (DONE) {
            last = live && (p + 1u == n || !(w.meta[p + 1u] & kCont));
            if (last) {
                r = w.wrun[p];
                head = w.run_head[r];
                const uint32_t mh = w.meta[head];  // with cont(p) the first frame is a member as well
                if ((m & kMember) && !(m & kMf) && (mh & kMember) && m_off(mh) == 0u && head <= p) {
                    v[0] = 1u;
                    v[1] = 20u + m_off(m) * 8u + m_pay(m);
                }
            }
        } else {
            v[0] = live && !(m & kCont);
        }
        const uint64_t mine0 = v[0], mine1 = v[1];
        block_excl_scan(v, tot, lds);
        if (APPLY && live) {
            if (DONE) {
                if (last) {
                    const uint64_t s = carry[0] + v[0], at = carry[1] + v[1];
                    w.run_seg[r] = mine0 ? (uint32_t)s : kNone;
                    if (mine0) {
                        w.run_dst[r] = at;
                        o.out_off[s] = at;
                        o.first_pos[s] = head;
                        o.frag_cnt[s] = p - head + 1u;
                    }
                }
                (void)mine1;
            } else {
                const uint32_t run = (uint32_t)(carry[0] + v[0] + mine0) - 1u;  // p = 0 starts run 0
                w.wrun[p] = run;
                if (mine0) w.run_head[run] = p;
            }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) carry[k] += tot[k];
    }
    if (!APPLY && threadIdx.x == 0) {
        w.sums[2u * blockIdx.x] = carry[0];
        w.sums[2u * blockIdx.x + 1u] = carry[1];
    }
}

// One workgroup: sums (nb pairs) → their exclusive prefix in place; DONE: the totals close the outputs.
template <bool DONE>
__global__ __launch_bounds__(kBlock) void reasm_scan_sums_kernel(uint64_t* __restrict__ sums, uint32_t nb, ReasmOut o) {
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
    if (DONE && threadIdx.x == 0) {
        *o.n_out = carry[0];
        if (carry[0] == 0u) o.out_off[0] = 0;  // with datagrams, entry 0 belongs to the first of them
        o.out_off[carry[0]] = carry[1];
    }
}

__global__ __launch_bounds__(kBlock) void reasm_emit_kernel(const uint8_t* __restrict__ base,
                                                            const uint64_t* __restrict__ offsets, uint32_t n,
                                                            const uint32_t* __restrict__ order, ReasmWorkPtrs w,
                                                            ReasmOut o) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * kWavesPerBlock;
    const uint64_t groups = ((uint64_t)n + kGroup - 1u) / kGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); g < groups; g += nwaves) {
        const uint32_t g0 = (uint32_t)(g * kGroup), cnt = min(kGroup, n - g0);
        Piece pc{0u, 0u, 0u, 0u};
        if (lane < cnt) {
            const uint32_t p = g0 + lane, m = w.meta[p], f = order[p];
            if (f < n) {
                const uint32_t r = w.wrun[p];
                const uint32_t s = (m & kMember) ? w.run_seg[r] : kNone;
                o.frame_seg[f] = s;
                if (s != kNone) {
                    const uint64_t off = offsets[f], at = w.run_dst[r];
                    pc = Piece{off + 20u, at + 20u + (uint64_t)m_off(m) * 8u, m_pay(m), 0u};
                    if (w.run_head[r] == p) {  // the datagram's header: this fragment's, whole again
                        const FrameWin F = frame_win(base + off, 20u);
                        const uint32_t dlen = (uint32_t)(o.out_off[(uint64_t)s + 1] - at);
                        uint32_t h[5] = {(F.at(0) & 0xFFFFu) | (bswap16(dlen) << 16), F.at(4) & 0x00C0FFFFu,
                                         F.at(8) & 0xFFFFu, F.at(12), F.at(16)};
                        uint32_t sum = 0;
#pragma unroll
                        for (int k = 0; k < 5; ++k) sum += (h[k] & 0xFFFFu) + (h[k] >> 16);
                        sum = (sum & 0xFFFFu) + (sum >> 16);
                        sum = (sum & 0xFFFFu) + (sum >> 16);
                        h[2] |= (~sum & 0xFFFFu) << 16;
                        store_header(o.out + at, h, 20u);
                    }
                }
            }
        }
        copy_group(base, o.out, pc, cnt, lane);
    }
}

uint32_t scan_block_frames(const LaunchCfg& c) {
    if (c.run_segs <= 0) return kScanBlockDefault;
    return std::min<uint32_t>(std::max<uint32_t>((uint32_t)c.run_segs, kScanBlockMin), kScanBlockMax);
}

uint32_t copy_grid(const LaunchCfg& c, uint64_t tasks) {
    const int bpc = c.blocks_per_cu >= 1 && c.blocks_per_cu <= 8 ? c.blocks_per_cu : 8;
    const uint64_t groups = (tasks + kGroup - 1) / kGroup;
    return (uint32_t)std::min<uint64_t>((groups + kWavesPerBlock - 1) / kWavesPerBlock,
                                        (uint64_t)std::max(c.cus, 1) * bpc);
}

struct ReasmWork {
    uint64_t sums, run_dst, meta, wrun, run_head, run_seg, fkey, sort, total;  // byte offsets from an 8-aligned start
};

ReasmWork reasm_layout(uint64_t n) {
    ReasmWork w;
    const uint64_t nb_max = (n + kScanBlockMin - 1) / kScanBlockMin;  // the smallest scan block a tune can ask for
    w.sums = 0;
    w.run_dst = w.sums + 16 * (nb_max + 1);
    w.meta = w.run_dst + 8 * n;
    w.wrun = w.meta + 4 * n;
    w.run_head = w.wrun + 4 * n;
    w.run_seg = w.run_head + 4 * n;
    w.fkey = w.run_seg + 4 * n;
    w.sort = (w.fkey + 4 * n + 7u) & ~7ull;
    w.total = w.sort + flow_sort_bytes(n) + 8;  // + the rounding of the caller's pointer
    return w;
}

}  // namespace

hipError_t launch_frag(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu,
                       uint64_t n, const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags,
                       uint8_t* d_out, const uint64_t* d_out_off, uint8_t* d_status, hipStream_t st) {
    if (n_frags == 0) return hipSuccess;
    hipLaunchKernelGGL(frag_kernel, dim3(copy_grid(c, n_frags)), dim3(kBlock), 0, st,
                       static_cast<const uint8_t*>(d_base), d_offsets, d_mtu, n, d_frag_first, d_frag_src, n_frags,
                       d_out, d_out_off, d_status);
    return hipGetLastError();
}

uint64_t reasm_work_bytes(uint64_t n) { return reasm_layout(n).total; }

hipError_t launch_reasm(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, uint64_t n64,
                        uint32_t* d_order, const ReasmDevOut& out, void* work, hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (frag_api.cpp)
    const ReasmWork L = reasm_layout(n);
    uint8_t* wb = reinterpret_cast<uint8_t*>(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    const ReasmWorkPtrs w{reinterpret_cast<uint64_t*>(wb + L.sums),     reinterpret_cast<uint64_t*>(wb + L.run_dst),
                          reinterpret_cast<uint32_t*>(wb + L.meta),     reinterpret_cast<uint32_t*>(wb + L.wrun),
                          reinterpret_cast<uint32_t*>(wb + L.run_head), reinterpret_cast<uint32_t*>(wb + L.run_seg),
                          reinterpret_cast<uint32_t*>(wb + L.fkey)};
    const ReasmOut o{out.n_out, out.out, out.out_off, out.first_pos, out.frag_cnt, out.frame_seg};
    const uint8_t* base = static_cast<const uint8_t*>(d_base);
    const uint32_t per = scan_block_frames(c);
    const uint32_t nb = (uint32_t)(((uint64_t)n + per - 1) / per);
    if (n) {
        const FlowSortWork S = flow_sort_work(wb + L.sort, n);
        const uint32_t kgrid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(reasm_key_kernel, dim3(kgrid), dim3(kBlock), 0, st, base, d_offsets, n, S.keys[0], S.idx[0],
                           w.fkey, out.is_frag);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = launch_flow_sort(c, n, S, d_order, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(reasm_regather_kernel, dim3(kgrid), dim3(kBlock), 0, st, d_order, n, w.fkey, S.keys[0],
                           S.idx[0]);
        e = hipGetLastError();
        if (e == hipSuccess) e = launch_flow_sort(c, n, S, d_order, st);
        if (e != hipSuccess) return e;
        const uint64_t hw = ((uint64_t)n + kHeadFrames - 1) / kHeadFrames;
        hipLaunchKernelGGL(reasm_head_kernel, dim3((uint32_t)((hw + kWavesPerBlock - 1) / kWavesPerBlock)),
                           dim3(kBlock), 0, st, base, d_offsets, n, d_order, w.meta);
        hipLaunchKernelGGL((reasm_scan_block_kernel<false, false>), dim3(nb), dim3(kBlock), 0, st, n, per, w, o);
        hipLaunchKernelGGL(reasm_scan_sums_kernel<false>, dim3(1), dim3(kBlock), 0, st, w.sums, nb, o);
        hipLaunchKernelGGL((reasm_scan_block_kernel<false, true>), dim3(nb), dim3(kBlock), 0, st, n, per, w, o);
        hipLaunchKernelGGL((reasm_scan_block_kernel<true, false>), dim3(nb), dim3(kBlock), 0, st, n, per, w, o);
    }
    hipLaunchKernelGGL(reasm_scan_sums_kernel<true>, dim3(1), dim3(kBlock), 0, st, w.sums, nb, o);
    if (n) {
        hipLaunchKernelGGL((reasm_scan_block_kernel<true, true>), dim3(nb), dim3(kBlock), 0, st, n, per, w, o);
        hipLaunchKernelGGL(reasm_emit_kernel, dim3(copy_grid(c, n)), dim3(kBlock), 0, st, base, d_offsets, n, d_order,
                           w, o);
    }
    return hipGetLastError();
}

}  // namespace nsx
