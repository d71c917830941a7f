// nat_kernels.hip — the gfx950 kernel of the in-place NAT rewrite (nsx_nat_ipv4_tcp_rewrite_dev /
// nsx_nat_ipv6_tcp_rewrite_dev, include/nsx_csum.h): per frame a lookup of its address / port tuple in a
// translation table, new addresses, ports and TTL / hop limit written over the old, and both checksums corrected
// from the old and new words alone (RFC 1624 eqn. 3). The payload is neither read nor written.
//
// One lane per frame, one launch, no grid-stride loop: the work per frame is a handful of header dwords, one or a
// few table entries and two or three stores, so there is no launch shape worth overriding.
//   read     the header through FrameWin (aligned dwords realigned by v_alignbyte; nothing outside the dwords that
//            hold the frame's own bytes is loaded), the receive pass's conditions through frame_wellformed.
//   probe    FNV-1a over the tuple's dwords (the flow key of gro_flow_kernels.hip), then a COUNTED loop of at most
//            `slots` iterations over 16-byte loads of whole entries: an entry that is not occupied ends it with a
//            miss, an occupied one whose whole match tuple equals the frame's with a hit. A table without an empty
//            entry — never built by nsx_nat_table_build_host, but the table is the caller's device memory — ends in
//            a miss after `slots` probes; no table contents can make the loop spin.
//   update   in registers; see csum_update.
//   store    only whole dword groups of the frame's own header are written (IPv4: bytes 8-19, TCP bytes 0-3 and
//            16-19; IPv6: bytes 4-43 and TCP bytes 16-19), each by store_own: byte and 16-bit stores up to the next
//            4-byte boundary, aligned dword stores between, 16-bit and byte stores for the rest. No store covers a
//            byte outside [offsets[i], offsets[i+1]), whatever the frame's alignment: the neighbour's bytes — which
//            another lane may be writing — are never read-modify-written, and nothing is stored past the buffer.
//   hit      one __ballot per wave, written by its lane 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csum_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

typedef uint32_t u32x4a __attribute__((ext_vector_type(4)));  // 16 bytes at a 16-byte-aligned address

// The two big-endian 16-bit words of a little-endian dword, added up.
__device__ __forceinline__ uint32_t be_words(uint32_t w) {
    const uint32_t b = bswap32(w);
    return (b >> 16) + (b & 0xFFFFu);
}

// RFC 1624 eqn. 3 as include/nsx_csum.h evaluates it: hc the field (big-endian value), acc the sum over the covered
// words of (~m & 0xFFFF) + m' (at most 18 words: below 2^22).
__device__ __forceinline__ uint32_t csum_update(uint32_t hc, uint32_t acc) {
    const uint32_t x = (~hc & 0xFFFFu) + acc;
    const uint32_t fold = x ? 1u + (x - 1u) % 0xFFFFu : 0u;
    return ~fold & 0xFFFFu;
}

// (~m & 0xFFFF) + m' over the big-endian words of the dwords old -> repl.
__device__ __forceinline__ uint32_t delta(uint32_t old, uint32_t repl) { return be_words(~old) + be_words(repl); }
// The same for the one word in the low halves of old and repl.
__device__ __forceinline__ uint32_t delta16(uint32_t old, uint32_t repl) {
    return (~bswap16(old) & 0xFFFFu) + bswap16(repl);
}

// The 4·K bytes v[0..K) (little-endian dwords) to q[0, 4K), q at any alignment, all of them the frame's own: bytes
// up to the next 4-byte boundary by a byte and / or a 16-bit store, whole aligned dwords, and the rest by a 16-bit
// and / or a byte store. Every store is naturally aligned and covers bytes of [q, q + 4K) only.
template <uint32_t K>
__device__ __forceinline__ void store_own(uint8_t* q, const uint32_t (&v)[K]) {
    const uint32_t a = (uint32_t)((uintptr_t)q & 3u), head = (4u - a) & 3u;  // head = a: 0 -> 0, 1 -> 3, 2 -> 2, 3 -> 1
    if (a & 1u) q[0] = (uint8_t)v[0];
    if (head & 2u) *reinterpret_cast<uint16_t*>(q + (a & 1u)) = (uint16_t)(v[0] >> (8u * (a & 1u)));
    // run bytes [head + 4j, head + 4j + 4): an aligned dword; the last of them (j = K - 1) only when head == 0
#pragma unroll
    for (uint32_t j = 0; j < K; ++j) {
        const uint32_t x = __builtin_amdgcn_alignbyte(j + 1 < K ? v[j + 1] : 0u, v[j], head);
        uint8_t* d = q + head + 4u * j;
        if (j + 1 < K || head == 0u) {
            *reinterpret_cast<uint32_t*>(d) = x;
        } else {  // the 4 - head = a bytes left, from an aligned address
            if (a & 2u) *reinterpret_cast<uint16_t*>(d) = (uint16_t)x;
            if (a & 1u) d[a & 2u] = (uint8_t)(x >> (8u * (a & 2u)));
        }
    }
}

template <bool V6>
__global__ __launch_bounds__(kBlock) void nat_rewrite_kernel(uint8_t* __restrict__ base,
                                                             const uint64_t* __restrict__ offsets, uint32_t n,
                                                             const uint64_t* __restrict__ valid,
                                                             const uint8_t* __restrict__ table, uint32_t slot_mask,
                                                             uint32_t ttl_dec, uint64_t* __restrict__ hit_mask) {
    constexpr uint32_t kT = V6 ? 9u : 3u;      // tuple dwords
    constexpr uint32_t kE = 2u * kT + 2u;      // entry dwords: match, state, new, zero
    constexpr uint32_t kAddr = V6 ? 8u : 12u;  // frame byte of the first address dword
    const uint64_t gi = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = gi < n;
    const uint32_t i = (uint32_t)gi;
    bool hit = false;
    if (live && ((valid[i >> 6] >> (i & 63u)) & 1u)) {  // a frame the mask rejects is not read at all
        const uint64_t o0 = offsets[i], o1 = offsets[(uint64_t)i + 1];
        // a frame longer than any length field can say is not well-formed
        const uint32_t flen = (uint32_t)min(o1 - o0, (uint64_t)0x20000u);
        uint8_t* p = base + o0;
        const FrameWin F = frame_win(p, flen);
        uint32_t iph, seg;
        const uint32_t h0 = F.at(0), h1 = F.at(4), h2 = V6 ? 0u : F.at(8);
        // well-formed: iph + 20 <= flen, so every byte read or written below is the frame's own:
        // IPv4 [8, 20) and [iph, iph + 20), IPv6 [4, 60)
        const uint32_t ttl = V6 ? h1 >> 24 : h2 & 0xFFu;
        if (frame_wellformed<V6>(h0, h1, h2, flen, iph, seg) && ttl > ttl_dec) {
            uint32_t t[kT], e[kE];
#pragma unroll
            for (uint32_t k = 0; k + 1 < kT; ++k) t[k] = F.at(kAddr + 4u * k);
            t[kT - 1] = F.at(iph);  // the ports
            uint32_t h = 0x811C9DC5u;
#pragma unroll
            for (uint32_t k = 0; k < kT; ++k) h = (h ^ t[k]) * 0x01000193u;
            // slot_mask + 1 probes at the most, whatever the table holds (slot_mask < 2^31: the count cannot wrap)
            for (uint32_t probe = 0; probe <= slot_mask && !hit; ++probe) {
                const uint32_t slot = (h + probe) & slot_mask;
                const u32x4a* ent = reinterpret_cast<const u32x4a*>(table + (uint64_t)slot * (4u * kE));
#pragma unroll
                for (uint32_t c = 0; c < kE / 4u; ++c) {
                    const u32x4a x = ent[c];
                    e[4u * c] = x.x, e[4u * c + 1] = x.y, e[4u * c + 2] = x.z, e[4u * c + 3] = x.w;
                }
                if (e[kT] != 1u) break;  // not occupied: a miss
                bool eq = true;
#pragma unroll
                for (uint32_t k = 0; k < kT; ++k) eq = eq && e[k] == t[k];
                hit = eq;
            }
            if (hit) {
                const uint32_t* nw = e + kT + 1u;  // the new tuple
                uint32_t addr = 0;                 // the address words' part of both sums
#pragma unroll
                for (uint32_t k = 0; k + 1 < kT; ++k) addr += delta(t[k], nw[k]);
                const uint32_t t4 = F.at(iph + 16u);  // TCP bytes 16-19: the checksum, the urgent pointer
                const uint32_t tc = csum_update(bswap16(t4), addr + delta(t[kT - 1], nw[kT - 1]));
                const uint32_t tcp4[1] = {(t4 & 0xFFFF0000u) | bswap16(tc)};
                if constexpr (V6) {
                    uint32_t v[10];  // bytes 4-43: payload length, next header, hop limit; addresses; ports
                    v[0] = (h1 & 0x00FFFFFFu) | ((ttl - ttl_dec) << 24);
#pragma unroll
                    for (uint32_t k = 0; k < kT; ++k) v[1 + k] = nw[k];
                    store_own(p + 4, v);
                } else {
                    // bytes 8-11: TTL, protocol, header checksum (over the word at bytes 8-9 and the addresses)
                    const uint32_t w89 = (h2 & 0xFF00u) | (ttl - ttl_dec);
                    const uint32_t hc = csum_update(bswap16(h2 >> 16), addr + delta16(h2, w89));
                    const uint32_t v[3] = {w89 | (bswap16(hc) << 16), nw[0], nw[1]};
                    const uint32_t ports[1] = {nw[2]};
                    store_own(p + 8, v);
                    store_own(p + iph, ports);
                }
                store_own(p + iph + 16u, tcp4);
            }
        }
    }
    const uint64_t word = __ballot(hit);  // lanes past n vote 0: bits past n stay clear
    if (live && (threadIdx.x & 63u) == 0u) hit_mask[i >> 6] = word;
}

}  // namespace

hipError_t launch_nat_rewrite(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n64, const uint64_t* valid,
                              const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit, hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (nat_api.cpp)
    if (!n) return hipSuccess;
    const uint32_t grid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
    const uint32_t slot_mask = (uint32_t)(slots - 1);  // slots a power of two <= 2^31 (nat_api.cpp)
    uint8_t* base = static_cast<uint8_t*>(d_base);
    const uint8_t* table = static_cast<const uint8_t*>(d_table);
    if (ipver == 6)
        hipLaunchKernelGGL(nat_rewrite_kernel<true>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, valid, table,
                           slot_mask, ttl_dec, d_hit);
    else
        hipLaunchKernelGGL(nat_rewrite_kernel<false>, dim3(grid), dim3(kBlock), 0, st, base, d_offsets, n, valid,
                           table, slot_mask, ttl_dec, d_hit);
    return hipGetLastError();
}

}  // namespace nsx
