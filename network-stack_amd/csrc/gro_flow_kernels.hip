// gro_flow_kernels.hip — gfx950 kernels of flow-keyed TCP receive coalescing (nsx_gro_flow_ipv4_tcp_dev /
// nsx_gro_flow_ipv6_tcp_dev, include/nsx_csum.h): the frames of many interleaved connections are put in a stable
// order by a 32-bit flow key, and the passes of gro_kernels.hip run over that order (launch_gro_ordered). A key
// collision costs merges and nothing else: same(i, i-1) still compares every field.
//
// One serial chain of launches, none of which waits on another workgroup (cross-tile ordering comes from the
// launch boundary, never from a flag, a ticket or a look-back):
//   key      one lane per frame: the head pass's membership test, then FNV-1a over the address dwords and the
//            ports; 0xFFFFFFFF for a non-member. Writes the key and the identity index.
//   then per 8-bit digit, least significant first (a stable LSD radix sort of (key, index), four passes):
//   hist     a workgroup per tile of rows × 256 keys: the tile's digit counts into the (digit × tile) table.
//   scan     one workgroup: the table's exclusive prefix sums in place, digit-major, so an entry becomes the
//            output position of its tile's first key with that digit. It sweeps 8,192 entries at a time (32 per
//            thread, 16-byte loads and stores), as often as the table needs.
//   scatter  a workgroup per tile. Wave w owns the w-th quarter of the tile, in arrival order. It counts its
//            digits into its LDS row; after one barrier thread d turns the four rows of digit d into the waves'
//            bases; then every wave walks its keys 64 at a time: the lanes with equal digits find each other by
//            __ballot on the eight digit bits, the rank among them is the count of lower lanes, and the lowest
//            lane moves the wave's base on. Arrival order inside a tile = (wave, row, lane), which is what makes
//            the sort stable.
//   The key and index buffers ping-pong inside the workspace; the last scatter writes indices only, to d_order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "csum_kernels.h"
#include "kernel_util.h"

namespace nsx {
namespace {

constexpr uint32_t kDigitBits = 8, kDigits = 1u << kDigitBits, kPasses = 32u / kDigitBits;
constexpr uint32_t kTileRowsDefault = 16, kTileRowsMax = 64;  // keys per tile in units of kBlock
constexpr uint32_t kScanPer = 32;                             // table entries per thread and sweep of the scan
constexpr uint32_t kNoFlow = 0xFFFFFFFFu;
static_assert(kDigits == kBlock, "thread d owns digit d");
static_assert(kDigits % kScanPer == 0 && kScanPer % 4 == 0, "the scan takes whole threads, 16 bytes at a time");

// ------------------------------------------------------------------------------------------------ key pass
template <bool V6>
__global__ __launch_bounds__(kBlock) void flow_key_kernel(const uint8_t* __restrict__ base,
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
        uint32_t iph, seg;
        // well-formed: iph + 20 <= flen, so the ports and byte 12 are inside the frame (and the window clamps)
        const uint32_t h0 = F.at(0), h1 = F.at(4), h2 = V6 ? 0u : F.at(8);
        if (frame_wellformed<V6>(h0, h1, h2, flen, iph, seg) && tcp_doff_fits(F.at(iph + 12u), seg)) {
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

// ------------------------------------------------------------------------------------------------ radix sort
__device__ __forceinline__ uint32_t digit_of(uint32_t key, uint32_t shift) { return (key >> shift) & (kDigits - 1u); }

__global__ __launch_bounds__(kBlock) void flow_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                           uint32_t tile_keys, uint32_t shift, uint32_t ntiles,
                                                           uint32_t* __restrict__ table) {
    __shared__ uint32_t h[kDigits];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * tile_keys, hi = min(lo + tile_keys, (uint64_t)n);
    for (uint64_t t = lo + threadIdx.x; t < hi; t += kBlock) atomicAdd(&h[digit_of(keys[t], shift)], 1u);
    __syncthreads();
    table[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// One workgroup: the table's `entries` counts → their exclusive prefix sums, in place (the total is n < 2^32).
__global__ __launch_bounds__(kBlock) void flow_scan_kernel(uint32_t* __restrict__ table, uint64_t entries) {
    __shared__ uint32_t wsum[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint64_t t = 0; t < entries; t += (uint64_t)kBlock * kScanPer) {  // block-uniform trip count
        const uint64_t e0 = t + (uint64_t)threadIdx.x * kScanPer;
        const bool live = e0 < entries;  // entries is a multiple of kDigits: a thread has all its entries or none
        uint32_t v[kScanPer], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; k += 4u) {
            const u32x4 x = live ? *reinterpret_cast<const u32x4*>(table + e0 + k) : u32x4{0u, 0u, 0u, 0u};
            v[k] = x.x, v[k + 1] = x.y, v[k + 2] = x.z, v[k + 3] = x.w;
        }
#pragma unroll
        for (uint32_t k = 0; k < kScanPer; ++k) {
            const uint32_t x = v[k];
            v[k] = sum;
            sum += x;
        }
        uint32_t incl = sum;
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t y = __shfl_up(incl, d, 64);
            if (lane >= d) incl += y;
        }
        if (lane == 63u) wsum[w] = incl;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
        for (uint32_t j = 0; j < kWavesPerBlock; ++j) {
            const uint32_t s = wsum[j];
            if (j < w) pre += s;
            tot += s;
        }
        const uint32_t b = carry + pre + incl - sum;
        if (live) {
#pragma unroll
            for (uint32_t k = 0; k < kScanPer; k += 4u)
                *reinterpret_cast<u32x4*>(table + e0 + k) = u32x4{b + v[k], b + v[k + 1], b + v[k + 2], b + v[k + 3]};
        }
        carry += tot;
        __syncthreads();
    }
}

// LAST: the final digit — only the indices are written (to d_order).
template <bool LAST>
__global__ __launch_bounds__(kBlock) void flow_scatter_kernel(const uint32_t* __restrict__ keys_in,
                                                              const uint32_t* __restrict__ idx_in, uint32_t n,
                                                              uint32_t rows, uint32_t shift, uint32_t ntiles,
                                                              const uint32_t* __restrict__ table,
                                                              uint32_t* __restrict__ keys_out,
                                                              uint32_t* __restrict__ idx_out) {
    __shared__ uint32_t wbase[kWavesPerBlock][kDigits];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t wave_keys = (uint64_t)rows * kWave;
    const uint64_t wlo = ((uint64_t)blockIdx.x * kWavesPerBlock + w) * wave_keys;  // this wave's keys: [wlo, whi)
    const uint64_t whi = min(wlo + wave_keys, (uint64_t)n);
    // the wave's digit counts
    for (uint32_t j = lane; j < kDigits; j += kWave) wbase[w][j] = 0u;
    __syncthreads();
    for (uint64_t t = wlo + lane; t < whi; t += kWave) atomicAdd(&wbase[w][digit_of(keys_in[t], shift)], 1u);
    __syncthreads();
    {  // digit d = threadIdx.x: where each wave's keys with that digit start
        uint32_t b = table[(uint64_t)threadIdx.x * ntiles + blockIdx.x];
        for (uint32_t j = 0; j < kWavesPerBlock; ++j) {
            const uint32_t c = wbase[j][threadIdx.x];
            wbase[j][threadIdx.x] = b;
            b += c;
        }
    }
    __syncthreads();
    // From here on a wave touches its own LDS row only: a wave's DS operations run in order, the fences keep the
    // compiler from moving them across each other.
    for (uint64_t t0 = wlo; t0 < whi; t0 += kWave) {  // wave-uniform
        const uint64_t t = t0 + lane;
        const bool live = t < whi;
        const uint32_t key = live ? keys_in[t] : 0u;
        const uint32_t d = digit_of(key, shift);
        uint64_t peers = __ballot(live);  // the live lanes with this lane's digit
#pragma unroll
        for (uint32_t b = 0; b < kDigitBits; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank =  // the peers in lower lanes
            __builtin_amdgcn_mbcnt_hi((uint32_t)(peers >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)peers, 0u));
        const uint32_t pos = live ? wbase[w][d] + rank : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (live && rank == 0u) wbase[w][d] = pos + (uint32_t)__popcll(peers);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (live && pos < n) {  // pos < n whenever the table is this pass's; the test costs nothing
            idx_out[pos] = idx_in[t];
            if (!LAST) keys_out[pos] = key;
        }
    }
}

uint32_t tile_rows(const LaunchCfg& c) {
    if (c.rows <= 0) return kTileRowsDefault;
    return std::min<uint32_t>((uint32_t)c.rows, kTileRowsMax);
}

// the sort's own scratch over n keys: byte offsets from an 8-aligned start
struct SortLayout {
    uint64_t keys[2], idx[2], table, total;
};

SortLayout sort_layout(uint64_t n) {
    SortLayout w;
    const uint64_t tiles_max = (n + kBlock - 1) / kBlock;  // the smallest tile a tune can ask for
    w.keys[0] = 0;
    w.keys[1] = w.keys[0] + 4 * n;
    w.idx[0] = w.keys[1] + 4 * n;
    w.idx[1] = w.idx[0] + 4 * n;
    w.table = w.idx[1] + 4 * n;
    w.total = w.table + 4 * (uint64_t)kDigits * tiles_max;
    return w;
}

// launch_gro_ordered's own scratch comes first, the sort's behind it
uint64_t flow_sort_at(uint64_t n) { return (gro_work_bytes(n) + 7u) & ~7ull; }

}  // namespace

uint64_t flow_sort_bytes(uint64_t n) { return sort_layout(n).total; }

FlowSortWork flow_sort_work(void* work, uint64_t n) {
    const SortLayout L = sort_layout(n);
    uint8_t* w = static_cast<uint8_t*>(work);
    return {{reinterpret_cast<uint32_t*>(w + L.keys[0]), reinterpret_cast<uint32_t*>(w + L.keys[1])},
            {reinterpret_cast<uint32_t*>(w + L.idx[0]), reinterpret_cast<uint32_t*>(w + L.idx[1])},
            reinterpret_cast<uint32_t*>(w + L.table)};
}

uint64_t gro_flow_work_bytes(uint64_t n) {
    return flow_sort_at(n) + flow_sort_bytes(n) + 8;  // + the rounding of the caller's pointer
}

hipError_t launch_gro_flow(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n64,
                           const uint64_t* valid, uint32_t* d_order, const GroOut& o, void* work, hipStream_t st) {
    const uint32_t n = (uint32_t)n64;  // n < 2^32 - 1 (csum_api.cpp)
    uint8_t* w = reinterpret_cast<uint8_t*>(((uintptr_t)work + 7u) & ~(uintptr_t)7u);
    if (n) {
        const FlowSortWork S = flow_sort_work(w + flow_sort_at(n), n);
        const uint8_t* base = static_cast<const uint8_t*>(d_base);
        const uint32_t kgrid = (uint32_t)(((uint64_t)n + kBlock - 1) / kBlock);
        if (ipver == 6)
            hipLaunchKernelGGL(flow_key_kernel<true>, dim3(kgrid), dim3(kBlock), 0, st, base, d_offsets, n, valid,
                               S.keys[0], S.idx[0]);
        else
            hipLaunchKernelGGL(flow_key_kernel<false>, dim3(kgrid), dim3(kBlock), 0, st, base, d_offsets, n, valid,
                               S.keys[0], S.idx[0]);
        const hipError_t e = launch_flow_sort(c, n, S, d_order, st);
        if (e != hipSuccess) return e;
    }
    return launch_gro_ordered(c, ipver, d_base, d_offsets, n64, valid, d_order, o, w, st);
}

// The hist / scan / scatter loop: S.keys[0] / S.idx[0] hold the keys and the identity index of n >= 1 frames.
// (Defined behind its first caller: the kernels are instantiated, and so laid out in the code object, in the order
// they always were.)
hipError_t launch_flow_sort(const LaunchCfg& c, uint32_t n, const FlowSortWork& S, uint32_t* d_order, hipStream_t st) {
    const uint32_t rows = tile_rows(c), tile_keys = rows * kBlock;
    const uint32_t ntiles = (uint32_t)(((uint64_t)n + tile_keys - 1) / tile_keys);
    const uint64_t entries = (uint64_t)kDigits * ntiles;
    for (uint32_t p = 0; p < kPasses; ++p) {
        const uint32_t shift = p * kDigitBits, a = p & 1u, b = a ^ 1u;
        hipLaunchKernelGGL(flow_hist_kernel, dim3(ntiles), dim3(kBlock), 0, st, S.keys[a], n, tile_keys, shift, ntiles,
                           S.table);
        hipLaunchKernelGGL(flow_scan_kernel, dim3(1), dim3(kBlock), 0, st, S.table, entries);
        if (p + 1 < kPasses)
            hipLaunchKernelGGL(flow_scatter_kernel<false>, dim3(ntiles), dim3(kBlock), 0, st, S.keys[a], S.idx[a], n,
                               rows, shift, ntiles, S.table, S.keys[b], S.idx[b]);
        else
            hipLaunchKernelGGL(flow_scatter_kernel<true>, dim3(ntiles), dim3(kBlock), 0, st, S.keys[a], S.idx[a], n,
                               rows, shift, ntiles, S.table, S.keys[b], d_order);
    }
    return hipGetLastError();
}

}  // namespace nsx
