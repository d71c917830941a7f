// kernel_util.h — device helpers shared by the kernel files (csum_kernels.hip, gro_kernels.hip,
// gro_flow_kernels.hip, nat_kernels.hip): the wave / row constants, the 16-byte chunk type, buffer descriptors and their 16-byte
// loads, byte masks, the v_alignbyte realignment, and receive coalescing's clamped frame window (FrameWin) and
// membership test. Everything is __forceinline__ in an unnamed namespace, so each kernel file gets its own copies and
// the code generated for a kernel does not depend on which file defines the helper
// (profiles/gro_kernels_vs_parent.txt). Not a public header; device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsx {
namespace {

constexpr uint32_t kWave = 64;
constexpr uint32_t kRow = 1024;        // bytes per wave-wide 16 B/lane load
constexpr uint32_t kBlock = 256;       // 4 waves
constexpr uint32_t kWavesPerBlock = kBlock / kWave;

// 16 bytes at a 4-byte-aligned address: hipcc emits one global_load_dwordx4
// (gfx950 serves dword-aligned multi-dword global loads in hardware).
typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// Mask for the chunk of lane byte offset ql inside a row whose segment bytes are
// [lo_r, hi_r) relative to the row start (both clamped, 32-bit).
__device__ __forceinline__ uint32_t keep_mask(int32_t lo_r, int32_t hi_r, int32_t d) {
    const int32_t e = min(max(hi_r - d, 0), 4), s = min(max(lo_r - d, 0), 4);
    const uint32_t me = e >= 4 ? 0xFFFFFFFFu : ((1u << (8 * e)) - 1u);
    const uint32_t ms = s >= 4 ? 0xFFFFFFFFu : ((1u << (8 * s)) - 1u);
    return me & ~ms;
}

constexpr uint32_t kOOB = 0x80000000u;  // voffset that is always out of range (num_records < 2^31)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, uint64_t bytes) {
    // Wave-uniform inputs only, so no waterfall loop (guide T20); clamp without a
    // 64-bit unsigned compare (SALU has none: hipcc would borrow VGPRs for it).
    const uint32_t nr = (bytes >> 31) ? kOOB - 1 : (uint32_t)bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)nr, 0x00020000);
}

template <bool NT>
__device__ __forceinline__ u32x4 bld16(__amdgpu_buffer_rsrc_t r, uint32_t voff) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    v4u x = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, NT ? 2 : 0);
    return u32x4{x.x, x.y, x.z, x.w};
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t k) {
    const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)v, k);
    const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(v >> 32), k);
    return ((uint64_t)hi << 32) | lo;
}

// Keep bytes [lo, hi) (0 ≤ lo ≤ hi ≤ 16) of a 16-byte chunk.
__device__ __forceinline__ u32x4 keep_bytes(u32x4 x, int32_t lo, int32_t hi) {
    x.x &= keep_mask(lo, hi, 0);
    x.y &= keep_mask(lo, hi, 4);
    x.z &= keep_mask(lo, hi, 8);
    x.w &= keep_mask(lo, hi, 12);
    return x;
}

__device__ __forceinline__ uint32_t bperm(uint32_t v, uint32_t src_lane) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(src_lane * 4), (int)v);
}

// Five source dwords (lo, hi) shifted down by sh bytes: the 16 bytes that start sh bytes into lo.
__device__ __forceinline__ u32x4 realign(u32x4 lo, uint32_t hi, uint32_t sh) {
    return u32x4{__builtin_amdgcn_alignbyte(lo.y, lo.x, sh), __builtin_amdgcn_alignbyte(lo.z, lo.y, sh),
                 __builtin_amdgcn_alignbyte(lo.w, lo.z, sh), __builtin_amdgcn_alignbyte(hi, lo.w, sh)};
}

__device__ __forceinline__ uint32_t bswap16(uint32_t v) { return ((v & 0xFFu) << 8) | ((v >> 8) & 0xFFu); }
__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

// A frame's bytes as dwords: the window starts at the frame's address rounded down to 4 bytes; a dword that
// holds no byte of the frame is not loaded and reads 0 (an aligned dword holding a readable byte never crosses a
// page). at(b): the little-endian dword at frame byte b (a multiple of 4).
struct FrameWin {
    const uint32_t* w;
    uint32_t sh, end;  // frame start inside the first dword; window bytes up to the frame's end
    __device__ __forceinline__ uint32_t word(uint32_t k) const { return 4u * k < end ? w[k] : 0u; }
    __device__ __forceinline__ uint32_t at(uint32_t b) const {
        const uint32_t k = b >> 2;
        return __builtin_amdgcn_alignbyte(word(k + 1), word(k), sh);
    }
};

__device__ __forceinline__ FrameWin frame_win(const uint8_t* p, uint32_t flen) {
    const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
    return FrameWin{reinterpret_cast<const uint32_t*>(p - sh), sh, flen ? sh + flen : 0u};
}

// Well-formed as the receive pass of the IP version defines (include/nsx_csum.h: length, version, protocol and
// fragment conditions), from the frame's length and its header dwords 0, 1 and 2 (h2: IPv4 only); iph = the IP
// header's bytes, seg = the TCP segment's. One half of receive coalescing's membership test as the key pass of
// gro_flow_kernels.hip makes it; the other is tcp_doff_fits below, on dword 3 of the TCP header. (The head pass of
// gro_kernels.hip has the same conditions written out: see there.)
template <bool V6>
__device__ __forceinline__ bool frame_wellformed(uint32_t h0, uint32_t h1, uint32_t h2, uint32_t flen, uint32_t& iph,
                                                 uint32_t& seg) {
    bool ok;
    if constexpr (V6) {
        iph = 40u;
        ok = flen >= 60u && (h0 & 0xF0u) == 0x60u && 40u + bswap16(h1) == flen && ((h1 >> 16) & 0xFFu) == 6u;
        seg = flen - 40u;
    } else {
        iph = (h0 & 15u) * 4u;
        ok = flen >= 40u && (h0 & 0xF0u) == 0x40u && iph >= 20u && iph <= flen && bswap16(h0 >> 16) == flen &&
             (h1 & 0xFF3F0000u) == 0u && ((h2 >> 8) & 0xFFu) == 6u && flen - iph >= 20u;
        seg = flen - iph;
    }
    return ok;
}

// 5 <= doff and doff*4 <= segment length, doff from TCP header dword 3 (bytes 12-15)
__device__ __forceinline__ bool tcp_doff_fits(uint32_t t3, uint32_t seg) {
    const uint32_t doff = (t3 >> 4) & 15u;
    return doff >= 5u && doff * 4u <= seg;
}

}  // namespace
}  // namespace nsx
