// icmp_kernels.h — internal launcher interface between icmp_api.cpp and icmp_kernels.hip (nsx_icmp_*,
// include/nsx_csum.h). A header of its own, so that csum_kernels.h — which every existing kernel file includes —
// stays as it is. Not a public header.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "csum_kernels.h"

namespace nsx {

// nsx_icmp_err_cfg as the kernels take it: our address as little-endian dwords (IPv4: src[0] only).
struct IcmpErrCfg {
    uint32_t src[4];
    uint32_t ttl, ident0;
    uint64_t max_out;
};
// The writable device arrays of include/nsx_csum.h nsx_icmp_err_out, member for member.
struct IcmpErrOut {
    uint64_t* n_out;
    uint8_t* out;
    uint64_t* out_off;
    uint32_t* src_frame;
    uint8_t* status;
};
// Scratch bytes of one launch_icmp_err over n frames (whatever the tune).
uint64_t icmp_err_work_bytes(uint64_t n);
// Plan (status, message length, block sums), the sums' prefix, apply (rank, offsets, SENT / LIMITED), emit: one
// serial chain of four launches; n == 0: the sums kernel alone, which writes *n_out = 0 and out_off[0] = 0.
// n < 2^32 - 1, work of at least icmp_err_work_bytes(n), cfg.ttl <= 255 (icmp_api.cpp checks all of it). arg
// nullable. c.run_segs = frames per scan block (0 = 4096, clamped to 16..65536), c.blocks_per_cu = the emit kernel's
// grid (default 8).
hipError_t launch_icmp_err(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                           const uint32_t* req, const uint32_t* arg, const IcmpErrCfg& cfg, const IcmpErrOut& o,
                           void* work, hipStream_t st);
// The request helpers: one launch each, a lane per frame; none for n == 0.
hipError_t launch_icmp_req_frag(const uint8_t* status, const uint32_t* mtu, uint64_t n, uint32_t* req, uint32_t* arg,
                                hipStream_t st);
hipError_t launch_icmp_req_ttl(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                               const uint64_t* valid, uint32_t ttl_dec, uint32_t* req, uint32_t* arg, hipStream_t st);
// The ICMP receive verify: a wave per 64-frame mask word, statically split, as launch_udp_rx; c.run_segs = frames per
// metadata step (1..64, default 16), c.blocks_per_cu the grid (default 8). ip_raw (IPv4 only) / icmp_raw / type
// nullable.
hipError_t launch_icmp_rx(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                          uint64_t* mask, uint16_t* ip_raw, uint16_t* icmp_raw, uint16_t* type, hipStream_t st);
// The in-place echo reply: one launch, a lane per frame; none for n == 0. ttl <= 255.
hipError_t launch_icmp_echo(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* valid,
                            uint32_t ttl, uint64_t* d_hit, hipStream_t st);

}  // namespace nsx
