/* nsx_icmp_tune.h — the _tuned twins of ICMP error generation and the ICMP receive verify (nsx_csum.h:
 * nsx_icmp_err_ipv4_dev / nsx_icmp_err_ipv6_dev and nsx_icmp_rx_ipv4_verify_dev / nsx_icmp_rx_ipv6_verify_dev), for
 * benchmarks and tests. Not part of nsx_tune.h: include this header, which brings that one in. The twins reuse
 * nsx_tune unchanged, with the meanings the other families give the same fields:
 *   blocks_per_cu  error generation: the grid of the emit kernel; verify: the grid. 1..8 blocks of 256 threads per
 *                  CU (default 8), never more blocks than the batch has wave tasks (16 messages, or 64 frames, each).
 *   run_segs       error generation: frames per scan block of the prefix sums (0 = 4096; clamped to 16..65536);
 *                  verify: frames per metadata step (1..64, default 16), as nsx_udp_rx_*_verify_dev_tuned.
 * Every other field is ignored. Every setting is bit-exact. tune NULL = the product call. nsx_icmp_err_work_bytes
 * covers every setting. The echo reply and the request helpers have no twins: one lane per frame, there is no launch
 * shape to override. */
#ifndef NSX_ICMP_TUNE_H
#define NSX_ICMP_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_icmp_err_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,
                                const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* out,
                                void* d_work, uint64_t work_bytes, nsx_stream_t stream, const nsx_tune* tune);
int nsx_icmp_err_ipv6_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,
                                const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* out,
                                void* d_work, uint64_t work_bytes, nsx_stream_t stream, const nsx_tune* tune);
int nsx_icmp_rx_ipv4_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                      uint16_t* d_ip_raw, uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream,
                                      const nsx_tune* tune);
int nsx_icmp_rx_ipv6_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                      uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream,
                                      const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_ICMP_TUNE_H */
