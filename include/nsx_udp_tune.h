/* nsx_udp_tune.h — the _tuned twins of the UDP passes (nsx_csum.h: nsx_udp_tx_*, nsx_udp_uso_*, nsx_udp_rx_*), for
 * benchmarks and tests. Not part of nsx_tune.h: include this header, which brings that one in. The twins reuse
 * nsx_tune unchanged; two of its fields are read, every other is ignored:
 *   blocks_per_cu  the grid: 1..8 blocks of 256 threads per CU (default 4 for transmit and segmentation, 8 for
 *                  receive), never more blocks than the batch has wave tasks.
 *   run_segs       transmit and segmentation: 1..64 frames per wave task (default: up to 16, fewer for long frames
 *                  and small batches). Receive: a wave task is always one 64-frame mask word; run_segs is the 1..64
 *                  frames whose headers the wave's lanes read per step of it (default 16).
 * Every setting is bit-exact. tune NULL = the product call. */
#ifndef NSX_UDP_TUNE_H
#define NSX_UDP_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_udp_tx_ipv4_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                                    const uint64_t* d_data_off, uint64_t data_bytes, uint64_t n, uint32_t flags,
                                    uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw,
                                    nsx_stream_t stream, const nsx_tune* tune);
int nsx_udp_tx_ipv6_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                                    const uint64_t* d_data_off, uint64_t data_bytes, uint64_t n, uint32_t flags,
                                    uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw,
                                    nsx_stream_t stream, const nsx_tune* tune);
int nsx_udp_uso_ipv4_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                                     const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso,
                                     uint64_t n, const uint64_t* d_frame_first, const uint32_t* d_frame_seg,
                                     uint64_t n_frames, uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,
                                     uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune);
int nsx_udp_uso_ipv6_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                                     const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso,
                                     uint64_t n, const uint64_t* d_frame_first, const uint32_t* d_frame_seg,
                                     uint64_t n_frames, uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,
                                     uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune);
int nsx_udp_rx_ipv4_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                     uint16_t* d_ip_raw, uint16_t* d_udp_raw, nsx_stream_t stream,
                                     const nsx_tune* tune);
int nsx_udp_rx_ipv6_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                     uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_UDP_TUNE_H */
