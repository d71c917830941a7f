/* nsx_tx_tune.h — the _tuned twins of the fused transmit pass (nsx_csum.h: nsx_tx_ipv4_tcp_build_dev and
 * friends). Part of nsx_tune.h, which includes it: include that header. They reuse nsx_tune unchanged, and its
 * fields mean what they mean for the TCP build: kernel = NSX_TUNE_KERNEL_BUILD_PLAIN or _BUILD_GENERAL, run_segs
 * 1..64 frames per wave task, xcd_chunk, blocks_per_cu; for the host calls also shards_per_device and chunk_bytes
 * (which every host call honours, nsx_tune.h).
 * tune NULL = the product call. The twins of segmentation offload (nsx_tso_*) follow them. */
#ifndef NSX_TX_TUNE_H
#define NSX_TX_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_tx_ipv4_tcp_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                                    const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                                    uint64_t data_bytes, uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                    uint16_t* d_tcp_raw, nsx_stream_t stream, const nsx_tune* tune);
int nsx_tx_ipv6_tcp_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                                    const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                                    uint64_t data_bytes, uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                                    uint16_t* d_tcp_raw, nsx_stream_t stream, const nsx_tune* tune);
int nsx_tx_ipv4_tcp_build_host_tuned(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                     const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                     uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_tcp_raw,
                                     int num_gpus, const nsx_tune* tune);
int nsx_tx_ipv6_tcp_build_host_tuned(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                     const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                     uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_tcp_raw,
                                     int num_gpus, const nsx_tune* tune);

/* Segmentation offload (nsx_tso_*): run_segs counts frames per wave task; its host calls honour chunk_bytes too. */
int nsx_tso_ipv4_tcp_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                                     const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                                     uint64_t data_bytes, const uint32_t* d_mss, uint64_t n,
                                     const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                                     uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_tcp_raw,
                                     nsx_stream_t stream, const nsx_tune* tune);
int nsx_tso_ipv6_tcp_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                                     const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                                     uint64_t data_bytes, const uint32_t* d_mss, uint64_t n,
                                     const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                                     uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_tcp_raw,
                                     nsx_stream_t stream, const nsx_tune* tune);
int nsx_tso_ipv4_tcp_build_host_tuned(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                      const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                      const uint32_t* h_mss, uint64_t n, const uint64_t* h_frame_first,
                                      const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,
                                      const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus,
                                      const nsx_tune* tune);
int nsx_tso_ipv6_tcp_build_host_tuned(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                      const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                      const uint32_t* h_mss, uint64_t n, const uint64_t* h_frame_first,
                                      const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,
                                      const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus,
                                      const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_TX_TUNE_H */
