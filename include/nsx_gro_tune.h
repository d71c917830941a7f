/* nsx_gro_tune.h — the _tuned twins of receive coalescing (nsx_csum.h: nsx_gro_ipv4_tcp_dev / nsx_gro_ipv6_tcp_dev
 * and the flow-keyed nsx_gro_flow_ipv4_tcp_dev / nsx_gro_flow_ipv6_tcp_dev).
 * Part of nsx_tune.h, which includes it: include that header. They reuse nsx_tune unchanged: run_segs = frames per
 * scan block of the prefix sums (0 = 4096; clamped to 16..65536 — tests reach the multi-block scan with a few
 * hundred frames), blocks_per_cu = the grid of the copy kernel (1..8 blocks of 256 threads per CU, default 8).
 * For the flow-keyed calls rows gains a meaning: keys per tile of the radix sort in units of 256 (0 = the default,
 * 16; 1..64 valid, a larger value is taken as 64) — with rows = 1 a few hundred frames span several tiles.
 * nsx_gro_* ignores rows. The other fields are ignored. tune NULL = the product call. nsx_gro_work_bytes and
 * nsx_gro_flow_work_bytes cover every setting. */
#ifndef NSX_GRO_TUNE_H
#define NSX_GRO_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_gro_ipv4_tcp_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                               const nsx_gro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                               const nsx_tune* tune);
int nsx_gro_ipv6_tcp_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                               const nsx_gro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                               const nsx_tune* tune);

/* the flow-keyed calls (declared as in nsx_csum.h, the return type on a line of its own) */
int
nsx_gro_flow_ipv4_tcp_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                uint32_t* d_order, const nsx_gro_out* out, void* d_work, uint64_t work_bytes,
                                nsx_stream_t stream, const nsx_tune* tune);
int
nsx_gro_flow_ipv6_tcp_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                uint32_t* d_order, const nsx_gro_out* out, void* d_work, uint64_t work_bytes,
                                nsx_stream_t stream, const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_GRO_TUNE_H */
