/* nsx_ugro_tune.h — the _tuned twins of UDP receive coalescing (nsx_csum.h: nsx_ugro_ipv4_dev / nsx_ugro_ipv6_dev
 * and the flow-keyed nsx_ugro_flow_ipv4_dev / nsx_ugro_flow_ipv6_dev), for benchmarks and tests. Not part of
 * nsx_tune.h: include this header, which brings that one in. The twins reuse nsx_tune unchanged, with the meanings
 * the TCP calls give the same fields:
 *   run_segs       frames per scan block of the prefix sums (0 = 4096; clamped to 16..65536 — tests reach the
 *                  multi-block scan with a few hundred frames).
 *   blocks_per_cu  the grid of the copy kernel: 1..8 blocks of 256 threads per CU (default 8), never more blocks
 *                  than the batch has wave tasks.
 *   rows           the flow-keyed calls only: keys per tile of the radix sort in units of 256 (0 = the default, 16;
 *                  1..64 valid, a larger value is taken as 64). nsx_ugro_ipvX_dev ignores it.
 * Every other field is ignored. Every setting is bit-exact. tune NULL = the product call. nsx_ugro_work_bytes and
 * nsx_ugro_flow_work_bytes cover every setting. */
#ifndef NSX_UGRO_TUNE_H
#define NSX_UGRO_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_ugro_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                            const nsx_ugro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                            const nsx_tune* tune);
int nsx_ugro_ipv6_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                            const nsx_ugro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                            const nsx_tune* tune);
int nsx_ugro_flow_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 uint32_t* d_order, const nsx_ugro_out* out, void* d_work, uint64_t work_bytes,
                                 nsx_stream_t stream, const nsx_tune* tune);
int nsx_ugro_flow_ipv6_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 uint32_t* d_order, const nsx_ugro_out* out, void* d_work, uint64_t work_bytes,
                                 nsx_stream_t stream, const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_UGRO_TUNE_H */
