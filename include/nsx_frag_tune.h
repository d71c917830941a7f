/* nsx_frag_tune.h — the _tuned twins of IPv4 fragmentation and reassembly (nsx_csum.h: nsx_frag_ipv4_dev and
 * nsx_reasm_ipv4_dev), for benchmarks and tests. Not part of nsx_tune.h: include this header, which brings that one
 * in. The twins reuse nsx_tune unchanged, with the meanings the coalescing calls give the same fields:
 *   blocks_per_cu  the grid of the copy kernel: 1..8 blocks of 256 threads per CU (default 8), never more blocks
 *                  than the batch has wave tasks (16 output slots, or 16 positions of the order, each).
 *   run_segs       reassembly only: frames per scan block of the prefix sums (0 = 4096; clamped to 16..65536).
 *   rows           reassembly only: keys per tile of the radix sort in units of 256 (0 = the default, 16; 1..64 valid,
 *                  a larger value is taken as 64).
 * Every other field is ignored. Every setting is bit-exact. tune NULL = the product call. nsx_reasm_work_bytes
 * covers every setting. */
#ifndef NSX_FRAG_TUNE_H
#define NSX_FRAG_TUNE_H

#include "nsx_tune.h"

#ifdef __cplusplus
extern "C" {
#endif

int nsx_frag_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu, uint64_t n,
                            const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags, uint8_t* d_out,
                            const uint64_t* d_out_off, uint8_t* d_status, nsx_stream_t stream, const nsx_tune* tune);
int nsx_reasm_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                             const nsx_reasm_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                             const nsx_tune* tune);

#ifdef __cplusplus
}
#endif
#endif /* NSX_FRAG_TUNE_H */
