// nat_api.cpp — the C ABI of the in-place NAT rewrite (include/nsx_csum.h nsx_nat_*_tcp_rewrite_dev): everything
// validated on the host, then the one launch of nat_kernels.hip. The table is built by nsx_nat_table_build_host
// (host_plan.cpp, no HIP). A file of its own so that csum_api.cpp keeps referring to the launchers of the checksum
// families only.
#include <hip/hip_runtime_api.h>

#include "../../include/nsx_csum.h"
#include "api_util.h"
#include "csum_kernels.h"
#include "host_plan.h"

static int nat_dev(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                   const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit, nsx_stream_t stream) {
    // an empty batch has no frame bytes and no mask words
    if ((n && (!d_base || !d_valid || !d_hit)) || !d_offsets || !d_table || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    if (!nsx::nat_slots_ok(slots) || ((uintptr_t)d_table & 15u) || ttl_dec > 255u) return NSX_EINVAL;
    if (nsx::current_device() < 0) return NSX_ENODEV;
    return nsx::map_err(nsx::launch_nat_rewrite(ipver, d_base, d_offsets, n, d_valid, d_table, slots, ttl_dec, d_hit,
                                                static_cast<hipStream_t>(stream)));
}

extern "C" {

int nsx_nat_ipv4_tcp_rewrite_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit,
                                 nsx_stream_t stream) {
    return nat_dev(4, d_base, d_offsets, n, d_valid, d_table, slots, ttl_dec, d_hit, stream);
}

int nsx_nat_ipv6_tcp_rewrite_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit,
                                 nsx_stream_t stream) {
    return nat_dev(6, d_base, d_offsets, n, d_valid, d_table, slots, ttl_dec, d_hit, stream);
}

}  // extern "C"
