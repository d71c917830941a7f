// ugro_api.cpp — the C ABI of UDP receive coalescing (include/nsx_csum.h nsx_ugro_*, include/nsx_ugro_tune.h the
// _tuned twins): everything validated on the host, then the launches of ugro_kernels.hip (the flow-keyed calls: its
// key pass and the radix sort of gro_flow_kernels.hip before them). A file of its own, as udp_api.cpp and nat_api.cpp:
// the CPU build of the host driver links csum_api.cpp against stand-ins for the launchers of the checksum families
// only, and these calls have no host forms.
#include <hip/hip_runtime_api.h>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_ugro_tune.h"
#include "api_util.h"
#include "csum_kernels.h"

namespace {

// flow: the flow-keyed call (d_order an output), else coalescing by adjacency
int ugro_dev(int ipver, bool flow, const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
             uint32_t* d_order, const nsx_ugro_out* o, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
             const nsx_tune* tune) {
    // an empty batch has no frame bytes, no mask words and no order
    if ((n && (!d_base || !d_valid)) || !d_offsets || !d_work || !o || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    if (flow && n && !d_order) return NSX_EINVAL;
    if (!o->n_super || !o->src || !o->dst || !o->ident || !o->ttl || !o->tclass || !o->flow || !o->src_port ||
        !o->dst_port || !o->gso || !o->data || !o->data_off || !o->first_frame || !o->frame_cnt || !o->frame_seg)
        return NSX_EINVAL;
    if (work_bytes < (flow ? nsx::ugro_flow_work_bytes(n) : nsx::ugro_work_bytes(n))) return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    const nsx::UgroOut g{o->n_super, o->src,      o->dst,      o->ident, o->ttl,  o->tclass,   o->flow,        o->src_port,
                         o->dst_port, o->gso,     o->data,     o->data_off, o->first_frame, o->frame_cnt, o->frame_seg};
    const nsx::LaunchCfg c = nsx::launch_cfg(nsx::device_cus(dev), tune);
    if (flow)
        return nsx::map_err(nsx::launch_ugro_flow(c, ipver, d_base, d_offsets, n, d_valid, d_order, g, d_work,
                                                  static_cast<hipStream_t>(stream)));
    return nsx::map_err(
        nsx::launch_ugro(c, ipver, d_base, d_offsets, n, d_valid, g, d_work, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nsx_ugro_work_bytes(uint64_t n, uint64_t* out) {
    if (!out || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    *out = nsx::ugro_work_bytes(n);
    return NSX_OK;
}

int nsx_ugro_flow_work_bytes(uint64_t n, uint64_t* out) {
    if (!out || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    *out = nsx::ugro_flow_work_bytes(n);
    return NSX_OK;
}

#define NSX_UGRO_DEV(V)                                                                                              \
    int nsx_ugro_ipv##V##_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,    \
                              const nsx_ugro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream) {     \
        return ugro_dev(V, false, d_base, d_offsets, n, d_valid, nullptr, out, d_work, work_bytes, stream, nullptr); \
    }                                                                                                                \
    int nsx_ugro_ipv##V##_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n,                       \
                                    const uint64_t* d_valid, const nsx_ugro_out* out, void* d_work,                  \
                                    uint64_t work_bytes, nsx_stream_t stream, const nsx_tune* tune) {                \
        return ugro_dev(V, false, d_base, d_offsets, n, d_valid, nullptr, out, d_work, work_bytes, stream, tune);    \
    }                                                                                                                \
    int nsx_ugro_flow_ipv##V##_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n,                        \
                                   const uint64_t* d_valid, uint32_t* d_order, const nsx_ugro_out* out,              \
                                   void* d_work, uint64_t work_bytes, nsx_stream_t stream) {                         \
        return ugro_dev(V, true, d_base, d_offsets, n, d_valid, d_order, out, d_work, work_bytes, stream, nullptr);  \
    }                                                                                                                \
    int nsx_ugro_flow_ipv##V##_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n,                  \
                                         const uint64_t* d_valid, uint32_t* d_order, const nsx_ugro_out* out,        \
                                         void* d_work, uint64_t work_bytes, nsx_stream_t stream,                     \
                                         const nsx_tune* tune) {                                                     \
        return ugro_dev(V, true, d_base, d_offsets, n, d_valid, d_order, out, d_work, work_bytes, stream, tune);     \
    }
NSX_UGRO_DEV(4)
NSX_UGRO_DEV(6)
#undef NSX_UGRO_DEV

}  // extern "C"
