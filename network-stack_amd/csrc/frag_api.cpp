// frag_api.cpp — the C ABI of IPv4 fragmentation and reassembly (include/nsx_csum.h nsx_frag_ipv4_dev and nsx_reasm_*,
// include/nsx_frag_tune.h the _tuned twins): everything validated on the host, then the launches of frag_kernels.hip.
// A file of its own, as ugro_api.cpp: these calls have no host forms. The frame map's host helpers
// (nsx_frag_count_host, nsx_frag_layout_host) are in host_plan.cpp, which stays free of HIP.
#include <hip/hip_runtime_api.h>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_frag_tune.h"
#include "api_util.h"
#include "csum_kernels.h"

namespace {

int frag_dev(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu, uint64_t n,
             const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags, uint8_t* d_out,
             const uint64_t* d_out_off, uint8_t* d_status, nsx_stream_t stream, const nsx_tune* tune) {
    // every frame has a slot: an empty batch has no slots, and only an empty batch has none
    if (n >= (1ull << 32) || n_frags < n || (n == 0 && n_frags)) return NSX_EINVAL;
    if (n && (!d_base || !d_offsets || !d_mtu || !d_frag_first || !d_frag_src || !d_out || !d_out_off || !d_status))
        return NSX_EINVAL;
    if (n_frags == 0) return NSX_OK;  // nothing to launch: no device is looked for
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    const nsx::LaunchCfg c = nsx::launch_cfg(nsx::device_cus(dev), tune);
    return nsx::map_err(nsx::launch_frag(c, d_base, d_offsets, d_mtu, n, d_frag_first, d_frag_src, n_frags, d_out,
                                         d_out_off, d_status, static_cast<hipStream_t>(stream)));
}

int reasm_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order, const nsx_reasm_out* o,
              void* d_work, uint64_t work_bytes, nsx_stream_t stream, const nsx_tune* tune) {
    // an empty batch has no frame bytes and no order
    if ((n && (!d_base || !d_order)) || !d_offsets || !d_work || !o || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    if (!o->n_out || !o->out || !o->out_off || !o->first_pos || !o->frag_cnt || !o->frame_seg || !o->is_frag)
        return NSX_EINVAL;
    if (work_bytes < nsx::reasm_work_bytes(n)) return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    const nsx::ReasmDevOut g{o->n_out, o->out, o->out_off, o->first_pos, o->frag_cnt, o->frame_seg, o->is_frag};
    const nsx::LaunchCfg c = nsx::launch_cfg(nsx::device_cus(dev), tune);
    return nsx::map_err(
        nsx::launch_reasm(c, d_base, d_offsets, n, d_order, g, d_work, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nsx_frag_ipv4_dev(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu, uint64_t n,
                      const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags, uint8_t* d_out,
                      const uint64_t* d_out_off, uint8_t* d_status, nsx_stream_t stream) {
    return frag_dev(d_base, d_offsets, d_mtu, n, d_frag_first, d_frag_src, n_frags, d_out, d_out_off, d_status, stream,
                    nullptr);
}

int nsx_frag_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu, uint64_t n,
                            const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags, uint8_t* d_out,
                            const uint64_t* d_out_off, uint8_t* d_status, nsx_stream_t stream, const nsx_tune* tune) {
    return frag_dev(d_base, d_offsets, d_mtu, n, d_frag_first, d_frag_src, n_frags, d_out, d_out_off, d_status, stream,
                    tune);
}

int nsx_reasm_work_bytes(uint64_t n, uint64_t* out) {
    if (!out || n >= 0xFFFFFFFFull) return NSX_EINVAL;
    *out = nsx::reasm_work_bytes(n);
    return NSX_OK;
}

int nsx_reasm_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                       const nsx_reasm_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream) {
    return reasm_dev(d_base, d_offsets, n, d_order, out, d_work, work_bytes, stream, nullptr);
}

int nsx_reasm_ipv4_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                             const nsx_reasm_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream,
                             const nsx_tune* tune) {
    return reasm_dev(d_base, d_offsets, n, d_order, out, d_work, work_bytes, stream, tune);
}

}  // extern "C"
