// udp_api.cpp — the C ABI of the UDP passes (include/nsx_csum.h nsx_udp_*_dev, include/nsx_udp_tune.h their _tuned
// twins): everything validated on the host, then the one launch of udp_kernels.hip. The two layout helpers are in
// host_plan.cpp (no HIP). A file of its own, as nat_api.cpp: the CPU build of the host driver links csum_api.cpp
// against stand-ins for the launchers of the checksum families only, and UDP has no host forms.
#include <hip/hip_runtime_api.h>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_udp_tune.h"
#include "api_util.h"
#include "csum_kernels.h"
#include "host_plan.h"

namespace {

bool udp_hdr_ok(const nsx_udp_hdr_soa* u) { return u && u->src_port && u->dst_port; }
// NSX_UDP_NO_CSUM on IPv4 and nothing else
bool flags_ok(int ipver, uint32_t flags) { return !(flags & ~(ipver == 4 ? NSX_UDP_NO_CSUM : 0u)); }

// uso: the segmentation call (n super-datagrams, n_frames frames), else n == n_frames frames
int build_dev(int ipver, bool uso, const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
              const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso, uint64_t n,
              const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames, uint32_t flags,
              uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw, nsx_stream_t stream,
              const nsx_tune* tune) {
    if (!flags_ok(ipver, flags)) return NSX_EINVAL;
    if (n_frames == 0) return NSX_OK;
    if (!nsx::ip_hdr_ok(ip) || !udp_hdr_ok(udp) || !d_data_off || !d_out || !d_out_off || (data_bytes && !d_data))
        return NSX_EINVAL;
    if (uso && (n == 0 || n >= (1ull << 32) || n_frames < n || !d_gso || !d_frame_first || !d_frame_seg))
        return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    const nsx::UdpUsoMap m{d_gso, d_frame_first, d_frame_seg};
    return nsx::map_err(nsx::launch_udp_build(nsx::launch_cfg(nsx::device_cus(dev), tune), ipver, nsx::to_soa(*ip),
                                              udp->src_port, udp->dst_port, uso ? &m : nullptr, n, d_data, d_data_off,
                                              data_bytes, n_frames, flags & NSX_UDP_NO_CSUM, d_out, d_out_off,
                                              d_udp_raw, static_cast<hipStream_t>(stream)));
}

int rx_dev(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask, uint16_t* d_ip_raw,
           uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune) {
    if (n == 0) return NSX_OK;
    if (!d_base || !d_offsets || !d_mask || n > ((uint64_t)1 << 40)) return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    return nsx::map_err(nsx::launch_udp_rx(nsx::launch_cfg(nsx::device_cus(dev), tune), ipver, d_base, d_offsets, n,
                                           d_mask, d_ip_raw, d_udp_raw, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

#define NSX_UDP_DEV(V)                                                                                              \
    int nsx_udp_tx_ipv##V##_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,  \
                                      const uint64_t* d_data_off, uint64_t data_bytes, uint64_t n, uint32_t flags,  \
                                      uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw,               \
                                      nsx_stream_t stream) {                                                        \
        return build_dev(V, false, ip, udp, d_data, d_data_off, data_bytes, nullptr, n, nullptr, nullptr, n, flags, \
                         d_out, d_out_off, d_udp_raw, stream, nullptr);                                             \
    }                                                                                                               \
    int nsx_udp_tx_ipv##V##_build_dev_tuned(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp,                   \
                                            const uint8_t* d_data, const uint64_t* d_data_off, uint64_t data_bytes, \
                                            uint64_t n, uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,  \
                                            uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune) {       \
        return build_dev(V, false, ip, udp, d_data, d_data_off, data_bytes, nullptr, n, nullptr, nullptr, n, flags, \
                         d_out, d_out_off, d_udp_raw, stream, tune);                                                \
    }                                                                                                               \
    int nsx_udp_uso_ipv##V##_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data, \
                                       const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso,      \
                                       uint64_t n, const uint64_t* d_frame_first, const uint32_t* d_frame_seg,      \
                                       uint64_t n_frames, uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off, \
                                       uint16_t* d_udp_raw, nsx_stream_t stream) {                                  \
        return build_dev(V, true, ip, udp, d_data, d_data_off, data_bytes, d_gso, n, d_frame_first, d_frame_seg,    \
                         n_frames, flags, d_out, d_out_off, d_udp_raw, stream, nullptr);                            \
    }                                                                                                               \
    int nsx_udp_uso_ipv##V##_build_dev_tuned(                                                                       \
        const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data, const uint64_t* d_data_off,    \
        uint64_t data_bytes, const uint32_t* d_gso, uint64_t n, const uint64_t* d_frame_first,                      \
        const uint32_t* d_frame_seg, uint64_t n_frames, uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off,  \
        uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune) {                                           \
        return build_dev(V, true, ip, udp, d_data, d_data_off, data_bytes, d_gso, n, d_frame_first, d_frame_seg,    \
                         n_frames, flags, d_out, d_out_off, d_udp_raw, stream, tune);                               \
    }
NSX_UDP_DEV(4)
NSX_UDP_DEV(6)
#undef NSX_UDP_DEV

int nsx_udp_rx_ipv4_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_ip_raw, uint16_t* d_udp_raw, nsx_stream_t stream) {
    return rx_dev(4, d_base, d_offsets, n, d_mask, d_ip_raw, d_udp_raw, stream, nullptr);
}

int nsx_udp_rx_ipv4_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                     uint16_t* d_ip_raw, uint16_t* d_udp_raw, nsx_stream_t stream,
                                     const nsx_tune* tune) {
    return rx_dev(4, d_base, d_offsets, n, d_mask, d_ip_raw, d_udp_raw, stream, tune);
}

int nsx_udp_rx_ipv6_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_udp_raw, nsx_stream_t stream) {
    return rx_dev(6, d_base, d_offsets, n, d_mask, nullptr, d_udp_raw, stream, nullptr);
}

int nsx_udp_rx_ipv6_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                     uint16_t* d_udp_raw, nsx_stream_t stream, const nsx_tune* tune) {
    return rx_dev(6, d_base, d_offsets, n, d_mask, nullptr, d_udp_raw, stream, tune);
}

}  // extern "C"
