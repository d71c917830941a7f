// icmp_api.cpp — the C ABI of the ICMP family (include/nsx_csum.h nsx_icmp_*, include/nsx_icmp_tune.h the _tuned
// twins): everything validated on the host, then the launches of icmp_kernels.hip. A file of its own, as nat_api.cpp
// and frag_api.cpp: these calls have no host forms and no host-side planner.
#include <hip/hip_runtime_api.h>

#include <string.h>

#include "../../include/nsx_csum.h"
#include "../../include/nsx_icmp_tune.h"
#include "api_util.h"
#include "icmp_kernels.h"

namespace {

constexpr uint64_t kMaxFrames = 0xFFFFFFFFull;  // n >= 2^32 - 1 is refused

int err_dev(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,
            const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* o, void* d_work,
            uint64_t work_bytes, nsx_stream_t stream, const nsx_tune* tune) {
    // an empty batch has no frames and no requests; n_out and out_off are written all the same
    if (!cfg || !o || !o->n_out || !o->out_off || !d_work || n >= kMaxFrames) return NSX_EINVAL;
    if (n && (!d_base || !d_offsets || !d_req || !o->out || !o->src_frame || !o->status)) return NSX_EINVAL;
    if (cfg->ttl > 255u || work_bytes < nsx::icmp_err_work_bytes(n)) return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    nsx::IcmpErrCfg k;
    memcpy(k.src, cfg->src, 16);
    k.ttl = cfg->ttl;
    k.ident0 = cfg->ident0;
    k.max_out = cfg->max_out;
    const nsx::IcmpErrOut g{o->n_out, o->out, o->out_off, o->src_frame, o->status};
    const nsx::LaunchCfg c = nsx::launch_cfg(nsx::device_cus(dev), tune);
    return nsx::map_err(nsx::launch_icmp_err(c, ipver, d_base, d_offsets, n, d_req, d_arg, k, g, d_work,
                                             static_cast<hipStream_t>(stream)));
}

int req_ttl_dev(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                uint32_t ttl_dec, uint32_t* d_req, uint32_t* d_arg, nsx_stream_t stream) {
    if ((n && (!d_base || !d_offsets || !d_valid || !d_req || !d_arg)) || n >= kMaxFrames || ttl_dec > 255u)
        return NSX_EINVAL;
    if (nsx::current_device() < 0) return NSX_ENODEV;
    return nsx::map_err(nsx::launch_icmp_req_ttl(ipver, d_base, d_offsets, n, d_valid, ttl_dec, d_req, d_arg,
                                                 static_cast<hipStream_t>(stream)));
}

int rx_dev(int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask, uint16_t* d_ip_raw,
           uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream, const nsx_tune* tune) {
    if ((n && (!d_base || !d_offsets || !d_mask)) || n >= kMaxFrames) return NSX_EINVAL;
    const int dev = nsx::current_device();
    if (dev < 0) return NSX_ENODEV;
    return nsx::map_err(nsx::launch_icmp_rx(nsx::launch_cfg(nsx::device_cus(dev), tune), ipver, d_base, d_offsets, n,
                                            d_mask, d_ip_raw, d_icmp_raw, d_type, static_cast<hipStream_t>(stream)));
}

int echo_dev(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid, uint32_t ttl,
             uint64_t* d_hit, nsx_stream_t stream) {
    if ((n && (!d_base || !d_offsets || !d_valid || !d_hit)) || n >= kMaxFrames || ttl > 255u) return NSX_EINVAL;
    if (nsx::current_device() < 0) return NSX_ENODEV;
    return nsx::map_err(
        nsx::launch_icmp_echo(ipver, d_base, d_offsets, n, d_valid, ttl, d_hit, static_cast<hipStream_t>(stream)));
}

}  // namespace

extern "C" {

int nsx_icmp_err_work_bytes(uint64_t n, uint64_t* out) {
    if (!out || n >= kMaxFrames) return NSX_EINVAL;
    *out = nsx::icmp_err_work_bytes(n);
    return NSX_OK;
}

#define NSX_ICMP_ERR(V)                                                                                               \
    int nsx_icmp_err_ipv##V##_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,   \
                                  const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* out,    \
                                  void* d_work, uint64_t work_bytes, nsx_stream_t stream) {                           \
        return err_dev(V, d_base, d_offsets, n, d_req, d_arg, cfg, out, d_work, work_bytes, stream, nullptr);         \
    }                                                                                                                 \
    int nsx_icmp_err_ipv##V##_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n,                    \
                                        const uint32_t* d_req, const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg,    \
                                        const nsx_icmp_err_out* out, void* d_work, uint64_t work_bytes,               \
                                        nsx_stream_t stream, const nsx_tune* tune) {                                  \
        return err_dev(V, d_base, d_offsets, n, d_req, d_arg, cfg, out, d_work, work_bytes, stream, tune);            \
    }                                                                                                                 \
    int nsx_icmp_req_ttl_ipv##V##_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n,                      \
                                      const uint64_t* d_valid, uint32_t ttl_dec, uint32_t* d_req, uint32_t* d_arg,    \
                                      nsx_stream_t stream) {                                                          \
        return req_ttl_dev(V, d_base, d_offsets, n, d_valid, ttl_dec, d_req, d_arg, stream);                          \
    }                                                                                                                 \
    int nsx_icmp_echo_reply_ipv##V##_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid, \
                                         uint32_t ttl, uint64_t* d_hit, nsx_stream_t stream) {                        \
        return echo_dev(V, d_base, d_offsets, n, d_valid, ttl, d_hit, stream);                                        \
    }
NSX_ICMP_ERR(4)
NSX_ICMP_ERR(6)
#undef NSX_ICMP_ERR

int nsx_icmp_req_frag_dev(const uint8_t* d_status, const uint32_t* d_mtu, uint64_t n, uint32_t* d_req, uint32_t* d_arg,
                          nsx_stream_t stream) {
    if ((n && (!d_status || !d_mtu || !d_req || !d_arg)) || n >= kMaxFrames) return NSX_EINVAL;
    if (nsx::current_device() < 0) return NSX_ENODEV;
    return nsx::map_err(nsx::launch_icmp_req_frag(d_status, d_mtu, n, d_req, d_arg, static_cast<hipStream_t>(stream)));
}

int nsx_icmp_rx_ipv4_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                uint16_t* d_ip_raw, uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream) {
    return rx_dev(4, d_base, d_offsets, n, d_mask, d_ip_raw, d_icmp_raw, d_type, stream, nullptr);
}

int nsx_icmp_rx_ipv4_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                      uint16_t* d_ip_raw, uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream,
                                      const nsx_tune* tune) {
    return rx_dev(4, d_base, d_offsets, n, d_mask, d_ip_raw, d_icmp_raw, d_type, stream, tune);
}

int nsx_icmp_rx_ipv6_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream) {
    return rx_dev(6, d_base, d_offsets, n, d_mask, nullptr, d_icmp_raw, d_type, stream, nullptr);
}

int nsx_icmp_rx_ipv6_verify_dev_tuned(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                      uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream,
                                      const nsx_tune* tune) {
    return rx_dev(6, d_base, d_offsets, n, d_mask, nullptr, d_icmp_raw, d_type, stream, tune);
}

}  // extern "C"
