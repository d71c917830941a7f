// api_util.h — what csum_api.cpp, host_batch.cpp and nat_api.cpp share: the ABI structs as the launchers' structs,
// the HIP error mapping, the calling thread's device and the cached per-device CU count (all defined in csum_api.cpp).
#pragma once
#include "../../include/nsx_csum.h"
#include "csum_kernels.h"

namespace nsx {

int map_err(hipError_t e);  // NSX_OK / NSX_ENOMEM / NSX_ENODEV / NSX_EIO; clears HIP's last error
int device_cus(int dev);    // compute units of device `dev`, queried once; 0 when it cannot be used
int device_count();         // 0 when HIP reports none or fails
int current_device();       // current device of the calling thread, or -1 when there is no usable GPU

inline TcpHdrSoA to_soa(const nsx_tcp_hdr_soa& h) {
    return {h.src_port, h.dst_port, h.seq_num, h.ack_num, h.offset, h.control, h.window, h.urgent_ptr};
}
inline IpHdrSoA to_soa(const nsx_ip_hdr_soa& a) { return {a.src, a.dst, a.ident, a.ttl, a.tclass, a.flow}; }
inline GroOut to_soa(const nsx_gro_out& o) {
    return {o.n_super, o.src,      o.dst,         o.ident,     o.ttl,     o.tclass,
            o.flow,    o.src_port, o.dst_port,    o.seq_num,   o.ack_num, o.offset,
            o.control, o.window,   o.urgent_ptr,  o.mss,       o.opts,    o.opt_off,
            o.data,    o.data_off, o.first_frame, o.frame_cnt, o.frame_seg};
}
inline TcpParsedSoA to_soa(const nsx_tcp_parsed_soa& o) {
    return {o.src_port, o.dst_port, o.seq_num,    o.ack_num,  o.offset,    o.control,
            o.window,   o.checksum, o.urgent_ptr, o.data_off, o.n_options, o.status};
}

}  // namespace nsx
