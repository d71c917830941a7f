// csum_kernels.h — internal launcher interface between the C ABI (csum_api.cpp, nat_api.cpp, udp_api.cpp,
// ugro_api.cpp, frag_api.cpp, host_batch.cpp) and the gfx950 kernels (csum_kernels.hip, gro_kernels.hip,
// gro_flow_kernels.hip, nat_kernels.hip, udp_kernels.hip, ugro_kernels.hip, frag_kernels.hip). Not a public header.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

struct nsx_tune;  // include/nsx_tune.h

namespace nsx {

// Per-call launch configuration: the device's CU count plus the optional
// overrides of include/nsx_tune.h (0 = the per-path default measured best on
// MI355X). Built per call from the caller's nsx_tune (or none);
// there is no process-wide tuning state.
struct LaunchCfg {
    int cus = 0;              // compute units of the device
    int blocks_per_cu = 0;    // persistent grid = cus × blocks_per_cu blocks of 256 threads
    int segs_per_wave = 0;    // fixed short-segment paths: segments per wave task (1, 2, 4, 8)
    int block_mode = 0;       // 0 auto (a block per segment when n < 4·cus), 1 never, 2 always
    int rows = 0;             // ragged scan kernel: 1 KiB rows per batch (4, 8, 16); flow GRO: 256-key rows per sort tile
    int run_segs = 0;         // ragged scan kernel: segments per wave task (1..63)
    int xcd_chunk = 0;        // XCD deal: 0 auto, 1..20 = chunks of 2^k tasks, else contiguous eighths
    int64_t window_bytes = 0; // fixed short-segment path: back-to-back launches of ≤ this many bytes (0 auto, -1 one)
    int kernel = 0;           // force an alternative code path (nsx_tune.h NSX_TUNE_KERNEL_*); 0 = by layout
    int deal = 0;             // -1: equal static shares (no dealt runs) for this call
};

// The LaunchCfg of one call on a device with `cus` compute units; t nullable (csum_api.cpp).
LaunchCfg launch_cfg(int cus, const nsx_tune* t);

// Kernel launches nsx_csum_fixed_dev makes for this batch (its back-to-back windows).
uint64_t fixed_launch_count(const LaunchCfg& c, uintptr_t base, uint64_t stride, uint32_t seg_len, uint64_t n);
// Launches one IPv4 header call makes (the packed 20 B kernel's windows).
uint64_t ipv4_hdr_launch_count(const LaunchCfg& c, uintptr_t base, uint64_t stride, uint32_t hdr_off, uint64_t n);

hipError_t launch_fixed(const LaunchCfg& c, const void* d_base, uint64_t stride, uint32_t seg_len,
                        uint64_t n, const uint32_t* partial, uint16_t* out, hipStream_t st);
hipError_t launch_ragged(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         const uint32_t* partial, uint16_t* out, uint8_t* ok, hipStream_t st);
// Fused receive pass: IPv4 (ipver 4: header + pseudo-header + TCP checksum) or IPv6 (ipver 6: pseudo-header +
// TCP checksum) per frame into a validity bitmask (ceil(n/64) words); ip_raw (IPv4 only) / tcp_raw nullable.
// false for overrides that name no shape of the receive kernels (segs_per_wave outside {0, 1, 2, 5-9}, or 5-9 off the
// default grid): NSX_EINVAL
bool rx_tune_valid(const LaunchCfg& c);
bool ragged_tune_valid(const LaunchCfg& c);
hipError_t launch_rx_tcp(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         uint64_t* mask, uint16_t* ip_raw, uint16_t* tcp_raw, hipStream_t st);
hipError_t launch_pseudo_ipv4(const uint8_t* src, const uint8_t* dst, const uint32_t* len, uint8_t proto,
                              uint64_t n, uint32_t* partial, uint32_t max_blocks, hipStream_t st);
hipError_t launch_pseudo_ipv6(const uint8_t* src, const uint8_t* dst, const uint32_t* len, uint8_t nh,
                              uint64_t n, uint32_t* partial, uint32_t max_blocks, hipStream_t st);
hipError_t launch_verify_mask(const uint16_t* raw, uint64_t n, uint64_t* mask, uint32_t max_blocks,
                              hipStream_t st);
struct TcpHdrSoA {  // device arrays, one entry per segment (tcp.go:39-54 field order)
    const uint16_t* src_port;
    const uint16_t* dst_port;
    const uint32_t* seq;
    const uint32_t* ack;
    const uint8_t* offset;
    const uint8_t* ctl;
    const uint16_t* window;
    const uint16_t* urgent;
};
struct IpHdrSoA {  // device arrays of the transmit pass, one entry per frame (include/nsx_csum.h nsx_ip_hdr_soa)
    const uint8_t* src;
    const uint8_t* dst;
    const uint16_t* ident;
    const uint8_t* ttl;
    const uint8_t* tclass;
    const uint32_t* flow;
};
// TCP wire images (ip null), or whole IPv4 / IPv6 datagrams (ipver 4 / 6: ip's fields, partial unused).
hipError_t launch_tcp_build(const LaunchCfg& c, int ipver, const IpHdrSoA* ip, const TcpHdrSoA& h,
                            const uint8_t* opts, const uint64_t* opt_off, const uint8_t* data,
                            const uint64_t* data_off, uint64_t data_bytes, const uint32_t* partial, uint64_t n,
                            uint8_t* out, const uint64_t* out_off, uint16_t* raw, hipStream_t st);
// Segmentation offload (nsx_tso_*): the frame map over per-super-segment arrays (include/nsx_csum.h).
struct TsoMap {
    const uint32_t* mss;          // per super-segment: payload bytes per frame
    const uint64_t* frame_first;  // per super-segment: its first frame
    const uint32_t* frame_seg;    // per frame: its super-segment
};
// The transmit pass over super-segments: h, ip, opt_off and data_off hold one entry per super-segment; out_off
// (n_frames + 1) and raw (n_frames, nullable) one per frame.
hipError_t launch_tso_build(const LaunchCfg& c, int ipver, const IpHdrSoA& ip, const TsoMap& tso, const TcpHdrSoA& h,
                            const uint8_t* opts, const uint64_t* opt_off, const uint8_t* data,
                            const uint64_t* data_off, uint64_t data_bytes, uint64_t n_frames, uint8_t* out,
                            const uint64_t* out_off, uint16_t* raw, hipStream_t st);
// Receive coalescing (nsx_gro_*, gro_kernels.hip): the writable device arrays of include/nsx_csum.h nsx_gro_out,
// member for member.
struct GroOut {
    uint64_t* n_super;
    uint8_t* src;
    uint8_t* dst;
    uint16_t* ident;
    uint8_t* ttl;
    uint8_t* tclass;
    uint32_t* flow;
    uint16_t* src_port;
    uint16_t* dst_port;
    uint32_t* seq_num;
    uint32_t* ack_num;
    uint8_t* offset;
    uint8_t* control;
    uint16_t* window;
    uint16_t* urgent_ptr;
    uint32_t* mss;
    uint8_t* opts;
    uint64_t* opt_off;
    uint8_t* data;
    uint64_t* data_off;
    uint64_t* first_frame;
    uint32_t* frame_cnt;
    uint32_t* frame_seg;
};
// Scratch bytes of one launch_gro over n frames (whatever the tune).
uint64_t gro_work_bytes(uint64_t n);
// Frames → super-segments (ipver 4 / 6); n < 2^32 - 1, work of at least gro_work_bytes(n). c.run_segs = frames per
// scan block (0 = 4096, clamped to 16..65536), c.blocks_per_cu = the copy kernel's grid (default 8).
hipError_t launch_gro(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                      const uint64_t* valid, const GroOut& o, void* work, hipStream_t st);
// The same passes over the batch whose frame p is frame order[p] of the input (n entries, a permutation of 0..n-1):
// offsets, the valid bit and frame_seg go through the order; first_frame holds positions (gro_kernels.hip).
hipError_t launch_gro_ordered(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                              const uint64_t* valid, const uint32_t* order, const GroOut& o, void* work,
                              hipStream_t st);
// Flow-keyed receive coalescing (nsx_gro_flow_*, gro_flow_kernels.hip): scratch bytes of one launch_gro_flow over n
// frames (whatever the tune; >= gro_work_bytes(n)).
uint64_t gro_flow_work_bytes(uint64_t n);
// Key pass, stable radix sort of the frame indices by key into d_order, then launch_gro_ordered: one serial chain
// of launches. n == 0 writes no order. c.rows = keys per sort tile in units of 256 (0 = the default, clamped to
// 1..64).
hipError_t launch_gro_flow(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                           const uint64_t* valid, uint32_t* d_order, const GroOut& o, void* work, hipStream_t st);
// The stable radix sort of launch_gro_flow on its own (gro_flow_kernels.hip), shared with UDP receive coalescing:
// flow_sort_bytes(n) bytes of scratch at an 8-aligned address, split by flow_sort_work. The caller's key pass writes
// the keys and the identity index to keys[0] / idx[0]; launch_flow_sort (n >= 1) leaves the frame indices in stable
// ascending key order in d_order. c.rows as above.
struct FlowSortWork {
    uint32_t* keys[2];
    uint32_t* idx[2];
    uint32_t* table;
};
uint64_t flow_sort_bytes(uint64_t n);
FlowSortWork flow_sort_work(void* work, uint64_t n);
hipError_t launch_flow_sort(const LaunchCfg& c, uint32_t n, const FlowSortWork& s, uint32_t* d_order, hipStream_t st);
// UDP receive coalescing (nsx_ugro_*, ugro_kernels.hip): the writable device arrays of include/nsx_csum.h
// nsx_ugro_out, member for member.
struct UgroOut {
    uint64_t* n_super;
    uint8_t* src;
    uint8_t* dst;
    uint16_t* ident;
    uint8_t* ttl;
    uint8_t* tclass;
    uint32_t* flow;
    uint16_t* src_port;
    uint16_t* dst_port;
    uint32_t* gso;
    uint8_t* data;
    uint64_t* data_off;
    uint64_t* first_frame;
    uint32_t* frame_cnt;
    uint32_t* frame_seg;
};
// Scratch bytes of one launch_ugro / launch_ugro_flow over n frames (whatever the tune; flow >= plain).
uint64_t ugro_work_bytes(uint64_t n);
uint64_t ugro_flow_work_bytes(uint64_t n);
// Datagrams → super-datagrams (ipver 4 / 6); n < 2^32 - 1, work of at least ugro_work_bytes(n). c.run_segs and
// c.blocks_per_cu as launch_gro.
hipError_t launch_ugro(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                       const uint64_t* valid, const UgroOut& o, void* work, hipStream_t st);
// Key pass, launch_flow_sort into d_order, then the same passes over that order: one serial chain of launches.
// n == 0 writes no order. Work of at least ugro_flow_work_bytes(n).
hipError_t launch_ugro_flow(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                            const uint64_t* valid, uint32_t* d_order, const UgroOut& o, void* work, hipStream_t st);
// The in-place NAT rewrite (nsx_nat_*, nat_kernels.hip): one launch, a lane per frame; none for n == 0. n < 2^32 - 1,
// slots a power of two <= 2^31, the table 16-byte aligned, ttl_dec <= 255 (nat_api.cpp checks all of it).
hipError_t launch_nat_rewrite(int ipver, void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* valid,
                              const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit, hipStream_t st);
// The UDP passes (nsx_udp_*, udp_kernels.hip). The frame map of segmentation offload over per-super-datagram arrays:
struct UdpUsoMap {
    const uint32_t* gso;          // per super-datagram: payload bytes per datagram
    const uint64_t* frame_first;  // per super-datagram: its first frame
    const uint32_t* frame_seg;    // per frame: its super-datagram
};
// Whole IPv4 / IPv6 datagrams carrying UDP (ipver 4 / 6), n_frames of them; uso null: one entry per frame in every
// array (n_super unused), else one per super-datagram (n_super >= 1 of them). c.run_segs = frames per wave task
// (1..64), c.blocks_per_cu the grid (default 4). One launch; none for n_frames == 0.
hipError_t launch_udp_build(const LaunchCfg& c, int ipver, const IpHdrSoA& ip, const uint16_t* src_port,
                            const uint16_t* dst_port, const UdpUsoMap* uso, uint64_t n_super, const uint8_t* data,
                            const uint64_t* data_off, uint64_t data_bytes, uint64_t n_frames, uint32_t no_csum,
                            uint8_t* out, const uint64_t* out_off, uint16_t* raw, hipStream_t st);
// The UDP receive verify: a wave per 64-frame mask word, statically split; c.run_segs = frames per metadata step
// (1..64, default 16), c.blocks_per_cu the grid (default 8). ip_raw (IPv4 only) / udp_raw nullable.
hipError_t launch_udp_rx(const LaunchCfg& c, int ipver, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                         uint64_t* mask, uint16_t* ip_raw, uint16_t* udp_raw, hipStream_t st);
// IPv4 fragmentation (nsx_frag_*, frag_kernels.hip): one launch over the n_frags output slots of the frame map, none
// for n_frags == 0. n < 2^32 (frag_api.cpp). c.blocks_per_cu = the grid (default 8).
hipError_t launch_frag(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu,
                       uint64_t n, const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags,
                       uint8_t* d_out, const uint64_t* d_out_off, uint8_t* d_status, hipStream_t st);
// IPv4 reassembly (nsx_reasm_*, frag_kernels.hip): the writable device arrays of include/nsx_csum.h nsx_reasm_out,
// member for member.
struct ReasmDevOut {
    uint64_t* n_out;
    uint8_t* out;
    uint64_t* out_off;
    uint64_t* first_pos;
    uint32_t* frag_cnt;
    uint32_t* frame_seg;
    uint64_t* is_frag;
};
// Scratch bytes of one launch_reasm over n frames (whatever the tune).
uint64_t reasm_work_bytes(uint64_t n);
// Key pass, launch_flow_sort by fragment offset and again by datagram key into d_order, then the run passes and the
// copy over that order: one serial chain of launches. n < 2^32 - 1; n == 0 writes no order. c.run_segs, c.rows and
// c.blocks_per_cu as launch_ugro_flow.
hipError_t launch_reasm(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                        uint32_t* d_order, const ReasmDevOut& out, void* work, hipStream_t st);
struct TcpParsedSoA {  // device arrays, one entry per segment; every member nullable
    uint16_t* src_port;
    uint16_t* dst_port;
    uint32_t* seq;
    uint32_t* ack;
    uint8_t* offset;
    uint8_t* ctl;
    uint16_t* window;
    uint16_t* checksum;
    uint16_t* urgent;
    uint64_t* data_off;
    uint8_t* n_options;
    uint8_t* status;
};
// parseSegment (tcp.go:130-185) over segments d_base[d_offsets[i], d_offsets[i+1]).
hipError_t launch_tcp_parse(const LaunchCfg& c, const void* d_base, const uint64_t* d_offsets, uint64_t n,
                            const TcpParsedSoA& o, hipStream_t st);
// mode 0 verify (out), 1 fill (out nullable), 2 verify into the bitmask `mask` (ceil(n/64) words)
hipError_t launch_ipv4_hdr(const LaunchCfg& c, uint8_t* base, uint64_t stride, uint32_t hdr_off, uint64_t n,
                           int mode, uint16_t* out, uint64_t* mask, hipStream_t st);
// The per-stream deal counter sets (csum_kernels.hip deal_heads): return stream st's for reuse; sets given out.
void deal_release(hipStream_t st);
uint32_t deal_sets_in_use(int dev);
hipError_t launch_fill_splitmix64(void* d_buf, uint64_t byte_off, uint64_t nbytes, uint64_t seed,
                                  uint32_t max_blocks, hipStream_t st);

}  // namespace nsx
