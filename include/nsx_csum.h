/*
 * nsx_csum.h — C ABI of the MI355X-native Internet checksum (RFC 1071) path.
 *
 * This is the drop-in boundary for the reference's one checksum function,
 *   transport/tcp/tcp.go:72-95  func (s segment) computeChecksum(ipPseudoHeader []byte) uint16
 * (reference: oneee-playground/network-stack, pure Go). A Go caller reaches it
 * through the cgo shim in network-stack_amd/go/transport/tcp/ (INTEGRATION.md).
 *
 * Semantics shared by every entry point (tcp.go:68-95):
 *   - the checksummed stream is prefix ‖ segment (tcp.go:73); an odd total is
 *     zero-padded (tcp.go:74-77);
 *   - 16-bit big-endian words are added with end-around carry (tcp.go:79-92);
 *   - the RAW one's-complement sum is returned, NOT complemented (tcp.go:94).
 *     0x0000 only for an all-zero input; a nonzero input whose sum is
 *     ≡ 0 mod 0xFFFF gives 0xFFFF. The sender stores nsx_field(raw) = ~raw
 *     (tcp_test.go:28); a receiver accepts iff raw == 0xFFFF (tcp.go:70).
 *
 * Conventions:
 *   - Return 0 (NSX_OK) or a negative errno-style code; never abort or print.
 *   - The caller owns every buffer. No pointer is retained after the stream
 *     work completes (device calls) or after return (host calls).
 *   - Device calls are asynchronous on `stream` (a hipStream_t; NULL = the
 *     default stream of the current device). Device pointers must belong to the
 *     device current on the calling thread. No host synchronisation, no
 *     allocation inside device calls (hipGraph-capturable).
 *   - Re-entrant; no global mutable state on the data path.
 *   - A device call on a host with no usable GPU returns NSX_ENODEV. There is no
 *     CPU fallback for the batch/device entry points.
 */
#ifndef NSX_CSUM_H
#define NSX_CSUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSX_OK      0
#define NSX_EIO    (-5)   /* a HIP runtime call or kernel launch failed */
#define NSX_ENOMEM (-12)  /* host or device allocation failed */
#define NSX_ENODEV (-19)  /* no usable GPU / bad device ordinal */
#define NSX_EINVAL (-22)  /* null pointer with nonzero length, bad sizes */

#define NSX_ABI_VERSION 2  /* 2: process-wide tuning knobs removed (nsx_tune.h) */

typedef void* nsx_stream_t; /* hipStream_t, opaque to C/Go callers */

/* ----------------------------------------------------------------------------
 * Single segment, host CPU.
 * Replaces: transport/tcp/tcp.go:72-95 computeChecksum (called from
 * tcp_test.go:28,30). Exactly its semantics over prefix ‖ seg, without the
 * reference's allocation/copy of the concatenation (tcp.go:73) and without
 * writing into the prefix's spare capacity. For per-segment cgo calls; never
 * touches the GPU (a per-segment cgo call must not drive the device).
 * prefix may be NULL iff prefix_len == 0; likewise seg.
 */
int nsx_csum16(const uint8_t* prefix, size_t prefix_len,
               const uint8_t* seg, size_t seg_len, uint16_t* out_raw_sum);

/* ----------------------------------------------------------------------------
 * Device-resident batches (the hot path). One result (raw sum) per segment.
 *
 * d_prefix_partial (nullable): per-segment integer sum of the prefix's
 * big-endian 16-bit words (e.g. an IPv4/IPv6 TCP pseudo-header, whose length is
 * even), folded or not; result[i] = raw sum over prefix_i ‖ segment_i.
 * Produce it with nsx_pseudo_ipv4_partial_dev or nsx_csum_fixed_dev on the
 * pseudo-headers themselves.
 */

/* Fixed stride: segment i occupies d_base[i*stride, i*stride + seg_len).
 * The span [d_base, d_base + (n-1)*stride + seg_len) must be readable.
 * Replaces a Go loop of computeChecksum over equal-size segments (tcp.go:72). */
int nsx_csum_fixed_dev(const void* d_base, uint64_t stride, uint32_t seg_len, uint64_t n,
                       const uint32_t* d_prefix_partial, uint16_t* d_out, nsx_stream_t stream);

/* Ragged: segment i occupies d_base[d_offsets[i], d_offsets[i+1]); d_offsets
 * has n+1 non-decreasing entries; segments may start at any byte (dense packing,
 * odd starts). The span [d_base + d_offsets[0], d_base + d_offsets[n]) must be
 * readable. */
int nsx_csum_ragged_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n,
                        const uint32_t* d_prefix_partial, uint16_t* d_out, nsx_stream_t stream);

/* Receive-side verify (tcp.go:70): d_ok[i] = (raw_i == 0xFFFF), where raw_i is
 * the ragged-batch raw sum with the optional prefix partial. d_raw (nullable)
 * also receives the raw sums. */
int nsx_verify_ragged_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n,
                          const uint32_t* d_prefix_partial, uint8_t* d_ok, uint16_t* d_raw,
                          nsx_stream_t stream);

/* IPv4 TCP pseudo-header partials (RFC 9293 §3.1: src(4) dst(4) 0 proto len(2))
 * for n segments: d_src/d_dst are n×4 address bytes as ip.Addr.Raw()
 * (network/ip/v4/ipv4.go:15), d_len the TCP length of each segment, proto e.g.
 * ip.NextProtoTCP = 6 (network/ip/protocols.go:8). Writes the integer BE-word
 * sum to d_partial[i] (the d_prefix_partial convention above). */
int nsx_pseudo_ipv4_partial_dev(const uint8_t* d_src, const uint8_t* d_dst,
                                const uint32_t* d_len, uint8_t proto, uint64_t n,
                                uint32_t* d_partial, nsx_stream_t stream);

/* IPv6 TCP pseudo-header partials (RFC 8200 §8.1: src(16) dst(16) len(4)
 * zero(3) next_header(1)) for n segments: d_src/d_dst are n×16 address bytes as
 * ip.Addr.Raw() (network/ip/v6/ipv6.go:16), d_len the upper-layer length, and
 * next_header e.g. ip.NextProtoTCP = 6. Same d_partial convention as above. */
int nsx_pseudo_ipv6_partial_dev(const uint8_t* d_src, const uint8_t* d_dst,
                                const uint32_t* d_len, uint8_t next_header, uint64_t n,
                                uint32_t* d_partial, nsx_stream_t stream);

/* Receive-side verify as a bitmask (tcp.go:70): bit (i % 64) of d_mask[i / 64]
 * is set iff d_raw[i] == 0xFFFF; bits past n in the last word are 0. d_mask
 * holds ceil(n/64) words. Pairs with nsx_csum_fixed_dev / nsx_csum_ragged_dev. */
int nsx_verify_mask_dev(const uint16_t* d_raw, uint64_t n, uint64_t* d_mask, nsx_stream_t stream);

/* Fused sender path: segment.bytes() + computeChecksum +
 * field write in one GPU pass (transport/tcp/tcp.go:98-128, :68-71). For each
 * segment i it writes the wire image — the 20-byte big-endian header built from
 * the fields below (checksum field = ~raw), the option bytes
 * d_opts[d_opt_off[i], d_opt_off[i+1]) followed by the reference's padding of
 * `remainder` zero bytes (tcp.go:118-121), then the payload
 * d_data[d_data_off[i], d_data_off[i+1]) — to d_out + d_out_off[i], where raw is
 * the sum over prefix_i ‖ image with the field zero. d_out_off[i] must be a
 * multiple of 4 and leave room for nsx_tcp_wire_len bytes; up to 3 bytes after
 * each image are zero-filled (use nsx_tcp_layout_host). d_opt_off nullable (no
 * options); data_bytes = size of the d_data buffer. d_raw (nullable) receives
 * the raw sums. All nsx_tcp_hdr_soa members are device arrays of n entries;
 * `offset` is the whole byte 12, as the reference stores it (tcp.go:106); a
 * NULL `offset` computes it on the device as computeOffset() does (tcp.go:59-66):
 * uint8((20 + option bytes + 3) / 4).
 * Each wire image must be shorter than 2^31 bytes (TCP segments are ≤ 64 KiB;
 * TSO super-segments ≤ 256 KiB). */
typedef struct {
    const uint16_t* src_port;
    const uint16_t* dst_port;
    const uint32_t* seq_num;
    const uint32_t* ack_num;
    const uint8_t* offset;
    const uint8_t* control;  /* ctl.byte() (tcp.go:192-203) */
    const uint16_t* window;
    const uint16_t* urgent_ptr;
} nsx_tcp_hdr_soa;

int nsx_tcp_build_dev(const nsx_tcp_hdr_soa* hdr, const uint8_t* d_opts, const uint64_t* d_opt_off,
                      const uint8_t* d_data, const uint64_t* d_data_off, uint64_t data_bytes,
                      const uint32_t* d_prefix_partial, uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                      uint16_t* d_raw, nsx_stream_t stream);

/* Receive-side parse (parseSegment, transport/tcp/tcp.go:130-185) of n TCP
 * segments d_base[d_offsets[i], d_offsets[i+1]) (any alignment, d_offsets as
 * for nsx_csum_ragged_dev) into device arrays of n entries; every member of
 * *out is nullable. Fields as the reference reads them (offset = the whole byte
 * 12, control = ctl.byte(), checksum = bytes 16-17); data_off[i] = d_offsets[i]
 * + offset*4 (the payload, s.data = raw[dataAt:]); n_options = the options the
 * reference appends (NOP and MSS; EOL ends the walk). status[i]:
 *   NSX_TCP_PARSE_OK            parsed;
 *   NSX_TCP_PARSE_SHORT         fewer than 20 bytes ("segment too short", :131);
 *   NSX_TCP_PARSE_OFFSET        offset*4 > length ("advertised data offset too
 *                               long", :152);
 *   NSX_TCP_PARSE_OPTION_RANGE  an MSS option whose length runs past the segment
 *                               (the reference's slice panics or reads past the
 *                               segment, :173-174);
 *   NSX_TCP_PARSE_OPTION_KIND   an option kind other than 0-2 before dataAt (the
 *                               reference's loop never advances, :160-179).
 * On any status but OK the fields, data_off and n_options are 0 (the reference
 * returns segment{}). */
#define NSX_TCP_PARSE_OK 0
#define NSX_TCP_PARSE_SHORT 1
#define NSX_TCP_PARSE_OFFSET 2
#define NSX_TCP_PARSE_OPTION_RANGE 3
#define NSX_TCP_PARSE_OPTION_KIND 4
typedef struct {
    uint16_t* src_port;
    uint16_t* dst_port;
    uint32_t* seq_num;
    uint32_t* ack_num;
    uint8_t* offset;
    uint8_t* control;
    uint16_t* window;
    uint16_t* checksum;
    uint16_t* urgent_ptr;
    uint64_t* data_off;
    uint8_t* n_options;
    uint8_t* status;
} nsx_tcp_parsed_soa;

int nsx_tcp_parse_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const nsx_tcp_parsed_soa* out,
                      nsx_stream_t stream);

/* Wire length of segment.bytes() with opt_len option bytes (tcp.go:98-128). */
uint64_t nsx_tcp_wire_len(uint64_t opt_len, uint64_t data_len);

/* 4-byte-aligned output offsets for nsx_tcp_build_dev (host arrays; h_opt_off
 * nullable): h_out_off[i] = Σ_{j<i} round_up4(wire_len_j), h_out_off[n] = total. */
int nsx_tcp_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, uint64_t n, uint64_t* h_out_off);

/* Fused transmit pass (the transmit twin of the receive passes below, SURVEY.md
 * §8 f1 + f2 + f3 in one launch): whole IPv4 / IPv6 datagrams carrying TCP,
 * built from the segment fields plus the per-frame IP fields of nsx_ip_hdr_soa
 * (device arrays; src / dst as ip.Addr.Raw(), network/ip/v4/ipv4.go:15,
 * v6/ipv6.go:16). Frame i is written at d_out + d_out_off[i]. Its TCP part is
 * exactly the image nsx_tcp_build_dev writes (fields, options, the reference's
 * padding, payload; a NULL `offset` computed on the device); let wire be
 * nsx_tcp_wire_len of it.
 *   IPv4: 20 header bytes (no IP options) then the image: 0x45, 0x00, total
 *     length 20 + wire, ident, 0x40 0x00 (DF, offset 0), ttl, 6
 *     (ip.NextProtoTCP, network/ip/protocols.go:8), the header checksum (~raw
 *     over the 20 bytes with the field zero, RFC 791 §3.1), src, dst.
 *   IPv6: the 40-byte fixed header of RFC 8200 §3 then the image: version 6,
 *     tclass, flow, payload length wire, Next Header 6, hop limit ttl, src, dst.
 * The TCP checksum field is ~raw, raw being the computeChecksum sum
 * (tcp.go:72-95) over the pseudo-header ‖ the image with the field zero; the
 * pseudo-header is built from the frame's own src / dst, protocol 6 and wire
 * (RFC 9293 §3.1, 12 bytes; RFC 8200 §8.1, 40 bytes) — there is no partials
 * argument and no second launch. d_tcp_raw (nullable) receives raw.
 * Layout rule as nsx_tcp_build_dev: d_out_off[i] a multiple of 4 with room for
 * the frame rounded up to 4 bytes, the up to 3 bytes after a frame zero-filled,
 * bytes between a padded frame and the next offset left as they were.
 * nsx_tx_layout_host makes packed offsets, h_out_off[i] = Σ_{j<i}
 * round_up4(ip_hdr_len + wire_j), ip_hdr_len 20 or 40 (NSX_EINVAL otherwise).
 * When every frame length is a multiple of 4 and the layout is packed,
 * d_out_off is directly the d_offsets of nsx_rx_ipv4_tcp_verify_dev /
 * nsx_rx_ipv6_tcp_verify_dev over d_out.
 * A frame whose length does not fit its 16-bit length field (IPv4 wire > 65515,
 * IPv6 wire > 65535) is not built: nothing is written for it, padding included,
 * and d_tcp_raw[i] = 0 (a built frame's raw sum is never 0: the pseudo-header
 * holds the byte 6). That holds for a payload of any length the 64-bit offsets
 * can say, 2^31 and 2^32 bytes and more included: nsx_tcp_build_dev's limit of
 * 2^31 bytes per image is a limit on what is built and does not apply to a
 * frame that is not. Validation and conventions as nsx_tcp_build_dev; no
 * allocation, no host sync, no per-stream counters: the call can be captured
 * into a graph. */
typedef struct {
    const uint8_t*  src;     /* n×4 (IPv4) or n×16 (IPv6) bytes, ip.Addr.Raw() */
    const uint8_t*  dst;
    const uint16_t* ident;   /* IPv4 identification; NULL = 0; ignored for IPv6 */
    const uint8_t*  ttl;     /* TTL / hop limit; NULL = 64 */
    const uint8_t*  tclass;  /* IPv6 traffic class; NULL = 0; ignored for IPv4 (TOS = 0) */
    const uint32_t* flow;    /* IPv6 flow label (low 20 bits); NULL = 0; ignored for IPv4 */
} nsx_ip_hdr_soa;

int nsx_tx_ipv4_tcp_build_dev(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                              const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                              uint64_t data_bytes, uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                              uint16_t* d_tcp_raw, nsx_stream_t stream);
int nsx_tx_ipv6_tcp_build_dev(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                              const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                              uint64_t data_bytes, uint64_t n, uint8_t* d_out, const uint64_t* d_out_off,
                              uint16_t* d_tcp_raw, nsx_stream_t stream);
int nsx_tx_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, uint64_t n, uint32_t ip_hdr_len,
                       uint64_t* h_out_off);

/* TCP segmentation offload on the fused transmit pass: the caller hands over n
 * super-segments — per connection one header template, one option block and a
 * run of payload far longer than one MSS — instead of one array entry per
 * frame, and the transmit kernel cuts them. Super-segment s has one entry in
 * every nsx_tcp_hdr_soa and nsx_ip_hdr_soa array, option bytes
 * d_opts[d_opt_off[s], d_opt_off[s+1]), payload d_data[d_data_off[s],
 * d_data_off[s+1]) of len_s bytes, and d_mss[s] >= 1, the payload bytes per
 * frame (Linux gso_size: options and headers are not counted). It yields
 * cnt_s = max(1, ceil(len_s / mss_s)) frames. Frame j of s (0 <= j < cnt_s) is
 * exactly the frame nsx_tx_ipv4_tcp_build_dev / nsx_tx_ipv6_tcp_build_dev builds
 * from s's fields, except:
 *   payload   d_data[d_data_off[s] + j*mss, min(d_data_off[s] + (j+1)*mss,
 *             d_data_off[s+1])) — empty when len_s == 0. The kernel reads no
 *             payload byte outside s's own range, whatever the frame map says.
 *   seq_num   seq_num[s] + j*mss modulo 2^32.
 *   control   FIN (0x01) and PSH (0x08) are kept only on the last frame
 *             (j == cnt_s - 1), CWR (0x80) only on the first (j == 0); every
 *             other bit is copied to every frame. This is the rule of Linux's
 *             tcp_gso_segment. SYN is merely copied: a caller does not offload
 *             SYN segments.
 *   ident     IPv4: (ident[s] + j) modulo 2^16, ident[s] = 0 when the array is
 *             NULL. IPv6 flow label and traffic class are copied.
 * Everything else — ack, window, urgent pointer, the options with the
 * reference's padding, ports, addresses, TTL — is copied to every frame; with
 * `offset` NULL, computeOffset() runs as in nsx_tcp_build_dev. The IPv4 total
 * length / IPv6 payload length, the IPv4 header checksum, the pseudo-header and
 * the TCP checksum follow from the frame's own slice. A frame whose TCP part
 * does not fit its IP length field is not built and its raw sum is 0, as in
 * the transmit pass.
 * Frame map (host helpers below; the device calls take them as device arrays):
 *   frame_first (n + 1): prefix sum of cnt_s — super-segment s owns frames
 *     [frame_first[s], frame_first[s+1]); frame_first[n] = n_frames.
 *   frame_seg (n_frames): the super-segment of each frame.
 *   out_off (n_frames + 1): the frame slots, layout rule as the transmit pass.
 * nsx_tso_count_host writes h_frame_first (NSX_EINVAL: a NULL array, an mss of
 * 0, decreasing data offsets, n >= 2^32). nsx_tso_layout_host writes
 * h_frame_seg and the packed offsets nsx_tx_layout_host would give the expanded
 * batch, h_out_off[f] = sum of round_up4(ip_hdr_len + wire) over the frames
 * before f (NSX_EINVAL as above, for decreasing option offsets, ip_hdr_len other
 * than 20 or 40, and an h_frame_first that is not nsx_tso_count_host's).
 * h_opt_off is nullable in both the layout and the build calls.
 * d_tcp_raw (nullable) has n_frames entries. The device calls validate their
 * pointers as the transmit pass does, return NSX_OK without a launch when
 * n_frames == 0, and do no allocation, no host sync and use no per-stream
 * counters: they can be captured into a graph. data_bytes = the extent of
 * d_data, as in nsx_tcp_build_dev.
 * There is no segmenting form of the IP-less nsx_tcp_build_dev: its caller-made
 * pseudo-header partial depends on each frame's own length, so it cannot be
 * given once per super-segment. */
int nsx_tso_count_host(const uint64_t* h_data_off, const uint32_t* h_mss, uint64_t n, uint64_t* h_frame_first);
int nsx_tso_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, const uint32_t* h_mss,
                        const uint64_t* h_frame_first, uint64_t n, uint32_t ip_hdr_len, uint32_t* h_frame_seg,
                        uint64_t* h_out_off);
int nsx_tso_ipv4_tcp_build_dev(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                               const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                               uint64_t data_bytes, const uint32_t* d_mss, uint64_t n,
                               const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                               uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_tcp_raw, nsx_stream_t stream);
int nsx_tso_ipv6_tcp_build_dev(const nsx_ip_hdr_soa* ip, const nsx_tcp_hdr_soa* tcp, const uint8_t* d_opts,
                               const uint64_t* d_opt_off, const uint8_t* d_data, const uint64_t* d_data_off,
                               uint64_t data_bytes, const uint32_t* d_mss, uint64_t n,
                               const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                               uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_tcp_raw, nsx_stream_t stream);

/* UDP (RFC 768; over IPv6 RFC 8200 §8.1): the fused transmit pass, its
 * segmentation offload and the receive verify for the other transport — the
 * twins of nsx_tx_*, nsx_tso_* and nsx_rx_* above, as kernels of their own
 * (csrc/udp_kernels.hip). The checksum is the same computeChecksum sum
 * (tcp.go:72-95) with three rules TCP does not have: a computed checksum of 0
 * is sent as 0xFFFF (RFC 768); a received field of 0 means "no checksum" on
 * IPv4 (RFC 768); a received field of 0 is illegal on IPv6 (RFC 8200 §8.1).
 * There are device calls only: no _host forms and no sharding; receive
 * coalescing is nsx_ugro_* below (UDP receive coalescing), the NAT rewrite stays
 * TCP; UDP-Lite, IPv6 zero-checksum tunnels
 * (RFC 6935) and extension headers are not handled.
 *
 * Transmit (nsx_udp_tx_ipv4_build_dev / nsx_udp_tx_ipv6_build_dev): n frames
 * from the per-frame IP fields of nsx_ip_hdr_soa (as the TCP transmit pass: the
 * same device arrays, the same NULL defaults), the ports of nsx_udp_hdr_soa
 * (device arrays, host byte order) and the payload d_data[d_data_off[i],
 * d_data_off[i+1]) at any source alignment; data_bytes = the extent of d_data.
 * Frame i is written at d_out + d_out_off[i] under the transmit pass's layout
 * rule: d_out_off[i] a multiple of 4 with room for the frame rounded up to 4
 * bytes, the up to 3 bytes after a frame zero-filled, everything else left as
 * it was. The frame:
 *   IP header   exactly the one nsx_tx_ipv4_tcp_build_dev /
 *               nsx_tx_ipv6_tcp_build_dev writes (IPv4: 0x45, 0x00, total
 *               length, ident, 0x40 0x00, ttl, protocol, header checksum, src,
 *               dst; IPv6: version 6, tclass, flow, payload length, Next
 *               Header, hop limit ttl, src, dst), with the protocol / Next
 *               Header byte 17 and the length that of the UDP datagram (IPv4
 *               total length 20 + 8 + payload, IPv6 payload length 8 + payload).
 *   UDP header  8 bytes, big-endian: source port, destination port, length =
 *               8 + payload, checksum.
 *   payload     the bytes of d_data, unchanged.
 * Checksum: raw is the computeChecksum sum over the pseudo-header ‖ the
 * datagram (UDP header and payload) with the field zero. The IPv4
 * pseudo-header is src(4) dst(4) 0 17 UDP length(2); the IPv6 one is that of
 * RFC 8200 §8.1: src(16) dst(16), the UDP length as a 4-byte field, 3 zero
 * bytes, Next Header 17. The stored field is ~raw, except that 0x0000 is stored
 * as 0xFFFF. d_udp_raw[i] (nullable) receives raw.
 * flags: NSX_UDP_NO_CSUM (bit 0, IPv4 only) stores the field 0 ("not computed",
 * RFC 768) in every frame; d_udp_raw still receives raw. On IPv6 it is
 * NSX_EINVAL, and so is any other flag bit on either version.
 * A payload above 65507 bytes (IPv4) or 65527 bytes (IPv6) does not fit the
 * length fields and is not built: nothing is written for that frame, padding
 * included, and its raw is 0. A built frame's raw is never 0 (the pseudo-header
 * holds the byte 17). That holds for any length the 64-bit offsets can say, 2^32
 * bytes and more included.
 * nsx_udp_layout_host gives the packed offsets: h_out_off[i] = Σ_{j<i}
 * round_up4(ip_hdr_len + 8 + len_j), n + 1 entries, ip_hdr_len 20 or 40
 * (NSX_EINVAL otherwise, for a NULL array and for decreasing offsets; nothing
 * is written then).
 * Conventions of the device calls, as the transmit pass: everything is
 * validated before any launch (NSX_EINVAL: ip or udp NULL, ip->src, ip->dst or
 * a port array NULL, d_data_off / d_out / d_out_off NULL, d_data NULL with
 * data_bytes nonzero, a bad flag); n == 0 is NSX_OK without a launch;
 * NSX_ENODEV without a GPU. No allocation, no host sync, no per-stream
 * counters: the calls can be captured into a graph.
 *
 * Segmentation offload (nsx_udp_uso_ipv4_build_dev / nsx_udp_uso_ipv6_build_dev;
 * Linux UDP_SEGMENT, __udp_gso_segment): n super-datagrams in, n_frames
 * datagrams out. Super-datagram s has one entry in every nsx_ip_hdr_soa /
 * nsx_udp_hdr_soa array, the payload d_data[d_data_off[s], d_data_off[s+1]) of
 * len_s bytes and d_gso[s] >= 1, the payload bytes per datagram. The frame map
 * is segmentation offload's own: nsx_tso_count_host(h_data_off, h_gso, n,
 * h_frame_first) is used as it stands — cnt_s = max(1, ceil(len_s / gso_s)),
 * frame_first (n + 1) its prefix sum, frame_seg (n_frames) the super-datagram
 * of each frame, out_off (n_frames + 1) the frame slots.
 * nsx_udp_uso_layout_host writes h_frame_seg and the packed offsets
 * nsx_udp_layout_host would give the expanded batch, with nsx_tso_layout_host's
 * NSX_EINVAL cases: a NULL array, a gso of 0, decreasing offsets, n >= 2^32,
 * ip_hdr_len other than 20 or 40, and an h_frame_first that is not
 * nsx_tso_count_host's.
 * Frame j of s (0 <= j < cnt_s) is exactly the frame nsx_udp_tx_* builds from
 * s's fields, except:
 *   payload   d_data[d_data_off[s] + j*gso, min(d_data_off[s] + (j+1)*gso,
 *             d_data_off[s+1])) — empty when len_s == 0. The kernel reads no
 *             payload byte outside s's own range, whatever the frame map says
 *             (j = f - frame_first[frame_seg[f]] modulo 2^64; a slice that would
 *             start past the range is empty).
 *   ident     IPv4: (ident[s] + j) modulo 2^16, ident[s] = 0 when the array is
 *             NULL.
 * The UDP length, the IP length, the IPv4 header checksum and the UDP checksum
 * follow from the frame's own slice; ports, addresses, TTL, traffic class and
 * flow label are copied to every frame. flags, d_udp_raw (n_frames entries)
 * and the not-built rule as above. The device calls return NSX_OK without a
 * launch when n_frames == 0; else n == 0, n >= 2^32, n_frames < n and a NULL
 * d_gso / d_frame_first / d_frame_seg are NSX_EINVAL too.
 *
 * Receive verify (nsx_udp_rx_ipv4_verify_dev / nsx_udp_rx_ipv6_verify_dev):
 * input as nsx_rx_ipv4_tcp_verify_dev — densely packed frames at any alignment,
 * frame i = d_base[d_offsets[i], d_offsets[i+1]), d_offsets with n + 1 entries.
 * Bit (i % 64) of d_mask[i / 64] is set iff frame i
 *   - is well-formed. IPv4: version 4, IHL >= 5, IHL*4 <= frame length, total
 *     length == frame length, MF clear and fragment offset 0, protocol 17.
 *     IPv6: at least 48 bytes, version 6, 40 + payload length == frame length,
 *     Next Header 17 (extension headers are not walked). Both: with P the IP
 *     payload length (frame length less the IP header) and U the UDP length
 *     field, 8 <= U <= P. Bytes past U are padding and are ignored, as Linux
 *     trims them;
 *   - IPv4 only: has a valid header checksum — raw over the IHL*4 header bytes
 *     is 0xFFFF;
 *   - has a valid UDP checksum: raw is taken over the pseudo-header built from
 *     the frame's own addresses, 17 and U ‖ the first U bytes of the datagram;
 *     raw == 0xFFFF verifies. On IPv4 a checksum field of 0 also verifies,
 *     whatever raw is. On IPv6 a field of 0 does not verify, whatever raw is.
 * d_ip_raw (IPv4, nullable) is as in the TCP pass: the header's raw sum, 0 when
 * the frame holds fewer than 20 bytes, IHL < 5 or IHL*4 exceeds the frame.
 * d_udp_raw (nullable) is that raw, 0 unless the frame is well-formed. Bits
 * past n in the last word are 0; d_mask holds ceil(n/64) words. No byte outside
 * a frame's own range is read. The split over the GPU's waves is static — a wave
 * per mask word, no per-stream deal counters — so the call can be captured into
 * a graph on any stream. n == 0 is NSX_OK without a launch; a NULL d_base,
 * d_offsets or d_mask is NSX_EINVAL; NSX_ENODEV without a GPU. */
typedef struct {
    const uint16_t* src_port;  /* n entries, host byte order */
    const uint16_t* dst_port;
} nsx_udp_hdr_soa;             /* device arrays */
#define NSX_UDP_NO_CSUM 1u     /* flags bit 0, IPv4 only: send checksum field 0 ("not computed", RFC 768) */

int nsx_udp_layout_host(const uint64_t* h_data_off, uint64_t n, uint32_t ip_hdr_len, uint64_t* h_out_off);
int nsx_udp_uso_layout_host(const uint64_t* h_data_off, const uint32_t* h_gso, const uint64_t* h_frame_first,
                            uint64_t n, uint32_t ip_hdr_len, uint32_t* h_frame_seg, uint64_t* h_out_off);
int nsx_udp_tx_ipv4_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                              const uint64_t* d_data_off, uint64_t data_bytes, uint64_t n, uint32_t flags,
                              uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw, nsx_stream_t stream);
int nsx_udp_tx_ipv6_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                              const uint64_t* d_data_off, uint64_t data_bytes, uint64_t n, uint32_t flags,
                              uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw, nsx_stream_t stream);
int nsx_udp_uso_ipv4_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                               const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso, uint64_t n,
                               const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                               uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw,
                               nsx_stream_t stream);
int nsx_udp_uso_ipv6_build_dev(const nsx_ip_hdr_soa* ip, const nsx_udp_hdr_soa* udp, const uint8_t* d_data,
                               const uint64_t* d_data_off, uint64_t data_bytes, const uint32_t* d_gso, uint64_t n,
                               const uint64_t* d_frame_first, const uint32_t* d_frame_seg, uint64_t n_frames,
                               uint32_t flags, uint8_t* d_out, const uint64_t* d_out_off, uint16_t* d_udp_raw,
                               nsx_stream_t stream);
int nsx_udp_rx_ipv4_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_ip_raw, uint16_t* d_udp_raw, nsx_stream_t stream);
int nsx_udp_rx_ipv6_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_udp_raw, nsx_stream_t stream);

/* IPv4 header checksums (RFC 791 §3.1; SURVEY.md §8 f3 — the reference has no
 * IPv4 header codec, network/ip/v4/ipv4.go holds addresses only). Packet i's
 * header starts at d_base + i*stride + hdr_off (any alignment) and is IHL*4
 * bytes, IHL = low nibble of its first byte.
 *   mode 0 (receive): d_out_raw[i] = raw sum over the header as it stands;
 *          the header is valid iff it is 0xFFFF.
 *   mode 1 (send):    d_out_raw[i] (nullable) = raw sum with bytes 10-11 taken
 *          as zero, and ~raw is written big-endian into bytes 10-11 in place.
 * A malformed header (IHL < 5, or hdr_off + IHL*4 > stride) yields 0 and is
 * left untouched. At least 20 bytes must be readable at every header start;
 * stride and hdr_off ≤ 2^22 (NSX_EINVAL otherwise). */
int nsx_ipv4_hdr_csum_dev(void* d_base, uint64_t stride, uint32_t hdr_off, uint64_t n, int mode,
                          uint16_t* d_out_raw, nsx_stream_t stream);

/* IPv4 header verify straight into a bitmask (the receive side of f3 fused with
 * the f2 mask convention, tcp.go:70 rule applied to RFC 791 headers): bit
 * (i % 64) of d_mask[i / 64] is set iff header i is well-formed and its raw sum
 * is 0xFFFF (= nsx_ipv4_hdr_csum_dev mode 0 followed by nsx_verify_mask_dev,
 * one pass, 1 bit written per header instead of 16); bits past n in the last
 * word are 0. d_mask holds ceil(n/64) words. Same layout rules and limits as
 * nsx_ipv4_hdr_csum_dev; the headers are only read. */
int nsx_ipv4_hdr_verify_mask_dev(const void* d_base, uint64_t stride, uint32_t hdr_off, uint64_t n,
                                 uint64_t* d_mask, nsx_stream_t stream);

/* Fused receive pass (SURVEY.md §8 f2 + f3 in one launch): n received IPv4
 * datagrams carrying TCP, densely packed — frame i = d_base[d_offsets[i],
 * d_offsets[i+1]), any alignment, d_offsets as for nsx_csum_ragged_dev. Bit
 * (i % 64) of d_mask[i / 64] is set iff frame i
 *   - is a well-formed, unfragmented IPv4 datagram carrying TCP: version 4,
 *     IHL >= 5, IHL*4 <= frame length, total length (bytes 2-3) == frame
 *     length, MF clear and fragment offset 0 (a fragment's TCP checksum covers
 *     bytes it does not hold), protocol 6 (ip.NextProtoTCP,
 *     network/ip/protocols.go:8), and a TCP segment (total − IHL*4 bytes) of at
 *     least 20 bytes (tcp.go:131, minSegmentLength);
 *   - has a valid header checksum: the raw sum over its IHL*4 header bytes is
 *     0xFFFF (RFC 791 §3.1);
 *   - has a valid TCP checksum: the raw sum over the pseudo-header built from
 *     the header's own source and destination (ip.Addr.Raw(),
 *     network/ip/v4/ipv4.go:15), 0, 6, TCP length ‖ the segment is 0xFFFF
 *     (tcp.go:70 receiver rule over computeChecksum, tcp.go:72-95).
 * Bits past n in the last word are 0; d_mask holds ceil(n/64) words.
 * d_ip_raw (nullable): the header's raw sum (0 when IHL < 5 or IHL*4 exceeds the
 * frame). d_tcp_raw (nullable): the raw sum over pseudo-header ‖ segment (0
 * unless the frame is well-formed as above). One pass over the frame bytes.
 * Work split: the batch's last eighth of frames is dealt to the GPU's waves as
 * they finish, from counters the library keeps per stream (64 streams per
 * device, in the library's own device memory; every launch leaves them at zero
 * for the stream's next, so launches sharing them must run one after another).
 * Only a handle that is one ordered queue of the current device gets counters:
 * a stream the caller created, or the null stream. hipStreamPerThread (one
 * handle, a different stream per host thread), a stream of another device, a
 * stream being captured into a graph, and streams past the 64th split the
 * batch statically instead; results are the same either way. See
 * nsx_stream_release. */
int nsx_rx_ipv4_tcp_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_ip_raw, uint16_t* d_tcp_raw, nsx_stream_t stream);

/* The same receive pass for IPv6 (the IPv6 pseudo-header of
 * ip.Addr.Raw(), network/ip/v6/ipv6.go:16): frame i is an IPv6 packet whose
 * fixed 40-byte header (RFC 8200 §3) is followed directly by a TCP segment.
 * Bit (i % 64) of d_mask[i / 64] is set iff frame i
 *   - is well-formed: at least 40 bytes, version 6, 40 + payload length (bytes
 *     4-5) == frame length, Next Header (byte 6) == 6 (ip.NextProtoTCP; a
 *     packet with extension headers is not walked and does not verify), and a
 *     payload of at least 20 bytes (tcp.go:131);
 *   - has a valid TCP checksum: the raw sum over the RFC 8200 §8.1 pseudo-header
 *     src(16) dst(16) payload length(4) 0 0 0 6 from the header's own addresses
 *     ‖ the segment is 0xFFFF (tcp.go:70 over computeChecksum, tcp.go:72-95).
 * IPv6 has no header checksum. d_tcp_raw (nullable): that raw sum, 0 unless the
 * frame is well-formed. Layout rules and work split as
 * nsx_rx_ipv4_tcp_verify_dev. */
int nsx_rx_ipv6_tcp_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                               uint16_t* d_tcp_raw, nsx_stream_t stream);

/* TCP receive coalescing (GRO), the inverse of segmentation offload: the frames
 * of a receive batch in, super-segments out — per run of consecutive in-order
 * frames of one connection one set of header fields, one option block and one
 * contiguous payload run, in exactly the arrays nsx_tso_ipv4_tcp_build_dev /
 * nsx_tso_ipv6_tcp_build_dev take. Input as the receive pass: d_base, d_offsets
 * (n + 1), n, and d_valid, that pass's bitmask over the same frames (required).
 *
 * Member. Frame i is a member iff its d_valid bit is set, it is well-formed as
 * the receive pass of its IP version defines (the length, version, protocol and
 * fragment conditions above — re-checked here, so a wrong mask never makes the
 * kernels read outside the frame's own byte range, nor a frame whose bit is
 * clear at all), and its TCP data offset doff (high nibble of byte 12) has
 * 5 <= doff and doff*4 <= TCP segment length, which the receive pass does not
 * check. A non-member belongs to no super-segment and breaks runs. For a member:
 * pay_i = segment length - doff*4; c_i = the control byte (byte 13); its option
 * bytes are segment bytes [20, doff*4) verbatim, padding included (a multiple
 * of 4 bytes).
 *
 * same(i, i-1), purely pairwise, holds iff both frames are members; src, dst and
 * TTL / hop limit are equal; IPv4: both have IHL 5, equal TOS, equal bytes 6-7,
 * and ident_i == ident_{i-1} + 1 mod 2^16; IPv6: the first 4 header bytes
 * (version, class, flow) are equal; the TCP ports, ack, window and urgent
 * pointer are equal; byte 12 is equal and the option bytes are identical;
 * seq_i == seq_{i-1} + pay_{i-1} mod 2^32; c_{i-1} & (FIN|SYN|RST|PSH|URG) == 0;
 * c_i & (SYN|RST|URG|CWR) == 0; and (c_i ^ c_{i-1}) & ~(FIN|PSH|CWR) == 0.
 *
 * join(i) — frame i continues frame i-1's super-segment — holds iff
 * same(i, i-1), 1 <= pay_i <= pay_{i-1}, and NOT (i >= 2 and same(i-1, i-2) and
 * pay_{i-1} < pay_{i-2}). The last clause is a three-frame window, not a
 * recursion: frame i-1 was itself a short tail. Every frame of a run but the
 * last therefore carries the same payload length; strictly decreasing runs lose
 * a few merges (1000, 800, 600, 400, 200 gives [1000, 800], [600], [400],
 * [200]). A member that does not join is a head. Super-segments are numbered in
 * frame order; n_super = the number of heads.
 *
 * Coalescing is by adjacency only: these calls keep no flow table, so they merge
 * a flow's frames only where they arrive back to back. For a queue on which many
 * connections interleave, nsx_gro_flow_ipv4_tcp_dev / nsx_gro_flow_ipv6_tcp_dev
 * below coalesce per connection. A super-segment has no IP length field, so
 * there is no 64 KiB cap on it.
 *
 * Every member of nsx_gro_out is a writable device array and required. For
 * super-segment s with first frame f and last frame l, all written:
 *   src, dst, ident (IPv4; 0 for IPv6), ttl, tclass (IPv4: the TOS byte), flow
 *     (IPv6; 0 for IPv4) from f — n x 4 (IPv4) or n x 16 (IPv6) address bytes;
 *   src_port, dst_port, seq_num, ack_num, window, urgent_ptr and offset (the
 *     whole byte 12) from f; control = c_f | (c_l & (FIN|PSH));
 *   mss[s] = max(pay_f, 1);
 *   opts[opt_off[s], opt_off[s+1]) = f's option bytes;
 *   data[data_off[s], data_off[s+1]) = the payloads of f..l back to back;
 *   first_frame[s] = f; frame_cnt[s] = l - f + 1.
 * opt_off[0] = data_off[0] = 0 and both are packed without gaps (n_super + 1
 * entries). frame_seg[i] = frame i's super-segment, 0xFFFFFFFF for a non-member.
 * *n_super is a uint64_t in device memory. Per-super-segment entries at index
 * >= n_super, offset entries past n_super, and data / opts bytes past the last
 * offset are left exactly as they were. Worst-case extents: n entries per
 * array, n + 1 offsets, d_offsets[n] - d_offsets[0] data bytes, 40*n option
 * bytes.
 *
 * The defining property: for frames the transmit pass can express (IPv4 with
 * IHL 5, DF set, MF clear and TOS 0; any IPv6 frame with Next Header 6), the
 * output arrays go straight into nsx_tso_ipv4_tcp_build_dev /
 * nsx_tso_ipv6_tcp_build_dev (frame_first = the prefix sum of frame_cnt) and
 * rebuild every member frame byte for byte. What nsx_ip_hdr_soa cannot carry is
 * lost: IPv4 options (such a frame is a singleton, its options dropped), a
 * clear DF bit and a nonzero TOS (kept in tclass, which the IPv4 transmit pass
 * ignores).
 *
 * nsx_gro_work_bytes gives the scratch one call over n frames needs; d_work is
 * device memory of at least that many bytes, free for reuse once the stream has
 * run the call. NSX_EINVAL, checked before any launch: a NULL pointer or
 * member (d_base and d_valid may be NULL when n == 0), n >= 2^32 - 1,
 * work_bytes too small. Then NSX_ENODEV without a GPU.
 * n == 0 writes *n_super = 0 and opt_off[0] = data_off[0] = 0, on the stream like
 * everything else. No allocation, no host sync, no per-stream counters: the
 * calls can be captured into a graph. There are no _host forms and no
 * multi-GPU sharding (a run would straddle a shard boundary). */
typedef struct {
    uint64_t* n_super;
    uint8_t*  src;          /* nsx_ip_hdr_soa members */
    uint8_t*  dst;
    uint16_t* ident;
    uint8_t*  ttl;
    uint8_t*  tclass;
    uint32_t* flow;
    uint16_t* src_port;     /* nsx_tcp_hdr_soa members */
    uint16_t* dst_port;
    uint32_t* seq_num;
    uint32_t* ack_num;
    uint8_t*  offset;
    uint8_t*  control;
    uint16_t* window;
    uint16_t* urgent_ptr;
    uint32_t* mss;
    uint8_t*  opts;
    uint64_t* opt_off;
    uint8_t*  data;
    uint64_t* data_off;
    uint64_t* first_frame;
    uint32_t* frame_cnt;
    uint32_t* frame_seg;    /* per frame */
} nsx_gro_out;

int nsx_gro_work_bytes(uint64_t n, uint64_t* out);
int nsx_gro_ipv4_tcp_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                         const nsx_gro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream);
int nsx_gro_ipv6_tcp_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                         const nsx_gro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream);

/* Flow-keyed receive coalescing: nsx_gro_* per connection, however the
 * connections interleave in the batch (RSS hashes many connections onto one
 * queue). The frames are put in a stable order by a 32-bit flow key, and the
 * rules above, unchanged, run over that order. A key collision therefore never
 * makes a wrong merge — same() still compares every field — it only costs
 * merges. Arguments as nsx_gro_*, plus d_order (n entries, an output).
 *
 * Flow key. The key of a non-member (Member above) is 0xFFFFFFFF; a frame whose
 * d_valid bit is clear is not read at all, and of a frame whose bit is set at
 * most the IP header and the first 16 TCP bytes are read, never a byte outside
 * the frame's own range. For a member take these little-endian dwords in order:
 * IPv4 the IP header's bytes 12-15 and 16-19 (src, dst), IPv6 its bytes 8-39
 * (8 dwords); then TCP bytes 0-3 (the ports). h = 0x811C9DC5; for each dword w,
 * h = ((h ^ w) * 0x01000193) mod 2^32; key = h. A member whose hash happens to
 * be 0xFFFFFFFF keeps that key: it sorts among the non-members and merely loses
 * merges.
 *
 * Order. d_order = the stable ascending sort of the frame indices 0..n-1 by
 * key: equal keys keep arrival order (numpy.argsort(keys, kind="stable"), bit
 * for bit). So a connection's frames become consecutive, in arrival order;
 * super-segments come out grouped by key, not by arrival; non-members come last.
 *
 * Outputs. Let B' be the batch whose frame p is frame d_order[p] of the input,
 * with valid'[p] = valid[d_order[p]]. Every member of nsx_gro_out is exactly
 * what nsx_gro_ipvX_tcp_dev writes over B' — the regions left untouched
 * included — except:
 *   first_frame[s] is a position: super-segment s consists of the frames
 *     d_order[first_frame[s] + j], 0 <= j < frame_cnt[s];
 *   frame_seg stays indexed by the original frame:
 *     frame_seg[d_order[p]] = frame_seg'[p].
 * Fed to nsx_tso_*_build_dev (frame_first = the prefix sum of frame_cnt,
 * frame_seg = frame_seg', that is frame_seg gathered through d_order), the
 * outputs rebuild at output position p frame d_order[p] byte for byte, for the
 * frames the transmit pass can express (the condition above).
 *
 * nsx_gro_flow_work_bytes(n) >= nsx_gro_work_bytes(n) gives the scratch, for
 * every tune setting. NSX_EINVAL before any launch: a NULL pointer or member
 * (d_base, d_valid and d_order may be NULL when n == 0), n >= 2^32 - 1,
 * work_bytes too small. Then NSX_ENODEV without a GPU. n == 0 behaves as
 * nsx_gro_* and does not write d_order. No allocation, no host sync, no
 * per-stream counters; the call is one serial chain of launches and can be
 * captured into a graph. The return type stands on a line of its own in these
 * declarations: nsx_gro_* above is a closed set of three. */
int
nsx_gro_flow_work_bytes(uint64_t n, uint64_t* out);
int
nsx_gro_flow_ipv4_tcp_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                          uint32_t* d_order, const nsx_gro_out* out, void* d_work, uint64_t work_bytes,
                          nsx_stream_t stream);
int
nsx_gro_flow_ipv6_tcp_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                          uint32_t* d_order, const nsx_gro_out* out, void* d_work, uint64_t work_bytes,
                          nsx_stream_t stream);

/* UDP receive coalescing (Linux UDP_GRO), the inverse of UDP segmentation
 * offload: the datagrams of a receive batch in, super-datagrams out — per run of
 * consecutive datagrams of one flow one set of header fields and one contiguous
 * payload run, in exactly the arrays nsx_udp_uso_ipv4_build_dev /
 * nsx_udp_uso_ipv6_build_dev take. nsx_ugro_ipv4_dev / nsx_ugro_ipv6_dev
 * coalesce by adjacency, as nsx_gro_* does for TCP; nsx_ugro_flow_ipv4_dev /
 * nsx_ugro_flow_ipv6_dev coalesce per flow, as nsx_gro_flow_* does. Kernels of
 * their own (csrc/ugro_kernels.hip); the TCP calls are untouched.
 *
 * Input as nsx_gro_*: d_base, d_offsets (n + 1 entries), n, and d_valid, the
 * bitmask of nsx_udp_rx_ipv4_verify_dev / nsx_udp_rx_ipv6_verify_dev over the
 * same frames (required).
 *
 * UDP member. Frame i is a member iff its d_valid bit is set; it is well-formed
 * as the UDP receive verify defines (version, lengths, protocol / Next Header
 * 17, no fragment, and with P the IP payload length and U the UDP length field,
 * 8 <= U <= P — re-checked here, so a wrong mask never makes a kernel read
 * outside the frame's own byte range, and a frame whose bit is clear is not
 * read at all); U == P, no padding past the UDP length; and its UDP checksum
 * field is not 0 (Linux udp_gro_receive_segment also requires a nonzero
 * checksum, "for symmetry with GSO"). A non-member belongs to no
 * super-datagram: its frame_seg is 0xFFFFFFFF and it breaks runs. For a member
 * pay_i = U - 8.
 *
 * UDP same(i, i-1), purely pairwise, holds iff both frames are members; src,
 * dst and TTL / hop limit are equal; IPv4: both have IHL 5, equal TOS, equal
 * bytes 6-7, and ident_i == ident_{i-1} + 1 mod 2^16; IPv6: the first 4 header
 * bytes (version, class, flow) are equal; and both UDP ports are equal.
 *
 * join(i) is the three-frame window of nsx_gro_*, word for word: it holds iff
 * same(i, i-1), 1 <= pay_i <= pay_{i-1}, and NOT (i >= 2 and same(i-1, i-2) and
 * pay_{i-1} < pay_{i-2}). Every datagram of a run but the last therefore has
 * the same payload length (1000, 800, 600, 400, 200 gives [1000, 800], [600],
 * [400], [200]). A member that does not join is a head; super-datagrams are
 * numbered in frame order; n_super = the number of heads. There is no
 * 64-datagram cap and no 64 KiB cap on a super-datagram, unlike Linux's
 * UDP_GRO_CNT_MAX: it has no length field.
 *
 * Every member of nsx_ugro_out is a writable device array and required. For
 * super-datagram s with first frame f and last frame l, all written:
 *   src, dst, ident (IPv4; 0 for IPv6), ttl, tclass (IPv4: the TOS byte), flow
 *     (IPv6; 0 for IPv4), src_port and dst_port from f, exactly as nsx_gro_out
 *     takes them from f — n x 4 (IPv4) or n x 16 (IPv6) address bytes;
 *   gso[s] = max(pay_f, 1);
 *   data[data_off[s], data_off[s+1]) = the payloads of f..l back to back;
 *   first_frame[s] = f; frame_cnt[s] = l - f + 1.
 * data_off[0] = 0 and the offsets are packed without gaps (n_super + 1 entries).
 * frame_seg[i] = frame i's super-datagram, 0xFFFFFFFF for a non-member.
 * *n_super is a uint64_t in device memory. Entries at index >= n_super, offset
 * entries past n_super, and data bytes past the last offset are left exactly
 * as they were. Worst-case extents: n entries per array, n + 1 offsets,
 * d_offsets[n] - d_offsets[0] data bytes.
 *
 * Flow-keyed form, related to the adjacent form exactly as nsx_gro_flow_* is to
 * nsx_gro_*: the UDP flow key is FNV-1a as defined there (h = 0x811C9DC5; for
 * each dword w, h = ((h ^ w) * 0x01000193) mod 2^32) over the little-endian
 * address dwords (IPv4 header bytes 12-19, IPv6 header bytes 8-39), then the
 * dword holding the two UDP ports (UDP bytes 0-3); a non-member gets
 * 0xFFFFFFFF. Of a frame whose bit is set at most the IP header and the 8 UDP
 * header bytes are read for the key. d_order (n entries, an output) is the
 * stable ascending sort of the frame indices by key, bit for bit
 * numpy.argsort(keys, kind="stable"); the rules above run over that order;
 * first_frame[s] is a position in d_order; frame_seg stays indexed by the
 * original frame (frame_seg[d_order[p]] = frame_seg'[p]). A key collision
 * costs merges and never merges wrongly. nsx_ugro_flow_work_bytes(n) >=
 * nsx_ugro_work_bytes(n) for every tune setting.
 *
 * The defining property of UDP coalescing: for frames the UDP transmit pass can
 * express (IPv4 with IHL 5, bytes 6-7 == 0x40 0x00 and TOS 0; any IPv6 member),
 * the outputs go straight into nsx_udp_uso_ipv4_build_dev /
 * nsx_udp_uso_ipv6_build_dev with flags 0 (frame_first = the prefix sum of
 * frame_cnt; frame_seg as it stands for the adjacent form over a batch of
 * members, gathered through d_order for the flow-keyed one) and rebuild every
 * member frame byte for byte, the UDP checksum included: a verified nonzero
 * field is exactly what the transmit pass stores, 0xFFFF where the field-zero
 * raw sum is 0xFFFF. IPv4 options, a clear DF bit and a nonzero TOS are lost,
 * as for TCP. A datagram whose IPv4 checksum field is 0 is valid to the verify
 * but could not be rebuilt by a pass that computes checksums, so it stays a
 * non-member; so does a padded datagram.
 *
 * Validation and conventions as nsx_gro_* and nsx_gro_flow_*: NSX_EINVAL before
 * any launch for a NULL pointer or struct member, n >= 2^32 - 1, or work_bytes
 * too small (d_base and d_valid, and d_order for the flow-keyed form, may be
 * NULL when n == 0); then NSX_ENODEV without a GPU. n == 0 writes *n_super = 0
 * and data_off[0] = 0 on the stream and does not write d_order. No allocation,
 * no host sync, no per-stream counters: each call is one serial chain of
 * launches and can be captured into a graph. 64-bit offsets throughout: frames
 * may lie past 2^32 in d_base. There are no _host forms and no sharding. The
 * _tuned twins are in nsx_ugro_tune.h. */
typedef struct {
    uint64_t* n_super;
    uint8_t*  src;          /* nsx_ip_hdr_soa members */
    uint8_t*  dst;
    uint16_t* ident;
    uint8_t*  ttl;
    uint8_t*  tclass;
    uint32_t* flow;
    uint16_t* src_port;     /* nsx_udp_hdr_soa members */
    uint16_t* dst_port;
    uint32_t* gso;
    uint8_t*  data;
    uint64_t* data_off;
    uint64_t* first_frame;
    uint32_t* frame_cnt;
    uint32_t* frame_seg;    /* per frame */
} nsx_ugro_out;

int nsx_ugro_work_bytes(uint64_t n, uint64_t* out);
int nsx_ugro_flow_work_bytes(uint64_t n, uint64_t* out);
int nsx_ugro_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                      const nsx_ugro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream);
int nsx_ugro_ipv6_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                      const nsx_ugro_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream);
int nsx_ugro_flow_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                           uint32_t* d_order, const nsx_ugro_out* out, void* d_work, uint64_t work_bytes,
                           nsx_stream_t stream);
int nsx_ugro_flow_ipv6_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                           uint32_t* d_order, const nsx_ugro_out* out, void* d_work, uint64_t work_bytes,
                           nsx_stream_t stream);

/* In-place NAT rewrite with incremental checksum update (RFC 1071 §2(4),
 * RFC 1624): the frames of a receive batch, that pass's validity mask and a
 * translation table in; the same frames out, the matching ones with new
 * addresses, ports and TTL / hop limit and both checksums corrected from the
 * old and new field values alone — the payload is neither read nor written. A
 * bitmask says which frames were translated. Input as the receive pass: d_base
 * (written here), d_offsets (n + 1), n, and d_valid, that pass's bitmask over
 * the same frames (required).
 *
 * Tuple. The bytes as they stand on the wire. IPv4: 12 bytes — IP header bytes
 * 12-19 (src, dst), then TCP bytes 0-3 (the two ports; the TCP header starts
 * IHL*4 bytes into the frame). IPv6: 36 bytes — IP header bytes 8-39, then TCP
 * bytes 0-3 (frame bytes 40-43). h_match and h_new are n_rules tuples each,
 * packed: rule r turns the tuple h_match[r] into the tuple h_new[r].
 *
 * Table. slots entries, slots a power of two; an entry is two tuples with a
 * state dword between them:
 *                                IPv4 (32 B per entry)   IPv6 (80 B per entry)
 *   match tuple                  bytes 0-11              bytes 0-35
 *   state (little-endian dword)  bytes 12-15             bytes 36-39
 *   new tuple                    bytes 16-27             bytes 40-75
 *   zero                         bytes 28-31             bytes 76-79
 * State 1 means occupied; any other state value means empty. The table base
 * must be 16-byte aligned (NSX_EINVAL otherwise).
 *
 * Hash. h = 0x811C9DC5; for each little-endian dword w of the tuple, in order
 * (3 dwords for IPv4, 9 for IPv6), h = ((h ^ w) * 0x01000193) mod 2^32; the home
 * slot is h & (slots - 1). This is the same key that nsx_gro_flow_* defines for
 * a member: FNV-1a over the address dwords, then the ports.
 *
 * Lookup. Probe home, home + 1, ... modulo slots. The first entry that is not
 * occupied ends the lookup with a miss; an occupied entry whose match tuple
 * equals the frame's tuple, all of its bytes, is a hit (the hash alone is never
 * a match); after slots probes the lookup is a miss. This is a total function
 * of arbitrary table bytes: a table without an empty entry costs slots probes
 * per frame and nothing else.
 *
 * nsx_nat_table_slots gives the smallest power of two >= max(16, 2*n_rules)
 * (NSX_EINVAL: a NULL out_slots, n_rules >= 2^31). nsx_nat_table_build_host
 * zero-fills the slots entries at h_table and inserts the rules in order, each
 * into the first entry its lookup finds not occupied. NSX_EINVAL: ip_ver not 4
 * or 6; a NULL h_match or h_new with n_rules > 0, a NULL h_table; slots not a
 * power of two, slots < 2*n_rules, slots < 16 or slots > 2^31; two rules with
 * the same match tuple (the table's contents are then unspecified). Host
 * memory only, no GPU needed; the caller copies the table to the device.
 *
 * Rewrite. Frame i is translated iff its d_valid bit is set; it is well-formed
 * as the receive pass of its IP version defines (the length, version, protocol
 * and fragment conditions above — re-checked here, so a wrong mask never makes
 * the kernel touch a byte outside the frame's own range, nor a frame whose bit
 * is clear at all); its TTL (IPv4 byte 8) / hop limit (IPv6 byte 7) t satisfies
 * t > ttl_dec; and its tuple hits the table. ttl_dec > 255 is NSX_EINVAL,
 * ttl_dec = 0 is allowed. The TCP data offset is not looked at. IPv4 frames
 * with IP options (IHL > 5) are translated like any other. A frame that is not
 * translated is left byte for byte as it was. Bit (i % 64) of d_hit[i / 64] is
 * set iff frame i was translated; bits past n are 0; d_hit has ceil(n/64) words
 * and is required. No byte outside a translated frame's own range is written,
 * whatever the alignment of the frames.
 *
 * A translated frame changes only in: TTL / hop limit, which becomes
 * t - ttl_dec; src and dst, the address part of the new tuple; TCP bytes 0-3,
 * the port part of the new tuple; IPv4 header bytes 10-11 (the header
 * checksum); TCP bytes 16-17 (the TCP checksum).
 *
 * Checksum update (RFC 1624 eqn. 3), evaluated exactly so. Let fold(x) = 0 if
 * x = 0, else 1 + (x - 1) mod 0xFFFF. For a checksum field HC (read big-endian)
 * and the big-endian 16-bit words m_k -> m'_k it covers, every listed word
 * included whether or not its value changed:
 *   HC' = ~fold((~HC & 0xFFFF) + SUM_k ((~m_k & 0xFFFF) + m'_k)) & 0xFFFF.
 * The IPv4 header checksum covers the word at bytes 8-9 (TTL, protocol) and
 * the 4 address words; the IPv4 TCP checksum the 4 address words (its
 * pseudo-header) and the 2 port words; the IPv6 TCP checksum the 16 address
 * words and the 2 port words. The hop limit is covered by no checksum.
 * Consequence: for a frame whose checksum verified before, the new field equals
 * what a full recomputation over the rewritten frame stores (~sum with the
 * field zero, as the transmit pass writes it), bit for bit; for a frame whose
 * checksum was wrong, it stays wrong by the same one's-complement difference.
 *
 * NSX_EINVAL before anything else: a NULL pointer (d_base, d_valid and d_hit may
 * be NULL when n == 0), n >= 2^32 - 1, slots not a power of two or > 2^31, a
 * misaligned table, ttl_dec > 255. Then NSX_ENODEV without a GPU. No
 * allocation, no host sync, no per-stream counters: one launch (none for
 * n == 0), which can be captured into a graph. There are no _host forms (header
 * edits over PCIe make no sense), no _tuned twins (one lane per frame: there is
 * no launch shape to override) and no multi-GPU sharding. */
int nsx_nat_table_slots(uint64_t n_rules, uint64_t* out_slots);
int nsx_nat_table_build_host(uint32_t ip_ver, const uint8_t* h_match, const uint8_t* h_new, uint64_t n_rules,
                             void* h_table, uint64_t slots);
int nsx_nat_ipv4_tcp_rewrite_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit,
                                 nsx_stream_t stream);
int nsx_nat_ipv6_tcp_rewrite_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 const void* d_table, uint64_t slots, uint32_t ttl_dec, uint64_t* d_hit,
                                 nsx_stream_t stream);

/* IPv4 fragmentation and reassembly (RFC 791 §2.3, §3.2) on device-resident
 * frames: nsx_frag_ipv4_dev cuts the frames that do not fit their link's MTU
 * into fragments; nsx_reasm_ipv4_dev puts the fragments of a receive batch back
 * into whole datagrams, which then go into nsx_rx_ipv4_tcp_verify_dev or
 * nsx_udp_rx_ipv4_verify_dev (neither of which accepts a fragment). Kernels of
 * their own (csrc/frag_kernels.hip); no other call changes. IPv4 only: IPv6
 * fragments in an extension header (RFC 8200 §4.5), and no pass here walks
 * extension headers.
 *
 * Fragmentation. Input as the receive passes take it: n densely packed frames,
 * frame i = d_base[d_offsets[i], d_offsets[i+1]) of len_i bytes at any
 * alignment, and d_mtu[i] >= 28, the MTU of the link frame i goes out on. With
 * per_i = (mtu_i - 20) & ~7, frame i takes cnt_i output slots: 1 if
 * len_i <= mtu_i, else ceil((len_i - 20) / per_i). The frame map, built as for
 * segmentation offload: frag_first (n + 1 entries) is the prefix sum of cnt_i;
 * frag_src (n_frags entries) the source frame of each slot; out_off
 * (n_frags + 1 entries) is dense, out_off[0] = 0, no padding: the slot of a
 * frame that fits is len_i bytes, slot j of a frame that does not is
 * 20 + min(per_i, len_i - 20 - j*per_i) bytes. nsx_frag_count_host writes
 * frag_first, nsx_frag_layout_host frag_src and out_off; host memory, no GPU.
 * NSX_EINVAL, with nothing written: a NULL array (h_mtu, and h_frag_src when
 * there is no slot, may be NULL for n == 0), decreasing offsets, an mtu below
 * 28, a frame of 2^30 bytes or more, n >= 2^32, an h_frag_first that is not
 * nsx_frag_count_host's.
 *
 * The device rule for frame i; d_status (n entries) receives its status:
 *   NSX_FRAG_PASS (0)  len_i <= mtu_i: its one slot is the frame byte for byte,
 *                      whatever it holds.
 *   NSX_FRAG_CUT (1)   len_i > mtu_i, and the frame is version 4 with IHL 5,
 *                      its total length equals len_i, DF is clear, and with o
 *                      its own fragment offset field o*8 + len_i - 20 <= 65535.
 *   NSX_FRAG_DF (2)    as CUT but DF is set: the caller owes an ICMP
 *                      "fragmentation needed" (RFC 1191).
 *   NSX_FRAG_BAD (3)   any other frame longer than its mtu; and any frame
 *                      whose mtu, as the device sees it, is below 28.
 * Fragment j of a CUT frame is the frame's 20 header bytes followed by payload
 * bytes [j*per, min((j+1)*per, len - 20)), with: total length its own; fragment
 * offset o + j*per/8; MF set on every fragment but the last, which keeps the
 * frame's own MF (so a fragment can be cut again, as RFC 791 allows: the
 * offsets add); the reserved and DF bits of byte 6, ident, TOS, TTL, protocol
 * and the addresses copied; and the header checksum updated from the frame's
 * own field by RFC 1624 eqn. 3 with the fold defined for nsx_nat_* above, over
 * word 1 (bytes 2-3) and word 3 (bytes 6-7), both included whether or not they
 * changed. A valid header stays valid and equals a full recomputation; a wrong
 * one stays wrong by the same one's-complement difference. For statuses 2 and 3
 * every byte of the frame's slots is written as zero: a zero version nibble
 * fails every downstream pass by itself. Nothing outside the slots is written,
 * and no byte outside a frame's own range is read. A slot whose extent in
 * d_out_off is not what the rule above gives it (a map that is not the host
 * helpers') is not written; nor is a frame or slot of 2^30 bytes or more, which
 * the host helpers refuse: such a frame gets status 3 and its slots stay as
 * they were.
 *
 * nsx_frag_ipv4_dev: NSX_EINVAL for n >= 2^32, n_frags < n, n_frags > 0 with
 * n == 0, or a NULL pointer with n > 0; n_frags == 0 is then NSX_OK without a
 * launch (and without looking for a device); then NSX_ENODEV without a GPU.
 *
 * Reassembly. Input: d_base, d_offsets (n + 1), n as above. There is no validity
 * mask: the transport verifies cannot accept a fragment, so this pass checks
 * the header itself. Frame i of len bytes is a member iff len >= 21; it is
 * version 4 with IHL 5; its total length equals len; the raw sum over its 20
 * header bytes is 0xFFFF; it is a fragment: MF is set or its offset field o is
 * nonzero; and with pay = len - 20: pay >= 1, pay % 8 == 0 when MF is set, and
 * o*8 + pay <= 65515. is_frag (ceil(n/64) words) holds the member bits; bits
 * past n are 0.
 *
 * Key: FNV-1a as nsx_gro_flow_* defines it, over three little-endian dwords:
 * header bytes 12-15, header bytes 16-19, and b4 | b5<<8 | b9<<16 (ident and
 * protocol); a non-member gets 0xFFFFFFFF. Order: let o1 be the stable
 * ascending argsort of the fragment offset field (0 for a non-member); then
 * d_order = o1[stable argsort of key[o1]] — two runs of the radix sort of
 * nsx_gro_flow_*; bit for bit numpy.lexsort((arrival, off, key)). d_order has n
 * entries and is an output.
 *
 * Over the positions p of that order, cont(p) holds iff the frames at p-1 and p
 * are both members; src, dst, ident and protocol are equal, compared in full (a
 * key collision costs a datagram and never merges wrongly); MF is set on the
 * frame at p-1; and o_p*8 == o_{p-1}*8 + pay_{p-1}: exact abutment — an
 * overlap, a gap or a duplicate breaks the run. A run is a maximal chain of
 * cont. It is complete iff its first frame has offset 0 and its last has MF
 * clear; its datagram is then 20 + o_last*8 + pay_last bytes long. Complete
 * runs are numbered in position order; *n_out (a uint64_t in device memory) is
 * their count.
 *
 * Datagram s is written to out[out_off[s], out_off[s+1]): dense, out_off[0] = 0,
 * n_out + 1 entries. It is the first fragment's header with the total length
 * set to the datagram's, MF and the offset cleared (byte 6 & 0xC0 kept, byte 7
 * zero) and the header checksum recomputed (~sum with the field zero), then each
 * fragment's payload at out_off[s] + 20 + o*8. first_pos[s] is the position in
 * d_order of the run's first fragment, frag_cnt[s] the run's length;
 * frame_seg[i] (n entries, indexed by frame) is the datagram that consumed
 * frame i, or 0xFFFFFFFF. A member with no datagram is a leftover: the caller
 * carries it into its next batch. There are no timers and no cross-batch state.
 * Entries, offsets and bytes past the last one written are left exactly as they
 * were. Worst-case extents: n entries per array, n + 1 offsets,
 * d_offsets[n] - d_offsets[0] output bytes.
 *
 * RFC 4963: two datagrams with the same (src, dst, ident, protocol) in one
 * batch are one key here, and their fragments can be mixed into one datagram
 * whose pieces abut; the transport checksum then refuses it, exactly as on any
 * RFC 791 host.
 *
 * The defining property: for frames with IHL 5, a valid header checksum and DF
 * clear, nsx_frag_ipv4_dev followed by nsx_reasm_ipv4_dev rebuilds every cut
 * frame byte for byte, in any order of the fragments; the output with its
 * out_off goes straight into the receive verifies.
 *
 * nsx_reasm_ipv4_dev: NSX_EINVAL before any launch for a NULL pointer or struct
 * member (d_base and d_order may be NULL when n == 0), n >= 2^32 - 1, or
 * work_bytes below nsx_reasm_work_bytes(n); then NSX_ENODEV without a GPU.
 * n == 0 writes *n_out = 0 and out_off[0] = 0 on the stream and no order.
 * Both calls: no allocation, no host sync, no per-stream counters; each is one
 * serial chain of launches and can be captured into a graph; 64-bit offsets
 * throughout: frames may lie past 2^32 in d_base. There are no _host forms. The
 * _tuned twins are in nsx_frag_tune.h. */
#define NSX_FRAG_PASS 0
#define NSX_FRAG_CUT  1
#define NSX_FRAG_DF   2
#define NSX_FRAG_BAD  3
typedef struct {
    uint64_t* n_out;
    uint8_t*  out;
    uint64_t* out_off;
    uint64_t* first_pos;
    uint32_t* frag_cnt;
    uint32_t* frame_seg;    /* per frame */
    uint64_t* is_frag;      /* ceil(n/64) words */
} nsx_reasm_out;

int nsx_frag_count_host(const uint64_t* h_offsets, const uint32_t* h_mtu, uint64_t n, uint64_t* h_frag_first);
int nsx_frag_layout_host(const uint64_t* h_offsets, const uint32_t* h_mtu, const uint64_t* h_frag_first, uint64_t n,
                         uint32_t* h_frag_src, uint64_t* h_out_off);
int nsx_frag_ipv4_dev(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_mtu, uint64_t n,
                      const uint64_t* d_frag_first, const uint32_t* d_frag_src, uint64_t n_frags, uint8_t* d_out,
                      const uint64_t* d_out_off, uint8_t* d_status, nsx_stream_t stream);
int nsx_reasm_work_bytes(uint64_t n, uint64_t* out);
int nsx_reasm_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint32_t* d_order,
                       const nsx_reasm_out* out, void* d_work, uint64_t work_bytes, nsx_stream_t stream);

/* ICMP and ICMPv6 (RFC 792, RFC 4443) on device-resident frames: error
 * generation for the frames the other passes hand back (NSX_FRAG_DF: RFC 1191
 * "fragmentation needed"; the frames the NAT rewrite refuses on TTL: "time
 * exceeded"), a receive verify that tells a ping from garbage, and the echo
 * reply written over the request in place. Kernels of their own
 * (csrc/icmp_kernels.hip); no other call changes. Input everywhere as the
 * receive passes take it: n densely packed frames, frame i = d_base[d_offsets[i],
 * d_offsets[i+1]) of len_i bytes at any alignment, d_offsets with n + 1 entries.
 *
 * Error generation (nsx_icmp_err_ipv4_dev / nsx_icmp_err_ipv6_dev). d_req holds
 * one request word per frame: 0 is no request, else bits 0-7 are the ICMP type,
 * bits 8-15 the code and bits 16-31 must be 0. Allowed types: 3 (destination
 * unreachable), 11 (time exceeded) and 12 (parameter problem) on IPv4; 1
 * (destination unreachable), 2 (packet too big), 3 (time exceeded) and 4
 * (parameter problem) on IPv6; any code. d_arg[i] (d_arg NULL: all zero) is
 * written big-endian into ICMP header bytes 4-7: the next-hop MTU in its low
 * half on IPv4 (RFC 1191), the 32-bit MTU on IPv6, the pointer (ptr << 24 on
 * IPv4, RFC 792; the 32-bit pointer on IPv6). cfg is host memory read at call
 * time: src our own address (IPv4: its first 4 bytes), ttl the TTL / hop limit
 * of every message (ttl > 255 is NSX_EINVAL), ident0 the first IPv4 ident,
 * max_out the most messages one call makes.
 *
 * status (n entries) receives, by the first rule that matches:
 *   NSX_ICMP_NONE (0)     the request is 0. The frame is not read.
 *   NSX_ICMP_BAD (3)      the request is not an allowed one (the frame is then
 *                         not read either), or the frame is malformed. IPv4:
 *                         fewer than 20 bytes, version != 4, IHL < 5, IHL*4 >
 *                         len, or total length != len. IPv6: fewer than 40
 *                         bytes, version != 6, or 40 + payload length != len.
 *   NSX_ICMP_QUIET (2)    the RFCs say to stay silent. IPv4 (RFC 1122 §3.2.2,
 *                         RFC 1812 §4.3.2.7): the fragment offset field is
 *                         nonzero (MF alone does not count: the first fragment
 *                         is answered); src is 0.0.0.0 or src[0] >= 224;
 *                         dst[0] >= 224; the protocol is 1 and the ICMP type
 *                         byte at frame byte IHL*4 is absent or is not one of
 *                         the query types 0, 8, 9, 10, 13, 14, 15, 16, 17, 18.
 *                         IPv6 (RFC 4443 §2.4(e)): src is :: or src[0] == 0xFF;
 *                         dst[0] == 0xFF, unless the request is type 2, or type
 *                         4 with code 2; Next Header is 58 and the type byte at
 *                         frame byte 40 is absent, is below 128 (an error), or
 *                         is 137 (a redirect). Extension headers are not
 *                         walked: an ICMPv6 error behind one is answered.
 *   NSX_ICMP_LIMITED (4)  the frame's rank among the frames not refused above,
 *                         in frame order, is >= max_out: the per-call rate cap
 *                         of RFC 1812 §4.3.2.8 and RFC 4443 §2.4(f).
 *   NSX_ICMP_SENT (1)     everything else.
 * The SENT frames are numbered in frame order, s = 0 .. n_out - 1; *n_out is a
 * uint64_t in device memory; src_frame[s] is the frame's index; out_off is
 * dense, n_out + 1 entries, out_off[0] = 0. Message s is hdr + 8 + q bytes at
 * out[out_off[s], out_off[s+1]), q = min(len, Q): Q = 548 on IPv4 (RFC 1812
 * §4.3.2.3: 576 bytes in all), 1232 on IPv6 (RFC 4443 §2.4(c): 1280 in all).
 *   IPv4: 45 C0, the total length 28 + q, ident = (ident0 + s) mod 2^16, 00 00,
 *         cfg.ttl, 01, the header checksum (~sum with the field zero); src =
 *         cfg.src, dst = the offending frame's src; type, code, the ICMP
 *         checksum — ~raw over the 8 + q ICMP bytes with the field zero, an odd
 *         tail padded with a zero byte (ICMP has no 0 -> 0xFFFF rule) — d_arg
 *         big-endian; then the frame's first q bytes.
 *   IPv6: 60 00 00 00, the payload length 8 + q, 3A, cfg.ttl; cfg.src, the
 *         offending frame's src; type, code, the checksum — ~raw over the
 *         RFC 8200 §8.1 pseudo-header (src, dst, the 32-bit upper-layer length
 *         8 + q, next header 58) ‖ the message — d_arg big-endian; the quote.
 * Entries, offsets and bytes past the last one written stay as they were; n == 0
 * writes *n_out = 0 and out_off[0] = 0 on the stream. Worst-case extents:
 * min(n, max_out) entries of src_frame, one more of out_off, and SUM_i (hdr + 8
 * + min(len_i, Q)) output bytes (at most min(n, max_out) * (hdr + 8 + Q)); the
 * cap bounds them. d_work is scratch of nsx_icmp_err_work_bytes(n) bytes
 * (nondecreasing in n), work_bytes what the caller really has.
 *
 * Request helpers, so that frag -> errors and NAT -> errors stay on the device.
 * Each is one launch, writes d_req[i] and d_arg[i] only where its condition
 * holds and leaves every other entry as it was: the caller zeroes the arrays
 * first, and the helpers compose on the same arrays.
 *   nsx_icmp_req_frag_dev       d_status[i] == NSX_FRAG_DF (nsx_frag_ipv4_dev's
 *                               status): req = 3 | 4<<8, arg = d_mtu[i] & 0xFFFF.
 *   nsx_icmp_req_ttl_ipv4_dev,  frame i's d_valid bit is set, the frame holds a
 *   nsx_icmp_req_ttl_ipv6_dev   whole IP header of its version (IPv4: 20 bytes
 *                               or more, version 4, 5 <= IHL, IHL*4 <= len;
 *                               IPv6: 40 bytes or more, version 6 — re-checked,
 *                               so a wrong mask reads nothing outside the frame
 *                               and a clear bit reads nothing at all) and its
 *                               TTL / hop limit t satisfies t <= ttl_dec: req =
 *                               11 (IPv6: 3), code 0, arg = 0. With the receive
 *                               pass's mask this is exactly the set the NAT
 *                               rewrite refuses on TTL. ttl_dec > 255 is
 *                               NSX_EINVAL.
 *
 * Receive verify (nsx_icmp_rx_ipv4_verify_dev / nsx_icmp_rx_ipv6_verify_dev),
 * in the shape of nsx_udp_rx_*_verify_dev. Frame i is well-formed iff
 *   IPv4: version 4, IHL >= 5, IHL*4 + 8 <= len, total length == len, MF clear
 *         and fragment offset 0, protocol 1;
 *   IPv6: len >= 48, version 6, 40 + payload length == len, Next Header 58
 *         (extension headers are not walked).
 * Bit (i % 64) of d_mask[i / 64] is set iff frame i is well-formed and verifies:
 * IPv4, the raw sum over the IHL*4 header bytes is 0xFFFF and the raw sum over
 * bytes [IHL*4, len) is 0xFFFF (ICMP has no pseudo-header); IPv6, the raw sum
 * over the RFC 8200 §8.1 pseudo-header (the frame's own addresses, len - 40,
 * 58) ‖ bytes [40, len) is 0xFFFF. There is no zero-checksum exception on
 * either. d_ip_raw (IPv4, nullable) is the header's raw sum, 0 when the frame
 * holds fewer than 20 bytes, IHL < 5 or IHL*4 exceeds the frame; d_icmp_raw
 * (nullable) is that raw, 0 unless the frame is well-formed; d_type (nullable, n
 * uint16_t) is type << 8 | code, and 0xFFFF unless the bit is set: the demux a
 * caller needs to pick the echo requests. Bits past n in the last word are 0;
 * d_mask holds ceil(n/64) words. The split over the waves is static.
 *
 * Echo reply in place (nsx_icmp_echo_reply_ipv4_dev / _ipv6_dev). Frame i is
 * answered iff its d_valid bit is set (d_valid: the verify's mask, required);
 * it is well-formed as the verify defines (re-checked here, as the NAT rewrite
 * does, so a wrong mask never makes the kernel touch a byte outside the frame's
 * own range, nor a frame whose bit is clear at all; the sums are not looked
 * at); it is type 8 code 0 (IPv6: type 128 code 0); and dst[0] < 224 (IPv6:
 * dst[0] != 0xFF), because the old dst becomes the new src. An answered frame
 * changes only in: src and dst, which are swapped; TTL / hop limit, which
 * becomes ttl (ttl > 255 is NSX_EINVAL); the type, which becomes 0 (IPv6: 129);
 * the IPv4 header checksum, updated by RFC 1624 eqn. 3 with the fold defined for
 * nsx_nat_* above over the word at bytes 8-9; and the ICMP checksum, updated
 * the same way over ICMP word 0. The address swap leaves both the header sum
 * and the IPv6 pseudo-header sum unchanged, and the hop limit is covered by no
 * checksum. IP options and the payload are neither read nor written. A frame
 * that is not answered is left byte for byte as it was. Bit (i % 64) of
 * d_hit[i / 64] is set iff frame i was answered; bits past n are 0; d_hit has
 * ceil(n/64) words and is required. Consequence: a verified request becomes a
 * reply that verifies and equals a full recomputation (~sum with the field
 * zero), bit for bit; a wrong one stays wrong by the same one's-complement
 * difference.
 *
 * All calls: NSX_EINVAL before anything else — a NULL pointer (every array may
 * be NULL when n == 0, except cfg, the out struct, its n_out and out_off, and
 * d_work of the error calls; d_arg of the error calls and the nullable outputs
 * of the verify may always be NULL), n >= 2^32 - 1, ttl or ttl_dec > 255,
 * work_bytes below nsx_icmp_err_work_bytes(n) — then NSX_ENODEV without a GPU;
 * n == 0 is then NSX_OK without a launch (the error calls: with the one that
 * writes *n_out and out_off[0]). No allocation, no host sync, no per-stream
 * counters: each call is one serial chain of launches and can be captured into
 * a graph; 64-bit offsets throughout: frames may lie past 2^32 in d_base. No
 * byte outside a frame's own range is read, and no byte outside a slot or frame
 * that the rules name is written. There are no _host forms and no multi-GPU
 * sharding. The _tuned twins of the error and verify calls are in
 * nsx_icmp_tune.h. */
#define NSX_ICMP_NONE    0
#define NSX_ICMP_SENT    1
#define NSX_ICMP_QUIET   2
#define NSX_ICMP_BAD     3
#define NSX_ICMP_LIMITED 4
typedef struct {
    uint8_t  src[16];       /* our own address; IPv4: the first 4 bytes */
    uint32_t ttl;           /* TTL / hop limit of every message, <= 255 */
    uint32_t ident0;        /* IPv4: message s carries (ident0 + s) mod 2^16 */
    uint64_t max_out;       /* the most messages one call makes */
} nsx_icmp_err_cfg;         /* host memory, read at call time */
typedef struct {
    uint64_t* n_out;
    uint8_t*  out;
    uint64_t* out_off;
    uint32_t* src_frame;
    uint8_t*  status;       /* per frame */
} nsx_icmp_err_out;         /* device arrays */

int nsx_icmp_err_work_bytes(uint64_t n, uint64_t* out);
int nsx_icmp_err_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,
                          const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* out,
                          void* d_work, uint64_t work_bytes, nsx_stream_t stream);
int nsx_icmp_err_ipv6_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint32_t* d_req,
                          const uint32_t* d_arg, const nsx_icmp_err_cfg* cfg, const nsx_icmp_err_out* out,
                          void* d_work, uint64_t work_bytes, nsx_stream_t stream);
int nsx_icmp_req_frag_dev(const uint8_t* d_status, const uint32_t* d_mtu, uint64_t n, uint32_t* d_req, uint32_t* d_arg,
                          nsx_stream_t stream);
int nsx_icmp_req_ttl_ipv4_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                              uint32_t ttl_dec, uint32_t* d_req, uint32_t* d_arg, nsx_stream_t stream);
int nsx_icmp_req_ttl_ipv6_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                              uint32_t ttl_dec, uint32_t* d_req, uint32_t* d_arg, nsx_stream_t stream);
int nsx_icmp_rx_ipv4_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                uint16_t* d_ip_raw, uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream);
int nsx_icmp_rx_ipv6_verify_dev(const void* d_base, const uint64_t* d_offsets, uint64_t n, uint64_t* d_mask,
                                uint16_t* d_icmp_raw, uint16_t* d_type, nsx_stream_t stream);
int nsx_icmp_echo_reply_ipv4_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 uint32_t ttl, uint64_t* d_hit, nsx_stream_t stream);
int nsx_icmp_echo_reply_ipv6_dev(void* d_base, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_valid,
                                 uint32_t ttl, uint64_t* d_hit, nsx_stream_t stream);

/* ----------------------------------------------------------------------------
 * Host-resident batches: pinned staging, H2D → kernel → D2H double-buffered
 * over two streams per GPU, segments sharded contiguously across num_gpus
 * devices (0 = auto: one GPU per 64 MiB of batch, up to all visible). No
 * collective: shards are independent.
 * h_prefix_partial nullable.
 */
int nsx_csum_fixed_host(const uint8_t* h_base, uint64_t stride, uint32_t seg_len, uint64_t n,
                        const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus);

int nsx_csum_ragged_host(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n,
                         const uint32_t* h_prefix_partial, uint16_t* h_out, int num_gpus);

/* The fused receive pass (nsx_rx_ipv4_tcp_verify_dev) over host-resident
 * datagrams: h_mask receives ceil(n/64) words. Shards and chunks start on
 * 64-frame mask words. */
int nsx_rx_ipv4_tcp_verify_host(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n, uint64_t* h_mask,
                                int num_gpus);
int nsx_rx_ipv6_tcp_verify_host(const uint8_t* h_base, const uint64_t* h_offsets, uint64_t n, uint64_t* h_mask,
                                int num_gpus);

/* The fused sender pass (nsx_tcp_build_dev) over host-resident segments: the
 * header fields (nsx_tcp_hdr_soa members here are HOST arrays of n entries;
 * `offset` nullable as for the device call), options (h_opt_off nullable),
 * payloads, partials (nullable) and the output are in host memory, pageable or
 * pinned (nsx_alloc_pinned; pinned data and output are DMA'd directly). Writes
 * each wire image to h_out + h_out_off[i] with the device call's layout rule
 * (h_out_off[i] a multiple of 4, room for the image rounded up to 4 bytes, the
 * up to 3 bytes after it zero-filled; nsx_tcp_layout_host makes such offsets;
 * bytes between a padded image and the next offset are left as they are) and
 * the raw sums to h_raw (nullable). Offsets must be non-decreasing and every
 * image shorter than 2^31 bytes (NSX_EINVAL otherwise, checked before any copy).
 * Sharded by image bytes over num_gpus devices like the calls above (0 = auto),
 * chunks of <= 64 MiB of images double-buffered per device.
 * Replaces a Go send loop over bytes() + computeChecksum + the field store
 * (transport/tcp/tcp.go:98-128, :110, :68-71) whose images then go into the
 * transport's pipe or socket buffers (transport/pipe/pipe.go:92-124). */
int nsx_tcp_build_host(const nsx_tcp_hdr_soa* h_hdr, const uint8_t* h_opts, const uint64_t* h_opt_off,
                       const uint8_t* h_data, const uint64_t* h_data_off, const uint32_t* h_prefix_partial,
                       uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_raw, int num_gpus);

/* The fused transmit pass (nsx_tx_ipv4_tcp_build_dev / nsx_tx_ipv6_tcp_build_dev)
 * over host-resident inputs: nsx_tcp_build_host with the nsx_ip_hdr_soa arrays
 * (HOST arrays here) staged alongside the TCP fields, same chunks, shards and
 * layout rule, whole datagrams written to h_out + h_out_off[i] and the TCP raw
 * sums to h_tcp_raw (nullable). A batch holding a frame that does not fit its
 * IP length field (IPv4 wire > 65515, IPv6 wire > 65535) is NSX_EINVAL, checked
 * with the offsets before any copy. */
int nsx_tx_ipv4_tcp_build_host(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                               const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                               uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_tcp_raw,
                               int num_gpus);
int nsx_tx_ipv6_tcp_build_host(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                               const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                               uint64_t n, uint8_t* h_out, const uint64_t* h_out_off, uint16_t* h_tcp_raw,
                               int num_gpus);

/* Segmentation offload (nsx_tso_ipv4_tcp_build_dev / nsx_tso_ipv6_tcp_build_dev)
 * over host-resident inputs: the nsx_tx_*_build_host job with every array but
 * h_out_off, h_frame_seg and h_tcp_raw (nullable, n_frames entries) holding one
 * entry per super-segment. Checked before any copy (NSX_EINVAL): the offsets and
 * h_mss as nsx_tso_count_host checks them, h_frame_first and h_frame_seg against
 * what nsx_tso_count_host / nsx_tso_layout_host give, the frame slots against
 * the layout rule, and every frame against its IP length field. Sharded by
 * image bytes, chunks of <= 64 MiB double-buffered; a shard and a chunk end on
 * a super-segment boundary, and a super-segment larger than the budget is a
 * chunk of its own. A super-segment's fields, options and payload go to the
 * device once, not once per frame; the frame map and the offsets are rebased
 * per chunk. Pageable or pinned memory. */
int nsx_tso_ipv4_tcp_build_host(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                const uint32_t* h_mss, uint64_t n, const uint64_t* h_frame_first,
                                const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,
                                const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus);
int nsx_tso_ipv6_tcp_build_host(const nsx_ip_hdr_soa* h_ip, const nsx_tcp_hdr_soa* h_tcp, const uint8_t* h_opts,
                                const uint64_t* h_opt_off, const uint8_t* h_data, const uint64_t* h_data_off,
                                const uint32_t* h_mss, uint64_t n, const uint64_t* h_frame_first,
                                const uint32_t* h_frame_seg, uint64_t n_frames, uint8_t* h_out,
                                const uint64_t* h_out_off, uint16_t* h_tcp_raw, int num_gpus);

/* The host batch calls keep per-device streams and grow-only device/pinned
 * staging buffers across calls (a transport calls them once per batch). This
 * frees the cached buffers; the next call re-allocates. Safe to call at any
 * time; concurrent host batch calls on a device wait for each other. */
int nsx_host_cache_release(void);

/* Return the per-stream work-deal counters the device calls above gave
 * `stream` (nsx_rx_ipv4_tcp_verify_dev and friends) before the caller destroys
 * it: call after the stream has drained (hipStreamSynchronize) and before
 * hipStreamDestroy. The counters go to the next new stream; without this, a
 * process that creates and destroys streams in a loop keeps the first 64 on the
 * dealt path and splits every later one statically (correct, ~2% slower). */
int nsx_stream_release(nsx_stream_t stream);

/* Pinned (DMA-registered) host memory for zero-copy staging from Go via
 * unsafe.Slice (cgo forbids C retaining Go pointers; runtime.Pinner does not
 * DMA-register). */
int nsx_alloc_pinned(size_t bytes, void** out);
int nsx_free_pinned(void* p);

/* ----------------------------------------------------------------------------
 * Sharding plan (host logic, no GPU): split n segments over `parts` shards.
 * Fixed stride (h_offsets NULL): contiguous index ranges of near-equal count.
 * Ragged: contiguous index ranges of near-equal BYTE count using the prefix-sum
 * offsets. Writes parts+1 boundaries to out_bounds (out_bounds[0]=0,
 * out_bounds[parts]=n).
 */
int nsx_shard_plan(const uint64_t* h_offsets, uint64_t n, int parts, uint64_t* out_bounds);

/* ----------------------------------------------------------------------------
 * Synthetic batches (bench/test data): byte j of the stream is
 * byte j%8 of the little-endian word splitmix64(seed, j/8); writes stream bytes
 * [byte_off, byte_off + nbytes) to d_buf. Counter-based, so any range can be
 * regenerated on the host. */
int nsx_fill_splitmix64_dev(void* d_buf, uint64_t byte_off, uint64_t nbytes, uint64_t seed,
                            nsx_stream_t stream);

/* ----------------------------------------------------------------------------
 * Introspection. (Benchmark/test launch overrides are per call, in
 * include/nsx_tune.h — not part of this boundary.)
 */
int nsx_abi_version(void);
int nsx_device_count(int* out_count);        /* NSX_OK with 0 when no GPU */
const char* nsx_strerror(int code);

/* Receiver/sender helpers (tcp.go:68-71, tcp_test.go:28-31). */
static inline uint16_t nsx_field(uint16_t raw_sum) { return (uint16_t)~raw_sum; }
static inline int nsx_verify(uint16_t raw_sum) { return raw_sum == 0xFFFF; }

#ifdef __cplusplus
}
#endif
#endif /* NSX_CSUM_H */
