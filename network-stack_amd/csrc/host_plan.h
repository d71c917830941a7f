// host_plan.h — everything a host batch call decides before its first copy: argument and layout validation,
// shard bounds, chunk cuts and the sender job's staging layout. No HIP: host_plan.cpp builds with a plain C++
// compiler and is tested on its own (tests/cpp/test_host_plan.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/nsx_csum.h"

namespace nsx {

constexpr uint64_t kChunkBytes = 64ull << 20;  // default chunk budget (nsx_tune.chunk_bytes 0), and the auto shard size

// ---- chunks: segments [c0, c1) of a shard, and the host byte span [byte_lo, byte_hi) copied for them ----
struct Chunk {
    uint64_t c0, c1;
    uint64_t byte_lo, byte_hi;
};
enum class Cut {
    kFixed,   // by count: max(1, budget / max(stride, seg_len, 1)) segments per chunk
    kRagged,  // by bytes over offsets; a segment larger than the budget is a chunk of its own
    kRx,      // by bytes on whole 64-frame mask words: max(64, floor64) frames unless the chunk is the shard's last
};
std::vector<Chunk> plan_chunks(Cut cut, const uint64_t* offsets, uint64_t stride, uint32_t seg_len, uint64_t lo,
                               uint64_t hi, uint64_t budget);
// The sender job: the budget bounds image bytes (seg_out) and payload bytes (data_off) at once; image spans.
std::vector<Chunk> plan_sender_chunks(const uint64_t* seg_out, const uint64_t* data_off, uint64_t lo, uint64_t hi,
                                      uint64_t budget);

// ---- shards ----
// GPUs an auto call (num_gpus <= 0) uses: all of them, but no shard smaller than one default chunk.
int auto_gpus(uint64_t bytes, int device_count);
// parts + 1 shard bounds (shard_plan of host_csum.h); align64 starts every shard on a 64-frame mask word.
std::vector<uint64_t> shard_bounds(const uint64_t* offsets, uint64_t n, int parts, bool align64);

// ---- the sender job's staging layout ----
constexpr int kTcpFields = 8, kIpFields = 6, kAllFields = kTcpFields + kIpFields + 1;
// The field arrays in the order of nsx_tcp_hdr_soa's members, then nsx_ip_hdr_soa's, then the mss: host source
// (null where the caller passed none) and entry size. n = 8 (TCP images), 14 (datagrams) or 15 (segmentation).
struct FieldSet {
    int n;
    const void* src[kAllFields];
    uint64_t esz[kAllFields];
};
FieldSet sender_fields(const nsx_tcp_hdr_soa* tcp, const nsx_ip_hdr_soa* ip, int ipver, const uint32_t* mss);
// The field block of a chunk of cn segments: sub-array f starts at at[f], each 256 B-aligned. Returns its bytes.
uint64_t field_block(const FieldSet& fs, uint64_t cn, uint64_t at[kAllFields]);
// The same arrays inside a staged block at `base`, as the ABI's structs (null where the source was null).
void field_block_soa(const FieldSet& fs, const uint64_t at[kAllFields], uint8_t* base, nsx_tcp_hdr_soa* tcp,
                     nsx_ip_hdr_soa* ip, const uint32_t** mss);
// The rebased offsets of cn segments and fn frames as 8-byte words of one block: data_off (cn + 1) at 0, out_off
// (fn + 1) at at_out, opt_off (cn + 1, when given) at at_opt; with segmentation frame_first (cn + 1) at at_first
// and frame_seg (fn 4-byte entries) at at_seg.
struct OffBlock {
    uint64_t at_out, at_opt, at_first, at_seg, words;
};
OffBlock off_block(uint64_t cn, uint64_t fn, bool opts, bool tso);
// The staged payload keeps its byte offset mod 256 and sits >= 256 B into its buffer; the image span keeps its offset
// mod 256: every segment takes the kernel path it would take in a device-resident batch at a 256-aligned base.
inline uint64_t lead_data(uint64_t d0) { return 256 + (d0 & 255); }
inline uint64_t lead_out(uint64_t byte_lo) { return byte_lo & 255; }

// ---- validators ----
bool tcp_hdr_ok(const nsx_tcp_hdr_soa* h);  // every member but the optional `offset`
bool ip_hdr_ok(const nsx_ip_hdr_soa* ip);   // src and dst
inline uint64_t tso_frames(uint64_t len, uint32_t mss) { return len ? (len + mss - 1) / mss : 1; }
constexpr uint64_t kTsoBad = ~0ull;
// One walk of the segmentation frame map: every mss non-zero, data (and option) offsets non-decreasing, and, where
// `expect` is given, expect[i] each super-segment's first frame and expect[n] the total. Writes the first frames
// and the total to `first` (n + 1) where given. Returns the total, or kTsoBad.
uint64_t tso_walk(const uint64_t* opt_off, const uint64_t* data_off, const uint32_t* mss, uint64_t n,
                  const uint64_t* expect, uint64_t* first);
// The sender layout, one slot per segment: non-decreasing offsets, 4-aligned image slots that hold their image and
// its zero padding, images shorter than 2^31 bytes, and with an IP header (ip_hdr_len 20 / 40, else 0) a TCP part
// that fits the IP length field. *gaps: some slot is longer than its padded image.
bool sender_layout_ok(uint32_t ip_hdr_len, const uint64_t* opt_off, const uint64_t* data_off,
                      const uint64_t* out_off, uint64_t n, bool* gaps);
// The same per frame of a walked frame map of n_frames, plus frame_seg; seg_out (n + 1) receives each
// super-segment's first image offset.
bool tso_layout_ok(uint32_t ip_hdr_len, const uint64_t* opt_off, const uint64_t* data_off, const uint32_t* mss,
                   uint64_t n, const uint32_t* frame_seg, const uint64_t* out_off, uint64_t n_frames,
                   uint64_t* seg_out, bool* gaps);

// ---- the UDP passes' layouts (include/nsx_csum.h nsx_udp_layout_host / nsx_udp_uso_layout_host) ----
// The 4-padded slot of a UDP frame: IP header, the 8-byte UDP header, the payload.
inline uint64_t udp_slot(uint32_t ip_hdr_len, uint64_t payload) { return (ip_hdr_len + 8u + payload + 3u) & ~3ull; }
// Packed slots of n frames into out_off (n + 1); false, with nothing written, for decreasing offsets.
bool udp_layout(uint32_t ip_hdr_len, const uint64_t* data_off, uint64_t n, uint64_t* out_off);
// frame_seg and the packed slots of a walked frame map (tso_walk: the map is segmentation offload's own) over its
// cuts of gso payload bytes; returns the frame count.
uint64_t udp_uso_layout(uint32_t ip_hdr_len, const uint64_t* data_off, const uint32_t* gso, uint64_t n,
                        uint32_t* frame_seg, uint64_t* out_off);

// ---- the NAT rewrite's translation table (include/nsx_csum.h nsx_nat_*) ----
// Tuple and entry bytes per IP version: 12 / 32 (IPv4), 36 / 80 (IPv6). An entry: match tuple, state dword
// (little-endian, 1 = occupied), new tuple, zero dword.
constexpr uint64_t kNatMaxSlots = 1ull << 31;
inline uint32_t nat_tuple_bytes(uint32_t ip_ver) { return ip_ver == 6 ? 36u : 12u; }
inline uint32_t nat_entry_bytes(uint32_t ip_ver) { return 2u * nat_tuple_bytes(ip_ver) + 8u; }
inline bool nat_slots_ok(uint64_t slots) { return slots && !(slots & (slots - 1)) && slots <= kNatMaxSlots; }
// FNV-1a over the tuple's little-endian dwords: nsx_gro_flow_*'s flow key.
uint32_t nat_hash(const uint8_t* tuple, uint32_t tuple_bytes);
// Zero-fills the table and inserts the rules in order by linear probing from the home slot. False (arguments the
// header refuses, or two rules with one match tuple) is NSX_EINVAL.
bool nat_table_build(uint32_t ip_ver, const uint8_t* match, const uint8_t* repl, uint64_t n_rules, uint8_t* table,
                     uint64_t slots);

}  // namespace nsx
