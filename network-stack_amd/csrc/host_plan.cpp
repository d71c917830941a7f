// host_plan.cpp — the host batch calls' planning and validation (host_plan.h), and the ABI's host-only layout
// calls over the same walks. No HIP.
#include "host_plan.h"

#include <algorithm>
#include <cstring>

#include "host_csum.h"

namespace nsx {

// The largest c1 in (c0, hi] whose span from c0 fits the budget, at least c0 + 1. Every host call has checked that
// its offsets do not decrease, so fits() is monotone: a binary search per chunk, not a pass over a million offsets.
template <class Fits>
static uint64_t chunk_end(uint64_t c0, uint64_t hi, Fits fits) {
    uint64_t a = c0 + 1, b = hi;
    while (a < b) {
        const uint64_t m = a + (b - a + 1) / 2;
        if (fits(m))
            a = m;
        else
            b = m - 1;
    }
    return a;
}

std::vector<Chunk> plan_chunks(Cut cut, const uint64_t* offsets, uint64_t stride, uint32_t seg_len, uint64_t lo,
                               uint64_t hi, uint64_t budget) {
    std::vector<Chunk> v;
    if (cut == Cut::kFixed) {
        const uint64_t per = std::max<uint64_t>(1, budget / std::max<uint64_t>({stride, seg_len, 1}));
        for (uint64_t c0 = lo; c0 < hi; c0 += per) {
            const uint64_t c1 = std::min(hi, c0 + per);
            v.push_back({c0, c1, c0 * stride, (c1 - 1) * stride + seg_len});
        }
        return v;
    }
    for (uint64_t c0 = lo; c0 < hi;) {
        uint64_t c1 = chunk_end(c0, hi, [=](uint64_t k) { return offsets[k] - offsets[c0] <= budget; });
        if (cut == Cut::kRx && c1 < hi) c1 = std::min(hi, c0 + std::max<uint64_t>(64, (c1 - c0) / 64 * 64));
        v.push_back({c0, c1, offsets[c0], offsets[c1]});
        c0 = c1;
    }
    return v;
}

std::vector<Chunk> plan_sender_chunks(const uint64_t* seg_out, const uint64_t* data_off, uint64_t lo, uint64_t hi,
                                      uint64_t budget) {
    std::vector<Chunk> v;
    for (uint64_t c0 = lo; c0 < hi;) {
        const uint64_t c1 = chunk_end(c0, hi, [=](uint64_t k) {
            return seg_out[k] - seg_out[c0] <= budget && data_off[k] - data_off[c0] <= budget;
        });
        v.push_back({c0, c1, seg_out[c0], seg_out[c1]});
        c0 = c1;
    }
    return v;
}

int auto_gpus(uint64_t bytes, int device_count) {
    const uint64_t want = std::max<uint64_t>(1, (bytes + kChunkBytes - 1) / kChunkBytes);
    return (int)std::min<uint64_t>(want, (uint64_t)device_count);
}

std::vector<uint64_t> shard_bounds(const uint64_t* offsets, uint64_t n, int parts, bool align64) {
    std::vector<uint64_t> b(parts + 1);
    shard_plan(offsets, n, parts, b.data());
    if (align64)
        for (int g = 1; g < parts; ++g) b[g] = std::min<uint64_t>(n, (b[g] + 63) / 64 * 64);
    return b;
}

FieldSet sender_fields(const nsx_tcp_hdr_soa* t, const nsx_ip_hdr_soa* ip, int ipver, const uint32_t* mss) {
    const uint64_t alen = ipver == 4 ? 4 : 16;
    FieldSet fs{kTcpFields,
                {t->src_port, t->dst_port, t->seq_num, t->ack_num, t->offset, t->control, t->window, t->urgent_ptr},
                {2, 2, 4, 4, 1, 1, 2, 2}};
    if (!ip) return fs;
    const void* a[kIpFields] = {ip->src, ip->dst, ip->ident, ip->ttl, ip->tclass, ip->flow};
    const uint64_t as[kIpFields] = {alen, alen, 2, 1, 1, 4};
    for (int f = 0; f < kIpFields; ++f) fs.src[fs.n] = a[f], fs.esz[fs.n++] = as[f];
    if (mss) fs.src[fs.n] = mss, fs.esz[fs.n++] = 4;
    return fs;
}

uint64_t field_block(const FieldSet& fs, uint64_t cn, uint64_t at[kAllFields]) {
    uint64_t end = 0;
    for (int f = 0; f < fs.n; ++f) {
        at[f] = end;
        end += (cn * fs.esz[f] + 255) & ~255ull;
    }
    return end;
}

void field_block_soa(const FieldSet& fs, const uint64_t at[kAllFields], uint8_t* base, nsx_tcp_hdr_soa* tcp,
                     nsx_ip_hdr_soa* ip, const uint32_t** mss) {
    const void* p[kAllFields] = {};
    for (int f = 0; f < fs.n; ++f) p[f] = fs.src[f] ? base + at[f] : nullptr;
    *tcp = {(const uint16_t*)p[0], (const uint16_t*)p[1], (const uint32_t*)p[2], (const uint32_t*)p[3],
            (const uint8_t*)p[4],  (const uint8_t*)p[5],  (const uint16_t*)p[6], (const uint16_t*)p[7]};
    *ip = {(const uint8_t*)p[8],  (const uint8_t*)p[9],  (const uint16_t*)p[10],
           (const uint8_t*)p[11], (const uint8_t*)p[12], (const uint32_t*)p[13]};
    *mss = (const uint32_t*)p[14];
}

OffBlock off_block(uint64_t cn, uint64_t fn, bool opts, bool tso) {
    OffBlock b;
    b.at_out = cn + 1;
    b.at_opt = b.at_out + fn + 1;
    b.at_first = b.at_opt + (opts ? cn + 1 : 0);
    b.at_seg = b.at_first + cn + 1;
    b.words = tso ? b.at_seg + (fn + 1) / 2 : b.at_first;
    return b;
}

bool tcp_hdr_ok(const nsx_tcp_hdr_soa* h) {
    return h && h->src_port && h->dst_port && h->seq_num && h->ack_num && h->control && h->window && h->urgent_ptr;
}

bool ip_hdr_ok(const nsx_ip_hdr_soa* ip) { return ip && ip->src && ip->dst; }

uint64_t tso_walk(const uint64_t* opt_off, const uint64_t* data_off, const uint32_t* mss, uint64_t n,
                  const uint64_t* expect, uint64_t* first) {
    uint64_t f = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (mss[i] == 0 || data_off[i + 1] < data_off[i] || (opt_off && opt_off[i + 1] < opt_off[i]) ||
            (expect && expect[i] != f))
            return kTsoBad;
        if (first) first[i] = f;
        f += tso_frames(data_off[i + 1] - data_off[i], mss[i]);
    }
    if (expect && expect[n] != f) return kTsoBad;
    if (first) first[n] = f;
    return f;
}

namespace {

uint64_t opt_len(const uint64_t* opt_off, uint64_t i) { return opt_off ? opt_off[i + 1] - opt_off[i] : 0; }
uint64_t slot_of(uint32_t iph, uint64_t wire) { return (iph + wire + 3) & ~3ull; }  // the 4-padded image

// One slot [out_off[f], out_off[f + 1]) against the image it must hold.
bool slot_ok(uint32_t iph, uint64_t wire, const uint64_t* out_off, uint64_t f, bool* gaps) {
    const uint64_t wire_max = iph == 20 ? 65515 : iph == 40 ? 65535 : ~0ull, slot = slot_of(iph, wire);
    if (out_off[f + 1] < out_off[f] || (out_off[f] & 3) || wire > wire_max || slot >= (1ull << 31) ||
        out_off[f + 1] - out_off[f] < slot)
        return false;
    *gaps |= out_off[f + 1] - out_off[f] > slot;
    return true;
}

// fn(i, f, wire) for every frame f of every super-segment i of a walked frame map; stops at the first false.
template <class F>
bool each_tso_frame(const uint64_t* opt_off, const uint64_t* data_off, const uint32_t* mss, uint64_t n, F&& fn) {
    uint64_t f = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = data_off[i + 1] - data_off[i], cnt = tso_frames(len, mss[i]);
        for (uint64_t k = 0; k < cnt; ++k, ++f)
            if (!fn(i, f, nsx_tcp_wire_len(opt_len(opt_off, i), std::min<uint64_t>(mss[i], len - k * mss[i]))))
                return false;
    }
    return true;
}

// Packed 4-aligned slots: nsx_tcp_layout_host (ip_hdr_len 0) and nsx_tx_layout_host.
void packed_layout(uint32_t iph, const uint64_t* opt_off, const uint64_t* data_off, uint64_t n, uint64_t* out_off) {
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        out_off[i] = at;
        at += slot_of(iph, nsx_tcp_wire_len(opt_len(opt_off, i), data_off[i + 1] - data_off[i]));
    }
    out_off[n] = at;
}

}  // namespace

bool sender_layout_ok(uint32_t iph, const uint64_t* opt_off, const uint64_t* data_off, const uint64_t* out_off,
                      uint64_t n, bool* gaps) {
    *gaps = false;
    for (uint64_t i = 0; i < n; ++i)
        if (data_off[i + 1] < data_off[i] || (opt_off && opt_off[i + 1] < opt_off[i]) ||
            !slot_ok(iph, nsx_tcp_wire_len(opt_len(opt_off, i), data_off[i + 1] - data_off[i]), out_off, i, gaps))
            return false;
    return true;
}

bool tso_layout_ok(uint32_t iph, const uint64_t* opt_off, const uint64_t* data_off, const uint32_t* mss, uint64_t n,
                   const uint32_t* frame_seg, const uint64_t* out_off, uint64_t n_frames, uint64_t* seg_out,
                   bool* gaps) {
    *gaps = false;
    seg_out[n] = out_off[n_frames];
    uint64_t next = 0;  // the super-segment whose first frame comes next
    return each_tso_frame(opt_off, data_off, mss, n, [&](uint64_t i, uint64_t f, uint64_t wire) {
        if (i == next) seg_out[next++] = out_off[f];
        return frame_seg[f] == i && slot_ok(iph, wire, out_off, f, gaps);
    });
}

// ---- the UDP passes' layouts ----
bool udp_layout(uint32_t iph, const uint64_t* data_off, uint64_t n, uint64_t* out_off) {
    for (uint64_t i = 0; i < n; ++i)
        if (data_off[i + 1] < data_off[i]) return false;  // everything checked before anything is written
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        out_off[i] = at;
        at += udp_slot(iph, data_off[i + 1] - data_off[i]);
    }
    out_off[n] = at;
    return true;
}

uint64_t udp_uso_layout(uint32_t iph, const uint64_t* data_off, const uint32_t* gso, uint64_t n, uint32_t* frame_seg,
                        uint64_t* out_off) {
    uint64_t f = 0, at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = data_off[i + 1] - data_off[i], cnt = tso_frames(len, gso[i]);
        for (uint64_t k = 0; k < cnt; ++k, ++f) {
            frame_seg[f] = (uint32_t)i;
            out_off[f] = at;
            at += udp_slot(iph, std::min<uint64_t>(gso[i], len - k * gso[i]));
        }
    }
    out_off[f] = at;
    return f;
}

// ---- IPv4 fragmentation's frame map ----
namespace {

constexpr uint64_t kFragBad = ~0ull;
constexpr uint64_t kFragLenCap = 1ull << 30;  // a frame this long is refused (include/nsx_csum.h)

// Output slots of a frame of len bytes at this mtu (>= 28): 1 when it fits, else the pieces of (mtu - 20) & ~7 bytes.
uint64_t frag_slots(uint64_t len, uint32_t mtu) {
    const uint64_t per = (mtu - 20u) & ~7u;
    return len <= mtu ? 1 : (len - 20 + per - 1) / per;
}

// The prefix sum of frag_slots into first (nullable), checked against expect (nullable): the slot count, or kFragBad.
uint64_t frag_walk(const uint64_t* offsets, const uint32_t* mtu, uint64_t n, const uint64_t* expect, uint64_t* first) {
    uint64_t f = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] >= kFragLenCap || mtu[i] < 28 ||
            (expect && expect[i] != f))
            return kFragBad;
        f += frag_slots(offsets[i + 1] - offsets[i], mtu[i]);
    }
    if (expect && expect[n] != f) return kFragBad;
    if (first) {  // everything checked before anything is written
        f = 0;
        for (uint64_t i = 0; i < n; ++i) {
            first[i] = f;
            f += frag_slots(offsets[i + 1] - offsets[i], mtu[i]);
        }
        first[n] = f;
    }
    return f;
}

}  // namespace

// ---- the NAT rewrite's translation table ----
uint32_t nat_hash(const uint8_t* t, uint32_t tuple_bytes) {
    uint32_t h = 0x811C9DC5u;
    for (uint32_t k = 0; k < tuple_bytes; k += 4) {
        const uint32_t lo = (uint32_t)t[k] | (uint32_t)t[k + 1] << 8, hi = (uint32_t)t[k + 2] | (uint32_t)t[k + 3] << 8;
        h = (h ^ (lo | hi << 16)) * 0x01000193u;
    }
    return h;
}

bool nat_table_build(uint32_t ip_ver, const uint8_t* match, const uint8_t* repl, uint64_t n_rules, uint8_t* table,
                     uint64_t slots) {
    if ((ip_ver != 4 && ip_ver != 6) || !table || (n_rules && (!match || !repl))) return false;
    if (!nat_slots_ok(slots) || slots < 16 || n_rules > slots / 2) return false;
    const uint32_t tb = nat_tuple_bytes(ip_ver), eb = nat_entry_bytes(ip_ver);
    std::memset(table, 0, slots * eb);
    for (uint64_t r = 0; r < n_rules; ++r) {
        const uint8_t* m = match + r * tb;
        const uint64_t home = nat_hash(m, tb) & (slots - 1);
        bool placed = false;
        for (uint64_t p = 0; p < slots && !placed; ++p) {  // at most half the entries are occupied: an empty one exists
            uint8_t* e = table + ((home + p) & (slots - 1)) * eb;
            const bool occupied = e[tb] == 1 && !e[tb + 1] && !e[tb + 2] && !e[tb + 3];
            if (occupied) {
                if (!std::memcmp(e, m, tb)) return false;  // a second rule for one match tuple
                continue;
            }
            std::memcpy(e, m, tb);
            e[tb] = 1;  // the state dword, little-endian
            std::memcpy(e + tb + 4, repl + r * tb, tb);
            placed = true;
        }
        if (!placed) return false;
    }
    return true;
}

}  // namespace nsx

extern "C" {

uint64_t nsx_tcp_wire_len(uint64_t opt_len, uint64_t data_len) {
    return 20u + opt_len + (opt_len ? (20u + opt_len) % 4u : 0u) + data_len;
}

int nsx_tcp_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, uint64_t n, uint64_t* h_out_off) {
    if (!h_out_off || (n && !h_data_off)) return NSX_EINVAL;
    nsx::packed_layout(0, h_opt_off, h_data_off, n, h_out_off);
    return NSX_OK;
}

int nsx_tx_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, uint64_t n, uint32_t ip_hdr_len,
                       uint64_t* h_out_off) {
    if ((ip_hdr_len != 20 && ip_hdr_len != 40) || !h_out_off || (n && !h_data_off)) return NSX_EINVAL;
    nsx::packed_layout(ip_hdr_len, h_opt_off, h_data_off, n, h_out_off);
    return NSX_OK;
}

int nsx_tso_count_host(const uint64_t* h_data_off, const uint32_t* h_mss, uint64_t n, uint64_t* h_frame_first) {
    if (!h_frame_first || n >= (1ull << 32) || (n && (!h_data_off || !h_mss))) return NSX_EINVAL;
    return nsx::tso_walk(nullptr, h_data_off, h_mss, n, nullptr, h_frame_first) == nsx::kTsoBad ? NSX_EINVAL : NSX_OK;
}

int nsx_tso_layout_host(const uint64_t* h_opt_off, const uint64_t* h_data_off, const uint32_t* h_mss,
                        const uint64_t* h_frame_first, uint64_t n, uint32_t ip_hdr_len, uint32_t* h_frame_seg,
                        uint64_t* h_out_off) {
    if ((ip_hdr_len != 20 && ip_hdr_len != 40) || !h_out_off || !h_frame_first || n >= (1ull << 32) ||
        (n && (!h_data_off || !h_mss)))
        return NSX_EINVAL;
    // everything checked before anything is written
    const uint64_t frames = nsx::tso_walk(h_opt_off, h_data_off, h_mss, n, h_frame_first, nullptr);
    if (frames == nsx::kTsoBad || (frames && !h_frame_seg)) return NSX_EINVAL;
    uint64_t at = 0;
    nsx::each_tso_frame(h_opt_off, h_data_off, h_mss, n, [&](uint64_t i, uint64_t f, uint64_t wire) {
        h_frame_seg[f] = (uint32_t)i;
        h_out_off[f] = at;
        at += nsx::slot_of(ip_hdr_len, wire);
        return true;
    });
    h_out_off[frames] = at;
    return NSX_OK;
}

int nsx_udp_layout_host(const uint64_t* h_data_off, uint64_t n, uint32_t ip_hdr_len, uint64_t* h_out_off) {
    if ((ip_hdr_len != 20 && ip_hdr_len != 40) || !h_out_off || (n && !h_data_off)) return NSX_EINVAL;
    return nsx::udp_layout(ip_hdr_len, h_data_off, n, h_out_off) ? NSX_OK : NSX_EINVAL;
}

int nsx_udp_uso_layout_host(const uint64_t* h_data_off, const uint32_t* h_gso, const uint64_t* h_frame_first,
                            uint64_t n, uint32_t ip_hdr_len, uint32_t* h_frame_seg, uint64_t* h_out_off) {
    if ((ip_hdr_len != 20 && ip_hdr_len != 40) || !h_out_off || !h_frame_first || n >= (1ull << 32) ||
        (n && (!h_data_off || !h_gso)))
        return NSX_EINVAL;
    // everything checked before anything is written: the map must be nsx_tso_count_host's
    const uint64_t frames = nsx::tso_walk(nullptr, h_data_off, h_gso, n, h_frame_first, nullptr);
    if (frames == nsx::kTsoBad || (frames && !h_frame_seg)) return NSX_EINVAL;
    nsx::udp_uso_layout(ip_hdr_len, h_data_off, h_gso, n, h_frame_seg, h_out_off);
    return NSX_OK;
}

int nsx_frag_count_host(const uint64_t* h_offsets, const uint32_t* h_mtu, uint64_t n, uint64_t* h_frag_first) {
    if (!h_frag_first || !h_offsets || n >= (1ull << 32) || (n && !h_mtu)) return NSX_EINVAL;
    return nsx::frag_walk(h_offsets, h_mtu, n, nullptr, h_frag_first) == nsx::kFragBad ? NSX_EINVAL : NSX_OK;
}

int nsx_frag_layout_host(const uint64_t* h_offsets, const uint32_t* h_mtu, const uint64_t* h_frag_first, uint64_t n,
                         uint32_t* h_frag_src, uint64_t* h_out_off) {
    if (!h_out_off || !h_frag_first || !h_offsets || n >= (1ull << 32) || (n && !h_mtu)) return NSX_EINVAL;
    // everything checked before anything is written: the map must be nsx_frag_count_host's
    const uint64_t slots = nsx::frag_walk(h_offsets, h_mtu, n, h_frag_first, nullptr);
    if (slots == nsx::kFragBad || (slots && !h_frag_src)) return NSX_EINVAL;
    uint64_t f = 0, at = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t len = h_offsets[i + 1] - h_offsets[i], per = (h_mtu[i] - 20u) & ~7u;
        const uint64_t cnt = nsx::frag_slots(len, h_mtu[i]);
        for (uint64_t j = 0; j < cnt; ++j, ++f) {
            h_frag_src[f] = (uint32_t)i;
            h_out_off[f] = at;
            at += len <= h_mtu[i] ? len : 20 + std::min(per, len - 20 - j * per);
        }
    }
    h_out_off[f] = at;
    return NSX_OK;
}

int nsx_nat_table_slots(uint64_t n_rules, uint64_t* out_slots) {
    if (!out_slots || n_rules >= (1ull << 31)) return NSX_EINVAL;
    uint64_t s = 16;
    while (s < 2 * n_rules) s <<= 1;
    *out_slots = s;
    return NSX_OK;
}

int nsx_nat_table_build_host(uint32_t ip_ver, const uint8_t* h_match, const uint8_t* h_new, uint64_t n_rules,
                             void* h_table, uint64_t slots) {
    return nsx::nat_table_build(ip_ver, h_match, h_new, n_rules, static_cast<uint8_t*>(h_table), slots) ? NSX_OK
                                                                                                      : NSX_EINVAL;
}

}  // extern "C"
