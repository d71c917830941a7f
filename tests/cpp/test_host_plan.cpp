// test_host_plan.cpp — the host batch calls' planning unit (network-stack_amd/csrc/host_plan.cpp) on its own, built
// with AddressSanitizer + UBSan by tests/test_host_plan_cpp.py: chunk cuts, shard bounds, the sender job's staging
// layout and the frame-map validators, on hand-computed cases and seeded random ones. Prints OK.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../network-stack_amd/csrc/host_plan.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

using nsx::Chunk;
using nsx::Cut;
using U64 = std::vector<uint64_t>;

static const uint64_t kBudgets[] = {1, 64, 4096, 64ull << 20};

static U64 prefix(const U64& lens, uint64_t lead) {
    U64 off(lens.size() + 1, lead);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    return off;
}

// lengths with empty segments, runs of small ones and a few far above the small budgets
static U64 random_lens(std::mt19937_64& rng, size_t n, uint64_t big) {
    U64 v(n);
    for (auto& x : v) {
        const uint64_t k = rng() % 10;
        x = k == 0 ? 0 : k == 1 ? big + rng() % big : rng() % 200;
    }
    return v;
}

// chunks tile [lo, hi) in order, without gap or overlap
static void check_tiling(const std::vector<Chunk>& v, uint64_t lo, uint64_t hi) {
    uint64_t at = lo;
    for (const Chunk& c : v) {
        CHECK(c.c0 == at && c.c1 > c.c0 && c.c1 <= hi);
        at = c.c1;
    }
    CHECK(at == hi);
}

static void check_offset_cut(Cut cut, const U64& off, uint64_t lo, uint64_t hi, uint64_t budget) {
    const std::vector<Chunk> v = nsx::plan_chunks(cut, off.data(), 0, 0, lo, hi, budget);
    check_tiling(v, lo, hi);
    for (const Chunk& c : v) {
        CHECK(c.byte_lo == off[c.c0] && c.byte_hi == off[c.c1]);
        const uint64_t cn = c.c1 - c.c0;
        if (cut == Cut::kRx) {
            CHECK(c.byte_hi - c.byte_lo <= budget || cn <= 64);
            if (lo % 64 == 0) CHECK(c.c0 % 64 == 0);
            if (c.c1 < hi) CHECK(cn >= 64 && cn % 64 == 0);  // only the shard's last chunk is partial
        } else {
            CHECK(c.byte_hi - c.byte_lo <= budget || cn == 1);
            if (c.c1 < hi) CHECK(off[c.c1 + 1] - off[c.c0] > budget);  // and no chunk stops early
        }
    }
}

static void test_fixed() {
    // 37 segments of 1500 B every 1503 B, 4096 B budget: two per chunk, the last alone
    std::vector<Chunk> v = nsx::plan_chunks(Cut::kFixed, nullptr, 1503, 1500, 0, 37, 4096);
    CHECK(v.size() == 19 && v[0].c1 == 2 && v[18].c0 == 36 && v[18].c1 == 37);
    CHECK(v[1].byte_lo == 2 * 1503 && v[1].byte_hi == 3 * 1503 + 1500);
    v = nsx::plan_chunks(Cut::kFixed, nullptr, 1503, 5000, 0, 37, 4096);  // larger than the budget: one each
    CHECK(v.size() == 37);
    v = nsx::plan_chunks(Cut::kFixed, nullptr, 0, 0, 3, 10, 1);  // zero stride and length: max(stride, seg_len, 1)
    CHECK(v.size() == 7);
    std::mt19937_64 rng(0x1071);
    for (int it = 0; it < 200; ++it) {
        const uint64_t stride = rng() % 3000, seg_len = rng() % 3000, lo = rng() % 50, hi = lo + rng() % 300;
        for (uint64_t budget : kBudgets) {
            v = nsx::plan_chunks(Cut::kFixed, nullptr, stride, (uint32_t)seg_len, lo, hi, budget);
            check_tiling(v, lo, hi);
            const uint64_t span = std::max<uint64_t>(std::max(stride, seg_len), 1), per = std::max<uint64_t>(1, budget / span);
            for (const Chunk& c : v) {
                CHECK(c.byte_lo == c.c0 * stride && c.byte_hi == (c.c1 - 1) * stride + seg_len);
                CHECK(c.c1 - c.c0 == per || c.c1 == hi);
                CHECK((c.c1 - c.c0) * span <= budget || c.c1 - c.c0 == 1);
            }
        }
    }
}

static void test_ragged_and_rx() {
    const U64 off = {0, 10, 20, 100, 100, 130};
    std::vector<Chunk> v = nsx::plan_chunks(Cut::kRagged, off.data(), 0, 0, 0, 5, 64);
    CHECK(v.size() == 3 && v[0].c1 == 2 && v[1].c1 == 3 && v[2].c1 == 5 && v[1].byte_lo == 20 && v[1].byte_hi == 100);
    // 200 frames of 40 B: 51 fit 2048 B, a chunk is never below one mask word; 130 fit 5200 B, floored to 128
    const U64 rx = prefix(U64(200, 40), 0);
    v = nsx::plan_chunks(Cut::kRx, rx.data(), 0, 0, 0, 200, 2048);
    CHECK(v.size() == 4 && v[0].c1 == 64 && v[2].c1 == 192 && v[3].c1 == 200);
    v = nsx::plan_chunks(Cut::kRx, rx.data(), 0, 0, 0, 200, 5200);
    CHECK(v.size() == 2 && v[0].c1 == 128);
    v = nsx::plan_chunks(Cut::kRx, rx.data(), 0, 0, 64, 200, 64ull << 20);
    CHECK(v.size() == 1 && v[0].c0 == 64 && v[0].c1 == 200 && v[0].byte_lo == 64 * 40);
    std::mt19937_64 rng(0x1072);
    for (int it = 0; it < 100; ++it) {
        const size_t n = 1 + rng() % 700;
        const U64 o = prefix(random_lens(rng, n, 5000), rng() % 7);
        for (uint64_t budget : kBudgets) {
            const uint64_t lo = rng() % n, lo64 = lo / 64 * 64;
            check_offset_cut(Cut::kRagged, o, lo, n, budget);
            check_offset_cut(Cut::kRagged, o, 0, lo, budget);
            check_offset_cut(Cut::kRx, o, lo64, n, budget);
            check_offset_cut(Cut::kRx, o, 0, lo64, budget);
        }
    }
}

static void test_sender_cut() {
    const U64 seg_out = {0, 40, 80, 120, 160}, data_off = {0, 0, 100, 100, 100};
    std::vector<Chunk> v = nsx::plan_sender_chunks(seg_out.data(), data_off.data(), 0, 4, 100);
    CHECK(v.size() == 2 && v[0].c1 == 2 && v[1].byte_lo == 80 && v[1].byte_hi == 160);
    std::mt19937_64 rng(0x1073);
    for (int it = 0; it < 100; ++it) {
        const size_t n = 1 + rng() % 400;
        const U64 d = prefix(random_lens(rng, n, 5000), rng() % 300);
        U64 img(n);
        for (size_t i = 0; i < n; ++i) img[i] = (20 + (d[i + 1] - d[i]) + 3 + 4 * (rng() % 3)) & ~3ull;
        const U64 o = prefix(img, 0);
        for (uint64_t budget : kBudgets) {
            const uint64_t lo = rng() % n;
            v = nsx::plan_sender_chunks(o.data(), d.data(), lo, n, budget);
            check_tiling(v, lo, n);
            for (const Chunk& c : v) {
                CHECK(c.byte_lo == o[c.c0] && c.byte_hi == o[c.c1]);
                CHECK((c.byte_hi - c.byte_lo <= budget && d[c.c1] - d[c.c0] <= budget) || c.c1 - c.c0 == 1);
                if (c.c1 < n) CHECK(o[c.c1 + 1] - o[c.c0] > budget || d[c.c1 + 1] - d[c.c0] > budget);
            }
        }
    }
}

static void test_shards() {
    CHECK(nsx::auto_gpus(0, 8) == 1 && nsx::auto_gpus(64ull << 20, 8) == 1 && nsx::auto_gpus((64ull << 20) + 1, 8) == 2);
    CHECK(nsx::auto_gpus(1ull << 40, 8) == 8);
    std::mt19937_64 rng(0x1074);
    for (int it = 0; it < 200; ++it) {
        const uint64_t n = 1 + rng() % 3000;
        const int parts = (int)std::min<uint64_t>(n, 1 + rng() % 24);
        const U64 off = prefix(random_lens(rng, n, 9000), 1);
        for (int mode = 0; mode < 3; ++mode) {  // by count; by bytes; by bytes on mask words
            const U64 b = nsx::shard_bounds(mode ? off.data() : nullptr, n, parts, mode == 2);
            CHECK(b.size() == (size_t)parts + 1 && b[0] == 0 && b[parts] == n);
            for (int g = 0; g < parts; ++g) {
                CHECK(b[g] <= b[g + 1]);
                if (mode == 2) CHECK(b[g] % 64 == 0 || b[g] == n);  // a bound clipped to n starts an empty shard
            }
        }
    }
}

static void test_staging_layout() {
    uint16_t p16[1];
    uint32_t p32[1];
    uint8_t p8[1];
    const nsx_tcp_hdr_soa tcp{p16, p16, p32, p32, nullptr, p8, p16, p16};  // offset NULL: computed on the device
    const nsx_ip_hdr_soa ip{p8, p8, nullptr, p8, nullptr, p32};
    for (int ipver : {4, 6}) {
        for (int set = 0; set < 3; ++set) {  // TCP images, datagrams, segmentation offload
            const nsx::FieldSet fs = nsx::sender_fields(&tcp, set ? &ip : nullptr, ipver, set == 2 ? p32 : nullptr);
            CHECK(fs.n == (set == 0 ? 8 : set == 1 ? 14 : 15));
            uint64_t per_seg = 0;
            for (int f = 0; f < fs.n; ++f) per_seg += fs.esz[f];
            CHECK(per_seg == 18u + (set ? 2u * (ipver == 4 ? 4u : 16u) + 8u : 0u) + (set == 2 ? 4u : 0u));
            for (uint64_t cn : {1ull, 2ull, 127ull, 128ull, 129ull, 5000ull}) {
                uint64_t at[nsx::kAllFields];
                const uint64_t bytes = nsx::field_block(fs, cn, at);
                for (int f = 0; f < fs.n; ++f) {
                    CHECK(at[f] % 256 == 0);
                    CHECK(at[f] + cn * fs.esz[f] <= (f + 1 < fs.n ? at[f + 1] : bytes));
                }
                CHECK(bytes % 256 == 0);
                uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(0x10000));
                nsx_tcp_hdr_soa dt;
                nsx_ip_hdr_soa di;
                const uint32_t* dm;
                nsx::field_block_soa(fs, at, base, &dt, &di, &dm);
                CHECK((const uint8_t*)dt.src_port == base && (const uint8_t*)dt.seq_num == base + at[2]);
                CHECK(dt.offset == nullptr && dt.control == base + at[5] && (const uint8_t*)dt.urgent_ptr == base + at[7]);
                CHECK(set ? (di.src == base + at[8] && !di.ident && di.ttl == base + at[11] && !di.tclass &&
                             (const uint8_t*)di.flow == base + at[13])
                          : (!di.src && !di.dst && !di.flow));
                CHECK(set == 2 ? (const uint8_t*)dm == base + at[14] : dm == nullptr);
            }
        }
    }
    for (uint64_t cn : {1ull, 7ull, 64ull})
        for (uint64_t fn : {1ull, 2ull, 7ull, 64ull, 1001ull})
            for (int opts = 0; opts < 2; ++opts)
                for (int tso = 0; tso < 2; ++tso) {
                    const nsx::OffBlock b = nsx::off_block(cn, fn, opts, tso);
                    CHECK(b.at_out == cn + 1 && b.at_opt == b.at_out + fn + 1);  // data_off, then out_off
                    CHECK(b.at_first == b.at_opt + (opts ? cn + 1 : 0));
                    if (tso) {
                        CHECK(b.at_seg == b.at_first + cn + 1 && b.words >= b.at_seg && (b.words - b.at_seg) * 8 >= fn * 4);
                        CHECK(b.words == b.at_seg + (fn + 1) / 2);
                    } else {
                        CHECK(b.words == b.at_first);
                    }
                }
    for (uint64_t d0 : {0ull, 1ull, 7ull, 255ull, 256ull, 1000003ull}) {
        CHECK(nsx::lead_data(d0) >= 256 && nsx::lead_data(d0) < 512 && nsx::lead_data(d0) % 256 == d0 % 256);
        CHECK(nsx::lead_out(d0) < 256 && nsx::lead_out(d0) % 256 == d0 % 256);
    }
}

static void test_frame_map() {
    const U64 doff = {0, 3000, 3000, 9000}, ooff = {0, 4, 4, 12};
    const std::vector<uint32_t> mss = {1460, 1460, 1000};
    U64 first(4, 77);
    CHECK(nsx_tso_count_host(doff.data(), mss.data(), 3, first.data()) == NSX_OK);
    CHECK((first == U64{0, 3, 4, 10}));
    CHECK(nsx::tso_frames(0, 5) == 1 && nsx::tso_frames(5, 5) == 1 && nsx::tso_frames(6, 5) == 2);
    const std::vector<uint32_t> mss0 = {1460, 0, 1000};
    const U64 doff_back = {0, 3000, 2999, 9000}, ooff_back = {0, 4, 3, 12};
    CHECK(nsx_tso_count_host(doff.data(), mss0.data(), 3, first.data()) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(doff_back.data(), mss.data(), 3, first.data()) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(doff.data(), mss.data(), 1ull << 32, first.data()) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(nullptr, mss.data(), 3, first.data()) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(doff.data(), nullptr, 3, first.data()) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(doff.data(), mss.data(), 3, nullptr) == NSX_EINVAL);
    CHECK(nsx_tso_count_host(nullptr, nullptr, 0, first.data()) == NSX_OK && first[0] == 0);
    first = {0, 3, 4, 10};
    // the walk accepts the count's own output and refuses every other map
    CHECK(nsx::tso_walk(ooff.data(), doff.data(), mss.data(), 3, first.data(), nullptr) == 10);
    CHECK(nsx::tso_walk(ooff.data(), doff.data(), mss0.data(), 3, first.data(), nullptr) == nsx::kTsoBad);
    CHECK(nsx::tso_walk(ooff.data(), doff_back.data(), mss.data(), 3, first.data(), nullptr) == nsx::kTsoBad);
    CHECK(nsx::tso_walk(ooff_back.data(), doff.data(), mss.data(), 3, first.data(), nullptr) == nsx::kTsoBad);
    for (const U64& bad : {U64{0, 3, 4, 11}, U64{0, 2, 4, 10}, U64{1, 3, 4, 10}, U64{0, 3, 5, 10}, U64{0, 1, 3, 5}})
        CHECK(nsx::tso_walk(ooff.data(), doff.data(), mss.data(), 3, bad.data(), nullptr) == nsx::kTsoBad);
    // nsx_tso_layout_host: refusals write nothing
    std::vector<uint32_t> seg(10, 0xEEEE);
    U64 off(11, 0xEEEE);
    const U64 wrong = {0, 3, 4, 11};
    CHECK(nsx_tso_layout_host(ooff.data(), doff.data(), mss.data(), wrong.data(), 3, 20, seg.data(), off.data()) == NSX_EINVAL);
    CHECK(nsx_tso_layout_host(ooff.data(), doff.data(), mss.data(), first.data(), 3, 24, seg.data(), off.data()) == NSX_EINVAL);
    CHECK(nsx_tso_layout_host(ooff.data(), doff.data(), mss.data(), first.data(), 3, 20, nullptr, off.data()) == NSX_EINVAL);
    for (uint32_t s : seg) CHECK(s == 0xEEEE);
    for (uint64_t o : off) CHECK(o == 0xEEEE);
    CHECK(nsx_tso_layout_host(ooff.data(), doff.data(), mss.data(), first.data(), 3, 20, seg.data(), off.data()) == NSX_OK);
    CHECK((seg == std::vector<uint32_t>{0, 0, 0, 1, 2, 2, 2, 2, 2, 2}));
    CHECK(off[0] == 0 && off[1] == 20 + 24 + 1460 && off[4] - off[3] == 40 && off[10] - off[9] == 20 + 28 + 1000);
    // the sender's check of that layout: first image offsets per super-segment, no gaps; then each malformation
    U64 seg_out(4);
    bool gaps = true;
    CHECK(nsx::tso_layout_ok(20, ooff.data(), doff.data(), mss.data(), 3, seg.data(), off.data(), 10, seg_out.data(), &gaps));
    CHECK(!gaps && seg_out[3] == off[10]);
    for (int i = 0; i < 3; ++i) CHECK(seg_out[i] == off[first[i]]);
    auto ok = [&](const std::vector<uint32_t>& s, const U64& o, uint32_t iph = 20) {
        return nsx::tso_layout_ok(iph, ooff.data(), doff.data(), mss.data(), 3, s.data(), o.data(), 10, seg_out.data(), &gaps);
    };
    std::vector<uint32_t> wrong_seg = seg;
    wrong_seg[2] = 2;
    U64 shifted = off, shorter = off, back = off, wide = off;
    for (auto& x : shifted) x += 2;
    shorter[2] -= 4;
    back[3] = back[1];
    for (size_t f = 5; f < wide.size(); ++f) wide[f] += 8;
    CHECK(!ok(wrong_seg, off) && !ok(seg, shifted) && !ok(seg, shorter) && !ok(seg, back));
    CHECK(!ok(seg, off, 40));  // slots laid out for IPv4 headers do not hold IPv6 datagrams
    CHECK(ok(seg, wide) && gaps && seg_out[2] == wide[4]);
    // a frame whose TCP part does not fit the IPv4 length field
    const U64 d1 = {0, 65496}, o1 = {0, 20 + 20 + 65496};
    const std::vector<uint32_t> m1 = {65496}, s1 = {0};
    CHECK(!nsx::tso_layout_ok(20, nullptr, d1.data(), m1.data(), 1, s1.data(), o1.data(), 1, seg_out.data(), &gaps));
    CHECK(nsx::tso_layout_ok(40, nullptr, d1.data(), m1.data(), 1, s1.data(), U64{0, 40 + 20 + 65496}.data(), 1,
                             seg_out.data(), &gaps));
}

static void test_sender_layout() {
    const U64 doff = {7, 7, 8, 1488}, ooff = {1, 1, 5, 5};
    U64 packed(4), tx(4);
    CHECK(nsx_tcp_layout_host(ooff.data(), doff.data(), 3, packed.data()) == NSX_OK);
    CHECK((packed == U64{0, 20, 48, 1548}));  // 20; 20 + 4 + 1 padded to 28; 20 + 1480
    CHECK(nsx_tx_layout_host(ooff.data(), doff.data(), 3, 40, tx.data()) == NSX_OK && (tx == U64{0, 60, 128, 1668}));
    CHECK(nsx_tx_layout_host(ooff.data(), doff.data(), 3, 24, tx.data()) == NSX_EINVAL);
    CHECK(nsx_tcp_wire_len(0, 5) == 25 && nsx_tcp_wire_len(1, 0) == 22 && nsx_tcp_wire_len(4, 1) == 25);
    bool gaps = true;
    CHECK(nsx::sender_layout_ok(0, ooff.data(), doff.data(), packed.data(), 3, &gaps) && !gaps);
    CHECK(!nsx::sender_layout_ok(20, ooff.data(), doff.data(), packed.data(), 3, &gaps));  // no room for IP headers
    CHECK(nsx::sender_layout_ok(40, ooff.data(), doff.data(), tx.data(), 3, &gaps) && !gaps);
    U64 wide = packed, odd = packed, tight = packed;
    wide[2] += 4, wide[3] += 4;
    odd[1] += 2;
    tight[3] -= 4;
    CHECK(nsx::sender_layout_ok(0, ooff.data(), doff.data(), wide.data(), 3, &gaps) && gaps);
    CHECK(!nsx::sender_layout_ok(0, ooff.data(), doff.data(), odd.data(), 3, &gaps));
    CHECK(!nsx::sender_layout_ok(0, ooff.data(), doff.data(), tight.data(), 3, &gaps));
    const U64 dback = {7, 9, 8, 1488};
    CHECK(!nsx::sender_layout_ok(0, ooff.data(), dback.data(), wide.data(), 3, &gaps));
    uint16_t p16[1];
    uint32_t p32[1];
    uint8_t p8[1];
    nsx_tcp_hdr_soa tcp{p16, p16, p32, p32, nullptr, p8, p16, p16};
    CHECK(nsx::tcp_hdr_ok(&tcp) && !nsx::tcp_hdr_ok(nullptr));
    tcp.window = nullptr;
    CHECK(!nsx::tcp_hdr_ok(&tcp));
    nsx_ip_hdr_soa ip{p8, p8, nullptr, nullptr, nullptr, nullptr};
    CHECK(nsx::ip_hdr_ok(&ip) && !nsx::ip_hdr_ok(nullptr));
    ip.dst = nullptr;
    CHECK(!nsx::ip_hdr_ok(&ip));
}

int main() {
    test_fixed();
    test_ragged_and_rx();
    test_sender_cut();
    test_shards();
    test_staging_layout();
    test_frame_map();
    test_sender_layout();
    std::printf("OK\n");
    return 0;
}
