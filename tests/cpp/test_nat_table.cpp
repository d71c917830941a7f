// test_nat_table.cpp — the NAT rewrite's table builder (nsx_nat_table_slots, nsx_nat_table_build_host in
// network-stack_amd/csrc/host_plan.cpp) on its own, built with AddressSanitizer + UBSan by
// tests/test_nat_table_cpp.py. The tables live in exactly sized heap blocks, so a byte written past slots entries
// is a report. Covered: n_rules = 0, exactly half full, wrap-around past the last slot, duplicates, the refusals,
// and seeded random rule sets looked up again with a probe written here. Prints OK.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

using Bytes = std::vector<uint8_t>;

static uint32_t tuple_bytes(uint32_t v) { return v == 6 ? 36 : 12; }
static uint32_t entry_bytes(uint32_t v) { return v == 6 ? 80 : 32; }

// the header's hash, restated
static uint32_t key(const uint8_t* t, uint32_t tb) {
    uint32_t h = 0x811C9DC5u;
    for (uint32_t k = 0; k < tb; k += 4) {
        uint32_t w;
        std::memcpy(&w, t + k, 4);  // the test runs on a little-endian host
        h = (h ^ w) * 0x01000193u;
    }
    return h;
}

static bool occupied(const uint8_t* e, uint32_t tb) {
    uint32_t s;
    std::memcpy(&s, e + tb, 4);
    return s == 1;
}

// the header's lookup, restated: the entry's slot, or -1 for a miss
static int64_t lookup(const Bytes& table, uint64_t slots, uint32_t v, const uint8_t* t) {
    const uint32_t tb = tuple_bytes(v), eb = entry_bytes(v);
    const uint64_t home = key(t, tb) & (slots - 1);
    for (uint64_t p = 0; p < slots; ++p) {
        const uint64_t s = (home + p) & (slots - 1);
        const uint8_t* e = table.data() + s * eb;
        if (!occupied(e, tb)) return -1;
        if (!std::memcmp(e, t, tb)) return (int64_t)s;
    }
    return -1;
}

static Bytes random_tuples(std::mt19937_64& rng, uint64_t n, uint32_t v) {
    Bytes b(n * tuple_bytes(v));
    for (auto& x : b) x = (uint8_t)rng();
    return b;
}

// a tuple whose home slot is `home`: random bytes, the last dword searched for
static void tuple_at_home(std::mt19937_64& rng, uint32_t v, uint64_t home, uint64_t slots, uint8_t* t) {
    const uint32_t tb = tuple_bytes(v);
    for (;;) {
        for (uint32_t k = 0; k < tb; ++k) t[k] = (uint8_t)rng();
        if ((key(t, tb) & (slots - 1)) == home) return;
    }
}

static uint64_t count_occupied(const Bytes& table, uint64_t slots, uint32_t v) {
    uint64_t c = 0;
    for (uint64_t s = 0; s < slots; ++s) c += occupied(table.data() + s * entry_bytes(v), tuple_bytes(v));
    return c;
}

static void check_built(uint32_t v, const Bytes& match, const Bytes& repl, uint64_t n, uint64_t slots) {
    const uint32_t tb = tuple_bytes(v), eb = entry_bytes(v);
    Bytes table(slots * eb, 0xCD);  // exactly sized: ASan sees a write past the last entry
    CHECK(nsx_nat_table_build_host(v, n ? match.data() : nullptr, n ? repl.data() : nullptr, n, table.data(), slots) ==
          NSX_OK);
    CHECK(count_occupied(table, slots, v) == n);
    for (uint64_t r = 0; r < n; ++r) {
        const int64_t s = lookup(table, slots, v, match.data() + r * tb);
        CHECK(s >= 0);
        const uint8_t* e = table.data() + (uint64_t)s * eb;
        CHECK(!std::memcmp(e + tb + 4, repl.data() + r * tb, tb));
        for (uint32_t k = 0; k < 4; ++k) CHECK(e[2 * tb + 4 + k] == 0);
    }
    for (uint64_t s = 0; s < slots; ++s) {  // an entry that is not occupied is all zero
        const uint8_t* e = table.data() + s * eb;
        if (occupied(e, tb)) continue;
        for (uint32_t k = 0; k < eb; ++k) CHECK(e[k] == 0);
    }
}

int main() {
    std::mt19937_64 rng(0x4A7);
    // nsx_nat_table_slots
    uint64_t s = 0;
    const uint64_t want[][2] = {{0, 16}, {1, 16}, {8, 16}, {9, 32}, {16, 32}, {17, 64}, {1u << 20, 1u << 21},
                                {(1ull << 30) + 1, 1ull << 32}, {(1ull << 31) - 1, 1ull << 32}};
    for (const auto& w : want) CHECK(nsx_nat_table_slots(w[0], &s) == NSX_OK && s == w[1]);
    CHECK(nsx_nat_table_slots(1ull << 31, &s) == NSX_EINVAL && nsx_nat_table_slots(~0ull, &s) == NSX_EINVAL);
    CHECK(nsx_nat_table_slots(4, nullptr) == NSX_EINVAL);

    for (uint32_t v : {4u, 6u}) {
        const uint32_t tb = tuple_bytes(v), eb = entry_bytes(v);
        // n_rules = 0: the table is zero-filled, NULL rule arrays are fine
        check_built(v, {}, {}, 0, 16);
        check_built(v, {}, {}, 0, 1024);
        // exactly half full, and every load below it
        for (uint64_t slots : {16ull, 64ull, 4096ull})
            for (uint64_t n : {uint64_t(1), slots / 2 - 1, slots / 2})
                check_built(v, random_tuples(rng, n, v), random_tuples(rng, n, v), n, slots);
        // wrap-around: 6 tuples whose home is the last slot but one land in slots 14, 15, 0, 1, 2, 3, in rule order
        {
            const uint64_t slots = 16, n = 6;
            Bytes match(n * tb), repl = random_tuples(rng, n, v);
            for (uint64_t r = 0; r < n; ++r) tuple_at_home(rng, v, 14, slots, match.data() + r * tb);
            check_built(v, match, repl, n, slots);
            Bytes table(slots * eb);
            CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), n, table.data(), slots) == NSX_OK);
            for (uint64_t r = 0; r < n; ++r)
                CHECK(lookup(table, slots, v, match.data() + r * tb) == (int64_t)((14 + r) & 15));
            uint8_t absent[36];
            tuple_at_home(rng, v, 14, slots, absent);  // walks the whole chain to the empty slot 4
            CHECK(lookup(table, slots, v, absent) == -1);
        }
        // duplicates: anywhere in the rule list, and behind a collision chain
        {
            Bytes match = random_tuples(rng, 8, v), repl = random_tuples(rng, 8, v), table(32 * eb);
            CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), 8, table.data(), 32) == NSX_OK);
            Bytes dup = match;
            std::memcpy(dup.data() + 7 * tb, dup.data(), tb);
            CHECK(nsx_nat_table_build_host(v, dup.data(), repl.data(), 8, table.data(), 32) == NSX_EINVAL);
            dup = match;
            std::memcpy(dup.data() + 1 * tb, dup.data(), tb);
            CHECK(nsx_nat_table_build_host(v, dup.data(), repl.data(), 8, table.data(), 32) == NSX_EINVAL);
            for (uint64_t r = 0; r < 4; ++r) tuple_at_home(rng, v, 30, 32, dup.data() + r * tb);
            std::memcpy(dup.data() + 4 * tb, dup.data(), tb);  // found after wrapping past three other entries
            CHECK(nsx_nat_table_build_host(v, dup.data(), repl.data(), 5, table.data(), 32) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, dup.data(), repl.data(), 4, table.data(), 32) == NSX_OK);
            // equal new tuples are no duplicates
            for (uint64_t r = 1; r < 8; ++r) std::memcpy(repl.data() + r * tb, repl.data(), tb);
            CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), 8, table.data(), 32) == NSX_OK);
        }
        // refusals: nothing is written (the block is one byte long)
        {
            Bytes match = random_tuples(rng, 9, v), repl = random_tuples(rng, 9, v), tiny(1);
            for (uint64_t slots : {0ull, 1ull, 8ull, 16ull, 17ull, 24ull, 48ull, (1ull << 31) + 1, 1ull << 32, ~0ull})
                CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), 9, tiny.data(), slots) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, nullptr, repl.data(), 9, tiny.data(), 32) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, match.data(), nullptr, 9, tiny.data(), 32) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), 9, nullptr, 32) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, nullptr, nullptr, 0, nullptr, 16) == NSX_EINVAL);
            CHECK(nsx_nat_table_build_host(v, match.data(), repl.data(), 1ull << 40, tiny.data(), 1ull << 31) ==
                  NSX_EINVAL);
        }
        for (uint32_t bad : {0u, 5u, 7u, 46u}) {
            Bytes match = random_tuples(rng, 2, 6), table(16 * 80);
            CHECK(nsx_nat_table_build_host(bad, match.data(), match.data(), 2, table.data(), 16) == NSX_EINVAL);
        }
        // seeded random rule sets at random loads
        for (int it = 0; it < 40; ++it) {
            const uint64_t slots = 16ull << (rng() % 8), n = rng() % (slots / 2 + 1);
            check_built(v, random_tuples(rng, n, v), random_tuples(rng, n, v), n, slots);
        }
    }
    std::printf("OK\n");
    return 0;
}
