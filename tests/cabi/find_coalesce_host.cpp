// find_coalesce_host.cpp — TEST INFRASTRUCTURE: the host bookkeeping of captured finds (csrc/meepo_find_coalesce.h) under ASan + UBSan, no GPU and no
// HIP: the overlap test against a byte-map reference, the descriptor's rebuild at its limits (16 requests, 2^31 blocks, empty requests), and the table
// of recorded nodes (oldest out, one entry per capture id).  Built and run by tests/test_find_coalesce_host.py; exit status 0 and one "ok" line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "meepo_find_coalesce.h"

using namespace mee;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "find_coalesce_host: line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main() {
    // ---- bytes_overlap: half-open ranges; null or empty ranges touch nothing
    char* base = (char*)0x10000;
    CHECK(bytes_overlap(base, 16, base + 15, 1) && !bytes_overlap(base, 16, base + 16, 1) && !bytes_overlap(base + 16, 4, base, 16));
    CHECK(!bytes_overlap(nullptr, 16, base, 16) && !bytes_overlap(base, 0, base, 16) && bytes_overlap(base + 4, 4, base, 16));

    // ---- find_request_disjoint against a byte map: an arena of 4096 bytes, requests placed at random in it
    const uint64_t row_bytes = 16, arena = 4096;
    int joined = 0, refused = 0;
    for (int trial = 0; trial < 4000; ++trial) {
        FindMany m{};
        std::vector<uint8_t> reads(arena, 0), writes(arena, 0);
        for (int q = 0; q < 6; ++q) {
            const uint64_t n = 1 + rnd() % 6;
            const uint64_t ko = (rnd() % (arena - n * 8)) & ~7ull, oo = (rnd() % (arena - n * row_bytes)) & ~15ull, fo = rnd() % (arena - n);
            const bool has_found = rnd() % 4 != 0;
            const int64_t* keys = (const int64_t*)(base + ko);
            f32x4* out = (f32x4*)(base + oo);
            uint8_t* found = has_found ? (uint8_t*)(base + fo) : nullptr;
            bool clash = false;   // the new request's writes on anything touched before, its reads on anything written before
            for (uint64_t b = 0; b < n * row_bytes; ++b) clash = clash || reads[oo + b] || writes[oo + b];
            for (uint64_t b = 0; has_found && b < n; ++b) clash = clash || reads[fo + b] || writes[fo + b];
            for (uint64_t b = 0; b < n * 8; ++b) clash = clash || writes[ko + b];
            CHECK(find_request_disjoint(m, row_bytes, keys, n, out, found) == !clash);
            if (clash) { ++refused; continue; }
            CHECK(find_many_append(m, keys, n, out, found, (uint32_t)(1 + rnd() % 3)));
            for (uint64_t b = 0; b < n * row_bytes; ++b) writes[oo + b] = 1;
            for (uint64_t b = 0; has_found && b < n; ++b) writes[fo + b] = 1;
            for (uint64_t b = 0; b < n * 8; ++b) reads[ko + b] = 1;
            ++joined;
        }
        for (uint32_t q = 0; q < m.count; ++q) CHECK(m.first_block[q] < m.first_block[q + 1]);
    }
    CHECK(joined > 1000 && refused > 1000);
    {   // a request's own keys may lie in its own output's neighbourhood but two requests may share KEYS (both only read them)
        FindMany m{};
        CHECK(find_many_append(m, (const int64_t*)base, 4, (f32x4*)(base + 1024), nullptr, 1));
        CHECK(find_request_disjoint(m, row_bytes, (const int64_t*)base, 4, base + 2048, nullptr));
        CHECK(!find_request_disjoint(m, row_bytes, (const int64_t*)(base + 1024 + 56), 1, base + 2048, nullptr));   // keys in the last bytes of an earlier output
        CHECK(!find_request_disjoint(m, row_bytes, (const int64_t*)(base + 3000), 4, base + 16, nullptr));          // output over an earlier request's keys
    }

    // ---- find_many_append at its limits: `m` stays as it was when a request is refused
    {
        FindMany m{};
        CHECK(!find_many_append(m, (const int64_t*)base, 0, (f32x4*)base, nullptr, 1) && !find_many_append(m, (const int64_t*)base, 8, (f32x4*)base, nullptr, 0) && m.count == 0);
        uint32_t total = 0;
        for (int q = 0; q < kMaxFindRequests; ++q) {
            const uint32_t blocks = 1 + (uint32_t)(rnd() % 1000);
            CHECK(find_many_append(m, (const int64_t*)base + q, 8 + q, (f32x4*)base + q, nullptr, blocks));
            CHECK(m.first_block[q] == total && m.n[q] == (uint64_t)(8 + q) && m.keys[q] == (const int64_t*)base + q);
            total += blocks;
            CHECK(m.count == (uint32_t)q + 1 && m.first_block[m.count] == total);
            for (int i = q + 2; i <= kMaxFindRequests; ++i) CHECK(m.first_block[i] == 0xFFFFFFFFu);   // what the kernel's block-to-request count relies on
        }
        const FindMany full = m;
        CHECK(!find_many_append(m, (const int64_t*)base, 8, (f32x4*)base, nullptr, 1) && !memcmp(&m, &full, sizeof m));
        FindMany big{};
        CHECK(find_many_append(big, (const int64_t*)base, 8, (f32x4*)base, nullptr, (1u << 30) + 5));
        CHECK(find_many_append(big, (const int64_t*)base, 8, (f32x4*)base, nullptr, (1u << 30) - 6) && big.first_block[2] == (1u << 31) - 1);
        const FindMany before = big;
        CHECK(!find_many_append(big, (const int64_t*)base, 8, (f32x4*)base, nullptr, 1) && !memcmp(&big, &before, sizeof big));   // the grid stays below 2^31 blocks
        FindMany huge{};
        CHECK(!find_many_append(huge, (const int64_t*)base, 8, (f32x4*)base, nullptr, 1u << 31) && huge.count == 0);
    }

    // ---- FindNodes: one entry per capture id, free entries first, then the entry used longest ago
    {
        FindNodes* nodes = new FindNodes();   // (on the heap: ASan watches its bounds)
        CHECK(!nodes->get(0) && !nodes->get(7));
        for (unsigned long long id = 1; id <= (unsigned long long)kFindNodes; ++id) {
            FindNode& e = nodes->put(id);
            CHECK(e.capture_id == id && !e.off && !e.node && e.m.count == 0);
            e.node = base + id;
        }
        for (unsigned long long id = 1; id <= (unsigned long long)kFindNodes; ++id) CHECK(nodes->get(id) && nodes->get(id)->node == base + id);
        CHECK(&nodes->put(2) == nodes->get(2) && nodes->get(2)->node == base + 2);   // an entry that exists is kept as it is ...
        (void)nodes->put(1);                                                          // ... and is the newest now
        FindNode& fresh = nodes->put(100);                                            // pushes out id 3, the one used longest ago
        CHECK(fresh.capture_id == 100 && !fresh.node && !nodes->get(3) && nodes->get(1) && nodes->get(2) && nodes->get(4));
        for (int i = 0; i < 1000; ++i) {
            const unsigned long long id = 1 + rnd() % 9;
            FindNode& e = nodes->put(id);
            CHECK(e.capture_id == id && nodes->get(id) == &e);
            int live = 0;
            for (const FindNode& c : nodes->e) live += c.capture_id == id;
            CHECK(live == 1);
        }
        delete nodes;
    }
    printf("find_coalesce_host ok\n");
    return 0;
}
