// meepo_find_coalesce.h — the HOST bookkeeping of captured finds that share a kernel node (meepo_find.hip: find_captured).  Plain C++ without a
// HIP type in it, so that tests/cabi/find_coalesce_host.cpp drives it under ASan / UBSan: the request descriptor of find_many_kernel, the test
// that a further request may join the requests of a node, the descriptor's rebuild, and the small table of recorded nodes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mee {

typedef float f32x4 __attribute__((ext_vector_type(4)));   // (as in meepo_device.h)

// Several lookup requests of one table in ONE launch (mee_find_many; captured finds): the request descriptors travel in the kernel argument; a block
// finds its request by its index (<= kMaxFindRequests entries).
constexpr int kMaxFindRequests = 16;
struct FindMany {
    const int64_t* keys[kMaxFindRequests];
    f32x4* out[kMaxFindRequests];
    uint8_t* found[kMaxFindRequests];
    uint64_t n[kMaxFindRequests];
    uint32_t first_block[kMaxFindRequests + 1];   // request q owns blocks first_block[q] .. first_block[q + 1] - 1; [count] = the grid; behind it 0xFFFFFFFF
    uint32_t count;
};

inline bool bytes_overlap(const void* a, uint64_t a_bytes, const void* b, uint64_t b_bytes) {
    const uint64_t pa = (uint64_t)(uintptr_t)a, pb = (uint64_t)(uintptr_t)b;
    return a && b && a_bytes && b_bytes && pa < pb + b_bytes && pb < pa + a_bytes;
}

// One more request beside the requests of `m`, all in one kernel: true when nothing it writes (out: row_bytes per key, found: one byte per key, nullable)
// touches what they write or read, and nothing it reads (keys) touches what they write.  Chained launches that share a buffer have a defined
// winner; requests inside one kernel do not.
inline bool find_request_disjoint(const FindMany& m, uint64_t row_bytes, const int64_t* keys, uint64_t n, const void* out, const uint8_t* found) {
    for (uint32_t q = 0; q < m.count; ++q) {
        const uint64_t qn = m.n[q];
        const void* w[2] = {out, found};
        const uint64_t wb[2] = {n * row_bytes, n};
        for (int i = 0; i < 2; ++i) {
            if (bytes_overlap(w[i], wb[i], m.out[q], qn * row_bytes) || bytes_overlap(w[i], wb[i], m.found[q], qn) || bytes_overlap(w[i], wb[i], m.keys[q], qn * 8)) return false;
        }
        if (bytes_overlap(keys, n * 8, m.out[q], qn * row_bytes) || bytes_overlap(keys, n * 8, m.found[q], qn)) return false;
    }
    return true;
}

// `m` with one more request of `blocks` blocks behind the others (first_block[] and with it the grid, first_block[count], follow); false — and `m` as it
// was — when the descriptor is full, the request is empty or the grid would reach 2^31 blocks
inline bool find_many_append(FindMany& m, const int64_t* keys, uint64_t n, f32x4* out, uint8_t* found, uint32_t blocks) {
    if (m.count >= (uint32_t)kMaxFindRequests || n == 0 || blocks == 0) return false;
    const uint64_t total = (uint64_t)(m.count ? m.first_block[m.count] : 0u) + blocks;
    if (total >= (1ull << 31)) return false;
    const uint32_t q = m.count;
    if (q == 0) m.first_block[0] = 0;
    m.keys[q] = keys; m.out[q] = out; m.found[q] = found; m.n[q] = n;
    m.first_block[q + 1] = (uint32_t)total;
    for (uint32_t i = q + 2; i <= (uint32_t)kMaxFindRequests; ++i) m.first_block[i] = 0xFFFFFFFFu;   // no block reaches the entries behind the grid size (find_many_kernel counts)
    m.count = q + 1;
    return true;
}

// The latest find node of a stream capture: what a further find has to agree with to join it.  `graph`, `node` and `func` are the HIP handles and the
// kernel instance (which says row shape, keys in flight and policy bits), kept as plain pointers.
struct FindNode {
    unsigned long long capture_id;   // 0: the entry is free
    bool off;                        // coalescing was switched off for this capture (a HIP call failed): every find gets a launch of its own
    void *graph, *node;
    const void* func;
    const void* table;
    const int64_t* tkeys;
    const void* values;
    uint64_t nb;
    uint32_t defv_bits, dim4, block;
    FindMany m;
    uint64_t age;
};

// A few captures may be open at once (one per capturing thread); an id never comes back, so an entry that is pushed out is merely a capture whose
// next find starts a node of its own.  Not thread-safe: the caller holds the library's lock.
constexpr int kFindNodes = 4;
struct FindNodes {
    FindNode e[kFindNodes] = {};
    uint64_t clock = 0;
    FindNode* get(unsigned long long capture_id) {
        for (FindNode& r : e) if (r.capture_id == capture_id && capture_id) return &r;
        return nullptr;
    }
    // the entry of `capture_id`, made from the oldest one when it has none
    FindNode& put(unsigned long long capture_id) {
        FindNode* r = get(capture_id);
        if (!r) {
            r = &e[0];
            for (FindNode& c : e) if (c.capture_id == 0 || (r->capture_id != 0 && c.age < r->age)) r = &c;
            *r = FindNode{};
            r->capture_id = capture_id;
        }
        r->age = ++clock;
        return *r;
    }
};

}  // namespace mee
