// mixed_group_test.cpp — the mixed group (members of different dims) through the C-ABI alone: create, layout, one pooled lookup checked against
// sums computed on the host in position order, the argument errors, destroy; then the same through the C++ wrapper meepo::MixedGroup
// (include/meepo_embedding.hpp) with a member wider than 128 floats.  Exit code 0 = all checks passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "meepo_embedding.h"
#include "meepo_embedding.hpp"

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define MEECK(x) do { int rc_ = (x); if (rc_ != MEE_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, mee_last_error()); return 3; } } while (0)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 4; } } while (0)

static uint64_t mix64(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x; }
static float row_value(int64_t key, int j, uint64_t seed) { return (float)(mix64((uint64_t)key ^ mix64(seed + j)) >> 40) * 0x1p-24f - 0.5f; }

// meepo::MixedGroup over two meepo::Table of dims 8 and 256 (a width above 128: the lookup instance with the full-width run-time row shape):
// layout, one pooled lookup (mean) against host sums, bf16 accepted, an error arrives as meepo::Error, the step is refused without max_apply_batch
static int wrapper_checks(hipStream_t st) {
    const uint32_t dims[2] = {256, 8};
    const size_t B = 2, per_table = 24;
    std::vector<int64_t> tkeys(per_table);
    for (size_t i = 0; i < per_table; ++i) tkeys[i] = (int64_t)(5000 + 3 * i);
    int64_t* d_tk;
    HIPCK(hipMalloc(&d_tk, per_table * 8));
    HIPCK(hipMemcpy(d_tk, tkeys.data(), per_table * 8, hipMemcpyHostToDevice));
    meepo::TableOptions o;
    o.capacity = 256; o.max_batch = 256; o.default_value = -1.5f;
    o.dim = dims[0];
    meepo::Table wide(o);
    o.dim = dims[1];
    meepo::Table narrow(o);
    meepo::Table* members[2] = {&wide, &narrow};
    for (int j = 0; j < 2; ++j) {
        std::vector<float> rows(per_table * dims[j]);
        for (size_t i = 0; i < per_table; ++i)
            for (uint32_t e = 0; e < dims[j]; ++e) rows[i * dims[j] + e] = row_value(tkeys[i], (int)e, 20 + j);
        float* d_rows;
        HIPCK(hipMalloc(&d_rows, rows.size() * 4));
        HIPCK(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        members[j]->insert(d_tk, d_rows, per_table, st);
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipFree(d_rows));
    }
    meepo::MixedGroup grp(members, 2);
    CHECK(grp.size() == 2);
    uint64_t offs[2];
    const uint64_t total = grp.layout(B, offs);
    CHECK(offs[1] == 0 && offs[0] == B * 8 && total == B * (8 + 256) && grp.layout(0) == 0);
    // member 0: bags of 3 and 17 keys (one tile; the four tiles together), member 1: an empty bag and one of 2 keys, the second key absent
    std::vector<int64_t> keys;
    std::vector<uint64_t> bo(1, 0);
    const size_t lens[4] = {3, 17, 0, 2};
    for (size_t b = 0; b < 4; ++b) {
        for (size_t q = 0; q < lens[b]; ++q) keys.push_back(tkeys[(5 * b + 7 * q) % per_table]);
        bo.push_back(keys.size());
    }
    keys.back() = 777777;
    const size_t n = keys.size();
    int64_t* d_keys; uint64_t* d_bo; float* d_out; uint8_t* d_found;
    HIPCK(hipMalloc(&d_keys, n * 8)); HIPCK(hipMalloc(&d_bo, bo.size() * 8)); HIPCK(hipMalloc(&d_out, total * 4)); HIPCK(hipMalloc(&d_found, n));
    HIPCK(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(d_bo, bo.data(), bo.size() * 8, hipMemcpyHostToDevice));
    bool threw = false;
    try { grp.find_pooled(d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, nullptr, 7); } catch (const meepo::Error& e) { threw = e.code() == MEE_ERR_INVALID_ARG; }
    CHECK(threw);
    threw = false;
    try { grp.apply_adagrad_pooled(d_keys, d_bo, B, d_out, (const uint32_t*)d_found, nullptr, n, 0.1f); } catch (const meepo::Error& e) { threw = e.code() == MEE_ERR_UNSUPPORTED; }
    CHECK(threw);
    threw = false;   // (a group without a step has no apply to tune)
    try { grp.set_tuning("apply_xcd_split", -1); } catch (const meepo::Error& e) { threw = e.code() == MEE_ERR_UNSUPPORTED; }
    CHECK(threw);
    grp.find_pooled(d_keys, n, d_bo, B, d_out, MEE_DTYPE_BF16, d_found, nullptr, MEE_POOL_SUM, false, st);   // (half the buffer: accepted, result not read)
    grp.find_pooled(d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, nullptr, MEE_POOL_MEAN, false, st);
    std::vector<float> out(total);
    std::vector<uint8_t> found(n);
    HIPCK(hipMemcpyAsync(out.data(), d_out, total * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(found.data(), d_found, n, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (int j = 0; j < 2; ++j)
        for (size_t b = 0; b < B; ++b)
            for (uint32_t e = 0; e < dims[j]; ++e) {
                float s = 0.0f;
                bool first = true;
                const uint64_t lo = bo[j * B + b], hi = bo[j * B + b + 1];
                for (uint64_t i = lo; i < hi; ++i) {
                    const float v = keys[i] == 777777 ? -1.5f : row_value(keys[i], (int)e, 20 + j);
                    s = first ? v : s + v;
                    first = false;
                }
                if (hi > lo) s = s / (float)(hi - lo);
                CHECK(out[offs[j] + b * dims[j] + e] == s);
            }
    for (size_t i = 0; i < n; ++i) CHECK(found[i] == (keys[i] != 777777));
    HIPCK(hipFree(d_keys)); HIPCK(hipFree(d_bo)); HIPCK(hipFree(d_out)); HIPCK(hipFree(d_found)); HIPCK(hipFree(d_tk));
    return 0;
}

int main() {
    const uint32_t T = 3, dims[T] = {64, 8, 64 + 36};   // classes by ascending dim: member 1 (8), member 0 (64), member 2 (100)
    const size_t B = 3, per_table = 40;
    hipStream_t st;
    HIPCK(hipStreamCreate(&st));
    mee_table* t[T];
    std::vector<int64_t> tkeys(per_table);
    for (size_t i = 0; i < per_table; ++i) tkeys[i] = (int64_t)(1000 + i);
    int64_t* d_tk;
    HIPCK(hipMalloc(&d_tk, per_table * 8));
    HIPCK(hipMemcpy(d_tk, tkeys.data(), per_table * 8, hipMemcpyHostToDevice));
    for (uint32_t j = 0; j < T; ++j) {
        mee_config c{};
        c.struct_size = sizeof c; c.device = 0; c.capacity = 256; c.dim = dims[j]; c.max_batch = 256; c.default_value = 0.25f;
        MEECK(mee_table_create(&c, &t[j]));
        std::vector<float> rows(per_table * dims[j]);
        for (size_t i = 0; i < per_table; ++i)
            for (uint32_t e = 0; e < dims[j]; ++e) rows[i * dims[j] + e] = row_value(tkeys[i], (int)e, 10 + j);
        float* d_rows;
        HIPCK(hipMalloc(&d_rows, rows.size() * 4));
        HIPCK(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        MEECK(mee_insert(t[j], d_tk, d_rows, per_table, st));
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipFree(d_rows));
    }
    // argument errors: a message, not a crash
    mee_mixed_group* g = nullptr;
    CHECK(mee_mixed_group_create(nullptr, T, 0, &g) == MEE_ERR_INVALID_ARG && strlen(mee_last_error()) > 0);
    CHECK(mee_mixed_group_create(t, 0, 0, &g) == MEE_ERR_INVALID_ARG);
    CHECK(mee_mixed_group_create(t, T, 0, nullptr) == MEE_ERR_INVALID_ARG);
    CHECK(mee_mixed_group_layout(nullptr, B, nullptr, nullptr) == MEE_ERR_INVALID_ARG);
    MEECK(mee_mixed_group_create(t, T, 0, &g));
    uint64_t offs[T], total = 0;
    MEECK(mee_mixed_group_layout(g, B, offs, &total));
    CHECK(offs[1] == 0 && offs[0] == B * 8 && offs[2] == B * (8 + 64) && total == B * (8 + 64 + 100));

    // bags: member j's bag b holds b + 2 * j keys (bag 0 of member 0 is empty); one absent key ends member 2's last bag
    std::vector<int64_t> keys;
    std::vector<uint64_t> bo(1, 0);
    for (uint32_t j = 0; j < T; ++j)
        for (size_t b = 0; b < B; ++b) {
            for (size_t q = 0; q < b + 2 * j; ++q) keys.push_back(tkeys[(7 * j + 3 * b + q) % per_table]);
            if (j == 2 && b == B - 1) keys.push_back(555555);
            bo.push_back(keys.size());
        }
    const size_t n = keys.size();
    int64_t* d_keys; uint64_t* d_bo; float* d_out; uint8_t* d_found;
    HIPCK(hipMalloc(&d_keys, n * 8)); HIPCK(hipMalloc(&d_bo, bo.size() * 8)); HIPCK(hipMalloc(&d_out, total * 4)); HIPCK(hipMalloc(&d_found, n));
    HIPCK(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(d_bo, bo.data(), bo.size() * 8, hipMemcpyHostToDevice));
    CHECK(mee_mixed_group_find_pooled(g, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, nullptr, 7, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_mixed_group_find_pooled(g, d_keys, n, d_bo, B, d_out, 9, d_found, nullptr, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_mixed_group_find_pooled(g, d_keys, n, nullptr, B, d_out, MEE_DTYPE_F32, d_found, nullptr, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_mixed_group_find_pooled(g, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, nullptr, nullptr, MEE_POOL_SUM, 1, st) == MEE_ERR_INVALID_ARG);
    // no step without max_apply_batch
    CHECK(mee_mixed_group_apply_adagrad_pooled(g, d_keys, d_bo, B, d_out, (const uint32_t*)d_found, nullptr, n, 0.1f, 1e-10f, st) == MEE_ERR_UNSUPPORTED);
    MEECK(mee_mixed_group_find_pooled(g, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, nullptr, MEE_POOL_SUM, 0, st));
    std::vector<float> out(total);
    std::vector<uint8_t> found(n);
    HIPCK(hipMemcpyAsync(out.data(), d_out, total * 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipMemcpyAsync(found.data(), d_found, n, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    for (uint32_t j = 0; j < T; ++j)
        for (size_t b = 0; b < B; ++b)
            for (uint32_t e = 0; e < dims[j]; ++e) {
                float s = 0.0f;
                bool first = true;
                for (uint64_t i = bo[j * B + b]; i < bo[j * B + b + 1]; ++i) {
                    const float v = keys[i] == 555555 ? 0.25f : row_value(keys[i], (int)e, 10 + j);
                    s = first ? v : s + v;
                    first = false;
                }
                CHECK(out[offs[j] + b * dims[j] + e] == s);
            }
    for (size_t i = 0; i < n; ++i) CHECK(found[i] == (keys[i] != 555555));
    MEECK(mee_mixed_group_destroy(g));
    MEECK(mee_mixed_group_destroy(nullptr));
    for (uint32_t j = 0; j < T; ++j) MEECK(mee_table_destroy(t[j]));
    try {
        if (int rc = wrapper_checks(st)) return rc;
    } catch (const std::exception& e) {
        fprintf(stderr, "meepo::MixedGroup: %s\n", e.what());
        return 5;
    }
    printf("mixed_group_test ok: %u tables of dims 64/8/100, %zu bags each, %zu keys pooled in one launch through the C-ABI; meepo::MixedGroup over dims 256/8\n", T, B, n);
    return 0;
}
