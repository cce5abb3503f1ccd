// group_admit_test.cpp — admission over a table group through the C-ABI and the C++ wrapper (include/meepo_embedding.hpp) alone: create, two admitting
// calls with a host-side check of found, size and the rows of one small batch, per-member thresholds, the grouped decay, the argument errors, destroy.
// Exit code 0 = all checks passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "meepo_embedding.h"
#include "meepo_embedding.hpp"

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 4; } } while (0)

constexpr uint32_t kDim = 8;
constexpr size_t kMaxN = 8;

struct Batch {   // device buffers of one small jagged batch and their host copies
    int64_t* d_keys = nullptr;
    uint64_t* d_off = nullptr;
    float* d_out = nullptr;
    uint8_t* d_found = nullptr;
    uint32_t* d_thr = nullptr;
    std::vector<float> out;
    std::vector<uint8_t> found;
    size_t n = 0;
    int alloc() {
        HIPCK(hipMalloc(&d_keys, kMaxN * 8)); HIPCK(hipMalloc(&d_off, 3 * 8)); HIPCK(hipMalloc(&d_out, kMaxN * kDim * 4)); HIPCK(hipMalloc(&d_found, kMaxN));
        HIPCK(hipMalloc(&d_thr, 2 * 4));
        return 0;
    }
    int set(const std::vector<int64_t>& keys, const std::vector<uint64_t>& off) {
        n = keys.size();
        HIPCK(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_off, off.data(), 3 * 8, hipMemcpyHostToDevice));
        return 0;
    }
    int fetch(hipStream_t st) {
        out.assign(n * kDim, 0.f); found.assign(n, 9);
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipMemcpy(out.data(), d_out, n * kDim * 4, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(found.data(), d_found, n, hipMemcpyDeviceToHost));
        return 0;
    }
    bool row_is(size_t i, float v) const { for (uint32_t e = 0; e < kDim; ++e) if (out[i * kDim + e] != v) return false; return true; }
    bool rows_equal(size_t i, size_t j) const { return memcmp(&out[i * kDim], &out[j * kDim], kDim * 4) == 0; }
};

static int run() {
    hipStream_t st;
    HIPCK(hipStreamCreate(&st));
    meepo::TableOptions o;
    o.capacity = 256; o.dim = kDim; o.max_batch = 64; o.optimizer = MEE_OPT_ADAGRAD; o.initializer = MEE_INIT_UNIFORM; o.init_scale = 0.1f; o.admission = true;
    o.init_seed = 1; o.default_value = -1.f;
    meepo::Table t0(o);
    o.init_seed = 2; o.default_value = -2.f;
    meepo::Table t1(o);
    meepo::Table* members[2] = {&t0, &t1};
    meepo::Group grp(members, 2, /*max_apply_batch=*/4);
    Batch b;
    if (int rc = b.alloc()) return rc;

    // call 1, min_count 2: member 0 sees key 10 twice (created in this call) and key 11 once; member 1 sees 10 and 12 once each
    if (int rc = b.set({10, 11, 10, 10, 12}, {0, 3, 5})) return rc;
    grp.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 2, nullptr, st);
    if (int rc = b.fetch(st)) return rc;
    for (size_t i = 0; i < b.n; ++i) CHECK(b.found[i] == 0);
    CHECK(t0.size(st) == 1 && t1.size(st) == 0);
    CHECK(!b.row_is(0, -1.f) && b.rows_equal(0, 2));        // every occurrence of the created key returns its initial row
    CHECK(b.row_is(1, -1.f) && b.row_is(3, -2.f) && b.row_is(4, -2.f));   // not admitted: the member's default row
    const std::vector<float> first = b.out;
    // call 2: the second sighting admits the rest; found = present before
    grp.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 2, nullptr, st);
    if (int rc = b.fetch(st)) return rc;
    CHECK(b.found[0] == 1 && b.found[1] == 0 && b.found[2] == 1 && b.found[3] == 0 && b.found[4] == 0);
    CHECK(t0.size(st) == 2 && t1.size(st) == 2);
    CHECK(memcmp(&b.out[0], &first[0], kDim * 4) == 0 && b.rows_equal(0, 2));   // the stored row is the row call 1 returned
    CHECK(!b.row_is(1, -1.f) && !b.row_is(3, -2.f) && !b.row_is(4, -2.f));
    CHECK(!b.rows_equal(0, 3));                                                // key 10 of member 1 came from member 1's initializer
    {   // ... and a plain find of member 1 returns what the admitting call returned
        std::vector<float> rows(2 * kDim);
        t1.find(b.d_keys + 3, 2, b.d_out, b.d_found, st);
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipMemcpy(rows.data(), b.d_out, rows.size() * 4, hipMemcpyDeviceToHost));
        CHECK(memcmp(rows.data(), &b.out[3 * kDim], rows.size() * 4) == 0);
    }

    // per-member thresholds {3, 1}: member 0 only counts key 20, member 1 creates key 21 at first sight
    const uint32_t thr[2] = {3, 1};
    HIPCK(hipMemcpy(b.d_thr, thr, sizeof thr, hipMemcpyHostToDevice));
    if (int rc = b.set({20, 21}, {0, 1, 2})) return rc;
    grp.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 99, b.d_thr, st);
    if (int rc = b.fetch(st)) return rc;
    CHECK(b.row_is(0, -1.f) && !b.row_is(1, -2.f) && t0.size(st) == 2 && t1.size(st) == 3);
    // the decay: shift >= 32 zeroes every member's sketch, so key 20's next sighting is a first one again (without the decay it would be admitted)
    grp.admission_decay(32, st);
    grp.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 2, nullptr, st);
    if (int rc = b.fetch(st)) return rc;
    CHECK(b.row_is(0, -1.f) && b.found[0] == 0 && b.found[1] == 1 && t0.size(st) == 2);
    grp.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, nullptr, 2, nullptr, st);   // no found buffer: n <= max_apply_batch
    if (int rc = b.fetch(st)) return rc;
    CHECK(!b.row_is(0, -1.f) && t0.size(st) == 3);
    CHECK(t0.status(st) == 0 && t1.status(st) == 0);

    // the argument errors: nothing is launched or written
    mee_group* raw = nullptr;
    mee_table* handles[2] = {t0.handle(), t1.handle()};
    CHECK(mee_group_create(handles, 2, 4, &raw) == MEE_OK);
    if (int rc = b.set({30, 31, 32, 33, 34}, {0, 2, 5})) return rc;
    CHECK(mee_group_find_or_insert_admit(nullptr, b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 1, nullptr, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_find_or_insert_admit(raw, b.d_keys, b.d_off, b.n, nullptr, MEE_DTYPE_F32, b.d_found, 1, nullptr, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_find_or_insert_admit(raw, nullptr, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 1, nullptr, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_find_or_insert_admit(raw, b.d_keys, nullptr, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 1, nullptr, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_find_or_insert_admit(raw, b.d_keys, b.d_off, b.n, b.d_out, 7, b.d_found, 1, nullptr, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_find_or_insert_admit(raw, b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, nullptr, 1, nullptr, st) == MEE_ERR_BATCH_TOO_LARGE);   // 5 > 4
    CHECK(mee_group_find_or_insert_admit(raw, nullptr, b.d_off, 0, nullptr, MEE_DTYPE_F32, nullptr, 1, nullptr, st) == MEE_OK);                      // n == 0
    CHECK(mee_group_admission_decay(nullptr, 1, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_group_destroy(raw) == MEE_OK);
    {   // a member created without MEE_FLAG_ADMISSION: UNSUPPORTED, the message names it
        o.admission = false;
        meepo::Table plain(o);
        meepo::Table* mixed[2] = {&t0, &plain};
        meepo::Group g2(mixed, 2);
        bool threw = false;
        try { g2.find_or_insert_admit(b.d_keys, b.d_off, b.n, b.d_out, MEE_DTYPE_F32, b.d_found, 1, nullptr, st); }
        catch (const meepo::Error& e) { threw = e.code() == MEE_ERR_UNSUPPORTED && strstr(e.what(), "member 1") != nullptr; }
        CHECK(threw);
        threw = false;
        try { g2.admission_decay(1, st); } catch (const meepo::Error& e) { threw = e.code() == MEE_ERR_UNSUPPORTED; }
        CHECK(threw);
        CHECK(plain.size(st) == 0);
    }
    CHECK(t0.size(st) == 3 && t1.size(st) == 3);   // the refused calls created nothing
    HIPCK(hipFree(b.d_keys)); HIPCK(hipFree(b.d_off)); HIPCK(hipFree(b.d_out)); HIPCK(hipFree(b.d_found)); HIPCK(hipFree(b.d_thr));
    HIPCK(hipStreamDestroy(st));
    return 0;
}

int main() {
    int rc;
    try { rc = run(); } catch (const meepo::Error& e) { fprintf(stderr, "meepo::Error %d: %s\n", e.code(), e.what()); return 3; }
    if (rc == 0) printf("group_admit_test ok\n");
    return rc;
}
