// tiered_bags_test.cpp — the pooled lookup of a hot/cold pair through the C-ABI alone (mee_find_pooled_tiered): a hot table in HBM and a
// cold table whose rows live in pinned host memory, keys alternating between them inside every bag; sums and means checked against sums
// computed on the host in position order, the found mask, the hit counters the count flags feed, the argument errors.  Exit code 0 = all
// checks passed.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "meepo_embedding.h"

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)
#define MEECK(x) do { int rc_ = (x); if (rc_ != MEE_OK) { fprintf(stderr, "%s -> %d: %s\n", #x, rc_, mee_last_error()); return 3; } } while (0)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 4; } } while (0)

static uint64_t mix64(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x; }
static float row_value(int64_t key, int j) { return (float)(mix64((uint64_t)key ^ mix64(77 + j)) >> 40) * 0x1p-24f - 0.5f; }

static const uint32_t kDim = 64;
static const int64_t kAbsent = 999999;
static const float kHotDefault = 0.25f, kColdDefault = -3.0f;   // an absent key reads the HOT table's default row

static int make_table(uint32_t value_memory, uint32_t dim, uint32_t flags, float defv, mee_table** t) {
    mee_config c{};
    c.struct_size = sizeof c; c.device = 0; c.capacity = 512; c.dim = dim; c.max_batch = 512; c.default_value = defv;
    c.value_memory = value_memory; c.flags = flags;
    MEECK(mee_table_create(&c, t));
    return 0;
}

int main() {
    hipStream_t st;
    HIPCK(hipStreamCreate(&st));
    mee_table *hot, *cold, *plain, *wide;
    if (int rc = make_table(MEE_MEM_HBM, kDim, MEE_FLAG_TRACK_HITS, kHotDefault, &hot)) return rc;
    if (int rc = make_table(MEE_MEM_HOST_PINNED, kDim, MEE_FLAG_TRACK_HITS, kColdDefault, &cold)) return rc;
    if (int rc = make_table(MEE_MEM_HBM, kDim, 0, 0.f, &plain)) return rc;      // no hit counters
    if (int rc = make_table(MEE_MEM_HBM, 2 * kDim, 0, 0.f, &wide)) return rc;   // another dim

    // 60 stored keys: even index -> hot, odd index -> cold
    const size_t per_tier = 30;
    std::vector<int64_t> hk(per_tier), ck(per_tier);
    for (size_t i = 0; i < per_tier; ++i) { hk[i] = (int64_t)(1000 + 2 * i); ck[i] = (int64_t)(1001 + 2 * i); }
    for (int tier = 0; tier < 2; ++tier) {
        const std::vector<int64_t>& k = tier ? ck : hk;
        std::vector<float> rows(per_tier * kDim);
        for (size_t i = 0; i < per_tier; ++i)
            for (uint32_t e = 0; e < kDim; ++e) rows[i * kDim + e] = row_value(k[i], (int)e);
        int64_t* d_k; float* d_rows;
        HIPCK(hipMalloc(&d_k, per_tier * 8)); HIPCK(hipMalloc(&d_rows, rows.size() * 4));
        HIPCK(hipMemcpy(d_k, k.data(), per_tier * 8, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(d_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
        MEECK(mee_insert(tier ? cold : hot, d_k, d_rows, per_tier, st));
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipFree(d_k)); HIPCK(hipFree(d_rows));
    }

    // bags of 3, 17 (the four tiles together), 0, 2 and 9 keys: consecutive keys, so hot and cold alternate by position; one absent key,
    // one reserved key, and key 1001 (cold) three times in all
    const size_t lens[5] = {3, 17, 0, 2, 9};
    std::vector<int64_t> keys;
    std::vector<uint64_t> bo(1, 0);
    for (size_t b = 0; b < 5; ++b) {
        for (size_t q = 0; q < lens[b]; ++q) keys.push_back((int64_t)(1000 + (11 * b + q) % (2 * per_tier)));
        bo.push_back(keys.size());
    }
    keys[5] = kAbsent; keys[9] = MEE_EMPTY_KEY; keys[12] = 1001; keys[21] = 1001;
    const size_t n = keys.size(), B = 5;
    int64_t* d_keys; uint64_t* d_bo; float* d_out; uint8_t* d_found;
    HIPCK(hipMalloc(&d_keys, n * 8)); HIPCK(hipMalloc(&d_bo, bo.size() * 8)); HIPCK(hipMalloc(&d_out, B * kDim * 4)); HIPCK(hipMalloc(&d_found, n));
    HIPCK(hipMemcpy(d_keys, keys.data(), n * 8, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(d_bo, bo.data(), bo.size() * 8, hipMemcpyHostToDevice));

    // argument errors: a message, not a crash
    CHECK(mee_find_pooled_tiered(nullptr, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG && strlen(mee_last_error()) > 0);
    CHECK(mee_find_pooled_tiered(hot, nullptr, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, hot, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, wide, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 4, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, 7, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, d_out, 9, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, (char*)d_out + 4, MEE_DTYPE_BF16, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, cold, d_keys, n, nullptr, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, 0, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(hot, plain, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, MEE_TIER_COUNT_COLD, st) == MEE_ERR_INVALID_ARG);
    CHECK(mee_find_pooled_tiered(plain, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, MEE_TIER_COUNT_HOT, st) == MEE_ERR_INVALID_ARG);
    MEECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, 0, nullptr, MEE_DTYPE_F32, nullptr, MEE_POOL_SUM, 0, st));   // no bags: nothing to write

    std::vector<float> out(B * kDim);
    std::vector<uint8_t> found(n);
    for (int mode = 0; mode < 2; ++mode) {   // sum counts nothing, mean counts both tiers
        HIPCK(hipMemsetAsync(d_found, 7, n, st));
        MEECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_F32, d_found, mode ? MEE_POOL_MEAN : MEE_POOL_SUM,
                                     mode ? (MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT) : 0, st));
        HIPCK(hipMemcpyAsync(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(found.data(), d_found, n, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        for (size_t b = 0; b < B; ++b)
            for (uint32_t e = 0; e < kDim; ++e) {
                float s = 0.0f;
                bool first = true;
                for (uint64_t i = bo[b]; i < bo[b + 1]; ++i) {
                    const bool stored = keys[i] >= 1000 && keys[i] < (int64_t)(1000 + 2 * per_tier);
                    const float v = stored ? row_value(keys[i], (int)e) : kHotDefault;
                    s = first ? v : s + v;
                    first = false;
                }
                if (mode && bo[b + 1] > bo[b]) s = s / (float)(bo[b + 1] - bo[b]);
                CHECK(out[b * kDim + e] == s);
            }
        for (size_t i = 0; i < n; ++i) CHECK(found[i] == (keys[i] >= 1000 && keys[i] < (int64_t)(1000 + 2 * per_tier)));
    }
    // d_found is nullable (not written); bf16 rows are accepted
    MEECK(mee_find_pooled_tiered(hot, cold, d_keys, n, d_bo, B, d_out, MEE_DTYPE_BF16, nullptr, MEE_POOL_SUM, 0, st));
    HIPCK(hipStreamSynchronize(st));

    // the one counted call: every stored position counted once in its own tier; key 1001 (cold) was looked up three times
    int64_t* d_scan;
    HIPCK(hipMalloc(&d_scan, 512 * 8));
    size_t hot_hit = 0, cold_hit = 0, thrice = 0;
    MEECK(mee_hits_scan(hot, 1, 0xFFFFFFFFu, 0, d_scan, 512, &hot_hit, st));
    MEECK(mee_hits_scan(cold, 1, 0xFFFFFFFFu, 0, d_scan, 512, &cold_hit, st));
    MEECK(mee_hits_scan(cold, 3, 0xFFFFFFFFu, 0, d_scan, 512, &thrice, st));
    int64_t which = 0;
    HIPCK(hipMemcpy(&which, d_scan, 8, hipMemcpyDeviceToHost));
    std::vector<bool> seen_hot(2 * per_tier, false), seen_cold(2 * per_tier, false);
    size_t want_hot = 0, want_cold = 0;
    for (size_t i = 0; i < n; ++i) {
        if (keys[i] < 1000 || keys[i] >= (int64_t)(1000 + 2 * per_tier)) continue;
        std::vector<bool>& seen = (keys[i] & 1) ? seen_cold : seen_hot;
        size_t& want = (keys[i] & 1) ? want_cold : want_hot;
        if (!seen[keys[i] - 1000]) { seen[keys[i] - 1000] = true; ++want; }
    }
    CHECK(hot_hit == want_hot && cold_hit == want_cold && want_hot > 0 && want_cold > 0);
    CHECK(thrice == 1 && which == 1001);

    HIPCK(hipFree(d_scan)); HIPCK(hipFree(d_keys)); HIPCK(hipFree(d_bo)); HIPCK(hipFree(d_out)); HIPCK(hipFree(d_found));
    MEECK(mee_table_destroy(hot)); MEECK(mee_table_destroy(cold)); MEECK(mee_table_destroy(plain)); MEECK(mee_table_destroy(wide));
    printf("tiered_bags_test ok: %zu keys in %zu bags pooled over a hot (HBM) and a cold (pinned host) table in one launch through the C-ABI\n", n, B);
    return 0;
}
