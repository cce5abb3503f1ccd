// host_transcript.cpp — TEST INFRASTRUCTURE: a record of what the HOST layer of the pooled lookups and of the optimizer steps decides.
//
// Linked against the host-only library of build_sanitized.sh (launches do nothing; hip_host_stub.cpp logs them), it walks a table of cases over every
// entry point of the two families and prints one line per case: the name, the return code, mee_last_error() on failure, and behind " | " each kernel the
// call launched — instance (template arguments), grid.x, block.x.  tests/test_host_transcript.py compares the output with tests/golden/host_transcript.txt, which was
// written by this program linked against the sources as they were BEFORE the host layer was consolidated: a change of that layer that moves a refusal,
// a message, a kernel instance or a grid shows up as a diff.  Kernels do not run: the buffers only have to exist, no value means anything.
// usage: host_transcript LOGFILE   (LOGFILE: a scratch file for the stub's launch log)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "meepo_embedding.h"

static const char* g_log;

// a logged line without the kernel's parameter list: "void mee::kern<3, true>(int*, int) grid 7 block 256" -> "mee::kern<3, true> grid 7 block 256"
static std::string shorten(const std::string& line) {
    int depth = 0;
    size_t open = std::string::npos;
    for (size_t i = 0; i < line.size(); ++i) {
        if (line[i] == '<') ++depth;
        else if (line[i] == '>') --depth;
        else if (line[i] == '(' && depth == 0) { open = i; break; }
    }
    const size_t tail = line.rfind(" grid ");
    if (open == std::string::npos || tail == std::string::npos) return line;
    std::string head = line.substr(0, open);
    if (head.rfind("void ", 0) == 0) head = head.substr(5);
    return head + line.substr(tail);
}

static void report(const char* name, int rc) {
    if (rc == MEE_OK) printf("%s: 0", name);
    else printf("%s: %d %s", name, rc, mee_last_error());
    if (FILE* f = fopen(g_log, "r")) {
        char buf[8192];
        while (fgets(buf, sizeof buf, f)) {
            std::string s(buf);
            while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
            printf(" | %s", shorten(s).c_str());
        }
        fclose(f);
    }
    printf("\n");
}
static void clear_log() { if (FILE* f = fopen(g_log, "w")) fclose(f); }   // (what building the fixtures launched is not part of a case)
#define CASE(name, call) do { clear_log(); const int rc_ = (call); report(name, rc_); } while (0)
#define MUST(call) do { if ((call) != MEE_OK) { fprintf(stderr, "setup failed: %s: %s\n", #call, mee_last_error()); exit(2); } } while (0)

static mee_table* table(uint32_t dim, uint32_t optimizer, uint32_t flags = 0, uint32_t memory = MEE_MEM_HBM) {
    mee_config c{};
    c.struct_size = sizeof c; c.capacity = 64; c.dim = dim; c.optimizer = optimizer; c.max_batch = 64; c.initial_accumulator = 0.1f;
    c.value_memory = memory; c.flags = flags;
    mee_table* t = nullptr;
    MUST(mee_table_create(&c, &t));
    return t;
}
static mee_group* group(std::vector<mee_table*> members, uint64_t max_apply_batch = 0) {
    mee_group* g = nullptr;
    MUST(mee_group_create(members.data(), (uint32_t)members.size(), max_apply_batch, &g));
    return g;
}
static mee_mixed_group* mixed(std::vector<mee_table*> members, uint64_t max_apply_batch = 0) {
    mee_mixed_group* g = nullptr;
    MUST(mee_mixed_group_create(members.data(), (uint32_t)members.size(), max_apply_batch, &g));
    return g;
}

// the buffers every case shares (nothing reads or writes them: kernels do not run)
alignas(64) static char out_buf[1 << 20];
static int64_t keys[128], located[128], slots[128];
static uint64_t offsets[256], member_bags[8];
static float weights[128], grads[64 * 128 * 4], wgrads[128];
static uint8_t found[128];
static uint32_t index32[128];
static void* const out = out_buf;
static float* const outf = (float*)out_buf;
static void* const odd = out_buf + 4;   // misaligned for a bf16 (8-byte) and a keyed fp32 (16-byte) output
static const int SUM = MEE_POOL_SUM, MEAN = MEE_POOL_MEAN, F32 = MEE_DTYPE_F32, BF16 = MEE_DTYPE_BF16;
static const size_t kShort = 8, kLong = 48, kBags = 4;   // an average bag of 2 keys and of 12: the two launch shapes

static std::string nm(const char* a, const std::string& b) { return std::string(a) + " " + b; }

// ---- pooled lookups ---------------------------------------------------------------------------------------------------------------------------
static void pooled_tables() {
    mee_table *t64 = table(64, MEE_OPT_NONE), *t128 = table(128, MEE_OPT_NONE), *t24 = table(24, MEE_OPT_NONE);
    mee_table *b64 = table(64, MEE_OPT_NONE, MEE_FLAG_BF16_ROWS), *b24 = table(24, MEE_OPT_NONE, MEE_FLAG_BF16_ROWS), *i64 = table(64, MEE_OPT_NONE, MEE_FLAG_INT8_ROWS);
    struct { const char* n; mee_table* t; } shapes[] = {{"dim64", t64}, {"dim128", t128}, {"dim24", t24}, {"bf16rows64", b64}, {"bf16rows24", b24}};
    for (auto& s : shapes)
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_find_pooled", std::string(s.n) + (n == kShort ? " short" : " long")).c_str(), mee_find_pooled(s.t, keys, n, offsets, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled mean no-found", mee_find_pooled(t64, keys, kShort, offsets, kBags, outf, nullptr, MEAN, nullptr));
    CASE("mee_find_pooled n_bags=0", mee_find_pooled(t64, nullptr, 0, nullptr, 0, nullptr, nullptr, SUM, nullptr));
    CASE("mee_find_pooled n=0", mee_find_pooled(t64, nullptr, 0, offsets, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled null table", mee_find_pooled(nullptr, keys, kShort, offsets, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled null keys", mee_find_pooled(t64, nullptr, kShort, offsets, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled null offsets", mee_find_pooled(t64, keys, kShort, nullptr, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled null out", mee_find_pooled(t64, keys, kShort, offsets, kBags, nullptr, found, SUM, nullptr));
    CASE("mee_find_pooled bad mode", mee_find_pooled(t64, keys, kShort, offsets, kBags, outf, found, 7, nullptr));
    CASE("mee_find_pooled int8 rows", mee_find_pooled(i64, keys, kShort, offsets, kBags, outf, found, SUM, nullptr));
    CASE("mee_find_pooled int8 rows + bad mode", mee_find_pooled(i64, keys, kShort, offsets, kBags, outf, found, 7, nullptr));
    CASE("mee_find_pooled null out + bad mode", mee_find_pooled(t64, keys, kShort, offsets, kBags, nullptr, found, 7, nullptr));

    for (auto& s : shapes) {
        if (s.t == b24) continue;
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_find_pooled_weighted", std::string(s.n) + (n == kShort ? " short" : " long located")).c_str(),
                 mee_find_pooled_weighted(s.t, keys, n, offsets, kBags, weights, outf, found, n == kShort ? nullptr : located, nullptr));
    }
    CASE("mee_find_pooled_weighted n=0 null weights", mee_find_pooled_weighted(t64, nullptr, 0, offsets, kBags, nullptr, outf, found, located, nullptr));
    CASE("mee_find_pooled_weighted n_bags=0", mee_find_pooled_weighted(t64, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    CASE("mee_find_pooled_weighted null table", mee_find_pooled_weighted(nullptr, keys, kShort, offsets, kBags, weights, outf, found, nullptr, nullptr));
    CASE("mee_find_pooled_weighted null weights", mee_find_pooled_weighted(t64, keys, kShort, offsets, kBags, nullptr, outf, found, nullptr, nullptr));
    CASE("mee_find_pooled_weighted null out", mee_find_pooled_weighted(t64, keys, kShort, offsets, kBags, weights, nullptr, found, nullptr, nullptr));
    CASE("mee_find_pooled_weighted int8 rows + null weights", mee_find_pooled_weighted(i64, keys, kShort, offsets, kBags, nullptr, outf, found, nullptr, nullptr));

    for (uint32_t dt : {F32, BF16}) {
        const std::string d = dt == F32 ? "f32" : "bf16";
        for (auto& s : shapes) CASE(nm("mee_find_pooled_as", d + " " + s.n + " short").c_str(), mee_find_pooled_as(s.t, keys, kShort, offsets, kBags, nullptr, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_find_pooled_as", d + " dim64 long mean").c_str(), mee_find_pooled_as(t64, keys, kLong, offsets, kBags, nullptr, out, dt, found, nullptr, MEAN, nullptr));
        CASE(nm("mee_find_pooled_as", d + " bf16rows64 long").c_str(), mee_find_pooled_as(b64, keys, kLong, offsets, kBags, nullptr, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_find_pooled_as", d + " weighted dim64 short").c_str(), mee_find_pooled_as(t64, keys, kShort, offsets, kBags, weights, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_find_pooled_as", d + " weighted located dim128 long").c_str(), mee_find_pooled_as(t128, keys, kLong, offsets, kBags, weights, out, dt, found, located, SUM, nullptr));
        CASE(nm("mee_find_pooled_as", d + " weighted dim24 long").c_str(), mee_find_pooled_as(t24, keys, kLong, offsets, kBags, weights, out, dt, nullptr, nullptr, SUM, nullptr));
    }
    CASE("mee_find_pooled_as n_bags=0", mee_find_pooled_as(t64, nullptr, 0, nullptr, 0, nullptr, nullptr, F32, nullptr, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as null table", mee_find_pooled_as(nullptr, keys, kShort, offsets, kBags, nullptr, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as null keys", mee_find_pooled_as(t64, nullptr, kShort, offsets, kBags, nullptr, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as null out", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, nullptr, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as bad dtype", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, 9, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as int8 dtype", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, MEE_DTYPE_INT8, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as misaligned bf16", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, odd, BF16, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as bad mode", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, F32, found, nullptr, -1, nullptr));
    CASE("mee_find_pooled_as weighted mean", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, weights, out, F32, found, nullptr, MEAN, nullptr));
    CASE("mee_find_pooled_as located without weights", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, F32, found, located, SUM, nullptr));
    CASE("mee_find_pooled_as weighted bf16 rows", mee_find_pooled_as(b64, keys, kShort, offsets, kBags, weights, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as int8 rows", mee_find_pooled_as(i64, keys, kShort, offsets, kBags, nullptr, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as int8 rows + null out", mee_find_pooled_as(i64, keys, kShort, offsets, kBags, nullptr, nullptr, F32, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as null out + bad dtype", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, nullptr, 9, found, nullptr, SUM, nullptr));
    CASE("mee_find_pooled_as bad dtype + bad mode", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, 9, found, nullptr, 7, nullptr));
    CASE("mee_find_pooled_as bad mode + located without weights", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, nullptr, out, F32, found, located, 7, nullptr));
    CASE("mee_find_pooled_as weighted mean + misaligned bf16", mee_find_pooled_as(t64, keys, kShort, offsets, kBags, weights, odd, BF16, found, nullptr, MEAN, nullptr));

    // the hot/cold pair
    const uint32_t HITS = MEE_FLAG_TRACK_HITS;
    mee_table *h64 = table(64, MEE_OPT_NONE, HITS), *c64 = table(64, MEE_OPT_NONE, HITS, MEE_MEM_HOST_PINNED), *c64n = table(64, MEE_OPT_NONE, 0, MEE_MEM_HOST_PINNED);
    mee_table *h128 = table(128, MEE_OPT_NONE), *c128 = table(128, MEE_OPT_NONE, 0, MEE_MEM_HOST_PINNED), *h24 = table(24, MEE_OPT_NONE), *c24 = table(24, MEE_OPT_NONE);
    for (uint32_t fl = 0; fl < 4; ++fl)
        CASE(nm("mee_find_pooled_tiered", "dim64 short f32 flags=" + std::to_string(fl)).c_str(), mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, F32, found, SUM, fl, nullptr));
    CASE("mee_find_pooled_tiered dim64 long f32", mee_find_pooled_tiered(h64, c64, keys, kLong, offsets, kBags, out, F32, found, MEAN, 0, nullptr));
    CASE("mee_find_pooled_tiered dim64 long bf16", mee_find_pooled_tiered(h64, c64, keys, kLong, offsets, kBags, out, BF16, found, SUM, 3, nullptr));
    CASE("mee_find_pooled_tiered dim64 short bf16", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, BF16, nullptr, SUM, 0, nullptr));
    for (size_t n : {kShort, kLong}) {
        CASE(nm("mee_find_pooled_tiered dim128", n == kShort ? "short" : "long").c_str(), mee_find_pooled_tiered(h128, c128, keys, n, offsets, kBags, out, F32, found, SUM, 0, nullptr));
        CASE(nm("mee_find_pooled_tiered dim24", n == kShort ? "short" : "long").c_str(), mee_find_pooled_tiered(h24, c24, keys, n, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    }
    CASE("mee_find_pooled_tiered n_bags=0", mee_find_pooled_tiered(h64, c64, nullptr, 0, nullptr, 0, nullptr, F32, nullptr, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered null cold", mee_find_pooled_tiered(h64, nullptr, keys, kShort, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered null out", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, nullptr, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered same table", mee_find_pooled_tiered(h64, h64, keys, kShort, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered dims differ", mee_find_pooled_tiered(h64, c128, keys, kShort, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered unknown flag", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, F32, found, SUM, 4, nullptr));
    CASE("mee_find_pooled_tiered cold without counters", mee_find_pooled_tiered(h64, c64n, keys, kShort, offsets, kBags, out, F32, found, SUM, MEE_TIER_COUNT_COLD, nullptr));
    CASE("mee_find_pooled_tiered hot without counters", mee_find_pooled_tiered(h128, c128, keys, kShort, offsets, kBags, out, F32, found, SUM, MEE_TIER_COUNT_HOT, nullptr));
    CASE("mee_find_pooled_tiered bf16-row hot", mee_find_pooled_tiered(b64, c64, keys, kShort, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered int8-row cold", mee_find_pooled_tiered(h64, i64, keys, kShort, offsets, kBags, out, F32, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered bad dtype", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, 9, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered misaligned bf16", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, odd, BF16, found, SUM, 0, nullptr));
    CASE("mee_find_pooled_tiered bad mode", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, F32, found, 7, 0, nullptr));
    CASE("mee_find_pooled_tiered same table + bad mode", mee_find_pooled_tiered(h64, h64, keys, kShort, offsets, kBags, out, F32, found, 7, 0, nullptr));
    CASE("mee_find_pooled_tiered unknown flag + bad dtype", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, 9, found, SUM, 4, nullptr));
    CASE("mee_find_pooled_tiered bad dtype + bad mode", mee_find_pooled_tiered(h64, c64, keys, kShort, offsets, kBags, out, 9, found, 7, 0, nullptr));

    for (auto& s : shapes) {
        if (s.t == b64 || s.t == b24) continue;
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_pooled_weighted_backward", std::string(s.n) + (n == kShort ? " short" : " long")).c_str(),
                 mee_pooled_weighted_backward(s.t, keys, located, n, offsets, kBags, weights, grads, grads, n == kShort ? wgrads : nullptr, nullptr));
    }
    CASE("mee_pooled_weighted_backward no handles", mee_pooled_weighted_backward(t64, keys, nullptr, kShort, offsets, kBags, weights, grads, grads, wgrads, nullptr));
    CASE("mee_pooled_weighted_backward n_bags=0", mee_pooled_weighted_backward(t64, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    CASE("mee_pooled_weighted_backward null table", mee_pooled_weighted_backward(nullptr, keys, located, kShort, offsets, kBags, weights, grads, grads, wgrads, nullptr));
    CASE("mee_pooled_weighted_backward null bag grads", mee_pooled_weighted_backward(t64, keys, located, kShort, offsets, kBags, weights, nullptr, grads, wgrads, nullptr));
    CASE("mee_pooled_weighted_backward null grads out", mee_pooled_weighted_backward(t64, keys, located, kShort, offsets, kBags, weights, grads, nullptr, wgrads, nullptr));
    CASE("mee_pooled_weighted_backward bf16 rows + null weights", mee_pooled_weighted_backward(b64, keys, located, kShort, offsets, kBags, nullptr, grads, grads, wgrads, nullptr));
}

static void pooled_groups() {
    auto fp32 = [](uint32_t dim, uint32_t flags = 0) { return group({table(dim, MEE_OPT_NONE, flags), table(dim, MEE_OPT_NONE, flags)}); };
    mee_group *g64 = fp32(64), *g128 = fp32(128), *g24 = fp32(24), *g24x3 = group({table(24, MEE_OPT_NONE), table(24, MEE_OPT_NONE), table(24, MEE_OPT_NONE)});
    mee_group *gb64 = fp32(64, MEE_FLAG_BF16_ROWS), *gb24 = fp32(24, MEE_FLAG_BF16_ROWS);
    struct { const char* n; mee_group* g; size_t B; } shapes[] = {{"dim64", g64, 2}, {"dim128", g128, 2}, {"dim24", g24, 2}, {"bf16rows64", gb64, 2}, {"bf16rows24", gb24, 2}};
    auto len = [](size_t n) { return n == kShort ? " short" : " long"; };

    for (auto& s : shapes)
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_group_find_pooled", std::string(s.n) + len(n)).c_str(), mee_group_find_pooled(s.g, keys, n, offsets, s.B, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled located mean", mee_group_find_pooled(g64, keys, kShort, offsets, 2, outf, nullptr, located, MEAN, nullptr));
    CASE("mee_group_find_pooled bags=0", mee_group_find_pooled(g64, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled null group", mee_group_find_pooled(nullptr, keys, kShort, offsets, 2, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled null offsets", mee_group_find_pooled(g64, keys, kShort, nullptr, 2, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled null keys", mee_group_find_pooled(g64, nullptr, kShort, offsets, 2, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled bad mode", mee_group_find_pooled(g64, keys, kShort, offsets, 2, outf, found, nullptr, 7, nullptr));
    CASE("mee_group_find_pooled located on bf16 rows", mee_group_find_pooled(gb64, keys, kShort, offsets, 2, outf, found, located, SUM, nullptr));
    CASE("mee_group_find_pooled located on bf16 rows + null out", mee_group_find_pooled(gb64, keys, kShort, offsets, 2, nullptr, found, located, SUM, nullptr));
    CASE("mee_group_find_pooled null out + bad mode", mee_group_find_pooled(g64, keys, kShort, offsets, 2, nullptr, found, nullptr, 7, nullptr));

    for (auto& s : shapes)
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_group_find_pooled_jagged", std::string(s.n) + len(n)).c_str(), mee_group_find_pooled_jagged(s.g, keys, n, offsets, kBags, member_bags, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_jagged located mean", mee_group_find_pooled_jagged(g64, keys, kShort, offsets, kBags, member_bags, outf, nullptr, located, MEAN, nullptr));
    CASE("mee_group_find_pooled_jagged n_bags=0", mee_group_find_pooled_jagged(g64, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_jagged null group", mee_group_find_pooled_jagged(nullptr, keys, kShort, offsets, kBags, member_bags, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_jagged null member bags", mee_group_find_pooled_jagged(g64, keys, kShort, offsets, kBags, nullptr, outf, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_jagged bad mode", mee_group_find_pooled_jagged(g64, keys, kShort, offsets, kBags, member_bags, outf, found, nullptr, 7, nullptr));
    CASE("mee_group_find_pooled_jagged located on bf16 rows", mee_group_find_pooled_jagged(gb64, keys, kShort, offsets, kBags, member_bags, outf, found, located, SUM, nullptr));
    CASE("mee_group_find_pooled_jagged null member bags + bad mode", mee_group_find_pooled_jagged(g64, keys, kShort, offsets, kBags, nullptr, outf, found, nullptr, 7, nullptr));

    for (auto& s : shapes) {
        if (s.g == gb64 || s.g == gb24) continue;
        for (size_t n : {kShort, kLong})
            CASE(nm("mee_group_find_pooled_weighted", std::string(s.n) + len(n) + (n == kLong ? " located" : "")).c_str(),
                 mee_group_find_pooled_weighted(s.g, keys, n, offsets, s.B, weights, outf, found, n == kLong ? located : nullptr, nullptr));
    }
    CASE("mee_group_find_pooled_weighted n=0 null weights", mee_group_find_pooled_weighted(g64, nullptr, 0, offsets, 2, nullptr, outf, found, nullptr, nullptr));
    CASE("mee_group_find_pooled_weighted bags=0", mee_group_find_pooled_weighted(g64, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    CASE("mee_group_find_pooled_weighted null group", mee_group_find_pooled_weighted(nullptr, keys, kShort, offsets, 2, weights, outf, found, nullptr, nullptr));
    CASE("mee_group_find_pooled_weighted null weights", mee_group_find_pooled_weighted(g64, keys, kShort, offsets, 2, nullptr, outf, found, nullptr, nullptr));
    CASE("mee_group_find_pooled_weighted bf16 rows", mee_group_find_pooled_weighted(gb64, keys, kShort, offsets, 2, weights, outf, found, nullptr, nullptr));
    CASE("mee_group_find_pooled_weighted bf16 rows + null weights", mee_group_find_pooled_weighted(gb64, keys, kShort, offsets, 2, nullptr, outf, found, nullptr, nullptr));

    for (uint32_t dt : {F32, BF16}) {
        const std::string d = dt == F32 ? "f32" : "bf16";
        for (auto& s : shapes) CASE(nm("mee_group_find_pooled_as", d + " " + s.n + " short").c_str(), mee_group_find_pooled_as(s.g, keys, kShort, offsets, s.B, nullptr, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_group_find_pooled_as", d + " dim64 long located mean").c_str(), mee_group_find_pooled_as(g64, keys, kLong, offsets, 2, nullptr, out, dt, found, located, MEAN, nullptr));
        CASE(nm("mee_group_find_pooled_as", d + " bf16rows64 long").c_str(), mee_group_find_pooled_as(gb64, keys, kLong, offsets, 2, nullptr, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_group_find_pooled_as", d + " weighted dim64 short").c_str(), mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, weights, out, dt, found, nullptr, SUM, nullptr));
        CASE(nm("mee_group_find_pooled_as", d + " weighted located dim128 long").c_str(), mee_group_find_pooled_as(g128, keys, kLong, offsets, 2, weights, out, dt, found, located, SUM, nullptr));
        CASE(nm("mee_group_find_pooled_as", d + " weighted dim24 long").c_str(), mee_group_find_pooled_as(g24, keys, 6 * 12, offsets, 2, weights, out, dt, nullptr, nullptr, SUM, nullptr));
    }
    CASE("mee_group_find_pooled_as bags=0", mee_group_find_pooled_as(g64, nullptr, 0, nullptr, 0, nullptr, nullptr, F32, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as null group", mee_group_find_pooled_as(nullptr, keys, kShort, offsets, 2, nullptr, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as null out", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, nullptr, nullptr, F32, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as bad dtype", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, nullptr, out, 9, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as misaligned bf16", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, nullptr, odd, BF16, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as bad mode", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, nullptr, out, F32, found, nullptr, 7, nullptr));
    CASE("mee_group_find_pooled_as weighted mean", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, weights, out, F32, found, nullptr, MEAN, nullptr));
    CASE("mee_group_find_pooled_as weighted bf16 rows", mee_group_find_pooled_as(gb64, keys, kShort, offsets, 2, weights, out, F32, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as located on bf16 rows", mee_group_find_pooled_as(gb64, keys, kShort, offsets, 2, nullptr, out, F32, found, located, SUM, nullptr));
    CASE("mee_group_find_pooled_as weighted bf16 rows + bad dtype", mee_group_find_pooled_as(gb64, keys, kShort, offsets, 2, weights, out, 9, found, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_as bad dtype + weighted mean", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, weights, out, 9, found, nullptr, MEAN, nullptr));
    CASE("mee_group_find_pooled_as bad mode + weighted", mee_group_find_pooled_as(g64, keys, kShort, offsets, 2, weights, out, F32, found, nullptr, 7, nullptr));

    // groups of hot/cold pairs
    const uint32_t HITS = MEE_FLAG_TRACK_HITS;
    mee_group *h64 = fp32(64, HITS), *c64 = fp32(64, HITS), *c64n = fp32(64), *h128 = fp32(128), *c128 = fp32(128), *h24 = fp32(24), *c24 = fp32(24);
    for (uint32_t fl = 0; fl < 4; ++fl) {
        const std::string f = "flags=" + std::to_string(fl);
        CASE(nm("mee_group_find_pooled_tiered dim64 short f32", f).c_str(), mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, out, F32, found, SUM, fl, nullptr));
        CASE(nm("mee_group_find_pooled_tiered_jagged dim64 short", f).c_str(), mee_group_find_pooled_tiered_jagged(h64, c64, keys, kShort, offsets, kBags, member_bags, outf, found, SUM, fl, nullptr));
        CASE(nm("mee_group_find_pooled_tiered_keyed dim64 short f32", f).c_str(), mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, SUM, fl, nullptr));
    }
    struct { const char* n; mee_group *h, *c; } pairs[] = {{"dim64", h64, c64}, {"dim128", h128, c128}, {"dim24", h24, c24}};
    for (auto& p : pairs)
        for (size_t n : {kShort, kLong}) {
            CASE(nm("mee_group_find_pooled_tiered", std::string(p.n) + len(n) + " bf16 mean").c_str(), mee_group_find_pooled_tiered(p.h, p.c, keys, n, offsets, 2, out, BF16, found, MEAN, 0, nullptr));
            CASE(nm("mee_group_find_pooled_tiered", std::string(p.n) + len(n) + " f32").c_str(), mee_group_find_pooled_tiered(p.h, p.c, keys, n, offsets, 2, out, F32, nullptr, SUM, 0, nullptr));
            CASE(nm("mee_group_find_pooled_tiered_jagged", std::string(p.n) + len(n)).c_str(), mee_group_find_pooled_tiered_jagged(p.h, p.c, keys, n, offsets, kBags, member_bags, outf, found, MEAN, 0, nullptr));
            CASE(nm("mee_group_find_pooled_tiered_keyed", std::string(p.n) + len(n) + " bf16 index").c_str(),
                 mee_group_find_pooled_tiered_keyed(p.h, p.c, keys, n, offsets, 2, out, BF16, 0, found, index32, MEAN, 0, nullptr));
            CASE(nm("mee_group_find_pooled_tiered_keyed", std::string(p.n) + len(n) + " f32 stride").c_str(),
                 mee_group_find_pooled_tiered_keyed(p.h, p.c, keys, n, offsets, 2, out, F32, 512, nullptr, nullptr, SUM, 0, nullptr));
        }
    CASE("mee_group_find_pooled_tiered bags=0", mee_group_find_pooled_tiered(h64, c64, nullptr, 0, nullptr, 0, nullptr, F32, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered null cold", mee_group_find_pooled_tiered(h64, nullptr, keys, kShort, offsets, 2, out, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered null out", mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, nullptr, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered same group", mee_group_find_pooled_tiered(h64, h64, keys, kShort, offsets, 2, out, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered dims differ", mee_group_find_pooled_tiered(h64, c128, keys, kShort, offsets, 2, out, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered table counts differ", mee_group_find_pooled_tiered(g24x3, c24, keys, kShort, offsets, 2, out, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered unknown flag", mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, out, F32, found, SUM, 8, nullptr));
    CASE("mee_group_find_pooled_tiered cold without counters", mee_group_find_pooled_tiered(h64, c64n, keys, kShort, offsets, 2, out, F32, found, SUM, MEE_TIER_COUNT_COLD, nullptr));
    CASE("mee_group_find_pooled_tiered bf16-row hot", mee_group_find_pooled_tiered(gb64, c64, keys, kShort, offsets, 2, out, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered bad dtype", mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, out, 9, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered bad mode", mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, out, F32, found, 7, 0, nullptr));
    CASE("mee_group_find_pooled_tiered same group + bad dtype", mee_group_find_pooled_tiered(h64, h64, keys, kShort, offsets, 2, out, 9, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered null out + same group", mee_group_find_pooled_tiered(h64, h64, keys, kShort, offsets, 2, nullptr, F32, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered bad dtype + bad mode", mee_group_find_pooled_tiered(h64, c64, keys, kShort, offsets, 2, out, 9, found, 7, 0, nullptr));

    CASE("mee_group_find_pooled_tiered_jagged n_bags=0", mee_group_find_pooled_tiered_jagged(h64, c64, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged null hot", mee_group_find_pooled_tiered_jagged(nullptr, c64, keys, kShort, offsets, kBags, member_bags, outf, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged null member bags", mee_group_find_pooled_tiered_jagged(h64, c64, keys, kShort, offsets, kBags, nullptr, outf, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged same group", mee_group_find_pooled_tiered_jagged(h64, h64, keys, kShort, offsets, kBags, member_bags, outf, found, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged hot without counters", mee_group_find_pooled_tiered_jagged(c64n, c64, keys, kShort, offsets, kBags, member_bags, outf, found, SUM, MEE_TIER_COUNT_HOT, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged bad mode", mee_group_find_pooled_tiered_jagged(h64, c64, keys, kShort, offsets, kBags, member_bags, outf, found, 7, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_jagged unknown flag + bad mode", mee_group_find_pooled_tiered_jagged(h64, c64, keys, kShort, offsets, kBags, member_bags, outf, found, 7, 8, nullptr));

    CASE("mee_group_find_pooled_tiered_keyed bags=0", mee_group_find_pooled_tiered_keyed(h64, c64, nullptr, 0, nullptr, 0, nullptr, F32, 0, nullptr, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed null cold", mee_group_find_pooled_tiered_keyed(h64, nullptr, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed same group", mee_group_find_pooled_tiered_keyed(h64, h64, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed bad mode", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, 7, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed bad dtype", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, 9, 0, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed misaligned f32", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, odd, F32, 0, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed narrow stride", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, F32, 64, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed stride not x4", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, F32, 130, found, nullptr, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed index past 2^32", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, (size_t)1 << 31, out, F32, 0, found, index32, SUM, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed bad mode + bad dtype", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, 9, 0, found, nullptr, 7, 0, nullptr));
    CASE("mee_group_find_pooled_tiered_keyed unknown flag + narrow stride", mee_group_find_pooled_tiered_keyed(h64, c64, keys, kShort, offsets, 2, out, F32, 64, found, nullptr, SUM, 8, nullptr));

    // the keyed layout of a uniform group
    for (uint32_t dt : {F32, BF16}) {
        const std::string d = dt == F32 ? "f32" : "bf16";
        for (auto& s : shapes) {
            const bool rows32 = s.g != gb64 && s.g != gb24;
            CASE(nm("mee_group_find_pooled_keyed", d + " " + s.n + " short").c_str(), mee_group_find_pooled_keyed(s.g, keys, kShort, offsets, s.B, out, dt, 0, found, nullptr, nullptr, SUM, nullptr));
            CASE(nm("mee_group_find_pooled_keyed", d + " " + s.n + " long stride" + (rows32 ? " located index" : "")).c_str(),
                 mee_group_find_pooled_keyed(s.g, keys, 6 * 12, offsets, s.B, out, dt, 1024, nullptr, rows32 ? located : nullptr, rows32 ? index32 : nullptr, MEAN, nullptr));
        }
    }
    CASE("mee_group_find_pooled_keyed bags=0", mee_group_find_pooled_keyed(g64, nullptr, 0, nullptr, 0, nullptr, F32, 0, nullptr, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed null group", mee_group_find_pooled_keyed(nullptr, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed null out", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, nullptr, F32, 0, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed bad mode", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, nullptr, 7, nullptr));
    CASE("mee_group_find_pooled_keyed bad dtype", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, 9, 0, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed misaligned f32", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, odd, F32, 0, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed misaligned bf16", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, odd, BF16, 0, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed narrow stride", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, F32, 124, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed stride not x4", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, F32, 129, found, nullptr, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed index past 2^32", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, (size_t)1 << 31, out, F32, 0, found, nullptr, index32, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed located on bf16 rows", mee_group_find_pooled_keyed(gb64, keys, kShort, offsets, 2, out, F32, 0, found, located, nullptr, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed index on bf16 rows", mee_group_find_pooled_keyed(gb64, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, index32, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed index on bf16 rows + null out", mee_group_find_pooled_keyed(gb64, keys, kShort, offsets, 2, nullptr, F32, 0, found, nullptr, index32, SUM, nullptr));
    CASE("mee_group_find_pooled_keyed bad mode + bad dtype", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, 9, 0, found, nullptr, nullptr, 7, nullptr));
    CASE("mee_group_find_pooled_keyed bad dtype + narrow stride", mee_group_find_pooled_keyed(g64, keys, kShort, offsets, 2, out, 9, 124, found, nullptr, nullptr, SUM, nullptr));

    for (auto& s : shapes) {
        if (s.g == gb64 || s.g == gb24) continue;
        for (size_t n : {kShort, (size_t)6 * 12})
            CASE(nm("mee_group_pooled_weighted_backward", std::string(s.n) + (n == kShort ? " short" : " long")).c_str(),
                 mee_group_pooled_weighted_backward(s.g, keys, located, n, offsets, s.B, weights, grads, grads, n == kShort ? wgrads : nullptr, nullptr));
    }
    CASE("mee_group_pooled_weighted_backward bags=0", mee_group_pooled_weighted_backward(g64, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
    CASE("mee_group_pooled_weighted_backward null group", mee_group_pooled_weighted_backward(nullptr, keys, located, kShort, offsets, 2, weights, grads, grads, wgrads, nullptr));
    CASE("mee_group_pooled_weighted_backward null weights", mee_group_pooled_weighted_backward(g64, keys, located, kShort, offsets, 2, nullptr, grads, grads, wgrads, nullptr));
    CASE("mee_group_pooled_weighted_backward bf16 rows + null weights", mee_group_pooled_weighted_backward(gb64, keys, located, kShort, offsets, 2, nullptr, grads, grads, wgrads, nullptr));
}

static void pooled_mixed() {
    auto t = [](uint32_t dim) { return table(dim, MEE_OPT_NONE); };
    mee_mixed_group *one = mixed({t(16), t(16)}), *two = mixed({t(8), t(16)}), *wide = mixed({t(64), t(128), t(256)});
    struct { const char* n; mee_mixed_group* g; } groups[] = {{"one class", one}, {"two classes", two}, {"three classes wide", wide}};
    for (auto& s : groups)
        for (uint32_t dt : {F32, BF16})
            for (int ins : {0, 1})
                for (size_t n : {kShort, kLong}) {
                    if (s.g == wide && n != (ins ? kLong : kShort)) continue;
                    const size_t nn = s.g == wide && n == kLong ? 6 * 12 : n;
                    const std::string what = std::string(s.n) + (dt == F32 ? " f32" : " bf16") + (ins ? " insert" : "") + (n == kShort ? " short" : " long");
                    CASE(nm("mee_mixed_group_find_pooled", what).c_str(), mee_mixed_group_find_pooled(s.g, keys, nn, offsets, 2, out, dt, found, ins ? located : nullptr, ins ? MEAN : SUM, ins, nullptr));
                    CASE(nm("mee_mixed_group_find_pooled_keyed", what).c_str(),
                         mee_mixed_group_find_pooled_keyed(s.g, keys, nn, offsets, 2, out, dt, ins ? 1024 : 0, found, ins ? located : nullptr, ins ? nullptr : index32, ins ? MEAN : SUM, ins, nullptr));
                }
    for (auto& s : groups) {
        if (s.g == wide) continue;
        const std::string c = s.n;
        CASE(nm("mee_mixed_group_find_pooled", c + " bags=0").c_str(), mee_mixed_group_find_pooled(s.g, nullptr, 0, nullptr, 0, nullptr, F32, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " n=0 insert").c_str(), mee_mixed_group_find_pooled(s.g, nullptr, 0, offsets, 2, out, F32, nullptr, nullptr, SUM, 1, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " null out").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, nullptr, F32, found, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " bad dtype").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, out, 9, found, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " misaligned bf16").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, odd, BF16, found, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " bad mode").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, out, F32, found, nullptr, 7, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " insert without found").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, out, F32, nullptr, nullptr, SUM, 1, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " bad dtype + bad mode").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, out, 9, found, nullptr, 7, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled", c + " bad mode + insert without found").c_str(), mee_mixed_group_find_pooled(s.g, keys, kShort, offsets, 2, out, F32, nullptr, nullptr, 7, 1, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " bags=0").c_str(), mee_mixed_group_find_pooled_keyed(s.g, nullptr, 0, nullptr, 0, nullptr, F32, 0, nullptr, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " null keys").c_str(), mee_mixed_group_find_pooled_keyed(s.g, nullptr, kShort, offsets, 2, out, F32, 0, found, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " bad mode").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, nullptr, 7, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " insert without found").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, out, F32, 0, nullptr, nullptr, nullptr, SUM, 1, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " bad dtype").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, out, 9, 0, found, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " misaligned f32").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, odd, F32, 0, found, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " narrow stride").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, out, F32, 16, found, nullptr, nullptr, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " index past 2^32").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, (size_t)1 << 31, out, F32, 0, found, nullptr, index32, SUM, 0, nullptr));
        CASE(nm("mee_mixed_group_find_pooled_keyed", c + " insert without found + bad dtype").c_str(), mee_mixed_group_find_pooled_keyed(s.g, keys, kShort, offsets, 2, out, 9, 0, nullptr, nullptr, nullptr, SUM, 1, nullptr));
    }
    CASE("mee_mixed_group_find_pooled null group", mee_mixed_group_find_pooled(nullptr, keys, kShort, offsets, 2, out, F32, found, nullptr, SUM, 0, nullptr));
    CASE("mee_mixed_group_find_pooled_keyed null group", mee_mixed_group_find_pooled_keyed(nullptr, keys, kShort, offsets, 2, out, F32, 0, found, nullptr, nullptr, SUM, 0, nullptr));
}

// ---- optimizer steps ---------------------------------------------------------------------------------------------------------------------------
struct Scalars { float lr = 0.1f, b = 0.9f, c = 0.999f, d = 1e-8f; uint64_t step = 1; };   // adagrad: lr, d = eps; adam: lr, b, c = betas, d = eps, step; ftrl: lr, b = beta, c = l1, d = l2
static Scalars ok_scalars(uint32_t kind) { Scalars s; if (kind == MEE_OPT_FTRL) { s.b = 1.f; s.c = 0.01f; s.d = 0.001f; } return s; }
static const char* kind_name(uint32_t kind) { return kind == MEE_OPT_ADAGRAD ? "adagrad" : kind == MEE_OPT_ADAM ? "adam" : "ftrl"; }
enum Form { ByKey, Located, Indexed, Pooled };
static const char* form_suffix(Form f) { return f == ByKey ? "" : f == Located ? "_located" : f == Indexed ? "_indexed" : "_pooled"; }

struct TableStep { mee_table* t; const int64_t* k = keys; const int64_t* sl = slots; const float* g = grads; size_t rows = 16; const uint32_t* idx = index32; size_t n = 32; };
static int table_step(uint32_t kind, Form f, const TableStep& a, const Scalars& s) {
    if (kind == MEE_OPT_ADAGRAD)
        return f == ByKey ? mee_apply_adagrad(a.t, a.k, a.g, a.n, s.lr, s.d, nullptr) : f == Located ? mee_apply_adagrad_located(a.t, a.k, a.sl, a.g, a.n, s.lr, s.d, nullptr)
                                                                                       : mee_apply_adagrad_indexed(a.t, a.k, a.g, a.rows, a.idx, a.n, s.lr, s.d, nullptr);
    if (kind == MEE_OPT_ADAM)
        return f == ByKey ? mee_apply_adam(a.t, a.k, a.g, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr) : f == Located ? mee_apply_adam_located(a.t, a.k, a.sl, a.g, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr)
                                                                                                    : mee_apply_adam_indexed(a.t, a.k, a.g, a.rows, a.idx, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr);
    return f == ByKey ? mee_apply_ftrl(a.t, a.k, a.g, a.n, s.lr, s.b, s.c, s.d, nullptr) : f == Located ? mee_apply_ftrl_located(a.t, a.k, a.sl, a.g, a.n, s.lr, s.b, s.c, s.d, nullptr)
                                                                                        : mee_apply_ftrl_indexed(a.t, a.k, a.g, a.rows, a.idx, a.n, s.lr, s.b, s.c, s.d, nullptr);
}
struct GroupStep { mee_group* g; const int64_t* k = keys; const uint64_t* off = offsets; size_t B = 2; const float* gr = grads; size_t rows = 16; const uint32_t* idx = index32; const int64_t* loc = nullptr; size_t n = 32; };
static int group_step(uint32_t kind, Form f, const GroupStep& a, const Scalars& s) {
    if (kind == MEE_OPT_ADAGRAD)
        return f == ByKey ? mee_group_apply_adagrad(a.g, a.k, a.off, a.gr, a.n, s.lr, s.d, nullptr)
             : f == Pooled ? mee_group_apply_adagrad_pooled(a.g, a.k, a.off, a.B, a.gr, a.idx, a.loc, a.n, s.lr, s.d, nullptr)
                           : mee_group_apply_adagrad_indexed(a.g, a.k, a.off, a.gr, a.rows, a.idx, a.n, s.lr, s.d, nullptr);
    if (kind == MEE_OPT_ADAM)
        return f == ByKey ? mee_group_apply_adam(a.g, a.k, a.off, a.gr, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr)
             : f == Pooled ? mee_group_apply_adam_pooled(a.g, a.k, a.off, a.B, a.gr, a.idx, a.loc, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr)
                           : mee_group_apply_adam_indexed(a.g, a.k, a.off, a.gr, a.rows, a.idx, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr);
    return f == ByKey ? mee_group_apply_ftrl(a.g, a.k, a.off, a.gr, a.n, s.lr, s.b, s.c, s.d, nullptr)
         : f == Pooled ? mee_group_apply_ftrl_pooled(a.g, a.k, a.off, a.B, a.gr, a.idx, a.loc, a.n, s.lr, s.b, s.c, s.d, nullptr)
                       : mee_group_apply_ftrl_indexed(a.g, a.k, a.off, a.gr, a.rows, a.idx, a.n, s.lr, s.b, s.c, s.d, nullptr);
}
struct MixedStep { mee_mixed_group* g; const int64_t* k = keys; const uint64_t* off = offsets; size_t B = 2; const float* gr = grads; const uint32_t* bag = index32; const int64_t* loc = nullptr; size_t n = 32; };
static int mixed_step(uint32_t kind, const MixedStep& a, const Scalars& s) {
    if (kind == MEE_OPT_ADAGRAD) return mee_mixed_group_apply_adagrad_pooled(a.g, a.k, a.off, a.B, a.gr, a.bag, a.loc, a.n, s.lr, s.d, nullptr);
    if (kind == MEE_OPT_ADAM) return mee_mixed_group_apply_adam_pooled(a.g, a.k, a.off, a.B, a.gr, a.bag, a.loc, a.n, s.lr, s.b, s.c, s.d, s.step, nullptr);
    return mee_mixed_group_apply_ftrl_pooled(a.g, a.k, a.off, a.B, a.gr, a.bag, a.loc, a.n, s.lr, s.b, s.c, s.d, nullptr);
}
// the bad scalars of a rule, each with a name: Adam's step 0; every way FTRL's four can be wrong
static std::vector<std::pair<std::string, Scalars>> bad_scalars(uint32_t kind) {
    std::vector<std::pair<std::string, Scalars>> v;
    auto with = [&](const char* n, auto set) { Scalars s = ok_scalars(kind); set(s); v.push_back({n, s}); };
    if (kind == MEE_OPT_ADAM) with("step=0", [](Scalars& s) { s.step = 0; });
    if (kind == MEE_OPT_FTRL) {
        with("lr=0", [](Scalars& s) { s.lr = 0.f; });
        with("lr<0", [](Scalars& s) { s.lr = -0.1f; });
        with("lr=inf", [](Scalars& s) { s.lr = INFINITY; });
        with("lr=nan", [](Scalars& s) { s.lr = NAN; });
        with("beta<0", [](Scalars& s) { s.b = -1.f; });
        with("beta=nan", [](Scalars& s) { s.b = NAN; });
        with("l1<0", [](Scalars& s) { s.c = -0.5f; });
        with("l1=nan", [](Scalars& s) { s.c = NAN; });
        with("l2<0", [](Scalars& s) { s.d = -2.f; });
        with("l2=nan", [](Scalars& s) { s.d = NAN; });
    }
    return v;
}

static void steps() {
    const uint32_t kinds[] = {MEE_OPT_ADAGRAD, MEE_OPT_ADAM, MEE_OPT_FTRL};
    mee_table* bf16_table = table(64, MEE_OPT_NONE, MEE_FLAG_BF16_ROWS);
    mee_table* plain = table(64, MEE_OPT_NONE);
    mee_group* bf16_group = group({table(64, MEE_OPT_NONE, MEE_FLAG_BF16_ROWS), table(64, MEE_OPT_NONE, MEE_FLAG_BF16_ROWS)});
    for (uint32_t kind : kinds) {
        const uint32_t other = kind == MEE_OPT_ADAM ? MEE_OPT_ADAGRAD : MEE_OPT_ADAM;
        const Scalars ok = ok_scalars(kind);
        const auto bad = bad_scalars(kind);
        mee_table *t = table(64, kind), *t24 = table(24, kind), *wrong = table(64, other);
        for (Form f : {ByKey, Located, Indexed}) {
            const std::string e = std::string("mee_apply_") + kind_name(kind) + form_suffix(f);
            auto step = [&](const std::string& what, TableStep a, const Scalars& s) { CASE((e + " " + what).c_str(), table_step(kind, f, a, s)); };
            step("dim64", {t}, ok);
            step("n=0", [&] { TableStep a{t, nullptr, nullptr, nullptr, 16, nullptr, 0}; return a; }(), ok);
            step("null keys", [&] { TableStep a{t}; a.k = nullptr; return a; }(), ok);
            const bool shared = f == ByKey;   // the refusals of the path all three forms share: once per optimizer
            if (shared) {
                step("dim24 n=64", [&] { TableStep a{t24}; a.n = 64; return a; }(), ok);
                step("null table", {nullptr}, ok);
                step("null grads", [&] { TableStep a{t}; a.g = nullptr; return a; }(), ok);
                step("no optimizer", {plain}, ok);
                step("wrong optimizer + null grads", [&] { TableStep a{wrong}; a.g = nullptr; return a; }(), ok);
                step("wrong optimizer + n over max_batch", [&] { TableStep a{wrong}; a.n = 65; return a; }(), ok);
            }
            if (f == Located) step("null slots", [&] { TableStep a{t}; a.sl = nullptr; return a; }(), ok);
            if (f == Indexed) {
                step("null index", [&] { TableStep a{t}; a.idx = nullptr; return a; }(), ok);
                step("n_grad_rows=0", [&] { TableStep a{t}; a.rows = 0; return a; }(), ok);
                step("n_grad_rows=2^32", [&] { TableStep a{t}; a.rows = (size_t)1 << 32; return a; }(), ok);
                step("n_grad_rows=2^32-1", [&] { TableStep a{t}; a.rows = 0xFFFFFFFFull; return a; }(), ok);
            }
            step("wrong optimizer", {wrong}, ok);
            step("n over max_batch", [&] { TableStep a{t}; a.n = 65; return a; }(), ok);
            step("bf16-row table", {bf16_table}, ok);
            for (size_t i = 0; i < bad.size(); ++i)
                if (f == ByKey || i == (size_t)f) step(bad[i].first, {t}, bad[i].second);
            if (!bad.empty()) {   // two faults at once: which refusal wins
                step(bad[0].first + " + null keys", [&] { TableStep a{t}; a.k = nullptr; return a; }(), bad[0].second);
                step(bad[0].first + " + wrong optimizer", {wrong}, bad[0].second);
                step(bad[0].first + " + bf16-row table", {bf16_table}, bad[0].second);
                if (f == Located) step(bad[0].first + " + null slots", [&] { TableStep a{t}; a.sl = nullptr; return a; }(), bad[0].second);
                if (f == Indexed) step(bad[0].first + " + n_grad_rows=0", [&] { TableStep a{t}; a.rows = 0; return a; }(), bad[0].second);
            }
            if (f == Located) step("null slots + bf16-row table", [&] { TableStep a{bf16_table}; a.sl = nullptr; return a; }(), ok);
            if (f == Indexed) step("null index + null table", [&] { TableStep a{nullptr}; a.idx = nullptr; return a; }(), ok);
            // mee_apply_prepare, then the step: with other keys, with another n, with the prepared batch
            CASE((e + " / mee_apply_prepare").c_str(), mee_apply_prepare(t, keys, 32, nullptr));
            step("other keys than prepared", [&] { TableStep a{t}; a.k = keys + 1; return a; }(), ok);
            if (shared) step("other n than prepared", [&] { TableStep a{t}; a.n = 16; return a; }(), ok);
            step("as prepared", {t}, ok);
            if (shared) step("after the prepared step", {t}, ok);
        }
        CASE((std::string("mee_apply_prepare twice ") + kind_name(kind)).c_str(), (mee_apply_prepare(t, keys, 32, nullptr), mee_apply_prepare(t, keys, 32, nullptr)));
        CASE((std::string("mee_apply_discard ") + kind_name(kind)).c_str(), mee_apply_discard(t, nullptr));

        mee_group *g = group({table(64, kind), table(64, kind)}, 64), *g24 = group({table(24, kind), table(24, kind), table(24, kind)}, 64);
        mee_group *gwrong = group({table(64, other), table(64, other)}, 64), *g0 = group({table(64, kind), table(64, kind)}, 0);
        for (Form f : {ByKey, Pooled, Indexed}) {
            const std::string e = std::string("mee_group_apply_") + kind_name(kind) + form_suffix(f);
            auto step = [&](const std::string& what, GroupStep a, const Scalars& s) { CASE((e + " " + what).c_str(), group_step(kind, f, a, s)); };
            step("dim64", {g}, ok);
            step("n=0", [&] { GroupStep a{g}; a.k = nullptr; a.gr = nullptr; a.idx = nullptr; a.n = 0; return a; }(), ok);
            step("null offsets", [&] { GroupStep a{g}; a.off = nullptr; return a; }(), ok);
            const bool shared = f == ByKey;   // the refusals of the path all three forms share: once per optimizer
            if (shared) {
                step("dim24 x3 n=64", [&] { GroupStep a{g24}; a.n = 64; return a; }(), ok);
                step("n=0 null offsets", [&] { GroupStep a{g}; a.k = nullptr; a.off = nullptr; a.gr = nullptr; a.idx = nullptr; a.n = 0; return a; }(), ok);
                step("null group", {nullptr}, ok);
                step("null keys", [&] { GroupStep a{g}; a.k = nullptr; return a; }(), ok);
                step("null grads", [&] { GroupStep a{g}; a.gr = nullptr; return a; }(), ok);
                step("max_apply_batch=0 + null grads", [&] { GroupStep a{g0}; a.gr = nullptr; return a; }(), ok);
                step("wrong optimizer + n over max_apply_batch", [&] { GroupStep a{gwrong}; a.n = 65; return a; }(), ok);
            }
            if (f == Pooled) {
                step("located", [&] { GroupStep a{g}; a.loc = located; return a; }(), ok);
                step("located, no keys or offsets", [&] { GroupStep a{g}; a.loc = located; a.k = nullptr; a.off = nullptr; return a; }(), ok);
                step("null index", [&] { GroupStep a{g}; a.idx = nullptr; return a; }(), ok);
                step("bags_per_table=0", [&] { GroupStep a{g}; a.B = 0; return a; }(), ok);
            }
            if (f == Indexed) {
                step("null index", [&] { GroupStep a{g}; a.idx = nullptr; return a; }(), ok);
                step("n_grad_rows=0", [&] { GroupStep a{g}; a.rows = 0; return a; }(), ok);
                step("n_grad_rows=2^32", [&] { GroupStep a{g}; a.rows = (size_t)1 << 32; return a; }(), ok);
            }
            step("wrong optimizer", {gwrong}, ok);
            step("max_apply_batch=0", {g0}, ok);
            step("n over max_apply_batch", [&] { GroupStep a{g}; a.n = 65; return a; }(), ok);
            step("bf16-row group", {bf16_group}, ok);
            for (size_t i = 0; i < bad.size(); ++i)
                if (i == 0 || i == (size_t)f + 3) step(bad[i].first, {g}, bad[i].second);
            if (!bad.empty()) {
                step(bad[0].first + " + null grads", [&] { GroupStep a{g}; a.gr = nullptr; return a; }(), bad[0].second);
                step(bad[0].first + " + bf16-row group", {bf16_group}, bad[0].second);
                step(bad[0].first + " + max_apply_batch=0", {g0}, bad[0].second);
                if (f == Pooled) step(bad[0].first + " + null index", [&] { GroupStep a{g}; a.idx = nullptr; return a; }(), bad[0].second);
                if (f == Indexed) step(bad[0].first + " + n_grad_rows=0", [&] { GroupStep a{g}; a.rows = 0; return a; }(), bad[0].second);
            }
            if (f == Pooled) step("null index + null group", [&] { GroupStep a{nullptr}; a.idx = nullptr; return a; }(), ok);
        }

        mee_mixed_group *one = mixed({table(16, kind), table(16, kind)}, 64), *two = mixed({table(8, kind), table(16, kind)}, 64);
        mee_mixed_group *mwrong = mixed({table(8, other), table(16, other)}, 64), *m0 = mixed({table(8, kind), table(16, kind)}, 0);
        const std::string e = std::string("mee_mixed_group_apply_") + kind_name(kind) + "_pooled";
        for (auto& m : {std::make_pair("one class", one), std::make_pair("two classes", two)}) {
            const bool first = m.second == one;
            auto step = [&](const std::string& what, MixedStep a, const Scalars& s) { CASE((e + " " + m.first + " " + what).c_str(), mixed_step(kind, a, s)); };
            step("by key", {m.second}, ok);
            step("located", [&] { MixedStep a{m.second}; a.loc = located; return a; }(), ok);
            step("located, no keys or offsets", [&] { MixedStep a{m.second}; a.loc = located; a.k = nullptr; a.off = nullptr; return a; }(), ok);
            step("n=0", [&] { MixedStep a{m.second}; a.k = nullptr; a.gr = nullptr; a.bag = nullptr; a.n = 0; return a; }(), ok);
            step("null keys", [&] { MixedStep a{m.second}; a.k = nullptr; return a; }(), ok);
            step("null bag index", [&] { MixedStep a{m.second}; a.bag = nullptr; return a; }(), ok);
            if (first) {
                step("null offsets", [&] { MixedStep a{m.second}; a.off = nullptr; return a; }(), ok);
                step("null grads", [&] { MixedStep a{m.second}; a.gr = nullptr; return a; }(), ok);
                step("bags_per_table=0", [&] { MixedStep a{m.second}; a.B = 0; return a; }(), ok);
            }
            step("n over max_apply_batch", [&] { MixedStep a{m.second}; a.n = 65; return a; }(), ok);
            for (size_t i = 0; i < bad.size(); ++i)
                if (first || i == 0) step(bad[i].first, {m.second}, bad[i].second);
            if (!bad.empty()) step(bad[0].first + " + null grads", [&] { MixedStep a{m.second}; a.gr = nullptr; return a; }(), bad[0].second);
        }
        CASE((e + " null group").c_str(), mixed_step(kind, {nullptr}, ok));
        CASE((e + " wrong optimizer").c_str(), mixed_step(kind, {mwrong}, ok));
        CASE((e + " max_apply_batch=0").c_str(), mixed_step(kind, {m0}, ok));
        CASE((e + " wrong optimizer + n over max_apply_batch").c_str(), mixed_step(kind, [&] { MixedStep a{mwrong}; a.n = 65; return a; }(), ok));
        if (!bad.empty()) CASE((e + " " + bad[0].first + " + wrong optimizer").c_str(), mixed_step(kind, {mwrong}, bad[0].second));
    }
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: host_transcript LOGFILE\n"); return 2; }
    g_log = argv[1];
    setenv("MEE_STUB_LAUNCH_LOG", g_log, 1);
    setenv("MEE_ROCTX", "0", 1);
    pooled_tables();
    pooled_groups();
    pooled_mixed();
    steps();
    return 0;   // (tables and groups live until the process ends)
}
