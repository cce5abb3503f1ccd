// sharded_mp_test.cpp — the row-sharded table through the C-ABI with G > 1 ranks, from plain C++ (no Python, no torch).
//
// usage: sharded_mp_test [G] [threads]        (default 2 ranks, one process each)
// `threads`: the G ranks are THREADS of this one process, every one with a context, a table and a communicator handle of its own on device 0 (the stand-in
// for librccl keeps its group state per thread) — how G = 8, the node's GPU count, runs on a box that lets one job keep at most 6 processes on its card.
// The parent forks G rank processes BEFORE any HIP call (a forked child of a process that has initialised HIP is unusable); rank r uses
// device r when the box has >= G GPUs (then the library binds the real RCCL: ranks exchange over xGMI), else every rank uses device 0 and
// the environment must name a stand-in for librccl in MEE_RCCL_LIB (RCCL itself refuses several ranks on one device; the test suite's
// tests/cabi/fake_rccl.cpp carries ncclSend/ncclRecv through shared memory).  Rank 0 makes the ncclUniqueId and hands it to the others
// through a shared page.
//
// Sequence per rank (every mee_sharded_* call is collective): insert its slice of N keys with key-derived rows -> size == N -> find a
// permutation of ALL keys (+ absent ones) -> one sparse-Adagrad step on its slice -> find again and compare with the update computed on the
// host -> a SKEWED step (a quarter of the slice twice more, with other gradients: with MEE_SHARDED_DEDUP the rank sends one summed row per distinct key) ->
// remove half of its slice -> size, found masks.  Twice: exact segments, and padded segments with pre-exchange dedup (mee_sharded_create_ex).
// Then the same two layouts on a sparse-Adam table (adam_table): two mee_sharded_apply_adam steps, the second with other betas and eps and with
// contributions to one key from two ranks, checked (values, m and v) against SparseAdam computed in double on the host.
// Exit code 0 = every rank passed.
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
#include <hip/hip_runtime.h>

#include <sys/mman.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "meepo_embedding.h"

#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "[rank %d] %s: %s\n", g_rank, #x, hipGetErrorString(e_)); return 2; } } while (0)
#define MEECK(x) do { int rc_ = (x); if (rc_ != MEE_OK) { fprintf(stderr, "[rank %d] %s -> %d: %s\n", g_rank, #x, rc_, mee_last_error()); return 3; } } while (0)
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "[rank %d] CHECK failed: %s (line %d)\n", g_rank, #c, __LINE__); return 4; } } while (0)

static thread_local int g_rank = -1;
// read in main() before any rank starts: the ROCm runtime and the libraries it loads may call setenv while rank threads run
static bool g_rccl_stand_in = false;
static uint64_t mix64(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31; return x; }
static float row_value(int64_t key, int j, uint64_t seed) { return (float)(mix64((uint64_t)key ^ mix64(seed + j)) >> 40) * 0x1p-24f - 0.5f; }

struct Shared {            // one page shared by the parent and the ranks
    volatile int id_ready;
    char id[MEE_COMM_ID_BYTES];
};

template <typename T> struct Dev {
    T* p = nullptr;
    explicit Dev(size_t n) { if (hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)) != hipSuccess) p = nullptr; }
    ~Dev() { if (p) (void)hipFree(p); }
    void up(const std::vector<T>& h) { (void)hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice); }
    std::vector<T> down(size_t m) const { std::vector<T> h(m); (void)hipMemcpy(h.data(), p, m * sizeof(T), hipMemcpyDeviceToHost); return h; }
};

// SparseAdam in double (SPEC.md §4): one key's element over two steps.  m, v start at 0; g2 is the sum of step 2's contributions (their |.| summed
// in g2abs: the scale of what rounding a partial sum may change); every result carries the scale its fp32 computation rounds relative to.
struct AdamStep { float lr, beta1, beta2, eps; int t; };
struct AdamRef { double w, m, v, w_scale, m_scale, v_scale; };
static AdamRef adam_ref(double w0, double g1, double g2, double g2abs, const AdamStep& s1, const AdamStep& s2) {
    auto lr_t = [](const AdamStep& s) { return (double)s.lr * std::sqrt(1.0 - std::pow((double)s.beta2, s.t)) / (1.0 - std::pow((double)s.beta1, s.t)); };
    const double a1 = 1.0 - (double)s1.beta1, b1 = 1.0 - (double)s1.beta2, a2 = 1.0 - (double)s2.beta1, b2 = 1.0 - (double)s2.beta2;
    const double m1 = a1 * g1, v1 = b1 * g1 * g1;
    const double d1 = lr_t(s1) * m1 / (std::sqrt(v1) + (double)s1.eps);            // eps outside the square root, on the uncorrected v
    const double m2 = (double)s2.beta1 * m1 + a2 * g2, v2 = (double)s2.beta2 * v1 + b2 * g2 * g2;
    const double den2 = std::sqrt(v2) + (double)s2.eps, d2 = lr_t(s2) * m2 / den2;
    AdamRef r;
    r.w = w0 - d1 - d2; r.m = m2; r.v = v2;
    r.m_scale = (double)s2.beta1 * std::fabs(m1) + a2 * g2abs;
    r.v_scale = (double)s2.beta2 * v1 + b2 * g2abs * g2abs;
    r.w_scale = std::fabs(w0) + std::fabs(d1) + lr_t(s2) * r.m_scale / den2;
    return r;
}

// Sparse Adam across the shards, exact segments (variant 0) or padded segments + pre-exchange aggregation (variant 1).  Every rank inserts its slice,
// step 1 applies the slice once (defaults, t = 1), step 2 (t = 2, beta1 0.8, beta2 0.99, eps 1e-4: eps is then a fifth of sqrt(v), so where it sits
// shows) sends the slice again, its first eighth a second time (an in-rank duplicate: Adam's pairs travel un-aggregated even under MEE_SHARDED_DEDUP) and the
// first quarter of the NEXT rank's slice: those keys are reduced from two ranks' pairs at their owner.  Then every rank reads its slice's rows through
// the sharded find and m, v of every key its own shard holds (mee_find_plane), all against adam_ref.
static int adam_table(int rank, int G, void* comm, int device, const std::vector<int64_t>& all, size_t N, size_t n_abs, int variant) {
    const uint32_t dim = 64;
    const size_t per = N / G;
    auto slice_lo = [&](int r) { return (size_t)r * per; };
    auto slice_cnt = [&](int r) { return r == G - 1 ? N - (size_t)r * per : per; };
    const AdamStep s1{0.01f, 0.9f, 0.999f, 1e-8f, 1}, s2{0.005f, 0.8f, 0.99f, 1e-4f, 2};
    auto g1_of = [](int64_t k, uint32_t j) { return 0.02f * row_value(k, (int)j, 6); };
    auto ga_of = [](int64_t k, uint32_t j) { return 0.02f * row_value(k, (int)j, 8); };                 // step 2, the slice's own pair
    auto gb_of = [](int64_t k, uint32_t j) { return 0.02f * row_value(k, (int)j, 9); };                 // step 2, the in-rank duplicate
    auto gc_of = [](int64_t k, uint32_t j, int src) { return 0.02f * row_value(k, (int)j, 10 + src); };  // step 2, from the previous rank
    mee_config c{};
    c.struct_size = sizeof c; c.device = device; c.capacity = (uint64_t)(N / G * 2.0); c.dim = dim; c.optimizer = MEE_OPT_ADAM;
    c.max_batch = 2 * (N + n_abs); c.default_value = -3.0f;
    mee_table* table = nullptr;
    MEECK(mee_table_create(&c, &table));
    mee_sharded_options o{};
    o.struct_size = sizeof o; o.max_batch = N + n_abs; o.pad_slack = variant ? 1.5 : 0.0; o.flags = variant ? MEE_SHARDED_DEDUP : 0u;
    mee_sharded* s = nullptr;
    MEECK(mee_sharded_create_ex(table, comm, &o, &s));

    const size_t lo = slice_lo(rank), cnt = slice_cnt(rank);
    const int next = (rank + 1) % G;
    const size_t n_dup = cnt / 8, n_next = G > 1 ? slice_cnt(next) / 4 : 0, n2 = cnt + n_dup + n_next;
    CHECK(n2 <= N + n_abs);
    std::vector<int64_t> k2(n2);
    std::vector<float> rows(cnt * dim), g1(cnt * dim), g2(n2 * dim);
    for (size_t i = 0; i < n2; ++i) {
        const bool own = i < cnt + n_dup;
        k2[i] = own ? all[lo + (i < cnt ? i : i - cnt)] : all[slice_lo(next) + (i - cnt - n_dup)];
        for (uint32_t j = 0; j < dim; ++j) g2[i * dim + j] = i < cnt ? ga_of(k2[i], j) : own ? gb_of(k2[i], j) : gc_of(k2[i], j, rank);
    }
    for (size_t i = 0; i < cnt; ++i)
        for (uint32_t j = 0; j < dim; ++j) { rows[i * dim + j] = row_value(all[lo + i], (int)j, 2); g1[i * dim + j] = g1_of(all[lo + i], j); }
    Dev<int64_t> d_k2(n2), d_all(N); Dev<float> d_rows(cnt * dim), d_g1(cnt * dim), d_g2(n2 * dim), d_out(N * dim); Dev<uint8_t> d_f(N);
    CHECK(d_k2.p && d_all.p && d_rows.p && d_g1.p && d_g2.p && d_out.p && d_f.p);
    d_k2.up(k2); d_rows.up(rows); d_g1.up(g1); d_g2.up(g2);
    d_all.up(std::vector<int64_t>(all.begin(), all.begin() + N));
    const int64_t* d_mine = d_k2.p;   // (the first cnt keys of the step-2 batch are the slice itself)
    MEECK(mee_sharded_insert(s, d_mine, d_rows.p, cnt, nullptr));
    MEECK(mee_sharded_apply_adam(s, d_mine, d_g1.p, cnt, s1.lr, s1.beta1, s1.beta2, s1.eps, (uint64_t)s1.t, nullptr));
    MEECK(mee_sharded_apply_adam(s, d_k2.p, d_g2.p, n2, s2.lr, s2.beta1, s2.beta2, s2.eps, (uint64_t)s2.t, nullptr));
    size_t total = 0;
    MEECK(mee_sharded_size(s, &total, nullptr));   // a collective after the apply: every rank's pairs have been applied before anybody looks
    CHECK(total == N);

    // the reference of global key i (slice sl, position li in it)
    auto ref_of = [&](size_t i, uint32_t j) {
        int sl = (int)(i / per); if (sl > G - 1) sl = G - 1;
        const size_t li = i - slice_lo(sl), cs = slice_cnt(sl);
        const int64_t k = all[i];
        double g2s = ga_of(k, j), g2abs = std::fabs(g2s);
        if (li < cs / 8) { const double b = gb_of(k, j); g2s += b; g2abs += std::fabs(b); }
        const int prev = (sl + G - 1) % G;
        if (G > 1 && li < cs / 4) { const double x = gc_of(k, j, prev); g2s += x; g2abs += std::fabs(x); }
        return adam_ref(row_value(k, (int)j, 2), g1_of(k, j), g2s, g2abs, s1, s2);
    };
    MEECK(mee_sharded_find(s, d_mine, cnt, d_out.p, d_f.p, nullptr));
    HIPCK(hipDeviceSynchronize());
    auto out = d_out.down(cnt * dim); auto f = d_f.down(cnt);
    for (size_t i = 0; i < cnt; ++i) {
        CHECK(f[i] == 1);
        for (uint32_t j = 0; j < dim; ++j) {
            const AdamRef r = ref_of(lo + i, j);
            CHECK(std::fabs(out[i * dim + j] - r.w) <= 1e-6 * r.w_scale + 1e-9);
        }
    }
    // m and v of what this shard holds: every key of ALL slices is looked up in the local table, the ones it owns are found
    size_t local = 0, seen = 0;
    MEECK(mee_size(table, &local, nullptr));
    for (uint32_t plane = 1; plane <= 2; ++plane) {
        MEECK(mee_find_plane(table, plane, d_all.p, N, d_out.p, d_f.p, nullptr));
        HIPCK(hipDeviceSynchronize());
        out = d_out.down(N * dim); f = d_f.down(N);
        seen = 0;
        for (size_t i = 0; i < N; ++i) {
            if (!f[i]) continue;
            ++seen;
            for (uint32_t j = 0; j < dim; ++j) {
                const AdamRef r = ref_of(i, j);
                const double x = out[i * dim + j];
                if (plane == 1) CHECK(std::fabs(x - r.m) <= 1e-6 * r.m_scale + 1e-15);
                else CHECK(std::fabs(x - r.v) <= 1e-6 * r.v_scale + 1e-20);
            }
        }
        CHECK(seen == local && local > N / G / 2);
    }
    uint32_t bits = 7;
    MEECK(mee_sharded_status(s, &bits, nullptr));
    CHECK(bits == 0);
    MEECK(mee_status(table, &bits, nullptr));
    CHECK(bits == 0);
    MEECK(mee_sharded_destroy(s));
    MEECK(mee_table_destroy(table));
    return 0;
}

static int run_rank(int rank, int G, Shared* sh) {
    g_rank = rank;
    int ndev = 0;
    HIPCK(hipGetDeviceCount(&ndev));
    CHECK(ndev >= 1);
    const int device = ndev >= G ? rank : 0;
    if (ndev < G && !g_rccl_stand_in) {
        fprintf(stderr, "[rank %d] %d ranks on %d GPU(s) need MEE_RCCL_LIB (a stand-in for librccl: RCCL refuses several ranks per device)\n", rank, G, ndev);
        return 5;
    }
    HIPCK(hipSetDevice(device));
    if (rank == 0) {
        MEECK(mee_comm_unique_id(sh->id));
        __sync_synchronize();
        sh->id_ready = 1;
    } else {
        for (int spins = 0; !sh->id_ready; ++spins) { if (spins > 600000) { fprintf(stderr, "[rank %d] no communicator id after 60 s\n", rank); return 6; } usleep(100); }
        __sync_synchronize();
    }
    void* comm = nullptr;
    MEECK(mee_comm_create(sh->id, (uint32_t)G, (uint32_t)rank, device, &comm));

    const uint32_t dim = 64;
    const size_t N = 60000, per = N / G, n_abs = 500;
    const float lr = 0.05f, eps = 1e-10f, acc0 = 0.1f;
    std::vector<int64_t> all(N + n_abs);
    for (size_t i = 0; i < N + n_abs; ++i) all[i] = (int64_t)mix64(11 + (i + 1) * 0x9E3779B97F4A7C15ull);   // the last n_abs are never inserted
    const size_t lo = (size_t)rank * per, cnt = rank == G - 1 ? N - lo : per;

    for (int variant = 0; variant < 2; ++variant) {
        mee_config c{};
        c.struct_size = sizeof c; c.device = device; c.capacity = (uint64_t)(N / G * 2.0); c.dim = dim; c.optimizer = MEE_OPT_ADAGRAD;
        c.max_batch = 2 * (N + n_abs); c.default_value = -3.0f; c.initial_accumulator = acc0;
        mee_table* table = nullptr;
        MEECK(mee_table_create(&c, &table));
        mee_sharded_options o{};
        o.struct_size = sizeof o; o.max_batch = N + n_abs; o.pad_slack = variant ? 1.5 : 0.0; o.flags = variant ? MEE_SHARDED_DEDUP : 0u;
        mee_sharded* s = nullptr;
        MEECK(mee_sharded_create_ex(table, comm, &o, &s));
        uint32_t gg = 0, rr = 99; uint64_t seg = 0;
        MEECK(mee_sharded_info(s, &gg, &rr, &seg));
        CHECK(gg == (uint32_t)G && rr == (uint32_t)rank && (seg != 0) == (variant == 1));

        // ---- insert my slice ----
        std::vector<int64_t> mine(all.begin() + lo, all.begin() + lo + cnt);
        std::vector<float> rows(cnt * dim), grads(cnt * dim);
        for (size_t i = 0; i < cnt; ++i)
            for (uint32_t j = 0; j < dim; ++j) { rows[i * dim + j] = row_value(mine[i], (int)j, 2); grads[i * dim + j] = 0.02f * row_value(mine[i], (int)j, 6); }
        Dev<int64_t> d_mine(cnt); Dev<float> d_rows(cnt * dim), d_grads(cnt * dim);
        CHECK(d_mine.p && d_rows.p && d_grads.p);
        d_mine.up(mine); d_rows.up(rows); d_grads.up(grads);
        MEECK(mee_sharded_insert(s, d_mine.p, d_rows.p, cnt, nullptr));
        size_t total = 0;
        MEECK(mee_sharded_size(s, &total, nullptr));
        CHECK(total == N);
        size_t local = 0;
        MEECK(mee_size(table, &local, nullptr));
        CHECK(local > N / G / 2 && local < N / G * 2);   // the keys spread over the shards

        // ---- find a permutation of ALL keys, the absent ones in between, and a few duplicates ----
        const size_t nq = N + n_abs;
        std::vector<int64_t> q(nq);
        for (size_t i = 0; i < nq; ++i) q[i] = all[(i * 7919 + (size_t)rank * 13) % nq];
        for (size_t i = 0; i < 200; ++i) q[i * 3 + 1] = q[7];   // duplicates of one key
        Dev<int64_t> d_q(nq); Dev<float> d_out(nq * dim); Dev<uint8_t> d_f(nq);
        CHECK(d_q.p && d_out.p && d_f.p);
        d_q.up(q);
        MEECK(mee_sharded_find(s, d_q.p, nq, d_out.p, d_f.p, nullptr));
        HIPCK(hipDeviceSynchronize());
        auto out = d_out.down(nq * dim); auto f = d_f.down(nq);
        // (which keys are stored: index in `all` below N)
        for (size_t i = 0; i < nq; ++i) {
            size_t idx = (i * 7919 + (size_t)rank * 13) % nq;
            if (i % 3 == 1 && i / 3 < 200) idx = (7 * 7919 + (size_t)rank * 13) % nq;
            const bool stored = idx < N;
            CHECK(f[i] == (stored ? 1 : 0));
            for (uint32_t j = 0; j < dim; j += 7) CHECK(out[i * dim + j] == (stored ? row_value(all[idx], (int)j, 2) : -3.0f));
        }

        // ---- one sparse-Adagrad step on my slice; every key is updated exactly once (the slices are disjoint) ----
        MEECK(mee_sharded_apply_adagrad(s, d_mine.p, d_grads.p, cnt, lr, eps, nullptr));
        MEECK(mee_sharded_size(s, &total, nullptr));   // a collective after the apply: every rank's pairs have been applied before anybody looks
        MEECK(mee_sharded_find(s, d_mine.p, cnt, d_out.p, d_f.p, nullptr));
        HIPCK(hipDeviceSynchronize());
        out = d_out.down(cnt * dim); f = d_f.down(cnt);
        for (size_t i = 0; i < cnt; ++i) {
            CHECK(f[i] == 1);
            for (uint32_t j = 0; j < dim; j += 5) {
                const float g = grads[i * dim + j], an = fmaf(g, g, acc0), qv = g / (sqrtf(an) + eps), w = fmaf(-lr, qv, rows[i * dim + j]);
                CHECK(fabsf(out[i * dim + j] - w) <= 1e-6f * fabsf(w) + 1e-9f);
            }
        }

        // ---- a skewed step: the first quarter of my slice THREE times in one batch (gradients g, 2g and -g/2: their sum is 2.5 g), the rest once.  The
        // dedup context adds a key's three rows up on this rank before they travel; the owner applies one update per key either way ----
        {
            const size_t quarter = cnt / 4, n2 = cnt + 2 * quarter;
            std::vector<int64_t> k2(mine);
            std::vector<float> g2(grads);
            k2.insert(k2.end(), mine.begin(), mine.begin() + quarter); k2.insert(k2.end(), mine.begin(), mine.begin() + quarter);
            g2.resize(n2 * dim);
            for (size_t i = 0; i < quarter; ++i)
                for (uint32_t j = 0; j < dim; ++j) { g2[(cnt + i) * dim + j] = 2.0f * grads[i * dim + j]; g2[(cnt + quarter + i) * dim + j] = -0.5f * grads[i * dim + j]; }
            Dev<int64_t> d_k2(n2); Dev<float> d_g2(n2 * dim);
            CHECK(d_k2.p && d_g2.p);
            d_k2.up(k2); d_g2.up(g2);
            MEECK(mee_sharded_apply_adagrad(s, d_k2.p, d_g2.p, n2, lr, eps, nullptr));
            MEECK(mee_sharded_size(s, &total, nullptr));
            MEECK(mee_sharded_find(s, d_mine.p, cnt, d_out.p, d_f.p, nullptr));
            HIPCK(hipDeviceSynchronize());
            out = d_out.down(cnt * dim);
            for (size_t i = 0; i < cnt; ++i)
                for (uint32_t j = 0; j < dim; j += 5) {
                    const float g = grads[i * dim + j], a1 = fmaf(g, g, acc0), w1 = fmaf(-lr, g / (sqrtf(a1) + eps), rows[i * dim + j]);   // after the first step
                    const float gs = i < quarter ? (float)((double)g + (double)(2.0f * g) + (double)(-0.5f * g)) : g;
                    const float a2 = fmaf(gs, gs, a1), w2 = fmaf(-lr, gs / (sqrtf(a2) + eps), w1);
                    CHECK(fabsf(out[i * dim + j] - w2) <= 2e-6f * fabsf(w2) + 1e-9f);
                }
        }

        // ---- remove the first half of my slice ----
        const size_t half = cnt / 2;
        MEECK(mee_sharded_remove(s, d_mine.p, half, d_f.p, nullptr));
        HIPCK(hipDeviceSynchronize());
        f = d_f.down(half);
        for (size_t i = 0; i < half; ++i) CHECK(f[i] == 1);
        MEECK(mee_sharded_size(s, &total, nullptr));
        size_t removed = 0;
        for (int r2 = 0; r2 < G; ++r2) removed += ((r2 == G - 1 ? N - (size_t)r2 * per : per)) / 2;
        CHECK(total == N - removed);
        MEECK(mee_sharded_find(s, d_mine.p, cnt, d_out.p, d_f.p, nullptr));
        HIPCK(hipDeviceSynchronize());
        f = d_f.down(cnt);
        for (size_t i = 0; i < cnt; ++i) CHECK(f[i] == (i < half ? 0 : 1));
        uint32_t bits = 7;
        MEECK(mee_sharded_status(s, &bits, nullptr));
        CHECK(bits == 0);
        MEECK(mee_status(table, &bits, nullptr));
        CHECK(bits == 0);
        MEECK(mee_sharded_destroy(s));
        MEECK(mee_table_destroy(table));
    }
    for (int variant = 0; variant < 2; ++variant)
        if (int rc = adam_table(rank, G, comm, device, all, N, n_abs, variant)) return rc;
    MEECK(mee_comm_destroy(comm));
    return 0;
}

// a crash of this program must say where: the test runner only sees the exit status otherwise
static void on_crash(int sig) {
    void* frames[48];
    const int n = backtrace(frames, 48);
    const char msg[] = "sharded_mp_test: fatal signal, backtrace:\n";
    (void)!write(2, msg, sizeof msg - 1);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}

int main(int argc, char** argv) {
    signal(SIGSEGV, on_crash); signal(SIGBUS, on_crash); signal(SIGABRT, on_crash); signal(SIGFPE, on_crash);
    setvbuf(stdout, nullptr, _IONBF, 0);
    const int G = argc > 1 ? atoi(argv[1]) : 2;
    const bool threads = argc > 2 && !strcmp(argv[2], "threads");
    g_rccl_stand_in = getenv("MEE_RCCL_LIB") != nullptr;
    if (G < 1 || G > 8) { fprintf(stderr, "usage: sharded_mp_test [G = 1..8] [threads]\n"); return 64; }
    Shared* sh = (Shared*)mmap(nullptr, 4096, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_ANONYMOUS, -1, 0);
    if (sh == MAP_FAILED) { perror("mmap"); return 65; }
    memset((void*)sh, 0, sizeof *sh);
    if (threads) {   // one process, G rank threads
        std::vector<int> rcs(G, 0);
        std::vector<std::thread> ts;
        for (int r = 0; r < G; ++r) ts.emplace_back([&, r] { rcs[r] = run_rank(r, G, sh); });
        for (auto& t : ts) t.join();
        int worst = 0;
        for (int rc : rcs) if (rc > worst) worst = rc;
        if (worst == 0) printf("sharded_mp_test ok: %d rank THREADS through mee_sharded_* (exact segments; padded segments + pre-exchange dedup; Adagrad and Adam)\n", G);
        return worst;
    }
    std::vector<pid_t> kids;
    for (int r = 0; r < G; ++r) {   // fork first, HIP later: nothing in this process has touched the GPU
        const pid_t pid = fork();
        if (pid < 0) { perror("fork"); return 66; }
        if (pid == 0) _exit(run_rank(r, G, sh));
        kids.push_back(pid);
    }
    int worst = 0;
    for (pid_t pid : kids) {
        int st = 0;
        if (waitpid(pid, &st, 0) < 0) { worst = 67; continue; }
        const int rc = WIFEXITED(st) ? WEXITSTATUS(st) : 128 + (WIFSIGNALED(st) ? WTERMSIG(st) : 0);
        if (rc > worst) worst = rc;
    }
    if (worst == 0) printf("sharded_mp_test ok: %d ranks through mee_sharded_* (exact segments; padded segments + pre-exchange dedup; Adagrad and Adam)\n", G);
    return worst;
}
