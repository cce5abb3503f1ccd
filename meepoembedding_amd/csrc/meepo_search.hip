// meepo_search.hip — exact top-k inner-product search over a table's live rows (SPEC.md §3 "Search"): "which keys match this query vector best", answered
// by a brute-force scan of the table in place — no [N, dim] copy, never stale.  score(q, key) = sum_j bf16(q_j) * bf16(row_j), products exact, fp32 sum.
//
// Launches (DESIGN.md §4 "Search").
//   scan     search_scan_kernel<KS, ROWS>, KS = dim / 16: a persistent grid of ONE-WAVE blocks, each over a contiguous range of 32-slot steps.  Per
//            step: the 32 keys by one coalesced load (asked for one step ahead), a ballot for the live mask (a step without a live slot is skipped),
//            the live rows straight from the row plane into the B operand of v_mfma_f32_32x32x16_bf16 — lane l holds 8 consecutive elements of row
//            l & 31 at column 16 s + 8 (l >> 5) for k-step s: one 16-byte load of a bf16 row, two and a round-and-pack of an fp32 row; a dead lane loads
//            nothing and feeds zeros.  The A operand — the queries, rounded once — is staged in LDS in fragment order (lane-linear 16-byte reads, no
//            bank conflict) once per block; a row block of 32 queries is KS matrix instructions, and row blocks beyond the first reuse the step's B.
//            The 16 accumulators of a lane are 16 queries' scores of the lane's slot.  Selection per query in LDS: the score of the current k-th best
//            (one compare per accumulator on the hot path), its exact image and key (the contract's total order, for the rare lane that passes), a
//            buffer of 2 max(k, 8) candidates and its counter.  Lanes that beat the threshold append by ballot ranks — a block is one wave, so there is
//            no atomic and no barrier instruction; a full buffer is pruned to its best k by an in-wave bitonic sort, which raises the threshold.
//            At the end the block writes its best k per query, sorted, to workspace[block][query][k].
//   merge    search_merge_kernel, one wave per query: the running best k as one entry per lane; the heads of 64 lists are read by one load, a list
//            whose head does not beat the current k-th is never touched, the others fold in by a bitonic merge of 128.  It writes the padded tail itself.
//   batched  mee_search_batch, any number of queries in one call: the queries in tiles of one row block, search_batch_scan_kernel<KS, ROWS, METRIC,
//            FILTER> — the same scan body, one (tile, step range) pair per one-wave block — first over a prefix of the slots (the seed pass), search_seed_merge_kernel for each
//            query's best k of the prefix, then over the rest with every threshold starting at the prefix's k-th entry, and the merge above with
//            the seed as one more list.
//   cosine   mee_search_metric(MEE_METRIC_COSINE): the batched launches with search_batch_scan_kernel<.., MEE_METRIC_COSINE> — the row norm from the B registers
//            (one square root per lane and step), the query norms in LDS, a widened product threshold on the hot path and the exact four-operation
//            score on the rare one (DESIGN.md §4 "Search", "Metric").  The inner-product instances do not change by it.
//   wide     256 < dim <= MEE_SEARCH_MAX_DIM, the batched entry points only: search_wide_scan_kernel<ROWS, METRIC, FILTER> in the batched launches' place — a row
//            walked in chunks of 256 columns into the same 16 accumulators, one row block of at most 32 queries per block, the absent queries of a
//            tile not staged (DESIGN.md §4 "Search", "Wide rows").  The selection, the seed pass and the merges are the ones above.
//   exclude  mee_search_filtered, "the best k except these": search_exclude_prepare_kernel sorts each exclude row into the workspace (an LDS bitonic sort,
//            one block a row), then the batched launches with the FILTER instances of the two scan kernels — a lane that is about to append first looks
//            its key up in its query's sorted row by a lower-bound search in global memory (DESIGN.md §4 "Search", "Exclusion").  The hot path, the
//            merges and every unfiltered instance do not change by it.
//   groups   mee_group_search, every member of a table group against its own queries in three launches whatever the number of members:
//            group_search_plan_kernel (one block: the members' steps from the group's device descriptors, ONE step length for the collection, each
//            member's ranges as a prefix array), search_group_scan_kernel<KS, ROWS, METRIC> / search_group_wide_scan_kernel<ROWS, METRIC> — the scan
//            bodies above behind a decoder that finds its member by a binary search of the block's range index in that array — and
//            group_search_merge_kernel, one wave per (member, query) over the member's own lists.  No seed pass (DESIGN.md §4 "Search", "Groups").
// Only vector stores, no atomics, nothing of the table is written.
//
// The upstream snapshot has no search; the semantics are SPEC.md §3 "Search".
#include <hip/hip_runtime.h>

#include "meepo_table_int.h"
#include "meepo_mma_operand.h"

namespace mee {

constexpr uint32_t kSearchBlocksPerCU = 8;   // one-wave blocks the grid holds per CU, at most: the lists the merge reads per query
constexpr uint32_t kSearchMinCap = 8;        // a candidate buffer holds 2 max(k, kSearchMinCap) entries
static_assert(2 * MEE_SEARCH_MAX_K <= 128, "a prune sorts a buffer as two entries per lane");
__host__ __device__ constexpr uint32_t search_cap(uint32_t k) { return 2 * (k < kSearchMinCap ? kSearchMinCap : k); }

// The bytes of a block's selection state in LDS (SearchSel below; search_sel_at lays the same regions out in this order): nq queries with a buffer of
// search_cap(k) candidates each — a key and an image per candidate — and the per-query words, padded to qp queries: the k-th best's key, image and
// score, and the buffer's counter; `norms`: one more word, the query's norm (the cosine scan; the wide scan keeps the room whatever its metric).
// Every byte count of the host, every tile rule and every LDS budget below comes from here.
__host__ __device__ constexpr size_t search_sel_bytes(size_t nq, size_t qp, uint32_t k, bool norms) {
    return nq * search_cap(k) * sizeof(int64_t)      // buf_key
           + qp * sizeof(int64_t)                    // thr_key
           + nq * search_cap(k) * sizeof(uint32_t)   // buf_img
           + qp * sizeof(uint32_t)                   // thr_img
           + qp * sizeof(float)                      // thr_sc
           + qp * sizeof(uint32_t)                   // cnt
           + (norms ? qp * sizeof(float) : 0);       // qn
}
// the byte counts the layout has had since the first scan: 12 per candidate, 20 per padded query, 24 with a norm
static_assert(search_sel_bytes(1, 0, MEE_SEARCH_MAX_K, false) == search_cap(MEE_SEARCH_MAX_K) * 12 && search_sel_bytes(0, 1, 1, false) == 20 &&
              search_sel_bytes(0, 1, 1, true) == 24, "the selection state's size is part of every tile rule and LDS budget");
__host__ __device__ constexpr size_t search_pad32(size_t nq) { return (nq + 31) / 32 * 32; }
// the LDS of the largest call: the queries (bf16) and the state of the most queries a call takes, each with the smallest buffer
static_assert(MEE_SEARCH_MAX_QUERY_ELEMS * 2 + search_sel_bytes(MEE_SEARCH_MAX_QK / kSearchMinCap, search_pad32(MEE_SEARCH_MAX_QK / kSearchMinCap), kSearchMinCap, false) <= 65536,
              "the scan's LDS budget");
// the cosine scan keeps its norms and is served in tiles of one row block at most
constexpr uint32_t kSearchCosineTileMax = 32;
static_assert(MEE_SEARCH_MAX_QUERY_ELEMS * 2 + search_sel_bytes(MEE_SEARCH_MAX_QK / kSearchMinCap, kSearchCosineTileMax, kSearchMinCap, true) <= 65536, "the cosine scan's LDS budget");

// The order-preserving integer image of a score (never NaN here; a zero comes as +0.0): greater score <=> greater image; every image is >= 0x007FFFFF
// (-inf), so 0 marks "no entry".
__device__ __forceinline__ uint32_t score_image(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float image_score(uint32_t m) { return __builtin_bit_cast(float, (m & 0x80000000u) ? (m ^ 0x80000000u) : ~m); }
// the contract's total order: greater score first, equal scores by the smaller key
__device__ __forceinline__ bool search_better(uint32_t ai, int64_t ak, uint32_t bi, int64_t bk) { return ai > bi || (ai == bi && ak < bk); }

// ---- in-wave bitonic network over 64 E entries, entry idx = lane + 64 e, best first ---------------------------------------------------------------
// One phase: the compare-exchanges of strides k2 / 2 .. 1; blocks of k2 entries come out best first where (idx & k2) == 0, worst first elsewhere.
// k2 = 64 E alone turns a bitonic sequence into a sorted one (the merge kernel).  All 64 lanes, convergent.
template <int E>
__device__ __forceinline__ void bitonic_phase(uint32_t (&img)[E], int64_t (&key)[E], int lane, int k2) {
#pragma unroll 1
    for (int j = k2 >> 1; j >= 1; j >>= 1) {
        if (j == 64) {   // E == 2, the last phase: the pair is the lane's own two entries, the lower index keeps the better
            if constexpr (E == 2) {
                if (search_better(img[1], key[1], img[0], key[0])) {
                    const uint32_t ti = img[0]; img[0] = img[1]; img[1] = ti;
                    const int64_t tk = key[0]; key[0] = key[1]; key[1] = tk;
                }
            }
            continue;
        }
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int idx = lane + 64 * e;
            const uint32_t pi = (uint32_t)__shfl_xor((int)img[e], j);
            const int64_t pk = (int64_t)__shfl_xor((long long)key[e], j);
            const bool keep_better = ((idx & j) == 0) == ((idx & k2) == 0);
            if (search_better(img[e], key[e], pi, pk) != keep_better) { img[e] = pi; key[e] = pk; }   // (identical entries: either copy)
        }
    }
}
// the first n_sort entries (a power of two, 2 .. 64 E; the others must be empty) sorted best first
template <int E>
__device__ __forceinline__ void bitonic_sort(uint32_t (&img)[E], int64_t (&key)[E], int lane, int n_sort) {
#pragma unroll 1
    for (int k2 = 2; k2 <= n_sort; k2 <<= 1) bitonic_phase<E>(img, key, lane, k2);
}

// ---- the scan's selection state of one block (= one wave), in LDS ---------------------------------------------------------------------------------
struct SearchSel {
    int64_t* buf_key;    // [nq][cap]
    int64_t* thr_key;    // [qp]  the k-th best entry's key and image (image 0: fewer than k entries so far) ...
    uint32_t* buf_img;   // [nq][cap]
    uint32_t* thr_img;   // [qp]
    float* thr_sc;       // [qp]  ... and its score: what the hot path compares against (-inf: none yet; +inf for the padding queries past nq)
    uint32_t* cnt;       // [qp]  entries in the buffer
    uint32_t k, cap;
};
// a block is one wave: LDS traffic between its lanes needs the compiler's fence and the wave's own in-order LDS queue, no barrier instruction
__device__ __forceinline__ void wave_lds_sync() { __syncthreads(); }

// query q's buffer pruned to its best min(n, k), sorted best first; with k entries the threshold is the k-th.  q is wave-uniform.
template <int E>
__device__ __forceinline__ void search_prune(const SearchSel& s, uint32_t q, int lane) {
    const uint32_t n = s.cnt[q];
    uint32_t img[E];
    int64_t key[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t idx = lane + 64 * e;
        const bool in = idx < n;
        img[e] = in ? s.buf_img[q * s.cap + idx] : 0u;
        key[e] = in ? s.buf_key[q * s.cap + idx] : kEmpty;
    }
    int n_sort = 2;
    while ((uint32_t)n_sort < n) n_sort <<= 1;   // n <= cap <= 64 E
    bitonic_sort<E>(img, key, lane, n_sort);
    const uint32_t keep = n < s.k ? n : s.k;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const uint32_t idx = lane + 64 * e;
        if (idx < keep) { s.buf_img[q * s.cap + idx] = img[e]; s.buf_key[q * s.cap + idx] = key[e]; }
    }
    if (n >= s.k && lane == (int)s.k - 1) {   // (k <= 64: the k-th entry is lane k - 1's first)
        s.thr_img[q] = img[0]; s.thr_key[q] = key[0]; s.thr_sc[q] = image_score(img[0]);
    }
    if (lane == 0) s.cnt[q] = keep;
    wave_lds_sync();
}
__device__ __forceinline__ void search_prune_any(const SearchSel& s, uint32_t q, int lane) {
    if (s.cap > 64) search_prune<2>(s, q, lane); else search_prune<1>(s, q, lane);   // wave-uniform
}

// The lanes with `beat` append (img, key) to the buffer of their half's query q (lanes 0-31 share one query, lanes 32-63 another), in lane order, by
// ballot ranks; a buffer that fills up is pruned, and what did not fit is tried again against the raised threshold.  All 64 lanes, convergent.
__device__ __forceinline__ void search_append(const SearchSel& s, uint32_t q, bool beat, uint32_t img, int64_t key, int lane) {
    const int half = lane >> 5, col = lane & 31;
    while (true) {
        const uint64_t m = __ballot(beat);
        if (!m) break;   // wave-uniform
        const uint32_t mh = (uint32_t)(m >> (32 * half));
        const uint32_t c = mh ? s.cnt[q] : 0u;   // (a half with a candidate has q < nq)
        const uint32_t room = s.cap - c;         // > 0: a buffer is pruned the moment it fills
        const uint32_t rank = __popc(mh & ((1u << col) - 1u));
        if (beat && rank < room) {
            s.buf_img[q * s.cap + c + rank] = img;
            s.buf_key[q * s.cap + c + rank] = key;
            beat = false;
        }
        const uint32_t total = __popc(mh), taken = total < room ? total : room;
        if (mh && col == 0) s.cnt[q] = c + taken;
        wave_lds_sync();
        uint64_t pm = __ballot(mh && col == 0 && c + taken >= s.cap);
        while (pm) {   // wave-uniform: at most the two halves' queries
            const int src = __ffsll((unsigned long long)pm) - 1;
            pm &= pm - 1;
            search_prune_any(s, (uint32_t)__shfl((int)q, src), lane);
        }
        if (beat) beat = search_better(img, key, s.thr_img[q], s.thr_key[q]);
    }
}

// ---- exclusion (SPEC.md §3 "Search", "Exclusion"; DESIGN.md §4 "Search", "Exclusion") ---------------------------------------------------------------
// The exclude lists as search_exclude_prepare_kernel leaves them: row r is sorted[r * ep, + count[r]), ascending; what lies behind a row's count is never
// read.  Query q of a block reads row q * per_query — the body is handed the lists of its tile's first query, or the one list of a broadcast.
struct SearchFilter {
    const int64_t* sorted;
    const uint32_t* count;
    uint32_t ep, per_query;   // ep: entries between two rows (a power of two); per_query: 1, or 0 where one row serves every query
};
// Is `key` in query q's exclude row?  A lower-bound search over the row's valid entries alone: at most 12 dependent loads and the one that compares
// (count <= MEE_SEARCH_MAX_EXCLUDE = 2^12).  Lanes diverge in here; the caller's ballots come after.
__device__ __forceinline__ bool search_excluded(const SearchFilter& f, uint32_t q, int64_t key) {
    const size_t r = (size_t)q * f.per_query;
    const int64_t* __restrict__ row = f.sorted + r * f.ep;
    const uint32_t n = f.count[r];
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && row[lo] == key;
}

// the filter as a block sees it whose first query is the call's query q0
__device__ __forceinline__ SearchFilter search_filter_at(const SearchFilter& f, uint32_t q0) {
    const size_t r = (size_t)q0 * f.per_query;
    return SearchFilter{f.sorted + r * f.ep, f.count + r, f.ep, f.per_query};
}
// what a scan kernel carries as its last parameter: the filter's words in a FILTER instance, nothing in the others
struct SearchNoFilter {};
template <bool FILTER> using SearchFilterOf = std::conditional_t<FILTER, SearchFilter, SearchNoFilter>;
__device__ __forceinline__ SearchFilter search_filter_of(const SearchFilter& f) { return f; }
__device__ __forceinline__ SearchFilter search_filter_of(const SearchNoFilter&) { return SearchFilter{}; }   // (never read: every use sits behind FILTER)

// One exclude row per block of kExcludeThreads threads: the row's n_exclude keys into LDS — an entry <= kReclaimed (it matches no live key; search's own
// padding key is one) and the padding up to `ep` as INT64_MAX — an LDS bitonic sort, ascending, over ep = next pow2(n_exclude) entries (32 KB at the most),
// and the sorted row [ep] and the count n of its valid entries to the workspace.  The n valid entries are the first n of the sorted row whatever they
// are: nothing sorts behind INT64_MAX, and an INT64_MAX among the first n is one the caller listed.  LDS (dynamic): ep x 8 B | one count per wave.
constexpr uint32_t kExcludeThreads = 256;
__global__ __launch_bounds__(kExcludeThreads) void search_exclude_prepare_kernel(const int64_t* __restrict__ exclude, uint32_t n_exclude, uint32_t ep,
                                                                                 int64_t* __restrict__ sorted, uint32_t* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char search_lds[];
    int64_t* const e = reinterpret_cast<int64_t*>(search_lds);
    uint32_t* const wave_n = reinterpret_cast<uint32_t*>(e + ep);
    const uint32_t tid = threadIdx.x, row = blockIdx.x;
    uint32_t mine = 0;
    for (uint32_t i = tid; i < ep; i += kExcludeThreads) {
        const int64_t key = i < n_exclude ? exclude[(size_t)row * n_exclude + i] : kEmpty;
        const bool valid = key > kReclaimed;
        e[i] = valid ? key : INT64_MAX;
        mine += valid;
    }
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d);
    if ((tid & 63) == 0) wave_n[tid >> 6] = mine;
    __syncthreads();
    for (uint32_t k2 = 2; k2 <= ep; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j >= 1; j >>= 1) {
            for (uint32_t p = tid; p < ep / 2; p += kExcludeThreads) {   // pair p: the entries i and i + j, i with bit j clear
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int64_t a = e[i], b = e[i + j];
                if ((a > b) == ((i & k2) == 0)) { e[i] = b; e[i + j] = a; }
            }
            __syncthreads();
        }
    }
    for (uint32_t i = tid; i < ep; i += kExcludeThreads) sorted[(size_t)row * ep + i] = e[i];
    if (tid == 0) count[row] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

// ---- cosine (SPEC.md §3 "Search", "Metric"): score = dot / (sqrtf(qq) * sqrtf(rr)), four correctly rounded fp32 operations ---------------------------
// (cosine_score and sum_squares, the arithmetic the shared-slate score uses too: meepo_mma_operand.h)
// The norms between which the hot path's product compare is argued below; a live row outside them takes the rare path every time, a query outside
// them accepts every row.
constexpr float kCosNormMin = 0x1p-50f, kCosNormMax = 0x1p50f;

// The hot path's threshold for a query whose k-th best cosine is `thr` (-inf: none yet; +inf: a padding query) and whose norm is qn: the hot path
// accepts accumulator `acc` of a row of norm rn iff  acc >= fl(pre * rn),  one multiply and one compare.  It may accept too much — the rare path
// computes the exact score and decides — but must never reject a row whose exact score s = fl(acc / d), d = fl(qn * rn), reaches thr.
// With u = 2^-24 and qn, rn in [kCosNormMin, kCosNormMax] (so d is a normal number, d = qn rn (1 + e1), |e1| <= u):
//   s >= thr  =>  acc / d >= pred(thr), the next float below thr (division rounds to nearest and is monotone)  =>  acc >= pred(thr) d.
//   P = fl(thr qn) = thr qn (1 + e3), and the compare's right side is pre rn (1 + e2); |e2|, |e3| <= u while the products are normal numbers.
//   thr > 0: pred(thr) >= thr (1 - 2u), so pred(thr) d >= thr qn rn (1 - 2u)(1 - u).  pre = fl(P (1 - 8u)) <= thr qn (1 + u)(1 - 8u)(1 + u), and
//            times (1 + u) rn that stays below thr qn rn (1 - 4u): the threshold is LOWERED, toward zero, by more than the roundings can raise it.
//   thr < 0: pred(thr) >= thr (1 + 2u) (it lies further from zero), so pred(thr) d >= thr qn rn (1 + 2u)(1 + u), and pre = fl(P (1 + 8u)) is
//            thr qn (1 + 5u) or further from zero after all three roundings: the threshold is lowered AWAY from zero.
//   |P| < 2^-60, thr = +-0 included: relative bounds end where products turn subnormal, so the threshold is the constant -2^-58: pred(thr) d
//            >= -(|thr| qn (1 + 4u) + 2^-149 2^50 (1 + u)) rn > -2^-58 rn, and -2^-58 rn is exact (rn >= 2^-50).  A positive such thr accepts acc >= ~0.
//   thr = -inf: pre = -inf accepts every row with rn > 0.  thr = +inf: pre = +inf rejects everything but acc = +inf, whose score ties it.
//   An overflowing pre rn (a threshold left by a row outside the norm range) is +inf only where the real product exceeds every finite acc, or -inf.
//   A zero row or a dead lane: the scan hands in rn = NaN (the score 0 / 0 is NaN for every query), and a NaN accumulator or norm passes no compare.
// A query of norm 0 or NaN has only NaN scores: +inf.  A query whose norm lies outside the range: -inf, every live row takes the rare path.
__device__ __forceinline__ float cosine_prefilter(float thr, float qn) {
    if (!(qn > 0.f)) return __builtin_inff();
    if (!(qn >= kCosNormMin && qn <= kCosNormMax)) return -__builtin_inff();
    const float P = thr * qn;
    if (!(__builtin_fabsf(P) >= 0x1p-60f)) return -0x1p-58f;
    return P * (P > 0.f ? 1.f - 0x1p-21f : 1.f + 0x1p-21f);
}

// ---- what the scan bodies share around their matrix instructions --------------------------------------------------------------------------------
// the selection state of nq queries, its per-query words padded to qp, from LDS at `base` (8-byte aligned), region by region in the order
// search_sel_bytes sums them: buf_key | thr_key | buf_img | thr_img | thr_sc | cnt | qn (cosine only: [qp] query norms)
__device__ __forceinline__ SearchSel search_sel_at(unsigned char* base, uint32_t nq, uint32_t qp, uint32_t k, float*& qn) {
    SearchSel s;
    s.k = k; s.cap = search_cap(k);
    s.buf_key = reinterpret_cast<int64_t*>(base);
    s.thr_key = s.buf_key + (size_t)nq * s.cap;
    s.buf_img = reinterpret_cast<uint32_t*>(s.thr_key + qp);
    s.thr_img = s.buf_img + (size_t)nq * s.cap;
    s.thr_sc = reinterpret_cast<float*>(s.thr_img + qp);
    s.cnt = reinterpret_cast<uint32_t*>(s.thr_sc + qp);
    qn = reinterpret_cast<float*>(s.cnt + qp);
    return s;
}
// empty buffers, and every threshold at its seed (search_scan_body) or at nothing; cosine: the staged norms qn[0, qp) are read
template <int METRIC>
__device__ __forceinline__ void search_sel_start(const SearchSel& s, const float* qn, uint32_t nq, uint32_t qp, const int64_t* __restrict__ seed_keys,
                                                 const uint32_t* __restrict__ seed_img, int lane) {
    const uint32_t k = s.k;
    if constexpr (METRIC == MEE_METRIC_COSINE) wave_lds_sync();
    for (uint32_t q = lane; q < qp; q += 64) {
        uint32_t ti = 0u;
        int64_t tk = kEmpty;
        if (seed_img && q < nq) { ti = seed_img[(size_t)q * k + k - 1]; tk = seed_keys[(size_t)q * k + k - 1]; }
        s.thr_key[q] = tk; s.thr_img[q] = ti; s.cnt[q] = 0u;
        const float ts = q < nq ? (ti ? image_score(ti) : -__builtin_inff()) : __builtin_inff();   // nothing beats a padding query's threshold
        if constexpr (METRIC == MEE_METRIC_COSINE) s.thr_sc[q] = cosine_prefilter(ts, qn[q]);
        else s.thr_sc[q] = ts;
    }
    wave_lds_sync();
}
// A step's 16 accumulators against the thresholds: accumulator r of lane (half, col) is query qbase + 8 (r / 4) + r % 4 (qbase = 32 rb + 4 half) against
// the lane's slot (key; cosine: of norm rn, `wild` as the scan bodies set it).  NaN passes no compare.  FILTER: a lane that would append first looks its
// key up in its query's exclude row (flt; unused otherwise) and appends only if it is absent — the hot path and the thresholds never see the filter,
// and an excluded key never raises a threshold.
template <int METRIC, bool FILTER>
__device__ __forceinline__ void search_select(const SearchSel& s, const float* qn, const f32x16& acc, uint32_t qbase, uint32_t nq, bool live, int64_t key,
                                              float rn, bool wild, int lane, [[maybe_unused]] const SearchFilter& flt) {
    const int col = lane & 31;
    uint32_t hot = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        if constexpr (METRIC == MEE_METRIC_COSINE) {   // thr_sc is cosine_prefilter's value: one multiply and one compare
            if (__ballot(live && acc[r] >= s.thr_sc[qbase + 8 * (r >> 2) + (r & 3)] * rn)) hot |= 1u << r;
        } else {
            if (__ballot(live && acc[r] >= s.thr_sc[qbase + 8 * (r >> 2) + (r & 3)])) hot |= 1u << r;
        }
    }
    if constexpr (METRIC == MEE_METRIC_COSINE) hot = wild ? 0xFFFFu : hot;
    while (hot) {   // wave-uniform, rare once the thresholds have risen
        const int r = __ffs(hot) - 1;
        hot &= hot - 1;
        float sc = acc[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) sc = r == i ? acc[i] : sc;
        if constexpr (METRIC != MEE_METRIC_COSINE) sc += 0.f;   // -0.0 -> +0.0: equal scores have one image
        const uint32_t q = qbase + 8 * (r >> 2) + (r & 3);
        if constexpr (METRIC == MEE_METRIC_COSINE) sc = cosine_score(sc, qn[q], rn);   // the exact score, its zero as +0.0 too; 0 / 0 = NaN is no candidate
        const uint32_t img = score_image(sc);
        bool beat = live && q < nq && sc == sc && search_better(img, key, s.thr_img[q], s.thr_key[q]);
        if constexpr (FILTER) {   // divergent; search_append's ballots are wave-uniform again
            if (beat) beat = !search_excluded(flt, q, key);
        }
        search_append(s, q, beat, img, key, lane);
        if constexpr (METRIC == MEE_METRIC_COSINE) {   // the thresholds a prune may have raised, as the hot path wants them (q < qp: no query's word is a stranger's)
            if (col == 0) s.thr_sc[q] = cosine_prefilter(s.thr_img[q] ? image_score(s.thr_img[q]) : -__builtin_inff(), qn[q]);
            wave_lds_sync();
        }
    }
}
// the block's best k per query, sorted, padded with the empty marker, to rows out_row0 + q of the lists
__device__ __forceinline__ void search_write_lists(const SearchSel& s, uint32_t nq, size_t out_row0, int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img,
                                                   int lane) {
    const uint32_t k = s.k;
    for (uint32_t q = 0; q < nq; ++q) {   // wave-uniform
        search_prune_any(s, q, lane);
        const uint32_t n = s.cnt[q];
        const size_t o = (out_row0 + q) * k;
        for (uint32_t i = lane; i < k; i += 64) {
            ws_img[o + i] = i < n ? s.buf_img[q * s.cap + i] : 0u;
            ws_keys[o + i] = i < n ? s.buf_key[q * s.cap + i] : kEmpty;
        }
    }
}

// ---- what a block scans (both row shapes) ---------------------------------------------------------------------------------------------------------
// The nq_all queries of a call are cut into n_tiles tiles of `tile` queries (the last one shorter), the steps [step0, step_end) into ranges of
// steps_per_range; a one-wave block serves one (tile, range) pair.  The grid is flat and the tile index varies fastest, so the blocks that walk one
// range are neighbours.  Lists: [range][nq_all][k] — a tile's block writes its own query rows of its range's list, so the merge reads every
// query's lists at one stride whatever its tile.
// The one decoder of both row shapes: it hands SCAN, the row shape's body (search_scan_body or search_wide_scan_body), the block's queries
// [q0, q0 + nq) (dim columns each), its steps [s0, s1), its seed lists and its exclude lists from q0 on, and the first row of its lists.
// seed_*: null or [nq_all][k].  flt: the lists of ALL the call's queries, or the one broadcast list (unread in an instance without FILTER).
// The two bodies share ONE signature on purpose, the narrow one's unused leading row width included: SCAN is called as a plain function with
// __restrict__ parameters, and that call — not a lambda or a struct of the values — is what keeps each kernel's machine code as it was.
template <auto SCAN>
__device__ __forceinline__ void search_scan_block(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity, uint32_t dim,
                                                  const float* __restrict__ queries, uint32_t nq_all, uint32_t tile, uint32_t n_tiles, uint32_t k,
                                                  uint64_t step0, uint64_t step_end, uint64_t steps_per_range,
                                                  const int64_t* __restrict__ seed_keys, const uint32_t* __restrict__ seed_img,
                                                  int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img, const SearchFilter& flt) {
    const uint32_t t = blockIdx.x % n_tiles, range = blockIdx.x / n_tiles;
    const uint32_t q0 = t * tile, nq = nq_all - q0 < tile ? nq_all - q0 : tile;
    uint64_t s0 = step0 + (uint64_t)range * steps_per_range, s1 = s0 + steps_per_range;
    if (s1 > step_end) s1 = step_end;
    if (s0 > s1) s0 = s1;
    SCAN(dim, tkeys, values, capacity, queries + (size_t)q0 * dim, nq, k, s0, s1, seed_keys ? seed_keys + (size_t)q0 * k : nullptr,
         seed_img ? seed_img + (size_t)q0 * k : nullptr, (size_t)range * nq_all + q0, ws_keys, ws_img, search_filter_at(flt, q0));
}

// cosine: the norm of the lane's slot from rr, its half's share of the squares of the operand registers themselves (an fp32 row after its rounding) —
// the other half's share from lane ^ 32, one square root per lane and step.  All 16 accumulators of a lane belong to this slot.
// A zero row (and a dead lane) has the score 0 / 0 = NaN for every query.  Its norm is kept as NaN, not 0: the score stays NaN, and the hot path's
// compare fails at once where  0 >= thr * 0  would send the row to the rare path at every step.
// wild: a live row of the step whose norm lies outside the product compare's range — every query looks at the step exactly.
__device__ __forceinline__ float cosine_row_norm(float rr, bool live, bool& wild) {
    rr += __shfl_xor(rr, 32);
    const float rn = rr > 0.f ? __builtin_sqrtf(rr) : __builtin_nanf("");
    wild = __ballot(live && (rn > kCosNormMax || (rn < kCosNormMin && rn > 0.f))) != 0;
    return rn;
}

// The scan of one block, rows of dim = 16 KS <= 256.
// LDS (dynamic; the host computes the same sum, search_lds_bytes): A fragments [n_rb][KS][64] x 16 B | the selection state (search_sel_at).
// METRIC == MEE_METRIC_COSINE: thr_sc holds cosine_prefilter of the threshold instead of the threshold's score.
template <int KS, int ROWS, int METRIC, bool FILTER>
__device__ __forceinline__ void search_scan_body(uint32_t /* 16 KS */, const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity,
                                                 const float* __restrict__ queries, uint32_t nq, uint32_t k, uint64_t s0, uint64_t s1,
                                                 const int64_t* __restrict__ seed_keys, const uint32_t* __restrict__ seed_img, size_t out_row0,
                                                 int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img, const SearchFilter& flt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char search_lds[];
    constexpr uint32_t dim = 16 * KS;
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const uint32_t n_rb = (nq + 31) / 32, qp = n_rb * 32;
    u32x4* const afrag = reinterpret_cast<u32x4*>(search_lds);
    [[maybe_unused]] float* qn;   // (cosine only)
    const SearchSel s = search_sel_at(search_lds + (size_t)qp * dim * 2, nq, qp, k, qn);

    // ---- the queries, rounded once, in fragment order: fragment (rb, ks) is 64 lanes x 16 bytes, lane (half, col) = query rb * 32 + col, elements as B's
    [[maybe_unused]] float qq = 0.f;
    for (uint32_t f = 0; f < n_rb * KS; ++f) {
        const uint32_t q = (f / KS) * 32 + col, ks = f % KS;
        u32x4 p = {0u, 0u, 0u, 0u};
        if (q < nq) {
            const f32x4* src = reinterpret_cast<const f32x4*>(queries + (size_t)q * dim + 16 * ks + 8 * half);
            const f32x4 x = src[0], y = src[1];
            p = u32x4{bf16x2_of(x.x, x.y), bf16x2_of(x.z, x.w), bf16x2_of(y.x, y.y), bf16x2_of(y.z, y.w)};
        }
        afrag[f * 64 + lane] = p;
        if constexpr (METRIC == MEE_METRIC_COSINE) {   // the query's norm from the rounded values: this lane's eight elements of every k-step, then the other half's
            qq = sum_squares(p, ks == 0 ? 0.f : qq);
            if (ks == KS - 1) {
                qq += __shfl_xor(qq, 32);
                if (half == 0) qn[q] = __builtin_sqrtf(qq);   // (a padding query: 0)
            }
        }
    }
    search_sel_start<METRIC>(s, qn, nq, qp, seed_keys, seed_img, lane);

    // ---- the block's steps: 32 consecutive slots each, the keys one step ahead
    int64_t key_next = kEmpty;
    if (s0 < s1 && s0 * 32 + col < capacity) key_next = __builtin_nontemporal_load(tkeys + s0 * 32 + col);
    for (uint64_t step = s0; step < s1; ++step) {   // wave-uniform
        const int64_t key = key_next;
        const uint64_t slot = step * 32 + col;
        key_next = kEmpty;
        if (step + 1 < s1 && slot + 32 < capacity) key_next = __builtin_nontemporal_load(tkeys + slot + 32);   // slots at or past capacity are never addressed
        const bool live = key > kReclaimed;
        if (!__ballot(live)) continue;   // wave-uniform
        bf16x8 b[KS];
        search_load_b<KS, ROWS>(values, slot, half, live, b);
        [[maybe_unused]] float rn = 0.f;
        [[maybe_unused]] bool wild = false;
        if constexpr (METRIC == MEE_METRIC_COSINE) {   // the lane's eight elements of every k-step
            float rr = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) rr = sum_squares(__builtin_bit_cast(u32x4, b[ks]), rr);
            rn = cosine_row_norm(rr, live, wild);
        }
        for (uint32_t rb = 0; rb < n_rb; ++rb) {
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, afrag[(rb * KS + ks) * 64 + lane]), b[ks], acc, 0, 0, 0);
            search_select<METRIC, FILTER>(s, qn, acc, rb * 32 + 4 * half, nq, live, key, rn, wild, lane, flt);
        }
    }

    search_write_lists(s, nq, out_row0, ws_keys, ws_img, lane);
}

// mee_search: all nq queries in every block, block b over steps [b, b + 1) * steps_per_block, list b
template <int KS, int ROWS>
__global__ __launch_bounds__(64) void search_scan_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity,
                                                         const float* __restrict__ queries, uint32_t nq, uint32_t k, uint64_t steps_per_block,
                                                         int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img) {
    const uint64_t n_steps = (capacity + 31) / 32;
    const uint64_t s0 = (uint64_t)blockIdx.x * steps_per_block, s1 = s0 + steps_per_block < n_steps ? s0 + steps_per_block : n_steps;
    search_scan_body<KS, ROWS, MEE_METRIC_IP, false>(16 * KS, tkeys, values, capacity, queries, nq, k, s0, s1, nullptr, nullptr, (size_t)blockIdx.x * nq, ws_keys, ws_img, SearchFilter{});
}

// flt (FILTER): the lists of ALL the call's queries, or the one broadcast list; a tile's block addresses its own rows from q0 on
template <int KS, int ROWS, int METRIC, bool FILTER>
__global__ __launch_bounds__(64) void search_batch_scan_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity,
                                                               const float* __restrict__ queries, uint32_t nq_all, uint32_t tile, uint32_t n_tiles, uint32_t k,
                                                               uint64_t step0, uint64_t step_end, uint64_t steps_per_range,
                                                               const int64_t* __restrict__ seed_keys, const uint32_t* __restrict__ seed_img,
                                                               int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img, SearchFilterOf<FILTER> flt) {
    search_scan_block<search_scan_body<KS, ROWS, METRIC, FILTER>>(tkeys, values, capacity, 16 * KS, queries, nq_all, tile, n_tiles, k, step0, step_end, steps_per_range, seed_keys,
                                                                  seed_img, ws_keys, ws_img, search_filter_of(flt));
}

// ---- wide rows, 256 < dim <= MEE_SEARCH_MAX_DIM (DESIGN.md §4 "Search", "Wide rows") -------------------------------------------------------------
// A row no longer fits the registers as one B operand, and 32 queries of it no longer fit the LDS beside the selection state.  So the row is walked
// in CHUNKS of kWideChunkKS k-steps (256 columns; the last chunk of a row may be shorter): per step a chunk of B is loaded as search_load_b loads a
// row, its matrix instructions go into the step's 16 accumulators, and only then is the next chunk asked for — one chunk of operand registers is live
// at a time (an fp32 chunk is 128 registers in flight before its packing, so a second one would leave no room for two waves per SIMD; the latency
// is left to the other waves of the CU).  A block serves ONE row block: a tile of nq <= 32 queries, B is never needed twice.  The A fragments hold
// the tile's nq queries and nothing for the absent ones: fragment (ks, half) is nq x 16 bytes, query col at [col] — lane-linear in each half — and a
// lane whose col >= nq feeds zeros without an LDS read.
// LDS: A fragments [dim / 16][2][nq] x 16 B | the selection state of nq queries, per-query words padded to 32 (search_sel_at).
constexpr uint32_t kWideLdsBudget = 40 * 1024;   // per block: four blocks share a CU's 160 KB (search_wide_tile)
__host__ __device__ constexpr uint32_t search_wide_lds_bytes(uint32_t dim, uint32_t nq, uint32_t k) { return nq * dim * 2 + (uint32_t)search_sel_bytes(nq, 32, k, true); }
// the queries of a tile: as many as the budget holds (the bytes are linear in nq), in eights (a fragment's half is then whole 128-byte rows of the
// LDS), at most one row block
__host__ __device__ constexpr uint32_t search_wide_tile(uint32_t dim, uint32_t k) {
    const uint32_t t = (kWideLdsBudget - search_wide_lds_bytes(dim, 0, k)) / (search_wide_lds_bytes(dim, 1, k) - search_wide_lds_bytes(dim, 0, k)) / 8 * 8;
    return t < 32 ? t : 32;
}
static_assert(search_wide_tile(MEE_SEARCH_MAX_DIM, MEE_SEARCH_MAX_K) >= 8, "every (dim, k) is served in tiles of at least 8 queries");

// search_scan_body for a wide row: dim is a run-time value, nq <= 32; everything else as there.
template <int ROWS, int METRIC, bool FILTER>
__device__ __forceinline__ void search_wide_scan_body(uint32_t dim, const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity,
                                                      const float* __restrict__ queries, uint32_t nq, uint32_t k, uint64_t s0, uint64_t s1,
                                                      const int64_t* __restrict__ seed_keys, const uint32_t* __restrict__ seed_img, size_t out_row0,
                                                      int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img, const SearchFilter& flt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char search_lds[];
    const int lane = threadIdx.x, half = lane >> 5, col = lane & 31;
    const uint32_t ks_all = dim / 16, n_full = ks_all / kWideChunkKS * kWideChunkKS;
    constexpr uint32_t esz = ROWS == kRowsBF16 ? 2 : 4;   // bytes of a stored element
    u32x4* const afrag = reinterpret_cast<u32x4*>(search_lds);
    [[maybe_unused]] float* qn;   // (cosine only)
    const SearchSel s = search_sel_at(search_lds + (size_t)nq * dim * 2, nq, 32, k, qn);

    // ---- the tile's queries, rounded once; a query's norm from the rounded values, a padding query's as 0
    [[maybe_unused]] float qq = 0.f;
    if ((uint32_t)col < nq) {
        const f32x4* src = reinterpret_cast<const f32x4*>(queries + (size_t)col * dim + 8 * half);
        for (uint32_t ks = 0; ks < ks_all; ++ks) {
            const f32x4 x = src[4 * ks], y = src[4 * ks + 1];
            const u32x4 p = {bf16x2_of(x.x, x.y), bf16x2_of(x.z, x.w), bf16x2_of(y.x, y.y), bf16x2_of(y.z, y.w)};
            afrag[((size_t)ks * 2 + half) * nq + col] = p;
            if constexpr (METRIC == MEE_METRIC_COSINE) qq = sum_squares(p, qq);
        }
    }
    if constexpr (METRIC == MEE_METRIC_COSINE) {
        qq += __shfl_xor(qq, 32);
        if (half == 0) qn[col] = __builtin_sqrtf(qq);
    }
    search_sel_start<METRIC>(s, qn, nq, 32, seed_keys, seed_img, lane);   // (its fence also stands between the fragments' stores and their reads)

    // ---- the block's steps, as search_scan_body walks them
    int64_t key_next = kEmpty;
    if (s0 < s1 && s0 * 32 + col < capacity) key_next = __builtin_nontemporal_load(tkeys + s0 * 32 + col);
    for (uint64_t step = s0; step < s1; ++step) {   // wave-uniform
        const int64_t key = key_next;
        const uint64_t slot = step * 32 + col;
        key_next = kEmpty;
        if (step + 1 < s1 && slot + 32 < capacity) key_next = __builtin_nontemporal_load(tkeys + slot + 32);   // slots at or past capacity are never addressed
        const bool live = key > kReclaimed;
        if (!__ballot(live)) continue;   // wave-uniform
        const unsigned char* const row = reinterpret_cast<const unsigned char*>(values) + (slot * dim + 8 * half) * esz;   // the lane's eight elements of k-step 0
        f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float rr = 0.f;
#pragma unroll 1
        for (uint32_t ks0 = 0; ks0 < n_full; ks0 += kWideChunkKS)
            search_wide_chunk<ROWS, METRIC, true>(row + (size_t)ks0 * 16 * esz, afrag, ks0, kWideChunkKS, nq, half, col, live, acc, rr);
        if (n_full < ks_all)
            search_wide_chunk<ROWS, METRIC, false>(row + (size_t)n_full * 16 * esz, afrag, n_full, (int)(ks_all - n_full), nq, half, col, live, acc, rr);
        [[maybe_unused]] float rn = 0.f;
        [[maybe_unused]] bool wild = false;
        if constexpr (METRIC == MEE_METRIC_COSINE) rn = cosine_row_norm(rr, live, wild);   // behind the last chunk
        search_select<METRIC, FILTER>(s, qn, acc, 4 * half, nq, live, key, rn, wild, lane, flt);
    }
    search_write_lists(s, nq, out_row0, ws_keys, ws_img, lane);
}

// the scan kernel of a wide row: search_batch_scan_kernel's parameters and the row width; tile <= 32
template <int ROWS, int METRIC, bool FILTER>
__global__ __launch_bounds__(64) void search_wide_scan_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t capacity, uint32_t dim,
                                                              const float* __restrict__ queries, uint32_t nq_all, uint32_t tile, uint32_t n_tiles, uint32_t k,
                                                              uint64_t step0, uint64_t step_end, uint64_t steps_per_range,
                                                              const int64_t* __restrict__ seed_keys, const uint32_t* __restrict__ seed_img,
                                                              int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img, SearchFilterOf<FILTER> flt) {
    search_scan_block<search_wide_scan_body<ROWS, METRIC, FILTER>>(tkeys, values, capacity, dim, queries, nq_all, tile, n_tiles, k, step0, step_end, steps_per_range, seed_keys,
                                                                   seed_img, ws_keys, ws_img, search_filter_of(flt));
}

// Query q's best k of n_lists sorted lists, list l at [(l * nq + q) * k, + k): lane i < k ends with entry i in (img, key), image 0 behind the real ones.
__device__ __forceinline__ void search_merge_lists(const int64_t* __restrict__ ws_keys, const uint32_t* __restrict__ ws_img, uint32_t n_lists, uint32_t nq,
                                                   uint32_t k, uint32_t q, int lane, uint32_t& best_img, int64_t& best_key) {
    uint32_t img[2] = {0u, 0u};            // [0]: the running best, entry `lane`, best first, empty behind the entries and at or past k
    int64_t key[2] = {kEmpty, kEmpty};
    uint32_t thr_i = 0u;                   // the k-th best so far (image 0: fewer than k)
    int64_t thr_k = kEmpty;
    for (uint32_t lb = 0; lb < n_lists; lb += 64) {   // wave-uniform
        uint32_t hi = 0u;
        int64_t hk = kEmpty;
        if (lb + lane < n_lists) {
            const size_t o = ((size_t)(lb + lane) * nq + q) * k;
            hi = ws_img[o]; hk = ws_keys[o];
        }
        uint64_t m = __ballot(hi != 0u && search_better(hi, hk, thr_i, thr_k));
        while (m) {   // wave-uniform
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            if (!search_better((uint32_t)__shfl((int)hi, src), (int64_t)__shfl((long long)hk, src), thr_i, thr_k)) continue;   // the threshold has risen since
            const size_t o = ((size_t)(lb + src) * nq + q) * k;
            const uint32_t i = 63 - lane;   // the list worst first behind the running best: a bitonic sequence of 128
            img[1] = i < k ? ws_img[o + i] : 0u;
            key[1] = i < k ? ws_keys[o + i] : kEmpty;
            bitonic_phase<2>(img, key, lane, 128);
            if ((uint32_t)lane >= k) { img[0] = 0u; key[0] = kEmpty; }
            thr_i = (uint32_t)__shfl((int)img[0], (int)k - 1);
            thr_k = (int64_t)__shfl((long long)key[0], (int)k - 1);
        }
    }
    best_img = img[0]; best_key = key[0];
}

__global__ __launch_bounds__(64) void search_merge_kernel(const int64_t* __restrict__ ws_keys, const uint32_t* __restrict__ ws_img, uint32_t n_lists, uint32_t nq,
                                                          uint32_t k, int64_t* __restrict__ out_keys, float* __restrict__ out_scores,
                                                          uint32_t* __restrict__ out_counts) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    uint32_t img;
    int64_t key;
    search_merge_lists(ws_keys, ws_img, n_lists, nq, k, q, lane, img, key);
    const bool real = (uint32_t)lane < k && img != 0u;
    if ((uint32_t)lane < k) {
        out_keys[(size_t)q * k + lane] = real ? key : kEmpty;
        out_scores[(size_t)q * k + lane] = real ? image_score(img) : -__builtin_inff();
    }
    const uint64_t rm = __ballot(real);
    if (out_counts && lane == 0) out_counts[q] = (uint32_t)__popcll(rm);
}

// The seed merge of the batched search: the seed pass's lists into one more list, [nq][k], sorted, padded with image 0 / the empty key.
__global__ __launch_bounds__(64) void search_seed_merge_kernel(const int64_t* __restrict__ ws_keys, const uint32_t* __restrict__ ws_img, uint32_t n_lists,
                                                               uint32_t nq, uint32_t k, int64_t* __restrict__ seed_keys, uint32_t* __restrict__ seed_img) {
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x;
    uint32_t img;
    int64_t key;
    search_merge_lists(ws_keys, ws_img, n_lists, nq, k, q, lane, img, key);
    if ((uint32_t)lane < k) {
        seed_img[(size_t)q * k + lane] = img;
        seed_keys[(size_t)q * k + lane] = img != 0u ? key : kEmpty;
    }
}

// ---- groups: every member of a table group searched in ONE scan (SPEC.md §3 "Search", "Groups"; DESIGN.md §4 "Search", "Groups") ------------------
// The members' steps are cut into ranges of ONE length S, so that the collection's total work, not each member's, is spread over the block budget:
// member j owns the ranges [first[j], first[j + 1]) of a flat range index, ceil(steps_j / S) of them (the last one shorter, a small member's only one
// shorter than S).  The plan lies at the front of the workspace: S (8 bytes), first[0 .. n_tables] (a word each), rounded up to 16 bytes; the lists
// [range][n_queries][k] follow — a member's lists are consecutive, so its merge is search_merge_lists from list first[j] on.
__host__ __device__ constexpr size_t group_search_plan_bytes(uint32_t n_tables) { return (8 + 4 * ((size_t)n_tables + 1) + 15) / 16 * 16; }
__device__ __forceinline__ const uint32_t* group_search_first(const uint64_t* plan) { return reinterpret_cast<const uint32_t*>(plan + 1); }
// the slots of a member (SPEC.md §2: capacity = buckets x bucket width, exactly — what mee_table keeps as `capacity`) and the 32-slot steps over them
__host__ __device__ constexpr uint64_t group_search_slots(uint64_t nb) { return nb * (uint64_t)kW; }
__host__ __device__ constexpr uint64_t group_search_steps(uint64_t nb) { return (group_search_slots(nb) + 31) / 32; }

// The plan, on the device: it reads the descriptors group_refresh keeps current, so it follows mee_reserve without a host copy and stands in a captured
// graph.  One block, thread j = member j (blockDim = n_tables rounded up to whole waves, <= kMaxGroupTables): the sum of the members' steps by a wave
// and a block reduction, S = ceil(sum / max_ranges), each member's ranges, and their exclusive prefix by a wave scan and the waves' totals.
// sum_j ceil(steps_j / S) <= sum / S + n_tables <= max_ranges + n_tables: what the host sized the grid and the lists for, so nothing is read back.
__global__ __launch_bounds__(kMaxGroupTables) void group_search_plan_kernel(const GroupDesc* __restrict__ desc, uint32_t n_tables, uint32_t max_ranges,
                                                                            uint64_t* __restrict__ plan) {
    __shared__ uint64_t wave_steps[kMaxGroupTables / 64];
    __shared__ uint32_t wave_ranges[kMaxGroupTables / 64];
    const uint32_t j = threadIdx.x, lane = j & 63, w = j >> 6, n_waves = blockDim.x >> 6;
    const uint64_t steps = j < n_tables ? group_search_steps(desc[j].nb) : 0;
    unsigned long long sum = steps;
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) wave_steps[w] = sum;
    __syncthreads();
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_waves; ++i) total += wave_steps[i];
    const uint64_t S = total > max_ranges ? (total + max_ranges - 1) / max_ranges : 1;
    const uint32_t ranges = j >= n_tables ? 0u : steps > S ? (uint32_t)((steps + S - 1) / S) : 1u;
    uint32_t incl = ranges;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d);
        if ((int)lane >= d) incl += up;
    }
    if (lane == 63) wave_ranges[w] = incl;
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t i = 0; i < w; ++i) before += wave_ranges[i];
    uint32_t* const first = reinterpret_cast<uint32_t*>(plan + 1);
    if (j < n_tables) first[j] = before + incl - ranges;
    if (j == n_tables - 1) first[n_tables] = before + incl;
    if (j == 0) plan[0] = S;
}

// search_scan_block for a group: the flat grid holds n_tiles blocks per range index r, for every r the host's bound allows; a block past the plan's
// last range returns at once.  The member of r is the upper bound of r in first[] — first[] rises strictly, every member has a range — by one binary
// search in global memory (a few hundred L2-resident words at the most, read once per block; the scan body owns the dynamic LDS from offset 0), the
// same in every lane and said so.  The member's planes and slot count come from its descriptor; SCAN is called as search_scan_block calls it,
// without seeds and without a filter.  queries: [n_tables][nq_all][dim].
template <auto SCAN>
__device__ __forceinline__ void search_group_scan_block(const GroupDesc* __restrict__ desc, uint32_t n_tables, uint32_t dim, const float* __restrict__ queries,
                                                        uint32_t nq_all, uint32_t tile, uint32_t n_tiles, uint32_t k, const uint64_t* __restrict__ plan,
                                                        int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img) {
    const uint32_t t = blockIdx.x % n_tiles, r = blockIdx.x / n_tiles;
    const uint32_t* __restrict__ first = group_search_first(plan);
    if (r >= first[n_tables]) return;   // block-uniform
    uint32_t lo = 0, hi = n_tables;     // first[lo] <= r < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= r) lo = mid; else hi = mid;
    }
    const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
    const GroupDesc d = desc[j];
    const uint64_t capacity = group_search_slots(d.nb), n_steps = group_search_steps(d.nb), S = plan[0];
    const uint32_t q0 = t * tile, nq = nq_all - q0 < tile ? nq_all - q0 : tile;
    uint64_t s0 = (uint64_t)(r - first[j]) * S, s1 = s0 + S;
    if (s1 > n_steps) s1 = n_steps;
    if (s0 > s1) s0 = s1;
    SCAN(dim, d.tkeys, d.values, capacity, queries + ((size_t)j * nq_all + q0) * dim, nq, k, s0, s1, nullptr, nullptr, (size_t)r * nq_all + q0, ws_keys, ws_img,
         SearchFilter{});
}

template <int KS, int ROWS, int METRIC>
__global__ __launch_bounds__(64) void search_group_scan_kernel(const GroupDesc* __restrict__ desc, uint32_t n_tables, const float* __restrict__ queries,
                                                               uint32_t nq_all, uint32_t tile, uint32_t n_tiles, uint32_t k, const uint64_t* __restrict__ plan,
                                                               int64_t* __restrict__ ws_keys, uint32_t* __restrict__ ws_img) {
    search_group_scan_block<search_scan_body<KS, ROWS, METRIC, false>>(desc, n_tables, 16 * KS, queries, nq_all, tile, n_tiles, k, plan, ws_keys, ws_img);
}
template <int ROWS, int METRIC>
__global__ __launch_bounds__(64) void search_group_wide_scan_kernel(const GroupDesc* __restrict__ desc, uint32_t n_tables, uint32_t dim,
                                                                    const float* __restrict__ queries, uint32_t nq_all, uint32_t tile, uint32_t n_tiles,
                                                                    uint32_t k, const uint64_t* __restrict__ plan, int64_t* __restrict__ ws_keys,
                                                                    uint32_t* __restrict__ ws_img) {
    search_group_scan_block<search_wide_scan_body<ROWS, METRIC, false>>(desc, n_tables, dim, queries, nq_all, tile, n_tiles, k, plan, ws_keys, ws_img);
}

// One wave per (member, query): search_merge_kernel over the member's own lists, into row member * nq + query of the outputs — its epilogue, written out
// again: keys and scores, the padded tail and the count, no memset in front (search_merge_kernel keeps its machine code that way).
__global__ __launch_bounds__(64) void group_search_merge_kernel(const uint64_t* __restrict__ plan, const int64_t* __restrict__ ws_keys,
                                                                const uint32_t* __restrict__ ws_img, uint32_t nq, uint32_t k, int64_t* __restrict__ out_keys,
                                                                float* __restrict__ out_scores, uint32_t* __restrict__ out_counts) {
    const uint32_t j = blockIdx.x / nq, q = blockIdx.x % nq;
    const int lane = threadIdx.x;
    const uint32_t* __restrict__ first = group_search_first(plan);
    const uint32_t f0 = first[j], n_lists = first[j + 1] - f0;
    const size_t o = (size_t)f0 * nq * k;
    uint32_t img;
    int64_t key;
    search_merge_lists(ws_keys + o, ws_img + o, n_lists, nq, k, q, lane, img, key);
    const size_t row = blockIdx.x;
    const bool real = (uint32_t)lane < k && img != 0u;
    if ((uint32_t)lane < k) {
        out_keys[row * k + lane] = real ? key : kEmpty;
        out_scores[row * k + lane] = real ? image_score(img) : -__builtin_inff();
    }
    const uint64_t rm = __ballot(real);
    if (out_counts && lane == 0) out_counts[row] = (uint32_t)__popcll(rm);
}

// =========================================================================================================
// host side
// =========================================================================================================
static size_t search_lds_bytes(uint32_t dim, size_t nq, uint32_t k, int metric) {
    return search_pad32(nq) * dim * 2 + search_sel_bytes(nq, search_pad32(nq), k, metric == MEE_METRIC_COSINE);
}
// the pointers every search entry point is handed
static int search_pointer_check(const float* d_queries, const int64_t* d_out_keys, const float* d_out_scores, const void* d_workspace, const char* name) {
    if (!d_queries || !d_out_keys || !d_out_scores || !d_workspace) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (((uintptr_t)d_queries & 15) || ((uintptr_t)d_workspace & 7)) return fail(MEE_ERR_INVALID_ARG, "%s: queries must be 16-byte aligned, the workspace 8-byte aligned", name);
    return MEE_OK;
}
// what the entry points refuse, before anything is launched; -> the blocks of the largest grid a search of this device launches.  batch: n_queries
// is held against mee_search_batch's cap instead of the per-call limits.
static int search_check(const mee_table* t, size_t nq, uint32_t k, const char* name, uint32_t* max_grid, bool batch = false) {
    if (!t) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    const uint32_t max_dim = batch ? MEE_SEARCH_MAX_DIM : 256;   // the batched entry points alone have the wide scan
    if (t->dim % 16 || t->dim < 16 || t->dim > max_dim) return fail(MEE_ERR_INVALID_ARG, "%s: dim must be a multiple of 16 in [16, %u] (got %u)", name, max_dim, t->dim);
    if (k < 1 || k > MEE_SEARCH_MAX_K) return fail(MEE_ERR_INVALID_ARG, "%s: k must be in [1, %d] (got %u)", name, MEE_SEARCH_MAX_K, k);
    const size_t kk = k < kSearchMinCap ? kSearchMinCap : k;
    if (batch && (nq < 1 || nq > MEE_SEARCH_BATCH_MAX_QUERIES))
        return fail(MEE_ERR_INVALID_ARG, "%s: n_queries must be in [1, %d] (got %zu)", name, MEE_SEARCH_BATCH_MAX_QUERIES, nq);
    if (!batch && (nq < 1 || nq > MEE_SEARCH_MAX_QK / kk || (nq + 31) / 32 * 32 * t->dim > MEE_SEARCH_MAX_QUERY_ELEMS))
        return fail(MEE_ERR_INVALID_ARG, "%s: n_queries = %zu is outside the per-call limits for k = %u and dim = %u: n_queries >= 1, n_queries * max(k, %u) <= %d and "
                    "n_queries rounded up to a multiple of 32, times dim, <= %d", name, nq, k, t->dim, kSearchMinCap, MEE_SEARCH_MAX_QK, MEE_SEARCH_MAX_QUERY_ELEMS);
    if (int rc = refuse_narrow_rows(t, name, false)) return rc;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    *max_grid = (uint32_t)cus * kSearchBlocksPerCU;
    return MEE_OK;
}

// ---- the batched search's launch plan (DESIGN.md §4 "Search", "Batched") --------------------------------------------------------------------------
// The three tuning constants can be set at build time (-D) for the measurements of profiles/search.md; the values here are the ones kept.
#ifndef MEE_SEARCH_SEED_DIV
#define MEE_SEARCH_SEED_DIV 32
#endif
#ifndef MEE_SEARCH_TILE_MAX_QUERIES
#define MEE_SEARCH_TILE_MAX_QUERIES 32
#endif
constexpr uint32_t kSearchSeedDiv = MEE_SEARCH_SEED_DIV;                 // the seed pass scans the first n_steps / kSearchSeedDiv steps
constexpr uint32_t kSearchSeedMinSteps = 64;                             // ... unless that is fewer steps than this: such a table has no seed pass
constexpr uint32_t kSearchSeedGridDiv = 4;                               // the seed pass's share of the block budget
constexpr uint32_t kSearchTileMaxQueries = MEE_SEARCH_TILE_MAX_QUERIES;  // a tile is at most one row block of 32 queries (MEE_SEARCH_MAX_QK: no cap)

// The queries of one tile: at most what one mee_search call accepts for this k and dim, so a block's LDS stays inside search_lds_bytes' budget, and
// at most one row block — a fraction of that LDS, so more waves stay resident; measured against tiles at the per-call limit in profiles/search.md.
static uint32_t search_batch_tile(uint32_t dim, uint32_t k, int metric) {
    if (dim > 256) return search_wide_tile(dim, k);   // the wide scan's own rule: its LDS budget, one row block
    const uint32_t by_qk = MEE_SEARCH_MAX_QK / (k < kSearchMinCap ? kSearchMinCap : k), by_elems = MEE_SEARCH_MAX_QUERY_ELEMS / dim / 32 * 32;
    const uint32_t limit = by_qk < by_elems ? by_qk : by_elems;
    const uint32_t cap = metric == MEE_METRIC_COSINE && kSearchCosineTileMax < kSearchTileMaxQueries ? kSearchCosineTileMax : kSearchTileMaxQueries;
    return limit < cap ? limit : cap;
}

struct SearchBatchPlan {
    uint32_t tile, n_tiles;
    uint32_t ranges, seed_ranges;   // lists per query of the main scan / of the seed pass (0: no seed pass); with a table's step count the actual
                                    // figures, without one (n_steps == UINT64_MAX) the largest any table gives: what the workspace is sized for
    uint64_t seed_steps, per_range, per_seed_range;
    uint64_t lists() const { return 1 + (uint64_t)ranges + seed_ranges; }   // list 0 is the seed area
};
static SearchBatchPlan search_batch_plan(uint32_t dim, uint32_t nq, uint32_t k, uint32_t max_grid, uint64_t n_steps, int metric) {
    SearchBatchPlan p{};
    p.tile = search_batch_tile(dim, k, metric);
    p.n_tiles = (nq + p.tile - 1) / p.tile;
    p.ranges = max_grid / p.n_tiles > 1 ? max_grid / p.n_tiles : 1;   // the block budget divided between the tiles
    p.seed_ranges = max_grid / kSearchSeedGridDiv / p.n_tiles > 1 ? max_grid / kSearchSeedGridDiv / p.n_tiles : 1;
    if (n_steps == UINT64_MAX) return p;
    p.seed_steps = n_steps / kSearchSeedDiv >= kSearchSeedMinSteps ? n_steps / kSearchSeedDiv : 0;
    const uint64_t main_steps = n_steps - p.seed_steps;
    p.per_range = main_steps > p.ranges ? (main_steps + p.ranges - 1) / p.ranges : 1;
    p.ranges = main_steps > p.per_range ? (uint32_t)((main_steps + p.per_range - 1) / p.per_range) : 1;
    if (p.seed_steps) {
        p.per_seed_range = (p.seed_steps + p.seed_ranges - 1) / p.seed_ranges;
        p.seed_ranges = (uint32_t)((p.seed_steps + p.per_seed_range - 1) / p.per_seed_range);
    } else {
        p.seed_ranges = 0;
    }
    return p;
}

}  // namespace mee

using namespace mee;

// the batched search of either metric: what mee_search_batch[_workspace_bytes] and mee_search_metric[_workspace_bytes] share
static int search_batch_workspace(const mee_table* t, int metric, size_t n_queries, uint32_t k, uint64_t* bytes_out, const char* name) {
    if (!bytes_out) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    *bytes_out = 0;
    uint32_t max_grid = 0;
    if (int rc = search_check(t, n_queries, k, name, &max_grid, true)) return rc;
    // the seed area, the main lists and the seed pass's lists, each [n_queries][k] keys and images; the layout needs no padding
    *bytes_out = search_batch_plan(t->dim, (uint32_t)n_queries, k, max_grid, UINT64_MAX, metric).lists() * n_queries * k * 12;
    return MEE_OK;
}

// the exclude lists of a filtered search as the caller hands them in: [rows][n] keys, rows == n_queries or 1
struct SearchExclude {
    const int64_t* d_keys;
    size_t rows, n;
};
// the entries between two sorted rows, and the bytes of the sorted-list area in front of the metric's own workspace: the sorted rows, then one count
// per row, rounded up to 8 bytes
static uint32_t search_exclude_ep(size_t n) {
    uint32_t ep = 1;
    while (ep < n) ep <<= 1;
    return ep;
}
static uint64_t search_exclude_bytes(size_t rows, size_t n) { return (uint64_t)rows * search_exclude_ep(n) * 8 + (rows + 1) / 2 * 8; }
static int search_exclude_check(size_t n_queries, size_t rows, size_t n, const char* name) {
    if (n < 1 || n > MEE_SEARCH_MAX_EXCLUDE) return fail(MEE_ERR_INVALID_ARG, "%s: n_exclude must be in [1, %d] (got %zu)", name, MEE_SEARCH_MAX_EXCLUDE, n);
    if (rows != 1 && rows != n_queries) return fail(MEE_ERR_INVALID_ARG, "%s: exclude_rows must be n_queries (%zu) or 1 (got %zu)", name, n_queries, rows);
    return MEE_OK;
}

// One scan launch of the table's row shape: the call's nq queries in n_tiles tiles of `tile`, each tile against `ranges` ranges of per_range steps of
// [step0, step_end) — one one-wave block per (tile, range) pair; seed lists (or null) in, the lists [ranges][nq][k] out.
struct SearchTiles {
    const float* d_queries;
    uint32_t nq, tile, n_tiles, k;
};
template <int METRIC, bool FILTER>
static void search_scan_launch(const mee_table* t, hipStream_t st, const SearchTiles& q, uint32_t ranges, uint64_t step0, uint64_t step_end, uint64_t per_range,
                               const int64_t* seed_keys, const uint32_t* seed_img, int64_t* out_keys, uint32_t* out_img, SearchFilterOf<FILTER> flt) {
    const uint32_t blocks = q.n_tiles * ranges, tile_nq = q.tile < q.nq ? q.tile : q.nq;
    if (t->dim > 256) with_flag(t->bf16_rows, [&](auto bf16) {
        search_wide_scan_kernel<bf16 ? kRowsBF16 : kRowsF32, METRIC, FILTER><<<blocks, 64, search_wide_lds_bytes(t->dim, tile_nq, q.k), st>>>(
            t->keys, t->values, t->capacity, t->dim, q.d_queries, q.nq, q.tile, q.n_tiles, q.k, step0, step_end, per_range, seed_keys, seed_img, out_keys, out_img, flt);
    });
    else with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)(t->dim / 16), [&](auto ks) { with_flag(t->bf16_rows, [&](auto bf16) {
        search_batch_scan_kernel<ks, bf16 ? kRowsBF16 : kRowsF32, METRIC, FILTER><<<blocks, 64, search_lds_bytes(t->dim, tile_nq, q.k, METRIC), st>>>(
            t->keys, t->values, t->capacity, q.d_queries, q.nq, q.tile, q.n_tiles, q.k, step0, step_end, per_range, seed_keys, seed_img, out_keys, out_img, flt);
    }); });
}

// FILTER: `ex` is read, d_workspace begins with the sorted-list area, and one more launch — search_exclude_prepare_kernel — goes in front
template <int METRIC, bool FILTER = false>
static int search_batch_launch(const mee_table* t, const float* d_queries, size_t n_queries, uint32_t k, int64_t* d_out_keys, float* d_out_scores,
                               uint32_t* d_out_counts, void* d_workspace, void* stream, const char* name, const SearchExclude& ex = {}) {
    uint32_t max_grid = 0;
    if (int rc = search_check(t, n_queries, k, name, &max_grid, true)) return rc;
    if (int rc = search_pointer_check(d_queries, d_out_keys, d_out_scores, d_workspace, name)) return rc;
    SearchFilterOf<FILTER> flt{};
    if constexpr (FILTER) {
        if (int rc = search_exclude_check(n_queries, ex.rows, ex.n, name)) return rc;
        if (!ex.d_keys || ((uintptr_t)ex.d_keys & 7)) return fail(MEE_ERR_INVALID_ARG, "%s: the exclude keys must be a non-null, 8-byte aligned pointer", name);
    }
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    const uint32_t nq = (uint32_t)n_queries;
    if constexpr (FILTER) {   // the sorted rows and their counts, then the workspace of the unfiltered launches
        const uint32_t ep = search_exclude_ep(ex.n);
        int64_t* sorted = (int64_t*)d_workspace;
        uint32_t* count = (uint32_t*)(sorted + ex.rows * ep);
        search_exclude_prepare_kernel<<<(uint32_t)ex.rows, kExcludeThreads, (size_t)ep * 8 + 16, st>>>(ex.d_keys, (uint32_t)ex.n, ep, sorted, count);
        flt = SearchFilter{sorted, count, ep, ex.rows == 1 ? 0u : 1u};
        d_workspace = (unsigned char*)d_workspace + search_exclude_bytes(ex.rows, ex.n);
    }
    const uint64_t n_steps = (t->capacity + 31) / 32;
    const SearchBatchPlan p = search_batch_plan(t->dim, nq, k, max_grid, n_steps, METRIC);
    // lists of [nq][k] entries: 0 the seed area, 1 .. ranges the main scan's, then the seed pass's; the key plane of all lists, then the image plane
    const size_t list = (size_t)nq * k;
    int64_t* ws_keys = (int64_t*)d_workspace;
    uint32_t* ws_img = (uint32_t*)(ws_keys + p.lists() * list);
    const SearchTiles tiles{d_queries, nq, p.tile, p.n_tiles, k};
    const bool seeded = p.seed_ranges != 0;
    if (seeded) {   // the seed pass and its merge, then the main scan from the seed's thresholds
        const size_t so = (1 + (size_t)p.ranges) * list;
        search_scan_launch<METRIC, FILTER>(t, st, tiles, p.seed_ranges, 0, p.seed_steps, p.per_seed_range, nullptr, nullptr, ws_keys + so, ws_img + so, flt);
        search_seed_merge_kernel<<<nq, 64, 0, st>>>(ws_keys + so, ws_img + so, p.seed_ranges, nq, k, ws_keys, ws_img);
    }
    search_scan_launch<METRIC, FILTER>(t, st, tiles, p.ranges, p.seed_steps, n_steps, p.per_range, seeded ? ws_keys : nullptr, seeded ? ws_img : nullptr, ws_keys + list,
                                       ws_img + list, flt);
    // the seed area is one more list in front of the main scan's: the prefix is not scanned again
    if (seeded) search_merge_kernel<<<nq, 64, 0, st>>>(ws_keys, ws_img, 1 + p.ranges, nq, k, d_out_keys, d_out_scores, d_out_counts);
    else search_merge_kernel<<<nq, 64, 0, st>>>(ws_keys + list, ws_img + list, p.ranges, nq, k, d_out_keys, d_out_scores, d_out_counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}
static int search_metric_check(int metric, const char* name) {
    if (metric == MEE_METRIC_IP || metric == MEE_METRIC_COSINE) return MEE_OK;
    return fail(MEE_ERR_INVALID_ARG, "%s: metric must be MEE_METRIC_IP (0) or MEE_METRIC_COSINE (1) (got %d)", name, metric);
}

// ---- the grouped search's launch plan on the host: the tiles as search_batch_plan cuts them, the ranges of the WHOLE collection, and with them the
// bound on the range indices the device-side plan can hand out — the blocks of the grid and the lists of the workspace
struct GroupSearchShape {
    uint32_t tile, n_tiles;
    uint32_t max_ranges;   // R: the block budget divided between the tiles
    uint32_t lists;        // R + n_tables
    uint64_t bytes(uint32_t n_tables, size_t nq, uint32_t k) const { return group_search_plan_bytes(n_tables) + (uint64_t)lists * nq * k * 12; }
};
// what both group entry points refuse, before anything is launched or written
static int group_search_check(const mee_group* g, int metric, size_t nq, uint32_t k, const char* name, GroupSearchShape* s) {
    if (!g) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = search_metric_check(metric, name)) return rc;
    if (g->dim % 16 || g->dim < 16 || g->dim > MEE_SEARCH_MAX_DIM)
        return fail(MEE_ERR_INVALID_ARG, "%s: dim must be a multiple of 16 in [16, %d] (got %u)", name, MEE_SEARCH_MAX_DIM, g->dim);
    if (k < 1 || k > MEE_SEARCH_MAX_K) return fail(MEE_ERR_INVALID_ARG, "%s: k must be in [1, %d] (got %u)", name, MEE_SEARCH_MAX_K, k);
    if (nq < 1 || nq > MEE_SEARCH_BATCH_MAX_QUERIES / g->n_tables)
        return fail(MEE_ERR_INVALID_ARG, "%s: n_tables * n_queries must be in [1, %d] (got %u tables x %zu queries)", name, MEE_SEARCH_BATCH_MAX_QUERIES, g->n_tables, nq);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g->device) != hipSuccess || cus <= 0) cus = 256;
    const uint32_t max_grid = (uint32_t)cus * kSearchBlocksPerCU;
    s->tile = search_batch_tile(g->dim, k, metric);
    s->n_tiles = ((uint32_t)nq + s->tile - 1) / s->tile;
    s->max_ranges = max_grid / s->n_tiles > 1 ? max_grid / s->n_tiles : 1;
    s->lists = s->max_ranges + g->n_tables;
    return MEE_OK;
}
// The one scan launch of a group's row shape: search_scan_launch's dispatch with the grouped kernels, n_tiles x lists one-wave blocks.
template <int METRIC>
static void group_search_scan_launch(const mee_group* g, hipStream_t st, const SearchTiles& q, uint32_t lists, const uint64_t* plan, int64_t* out_keys, uint32_t* out_img) {
    const uint32_t blocks = q.n_tiles * lists, tile_nq = q.tile < q.nq ? q.tile : q.nq;
    if (g->dim > 256) with_flag(g->bf16_rows, [&](auto bf16) {
        search_group_wide_scan_kernel<bf16 ? kRowsBF16 : kRowsF32, METRIC><<<blocks, 64, search_wide_lds_bytes(g->dim, tile_nq, q.k), st>>>(
            g->d_desc, g->n_tables, g->dim, q.d_queries, q.nq, q.tile, q.n_tiles, q.k, plan, out_keys, out_img);
    });
    else with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)(g->dim / 16), [&](auto ks) { with_flag(g->bf16_rows, [&](auto bf16) {
        search_group_scan_kernel<ks, bf16 ? kRowsBF16 : kRowsF32, METRIC><<<blocks, 64, search_lds_bytes(g->dim, tile_nq, q.k, METRIC), st>>>(
            g->d_desc, g->n_tables, q.d_queries, q.nq, q.tile, q.n_tiles, q.k, plan, out_keys, out_img);
    }); });
}

extern "C" {

int mee_search_workspace_bytes(const mee_table* t, size_t n_queries, uint32_t k, uint64_t* bytes_out) {
    if (!bytes_out) return fail(MEE_ERR_INVALID_ARG, "mee_search_workspace_bytes: null argument");
    *bytes_out = 0;
    uint32_t max_grid = 0;
    if (int rc = search_check(t, n_queries, k, "mee_search_workspace_bytes", &max_grid)) return rc;
    *bytes_out = (uint64_t)max_grid * n_queries * k * 12;   // a key and an image per (block, query, rank); independent of the table's capacity
    return MEE_OK;
}

int mee_search(const mee_table* t, const float* d_queries, size_t n_queries, uint32_t k, int64_t* d_out_keys, float* d_out_scores, uint32_t* d_out_counts,
               void* d_workspace, void* stream) {
    MEE_RANGE("mee_search");
    uint32_t max_grid = 0;
    if (int rc = search_check(t, n_queries, k, "mee_search", &max_grid)) return rc;
    if (int rc = search_pointer_check(d_queries, d_out_keys, d_out_scores, d_workspace, "mee_search")) return rc;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    const uint64_t n_steps = (t->capacity + 31) / 32;
    const uint64_t per_block = (n_steps + max_grid - 1) / max_grid;
    const uint32_t grid = (uint32_t)((n_steps + per_block - 1) / per_block);   // <= max_grid: what mee_search_workspace_bytes sized the workspace for
    const uint32_t nq = (uint32_t)n_queries;
    int64_t* ws_keys = (int64_t*)d_workspace;
    uint32_t* ws_img = (uint32_t*)(ws_keys + (size_t)grid * nq * k);
    const size_t lds = search_lds_bytes(t->dim, nq, k, MEE_METRIC_IP);
    with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)(t->dim / 16), [&](auto ks) { with_flag(t->bf16_rows, [&](auto bf16) {
        search_scan_kernel<ks, bf16 ? kRowsBF16 : kRowsF32><<<grid, 64, lds, st>>>(t->keys, t->values, t->capacity, d_queries, nq, k, per_block, ws_keys, ws_img);
    }); });
    search_merge_kernel<<<nq, 64, 0, st>>>(ws_keys, ws_img, grid, nq, k, d_out_keys, d_out_scores, d_out_counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_search_batch_workspace_bytes(const mee_table* t, size_t n_queries, uint32_t k, uint64_t* bytes_out) {
    return search_batch_workspace(t, MEE_METRIC_IP, n_queries, k, bytes_out, "mee_search_batch_workspace_bytes");
}

int mee_search_batch(const mee_table* t, const float* d_queries, size_t n_queries, uint32_t k, int64_t* d_out_keys, float* d_out_scores,
                     uint32_t* d_out_counts, void* d_workspace, void* stream) {
    MEE_RANGE("mee_search_batch");
    return search_batch_launch<MEE_METRIC_IP>(t, d_queries, n_queries, k, d_out_keys, d_out_scores, d_out_counts, d_workspace, stream, "mee_search_batch");
}

int mee_search_metric_workspace_bytes(const mee_table* t, int metric, size_t n_queries, uint32_t k, uint64_t* bytes_out) {
    if (bytes_out) *bytes_out = 0;
    if (int rc = search_metric_check(metric, "mee_search_metric_workspace_bytes")) return rc;
    if (metric == MEE_METRIC_IP) return mee_search_batch_workspace_bytes(t, n_queries, k, bytes_out);
    return search_batch_workspace(t, metric, n_queries, k, bytes_out, "mee_search_metric_workspace_bytes");
}

int mee_search_metric(const mee_table* t, int metric, const float* d_queries, size_t n_queries, uint32_t k, int64_t* d_out_keys, float* d_out_scores,
                      uint32_t* d_out_counts, void* d_workspace, void* stream) {
    if (int rc = search_metric_check(metric, "mee_search_metric")) return rc;
    if (metric == MEE_METRIC_IP) return mee_search_batch(t, d_queries, n_queries, k, d_out_keys, d_out_scores, d_out_counts, d_workspace, stream);
    MEE_RANGE("mee_search_metric");
    return search_batch_launch<MEE_METRIC_COSINE>(t, d_queries, n_queries, k, d_out_keys, d_out_scores, d_out_counts, d_workspace, stream, "mee_search_metric");
}

int mee_search_filtered_workspace_bytes(const mee_table* t, int metric, size_t n_queries, uint32_t k, size_t exclude_rows, size_t n_exclude, uint64_t* bytes_out) {
    const char* name = "mee_search_filtered_workspace_bytes";
    if (bytes_out) *bytes_out = 0;
    if (int rc = search_metric_check(metric, name)) return rc;
    uint64_t base = 0;
    if (int rc = search_batch_workspace(t, metric, n_queries, k, &base, name)) return rc;
    if (int rc = search_exclude_check(n_queries, exclude_rows, n_exclude, name)) return rc;
    *bytes_out = search_exclude_bytes(exclude_rows, n_exclude) + base;
    return MEE_OK;
}

int mee_search_filtered(const mee_table* t, int metric, const float* d_queries, size_t n_queries, uint32_t k, const int64_t* d_exclude, size_t exclude_rows,
                        size_t n_exclude, int64_t* d_out_keys, float* d_out_scores, uint32_t* d_out_counts, void* d_workspace, void* stream) {
    if (int rc = search_metric_check(metric, "mee_search_filtered")) return rc;
    MEE_RANGE("mee_search_filtered");
    const SearchExclude ex{d_exclude, exclude_rows, n_exclude};
    if (metric == MEE_METRIC_IP)
        return search_batch_launch<MEE_METRIC_IP, true>(t, d_queries, n_queries, k, d_out_keys, d_out_scores, d_out_counts, d_workspace, stream, "mee_search_filtered", ex);
    return search_batch_launch<MEE_METRIC_COSINE, true>(t, d_queries, n_queries, k, d_out_keys, d_out_scores, d_out_counts, d_workspace, stream, "mee_search_filtered", ex);
}

int mee_group_search_workspace_bytes(const mee_group* g, int metric, size_t n_queries, uint32_t k, uint64_t* bytes_out) {
    const char* name = "mee_group_search_workspace_bytes";
    if (!bytes_out) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    *bytes_out = 0;
    GroupSearchShape s{};
    if (int rc = group_search_check(g, metric, n_queries, k, name, &s)) return rc;
    *bytes_out = s.bytes(g->n_tables, n_queries, k);
    return MEE_OK;
}

int mee_group_search(mee_group* g, int metric, const float* d_queries, size_t n_queries, uint32_t k, int64_t* d_out_keys, float* d_out_scores,
                     uint32_t* d_out_counts, void* d_workspace, void* stream) {
    MEE_RANGE("mee_group_search");
    GroupSearchShape s{};
    if (int rc = group_search_check(g, metric, n_queries, k, "mee_group_search", &s)) return rc;
    if (int rc = search_pointer_check(d_queries, d_out_keys, d_out_scores, d_workspace, "mee_group_search")) return rc;
    if (int rc = group_refresh(g, stream)) return rc;   // a member's planes and slot count may have moved (mee_reserve)
    DeviceGuard guard(g->device);
    hipStream_t st = as_stream(stream);
    const uint32_t nq = (uint32_t)n_queries;
    uint64_t* plan = (uint64_t*)d_workspace;
    int64_t* ws_keys = (int64_t*)((unsigned char*)d_workspace + group_search_plan_bytes(g->n_tables));
    uint32_t* ws_img = (uint32_t*)(ws_keys + (size_t)s.lists * nq * k);
    group_search_plan_kernel<<<1, (g->n_tables + 63) / 64 * 64, 0, st>>>(g->d_desc, g->n_tables, s.max_ranges, plan);
    const SearchTiles tiles{d_queries, nq, s.tile, s.n_tiles, k};
    if (metric == MEE_METRIC_COSINE) group_search_scan_launch<MEE_METRIC_COSINE>(g, st, tiles, s.lists, plan, ws_keys, ws_img);
    else group_search_scan_launch<MEE_METRIC_IP>(g, st, tiles, s.lists, plan, ws_keys, ws_img);
    group_search_merge_kernel<<<g->n_tables * nq, 64, 0, st>>>(plan, ws_keys, ws_img, nq, k, d_out_keys, d_out_scores, d_out_counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
