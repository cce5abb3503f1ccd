// meepo_device.h — device-side building blocks shared by the gfx950 kernels (wave64 only).
//
// Geometry used everywhere: a wave (64 lanes) is split into 4 "tiles" of 16 lanes.  One tile serves one key:
// its 16 lanes load the 16 keys of a bucket (one 128-byte line, 8 B per lane), a wave-wide __ballot turns the
// compares into a 64-bit mask of which each tile reads its own 16 bits, and the same 16 lanes then move the
// embedding row as float4 (16 lanes x 16 B = 256 B per instruction for dim 64).
//
// Reference anchor: /root/reference/README.md:2 (no code upstream); semantics: SPEC.md §1-§4.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/meepo_embedding.h"   // MEE_OPT_*, MEE_STATUS_*: what creating a key writes

namespace mee {

typedef float f32x4 __attribute__((ext_vector_type(4)));   // what __builtin_nontemporal_load / _store move as one dwordx4

constexpr int64_t kEmpty = INT64_MIN;
constexpr int64_t kReclaimed = INT64_MIN + 1;
constexpr int kW = 16;                                   // bucket width == tile width
constexpr unsigned long long kBias = 0x8000000000000000ull;  // scratch stores key^kBias so that 0 == empty
constexpr uint32_t kNoGroup = 0xFFFFFFFFu;
// Slot handles of mee_find_located / mee_find_or_insert_located: bits [0, 40) = the slot, bits [40, 62) = the table's layout epoch when the
// handle was made (bumped by remove / clear / reserve: whatever can move or free a row).  mee_apply_*_located ignores a handle of another
// epoch and raises MEE_STATUS_STALE_HANDLE instead of updating whatever lives in that slot now.  -1 = absent.
constexpr int kHandleSlotBits = 40;
constexpr int64_t kHandleSlotMask = (1ll << kHandleSlotBits) - 1;
constexpr uint32_t kHandleEpochMask = (1u << 22) - 1;
// decode: the slot a handle names, or -1 (absent, out of range, or made under another layout epoch: `stale`)
__device__ __forceinline__ int64_t handle_slot(int64_t h, int64_t tag, uint64_t capacity, bool& stale) {
    stale = h >= 0 && (h & ~kHandleSlotMask) != tag;
    const int64_t s = h & kHandleSlotMask;
    return (h >= 0 && !stale && (uint64_t)s < capacity) ? s : -1;   // a handle is the caller's data: never index past the planes
}

// SPEC.md §1
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31; return x;
}
__host__ __device__ __forceinline__ uint64_t mix64b(uint64_t x) {
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33; return x;
}
// admission policy (SPEC.md §3 find_or_insert_admit): the counter of `key` in row 0..2 of a count-min sketch of 3 rows of 2^log2w counters
__device__ __forceinline__ uint32_t sketch_index(int64_t key, int row, uint32_t log2w) {
    constexpr uint64_t A[3] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull};
    return (uint32_t)(mix64((uint64_t)key ^ A[row]) >> (64 - log2w)) + ((uint32_t)row << log2w);
}
__device__ __forceinline__ uint64_t bucket_of(int64_t key, uint64_t nb) { return __umul64hi(mix64((uint64_t)key), nb); }
// SPEC.md §1/§2: stride (in buckets) of a key's probe sequence — double hashing, 1 <= stride < nb
__device__ __forceinline__ uint64_t step_of(int64_t key, uint64_t nb) { return nb > 1 ? 1 + __umul64hi(mix64b((uint64_t)key), nb - 1) : 1; }
__device__ __forceinline__ uint64_t next_bucket(uint64_t b, uint64_t stride, uint64_t nb) { b += stride; return b >= nb ? b - nb : b; }
__device__ __forceinline__ uint32_t owner_of(int64_t key, uint32_t g) { return (uint32_t)__umul64hi(mix64b((uint64_t)key), (uint64_t)g); }
__device__ __forceinline__ bool reserved_key(int64_t k) { return k <= kReclaimed; }

// Table keys are read with plain loads by read-only kernels (find/assign/apply: no key changes while they run)
// and with agent-scope relaxed atomic loads (global_load … sc1: bypasses the per-CU L1) by kernels that claim
// slots concurrently, so a retry after a lost CAS never re-reads a stale L1 line.
template <bool COHERENT>
__device__ __forceinline__ int64_t load_table_key(const int64_t* p) {
    if constexpr (COHERENT) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

__device__ __forceinline__ uint32_t tile_bits(uint64_t wave_mask, int tile) {
    return (uint32_t)(wave_mask >> (tile * kW)) & 0xFFFFu;
}

// Locate `key` (SPEC.md §2 probe sequence); with CLAIM also place it when absent: CAS into the first RECLAIMED slot
// met on the way if there is one, else into the first EMPTY slot of the bucket that ended the probe.  Must be called
// by ALL 64 lanes in convergent control flow; tiles without work pass active=false.  Returns the slot or -1.
template <bool CLAIM, bool COHERENT>
__device__ __forceinline__ int64_t tile_locate(int64_t* __restrict__ tkeys, uint64_t nb, int64_t key, bool active,
                                               int tile, int tl, bool& is_new, bool& full) {
    const uint64_t b0 = bucket_of(key, nb), stride = step_of(key, nb);
    uint64_t b = b0;
    uint64_t steps = 0;
    uint32_t retries = 0;  // lost-CAS re-reads; bounded so that every wave reaches the exit
    int64_t tomb = -1;     // first RECLAIMED slot seen on this probe
    bool pend = active;
    int64_t slot = -1;
    is_new = false; full = false;
    while (__any(pend)) {
        const int64_t k = pend ? load_table_key<COHERENT>(tkeys + b * kW + tl) : kEmpty;
        const uint32_t tm = tile_bits(__ballot(pend && k == key), tile);
        const uint32_t te = tile_bits(__ballot(pend && k == kEmpty), tile);
        long long cas_old = 0;
        int64_t target = -1;
        long long expect = kEmpty;
        if constexpr (CLAIM) {
            const uint32_t tr = tile_bits(__ballot(pend && k == kReclaimed), tile);
            if (pend && tomb < 0 && tr) tomb = (int64_t)(b * kW) + (__ffs(tr) - 1);
            const bool last = steps + 1 >= nb;  // the whole sequence has been scanned after this bucket
            if (pend && !tm && (te || (last && tomb >= 0))) {
                target = tomb >= 0 ? tomb : (int64_t)(b * kW) + (__ffs(te) - 1);
                expect = tomb >= 0 ? kReclaimed : kEmpty;
                if (tl == 0)
                    cas_old = (long long)atomicCAS((unsigned long long*)(tkeys + target), (unsigned long long)expect,
                                                   (unsigned long long)key);
            }
            cas_old = __shfl(cas_old, tile * kW);
        }
        if (pend) {
            if (tm) { slot = (int64_t)(b * kW) + (__ffs(tm) - 1); pend = false; }
            else if (CLAIM && target >= 0) {
                if (cas_old == expect) { slot = target; is_new = true; pend = false; }
                else if (cas_old == key) { slot = target; pend = false; }
                else if (++retries > (1u << 20)) { full = true; pend = false; }
                else if (expect == kReclaimed) { tomb = -1; b = b0; steps = 0; }  // lost a tombstone: start over
                // else: another key took that EMPTY slot — re-read the same bucket
            } else if (te) pend = false;  // absent
            else if (++steps >= nb) { full = true; pend = false; }
            else b = next_bucket(b, stride, nb);
        }
    }
    return slot;
}

// The read-only probe of the lookups, with the keys already in flight: the caller has computed b = bucket_of(key, nb) and requested that
// bucket's line, k = tkeys[b * kW + tl] (kEmpty where !act) — for ALL the keys its tile handles, back to back, before it examines any of
// them; that is the whole point of the shape (a request per probe made every key wait for its predecessor's round trip).  From there the
// tile walks the key's SPEC.md §2 sequence until it meets the key, an EMPTY slot, or has visited all nb buckets.  Must be called by ALL
// 64 lanes in convergent control flow; tiles without work pass act = false.  Plain loads (see load_table_key), and it never writes:
// nothing is claimed, so no table key may change while the kernel runs.  Returns the slot or -1.
__device__ __forceinline__ int64_t tile_probe(const int64_t* __restrict__ tkeys, uint64_t nb, int64_t key, bool act, uint64_t b, int64_t k,
                                              int tile, int tl) {
    int64_t slot = -1;
    bool pend = act;
    uint64_t steps = 0;
    while (true) {
        const uint32_t tm = tile_bits(__ballot(pend && k == key), tile);
        const uint32_t te = tile_bits(__ballot(pend && k == kEmpty), tile);
        if (pend) {
            if (tm) { slot = (int64_t)(b * kW) + (__ffs(tm) - 1); pend = false; }
            else if (te || ++steps >= nb) pend = false;
            else b = next_bucket(b, step_of(key, nb), nb);
        }
        if (!__any(pend)) break;
        k = pend ? tkeys[b * kW + tl] : kEmpty;
    }
    return slot;
}

// ---- jagged batches over the members of a group: segment j = positions [offsets[j * stride], offsets[(j + 1) * stride]) of the n keys ------------
// Stages the n_tables + 1 segment bounds in LDS (loff: kMaxGroupTables + 1 entries) and ends with the barrier.  stride = 1, or bags_per_table
// where the bounds are every stride-th entry of a bag-offset array.  The offsets are the caller's: a bound beyond n is stored as n, which
// changes nothing for a position i < n (min(o, n) <= i iff o <= i) and keeps every bound, and every difference of two, at or below n.
__device__ __forceinline__ void stage_offsets(uint64_t* loff, const uint64_t* __restrict__ offsets, uint64_t stride, uint32_t n_tables, uint64_t n) {
    for (uint32_t j = threadIdx.x; j <= n_tables; j += blockDim.x) {
        const uint64_t o = offsets[(uint64_t)j * stride];
        loff[j] = o < n ? o : n;
    }
    __syncthreads();
}
// The member of position i: the last j < n_tables with loff[j] <= i (0 when there is none), so empty segments are skipped by the search
// itself and the result always names a member.  Whether i lies inside the segments at all — loff[0] <= i < loff[n_tables], and i < n — is
// the caller's test.
__device__ __forceinline__ uint32_t member_of_position(const uint64_t* loff, uint32_t n_tables, uint64_t i) {
    uint32_t lo = 0, hi = n_tables;   // invariant: loff[lo] <= i < loff[hi] once i is inside [loff[0], loff[n_tables])
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (loff[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// A wave step of a 4R-position kernel leaves tile t's result of round r in slot[r] of that tile's lanes; lane j < 4R collects the slot of
// position base + j (round j / 4, tile j % 4), so that the step's slots leave as ONE coalesced store.  All 64 lanes call it; lanes >= 4R get -1.
template <int R>
__device__ __forceinline__ int64_t collect_slots(const int64_t (&slot)[R], int lane) {
    int64_t mine = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t v = __shfl(slot[r], (lane & 3) * kW);
        if ((lane >> 2) == r) mine = v;
    }
    return mine;
}

// ---- bf16 output of the lookups (SPEC.md §3 "Output type") ------------------------------------------------------------------
// A lane that holds a float4 of a row stores it as 4 bf16 = 8 bytes; a row of dim bf16 is dim4 such 8-byte groups, so group g of
// output row i sits at index i * dim4 + g of a u32x2 array — the SAME index the fp32 kernels use on their f32x4 array.
// two fp32 -> two bfloat16 in one word, round to nearest even: plain casts, which gfx950 does with its packed convert (v_cvt_pk_bf16_f32).  It agrees
// with the integer rule of the spec on every finite value, denormals included (HIP kernels run with fp32 denormals on), sends a finite value beyond
// the largest bf16 to inf and a NaN to a NaN: tests/test_bf16_out.py checks exactly these on the device.  (The integer rule written out costs ~30
// VALU instructions per float4 in the wave's dependent tail — +0.4 us on a latency-bound dim-16 lookup — and a __builtin_convertvector of float2
// pairs made two pooled instances spill 32 B: profiles/bf16_out.md, profiles/bf16_out_resource_usage.txt.)
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bf16x2_of(float a, float b) {
    return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)a) | ((uint32_t)__builtin_bit_cast(uint16_t, (__bf16)b) << 16);
}
__device__ __forceinline__ u32x2 bf16x4_of(float a, float b, float c, float d) {
    u32x2 p;
    p.x = bf16x2_of(a, b);
    p.y = bf16x2_of(c, d);
    return p;
}
// the store of one such group; CACHED = false: a streaming (non-temporal) store, as the fp32 kernels use for outputs nothing re-reads from cache
template <bool CACHED, class V4>
__device__ __forceinline__ void store_bf16x4(void* out, uint64_t idx, const V4& v) {
    const u32x2 p = bf16x4_of(v.x, v.y, v.z, v.w);
    if constexpr (CACHED) reinterpret_cast<u32x2*>(out)[idx] = p;
    else __builtin_nontemporal_store(p, reinterpret_cast<u32x2*>(out) + idx);
}

// ---- the 16-byte result stores of the find family (fp32 output, compiled row shapes) ----------------------------------------------
// One wave step of find_span writes 4R consecutive result rows.  RowStore is those rows as a store target, and the ONE place that says how
// a 16-byte element group of a result row leaves under the call's policy: CACHED, a plain store (the line stays in the XCD's L2 for whoever
// reads the rows next), or streaming, a non-temporal global store.  Write-through forms of the streaming store were measured and lost
// (profiles/find_write_through.md): `sc1` and `sc0 sc1` take 1.5 us off a launch's floor, as the dirty lines they do not leave behind
// predict, and add 4.2 us per 256K keys to its slope; `sc1 nt` is `nt`; write-through for the batch's tail alone gains nothing either.
template <bool CACHED>
struct RowStore {
    f32x4* first;   // group 0 of the step's first row
    // first_group: the index in `out` of the step's first element group
    __device__ __forceinline__ RowStore(f32x4* __restrict__ out, uint64_t first_group) : first(out + first_group) {}
    // group g of the step (row-in-step * dim4 + group-in-row)
    __device__ __forceinline__ void operator()(uint32_t g, const f32x4 v) const {
        if constexpr (CACHED) first[g] = v;
        else __builtin_nontemporal_store(v, first + g);
    }
};

// ---- bf16 ROWS (SPEC.md §3 "Row storage type"): a table whose value plane holds bf16 ----------------------------------------------
// The element group a lane owns — 4 elements — is 8 bytes there: group g of slot s sits at index s * dim4 + g of a u32x2 array, the SAME index
// the fp32 kernels use on their float4 array.  Widening is exact: the 16 stored bits become the upper half of the fp32 word.
__device__ __forceinline__ f32x4 widen_bf16x4(const u32x2 p) {
    f32x4 v;
    v.x = __builtin_bit_cast(float, p.x << 16); v.y = __builtin_bit_cast(float, (p.x >> 16) << 16);
    v.z = __builtin_bit_cast(float, p.y << 16); v.w = __builtin_bit_cast(float, (p.y >> 16) << 16);
    return v;
}

// ---- int8 ROWS (SPEC.md §3 "Row storage type"): a table whose value plane holds int8 codes and one fp32 scale per row --------------------
// A slot's row is dim two's-complement codes followed by a 16-byte tail (the scale, then twelve zero bytes): dim4 + 4 words of 32 bits.  The element
// group a lane owns — 4 elements — is ONE word there: group g of slot s is word s * (dim4 + 4) + g, the row's scale is word s * (dim4 + 4) + dim4 (the
// same address in every lane of the tile, asked for next to the groups, never behind them).  All of it in 64 bits.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // one 16-byte group of a packed row
__device__ __forceinline__ uint64_t i8_row_word(int64_t slot, uint32_t dim4) { return (uint64_t)slot * ((uint64_t)dim4 + 4u); }
// D of the spec: y = (float)q * scale, one multiply per element (the library is built with -ffp-contract=off)
__device__ __forceinline__ f32x4 dequant_i8x4(uint32_t w, float scale) {
    f32x4 v;
    v.x = (float)(int8_t)(w & 0xFFu) * scale; v.y = (float)(int8_t)((w >> 8) & 0xFFu) * scale;
    v.z = (float)(int8_t)((w >> 16) & 0xFFu) * scale; v.w = (float)(int8_t)(w >> 24) * scale;
    return v;
}
// Q of the spec for four elements under the row's scale: a true division (no reciprocal), rint = ties to even, clamped to [-127, 127]; scale == 0: codes 0
__device__ __forceinline__ uint32_t quant_i8x4(const f32x4 x, float scale) {
    if (scale == 0.f) return 0u;
    const float e[4] = {x.x, x.y, x.z, x.w};
    uint32_t w = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float r = fminf(fmaxf(__builtin_rintf(e[k] / scale), -127.f), 127.f);
        w |= ((uint32_t)(int)r & 0xFFu) << (8 * k);
    }
    return w;
}

// ---- the row storage type of a lookup instance (SPEC.md §3 "Row storage type") -------------------------------------------------------
// A kernel's `bool BROWS` converts to kRowsF32 (false) / kRowsBF16 (true).  RowType<ROWS> is everything a lookup or the export knows about how a
// plane of that type holds a row; the geometry is the same for all three: a 16-lane tile per row, lane tl owns element group c * 16 + tl.
constexpr int kRowsF32 = 0, kRowsBF16 = 1, kRowsI8 = 2;
template <int ROWS>
struct RowType {
    static constexpr bool kI8 = ROWS == kRowsI8;
    static_assert(ROWS == kRowsF32 || ROWS == kRowsBF16 || kI8, "a row storage type");
    // the element group a lane loads — 4 elements: 16, 8 or 4 bytes
    using Group = std::conditional_t<ROWS == kRowsF32, f32x4, std::conditional_t<ROWS == kRowsBF16, u32x2, uint32_t>>;
    static __device__ __forceinline__ const Group* plane(const void* values) { return reinterpret_cast<const Group*>(values); }
    // group g of slot s is plane[first(s, dim4) + g]
    static __device__ __forceinline__ uint64_t first(int64_t slot, uint32_t dim4) {
        if constexpr (kI8) return i8_row_word(slot, dim4); else return (uint64_t)slot * dim4;
    }
    // STREAM: the streaming-rows policy of the find, a non-temporal load
    template <bool STREAM>
    static __device__ __forceinline__ Group load(const Group* p) {
        if constexpr (STREAM) return __builtin_nontemporal_load(p); else return *p;
    }
    // what a row needs loaded beside its groups: the scale word of an int8 row, by every lane of the tile (one address per tile) and issued WITH the
    // row's groups, never behind them; nothing (0) for the others.  HIT: the caller knows that the key was found (the load is unconditional), otherwise a
    // missing key (slot < 0) loads nothing
    template <bool STREAM, bool HIT>
    static __device__ __forceinline__ uint32_t load_tail(const Group* plane, int64_t slot, uint32_t dim4) {
        if constexpr (kI8) return (HIT || slot >= 0) ? load<STREAM>(plane + first(slot, dim4) + dim4) : 0u; else return 0u;
    }
    // What a missing key yields is the table's default row, def4.  An fp32 or bf16 plane can hold it as a Group (a bf16 table's default is a bf16 value:
    // packing it loses nothing), selected where the row would have been loaded; no scale makes int8 codes of it, so there the Group is 0 and value() puts
    // def4 in its place (`hit` and `def4` matter to an int8 row only).
    static __device__ __forceinline__ Group missing(const f32x4 def4) {
        if constexpr (ROWS == kRowsF32) return def4;
        else if constexpr (ROWS == kRowsBF16) return bf16x4_of(def4.x, def4.y, def4.z, def4.w);
        else return 0u;
    }
    // a group as fp32: as it is, widened (exact), or dequantized under the row's scale word
    static __device__ __forceinline__ f32x4 value(const Group g, uint32_t tail, bool hit, const f32x4 def4) {
        if constexpr (ROWS == kRowsF32) return g;
        else if constexpr (ROWS == kRowsBF16) return widen_bf16x4(g);
        else return hit ? dequant_i8x4(g, __builtin_bit_cast(float, tail)) : def4;
    }
    // the store of a group as element group idx of a bf16 output: a bf16 row's 8 bytes leave as they came (no second rounding), the others are rounded
    // here, once (store_bf16x4); CACHED as there
    template <bool CACHED>
    static __device__ __forceinline__ void store_bf16(void* __restrict__ out, uint64_t idx, const Group g, uint32_t tail, bool hit, const f32x4 def4) {
        if constexpr (ROWS != kRowsBF16) store_bf16x4<CACHED>(out, idx, value(g, tail, hit, def4));
        else if constexpr (CACHED) reinterpret_cast<u32x2*>(out)[idx] = g;
        else __builtin_nontemporal_store(g, reinterpret_cast<u32x2*>(out) + idx);
    }
    // ... of an fp32 or (BF16_OUT) bf16 output
    template <bool BF16_OUT, bool CACHED>
    static __device__ __forceinline__ void store(void* __restrict__ out, uint64_t idx, const Group g, uint32_t tail, bool hit, const f32x4 def4) {
        if constexpr (BF16_OUT) store_bf16<CACHED>(out, idx, g, tail, hit, def4);
        else {
            const f32x4 v = value(g, tail, hit, def4);
            RowStore<CACHED>(reinterpret_cast<f32x4*>(out), idx)(0, v);
        }
    }
};

// ---- pooled lookups (meepo_find.hip: one table and the uniform group; meepo_mixed.hip: the mixed group) ------------------------------
// a bag of this many keys or more is served by the wave's four tiles together (pooled_bags)
constexpr uint32_t kPoolLong = 16;

// probe + row load of up to U keys per tile (the find_kernel pattern); row[u] is only defined where inb[u].
// located (nullable) receives tag | slot per position: tag = member << kGroupSlotBits for a group (EMPTY when absent), or the table's
// handle tag (handle_tag_of) for one table with TAGGED (-1 when absent: the format of mee_find_located)
// ROWS: the storage type of `values` (RowType): a bf16 row is widened at its load, everything behind the load is the fp32 code
template <int DIM4, int U, int C, bool TAGGED = false, int ROWS = kRowsF32>
__device__ __forceinline__ void pooled_fetch(const int64_t* __restrict__ tkeys, const float4* __restrict__ values, uint64_t nb,
                                             uint32_t dim4, const int64_t (&key)[U], const uint64_t (&pos)[U],
                                             const bool (&inb)[U], int tile, int tl, float4 def4, float4 (&row)[U][C],
                                             uint8_t* __restrict__ found, int64_t* __restrict__ located = nullptr, uint64_t tag = 0) {
    static_assert(ROWS != kRowsI8, "no int8 pooled lookup: it faulted on the GPU and the cause is open (an int8 row also needs its scale word loaded and its default kept in fp32)");
    using RT = RowType<ROWS>;
    int64_t slot[U], kb[U];
    uint64_t bk[U];
    bool act[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        act[u] = inb[u] && !reserved_key(key[u]);
        bk[u] = bucket_of(key[u], nb);
        kb[u] = act[u] ? tkeys[bk[u] * kW + tl] : kEmpty;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u] = tile_probe(tkeys, nb, key[u], act[u], bk[u], kb[u], tile, tl);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                if constexpr (ROWS == kRowsF32) row[u][c] = slot[u] >= 0 ? values[(uint64_t)slot[u] * dim4 + c * 16 + tl] : def4;   // (a float4 plane as it is)
                else {
                    const f32x4 v = RT::value(slot[u] >= 0 ? RT::plane(values)[RT::first(slot[u], dim4) + c * 16 + tl] : RT::missing(f32x4{def4.x, def4.y, def4.z, def4.w}), 0u, true, f32x4{});
                    row[u][c] = make_float4(v.x, v.y, v.z, v.w);
                }
            }
        if (found && inb[u] && tl == 0) found[pos[u]] = slot[u] >= 0;
        // the located row: lets the backward skip its own probe pass
        if (located && inb[u] && tl == 0) located[pos[u]] = slot[u] >= 0 ? (int64_t)(tag | (uint64_t)slot[u]) : (TAGGED ? -1 : kEmpty);
    }
}

// The cold table of a hot/cold pair (mee_find_pooled_tiered), as the pooled kernel receives it beside the hot table's own planes.
struct TierArgs {
    const int64_t* tkeys;    // the cold index (HBM)
    const float4* values;    // the cold rows: device-mapped pinned host memory for a cold tier, read with plain loads (as find_missing_kernel does)
    uint64_t nb;
    uint32_t* hot_hits;      // per-slot hit counters of the two tables; null = that tier's hits are not counted
    uint32_t* cold_hits;
};

// pooled_fetch over a hot/cold pair: the row of a position is the hot table's if the hot table holds the key, else the cold table's if that
// one does, else def4 (the HOT table's default row); found = either tier holds it.  The U hot bucket lines are requested back to back and
// probed as in pooled_fetch; then ONE wave-uniform decision: a wave whose positions were all served by the hot table (the working set of a
// well-placed pair) pays that ballot and runs pooled_fetch's row loads.  Otherwise the cold index is probed for the positions the hot probe
// missed — by all 64 lanes in convergent control flow, tiles without a miss pass act = false — and each row is loaded from the plane that
// holds it (one load per row: the address is selected, not the data).  Counting (nullable counters, wave-uniform branches): one atomicAdd
// per found position by the tile's first lane, as find_kernel (kFindCountHits, meepo_find.hip) and find_missing_kernel (FLAGS & 2) do it.
// BY_FLAGS (a GROUP of pairs: the tiles of a wave may work for different members, so the hot planes, `cold` and its counters differ from tile to
// tile): whether a tier is counted is then read from the launch's `count` bits (kTierCountCold | kTierCountHot), never from a member's pointer —
// every wave-uniform branch stays on a fact of the whole launch.
constexpr uint32_t kTierCountCold = 1, kTierCountHot = 2;   // = MEE_TIER_COUNT_COLD / MEE_TIER_COUNT_HOT (include/meepo_embedding.h)
template <int DIM4, int U, int C, bool BY_FLAGS = false>
__device__ __forceinline__ void pooled_fetch_tiered(const int64_t* __restrict__ tkeys, const float4* __restrict__ values, uint64_t nb,
                                                    const TierArgs& cold, uint32_t dim4, const int64_t (&key)[U], const uint64_t (&pos)[U],
                                                    const bool (&inb)[U], int tile, int tl, float4 def4, float4 (&row)[U][C],
                                                    uint8_t* __restrict__ found, uint32_t count = 0) {
    const bool count_cold = BY_FLAGS ? (count & kTierCountCold) != 0 : cold.cold_hits != nullptr;
    const bool count_hot = BY_FLAGS ? (count & kTierCountHot) != 0 : cold.hot_hits != nullptr;
    int64_t slot[U], kb[U];
    uint64_t bk[U];
    bool act[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        act[u] = inb[u] && !reserved_key(key[u]);
        bk[u] = bucket_of(key[u], nb);
        kb[u] = act[u] ? tkeys[bk[u] * kW + tl] : kEmpty;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) slot[u] = tile_probe(tkeys, nb, key[u], act[u], bk[u], kb[u], tile, tl);
    bool missed = false;
#pragma unroll
    for (int u = 0; u < U; ++u) missed = missed || (act[u] && slot[u] < 0);
    if (!__any(missed)) {   // wave-uniform: nothing for the cold tier
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)
                    row[u][c] = slot[u] >= 0 ? values[(uint64_t)slot[u] * dim4 + c * 16 + tl] : def4;
            if (found && inb[u] && tl == 0) found[pos[u]] = slot[u] >= 0;
        }
    } else {
        int64_t cslot[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            act[u] = act[u] && slot[u] < 0;   // from here on: the positions the cold index is asked about
            bk[u] = bucket_of(key[u], cold.nb);
            kb[u] = act[u] ? cold.tkeys[bk[u] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) cslot[u] = tile_probe(cold.tkeys, cold.nb, key[u], act[u], bk[u], kb[u], tile, tl);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool hit = slot[u] >= 0 || cslot[u] >= 0;
            const float4* src = slot[u] >= 0 ? values + (uint64_t)slot[u] * dim4 : cold.values + (uint64_t)(cslot[u] >= 0 ? cslot[u] : 0) * dim4;
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)
                    row[u][c] = hit ? src[c * 16 + tl] : def4;
            if (found && inb[u] && tl == 0) found[pos[u]] = hit;
        }
        if (count_cold) {   // wave-uniform
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (cslot[u] >= 0 && tl == 0) atomicAdd(&cold.cold_hits[cslot[u]], 1u);
        }
    }
    if (count_hot) {   // wave-uniform (sampled calls)
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (slot[u] >= 0 && tl == 0) atomicAdd(&cold.hot_hits[slot[u]], 1u);
    }
}

// ---- the bag walk of the pooled lookups and of their backward ------------------------------------------------------------------
// Geometry: a wave step serves BPW consecutive bags.  BPW = 4: tile t takes bag `bag0 + t`; a bag of fewer than kPoolLong keys is walked by its
// tile alone, U positions a round (its keys and weights come with ONE coalesced load per tile, lane tl holds position begin + tl, and reach the
// rounds by shuffles); then every bag of kPoolLong keys or more is walked by the four tiles together, tile t on positions i + 4u + t.  BPW = 1: the
// wave walks bag0 that way whatever its length.  Three callers: find_pooled_kernel and pooled_weighted_backward_kernel (meepo_find.hip),
// mixed_find_pooled_kernel (meepo_mixed.hip).

// what a walk needs of the table a bag belongs to: its planes, its default row, and the tag of its located rows (pooled_fetch)
struct PooledTable {
    const int64_t* tkeys;
    const float4* values;
    uint64_t nb;
    float4 def4;
    uint64_t tag;
};

// ... of a group member: Desc = GroupDesc (meepo_host.h); its located rows carry the member above the slot bits
template <class Desc>
__device__ __forceinline__ PooledTable pooled_table(const Desc& d, uint64_t member, int slot_bits) {
    return PooledTable{d.tkeys, d.values, d.nb, make_float4(d.defv, d.defv, d.defv, d.defv), member << slot_bits};
}

// the key span of a bag.  Offsets are the caller's: a bag never reaches past the key array, and a decreasing pair is an empty bag
__device__ __forceinline__ void pooled_span(const uint64_t* __restrict__ offsets, uint64_t bag, bool has, uint64_t n_keys, uint64_t& begin, uint64_t& end) {
    begin = has ? offsets[bag] : 0; end = has ? offsets[bag + 1] : 0;
    end = end < n_keys ? end : n_keys;
    begin = begin < end ? begin : end;
}

// a short bag [begin, end) has fewer than 16 keys: lane tl of its tile loads key (and weight) begin + tl ...
template <bool WEIGHTED>
__device__ __forceinline__ void pooled_short_prefetch(const int64_t* __restrict__ keys, const float* __restrict__ weights, uint64_t begin, uint64_t end,
                                                      bool is_long, int tl, int64_t& kpre, float& wpre) {
    kpre = (!is_long && begin + tl < end) ? keys[begin + tl] : kEmpty;
    wpre = 0.f;
    if constexpr (WEIGHTED) wpre = (!is_long && begin + tl < end) ? weights[begin + tl] : 0.f;
}
// ... and a round of the tile takes positions i .. i + U - 1 out of those registers (wv only with WEIGHTED)
template <int U, bool WEIGHTED>
__device__ __forceinline__ void pooled_short_positions(uint64_t i, uint64_t begin, uint64_t end, int64_t kpre, float wpre, int tile, uint64_t (&pos)[U],
                                                       int64_t (&kv)[U], float (&wv)[U], bool (&inb)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        pos[u] = i + u; inb[u] = pos[u] < end;
        kv[u] = __shfl(kpre, tile * 16 + (int)((pos[u] - begin) & 15));
        if constexpr (WEIGHTED) wv[u] = __shfl(wpre, tile * 16 + (int)((pos[u] - begin) & 15));
    }
}
// a round of the four tiles on one long bag: positions i .. i + 4U - 1 (< eq), tile t takes i + 4u + t, the weight loaded next to the key
template <int U, bool WEIGHTED>
__device__ __forceinline__ void pooled_long_positions(uint64_t i, uint64_t eq, const int64_t* __restrict__ keys, const float* __restrict__ weights, int tile,
                                                      uint64_t (&pos)[U], int64_t (&kv)[U], float (&wv)[U], bool (&inb)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        pos[u] = i + (uint64_t)u * 4 + tile; inb[u] = pos[u] < eq; kv[u] = inb[u] ? keys[pos[u]] : kEmpty;
        if constexpr (WEIGHTED) wv[u] = inb[u] ? weights[pos[u]] : 0.f;
    }
}

// one element group of the next row joins the running sum: the product rounded first (WEIGHTED), then the sum, no fma (the library is built with
// -ffp-contract=off); the first row is ASSIGNED — a bag whose first row holds -0.0 keeps it
template <bool WEIGHTED>
__device__ __forceinline__ void pooled_add(float4& acc, float4 v, float w, bool first) {
    if constexpr (WEIGHTED) { v.x = w * v.x; v.y = w * v.y; v.z = w * v.z; v.w = w * v.w; }
    if (first) acc = v;
    else { acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w; }
}

// the finished row of a bag of `len` keys goes to the element groups out[o ...]: the mean's division only for a bag that has keys, and a bf16 row
// is rounded here, once
template <int DIM4, int C, bool BF16>
__device__ __forceinline__ void pooled_store(float4* __restrict__ out, uint64_t o, const float4 (&acc)[C], uint64_t len, int mean, uint32_t dim4, int tl) {
    const float flen = (float)len;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
            float4 v = acc[c];
            if (mean && len > 0) { v.x = v.x / flen; v.y = v.y / flen; v.z = v.z / flen; v.w = v.w / flen; }
            if constexpr (BF16) store_bf16x4<true>(out, o + c * 16 + tl, v); else out[o + c * 16 + tl] = v;
        }
}

// The bags one wave serves in one step of a pooled lookup (SPEC.md §3): bags bag0 .. bag0 + nvalid - 1 (nvalid <= BPW; bag0 exists), the row of bag b =
// the rows of its keys added up in position order (pooled_add), divided for the mean, stored at out[row_of(b) ...] (pooled_store).  The partial sum of
// a bag lives in registers, so a bag costs ONE output row.  In the long phase every tile adds the 4U rows of a round in position order out of the other
// tiles' registers (shuffles), so all four keep the same running sum and a long bag has 4U keys in flight instead of U.
// What differs between the callers comes in two callables:
//   table_of(b, PooledTable&) -> bool   fills in the table of bag b; false = the bag is to be treated as empty (a row of zeros, nothing probed)
//   row_of(b) -> uint64_t               the index of bag b's output row, in element groups
// With BPW = 4 the tiles of a wave may get different tables in the short phase; the long phase asks again for bag q and all four tiles switch to it.
// C: float4 per lane per row.  TAGGED: absent keys leave -1 in `located` (the format of mee_find_located), otherwise EMPTY.  TIERED: `tier` brings the
// cold table of a hot/cold pair, `located` is never read.  BROWS: the value planes hold bf16 rows, widened at their load (pooled_fetch).
// TIERED over a GROUP of pairs: the cold table belongs to the bag like the hot one, so table_of takes a third argument —
//   table_of(b, PooledTable&, TierArgs&) -> bool   also fills in the cold table (and, under the launch's count bits, the counters) of bag b's member
// — and `tier` is not read; `tier_count` carries the launch's count bits (kTierCountCold | kTierCountHot), the one thing about the tiers that is the
// same for every bag.  The cold table then switches wherever the hot one does: per tile in the short phase, to bag q's for all four tiles in the long one.
template <int DIM4, int U, int BPW, int C, bool WEIGHTED, bool BF16, bool TIERED, bool BROWS, bool TAGGED, class TableOf, class RowOf>
__device__ __forceinline__ void pooled_bags(uint64_t bag0, uint32_t nvalid, uint32_t dim4, const int64_t* __restrict__ keys, const uint64_t* __restrict__ offsets,
                                            uint64_t n_keys, const float* __restrict__ weights, float4* __restrict__ out, uint8_t* __restrict__ found,
                                            int64_t* __restrict__ located, int mean, const TierArgs& tier, int tile, int tl, TableOf&& table_of, RowOf&& row_of,
                                            uint32_t tier_count = 0) {
    constexpr bool TIER_PER_BAG = TIERED && std::is_invocable_v<TableOf&, uint64_t, PooledTable&, TierArgs&>;
    const uint64_t bag = BPW == 4 ? bag0 + tile : bag0;
    const bool has = BPW == 4 ? (uint32_t)tile < nvalid : true;
    uint64_t begin, end;
    pooled_span(offsets, bag, has, n_keys, begin, end);
    PooledTable t;
    TierArgs cold_of_bag;   // (TIER_PER_BAG only)
    auto table = [&](uint64_t b) {
        if constexpr (TIER_PER_BAG) return table_of(b, t, cold_of_bag);
        else return table_of(b, t);
    };
    if (!table(has ? bag : bag0)) begin = end = 0;
    const bool is_long = BPW == 1 || end - begin >= kPoolLong;
    float4 acc[C];
    float4 row[U][C];
    auto fetch = [&](const int64_t (&kv)[U], const uint64_t (&pos)[U], const bool (&inb)[U]) {
        if constexpr (TIER_PER_BAG) pooled_fetch_tiered<DIM4, U, C, true>(t.tkeys, t.values, t.nb, cold_of_bag, dim4, kv, pos, inb, tile, tl, t.def4, row, found, tier_count);
        else if constexpr (TIERED) pooled_fetch_tiered<DIM4, U, C>(t.tkeys, t.values, t.nb, tier, dim4, kv, pos, inb, tile, tl, t.def4, row, found);
        else pooled_fetch<DIM4, U, C, TAGGED, BROWS ? kRowsBF16 : kRowsF32>(t.tkeys, t.values, t.nb, dim4, kv, pos, inb, tile, tl, t.def4, row, found, located, t.tag);
    };
    // ---- short bags: one tile per bag ----
    if constexpr (BPW == 4) {
        uint64_t i = is_long ? end : begin;
        bool first = true;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        int64_t kpre;
        float wpre;
        pooled_short_prefetch<WEIGHTED>(keys, weights, begin, end, is_long, tl, kpre, wpre);
        while (__any(i < end)) {  // wave-uniform; tiles whose bag is done idle through the ballots
            uint64_t pos[U];
            int64_t kv[U];
            float wv[U];
            bool inb[U];
            pooled_short_positions<U, WEIGHTED>(i, begin, end, kpre, wpre, tile, pos, kv, wv, inb);
            fetch(kv, pos, inb);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!inb[u]) continue;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) pooled_add<WEIGHTED>(acc[c], row[u][c], WEIGHTED ? wv[u] : 0.f, first);
                first = false;
            }
            i += U;
        }
        if (has && !is_long) pooled_store<DIM4, C, BF16>(out, row_of(bag), acc, end - begin, mean, dim4, tl);
    }
    // ---- long bags: the four tiles share one bag at a time ----
    const uint64_t long_mask = __ballot(is_long && has);
    if (!long_mask) return;   // wave-uniform
    for (int q = 0; q < BPW; ++q) {
        if (!((long_mask >> (q * 16)) & 1)) continue;   // wave-uniform
        // the span of bag q to every lane.  BPW = 1: every lane holds bag0's span already; using it without the broadcast is what keeps the bf16-row
        // group's dim-128 instance at 7 waves per SIMD.  Not for the tiered instances: without the broadcast, as it is or as a scalar (readfirstlane),
        // the pair's lookup on bags of 20 measures 5 % slower than with it — same occupancy, cause not found (profiles/pooled_shared_body.md §2)
        constexpr bool OWN_SPAN = BPW == 1 && !TIERED;
        const uint64_t bq = OWN_SPAN ? begin : __shfl(begin, q * 16), eq = OWN_SPAN ? end : __shfl(end, q * 16);
        if constexpr (BPW == 4) (void)table(bag0 + q);   // all four tiles work for bag q's table now (a long bag is not empty)
        bool first = true;
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (uint64_t i = bq; i < eq; i += 4 * U) {   // wave-uniform
            uint64_t pos[U];
            int64_t kv[U];
            float wv[U];
            bool inb[U];
            pooled_long_positions<U, WEIGHTED>(i, eq, keys, weights, tile, pos, kv, wv, inb);
            fetch(kv, pos, inb);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int src = 0; src < 4; ++src) {
                    if (i + (uint64_t)u * 4 + src >= eq) continue;   // wave-uniform
                    float w = 0.f;
                    if constexpr (WEIGHTED) w = __shfl(wv[u], src * 16 + tl);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        float4 v;   // every tile reads the row tile `src` fetched
                        v.x = __shfl(row[u][c].x, src * 16 + tl); v.y = __shfl(row[u][c].y, src * 16 + tl);
                        v.z = __shfl(row[u][c].z, src * 16 + tl); v.w = __shfl(row[u][c].w, src * 16 + tl);
                        pooled_add<WEIGHTED>(acc[c], v, w, first);
                    }
                    first = false;
                }
        }
        if (tile == 0) pooled_store<DIM4, C, BF16>(out, row_of(bag0 + q), acc, eq - bq, mean, dim4, tl);
    }
}

// ---- the keyed layout of the pooled group lookups (SPEC.md §3 "Keyed output") ---------------------------------------------------------
// What a keyed launch gets beside the table-major launch's arguments: the output's row stride in element groups (float4 for fp32, 8 bytes for bf16),
// the step index array (nullable) and the two factors of its value, step = sample * step_sample + member * step_member — (T, 1) for the uniform
// step, which reads the keyed gradient as [B * T, dim]; (1, B) = the bag itself for a mixed group's.
struct KeyedOut {
    uint64_t stride4;
    uint32_t* step_index;
    uint64_t step_sample, step_member;
};
// a kernel's last argument T with KeyedOut behind it (KEYED), or T itself: the table-major instances keep their argument list
template <class T> struct WithKeyed : T { KeyedOut keyed; };
template <bool KEYED, class T> using KeyedArg = std::conditional_t<KEYED, WithKeyed<T>, T>;

// The step index of the bags one wave serves in one step (pooled_bags' geometry: BPW = 4, tile t has bag0 + t; BPW = 1, the wave has bag0): every key
// position the bag covers — its span as the walk clamps it (pooled_span) — gets the bag's `row`, 16 (64) consecutive positions per store.  Written
// beside the walk, not inside it: pooled_bags and the instances without a step index stay the code they were.  row_of_bag(b) -> uint32_t.
template <int BPW, class RowOfBag>
__device__ __forceinline__ void keyed_step_index(uint64_t bag0, uint32_t nvalid, const uint64_t* __restrict__ offsets, uint64_t n_keys, int tile, int tl,
                                                 uint32_t* __restrict__ step_index, RowOfBag&& row_of_bag) {
    const uint64_t bag = BPW == 4 ? bag0 + tile : bag0;
    const bool has = BPW == 4 ? (uint32_t)tile < nvalid : true;
    uint64_t begin = has ? offsets[bag] : 0, end = has ? offsets[bag + 1] : 0;
    end = end < n_keys ? end : n_keys;
    begin = begin < end ? begin : end;
    if (begin == end) return;
    const uint32_t row = row_of_bag(bag);
    const int lanes = BPW == 4 ? 16 : 64, l = BPW == 4 ? tl : tile * 16 + tl;
    for (uint64_t i = begin + l; i < end; i += lanes) step_index[i] = row;
}

// SPEC.md §3 "Initial row", four consecutive elements starting at j0
__device__ __forceinline__ float4 initial_row4(int64_t key, uint32_t j0, uint32_t initializer, float init_scale,
                                               uint64_t init_seed, float default_value) {
    if (initializer == 0) return make_float4(default_value, default_value, default_value, default_value);
    float r[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t h = mix64((uint64_t)key ^ mix64(init_seed + j0 + q));
        const float u = (float)(h >> 40) * 0x1p-24f;
        r[q] = init_scale * (2.0f * u - 1.0f);
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}

// SPEC.md §4 (explicit fma only where the spec writes it; file is compiled with -ffp-contract=off)
__device__ __forceinline__ void adagrad1(float& w, float& a, float g, float lr, float eps) {
    const float an = __builtin_fmaf(g, g, a);
    const float q = g / (__builtin_sqrtf(an) + eps);
    w = __builtin_fmaf(-lr, q, w);
    a = an;
}
__device__ __forceinline__ void adam1(float& w, float& m, float& v, float g, float step_size, float omb1, float omb2,
                                      float eps) {
    const float mn = __builtin_fmaf(omb1, g - m, m);
    const float gg = g * g;
    const float vn = __builtin_fmaf(omb2, gg - v, v);
    const float q = mn / (__builtin_sqrtf(vn) + eps);
    w = __builtin_fmaf(-step_size, q, w);
    m = mn; v = vn;
}
// FTRL-Proximal (SPEC.md §4): z in plane 1, n in plane 2; every line one fp32 operation rounded on its own, no fma
__device__ __forceinline__ void ftrl1(float& w, float& z, float& n, float g, float lr, float beta, float l1, float l2) {
    const float gg = g * g;
    const float nn = n + gg;
    const float sn = __builtin_sqrtf(nn);
    const float sig = (sn - __builtin_sqrtf(n)) / lr;
    const float sw = sig * w;
    const float zn = (z + g) - sw;
    const float den = (beta + sn) / lr + l2;
    w = __builtin_fabsf(zn) <= l1 ? 0.0f : (__builtin_copysignf(l1, zn) - zn) / den;   // (a NaN z' fails the comparison and propagates)
    z = zn; n = nn;
}
// an optimizer with a second state plane (s2): Adam's v, FTRL's n
__host__ __device__ constexpr bool opt_has_s2(uint32_t kind) { return kind == MEE_OPT_ADAM || kind == MEE_OPT_FTRL; }

// ---- the creation of a key, said once -----------------------------------------------------------------------------------------------------------
// What a tile does once tile_locate<claim> has given it `slot` (>= 0) of `key` in the table (d: its planes and default value — GroupDesc; in: its
// initializer, optimizer and hit counters — GroupInit, meepo_host.h): with ROWS_OUT every such tile — the one whose CAS created the key and one that met
// a duplicate's creation alike — writes the key's initial row, a function of the key and the table's initializer alone, into row i of `out` (BF16: that
// copy is rounded, the stored row is not), so nothing has to read the created rows back; the creator (is_new) also writes the table's row, the
// initial Adagrad, Adam or FTRL state and a zero hit counter.
template <bool ROWS_OUT, bool BF16, class Desc, class Init>
__device__ __forceinline__ void creation_write(const Desc& d, const Init& in, uint32_t dim4, int64_t key, int64_t slot, bool is_new, float4* __restrict__ out,
                                               uint64_t i, int tl) {
    if (ROWS_OUT || is_new) {
        for (uint32_t c = tl; c < dim4; c += 16) {
            const float4 row = initial_row4(key, c * 4, in.initializer, in.init_scale, in.init_seed, d.defv);
            if constexpr (ROWS_OUT) {
                if constexpr (BF16) store_bf16x4<true>(out, i * dim4 + c, row); else out[i * dim4 + c] = row;
            }
            if (is_new) {
                d.values[(uint64_t)slot * dim4 + c] = row;
                if (in.optimizer == MEE_OPT_ADAGRAD) d.s1[(uint64_t)slot * dim4 + c] = make_float4(in.init_acc, in.init_acc, in.init_acc, in.init_acc);
                if (opt_has_s2(in.optimizer)) {   // Adam: m = v = 0; FTRL: z = 0, n = initial_accumulator
                    const float n0 = in.optimizer == MEE_OPT_FTRL ? in.init_acc : 0.f;
                    d.s1[(uint64_t)slot * dim4 + c] = make_float4(0.f, 0.f, 0.f, 0.f);
                    d.s2[(uint64_t)slot * dim4 + c] = make_float4(n0, n0, n0, n0);
                }
            }
        }
    }
    if (is_new && in.hits && tl == 0) in.hits[slot] = 0;
}

// The creation pass of every grouped find_or_insert (the kernels are thin wrappers: meepo_group.hip, meepo_mixed.hip): each position of the jagged
// batch that the found mask leaves missing claims (or finds, when a duplicate got there first) its key's slot in its member's table — one creator per
// distinct key, the CAS decides — and creation_write does the rest.  One tile per position; a wave with nothing missing leaves at the first
// wave-uniform `continue` (the steady state of a trained vocabulary).  What differs between the operators comes in as a callable:
//   member_of(lo, live) -> {d, in, dim4}: pointers to the descriptor and the init record member lo creates in (for a group of pairs: of the tier
//                          to_cold selects) and its row width; `live` = the position has a key to create or a tombstone to flag.  RESERVED_KEY (a
//                          RECLAIMED key in the batch; EMPTY is padding, silent) and TABLE_FULL go to that record's status word.
//   gate(lo, key) -> bool:  whether a missing key of member lo may be created at all (admission: the creations over a group of pairs, meepo_group.hip).
//                          It stands behind the tombstone's flag and in front of the second `continue`, so a wave whose missing keys were all turned
//                          away leaves there; a position turned away keeps what the lookup wrote.  NoGate, the default, is no code at all.
//                          (ensure_admit_grouped_kernel, meepo_group.hip, keeps its own text with its gate in the same place.)
struct NoGate {};
template <bool ROWS_OUT, bool BF16, class MemberOf, class Gate = NoGate>
__device__ __forceinline__ void ensure_grouped_body(uint64_t* loff, uint32_t n_tables, const uint64_t* __restrict__ offsets, uint64_t off_stride,
                                                    const int64_t* __restrict__ keys, uint64_t n, const uint8_t* __restrict__ found,
                                                    float4* __restrict__ out, MemberOf&& member_of, Gate gate = Gate{}) {
    stage_offsets(loff, offsets, off_stride, n_tables, n);
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 4; base < n; base += n_waves * 4) {
        const uint64_t i = base + tile;
        bool act = i < n && i >= loff[0] && i < loff[n_tables] && found[i] == 0;
        const int64_t key = act ? keys[i] : kEmpty;
        const bool tomb = act && key == kReclaimed;
        act = act && !reserved_key(key);
        if (!__any(act || tomb)) continue;  // wave-uniform: nothing missing here
        const uint32_t lo = member_of_position(loff, n_tables, i);
        const auto m = member_of(lo, act || tomb);
        if (tomb && tl == 0) atomicOr(m.in->status, (uint32_t)MEE_STATUS_RESERVED_KEY);
        if constexpr (!std::is_same_v<Gate, NoGate>) {
            if (act) act = gate(lo, key);
        }
        if (!__any(act)) continue;  // wave-uniform: a tombstone was all there was (or nobody passed the gate)
        const auto d = *m.d;
        bool is_new, full;
        const int64_t slot = tile_locate<true, true>(const_cast<int64_t*>(d.tkeys), d.nb, key, act, tile, tl, is_new, full);
        if (act) {
            const auto in = *m.in;
            if (slot >= 0) creation_write<ROWS_OUT, BF16>(d, in, m.dim4, key, slot, is_new, out, i, tl);
            if (full && tl == 0) atomicOr(in.status, (uint32_t)MEE_STATUS_TABLE_FULL);
        }
    }
}

}  // namespace mee
