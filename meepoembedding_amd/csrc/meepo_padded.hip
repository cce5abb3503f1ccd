// meepo_padded.hip — the padded sequence lookup (SPEC.md §3 "find_padded"): one table or a uniform group, a hot/cold pair or a group of pairs; one launch.
// out[b, j, :] = the row of bag b's j-th KEPT key, zeros behind the end of a short bag; a bag longer than max_len keeps its first or its last
// max_len keys.  The row bytes cross HBM once: no [n, dim] array between the table and the [n_bags, max_len, dim] block a sequence model reads.
#include <hip/hip_runtime.h>

#include "meepo_table_int.h"

namespace mee {

// the per-position and per-bag outputs of a padded lookup, every one nullable (kernel-uniform conditions)
struct PaddedOuts {
    uint8_t* found;         // [n]
    int64_t* lengths;       // [n_bags]
    int64_t* step_keys;     // [n]
    uint32_t* grad_index;   // [n]
};

// r / d for r < d + 16: what one of a wave step's (at most 16) consecutive slots lies beyond the step's first bag.  No 64-bit division per tile
__device__ __forceinline__ uint32_t small_quot(uint64_t r, uint64_t d) { return d >= 16 ? (uint32_t)(r >= d) : (uint32_t)r / (uint32_t)d; }

// Geometry: the work item is an output SLOT s = b * L + j — one 16-lane tile per slot, U slots in flight per tile, a wave step takes the 4U consecutive
// slots base .. base + 4U - 1 (the find kernel's shape: the slots of a step are one contiguous piece of `out`).  Nothing is carried from slot to slot,
// so no tile waits for another and a bag's length does not matter to the balance: a kept position costs its tile one probe and one row, a slot behind the
// end of its bag a row of zeros.  Bag and slot-in-bag of the step's first slot come from ONE wave-uniform 64-bit division, the tiles' from small_quot.
// The truncated positions of a bag longer than L (found 0, step key EMPTY, grad index 0: three small stores each, no probe) are shared out among the
// bag's L slots: slot j takes the j-th piece of ceil((len - L) / L) consecutive positions, its 16 lanes side by side — a bag of 10 000 positions cut to
// 50 is the work of 50 tiles, 13 rounds each.
// GROUPED: bag b is member b / bags_per_table's (its planes, its default row); one slot in flight per tile, since the table is per slot.
// BROWS: the planes hold bf16 rows; with BF16 as well the stored bits leave as they are.  CACHED: plain result stores, otherwise streaming ones.
template <int DIM4, int U, bool GROUPED, bool BF16, bool BROWS, bool CACHED>
__global__ __launch_bounds__(256) void find_padded_kernel(const int64_t* __restrict__ tkeys_, const float4* __restrict__ values_, uint64_t nb_, float defv,
                                                          uint32_t dim4_rt, const GroupDesc* __restrict__ desc, uint64_t bags_per_table,
                                                          const int64_t* __restrict__ keys, uint64_t n_keys, const uint64_t* __restrict__ offsets,
                                                          uint64_t n_bags, uint64_t L, uint32_t keep_last, void* __restrict__ out, PaddedOuts o) {
    static_assert(!GROUPED || U == 1, "a group's slots bring their own table: one in flight per tile");
    static_assert(U >= 1 && U <= 4, "small_quot serves steps of at most 16 slots");
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 16;   // float4 per lane per row (any dim: up to 1024 floats = 16 per lane)
    constexpr int SPW = 4 * U;
    const uint64_t n_slots = n_bags * L;       // (the entry points refuse a product beyond 2^56)
    const bool per_position = o.found || o.step_keys || o.grad_index;

    for (uint64_t base_ = wave * SPW; base_ < n_slots; base_ += n_waves * SPW) {
        // (uniform anyway: says so to the compiler, the division stays off the vector unit where it can)
        const uint64_t base = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)base_) | ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(base_ >> 32)) << 32);
        const uint64_t b0 = base / L, r0 = base - b0 * L;
        uint64_t m0 = 0, mr0 = 0;
        if constexpr (GROUPED) { m0 = b0 / bags_per_table; mr0 = b0 - m0 * bags_per_table; }
        PooledTable t = PooledTable{tkeys_, values_, nb_, make_float4(defv, defv, defv, defv), 0};
        uint64_t pos[U], bag[U], j[U], begin[U], len[U];
        int64_t kv[U];
        bool has[U], live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = r0 + (uint64_t)(u * 4 + tile);
            const uint32_t q = small_quot(r, L);
            has[u] = base + (uint64_t)(u * 4 + tile) < n_slots;
            bag[u] = has[u] ? b0 + q : b0;
            j[u] = r - (uint64_t)q * L;
            uint64_t end;
            pooled_span(offsets, bag[u], has[u], n_keys, begin[u], end);
            len[u] = end - begin[u];
            const uint64_t kept = len[u] < L ? len[u] : L;
            live[u] = has[u] && j[u] < kept;
            pos[u] = (keep_last ? end - kept : begin[u]) + j[u];
            kv[u] = live[u] ? keys[pos[u]] : kEmpty;
            if (o.lengths && has[u] && j[u] == 0 && tl == 0) o.lengths[bag[u]] = (int64_t)kept;
            if constexpr (GROUPED) {
                const uint64_t member = has[u] ? m0 + small_quot(mr0 + q, bags_per_table) : m0;
                t = pooled_table(desc[member], member, kGroupSlotBits);
            }
        }
        float4 row[U][C];
        pooled_fetch<DIM4, U, C, false, BROWS ? kRowsBF16 : kRowsF32>(t.tkeys, t.values, t.nb, dim4, kv, pos, live, tile, tl, t.def4, row, o.found);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!has[u]) continue;
            const uint64_t s = base + (uint64_t)(u * 4 + tile);
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                    const uint64_t idx = s * dim4 + (uint32_t)(c * 16 + tl);   // 64-bit: n_bags * L * dim may pass 2^32
                    const float4 r4 = live[u] ? row[u][c] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const f32x4 v = {r4.x, r4.y, r4.z, r4.w};
                    if constexpr (BF16 && BROWS) {   // a widened bf16 row: its upper halves ARE the stored bits (no second rounding, NaN payloads kept)
                        u32x2 p;
                        p.x = (__float_as_uint(r4.x) >> 16) | (__float_as_uint(r4.y) & 0xFFFF0000u);
                        p.y = (__float_as_uint(r4.z) >> 16) | (__float_as_uint(r4.w) & 0xFFFF0000u);
                        if constexpr (CACHED) reinterpret_cast<u32x2*>(out)[idx] = p;
                        else __builtin_nontemporal_store(p, reinterpret_cast<u32x2*>(out) + idx);
                    } else if constexpr (BF16) store_bf16x4<CACHED>(out, idx, v);
                    else RowStore<CACHED>(reinterpret_cast<f32x4*>(out), idx)(0, v);
                }
            if (live[u] && tl == 0) {
                if (o.step_keys) o.step_keys[pos[u]] = kv[u];
                if (o.grad_index) o.grad_index[pos[u]] = (uint32_t)s;   // (asked for only with n_bags * L < 2^31)
            }
            if (per_position && len[u] > L) {   // the slot's share of its bag's truncated positions
                const uint64_t cut = len[u] - L, per = (cut + L - 1) / L;
                const uint64_t first = keep_last ? begin[u] : begin[u] + L;
                const uint64_t t0 = j[u] * per, t1 = t0 + per < cut ? t0 + per : cut;
                for (uint64_t x = t0 + (uint64_t)tl; x < t1; x += 16) {
                    if (o.found) o.found[first + x] = 0;
                    if (o.step_keys) o.step_keys[first + x] = kEmpty;
                    if (o.grad_index) o.grad_index[first + x] = 0u;
                }
            }
        }
    }
}

// The same lookup over a hot/cold pair (mee_find_padded_tiered: the table arguments are the HOT table's, `tier` is a TierArgs with the cold one and the
// counters that this launch feeds, null = not counted) or, GROUPED, over a group of pairs (mee_group_find_padded_tiered: `desc` holds the hot members,
// `tier` is a GroupTier; the slot's pair is (s / L) / bags_per_table, whose cold keys, rows and counters come per tile, group_pair_tables).  fp32 rows.
// The fetch is pooled_fetch_tiered: hot probe, ONE wave-uniform decision, the cold probe for what the hot one missed, each row from the plane that holds
// it, a key in neither tier the HOT table's default row.  The tiles of a wave may work for different pairs, so whether a tier is counted is read from
// the launch's count bits (BY_FLAGS), never from a member's pointer.
// The slot geometry, the store of a slot and the truncated share are find_padded_kernel's, REPEATED here and not shared through a function: with
// the body of both kernels behind one __forceinline__ function (or its three pieces behind three) none of find_padded_kernel's 48 instances kept its
// code — the compiler simplifies every function on its own before it inlines — and its group instances then measured 5-8 % slower than before
// (profiles/find_padded_tiered.md §1).  A change to the geometry, the clamping, the store or the share has to be made in both kernels;
// tests/test_find_padded_tiered.py compares the two bit for bit, output by output.
template <int DIM4, int U, bool GROUPED, bool BF16, bool CACHED>
__global__ __launch_bounds__(256) void find_padded_tiered_kernel(const int64_t* __restrict__ tkeys_, const float4* __restrict__ values_, uint64_t nb_, float defv,
                                                                 uint32_t dim4_rt, const GroupDesc* __restrict__ desc, uint64_t bags_per_table,
                                                                 const int64_t* __restrict__ keys, uint64_t n_keys, const uint64_t* __restrict__ offsets,
                                                                 uint64_t n_bags, uint64_t L, uint32_t keep_last, void* __restrict__ out, PaddedOuts o,
                                                                 std::conditional_t<GROUPED, GroupTier, TierArgs> tier) {
    static_assert(!GROUPED || U == 1, "a group's slots bring their own pair: one in flight per tile");
    static_assert(U >= 1 && U <= 4, "small_quot serves steps of at most 16 slots");
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 16;
    constexpr int SPW = 4 * U;
    const uint64_t n_slots = n_bags * L;
    const bool per_position = o.found || o.step_keys || o.grad_index;

    for (uint64_t base_ = wave * SPW; base_ < n_slots; base_ += n_waves * SPW) {
        const uint64_t base = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)base_) | ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(base_ >> 32)) << 32);
        const uint64_t b0 = base / L, r0 = base - b0 * L;
        uint64_t m0 = 0, mr0 = 0;
        if constexpr (GROUPED) { m0 = b0 / bags_per_table; mr0 = b0 - m0 * bags_per_table; }
        PooledTable t = PooledTable{tkeys_, values_, nb_, make_float4(defv, defv, defv, defv), 0};
        TierArgs cold;
        if constexpr (!GROUPED) cold = tier;
        uint64_t pos[U], bag[U], j[U], begin[U], len[U];
        int64_t kv[U];
        bool has[U], live[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint64_t r = r0 + (uint64_t)(u * 4 + tile);
            const uint32_t q = small_quot(r, L);
            has[u] = base + (uint64_t)(u * 4 + tile) < n_slots;
            bag[u] = has[u] ? b0 + q : b0;
            j[u] = r - (uint64_t)q * L;
            uint64_t end;
            pooled_span(offsets, bag[u], has[u], n_keys, begin[u], end);
            len[u] = end - begin[u];
            const uint64_t kept = len[u] < L ? len[u] : L;
            live[u] = has[u] && j[u] < kept;
            pos[u] = (keep_last ? end - kept : begin[u]) + j[u];
            kv[u] = live[u] ? keys[pos[u]] : kEmpty;
            if (o.lengths && has[u] && j[u] == 0 && tl == 0) o.lengths[bag[u]] = (int64_t)kept;
            if constexpr (GROUPED) {   // (a slot past the end stays with the step's first pair: a member inside the group, nothing probed)
                const uint64_t member = has[u] ? m0 + small_quot(mr0 + q, bags_per_table) : m0;
                group_pair_tables(desc, tier, member, t, cold);
            }
        }
        float4 row[U][C];
        if constexpr (GROUPED) pooled_fetch_tiered<DIM4, U, C, true>(t.tkeys, t.values, t.nb, cold, dim4, kv, pos, live, tile, tl, t.def4, row, o.found, tier.count);
        else pooled_fetch_tiered<DIM4, U, C>(t.tkeys, t.values, t.nb, cold, dim4, kv, pos, live, tile, tl, t.def4, row, o.found);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!has[u]) continue;
            const uint64_t s = base + (uint64_t)(u * 4 + tile);
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                    const uint64_t idx = s * dim4 + (uint32_t)(c * 16 + tl);   // 64-bit: n_bags * L * dim may pass 2^32
                    const float4 r4 = live[u] ? row[u][c] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const f32x4 v = {r4.x, r4.y, r4.z, r4.w};
                    if constexpr (BF16) store_bf16x4<CACHED>(out, idx, v);
                    else RowStore<CACHED>(reinterpret_cast<f32x4*>(out), idx)(0, v);
                }
            if (live[u] && tl == 0) {
                if (o.step_keys) o.step_keys[pos[u]] = kv[u];
                if (o.grad_index) o.grad_index[pos[u]] = (uint32_t)s;   // (asked for only with n_bags * L < 2^31)
            }
            if (per_position && len[u] > L) {   // the slot's share of its bag's truncated positions
                const uint64_t cut = len[u] - L, per = (cut + L - 1) / L;
                const uint64_t first = keep_last ? begin[u] : begin[u] + L;
                const uint64_t t0 = j[u] * per, t1 = t0 + per < cut ? t0 + per : cut;
                for (uint64_t x = t0 + (uint64_t)tl; x < t1; x += 16) {
                    if (o.found) o.found[first + x] = 0;
                    if (o.step_keys) o.step_keys[first + x] = kEmpty;
                    if (o.grad_index) o.grad_index[first + x] = 0u;
                }
            }
        }
    }
}

// a block the Infinity Cache holds is read from there by the model's next kernel: plain stores; a larger one streams (profiles/find_write_through.md)
static bool padded_cached(uint64_t n_slots, uint32_t dim4, uint32_t out_dtype) { return n_slots * dim4 * (out_dtype == MEE_DTYPE_BF16 ? 8u : 16u) <= kCachedOutputBytes; }

// the launch of either form: the row shape, the output type, the row type and the store policy pick the instance; `keep` and the optional outputs
// are kernel arguments
template <bool GROUPED>
static void padded_launch(const mee_table* t, const mee_group* g, uint32_t dim4, bool bf16_rows, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                          uint64_t n_bags, uint64_t bags_per_table, uint64_t max_len, uint32_t flags, void* d_out, uint32_t out_dtype, const PaddedOuts& o,
                          hipStream_t st) {
    const uint64_t n_slots = n_bags * max_len;
    const bool cached = padded_cached(n_slots, dim4, out_dtype);
    with_row_shape(dim4, [&](auto d4) { with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_flag(bf16_rows, [&](auto brows) { with_flag(cached, [&](auto ca) {
        constexpr int U = GROUPED ? 1 : RowShape<d4>::rows_per_tile;
        const unsigned grid = grid_for(n_slots, 4 * 4 * U, 1u << 20);
        if constexpr (GROUPED)
            find_padded_kernel<d4, U, true, bf16, brows, ca><<<grid, 256, 0, st>>>(nullptr, nullptr, 0, 0.f, dim4, g->d_desc, bags_per_table, d_keys, n, d_bag_offsets, n_bags, max_len,
                                                                                   flags & MEE_PAD_KEEP_LAST, d_out, o);
        else
            find_padded_kernel<d4, U, false, bf16, brows, ca><<<grid, 256, 0, st>>>(t->keys, (const float4*)t->values, t->nb, t->default_value, dim4, nullptr, 1, d_keys, n, d_bag_offsets,
                                                                                    n_bags, max_len, flags & MEE_PAD_KEEP_LAST, d_out, o);
    }); }); }); });
}

// ... of the tiered forms: one pair (hot, cold; the counters of the tiers this launch counts in its TierArgs) or a group of pairs (hot_g, cold_g; the
// count bits in its GroupTier)
template <bool GROUPED>
static void padded_tiered_launch(const mee_table* hot, const mee_table* cold, const mee_group* hot_g, const mee_group* cold_g, uint32_t dim4, uint32_t count_flags,
                                 const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, uint64_t n_bags, uint64_t bags_per_table, uint64_t max_len, uint32_t flags,
                                 void* d_out, uint32_t out_dtype, const PaddedOuts& o, hipStream_t st) {
    const uint64_t n_slots = n_bags * max_len;
    const bool cached = padded_cached(n_slots, dim4, out_dtype);
    with_row_shape(dim4, [&](auto d4) { with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_flag(cached, [&](auto ca) {
        constexpr int U = GROUPED ? 1 : RowShape<d4>::rows_per_tile;
        const unsigned grid = grid_for(n_slots, 4 * 4 * U, 1u << 20);
        if constexpr (GROUPED) {
            const GroupTier tier{cold_g->d_desc, hot_g->d_init, cold_g->d_init, count_flags};
            find_padded_tiered_kernel<d4, U, true, bf16, ca><<<grid, 256, 0, st>>>(nullptr, nullptr, 0, 0.f, dim4, hot_g->d_desc, bags_per_table, d_keys, n, d_bag_offsets, n_bags, max_len,
                                                                                   flags & MEE_PAD_KEEP_LAST, d_out, o, tier);
        } else {
            const TierArgs tier{cold->keys, (const float4*)cold->values, cold->nb, (count_flags & MEE_TIER_COUNT_HOT) ? hot->hits : nullptr,
                                (count_flags & MEE_TIER_COUNT_COLD) ? cold->hits : nullptr};
            find_padded_tiered_kernel<d4, U, false, bf16, ca><<<grid, 256, 0, st>>>(hot->keys, (const float4*)hot->values, hot->nb, hot->default_value, dim4, nullptr, 1, d_keys, n,
                                                                                    d_bag_offsets, n_bags, max_len, flags & MEE_PAD_KEEP_LAST, d_out, o, tier);
        }
    }); }); });
}

// what every entry point checks about the shape of the call, before anything is launched or written
static int padded_check(const char* name, bool bags, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, uint64_t n_bags, size_t max_len, uint32_t flags,
                        const void* d_out, uint32_t out_dtype, const uint32_t* d_grad_index_out) {
    if ((bags && (!d_bag_offsets || !d_out)) || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (max_len == 0) return fail(MEE_ERR_INVALID_ARG, "%s: max_len must be at least 1", name);
    if (flags & ~(uint32_t)MEE_PAD_KEEP_LAST) return fail(MEE_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x (MEE_PAD_KEEP_FIRST or MEE_PAD_KEEP_LAST)", name, flags);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    uint64_t n_slots = 0;
    if (__builtin_mul_overflow(n_bags, (uint64_t)max_len, &n_slots) || n_slots > (1ull << 56))
        return fail(MEE_ERR_INVALID_ARG, "%s: n_bags * max_len is beyond 2^56 slots", name);
    if (d_grad_index_out && n_slots >= (1ull << 31))
        return fail(MEE_ERR_INVALID_ARG, "%s: d_grad_index_out names a slot in 31 bits (the indexed apply reads indices below 2^31) and n_bags * max_len is %llu", name,
                    (unsigned long long)n_slots);
    return MEE_OK;
}

}  // namespace mee

using namespace mee;

extern "C" {

int mee_find_padded_as(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, size_t max_len, uint32_t flags, void* d_out,
                       uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out, uint32_t* d_grad_index_out, void* stream) {
    MEE_RANGE("mee_find_padded_as");
    MEE_NO_INT8_ROWS(t, "mee_find_padded_as");   // (an int8-row table has no padded lookup: pooled_fetch does not read such rows)
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_as: null argument");
    if (int rc = padded_check("mee_find_padded_as", n_bags != 0, d_keys, n, d_bag_offsets, n_bags, max_len, flags, d_out, out_dtype, d_grad_index_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    DeviceGuard guard(t->device);
    padded_launch<false>(t, nullptr, t->dim4, t->bf16_rows, d_keys, n, d_bag_offsets, n_bags, 1, max_len, flags, d_out, out_dtype,
                         PaddedOuts{d_found, d_lengths_out, d_step_keys_out, d_grad_index_out}, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_group_find_padded_as(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, size_t max_len, uint32_t flags, void* d_out,
                             uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out, uint32_t* d_grad_index_out, void* stream) {
    MEE_RANGE("mee_group_find_padded_as");
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_padded_as: null argument");
    uint64_t n_bags = 0;
    if (__builtin_mul_overflow((uint64_t)g->n_tables, (uint64_t)bags_per_table, &n_bags)) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_padded_as: n_tables * bags_per_table overflows");
    if (int rc = padded_check("mee_group_find_padded_as", n_bags != 0, d_keys, n, d_bag_offsets, n_bags, max_len, flags, d_out, out_dtype, d_grad_index_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    if (int rc = group_refresh(g, stream)) return rc;
    DeviceGuard guard(g->device);
    padded_launch<true>(nullptr, g, g->dim4, g->bf16_rows, d_keys, n, d_bag_offsets, n_bags, bags_per_table, max_len, flags, d_out, out_dtype,
                        PaddedOuts{d_found, d_lengths_out, d_step_keys_out, d_grad_index_out}, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// the padded lookup of a hot/cold pair: mee_find_pooled_tiered's checks of the two tables and padded_check's of the call, then one launch
int mee_find_padded_tiered(const mee_table* hot, const mee_table* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, size_t max_len,
                           uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out,
                           uint32_t* d_grad_index_out, void* stream) {
    MEE_RANGE("mee_find_padded_tiered");
    MEE_FP32_ROWS_ONLY(hot, "mee_find_padded_tiered");
    MEE_FP32_ROWS_ONLY(cold, "mee_find_padded_tiered");
    if (!hot || !cold) return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_tiered: null argument");
    if (hot == cold) return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_tiered: hot and cold are the same table (a key lives in exactly one tier)");
    if (hot->device != cold->device || hot->dim != cold->dim)
        return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_tiered: the tiers differ in device (%d, %d) or dim (%u, %u)", hot->device, cold->device, hot->dim, cold->dim);
    if (count_flags & ~(uint32_t)(MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT))
        return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_tiered: unknown count flag bits 0x%x (MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT)", count_flags);
    if (((count_flags & MEE_TIER_COUNT_COLD) && !cold->hits) || ((count_flags & MEE_TIER_COUNT_HOT) && !hot->hits))
        return fail(MEE_ERR_INVALID_ARG, "mee_find_padded_tiered: a count flag needs that tier created with MEE_FLAG_TRACK_HITS");
    if (int rc = padded_check("mee_find_padded_tiered", n_bags != 0, d_keys, n, d_bag_offsets, n_bags, max_len, flags, d_out, out_dtype, d_grad_index_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    DeviceGuard guard(hot->device);
    padded_tiered_launch<false>(hot, cold, nullptr, nullptr, hot->dim4, count_flags, d_keys, n, d_bag_offsets, n_bags, 1, max_len, flags, d_out, out_dtype,
                                PaddedOuts{d_found, d_lengths_out, d_step_keys_out, d_grad_index_out}, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// ... of a group of pairs: member j of `hot` and member j of `cold` are the two tiers of pair j (tiered_groups_check)
int mee_group_find_padded_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, size_t max_len,
                                 uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out,
                                 uint32_t* d_grad_index_out, void* stream) {
    MEE_RANGE("mee_group_find_padded_tiered");
    if (!hot || !cold) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_padded_tiered: null argument");
    if (int rc = tiered_groups_check(hot, cold, count_flags, "mee_group_find_padded_tiered")) return rc;
    uint64_t n_bags = 0;
    if (__builtin_mul_overflow((uint64_t)hot->n_tables, (uint64_t)bags_per_table, &n_bags))
        return fail(MEE_ERR_INVALID_ARG, "mee_group_find_padded_tiered: n_tables * bags_per_table overflows");
    if (int rc = padded_check("mee_group_find_padded_tiered", n_bags != 0, d_keys, n, d_bag_offsets, n_bags, max_len, flags, d_out, out_dtype, d_grad_index_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    if (int rc = group_refresh(hot, stream)) return rc;
    if (int rc = group_refresh(cold, stream)) return rc;
    DeviceGuard guard(hot->device);
    padded_tiered_launch<true>(nullptr, nullptr, hot, cold, hot->dim4, count_flags, d_keys, n, d_bag_offsets, n_bags, bags_per_table, max_len, flags, d_out, out_dtype,
                               PaddedOuts{d_found, d_lengths_out, d_step_keys_out, d_grad_index_out}, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
