// meepo_move.hip — tier migration (SPEC.md §3 move): "this key, with everything it owns, now lives in that table".  mee_move takes the keys of a batch
// that `src` holds out of `src` and into `dst` — the values row and every optimizer plane, bit for bit — without an [n, dim] buffer in between and
// without a host synchronisation; mee_group_move does it for every member pair of two groups (the hot and the cold tables of a collection of pairs)
// over one jagged batch.  Either table may keep its planes in HBM or in pinned, device-mapped host memory: the same loads and stores reach both.
//
// Launches.  No limit (max_moves >= n: demote, and rebalance, which slices its lists on the host):
//   1. move      per position: probe src (tile_probe), request the key's rows from every plane of src, claim in dst (tile_locate<claim>), store the
//                rows, and leave the src slot (or -1: absent, reserved, outside the segments, no room in dst) in src's per-batch slot list
//   2. mark      per position with a slot: RECLAIMED into the src key by one atomic exchange; the occurrence that reads the live key back counts
// A limit that can bind (promote with room for part of the candidates):
//   1. locate    the probe alone: the src slot per position            2. cut   an exclusive scan of "present" per table / segment (one block each):
//   3. move      the same body, reading the slot list instead of          positions whose rank reaches the limit lose their slot
//                probing                                               4. mark
// Why src keys are tombstoned by a launch of their own: every occurrence of a duplicate key must report d_moved = 1 and does the same idempotent work
// (claim-or-find in dst, the same row bytes to the same slot).  With the tombstone in the move launch an occurrence in another wave would probe src
// after it and read "absent"; and tile_probe is only right while no src key changes (plain loads, per-CU L1).  Behind the kernel boundary the slot
// list is all mark needs.  Rows of a tombstoned slot are never touched: nothing claims src slots in these launches.
// A key for which dst has no room keeps its src slot: its position writes -1 into the slot list, so mark leaves it alone (SPEC.md §3: it stays in src).
//
// The upstream snapshot has no code for tiers; the semantics are SPEC.md §3 (move) and "Tiering".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "meepo_table_int.h"

namespace mee {

// ---- the move of one wave step's positions --------------------------------------------------------------------------------------------------
// One 16-lane tile per position, R positions in flight per tile (RowShape), the step's keys by ONE coalesced load.  DIM4 = 16 / 32: the rows of all NP
// planes (values; + acc | m; + v) are requested before the claim and leave as one 16-byte group per lane and plane; DIM4 = 0 loops at run time.
// seg_of(i, s, d, local) -> bool: is batch position i served, and if so by which tables (src, dst) and at which index of src's slot list — what
// differs between one pair of tables and a group of pairs.  LOCATED (the limit path, DIM4 = 0, NP = 3 only): the src slot comes from the slot list
// the locate and cut passes left, and planes the optimizer does not have are null.
// Must be run by ALL 64 lanes in convergent control flow: tiles without work pass through the probes inactive.
template <int DIM4, int NP, bool LOCATED, class SegOf>
__device__ __forceinline__ void move_body(const int64_t* __restrict__ keys, uint64_t n, uint32_t dim4_rt, uint8_t* __restrict__ moved, SegOf&& seg_of) {
    static_assert(!LOCATED || (DIM4 == 0 && NP == 3), "the limit path has one instance");
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 1;
    constexpr int R = RowShape<DIM4>::rows_per_tile;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {   // wave-uniform
        MoveTable s[R], d[R];
        uint64_t loc[R], b[R];
        int64_t key[R], kb[R], sslot[R], dslot[R];
        bool inb[R], act[R], is_new[R], full[R];
        const int64_t kmine = (lane < 4 * R && base + lane < n) ? keys[base + lane] : kEmpty;   // one coalesced load for the wave step
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            inb[r] = seg_of(i, s[r], d[r], loc[r]);
            key[r] = __shfl(kmine, r * 4 + tile);
            act[r] = inb[r] && !reserved_key(key[r]);
            if constexpr (!LOCATED) {   // (the locate pass has flagged it already)
                if (inb[r] && tl == 0 && key[r] == kReclaimed) atomicOr(s[r].status, (uint32_t)MEE_STATUS_RESERVED_KEY);   // as remove does; EMPTY = padding, silent
                b[r] = bucket_of(key[r], s[r].nb);
                kb[r] = act[r] ? s[r].tkeys[b[r] * kW + tl] : kEmpty;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (LOCATED) sslot[r] = act[r] ? (int64_t)s[r].slots[loc[r]] : -1;
            else sslot[r] = tile_probe(s[r].tkeys, s[r].nb, key[r], act[r], b[r], kb[r], tile, tl);
        }
        float4 row[R][NP][C];
        if constexpr (DIM4 != 0) {   // every row of the step is in flight before the first claim
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int p = 0; p < NP; ++p)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        row[r][p][c] = sslot[r] >= 0 ? s[r].plane[p][(uint64_t)sslot[r] * DIM4 + c * 16 + tl] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) dslot[r] = tile_locate<true, true>(d[r].tkeys, d[r].nb, key[r], sslot[r] >= 0, tile, tl, is_new[r], full[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!inb[r]) continue;
            const bool ok = sslot[r] >= 0 && dslot[r] >= 0;
            if (ok) {
                if constexpr (DIM4 != 0) {
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int c = 0; c < C; ++c) d[r].plane[p][(uint64_t)dslot[r] * DIM4 + c * 16 + tl] = row[r][p][c];
                } else {
                    for (uint32_t c = tl; c < dim4; c += 16)
#pragma unroll
                        for (int p = 0; p < NP; ++p) {
                            if (LOCATED && !s[r].plane[p]) continue;
                            d[r].plane[p][(uint64_t)dslot[r] * dim4 + c] = s[r].plane[p][(uint64_t)sslot[r] * dim4 + c];
                        }
                }
            }
            if (tl == 0) {
                if (ok && is_new[r] && d[r].hits) d[r].hits[dslot[r]] = 0;   // a created slot starts a new window; an existing one keeps its counter
                s[r].slots[loc[r]] = ok ? sslot[r] : -1;                     // what the mark launch tombstones
                if (moved) moved[base + r * 4 + tile] = ok;
                if (full[r]) atomicOr(d[r].status, (uint32_t)MEE_STATUS_TABLE_FULL);
            }
        }
    }
}

// the segment of a batch position in a jagged batch whose n_tables + 1 offsets are staged in LDS (stage_offsets, meepo_device.h: cut at n).  The offsets
// are caller data and are never trusted: a position is served only where loff[lo] <= i < loff[lo + 1], so that its index in the member's slot
// list, i - loff[lo], stays below n whatever the array holds.
__device__ __forceinline__ bool member_of(const uint64_t* loff, uint32_t n_tables, uint64_t i, uint32_t& lo) {
    lo = member_of_position(loff, n_tables, i);
    return loff[lo] <= i && i < loff[lo + 1];
}

template <int DIM4, int NP, bool LOCATED = false>
__global__ __launch_bounds__(256) void move_kernel(MoveTable src, MoveTable dst, const int64_t* __restrict__ keys, uint32_t n, uint32_t dim4_rt,
                                                   uint8_t* __restrict__ moved, unsigned long long* __restrict__ n_moved) {
    if (n_moved && blockIdx.x == 0 && threadIdx.x == 0) *n_moved = 0;   // the mark launch behind this one adds to it
    move_body<DIM4, NP, LOCATED>(keys, n, dim4_rt, moved, [&](uint64_t i, MoveTable& s, MoveTable& d, uint64_t& loc) {
        s = src; d = dst; loc = i;
        return i < n;
    });
}

template <int DIM4, int NP, bool LOCATED = false>
__global__ __launch_bounds__(256) void move_grouped_kernel(const MoveTable* __restrict__ src, const MoveTable* __restrict__ dst, uint32_t n_tables,
                                                           const uint64_t* __restrict__ offsets, const int64_t* __restrict__ keys, uint64_t n,
                                                           uint32_t dim4_rt, uint8_t* __restrict__ moved, unsigned long long* __restrict__ n_moved) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    if (n_moved && blockIdx.x == 0)
        for (uint32_t j = threadIdx.x; j < n_tables; j += blockDim.x) n_moved[j] = 0;
    stage_offsets(loff, offsets, 1, n_tables, n);
    move_body<DIM4, NP, LOCATED>(keys, n, dim4_rt, moved, [&](uint64_t i, MoveTable& s, MoveTable& d, uint64_t& loc) {
        uint32_t lo;
        const bool in = i < n && member_of(loff, n_tables, i, lo);
        s = src[in ? lo : 0]; d = dst[in ? lo : 0];
        loc = in ? i - loff[lo] : 0;
        return in;
    });
}

// ---- the limit path, pass 1: the probe alone.  slots[local] = the src slot of every served position (-1: absent or reserved) ---------------------
template <class SegOf>
__device__ __forceinline__ void move_locate_body(const int64_t* __restrict__ keys, uint64_t n, SegOf&& seg_of) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr int R = 2;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {   // wave-uniform
        MoveTable s[R], d;
        uint64_t loc[R], b[R];
        int64_t key[R], kb[R], slot[R];
        bool inb[R], act[R];
        const int64_t kmine = (lane < 4 * R && base + lane < n) ? keys[base + lane] : kEmpty;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            inb[r] = seg_of(base + r * 4 + tile, s[r], d, loc[r]);
            key[r] = __shfl(kmine, r * 4 + tile);
            act[r] = inb[r] && !reserved_key(key[r]);
            if (inb[r] && tl == 0 && key[r] == kReclaimed) atomicOr(s[r].status, (uint32_t)MEE_STATUS_RESERVED_KEY);
            b[r] = bucket_of(key[r], s[r].nb);
            kb[r] = act[r] ? s[r].tkeys[b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(s[r].tkeys, s[r].nb, key[r], act[r], b[r], kb[r], tile, tl);
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (inb[r] && tl == 0) s[r].slots[loc[r]] = slot[r];
    }
}
__global__ __launch_bounds__(256) void move_locate_kernel(MoveTable src, const int64_t* __restrict__ keys, uint32_t n) {
    move_locate_body(keys, n, [&](uint64_t i, MoveTable& s, MoveTable&, uint64_t& loc) { s = src; loc = i; return i < n; });
}
__global__ __launch_bounds__(256) void move_locate_grouped_kernel(const MoveTable* __restrict__ src, uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ keys, uint64_t n) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    stage_offsets(loff, offsets, 1, n_tables, n);
    move_locate_body(keys, n, [&](uint64_t i, MoveTable& s, MoveTable&, uint64_t& loc) {
        uint32_t lo;
        const bool in = i < n && member_of(loff, n_tables, i, lo);
        s = src[in ? lo : 0];
        loc = in ? i - loff[lo] : 0;
        return in;
    });
}

// ---- the limit path, pass 2: positions of a slot list whose rank among the present ones reaches `limit` lose their slot ----------------------
// One block per list: an exclusive scan in position order, 1024 positions a round (a ballot per wave, the 16 wave totals through LDS).  The rare
// path, and a list is at most max_batch long.
constexpr int kCutBlock = 1024;
__device__ __forceinline__ void cut_list(long long* slots, uint64_t len, uint64_t limit) {
    __shared__ uint32_t wsum[kCutBlock / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t before = 0;   // present positions in front of this round
    for (uint64_t base = 0; base < len; base += kCutBlock) {   // block-uniform
        const uint64_t i = base + threadIdx.x;
        const bool present = i < len && slots[i] >= 0;
        const uint64_t bal = __ballot(present);
        if (lane == 0) wsum[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t in_front = 0, total = 0;
#pragma unroll
        for (int k = 0; k < kCutBlock / 64; ++k) {
            const uint32_t v = wsum[k];
            in_front += k < w ? v : 0u;
            total += v;
        }
        const uint64_t rank = before + in_front + (uint64_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (present && rank >= limit) slots[i] = -1;
        before += total;
        __syncthreads();
    }
}
__global__ __launch_bounds__(kCutBlock) void move_cut_kernel(MoveTable src, uint32_t n, uint64_t limit) { cut_list(src.slots, n, limit); }
// block j: member j's segment, limit limits[j]
__global__ __launch_bounds__(kCutBlock) void move_cut_grouped_kernel(const MoveTable* __restrict__ src, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                     const uint64_t* __restrict__ limits) {
    const uint32_t j = blockIdx.x;
    uint64_t begin = offsets[j], end = offsets[j + 1];
    end = end < n ? end : n;
    begin = begin < end ? begin : end;   // (member_of serves exactly [begin, end) of a non-decreasing offsets array; whatever it holds, end - begin <= n)
    cut_list(src[j].slots, end - begin, limits[j]);
}

// ---- the last pass: tombstones.  One thread per position; the src key of every slot the move left in the list becomes RECLAIMED by one exchange,
// and the occurrence that reads the live key back is the one that counts the key — summed per wave (and member) before the global atomic.
__global__ __launch_bounds__(256) void move_mark_kernel(MoveTable src, uint32_t n, unsigned long long* __restrict__ n_moved) {
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        const long long slot = i < n ? src.slots[i] : -1;
        const bool counted = slot >= 0 && atomicExch((unsigned long long*)(src.tkeys + slot), (unsigned long long)kReclaimed) != (unsigned long long)kReclaimed;
        const uint64_t bal = __ballot(counted);
        if (n_moved && bal && lane == 0) atomicAdd(n_moved, (unsigned long long)__popcll(bal));
    }
}
__global__ __launch_bounds__(256) void move_mark_grouped_kernel(const MoveTable* __restrict__ src, uint32_t n_tables, const uint64_t* __restrict__ offsets, uint64_t n,
                                                                unsigned long long* __restrict__ n_moved) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    stage_offsets(loff, offsets, 1, n_tables, n);
    const int lane = threadIdx.x & 63;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {   // block-uniform
        const uint64_t i = i0 + threadIdx.x;
        uint32_t member = 0;
        const bool in = i < n && member_of(loff, n_tables, i, member);
        bool counted = false;
        if (in) {
            const MoveTable s = src[member];
            const long long slot = s.slots[i - loff[member]];
            counted = slot >= 0 && atomicExch((unsigned long long*)(s.tkeys + slot), (unsigned long long)kReclaimed) != (unsigned long long)kReclaimed;
        }
        uint64_t rest = __ballot(counted);
        while (n_moved && rest) {   // wave-uniform: one atomic per member the wave's positions belong to (nearly always one)
            const int first = __ffsll((unsigned long long)rest) - 1;
            const uint32_t m = __shfl(member, first);
            const uint64_t same = __ballot(counted && member == m);
            if (lane == first) atomicAdd(&n_moved[m], (unsigned long long)__popcll(same));
            rest &= ~same;
        }
    }
}

// =========================================================================================================
// host side
// =========================================================================================================
static MoveTable move_table_of(const mee_table* t) {
    return MoveTable{t->keys, {(float4*)t->values, (float4*)t->s1, (float4*)t->s2}, t->nb, &t->ctr->status, t->hits, t->g.sres};
}
static int planes_of(uint32_t optimizer) { return opt_has_s2(optimizer) ? 3 : optimizer == MEE_OPT_ADAGRAD ? 2 : 1; }

// what a move refuses about one (src, dst) pair before anything is launched or written; `member` < 0: the pair of mee_move
static int move_pair_check(const mee_table* s, const mee_table* d, size_t n, const char* name, int member) {
    char who[32] = "";
    if (member >= 0) snprintf(who, sizeof who, " (member %d)", member);
    if (s == d) return fail(MEE_ERR_INVALID_ARG, "%s: src and dst are the same table%s", name, who);
    MEE_FP32_ROWS_ONLY(s, name);
    MEE_FP32_ROWS_ONLY(d, name);
    if (s->device != d->device || s->dim != d->dim || s->optimizer != d->optimizer)
        return fail(MEE_ERR_INVALID_ARG, "%s: src and dst differ in device (%d, %d), dim (%u, %u) or optimizer (%u, %u)%s — a key moves with every plane it owns", name,
                    s->device, d->device, s->dim, d->dim, s->optimizer, d->optimizer, who);
    for (const mee_table* t : {s, d}) {
        if (t->pending.n && !t->pending.by_forward)
            return fail(MEE_ERR_INVALID_ARG, "%s: a prepared apply is pending on a table%s (finish it with mee_apply_* or mee_apply_discard)", name, who);
        if (n > t->max_batch)
            return fail(MEE_ERR_BATCH_TOO_LARGE, "%s: n=%zu exceeds config.max_batch=%llu%s", name, n, (unsigned long long)t->max_batch, who);
    }
    return MEE_OK;
}

}  // namespace mee

using namespace mee;

extern "C" {

int mee_move(mee_table* src, mee_table* dst, const int64_t* d_keys, size_t n, uint64_t max_moves, uint8_t* d_moved, uint64_t* d_n_moved, void* stream) {
    MEE_RANGE("mee_move");
    if (!src || !dst || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_move: null argument");
    if (int rc = move_pair_check(src, dst, n, "mee_move", -1)) return rc;
    // from here on as mee_remove on src and mee_insert on dst: a partition a training forward left pending on either is dropped
    if (int rc = check_batch(src, n, "mee_move", stream)) return rc;
    if (int rc = check_batch(dst, n, "mee_move", stream)) return rc;
    DeviceGuard g(src->device);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (d_n_moved) zero_words(d_n_moved, sizeof *d_n_moved, st);
        MEE_HIP(hipGetLastError());
        return MEE_OK;
    }
    ++src->handle_epoch;   // rows leave src: slot handles handed out before this call are stale
    const uint32_t nn = (uint32_t)n;
    const MoveTable s = move_table_of(src), d = move_table_of(dst);
    unsigned long long* cnt = (unsigned long long*)d_n_moved;
    if (max_moves >= n) {
        with_row_shape(src->dim4, [&](auto d4) { with_value<1, 2, 3>(planes_of(src->optimizer), [&](auto np) {
            move_kernel<d4, np><<<grid_for(n, 16 * RowShape<d4>::rows_per_tile, 1u << 16), 256, 0, st>>>(s, d, d_keys, nn, src->dim4, d_moved, cnt);
        }); });
    } else {
        move_locate_kernel<<<grid_for(n, 32, 1u << 16), 256, 0, st>>>(s, d_keys, nn);
        move_cut_kernel<<<1, kCutBlock, 0, st>>>(s, nn, max_moves);
        move_kernel<0, 3, true><<<grid_for(n, 16, 1u << 16), 256, 0, st>>>(s, d, d_keys, nn, src->dim4, d_moved, cnt);
    }
    move_mark_kernel<<<grid_for(n, 256, 1u << 16), 256, 0, st>>>(s, nn, cnt);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_group_move(mee_group* src, mee_group* dst, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, const uint64_t* d_max_moves, uint8_t* d_moved,
                   uint64_t* d_n_moved, void* stream) {
    MEE_RANGE("mee_group_move");
    if (!src || !dst || !d_offsets || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_group_move: null argument");
    if (int rc = tiered_groups_check(src, dst, 0, "mee_group_move")) return rc;
    // The member offsets live on the device and the call reads nothing back, so the bound on a segment is the bound on the whole batch: n itself may not
    // exceed a member's max_batch (a segment indexes its src member's per-batch slot list).
    for (uint32_t j = 0; j < src->n_tables; ++j)
        if (int rc = move_pair_check(src->tables[j], dst->tables[j], n, "mee_group_move", (int)j)) return rc;
    for (uint32_t j = 1; j < src->n_tables; ++j)   // the number of planes is a property of the launch, not a per-member branch
        if (src->tables[j]->optimizer != src->tables[0]->optimizer)
            return fail(MEE_ERR_INVALID_ARG, "mee_group_move: member %u differs from member 0 in optimizer (%u vs %u): one grouped move carries one set of planes", j,
                        src->tables[j]->optimizer, src->tables[0]->optimizer);
    {   // a table that is a member twice would be probed read-only by one segment while another claims in it, and lend one slot list to two segments
        std::vector<const mee_table*> all(src->tables.begin(), src->tables.end());
        all.insert(all.end(), dst->tables.begin(), dst->tables.end());
        std::sort(all.begin(), all.end());
        if (std::adjacent_find(all.begin(), all.end()) != all.end())
            return fail(MEE_ERR_INVALID_ARG, "mee_group_move: a table is a member more than once across the two groups (every member moves through its own tables)");
    }
    for (mee_group* g : {src, dst})
        for (mee_table* t : g->tables)
            if (int rc = check_batch(t, n, "mee_group_move", stream)) return rc;
    if (int rc = group_refresh(src, stream)) return rc;
    if (int rc = group_refresh(dst, stream)) return rc;
    DeviceGuard guard(src->device);
    hipStream_t st = as_stream(stream);
    unsigned long long* cnt = (unsigned long long*)d_n_moved;
    const uint32_t nt = src->n_tables;
    if (n == 0) {
        if (d_n_moved) zero_words(d_n_moved, nt * sizeof *d_n_moved, st);
        MEE_HIP(hipGetLastError());
        return MEE_OK;
    }
    for (mee_table* t : src->tables) ++t->handle_epoch;
    if (!d_max_moves) {
        with_row_shape(src->dim4, [&](auto d4) { with_value<1, 2, 3>(planes_of(src->tables[0]->optimizer), [&](auto np) {
            move_grouped_kernel<d4, np><<<grid_for(n, 16 * RowShape<d4>::rows_per_tile, 8192), 256, 0, st>>>(src->d_move, dst->d_move, nt, d_offsets, d_keys, n, src->dim4,
                                                                                                           d_moved, cnt);
        }); });
    } else {
        move_locate_grouped_kernel<<<grid_for(n, 32, 8192), 256, 0, st>>>(src->d_move, nt, d_offsets, d_keys, n);
        move_cut_grouped_kernel<<<nt, kCutBlock, 0, st>>>(src->d_move, d_offsets, n, d_max_moves);
        move_grouped_kernel<0, 3, true><<<grid_for(n, 16, 8192), 256, 0, st>>>(src->d_move, dst->d_move, nt, d_offsets, d_keys, n, src->dim4, d_moved, cnt);
    }
    move_mark_grouped_kernel<<<grid_for(n, 256, 8192), 256, 0, st>>>(src->d_move, nt, d_offsets, n, cnt);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
