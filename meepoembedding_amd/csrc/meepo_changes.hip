// meepo_changes.hip — the change log and the delta export (SPEC.md §3 "Change log"): "which keys changed since the last save, and what do they hold now".
// A change log (mee_changes) is a SET of int64 keys on one device: a table key plane and nothing else — 16 x prime buckets of 128 bytes, the hash and the
// probe sequence of SPEC.md §2, 8 bytes per slot — plus two device words, `size` (distinct keys stored) and `invalid` (sticky: a key found no room).  It
// belongs to no table; which table's mutations it records is the caller's business (the Python layer notes every mutator's batch, table.py).
//
// Launches.
//   note          per batch position: claim-or-find the key in the log's plane (tile_locate<claim>); the positions a wave step created are counted by
//                 ballots and leave as ONE atomic on `size`; a key without room sets `invalid` and is not stored.  mee_changes_group_note: the same body,
//                 the log of a position picked by its segment of a jagged batch (stage_offsets / member_of, as meepo_move.hip's grouped kernels).
//   export        mee_export_changed, per 64 slots of the log's range and wave: the stored keys are probed in the table (tile_probe: read-only, as find),
//                 sixteen at a time; the wave then takes ONE ticket per list — held keys (upserts) and absent keys (removed) — by a ballot and a single
//                 atomic each, writes the keys from the lanes that hold them and copies the rows of every plane, one 16-lane tile per row.
//   publish       mee_publish_changed / mee_group_publish_changed: the same walk and probe, twice — the held keys' values rows go straight into a serving
//                 table (claimed or found there, rounded once for bf16 rows), then the absent keys are tombstoned there (see "publish" below).
// Why a key set and not a bitmap over the table's slots: a bitmap loses the key of a slot that was removed (the delta must name it) and dies with
// mee_reserve, which moves every key to another slot (DESIGN.md §4 "Change log and delta export").
//
// The upstream snapshot has no code for checkpoints; the semantics are SPEC.md §3 "Change log".
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "meepo_table_int.h"

namespace mee {

struct ChangeState {             // device-resident, persistent
    unsigned long long size;     // distinct keys stored
    uint32_t invalid;            // sticky: some noted key found no room (or mee_changes_invalidate): the log no longer names every change
    uint32_t pad;
};
struct ChangeSet {               // a log as a kernel sees it: a kernel argument for one log, per member and device resident for a group of logs
    int64_t* keys;
    uint64_t nb;
    ChangeState* state;
};

constexpr int kNoteRounds = 2;   // keys in flight per 16-lane tile of the note kernels (RowShape<16>::rows_per_tile: a key is one 8-byte "row")

// ---- note: one wave step's positions ------------------------------------------------------------------------------------------------------
// One 16-lane tile per position, kNoteRounds positions per tile, the step's keys by ONE coalesced load.  log_of(i, ChangeSet&) -> bool: is batch
// position i noted at all, and in which log — what differs between one log and a group of logs.  EMPTY and RECLAIMED are padding: skipped silently.
// Must be run by ALL 64 lanes in convergent control flow: tiles without work pass through the claims inactive.
template <class LogOf>
__device__ __forceinline__ void note_body(const int64_t* __restrict__ keys, uint64_t n, LogOf&& log_of) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr int R = kNoteRounds;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {   // wave-uniform
        ChangeSet c[R];
        int64_t key[R];
        bool act[R], is_new[R], full[R];
        const int64_t kmine = (lane < 4 * R && base + lane < n) ? keys[base + lane] : kEmpty;   // one coalesced load for the wave step
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool in = log_of(base + r * 4 + tile, c[r]);
            key[r] = __shfl(kmine, r * 4 + tile);
            act[r] = in && !reserved_key(key[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) (void)tile_locate<true, true>(c[r].keys, c[r].nb, key[r], act[r], tile, tl, is_new[r], full[r]);
        uint64_t rest[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (act[r] && full[r] && tl == 0) atomicOr(&c[r].state->invalid, 1u);
            rest[r] = __ballot(act[r] && is_new[r] && tl == 0);
        }
        // `size`: one atomic per log the step's creations belong to (one log: one atomic per wave step)
        while (true) {   // wave-uniform
            int first = -1;
            unsigned long long sp = 0;
#pragma unroll
            for (int r = R - 1; r >= 0; --r)
                if (rest[r]) { first = __ffsll((unsigned long long)rest[r]) - 1; sp = (unsigned long long)__shfl((long long)(uintptr_t)c[r].state, first); }
            if (first < 0) break;
            uint32_t cnt = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t same = __ballot(act[r] && is_new[r] && tl == 0 && (unsigned long long)(uintptr_t)c[r].state == sp) & rest[r];
                cnt += (uint32_t)__popcll(same);
                rest[r] &= ~same;
            }
            if (lane == first) atomicAdd(&reinterpret_cast<ChangeState*>((uintptr_t)sp)->size, (unsigned long long)cnt);
        }
    }
}

__global__ __launch_bounds__(256) void changes_note_kernel(ChangeSet log, const int64_t* __restrict__ keys, uint64_t n) {
    note_body(keys, n, [&](uint64_t i, ChangeSet& c) { c = log; return i < n; });
}

// the segment of a batch position: the offsets are caller data and are never trusted (meepo_move.hip, member_of): a position outside
// [offsets[0], offsets[n_tables]) or at or past n is noted nowhere
__global__ __launch_bounds__(256) void changes_group_note_kernel(const ChangeSet* __restrict__ logs, uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                                 const int64_t* __restrict__ keys, uint64_t n) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    stage_offsets(loff, offsets, 1, n_tables, n);
    note_body(keys, n, [&](uint64_t i, ChangeSet& c) {
        const uint32_t lo = member_of_position(loff, n_tables, i);
        const bool in = i < n && loff[lo] <= i && i < loff[lo + 1];
        c = logs[in ? lo : 0];
        return in;
    });
}

// empty, size = 0, invalid = 0
__global__ __launch_bounds__(256) void changes_clear_kernel(ChangeSet log, uint64_t capacity) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < capacity; i += (uint64_t)gridDim.x * blockDim.x) log.keys[i] = kEmpty;
    if (blockIdx.x == 0 && threadIdx.x == 0) { log.state->size = 0; log.state->invalid = 0; }
}
__global__ void changes_invalidate_kernel(ChangeState* state) { state->invalid = 1u; }

// ---- the delta export ---------------------------------------------------------------------------------------------------------------------
struct ChangedPlanes {           // the planes a launch copies: values, then the optimizer planes the table has AND the caller asked for
    const float4* src[3];
    float4* dst[3];
};
constexpr int kChangedProbes = 4;   // keys in flight per tile while the table is probed: a wave asks about 16 keys of its 64 slots at a time

// lane of the idx-th set bit of m (idx < 16), or -1
__device__ __forceinline__ int nth_set_lane(uint64_t m, int idx) {
#pragma unroll
    for (int q = 0; q < 15; ++q)
        if (q < idx) m &= m - 1;
    return m ? __ffsll((unsigned long long)m) - 1 : -1;
}
__device__ __forceinline__ uint64_t drop_lowest_16(uint64_t m) {
#pragma unroll
    for (int q = 0; q < 16; ++q) m &= m - 1;   // x & (x - 1) of 0 stays 0
    return m;
}

// The batched read-only probe of a wave step's keys (the export and both publish launches): lane l holds key kmine, `mask` = the lanes whose key is
// asked about.  The keys are probed in `tkeys` 4 x kChangedProbes at a time (tile_probe: plain loads, so no key of that table may change into or out
// of any of the asked keys while the kernel runs); the slot (or -1) comes back to the lane that holds the key.  Lanes outside the mask get -1.  Must be
// called by ALL 64 lanes in convergent control flow; `mask` is wave-uniform.
__device__ __forceinline__ int64_t probe_step_keys(const int64_t* __restrict__ tkeys, uint64_t nb, int64_t kmine, uint64_t mask, int lane, int tile, int tl) {
    constexpr int P = kChangedProbes;
    int64_t myslot = -1;
    for (uint64_t rest = mask; rest; rest = drop_lowest_16(rest)) {   // wave-uniform
        int from[P];
        int64_t key[P], kb[P], slot[P];
        uint64_t b[P];
        bool act[P];
#pragma unroll
        for (int r = 0; r < P; ++r) {
            from[r] = nth_set_lane(rest, r * 4 + tile);
            key[r] = __shfl(kmine, from[r] >= 0 ? from[r] : 0);
            act[r] = from[r] >= 0;
            b[r] = bucket_of(key[r], nb);
            kb[r] = act[r] ? tkeys[b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < P; ++r) slot[r] = tile_probe(tkeys, nb, key[r], act[r], b[r], kb[r], tile, tl);
#pragma unroll
        for (int r = 0; r < P; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int owner = __shfl(from[r], q * kW);
                const int64_t sq = __shfl(slot[r], q * kW);
                if (lane == owner) myslot = sq;
            }
    }
    return myslot;
}

// DIM4 = 16 / 32: RowShape<DIM4>::rows_per_tile rows of all NP planes are requested before the first store and move as 16-byte groups per lane;
// DIM4 = 0 loops at run time.  All slot-to-row arithmetic in 64 bits.
template <int DIM4, int NP>
__global__ __launch_bounds__(256) void export_changed_kernel(const int64_t* __restrict__ lkeys, uint64_t begin, uint64_t end, const int64_t* __restrict__ tkeys,
                                                             uint64_t nb, ChangedPlanes pl, uint32_t dim4_rt, int64_t* __restrict__ keys_out, uint64_t cap,
                                                             int64_t* __restrict__ removed_out, uint64_t removed_cap, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 1;
    constexpr int R = RowShape<DIM4>::rows_per_tile;
    for (uint64_t s0 = begin + wave * 64; s0 < end; s0 += n_waves * 64) {   // wave-uniform
        const int64_t kmine = s0 + lane < end ? lkeys[s0 + lane] : kEmpty;   // the log's slots as they lie: one coalesced load
        const bool stored = !reserved_key(kmine);
        const uint64_t sm = __ballot(stored);
        if (!sm) continue;   // wave-uniform
        // ---- probe the table for every stored key, 4P at a time; the slot comes back to the lane that holds the key
        const int64_t myslot = probe_step_keys(tkeys, nb, kmine, sm, lane, tile, tl);
        // ---- one ticket per list
        const uint64_t um = __ballot(stored && myslot >= 0), rm = sm & ~um;
        unsigned long long up0 = 0, rm0 = 0;
        if (lane == 0 && um) up0 = atomicAdd(&counts[0], (unsigned long long)__popcll(um));
        if (lane == 0 && rm) rm0 = atomicAdd(&counts[1], (unsigned long long)__popcll(rm));
        up0 = __shfl(up0, 0); rm0 = __shfl(rm0, 0);
        const uint64_t below = (1ull << lane) - 1ull;
        if (stored && myslot >= 0) {
            const uint64_t pos = up0 + (uint64_t)__popcll(um & below);
            if (pos < cap) keys_out[pos] = kmine;
        } else if (stored) {
            const uint64_t pos = rm0 + (uint64_t)__popcll(rm & below);
            if (pos < removed_cap) removed_out[pos] = kmine;
        }
        // ---- the rows of the held keys: one tile per row, 4R rows a round, every plane
        uint64_t done = 0;
        for (uint64_t rest = um; rest;) {   // wave-uniform
            int64_t tslot[R];
            uint64_t pos[R];
            bool has[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int from = nth_set_lane(rest, r * 4 + tile);
                tslot[r] = __shfl(myslot, from >= 0 ? from : 0);
                pos[r] = up0 + done + (uint64_t)(r * 4 + tile);
                has[r] = from >= 0 && tslot[r] >= 0 && pos[r] < cap;
            }
            if constexpr (DIM4 != 0) {
                float4 row[R][NP][C];
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int p = 0; p < NP; ++p)
#pragma unroll
                        for (int c = 0; c < C; ++c)
                            row[r][p][c] = has[r] ? pl.src[p][(uint64_t)tslot[r] * DIM4 + c * 16 + tl] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (has[r]) {
#pragma unroll
                        for (int p = 0; p < NP; ++p)
#pragma unroll
                            for (int c = 0; c < C; ++c) pl.dst[p][pos[r] * DIM4 + c * 16 + tl] = row[r][p][c];
                    }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (has[r])
                        for (uint32_t c = tl; c < dim4; c += 16)
#pragma unroll
                            for (int p = 0; p < NP; ++p) pl.dst[p][pos[r] * dim4 + c] = pl.src[p][(uint64_t)tslot[r] * dim4 + c];
            }
#pragma unroll
            for (int q = 0; q < 4 * R; ++q) rest &= rest - 1;
            done += 4 * R;
        }
    }
}

// ---- publish: log -> trainer table -> serving table (SPEC.md §3 "Publish") ----------------------------------------------------------------
// Two launches over the same walk of the log (64 slots per wave step, the stored keys probed read-only in src as the export probes them):
//   upsert   the keys src holds: their values rows are requested from src, 4R a round, BEFORE the first claim; each key is then claimed or found in
//            dst (tile_locate<claim, coherent>: other tiles of this launch claim in the same table) and the row is stored — 16 bytes per lane into an
//            fp32-row dst, the four floats rounded once (bf16x4_of) and 8 bytes per lane into a bf16-row dst.  No state plane is read.
//   remove   behind the kernel boundary: the keys src does not hold are located in dst and tombstoned.
// Why two: the contract is the composition "insert the upserts, THEN remove the rest".  Which keys find room in a crowded dst is part of it: a tombstone
// written while the claims are under way frees a slot the composition's insert never saw, so a key the composition drops (TABLE_FULL) could be stored.
// Behind the kernel boundary every claim has been made against the table as insert sees it, and the remove launch may probe with plain loads (below).
struct PublishTables {           // wave-uniform: src as it is read, dst as it is written
    const int64_t* skeys;
    const float4* srows;
    uint64_t snb;
    int64_t* dkeys;
    void* drows;                 // fp32 rows (float4 groups) or bf16 rows (8-byte groups)
    uint64_t dnb;
    uint32_t* dstatus;
    uint32_t* dhits;             // null without MEE_FLAG_TRACK_HITS
};
struct PublishStep {             // the 64 log slots one wave step walks
    const int64_t* lkeys;
    uint64_t s0, end;            // the step's first slot and the end of the range, both in that log
    PublishTables t;
    unsigned long long* counts;  // the four words of that log's publish
};
static __device__ __forceinline__ PublishTables publish_tables_of(const MoveTable& s, const MoveTable& d) {
    return PublishTables{s.tkeys, s.plane[0], s.nb, d.tkeys, d.plane[0], d.nb, d.status, d.hits};
}

// step_of(step, PublishStep&): what wave step `step` < n_steps works on — what differs between one table and a group.  Counts leave as one atomic per
// wave step and list.  Must be run by ALL 64 lanes in convergent control flow.
template <int DIM4, bool BF16, class StepOf>
__device__ __forceinline__ void publish_upsert_body(uint64_t n_steps, uint32_t dim4_rt, StepOf&& step_of) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 1;
    constexpr int R = RowShape<DIM4>::rows_per_tile;
    for (uint64_t step = wave; step < n_steps; step += n_waves) {   // wave-uniform
        PublishStep p;
        step_of(step, p);
        const int64_t kmine = p.s0 + lane < p.end ? p.lkeys[p.s0 + lane] : kEmpty;   // the log's slots as they lie: one coalesced load
        const bool stored = !reserved_key(kmine);
        const uint64_t sm = __ballot(stored);
        if (!sm) continue;   // wave-uniform
        const int64_t myslot = probe_step_keys(p.t.skeys, p.t.snb, kmine, sm, lane, tile, tl);
        uint32_t n_placed = 0, n_full = 0;
        for (uint64_t rest = __ballot(stored && myslot >= 0); rest;) {   // wave-uniform: the held keys, one tile per key, 4R a round
            int64_t key[R], sslot[R], dslot[R];
            bool has[R], is_new[R], full[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int from = nth_set_lane(rest, r * 4 + tile);
                has[r] = from >= 0;
                key[r] = __shfl(kmine, has[r] ? from : 0);
                sslot[r] = __shfl(myslot, has[r] ? from : 0);
            }
            float4 row[R][C];
            if constexpr (DIM4 != 0) {   // every row of the round is in flight before the first claim
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < C; ++c) row[r][c] = has[r] ? p.t.srows[(uint64_t)sslot[r] * DIM4 + c * 16 + tl] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int r = 0; r < R; ++r) dslot[r] = tile_locate<true, true>(p.t.dkeys, p.t.dnb, key[r], has[r], tile, tl, is_new[r], full[r]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = has[r] && dslot[r] >= 0;   // (a claim that found no slot reports `full`)
                if (ok) {
                    const uint64_t o = (uint64_t)dslot[r] * dim4;
                    if constexpr (DIM4 != 0) {
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            if constexpr (BF16) reinterpret_cast<u32x2*>(p.t.drows)[o + c * 16 + tl] = bf16x4_of(row[r][c].x, row[r][c].y, row[r][c].z, row[r][c].w);
                            else reinterpret_cast<float4*>(p.t.drows)[o + c * 16 + tl] = row[r][c];
                        }
                    } else {
                        for (uint32_t c = tl; c < dim4; c += 16) {
                            const float4 v = p.t.srows[(uint64_t)sslot[r] * dim4 + c];
                            if constexpr (BF16) reinterpret_cast<u32x2*>(p.t.drows)[o + c] = bf16x4_of(v.x, v.y, v.z, v.w);
                            else reinterpret_cast<float4*>(p.t.drows)[o + c] = v;
                        }
                    }
                    if (is_new[r] && p.t.dhits && tl == 0) p.t.dhits[dslot[r]] = 0;   // a created slot starts a new window; an existing one keeps its counter
                }
                const uint64_t fm = __ballot(has[r] && full[r] && tl == 0);
                if (fm && lane == __ffsll((unsigned long long)fm) - 1) atomicOr(p.t.dstatus, (uint32_t)MEE_STATUS_TABLE_FULL);
                n_placed += (uint32_t)__popcll(__ballot(ok && tl == 0));
                n_full += (uint32_t)__popcll(fm);
            }
#pragma unroll
            for (int q = 0; q < 4 * R; ++q) rest &= rest - 1;
        }
        if (lane == 0 && n_placed) atomicAdd(&p.counts[0], (unsigned long long)n_placed);
        if (lane == 0 && n_full) atomicAdd(&p.counts[2], (unsigned long long)n_full);
    }
}

// The keys of the step that src does not hold leave dst.  The probe of dst is the read-only one (plain loads) although this launch writes dst's keys,
// because of WHAT it writes: every key of the log is handled by exactly one lane of one wave (a log holds a key once), so the only change another wave can
// make under a probe for key K is to turn a live key OTHER than K into RECLAIMED.  A probe stops at K or at an EMPTY slot and walks past everything else:
// whether a stale line still shows the live foreign key or already the tombstone, it is neither, and the probe's outcome is the same.  EMPTY slots are
// never made or filled here, and the upsert launch's claims are behind a kernel boundary.
template <class StepOf>
__device__ __forceinline__ void publish_remove_body(uint64_t n_steps, StepOf&& step_of) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t step = wave; step < n_steps; step += n_waves) {   // wave-uniform
        PublishStep p;
        step_of(step, p);
        const int64_t kmine = p.s0 + lane < p.end ? p.lkeys[p.s0 + lane] : kEmpty;
        const bool stored = !reserved_key(kmine);
        const uint64_t sm = __ballot(stored);
        if (!sm) continue;   // wave-uniform
        const int64_t sslot = probe_step_keys(p.t.skeys, p.t.snb, kmine, sm, lane, tile, tl);   // src has not changed since the upsert launch
        const uint64_t rm = __ballot(stored && sslot < 0);
        if (!rm) continue;   // wave-uniform
        const int64_t dslot = probe_step_keys(p.t.dkeys, p.t.dnb, kmine, rm, lane, tile, tl);
        if (dslot >= 0) (void)atomicExch((unsigned long long*)(p.t.dkeys + dslot), (unsigned long long)kReclaimed);   // by the lane that holds the key
        if (lane == 0) atomicAdd(&p.counts[1], (unsigned long long)__popcll(rm));
    }
}

template <int DIM4, bool BF16>
__global__ __launch_bounds__(256) void publish_upsert_kernel(ChangeSet log, uint64_t begin, uint64_t end, PublishTables t, uint32_t dim4_rt,
                                                             unsigned long long* __restrict__ counts) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[3] = log.state->invalid;   // as this launch read it
    publish_upsert_body<DIM4, BF16>((end - begin + 63) / 64, dim4_rt, [&](uint64_t step, PublishStep& p) { p = PublishStep{log.keys, begin + step * 64, end, t, counts}; });
}
__global__ __launch_bounds__(256) void publish_remove_kernel(ChangeSet log, uint64_t begin, uint64_t end, PublishTables t, unsigned long long* __restrict__ counts) {
    publish_remove_body((end - begin + 63) / 64, [&](uint64_t step, PublishStep& p) { p = PublishStep{log.keys, begin + step * 64, end, t, counts}; });
}

// The group form: the flat work space is the concatenation of the members' log capacities, each rounded up to a multiple of 64, so a wave step lies in
// one member and everything in PublishStep is wave-uniform.  lb: the n_tables + 1 bounds of that space, staged in LDS (stage_offsets).
__device__ __forceinline__ void publish_group_step(const uint64_t* lb, uint32_t n_tables, const ChangeSet* __restrict__ logs, const MoveTable* __restrict__ src,
                                                   const MoveTable* __restrict__ dst, unsigned long long* counts, uint64_t step, PublishStep& p) {
    const uint64_t f = step * 64;
    const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)member_of_position(lb, n_tables, f));   // (the same in every lane: say so)
    const ChangeSet lg = logs[j];
    p = PublishStep{lg.keys, f - lb[j], lg.nb * (uint64_t)kW, publish_tables_of(src[j], dst[j]), counts + 4 * (uint64_t)j};
}
template <int DIM4, bool BF16>
__global__ __launch_bounds__(256) void publish_upsert_grouped_kernel(const ChangeSet* __restrict__ logs, const uint64_t* __restrict__ bounds, uint32_t n_tables,
                                                                     const MoveTable* __restrict__ src, const MoveTable* __restrict__ dst, uint32_t dim4_rt,
                                                                     unsigned long long* __restrict__ counts) {
    __shared__ uint64_t lb[kMaxGroupTables + 1];
    if (blockIdx.x == 0)
        for (uint32_t j = threadIdx.x; j < n_tables; j += blockDim.x) counts[4 * (uint64_t)j + 3] = logs[j].state->invalid;
    stage_offsets(lb, bounds, 1, n_tables, ~0ull);
    publish_upsert_body<DIM4, BF16>(lb[n_tables] / 64, dim4_rt, [&](uint64_t step, PublishStep& p) { publish_group_step(lb, n_tables, logs, src, dst, counts, step, p); });
}
__global__ __launch_bounds__(256) void publish_remove_grouped_kernel(const ChangeSet* __restrict__ logs, const uint64_t* __restrict__ bounds, uint32_t n_tables,
                                                                     const MoveTable* __restrict__ src, const MoveTable* __restrict__ dst,
                                                                     unsigned long long* __restrict__ counts) {
    __shared__ uint64_t lb[kMaxGroupTables + 1];
    stage_offsets(lb, bounds, 1, n_tables, ~0ull);
    publish_remove_body(lb[n_tables] / 64, [&](uint64_t step, PublishStep& p) { publish_group_step(lb, n_tables, logs, src, dst, counts, step, p); });
}

// =========================================================================================================
// host side
// =========================================================================================================
static int changes_device_check(int device, const char* name) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MEE_ERR_NO_DEVICE, "%s: no HIP device visible (this backend has no CPU fallback)", name);
    if (device < 0 || device >= ndev) return fail(MEE_ERR_INVALID_ARG, "%s: device %d out of range (have %d)", name, device, ndev);
    hipDeviceProp_t prop;
    MEE_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MEE_ERR_NO_DEVICE, "%s: device %d is %s; this library is built for gfx950 only", name, device, prop.gcnArchName);
    return MEE_OK;
}

}  // namespace mee

struct mee_changes {
    int device;
    uint64_t capacity, nb;
    int64_t* keys;
    mee::ChangeState* state;
};
struct mee_changes_group {
    int device;
    uint32_t n_tables;
    mee::ChangeSet* d_logs;   // [n_tables], device: a log's plane never moves, so this is uploaded once
    // mee_group_publish_changed walks all the logs as one flat space: the members' capacities, each rounded up to a multiple of 64, end to end
    uint64_t* d_bounds;       // [n_tables + 1], device, uploaded with d_logs
    uint64_t walk_slots;      // = bounds[n_tables]
};

using namespace mee;

static ChangeSet change_set_of(const mee_changes* c) { return ChangeSet{c->keys, c->nb, c->state}; }

// what a publish refuses about one (src, dst) pair before anything is launched or written; `member` < 0: the pair of mee_publish_changed
static int publish_pair_check(const mee_table* s, const mee_table* d, const char* name, int member) {
    char who[32] = "";
    if (member >= 0) snprintf(who, sizeof who, " (member %d)", member);
    if (s == d) return fail(MEE_ERR_INVALID_ARG, "%s: src and dst are the same table%s", name, who);
    if (s->device != d->device || s->dim != d->dim)
        return fail(MEE_ERR_INVALID_ARG, "%s: src and dst differ in device (%d, %d) or dim (%u, %u)%s", name, s->device, d->device, s->dim, d->dim, who);
    if (d->optimizer != MEE_OPT_NONE)
        return fail(MEE_ERR_UNSUPPORTED, "%s: dst has an optimizer (%u)%s — a publish carries the values row only, into a table without state planes", name, d->optimizer, who);
    if (s->bf16_rows || s->int8_rows)
        return fail(MEE_ERR_UNSUPPORTED, "%s: src stores %s rows%s — the source of a publish is an fp32-row table", name, s->bf16_rows ? "bf16" : "int8", who);
    if (d->int8_rows)
        return fail(MEE_ERR_UNSUPPORTED, "%s: dst stores int8 rows%s — publish into fp32 or bf16 rows (an int8-row table takes the delta through mee_insert and mee_remove)", name, who);
    return MEE_OK;
}

extern "C" {

int mee_changes_create(int32_t device, uint64_t capacity, mee_changes** out) {
    MEE_RANGE("mee_changes_create");
    if (!out) return fail(MEE_ERR_INVALID_ARG, "mee_changes_create: null argument");
    *out = nullptr;
    if (capacity == 0 || capacity > (1ull << 40)) return fail(MEE_ERR_INVALID_ARG, "mee_changes_create: capacity must be in [1, 2^40]");
    if (int rc = changes_device_check(device, "mee_changes_create")) return rc;
    DeviceGuard g(device);
    if (g.err != hipSuccess) return fail(MEE_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(g.err));
    mee_changes* c = new (std::nothrow) mee_changes();
    if (!c) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    c->device = device;
    c->nb = next_prime((capacity + kW - 1) / kW);   // SPEC.md §2, as mee_table_create rounds
    c->capacity = c->nb * kW;
    c->keys = nullptr; c->state = nullptr;
    hipError_t e = hipMalloc((void**)&c->keys, c->capacity * sizeof(int64_t));
    if (e == hipSuccess) e = hipMalloc((void**)&c->state, sizeof(ChangeState));
    if (e == hipSuccess) {
        changes_clear_kernel<<<grid_for(c->capacity, 256, 2048), 256, 0, nullptr>>>(change_set_of(c), c->capacity);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipFree(c->keys); (void)hipFree(c->state);
        delete c;
        return fail(e == hipErrorOutOfMemory ? MEE_ERR_OUT_OF_MEMORY : MEE_ERR_HIP, "mee_changes_create: %s", hipGetErrorString(e));
    }
    *out = c;
    return MEE_OK;
}

int mee_changes_destroy(mee_changes* c) {
    if (!c) return MEE_OK;
    DeviceGuard g(c->device);
    (void)hipFree(c->keys); (void)hipFree(c->state);
    delete c;
    return MEE_OK;
}

int mee_changes_note(mee_changes* c, const int64_t* d_keys, size_t n, void* stream) {
    MEE_RANGE("mee_changes_note");
    if (!c || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_changes_note: null argument");
    if (n == 0) return MEE_OK;
    DeviceGuard g(c->device);
    changes_note_kernel<<<grid_for(n, 16 * kNoteRounds, 1u << 16), 256, 0, as_stream(stream)>>>(change_set_of(c), d_keys, n);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_changes_group_create(mee_changes* const* logs, uint32_t n_tables, mee_changes_group** out) {
    MEE_RANGE("mee_changes_group_create");
    if (!logs || !out) return fail(MEE_ERR_INVALID_ARG, "mee_changes_group_create: null argument");
    *out = nullptr;
    if (n_tables == 0 || n_tables > kMaxGroupTables) return fail(MEE_ERR_INVALID_ARG, "mee_changes_group_create: n_tables must be in [1, %u]", kMaxGroupTables);
    std::vector<ChangeSet> sets(n_tables);
    std::vector<uint64_t> bounds(n_tables + 1, 0);
    for (uint32_t j = 0; j < n_tables; ++j) {
        if (!logs[j]) return fail(MEE_ERR_INVALID_ARG, "mee_changes_group_create: log %u is null", j);
        if (logs[j]->device != logs[0]->device)
            return fail(MEE_ERR_INVALID_ARG, "mee_changes_group_create: log %u is on device %d, log 0 on device %d", j, logs[j]->device, logs[0]->device);
        sets[j] = change_set_of(logs[j]);
        bounds[j + 1] = bounds[j] + ((logs[j]->capacity + 63) & ~63ull);
    }
    DeviceGuard g(logs[0]->device);
    mee_changes_group* grp = new (std::nothrow) mee_changes_group();
    if (!grp) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    grp->device = logs[0]->device; grp->n_tables = n_tables; grp->d_logs = nullptr; grp->d_bounds = nullptr; grp->walk_slots = bounds[n_tables];
    hipError_t e = hipMalloc((void**)&grp->d_logs, n_tables * sizeof(ChangeSet));
    if (e == hipSuccess) e = hipMalloc((void**)&grp->d_bounds, bounds.size() * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(grp->d_logs, sets.data(), n_tables * sizeof(ChangeSet), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(grp->d_bounds, bounds.data(), bounds.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(grp->d_logs); (void)hipFree(grp->d_bounds);
        delete grp;
        return fail(e == hipErrorOutOfMemory ? MEE_ERR_OUT_OF_MEMORY : MEE_ERR_HIP, "mee_changes_group_create: %s", hipGetErrorString(e));
    }
    *out = grp;
    return MEE_OK;
}

int mee_changes_group_destroy(mee_changes_group* g) {
    if (!g) return MEE_OK;
    DeviceGuard guard(g->device);
    (void)hipFree(g->d_logs); (void)hipFree(g->d_bounds);
    delete g;
    return MEE_OK;
}

int mee_changes_group_note(mee_changes_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* stream) {
    MEE_RANGE("mee_changes_group_note");
    if (!g || !d_offsets || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_changes_group_note: null argument");
    if (n == 0) return MEE_OK;
    DeviceGuard guard(g->device);
    changes_group_note_kernel<<<grid_for(n, 16 * kNoteRounds, 8192), 256, 0, as_stream(stream)>>>(g->d_logs, g->n_tables, d_offsets, d_keys, n);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_changes_info_get(const mee_changes* c, mee_changes_info* out) {
    MEE_RANGE("mee_changes_info_get");
    if (!c || !out) return fail(MEE_ERR_INVALID_ARG, "mee_changes_info_get: null argument");
    DeviceGuard g(c->device);
    ChangeState s;
    MEE_HIP(hipDeviceSynchronize());   // [syncs]: behind every note of every stream
    MEE_HIP(hipMemcpy(&s, c->state, sizeof s, hipMemcpyDeviceToHost));
    out->capacity = c->capacity;
    out->size = s.size;
    out->invalid = s.invalid;
    out->pad = 0;
    return MEE_OK;
}

int mee_changes_clear(mee_changes* c, void* stream) {
    MEE_RANGE("mee_changes_clear");
    if (!c) return fail(MEE_ERR_INVALID_ARG, "mee_changes_clear: null argument");
    DeviceGuard g(c->device);
    changes_clear_kernel<<<grid_for(c->capacity, 256, 2048), 256, 0, as_stream(stream)>>>(change_set_of(c), c->capacity);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_changes_invalidate(mee_changes* c, void* stream) {
    MEE_RANGE("mee_changes_invalidate");
    if (!c) return fail(MEE_ERR_INVALID_ARG, "mee_changes_invalidate: null argument");
    DeviceGuard g(c->device);
    changes_invalidate_kernel<<<1, 1, 0, as_stream(stream)>>>(c->state);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_export_changed(const mee_table* t, const mee_changes* c, uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out,
                       float* d_state1_out, float* d_state2_out, size_t cap, int64_t* d_removed_out, size_t removed_cap, uint64_t* d_counts_out, void* stream) {
    MEE_RANGE("mee_export_changed");
    if (!t || !c || !d_keys_out || !d_values_out || !d_removed_out || !d_counts_out) return fail(MEE_ERR_INVALID_ARG, "mee_export_changed: null argument");
    MEE_FP32_ROWS_ONLY(t, "mee_export_changed");   // a serving table has no training delta
    if (t->device != c->device) return fail(MEE_ERR_INVALID_ARG, "mee_export_changed: the table is on device %d, the change log on device %d", t->device, c->device);
    const uint64_t end = slot_end < c->capacity ? slot_end : c->capacity;
    const uint64_t slots = slot_begin < end ? end - slot_begin : 0;
    if (cap < slots || removed_cap < slots)   // a range of S slots holds at most S keys, and all of them may land in either list
        return fail(MEE_ERR_INVALID_ARG, "mee_export_changed: cap=%zu / removed_cap=%zu below the %llu slots of the range", cap, removed_cap, (unsigned long long)slots);
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(d_counts_out, 2 * sizeof(uint64_t), st);
    if (slots) {
        ChangedPlanes pl{};
        int np = 0;
        pl.src[np] = (const float4*)t->values; pl.dst[np++] = (float4*)d_values_out;
        if (t->s1 && d_state1_out) { pl.src[np] = (const float4*)t->s1; pl.dst[np++] = (float4*)d_state1_out; }
        if (t->s2 && d_state2_out) { pl.src[np] = (const float4*)t->s2; pl.dst[np++] = (float4*)d_state2_out; }
        with_row_shape(t->dim4, [&](auto d4) { with_value<1, 2, 3>(np, [&](auto n_planes) {
            export_changed_kernel<d4, n_planes><<<grid_for(slots, 256, 1u << 16), 256, 0, st>>>(c->keys, slot_begin, end, t->keys, t->nb, pl, t->dim4, d_keys_out, cap,
                                                                                             d_removed_out, removed_cap, (unsigned long long*)d_counts_out);
        }); });
    }
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_publish_changed(const mee_table* src, const mee_changes* log, mee_table* dst, uint64_t slot_begin, uint64_t slot_end, uint64_t* d_counts_out, void* stream) {
    MEE_RANGE("mee_publish_changed");
    if (!src || !log || !dst || !d_counts_out) return fail(MEE_ERR_INVALID_ARG, "mee_publish_changed: null argument");
    if (int rc = publish_pair_check(src, dst, "mee_publish_changed", -1)) return rc;
    if (src->device != log->device) return fail(MEE_ERR_INVALID_ARG, "mee_publish_changed: the tables are on device %d, the change log on device %d", src->device, log->device);
    const uint64_t end = slot_end < log->capacity ? slot_end : log->capacity;
    const uint64_t slots = slot_begin < end ? end - slot_begin : 0;
    DeviceGuard g(src->device);
    hipStream_t st = as_stream(stream);
    zero_words(d_counts_out, 4 * sizeof(uint64_t), st);
    if (slots) {
        ++dst->handle_epoch;   // rows are freed: slot handles handed out before this call are stale
        const PublishTables t{src->keys, (const float4*)src->values, src->nb, dst->keys, dst->values, dst->nb, &dst->ctr->status, dst->hits};
        const unsigned grid = grid_for(slots, 256, 1u << 16);
        unsigned long long* counts = (unsigned long long*)d_counts_out;
        with_row_shape(src->dim4, [&](auto d4) { with_flag(dst->bf16_rows, [&](auto bf16) {
            publish_upsert_kernel<d4, bf16><<<grid, 256, 0, st>>>(change_set_of(log), slot_begin, end, t, src->dim4, counts);
        }); });
        publish_remove_kernel<<<grid, 256, 0, st>>>(change_set_of(log), slot_begin, end, t, counts);
    }
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_group_publish_changed(const mee_group* src, const mee_changes_group* logs, mee_group* dst, uint64_t* d_counts_out, void* stream) {
    MEE_RANGE("mee_group_publish_changed");
    if (!src || !logs || !dst || !d_counts_out) return fail(MEE_ERR_INVALID_ARG, "mee_group_publish_changed: null argument");
    if (src == dst) return fail(MEE_ERR_INVALID_ARG, "mee_group_publish_changed: src and dst are the same group");
    if (src->n_tables != dst->n_tables || src->n_tables != logs->n_tables || src->dim != dst->dim || src->device != dst->device || src->device != logs->device)
        return fail(MEE_ERR_INVALID_ARG, "mee_group_publish_changed: src, logs and dst differ in the number of tables (%u, %u, %u), dim (%u, %u) or device (%d, %d, %d)", src->n_tables,
                    logs->n_tables, dst->n_tables, src->dim, dst->dim, src->device, logs->device, dst->device);
    for (uint32_t j = 0; j < src->n_tables; ++j)
        if (int rc = publish_pair_check(src->tables[j], dst->tables[j], "mee_group_publish_changed", (int)j)) return rc;
    {   // a table that is a member twice would be probed read-only by one member's walk while another claims in it
        std::vector<const mee_table*> all(src->tables.begin(), src->tables.end());
        all.insert(all.end(), dst->tables.begin(), dst->tables.end());
        std::sort(all.begin(), all.end());
        if (std::adjacent_find(all.begin(), all.end()) != all.end())
            return fail(MEE_ERR_INVALID_ARG, "mee_group_publish_changed: a table is a member more than once across the two groups");
    }
    if (int rc = group_refresh(const_cast<mee_group*>(src), stream)) return rc;   // (re-reads the planes of a member that was rehashed: a cache, not the group's value)
    if (int rc = group_refresh(dst, stream)) return rc;
    DeviceGuard guard(src->device);
    hipStream_t st = as_stream(stream);
    const uint32_t nt = src->n_tables;
    zero_words(d_counts_out, (size_t)nt * 4 * sizeof(uint64_t), st);
    for (mee_table* t : dst->tables) ++t->handle_epoch;
    const unsigned grid = grid_for(logs->walk_slots, 256, 8192);
    unsigned long long* counts = (unsigned long long*)d_counts_out;
    with_row_shape(src->dim4, [&](auto d4) { with_flag(dst->bf16_rows, [&](auto bf16) {
        publish_upsert_grouped_kernel<d4, bf16><<<grid, 256, 0, st>>>(logs->d_logs, logs->d_bounds, nt, src->d_move, dst->d_move, src->dim4, counts);
    }); });
    publish_remove_grouped_kernel<<<grid, 256, 0, st>>>(logs->d_logs, logs->d_bounds, nt, src->d_move, dst->d_move, counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
