// meepo_find.hip — the lookups of the table: find (the headline kernel), the training forward (find + the apply's partition in one
// launch), find_many, the sparse second pass, pooled find; their half of the C-ABI.  Table layout and scratch: meepo_table.hip,
// meepo_table_int.h.  Reference anchor: /root/reference/README.md:2 (no code in the snapshot: semantics from SPEC.md §3).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "meepo_apply_part.h"
#include "meepo_find_coalesce.h"


namespace mee {

// ---- find (SPEC.md §3) — the headline kernel --------------------------------------------------------------
// One tile per key, R keys in flight per tile: the R bucket lines are requested back to back, then the R rows.
// DIM4 = dim/4 when it is a multiple of 16 (each lane moves DIM4/16 element groups per row), 0 = any dim at run time.
// ROWS: the storage type of `values` (RowType, meepo_device.h).  Every type has the same tiles, the same R keys in flight and the same index arithmetic on
// the output; what a lane loads per element group (16, 8 or 4 bytes, an int8 row's scale word beside them), what a missing key reads and how a group leaves
// as fp32 or bf16 is RowType's.  fp32 and bf16 rows share one gather written through it; the int8 gather is a block of its own in find_span (the same
// steps spelled out: through the shared blocks its dim-64 instances measured slower).  A bf16-row or int8-row plane is served by the plain find only
// (mee_find / _ex / _as: the hint bits and kFindBF16Out).
//
// NT: the policy bits of an instance.  The numbers are part of the kernels' names (find_kernel<16, 2, 64>), which profiles/ and tools/ key on.
constexpr int kFindStreamRows = 1;      // row loads are non-temporal (a stream without reuse).  Compiled row shapes only: the run-time shape (DIM4 = 0) loads cached
constexpr int kFindStreamBuckets = 2;   // the first bucket line of every key is loaded non-temporal; every shape
constexpr int kFindCachedStores = 4;    // the result rows leave as plain stores (they stay in L2 / the Infinity Cache for whoever reads them next); without it
                                        // as streaming stores (RowStore).  Compiled row shapes only: the run-time shape stores cached
constexpr int kFindCountHits = 16;      // one atomicAdd to hits[slot] per found position: access statistics for the hot/cold policy (sampled calls)
constexpr int kFindLocated = 64;        // mee_find_located: slots_out[i] = the slot handle of position i (-1 = absent), for the apply of the same step
constexpr int kFindSkipPadding = 128;   // owner side of a padded sharded exchange: an EMPTY position is padding nobody reads: no row, found byte 1
constexpr int kFindBF16Out = 256;       // `out` is a bf16 array (SPEC.md §3 "Output type"): an element group leaves as 4 bf16 in one 8-byte store
// the three bits a caller's hint carries: the table's "find_nt" setting and the MEE_FIND_* flags of mee_find_ex / mee_find_as
constexpr int kFindHintBits = kFindStreamRows | kFindStreamBuckets | kFindCachedStores;

// the store of one dequantized element group of an int8 ROW under find_span's NT bits: a float4, or 4 bf16 rounded here, once
// (compiled shapes: group g of the wave step `st`, which is index `first + g` of `out`)
template <int NT, bool CACHED>
__device__ __forceinline__ void store_qrow(f32x4* __restrict__ out, uint64_t first, const RowStore<CACHED>& st, uint32_t g, const f32x4 v) {
    if constexpr ((NT & kFindBF16Out) != 0) store_bf16x4<CACHED>(out, first + g, v);
    else st(g, v);
}

// the find of n positions by `n_waves` waves of which this is wave `wave` (each wave step takes 4R consecutive positions)
template <int DIM4, int R, int NT, int ROWS = kRowsF32>
__device__ __forceinline__ void find_span(const int64_t* __restrict__ tkeys, const f32x4* __restrict__ values, uint64_t nb,
                                          const int64_t* __restrict__ keys, uint64_t n, f32x4* __restrict__ out,
                                          uint8_t* __restrict__ found, float defv, uint32_t dim4_rt, uint32_t* hits,
                                          int64_t* __restrict__ slots_out, uint64_t wave, uint64_t n_waves, int64_t handle_tag = 0) {
    static_assert(ROWS == kRowsF32 || (NT & ~(kFindHintBits | kFindBF16Out)) == 0, "bf16 rows and int8 rows: the plain find only");
    using RT = RowType<ROWS>;
    constexpr bool STREAM_ROWS = (NT & kFindStreamRows) != 0, CACHED = (NT & kFindCachedStores) != 0, BF16_OUT = (NT & kFindBF16Out) != 0;
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int KPW = 4 * R;
    const f32x4 def4 = {defv, defv, defv, defv};
    const typename RT::Group* __restrict__ plane = RT::plane(values);

    for (uint64_t base = wave * KPW; base < n; base += n_waves * KPW) {
        const RowStore<CACHED> st(out, base * DIM4);   // the step's fp32 result rows (compiled shapes; bf16 out and the run-time shape store for themselves)
        int64_t key[R];
        int64_t slot[R];
        uint64_t b[R];
        int64_t kb[R];
        bool inb[R], act[R];
        // ONE coalesced load brings the wave step's 4R keys (lane j reads keys[base + j]); the tiles take theirs by shuffle.  (A load per
        // tile and round made the compiler wait for round r's key before it requested round r + 1's: a dependent memory round trip per round.)
        const int64_t kmine = (lane < KPW && base + lane < n) ? keys[base + lane] : kEmpty;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            inb[r] = i < n;
            key[r] = __shfl(kmine, r * 4 + tile);
            act[r] = inb[r] && !reserved_key(key[r]);
            if constexpr ((NT & kFindSkipPadding) != 0) {  // the found byte of padding says "served" so that a second-tier pass over the same buffers (mee_find_missing
                // / mee_find_or_insert_missing on the cold table of a tiered shard) leaves it alone instead of reading a byte nobody wrote
                if (inb[r] && !act[r] && tl == 0 && found) found[i] = 1;
                inb[r] = act[r];
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            b[r] = bucket_of(key[r], nb);
            kb[r] = act[r] ? ((NT & kFindStreamBuckets) ? __builtin_nontemporal_load(&tkeys[b[r] * kW + tl]) : tkeys[b[r] * kW + tl]) : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys, nb, key[r], act[r], b[r], kb[r], tile, tl);
        if constexpr ((NT & kFindCountHits) != 0) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (slot[r] >= 0 && tl == 0) atomicAdd(&hits[slot[r]], 1u);
        }
        if constexpr (ROWS == kRowsI8) {
            // The parent text of the int8 gather: through the shared blocks below the dim-64 instances measured 6-11 % slower (profiles/find_row_types.md)
            const uint32_t* __restrict__ qrows = reinterpret_cast<const uint32_t*>(values);
            if constexpr (DIM4 != 0) {
                constexpr int C = DIM4 / 16;
                uint32_t row[R][C], sc[R];
                bool all_hit = true;   // the wave-uniform common case, as below
#pragma unroll
                for (int r = 0; r < R; ++r) all_hit = all_hit && inb[r] && slot[r] >= 0;
                if (__all(all_hit)) {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t* __restrict__ q = qrows + i8_row_word(slot[r], DIM4);
#pragma unroll
                        for (int c = 0; c < C; ++c) row[r][c] = STREAM_ROWS ? __builtin_nontemporal_load(&q[c * 16 + tl]) : q[c * 16 + tl];
                        sc[r] = STREAM_ROWS ? __builtin_nontemporal_load(&q[DIM4]) : q[DIM4];
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
#pragma unroll
                        for (int c = 0; c < C; ++c) store_qrow<NT>(out, base * DIM4, st, (r * 4 + tile) * DIM4 + c * 16 + tl, dequant_i8x4(row[r][c], __builtin_bit_cast(float, sc[r])));
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const uint32_t* __restrict__ q = qrows + i8_row_word(slot[r] >= 0 ? slot[r] : 0, DIM4);
#pragma unroll
                        for (int c = 0; c < C; ++c) row[r][c] = slot[r] >= 0 ? (STREAM_ROWS ? __builtin_nontemporal_load(&q[c * 16 + tl]) : q[c * 16 + tl]) : 0u;
                        sc[r] = slot[r] >= 0 ? (STREAM_ROWS ? __builtin_nontemporal_load(&q[DIM4]) : q[DIM4]) : 0u;
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        if (inb[r]) {
#pragma unroll
                            for (int c = 0; c < C; ++c)
                                store_qrow<NT>(out, base * DIM4, st, (r * 4 + tile) * DIM4 + c * 16 + tl, slot[r] >= 0 ? dequant_i8x4(row[r][c], __builtin_bit_cast(float, sc[r])) : def4);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t i = base + r * 4 + tile;
                    if (inb[r]) {
                        const uint32_t* __restrict__ q = qrows + i8_row_word(slot[r] >= 0 ? slot[r] : 0, dim4);
                        const float scale = slot[r] >= 0 ? __builtin_bit_cast(float, q[dim4]) : 0.f;
                        for (uint32_t c = tl; c < dim4; c += 16) {
                            const f32x4 v = slot[r] >= 0 ? dequant_i8x4(q[c], scale) : def4;
                            if constexpr (BF16_OUT) store_bf16x4<true>(out, i * dim4 + c, v); else out[i * dim4 + c] = v;
                        }
                    }
                }
            }
        } else if constexpr (DIM4 != 0) {
            constexpr int C = DIM4 / 16;
            typename RT::Group row[R][C];
            uint32_t tail[R];
            // Common case, decided per wave: every position of the wave step is inside the batch and was found.  Then the R row loads
            // and the R stores are straight-line code and leave back to back; with a per-lane condition around each load the compiler
            // waited for round r's row before it requested round r + 1's (seen in the ISA of the located variant: +8 us per 256K keys).
            bool all_hit = true;
#pragma unroll
            for (int r = 0; r < R; ++r) all_hit = all_hit && inb[r] && slot[r] >= 0;
            if (__all(all_hit)) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
#pragma unroll
                    for (int c = 0; c < C; ++c) row[r][c] = RT::template load<STREAM_ROWS>(&plane[RT::first(slot[r], DIM4) + c * 16 + tl]);
                    tail[r] = RT::template load_tail<STREAM_ROWS, true>(plane, slot[r], DIM4);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t i = base + r * 4 + tile;
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if constexpr (BF16_OUT) RT::template store_bf16<CACHED>(out, i * DIM4 + c * 16 + tl, row[r][c], tail[r], true, def4);
                        else st((r * 4 + tile) * DIM4 + c * 16 + tl, RT::value(row[r][c], tail[r], true, def4));
                    }
                }
                // An empty statement that keeps this block's tail its own.  The compiler merged the step's last store with the last store of the per-lane
                // path below, and the merged block waits with vmcnt(0): for the row it stores, and with it for every store of the step issued before it.
                // Apart, the stores leave behind a vmcnt(k) ladder, each as its own row arrives: 32.1 -> 31.2 us per 256K-key launch into rotating buffers
                // (profiles/find_write_through.md).  Streaming fp32 stores only: the cached and the bf16-out instances go without.
                if constexpr (!CACHED && !BF16_OUT) asm volatile("; find_span: end of the all-hit stores");
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        row[r][c] = slot[r] >= 0 ? RT::template load<STREAM_ROWS>(&plane[RT::first(slot[r], DIM4) + c * 16 + tl]) : RT::missing(def4);
                    tail[r] = RT::template load_tail<STREAM_ROWS, false>(plane, slot[r], DIM4);
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t i = base + r * 4 + tile;
                    if (inb[r]) {
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            if constexpr (BF16_OUT) RT::template store_bf16<CACHED>(out, i * DIM4 + c * 16 + tl, row[r][c], tail[r], slot[r] >= 0, def4);
                            else st((r * 4 + tile) * DIM4 + c * 16 + tl, RT::value(row[r][c], tail[r], slot[r] >= 0, def4));
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (inb[r]) {
                    const uint32_t tail = RT::template load_tail<false, false>(plane, slot[r], dim4);
                    for (uint32_t c = tl; c < dim4; c += 16)
                        RT::template store<BF16_OUT, true>(out, i * dim4 + c, slot[r] >= 0 ? plane[RT::first(slot[r], dim4) + c] : RT::missing(def4), tail, slot[r] >= 0, def4);
                }
            }
        }
        if constexpr ((NT & kFindLocated) != 0) {
            const int64_t mine = collect_slots(slot, lane);   // ONE coalesced store per wave step
            if (lane < KPW && base + lane < n) slots_out[base + lane] = mine >= 0 ? (mine | handle_tag) : mine;   // tag: the table's layout epoch (see handle_tag_of)
        }
        if (found) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i0 = base + r * 4;
                if ((NT & kFindSkipPadding) == 0 && i0 + 4 <= n && (reinterpret_cast<uintptr_t>(found) & 3) == 0) {
                    // the four tiles' found bytes of this round leave as ONE aligned 4-byte store
                    const uint64_t m = __ballot(slot[r] >= 0);
                    const uint32_t w = (uint32_t)(m & 1) | ((uint32_t)((m >> 16) & 1) << 8) | ((uint32_t)((m >> 32) & 1) << 16) |
                                       ((uint32_t)((m >> 48) & 1) << 24);
                    if (lane == 0) *reinterpret_cast<uint32_t*>(found + i0) = w;
                } else {
                    const uint64_t i = i0 + tile;
                    if (inb[r] && tl == 0) found[i] = slot[r] >= 0;   // (kFindSkipPadding: inb excludes padding)
                }
            }
        }
    }
}

template <int DIM4, int R, int NT, int ROWS = kRowsF32>
__global__ __launch_bounds__(256) void find_kernel(const int64_t* __restrict__ tkeys, const f32x4* __restrict__ values,
                                                   uint64_t nb, const int64_t* __restrict__ keys, uint64_t n,
                                                   f32x4* __restrict__ out, uint8_t* __restrict__ found, float defv,
                                                   uint32_t dim4_rt, uint32_t* hits, int64_t* __restrict__ slots_out = nullptr, int64_t handle_tag = 0) {
    find_span<DIM4, R, NT, ROWS>(tkeys, values, nb, keys, n, out, found, defv, dim4_rt, hits, slots_out,
                           (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), (uint64_t)gridDim.x * (blockDim.x >> 6), handle_tag);
}

// The training forward (mee_find_located_prepare): the located find whose launch gives its first `part_blocks` blocks the partition role of
// the bucketed apply (meepo_apply_part.h).  The partition of the step's backward — a latency-bound 15-18 us of LDS histograms for a 256K-key
// batch — runs beside the forward's row gather, which is bound by bytes and takes twice as long: the backward starts with its update kernel.
// Block size = the find's own 256 threads.  The first version used 1024-thread blocks for the sake of the partition role (64 blocks x 1024
// threads); measured with the role switched off, the FIND in 1024-thread blocks takes 47 us against 39 us in 256-thread blocks (a block's 16
// waves each do one short pass, the block holds its 16 wave slots until the slowest of them is done; 512-thread blocks: 42 us) — the launch
// took as long as its slow find and hid nothing.  With 256-thread blocks the role runs as 128 blocks x 256 threads x 8 keys, each making two
// round trips to memory (meepo_apply_part.h): 42.5 us for the launch against 40 us with the role switched off.
constexpr int kFindPrepareThreads = 256;
constexpr int kFindPrepareR = 2;   // keys in flight per tile at dim 64
template <int DIM4, int R, int NT>
__global__ __launch_bounds__(kFindPrepareThreads, 8) void find_prepare_kernel(const int64_t* __restrict__ tkeys, const f32x4* __restrict__ values, uint64_t nb,
                                                           const int64_t* __restrict__ keys, uint64_t n, f32x4* __restrict__ out,
                                                           uint8_t* __restrict__ found, float defv, uint32_t dim4_rt, int64_t* __restrict__ slots_out,
                                                           int64_t handle_tag, uint32_t part_blocks, uint32_t nbk_hash, uint32_t nbk, uint32_t per_block,
                                                           BucketScratch bk, uint32_t* status, OpCounters* op, uint32_t xcd_split) {
    extern __shared__ unsigned long long part_lds[];   // PartHot, then one counter per bucket (meepo_apply_part.h)
    __shared__ unsigned long long part_wsum[kFindPrepareThreads / 64];
    if (blockIdx.x < part_blocks) {   // block-uniform
        PartHot* hot = reinterpret_cast<PartHot*>(part_lds);
        sort_role<kFindPrepareThreads>(keys, (uint32_t)n, nbk_hash, nbk, per_block, blockIdx.x, part_blocks, bk, status, op, reinterpret_cast<uint32_t*>(hot + 1), part_wsum, hot, true, xcd_split);
        return;
    }
    find_span<DIM4, R, NT>(tkeys, values, nb, keys, n, out, found, defv, dim4_rt, nullptr, slots_out,
                           (uint64_t)(blockIdx.x - part_blocks) * (blockDim.x >> 6) + (threadIdx.x >> 6), (uint64_t)(gridDim.x - part_blocks) * (blockDim.x >> 6),
                           handle_tag);
}

// Several lookup requests of one table in ONE launch (mee_find_many; consecutive finds of a stream capture: find_captured below): the per-launch
// latency floor (~5 us: dispatch + the dependent chain of the first and last waves) is paid once for all of them, so four queued 256K-key requests
// run at the rate of one 1M-key launch.  The request descriptors (FindMany, meepo_find_coalesce.h) travel in the kernel argument; a block finds its
// request by its index.  A request's blocks stride over it like find_kernel's grid over its batch.
template <int DIM4, int R, int NT>
__global__ __launch_bounds__(256) void find_many_kernel(const int64_t* __restrict__ tkeys, const f32x4* __restrict__ values, uint64_t nb,
                                                        FindMany m, float defv, uint32_t dim4_rt) {
    // The request of a block: how many of first_block[1..15] it has reached — behind the grid size the entries hold 0xFFFFFFFF (find_many_append) —, counted
    // in straight-line code.  (A search loop cost a dependent scalar load per request in front of the block's own, the request's fields a round trip
    // behind it, the block size and the table's planes two more: a launch of ONE request took 33.3 us where find_kernel takes 32.3.)  The empty asm
    // statement wants every argument the block needs in a register: the scalar loads — request 0's fields among them — leave as ONE batch at the top
    // and a block of request 0 starts after one round trip; the blocks of later requests load their fields in a second one, once q is known.
    const int64_t* keys = m.keys[0];
    uint64_t n = m.n[0];
    f32x4* out = m.out[0];
    uint8_t* found = m.found[0];
    uint32_t fb[kMaxFindRequests];
#pragma unroll
    for (int i = 1; i < kMaxFindRequests; ++i) fb[i] = m.first_block[i];
    uint32_t bdim = blockDim.x;
    asm volatile("; find_many_kernel: arguments" : "+s"(tkeys), "+s"(values), "+s"(nb), "+s"(defv), "+s"(keys), "+s"(n), "+s"(out), "+s"(found), "+s"(bdim),
                 "+s"(fb[1]), "+s"(fb[2]), "+s"(fb[3]), "+s"(fb[4]), "+s"(fb[5]), "+s"(fb[6]), "+s"(fb[7]));
    uint32_t q = 0;
#pragma unroll
    for (int i = 1; i < kMaxFindRequests; ++i) q += blockIdx.x >= fb[i];
    uint32_t first = 0, end = fb[1];
    if (q != 0) {   // block-uniform
        keys = m.keys[q]; n = m.n[q]; out = m.out[q]; found = m.found[q];
        first = m.first_block[q]; end = m.first_block[q + 1];
    }
    find_span<DIM4, R, NT>(tkeys, values, nb, keys, n, out, found, defv, dim4_rt, nullptr, nullptr,
                           (uint64_t)(blockIdx.x - first) * (bdim >> 6) + (threadIdx.x >> 6), (uint64_t)(end - first) * (bdim >> 6));
}

// ---- sparse second pass (SPEC.md §3 find_missing; last pass of find_or_insert): only positions whose found byte is 0 -----
// A wave reads 64 keys + found bytes with one coalesced load each and leaves at once when nothing is missing (the common
// case: a hot tier that holds the working set, a trained vocabulary); the missing ones are probed four at a time.
// FLAGS bit 0: set found[i] = 1 where the key is stored here (tier pass; off = rows only), bit 1: count the hit.
template <int FLAGS>
__global__ __launch_bounds__(256) void find_missing_kernel(const int64_t* __restrict__ tkeys, const float4* __restrict__ values,
                                                           uint64_t nb, uint32_t dim4, const int64_t* __restrict__ keys, uint64_t n,
                                                           float4* __restrict__ out, uint8_t* __restrict__ found, uint32_t* hits) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 64; base < n; base += n_waves * 64) {
        const uint64_t i = base + lane;
        const int64_t k = i < n ? keys[i] : kEmpty;
        uint64_t rest = __ballot(i < n && found[i] == 0 && !reserved_key(k));
        while (rest) {  // wave-uniform
            uint64_t mm = rest;
            int p = -1;
            for (int q = 0; q <= tile; ++q) {
                if (mm) { p = __ffsll((unsigned long long)mm) - 1; mm &= mm - 1; } else p = -1;
            }
            const int64_t key = __shfl(k, p >= 0 ? p : 0);
            bool is_new, full;
            const int64_t slot = tile_locate<false, false>(const_cast<int64_t*>(tkeys), nb, key, p >= 0, tile, tl, is_new, full);
            if (p >= 0 && slot >= 0) {
                const uint64_t dst = (base + (uint64_t)p) * dim4, src = (uint64_t)slot * dim4;
                for (uint32_t c = tl; c < dim4; c += 16) out[dst + c] = values[src + c];
                if (tl == 0) {
                    if (FLAGS & 1) found[base + p] = 1;
                    if (FLAGS & 2) atomicAdd(&hits[slot], 1u);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) rest &= rest - 1;
        }
    }
}

// ---- pooled find (SPEC.md §3): out[b,:] = the rows of bag b's keys added up in position order (sum | mean) ----------------
// A bag costs ONE output row instead of one per key: with L keys per bag the write traffic of the lookup drops from 256 B per key
// to 256/L.  The walk over a wave's bags and the accumulation are pooled_bags (meepo_device.h); the kernels here say which table a bag
// belongs to and where its row goes.
// JAGGED bag -> member map (mee_group_find_pooled_jagged): the member j with member_bags[j] <= bag < member_bags[j + 1], by an upper-bound
// search over member_bags[1 .. n_members] (at most ten dependent reads of an L2-resident array for 1024 members).  The array is the
// caller's: whatever it holds, the member stays inside [0, n_members); false = the bag lies outside [member_bags[0], member_bags[n_members]).
__device__ __forceinline__ bool jagged_member(const uint64_t* __restrict__ member_bags, uint32_t n_members, uint64_t bag, uint64_t& member) {
    uint32_t lo = 0, hi = n_members;   // lo ends as the number of entries member_bags[1 .. n_members] that are <= bag
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (member_bags[mid + 1] <= bag) lo = mid + 1; else hi = mid;
    }
    member = lo < n_members ? lo : (n_members ? n_members - 1 : 0);   // (a group has at least one table: mee_group_create refuses none; the launch checks again)
    return lo < n_members && bag >= member_bags[0];
}

// BPW = bags per wave: 4 = a tile per short bag, the four tiles together on a long one (batches of mostly short bags), 1 = every bag gets
// a whole wave (batches whose AVERAGE bag is long: a wave that had to walk four long bags one after the other would be latency-bound).
// The body is pooled_bags per wave step (a group's four-bags-per-wave instances excepted: they keep a copy of the walk, see the loop), with two callables: table_of — the kernel's own table arguments for one table; with GROUPED
// (mee_group_find_pooled) the descriptor of member b / bags_per_table; with JAGGED (mee_group_find_pooled_jagged: the members' bag counts
// differ) that of the member jagged_member finds, and a bag outside the map is empty — and row_of, b * dim4.  The other parameters go
// through to the walk:
// WEIGHTED (mee_find_pooled_weighted / mee_group_find_pooled_weighted): position i adds weights[i] * row_i; SUM only.  A single table's
// located rows then carry its handle tag and -1 for an absent key (TAGGED), a group's the member and EMPTY.
// BF16: `out` holds bf16 rows (SPEC.md §3 "Output type").
// TIERED (mee_find_pooled_tiered; one hot/cold pair, unweighted): the table arguments are the HOT table's, `tier` brings the cold one.
// GROUPED && TIERED (mee_group_find_pooled_tiered; a collection of pairs, unweighted, no jagged map, no located rows): `desc` holds the HOT
// members, `tier` is a GroupTier — the cold members' descriptors, both groups' GroupInit (for the hit counters) and the launch's count bits.
// Bag b's hot AND cold table are member b / bags_per_table's: table_of fills in both, per tile in the short phase of a four-bags-per-wave
// step (bags_per_table need not be a multiple of 4: one wave may serve two members) and again for bag q in the long phase.  Both launch
// shapes go through pooled_bags; a member's counters are read only under the launch's count bit.  With JAGGED as well
// (mee_group_find_pooled_tiered_jagged: the owner's side of a sharded group of pairs) the member is jagged_member's instead of b / bags_per_table
// and a bag outside the map is empty; fp32 out only.
// BROWS (one bf16-row table, or with GROUPED a bf16-row group — every member's plane, JAGGED included; unweighted: SPEC.md §3 "Row
// storage type"): the value planes hold bf16 rows.  One storage type per group, so this is a property of the launch, never a per-member
// branch in the fetch.
// KEYED (mee_group_find_pooled_keyed / mee_group_find_pooled_tiered_keyed; a uniform group or a group of pairs, unweighted, no jagged map: SPEC.md §3
// "Keyed output"): bag b = member j's sample s (j = b / bags_per_table) is written to out[s * stride4 + j * dim4 ...] — one row per sample, the members'
// pooled vectors side by side — instead of out[b * dim4 ...], and tier.keyed (KeyedOut, meepo_device.h) also brings the step index, written per wave step
// beside the walk.  Only row_of differs inside it: the order of the additions and the mean's division are the table-major instances'.  KeyedOut rides
// behind the last argument (KeyedArg), so the table-major instances keep their argument list as it was.
// (GroupTier and group_pair_tables, the pair of a member: meepo_table_int.h — the padded lookup of a group of pairs reads them too)
template <int DIM4, int U, int BPW, bool GROUPED = false, bool WEIGHTED = false, bool BF16 = false, bool JAGGED = false, bool TIERED = false, bool BROWS = false, bool KEYED = false>
__global__ __launch_bounds__(256) void find_pooled_kernel(const int64_t* __restrict__ tkeys_, const float4* __restrict__ values_,
                                                          uint64_t nb_, const int64_t* __restrict__ keys,
                                                          const uint64_t* __restrict__ offsets, uint64_t n_bags,
                                                          float4* __restrict__ out, uint8_t* __restrict__ found, float defv,
                                                          uint32_t dim4_rt, int mean, const GroupDesc* __restrict__ desc = nullptr,
                                                          uint64_t bags_per_table = 1, int64_t* __restrict__ located = nullptr,
                                                          uint64_t n_keys = ~0ull, const float* __restrict__ weights = nullptr,
                                                          int64_t handle_tag = 0, const uint64_t* __restrict__ member_bags = nullptr,
                                                          uint32_t n_members = 0, KeyedArg<KEYED, std::conditional_t<GROUPED && TIERED, GroupTier, TierArgs>> tier = {}) {
    static_assert(!JAGGED || (GROUPED && !WEIGHTED && !BF16), "the jagged map is the group's plain fp32 lookup");
    static_assert(!KEYED || (GROUPED && !WEIGHTED && !JAGGED), "the keyed layout is the plain sum / mean of a group with bags_per_table bags per member");
    static_assert(!TIERED || (!WEIGHTED && (!JAGGED || GROUPED)), "the tiered form is the plain sum / mean of one pair or of a group of pairs (the group's also with a jagged map)");
    static_assert(!BROWS || (!WEIGHTED && !TIERED), "bf16 rows: the plain sum / mean of one table or of a bf16-row group (jagged map included)");
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 16;   // float4 per lane per row (any dim: up to 1024 floats = 16 per lane)
    constexpr bool TAGGED = WEIGHTED && !GROUPED;
    auto table_of = [&](uint64_t b, PooledTable& t) {
        if constexpr (GROUPED) {
            uint64_t member;
            bool in_map = true;
            if constexpr (JAGGED) in_map = jagged_member(member_bags, n_members, b, member);
            else member = b / bags_per_table;
            t = pooled_table(desc[member], member, kGroupSlotBits);
            return in_map;
        } else {
            t = PooledTable{tkeys_, values_, nb_, make_float4(defv, defv, defv, defv), TAGGED ? (uint64_t)handle_tag : 0};
            return true;
        }
    };
    auto row_of = [&](uint64_t b) {
        if constexpr (KEYED) { const uint64_t j = b / bags_per_table; return (b - j * bags_per_table) * tier.keyed.stride4 + j * dim4; }   // sample b mod B, member b / B
        else return b * dim4;
    };
    for (uint64_t b0 = wave * BPW; b0 < n_bags; b0 += n_waves * BPW) {
        if constexpr (KEYED) {   // the step index of this step's bags, beside the walk (keyed_step_index, meepo_device.h)
            if (tier.keyed.step_index)   // kernel-uniform
                keyed_step_index<BPW>(b0, (uint32_t)(n_bags - b0 < BPW ? n_bags - b0 : BPW), offsets, n_keys, tile, tl, tier.keyed.step_index, [&](uint64_t b) {
                    const uint64_t j = b / bags_per_table;
                    return (uint32_t)((b - j * bags_per_table) * tier.keyed.step_sample + j * tier.keyed.step_member);
                });
        }
        if constexpr (GROUPED && TIERED) {
            auto pair_of = [&](uint64_t b, PooledTable& t, TierArgs& cold) {   // the hot and the cold table of bag b's member
                uint64_t member;
                bool in_map = true;
                if constexpr (JAGGED) in_map = jagged_member(member_bags, n_members, b, member);   // (outside the map: an empty bag, the member still inside the group)
                else member = b / bags_per_table;
                group_pair_tables(desc, tier, member, t, cold);
                return in_map;
            };
            pooled_bags<DIM4, U, BPW, C, false, BF16, true, false, false>(b0, (uint32_t)(n_bags - b0 < BPW ? n_bags - b0 : BPW), dim4, keys, offsets, n_keys, nullptr, out, found,
                                                                          nullptr, mean, TierArgs{}, tile, tl, pair_of, row_of, tier.count);
        } else if constexpr (!(GROUPED && BPW == 4)) {
            pooled_bags<DIM4, U, BPW, C, WEIGHTED, BF16, TIERED, BROWS, TAGGED>(b0, (uint32_t)(n_bags - b0 < BPW ? n_bags - b0 : BPW), dim4, keys, offsets, n_keys, weights, out, found,
                                                                                (GROUPED && BROWS) ? nullptr : located,   // (a bf16-row group hands out no located rows: refused at the entry points)
                                                                                mean, tier, tile, tl, table_of, row_of);
        } else {
            // NOT converted: a group's four-bags-per-wave instances keep their own copy of the walk.  Through pooled_bags the collection step's
            // lookup (find_pooled_kernel<16, 2, 4, true>) measured 1 % above its time before (profiles/pooled_shared_body.md §2), and no way of
            // writing the callables brought it back.  A change to the order of the additions, the mean's division, the long-bag rule or the
            // clamping of the offsets in pooled_bags has to be made here too (tests/test_gpu_parity.py and test_mixed_groups.py compare the two).
            const uint64_t bag = b0 + tile;
            const bool has = bag < n_bags;
            uint64_t begin = has ? offsets[bag] : 0, end = has ? offsets[bag + 1] : 0;
            end = end < n_keys ? end : n_keys;          // offsets are the caller's: never read past the key array,
            begin = begin < end ? begin : end;          // and a decreasing pair is an empty bag
            uint64_t member = 0;
            if constexpr (JAGGED) {
                if (!jagged_member(member_bags, n_members, has ? bag : 0, member)) begin = end = 0;   // a bag outside the map: empty
            } else member = (has ? bag : 0) / bags_per_table;
            GroupDesc d = desc[member];
            const int64_t* tkeys = d.tkeys;
            const float4* values = d.values;
            uint64_t nb = d.nb;
            float4 def4 = make_float4(d.defv, d.defv, d.defv, d.defv);
            const bool is_long = end - begin >= kPoolLong;
            float4 acc[C];
            float4 row[U][C];
            // ---- short bags: one tile per bag ----
            if constexpr (BPW == 4) {
                uint64_t i = is_long ? end : begin;
                bool first = true;
    #pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                // a short bag has fewer than 16 keys: its tile fetches them all with one coalesced load, lane tl holds key begin + tl
                const int64_t kpre = (!is_long && begin + tl < end) ? keys[begin + tl] : kEmpty;
                float wpre = 0.f;   // the same for the weights
                if constexpr (WEIGHTED) wpre = (!is_long && begin + tl < end) ? weights[begin + tl] : 0.f;
                while (__any(i < end)) {  // wave-uniform; tiles whose bag is done idle through the ballots
                    uint64_t pos[U];
                    int64_t kv[U];
                    float wv[U];
                    bool inb[U];
    #pragma unroll
                    for (int u = 0; u < U; ++u) {
                        pos[u] = i + u; inb[u] = pos[u] < end;
                        kv[u] = __shfl(kpre, tile * 16 + (int)((pos[u] - begin) & 15));
                        if constexpr (WEIGHTED) wv[u] = __shfl(wpre, tile * 16 + (int)((pos[u] - begin) & 15));
                    }
                    pooled_fetch<DIM4, U, C, TAGGED, BROWS ? kRowsBF16 : kRowsF32>(tkeys, values, nb, dim4, kv, pos, inb, tile, tl, def4, row, found, (GROUPED && BROWS) ? nullptr : located,   // (a bf16-row group hands out no located rows: refused at the entry points)
                                                          member << kGroupSlotBits);
    #pragma unroll
                    for (int u = 0; u < U; ++u) {
                        if (!inb[u]) continue;
    #pragma unroll
                        for (int c = 0; c < C; ++c)
                            if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                                if constexpr (WEIGHTED) {   // (the unweighted instances keep their code exactly)
                                    float4 v = row[u][c];
                                    v.x = wv[u] * v.x; v.y = wv[u] * v.y; v.z = wv[u] * v.z; v.w = wv[u] * v.w;
                                    if (first) acc[c] = v;
                                    else { acc[c].x += v.x; acc[c].y += v.y; acc[c].z += v.z; acc[c].w += v.w; }
                                } else {
                                    if (first) acc[c] = row[u][c];
                                    else { acc[c].x += row[u][c].x; acc[c].y += row[u][c].y; acc[c].z += row[u][c].z; acc[c].w += row[u][c].w; }
                                }
                            }
                        first = false;
                    }
                    i += U;
                }
                if (has && !is_long) {
                    const float len = (float)(end - begin);
    #pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                            float4 v = acc[c];
                            if (mean && end > begin) { v.x = v.x / len; v.y = v.y / len; v.z = v.z / len; v.w = v.w / len; }
                            if constexpr (BF16) store_bf16x4<true>(out, row_of(bag) + c * 16 + tl, v); else out[row_of(bag) + c * 16 + tl] = v;
                        }
                }
            }
            // ---- long bags: the four tiles share one bag at a time ----
            const uint64_t long_mask = __ballot(is_long && has);
            if (!long_mask) continue;   // wave-uniform
            for (int q = 0; q < BPW; ++q) {
                if (!((long_mask >> (q * 16)) & 1)) continue;   // wave-uniform
                const uint64_t bq = __shfl(begin, q * 16), eq = __shfl(end, q * 16);
                if constexpr (JAGGED) (void)jagged_member(member_bags, n_members, b0 + q, member);   // (a long bag is not empty: it lies inside the map)
                else member = (b0 + q) / bags_per_table;
                d = desc[member];   // all four tiles work for bag q's table now
                tkeys = d.tkeys; values = d.values; nb = d.nb; def4 = make_float4(d.defv, d.defv, d.defv, d.defv);
                bool first = true;
    #pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = make_float4(0.f, 0.f, 0.f, 0.f);
                for (uint64_t i = bq; i < eq; i += 4 * U) {   // wave-uniform
                    uint64_t pos[U];
                    int64_t kv[U];
                    float wv[U];
                    bool inb[U];
    #pragma unroll
                    for (int u = 0; u < U; ++u) {
                        pos[u] = i + (uint64_t)u * 4 + tile; inb[u] = pos[u] < eq; kv[u] = inb[u] ? keys[pos[u]] : kEmpty;
                        if constexpr (WEIGHTED) wv[u] = inb[u] ? weights[pos[u]] : 0.f;   // next to the key
                    }
                    pooled_fetch<DIM4, U, C, TAGGED, BROWS ? kRowsBF16 : kRowsF32>(tkeys, values, nb, dim4, kv, pos, inb, tile, tl, def4, row, found, (GROUPED && BROWS) ? nullptr : located,   // (a bf16-row group hands out no located rows: refused at the entry points)
                                                          member << kGroupSlotBits);
    #pragma unroll
                    for (int u = 0; u < U; ++u)
    #pragma unroll
                        for (int src = 0; src < 4; ++src) {
                            if (i + (uint64_t)u * 4 + src >= eq) continue;   // wave-uniform
                            float w = 0.f;
                            if constexpr (WEIGHTED) w = __shfl(wv[u], src * 16 + tl);
    #pragma unroll
                            for (int c = 0; c < C; ++c) {
                                float4 v;   // every tile reads the row tile `src` fetched: all four keep the same running sum
                                v.x = __shfl(row[u][c].x, src * 16 + tl); v.y = __shfl(row[u][c].y, src * 16 + tl);
                                v.z = __shfl(row[u][c].z, src * 16 + tl); v.w = __shfl(row[u][c].w, src * 16 + tl);
                                if constexpr (WEIGHTED) { v.x = w * v.x; v.y = w * v.y; v.z = w * v.z; v.w = w * v.w; }
                                if (first) acc[c] = v;
                                else { acc[c].x += v.x; acc[c].y += v.y; acc[c].z += v.z; acc[c].w += v.w; }
                            }
                            first = false;
                        }
                }
                if (tile == 0) {
                    const float len = (float)(eq - bq);
    #pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) {
                            float4 v = acc[c];
                            if (mean && eq > bq) { v.x = v.x / len; v.y = v.y / len; v.z = v.z / len; v.w = v.w / len; }
                            if constexpr (BF16) store_bf16x4<true>(out, row_of(b0 + q) + c * 16 + tl, v); else out[row_of(b0 + q) + c * 16 + tl] = v;
                        }
                }
            }
        }
    }
}

// ---- backward of the weighted pooled lookup (SPEC.md §3) ------------------------------------------------------------------
// grads[i] = weights[i] * bag_grads[bag(i)] (one fp32 multiply per element) and, when weight_grads is given, weight_grads[i] =
// sum_j bag_grads[bag(i), j] * row_i[j] in fp64, rounded once.  The bag-to-wave geometry of the forward, from the same pieces (pooled_span,
// pooled_short_* and pooled_long_positions, meepo_device.h): a tile per short bag, the wave's four tiles on one long bag, or a wave per
// bag (BPW 1).  The bag's grad row is loaded into registers once.  Nothing here depends on the order of positions or is carried from
// round to round, so each round of positions goes straight to pooled_bwd_positions.

// the U positions one tile handles in one round: store w * G, then (weight_grads) fetch the rows and reduce the dot products across
// the tile's 16 lanes.  A row comes through its handle when the caller passed one (`handles`), otherwise from a probe (pooled_fetch);
// a handle of an absent key reads the default row, a handle the table cannot vouch for (another layout epoch, out of range, another
// member) falls back to the probe.
template <int DIM4, int U, int C, bool GROUPED>
__device__ __forceinline__ void pooled_bwd_positions(const PooledTable& t, uint64_t capacity, uint32_t dim4, const int64_t (&key)[U], const uint64_t (&pos)[U],
                                                     const bool (&inb)[U], const float (&w)[U], const int64_t* __restrict__ handles, int tile, int tl,
                                                     const float4 (&g)[C], float4* __restrict__ grads, float* __restrict__ weight_grads) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (!inb[u]) continue;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)
                grads[pos[u] * dim4 + c * 16 + tl] = make_float4(w[u] * g[c].x, w[u] * g[c].y, w[u] * g[c].z, w[u] * g[c].w);
    }
    if (!weight_grads) return;   // kernel-uniform: no table row is read
    bool probe[U];
    int64_t hs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        hs[u] = -1;
        probe[u] = inb[u];
        if (handles && inb[u]) {
            const int64_t h = handles[pos[u]];
            if (h < 0) probe[u] = false;   // absent when the forward ran: the default row
            else if constexpr (GROUPED) {
                const uint64_t s = (uint64_t)h & ((1ull << kGroupSlotBits) - 1);
                if (((uint64_t)h >> kGroupSlotBits) == (t.tag >> kGroupSlotBits) && s < capacity) { hs[u] = (int64_t)s; probe[u] = false; }
            } else {
                bool stale;
                hs[u] = handle_slot(h, (int64_t)t.tag, capacity, stale);
                probe[u] = hs[u] < 0;
            }
        }
    }
    float4 row[U][C];
    pooled_fetch<DIM4, U, C>(t.tkeys, t.values, t.nb, dim4, key, pos, probe, tile, tl, t.def4, row, nullptr);
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (hs[u] >= 0) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4) row[u][c] = t.values[(uint64_t)hs[u] * dim4 + c * 16 + tl];
        }
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (inb[u] && (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)) {
                s += (double)g[c].x * (double)row[u][c].x; s += (double)g[c].y * (double)row[u][c].y;
                s += (double)g[c].z * (double)row[u][c].z; s += (double)g[c].w * (double)row[u][c].w;
            }
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m);   // across the tile's 16 lanes
        if (inb[u] && tl == 0) weight_grads[pos[u]] = (float)s;
    }
}

template <int DIM4, int U, int BPW, bool GROUPED = false>
__global__ __launch_bounds__(256) void pooled_weighted_backward_kernel(const int64_t* __restrict__ tkeys_, const float4* __restrict__ values_,
                                                                       uint64_t nb_, uint64_t capacity_, const int64_t* __restrict__ keys,
                                                                       const int64_t* __restrict__ handles, int64_t handle_tag,
                                                                       const uint64_t* __restrict__ offsets, uint64_t n_bags,
                                                                       const float* __restrict__ weights, const float4* __restrict__ bag_grads,
                                                                       float4* __restrict__ grads, float* __restrict__ weight_grads, float defv,
                                                                       uint32_t dim4_rt, const GroupDesc* __restrict__ desc,
                                                                       uint64_t bags_per_table, uint64_t n_keys) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 16;
    auto table_of = [&](uint64_t b, PooledTable& t) {
        if constexpr (GROUPED) {
            t = pooled_table(desc[b / bags_per_table], b / bags_per_table, kGroupSlotBits);
        } else t = PooledTable{tkeys_, values_, nb_, make_float4(defv, defv, defv, defv), (uint64_t)handle_tag};
    };
    auto grad_row = [&](uint64_t b, bool live, float4 (&g)[C]) {   // the bag's grad row, once into registers
#pragma unroll
        for (int c = 0; c < C; ++c)
            g[c] = (live && (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)) ? bag_grads[b * dim4 + c * 16 + tl] : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    for (uint64_t b0 = wave * BPW; b0 < n_bags; b0 += n_waves * BPW) {
        const uint64_t bag = BPW == 4 ? b0 + tile : b0;
        const bool has = bag < n_bags;
        uint64_t begin, end;
        pooled_span(offsets, bag, has, n_keys, begin, end);
        PooledTable t;
        table_of(has ? bag : b0, t);
        const bool is_long = BPW == 1 || end - begin >= kPoolLong;
        float4 g[C];
        uint64_t pos[U];
        int64_t kv[U];
        float wv[U];
        bool inb[U];
        // ---- short bags: one tile per bag ----
        if constexpr (BPW == 4) {
            grad_row(bag, has && !is_long && end > begin, g);
            int64_t kpre;
            float wpre;
            pooled_short_prefetch<true>(keys, weights, begin, end, is_long, tl, kpre, wpre);
            for (uint64_t i = is_long ? end : begin; __any(i < end); i += U) {  // wave-uniform
                pooled_short_positions<U, true>(i, begin, end, kpre, wpre, tile, pos, kv, wv, inb);
                pooled_bwd_positions<DIM4, U, C, GROUPED>(t, GROUPED ? t.nb * kW : capacity_, dim4, kv, pos, inb, wv, handles, tile, tl, g, grads, weight_grads);
            }
        }
        // ---- long bags: the four tiles share one bag at a time ----
        const uint64_t long_mask = __ballot(is_long && has);
        if (!long_mask) continue;   // wave-uniform
        for (int q = 0; q < BPW; ++q) {
            if (!((long_mask >> (q * 16)) & 1)) continue;   // wave-uniform
            const uint64_t bq = __shfl(begin, q * 16), eq = __shfl(end, q * 16);
            if constexpr (BPW == 4) table_of(b0 + q, t);
            grad_row(b0 + q, true, g);
            for (uint64_t i = bq; i < eq; i += 4 * U) {   // wave-uniform
                pooled_long_positions<U, true>(i, eq, keys, weights, tile, pos, kv, wv, inb);
                pooled_bwd_positions<DIM4, U, C, GROUPED>(t, GROUPED ? t.nb * kW : capacity_, dim4, kv, pos, inb, wv, handles, tile, tl, g, grads, weight_grads);
            }
        }
    }
}

// One instance is created here, ahead of the launch function that creates the others: one bf16-row table, bf16 out, dim 64, four bags per wave.  The compiler's
// output for it depends on when it meets it (nothing else does: tools/kernel_code_hashes.py against the commit before the launches were unified); with it met
// first, every kernel of this file is that commit's, byte for byte, in both orders of pooled_find's arms that were tried (profiles/host_layer.md).
// The line serves that comparison alone — the instance is one the launch function reaches anyway, and its bytes still depend on the compiler's version: once
// byte-identity with that commit no longer matters it may be removed.
template __global__ void find_pooled_kernel<16, 2, 4, false, false, true, false, false, true, false>(const int64_t*, const float4*, uint64_t, const int64_t*, const uint64_t*, uint64_t, float4*, uint8_t*, float,
                                                                                                       uint32_t, int, const GroupDesc*, uint64_t, int64_t*, uint64_t, const float*, int64_t, const uint64_t*, uint32_t, TierArgs);
}  // namespace mee

using namespace mee;

namespace mee {
// The library's own store policy for a dense output (nobody gave a hint).  One call cannot tell whether its output will be re-read from cache; the last few calls
// can: a ring of the latest calls' output buffers (base address, bytes).  The same buffer as the call before: the caller reuses one result buffer — cached stores
// while it fits (<= 128 MB: the Infinity Cache absorbs it).  Another buffer, and the distinct buffers of the last eight calls add up to more than 64 MB: the results
// rotate (a server's independent requests, a trainer's per-step activations), every one of them has to reach HBM and nothing re-reads it from cache — streaming
// stores (measured into 6 x 64 MB buffers: 38.6 -> 33.2 us per 256K-key find; two alternating 64 MB buffers: 35.4 cached).  mee_find_ex / "find_nt" stay authoritative.
static bool outputs_rotate(const mee_table* t, const void* d_out, uint64_t bytes) {
    mee_table* m = const_cast<mee_table*>(t);   // (policy state only; see meepo_table_int.h)
    const uint64_t p = (uint64_t)(uintptr_t)d_out;
    const uint32_t head = __atomic_load_n(&m->out_ring_head, __ATOMIC_RELAXED);
    if (__atomic_load_n(&m->out_ring_ptr[(head + 7u) & 7u], __ATOMIC_RELAXED) == p) return false;
    const uint32_t slot = __atomic_fetch_add(&m->out_ring_head, 1u, __ATOMIC_RELAXED) & 7u;
    __atomic_store_n(&m->out_ring_ptr[slot], p, __ATOMIC_RELAXED);
    __atomic_store_n(&m->out_ring_bytes[slot], bytes, __ATOMIC_RELAXED);
    uint64_t seen[8], total = 0;
    int distinct = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t q = __atomic_load_n(&m->out_ring_ptr[i], __ATOMIC_RELAXED);
        if (!q) continue;
        bool dup = false;
        for (int j = 0; j < distinct; ++j) dup = dup || seen[j] == q;
        if (dup) continue;
        seen[distinct++] = q;
        total += __atomic_load_n(&m->out_ring_bytes[i], __ATOMIC_RELAXED);
    }
    return distinct >= 2 && total > (64ull << 20);
}

// ---- captured finds: consecutive lookups of one table share a kernel node ---------------------------------------------------------------
// A caller that records a queue of lookups into a hipGraph gets one kernel node per call, chained: each pays the per-launch floor (~4.6 us of a
// 31 us 256K-key find), because consecutive nodes of an in-order stream do not overlap.  Under capture nothing has run yet, so the library can see
// that a plain find's ONLY predecessor is its own earlier find of the same table, and serve both from that node: the node is a find_many_kernel
// launch, and the later call extends its request descriptor instead of adding a node (one hipGraphKernelNodeSetParams call: the same function, the
// by-value FindMany and the grid change).  The graph stays one linear chain with fewer, fatter nodes; what a replay leaves in memory is what the
// chained launches leave.  A call joins the node in front of it only when
//   - the stream's dependency set is exactly that node (nothing of ours or of anybody else's was captured in between, no fork or join),
//   - table, plane pointers, bucket count, default value, kernel instance (row shape, keys in flight, the call's policy bits) and block size agree,
//   - the descriptor has room and the request's buffers are disjoint from the node's (find_request_disjoint: chained launches that share a buffer
//     have a defined winner, requests inside one kernel do not).
// Otherwise the call starts the next node.  Any HIP error on the way: the call is launched the ordinary way and the capture is left alone from then on.
// Eager launches never come here.  Off: mee_set_tuning("find_coalesce", 0), or MEE_FIND_COALESCE=0 in the environment (read when the library loads).
// The two graph calls are weak references: a HIP runtime without them leaves every find a launch of its own.
#pragma weak hipStreamGetCaptureInfo_v2
#pragma weak hipGraphKernelNodeSetParams
static std::mutex g_find_nodes_mu;
static FindNodes g_find_nodes;   // (under g_find_nodes_mu)
static const bool g_find_coalesce_env = [] { const char* e = getenv("MEE_FIND_COALESCE"); return !(e && e[0] == '0'); }();

// the capturing stream's capture id and its dependency set when that is ONE node (else *dep = null); false: not capturing, or the query failed
static bool capture_state(hipStream_t st, unsigned long long* id, hipGraph_t* graph, hipGraphNode_t* dep) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const hipGraphNode_t* deps = nullptr;
    size_t n_deps = 0;
    *id = 0; *graph = nullptr; *dep = nullptr;
    if (hipStreamGetCaptureInfo_v2(st, &cs, id, graph, &deps, &n_deps) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (cs != hipStreamCaptureStatusActive || *id == 0) return false;
    if (n_deps == 1 && deps) *dep = deps[0];
    return true;
}

// One plain find of `n` keys on the capturing stream `st`, as `blocks` blocks of `block` threads of the find_many_kernel instance `func`.
// true: the request is in the graph (it joined the node in front of it, or got a node of its own).  false: the caller launches find_kernel.
static bool find_captured(const void* func, const mee_table* t, const float* plane, float defv, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found,
                          unsigned block, unsigned blocks, hipStream_t st) {
    mee_table* mt = const_cast<mee_table*>(t);   // (statistics only)
    auto own_node = [&](bool launched) { __atomic_fetch_add(&mt->find_nodes, 1ull, __ATOMIC_RELAXED); return launched; };
    if (!g_find_coalesce_env || !t->find_coalesce || !hipStreamGetCaptureInfo_v2 || !hipGraphKernelNodeSetParams) return own_node(false);
    unsigned long long id;
    hipGraph_t graph;
    hipGraphNode_t dep;
    if (!capture_state(st, &id, &graph, &dep)) return own_node(false);
    std::lock_guard<std::mutex> lk(g_find_nodes_mu);
    FindNode* r = g_find_nodes.get(id);
    if (r && r->off) return own_node(false);
    const int64_t* tkeys = t->keys;
    const f32x4* values = (const f32x4*)plane;
    uint64_t nb = t->nb;
    uint32_t dim4 = t->dim4, defv_bits;
    memcpy(&defv_bits, &defv, 4);
    FindMany m;
    void* args[6] = {&tkeys, &values, &nb, &m, &defv, &dim4};   // find_many_kernel's parameters, in order
    if (r && r->node && dep == r->node && graph == r->graph && func == r->func && t == r->table && tkeys == r->tkeys && values == r->values && nb == r->nb &&
        defv_bits == r->defv_bits && dim4 == r->dim4 && block == r->block) {
        m = r->m;
        if (find_request_disjoint(m, (uint64_t)t->dim * 4, d_keys, n, d_out, d_found) && find_many_append(m, d_keys, n, (f32x4*)d_out, d_found, blocks)) {
            hipKernelNodeParams p;   // built completely before the one call that edits the node
            memset(&p, 0, sizeof p);
            p.func = const_cast<void*>(func);
            p.gridDim = dim3(m.first_block[m.count]);
            p.blockDim = dim3(block);
            p.kernelParams = args;
            if (hipGraphKernelNodeSetParams((hipGraphNode_t)r->node, &p) == hipSuccess) {
                r->m = m;
                __atomic_fetch_add(&mt->find_merged, 1ull, __ATOMIC_RELAXED);
                return true;
            }
            (void)hipGetLastError();   // the node is as it was: this capture's finds are launches of their own from here on
            r->off = true;
            return own_node(false);
        }
    }
    m = FindMany{};
    (void)find_many_append(m, d_keys, n, (f32x4*)d_out, d_found, blocks);   // (n > 0 and 1 <= blocks <= 2^22: find_plane)
    FindNode& e = g_find_nodes.put(id);
    e.node = nullptr;   // whatever it named is no longer the stream's latest node
    if (hipLaunchKernel(func, dim3(blocks), dim3(block), args, 0, st) != hipSuccess) {
        (void)hipGetLastError();
        e.off = true;
        return own_node(false);
    }
    unsigned long long id2;
    if (capture_state(st, &id2, &graph, &dep) && id2 == id && dep) {
        e.graph = graph; e.node = dep; e.func = func; e.table = t; e.tkeys = tkeys; e.values = values; e.nb = nb;
        e.defv_bits = defv_bits; e.dim4 = dim4; e.block = block; e.m = m;
    }
    return own_node(true);
}

// every dense lookup of one plane (declared with FindPath in meepo_table_int.h: find_or_insert's first pass calls it too)
int find_plane(const mee_table* t, const float* plane, float miss_value, const int64_t* d_keys, size_t n, float* d_out,
               uint8_t* d_found, void* stream, FindPath path) {
    if (n == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    const unsigned fblock = t->find_block == 64 || t->find_block == 128 ? (unsigned)t->find_block : 256u;   // (launch bound of find_kernel: 256)
    const bool bf16 = path.out_dtype == MEE_DTYPE_BF16;   // d_out holds bf16 rows (Plain, Located and SkipPadding only: the entry points see to that)
    const uint64_t out_bytes = (uint64_t)n * t->dim * (bf16 ? 2 : 4);   // what the call really writes
    const int nt = path.nt >= 0 ? path.nt : t->find_nt >= 0 ? (t->find_nt & kFindHintBits)
                 : (out_bytes <= kCachedOutputBytes && !outputs_rotate(t, d_out, out_bytes) ? kFindCachedStores : 0);
    const bool located_cached = t->find_nt >= 0 && (t->find_nt & kFindCachedStores);   // the located find streams its output unless "find_nt" asks otherwise (below)
    if (path.kind == FindPath::Missing || path.kind == FindPath::CountedMissing) {
        with_value<3, 1>(path.kind == FindPath::CountedMissing ? 3 : 1, [&](auto flags) {
            find_missing_kernel<flags><<<grid_for(n, 256, 8192), 256, 0, st>>>(t->keys, (const float4*)plane, t->nb, t->dim4, d_keys, n, (float4*)d_out, d_found, t->hits);
        });
    } else if (t->bf16_rows || t->int8_rows) with_row_shape(t->dim4, [&](auto d4) {
        // a bf16-ROW or int8-ROW table (Plain only: the entry points see to that): find_span's kRowsBF16 / kRowsI8 instances, per row shape at its default keys
        // in flight, fp32 or bf16 out
        constexpr int D4 = d4;
        constexpr int R = RowShape<D4>::rows_per_tile;
        const unsigned grid = grid_for(n, (fblock / 64u) * 4u * (unsigned)R, t->find_grid_cap > 0 ? (unsigned)t->find_grid_cap : (1u << 22));
        with_flag(t->int8_rows, [&](auto i8) { with_flag(bf16, [&](auto b16) { with_value<0, 1, 2, 3, 4, 5, 6, 7>(nt, [&](auto ntc) {
            find_kernel<D4, R, (decltype(b16)::value ? kFindBF16Out : 0) | decltype(ntc)::value, decltype(i8)::value ? kRowsI8 : kRowsBF16><<<grid, fblock, 0, st>>>(t->keys, (const f32x4*)plane, t->nb, d_keys, n, (f32x4*)d_out, d_found, miss_value, t->dim4, nullptr, nullptr, 0);
        }); }); });
    });
    else if (bf16) with_row_shape(t->dim4, [&](auto d4) {
        // bf16 out: the same kernel with kFindBF16Out, instantiated for each row shape's default keys in flight only ("find_rounds" does not apply)
        constexpr int D4 = d4;
        constexpr int R = RowShape<D4>::rows_per_tile;
        const unsigned grid = grid_for(n, (fblock / 64u) * 4u * (unsigned)R, t->find_grid_cap > 0 ? (unsigned)t->find_grid_cap : (1u << 22));
        auto find = [&](auto ntc, int64_t* slots_out, int64_t tag) {
            find_kernel<D4, R, kFindBF16Out | ntc><<<grid, fblock, 0, st>>>(t->keys, (const f32x4*)plane, t->nb, d_keys, n, (f32x4*)d_out, d_found, miss_value, t->dim4, nullptr, slots_out, tag);
        };
        if (path.kind == FindPath::Located) {   // (the store policy of the fp32 located find)
            with_value<kFindLocated | kFindCachedStores, kFindLocated>(located_cached ? kFindLocated | kFindCachedStores : kFindLocated, [&](auto ntc) { find(ntc, path.slots_out, handle_tag_of(t)); });
        } else if (path.kind == FindPath::SkipPadding) {   // owner pass of a padded sharded exchange whose rows travel as bf16 (the fp32 one's store policy)
            with_value<kFindSkipPadding | kFindCachedStores, kFindSkipPadding>(kFindSkipPadding | (nt & kFindCachedStores), [&](auto ntc) { find(ntc, nullptr, 0); });
        } else {
            with_value<0, 1, 2, 3, 4, 5, 6, 7>(nt, [&](auto ntc) { find(ntc, nullptr, 0); });
        }
    });
    else with_row_shape(t->dim4, [&](auto d4) {
        constexpr int D4 = d4;
        int R = t->find_rounds > 0 ? t->find_rounds : RowShape<D4>::rows_per_tile;
        if (D4 != 16 && R > 4) R = 4;
        if (D4 != 16 && D4 != 32 && R > 2) R = 2;
        R = R >= 8 ? 8 : R >= 4 ? 4 : R >= 2 ? 2 : 1;
        const unsigned grid = grid_for(n, (fblock / 64u) * 4u * (unsigned)R, t->find_grid_cap > 0 ? (unsigned)t->find_grid_cap : (1u << 22));
        auto find = [&](auto rr, auto ntc, unsigned grid_x, unsigned block, uint32_t* hits = nullptr, int64_t* slots_out = nullptr, int64_t tag = 0) {
            find_kernel<D4, rr, ntc><<<grid_x, block, 0, st>>>(t->keys, (const f32x4*)plane, t->nb, d_keys, n, (f32x4*)d_out, d_found, miss_value, t->dim4, hits, slots_out, tag);
        };
        if (path.kind == FindPath::SkipPadding) {   // owner pass of a padded sharded exchange: EMPTY positions get neither a row nor a found byte (nobody reads them)
            with_value<2, 1>(R >= 2 ? 2 : 1, [&](auto rr) { with_value<kFindSkipPadding | kFindCachedStores, kFindSkipPadding>(kFindSkipPadding | (nt & kFindCachedStores), [&](auto ntc) { find(rr, ntc, grid, 256); }); });
        } else if (path.kind == FindPath::Located) {   // located find: the plain kernel + one 8-byte store per key
            // cache policy of `out`: this is the forward of a TRAINING step — the apply that follows sweeps the Infinity Cache before the next
            // forward, so keeping the dense output cached buys nothing and streaming stores win (136.9 -> 132.5 us per find + Adagrad step)
            with_value<2, 1>(R >= 2 ? 2 : 1, [&](auto rr) { with_value<kFindLocated | kFindCachedStores, kFindLocated>(located_cached ? kFindLocated | kFindCachedStores : kFindLocated, [&](auto ntc) { find(rr, ntc, grid, fblock, nullptr, path.slots_out, handle_tag_of(t)); }); });
        } else if (path.kind == FindPath::Counted) {   // sampled statistics pass: one key in flight per tile
            find(std::integral_constant<int, 1>{}, std::integral_constant<int, kFindCountHits | kFindCachedStores>{}, grid_for(n, 16, 1u << 22), 256, t->hits);
        } else {
            // under stream capture a plain find joins the find node in front of it, or starts the next one (find_captured above); eager launches stay find_kernel's
            const bool captured = path.kind == FindPath::Plain && stream_is_capturing(st);
            auto plain = [&](auto rr) { with_value<0, 1, 2, 3, 4, 5, 6, 7>(nt, [&](auto ntc) {
                if (path.kind == FindPath::Unordered)   // (any block order, at find_kernel's launch bound; the launch takes the parameters' exact types)
                    hipExtLaunchKernelGGL((find_kernel<D4, rr, ntc>), dim3(grid), dim3(256), 0, st, nullptr, nullptr, hipExtAnyOrderLaunch, (const int64_t*)t->keys,
                                          (const f32x4*)plane, t->nb, d_keys, (uint64_t)n, (f32x4*)d_out, d_found, miss_value, t->dim4, (uint32_t*)nullptr, (int64_t*)nullptr, (int64_t)0);
                else if (!captured || !find_captured((const void*)&find_many_kernel<D4, rr, ntc>, t, plane, miss_value, d_keys, n, d_out, d_found, fblock, grid, st))
                    find(rr, ntc, grid, fblock);
            }); };
            if constexpr (D4 == 16) with_value<8, 4, 2, 1>(R, plain);
            else if constexpr (D4 == 32) with_value<4, 2, 1>(R, plain);
            else with_value<2, 1>(R, plain);
        }
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // namespace mee
extern "C" {

// mee_find_ex / mee_find_as: the call's hints become the kernel's policy bits; the output's size is counted in its own element type
static int find_hinted(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint8_t* d_found, uint32_t flags, uint32_t out_dtype, void* stream,
                       const char* name) {
    if (!t || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (flags & ~(uint32_t)(MEE_FIND_STREAM_STORES | MEE_FIND_CACHED_STORES | MEE_FIND_STREAM_ROWS | MEE_FIND_STREAM_BUCKETS))
        return fail(MEE_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", name, flags);
    if ((flags & MEE_FIND_STREAM_STORES) && (flags & MEE_FIND_CACHED_STORES))
        return fail(MEE_ERR_INVALID_ARG, "%s: MEE_FIND_STREAM_STORES and MEE_FIND_CACHED_STORES exclude each other", name);
    if (flags == MEE_FIND_DEFAULT) return find_plane(t, t->values, t->default_value, d_keys, n, (float*)d_out, d_found, stream, {FindPath::Plain, nullptr, -1, out_dtype});
    const uint64_t out_bytes = (uint64_t)n * t->dim * (out_dtype == MEE_DTYPE_BF16 ? 2 : 4);
    const bool cached_out = (flags & MEE_FIND_CACHED_STORES) ||
                            (!(flags & MEE_FIND_STREAM_STORES) && out_bytes <= kCachedOutputBytes && !outputs_rotate(t, d_out, out_bytes));
    const int nt = (flags & MEE_FIND_STREAM_ROWS ? kFindStreamRows : 0) | (flags & MEE_FIND_STREAM_BUCKETS ? kFindStreamBuckets : 0) | (cached_out ? kFindCachedStores : 0);
    return find_plane(t, t->values, t->default_value, d_keys, n, (float*)d_out, d_found, stream, {FindPath::Plain, nullptr, nt, out_dtype});
}

int mee_find(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream) {
    MEE_RANGE("mee_find");
    if (!t || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "mee_find: null argument");
    return find_plane(t, t->values, t->default_value, d_keys, n, d_out, d_found, stream);
}

int mee_find_ex(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, uint32_t flags, void* stream) {
    MEE_RANGE("mee_find_ex");
    return find_hinted(t, d_keys, n, d_out, d_found, flags, MEE_DTYPE_F32, stream, "mee_find_ex");
}

int mee_find_as(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, uint32_t flags, void* stream) {
    MEE_RANGE("mee_find_as");
    return find_hinted(t, d_keys, n, d_out, d_found, flags, out_dtype, stream, "mee_find_as");
}

}  // extern "C"
namespace mee {
// mee_find for the owner side of a padded sharded exchange (meepo_sharded.hip): MEE_EMPTY_KEY positions are padding that nobody reads —
// they get neither a default row nor a found byte.  out_dtype = MEE_DTYPE_BF16: d_out holds bf16 rows (the rows of a bf16 sharded lookup are
// rounded here, on the owner, before they travel)
int find_skip_padding(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint8_t* d_found, void* stream, uint32_t out_dtype) {
    if (!t || (n && (!d_keys || !d_out || !d_found))) return fail(MEE_ERR_INVALID_ARG, "find_skip_padding: null argument");
    if (int rc = check_out_dtype(d_out, out_dtype, "find_skip_padding")) return rc;
    return find_plane(t, t->values, t->default_value, d_keys, n, (float*)d_out, d_found, stream, {FindPath::SkipPadding, nullptr, -1, out_dtype});
}
}  // namespace mee
extern "C" {

int mee_find_located(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream) {
    MEE_RANGE("mee_find_located");
    MEE_FP32_ROWS_ONLY(t, "mee_find_located");
    if (!t || (n && (!d_keys || !d_out || !d_slots_out))) return fail(MEE_ERR_INVALID_ARG, "mee_find_located: null argument");
    return find_plane(t, t->values, t->default_value, d_keys, n, d_out, d_found, stream, {FindPath::Located, d_slots_out});
}
int mee_find_located_as(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out, void* stream) {
    MEE_RANGE("mee_find_located_as");
    MEE_FP32_ROWS_ONLY(t, "mee_find_located_as");
    if (!t || (n && (!d_keys || !d_out || !d_slots_out))) return fail(MEE_ERR_INVALID_ARG, "mee_find_located_as: null argument");
    if (int rc = check_out_dtype(d_out, out_dtype, "mee_find_located_as")) return rc;
    return find_plane(t, t->values, t->default_value, d_keys, n, (float*)d_out, d_found, stream, {FindPath::Located, d_slots_out, -1, out_dtype});
}

int mee_find_many(const mee_table* t, const mee_find_request* reqs, uint32_t count, void* stream) {
    MEE_RANGE("mee_find_many");
    MEE_FP32_ROWS_ONLY(t, "mee_find_many");
    if (!t || !reqs) return fail(MEE_ERR_INVALID_ARG, "mee_find_many: null argument");
    if (count == 0) return MEE_OK;
    if (count > (uint32_t)kMaxFindRequests) return fail(MEE_ERR_INVALID_ARG, "mee_find_many: %u requests (at most %d per call)", count, kMaxFindRequests);
    FindMany m{};
    const int R = with_row_shape(t->dim4, [](auto d4) { return RowShape<d4>::rows_per_tile; });
    uint64_t blocks = 0, out_bytes = 0;
    for (uint32_t q = 0; q < count; ++q) {
        if (reqs[q].n == 0) continue;
        if (!reqs[q].d_keys || !reqs[q].d_out) return fail(MEE_ERR_INVALID_ARG, "mee_find_many: request %u has a null buffer", q);
        const uint64_t req_blocks = (reqs[q].n + 16ull * R - 1) / (16ull * R);
        blocks += req_blocks;
        if (req_blocks >= (1ull << 31) || !find_many_append(m, reqs[q].d_keys, reqs[q].n, (f32x4*)reqs[q].d_out, reqs[q].d_found, (uint32_t)req_blocks))
            return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_find_many: %llu blocks", (unsigned long long)blocks);
        out_bytes += (uint64_t)reqs[q].n * t->dim * 4;
    }
    if (m.count == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    const bool cached_out = out_bytes <= kCachedOutputBytes;   // same policy as mee_find, on the total output of the launch
    with_row_shape(t->dim4, [&](auto d4) { with_value<kFindCachedStores, 0>(cached_out ? kFindCachedStores : 0, [&](auto ntc) {
        find_many_kernel<d4, RowShape<d4>::rows_per_tile, ntc><<<(unsigned)blocks, 256, 0, st>>>(t->keys, (const f32x4*)t->values, t->nb, m, t->default_value, t->dim4);
    }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_find_capture_stats(const mee_table* t, uint64_t* nodes, uint64_t* merged) {
    if (!t || !nodes || !merged) return fail(MEE_ERR_INVALID_ARG, "mee_find_capture_stats: null argument");
    *nodes = __atomic_load_n(&t->find_nodes, __ATOMIC_RELAXED);
    *merged = __atomic_load_n(&t->find_merged, __ATOMIC_RELAXED);
    return MEE_OK;
}

int mee_find_unordered(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream) {
    MEE_RANGE("mee_find_unordered");
    MEE_FP32_ROWS_ONLY(t, "mee_find_unordered");
    if (!t || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "mee_find_unordered: null argument");
    return find_plane(t, t->values, t->default_value, d_keys, n, d_out, d_found, stream, {FindPath::Unordered});
}

int mee_find_missing(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream) {
    MEE_RANGE("mee_find_missing");
    MEE_FP32_ROWS_ONLY(t, "mee_find_missing");
    if (!t || (n && (!d_keys || !d_out || !d_found))) return fail(MEE_ERR_INVALID_ARG, "mee_find_missing: null argument");
    return find_plane(t, t->values, t->default_value, d_keys, n, d_out, d_found, stream, {FindPath::Missing});
}

int mee_find_counted(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int missing_only, void* stream) {
    MEE_RANGE("mee_find_counted");
    MEE_FP32_ROWS_ONLY(t, "mee_find_counted");
    if (!t || (n && (!d_keys || !d_out || !d_found))) return fail(MEE_ERR_INVALID_ARG, "mee_find_counted: null argument");
    if (!t->hits) return fail(MEE_ERR_UNSUPPORTED, "mee_find_counted: table was created without MEE_FLAG_TRACK_HITS");
    return find_plane(t, t->values, t->default_value, d_keys, n, d_out, d_found, stream, {missing_only ? FindPath::CountedMissing : FindPath::Counted});
}

}  // extern "C"

// What every keyed entry point checks about its output before anything is launched or written; -> the row stride in element groups.
// width = the elements a row holds (T * dim, a mixed group's sum of dims); out_row_stride in elements, 0 = width.
int mee::keyed_out_check(const char* name, uint64_t width, uint64_t n_tables, uint64_t bags_per_table, const void* d_out, uint32_t out_dtype,
                         uint64_t out_row_stride, bool want_index, uint64_t* stride4) {
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (out_dtype == MEE_DTYPE_F32 && ((uintptr_t)d_out & 15)) return fail(MEE_ERR_INVALID_ARG, "%s: an fp32 keyed output must be 16-byte aligned", name);
    const uint64_t stride = out_row_stride ? out_row_stride : width;
    if (stride < width || (stride & 3))
        return fail(MEE_ERR_INVALID_ARG, "%s: out_row_stride = %llu elements must be a multiple of 4 and at least the row's width %llu", name,
                    (unsigned long long)stride, (unsigned long long)width);
    if (want_index && (bags_per_table > 0xFFFFFFFFull || n_tables * bags_per_table >= (1ull << 32)))
        return fail(MEE_ERR_INVALID_ARG, "%s: the step index is 32 bits: n_tables * bags_per_table must stay below 2^32", name);
    *stride4 = stride / 4;
    return MEE_OK;
}

// ---- the pooled lookups: one table, a hot/cold pair, a group, a group of pairs — every form is a PooledCall (meepo_table_int.h) ----------------------
// What every form refuses, once, in the order the entry points always had: null arguments, the pair's or the two groups' mismatches, out_dtype, mode,
// weights with MEAN, a single table's located rows without weights, the keyed output's shape (-> stride4).
static int pooled_check(const PooledCall& c, uint64_t* stride4) {
    const char* name = c.name;
    const bool grouped = c.source == PooledCall::Group || c.source == PooledCall::GroupOfPairs;
    const bool null_source = grouped ? !c.group || (c.source == PooledCall::GroupOfPairs && !c.cold_group) : !c.table || (c.source == PooledCall::Pair && !c.cold);
    if (null_source || (c.bags && (!c.offsets || !c.out || (c.jagged && !c.member_bags))) || (c.n && !c.keys)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (c.source == PooledCall::Pair) {
        const mee_table *hot = c.table, *cold = c.cold;
        if (hot == cold) return fail(MEE_ERR_INVALID_ARG, "%s: hot and cold are the same table (a key lives in exactly one tier)", name);
        if (hot->device != cold->device || hot->dim != cold->dim)
            return fail(MEE_ERR_INVALID_ARG, "%s: the tiers differ in device (%d, %d) or dim (%u, %u)", name, hot->device, cold->device, hot->dim, cold->dim);
        if (c.tier_flags & ~(uint32_t)(MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT)) return fail(MEE_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", name, c.tier_flags);
        if (((c.tier_flags & MEE_TIER_COUNT_COLD) && !cold->hits) || ((c.tier_flags & MEE_TIER_COUNT_HOT) && !hot->hits))
            return fail(MEE_ERR_INVALID_ARG, "%s: a count flag needs that tier created with MEE_FLAG_TRACK_HITS", name);
    }
    if (c.source == PooledCall::GroupOfPairs) { if (int rc = tiered_groups_check(c.group, c.cold_group, c.tier_flags, name)) return rc; }
    if (!c.keyed) { if (int rc = check_out_dtype(c.out, c.out_dtype, name)) return rc; }   // (keyed: keyed_out_check's, behind the mode)
    if (c.mode != MEE_POOL_SUM && c.mode != MEE_POOL_MEAN) return fail(MEE_ERR_INVALID_ARG, "%s: mode must be MEE_POOL_SUM or MEE_POOL_MEAN", name);
    if (c.weights && c.mode != MEE_POOL_SUM) return fail(MEE_ERR_INVALID_ARG, "%s: weighted pooling is MEE_POOL_SUM only", name);
    if (!grouped && c.located && !c.weights) return fail(MEE_ERR_INVALID_ARG, "%s: d_located_out is the weighted form's output (pass weights of 1.0f for a plain sum)", name);
    if (c.keyed) {
        if (int rc = keyed_out_check(name, (uint64_t)c.group->n_tables * c.group->dim4 * 4, c.group->n_tables, c.bags, c.out, c.out_dtype, c.out_row_stride, c.step_index != nullptr, stride4)) return rc;
    }
    const bool tiered = c.source == PooledCall::Pair || c.source == PooledCall::GroupOfPairs;
    if ((!grouped && (c.jagged || c.keyed)) || (c.jagged && (c.keyed || c.out_dtype != MEE_DTYPE_F32)) ||
        (c.weights && (c.jagged || c.keyed || tiered || (grouped ? c.group->bf16_rows : c.table->bf16_rows))))
        return fail(MEE_ERR_UNSUPPORTED, "%s: no pooled kernel serves this combination of source, weights, jagged map, keyed output and out_dtype", name);   // (no entry point asks for one)
    if (c.jagged && c.group->n_tables == 0) return fail(MEE_ERR_INVALID_ARG, "%s: the group has no tables", name);   // the kernel keeps the member inside [0, n_tables)
    return MEE_OK;
}

// The one launch of find_pooled_kernel.  Its instances are those the forms reach and no others: a table or a group (fp32 rows: weighted or not; bf16 rows:
// unweighted), a group's jagged map (fp32 out; either row type; pairs too), a pair or a group of pairs (fp32 rows, unweighted), a group's or a group of
// pairs' keyed output.  Kernel arguments a form has no use for keep the values the kernel ignores (null, 0, one bag per table).
int mee::pooled_find(const PooledCall& c) {
    uint64_t stride4 = 0;
    if (int rc = pooled_check(c, &stride4)) return rc;
    if (c.bags == 0) return MEE_OK;
    mee_group* const g = c.group;
    const mee_table* const t = c.table;
    if (g) { if (int rc = group_refresh(g, c.stream)) return rc; }
    if (c.cold_group) { if (int rc = group_refresh(c.cold_group, c.stream)) return rc; }
    DeviceGuard guard(g ? g->device : t->device);
    hipStream_t st = as_stream(c.stream);
    const bool tiered = c.source == PooledCall::Pair || c.source == PooledCall::GroupOfPairs;
    const uint32_t dim4 = g ? g->dim4 : t->dim4;
    const uint64_t per_table = g && !c.jagged ? c.bags : 1;
    const uint64_t n_bags = g && !c.jagged ? (uint64_t)g->n_tables * c.bags : c.bags;
    int64_t* const located = !g && !c.weights ? nullptr : c.located;             // a table's located rows are the weighted instances' ...
    const int64_t tag = !g && c.weights ? handle_tag_of(t) : 0;                   // ... in the format of mee_find_located
    const bool brows_rt = g ? g->bf16_rows : t->bf16_rows;
    const TierArgs pair_tier = c.cold ? TierArgs{c.cold->keys, (const float4*)c.cold->values, c.cold->nb, (c.tier_flags & MEE_TIER_COUNT_HOT) ? t->hits : nullptr,
                                                 (c.tier_flags & MEE_TIER_COUNT_COLD) ? c.cold->hits : nullptr} : TierArgs{};
    const GroupTier group_tier = c.cold_group ? GroupTier{c.cold_group->d_desc, g->d_init, c.cold_group->d_init, c.tier_flags} : GroupTier{};
    const KeyedOut keyed{stride4, c.step_index, c.index_by_bag || !g ? 1ull : g->n_tables, c.index_by_bag ? (uint64_t)c.bags : 1ull};
    with_pooled_shape(dim4, c.n, n_bags, [&](auto d4, auto u, auto bpw, unsigned grid) {
        // the kernel's arguments, once; `last` is the TierArgs | GroupTier | WithKeyed<> of either the instance takes
        auto launch = [&](auto kernel, auto last) {
            kernel<<<grid, 256, 0, st>>>(t ? t->keys : nullptr, t ? (const float4*)t->values : nullptr, t ? t->nb : 0, c.keys, c.offsets, n_bags, (float4*)c.out, c.found,
                                         t ? t->default_value : 0.f, dim4, c.mode == MEE_POOL_MEAN, g ? g->d_desc : nullptr, per_table, located, c.n, c.weights, tag,
                                         c.member_bags, c.jagged ? g->n_tables : 0, last);
        };
        // the tiered forms, a wave per bag at dim 64: two keys in flight per tile — 66 VGPRs / 7 waves where the one-table kernel's four take 93 / 5 here, at the same
        // measured time (profiles/tiered_bags.md); four measured no better for a group of pairs either (profiles/tiered_groups.md)
        constexpr int ut = (bpw == 1 && u > 2) ? 2 : u;
        // one arm per form, each naming its instances; pooled_check has refused every combination of fields that has no arm
        const bool bf16_out = c.out_dtype == MEE_DTYPE_BF16;
        auto plain = [&](auto grouped) { with_flag(c.weights != nullptr, [&](auto weighted) { with_flag(bf16_out, [&](auto bf16) {
            if constexpr (!weighted) { if (brows_rt) { launch(find_pooled_kernel<d4, u, bpw, grouped, false, bf16, false, false, true>, TierArgs{}); return; } }
            launch(find_pooled_kernel<d4, u, bpw, grouped, weighted, bf16>, TierArgs{});
        }); }); };
        const bool is_plain = !c.jagged && !c.keyed;
        if (!g && !tiered) plain(std::false_type{});
        else if (!g) with_flag(bf16_out, [&](auto bf16) { launch(find_pooled_kernel<d4, ut, bpw, false, false, bf16, false, true>, pair_tier); });
        else if (!tiered && is_plain) plain(std::true_type{});
        else if (!tiered && c.jagged) with_flag(brows_rt, [&](auto brows) { launch(find_pooled_kernel<d4, u, bpw, true, false, false, true, false, brows>, TierArgs{}); });
        else if (tiered && is_plain) with_flag(bf16_out, [&](auto bf16) { launch(find_pooled_kernel<d4, ut, bpw, true, false, bf16, false, true>, group_tier); });
        else if (tiered && c.jagged) launch(find_pooled_kernel<d4, ut, bpw, true, false, false, true, true>, group_tier);
        else if (!tiered) with_flag(bf16_out, [&](auto bf16) { with_flag(brows_rt, [&](auto brows) {
            launch(find_pooled_kernel<d4, u, bpw, true, false, bf16, false, false, brows, true>, WithKeyed<TierArgs>{{}, keyed}); }); });
        else with_flag(bf16_out, [&](auto bf16) { launch(find_pooled_kernel<d4, ut, bpw, true, false, bf16, false, true, false, true>, WithKeyed<GroupTier>{group_tier, keyed}); });
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// the fields every entry point of the family has
static PooledCall pooled_call(const char* name, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                              int mode, void* stream) {
    PooledCall c{name};
    c.keys = d_keys; c.n = n; c.offsets = d_bag_offsets; c.bags = bags; c.out = d_out; c.out_dtype = out_dtype; c.found = d_found; c.mode = mode; c.stream = stream;
    return c;
}

extern "C" {

int mee_find_pooled(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, float* d_out,
                    uint8_t* d_found, int mode, void* stream) {
    MEE_RANGE("mee_find_pooled");
    MEE_NO_INT8_ROWS(t, "mee_find_pooled");   // (an int8-row table has no pooled lookup yet)
    return pooled_find(pooled_call("mee_find_pooled", d_keys, n, d_bag_offsets, n_bags, d_out, MEE_DTYPE_F32, d_found, mode, stream).of(t));
}

int mee_find_pooled_weighted(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                             const float* d_weights, float* d_out, uint8_t* d_found, int64_t* d_located_out, void* stream) {
    MEE_RANGE("mee_find_pooled_weighted");
    MEE_FP32_ROWS_ONLY(t, "mee_find_pooled_weighted");
    if (n && !d_weights) return fail(MEE_ERR_INVALID_ARG, "mee_find_pooled_weighted: null argument");
    PooledCall c = pooled_call("mee_find_pooled_weighted", d_keys, n, d_bag_offsets, n_bags, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, stream).of(t);
    c.weights = d_weights;   // null only with n = 0: every bag is empty, the plain sum's zeros (and nothing is located)
    c.located = d_weights ? d_located_out : nullptr;
    return pooled_find(c);
}

int mee_find_pooled_as(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const float* d_weights,
                       void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream) {
    MEE_RANGE("mee_find_pooled_as");
    if (d_weights) MEE_FP32_ROWS_ONLY(t, "mee_find_pooled_as");
    MEE_NO_INT8_ROWS(t, "mee_find_pooled_as");
    PooledCall c = pooled_call("mee_find_pooled_as", d_keys, n, d_bag_offsets, n_bags, d_out, out_dtype, d_found, mode, stream).of(t);
    c.weights = d_weights;
    c.located = d_located_out;
    return pooled_find(c);
}

// the pooled lookup of a hot/cold pair: find_pooled_kernel's TIERED instances, the hot table in the table arguments, the cold one in TierArgs
int mee_find_pooled_tiered(const mee_table* hot, const mee_table* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                           void* d_out, uint32_t out_dtype, uint8_t* d_found, int mode, uint32_t flags, void* stream) {
    MEE_RANGE("mee_find_pooled_tiered");
    MEE_FP32_ROWS_ONLY(hot, "mee_find_pooled_tiered");
    MEE_FP32_ROWS_ONLY(cold, "mee_find_pooled_tiered");
    PooledCall c = pooled_call("mee_find_pooled_tiered", d_keys, n, d_bag_offsets, n_bags, d_out, out_dtype, d_found, mode, stream).of(hot, cold);
    c.tier_flags = flags;
    return pooled_find(c);
}

int mee_pooled_weighted_backward(const mee_table* t, const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets,
                                 size_t n_bags, const float* d_weights, const float* d_bag_grads, float* d_grads_out, float* d_weight_grads_out,
                                 void* stream) {
    MEE_RANGE("mee_pooled_weighted_backward");
    MEE_FP32_ROWS_ONLY(t, "mee_pooled_weighted_backward");
    if (!t || (n_bags && (!d_bag_offsets || !d_bag_grads)) || (n && (!d_keys || !d_weights || !d_grads_out)))
        return fail(MEE_ERR_INVALID_ARG, "mee_pooled_weighted_backward: null argument");
    if (n_bags == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    with_pooled_shape(t->dim4, n, n_bags, [&](auto d4, auto u, auto bpw, unsigned grid) {
        pooled_weighted_backward_kernel<d4, u, bpw><<<grid, 256, 0, st>>>(t->keys, (const float4*)t->values, t->nb, t->capacity, d_keys, d_located, handle_tag_of(t), d_bag_offsets,
                                                                          n_bags, d_weights, (const float4*)d_bag_grads, (float4*)d_grads_out, d_weight_grads_out, t->default_value, t->dim4, nullptr, 1, n);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_find_plane(const mee_table* t, uint32_t plane, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream) {
    MEE_RANGE("mee_find_plane");
    MEE_FP32_ROWS_ONLY(t, "mee_find_plane");
    if (!t || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "mee_find_plane: null argument");
    const float* p = plane_of(t, plane);
    if (!p) return fail(MEE_ERR_UNSUPPORTED, "mee_find_plane: plane %u does not exist (optimizer=%u)", plane, t->optimizer);
    return find_plane(t, p, plane == 0 ? t->default_value : 0.0f, d_keys, n, d_out, d_found, stream);
}

// ---- the embedding-bag collection: pooled lookups of a whole group in one launch, and their backward -----------------------
int mee_group_find_pooled(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                          float* d_out, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream) {
    MEE_RANGE("mee_group_find_pooled");
    if (d_located_out) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled", "d_located_out (the located rows serve the backward) is");
    PooledCall c = pooled_call("mee_group_find_pooled", d_keys, n, d_bag_offsets, bags_per_table, d_out, MEE_DTYPE_F32, d_found, mode, stream).of(g);
    c.located = d_located_out;
    return pooled_find(c);
}

// the same lookup with the members' bag counts read from d_member_bags (the owner's side of a sharded group: the runs that arrive per member)
int mee_group_find_pooled_jagged(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                                 const uint64_t* d_member_bags, float* d_out, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream) {
    MEE_RANGE("mee_group_find_pooled_jagged");
    if (d_located_out) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_jagged", "d_located_out (the located rows serve the backward) is");
    PooledCall c = pooled_call("mee_group_find_pooled_jagged", d_keys, n, d_bag_offsets, n_bags, d_out, MEE_DTYPE_F32, d_found, mode, stream).of(g);
    c.located = d_located_out;
    c.jagged = true; c.member_bags = d_member_bags;
    return pooled_find(c);
}

int mee_group_find_pooled_weighted(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                   const float* d_weights, float* d_out, uint8_t* d_found, int64_t* d_located_out, void* stream) {
    MEE_RANGE("mee_group_find_pooled_weighted");
    MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_weighted");
    if (n && !d_weights) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_pooled_weighted: null argument");
    PooledCall c = pooled_call("mee_group_find_pooled_weighted", d_keys, n, d_bag_offsets, bags_per_table, d_out, MEE_DTYPE_F32, d_found, MEE_POOL_SUM, stream).of(g);
    c.weights = d_weights;   // null only with n = 0
    c.located = d_located_out;
    return pooled_find(c);
}

int mee_group_find_pooled_as(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_weights,
                             void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream) {
    MEE_RANGE("mee_group_find_pooled_as");
    if (d_weights) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_as", "the weighted form (d_weights) is");
    if (d_located_out) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_as", "d_located_out (the located rows serve the backward) is");
    PooledCall c = pooled_call("mee_group_find_pooled_as", d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, mode, stream).of(g);
    c.weights = d_weights;
    c.located = d_located_out;
    return pooled_find(c);
}

// the pooled lookup of a GROUP of hot/cold pairs: find_pooled_kernel's GROUPED && TIERED instances, the hot group's descriptors in `desc`, the cold group's
// (and both groups' GroupInit, for the hit counters) in GroupTier
int mee_group_find_pooled_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                 void* d_out, uint32_t out_dtype, uint8_t* d_found, int mode, uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_pooled_tiered");
    PooledCall c = pooled_call("mee_group_find_pooled_tiered", d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, mode, stream).of(hot, cold);
    c.tier_flags = flags;
    return pooled_find(c);
}

// the same lookup with the members' bag counts read from d_member_bags, as mee_group_find_pooled_jagged reads them: find_pooled_kernel's GROUPED && JAGGED && TIERED
// instances (fp32 out: the partial rows of a sharded bag travel as fp32)
int mee_group_find_pooled_tiered_jagged(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                                        const uint64_t* d_member_bags, float* d_out, uint8_t* d_found, int mode, uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_pooled_tiered_jagged");
    PooledCall c = pooled_call("mee_group_find_pooled_tiered_jagged", d_keys, n, d_bag_offsets, n_bags, d_out, MEE_DTYPE_F32, d_found, mode, stream).of(hot, cold);
    c.tier_flags = flags;
    c.jagged = true; c.member_bags = d_member_bags;
    return pooled_find(c);
}

// ---- the keyed layout (SPEC.md §3 "Keyed output"): out[s, j * dim ...] = the pooled row of member j's sample s, one row per sample --------------
int mee_group_find_pooled_keyed(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out,
                                uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found, int64_t* d_located_out, uint32_t* d_step_index_out, int mode,
                                void* stream) {
    MEE_RANGE("mee_group_find_pooled_keyed");
    if (d_located_out) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_keyed", "d_located_out (the located rows serve the backward) is");
    if (d_step_index_out) MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_keyed", "d_step_index_out (the step index serves the backward) is");
    PooledCall c = pooled_call("mee_group_find_pooled_keyed", d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, mode, stream).of(g);
    c.located = d_located_out;
    c.keyed = true; c.out_row_stride = out_row_stride; c.step_index = d_step_index_out;
    return pooled_find(c);
}

// mee_group_find_pooled_tiered with the keyed store: the same GROUPED && TIERED instances and keys in flight, KEYED
int mee_group_find_pooled_tiered_keyed(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                       void* d_out, uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found, uint32_t* d_step_index_out, int mode,
                                       uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_pooled_tiered_keyed");
    PooledCall c = pooled_call("mee_group_find_pooled_tiered_keyed", d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, mode, stream).of(hot, cold);
    c.tier_flags = flags;
    c.keyed = true; c.out_row_stride = out_row_stride; c.step_index = d_step_index_out;
    return pooled_find(c);
}

int mee_group_pooled_weighted_backward(mee_group* g, const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets,
                                       size_t bags_per_table, const float* d_weights, const float* d_bag_grads, float* d_grads_out,
                                       float* d_weight_grads_out, void* stream) {
    MEE_RANGE("mee_group_pooled_weighted_backward");
    MEE_FP32_GROUP_ONLY(g, "mee_group_pooled_weighted_backward");
    if (!g || (bags_per_table && (!d_bag_offsets || !d_bag_grads)) || (n && (!d_keys || !d_weights || !d_grads_out)))
        return fail(MEE_ERR_INVALID_ARG, "mee_group_pooled_weighted_backward: null argument");
    if (bags_per_table == 0) return MEE_OK;
    if (int rc = group_refresh(g, stream)) return rc;
    DeviceGuard guard(g->device);
    hipStream_t st = as_stream(stream);
    const uint64_t n_bags = (uint64_t)g->n_tables * bags_per_table;
    with_pooled_shape(g->dim4, n, n_bags, [&](auto d4, auto u, auto bpw, unsigned grid) {
        pooled_weighted_backward_kernel<d4, u, bpw, true><<<grid, 256, 0, st>>>(nullptr, nullptr, 0, 0, d_keys, d_located, 0, d_bag_offsets, n_bags, d_weights,
                                                                                (const float4*)d_bag_grads, (float4*)d_grads_out, d_weight_grads_out, 0.f, g->dim4, g->d_desc, bags_per_table, n);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
// The training forward: mee_find_located whose launch also carries mee_apply_prepare for the SAME keys (the partition half of the bucketed
// apply, run by the launch's first blocks beside the row gather).  (Table without optimizer: plain mee_find_located.)
int mee::find_located_prepare(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out, void* stream, const char* name) {
    MEE_FP32_ROWS_ONLY(t, name);
    if (!t || (n && (!d_keys || !d_out || !d_slots_out))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (t->pending.n) return fail(MEE_ERR_INVALID_ARG, "%s: a prepared apply is already pending", name);
    if (n == 0) return MEE_OK;
    if (t->optimizer == MEE_OPT_NONE) return find_plane(t, t->values, t->default_value, d_keys, n, (float*)d_out, d_found, stream, {FindPath::Located, d_slots_out, -1, out_dtype});
    if (n > t->max_batch) return fail(MEE_ERR_BATCH_TOO_LARGE, "%s: n=%zu exceeds config.max_batch=%llu", name, n, (unsigned long long)t->max_batch);
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    const bool separate = t->prepare_debug & 1;   // the partition as launches of its own behind the find
    const PartPlan plan = bucket_plan(t->bk, n, st, separate ? kPartThreads : kFindPrepareThreads);
    const uint32_t part_blocks = separate ? 0u : plan.blocks;
    const int nt = kFindLocated | (t->find_nt >= 0 ? t->find_nt & kFindCachedStores : 0);   // the located find's store policy (find_plane)
    with_row_shape(t->dim4, [&](auto d4) {
        constexpr int R = d4 == 16 ? kFindPrepareR : d4 == 32 ? 2 : 1;
        const unsigned find_cap = t->prepare_debug >> 8;
        const unsigned find_blocks = grid_for(n, (kFindPrepareThreads / 64) * 4u * (unsigned)R, find_cap ? find_cap : 1u << 22);
        auto launch = [&](auto bf16, auto ntc) {
            find_prepare_kernel<d4, R, (bf16 ? kFindBF16Out : 0) | ntc><<<part_blocks + find_blocks, kFindPrepareThreads, sizeof(PartHot) + plan.nbk * 4, st>>>(t->keys, (const f32x4*)t->values, t->nb, d_keys, n,
                (f32x4*)d_out, d_found, t->default_value, t->dim4, d_slots_out, handle_tag_of(t), part_blocks, plan.nbk_hash, plan.nbk, plan.per_block, t->bk, &t->ctr->status, t->op, t->bk.xcd_split);
        };
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_value<kFindLocated | kFindCachedStores, kFindLocated>(nt, [&](auto ntc) { launch(bf16, ntc); }); });
    });
    MEE_HIP(hipGetLastError());
    if (separate) { if (int rc = bucket_partition_launch(t, d_keys, (uint32_t)n, plan, st)) return rc; }
    t->pending = {plan, n, d_keys, true};
    return MEE_OK;
}
extern "C" {

int mee_find_located_prepare(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream) {
    MEE_RANGE("mee_find_located_prepare");
    return find_located_prepare(t, d_keys, n, d_out, MEE_DTYPE_F32, d_found, d_slots_out, stream, "mee_find_located_prepare");
}
int mee_find_located_prepare_as(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out, void* stream) {
    MEE_RANGE("mee_find_located_prepare_as");
    return find_located_prepare(t, d_keys, n, d_out, out_dtype, d_found, d_slots_out, stream, "mee_find_located_prepare_as");
}

}  // extern "C"
