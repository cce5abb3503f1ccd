// meepo_group.hip — one find launch over the batches of MANY tables (a model's embedding collection).
//
// A recommendation model looks up tens of tables per step, each with a small batch; a find launch has a latency floor
// of ~7.6 us (dispatch + three dependent memory round trips, profiles/r01_find.md), so T separate launches cost T floors.
// A group holds the tables' plane descriptors on the device; mee_find_grouped serves the concatenated key batch
// (segment j = the keys of table j, segment bounds in a DEVICE offsets array, "jagged" layout) with ONE kernel whose
// tiles first locate their segment (binary search over the offsets, staged in LDS) and then run the ordinary probe +
// row gather against that table's planes.  Results are identical to calling mee_find per table (SPEC.md §3).
//
// Reference anchor: /root/reference/README.md:2 ("lookuptable-style … Embedding designed for recommendation systems").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>

#include "meepo_device.h"
#include "meepo_host.h"

namespace mee {


// One tile per key, R keys in flight per tile (same shape as find_kernel).  DIM4 = dim/4 when it is 16 or 32, 0 = any.
// LOCATE: no rows move; gslot[i] = member << 48 | slot of the key (kEmpty when absent / reserved / outside the segments) —
// the first pass of a grouped apply.
// BF16: `out` holds bf16 rows (SPEC.md §3 "Output type"): the lane's float4 leaves as 4 bf16 in one 8-byte store; BF16 = false is the code it was.
// BROWS: a bf16-row group (SPEC.md §3 "Row storage type") — every member's `values` is a bf16-row plane, read and stored through RowType (meepo_device.h) as
// find_span does it: same tiles, same index arithmetic; a member's default row is packed from its defv, which is a bf16 value already.  One storage type per
// group: a property of the launch, not a per-member branch.  The fp32 arm keeps its float4 loads and stores: through RowType's f32x4 its instances come out
// as other code (profiles/find_row_types.md).
template <int DIM4, int R, bool STREAM_OUT, bool LOCATE = false, bool BF16 = false, bool BROWS = false>
__global__ __launch_bounds__(256) void find_grouped_kernel(const GroupDesc* __restrict__ desc, uint32_t n_tables,
                                                           const uint64_t* __restrict__ offsets, const int64_t* __restrict__ keys,
                                                           uint64_t n, float4* __restrict__ out, uint8_t* __restrict__ found,
                                                           uint32_t dim4_rt, int64_t* __restrict__ gslot = nullptr,
                                                           const GroupInit* __restrict__ init = nullptr, uint64_t off_stride = 1) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    // mirrors stage_offsets (meepo_device.h) without its cut at n: the lookup path keeps its machine code
    for (uint32_t j = threadIdx.x; j <= n_tables; j += blockDim.x) loff[j] = offsets[(uint64_t)j * off_stride];  // stride > 1: the
    __syncthreads();                                                     // segment bounds are every stride-th entry of a bag-offset array
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 1;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {
        int64_t key[R], slot[R], kb[R];
        uint64_t b[R];
        GroupDesc d[R];
        uint32_t member[R];
        bool inb[R], act[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            // segment of position i: the last j with loff[j] <= i (empty segments are skipped by the search itself)
            uint32_t lo = 0, hi = n_tables;   // mirrors member_of_position (meepo_device.h): the lookup path keeps its machine code
            inb[r] = i < n && i >= loff[0] && i < loff[n_tables];
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (loff[mid] <= i) lo = mid; else hi = mid;
            }
            member[r] = lo;
            d[r] = desc[inb[r] ? lo : 0];   // 32 B, L1/L2 resident (staging the descriptors in LDS as well measured 3 % slower)
            key[r] = inb[r] ? keys[i] : kEmpty;
            act[r] = inb[r] && !reserved_key(key[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            b[r] = bucket_of(key[r], d[r].nb);
            kb[r] = act[r] ? d[r].tkeys[b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(d[r].tkeys, d[r].nb, key[r], act[r], b[r], kb[r], tile, tl);
        if constexpr (LOCATE) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (i < n && tl == 0) gslot[i] = slot[r] >= 0 ? (int64_t)(((uint64_t)member[r] << kGroupSlotBits) | (uint64_t)slot[r]) : kEmpty;
                if (inb[r] && key[r] == kReclaimed && tl == 0) atomicOr(init[member[r]].status, (uint32_t)MEE_STATUS_RESERVED_KEY);  // as mee_apply_* does
            }
            continue;
        }
        if constexpr (BROWS) {
            static_assert(!LOCATE, "bf16 rows: the lookups only");
            using RT = RowType<kRowsBF16>;
            if constexpr (DIM4 != 0) {
                RT::Group row[R][C];
#pragma unroll
                for (int r = 0; r < R; ++r)
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        row[r][c] = slot[r] >= 0 ? RT::plane(d[r].values)[RT::first(slot[r], DIM4) + c * 16 + tl] : RT::missing(f32x4{d[r].defv, d[r].defv, d[r].defv, d[r].defv});
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t i = base + r * 4 + tile;
                    if (inb[r])
#pragma unroll
                        for (int c = 0; c < C; ++c) RT::store<BF16, !STREAM_OUT>(out, i * DIM4 + c * 16 + tl, row[r][c], 0u, true, f32x4{});
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint64_t i = base + r * 4 + tile;
                    if (inb[r])
                        for (uint32_t c = tl; c < dim4; c += 16)
                            RT::store<BF16, true>(out, i * dim4 + c, slot[r] >= 0 ? RT::plane(d[r].values)[RT::first(slot[r], dim4) + c] : RT::missing(f32x4{d[r].defv, d[r].defv, d[r].defv, d[r].defv}),
                                                  0u, true, f32x4{});
                }
            }
        } else if constexpr (DIM4 != 0) {
            float4 row[R][C];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c)
                    row[r][c] = slot[r] >= 0 ? d[r].values[(uint64_t)slot[r] * DIM4 + c * 16 + tl]
                                             : make_float4(d[r].defv, d[r].defv, d[r].defv, d[r].defv);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (inb[r])
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        if constexpr (BF16) {
                            store_bf16x4<!STREAM_OUT>(out, i * DIM4 + c * 16 + tl, row[r][c]);
                        } else if constexpr (STREAM_OUT) {   // a dense output beyond the Infinity Cache: streaming stores (find_kernel's policy)
                            const f32x4 v = {row[r][c].x, row[r][c].y, row[r][c].z, row[r][c].w};
                            __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out) + i * DIM4 + c * 16 + tl);
                        } else {
                            out[i * DIM4 + c * 16 + tl] = row[r][c];
                        }
                    }
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (inb[r])
                    for (uint32_t c = tl; c < dim4; c += 16) {
                        const float4 v = slot[r] >= 0 ? d[r].values[(uint64_t)slot[r] * dim4 + c]
                                                      : make_float4(d[r].defv, d[r].defv, d[r].defv, d[r].defv);
                        if constexpr (BF16) store_bf16x4<true>(out, i * dim4 + c, v); else out[i * dim4 + c] = v;
                    }
            }
        }
        if (found) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (inb[r] && tl == 0) found[i] = slot[r] >= 0;
            }
        }
    }
}

// The row gather and the stores of one wave step of the grouped finds over fp32 rows, for a step whose rows may come from either plane of a pair: `src[r]` is
// the first element group of position r's row in the plane that holds it (any valid address where !hit[r]: it is not read), an absent key reads
// defv[r].  Straight-line per round, the R x C loads back to back before the first store, as in find_grouped_kernel.
template <int DIM4, int R, bool STREAM_OUT, bool BF16>
__device__ __forceinline__ void grouped_rows_out(const float4* const (&src)[R], const bool (&hit)[R], const float (&defv)[R], const bool (&inb)[R],
                                                 float4* __restrict__ out, uint64_t base, int tile, int tl, uint32_t dim4) {
    if constexpr (DIM4 != 0) {
        constexpr int C = DIM4 / 16;
        float4 row[R][C];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < C; ++c) row[r][c] = hit[r] ? src[r][c * 16 + tl] : make_float4(defv[r], defv[r], defv[r], defv[r]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            if (inb[r])
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if constexpr (BF16) {
                        store_bf16x4<!STREAM_OUT>(out, i * DIM4 + c * 16 + tl, row[r][c]);
                    } else if constexpr (STREAM_OUT) {
                        const f32x4 v = {row[r][c].x, row[r][c].y, row[r][c].z, row[r][c].w};
                        __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(out) + i * DIM4 + c * 16 + tl);
                    } else {
                        out[i * DIM4 + c * 16 + tl] = row[r][c];
                    }
                }
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            if (inb[r])
                for (uint32_t c = tl; c < dim4; c += 16) {
                    const float4 v = hit[r] ? src[r][c] : make_float4(defv[r], defv[r], defv[r], defv[r]);
                    if constexpr (BF16) store_bf16x4<true>(out, i * dim4 + c, v); else out[i * dim4 + c] = v;
                }
        }
    }
}

// find_grouped_kernel over a GROUP of hot/cold pairs (mee_group_find_tiered): `hot` holds the HOT member of every pair, `cold` the cold one, a key lives
// in exactly one of them.  Same tiles, same segment search (offsets stride 1), same first probe — member j's hot index, the R bucket lines requested
// back to back.  Then ONE wave-uniform decision: a wave step in which no active position missed runs find_grouped_kernel's row gather and stores and
// never looks at a cold descriptor (the steady state of a well-placed collection).  Otherwise the cold descriptor of every missed position's member
// is loaded — inside this branch only — and the cold index probed by all 64 lanes in convergent control flow, tiles without a miss pass act = false;
// each row is then loaded ONCE, from the plane that holds it (the address is selected, not the data; slot 0 of a cold plane where neither tier
// holds the key: a valid address that is not read).  The cold plane may be pinned host memory: plain loads.  An absent or reserved key reads the HOT
// member's defv; found[i] (nullable) = either tier holds the key; positions outside the segments or at or past n are left alone, as there.
// count (kTierCountCold | kTierCountHot, the launch's bits — never a member's pointer — so every wave-uniform branch is on a fact of the launch): one
// atomicAdd per found position by the tile's first lane on that member's counter, as find_kernel (kFindCountHits) and find_missing_kernel do it.
template <int DIM4, int R, bool STREAM_OUT, bool BF16 = false>
__global__ __launch_bounds__(256) void find_grouped_tiered_kernel(const GroupDesc* __restrict__ hot, const GroupInit* __restrict__ hot_init,
                                                                  const GroupDesc* __restrict__ cold, const GroupInit* __restrict__ cold_init,
                                                                  uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                                  const int64_t* __restrict__ keys, uint64_t n, float4* __restrict__ out,
                                                                  uint8_t* __restrict__ found, uint32_t dim4_rt, uint32_t count) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    for (uint32_t j = threadIdx.x; j <= n_tables; j += blockDim.x) loff[j] = offsets[j];   // mirrors stage_offsets (meepo_device.h), as find_grouped_kernel
    __syncthreads();
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {
        int64_t key[R], slot[R], kb[R];
        uint64_t b[R];
        const int64_t* tkeys[R];
        uint64_t nb[R];
        const float4* src[R];   // first the hot plane, then the row
        float defv[R];
        uint32_t member[R];
        bool inb[R], act[R], hit[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            uint32_t lo = 0, hi = n_tables;   // mirrors member_of_position (meepo_device.h), as find_grouped_kernel
            inb[r] = i < n && i >= loff[0] && i < loff[n_tables];
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (loff[mid] <= i) lo = mid; else hi = mid;
            }
            member[r] = inb[r] ? lo : 0;
            const GroupDesc d = hot[member[r]];
            tkeys[r] = d.tkeys; nb[r] = d.nb; src[r] = d.values; defv[r] = d.defv;
            key[r] = inb[r] ? keys[i] : kEmpty;
            act[r] = inb[r] && !reserved_key(key[r]);
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            b[r] = bucket_of(key[r], nb[r]);
            kb[r] = act[r] ? tkeys[r][b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys[r], nb[r], key[r], act[r], b[r], kb[r], tile, tl);
        bool missed = false;
#pragma unroll
        for (int r = 0; r < R; ++r) missed = missed || (act[r] && slot[r] < 0);
        if (!__any(missed)) {   // wave-uniform: nothing for the cold tier
#pragma unroll
            for (int r = 0; r < R; ++r) {
                hit[r] = slot[r] >= 0;
                src[r] += (uint64_t)(hit[r] ? slot[r] : 0) * dim4;
            }
            grouped_rows_out<DIM4, R, STREAM_OUT, BF16>(src, hit, defv, inb, out, base, tile, tl, dim4);
        } else {
            int64_t cslot[R];
            const float4* cvalues[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                act[r] = act[r] && slot[r] < 0;   // from here on: the positions the cold index is asked about
                const GroupDesc* c = cold + (act[r] ? member[r] : 0);
                tkeys[r] = c->tkeys; nb[r] = c->nb; cvalues[r] = c->values;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                b[r] = bucket_of(key[r], nb[r]);
                kb[r] = act[r] ? tkeys[r][b[r] * kW + tl] : kEmpty;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) cslot[r] = tile_probe(tkeys[r], nb[r], key[r], act[r], b[r], kb[r], tile, tl);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                hit[r] = slot[r] >= 0 || cslot[r] >= 0;
                src[r] = slot[r] >= 0 ? src[r] + (uint64_t)slot[r] * dim4 : cvalues[r] + (uint64_t)(cslot[r] >= 0 ? cslot[r] : 0) * dim4;
            }
            grouped_rows_out<DIM4, R, STREAM_OUT, BF16>(src, hit, defv, inb, out, base, tile, tl, dim4);
            if (count & kTierCountCold) {   // wave-uniform
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (cslot[r] >= 0 && tl == 0) atomicAdd(&cold_init[member[r]].hits[cslot[r]], 1u);
            }
        }
        if (found) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint64_t i = base + r * 4 + tile;
                if (inb[r] && tl == 0) found[i] = hit[r];
            }
        }
        if (count & kTierCountHot) {   // wave-uniform (sampled calls)
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (slot[r] >= 0 && tl == 0) atomicAdd(&hot_init[member[r]].hits[slot[r]], 1u);
        }
    }
}

// Second pass of a grouped find_or_insert: ensure_grouped_body (meepo_device.h) with member j creating in desc[j] / init[j], and the
// initial row of every position that obtained a slot written into `out`.  BF16: `out` holds bf16 rows — the returned copy is rounded, the table's row is not.
template <bool BF16 = false>
__global__ __launch_bounds__(256) void ensure_grouped_kernel(const GroupDesc* __restrict__ desc, const GroupInit* __restrict__ init,
                                                             uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                             const int64_t* __restrict__ keys, uint64_t n,
                                                             const uint8_t* __restrict__ found, uint32_t dim4, float4* __restrict__ out) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<true, BF16>(loff, n_tables, offsets, 1, keys, n, found, out,
                                    [&](uint32_t lo, bool) { return GroupMember{desc + lo, init + lo, dim4}; });
}

// The creation of mee_group_find_or_insert_admit, the decision fused in: the tile of a missing position first reads its member's three sketch
// counters — final since the kernel boundary behind sketch_add_grouped_kernel, and not written here — and goes on to tile_locate only when their
// minimum reached that member's threshold (min_counts[member] when given, else min_count); otherwise the position keeps the default row the find
// pass wrote.  Everything else is ensure_grouped_kernel's.  This kernel keeps its own text — it mirrors ensure_grouped_body (meepo_device.h:
// stage_offsets, member_of_position, creation_write) with the gate in front of tile_locate: as a wrapper around that body it measured about
// 1 us per call slower with a tenth of the batch admitted, in two series (profiles/grouped_creation.md).
template <bool BF16>
__global__ __launch_bounds__(256) void ensure_admit_grouped_kernel(const GroupDesc* __restrict__ desc, const GroupInit* __restrict__ init,
                                                                   const GroupAdmit* __restrict__ admit, uint32_t n_tables,
                                                                   const uint64_t* __restrict__ offsets, const int64_t* __restrict__ keys, uint64_t n,
                                                                   const uint8_t* __restrict__ found, uint32_t dim4, float4* __restrict__ out,
                                                                   uint32_t min_count, const uint32_t* __restrict__ min_counts) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    for (uint32_t j = threadIdx.x; j <= n_tables; j += blockDim.x) loff[j] = offsets[j];
    __syncthreads();
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 4; base < n; base += n_waves * 4) {
        const uint64_t i = base + tile;
        bool act = i < n && i >= loff[0] && i < loff[n_tables] && found[i] == 0;
        const int64_t key = act ? keys[i] : kEmpty;
        const bool tomb = act && key == kReclaimed;   // a reserved key in the batch: flagged like mee_find_or_insert does (EMPTY = padding, silent)
        act = act && !reserved_key(key);
        if (!__any(act || tomb)) continue;  // wave-uniform: nothing missing here (the steady state of a trained vocabulary)
        uint32_t lo = 0, hi = n_tables;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (loff[mid] <= i) lo = mid; else hi = mid;
        }
        if (tomb && tl == 0) atomicOr(init[lo].status, (uint32_t)MEE_STATUS_RESERVED_KEY);
        if (act) {   // the 16 lanes of a tile read the same three counters: one request each
            const GroupAdmit a = admit[lo];
            uint32_t est = 0xFFFFFFFFu;
#pragma unroll
            for (int r = 0; r < 3; ++r) est = min(est, a.sketch[sketch_index(key, r, a.log2w)]);
            act = est >= (min_counts ? min_counts[lo] : min_count);
        }
        if (!__any(act)) continue;  // wave-uniform: counted, nobody admitted
        const GroupDesc d = desc[act ? lo : 0];
        bool is_new, full;
        const int64_t slot = tile_locate<true, true>(const_cast<int64_t*>(d.tkeys), d.nb, key, act, tile, tl, is_new, full);
        if (act) {
            const GroupInit in = init[lo];
            if (slot >= 0) {
                for (uint32_t c = tl; c < dim4; c += 16) {
                    const float4 row = initial_row4(key, c * 4, in.initializer, in.init_scale, in.init_seed, d.defv);
                    if constexpr (BF16) store_bf16x4<true>(out, i * dim4 + c, row); else out[i * dim4 + c] = row;
                    if (is_new) {
                        d.values[(uint64_t)slot * dim4 + c] = row;
                        if (in.optimizer == MEE_OPT_ADAGRAD) d.s1[(uint64_t)slot * dim4 + c] = make_float4(in.init_acc, in.init_acc, in.init_acc, in.init_acc);
                        if (in.optimizer == MEE_OPT_ADAM) {
                            d.s1[(uint64_t)slot * dim4 + c] = make_float4(0.f, 0.f, 0.f, 0.f);
                            d.s2[(uint64_t)slot * dim4 + c] = make_float4(0.f, 0.f, 0.f, 0.f);
                        }
                        if (in.optimizer == MEE_OPT_FTRL) {
                            d.s1[(uint64_t)slot * dim4 + c] = make_float4(0.f, 0.f, 0.f, 0.f);
                            d.s2[(uint64_t)slot * dim4 + c] = make_float4(in.init_acc, in.init_acc, in.init_acc, in.init_acc);
                        }
                    }
                }
                if (is_new && in.hits && tl == 0) in.hits[slot] = 0;
            }
            if (full && tl == 0) atomicOr(in.status, (uint32_t)MEE_STATUS_TABLE_FULL);
        }
    }
}

// Grouped admission, the counting launch (between the find and the creation of mee_group_find_or_insert_admit): one thread per position of the jagged
// batch, positions indexed in 64 bits.  A position inside [offsets[0], offsets[n_tables]) and below n whose found byte is 0 and whose key is not
// reserved adds 1 to the three counters of ITS member's sketch (stage_offsets / member_of_position, meepo_device.h); a key that occurs
// c times adds c.  Integer atomicAdd commutes: the sketch after the launch does not depend on the order.  off_stride: stage_offsets' — 1 for a jagged
// batch, bags_per_table where the members' bounds are every bags_per_table-th entry of a bag-offset array (mee_group_ensure_admit_tiered).
__global__ __launch_bounds__(256) void sketch_add_grouped_kernel(const GroupAdmit* __restrict__ admit, uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                                 uint64_t off_stride, const int64_t* __restrict__ keys, uint64_t n,
                                                                 const uint8_t* __restrict__ found) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    stage_offsets(loff, offsets, off_stride, n_tables, n);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        if (i < loff[0] || i >= loff[n_tables] || found[i]) continue;
        const int64_t k = keys[i];
        if (reserved_key(k)) continue;
        const GroupAdmit a = admit[member_of_position(loff, n_tables, i)];
#pragma unroll
        for (int r = 0; r < 3; ++r) atomicAdd(&a.sketch[sketch_index(k, r, a.log2w)], 1u);
    }
}
// mee_group_admission_decay: blockIdx.y = member, every counter of its sketch >>= shift (>= 32: zero), as sketch_decay_kernel ages one table's
__global__ __launch_bounds__(256) void sketch_decay_grouped_kernel(const GroupAdmit* __restrict__ admit, uint32_t shift) {
    const GroupAdmit a = admit[blockIdx.y];
    const uint64_t n = 3ull << a.log2w;
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        a.sketch[i] = shift >= 32 ? 0u : a.sketch[i] >> shift;
}

// The creation passes over a GROUP of hot/cold pairs: ensure_grouped_body with member j creating in ONE tier of its pair — the cold table where
// to_cold[j] != 0 (null: every member creates hot) — as mee_find_or_insert_missing on that table creates: the initial row from THAT table's
// initializer, its initial optimizer state, a zero hit counter; TABLE_FULL and RESERVED_KEY (a tombstone value in the batch) go to that table's status word.
struct TierOf {
    const GroupDesc *hot_desc, *cold_desc;
    const GroupInit *hot_init, *cold_init;
    const uint8_t* to_cold;
    uint32_t dim4;
    __device__ GroupMember operator()(uint32_t lo, bool live) const {
        const bool goes_cold = to_cold && live && to_cold[lo] != 0;
        return GroupMember{(goes_cold ? cold_desc : hot_desc) + lo, (goes_cold ? cold_init : hot_init) + lo, dim4};
    }
};

// mee_group_ensure_tiered (the pooled lookup with insert_missing): member segments are every bags_per_table-th bag offset (the off_stride of
// group_locate).  No row is written back — the pooled lookup that follows reads the tables — so no [n, dim] buffer exists.
__global__ __launch_bounds__(256) void ensure_tiered_grouped_kernel(const GroupDesc* __restrict__ hot_desc, const GroupInit* __restrict__ hot_init,
                                                                    const GroupDesc* __restrict__ cold_desc, const GroupInit* __restrict__ cold_init,
                                                                    uint32_t n_tables, const uint64_t* __restrict__ offsets, uint64_t bags_per_table,
                                                                    const int64_t* __restrict__ keys, uint64_t n, const uint8_t* __restrict__ found,
                                                                    const uint8_t* __restrict__ to_cold, uint32_t dim4) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<false, false>(loff, n_tables, offsets, bags_per_table, keys, n, found, nullptr,
                                      TierOf{hot_desc, cold_desc, hot_init, cold_init, to_cold, dim4});
}

// mee_group_find_or_insert_tiered (the unpooled find_or_insert over a group of pairs), which returns a row per position: what ensure_grouped_kernel<BF16>
// does, in the tier to_cold selects, over the n_tables + 1 jagged offsets of the lookup.
template <bool BF16>
__global__ __launch_bounds__(256) void ensure_tiered_grouped_rows_kernel(const GroupDesc* __restrict__ hot_desc, const GroupInit* __restrict__ hot_init,
                                                                         const GroupDesc* __restrict__ cold_desc, const GroupInit* __restrict__ cold_init,
                                                                         uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                                         const int64_t* __restrict__ keys, uint64_t n, const uint8_t* __restrict__ found,
                                                                         const uint8_t* __restrict__ to_cold, uint32_t dim4, float4* __restrict__ out) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<true, BF16>(loff, n_tables, offsets, 1, keys, n, found, out, TierOf{hot_desc, cold_desc, hot_init, cold_init, to_cold, dim4});
}

// Admission over a group of pairs (SPEC.md §3 "Tiering": the pair's sketch is its HOT table's).  The gate of the two creations below: the tile of a
// missing position reads the three counters of its member's hot sketch — `admit` is the HOT group's d_admit whatever to_cold says, final since the
// kernel boundary behind sketch_add_grouped_kernel and not written here; the 16 lanes of a tile read the same three words, one request each — and
// the key goes on to tile_locate only when their minimum reached min_counts[member] (when given, else min_count).
struct AdmitGate {
    const GroupAdmit* admit;
    uint32_t min_count;
    const uint32_t* min_counts;
    __device__ bool operator()(uint32_t lo, int64_t key) const {
        const GroupAdmit a = admit[lo];
        uint32_t est = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < 3; ++r) est = min(est, a.sketch[sketch_index(key, r, a.log2w)]);
        return est >= (min_counts ? min_counts[lo] : min_count);
    }
};

// mee_group_ensure_admit_tiered: ensure_tiered_grouped_kernel behind the gate (no rows out; member bounds every bags_per_table-th bag offset)
__global__ __launch_bounds__(256) void ensure_admit_tiered_grouped_kernel(const GroupDesc* __restrict__ hot_desc, const GroupInit* __restrict__ hot_init,
                                                                          const GroupDesc* __restrict__ cold_desc, const GroupInit* __restrict__ cold_init,
                                                                          const GroupAdmit* __restrict__ hot_admit, uint32_t n_tables,
                                                                          const uint64_t* __restrict__ offsets, uint64_t bags_per_table,
                                                                          const int64_t* __restrict__ keys, uint64_t n, const uint8_t* __restrict__ found,
                                                                          const uint8_t* __restrict__ to_cold, uint32_t dim4, uint32_t min_count,
                                                                          const uint32_t* __restrict__ min_counts) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<false, false>(loff, n_tables, offsets, bags_per_table, keys, n, found, nullptr,
                                      TierOf{hot_desc, cold_desc, hot_init, cold_init, to_cold, dim4}, AdmitGate{hot_admit, min_count, min_counts});
}

// mee_group_find_or_insert_admit_tiered: ensure_tiered_grouped_rows_kernel<BF16> behind the gate; a position turned away keeps the hot default row
// the lookup wrote
template <bool BF16>
__global__ __launch_bounds__(256) void ensure_admit_tiered_grouped_rows_kernel(const GroupDesc* __restrict__ hot_desc, const GroupInit* __restrict__ hot_init,
                                                                               const GroupDesc* __restrict__ cold_desc, const GroupInit* __restrict__ cold_init,
                                                                               const GroupAdmit* __restrict__ hot_admit, uint32_t n_tables,
                                                                               const uint64_t* __restrict__ offsets, const int64_t* __restrict__ keys,
                                                                               uint64_t n, const uint8_t* __restrict__ found,
                                                                               const uint8_t* __restrict__ to_cold, uint32_t dim4, float4* __restrict__ out,
                                                                               uint32_t min_count, const uint32_t* __restrict__ min_counts) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<true, BF16>(loff, n_tables, offsets, 1, keys, n, found, out, TierOf{hot_desc, cold_desc, hot_init, cold_init, to_cold, dim4},
                                    AdmitGate{hot_admit, min_count, min_counts});
}

}  // namespace mee

using namespace mee;


static int upload_descriptors(mee_group* g) {
    std::vector<GroupDesc> h(g->n_tables);
    std::vector<GroupInit> hi(g->n_tables);
    std::vector<MoveTable> hm(g->n_tables);
    std::vector<GroupAdmit> ha(g->n_tables);
    for (uint32_t j = 0; j < g->n_tables; ++j) {
        const TableView v = table_view(g->tables[j]);
        h[j] = GroupDesc{v.keys, (float4*)v.values, (float4*)v.s1, (float4*)v.s2, v.nb, v.default_value, 0};   // (a bf16-row member: its bf16 plane behind the same pointer — the launch knows, g->bf16_rows)
        hi[j] = GroupInit{v.init_seed, v.status, v.hits, v.initializer, v.optimizer, v.init_scale, v.init_acc};
        hm[j] = MoveTable{const_cast<int64_t*>(v.keys), {(float4*)v.values, (float4*)v.s1, (float4*)v.s2}, v.nb, v.status, v.hits, v.batch_slots};
        ha[j] = GroupAdmit{v.sketch, v.sketch_log2w, 0};
        g->generations[j] = v.generation;
    }
    MEE_HIP(hipMemcpy(g->d_desc, h.data(), h.size() * sizeof(GroupDesc), hipMemcpyHostToDevice));  // synchronous, rare
    MEE_HIP(hipMemcpy(g->d_init, hi.data(), hi.size() * sizeof(GroupInit), hipMemcpyHostToDevice));
    MEE_HIP(hipMemcpy(g->d_move, hm.data(), hm.size() * sizeof(MoveTable), hipMemcpyHostToDevice));
    MEE_HIP(hipMemcpy(g->d_admit, ha.data(), ha.size() * sizeof(GroupAdmit), hipMemcpyHostToDevice));
    return MEE_OK;
}

namespace mee {
int group_refresh(mee_group* g, void* stream) {
    for (uint32_t j = 0; j < g->n_tables; ++j)
        if (table_view(g->tables[j]).generation != g->generations[j]) {   // a table was rehashed: its planes moved
            DeviceGuard guard(g->device);
            MEE_HIP(hipStreamSynchronize((hipStream_t)stream));           // launches in flight may still read the old descriptors
            return upload_descriptors(g);
        }
    return MEE_OK;
}
int group_locate(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, uint64_t off_stride, size_t n, int64_t* d_gslot, hipStream_t st) {
    find_grouped_kernel<0, 2, false, true><<<grid_for(n, 32, 8192), 256, 0, st>>>(g->d_desc, g->n_tables, d_offsets, d_keys, n, nullptr, nullptr, g->dim4, d_gslot, g->d_init, off_stride);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}
}  // namespace mee

extern "C" {

int mee_group_create(mee_table* const* tables, uint32_t n_tables, uint64_t max_apply_batch, mee_group** out) {
    MEE_RANGE("mee_group_create");
    if (!tables || !out || n_tables == 0 || n_tables > kMaxGroupTables)
        return fail(MEE_ERR_INVALID_ARG, "mee_group_create: need 1..%u tables", kMaxGroupTables);
    *out = nullptr;
    for (uint32_t j = 0; j < n_tables; ++j)
        if (!tables[j]) return fail(MEE_ERR_INVALID_ARG, "mee_group_create: table %u is null", j);
    for (uint32_t j = 0; j < n_tables; ++j) MEE_NO_INT8_ROWS(tables[j], "mee_group_create");   // (an int8-row table is no member: covers every mee_group_* operator)
    const TableView v0 = table_view(tables[0]);
    // one row storage type per group: it is a compile-time property of every launch (the BROWS instances), not a per-member branch in the row fetch
    for (uint32_t j = 1; j < n_tables; ++j)
        if (table_view(tables[j]).bf16_rows != v0.bf16_rows)
            return fail(MEE_ERR_UNSUPPORTED, "mee_group_create: table %u is %s and table 0 is %s — a group holds fp32-row tables or bf16-row table members (MEE_FLAG_BF16_ROWS), never both",
                        j, v0.bf16_rows ? "an fp32-row table" : "a bf16-row table", v0.bf16_rows ? "a bf16-row table" : "an fp32-row table");
    if (v0.bf16_rows && max_apply_batch)
        return fail(MEE_ERR_INVALID_ARG, "mee_group_create: max_apply_batch must be 0 for a group of bf16-row tables (a serving group has no step and no scratch table)");
    for (uint32_t j = 1; j < n_tables; ++j) {
        const TableView v = table_view(tables[j]);
        if (v.device != v0.device || v.dim != v0.dim)
            return fail(MEE_ERR_INVALID_ARG, "mee_group_create: table %u differs from table 0 in device or dim (%d/%u vs %d/%u)", j, v.device, v.dim, v0.device, v0.dim);
        if (max_apply_batch && v.optimizer != v0.optimizer)
            return fail(MEE_ERR_INVALID_ARG, "mee_group_create: a group with grouped apply needs one optimizer for all members (table %u: %u vs %u)", j, v.optimizer, v0.optimizer);
    }
    if (max_apply_batch > (1ull << 30)) return fail(MEE_ERR_INVALID_ARG, "mee_group_create: max_apply_batch must be <= 2^30");
    mee_group* g = new (std::nothrow) mee_group();
    if (!g) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    g->device = v0.device; g->n_tables = n_tables; g->dim = v0.dim; g->dim4 = v0.dim4; g->bf16_rows = v0.bf16_rows; g->d_desc = nullptr;
    g->optimizer = v0.optimizer; g->max_apply_batch = max_apply_batch; g->scratch = nullptr; g->d_gslot = nullptr;
    g->d_init = nullptr; g->d_move = nullptr; g->d_fmask = nullptr; g->d_admit = nullptr; g->no_admission = -1;
    for (uint32_t j = n_tables; j-- > 0;)
        if (!table_view(tables[j]).sketch) g->no_admission = (int)j;
    g->tables.assign(tables, tables + n_tables);
    g->generations.assign(n_tables, 0);
    DeviceGuard guard(g->device);
    hipError_t e = hipMalloc((void**)&g->d_desc, n_tables * sizeof(GroupDesc));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_init, n_tables * sizeof(GroupInit));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_move, n_tables * sizeof(MoveTable));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_admit, n_tables * sizeof(GroupAdmit));
    if (e == hipSuccess && max_apply_batch) e = hipMalloc((void**)&g->d_fmask, max_apply_batch);
    if (e != hipSuccess) { mee_group_destroy(g); return fail(MEE_ERR_OUT_OF_MEMORY, "hipMalloc(group descriptors): %s", hipGetErrorString(e)); }
    if (int rc = upload_descriptors(g)) { mee_group_destroy(g); return rc; }
    if (max_apply_batch && g->optimizer != MEE_OPT_NONE) {
        // the group's own group table, per-position arrays and counters: a 16-slot table that only lends its scratch
        mee_config c{};
        c.struct_size = sizeof c; c.device = g->device; c.capacity = 16; c.dim = g->dim; c.optimizer = g->optimizer; c.max_batch = max_apply_batch;
        int rc = mee_table_create(&c, &g->scratch);
        if (rc == MEE_OK && hipMalloc((void**)&g->d_gslot, max_apply_batch * sizeof(int64_t)) != hipSuccess)
            rc = fail(MEE_ERR_OUT_OF_MEMORY, "hipMalloc(group slot list)");
        if (rc != MEE_OK) { mee_group_destroy(g); return rc; }
    }
    *out = g;
    return MEE_OK;
}

int mee_group_value_dtype(const mee_group* g, uint32_t* out) {
    if (!g || !out) return fail(MEE_ERR_INVALID_ARG, "mee_group_value_dtype: null argument");
    *out = g->bf16_rows ? MEE_DTYPE_BF16 : MEE_DTYPE_F32;
    return MEE_OK;
}

int mee_group_set_tuning(mee_group* g, const char* name, int value) {
    if (!g || !name) return fail(MEE_ERR_INVALID_ARG, "mee_group_set_tuning: null argument");
    if (!g->scratch) return fail(MEE_ERR_UNSUPPORTED, "mee_group_set_tuning: the group has no apply of its own (max_apply_batch = 0 or tables without optimizer)");
    return mee_set_tuning(g->scratch, name, value);
}

int mee_group_destroy(mee_group* g) {
    MEE_RANGE("mee_group_destroy");
    if (!g) return MEE_OK;
    DeviceGuard guard(g->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(g->d_desc);
    (void)hipFree(g->d_init);
    (void)hipFree(g->d_move);
    (void)hipFree(g->d_admit);
    (void)hipFree(g->d_fmask);
    (void)hipFree(g->d_gslot);
    if (g->scratch) mee_table_destroy(g->scratch);
    delete g;
    return MEE_OK;
}

}  // extern "C"

// ---- a group of hot/cold pairs: member j of `hot` and member j of `cold` are the two tiers of pair j (a key lives in exactly one of them) ----
int mee::tiered_groups_check(const mee_group* hot, const mee_group* cold, uint32_t count_flags, const char* name) {
    MEE_FP32_GROUP_ONLY(hot, name);
    MEE_FP32_GROUP_ONLY(cold, name);
    if (!hot || !cold) return fail(MEE_ERR_INVALID_ARG, "%s: null group", name);
    if (hot == cold) return fail(MEE_ERR_INVALID_ARG, "%s: hot and cold are the same group (a key lives in exactly one tier)", name);
    if (hot->device != cold->device || hot->dim != cold->dim || hot->n_tables != cold->n_tables)
        return fail(MEE_ERR_INVALID_ARG, "%s: the groups differ in device (%d, %d), dim (%u, %u) or number of tables (%u, %u)", name, hot->device, cold->device,
                    hot->dim, cold->dim, hot->n_tables, cold->n_tables);
    for (uint32_t j = 0; j < hot->n_tables; ++j)
        if (hot->tables[j] == cold->tables[j]) return fail(MEE_ERR_INVALID_ARG, "%s: member %u is the same table in both groups (a key lives in exactly one tier)", name, j);
    if (count_flags & ~(uint32_t)(MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT)) return fail(MEE_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", name, count_flags);
    for (uint32_t j = 0; j < hot->n_tables; ++j)   // (only under a count bit: the plain lookup does not walk the members)
        if (((count_flags & MEE_TIER_COUNT_COLD) && !table_view(cold->tables[j]).hits) || ((count_flags & MEE_TIER_COUNT_HOT) && !table_view(hot->tables[j]).hits))
            return fail(MEE_ERR_INVALID_ARG, "%s: a count flag needs every member of that tier created with MEE_FLAG_TRACK_HITS (member %u has no counters)", name, j);
    return MEE_OK;
}

extern "C" int mee_group_ensure_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                       const uint8_t* d_found, const uint8_t* d_to_cold, void* stream) {
    MEE_RANGE("mee_group_ensure_tiered");
    if (!hot || !cold || (bags_per_table && !d_bag_offsets) || (n && (!d_keys || !d_found))) return fail(MEE_ERR_INVALID_ARG, "mee_group_ensure_tiered: null argument");
    if (int rc = tiered_groups_check(hot, cold, 0, "mee_group_ensure_tiered")) return rc;
    if (bags_per_table == 0 || n == 0) return MEE_OK;
    if (int rc = group_refresh(hot, stream)) return rc;
    if (int rc = group_refresh(cold, stream)) return rc;
    DeviceGuard guard(hot->device);
    ensure_tiered_grouped_kernel<<<grid_for(n, 16, 8192), 256, 0, (hipStream_t)stream>>>(hot->d_desc, hot->d_init, cold->d_desc, cold->d_init, hot->n_tables, d_bag_offsets,
                                                                                        bags_per_table, d_keys, n, d_found, d_to_cold, hot->dim4);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

static int launch_find_grouped(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                               hipStream_t st) {
    const bool bf16 = out_dtype == MEE_DTYPE_BF16;
    const bool stream_out = (uint64_t)n * g->dim * (bf16 ? 2 : 4) > kCachedOutputBytes;   // find_kernel's store policy, on the bytes really written
    // every block starts by staging the offsets in LDS (a global round trip + a barrier): blocks must live long enough to
    // amortise it, so the grid is capped and strides (measured: 8192 blocks best from 200K to 1M positions)
    const unsigned grid_cap = 8192;
    with_row_shape(g->dim4, [&](auto d4) { with_flag(stream_out, [&](auto so) {
        constexpr int R = RowShape<d4>::rows_per_tile;   // (a block: 16 tiles of R keys in flight)
        if (g->bf16_rows) with_flag(bf16, [&](auto b16) {   // a bf16-row group: the BROWS instances, fp32 or bf16 out
            find_grouped_kernel<d4, R, so, false, b16, true><<<grid_for(n, 16 * R, grid_cap), 256, 0, st>>>(g->d_desc, g->n_tables, d_offsets, d_keys, n, (float4*)d_out, d_found, g->dim4);
        });
        else if (bf16) find_grouped_kernel<d4, R, so, false, true><<<grid_for(n, 16 * R, grid_cap), 256, 0, st>>>(g->d_desc, g->n_tables, d_offsets, d_keys, n, (float4*)d_out, d_found, g->dim4);
        else find_grouped_kernel<d4, R, so><<<grid_for(n, 16 * R, grid_cap), 256, 0, st>>>(g->d_desc, g->n_tables, d_offsets, d_keys, n, (float4*)d_out, d_found, g->dim4);
    }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

static int find_grouped_common(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                               void* stream, const char* name) {
    if (!g || !d_offsets || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (n == 0) return MEE_OK;
    if (int rc = group_refresh(g, stream)) return rc;
    DeviceGuard guard(g->device);
    return launch_find_grouped(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, (hipStream_t)stream);
}

// What every grouped find_or_insert does in front of its creation launches: the argument checks, the group's own found mask where the caller gave none
// (n <= max_apply_batch then), the descriptor refresh, and the ordinary grouped find, which serves every stored key and yields the present-before
// mask.  Then create(st, d_found) launches what creates the missing keys, on the same stream and device.
template <class Create>
static int group_find_then_create(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                  void* stream, const char* name, Create&& create) {
    MEE_FP32_GROUP_ONLY(g, name);
    if (!g || !d_offsets || (n && (!d_keys || !d_out))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (n == 0) return MEE_OK;
    if (!d_found) {
        if (n > g->max_apply_batch)
            return fail(MEE_ERR_BATCH_TOO_LARGE, "%s: without a found buffer n=%zu must be <= max_apply_batch=%llu", name, n, (unsigned long long)g->max_apply_batch);
        d_found = g->d_fmask;
    }
    if (int rc = group_refresh(g, stream)) return rc;
    DeviceGuard guard(g->device);
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_find_grouped(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, st)) return rc;
    create(st, d_found);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

static int group_find_or_insert_common(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                       void* stream, const char* name) {
    // missing positions create their key (one creator per distinct key: the CAS decides) and return its initial row
    return group_find_then_create(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream, name, [&](hipStream_t st, uint8_t* found) {
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto b16) {
            ensure_grouped_kernel<b16><<<grid_for(n, 16, 8192), 256, 0, st>>>(g->d_desc, g->d_init, g->n_tables, d_offsets, d_keys, n, found, g->dim4, (float4*)d_out);
        });
    });
}

// every member has a sketch, or MEE_ERR_UNSUPPORTED naming the first that has none
static int group_admission_check(const mee_group* g, const char* name) {
    MEE_FP32_GROUP_ONLY(g, name);
    if (g && g->no_admission >= 0)
        return fail(MEE_ERR_UNSUPPORTED, "%s: member %d was created without MEE_FLAG_ADMISSION (every member needs its own sketch)", name, g->no_admission);
    return MEE_OK;
}

extern "C" int mee_group_find_or_insert_admit(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                              uint32_t min_count, const uint32_t* d_min_counts, void* stream) {
    MEE_RANGE("mee_group_find_or_insert_admit");
    const char* name = "mee_group_find_or_insert_admit";
    if (int rc = group_admission_check(g, name)) return rc;
    return group_find_then_create(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream, name, [&](hipStream_t st, uint8_t* found) {
        // every missing position counts its key in its member's sketch ...
        sketch_add_grouped_kernel<<<grid_for(n, 256, 4096), 256, 0, st>>>(g->d_admit, g->n_tables, d_offsets, 1, d_keys, n, found);
        // ... then the creation of mee_group_find_or_insert, for the positions whose estimate reached their member's threshold
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto b16) {
            ensure_admit_grouped_kernel<b16><<<grid_for(n, 16, 8192), 256, 0, st>>>(g->d_desc, g->d_init, g->d_admit, g->n_tables, d_offsets, d_keys, n, found, g->dim4, (float4*)d_out,
                                                                                   min_count, d_min_counts);
        });
    });
}

extern "C" int mee_group_admission_decay(mee_group* g, uint32_t shift, void* stream) {
    MEE_RANGE("mee_group_admission_decay");
    if (int rc = group_admission_check(g, "mee_group_admission_decay")) return rc;
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_group_admission_decay: null group");
    if (int rc = group_refresh(g, stream)) return rc;
    DeviceGuard guard(g->device);
    uint32_t log2w = 0;
    for (mee_table* t : g->tables) log2w = std::max(log2w, table_view(t).sketch_log2w);
    const unsigned per_member = g->n_tables >= 2048 / 4 ? 4 : 2048 / g->n_tables;   // ~2048 blocks in all, as mee_admission_decay launches for one table
    sketch_decay_grouped_kernel<<<dim3(grid_for(3ull << log2w, 256, per_member), g->n_tables), 256, 0, (hipStream_t)stream>>>(g->d_admit, shift);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// the one launch of the unpooled lookup over a group of pairs; the store policy is launch_find_grouped's, on the bytes really written
static int launch_find_grouped_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                      uint8_t* d_found, uint32_t count, hipStream_t st) {
    const bool bf16 = out_dtype == MEE_DTYPE_BF16;
    const bool stream_out = (uint64_t)n * hot->dim * (bf16 ? 2 : 4) > kCachedOutputBytes;
    with_row_shape(hot->dim4, [&](auto d4) { with_flag(stream_out, [&](auto so) { with_flag(bf16, [&](auto b16) {
        constexpr int R = RowShape<d4>::rows_per_tile;
        find_grouped_tiered_kernel<d4, R, so, b16><<<grid_for(n, 16 * R, 8192), 256, 0, st>>>(hot->d_desc, hot->d_init, cold->d_desc, cold->d_init, hot->n_tables, d_offsets, d_keys, n,
                                                                                             (float4*)d_out, d_found, hot->dim4, count);
    }); }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// what admits of a group of pairs: a threshold for all members or one per member (device, n_tables entries); null = the call does not admit
struct TierAdmission {
    uint32_t min_count;
    const uint32_t* d_min_counts;
};

// creates: mee_group_find_or_insert_tiered (d_found required, d_to_cold read); with `admits` mee_group_find_or_insert_admit_tiered, whose creation
// stands behind the hot sketches; otherwise mee_group_find_tiered
static int group_find_tiered_common(mee_group* hot, mee_group* cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                    uint8_t* d_found, bool creates, const uint8_t* d_to_cold, uint32_t flags, void* stream, const char* name,
                                    const TierAdmission* admits = nullptr) {
    if (!hot || !cold || !d_offsets || (n && (!d_keys || !d_out || (creates && !d_found)))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = tiered_groups_check(hot, cold, flags, name)) return rc;
    if (admits)   // the pair's sketch is its hot table's: the cold members need none
        if (int rc = group_admission_check(hot, name)) return rc;
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (n == 0) return MEE_OK;
    if (int rc = group_refresh(hot, stream)) return rc;
    if (int rc = group_refresh(cold, stream)) return rc;
    DeviceGuard guard(hot->device);
    hipStream_t st = (hipStream_t)stream;
    // 1) the lookup over both tiers serves every stored key and yields the present-before mask
    if (int rc = launch_find_grouped_tiered(hot, cold, d_keys, d_offsets, n, d_out, out_dtype, d_found, flags, st)) return rc;
    if (!creates) return MEE_OK;
    // 2) missing positions create their key in the tier their member was told (one creator per distinct key: the CAS decides) and return its initial row
    if (!admits) {
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto b16) {
            ensure_tiered_grouped_rows_kernel<b16><<<grid_for(n, 16, 8192), 256, 0, st>>>(hot->d_desc, hot->d_init, cold->d_desc, cold->d_init, hot->n_tables, d_offsets, d_keys, n, d_found,
                                                                                         d_to_cold, hot->dim4, (float4*)d_out);
        });
    } else {
        // 2a) every position in neither tier counts its key in its member's HOT sketch ...
        sketch_add_grouped_kernel<<<grid_for(n, 256, 4096), 256, 0, st>>>(hot->d_admit, hot->n_tables, d_offsets, 1, d_keys, n, d_found);
        // 2b) ... then the same creation, for the positions whose estimate reached their member's threshold
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto b16) {
            ensure_admit_tiered_grouped_rows_kernel<b16><<<grid_for(n, 16, 8192), 256, 0, st>>>(hot->d_desc, hot->d_init, cold->d_desc, cold->d_init, hot->d_admit, hot->n_tables, d_offsets,
                                                                                               d_keys, n, d_found, d_to_cold, hot->dim4, (float4*)d_out, admits->min_count,
                                                                                               admits->d_min_counts);
        });
    }
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

extern "C" int mee_group_ensure_admit_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                             const uint8_t* d_found, const uint8_t* d_to_cold, uint32_t min_count, const uint32_t* d_min_counts, void* stream) {
    MEE_RANGE("mee_group_ensure_admit_tiered");
    const char* name = "mee_group_ensure_admit_tiered";
    if (!hot || !cold || (bags_per_table && !d_bag_offsets) || (n && (!d_keys || !d_found))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = tiered_groups_check(hot, cold, 0, name)) return rc;
    if (int rc = group_admission_check(hot, name)) return rc;
    if (bags_per_table == 0 || n == 0) return MEE_OK;
    if (int rc = group_refresh(hot, stream)) return rc;
    if (int rc = group_refresh(cold, stream)) return rc;
    DeviceGuard guard(hot->device);
    hipStream_t st = (hipStream_t)stream;
    sketch_add_grouped_kernel<<<grid_for(n, 256, 4096), 256, 0, st>>>(hot->d_admit, hot->n_tables, d_bag_offsets, bags_per_table, d_keys, n, d_found);
    ensure_admit_tiered_grouped_kernel<<<grid_for(n, 16, 8192), 256, 0, st>>>(hot->d_desc, hot->d_init, cold->d_desc, cold->d_init, hot->d_admit, hot->n_tables, d_bag_offsets,
                                                                             bags_per_table, d_keys, n, d_found, d_to_cold, hot->dim4, min_count, d_min_counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

extern "C" {

int mee_group_find_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                          uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_tiered");
    return group_find_tiered_common(hot, cold, d_keys, d_offsets, n, d_out, out_dtype, d_found, false, nullptr, flags, stream, "mee_group_find_tiered");
}
int mee_group_find_or_insert_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                    uint8_t* d_found, const uint8_t* d_to_cold, uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_or_insert_tiered");
    return group_find_tiered_common(hot, cold, d_keys, d_offsets, n, d_out, out_dtype, d_found, true, d_to_cold, flags, stream, "mee_group_find_or_insert_tiered");
}
int mee_group_find_or_insert_admit_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                          uint8_t* d_found, const uint8_t* d_to_cold, uint32_t min_count, const uint32_t* d_min_counts, uint32_t flags, void* stream) {
    MEE_RANGE("mee_group_find_or_insert_admit_tiered");
    const TierAdmission admits{min_count, d_min_counts};
    return group_find_tiered_common(hot, cold, d_keys, d_offsets, n, d_out, out_dtype, d_found, true, d_to_cold, flags, stream, "mee_group_find_or_insert_admit_tiered",
                                    &admits);
}

int mee_find_grouped(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, float* d_out, uint8_t* d_found,
                     void* stream) {
    MEE_RANGE("mee_find_grouped");
    return find_grouped_common(g, d_keys, d_offsets, n, d_out, MEE_DTYPE_F32, d_found, stream, "mee_find_grouped");
}
int mee_find_grouped_as(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                        void* stream) {
    MEE_RANGE("mee_find_grouped_as");
    return find_grouped_common(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream, "mee_find_grouped_as");
}

int mee_group_find_or_insert(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, float* d_out, uint8_t* d_found,
                             void* stream) {
    MEE_RANGE("mee_group_find_or_insert");
    return group_find_or_insert_common(g, d_keys, d_offsets, n, d_out, MEE_DTYPE_F32, d_found, stream, "mee_group_find_or_insert");
}
int mee_group_find_or_insert_as(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                void* stream) {
    MEE_RANGE("mee_group_find_or_insert_as");
    return group_find_or_insert_common(g, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream, "mee_group_find_or_insert_as");
}

}  // extern "C"
