// meepo_score.hip — inner products of GIVEN candidate keys, probed in place (SPEC.md §3 "Score"): "how well do these ids match this query vector", the
// re-ranking step behind a search.  out[q][c] = score(q, keys[q][c]) = sum_j bf16(q_j) * bf16(row_j) — search's score, products exact, fp32 sum — or -inf
// for a key the table does not hold.  The hash probe, the row gather and the dot product are ONE launch: no [Q, C, dim] block is written or read back.
//
// Launch (DESIGN.md §4 "Score").  score_kernel<C4, ROWS>, C4 = ceil(dim / 64): a flat 1-D grid of four-wave blocks over UNITS; a unit is one query and
// one span of its slate, a block walks units blockIdx.x, + gridDim.x, ... (64-bit).  A wave step takes 4R consecutive candidates of the span, one 16-lane
// tile per key and R keys in flight per tile, in find_span's memory order: the 4R keys by one coalesced load and shuffles, the R bucket lines back to
// back (the shared read-only probe of meepo_device.h), then the R rows — straight-line where every position of the step is in range and found.
//   query    lane tl of every tile only ever touches element groups tl, 16 + tl, ... of a row, so it loads exactly those groups of its unit's query once,
//            rounds them to bf16 once and keeps them (as the fp32 values of the rounded bf16: at most 16 registers) for every key of the unit.  No LDS.
//   row      16-byte (fp32) or 8-byte (bf16) groups through RowType; an fp32 group is rounded to bf16 in registers as the search's operand load does,
//            a bf16 group is taken verbatim.  A lane whose last group lies past the row (dim not a multiple of 64) loads an address inside the row
//            instead — the load stays unconditional — and feeds zeros on both sides.
//   dot      one fp32 accumulator per key, fma of the rounded values (every product is exact), then the tile's 16 lanes by xor 8 / 4 / 2 / 1.
//   cosine   score_kernel<.., MEE_METRIC_COSINE> (mee_score_metric): a second accumulator per key, the row's squares, beside the dot product and through
//            the same shuffles; the query's squares once per unit from the kept values; then search's four operations, dot / (sqrtf(qq) * sqrtf(rr)).
//   stores   the 4R scores of a step reach lanes 0 .. 4R - 1 by shuffle and leave as one coalesced store, the found bytes likewise.
//   wide     256 < dim <= MEE_SEARCH_MAX_DIM: score_wide_kernel<P, ROWS, METRIC>, a whole wave per key and four keys per wave step (below).
// Only vector stores, no atomics, no LDS, nothing of the table is written (hit counters included).
//
// The upstream snapshot has no such operator; the semantics are SPEC.md §3 "Score".
#include <hip/hip_runtime.h>

#include "meepo_table_int.h"
#include "meepo_mma_operand.h"

namespace mee {

constexpr int kScoreWaves = 4;                // waves of a block: a block step is kScoreWaves wave steps
constexpr uint32_t kScoreBlocksPerCU = 8;     // the grid a span is sized for: this many blocks per CU, when the slates are large enough to give them
constexpr uint32_t kScoreMaxSpanSteps = 8;    // block steps of a span at most: 8 wave steps per wave behind one query load
constexpr uint32_t kScoreMaxGrid = 1u << 22;  // blocks at most (find's cap); more units than that are walked by the blocks' loops
// keys in flight per tile: a step's rows are R * C4 groups of registers per lane and leave no row stores behind, so a dim-64 step holds four keys
// where the find holds two
template <int C4> struct ScoreShape { static constexpr int R = C4 == 1 ? 4 : 2; };

// an element group of a stored row as the four fp32 values of its bf16 image: an fp32 row rounded once, ties to even; a bf16 row's bits as they are
template <int ROWS>
__device__ __forceinline__ f32x4 score_operand(const typename RowType<ROWS>::Group g) {
    if constexpr (ROWS == kRowsBF16) return widen_bf16x4(g);
    else return widen_bf16x4(bf16x4_of(g.x, g.y, g.z, g.w));
}

// the R rows of a wave step, group c of round r in row[r][c].  HIT: every slot is a row (the loads are unconditional and leave back to back);
// otherwise a tile without a row loads nothing and holds zeros.  last: the in-row index of the lane's last group (score_kernel).
template <int C4, int R, int ROWS, bool HIT>
__device__ __forceinline__ void score_load_rows(const typename RowType<ROWS>::Group* __restrict__ plane, const int64_t (&slot)[R], uint32_t dim4, int tl, uint32_t last,
                                                typename RowType<ROWS>::Group (&row)[R][C4]) {
    using RT = RowType<ROWS>;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint64_t first = RT::first(HIT || slot[r] >= 0 ? slot[r] : 0, dim4);
#pragma unroll
        for (int c = 0; c < C4; ++c) {
            const uint32_t g = c < C4 - 1 ? (uint32_t)(c * 16 + tl) : last;
            row[r][c] = (HIT || slot[r] >= 0) ? plane[first + g] : typename RT::Group{};
        }
    }
}

// the sum over a 16-lane tile, in every lane of it
__device__ __forceinline__ float score_tile_sum(float a) {
    a += __shfl_xor(a, 8); a += __shfl_xor(a, 4); a += __shfl_xor(a, 2); a += __shfl_xor(a, 1);   // (stays inside the 16-lane tile)
    return a;
}

// a group's four products, or its four squares, on top of `a`: every product is exact, the sum is fp32 in element order
__device__ __forceinline__ float dot4(const f32x4 x, const f32x4 y, float a) {
    a = __builtin_fmaf(x.x, y.x, a); a = __builtin_fmaf(x.y, y.y, a);
    a = __builtin_fmaf(x.z, y.z, a); a = __builtin_fmaf(x.w, y.w, a);
    return a;
}
__device__ __forceinline__ float squares4(const f32x4 v, float a) { return dot4(v, v, a); }

template <int C4, int ROWS, int METRIC>
__global__ __launch_bounds__(kScoreWaves * 64) void score_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t nb, uint32_t dim4,
                                                                 const f32x4* __restrict__ queries, const int64_t* __restrict__ keys, uint64_t n_cand, uint64_t span,
                                                                 uint64_t spans_per_query, uint64_t n_units, float* __restrict__ out, uint8_t* __restrict__ found) {
    using RT = RowType<ROWS>;
    constexpr int R = ScoreShape<C4>::R, KPW = 4 * R;
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15, wave = threadIdx.x >> 6;
    const typename RT::Group* __restrict__ plane = RT::plane(values);
    // The lane's element groups are c * 16 + tl, c < C4.  All but the last lie inside the row (16 (C4 - 1) < dim4); the last may not (dims 16, 32, 48:
    // 4, 8, 12 live lanes of a tile; dim 80: four lanes hold a second group).  Such a lane addresses the row's last group instead and multiplies zeros.
    const bool last_live = (uint32_t)((C4 - 1) * 16 + tl) < dim4;
    const uint32_t last = last_live ? (uint32_t)((C4 - 1) * 16 + tl) : dim4 - 1;

    for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {   // block-uniform
        const uint64_t q = unit / spans_per_query, c0 = (unit - q * spans_per_query) * span;
        const uint64_t c1 = n_cand - c0 < span ? n_cand : c0 + span;        // (c0 < n_cand: spans_per_query = ceil(n_cand / span))
        f32x4 qv[C4];
#pragma unroll
        for (int c = 0; c < C4; ++c) {
            const f32x4 x = queries[q * dim4 + (c < C4 - 1 ? (uint32_t)(c * 16 + tl) : last)];
            qv[c] = widen_bf16x4(bf16x4_of(x.x, x.y, x.z, x.w));
        }
        if (!last_live) qv[C4 - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float qn = 0.f;   // cosine: the query's norm, from the rounded values every tile holds
        if constexpr (METRIC == MEE_METRIC_COSINE) {
            float qq = 0.f;
#pragma unroll
            for (int c = 0; c < C4; ++c) qq = squares4(qv[c], qq);
            qn = __builtin_sqrtf(score_tile_sum(qq));
        }
        const int64_t* __restrict__ qkeys = keys + q * n_cand;
        float* __restrict__ qout = out + q * n_cand;
        uint8_t* __restrict__ qfound = found ? found + q * n_cand : nullptr;

        for (uint64_t base = c0 + (uint64_t)wave * KPW; base < c1; base += kScoreWaves * KPW) {   // wave-uniform
            int64_t key[R], slot[R], kb[R];
            uint64_t b[R];
            bool act[R];
            // one coalesced load brings the step's 4R keys; the tiles take theirs by shuffle (position base + 4 r + tile, as find_span)
            const int64_t kmine = (lane < KPW && base + lane < c1) ? qkeys[base + lane] : kEmpty;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                key[r] = __shfl(kmine, r * 4 + tile);
                act[r] = !reserved_key(key[r]);   // (a position past the span holds EMPTY)
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                b[r] = bucket_of(key[r], nb);
                kb[r] = act[r] ? tkeys[b[r] * kW + tl] : kEmpty;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys, nb, key[r], act[r], b[r], kb[r], tile, tl);

            // Common case, decided per wave: every position of the step is inside the span and was found — the R row requests are straight-line code
            // (find_span records what a per-lane condition around each load cost).  A slate with absent ids takes the other arm for that step only.
            typename RT::Group row[R][C4];
            bool all_hit = true;
#pragma unroll
            for (int r = 0; r < R; ++r) all_hit = all_hit && slot[r] >= 0;
            if (__all(all_hit)) score_load_rows<C4, R, ROWS, true>(plane, slot, dim4, tl, last, row);
            else score_load_rows<C4, R, ROWS, false>(plane, slot, dim4, tl, last, row);

            float sc[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                float a = 0.f;
                [[maybe_unused]] float rr = 0.f;
#pragma unroll
                for (int c = 0; c < C4; ++c) {
                    f32x4 v = score_operand<ROWS>(row[r][c]);
                    if (c == C4 - 1 && !last_live) v = f32x4{0.f, 0.f, 0.f, 0.f};
                    // dot4 / squares4 written out: through the helpers the four C4 == 1 instances (R = 4) are allocated other registers
                    a = __builtin_fmaf(qv[c].x, v.x, a); a = __builtin_fmaf(qv[c].y, v.y, a);
                    a = __builtin_fmaf(qv[c].z, v.z, a); a = __builtin_fmaf(qv[c].w, v.w, a);
                    if constexpr (METRIC == MEE_METRIC_COSINE) {
                        rr = __builtin_fmaf(v.x, v.x, rr); rr = __builtin_fmaf(v.y, v.y, rr);
                        rr = __builtin_fmaf(v.z, v.z, rr); rr = __builtin_fmaf(v.w, v.w, rr);
                    }
                }
                a += __shfl_xor(a, 8); a += __shfl_xor(a, 4); a += __shfl_xor(a, 2); a += __shfl_xor(a, 1);   // (stays inside the 16-lane tile)
                if constexpr (METRIC == MEE_METRIC_COSINE) a = a / (qn * __builtin_sqrtf(score_tile_sum(rr)));   // search's four operations; 0 / 0 = NaN is returned
                sc[r] = slot[r] >= 0 ? a + 0.f : -__builtin_inff();   // + 0.f: a zero leaves as +0.0, as the scan's does; a NaN stays a NaN
            }
            // lane j < 4R collects position base + j (round j / 4, tile j % 4): ONE coalesced store of the scores, one of the found bytes
            float smine = 0.f;
            int fmine = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float s = __shfl(sc[r], (lane & 3) * kW);
                const int f = __shfl((int)(slot[r] >= 0), (lane & 3) * kW);
                if ((lane >> 2) == r) { smine = s; fmine = f; }
            }
            if (lane < KPW && base + lane < c1) {
                qout[base + lane] = smine;
                if (qfound) qfound[base + lane] = (uint8_t)fmine;
            }
        }
    }
}

// ---- wide rows, 256 < dim <= MEE_SEARCH_MAX_DIM (DESIGN.md §4 "Score", "Wide rows") -------------------------------------------------------------
// score_wide_kernel<P, ROWS, METRIC>, P = ceil(dim / 256) in 2 .. 4: a row of 1 to 4 KB does not fit a 16-lane tile's registers R keys deep, so a WHOLE
// WAVE reduces one key.  A row is walked in P passes of 64 element groups, one group per lane and pass: lane l owns groups l, 64 + l, ... of every
// row and of its unit's query (P groups, rounded once, kept as fp32: at most 16 registers).  Units, spans, the step's keys and the probe are
// score_kernel's with one key per 16-lane tile: a wave step is 4 keys — one coalesced key load, the four bucket lines back to back, the shared
// read-only probe — then the four rows' 4 P groups are requested back to back by all 64 lanes (a pass is 1 KB of an fp32 row, contiguous), each key
// carries one dot accumulator (cosine: and one squares accumulator) through its passes, and a wave sum (xor 32 .. 1) ends it.  A lane whose group of
// the last pass lies past the row addresses the row's last group instead — the load stays unconditional — and feeds zeros on both sides.
// Stores as score_kernel: the step's four scores and found bytes leave lanes 0 .. 3 as one store each.  No LDS, no atomics.
__device__ __forceinline__ float score_wave_sum(float a) {
    a += __shfl_xor(a, 32); a += __shfl_xor(a, 16);
    return score_tile_sum(a);
}

template <int P, int ROWS, int METRIC>
__global__ __launch_bounds__(kScoreWaves * 64) void score_wide_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t nb, uint32_t dim4,
                                                                      const f32x4* __restrict__ queries, const int64_t* __restrict__ keys, uint64_t n_cand, uint64_t span,
                                                                      uint64_t spans_per_query, uint64_t n_units, float* __restrict__ out, uint8_t* __restrict__ found) {
    using RT = RowType<ROWS>;
    constexpr int KPW = 4;   // keys of a wave step: one per tile of the probe
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15, wave = threadIdx.x >> 6;
    const typename RT::Group* __restrict__ plane = RT::plane(values);
    // the lane's group of pass c is 64 c + lane; all but the last pass lie inside the row (64 (P - 1) < dim4 <= 64 P)
    const bool last_live = (uint32_t)((P - 1) * 64 + lane) < dim4;
    const uint32_t last = last_live ? (uint32_t)((P - 1) * 64 + lane) : dim4 - 1;

    for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {   // block-uniform
        const uint64_t q = unit / spans_per_query, c0 = (unit - q * spans_per_query) * span;
        const uint64_t c1 = n_cand - c0 < span ? n_cand : c0 + span;
        f32x4 qv[P];
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const f32x4 x = queries[q * dim4 + (c < P - 1 ? (uint32_t)(c * 64 + lane) : last)];
            qv[c] = widen_bf16x4(bf16x4_of(x.x, x.y, x.z, x.w));
        }
        if (!last_live) qv[P - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] float qn = 0.f;   // cosine: the query's norm, from the rounded values
        if constexpr (METRIC == MEE_METRIC_COSINE) {
            float qq = 0.f;
#pragma unroll
            for (int c = 0; c < P; ++c) qq = squares4(qv[c], qq);
            qn = __builtin_sqrtf(score_wave_sum(qq));
        }
        const int64_t* __restrict__ qkeys = keys + q * n_cand;
        float* __restrict__ qout = out + q * n_cand;
        uint8_t* __restrict__ qfound = found ? found + q * n_cand : nullptr;

        for (uint64_t base = c0 + (uint64_t)wave * KPW; base < c1; base += kScoreWaves * KPW) {   // wave-uniform
            // tile t probes position base + t, as score_kernel's round 0
            const int64_t kmine = (lane < KPW && base + lane < c1) ? qkeys[base + lane] : kEmpty;
            const int64_t key = __shfl(kmine, tile);
            const bool act = !reserved_key(key);   // (a position past the span holds EMPTY)
            const uint64_t b = bucket_of(key, nb);
            const int64_t kb = act ? tkeys[b * kW + tl] : kEmpty;
            const int64_t probed = tile_probe(tkeys, nb, key, act, b, kb, tile, tl);
            int64_t slot[KPW];   // every lane learns the four slots: the whole wave walks each row
#pragma unroll
            for (int r = 0; r < KPW; ++r) slot[r] = __shfl(probed, r * kW);

            typename RT::Group row[KPW][P];
            const bool all_hit = slot[0] >= 0 && slot[1] >= 0 && slot[2] >= 0 && slot[3] >= 0;   // wave-uniform
#pragma unroll
            for (int r = 0; r < KPW; ++r) {
                const uint64_t first = RT::first(all_hit || slot[r] >= 0 ? slot[r] : 0, dim4);
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    const uint32_t g = c < P - 1 ? (uint32_t)(c * 64 + lane) : last;
                    row[r][c] = (all_hit || slot[r] >= 0) ? plane[first + g] : typename RT::Group{};
                }
            }

            float smine = 0.f;
            int fmine = 0;
#pragma unroll
            for (int r = 0; r < KPW; ++r) {
                float a = 0.f;
                [[maybe_unused]] float rr = 0.f;
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    f32x4 v = score_operand<ROWS>(row[r][c]);
                    if (c == P - 1 && !last_live) v = f32x4{0.f, 0.f, 0.f, 0.f};
                    a = dot4(qv[c], v, a);
                    if constexpr (METRIC == MEE_METRIC_COSINE) rr = squares4(v, rr);
                }
                a = score_wave_sum(a);
                if constexpr (METRIC == MEE_METRIC_COSINE) a = a / (qn * __builtin_sqrtf(score_wave_sum(rr)));   // search's four operations; 0 / 0 = NaN is returned
                if (lane == r) { smine = slot[r] >= 0 ? a + 0.f : -__builtin_inff(); fmine = slot[r] >= 0; }   // + 0.f: a zero leaves as +0.0; a NaN stays a NaN
            }
            if (lane < KPW && base + lane < c1) {
                qout[base + lane] = smine;
                if (qfound) qfound[base + lane] = (uint8_t)fmine;
            }
        }
    }
}

// ---- a shared slate: every query against the SAME keys (SPEC.md §3 "Score", "Shared slate"; DESIGN.md §4 "Score", "Shared slate") ----------------
// out[q][c] = score(q, keys[c]) is a matrix product once a key's row is in registers, so the row bytes are paid once per QUERY TILE, not once per
// query: the scan's operand loop (meepo_mma_operand.h) fed by probed slots, writing a dense block.
//   units    the queries in tiles that fit the LDS as rounded bf16 fragments (shared_tile), the keys in spans of whole block steps; a block of
//            kSharedWaves waves serves (tile, span) pairs blockIdx.x, + gridDim.x, ..., the tile index fastest: the blocks that gather one span's rows
//            are neighbours in time.  The tile is staged once per unit in fragment order, with the queries' norms (cosine).
//   step     a wave takes 32 consecutive keys of the span — the 32 columns of v_mfma_f32_32x32x16_bf16: one coalesced key load, eight probe rounds
//            of four keys (one 16-lane tile each, the shared read-only probe) with the eight bucket lines requested back to back, the slots handed
//            round by shuffle so that lane (half, col) holds the slot of key col.
//   B        the lane's part of ITS key's row, exactly as the scan loads a slot's (search_load_b / search_wide_chunk); an absent key loads nothing
//            and holds zeros; a step whose 32 keys were all found takes straight-line loads (wave-uniform).
//   product  narrow rows: B stays in registers for every row block of 32 queries of the tile.  Wide rows: a tile is one row block, the row is walked
//            in chunks of kWideChunkKS k-steps, one chunk of B live at a time.
//   stores   accumulator i of lane (half, col) is query 32 rb + 8 (i / 4) + 4 half + i % 4 against key col: each accumulator index leaves as two
//            runs of 32 consecutive floats, one per half.  -inf for an absent key, + 0.f on a real score, a NaN as it is.  found[c]: the first tile's
//            blocks.  Cosine: rr from the B registers, the other half's share by shuffle; the exact four operations per output.
// Vector stores only, no atomics, nothing of the table is written.
constexpr int kSharedWaves = 8;                    // waves of a block: they share one staged query tile
constexpr int kSharedWideWaves = 4;                // ... of a wide row's block: a chunk of an fp32 row in flight needs more than the 256 registers of an 8-wave block's lane
constexpr uint32_t kSharedLdsBudget = 64 * 1024;   // A fragments and norms of a tile: two blocks fit a CU's 160 KB — and its registers up to 128 VGPRs
constexpr uint32_t kSharedMaxSpanSteps = 16;       // block steps of a span at most, behind one staging of the tile
// the queries of a tile: what the budget holds at dim * 2 bytes of fragments and one norm each — whole row blocks of a narrow row (at least one: 8.3 KB
// at dim 256), one row block at most, in eights, of a wide row (24 queries at dim 1024)
__host__ __device__ constexpr uint32_t shared_tile(uint32_t dim) {
    const uint32_t fit = kSharedLdsBudget / (dim * 2 + 4);
    return dim <= 256 ? fit / 32 * 32 : (fit < 32 ? fit / 8 * 8 : 32);
}
static_assert(shared_tile(256) >= 32 && shared_tile(MEE_SEARCH_MAX_DIM) >= 8, "every dim is served in tiles of at least 8 queries");

// A step's 32 keys [base, base + 32) below c1 probed: the slot of key base + col (or -1) in lanes (0, col) and (1, col).  All 64 lanes, convergent.
__device__ __forceinline__ int64_t shared_probe_step(const int64_t* __restrict__ tkeys, uint64_t nb, const int64_t* __restrict__ keys, uint64_t base, uint64_t c1, int lane) {
    constexpr int R = 8;   // rounds: four keys each, key 4 r + tile by tile `tile`
    const int tile = lane >> 4, tl = lane & 15, col = lane & 31;
    const int64_t kmine = (lane < 32 && base + lane < c1) ? keys[base + lane] : kEmpty;
    int64_t key[R], kb[R], slot[R];
    uint64_t b[R];
    bool act[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        key[r] = __shfl(kmine, r * 4 + tile);
        act[r] = !reserved_key(key[r]);   // (a position past the span holds EMPTY)
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        b[r] = bucket_of(key[r], nb);
        kb[r] = act[r] ? tkeys[b[r] * kW + tl] : kEmpty;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys, nb, key[r], act[r], b[r], kb[r], tile, tl);
    int64_t mine = -1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t v = __shfl(slot[r], (col & 3) * kW);
        if ((col >> 2) == r) mine = v;
    }
    return mine;
}

// The 16 accumulators of a row block leave: accumulator i is query qb + 8 (i / 4) + i % 4 of the tile (qb = 32 rb + 4 half) against the lane's key,
// out points at the tile's first row and the key's column.  rn (cosine): the row's norm; qn: the tile's norms in LDS.
template <int METRIC>
__device__ __forceinline__ void shared_store(const f32x16& acc, uint32_t qb, uint32_t nq, bool in_span, bool live, [[maybe_unused]] float rn,
                                             [[maybe_unused]] const float* qn, float* __restrict__ out, uint64_t n_cand) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const uint32_t q = qb + 8 * (i >> 2) + (i & 3);
        float s = acc[i];
        if constexpr (METRIC == MEE_METRIC_COSINE) s = cosine_score(s, qn[q < nq ? q : 0], rn);   // the four operations; 0 / 0 = NaN is returned
        else s += 0.f;                                                                            // a zero leaves as +0.0; a NaN stays a NaN
        if (in_span && q < nq) __builtin_nontemporal_store(live ? s : -__builtin_inff(), out + (uint64_t)q * n_cand);
    }
}

// what the two kernels' blocks share per unit: the unit's tile and span
struct SharedUnit { uint64_t q0; uint32_t nq; uint64_t c0, c1; bool first_tile; };
__device__ __forceinline__ SharedUnit shared_unit(uint64_t unit, uint64_t nq_all, uint32_t tile, uint64_t n_tiles, uint64_t n_cand, uint64_t span) {
    const uint64_t t = unit % n_tiles, sp = unit / n_tiles;
    SharedUnit u;
    u.q0 = t * tile;
    u.nq = nq_all - u.q0 < tile ? (uint32_t)(nq_all - u.q0) : tile;
    u.c0 = sp * span;
    u.c1 = n_cand - u.c0 < span ? n_cand : u.c0 + span;   // (c0 < n_cand: the spans are ceil(n_cand / span))
    u.first_tile = t == 0;
    return u;
}

// rows of dim = 16 KS <= 256.  LDS (dynamic): A fragments [n_rb][KS][64] x 16 B, the scan's layout | qn [32 n_rb]
template <int KS, int ROWS, int METRIC>
__global__ __launch_bounds__(kSharedWaves * 64) void score_shared_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t nb,
                                                                          const float* __restrict__ queries, uint64_t nq_all, uint32_t tile, uint64_t n_tiles,
                                                                          const int64_t* __restrict__ keys, uint64_t n_cand, uint64_t span, uint64_t n_units,
                                                                          float* __restrict__ out, uint8_t* __restrict__ found) {
    extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
    constexpr uint32_t dim = 16 * KS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    u32x4* const afrag = reinterpret_cast<u32x4*>(score_lds);

    for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {   // block-uniform
        const SharedUnit u = shared_unit(unit, nq_all, tile, n_tiles, n_cand, span);
        const uint32_t n_rb = (u.nq + 31) / 32;
        float* const qn = reinterpret_cast<float*>(score_lds + (size_t)n_rb * 32 * dim * 2);
        if (unit != blockIdx.x) __syncthreads();   // the previous unit's fragments are still being read
        // ---- the tile's queries, rounded once, in fragment order: a wave stages whole row blocks, so a query's norm is one lane pair's sum
        for (uint32_t rb = wave; rb < n_rb; rb += kSharedWaves) {
            const uint32_t q = rb * 32 + col;
            const f32x4* src = reinterpret_cast<const f32x4*>(queries + (u.q0 + (q < u.nq ? q : 0)) * dim + 8 * half);
            [[maybe_unused]] float qq = 0.f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                u32x4 p = {0u, 0u, 0u, 0u};
                if (q < u.nq) {
                    const f32x4 x = src[4 * ks], y = src[4 * ks + 1];
                    p = u32x4{bf16x2_of(x.x, x.y), bf16x2_of(x.z, x.w), bf16x2_of(y.x, y.y), bf16x2_of(y.z, y.w)};
                }
                afrag[(rb * KS + ks) * 64 + lane] = p;
                if constexpr (METRIC == MEE_METRIC_COSINE) qq = sum_squares(p, qq);
            }
            if constexpr (METRIC == MEE_METRIC_COSINE) {
                qq += __shfl_xor(qq, 32);
                if (half == 0) qn[q] = __builtin_sqrtf(qq);   // (a padding query: 0, never used)
            }
        }
        __syncthreads();

        for (uint64_t base = u.c0 + (uint64_t)wave * 32; base < u.c1; base += kSharedWaves * 32) {   // wave-uniform
            const int64_t slot = shared_probe_step(tkeys, nb, keys, base, u.c1, lane);
            const bool live = slot >= 0, in_span = base + col < u.c1;
            bf16x8 b[KS];
            if (__all(live)) search_load_b<KS, ROWS>(values, (uint64_t)slot, half, true, b);   // the common step: straight-line loads
            else search_load_b<KS, ROWS>(values, (uint64_t)slot, half, live, b);
            [[maybe_unused]] float rn = 0.f;
            if constexpr (METRIC == MEE_METRIC_COSINE) {   // the lane's eight elements of every k-step, then the other half's
                float rr = 0.f;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) rr = sum_squares(__builtin_bit_cast(u32x4, b[ks]), rr);
                rr += __shfl_xor(rr, 32);
                rn = __builtin_sqrtf(rr);
            }
            if (u.first_tile && found && half == 0 && in_span) found[base + col] = (uint8_t)live;
            float* const o = out + u.q0 * n_cand + base + col;
            for (uint32_t rb = 0; rb < n_rb; ++rb) {
                f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, afrag[(rb * KS + ks) * 64 + lane]), b[ks], acc, 0, 0, 0);
                shared_store<METRIC>(acc, rb * 32 + 4 * half, u.nq, in_span, live, rn, qn, o, n_cand);
            }
        }
    }
}

// rows of 256 < dim <= MEE_SEARCH_MAX_DIM: tile <= 32 queries, one row block.  LDS (dynamic): A fragments [dim / 16][2][nq] x 16 B, the wide scan's
// layout (search_wide_chunk reads it) | qn [32]
template <int ROWS, int METRIC>
__global__ __launch_bounds__(kSharedWideWaves * 64) void score_shared_wide_kernel(const int64_t* __restrict__ tkeys, const void* __restrict__ values, uint64_t nb, uint32_t dim,
                                                                               const float* __restrict__ queries, uint64_t nq_all, uint32_t tile, uint64_t n_tiles,
                                                                               const int64_t* __restrict__ keys, uint64_t n_cand, uint64_t span, uint64_t n_units,
                                                                               float* __restrict__ out, uint8_t* __restrict__ found) {
    extern __shared__ __attribute__((aligned(16))) unsigned char score_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
    const uint32_t ks_all = dim / 16, n_full = ks_all / kWideChunkKS * kWideChunkKS;
    constexpr uint32_t esz = ROWS == kRowsBF16 ? 2 : 4;   // bytes of a stored element
    u32x4* const afrag = reinterpret_cast<u32x4*>(score_lds);

    for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {   // block-uniform
        const SharedUnit u = shared_unit(unit, nq_all, tile, n_tiles, n_cand, span);
        const uint32_t nq = u.nq;
        float* const qn = reinterpret_cast<float*>(score_lds + (size_t)nq * dim * 2);
        if (unit != blockIdx.x) __syncthreads();   // the previous unit's fragments are still being read
        // ---- the tile's queries, rounded once: wave w stages k-steps w, w + kSharedWideWaves, ...
        if ((uint32_t)col < nq) {
            const f32x4* src = reinterpret_cast<const f32x4*>(queries + (u.q0 + col) * dim + 8 * half);
            for (uint32_t ks = wave; ks < ks_all; ks += kSharedWideWaves) {
                const f32x4 x = src[4 * ks], y = src[4 * ks + 1];
                afrag[((size_t)ks * 2 + half) * nq + col] = u32x4{bf16x2_of(x.x, x.y), bf16x2_of(x.z, x.w), bf16x2_of(y.x, y.y), bf16x2_of(y.z, y.w)};
            }
        }
        __syncthreads();
        if constexpr (METRIC == MEE_METRIC_COSINE) {   // the norms from the staged fragments, by one wave in k-step order
            if (wave == 0) {
                float qq = 0.f;
                if ((uint32_t)col < nq)
                    for (uint32_t ks = 0; ks < ks_all; ++ks) qq = sum_squares(afrag[((size_t)ks * 2 + half) * nq + col], qq);
                qq += __shfl_xor(qq, 32);
                if (half == 0) qn[col] = __builtin_sqrtf(qq);   // (a padding query: 0, never used)
            }
            __syncthreads();
        }

        for (uint64_t base = u.c0 + (uint64_t)wave * 32; base < u.c1; base += kSharedWideWaves * 32) {   // wave-uniform
            const int64_t slot = shared_probe_step(tkeys, nb, keys, base, u.c1, lane);
            const bool live = slot >= 0, in_span = base + col < u.c1;
            const unsigned char* const row = reinterpret_cast<const unsigned char*>(values) + ((uint64_t)slot * dim + 8 * half) * esz;   // the lane's eight elements of k-step 0
            f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float rr = 0.f;
            if (__all(live)) {   // the common step: straight-line loads
#pragma unroll 1
                for (uint32_t ks0 = 0; ks0 < n_full; ks0 += kWideChunkKS)
                    search_wide_chunk<ROWS, METRIC, true>(row + (size_t)ks0 * 16 * esz, afrag, ks0, kWideChunkKS, nq, half, col, true, acc, rr);
                if (n_full < ks_all)
                    search_wide_chunk<ROWS, METRIC, false>(row + (size_t)n_full * 16 * esz, afrag, n_full, (int)(ks_all - n_full), nq, half, col, true, acc, rr);
            } else {
#pragma unroll 1
                for (uint32_t ks0 = 0; ks0 < n_full; ks0 += kWideChunkKS)
                    search_wide_chunk<ROWS, METRIC, true>(row + (size_t)ks0 * 16 * esz, afrag, ks0, kWideChunkKS, nq, half, col, live, acc, rr);
                if (n_full < ks_all)
                    search_wide_chunk<ROWS, METRIC, false>(row + (size_t)n_full * 16 * esz, afrag, n_full, (int)(ks_all - n_full), nq, half, col, live, acc, rr);
            }
            [[maybe_unused]] float rn = 0.f;
            if constexpr (METRIC == MEE_METRIC_COSINE) {
                rr += __shfl_xor(rr, 32);
                rn = __builtin_sqrtf(rr);
            }
            if (u.first_tile && found && half == 0 && in_span) found[base + col] = (uint8_t)live;
            shared_store<METRIC>(acc, 4 * half, nq, in_span, live, rn, qn, out + u.q0 * n_cand + base + col, n_cand);
        }
    }
}

}  // namespace mee

using namespace mee;

// mee_score and mee_score_metric: one check, one launch plan, the kernel of the metric
template <int METRIC>
static int score_launch(const mee_table* t, const float* d_queries, size_t n_queries, const int64_t* d_keys, size_t n_cand, float* d_out_scores, uint8_t* d_out_found,
                        void* stream, const char* name) {
    if (!t) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (t->dim % 16 || t->dim < 16 || t->dim > MEE_SEARCH_MAX_DIM)
        return fail(MEE_ERR_INVALID_ARG, "%s: dim must be a multiple of 16 in [16, %d] (got %u)", name, MEE_SEARCH_MAX_DIM, t->dim);
    if (int rc = refuse_narrow_rows(t, name, false)) return rc;
    if (n_queries == 0 || n_cand == 0) return MEE_OK;   // as mee_find's n == 0
    if (!d_queries || !d_keys || !d_out_scores) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (((uintptr_t)d_queries & 15) || ((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_scores & 3))
        return fail(MEE_ERR_INVALID_ARG, "%s: queries must be 16-byte aligned, keys 8-byte aligned, scores 4-byte aligned", name);
    if (n_cand > (SIZE_MAX >> 4) / n_queries) return fail(MEE_ERR_INVALID_ARG, "%s: n_queries * n_cand = %zu * %zu does not fit", name, n_queries, n_cand);
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    // A span is a whole number of block steps: as many as leave the device kScoreBlocksPerCU blocks per CU, at least one (a small Q * C spreads
    // over as many blocks as it has block steps), at most kScoreMaxSpanSteps and no more than a slate has.  launch(span, spans_per_query, n_units, grid)
    auto spans = [&](uint64_t block_step, auto launch) {
        const uint64_t steps_per_query = (n_cand + block_step - 1) / block_step;
        uint64_t span_steps = (uint64_t)n_queries * steps_per_query / ((uint64_t)cus * kScoreBlocksPerCU);
        span_steps = span_steps < 1 ? 1 : span_steps > kScoreMaxSpanSteps ? kScoreMaxSpanSteps : span_steps;
        if (span_steps > steps_per_query) span_steps = steps_per_query;
        const uint64_t span = span_steps * block_step, spans_per_query = (n_cand + span - 1) / span, n_units = (uint64_t)n_queries * spans_per_query;
        launch(span, spans_per_query, n_units, n_units < kScoreMaxGrid ? (uint32_t)n_units : kScoreMaxGrid);
    };
    if (t->dim > 256) with_value<2, 3, 4>((int)((t->dim + 255) / 256), [&](auto p) { with_flag(t->bf16_rows, [&](auto bf16) {   // a wave per key, four keys per wave step
        spans((uint64_t)kScoreWaves * 4, [&](uint64_t span, uint64_t spans_per_query, uint64_t n_units, uint32_t grid) {
            score_wide_kernel<p, bf16 ? kRowsBF16 : kRowsF32, METRIC><<<grid, kScoreWaves * 64, 0, st>>>(t->keys, t->values, t->nb, t->dim4, (const f32x4*)d_queries, d_keys, n_cand,
                                                                                                      span, spans_per_query, n_units, d_out_scores, d_out_found);
        });
    }); });
    else with_value<1, 2, 3, 4>((int)((t->dim + 63) / 64), [&](auto c4) { with_flag(t->bf16_rows, [&](auto bf16) {
        spans((uint64_t)kScoreWaves * 4 * ScoreShape<c4>::R, [&](uint64_t span, uint64_t spans_per_query, uint64_t n_units, uint32_t grid) {
            score_kernel<c4, bf16 ? kRowsBF16 : kRowsF32, METRIC><<<grid, kScoreWaves * 64, 0, st>>>(t->keys, t->values, t->nb, t->dim4, (const f32x4*)d_queries, d_keys, n_cand, span,
                                                                                                  spans_per_query, n_units, d_out_scores, d_out_found);
        });
    }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// mee_score_shared: score_launch's checks, then (tile, span) units over the one slate
template <int METRIC>
static int score_shared_launch(const mee_table* t, const float* d_queries, size_t n_queries, const int64_t* d_keys, size_t n_cand, float* d_out_scores,
                               uint8_t* d_out_found, void* stream) {
    const char* const name = "mee_score_shared";
    if (!t) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (t->dim % 16 || t->dim < 16 || t->dim > MEE_SEARCH_MAX_DIM)
        return fail(MEE_ERR_INVALID_ARG, "%s: dim must be a multiple of 16 in [16, %d] (got %u)", name, MEE_SEARCH_MAX_DIM, t->dim);
    if (int rc = refuse_narrow_rows(t, name, false)) return rc;
    if (n_queries == 0 || n_cand == 0) return MEE_OK;   // as mee_find's n == 0
    if (!d_queries || !d_keys || !d_out_scores) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (((uintptr_t)d_queries & 15) || ((uintptr_t)d_keys & 7) || ((uintptr_t)d_out_scores & 3))
        return fail(MEE_ERR_INVALID_ARG, "%s: queries must be 16-byte aligned, keys 8-byte aligned, scores 4-byte aligned", name);
    if (n_cand > (SIZE_MAX >> 4) / n_queries) return fail(MEE_ERR_INVALID_ARG, "%s: n_queries * n_cand = %zu * %zu does not fit", name, n_queries, n_cand);
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) != hipSuccess || cus <= 0) cus = 256;
    const int waves = t->dim > 256 ? kSharedWideWaves : kSharedWaves;
    const uint64_t block_step = (uint64_t)waves * 32;
    const uint64_t steps = (n_cand + block_step - 1) / block_step;
    // The tile: as many queries as the LDS holds — the slate's rows are gathered once per tile.  A slate too short to give every CU a block at
    // that tile is served in smaller tiles of whole row blocks (its rows then come from the L2 the neighbouring blocks share).
    uint32_t tile = shared_tile(t->dim);
    if (t->dim <= 256) {
        const uint64_t want = ((uint64_t)cus + steps - 1) / steps;           // tiles that give every CU a block
        const uint64_t fair = ((n_queries + want - 1) / want + 31) / 32 * 32;   // queries of such a tile, in row blocks
        if (fair < tile) tile = (uint32_t)fair;
    }
    const uint64_t n_tiles = (n_queries + tile - 1) / tile;
    // A span is a whole number of block steps, sized as score_launch sizes it, for two blocks per CU: what the LDS holds, and what the registers hold
    // of an instance up to 128 VGPRs.  The wider instances (fp32 rows from dim 144, cosine 112; bf16 rows from dim 208, cosine 192; the wide fp32 kernel) keep ONE block
    // resident per CU and run this grid as two rounds of blocks
    uint64_t span_steps = n_tiles * steps / ((uint64_t)cus * 2);
    span_steps = span_steps < 1 ? 1 : span_steps > kSharedMaxSpanSteps ? kSharedMaxSpanSteps : span_steps;
    if (span_steps > steps) span_steps = steps;
    const uint64_t span = span_steps * block_step, n_units = n_tiles * ((n_cand + span - 1) / span);
    const uint32_t grid = n_units < kScoreMaxGrid ? (uint32_t)n_units : kScoreMaxGrid;
    const size_t lds = (size_t)tile * t->dim * 2 + (t->dim <= 256 ? tile : 32) * sizeof(float);
    with_flag(t->bf16_rows, [&](auto bf16) {
        constexpr int ROWS = bf16 ? kRowsBF16 : kRowsF32;
        if (t->dim > 256)
            score_shared_wide_kernel<ROWS, METRIC><<<grid, kSharedWideWaves * 64, lds, st>>>(t->keys, t->values, t->nb, t->dim, d_queries, n_queries, tile, n_tiles, d_keys, n_cand, span,
                                                                                        n_units, d_out_scores, d_out_found);
        else with_value<1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>((int)(t->dim / 16), [&](auto ks) {
            score_shared_kernel<ks, ROWS, METRIC><<<grid, kSharedWaves * 64, lds, st>>>(t->keys, t->values, t->nb, d_queries, n_queries, tile, n_tiles, d_keys, n_cand, span, n_units,
                                                                                       d_out_scores, d_out_found);
        });
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

extern "C" {

int mee_score_shared(const mee_table* t, int metric, const float* d_queries, size_t n_queries, const int64_t* d_keys, size_t n_cand, float* d_out_scores,
                     uint8_t* d_out_found, void* stream) {
    if (metric != MEE_METRIC_IP && metric != MEE_METRIC_COSINE)
        return fail(MEE_ERR_INVALID_ARG, "mee_score_shared: metric must be MEE_METRIC_IP (0) or MEE_METRIC_COSINE (1) (got %d)", metric);
    MEE_RANGE("mee_score_shared");
    if (metric == MEE_METRIC_IP) return score_shared_launch<MEE_METRIC_IP>(t, d_queries, n_queries, d_keys, n_cand, d_out_scores, d_out_found, stream);
    return score_shared_launch<MEE_METRIC_COSINE>(t, d_queries, n_queries, d_keys, n_cand, d_out_scores, d_out_found, stream);
}

int mee_score(const mee_table* t, const float* d_queries, size_t n_queries, const int64_t* d_keys, size_t n_cand, float* d_out_scores, uint8_t* d_out_found,
              void* stream) {
    MEE_RANGE("mee_score");
    return score_launch<MEE_METRIC_IP>(t, d_queries, n_queries, d_keys, n_cand, d_out_scores, d_out_found, stream, "mee_score");
}

int mee_score_metric(const mee_table* t, int metric, const float* d_queries, size_t n_queries, const int64_t* d_keys, size_t n_cand, float* d_out_scores,
                     uint8_t* d_out_found, void* stream) {
    if (metric == MEE_METRIC_IP) return mee_score(t, d_queries, n_queries, d_keys, n_cand, d_out_scores, d_out_found, stream);
    if (metric != MEE_METRIC_COSINE) return fail(MEE_ERR_INVALID_ARG, "mee_score_metric: metric must be MEE_METRIC_IP (0) or MEE_METRIC_COSINE (1) (got %d)", metric);
    MEE_RANGE("mee_score_metric");
    return score_launch<MEE_METRIC_COSINE>(t, d_queries, n_queries, d_keys, n_cand, d_out_scores, d_out_found, stream, "mee_score_metric");
}

}  // extern "C"
