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

extern "C" {


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
