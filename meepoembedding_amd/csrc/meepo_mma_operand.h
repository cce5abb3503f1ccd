// meepo_mma_operand.h — what the kernels around v_mfma_f32_32x32x16_bf16 share about its operands: the search scans (meepo_search.hip), which feed it
// consecutive slots, and the shared-slate score (meepo_score.hip), which feeds it probed slots.  The B operand straight from a stored row, a chunk of a
// wide row through the matrix instruction, a norm's squares out of the operand registers, and the cosine arithmetic.  Device code only; every function
// is forced inline, and each is passed exactly as the scans have always passed it (their code generation is sensitive to that: meepo_search.hip).
#pragma once
#include "meepo_table_int.h"

namespace mee {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- cosine (SPEC.md §3 "Search", "Metric"): score = dot / (sqrtf(qq) * sqrtf(rr)), four correctly rounded fp32 operations ---------------------------
__device__ __forceinline__ float cosine_score(float dot, float qn, float rn) { return dot / (qn * rn) + 0.f; }   // + 0.f: a zero leaves as +0.0

// A lane's share of a norm: the squares of its eight bf16 elements of one k-step on top of `a`.  Every square is exact in fp32 (16 significant bits).
__device__ __forceinline__ float sum_squares(const u32x4 p, float a) {
    const uint32_t w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = __builtin_bit_cast(float, w[i] << 16), hi = __builtin_bit_cast(float, w[i] & 0xFFFF0000u);
        a = __builtin_fmaf(lo, lo, a);
        a = __builtin_fmaf(hi, hi, a);
    }
    return a;
}

// KS k-steps of the B operand from the lane's part of a row: b[s] = the eight elements at `at` + 16 s, as bf16 — one 16-byte load of a bf16 row, two and
// a round-and-pack of an fp32 row (`at` points at the stored elements: 2 or 4 bytes each).  A dead lane loads nothing and holds zeros; so does a k-step
// at or past n_ks (the short last chunk of a wide row; n_ks == KS elsewhere, and the test folds away).
template <int KS, int ROWS>
__device__ __forceinline__ void search_load_ksteps(const void* __restrict__ at, int n_ks, bool live, bf16x8 (&b)[KS]) {
    if constexpr (ROWS == kRowsBF16) {
        const u32x4* row = reinterpret_cast<const u32x4*>(at);
        u32x4 v[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) v[s] = live && s < n_ks ? __builtin_nontemporal_load(row + 2 * s) : u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int s = 0; s < KS; ++s) b[s] = __builtin_bit_cast(bf16x8, v[s]);
    } else {
        const f32x4* row = reinterpret_cast<const f32x4*>(at);
        f32x4 x[KS], y[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            x[s] = live && s < n_ks ? __builtin_nontemporal_load(row + 4 * s) : f32x4{0.f, 0.f, 0.f, 0.f};
            y[s] = live && s < n_ks ? __builtin_nontemporal_load(row + 4 * s + 1) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const u32x4 p = {bf16x2_of(x[s].x, x[s].y), bf16x2_of(x[s].z, x[s].w), bf16x2_of(y[s].x, y[s].y), bf16x2_of(y[s].z, y[s].w)};
            b[s] = __builtin_bit_cast(bf16x8, p);
        }
    }
}
// The B operand of a step: lane (half, col) holds elements [16 s + 8 half, + 8) of slot's row for k-step s, as bf16.  A dead lane loads nothing.
template <int KS, int ROWS>
__device__ __forceinline__ void search_load_b(const void* __restrict__ values, uint64_t slot, int half, bool live, bf16x8 (&b)[KS]) {
    if constexpr (ROWS == kRowsBF16) search_load_ksteps<KS, ROWS>(reinterpret_cast<const u32x4*>(values) + slot * (uint64_t)(2 * KS) + half, KS, live, b);   // a row is 2 KS groups of 16 bytes
    else search_load_ksteps<KS, ROWS>(reinterpret_cast<const f32x4*>(values) + slot * (uint64_t)(4 * KS) + 2 * half, KS, live, b);                             // ... 4 KS groups of four floats
}

// ---- wide rows, 256 < dim <= MEE_SEARCH_MAX_DIM: a row is walked in CHUNKS of kWideChunkKS k-steps (DESIGN.md §4 "Search", "Wide rows") -----------
constexpr int kWideChunkKS = 16;

// One chunk of a step: n_ks k-steps from k-step ks0 on (FULL: n_ks == kWideChunkKS, and no test of it is left in the code) of the row part at `at`
// into acc, the squares of the operand into rr (cosine).  The A fragments are the wide layout: fragment (ks, half) is nq x 16 bytes, query col at
// [col]; a lane whose col >= nq feeds zeros without an LDS read.
template <int ROWS, int METRIC, bool FULL>
__device__ __forceinline__ void search_wide_chunk(const void* __restrict__ at, const u32x4* afrag, uint32_t ks0, int n_ks, uint32_t nq, int half, int col, bool live,
                                                  f32x16& acc, float& rr) {
    bf16x8 b[kWideChunkKS];
    search_load_ksteps<kWideChunkKS, ROWS>(at, FULL ? kWideChunkKS : n_ks, live, b);
#pragma unroll
    for (int s = 0; s < kWideChunkKS; ++s) {
        if (FULL || s < n_ks) {   // wave-uniform: the fragments of a k-step past the row do not exist
            if constexpr (METRIC == MEE_METRIC_COSINE) rr = sum_squares(__builtin_bit_cast(u32x4, b[s]), rr);
            const u32x4 a = (uint32_t)col < nq ? afrag[((size_t)(ks0 + s) * 2 + half) * nq + col] : u32x4{0u, 0u, 0u, 0u};
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), b[s], acc, 0, 0, 0);
        }
    }
}

}  // namespace mee
