// meepo_pool_max.hip — max pooling for embedding bags (SPEC.md §3 "find_pooled_max"): one table or a uniform group, fp32 rows; the lookup and its backward,
// one launch each.  out[b, j] = the maximum over bag b's positions of row[p][j], argmax[b, j] = the batch position that holds it.  No arithmetic touches a
// value: what leaves is a copy of a stored (or default) element, so there is nothing to round in fp32.
#include <hip/hip_runtime.h>

#include "meepo_table_int.h"

namespace mee {

constexpr uint32_t kNoArgmax = 0xFFFFFFFFu;   // the argmax of an empty bag

// One element group of the row at batch position p meets the running maximum.  The rule is the sequential scan's: the bag's first row is ASSIGNED (a NaN
// there stays, -0.0 stays), a later element replaces the running one iff it is greater by the IEEE comparison — so the first of equal values wins, +0.0 behind
// -0.0 does not replace it, and a NaN behind the first position is never taken.  Compare and select only: the bits are the row's.
template <bool ARGMAX>
__device__ __forceinline__ void pooled_max_take(float4& m, u32x4& a, float4 v, uint32_t p, bool first) {
    const bool tx = first || v.x > m.x, ty = first || v.y > m.y, tz = first || v.z > m.z, tw = first || v.w > m.w;
    m.x = tx ? v.x : m.x; m.y = ty ? v.y : m.y; m.z = tz ? v.z : m.z; m.w = tw ? v.w : m.w;
    if constexpr (ARGMAX) { a.x = tx ? p : a.x; a.y = ty ? p : a.y; a.z = tz ? p : a.z; a.w = tw ? p : a.w; }
}

// the finished element groups C0 .. C0 + CN - 1 of a bag go to out[o ...] (a bf16 row is rounded here, once) and, with ARGMAX, one 16-byte index group per
// lane beside each: argmax is [n_bags, dim] uint32, so group g of bag b has the index it has in an fp32 `out`
template <int DIM4, int C0, int CN, bool BF16, bool ARGMAX>
__device__ __forceinline__ void pooled_max_store(void* __restrict__ out, uint32_t* __restrict__ argmax, uint64_t o, const float4 (&m)[CN], const u32x4 (&a)[CN],
                                                 uint32_t dim4, int tl) {
#pragma unroll
    for (int k = 0; k < CN; ++k)
        if (DIM4 != 0 || (uint32_t)((C0 + k) * 16 + tl) < dim4) {
            const uint64_t idx = o + (uint32_t)((C0 + k) * 16 + tl);
            if constexpr (BF16) store_bf16x4<true>(out, idx, m[k]); else reinterpret_cast<float4*>(out)[idx] = m[k];
            if constexpr (ARGMAX) reinterpret_cast<u32x4*>(argmax)[idx] = a[k];
        }
}

// The bags one wave serves in one step, in the geometry of pooled_bags (meepo_device.h) and from its pieces: a tile per short bag, the four tiles together on
// a long one — every tile consumes the round's 4U rows in position order out of the other tiles' registers, so all four keep the same running maximum and
// index — or (BPW = 1) the wave on bag0 whatever its length.  The combine and the store are this file's.
// C = the float4 per lane per row that pooled_fetch is asked for; this call keeps the maximum of the groups C0 .. C0 + CN - 1 of them.  The compiled row shapes
// keep all (C0 = 0, CN = C).  The run-time shape (C = 16) would need 64 VGPRs of running maxima and 64 of indices next to the 64 of a row: its kernel walks
// a bag once per chunk of four groups (256 elements) instead, probing again for every chunk beyond the first — rows of up to 256 elements pay nothing for it —
// and a chunk's walk never reads the groups outside it, so their loads are not issued.  found is written by the first chunk's walk (nullptr for the others).
template <int DIM4, int U, int BPW, int C, int C0, int CN, bool BF16, bool ARGMAX, class TableOf>
__device__ __forceinline__ void pooled_max_bags(uint64_t bag0, uint32_t nvalid, uint32_t dim4, const int64_t* __restrict__ keys, const uint64_t* __restrict__ offsets,
                                                uint64_t n_keys, void* __restrict__ out, uint8_t* __restrict__ found, uint32_t* __restrict__ argmax, int tile, int tl,
                                                TableOf&& table_of) {
    static_assert(C0 + CN <= C, "the chunk lies inside the row");
    const uint64_t bag = BPW == 4 ? bag0 + tile : bag0;
    const bool has = BPW == 4 ? (uint32_t)tile < nvalid : true;
    uint64_t begin, end;
    pooled_span(offsets, bag, has, n_keys, begin, end);
    PooledTable t;
    table_of(has ? bag : bag0, t);
    const bool is_long = BPW == 1 || end - begin >= kPoolLong;
    float4 m[CN];
    u32x4 a[CN];
    float4 row[U][C];
    uint64_t pos[U];
    int64_t kv[U];
    float wv[U];   // (the shared position helpers' weight slot: never read here)
    bool inb[U];
    auto reset = [&] {   // an empty bag's row: +0.0 everywhere, no position
#pragma unroll
        for (int k = 0; k < CN; ++k) { m[k] = make_float4(0.f, 0.f, 0.f, 0.f); a[k] = u32x4{kNoArgmax, kNoArgmax, kNoArgmax, kNoArgmax}; }
    };
    // ---- short bags: one tile per bag ----
    if constexpr (BPW == 4) {
        bool first = true;
        reset();
        int64_t kpre;
        float wpre;
        pooled_short_prefetch<false>(keys, nullptr, begin, end, is_long, tl, kpre, wpre);
        for (uint64_t i = is_long ? end : begin; __any(i < end); i += U) {   // wave-uniform; tiles whose bag is done idle through the ballots
            pooled_short_positions<U, false>(i, begin, end, kpre, wpre, tile, pos, kv, wv, inb);
            pooled_fetch<DIM4, U, C>(t.tkeys, t.values, t.nb, dim4, kv, pos, inb, tile, tl, t.def4, row, found);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!inb[u]) continue;
#pragma unroll
                for (int k = 0; k < CN; ++k)
                    if (DIM4 != 0 || (uint32_t)((C0 + k) * 16 + tl) < dim4) pooled_max_take<ARGMAX>(m[k], a[k], row[u][C0 + k], (uint32_t)pos[u], first);
                first = false;
            }
        }
        if (has && !is_long) pooled_max_store<DIM4, C0, CN, BF16, ARGMAX>(out, argmax, bag * dim4, m, a, dim4, tl);
    }
    // ---- long bags: the four tiles share one bag at a time ----
    const uint64_t long_mask = __ballot(is_long && has);
    if (!long_mask) return;   // wave-uniform
    for (int q = 0; q < BPW; ++q) {
        if (!((long_mask >> (q * 16)) & 1)) continue;   // wave-uniform
        const uint64_t bq = BPW == 1 ? begin : __shfl(begin, q * 16), eq = BPW == 1 ? end : __shfl(end, q * 16);
        if constexpr (BPW == 4) table_of(bag0 + q, t);   // all four tiles work for bag q's table now
        bool first = true;
        reset();
        for (uint64_t i = bq; i < eq; i += 4 * U) {   // wave-uniform
            pooled_long_positions<U, false>(i, eq, keys, nullptr, tile, pos, kv, wv, inb);
            pooled_fetch<DIM4, U, C>(t.tkeys, t.values, t.nb, dim4, kv, pos, inb, tile, tl, t.def4, row, found);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int src = 0; src < 4; ++src) {
                    const uint64_t p = i + (uint64_t)u * 4 + src;   // the position tile `src` fetched in this round
                    if (p >= eq) continue;   // wave-uniform
#pragma unroll
                    for (int k = 0; k < CN; ++k) {
                        float4 v;
                        v.x = __shfl(row[u][C0 + k].x, src * 16 + tl); v.y = __shfl(row[u][C0 + k].y, src * 16 + tl);
                        v.z = __shfl(row[u][C0 + k].z, src * 16 + tl); v.w = __shfl(row[u][C0 + k].w, src * 16 + tl);
                        pooled_max_take<ARGMAX>(m[k], a[k], v, (uint32_t)p, first);
                    }
                    first = false;
                }
        }
        if (tile == 0) pooled_max_store<DIM4, C0, CN, BF16, ARGMAX>(out, argmax, (bag0 + q) * dim4, m, a, dim4, tl);
    }
}

// BPW, U: the launch shapes of find_pooled_kernel (meepo_find.hip).  GROUPED (mee_group_find_pooled_max): bag b is member b / bags_per_table's — its planes, its
// default row.  BF16: `out` holds bf16 rows, rounded once at the store; the comparisons are made on the fp32 values.  ARGMAX: argmax is written (positions are
// 32 bits: the entry points refuse n >= 2^32 with it).
template <int DIM4, int U, int BPW, bool GROUPED, bool BF16, bool ARGMAX>
__global__ __launch_bounds__(256) void find_pooled_max_kernel(const int64_t* __restrict__ tkeys_, const float4* __restrict__ values_, uint64_t nb_, float defv,
                                                              uint32_t dim4_rt, const GroupDesc* __restrict__ desc, uint64_t bags_per_table,
                                                              const int64_t* __restrict__ keys, uint64_t n_keys, const uint64_t* __restrict__ offsets,
                                                              uint64_t n_bags, void* __restrict__ out, uint8_t* __restrict__ found, uint32_t* __restrict__ argmax) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    auto table_of = [&](uint64_t b, PooledTable& t) {
        if constexpr (GROUPED) t = pooled_table(desc[b / bags_per_table], b / bags_per_table, kGroupSlotBits);
        else t = PooledTable{tkeys_, values_, nb_, make_float4(defv, defv, defv, defv), 0};
    };
    for (uint64_t b0 = wave * BPW; b0 < n_bags; b0 += n_waves * BPW) {
        const uint32_t nvalid = (uint32_t)(n_bags - b0 < BPW ? n_bags - b0 : BPW);
        if constexpr (DIM4 != 0) {
            pooled_max_bags<DIM4, U, BPW, DIM4 / 16, 0, DIM4 / 16, BF16, ARGMAX>(b0, nvalid, dim4, keys, offsets, n_keys, out, found, argmax, tile, tl, table_of);
        } else {   // the run-time row shape, a chunk of 256 elements per walk (kernel-uniform conditions)
            pooled_max_bags<0, U, BPW, 16, 0, 4, BF16, ARGMAX>(b0, nvalid, dim4, keys, offsets, n_keys, out, found, argmax, tile, tl, table_of);
            if (dim4 > 64) pooled_max_bags<0, U, BPW, 16, 4, 4, BF16, ARGMAX>(b0, nvalid, dim4, keys, offsets, n_keys, out, nullptr, argmax, tile, tl, table_of);
            if (dim4 > 128) pooled_max_bags<0, U, BPW, 16, 8, 4, BF16, ARGMAX>(b0, nvalid, dim4, keys, offsets, n_keys, out, nullptr, argmax, tile, tl, table_of);
            if (dim4 > 192) pooled_max_bags<0, U, BPW, 16, 12, 4, BF16, ARGMAX>(b0, nvalid, dim4, keys, offsets, n_keys, out, nullptr, argmax, tile, tl, table_of);
        }
    }
}

// ---- the backward (SPEC.md §3 "pooled_max_backward"): grads[i, j] = argmax[bag(i), j] == i ? bag_grads[bag(i), j] : +0.0 ----------------------------------
// The geometry of the forward and the walk of pooled_weighted_backward_kernel (meepo_find.hip) without its row fetch: the bag's grad row and argmax row are
// loaded into registers once, every position the bag covers gets a select and a store.  No key and no table row is read, so the one kernel serves a table
// and a group (whose bags are the members' bags side by side).  Nothing is carried from position to position.  U positions per tile and round.
template <int DIM4, int U, int BPW>
__global__ __launch_bounds__(256) void pooled_max_backward_kernel(const uint64_t* __restrict__ offsets, uint64_t n_bags, uint64_t n_keys, const u32x4* __restrict__ argmax,
                                                                  const float4* __restrict__ bag_grads, float4* __restrict__ grads, uint32_t dim4_rt) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    constexpr int C = DIM4 ? DIM4 / 16 : 16;
    for (uint64_t b0 = wave * BPW; b0 < n_bags; b0 += n_waves * BPW) {
        const uint64_t bag = BPW == 4 ? b0 + tile : b0;
        const bool has = bag < n_bags;
        uint64_t begin, end;
        pooled_span(offsets, bag, has, n_keys, begin, end);
        const bool is_long = BPW == 1 || end - begin >= kPoolLong;
        float4 g[C];
        u32x4 a[C];
        auto bag_rows = [&](uint64_t b, bool live) {   // the bag's grad row and argmax row, once into registers
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const bool ld = live && (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4);
                g[c] = ld ? bag_grads[b * dim4 + c * 16 + tl] : make_float4(0.f, 0.f, 0.f, 0.f);
                a[c] = ld ? argmax[b * dim4 + c * 16 + tl] : u32x4{kNoArgmax, kNoArgmax, kNoArgmax, kNoArgmax};
            }
        };
        auto put = [&](uint64_t p) {   // position p's grad row: the winner's element is a copy of the bag's (a -0.0 stays -0.0), every other +0.0
            const uint32_t q = (uint32_t)p;   // (n < 2^32: the entry points see to that)
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (DIM4 != 0 || (uint32_t)(c * 16 + tl) < dim4)
                    grads[p * dim4 + c * 16 + tl] = make_float4(a[c].x == q ? g[c].x : 0.f, a[c].y == q ? g[c].y : 0.f, a[c].z == q ? g[c].z : 0.f, a[c].w == q ? g[c].w : 0.f);
        };
        // ---- short bags: one tile per bag ----
        if constexpr (BPW == 4) {
            bag_rows(bag, has && !is_long && end > begin);
            for (uint64_t i = is_long ? end : begin; i < end; i += U)
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (i + u < end) put(i + u);
        }
        // ---- long bags: the four tiles share one bag at a time ----
        const uint64_t long_mask = __ballot(is_long && has);
        if (!long_mask) continue;   // wave-uniform
        for (int q = 0; q < BPW; ++q) {
            if (!((long_mask >> (q * 16)) & 1)) continue;   // wave-uniform
            const uint64_t bq = __shfl(begin, q * 16), eq = __shfl(end, q * 16);
            bag_rows(b0 + q, true);
            for (uint64_t i = bq; i < eq; i += 4 * U)   // wave-uniform
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (i + (uint64_t)u * 4 + tile < eq) put(i + (uint64_t)u * 4 + tile);
        }
    }
}

// what both lookups check about the call, before anything is launched or written
static int pooled_max_check(const char* name, bool bags, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, const void* d_out, uint32_t out_dtype,
                            const uint32_t* d_argmax_out) {
    if ((bags && (!d_bag_offsets || !d_out)) || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (d_argmax_out && (uint64_t)n >= (1ull << 32))
        return fail(MEE_ERR_INVALID_ARG, "%s: d_argmax_out names a batch position in 32 bits and n is %llu", name, (unsigned long long)n);
    if ((uintptr_t)d_argmax_out & 15) return fail(MEE_ERR_INVALID_ARG, "%s: d_argmax_out must be 16-byte aligned", name);
    return MEE_OK;
}

// ... and both backwards
static int pooled_max_backward_check(const char* name, size_t n, const uint64_t* d_bag_offsets, uint64_t n_bags, const uint32_t* d_argmax, const float* d_bag_grads,
                                     const float* d_grads_out) {
    if ((n_bags && (!d_bag_offsets || !d_argmax || !d_bag_grads)) || (n && !d_grads_out)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if ((uint64_t)n >= (1ull << 32)) return fail(MEE_ERR_INVALID_ARG, "%s: d_argmax names a batch position in 32 bits and n is %llu", name, (unsigned long long)n);
    if ((uintptr_t)d_argmax & 15) return fail(MEE_ERR_INVALID_ARG, "%s: d_argmax must be 16-byte aligned", name);
    return MEE_OK;
}

// the launch of either lookup: the pooled launch shape, the output type and whether argmax is asked for pick the instance
template <bool GROUPED>
static void pooled_max_launch(const mee_table* t, const mee_group* g, uint32_t dim4, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, uint64_t n_bags,
                              uint64_t bags_per_table, void* d_out, uint32_t out_dtype, uint8_t* d_found, uint32_t* d_argmax_out, hipStream_t st) {
    with_pooled_shape(dim4, n, n_bags, [&](auto d4, auto u, auto bpw, unsigned grid) {
        with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_flag(d_argmax_out != nullptr, [&](auto am) {
            if constexpr (GROUPED)
                find_pooled_max_kernel<d4, u, bpw, true, bf16, am><<<grid, 256, 0, st>>>(nullptr, nullptr, 0, 0.f, dim4, g->d_desc, bags_per_table, d_keys, n, d_bag_offsets, n_bags,
                                                                                        d_out, d_found, d_argmax_out);
            else
                find_pooled_max_kernel<d4, u, bpw, false, bf16, am><<<grid, 256, 0, st>>>(t->keys, (const float4*)t->values, t->nb, t->default_value, dim4, nullptr, 1, d_keys, n,
                                                                                         d_bag_offsets, n_bags, d_out, d_found, d_argmax_out);
        }); });
    });
}

static void pooled_max_backward_launch(uint32_t dim4, size_t n, const uint64_t* d_bag_offsets, uint64_t n_bags, const uint32_t* d_argmax, const float* d_bag_grads,
                                       float* d_grads_out, hipStream_t st) {
    with_pooled_shape(dim4, n, n_bags, [&](auto d4, auto u, auto bpw, unsigned grid) {
        pooled_max_backward_kernel<d4, u, bpw><<<grid, 256, 0, st>>>(d_bag_offsets, n_bags, n, (const u32x4*)d_argmax, (const float4*)d_bag_grads, (float4*)d_grads_out, dim4);
    });
}

}  // namespace mee

using namespace mee;

extern "C" {

int mee_find_pooled_max(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, void* d_out, uint32_t out_dtype,
                        uint8_t* d_found, uint32_t* d_argmax_out, void* stream) {
    MEE_RANGE("mee_find_pooled_max");
    MEE_FP32_ROWS_ONLY(t, "mee_find_pooled_max");
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_find_pooled_max: null argument");
    if (int rc = pooled_max_check("mee_find_pooled_max", n_bags != 0, d_keys, n, d_bag_offsets, d_out, out_dtype, d_argmax_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    DeviceGuard guard(t->device);
    pooled_max_launch<false>(t, nullptr, t->dim4, d_keys, n, d_bag_offsets, n_bags, 1, d_out, out_dtype, d_found, d_argmax_out, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_group_find_pooled_max(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype,
                              uint8_t* d_found, uint32_t* d_argmax_out, void* stream) {
    MEE_RANGE("mee_group_find_pooled_max");
    MEE_FP32_GROUP_ONLY(g, "mee_group_find_pooled_max");
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_pooled_max: null argument");
    uint64_t n_bags = 0;
    if (__builtin_mul_overflow((uint64_t)g->n_tables, (uint64_t)bags_per_table, &n_bags)) return fail(MEE_ERR_INVALID_ARG, "mee_group_find_pooled_max: n_tables * bags_per_table overflows");
    if (int rc = pooled_max_check("mee_group_find_pooled_max", n_bags != 0, d_keys, n, d_bag_offsets, d_out, out_dtype, d_argmax_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    if (int rc = group_refresh(g, stream)) return rc;   // a member's planes may have moved (mee_reserve)
    DeviceGuard guard(g->device);
    pooled_max_launch<true>(nullptr, g, g->dim4, d_keys, n, d_bag_offsets, n_bags, bags_per_table, d_out, out_dtype, d_found, d_argmax_out, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_pooled_max_backward(const mee_table* t, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const uint32_t* d_argmax, const float* d_bag_grads,
                            float* d_grads_out, void* stream) {
    MEE_RANGE("mee_pooled_max_backward");
    MEE_FP32_ROWS_ONLY(t, "mee_pooled_max_backward");
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_pooled_max_backward: null argument");
    if (int rc = pooled_max_backward_check("mee_pooled_max_backward", n, d_bag_offsets, n_bags, d_argmax, d_bag_grads, d_grads_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    DeviceGuard guard(t->device);
    pooled_max_backward_launch(t->dim4, n, d_bag_offsets, n_bags, d_argmax, d_bag_grads, d_grads_out, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_group_pooled_max_backward(mee_group* g, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const uint32_t* d_argmax, const float* d_bag_grads,
                                  float* d_grads_out, void* stream) {
    MEE_RANGE("mee_group_pooled_max_backward");
    MEE_FP32_GROUP_ONLY(g, "mee_group_pooled_max_backward");
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_group_pooled_max_backward: null argument");
    uint64_t n_bags = 0;
    if (__builtin_mul_overflow((uint64_t)g->n_tables, (uint64_t)bags_per_table, &n_bags)) return fail(MEE_ERR_INVALID_ARG, "mee_group_pooled_max_backward: n_tables * bags_per_table overflows");
    if (int rc = pooled_max_backward_check("mee_group_pooled_max_backward", n, d_bag_offsets, n_bags, d_argmax, d_bag_grads, d_grads_out)) return rc;
    if (n_bags == 0) return MEE_OK;
    DeviceGuard guard(g->device);
    pooled_max_backward_launch(g->dim4, n, d_bag_offsets, n_bags, d_argmax, d_bag_grads, d_grads_out, as_stream(stream));
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"
