// meepo_mixed.hip — a table group whose members differ in row width (SPEC.md §3 "Mixed groups"): the embedding-bag collection of a model
// with per-feature widths.  One pooled-lookup launch serves every member through the bag walk all pooled lookups share (pooled_bags,
// meepo_device.h); the optimizer step is the uniform group's grouped apply
// (meepo_table.hip / meepo_apply.hip, untouched) run once per width class on handles a small select launch re-bases to that class.
//
// Output layout ("class-major"): a class = the members of one dim, classes by ascending dim, members inside a class in the caller's order;
// member j's B bag rows are one [B, dim_j] block, the blocks follow each other class by class — so every class is one [T_c * B, dim_c]
// array, exactly what the uniform group's lookup writes and its apply reads (meepo_mixed_plan.h holds the bookkeeping).
#include <hip/hip_runtime.h>

#include <new>

#include "meepo_device.h"
#include "meepo_host.h"
#include "meepo_mixed_plan.h"
#include "meepo_table_int.h"

namespace mee {

struct MixedDesc {   // per member, device resident, beside its GroupDesc / GroupInit (caller's member order)
    uint64_t off4;   // the sum of dim4 over the blocks before this member's: its block starts at float4 (bf16: 8-byte group) B * off4
    uint32_t dim4, cls, rank;
    uint32_t col4;   // keyed layout (SPEC.md §3 "Keyed output"): the sum of dim4 over the members before this one in the CALLER's order — its column in a sample's row
};
struct KeyedMean {   // the last argument of the keyed lookup's instances
    int mean;
    KeyedOut keyed;
};

// The pooled lookup of a mixed group, one launch.  Waves are mapped to bags PER MEMBER: with BPW = 4 a member's B bags take Bp / 4 wave
// steps (Bp = B rounded up to a multiple of 4, in this mapping only), so the four bags of a wave never straddle two members and the
// member — its planes, its dim4, its output block — is wave-uniform: the branch to the row shape (DIM4 16 / 32 / run time) does not
// diverge.  BPW = 1 (the batch's average bag is long): a wave per bag.  The unrolls per shape are those of RowShape.
// A kernel's register budget is that of its widest path, and the run-time shape at its full width (16 float4 per lane: any dim up to 1024)
// takes 256 VGPRs — one wave per SIMD for the dim-64 members too.  CW = float4 per lane per row of the run-time shape (DIM4 = 0), which then serves
// dim4 <= 16 * CW; CW = 2 is the instance for groups whose run-time widths are all <= 128
// (8, 16, 32, 100, ...): the run-time path then holds no more row registers than the dim-128 path (82 VGPRs, 5 waves per SIMD with four bags
// per wave), and the launch picks it.  All instances beside the uniform group's: profiles/mixed_groups.md.
// KEYED (mee_mixed_group_find_pooled_keyed): member j's sample s goes to out[s * stride4 + col4_j ...] instead of its class-major block, and the walk also
// writes the step index beside the walk — the bag itself, the row of the class-major gradient the step reads (KeyedOut, meepo_device.h).
template <int BPW, bool BF16, int CW, bool KEYED = false>
__global__ __launch_bounds__(256) void mixed_find_pooled_kernel(const GroupDesc* __restrict__ desc, const MixedDesc* __restrict__ mdesc, uint32_t n_tables,
                                                                const int64_t* __restrict__ keys, const uint64_t* __restrict__ offsets,
                                                                uint64_t bags_per_table, float4* __restrict__ out, uint8_t* __restrict__ found,
                                                                int64_t* __restrict__ located, uint64_t n_keys, std::conditional_t<KEYED, KeyedMean, int> mean_) {
    int mean;   // (the table-major instances keep their argument list: the keyed ones get KeyedOut behind the mean flag)
    if constexpr (KEYED) mean = mean_.mean; else mean = mean_;
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t B = bags_per_table;
    const uint64_t per_member = BPW == 4 ? (B + 3) / 4 : B;   // wave steps per member
    const uint64_t n_units = (uint64_t)n_tables * per_member;
    for (uint64_t w = wave; w < n_units; w += n_waves) {
        const uint32_t member = __builtin_amdgcn_readfirstlane((uint32_t)(w / per_member));   // (uniform anyway: says so to the compiler)
        const uint64_t local0 = (w - (uint64_t)member * per_member) * BPW;
        const GroupDesc d = desc[member];
        const MixedDesc md = mdesc[member];
        const uint64_t rest = B - local0;
        const uint32_t nvalid = rest < (uint64_t)BPW ? (uint32_t)rest : (uint32_t)BPW;
        const uint64_t bag0 = (uint64_t)member * B + local0;
        const uint64_t row0 = (md.off4 * B) + local0 * md.dim4;
        const PooledTable t = pooled_table(d, member, kGroupSlotBits);
        // the bags of ONE member through the shared walk (pooled_bags, meepo_device.h) at the member's row shape: C = float4 per lane per row
        auto bags = [&](auto d4) {
            constexpr int C = d4 ? d4 / 16 : CW;
            constexpr int U = BPW == 4 ? RowShape<d4>::pooled_unroll_4 : RowShape<d4>::pooled_unroll_1;
            const uint32_t dim4 = d4 ? (uint32_t)d4 : md.dim4;
            if constexpr (KEYED)
                pooled_bags<d4, U, BPW, C, false, BF16, false, false, false>(
                    bag0, nvalid, dim4, keys, offsets, n_keys, nullptr, out, found, located, mean, TierArgs{}, tile, tl,
                    [&](uint64_t, PooledTable& bt) { bt = t; return true; }, [&](uint64_t b) { return (b - bag0 + local0) * mean_.keyed.stride4 + md.col4; });
            else
            pooled_bags<d4, U, BPW, C, false, BF16, false, false, false>(
                bag0, nvalid, dim4, keys, offsets, n_keys, nullptr, out, found, located, mean, TierArgs{}, tile, tl,
                [&](uint64_t, PooledTable& bt) { bt = t; return true; }, [&](uint64_t b) { return row0 + (b - bag0) * dim4; });
        };
        if constexpr (KEYED) {   // the step index of this step's bags: the bag itself (keyed_step_index, meepo_device.h)
            if (mean_.keyed.step_index) keyed_step_index<BPW>(bag0, nvalid, offsets, n_keys, tile, tl, mean_.keyed.step_index, [](uint64_t b) { return (uint32_t)b; });
        }
        if (md.dim4 == 16) bags(std::integral_constant<int, 16>{});
        else if (md.dim4 == 32) bags(std::integral_constant<int, 32>{});
        else bags(std::integral_constant<int, 0>{});
    }
}

// One tile per key position, read-only.
// SELECT = false: found[i] = the key is stored in its member (the present-before mask of a lookup with insert_missing).
// SELECT = true (the class select of the step): a position of one of class `cls`'s members gets its handle with the member re-based to
// its rank in the class — decoded from located_in, or probed when located_in is null — and its bag's row of the class's gradient block,
// rank * B + (bag mod B); every other position gets EMPTY, which the bucketed apply skips.  A handle is the caller's data: one that names
// no member of the group or a slot beyond the member's planes is dropped.  A RECLAIMED key flags its member (as group_locate does).
template <bool SELECT>
__global__ __launch_bounds__(256) void mixed_locate_kernel(const GroupDesc* __restrict__ desc, const MixedDesc* __restrict__ mdesc,
                                                           const GroupInit* __restrict__ init, uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                           uint64_t bags_per_table, const int64_t* __restrict__ keys, uint64_t n, uint8_t* __restrict__ found,
                                                           const int64_t* __restrict__ located_in, const uint32_t* __restrict__ bag_of, uint32_t cls,
                                                           int64_t* __restrict__ handles, uint32_t* __restrict__ rows) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    const uint64_t B = bags_per_table;
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    if (SELECT && located_in) {   // kernel-uniform: a thread per position, nothing probed
        for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
            const int64_t h = located_in[i];
            const uint64_t m = (uint64_t)h >> kGroupSlotBits, s = (uint64_t)h & ((1ull << kGroupSlotBits) - 1);
            int64_t o = kEmpty;
            uint32_t r = 0;
            if (h >= 0 && m < n_tables) {
                const MixedDesc md = mdesc[m];
                if (md.cls == cls && s < desc[m].nb * kW) {
                    o = (int64_t)(((uint64_t)md.rank << kGroupSlotBits) | s);
                    r = (uint32_t)(md.rank * B + bag_of[i] % B);
                }
            }
            handles[i] = o; rows[i] = r;
        }
        return;
    }
    stage_offsets(loff, offsets, B, n_tables, n);   // member j's keys: from bag offset j * B on
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = wave * 4; base < n; base += n_waves * 4) {
        const uint64_t i = base + tile;
        const bool inb = i < n && i >= loff[0] && i < loff[n_tables];
        const uint32_t m = inb ? member_of_position(loff, n_tables, i) : 0;
        const MixedDesc md = mdesc[m];
        const bool mine = inb && (!SELECT || md.cls == cls);
        const int64_t key = mine ? keys[i] : kEmpty;
        const bool act = mine && !reserved_key(key);
        const GroupDesc d = desc[m];
        const uint64_t b = bucket_of(key, d.nb);
        const int64_t kb = act ? d.tkeys[b * kW + tl] : kEmpty;
        const int64_t slot = tile_probe(d.tkeys, d.nb, key, act, b, kb, tile, tl);
        if (i < n && tl == 0) {
            if constexpr (SELECT) {
                handles[i] = slot >= 0 ? (int64_t)(((uint64_t)md.rank << kGroupSlotBits) | (uint64_t)slot) : kEmpty;
                rows[i] = slot >= 0 ? (uint32_t)(md.rank * B + bag_of[i] % B) : 0u;
                if (mine && key == kReclaimed) atomicOr(init[m].status, (uint32_t)MEE_STATUS_RESERVED_KEY);
            } else found[i] = slot >= 0;
        }
    }
}

// The creation pass of a lookup with insert_missing: ensure_grouped_body (meepo_device.h) with member j creating in desc[j] / init[j] at the member's
// own dim4, over the segments that begin at every bags_per_table-th bag offset.  No row is written back: the lookup that follows reads the tables.
__global__ __launch_bounds__(256) void mixed_ensure_kernel(const GroupDesc* __restrict__ desc, const MixedDesc* __restrict__ mdesc,
                                                           const GroupInit* __restrict__ init, uint32_t n_tables, const uint64_t* __restrict__ offsets,
                                                           uint64_t bags_per_table, const int64_t* __restrict__ keys, uint64_t n,
                                                           const uint8_t* __restrict__ found) {
    __shared__ uint64_t loff[kMaxGroupTables + 1];
    ensure_grouped_body<false, false>(loff, n_tables, offsets, bags_per_table, keys, n, found, nullptr,
                                      [&](uint32_t lo, bool) { return GroupMember{desc + lo, init + lo, mdesc[lo].dim4}; });
}

// The backward's side of the keyed layout: a keyed gradient [B, stride] (fp32, or BF16 widened — exact) is taken apart into the class-major fp32
// blocks the step reads, member j's row s from in[s * stride4 + col4_j ...] to out[(B * off4_j + s * dim4_j) ...].  One tile per bag row, one element
// group per lane and round.  MEAN: every element is divided by (float)max(len, 1), len = offsets[b + 1] - offsets[b] as the caller wrote them (a
// division, not a multiplication by the reciprocal: what `g / lens.clamp(min=1)` gives).
template <bool BF16>
__global__ __launch_bounds__(256) void mixed_keyed_grads_kernel(const MixedDesc* __restrict__ mdesc, uint32_t n_tables, uint64_t bags_per_table,
                                                                const void* __restrict__ in, uint64_t stride4, const uint64_t* __restrict__ offsets, int mean,
                                                                float4* __restrict__ out) {
    const uint64_t B = bags_per_table, n_bags = (uint64_t)n_tables * B;
    const int tl = threadIdx.x & 15;
    const uint64_t tile0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4, n_tiles = ((uint64_t)gridDim.x * blockDim.x) >> 4;
    for (uint64_t b = tile0; b < n_bags; b += n_tiles) {
        const uint64_t j = b / B, s = b - j * B;
        const MixedDesc md = mdesc[j];
        float len = 1.f;
        if (mean) {
            const int64_t l = (int64_t)(offsets[b + 1] - offsets[b]);
            len = (float)(l > 1 ? l : 1);
        }
        const uint64_t src = s * stride4 + md.col4, dst = md.off4 * B + s * md.dim4;
        for (uint32_t c = tl; c < md.dim4; c += 16) {
            float4 v;
            if constexpr (BF16) {
                const f32x4 w = widen_bf16x4(reinterpret_cast<const u32x2*>(in)[src + c]);
                v = make_float4(w.x, w.y, w.z, w.w);
            } else v = reinterpret_cast<const float4*>(in)[src + c];
            if (mean) { v.x = v.x / len; v.y = v.y / len; v.z = v.z / len; v.w = v.w / len; }
            out[dst + c] = v;
        }
    }
}

}  // namespace mee

using namespace mee;

struct mee_mixed_group {
    int device = 0;
    uint32_t n_tables = 0, optimizer = 0;
    uint64_t max_apply_batch = 0;
    std::vector<mee_table*> tables;
    std::vector<uint64_t> generations;   // of each table when its descriptor was last uploaded (mee_reserve moves planes)
    MixedPlan plan;
    int run_time_cw = 2;                 // float4 per lane of the lookup's run-time row shape: 2 while every width without an instance of its own is <= 128
    std::vector<mee_group*> sub;         // one ordinary group per class (its members in the caller's order): the step, and the whole lookup when there is one class
    GroupDesc* d_desc = nullptr;
    GroupInit* d_init = nullptr;
    MixedDesc* d_mdesc = nullptr;
    int64_t* d_handles = nullptr;        // [max_apply_batch] the class select's handles and gradient rows (one class at a time, stream-ordered)
    uint32_t* d_rows = nullptr;
};

static int mixed_upload(mee_mixed_group* g) {
    std::vector<GroupDesc> h(g->n_tables);
    std::vector<GroupInit> hi(g->n_tables);
    std::vector<MixedDesc> hm(g->n_tables);
    uint32_t col4 = 0;
    for (uint32_t j = 0; j < g->n_tables; ++j) {
        const TableView v = table_view(g->tables[j]);
        h[j] = GroupDesc{v.keys, (float4*)v.values, (float4*)v.s1, (float4*)v.s2, v.nb, v.default_value, 0};
        hi[j] = GroupInit{v.init_seed, v.status, v.hits, v.initializer, v.optimizer, v.init_scale, v.init_acc};
        hm[j] = MixedDesc{g->plan.off4[j], v.dim4, g->plan.cls[j], g->plan.rank[j], col4};
        col4 += v.dim4;
        g->generations[j] = v.generation;
    }
    MEE_HIP(hipMemcpy(g->d_desc, h.data(), h.size() * sizeof(GroupDesc), hipMemcpyHostToDevice));  // synchronous, rare
    MEE_HIP(hipMemcpy(g->d_init, hi.data(), hi.size() * sizeof(GroupInit), hipMemcpyHostToDevice));
    MEE_HIP(hipMemcpy(g->d_mdesc, hm.data(), hm.size() * sizeof(MixedDesc), hipMemcpyHostToDevice));
    return MEE_OK;
}

// group_refresh for the mixed descriptors (the class groups run their own check inside their operators)
static int mixed_refresh(mee_mixed_group* g, void* stream) {
    for (uint32_t j = 0; j < g->n_tables; ++j)
        if (table_view(g->tables[j]).generation != g->generations[j]) {   // a table was rehashed: its planes moved
            DeviceGuard guard(g->device);
            MEE_HIP(hipStreamSynchronize((hipStream_t)stream));           // launches in flight may still read the old descriptors
            return mixed_upload(g);
        }
    return MEE_OK;
}

// The prelude of a lookup with insert_missing.  `found` = present before the call, for a key repeated in the batch too: a read-only probe pass fixes the
// mask before the ensure pass creates anything; the lookup that follows leaves the mask alone.
static int mixed_insert_missing(mee_mixed_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, uint64_t B, uint8_t* d_found, hipStream_t st) {
    DeviceGuard guard(g->device);
    mixed_locate_kernel<false><<<grid_for(n, 16, 8192), 256, 0, st>>>(g->d_desc, g->d_mdesc, g->d_init, g->n_tables, d_bag_offsets, B, d_keys, n, d_found,
                                                                      nullptr, nullptr, 0, nullptr, nullptr);
    mixed_ensure_kernel<<<grid_for(n, 16, 8192), 256, 0, st>>>(g->d_desc, g->d_mdesc, g->d_init, g->n_tables, d_bag_offsets, B, d_keys, n, d_found);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

extern "C" {

int mee_mixed_group_create(mee_table* const* tables, uint32_t n_tables, uint64_t max_apply_batch, mee_mixed_group** out) {
    MEE_RANGE("mee_mixed_group_create");
    if (!tables || !out || n_tables == 0 || n_tables > kMaxGroupTables)
        return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_create: need 1..%u tables", kMaxGroupTables);
    *out = nullptr;
    for (uint32_t j = 0; j < n_tables; ++j)
        if (!tables[j]) return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_create: table %u is null", j);
    for (uint32_t j = 0; j < n_tables; ++j) MEE_FP32_ROWS_ONLY(tables[j], "mee_mixed_group_create");   // covers every mee_mixed_group_* operator
    const TableView v0 = table_view(tables[0]);
    std::vector<uint32_t> dim4(n_tables);
    for (uint32_t j = 0; j < n_tables; ++j) {
        const TableView v = table_view(tables[j]);
        dim4[j] = v.dim4;
        if (v.device != v0.device)
            return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_create: table %u is on device %d, table 0 on device %d", j, v.device, v0.device);
        if (max_apply_batch && v.optimizer != v0.optimizer)
            return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_create: a group with an optimizer step needs one optimizer for all members (table %u: %u vs %u)", j, v.optimizer, v0.optimizer);
    }
    if (max_apply_batch > (1ull << 30)) return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_create: max_apply_batch must be <= 2^30");
    mee_mixed_group* g = new (std::nothrow) mee_mixed_group();
    if (!g) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    g->device = v0.device; g->n_tables = n_tables; g->optimizer = v0.optimizer; g->max_apply_batch = max_apply_batch;
    g->tables.assign(tables, tables + n_tables);
    g->generations.assign(n_tables, 0);
    g->plan = mixed_plan(dim4.data(), n_tables);
    for (uint32_t d4 : dim4) if (d4 > 32) g->run_time_cw = 16;
    for (size_t c = 0; c < g->plan.class_dim4.size(); ++c) {
        std::vector<mee_table*> members;
        for (uint32_t j : g->plan.class_members[c]) members.push_back(tables[j]);
        mee_group* s = nullptr;
        if (int rc = mee_group_create(members.data(), (uint32_t)members.size(), max_apply_batch, &s)) { mee_mixed_group_destroy(g); return rc; }
        g->sub.push_back(s);
    }
    DeviceGuard guard(g->device);
    hipError_t e = hipMalloc((void**)&g->d_desc, n_tables * sizeof(GroupDesc));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_init, n_tables * sizeof(GroupInit));
    if (e == hipSuccess) e = hipMalloc((void**)&g->d_mdesc, n_tables * sizeof(MixedDesc));
    if (e == hipSuccess && max_apply_batch && g->sub.size() > 1) {
        e = hipMalloc((void**)&g->d_handles, max_apply_batch * sizeof(int64_t));
        if (e == hipSuccess) e = hipMalloc((void**)&g->d_rows, max_apply_batch * sizeof(uint32_t));
    }
    if (e != hipSuccess) { mee_mixed_group_destroy(g); return fail(MEE_ERR_OUT_OF_MEMORY, "hipMalloc(mixed group): %s", hipGetErrorString(e)); }
    if (int rc = mixed_upload(g)) { mee_mixed_group_destroy(g); return rc; }
    *out = g;
    return MEE_OK;
}

int mee_mixed_group_destroy(mee_mixed_group* g) {
    MEE_RANGE("mee_mixed_group_destroy");
    if (!g) return MEE_OK;
    {
        DeviceGuard guard(g->device);
        (void)hipDeviceSynchronize();
        (void)hipFree(g->d_desc);
        (void)hipFree(g->d_init);
        (void)hipFree(g->d_mdesc);
        (void)hipFree(g->d_handles);
        (void)hipFree(g->d_rows);
    }
    for (mee_group* s : g->sub) mee_group_destroy(s);
    delete g;
    return MEE_OK;
}

int mee_mixed_group_layout(const mee_mixed_group* g, uint64_t bags_per_table, uint64_t* elem_offsets, uint64_t* total_elems) {
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_layout: null group");
    if (elem_offsets)
        for (uint32_t j = 0; j < g->n_tables; ++j) elem_offsets[j] = bags_per_table * g->plan.off4[j] * 4;
    if (total_elems) *total_elems = bags_per_table * g->plan.total4 * 4;
    return MEE_OK;
}

int mee_mixed_group_set_tuning(mee_mixed_group* g, const char* name, int value) {
    if (!g || !name) return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_set_tuning: null argument");
    for (mee_group* s : g->sub)
        if (int rc = mee_group_set_tuning(s, name, value)) return rc;
    return MEE_OK;
}

int mee_mixed_group_find_pooled(mee_mixed_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located, int mode, int insert_missing, void* stream) {
    MEE_RANGE("mee_mixed_group_find_pooled");
    const char* name = "mee_mixed_group_find_pooled";
    if (!g || (bags_per_table && (!d_bag_offsets || !d_out)) || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (int rc = check_out_dtype(d_out, out_dtype, name)) return rc;
    if (mode != MEE_POOL_SUM && mode != MEE_POOL_MEAN) return fail(MEE_ERR_INVALID_ARG, "%s: mode must be MEE_POOL_SUM or MEE_POOL_MEAN", name);
    if (insert_missing && n && !d_found) return fail(MEE_ERR_INVALID_ARG, "%s: insert_missing needs d_found (the present-before mask)", name);
    if (bags_per_table == 0) return MEE_OK;
    if (int rc = mixed_refresh(g, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t B = bags_per_table;
    if (insert_missing && n) {
        if (int rc = mixed_insert_missing(g, d_keys, n, d_bag_offsets, B, d_found, st)) return rc;
        d_found = nullptr;
    }
    if (g->sub.size() == 1)   // one width: the uniform group's launch, bit for bit
        return mee_group_find_pooled_as(g->sub[0], d_keys, n, d_bag_offsets, bags_per_table, nullptr, d_out, out_dtype, d_found, d_located, mode, stream);
    DeviceGuard guard(g->device);
    const uint64_t n_bags = (uint64_t)g->n_tables * B;
    const bool wave_per_bag = pooled_wave_per_bag(n, n_bags);
    const uint64_t units = (uint64_t)g->n_tables * (wave_per_bag ? B : (B + 3) / 4);
    with_flag(wave_per_bag, [&](auto wpb) { with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_value<2, 16>(g->run_time_cw, [&](auto cw) {
        mixed_find_pooled_kernel<wpb ? 1 : 4, bf16, cw><<<grid_for(units, 4, 1u << 20), 256, 0, st>>>(g->d_desc, g->d_mdesc, g->n_tables, d_keys, d_bag_offsets, B, (float4*)d_out,
                                                                                                  d_found, d_located, n, mode == MEE_POOL_MEAN);
    }); }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// ---- the keyed layout (SPEC.md §3 "Keyed output"): one row per sample, member j's pooled vector at column col_j = the sum of the dims before it ----
static uint64_t mixed_width(const mee_mixed_group* g) {
    uint64_t w = 0;
    for (mee_table* t : g->tables) w += (uint64_t)table_view(t).dim4 * 4;
    return w;
}

int mee_mixed_group_keyed_layout(const mee_mixed_group* g, uint64_t* col_offsets, uint64_t* width) {
    if (!g) return fail(MEE_ERR_INVALID_ARG, "mee_mixed_group_keyed_layout: null group");
    uint64_t w = 0;
    for (uint32_t j = 0; j < g->n_tables; ++j) {
        if (col_offsets) col_offsets[j] = w;
        w += (uint64_t)table_view(g->tables[j]).dim4 * 4;
    }
    if (width) *width = w;
    return MEE_OK;
}

int mee_mixed_group_find_pooled_keyed(mee_mixed_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      void* d_out, uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found, int64_t* d_located,
                                      uint32_t* d_step_index_out, int mode, int insert_missing, void* stream) {
    MEE_RANGE("mee_mixed_group_find_pooled_keyed");
    const char* name = "mee_mixed_group_find_pooled_keyed";
    if (!g || (bags_per_table && (!d_bag_offsets || !d_out)) || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (mode != MEE_POOL_SUM && mode != MEE_POOL_MEAN) return fail(MEE_ERR_INVALID_ARG, "%s: mode must be MEE_POOL_SUM or MEE_POOL_MEAN", name);
    if (insert_missing && n && !d_found) return fail(MEE_ERR_INVALID_ARG, "%s: insert_missing needs d_found (the present-before mask)", name);
    uint64_t stride4 = 0;
    if (int rc = keyed_out_check(name, mixed_width(g), g->n_tables, bags_per_table, d_out, out_dtype, out_row_stride, d_step_index_out != nullptr, &stride4)) return rc;
    if (bags_per_table == 0) return MEE_OK;
    if (int rc = mixed_refresh(g, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t B = bags_per_table;
    if (insert_missing && n) {
        if (int rc = mixed_insert_missing(g, d_keys, n, d_bag_offsets, B, d_found, st)) return rc;
        d_found = nullptr;
    }
    if (g->sub.size() == 1) {   // one width: the uniform group's keyed launch; the step index names the bag, as the mixed step reads class-major rows
        PooledCall c{name};
        c.of(g->sub[0]);
        c.keys = d_keys; c.n = n; c.offsets = d_bag_offsets; c.bags = bags_per_table; c.out = d_out; c.out_dtype = out_dtype; c.found = d_found; c.located = d_located;
        c.mode = mode; c.keyed = true; c.out_row_stride = stride4 * 4; c.step_index = d_step_index_out; c.index_by_bag = true; c.stream = stream;
        return pooled_find(c);
    }
    DeviceGuard guard(g->device);
    const uint64_t n_bags = (uint64_t)g->n_tables * B;
    const bool wave_per_bag = pooled_wave_per_bag(n, n_bags);
    const uint64_t units = (uint64_t)g->n_tables * (wave_per_bag ? B : (B + 3) / 4);
    const KeyedOut keyed{stride4, d_step_index_out, 1ull, B};
    with_flag(wave_per_bag, [&](auto wpb) { with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) { with_value<2, 16>(g->run_time_cw, [&](auto cw) {
        mixed_find_pooled_kernel<wpb ? 1 : 4, bf16, cw, true><<<grid_for(units, 4, 1u << 20), 256, 0, st>>>(g->d_desc, g->d_mdesc, g->n_tables, d_keys, d_bag_offsets, B,
                                                                                                        (float4*)d_out, d_found, d_located, n, KeyedMean{mode == MEE_POOL_MEAN, keyed});
    }); }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_mixed_group_keyed_grads(mee_mixed_group* g, const void* d_keyed_grads, uint32_t in_dtype, size_t row_stride, size_t bags_per_table,
                                const uint64_t* d_bag_offsets, int mode, float* d_bag_grads_out, void* stream) {
    MEE_RANGE("mee_mixed_group_keyed_grads");
    const char* name = "mee_mixed_group_keyed_grads";
    if (!g || (bags_per_table && (!d_keyed_grads || !d_bag_grads_out))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (mode != MEE_POOL_SUM && mode != MEE_POOL_MEAN) return fail(MEE_ERR_INVALID_ARG, "%s: mode must be MEE_POOL_SUM or MEE_POOL_MEAN", name);
    if (mode == MEE_POOL_MEAN && bags_per_table && !d_bag_offsets) return fail(MEE_ERR_INVALID_ARG, "%s: MEE_POOL_MEAN needs d_bag_offsets (the bags' lengths)", name);
    if ((uintptr_t)d_bag_grads_out & 15) return fail(MEE_ERR_INVALID_ARG, "%s: d_bag_grads_out must be 16-byte aligned", name);
    uint64_t stride4 = 0;
    if (int rc = keyed_out_check(name, mixed_width(g), g->n_tables, bags_per_table, d_keyed_grads, in_dtype, row_stride, false, &stride4)) return rc;
    if (bags_per_table == 0) return MEE_OK;
    DeviceGuard guard(g->device);
    hipStream_t st = (hipStream_t)stream;
    const uint64_t n_bags = (uint64_t)g->n_tables * bags_per_table;
    with_flag(in_dtype == MEE_DTYPE_BF16, [&](auto bf16) {
        mixed_keyed_grads_kernel<bf16><<<grid_for(n_bags, 16, 1u << 20), 256, 0, st>>>(g->d_mdesc, g->n_tables, bags_per_table, d_keyed_grads, stride4, d_bag_offsets,
                                                                                       mode == MEE_POOL_MEAN, (float4*)d_bag_grads_out);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

}  // extern "C"

// the step: per class, the select launch and the class group's pooled step (group_apply_pooled, meepo_table.hip) on the class's slice of bag_grads.
// The scalars are refused before anything else, so before the first class's select launch.
static int mixed_apply_common(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads,
                              const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, uint32_t kind, const OptScalars& s, void* stream, const char* name) {
    OptArgs a;
    if (int rc = opt_args(kind, s, name, &a)) return rc;
    if (!g || (n && ((!d_keys && !d_located) || !d_bag_grads || !d_bag_of_position || !bags_per_table)) || (n && !d_located && !d_bag_offsets))
        return fail(MEE_ERR_INVALID_ARG, "%s: null argument / zero bags_per_table", name);
    if (!g->max_apply_batch || g->optimizer == MEE_OPT_NONE) return fail(MEE_ERR_UNSUPPORTED, "%s: group was created with max_apply_batch = 0 or its tables have no optimizer", name);
    if (g->optimizer != kind) return fail(MEE_ERR_UNSUPPORTED, "%s: the group's tables were created with optimizer=%u", name, g->optimizer);
    if (n > g->max_apply_batch) return fail(MEE_ERR_BATCH_TOO_LARGE, "%s: n=%zu exceeds the group's max_apply_batch=%llu", name, n, (unsigned long long)g->max_apply_batch);
    if (n == 0) return MEE_OK;
    if (g->sub.size() == 1)   // one width: the uniform group's step
        return group_apply_pooled(g->sub[0], d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, a, stream, name);
    if (int rc = mixed_refresh(g, stream)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t B = bags_per_table;
    for (size_t c = 0; c < g->sub.size(); ++c) {
        {
            DeviceGuard guard(g->device);
            const unsigned grid = d_located ? grid_for(n, 256, 8192) : grid_for(n, 16, 8192);
            mixed_locate_kernel<true><<<grid, 256, 0, st>>>(g->d_desc, g->d_mdesc, g->d_init, g->n_tables, d_bag_offsets, B, d_keys, n, nullptr, d_located,
                                                            d_bag_of_position, (uint32_t)c, g->d_handles, g->d_rows);
            MEE_HIP(hipGetLastError());
        }
        // the class is one [T_c * B, dim_c] array of bag_grads; positions of other classes carry EMPTY handles
        if (int rc = group_apply_pooled(g->sub[c], nullptr, nullptr, bags_per_table, d_bag_grads + B * g->plan.class_off4[c] * 4, g->d_rows, g->d_handles, n, a, stream, name)) return rc;
    }
    return MEE_OK;
}

extern "C" {

int mee_mixed_group_apply_adagrad_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                         const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr,
                                         float eps, void* stream) {
    MEE_RANGE("mee_mixed_group_apply_adagrad_pooled");
    return mixed_apply_common(g, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, MEE_OPT_ADAGRAD, {lr, eps}, stream,
                              "mee_mixed_group_apply_adagrad_pooled");
}

int mee_mixed_group_apply_adam_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr,
                                      float beta1, float beta2, float eps, uint64_t step, void* stream) {
    MEE_RANGE("mee_mixed_group_apply_adam_pooled");
    return mixed_apply_common(g, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, MEE_OPT_ADAM, {lr, beta1, beta2, eps, step}, stream,
                              "mee_mixed_group_apply_adam_pooled");
}

int mee_mixed_group_apply_ftrl_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr,
                                      float beta, float l1, float l2, void* stream) {
    MEE_RANGE("mee_mixed_group_apply_ftrl_pooled");
    return mixed_apply_common(g, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, MEE_OPT_FTRL, {lr, beta, l1, l2}, stream,
                              "mee_mixed_group_apply_ftrl_pooled");
}

}  // extern "C"
