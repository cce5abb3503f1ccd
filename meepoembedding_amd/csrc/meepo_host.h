// meepo_host.h — host-side plumbing shared by the C-ABI translation units (error slot, device guard).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/meepo_embedding.h"

namespace mee {

char* last_error_buf();  // thread-local, 512 bytes (defined in meepo_table.hip)

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(last_error_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}

#define MEE_HIP(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return ::mee::fail(e_ == hipErrorOutOfMemory ? MEE_ERR_OUT_OF_MEMORY : MEE_ERR_HIP,           \
                               "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// the typed-output forms (mee_*_as): fp32 or bf16 rows; a bf16 row group is one 8-byte store, so the buffer is 8-byte aligned
inline int check_out_dtype(const void* d_out, uint32_t out_dtype, const char* name) {
    if (out_dtype != MEE_DTYPE_F32 && out_dtype != MEE_DTYPE_BF16)   // (MEE_DTYPE_INT8 names a row storage type only)
        return fail(MEE_ERR_INVALID_ARG, "%s: unknown out_dtype %u (MEE_DTYPE_F32 or MEE_DTYPE_BF16)", name, out_dtype);
    if (out_dtype == MEE_DTYPE_BF16 && ((uintptr_t)d_out & 7)) return fail(MEE_ERR_INVALID_ARG, "%s: a bf16 output must be 8-byte aligned", name);
    return MEE_OK;
}

// roctx ranges around every operator of the C-ABI (tracing), so that `rocprofv3 --marker-trace --kernel-trace` groups the kernels by the
// operator that launched them.  The marker library (librocprofiler-sdk-roctx.so.1, part of ROCm) is bound with dlopen at the first operator call; when
// it is not there — or MEE_ROCTX=0 — a range is one predictable branch.  Without a profiler attached a push / pop pair costs ~0.1 us of host time.
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
};
const Roctx& roctx_api();   // (meepo_table.hip)
struct OpRange {
    bool on;
    explicit OpRange(const char* name) { const Roctx& r = roctx_api(); on = r.push != nullptr; if (on) (void)r.push(name); }
    ~OpRange() { if (on) (void)roctx_api().pop(); }
    OpRange(const OpRange&) = delete;
    OpRange& operator=(const OpRange&) = delete;
};
#define MEE_RANGE(name) ::mee::OpRange mee_range_(name)

// Makes `device` current for the scope of one API call and restores the caller's device afterwards.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) { err = hipSetDevice(device); switched = (err == hipSuccess); }
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

// what other translation units may know about a table (defined in meepo_table.hip)
struct TableView {
    int device;
    const int64_t* keys;
    const float* values;
    uint64_t nb;
    uint32_t dim, dim4;
    float default_value;
    uint64_t generation;   // bumped whenever the planes move (mee_reserve)
    float *s1, *s2;        // optimizer planes (null without)
    uint32_t optimizer;
    // what creating a key needs (find_or_insert): initial row, initial state, the sticky status word, the hit counters
    uint32_t initializer;
    float init_scale, init_acc;
    uint64_t init_seed;
    uint32_t* status;
    uint32_t* hits;
    bool bf16_rows;        // the value plane holds bf16 rows (MEE_FLAG_BF16_ROWS): `values` is then dim4 8-byte groups per slot
    long long* batch_slots;   // the per-position slot list of the table's per-batch scratch (>= 2 * max_batch entries: insert, remove and move borrow it)
    uint32_t* sketch;         // the admission sketch (MEE_FLAG_ADMISSION; null without): 3 rows of 2^sketch_log2w counters
    uint32_t sketch_log2w;
};
TableView table_view(const mee_table* t);
// The operators a serving table — bf16 rows or int8 rows — does not have (include/meepo_embedding.h, MEE_FLAG_BF16_ROWS / MEE_FLAG_INT8_ROWS) — and every
// create that takes tables — say so through this one check, before they launch or write anything: MEE_ERR_UNSUPPORTED naming `op` and the table's row
// type, MEE_OK for an fp32 table or a null one (defined in meepo_table.hip).  bf16_too = false: only an int8-row table is refused (mee_group_create, which
// takes bf16-row members).
int refuse_narrow_rows(const mee_table* t, const char* op, bool bf16_too = true);
#define MEE_FP32_ROWS_ONLY(t, op) do { if (int rc_ = ::mee::refuse_narrow_rows((t), (op))) return rc_; } while (0)
#define MEE_NO_INT8_ROWS(t, op) do { if (int rc_ = ::mee::refuse_narrow_rows((t), (op), false)) return rc_; } while (0)
int find_skip_padding(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint8_t* d_found, void* stream, uint32_t out_dtype = MEE_DTYPE_F32);   // meepo_find.hip

// ---- table groups (meepo_group.hip: grouped find / locate; meepo_table.hip: grouped apply) ---------------------------------
struct GroupDesc {   // 48 bytes per member table, device resident
    const int64_t* tkeys;
    float4* values;
    float4* s1;
    float4* s2;
    uint64_t nb;
    float defv;
    uint32_t pad;
};
struct GroupInit {   // per member, device resident: what creating a key in that table needs (grouped find_or_insert)
    uint64_t init_seed;
    uint32_t* status;
    uint32_t* hits;
    uint32_t initializer, optimizer;
    float init_scale, init_acc;
};
struct GroupMember {   // what ensure_grouped_body (meepo_device.h) asks of a member: the table a position creates in, and its row width in float4
    const GroupDesc* d;
    const GroupInit* in;
    uint32_t dim4;
};
struct GroupAdmit {   // per member, device resident: its admission sketch (grouped find_or_insert_admit / admission_decay); null without MEE_FLAG_ADMISSION
    uint32_t* sketch;
    uint32_t log2w, pad;
};
struct MoveTable {   // one side of a move (meepo_move.hip): a kernel argument for mee_move, per member and device resident for mee_group_move
    int64_t* tkeys;
    float4* plane[3];    // values, acc | m, v (null where the optimizer has none)
    uint64_t nb;
    uint32_t* status;
    uint32_t* hits;      // null without MEE_FLAG_TRACK_HITS
    long long* slots;    // the table's per-batch slot list (TableView::batch_slots): a move keeps the src slot of every position there between its launches
};
constexpr int kGroupSlotBits = 48;   // grouped apply names a row by (member << 48 | slot): unique per (table, key), never a reserved key
constexpr uint32_t kMaxGroupTables = 1024;   // offsets staged in LDS: (1024 + 1) x 8 B

inline unsigned grid_for(size_t work_items, unsigned per_block, unsigned cap) {
    size_t g = (work_items + per_block - 1) / per_block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// A dense output up to this size stays in the Infinity Cache: cached stores by default, streaming stores beyond (each site adds its own conditions)
constexpr uint64_t kCachedOutputBytes = 128ull << 20;

// ---- compile-time dispatch: a run-time choice becomes a constant for a generic lambda.  The row shapes: every row kernel has one instance for dim4 16
// (dim 64), one for dim4 32 (dim 128), and DIM4 = 0 for every other width, which loops at run time; this is the only place that says which widths have their own.
template <class F> decltype(auto) with_row_shape(uint32_t dim4, F&& f) {
    if (dim4 == 16) return f(std::integral_constant<int, 16>{});
    if (dim4 == 32) return f(std::integral_constant<int, 32>{});
    return f(std::integral_constant<int, 0>{});
}
template <class F> void with_flag(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// only the listed values are instantiated; the last one also takes any value that matches none (the `default:` of a switch)
template <int V, int... Rest, class F> void with_value(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else with_value<Rest...>(v, f);
}
template <int DIM4> struct RowShape {   // what the row kernels' launches share per row shape
    static constexpr int rows_per_tile = DIM4 == 16 ? 2 : 1;                     // keys in flight per 16-lane tile (R): the plain finds' default
    static constexpr int pooled_unroll_1 = DIM4 == 16 ? 4 : DIM4 == 32 ? 2 : 1;   // keys in flight per tile of a pooled lookup, one bag per wave
    static constexpr int pooled_unroll_4 = DIM4 == 16 ? 2 : 1;                    // ... four bags per wave
};
// The launch shape of a pooled lookup, picked by the batch's average bag (n, the number of keys, is a host value): 12 keys or more per bag -> one bag per
// wave, shorter -> four bags per wave.  with_pooled_shape (meepo_find.hip) and the mixed group's launches (meepo_mixed.hip) ask here.
inline bool pooled_wave_per_bag(size_t n, uint64_t n_bags) { return n / n_bags >= 12; }
// The launch shape of a pooled lookup over one row width (meepo_find.hip, meepo_pool_max.hip).  n (the number of keys, a host value) only picks it: mostly
// short bags -> four bags per wave on a grid of n_bags / 16 blocks, a long average -> one bag per wave on n_bags / 4.  f(d4, unroll, bags_per_wave, grid).
template <class F> void with_pooled_shape(uint32_t dim4, size_t n, uint64_t n_bags, F&& f) {
    with_row_shape(dim4, [&](auto d4) {
        if (pooled_wave_per_bag(n, n_bags)) f(d4, std::integral_constant<int, RowShape<d4>::pooled_unroll_1>{}, std::integral_constant<int, 1>{}, grid_for(n_bags, 4, 1u << 20));
        else f(d4, std::integral_constant<int, RowShape<d4>::pooled_unroll_4>{}, std::integral_constant<int, 4>{}, grid_for(n_bags, 16, 1u << 20));
    });
}
// FTRL-Proximal's step arguments (SPEC.md §4): lr finite and > 0; beta, l1, l2 neither NaN nor negative (checked before any launch)
inline bool ftrl_args_ok(float lr, float beta, float l1, float l2) { return lr > 0.f && lr < __builtin_inff() && beta >= 0.f && l1 >= 0.f && l2 >= 0.f; }

}  // namespace mee

#include <vector>
struct mee_group {
    int device;
    uint32_t n_tables, dim, dim4, optimizer;
    bool bf16_rows;        // every member is a bf16-row table (a serving group: lookups only); false: every member stores fp32 rows.  Never mixed (mee_group_create)
    std::vector<mee_table*> tables;
    std::vector<uint64_t> generations;   // of each table when its descriptor was last uploaded (mee_reserve moves planes)
    mee::GroupDesc* d_desc;
    mee::GroupInit* d_init;
    mee::MoveTable* d_move;   // the members as mee_group_move sees them, uploaded with the descriptors
    mee::GroupAdmit* d_admit; // the members' admission sketches, uploaded with the descriptors
    int no_admission;      // the first member created without MEE_FLAG_ADMISSION, -1 when every member has a sketch
    uint8_t* d_fmask;      // [max_apply_batch] found mask of grouped find_or_insert when the caller passes none
    // grouped apply (max_apply_batch > 0): a scratch-only table whose group table / per-position arrays serve the whole
    // jagged batch, and the located rows of the batch
    uint64_t max_apply_batch;
    mee_table* scratch;
    int64_t* d_gslot;
};
namespace mee {
int group_refresh(mee_group* g, void* stream);   // re-upload descriptors of members whose planes moved
int group_locate(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, uint64_t off_stride, size_t n, int64_t* d_gslot, hipStream_t st);
// refuse_narrow_rows for a group: the operators a bf16-row group does not have (include/meepo_embedding.h, the group section) say so through this one check,
// before they launch or write anything: MEE_ERR_UNSUPPORTED naming `op` (and `what` of it, when only an argument is refused), MEE_OK for an fp32 group or a
// null one (defined next to refuse_narrow_rows in meepo_table.hip)
int refuse_bf16_group(const mee_group* g, const char* op, const char* what = nullptr);
#define MEE_FP32_GROUP_ONLY(g, ...) do { if (int rc_ = ::mee::refuse_bf16_group((g), __VA_ARGS__)) return rc_; } while (0)
// what the operators over a GROUP of hot/cold pairs (mee_group_find_pooled_tiered, mee_group_ensure_tiered, mee_group_find_tiered, mee_group_find_or_insert_tiered) check about their two groups before anything
// is launched or written: fp32 rows (MEE_ERR_UNSUPPORTED), two different groups of one device, dim and number of tables, no table that is member j of
// both, only known count bits (MEE_TIER_COUNT_*) and the counters they need in EVERY member of that tier (MEE_ERR_INVALID_ARG).  Host only;
// defined in meepo_group.hip.
int tiered_groups_check(const mee_group* hot, const mee_group* cold, uint32_t count_flags, const char* name);
// The keyed pooled lookups (SPEC.md §3 "Keyed output"; defined in meepo_find.hip).  keyed_out_check: what every keyed entry point checks about its output
// before anything is launched or written — dtype and alignment (16 bytes for fp32, 8 for bf16), out_row_stride (elements; 0 = width) a multiple of 4 and
// at least `width`, and n_tables * bags_per_table < 2^32 when a step index is asked for; -> the stride in element groups.
int keyed_out_check(const char* name, uint64_t width, uint64_t n_tables, uint64_t bags_per_table, const void* d_out, uint32_t out_dtype,
                    uint64_t out_row_stride, bool want_index, uint64_t* stride4);
}
