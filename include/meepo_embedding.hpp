// meepo_embedding.hpp — C++17 host-side interface over the C-ABI (include/meepo_embedding.h), header-only.
//
// This is the "C++ host code" BASELINE.json's north_star puts above the thin C-ABI: RAII owners and lookuptable-style
// methods (find / insert / assign / remove / find_or_insert / export / size, sparse Adagrad/Adam apply), a hot/cold
// pair, the shard router and the peer-mapped exchange context.  The reference snapshot defines no C++ interface
// (/root/reference/README.md:2 is its only functional statement); names follow the verbs the north_star lists.
// Every pointer argument is DEVICE memory; every call is asynchronous on the given stream unless noted; errors are
// thrown as meepo::Error (code + the library's message).  tests/cabi/host_cpp_test.cpp drives all of it on the GPU.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "meepo_embedding.h"

namespace meepo {

class Error : public std::runtime_error {
public:
    Error(int code, const std::string& msg) : std::runtime_error("meepo error " + std::to_string(code) + ": " + msg), code_(code) {}
    int code() const noexcept { return code_; }
private:
    int code_;
};

inline void check(int rc) {
    if (rc != MEE_OK) throw Error(rc, mee_last_error());
}

struct TableOptions {
    int32_t device = 0;
    uint64_t capacity = 0;      // slots (rounded up to 16 x a prime); size for load <= 0.85
    uint32_t dim = 64;
    uint32_t optimizer = MEE_OPT_NONE;
    uint64_t max_batch = 1u << 20;
    float default_value = 0.0f;
    float initial_accumulator = 0.0f;
    uint32_t initializer = MEE_INIT_CONSTANT;
    float init_scale = 0.0f;
    uint64_t init_seed = 0;
    uint32_t value_memory = MEE_MEM_HBM;  // MEE_MEM_HOST_PINNED = cold tier (rows in pinned host DRAM)
    bool bf16_rows = false;     // MEE_FLAG_BF16_ROWS: a serving table that stores its rows as bf16 (no optimizer, dim % 8 == 0, HBM)
    bool admission = false;     // MEE_FLAG_ADMISSION: the table keeps a count-min sketch (mee_find_or_insert_admit, Group::find_or_insert_admit)
    bool int8_rows = false;     // MEE_FLAG_INT8_ROWS: a serving table that stores its rows as int8 codes + one fp32 scale (no optimizer, dim % 16 == 0, HBM; not with bf16_rows)
};

// One HBM-resident shard (SPEC.md §2-§4).  Move-only.
class Table {
public:
    explicit Table(const TableOptions& o) {
        mee_config c{};
        c.struct_size = sizeof c; c.device = o.device; c.capacity = o.capacity; c.dim = o.dim; c.optimizer = o.optimizer;
        c.max_batch = o.max_batch; c.default_value = o.default_value; c.initial_accumulator = o.initial_accumulator;
        c.initializer = o.initializer; c.init_scale = o.init_scale; c.init_seed = o.init_seed; c.value_memory = o.value_memory;
        c.flags = (o.bf16_rows ? MEE_FLAG_BF16_ROWS : 0u) | (o.int8_rows ? MEE_FLAG_INT8_ROWS : 0u) | (o.admission ? MEE_FLAG_ADMISSION : 0u);
        check(mee_table_create(&c, &t_));
    }
    ~Table() { if (t_) mee_table_destroy(t_); }
    Table(Table&& other) noexcept : t_(std::exchange(other.t_, nullptr)) {}
    Table& operator=(Table&& other) noexcept { if (this != &other) { if (t_) mee_table_destroy(t_); t_ = std::exchange(other.t_, nullptr); } return *this; }
    Table(const Table&) = delete;
    Table& operator=(const Table&) = delete;

    mee_table* handle() const noexcept { return t_; }
    mee_table_info info() const { mee_table_info i{}; check(mee_table_info_get(t_, &i)); return i; }
    uint32_t value_dtype() const { uint32_t d = MEE_DTYPE_F32; check(mee_table_value_dtype(t_, &d)); return d; }   // MEE_DTYPE_BF16: a bf16-row table, MEE_DTYPE_INT8: an int8-row table

    void find(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream = nullptr) const { check(mee_find(t_, d_keys, n, d_out, d_found, stream)); }
    // ... with this call's cache policy (MEE_FIND_* flags)
    void find(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, uint32_t flags, void* stream) const { check(mee_find_ex(t_, d_keys, n, d_out, d_found, flags, stream)); }
    // embedding bag: d_out[b,:] = sum (MEE_POOL_SUM) or mean (MEE_POOL_MEAN) of the rows of d_keys[d_bag_offsets[b] .. d_bag_offsets[b+1])
    void find_pooled(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, float* d_out, uint8_t* d_found = nullptr, int mode = MEE_POOL_SUM, void* stream = nullptr) const {
        check(mee_find_pooled(t_, d_keys, n, d_bag_offsets, n_bags, d_out, d_found, mode, stream));
    }
    // weighted embedding bag (SUM): d_out[b,:] = sum of d_weights[i] * row_i over the bag in position order; d_located_out = mee_find_located handles
    void find_pooled_weighted(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const float* d_weights, float* d_out, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, void* stream = nullptr) const { check(mee_find_pooled_weighted(t_, d_keys, n, d_bag_offsets, n_bags, d_weights, d_out, d_found, d_located_out, stream)); }
    // its backward: d_grads_out[i,:] = d_weights[i] * d_bag_grads[bag(i),:] (feed to apply_*), d_weight_grads_out[i] = <d_bag_grads[bag(i)], row_i> (nullable)
    void pooled_weighted_backward(const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const float* d_weights, const float* d_bag_grads, float* d_grads_out, float* d_weight_grads_out = nullptr, void* stream = nullptr) const { check(mee_pooled_weighted_backward(t_, d_keys, d_located, n, d_bag_offsets, n_bags, d_weights, d_bag_grads, d_grads_out, d_weight_grads_out, stream)); }
    // max pooling (torch.nn.EmbeddingBag mode="max"): d_out[b, j] = the first greatest row[p][j] over the bag's positions, d_argmax_out[b, j] = that batch position (nullable)
    void find_pooled_max(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, uint32_t* d_argmax_out = nullptr, void* stream = nullptr) const { check(mee_find_pooled_max(t_, d_keys, n, d_bag_offsets, n_bags, d_out, out_dtype, d_found, d_argmax_out, stream)); }
    // its backward: d_grads_out[i, j] = d_argmax[bag(i), j] == i ? d_bag_grads[bag(i), j] : +0.0 (feed to apply_*)
    void pooled_max_backward(size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const uint32_t* d_argmax, const float* d_bag_grads, float* d_grads_out, void* stream = nullptr) const { check(mee_pooled_max_backward(t_, n, d_bag_offsets, n_bags, d_argmax, d_bag_grads, d_grads_out, stream)); }
    // second-tier pass: fills only the positions an earlier find (on another table) left with d_found == 0
    void find_missing(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream = nullptr) const { check(mee_find_missing(t_, d_keys, n, d_out, d_found, stream)); }
    void insert(const int64_t* d_keys, const float* d_values, size_t n, void* stream = nullptr) { check(mee_insert(t_, d_keys, d_values, n, stream)); }
    void assign(const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_assign(t_, d_keys, d_values, n, d_found, stream)); }
    // rows of in_dtype (MEE_DTYPE_BF16: a bf16-row table stores the caller's bf16 rows verbatim; d_values 16-byte aligned)
    void insert_as(const int64_t* d_keys, const void* d_values, uint32_t in_dtype, size_t n, void* stream = nullptr) { check(mee_insert_as(t_, d_keys, d_values, in_dtype, n, stream)); }
    void assign_as(const int64_t* d_keys, const void* d_values, uint32_t in_dtype, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_assign_as(t_, d_keys, d_values, in_dtype, n, d_found, stream)); }
    void remove(const int64_t* d_keys, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_remove(t_, d_keys, n, d_found, stream)); }
    // tier migration (mee_move): the batch's keys that this table holds leave it for dst, rows and optimizer state; d_n_moved: one device word
    void move_to(Table& dst, const int64_t* d_keys, size_t n, uint64_t max_moves = UINT64_MAX, uint8_t* d_moved = nullptr, uint64_t* d_n_moved = nullptr, void* stream = nullptr) { check(mee_move(t_, dst.t_, d_keys, n, max_moves, d_moved, d_n_moved, stream)); }
    // eviction by the hit counters (mee_evict; MEE_FLAG_TRACK_HITS tables): up to max_evict keys hit at most max_hits times leave, their rows and state handed out; d_n_out: one device word
    void evict(uint32_t max_hits, uint64_t max_evict, uint32_t flags = 0, int64_t* d_keys_out = nullptr, float* d_values_out = nullptr, float* d_state1_out = nullptr, float* d_state2_out = nullptr, uint32_t* d_hits_out = nullptr, size_t cap = 0, uint64_t* d_n_out = nullptr, void* stream = nullptr) { check(mee_evict(t_, max_hits, max_evict, flags, d_keys_out, d_values_out, d_state1_out, d_state2_out, d_hits_out, cap, d_n_out, stream)); }
    void hits_find(const int64_t* d_keys, size_t n, uint32_t* d_hits_out, void* stream = nullptr) const { check(mee_hits_find(t_, d_keys, n, d_hits_out, stream)); }
    void hits_assign(const int64_t* d_keys, size_t n, const uint32_t* d_hits, void* stream = nullptr) { check(mee_hits_assign(t_, d_keys, n, d_hits, stream)); }
    void hits_decay(uint32_t shift = 1, void* stream = nullptr) { check(mee_hits_decay(t_, shift, stream)); }
    void find_or_insert(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_find_or_insert(t_, d_keys, n, d_out, d_found, stream)); }
    // the forward of a training step over a growing vocabulary: rows + the slot of every key, for apply_*_located of the same step
    void find_or_insert_located(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream = nullptr) { check(mee_find_or_insert_located(t_, d_keys, n, d_out, d_found, d_slots_out, stream)); }
    // forward + backward of one training step: the located lookup (prepare = true: its launch also partitions the batch for the apply of the
    // SAME d_keys / n that must follow — mee_find_located_prepare / mee_find_or_insert_located_prepare), then the update at the slots it found
    void find_located(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, bool prepare = false, void* stream = nullptr) {
        check(prepare ? mee_find_located_prepare(t_, d_keys, n, d_out, d_found, d_slots_out, stream) : mee_find_located(t_, d_keys, n, d_out, d_found, d_slots_out, stream));
    }
    void find_or_insert_located_prepare(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream = nullptr) { check(mee_find_or_insert_located_prepare(t_, d_keys, n, d_out, d_found, d_slots_out, stream)); }
    // the same lookups with fp32 or bf16 result rows (out_dtype = MEE_DTYPE_F32 | MEE_DTYPE_BF16: the fp32 result rounded once to bf16; d_out 8-byte aligned)
    void find_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, uint32_t flags = MEE_FIND_DEFAULT, void* stream = nullptr) const { check(mee_find_as(t_, d_keys, n, d_out, out_dtype, d_found, flags, stream)); }
    void find_located_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out, bool prepare = false, void* stream = nullptr) {
        check(prepare ? mee_find_located_prepare_as(t_, d_keys, n, d_out, out_dtype, d_found, d_slots_out, stream) : mee_find_located_as(t_, d_keys, n, d_out, out_dtype, d_found, d_slots_out, stream));
    }
    void find_or_insert_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_find_or_insert_as(t_, d_keys, n, d_out, out_dtype, d_found, stream)); }
    void find_or_insert_located_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out, bool prepare = false, void* stream = nullptr) {
        check(prepare ? mee_find_or_insert_located_prepare_as(t_, d_keys, n, d_out, out_dtype, d_found, d_slots_out, stream) : mee_find_or_insert_located_as(t_, d_keys, n, d_out, out_dtype, d_found, d_slots_out, stream));
    }
    // d_weights nullable (non-null: the weighted sum, whose d_located_out receives mee_find_located handles)
    void find_pooled_as(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const float* d_weights, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, int mode = MEE_POOL_SUM, void* stream = nullptr) const {
        check(mee_find_pooled_as(t_, d_keys, n, d_bag_offsets, n_bags, d_weights, d_out, out_dtype, d_found, d_located_out, mode, stream));
    }
    // padded sequence lookup: d_out [n_bags, max_len, dim] of out_dtype, zeros behind a short bag, a long bag cut to its first / last (flags = MEE_PAD_KEEP_*)
    // max_len keys; d_step_keys_out / d_grad_index_out are what apply_*_indexed over the dense grad needs.  Every output but d_out is nullable
    void find_padded_as(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, size_t max_len, uint32_t flags, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int64_t* d_lengths_out = nullptr, int64_t* d_step_keys_out = nullptr, uint32_t* d_grad_index_out = nullptr, void* stream = nullptr) const {
        check(mee_find_padded_as(t_, d_keys, n, d_bag_offsets, n_bags, max_len, flags, d_out, out_dtype, d_found, d_lengths_out, d_step_keys_out, d_grad_index_out, stream));
    }
    // ... over a hot/cold pair: this table is the HOT tier, `cold` the cold one (mee_find_padded_tiered): find_padded_as on the union of the two, one launch;
    // count_flags = MEE_TIER_COUNT_* (a word of its own: MEE_PAD_KEEP_LAST and MEE_TIER_COUNT_COLD are both 1)
    void find_padded_tiered(const Table& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, size_t max_len, uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int64_t* d_lengths_out = nullptr, int64_t* d_step_keys_out = nullptr, uint32_t* d_grad_index_out = nullptr, void* stream = nullptr) const {
        check(mee_find_padded_tiered(t_, cold.t_, d_keys, n, d_bag_offsets, n_bags, max_len, flags, count_flags, d_out, out_dtype, d_found, d_lengths_out, d_step_keys_out, d_grad_index_out, stream));
    }
    void apply_adagrad_located(const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) { check(mee_apply_adagrad_located(t_, d_keys, d_slots, d_grads, n, lr, eps, stream)); }
    void apply_adam_located(const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_apply_adam_located(t_, d_keys, d_slots, d_grads, n, lr, beta1, beta2, eps, step, stream));
    }
    void apply_discard(void* stream = nullptr) { check(mee_apply_discard(t_, stream)); }
    void find_plane(uint32_t plane, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found = nullptr, void* stream = nullptr) const { check(mee_find_plane(t_, plane, d_keys, n, d_out, d_found, stream)); }
    void assign_plane(uint32_t plane, const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_assign_plane(t_, plane, d_keys, d_values, n, d_found, stream)); }
    void apply_adagrad(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) { check(mee_apply_adagrad(t_, d_keys, d_grads, n, lr, eps, stream)); }
    void apply_adam(const int64_t* d_keys, const float* d_grads, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_apply_adam(t_, d_keys, d_grads, n, lr, beta1, beta2, eps, step, stream));
    }
    // backward of find_pooled: position i takes grad row d_grad_index[i] (its bag)
    void apply_adagrad_indexed(const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) {
        check(mee_apply_adagrad_indexed(t_, d_keys, d_grads, n_grad_rows, d_grad_index, n, lr, eps, stream));
    }
    void apply_adam_indexed(const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_apply_adam_indexed(t_, d_keys, d_grads, n_grad_rows, d_grad_index, n, lr, beta1, beta2, eps, step, stream));
    }
    // FTRL-Proximal (a table created with MEE_OPT_FTRL): by key, on the forward's slot handles, on indexed gradient rows
    void apply_ftrl(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) { check(mee_apply_ftrl(t_, d_keys, d_grads, n, lr, beta, l1, l2, stream)); }
    void apply_ftrl_located(const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_apply_ftrl_located(t_, d_keys, d_slots, d_grads, n, lr, beta, l1, l2, stream));
    }
    void apply_ftrl_indexed(const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_apply_ftrl_indexed(t_, d_keys, d_grads, n_grad_rows, d_grad_index, n, lr, beta, l1, l2, stream));
    }
    // the next four synchronise the stream (they return host values)
    size_t size(void* stream = nullptr) const { size_t n = 0; check(mee_size(t_, &n, stream)); return n; }
    uint32_t status(void* stream = nullptr) const { uint32_t b = 0; check(mee_status(t_, &b, stream)); return b; }
    size_t export_all(int64_t* d_keys_out, float* d_values_out, size_t cap, float* d_state1_out = nullptr, float* d_state2_out = nullptr, void* stream = nullptr) const {
        size_t n = 0; check(mee_export(t_, d_keys_out, d_values_out, d_state1_out, d_state2_out, cap, &n, stream)); return n;
    }
    // pairs stored in slots [slot_begin, slot_end): checkpoint / rehash in bounded pieces; returns how many the range holds
    size_t export_range(uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out, size_t cap, float* d_state1_out = nullptr, float* d_state2_out = nullptr, void* stream = nullptr) const {
        size_t n = 0; check(mee_export_range(t_, slot_begin, slot_end, d_keys_out, d_values_out, d_state1_out, d_state2_out, cap, &n, stream)); return n;
    }
    // sync-free: padded outputs of length n (MEE_EMPTY_KEY between the distinct keys, counts 0 there); see mee_dedup_sum
    void dedup_sum(const int64_t* d_keys, const float* d_grads, size_t n, int64_t* d_uniq_out, float* d_gsum_out, uint32_t* d_counts_out, int64_t* d_inverse_out,
                   int64_t miss_index = -1, void* stream = nullptr) {
        check(mee_dedup_sum(t_, d_keys, d_grads, n, d_uniq_out, d_gsum_out, d_counts_out, d_inverse_out, miss_index, stream));
    }
    // sync-free: d_uniq_out[n] = every distinct key once, EMPTY everywhere else (also between the keys), d_inverse_out[i] = index into it (miss_index for reserved keys)
    void dedup_keys(const int64_t* d_keys, size_t n, int64_t* d_uniq_out, int64_t* d_inverse_out, int64_t miss_index = -1, void* stream = nullptr) {
        check(mee_dedup_keys(t_, d_keys, n, d_uniq_out, d_inverse_out, miss_index, stream));
    }
    void clear(void* stream = nullptr) { check(mee_clear(t_, stream)); }
    // rehash in place to at least `capacity` slots (synchronises; old and new planes must fit together)
    void reserve(uint64_t capacity, void* stream = nullptr) { check(mee_reserve(t_, capacity, stream)); }
    void clear_status(void* stream = nullptr) { check(mee_clear_status(t_, stream)); }
    void set_tuning(const char* name, int value) { check(mee_set_tuning(t_, name, value)); }

private:
    mee_table* t_ = nullptr;
};

// Many tables (same device, same dim) served by ONE find launch over their concatenated ("jagged") key batches.
// Members that are all bf16-row tables (TableOptions::bf16_rows) make a bf16-row group, the serving form of a collection: max_apply_batch must be 0, the
// lookups (find, find_pooled without weights or located rows, the jagged form) are bit for bit the per-member lookups, and everything that trains —
// find_or_insert, apply_*, the weighted forms — throws MEE_ERR_UNSUPPORTED.  fp32-row and bf16-row tables never share a group.
class Group {
public:
    Group(Table* const* tables, uint32_t n, uint64_t max_apply_batch = 0) {
        std::string h(n * sizeof(mee_table*), '\0');
        auto** raw = reinterpret_cast<mee_table**>(&h[0]);
        for (uint32_t j = 0; j < n; ++j) raw[j] = tables[j]->handle();
        check(mee_group_create(raw, n, max_apply_batch, &g_));
    }
    ~Group() { if (g_) mee_group_destroy(g_); }
    Group(const Group&) = delete;
    Group& operator=(const Group&) = delete;
    mee_group* handle() const noexcept { return g_; }
    uint32_t value_dtype() const { uint32_t d = MEE_DTYPE_F32; check(mee_group_value_dtype(g_, &d)); return d; }   // MEE_DTYPE_BF16: a bf16-row group
    // segment j = d_keys[d_offsets[j] .. d_offsets[j+1]); d_offsets: n_tables + 1 values in DEVICE memory; n = total positions
    void find(const int64_t* d_keys, const uint64_t* d_offsets, size_t n, float* d_out, uint8_t* d_found, void* stream = nullptr) {
        check(mee_find_grouped(g_, d_keys, d_offsets, n, d_out, d_found, stream));
    }
    // the grouped lookups with fp32 or bf16 result rows (MEE_DTYPE_*): mee_find_grouped_as / mee_group_find_or_insert_as / mee_group_find_pooled_as
    void find_as(const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, void* stream = nullptr) { check(mee_find_grouped_as(g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream)); }
    void find_or_insert_as(const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, void* stream = nullptr) { check(mee_group_find_or_insert_as(g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, stream)); }
    // admission over the collection (mee_group_find_or_insert_admit): every member counts absent keys in its own sketch and creates a key once its
    // estimate reached min_count — or d_min_counts[member] (device, n_tables entries) when given; admission_decay ages every member's sketch
    void find_or_insert_admit(const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, uint32_t min_count,
                              const uint32_t* d_min_counts = nullptr, void* stream = nullptr) {
        check(mee_group_find_or_insert_admit(g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, min_count, d_min_counts, stream));
    }
    void admission_decay(uint32_t shift = 1, void* stream = nullptr) { check(mee_group_admission_decay(g_, shift, stream)); }
    void find_pooled_as(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_weights, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, int mode = MEE_POOL_SUM, void* stream = nullptr) {
        check(mee_group_find_pooled_as(g_, d_keys, n, d_bag_offsets, bags_per_table, d_weights, d_out, out_dtype, d_found, d_located_out, mode, stream));
    }
    // Table::find_padded_as of every member on its bags_per_table bags, one launch (bag b belongs to member b / bags_per_table)
    void find_padded_as(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, size_t max_len, uint32_t flags, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int64_t* d_lengths_out = nullptr, int64_t* d_step_keys_out = nullptr, uint32_t* d_grad_index_out = nullptr, void* stream = nullptr) {
        check(mee_group_find_padded_as(g_, d_keys, n, d_bag_offsets, bags_per_table, max_len, flags, d_out, out_dtype, d_found, d_lengths_out, d_step_keys_out, d_grad_index_out, stream));
    }
    // the keyed layout: one row per sample, the members' pooled vectors side by side ([bags_per_table, n_tables * dim]; out_row_stride in elements, 0 = that
    // width); d_step_index_out = the d_grad_index with which apply_*_pooled reads the keyed gradient in place (mee_group_find_pooled_keyed)
    void find_pooled_keyed(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, size_t out_row_stride = 0, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, uint32_t* d_step_index_out = nullptr, int mode = MEE_POOL_SUM, void* stream = nullptr) {
        check(mee_group_find_pooled_keyed(g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, out_row_stride, d_found, d_located_out, d_step_index_out, mode, stream));
    }
    // ... over a collection of hot/cold pairs (mee_group_find_pooled_tiered_keyed)
    void find_pooled_tiered_keyed(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, size_t out_row_stride = 0, uint8_t* d_found = nullptr, uint32_t* d_step_index_out = nullptr, int mode = MEE_POOL_SUM, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_pooled_tiered_keyed(g_, cold.g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, out_row_stride, d_found, d_step_index_out, mode, flags, stream));
    }
    void set_tuning(const char* name, int value) { check(mee_group_set_tuning(g_, name, value)); }   // knobs of the group's own apply; never change results
    void apply_adagrad(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) {
        check(mee_group_apply_adagrad(g_, d_keys, d_offsets, d_grads, n, lr, eps, stream));
    }
    void apply_adam(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_group_apply_adam(g_, d_keys, d_offsets, d_grads, n, lr, beta1, beta2, eps, step, stream));
    }
    // the weighted embedding-bag collection: bag b belongs to member b / bags_per_table (mee_group_find_pooled_weighted / mee_group_pooled_weighted_backward)
    void find_pooled_weighted(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_weights, float* d_out, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, void* stream = nullptr) { check(mee_group_find_pooled_weighted(g_, d_keys, n, d_bag_offsets, bags_per_table, d_weights, d_out, d_found, d_located_out, stream)); }
    void pooled_weighted_backward(const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_weights, const float* d_bag_grads, float* d_grads_out, float* d_weight_grads_out = nullptr, void* stream = nullptr) { check(mee_group_pooled_weighted_backward(g_, d_keys, d_located, n, d_bag_offsets, bags_per_table, d_weights, d_bag_grads, d_grads_out, d_weight_grads_out, stream)); }
    // max pooling over the collection (mee_group_find_pooled_max / mee_group_pooled_max_backward): argmax positions are absolute in the whole batch
    void find_pooled_max(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, uint32_t* d_argmax_out = nullptr, void* stream = nullptr) { check(mee_group_find_pooled_max(g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, d_argmax_out, stream)); }
    void pooled_max_backward(size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const uint32_t* d_argmax, const float* d_bag_grads, float* d_grads_out, void* stream = nullptr) { check(mee_group_pooled_max_backward(g_, n, d_bag_offsets, bags_per_table, d_argmax, d_bag_grads, d_grads_out, stream)); }
    // the collection with a different number of bags per member: bag b belongs to member j with d_member_bags[j] <= b < d_member_bags[j + 1]
    // (mee_group_find_pooled_jagged), and its backward, mee_apply_*_indexed per member (mee_group_apply_*_indexed)
    void find_pooled_jagged(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const uint64_t* d_member_bags, float* d_out, uint8_t* d_found = nullptr, int64_t* d_located_out = nullptr, int mode = MEE_POOL_SUM, void* stream = nullptr) {
        check(mee_group_find_pooled_jagged(g_, d_keys, n, d_bag_offsets, n_bags, d_member_bags, d_out, d_found, d_located_out, mode, stream));
    }
    void apply_adagrad_indexed(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) {
        check(mee_group_apply_adagrad_indexed(g_, d_keys, d_offsets, d_grads, n_grad_rows, d_grad_index, n, lr, eps, stream));
    }
    void apply_adam_indexed(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_group_apply_adam_indexed(g_, d_keys, d_offsets, d_grads, n_grad_rows, d_grad_index, n, lr, beta1, beta2, eps, step, stream));
    }
    // FTRL-Proximal over a group of MEE_OPT_FTRL tables: per position, pooled (a bag's grad row for each of its keys), indexed
    void apply_ftrl(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_group_apply_ftrl(g_, d_keys, d_offsets, d_grads, n, lr, beta, l1, l2, stream));
    }
    void apply_ftrl_pooled(const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads, const uint32_t* d_grad_index, const int64_t* d_located, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_group_apply_ftrl_pooled(g_, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_grad_index, d_located, n, lr, beta, l1, l2, stream));
    }
    void apply_ftrl_indexed(const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_group_apply_ftrl_indexed(g_, d_keys, d_offsets, d_grads, n_grad_rows, d_grad_index, n, lr, beta, l1, l2, stream));
    }
    // a collection of hot/cold pairs: this group holds the HOT tables, `cold` the cold ones, member j of both = pair j (mee_group_find_pooled_tiered /
    // mee_group_ensure_tiered).  One pooled launch over both tiers of every member; flags = MEE_TIER_COUNT_*.  ensure_tiered creates the keys d_found
    // marks as missing, member j in its cold table where d_to_cold[j] != 0 (null: all hot).
    void find_pooled_tiered(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int mode = MEE_POOL_SUM, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_pooled_tiered(g_, cold.g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, mode, flags, stream));
    }
    // ... with the members' bag counts read from d_member_bags [n_tables + 1] on the device (mee_group_find_pooled_tiered_jagged; fp32 out)
    void find_pooled_tiered_jagged(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const uint64_t* d_member_bags, float* d_out, uint8_t* d_found = nullptr, int mode = MEE_POOL_SUM, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_pooled_tiered_jagged(g_, cold.g_, d_keys, n, d_bag_offsets, n_bags, d_member_bags, d_out, d_found, mode, flags, stream));
    }
    // the padded sequence lookup over the same collection of pairs, one launch (mee_group_find_padded_tiered): Table::find_padded_tiered of pair
    // b / bags_per_table on bag b; flags = MEE_PAD_KEEP_*, count_flags = MEE_TIER_COUNT_*
    void find_padded_tiered(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, size_t max_len, uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int64_t* d_lengths_out = nullptr, int64_t* d_step_keys_out = nullptr, uint32_t* d_grad_index_out = nullptr, void* stream = nullptr) {
        check(mee_group_find_padded_tiered(g_, cold.g_, d_keys, n, d_bag_offsets, bags_per_table, max_len, flags, count_flags, d_out, out_dtype, d_found, d_lengths_out, d_step_keys_out, d_grad_index_out, stream));
    }
    void ensure_tiered(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const uint8_t* d_found, const uint8_t* d_to_cold = nullptr, void* stream = nullptr) {
        check(mee_group_ensure_tiered(g_, cold.g_, d_keys, n, d_bag_offsets, bags_per_table, d_found, d_to_cold, stream));
    }
    // the unpooled lookups over the same collection of pairs, a row per position of the jagged batch (mee_group_find_tiered: one launch;
    // mee_group_find_or_insert_tiered: two, d_found required = present before the call)
    void find_tiered(Group& cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_tiered(g_, cold.g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, flags, stream));
    }
    void find_or_insert_tiered(Group& cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, const uint8_t* d_to_cold = nullptr, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_or_insert_tiered(g_, cold.g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, d_to_cold, flags, stream));
    }
    // admission over the collection of pairs (each pair counts in its HOT table's sketch: this group's members need MEE_FLAG_ADMISSION, `cold`'s do not):
    // mee_group_find_or_insert_admit_tiered, three launches, and mee_group_ensure_admit_tiered, two; min_count, or d_min_counts[member] when given
    void find_or_insert_admit_tiered(Group& cold, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, uint32_t min_count, const uint32_t* d_min_counts = nullptr, const uint8_t* d_to_cold = nullptr, uint32_t flags = 0, void* stream = nullptr) {
        check(mee_group_find_or_insert_admit_tiered(g_, cold.g_, d_keys, d_offsets, n, d_out, out_dtype, d_found, d_to_cold, min_count, d_min_counts, flags, stream));
    }
    void ensure_admit_tiered(Group& cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const uint8_t* d_found, uint32_t min_count, const uint32_t* d_min_counts = nullptr, const uint8_t* d_to_cold = nullptr, void* stream = nullptr) {
        check(mee_group_ensure_admit_tiered(g_, cold.g_, d_keys, n, d_bag_offsets, bags_per_table, d_found, d_to_cold, min_count, d_min_counts, stream));
    }
    // mee_move per member on its segment of the jagged batch (mee_group_move); d_max_moves / d_n_moved: n_tables device words each, nullable
    void move_to(Group& dst, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, const uint64_t* d_max_moves = nullptr, uint8_t* d_moved = nullptr, uint64_t* d_n_moved = nullptr, void* stream = nullptr) {
        check(mee_group_move(g_, dst.g_, d_keys, d_offsets, n, d_max_moves, d_moved, d_n_moved, stream));
    }
private:
    mee_group* g_ = nullptr;
};

// An embedding-bag collection whose tables differ in dim: one pooled-lookup launch, class-major output (mee_mixed_group_*).
class MixedGroup {
public:
    MixedGroup(Table* const* tables, uint32_t n, uint64_t max_apply_batch = 0) : n_(n) {
        std::string h(n * sizeof(mee_table*), '\0');
        auto** raw = reinterpret_cast<mee_table**>(&h[0]);
        for (uint32_t j = 0; j < n; ++j) raw[j] = tables[j]->handle();
        check(mee_mixed_group_create(raw, n, max_apply_batch, &g_));
    }
    ~MixedGroup() { if (g_) mee_mixed_group_destroy(g_); }
    MixedGroup(const MixedGroup&) = delete;
    MixedGroup& operator=(const MixedGroup&) = delete;
    uint32_t size() const { return n_; }
    // element offset of every member's [bags_per_table, dim_j] block (elem_offsets: size() entries, nullable) -> the total element count
    uint64_t layout(uint64_t bags_per_table, uint64_t* elem_offsets = nullptr) const {
        uint64_t total = 0;
        check(mee_mixed_group_layout(g_, bags_per_table, elem_offsets, &total));
        return total;
    }
    void find_pooled(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, uint8_t* d_found = nullptr, int64_t* d_located = nullptr, int mode = MEE_POOL_SUM, bool insert_missing = false, void* stream = nullptr) {
        check(mee_mixed_group_find_pooled(g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, d_found, d_located, mode, insert_missing, stream));
    }
    void apply_adagrad_pooled(const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) {
        check(mee_mixed_group_apply_adagrad_pooled(g_, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, lr, eps, stream));
    }
    void apply_adam_pooled(const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr, uint64_t step, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, void* stream = nullptr) {
        check(mee_mixed_group_apply_adam_pooled(g_, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, lr, beta1, beta2, eps, step, stream));
    }
    void apply_ftrl_pooled(const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        check(mee_mixed_group_apply_ftrl_pooled(g_, d_keys, d_bag_offsets, bags_per_table, d_bag_grads, d_bag_of_position, d_located, n, lr, beta, l1, l2, stream));
    }
    // the keyed layout: member j's pooled vector at column col_offsets[j] of its sample's row (mee_mixed_group_keyed_layout -> the row's width in elements)
    uint64_t keyed_layout(uint64_t* col_offsets = nullptr) const {
        uint64_t width = 0;
        check(mee_mixed_group_keyed_layout(g_, col_offsets, &width));
        return width;
    }
    void find_pooled_keyed(const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out, uint32_t out_dtype = MEE_DTYPE_F32, size_t out_row_stride = 0, uint8_t* d_found = nullptr, int64_t* d_located = nullptr, uint32_t* d_step_index_out = nullptr, int mode = MEE_POOL_SUM, bool insert_missing = false, void* stream = nullptr) {
        check(mee_mixed_group_find_pooled_keyed(g_, d_keys, n, d_bag_offsets, bags_per_table, d_out, out_dtype, out_row_stride, d_found, d_located, d_step_index_out, mode, insert_missing, stream));
    }
    // the keyed gradient taken apart into the class-major fp32 buffer the step reads (mee_mixed_group_keyed_grads; d_bag_offsets with MEE_POOL_MEAN only)
    void keyed_grads(const void* d_keyed_grads, uint32_t in_dtype, size_t row_stride, size_t bags_per_table, const uint64_t* d_bag_offsets, int mode, float* d_bag_grads_out, void* stream = nullptr) {
        check(mee_mixed_group_keyed_grads(g_, d_keyed_grads, in_dtype, row_stride, bags_per_table, d_bag_offsets, mode, d_bag_grads_out, stream));
    }
    void set_tuning(const char* name, int value) { check(mee_mixed_group_set_tuning(g_, name, value)); }
private:
    mee_mixed_group* g_ = nullptr;
    uint32_t n_ = 0;
};

// Hot (HBM) table backed by a cold table whose rows live in pinned host DRAM: one logical table, sync-free lookup.
class TieredTable {
public:
    TieredTable(Table hot, Table cold) : hot_(std::move(hot)), cold_(std::move(cold)) {}
    Table& hot() noexcept { return hot_; }
    Table& cold() noexcept { return cold_; }
    void find(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream = nullptr) const {
        hot_.find(d_keys, n, d_out, d_found, stream);          // d_found is required: the second pass reads it
        cold_.find_missing(d_keys, n, d_out, d_found, stream);
    }
    void apply_adagrad(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) {
        hot_.apply_adagrad(d_keys, d_grads, n, lr, eps, stream);  // a key lives in one tier; each table ignores keys it does not hold
        cold_.apply_adagrad(d_keys, d_grads, n, lr, eps, stream);
    }
    void apply_ftrl(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float beta = 1.0f, float l1 = 0.0f, float l2 = 0.0f, void* stream = nullptr) {
        hot_.apply_ftrl(d_keys, d_grads, n, lr, beta, l1, l2, stream);
        cold_.apply_ftrl(d_keys, d_grads, n, lr, beta, l1, l2, stream);
    }
    size_t size(void* stream = nullptr) const { return hot_.size(stream) + cold_.size(stream); }
private:
    Table hot_, cold_;
};

// Shard partition / un-permute workspace (SPEC.md §5).
class Router {
public:
    Router(int32_t device, uint64_t max_batch, uint32_t n_shards) { check(mee_router_create(device, max_batch, n_shards, &r_)); }
    ~Router() { if (r_) mee_router_destroy(r_); }
    Router(Router&& o) noexcept : r_(std::exchange(o.r_, nullptr)) {}
    Router(const Router&) = delete;
    Router& operator=(const Router&) = delete;
    mee_router* handle() const noexcept { return r_; }
    void partition(const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts, int64_t* d_perm, void* stream = nullptr) { check(mee_partition(r_, d_keys, n, d_send_keys, d_counts, d_perm, stream)); }
    // the same, EMPTY keys (padding) belong to no shard
    void partition_padded(const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts, int64_t* d_perm, void* stream = nullptr) { check(mee_partition_padded(r_, d_keys, n, d_send_keys, d_counts, d_perm, stream)); }
    static void scatter_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out, void* stream = nullptr) { check(mee_scatter_rows(d_rows, d_perm, n, row_bytes, d_out, stream)); }
    static void gather_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out, void* stream = nullptr) { check(mee_gather_rows(d_rows, d_perm, n, row_bytes, d_out, stream)); }
private:
    mee_router* r_ = nullptr;
};

// Peer-mapped exchange context of the all-to-all-free sharded find.  The caller moves the exported handles between
// ranks (any side channel); the two cross-rank barriers per lookup are barrier() (or any collective on the stream):
// partition -> push -> barrier -> find -> barrier -> read rows()/found().
class PeerExchange {
public:
    PeerExchange(int32_t device, uint32_t n_shards, uint32_t rank, uint64_t slots_per_peer, uint64_t max_batch, uint32_t dim, bool with_payload = false) {
        check(mee_p2p_create(device, n_shards, rank, slots_per_peer, max_batch, dim, with_payload ? 1 : 0, &c_));
    }
    ~PeerExchange() { if (c_) mee_p2p_destroy(c_); }
    PeerExchange(const PeerExchange&) = delete;
    PeerExchange& operator=(const PeerExchange&) = delete;
    void export_handles(void* handles_6x64) { check(mee_p2p_export(c_, handles_6x64)); }
    void connect(const void* all_handles_rank_major) { check(mee_p2p_connect(c_, all_handles_rank_major)); }
    void push(Router& r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts, size_t n, void* stream = nullptr) { check(mee_p2p_push(c_, r.handle(), d_send_keys, d_perm, d_counts, n, stream)); }
    void find(const Table& t, void* stream = nullptr) { check(mee_p2p_find(c_, t.handle(), stream)); }
    // the cross-rank barrier of the sequences above as a one-wave kernel over peer-mapped flags (no collective library needed)
    void barrier(void* stream = nullptr) { check(mee_p2p_barrier(c_, stream)); }
    void push_rows(Router& r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts, const float* d_rows, size_t n, void* stream = nullptr) {
        check(mee_p2p_push_rows(c_, r.handle(), d_send_keys, d_perm, d_counts, d_rows, n, stream));
    }
    int64_t* inbox_keys() const { int64_t* k = nullptr; check(mee_p2p_inbox(c_, &k, nullptr, nullptr)); return k; }
    float* inbox_rows() const { float* r = nullptr; check(mee_p2p_inbox(c_, nullptr, &r, nullptr)); return r; }
    uint64_t inbox_slots() const { uint64_t n = 0; check(mee_p2p_inbox(c_, nullptr, nullptr, &n)); return n; }
    float* rows() const { float* o = nullptr; check(mee_p2p_buffers(c_, &o, nullptr)); return o; }
    uint8_t* found() const { uint8_t* f = nullptr; check(mee_p2p_buffers(c_, nullptr, &f)); return f; }
    uint32_t status(void* stream = nullptr) { uint32_t b = 0; check(mee_p2p_status(c_, &b, stream)); return b; }
private:
    mee_p2p* c_ = nullptr;
};

// An RCCL communicator made through the library (callers that link RCCL themselves pass their own ncclComm_t instead).
class Communicator {
public:
    static void unique_id(void* id_128_bytes) { check(mee_comm_unique_id(id_128_bytes)); }   // one rank calls, all ranks share the bytes
    Communicator(const void* id_128_bytes, uint32_t n_ranks, uint32_t rank, int32_t device) { check(mee_comm_create(id_128_bytes, n_ranks, rank, device, &c_)); }
    ~Communicator() { if (c_) mee_comm_destroy(c_); }
    Communicator(const Communicator&) = delete;
    Communicator& operator=(const Communicator&) = delete;
    void* handle() const noexcept { return c_; }   // an ncclComm_t
private:
    void* c_ = nullptr;
};

// One rank's view of the row-sharded table (SPEC.md §5): every verb is collective over the communicator's ranks and runs the
// whole exchange — partition, grouped ncclSend/ncclRecv, the local shard's operator, rows back, un-permute — on `stream`.
class ShardedTable {
public:
    // pad_slack = 0: exact message sizes (one host sync per call); >= 1: fixed EMPTY-padded segments, no host sync
    ShardedTable(Table& local, void* nccl_comm, uint64_t max_batch, double pad_slack = 0.0) { check(mee_sharded_create(local.handle(), nccl_comm, max_batch, pad_slack, &s_)); }
    // with options: a cold table behind `local` (every shard a hot/cold pair), pre-exchange dedup of lookups (MEE_SHARDED_DEDUP)
    ShardedTable(Table& local, void* nccl_comm, uint64_t max_batch, double pad_slack, Table* cold, uint32_t flags = 0, uint64_t hot_key_limit = 0) {
        mee_sharded_options o{};
        o.struct_size = sizeof o; o.flags = flags; o.max_batch = max_batch; o.pad_slack = pad_slack; o.cold = cold ? cold->handle() : nullptr; o.hot_key_limit = hot_key_limit;
        check(mee_sharded_create_ex(local.handle(), nccl_comm, &o, &s_));
    }
    ~ShardedTable() { if (s_) mee_sharded_destroy(s_); }
    ShardedTable(const ShardedTable&) = delete;
    ShardedTable& operator=(const ShardedTable&) = delete;
    void find(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_find(s_, d_keys, n, d_out, d_found, stream)); }
    void find_or_insert(const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_find_or_insert(s_, d_keys, n, d_out, d_found, stream)); }
    // the lookups with fp32 or bf16 result rows (MEE_DTYPE_*; bf16: the owner rounds, half the row bytes travel; the same out_dtype on every rank)
    void find_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_find_as(s_, d_keys, n, d_out, out_dtype, d_found, stream)); }
    void find_or_insert_as(const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_find_or_insert_as(s_, d_keys, n, d_out, out_dtype, d_found, stream)); }
    // bytes handed to ncclSend / ncclRecv since creation (host counters, no synchronisation)
    void traffic(uint64_t* sent_bytes, uint64_t* received_bytes) const { check(mee_sharded_traffic(s_, sent_bytes, received_bytes)); }
    void insert(const int64_t* d_keys, const float* d_values, size_t n, void* stream = nullptr) { check(mee_sharded_insert(s_, d_keys, d_values, n, stream)); }
    void assign(const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_assign(s_, d_keys, d_values, n, d_found, stream)); }
    void remove(const int64_t* d_keys, size_t n, uint8_t* d_found = nullptr, void* stream = nullptr) { check(mee_sharded_remove(s_, d_keys, n, d_found, stream)); }
    void apply_adagrad(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float eps = 1e-10f, void* stream = nullptr) { check(mee_sharded_apply_adagrad(s_, d_keys, d_grads, n, lr, eps, stream)); }
    void apply_adam(const int64_t* d_keys, const float* d_grads, size_t n, float lr, float b1, float b2, float eps, uint64_t step, void* stream = nullptr) { check(mee_sharded_apply_adam(s_, d_keys, d_grads, n, lr, b1, b2, eps, step, stream)); }
    size_t size(void* stream = nullptr) { size_t n = 0; check(mee_sharded_size(s_, &n, stream)); return n; }
    uint32_t status(void* stream = nullptr) { uint32_t b = 0; check(mee_sharded_status(s_, &b, stream)); return b; }
    void clear_status(void* stream = nullptr) { check(mee_sharded_clear_status(s_, stream)); }
private:
    mee_sharded* s_ = nullptr;
};

// A change log (SPEC.md §3 "Change log"): the set of keys noted since it was last cleared, and the delta of a table over it.  Move-only.
class ChangeLog {
public:
    ChangeLog(int32_t device, uint64_t capacity) { check(mee_changes_create(device, capacity, &c_)); }
    ~ChangeLog() { if (c_) mee_changes_destroy(c_); }
    ChangeLog(ChangeLog&& other) noexcept : c_(std::exchange(other.c_, nullptr)) {}
    ChangeLog& operator=(ChangeLog&& other) noexcept { if (this != &other) { if (c_) mee_changes_destroy(c_); c_ = std::exchange(other.c_, nullptr); } return *this; }
    ChangeLog(const ChangeLog&) = delete;
    ChangeLog& operator=(const ChangeLog&) = delete;
    mee_changes* handle() const noexcept { return c_; }
    void note(const int64_t* d_keys, size_t n, void* stream = nullptr) { check(mee_changes_note(c_, d_keys, n, stream)); }
    mee_changes_info info() const { mee_changes_info i{}; check(mee_changes_info_get(c_, &i)); return i; }   // [syncs]
    void clear(void* stream = nullptr) { check(mee_changes_clear(c_, stream)); }
    void invalidate(void* stream = nullptr) { check(mee_changes_invalidate(c_, stream)); }
    // the delta of `t` over the log's slots [slot_begin, slot_end): upserts (keys, rows, planes) and removed keys; d_counts_out: two device words
    void export_changed(const Table& t, uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out, float* d_state1_out, float* d_state2_out, size_t cap,
                        int64_t* d_removed_out, size_t removed_cap, uint64_t* d_counts_out, void* stream = nullptr) const {
        check(mee_export_changed(t.handle(), c_, slot_begin, slot_end, d_keys_out, d_values_out, d_state1_out, d_state2_out, cap, d_removed_out, removed_cap, d_counts_out, stream));
    }
    // the delta of `src` over the log's slots [slot_begin, slot_end) straight into the serving table `dst` (SPEC.md §3 "Publish"): no buffer, no
    // synchronisation; d_counts_out: four device words (placed, absent from src, dropped for lack of room, the log's invalid word)
    void publish(const Table& src, Table& dst, uint64_t slot_begin, uint64_t slot_end, uint64_t* d_counts_out, void* stream = nullptr) const {
        check(mee_publish_changed(src.handle(), c_, dst.handle(), slot_begin, slot_end, d_counts_out, stream));
    }
private:
    mee_changes* c_ = nullptr;
};

// One note launch for the logs of a table group: position i of segment j of a jagged batch is noted in logs[j].  Move-only; the logs outlive it.
class ChangeLogGroup {
public:
    ChangeLogGroup(mee_changes* const* logs, uint32_t n_tables) { check(mee_changes_group_create(logs, n_tables, &g_)); }
    ~ChangeLogGroup() { if (g_) mee_changes_group_destroy(g_); }
    ChangeLogGroup(ChangeLogGroup&& other) noexcept : g_(std::exchange(other.g_, nullptr)) {}
    ChangeLogGroup& operator=(ChangeLogGroup&& other) noexcept { if (this != &other) { if (g_) mee_changes_group_destroy(g_); g_ = std::exchange(other.g_, nullptr); } return *this; }
    ChangeLogGroup(const ChangeLogGroup&) = delete;
    ChangeLogGroup& operator=(const ChangeLogGroup&) = delete;
    void note(const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* stream = nullptr) { check(mee_changes_group_note(g_, d_keys, d_offsets, n, stream)); }
    // ChangeLog::publish for every member over the whole of its log, in one launch sequence; d_counts_out: n_tables x 4 device words
    void publish(const Group& src, Group& dst, uint64_t* d_counts_out, void* stream = nullptr) const { check(mee_group_publish_changed(src.handle(), g_, dst.handle(), d_counts_out, stream)); }
private:
    mee_changes_group* g_ = nullptr;
};

}  // namespace meepo
