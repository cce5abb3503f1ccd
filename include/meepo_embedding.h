/*
 * meepo_embedding.h — C-ABI of the MI355X (gfx950) GPU backend for a dynamic lookup-table embedding.
 *
 * Drop-in boundary.  The reference snapshot defines NO interface for this path: its only functional
 * statement is /root/reference/README.md:2 ("A distributed high-performance dynamic lookuptable-style
 * Embedding … Supports GPU, CPU, remote distributed KV (such as Redis), SSD, and other backends").  The verbs
 * below (find / insert / assign / export + sparse Adagrad/Adam apply) are the ones BASELINE.json's north_star
 * names for the GPU backend; each entry point cites README.md:2 as the (only) reference anchor and SPEC.md
 * for the semantics it implements.  A maintainer's binding stub is shown in INTEGRATION.md.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no C++/torch types.  `stream` is a hipStream_t passed as void*
 *    (NULL = the default stream).
 *  - Every `d_*` pointer is DEVICE memory on the table's device, caller-owned, and must stay valid until the
 *    stream reaches the op.  The library never frees or retains caller buffers.
 *  - All ops are asynchronous and stream-ordered unless marked [syncs].  No op allocates device memory after
 *    mee_table_create() (safe for hipGraph capture except the [syncs] ones).
 *  - Captured finds: under stream capture, consecutive plain finds of ONE table (mee_find / mee_find_ex / mee_find_plane, fp32 rows and fp32
 *    output) with nothing else captured on the stream between them may share ONE kernel node of the graph instead of one node each (the
 *    per-launch latency is then paid once per node; up to 16 requests per node, and only requests whose output and key buffers are disjoint
 *    from each other's).  What a replay leaves in memory is exactly what the chained launches leave; a capture sees fewer kernel nodes and
 *    the kernel name find_many_kernel where an eager launch runs find_kernel.  mee_set_tuning("find_coalesce", 0), or MEE_FIND_COALESCE=0 in
 *    the environment when the library is loaded, gives every captured find a node of its own; mee_find_capture_stats counts both kinds.
 *  - Return value: MEE_OK or a negative error code; mee_last_error() gives a thread-local message.
 *    Device-side conditions (table full, reserved key in a batch) set sticky bits read by mee_status().
 *  - Mutators (insert/assign/find_or_insert/apply_*), the duplicate reductions (dedup_keys/dedup_sum: they use the table's per-batch
 *    scratch) AND the [syncs] calls (size/status/export/hits_scan/probe_length: they share the table's counter block and its pinned
 *    read-back word) on ONE table must be ordered
 *    by the caller (same stream or events; from several host threads: one such call at a time per table);
 *    concurrent mee_find* calls on different streams / threads are safe.  n must be ≤ config.max_batch for
 *    every op except mee_find (any n).
 *  - There is no CPU fallback: creating a table without a usable gfx950 device fails with MEE_ERR_NO_DEVICE.
 */
#ifndef MEEPO_EMBEDDING_H
#define MEEPO_EMBEDDING_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MEE_ABI_VERSION 2   /* 2: mee_dedup_sum is sync-free and padded (round 5) */

#define MEE_EMPTY_KEY     INT64_MIN       /* SPEC.md §2: reserved, never stored; in a batch it is padding (skipped silently) */
#define MEE_RECLAIMED_KEY (INT64_MIN + 1) /* SPEC.md §2: reserved, the tombstone mee_remove leaves */
#define MEE_BUCKET_WIDTH  16              /* keys per bucket = one 128-byte line */

enum { MEE_OK = 0, MEE_ERR_INVALID_ARG = -1, MEE_ERR_OUT_OF_MEMORY = -2, MEE_ERR_HIP = -3,
       MEE_ERR_NO_DEVICE = -4, MEE_ERR_BATCH_TOO_LARGE = -5, MEE_ERR_UNSUPPORTED = -6,
       MEE_ERR_RCCL = -7 /* an RCCL call failed, or librccl.so.1 could not be loaded */ };

enum { MEE_OPT_NONE = 0, MEE_OPT_ADAGRAD = 1, MEE_OPT_ADAM = 2, MEE_OPT_FTRL = 3 };   /* state planes: none | acc | m, v | z, n (FTRL-Proximal: mee_apply_ftrl) */
enum { MEE_INIT_CONSTANT = 0, MEE_INIT_UNIFORM = 1 };
/* MEE_STATUS_STALE_HANDLE: mee_apply_*_located met a slot handle made before the table's latest mee_remove / mee_clear / mee_reserve; such
 * positions receive no update (the slot may hold another key by now).
 * MEE_STATUS_INTERNAL: a per-batch scratch area that is sized so that no batch can exhaust it was exhausted after all (a defect of the library:
 * the batch's updates are not to be trusted); never observed, reported rather than hidden. */
enum { MEE_STATUS_TABLE_FULL = 1u, MEE_STATUS_RESERVED_KEY = 2u, MEE_STATUS_STALE_HANDLE = 4u, MEE_STATUS_INTERNAL = 8u };
/* MEE_MEM_HOST_PINNED: rows in pinned, device-mapped host DRAM, read and written by the same kernels over PCIe — the
 * cold tier of a hot/cold pair (BASELINE configs[4]); see meepoembedding_amd/tiered.py. */
enum { MEE_MEM_HBM = 0, MEE_MEM_HOST_PINNED = 1 };
/* MEE_FLAG_TRACK_HITS: keep a per-slot access counter (4 B/slot) fed by mee_find_counted and read by mee_hits_scan —
 * the statistics a hot/cold placement policy needs. */
/* MEE_FLAG_ADMISSION: keep a count-min sketch (3 x max(2^12, capacity / 16 rounded up to a power of two) 32-bit counters) of how
 * often ABSENT keys were asked for — the state of the admission policy of mee_find_or_insert_admit (SPEC.md §3). */
/* MEE_FLAG_BF16_ROWS: the value plane holds bf16 rows, 2 x dim bytes per slot — a SERVING table (SPEC.md §3 "Row storage type"): writes round
 * each fp32 element once to bfloat16 (the rule of "typed output" below), reads widen exactly, and everything observable is that of an fp32
 * table that was handed the rounded rows and created with the rounded default_value.  Needs optimizer = MEE_OPT_NONE, dim a multiple of 8,
 * MEE_MEM_HBM and neither of the two flags above (MEE_ERR_INVALID_ARG otherwise).  The operators it has: mee_find / _ex / _as, mee_find_pooled
 * and mee_find_pooled_as without weights, mee_insert / mee_assign and their _as forms, mee_remove, mee_locate, mee_export / _range (fp32 out,
 * widened), mee_reserve, mee_clear, mee_size / mee_status / mee_clear_status, mee_probe_length / _histogram, mee_dedup_keys, mee_table_info_get
 * (table_bytes = capacity x (8 + 2 x dim)), mee_set_tuning, mee_table_plane (plane 0, row_stride_bytes = 2 x dim) and mee_table_value_dtype.
 * Every other operator handed such a table — and every other create that takes tables — returns MEE_ERR_UNSUPPORTED, launches nothing and writes
 * nothing.  The one create that takes them is mee_group_create, for a group whose members are ALL bf16-row tables (a serving group: see "table groups"). */
/* MEE_FLAG_INT8_ROWS: the value plane holds int8 rows — dim two's-complement codes followed by a 16-byte tail (the row's fp32 scale, then twelve zero
 * bytes), dim + 16 bytes per slot: the other SERVING table (SPEC.md §3 "Row storage type").  A written fp32 row x is quantized once, in fp32, nothing
 * contracted: scale = max|x_i| / 127 (one correctly rounded division), q_i = clamp(rint(x_i / scale), -127, 127) with ties to even, every code 0 when
 * scale == 0; a read gives y_i = (float)q_i * scale.  Everything observable is that of an fp32 table that was handed the rows D(Q(x)) and created with the
 * same default_value (fp32, not quantized: a missing key's row).  Rows must be finite: a row holding NaN or +-inf gives unspecified values in that row and
 * touches nothing else.  Create-time rules as for MEE_FLAG_BF16_ROWS (MEE_ERR_INVALID_ARG otherwise): optimizer = MEE_OPT_NONE, MEE_MEM_HBM, neither
 * MEE_FLAG_TRACK_HITS nor MEE_FLAG_ADMISSION, not together with MEE_FLAG_BF16_ROWS, and dim a multiple of 16.  The operators it has are those of a
 * bf16-row table WITHOUT the pooled lookups (mee_find_pooled / _as: MEE_ERR_UNSUPPORTED), and with fp32 input only: mee_insert_as / mee_assign_as take
 * MEE_DTYPE_F32 (MEE_DTYPE_BF16: MEE_ERR_UNSUPPORTED), mee_find / _ex / _as write fp32 or bf16 rows (a bf16 result rounds y once, by the rule of
 * "typed output"), mee_export / _range write dequantized fp32 rows, mee_reserve moves rows verbatim; mee_table_info_get: table_bytes = capacity x (8 + dim + 16), workspace_bytes = an fp32 table's
 * + max_batch x (dim + 16); mee_table_plane: plane 0, row_stride_bytes = dim + 16; mee_table_value_dtype: MEE_DTYPE_INT8.  Every other operator handed
 * such a table — and EVERY create that takes tables, mee_group_create included — returns MEE_ERR_UNSUPPORTED, launches nothing and writes nothing. */
enum { MEE_FLAG_TRACK_HITS = 1u, MEE_FLAG_ADMISSION = 2u, MEE_FLAG_BF16_ROWS = 4u, MEE_FLAG_INT8_ROWS = 8u };

typedef struct mee_table  mee_table;  /* one HBM-resident hash table (one shard) */
typedef struct mee_router mee_router; /* workspace for the shard partition / un-permute kernels */
typedef struct mee_p2p    mee_p2p;    /* peer-mapped buffers of the all-to-all-free sharded find */
typedef struct mee_sharded mee_sharded; /* one rank's context of the row-sharded table: local shard + RCCL communicator */
#define MEE_IPC_HANDLE_BYTES 64

typedef struct mee_config {
    uint32_t struct_size;         /* = sizeof(mee_config); ABI guard */
    int32_t  device;              /* HIP device ordinal */
    uint64_t capacity;            /* requested slots; rounded up to 16 x (smallest prime >= capacity/16) (SPEC.md §2) */
    uint32_t dim;                 /* floats per row: multiple of 4, 4..1024 (MEE_FLAG_BF16_ROWS: multiple of 8; MEE_FLAG_INT8_ROWS: of 16) */
    uint32_t optimizer;           /* MEE_OPT_*: which state planes to allocate (Adagrad one; Adam and FTRL two) */
    uint64_t max_batch;           /* largest n of any mutating op: sizes the workspace — with an optimizer ~(56 + 10 dim) B per position of HBM
                                   * (0.7 GB at 1M x dim 64: the pending records of a skewed batch's worst case); see mee_table_info.workspace_bytes */
    float    default_value;       /* fill for rows of absent keys */
    float    initial_accumulator; /* Adagrad acc, FTRL n of a newly inserted key */
    uint32_t initializer;         /* MEE_INIT_*: initial row for find_or_insert */
    float    init_scale;
    uint64_t init_seed;
    uint32_t value_memory;        /* MEE_MEM_*: where the value/state planes live (the key plane is always in HBM) */
    uint32_t flags;               /* MEE_FLAG_* bits, 0 by default */
} mee_config;

typedef struct mee_table_info {
    uint64_t capacity, n_buckets, max_batch;
    uint32_t dim, optimizer;
    uint64_t table_bytes;     /* keys + all planes resident in HBM (a bf16-row table: capacity x (8 + 2 x dim); an int8-row table: capacity x (8 + dim + 16)) */
    uint64_t workspace_bytes;
} mee_table_info;

int         mee_abi_version(void);
const char* mee_last_error(void);

/* ---- table lifetime (README.md:2 "GPU … backend"; SPEC.md §2) ------------------------------------------ */
int mee_table_create(const mee_config* cfg, mee_table** out);
int mee_table_destroy(mee_table* t);
int mee_table_info_get(const mee_table* t, mee_table_info* out);
int mee_clear(mee_table* t, void* stream);
/* performance knobs; never change results.  "find_rounds" (keys in flight per 16-lane tile: 1/2/4/8), "find_grid_cap" (max blocks of
 * the find grid, 0 = unbounded), "find_nt" (cache policy of a find: bit 0 streaming row loads, bit 1 streaming bucket loads, bit 2 cached
 * stores of the dense output; -1 = the library's rule: cached loads; cached stores while one call's output is <= 128 MB and the table's latest
 * lookups wrote to one buffer, streaming stores once their output buffers rotate (the distinct buffers of the last eight calls exceed 64 MB);
 * prefer mee_find_ex: the hint with the CALL), "find_coalesce" (1 = consecutive plain finds of a stream capture may share a kernel node — "captured
 * finds" above —, 0 = one node per call; default 1),
 * "apply_bucket_max" (target positions per bucket of the apply, 1..352; 0 = the library's rule: one bucket per resident block slot, as many
 * rounds as the batch needs; the bucket COUNT never exceeds what the table's scratch was sized for at creation — the default rule at max_batch —, so a
 * small value on a batch near max_batch gives larger buckets than asked for), "apply_kernel" (-1 = the library's choice by the stream's skew, 0 = LEAN,
 * 1 = FULL: meepo_apply.hip), "apply_skew_adapt" (0: the partition ignores the latest batch's skew report), "apply_xcd_split" (1..1023: share per 1024 of a
 * bucket pair's hash range that goes to the even bucket — even and odd XCDs differ in read-modify-write rate —, 0 = even halves; -1 = as calibrated on this
 * device when its first table was created).  Unknown names: MEE_ERR_INVALID_ARG. */
int mee_set_tuning(mee_table* t, const char* name, int value);
/* What the library measured on `device` when the first table with an optimizer was created there (or measures now): the apply's blocks run on the XCD their index
 * picks, and one parity's read-modify-write stream can be slower than the other's.  A probe kernel with the apply's access pattern is timed by block-index parity
 * (three launches, the first discarded); "apply_xcd_split" defaults to the share that equalises the two — 0 (even halves) unless both measured launches put the same
 * parity at least 5 % behind and blocks b and b + 8 were seen on one XCD throughout.  The environment variable MEE_XCD_SPLIT pins the value (0..1023). */
typedef struct mee_calibration {
    uint32_t struct_size;                 /* = sizeof(mee_calibration) */
    uint32_t xcd_split;                   /* the value tables on this device start with (0 = even halves) */
    uint32_t from_env;                    /* 1: MEE_XCD_SPLIT, nothing was measured */
    uint32_t placement_consistent;        /* 1: in both measured launches, blocks b and b + 8 ran on the same XCD */
    float    odd_over_even[2];            /* mean block time of odd-indexed blocks / even-indexed blocks, per measured launch */
    float    block_us_by_index_mod_8[8];  /* last launch: mean block time by block index mod 8 */
    uint32_t xcc_of_index_mod_8[8];       /* last launch: the XCC id blocks 0..7 reported */
} mee_calibration;
int mee_device_calibration(int32_t device, mee_calibration* out);

/* ---- lookup-table operators (README.md:2 "lookuptable-style"; SPEC.md §3) ------------------------------ */
/* out[i,:] = row of keys[i] or default_value; found nullable. */
int mee_find(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream);
/* mee_find with the cache policy of THIS call in `flags` (never changes results).  Hints are per request, not per table: two request
 * queues with different access patterns share one table without touching anything the other one's calls read (mee_set_tuning("find_nt")
 * stays as the table's default for callers that pass MEE_FIND_DEFAULT and for mee_find).
 *   MEE_FIND_STREAM_STORES  the dense output is not re-read from cache (result buffers that rotate, outputs beyond the Infinity Cache): the rows
 *                           leave as non-temporal stores (write-through stores were measured and are slower: profiles/find_write_through.md)
 *   MEE_FIND_CACHED_STORES  the opposite: keep the output cached whatever its size (at most one of the two; neither = the library's rule: cached
 *                           while one call's output is <= 128 MB and the table's latest lookups did not rotate over output buffers)
 *   MEE_FIND_STREAM_ROWS    rows are not looked up again soon (uniform streams over a table far larger than the caches); a skewed stream
 *                           wants its hot rows cached and must not set it
 *   MEE_FIND_STREAM_BUCKETS the same for the 128-byte key lines */
enum { MEE_FIND_DEFAULT = 0u, MEE_FIND_STREAM_STORES = 1u, MEE_FIND_CACHED_STORES = 2u, MEE_FIND_STREAM_ROWS = 4u, MEE_FIND_STREAM_BUCKETS = 8u };
int mee_find_ex(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, uint32_t flags, void* stream);
/* mee_find whose launch is NOT ordered behind earlier work of `stream` (hipExtAnyOrderLaunch): it may begin while previous kernels of
 * the stream are still running, so consecutive lookups on one stream overlap their launch latency (measured on MI355X: 32.3 -> 30.8 us
 * per 256K-key lookup).  The caller guarantees that d_keys is complete before the call is issued to the device and that nothing
 * earlier in the stream still reads or writes d_out / d_found (independent requests with buffers of their own).  Work submitted to the
 * stream AFTER it is ordered behind it as usual.  Same results as mee_find. */
int mee_find_unordered(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream);
/* Several lookup requests of ONE table in one launch (a server draining its request queue): request q is exactly
 * mee_find(t, reqs[q].d_keys, reqs[q].n, reqs[q].d_out, reqs[q].d_found) (d_found nullable).  `reqs` is a HOST array of at most 16
 * entries (read during the call; the buffers it names are device memory).  The per-launch latency floor is paid once: four
 * 256K-key requests cost what one 1M-key lookup costs. */
typedef struct mee_find_request { const int64_t* d_keys; size_t n; float* d_out; uint8_t* d_found; } mee_find_request;
int mee_find_many(const mee_table* t, const mee_find_request* reqs, uint32_t count, void* stream);
/* Read-only statistics of the rule "captured finds" above: how many plain finds of `t` issued under stream capture got a kernel node of their own
 * (*nodes) and how many joined the node of the find in front of them (*merged), since the table was created.  Eager calls count as neither. */
int mee_find_capture_stats(const mee_table* t, uint64_t* nodes, uint64_t* merged);
/* mee_find that also reports where each key lives: d_slots_out[i] = an opaque slot handle, -1 for absent / reserved keys.  The
 * handles feed mee_apply_*_located of the SAME training step (forward find -> backward apply) and stay valid only until the next
 * call that can move or free a row of this table (mee_remove, mee_clear, mee_reserve; inserting OTHER keys is fine).  A handle carries
 * the table's layout epoch (bits 40..61; bits 0..39 = the slot mee_locate reports): mee_apply_*_located skips handles of an earlier
 * epoch and raises MEE_STATUS_STALE_HANDLE, so a kept-too-long handle can never update another key's row. */
int mee_find_located(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream);
/* The training forward: mee_find_located + mee_apply_prepare for the same keys in ONE launch.  The grad-independent half of the step's
 * backward (the partition of the batch by hash bucket: latency-bound, 15-18 us per 256K keys) is run by the launch's first blocks beside the
 * row gather (bound by bytes, twice as long), so the following mee_apply_*_located(d_keys, d_slots_out, …) with the SAME d_keys / n starts
 * with its update kernel.  Same rules as mee_apply_prepare while the prepared apply is pending (mee_apply_discard drops it); tables without
 * an optimizer: plain mee_find_located. */
int mee_find_located_prepare(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream);
/* The same for a growing vocabulary: mee_find_or_insert_located whose first launch also carries the partition (absent keys are then created by
 * its second pass exactly as in mee_find_or_insert_located; d_found = present BEFORE the call, nullable). */
int mee_find_or_insert_located_prepare(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream);
/* second-tier pass after a mee_find on another table (same keys/out/found buffers): positions with d_found[i] == 0
 * that THIS table holds get their row and d_found[i] = 1; every other position is left untouched.  No host sync, no
 * compaction: this is how a hot (HBM) table is backed by a cold (pinned host) one inside one stream. */
int mee_find_missing(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream);
/* mee_find (missing_only = 0) or mee_find_missing (missing_only = 1) that also adds 1 to the hit counter of every key
 * it finds.  Meant for SAMPLED calls on a hot table (one atomic per found key) and for every call on a cold table (its
 * hits are PCIe-bound anyway).  d_found is required. */
int mee_find_counted(const mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int missing_only,
                     void* stream);
/* [syncs] keys whose hit counter lies in [min_hits, max_hits] (at most cap are written; *n_out = how many qualified);
 * reset != 0 zeroes every counter, which starts a new observation window. */
int mee_hits_scan(mee_table* t, uint32_t min_hits, uint32_t max_hits, int reset, int64_t* d_keys_out, size_t cap, size_t* n_out,
                  void* stream);
/* Eviction by the hit counters (SPEC.md §3 evict; tables created with MEE_FLAG_TRACK_HITS): make room in a table that is filling up, and hand the
 * evicted keys' rows and optimizer state out so that a tier behind this one can take them.
 * C = the stored keys whose counter is <= max_hits when the call starts; L = max_evict, or min(max_evict, cap) when at least one of the five output
 * buffers is non-null (a key is never evicted without its row being handed out when a row was asked for); m = min(|C|, L).  The call evicts a set
 * E of m keys of C.  Without MEE_EVICT_LEAST which keys of C are taken is unspecified when |C| > m (as for mee_hits_scan's cap).  With
 * MEE_EVICT_LEAST every evicted counter is <= every counter of C \ E, compared as full 32-bit values: the evicted counters are exactly the m
 * smallest of C, and only the choice among keys that tie at the cut is unspecified.
 * An evicted key's slot becomes RECLAIMED and its counter 0: mee_find reports it absent, mee_size drops by m, and the table is otherwise what
 * mee_remove(E) leaves (probe rule, tombstone reuse, key-sorted export with state); the keys that stay keep rows, state and counters bit for bit.
 * MEE_EVICT_RESET: every counter is zero after the selection has been made (a new observation window).
 * Outputs (all DEVICE memory, all nullable, `cap` entries / rows each): positions 0 .. m-1 of every non-null buffer describe E, each key once, in one
 * unspecified order shared by all buffers — the key, its values row, its acc | m and v rows bit for bit, its counter before the call.  A state
 * buffer for a plane the table lacks is ignored, as mee_export ignores it.  *d_n_out (one DEVICE word, nullable) = m.  max_evict == 0 evicts
 * nothing, writes 0 and still honours MEE_EVICT_RESET.  The status word is not touched.
 * Host side as mee_remove: slot handles taken before the call are stale, a partition a training forward left pending is dropped; a pending
 * mee_apply_prepare is MEE_ERR_INVALID_ARG, like unknown flag bits and a null table; a table without MEE_FLAG_TRACK_HITS, or with bf16 or int8
 * rows, is MEE_ERR_UNSUPPORTED — all refused before anything is launched or written.  MEE_MEM_HBM or MEE_MEM_HOST_PINNED.
 * No host synchronisation, no allocation, nothing read back: capturable.  Launches: the zeroing of the operator's counter words and ONE launch that
 * selects, hands out and tombstones; with MEE_EVICT_LEAST the zeroing and FOUR launches (three histogram passes of an exact radix select over the
 * counters, 10 + 11 + 11 bits from the top, then the eviction), whatever the table holds.  Each pass reads the key and counter planes once. */
enum { MEE_EVICT_LEAST = 1u, MEE_EVICT_RESET = 2u };
int mee_evict(mee_table* t, uint32_t max_hits, uint64_t max_evict, uint32_t flags, int64_t* d_keys_out, float* d_values_out,
              float* d_state1_out, float* d_state2_out, uint32_t* d_hits_out /* all five nullable */, size_t cap,
              uint64_t* d_n_out /* device, one word, nullable */, void* stream);
/* The hit counters by key (MEE_FLAG_TRACK_HITS tables; n <= max_batch; no synchronisation) — what carries LFU state through a checkpoint or a tier
 * move, and ages it.  mee_hits_find: d_hits_out[i] = the counter of d_keys[i], 0 for an absent or reserved key.  mee_hits_assign: the counter of
 * every present key becomes d_hits[i]; absent and reserved keys are ignored; a key twice in the batch keeps one of its values, which is
 * unspecified.  mee_hits_decay: every counter becomes c >> shift (shift >= 32: 0), as mee_admission_decay ages the sketch. */
int mee_hits_find(const mee_table* t, const int64_t* d_keys, size_t n, uint32_t* d_hits_out, void* stream);
int mee_hits_assign(mee_table* t, const int64_t* d_keys, size_t n, const uint32_t* d_hits, void* stream);
int mee_hits_decay(mee_table* t, uint32_t shift, void* stream);
/* Pooled lookup ("embedding bag"): bag b = d_keys[d_bag_offsets[b] .. d_bag_offsets[b+1]) (n_bags+1 uint64 offsets in DEVICE
 * memory); d_out[b,:] = the rows mee_find would return for the bag's positions, added in position order in fp32
 * (MEE_POOL_SUM) and divided by the bag length (MEE_POOL_MEAN); an empty bag gives zeros.  d_found (nullable) is per KEY,
 * indexed like d_keys; n = number of keys (a host value: it only picks the launch shape — a tile per bag, or a whole wave
 * per bag when the average bag is long).  The sum lives in registers: one output row per bag instead of one per key. */
enum { MEE_POOL_SUM = 0, MEE_POOL_MEAN = 1 };
int mee_find_pooled(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, float* d_out,
                    uint8_t* d_found, int mode, void* stream);
/* Weighted pooled lookup (torch.nn.EmbeddingBag with per_sample_weights; SUM only): d_weights = one fp32 weight per key position
 * (device, indexed like d_keys).  d_out[b,:] = the rows mee_find would return for the bag's positions, each multiplied by its weight
 * and added in position order in fp32: acc = w_first * row_first, then acc = acc + (w_i * row_i) — every product rounded, then every
 * sum (no fma).  With all weights 1.0f the result is bit-identical to mee_find_pooled(MEE_POOL_SUM).  An empty bag gives zeros; absent
 * and reserved keys contribute w_i * the default row.  d_found (nullable) as in mee_find_pooled.  d_located_out (nullable, int64[n])
 * receives each position's slot handle in the format of mee_find_located (-1 = absent): mee_apply_*_located and
 * mee_pooled_weighted_backward of the same step accept it.  Offsets past n are cut at n, a decreasing pair is an empty bag. */
int mee_find_pooled_weighted(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                             const float* d_weights, float* d_out, uint8_t* d_found, int64_t* d_located_out, void* stream);
/* Its backward, before the table step: d_grads_out[i,:] = d_weights[i] * d_bag_grads[bag(i),:] (one fp32 multiply per element;
 * d_bag_grads = [n_bags, dim]) and, when d_weight_grads_out (nullable, fp32[n]) is given, d_weight_grads_out[i] = sum_j
 * d_bag_grads[bag(i), j] * row_i[j], row_i = the row mee_find returns for key i at the time of the call (the default row when absent):
 * products and sum in fp64, rounded once to fp32 (the order of the sum is unspecified).  Without d_weight_grads_out no table row is
 * read.  d_located (nullable) = the handles mee_find_pooled_weighted of this step wrote: the rows are read through them instead of a
 * probe (a handle of another layout epoch is probed again).  Positions that no bag covers are not written (nor do they get a handle
 * from the forward), so the table step may only be given covered positions: the step is exactly mee_apply_*(d_keys, d_grads_out) —
 * or mee_apply_*_located with the same handles — when the bags partition [0, n) (d_bag_offsets[0] = 0, d_bag_offsets[n_bags] = n,
 * non-decreasing), as a batch of samples' bags does. */
int mee_pooled_weighted_backward(const mee_table* t, const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets,
                                 size_t n_bags, const float* d_weights, const float* d_bag_grads, float* d_grads_out, float* d_weight_grads_out,
                                 void* stream);
/* Max pooling (torch.nn.EmbeddingBag mode="max"; fp32-row tables).  Bags and their clamping are mee_find_pooled's; the row of a position is what
 * mee_find returns (the stored row, or the default row for an absent or reserved key — it takes part like any row).  For every element j the bag is
 * scanned in ascending position: the first position p0 gives m = row[p0][j], a = p0; each later position p replaces them iff row[p][j] > m (the IEEE
 * comparison).  So the first of equal values wins, +0.0 behind -0.0 does not replace it, a NaN at the first position stays and a NaN at a later one is
 * never taken.  d_out[b, j] = m, a copy of the bits (no arithmetic: nothing is rounded in fp32); with out_dtype = MEE_DTYPE_BF16 (8-byte aligned) m is
 * rounded once, the comparisons are still made in fp32.  d_argmax_out (nullable; [n_bags, dim] uint32, 16-byte aligned) receives a, the ABSOLUTE batch
 * position.  An empty bag gives +0.0 everywhere and argmax 0xFFFFFFFF.  d_found (nullable) is per key, as in mee_find.  Reads only: the table, its
 * status word, hit counters and sketch stay as they are.  One launch, no host synchronisation, no allocation.
 * MEE_ERR_UNSUPPORTED: a bf16-row or int8-row table.  MEE_ERR_INVALID_ARG, before anything is launched or written: a null pointer where rows are
 * due, an unknown out_dtype, a misaligned bf16 d_out or d_argmax_out, n >= 2^32 with d_argmax_out.  n_bags == 0 succeeds and writes nothing. */
int mee_find_pooled_max(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, void* d_out,
                        uint32_t out_dtype, uint8_t* d_found /* nullable */, uint32_t* d_argmax_out /* nullable */, void* stream);
/* Its backward, before the table step: for every position i that bag b covers, d_grads_out[i, j] = (d_argmax[b, j] == i) ? d_bag_grads[b, j] : +0.0
 * — a copy of the bits (a -0.0 gradient stays -0.0 at the winner).  d_argmax = what mee_find_pooled_max of this step wrote, d_bag_grads = [n_bags,
 * dim] fp32.  Positions that no bag covers are not written; no table row and no key is read.  The table step is then mee_apply_*(d_keys,
 * d_grads_out) when the bags partition [0, n): every key of a bag takes a step, with zeros where it did not win.  MEE_ERR_INVALID_ARG: a null
 * pointer where rows are due, a misaligned d_argmax, n >= 2^32 (always: positions are 32 bits). */
int mee_pooled_max_backward(const mee_table* t, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const uint32_t* d_argmax,
                            const float* d_bag_grads, float* d_grads_out, void* stream);
/* Pooled lookup over a hot/cold PAIR of tables (a key lives in exactly one of them; meepoembedding_amd/tiered.py): mee_find_pooled on the
 * union, bit for bit — the rows of a bag's positions added in position order in fp32 (the first copied, each later one added, no fma),
 * MEE_POOL_MEAN divides by (float)length, an empty bag gives zeros, offsets past n are cut at n, a decreasing pair is an empty bag.  The
 * row of a position is the hot table's if `hot` holds the key, else the cold table's if `cold` holds it, else a row of HOT's default_value
 * (reserved keys too); d_found[i] (nullable: not written) = 1 iff either table holds d_keys[i].  d_out = [n_bags, dim] fp32, or bf16
 * (out_dtype = MEE_DTYPE_BF16, 8-byte aligned: the finished bag row rounded once).  flags: MEE_TIER_COUNT_COLD adds 1 to the cold table's
 * hit counter for every position found there, MEE_TIER_COUNT_HOT the same for the hot table (meant for sampled calls); each needs its
 * table created with MEE_FLAG_TRACK_HITS.  ONE launch that probes both tables per position, no host synchronisation, capturable like
 * mee_find_pooled; `cold` may be a MEE_MEM_HOST_PINNED table (its rows are read over PCIe by the same launch).  MEE_ERR_INVALID_ARG: a
 * null table, hot == cold, different devices or dims, unknown flag bits, a count flag without the counters, an unknown out_dtype / mode,
 * a misaligned bf16 d_out.  n_bags == 0 writes nothing; bags over n == 0 keys are empty bags. */
enum { MEE_TIER_COUNT_COLD = 1, MEE_TIER_COUNT_HOT = 2 };
int mee_find_pooled_tiered(const mee_table* hot, const mee_table* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                           void* d_out, uint32_t out_dtype, uint8_t* d_found /* nullable: not written */, int mode, uint32_t flags, void* stream);
/* upsert; duplicate keys: last occurrence wins. */
int mee_insert(mee_table* t, const int64_t* d_keys, const float* d_values, size_t n, void* stream);
/* overwrite only if present; d_found nullable; duplicates: last occurrence wins. */
int mee_assign(mee_table* t, const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found, void* stream);
/* the same two verbs on one plane of the table: 0 = values, 1 = acc | m, 2 = v (state planes read 0 for absent keys).
 * They let a caller move a key together with its optimizer state between tables (hot/cold tiers, re-sharding). */
int mee_find_plane(const mee_table* t, uint32_t plane, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found,
                   void* stream);
int mee_assign_plane(mee_table* t, uint32_t plane, const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found,
                     void* stream);
/* delete present keys (their slots become RECLAIMED and are reused by later inserts); d_found nullable. */
int mee_remove(mee_table* t, const int64_t* d_keys, size_t n, uint8_t* d_found, void* stream);
/* find, inserting absent keys with their initial row first; d_found (nullable) = present before the call. */
int mee_find_or_insert(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream);
/* mee_find_or_insert that also reports where every key lives now: d_slots_out[i] = the slot of keys[i] after the call (-1 only for
 * reserved keys and for keys that could not be created: table full) — the handles mee_apply_*_located of the same training step
 * takes instead of probing again.  Same validity as mee_find_located's handles: until the table's layout changes. */
int mee_find_or_insert_located(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, int64_t* d_slots_out, void* stream);
/* Admission policy: mee_find_or_insert that creates an absent key only once it has been asked for often enough.  Every absent
 * position adds 1 to its key's sketch counters; a key whose estimate — after ALL additions of this batch — is >= min_count is
 * created (initial row, initial optimizer state) and all its occurrences return that row; other absent keys return the default
 * row and stay absent.  d_found (nullable) = present before the call.  Deterministic per batch (SPEC.md §3); a count-min sketch
 * only over-estimates, so a key is never admitted later than after min_count requests.  mee_admission_decay: every counter >>= shift
 * (shift >= 32: zero) — a new observation window. */
int mee_find_or_insert_admit(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, uint32_t min_count, void* stream);
int mee_admission_decay(mee_table* t, uint32_t shift, void* stream);
/* Tiered pairs (a key lives in exactly one of two tables): the same two mutators restricted to the positions whose
 * d_found byte is 0, i.e. keys that an earlier pass found in NEITHER table.  d_found is only read. */
int mee_insert_missing(mee_table* t, const int64_t* d_keys, const float* d_values, size_t n, const uint8_t* d_found, void* stream);
int mee_find_or_insert_missing(mee_table* t, const int64_t* d_keys, size_t n, float* d_out, const uint8_t* d_found, void* stream);
/* Admission into a tiered pair (SPEC.md §3 "Tiering": the pair's sketch is its HOT table's): the admitting sibling of mee_find_or_insert_missing, on
 * buffers a find over both tiers already filled.  Every position with d_found[i] == 0 and a non-reserved key adds 1 to its key's counters in
 * `counts`'s sketch (the pair's hot table); a key whose estimate — after ALL additions of this batch — is >= min_count is created in `t` (the tier
 * the pair picked: `counts` itself, or the cold table) exactly as mee_find_or_insert_missing creates it, and all its occurrences receive its initial
 * row in d_out; every other position of d_out is left untouched, and d_found is only read.  RECLAIMED among the missing positions sets
 * MEE_STATUS_RESERVED_KEY on t, TABLE_FULL lands on t, as there.  counts == t is legal.  fp32 rows, one dim and one device for both tables,
 * n <= t's max_batch (MEE_ERR_BATCH_TOO_LARGE); MEE_ERR_UNSUPPORTED when `counts` was created without MEE_FLAG_ADMISSION (t needs no sketch) or
 * either table stores narrow rows.  Three launches (count, decide, create) on t's scratch; no host synchronisation, no allocation, capturable. */
int mee_find_or_insert_admit_missing(mee_table* t, mee_table* counts, const int64_t* d_keys, size_t n, float* d_out, const uint8_t* d_found,
                                     uint32_t min_count, void* stream);
/* [syncs] all stored pairs, unspecified order; d_state1/d_state2 (nullable) receive acc|m and v rows in the
 * same order.  At most `cap` pairs are written; *n_out = number stored in the table. */
int mee_export(const mee_table* t, int64_t* d_keys_out, float* d_values_out, float* d_state1_out,
               float* d_state2_out, size_t cap, size_t* n_out, void* stream);
/* [syncs] the same over the slot range [slot_begin, min(slot_end, capacity)): checkpointing / rehashing a table that
 * fills most of HBM walks it in ranges with bounded scratch (a range of S slots holds at most S pairs); the union over a
 * partition of [0, capacity) is mee_export's set.  *n_out = pairs stored in the range. */
int mee_export_range(const mee_table* t, uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out,
                     float* d_state1_out, float* d_state2_out, size_t cap, size_t* n_out, void* stream);
/* [syncs] rehash in place to at least new_capacity slots (rounded up like mee_table_create; growing or shrinking): every
 * stored pair, its optimizer planes and hit counter move device-to-device into new planes, then the old ones are freed —
 * old and new planes must fit in memory together.  No observable of SPEC.md §3 changes; capacity below the number of
 * stored keys is MEE_ERR_INVALID_ARG; on any error the table is untouched.  Not concurrent with other calls on `t`. */
int mee_reserve(mee_table* t, uint64_t new_capacity, void* stream);
int mee_size(const mee_table* t, size_t* n_out, void* stream);        /* [syncs] */
int mee_status(const mee_table* t, uint32_t* bits_out, void* stream); /* [syncs] */
int mee_clear_status(mee_table* t, void* stream);
/* probe only: d_slots_out[i] = the slot handle of d_keys[i] (-1 = absent / reserved), d_found nullable.  No row is touched. */
int mee_locate(const mee_table* t, const int64_t* d_keys, size_t n, int64_t* d_slots_out, uint8_t* d_found, void* stream);
/* Base address of one plane (0 = values, 1 = acc | m, 2 = v): row of slot s at ptr + s * row_stride_bytes.  A device pointer for
 * MEE_MEM_HBM tables; for MEE_MEM_HOST_PINNED tables the address is valid on the HOST as well (pinned, device-mapped) — this is what
 * a staged transfer (host-side gather + hipMemcpyAsync on a side stream) of a cold tier reads.  Invalidated by mee_reserve / destroy;
 * the caller orders its accesses against the table's operators. */
int mee_table_plane(const mee_table* t, uint32_t plane, void** ptr_out, uint64_t* row_stride_bytes, uint32_t* value_memory);
/* [syncs] measurement aid (SURVEY.md §8d "mean probe length"): the number of buckets a find visits for d_keys, summed over
 * the batch (reserved keys visit none); divide by n for the mean.  Changes nothing. */
int mee_probe_length(const mee_table* t, const int64_t* d_keys, size_t n, uint64_t* buckets_visited_out, void* stream);
/* [syncs] the same as a histogram (SURVEY.md §5 "metrics"): hist_out[0 .. 3] = how many of the batch's lookups visit 1 / 2 / 3 / 4 or more buckets
 * (reserved keys visit none and are not counted). */
int mee_probe_histogram(const mee_table* t, const int64_t* d_keys, size_t n, uint64_t* hist_out /* [4] */, void* stream);

/* ---- table groups: one launch for the lookups of many tables (a model's embedding collection) ----------------
 * All tables of a group live on one device and have the same dim.  The key batches of the tables are concatenated
 * ("jagged" layout): segment j = d_keys[d_offsets[j] .. d_offsets[j+1]), d_offsets = n_tables+1 non-decreasing uint64 in
 * DEVICE memory, n = total positions (host value; positions outside [d_offsets[0], d_offsets[n_tables]) are left
 * untouched).  Results are identical to mee_find on each table with its segment; the launch latency floor is paid once
 * instead of n_tables times.  Asynchronous on `stream`; after mee_reserve on a member the next call re-reads that
 * table's planes (one stream synchronisation).  The group does not own the tables: destroy it before them.  Calls on one
 * group that use its scratch (mee_group_find_or_insert / _admit without d_found, mee_group_apply_*) must be ordered by the caller;
 * mee_find_grouped / mee_group_find_pooled calls may run concurrently on several streams.
 *
 * Row storage: a group holds fp32-row tables, or ONLY tables created with MEE_FLAG_BF16_ROWS — a bf16-row group, the serving form of a collection.  A
 * mix of the two is MEE_ERR_UNSUPPORTED (one storage type per group: the row type is a compile-time property of every launch, not a per-member branch
 * in the row fetch), and a bf16-row group needs max_apply_batch = 0 (MEE_ERR_INVALID_ARG otherwise: it has no step and no scratch table).  Each lookup
 * of a bf16-row group is, bit for bit, that lookup on each bf16-row member — hence the fp32 group over fp32 tables that were handed the rounded rows
 * and created with the rounded default_value; found masks, reserved keys, positions outside the segments, empty bags, the clamping of the offsets and
 * each member's own default row included.  The operators it has: mee_find_grouped / _as (fp32 out widens exactly, bf16 out returns the stored bits),
 * mee_group_find_pooled / _as without weights (SUM | MEAN; rows widened and added in fp32 in position order, the finished bag row rounded once for bf16
 * out), mee_group_find_pooled_jagged, mee_group_value_dtype, mee_group_destroy; mee_reserve on a member between lookups keeps working.  Everything else
 * — mee_group_find_or_insert / _as / _admit, mee_group_admission_decay, every mee_group_apply_*, mee_group_find_pooled_weighted and a non-null d_weights of mee_group_find_pooled_as,
 * mee_group_pooled_weighted_backward, and a non-null d_located_out of any pooled form (located rows exist for the backward, which this group does not
 * have) — returns MEE_ERR_UNSUPPORTED before anything is launched or written; mee_group_set_tuning answers as for any group without an apply. */
typedef struct mee_group mee_group;
int mee_group_create(mee_table* const* tables, uint32_t n_tables, uint64_t max_apply_batch, mee_group** out);
int mee_group_destroy(mee_group* g);
/* mee_set_tuning for the group's own apply ("apply_bucket_max", "apply_kernel", …: as for a table; groups created with
 * max_apply_batch = 0 have nothing to tune: MEE_ERR_UNSUPPORTED). */
int mee_group_set_tuning(mee_group* g, const char* name, int value);
/* the members' row storage type: MEE_DTYPE_F32, or MEE_DTYPE_BF16 for a bf16-row group */
int mee_group_value_dtype(const mee_group* g, uint32_t* out);
int mee_find_grouped(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, float* d_out, uint8_t* d_found,
                     void* stream);
/* mee_find_or_insert over the jagged layout (three launches): absent keys are created in their member table with that
 * table's initial row / optimizer state first; d_found (nullable when n <= max_apply_batch) = present before the call. */
int mee_group_find_or_insert(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, float* d_out, uint8_t* d_found,
                             void* stream);
/* Admission over the jagged layout: mee_find_or_insert_admit of every member on its segment, each member counting in ITS OWN sketch (the group
 * keeps none), in three launches whatever the number of tables — the grouped find, one counting launch, one creation launch that reads the
 * final counters itself.  A position inside [d_offsets[0], d_offsets[n_tables]) and below n whose key is absent and not reserved adds 1 to its
 * member's three counters (a key that occurs c times adds c); then the key is created — initial row, initial optimizer state, all its
 * occurrences return that row — when the minimum of the three is >= the member's threshold, and returns the default row and stays absent
 * otherwise.  Positions outside the segments are neither written, counted nor created.  The threshold is min_count, or d_min_counts[member]
 * when d_min_counts (DEVICE memory, n_tables entries, nullable) is given; 0 or 1 admits at first sight: that segment gets
 * mee_group_find_or_insert's result and its sketch still counts.  out_dtype: MEE_DTYPE_F32 or MEE_DTYPE_BF16 (the fp32 result rounded once;
 * the tables stay fp32).  d_found (nullable when n <= max_apply_batch, else MEE_ERR_BATCH_TOO_LARGE) = present before the call.  A tombstone
 * value in a segment sets MEE_STATUS_RESERVED_KEY on that member, MEE_STATUS_TABLE_FULL lands on the member that had no room.  No host
 * synchronisation, no allocation, capturable; no limit on n beyond mee_group_find_or_insert's.  Refused before anything is launched or written:
 * a bf16-row group and a member created without MEE_FLAG_ADMISSION (MEE_ERR_UNSUPPORTED, the message names the member), null arguments
 * (MEE_ERR_INVALID_ARG).  mee_group_admission_decay: mee_admission_decay of every member, one launch. */
int mee_group_find_or_insert_admit(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                   uint8_t* d_found, uint32_t min_count, const uint32_t* d_min_counts, void* stream);
int mee_group_admission_decay(mee_group* g, uint32_t shift, void* stream);
/* One sparse-optimizer step over the same jagged layout (groups created with max_apply_batch >= n; all members have the
 * same optimizer): identical to mee_apply_* on each table with its segment of keys and grads (absent keys ignored,
 * duplicates of a key inside its segment summed in fp64 and applied once), in a fixed number of launches whatever the
 * number of tables.  Status bits (RESERVED_KEY for a tombstone value in a segment) land on the member of that segment. */
int mee_group_apply_adagrad(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr,
                            float eps, void* stream);
int mee_group_apply_adam(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr,
                         float beta1, float beta2, float eps, uint64_t step, void* stream);

/* The embedding-bag collection: every member table serves `bags_per_table` bags (one per sample of the batch), bag b belongs
 * to member b / bags_per_table, d_bag_offsets holds n_tables x bags_per_table + 1 key offsets (device) and d_out one pooled row
 * per bag — mee_find_pooled on every member, in one launch.  Backward: mee_apply_*_indexed on every member in the usual 7
 * launches; d_grad_index[i] = the bag of key position i, d_bag_grads = [n_bags, dim] (pre-scaled by 1/length for MEAN).
 * d_located_out / d_located (nullable, int64[n]): the forward can hand the rows it located (opaque per-position handles) to
 * the backward of the SAME step, which then skips its own probe pass (6 launches).  The handles are only valid while no
 * key of the batch is removed, no member is rehashed and no slot they name is reused: i.e. forward -> backward. */
int mee_group_find_pooled(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                          float* d_out, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream);
int mee_group_apply_adagrad_pooled(mee_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                   const float* d_bag_grads, const uint32_t* d_grad_index, const int64_t* d_located, size_t n, float lr,
                                   float eps, void* stream);
int mee_group_apply_adam_pooled(mee_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                const float* d_bag_grads, const uint32_t* d_grad_index, const int64_t* d_located, size_t n, float lr,
                                float beta1, float beta2, float eps, uint64_t step, void* stream);
/* The same collection where the members' bag counts DIFFER (the owner's side of a sharded group's bags: the runs that arrive per member
 * change from member to member and from step to step).  mee_group_find_pooled_jagged is mee_group_find_pooled except for the bag -> member
 * map: bag b belongs to the member j with d_member_bags[j] <= b < d_member_bags[j + 1] (n_tables + 1 non-decreasing uint64 in DEVICE
 * memory; a member may have no bags; [0, B, 2B, …] gives mee_group_find_pooled(bags_per_table = B) bit for bit, handles included).  A bag
 * below d_member_bags[0] or at or beyond d_member_bags[n_tables] is an empty bag: a row of zeros, nothing probed.  The map is caller data
 * and is never trusted: whatever it holds, the member used stays inside the group.  d_out [n_bags, dim] fp32 (no typed and no weighted
 * form: the partial rows of a sharded bag travel as fp32).  Never synchronises, capturable, safe on several streams at once. */
int mee_group_find_pooled_jagged(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                                 const uint64_t* d_member_bags /* [n_tables + 1], device */, float* d_out, uint8_t* d_found,
                                 int64_t* d_located_out, int mode, void* stream);
/* mee_apply_*_indexed on every member with its segment of the jagged batch (d_offsets = n_tables + 1 member offsets, as mee_group_apply_*),
 * in the grouped apply's fixed number of launches: position i takes row d_grad_index[i] of d_grads [n_grad_rows, dim]; indices >=
 * n_grad_rows are clamped.  Refusals as mee_group_apply_* and mee_apply_*_indexed. */
int mee_group_apply_adagrad_indexed(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows,
                                    const uint32_t* d_grad_index, size_t n, float lr, float eps, void* stream);
int mee_group_apply_adam_indexed(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows,
                                 const uint32_t* d_grad_index, size_t n, float lr, float beta1, float beta2, float eps, uint64_t step, void* stream);
/* The FTRL-Proximal step (mee_apply_ftrl, below) over a group whose members were created with MEE_OPT_FTRL: mee_group_apply_adagrad,
 * mee_group_apply_adagrad_pooled and mee_group_apply_adagrad_indexed with (beta, l1, l2) after lr; the same launches, refusals and argument checks. */
int mee_group_apply_ftrl(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n, float lr, float beta,
                         float l1, float l2, void* stream);
int mee_group_apply_ftrl_pooled(mee_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table, const float* d_bag_grads,
                                const uint32_t* d_grad_index, const int64_t* d_located, size_t n, float lr, float beta, float l1, float l2,
                                void* stream);
int mee_group_apply_ftrl_indexed(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, const float* d_grads, size_t n_grad_rows,
                                 const uint32_t* d_grad_index, size_t n, float lr, float beta, float l1, float l2, void* stream);
/* The weighted forms over the collection: mee_find_pooled_weighted / mee_pooled_weighted_backward on every member, bag b belonging to
 * member b / bags_per_table, in one launch each.  d_located_out / d_located are in the group's format (as mee_group_find_pooled's); the
 * step after the backward is mee_group_apply_*(d_keys, member offsets, d_grads_out) — the grads are per position, not per bag. */
int mee_group_find_pooled_weighted(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                   const float* d_weights, float* d_out, uint8_t* d_found, int64_t* d_located_out, void* stream);
int mee_group_pooled_weighted_backward(mee_group* g, const int64_t* d_keys, const int64_t* d_located, size_t n, const uint64_t* d_bag_offsets,
                                       size_t bags_per_table, const float* d_weights, const float* d_bag_grads, float* d_grads_out,
                                       float* d_weight_grads_out, void* stream);
/* Max pooling over the collection (fp32-row groups): mee_find_pooled_max / mee_pooled_max_backward of member b / bags_per_table on its bags, in one
 * launch each; every member uses its own default row, and the argmax positions are absolute in the whole batch.  The step after the backward is
 * mee_group_apply_*(d_keys, member offsets, d_grads_out).  Refusals as the table forms'; MEE_ERR_UNSUPPORTED for a bf16-row group.  The lookup
 * re-reads a member's planes in its first call after mee_reserve on that member, as every group lookup does; the backward reads no table. */
int mee_group_find_pooled_max(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out,
                              uint32_t out_dtype, uint8_t* d_found /* nullable */, uint32_t* d_argmax_out /* nullable */, void* stream);
int mee_group_pooled_max_backward(mee_group* g, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, const uint32_t* d_argmax,
                                  const float* d_bag_grads, float* d_grads_out, void* stream);
/* The embedding-bag collection over hot/cold PAIRS: member j of hot_group and member j of cold_group are the two tiers of pair j (a key lives in
 * exactly one of them; meepoembedding_amd/tiered.py, TieredTableGroup).  mee_group_find_pooled_tiered is, by definition, mee_find_pooled_tiered(hot
 * member b / bags_per_table, cold member b / bags_per_table) on every bag b, bit for bit, in ONE launch for all n_tables x bags_per_table bags: a
 * position is probed in its member's hot index, in the cold one only where a wave missed, the row comes from the plane that holds it, an absent or
 * reserved key reads that member's HOT table's default row, d_found[i] (nullable: not written) = 1 iff either tier holds the key; SUM | MEAN, offsets
 * past n cut at n, a decreasing pair an empty bag; d_out = [n_tables x bags_per_table, dim] fp32 or bf16 (the finished bag row rounded once).  No
 * weights, no jagged map, no located rows.  flags = MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT: every position found in that tier adds 1 to its slot's
 * hit counter in that member's table; EVERY member of the tier must have been created with MEE_FLAG_TRACK_HITS.
 * mee_group_ensure_tiered creates, for every position with d_found[i] == 0 (a mask an earlier lookup wrote: "in neither tier"), the key in ONE tier of
 * its member — the cold table where d_to_cold[member] != 0 (n_tables bytes in DEVICE memory; null: every member creates hot) — exactly as
 * mee_find_or_insert_missing on that table does: initial row from that table's initializer, initial optimizer state, a zero hit counter, TABLE_FULL /
 * RESERVED_KEY (a tombstone value in the batch) on that table's status word, one creation per distinct key.  Member segments are every
 * bags_per_table-th bag offset, cut at n.  No row is returned: there is no [n, dim] buffer.  d_found is only read.
 * Both: no host synchronisation and no allocation, capturable like mee_find_pooled_tiered; after mee_reserve on a member of either group the next call
 * re-reads that table's planes (one stream synchronisation).  bags_per_table == 0 succeeds and writes nothing.  MEE_ERR_INVALID_ARG before anything
 * is launched or written: a null group, hot_group == cold_group, groups that differ in device, dim or number of tables, a member that is the same
 * table in both, an unknown mode / out_dtype / flag bit, a misaligned bf16 d_out, a count flag when a member of that tier has no counters;
 * MEE_ERR_UNSUPPORTED: a bf16-row group. */
int mee_group_find_pooled_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                                 size_t bags_per_table, void* d_out, uint32_t out_dtype, uint8_t* d_found /* nullable: not written */, int mode,
                                 uint32_t flags, void* stream);
int mee_group_ensure_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                            size_t bags_per_table, const uint8_t* d_found, const uint8_t* d_to_cold /* [n_tables], device; nullable: all hot */,
                            void* stream);
/* mee_group_find_pooled_tiered where the members' bag counts DIFFER (the owner's side of a sharded group of pairs: the runs that arrive per member
 * change from member to member and from step to step).  mee_group_find_pooled_tiered_jagged is mee_group_find_pooled_tiered except for the bag ->
 * member map, which is mee_group_find_pooled_jagged's: bag b belongs to the member j with d_member_bags[j] <= b < d_member_bags[j + 1] (n_tables + 1
 * non-decreasing uint64 in DEVICE memory; a member may have no bags; [0, B, 2B, …] gives mee_group_find_pooled_tiered(bags_per_table = B,
 * MEE_DTYPE_F32) bit for bit).  A bag below d_member_bags[0] or at or beyond d_member_bags[n_tables] is an empty bag: a row of zeros, nothing probed,
 * the d_found bytes of its positions not written.  On every other bag the result is, bit for bit, mee_find_pooled_tiered(hot member j, cold member
 * j) on that bag: the hot index first, the cold one only where a wave missed, the row from the plane that holds it, fp32 sums in position order
 * without fma, MEAN's division by (float)length, that member's HOT default row for an absent or reserved key, offsets past n cut at n, a decreasing
 * pair an empty bag.  The map is caller data and is never trusted: whatever it holds, the member used stays inside the group.  d_out [n_bags, dim]
 * fp32 only (the partial rows of a sharded bag travel as fp32); d_found nullable: not written.  flags = MEE_TIER_COUNT_*, as above.  One launch,
 * no host synchronisation, no allocation, capturable.  n_bags == 0 succeeds and writes nothing.  MEE_ERR_INVALID_ARG before anything is launched: a
 * null pointer, an unknown mode, and what mee_group_find_pooled_tiered refuses about its two groups and its flags; MEE_ERR_UNSUPPORTED: a bf16-row
 * group. */
int mee_group_find_pooled_tiered_jagged(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                                        size_t n_bags, const uint64_t* d_member_bags /* [n_tables + 1], device */, float* d_out,
                                        uint8_t* d_found /* nullable: not written */, int mode, uint32_t flags, void* stream);
/* The UNPOOLED lookups over the same two groups — a row per position of the jagged batch (d_offsets = n_tables + 1 member offsets in DEVICE memory,
 * as mee_find_grouped; sequence features, whose model wants every id's row).  mee_group_find_tiered is, by definition and bit for bit, on every
 * member's segment: mee_find on hot member j, then mee_find_missing on cold member j over the same buffers (with count flags the mee_find_counted
 * forms) — TieredLookupTable.find — in ONE launch for the whole collection: a position is probed in its member's hot index, in the cold one only
 * where a wave missed, the row comes from the plane that holds it, an absent or reserved key reads that member's HOT table's default row,
 * d_found[i] (nullable: not written) = 1 iff either tier holds the key; positions outside [d_offsets[0], d_offsets[n_tables]) or at or past n are
 * left alone, as mee_find_grouped leaves them.  d_out = [n, dim] fp32 or bf16 (every element rounded once).  flags = MEE_TIER_COUNT_COLD |
 * MEE_TIER_COUNT_HOT as above.
 * mee_group_find_or_insert_tiered is that lookup, flags included, followed by mee_find_or_insert_missing on the tier d_to_cold selects for the
 * member (null: every member creates hot), in ONE more launch: two launches whatever the number of tables.  d_found (required) = present before the
 * call; every position it leaves missing receives its key's initial row — the same row at every occurrence of a repeated new key, rounded for a
 * bf16 d_out while the stored row is not — and TABLE_FULL / RESERVED_KEY go to the status word of the table that was asked to create.
 * Both: no host synchronisation and no allocation, capturable; after mee_reserve on a member of either group the next call re-reads that table's
 * planes (one stream synchronisation).  n == 0 succeeds and writes nothing.  MEE_ERR_INVALID_ARG before anything is launched or written: a null
 * pointer, hot_group == cold_group, groups that differ in device, dim or number of tables, a member that is the same table in both, an unknown
 * out_dtype / flag bit, a misaligned bf16 d_out, a count flag when a member of that tier has no counters; MEE_ERR_UNSUPPORTED: a bf16-row group. */
int mee_group_find_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, const uint64_t* d_offsets, size_t n,
                          void* d_out, uint32_t out_dtype, uint8_t* d_found /* nullable: not written */, uint32_t flags, void* stream);
int mee_group_find_or_insert_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, const uint64_t* d_offsets, size_t n,
                                    void* d_out, uint32_t out_dtype, uint8_t* d_found /* required: present before the call */,
                                    const uint8_t* d_to_cold /* [n_tables], device; nullable: all hot */, uint32_t flags, void* stream);
/* Admission over a group of pairs (SPEC.md §3 "Tiering"): a pair's sketch is its HOT table's, so every member of hot_group must have been created with
 * MEE_FLAG_ADMISSION (MEE_ERR_UNSUPPORTED naming the first that was not); the cold members need no sketch, and one they have is never touched.
 * mee_group_find_or_insert_admit_tiered is mee_group_find_or_insert_tiered with the creation behind the sketches, THREE launches whatever the number of
 * pairs: (1) that lookup, flags included; (2) every position inside the segments whose d_found byte is 0 and whose key is not reserved adds 1 to its
 * key's three counters in its member's hot sketch (a key that occurs c times adds c); (3) one creation launch in which a missing key goes on only when
 * the minimum of its counters — after ALL additions of the batch — reached the member's threshold: min_count, or d_min_counts[member] when
 * d_min_counts (DEVICE memory, n_tables entries, nullable) is given.  An admitted key is created once, in the tier d_to_cold selects for its member, as
 * mee_find_or_insert_missing on that table creates it, and all its occurrences return that initial row; every other absent key keeps the hot default
 * row and stays absent.  0 and 1 admit at first sight: the result, the tables and the status words are mee_group_find_or_insert_tiered's, and the
 * sketch still counts.  TABLE_FULL / RESERVED_KEY go to the status word of the table that was asked to create.  Positions outside
 * [d_offsets[0], d_offsets[n_tables]) or at or past n are not written, not counted and create nothing.  out_dtype = MEE_DTYPE_BF16 rounds the returned
 * copy once.  The groups keep no counters: these calls and mee_find_or_insert_admit / mee_find_or_insert_admit_missing / mee_admission_decay on the
 * tables interleave freely.
 * mee_group_ensure_admit_tiered is mee_group_ensure_tiered behind the same gate, TWO launches (count, then the gated creation with no rows out): member
 * segments are every bags_per_table-th bag offset, cut at n.
 * Both: no host synchronisation, no allocation, capturable; the argument checks are those of the non-admitting forms. */
int mee_group_find_or_insert_admit_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, const uint64_t* d_offsets, size_t n,
                                          void* d_out, uint32_t out_dtype, uint8_t* d_found /* required: present before the call */,
                                          const uint8_t* d_to_cold /* [n_tables], device; nullable: all hot */, uint32_t min_count,
                                          const uint32_t* d_min_counts /* [n_tables], device; nullable */, uint32_t flags, void* stream);
int mee_group_ensure_admit_tiered(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                                  size_t bags_per_table, const uint8_t* d_found, const uint8_t* d_to_cold /* [n_tables], device; nullable: all hot */,
                                  uint32_t min_count, const uint32_t* d_min_counts /* [n_tables], device; nullable */, void* stream);

/* ---- tier migration (SPEC.md §3 move): "this key, with everything it owns, now lives in that table" --------------------------------------
 * Let P be the batch positions whose key is not reserved and is stored in `src` when the call starts, in ascending order; the first max_moves of them
 * are SERVED (UINT64_MAX: all).  Every key at a served position ends the call stored in `dst` and absent from `src`: its values row and every
 * optimizer plane (acc | m, v) copied bit for bit; a key `dst` already held has its row and state overwritten there (an upsert) and keeps its hit
 * counter, a slot created in `dst` starts with hit counter 0; the `src` slot becomes RECLAIMED.  Duplicates are legal: every occurrence counts
 * against max_moves, the key moves once.  d_moved[i] (nullable: not written) = 1 for served positions whose key got a slot in `dst`, 0 for every
 * other i < n; *d_n_moved (DEVICE memory, nullable) = the number of DISTINCT keys moved.  A key for which `dst` has no room STAYS IN `src`,
 * untouched, and MEE_STATUS_TABLE_FULL goes to dst's status word (which of several such keys find room is decided by the race of the claims, as
 * for mee_insert).  RECLAIMED in the batch sets MEE_STATUS_RESERVED_KEY on `src`, as mee_remove does; EMPTY is padding.  In everything else both
 * tables are left as the sequence  mee_insert(dst, k, mee_find(src, k)); mee_assign_plane(dst, p, k, mee_find_plane(src, p, k)) per state plane;
 * mee_remove(src, k)  over the moved keys leaves them: size, probe rule, tombstone reuse, key-sorted export.
 * Either table may be MEE_MEM_HBM or MEE_MEM_HOST_PINNED, with or without MEE_FLAG_TRACK_HITS.  Two launches (four when max_moves < n), no
 * [n, dim] buffer, no allocation, no host synchronisation and nothing read back: capturable.  Host side as mee_remove on `src` and mee_insert on
 * `dst`: a partition a training forward left pending on either is dropped, slot handles taken from `src` before the call are stale.
 * Refused before anything is launched or written — MEE_ERR_INVALID_ARG: a null table (or null d_keys with n > 0), src == dst, different device,
 * dim or optimizer, a partition of mee_apply_prepare pending on either; MEE_ERR_UNSUPPORTED: a bf16-row or int8-row table on either side;
 * MEE_ERR_BATCH_TOO_LARGE: n above either table's max_batch.  n == 0 writes 0 to *d_n_moved.
 * mee_group_move is, by definition, mee_move(src_group member j, dst_group member j, segment j, d_max_moves[j]) for every member, segment j =
 * positions d_offsets[j] .. d_offsets[j + 1] - 1 (n_tables + 1 offsets in DEVICE memory, cut at n), in ONE launch sequence whatever the number of
 * members.  d_max_moves: n_tables limits in DEVICE memory (null: no limit); d_n_moved: n_tables counts in DEVICE memory (nullable).  Positions
 * outside [d_offsets[0], d_offsets[n_tables]) or at or past n are not looked at and their d_moved bytes are not written.  Refused like the other
 * operators over two groups (null, the same group twice, groups that differ in device, dim or number of tables, a member that is the same table in
 * both, a bf16-row group), plus per member what mee_move refuses (messages name the member), plus a table that is a member more than once across
 * the two groups.  The offsets are never read by the host, so the batch bound is on n: n above the max_batch of any member of either group is
 * MEE_ERR_BATCH_TOO_LARGE.  After mee_reserve on a member the next call re-reads that table's planes (one stream synchronisation). */
int mee_move(mee_table* src, mee_table* dst, const int64_t* d_keys, size_t n, uint64_t max_moves, uint8_t* d_moved /* [n], nullable */,
             uint64_t* d_n_moved /* device, one word, nullable */, void* stream);
int mee_group_move(mee_group* src_group, mee_group* dst_group, const int64_t* d_keys, const uint64_t* d_offsets, size_t n,
                   const uint64_t* d_max_moves /* device [n_tables], nullable = no limit */, uint8_t* d_moved /* [n], nullable */,
                   uint64_t* d_n_moved /* device [n_tables], nullable */, void* stream);

/* ---- typed output: the lookups above with fp32 OR bf16 result rows (SPEC.md §3 "Output type") --------------------------------
 * The models these tables feed run in bf16; a lookup that writes bf16 itself saves the cast in front of the first dense layer and half
 * of its own store traffic.  Tables, optimizer state and every accumulation stay fp32: with out_dtype = MEE_DTYPE_BF16 the result is, by
 * definition, the fp32 result of the same operator with every element rounded ONCE to bfloat16, round to nearest even
 *     u = bits(x);  bf16_bits(x) = (u + 0x7FFF + ((u >> 16) & 1)) >> 16      (x not a NaN; a NaN gives a NaN)
 * — ±0, ±inf and denormals follow from the formula (denormals are not flushed, a finite value beyond the largest bf16 becomes inf);
 * for a pooled lookup it is the FINISHED bag row that is rounded, no intermediate.  d_found, slot handles, status bits, the partition a
 * *_prepare form leaves behind and (find_or_insert) the table afterwards are those of the fp32 call.  With MEE_DTYPE_F32 every form below
 * IS the operator it is named after, bit for bit.  d_out: [rows, dim] of the chosen type; a bf16 buffer must be 8-byte aligned, anything
 * else — like an unknown out_dtype — is MEE_ERR_INVALID_ARG.  The "find_rounds" knob does not apply to bf16 lookups.
 *   mee_find_as                              flags as mee_find_ex (MEE_FIND_DEFAULT: the library's own choice, as mee_find)
 *   mee_find_pooled_as                       d_weights nullable (non-null: mee_find_pooled_weighted, MEE_POOL_SUM only); d_located_out
 *                                            (nullable) is the weighted form's output
 *   mee_group_find_pooled_as                 d_weights nullable (non-null: mee_group_find_pooled_weighted)
 * No typed form exists for find_missing / find_counted / find_plane / find_many / find_unordered / find_or_insert_admit /
 * find_or_insert_missing, the mee_p2p_* lookups and mee_export: they return fp32.  Gradients handed to mee_apply_* are fp32.
 * The sharded lookups have typed forms of their own, mee_sharded_find_as / mee_sharded_find_or_insert_as (declared with the other mee_sharded_*
 * operators): there the OWNER of a key rounds its row, before the rows travel — a lookup then puts 8 + 2·dim + 1 bytes on the wire (key out, bf16
 * row and found byte back) instead of 8 + 4·dim + 1: 137 instead of 265 B at dim 64. */
/* MEE_DTYPE_INT8 names a ROW STORAGE type only (mee_table_value_dtype of a table created with MEE_FLAG_INT8_ROWS): as an out_dtype or an in_dtype it is
 * MEE_ERR_INVALID_ARG. */
enum { MEE_DTYPE_F32 = 0, MEE_DTYPE_BF16 = 1, MEE_DTYPE_INT8 = 2 };
int mee_find_as(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, uint32_t flags, void* stream);
/* Typed INPUT: mee_insert / mee_assign whose d_values holds rows of in_dtype.  MEE_DTYPE_F32: they ARE mee_insert / mee_assign.  MEE_DTYPE_BF16 on a
 * table created with MEE_FLAG_BF16_ROWS: d_values is [n, dim] bf16, 16-byte aligned, and the rows are stored VERBATIM (no rounding, NaN payloads
 * included); on an fp32 table it is MEE_ERR_UNSUPPORTED.  An unknown in_dtype or a misaligned bf16 buffer is MEE_ERR_INVALID_ARG. */
int mee_insert_as(mee_table* t, const int64_t* d_keys, const void* d_values, uint32_t in_dtype, size_t n, void* stream);
int mee_assign_as(mee_table* t, const int64_t* d_keys, const void* d_values, uint32_t in_dtype, size_t n, uint8_t* d_found, void* stream);
/* MEE_DTYPE_F32, MEE_DTYPE_BF16 for a table created with MEE_FLAG_BF16_ROWS, or MEE_DTYPE_INT8 for one created with MEE_FLAG_INT8_ROWS (mee_table_info is a fixed 48 bytes: the row type has its own call) */
int mee_table_value_dtype(const mee_table* t, uint32_t* out);
int mee_find_located_as(const mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out,
                        void* stream);
int mee_find_located_prepare_as(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_slots_out,
                                void* stream);
int mee_find_or_insert_as(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, void* stream);
int mee_find_or_insert_located_as(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                  int64_t* d_slots_out, void* stream);
int mee_find_or_insert_located_prepare_as(mee_table* t, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                                          int64_t* d_slots_out, void* stream);
int mee_find_pooled_as(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, const float* d_weights,
                       void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream);
int mee_find_grouped_as(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                        void* stream);
int mee_group_find_or_insert_as(mee_group* g, const int64_t* d_keys, const uint64_t* d_offsets, size_t n, void* d_out, uint32_t out_dtype,
                                uint8_t* d_found, void* stream);
int mee_group_find_pooled_as(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                             const float* d_weights, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located_out, int mode, void* stream);

/* ---- padded sequence lookup (SPEC.md §3 "find_padded") ------------------------------------------------------------------------
 * What a sequence model reads: d_out[b, j, :] for b < n_bags, j < max_len — one slot per history position, zeros behind the end of a short
 * history, a long history cut to max_len — written by ONE launch, with no [n, dim] array in between.  Bags are mee_find_pooled's, clamped the
 * same way: end = min(d_bag_offsets[b+1], n), begin = min(d_bag_offsets[b], end), len = end - begin (a decreasing pair is an empty bag).
 * kept = min(len, max_len); flags = MEE_PAD_KEEP_FIRST keeps positions begin .. begin+kept-1, MEE_PAD_KEEP_LAST end-kept .. end-1; the j-th
 * kept position (batch order) fills slot j.
 *   d_out            [n_bags, max_len, dim] of out_dtype (MEE_DTYPE_F32 | MEE_DTYPE_BF16, a bf16 buffer 8-byte aligned).  A kept slot holds, bit
 *                    for bit, the row mee_find / mee_find_as returns for that key (the stored row, or the default row for an absent or reserved
 *                    key); every other slot is +0.0 in every element (bf16: 0x0000).  EVERY element is written: the caller never clears it.
 *   d_found          [n] nullable.  A kept position: as mee_find.  A position inside a bag that is not kept (truncated): not probed, 0.
 *   d_lengths_out    [n_bags] nullable: kept, per bag — the mask of the block.
 *   d_step_keys_out  [n] int64 and
 *   d_grad_index_out [n] uint32, both nullable: what the backward needs.  A kept position i in slot j of bag b: step key = d_keys[i], grad index =
 *                    b * max_len + j; a truncated one: EMPTY (padding, skipped by every operator) and 0.  The table step of the lookup is then
 *                    mee_apply_*_indexed(d_step_keys_out, the dense grad as [n_bags * max_len, dim], d_grad_index_out).  With d_grad_index_out
 *                    and n_bags * max_len >= 2^31 the call is MEE_ERR_INVALID_ARG (the indexed apply reads indices below 2^31).
 * A position that lies in no bag (before d_bag_offsets[0], at or after d_bag_offsets[n_bags]) is written in no per-position output.  Bags that
 * overlap (offsets that go down and up again) are served one by one; a position two bags share gets the per-position values of either.
 * Nothing is read past d_keys[n-1].  The table, its hit counters, its admission sketch and its status word are not touched.  mee_find_padded_as
 * never synchronises or allocates, can be captured, and may run on several streams at once.  mee_group_find_padded_as is the same EXCEPT in the
 * first call after mee_reserve on a member (below): that call synchronises the stream once and must not be captured — a group form is capturable
 * only while no member has been reserved since the group's last call.
 * Row storage: fp32 rows (HBM or pinned host memory) and bf16 rows (MEE_FLAG_BF16_ROWS: fp32 out widens exactly, bf16 out returns the stored
 * bits); an int8-row table is MEE_ERR_UNSUPPORTED.
 * mee_group_find_padded_as: n_bags = n_tables * bags_per_table, bag b belongs to member b / bags_per_table (bags_per_table need not be a multiple
 * of 4) and is, by definition, that member's mee_find_padded_as bag: its rows, its default row.  A uniform fp32 group or a bf16-row group; one
 * launch whatever the number of tables.  After mee_reserve on a member the next call re-reads that table's planes (one stream synchronisation).
 * MEE_ERR_INVALID_ARG, before anything is launched or written: a null table or group, null d_bag_offsets or d_out with bags to serve, null d_keys
 * with n > 0, max_len == 0, an unknown flag bit, an unknown out_dtype (MEE_DTYPE_INT8 included), a misaligned bf16 d_out, n_bags * max_len beyond
 * 2^56, the 2^31 rule above.  Zero bags succeed and write nothing.
 * Not served: mixed groups, int8-row tables, the sharded and peer-mapped forms, left padding or a pad value other than zero, located rows
 * (DESIGN.md §6).  Hot/cold pairs and groups of pairs: mee_find_padded_tiered / mee_group_find_padded_tiered below; only those count hits. */
enum { MEE_PAD_KEEP_FIRST = 0, MEE_PAD_KEEP_LAST = 1 };
int mee_find_padded_as(const mee_table* t, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags, size_t max_len,
                       uint32_t flags, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out,
                       uint32_t* d_grad_index_out, void* stream);
int mee_group_find_padded_as(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, size_t max_len,
                             uint32_t flags, void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out,
                             uint32_t* d_grad_index_out, void* stream);

/* The padded lookup over a hot/cold pair (SPEC.md §3 "Tiering") and over a group of pairs: mee_find_padded_as on the UNION of the two tables, bit
 * for bit, in ONE launch that probes the hot index, then the cold index for what the hot one missed, and takes each row from the plane that holds
 * it.  A kept position reads the hot table's row if `hot` holds its key, else the cold table's row if `cold` holds it, else a row of HOT's
 * default_value (reserved keys too); d_found[i] = 1 iff either tier holds the key.  d_out, d_lengths_out, d_step_keys_out, d_grad_index_out, the
 * truncated positions (found 0, step key EMPTY, grad index 0, no probe), the clamping of the offsets and the positions in no bag (left alone) are
 * mee_find_padded_as's.  flags = MEE_PAD_KEEP_*; count_flags = MEE_TIER_COUNT_COLD | MEE_TIER_COUNT_HOT, a word of its own because
 * MEE_PAD_KEEP_LAST and MEE_TIER_COUNT_COLD are both 1: every KEPT position found in a tier adds 1 to that slot's hit counter when that tier's bit
 * is set; a truncated position counts nothing.  fp32 rows only (a pair takes no narrow rows: MEE_ERR_UNSUPPORTED); fp32 or bf16 out.
 * mee_group_find_padded_tiered: member j of `hot` and member j of `cold` are the two tiers of pair j; n_bags = n_tables * bags_per_table, bag b is,
 * by definition, the pair form of pair b / bags_per_table on that bag (its rows, its hot default, its counters).
 * MEE_ERR_INVALID_ARG, before anything is launched or written: a null table or group; hot == cold (a group: also a table that is member j of both);
 * tiers that differ in device or dim (groups: or number of tables); an unknown bit in either flag word; a count bit without that tier's
 * MEE_FLAG_TRACK_HITS (a group: in EVERY member of that tier); and every refusal of mee_find_padded_as about the call's shape.  Zero bags succeed
 * and write nothing.  Both are one launch, never allocate and never synchronise — the group form EXCEPT in the first call after mee_reserve on a
 * member of either group, which re-reads that table's planes (one stream synchronisation, not capturable). */
int mee_find_padded_tiered(const mee_table* hot, const mee_table* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                           size_t max_len, uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype, uint8_t* d_found,
                           int64_t* d_lengths_out, int64_t* d_step_keys_out, uint32_t* d_grad_index_out, void* stream);
int mee_group_find_padded_tiered(mee_group* hot, mee_group* cold, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                                 size_t bags_per_table, size_t max_len, uint32_t flags, uint32_t count_flags, void* d_out, uint32_t out_dtype,
                                 uint8_t* d_found, int64_t* d_lengths_out, int64_t* d_step_keys_out, uint32_t* d_grad_index_out, void* stream);

/* ---- mixed groups: an embedding-bag collection whose tables differ in dim (SPEC.md §3 "Mixed groups") ------------------------
 * The members share a device (and, with max_apply_batch, an optimizer); every dim is a multiple of 4.  Pooled lookups only: bag b belongs
 * to member b / bags_per_table, and by definition every operator is the single-table operator of each member with its bags.
 * Output layout ("class-major"): a class = the members of one dim; classes by ascending dim, members inside a class in the caller's order.
 * Member j's bags_per_table bag rows are one contiguous [bags_per_table, dim_j] block and the blocks follow each other class by class, so
 * a class is one [T_c * bags_per_table, dim_c] array.  mee_mixed_group_layout reports every block's element offset (the same for fp32
 * and bf16 elements) and the total element count; d_bag_grads of the step has the same layout, fp32.  d_keys, d_bag_offsets, d_found
 * and d_located keep the caller's member order; d_located[i] = member << 48 | slot with the caller's member index (EMPTY when absent).
 *   mee_mixed_group_find_pooled   one launch.  insert_missing != 0: absent keys are first created in their member tables (initial row /
 *                                 state, as mee_group_find_or_insert; two more launches), d_found (required then) = present before the
 *                                 call, TABLE_FULL / RESERVED_KEY land on the member.  d_found / d_located nullable otherwise.
 *   mee_mixed_group_apply_*       mee_apply_*_indexed per member: position i takes the row of bag d_bag_of_position[i] (its index in the
 *                                 caller's order, as mee_group_apply_*_pooled) — per class one select launch and the grouped apply of
 *                                 mee_group_apply_*_pooled.  d_located (nullable): the handles mee_mixed_group_find_pooled of the SAME step filled.
 * A group whose members all share one dim runs the launches of mee_group_find_pooled_as / mee_group_apply_*_pooled, bit for bit.
 * Refusals as mee_group_create / mee_group_apply_*.  No weighted, jagged or unpooled form.  Calls that use the group's step buffers
 * (mee_mixed_group_apply_*) must be ordered by the caller. */
typedef struct mee_mixed_group mee_mixed_group;
int mee_mixed_group_create(mee_table* const* tables, uint32_t n_tables, uint64_t max_apply_batch, mee_mixed_group** out);
int mee_mixed_group_destroy(mee_mixed_group* g);
int mee_mixed_group_layout(const mee_mixed_group* g, uint64_t bags_per_table, uint64_t* elem_offsets /* [n_tables], nullable */,
                           uint64_t* total_elems /* nullable */);
int mee_mixed_group_find_pooled(mee_mixed_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                void* d_out, uint32_t out_dtype, uint8_t* d_found, int64_t* d_located /* nullable */, int mode,
                                int insert_missing, void* stream);
int mee_mixed_group_apply_adagrad_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                         const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located /* nullable */,
                                         size_t n, float lr, float eps, void* stream);
int mee_mixed_group_apply_adam_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located /* nullable */,
                                      size_t n, float lr, float beta1, float beta2, float eps, uint64_t step, void* stream);
int mee_mixed_group_set_tuning(mee_mixed_group* g, const char* name, int value);   /* forwarded to every class's apply */

/* ---- keyed output of the pooled group lookups (SPEC.md §3 "Keyed output") ------------------------------------------------------
 * The table-major lookups above write bag b = j * B + s (member j's sample s, B = bags_per_table, T = n_tables) as row b.  The keyed forms write
 * the SAME pooled rows, bit for bit, one row per sample with the members side by side, which is what a dense network reads:
 *     out[s * out_row_stride + col_j ... + dim_j)    col_j = the sum of dim_i over the members i < j in the caller's order (j * dim for a uniform group)
 * out_row_stride is in ELEMENTS, a multiple of 4, at least the width W = col_T; 0 means W.  A larger stride writes into a wider feature row: the
 * columns outside [0, W) of a row are never written.  d_out must be 16-byte aligned for fp32, 8-byte for bf16.
 * d_step_index_out (nullable, uint32 [n]): for every key position a bag covers, the row of the gradient that the pooled step reads for it —
 *     s * T + j  (uniform and tiered groups): mee_group_apply_*_pooled takes the keyed gradient [B, T * dim] (contiguous) AS IT IS, viewed [B * T, dim],
 *                with this array as d_grad_index — no gradient copy;
 *     b          (mixed groups): d_bag_of_position of mee_mixed_group_apply_*_pooled, whose class-major d_bag_grads mee_mixed_group_keyed_grads makes.
 * Positions no bag covers are not written.  d_found, d_located(_out), mode, insert_missing and flags are the table-major sibling's.
 *   mee_group_find_pooled_keyed          = mee_group_find_pooled_as without weights (fp32-row and bf16-row groups)
 *   mee_group_find_pooled_tiered_keyed   = mee_group_find_pooled_tiered, hit counting included; no located rows, as there
 *   mee_mixed_group_find_pooled_keyed    = mee_mixed_group_find_pooled
 *   mee_mixed_group_keyed_layout         host only: col_offsets[n_tables] (nullable) and W (nullable), in elements
 *   mee_mixed_group_keyed_grads          one launch: the keyed gradient [B, row_stride] (in_dtype MEE_DTYPE_F32 or MEE_DTYPE_BF16, widened) taken apart
 *                                        into the class-major fp32 buffer d_bag_grads_out (mee_mixed_group_layout); MEE_POOL_MEAN divides row b by
 *                                        (float)max(d_bag_offsets[b + 1] - d_bag_offsets[b], 1) (d_bag_offsets is read with MEE_POOL_MEAN only)
 * MEE_ERR_INVALID_ARG, before anything is launched or written: a null pointer where rows are due, an unknown mode or dtype, a stride below W or not a
 * multiple of 4, a misaligned d_out, T * B >= 2^32 with d_step_index_out.  MEE_ERR_UNSUPPORTED wherever the sibling is (d_located_out or
 * d_step_index_out on a bf16-row group: both serve a backward).  bags_per_table == 0 succeeds and writes nothing.  Sync-free and capturable.
 * No weighted, jagged, sharded or single-table form (a single table's [n_bags, dim] is keyed already). */
int mee_group_find_pooled_keyed(mee_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table, void* d_out,
                                uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found, int64_t* d_located_out /* nullable */,
                                uint32_t* d_step_index_out /* nullable */, int mode, void* stream);
int mee_group_find_pooled_tiered_keyed(mee_group* hot_group, mee_group* cold_group, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets,
                                       size_t bags_per_table, void* d_out, uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found,
                                       uint32_t* d_step_index_out /* nullable */, int mode, uint32_t flags, void* stream);
/* (the mixed group's three: the return type on a line of its own — tests/test_mixed_groups.py pins the list of the class-major operators, which it
 * reads off the one-line declarations above) */
int
mee_mixed_group_find_pooled_keyed(mee_mixed_group* g, const int64_t* d_keys, size_t n, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      void* d_out, uint32_t out_dtype, size_t out_row_stride, uint8_t* d_found, int64_t* d_located /* nullable */,
                                      uint32_t* d_step_index_out /* nullable */, int mode, int insert_missing, void* stream);
int
mee_mixed_group_keyed_layout(const mee_mixed_group* g, uint64_t* col_offsets /* [n_tables], nullable */, uint64_t* width /* nullable */);
int
mee_mixed_group_keyed_grads(mee_mixed_group* g, const void* d_keyed_grads, uint32_t in_dtype, size_t row_stride, size_t bags_per_table,
                                const uint64_t* d_bag_offsets /* MEE_POOL_MEAN only */, int mode, float* d_bag_grads_out, void* stream);
/* mee_mixed_group_apply_adagrad_pooled with the FTRL-Proximal rule (mee_apply_ftrl, below): (beta, l1, l2) after lr, checked before the first launch */
int
mee_mixed_group_apply_ftrl_pooled(mee_mixed_group* g, const int64_t* d_keys, const uint64_t* d_bag_offsets, size_t bags_per_table,
                                      const float* d_bag_grads, const uint32_t* d_bag_of_position, const int64_t* d_located /* nullable */,
                                      size_t n, float lr, float beta, float l1, float l2, void* stream);

/* ---- sparse optimizers (north_star "sparse-optimizer (Adagrad/Adam) scatter-update"; SPEC.md §4) -------- */
int mee_apply_adagrad(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n, float lr, float eps,
                      void* stream);
int mee_apply_adam(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n, float lr, float beta1,
                   float beta2, float eps, uint64_t step, void* stream);
/* The same step on the slots mee_find_located reported for these keys in the forward pass of the step: the main pass needs no
 * probe of its own (128 B of bucket line and one dependent memory round trip less per key).  d_keys is still required (duplicate
 * reduction); a handle of -1 (key absent at lookup time) receives no update; out-of-range handles are ignored. */
int mee_apply_adagrad_located(mee_table* t, const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr,
                              float eps, void* stream);
int mee_apply_adam_located(mee_table* t, const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr,
                           float beta1, float beta2, float eps, uint64_t step, void* stream);
/* The same with an indirection on the grads: position i takes row d_grad_index[i] of d_grads ([n_grad_rows, dim]) — the
 * backward of a pooled lookup (every key of a bag receives the bag's grad row; for MEE_POOL_MEAN the caller scales the bag
 * rows by 1/length).  Indices >= n_grad_rows are clamped to the last row: bad caller data never reads out of bounds. */
int mee_apply_adagrad_indexed(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index,
                              size_t n, float lr, float eps, void* stream);
int mee_apply_adam_indexed(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index,
                           size_t n, float lr, float beta1, float beta2, float eps, uint64_t step, void* stream);
/* FTRL-Proximal (SPEC.md §4 "FTRL-Proximal"; McMahan et al. 2013, Algorithm 1) on a table created with MEE_OPT_FTRL: three fp32 planes per key,
 * the row w (plane 0), z (plane 1, +0.0 at creation) and n (plane 2, config.initial_accumulator at creation).  lr is the paper's alpha, beta its
 * beta, l1 / l2 its lambda1 / lambda2; g is the key's reduced gradient (duplicates summed in fp64 and applied once, as for the other rules):
 *     n' = n + g*g;  sig = (sqrt(n') - sqrt(n)) / lr;  z' = (z + g) - sig*w;
 *     w' = |z'| <= l1 ? +0.0 : (copysign(l1, z') - z') / ((beta + sqrt(n')) / lr + l2)
 * every operation rounded to fp32 on its own, no fma: a coordinate whose |z'| stays within l1 is exactly +0.0.  The three forms (by key, located,
 * indexed) are the Adagrad entry points' with (beta, l1, l2) after lr: absent keys ignored, the same handles, clamping, pending partition and capture.
 * MEE_ERR_INVALID_ARG before anything is launched or written: lr not finite or <= 0; beta, l1 or l2 NaN or negative.  MEE_ERR_UNSUPPORTED on a
 * table (or a group, below) of another optimizer.  Out of scope: the sharded step (mee_sharded_apply_*) and the peer-mapped mutators know
 * Adagrad and Adam only. */
int mee_apply_ftrl(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n, float lr, float beta, float l1, float l2, void* stream);
int mee_apply_ftrl_located(mee_table* t, const int64_t* d_keys, const int64_t* d_slots, const float* d_grads, size_t n, float lr, float beta,
                           float l1, float l2, void* stream);
int mee_apply_ftrl_indexed(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n_grad_rows, const uint32_t* d_grad_index, size_t n,
                           float lr, float beta, float l1, float l2, void* stream);
/* Optional split of an apply: mee_apply_prepare groups the batch's keys (occurrence counts, per-key position lists) — everything
 * that does not need the grads — so it can run early (e.g. on a side stream beside the forward lookup and the dense
 * model); the following mee_apply_adagrad / mee_apply_adam with the SAME d_keys / n then only streams the updates.
 * While a prepared apply is pending only mee_find*, mee_locate, mee_size/status/export and mee_apply_* are accepted;
 * mee_apply_discard drops it.  The caller orders the two streams (event / wait).  (The partition a training forward leaves —
 * mee_find_located_prepare / mee_find_or_insert_located_prepare — is softer: a mutator or mee_reserve that comes before the backward drops
 * it itself, and the apply that follows partitions its batch again.) */
int mee_apply_prepare(mee_table* t, const int64_t* d_keys, size_t n, void* stream);
int mee_apply_discard(mee_table* t, void* stream);
/* Duplicate-key reduction on its own (SPEC.md §4), sync-free: what a rank runs on its gradients before they travel to the keys' owners, so that
 * one (key, summed row) pair per DISTINCT key crosses xGMI instead of one row per occurrence.  Outputs sized for n, padded like mee_dedup_keys' (below):
 *   d_uniq_out[n]          every distinct non-reserved key exactly once, at an unspecified position; MEE_EMPTY_KEY elsewhere (padding, possibly BETWEEN keys)
 *   d_gsum_out[n, dim]     at a key's position: the rows of its occurrences added up in fp64 and rounded once to fp32 (a key that occurs once: its row, bit for
 *                          bit); rows at padding positions are NOT written.  d_grads / d_gsum_out are nullable together (keys, counts and inverse only);
 *                          dim = the table's dim
 *   d_counts_out[n]        (nullable) occurrences of the key; 0 at padding positions
 *   d_inverse_out[n]       (nullable) index of d_keys[i] in d_uniq_out, or miss_index for reserved keys
 * The number of distinct keys never travels to the host; consumers take the padded arrays at their fixed length n (every operator and
 * mee_partition_padded skip MEE_EMPTY_KEY).  Uses the table's per-batch scratch only (no table row is read): n <= config.max_batch. */
int mee_dedup_sum(mee_table* t, const int64_t* d_keys, const float* d_grads, size_t n, int64_t* d_uniq_out,
                  float* d_gsum_out, uint32_t* d_counts_out, int64_t* d_inverse_out, int64_t miss_index,
                  void* stream);

/* The keys-only, sync-free form (what a sharded lookup of a skewed batch needs before the exchange): every distinct non-reserved
 * key of the batch occurs exactly once in d_uniq_out[0 .. n), at an unspecified position; every other entry is MEE_EMPTY_KEY
 * (padding — it may lie BETWEEN the keys: each hash bucket of the batch fills the front of a slice of its own, so that no block
 * has to reserve its place from a shared counter); d_inverse_out[i] = index of d_keys[i] in d_uniq_out, or miss_index for
 * reserved keys.  The number of distinct keys never travels to the host: consumers take the padded array at its fixed length n
 * (padding is skipped by every operator and by mee_partition_padded). */
int mee_dedup_keys(mee_table* t, const int64_t* d_keys, size_t n, int64_t* d_uniq_out, int64_t* d_inverse_out, int64_t miss_index,
                   void* stream);

/* ---- hashing and shard routing (README.md:2 "distributed"; SPEC.md §1, §5) ----------------------------- */
/* any output nullable: mix64(key), bucket(key, n_buckets), owner(key, n_shards). */
int mee_hash_batch(const int64_t* d_keys, size_t n, uint64_t n_buckets, uint32_t n_shards, uint64_t* d_mix_out,
                   uint64_t* d_bucket_out, uint32_t* d_owner_out, void* stream);
int mee_router_create(int32_t device, uint64_t max_batch, uint32_t n_shards, mee_router** out);
int mee_router_destroy(mee_router* r);
/* stable partition by owner: d_send_keys[n], d_counts[n_shards] (uint64), d_perm[n] (batch position). */
int mee_partition(mee_router* r, const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts,
                  int64_t* d_perm, void* stream);
/* the same, dropping MEE_EMPTY_KEY positions (padding belongs to no shard): the counts add up to the non-padding keys, only the
 * first sum(counts) entries of d_send_keys / d_perm are written. */
int mee_partition_padded(mee_router* r, const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts,
                         int64_t* d_perm, void* stream);
/* out[perm[q], :] = rows[q, :] (row_bytes multiple of 4); inverse of the partition for returned rows/masks. */
int mee_scatter_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out,
                     void* stream);
/* out[q, :] = rows[perm[q], :] — forward permutation of per-key payloads (values / grads) into send order. */
int mee_gather_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out,
                    void* stream);

/* ---- embedding bags over a sharded table (SPEC.md §5 "Pooled lookups"): the partition is stable, so the positions of bag b owned by rank p are
 * one contiguous RUN of destination segment p.  The owner pools every run (mee_find_pooled over the received keys) and one row per run travels
 * instead of one per key.  All three take a stream, never synchronise and can be captured.  Caller data is never used as an address unchecked:
 * perm entries are only compared, bags and run indices are kept inside their arrays (as mee_apply_*_indexed clamps d_grad_index).
 *
 * mee_bag_runs — the source's side.  d_perm[n] / d_counts[n_shards] are what mee_partition wrote for the batch, d_bag_offsets[n_bags + 1] the bags of
 * the batch (they must partition [0, n): offsets[0] = 0, non-decreasing, offsets[n_bags] = n).  A run starts at the first entry of a segment and
 * wherever the bag of perm[q] differs from the bag of perm[q - 1] (the bag of a position: by search in d_bag_offsets; empty bags have no run).
 *   d_run_bag[R]  (uint32) the bag of each run        d_run_len[R]  (uint32) its positions        d_run_counts[n_shards]  (uint64) runs per segment
 * Runs are listed in segment order, R = sum(d_run_counts) <= n: size d_run_bag / d_run_len for n.  n <= the router's max_batch. */
int mee_bag_runs(mee_router* r, const int64_t* d_perm, const uint64_t* d_counts, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                 uint32_t* d_run_bag, uint32_t* d_run_len, uint64_t* d_run_counts, void* stream);
/* mee_run_offsets — the owner's side.  d_run_len[n_runs] = the run lengths received from all ranks, in source-rank order (n_runs <= n_shards x
 * max_batch).  d_offsets[n_runs + 1] (uint64) = their exclusive prefix sum: the d_bag_offsets of mee_find_pooled over the received keys, one
 * "bag" per run.  d_run_of_key[n_keys] (uint32, nullable) = the run of every received key: the d_grad_index of mee_apply_*_indexed over one
 * gradient row per run. */
int mee_run_offsets(mee_router* r, const uint32_t* d_run_len, size_t n_runs, uint64_t* d_offsets, uint32_t* d_run_of_key, size_t n_keys,
                    void* stream);
/* mee_combine_bag_runs — back at the source.  d_partials[n_runs, dim] (fp32, 16-byte aligned) = the owners' pooled rows of this rank's runs, in
 * the order mee_bag_runs listed them; d_run_bag / d_run_counts as it wrote them.  d_out[n_bags, dim], fp32 or bf16 (out_dtype = MEE_DTYPE_*):
 * the partial rows of bag b in ascending owner rank — the first one copied, each further one added in fp32 (no fma) —, for MEE_POOL_MEAN
 * then divided by (float)(bag length), for bf16 then rounded once; a bag without a run (an empty bag) is zeros.  No atomics: the order is this
 * one on every run.  dim: a positive multiple of 4. */
int mee_combine_bag_runs(mee_router* r, const float* d_partials, const uint32_t* d_run_bag, const uint64_t* d_run_counts, size_t n_runs,
                         const uint64_t* d_bag_offsets, size_t n_bags, uint32_t dim, int mode, void* d_out, uint32_t out_dtype, void* stream);

/* ---- table groups over sharded tables (SPEC.md §5 "Groups"): owner(key) does not depend on the table and the partition is stable, so ONE mee_partition
 * serves the whole jagged batch of a group, and inside every owner segment the entries of member 0 come before those of member 1, and so on.  Both calls
 * take a stream, never synchronise, read nothing back and can be captured; caller data is never used as an address unchecked.
 *
 * mee_segment_counts — the source's side.  d_perm[n] / d_counts[n_shards] are what mee_partition wrote, d_offsets[n_tables + 1] the member segments of
 * the batch (non-decreasing).  d_cell_counts[n_shards, n_tables] (uint64): cell (p, j) = the number of entries of owner segment p whose batch position
 * lies in [offsets[j], offsets[j + 1]).  Positions outside [offsets[0], offsets[n_tables]) belong to no cell.  Row p is what rank p is sent as counts;
 * its sum is the number of keys it is sent.  n <= the router's max_batch (MEE_ERR_BATCH_TOO_LARGE), 1 <= n_tables <= 1024. */
int mee_segment_counts(mee_router* r, const int64_t* d_perm, const uint64_t* d_counts, size_t n, const uint64_t* d_offsets, size_t n_tables,
                       uint64_t* d_cell_counts, void* stream);
/* mee_regroup — the owner's side.  d_recv_keys[n_recv] = the keys received from all ranks, source-major: source 0's members 0 … n_tables - 1, then
 * source 1's, …; d_recv_cells[n_shards, n_tables] (uint64) = the received cell counts, row s from source rank s.  Writes the batch TABLE-MAJOR, the
 * order the mee_group_* operators take: member j, inside it source rank ascending, inside that arrival order.
 *   d_keys_out[n_recv]     the keys           d_order_out[n_recv]  (int64) order[q] = the source-major index of table-major position q, the convention
 *   d_offsets_out[n_tables + 1] (uint64) the member offsets        of d_perm: mee_gather_rows brings received rows into table-major order,
 *                                                                  mee_scatter_rows brings result rows back into source-major order
 * Positions past the sum of the cells are left alone.  n_recv <= n_shards x max_batch and < 2^32 - 2048 (MEE_ERR_BATCH_TOO_LARGE); 1 <= n_tables <= 1024
 * and n_shards x n_tables <= 8128.  16-byte accesses when d_recv_keys, d_keys_out and d_order_out are 16-byte aligned. */
int mee_regroup(mee_router* r, const int64_t* d_recv_keys, const uint64_t* d_recv_cells, size_t n_recv, size_t n_tables, int64_t* d_keys_out,
                int64_t* d_order_out, uint64_t* d_offsets_out, void* stream);

/* ---- sharded find over peer-mapped memory (README.md:2 "distributed"; SPEC.md §5) ---------------------------------
 * One context per rank; all ranks use the same n_shards / slots_per_peer / max_batch / dim.  The local buffers
 * (key inbox, destination inbox, fill counts, result rows, found bytes, and the payload-row inbox if any) are exported as HIP IPC handles, the caller
 * exchanges them (any side channel) and connects.  Per lookup, after mee_partition:
 *   mee_p2p_push  stores this rank's keys + batch positions into their owners' inboxes            (xGMI stores)
 *   -- barrier across ranks on the stream --
 *   mee_p2p_find  probes what arrived and stores each row straight into the requester's buffers   (xGMI stores)
 *   -- barrier across ranks on the stream --
 * after which mee_p2p_buffers() rows/found [0, n) hold the result in batch order.  slots_per_peer bounds how many keys
 * one rank may send to one owner per lookup; exceeding it drops keys and sets bit 0 of mee_p2p_status. */
int mee_p2p_create(int32_t device, uint32_t n_shards, uint32_t rank, uint64_t slots_per_peer, uint64_t max_batch, uint32_t dim,
                   int with_payload, mee_p2p** out);
int mee_p2p_destroy(mee_p2p* c);
#define MEE_P2P_BUFFERS 6
int mee_p2p_export(mee_p2p* c, void* handles /* MEE_P2P_BUFFERS x MEE_IPC_HANDLE_BYTES */);
int mee_p2p_connect(mee_p2p* c, const void* all_handles /* n_shards x MEE_P2P_BUFFERS x MEE_IPC_HANDLE_BYTES, rank-major */);
/* result buffers: max_batch + 1 rows / bytes — the spare last one is never written by a lookup; a caller that expands a
 * de-duplicated lookup through an index array parks its "no such key" positions there. */
int mee_p2p_buffers(mee_p2p* c, float** d_out, uint8_t** d_found);
int mee_p2p_push(mee_p2p* c, mee_router* r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts, size_t n,
                 void* stream);
int mee_p2p_find(mee_p2p* c, const mee_table* t, void* stream);
/* Mutators over peer-mapped memory (contexts created with with_payload != 0): push (key, row) pairs into the owners'
 * inboxes; every segment is padded to slots_per_peer with MEE_EMPTY_KEY (= padding, SPEC.md §2), so after the barrier
 * the owner hands its WHOLE inbox — mee_p2p_inbox(): n_shards x slots_per_peer keys and rows, ordered by source rank then
 * batch position — to mee_insert / mee_assign / mee_apply_* with a fixed n; a second barrier frees the inbox.  d_rows may be
 * null: keys only, still padded (the owner runs mee_find_or_insert over the inbox, then mee_p2p_find returns the rows). */
int mee_p2p_push_rows(mee_p2p* c, mee_router* r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts,
                      const float* d_rows, size_t n, void* stream);
int mee_p2p_inbox(mee_p2p* c, int64_t** d_keys, float** d_rows, uint64_t* n_slots);
/* The barrier of the sequences above without a collective library: a one-wave kernel announces this rank's arrival in a
 * flag word on every peer and waits (bounded: 5 s, then bit 1 of mee_p2p_status) until every peer has announced its own.
 * Collective: every rank calls it the same number of times, in the same order relative to its pushes and finds. */
int mee_p2p_barrier(mee_p2p* c, void* stream);
int mee_p2p_status(mee_p2p* c, uint32_t* bits_out, void* stream); /* [syncs]; bit 0: inbox overflow, bit 1: barrier time-out */


/* ---- row-sharded table over RCCL (README.md:2 "distributed"; SPEC.md §5; SURVEY.md §8b "sharded variants take a communicator
 * handle", §8e) -------------------------------------------------------------------------------------------------------------
 * One process per GPU; every rank owns the keys with owner(key, G) == rank in its own mee_table and creates one context over
 * an RCCL communicator of the G ranks.  Every mee_sharded_* operator below is COLLECTIVE: all ranks call it, in the same order,
 * each with its own batch (n may differ per rank, 0 included).  On the caller's stream it runs
 *     mee_partition -> keys (+ value / gradient rows) to their owners: ncclGroupStart, G x ncclSend/ncclRecv, ncclGroupEnd
 *     -> the local table's operator over what arrived, ordered by source rank then batch position (so last-wins holds across
 *     ranks) -> rows and found bytes back in ONE grouped exchange -> un-permute into batch order.
 * Results are those of ONE table holding all shards (SPEC.md §5).  d_* pointers are device memory on the communicator's device.
 *
 * `nccl_comm` is an ncclComm_t passed as void*: the caller's own (borrowed, must outlive the context), or one made with the
 * three helpers below by callers that do not link RCCL themselves (the library binds librccl.so.1 at first use; the environment
 * variable MEE_RCCL_LIB names another library to bind instead — a particular RCCL build, or the test suite's stand-in).
 *
 * Segment layout, fixed at creation:
 *   pad_slack = 0   exact: message sizes come from a counts exchange and ONE host synchronisation per operator [syncs].
 *   pad_slack >= 1  padded: every (source, owner) segment holds max_batch / G * pad_slack + 1024 positions, unused ones padded
 *                   with MEE_EMPTY_KEY; message sizes are constants and nothing returns to the host.  A batch that sends one
 *                   owner more than that loses the surplus keys and sets bit 0 of mee_sharded_status (check it when convenient;
 *                   skewed batches: mee_dedup_keys first, or the exact layout).  Mutators then hand the local table G x segment
 *                   positions per call: create it with max_batch >= that.
 *
 * Errors inside a collective operator: everything a rank needs for an operator is allocated when its context is created (owner-side buffers
 * for G x max_batch arrivals; every rank must pass the same max_batch and pad_slack — checked collectively at creation), so no rank can
 * drop out for memory between two exchange steps.  If an RCCL call itself fails, the context aborts its communicator (ncclCommAbort: peers
 * blocked in the same collective return with an error instead of waiting forever) and every later call on it returns MEE_ERR_RCCL.
 * OWNERSHIP after an abort: a context only borrows its communicator, and ncclCommAbort frees it.  The abort is recorded per communicator:
 * every OTHER context that shares it fails at once with MEE_ERR_RCCL as well (none of them touches the freed communicator again),
 * mee_comm_destroy() of an aborted communicator does nothing and returns MEE_OK, and a caller that passed in an ncclComm_t of its own asks
 * mee_comm_aborted(comm) — 1: aborted and freed, do NOT call ncclCommDestroy on it — before it destroys it. */
#define MEE_COMM_ID_BYTES 128
int mee_comm_unique_id(void* id_out /* MEE_COMM_ID_BYTES */);                    /* ncclGetUniqueId: one rank calls, all ranks share the bytes */
int mee_comm_create(const void* id, uint32_t n_ranks, uint32_t rank, int32_t device, void** comm_out); /* ncclCommInitRank (collective) */
int mee_comm_destroy(void* comm);
int mee_comm_aborted(void* comm);   /* 1: this library aborted (and thereby freed) the communicator after an RCCL error.  The mark belongs to the ADDRESS: it is cleared when a
                                     * context is created on a communicator at that address again (mee_sharded_create*: the caller vouches that a live one is there) and by mee_comm_create */
int mee_sharded_create(mee_table* local, void* nccl_comm, uint64_t max_batch /* largest n of a rank per call: the same on every rank */,
                       double pad_slack, mee_sharded** out);
/* The same with options (BASELINE configs[4]; SURVEY.md §7 lever (a)):
 *   cold   the shard is a hot/cold PAIR: `local` holds its hot keys in HBM, `cold` (a table created with MEE_MEM_HOST_PINNED, same dim and
 *          optimizer, same device) the rest.  A key lives in exactly one of the two.  On the owner side a lookup is mee_find on the hot
 *          table + mee_find_missing on the cold one over the same buffers; assign / remove / apply_* go to both (each ignores keys it does
 *          not hold, found masks are OR-ed); new keys are created in the hot table while it holds fewer than hot_key_limit keys (0 = 3/4 of
 *          its capacity; an upper bound is kept on the host and refreshed with one mee_size — a synchronisation — only when it is hit),
 *          else in the cold one.  Which keys are hot is the caller's policy (mee_find_plane / mee_assign_plane move a key with its state).
 *   MEE_SHARDED_DEDUP   lookups (find, find_or_insert) exchange only the batch's DISTINCT keys: mee_dedup_keys on a scratch table of the
 *          context's own -> the padded unique list is partitioned (padding belongs to no shard) -> keys out, rows back -> every occurrence
 *          takes its key's row.  mee_sharded_apply_adagrad sends ONE (key, summed gradient row) pair per distinct key of the
 *          rank's batch: mee_dedup_sum adds the rank's rows of a key up in fp64 and rounds once, the owner's apply adds the ranks' partial sums
 *          up in fp64 again — within 1e-6 (relative) of the un-aggregated update, not bit-identical to it (one extra rounding per rank and key).
 *          mee_sharded_apply_adam sends its pairs un-aggregated under this flag too: Adam's step hardly depends on the size of the gradient, so
 *          where the ranks' partial sums cancel, one rounding of a partial sum would reach the row as a large relative error (SPEC.md §5).
 *          On skewed key streams the bytes on xGMI then scale with the distinct keys, in both directions of a training step, while the result
 *          counts lookups.  Costs ~0.1-0.2 ms of local work per 1M keys: it pays where the saved link time exceeds that. */
enum { MEE_SHARDED_DEDUP = 1u };
typedef struct mee_sharded_options {
    uint32_t struct_size;     /* = sizeof(mee_sharded_options); ABI guard */
    uint32_t flags;           /* MEE_SHARDED_* bits */
    uint64_t max_batch;       /* largest n of a rank per call: the same on every rank */
    double   pad_slack;       /* 0 = exact segments, >= 1 = padded segments (see above) */
    mee_table* cold;          /* nullable: the cold tier behind `local` */
    uint64_t hot_key_limit;   /* with `cold`: keys the hot table may hold before new keys go cold (0 = 3/4 of its capacity) */
} mee_sharded_options;
int mee_sharded_create_ex(mee_table* local, void* nccl_comm, const mee_sharded_options* options, mee_sharded** out);
int mee_sharded_destroy(mee_sharded* s);
int mee_sharded_info(const mee_sharded* s, uint32_t* n_shards, uint32_t* rank, uint64_t* segment_capacity /* 0 = exact layout */);
int mee_sharded_find(mee_sharded* s, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found /* nullable */, void* stream);
int mee_sharded_find_or_insert(mee_sharded* s, const int64_t* d_keys, size_t n, float* d_out, uint8_t* d_found, void* stream);
/* The two lookups with fp32 OR bf16 result rows (MEE_DTYPE_*, "typed output" above).  MEE_DTYPE_F32: they ARE mee_sharded_find /
 * mee_sharded_find_or_insert, bit for bit and byte for byte on the wire.  MEE_DTYPE_BF16: d_out is [n, dim] bf16, 8-byte aligned; the result is
 * the fp32 result of the same call with every element rounded once to bf16 — by the key's OWNER, before the rows travel, so the rows leg of the
 * way back carries 2·dim bytes per key instead of 4·dim and no fp32 row crosses the link (a tiered shard rounds after its two fp32 tier passes).
 * d_found, the status bits, the table after a find_or_insert and the keys an overflowing padded segment drops are those of the fp32 call;
 * dropped keys get bf16(default_value) and found = 0.  COLLECTIVE like every mee_sharded_* operator, and every rank passes the SAME out_dtype
 * to a given call: a mismatch is a message-size mismatch between the two ends of a send/receive pair.  fp32 and bf16 calls may alternate freely
 * on one context. */
int mee_sharded_find_as(mee_sharded* s, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found /* nullable */, void* stream);
int mee_sharded_find_or_insert_as(mee_sharded* s, const int64_t* d_keys, size_t n, void* d_out, uint32_t out_dtype, uint8_t* d_found, void* stream);
/* Bytes this context has handed to ncclSend / ncclRecv since it was created (either pointer nullable): a host-side counter, never synchronises.
 * Counted: every message to or from ANOTHER rank — keys, payload rows, rows and found bytes on the way back, and the exact layout's counts
 * exchange (8 B to and from every peer per operator).  Not counted: the segment a rank keeps for itself (a device copy) and the all-reduces of
 * creation and mee_sharded_size.  One exact-layout lookup without MEE_SHARDED_DEDUP, with k_out of the rank's keys owned by other ranks, k_in
 * keys arriving from other ranks and e = 4 (fp32) or 2 (bf16) bytes per element:
 *     sent     = 8·k_out + (e·dim + 1)·k_in  + 8·(G - 1)
 *     received = 8·k_in  + (e·dim + 1)·k_out + 8·(G - 1) */
int mee_sharded_traffic(const mee_sharded* s, uint64_t* sent_bytes, uint64_t* received_bytes);
int mee_sharded_insert(mee_sharded* s, const int64_t* d_keys, const float* d_values, size_t n, void* stream);
int mee_sharded_assign(mee_sharded* s, const int64_t* d_keys, const float* d_values, size_t n, uint8_t* d_found, void* stream);
int mee_sharded_remove(mee_sharded* s, const int64_t* d_keys, size_t n, uint8_t* d_found, void* stream);
/* one update per distinct key over everything that reaches a shard.  Exact layout: when more pairs arrive than the local table's max_batch
 * (a skewed step, or G ranks x max_batch against a table made for one rank's batch) the arrivals are split by key range — every key's pairs
 * in one chunk, one apply per chunk (one more host synchronisation; MEE_ERR_BATCH_TOO_LARGE only if a single chunk still exceeds max_batch,
 * i.e. one key dominates).  Padded layout: the local table receives G x segment positions per call, a constant known to every rank: a
 * table with a smaller max_batch is refused on every rank alike, before anything is exchanged. */
int mee_sharded_apply_adagrad(mee_sharded* s, const int64_t* d_keys, const float* d_grads, size_t n, float lr, float eps, void* stream);
int mee_sharded_apply_adam(mee_sharded* s, const int64_t* d_keys, const float* d_grads, size_t n, float lr, float beta1, float beta2,
                           float eps, uint64_t step, void* stream);
int mee_sharded_size(mee_sharded* s, size_t* n_out, void* stream);       /* [syncs] keys stored over all shards (ncclAllReduce) */
/* [syncs]; bit 0: a padded segment overflowed (the lookups it could not send returned the default row and found = 0; mutators lost the
 * surplus pairs).  Sticky until mee_sharded_clear_status. */
int mee_sharded_status(mee_sharded* s, uint32_t* bits_out, void* stream);
int mee_sharded_clear_status(mee_sharded* s, void* stream);

/* ---- change log and delta export (README.md:2 "dynamic lookuptable-style"; SPEC.md §3 "Change log") ------------------------------------------
 * A change log is a SET of int64 keys on one device: a table key plane and nothing else — `capacity` rounded as mee_table_create rounds it (16 x the
 * smallest prime >= capacity / 16), the hash and probe sequence of SPEC.md §2, 8 bytes per slot — and two device words: `size`, the distinct keys stored,
 * and `invalid`, sticky.  It belongs to no table: the caller notes the keys of every batch that may change a table's membership, rows or optimizer
 * planes (the Python layer does so in every mutator of a tracked table), and mee_export_changed turns the set into the table's delta.
 *
 * mee_changes_note adds every key of the batch that is neither MEE_EMPTY_KEY nor MEE_RECLAIMED_KEY (both are padding: ignored silently); duplicates — inside
 * a batch and across calls — are stored once.  A key for which the set has no room is not stored and sets `invalid`; nothing else is touched.  One launch,
 * no synchronisation, no allocation: safe under stream capture.  n = 0 succeeds and launches nothing; a null log, or null keys with n > 0, is refused.
 * mee_changes_group_note notes position i of segment j = [d_offsets[j], d_offsets[j + 1]) of a jagged batch in logs[j], in ONE launch whatever the number
 * of logs; d_offsets holds n_tables + 1 values on the device and is never trusted: a position outside [d_offsets[0], d_offsets[n_tables]) or at or
 * past n is noted nowhere.  The logs of a group share one device (at most 1024 of them).
 * mee_changes_clear empties the set and resets `invalid`; mee_changes_invalidate sets `invalid` (the caller did something the log cannot name, e.g.
 * mee_clear); mee_changes_info_get [syncs, the whole device] reads the two words back.
 *
 * mee_export_changed walks the log's slots [slot_begin, min(slot_end, the log's capacity)) and probes every key stored there in `t` — read-only, as
 * mee_find: no key of `t` or `c` may change while it runs.  A key `t` holds is appended to the upsert outputs: the key, its values row and every
 * optimizer plane `t` has, bit for bit, in one shared unspecified order (an output for a plane `t` lacks is ignored; a null state output skips that
 * plane).  A key `t` does not hold is appended to d_removed_out.  d_counts_out (device, 2 words, zeroed by the call first) receives the number of upserts
 * and the number of removed keys; nothing is written at or past them; every key of the range appears exactly once, in one of the two lists.  cap and
 * removed_cap (in keys) must both be at least the number of slots in the range: anything smaller is MEE_ERR_INVALID_ARG before any launch.  No
 * synchronisation, no allocation.  Refused before anything is launched or written: a null table, log, keys / values / removed / counts output, a
 * bf16-row or int8-row table (MEE_ERR_UNSUPPORTED: a serving table has no training delta), `t` and `c` on different devices.
 * The contract (SPEC.md §3): if every key whose membership, row or state plane changed in `t` since the log was last cleared was noted and invalid == 0,
 * then a table that equalled `t` at that moment equals `t` now after mee_insert + mee_assign_plane of the upserts and mee_remove of the removed keys,
 * taken over a partition of the log's slots. */
typedef struct mee_changes mee_changes;
typedef struct mee_changes_group mee_changes_group;
typedef struct mee_changes_info {
    uint64_t capacity, size;
    uint32_t invalid, pad;
} mee_changes_info;
int mee_changes_create(int32_t device, uint64_t capacity, mee_changes** out);
int mee_changes_destroy(mee_changes* c);
int mee_changes_note(mee_changes* c, const int64_t* d_keys, size_t n, void* stream);
int mee_changes_group_create(mee_changes* const* logs, uint32_t n_tables, mee_changes_group** out);
int mee_changes_group_destroy(mee_changes_group* g);
int mee_changes_group_note(mee_changes_group* g, const int64_t* d_keys, const uint64_t* d_offsets /* [n_tables + 1], device */, size_t n, void* stream);
int mee_changes_info_get(const mee_changes* c, mee_changes_info* out);   /* [syncs] */
int mee_changes_clear(mee_changes* c, void* stream);
int mee_changes_invalidate(mee_changes* c, void* stream);
int mee_export_changed(const mee_table* t, const mee_changes* c, uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out,
                       float* d_state1_out /* nullable */, float* d_state2_out /* nullable */, size_t cap, int64_t* d_removed_out, size_t removed_cap,
                       uint64_t* d_counts_out /* device, 2 words */, void* stream);

/* ---- publish: a change log's delta of a trainer table, device to device into a serving table (SPEC.md §3 "Publish") ----------------------------
 * mee_publish_changed walks the log's slots [slot_begin, min(slot_end, the log's capacity)) and probes every key stored there in `src` — read-only, as
 * mee_find; `src` and the log are never written.  A key `src` holds is an upsert: `dst` ends up holding it with src's VALUES row (no state plane travels) —
 * bit for bit in an fp32-row dst, rounded once by the rule of SPEC.md "Output type" in a bf16-row dst: exactly what mee_insert(dst, key, row) stores.  A
 * key dst lacks is placed by the placement rule of SPEC.md §2; a slot created in a dst with MEE_FLAG_TRACK_HITS starts at counter 0, an existing one keeps
 * its counter.  A key `src` does not hold is removed from dst as mee_remove removes it (no-op if dst lacks it).  A key for which dst has no room is
 * dropped: dst stays without it and MEE_STATUS_TABLE_FULL goes to dst's status word.
 * d_counts_out (device, 4 words, zeroed by the call first): [0] the keys that got a slot in dst (new or overwritten), [1] the keys src does not hold,
 * [2] the keys dropped for lack of room, [3] the log's `invalid` word as the launch read it (non-zero: the log does not name every change — rebuild dst).
 * After the call over a partition of the log's slots dst equals — in mee_export sorted by key, mee_size and status bits — what mee_insert of
 * mee_export_changed's upserts followed by mee_remove of its removed keys leaves; so a dst that equalled "src rounded" when the log was last cleared
 * equals "src rounded" now.  Two launches, no [n, dim] buffer, no synchronisation, no allocation: safe under stream capture; independent of either
 * table's max_batch.  Slot handles of dst from before the call are stale.  No lookup of dst may run concurrently (stream order).
 * Refused before anything is launched or written: a null table, log or counts, src == dst, a dim or device mismatch among the three
 * (MEE_ERR_INVALID_ARG); a dst with an optimizer, a src with bf16 or int8 rows, a dst with int8 rows (MEE_ERR_UNSUPPORTED).  slot_begin >= slot_end
 * succeeds and zeroes the counts.
 * mee_group_publish_changed is mee_publish_changed on every member j of two groups over the WHOLE of log j, in one launch sequence whatever the number
 * of tables: src a group of fp32-row tables, dst a group of optimizer-less fp32-row tables or of bf16-row tables, logs a mee_changes_group, all three of
 * the same n_tables, dim and device; no table may be a member twice across the two groups.  d_counts_out holds n_tables x 4 words, member j's at 4j.
 * A member whose log is empty costs its slot scan.  Like every group operator it re-reads, behind a stream synchronisation, the planes of a member that
 * mee_reserve moved: the first call after a reserve must not be captured. */
int mee_publish_changed(const mee_table* src, const mee_changes* log, mee_table* dst, uint64_t slot_begin, uint64_t slot_end,
                        uint64_t* d_counts_out /* device, 4 words */, void* stream);
int mee_group_publish_changed(const mee_group* src, const mee_changes_group* logs, mee_group* dst,
                              uint64_t* d_counts_out /* device, n_tables x 4 words */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MEEPO_EMBEDDING_H */
