// meepo_router.hip — hashing KATs on device, stable shard partition and row (un)permutation for gfx950.
//
// Reference anchor: /root/reference/README.md:2 ("A distributed … Embedding"); no code upstream.  Semantics:
// SPEC.md §1 (hashing) and §5 (sharding).  The partition is a three-kernel counting sort by owner that keeps
// batch order inside each shard segment: per-block histograms (wave ballot + popcount per shard), a per-shard
// scan over blocks (one wave per shard, shuffle prefix-sum), and a scatter that recomputes each key's rank
// from the same ballots.  The run bookkeeping of the sharded embedding bags (bag_runs) is the same sort with
// "first position of a run in segment p" in the place of "key owned by p": both go through count_owners.
// Further down: the run offsets and the combination of the owners' partial bag rows, the cells and the regrouping
// of a sharded table group's jagged batch (segment_counts, regroup), and the peer-to-peer sharded find, whose owner-side kernel probes with the lookups' tile_probe (meepo_device.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>

#include "meepo_device.h"
#include "meepo_host.h"

struct mee_router {
    int device;
    uint64_t max_batch;
    uint32_t n_shards;
    uint32_t max_blocks;
    uint32_t* blockcnt;  // [max_blocks][n_shards] counts, then exclusive offsets inside the shard segment
    uint64_t* base;      // [n_shards] start of each shard segment
    uint64_t* run_base;  // [n_shards] start of each segment's runs (mee_bag_runs: the partition's own `base` stays as the partition left it)
    uint64_t* run_sums;  // [max_blocks * n_shards + 1] per-block sums of received run lengths (mee_run_offsets)
};

struct mee_p2p {
    int device;
    uint32_t n_shards, rank, dim;
    uint64_t cap, max_batch;
    // local symmetric buffers, exported to the peers
    int64_t* inbox_keys;   // [n_shards][cap]
    int32_t* inbox_dst;    // [n_shards][cap]
    uint32_t* inbox_cnt;   // [n_shards] fill counts, followed by [n_shards] barrier flags (flag q = the last epoch rank q announced here)
    float* out;            // [max_batch][dim]
    uint8_t* found;        // [max_batch]
    float* inbox_rows;     // [n_shards][cap][dim] payload rows of pushed (key, row) pairs; null unless created with payload
    uint32_t* status;      // [0] bit 0: a segment overflowed `cap`, bit 1: a barrier timed out; [1] barriers executed so far (the epoch)
    // device-resident pointer tables (index = rank) and their host copies
    void** d_tables;       // kP2PBuffers tables of n_shards pointers each
    void* h_tables[6][64];
    bool connected;
};

namespace mee {

constexpr int kPartBlock = 1024;  // positions per block in the partition and run kernels (one per thread): 4x fewer rows for the scan
constexpr int kMaxShards = 64;
constexpr uint32_t kNoOwner = 0xFFFFFFFFu;   // a position the counting sort leaves out

// inclusive prefix sum over the wave's 64 lanes
template <class T>
__device__ __forceinline__ T wave_scan_inclusive(T v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// The block step of the stable counting sort: thread t holds position blockIdx.x * kPartBlock + t, whose owner is o < g (kNoOwner: none).
// Fills wcnt[w][p] = how many positions of wave w have owner p; with RANK returns how many EARLIER positions of the block have the
// thread's own owner (0 for kNoOwner).  All kPartBlock threads call it (ballots, one barrier).
template <bool RANK>
__device__ __forceinline__ uint32_t count_owners(uint32_t o, uint32_t g, uint32_t (&wcnt)[kPartBlock / 64][kMaxShards]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t r = 0;
    for (uint32_t p = 0; p < g; ++p) {
        const uint64_t m = __ballot(o == p);
        if (RANK && o == p) r = (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (lane == 0) wcnt[w][p] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (RANK && o != kNoOwner)
        for (int ww = 0; ww < w; ++ww) r += wcnt[ww][o];
    return r;
}
// after count_owners: the block's count per owner, one row of blockcnt
__device__ __forceinline__ void store_block_counts(const uint32_t (&wcnt)[kPartBlock / 64][kMaxShards], uint32_t g, uint32_t* blockcnt) {
    if (threadIdx.x < g) {
        uint32_t c = 0;
#pragma unroll
        for (int ww = 0; ww < kPartBlock / 64; ++ww) c += wcnt[ww][threadIdx.x];
        blockcnt[(uint64_t)blockIdx.x * g + threadIdx.x] = c;
    }
}

__global__ void hash_batch_kernel(const int64_t* __restrict__ keys, uint64_t n, uint64_t nb, uint32_t g, uint64_t* mix_out,
                                  uint64_t* bucket_out, uint32_t* owner_out) {
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t k = keys[i];
        if (mix_out) mix_out[i] = mix64((uint64_t)k);
        if (bucket_out) bucket_out[i] = bucket_of(k, nb);
        if (owner_out) owner_out[i] = owner_of(k, g);
    }
}

// SKIP_PAD: EMPTY keys (padding, SPEC.md §2) belong to nobody: not counted, not sent
template <bool SKIP_PAD>
__global__ __launch_bounds__(kPartBlock) void part_count_kernel(const int64_t* __restrict__ keys, uint32_t n, uint32_t g,
                                                                uint32_t* blockcnt) {
    __shared__ uint32_t wcnt[kPartBlock / 64][kMaxShards];
    const uint32_t i = blockIdx.x * kPartBlock + threadIdx.x;
    const int64_t key = i < n ? keys[i] : kEmpty;
    const bool inb = i < n && !(SKIP_PAD && key == kEmpty);
    count_owners<false>(inb ? owner_of(key, g) : kNoOwner, g, wcnt);
    store_block_counts(wcnt, g, blockcnt);
}

// one block; wave w scans shards w, w+nwaves, … over all key blocks
__global__ __launch_bounds__(1024) void part_scan_kernel(uint32_t* blockcnt, uint32_t n_blocks, uint32_t g, uint64_t* base,
                                                         uint64_t* counts_out) {
    __shared__ uint64_t total[kMaxShards];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (uint32_t p = w; p < g; p += nw) {
        uint32_t run = 0;
        for (uint32_t b0 = 0; b0 < n_blocks; b0 += 64) {
            const uint32_t b = b0 + lane;
            const uint32_t c = b < n_blocks ? blockcnt[(uint64_t)b * g + p] : 0;
            const uint32_t incl = wave_scan_inclusive(c, lane);
            if (b < n_blocks) blockcnt[(uint64_t)b * g + p] = run + incl - c;
            run += __shfl(incl, 63);
        }
        if (lane == 0) total[p] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t acc = 0;
        for (uint32_t p = 0; p < g; ++p) {
            base[p] = acc;
            counts_out[p] = total[p];
            acc += total[p];
        }
    }
}

template <bool SKIP_PAD>
__global__ __launch_bounds__(kPartBlock) void part_scatter_kernel(const int64_t* __restrict__ keys, uint32_t n, uint32_t g,
                                                                  const uint32_t* __restrict__ blockoff,
                                                                  const uint64_t* __restrict__ base, int64_t* send_keys,
                                                                  int64_t* perm) {
    __shared__ uint32_t wcnt[kPartBlock / 64][kMaxShards];
    const uint32_t i = blockIdx.x * kPartBlock + threadIdx.x;
    const int64_t key = i < n ? keys[i] : kEmpty;
    const bool inb = i < n && !(SKIP_PAD && key == kEmpty);
    const uint32_t o = inb ? owner_of(key, g) : kNoOwner;
    const uint32_t r = count_owners<true>(o, g, wcnt);
    if (inb) {
        const uint64_t dst = base[o] + blockoff[(uint64_t)blockIdx.x * g + o] + r;
        send_keys[dst] = key;
        perm[dst] = (int64_t)i;
    }
}

// SCATTER: out[perm[q]] = rows[q];  else out[q] = rows[perm[q]].  One element of type T per thread step.
template <typename T, bool SCATTER>
__global__ void permute_rows_kernel(const T* __restrict__ rows, const int64_t* __restrict__ perm, uint64_t n, uint32_t epr,
                                    T* __restrict__ out) {
    const uint64_t total = n * epr;
    for (uint64_t idx = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = idx / epr;
        const uint32_t e = (uint32_t)(idx - q * epr);
        const uint64_t p = (uint64_t)perm[q];
        if (SCATTER) out[p * epr + e] = rows[idx];
        else out[idx] = rows[p * epr + e];
    }
}

template <bool SCATTER>
static int permute_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out, void* stream,
                        const char* name) {
    if (n && (!d_rows || !d_perm || !d_out)) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (n == 0 || row_bytes == 0) return MEE_OK;
    hipStream_t st = (hipStream_t)stream;
    const bool a16 = row_bytes % 16 == 0 && ((uintptr_t)d_rows % 16 == 0) && ((uintptr_t)d_out % 16 == 0);
    const bool a4 = row_bytes % 4 == 0 && ((uintptr_t)d_rows % 4 == 0) && ((uintptr_t)d_out % 4 == 0);
    if (a16) {
        const uint32_t epr = (uint32_t)(row_bytes / 16);
        permute_rows_kernel<float4, SCATTER><<<grid_for(n * epr, 256, 1u << 16), 256, 0, st>>>((const float4*)d_rows, d_perm, n, epr, (float4*)d_out);
    } else if (a4) {
        const uint32_t epr = (uint32_t)(row_bytes / 4);
        permute_rows_kernel<uint32_t, SCATTER><<<grid_for(n * epr, 256, 1u << 16), 256, 0, st>>>((const uint32_t*)d_rows, d_perm, n, epr, (uint32_t*)d_out);
    } else {
        const uint32_t epr = (uint32_t)row_bytes;
        permute_rows_kernel<uint8_t, SCATTER><<<grid_for(n * epr, 256, 1u << 16), 256, 0, st>>>((const uint8_t*)d_rows, d_perm, n, epr, (uint8_t*)d_out);
    }
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// ---- embedding bags over a sharded table (SPEC.md §5 "Pooled lookups") ------------------------------------------------------
// The partition is stable, so inside a destination segment the batch positions ascend and the bags of those positions never decrease: the
// positions of bag b owned by rank p are one contiguous RUN of segment p.  The source lists its runs (bag_runs: the same three-launch
// counting sort as the partition, with "first position of a run in segment p" in the place of "key owned by p"), the owner turns the
// received run lengths into the bag_offsets / grad_index of its local pooled lookup / indexed apply (run_offsets), and the source adds
// the owners' partial rows up in rank order (combine_bag_runs).  Nothing here trusts caller data with an address: perm entries are only
// compared, bags come out of a search over [0, n_bags), run indices are kept inside [0, n_runs).
// the last b in [0, m) with off[b] <= i (m >= 1): the bag of batch position i under bag_offsets, the run of received key i under run offsets
__device__ __forceinline__ uint32_t last_not_above(const uint64_t* __restrict__ off, uint32_t m, uint64_t i) {
    uint32_t lo = 0, hi = m - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct RunPos {
    bool head;        // this position starts a run
    uint32_t seg;     // its destination segment (kNoOwner when it is no run start: the owner id of the counting sort)
    uint32_t bag;
    uint32_t seg_end; // one past the segment's last position
};

// what position q = blockIdx.x * kPartBlock + threadIdx.x is; all threads of the block call it (LDS staging + barriers)
__device__ __forceinline__ RunPos run_position(const int64_t* __restrict__ perm, const uint64_t* __restrict__ counts, uint32_t g, uint32_t n,
                                               const uint64_t* __restrict__ off, uint32_t n_bags, uint32_t* s_end, uint32_t* s_bag) {
    if (threadIdx.x == 0) {   // segment ends, never past n whatever the counts say
        uint64_t acc = 0;
        for (uint32_t p = 0; p < g; ++p) {
            const uint64_t c = counts[p];
            acc += c < n ? c : n;
            acc = acc < n ? acc : n;
            s_end[p] = (uint32_t)acc;
        }
    }
    __syncthreads();
    const uint32_t q = blockIdx.x * kPartBlock + threadIdx.x;
    const bool inb = q < s_end[g - 1];
    uint32_t seg = 0;
    while (seg + 1 < g && s_end[seg] <= q) ++seg;   // g <= 64 LDS words
    const uint32_t seg_begin = seg ? s_end[seg - 1] : 0;
    const uint32_t bag = inb ? last_not_above(off, n_bags, (uint64_t)perm[q]) : 0;
    s_bag[threadIdx.x] = bag;
    __syncthreads();
    uint32_t prev = 0;
    if (inb && q > seg_begin) prev = threadIdx.x ? s_bag[threadIdx.x - 1] : last_not_above(off, n_bags, (uint64_t)perm[q - 1]);
    RunPos r;
    r.head = inb && (q == seg_begin || bag != prev);
    r.seg = r.head ? seg : kNoOwner;
    r.bag = bag;
    r.seg_end = s_end[seg];
    return r;
}

__global__ __launch_bounds__(kPartBlock) void run_count_kernel(const int64_t* __restrict__ perm, const uint64_t* __restrict__ counts, uint32_t g, uint32_t n,
                                                              const uint64_t* __restrict__ off, uint32_t n_bags, uint32_t* blockcnt) {
    __shared__ uint32_t s_end[kMaxShards], s_bag[kPartBlock], wcnt[kPartBlock / 64][kMaxShards];
    const RunPos r = run_position(perm, counts, g, n, off, n_bags, s_end, s_bag);
    count_owners<false>(r.seg, g, wcnt);
    store_block_counts(wcnt, g, blockcnt);
}

__global__ __launch_bounds__(kPartBlock) void run_scatter_kernel(const int64_t* __restrict__ perm, const uint64_t* __restrict__ counts, uint32_t g, uint32_t n,
                                                                const uint64_t* __restrict__ off, uint32_t n_bags, const uint32_t* __restrict__ blockoff,
                                                                const uint64_t* __restrict__ run_base, uint32_t* __restrict__ run_bag,
                                                                uint32_t* __restrict__ run_len) {
    __shared__ uint32_t s_end[kMaxShards], s_bag[kPartBlock], wcnt[kPartBlock / 64][kMaxShards];
    const RunPos r = run_position(perm, counts, g, n, off, n_bags, s_end, s_bag);
    const uint32_t rank = count_owners<true>(r.seg, g, wcnt);
    if (r.head) {
        const uint64_t dst = run_base[r.seg] + blockoff[(uint64_t)blockIdx.x * g + r.seg] + rank;   // < the number of run starts <= n
        const uint32_t q = blockIdx.x * kPartBlock + threadIdx.x;
        // the run ends at the segment's first position of a later bag: positions ascend inside a segment
        const uint64_t bag_end = off[r.bag + 1];
        uint32_t lo = q + 1, hi = r.seg_end;
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)perm[mid] < bag_end) lo = mid + 1; else hi = mid;
        }
        run_bag[dst] = r.bag;
        run_len[dst] = lo - q;
    }
}

// exclusive scan of one value per thread over the block; `total` = the block's sum.  s_w: blockDim.x / 64 words of LDS
__device__ __forceinline__ uint64_t block_scan_exclusive(uint64_t v, uint64_t* s_w, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const uint64_t incl = wave_scan_inclusive(v, lane);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (int ww = 0; ww < nw; ++ww) {
        if (ww < w) before += s_w[ww];
        total += s_w[ww];
    }
    __syncthreads();   // s_w may be written again
    return before + incl - v;
}

__global__ __launch_bounds__(kPartBlock) void run_len_sum_kernel(const uint32_t* __restrict__ run_len, uint64_t n_runs, uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_w[kPartBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPartBlock + threadIdx.x;
    uint64_t total;
    (void)block_scan_exclusive(i < n_runs ? run_len[i] : 0, s_w, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one block: the block sums become their exclusive prefix
__global__ __launch_bounds__(kPartBlock) void run_len_scan_kernel(uint64_t* sums, uint32_t n_blocks) {
    __shared__ uint64_t s_w[kPartBlock / 64];
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kPartBlock) {   // block-uniform
        const uint32_t b = b0 + threadIdx.x;
        uint64_t total;
        const uint64_t ex = block_scan_exclusive(b < n_blocks ? sums[b] : 0, s_w, total);
        if (b < n_blocks) sums[b] = carry + ex;
        carry += total;
    }
}

__global__ __launch_bounds__(kPartBlock) void run_offsets_kernel(const uint32_t* __restrict__ run_len, uint64_t n_runs, const uint64_t* __restrict__ sums,
                                                                uint64_t* __restrict__ offsets) {
    __shared__ uint64_t s_w[kPartBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPartBlock + threadIdx.x;
    const uint64_t len = i < n_runs ? run_len[i] : 0;
    uint64_t total;
    const uint64_t ex = sums[blockIdx.x] + block_scan_exclusive(len, s_w, total);
    if (i < n_runs) offsets[i] = ex;
    if (i + 1 == n_runs) offsets[n_runs] = ex + len;
}

__global__ void run_of_key_kernel(const uint64_t* __restrict__ offsets, uint32_t n_runs, uint64_t n_keys, uint32_t* __restrict__ run_of_key) {
    for (uint64_t k = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; k < n_keys; k += (uint64_t)gridDim.x * blockDim.x)
        run_of_key[k] = last_not_above(offsets, n_runs, k);   // in [0, n_runs) whatever the lengths add up to
}

// out[b] = the partial rows of bag b added up in ascending segment (= owner rank) order: the first one copied, each further one added in fp32 (no
// fma: the file is compiled with -ffp-contract=off), MEAN then divides by (float)length; a bag without a partial is zeros.  One 16-lane tile per
// bag, four bags per wave.  The bag's run in segment p is found by binary search (run_bag ascends inside a segment): lane tl of the tile searches
// segment 16 k + tl, so the searches of 16 segments are in flight together, and their results come back to the whole tile by shuffles in segment
// order.  Rows move as float4, up to four of them in flight per tile; the column groups of a row wider than the instance (run-time dim) are
// independent sums and take one sweep over the found runs each, so no accumulator array is indexed at run time.
template <int DIM4, bool BF16>
__global__ __launch_bounds__(256) void combine_bag_runs_kernel(const float4* __restrict__ partials, const uint32_t* __restrict__ run_bag,
                                                               const uint64_t* __restrict__ run_counts, uint32_t g, uint64_t n_runs,
                                                               const uint64_t* __restrict__ bag_offsets, uint64_t n_bags, uint32_t dim4_rt, int mean,
                                                               void* __restrict__ out) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    // lane l holds the run range of segment l (g <= 64), never past n_runs
    const uint64_t seg_c = (uint32_t)lane < g ? run_counts[lane] : 0;
    const uint64_t seg_incl = wave_scan_inclusive(seg_c < n_runs ? seg_c : n_runs, lane);
    const uint64_t seg_hi = seg_incl < n_runs ? seg_incl : n_runs;
    const uint64_t seg_lo_all = __shfl_up(seg_hi, 1);
    const uint64_t seg_lo = lane ? seg_lo_all : 0;
    for (uint64_t b0 = wave * 4; b0 < n_bags; b0 += n_waves * 4) {   // wave-uniform
        const uint64_t bag = b0 + tile;
        const bool has = bag < n_bags;
        const uint64_t begin = has ? bag_offsets[bag] : 0, end = has ? bag_offsets[bag + 1] : 0;
        const float len = end > begin ? (float)(end - begin) : 0.f;
        // lane tl searches segments tl, 16 + tl, 32 + tl, 48 + tl (g <= 64): where is the bag's run there?
        int64_t mine[kMaxShards / 16];
#pragma unroll
        for (int k = 0; k < kMaxShards / 16; ++k) {
            mine[k] = -1;
            if ((uint32_t)k * 16 >= g) continue;   // wave-uniform
            const uint32_t p = (uint32_t)k * 16 + tl;
            uint64_t lo = __shfl(seg_lo, (int)p), hi = __shfl(seg_hi, (int)p);
            if (p >= g || !has) hi = lo;
            const uint64_t stop = hi;
            while (lo < hi) {
                const uint64_t mid = lo + (hi - lo) / 2;
                if (run_bag[mid] < bag) lo = mid + 1; else hi = mid;
            }
            if (lo < stop && run_bag[lo] == bag) mine[k] = (int64_t)lo;
        }
        for (uint32_t c0 = 0; c0 < dim4; c0 += 16) {   // wave-uniform: one column group of 16 float4 per sweep
            const uint32_t c = c0 + tl;
            const bool col = DIM4 != 0 || c < dim4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            bool first = true;
#pragma unroll
            for (int k = 0; k < kMaxShards / 16; ++k) {
                if ((uint32_t)k * 16 >= g) continue;   // wave-uniform
#pragma unroll
                for (int j0 = 0; j0 < 16; j0 += 4) {
                    int64_t r[4];
                    float4 row[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) r[u] = __shfl(mine[k], tile * 16 + j0 + u);
#pragma unroll
                    for (int u = 0; u < 4; ++u) row[u] = (r[u] >= 0 && col) ? partials[(uint64_t)r[u] * dim4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (r[u] < 0) continue;
                        if (first) acc = row[u];
                        else { acc.x += row[u].x; acc.y += row[u].y; acc.z += row[u].z; acc.w += row[u].w; }
                        first = false;
                    }
                }
            }
            if (has && col) {
                if (mean && !first && len > 0.f) { acc.x = acc.x / len; acc.y = acc.y / len; acc.z = acc.z / len; acc.w = acc.w / len; }
                if constexpr (BF16) store_bf16x4<true>(out, bag * dim4 + c, acc);
                else reinterpret_cast<float4*>(out)[bag * dim4 + c] = acc;
            }
        }
    }
}

// ---- sharded table groups (SPEC.md §5 "Groups"): the cells of a partitioned jagged batch, and the owner's source-major -> table-major regrouping ----
// owner(key, G) does not depend on the table and the partition is stable, so one partition serves a whole jagged batch: inside owner segment p the
// positions ascend, hence the entries of table segment j are one contiguous CELL (p, j) of it, bounded by two binary searches in perm.
// grid: x = owner segment, y = 256 cells of it.  The 257 bounds of a block's cells go through LDS: one search per bound, G (T + 1) in all (+ one per
// further 256 cells).  perm entries are only compared; a segment never reaches past n whatever the counts say.
__global__ __launch_bounds__(256) void segment_counts_kernel(const int64_t* __restrict__ perm, const uint64_t* __restrict__ counts, uint32_t n,
                                                            const uint64_t* __restrict__ offsets, uint32_t n_tables, uint64_t* __restrict__ cells) {
    __shared__ uint32_t s_bound[257];
    const uint32_t p = blockIdx.x, j0 = blockIdx.y * 256;
    uint64_t acc = 0;
    uint32_t seg_begin = 0;
    for (uint32_t pp = 0; pp <= p; ++pp) {   // block-uniform
        seg_begin = (uint32_t)acc;
        const uint64_t c = counts[pp];
        acc += c < n ? c : n;
        acc = acc < n ? acc : n;
    }
    const uint32_t seg_end = (uint32_t)acc;
    for (uint32_t k = threadIdx.x; k < 257; k += 256) {
        const uint32_t j = j0 + k;
        if (j > n_tables) continue;
        const uint64_t bound = offsets[j];
        uint32_t lo = seg_begin, hi = seg_end;   // the first entry of the segment whose position is not below the bound
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if ((uint64_t)perm[mid] < bound) lo = mid + 1; else hi = mid;
        }
        s_bound[k] = lo;
    }
    __syncthreads();
    const uint32_t j = j0 + threadIdx.x;
    if (j < n_tables) {
        const uint32_t b = s_bound[threadIdx.x], e = s_bound[threadIdx.x + 1];
        cells[(uint64_t)p * n_tables + j] = e > b ? e - b : 0;   // (offsets that decrease: an empty cell)
    }
}

// The owner's side.  What arrived is source-major: cell (s, j) = the keys of source rank s for member table j, at cell index s T + j.  The group kernels
// take the batch table-major: cell (s, j) at cell index j G + s.  Every block scans the G T cell lengths twice (source-major and table-major, into LDS:
// two block scans per 512 cells, nothing next to the copy) and then copies its own tile of V x 512 consecutive TABLE-MAJOR positions: a thread finds
// the cell of its first position by binary search in the LDS offsets (empty cells are skipped by the search itself), so consecutive lanes write
// consecutive positions and read consecutive positions of one cell.  V = 2 (all three arrays 16-byte aligned): a thread owns an aligned pair of
// positions, stores keys and order as 16 bytes each and loads the keys as 16 bytes when the pair lies in one cell at an even source position.
// Cell lengths are caller data: every offset is kept inside [0, n_recv] and a source position is only used below n_recv; positions past the cells' sum
// are left alone.  No atomics, no workspace: the launch only reads the cells and the keys.
constexpr int kRegroupMaxCells = 8128;   // 2 x (cells + 1) 32-bit offsets in LDS
constexpr int kRegroupBlock = 512;       // threads per block: a tile of V x 512 positions per scan of the cells

__device__ __forceinline__ uint32_t lds_last_not_above(const uint32_t* off, uint32_t m, uint32_t q) {   // the last c in [0, m) with off[c] <= q (off[0] = 0)
    uint32_t lo = 0, hi = m - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= q) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int V>
__global__ __launch_bounds__(kRegroupBlock) void regroup_kernel(const int64_t* __restrict__ recv_keys, const uint64_t* __restrict__ recv_cells, uint32_t n_recv,
                                                             uint32_t g, uint32_t n_tables, int64_t* __restrict__ keys_out, int64_t* __restrict__ order_out,
                                                             uint64_t* __restrict__ offsets_out) {
    extern __shared__ uint32_t s_off[];   // [cells + 1] table-major offsets (by j G + s), then [cells + 1] source-major offsets (by s T + j)
    __shared__ uint64_t s_w[kRegroupBlock / 64];
    const uint32_t n_cells = g * n_tables;
    uint32_t* dst_off = s_off;
    uint32_t* src_off = s_off + n_cells + 1;
    uint64_t carry_d = 0, carry_s = 0;
    for (uint32_t c0 = 0; c0 < n_cells; c0 += kRegroupBlock) {   // block-uniform
        const uint32_t c = c0 + threadIdx.x;
        uint64_t len_d = 0, len_s = 0;
        if (c < n_cells) {
            const uint32_t j = c / g, s = c - j * g;
            len_d = recv_cells[(uint64_t)s * n_tables + j];
            len_s = recv_cells[c];
            len_d = len_d < n_recv ? len_d : n_recv;
            len_s = len_s < n_recv ? len_s : n_recv;
        }
        uint64_t total_d, total_s;
        const uint64_t ex_d = carry_d + block_scan_exclusive(len_d, s_w, total_d);
        const uint64_t ex_s = carry_s + block_scan_exclusive(len_s, s_w, total_s);
        if (c < n_cells) {
            dst_off[c] = (uint32_t)(ex_d < n_recv ? ex_d : n_recv);
            src_off[c] = (uint32_t)(ex_s < n_recv ? ex_s : n_recv);
        }
        carry_d += total_d;
        carry_s += total_s;
        carry_d = carry_d < n_recv ? carry_d : n_recv;
        carry_s = carry_s < n_recv ? carry_s : n_recv;
    }
    if (threadIdx.x == 0) {
        dst_off[n_cells] = (uint32_t)carry_d;
        src_off[n_cells] = (uint32_t)carry_s;
    }
    __syncthreads();
    const uint32_t total = dst_off[n_cells];
    if (blockIdx.x == 0)
        for (uint32_t j = threadIdx.x; j <= n_tables; j += kRegroupBlock) offsets_out[j] = dst_off[j * g];   // (j = T: the cells' sum)

    const uint32_t q0 = (blockIdx.x * kRegroupBlock + threadIdx.x) * V;
    if (q0 >= total) return;
    const uint32_t c = lds_last_not_above(dst_off, n_cells, q0);   // table-major cell j G + s
    const uint32_t j = c / g, s = c - j * g;
    const uint64_t src = (uint64_t)src_off[s * n_tables + j] + (q0 - dst_off[c]);
    if constexpr (V == 1) {
        if (src < n_recv) {
            keys_out[q0] = recv_keys[src];
            order_out[q0] = (int64_t)src;
        }
    } else {
        const bool two = q0 + 1 < total;
        uint64_t src1 = src + 1;
        if (two && q0 + 1 >= dst_off[c + 1]) {   // the pair straddles a cell boundary (and any empty cells behind it)
            const uint32_t c1 = lds_last_not_above(dst_off, n_cells, q0 + 1);
            const uint32_t j1 = c1 / g, s1 = c1 - j1 * g;
            src1 = (uint64_t)src_off[s1 * n_tables + j1] + (q0 + 1 - dst_off[c1]);
        }
        const bool ok0 = src < n_recv, ok1 = two && src1 < n_recv;
        longlong2 k = make_longlong2(kEmpty, kEmpty);
        if (ok0 && ok1 && src1 == src + 1 && (src & 1) == 0) k = *reinterpret_cast<const longlong2*>(recv_keys + src);
        else {
            if (ok0) k.x = recv_keys[src];
            if (ok1) k.y = recv_keys[src1];
        }
        if (ok0 && ok1) {
            *reinterpret_cast<longlong2*>(keys_out + q0) = k;
            *reinterpret_cast<longlong2*>(order_out + q0) = make_longlong2((long long)src, (long long)src1);
        } else {
            if (ok0) { keys_out[q0] = k.x; order_out[q0] = (int64_t)src; }
            if (ok1) { keys_out[q0 + 1] = k.y; order_out[q0 + 1] = (int64_t)src1; }
        }
    }
}

// ---- peer-to-peer sharded find (SPEC.md §5 without the all-to-alls) ---------------------------------------------
// Every rank owns five "symmetric" buffers that its peers map through HIP IPC: an inbox of keys and of destination
// indices with one segment per source rank, the segment fill counts, and its result rows / found bytes.  A lookup is
//   push:  each rank's partitioned keys (+ their batch positions) are stored straight into the owners' inboxes (xGMI)
//   find:  each owner probes what arrived and stores every row straight into the requester's result buffer (xGMI)
// with one stream-ordered barrier after each phase.  No all-to-all, no un-permute pass, no host sync.
constexpr int kP2PBuffers = 6;  // inbox keys, inbox dst, inbox counts, result rows, result found bytes, inbox payload rows
struct P2PPeers {            // device-resident pointer tables, index = rank
    int64_t** keys; int32_t** dst; uint32_t** cnt; float** out; uint8_t** found; float** rows;
};

// grid: x over positions inside a segment, y = destination rank
__global__ __launch_bounds__(256) void p2p_push_kernel(const int64_t* __restrict__ send_keys, const int64_t* __restrict__ perm,
                                                       const uint64_t* __restrict__ counts, const uint64_t* __restrict__ base,
                                                       P2PPeers peers, uint32_t me, uint64_t cap, uint32_t* status, int pad) {
    const uint32_t p = blockIdx.y;
    const uint64_t cnt = counts[p];
    const uint64_t take = cnt < cap ? cnt : cap;
    int64_t* __restrict__ dk = peers.keys[p] + (uint64_t)me * cap;
    int32_t* __restrict__ dd = peers.dst[p] + (uint64_t)me * cap;
    const uint64_t b0 = base[p];
    for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < take; j += (uint64_t)gridDim.x * blockDim.x) {
        dk[j] = send_keys[b0 + j];
        dd[j] = (int32_t)perm[b0 + j];
    }
    if (pad)  // the owner will hand the whole fixed-size inbox to an operator: unused positions become padding keys
        for (uint64_t j = take + blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < cap; j += (uint64_t)gridDim.x * blockDim.x) dk[j] = kEmpty;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        peers.cnt[p][me] = (uint32_t)take;
        if (cnt > cap) atomicOr(status, 1u);
    }
}

// Cross-rank barrier over the peer-mapped flag words: every rank announces epoch e in the flag word it owns on every peer
// (system-scope release store: the rank's earlier kernels — whose stores into peer memory were made visible by their kernel
// end — are ordered before it), then waits until all peers have announced e here.  One wave; the wait is bounded (wall clock)
// so the grid always drains: on time-out bit 1 of the status word is set and the caller must not trust the step.
__global__ __launch_bounds__(64) void p2p_barrier_kernel(P2PPeers peers, uint32_t me, uint32_t n_shards, uint32_t* status,
                                                         unsigned long long timeout_ticks) {
    const uint32_t q = threadIdx.x;
    // the epoch lives in device memory and is advanced by the kernel itself (every rank runs the same number of barriers),
    // so a captured launch stays correct when it is replayed
    uint32_t epoch = 0;
    if (q == 0) { epoch = status[1] + 1; status[1] = epoch; }
    epoch = __shfl(epoch, 0);
    if (q < n_shards) {
        uint32_t* theirs = peers.cnt[q] + n_shards + me;   // my flag word at rank q
        __hip_atomic_store(theirs, epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t* mine = peers.cnt[me] + n_shards + q;   // rank q's flag word here
        const unsigned long long t0 = wall_clock64();
        while ((int32_t)(__hip_atomic_load(mine, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0) {
            if (wall_clock64() - t0 > timeout_ticks) { atomicOr(status, 2u); break; }
            __builtin_amdgcn_s_sleep(8);
        }
    }
}

// payload rows of a push: one 16-lane tile copies row perm[b0+j] of the batch into position j of the owner's segment
__global__ __launch_bounds__(256) void p2p_push_rows_kernel(const float4* __restrict__ rows, const int64_t* __restrict__ perm,
                                                            const uint64_t* __restrict__ counts, const uint64_t* __restrict__ base,
                                                            P2PPeers peers, uint32_t me, uint64_t cap, uint32_t dim4) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint32_t p = blockIdx.y;
    const uint64_t cnt = counts[p];
    const uint64_t take = cnt < cap ? cnt : cap;
    float4* __restrict__ dr = reinterpret_cast<float4*>(peers.rows[p]) + (uint64_t)me * cap * dim4;
    const uint64_t b0 = base[p];
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t j0 = wave * 4; j0 < take; j0 += n_waves * 4) {
        const uint64_t j = j0 + tile;
        if (j >= take) continue;
        const uint64_t src = (uint64_t)perm[b0 + j] * dim4;
        for (uint32_t c = tl; c < dim4; c += 16) dr[j * dim4 + c] = rows[src + c];
    }
}

// grid: x over the positions of one inbox segment, y = source rank.  Same shape as find_kernel: R keys in flight per
// 16-lane tile (bucket lines requested back to back, then the rows); DIM4 = dim/4 when 16 or 32, else 0 (run-time dim).
// Rows and found bytes are stored into the requester's buffers — peer memory, i.e. xGMI stores, for remote sources.
template <int DIM4, int R>
__global__ __launch_bounds__(256) void p2p_find_kernel(const int64_t* __restrict__ tkeys, const float4* __restrict__ values, uint64_t nb,
                                                       uint32_t dim4_rt, float defv, const int64_t* __restrict__ in_keys,
                                                       const int32_t* __restrict__ in_dst, const uint32_t* __restrict__ in_cnt,
                                                       P2PPeers peers, uint64_t cap) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint32_t s = blockIdx.y;
    const uint32_t cnt = in_cnt[s];
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
    const int64_t* __restrict__ seg_keys = in_keys + (uint64_t)s * cap;
    const int32_t* __restrict__ seg_dst = in_dst + (uint64_t)s * cap;
    float4* __restrict__ outp = reinterpret_cast<float4*>(peers.out[s]);
    uint8_t* __restrict__ fnd = peers.found[s];
    const uint32_t dim4 = DIM4 ? DIM4 : dim4_rt;
    const float4 def4 = make_float4(defv, defv, defv, defv);
    for (uint32_t base = wave * 4 * R; base < cnt; base += n_waves * 4 * R) {  // wave-uniform
        int64_t key[R], slot[R];
        int32_t dst[R];
        bool inb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint32_t i = base + r * 4 + tile;
            inb[r] = i < cnt;
            key[r] = inb[r] ? seg_keys[i] : kEmpty;
            dst[r] = inb[r] ? seg_dst[i] : 0;
        }
        uint64_t b[R];
        int64_t kb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            b[r] = bucket_of(key[r], nb);
            kb[r] = (inb[r] && !reserved_key(key[r])) ? tkeys[b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys, nb, key[r], inb[r] && !reserved_key(key[r]), b[r], kb[r], tile, tl);
        if constexpr (DIM4 != 0) {
            constexpr int C = DIM4 / 16;
            float4 row[R][C];
#pragma unroll
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int c = 0; c < C; ++c) row[r][c] = slot[r] >= 0 ? values[(uint64_t)slot[r] * DIM4 + c * 16 + tl] : def4;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (inb[r]) {
#pragma unroll
                    for (int c = 0; c < C; ++c) outp[(uint64_t)dst[r] * DIM4 + c * 16 + tl] = row[r][c];
                }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (inb[r])
                    for (uint32_t c = tl; c < dim4; c += 16)
                        outp[(uint64_t)dst[r] * dim4 + c] = slot[r] >= 0 ? values[(uint64_t)slot[r] * dim4 + c] : def4;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (inb[r] && tl == 0) fnd[dst[r]] = slot[r] >= 0;
    }
}

}  // namespace mee

using namespace mee;

extern "C" {

int mee_hash_batch(const int64_t* d_keys, size_t n, uint64_t n_buckets, uint32_t n_shards, uint64_t* d_mix_out,
                   uint64_t* d_bucket_out, uint32_t* d_owner_out, void* stream) {
    MEE_RANGE("mee_hash_batch");
    if (n && !d_keys) return fail(MEE_ERR_INVALID_ARG, "mee_hash_batch: null keys");
    if (n == 0) return MEE_OK;
    hash_batch_kernel<<<grid_for(n, 256, 1u << 14), 256, 0, (hipStream_t)stream>>>(d_keys, n, n_buckets, n_shards, d_mix_out,
                                                                                 d_bucket_out, d_owner_out);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_router_destroy(mee_router* r) {
    MEE_RANGE("mee_router_destroy");
    if (!r) return MEE_OK;
    DeviceGuard g(r->device);
    if (r->blockcnt) (void)hipFree(r->blockcnt);
    if (r->base) (void)hipFree(r->base);
    if (r->run_base) (void)hipFree(r->run_base);
    if (r->run_sums) (void)hipFree(r->run_sums);
    delete r;
    return MEE_OK;
}

int mee_router_create(int32_t device, uint64_t max_batch, uint32_t n_shards, mee_router** out) {
    MEE_RANGE("mee_router_create");
    if (!out) return fail(MEE_ERR_INVALID_ARG, "mee_router_create: null out");
    *out = nullptr;
    if (n_shards == 0 || n_shards > (uint32_t)kMaxShards || max_batch == 0 || max_batch > (1ull << 30))
        return fail(MEE_ERR_INVALID_ARG, "mee_router_create: n_shards must be 1..%d and max_batch 1..2^30", kMaxShards);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MEE_ERR_NO_DEVICE, "mee_router_create: no HIP device visible (this backend has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MEE_ERR_INVALID_ARG, "mee_router_create: device %d out of range", device);
    DeviceGuard g(device);
    mee_router* r = new (std::nothrow) mee_router();
    if (!r) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    r->device = device; r->max_batch = max_batch; r->n_shards = n_shards;
    r->max_blocks = (uint32_t)((max_batch + kPartBlock - 1) / kPartBlock);
    r->blockcnt = nullptr; r->base = nullptr; r->run_base = nullptr; r->run_sums = nullptr;
    if (hipMalloc((void**)&r->blockcnt, (size_t)r->max_blocks * n_shards * 4) != hipSuccess ||
        hipMalloc((void**)&r->base, n_shards * 8) != hipSuccess || hipMalloc((void**)&r->run_base, n_shards * 8) != hipSuccess ||
        hipMalloc((void**)&r->run_sums, ((size_t)r->max_blocks * n_shards + 1) * 8) != hipSuccess) {
        mee_router_destroy(r);
        return fail(MEE_ERR_OUT_OF_MEMORY, "mee_router_create: hipMalloc failed");
    }
    *out = r;
    return MEE_OK;
}

static int partition_common(mee_router* r, const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts, int64_t* d_perm,
                            void* stream, bool skip_pad, const char* name) {
    if (!r || !d_counts || (n && (!d_keys || !d_send_keys || !d_perm))) return fail(MEE_ERR_INVALID_ARG, "%s: null argument", name);
    if (n > r->max_batch) return fail(MEE_ERR_BATCH_TOO_LARGE, "%s: n=%zu exceeds max_batch=%llu", name, n, (unsigned long long)r->max_batch);
    DeviceGuard g(r->device);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nblk = (uint32_t)((n + kPartBlock - 1) / kPartBlock);
    if (nblk) with_flag(skip_pad, [&](auto sp) { part_count_kernel<sp><<<nblk, kPartBlock, 0, st>>>(d_keys, (uint32_t)n, r->n_shards, r->blockcnt); });
    part_scan_kernel<<<1, 1024, 0, st>>>(r->blockcnt, nblk, r->n_shards, r->base, d_counts);
    if (nblk) with_flag(skip_pad, [&](auto sp) { part_scatter_kernel<sp><<<nblk, kPartBlock, 0, st>>>(d_keys, (uint32_t)n, r->n_shards, r->blockcnt, r->base, d_send_keys, d_perm); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}
int mee_partition(mee_router* r, const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts, int64_t* d_perm,
                  void* stream) {
    MEE_RANGE("mee_partition");
    return partition_common(r, d_keys, n, d_send_keys, d_counts, d_perm, stream, false, "mee_partition");
}
int mee_partition_padded(mee_router* r, const int64_t* d_keys, size_t n, int64_t* d_send_keys, uint64_t* d_counts, int64_t* d_perm,
                         void* stream) {
    MEE_RANGE("mee_partition_padded");
    return partition_common(r, d_keys, n, d_send_keys, d_counts, d_perm, stream, true, "mee_partition_padded");
}

// ---- embedding bags over a sharded table: run bookkeeping and the combination of the owners' partial rows -------------------
int mee_bag_runs(mee_router* r, const int64_t* d_perm, const uint64_t* d_counts, size_t n, const uint64_t* d_bag_offsets, size_t n_bags,
                 uint32_t* d_run_bag, uint32_t* d_run_len, uint64_t* d_run_counts, void* stream) {
    MEE_RANGE("mee_bag_runs");
    if (!r || !d_counts || !d_bag_offsets || !d_run_counts || (n && (!d_perm || !d_run_bag || !d_run_len)))
        return fail(MEE_ERR_INVALID_ARG, "mee_bag_runs: null argument");
    if (n > r->max_batch) return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_bag_runs: n=%zu exceeds max_batch=%llu", n, (unsigned long long)r->max_batch);
    if (n_bags > 0xFFFFFFFFull || (n && n_bags == 0)) return fail(MEE_ERR_INVALID_ARG, "mee_bag_runs: n_bags must be in [1, 2^32) when there are positions (the bags partition them)");
    DeviceGuard g(r->device);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nblk = (uint32_t)((n + kPartBlock - 1) / kPartBlock);
    if (nblk) run_count_kernel<<<nblk, kPartBlock, 0, st>>>(d_perm, d_counts, r->n_shards, (uint32_t)n, d_bag_offsets, (uint32_t)n_bags, r->blockcnt);
    part_scan_kernel<<<1, 1024, 0, st>>>(r->blockcnt, nblk, r->n_shards, r->run_base, d_run_counts);
    if (nblk) run_scatter_kernel<<<nblk, kPartBlock, 0, st>>>(d_perm, d_counts, r->n_shards, (uint32_t)n, d_bag_offsets, (uint32_t)n_bags, r->blockcnt, r->run_base, d_run_bag, d_run_len);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_run_offsets(mee_router* r, const uint32_t* d_run_len, size_t n_runs, uint64_t* d_offsets, uint32_t* d_run_of_key, size_t n_keys, void* stream) {
    MEE_RANGE("mee_run_offsets");
    if (!r || !d_offsets || (n_runs && !d_run_len)) return fail(MEE_ERR_INVALID_ARG, "mee_run_offsets: null argument");
    if (n_runs > (size_t)r->max_batch * r->n_shards)
        return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_run_offsets: n_runs=%zu exceeds n_shards x max_batch=%llu", n_runs, (unsigned long long)(r->max_batch * r->n_shards));
    if (n_runs > 0xFFFFFFFFull) return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_run_offsets: n_runs=%zu does not fit the 32-bit run index", n_runs);
    if (d_run_of_key && n_keys && n_runs == 0) return fail(MEE_ERR_INVALID_ARG, "mee_run_offsets: %zu keys but no run", n_keys);
    DeviceGuard g(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (n_runs == 0) {
        MEE_HIP(hipMemsetAsync(d_offsets, 0, 8, st));
        return MEE_OK;
    }
    const uint32_t nblk = (uint32_t)((n_runs + kPartBlock - 1) / kPartBlock);   // <= max_blocks * n_shards
    run_len_sum_kernel<<<nblk, kPartBlock, 0, st>>>(d_run_len, n_runs, r->run_sums);
    run_len_scan_kernel<<<1, kPartBlock, 0, st>>>(r->run_sums, nblk);
    run_offsets_kernel<<<nblk, kPartBlock, 0, st>>>(d_run_len, n_runs, r->run_sums, d_offsets);
    if (d_run_of_key && n_keys) run_of_key_kernel<<<grid_for(n_keys, 256, 1u << 16), 256, 0, st>>>(d_offsets, (uint32_t)n_runs, n_keys, d_run_of_key);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_combine_bag_runs(mee_router* r, const float* d_partials, const uint32_t* d_run_bag, const uint64_t* d_run_counts, size_t n_runs,
                         const uint64_t* d_bag_offsets, size_t n_bags, uint32_t dim, int mode, void* d_out, uint32_t out_dtype, void* stream) {
    MEE_RANGE("mee_combine_bag_runs");
    if (!r || !d_run_counts || (n_bags && (!d_bag_offsets || !d_out)) || (n_runs && (!d_partials || !d_run_bag)))
        return fail(MEE_ERR_INVALID_ARG, "mee_combine_bag_runs: null argument");
    if (int rc = check_out_dtype(d_out, out_dtype, "mee_combine_bag_runs")) return rc;
    if (mode != MEE_POOL_SUM && mode != MEE_POOL_MEAN) return fail(MEE_ERR_INVALID_ARG, "mee_combine_bag_runs: mode must be MEE_POOL_SUM or MEE_POOL_MEAN");
    if (dim < 4 || (dim & 3) || ((uintptr_t)d_partials & 15) || (out_dtype == MEE_DTYPE_F32 && ((uintptr_t)d_out & 15)))
        return fail(MEE_ERR_INVALID_ARG, "mee_combine_bag_runs: dim must be a positive multiple of 4 and fp32 rows 16-byte aligned");
    if (n_runs > 0xFFFFFFFFull) return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_combine_bag_runs: n_runs=%zu", n_runs);
    if (n_bags == 0) return MEE_OK;
    DeviceGuard g(r->device);
    hipStream_t st = (hipStream_t)stream;
    with_row_shape(dim / 4, [&](auto d4) { with_flag(out_dtype == MEE_DTYPE_BF16, [&](auto bf16) {
        combine_bag_runs_kernel<d4, bf16><<<grid_for(n_bags, 16, 1u << 20), 256, 0, st>>>((const float4*)d_partials, d_run_bag, d_run_counts, r->n_shards, n_runs,
                                                                                         d_bag_offsets, n_bags, dim / 4, mode == MEE_POOL_MEAN, d_out);
    }); });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// ---- sharded table groups: the (owner, table) cells of a partitioned jagged batch, and the owner's regrouping -----------------------------------
int mee_segment_counts(mee_router* r, const int64_t* d_perm, const uint64_t* d_counts, size_t n, const uint64_t* d_offsets, size_t n_tables,
                       uint64_t* d_cell_counts, void* stream) {
    MEE_RANGE("mee_segment_counts");
    if (!r || !d_counts || !d_offsets || !d_cell_counts || (n && !d_perm)) return fail(MEE_ERR_INVALID_ARG, "mee_segment_counts: null argument");
    if (n > r->max_batch) return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_segment_counts: n=%zu exceeds max_batch=%llu", n, (unsigned long long)r->max_batch);
    if (n_tables == 0 || n_tables > kMaxGroupTables) return fail(MEE_ERR_INVALID_ARG, "mee_segment_counts: n_tables must be in [1, %u]", kMaxGroupTables);
    DeviceGuard g(r->device);
    const dim3 grid(r->n_shards, (unsigned)((n_tables + 255) / 256));
    segment_counts_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d_perm, d_counts, (uint32_t)n, d_offsets, (uint32_t)n_tables, d_cell_counts);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_regroup(mee_router* r, const int64_t* d_recv_keys, const uint64_t* d_recv_cells, size_t n_recv, size_t n_tables, int64_t* d_keys_out,
                int64_t* d_order_out, uint64_t* d_offsets_out, void* stream) {
    MEE_RANGE("mee_regroup");
    if (!r || !d_recv_cells || !d_offsets_out || (n_recv && (!d_recv_keys || !d_keys_out || !d_order_out))) return fail(MEE_ERR_INVALID_ARG, "mee_regroup: null argument");
    if (n_recv > (size_t)r->max_batch * r->n_shards)
        return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_regroup: n_recv=%zu exceeds n_shards x max_batch=%llu", n_recv, (unsigned long long)(r->max_batch * r->n_shards));
    if (n_recv > 0xFFFFFFFFull - 2 * kPartBlock) return fail(MEE_ERR_BATCH_TOO_LARGE, "mee_regroup: n_recv=%zu does not fit the 32-bit position", n_recv);
    if (n_tables == 0 || n_tables > kMaxGroupTables || n_tables * r->n_shards > (size_t)kRegroupMaxCells)
        return fail(MEE_ERR_INVALID_ARG, "mee_regroup: n_tables must be in [1, %u] and n_shards x n_tables <= %d (the cell offsets live in LDS)", kMaxGroupTables, kRegroupMaxCells);
    DeviceGuard g(r->device);
    const size_t lds = 2 * (n_tables * r->n_shards + 1) * sizeof(uint32_t);
    const bool a16 = (((uintptr_t)d_recv_keys | (uintptr_t)d_keys_out | (uintptr_t)d_order_out) & 15) == 0;
    with_flag(a16, [&](auto wide) {
        constexpr int V = decltype(wide)::value ? 2 : 1;
        regroup_kernel<V><<<grid_for(n_recv, kRegroupBlock * V, 1u << 23), kRegroupBlock, lds, (hipStream_t)stream>>>(
            d_recv_keys, d_recv_cells, (uint32_t)n_recv, r->n_shards, (uint32_t)n_tables, d_keys_out, d_order_out, d_offsets_out);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// ---- peer-to-peer exchange: lifetime and IPC ----------------------------------------------------------------------
int mee_p2p_destroy(mee_p2p* c) {
    MEE_RANGE("mee_p2p_destroy");
    if (!c) return MEE_OK;
    DeviceGuard g(c->device);
    (void)hipDeviceSynchronize();
    if (c->connected)
        for (int b = 0; b < kP2PBuffers; ++b)
            for (uint32_t p = 0; p < c->n_shards; ++p)
                if (p != c->rank && c->h_tables[b][p]) (void)hipIpcCloseMemHandle(c->h_tables[b][p]);
    void* mine[] = {c->inbox_keys, c->inbox_dst, c->inbox_cnt, c->out, c->found, c->inbox_rows, c->status, c->d_tables};
    for (void* p : mine) if (p) (void)hipFree(p);
    delete c;
    return MEE_OK;
}

int mee_p2p_create(int32_t device, uint32_t n_shards, uint32_t rank, uint64_t slots_per_peer, uint64_t max_batch, uint32_t dim,
                   int with_payload, mee_p2p** out) {
    MEE_RANGE("mee_p2p_create");
    if (!out) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_create: null out");
    *out = nullptr;
    if (n_shards == 0 || n_shards > (uint32_t)kMaxShards || rank >= n_shards || slots_per_peer == 0 || max_batch == 0 ||
        max_batch > (1ull << 30) || dim < 4 || (dim & 3))
        return fail(MEE_ERR_INVALID_ARG, "mee_p2p_create: bad arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(MEE_ERR_NO_DEVICE, "mee_p2p_create: no HIP device visible");
    if (device < 0 || device >= ndev) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_create: device %d out of range", device);
    DeviceGuard g(device);
    mee_p2p* c = new (std::nothrow) mee_p2p();
    if (!c) return fail(MEE_ERR_OUT_OF_MEMORY, "host allocation failed");
    memset(c, 0, sizeof *c);
    c->device = device; c->n_shards = n_shards; c->rank = rank; c->dim = dim; c->cap = slots_per_peer; c->max_batch = max_batch;
    const uint64_t slots = (uint64_t)n_shards * slots_per_peer;
    // The five peer-visible buffers are FINE-GRAINED device memory: peers store into them from inside kernels and the
    // owner reads them in its next kernel with nothing but a collective in between, so they must stay coherent across
    // GPUs without relying on a system-scope cache invalidate at the reader's kernel start (coarse-grained hipMalloc
    // memory is only guaranteed coherent at host-visible synchronisation points).  Set MEE_P2P_COARSE=1 to use plain
    // hipMalloc instead (single-GPU rehearsals).
    const bool fine = getenv("MEE_P2P_COARSE") == nullptr;
    auto sym_alloc = [&](void** p, size_t bytes) {
        return fine ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocFinegrained) : hipMalloc(p, bytes);
    };
    if (sym_alloc((void**)&c->inbox_keys, slots * 8) != hipSuccess || sym_alloc((void**)&c->inbox_dst, slots * 4) != hipSuccess ||
        sym_alloc((void**)&c->inbox_cnt, 2 * n_shards * 4) != hipSuccess || sym_alloc((void**)&c->out, (max_batch + 1) * (uint64_t)dim * 4) != hipSuccess ||   // + one spare row: see mee_p2p_buffers
        sym_alloc((void**)&c->found, max_batch + 1) != hipSuccess ||
        (with_payload && sym_alloc((void**)&c->inbox_rows, slots * (uint64_t)dim * 4) != hipSuccess) ||
        hipMalloc((void**)&c->status, 8) != hipSuccess ||
        hipMalloc((void**)&c->d_tables, kP2PBuffers * (size_t)n_shards * sizeof(void*)) != hipSuccess) {
        mee_p2p_destroy(c);
        return fail(MEE_ERR_OUT_OF_MEMORY, "mee_p2p_create: device allocation failed (%s)", fine ? "fine-grained" : "coarse-grained");
    }
    if (hipMemset(c->inbox_cnt, 0, 2 * n_shards * 4) != hipSuccess || hipMemset(c->status, 0, 8) != hipSuccess) {
        mee_p2p_destroy(c);
        return fail(MEE_ERR_HIP, "mee_p2p_create: hipMemset failed");
    }
    *out = c;
    return MEE_OK;
}

static void* p2p_local(const mee_p2p* c, int b) {
    switch (b) { case 0: return c->inbox_keys; case 1: return c->inbox_dst; case 2: return c->inbox_cnt; case 3: return c->out; case 4: return c->found; default: return c->inbox_rows; }
}

int mee_p2p_export(mee_p2p* c, void* handles) {
    MEE_RANGE("mee_p2p_export");
    if (!c || !handles) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_export: null argument");
    static_assert(sizeof(hipIpcMemHandle_t) == MEE_IPC_HANDLE_BYTES, "IPC handle size");
    DeviceGuard g(c->device);
    memset(handles, 0, (size_t)kP2PBuffers * MEE_IPC_HANDLE_BYTES);
    for (int b = 0; b < kP2PBuffers; ++b) {
        if (!p2p_local(c, b)) continue;  // no payload inbox
        hipIpcMemHandle_t h;
        MEE_HIP(hipIpcGetMemHandle(&h, p2p_local(c, b)));
        memcpy((char*)handles + b * MEE_IPC_HANDLE_BYTES, &h, MEE_IPC_HANDLE_BYTES);
    }
    return MEE_OK;
}

int mee_p2p_connect(mee_p2p* c, const void* all_handles) {
    MEE_RANGE("mee_p2p_connect");
    if (!c || !all_handles) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_connect: null argument");
    if (c->connected) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_connect: already connected");
    DeviceGuard g(c->device);
    for (uint32_t p = 0; p < c->n_shards; ++p)
        for (int b = 0; b < kP2PBuffers; ++b) {
            if (p == c->rank || !p2p_local(c, b)) { c->h_tables[b][p] = p2p_local(c, b); continue; }
            hipIpcMemHandle_t h;
            memcpy(&h, (const char*)all_handles + ((size_t)p * kP2PBuffers + b) * MEE_IPC_HANDLE_BYTES, MEE_IPC_HANDLE_BYTES);
            void* ptr = nullptr;
            MEE_HIP(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
            c->h_tables[b][p] = ptr;
        }
    for (int b = 0; b < kP2PBuffers; ++b)
        MEE_HIP(hipMemcpy(c->d_tables + (size_t)b * c->n_shards, c->h_tables[b], c->n_shards * sizeof(void*), hipMemcpyHostToDevice));
    c->connected = true;
    return MEE_OK;
}

int mee_p2p_buffers(mee_p2p* c, float** d_out, uint8_t** d_found) {
    if (!c) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_buffers: null argument");
    if (d_out) *d_out = c->out;
    if (d_found) *d_found = c->found;
    return MEE_OK;
}

static P2PPeers p2p_peers(const mee_p2p* c) {
    P2PPeers pp;
    pp.keys = (int64_t**)(c->d_tables + 0 * (size_t)c->n_shards);
    pp.dst = (int32_t**)(c->d_tables + 1 * (size_t)c->n_shards);
    pp.cnt = (uint32_t**)(c->d_tables + 2 * (size_t)c->n_shards);
    pp.out = (float**)(c->d_tables + 3 * (size_t)c->n_shards);
    pp.found = (uint8_t**)(c->d_tables + 4 * (size_t)c->n_shards);
    pp.rows = (float**)(c->d_tables + 5 * (size_t)c->n_shards);
    return pp;
}

int mee_p2p_push(mee_p2p* c, mee_router* r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts, size_t n,
                 void* stream) {
    MEE_RANGE("mee_p2p_push");
    if (!c || !r || !d_counts || (n && (!d_send_keys || !d_perm))) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push: null argument");
    if (!c->connected) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push: not connected");
    if (r->n_shards != c->n_shards || n > c->max_batch) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push: router/batch mismatch");
    DeviceGuard g(c->device);
    const dim3 grid(grid_for(n / c->n_shards + 256, 256, 1024), c->n_shards);
    p2p_push_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(d_send_keys, d_perm, d_counts, r->base, p2p_peers(c), c->rank, c->cap, c->status, 0);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_p2p_push_rows(mee_p2p* c, mee_router* r, const int64_t* d_send_keys, const int64_t* d_perm, const uint64_t* d_counts,
                      const float* d_rows, size_t n, void* stream) {
    MEE_RANGE("mee_p2p_push_rows");
    if (!c || !r || !d_counts || (n && (!d_send_keys || !d_perm))) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push_rows: null argument");
    if (!c->connected || !c->inbox_rows) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push_rows: context not connected or created without payload");
    if (r->n_shards != c->n_shards || n > c->max_batch) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_push_rows: router/batch mismatch");
    DeviceGuard g(c->device);
    hipStream_t st = (hipStream_t)stream;
    const dim3 gk(grid_for(c->cap, 256, 1024), c->n_shards);
    p2p_push_kernel<<<gk, 256, 0, st>>>(d_send_keys, d_perm, d_counts, r->base, p2p_peers(c), c->rank, c->cap, c->status, 1);
    if (d_rows) {  // null: keys only, padded (an owner-side find_or_insert over the whole inbox)
        const dim3 gr(grid_for(n / c->n_shards + 64, 16, 4096), c->n_shards);
        p2p_push_rows_kernel<<<gr, 256, 0, st>>>((const float4*)d_rows, d_perm, d_counts, r->base, p2p_peers(c), c->rank, c->cap, c->dim / 4);
    }
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_p2p_inbox(mee_p2p* c, int64_t** d_keys, float** d_rows, uint64_t* n_slots) {
    if (!c) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_inbox: null argument");
    if (d_keys) *d_keys = c->inbox_keys;
    if (d_rows) *d_rows = c->inbox_rows;
    if (n_slots) *n_slots = (uint64_t)c->n_shards * c->cap;
    return MEE_OK;
}

int mee_p2p_find(mee_p2p* c, const mee_table* t, void* stream) {
    MEE_RANGE("mee_p2p_find");
    if (!c || !t) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_find: null argument");
    MEE_FP32_ROWS_ONLY(t, "mee_p2p_find");
    if (!c->connected) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_find: not connected");
    const TableView v = table_view(t);
    if (v.dim != c->dim || v.device != c->device) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_find: table dim/device mismatch");
    DeviceGuard g(c->device);
    const dim3 grid(grid_for(c->cap, 32, 1u << 16), c->n_shards);
    hipStream_t st = (hipStream_t)stream;
    with_row_shape(v.dim4, [&](auto d4) {
        p2p_find_kernel<d4, RowShape<d4>::rows_per_tile><<<grid, 256, 0, st>>>(v.keys, (const float4*)v.values, v.nb, v.dim4, v.default_value, c->inbox_keys,
                                                                               c->inbox_dst, c->inbox_cnt, p2p_peers(c), c->cap);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_p2p_barrier(mee_p2p* c, void* stream) {
    MEE_RANGE("mee_p2p_barrier");
    if (!c) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_barrier: null argument");
    if (!c->connected) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_barrier: not connected");
    DeviceGuard g(c->device);
    // wall_clock64 ticks at 100 MHz: wait at most 5 s for the slowest rank
    p2p_barrier_kernel<<<1, 64, 0, (hipStream_t)stream>>>(p2p_peers(c), c->rank, c->n_shards, c->status, 500000000ull);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_p2p_status(mee_p2p* c, uint32_t* bits_out, void* stream) {
    MEE_RANGE("mee_p2p_status");
    if (!c || !bits_out) return fail(MEE_ERR_INVALID_ARG, "mee_p2p_status: null argument");
    DeviceGuard g(c->device);
    MEE_HIP(hipMemcpyAsync(bits_out, c->status, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    MEE_HIP(hipStreamSynchronize((hipStream_t)stream));
    return MEE_OK;
}

int mee_scatter_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out, void* stream) {
    MEE_RANGE("mee_scatter_rows");
    return permute_rows<true>(d_rows, d_perm, n, row_bytes, d_out, stream, "mee_scatter_rows");
}
int mee_gather_rows(const void* d_rows, const int64_t* d_perm, size_t n, size_t row_bytes, void* d_out, void* stream) {
    MEE_RANGE("mee_gather_rows");
    return permute_rows<false>(d_rows, d_perm, n, row_bytes, d_out, stream, "mee_gather_rows");
}

}  // extern "C"
