// meepo_export.hip — everything that walks the whole table or reports on it: export, size, rehash (mee_reserve), the hit-counter scan of
// the hot/cold policy, eviction by those counters (mee_evict) and the counters by key, probe-length statistics, the status word; their half of the
// C-ABI.  Table layout: meepo_table.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>
#include <cstring>

#include "meepo_apply_part.h"

namespace mee {

// ---- access statistics for the hot/cold policy: keys whose hit counter lies in [lo, hi], optional reset ---------------
__global__ __launch_bounds__(256) void hits_scan_kernel(const int64_t* __restrict__ tkeys, uint32_t* hits, uint64_t capacity, uint32_t lo,
                                                        uint32_t hi, int reset, int64_t* keys_out, uint64_t cap, OpCounters* op) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr uint64_t kSpan = 64ull * 16;
    for (uint64_t c0 = wave * kSpan; c0 < capacity; c0 += n_waves * kSpan) {
        int64_t k[16];
        uint64_t m[16];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint64_t s = c0 + (uint64_t)j * 64 + lane;
            k[j] = s < capacity ? tkeys[s] : kEmpty;
            const uint32_t hcount = s < capacity ? hits[s] : 0;
            if (reset && s < capacity && hcount) hits[s] = 0;
            m[j] = __ballot(!reserved_key(k[j]) && hcount >= lo && hcount <= hi);
            total += (uint32_t)__popcll(m[j]);
        }
        if (!total) continue;  // wave-uniform
        unsigned long long pos0 = 0;
        if (lane == 0) pos0 = atomicAdd(&op->n_export, (unsigned long long)total);
        pos0 = __shfl(pos0, 0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if ((m[j] >> lane) & 1) {
                const uint64_t pos = pos0 + (uint64_t)__popcll(m[j] & ((1ull << lane) - 1));
                if (pos < cap) keys_out[pos] = k[j];
            }
            pos0 += (uint64_t)__popcll(m[j]);
        }
    }
}

// ---- eviction by the hit counters (SPEC.md §3 evict): selection, hand-out of the victims' rows, tombstones ---------------------------------------
// A CANDIDATE is a stored key whose counter is <= max_hits when the call starts; m = min(candidates, limit) of them are evicted.
//
// Threshold form, ONE launch (evict_kernel<false>) behind the zeroing of the ticket and the count word: a wave reads 512 consecutive slots (8
// coalesced key loads, 8 counter loads) and ballots the candidates; the 16 waves of a block add their counts up through LDS and take ONE ticket for
// all of them (a ticket per wave, as hits_scan_kernel takes it, ran into the rate of returning atomics on one word: 26K tickets at ~90 per us were
// 300 us of a scan that reads its planes in 50: profiles/evict.md); those whose position stays below the limit are the victims, served in slot order
// within the block.  Their key and counter leave from their own lane, their rows four at a time (a 16-lane tile per row, as export_kernel copies them: plain
// loads, which over a pinned-host plane is the zero-copy read of the cold tier), then the lane stores RECLAIMED and a zero counter.  A slot is touched
// by one lane of one wave and nothing probes while the launch runs, so the stores are plain.
//
// MEE_EVICT_LEAST, FIVE launches whatever the table holds:   zero (tickets, cuts, histograms, count word)
//                                                            evict_hist_kernel<0>   candidates per value of counter bits 31..22
//                                                            evict_hist_kernel<1>   cut 0 from histogram 0; the class it names, per value of bits 21..11
//                                                            evict_hist_kernel<2>   cut 1 from histogram 1; its class, per value of bits 10..0
//                                                            evict_kernel<true>     cut 2 from histogram 2: the threshold T and how many counters == T to take
// A cut (evict_cut) is a 256-thread scan of one histogram: the bin that holds the k-th smallest of the class the earlier cuts left, and the rank inside
// it.  Every block of the launch behind a histogram derives it for itself from the device words the launch before wrote — stream order is all that
// orders them, nothing is handed from block to block inside a launch — and block 0 stores it (EvictScratch::cut) for the launch after.  Behind the last
// digit the victims are every candidate below T and, by a second ticket aggregated over the wave (ballot) and the block (LDS), the first `take` of the
// candidates at T that come for one: exactly the m smallest counters, ties at the cut by arrival.
// Histogram: counters of a real table are nearly all tiny, so one digit value takes nearly every slot.  A wave peels the value of its first candidate
// lane (a ballot of the lanes that share it, ONE LDS add of the popcount), at most twice, before the lanes left add one by one; a block adds its LDS
// bins that are not zero to the global histogram when it is done: global atomics per launch = blocks x occupied bins.  An LDS bin is 32 bits: a block
// sees capacity / gridDim slots, 2^32 only beyond 2^43 slots.
// Both kernels give a wave two spans where the table has them (grid = a block per two block spans at most): the second span's loads are then issued
// by a wave that has its kernel arguments and cut already.
__device__ __forceinline__ EvictCut evict_cut(const unsigned long long* __restrict__ hist, int digit, EvictCut in, bool first, uint64_t limit) {
    __shared__ unsigned long long wtot[4];
    __shared__ EvictCut res;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t per = evict_bins(digit) / 256;   // bins of each of the block's first 256 threads: 4 or 8 consecutive ones (the others hold none)
    const bool holds = threadIdx.x < 256;
    unsigned long long h[8], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        h[j] = holds && j < per ? hist[threadIdx.x * per + j] : 0ull;
        sum += h[j];
    }
    unsigned long long inc = sum;   // inclusive scan over the wave, the four wave totals through LDS
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63 && w < 4) wtot[w] = inc;
    if (threadIdx.x == 0) res = EvictCut{0ull, 0u, 0u};
    __syncthreads();
    unsigned long long before = inc - sum, total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        before += q < w ? wtot[q] : 0ull;
        total += wtot[q];
    }
    const unsigned long long k = first ? (total < limit ? total : limit) : in.k;   // m = min(candidates, limit): known once histogram 0 is
    if (holds && (first || in.valid) && k >= 1 && before < k && k <= before + sum) {         // the one thread whose bins hold rank k
        unsigned long long below = before;
        uint32_t bin = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            if (j < per && below < k && k <= below + h[j]) { bin = threadIdx.x * per + j; break; }
            below += h[j];
        }
        res = EvictCut{k - below, (first ? 0u : in.prefix) | bin << evict_shift(digit), 1u};
    }
    __syncthreads();
    return res;
}

template <int DIGIT>
__global__ __launch_bounds__(256) void evict_hist_kernel(const int64_t* __restrict__ tkeys, const uint32_t* __restrict__ hits, uint64_t capacity,
                                                         uint32_t max_hits, uint64_t limit, EvictScratch* sc) {
    __shared__ uint32_t lh[kEvictBins];
    constexpr uint32_t bins = evict_bins(DIGIT);
    EvictCut cut{limit, 0u, 1u};
    if constexpr (DIGIT > 0) {
        if constexpr (DIGIT > 1) cut = sc->cut[DIGIT - 2];   // what block 0 of the launch before stored
        cut = evict_cut(sc->hist[DIGIT - 1], DIGIT - 1, cut, DIGIT == 1, limit);
        if (blockIdx.x == 0 && threadIdx.x == 0) sc->cut[DIGIT - 1] = cut;
        if (!cut.valid) return;   // block-uniform: nothing will be evicted
    }
    for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x) lh[b] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr uint64_t kSpan = 64ull * 16;
    for (uint64_t c0 = wave * kSpan; c0 < capacity; c0 += n_waves * kSpan) {
        int64_t k[16];
        uint32_t h[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint64_t s = c0 + (uint64_t)j * 64 + lane;
            k[j] = s < capacity ? tkeys[s] : kEmpty;
            h[j] = s < capacity ? hits[s] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            bool in = !reserved_key(k[j]) && h[j] <= max_hits;   // (EMPTY and RECLAIMED slots are no candidates, whatever their counter word holds)
            if constexpr (DIGIT > 0) in = in && ((h[j] ^ cut.prefix) >> evict_shift(DIGIT - 1)) == 0u;
            const uint32_t d = (h[j] >> evict_shift(DIGIT)) & (bins - 1u);
            uint64_t rest = __ballot(in);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (!rest) break;   // wave-uniform
                const int head = __ffsll((unsigned long long)rest) - 1;
                const uint32_t d0 = __shfl(d, head);
                const uint64_t same = __ballot(in && d == d0) & rest;
                if (lane == head) atomicAdd(&lh[d0], (uint32_t)__popcll(same));
                rest &= ~same;
            }
            if ((rest >> lane) & 1) atomicAdd(&lh[d], 1u);
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins; b += blockDim.x)
        if (lh[b]) atomicAdd(&sc->hist[DIGIT][b], (unsigned long long)lh[b]);
}

constexpr int kEvictGroups = 8;   // 64-slot groups of a wave's span in evict_kernel: two ballot masks per group stay in scalar registers
constexpr int kEvictBlock = 1024;  // threads of an evict_kernel block: its 16 waves share ONE ticket per 8192 slots
template <bool LEAST>
__global__ __launch_bounds__(kEvictBlock) void evict_kernel(int64_t* tkeys, uint32_t* hits, const float4* __restrict__ values, const float4* __restrict__ s1,
                                                            const float4* __restrict__ s2, uint64_t capacity, uint32_t dim4, uint32_t max_hits,
                                                            uint64_t limit, int reset, int64_t* keys_out, float4* values_out, float4* s1_out,
                                                            float4* s2_out, uint32_t* hits_out, unsigned long long* n_out, EvictScratch* sc) {
    constexpr int kWaves = kEvictBlock / 64;
    __shared__ uint32_t w_sure[kWaves], w_tie[kWaves];   // per wave of the block: sure victims, members of the tied class in its span
    __shared__ unsigned long long b_pos0;                // the block's first output position
    __shared__ uint32_t b_allowed;                       // members of the tied class the block may take
    uint32_t thr = 0;            // LEAST: candidates below it are victims, candidates at it while the tie ticket lasts
    uint64_t take = limit;       // tickets of the tied class that are served (threshold form: every candidate is "tied", the first `limit` are served)
    bool on = true;
    if constexpr (LEAST) {
        const EvictCut cut = evict_cut(sc->hist[kEvictDigits - 1], kEvictDigits - 1, sc->cut[kEvictDigits - 2], false, limit);
        if (blockIdx.x == 0 && threadIdx.x == 0) sc->cut[kEvictDigits - 1] = cut;
        thr = cut.prefix; take = cut.k; on = cut.valid != 0u;
    }
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15, w = threadIdx.x >> 6;
    const uint64_t lt = (1ull << lane) - 1ull;
    constexpr uint64_t kSpan = 64ull * kEvictGroups, kBlockSpan = kSpan * kWaves;
    for (uint64_t b0 = (uint64_t)blockIdx.x * kBlockSpan; b0 < capacity; b0 += (uint64_t)gridDim.x * kBlockSpan) {   // block-uniform
        const uint64_t c0 = b0 + (uint64_t)w * kSpan;   // (a wave whose span starts past the end has no candidates and still meets the barriers)
        int64_t k[kEvictGroups];
        uint32_t h[kEvictGroups];
        uint64_t ms[kEvictGroups], mt[kEvictGroups];   // per 64-slot group: sure victims (below the threshold), members of the tied class
        uint32_t n_sure = 0, n_tie = 0;
#pragma unroll
        for (int j = 0; j < kEvictGroups; ++j) {
            const uint64_t s = c0 + (uint64_t)j * 64 + lane;
            k[j] = s < capacity ? tkeys[s] : kEmpty;
            h[j] = s < capacity ? hits[s] : 0u;
        }
#pragma unroll
        for (int j = 0; j < kEvictGroups; ++j) {
            const bool cand = on && !reserved_key(k[j]) && h[j] <= max_hits;
            ms[j] = LEAST ? __ballot(cand && h[j] < thr) : 0ull;
            mt[j] = __ballot(cand && (!LEAST || h[j] == thr));
            n_sure += (uint32_t)__popcll(ms[j]);
            n_tie += (uint32_t)__popcll(mt[j]);
        }
        if (lane == 0) { w_sure[w] = n_sure; w_tie[w] = n_tie; }
        __syncthreads();
        if (threadIdx.x == 0) {   // ONE ticket for the block's ties, ONE range of output positions for its victims
            uint32_t sure = 0, tie = 0;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) { sure += w_sure[q]; tie += w_tie[q]; }
            unsigned long long t0 = 0;
            if (tie) t0 = atomicAdd(LEAST ? &sc->tie_ticket : &sc->out_ticket, (unsigned long long)tie);
            const uint32_t al = t0 >= take ? 0u : (take - t0 < tie ? (uint32_t)(take - t0) : tie);
            unsigned long long p0 = t0;   // threshold form: the ticket is the output position
            if constexpr (LEAST) p0 = sure + al ? atomicAdd(&sc->out_ticket, (unsigned long long)(sure + al)) : 0ull;
            if (n_out && sure + al) atomicAdd(n_out, (unsigned long long)(sure + al));
            b_allowed = al; b_pos0 = p0;
        }
        __syncthreads();
        // this wave's share: the block's ties are served in wave order, its victims are written in wave order
        uint32_t ties_before = 0, allowed = 0;
        unsigned long long pos0 = b_pos0;
        {
            const uint32_t al = b_allowed;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) {
                const uint32_t tq = w_tie[q];
                const uint32_t aq = ties_before >= al ? 0u : (al - ties_before < tq ? al - ties_before : tq);   // ties wave q takes
                if (q < w) pos0 += w_sure[q] + aq;
                if (q == w) allowed = aq;
                ties_before += tq;
            }
        }
        if (n_sure + allowed || reset) {   // wave-uniform
            uint32_t t_done = 0;
#pragma unroll
            for (int j = 0; j < kEvictGroups; ++j) {
                const uint64_t s = c0 + (uint64_t)j * 64 + lane;
                const bool victim = ((ms[j] >> lane) & 1) || (((mt[j] >> lane) & 1) && t_done + (uint32_t)__popcll(mt[j] & lt) < allowed);
                const uint64_t v = __ballot(victim);
                t_done += (uint32_t)__popcll(mt[j]);
                if (victim) {
                    const uint64_t pos = pos0 + (uint64_t)__popcll(v & lt);
                    if (pos < limit) {   // (always: m <= limit positions are handed out)
                        if (keys_out) keys_out[pos] = k[j];
                        if (hits_out) hits_out[pos] = h[j];
                    }
                    tkeys[s] = kReclaimed;
                }
                if (s < capacity && h[j] && (victim || reset)) hits[s] = 0u;
                uint64_t rest = (values_out || s1_out || s2_out) ? v : 0ull;
                uint64_t done = 0;
                while (rest) {  // wave-uniform
                    uint64_t mm = rest;
                    int p = -1;
                    for (int q = 0; q <= tile; ++q) {
                        if (mm) { p = __ffsll((unsigned long long)mm) - 1; mm &= mm - 1; } else p = -1;
                    }
                    const uint64_t pos = pos0 + done + tile;
                    if (p >= 0 && pos < limit) {
                        const uint64_t src = (c0 + (uint64_t)j * 64 + p) * dim4, dst = pos * dim4;
                        for (uint32_t c = tl; c < dim4; c += 16) {
                            if (values_out) values_out[dst + c] = values[src + c];
                            if (s1_out) s1_out[dst + c] = s1[src + c];
                            if (s2_out) s2_out[dst + c] = s2[src + c];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) rest &= rest - 1;  // x & (x-1) of 0 stays 0
                    done += 4;
                }
                pos0 += (uint64_t)__popcll(v);
            }
        }
        __syncthreads();   // the wave counts are rewritten by the next round
    }
}

// the zeroing in front of an eviction: the scratch words the form uses (tickets; LEAST: cuts and histograms too) and the caller's count word, one launch
__global__ __launch_bounds__(1024) void evict_zero_kernel(uint32_t* scratch, uint32_t n_words, unsigned long long* n_out) {
    for (uint32_t i = threadIdx.x; i < n_words; i += blockDim.x) scratch[i] = 0u;
    if (n_out && threadIdx.x == 0) *n_out = 0ull;
}

// ---- the counters by key (SPEC.md §3 hits_find / hits_assign): a 16-lane tile per key, the read-only probe of the lookups ---------------------------
template <bool ASSIGN>
__global__ __launch_bounds__(256) void hits_keys_kernel(const int64_t* __restrict__ tkeys, uint64_t nb, uint32_t* hits, const int64_t* __restrict__ keys,
                                                        uint32_t n, uint32_t* __restrict__ hits_out, const uint32_t* __restrict__ hits_in) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr int R = 2;
    for (uint64_t base = wave * 4 * R; base < n; base += n_waves * 4 * R) {   // wave-uniform
        uint64_t b[R];
        int64_t key[R], kb[R], slot[R];
        bool act[R];
        const int64_t kmine = (lane < 4 * R && base + lane < n) ? keys[base + lane] : kEmpty;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            key[r] = __shfl(kmine, r * 4 + tile);
            act[r] = base + r * 4 + tile < n && !reserved_key(key[r]);
            b[r] = bucket_of(key[r], nb);
            kb[r] = act[r] ? tkeys[b[r] * kW + tl] : kEmpty;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = tile_probe(tkeys, nb, key[r], act[r], b[r], kb[r], tile, tl);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint64_t i = base + r * 4 + tile;
            if (i >= n || tl != 0) continue;
            if constexpr (ASSIGN) { if (slot[r] >= 0) hits[slot[r]] = hits_in[i]; }
            else hits_out[i] = slot[r] >= 0 ? hits[slot[r]] : 0u;
        }
    }
}
// hits_decay: every counter >>= shift (>= 32: zero), as sketch_decay ages the admission sketch
__global__ __launch_bounds__(256) void hits_decay_kernel(uint32_t* hits, uint64_t capacity, uint32_t shift) {
    for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < capacity; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = hits[s];
        if (c) hits[s] = shift >= 32u ? 0u : c >> shift;
    }
}

// ---- probe-length statistics (SURVEY.md §8d "mean probe length"): buckets visited per lookup, summed over the batch ----
__global__ __launch_bounds__(256) void probe_length_kernel(const int64_t* __restrict__ tkeys, uint64_t nb, const int64_t* __restrict__ keys,
                                                           uint64_t n, OpCounters* op) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    unsigned long long visited = 0, hist = 0;   // hist: four 16-bit counters (a wave takes at most 4096 keys per counter before they are flushed below)
    uint32_t rounds = 0;
    auto flush = [&]() {
        unsigned long long h = hist;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {   // field-wise sums: 64 lanes x 2^10 per field stay below 2^16
            const unsigned long long o = (unsigned long long)(uint32_t)__shfl_down((int)(uint32_t)h, d) | (unsigned long long)(uint32_t)__shfl_down((int)(uint32_t)(h >> 32), d) << 32;
            h += o;
        }
        if (lane == 0)
            for (int q = 0; q < 4; ++q) { const unsigned long long c = (h >> (16 * q)) & 0xFFFFull; if (c) atomicAdd(&op->hist[q], c); }
        hist = 0;
    };
    for (uint64_t base = wave * 4; base < n; base += n_waves * 4) {
        const uint64_t i = base + tile;
        const int64_t key = i < n ? keys[i] : kEmpty;
        bool pend = i < n && !reserved_key(key);
        uint64_t b = bucket_of(key, nb), steps = 0;
        uint32_t mine = 0;
        while (__any(pend)) {
            const int64_t k = pend ? tkeys[b * kW + tl] : kEmpty;
            const uint32_t tm = tile_bits(__ballot(pend && k == key), tile);
            const uint32_t te = tile_bits(__ballot(pend && k == kEmpty), tile);
            if (pend) {
                if (tl == 0) { ++visited; ++mine; }
                if (tm || te || ++steps >= nb) pend = false;
                else b = next_bucket(b, step_of(key, nb), nb);
            }
        }
        if (mine) hist += 1ull << (16 * (min(mine, 4u) - 1u));
        if (++rounds == 1000) { flush(); rounds = 0; }   // (wave-uniform)
    }
    flush();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) visited += __shfl_down(visited, d);
    if (lane == 0 && visited) atomicAdd(&op->n_export, visited);
}

// ---- size (SPEC.md §3): count stored keys by scanning the key plane (keeps every atomic off the insert path) ----
__global__ __launch_bounds__(256) void count_kernel(const int64_t* __restrict__ tkeys, uint64_t capacity, OpCounters* op) {
    __shared__ uint32_t wsum[4];
    uint32_t c = 0;
    for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < capacity; s += (uint64_t)gridDim.x * blockDim.x)
        c += !reserved_key(tkeys[s]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(&op->n_export, (unsigned long long)tot);
    }
}

// ---- reserve / rehash (SPEC.md §3): every stored pair moves, device to device, into key/row planes of another capacity ----
// A wave reads 64 consecutive old slots (one coalesced key load), then its four tiles take the stored keys four at a
// time: claim a slot in the new key plane (same CAS protocol as insert: all keys are distinct, claims of different
// waves race for slots) and copy the row, the optimizer planes and the hit counter.
__global__ __launch_bounds__(256) void rehash_kernel(const int64_t* __restrict__ okeys, const float4* __restrict__ ov,
                                                     const float4* __restrict__ o1, const float4* __restrict__ o2,
                                                     const uint32_t* __restrict__ ohits, uint64_t old_capacity, int64_t* nkeys,
                                                     float4* nv, float4* n1, float4* n2, uint32_t* nhits, uint64_t nnb,
                                                     uint32_t dim4, Counters* ctr) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t c0 = wave * 64; c0 < old_capacity; c0 += n_waves * 64) {
        const uint64_t s = c0 + lane;
        const int64_t k = s < old_capacity ? okeys[s] : kEmpty;
        uint64_t rest = __ballot(!reserved_key(k));
        while (rest) {  // wave-uniform
            uint64_t mm = rest;
            int p = -1;
            for (int q = 0; q <= tile; ++q) {
                if (mm) { p = __ffsll((unsigned long long)mm) - 1; mm &= mm - 1; } else p = -1;
            }
            const int64_t key = __shfl(k, p >= 0 ? p : 0);
            bool is_new, full;
            const int64_t slot = tile_locate<true, true>(nkeys, nnb, key, p >= 0, tile, tl, is_new, full);
            if (p >= 0) {
                if (slot >= 0) {
                    const uint64_t src = (c0 + (uint64_t)p) * dim4, dst = (uint64_t)slot * dim4;
                    for (uint32_t c = tl; c < dim4; c += 16) {
                        nv[dst + c] = ov[src + c];
                        if (n1) n1[dst + c] = o1[src + c];
                        if (n2) n2[dst + c] = o2[src + c];
                    }
                    if (nhits && tl == 0) nhits[slot] = ohits[c0 + p];
                } else if (tl == 0) {
                    atomicOr(&ctr->status, (uint32_t)MEE_STATUS_TABLE_FULL);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) rest &= rest - 1;
        }
    }
}

// ---- export (SPEC.md §3) -----------------------------------------------------------------------------------
// A wave owns a chunk of 1024 consecutive slots.  Pass A: 16 coalesced key loads, ballot + popcount -> occupied
// count, ONE atomic reserves the chunk's output range.  Pass B: per 64-slot group, ranks from the ballot mask;
// keys are written by their own lane, rows are copied four at a time (one per 16-lane tile).
// ROWS: the storage type of `values` (RowType, meepo_device.h).  A bf16-row or int8-row plane has no state planes; its groups are widened or dequantized
// (the tile loads the row's scale with its words) on their way into the fp32 values_out — source and destination are different buffers, so nothing is
// expanded in place.
constexpr int kExportGroups = 16;

template <int ROWS>
__global__ __launch_bounds__(256) void export_kernel(const int64_t* __restrict__ tkeys, const float4* __restrict__ values,
                                                     const float4* __restrict__ s1, const float4* __restrict__ s2,
                                                     uint64_t begin, uint64_t capacity /* = end of the slot range */, uint32_t dim4,
                                                     int64_t* keys_out, float4* values_out,
                                                     float4* s1_out, float4* s2_out, uint64_t cap, OpCounters* op) {
    const int lane = threadIdx.x & 63, tile = lane >> 4, tl = lane & 15;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t n_waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    constexpr uint64_t kSpan = 64ull * kExportGroups;
    for (uint64_t c0 = begin + wave * kSpan; c0 < capacity; c0 += n_waves * kSpan) {
        int64_t k[kExportGroups];
        uint64_t m[kExportGroups];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < kExportGroups; ++j) {
            const uint64_t s = c0 + (uint64_t)j * 64 + lane;
            k[j] = s < capacity ? tkeys[s] : kEmpty;
            m[j] = __ballot(!reserved_key(k[j]));
            total += (uint32_t)__popcll(m[j]);
        }
        if (!total) continue;  // wave-uniform
        unsigned long long pos0 = 0;
        if (lane == 0) pos0 = atomicAdd(&op->n_export, (unsigned long long)total);
        pos0 = __shfl(pos0, 0);
#pragma unroll
        for (int j = 0; j < kExportGroups; ++j) {
            if (!reserved_key(k[j])) {
                const uint64_t pos = pos0 + (uint64_t)__popcll(m[j] & ((1ull << lane) - 1));
                if (keys_out && pos < cap) keys_out[pos] = k[j];
            }
            uint64_t rest = m[j];
            uint64_t done = 0;
            while (rest) {  // wave-uniform
                uint64_t mm = rest;
                int p = -1;
                for (int q = 0; q <= tile; ++q) {
                    if (mm) { p = __ffsll((unsigned long long)mm) - 1; mm &= mm - 1; } else p = -1;
                }
                const uint64_t pos = pos0 + done + tile;
                if (p >= 0 && pos < cap) {
                    const uint64_t src = (c0 + (uint64_t)j * 64 + p) * dim4, dst = pos * dim4;
                    using RT = RowType<ROWS>;
                    const uint32_t tail = RT::template load_tail<false, true>(RT::plane(values), (int64_t)(c0 + (uint64_t)j * 64 + p), dim4);
                    for (uint32_t c = tl; c < dim4; c += 16) {
                        if constexpr (ROWS == kRowsF32) {   // (a float4 plane as it is)
                            if (values_out) values_out[dst + c] = values[src + c];
                        } else if (values_out) {
                            const f32x4 v = RT::value(RT::plane(values)[RT::first((int64_t)(c0 + (uint64_t)j * 64 + p), dim4) + c], tail, true, f32x4{});
                            values_out[dst + c] = make_float4(v.x, v.y, v.z, v.w);
                        }
                        if (s1_out) s1_out[dst + c] = s1[src + c];
                        if (s2_out) s2_out[dst + c] = s2[src + c];
                    }
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) rest &= rest - 1;  // x & (x-1) of 0 stays 0
                done += 4;
            }
            pos0 += (uint64_t)__popcll(m[j]);
        }
    }
}

}  // namespace mee

using namespace mee;

extern "C" {

int mee_reserve(mee_table* t, uint64_t new_capacity, void* stream) {
    MEE_RANGE("mee_reserve");
    if (!t || new_capacity == 0) return fail(MEE_ERR_INVALID_ARG, "mee_reserve: null table or zero capacity");
    if (t->pending.n) {
        if (!t->pending.by_forward) return fail(MEE_ERR_INVALID_ARG, "mee_reserve: a prepared apply is pending on this table (finish it with mee_apply_* or mee_apply_discard)");
        if (int rc = mee_apply_discard(t, stream)) return rc;   // a training forward's partition: the apply that follows partitions its batch again
    }
    size_t stored = 0;
    if (int rc = mee_size(t, &stored, stream)) return rc;
    const uint64_t nnb = next_prime((new_capacity + kW - 1) / kW), ncap = nnb * kW;
    if (ncap < stored) return fail(MEE_ERR_INVALID_ARG, "mee_reserve: capacity %llu is below the %zu stored keys", (unsigned long long)ncap, stored);
    if (nnb == t->nb) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    int64_t* nkeys = nullptr; uint32_t* nhits = nullptr;
    float *nv = nullptr, *n1 = nullptr, *n2 = nullptr;
    const uint64_t plane = ncap * (uint64_t)t->row_bytes;
    hipError_t e = hipMalloc((void**)&nkeys, ncap * sizeof(int64_t));
    if (e == hipSuccess && t->hits) e = hipMalloc((void**)&nhits, ncap * sizeof(uint32_t));
    if (e == hipSuccess) e = plane_alloc(t->value_memory, &nv, plane);
    if (e == hipSuccess && t->s1) e = plane_alloc(t->value_memory, &n1, plane);
    if (e == hipSuccess && t->s2) e = plane_alloc(t->value_memory, &n2, plane);
    if (e == hipSuccess) {
        fill_keys(nkeys, ncap, kEmpty, st);
        e = hipGetLastError();
    }
    if (e == hipSuccess && nhits) e = hipMemsetAsync(nhits, 0, ncap * sizeof(uint32_t), st);
    if (e == hipSuccess) {
        rehash_kernel<<<grid_for(t->capacity, 256, 1u << 16), 256, 0, st>>>(t->keys, (const float4*)t->values, (const float4*)t->s1, (const float4*)t->s2,
                                                                          t->hits, t->capacity, nkeys, (float4*)nv, (float4*)n1, (float4*)n2, nhits, nnb,
                                                                          t->mv_dim4, t->ctr);   // (rows move bit for bit, as opaque 16-byte groups)
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {   // the table is untouched
        (void)hipFree(nkeys); (void)hipFree(nhits);
        plane_free(t->value_memory, nv); plane_free(t->value_memory, n1); plane_free(t->value_memory, n2);
        return fail(e == hipErrorOutOfMemory ? MEE_ERR_OUT_OF_MEMORY : MEE_ERR_HIP, "mee_reserve(%llu slots): %s (old and new planes must fit together)",
                    (unsigned long long)ncap, hipGetErrorString(e));
    }
    (void)hipFree(t->keys); (void)hipFree(t->hits);
    plane_free(t->value_memory, t->values); plane_free(t->value_memory, t->s1); plane_free(t->value_memory, t->s2);
    t->keys = nkeys; t->hits = nhits; t->values = nv; t->s1 = n1; t->s2 = n2;
    t->nb = nnb; t->capacity = ncap;
    t->table_bytes = ncap * sizeof(int64_t) + (nhits ? ncap * sizeof(uint32_t) : 0) + plane * (1 + (n1 != nullptr) + (n2 != nullptr));
    ++t->generation;
    ++t->handle_epoch;
    return MEE_OK;
}

int mee_hits_scan(mee_table* t, uint32_t min_hits, uint32_t max_hits, int reset, int64_t* d_keys_out, size_t cap, size_t* n_out,
                  void* stream) {
    MEE_RANGE("mee_hits_scan");
    MEE_FP32_ROWS_ONLY(t, "mee_hits_scan");
    if (!t || !n_out || (cap && !d_keys_out)) return fail(MEE_ERR_INVALID_ARG, "mee_hits_scan: null argument");
    if (!t->hits) return fail(MEE_ERR_UNSUPPORTED, "mee_hits_scan: table was created without MEE_FLAG_TRACK_HITS");
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(&t->op->n_export, sizeof(unsigned long long), st);
    hits_scan_kernel<<<grid_for(t->capacity, 4 * 1024, 4096), 256, 0, st>>>(t->keys, t->hits, t->capacity, min_hits, max_hits, reset, d_keys_out, cap, t->op);
    MEE_HIP(hipGetLastError());
    MEE_HIP(hipMemcpyAsync(t->h_op, t->op, sizeof(OpCounters), hipMemcpyDeviceToHost, st));
    MEE_HIP(hipStreamSynchronize(st));
    *n_out = (size_t)t->h_op->n_export;  // how many keys qualified; min(*n_out, cap) were written
    return MEE_OK;
}

int mee_evict(mee_table* t, uint32_t max_hits, uint64_t max_evict, uint32_t flags, int64_t* d_keys_out, float* d_values_out, float* d_state1_out,
              float* d_state2_out, uint32_t* d_hits_out, size_t cap, uint64_t* d_n_out, void* stream) {
    MEE_RANGE("mee_evict");
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_evict: null table");
    if (flags & ~(uint32_t)(MEE_EVICT_LEAST | MEE_EVICT_RESET)) return fail(MEE_ERR_INVALID_ARG, "mee_evict: unknown flag bits 0x%x", flags);
    MEE_FP32_ROWS_ONLY(t, "mee_evict");
    if (!t->hits) return fail(MEE_ERR_UNSUPPORTED, "mee_evict: table was created without MEE_FLAG_TRACK_HITS");
    if (int rc = check_batch(t, 0, "mee_evict", stream)) return rc;   // as mee_remove: a partition a training forward left pending is dropped, a prepared apply refuses
    // a key never leaves without its row being handed out when a row was asked for
    const bool hands_out = d_keys_out || d_values_out || d_state1_out || d_state2_out || d_hits_out;
    const uint64_t limit = hands_out && (uint64_t)cap < max_evict ? (uint64_t)cap : max_evict;
    const bool least = (flags & MEE_EVICT_LEAST) != 0;
    const int reset = (flags & MEE_EVICT_RESET) != 0;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    ++t->handle_epoch;   // rows are freed: slot handles handed out before this call are stale
    unsigned long long* cnt = (unsigned long long*)d_n_out;
    const unsigned grid = grid_for(t->capacity, 2 * kEvictBlock * kEvictGroups, 4096), hist_grid = grid_for(t->capacity, 2 * 4 * 1024, 2048);
    evict_zero_kernel<<<1, 1024, 0, st>>>((uint32_t*)t->evict, (uint32_t)((least ? sizeof(EvictScratch) : kEvictTicketBytes) / 4), cnt);
    if (least) {
        evict_hist_kernel<0><<<hist_grid, 256, 0, st>>>(t->keys, t->hits, t->capacity, max_hits, limit, t->evict);
        evict_hist_kernel<1><<<hist_grid, 256, 0, st>>>(t->keys, t->hits, t->capacity, max_hits, limit, t->evict);
        evict_hist_kernel<2><<<hist_grid, 256, 0, st>>>(t->keys, t->hits, t->capacity, max_hits, limit, t->evict);
    }
    with_flag(least, [&](auto l) {
        evict_kernel<decltype(l)::value><<<grid, kEvictBlock, 0, st>>>(t->keys, t->hits, (const float4*)t->values, (const float4*)t->s1, (const float4*)t->s2, t->capacity, t->dim4,
                                                             max_hits, limit, reset, d_keys_out, (float4*)d_values_out, t->s1 ? (float4*)d_state1_out : nullptr,
                                                             t->s2 ? (float4*)d_state2_out : nullptr, d_hits_out, cnt, t->evict);
    });
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

// what the three counter operators refuse before anything is launched
static int hits_op_check(const mee_table* t, const char* name) {
    if (!t) return fail(MEE_ERR_INVALID_ARG, "%s: null table", name);
    MEE_FP32_ROWS_ONLY(t, name);
    if (!t->hits) return fail(MEE_ERR_UNSUPPORTED, "%s: table was created without MEE_FLAG_TRACK_HITS", name);
    return MEE_OK;
}
int mee_hits_find(const mee_table* t, const int64_t* d_keys, size_t n, uint32_t* d_hits_out, void* stream) {
    MEE_RANGE("mee_hits_find");
    if (int rc = hits_op_check(t, "mee_hits_find")) return rc;
    if (n && (!d_keys || !d_hits_out)) return fail(MEE_ERR_INVALID_ARG, "mee_hits_find: null argument");
    if (int rc = check_batch(const_cast<mee_table*>(t), n, "mee_hits_find", stream, false)) return rc;   // a lookup: no per-batch scratch, nothing pending is touched
    if (n == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hits_keys_kernel<false><<<grid_for(n, 32, 1u << 16), 256, 0, as_stream(stream)>>>(t->keys, t->nb, t->hits, d_keys, (uint32_t)n, d_hits_out, nullptr);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}
int mee_hits_assign(mee_table* t, const int64_t* d_keys, size_t n, const uint32_t* d_hits, void* stream) {
    MEE_RANGE("mee_hits_assign");
    if (int rc = hits_op_check(t, "mee_hits_assign")) return rc;
    if (n && (!d_keys || !d_hits)) return fail(MEE_ERR_INVALID_ARG, "mee_hits_assign: null argument");
    if (int rc = check_batch(t, n, "mee_hits_assign", stream, false)) return rc;   // no row moves and no scratch is used: handles and a pending partition stay
    if (n == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hits_keys_kernel<true><<<grid_for(n, 32, 1u << 16), 256, 0, as_stream(stream)>>>(t->keys, t->nb, t->hits, d_keys, (uint32_t)n, nullptr, d_hits);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}
int mee_hits_decay(mee_table* t, uint32_t shift, void* stream) {
    MEE_RANGE("mee_hits_decay");
    if (int rc = hits_op_check(t, "mee_hits_decay")) return rc;
    DeviceGuard g(t->device);
    hits_decay_kernel<<<grid_for(t->capacity, 256 * 16, 2048), 256, 0, as_stream(stream)>>>(t->hits, t->capacity, shift);
    MEE_HIP(hipGetLastError());
    return MEE_OK;
}

int mee_export(const mee_table* t, int64_t* d_keys_out, float* d_values_out, float* d_state1_out, float* d_state2_out,
               size_t cap, size_t* n_out, void* stream) {
    MEE_RANGE("mee_export");
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_export: null argument");
    return mee_export_range(t, 0, t->capacity, d_keys_out, d_values_out, d_state1_out, d_state2_out, cap, n_out, stream);
}

int mee_export_range(const mee_table* t, uint64_t slot_begin, uint64_t slot_end, int64_t* d_keys_out, float* d_values_out,
                     float* d_state1_out, float* d_state2_out, size_t cap, size_t* n_out, void* stream) {
    MEE_RANGE("mee_export_range");
    if (!t || !n_out) return fail(MEE_ERR_INVALID_ARG, "mee_export: null argument");
    if (slot_end > t->capacity) slot_end = t->capacity;
    if (slot_begin > slot_end) return fail(MEE_ERR_INVALID_ARG, "mee_export_range: slot_begin %llu > slot_end %llu", (unsigned long long)slot_begin, (unsigned long long)slot_end);
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(&t->op->n_export, sizeof(unsigned long long), st);
    with_value<kRowsI8, kRowsBF16, kRowsF32>(t->int8_rows ? kRowsI8 : t->bf16_rows ? kRowsBF16 : kRowsF32, [&](auto rows) {
        export_kernel<decltype(rows)::value><<<grid_for(slot_end - slot_begin, 4 * 64 * kExportGroups, 256 * 16), 256, 0, st>>>(
            t->keys, (const float4*)t->values, (const float4*)t->s1, (const float4*)t->s2, slot_begin, slot_end, t->dim4, d_keys_out,
            (float4*)d_values_out, t->s1 ? (float4*)d_state1_out : nullptr, t->s2 ? (float4*)d_state2_out : nullptr, cap, t->op);
    });
    MEE_HIP(hipGetLastError());
    MEE_HIP(hipMemcpyAsync(t->h_op, t->op, sizeof(OpCounters), hipMemcpyDeviceToHost, st));
    MEE_HIP(hipStreamSynchronize(st));
    *n_out = (size_t)t->h_op->n_export;
    return MEE_OK;
}

static int read_counters(const mee_table* t, void* stream) {
    DeviceGuard g(t->device);
    MEE_HIP(hipMemcpyAsync(t->h_ctr, t->ctr, sizeof(Counters), hipMemcpyDeviceToHost, as_stream(stream)));
    MEE_HIP(hipStreamSynchronize(as_stream(stream)));
    return MEE_OK;
}
int mee_size(const mee_table* t, size_t* n_out, void* stream) {
    MEE_RANGE("mee_size");
    if (!t || !n_out) return fail(MEE_ERR_INVALID_ARG, "mee_size: null argument");
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(&t->op->n_export, sizeof(unsigned long long), st);
    count_kernel<<<grid_for(t->capacity, 256 * 16, 2048), 256, 0, st>>>(t->keys, t->capacity, t->op);
    MEE_HIP(hipGetLastError());
    MEE_HIP(hipMemcpyAsync(t->h_op, t->op, sizeof(OpCounters), hipMemcpyDeviceToHost, st));
    MEE_HIP(hipStreamSynchronize(st));
    *n_out = (size_t)t->h_op->n_export;
    return MEE_OK;
}
int mee_table_plane(const mee_table* t, uint32_t plane, void** ptr_out, uint64_t* row_stride_bytes, uint32_t* value_memory) {
    if (!t || !ptr_out) return fail(MEE_ERR_INVALID_ARG, "mee_table_plane: null argument");
    const float* p = plane_of(t, plane);
    if (!p) return fail(MEE_ERR_UNSUPPORTED, "mee_table_plane: plane %u does not exist (optimizer=%u)", plane, t->optimizer);
    *ptr_out = const_cast<float*>(p);
    if (row_stride_bytes) *row_stride_bytes = t->row_bytes;   // 4 x dim, 2 x dim (bf16 rows) or dim + 16 (int8 rows)
    if (value_memory) *value_memory = t->value_memory;
    return MEE_OK;
}

int mee_probe_length(const mee_table* t, const int64_t* d_keys, size_t n, uint64_t* buckets_visited_out, void* stream) {
    MEE_RANGE("mee_probe_length");
    if (!t || !buckets_visited_out || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_probe_length: null argument");
    *buckets_visited_out = 0;
    if (n == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(&t->op->n_export, sizeof(unsigned long long), st);
    probe_length_kernel<<<grid_for(n, 16, 4096), 256, 0, st>>>(t->keys, t->nb, d_keys, n, t->op);
    MEE_HIP(hipGetLastError());
    MEE_HIP(hipMemcpyAsync(t->h_op, t->op, sizeof(OpCounters), hipMemcpyDeviceToHost, st));
    MEE_HIP(hipStreamSynchronize(st));
    *buckets_visited_out = (uint64_t)t->h_op->n_export;
    return MEE_OK;
}
int mee_probe_histogram(const mee_table* t, const int64_t* d_keys, size_t n, uint64_t* hist_out /* [4] */, void* stream) {
    MEE_RANGE("mee_probe_histogram");
    if (!t || !hist_out || (n && !d_keys)) return fail(MEE_ERR_INVALID_ARG, "mee_probe_histogram: null argument");
    for (int q = 0; q < 4; ++q) hist_out[q] = 0;
    if (n == 0) return MEE_OK;
    DeviceGuard g(t->device);
    hipStream_t st = as_stream(stream);
    zero_words(&t->op->n_export, sizeof(unsigned long long), st);
    zero_words(t->op->hist, sizeof t->op->hist, st);
    probe_length_kernel<<<grid_for(n, 16, 4096), 256, 0, st>>>(t->keys, t->nb, d_keys, n, t->op);
    MEE_HIP(hipGetLastError());
    MEE_HIP(hipMemcpyAsync(t->h_op, t->op, sizeof(OpCounters), hipMemcpyDeviceToHost, st));
    MEE_HIP(hipStreamSynchronize(st));
    for (int q = 0; q < 4; ++q) hist_out[q] = (uint64_t)t->h_op->hist[q];
    return MEE_OK;
}
int mee_status(const mee_table* t, uint32_t* bits_out, void* stream) {
    MEE_RANGE("mee_status");
    if (!t || !bits_out) return fail(MEE_ERR_INVALID_ARG, "mee_status: null argument");
    if (int rc = read_counters(t, stream)) return rc;
    *bits_out = t->h_ctr->status;
    return MEE_OK;
}
int mee_clear_status(mee_table* t, void* stream) {
    MEE_RANGE("mee_clear_status");
    if (!t) return fail(MEE_ERR_INVALID_ARG, "mee_clear_status: null table");
    DeviceGuard g(t->device);
    zero_words(&t->ctr->status, sizeof(uint32_t), as_stream(stream));
    return MEE_OK;
}


}  // extern "C"
