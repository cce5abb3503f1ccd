// part_plan_test.cpp — TEST INFRASTRUCTURE: the host's planning arithmetic in front of every partition (part_plan_for, csrc/meepo_apply_part.h) against recorded plans.
//
// usage: part_plan_test tests/golden/part_plan.txt.  One case per row: the inputs
//   n  threads  slots  bucket_max  n_buckets_max  prev_units  capturing  sticky  kernel_choice  slots_of  bucket_max_of
// and the plan they must give
//   nbk_hash  nbk  grid  full  blocks  per_block  totals_by_atomics
// The rows were recorded from bucket_count_for / part_geometry / bucket_totals_by_atomics of the commit BEFORE that arithmetic moved into part_plan_for (host-only
// compile, capture status and pinned word set per row), never from part_plan_for itself.  Host-only compile (hipcc --cuda-host-only), no GPU, no HIP call.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "meepo_apply_part.h"

int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "part_plan_test: cannot open the table of cases\n"); return 64; }
    unsigned long long n;
    unsigned threads, slots, bucket_max, n_buckets_max, prev, slots_of, bucket_max_of, e_hash, e_nbk, e_grid, e_blocks, e_per_block;
    int capturing, sticky, kernel_choice, e_full, e_atom, rows = 0, bad = 0;
    while (fscanf(f, "%llu %u %u %u %u %u %d %d %d %u %u %u %u %u %d %u %u %d", &n, &threads, &slots, &bucket_max, &n_buckets_max, &prev, &capturing, &sticky, &kernel_choice, &slots_of,
                  &bucket_max_of, &e_hash, &e_nbk, &e_grid, &e_full, &e_blocks, &e_per_block, &e_atom) == 18) {
        const mee::PartPlan p = mee::part_plan_for(n, threads, mee::PartInputs{slots, bucket_max, n_buckets_max, prev, capturing != 0, sticky != 0, kernel_choice, slots_of, bucket_max_of});
        ++rows;
        if (p.nbk_hash == e_hash && p.nbk == e_nbk && p.grid == e_grid && p.full == (e_full != 0) && p.blocks == e_blocks && p.per_block == e_per_block &&
            p.totals_by_atomics == (e_atom != 0)) continue;
        if (++bad <= 20)
            printf("row %d (n=%llu threads=%u slots=%u bucket_max=%u n_buckets_max=%u prev=%u capturing=%d sticky=%d kernel_choice=%d slots_of=%u bucket_max_of=%u): "
                   "plan %u %u %u %d %u %u %d, expected %u %u %u %d %u %u %d\n", rows, n, threads, slots, bucket_max, n_buckets_max, prev, capturing, sticky, kernel_choice, slots_of,
                   bucket_max_of, p.nbk_hash, p.nbk, p.grid, (int)p.full, p.blocks, p.per_block, (int)p.totals_by_atomics, e_hash, e_nbk, e_grid, e_full, e_blocks, e_per_block, e_atom);
    }
    const bool whole = feof(f) != 0;   // (a row that does not parse ends the loop early: not a pass)
    fclose(f);
    if (bad || !whole || !rows) { printf("part_plan_test FAILED: %d of %d rows differ%s\n", bad, rows, whole ? "" : ", table not read to its end"); return 1; }
    printf("part_plan_test ok: %d rows\n", rows);
    return 0;
}
