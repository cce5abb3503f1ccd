"""CPU: the host's decision in front of every partition — buckets, hot-key buckets, partition blocks, apply grid, LEAN or FULL — is one pure
function (part_plan_for, csrc/meepo_apply_part.h).  tests/cabi/part_plan_test.cpp, compiled host-only, runs it over tests/golden/part_plan.txt: every
field of every plan must equal what the arithmetic gave before it was moved into that function (the rows were recorded from the commit before, through
the same host-only compile).  The table is no full cross product; it holds
  - every state of the stream (0 / 1 / 146 / 768 units reported by the previous batch x capturing x sticky x apply_kernel -1 / 0 / 1) at n = 262144 on 768 block slots;
  - every n in {1, 127, 129, 30000, 98304, 98305, 262144, 1048576, 5000000}: uniform, behind a skewed batch, capturing; and on 312 block slots (104 CUs);
  - apply_bucket_max 0 / 128 / 352 with n_buckets_max sized for max_batch 262144 and 5000000 (the small one with the large n is the knob's out-of-bounds case);
  - the training forward's partition (256 threads) and the dedup consumers' own geometry (6 and 5 blocks per CU, buckets of 683);
  - apply_kernel and the sticky counter at n = 30000 and n = 5000000."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "part_plan.txt")
COLUMNS = ("n threads slots bucket_max n_buckets_max prev_units capturing sticky kernel_choice slots_of bucket_max_of "
           "nbk_hash nbk grid full blocks per_block totals_by_atomics").split()


def _rows():
    with open(GOLDEN) as f:
        return [dict(zip(COLUMNS, map(int, line.split()))) for line in f if line.strip()]


def _one(rows, **inputs):
    base = dict(threads=1024, slots=768, bucket_max=0, prev_units=0, capturing=0, sticky=0, kernel_choice=-1, slots_of=0, bucket_max_of=0)
    base.update(inputs)
    hits = [r for r in rows if all(r[k] == v for k, v in base.items())]
    assert len(hits) == 1, (base, len(hits))
    return hits[0]


def test_table_holds_the_rows_derived_by_hand():
    """Anchors against a recording mistake: plans that follow from the documented rules alone (768 slots, buckets of up to 352)."""
    rows = _rows()
    r = _one(rows, n=262144, n_buckets_max=7808)            # one round of the block slots
    assert (r["nbk_hash"], r["nbk"], r["grid"], r["full"]) == (768, 768, 768, 0)
    r = _one(rows, n=1048576, n_buckets_max=7808)           # ceil(1048576 / (768 x 352)) = 4 rounds
    assert (r["nbk_hash"], r["nbk"]) == (3072, 3072)
    r = _one(rows, n=30000, n_buckets_max=7808)             # fewer keys than 768 x 128: buckets of 128
    assert (r["nbk_hash"], r["nbk"]) == (235, 235)
    r = _one(rows, n=262144, n_buckets_max=896, prev_units=146)   # 768 - (146 + 146 / 16 + 1) hash buckets, kHotCap hot buckets
    assert (r["nbk_hash"], r["nbk"], r["grid"], r["full"]) == (612, 612 + 128, 768, 1)
    # every axis is there
    for col, values in (("n", {1, 127, 129, 30000, 98304, 98305, 262144, 1048576, 5000000}), ("slots", {768, 312}), ("capturing", {0, 1}), ("sticky", {0, 1}),
                        ("kernel_choice", {-1, 0, 1}), ("bucket_max", {0, 128, 352}), ("threads", {1024, 256}), ("slots_of", {0, 1536, 1280, 624, 520}), ("bucket_max_of", {0, 683})):
        assert {r[col] for r in rows} == values, col
    assert {r["prev_units"] for r in rows if r["slots"] == 768} == {0, 1, 146, 768}


def test_part_plan_for_matches_recorded_plans():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(ROOT, "build", "part_plan")
    os.makedirs(out, exist_ok=True)
    obj, exe = os.path.join(out, "part_plan_test.o"), os.path.join(out, "part_plan_test")
    subprocess.check_call([hipcc, "--cuda-host-only", "-std=c++17", "-O1", "-fPIC", "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "meepoembedding_amd", "csrc"),
                           "-c", os.path.join(ROOT, "tests", "cabi", "part_plan_test.cpp"), "-o", obj])
    subprocess.check_call(["g++", obj, "-o", exe])   # (no HIP call in it: nothing to link against)
    r = subprocess.run([exe, GOLDEN], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "part_plan_test ok: 173 rows" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
