"""Search (SPEC.md §3 "Search"): LookupTable.search against what a user ran before it, on one MI355X.  Numbers go to profiles/search.md.

Per shape the two paths take turns inside ONE timing loop, in chunks of 5 calls between device events; the whole sequence runs twice and the spread of
a row is its pass-to-pass difference (the method of profiles/int8_rows.md).
    search            table.search(queries, k): one mee_search call inside the per-call limits, one mee_search_batch call (tiled queries, seed pass,
                      seeded main scan, merge) past them
    NAME              --libs NAME=PATH,…: the same table searched through ANOTHER build of the library, loaded beside this one — the parent commit's
                      (no mee_search_batch: the batch is split into mee_search calls by the per-call limits, as its Python layer did) or a build of
                      this tree with another seed divisor or tile rule (-DMEE_SEARCH_SEED_DIV=…, -DMEE_SEARCH_TILE_MAX_QUERIES=32).  With --metric cosine the
                      row goes through that build's mee_search_metric; with --exclude it becomes "NAME filtered" and "NAME filtered shared", through its
                      mee_search_filtered.  Naming one build twice (parent=P,parent2=P) gives a row's noise floor: the same code against itself;
                      naming this tree's own library too (tree=…) times like against like: the rows above go through LookupTable.search (a workspace
                      query and result allocations per call), a NAME row through bare calls on buffers the tool holds
    matmul + topk     on a PREBUILT [N, dim] bf16 matrix of the same table: queries.bfloat16() @ M.T, torch.topk, keys[positions]
    refresh           building that matrix — export() and the cast to bf16 — timed once and reported apart: the cost the matrix path pays after every
                      publish, and the second copy of the table it keeps
--metric cosine adds two rows and changes one (profiles/search.md "Metric"):
    cosine            table.search(queries, k, metric="cosine"): mee_search_metric, the batched launches for every Q
    ip same launches  mee_search_batch called directly for every Q: the inner product through the very launches the cosine takes — what the norm costs
    matmul + topk     the matrix is the NORMALISED bf16 matrix (rows / |row|), the queries are normalised per call; refresh includes the normalisation
--exclude E,… replaces the rows by the exclusion measurement (profiles/search.md "Exclusion"), one record per E; the exclude rows are each query's own top
E scorers (read off the matrix), the case in which the filter is asked most often:
    search            the unfiltered search of the same shape, in the same loop
    filtered          table.search(queries, k, exclude=[Q, E]): mee_search_filtered — the sort of the rows and the filtered launches
    filtered shared   the same with one [1, E] row (query 0's) for every query
    overfetch+filter  only where k + E <= 64: table.search(queries, k + E) and the filter in torch (compare, stable argsort, gather)
--group T replaces the rows by the grouped measurement (profiles/search.md "Groups"): `group`, one TableGroup.search over T tables of --keys keys, and
`loop`, the T table.search calls it stands for.
usage: python tools/search_bench.py [--group T] [--metric ip|cosine] [--exclude 54,64,4096] [--keys N] [--dim D] [--reps K] [--queries 1,32,128,1024] [--ks 10,64] [--libs parent=PATH,…] [--no-matmul]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from meepoembedding_amd import LookupTable, _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--keys", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--queries", default="1,32,128,1024")
ap.add_argument("--ks", default="10,64", help="one Q and one k: a shape on its own for `rocprofv3 --kernel-trace --stats`, which times the scan and the merge apart")
ap.add_argument("--libs", default="", help="NAME=PATH,…: other builds of the library, each a row of its own")
ap.add_argument("--metric", default="ip", choices=["ip", "cosine"])
ap.add_argument("--exclude", default="", help="E,…: time search(exclude=...) with each query's top E scorers excluded against the unfiltered search")
ap.add_argument("--no-matmul", action="store_true", help="leave the matrix path out (a kernel trace of the search alone)")
ap.add_argument("--group", type=int, default=0, help="T: time TableGroup.search over T tables of --keys keys each against the loop of T table.search calls, and nothing else")
args = ap.parse_args()
dev = torch.device("cuda", 0)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
PEAK = 8e12   # bytes / s


def timed_rows(rows, reps, chunk=5):
    names = list(rows)
    for nm in names:
        for _ in range(3):
            rows[nm]()
    torch.cuda.synchronize()
    total = dict.fromkeys(names, 0.0)
    for _ in range(reps // chunk):
        for nm in names:
            ev[0].record()
            for _ in range(chunk):
                rows[nm]()
            ev[1].record()
            torch.cuda.synchronize()
            total[nm] += ev[0].elapsed_time(ev[1]) * 1e3
    return {nm: total[nm] / (reps // chunk * chunk) for nm in names}


def group_mode():
    """--group T (profiles/search.md "Groups"): T tables of --keys keys each at load 0.75, fp32 rows and bf16 rows; `group` = TableGroup.search(queries
    [T, Q, dim], k), three launches, and `loop` = T LookupTable.search(queries[j], k) calls — this tree's single-table path — take turns in one timing
    loop, two passes.  Both are checked equal before they are timed."""
    from meepoembedding_amd import TableGroup
    for value_dtype in (torch.float32, torch.bfloat16):
        tables = [LookupTable(int(args.keys / 0.75), args.dim, device=dev, max_batch=1 << 20, value_dtype=value_dtype) for _ in range(args.group)]
        for t in tables:
            bench.populate(t, synth, args.keys, args.dim, dev, 1 << 20)
        group = TableGroup(tables)
        steps = sum((t.capacity + 31) // 32 for t in tables)
        for nq in [int(x) for x in args.queries.split(",")]:
            queries = torch.randn(args.group, nq, args.dim, device=dev)
            for k in [int(x) for x in args.ks.split(",")]:
                rows = {"group": lambda: group.search(queries, k, metric=args.metric),
                        "loop": lambda: [t.search(queries[j], k, metric=args.metric) for j, t in enumerate(tables)]}
                got = group.search(queries, k, metric=args.metric)
                for j, (lk, ls) in enumerate(rows["loop"]()):
                    assert torch.equal(got[0][j], lk) and torch.equal(got[1][j].view(torch.int32), ls.view(torch.int32)), f"member {j}: group and table search disagree"
                passes = [timed_rows(rows, args.reps) for _ in range(2)]
                us = {nm: (passes[0][nm] + passes[1][nm]) / 2 for nm in rows}
                rec = {"group": args.group, "metric": args.metric, "rows": str(value_dtype).split(".")[1], "keys_per_table": tables[0].size(), "steps": steps, "dim": args.dim,
                       "Q": nq, "k": k, "us": {nm: round(v, 1) for nm, v in us.items()}, "spread_us": {nm: round(abs(passes[0][nm] - passes[1][nm]), 1) for nm in rows},
                       "loop_over_group": round(us["loop"] / us["group"], 2)}
                print("SEARCH_BENCH " + json.dumps(rec), flush=True)
        group.close()
        for t in tables:
            t.close()
        torch.cuda.empty_cache()


if args.group:
    group_mode()
    sys.exit(0)

WIDE = args.dim > 256   # mee_search has no such row: every Q is ONE mee_search_batch call (DESIGN.md §4 "Search", "Wide rows"); no split-call row


def per_call_limit(k):
    if WIDE:
        return 0
    return min(_lib.SEARCH_MAX_QK // max(k, 8), _lib.SEARCH_MAX_QUERY_ELEMS // args.dim // 32 * 32)


def other_build(path):
    """-> search(t, queries, k, metric="ip", exclude=None) through the library at `path`, on the handle of this process's table (the table layout is the
    same in every build named above): its mee_search_batch past the per-call limits if it has one, split mee_search calls otherwise; metric="cosine"
    and exclude=[Q or 1, E] as ONE call of its mee_search_metric / mee_search_filtered, as table.search makes it at the shapes timed here; buffers and
    workspace allocated once per shape"""
    L = C.CDLL(path)
    names = [nm for nm in _lib.PROTOTYPES if nm.startswith("mee_search") and hasattr(L, nm)]
    for nm in names:
        getattr(L, nm).restype, getattr(L, nm).argtypes = _lib.PROTOTYPES[nm]
    held = {}

    def search(t, queries, k, metric="ip", exclude=None):
        nq, step = queries.shape[0], per_call_limit(k)
        batched = nq > step and "mee_search_batch" in names
        if batched:
            step = _lib.SEARCH_BATCH_MAX_QUERIES
        shape = (nq, k, metric, None if exclude is None else tuple(exclude.shape))
        if shape not in held:
            need = C.c_uint64()
            if exclude is not None:
                _lib.check(L.mee_search_filtered_workspace_bytes(t._h, _lib.METRICS[metric], nq, k, exclude.shape[0], exclude.shape[1], C.byref(need)))
            elif metric != "ip":
                _lib.check(L.mee_search_metric_workspace_bytes(t._h, _lib.METRICS[metric], nq, k, C.byref(need)))
            else:
                _lib.check((L.mee_search_batch_workspace_bytes if batched else L.mee_search_workspace_bytes)(t._h, min(nq, step), k, C.byref(need)))
            if any(key[:2] != shape[:2] for key in held):   # the rows of one (Q, k) take turns: their buffers stay
                held.clear()
            held[shape] = (torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, device=dev), torch.empty(need.value, dtype=torch.uint8, device=dev))
        ok, osc, ws = held[shape]
        if exclude is not None:
            _lib.check(L.mee_search_filtered(t._h, _lib.METRICS[metric], queries.data_ptr(), nq, k, exclude.data_ptr(), exclude.shape[0], exclude.shape[1], ok.data_ptr(),
                                             osc.data_ptr(), None, ws.data_ptr(), None))
            return ok, osc
        if metric != "ip":
            _lib.check(L.mee_search_metric(t._h, _lib.METRICS[metric], queries.data_ptr(), nq, k, ok.data_ptr(), osc.data_ptr(), None, ws.data_ptr(), None))
            return ok, osc
        for s in range(0, nq, step):
            n = min(step, nq - s)
            _lib.check((L.mee_search_batch if batched else L.mee_search)(t._h, queries[s:s + n].data_ptr(), n, k, ok[s:s + n].data_ptr(), osc[s:s + n].data_ptr(),
                                                                         None, ws.data_ptr(), None))
        return ok, osc
    return search


def same_launches(t, queries, k, held={}):
    """mee_search_batch called directly, whatever Q: the launches mee_search_metric takes, ranking by the inner product"""
    nq = queries.shape[0]
    if (nq, k) not in held:
        need = C.c_uint64()
        _lib.check(_lib.lib().mee_search_batch_workspace_bytes(t._h, nq, k, C.byref(need)))
        held.clear()
        held[nq, k] = (torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, device=dev), torch.empty(need.value, dtype=torch.uint8, device=dev))
    ok, osc, ws = held[nq, k]
    _lib.check(_lib.lib().mee_search_batch(t._h, queries.data_ptr(), nq, k, ok.data_ptr(), osc.data_ptr(), None, ws.data_ptr(), None))
    return ok, osc


others = {nm: other_build(path) for nm, path in (x.split("=") for x in args.libs.split(",") if x)}
results = []
for value_dtype in (torch.float32, torch.bfloat16):
    t = LookupTable(int(args.keys / 0.75), args.dim, device=dev, max_batch=1 << 21, value_dtype=value_dtype)
    bench.populate(t, synth, args.keys, args.dim, dev, 1 << 20)
    n = t.size()
    row_bytes = args.dim * (4 if value_dtype == torch.float32 else 2)
    scan_bytes = t.capacity * 8 + n * row_bytes   # what the scan asks for: the key plane and the live rows
    torch.cuda.synchronize()
    ev[0].record()
    ekeys, erows = t.export()[:2]
    matrix = (erows / erows.norm(dim=1, keepdim=True) if args.metric == "cosine" else erows).to(torch.bfloat16)
    ev[1].record()
    torch.cuda.synchronize()
    refresh_us = ev[0].elapsed_time(ev[1]) * 1e3
    del erows
    for nq in [int(x) for x in args.queries.split(",")]:
        queries = torch.randn(nq, args.dim, device=dev)
        for k in [int(x) for x in args.ks.split(",")]:
            def matmul_topk():
                qm = queries / queries.norm(dim=1, keepdim=True) if args.metric == "cosine" else queries
                pos = torch.topk(qm.to(torch.bfloat16) @ matrix.T, k, dim=1).indices
                return ekeys[pos]

            if args.exclude:
                qm = queries / queries.norm(dim=1, keepdim=True) if args.metric == "cosine" else queries
                top = ekeys[torch.topk(qm.to(torch.bfloat16) @ matrix.T, max(int(e) for e in args.exclude.split(",")), dim=1).indices]
                for ne in [int(e) for e in args.exclude.split(",")]:
                    ex = top[:, :ne].contiguous()
                    rows = {"search": lambda: t.search(queries, k, metric=args.metric), "filtered": lambda: t.search(queries, k, metric=args.metric, exclude=ex),
                            "filtered shared": lambda: t.search(queries, k, metric=args.metric, exclude=ex[:1])}
                    for nm, fn in others.items():
                        rows[nm + " filtered"] = lambda fn=fn: fn(t, queries, k, args.metric, ex)
                        rows[nm + " filtered shared"] = lambda fn=fn: fn(t, queries, k, args.metric, ex[:1])
                        assert torch.equal(rows[nm + " filtered"]()[0], rows["filtered"]()[0]) and torch.equal(rows[nm + " filtered shared"]()[0], rows["filtered shared"]()[0]), \
                            f"{nm} and this tree's filtered search disagree"
                    if k + ne <= _lib.SEARCH_MAX_K:
                        def overfetch():
                            wk, ws = t.search(queries, k + ne, metric=args.metric)
                            keep = ~(wk[:, :, None] == ex[:, None, :]).any(-1)
                            at = keep.to(torch.int8).argsort(dim=1, descending=True, stable=True)[:, :k]
                            return wk.gather(1, at), ws.gather(1, at)
                        rows["overfetch+filter"] = overfetch
                        assert torch.equal(overfetch()[0], rows["filtered"]()[0])
                    assert not torch.isin(rows["filtered"]()[0], ex[:1]).logical_and(torch.arange(nq, device=dev)[:, None] == 0).any()
                    passes = [timed_rows(rows, args.reps) for _ in range(2)]
                    rec = {"exclude": ne, "metric": args.metric, "rows": str(value_dtype).split(".")[1], "keys": n, "dim": args.dim, "Q": nq, "k": k,
                           "us": {nm: round((passes[0][nm] + passes[1][nm]) / 2, 1) for nm in rows}, "spread_us": {nm: round(abs(passes[0][nm] - passes[1][nm]), 1) for nm in rows}}
                    print("SEARCH_BENCH " + json.dumps(rec), flush=True)
                    results.append(rec)
                del top
                continue
            got = t.search(queries, k, metric=args.metric)[0]
            same = float((got == matmul_topk()).float().mean())   # (bf16 scores of the matrix path round differently: near-ties may swap)
            rows = {"search": lambda: t.search(queries, k)}
            if args.metric == "cosine":
                rows = {"cosine": lambda: t.search(queries, k, metric="cosine"), "ip same launches": lambda: same_launches(t, queries, k), **rows}
                assert torch.equal(same_launches(t, queries, k)[0], t.search(queries, k)[0])
            if not args.no_matmul:
                rows["matmul + topk"] = matmul_topk
            for nm, fn in others.items():   # (against the first row: "search", or "cosine")
                rows[nm] = lambda fn=fn: fn(t, queries, k, args.metric)
                assert torch.equal(fn(t, queries, k, args.metric)[0], got), f"{nm} and this tree's search disagree"   # exact by contract, whatever the build
            passes = [timed_rows(rows, args.reps) for _ in range(2)]
            us = {nm: (passes[0][nm] + passes[1][nm]) / 2 for nm in rows}
            # this tree: one call either way; past the limits every tile's blocks ask for the table (tiles that walk one range may meet in L2), in
            # four launches.  A build without the batch entry point: `split` calls of two launches, each a scan of the table.
            split = -(-nq // per_call_limit(k)) if not WIDE else 0
            tiles = -(-nq // min(per_call_limit(k), 32)) if not WIDE and nq > per_call_limit(k) else 1   # search_batch_tile: one row block at the most
            if WIDE:   # search_wide_tile: what 40 KB of LDS hold of rounded queries and candidate buffers, in eights, one row block at the most
                tiles = -(-nq // min((40 * 1024 - 768) // (args.dim * 2 + 2 * max(k, 8) * 12) // 8 * 8, 32))
            rec = {"metric": args.metric, "rows": str(value_dtype).split(".")[1], "keys": n, "dim": args.dim, "Q": nq, "k": k, "native_calls": 1, "launches": 4 if tiles > 1 or WIDE else 2,
                   "tiles": tiles, "split_native_calls": split, "split_launches": 2 * split,
                   "us": {nm: round(v, 1) for nm, v in us.items()}, "spread_us": {nm: round(abs(passes[0][nm] - passes[1][nm]), 1) for nm in rows},
                   "search_bytes": tiles * scan_bytes, "split_bytes": split * scan_bytes, "matmul_bytes": n * args.dim * 2 + 2 * nq * n * 2,
                   "search_fraction_of_8TBs": round(tiles * scan_bytes / (us["search"] * 1e-6) / PEAK, 3), "refresh_us": round(refresh_us, 1),
                   "refresh_extra_bytes": n * args.dim * 2, "keys_equal_fraction": round(same, 4)}
            print("SEARCH_BENCH " + json.dumps(rec), flush=True)
            results.append(rec)
    del matrix, ekeys
    t.close()
    torch.cuda.empty_cache()
print("SEARCH_BENCH_ALL " + json.dumps(results), flush=True)
