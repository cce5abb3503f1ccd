"""No GPU: what the lookup operators of table.py / tiered.py / sharded.py hand to the LIBRARY — every mee_* call in order, its scalar arguments and, for
every pointer argument, which tensor it is — pinned for each operator with and without caller buffers, at fp32 and bf16, with each optional argument,
at n == 0 and at zero bags; so that a change of the Python layer that is meant to leave behaviour alone can show it.  And the refusals: a caller's
result buffer that is too small, of another dtype, not contiguous or on another device is refused before anything reaches the library.

The library is a recording stand-in that returns 0; the objects are made with __new__ on torch.device("cpu").  A tensor is named by the role the
test passed it in as ("keys", "out", ...); a tensor the operator allocated itself is recorded by dtype and shape.  The expected transcripts are
data: tests/golden/table_call_transcripts.json, written by `python tests/test_table_transcripts.py --record`.

Not run under the stub (they are no lookups, or need more than a handle): the constructors, export / evict / move_to / reserve (they read counts
back from the device), the optimizer steps other than MixedTableGroup.apply_pooled (its buffers share the lookups' rule), the host-logic sharded
classes (they need torch.distributed), the tiered classes over tiers that are not native tables (they call no library; tests/test_tiered*.py)."""
import contextlib
import ctypes as C
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "table_call_transcripts.json")
DIM = 8
CPU = torch.device("cpu")
F32, BF16, U8, I64, I32 = torch.float32, torch.bfloat16, torch.uint8, torch.int64, torch.int32


# ---- the stand-in for the library ------------------------------------------------------------------------------------------------------
class _Ptr(int):
    """what data_ptr() returns under the stub: the address, and the tensor it came from"""
    tensor = None


class _H(str):
    """a handle with a name; false, so that no __del__ hands it to the real library"""
    def __bool__(self):
        return False


class Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


_real_data_ptr = torch.Tensor.data_ptr


def _tracked_data_ptr(self):
    p = _Ptr(_real_data_ptr(self))
    p.tensor = self
    return p


@contextlib.contextmanager
def stubbed():
    from meepoembedding_amd import _lib
    from meepoembedding_amd import table as tm
    rec = Recorder()
    saved = (_lib.lib, tm._stream_ptr)
    _lib.lib, tm._stream_ptr = (lambda: rec), (lambda device: 0)
    torch.Tensor.data_ptr = _tracked_data_ptr
    try:
        yield rec
    finally:
        _lib.lib, tm._stream_ptr = saved
        del torch.Tensor.data_ptr


def _dt(d):
    return str(d).replace("torch.", "")


def _same(t, r):
    if t is r or t._base is r or (r._base is not None and (t is r._base or t._base is r._base)):
        return True
    a = _real_data_ptr(t)
    return a != 0 and a == _real_data_ptr(r) and t.dtype == r.dtype


def _tensor_id(t, roles, fresh):
    """the role's name, or for a tensor the operator made itself: dtype, shape and its number among those, in order of first appearance"""
    for name, r in roles.items():
        if isinstance(r, torch.Tensor) and _same(t, r):
            return name if t.numel() == r.numel() else f"{name}[{t.numel()} of {r.numel()}]"
    k = next((j for j, f in enumerate(fresh) if _same(t, f)), len(fresh))
    if k == len(fresh):
        fresh.append(t)
    return {"fresh": [_dt(t.dtype), list(t.shape), k]}


def _describe(a, roles, fresh):
    if a is None or isinstance(a, (bool, float, _H)):
        return a
    if isinstance(a, _Ptr):
        return _tensor_id(a.tensor, roles, fresh)
    if isinstance(a, int):
        return a
    if isinstance(a, (str, bytes)):
        return str(a)
    if isinstance(a, C.Array) and a._type_.__name__ == "FindRequest":
        by_ptr = {_real_data_ptr(r): name for name, r in roles.items() if isinstance(r, torch.Tensor) and r.numel()}
        return [[by_ptr.get(q.d_keys, "fresh"), q.n, by_ptr.get(q.d_out, "fresh"), by_ptr.get(q.d_found, "fresh")] for q in a]
    return type(a).__name__   # (byref of a count the stub never writes)


def _returned(x, roles, fresh, into):
    if isinstance(x, (tuple, list)):
        for y in x:
            _returned(y, roles, fresh, into)
    elif isinstance(x, torch.Tensor):
        who = _tensor_id(x, roles, fresh)
        into.append({"dtype": _dt(x.dtype), "shape": list(x.shape), "is": who if isinstance(who, str) else f"fresh {who['fresh'][2]}"})
    else:
        into.append(x)
    return into


# ---- the objects ---------------------------------------------------------------------------------------------------------------------------
def _table(name, dim=DIM, admission=False):
    from meepoembedding_amd import LookupTable
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim, t.value_dtype, t.layout_epoch = _H(name), CPU, dim, F32, 0
    t.max_batch, t.capacity, t.track_hits, t.optimizer, t.default_value = 1 << 20, 1 << 10, True, 1, 0.0
    t._opts = {"admission": admission}
    return t


def _group(name, tables):
    from meepoembedding_amd import TableGroup
    g = TableGroup.__new__(TableGroup)
    g._h, g.tables, g.device, g.dim, g.value_dtype, g._min_count_cache = _H(name), tables, CPU, tables[0].dim, F32, {}
    return g


def _mixed():
    from meepoembedding_amd import MixedTableGroup
    g = MixedTableGroup.__new__(MixedTableGroup)
    g.tables = [_table("m0", DIM), _table("m1", 2 * DIM)]
    g._h, g.device, g.dims = _H("mixed"), CPU, [DIM, 2 * DIM]
    return g


def _pair(j=0):
    from meepoembedding_amd import TieredLookupTable
    p = TieredLookupTable.__new__(TieredLookupTable)
    p.hot, p.cold, p.dim = _table(f"hot{j}", admission=True), _table(f"cold{j}"), DIM
    p.supports_pooled_out_dtype, p.optimizer, p.hot_key_limit, p._hot_keys_ub, p.policy = True, 1, 768, 0, True
    p.sample_every, p.promote_threshold, p._calls, p.rebalance_every, p._train_steps = 2, 2, 0, 0, 0
    return p


def _tiered_group():
    from meepoembedding_amd import TieredTableGroup
    g = TieredTableGroup.__new__(TieredTableGroup)
    g.tables = [_pair(0), _pair(1)]
    g.dim, g.policy, g.optimizer, g.sample_every, g._calls, g._native = DIM, True, 1, 2, 0, True
    g.hot_group, g.cold_group = _group("hot_group", [p.hot for p in g.tables]), _group("cold_group", [p.cold for p in g.tables])
    g._goes_cold, g._d_goes_cold = [False, False], torch.zeros(2, dtype=U8)
    return g


def _router():
    from meepoembedding_amd import Router
    r = Router.__new__(Router)
    r._h, r.device, r.n_shards, r.max_batch = _H("router"), CPU, 2, 1 << 10
    return r


def _rccl():
    from meepoembedding_amd import _lib
    from meepoembedding_amd.sharded import RcclShardedTable
    t = RcclShardedTable.__new__(RcclShardedTable)
    t._lib, t._check, t._C, t._h, t._comm, t.device, t.dim = _lib, _lib.check, C, _H("sharded"), None, CPU, DIM
    t._s = lambda: 0
    return t


MAKE = {"table": lambda: _table("table", admission=True), "group": lambda: _group("group", [_table("g0", admission=True), _table("g1", admission=True)]),
        "mixed": _mixed, "pair": _pair, "tgroup": _tiered_group, "router": _router, "rccl": _rccl}


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
class Shape:
    """one batch: n keys, the bags of one table, the bags and the segments of a group of two members"""
    def __init__(self, name, n, bags, group_bags, offsets, member_bags):
        self.name, self.n = name, n
        self.keys = torch.arange(10, 10 + n, dtype=I64)
        self.bags, self.group_bags, self.offsets, self.member_bags = (torch.tensor(x, dtype=I64) for x in (bags, group_bags, offsets, member_bags))
        self.nb, self.gnb = len(bags) - 1, len(group_bags) - 1
        self.bpt = self.gnb // 2


SHAPES = [Shape("n6", 6, [0, 2, 6], [0, 1, 3, 4, 6], [0, 2, 6], [0, 1, 4]),
          Shape("n0", 0, [0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0], [0, 1, 4]),
          Shape("nobags", 0, [0], [0], [0, 0, 0], [0, 0, 0])]


def _find_many(obj, keys, out=None, found=None):
    return obj.find_many([keys, (keys, out, found)])


def _cases(s):
    """-> (id, object kind, method name or callable, arguments, {caller-buffer role: (dtype, shape)}) for one Shape.  `out` follows out_dtype."""
    n, nb, gnb, bpt, D = s.n, s.nb, s.gnb, s.bpt, DIM
    rows = lambda dt=F32: {"out": (dt, (n, D)), "found": (U8, (n,))}
    bf = {"out_dtype": BF16}

    def variants(kind, method, base, bufs, *vs, name=None):
        for v in vs:
            v = dict(v)
            extra = v.pop("_bufs", {})
            b = {**bufs, **extra}
            if v.get("out_dtype") == BF16 and "out" in b:
                b["out"] = (BF16, b["out"][1])
            tag = ",".join(f"{k}={_dt(x) if isinstance(x, torch.dtype) else x}" for k, x in v.items() if not isinstance(x, torch.Tensor))
            tag += "".join(f",{k}" for k, x in v.items() if isinstance(x, torch.Tensor)) + "".join(f",+{r}" for r in extra if r != "out")
            yield f"{kind}.{name or method}({tag.strip(',')})@{s.name}", kind, method, {**base, **v}, b

    w = torch.ones(n)
    loc = {"_bufs": {"located": (I64, (n,))}}
    idx = {"_bufs": {"step_index": (I32, (n,))}}
    k = {"keys": s.keys}
    # one table
    yield from variants("table", "find", k, rows(), {}, {"flags": 3}, {"unordered": True}, bf, {"want_found": False})
    yield from variants("table", _find_many, k, rows(), {}, name="find_many")
    pooled = {"out": (F32, (nb, D)), "found": (U8, (n,))}
    kb = {"keys": s.keys, "bag_offsets": s.bags}
    yield from variants("table", "find_pooled", kb, pooled, {}, {"mode": "mean"}, {"weights": w}, {"weights": w, **loc}, bf, {"weights": w, **bf},
                        {"weights": w, **bf, **loc}, {"mode": "max"}, {"mode": "max", **bf})
    am = {"_bufs": {"argmax": (I32, (nb, D))}}
    yield from variants("table", "find_pooled_max", kb, pooled, {}, {"with_argmax": True}, am, bf)
    yield from variants("table", "pooled_max_backward", {"bag_offsets": s.bags, "argmax": torch.zeros((nb, D), dtype=I32), "bag_grads": torch.zeros(nb, D), "n": n},
                        {"grads": (F32, (n, D))}, {})
    padded = {"out": (F32, (nb, 3, D)), "found": (U8, (n,))}
    pad_vs = ({}, {"keep": "last"}, {"with_step": True}, bf)
    yield from variants("table", "find_padded", {**kb, "max_len": 3}, padded, *pad_vs)
    wb = {"grads": (F32, (n, D)), "weight_grads": (F32, (n,))}
    yield from variants("table", "pooled_weighted_backward", {**kb, "weights": w, "bag_grads": torch.zeros(nb, D)}, wb, {}, {"located": torch.zeros(n, dtype=I64)},
                        {"want_weight_grads": False})
    yield from variants("table", "find_missing", k, rows(), {})
    yield from variants("table", "find_or_insert_missing", k, rows(), {})
    yield from variants("table", "insert_missing", {**k, "values": torch.zeros(n, D)}, {"found": (U8, (n,))}, {})
    yield from variants("table", "find_counted", k, rows(), {}, {"missing_only": True})
    yield from variants("table", "find_or_insert", k, rows(), {}, {"min_count": 2}, bf)
    located = {**rows(), "slots": (I64, (n,))}
    for m in ("find_located", "find_or_insert_located"):
        yield from variants("table", m, k, located, {}, {"prepare_apply": True}, bf, {"prepare_apply": True, **bf})
    # a group of two tables
    ko = {"keys": s.keys, "offsets": s.offsets}
    gb = {"keys": s.keys, "bag_offsets": s.group_bags}
    yield from variants("group", "find", ko, rows(), {}, bf)
    yield from variants("group", "find_or_insert", ko, rows(), {}, bf, {"min_count": 2}, {"min_count": (1, 2)}, {"min_count": 2, **bf})
    gpooled = {"out": (F32, (gnb, D)), "found": (U8, (n,))}
    keyed = {"layout": "keyed", "_bufs": {"out": (F32, (bpt, 2 * D))}}
    yield from variants("group", "find_pooled", gb, gpooled, {}, {"mode": "mean"}, loc, {"weights": w}, {"weights": w, **loc}, bf, {"weights": w, **bf}, {**bf, **loc},
                        keyed, {**keyed, "mode": "mean"}, {**keyed, "_bufs": {**keyed["_bufs"], **idx["_bufs"], **loc["_bufs"]}}, {**keyed, **bf},
                        {"mode": "max"})
    yield from variants("group", "find_pooled_max", gb, gpooled, {}, {"with_argmax": True}, {"_bufs": {"argmax": (I32, (gnb, D))}}, bf)
    yield from variants("group", "pooled_max_backward", {"bag_offsets": s.group_bags, "argmax": torch.zeros((gnb, D), dtype=I32), "bag_grads": torch.zeros(gnb, D), "n": n},
                        {"grads": (F32, (n, D))}, {})
    yield from variants("group", "find_padded", {**gb, "max_len": 3}, {"out": (F32, (gnb, 3, D)), "found": (U8, (n,))}, *pad_vs)
    jag = {"keys": s.keys, "bag_offsets": s.group_bags, "member_bags": s.member_bags}
    yield from variants("group", "find_pooled_jagged", jag, gpooled, {}, {"mode": "mean"}, loc)
    yield from variants("group", "pooled_weighted_backward", {**gb, "weights": w, "bag_grads": torch.zeros(gnb, D)}, wb, {}, {"located": torch.zeros(n, dtype=I64)},
                        {"want_weight_grads": False})
    # a group of two tables of dims D and 2 D
    total = bpt * 3 * D
    mpooled = {"out": (F32, (total,)), "found": (U8, (n,))}
    mkeyed = {"layout": "keyed", "_bufs": {"out": (F32, (bpt, 3 * D))}}
    yield from variants("mixed", "find_pooled", gb, mpooled, {}, {"mode": "mean"}, loc, {"insert_missing": True}, bf, {**bf, **loc}, mkeyed,
                        {**mkeyed, "insert_missing": True, "_bufs": {**mkeyed["_bufs"], **idx["_bufs"], **loc["_bufs"]}}, {**mkeyed, **bf})
    yield from variants("mixed", "apply_pooled", {**gb, "bag_grads": torch.zeros(total), "bag_of_position": torch.zeros(n, dtype=I32), "optimizer": "adagrad", "lr": 0.5},
                        {}, {}, loc)
    # a hot/cold pair of native tables
    yield from variants("pair", "find", k, {}, {})
    yield from variants("pair", "find_or_insert", k, {}, {}, {"min_count": 2})
    creating = ({"insert_missing": True}, {"insert_missing": True, "min_count": 2})
    yield from variants("pair", "find_pooled", kb, pooled, {}, {"mode": "mean"}, *creating, bf)
    yield from variants("pair", "find_padded", {**kb, "max_len": 3}, padded, *pad_vs)
    # a group of two pairs
    yield from variants("tgroup", "find", ko, rows(), {}, bf)
    yield from variants("tgroup", "find_or_insert", ko, rows(), {}, bf, {"min_count": 2}, {"min_count": (1, 2)})
    yield from variants("tgroup", "find_pooled", gb, gpooled, {}, {"mode": "mean"}, *creating, {"insert_missing": True, "min_count": (1, 2)}, bf, keyed,
                        {**keyed, "_bufs": {**keyed["_bufs"], **idx["_bufs"]}}, {**keyed, "insert_missing": True}, {**keyed, "insert_missing": True, "min_count": 2},
                        {**keyed, **bf})
    yield from variants("tgroup", "find_padded", {**gb, "max_len": 3}, {"out": (F32, (gnb, 3, D)), "found": (U8, (n,))}, *pad_vs)
    yield from variants("tgroup", "find_pooled_jagged", jag, gpooled, {}, {"mode": "mean"})
    # the sharded classes that call the library themselves
    runs = {"partials": torch.zeros(3, D), "run_bag": torch.zeros(3, dtype=I32), "run_counts": torch.zeros(2, dtype=I64), "bag_offsets": s.bags}
    yield from variants("router", "combine_bag_runs", runs, {"out": (F32, (nb, D))}, {}, {"mode": "mean"}, bf)
    for m in ("find", "find_or_insert"):
        yield from variants("rccl", m, k, rows(), {}, bf)


# keys without bags are refused by these (there is no bag to report them): their n == 0 / zero-bag forms still run
def all_cases():
    for s in SHAPES:
        yield from _cases(s)


def _run(kind, method, args, buffers):
    """one call under the stub -> (transcript, the recorder, the object)"""
    with stubbed() as rec:
        obj = MAKE[kind]()
        roles = {**{name: v for name, v in args.items() if isinstance(v, torch.Tensor)}, **buffers}
        if kind == "tgroup":
            roles["goes_cold"] = obj._d_goes_cold
        fn = getattr(obj, method) if isinstance(method, str) else (lambda **kw: method(obj, **kw))
        ret = fn(**args, **buffers)
        fresh = []
        calls = [[name, [_describe(a, roles, fresh) for a in a_]] for name, a_ in rec.calls]
        t = {"calls": calls, "returns": _returned(ret, roles, fresh, [])}
        if hasattr(obj, "_calls"):
            t["policy_calls"] = obj._calls
        return t


def _make(bufs):
    return {name: torch.empty(shape, dtype=dt) for name, (dt, shape) in bufs.items()}


REQUIRED = ("find_missing", "find_or_insert_missing", "insert_missing")   # their buffers are no option


def _transcripts():
    out = {}
    for cid, kind, method, args, bufs in all_cases():
        assert cid not in out and cid + "+buffers" not in out, f"two cases named {cid}"
        if method not in REQUIRED:
            out[cid] = _run(kind, method, args, {})
        if bufs:
            out[cid + "+buffers"] = _run(kind, method, args, _make(bufs))
    return out


def test_operators_call_the_library_as_recorded(built):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(_transcripts()))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], f"{name}:\n got      {got[name]}\n expected {want[name]}"


def test_every_lookup_operator_has_cases(built):
    """the omissions are the ones the docstring names: every public find* / pooled_* method of the five classes is driven"""
    from meepoembedding_amd import LookupTable, MixedTableGroup, TableGroup, TieredLookupTable, TieredTableGroup
    driven = {(kind, m if isinstance(m, str) else m.__name__.lstrip("_")) for _, kind, m, _, _ in all_cases()}
    skipped = {("table", "find_capture_stats"), ("table", "find_plane")}   # a counter read-back; a lookup without caller buffers or options (locate's sibling)
    for kind, cls in (("table", LookupTable), ("group", TableGroup), ("mixed", MixedTableGroup), ("pair", TieredLookupTable), ("tgroup", TieredTableGroup)):
        for name in dir(cls):
            if (name.startswith("find") or name.startswith("pooled_")) and callable(getattr(cls, name)):
                assert (kind, name) in driven or (kind, name) in skipped, f"{cls.__name__}.{name} has no transcript case"


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _wrong(dt, shape):
    numel = 1
    for d in shape:
        numel *= d
    other = {F32: torch.float64, BF16: torch.float16, U8: torch.int8, I64: torch.int32, I32: torch.int16}[dt]
    return {"short": torch.empty(numel - 1, dtype=dt), "dtype": torch.empty(shape, dtype=other),
            "strided": torch.empty(2 * numel, dtype=dt)[::2], "device": torch.empty(shape, dtype=dt, device="meta")}


def test_wrong_result_buffers_are_refused_before_any_call(built):
    """every operator x every caller-buffer role x (one element short, wrong dtype, non-contiguous with the right count, wrong device) ->
    MeepoError(ERR_INVALID_ARG), nothing reached the library, a pair's or tiered group's policy counter did not move.
    Two exceptions, both by the operators' own order of refusals: an `out` of another dtype is refused by the out_dtype check in front
    (ValueError, as before); the `out` of layout="keyed" follows the strided 2-D rule of the keyed block, which has tests of its own."""
    from meepoembedding_amd import _lib
    failures, tried = [], 0
    for cid, kind, method, args, bufs in _cases(SHAPES[0]):
        for role, (dt, shape) in bufs.items():
            if role == "out" and args.get("layout") == "keyed":
                continue
            for what, bad in _wrong(dt, shape).items():
                tried += 1
                with stubbed() as rec:
                    obj = MAKE[kind]()
                    fn = getattr(obj, method) if isinstance(method, str) else (lambda method=method, obj=obj, **kw: method(obj, **kw))
                    try:
                        fn(**args, **{**_make(bufs), role: bad})
                        failures.append(f"{cid}: {role} {what}: accepted, calls {[c[0] for c in rec.calls]}")
                    except _lib.MeepoError as e:
                        if e.code != _lib.ERR_INVALID_ARG:
                            failures.append(f"{cid}: {role} {what}: MeepoError code {e.code}")
                    except ValueError as e:
                        if not (role == "out" and what == "dtype"):
                            failures.append(f"{cid}: {role} {what}: ValueError {e}")
                    except Exception as e:  # noqa: BLE001
                        failures.append(f"{cid}: {role} {what}: {type(e).__name__} {e}")
                    if rec.calls:
                        failures.append(f"{cid}: {role} {what}: the library saw {[c[0] for c in rec.calls]}")
                    if getattr(obj, "_calls", 0) != 0 or any(getattr(p, "_calls", 0) for p in getattr(obj, "tables", [])):
                        failures.append(f"{cid}: {role} {what}: the policy counted the refused call")
    assert tried > 400
    assert not failures, f"{len(failures)} of {tried}:\n" + "\n".join(failures[:60])


BAD_MODE = [("table", "find_pooled", "bags", ValueError), ("group", "find_pooled", "group_bags", "MeepoError"), ("group", "find_pooled_keyed", "group_bags", "MeepoError"),
            ("group", "find_pooled_jagged", "group_bags", "MeepoError"), ("mixed", "find_pooled", "group_bags", "MeepoError"), ("pair", "find_pooled", "bags", ValueError),
            ("tgroup", "find_pooled", "group_bags", ValueError), ("tgroup", "find_pooled_jagged", "group_bags", "MeepoError")]


@pytest.mark.parametrize("kind,method,bags,error", BAD_MODE, ids=[f"{k}.{m}" for k, m, _, _ in BAD_MODE])
def test_a_bad_mode_is_refused_before_anything_is_allocated(built, kind, method, bags, error):
    from meepoembedding_amd import _lib
    s = SHAPES[0]
    kw = {"member_bags": s.member_bags} if method.endswith("jagged") else {"layout": "keyed"} if method.endswith("keyed") else {}
    with stubbed() as rec:
        obj = MAKE[kind]()
        with pytest.raises(_lib.MeepoError if error == "MeepoError" else error, match="mode must be 'sum' or 'mean'") as e:
            getattr(obj, method.replace("_keyed", ""))(s.keys, getattr(s, bags), mode="min", **kw)
        assert error != "MeepoError" or e.value.code == _lib.ERR_INVALID_ARG
        assert rec.calls == [] and getattr(obj, "_calls", 0) == 0


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(GOLDEN, "w") as f:
            json.dump(_transcripts(), f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")
