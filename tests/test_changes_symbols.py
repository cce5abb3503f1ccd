"""No GPU: the change log (SPEC.md §3 "Change log") as the library exports it and as the Python layer wires it — the ten entry points in the header,
the loader and the C++ wrappers; which methods of LookupTable and TableGroup note their batch, and that an untracked table issues no call it did not
issue before (a recording stand-in for the library); and the delta format of checkpoint.py over a dict-backed table."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mee_changes_clear", "mee_changes_create", "mee_changes_destroy", "mee_changes_group_create", "mee_changes_group_destroy", "mee_changes_group_note",
         "mee_changes_info_get", "mee_changes_invalidate", "mee_changes_note", "mee_export_changed"]
DIM = 8


def test_the_symbols(built):
    from meepoembedding_amd import _lib
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    assert sorted(set(re.findall(r"\bint\s+(mee_changes\w*|mee_export_changed)\(", header))) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1), flags=re.S)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    assert len(_lib.PROTOTYPES["mee_export_changed"][1]) == 13 and len(_lib.PROTOTYPES["mee_changes_group_note"][1]) == 5
    assert C.sizeof(_lib.ChangesInfo) == 24
    assert _lib.lib().mee_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"#define\s+MEE_ABI_VERSION\s+2\b", header)
    assert "meepo_changes.hip" in __import__("__graft_entry__").HIP_SOURCES


def test_cpp_wrappers_present():
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name in NAMES:
        wrapped = r"check\(" + name + r"\(" if not name.endswith("_destroy") else name + r"\("   # (a destructor does not throw)
        assert re.search(wrapped, hpp), f"include/meepo_embedding.hpp has no wrapper around {name}"


def test_null_arguments_are_refused(built):
    from meepoembedding_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.mee_changes_create(0, 0, C.byref(h)) == _lib.ERR_INVALID_ARG and not h.value
    assert L.mee_changes_create(0, 16, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_note(None, None, 0, None) == _lib.ERR_INVALID_ARG and L.mee_last_error().startswith(b"mee_changes_note:")
    assert L.mee_changes_group_create(None, 1, C.byref(h)) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_group_note(None, None, None, 0, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_info_get(None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_clear(None, None) == _lib.ERR_INVALID_ARG and L.mee_changes_invalidate(None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_export_changed(None, None, 0, 0, None, None, None, None, 0, None, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_changes_destroy(None) == 0 and L.mee_changes_group_destroy(None) == 0


def test_untracked_is_the_default():
    from meepoembedding_amd import ChangeLog, LookupTable, TableGroup
    assert LookupTable.change_log is None and LookupTable.__new__(LookupTable).change_log is None
    assert TableGroup.change_logs is None and TableGroup.__new__(TableGroup)._change_group is None
    assert callable(LookupTable.track_changes) and callable(TableGroup.track_changes) and ChangeLog.save_id is None


# ---- which methods note: a recording stand-in for the library -----------------------------------------------------------------------------------
@pytest.fixture
def recorded(built, monkeypatch):
    from meepoembedding_amd import table as tm
    calls = []

    class Recorder:   # stands in for the library: records what would have been launched
        def __getattr__(self, name):
            calls.append(name)
            return lambda *a: 0

    monkeypatch.setattr(tm._lib, "lib", lambda: Recorder())
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    return calls


def fake_table(tracked):
    from meepoembedding_amd import ChangeLog, LookupTable, _lib
    t = LookupTable.__new__(LookupTable)
    t._h, t.device, t.dim, t.value_dtype, t.optimizer, t.capacity, t.max_batch, t.layout_epoch = None, torch.device("cpu"), DIM, torch.float32, _lib.OPT_ADAM, 64, 4, 0
    if tracked:
        t.change_log = ChangeLog.__new__(ChangeLog)
        t.change_log._h, t.change_log.device = None, torch.device("cpu")
    return t


def table_mutators():
    """name -> (call(table), the library calls it issues itself, in order)"""
    keys, rows = torch.arange(6, dtype=torch.int64), torch.zeros(6, DIM)
    found, slots, gi = torch.zeros(6, dtype=torch.uint8), torch.zeros(6, dtype=torch.int64), torch.zeros(6, dtype=torch.int32)
    m = {
        "insert": (lambda t: t.insert(keys, rows), ["mee_insert"]),
        "insert_missing": (lambda t: t.insert_missing(keys, rows, found), ["mee_insert_missing"]),
        "find_or_insert_missing": (lambda t: t.find_or_insert_missing(keys, rows.clone(), found), ["mee_find_or_insert_missing"]),
        "assign": (lambda t: t.assign(keys, rows), ["mee_assign"]),
        "remove": (lambda t: t.remove(keys), ["mee_remove"]),
        "find_or_insert": (lambda t: t.find_or_insert(keys), ["mee_find_or_insert"]),
        "find_or_insert(min_count)": (lambda t: t.find_or_insert(keys, min_count=2), ["mee_find_or_insert_admit"]),
        "find_or_insert(bf16)": (lambda t: t.find_or_insert(keys, out_dtype=torch.bfloat16), ["mee_find_or_insert_as"]),
        "find_or_insert_located": (lambda t: t.find_or_insert_located(keys), ["mee_find_or_insert_located"]),
        "find_or_insert_located(prepare)": (lambda t: t.find_or_insert_located(keys, prepare_apply=True), ["mee_find_or_insert_located_prepare"]),
        "apply_adagrad": (lambda t: t.apply_adagrad(keys, rows, 0.1), ["mee_apply_adagrad"]),
        "apply_adagrad(slots)": (lambda t: t.apply_adagrad(keys, rows, 0.1, slots=slots), ["mee_apply_adagrad_located"]),
        "apply_adagrad(grad_index)": (lambda t: t.apply_adagrad(keys, rows, 0.1, grad_index=gi), ["mee_apply_adagrad_indexed"]),
        "apply_adam": (lambda t: t.apply_adam(keys, rows, 0.1), ["mee_apply_adam"]),
        "apply_adam(slots)": (lambda t: t.apply_adam(keys, rows, 0.1, slots=slots), ["mee_apply_adam_located"]),
        "apply_adam(grad_index)": (lambda t: t.apply_adam(keys, rows, 0.1, grad_index=gi), ["mee_apply_adam_indexed"]),
        "apply_ftrl": (lambda t: t.apply_ftrl(keys, rows, 0.1), ["mee_apply_ftrl"]),
        "apply_ftrl(slots)": (lambda t: t.apply_ftrl(keys, rows, 0.1, slots=slots), ["mee_apply_ftrl_located"]),
        "apply_ftrl(grad_index)": (lambda t: t.apply_ftrl(keys, rows, 0.1, grad_index=gi), ["mee_apply_ftrl_indexed"]),
    }
    for plane in (0, 1, 2):
        m[f"assign_plane({plane})"] = (lambda t, plane=plane: t.assign_plane(plane, keys, rows), ["mee_assign_plane"])
    return m


@pytest.mark.parametrize("name", sorted(table_mutators()))
def test_a_mutator_notes_once_in_front_of_its_own_calls(recorded, name):
    call, own = table_mutators()[name]
    call(fake_table(tracked=True))
    assert recorded == ["mee_changes_note"] + own, name
    del recorded[:]
    call(fake_table(tracked=False))
    assert recorded == own, f"{name}: an untracked table issues the calls it always issued"


def test_composed_mutators_clear_and_the_methods_that_note_nothing(recorded):
    keys, rows = torch.arange(6, dtype=torch.int64), torch.zeros(6, DIM)
    for tracked in (True, False):
        note = ["mee_changes_note"] if tracked else []
        t = fake_table(tracked)
        t.import_(keys, rows, rows, rows)        # through insert and assign_plane, max_batch (4) keys at a time
        assert recorded == (note + ["mee_insert"] + note + ["mee_assign_plane"] + note + ["mee_assign_plane"]) * 2
        del recorded[:]
        src, dst = fake_table(tracked), fake_table(tracked)
        src.move_to(dst, keys)                   # the keys leave one table and appear in the other
        assert recorded == note * 2 + ["mee_move"]
        del recorded[:]
        src.move_to(fake_table(False), keys)
        assert recorded == note + ["mee_move"]
        del recorded[:]
        t.evict(0, 5)                            # the evicted keys are only known afterwards
        assert recorded == ["mee_evict"] + note
        del recorded[:]
        t.evict(0, 5, spill=True)
        assert recorded == ["mee_evict"] + note
        del recorded[:]
        t.clear()
        assert recorded == (["mee_changes_invalidate"] if tracked else []) + ["mee_clear"]
        del recorded[:]
        t.find(keys); t.find_located(keys); t.find_located(keys, prepare_apply=True); t.find_plane(1, keys); t.locate(keys); t.reserve(128)
        t.find_pooled(keys, torch.tensor([0, 2, 6])); t.hits_of(keys); t.set_hits(keys, torch.zeros(6, dtype=torch.int32)); t.hits_decay(); t.apply_prepare(keys)
        assert not [c for c in recorded if c.startswith("mee_changes")], "lookups, reserve and the hit-counter operators note nothing"
        del recorded[:]


def fake_group(tracked):
    from meepoembedding_amd import TableGroup
    from meepoembedding_amd.changes import ChangeLogGroup
    g = TableGroup.__new__(TableGroup)
    g._h, g.device, g.dim, g._min_count_cache = None, torch.device("cpu"), DIM, {}
    g.tables = [fake_table(False), fake_table(False)]
    if tracked:
        g._change_group = ChangeLogGroup.__new__(ChangeLogGroup)
        g._change_group._h, g._change_group.device = None, torch.device("cpu")
    return g


def test_group_methods_note_with_one_grouped_launch(recorded):
    keys, rows = torch.arange(6, dtype=torch.int64), torch.zeros(6, DIM)
    off, bag_off, gi = torch.tensor([0, 2, 6]), torch.tensor([0, 1, 2, 4, 6]), torch.zeros(6, dtype=torch.int32)
    methods = {
        "find_or_insert": (lambda g: g.find_or_insert(keys, off), ["mee_group_find_or_insert"]),
        "find_or_insert(bf16)": (lambda g: g.find_or_insert(keys, off, out_dtype=torch.bfloat16), ["mee_group_find_or_insert_as"]),
        "find_or_insert(min_count)": (lambda g: g.find_or_insert(keys, off, min_count=2), ["mee_group_find_or_insert_admit"]),
        "apply_adagrad": (lambda g: g.apply_adagrad(keys, off, rows, 0.1), ["mee_group_apply_adagrad"]),
        "apply_adam": (lambda g: g.apply_adam(keys, off, rows, 0.1), ["mee_group_apply_adam"]),
        "apply_ftrl": (lambda g: g.apply_ftrl(keys, off, rows, 0.1), ["mee_group_apply_ftrl"]),
        "apply_pooled": (lambda g: g.apply_pooled(keys, bag_off, torch.zeros(4, DIM), gi, "adagrad", 0.1), ["mee_group_apply_adagrad_pooled"]),
        "apply_indexed": (lambda g: g.apply_indexed(keys, off, torch.zeros(3, DIM), gi, "adam", 0.1), ["mee_group_apply_adam_indexed"]),
        "move_to": (lambda g: g.move_to(fake_group(False), keys, off), ["mee_group_move"]),
    }
    for name, (call, own) in methods.items():
        call(fake_group(True))
        assert recorded == ["mee_changes_group_note"] + own, name
        del recorded[:]
        call(fake_group(False))
        assert recorded == own, f"{name}: an untracked group issues the calls it always issued"
        del recorded[:]
    fake_group(True).move_to(fake_group(True), keys, off)
    assert recorded == ["mee_changes_group_note"] * 2 + ["mee_group_move"]
    del recorded[:]
    g = fake_group(True)
    g.find(keys, off); g.find_pooled(keys, bag_off)
    assert recorded == ["mee_find_grouped", "mee_group_find_pooled"]


def test_the_bag_forms_take_every_bags_per_table_th_offset(built, monkeypatch):
    from meepoembedding_amd import table as tm
    seen = []
    g = fake_group(True)
    g._change_group.note = lambda k, o: seen.append(o.clone())
    monkeypatch.setattr(tm._lib, "lib", lambda: type("R", (), {"__getattr__": lambda self, n: (lambda *a: 0)})())
    monkeypatch.setattr(tm, "_stream_ptr", lambda device: 0)
    g.apply_pooled(torch.arange(6, dtype=torch.int64), torch.tensor([0, 1, 2, 4, 6]), torch.zeros(4, DIM), torch.zeros(6, dtype=torch.int32), "adagrad", 0.1)
    assert len(seen) == 1 and seen[0].tolist() == [0, 2, 6] and seen[0].is_contiguous()


# ---- the delta format over a dict-backed table --------------------------------------------------------------------------------------------------
class DictLog:
    """ChangeLog's interface over a Python set"""

    def __init__(self):
        self.keys, self.invalid, self.save_id = set(), False, None

    def note(self, keys):
        self.keys |= set(keys.tolist())

    def clear(self):
        self.keys, self.invalid = set(), False

    def iter_changed(self, table, chunk_slots, with_state=True):
        ks = sorted(self.keys)
        for s in range(0, len(ks), chunk_slots):
            part = ks[s:s + chunk_slots]
            held = [k for k in part if k in table.rows]
            gone = [k for k in part if k not in table.rows]
            planes = [torch.tensor(np.array([table.rows[k][p] for k in held], dtype=np.float32).reshape(len(held), DIM)) for p in range(2)]
            yield (torch.tensor(held, dtype=torch.int64), *planes, None, torch.tensor(gone, dtype=torch.int64))


class DictTable:
    """key -> (row, state1) behind the methods checkpoint.py uses of a LookupTable (an Adagrad table)"""
    dim, optimizer, max_batch = DIM, 1, 3

    def __init__(self):
        self.rows, self.change_log = {}, DictLog()

    def import_(self, keys, values, state1=None, state2=None):
        assert state2 is None
        self.change_log.note(keys)
        for i, k in enumerate(keys.tolist()):
            self.rows[k] = (values[i].numpy().copy(), state1[i].numpy().copy())

    def remove(self, keys):
        self.change_log.note(keys)
        for k in keys.tolist():
            self.rows.pop(k, None)

    def iter_export(self, chunk_slots, with_state=True):
        ks = sorted(self.rows)
        if ks:
            yield (torch.tensor(ks, dtype=torch.int64), *[torch.tensor(np.array([self.rows[k][p] for k in ks], dtype=np.float32)) for p in range(2)], None)

    def same_as(self, other):
        return sorted(self.rows) == sorted(other.rows) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for k in self.rows
                                                              for a, b in zip(self.rows[k], other.rows[k]))


def hand_made(keys, seed):
    rng = np.random.default_rng(seed)
    k = torch.tensor(keys, dtype=torch.int64)
    return k, torch.from_numpy(rng.standard_normal((len(keys), DIM)).astype(np.float32)), torch.from_numpy(rng.standard_normal((len(keys), DIM)).astype(np.float32))


def saved_chain(tmp_path):
    from meepoembedding_amd import checkpoint
    a = DictTable()
    a.import_(*hand_made([5, -7, 9, 11, 1 << 40, 13, 15], 1))
    base, d1, d2 = (str(tmp_path / x) for x in ("base", "d1", "d2"))
    assert checkpoint.save_base(a, base) == 7 and not a.change_log.keys and a.change_log.save_id
    a.import_(*hand_made([9, 21, 23], 2))                 # one overwritten, two new
    a.remove(torch.tensor([5, 99, -7]))                   # 99 was never there
    assert checkpoint.save_delta(a, d1, chunk_slots=2) == (3, 3) and not a.change_log.keys
    a.import_(*hand_made([5, 25], 3))                     # a removed key comes back
    a.remove(torch.tensor([21]))
    assert checkpoint.save_delta(a, d2) == (2, 1)
    return a, base, d1, d2


def test_delta_round_trip(tmp_path):
    from meepoembedding_amd import checkpoint
    a, base, d1, d2 = saved_chain(tmp_path)
    m1, m2 = (json.load(open(os.path.join(d, "meta.json"))) for d in (d1, d2))
    assert m1["format"] == "meepo-delta-v1" and (m1["dim"], m1["optimizer"], m1["planes"], m1["n"], m1["n_removed"]) == (DIM, 1, ["values", "state1"], 3, 3)
    assert m1["parent"] == json.load(open(os.path.join(base, "meta.json")))["extra"]["id"] and m2["parent"] == m1["id"] != m1["parent"]
    assert sorted(np.fromfile(os.path.join(d1, "removed.i64"), dtype="<i8").tolist()) == [-7, 5, 99]
    assert os.path.getsize(os.path.join(d1, "keys.i64")) == 24 and os.path.getsize(os.path.join(d1, "state1.f32")) == 3 * DIM * 4
    b = DictTable()
    assert checkpoint.restore(b, base, [d1, d2]) == 7
    assert b.same_as(a) and sorted(b.rows) == [5, 9, 11, 13, 15, 23, 25, 1 << 40]
    # keep: re-sharding restricts both lists
    even, odd = DictTable(), DictTable()
    checkpoint.restore(even, base, [d1, d2], keep=lambda k: k % 2 == 0)
    checkpoint.restore(odd, base, [d1, d2], keep=lambda k: k % 2 == 1)
    assert sorted(even.rows) == [1 << 40] and sorted(list(even.rows) + list(odd.rows)) == sorted(a.rows)
    assert checkpoint.load_delta(DictTable(), d1) == (3, 3)


def test_delta_refusals(tmp_path):
    from meepoembedding_amd import checkpoint
    a, base, d1, d2 = saved_chain(tmp_path)
    with pytest.raises(ValueError, match="parent"):       # a gap
        checkpoint.restore(DictTable(), base, [d2])
    with pytest.raises(ValueError, match="parent"):       # a reordering
        checkpoint.restore(DictTable(), base, [d2, d1])
    b = DictTable()
    with pytest.raises(ValueError, match="parent"):
        checkpoint.restore(b, base, [d1, d1])
    assert not b.rows, "the chain is checked before anything is loaded"
    with pytest.raises(ValueError, match="meepo-delta-v1"):   # a table checkpoint is no delta ...
        checkpoint.load_delta(DictTable(), base)
    with pytest.raises(ValueError, match="meepo-table-v1"):   # ... and a delta no table checkpoint
        checkpoint.load_into(DictTable(), d1)
    meta = json.load(open(os.path.join(d2, "meta.json")))
    json.dump({**meta, "format": "meepo-delta-v0"}, open(os.path.join(d2, "meta.json"), "w"))
    with pytest.raises(ValueError, match="meepo-delta-v1"):
        checkpoint.load_delta(DictTable(), d2)
    with open(os.path.join(d1, "removed.i64"), "r+b") as f:
        f.truncate(16)
    with pytest.raises(ValueError, match="removed.i64"):
        checkpoint.load_delta(DictTable(), d1)
    # an invalid log: nothing is written that could pass for a delta, and the log is left as it is
    a.import_(*hand_made([31], 4))
    a.change_log.invalid = True
    d3 = str(tmp_path / "d3")
    with pytest.raises(RuntimeError, match="invalid"):
        checkpoint.save_delta(a, d3)
    assert not os.path.exists(os.path.join(d3, "meta.json")) and a.change_log.keys == {31}
    # no log, or no base yet
    untracked = DictTable()
    untracked.change_log = None
    with pytest.raises(ValueError, match="track_changes"):
        checkpoint.save_delta(untracked, d3)
    with pytest.raises(ValueError, match="save_base"):
        checkpoint.save_delta(DictTable(), d3)
