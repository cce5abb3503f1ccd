"""No GPU: the publish operator (SPEC.md §3 "Publish") as the library exports it and as the Python layer wires it — the two entry points in the
header, the loader and the C++ wrappers, their null-argument refusals, and which library calls LookupTable.publish_to and TableGroup.publish_to
issue (a recording stand-in for the library, as tests/test_changes_symbols.py has one)."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mee_group_publish_changed", "mee_publish_changed"]
DIM = 8


def test_the_symbols(built):
    from meepoembedding_amd import _lib
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    assert sorted(set(re.findall(r"\bint\s+(mee_\w*publish\w*)\(", header))) == NAMES
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        decl = re.sub(r"/\*.*?\*/", "", re.search(r"\bint\s+" + name + r"\(([^;]*)\);", header).group(1), flags=re.S)
        assert len(_lib.PROTOTYPES[name][1]) == decl.count(",") + 1, f"{name}: bound with another number of arguments than declared"
    assert len(_lib.PROTOTYPES["mee_publish_changed"][1]) == 7 and len(_lib.PROTOTYPES["mee_group_publish_changed"][1]) == 5
    assert _lib.lib().mee_abi_version() == 2 == _lib.ABI_VERSION
    assert re.search(r"#define\s+MEE_ABI_VERSION\s+2\b", header)


def test_cpp_wrappers_present():
    hpp = open(os.path.join(ROOT, "include", "meepo_embedding.hpp")).read()
    for name in NAMES:
        assert re.search(r"check\(" + name + r"\(", hpp), f"include/meepo_embedding.hpp has no wrapper around {name}"


def test_null_arguments_are_refused(built):
    """the null check comes first, in front of anything that needs a device"""
    from meepoembedding_amd import _lib
    L = _lib.lib()
    assert L.mee_publish_changed(None, None, None, 0, 0, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_last_error().startswith(b"mee_publish_changed:")
    assert L.mee_group_publish_changed(None, None, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.mee_last_error().startswith(b"mee_group_publish_changed:")


# ---- which library calls publish_to issues: a recording stand-in for the library -----------------------------------------------------------------
@pytest.fixture
def recorded(built, monkeypatch):
    from meepoembedding_amd import table as tm
    calls = []

    class Recorder:   # stands in for the library: records what would have been launched; a publish "zeroes" its counts, as the library does first
        def __getattr__(self, name):
            calls.append(name)
            if name == "mee_publish_changed":
                return lambda *a: C.memset(a[5], 0, 4 * 8) and 0
            if name == "mee_group_publish_changed":
                return lambda *a: C.memset(a[3], 0, 2 * 4 * 8) and 0
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


def fake_group(tracked):
    from meepoembedding_amd import TableGroup
    from meepoembedding_amd.changes import ChangeLogGroup
    g = TableGroup.__new__(TableGroup)
    g._h, g.device, g.dim, g._min_count_cache = None, torch.device("cpu"), DIM, {}
    g.tables = [fake_table(False), fake_table(False)]
    if tracked:
        g._change_group = ChangeLogGroup.__new__(ChangeLogGroup)
        g._change_group._h, g._change_group.device = None, torch.device("cpu")
        g.change_logs = [fake_table(True).change_log for _ in g.tables]
    return g


def test_publish_to_is_one_library_call(recorded):
    src, serving = fake_table(True), fake_table(False)
    assert src.publish_to(serving) == (0, 0, 0)                       # check=True: the read-back is no library call
    assert recorded == ["mee_publish_changed"] and serving.layout_epoch == 1 and src.layout_epoch == 0
    del recorded[:]
    counts = src.publish_to(serving, check=False)
    assert recorded == ["mee_publish_changed"] and isinstance(counts, torch.Tensor) and counts.dtype == torch.int64 and tuple(counts.shape) == (4,)
    del recorded[:]
    src.publish_to(serving, clear=True, check=False)                  # the log is cleared BEHIND the publish; nothing is noted anywhere
    assert recorded == ["mee_publish_changed", "mee_changes_clear"]


def test_group_publish_to_is_one_library_call(recorded):
    g, serving = fake_group(True), fake_group(False)
    assert g.publish_to(serving) == [(0, 0, 0), (0, 0, 0)]
    assert recorded == ["mee_group_publish_changed"] and [t.layout_epoch for t in serving.tables] == [1, 1]
    del recorded[:]
    counts = g.publish_to(serving, check=False)
    assert recorded == ["mee_group_publish_changed"] and tuple(counts.shape) == (2, 4)
    del recorded[:]
    g.publish_to(serving, clear=True)
    assert recorded == ["mee_group_publish_changed", "mee_changes_clear", "mee_changes_clear"]


def test_publish_to_refuses_before_any_call(recorded):
    with pytest.raises(ValueError, match="track_changes"):
        fake_table(False).publish_to(fake_table(False))
    with pytest.raises(ValueError, match="tracked"):
        fake_table(True).publish_to(fake_table(True))
    with pytest.raises(ValueError, match="track_changes"):
        fake_group(False).publish_to(fake_group(False))
    with pytest.raises(ValueError, match="tracked"):
        fake_group(True).publish_to(fake_group(True))
    member_tracked = fake_group(False)
    member_tracked.tables[1] = fake_table(True)
    with pytest.raises(ValueError, match="tracked"):
        fake_group(True).publish_to(member_tracked)
    assert recorded == []


def test_the_checks_of_the_counts():
    from meepoembedding_amd import MeepoError
    from meepoembedding_amd.table import _publish_checked
    assert _publish_checked([5, 2, 0, 0]) == (5, 2, 0, 0)
    with pytest.raises(RuntimeError, match="rebuild the serving copy.*clear"):
        _publish_checked([5, 2, 3, 1])                               # an invalid log comes first
    with pytest.raises(MeepoError, match="no room for 3 keys"):
        _publish_checked([5, 2, 3, 0])
    assert not issubclass(RuntimeError, MeepoError)
