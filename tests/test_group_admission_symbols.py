"""No GPU: the built library exports the grouped admission entry points and the ctypes loader declares them with the header's argument lists."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {"mee_group_find_or_insert_admit": 10, "mee_group_admission_decay": 3}


def test_library_exports_and_loader_declares_grouped_admission(built):
    from meepoembedding_amd import _lib
    from meepoembedding_amd.table import TableGroup
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "meepo_embedding.h")).read()
    for name, n_args in SYMBOLS.items():
        assert hasattr(raw, name), f"{name} is not exported by {_lib.LIB_PATH}"
        fn = getattr(_lib.lib(), name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto and len(proto.group(1).split(",")) == n_args, f"{name}: prototype missing from include/meepo_embedding.h or its arity differs"
    assert "min_count" in inspect.signature(TableGroup.find_or_insert).parameters and hasattr(TableGroup, "admission_decay")
