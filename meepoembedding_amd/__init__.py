"""meepoembedding_amd — MI355X (gfx950) GPU backend for a dynamic lookup-table embedding.

The package is a thin host layer over libmeepo_hip.so (C-ABI: include/meepo_embedding.h; hand-written HIP
kernels in csrc/).  Importing the package does not touch the GPU; creating a table does, and fails loudly when
the HIP extension or a gfx950 device is missing — there is no CPU fallback.
"""
from ._lib import (EMPTY_KEY, INIT_CONSTANT, INIT_UNIFORM, OPT_ADAGRAD, OPT_ADAM, OPT_FTRL, OPT_NONE, RECLAIMED_KEY,
                   STATUS_RESERVED_KEY, STATUS_TABLE_FULL, MeepoError)
from .changes import ChangeLog
from .table import LookupTable, MixedTableGroup, Router, TableGroup, hash_batch, keyed_layout, mixed_layout
from .tiered import TieredLookupTable, TieredTableGroup

__all__ = ["LookupTable", "ChangeLog", "Router", "TableGroup", "MixedTableGroup", "TieredLookupTable", "TieredTableGroup", "mixed_layout", "keyed_layout", "hash_batch", "MeepoError", "OPT_NONE", "OPT_ADAGRAD", "OPT_ADAM", "OPT_FTRL",
           "INIT_CONSTANT", "INIT_UNIFORM", "STATUS_TABLE_FULL", "STATUS_RESERVED_KEY", "EMPTY_KEY", "RECLAIMED_KEY", "ShardedTieredTableGroup"]


def __getattr__(name):
    if name == "ShardedTieredTableGroup":   # sharded.py imports torch.distributed: only when the class is asked for
        from .sharded import ShardedTieredTableGroup
        return ShardedTieredTableGroup
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
