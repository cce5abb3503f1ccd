"""Change logs (SPEC.md §3 "Change log"): which keys of a table changed since the last save, and the table's delta over them.

A `ChangeLog` is a set of int64 keys on the device (mee_changes: a table key plane and two words, `size` and `invalid`).  It belongs to no table;
`LookupTable.track_changes(capacity)` attaches one, and from then on every mutator of that table notes its batch's keys in it — one launch on the
table's stream, in front of the mutator's own library calls.  `iter_changed(table)` turns the set into "these keys with their rows and optimizer
planes, and these keys are gone" (mee_export_changed), one slot range of the log at a time; checkpoint.save_delta writes exactly that.

A log that could not store a key (it was full), or whose table did something a key set cannot name (clear()), is `invalid`: the delta would be
incomplete, and save_delta refuses it.  clear() makes it usable again — after a full save.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import table as _table
from ._lib import MeepoError, check


class ChangeLog:
    """A device-resident set of changed keys.  capacity: the distinct keys it can hold between two saves (rounded up as a table's capacity is)."""
    save_id = None   # the id of the latest save_base / save_delta that cleared this log (checkpoint.py): the next delta's parent

    def __init__(self, capacity: int, device: int | torch.device = 0):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise MeepoError(_lib.ERR_NO_DEVICE, "ChangeLog needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        h = C.c_void_p()
        self._h = None
        check(_lib.lib().mee_changes_create(self.device.index, int(capacity), C.byref(h)))
        self._h = h
        self.capacity = self._info().capacity

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_changes_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _s(self) -> int:
        return _table._stream_ptr(self.device)

    def _info(self) -> _lib.ChangesInfo:
        info = _lib.ChangesInfo()
        check(_lib.lib().mee_changes_info_get(self._h, C.byref(info)))
        return info

    def note(self, keys: torch.Tensor) -> None:
        """Add the batch's keys to the set (EMPTY and RECLAIMED are padding).  One launch on the current stream, no synchronisation."""
        if keys.dtype != torch.int64 or keys.device != self.device:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"keys must be int64 on {self.device}")
        k = keys if keys.dim() == 1 and keys.is_contiguous() else keys.contiguous().view(-1)
        check(_lib.lib().mee_changes_note(self._h, k.data_ptr(), k.numel(), self._s()))

    def size(self) -> int:
        """distinct keys stored; synchronises"""
        return int(self._info().size)

    @property
    def invalid(self) -> bool:
        """the log no longer names every change (a key found no room, or invalidate()); synchronises"""
        return bool(self._info().invalid)

    def clear(self) -> None:
        check(_lib.lib().mee_changes_clear(self._h, self._s()))

    def invalidate(self) -> None:
        check(_lib.lib().mee_changes_invalidate(self._h, self._s()))

    def export_changed(self, table, slot_begin: int, slot_end: int, with_state: bool = True):
        """The delta of `table` over the log's slots [slot_begin, slot_end) -> (keys, values, state1 | None, state2 | None, removed): the noted keys the
        table holds with their rows and optimizer planes (one shared unspecified order), and the noted keys it does not hold.  One launch, then ONE
        read-back of the two counts."""
        slot_end = min(int(slot_end), self.capacity)
        cap = max(slot_end - int(slot_begin), 0)
        dev, dim = self.device, table.dim
        keys = torch.empty(cap, dtype=torch.int64, device=dev)
        vals = torch.empty((cap, dim), dtype=torch.float32, device=dev)
        s1 = torch.empty((cap, dim), dtype=torch.float32, device=dev) if with_state and table.optimizer != _lib.OPT_NONE else None
        s2 = torch.empty((cap, dim), dtype=torch.float32, device=dev) if with_state and table.optimizer in (_lib.OPT_ADAM, _lib.OPT_FTRL) else None
        removed = torch.empty(cap, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        check(_lib.lib().mee_export_changed(table._h, self._h, int(slot_begin), slot_end, keys.data_ptr(), vals.data_ptr(), _table._ptr(s1), _table._ptr(s2), cap,
                                            removed.data_ptr(), cap, counts.data_ptr(), self._s()))
        n, r = (int(x) for x in counts.tolist())   # the one synchronisation, as export_range has
        return keys[:n], vals[:n], (s1[:n] if s1 is not None else None), (s2[:n] if s2 is not None else None), removed[:r]

    def publish(self, table, serving, slot_begin: int = 0, slot_end: int | None = None) -> torch.Tensor:
        """The delta of `table` over the log's slots [slot_begin, slot_end) (None: to the end) straight into `serving`, device to device (SPEC.md §3
        "Publish", mee_publish_changed): the noted keys `table` holds end up in `serving` with the table's values row (rounded once for a bf16-row
        serving table), the noted keys it does not hold are removed there.  -> int64 device tensor [4]: keys placed, keys absent from `table`, keys
        dropped for lack of room (STATUS_TABLE_FULL on `serving`), the log's invalid word.  One library call, no buffer, no synchronisation."""
        for t in (table, serving):
            if t.device != self.device:
                raise MeepoError(_lib.ERR_INVALID_ARG, f"publish: both tables must be on {self.device}, the log's device")
        counts = torch.empty(4, dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_publish_changed(table._h, self._h, serving._h, int(slot_begin), 0xFFFFFFFFFFFFFFFF if slot_end is None else int(slot_end),
                                             counts.data_ptr(), self._s()))
        serving.layout_epoch += 1   # rows may have been freed: slot handles of `serving` from before are stale
        return counts

    def iter_changed(self, table, chunk_slots: int = 1 << 22, with_state: bool = True):
        """Generator over export_changed pieces covering the whole log (pieces without a key are skipped)."""
        for b in range(0, self.capacity, int(chunk_slots)):
            piece = self.export_changed(table, b, b + int(chunk_slots), with_state)
            if piece[0].numel() or piece[4].numel():
                yield piece


class ChangeLogGroup:
    """The logs of a table group's members behind ONE note launch (mee_changes_group_note): position i of segment j of a jagged batch goes to logs[j]."""

    def __init__(self, logs):
        self.logs = list(logs)
        if not self.logs:
            raise ValueError("a group of change logs needs at least one log")
        self.device = self.logs[0].device
        arr = (C.c_void_p * len(self.logs))(*[g._h for g in self.logs])
        h = C.c_void_p()
        self._h = None
        check(_lib.lib().mee_changes_group_create(arr, len(self.logs), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_changes_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def note(self, keys: torch.Tensor, offsets: torch.Tensor) -> None:
        """offsets: the n_tables + 1 member bounds (int64, on the device) of the flat key batch"""
        check(_lib.lib().mee_changes_group_note(self._h, keys.data_ptr(), offsets.data_ptr(), keys.numel(), _table._stream_ptr(self.device)))
