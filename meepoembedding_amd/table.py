"""Host-side lookup-table interface over the C-ABI (include/meepo_embedding.h).

Mirrors the operator set BASELINE.json's north_star names for the reference's GPU backend — find / insert /
assign / export (+ find_or_insert, size, sparse Adagrad/Adam apply).  The reference snapshot defines no
interface (only /root/reference/README.md:2, "dynamic lookuptable-style Embedding"); semantics are SPEC.md §3-§4.

torch is plumbing only: it owns the device buffers and the stream.  Every method takes/returns CUDA(HIP)
tensors on the table's device and enqueues on torch's current stream; nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple

import torch

from . import _lib
from ._lib import (INIT_CONSTANT, INIT_UNIFORM, OPT_ADAGRAD, OPT_ADAM, OPT_FTRL, OPT_NONE, STATUS_RESERVED_KEY,  # noqa: F401
                   STATUS_TABLE_FULL, MeepoError, check)


def _stream_ptr(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_weights(weights: torch.Tensor, mode: str, n: int, device: torch.device) -> torch.Tensor:
    """per_sample_weights of a weighted pooled lookup: checked like bag_offsets, before any launch"""
    if mode != "sum":
        raise ValueError(f"weighted pooling supports mode='sum' only (got {mode!r}), as torch.nn.EmbeddingBag does")
    if weights.dtype != torch.float32 or weights.device != device or weights.numel() != n or not weights.is_contiguous():
        raise MeepoError(_lib.ERR_INVALID_ARG, f"weights must be contiguous float32 with one entry per key ({n}) on {device}")
    return weights.view(-1)


def _n_bags(bag_offsets: torch.Tensor, device: torch.device) -> int:
    """the bag_offsets of a pooled lookup, checked before any launch -> the number of bags"""
    if bag_offsets.device != device or bag_offsets.dtype not in (torch.int64, torch.uint64) or not bag_offsets.is_contiguous() \
            or bag_offsets.numel() < 1:
        raise MeepoError(_lib.ERR_INVALID_ARG, f"bag_offsets must be contiguous int64 on {device} with n_bags + 1 entries")
    return bag_offsets.numel() - 1


def _check_bags(bag_offsets: torch.Tensor, n_tables: int, device: torch.device) -> int:
    """the bag_offsets of a group's pooled lookup (bag b belongs to member b // bags_per_table), checked before any launch -> bags_per_table"""
    nb = bag_offsets.numel() - 1
    if bag_offsets.device != device or bag_offsets.dtype not in (torch.int64, torch.uint64) or not bag_offsets.is_contiguous() \
            or nb < 0 or nb % n_tables:
        raise MeepoError(_lib.ERR_INVALID_ARG, f"bag_offsets must be contiguous int64 on {device} with n_tables * bags_per_table + 1 entries")
    return nb // n_tables


def _buffer(t: torch.Tensor | None, name: str, dtype, shape, device: torch.device) -> torch.Tensor:
    """THE rule for a result buffer (DESIGN.md "Result buffers"): None -> a fresh torch.empty(shape); a caller's tensor must have the dtype (one of
    the dtypes, where `dtype` is a tuple: the uint32 / int32 pairs; a fresh one gets the first), the operator's device, exactly prod(shape)
    elements — the shape itself is not compared, a flat buffer is legal — and be contiguous, or the call is refused before anything is launched.
    `shape`: a tuple, or an int for a 1-D buffer."""
    if t is None:
        return torch.empty(shape, dtype=dtype[0] if type(dtype) is tuple else dtype, device=device)
    if (t.dtype != dtype and (type(dtype) is not tuple or t.dtype not in dtype)) or t.device != device \
            or t.numel() != (shape if type(shape) is int else math.prod(shape)) or not t.is_contiguous():
        kinds = " or ".join(str(d) for d in dtype) if type(dtype) is tuple else str(dtype)
        raise MeepoError(_lib.ERR_INVALID_ARG, f"{name} must be a contiguous {kinds} buffer of shape {list(shape) if type(shape) is tuple else [shape]} on {device} "
                                               f"(got {t.dtype} {list(t.shape)} on {t.device}{'' if t.is_contiguous() else ', not contiguous'})")
    return t


def _pool_mode(mode: str, error=None) -> int:
    """the library's number for a pooled lookup's mode, checked before anything is allocated.  error: the caller's exception class for another
    name (ValueError in LookupTable and the tiered classes); without it MeepoError(ERR_INVALID_ARG), as the group classes raise"""
    if mode == "sum":
        return 0
    if mode == "mean":
        return 1
    msg = f"mode must be 'sum' or 'mean' (got {mode!r})"
    raise error(msg) if error is not None else MeepoError(_lib.ERR_INVALID_ARG, msg)


def _no_bags_for_keys(n: int, n_bags: int) -> None:
    if n and n_bags == 0:
        raise MeepoError(_lib.ERR_INVALID_ARG, "there are keys but no bags: no bag would report them")


def _pooled_args(k: torch.Tensor, device: torch.device, out, out_shape, out_dtype: torch.dtype, found, weights=None, mode: str = "sum", located=None,
                 keyed: bool = False):
    """what every pooled lookup prepares between its own argument checks and its launch, given the flat keys and the checked bag_offsets of its
    owner: the weights checked, then the result buffers by _buffer's rule — located (only where the caller passed one), out (keyed: the
    [bags_per_table, width] block by _keyed_out's rule) and found -> (n, weights | None, located | None, out, its row stride (keyed) | 0, found)"""
    n = k.numel()
    w = _check_weights(weights, mode, n, device) if weights is not None else None
    if located is not None:
        located = _buffer(located, "located", torch.int64, n, device)
    if keyed:
        out, stride = _keyed_out(out, out_shape[0], out_shape[1], out_dtype, device)
    else:
        out, stride = _buffer(out, "out", out_dtype, out_shape, device), 0
    return n, w, located, out, stride, _buffer(found, "found", torch.uint8, n, device)


def _ptr(t: torch.Tensor | None):
    return t.data_ptr() if t is not None else None


_OUT_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16}


def _out_dtype(out_dtype: torch.dtype, out: torch.Tensor | None = None) -> int:
    """MEE_DTYPE_* of a lookup's result rows (SPEC.md §3 "Output type"); a caller's `out` must have that dtype.  Checked before any launch."""
    if out_dtype not in _OUT_DTYPES:
        raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype}): the lookups write fp32 rows or their bf16 rounding")
    if out is not None and out.dtype != out_dtype:
        raise ValueError(f"out has dtype {out.dtype} but out_dtype is {out_dtype}")
    return _OUT_DTYPES[out_dtype]


def _fp32_only(out: torch.Tensor | None, op: str) -> None:
    """operators without a bf16 form say so instead of writing fp32 bytes into a bf16 buffer"""
    if out is not None and out.dtype != torch.float32:
        raise ValueError(f"{op} returns fp32 rows only (out has dtype {out.dtype}); bf16 output exists for find, find_located, find_or_insert, "
                         "find_or_insert_located, find_pooled and the TableGroup lookups")


_PAD_KEEP = {"first": _lib.PAD_KEEP_FIRST, "last": _lib.PAD_KEEP_LAST}


def _publish_checked(counts, who: str = "") -> tuple:
    """the four counts of a publish, read back (upserts, removed, dropped, invalid) -> the same, or the two refusals of publish_to(check=True)"""
    upserts, removed, dropped, invalid = (int(c) for c in counts)
    if invalid:
        raise RuntimeError(f"publish_to: the change log{who} is invalid — it does not name every change since it was cleared, so the serving copy may be "
                           "stale in keys it never saw: rebuild the serving copy (serving_copy() / checkpoint.load_into) and clear() the log")
    if dropped:
        raise MeepoError(_lib.ERR_OUT_OF_MEMORY, f"publish_to: the serving table{who} had no room for {dropped} keys (STATUS_TABLE_FULL): they are missing "
                                                 "there — rebuild it with a larger capacity")
    return upserts, removed, dropped, invalid


def keyed_layout(dims):
    """The keyed layout of a group's pooled lookup (SPEC.md §3 "Keyed output"): one row per sample, member j's pooled vector at column col_offsets[j] =
    the sum of the dims before it in the caller's order -> (col_offsets, width).  A uniform group: col_offsets[j] = j * dim."""
    cols, width = [], 0
    for d in dims:
        cols.append(width)
        width += int(d)
    return cols, width


def _check_layout(layout: str) -> bool:
    """-> whether a find_pooled call asks for the keyed layout"""
    if layout not in ("table", "keyed"):
        raise ValueError(f"layout must be 'table' or 'keyed' (got {layout!r})")
    return layout == "keyed"


def _keyed_out(out: torch.Tensor | None, bags_per_table: int, width: int, out_dtype: torch.dtype, device: torch.device):
    """the [bags_per_table, width] block of a keyed lookup -> (out, its row stride in elements): a fresh one, or the caller's 2-D tensor with
    stride(1) == 1 and any row stride the library takes (a view into a wider feature block)"""
    if out is None:
        return torch.empty((bags_per_table, width), dtype=out_dtype, device=device), width
    if out.dim() != 2 or tuple(out.shape) != (bags_per_table, width) or out.dtype != out_dtype or out.device != device or (width > 1 and out.stride(1) != 1):
        raise MeepoError(_lib.ERR_INVALID_ARG, f"a keyed out must be a {out_dtype} [{bags_per_table}, {width}] tensor on {device} with stride(1) == 1")
    return out, (out.stride(0) if bags_per_table > 1 else width)


def _step_index(step_index: torch.Tensor | None, n: int, device: torch.device):
    """the data pointer of a keyed lookup's step_index buffer (None: not asked for)"""
    return None if step_index is None else _buffer(step_index, "step_index", (torch.uint32, torch.int32), n, device).data_ptr()


def _find_padded(fn, handle, device: torch.device, dim: int, k: torch.Tensor, bag_offsets: torch.Tensor, n_bags: int, bags_arg: int, max_len: int,
                 keep: str, out, found, out_dtype: torch.dtype, with_step: bool):
    """the padded lookup of a table (fn = mee_find_padded_as, bags_arg = n_bags) or a group (mee_group_find_padded_as, bags_arg = bags_per_table):
    arguments checked before any launch, buffers allocated here — the per-position ones pre-set to what a position in no bag reports (not found,
    EMPTY, index 0), since the launch leaves those alone."""
    dt = _out_dtype(out_dtype, out)
    if keep not in _PAD_KEEP:
        raise ValueError(f"keep must be 'first' or 'last' (got {keep!r})")
    max_len = int(max_len)
    if max_len < 1:
        raise ValueError(f"max_len must be at least 1 (got {max_len})")
    n = k.numel()
    out = _buffer(out, "out", out_dtype, (n_bags, max_len, dim), device)
    found = torch.zeros(n, dtype=torch.uint8, device=device) if found is None else _buffer(found, "found", torch.uint8, n, device)
    lengths = torch.empty(n_bags, dtype=torch.int64, device=device)
    step_keys = torch.full((n,), _lib.EMPTY_KEY, dtype=torch.int64, device=device) if with_step else None
    grad_index = torch.zeros(n, dtype=torch.int32, device=device) if with_step else None   # (uint32 to the library: a slot number below 2^31)
    check(fn(handle, k.data_ptr(), n, bag_offsets.data_ptr(), bags_arg, max_len, _PAD_KEEP[keep], out.data_ptr(), dt, found.data_ptr(), lengths.data_ptr(),
             step_keys.data_ptr() if with_step else None, grad_index.data_ptr() if with_step else None, _stream_ptr(device)))
    out = out.view(n_bags, max_len, dim)
    return (out, found, lengths, step_keys, grad_index) if with_step else (out, found, lengths)


def _argmax_buffer(argmax: torch.Tensor | None, n_bags: int, dim: int, device: torch.device) -> torch.Tensor:
    """the [n_bags, dim] batch positions of max pooling: uint32 to the library (int32 holds the same bits; 0xFFFFFFFF = an empty bag)"""
    return _buffer(argmax, "argmax", (torch.uint32, torch.int32), (n_bags, dim), device)


def _find_pooled_max(fn, handle, device: torch.device, dim: int, k: torch.Tensor, bag_offsets: torch.Tensor, n_bags: int, bags_arg: int, out, found, argmax,
                     out_dtype: torch.dtype, with_argmax: bool):
    """max pooling over a table (fn = mee_find_pooled_max, bags_arg = n_bags) or a group (mee_group_find_pooled_max, bags_arg = bags_per_table):
    arguments checked before any launch, buffers allocated here"""
    dt = _out_dtype(out_dtype, out)
    n, _, _, out, _, found = _pooled_args(k, device, out, (n_bags, dim), out_dtype, found)
    if argmax is not None or with_argmax:
        argmax = _argmax_buffer(argmax, n_bags, dim, device)
    check(fn(handle, k.data_ptr(), n, bag_offsets.data_ptr(), bags_arg, out.data_ptr(), dt, found.data_ptr(), _ptr(argmax), _stream_ptr(device)))
    return out, found, argmax


def _pooled_max_backward(fn, handle, device: torch.device, dim: int, bag_offsets: torch.Tensor, n_bags: int, bags_arg: int, argmax: torch.Tensor,
                         bag_grads: torch.Tensor, n: int, grads):
    """the backward of max pooling over a table (mee_pooled_max_backward) or a group (mee_group_pooled_max_backward)"""
    a = _argmax_buffer(argmax, n_bags, dim, device)
    n = int(n)
    if bag_grads.dtype != torch.float32 or bag_grads.device != device or bag_grads.numel() != n_bags * dim:
        raise MeepoError(_lib.ERR_INVALID_ARG, f"bag_grads must be float32 [{n_bags}, {dim}] on {device}")
    g = bag_grads.contiguous()
    grads = _buffer(grads, "grads", torch.float32, (n, dim), device)
    check(fn(handle, n, bag_offsets.data_ptr(), bags_arg, a.data_ptr(), g.data_ptr(), grads.data_ptr(), _stream_ptr(device)))
    return grads


def _max_mode_only(**given) -> None:
    """find_pooled(mode="max") is find_pooled_max: the arguments of the other forms are refused by name"""
    for name, value in given.items():
        if value is not None:
            raise ValueError(f"find_pooled(mode='max') takes no {name}: max pooling has no weighted, located or keyed form (torch.nn.EmbeddingBag refuses "
                             "per_sample_weights with mode='max' too)")


def _padded_places(keys, bag_offsets, max_len: int, keep_last: bool):
    """find_padded's bookkeeping in torch, the ONE place a composition gets it from (nn.lookup_padded over a table without find_padded; the tiered
    classes over tiers that are not native tables) -> (lengths [n_bags] int64, step_keys [n] int64, grad_index [n] int32, the kept positions in slot
    order): the bags clamped as the library clamps them, kept = min(len, max_len) positions from the bag's front or back, slot b * max_len + j for
    the j-th of them; EMPTY / 0 everywhere else.  The kept positions come from the placement, never from the keys: a kept position whose key is
    EMPTY still fills its slot (with the default row)."""
    n = keys.numel()
    off = bag_offsets.to(torch.int64).clamp(min=0, max=n)
    end = off[1:]
    begin = torch.minimum(off[:-1], end)
    kept = (end - begin).clamp(max=max_len)
    first = end - kept if keep_last else begin
    j = torch.arange(max_len, device=keys.device)[None, :]
    live = j < kept[:, None]                                   # [n_bags, max_len]: the slots that hold a row
    pos = (first[:, None] + j)[live]
    slot = torch.nonzero(live.reshape(-1)).view(-1)
    step_keys = torch.full((n,), -(1 << 63), dtype=torch.int64, device=keys.device)
    grad_index = torch.zeros(n, dtype=torch.int32, device=keys.device)
    step_keys[pos] = keys[pos]
    grad_index[pos] = slot.to(torch.int32)
    return kept, step_keys, grad_index, pos


def _find_padded_composed(find_kept, dim: int, keys: torch.Tensor, bag_offsets: torch.Tensor, max_len: int, keep: str, out, found,
                          out_dtype: torch.dtype, with_step: bool):
    """find_padded's results by composition, for tables that have no launch of their own for it: _padded_places, then find_kept(kept keys, their
    positions) -> (rows [n_kept, dim] fp32, found [n_kept]) placed into a zeroed block, the rows rounded once for a bf16 block.  A truncated position
    reports found 0; a position in no bag keeps what the caller's `found` holds."""
    _out_dtype(out_dtype, out)   # the refusals of _find_padded, in its order, before anything is looked up or written
    if keep not in _PAD_KEEP:
        raise ValueError(f"keep must be 'first' or 'last' (got {keep!r})")
    max_len = int(max_len)
    if max_len < 1:
        raise ValueError(f"max_len must be at least 1 (got {max_len})")
    flat = keys.contiguous().view(-1)
    n, n_bags, device = flat.numel(), _n_bags(bag_offsets, flat.device), flat.device
    if out is not None:
        _buffer(out, "out", out_dtype, (n_bags, max_len, dim), device)
    if found is not None:
        _buffer(found, "found", torch.uint8, n, device)
    lengths, step_keys, grad_index, pos = _padded_places(flat, bag_offsets, max_len, keep == "last")
    block = torch.zeros((n_bags * max_len, dim), dtype=out_dtype, device=device)
    fnd = torch.zeros(n, dtype=torch.uint8, device=device) if found is None else found.view(-1)
    # every position inside a bag: not found unless kept and held (a position in no bag keeps the caller's byte).  No host read-back: the bags'
    # clamped spans as +1 / -1 marks, summed up
    off = bag_offsets.to(torch.int64).clamp(min=0, max=n)
    marks = torch.zeros(n + 1, dtype=torch.int64, device=device)
    marks.index_add_(0, torch.minimum(off[:-1], off[1:]), torch.ones(n_bags, dtype=torch.int64, device=device))
    marks.index_add_(0, off[1:], -torch.ones(n_bags, dtype=torch.int64, device=device))
    fnd[torch.cumsum(marks, 0)[:n] > 0] = 0
    if pos.numel():
        rows, f = find_kept(flat[pos].contiguous(), pos)
        block[grad_index[pos].to(torch.int64)] = rows.to(block.device).to(out_dtype)
        fnd[pos] = f.to(fnd.device).to(torch.uint8)
    block = block.view(n_bags, max_len, dim)
    if out is not None:
        out.view(n_bags, max_len, dim).copy_(block)
        block = out.view(n_bags, max_len, dim)
    return (block, fnd, lengths, step_keys, grad_index) if with_step else (block, fnd, lengths)


class SparseStep(NamedTuple):
    """One sparse optimizer step as a value: which optimizer and its scalars.  The table classes build it once per call and forward it; nothing
    else in the package tells the optimizers apart.  The fields stand in the order of apply_pooled / apply_indexed's loose form, so `*step` is it.
    FTRL-Proximal (kind "ftrl") has four scalars and uses the same six fields: eps carries beta, the two beta slots carry l1 and l2 (read them as
    .l1 / .l2), step is unused."""
    kind: str            # "adagrad" | "adam" | "ftrl"
    lr: float
    eps: float           # (ftrl: beta)
    beta1: float = 0.9   # (Adam only, like beta2 and step; ftrl: l1)
    beta2: float = 0.999   # (ftrl: l2)
    step: int = 1

    @classmethod
    def of(cls, optimizer: str, lr: float, eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1, error=None, *,
           l1: float = 0.0, l2: float = 0.0) -> "SparseStep":
        """from the loose form apply_pooled / apply_indexed and the nn layers take: the one place that checks the optimizer's name and resolves
        the default eps (1e-10 for Adagrad, 1e-8 for Adam; FTRL's beta: 1.0).  For "ftrl" the regularisation strengths come from l1 / l2 alone:
        beta1 / beta2 are ignored, so that Adam's defaults can never become one.  error: the caller's exception class for an unknown name
        (ValueError in the host-logic classes); without it MeepoError(ERR_INVALID_ARG), as the library's wrappers raise."""
        if optimizer not in ("adagrad", "adam", "ftrl"):
            msg = f"optimizer must be 'adagrad' or 'adam' or 'ftrl' (got {optimizer!r})"
            raise error(msg) if error is not None else MeepoError(_lib.ERR_INVALID_ARG, msg)
        if optimizer == "ftrl":
            return cls("ftrl", lr, 1.0 if eps is None else eps, l1, l2, step)
        if eps is None:
            eps = 1e-10 if optimizer == "adagrad" else 1e-8
        return cls(optimizer, lr, eps, beta1, beta2, step)

    @classmethod
    def ftrl(cls, lr: float, beta: float = 1.0, l1: float = 0.0, l2: float = 0.0) -> "SparseStep":
        """the FTRL-Proximal step of apply_ftrl's direct form"""
        return cls("ftrl", lr, beta, l1, l2)

    @property
    def l1(self) -> float:
        """FTRL's lambda1 (the beta1 slot)"""
        return self.beta1

    @property
    def l2(self) -> float:
        """FTRL's lambda2 (the beta2 slot)"""
        return self.beta2

    def loose_kw(self) -> dict:
        """the keywords the loose form needs beside `*step`: FTRL's l1 / l2 (its beta slots are not read there); nothing for the other two"""
        return {"l1": self.beta1, "l2": self.beta2} if self.kind == "ftrl" else {}

    def tail(self) -> tuple:
        """the step's own arguments in the order of the C-ABI — and of apply_adagrad / apply_adam / apply_ftrl's positional parameters
        (ftrl: lr, beta, l1, l2)"""
        if self.kind == "adagrad":
            return (self.lr, self.eps)
        if self.kind == "ftrl":
            return (self.lr, self.eps, self.beta1, self.beta2)
        return (self.lr, self.beta1, self.beta2, self.eps, self.step)

    def launch(self, stem: str, form: str, *args, stream: int) -> None:
        """the C entry point {stem}_{kind}{form} — mee_apply_adam_located, mee_group_apply_adagrad_pooled, … — on (args…, tail…, stream)"""
        check(getattr(_lib.lib(), f"{stem}_{self.kind}{form}")(*args, *self.tail(), stream))

    def apply_to(self, table, *args, **kw) -> None:
        """table.apply_adagrad / table.apply_adam / table.apply_ftrl(args…, tail…, **kw): any object with the methods (a CPU test adapter, a
        peer-mapped table, a foreign `local`) takes the step by their positional order"""
        getattr(table, "apply_" + self.kind)(*args, *self.tail(), **kw)


class LookupTable:
    """One HBM-resident shard: int64 key -> fp32[dim] row (+ optimizer state planes).

    value_dtype=torch.bfloat16: a SERVING table whose rows are stored as bf16, 2·dim bytes per slot (SPEC.md §3 "Row storage type").  insert / assign /
    import_ round fp32 rows once (or store bf16 rows verbatim), every read widens exactly, find(out_dtype=torch.bfloat16) returns the stored bits: the
    table is indistinguishable from an fp32 table fed the rounded rows.  No optimizer, hit counters, admission or host memory; dim a multiple of 8;
    the operators outside find / find_pooled (unweighted) / insert / assign / remove / locate / export / reserve / clear raise MeepoError(ERR_UNSUPPORTED).

    int8_rows=True (value_dtype stays torch.float32 in the call; the table then reports .value_dtype == torch.int8): the other serving table — a row is stored as dim int8 codes and one fp32 scale, dim + 16 bytes per slot.  insert / assign /
    import_ take fp32 rows and quantize each once (scale = max|x| / 127, codes rounded to nearest even), every read gives code x scale: the table is
    indistinguishable from an fp32 table fed the dequantized rows (a missing key returns default_value as it is).  Rows must be finite.  Same restrictions
    and operators as a bf16-row table, dim a multiple of 16; it has no find_pooled (ERR_UNSUPPORTED) and is a member of no group."""
    supports_out_dtype = True   # its lookups can write bf16 rows (out_dtype=torch.bfloat16); the tiered / sharded / peer tables cannot
    change_log = None           # the ChangeLog track_changes() attached (SPEC.md §3 "Change log"); None: no method issues a call it did not issue before

    def __init__(self, capacity: int, dim: int, *, device: int | torch.device = 0, optimizer: int = OPT_NONE,
                 max_batch: int = 1 << 20, default_value: float = 0.0, initial_accumulator: float = 0.0,
                 initializer: int = INIT_CONSTANT, init_scale: float = 0.0, init_seed: int = 0, value_memory: int = 0, track_hits: bool = False,
                 admission: bool = False, value_dtype: torch.dtype = torch.float32, int8_rows: bool = False):
        if value_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"value_dtype must be torch.float32 or torch.bfloat16 (got {value_dtype}): rows are stored as fp32 or as bf16"
                             + (" — int8 row storage is asked for with int8_rows=True" if value_dtype == torch.int8 else ""))
        if value_dtype == torch.bfloat16:   # a serving table: checked here, before any device is needed (the library checks again)
            if optimizer != OPT_NONE:
                raise ValueError("value_dtype=torch.bfloat16 is a serving table: it has no optimizer (train in fp32, then checkpoint.load_into a bf16-row table)")
            if track_hits or admission:
                raise ValueError("value_dtype=torch.bfloat16 excludes track_hits and admission")
            if value_memory != _lib.MEM_HBM:
                raise ValueError("value_dtype=torch.bfloat16 needs value_memory = MEM_HBM (a bf16-row table is no cold tier)")
            if dim % 8:
                raise ValueError(f"value_dtype=torch.bfloat16 needs dim to be a multiple of 8 (got {dim})")
        if int8_rows:   # the same rules, and whole 16-byte groups of codes
            if value_dtype != torch.float32:
                raise ValueError("int8_rows=True excludes value_dtype=torch.bfloat16: a table has one row storage type")
            if optimizer != OPT_NONE:
                raise ValueError("int8_rows=True is a serving table: it has no optimizer (train in fp32, then checkpoint.load_into an int8-row table)")
            if track_hits or admission:
                raise ValueError("int8_rows=True excludes track_hits and admission")
            if value_memory != _lib.MEM_HBM:
                raise ValueError("int8_rows=True needs value_memory = MEM_HBM (an int8-row table is no cold tier)")
            if dim % 16:
                raise ValueError(f"int8_rows=True needs dim to be a multiple of 16 (got {dim})")
        self.value_dtype = torch.int8 if int8_rows else value_dtype   # the row storage type, as mee_table_value_dtype reports it
        L = _lib.lib()
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise MeepoError(_lib.ERR_NO_DEVICE, "LookupTable needs a HIP device; there is no CPU fallback")
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        cfg = _lib.Config(struct_size=C.sizeof(_lib.Config), device=self.device.index, capacity=capacity, dim=dim,
                          optimizer=optimizer, max_batch=max_batch, default_value=default_value,
                          initial_accumulator=initial_accumulator, initializer=initializer, init_scale=init_scale,
                          init_seed=init_seed, value_memory=value_memory,
                          flags=(_lib.FLAG_TRACK_HITS if track_hits else 0) | (_lib.FLAG_ADMISSION if admission else 0)
                          | (_lib.FLAG_BF16_ROWS if value_dtype == torch.bfloat16 else 0) | (_lib.FLAG_INT8_ROWS if int8_rows else 0))
        self.track_hits = track_hits
        # (a bf16-row table's default row is the rounded value; an int8-row table's is the fp32 value as given)
        self.default_value = float(default_value) if value_dtype != torch.bfloat16 else float(torch.tensor(default_value, dtype=torch.float32).to(torch.bfloat16))
        h = C.c_void_p()
        self._h = None
        check(L.mee_table_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._opts = dict(device=self.device, optimizer=optimizer, max_batch=max_batch, default_value=default_value,
                          initial_accumulator=initial_accumulator, initializer=initializer, init_scale=init_scale, init_seed=init_seed,
                          value_memory=value_memory, track_hits=track_hits, admission=admission, value_dtype=value_dtype, int8_rows=int8_rows)
        info = _lib.TableInfo()
        check(L.mee_table_info_get(self._h, C.byref(info)))
        self.capacity, self.n_buckets, self.max_batch = info.capacity, info.n_buckets, info.max_batch
        self.dim, self.optimizer = info.dim, info.optimizer
        self.table_bytes, self.workspace_bytes = info.table_bytes, info.workspace_bytes
        # bumped by every call that can move or free a stored row (remove / clear / reserve): slot handles taken before it
        # (the `located` rows a pooled forward hands to its backward) are stale afterwards
        self.layout_epoch = 0

    # -- lifetime ----------------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers -----------------------------------------------------------------------------------------
    def _keys(self, keys: torch.Tensor) -> torch.Tensor:
        if keys.dtype != torch.int64 or keys.device != self.device:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"keys must be int64 on {self.device}")
        return keys if keys.dim() == 1 and keys.is_contiguous() else keys.contiguous().view(-1)   # (no view object per call for a batch that is flat already)

    def _rows(self, rows: torch.Tensor, n: int) -> torch.Tensor:
        if rows.dtype != torch.float32 or rows.device != self.device or rows.numel() != n * self.dim:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"rows must be float32 [{n},{self.dim}] on {self.device}")
        return rows.contiguous()

    def _s(self) -> int:
        return _stream_ptr(self.device)

    def track_changes(self, capacity: int):
        """Attach a ChangeLog of `capacity` keys (changes.py) -> the log.  From here on every mutator — insert, insert_missing, find_or_insert_missing,
        assign, assign_plane, remove, find_or_insert[_located], apply_*, import_, move_to (both tables), evict — notes its batch's keys in it on the
        table's stream, before its own first library call; clear() invalidates it (a key set cannot name "everything").  reserve, the lookups and the
        hit-counter operators note nothing: they change nothing export returns."""
        from .changes import ChangeLog
        _lib.refuse_narrow_rows("track_changes", self)
        self.change_log = ChangeLog(capacity, self.device)
        return self.change_log

    def _note(self, k: torch.Tensor) -> None:
        """the batch's keys into the attached change log, if there is one"""
        if self.change_log is not None:
            self.change_log.note(k)

    def _bag_keys(self, keys: torch.Tensor) -> torch.Tensor:
        """_keys for the operators that take a jagged batch, which may be empty (and then of any dtype)"""
        return self._keys(keys) if keys.numel() else keys

    def _rows_found(self, out, found, n: int, out_dtype: torch.dtype = torch.float32):
        """the two result buffers of a lookup that returns a row per key"""
        return _buffer(out, "out", out_dtype, (n, self.dim), self.device), _buffer(found, "found", torch.uint8, n, self.device)

    def _in_rows(self, rows: torch.Tensor, n: int):
        """the rows of insert / assign -> (contiguous tensor, MEE_DTYPE_* of its elements).  fp32 always; bf16 for a bf16-row table, which stores them verbatim."""
        if rows.dtype == torch.bfloat16 and self.value_dtype == torch.bfloat16:
            if rows.device != self.device or rows.numel() != n * self.dim:
                raise MeepoError(_lib.ERR_INVALID_ARG, f"rows must be [{n},{self.dim}] on {self.device}")
            r = rows.contiguous()
            if r.data_ptr() % 16:   # mee_*_as: a bf16 input is read in 16-byte groups
                r = r.clone()
            return r, _lib.DTYPE_BF16
        if rows.dtype == torch.bfloat16:
            raise MeepoError(_lib.ERR_UNSUPPORTED, "bf16 rows need a table created with value_dtype=torch.bfloat16 (an fp32 table stores fp32 rows, an int8-row table quantizes fp32 rows)")
        return self._rows(rows, n), _lib.DTYPE_F32

    # -- operators (SPEC.md §3) ----------------------------------------------------------------------------
    def find(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
             want_found: bool = True, unordered: bool = False, flags: int | None = None, out_dtype: torch.dtype = torch.float32):
        """unordered=True (mee_find_unordered): the launch is not ordered behind EARLIER work of the current stream — only for independent
        requests whose keys are complete and whose output buffers nothing earlier in the stream still touches.
        flags (mee_find_ex): this call's cache policy, an OR of _lib.FIND_* — e.g. FIND_STREAM_STORES for result buffers that rotate.
        out_dtype=torch.bfloat16 (mee_find_as): the rows rounded once to bf16 by the lookup itself (SPEC.md §3 "Output type")."""
        if flags is not None and unordered:
            raise ValueError("find(flags=..., unordered=True): mee_find_ex and mee_find_unordered are separate entry points; pass one of the two")
        dt = _out_dtype(out_dtype, out)
        if dt != _lib.DTYPE_F32 and unordered:
            raise ValueError("find(unordered=True) has no bf16 form: mee_find_unordered returns fp32 rows")
        k = self._keys(keys)
        n = k.numel()
        out = _buffer(out, "out", out_dtype, (n, self.dim), self.device)
        if found is not None or want_found:
            found = _buffer(found, "found", torch.uint8, n, self.device)
        if dt != _lib.DTYPE_F32:
            check(_lib.lib().mee_find_as(self._h, k.data_ptr(), n, out.data_ptr(), dt, _ptr(found), int(flags or 0), self._s()))
            return out, found
        if flags is not None:
            check(_lib.lib().mee_find_ex(self._h, k.data_ptr(), n, out.data_ptr(), _ptr(found), int(flags), self._s()))
            return out, found
        fn = _lib.lib().mee_find_unordered if unordered else _lib.lib().mee_find
        check(fn(self._h, k.data_ptr(), n, out.data_ptr(), _ptr(found), self._s()))
        return out, found

    def find_many(self, requests):
        """Several lookups of this table in ONE launch (mee_find_many): `requests` = up to 16 key tensors, or (keys, out, found) tuples with
        preallocated outputs.  Returns [(out, found), …] — each exactly what find() returns for that request."""
        reqs, res = (_lib.FindRequest * len(requests))(), []
        for q, r in enumerate(requests):
            keys, out, found = (r if isinstance(r, tuple) else (r, None, None))
            _fp32_only(out, "find_many")
            k = self._keys(keys)
            n = k.numel()
            out, found = self._rows_found(out, found, n)
            reqs[q] = _lib.FindRequest(k.data_ptr(), n, out.data_ptr(), found.data_ptr())
            res.append((out, found, k))   # k: keeps a contiguous copy alive until the launch is enqueued
        check(_lib.lib().mee_find_many(self._h, reqs, len(requests), self._s()))
        return [(o, f) for o, f, _ in res]

    def find_capture_stats(self):
        """(nodes, merged) — mee_find_capture_stats: this table's plain finds issued under stream capture that got a kernel node of their own, and
        those that joined the node of the find in front of them."""
        nodes, merged = C.c_uint64(0), C.c_uint64(0)
        check(_lib.lib().mee_find_capture_stats(self._h, C.byref(nodes), C.byref(merged)))
        return nodes.value, merged.value

    def _bag_offsets(self, bag_offsets: torch.Tensor) -> int:
        return _n_bags(bag_offsets, self.device)

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, weights: torch.Tensor | None = None, located: torch.Tensor | None = None,
                    out_dtype: torch.dtype = torch.float32):
        """Embedding-bag lookup: bag b = keys[bag_offsets[b]:bag_offsets[b+1]] (int64 offsets on the device) -> ([n_bags, dim]
        sums or means in position order, per-key found mask).  One output row per bag is written instead of one per key.
        weights (fp32 [n], mee_find_pooled_weighted; mode "sum" only): the bag is the sum of weights[i] * row_i.  located (int64[n]
        buffer, weighted form only) receives each key's slot handle for pooled_weighted_backward / apply_*(slots=...) of the same step.
        out_dtype=torch.bfloat16 (mee_find_pooled_as): the bag is accumulated in fp32 as always and the finished row rounded once.
        mode="max": find_pooled_max(keys, bag_offsets, out, found, out_dtype=out_dtype) without its argmax; weights and located are refused."""
        if mode == "max":
            _max_mode_only(weights=weights, located=located)
            return self.find_pooled_max(keys, bag_offsets, out=out, found=found, out_dtype=out_dtype)[:2]
        dt, m = _out_dtype(out_dtype, out), _pool_mode(mode, ValueError)
        k = self._bag_keys(keys)
        n_bags = self._bag_offsets(bag_offsets)
        if weights is None and located is not None:
            raise ValueError("find_pooled(located=...) is the weighted form's output: pass weights (all ones for a plain sum)")
        n, w, located, out, _, found = _pooled_args(k, self.device, out, (n_bags, self.dim), out_dtype, found, weights, mode, located)
        if dt != _lib.DTYPE_F32:
            check(_lib.lib().mee_find_pooled_as(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), n_bags, _ptr(w), out.data_ptr(), dt, found.data_ptr(),
                                                _ptr(located), m, self._s()))
        elif w is not None:
            check(_lib.lib().mee_find_pooled_weighted(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), n_bags, w.data_ptr(), out.data_ptr(), found.data_ptr(),
                                                      _ptr(located), self._s()))
        else:
            check(_lib.lib().mee_find_pooled(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), n_bags, out.data_ptr(), found.data_ptr(), m, self._s()))
        return out, found

    def find_pooled_max(self, keys: torch.Tensor, bag_offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                        argmax: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_argmax: bool = False):
        """Max pooling (mee_find_pooled_max; torch.nn.EmbeddingBag mode="max"): bags as find_pooled's -> (out [n_bags, dim], per-key found mask, argmax
        [n_bags, dim] uint32 | None).  out[b, j] is the first greatest element j among the rows find() returns for the bag's positions — a later position
        replaces the running one only where it is greater, so ties go to the first position and a NaN counts only at the bag's first position — copied bit
        for bit; argmax[b, j] (with_argmax=True, or a buffer passed as argmax) is the batch position it came from.  An empty bag: +0.0 and 0xFFFFFFFF.
        out_dtype=torch.bfloat16: the maximum, decided in fp32, is rounded once.  fp32-row tables only."""
        k = self._bag_keys(keys)
        n_bags = self._bag_offsets(bag_offsets)
        return _find_pooled_max(_lib.lib().mee_find_pooled_max, self._h, self.device, self.dim, k, bag_offsets, n_bags, n_bags, out, found, argmax, out_dtype,
                                with_argmax)

    def pooled_max_backward(self, bag_offsets: torch.Tensor, argmax: torch.Tensor, bag_grads: torch.Tensor, n: int, grads: torch.Tensor | None = None):
        """Backward of find_pooled_max (mee_pooled_max_backward) -> grads [n, dim]: position i of bag b gets bag_grads[b, j] where argmax[b, j] == i and +0.0
        elsewhere; positions no bag covers are not written.  The table step is then apply_*(keys, grads) for bags that partition [0, n): every key of a
        bag takes a step, with zeros where it did not win (SPEC.md §3 says what that means per optimizer)."""
        n_bags = self._bag_offsets(bag_offsets)
        return _pooled_max_backward(_lib.lib().mee_pooled_max_backward, self._h, self.device, self.dim, bag_offsets, n_bags, n_bags, argmax, bag_grads, n, grads)

    def find_padded(self, keys: torch.Tensor, bag_offsets: torch.Tensor, max_len: int, keep: str = "first", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_step: bool = False):
        """Padded sequence lookup (mee_find_padded_as): bag b = keys[bag_offsets[b]:bag_offsets[b+1]] -> (out [n_bags, max_len, dim], per-key found
        mask, lengths [n_bags] int64).  out[b, j] is the row find() returns for the bag's j-th kept key, zeros behind the end of a short bag; a bag
        longer than max_len keeps its first (keep="first") or its last (keep="last") max_len keys, and a key that is cut off is not looked up
        (found 0).  Every element of `out` is written, in one launch, with no [n, dim] array in between.
        with_step=True also returns (step_keys int64 [n], grad_index int32 [n]): the table step of the lookup is
        apply_*(step_keys, dense_grad.view(n_bags * max_len, dim), grad_index=grad_index) — cut-off keys are EMPTY there and take no step."""
        k = self._bag_keys(keys)
        n_bags = self._bag_offsets(bag_offsets)
        return _find_padded(_lib.lib().mee_find_padded_as, self._h, self.device, self.dim, k, bag_offsets, n_bags, n_bags, max_len, keep, out, found,
                            out_dtype, with_step)

    def pooled_weighted_backward(self, keys: torch.Tensor, bag_offsets: torch.Tensor, weights: torch.Tensor, bag_grads: torch.Tensor,
                                 located: torch.Tensor | None = None, want_weight_grads: bool = True, grads: torch.Tensor | None = None,
                                 weight_grads: torch.Tensor | None = None):
        """Backward of find_pooled(weights=...) (mee_pooled_weighted_backward) -> (grads [n, dim] = weights[i] * bag_grads[bag(i)],
        weight_grads [n] = <bag_grads[bag(i)], row_i> or None).  The table step is then apply_*(keys, grads[, slots=located]) — for bags
        that partition [0, n): positions no bag covers get no grads (nor handles from the forward).
        located = the handles find_pooled(weights=..., located=...) of this step wrote (the rows are read through them)."""
        k = self._bag_keys(keys)
        n_bags = self._bag_offsets(bag_offsets)
        w = _check_weights(weights, "sum", k.numel(), self.device)
        g = self._rows(bag_grads, n_bags)
        loc = self._slots(located, k.numel()) if located is not None else None
        grads, weight_grads = self._weighted_grads(grads, weight_grads, want_weight_grads, k.numel())
        check(_lib.lib().mee_pooled_weighted_backward(self._h, k.data_ptr(), _ptr(loc), k.numel(), bag_offsets.data_ptr(), n_bags, w.data_ptr(), g.data_ptr(),
                                                      grads.data_ptr(), _ptr(weight_grads), self._s()))
        return grads, weight_grads

    def _weighted_grads(self, grads, weight_grads, want_weight_grads: bool, n: int):
        """the two result buffers of pooled_weighted_backward (a table's and a group's)"""
        grads = _buffer(grads, "grads", torch.float32, (n, self.dim), self.device)
        if weight_grads is not None or want_weight_grads:
            weight_grads = _buffer(weight_grads, "weight_grads", torch.float32, n, self.device)
        return grads, weight_grads

    def find_missing(self, keys: torch.Tensor, out: torch.Tensor, found: torch.Tensor) -> None:
        """Second-tier pass: fill the positions an earlier find (on another table) left with found == 0."""
        _fp32_only(out, "find_missing")
        k = self._keys(keys)
        out, found = self._rows_found(out, found, k.numel())
        check(_lib.lib().mee_find_missing(self._h, k.data_ptr(), k.numel(), out.data_ptr(), found.data_ptr(), self._s()))

    def find_counted(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                     missing_only: bool = False):
        """find (or find_missing) that also bumps the hit counter of every key it finds (track_hits tables)."""
        _fp32_only(out, "find_counted")
        k = self._keys(keys)
        n = k.numel()
        out, found = self._rows_found(out, found, n)
        check(_lib.lib().mee_find_counted(self._h, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), int(missing_only), self._s()))
        return out, found

    def hits_scan(self, min_hits: int, max_hits: int, cap: int, reset: bool = False) -> torch.Tensor:
        """Keys whose hit counter lies in [min_hits, max_hits] (at most cap); reset zeroes all counters."""
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=self.device)
        n = C.c_size_t()
        check(_lib.lib().mee_hits_scan(self._h, min_hits, min(max_hits, 0xFFFFFFFF), int(reset), out.data_ptr(), cap, C.byref(n), self._s()))
        return out[: min(n.value, cap)]

    def insert(self, keys: torch.Tensor, values: torch.Tensor) -> None:
        """values: fp32 rows (a bf16-row table rounds them once), or bf16 rows for a bf16-row table (stored verbatim, mee_insert_as)."""
        k = self._keys(keys)
        v, dt = self._in_rows(values, k.numel())
        self._note(k)
        if dt != _lib.DTYPE_F32:
            check(_lib.lib().mee_insert_as(self._h, k.data_ptr(), v.data_ptr(), dt, k.numel(), self._s()))
            return
        check(_lib.lib().mee_insert(self._h, k.data_ptr(), v.data_ptr(), k.numel(), self._s()))

    def insert_missing(self, keys: torch.Tensor, values: torch.Tensor, found: torch.Tensor) -> None:
        """insert restricted to the positions with found == 0 (tiered pairs: keys found in neither table)."""
        k = self._keys(keys)
        v = self._rows(values, k.numel())
        found = _buffer(found, "found", torch.uint8, k.numel(), self.device)
        self._note(k)
        check(_lib.lib().mee_insert_missing(self._h, k.data_ptr(), v.data_ptr(), k.numel(), found.data_ptr(), self._s()))

    def find_or_insert_missing(self, keys: torch.Tensor, out: torch.Tensor, found: torch.Tensor) -> None:
        """find_or_insert restricted to the positions with found == 0; rows of those positions are written into out."""
        _fp32_only(out, "find_or_insert_missing")
        k = self._keys(keys)
        out, found = self._rows_found(out, found, k.numel())
        self._note(k)
        check(_lib.lib().mee_find_or_insert_missing(self._h, k.data_ptr(), k.numel(), out.data_ptr(), found.data_ptr(), self._s()))

    def assign(self, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        """values as in insert()."""
        k = self._keys(keys)
        v, dt = self._in_rows(values, k.numel())
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        self._note(k)
        if dt != _lib.DTYPE_F32:
            check(_lib.lib().mee_assign_as(self._h, k.data_ptr(), v.data_ptr(), dt, k.numel(), found.data_ptr(), self._s()))
            return found
        check(_lib.lib().mee_assign(self._h, k.data_ptr(), v.data_ptr(), k.numel(), found.data_ptr(), self._s()))
        return found

    def find_plane(self, plane: int, keys: torch.Tensor):
        """find on one plane: 0 = values, 1 = acc | m | z, 2 = v | n."""
        k = self._keys(keys)
        n = k.numel()
        out = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        found = torch.empty(n, dtype=torch.uint8, device=self.device)
        check(_lib.lib().mee_find_plane(self._h, plane, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), self._s()))
        return out, found

    def assign_plane(self, plane: int, keys: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
        k = self._keys(keys)
        v = self._rows(values, k.numel())
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        self._note(k)
        check(_lib.lib().mee_assign_plane(self._h, plane, k.data_ptr(), v.data_ptr(), k.numel(), found.data_ptr(), self._s()))
        return found

    def remove(self, keys: torch.Tensor) -> torch.Tensor:
        k = self._keys(keys)
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        self._note(k)
        check(_lib.lib().mee_remove(self._h, k.data_ptr(), k.numel(), found.data_ptr(), self._s()))
        self.layout_epoch += 1
        return found

    def move_to(self, dst: "LookupTable", keys: torch.Tensor, max_moves: int | None = None, want_moved: bool = False):
        """SPEC.md §3 move (mee_move): the keys of the batch that this table holds leave it for `dst` — the values row and every optimizer plane, bit for
        bit; a key `dst` already holds is overwritten there, a key `dst` has no room for stays here (TABLE_FULL on dst).  max_moves: only the first
        max_moves batch positions whose key is stored here are served (None: all).  -> (n_moved: int64 device tensor [1], the number of DISTINCT keys
        moved; moved mask [n] uint8 | None).  Two launches (four under a limit below n), no [n, dim] buffer, no synchronisation: the count stays on the
        device.  Slot handles taken from this table before the call are stale afterwards."""
        if not isinstance(dst, LookupTable):
            raise MeepoError(_lib.ERR_INVALID_ARG, "move_to: dst must be a LookupTable")
        k = self._keys(keys)
        n = k.numel()
        n_moved = torch.empty(1, dtype=torch.int64, device=self.device)
        moved = torch.empty(n, dtype=torch.uint8, device=self.device) if want_moved else None
        limit = 0xFFFFFFFFFFFFFFFF if max_moves is None else max(0, int(max_moves))
        self._note(k)   # the keys leave this table ...
        dst._note(k)    # ... and appear (or are overwritten) in that one
        check(_lib.lib().mee_move(self._h, dst._h, k.data_ptr(), n, limit, None if moved is None else moved.data_ptr(), n_moved.data_ptr(), self._s()))
        self.layout_epoch += 1
        return n_moved, moved

    def publish_to(self, serving: "LookupTable", check: bool = True, clear: bool = False):
        """SPEC.md §3 "Publish": refresh the serving table `serving` from this tracked table, device to device — every key noted in the attached change
        log that this table holds ends up in `serving` with this table's values row (bit for bit in an fp32-row table without optimizer, rounded once
        in a bf16-row table: what serving.insert would store), every noted key this table does not hold is removed there.  A `serving` that equalled
        this table (rounded) when the log was last cleared equals it again.  One library call (ChangeLog.publish), no [n, dim] buffer.
        check=True: ONE read-back of the counts -> (upserts, removed, dropped) as ints; RuntimeError if the log was invalid (it does not name every
        change), MeepoError if keys were dropped because `serving` had no room.  check=False: -> the int64 device tensor [4] (upserts, removed,
        dropped, invalid), and nothing synchronises.  clear=True clears the log behind the publish, in stream order; the default leaves it, because
        the same log may still owe a checkpoint.save_delta (which clears it).  Nothing is noted anywhere: `serving` must not be tracked itself.
        An int8-row `serving` is refreshed by composition instead — iter_changed(with_state=False), serving.insert in max_batch chunks,
        serving.remove — which synchronises once per piece of the log whatever `check` says; it returns (upserts, removed, None), and check=True
        raises on the log's invalid word and on serving's STATUS_TABLE_FULL bit."""
        log = self.change_log
        if log is None:
            raise ValueError("publish_to: this table has no change log (track_changes(capacity) first)")
        if not isinstance(serving, LookupTable):
            raise MeepoError(_lib.ERR_INVALID_ARG, "publish_to: serving must be a LookupTable")
        if serving.change_log is not None:
            raise ValueError("publish_to: the serving table is tracked itself, and a publish notes nothing in its log")
        if serving.value_dtype == torch.int8:
            return self._publish_composed(serving, check, clear)
        counts = log.publish(self, serving)
        if clear:
            log.clear()
        return _publish_checked(counts.tolist())[:3] if check else counts

    def _publish_composed(self, serving: "LookupTable", check: bool, clear: bool):
        """publish_to into an int8-row table: the composition the operator replaces"""
        log = self.change_log
        if check and log.invalid:
            _publish_checked((0, 0, 0, 1))
        upserts = removed = 0
        for k, v, _, _, gone in log.iter_changed(self, with_state=False):
            for s in range(0, k.numel(), serving.max_batch):
                serving.insert(k[s:s + serving.max_batch], v[s:s + serving.max_batch])
            for s in range(0, gone.numel(), serving.max_batch):
                serving.remove(gone[s:s + serving.max_batch])
            upserts, removed = upserts + k.numel(), removed + gone.numel()
        if clear:
            log.clear()
        if check and serving.status() & _lib.STATUS_TABLE_FULL:
            raise MeepoError(_lib.ERR_OUT_OF_MEMORY, "publish_to: the serving table had no room for some keys (STATUS_TABLE_FULL): rebuild it with a larger capacity")
        return upserts, removed, None

    def find_or_insert(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                       min_count: int | None = None, out_dtype: torch.dtype = torch.float32):
        """min_count (tables created with admission=True): an absent key is created only once the table's count-min sketch has seen it
        requested at least min_count times (this batch included); until then its positions return the default row.
        out_dtype=torch.bfloat16 (mee_find_or_insert_as): only the returned copy is rounded, the table's rows are created in fp32."""
        dt = _out_dtype(out_dtype, out)
        if dt != _lib.DTYPE_F32 and min_count is not None:
            raise ValueError("find_or_insert(min_count=...) has no bf16 form: mee_find_or_insert_admit returns fp32 rows")
        k = self._keys(keys)
        n = k.numel()
        out, found = self._rows_found(out, found, n, out_dtype)
        self._note(k)
        if dt != _lib.DTYPE_F32:
            check(_lib.lib().mee_find_or_insert_as(self._h, k.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), self._s()))
        elif min_count is not None:
            check(_lib.lib().mee_find_or_insert_admit(self._h, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), int(min_count), self._s()))
        else:
            check(_lib.lib().mee_find_or_insert(self._h, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), self._s()))
        return out, found

    def find_or_insert_located(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                               slots: torch.Tensor | None = None, prepare_apply: bool = False, out_dtype: torch.dtype = torch.float32):
        """find_or_insert() that also returns where every key lives now (-1: reserved key / table full): the handles for
        apply_*(…, slots=…) of the same training step — the forward of a step over a growing vocabulary.
        prepare_apply: as in find_located — the launch also partitions the batch for the apply of the SAME `keys` tensor that must follow."""
        return self._located(keys, out, found, slots, out_dtype, "mee_find_or_insert_located_prepare" if prepare_apply else "mee_find_or_insert_located")

    def _located(self, keys, out, found, slots, out_dtype, fn: str):
        """the four located lookups: (rows, found, slot handles); bf16 rows through the entry point's typed form (fn + "_as")"""
        dt = _out_dtype(out_dtype, out)
        k = self._keys(keys)
        n = k.numel()
        out = _buffer(out, "out", out_dtype, (n, self.dim), self.device)   # (spelled out: this is the training step's forward)
        found = _buffer(found, "found", torch.uint8, n, self.device)
        slots = _buffer(slots, "slots", torch.int64, n, self.device)
        if fn.startswith("mee_find_or_insert"):   # the two forms that create keys; find_located is a lookup
            self._note(k)
        if dt != _lib.DTYPE_F32:
            check(getattr(_lib.lib(), fn + "_as")(self._h, k.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), slots.data_ptr(), self._s()))
        else:
            check(getattr(_lib.lib(), fn)(self._h, k.data_ptr(), n, out.data_ptr(), found.data_ptr(), slots.data_ptr(), self._s()))
        return out, found, slots

    def admission_refusal(self) -> str | None:
        """why an admitting call (min_count) is refused on this table, or None: what the nn layers ask before they take a min_count"""
        return None if self._opts["admission"] else "the table was not created with admission=True (it has no sketch)"

    def admission_decay(self, shift: int = 1) -> None:
        """Every counter of the admission sketch >>= shift (>= 32: reset): starts a new observation window."""
        check(_lib.lib().mee_admission_decay(self._h, int(shift), self._s()))

    def size(self) -> int:
        n = C.c_size_t()
        check(_lib.lib().mee_size(self._h, C.byref(n), self._s()))
        return n.value

    def status(self) -> int:
        b = C.c_uint32()
        check(_lib.lib().mee_status(self._h, C.byref(b), self._s()))
        return b.value

    def locate(self, keys: torch.Tensor):
        """-> (slot handles [n] int64, -1 = absent; found [n] uint8).  Probe only: no row is read."""
        k = self._keys(keys)
        slots = torch.empty(k.numel(), dtype=torch.int64, device=self.device)
        found = torch.empty(k.numel(), dtype=torch.uint8, device=self.device)
        check(_lib.lib().mee_locate(self._h, k.data_ptr(), k.numel(), slots.data_ptr(), found.data_ptr(), self._s()))
        return slots, found

    def plane_host_view(self, plane: int = 0):
        """numpy view [capacity, dim] float32 of one plane of a MEM_HOST_PINNED table (pinned host DRAM the device also maps): what a
        staged cold-tier transfer gathers from on the host.  Valid until reserve() / close(); the caller orders its reads."""
        import numpy as np
        ptr, stride, mem = C.c_void_p(), C.c_uint64(), C.c_uint32()
        check(_lib.lib().mee_table_plane(self._h, plane, C.byref(ptr), C.byref(stride), C.byref(mem)))
        if mem.value != _lib.MEM_HOST_PINNED:
            raise MeepoError(_lib.ERR_UNSUPPORTED, "plane_host_view: the table's planes live in HBM")
        buf = (C.c_float * (self.capacity * self.dim)).from_address(ptr.value)
        return np.frombuffer(buf, dtype=np.float32).reshape(self.capacity, self.dim)

    def probe_length(self, keys: torch.Tensor) -> float:
        """Mean number of buckets a find visits for `keys` (measurement aid); synchronises."""
        k = self._keys(keys)
        tot = C.c_uint64()
        check(_lib.lib().mee_probe_length(self._h, k.data_ptr(), k.numel(), C.byref(tot), self._s()))
        return tot.value / max(1, k.numel())

    def probe_histogram(self, keys: torch.Tensor) -> list[int]:
        """[lookups of `keys` that visit 1, 2, 3, 4-or-more buckets] (mee_probe_histogram; reserved keys visit none); synchronises."""
        k = self._keys(keys)
        h = (C.c_uint64 * 4)()
        check(_lib.lib().mee_probe_histogram(self._h, k.data_ptr(), k.numel(), h, self._s()))
        return [int(x) for x in h]

    def clear_status(self) -> None:
        check(_lib.lib().mee_clear_status(self._h, self._s()))

    def clear(self) -> None:
        if self.change_log is not None:   # "every key is gone" is nothing a key set can name: the next save must be a full one
            self.change_log.invalidate()
        check(_lib.lib().mee_clear(self._h, self._s()))
        self.layout_epoch += 1

    def set_tuning(self, name: str, value: int) -> None:
        """Performance knob (never changes results): see mee_set_tuning in the header."""
        check(_lib.lib().mee_set_tuning(self._h, name.encode(), int(value)))

    def export(self, with_state: bool = False):
        """All (key, row) pairs in unspecified order; with_state also returns the optimizer planes."""
        n = self.size()
        keys = torch.empty(n, dtype=torch.int64, device=self.device)
        vals = torch.empty((n, self.dim), dtype=torch.float32, device=self.device)
        s1 = torch.empty((n, self.dim), dtype=torch.float32, device=self.device) if with_state and self.optimizer != OPT_NONE else None
        s2 = torch.empty((n, self.dim), dtype=torch.float32, device=self.device) if with_state and self.optimizer in (OPT_ADAM, OPT_FTRL) else None
        m = C.c_size_t()
        check(_lib.lib().mee_export(self._h, keys.data_ptr(), vals.data_ptr(), s1.data_ptr() if s1 is not None else None,
                                    s2.data_ptr() if s2 is not None else None, n, C.byref(m), self._s()))
        if m.value != n:
            raise MeepoError(_lib.ERR_HIP, f"export wrote {m.value} pairs, size() said {n}")
        return (keys, vals, s1, s2) if with_state else (keys, vals)

    def export_range(self, slot_begin: int, slot_end: int, with_state: bool = False):
        """The pairs stored in slots [slot_begin, slot_end) — export in bounded pieces (checkpoints, rehash of a table
        that fills most of HBM).  Always returns (keys, values, state1 | None, state2 | None)."""
        slot_end = min(slot_end, self.capacity)
        cap = max(slot_end - slot_begin, 0)
        keys = torch.empty(cap, dtype=torch.int64, device=self.device)
        vals = torch.empty((cap, self.dim), dtype=torch.float32, device=self.device)
        s1 = torch.empty((cap, self.dim), dtype=torch.float32, device=self.device) if with_state and self.optimizer != OPT_NONE else None
        s2 = torch.empty((cap, self.dim), dtype=torch.float32, device=self.device) if with_state and self.optimizer in (OPT_ADAM, OPT_FTRL) else None
        m = C.c_size_t()
        check(_lib.lib().mee_export_range(self._h, slot_begin, slot_end, keys.data_ptr(), vals.data_ptr(),
                                          s1.data_ptr() if s1 is not None else None, s2.data_ptr() if s2 is not None else None,
                                          cap, C.byref(m), self._s()))
        n = m.value
        return keys[:n], vals[:n], (s1[:n] if s1 is not None else None), (s2[:n] if s2 is not None else None)

    def iter_export(self, chunk_slots: int = 1 << 22, with_state: bool = True):
        """Generator over export_range pieces covering the whole table (empty pieces are skipped)."""
        for b in range(0, self.capacity, chunk_slots):
            piece = self.export_range(b, b + chunk_slots, with_state)
            if piece[0].numel():
                yield piece

    def evict(self, max_hits: int = 0, limit: int = 1 << 20, reset: bool = True, *, least: bool = False, spill: bool = False, with_state: bool = True):
        """Eviction by the hit counters (track_hits tables; SPEC.md §3 evict, mee_evict): up to `limit` keys looked up at most `max_hits` times since
        the counters were last reset leave the table; their slots become reusable tombstones.  reset: every counter is zeroed afterwards (a new window).
        least=True: the keys taken are the `limit` LEAST-hit ones among them (exact; ties at the cut unspecified) — what frees n slots of a table
        near its load limit: evict(0xFFFFFFFF, n, reset=False, least=True).
        -> how many keys left (one native call, one read-back of the count); spill=True: (keys, values, state1 | None, state2 | None, hits), the
        evicted keys with their rows, optimizer planes (with_state) and counters before the call, in one shared unspecified order — what a tier
        behind this table is fed with.  Slot handles taken before the call are stale."""
        max_hits, limit = int(max_hits), int(limit)
        if limit < 0 or max_hits < 0:
            raise ValueError(f"evict: max_hits and limit must be >= 0 (got {max_hits}, {limit})")
        cap = min(limit, self.capacity) if spill else 0
        bufs = [None] * 5
        if spill:
            rows = lambda: torch.empty((cap, self.dim), dtype=torch.float32, device=self.device)
            bufs = [torch.empty(cap, dtype=torch.int64, device=self.device), rows(),
                    rows() if with_state and self.optimizer != OPT_NONE else None, rows() if with_state and self.optimizer in (OPT_ADAM, OPT_FTRL) else None,
                    torch.empty(cap, dtype=torch.uint32, device=self.device)]
        tracked = self.change_log is not None
        if tracked and not spill:   # the evicted keys must be named: an EMPTY-prefilled key buffer (EMPTY is padding to the log) takes them
            cap = min(limit, self.capacity)
            bufs[0] = torch.full((cap,), _lib.EMPTY_KEY, dtype=torch.int64, device=self.device)
        n_out = torch.empty(1, dtype=torch.int64, device=self.device)
        flags = (_lib.EVICT_LEAST if least else 0) | (_lib.EVICT_RESET if reset else 0)
        check(_lib.lib().mee_evict(self._h, min(max_hits, 0xFFFFFFFF), min(limit, 0xFFFFFFFFFFFFFFFF), flags, *[None if b is None else b.data_ptr() for b in bufs], cap,
                                   n_out.data_ptr(), self._s()))
        self.layout_epoch += 1
        if tracked and not spill:
            self._note(bufs[0])
        n = int(n_out.item())
        if tracked and spill:
            self._note(bufs[0][:n])
        return tuple(None if b is None else b[:n] for b in bufs) if spill else n

    def _counts(self, counts: torch.Tensor, n: int) -> torch.Tensor:
        """the counters of set_hits, checked before any launch: one 32-bit word per key (torch.uint32, or torch.int32 read as its bit pattern)"""
        if counts.dtype not in (torch.uint32, torch.int32) or counts.device != self.device or counts.numel() != n or not counts.is_contiguous():
            raise MeepoError(_lib.ERR_INVALID_ARG, f"counts must be contiguous uint32 (or int32) with one entry per key ({n}) on {self.device}")
        return counts.view(-1)

    def hits_of(self, keys: torch.Tensor) -> torch.Tensor:
        """The hit counter of each key (track_hits tables; mee_hits_find) -> uint32 [n]; 0 for an absent or reserved key."""
        k = self._keys(keys)
        out = torch.empty(k.numel(), dtype=torch.uint32, device=self.device)
        check(_lib.lib().mee_hits_find(self._h, k.data_ptr(), k.numel(), out.data_ptr(), self._s()))
        return out

    def set_hits(self, keys: torch.Tensor, counts: torch.Tensor) -> None:
        """Set the hit counter of each present key (mee_hits_assign): LFU state restored from a checkpoint or carried over a tier move.  Absent and
        reserved keys are ignored; of a key that occurs twice one value stays."""
        k = self._keys(keys)
        c = self._counts(counts, k.numel())
        check(_lib.lib().mee_hits_assign(self._h, k.data_ptr(), k.numel(), c.data_ptr(), self._s()))

    def hits_decay(self, shift: int = 1) -> None:
        """Every hit counter >>= shift (>= 32: zero): ages the counters instead of resetting them, so that least-hit eviction sees more than one window."""
        if int(shift) < 0:
            raise ValueError(f"hits_decay: shift must be >= 0 (got {shift})")
        check(_lib.lib().mee_hits_decay(self._h, min(int(shift), 32), self._s()))

    def save(self, path: str, chunk_slots: int = 1 << 22, extra: dict | None = None) -> int:
        """Write a checkpoint directory (see checkpoint.py for the format); returns the number of pairs written."""
        from . import checkpoint
        return checkpoint.save_table(self, path, chunk_slots, extra)

    def load(self, path: str, chunk_pairs: int | None = None, keep=None) -> int:
        """Bulk-load a checkpoint directory into this table (rows + optimizer planes); returns pairs loaded."""
        from . import checkpoint
        return checkpoint.load_into(self, path, chunk_pairs, keep)

    def import_(self, keys: torch.Tensor, values: torch.Tensor, state1: torch.Tensor | None = None,
                state2: torch.Tensor | None = None) -> None:
        """Inverse of export(with_state=True): bulk-load pairs (and optimizer state) of any length, max_batch at a time.
        The on-disk checkpoint format is exactly export's arrays: int64 keys[N], fp32 values[N, dim] (+ state planes)."""
        k = self._keys(keys)
        n = k.numel()
        v, _ = self._in_rows(values, n)
        planes = [(1, state1), (2, state2)]
        for s in range(0, n, self.max_batch):
            e = min(n, s + self.max_batch)
            self.insert(k[s:e], v[s:e])
            for plane, st in planes:
                if st is not None:
                    self.assign_plane(plane, k[s:e], self._rows(st, n)[s:e])

    def reserve(self, capacity: int) -> None:
        """Rehash IN PLACE to at least `capacity` slots (device-to-device; old and new planes must fit together)."""
        check(_lib.lib().mee_reserve(self._h, int(capacity), self._s()))
        self.layout_epoch += 1
        info = _lib.TableInfo()
        check(_lib.lib().mee_table_info_get(self._h, C.byref(info)))
        self.capacity, self.n_buckets, self.table_bytes = info.capacity, info.n_buckets, info.table_bytes

    def maybe_grow(self, max_load: float = 0.8, factor: float = 2.0) -> bool:
        """The 'dynamic' in dynamic table, as an explicit between-steps call: when size()/capacity exceeds max_load,
        reserve(factor x capacity).  Synchronises (size)."""
        if self.size() <= max_load * self.capacity:
            return False
        self.reserve(int(self.capacity * factor))
        return True

    def resized(self, capacity: int, chunk: int = 1 << 22) -> "LookupTable":
        """Rehash into a NEW table of another capacity (same options): export -> import_, state planes included.
        The table itself never resizes (SPEC.md §2); growing is this explicit copy, which needs both tables to fit
        (plus one `chunk`-slot export piece)."""
        opts = self._opts.copy()
        new = LookupTable(capacity, self.dim, **opts)
        for ek, ev, e1, e2 in self.iter_export(chunk, with_state=True):   # bounded scratch: one slot range at a time
            new.import_(ek, ev, e1, e2)
        return new

    # -- sparse optimizers (SPEC.md §4) --------------------------------------------------------------------
    def _grad_index(self, grad_index: torch.Tensor, n: int) -> torch.Tensor:
        if grad_index.device != self.device or grad_index.numel() != n:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"grad_index must hold one entry per key on {self.device}")
        return grad_index.to(torch.int32).contiguous()   # read as uint32 by the kernels: indices are < 2^31

    def _slots(self, slots: torch.Tensor, n: int) -> torch.Tensor:
        if slots.dtype != torch.int64 or slots.device != self.device or slots.numel() != n:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"slots must be the int64 handles find_located returned for these keys, on {self.device}")
        return slots.contiguous()

    def find_located(self, keys: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                     slots: torch.Tensor | None = None, prepare_apply: bool = False, out_dtype: torch.dtype = torch.float32):
        """find() that also returns each key's slot handle (-1 = absent) for apply_*(…, slots=…) of the same training step.
        prepare_apply: the training forward (mee_find_located_prepare) — the launch also partitions the batch for the apply of the SAME
        `keys` tensor that must follow (its grad-independent half runs beside the row gather)."""
        return self._located(keys, out, found, slots, out_dtype, "mee_find_located_prepare" if prepare_apply else "mee_find_located")

    def apply_adagrad(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10,
                      grad_index: torch.Tensor | None = None, slots: torch.Tensor | None = None) -> None:
        """grad_index (optional, one int per key): position i takes row grad_index[i] of grads (pooled lookups: the bag).
        slots (optional): the handles find_located returned for `keys` in this step's forward (skips the probe)."""
        self._apply(SparseStep("adagrad", lr, eps), keys, grads, grad_index, slots)

    def apply_adam(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9, beta2: float = 0.999,
                   eps: float = 1e-8, step: int = 1, grad_index: torch.Tensor | None = None, slots: torch.Tensor | None = None) -> None:
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, grads, grad_index, slots)

    def apply_ftrl(self, keys: torch.Tensor, grads: torch.Tensor, lr: float, beta: float = 1.0, l1: float = 0.0, l2: float = 0.0,
                   grad_index: torch.Tensor | None = None, slots: torch.Tensor | None = None) -> None:
        """One FTRL-Proximal step (SPEC.md §4) on a table created with optimizer=OPT_FTRL: lr and beta set the per-coordinate learning rate
        lr / (beta + sqrt(n)), l1 drives coordinates to exactly 0.0, l2 shrinks the rest.  grad_index / slots as apply_adagrad's."""
        self._apply(SparseStep.ftrl(lr, beta, l1, l2), keys, grads, grad_index, slots)

    def _apply(self, step: SparseStep, keys, grads, grad_index, slots) -> None:
        """the three forms of the step: on the forward's slot handles, on indexed gradient rows, or plain"""
        k = self._keys(keys)
        n = k.numel()
        self._note(k)
        if slots is not None:
            g = self._rows(grads, n)
            step.launch("mee_apply", "_located", self._h, k.data_ptr(), self._slots(slots, n).data_ptr(), g.data_ptr(), n, stream=self._s())
        elif grad_index is not None:
            gi = self._grad_index(grad_index, n)
            g = grads.contiguous().view(-1, self.dim)
            step.launch("mee_apply", "_indexed", self._h, k.data_ptr(), g.data_ptr(), g.shape[0], gi.data_ptr(), n, stream=self._s())
        else:
            g = self._rows(grads, n)
            step.launch("mee_apply", "", self._h, k.data_ptr(), g.data_ptr(), n, stream=self._s())

    def apply_prepare(self, keys: torch.Tensor) -> None:
        """Group + plan the next apply of `keys` ahead of time (needs no grads; may run on a side stream).  The next
        apply_adagrad / apply_adam / apply_ftrl must be given the same tensor."""
        k = self._keys(keys)
        check(_lib.lib().mee_apply_prepare(self._h, k.data_ptr(), k.numel(), self._s()))

    def apply_discard(self) -> None:
        check(_lib.lib().mee_apply_discard(self._h, self._s()))

    def dedup_keys(self, keys: torch.Tensor, miss_index: int = -1):
        """Sync-free duplicate elimination: (uniq [n] = every distinct key once, EMPTY everywhere else — also between the keys —, inverse [n] = index into uniq, or
        miss_index for reserved keys).  How many keys are distinct stays on the device."""
        k = self._keys(keys)
        n = k.numel()
        uniq = torch.empty(n, dtype=torch.int64, device=self.device)
        inverse = torch.empty(n, dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_dedup_keys(self._h, k.data_ptr(), n, uniq.data_ptr(), inverse.data_ptr(), int(miss_index), self._s()))
        return uniq, inverse

    def dedup_sum(self, keys: torch.Tensor, grads: torch.Tensor | None = None, miss_index: int = -1, compact: bool = False):
        """Duplicate-key reduction alone (mee_dedup_sum, sync-free): (uniq [n], summed rows [n, dim] | None, counts [n], inverse [n]), PADDED like
        dedup_keys — every distinct key once in `uniq`, EMPTY elsewhere (also between the keys; counts 0 there, summed rows not written), inverse[i]
        = index of keys[i] in uniq (miss_index for reserved keys).  compact=True (one host synchronisation: torch.nonzero) squeezes the padding
        out: uniq / rows / counts of exactly the distinct keys, inverse re-indexed (reserved keys keep miss_index)."""
        k = self._keys(keys)
        n = k.numel()
        g = self._rows(grads, n) if grads is not None else None
        uniq = torch.empty(n, dtype=torch.int64, device=self.device)
        gs = torch.empty((n, self.dim), dtype=torch.float32, device=self.device) if g is not None else None
        cnt = torch.empty(n, dtype=torch.int32, device=self.device)
        inv = torch.empty(n, dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_dedup_sum(self._h, k.data_ptr(), g.data_ptr() if g is not None else None, n, uniq.data_ptr(),
                                       gs.data_ptr() if gs is not None else None, cnt.data_ptr(), inv.data_ptr(), int(miss_index), self._s()))
        if not compact:
            return uniq, gs, cnt, inv
        keep = cnt > 0
        sel = torch.nonzero(keep).view(-1)
        new_index = torch.cumsum(keep.to(torch.int64), 0) - 1           # padded index -> compact index
        valid = k > _lib.RECLAIMED_KEY
        inv_c = torch.where(valid, new_index[inv.clamp(0, max(n - 1, 0))], inv) if n else inv
        return uniq[sel], (gs[sel] if gs is not None else None), cnt[sel], inv_c


class TableGroup:
    """One find launch for the lookups of many tables (same device, same dim): mee_find_grouped.

    keys = the tables' key batches concatenated, offsets = n_tables + 1 int64/uint64 bounds ON THE DEVICE (segment j =
    keys[offsets[j]:offsets[j+1]]).  Returns (rows [n, dim], found [n]) — identical to find() per table.

    Members that are ALL bf16-row tables (value_dtype == torch.bfloat16) make a bf16-row group, the serving form of a collection (serving_copy() builds
    it from a trained group): find, find_pooled (unweighted, no located buffer) and find_pooled_jagged, each bit for bit the per-member lookup; every
    training method raises MeepoError(ERR_UNSUPPORTED).  fp32-row and bf16-row tables never share a group."""
    supports_out_dtype = True
    keyed_bags = True   # find_pooled(layout="keyed", step_index=)
    change_logs = None      # the members' ChangeLogs once track_changes() ran, and ...
    _change_group = None    # ... the ChangeLogGroup that notes a jagged batch in all of them with one launch

    def track_changes(self, capacity):
        """One ChangeLog per member (capacity: an int for all, or one per member) -> the list of logs.  Each is attached to its member too — a member's own
        mutators note in the same object — and the group's mutators (find_or_insert, apply_adagrad / apply_adam / apply_ftrl, apply_pooled,
        apply_indexed, move_to) note their jagged batch in all of them with ONE launch (mee_changes_group_note) over the member offsets they already have."""
        from .changes import ChangeLogGroup
        caps = [int(capacity)] * len(self.tables) if isinstance(capacity, int) else [int(c) for c in capacity]
        if len(caps) != len(self.tables):
            raise ValueError(f"track_changes: one capacity, or one per member: {len(self.tables)} values (got {len(caps)})")
        _lib.refuse_narrow_rows("TableGroup.track_changes", self)
        self.change_logs = [t.track_changes(c) for t, c in zip(self.tables, caps)]
        self._change_group = ChangeLogGroup(self.change_logs)
        return self.change_logs

    def _note(self, k: torch.Tensor, offsets: torch.Tensor, bags_per_table: int | None = None) -> None:
        """the jagged batch into the members' change logs, if the group is tracked.  bags_per_table: `offsets` are a pooled lookup's bag offsets, and the
        member bounds are every bags_per_table-th of them (as nn._member_offsets takes them)"""
        if self._change_group is not None and k.numel() and bags_per_table != 0:
            self._change_group.note(k, offsets if bags_per_table is None else offsets[::bags_per_table].contiguous())

    def __init__(self, tables, max_apply_batch: int = 0):
        self.tables = list(tables)
        if not self.tables:
            raise ValueError("a group needs at least one table")
        self.value_dtype = _lib.group_row_dtype("TableGroup", *self.tables)
        if self.value_dtype == torch.bfloat16 and max_apply_batch != 0:   # before any device is needed (the library checks again)
            raise ValueError("a group of bf16-row tables is a serving group: max_apply_batch must be 0 (it has no optimizer step)")
        self.device, self.dim = self.tables[0].device, self.tables[0].dim
        self._min_count_cache = {}   # find_or_insert(min_count=[...]): the device copy of every per-member threshold list seen so far
        arr = (C.c_void_p * len(self.tables))(*[t._h for t in self.tables])
        h = C.c_void_p()
        self._h = None
        with torch.cuda.device(self.device):
            check(_lib.lib().mee_group_create(arr, len(self.tables), int(max_apply_batch), C.byref(h)))
        self._h = h

    @property
    def layout_epoch(self):
        """Changes whenever a member table removed, cleared or rehashed rows: located handles from before are stale."""
        return tuple(t.layout_epoch for t in self.tables)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, name: str, value: int) -> None:
        """Performance knobs of the group's own apply ("apply_kernel", "apply_skew_adapt", …: mee_set_tuning); never change results."""
        check(_lib.lib().mee_group_set_tuning(self._h, name.encode(), int(value)))

    def serving_copy(self, chunk: int = 1 << 22) -> "TableGroup":
        """The train -> serve step in memory: a bf16-row TableGroup over NEW tables, one per member, of the member's capacity, device and default value
        (rounded), filled with the member's rows — values only, rounded once on the way in — one `chunk`-slot export piece at a time, the way
        LookupTable.resized() copies.  This group and its members are left as they are.  dim must be a multiple of 8, the members in HBM."""
        if self.dim % 8:
            raise ValueError(f"serving_copy needs dim to be a multiple of 8 (got {self.dim}): a bf16 row is dim / 8 16-byte groups")
        if any(t._opts["value_memory"] != _lib.MEM_HBM for t in self.tables):
            raise ValueError("serving_copy needs every member in HBM (value_memory = MEM_HBM): a bf16-row table is no cold tier")
        copies = []
        for t in self.tables:
            new = LookupTable(t.capacity, t.dim, device=t.device, max_batch=t.max_batch, default_value=t._opts["default_value"], value_dtype=torch.bfloat16)
            for ek, ev, _, _ in t.iter_export(chunk, with_state=False):   # bounded scratch: one slot range at a time
                new.import_(ek, ev)
            copies.append(new)
        return TableGroup(copies)

    def publish_to(self, serving_group: "TableGroup", check: bool = True, clear: bool = False):
        """LookupTable.publish_to for every member over the whole of its log, in ONE launch sequence whatever the number of members
        (mee_group_publish_changed): member j of this tracked group refreshes serving_group.tables[j].  serving_group: what serving_copy() returned, or
        a group of optimizer-less fp32 tables of the same dim.  check=True: one read-back -> a list of (upserts, removed, dropped) per member;
        RuntimeError if a member's log was invalid, MeepoError if a member dropped keys.  check=False: -> the int64 device tensor [n_tables, 4], no
        synchronisation.  clear=True clears every member's log behind the publish.  The first call after a reserve() of a member of either group
        synchronises the stream once (the group re-reads that member's planes) and must not be captured."""
        if self._change_group is None:
            raise ValueError("publish_to: this group has no change logs (track_changes(capacity) first)")
        if not isinstance(serving_group, TableGroup):
            raise MeepoError(_lib.ERR_INVALID_ARG, "publish_to: serving_group must be a TableGroup")
        if serving_group._change_group is not None or any(t.change_log is not None for t in serving_group.tables):
            raise ValueError("publish_to: the serving group is tracked itself, and a publish notes nothing in its logs")
        counts = torch.empty((len(self.tables), 4), dtype=torch.int64, device=self.device)
        _lib.check(_lib.lib().mee_group_publish_changed(self._h, self._change_group._h, serving_group._h, counts.data_ptr(), _stream_ptr(self.device)))
        for t in serving_group.tables:
            t.layout_epoch += 1
        if clear:
            for log in self.change_logs:
                log.clear()
        return [_publish_checked(c, f" of member {j}")[:3] for j, c in enumerate(counts.tolist())] if check else counts

    def _check_offsets(self, offsets: torch.Tensor) -> None:
        if offsets.device != self.device or offsets.dtype not in (torch.int64, torch.uint64) or offsets.numel() != len(self.tables) + 1 \
                or not offsets.is_contiguous():
            raise MeepoError(_lib.ERR_INVALID_ARG, f"offsets must be {len(self.tables) + 1} contiguous int64 values on {self.device}")

    def move_to(self, dst_group: "TableGroup", keys: torch.Tensor, offsets: torch.Tensor, max_moves=None, want_moved: bool = False):
        """LookupTable.move_to per member on its segment of the jagged batch (mee_group_move): member j's keys leave tables[j] for dst_group.tables[j],
        in one launch sequence whatever the number of members.  max_moves: None (no limit), or one limit per member — a list, or an int64 / uint64
        tensor of n_tables entries on the device.  -> (n_moved: int64 device tensor [n_tables], distinct keys moved per member; moved mask [n] uint8 |
        None — bytes of positions outside the segments are not written).  keys.numel() may not exceed any member's max_batch.  No synchronisation."""
        if not isinstance(dst_group, TableGroup):
            raise MeepoError(_lib.ERR_INVALID_ARG, "move_to: dst_group must be a TableGroup")
        self._check_offsets(offsets)
        k = self.tables[0]._bag_keys(keys)
        n, nt = k.numel(), len(self.tables)
        limits = None
        if max_moves is not None:
            limits = max_moves if isinstance(max_moves, torch.Tensor) else torch.tensor([max(0, int(m)) for m in max_moves], dtype=torch.int64).to(self.device)
            if limits.device != self.device or limits.dtype not in (torch.int64, torch.uint64) or limits.numel() != nt or not limits.is_contiguous():
                raise MeepoError(_lib.ERR_INVALID_ARG, f"max_moves must hold {nt} int64 limits (a list, or a contiguous tensor on {self.device})")
        n_moved = torch.empty(nt, dtype=torch.int64, device=self.device)
        moved = torch.empty(n, dtype=torch.uint8, device=self.device) if want_moved else None
        self._note(k, offsets)        # the keys leave these members ...
        dst_group._note(k, offsets)   # ... and appear in those
        check(_lib.lib().mee_group_move(self._h, dst_group._h, k.data_ptr(), offsets.data_ptr(), n, None if limits is None else limits.data_ptr(),
                                        None if moved is None else moved.data_ptr(), n_moved.data_ptr(), _stream_ptr(self.device)))
        for t in self.tables:
            t.layout_epoch += 1
        return n_moved, moved

    def apply_adagrad(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, eps: float = 1e-10) -> None:
        """One sparse-Adagrad step over the jagged batch == apply_adagrad per table (max_apply_batch >= keys.numel())."""
        self._apply(SparseStep("adagrad", lr, eps), keys, offsets, grads)

    def apply_adam(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, beta1: float = 0.9,
                   beta2: float = 0.999, eps: float = 1e-8, step: int = 1) -> None:
        self._apply(SparseStep("adam", lr, eps, beta1, beta2, step), keys, offsets, grads)

    def apply_ftrl(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, lr: float, beta: float = 1.0, l1: float = 0.0,
                   l2: float = 0.0) -> None:
        """One FTRL-Proximal step over the jagged batch == apply_ftrl per table (members created with optimizer=OPT_FTRL)."""
        self._apply(SparseStep.ftrl(lr, beta, l1, l2), keys, offsets, grads)

    def _apply(self, step: SparseStep, keys, offsets, grads, index=None, pooled: bool = False, located=None) -> None:
        """the three forms of the grouped step: a gradient row per position over member segments (`offsets` = the n_tables + 1 bounds), indexed rows
        over member segments, or a pooled lookup's backward (`offsets` = its bag_offsets, index = the bag of every position)"""
        bpt = self._check_bags(offsets) if pooled else self._check_offsets(offsets)
        k = self.tables[0]._bag_keys(keys)
        n, s = k.numel(), _stream_ptr(self.device)
        self._note(k, offsets, bpt if pooled else None)
        if index is None:
            g = self.tables[0]._rows(grads, n)
            step.launch("mee_group_apply", "", self._h, k.data_ptr(), offsets.data_ptr(), g.data_ptr(), n, stream=s)
            return
        gi = self.tables[0]._grad_index(index, n)
        g = grads.contiguous()
        if pooled:
            step.launch("mee_group_apply", "_pooled", self._h, k.data_ptr(), offsets.data_ptr(), bpt, g.data_ptr(), gi.data_ptr(),
                        located.data_ptr() if located is not None else None, n, stream=s)
            return
        if g.dtype != torch.float32 or g.dim() != 2 or g.shape[1] != self.dim or g.device != self.device:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"grads must be float32 [rows, {self.dim}] on {self.device}")
        step.launch("mee_group_apply", "_indexed", self._h, k.data_ptr(), offsets.data_ptr(), g.data_ptr(), g.shape[0], gi.data_ptr(), n, stream=s)

    # -- the embedding-bag collection: bags_per_table bags per member, bag b belongs to member b // bags_per_table ---------
    def _check_bags(self, bag_offsets: torch.Tensor) -> int:
        return _check_bags(bag_offsets, len(self.tables), self.device)

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, located: torch.Tensor | None = None, weights: torch.Tensor | None = None,
                    out_dtype: torch.dtype = torch.float32, layout: str = "table", step_index: torch.Tensor | None = None):
        """find_pooled of every member in one launch -> ([n_tables * bags_per_table, dim], per-key found mask).
        located (optional int64[n] buffer) receives the located rows for apply_pooled(located=...) of the same step.
        weights (fp32 [n], mode "sum" only): the weighted form, LookupTable.find_pooled(weights=...) per member.
        layout="keyed" (unweighted): the same rows as [bags_per_table, n_tables * dim] — row s holds sample s of every member side by side, what a
        dense network reads — written by the one launch (mee_group_find_pooled_keyed); `out` may be any 2-D view with stride(1) == 1, e.g. a column
        range of a wider feature block.  step_index (a uint32 / int32 [n] buffer, keyed only) receives the bag_of_position with which apply_pooled
        reads the keyed gradient in place.
        mode="max": find_pooled_max(keys, bag_offsets, out, found, out_dtype=out_dtype) without its argmax; located, weights, layout="keyed" and
        step_index are refused."""
        if mode == "max":
            _max_mode_only(weights=weights, located=located, step_index=step_index, layout="keyed" if _check_layout(layout) else None)
            return self.find_pooled_max(keys, bag_offsets, out=out, found=found, out_dtype=out_dtype)[:2]
        keyed = _check_layout(layout)
        dt = _out_dtype(out_dtype, None if keyed else out)
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        if keyed and weights is not None:
            raise ValueError("layout='keyed' has no weighted form (per-sample weights): use the table-major lookup")
        if step_index is not None and not keyed:
            raise ValueError("step_index is the keyed layout's (layout='keyed'): the table-major step takes the bag of every position")
        m, nt, s = _pool_mode(mode), len(self.tables), _stream_ptr(self.device)
        n, w, located, out, stride, found = _pooled_args(k, self.device, out, (bpt, nt * self.dim) if keyed else (bpt * nt, self.dim), out_dtype, found, weights,
                                                         mode, located, keyed)
        if keyed:
            check(_lib.lib().mee_group_find_pooled_keyed(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), dt, stride, found.data_ptr(),
                                                         _ptr(located), _step_index(step_index, n, self.device), m, s))
        elif dt != _lib.DTYPE_F32:   # mee_group_find_pooled_as: the finished bag rows rounded once to bf16
            check(_lib.lib().mee_group_find_pooled_as(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, _ptr(w), out.data_ptr(), dt, found.data_ptr(),
                                                      _ptr(located), m, s))
        elif w is not None:
            check(_lib.lib().mee_group_find_pooled_weighted(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, w.data_ptr(), out.data_ptr(), found.data_ptr(),
                                                            _ptr(located), s))
        else:
            check(_lib.lib().mee_group_find_pooled(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), found.data_ptr(), _ptr(located), m, s))
        return out, found

    def find_pooled_max(self, keys: torch.Tensor, bag_offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                        argmax: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_argmax: bool = False):
        """LookupTable.find_pooled_max of every member on its bags_per_table bags, in one launch (mee_group_find_pooled_max) -> (out [n_tables *
        bags_per_table, dim], per-key found mask, argmax | None).  Every member uses its own default row; argmax holds positions in the whole batch."""
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        return _find_pooled_max(_lib.lib().mee_group_find_pooled_max, self._h, self.device, self.dim, k, bag_offsets, bpt * len(self.tables), bpt, out, found,
                                argmax, out_dtype, with_argmax)

    def pooled_max_backward(self, bag_offsets: torch.Tensor, argmax: torch.Tensor, bag_grads: torch.Tensor, n: int, grads: torch.Tensor | None = None):
        """LookupTable.pooled_max_backward per member, in one launch (mee_group_pooled_max_backward) -> grads [n, dim].  The step is then
        apply_adagrad / apply_adam / apply_ftrl(keys, bag_offsets[::bags_per_table].contiguous(), grads): the grads are per position."""
        bpt = self._check_bags(bag_offsets)
        return _pooled_max_backward(_lib.lib().mee_group_pooled_max_backward, self._h, self.device, self.dim, bag_offsets, bpt * len(self.tables), bpt, argmax,
                                    bag_grads, n, grads)

    def find_padded(self, keys: torch.Tensor, bag_offsets: torch.Tensor, max_len: int, keep: str = "first", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32, with_step: bool = False):
        """LookupTable.find_padded of every member on its bags_per_table bags, in one launch (mee_group_find_padded_as) ->
        (out [n_tables * bags_per_table, max_len, dim], per-key found mask, lengths) and, with_step=True, (step_keys, grad_index): the step is
        apply_indexed(step_keys, bag_offsets[::bags_per_table].contiguous(), dense_grad.view(-1, dim), grad_index, ...)."""
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        return _find_padded(_lib.lib().mee_group_find_padded_as, self._h, self.device, self.dim, k, bag_offsets, bpt * len(self.tables), bpt, max_len, keep, out,
                            found, out_dtype, with_step)

    def apply_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, bag_grads: torch.Tensor, bag_of_position: torch.Tensor,
                     optimizer: str, lr: float, eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1,
                     located: torch.Tensor | None = None, *, l1: float = 0.0, l2: float = 0.0) -> None:
        """Backward of find_pooled over the group: one optimizer step, position i takes row bag_of_position[i] of bag_grads.
        optimizer "ftrl": eps is FTRL's beta (default 1.0), l1 / l2 its regularisation strengths; beta1 / beta2 / step are not read.
        located = the buffer the forward find_pooled of this step filled: skips the probe pass.
        After find_pooled(layout="keyed", step_index=idx): bag_grads = the keyed gradient [bags_per_table, n_tables * dim] viewed
        .view(bags_per_table * n_tables, dim), bag_of_position = idx — the step reads the keyed gradient where it lies."""
        if bag_grads.dim() == 2 and bag_grads.shape[1] != self.dim:   # (a keyed gradient handed over without its view would be read as rows of `dim`)
            raise MeepoError(_lib.ERR_INVALID_ARG, f"bag_grads must be [rows, {self.dim}] (a keyed gradient: .view(-1, {self.dim}))")
        self._apply(SparseStep.of(optimizer, lr, eps, beta1, beta2, step, l1=l1, l2=l2), keys, bag_offsets, bag_grads, bag_of_position, pooled=True, located=located)

    # -- the same collection with a different number of bags per member (the owner's side of ShardedTableGroup's bags) --------
    def find_pooled_jagged(self, keys: torch.Tensor, bag_offsets: torch.Tensor, member_bags: torch.Tensor, mode: str = "sum",
                           out: torch.Tensor | None = None, found: torch.Tensor | None = None, located: torch.Tensor | None = None):
        """find_pooled where bag b belongs to the member j with member_bags[j] <= b < member_bags[j + 1] (n_tables + 1 non-decreasing int64 on the
        device; members may have no bags; bags outside the map are empty) -> ([n_bags, dim] fp32, per-key found mask).  Sync-free."""
        _fp32_only(out, "find_pooled_jagged")
        self._check_offsets(member_bags)
        nb, m = _n_bags(bag_offsets, self.device), _pool_mode(mode)
        k = self.tables[0]._bag_keys(keys)
        _no_bags_for_keys(k.numel(), nb)
        n, _, located, out, _, found = _pooled_args(k, self.device, out, (nb, self.dim), torch.float32, found, located=located)
        check(_lib.lib().mee_group_find_pooled_jagged(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), nb, member_bags.data_ptr(), out.data_ptr(),
                                                      found.data_ptr(), _ptr(located), m, _stream_ptr(self.device)))
        return out, found

    def apply_indexed(self, keys: torch.Tensor, offsets: torch.Tensor, grads: torch.Tensor, grad_index: torch.Tensor, optimizer: str, lr: float,
                      eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1, *, l1: float = 0.0, l2: float = 0.0) -> None:
        """One optimizer step over the jagged batch == LookupTable.apply_*(grad_index=...) per member with its segment: position i takes row
        grad_index[i] of grads [rows, dim].  optimizer "ftrl": eps is beta, l1 / l2 as apply_pooled's."""
        self._apply(SparseStep.of(optimizer, lr, eps, beta1, beta2, step, l1=l1, l2=l2), keys, offsets, grads, grad_index)

    def pooled_weighted_backward(self, keys: torch.Tensor, bag_offsets: torch.Tensor, weights: torch.Tensor, bag_grads: torch.Tensor,
                                 located: torch.Tensor | None = None, want_weight_grads: bool = True, grads: torch.Tensor | None = None,
                                 weight_grads: torch.Tensor | None = None):
        """LookupTable.pooled_weighted_backward per member, in one launch -> (grads [n, dim], weight_grads [n] or None).  The step is
        then apply_adagrad / apply_adam(keys, bag_offsets[::bags_per_table].contiguous(), grads): the grads are per position."""
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        w = _check_weights(weights, "sum", k.numel(), self.device)
        g = self.tables[0]._rows(bag_grads, bpt * len(self.tables))
        loc = self.tables[0]._slots(located, k.numel()) if located is not None else None
        grads, weight_grads = self.tables[0]._weighted_grads(grads, weight_grads, want_weight_grads, k.numel())
        check(_lib.lib().mee_group_pooled_weighted_backward(self._h, k.data_ptr(), _ptr(loc), k.numel(), bag_offsets.data_ptr(), bpt, w.data_ptr(), g.data_ptr(),
                                                            grads.data_ptr(), _ptr(weight_grads), _stream_ptr(self.device)))
        return grads, weight_grads

    def find_or_insert(self, keys: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
                       out_dtype: torch.dtype = torch.float32, min_count=None):
        """find that first creates absent keys in their member table (initial row / state); found = present before.
        min_count (every member created with admission=True; mee_group_find_or_insert_admit, three launches): LookupTable.find_or_insert(min_count=)
        per member on its segment, each member counting in its own sketch — an absent key is created only once that sketch has seen it asked for
        min_count times, and returns the default row until then.  An int, or one threshold per member (a sequence of n_tables ints; 0 or 1 = at
        first sight); out_dtype=torch.bfloat16 rounds the returned copy."""
        if min_count is None:
            return self.find(keys, offsets, out, found, _fn="mee_group_find_or_insert", out_dtype=out_dtype)
        scalar, per_member = self._min_counts(min_count)
        dt = _out_dtype(out_dtype, out)
        k = self.tables[0]._bag_keys(keys)
        n = k.numel()
        self._check_offsets(offsets)
        out, found = self.tables[0]._rows_found(out, found, n, out_dtype)
        self._note(k, offsets)
        check(_lib.lib().mee_group_find_or_insert_admit(self._h, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(), scalar,
                                                        per_member.data_ptr() if per_member is not None else None, _stream_ptr(self.device)))
        return out, found

    def _min_counts(self, min_count):
        """-> (scalar threshold, None) or (0, the device copy of a per-member list — made once per value, so a step uploads nothing)"""
        if isinstance(min_count, int):
            if not 0 <= min_count < 1 << 32:
                raise ValueError(f"min_count must be in [0, 2^32) (got {min_count})")
            return min_count, None
        key = tuple(int(c) for c in min_count)
        if len(key) != len(self.tables):
            raise ValueError(f"min_count must be an int or one threshold per member: {len(self.tables)} values (got {len(key)})")
        if any(not 0 <= c < 1 << 32 for c in key):
            raise ValueError(f"every min_count must be in [0, 2^32) (got {list(key)})")
        if key not in self._min_count_cache:
            import numpy as np
            self._min_count_cache[key] = torch.from_numpy(np.array(key, dtype=np.uint32).view(np.int32)).to(self.device)   # uint32 bits behind an int32 tensor
        return 0, self._min_count_cache[key]

    def admission_refusal(self) -> str | None:
        """LookupTable.admission_refusal of the first member that has one, named"""
        return next((f"member {j} of the group: {r}" for j, r in enumerate(t.admission_refusal() for t in self.tables) if r), None)

    def admission_decay(self, shift: int = 1) -> None:
        """LookupTable.admission_decay of every member in one launch (mee_group_admission_decay): every sketch counter >>= shift (>= 32: reset)."""
        check(_lib.lib().mee_group_admission_decay(self._h, int(shift), _stream_ptr(self.device)))

    def find(self, keys: torch.Tensor, offsets: torch.Tensor, out: torch.Tensor | None = None, found: torch.Tensor | None = None,
             _fn: str = "mee_find_grouped", out_dtype: torch.dtype = torch.float32):
        """out_dtype=torch.bfloat16 (mee_find_grouped_as / mee_group_find_or_insert_as): LookupTable.find(out_dtype=...) per member."""
        dt = _out_dtype(out_dtype, out)
        k = self.tables[0]._bag_keys(keys)
        n = k.numel()
        self._check_offsets(offsets)
        out, found = self.tables[0]._rows_found(out, found, n, out_dtype)
        if _fn == "mee_group_find_or_insert":   # the form that creates keys; the plain find is a lookup
            self._note(k, offsets)
        if dt != _lib.DTYPE_F32:
            check(getattr(_lib.lib(), _fn + "_as")(self._h, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), dt, found.data_ptr(),
                                                   _stream_ptr(self.device)))
        else:
            check(getattr(_lib.lib(), _fn)(self._h, k.data_ptr(), offsets.data_ptr(), n, out.data_ptr(), found.data_ptr(),
                                           _stream_ptr(self.device)))
        return out, found


def mixed_layout(dims, bags_per_table: int):
    """The output layout of a mixed group (SPEC.md §3 "Mixed groups"), as mee_mixed_group_layout reports it: a class = the members of one dim,
    classes by ascending dim, members inside a class in the caller's order; member j's block is [bags_per_table, dims[j]] and the blocks
    follow each other class by class.  -> (class order: the member indices in block order, element offset of every member's block, total elements)."""
    dims = [int(d) for d in dims]
    order = sorted(range(len(dims)), key=lambda j: (dims[j], j))
    offsets, total = [0] * len(dims), 0
    for j in order:
        offsets[j] = total
        total += int(bags_per_table) * dims[j]
    return order, offsets, total


class MixedTableGroup:
    """An embedding-bag collection whose tables differ in dim (same device): ONE pooled-lookup launch for all members, one optimizer step
    (per dim class a select launch + the TableGroup step).  Pooled lookups only: bag b belongs to member b // bags_per_table.  The output is
    one flat buffer in the class-major layout of mixed_layout(); find_pooled hands back per-member [bags_per_table, dim_j] views of it in the
    caller's order.  Equal dims: the launches of TableGroup, bit for bit."""
    supports_out_dtype = True
    weighted_bags = False
    mixed_dims = True
    keyed_bags = True   # find_pooled(layout="keyed", step_index=), apply_pooled(layout="keyed")

    def __init__(self, tables, max_apply_batch: int = 0):
        self.tables = list(tables)
        if not self.tables:
            raise ValueError("a group needs at least one table")
        _lib.refuse_narrow_rows("MixedTableGroup", *self.tables)
        self.device = self.tables[0].device
        self.dims = [t.dim for t in self.tables]
        arr = (C.c_void_p * len(self.tables))(*[t._h for t in self.tables])
        h = C.c_void_p()
        self._h = None
        with torch.cuda.device(self.device):
            check(_lib.lib().mee_mixed_group_create(arr, len(self.tables), int(max_apply_batch), C.byref(h)))
        self._h = h

    @property
    def layout_epoch(self):
        """Changes whenever a member table removed, cleared or rehashed rows: located handles from before are stale."""
        return tuple(t.layout_epoch for t in self.tables)

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_mixed_group_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, name: str, value: int) -> None:
        """Performance knobs of every class's apply (mee_set_tuning); never change results."""
        check(_lib.lib().mee_mixed_group_set_tuning(self._h, name.encode(), int(value)))

    def admission_refusal(self) -> str:
        return "a mixed-width group creates unseen ids inside its pooled launch, which has no admission"

    def layout(self, bags_per_table: int):
        """-> (element offset of every member's [bags_per_table, dim_j] block, total elements), from the library (== mixed_layout(dims, B)[1:])."""
        offs = (C.c_uint64 * len(self.tables))()
        total = C.c_uint64()
        check(_lib.lib().mee_mixed_group_layout(self._h, int(bags_per_table), offs, C.byref(total)))
        return list(offs), int(total.value)

    def keyed_layout(self):
        """-> (the column of every member in a keyed row, the row's width), from the library (== keyed_layout(dims))."""
        cols = (C.c_uint64 * len(self.tables))()
        width = C.c_uint64()
        check(_lib.lib().mee_mixed_group_keyed_layout(self._h, cols, C.byref(width)))
        return list(cols), int(width.value)

    def views(self, flat: torch.Tensor, bags_per_table: int):
        """the per-member [bags_per_table, dim_j] views of a flat class-major buffer, in the caller's member order (no copy)"""
        _, offs, _ = mixed_layout(self.dims, bags_per_table)
        return [flat[o:o + bags_per_table * d].view(bags_per_table, d) for o, d in zip(offs, self.dims)]

    def _check_bags(self, bag_offsets: torch.Tensor) -> int:
        return _check_bags(bag_offsets, len(self.tables), self.device)

    def find_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, mode: str = "sum", out: torch.Tensor | None = None,
                    found: torch.Tensor | None = None, located: torch.Tensor | None = None, weights: torch.Tensor | None = None,
                    out_dtype: torch.dtype = torch.float32, insert_missing: bool = False, layout: str = "table",
                    step_index: torch.Tensor | None = None):
        """LookupTable.find_pooled of every member with its bags, in one launch -> (views, per-key found mask): views[j] is member j's
        [bags_per_table, dim_j] view of the flat class-major buffer (`out`, or a fresh one: views[j]._base).  located (optional int64[n]
        buffer) receives the located rows for apply_pooled(located=...) of the same step.  insert_missing: absent keys are created in their
        member first (initial row / state); found = present before the call.
        layout="keyed": the first result is ONE [bags_per_table, sum(dims)] tensor instead of the views — torch.cat(views, dim=1), written by the
        launch itself (mee_mixed_group_find_pooled_keyed; `out` may be any 2-D view with stride(1) == 1); step_index (uint32 / int32 [n], keyed
        only) receives the bag of every position, the bag_of_position of apply_pooled(layout="keyed")."""
        keyed = _check_layout(layout)
        if weights is not None:
            raise ValueError("a mixed group has no weighted bags (per_sample_weights): use one TableGroup per width")
        m = _pool_mode(mode)
        if step_index is not None and not keyed:
            raise ValueError("step_index is the keyed layout's (layout='keyed')")
        dt = _out_dtype(out_dtype, None if keyed else out)
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        _no_bags_for_keys(k.numel(), bpt)
        n, _, located, out, stride, found = _pooled_args(k, self.device, out, (bpt, sum(self.dims)) if keyed else mixed_layout(self.dims, bpt)[2], out_dtype, found,
                                                         located=located, keyed=keyed)
        if keyed:
            check(_lib.lib().mee_mixed_group_find_pooled_keyed(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), dt, stride, found.data_ptr(),
                                                               _ptr(located), _step_index(step_index, n, self.device), m, int(bool(insert_missing)),
                                                               _stream_ptr(self.device)))
            return out, found
        check(_lib.lib().mee_mixed_group_find_pooled(self._h, k.data_ptr(), n, bag_offsets.data_ptr(), bpt, out.data_ptr(), dt, found.data_ptr(), _ptr(located), m,
                                                     int(bool(insert_missing)), _stream_ptr(self.device)))
        return self.views(out.view(-1), bpt), found

    def apply_pooled(self, keys: torch.Tensor, bag_offsets: torch.Tensor, bag_grads: torch.Tensor, bag_of_position: torch.Tensor,
                     optimizer: str, lr: float, eps: float | None = None, beta1: float = 0.9, beta2: float = 0.999, step: int = 1,
                     located: torch.Tensor | None = None, l1: float = 0.0, l2: float = 0.0, layout: str = "table",
                     mean_offsets: torch.Tensor | None = None) -> None:
        """Backward of find_pooled: one optimizer step, position i takes the row of bag bag_of_position[i] (its index in the caller's order)
        of bag_grads — a flat fp32 buffer in the lookup's class-major layout.  located = the buffer the forward of this step filled.
        layout="keyed": bag_grads is the keyed gradient [bags_per_table, sum(dims)] (fp32 or bf16, stride(1) == 1), bag_of_position the step_index of
        the keyed lookup; one launch (mee_mixed_group_keyed_grads) takes it apart into the group's class-major step buffer first.  mean_offsets (the
        lookup's bag_offsets; keyed only): the backward of mode "mean" — row b is divided by max(len(b), 1) on the way."""
        step = SparseStep.of(optimizer, lr, eps, beta1, beta2, step, l1=l1, l2=l2)   # ("ftrl": eps is beta, l1 / l2 the regularisation strengths)
        keyed = _check_layout(layout)
        bpt = self._check_bags(bag_offsets)
        k = self.tables[0]._bag_keys(keys)
        gi = self.tables[0]._grad_index(bag_of_position, k.numel())
        total = mixed_layout(self.dims, bpt)[2]
        if keyed:
            width = sum(self.dims)
            if bag_grads.dtype not in _OUT_DTYPES:
                raise MeepoError(_lib.ERR_INVALID_ARG, "a keyed gradient must be float32 or bfloat16")
            kg, stride = _keyed_out(bag_grads, bpt, width, bag_grads.dtype, self.device)
            if mean_offsets is not None:
                self._check_bags(mean_offsets)
            if getattr(self, "_step_grads", None) is None or self._step_grads.numel() < total:   # the group's step buffer: the launches that use it are stream-ordered
                self._step_grads = torch.empty(total, dtype=torch.float32, device=self.device)
            check(_lib.lib().mee_mixed_group_keyed_grads(self._h, kg.data_ptr(), _OUT_DTYPES[kg.dtype], stride, bpt,
                                                         mean_offsets.data_ptr() if mean_offsets is not None else None, 0 if mean_offsets is None else 1,
                                                         self._step_grads.data_ptr(), _stream_ptr(self.device)))
            bag_grads = self._step_grads[:total]
        elif mean_offsets is not None:
            raise ValueError("mean_offsets is the keyed layout's (layout='keyed')")
        g = _buffer(bag_grads.contiguous(), "bag_grads", torch.float32, total, self.device)
        if located is not None:
            located = _buffer(located, "located", torch.int64, k.numel(), self.device)
        step.launch("mee_mixed_group_apply", "_pooled", self._h, k.data_ptr(), bag_offsets.data_ptr(), bpt, g.data_ptr(), gi.data_ptr(), _ptr(located), k.numel(),
                    stream=_stream_ptr(self.device))


def hash_batch(keys: torch.Tensor, n_buckets: int, n_shards: int):
    """SPEC.md §1 on device: (mix64, bucket, owner) as int64/int64/int32 tensors (bit patterns of the unsigned values)."""
    k = keys.contiguous().view(-1)
    n = k.numel()
    mix = torch.empty(n, dtype=torch.int64, device=k.device)
    bkt = torch.empty(n, dtype=torch.int64, device=k.device)
    own = torch.empty(n, dtype=torch.int32, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().mee_hash_batch(k.data_ptr(), n, n_buckets, n_shards, mix.data_ptr(), bkt.data_ptr(), own.data_ptr(),
                                        _stream_ptr(k.device)))
    return mix, bkt, own


class Router:
    """Shard partition / un-permute kernels (SPEC.md §5) with their workspace."""

    def __init__(self, n_shards: int, max_batch: int, device: int | torch.device = 0):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.n_shards, self.max_batch = n_shards, max_batch
        h = C.c_void_p()
        self._h = None
        check(_lib.lib().mee_router_create(self.device.index, max_batch, n_shards, C.byref(h)))
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            _lib.lib().mee_router_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def owner(self, keys: torch.Tensor) -> torch.Tensor:
        """owner(key) under this router's shard count (SPEC.md §5), int64 per key."""
        return hash_batch(keys, 1, self.n_shards)[2].to(torch.int64)

    def partition(self, keys: torch.Tensor, skip_padding: bool = False):
        """Stable partition by owner -> (send_keys, counts, perm).  skip_padding: EMPTY keys belong to no shard (only the first
        counts.sum() entries of send_keys / perm are meaningful)."""
        k = keys.contiguous().view(-1)
        n = k.numel()
        send = torch.empty_like(k)
        counts = torch.empty(self.n_shards, dtype=torch.int64, device=self.device)
        perm = torch.empty(n, dtype=torch.int64, device=self.device)
        fn = _lib.lib().mee_partition_padded if skip_padding else _lib.lib().mee_partition
        check(fn(self._h, k.data_ptr(), n, send.data_ptr(), counts.data_ptr(), perm.data_ptr(), _stream_ptr(self.device)))
        return send, counts, perm

    def scatter_rows(self, rows: torch.Tensor, perm: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """out[perm[q]] = rows[q]"""
        r = rows.contiguous()
        n = perm.numel()
        if out is None:
            out = torch.empty_like(r)
        rb = r.numel() * r.element_size() // max(n, 1)
        with torch.cuda.device(self.device):
            check(_lib.lib().mee_scatter_rows(r.data_ptr(), perm.data_ptr(), n, rb, out.data_ptr(), _stream_ptr(self.device)))
        return out

    def gather_rows(self, rows: torch.Tensor, perm: torch.Tensor, out: torch.Tensor | None = None, n_out: int | None = None) -> torch.Tensor:
        """out[q] = rows[perm[q]] for q < perm.numel(); `rows` may have a different number of rows than `perm`."""
        r = rows.contiguous()
        n = perm.numel()
        rb = r.numel() * r.element_size() // max(r.shape[0], 1) if r.dim() >= 1 and r.shape[0] else 0
        if out is None:
            out = torch.empty((n,) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device)
        with torch.cuda.device(self.device):
            check(_lib.lib().mee_gather_rows(r.data_ptr(), perm.data_ptr(), n, rb, out.data_ptr(), _stream_ptr(self.device)))
        return out

    # -- embedding bags over a sharded table (SPEC.md §5 "Pooled lookups") -----------------------------------------------
    def bag_runs(self, perm: torch.Tensor, counts: torch.Tensor, bag_offsets: torch.Tensor):
        """The runs of a partitioned batch (mee_bag_runs): (run_bag [n], run_len [n], run_counts [n_shards]) — int32 / int32 / int64, the
        runs in segment order; only the first run_counts.sum() entries of run_bag / run_len are meaningful.  Sync-free."""
        n, n_bags = perm.numel(), _n_bags(bag_offsets, self.device)
        run_bag = torch.empty(n, dtype=torch.int32, device=self.device)
        run_len = torch.empty(n, dtype=torch.int32, device=self.device)
        run_counts = torch.empty(self.n_shards, dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_bag_runs(self._h, perm.data_ptr(), counts.data_ptr(), n, bag_offsets.data_ptr(), n_bags, run_bag.data_ptr(),
                                      run_len.data_ptr(), run_counts.data_ptr(), _stream_ptr(self.device)))
        return run_bag, run_len, run_counts

    def run_offsets(self, run_len: torch.Tensor, n_keys: int | None = None):
        """The owner's side (mee_run_offsets): received run lengths -> (offsets [R + 1] int64 = the bag_offsets of the local find_pooled,
        run_of_key [n_keys] int32 = the grad_index of the local indexed apply, or None without n_keys)."""
        rl = run_len.contiguous()
        offsets = torch.empty(rl.numel() + 1, dtype=torch.int64, device=self.device)
        rok = torch.empty(n_keys, dtype=torch.int32, device=self.device) if n_keys is not None else None
        check(_lib.lib().mee_run_offsets(self._h, rl.data_ptr(), rl.numel(), offsets.data_ptr(), rok.data_ptr() if rok is not None else None,
                                         n_keys or 0, _stream_ptr(self.device)))
        return offsets, rok

    def combine_bag_runs(self, partials: torch.Tensor, run_bag: torch.Tensor, run_counts: torch.Tensor, bag_offsets: torch.Tensor,
                         mode: str = "sum", out: torch.Tensor | None = None, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """out[b] = the owners' partial rows of bag b added up in rank order (mee_combine_bag_runs), mean then divided by the bag length,
        bf16 then rounded once.  partials [R, dim] fp32 in the run order of bag_runs."""
        dt, m = _out_dtype(out_dtype, out), _pool_mode(mode, ValueError)
        n_bags = _n_bags(bag_offsets, self.device)
        p = partials.contiguous()
        if p.dtype != torch.float32 or p.dim() != 2:
            raise MeepoError(_lib.ERR_INVALID_ARG, "partials must be float32 [n_runs, dim]")
        out = _buffer(out, "out", out_dtype, (n_bags, p.shape[1]), self.device)
        check(_lib.lib().mee_combine_bag_runs(self._h, p.data_ptr(), run_bag.data_ptr(), run_counts.data_ptr(), p.shape[0], bag_offsets.data_ptr(),
                                              n_bags, p.shape[1], m, out.data_ptr(), dt, _stream_ptr(self.device)))
        return out

    # -- table groups over sharded tables (SPEC.md §5 "Groups") ------------------------------------------------------------
    def segment_counts(self, perm: torch.Tensor, counts: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        """The cells of a partitioned jagged batch (mee_segment_counts) -> int64 [n_shards, n_tables]: cell (p, j) = the entries of owner segment p whose
        batch position lies in member segment j = [offsets[j], offsets[j + 1]).  Row p is what rank p is sent as counts.  Sync-free."""
        if offsets.device != self.device or offsets.dtype not in (torch.int64, torch.uint64) or offsets.dim() != 1 or offsets.numel() < 2 \
                or not offsets.is_contiguous():
            raise MeepoError(_lib.ERR_INVALID_ARG, f"offsets must be n_tables + 1 contiguous int64 values on {self.device}")
        n_tables = offsets.numel() - 1
        cells = torch.empty((self.n_shards, n_tables), dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_segment_counts(self._h, perm.data_ptr(), counts.data_ptr(), perm.numel(), offsets.data_ptr(), n_tables, cells.data_ptr(),
                                            _stream_ptr(self.device)))
        return cells

    def regroup(self, recv_keys: torch.Tensor, recv_cells: torch.Tensor):
        """The owner's side (mee_regroup): the received keys, source-major (source 0's members 0 … T-1, then source 1's, …; recv_cells int64
        [n_shards, T] on the device = the received cell counts) -> (keys [n] table-major = member j, inside it source rank ascending, inside that
        arrival order; order [n] int64 = the source-major index of every table-major position, for gather_rows / scatter_rows; offsets [T + 1] int64 =
        the member offsets of the regrouped batch, what TableGroup's operators take).  Sync-free."""
        k = recv_keys.contiguous().view(-1)
        c = recv_cells.contiguous()
        if c.device != self.device or c.dtype not in (torch.int64, torch.uint64) or c.dim() != 2 or c.shape[0] != self.n_shards or c.shape[1] < 1:
            raise MeepoError(_lib.ERR_INVALID_ARG, f"recv_cells must be int64 [{self.n_shards}, n_tables] on {self.device}")
        n, n_tables = k.numel(), c.shape[1]
        keys_out = torch.empty_like(k)
        order = torch.empty(n, dtype=torch.int64, device=self.device)
        offsets = torch.empty(n_tables + 1, dtype=torch.int64, device=self.device)
        check(_lib.lib().mee_regroup(self._h, k.data_ptr(), c.data_ptr(), n, n_tables, keys_out.data_ptr(), order.data_ptr(), offsets.data_ptr(),
                                     _stream_ptr(self.device)))
        return keys_out, order, offsets
