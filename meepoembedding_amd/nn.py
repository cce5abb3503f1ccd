"""The caller side of the boundary: the lookup table as a trainable torch layer, registered as
`torch.library` custom ops on PyTorch-ROCm.

    meepo::lookup(keys, anchor, table_id, insert_missing) -> rows     forward  = find_or_insert (training: unseen ids get
                                                                                 their hashed initial row) or find (eval)
    meepo::apply_grad(keys, grad_rows, table_id)                      backward = the table's own sparse optimizer
                                                                                 (apply_adagrad / apply_adam), fed with
                                                                                 the dense grad of the output
    meepo::lookup_located / meepo::apply_grad_located                 the same pair over ONE HBM table: the forward
                                                                                 (find[_or_insert]_located) hands every key's slot
                                                                                 to the backward, whose apply then does not probe
    meepo::lookup_padded / meepo::apply_grad_padded                   padded sequences: [n_bags, max_len, dim], the backward an indexed step
    meepo::lookup_pooled[_weighted] / meepo::apply_grad_pooled[_weighted]   embedding bags (sum / mean; weighted sum with the grad of
                                                                                 the per-sample weights)
    meepo::lookup_pooled_max / meepo::apply_grad_pooled_max           embedding bags, mode "max": the lookup also hands out the winning position of
                                                                                 every element, from which the backward builds the [n, dim] grads its step takes
    meepo::lookup_pooled_keyed / meepo::apply_grad_pooled_keyed      a group's bags as [bags_per_table, sum of dims] (layout="keyed"): the lookup
                                                                                 writes that block and the index its step reads the gradient with

The update happens INSIDE backward, so the layer has no torch parameters and needs no torch optimizer.  Both ops have
fake (meta) kernels, so a model containing the layer traces and exports; they are opaque to the tracer (the table is
state outside the graph, addressed by `table_id`).  Plumbing only: no kernel lives here.
Reference anchor: /root/reference/README.md:2 ("Embedding designed for recommendation … systems").

What a table declares (tables are duck-typed; _traits() reads all of it once, when a layer is built, and nothing else here looks at a table's
type or attributes).  Always: dim, find, find_or_insert, apply_adagrad, apply_adam with LookupTable's (a group: TableGroup's) parameters.
    apply_ftrl                          optimizer="ftrl" can be served (a group instead: its apply_pooled / apply_indexed take l1=, l2=, and apply_ftrl serves
                                        the collection layer); without it a layer built with optimizer="ftrl" is refused at construction
Class-level flags, with the default that holds when a class says nothing:
    supports_out_dtype = False          its lookups take out_dtype=torch.bfloat16
    supports_pooled_out_dtype = False   its find_pooled does, though its find does not (may be set per instance: TieredLookupTable)
    weighted_bags = True                find_pooled(weights=, located=) and pooled_weighted_backward exist
    pools_with_insert = False           find_pooled(insert_missing=[, min_count=]) creates unseen ids itself and hands out no located rows
    mixed_dims = False                  members of different dims: find_pooled(out=flat, located=, insert_missing=), views(), dims
    hot_cold_pair = False               a hot/cold pair: DynamicEmbedding has no admitting forward over it
    keyed_bags = False                  a group whose find_pooled takes layout="keyed", step_index= (and a mixed group's apply_pooled layout="keyed",
                                        mean_offsets=); without it DynamicEmbeddingBag(layout="keyed") composes the table-major lookup and one permute
Optional methods:
    apply_pooled                        a group: bag b belongs to member b // bags_per_table, `tables` lists the members, the step is apply_pooled
    find_located, find_or_insert_located, apply_discard, max_batch      ONE table whose lookups hand out slot handles for apply_*(slots=)
    layout_epoch                        changes when stored rows move: handles a forward took are dropped by its backward
    find_padded                         the padded sequence lookup in one launch (LookupTable, TableGroup, TieredLookupTable, TieredTableGroup; the step
                                        is then apply_*(grad_index=) / a group's apply_indexed); without it DynamicEmbeddingSequence composes it from find
    find_pooled_max, pooled_max_backward   max pooling in one launch each (LookupTable, TableGroup); without them DynamicEmbeddingBag(mode="max") is refused
    admission_refusal() -> str | None   why a layer's min_count is refused over this table (None: it admits); a class without the method has
                                        no admission
`_nn_prepared` on a table with find_located is this module's: the (tensor, length) whose apply partition the last training forward left pending.
"""
from __future__ import annotations

import inspect
import itertools
import weakref
from typing import Callable, NamedTuple

import torch

from ._lib import refuse_narrow_rows as _refuse_narrow_rows
from .table import SparseStep, _padded_places, mixed_layout

_LAYERS: "weakref.WeakValueDictionary[int, _SparseLayer]" = weakref.WeakValueDictionary()
_IDS = itertools.count(1)


class _Traits(NamedTuple):
    grouped: bool             # bags belong to members; the pooled step is apply_pooled
    hands_located: bool       # lookup_pooled returns the located rows of its keys (a TableGroup on one device), not an empty tensor
    located_table: bool       # one table whose lookups hand out slot handles
    pools_with_insert: bool
    weighted_bags: bool
    mixed_dims: bool
    bf16_rows: bool
    bf16_bags: bool
    hot_cold_pair: bool
    has_epoch: bool
    admission_refusal: Callable[[], str | None] | None
    ftrl: bool                # optimizer="ftrl" can be served: apply_ftrl exists (a group: its apply_pooled takes l1= / l2=)
    native_padded: bool = False   # find_padded exists (one launch; pairs and tiered groups too); without it DynamicEmbeddingSequence composes find and a placement
    native_keyed: bool = False    # find_pooled(layout="keyed") exists (one launch writes [bags_per_table, sum of dims]); without it the bag layer composes a permute


def _traits(table) -> _Traits:
    """The protocol of the module docstring, read off a table once.  Only class-level things are looked at (and supports_pooled_out_dtype, which a
    pair sets in __init__), so an object made without __init__ has its class's traits."""
    grouped, inserts = hasattr(table, "apply_pooled"), bool(getattr(table, "pools_with_insert", False))
    located_table = hasattr(table, "find_or_insert_located")
    if located_table and not hasattr(table, "_nn_prepared"):
        table._nn_prepared = None   # kept on the table, not on a layer: two layers over one table see each other's pending partition
    bf16_rows = bool(getattr(table, "supports_out_dtype", False))
    ftrl = _takes_keyword(table.apply_pooled, "l1") if grouped else hasattr(table, "apply_ftrl")   # (a MixedTableGroup has the loose form alone)
    return _Traits(grouped, grouped and not inserts, located_table, inserts, bool(getattr(table, "weighted_bags", True)),
                   bool(getattr(table, "mixed_dims", False)), bf16_rows, bf16_rows or bool(getattr(table, "supports_pooled_out_dtype", False)),
                   bool(getattr(table, "hot_cold_pair", False)), hasattr(table, "layout_epoch"), getattr(table, "admission_refusal", None), ftrl,
                   hasattr(table, "find_padded"), bool(getattr(table, "keyed_bags", False)))


def _takes_keyword(fn, name: str) -> bool:
    try:
        return name in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False


def _admit_kw(layer) -> dict:
    """the creating lookup's min_count keyword — only when the layer has one, so tables without the keyword keep working"""
    return {} if layer.min_count is None else {"min_count": layer.min_count}


def _dtype_kw(layer) -> dict:
    """the lookup's out_dtype keyword — only when it is not the default, so tables without the keyword keep working at fp32"""
    return {} if layer.out_dtype == torch.float32 else {"out_dtype": layer.out_dtype}


def _layer(table_id: int) -> "_SparseLayer":
    try:
        return _LAYERS[table_id]
    except KeyError:
        raise RuntimeError(f"meepo: no live DynamicEmbedding with table_id {table_id}") from None


def _step_now(layer) -> SparseStep:
    """the optimizer step a backward takes: the layer's settings as they are now (a schedule may have changed lr) and its next step number"""
    layer.step += 1
    if layer.optimizer == "ftrl":   # eps is beta; the regularisation strengths stand in the beta slots
        return SparseStep("ftrl", layer.lr, layer.eps, layer.l1, layer.l2, layer.step)
    return SparseStep(layer.optimizer, layer.lr, layer.eps, layer.betas[0], layer.betas[1], layer.step)


def _bag_of(keys, bag_offsets):
    """-> (length of every bag, bag index of every position)"""
    lens = bag_offsets[1:] - bag_offsets[:-1]
    return lens, torch.repeat_interleave(torch.arange(lens.numel(), device=keys.device), lens, output_size=keys.numel())


def _member_offsets(group, bag_offsets):
    """the members' key offsets of a bag batch over a group: member j holds the bags [j * bags_per_table, (j + 1) * bags_per_table)"""
    return bag_offsets[::(bag_offsets.numel() - 1) // len(group.tables)].contiguous()


def _create_unseen(layer, keys, bag_offsets) -> None:
    """dynamic vocabulary (create_missing, training): unseen ids enter their table (hashed initial row + optimizer state) before the pooled lookup"""
    if layer.create_missing and layer.training and keys.numel():
        if layer.traits.grouped:
            layer.table.find_or_insert(keys, _member_offsets(layer.table, bag_offsets), **_admit_kw(layer))
        else:
            layer.table.find_or_insert(keys, **_admit_kw(layer))


def _epoch(table_id: int):
    layer = _layer(table_id)
    return layer.table.layout_epoch if layer.traits.has_epoch else None


def _save_epoch(ctx, table_id: int) -> None:
    """setup of a forward that hands slot handles to its backward: they are valid only while no table removes / clears / rehashes rows"""
    ctx.table_id, ctx.layout_epoch = table_id, _epoch(table_id)


def _fresh(ctx, located):
    """the forward's handles, or an empty tensor when a table changed between forward and backward: the step then probes for itself"""
    return located if _epoch(ctx.table_id) == ctx.layout_epoch else located.new_empty(0)


@torch.library.custom_op("meepo::lookup", mutates_args=())
def lookup(keys: torch.Tensor, anchor: torch.Tensor, table_id: int, insert_missing: bool) -> torch.Tensor:
    layer = _layer(table_id)
    flat = keys.reshape(-1)
    rows, _ = layer.table.find_or_insert(flat, **_admit_kw(layer)) if insert_missing else layer.table.find(flat)
    return rows.reshape(*keys.shape, layer.table.dim).clone()   # never alias the table's / exchange's buffers


@lookup.register_fake
def _(keys, anchor, table_id, insert_missing):
    return keys.new_empty((*keys.shape, _layer(table_id).table.dim), dtype=torch.float32)


@torch.library.custom_op("meepo::apply_grad", mutates_args=())
def apply_grad(keys: torch.Tensor, grad_rows: torch.Tensor, table_id: int) -> None:
    layer = _layer(table_id)
    g = grad_rows.reshape(-1, layer.table.dim).contiguous()
    _step_now(layer).apply_to(layer.table, keys.reshape(-1), g)


@apply_grad.register_fake
def _(keys, grad_rows, table_id):
    return None


def _setup(ctx, inputs, output):
    keys, _, table_id, _ = inputs
    ctx.save_for_backward(keys)
    ctx.table_id = table_id


def _backward(ctx, grad_out):
    (keys,) = ctx.saved_tensors
    apply_grad(keys, grad_out.contiguous().to(torch.float32), ctx.table_id)
    return None, None, None, None


lookup.register_autograd(_backward, setup_context=_setup)


# ---- the same pair for a plain HBM table: the forward hands its slot handles to the backward, whose apply then does not probe ------
@torch.library.custom_op("meepo::lookup_located", mutates_args=())
def lookup_located(keys: torch.Tensor, anchor: torch.Tensor, table_id: int, insert_missing: bool, prepare: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (rows [..., dim], slot handle of every key (-1 = absent) for the backward of this step).
    prepare: a backward for exactly these keys follows — the lookup's launch also partitions the batch for its apply (mee_find_located_prepare /
    mee_find_or_insert_located_prepare).  A partition that no backward consumed (a forward without backward, a second layer over the same
    table) is dropped here before the next one is made."""
    layer = _layer(table_id)
    table = layer.table
    flat = keys.reshape(-1)
    if table._nn_prepared is not None:   # an earlier forward's partition that no backward used
        table.apply_discard()
        table._nn_prepared = None
    prepare = prepare and flat.is_contiguous() and flat.numel() > 0 and flat.numel() <= table.max_batch
    rows, _, slots = (table.find_or_insert_located(flat, prepare_apply=prepare, **_dtype_kw(layer)) if insert_missing
                      else table.find_located(flat, prepare_apply=prepare, **_dtype_kw(layer)))
    if prepare:
        table._nn_prepared = (flat.data_ptr(), flat.numel())
    return rows.reshape(*keys.shape, table.dim), slots   # fresh tensors: nothing aliases the table


@lookup_located.register_fake
def _(keys, anchor, table_id, insert_missing, prepare=False):
    layer = _layer(table_id)
    return keys.new_empty((*keys.shape, layer.table.dim), dtype=layer.out_dtype), keys.new_empty(keys.numel())


@torch.library.custom_op("meepo::apply_grad_located", mutates_args=())
def apply_grad_located(keys: torch.Tensor, grad_rows: torch.Tensor, located: torch.Tensor, table_id: int) -> None:
    layer = _layer(table_id)
    g = grad_rows.reshape(-1, layer.table.dim).contiguous()
    slots = located if located.numel() == keys.numel() else None
    step = _step_now(layer)
    prepared = layer.table._nn_prepared
    if prepared is not None:   # the forward's partition is for exactly (this tensor, this length), or it is dropped
        flat = keys.reshape(-1)
        if prepared != (flat.data_ptr(), flat.numel()):
            layer.table.apply_discard()
        layer.table._nn_prepared = None
    step.apply_to(layer.table, keys.reshape(-1), g, slots=slots)


@apply_grad_located.register_fake
def _(keys, grad_rows, located, table_id):
    return None


def _setup_located(ctx, inputs, output):
    keys, _, table_id = inputs[:3]
    ctx.save_for_backward(keys, output[1])
    _save_epoch(ctx, table_id)
    ctx.mark_non_differentiable(output[1])


def _backward_located(ctx, grad_out, _grad_located):
    keys, located = ctx.saved_tensors
    apply_grad_located(keys, grad_out.contiguous().to(torch.float32), _fresh(ctx, located), ctx.table_id)   # a bf16 layer's grad is widened (exact): the step is the fp32 step
    return None, None, None, None, None


lookup_located.register_autograd(_backward_located, setup_context=_setup_located)


# ---- pooled: sum / mean per bag fused into the lookup, the bag's grad row indexed in the update ---------------------------
@torch.library.custom_op("meepo::lookup_pooled", mutates_args=())
def lookup_pooled(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, mean: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (pooled rows [n_bags, dim], located rows [n] — per-position handles the backward of this step reuses; empty for a
    single table, whose apply probes for itself)"""
    layer = _layer(table_id)
    if layer.traits.pools_with_insert:   # a ShardedLookupTable / ShardedTableGroup: the owners create unseen ids inside the pooled lookup's own exchange
        creates = layer.create_missing and layer.training
        out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", insert_missing=creates, **_dtype_kw(layer),
                                         **(_admit_kw(layer) if creates else {}))   # (min_count: a TieredTableGroup, whose creation pass admits)
        return out, keys.new_empty(0)
    _create_unseen(layer, keys, bag_offsets)
    if layer.traits.grouped:   # a TableGroup
        located = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
        out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", located=located, **_dtype_kw(layer))
        return out, located
    out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", **_dtype_kw(layer))
    return out, keys.new_empty(0)


@lookup_pooled.register_fake
def _(keys, bag_offsets, anchor, table_id, mean):
    layer = _layer(table_id)
    return (keys.new_empty((bag_offsets.numel() - 1, layer.table.dim), dtype=layer.out_dtype),
            keys.new_empty(keys.numel() if layer.traits.hands_located else 0))


@torch.library.custom_op("meepo::apply_grad_pooled", mutates_args=())
def apply_grad_pooled(keys: torch.Tensor, bag_offsets: torch.Tensor, grad_bags: torch.Tensor, located: torch.Tensor, table_id: int, mean: bool) -> None:
    layer = _layer(table_id)
    lens, bag_of = _bag_of(keys, bag_offsets)
    g = grad_bags.contiguous()
    if mean:   # d mean / d row = 1 / length for every member of the bag
        g = g / lens.clamp(min=1).to(torch.float32)[:, None]
    step = _step_now(layer)
    if layer.traits.grouped:   # a TableGroup: the whole collection in one step, on the rows the forward located
        layer.table.apply_pooled(keys, bag_offsets, g, bag_of, *step, located=located if located.numel() == keys.numel() else None, **step.loose_kw())
    else:
        step.apply_to(layer.table, keys, g, grad_index=bag_of)


@apply_grad_pooled.register_fake
def _(keys, bag_offsets, grad_bags, located, table_id, mean):
    return None


def _setup_pooled(ctx, inputs, output):
    keys, bag_offsets, _, table_id, mean = inputs
    ctx.save_for_backward(keys, bag_offsets, output[1])
    ctx.mean = mean
    _save_epoch(ctx, table_id)
    ctx.mark_non_differentiable(output[1])


def _backward_pooled(ctx, grad_out, _grad_located):
    keys, bag_offsets, located = ctx.saved_tensors
    apply_grad_pooled(keys, bag_offsets, grad_out.contiguous().to(torch.float32), _fresh(ctx, located), ctx.table_id, ctx.mean)   # widened BEFORE the mean's division
    return None, None, None, None, None


lookup_pooled.register_autograd(_backward_pooled, setup_context=_setup_pooled)


# ---- pooled over a MixedTableGroup (members of different dims): one lookup op whose flat class-major buffer the layer views per member --------
@torch.library.custom_op("meepo::lookup_pooled_mixed", mutates_args=())
def lookup_pooled_mixed(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, mean: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (the flat class-major buffer of every member's pooled rows (table.mixed_layout), located rows [n] for the backward of this step)"""
    layer = _layer(table_id)
    group = layer.table
    located = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
    flat = torch.empty(_mixed_total(group, bag_offsets), dtype=layer.out_dtype, device=keys.device)
    group.find_pooled(keys, bag_offsets, "mean" if mean else "sum", out=flat, located=located, out_dtype=layer.out_dtype,
                      insert_missing=layer.create_missing and layer.training)
    return flat, located


def _mixed_total(group, bag_offsets) -> int:
    return mixed_layout(group.dims, (bag_offsets.numel() - 1) // len(group.tables))[2]


@lookup_pooled_mixed.register_fake
def _(keys, bag_offsets, anchor, table_id, mean):
    layer = _layer(table_id)
    return keys.new_empty(_mixed_total(layer.table, bag_offsets), dtype=layer.out_dtype), keys.new_empty(keys.numel())


@torch.library.custom_op("meepo::apply_grad_pooled_mixed", mutates_args=())
def apply_grad_pooled_mixed(keys: torch.Tensor, bag_offsets: torch.Tensor, grad_flat: torch.Tensor, located: torch.Tensor, table_id: int, mean: bool) -> None:
    layer = _layer(table_id)
    group = layer.table
    lens, bag_of = _bag_of(keys, bag_offsets)
    g = grad_flat.contiguous()
    if mean:   # d mean / d row = 1 / length for every member of the bag; the bags of member j are rows of its own block
        bpt = lens.numel() // len(group.tables)
        inv = lens.clamp(min=1).to(torch.float32)
        g = g.clone()
        for j, v in enumerate(group.views(g, bpt)):
            v /= inv[j * bpt:(j + 1) * bpt, None]
    step = _step_now(layer)
    group.apply_pooled(keys, bag_offsets, g, bag_of, *step, located=located if located.numel() == keys.numel() else None, **step.loose_kw())


@apply_grad_pooled_mixed.register_fake
def _(keys, bag_offsets, grad_flat, located, table_id, mean):
    return None


def _backward_pooled_mixed(ctx, grad_flat, _grad_located):
    keys, bag_offsets, located = ctx.saved_tensors
    apply_grad_pooled_mixed(keys, bag_offsets, grad_flat.contiguous().to(torch.float32), _fresh(ctx, located), ctx.table_id, ctx.mean)
    return None, None, None, None, None


lookup_pooled_mixed.register_autograd(_backward_pooled_mixed, setup_context=_setup_pooled)


# ---- pooled over a group in the keyed layout (SPEC.md §3 "Keyed output"): [bags_per_table, sum of dims], a sample's pooled vectors side by side ------
# forward = the group's find_pooled(layout="keyed"), which writes that block and, per position, the row of the gradient its step reads (step_index);
# backward = apply_pooled on the keyed gradient where it lies, viewed [B * T, dim], through that index (a mixed group: its apply_pooled(layout="keyed"),
# one launch that takes the gradient apart into the class-major step buffer) — no permute in either direction and no _bag_of.
@torch.library.custom_op("meepo::lookup_pooled_keyed", mutates_args=())
def lookup_pooled_keyed(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, mean: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (keyed rows [bags_per_table, sum of dims], located rows [n] (empty where the group hands none out), step index [n] int32)"""
    layer = _layer(table_id)
    group, mode = layer.table, "mean" if mean else "sum"
    index = torch.zeros(keys.numel(), dtype=torch.int32, device=keys.device)
    creates = layer.create_missing and layer.training
    if layer.traits.pools_with_insert:   # a TieredTableGroup: unseen ids are created inside the pooled lookup
        out, _ = group.find_pooled(keys, bag_offsets, mode, insert_missing=creates, layout="keyed", step_index=index, **_dtype_kw(layer),
                                   **(_admit_kw(layer) if creates else {}))
        return out, keys.new_empty(0), index
    located = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
    if layer.traits.mixed_dims:
        out, _ = group.find_pooled(keys, bag_offsets, mode, located=located, out_dtype=layer.out_dtype, insert_missing=creates, layout="keyed", step_index=index)
        return out, located, index
    _create_unseen(layer, keys, bag_offsets)
    out, _ = group.find_pooled(keys, bag_offsets, mode, located=located, layout="keyed", step_index=index, **_dtype_kw(layer))
    return out, located, index


def _keyed_width(group) -> int:
    return sum(group.dims) if hasattr(group, "dims") else len(group.tables) * group.dim


@lookup_pooled_keyed.register_fake
def _(keys, bag_offsets, anchor, table_id, mean):
    layer = _layer(table_id)
    bpt = (bag_offsets.numel() - 1) // len(layer.table.tables)
    return (keys.new_empty((bpt, _keyed_width(layer.table)), dtype=layer.out_dtype),
            keys.new_empty(0 if layer.traits.pools_with_insert else keys.numel()), keys.new_empty(keys.numel(), dtype=torch.int32))


@torch.library.custom_op("meepo::apply_grad_pooled_keyed", mutates_args=())
def apply_grad_pooled_keyed(keys: torch.Tensor, bag_offsets: torch.Tensor, grad_keyed: torch.Tensor, located: torch.Tensor, step_index: torch.Tensor,
                            table_id: int, mean: bool) -> None:
    layer = _layer(table_id)
    group = layer.table
    loc = located if located.numel() == keys.numel() else None
    step = _step_now(layer)
    if layer.traits.mixed_dims:   # fp32 or bf16 as it came: the de-interleave launch widens and, for the mean, divides
        group.apply_pooled(keys, bag_offsets, grad_keyed, step_index, *step, located=loc, layout="keyed", mean_offsets=bag_offsets if mean else None, **step.loose_kw())
        return
    nt, bpt = len(group.tables), grad_keyed.shape[0]
    g = grad_keyed.view(bpt, nt, group.dim)
    if mean:   # d mean / d row = 1 / length: one division of the keyed block, bag j * B + s sits at [s, j]
        lens = (bag_offsets[1:] - bag_offsets[:-1]).clamp(min=1).to(torch.float32)
        g = g / lens.view(nt, bpt).t()[:, :, None]
    group.apply_pooled(keys, bag_offsets, g.view(bpt * nt, group.dim), step_index, *step, located=loc, **step.loose_kw())


@apply_grad_pooled_keyed.register_fake
def _(keys, bag_offsets, grad_keyed, located, step_index, table_id, mean):
    return None


def _setup_pooled_keyed(ctx, inputs, output):
    keys, bag_offsets, _, table_id, mean = inputs
    ctx.save_for_backward(keys, bag_offsets, output[1], output[2])
    ctx.mean = mean
    _save_epoch(ctx, table_id)
    ctx.mark_non_differentiable(output[1], output[2])


def _backward_pooled_keyed(ctx, grad_out, _grad_located, _grad_index):
    keys, bag_offsets, located, step_index = ctx.saved_tensors
    g = grad_out.contiguous()
    if not (_layer(ctx.table_id).traits.mixed_dims and g.dtype == torch.bfloat16):
        g = g.to(torch.float32)   # widened BEFORE the mean's division (a mixed group's de-interleave launch widens a bf16 grad itself)
    apply_grad_pooled_keyed(keys, bag_offsets, g, _fresh(ctx, located), step_index, ctx.table_id, ctx.mean)
    return None, None, None, None, None


lookup_pooled_keyed.register_autograd(_backward_pooled_keyed, setup_context=_setup_pooled_keyed)


# ---- weighted pooled (torch.nn.EmbeddingBag's per_sample_weights; SUM only): bag = sum of w_i * row_i ----------------------
# forward = find_pooled(weights=...), which also hands every position's handle to the backward; backward = pooled_weighted_backward
# (grads [n, dim] = w_i * the bag's grad row, and the grad of the weights when they need one), then the table's step on those grads
@torch.library.custom_op("meepo::lookup_pooled_weighted", mutates_args=())
def lookup_pooled_weighted(keys: torch.Tensor, bag_offsets: torch.Tensor, weights: torch.Tensor, anchor: torch.Tensor,
                           table_id: int) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (pooled rows [n_bags, dim], located rows [n] — per-position handles the backward of this step reuses)"""
    layer = _layer(table_id)
    _create_unseen(layer, keys, bag_offsets)
    located = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
    out, _ = layer.table.find_pooled(keys, bag_offsets, "sum", weights=weights.contiguous(), located=located, **_dtype_kw(layer))
    return out, located


@lookup_pooled_weighted.register_fake
def _(keys, bag_offsets, weights, anchor, table_id):
    layer = _layer(table_id)
    return (keys.new_empty((bag_offsets.numel() - 1, layer.table.dim), dtype=layer.out_dtype), keys.new_empty(keys.numel()))


@torch.library.custom_op("meepo::apply_grad_pooled_weighted", mutates_args=())
def apply_grad_pooled_weighted(keys: torch.Tensor, bag_offsets: torch.Tensor, weights: torch.Tensor, grad_bags: torch.Tensor,
                               located: torch.Tensor, table_id: int, weight_grad: bool) -> torch.Tensor:
    """The table step of a weighted bag; -> the grad of the weights ([n]; empty unless weight_grad)."""
    layer = _layer(table_id)
    loc = located if located.numel() == keys.numel() else None
    grads, wg = layer.table.pooled_weighted_backward(keys, bag_offsets, weights.contiguous(), grad_bags.contiguous(), located=loc,
                                                     want_weight_grads=weight_grad)
    if layer.traits.grouped:   # a TableGroup: one grouped step over the members' key segments (it probes for itself)
        _step_now(layer).apply_to(layer.table, keys, _member_offsets(layer.table, bag_offsets), grads)
    else:
        _step_now(layer).apply_to(layer.table, keys, grads, slots=loc)
    return wg if wg is not None else grads.new_empty(0)


@apply_grad_pooled_weighted.register_fake
def _(keys, bag_offsets, weights, grad_bags, located, table_id, weight_grad):
    return grad_bags.new_empty(keys.numel() if weight_grad else 0)


def _setup_pooled_weighted(ctx, inputs, output):
    keys, bag_offsets, weights, _, table_id = inputs
    ctx.save_for_backward(keys, bag_offsets, weights, output[1])
    _save_epoch(ctx, table_id)
    ctx.mark_non_differentiable(output[1])


def _backward_pooled_weighted(ctx, grad_out, _grad_located):
    keys, bag_offsets, weights, located = ctx.saved_tensors
    wg = apply_grad_pooled_weighted(keys, bag_offsets, weights, grad_out.contiguous().to(torch.float32), _fresh(ctx, located), ctx.table_id, ctx.needs_input_grad[2])
    return None, None, (wg.view(weights.shape) if ctx.needs_input_grad[2] else None), None, None


lookup_pooled_weighted.register_autograd(_backward_pooled_weighted, setup_context=_setup_pooled_weighted)


# ---- max pooled (torch.nn.EmbeddingBag mode="max"): bag[j] = the first greatest row_i[j] over the bag ---------------------------------------
# forward = find_pooled_max, one launch, which also says which position won every element (argmax); backward = pooled_max_backward (grads [n, dim] = the
# bag's grad element at the winner, +0.0 elsewhere), then the table's (the group's) step on those grads, as the weighted pair's
@torch.library.custom_op("meepo::lookup_pooled_max", mutates_args=())
def lookup_pooled_max(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (pooled rows [n_bags, dim], argmax [n_bags, dim] int32 — the batch position every element came from, -1 in an empty bag)"""
    layer = _layer(table_id)
    _create_unseen(layer, keys, bag_offsets)
    argmax = torch.empty((bag_offsets.numel() - 1, layer.table.dim), dtype=torch.int32, device=keys.device)
    out = layer.table.find_pooled_max(keys, bag_offsets, argmax=argmax, **_dtype_kw(layer))[0]
    return out, argmax


@lookup_pooled_max.register_fake
def _(keys, bag_offsets, anchor, table_id):
    layer = _layer(table_id)
    n_bags = bag_offsets.numel() - 1
    return keys.new_empty((n_bags, layer.table.dim), dtype=layer.out_dtype), keys.new_empty((n_bags, layer.table.dim), dtype=torch.int32)


@torch.library.custom_op("meepo::apply_grad_pooled_max", mutates_args=())
def apply_grad_pooled_max(keys: torch.Tensor, bag_offsets: torch.Tensor, argmax: torch.Tensor, grad_bags: torch.Tensor, table_id: int) -> None:
    layer = _layer(table_id)
    grads = layer.table.pooled_max_backward(bag_offsets, argmax, grad_bags.contiguous(), keys.numel())
    if layer.traits.grouped:   # a TableGroup: one grouped step over the members' key segments
        _step_now(layer).apply_to(layer.table, keys, _member_offsets(layer.table, bag_offsets), grads)
    else:
        _step_now(layer).apply_to(layer.table, keys, grads)


@apply_grad_pooled_max.register_fake
def _(keys, bag_offsets, argmax, grad_bags, table_id):
    return None


def _setup_pooled_max(ctx, inputs, output):
    keys, bag_offsets, _, table_id = inputs
    ctx.save_for_backward(keys, bag_offsets, output[1])
    ctx.table_id = table_id
    ctx.mark_non_differentiable(output[1])


def _backward_pooled_max(ctx, grad_out, _grad_argmax):
    keys, bag_offsets, argmax = ctx.saved_tensors
    apply_grad_pooled_max(keys, bag_offsets, argmax, grad_out.contiguous().to(torch.float32), ctx.table_id)   # a bf16 layer's grad is widened (exact)
    return None, None, None, None


lookup_pooled_max.register_autograd(_backward_pooled_max, setup_context=_setup_pooled_max)


# ---- the same pair of ops over a TableGroup: the whole embedding collection of a model in one lookup / one update -------
@torch.library.custom_op("meepo::lookup_jagged", mutates_args=())
def lookup_jagged(keys: torch.Tensor, offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, insert_missing: bool) -> torch.Tensor:
    layer = _layer(table_id)
    rows, _ = (layer.group.find_or_insert(keys, offsets, **_dtype_kw(layer), **_admit_kw(layer)) if insert_missing
               else layer.group.find(keys, offsets, **_dtype_kw(layer)))
    return rows


@lookup_jagged.register_fake
def _(keys, offsets, anchor, table_id, insert_missing):
    layer = _layer(table_id)
    return keys.new_empty((keys.numel(), layer.group.dim), dtype=layer.out_dtype)


@torch.library.custom_op("meepo::apply_grad_jagged", mutates_args=())
def apply_grad_jagged(keys: torch.Tensor, offsets: torch.Tensor, grad_rows: torch.Tensor, table_id: int) -> None:
    layer = _layer(table_id)
    _step_now(layer).apply_to(layer.group, keys, offsets, grad_rows.contiguous())


@apply_grad_jagged.register_fake
def _(keys, offsets, grad_rows, table_id):
    return None


def _setup_jagged(ctx, inputs, output):
    keys, offsets, _, table_id, _ = inputs
    ctx.save_for_backward(keys, offsets)
    ctx.table_id = table_id


def _backward_jagged(ctx, grad_out):
    keys, offsets = ctx.saved_tensors
    apply_grad_jagged(keys, offsets, grad_out.contiguous().to(torch.float32), ctx.table_id)
    return None, None, None, None, None


lookup_jagged.register_autograd(_backward_jagged, setup_context=_setup_jagged)


# ---- padded sequences (SPEC.md §3 "find_padded"): [n_bags, max_len, dim] with zeros behind a short bag, a long bag cut to max_len --------------
# forward = the table's (the group's) find_padded, which also says which slot every kept position went to; backward = the indexed step on exactly
# that: position i takes row grad_index[i] of the dense grad viewed as [n_bags * max_len, dim], cut-off positions are EMPTY and take no step.
# A hot/cold pair and a TieredTableGroup have find_padded too (one launch over both tiers, mee_find_padded_tiered / mee_group_find_padded_tiered; tiers
# that are not native tables compose it themselves): their backward is the pair's apply_*(grad_index=) and the group's apply_indexed.
# A table without find_padded (traits.native_padded False: a CPU adapter, a sharded table or group, a sharded group of pairs) is served by composition:
# find on the kept keys and a placement into a zeroed block (_padded_places, table.py: the one place the tiered classes' composition gets it from
# too); its backward gathers the kept slots' grad rows and runs the plain step.
def _kept_segments(layer, pos, bag_offsets, n: int):
    """the composition's compact batch is keys[pos] (pos ascending); for a group -> the members' offsets into it, else None"""
    if not layer.traits.grouped:
        return None
    bounds = _member_offsets(layer.table, bag_offsets).to(torch.int64).clamp(min=0, max=n)
    return torch.searchsorted(pos, bounds).contiguous()


@torch.library.custom_op("meepo::lookup_padded", mutates_args=())
def lookup_padded(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, max_len: int,
                  keep_last: bool) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (padded [n_bags, max_len, dim], lengths [n_bags], step_keys [n], grad_index [n]: what the backward of this step applies)"""
    layer = _layer(table_id)
    table = layer.table
    _create_unseen(layer, keys, bag_offsets)
    if layer.traits.native_padded:
        out, _, lengths, step_keys, grad_index = table.find_padded(keys, bag_offsets, max_len, "last" if keep_last else "first", with_step=True, **_dtype_kw(layer))
        return out, lengths, step_keys, grad_index
    lengths, step_keys, grad_index, pos = _padded_places(keys, bag_offsets, max_len, keep_last)
    seg = _kept_segments(layer, pos, bag_offsets, keys.numel())
    out = torch.zeros((lengths.numel() * max_len, table.dim), dtype=layer.out_dtype, device=keys.device)
    if pos.numel():
        kk = keys[pos].contiguous()
        rows, _ = table.find(kk, seg, **_dtype_kw(layer)) if seg is not None else table.find(kk, **_dtype_kw(layer))
        out[grad_index[pos].to(torch.int64)] = rows.to(out.device)
    return out.view(lengths.numel(), max_len, table.dim), lengths, step_keys, grad_index


@lookup_padded.register_fake
def _(keys, bag_offsets, anchor, table_id, max_len, keep_last):
    layer = _layer(table_id)
    n_bags = bag_offsets.numel() - 1
    return (keys.new_empty((n_bags, max_len, layer.table.dim), dtype=layer.out_dtype), keys.new_empty(n_bags), keys.new_empty(keys.numel()),
            keys.new_empty(keys.numel(), dtype=torch.int32))


@torch.library.custom_op("meepo::apply_grad_padded", mutates_args=())
def apply_grad_padded(step_keys: torch.Tensor, bag_offsets: torch.Tensor, grad_index: torch.Tensor, grad_padded: torch.Tensor, table_id: int) -> None:
    layer = _layer(table_id)
    table = layer.table
    g = grad_padded.contiguous().view(-1, table.dim)
    step = _step_now(layer)
    if layer.traits.native_padded:
        if layer.traits.grouped:
            seg = _member_offsets(table, bag_offsets).to(torch.int64).clamp(min=0, max=step_keys.numel()).contiguous()
            table.apply_indexed(step_keys, seg, g, grad_index, *step, **step.loose_kw())
        else:
            step.apply_to(table, step_keys, g, grad_index=grad_index)
        return
    pos = torch.nonzero(step_keys != -(1 << 63)).view(-1)   # (a kept EMPTY key takes no step anyway: every apply skips it)
    seg = _kept_segments(layer, pos, bag_offsets, step_keys.numel())
    if pos.numel():
        kk, gg = step_keys[pos].contiguous(), g[grad_index[pos].to(torch.int64)].contiguous()
        step.apply_to(table, kk, *(() if seg is None else (seg,)), gg)


@apply_grad_padded.register_fake
def _(step_keys, bag_offsets, grad_index, grad_padded, table_id):
    return None


def _setup_padded(ctx, inputs, output):
    ctx.save_for_backward(output[2], inputs[1], output[3])
    ctx.table_id = inputs[3]
    ctx.mark_non_differentiable(output[1], output[2], output[3])


def _backward_padded(ctx, grad_out, _g_lengths, _g_keys, _g_index):
    step_keys, bag_offsets, grad_index = ctx.saved_tensors
    apply_grad_padded(step_keys, bag_offsets, grad_index, grad_out.contiguous().to(torch.float32), ctx.table_id)   # a bf16 layer's grad is widened (exact)
    return None, None, None, None, None, None


lookup_padded.register_autograd(_backward_padded, setup_context=_setup_padded)


def _check_min_count(layer: str, table, traits: _Traits, min_count, creates: bool = True, rows_layer: bool = False,
                     out_dtype: torch.dtype = torch.float32):
    """A layer's min_count (admission, SPEC.md §3 find_or_insert_admit): None, or a threshold over a table that admits.  The layer's own rules are
    here; whether the table admits is the table's to say (admission_refusal).  Refused at construction, before any launch, saying which case it is."""
    if min_count is None:
        return None
    if not creates:
        raise ValueError(f"{layer}: min_count needs create_missing=True (admission decides when an unseen id is created; without creation there is nothing to decide)")
    if type(min_count) is not int or not 0 <= min_count < 1 << 32:   # (a bool is no int here)
        raise ValueError(f"{layer}: min_count must be an int in [0, 2^32) (got {min_count!r})")
    over = f"{layer}: min_count over {type(table).__name__}: "
    if rows_layer and traits.hot_cold_pair:
        raise ValueError(over + "this layer has no admitting forward over a hot/cold pair; use a DynamicEmbeddingCollection over "
                         "TieredTableGroup([pair]) (one segment), whose training forward admits")
    reason = traits.admission_refusal() if traits.admission_refusal is not None else \
        "admission exists on a LookupTable and on a TableGroup on one device, not on sharded or peer-mapped tables"
    if reason:
        raise ValueError(over + reason)
    if rows_layer and out_dtype != torch.float32:
        raise ValueError(f"{layer}: min_count has no bf16 form on one table (mee_find_or_insert_admit returns fp32 rows): use out_dtype=torch.float32")
    return min_count


class _SparseLayer(torch.nn.Module):
    """What the three layers share: the registration under a table_id, the anchor that makes autograd run the backward, the table's traits, the
    checked out_dtype and min_count, and the optimizer step's settings with its counter (_step_now)."""

    def __init__(self, table, optimizer, lr, eps, betas, out_dtype, min_count, pooled: bool = False, creates: bool = True, rows_layer: bool = False,
                 l1: float = 0.0, l2: float = 0.0):
        super().__init__()
        name = type(self).__name__
        _refuse_narrow_rows(name, table)
        self.table, self.traits = table, _traits(table)
        self.min_count = _check_min_count(name, table, self.traits, min_count, creates, rows_layer, out_dtype)
        first = SparseStep.of(optimizer, lr, eps, *betas, error=ValueError, l1=l1, l2=l2)   # checks the name, resolves the default eps (ftrl: beta)
        if optimizer == "ftrl" and not self.traits.ftrl:
            raise ValueError(f"{name}: optimizer='ftrl' needs a table with apply_ftrl (a group: apply_pooled / apply_indexed with l1= and l2=); "
                             f"{type(table).__name__} has none (the sharded tables keep Adagrad and Adam)")
        self.optimizer, self.lr, self.eps, self.betas, self.step = optimizer, lr, first.eps, betas, 0
        self.l1, self.l2 = l1, l2   # FTRL's regularisation strengths (read by optimizer="ftrl" alone)
        if out_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
        if out_dtype != torch.float32 and not (self.traits.bf16_bags if pooled else self.traits.bf16_rows):
            raise ValueError(f"{type(table).__name__} has no bf16 lookup (tiered, sharded and peer-mapped tables return fp32 rows): use out_dtype=torch.float32 and "
                             "cast in the model")
        self.out_dtype = out_dtype
        self.table_id = next(_IDS)
        _LAYERS[self.table_id] = self
        # autograd only runs backward for ops with an input that requires grad
        self._anchor = torch.nn.Parameter(torch.zeros(()), requires_grad=True)


class DynamicEmbeddingCollection(_SparseLayer):
    """All embedding tables of a model behind one module: keys = the tables' id batches concatenated, offsets = the
    n_tables + 1 segment bounds (int64, on the device) -> fp32 [len(keys), dim].  Forward is ONE grouped find_or_insert
    (find in eval mode), backward ONE grouped optimizer step, whatever the number of tables (TableGroup in table.py).
    out_dtype=torch.bfloat16: the lookup itself writes bf16 rows (the tables stay fp32; a bf16 grad is widened, which is exact).
    `group` may be a ShardedTableGroup (sharded.py): the same two ops, then ONE exchange per lookup and per step over the process group; or a
    TieredTableGroup (tiered.py), a collection of hot/cold pairs: forward is one launch (two in training), backward two grouped steps; or a
    ShardedTieredTableGroup, both at once (this layer and DynamicEmbeddingBag need nothing of their own for it).
    min_count (a TableGroup whose tables were all created with admission=True, or a TieredTableGroup whose HOT tables were): the training forward is
    the admitting grouped lookup — an unseen id is created only once its table's (its pair's hot table's) sketch has seen it min_count times; until
    then it reads the default row and its gradient is dropped by the step, which ignores absent keys.  Eval mode counts and creates nothing."""

    def __init__(self, group, optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None, betas=(0.9, 0.999),
                 out_dtype: torch.dtype = torch.float32, min_count: int | None = None, l1: float = 0.0, l2: float = 0.0):
        """optimizer="ftrl" (tables created with OPT_FTRL): eps is FTRL's beta (default 1.0), l1 / l2 its regularisation strengths; betas is not read."""
        super().__init__(group, optimizer, lr, eps, betas, out_dtype, min_count, l1=l1, l2=l2)
        self.group = group

    def forward(self, keys: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        return lookup_jagged(keys, offsets, self._anchor, self.table_id, self.training)


class DynamicEmbeddingBag(_SparseLayer):
    """torch.nn.EmbeddingBag over a lookup table — or over a TableGroup, which makes it an embedding-bag COLLECTION: bag b
    then belongs to member b // bags_per_table and the whole model's sparse forward is one launch, its backward seven.
    Over a MixedTableGroup (members of different dims) forward returns a list: member j's [bags_per_table, dim_j] tensor, views of one buffer.
    (keys [n], bag_offsets [n_bags + 1], both on the device) -> [n_bags, dim] sums or means; backward runs the table's sparse optimizer with the bag's grad row for every member (no [n, dim]
    tensor exists in either direction).  create_missing=True (training mode only): unseen ids are inserted with their
    hashed initial row first (one more pass over the ids); otherwise absent ids read the default row and are not trained.
    min_count (with create_missing=True; a LookupTable or TableGroup created with admission=True, or a TieredLookupTable / TieredTableGroup whose hot
    tables were): that creation pass admits — an unseen id is created only once its table's sketch has seen it min_count times, and pools as the
    default row, untrained, until then.
    mode="max" (a LookupTable or a TableGroup; table-major layout, no per_sample_weights): forward is one launch that keeps, per element, the first greatest
    value of the bag's rows and the position it came from; backward builds the [n, dim] grads — the bag's grad element at the winning position, +0.0 at the
    others — and runs the table's (the group's) step on them, so every id of a bag takes a step.  Bit for bit torch.nn.EmbeddingBag(mode="max") in the forward.
    layout="keyed" (groups only): forward returns ONE [bags_per_table, sum of dims] tensor — row s holds sample s of every member side by side (member j
    at column sum(dims[:j])), the block a dense network reads — for a MixedTableGroup too.  Over a TableGroup, TieredTableGroup or MixedTableGroup the
    lookup writes that block itself and the step reads the gradient where it lies; over any other group (sharded groups, CPU adapters) the layer
    composes the table-major lookup and one permute, with the same results."""

    def __init__(self, table, mode: str = "sum", optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None, betas=(0.9, 0.999),
                 create_missing: bool = False, out_dtype: torch.dtype = torch.float32, min_count: int | None = None, layout: str = "table",
                 l1: float = 0.0, l2: float = 0.0):
        """out_dtype=torch.bfloat16: the bag is accumulated in fp32 and the finished row rounded once by the lookup; backward widens the bf16 grad.
        optimizer="ftrl" (tables created with OPT_FTRL): eps is FTRL's beta (default 1.0), l1 / l2 its regularisation strengths; betas is not read."""
        if mode not in ("sum", "mean", "max"):
            raise ValueError(f"mode must be 'sum' or 'mean', or 'max' over a LookupTable or a TableGroup (got {mode!r})")
        if layout not in ("table", "keyed"):
            raise ValueError(f"layout must be 'table' or 'keyed' (got {layout!r})")
        if mode == "max":   # before anything is registered: the class must pool by max itself, and only the table-major layout does
            if not (hasattr(table, "find_pooled_max") and hasattr(table, "pooled_max_backward")):
                raise ValueError(f"mode='max': {type(table).__name__} has no find_pooled_max / pooled_max_backward (a LookupTable and a TableGroup have; hot/cold "
                                 "pairs, tiered, mixed and sharded groups pool by sum or mean)")
            if layout == "keyed":
                raise ValueError(f"mode='max' has no keyed layout: {type(table).__name__}.find_pooled_max writes [n_bags, dim]; use layout='table'")
        super().__init__(table, optimizer, lr, eps, betas, out_dtype, min_count, pooled=True, creates=create_missing, l1=l1, l2=l2)
        if layout == "keyed" and not self.traits.grouped:
            raise ValueError(f"layout='keyed' is a group's layout: {type(table).__name__} is one table (or one pair), whose [n_bags, dim] is keyed already")
        self.mode, self.create_missing, self.layout = mode, create_missing, layout

    def forward(self, keys: torch.Tensor, bag_offsets: torch.Tensor, per_sample_weights: torch.Tensor | None = None) -> torch.Tensor:
        """per_sample_weights (fp32 [n], mode "sum" only): the bag is the sum of w_i * row_i; backward also yields their grad.
        The weighted backward updates every position, so its bags must partition the keys: bag_offsets[0] = 0, bag_offsets[-1] = n.
        mode "max" takes no per_sample_weights, as in torch.nn.EmbeddingBag; its backward updates every position too (the same rule for the bags)."""
        if self.mode == "max":
            if per_sample_weights is not None:
                raise ValueError("per_sample_weights are not supported for mode='max', as in torch.nn.EmbeddingBag")
            return lookup_pooled_max(keys, bag_offsets, self._anchor, self.table_id)[0]
        if self.layout == "keyed":
            if per_sample_weights is not None:
                raise ValueError("layout='keyed' has no weighted bags: per_sample_weights are offered in the table-major layout only")
            if self.traits.native_keyed:
                return lookup_pooled_keyed(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
            nt = len(self.table.tables)   # composition: the table-major lookup and one permute (autograd runs the inverse on the gradient)
            if self.traits.mixed_dims:
                flat = lookup_pooled_mixed(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
                return torch.cat(self.table.views(flat, (bag_offsets.numel() - 1) // nt), dim=1)
            pooled = lookup_pooled(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
            return pooled.view(nt, -1, pooled.shape[1]).transpose(0, 1).reshape(-1, nt * pooled.shape[1])
        if self.traits.mixed_dims:   # a MixedTableGroup: one tensor per member, views of the one buffer the lookup wrote
            if per_sample_weights is not None:
                raise ValueError(f"{type(self.table).__name__} has no weighted bags: per_sample_weights are not offered over members of different dims")
            flat = lookup_pooled_mixed(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
            return self.table.views(flat, (bag_offsets.numel() - 1) // len(self.table.tables))
        if per_sample_weights is None:
            return lookup_pooled(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
        if self.mode != "sum":
            raise ValueError("per_sample_weights are only supported for mode='sum', as in torch.nn.EmbeddingBag")
        if not self.traits.weighted_bags:   # (a ShardedTableGroup: refused on every rank alike, before anything is exchanged; a TieredLookupTable)
            raise ValueError(f"{type(self.table).__name__} has no weighted bags: per_sample_weights are not offered over a sharded group or a hot/cold pair")
        return lookup_pooled_weighted(keys, bag_offsets, per_sample_weights, self._anchor, self.table_id)[0]


class DynamicEmbeddingSequence(_SparseLayer):
    """Sequence features as a sequence model reads them: (keys [n], bag_offsets [n_bags + 1], both on the device) -> (padded [n_bags, max_len, dim],
    lengths [n_bags] int64).  padded[b, j] is the row of bag b's j-th kept id, zeros behind the end of a short bag; a bag longer than max_len keeps
    its first (keep="first") or its last (keep="last") max_len ids; lengths is the mask.  Over a LookupTable or a TableGroup (bag b then belongs to
    member b // bags_per_table), and over a hot/cold pair or a TieredTableGroup of native tables (one launch over both tiers, which also feeds the
    placement policy's hit counters), the forward is ONE launch that writes the block directly and the backward the table's indexed step on the
    dense grad — no [n, dim] tensor exists in either direction, and ids that were cut off are neither looked up nor trained.  Any other table with
    find / find_or_insert / apply_* (a sharded table or group, a sharded group of pairs, CPU adapters) is served by composition, with the same results.
    create_missing=True (training mode only): unseen ids — cut-off ones too — are inserted with their hashed initial row first (one more pass over
    the ids); otherwise absent ids read the default row and are not trained."""

    def __init__(self, table_or_group, max_len: int, keep: str = "first", optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None,
                 betas=(0.9, 0.999), create_missing: bool = True, out_dtype: torch.dtype = torch.float32, l1: float = 0.0, l2: float = 0.0):
        if keep not in ("first", "last"):
            raise ValueError(f"keep must be 'first' or 'last' (got {keep!r})")
        if int(max_len) < 1:
            raise ValueError(f"max_len must be at least 1 (got {max_len})")
        super().__init__(table_or_group, optimizer, lr, eps, betas, out_dtype, None, l1=l1, l2=l2)
        self.max_len, self.keep, self.create_missing = int(max_len), keep, create_missing

    def forward(self, keys: torch.Tensor, bag_offsets: torch.Tensor):
        padded, lengths, _, _ = lookup_padded(keys, bag_offsets, self._anchor, self.table_id, self.max_len, self.keep == "last")
        return padded, lengths


class DynamicEmbedding(_SparseLayer):
    """ids (any int64 tensor) -> fp32 [..., dim].  The table must have been created with the matching optimizer planes.
    out_dtype=torch.bfloat16 (a LookupTable in HBM only): the lookup writes bf16 rows — what `.to(torch.bfloat16)` on the fp32 rows would give —
    and backward widens the bf16 grad before the table's fp32 step.
    min_count (a LookupTable created with admission=True; fp32 out): the training forward is find_or_insert(min_count=) and the backward the plain
    apply_* — the located forward has no admitting form; an id not yet admitted reads the default row and its gradient is dropped.  Not over a
    hot/cold pair: a DynamicEmbeddingCollection over TieredTableGroup([pair]) admits."""

    def __init__(self, table, optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None, betas=(0.9, 0.999),
                 out_dtype: torch.dtype = torch.float32, min_count: int | None = None, l1: float = 0.0, l2: float = 0.0):
        """optimizer="ftrl" (a table created with OPT_FTRL): eps is FTRL's beta (default 1.0), l1 / l2 its regularisation strengths; betas is not read."""
        super().__init__(table, optimizer, lr, eps, betas, out_dtype, min_count, rows_layer=True, l1=l1, l2=l2)
        self.fuse_backward_partition = True   # see forward()

    def forward(self, keys: torch.Tensor) -> torch.Tensor:
        if self.min_count is None and self.traits.located_table:   # one HBM table: the backward updates the rows at the slots this lookup found
            # training: the lookup's launch also partitions the batch for the backward's apply (nothing else may change the table in between:
            # the C-ABI refuses mutators while that partition is pending — table.apply_discard() drops it)
            return lookup_located(keys, self._anchor, self.table_id, self.training, self.training and torch.is_grad_enabled() and self.fuse_backward_partition)[0]
        return lookup(keys, self._anchor, self.table_id, self.training)   # sharded / tiered tables: their apply routes by key
