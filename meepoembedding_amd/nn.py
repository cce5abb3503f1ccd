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
    meepo::lookup_pooled[_weighted] / meepo::apply_grad_pooled[_weighted]   embedding bags (sum / mean; weighted sum with the grad of
                                                                                 the per-sample weights)

The update happens INSIDE backward, so the layer has no torch parameters and needs no torch optimizer.  Both ops have
fake (meta) kernels, so a model containing the layer traces and exports; they are opaque to the tracer (the table is
state outside the graph, addressed by `table_id`).  Works with a LookupTable, a TieredLookupTable, a ShardedLookupTable
or a PeerShardedTable (same method names).  Plumbing only: no kernel lives here.
Reference anchor: /root/reference/README.md:2 ("Embedding designed for recommendation … systems").
"""
from __future__ import annotations

import itertools
import weakref

import torch

from ._lib import refuse_narrow_rows as _refuse_narrow_rows

_LAYERS: "weakref.WeakValueDictionary[int, DynamicEmbedding]" = weakref.WeakValueDictionary()
_IDS = itertools.count(1)


def _check_out_dtype(table, out_dtype: torch.dtype, pooled: bool = False) -> torch.dtype:
    """A layer's out_dtype: fp32, or bf16 where the table's lookups can write it (LookupTable, TableGroup; pooled = a bag layer, whose lookup is
    find_pooled: also a TieredLookupTable, which pools to bf16 while its find returns fp32 rows).  Refused at construction."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"out_dtype must be torch.float32 or torch.bfloat16 (got {out_dtype})")
    if out_dtype != torch.float32 and not (getattr(table, "supports_out_dtype", False) or (pooled and getattr(table, "supports_pooled_out_dtype", False))):
        raise ValueError(f"{type(table).__name__} has no bf16 lookup (tiered, sharded and peer-mapped tables return fp32 rows): use out_dtype=torch.float32 and "
                         "cast in the model")
    return out_dtype


def _check_min_count(table, min_count, layer: str, creates: bool = True):
    """A layer's min_count (admission, SPEC.md §3 find_or_insert_admit): None, or a threshold for a LookupTable or a uniform fp32 TableGroup whose
    tables were all created with admission=True, or for a TieredTableGroup (and, under a bag layer, a TieredLookupTable) of native pairs whose HOT
    tables were (SPEC.md §3 "Tiering": a pair counts in its hot table's sketch).  Everything else is refused at construction, before any launch,
    saying which case it is."""
    if min_count is None:
        return None
    from .table import LookupTable, TableGroup
    from .tiered import TieredLookupTable, TieredTableGroup
    name = type(table).__name__
    if not creates:
        raise ValueError(f"{layer}: min_count needs create_missing=True (admission decides when an unseen id is created; without creation there is nothing to decide)")
    if isinstance(min_count, bool) or not isinstance(min_count, int) or not 0 <= min_count < 1 << 32:
        raise ValueError(f"{layer}: min_count must be an int in [0, 2^32) (got {min_count!r})")
    if "Sharded" in name:   # ShardedTieredTableGroup too: before the tiered cases
        raise ValueError(f"{layer}: min_count over {name}: admission exists on one device — a LookupTable, a TableGroup, a hot/cold pair or a TieredTableGroup — not on sharded or peer-mapped tables")
    if isinstance(table, TieredLookupTable) and layer == "DynamicEmbedding":
        raise ValueError(f"{layer}: min_count over {name}: this layer has no admitting forward over a hot/cold pair; use a DynamicEmbeddingCollection over "
                         "TieredTableGroup([pair]) (one segment), whose training forward admits")
    if isinstance(table, (TieredLookupTable, TieredTableGroup)):
        pairs = table.tables if isinstance(table, TieredTableGroup) else [table]
        for j, p in enumerate(pairs):
            if not p._native():
                raise ValueError(f"{layer}: min_count over {name}: admission needs hot/cold pairs of native LookupTables" +
                                 (f" (member {j} holds other objects)" if isinstance(table, TieredTableGroup) else ""))
            if not p.admission:
                raise ValueError(f"{layer}: min_count over {name}: a hot/cold pair counts in its hot table's sketch, so every hot table needs admission=True (" +
                                 (f"the hot table of member {j} has no sketch)" if isinstance(table, TieredTableGroup) else "this pair's hot table has no sketch)"))
        return min_count
    if getattr(table, "mixed_dims", False):
        raise ValueError(f"{layer}: min_count over {name}: a mixed-width group creates unseen ids inside its pooled launch, which has no admission")
    if not isinstance(table, (LookupTable, TableGroup)):
        raise ValueError(f"{layer}: min_count over {name}: admission exists on a LookupTable and on a TableGroup on one device, not on sharded or peer-mapped tables")
    members = table.tables if isinstance(table, TableGroup) else [table]
    for j, t in enumerate(members):
        if not t._opts["admission"]:
            raise ValueError(f"{layer}: min_count needs every table created with admission=True (" +
                             (f"member {j} of the group has no sketch)" if isinstance(table, TableGroup) else "this table has no sketch)"))
    return min_count


def _admit_kw(layer) -> dict:
    """the creating lookup's min_count keyword — only when the layer has one, so tables without the keyword keep working"""
    return {} if layer.min_count is None else {"min_count": layer.min_count}


def _dtype_kw(layer) -> dict:
    """the lookup's out_dtype keyword — only when it is not the default, so tables without the keyword keep working at fp32"""
    return {} if layer.out_dtype == torch.float32 else {"out_dtype": layer.out_dtype}


def _layer(table_id: int) -> "DynamicEmbedding":
    try:
        return _LAYERS[table_id]
    except KeyError:
        raise RuntimeError(f"meepo: no live DynamicEmbedding with table_id {table_id}") from None


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
    layer.step += 1
    if layer.optimizer == "adagrad":
        layer.table.apply_adagrad(keys.reshape(-1), g, lr=layer.lr, eps=layer.eps)
    else:
        layer.table.apply_adam(keys.reshape(-1), g, lr=layer.lr, beta1=layer.betas[0], beta2=layer.betas[1], eps=layer.eps, step=layer.step)


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
    if getattr(table, "_nn_prepared", None) is not None:   # an earlier forward's partition that no backward used
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
    layer.step += 1
    prepared = getattr(layer.table, "_nn_prepared", None)
    if prepared is not None:   # the forward's partition is for exactly (this tensor, this length), or it is dropped
        flat = keys.reshape(-1)
        if prepared != (flat.data_ptr(), flat.numel()):
            layer.table.apply_discard()
        layer.table._nn_prepared = None
    if layer.optimizer == "adagrad":
        layer.table.apply_adagrad(keys.reshape(-1), g, lr=layer.lr, eps=layer.eps, slots=slots)
    else:
        layer.table.apply_adam(keys.reshape(-1), g, lr=layer.lr, beta1=layer.betas[0], beta2=layer.betas[1], eps=layer.eps, step=layer.step,
                               slots=slots)


@apply_grad_located.register_fake
def _(keys, grad_rows, located, table_id):
    return None


def _setup_located(ctx, inputs, output):
    keys, _, table_id = inputs[:3]
    ctx.save_for_backward(keys, output[1])
    ctx.table_id = table_id
    ctx.layout_epoch = getattr(_layer(table_id).table, "layout_epoch", None)   # handles are slot numbers: stale once rows move
    ctx.mark_non_differentiable(output[1])


def _backward_located(ctx, grad_out, _grad_located):
    keys, located = ctx.saved_tensors
    if getattr(_layer(ctx.table_id).table, "layout_epoch", None) != ctx.layout_epoch:
        located = located.new_empty(0)   # the table changed between forward and backward: the apply probes for itself
    apply_grad_located(keys, grad_out.contiguous().to(torch.float32), located, ctx.table_id)   # a bf16 layer's grad is widened (exact): the step is the fp32 step
    return None, None, None, None, None


lookup_located.register_autograd(_backward_located, setup_context=_setup_located)


def _hands_located(table) -> bool:
    """does lookup_pooled over this table return the located rows of its keys (a TableGroup on one device) or an empty tensor (one table; the
    sharded tables and groups, whose pooled lookup creates unseen ids itself and whose handles do not cross the exchange)?"""
    return hasattr(table, "apply_pooled") and not getattr(table, "pools_with_insert", False)


# ---- pooled: sum / mean per bag fused into the lookup, the bag's grad row indexed in the update ---------------------------
@torch.library.custom_op("meepo::lookup_pooled", mutates_args=())
def lookup_pooled(keys: torch.Tensor, bag_offsets: torch.Tensor, anchor: torch.Tensor, table_id: int, mean: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (pooled rows [n_bags, dim], located rows [n] — per-position handles the backward of this step reuses; empty for a
    single table, whose apply probes for itself)"""
    layer = _layer(table_id)
    if getattr(layer.table, "pools_with_insert", False):   # a ShardedLookupTable / ShardedTableGroup: the owners create unseen ids inside the pooled lookup's own exchange
        creates = layer.create_missing and layer.training
        out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", insert_missing=creates, **_dtype_kw(layer),
                                         **(_admit_kw(layer) if creates else {}))   # (min_count: a TieredTableGroup, whose creation pass admits)
        return out, keys.new_empty(0)
    if layer.create_missing and layer.training and keys.numel():
        # dynamic vocabulary: unseen ids enter their table (hashed initial row + optimizer state) before the pooled lookup
        if hasattr(layer.table, "apply_pooled"):
            bpt = (bag_offsets.numel() - 1) // len(layer.table.tables)
            layer.table.find_or_insert(keys, bag_offsets[::bpt].contiguous(), **_admit_kw(layer))
        else:
            layer.table.find_or_insert(keys, **_admit_kw(layer))
    if hasattr(layer.table, "apply_pooled"):   # a TableGroup
        located = torch.empty(keys.numel(), dtype=torch.int64, device=keys.device)
        out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", located=located, **_dtype_kw(layer))
        return out, located
    out, _ = layer.table.find_pooled(keys, bag_offsets, "mean" if mean else "sum", **_dtype_kw(layer))
    return out, keys.new_empty(0)


@lookup_pooled.register_fake
def _(keys, bag_offsets, anchor, table_id, mean):
    layer = _layer(table_id)
    return (keys.new_empty((bag_offsets.numel() - 1, layer.table.dim), dtype=layer.out_dtype),
            keys.new_empty(keys.numel() if _hands_located(layer.table) else 0))


@torch.library.custom_op("meepo::apply_grad_pooled", mutates_args=())
def apply_grad_pooled(keys: torch.Tensor, bag_offsets: torch.Tensor, grad_bags: torch.Tensor, located: torch.Tensor, table_id: int, mean: bool) -> None:
    layer = _layer(table_id)
    lens = bag_offsets[1:] - bag_offsets[:-1]
    bag_of = torch.repeat_interleave(torch.arange(lens.numel(), device=keys.device), lens, output_size=keys.numel())
    g = grad_bags.contiguous()
    if mean:   # d mean / d row = 1 / length for every member of the bag
        g = g / lens.clamp(min=1).to(torch.float32)[:, None]
    layer.step += 1
    if hasattr(layer.table, "apply_pooled"):   # a TableGroup: the whole collection in one step, on the rows the forward located
        layer.table.apply_pooled(keys, bag_offsets, g, bag_of, layer.optimizer, lr=layer.lr, eps=layer.eps, beta1=layer.betas[0],
                                 beta2=layer.betas[1], step=layer.step, located=located if located.numel() == keys.numel() else None)
    elif layer.optimizer == "adagrad":
        layer.table.apply_adagrad(keys, g, lr=layer.lr, eps=layer.eps, grad_index=bag_of)
    else:
        layer.table.apply_adam(keys, g, lr=layer.lr, beta1=layer.betas[0], beta2=layer.betas[1], eps=layer.eps, step=layer.step,
                               grad_index=bag_of)


@apply_grad_pooled.register_fake
def _(keys, bag_offsets, grad_bags, located, table_id, mean):
    return None


def _setup_pooled(ctx, inputs, output):
    keys, bag_offsets, _, table_id, mean = inputs
    ctx.save_for_backward(keys, bag_offsets, output[1])
    ctx.table_id, ctx.mean = table_id, mean
    # the located handles are slot numbers: valid only while no member table removes / clears / rehashes rows
    ctx.layout_epoch = getattr(_layer(table_id).table, "layout_epoch", None)
    ctx.mark_non_differentiable(output[1])


def _backward_pooled(ctx, grad_out, _grad_located):
    keys, bag_offsets, located = ctx.saved_tensors
    if getattr(_layer(ctx.table_id).table, "layout_epoch", None) != ctx.layout_epoch:
        located = located.new_empty(0)   # a table changed between forward and backward: the apply probes for itself
    apply_grad_pooled(keys, bag_offsets, grad_out.contiguous().to(torch.float32), located, ctx.table_id, ctx.mean)   # widened BEFORE the mean's division
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
    from .table import mixed_layout
    return mixed_layout(group.dims, (bag_offsets.numel() - 1) // len(group.tables))[2]


@lookup_pooled_mixed.register_fake
def _(keys, bag_offsets, anchor, table_id, mean):
    layer = _layer(table_id)
    return keys.new_empty(_mixed_total(layer.table, bag_offsets), dtype=layer.out_dtype), keys.new_empty(keys.numel())


@torch.library.custom_op("meepo::apply_grad_pooled_mixed", mutates_args=())
def apply_grad_pooled_mixed(keys: torch.Tensor, bag_offsets: torch.Tensor, grad_flat: torch.Tensor, located: torch.Tensor, table_id: int, mean: bool) -> None:
    layer = _layer(table_id)
    group = layer.table
    lens = bag_offsets[1:] - bag_offsets[:-1]
    bag_of = torch.repeat_interleave(torch.arange(lens.numel(), device=keys.device), lens, output_size=keys.numel())
    g = grad_flat.contiguous()
    if mean:   # d mean / d row = 1 / length for every member of the bag; the bags of member j are rows of its own block
        bpt = lens.numel() // len(group.tables)
        inv = lens.clamp(min=1).to(torch.float32)
        g = g.clone()
        for j, v in enumerate(group.views(g, bpt)):
            v /= inv[j * bpt:(j + 1) * bpt, None]
    layer.step += 1
    group.apply_pooled(keys, bag_offsets, g, bag_of, layer.optimizer, lr=layer.lr, eps=layer.eps, beta1=layer.betas[0], beta2=layer.betas[1],
                       step=layer.step, located=located if located.numel() == keys.numel() else None)


@apply_grad_pooled_mixed.register_fake
def _(keys, bag_offsets, grad_flat, located, table_id, mean):
    return None


def _backward_pooled_mixed(ctx, grad_flat, _grad_located):
    keys, bag_offsets, located = ctx.saved_tensors
    if getattr(_layer(ctx.table_id).table, "layout_epoch", None) != ctx.layout_epoch:
        located = located.new_empty(0)   # a table changed between forward and backward: the step probes for itself
    apply_grad_pooled_mixed(keys, bag_offsets, grad_flat.contiguous().to(torch.float32), located, ctx.table_id, ctx.mean)
    return None, None, None, None, None


lookup_pooled_mixed.register_autograd(_backward_pooled_mixed, setup_context=_setup_pooled)


# ---- weighted pooled (torch.nn.EmbeddingBag's per_sample_weights; SUM only): bag = sum of w_i * row_i ----------------------
# forward = find_pooled(weights=...), which also hands every position's handle to the backward; backward = pooled_weighted_backward
# (grads [n, dim] = w_i * the bag's grad row, and the grad of the weights when they need one), then the table's step on those grads
@torch.library.custom_op("meepo::lookup_pooled_weighted", mutates_args=())
def lookup_pooled_weighted(keys: torch.Tensor, bag_offsets: torch.Tensor, weights: torch.Tensor, anchor: torch.Tensor,
                           table_id: int) -> tuple[torch.Tensor, torch.Tensor]:
    """-> (pooled rows [n_bags, dim], located rows [n] — per-position handles the backward of this step reuses)"""
    layer = _layer(table_id)
    if layer.create_missing and layer.training and keys.numel():
        if hasattr(layer.table, "apply_pooled"):
            bpt = (bag_offsets.numel() - 1) // len(layer.table.tables)
            layer.table.find_or_insert(keys, bag_offsets[::bpt].contiguous(), **_admit_kw(layer))
        else:
            layer.table.find_or_insert(keys, **_admit_kw(layer))
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
    layer.step += 1
    kw = dict(lr=layer.lr, eps=layer.eps) if layer.optimizer == "adagrad" else \
        dict(lr=layer.lr, beta1=layer.betas[0], beta2=layer.betas[1], eps=layer.eps, step=layer.step)
    apply = layer.table.apply_adagrad if layer.optimizer == "adagrad" else layer.table.apply_adam
    if hasattr(layer.table, "apply_pooled"):   # a TableGroup: one grouped step over the members' key segments (it probes for itself)
        apply(keys, bag_offsets[::(bag_offsets.numel() - 1) // len(layer.table.tables)].contiguous(), grads, **kw)
    else:
        apply(keys, grads, slots=loc, **kw)
    return wg if wg is not None else grads.new_empty(0)


@apply_grad_pooled_weighted.register_fake
def _(keys, bag_offsets, weights, grad_bags, located, table_id, weight_grad):
    return grad_bags.new_empty(keys.numel() if weight_grad else 0)


def _setup_pooled_weighted(ctx, inputs, output):
    keys, bag_offsets, weights, _, table_id = inputs
    ctx.save_for_backward(keys, bag_offsets, weights, output[1])
    ctx.table_id = table_id
    ctx.layout_epoch = getattr(_layer(table_id).table, "layout_epoch", None)   # as _setup_pooled
    ctx.mark_non_differentiable(output[1])


def _backward_pooled_weighted(ctx, grad_out, _grad_located):
    keys, bag_offsets, weights, located = ctx.saved_tensors
    if getattr(_layer(ctx.table_id).table, "layout_epoch", None) != ctx.layout_epoch:
        located = located.new_empty(0)   # a table changed between forward and backward: the backward probes for itself
    wg = apply_grad_pooled_weighted(keys, bag_offsets, weights, grad_out.contiguous().to(torch.float32), located, ctx.table_id, ctx.needs_input_grad[2])
    return None, None, (wg.view(weights.shape) if ctx.needs_input_grad[2] else None), None, None


lookup_pooled_weighted.register_autograd(_backward_pooled_weighted, setup_context=_setup_pooled_weighted)


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
    layer.step += 1
    if layer.optimizer == "adagrad":
        layer.group.apply_adagrad(keys, offsets, grad_rows.contiguous(), lr=layer.lr, eps=layer.eps)
    else:
        layer.group.apply_adam(keys, offsets, grad_rows.contiguous(), lr=layer.lr, beta1=layer.betas[0], beta2=layer.betas[1],
                               eps=layer.eps, step=layer.step)


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


class _SparseOptimizerSettings:
    def _init_settings(self, optimizer, lr, eps, betas, table=None, out_dtype: torch.dtype = torch.float32, pooled: bool = False):
        if optimizer not in ("adagrad", "adam"):
            raise ValueError("optimizer must be 'adagrad' or 'adam'")
        self.out_dtype = _check_out_dtype(table, out_dtype, pooled)
        self.optimizer, self.lr, self.betas = optimizer, lr, betas
        self.eps = eps if eps is not None else (1e-10 if optimizer == "adagrad" else 1e-8)
        self.step = 0
        self.table_id = next(_IDS)
        _LAYERS[self.table_id] = self
        # autograd only runs backward for ops with an input that requires grad
        self._anchor = torch.nn.Parameter(torch.zeros(()), requires_grad=True)


class DynamicEmbeddingCollection(torch.nn.Module, _SparseOptimizerSettings):
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
                 out_dtype: torch.dtype = torch.float32, min_count: int | None = None):
        super().__init__()
        _refuse_narrow_rows("DynamicEmbeddingCollection", group)
        self.group = group
        self.min_count = _check_min_count(group, min_count, "DynamicEmbeddingCollection")
        self._init_settings(optimizer, lr, eps, betas, group, out_dtype)

    def forward(self, keys: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        return lookup_jagged(keys, offsets, self._anchor, self.table_id, self.training)


class DynamicEmbeddingBag(torch.nn.Module, _SparseOptimizerSettings):
    """torch.nn.EmbeddingBag over a lookup table — or over a TableGroup, which makes it an embedding-bag COLLECTION: bag b
    then belongs to member b // bags_per_table and the whole model's sparse forward is one launch, its backward seven.
    Over a MixedTableGroup (members of different dims) forward returns a list: member j's [bags_per_table, dim_j] tensor, views of one buffer.
    (keys [n], bag_offsets [n_bags + 1], both on the device) -> [n_bags, dim] sums or means; backward runs the table's sparse optimizer with the bag's grad row for every member (no [n, dim]
    tensor exists in either direction).  create_missing=True (training mode only): unseen ids are inserted with their
    hashed initial row first (one more pass over the ids); otherwise absent ids read the default row and are not trained.
    min_count (with create_missing=True; a LookupTable or TableGroup created with admission=True, or a TieredLookupTable / TieredTableGroup whose hot
    tables were): that creation pass admits — an unseen id is created only once its table's sketch has seen it min_count times, and pools as the
    default row, untrained, until then."""

    def __init__(self, table, mode: str = "sum", optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None, betas=(0.9, 0.999),
                 create_missing: bool = False, out_dtype: torch.dtype = torch.float32, min_count: int | None = None):
        """out_dtype=torch.bfloat16: the bag is accumulated in fp32 and the finished row rounded once by the lookup; backward widens the bf16 grad."""
        super().__init__()
        _refuse_narrow_rows("DynamicEmbeddingBag", table)
        if mode not in ("sum", "mean"):
            raise ValueError("mode must be 'sum' or 'mean'")
        self.table, self.mode, self.create_missing = table, mode, create_missing
        self.min_count = _check_min_count(table, min_count, "DynamicEmbeddingBag", creates=create_missing)
        self._init_settings(optimizer, lr, eps, betas, table, out_dtype, pooled=True)

    def forward(self, keys: torch.Tensor, bag_offsets: torch.Tensor, per_sample_weights: torch.Tensor | None = None) -> torch.Tensor:
        """per_sample_weights (fp32 [n], mode "sum" only): the bag is the sum of w_i * row_i; backward also yields their grad.
        The weighted backward updates every position, so its bags must partition the keys: bag_offsets[0] = 0, bag_offsets[-1] = n."""
        if getattr(self.table, "mixed_dims", False):   # a MixedTableGroup: one tensor per member, views of the one buffer the lookup wrote
            if per_sample_weights is not None:
                raise ValueError(f"{type(self.table).__name__} has no weighted bags: per_sample_weights are not offered over members of different dims")
            flat = lookup_pooled_mixed(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
            return self.table.views(flat, (bag_offsets.numel() - 1) // len(self.table.tables))
        if per_sample_weights is None:
            return lookup_pooled(keys, bag_offsets, self._anchor, self.table_id, self.mode == "mean")[0]
        if self.mode != "sum":
            raise ValueError("per_sample_weights are only supported for mode='sum', as in torch.nn.EmbeddingBag")
        if not getattr(self.table, "weighted_bags", True):   # (a ShardedTableGroup: refused on every rank alike, before anything is exchanged; a TieredLookupTable)
            raise ValueError(f"{type(self.table).__name__} has no weighted bags: per_sample_weights are not offered over a sharded group or a hot/cold pair")
        return lookup_pooled_weighted(keys, bag_offsets, per_sample_weights, self._anchor, self.table_id)[0]


class DynamicEmbedding(torch.nn.Module):
    """ids (any int64 tensor) -> fp32 [..., dim].  The table must have been created with the matching optimizer planes.
    out_dtype=torch.bfloat16 (a LookupTable in HBM only): the lookup writes bf16 rows — what `.to(torch.bfloat16)` on the fp32 rows would give —
    and backward widens the bf16 grad before the table's fp32 step.
    min_count (a LookupTable created with admission=True; fp32 out): the training forward is find_or_insert(min_count=) and the backward the plain
    apply_* — the located forward has no admitting form; an id not yet admitted reads the default row and its gradient is dropped.  Not over a
    hot/cold pair: a DynamicEmbeddingCollection over TieredTableGroup([pair]) admits."""

    def __init__(self, table, optimizer: str = "adagrad", lr: float = 0.01, eps: float | None = None, betas=(0.9, 0.999),
                 out_dtype: torch.dtype = torch.float32, min_count: int | None = None):
        super().__init__()
        _refuse_narrow_rows("DynamicEmbedding", table)
        self.min_count = _check_min_count(table, min_count, "DynamicEmbedding")
        if self.min_count is not None and out_dtype != torch.float32:
            raise ValueError("DynamicEmbedding: min_count has no bf16 form on one table (mee_find_or_insert_admit returns fp32 rows): use out_dtype=torch.float32")
        if optimizer not in ("adagrad", "adam"):
            raise ValueError("optimizer must be 'adagrad' or 'adam'")
        self.out_dtype = _check_out_dtype(table, out_dtype)
        self.table, self.optimizer, self.lr, self.betas = table, optimizer, lr, betas
        self.eps = eps if eps is not None else (1e-10 if optimizer == "adagrad" else 1e-8)
        self.step = 0
        self.fuse_backward_partition = True   # see forward()
        self.table_id = next(_IDS)
        _LAYERS[self.table_id] = self
        # autograd only runs backward for ops with an input that requires grad
        self._anchor = torch.nn.Parameter(torch.zeros(()), requires_grad=True)

    def forward(self, keys: torch.Tensor) -> torch.Tensor:
        if self.min_count is None and hasattr(self.table, "find_or_insert_located"):   # one HBM table: the backward updates the rows at the slots this lookup found
            # training: the lookup's launch also partitions the batch for the backward's apply (nothing else may change the table in between:
            # the C-ABI refuses mutators while that partition is pending — table.apply_discard() drops it)
            return lookup_located(keys, self._anchor, self.table_id, self.training, self.training and torch.is_grad_enabled() and self.fuse_backward_partition)[0]
        return lookup(keys, self._anchor, self.table_id, self.training)   # sharded / tiered tables: their apply routes by key
