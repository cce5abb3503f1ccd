"""No GPU: what the three nn layers CALL on the table they sit on — every method, in order, with the keyword names the call binds and the scalar
values and tensors it passes — pinned for each kind of table the layers tell apart, so that a change of the Python layer that is meant to leave
behaviour alone can show it.  The tables are recording stubs with the real signatures; the arguments are recorded by the NAME they bind to
(positional or keyword: the same record) and only when the caller passed them (a keyword the layer leaves out — out_dtype at fp32, min_count without
admission — must stay left out: tables without it keep working).

The expected transcripts are data: tests/golden/nn_call_transcripts.json, written by `python tests/test_nn_transcripts.py --record`.
The 12 custom-op schemas, which traced and exported models carry, are pinned here too."""
import functools
import inspect
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nn_call_transcripts.json")
DIM = 4
BF16 = torch.bfloat16

SCHEMAS = """
meepo::apply_grad(Tensor keys, Tensor grad_rows, SymInt table_id) -> ()
meepo::apply_grad_jagged(Tensor keys, Tensor offsets, Tensor grad_rows, SymInt table_id) -> ()
meepo::apply_grad_located(Tensor keys, Tensor grad_rows, Tensor located, SymInt table_id) -> ()
meepo::apply_grad_pooled(Tensor keys, Tensor bag_offsets, Tensor grad_bags, Tensor located, SymInt table_id, bool mean) -> ()
meepo::apply_grad_pooled_mixed(Tensor keys, Tensor bag_offsets, Tensor grad_flat, Tensor located, SymInt table_id, bool mean) -> ()
meepo::apply_grad_pooled_weighted(Tensor keys, Tensor bag_offsets, Tensor weights, Tensor grad_bags, Tensor located, SymInt table_id, bool weight_grad) -> Tensor
meepo::lookup(Tensor keys, Tensor anchor, SymInt table_id, bool insert_missing) -> Tensor
meepo::lookup_jagged(Tensor keys, Tensor offsets, Tensor anchor, SymInt table_id, bool insert_missing) -> Tensor
meepo::lookup_located(Tensor keys, Tensor anchor, SymInt table_id, bool insert_missing, bool prepare=False) -> (Tensor, Tensor)
meepo::lookup_pooled(Tensor keys, Tensor bag_offsets, Tensor anchor, SymInt table_id, bool mean) -> (Tensor, Tensor)
meepo::lookup_pooled_mixed(Tensor keys, Tensor bag_offsets, Tensor anchor, SymInt table_id, bool mean) -> (Tensor, Tensor)
meepo::lookup_pooled_weighted(Tensor keys, Tensor bag_offsets, Tensor weights, Tensor anchor, SymInt table_id) -> (Tensor, Tensor)
""".strip().splitlines()


def test_the_twelve_op_schemas(built):
    import meepoembedding_amd.nn  # noqa: F401  (registers the ops)
    assert len(SCHEMAS) == 12
    for line in SCHEMAS:
        name = line.split("(")[0].split("::")[1]
        assert str(getattr(torch.ops.meepo, name).default._schema) == line


# ---- recording stubs -------------------------------------------------------------------------------------------------------------------
def _norm(v):
    if isinstance(v, torch.Tensor):
        return {"dtype": str(v.dtype).replace("torch.", ""), "shape": list(v.shape), "values": v.detach().to(torch.float64).flatten().tolist()}
    if isinstance(v, torch.dtype):
        return str(v)
    return v


def recorded(fn):
    sig = inspect.signature(fn)
    buffers = ("out", "found", "located", "slots") if fn.__name__.startswith("find") else ()   # a lookup's outputs: uninitialised when handed in

    @functools.wraps(fn)
    def wrapper(self, *args, **kw):
        bound = sig.bind(self, *args, **kw)   # no apply_defaults: only what the caller passed
        self.log.append([fn.__name__, {k: _norm(v.new_zeros(v.shape) if k in buffers and v is not None else v)
                                       for k, v in list(bound.arguments.items())[1:]}])
        return fn(self, *args, **kw)
    return wrapper


def _rows(n, dim=DIM, dtype=torch.float32):
    return torch.zeros((n, dim), dtype=dtype), torch.zeros(n, dtype=torch.uint8)


class PlainStub:
    """a duck table: the methods of tests/_cpu_backend.CpuTable plus the pooled ones, LookupTable's signatures"""
    dim = DIM

    def __init__(self):
        self.log = []

    @recorded
    def find(self, keys):
        return _rows(keys.numel())

    @recorded
    def find_or_insert(self, keys, min_count=None):
        return _rows(keys.numel())

    @recorded
    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, weights=None, located=None, out_dtype=torch.float32):
        if located is not None:
            located.zero_()
        return torch.zeros((bag_offsets.numel() - 1, DIM), dtype=out_dtype), torch.zeros(keys.numel(), dtype=torch.uint8)

    @recorded
    def pooled_weighted_backward(self, keys, bag_offsets, weights, bag_grads, located=None, want_weight_grads=True):
        return torch.ones((keys.numel(), DIM)), (torch.ones(keys.numel()) if want_weight_grads else None)

    @recorded
    def apply_adagrad(self, keys, grads, lr, eps=1e-10, grad_index=None, slots=None):
        pass

    @recorded
    def apply_adam(self, keys, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_index=None, slots=None):
        pass


class Bf16PlainStub(PlainStub):
    supports_out_dtype = True


class LocatedStub(PlainStub):
    """one table whose lookups hand out slot handles (a LookupTable in HBM)"""
    supports_out_dtype = True
    max_batch = 1 << 10

    def __init__(self):
        super().__init__()
        self.layout_epoch = 0

    @recorded
    def find_located(self, keys, out=None, found=None, slots=None, prepare_apply=False, out_dtype=torch.float32):
        return (*_rows(keys.numel(), dtype=out_dtype), torch.arange(keys.numel()))

    @recorded
    def find_or_insert_located(self, keys, out=None, found=None, slots=None, prepare_apply=False, out_dtype=torch.float32):
        return (*_rows(keys.numel(), dtype=out_dtype), torch.arange(keys.numel()))

    @recorded
    def apply_discard(self):
        pass


class GroupStub:
    """a group of two tables of one dim on one device (TableGroup's signatures)"""
    supports_out_dtype = True
    dim = DIM

    def __init__(self):
        self.log, self.tables, self.layout_epoch = [], [None, None], (0, 0)

    @recorded
    def find(self, keys, offsets, out=None, found=None, out_dtype=torch.float32):
        return _rows(keys.numel(), dtype=out_dtype)

    @recorded
    def find_or_insert(self, keys, offsets, out=None, found=None, out_dtype=torch.float32, min_count=None):
        return _rows(keys.numel(), dtype=out_dtype)

    @recorded
    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, located=None, weights=None, out_dtype=torch.float32):
        if located is not None:
            located.zero_()
        return torch.zeros((bag_offsets.numel() - 1, DIM), dtype=out_dtype), torch.zeros(keys.numel(), dtype=torch.uint8)

    @recorded
    def pooled_weighted_backward(self, keys, bag_offsets, weights, bag_grads, located=None, want_weight_grads=True):
        return torch.ones((keys.numel(), DIM)), (torch.ones(keys.numel()) if want_weight_grads else None)

    @recorded
    def apply_adagrad(self, keys, offsets, grads, lr, eps=1e-10):
        pass

    @recorded
    def apply_adam(self, keys, offsets, grads, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1):
        pass

    @recorded
    def apply_pooled(self, keys, bag_offsets, bag_grads, bag_of_position, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1, located=None):
        pass


class InsertingGroupStub(GroupStub):
    """a group whose pooled lookup creates unseen ids itself (a sharded group, a group of hot/cold pairs): no located rows, no weighted bags"""
    pools_with_insert = True
    weighted_bags = False
    supports_pooled_out_dtype = True

    @recorded
    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, insert_missing=False, out_dtype=torch.float32, min_count=None):
        return torch.zeros((bag_offsets.numel() - 1, DIM), dtype=out_dtype), torch.zeros(keys.numel(), dtype=torch.uint8)


class MixedStub:
    """a group whose two members differ in dim (MixedTableGroup's signatures); the views are the real class-major layout"""
    supports_out_dtype = True
    weighted_bags = False
    mixed_dims = True
    dims = [DIM, 2 * DIM]

    def __init__(self):
        self.log, self.tables, self.layout_epoch = [], [None, None], (0, 0)

    def views(self, flat, bags_per_table):
        from meepoembedding_amd.table import mixed_layout
        _, offs, _ = mixed_layout(self.dims, bags_per_table)
        return [flat[o:o + bags_per_table * d].view(bags_per_table, d) for o, d in zip(offs, self.dims)]

    @recorded
    def find_pooled(self, keys, bag_offsets, mode="sum", out=None, found=None, located=None, weights=None, out_dtype=torch.float32, insert_missing=False):
        out.zero_()
        located.zero_()
        return self.views(out, (bag_offsets.numel() - 1) // 2), torch.zeros(keys.numel(), dtype=torch.uint8)

    @recorded
    def apply_pooled(self, keys, bag_offsets, bag_grads, bag_of_position, optimizer, lr, eps=None, beta1=0.9, beta2=0.999, step=1, located=None):
        pass


# ---- the drive: every case is two training steps, one step whose handles went stale, one forward nobody backpropagates, one eval forward -----
KEYS = torch.tensor([11, 12, 11, 14, 15, 16], dtype=torch.int64)
BAGS = torch.tensor([0, 2, 3, 6], dtype=torch.int64)                 # 3 bags of one table
GROUP_BAGS = torch.tensor([0, 2, 2, 3, 5, 5, 6], dtype=torch.int64)  # 2 members x 3 bags, two of them empty
OFFSETS = torch.tensor([0, 2, 6], dtype=torch.int64)                 # 2 members


def _loss(out):
    outs = out if isinstance(out, list) else [out]
    return sum((o.float() * torch.arange(1, o.numel() + 1, dtype=torch.float32).view(o.shape)).sum() for o in outs)


def _bump(table):
    """what a remove / clear / reserve between forward and backward does to the handles"""
    if isinstance(getattr(table, "layout_epoch", None), int):
        table.layout_epoch += 1
    elif hasattr(table, "layout_epoch"):
        table.layout_epoch = tuple(e + 1 for e in table.layout_epoch)


def _drive(layer, table, forward):
    steps = []
    layer.train()
    for _ in range(2):
        _loss(forward(True)).backward()
        steps.append(layer.step)
    out = forward(True)
    _bump(table)
    _loss(out).backward()
    steps.append(layer.step)
    forward(False)           # a training forward without a backward ...
    forward(False)           # ... and the next one
    with torch.no_grad():
        forward(False)
    layer.eval()
    forward(False)
    assert steps == [1, 2, 3]
    return table.log


def _cases():
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag, DynamicEmbeddingCollection
    opts = {"adagrad": dict(optimizer="adagrad", lr=0.05), "adam": dict(optimizer="adam", lr=0.01, eps=1e-6, betas=(0.8, 0.95))}
    for opt, okw in opts.items():
        for dt in (torch.float32, BF16):
            tag = f"{opt}-{'bf16' if dt == BF16 else 'fp32'}"
            for stub in (PlainStub, Bf16PlainStub, LocatedStub):
                if dt == BF16 and stub is PlainStub:
                    continue
                t = stub()
                layer = DynamicEmbedding(t, out_dtype=dt, **okw)
                yield f"embedding-{stub.__name__}-{tag}", layer, t, lambda grad, layer=layer: layer(KEYS.view(2, 3))
            g = GroupStub()
            layer = DynamicEmbeddingCollection(g, out_dtype=dt, **okw)
            yield f"collection-GroupStub-{tag}", layer, g, lambda grad, layer=layer: layer(KEYS, OFFSETS)
            for stub in (PlainStub, Bf16PlainStub, LocatedStub, GroupStub, InsertingGroupStub, MixedStub):
                if dt == BF16 and stub is PlainStub:
                    continue
                bags = BAGS if stub in (PlainStub, Bf16PlainStub, LocatedStub) else GROUP_BAGS
                for mode in ("sum", "mean", "weighted"):
                    if mode == "weighted" and stub in (InsertingGroupStub, MixedStub):
                        continue
                    for create in (False, True):
                        t = stub()
                        layer = DynamicEmbeddingBag(t, mode="sum" if mode == "weighted" else mode, create_missing=create, out_dtype=dt, **okw)

                        def forward(grad, layer=layer, bags=bags, weighted=mode == "weighted"):
                            if not weighted:
                                return layer(KEYS, bags)
                            w = torch.tensor([1.0, 0.5, 2.0, -1.0, 0.25, 3.0], requires_grad=grad and layer.step % 2 == 0)   # with and without their grad
                            return layer(KEYS, bags, per_sample_weights=w)
                        yield f"bag-{stub.__name__}-{mode}-{'create' if create else 'nocreate'}-{tag}", layer, t, forward


def _transcripts():
    return {name: _drive(layer, table, forward) for name, layer, table, forward in _cases()}


def _pack(transcripts):
    """the golden file's form: every distinct tensor once, the calls refer to it by index (the same keys and offsets recur in every call)"""
    seen = {}

    def walk(x):
        if isinstance(x, dict) and "values" in x:
            return {"t": seen.setdefault(json.dumps(x, sort_keys=True), len(seen))}
        if isinstance(x, dict):
            return {k: walk(v) for k, v in x.items()}
        return [walk(v) for v in x] if isinstance(x, list) else x
    cases = walk(json.loads(json.dumps(transcripts)))
    return {"tensors": [json.loads(t) for t in seen], "cases": cases}


def _unpack(golden):
    def walk(x):
        if isinstance(x, dict) and set(x) == {"t"}:
            return golden["tensors"][x["t"]]
        if isinstance(x, dict):
            return {k: walk(v) for k, v in x.items()}
        return [walk(v) for v in x] if isinstance(x, list) else x
    return walk(golden["cases"])


def _first_difference(got, want):
    for j, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"call {j}: got {a}\n          expected {b}"
    return f"{len(got)} calls, expected {len(want)}: got {[c[0] for c in got]}, expected {[c[0] for c in want]}"


def test_layers_call_their_tables_as_recorded(built):
    with open(GOLDEN) as f:
        want = _unpack(json.load(f))
    got = json.loads(json.dumps(_transcripts()))
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], f"{name}: {_first_difference(got[name], want[name])}"


def test_the_step_counter_and_the_default_eps_reach_the_table(built):
    """spelled out, not only recorded: the first step passes step=1 and the second step=2; Adagrad's default eps is 1e-10, Adam's 1e-8; Adagrad is
    never handed betas or a step"""
    from meepoembedding_amd.nn import DynamicEmbedding, DynamicEmbeddingBag
    for optimizer, eps in (("adagrad", 1e-10), ("adam", 1e-8)):
        t = LocatedStub()
        layer = DynamicEmbedding(t, optimizer=optimizer, lr=0.5)
        for _ in range(2):
            _loss(layer(KEYS)).backward()
        applies = [c[1] for c in t.log if c[0] == "apply_" + optimizer]
        assert [c["eps"] for c in applies] == [eps, eps] and [c["lr"] for c in applies] == [0.5, 0.5]
        if optimizer == "adam":
            assert [(c["beta1"], c["beta2"], c["step"]) for c in applies] == [(0.9, 0.999, 1), (0.9, 0.999, 2)]
        else:
            assert all(set(c) == {"keys", "grads", "lr", "eps", "slots"} for c in applies)
        g = GroupStub()
        layer = DynamicEmbeddingBag(g, optimizer=optimizer, lr=0.5)
        for _ in range(2):
            _loss(layer(KEYS, GROUP_BAGS)).backward()
        applies = [c[1] for c in g.log if c[0] == "apply_pooled"]
        assert [(c["optimizer"], c["lr"], c["eps"], c["beta1"], c["beta2"], c["step"]) for c in applies] == \
            [(optimizer, 0.5, eps, 0.9, 0.999, 1), (optimizer, 0.5, eps, 0.9, 0.999, 2)]


if __name__ == "__main__":
    import sys
    if "--record" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        with open(GOLDEN, "w") as f:
            json.dump(_pack(_transcripts()), f, separators=(",", ":"), sort_keys=True)
            f.write("\n")
        print(f"wrote {GOLDEN}: {os.path.getsize(GOLDEN)} bytes")
