"""DynamicEmbeddingBag over a MixedTableGroup (members of different dims): trains like one torch.nn.EmbeddingBag per member."""
import numpy as np
import pytest
import torch

from meepoembedding_amd import synth

DIMS = (8, 64, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("mode,out_dtype", [("sum", torch.float32), ("mean", torch.float32), ("sum", torch.bfloat16)])
def test_mixed_bag_layer_trains_like_torch_embedding_bags(dev, mode, out_dtype):
    """one training step with Adagrad == torch.nn.EmbeddingBag(sparse=True) + Adagrad per member (tolerances of tests/test_nn_layer.py); non-empty
    bags, as there.  bf16: the forward equals the rounded fp32 rows; the reference's loss is computed on rows rounded the same way."""
    from meepoembedding_amd import OPT_ADAGRAD, LookupTable, MixedTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    torch.manual_seed(7)
    vocab, bpt = 120, 9
    keys = [torch.from_numpy(synth.keys_np(60 + j, 0, vocab)) for j in range(len(DIMS))]
    refs, opts, tables, heads = [], [], [], []
    for j, d in enumerate(DIMS):
        w0 = torch.rand(vocab, d) - 0.5
        ref = torch.nn.EmbeddingBag(vocab, d, mode=mode, sparse=True)
        with torch.no_grad():
            ref.weight.copy_(w0)
        refs.append(ref)
        opts.append(torch.optim.Adagrad(ref.parameters(), lr=0.05, eps=1e-10, initial_accumulator_value=0.1))
        t = LookupTable(512, d, device=dev, optimizer=OPT_ADAGRAD, max_batch=4096, initial_accumulator=0.1)
        t.insert(keys[j].to(dev), w0.to(dev))
        tables.append(t)
        heads.append(torch.randn(d, 1) * 0.1)
    group = MixedTableGroup(tables, max_apply_batch=4096)
    layer = DynamicEmbeddingBag(group, mode=mode, lr=0.05, eps=1e-10, out_dtype=out_dtype).to(dev)
    lens = torch.randint(1, 9, (len(DIMS) * bpt,))
    lens[1], lens[bpt + 2] = 17, 30          # bags the wave's four tiles share
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lens, 0)])
    ids = [torch.randint(0, vocab, (int(lens[j * bpt:(j + 1) * bpt].sum()),)) for j in range(len(DIMS))]
    target = torch.randn(bpt, 1)
    outs = layer(torch.cat([keys[j][ids[j]] for j in range(len(DIMS))]).to(dev), off.to(dev))
    assert isinstance(outs, list) and [tuple(o.shape) for o in outs] == [(bpt, d) for d in DIMS] and all(o.dtype == out_dtype for o in outs)
    assert len({o._base.data_ptr() for o in outs}) == 1          # views of the one buffer the one custom op produced
    loss_ref = 0
    for j in range(len(DIMS)):
        opts[j].zero_grad()
        pooled = refs[j](ids[j], off[j * bpt:(j + 1) * bpt] - off[j * bpt])
        np.testing.assert_allclose(outs[j].detach().float().cpu().numpy(), pooled.detach().numpy(), rtol=2e-5 if out_dtype == torch.float32 else 2.0 ** -8, atol=1e-6)
        if out_dtype == torch.bfloat16:   # the layer's rows are rounded once (to within half a bf16 ulp, above); the gradient passes straight through the
            # rounding — and, as for every bf16 tensor in autograd, arrives as bf16 itself: the cast pair below rounds the reference's gradient alike
            pooled = (pooled + (outs[j].detach().float().cpu() - pooled.detach())).to(torch.bfloat16).float()
        loss_ref = loss_ref + ((pooled @ heads[j] - target) ** 2).mean()
    loss_ref.backward()
    for o in opts:
        o.step()
    loss = sum(((o.float() @ heads[j].to(dev) - target.to(dev)) ** 2).mean() for j, o in enumerate(outs))
    loss.backward()
    np.testing.assert_allclose(float(loss.detach()), float(loss_ref.detach()), rtol=2e-5)
    for j, t in enumerate(tables):
        got, found = t.find(keys[j].to(dev))
        assert bool(found.all())
        np.testing.assert_allclose(got.cpu().numpy(), refs[j].weight.detach().numpy(), rtol=2e-5, atol=1e-6, err_msg=f"member {j} (dim {DIMS[j]})")
    with pytest.raises(ValueError, match="per_sample_weights"):
        layer(keys[0][:4].to(dev), torch.zeros(len(DIMS) * 2 + 1, dtype=torch.int64, device=dev), per_sample_weights=torch.ones(4, device=dev))
    group.close()


@pytest.mark.gpu
def test_create_missing_grows_the_member_tables(dev):
    """unseen ids enter their member table (of its own width) in a training forward, not in eval, and are trained by the backward"""
    from meepoembedding_amd import INIT_UNIFORM, OPT_ADAGRAD, LookupTable, MixedTableGroup
    from meepoembedding_amd.nn import DynamicEmbeddingBag
    tables = [LookupTable(256, d, device=dev, optimizer=OPT_ADAGRAD, max_batch=1024, initial_accumulator=0.1, initializer=INIT_UNIFORM, init_scale=0.1,
                          init_seed=j) for j, d in enumerate(DIMS)]
    group = MixedTableGroup(tables, max_apply_batch=1024)
    grow = DynamicEmbeddingBag(group, mode="sum", lr=0.05, create_missing=True).to(dev)
    n_t = len(DIMS)
    new_ids = torch.arange(10**9, 10**9 + n_t * 4, device=dev)
    new_off = torch.arange(0, n_t * 4 + 1, 2, dtype=torch.int64, device=dev)       # 2 bags of 2 ids per table
    grow.eval()
    outs = grow(new_ids, new_off)
    assert [t.size() for t in tables] == [0] * n_t and all(not bool(o.any()) for o in outs)
    grow.train()
    outs = grow(new_ids, new_off)
    assert [t.size() for t in tables] == [4] * n_t
    rows = [t.find(new_ids[4 * j:4 * j + 4])[0] for j, t in enumerate(tables)]
    for j, o in enumerate(outs):
        assert torch.equal(o, rows[j].view(2, 2, -1)[:, 0] + rows[j].view(2, 2, -1)[:, 1])
    sum(o.sum() for o in outs).backward()
    for j, t in enumerate(tables):
        after = t.find(new_ids[4 * j:4 * j + 4])[0]
        assert bool((after < rows[j]).all())          # every element saw a gradient of +1
    assert [t.size() for t in tables] == [4] * n_t and [t.status() for t in tables] == [0] * n_t
    group.close()
