"""The fused embedding layers against float64 torch.  Weights and upstream gradients are small integers
stored as float32 (range [-8, 8]): every sum of up to 2^16 terms is exact in fp32, so sum-mode outputs
and gradients are compared for EQUALITY whatever the summation order.  Mean mode multiplies by a rounded
1 / len: the forward is held to 2 ulp of the float32 result (one rounding of the reciprocal, one of the
product); a mean-mode gradient row sums n such products, each rounding of a partial sum adding at most
half an ulp of a value bounded by the sum of magnitudes, so it is held to (n + 2) * 2^-23 * sum |term|."""
import copy

import pytest
import torch

from nvtabular_amd import _lib, kernels_embedding as KE
from nvtabular_amd.framework_utils.torch.layers import ConcatenatedEmbeddings, MultiHotEmbeddings
from nvtabular_amd.framework_utils.torch.models import Model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23
CARDS = (1, 2, 100_003)
LENS = (0, 1, 300, 0, 2, 65, 0)   # a leading, an interior and a trailing empty bag


def _ints(shape, gen, lo=-8, hi=9):
    return torch.randint(lo, hi, shape, generator=gen).float().to(DEV)


def _layer(cls, dims, gen, **kw):
    shapes = {f"c{i}": (CARDS[i % 3], d) for i, d in enumerate(dims)}
    layer = cls(shapes, **kw).to(DEV)
    for p in layer.parameters():
        p.data = _ints(p.shape, gen)
    return layer, shapes


def _ids(shapes, batch, gen, dtype=torch.int64):
    return torch.stack([torch.randint(0, r, (batch,), generator=gen) for r, _ in shapes.values()], 1).to(DEV, dtype)


def _bags(rows, lens, gen):
    values = torch.randint(0, rows, (sum(lens),), generator=gen).to(DEV)
    offsets = torch.tensor([0] + list(lens)).cumsum(0).to(DEV)
    return values, offsets


def _bag_ref(w, values, offsets, mean):
    lens = offsets[1:] - offsets[:-1]
    bag = torch.repeat_interleave(torch.arange(lens.numel(), device=DEV), lens)
    out = torch.zeros(lens.numel(), w.shape[1], dtype=torch.float64, device=DEV).index_add_(0, bag, w.double()[values])
    return out / lens.clamp(min=1).unsqueeze(1) if mean else out


@pytest.mark.parametrize("dims", [[1], [3, 4, 23], [16, 128, 512], [520]])
@pytest.mark.parametrize("batch, dtype", [(1, torch.int64), (63, torch.int32), (65, torch.int64), (257, torch.int32)])
def test_gather_cat_equals_indexing(batch, dtype, dims):
    gen = torch.Generator().manual_seed(batch)
    layer, shapes = _layer(ConcatenatedEmbeddings, dims, gen)
    x = _ids(shapes, batch, gen, dtype)
    want = torch.cat([p.double()[x[:, i].long()] for i, p in enumerate(layer.parameters())], 1)
    assert torch.equal(layer(x).double(), want)
    assert torch.equal(layer(x[0]).double(), want[:1])                       # a 1-D x is one row
    wide = torch.stack([x, x + 1], 2).reshape(batch, -1)                    # x is wide[:, ::2]
    assert torch.equal(layer(wide[:, ::2]).double(), want)
    assert int(layer.out_of_range) == 0


def test_out_of_range_ids_are_masked_and_counted():
    gen = torch.Generator().manual_seed(0)
    layer, _ = _layer(ConcatenatedEmbeddings, [4, 3, 2], gen)      # rows 1, 2, 100 003
    x = torch.tensor([[-1, 1, 5], [0, 2, 7], [0, 0, 2 ** 40]], device=DEV)   # -1, rows, 2^40
    out = layer(x)
    w = [p.detach() for p in layer.parameters()]
    want = torch.cat([w[0][[0, 0, 0]], w[1][[1, 0, 0]], w[2][[5, 7, 0]]], 1)
    want[0, :4], want[1, 4:7], want[2, 7:] = 0, 0, 0
    assert torch.equal(out, want) and int(layer.out_of_range) == 3
    out.backward(torch.ones_like(out))
    assert [int(p.grad.sum()) for p in layer.parameters()] == [2 * 4, 2 * 3, 2 * 2]
    assert layer.embedding_layers[2].weight.grad[[5, 7]].eq(1).all()
    bags, _ = _layer(MultiHotEmbeddings, [4], gen)                 # one row: only id 0 is in range
    got = bags({"c0": (torch.tensor([0, -1, 1, 2 ** 40, 0], device=DEV), torch.tensor([0, 2], device=DEV))})
    assert torch.equal(got, bags.embedding_layers[0].weight.detach() * torch.tensor([[1.0], [1.0]], device=DEV))
    assert int(bags.out_of_range) == 3


@pytest.mark.parametrize("form", ["full", "starts", "starts2d", "loader"])
@pytest.mark.parametrize("mode, dims", [("sum", [8, 4]), ("mean", [8, 4]), ("sum", [3, 8]), ("mean", [23])])
def test_bags_equal_a_float64_sum(mode, dims, form):
    gen = torch.Generator().manual_seed(len(dims))
    layer, shapes = _layer(MultiHotEmbeddings, dims, gen, mode=mode)
    x, want = {}, []
    for i, (name, (rows, _)) in enumerate(shapes.items()):
        values, offsets = _bags(rows, LENS[i:] + LENS[:i], gen)
        want.append(_bag_ref(layer.embedding_layers[i].weight.detach(), values, offsets, mode == "mean"))
        if form == "loader":
            x[name + "__values"], x[name + "__offsets"] = values, offsets
        else:
            x[name] = (values, {"full": offsets, "starts": offsets[:-1], "starts2d": offsets[:-1, None]}[form])
    got = layer(x, batch_size=len(LENS) if form == "full" else None).double()
    want = torch.cat(want, 1)
    if mode == "sum":
        assert torch.equal(got, want)
    else:
        assert ((got - want).abs() <= 2 * ULP * want.abs()).all()
    assert int(layer.out_of_range) == 0


def test_all_bags_empty_and_max_mode():
    layer, _ = _layer(MultiHotEmbeddings, [8], torch.Generator().manual_seed(1), mode="mean")
    x = {"c0__values": torch.empty(0, dtype=torch.int64, device=DEV), "c0__offsets": torch.zeros(4, dtype=torch.int64, device=DEV)}
    out = layer(x)
    assert out.shape == (3, 8) and not out.any()
    out.sum().backward()
    assert not layer.embedding_layers[0].weight.grad.any()
    with pytest.raises(NotImplementedError):
        MultiHotEmbeddings({"a": (4, 4)}, mode="max")


def _check_grads(tables, weights, run, refs, tol=None):
    """``run()`` -> output; backward twice with the same integer upstream gradient: both equal ``refs``
    (float64, one per table) and each other bit for bit; a sparse gradient is coalesced and ascending."""
    rounds, flags = [], []   # (torch's gradient accumulation re-wraps a sparse gradient: the flag is read in a hook)
    for w in weights:
        w.register_hook(lambda g: flags.append(g.is_sparse and g.is_coalesced()))
    for _ in range(2):
        for w in weights:
            w.grad = None
        out = run()
        out.backward(_ints(out.shape, torch.Generator().manual_seed(7)))
        rounds.append([w.grad for w in weights])
    for c, (g, again, ref) in enumerate(zip(*rounds, refs)):
        if tables.sparse[c]:
            assert g.is_sparse and all(flags) and len(flags) == 2 * len(weights)
            idx = g._indices()[0]
            assert torch.equal(idx, again._indices()[0]) and torch.equal(g._values(), again._values())
            assert idx.dtype == torch.int64 and (idx[1:] > idx[:-1]).all()
            g = g.to_dense()
        else:
            assert torch.equal(g, again)
        if tol is None:
            assert torch.equal(g.double(), ref), c
        else:
            assert ((g.double() - ref).abs() <= tol[c]).all(), c


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("pattern, dims", [("distinct", [4, 3]), ("distinct", [8, 16]), ("hot", [4, 8]), ("hot", [23]),
                                           ("collide", [4, 8]), ("collide", [5, 2])])
def test_single_hot_gradients_equal_index_add(pattern, dims, sparse):
    gen = torch.Generator().manual_seed(3)
    rows = 2000 if pattern == "distinct" else 50
    batch = {"distinct": 300, "hot": 4 * _lib.EMB_CHUNK + 1, "collide": 200}[pattern]
    tables = KE.LayerTables([(rows, d) for d in dims], [sparse] * len(dims))
    weights = [_ints((rows, d), gen).requires_grad_() for d in dims]
    if pattern == "distinct":
        x = torch.stack([torch.randperm(rows, generator=gen)[:batch] for _ in dims], 1).to(DEV)
    elif pattern == "hot":      # one id in every row: a segment of 4 chunks + 1, folded
        x = torch.full((batch, len(dims)), 7, device=DEV)
    else:                       # the same small ids in both tables
        x = torch.randint(0, 5, (batch, 1), generator=gen).expand(batch, len(dims)).contiguous().to(DEV)
    grad = _ints((batch, sum(dims)), torch.Generator().manual_seed(7)).double()
    refs, col = [], 0
    for c, d in enumerate(dims):
        refs.append(torch.zeros(rows, d, dtype=torch.float64, device=DEV).index_add_(0, x[:, c], grad[:, col:col + d]))
        col += d
    _check_grads(tables, weights, lambda: KE.embed(tables, weights, ids=x), refs)


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("mode, dims", [("sum", [8, 4]), ("sum", [3]), ("mean", [8, 4]), ("mean", [5])])
def test_bag_gradients_equal_index_add(mode, dims, sparse):
    gen = torch.Generator().manual_seed(5)
    rows, lens = 40, LENS + (3 * _lib.EMB_CHUNK,)
    tables = KE.LayerTables([(rows, d) for d in dims], [sparse] * len(dims))
    weights = [_ints((rows, d), gen).requires_grad_() for d in dims]
    bags = [_bags(rows, lens[i:] + lens[:i], gen) for i in range(len(dims))]
    bags[0][0][-600:] = 11       # a hot id: its segment spans several chunks
    grad = _ints((len(lens), sum(dims)), torch.Generator().manual_seed(7)).double()
    refs, tol, col = [], [], 0
    for (values, offsets), d in zip(bags, dims):
        n = offsets[1:] - offsets[:-1]
        bag = torch.repeat_interleave(torch.arange(n.numel(), device=DEV), n)
        term = grad[bag, col:col + d] / (n[bag].unsqueeze(1) if mode == "mean" else 1)
        zero = torch.zeros(rows, d, dtype=torch.float64, device=DEV)
        refs.append(zero.clone().index_add_(0, values, term))
        tol.append((values.numel() + 2) * ULP * zero.clone().index_add_(0, values, term.abs()))
        col += d
    _check_grads(tables, weights, lambda: KE.embed(tables, weights, bags=bags, mode=mode), refs,
                 tol if mode == "mean" else None)


def test_model_matches_a_float64_torch_model():
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(11)
    shapes = ({"a": (30, 4), "b": (20, 8)}, {"m": (25, 4)})
    model = Model(shapes, 3, 0.0, [16, 8], [0.0, 0.0], max_output=4.0, bag_mode="mean").to(DEV)
    ref = copy.deepcopy(model).double()
    batch = 32
    x = _ids(shapes[0], batch, gen)
    values, offsets = _bags(25, [1 + i % 4 for i in range(batch)], gen)
    cont = torch.randn(batch, 3, generator=gen).to(DEV)
    got = model((x, {"m": (values, offsets[:-1, None])}), cont)
    got.sum().backward()
    w = [p for p in ref.initial_cat_layer.parameters()]
    emb = [torch.nn.functional.embedding_bag(values, ref.mh_cat_layer.embedding_layers[0].weight, offsets[:-1], mode="mean"),
           w[0][x[:, 0]], w[1][x[:, 1]], ref.initial_cont_layer(cont.double())]
    h = torch.cat(emb, 1)
    for layer in ref.layers:
        h = layer(h)
    want = (4.0 * torch.sigmoid(ref.output_layer(h))).view(-1)
    want.sum().backward()
    torch.testing.assert_close(got, want.float())
    for (name, p), q in zip(model.named_parameters(), ref.parameters()):
        torch.testing.assert_close(p.grad, q.grad.float(), msg=lambda m, name=name: f"{name}: {m}")


def test_optimizer_steps_change_exactly_the_touched_rows():
    gen = torch.Generator().manual_seed(2)
    layer = ConcatenatedEmbeddings({"a": (50, 4), "b": (60, 4)}, sparse_columns=["a"]).to(DEV)
    wa, wb = layer.embedding_layers[0].weight, layer.embedding_layers[1].weight
    before = [wa.detach().clone(), wb.detach().clone()]
    opts = [torch.optim.SparseAdam([wa], lr=0.1), torch.optim.SGD([wb], lr=0.1)]
    x = _ids({"a": (50, 4), "b": (60, 4)}, 16, gen)
    layer(x).sum().backward()
    assert wa.grad.is_sparse and not wb.grad.is_sparse
    for opt in opts:
        opt.step()
    for c, (w, old) in enumerate(zip((wa, wb), before)):
        changed = (w.detach() != old).any(1).nonzero()[:, 0]
        assert torch.equal(changed, torch.unique(x[:, c]))
