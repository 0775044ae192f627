"""``ConcatenatedEmbeddings`` and ``MultiHotEmbeddings``: the reference's embedding layers with one
fused launch for all tables of a layer and a sparse, deterministic backward (kernels_embedding).

Parameters are named ``embedding_layers.<i>.weight`` like the reference's ``torch.nn.Embedding`` /
``EmbeddingBag`` modules, so a ``state_dict`` trained there loads here and back.  An id outside its
table gives a slice of zeros and no gradient and is counted in ``layer.out_of_range`` (a device
tensor: reading the attribute costs no synchronisation) -- torch raises a device-side assert instead."""
import torch

from .... import kernels_embedding as KE


class _Table(torch.nn.Module):
    """One table: holds ``weight`` under the reference's name; the layer does the lookups."""

    def __init__(self, rows, dim):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(int(rows), int(dim)))
        torch.nn.init.normal_(self.weight)   # what torch.nn.Embedding / EmbeddingBag do

    def extra_repr(self):
        return f"{self.weight.shape[0]}, {self.weight.shape[1]}"


class _EmbeddingLayer(torch.nn.Module):
    def __init__(self, embedding_table_shapes, dropout, sparse=()):
        super().__init__()
        self.embedding_names = list(embedding_table_shapes.keys())
        shapes = [embedding_table_shapes[k] for k in self.embedding_names]
        self._tables = KE.LayerTables(shapes, sparse)
        self.embedding_layers = torch.nn.ModuleList([_Table(rows, dim) for rows, dim in shapes])
        self.dropout = torch.nn.Dropout(p=dropout)

    def _weights(self):
        return [layer.weight for layer in self.embedding_layers]

    @property
    def out_of_range(self) -> torch.Tensor:
        """int64 scalar tensor: ids outside their table seen by ``forward`` so far."""
        return self._tables.counter(self.embedding_layers[0].weight.device)[0]


class ConcatenatedEmbeddings(_EmbeddingLayer):
    """Map multiple categorical variables to concatenated embeddings.

    embedding_table_shapes: ``{column: (cardinality, embedding_size)}``; ``sparse_columns``: the columns
    whose weight gets a coalesced ``torch.sparse_coo_tensor`` gradient (``torch.optim.SparseAdam``, ``SGD``
    and ``Adagrad`` take it), the others get a dense one.  ``forward(x)``: int64 / int32 ``[B, ncat]`` or
    ``[ncat]`` -> float32 ``[B, sum of embedding sizes]``."""

    def __init__(self, embedding_table_shapes, dropout=0.0, sparse_columns=()):
        for col in sparse_columns:
            if col not in embedding_table_shapes:
                raise ValueError(f"{col} is not in embedding_table_shapes")
        super().__init__(embedding_table_shapes, dropout, [c in sparse_columns for c in embedding_table_shapes])

    def forward(self, x):
        if x.dim() <= 1:
            x = x.unsqueeze(0)
        return self.dropout(KE.embed(self._tables, self._weights(), ids=x))


class MultiHotEmbeddings(_EmbeddingLayer):
    """Sum or mean of the embeddings of every row's list, the columns side by side.

    ``forward(x, batch_size=None)``: ``x`` holds per column either ``x[name] = (values, offsets)`` --
    ``offsets`` ``[B, 1]`` or ``[B]`` bag starts, the last bag running to the end, as the reference takes
    them; with ``batch_size`` given, ``batch_size + 1`` offsets are taken as they are -- or the
    dataloader's ``x[name + "__values"]`` / ``x[name + "__offsets"]`` with ``B + 1`` offsets."""

    def __init__(self, embedding_table_shapes, dropout=0.0, mode="sum"):
        if mode == "max":
            raise NotImplementedError('mode="max" is not implemented on the device; "sum" and "mean" are')
        if mode not in KE.MODES:
            raise ValueError(f'mode must be "sum" or "mean", not {mode!r}')
        super().__init__(embedding_table_shapes, dropout)
        self.mode = mode

    def forward(self, x, batch_size=None):
        bags = []
        for name in self.embedding_names:
            if name in x:
                values, offsets = x[name]
                values, offsets = values.reshape(-1), offsets.reshape(-1)
                if batch_size is None or offsets.numel() != batch_size + 1:
                    end = torch.full((1,), values.numel(), dtype=offsets.dtype, device=offsets.device)
                    offsets = torch.cat([offsets, end])
            else:
                values, offsets = x[name + "__values"], x[name + "__offsets"]
            bags.append((values, offsets))
        return self.dropout(KE.embed(self._tables, self._weights(), bags=bags, mode=self.mode))
