"""``Model``: the reference's example network -- embeddings, BatchNorm on the continuous features, a
stack of Linear / ReLU / BatchNorm / Dropout blocks -- on the fused embedding layers.  Everything but
the embeddings is plain torch."""
import torch

from .layers import ConcatenatedEmbeddings, MultiHotEmbeddings


class Model(torch.nn.Module):
    """embedding_table_shapes: ``{column: (cardinality, embedding_size)}`` for the single-hot columns, or
    a ``(single_hot, multi_hot)`` tuple of two such dicts.  ``forward(x_cat, x_cont)``: ``x_cat`` is the
    id matrix ``[B, ncat]`` or a ``(id matrix, multi-hot dict)`` tuple (see ``MultiHotEmbeddings``),
    ``x_cont`` float ``[B, num_continuous]``; returns ``[B]``, times ``max_output * sigmoid`` if set."""

    def __init__(self, embedding_table_shapes, num_continuous, emb_dropout, layer_hidden_dims, layer_dropout_rates,
                 max_output=None, bag_mode="sum"):
        super().__init__()
        self.max_output = max_output
        mh_shapes = None
        if isinstance(embedding_table_shapes, tuple):
            embedding_table_shapes, mh_shapes = embedding_table_shapes
        embedding_size = 0
        if embedding_table_shapes:
            self.initial_cat_layer = ConcatenatedEmbeddings(embedding_table_shapes, dropout=emb_dropout)
            embedding_size += sum(dim for _, dim in embedding_table_shapes.values())
        if mh_shapes:
            self.mh_cat_layer = MultiHotEmbeddings(mh_shapes, dropout=emb_dropout, mode=bag_mode)
            embedding_size += sum(dim for _, dim in mh_shapes.values())
        self.initial_cont_layer = torch.nn.BatchNorm1d(num_continuous)
        sizes = [embedding_size + num_continuous] + list(layer_hidden_dims)
        self.layers = torch.nn.ModuleList(
            torch.nn.Sequential(torch.nn.Linear(n_in, n_out), torch.nn.ReLU(inplace=True), torch.nn.BatchNorm1d(n_out),
                                torch.nn.Dropout(rate))
            for n_in, n_out, rate in zip(sizes[:-1], sizes[1:], layer_dropout_rates))
        self.output_layer = torch.nn.Linear(sizes[-1], 1)

    def forward(self, x_cat, x_cont):
        mh_cat = None
        if isinstance(x_cat, tuple):
            x_cat, mh_cat = x_cat
        parts = []
        if mh_cat:   # (the reference's order: multi-hot, single-hot, continuous)
            batch = x_cat.shape[0] if x_cat is not None and x_cat.dim() == 2 else None
            parts.append(self.mh_cat_layer(mh_cat, batch_size=batch))
        if x_cat is not None and len(x_cat) > 0:
            parts.append(self.initial_cat_layer(x_cat))
        if x_cont is not None and len(x_cont) > 0:
            parts.append(self.initial_cont_layer(x_cont))
        x = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
        for layer in self.layers:
            x = layer(x)
        x = self.output_layer(x)
        if self.max_output:
            x = self.max_output * torch.sigmoid(x)
        return x.view(-1)
