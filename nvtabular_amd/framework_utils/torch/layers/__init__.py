from .embeddings import ConcatenatedEmbeddings, MultiHotEmbeddings

__all__ = ["ConcatenatedEmbeddings", "MultiHotEmbeddings"]
