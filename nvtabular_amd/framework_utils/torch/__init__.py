"""Torch layers and an example model on the fused embedding kernels (``layers``, ``models``)."""
