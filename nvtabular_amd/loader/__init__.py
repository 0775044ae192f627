"""Device dataloaders (the reference's ``nvtabular.loader``): batches of a Dataset as torch tensors."""
