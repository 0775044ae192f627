"""Model-side helpers that consume what the dataloaders hand out (``framework_utils.torch``)."""
