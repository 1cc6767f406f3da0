"""``utils`` of the drop-in: ``utils.augmentations.SSDAugmentationCUDA`` (the device training transform) and
``utils.check_grad_norm.check_grad_norm`` (the drivers' per-iteration gradient norm, two launches and one read)."""
