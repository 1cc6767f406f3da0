"""``utils`` of the drop-in: only ``utils.augmentations.SSDAugmentationCUDA`` (the device training transform)."""
