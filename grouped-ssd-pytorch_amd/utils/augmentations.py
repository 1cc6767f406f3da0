"""``utils.augmentations`` of the drop-in: ``SSDAugmentationCUDA``, the name train_lesion_multiphase_v2.py:527 gives the device
augmentation, is ``gssd.augment.DeviceSSDAugmentation`` -- the reference's ``SSDAugmentation`` (utils/augmentations.py:548-589)
on the MI355X, bitwise equal to it.  It runs on a collated batch after ``.cuda()``, not per study in the dataset: see
INTEGRATION.md.  The reference's per-study numpy / Pillow classes are not restated here."""
from gssd.augment import DeviceSSDAugmentation

__all__ = ['SSDAugmentationCUDA']


class SSDAugmentationCUDA(DeviceSSDAugmentation):
    """``SSDAugmentationCUDA(gt_pixel_jitter, expand_ratio, ssd_dim, means, use_normalize=..., p_only=...)``;
    ``aug(images_u8_cuda, targets) -> (images [B, 12, size, size], targets)``.  With ``use_pixel_link=True,
    pixel_link_version=config.version`` (train_lesion_multiphase_v2_pixellink.py:513-518) the targets are the PixelLink dict of
    detection_collate_v2_pixel_link, built on the device."""
