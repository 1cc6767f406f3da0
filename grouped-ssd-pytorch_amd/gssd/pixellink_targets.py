"""PixelLink training targets on the MI355X: ``PreparePixelLinkTargets`` (utils/augmentations.py:527-545) through
``label_to_mask_and_pixel_pos_weight`` (pixel_link/pixellink_data.py:15-99), collated as ``detection_collate_v2_pixel_link``
(data/data_custom_v2.py:399-434) does, for a whole batch in one launch of ``gssd_pixellink_targets`` (csrc/pixellink_targets.hip;
the contract is in include/gssd_hip.h).

``prepare_targets(boxes, size, version)`` -> the collate's dict:

* ``pixel_mask``, ``neg_pixel_mask``: int64 ``[B, M, M]``; ``pixel_pos_weight``: float32 ``[B, M, M]``; ``link_mask``: int64
  ``[B, 8, M, M]`` -- on the device, M = int(size / factor), factor 2 for version ``"2s"`` and 4 for any other string;
* ``'lables'`` (the reference's key, misspelled): float32 ``[n_i]`` per image; ``'boxes'``: float32 ``[n_i, 5]`` per image -- on the
  CPU for CPU boxes, as the collate builds them, on the device for device boxes.

The rasterisation restates ``cv2.drawContours(thickness=-1)`` of the reference's axis-aligned 4-vertex polygons as an inclusive,
clipped rectangle; it has not been checked against OpenCV (cv2 is not a dependency).  At most 255 boxes per image: the reference
counts coverage in uint8, which wraps past that.
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, check

MAX_BOXES = 255
MAX_SIDE = 256        # the kernel's LDS owner map: M <= 256 (size 512 with "2s")
NEIGHBORS = 8
# link direction j -> (dh, dw), pixellink_data.py:89-96
LINK_DIRS = ((1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1))


def factor_of(version):
    """``factor = 2 if version == "2s" else 4`` (pixellink_data.py:21); the version must be named (a string)."""
    if not isinstance(version, str):
        raise _lib.GssdError(f'pixellink targets: the version must be a string such as "4s" or "2s", got {version!r}')
    return 2 if version == '2s' else 4


def mask_side(size, version):
    """M = int(size / factor), the side of every target map."""
    return int(int(size) / factor_of(version))


def _check_geometry(size, version):
    size = int(size)
    M = mask_side(size, version)
    if not 1 <= M <= MAX_SIDE:
        raise _lib.GssdError(f'pixellink targets: size {size} with version {version!r} gives {M} x {M} maps; 1 .. {MAX_SIDE} supported')
    return size, factor_of(version), M


def _as_rows(b, i):
    """Shape check of one image's boxes (a numpy array or a tensor): ``[n, 4]`` / ``[n, 5]``, or empty -> n."""
    shape = tuple(b.shape)
    if len(shape) == 1 and shape[0] == 0:
        return 0
    if len(shape) != 2 or shape[1] not in (4, 5):
        raise _lib.GssdError(f'pixellink targets: boxes of image {i} must be [n, 4] or [n, 5], got {shape}')
    if shape[0] > MAX_BOXES:
        raise _lib.GssdError(f'pixellink targets: image {i} has {shape[0]} boxes; at most {MAX_BOXES} are supported (the reference '
                             'counts coverage in uint8)')
    return shape[0]


def offsets_of(counts):
    """int32 ``[B + 1]`` prefix sums of the per-image box counts."""
    o = np.zeros(len(counts) + 1, np.int32)
    o[1:] = np.cumsum(np.asarray(counts, np.int64))
    return o


def pack_boxes(boxes):
    """Host packing: per-image ``[n_i, 4|5]`` arrays -> (float32 ``[total, 4]`` corners, int32 offsets ``[B + 1]``)."""
    arrs = []
    for i, b in enumerate(boxes):
        a = np.asarray(b.cpu() if isinstance(b, torch.Tensor) else b, np.float32)
        a = a.reshape(0, 4) if a.size == 0 else a
        _as_rows(a, i)
        arrs.append(a[:, :4])
    offs = offsets_of([len(a) for a in arrs])
    packed = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 4), np.float32), np.float32)
    return packed, offs


def staging(packed, offs):
    """One host byte buffer [offsets | pad to 16 | boxes] for a single pinned upload -> (bytes, byte offset of the boxes)."""
    head = (offs.nbytes + 15) & ~15
    buf = np.zeros(head + max(packed.nbytes, 16), np.uint8)
    buf[:offs.nbytes] = offs.view(np.uint8)
    buf[head:head + packed.nbytes] = packed.reshape(-1).view(np.uint8)
    return buf, head


def launch(boxes_ptr, offsets_ptr, B, size, version, dev):
    """Allocate the four maps on ``dev`` and run the kernel on the current stream.  ``boxes_ptr`` / ``offsets_ptr``: device
    addresses of the packed float32 ``[total, 4]`` corners and the int32 ``[B + 1]`` offsets."""
    size, factor, M = _check_geometry(size, version)
    pixel_mask = torch.empty(B, M, M, dtype=torch.int64, device=dev)
    neg_pixel_mask = torch.empty(B, M, M, dtype=torch.int64, device=dev)
    pixel_pos_weight = torch.empty(B, M, M, dtype=torch.float32, device=dev)
    link_mask = torch.empty(B, NEIGHBORS, M, M, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.gssd_pixellink_targets(boxes_ptr, offsets_ptr, B, size, factor, pixel_mask.data_ptr(), neg_pixel_mask.data_ptr(),
                                         pixel_pos_weight.data_ptr(), link_mask.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return dict(pixel_mask=pixel_mask, neg_pixel_mask=neg_pixel_mask, pixel_pos_weight=pixel_pos_weight, link_mask=link_mask)


def _lists(boxes, labels):
    """The collate's ``'lables'`` (float32 ``[n_i]``) and ``'boxes'`` (float32 ``[n_i, 5]``) lists, fresh tensors where the boxes are."""
    lab_out, box_out = [], []
    for i, b in enumerate(boxes):
        t = b.to(torch.float32).clone() if isinstance(b, torch.Tensor) else torch.from_numpy(np.array(b, np.float32))
        t = t.reshape(-1, t.shape[-1] if t.numel() else 5)
        if labels is not None:
            lab = torch.as_tensor(np.asarray(labels[i], np.float32) if not isinstance(labels[i], torch.Tensor) else labels[i])
            lab = lab.to(device=t.device, dtype=torch.float32).reshape(-1)
            if lab.shape[0] != t.shape[0]:
                raise _lib.GssdError(f'pixellink targets: image {i} has {t.shape[0]} boxes but {lab.shape[0]} labels')
            t = torch.cat([t[:, :4], lab[:, None]], 1)
        elif t.shape[1] != 5:
            raise _lib.GssdError(f'pixellink targets: image {i} has [n, 4] boxes and no labels (pass labels= or [n, 5] targets)')
        lab_out.append(t[:, 4].contiguous())
        box_out.append(t)
    return lab_out, box_out


def prepare_targets(boxes, size, version, device=None, labels=None):
    """The collate's PixelLink target dict for a batch: ``boxes`` a list of per-image ``[n_i, 4]`` / ``[n_i, 5]`` (percent corners
    [+ label]) arrays or tensors, all on the CPU or all on one device; ``labels`` optional per-image ``[n_i]`` (they replace column
    4).  CPU boxes go to ``device`` (default: the current CUDA device) through one pinned staging upload; device boxes are joined
    on the device and the offsets come from their shapes, so nothing waits for the device.  One kernel launch either way."""
    boxes = list(boxes)
    if not boxes:
        raise _lib.GssdError('pixellink targets: empty batch')
    if labels is not None and len(labels) != len(boxes):
        raise _lib.GssdError(f'pixellink targets: {len(boxes)} images but {len(labels)} label arrays')
    size, _, _ = _check_geometry(size, version)
    lists = _lists(boxes, labels)
    B = len(boxes)
    on_dev = [isinstance(b, torch.Tensor) and b.is_cuda for b in boxes]
    if all(on_dev):
        dev = boxes[0].device
        if device is not None and torch.device(device) != dev:
            raise _lib.GssdError(f'pixellink targets: boxes are on {dev}, device={device}')
        counts = []
        for i, b in enumerate(boxes):
            if b.device != dev or b.dtype != torch.float32:
                raise _lib.GssdError(f'pixellink targets: image {i}: boxes must be float32 on {dev}, got {b.dtype} on {b.device}')
            counts.append(_as_rows(b, i))
        parts = [b[:, :4] for b in boxes if b.dim() == 2 and b.shape[0]]
        packed = torch.cat(parts).contiguous() if parts else torch.zeros(1, 4, dtype=torch.float32, device=dev)
        offs = torch.from_numpy(offsets_of(counts)).pin_memory().to(dev, non_blocking=True)
        out = launch(packed.data_ptr(), offs.data_ptr(), B, size, version, dev)
    elif any(on_dev):
        raise _lib.GssdError('pixellink targets: boxes must be all on the CPU or all on one device')
    else:
        packed, offs = pack_boxes(boxes)
        if device is not None:
            dev = torch.device(device)
        else:
            dev = torch.device('cuda', torch.cuda.current_device()) if torch.cuda.is_available() else torch.device('cpu')
        if dev.type != 'cuda':
            raise _lib.GssdError(f'pixellink targets: the targets are built on the MI355X (no CPU fallback), got device={device}')
        buf, head = staging(packed, offs)
        d = torch.from_numpy(buf).pin_memory().to(dev, non_blocking=True)
        out = launch(d.data_ptr() + head, d.data_ptr(), B, size, version, dev)
    out['lables'], out['boxes'] = lists
    return out
