"""Golden vectors for the device PixelLink targets: the reference's ``PreparePixelLinkTargets`` (utils/augmentations.py:527-545 ->
pixel_link/pixellink_data.py:15-99) on hand-made and random percent boxes, and its ``SSDAugmentation(use_pixel_link=True)`` chain
on seeded ``synth_study_u8`` studies.

Two things are supplied around the reference's own code: ``np.float`` (gone from numpy >= 1.24) is numpy's float64, and the
``cv2`` stub gets a ``drawContours`` that fills the axis-aligned rectangle between the contour's corners, both ends inclusive,
clipped to the image -- the definition the kernel states (include/gssd_hip.h).  It asserts that every contour it is given is such
a 4-vertex rectangle.  It is a restatement of cv2's polygon fill, not checked against OpenCV.

Outputs are kept as the collate stacks them; masks as uint8 (their values are 0 / 1) and the weight in the reference's float64.

    python tests/golden/make_golden_pixellink_targets.py     # rewrites tests/golden/pixellink_targets.npz  (build container only)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, sha, synth      # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
from pixellink_targets_ref import KEYS, VERSIONS, CHAIN_SEEDS, CHAIN_B, CHAIN_SRC, CHAIN_SIZE, CHAIN_BOXES   # noqa: E402


def draw_contours(image, contours, contour_idx, color, thickness=None):
    """cv2.drawContours(image, contours, -1, color, thickness=-1) for axis-aligned 4-vertex rectangles (see the module doc)."""
    assert contour_idx == -1 and thickness == -1
    pts = np.asarray(contours)
    assert pts.shape in ((1, 4, 2), (1, 1, 4, 2)), pts.shape          # label[i] and [label[i]] (pixellink_data.py:41, 59)
    H, W = image.shape[:2]
    for p in pts.reshape(-1, 4, 2):
        (xa, ya), (xb, yb), (xc, yc), (xd, yd) = p.tolist()
        assert ya == yb and xb == xc and yc == yd and xd == xa, p     # (x0,y0) (x1,y0) (x1,y1) (x0,y1)
        c0, c1 = max(min(xa, xb), 0), min(max(xa, xb), W - 1)
        r0, r1 = max(min(ya, yc), 0), min(max(ya, yc), H - 1)
        if c0 <= c1 and r0 <= r1:
            image[r0:r1 + 1, c0:c1 + 1] = color
    return image


def random_boxes(rng, n, lo=-0.15, hi=1.15, max_side=0.5):
    """n random percent boxes: centres across [lo, hi] so that some cross or leave every border; a few degenerate / inverted."""
    cx, cy = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    w, h = rng.uniform(0, max_side, n), rng.uniform(0, max_side, n)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    flip = rng.random(n) < 0.1
    b[flip] = b[flip][:, [2, 3, 0, 1]]
    line = rng.random(n) < 0.1
    b[line, 2] = b[line, 0]
    return np.hstack([b, np.zeros((n, 1))]).astype(np.float32)


def cases():
    """name -> (size, [per-image float32 [n, 5] percent boxes + label])."""
    rng = np.random.default_rng(20261016)
    z = lambda rows: np.array(rows, np.float32).reshape(-1, 5)       # noqa: E731
    edges = [z([[-0.2, -0.3, 0.1, 0.2, 0.], [0.85, -0.1, 1.3, 0.15, 0.], [0.9, 0.9, 1.5, 1.2, 0.], [-0.4, 0.8, 0.05, 1.0, 0.]]),
             z([[0., 0., 1., 1., 0.]]),                                     # the whole map
             z([[0.0, 0.4, 0.2, 0.6, 0.], [0.8, 0.4, 1.0, 0.6, 0.], [0.4, 0.0, 0.6, 0.2, 0.], [0.4, 0.8, 0.6, 1.0, 0.]]),
             z([[-1.0, -1.0, -0.5, -0.2, 0.], [1.2, 1.1, 1.9, 1.5, 0.]]),    # entirely outside: nothing drawn
             z([[0.98, 0.98, 1.0, 1.0, 0.], [0.0, 0.0, 0.01, 0.01, 0.]])]
    thin = [z([[0.5, 0.5, 0.5, 0.5, 0.]]),                                  # one pixel
            z([[0.2, 0.3, 0.2, 0.7, 0.], [0.3, 0.5, 0.8, 0.5, 0.]]),        # a column and a row
            z([[0.6, 0.6, 0.4, 0.4, 0.], [0.1, 0.9, 0.3, 0.8, 0.]]),        # inverted corners
            z([[0.2, 0.2, 0.205, 0.8, 0.], [0.0, 0.99, 1.0, 1.0, 0.]])]
    overlap = [z([[0.1, 0.1, 0.5, 0.5, 0.], [0.3, 0.3, 0.7, 0.7, 0.]]),     # 2-fold
               z([[0.1, 0.1, 0.5, 0.5, 0.], [0.3, 0.3, 0.7, 0.7, 0.], [0.2, 0.4, 0.6, 0.8, 0.]]),   # 3-fold
               z([[0.1, 0.1, 0.9, 0.9, 0.], [0.3, 0.3, 0.4, 0.4, 0.]]),     # the small box is covered: it owns nothing (not in R)
               z([[0.2, 0.2, 0.6, 0.6, 0.], [0.2, 0.2, 0.6, 0.6, 0.], [0.7, 0.7, 0.8, 0.9, 0.]]),   # identical duplicates
               z([[0.2, 0.2, 0.6, 0.6, 0.], [0.2, 0.2, 0.6, 0.6, 0.]]),     # duplicates only: R == 0
               z([[0.1, 0.1, 0.3, 0.3, 0.], [0.3, 0.1, 0.5, 0.3, 0.], [0.1, 0.3, 0.5, 0.5, 0.], [0.0, 0.0, 0.6, 0.6, 0.]])]
    empty = [np.zeros((0, 5), np.float32), z([[0.4, 0.4, 0.6, 0.6, 0.]]), np.zeros((0, 5), np.float32)]
    many = [random_boxes(rng, 255, -0.05, 1.05, 0.12), random_boxes(rng, 200, 0.2, 0.8, 0.3)]
    odd = [random_boxes(rng, int(rng.integers(0, 8))) for _ in range(6)] + edges[:2] + thin[:2]
    b32 = [random_boxes(rng, int(rng.integers(0, 21))) for _ in range(32)]
    out = {}
    for v in VERSIONS:
        out[f'edges_{v}'] = (64, v, edges)
        out[f'thin_{v}'] = (64, v, thin)
        out[f'overlap_{v}'] = (64, v, overlap)
        out[f'empty_{v}'] = (64, v, empty)
        out[f'many_{v}'] = (300, v, many)
        out[f'odd37_{v}'] = (37, v, odd)
        out[f'b32_{v}'] = (300, v, b32)
    return out


def collate(dicts):
    """The arrays of detection_collate_v2_pixel_link (data/data_custom_v2.py:399-434), masks as uint8, weight float64."""
    d = {k: np.stack([np.asarray(x[k]) for x in dicts]) for k in KEYS}
    for k in ('pixel_mask', 'neg_pixel_mask', 'link_mask'):
        assert d[k].min() >= 0 and d[k].max() <= 1, k
        d[k] = d[k].astype(np.uint8)
    assert d['pixel_pos_weight'].dtype == np.float64
    return d


def main():
    import random

    if not hasattr(np, 'float'):
        np.float = np.float64
    import_reference()
    sys.modules['cv2'].drawContours = draw_contours
    import utils.augmentations as A
    d, names = {}, []
    for name, (size, version, images) in cases().items():
        prep = A.PreparePixelLinkTargets(size, version)
        outs = []
        for b in images:
            _, _, lab = prep(None, b[:, :4], b[:, 4])
            A_ = int(np.count_nonzero(lab['pixel_mask']))
            assert A_ == 0 or abs(lab['pixel_pos_weight'].sum() - A_) <= 1e-9 * A_, name       # sum of weights == A
            outs.append(lab)
        pre = name + '__'
        d[pre + 'size'] = np.array(size, np.int64)
        d[pre + 'version'] = np.array(version)
        d[pre + 'counts'] = np.array([len(b) for b in images], np.int64)
        d[pre + 'boxes'] = np.concatenate(images).astype(np.float32)
        for k, v in collate(outs).items():
            d[pre + k] = v
        names.append(name)
        print(name, size, version, [len(b) for b in images])
    # the chain: SSDAugmentation(use_pixel_link=True) as the PixelLink driver builds it, CHAIN_B consecutive calls from one seed
    for v in VERSIONS:
        aug = A.SSDAugmentation(0.01, 1.5, CHAIN_SIZE, (49, 49, 49), use_normalize=True, use_pixel_link=True, pixel_link_version=v)
        studies = [synth.synth_study_u8(7000 + i, 4, CHAIN_SRC) for i in range(CHAIN_B)]
        random.seed(CHAIN_SEEDS[v])
        np.random.seed(CHAIN_SEEDS[v])
        outs, boxes = [], []
        for i in range(CHAIN_B):
            t = np.array(CHAIN_BOXES[i % 2], np.float32)
            _, bx, lab = aug(studies[i].copy(), t[:, :4], t[:, 4])
            boxes.append(np.hstack((bx, np.expand_dims(lab['labels'], 1))).astype(np.float32))   # data_custom_v2.py:288-292
            outs.append(lab)
        pre = f'chain_{v}__'
        d[pre + 'in_sha'] = np.frombuffer(bytes.fromhex(sha(np.stack(studies))), np.uint8)
        d[pre + 'counts'] = np.array([len(b) for b in boxes], np.int64)
        d[pre + 'boxes'] = np.concatenate(boxes)
        d[pre + 'next'] = np.array([random.random(), np.random.random_sample()], np.float64)
        for k, val in collate(outs).items():
            d[pre + k] = val
        print('chain', v, [len(b) for b in boxes])
    d['names'] = np.array(names)
    d['numpy_version'] = np.frombuffer(np.__version__.encode(), np.uint8)
    path = os.path.join(HERE, 'pixellink_targets.npz')
    np.savez_compressed(path, **d)
    print('pixellink_targets.npz written,', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
