"""Registry of the box-tail cases (gssd_pixellink_boxes_f32 / pixel_link.postprocess.component_boxes_device), shared by
tests/test_pixellink_box_cases_cpu.py (which proves every row fit for an EXACT comparison, with pixel_link/box_geometry.py alone) and
tests/test_gpu_pixellink_boxes.py (which runs the rows on the device).  TEST INFRASTRUCTURE ONLY.

A row is a batch: ``labels`` int32 [B,h,w] (hand-made maps, components numbered in raster order of their first pixel like the decode's),
``logits`` fp32 [B,2,h,w] (seeded), the destination size ``dst`` = (Hd, Wd) and the two filters.  The shapes are the smallest at which the
branch the row names can go wrong."""
import os

import numpy as np

from pixel_link import box_geometry as G
from pixel_link import pixel_link_config as cfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CFG_FILTERS = (cfg.min_height, cfg.min_area)          # (1, 3)
MAX_DET = 1024


def raster_labels(mask_ids):
    """Renumber a hand-made id map (0 = background) so that ids follow the raster order of each component's first pixel."""
    mask_ids = np.asarray(mask_ids)
    out = np.zeros(mask_ids.shape, np.int32)
    seen = {}
    for v in mask_ids.ravel():
        if v and v not in seen:
            seen[v] = len(seen) + 1
    for v, k in seen.items():
        out[mask_ids == v] = k
    return out


def _logits(shape, seed):
    return np.random.default_rng(seed).normal(0.0, 2.0, size=(shape[0], 2) + tuple(shape[1:])).astype(np.float32)


def _row(name, maps, dst, filters, seed):
    labels = np.stack([raster_labels(m) for m in maps]).astype(np.int32)
    return dict(name=name, labels=labels, logits=_logits(labels.shape, seed), dst=tuple(dst), min_height=filters[0], min_area=filters[1])


def _many_edged_polygon(k):
    """Filled convex lattice polygon whose edges are ALL primitive vectors (a, b) with |a|, |b| <= k, in order of angle (80 edges for k = 5,
    112 x 112 pixels): bool mask."""
    from math import atan2, gcd
    vecs = sorted(((a, b) for a in range(-k, k + 1) for b in range(-k, k + 1) if gcd(abs(a), abs(b)) == 1), key=lambda v: atan2(v[1], v[0]))
    pts = np.cumsum(np.asarray(vecs, np.int64), 0)
    pts -= pts.min(0)
    yy, xx = np.mgrid[0:pts[:, 1].max() + 1, 0:pts[:, 0].max() + 1]
    inside = np.ones(yy.shape, bool)
    for (ax, ay), (bx, by) in zip(pts, np.roll(pts, -1, 0)):
        inside &= (bx - ax) * (yy - ay) - (by - ay) * (xx - ax) >= 0
    return inside


def _hand_made():
    rows = []
    z = lambda h, w: np.zeros((h, w), np.int32)

    rows.append(_row('empty', [z(20, 20)], (20, 20), (0, 0), 1))

    m = z(20, 20)                                        # identity scale: one-vertex hull, two-vertex hull, a 3 x 3 block
    m[3, 4] = 1
    for i in range(8):
        m[5 + i, 9 + i] = 2
    m[15:18, 2:5] = 3
    rows.append(_row('identity_degenerate_nofilter', [m], (20, 20), (0, 0), 2))
    rows.append(_row('identity_degenerate_cfgfilter', [m], (20, 20), CFG_FILTERS, 2))

    m = z(150, 150)                                      # 150 -> 300: 2 x 2 pixels = 1 x 1, area 1 (dropped by min_area); 4 x 2 = 3 x 1, area 3 (kept)
    m[10, 10] = 1
    m[40, 60:62] = 2
    rows.append(_row('x2_filter_equalities', [m], (300, 300), CFG_FILTERS, 3))

    m = z(75, 75)                                        # 75 -> 300: the closed-form block, single pixel and column of test_pixellink_cpu.py
    m[10:13, 20:25] = 1
    m[40, 40] = 2
    m[50:60, 7] = 3
    rows.append(_row('x4_closed_form', [m], (300, 300), CFG_FILTERS, 4))
    rows.append(_row('x4_closed_form_minheight5', [m], (300, 300), (5, 3), 4))

    yy, xx = np.mgrid[0:40, 0:40]                        # identity: a diamond (four exactly tied edges) and an axis-aligned square
    m = z(40, 40)
    m[np.abs(xx - 12) + np.abs(yy - 10) <= 6] = 1
    m[24:35, 20:31] = 2
    rows.append(_row('ties_identity', [m], (40, 40), CFG_FILTERS, 5))

    yy, xx = np.mgrid[0:150, 0:150]                      # 150 -> 300: the same shapes up-scaled (the diamond becomes an octagon), the longest hull
    m0 = z(150, 150)
    m0[np.abs(xx - 50) + np.abs(yy - 60) <= 12] = 1
    m0[100:121, 30:51] = 2
    m1 = z(150, 150)
    m1[(xx - 75) ** 2 + (yy - 75) ** 2 <= 70 ** 2] = 1
    rows.append(_row('ties_x2_and_disc', [m0, m1], (300, 300), CFG_FILTERS, 6))

    m = z(40, 40)                                        # concavity and order: ring around a component, a "C", a dropped pixel between kept blocks
    m[2:13, 2:13] = 1
    m[4:11, 4:11] = 0
    m[6:8, 6:8] = 2
    m[16:27, 3:13] = 3
    m[19:24, 6:13] = 0
    m[30:34, 2:6] = 4
    m[31, 10] = 5
    m[30:34, 14:20] = 6
    m[16:20, 25:27] = 7                                  # several runs per row: a comb
    m[16:26, 25] = 7
    m[22:26, 25:30] = 7
    m[16:26, 32] = 7
    m[16, 25:33] = 7
    rows.append(_row('concave_and_order', [m], (80, 80), CFG_FILTERS, 7))

    rows.append(_row('whole_map', [np.ones((12, 10), np.int32)], (36, 30), CFG_FILTERS, 8))

    m0 = z(20, 20)                                       # borders: the bilinear border branch
    m0[0, 3:9] = 1
    m0[19, 5:16] = 2
    m0[5:13, 0] = 3
    m0[3:10, 19] = 4
    m1 = z(20, 20)                                       # diagonal bands in two corners: the rotated rectangle leaves the image (the clamp)
    yy, xx = np.mgrid[0:20, 0:20]
    m1[(np.abs(xx - yy) <= 1) & (xx < 7) & (yy < 7)] = 1
    m1[(np.abs(xx + yy - 34) <= 1) & (xx > 12) & (yy > 12)] = 2
    m1[(np.abs(xx + yy - 19) <= 1) & (xx > 13)] = 3
    rows.append(_row('borders_and_clamp', [m0, m1], (60, 60), CFG_FILTERS, 9))

    m = z(30, 40)                                        # non-integer ratio, non-square: 30 x 40 -> 90 x 100 (rows x 3, columns x 2.5)
    m[2:9, 3:6] = 1
    m[2:4, 3:15] = 1
    yy, xx = np.mgrid[0:30, 0:40]
    m[(np.abs(2 * (xx - 20) - 3 * (yy - 18)) <= 4) & (yy > 10) & (yy < 27)] = 2
    m[12:15, 33:40] = 3
    m[27, 1] = 4
    m[29, 30:40] = 5
    rows.append(_row('ratio_3_by_2p5', [m], (90, 100), CFG_FILTERS, 10))

    m = z(75, 75)                                        # 75 -> 200 (x 2.666...)
    yy, xx = np.mgrid[0:75, 0:75]
    m[(xx - 20) ** 2 + 4 * (yy - 15) ** 2 <= 150] = 1
    m[(np.abs(xx - 2 * yy + 40) <= 2) & (yy > 30) & (yy < 60)] = 2
    m[70:75, 70:75] = 3
    m[66, 3:5] = 4
    rows.append(_row('ratio_2p67', [m], (200, 200), CFG_FILTERS, 11))

    m = z(40, 40)                                        # down-scaling 40 x 40 -> 25 x 30: source rows / columns that no destination pixel reads
    m[3:20, 4:9] = 1
    m[2, 20] = 2                                         # row 2 is read by no destination row: the component vanishes
    m[22, 7] = 5                                         # so does this one: no destination column reads column 7
    m[24:36, 15:38] = 3
    m[24:30, 15:20] = 0
    m[38, 2:30] = 4
    rows.append(_row('downscale', [m], (25, 30), (0, 0), 12))

    m = z(163, 163)                                      # the largest square map of the decode (163 x 163 <= 26624 pixels) and a hull of 80
    m[20:132, 30:142][_many_edged_polygon(5)] = 1        # edges: the calipers' second batch of lanes
    rows.append(_row('largest_map_80_edges', [m], (163, 163), CFG_FILTERS, 14))

    m = z(64, 64)                                        # the cap: isolated pixels on every other row and column = exactly 1024 components
    m[::2, ::2] = np.arange(1, 1025).reshape(32, 32)
    rows.append(_row('cap_1024', [m], (128, 128), (0, 0), 13))
    return rows


_CACHE = {}


def hand_made_rows():
    if 'hand' not in _CACHE:
        _CACHE['hand'] = _hand_made()
    return _CACHE['hand']


def seeded_maps():
    """{name: (out1 [B,2,H,W], out2 [B,16,H,W])}: tests/golden/pixellink.npz's decode inputs (75 x 75) and pixellink2s_ref.decode_inputs
    (150 x 150) at B = 3."""
    if 'seeded' not in _CACHE:
        import pixellink2s_ref as R2
        g = np.load(os.path.join(GOLDEN, 'pixellink.npz'), allow_pickle=False)
        _CACHE['seeded'] = {'fixture75': (g['dec_out1'], g['dec_out2']), 'seeded150': R2.decode_inputs(21)}
    return _CACHE['seeded']


def oracle_labels(out1, out2, pixel_thr=None):
    """The CPU oracle's link decoding (bit-equal to the device decode: tests/test_gpu_pixellink*.py)."""
    import torch
    from oracle import pixellink_oracle as PO
    kw = {} if pixel_thr is None else dict(pixel_thr=pixel_thr)
    return PO.decode_links(torch.from_numpy(np.ascontiguousarray(out1)), torch.from_numpy(np.ascontiguousarray(out2)), **kw).astype(np.int32)


def seeded_rows():
    """The seeded maps as registry rows (labels from the CPU oracle's decoding), 300 x 300 destination, the config's filters."""
    if 'seeded_rows' not in _CACHE:
        _CACHE['seeded_rows'] = [dict(name=k, labels=oracle_labels(o1, o2), logits=np.ascontiguousarray(o1, np.float32), dst=(300, 300),
                                      min_height=cfg.min_height, min_area=cfg.min_area) for k, (o1, o2) in seeded_maps().items()]
    return _CACHE['seeded_rows']


def all_rows():
    return hand_made_rows() + seeded_rows()


def host_prob(logits):
    """The positive-class probability as mask_to_box forms it: float32(1 / (1 + exp(float64(l0 - l1))))."""
    logits = np.asarray(logits, np.float32)
    return (1.0 / (1.0 + np.exp((logits[:, 0] - logits[:, 1]).astype(np.float64)))).astype(np.float32)


def host_components(labels, dst):
    """component_boxes' loop for ONE image, before the filters: [(label, rect dict of min_area_rect, ys, xs)] for every component that has
    a destination pixel."""
    res = G.upscale_nearest(np.asarray(labels), dst)
    out = []
    for i in range(1, int(res.max()) + 1):
        ys, xs = np.nonzero(res == i)
        if len(ys):
            out.append((i, G.min_area_rect(np.stack([xs, ys], 1)), ys, xs))
    return out


def host_expected(row):
    """-> per image (boxes [[min_x, min_y, max_x, max_y]], scores) by box_geometry.component_boxes: the definition."""
    prob = host_prob(row['logits'])
    return [G.component_boxes(row['labels'][b], prob[b], row['dst'], row['min_height'], row['min_area']) for b in range(len(prob))]


# ---- the evaluation fixture of the test_net test -----------------------------------------------------------------------------------------
EVAL_THRESH = 0.6
EVAL_SIZE = 300                  # network pixels
EVAL_IMAGE = 128                 # the "dataset" images are 128 x 128: ground truth is scaled by 300 / 128
EVAL_BATCH = 3
EVAL_AP, EVAL_IOBB = (0.1, 0.5), (0.1, 0.5)


def eval_batches():
    """Two batches of 150 x 150 score maps (3 + 2 images).  The fourth image holds one detection whose score falls below the threshold
    (its ground truth still counts); the last image has no positive pixel (its ground truth does not)."""
    if 'eval' not in _CACHE:
        import pixellink2s_ref as R2
        a1, a2 = R2.decode_inputs(21)
        b1, b2 = R2.decode_inputs(23, B=2)
        b1[:, 0], b1[:, 1] = 8.0, -8.0
        b1[0, 0, 50, 40:53], b1[0, 1, 50, 40:53] = 0.0, np.float32(np.log(0.7 / 0.3))     # a thin line at p = 0.7: its blended score is below thresh
        b2[0, 0::2], b2[0, 1::2] = -5.0, 5.0
        _CACHE['eval'] = [(a1, a2), (b1, b2)]
    return _CACHE['eval']


def eval_annotations(host_dets):
    """Ground truth for the five images from the HOST detections ``host_dets`` (per image [[score, x0, y0, x1, y1], ...] in network pixels):
    every third detection, shifted and stretched by a few pixels, plus one box nothing matches; in dataset pixels, label column appended.
    The image without a detection still owns one box (which the reference never counts)."""
    annos = []
    for i, dets in enumerate(host_dets):
        boxes = [[d[1] + 3, d[2] - 2, d[3] + 5, d[4] + 1] for d in dets[::3]] + [[5.0 + i, 280.0, 20.0 + i, 295.0]]
        a = np.asarray(boxes, np.float64) * EVAL_IMAGE / EVAL_SIZE
        annos.append(np.concatenate([a, np.zeros((len(a), 1))], 1))
    return annos
