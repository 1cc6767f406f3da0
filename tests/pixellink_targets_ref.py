"""A numpy restatement of the PixelLink targets (include/gssd_hip.h, gssd_pixellink_targets), written in the kernel's gather form,
and the cases of tests/golden/pixellink_targets.npz (tests/golden/make_golden_pixellink_targets.py)."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pixellink_targets.npz')
DIRS = ((1, 1), (1, 0), (1, -1), (0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1))
KEYS = ('pixel_mask', 'neg_pixel_mask', 'pixel_pos_weight', 'link_mask')
# the chained cases: SSDAugmentation(use_pixel_link=True), CHAIN_B consecutive calls from one seed on synth_study_u8(7000 + i)
VERSIONS = ('4s', '2s')
CHAIN_SEEDS = {'4s': 7100, '2s': 7200}
CHAIN_B, CHAIN_SRC, CHAIN_SIZE = 4, 64, 300
CHAIN_BOXES = ([[0.30, 0.35, 0.55, 0.60, 0.]],
               [[0.10, 0.12, 0.30, 0.28, 0.], [0.45, 0.40, 0.70, 0.75, 0.], [0.50, 0.45, 0.92, 0.90, 0.]])


def factor_of(version):
    return 2 if version == '2s' else 4


def targets(boxes, size, version):
    """One image: float32 percent boxes [n, >= 4] -> (pixel_mask int64, neg int64, weight float64, link int64 [8, M, M])."""
    factor = factor_of(version)
    M = int(size / factor)
    b = np.asarray(boxes, np.float32)
    b = b.reshape(0, 4) if b.size == 0 else b[:, :4]
    c = (b * np.float32(size)).astype(np.float32).astype(np.int64)
    c = np.trunc(c / factor).astype(np.int64)                    # C division, truncation toward zero
    cnt = np.zeros((M, M), np.int64)
    owner = np.full((M, M), -1, np.int64)
    for i, (x0, y0, x1, y1) in enumerate(c):
        r0, r1 = max(min(y0, y1), 0), min(max(y0, y1), M - 1)
        c0, c1 = max(min(x0, x1), 0), min(max(x0, x1), M - 1)
        if r0 > r1 or c0 > c1:
            continue
        cnt[r0:r1 + 1, c0:c1 + 1] += 1
        owner[r0:r1 + 1, c0:c1 + 1] = i
    owner[cnt != 1] = -1
    pix = (cnt == 1).astype(np.int64)
    neg = (cnt == 0).astype(np.int64)
    area = np.bincount(owner[owner >= 0], minlength=len(c)) if len(c) else np.zeros(0, np.int64)
    A, R = int(area.sum()), int((area > 0).sum())
    weight = np.zeros((M, M), np.float64)
    link = np.zeros((8, M, M), np.int64)
    if R == 0:
        return pix, neg, weight, link
    avg = A / R
    for i in np.nonzero(area)[0]:
        weight[owner == i] = avg / float(area[i])
    idx = np.arange(M)
    for j, (dh, dw) in enumerate(DIRS):
        hit = np.zeros((M, M), bool)
        # gather: q is reached from p with clip(p + d) == q; per axis at most two such p
        for ph in _pre(idx, dh, M):
            for pw in _pre(idx, dw, M):
                ok = (ph[:, None] >= 0) & (pw[None, :] >= 0)
                src = owner[np.clip(ph, 0, M - 1)][:, np.clip(pw, 0, M - 1)]
                hit |= ok & (src == owner) & (owner >= 0)
        link[j] = hit
    return pix, neg, weight, link


def _pre(q, d, M):
    """Per-axis preimage of q under p -> clip(p + d, 0, M - 1): up to two index arrays, -1 where there is none."""
    a = q - d
    first = np.where((a >= 0) & (a < M), a, -1)
    if d == 0:
        return [first]
    edge = M - 1 if d > 0 else 0
    return [first, np.where(q == edge, q, -1)]


def batch(boxes_list, size, version):
    """The collate's stacked arrays (weight still float64) for a list of images."""
    outs = [targets(b, size, version) for b in boxes_list]
    return {k: np.stack([o[i] for o in outs]) for i, k in enumerate(KEYS)}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load():
    return np.load(GOLDEN, allow_pickle=False)


class Case:
    """One fixture case: its images' boxes, size, version and the reference's stacked outputs (weight in float64)."""

    def __init__(self, g, name):
        pre = name + '__'
        self.name = name
        self.size = int(g[pre + 'size'])
        self.version = str(g[pre + 'version'])
        counts = g[pre + 'counts']
        flat = g[pre + 'boxes']
        offs = np.concatenate([[0], np.cumsum(counts)])
        self.boxes = [flat[offs[i]:offs[i + 1]] for i in range(len(counts))]
        self.want = {k: g[pre + k] for k in KEYS}


def cases(g):
    return [Case(g, str(n)) for n in g['names']]
