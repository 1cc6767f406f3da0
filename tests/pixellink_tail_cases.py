"""Registry of the PixelLink tail cases (csrc/pixellink.hip: PixelLinkLoss forward / backward, the link decoding, the upsample-add cascade and
the final 1x1 convs with their weight gradients), shared by tests/test_pixellink_tail_cases_cpu.py (which proves every row reaches the branch
it names and that the classic mistakes fail at least one row), tests/golden/make_golden_pixellink_tail.py (what the imported reference
computes where it defines a result) and tests/test_gpu_pixellink_tail.py (which runs the rows on the device).  TEST INFRASTRUCTURE ONLY.

A row is rebuilt from its name and seed; nothing here reads a fixture.  The shapes are the smallest at which the branch the row names can go
wrong.  The restatements below (``mine`` / ``loss_reference``, ``decode64``, ``interp64``, ``final64``) are plain float64 statements of what the
kernels compute; each takes a ``mutant`` that applies one classic mistake, for the CPU module.  ``final32`` and the float32 forms of the
interp restatements give the e_cpu32 of the measured gates (GATES, at the end).

Loss rows.  No decision is left to rounding: d = out1[:, 0] - out1[:, 1] is a multiple of 2^-6 with |d| <= 6 and is exact in fp32 (out1[:, 1]
is a multiple of 2^-4, out1[:, 0] = out1[:, 1] + d), the background probability p0 = sigmoid(d) depends on d alone, and adjacent levels differ
by more than 64 fp32 ulp (asserted in the CPU module), so equal p0 means equal d and the mined mask, area and neg_area are exact.  The
'saturated' rows use d = -120, 0, 24 instead: p0 = 0, 0.5, 1 bit-exactly on any implementation.

Decode rows.  A row starts from a hand-made id map; the expected label map is its raster renumbering BY CONSTRUCTION.  Pixel logits are -+5,
links between 8-neighbours of the same id are lit by the row's mode, links between different ids are off."""
import functools
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = os.path.join(ROOT, 'grouped-ssd-pytorch_amd', 'gssd', 'csrc', 'pixellink.hip')

# the limits of csrc/pixellink.hip the rows are placed around (held against the source by the CPU module)
PL_SORT = 8192            # pl_loss_kernel (bitonic sort) up to here, pl_loss_select_kernel (radix select) above
PL_MAXPIX = 8192          # pl_decode_kernel up to here, pl_decode_lds_kernel above
PL_MAXPIX_LDS = 26624     # the decode's hard limit
PL_STAT_COMPS = 1024      # components with statistics
TP = 128                  # pixels per pass of the two weight-gradient kernels
NEG_POS_RATIO = 3         # pixel_link_config.neg_pos_ratio
PIXEL_THR, LINK_THR = 0.2, 0.8
EMPTY_COMP = (0.0, 1e9, 1e9, -1.0, -1.0, 0.0)
NEIGH = [(-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1)]


def source_constants():
    src = open(HIP).read()
    out = {k: int(re.search(r'constexpr int %s = (\d+);' % k, src).group(1)) for k in ('PL_SORT', 'PL_MAXPIX', 'PL_MAXPIX_LDS', 'PL_STAT_COMPS')}
    out['TP'] = sorted(set(int(v) for v in re.findall(r'constexpr int TP = (\d+);', src)))
    out['sort_switch'] = 'if (H * W <= PL_SORT)' in src
    out['decode_switch'] = 'if (H * W <= PL_MAXPIX)' in src
    out['decode_limit'] = '(long long)H * W <= PL_MAXPIX_LDS' in src
    out['wgrad_blocks'] = src.count('(total + 127) / 128')
    return out


# ------------------------------------------------------------------------------------------------------------------------------------------
# loss rows
# ------------------------------------------------------------------------------------------------------------------------------------------
GRID = 2.0 ** -6
JMAX = 384                                        # |d| <= 6
SAT = (-120.0, 0.0, 24.0)                         # p0 = 0, 0.5, 1
SORT_SIZES = [(5, 7), (31, 33), (32, 32), (25, 41), (64, 128)]
SELECT_SIZES = [(3, 2731), (91, 91), (100, 101)]
SWITCH = [(64, 128), (3, 2731)]                   # the last map of the sort, the first of the select


def _image_spec(content, n):
    """-> dict(npos, groups [(kind, count)], pos_cand, other, links, posw_zero): how the n pixels of one image are spent."""
    p8, p16 = max(1, n // 8), max(1, n // 16)
    s = dict(npos=p8, groups=[('any', (n - p8) * 3 // 4)], pos_cand=0, other=0, links='seeded', posw_zero=False)
    if content == 'ordinary':
        s.update(npos=max(1, n // 12), groups=[('any', (n - max(1, n // 12)) * 4 // 5)])
    elif content == 'no_positives':
        s.update(npos=0, groups=[('any', n if n >= 10000 else n - n // 10)])
    elif content == 'fewer_candidates':
        s.update(npos=n // 4, groups=[('any', 3 * (n // 4) - 1 - (n // 4) // 3)])
    elif content == 'exact_k':
        s.update(npos=n // 4, groups=[('any', 3 * (n // 4))])
    elif content == 'k_is_1':
        s.update(npos=1, groups=[('any', n // 2)])
    elif content == 'one_candidate':
        s.update(npos=2, groups=[('any', 1)])
    elif content.startswith('ties_'):
        k = NEG_POS_RATIO * p16
        a, b = max(2, k // 3), max(1, k // 3)
        below, tie = {'ties_straddle': (k - a, a + b), 'ties_ends': (k - a, a), 'ties_begins': (k - 1, a)}[content]
        s.update(npos=p16, groups=[('below', below), ('tie', tie), ('above', n // 8)])
    elif content.startswith('saturated_'):
        k = NEG_POS_RATIO * p16
        g = {'saturated_0': (k + 2, 2, 2), 'saturated_half': (k - 2, 4, 2), 'saturated_1': (1, 1, k)}[content]
        s.update(npos=p16, groups=[('s0', g[0]), ('s5', g[1]), ('s1', g[2])])
    elif content == 'mask_values':
        s.update(pos_cand=p8 // 2, groups=[('any', (n - p8) // 3)], other=2)
    elif content == 'no_candidates':
        s.update(groups=[])
    elif content == 'nothing_at_all':
        s.update(npos=0, groups=[], posw_zero=True)
    elif content == 'links_all_1':
        s.update(links=1)
    elif content == 'links_all_0':
        s.update(links=0)
    elif content == 'posw_zero':
        s.update(posw_zero=True)
    else:
        raise KeyError(content)
    return s


def _levels(kind, count, rng):
    if kind == 'any':
        return rng.integers(-JMAX, JMAX + 1, count) * GRID
    if kind == 'below':
        return rng.integers(-JMAX, 0, count) * GRID
    if kind == 'above':
        return rng.integers(1, JMAX + 1, count) * GRID
    return np.full(count, {'tie': 0.0, 's0': SAT[0], 's5': SAT[1], 's1': SAT[2]}[kind])


def _loss_image(content, H, W, rng):
    n = H * W
    s = _image_spec(content, n)
    order = rng.permutation(n)
    d = rng.integers(-JMAX, JMAX + 1, n) * GRID
    pix, neg = np.zeros(n, np.int64), np.zeros(n, np.uint8)
    npos = s['npos']
    pix[order[:npos]] = 1
    neg[order[:s['pos_cand']]] = 1                                   # candidates that are also positives
    at = npos
    for kind, count in s['groups']:
        idx = order[at:at + count]
        assert len(idx) == count, (content, H, W, 'the map is too small for the row')
        neg[idx] = 1
        d[idx] = _levels(kind, count, rng)
        at += count
    rest = order[at:]
    if s['other']:
        neg[rest[::2]] = s['other']                                  # mask values that are no candidates (2), the others stay 0
    c = rng.integers(-32, 33, n) / 16.0
    out1 = np.stack([c + d, c]).astype(np.float32)
    assert np.array_equal(out1[0].astype(np.float64) - out1[1].astype(np.float64), d)
    posw = (pix * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    if s['posw_zero']:
        posw[:] = 0
    link = (rng.random((8, n)) > 0.4).astype(np.int64) * pix[None]
    if s['links'] != 'seeded':
        link[:] = s['links']
    out2 = rng.normal(0, 2.0, (16, n)).astype(np.float32)
    r = lambda a: a.reshape(a.shape[:-1] + (H, W))
    return dict(out1=r(out1), out2=r(out2), pix=r(pix), neg=r(neg), posw=r(posw), link=r(link))


class LossRow:
    def __init__(self, contents, H, W, seed, ratio=NEG_POS_RATIO):
        self.contents, self.H, self.W, self.seed, self.ratio = tuple(contents), H, W, seed, ratio
        self.name = f"{'+'.join(contents) if len(contents) < 4 else 'mixed_batch'} {H}x{W}"
        self.B = len(contents)

    @property
    def through_criterion(self):
        """PixelLinkLoss normalises the mask to 0 / 1 and takes the configured ratio: rows that need another mask value or ratio go to the C
        entry alone; so does the row whose means are NaN by contract."""
        return self.ratio == NEG_POS_RATIO and not set(self.contents) & {'mask_values', 'nothing_at_all'}

    def build(self):
        rng = np.random.default_rng(self.seed)
        imgs = [_loss_image(c, self.H, self.W, rng) for c in self.contents]
        return {k: np.stack([im[k] for im in imgs]) for k in imgs[0]}


def _loss_rows():
    rows, seed = [], 100
    single = ['ordinary', 'no_positives', 'fewer_candidates', 'exact_k', 'k_is_1', 'one_candidate', 'ties_straddle', 'ties_ends', 'ties_begins',
              'mask_values', 'no_candidates', 'nothing_at_all', 'links_all_1', 'links_all_0', 'posw_zero']
    sat = ['saturated_0', 'saturated_half', 'saturated_1']
    mixed = ['no_positives', 'ties_straddle', 'no_candidates', 'ordinary']
    for H, W in SWITCH:                                              # the same content rule on both sides of the switch
        for c in single:
            rows.append(LossRow([c], H, W, seed, ratio=1 if c == 'k_is_1' else NEG_POS_RATIO))
            seed += 1
        rows.append(LossRow(sat, H, W, seed))
        rows.append(LossRow(mixed, H, W, seed + 1))
        seed += 2
    for H, W in SORT_SIZES[:-1] + SELECT_SIZES[1:]:
        for c in ('ordinary', 'ties_straddle'):
            rows.append(LossRow([c], H, W, seed))
            seed += 1
    rows.append(LossRow(sat, 5, 7, seed))
    for H, W in SELECT_SIZES[1:]:                                    # on 100 x 101 every pixel is a candidate: neg_area = 10000 exactly
        rows.append(LossRow(['no_positives'], H, W, seed + 1))
        seed += 1
    return rows


LOSS = _loss_rows()


def sigmoid64(d):
    return 1.0 / (1.0 + np.exp(-np.asarray(d, np.float64)))


def mine(d, neg, pix, ratio, mutant=None):
    """criterion.py:35-47 for one image in float64: -> (mined mask bool, area, ncand, neg_area).  ncand == 0 selects nothing (the reference
    raises there).  mutant: 'lt' (< at the cut), 'rank_plus_1', 'no_10000', 'mask_nonzero'."""
    d, neg, pix = np.asarray(d, np.float64).ravel(), np.asarray(neg).ravel(), np.asarray(pix).ravel()
    p0 = sigmoid64(d)
    cand = (neg != 0) if mutant == 'mask_nonzero' else (neg == 1)
    area, ncand = int(pix.sum()), int(cand.sum())
    r = area * ratio
    if r == 0 and mutant != 'no_10000':
        r = 10000
    k = min(r, ncand)
    if k == 0:
        return np.zeros(d.shape, bool), area, ncand, 0
    s = np.sort(p0[cand])
    thr = s[min(k + 1, ncand) - 1] if mutant == 'rank_plus_1' else s[k - 1]
    return cand & ((p0 < thr) if mutant == 'lt' else (p0 <= thr)), area, ncand, k


UPSTREAM = (1.0, 0.7, 2.0, 0.3)


@functools.lru_cache(maxsize=None)
def loss_reference(i):
    """Row LOSS[i] in float64: dict(inp, mask [B,H,W] bool, area, ncand, neg_area [B], per_image [B,4] (NaN where area + neg_area == 0),
    d1, d2 = gradients of sum_k UPSTREAM[k] * (1 / B) sum_b per_image[b, k] over the images where the term is defined, mask constant)."""
    import torch
    import torch.nn.functional as F
    row = LOSS[i]
    inp = row.build()
    B = row.B
    d = inp['out1'][:, 0].astype(np.float64) - inp['out1'][:, 1].astype(np.float64)
    m = [mine(d[b], inp['neg'][b], inp['pix'][b], row.ratio) for b in range(B)]
    mask = np.stack([x[0] for x in m]).reshape(B, row.H, row.W)
    area, ncand, neg_area = (np.array([x[j] for x in m], np.int64) for j in (1, 2, 3))
    o1 = torch.from_numpy(inp['out1']).double().requires_grad_()
    o2 = torch.from_numpy(inp['out2']).double().requires_grad_()
    pix, link = torch.from_numpy(inp['pix']), torch.from_numpy(inp['link'])
    posw = torch.from_numpy(inp['posw']).double()
    ce = F.cross_entropy(o1, pix, reduction='none')
    den = torch.from_numpy(area + neg_area).double()
    ok = den > 0
    sden = torch.where(ok, den, torch.ones_like(den))
    pos = (posw * ce).view(B, -1).sum(1) / sden
    neg = (torch.from_numpy(mask).double() * ce).view(B, -1).sum(1) / sden
    lce = torch.stack([F.cross_entropy(o2[:, 2 * n:2 * n + 2], link[:, n], reduction='none') for n in range(8)], 1)
    w = posw.unsqueeze(1)
    wp, wn = (link == 1).double() * w, (link == 0).double() * w
    swp, swn = wp.view(B, -1).sum(1), wn.view(B, -1).sum(1)
    lp = torch.where(swp == 0, torch.zeros_like(swp), (wp * lce).view(B, -1).sum(1) / swp.clamp_min(1e-300))
    ln = torch.where(swn == 0, torch.zeros_like(swn), (wn * lce).view(B, -1).sum(1) / swn.clamp_min(1e-300))
    okf = ok.double()
    total = (UPSTREAM[0] * (pos * okf).sum() + UPSTREAM[1] * (neg * okf).sum() + UPSTREAM[2] * lp.sum() + UPSTREAM[3] * ln.sum()) / B
    total.backward()
    nan = torch.full_like(den, float('nan'))
    per = torch.stack([torch.where(ok, pos, nan), torch.where(ok, neg, nan), lp, ln], 1).detach().numpy()
    return dict(inp=inp, mask=mask, area=area, ncand=ncand, neg_area=neg_area, per_image=per, d1=o1.grad.numpy(), d2=o2.grad.numpy())


def reference_defines_loss(i):
    """The reference's topk[-1] raises without a candidate; without a positive or mined pixel its means are NaN."""
    r = loss_reference(i)
    return bool((r['ncand'] >= 1).all() and (r['area'] + r['neg_area'] > 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------------
# decode rows
# ------------------------------------------------------------------------------------------------------------------------------------------
def raster_labels(ids):
    """Renumber an id map (0 = background) so that ids follow the raster order of each component's first pixel."""
    ids = np.asarray(ids)
    flat = ids.ravel()
    first = {}
    for i in np.flatnonzero(flat):
        first.setdefault(int(flat[i]), len(first) + 1)
    lut = np.zeros(int(flat.max()) + 1 if flat.size else 1, np.int32)
    for v, k in first.items():
        lut[v] = k
    return lut[ids].astype(np.int32)


def logits_from_ids(ids, mode, seed=0, decoys=False, score_seed=None):
    """-> (out1 [2,H,W], out2 [16,H,W]) for one id map.  mode: 'both' (each pixel of a same-id pair lights its link to the other), 'forward_only'
    (only the raster-earlier pixel does), 'backward_only', 'seeded' (one of the two, by seed).  decoys: positive pixels also light their links
    towards non-positive pixels and off the map, and every link of a non-positive pixel is lit.  score_seed: the positive pixels' logits vary."""
    ids = np.asarray(ids)
    H, W = ids.shape
    rng = np.random.default_rng(seed)
    on = np.zeros((8, H, W), bool)
    pos = ids > 0
    for n in (3, 4, 5, 6):                                            # each unordered pair once, from its raster-earlier pixel
        dy, dx = NEIGH[n]
        ys, xs = np.nonzero(pos)
        yy, xx = ys + dy, xs + dx
        ok = (yy < H) & (xx >= 0) & (xx < W)
        ys, xs, yy, xx = ys[ok], xs[ok], yy[ok], xx[ok]
        same = ids[ys, xs] == ids[yy, xx]
        ys, xs, yy, xx = ys[same], xs[same], yy[same], xx[same]
        pick = rng.random(len(ys)) < 0.5
        fwd = {'both': True, 'forward_only': True, 'backward_only': False, 'seeded': pick}[mode] & np.ones(len(ys), bool)
        bwd = {'both': True, 'forward_only': False, 'backward_only': True, 'seeded': ~pick}[mode] & np.ones(len(ys), bool)
        on[n, ys[fwd], xs[fwd]] = True
        on[(n + 4) & 7, yy[bwd], xx[bwd]] = True
    if decoys:
        for n, (dy, dx) in enumerate(NEIGH):
            ys, xs = np.nonzero(pos)
            yy, xx = ys + dy, xs + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            tgt_pos = np.zeros(len(ys), bool)
            tgt_pos[inside] = pos[yy[inside], xx[inside]]
            on[n, ys[~tgt_pos], xs[~tgt_pos]] = True                  # off the map, or towards a non-positive pixel
        on[:, ~pos] = True
    return _logits(pos, on, rng if score_seed is None else np.random.default_rng(score_seed), score_seed is not None)


# Varied scores: a positive pixel's logits are (-5 + j / 8, 5).  The statistics' score sum is held to count * 2^-24 * sum|score| of the float64
# sum -- the bound of fp32 ADDS, which has no room for the rounding of the summands.  A one-pixel component is a single summand, so only the
# levels whose fp32 score (two roundings: 1 + e0, then the divide; e0 = expf(-10 + j / 8) give or take an ulp) stays within 0.75 of that bound
# are used; j = 5, 7, 21 exceed it with correctly rounded arithmetic (tests/test_pixellink_tail_cases_cpu.py).
SCORE_J = (0, 2, 3, 4, 6, 8, 9, 10, 12, 13, 15, 16, 18, 22, 23, 25, 26, 28, 29, 31)


def score_level_ratio(j):
    """|fp32 score - float64 score| / (2^-24 * score) of the level, the worst over e0 one ulp either way."""
    f = np.float32
    a, c = f(-5 + j / 8), f(5)
    ref = 1.0 / (1.0 + np.exp(np.float64(a) - np.float64(c)))
    worst = 0.0
    for de in (-1, 0, 1):
        e0 = f(np.exp(np.float64(a - c)))
        e0 = np.nextafter(e0, f(de * 10)) if de else e0
        worst = max(worst, abs(float(f(f(1) / f(e0 + f(1)))) - ref) / (2.0 ** -24 * ref))
    return worst


def _logits(pos, on, rng, vary):
    H, W = pos.shape
    out1 = np.empty((2, H, W), np.float32)
    out1[0] = np.where(pos, -5.0, 5.0)
    out1[1] = np.where(pos, 5.0, -5.0)
    if vary:
        out1[0] = np.where(pos, -5.0 + np.asarray(SCORE_J)[rng.integers(0, len(SCORE_J), (H, W))] / 8.0, 5.0)
    out2 = np.empty((16, H, W), np.float32)
    out2[0::2] = np.where(on, -5.0, 5.0)
    out2[1::2] = np.where(on, 5.0, -5.0)
    return out1, out2


class DecodeRow:
    """builder() -> list of per-image (ids, out1, out2) (ids = the hand-made id map, 0 where the pixel must come out as background)."""

    def __init__(self, name, builder, max_comps=(512,), thr=(None, None), error=False):
        self.name, self.builder, self.max_comps, self.thr, self.error = name, builder, tuple(max_comps), thr, error

    def build(self):
        imgs = self.builder()
        ids = np.stack([im[0] for im in imgs])
        return dict(ids=ids, labels=np.stack([raster_labels(im[0]) for im in imgs]), out1=np.stack([im[1] for im in imgs]),
                    out2=np.stack([im[2] for im in imgs]))

    @property
    def thresholds(self):
        return (PIXEL_THR if self.thr[0] is None else self.thr[0], LINK_THR if self.thr[1] is None else self.thr[1])


def _from_ids(ids, mode='both', **kw):
    ids = np.asarray(ids, np.int32)
    return (ids,) + logits_from_ids(ids, mode, **kw)


def _row_wrap(H, W):
    """Every row holds two runs with ids of their own, linked inside the run only.  Last-column pixels light (0,+1) and (+1,+1), first-column
    pixels (0,-1), (+1,-1) and (-1,-1): each leaves the map, and the pixel at the flat index it would wrap to is positive with another id."""
    ids = np.zeros((H, W), np.int32)
    half = (W + 1) // 2
    for y in range(H):
        ids[y, :half], ids[y, half:] = 2 * y + 1, 2 * y + 2
    _, out1, out2 = _from_ids(ids, 'both')
    for n in (3, 4):
        out2[2 * n, :, W - 1], out2[2 * n + 1, :, W - 1] = -5.0, 5.0
    for n in (7, 6, 0):
        out2[2 * n, :, 0], out2[2 * n + 1, :, 0] = -5.0, 5.0
    return [(ids, out1, out2)]


def _one_direction():
    """16 two-pixel components on 16 x 20: pair k = (direction n = k % 8, variant k // 8); variant 0 lights only bit n of p, variant 1 only bit
    (n + 4) & 7 of q = p + direction n."""
    ids = np.zeros((16, 20), np.int32)
    on = np.zeros((8, 16, 20), bool)
    for k in range(16):
        n, var = k % 8, k // 8
        py, px = (k // 4) * 4 + 1, (k % 4) * 5 + 2
        qy, qx = py + NEIGH[n][0], px + NEIGH[n][1]
        ids[py, px] = ids[qy, qx] = k + 1
        if var == 0:
            on[n, py, px] = True
        else:
            on[(n + 4) & 7, qy, qx] = True
    return [(ids,) + _logits(ids > 0, on, None, False)]


def _diag_only(all_links):
    H, W = 9, 11
    yy, xx = np.mgrid[0:H, 0:W]
    board = (yy + xx) % 2 == 0
    if all_links:
        return [_from_ids(board.astype(np.int32), 'both', decoys=True)]
    ids = np.where(board, np.arange(1, H * W + 1).reshape(H, W), 0).astype(np.int32)
    _, out1, out2 = _from_ids(ids, 'both')
    for n in (3, 5):                                                  # only (0,+1) and (+1,0) lit: on a checkerboard they reach nobody
        out2[2 * n], out2[2 * n + 1] = -5.0, 5.0
    return [(ids, out1, out2)]


def _late_merge(mode):
    ids = np.zeros((12, 31), np.int32)
    ids[0:11, 0:13:2] = 1                                             # a comb: seven teeth that start as roots on row 0 ...
    ids[11, 0:13] = 1                                                 # ... and join on the last row
    ids[0:6, 15], ids[0:6, 19], ids[6, 15:20] = 2, 2, 2               # a U
    ids[2, 17] = 4                                                    # a pixel inside the U
    for t in range(8):
        ids[1 + t, 28 - t] = 3                                        # a '/' diagonal: its first raster pixel is reached through (+1,-1) only
    ids[3, 1], ids[9, 30] = 5, 6                                      # a pixel between two teeth (its neighbours have another id), a late one
    return [_from_ids(ids, mode, seed=5, decoys=True)]


def serpentine_ids(H, W):
    ids = np.zeros((H, W), np.int32)
    ids[0::2] = 1
    ids[1::4, W - 1] = 1
    ids[3::4, 0] = 1
    return ids


def _thresholds():
    """pixel_thres = link_thres = 0.5.  Column 4 of every row has a == c (probability exactly 0.5: not positive) between two runs that light
    their links towards it; rows 2 / 3 hold one id each side and the vertical links between them sit exactly at 0.5 (not lit)."""
    ids = np.zeros((6, 9), np.int32)
    for y in range(6):
        ids[y, 0:4], ids[y, 5:9] = 2 * y + 1, 2 * y + 2
    ids[1, 0:4], ids[1, 5:9] = ids[0, 0], ids[0, 8]                   # rows 0 and 1 belong together (really linked)
    _, out1, out2 = _from_ids(ids, 'both', decoys=True)
    out1[:, :, 4] = 1.25                                              # a == c
    for n in range(8):                                                # rows 2 <-> 3 (different ids): every link between them exactly at 0.5
        dy = NEIGH[n][0]
        if dy == 1:
            out2[2 * n:2 * n + 2, 2, :] = 0.75
        if dy == -1:
            out2[2 * n:2 * n + 2, 3, :] = 0.75
    ids[:, 4] = 0
    return [(ids, out1, out2)]


def _rank_chunks(H, W):
    HW = H * W
    per = -(-HW // 1024)
    flat = np.zeros(HW, np.int32)
    at = sorted({i for t in (1, 2, 5, 17, 64, 65, 500, 937, 1023) for i in (per * t - 1, per * t) if i < HW} | {HW - 1})
    flat[at] = np.arange(1, len(at) + 1)
    return [_from_ids(flat.reshape(H, W), 'both', decoys=True)]


def block_ids(H, W, bh, bw, seed):
    """Blocks of bh x bw tile the map; each is a component of its own or (one in four, by seed) background."""
    rng = np.random.default_rng(seed)
    nby, nbx = -(-H // bh), -(-W // bw)
    keep = rng.random((nby, nbx)) > 0.25
    blk = np.where(keep, np.arange(1, nby * nbx + 1).reshape(nby, nbx), 0)
    return np.repeat(np.repeat(blk, bh, 0), bw, 1)[:H, :W].astype(np.int32)


def isolated_ids(H, W, count):
    """The first `count` pixels (raster order) of the even-row, even-column lattice: `count` one-pixel components."""
    ids = np.zeros((H, W), np.int32)
    ys, xs = np.nonzero(np.ones((-(-H // 2), -(-W // 2)), bool))
    assert len(ys) >= count
    ids[2 * ys[:count], 2 * xs[:count]] = np.arange(1, count + 1)
    return ids


def checkerboard_ids(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where((yy + xx) % 2 == 0, yy * W + xx + 1, 0).astype(np.int32)


def _bars():
    ids = np.zeros((24, 64), np.int32)                                # one row = one wave: every wave holds one component
    for k in range(8):
        ids[3 * k:3 * k + 2, (5 if k % 2 else 0):(50 if k % 2 else 64)] = k + 1
    return [_from_ids(ids, 'seeded', seed=3, score_seed=11)]


def _stripes():
    H, W = 20, 70
    ids = np.zeros((H, W), np.int32)
    ids[0, :] = 1
    ids[1:H - 1, 0::2] = 1
    ids[H - 1, :] = 2
    ids[1:H - 1, 1::2] = 2
    return [_from_ids(ids, 'both', score_seed=12)]


def _decode_rows():
    D = DecodeRow
    rows = [D('row_wrap 5x13', lambda: _row_wrap(5, 13)), D('row_wrap 13x5', lambda: _row_wrap(13, 5)),
            D('one_direction', _one_direction),
            D('diag_only all links', lambda: _diag_only(True)), D('diag_only orthogonal links', lambda: _diag_only(False)),
            D('late_merge both', lambda: _late_merge('both')), D('late_merge seeded', lambda: _late_merge('seeded')),
            D('late_merge forward_only', lambda: _late_merge('forward_only')), D('late_merge backward_only', lambda: _late_merge('backward_only')),
            D('thresholds', _thresholds, thr=(0.5, 0.5))]
    for H in (75, 150):
        for mode in ('both', 'seeded'):
            rows.append(D(f'serpentine {H}x{H} {mode}', lambda H=H, mode=mode: [_from_ids(serpentine_ids(H, H), mode, seed=H)]))
    for H, W in ((5, 7), (31, 33), (32, 32), (25, 41), (75, 75)):
        rows.append(D(f'rank_chunks {H}x{W}', lambda H=H, W=W: _rank_chunks(H, W)))
    rows.append(D('sizes 1x1 positive', lambda: [_from_ids([[1]], 'both', decoys=True)]))
    rows.append(D('sizes 1x1 negative', lambda: [_from_ids([[0]], 'both', decoys=True)]))
    for H, W, bh, bw in ((1, 40, 1, 3), (40, 1, 3, 1), (64, 128, 6, 8), (3, 2731, 2, 9), (91, 91, 6, 8), (128, 208, 6, 8)):
        rows.append(D(f'sizes {H}x{W}', lambda H=H, W=W, bh=bh, bw=bw: [_from_ids(block_ids(H, W, bh, bw, H + W), 'seeded', seed=W, decoys=True)]))
    rows.append(D('sizes 1x26625', lambda: [_from_ids(np.zeros((1, PL_MAXPIX_LDS + 1), np.int32), 'both')], error=True))
    for count in (1023, 1024, 1025):
        rows.append(D(f'table {count}', lambda count=count: [_from_ids(isolated_ids(64, 66, count), 'both', decoys=True, score_seed=count)],
                      max_comps=(1, 512, 1024, 2048)))
    rows.append(D('table 2813', lambda: [_from_ids(checkerboard_ids(75, 75), 'both', score_seed=7)], max_comps=(1, 512, 1024, 2048)))
    rows.append(D('stats_paths bars', _bars))
    rows.append(D('stats_paths stripes', _stripes))
    rows.append(D('batch', lambda: [_one_direction()[0], _from_ids(np.zeros((16, 20), np.int32), 'both', decoys=True),
                                   _from_ids(block_ids(16, 20, 3, 4, 9), 'seeded', seed=9, decoys=True)]))
    return rows


DECODE = _decode_rows()


def is_connected(region):
    """8-connectivity of a bool map by a plain BFS."""
    region = np.asarray(region, bool)
    H, W = region.shape
    ys, xs = np.nonzero(region)
    if len(ys) == 0:
        return True
    seen = np.zeros_like(region)
    seen[ys[0], xs[0]] = True
    todo = [(int(ys[0]), int(xs[0]))]
    while todo:
        y, x = todo.pop()
        for dy, dx in NEIGH:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and region[yy, xx] and not seen[yy, xx]:
                seen[yy, xx] = True
                todo.append((yy, xx))
    return bool(seen.sum() == region.sum())


def decode64(out1, out2, pixel_thr=PIXEL_THR, link_thr=LINK_THR, mutant=None):
    """The link decoding of one image in float64, stated the way the kernel walks it (every pixel looks at its four forward neighbours; a pair
    is joined when either end lights its link to the other): -> int32 labels [H,W].  mutant: 'ge' (>= at both thresholds), 'no_clip' (flat
    neighbour index without the column test), 'opp_n' (opposite bit taken as n), 'drop_6' (no (+1,-1) neighbour)."""
    out1, out2 = np.asarray(out1, np.float64), np.asarray(out2, np.float64)
    _, H, W = out1.shape
    HW = H * W
    cmp = np.greater_equal if mutant == 'ge' else np.greater
    pos = cmp(sigmoid64(out1[1] - out1[0]), np.float64(np.float32(pixel_thr))).ravel()
    bits = [cmp(sigmoid64(out2[2 * n + 1] - out2[2 * n]), np.float64(np.float32(link_thr))).ravel() & pos for n in range(8)]
    parent = np.arange(HW)

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i in np.flatnonzero(pos):
        y, x = divmod(int(i), W)
        for n in (3, 4, 5, 6):
            if mutant == 'drop_6' and n == 6:
                continue
            dy, dx = NEIGH[n]
            if mutant == 'no_clip':
                q = i + dy * W + dx
                if q >= HW:
                    continue
            else:
                yy, xx = y + dy, x + dx
                if yy >= H or xx < 0 or xx >= W:
                    continue
                q = yy * W + xx
            if not pos[q]:
                continue
            if not (bits[n][i] or bits[n if mutant == 'opp_n' else (n + 4) & 7][q]):
                continue
            ra, rb = find(i), find(q)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(i) if pos[i] else -1 for i in range(HW)])
    return raster_labels(np.where(pos, roots + 1, 0).reshape(H, W))


def component_stats(labels, out1):
    """-> (count, min x, min y, max x, max y) int64 [n,5], score sums float64 [n] (scores are positive: also sum|score|) of one image."""
    labels = np.asarray(labels)
    n = int(labels.max())
    score = sigmoid64(np.asarray(out1[1], np.float64) - np.asarray(out1[0], np.float64))
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs] - 1
    box = np.zeros((n, 5), np.int64)
    box[:, 0] = np.bincount(lab, minlength=n)
    box[:, 1], box[:, 2] = 10 ** 9, 10 ** 9
    box[:, 3], box[:, 4] = -1, -1
    np.minimum.at(box[:, 1], lab, xs)
    np.minimum.at(box[:, 2], lab, ys)
    np.maximum.at(box[:, 3], lab, xs)
    np.maximum.at(box[:, 4], lab, ys)
    ssum = np.bincount(lab, weights=score[ys, xs], minlength=n)
    return box, ssum


# ------------------------------------------------------------------------------------------------------------------------------------------
# cascade and final rows
# ------------------------------------------------------------------------------------------------------------------------------------------
INTERP_SHAPES = [(3, 5, 7, 4), (1, 1, 4, 6), (5, 1, 5, 3), (4, 6, 1, 1), (2, 2, 1, 5), (19, 10, 38, 19), (7, 4, 3, 5), (3, 5, 3, 5)]
INTERP_C = (1, 18, 20)
INTERP = [(s, C) for s in INTERP_SHAPES for C in INTERP_C]
INTERP_B = 2
INTERP_BWD_FORMS = ('both', 'dout_null', 'dout2_null')


def interp_id(r):
    (Hs, Ws, Hd, Wd), C = r
    return f'{Hs}x{Ws}->{Hd}x{Wd} C{C}'


def interp_inputs(r):
    """NHWC float32: src, addend, dout (zero on every other pixel: the g == 0 skip when dout2 is NULL), dout2, and the non-zero pre-fills of
    d(src) and d(addend)."""
    (Hs, Ws, Hd, Wd), C = r
    rng = np.random.default_rng(1000 + Hs * 131 + Ws * 17 + Hd * 7 + Wd + 1000 * C)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    dout = f(INTERP_B, Hd, Wd, C)
    dout.reshape(INTERP_B, Hd * Wd, C)[:, 0::2] = 0
    return dict(src=f(INTERP_B, Hs, Ws, C), addend=f(INTERP_B, Hd, Wd, C), dout=dout, dout2=f(INTERP_B, Hd, Wd, C),
                dsrc0=f(INTERP_B, Hs, Ws, C), dadd0=f(INTERP_B, Hd, Wd, C))


def interp_weights(n_in, n_out, mutant=None, n_scale=None):
    """Row-stochastic [n_out, n_in] matrix of align_corners=True bilinear interpolation along one axis (float64).  mutant 'scale_in_out': the
    scale in / out; n_scale: the extent the scale is taken from (the other axis's, for the swapped-H/W mistake)."""
    n_scale = n_in if n_scale is None else n_scale
    if mutant == 'scale_in_out':
        scale = n_scale / n_out
    else:
        scale = (n_scale - 1) / (n_out - 1) if n_out > 1 else 0.0
    M = np.zeros((n_out, n_in))
    for o in range(n_out):
        s = scale * o
        i0 = min(int(s), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        l1 = s - i0
        M[o, i0] += 1.0 - l1
        M[o, i1] += l1
    return M


def interp64(src, Hd, Wd, mutant=None, dtype=np.float64):
    """out[b, y, x, c] = sum My[y, i] Mx[x, j] src[b, i, j, c].  mutant 'swap_hw': the row scale taken from Ws and the column scale from Hs."""
    src = np.asarray(src, dtype)
    _, Hs, Ws, _ = src.shape
    swap = mutant == 'swap_hw'
    My = interp_weights(Hs, Hd, mutant, Ws if swap else None)
    Mx = interp_weights(Ws, Wd, mutant, Hs if swap else None)
    return np.einsum('yi,xj,bijc->byxc', My.astype(dtype), Mx.astype(dtype), src)


def interp_bwd64(g, Hs, Ws, dtype=np.float64):
    g = np.asarray(g, dtype)
    _, Hd, Wd, _ = g.shape
    My, Mx = interp_weights(Hs, Hd).astype(dtype), interp_weights(Ws, Wd).astype(dtype)
    return np.einsum('yi,xj,byxc->bijc', My, Mx, g)


FINAL_SIZES = [(1, 1), (1, 127), (1, 128), (1, 129), (5, 50), (3, 257)]
FINAL = [(fam, nf, B, HW) for fam, top in (('final', 4), ('final5', 5)) for nf in range(1, top + 1) for B, HW in FINAL_SIZES]
FINAL_LD = (18, 20)


def final_id(r):
    return f'{r[0]} nf{r[1]} B{r[2]} HW{r[3]}'


def final_masks(nf):
    return [0, (1 << nf) - 1] + [1 << k for k in range(nf)]


def final_inputs(r):
    fam, nf, B, HW = r
    rng = np.random.default_rng(2000 + (fam == 'final5') * 500 + nf * 50 + B * 7 + HW)
    f = lambda *s: rng.normal(0, 1, s).astype(np.float32)
    return dict(feats=[f(B, HW, 18) for _ in range(nf)], w1=f(2, 2 * nf), b1=f(2), w2=f(16, 16 * nf), b2=f(16), d1=f(B, 2, HW), d2=f(B, 16, HW),
                g0=[f(B, HW, 18) for _ in range(nf)], dw1_0=rng.normal(0, 1, 4 * nf + 2), dw2_0=rng.normal(0, 1, 256 * nf + 16))


def final64(inp, acc_mask, mutant=None):
    """-> dict(out1 [B,2,HW], out2 [B,16,HW], g [nf][B,HW,18] (added to the pre-fill where bit k of acc_mask is set), dw1, dw2 (weights then
    bias, added to the pre-fill)) in float64.  mutant 'ignore_acc': the mask taken as 0."""
    c = lambda a: np.asarray(a, np.float64)
    nf = len(inp['feats'])
    x1 = np.concatenate([c(f)[..., :2] for f in inp['feats']], -1)        # [B,HW,2nf]
    x2 = np.concatenate([c(f)[..., 2:] for f in inp['feats']], -1)        # [B,HW,16nf]
    out1 = np.einsum('oc,bpc->bop', c(inp['w1']), x1) + c(inp['b1'])[None, :, None]
    out2 = np.einsum('oc,bpc->bop', c(inp['w2']), x2) + c(inp['b2'])[None, :, None]
    gx1 = np.einsum('oc,bop->bpc', c(inp['w1']), c(inp['d1']))
    gx2 = np.einsum('oc,bop->bpc', c(inp['w2']), c(inp['d2']))
    g = []
    for k in range(nf):
        v = np.concatenate([gx1[..., 2 * k:2 * k + 2], gx2[..., 16 * k:16 * k + 16]], -1)
        acc = (acc_mask >> k) & 1 and mutant != 'ignore_acc'
        g.append((c(inp['g0'][k]) + v) if acc else v)
    dw1 = np.concatenate([np.einsum('bop,bpc->oc', c(inp['d1']), x1).ravel(), c(inp['d1']).sum((0, 2))])
    dw2 = np.concatenate([np.einsum('bop,bpc->oc', c(inp['d2']), x2).ravel(), c(inp['d2']).sum((0, 2))])
    return dict(out1=out1, out2=out2, g=g, dw1=inp['dw1_0'] + dw1, dw2=inp['dw2_0'] + dw2)


def _fma32(a, b, c):
    """fp32 fma(a, b, c): the product of two fp32 numbers is exact in float64"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def final32(inp, acc_mask):
    """The same statement in float32 the way a thread of the kernels walks it -- the e_cpu32 of the gates: forward = one fma chain from the bias
    over (k, c); d(features) = an fma chain from 0 over o, then one add to the pre-fill; weight gradients = fp32 fma chains over the pixels of a
    128-pixel pass (the passes run over the flat B * HW index), the passes and the pre-fill summed in float64."""
    f32 = np.float32
    feats = [np.asarray(f, f32) for f in inp['feats']]
    nf = len(feats)
    B, HW, _ = feats[0].shape
    w, bias, d = (inp['w1'], inp['w2']), (inp['b1'], inp['b2']), (inp['d1'], inp['d2'])
    outs, gparts = [], []
    for j, (n, off) in enumerate(((2, 0), (16, 2))):
        out = np.empty((B, n, HW), f32)
        for o in range(n):
            a = np.full((B, HW), bias[j][o], f32)
            for k in range(nf):
                for c in range(n):
                    a = _fma32(w[j][o, k * n + c], feats[k][..., off + c], a)
            out[:, o] = a
        outs.append(out)
        gx = np.zeros((B, HW, n * nf), f32)
        for o in range(n):
            gx = _fma32(w[j][o][None, None, :], d[j][:, o, :, None], gx)
        gparts.append(gx)
    g = []
    for k in range(nf):
        v = np.concatenate([gparts[0][..., 2 * k:2 * k + 2], gparts[1][..., 16 * k:16 * k + 16]], -1)
        g.append((np.asarray(inp['g0'][k], f32) + v) if (acc_mask >> k) & 1 else v)
    P = B * HW
    dws = []
    for j, (n, off) in enumerate(((2, 0), (16, 2))):
        x = np.concatenate([f[..., off:off + n] for f in feats], -1).reshape(P, n * nf)
        df = np.asarray(d[j], f32).transpose(0, 2, 1).reshape(P, n)
        tot_w, tot_b = np.zeros((n, n * nf)), np.zeros(n)
        for base in range(0, P, TP):
            aw, ab = np.zeros((n, n * nf), f32), np.zeros(n, f32)
            for q in range(base, min(base + TP, P)):
                aw = _fma32(df[q][:, None], x[q][None, :], aw)
                ab = ab + df[q]
            tot_w += aw
            tot_b += ab
        dws.append(np.concatenate([tot_w.ravel(), tot_b]))
    return dict(out1=outs[0], out2=outs[1], g=g, dw1=inp['dw1_0'] + dws[0], dw2=inp['dw2_0'] + dws[1])


def relerr(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


# Gates e <= GATE * e_cpu32 + FLOOR (e = relerr against float64, e_cpu32 = the same figure of the float32 restatement on the CPU): twice the
# worst e / e_cpu32 per entry family over three MI355X runs of tests/test_gpu_pixellink_tail.py (figures in its docstring): 3.82 for the
# atomics of gssd_interp_add_bwd_f32 (against a float32 einsum), 1.00 for the final kernels (against final32, which walks the kernel's order).
FLOOR = 1e-7
GATES = {'interp_bwd': 7.64, 'final_fwd': 2.0, 'final_dfeat': 2.0, 'final_wgrad': 2.0}
# what tests/test_gpu_pixellink2s.py::test_final5_kernels and tests/test_gpu_pixellink.py::test_interp_add_backward allow
EXISTING_BOUND = {'interp_bwd': 2e-6, 'final_fwd': 1e-6, 'final_dfeat': 1e-6, 'final_wgrad': 1e-5}


def bound(family, e_cpu32):
    return GATES[family] * e_cpu32 + FLOOR
