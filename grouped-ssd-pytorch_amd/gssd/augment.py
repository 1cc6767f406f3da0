"""Device ``SSDAugmentation`` (utils/augmentations.py:548-589): the training transform of the 4-phase studies on the MI355X.

The reference runs a numpy / Pillow chain per study in DataLoader workers: ConvertFromInts, ToAbsoluteCoords, PixelJitter,
PhotometricDistort, Expand, RandomSampleCrop, RandomMirror, ToPercentCoords, SubtractMeans, [POnly], Normalize, ResizeFast.
Here the split is:

* the host PLANNER (``plan``) draws every random number in the reference's order from the same generators and does the box
  arithmetic with the reference's numpy dtypes; the pixels it never touches.  Per study it emits one ``gssd_aug_desc``
  (include/gssd_hip.h): source geometry and strides, Expand's canvas placement, the crop window, the mirror flag, brightness /
  contrast as float32, and offsets into the resampling coefficient tables;
* three HIP launches (csrc/augment.hip) per batch: extrema, quantise + horizontal Pillow pass, vertical pass + ``/ 255``;
* with ``use_pixel_link`` and a named ``pixel_link_version``, a fourth (csrc/pixellink_targets.hip) builds the PixelLink targets of
  ``PreparePixelLinkTargets`` (utils/augmentations.py:527-545) from the planned boxes; their corners ride in the descriptors'
  pinned upload.  That transform draws no random numbers, so the generators are consumed exactly as without it.

Random generators (the reference's trap): in augmentations.py the name ``random`` is Python's stdlib module (re-exported by
``from pixel_link.pixellink_data import *`` over ``from numpy import random``), so ``randint(0, 2)`` is inclusive -- a branch
fires with p = 2/3 -- and ``uniform`` / ``choice`` are stdlib; only PixelJitter draws from ``numpy.random``.  ``py_rng`` /
``np_rng`` replace the two global generators; a batch of B studies consumes them exactly as B consecutive reference calls.
"""
import random as _stdlib_random

import numpy as np
import torch

from . import _lib
from ._lib import lib, check
from .input_stage import resample_tables
from . import pixellink_targets as _plt

PHASES, SLICES = 4, 3

DESC_DTYPE = np.dtype([
    ('src', np.int64), ('work', np.int64), ('H', np.int32), ('W', np.int32),
    ('s_phase', np.int32), ('s_chan', np.int32), ('s_y', np.int32), ('s_x', np.int32),
    ('top', np.int32), ('left', np.int32), ('cy', np.int32), ('cx', np.int32), ('ch', np.int32), ('cw', np.int32),
    ('mirror', np.int32), ('fill', np.int32), ('delta', np.float32), ('alpha', np.float32),
    ('hb', np.int32), ('hk', np.int32), ('hks', np.int32), ('vb', np.int32), ('vk', np.int32), ('vks', np.int32),
    ('row0', np.int32), ('nrows', np.int32)])

# RandomSampleCrop's modes: only their count (stdlib choice draws an index) and which one is None matter -- with max_iou always
# inf its IoU rejection never fires, but every draw is still made
CROP_MODES = (None, (0.1, None), (0.3, None), (0.7, None), (0.9, None), (None, None))


class SamplePlan:
    """What the planner decided for one study (geometry in pixels; ``target`` is the reference's float32 ``[n, 5]``)."""
    __slots__ = ('H', 'W', 'brightness', 'delta', 'contrast', 'alpha', 'jitter_fallback', 'canvas', 'place', 'mode', 'rect',
                 'mirror', 'target')

    def branches(self):
        """The branch record the golden generator keeps for the reference (tests/golden/make_golden_augment.py)."""
        return dict(brightness=int(self.brightness), contrast=int(self.contrast), mirror=int(self.mirror), mode=int(self.mode),
                    jitter_fallback=int(self.jitter_fallback), crop_h=int(self.rect[3] - self.rect[1]),
                    crop_w=int(self.rect[2] - self.rect[0]))


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def plan_sample(H, W, target, pixeljitter, ratio, py, npr):
    """One reference call's random draws and box arithmetic for a ``[4, H, W, 3]`` study with ``target`` ``[n, 5]`` (percent
    coordinates + label).  ``py``: stdlib ``random`` (module or ``random.Random``); ``npr``: ``numpy.random`` or a RandomState."""
    t = np.array(target, dtype=np.float32).reshape(-1, 5)
    boxes, labels = t[:, :4].copy(), t[:, 4].copy()
    p = SamplePlan()
    p.H, p.W = int(H), int(W)
    # ToAbsoluteCoords: float32 * float32(size)
    wh = np.array([W, H, W, H], np.float32)
    boxes = _f32(boxes * wh)
    # PixelJitter: float64 noise scaled by the size, truncated to int8, added in float32; an inverted box keeps the original boxes
    noise = npr.uniform(-pixeljitter, pixeljitter, size=boxes.shape)
    noise = noise * np.array([W, H, W, H], np.float64)
    noise = noise.astype(np.int8).astype(np.float32)
    jittered = _f32(boxes + noise)
    ok = bool(np.all(jittered[:, 0] < jittered[:, 2]) and np.all(jittered[:, 1] < jittered[:, 3]))
    p.jitter_fallback = not ok
    if ok:
        boxes = jittered
    # PhotometricDistort: brightness, then a draw that picks one of two identical contrasts, then that contrast
    p.brightness = bool(py.randint(0, 2))
    p.delta = np.float32(py.uniform(-32, 32)) if p.brightness else np.float32(0.)
    py.randint(0, 2)
    p.contrast = bool(py.randint(0, 2))
    p.alpha = np.float32(py.uniform(0.5, 1.5)) if p.contrast else np.float32(1.)
    # Expand: canvas [int(H r), int(W r)] filled with the mean, the study at (int(top), int(left)); boxes shift (float64, rounded)
    r = py.uniform(1, ratio)
    left = py.uniform(0, W * r - W)
    top = py.uniform(0, H * r - H)
    ch, cw = int(H * r), int(W * r)
    it, il = int(top), int(left)
    p.canvas, p.place = (ch, cw), (it, il)
    boxes = (boxes.astype(np.float64) + np.array([il, it, il, it], np.float64)).astype(np.float32)
    # RandomSampleCrop (depends on geometry and boxes only)
    rect = None
    while rect is None:
        p.mode = py.choice(range(len(CROP_MODES)))                         # choice(seq) draws _randbelow(len(seq))
        if CROP_MODES[p.mode] is None:
            rect = (0, 0, cw, ch)
            break
        for _ in range(50):
            w = py.uniform(0.3 * cw, cw)
            h = py.uniform(0.3 * ch, ch)
            if h / w < 0.5 or h / w > 2:
                continue
            l_ = py.uniform(0, cw - w)
            t_ = py.uniform(0, ch - h)
            rc = (int(l_), int(t_), int(l_ + w), int(t_ + h))
            if boxes.shape[0] == 0:
                raise ValueError('RandomSampleCrop needs at least one box (the reference fails on an empty overlap)')
            centers = _f32((boxes[:, :2] + boxes[:, 2:]) / np.float32(2.0))
            mask = (rc[0] < centers[:, 0]) & (rc[1] < centers[:, 1]) & (rc[2] > centers[:, 0]) & (rc[3] > centers[:, 1])
            if not mask.any():
                continue
            b = boxes[mask].astype(np.float64)
            labels = labels[mask]
            lt = np.array(rc[:2], np.float64)
            b[:, :2] = np.maximum(b[:, :2], lt)
            b[:, :2] = (b[:, :2] - lt).astype(np.float32)
            b[:, 2:] = np.minimum(b[:, 2:], np.array(rc[2:], np.float64))
            b[:, 2:] = (b[:, 2:] - lt).astype(np.float32)
            boxes = b.astype(np.float32)
            rect = (rc[0], rc[1], min(rc[2], cw), min(rc[3], ch))
            break
    p.rect = rect
    wc, hc = rect[2] - rect[0], rect[3] - rect[1]
    # RandomMirror: x' = width - x (float32), the two x columns swapped
    p.mirror = bool(py.randint(0, 2))
    if p.mirror:
        boxes = boxes.copy()
        x0, x2 = boxes[:, 0].copy(), boxes[:, 2].copy()
        boxes[:, 0] = np.float32(wc) - x2
        boxes[:, 2] = np.float32(wc) - x0
    # ToPercentCoords: float32 / float32(size)
    boxes = _f32(boxes / np.array([wc, hc, wc, hc], np.float32))
    p.target = np.hstack((boxes, labels[:, None])).astype(np.float32)
    return p


class Plan:
    """A batch's plans: per-study ``SamplePlan``s in batch order (``Plan.cat`` joins plans made from different generators)."""

    def __init__(self, samples):
        self.samples = list(samples)

    @staticmethod
    def cat(plans):
        return Plan([s for p in plans for s in p.samples])

    @property
    def targets(self):
        return [s.target for s in self.samples]


def _as_studies(raw):
    """``raw``: a uint8 CUDA tensor ``[B, 4, H, W, 3]`` or ``[B, 4, 3, H, W]`` (the reference collate's layout), or a list of
    per-study ``[4, H, W, 3]`` / ``[4, 3, H, W]`` tensors.  Returns [(tensor, H, W, strides in bytes (phase, slice, y, x))]."""
    items = list(raw) if isinstance(raw, (list, tuple)) else None
    if items is None:
        if not isinstance(raw, torch.Tensor) or raw.dim() != 5:
            raise _lib.GssdError(f'augment: raw must be a uint8 CUDA tensor [B, 4, H, W, 3] or [B, 4, 3, H, W], or a list of studies, '
                                 f'got {type(raw).__name__} {tuple(getattr(raw, "shape", ()))}')
        items = [raw[b] for b in range(raw.shape[0])]
    out = []
    for t in items:
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise _lib.GssdError('augment: raw studies must be uint8 tensors on the MI355X (no CPU fallback)')
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[0] != PHASES or SLICES not in (t.shape[3], t.shape[1]):
            raise _lib.GssdError(f'augment: expected uint8 [4, H, W, 3] or [4, 3, H, W] studies, got {t.dtype} {tuple(t.shape)}')
        sp, a, b_, c = t.stride()
        if t.shape[3] == SLICES:
            H, W, st = t.shape[1], t.shape[2], (sp, c, a, b_)
        else:
            H, W, st = t.shape[2], t.shape[3], (sp, a, b_, c)
        if min(st) < 0 or max(st) * max(H, W, PHASES) >= 2 ** 31:
            raise _lib.GssdError(f'augment: unsupported strides {t.stride()}')
        out.append((t, int(H), int(W), tuple(int(v) for v in st)))
    if not out:
        raise _lib.GssdError('augment: empty batch')
    if len({x[0].device for x in out}) != 1:
        raise _lib.GssdError('augment: all studies must be on one device')
    return out


class _Tables:
    """Coefficient tables for every input size 1..cap -> ``size`` in one device int32 array: offsets[n] = (bounds, kk, ksize)."""

    def __init__(self, size, cap, dev):
        offs, parts, pos = {}, [], 0
        for n in range(1, cap + 1):
            if n == size:
                continue
            b, k = resample_tables(n, size)
            offs[n] = (pos, pos + b.size, k.shape[1])
            parts += [b.reshape(-1), k.reshape(-1)]
            pos += b.size + k.size
        host = np.concatenate(parts) if parts else np.zeros(1, np.int32)
        self.cap, self.offsets, self.host = cap, offs, host
        self.dev = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True) if torch.device(dev).type == 'cuda' else None


class DeviceSSDAugmentation:
    """``SSDAugmentation`` (utils/augmentations.py:548-589) with its constructor arguments and asserts, on the MI355X.

    ``aug(raw, targets)`` -> (fp32 CUDA ``[B, 12, size, size]``, list of ``torch.float32 [n_i, 5]``): ``raw`` as the reference's
    dataset returns it with an identity transform and collates it (uint8 ``[B, 4, 3, H, W]``, or ``[B, 4, H, W, 3]``, or a list of
    studies), ``targets`` pull_item's ``[n_i, 5]`` percent-coordinate arrays.  Bitwise equal to B consecutive reference calls
    from the same generator states.  No host synchronisation: descriptors reach the device through a pinned staging buffer.

    ``use_pixel_link=True, pixel_link_version="4s" | "2s"`` (train_lesion_multiphase_v2_pixellink.py:513-518): ``aug(raw, targets)``
    -> (images, the dict of ``detection_collate_v2_pixel_link`` (data/data_custom_v2.py:399-434)) -- the same images, and the
    PixelLink targets of the planned boxes (gssd/pixellink_targets.py): the four maps on the device, ``'lables'`` / ``'boxes'`` as
    CPU float32 tensors.  The reference's constructor defaults the version to "2s"; here it must be named."""

    def __init__(self, pixeljitter=0.01, ratio=1.5, size=300, mean=(104, 117, 123), use_normalize=False, p_only=False,
                 use_pixel_link=False, pixel_link_version=None):
        assert use_normalize, 'new ResizeFast implementation assumes --use_normalize to True!'      # the reference's assert
        if use_pixel_link and pixel_link_version is None:
            raise NotImplementedError('use_pixel_link (PreparePixelLinkTargets) needs a named version: pass pixel_link_version="4s" '
                                      'or "2s", as the reference driver does (config.version)')
        self.pixeljitter, self.ratio, self.size = pixeljitter, ratio, int(size)
        self.use_normalize, self.p_only, self.use_pixel_link = True, bool(p_only), bool(use_pixel_link)
        self.pixel_link_version = None
        if self.use_pixel_link:
            _plt._check_geometry(self.size, pixel_link_version)
            self.pixel_link_version = pixel_link_version
        m = np.asarray(mean, np.float32).reshape(-1)
        if m.size != SLICES:
            raise ValueError(f'mean must have {SLICES} values, got {m.size}')
        self.mean = m
        self._tables, self._retired = {}, []
        self.last_minmax = None

    def plan(self, sizes, targets, py_rng=None, np_rng=None):
        """Host half only: ``sizes`` [(H, W)] per study; draws from ``py_rng`` / ``np_rng`` (default: the global generators)."""
        py = py_rng if py_rng is not None else _stdlib_random
        npr = np_rng if np_rng is not None else np.random
        if len(sizes) != len(targets):
            raise _lib.GssdError(f'augment: {len(sizes)} studies but {len(targets)} targets')
        return Plan([plan_sample(H, W, np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.float32),
                                 self.pixeljitter, self.ratio, py, npr) for (H, W), t in zip(sizes, targets)])

    def _table(self, cap, dev):
        t = self._tables.get(dev)
        if t is None or t.cap < cap:
            if t is not None:
                self._retired.append(t)                    # launches already queued may still read it: never freed under them
            t = self._tables[dev] = _Tables(self.size, cap, dev)
        return t

    def descriptors(self, studies, plan, table, base=0):
        """The ``gssd_aug_desc`` array of a plan (``studies`` from ``_as_studies``; ``base`` = 0 gives offsets only)."""
        S = self.size
        d = np.zeros(len(plan.samples), DESC_DTYPE)
        work = 0
        for i, ((t, H, W, st), p) in enumerate(zip(studies, plan.samples)):
            if (H, W) != (p.H, p.W):
                raise _lib.GssdError(f'augment: study {i} is {H}x{W} but was planned as {p.H}x{p.W}')
            x0, y0, x1, y1 = p.rect
            ch, cw = y1 - y0, x1 - x0
            e = d[i]
            e['src'] = t.data_ptr() if base else 0
            e['H'], e['W'] = H, W
            e['s_phase'], e['s_chan'], e['s_y'], e['s_x'] = st
            e['top'], e['left'] = p.place
            e['cy'], e['cx'], e['ch'], e['cw'] = y0, x0, ch, cw
            e['mirror'] = int(p.mirror)
            e['fill'] = int(y0 < p.place[0] or x0 < p.place[1] or y1 > p.place[0] + H or x1 > p.place[1] + W)
            e['delta'], e['alpha'] = p.delta, p.alpha
            if cw != S:
                e['hb'], e['hk'], e['hks'] = table.offsets[cw]
            if ch != S:
                vb, vk, vks = table.offsets[ch]
                e['vb'], e['vk'], e['vks'] = vb, vk, vks
                bounds = table.host[vb:vb + 2 * S].reshape(S, 2)
                row0 = int(bounds[:, 0].min())
                e['row0'], e['nrows'] = row0, int((bounds[:, 0] + bounds[:, 1]).max()) - row0
            else:
                e['row0'], e['nrows'] = 0, S
            e['work'] = work
            work += (1 if self.p_only else PHASES) * int(e['nrows']) * S * SLICES
        return d, work

    def __call__(self, raw, targets, out=None, py_rng=None, np_rng=None):
        studies = _as_studies(raw)
        plan = self.plan([(H, W) for _, H, W, _ in studies], targets, py_rng, np_rng)
        if self.use_pixel_link:
            return self.run(studies, plan, out, pixel_link=True)
        images = self.run(studies, plan, out)
        return images, [torch.from_numpy(t) for t in plan.targets]

    def run(self, raw, plan, out=None, pixel_link=False):
        """Device half: the three passes for ``plan`` over ``raw`` (as in ``__call__``, or ``_as_studies``'s list).  With
        ``pixel_link`` (needs ``pixel_link_version``): (images, PixelLink target dict) from the plan's boxes."""
        studies = raw if isinstance(raw, list) and raw and isinstance(raw[0], tuple) else _as_studies(raw)
        if len(studies) != len(plan.samples):
            raise _lib.GssdError(f'augment: {len(studies)} studies but a plan for {len(plan.samples)}')
        dev, S, B = studies[0][0].device, self.size, len(studies)
        cap = max(max(p.canvas) for p in plan.samples)
        table = self._table(cap, dev)
        d, work_bytes = self.descriptors(studies, plan, table, base=1)
        max_rows = int(d['nrows'].max())
        max_cw = int(d['cw'].max())
        if out is None:
            out = torch.empty(B, PHASES * SLICES, S, S, dtype=torch.float32, device=dev)
        elif (out.dtype != torch.float32 or not out.is_cuda or tuple(out.shape) != (B, PHASES * SLICES, S, S)
              or not out.is_contiguous() or out.device != dev):
            raise _lib.GssdError(f'augment: out must be a contiguous fp32 CUDA tensor [{B}, 12, {S}, {S}]')
        staged = d.view(np.uint8)
        if pixel_link:
            if self.pixel_link_version is None:
                raise _lib.GssdError('augment: pixel_link targets need pixel_link_version')
            packed, offs = _plt.pack_boxes([t[:, :4] for t in plan.targets])
            tail, boxes_at = _plt.staging(packed, offs)
            desc_bytes = (staged.size + 15) & ~15
            staged = np.concatenate([staged, np.zeros(desc_bytes - staged.size, np.uint8), tail])
        desc = torch.from_numpy(staged).pin_memory().to(dev, non_blocking=True)
        work = torch.empty(max(work_bytes, 1), dtype=torch.uint8, device=dev)
        mm = torch.empty(B, SLICES, 2, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        m0, m1, m2 = (float(v) for v in self.mean)
        with torch.cuda.device(dev):
            check(lib.gssd_augment_minmax(desc.data_ptr(), B, int(d['ch'].max()), int(self.p_only), mm.data_ptr(), stream))
            check(lib.gssd_augment_horizontal(desc.data_ptr(), mm.data_ptr(), table.dev.data_ptr(), m0, m1, m2, work.data_ptr(), B,
                                              max_rows, max_cw, S, int(self.p_only), stream))
            check(lib.gssd_augment_vertical(desc.data_ptr(), table.dev.data_ptr(), work.data_ptr(), out.data_ptr(), B, S,
                                            int(self.p_only), stream))
        self.last_minmax, self.last_desc = mm, d
        if not pixel_link:
            return out
        base = desc.data_ptr() + desc_bytes
        targets = _plt.launch(base + boxes_at, base, B, S, self.pixel_link_version, dev)
        targets['lables'] = [torch.from_numpy(t[:, 4].copy()) for t in plan.targets]
        targets['boxes'] = [torch.from_numpy(t) for t in plan.targets]
        return out, targets

    def check_not_flat(self):
        """The reference's Normalize asserts ``img_min != img_max``; on the device that costs a sync, so it is opt-in."""
        mm = self.last_minmax.cpu().numpy()
        for b, e in enumerate(self.last_desc):
            lo, hi = [], []
            Hs, Ws = e['H'], e['W']
            inside = (max(e['cy'], e['top']) < min(e['cy'] + e['ch'], e['top'] + Hs)
                      and max(e['cx'], e['left']) < min(e['cx'] + e['cw'], e['left'] + Ws))
            if inside:
                for c in range(SLICES):
                    f = lambda u: (np.float32(np.float32(u) + e['delta']) * e['alpha']).astype(np.float32) - self.mean[c]  # noqa: E731
                    lo.append(f(255 - mm[b, c, 0]))
                    hi.append(f(mm[b, c, 1]))
            if e['fill']:
                lo.append(np.float32(0))
                hi.append(np.float32(0))
            assert min(lo) != max(hi), 'all-black image detected during Normalizing. check preprocessing'
