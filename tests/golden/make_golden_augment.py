"""Golden vectors for the device SSDAugmentation: the reference's ``SSDAugmentation`` (utils/augmentations.py:548-589, which calls
numpy and Pillow) run here on seeded ``synth_study_u8`` studies, both generators seeded per case.

For every case the fixture keeps the input (in full, or its synth seed + sha256 for the large ones), the seed, the output as
exact uint8 k-planes (``out == fl32(k / 255)``; sha256 + samples for the large ones), the targets, the next draw of each
generator after the call, and which branches the reference took (recorded by wrapping its classes), so the tests can assert
coverage.  Each case searches seeds until the reference takes the branches the case is for.

    python tests/golden/make_golden_augment.py     # rewrites tests/golden/augment.npz  (build container only)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference, sha, sample_idx, synth      # noqa: E402

# name, source size (H, W), output size, pixeljitter, mean, p_only, boxes (percent + label), required branches.  The size-37
# cases other than p_only share size and mean, so the GPU test can run them as one batch with mixed geometry.
BOX1 = [[0.30, 0.35, 0.55, 0.60, 1.]]
BOX3 = [[0.10, 0.12, 0.30, 0.28, 1.], [0.45, 0.40, 0.70, 0.75, 1.], [0.78, 0.70, 0.92, 0.90, 1.]]
THIN = [[0.40, 0.30, 0.42, 0.70, 1.]]                   # 1 px wide at 48: jitter of 0.05 * 48 px can invert it
CASES = [
    ('mode0', (48, 48), 37, 0.01, (104, 117, 123), False, BOX1, dict(mode=0, mirror=1, brightness=1, contrast=1)),
    ('mode1', (48, 48), 37, 0.01, (104, 117, 123), False, BOX3, dict(mode=1, mirror=0, brightness=0, contrast=1)),
    ('mode2', (48, 48), 37, 0.01, (104, 117, 123), False, BOX1, dict(mode=2, mirror=1, brightness=1, contrast=0)),
    ('mode3', (48, 48), 37, 0.01, (104, 117, 123), False, BOX3, dict(mode=3, mirror=0, brightness=0, contrast=0)),
    ('mode4_up', (48, 48), 37, 0.01, (104, 117, 123), False, BOX1, dict(mode=4, upsample=1)),
    ('mode5_drop', (48, 48), 37, 0.01, (104, 117, 123), False, BOX3, dict(mode=5, dropped=1)),
    ('jitter_fallback', (48, 48), 37, 0.05, (104, 117, 123), False, THIN, dict(jitter_fallback=1)),
    ('nonsquare', (40, 48), 37, 0.01, (104, 117, 123), False, BOX3, dict(mirror=1)),
    ('p_only', (48, 48), 37, 0.01, (49, 49, 49), True, BOX1, dict(brightness=1)),
    ('src96', (96, 96), 300, 0.01, (49, 49, 49), False, BOX1, dict(mirror=1)),
]
FULL = ('src96',)                                       # stored as sha256 + samples (the input regenerated from its seed)
BIG_B, BIG_SEED = 32, 4242


class Recorder:
    """Stands in for the reference module's ``random`` (stdlib) and logs each draw under the class that made it."""

    def __init__(self, rng):
        self.rng, self.ctx, self.log = rng, None, []

    def __getattr__(self, name):
        f = getattr(self.rng, name)

        def call(*a, **k):
            r = f(*a, **k)
            self.log.append((self.ctx, name, r))
            return r
        return call


def instrument(A, rec):
    """Wrap the reference's transform classes so the recorder knows which one draws; PixelJitter's fallback is seen directly."""
    state = {}
    for cls in (A.RandomBrightness, A.RandomContrast, A.RandomSampleCrop, A.RandomMirror, A.Expand, A.PixelJitter, A.ResizeFast):
        orig = cls.__dict__.get('_orig_call') or cls.__call__
        cls._orig_call = orig

        def wrapped(self, image, boxes=None, labels=None, _orig=orig, _name=cls.__name__):
            prev, rec.ctx = rec.ctx, _name
            try:
                out = _orig(self, image, boxes, labels)
            finally:
                rec.ctx = prev
            if _name == 'PixelJitter':
                state['jitter_fallback'] = int(out[1] is boxes)
            if _name == 'RandomSampleCrop':
                state['n_in'], state['n_out'] = len(boxes), len(out[1])
            if _name == 'ResizeFast':
                state['crop_h'], state['crop_w'] = image.shape[1], image.shape[2]
            return out
        cls.__call__ = wrapped
    return state


def branches(rec, state):
    def draws(ctx, name):
        return [r for c, n, r in rec.log if c == ctx and n == name]
    modes = (None, (0.1, None), (0.3, None), (0.7, None), (0.9, None), (None, None))
    return dict(brightness=int(bool(draws('RandomBrightness', 'randint')[0])),
                contrast=int(bool(draws('RandomContrast', 'randint')[0])),
                mirror=int(bool(draws('RandomMirror', 'randint')[0])),
                mode=modes.index(draws('RandomSampleCrop', 'choice')[-1]),
                jitter_fallback=state['jitter_fallback'], crop_h=int(state['crop_h']), crop_w=int(state['crop_w']),
                dropped=int(state['n_out'] < state['n_in']))


def main():
    import random

    import PIL
    import_reference()
    import utils.augmentations as A
    rec = Recorder(random)
    A.random = rec                                      # the module's `random` IS the stdlib module (see gssd/augment.py)
    assert A.random.rng is random
    state = instrument(A, rec)

    def run(aug, img, tgt, seed):
        random.seed(seed)
        np.random.seed(seed)
        rec.log.clear()
        t = np.array(tgt, np.float32)
        im, boxes, labels = aug(img.copy(), t[:, :4], t[:, 4])
        b = branches(rec, state)
        nxt = np.array([random.random(), np.random.random_sample()], np.float64)
        target = np.hstack((boxes, np.expand_dims(labels, 1))).astype(np.float32)
        return im, target, b, nxt

    def kplanes(im):
        k = np.rint(im.astype(np.float64) * 255).astype(np.uint8)
        assert np.array_equal((k.astype(np.float32) / np.float32(255.)), im), 'output is not k / 255'
        return k

    d = {'pillow_version': np.frombuffer(PIL.__version__.encode(), np.uint8),
         'numpy_version': np.frombuffer(np.__version__.encode(), np.uint8)}
    names = []
    for ci, (name, (H, W), size, pj, mean, p_only, boxes, want) in enumerate(CASES):
        aug = A.SSDAugmentation(pj, 1.5, size, mean, use_normalize=True, p_only=p_only)
        in_seed = 1000 + ci
        img = synth.synth_study_u8(in_seed, 4, max(H, W))[:, :H, :W].copy()
        for seed in range(20000):
            im, target, b, nxt = run(aug, img, boxes, seed)
            b['upsample'] = int(b['crop_w'] < size or b['crop_h'] < size)
            if all(b[k] == v for k, v in want.items()):
                break
        else:
            raise RuntimeError(f'no seed gives {want} for {name}')
        k = kplanes(im)
        pre = f'{name}__'
        d[pre + 'cfg'] = np.array([H, W, size, p_only, in_seed, seed], np.int64)
        d[pre + 'pixeljitter'] = np.array(pj, np.float64)
        d[pre + 'mean'] = np.array(mean, np.float32)
        d[pre + 'boxes'] = np.array(boxes, np.float32)
        d[pre + 'target'] = target
        d[pre + 'next'] = nxt
        d[pre + 'branches'] = np.array([b[k_] for k_ in BRANCH_KEYS], np.int64)
        if name in FULL:
            d[pre + 'in_sha'] = np.frombuffer(bytes.fromhex(sha(img)), np.uint8)
            d[pre + 'out_sha'] = np.frombuffer(bytes.fromhex(sha(k)), np.uint8)
            idx = sample_idx(k.size, 2048)
            d[pre + 'sample_idx'], d[pre + 'sample'] = idx, k.reshape(-1)[idx]
        else:
            d[pre + 'in'] = img
            d[pre + 'out'] = k
        names.append(name)
        print(name, 'seed', seed, b)
    # B = 32 consecutive calls from one seed on 512 x 512 studies -> 300 (the training geometry)
    aug = A.SSDAugmentation(0.01, 1.5, 300, (49, 49, 49), use_normalize=True)
    random.seed(BIG_SEED)
    np.random.seed(BIG_SEED)
    outs, targets, brs = [], [], []
    studies = [synth.synth_study_u8(900 + i, 4, 512) for i in range(4)]
    for i in range(BIG_B):
        rec.log.clear()
        t = np.array(BOX3 if i % 2 else BOX1, np.float32)
        im, boxes, labels = aug(studies[i % 4].copy(), t[:, :4], t[:, 4])
        brs.append([branches(rec, state)[k_] if k_ != 'upsample' else 0 for k_ in BRANCH_KEYS])
        outs.append(kplanes(im))
        targets.append(np.hstack((boxes, np.expand_dims(labels, 1))).astype(np.float32))
    nxt = np.array([random.random(), np.random.random_sample()], np.float64)
    k = np.stack(outs)
    d['big__out_sha'] = np.frombuffer(bytes.fromhex(sha(k)), np.uint8)
    idx = sample_idx(k.size, 4096)
    d['big__sample_idx'], d['big__sample'] = idx, k.reshape(-1)[idx]
    d['big__in_sha'] = np.frombuffer(bytes.fromhex(sha(np.stack(studies))), np.uint8)
    d['big__targets'] = np.concatenate(targets)
    d['big__counts'] = np.array([len(t) for t in targets], np.int64)
    d['big__next'] = nxt
    d['big__branches'] = np.array(brs, np.int64)
    d['names'] = np.array(names)
    d['branch_keys'] = np.array(BRANCH_KEYS)
    np.savez_compressed(os.path.join(HERE, 'augment.npz'), **d)
    print('augment.npz written; pillow', PIL.__version__, 'numpy', np.__version__, 'big sha', sha(k)[:16])


BRANCH_KEYS = ('brightness', 'contrast', 'mirror', 'mode', 'jitter_fallback', 'crop_h', 'crop_w', 'dropped', 'upsample')

if __name__ == '__main__':
    main()
