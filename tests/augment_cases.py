"""The cases of tests/golden/augment.npz (tests/golden/make_golden_augment.py) for the augmentation tests."""
import hashlib
import os
import random

import numpy as np

from gssd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment.npz')
BIG_B, BIG_SEED = 32, 4242
BOX1 = [[0.30, 0.35, 0.55, 0.60, 1.]]
BOX3 = [[0.10, 0.12, 0.30, 0.28, 1.], [0.45, 0.40, 0.70, 0.75, 1.], [0.78, 0.70, 0.92, 0.90, 1.]]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def load():
    return np.load(GOLDEN, allow_pickle=False)


class Case:
    def __init__(self, g, name):
        pre = name + '__'
        H, W, size, p_only, in_seed, seed = (int(v) for v in g[pre + 'cfg'])
        self.name, self.H, self.W, self.size, self.p_only, self.seed = name, H, W, size, bool(p_only), seed
        self.pixeljitter = float(g[pre + 'pixeljitter'])
        self.mean = g[pre + 'mean']
        self.boxes, self.target, self.next = g[pre + 'boxes'], g[pre + 'target'], g[pre + 'next']
        self.branches = dict(zip([str(k) for k in g['branch_keys']], (int(v) for v in g[pre + 'branches'])))
        if pre + 'in' in g.files:
            self.img, self.out, self.out_sha = g[pre + 'in'], g[pre + 'out'], None
        else:
            self.img = synth.synth_study_u8(in_seed, 4, max(H, W))[:, :H, :W].copy()
            assert sha(self.img) == bytes(g[pre + 'in_sha']).hex()
            self.out, self.out_sha = None, bytes(g[pre + 'out_sha']).hex()
            self.sample_idx, self.sample = g[pre + 'sample_idx'], g[pre + 'sample']

    def aug(self):
        from gssd.augment import DeviceSSDAugmentation
        return DeviceSSDAugmentation(self.pixeljitter, 1.5, self.size, tuple(float(v) for v in self.mean), use_normalize=True,
                                     p_only=self.p_only)

    def rngs(self):
        return random.Random(self.seed), np.random.RandomState(self.seed)

    def check_k(self, k):
        """k: uint8 [4, size, size, 3] (the reference's layout)."""
        if self.out is not None:
            return np.array_equal(k, self.out)
        return sha(k) == self.out_sha


def cases(g):
    return [Case(g, str(n)) for n in g['names']]


def big_inputs():
    studies = [synth.synth_study_u8(900 + i, 4, 512) for i in range(4)]
    targets = [np.array(BOX3 if i % 2 else BOX1, np.float32) for i in range(BIG_B)]
    return studies, targets


def next_draws(py, npr):
    return np.array([py.random(), npr.random_sample()], np.float64)
