"""Device SSDAugmentation, host half (no GPU): the planner against the reference's fixture (tests/golden/augment.npz), and a
numpy float32 restatement of the three device passes, driven by the planner's descriptors, against the fixture's images."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_cases as AC                       # noqa: E402
from oracle import input_oracle as IO            # noqa: E402


@pytest.fixture(scope='module')
def g():
    return AC.load()


@pytest.fixture(scope='module')
def cases(g):
    return AC.cases(g)


def _plan(case):
    py, npr = case.rngs()
    aug = case.aug()
    plan = aug.plan([(case.H, case.W)], [case.boxes], py, npr)
    return aug, plan, AC.next_draws(py, npr)


def test_planner_targets_and_generators_match_reference(cases):
    for c in cases:
        _, plan, nxt = _plan(c)
        t = plan.targets[0]
        assert t.dtype == np.float32 and t.shape == c.target.shape, c.name
        assert np.array_equal(t.view(np.uint32), c.target.view(np.uint32)), (c.name, t, c.target)
        assert np.array_equal(nxt, c.next), c.name                         # both generators consumed exactly as the reference
        b = plan.samples[0].branches()
        for k in ('brightness', 'contrast', 'mirror', 'mode', 'jitter_fallback', 'crop_h', 'crop_w'):
            assert b[k] == c.branches[k], (c.name, k)


def test_planner_batch_of_32_matches_consecutive_reference_calls(g):
    import random
    from gssd.augment import DeviceSSDAugmentation
    studies, targets = AC.big_inputs()
    assert AC.sha(np.stack(studies)) == bytes(g['big__in_sha']).hex()
    py, npr = random.Random(AC.BIG_SEED), np.random.RandomState(AC.BIG_SEED)
    aug = DeviceSSDAugmentation(0.01, 1.5, 300, (49, 49, 49), use_normalize=True)
    plan = aug.plan([(512, 512)] * AC.BIG_B, targets, py, npr)
    got = np.concatenate(plan.targets)
    assert [len(t) for t in plan.targets] == list(g['big__counts'])
    assert np.array_equal(got.view(np.uint32), g['big__targets'].view(np.uint32))
    assert np.array_equal(AC.next_draws(py, npr), g['big__next'])
    keys = [str(k) for k in g['branch_keys']]
    for s, rec in zip(plan.samples, g['big__branches']):
        b = s.branches()
        assert all(b[k] == int(rec[keys.index(k)]) for k in ('brightness', 'contrast', 'mirror', 'mode', 'crop_h', 'crop_w'))


def test_fixture_covers_every_branch(g, cases):
    recs = [c.branches for c in cases]
    keys = [str(k) for k in g['branch_keys']]
    recs += [dict(zip(keys, (int(v) for v in r))) for r in g['big__branches']]
    assert {r['mode'] for r in recs} == set(range(6))                      # every RandomSampleCrop mode, None included
    for k in ('brightness', 'contrast', 'mirror', 'jitter_fallback', 'dropped'):
        assert {r[k] for r in recs} == {0, 1}, k
    assert any(c.branches['upsample'] for c in cases) and any(c.branches['crop_w'] > c.size for c in cases)
    assert any(c.p_only for c in cases) and any(c.H != c.W for c in cases) and any(len(c.boxes) > 1 for c in cases)
    assert any(c.size == 300 for c in cases)
    assert bytes(g['pillow_version']).decode() and bytes(g['numpy_version']).decode()


def test_constructor_refusals():
    from gssd.augment import DeviceSSDAugmentation
    with pytest.raises(AssertionError, match='use_normalize'):
        DeviceSSDAugmentation()                                             # the reference refuses use_normalize=False
    with pytest.raises(NotImplementedError):
        DeviceSSDAugmentation(use_normalize=True, use_pixel_link=True)
    DeviceSSDAugmentation(use_normalize=True)


def test_no_cpu_fallback():
    import torch
    from gssd import _lib
    from gssd.augment import DeviceSSDAugmentation
    aug = DeviceSSDAugmentation(use_normalize=True)
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        aug(torch.zeros(1, 4, 16, 16, 3, dtype=torch.uint8), [np.array(AC.BOX1, np.float32)])


def restate(aug, img, e, table):
    """The device passes in numpy float32, from one descriptor: extrema, quantise, mirror, Pillow resize, / 255."""
    S, H, W = aug.size, int(e['H']), int(e['W'])
    Y = np.arange(e['cy'], e['cy'] + e['ch']) - e['top']
    X = np.arange(e['cx'], e['cx'] + e['cw']) - e['left']
    iy, ix = (Y >= 0) & (Y < H), (X >= 0) & (X < W)
    u = img[:, np.clip(Y, 0, H - 1)][:, :, np.clip(X, 0, W - 1)]
    v = (u.astype(np.float32) + e['delta']).astype(np.float32)
    v = (v * e['alpha']).astype(np.float32)
    v = (v - aug.mean).astype(np.float32)
    v = np.where((iy[:, None] & ix[None, :])[None, :, :, None], v, np.float32(0))
    if aug.p_only:
        v = np.repeat(v[2:3], 4, 0)
    assert bool(e['fill']) == (not (iy.all() and ix.all()))
    mn, mx = v.min(), v.max()
    q = (((v - mn) / (mx - mn)).astype(np.float32) * np.float32(255)).astype(np.uint8)
    if e['mirror']:
        q = q[:, :, ::-1]
    # the descriptor's table offsets point at the coefficients of the window's sizes
    for n, (ob, ok, ks) in ((int(e['cw']), (e['hb'], e['hk'], e['hks'])), (int(e['ch']), (e['vb'], e['vk'], e['vks']))):
        if n == S:
            assert ks == 0
            continue
        b, k, ksz = IO.resample_coeffs(n, S)
        assert ks == ksz and np.array_equal(table.host[ob:ob + 2 * S], b.reshape(-1))
        assert np.array_equal(table.host[ok:ok + S * ks], k.reshape(-1))
    return np.stack([IO.pil_resize_u8(np.ascontiguousarray(q[p]), S) for p in range(4)])


def test_numpy_restatement_of_descriptors_reproduces_fixture(cases):
    from gssd.augment import _Tables
    for c in cases:
        aug, plan, _ = _plan(c)
        p = plan.samples[0]
        table = _Tables(c.size, max(p.canvas), 'cpu')
        d, work = aug.descriptors([(None, c.H, c.W, (c.H * c.W * 3, 1, c.W * 3, 3))], plan, table)
        assert work == (1 if c.p_only else 4) * int(d[0]['nrows']) * c.size * 3
        k = restate(aug, c.img, d[0], table)
        assert c.check_k(k), c.name
        assert np.array_equal(k.astype(np.float32) / np.float32(255.), (k / 255.).astype(np.float32))


def test_drop_in_name():
    from gssd.augment import DeviceSSDAugmentation
    from utils.augmentations import SSDAugmentationCUDA
    assert issubclass(SSDAugmentationCUDA, DeviceSSDAugmentation)
    aug = SSDAugmentationCUDA(0.01, 1.5, 300, [49] * 3, use_normalize=True, p_only=False)
    assert aug.size == 300 and aug.mean.tolist() == [49.] * 3
    with pytest.raises(AssertionError):
        SSDAugmentationCUDA(0.01, 1.5, 300, [49] * 3, use_normalize=False)
