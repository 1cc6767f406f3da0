"""PixelLink training targets on the MI355X: bitwise against the reference's fixture (tests/golden/pixellink_targets.npz) and the
numpy restatement (tests/pixellink_targets_ref.py), through prepare_targets and through DeviceSSDAugmentation(use_pixel_link=True)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixellink_targets_ref as PR               # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return PR.load()


@pytest.fixture(scope='module')
def cases(g):
    return PR.cases(g)


def check(out, want, M, B, tag):
    """Device dict vs stacked reference arrays (masks 0 / 1 in any integer dtype, weight float64 -> the collate's float32)."""
    assert out['pixel_mask'].dtype == torch.int64 and out['neg_pixel_mask'].dtype == torch.int64, tag
    assert out['pixel_pos_weight'].dtype == torch.float32 and out['link_mask'].dtype == torch.int64, tag
    assert tuple(out['pixel_mask'].shape) == (B, M, M) and tuple(out['link_mask'].shape) == (B, 8, M, M), tag
    assert all(out[k].is_cuda for k in PR.KEYS), tag
    for k in PR.KEYS:
        got = out[k].cpu().numpy()
        w = want[k]
        if k == 'pixel_pos_weight':
            w = torch.tensor(w, dtype=torch.float32).numpy()                 # FloatTensor(float64 array): round to nearest
            assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), (tag, k)
        else:
            assert np.array_equal(got, w.astype(np.int64)), (tag, k)


def test_fixture_every_image_alone(cases):
    from gssd.pixellink_targets import prepare_targets, mask_side
    for c in cases:
        M = mask_side(c.size, c.version)
        for i, b in enumerate(c.boxes):
            out = prepare_targets([b], c.size, c.version)
            check(out, {k: c.want[k][i:i + 1] for k in PR.KEYS}, M, 1, f'{c.name}[{i}]')
            assert out['boxes'][0].shape == (len(b), 5) and torch.equal(out['boxes'][0], torch.from_numpy(b))
            assert out['lables'][0].dtype == torch.float32 and torch.equal(out['lables'][0], torch.from_numpy(b[:, 4].copy()))


def test_fixture_mixed_batches(cases):
    """Every case as its own batch, and every (size, version) group of images as one batch."""
    from gssd.pixellink_targets import prepare_targets, mask_side
    groups = {}
    for c in cases:
        M = mask_side(c.size, c.version)
        check(prepare_targets(c.boxes, c.size, c.version), c.want, M, len(c.boxes), c.name)
        grp = groups.setdefault((c.size, c.version), ([], {k: [] for k in PR.KEYS}))
        grp[0].extend(c.boxes)
        for k in PR.KEYS:
            grp[1][k].append(c.want[k])
    for (size, version), (boxes, want) in groups.items():
        want = {k: np.concatenate(v) for k, v in want.items()}
        check(prepare_targets(boxes, size, version), want, mask_side(size, version), len(boxes), f'{size}/{version}')


def random_image(rng):
    n = int(rng.integers(0, 21))
    cx, cy = rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 1.2, n)
    w, h = rng.uniform(0, 0.6, n) * (rng.random(n) > 0.1), rng.uniform(0, 0.6, n)    # ~10 % zero-width boxes
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, np.zeros(n)], 1).astype(np.float32)
    flip = rng.random(n) < 0.1
    b[flip, :4] = b[flip][:, [2, 3, 0, 1]]
    return b


def test_seeded_fuzz_against_restatement():
    from gssd.pixellink_targets import prepare_targets, mask_side
    rng = np.random.default_rng(99)
    total = 0
    for size in (37, 64, 300):
        for version in ('4s', '2s'):
            imgs = [random_image(rng) for _ in range(50)]
            total += len(imgs)
            want = PR.batch(imgs, size, version)
            check(prepare_targets(imgs, size, version), want, mask_side(size, version), len(imgs), f'fuzz {size}/{version}')
    assert total == 300


def test_device_boxes_non_default_stream_and_labels(cases):
    from gssd.pixellink_targets import prepare_targets
    c = next(c for c in cases if c.name == 'b32_2s')
    dev_boxes = [torch.from_numpy(b).cuda() for b in c.boxes]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = prepare_targets(dev_boxes, c.size, c.version)
    torch.cuda.current_stream().wait_stream(s)
    check(out, c.want, 150, 32, 'device boxes on a side stream')
    assert all(t.is_cuda for t in out['boxes']) and all(t.is_cuda for t in out['lables'])
    assert all(torch.equal(t.cpu(), torch.from_numpy(b)) for t, b in zip(out['boxes'], c.boxes))
    # [n, 4] boxes + labels= give the same maps; labels become column 4
    labels = [np.full(len(b), 1., np.float32) for b in c.boxes]
    out2 = prepare_targets([b[:, :4] for b in dev_boxes], c.size, c.version, labels=labels)
    check(out2, c.want, 150, 32, 'device [n, 4] + labels')
    assert all(torch.equal(t.cpu(), torch.from_numpy(l_)) for t, l_ in zip(out2['lables'], labels))


def test_augmentation_targets_images_and_draws(g):
    """DeviceSSDAugmentation(use_pixel_link=True): targets bitwise equal to the reference chain; images and the generators' next
    draws identical to the plain augmentation from the same seeds."""
    from gssd import synth
    from gssd.augment import DeviceSSDAugmentation
    studies = [synth.synth_study_u8(7000 + i, 4, PR.CHAIN_SRC) for i in range(PR.CHAIN_B)]
    assert PR.sha(np.stack(studies)) == bytes(g['chain_4s__in_sha']).hex()
    raw = torch.from_numpy(np.stack(studies)).cuda()
    tg = [np.array(PR.CHAIN_BOXES[i % 2], np.float32) for i in range(PR.CHAIN_B)]
    for v in PR.VERSIONS:
        pre, seed = f'chain_{v}__', PR.CHAIN_SEEDS[v]
        kw = dict(use_normalize=True)
        plain = DeviceSSDAugmentation(0.01, 1.5, PR.CHAIN_SIZE, (49, 49, 49), **kw)
        pl = DeviceSSDAugmentation(0.01, 1.5, PR.CHAIN_SIZE, (49, 49, 49), use_pixel_link=True, pixel_link_version=v, **kw)
        py0, np0 = random.Random(seed), np.random.RandomState(seed)
        x0, t0 = plain(raw, tg, py_rng=py0, np_rng=np0)
        py1, np1 = random.Random(seed), np.random.RandomState(seed)
        x1, t1 = pl(raw, tg, py_rng=py1, np_rng=np1)
        assert torch.equal(x0, x1), v
        nxt = np.array([py1.random(), np1.random_sample()])
        assert np.array_equal(nxt, np.array([py0.random(), np0.random_sample()])) and np.array_equal(nxt, g[pre + 'next'])
        M = PR.CHAIN_SIZE // PR.factor_of(v)
        check(t1, {k: g[pre + k] for k in PR.KEYS}, M, PR.CHAIN_B, f'chain {v}')
        assert set(t1) == {'pixel_mask', 'neg_pixel_mask', 'pixel_pos_weight', 'link_mask', 'lables', 'boxes'}
        got = np.concatenate([t.numpy() for t in t1['boxes']])
        assert np.array_equal(got.view(np.uint32), g[pre + 'boxes'].view(np.uint32))
        assert all(torch.equal(a, b) for a, b in zip(t1['boxes'], t0))
        assert all(torch.equal(l_, b[:, 4]) for l_, b in zip(t1['lables'], t0))


def test_pixellink_training_step_on_device_targets():
    """One PixelLink step (plain configuration, B = 2) on device-built "4s" targets: the four loss terms equal those of the same
    step on restatement-built targets, and the backward is finite."""
    from gssd import synth
    from gssd.pixellink_targets import prepare_targets
    from pixel_link.criterion import PixelLinkLoss
    from test_pixellink_cpu import PLAIN, build
    rng = np.random.default_rng(5)
    boxes = [random_image(rng) for _ in range(2)]
    boxes[0] = np.concatenate([boxes[0], np.array([[0.3, 0.3, 0.6, 0.7, 0.]], np.float32)])      # at least one owner
    tgt = prepare_targets(boxes, 300, '4s')
    ref = PR.batch(boxes, 300, '4s')
    ref_t = dict(pixel_mask=torch.from_numpy(ref['pixel_mask']), neg_pixel_mask=torch.from_numpy(ref['neg_pixel_mask']),
                 pixel_pos_weight=torch.from_numpy(ref['pixel_pos_weight']).float(), link_mask=torch.from_numpy(ref['link_mask']))
    for k in PR.KEYS:
        assert torch.equal(tgt[k].cpu(), ref_t[k]), k
    net = build(PLAIN).cuda().train()
    x = synth.synth_images(2, seed=313).cuda()
    o1, o2 = net(x)

    def losses(t):
        crit = PixelLinkLoss()
        pp, pn = crit.pixel_loss(o1, t['pixel_mask'], t['neg_pixel_mask'], t['pixel_pos_weight'])
        lp, ln = crit.link_loss(o2, t['link_mask'])
        return pp, pn, lp, ln
    with torch.no_grad():
        want = [float(v) for v in losses({k: v.cuda() for k, v in ref_t.items()})]
    pp, pn, lp, ln = losses(tgt)
    got = [float(v.detach()) for v in (pp, pn, lp, ln)]
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    assert all(np.isfinite(got)) and got[0] > 0 and got[2] > 0
    (pp + pn + 0.5 * lp + 0.5 * ln).backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(gr).all().item() for gr in grads)
