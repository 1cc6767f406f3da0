"""Device SSDAugmentation on the MI355X: bitwise against the reference's fixture (tests/golden/augment.npz)."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_cases as AC                       # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def g():
    return AC.load()


@pytest.fixture(scope='module')
def cases(g):
    return AC.cases(g)


def to_k(x):
    """[B, 12, S, S] fp32 -> uint8 k [B, 4, S, S, 3] with x == fl32(k / 255) checked (the reference's output form)."""
    x = x.cpu().numpy()
    k = np.rint(x.astype(np.float64) * 255).astype(np.uint8)
    assert np.array_equal(k.astype(np.float32) / np.float32(255.), x), 'output is not exactly k / 255'
    B, _, S, _ = x.shape
    return k.reshape(B, 4, 3, S, S).transpose(0, 1, 3, 4, 2)


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_every_case_alone_is_bitwise_equal(cases):
    for c in cases:
        py, npr = c.rngs()
        raw = torch.from_numpy(c.img[None]).cuda()
        x, t = c.aug()(raw, [c.boxes], py_rng=py, np_rng=npr)
        assert x.shape == (1, 12, c.size, c.size) and x.dtype == torch.float32
        assert c.check_k(to_k(x)[0]), c.name
        assert t[0].dtype == torch.float32 and same_bits(t[0].numpy(), c.target), c.name
        assert np.array_equal(AC.next_draws(py, npr), c.next), c.name


def test_one_batch_mixed_geometry_and_layouts(cases):
    """The size-37 cases in ONE call: own generators per study (Plan.cat), sources of different sizes and layouts."""
    from gssd.augment import Plan
    group = [c for c in cases if c.size == 37 and not c.p_only]
    assert len(group) >= 7
    aug = group[0].aug()
    plans, studies = [], []
    for i, c in enumerate(group):
        py, npr = c.rngs()
        plans.append(aug.plan([(c.H, c.W)], [c.boxes], py, npr))
        t = torch.from_numpy(c.img).cuda()
        studies.append(t if i % 2 else t.permute(0, 3, 1, 2).contiguous())        # [4, H, W, 3] and the collate's [4, 3, H, W]
    x = aug.run(studies, Plan.cat(plans))
    k = to_k(x)
    for i, c in enumerate(group):
        assert c.check_k(k[i]), c.name


def test_raw_layouts_in_place(cases):
    c = next(c for c in cases if c.name == 'mode3')
    base = torch.from_numpy(c.img[None]).cuda()
    planar = base.permute(0, 1, 4, 2, 3).contiguous()                          # [B, 4, 3, H, W] as the reference collates
    wide = torch.zeros(1, 4, c.H, c.W + 5, 3, dtype=torch.uint8, device='cuda')
    wide[:, :, :, 2:2 + c.W] = base
    for raw in (base, planar, planar.permute(0, 1, 3, 4, 2), wide[:, :, :, 2:2 + c.W]):   # contiguous / strided views
        py, npr = c.rngs()
        x, _ = c.aug()(raw, [c.boxes], py_rng=py, np_rng=npr)
        assert c.check_k(to_k(x)[0])


def test_batch_32_512_to_300(g):
    from gssd.augment import DeviceSSDAugmentation
    studies, targets = AC.big_inputs()
    raw = torch.from_numpy(np.stack([studies[i % 4] for i in range(AC.BIG_B)])).cuda()
    py, npr = random.Random(AC.BIG_SEED), np.random.RandomState(AC.BIG_SEED)
    aug = DeviceSSDAugmentation(0.01, 1.5, 300, (49, 49, 49), use_normalize=True)
    x, t = aug(raw, targets, py_rng=py, np_rng=npr)
    k = to_k(x)
    assert k.reshape(-1)[g['big__sample_idx']].tolist() == g['big__sample'].tolist()
    assert AC.sha(k) == bytes(g['big__out_sha']).hex()
    assert same_bits(np.concatenate([v.numpy() for v in t]), g['big__targets'])
    assert np.array_equal(AC.next_draws(py, npr), g['big__next'])
    aug.check_not_flat()


def test_global_generators_are_the_default(cases):
    c = next(c for c in cases if c.name == 'mode0')
    st = random.getstate(), np.random.get_state()
    try:
        random.seed(c.seed)
        np.random.seed(c.seed)
        x, t = c.aug()(torch.from_numpy(c.img[None]).cuda(), [c.boxes])
        assert c.check_k(to_k(x)[0]) and same_bits(t[0].numpy(), c.target)
        assert np.array_equal(AC.next_draws(random, np.random), c.next)
    finally:
        random.setstate(st[0])
        np.random.set_state(st[1])


def test_non_default_stream_and_out(cases):
    c = next(c for c in cases if c.name == 'mode4_up')
    s = torch.cuda.Stream()
    raw = torch.from_numpy(c.img[None]).cuda()
    out = torch.full((1, 12, c.size, c.size), float('nan'), device='cuda')
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        py, npr = c.rngs()
        x, _ = c.aug()(raw, [c.boxes], out=out, py_rng=py, np_rng=npr)
    torch.cuda.current_stream().wait_stream(s)
    assert x is out and c.check_k(to_k(out)[0])


def test_errors(cases):
    from gssd import _lib
    c = cases[0]
    aug = c.aug()
    raw = torch.from_numpy(c.img[None])
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        aug(raw, [c.boxes])
    with pytest.raises(_lib.GssdError, match='uint8'):
        aug(raw.cuda().float(), [c.boxes])
    with pytest.raises(_lib.GssdError, match='targets'):
        aug(raw.cuda(), [c.boxes, c.boxes])
    with pytest.raises(_lib.GssdError, match='out must be'):
        aug(raw.cuda(), [c.boxes], out=torch.empty(1, 12, c.size + 1, c.size, device='cuda'))
    plan = aug.plan([(c.H + 1, c.W)], [c.boxes])
    with pytest.raises(_lib.GssdError, match='planned'):
        aug.run(raw.cuda(), plan)


def test_gssdpp_training_step_on_augmented_batch(cases):
    """One GSSD++ step (forward, MultiBoxLoss, backward) on a B = 4 batch that the device augmentation made."""
    from gssd import synth
    from gssd.augment import DeviceSSDAugmentation
    from layers.modules import MultiBoxLoss
    from models.ssd_multiphase_custom_group import build_ssd
    c = next(c for c in cases if c.name == 'src96')
    raw = torch.from_numpy(np.stack([c.img] * 4)).cuda()
    aug = DeviceSSDAugmentation(0.01, 1.5, 300, (49, 49, 49), use_normalize=True)
    x, t = aug(raw, [AC.BOX1, AC.BOX3, AC.BOX1, AC.BOX3], py_rng=random.Random(5), np_rng=np.random.RandomState(5))
    net = build_ssd('train', 300, 2, True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.cuda().train()
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    ll, lc = crit(net(x), [v.cuda() for v in t])
    (ll + lc).backward()
    assert torch.isfinite(ll).item() and torch.isfinite(lc).item()
    assert all(torch.isfinite(p.grad).all().item() for p in net.parameters() if p.grad is not None)
