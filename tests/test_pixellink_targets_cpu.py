"""PixelLink training targets, host half (no GPU): the numpy gather-form restatement against the reference's fixture
(tests/golden/pixellink_targets.npz), the augmentation planner's boxes against the reference's chain, and the host code of
gssd/pixellink_targets.py: packing, offsets, versions, errors and the new C entry point."""
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixellink_targets_ref as PR               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def g():
    return PR.load()


def same(got, want, k):
    if k == 'pixel_pos_weight':
        return got.dtype == want.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    return np.array_equal(got, want)


def test_restatement_reproduces_every_fixture_case(g):
    cases = PR.cases(g)
    assert len(cases) == 14 and {c.version for c in cases} == {'4s', '2s'}
    for c in cases:
        got = PR.batch(c.boxes, c.size, c.version)
        for k in PR.KEYS:
            assert same(got[k], c.want[k], k), (c.name, k)
    # the cases cover what they are for
    by = {c.name: c for c in cases}
    assert max(len(b) for b in by['many_4s'].boxes) == 255 and 0 in [len(b) for b in by['empty_2s'].boxes]
    assert by['odd37_4s'].want['pixel_mask'].shape[1:] == (9, 9) and len(by['b32_2s'].boxes) == 32
    ov = by['overlap_4s']
    assert ov.want['pixel_mask'][4].sum() == 0 and ov.want['neg_pixel_mask'][4].sum() < 16 * 16      # duplicates only: R == 0


def test_restatement_border_links():
    """The scatter form's quirk: a box on the last row links to itself downwards (dh = +1 clips onto its own row)."""
    pix, neg, w, link = PR.targets(np.array([[0.5, 0.9, 0.75, 1.0]], np.float32), 64, '4s')       # rows 14..15, cols 8..12 of 16
    assert pix[14:16, 8:13].all() and pix.sum() == 10 and w[15, 8] == 1.0
    assert link[1, 15, 8:13].all() and link[1, 14, 8:13].sum() == 0        # (+1, 0): the last row gets it, the first does not
    assert link[5, 14, 8:13].all() and link[5, 15, 8:13].sum() == 0        # (-1, 0): row 14 from row 15, nothing reaches 15


def test_planner_boxes_and_generators_match_the_reference_chain(g):
    """SSDAugmentation(use_pixel_link=True) draws nothing more than the plain chain: the planner's boxes, the restatement of their
    targets and both generators' next draws equal the reference's."""
    from gssd import synth
    from gssd.augment import DeviceSSDAugmentation
    MG = PR
    for v in MG.VERSIONS:
        pre = f'chain_{v}__'
        studies = [synth.synth_study_u8(7000 + i, 4, MG.CHAIN_SRC) for i in range(MG.CHAIN_B)]
        assert PR.sha(np.stack(studies)) == bytes(g[pre + 'in_sha']).hex()
        aug = DeviceSSDAugmentation(0.01, 1.5, MG.CHAIN_SIZE, (49, 49, 49), use_normalize=True, use_pixel_link=True,
                                    pixel_link_version=v)
        py, npr = random.Random(MG.CHAIN_SEEDS[v]), np.random.RandomState(MG.CHAIN_SEEDS[v])
        tg = [np.array(MG.CHAIN_BOXES[i % 2], np.float32) for i in range(MG.CHAIN_B)]
        plan = aug.plan([(MG.CHAIN_SRC, MG.CHAIN_SRC)] * MG.CHAIN_B, tg, py, npr)
        got = np.concatenate(plan.targets)
        assert [len(t) for t in plan.targets] == list(g[pre + 'counts'])
        assert np.array_equal(got.view(np.uint32), g[pre + 'boxes'].view(np.uint32))
        assert np.array_equal(np.array([py.random(), npr.random_sample()]), g[pre + 'next'])
        r = PR.batch(plan.targets, MG.CHAIN_SIZE, v)
        for k in PR.KEYS:
            assert same(r[k], g[pre + k], k), (v, k)


def test_versions_and_geometry():
    from gssd import _lib
    from gssd import pixellink_targets as PT
    assert PT.factor_of('2s') == 2 and PT.factor_of('4s') == 4 and PT.factor_of('8s') == 4      # any other string means 4
    assert PT.mask_side(300, '4s') == 75 and PT.mask_side(300, '2s') == 150 and PT.mask_side(37, '4s') == 9
    assert PT.mask_side(512, '2s') == 256 and PT.mask_side(37, '2s') == 18
    for bad in (None, 4, b'2s'):
        with pytest.raises(_lib.GssdError, match='version'):
            PT.factor_of(bad)
    with pytest.raises(_lib.GssdError, match='supported'):
        PT.prepare_targets([np.zeros((0, 5), np.float32)], 516, '2s')                      # 258 x 258 maps
    with pytest.raises(_lib.GssdError, match='supported'):
        PT.prepare_targets([np.zeros((0, 5), np.float32)], 3, '4s')                        # 0 x 0 maps


def test_packing_offsets_and_staging():
    from gssd import pixellink_targets as PT
    b0 = np.arange(15, dtype=np.float32).reshape(3, 5)
    b1 = np.zeros((0, 5), np.float32)
    b2 = torch.arange(8, dtype=torch.float32).reshape(2, 4) + 100
    packed, offs = PT.pack_boxes([b0, b1, b2, []])
    assert offs.dtype == np.int32 and offs.tolist() == [0, 3, 3, 5, 5]
    assert packed.dtype == np.float32 and packed.flags.c_contiguous and packed.shape == (5, 4)
    assert np.array_equal(packed[:3], b0[:, :4]) and np.array_equal(packed[3:], b2.numpy())
    buf, head = PT.staging(packed, offs)
    assert head % 16 == 0 and head >= offs.nbytes and buf.dtype == np.uint8
    assert np.array_equal(buf[:offs.nbytes].view(np.int32), offs)
    assert np.array_equal(buf[head:head + packed.nbytes].view(np.float32).reshape(-1, 4), packed)
    packed, offs = PT.pack_boxes([b1])
    assert packed.shape == (0, 4) and offs.tolist() == [0, 0] and PT.staging(packed, offs)[0].size >= 16


def test_errors_before_any_device_work():
    from gssd import _lib
    from gssd import pixellink_targets as PT
    ok = np.array([[0.1, 0.1, 0.5, 0.5, 0.]], np.float32)
    with pytest.raises(_lib.GssdError, match='at most 255'):
        PT.pack_boxes([np.zeros((256, 5), np.float32)])
    with pytest.raises(_lib.GssdError, match='at most 255'):
        PT.prepare_targets([ok, np.zeros((256, 5), np.float32)], 300, '4s', device='cpu')
    PT.pack_boxes([np.zeros((255, 5), np.float32)])
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        PT.prepare_targets([ok], 300, '4s', device='cpu')
    with pytest.raises(_lib.GssdError, match=r'\[n, 4\] or \[n, 5\]'):
        PT.pack_boxes([np.zeros((2, 3), np.float32)])
    with pytest.raises(_lib.GssdError, match='no labels'):
        PT.prepare_targets([ok[:, :4]], 300, '4s', device='cpu')
    with pytest.raises(_lib.GssdError, match='labels'):
        PT.prepare_targets([ok], 300, '4s', device='cpu', labels=[np.zeros(2, np.float32)])
    with pytest.raises(_lib.GssdError, match='empty batch'):
        PT.prepare_targets([], 300, '4s')
    with pytest.raises(_lib.GssdError, match='version'):
        PT.prepare_targets([ok], 300, None)


def test_augmentation_constructor():
    from gssd.augment import DeviceSSDAugmentation
    from utils.augmentations import SSDAugmentationCUDA
    with pytest.raises(NotImplementedError, match='pixel_link_version'):
        DeviceSSDAugmentation(use_normalize=True, use_pixel_link=True)                    # the version must be named
    for v in ('4s', '2s'):
        a = SSDAugmentationCUDA(0.01, 1.5, 300, (49, 49, 49), use_normalize=True, use_pixel_link=True, pixel_link_version=v)
        assert a.use_pixel_link and a.pixel_link_version == v
    a = DeviceSSDAugmentation(use_normalize=True, pixel_link_version='4s')                 # no pixel link: the version is unused
    assert not a.use_pixel_link and a.pixel_link_version is None


def test_entry_point_in_header_bindings_library_and_runner():
    from gssd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read()
    m = re.search(r'int\s+gssd_pixellink_targets\s*\(([^;]*)\)\s*;', hdr)
    assert m and m.group(1).replace('\n', ' ').split(',')[-1].strip() == 'gssd_stream_t stream'
    argtypes = _lib.SIGNATURES['gssd_pixellink_targets'][1]
    assert len(argtypes) == len(m.group(1).split(",")) == 10
    assert hasattr(_lib.lib, 'gssd_pixellink_targets') and _lib.lib.gssd_plan_fn_index(b'gssd_pixellink_targets') >= 0
    assert _lib.lib.gssd_abi_version() == 8
    # the launcher refuses bad arguments before it touches a device
    lib = _lib.lib
    assert lib.gssd_pixellink_targets(None, None, 1, 300, 4, None, None, None, None, None) == -1
    assert b'invalid argument' in lib.gssd_last_error()
    p = 16                                                   # any non-null address: refused before use
    assert lib.gssd_pixellink_targets(p, p, 1, 516, 2, p, p, p, p, None) == -1                     # M = 258
    assert lib.gssd_pixellink_targets(p, p, 0, 300, 4, p, p, p, p, None) == -1
    assert lib.gssd_pixellink_targets(p, p, 1, 3, 4, p, p, p, p, None) == -1
