"""The PixelLink tail registry (tests/pixellink_tail_cases.py) is fit for what tests/test_gpu_pixellink_tail.py asserts with it: every loss
row leaves no mining decision to rounding and puts the cut where its name says, every decode row's id regions are 8-connected and its expected
label map is what the oracle's decoding (and the float64 restatement) give, the limits the rows are placed around are those of
csrc/pixellink.hip, and each classic mistake, applied to the float64 restatement, fails at least one row.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pixellink_tail_cases as K
from oracle import pixellink_oracle as PO


def test_limits_are_those_of_the_source():
    c = K.source_constants()
    assert c['PL_SORT'] == K.PL_SORT and c['PL_MAXPIX'] == K.PL_MAXPIX and c['PL_MAXPIX_LDS'] == K.PL_MAXPIX_LDS
    assert c['PL_STAT_COMPS'] == K.PL_STAT_COMPS and c['TP'] == [K.TP] and c['wgrad_blocks'] == 4      # one pass per 128 pixels, four launch sites
    assert c['sort_switch'] and c['decode_switch'] and c['decode_limit']
    from pixel_link import pixel_link_config as cfg, postprocess
    assert (cfg.neg_pos_ratio, cfg.pixel_conf_threshold, cfg.link_conf_threshold) == (K.NEG_POS_RATIO, K.PIXEL_THR, K.LINK_THR)
    assert postprocess.STAT_COMPS_MAX == K.PL_STAT_COMPS
    # the rows sit on both sides of every switch
    hw = lambda sizes: [h * w for h, w in sizes]
    assert hw(K.SORT_SIZES) == [35, 1023, 1024, 1025, K.PL_SORT] and hw(K.SELECT_SIZES)[0] == K.PL_SORT + 1
    names = [r.name for r in K.DECODE]
    assert len(set(names)) == len(names) and len({r.name for r in K.LOSS}) == len(K.LOSS)
    size = {r.name: r.build()['ids'].shape[1:] for r in K.DECODE if r.name.startswith('sizes')}
    assert size['sizes 64x128'][0] * size['sizes 64x128'][1] == K.PL_MAXPIX and size['sizes 3x2731'][0] * size['sizes 3x2731'][1] == K.PL_MAXPIX + 1
    assert size['sizes 128x208'][0] * size['sizes 128x208'][1] == K.PL_MAXPIX_LDS and size['sizes 1x26625'][1] == K.PL_MAXPIX_LDS + 1
    assert {hw_ for _, _, _, hw_ in K.FINAL} >= {1, K.TP - 1, K.TP, K.TP + 1} and any(B * HW > K.TP > HW for _, _, B, HW in K.FINAL)


# ---- loss ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(K.LOSS)), ids=[r.name for r in K.LOSS])
def test_loss_row_is_fit(i):
    row, ref = K.LOSS[i], K.loss_reference(i)
    inp = ref['inp']
    d = inp['out1'][:, 0].astype(np.float64) - inp['out1'][:, 1].astype(np.float64)
    sat = any(c.startswith('saturated') for c in row.contents)
    # the recipe: d on the grid (or a saturated level), exact in fp32
    on_grid = (np.abs(d) <= 6) & (d / K.GRID == np.round(d / K.GRID))
    assert bool((on_grid | (np.isin(d, K.SAT) & sat)).all())
    # the condition: adjacent distinct p0 levels of the row differ by more than 64 fp32 ulp
    lv = np.unique(K.sigmoid64(d))
    if len(lv) > 1:
        assert bool((np.diff(lv) > 64 * np.spacing(lv[1:].astype(np.float32)).astype(np.float64)).all()), row.name
    if sat:                                                           # the keys the radix select is fed: 0x00000000, 0x3f000000, 0x3f800000
        p0 = torch.softmax(torch.from_numpy(inp['out1']), 1)[:, 0].numpy()
        cand = inp['neg'] == 1
        assert sorted(set(p0[cand].view(np.uint32).tolist())) == [0x00000000, 0x3f000000, 0x3f800000]
    # the oracle (fp32 softmax of torch) mines the same mask: no decision depends on the implementation
    t = lambda k: torch.from_numpy(inp[k])
    vals = PO.pixel_link_loss(t('out1'), t('out2'), t('pix'), t('neg'), t('posw'), t('link'), neg_pos_ratio=row.ratio)
    assert np.array_equal(vals[4].numpy(), ref['mask'])
    with np.errstate(invalid='ignore'):
        want = ref['per_image'].mean(0)
    assert np.array_equal(np.isnan(vals[:4]), np.isnan(want))
    assert K.relerr(np.nan_to_num(np.array(vals[:4])), np.nan_to_num(want)) < 1e-6       # (the oracle's cross entropy is fp32)
    # the cut is where the name says
    for b, c in enumerate(row.contents):
        area, ncand, k, sel = int(ref['area'][b]), int(ref['ncand'][b]), int(ref['neg_area'][b]), int(ref['mask'][b].sum())
        dc = np.sort(d[b][inp['neg'][b] == 1])
        below = int((dc < dc[k - 1]).sum()) if k else 0
        upto = int((dc <= dc[k - 1]).sum()) if k else 0
        assert sel == upto
        if c == 'no_positives':
            assert area == 0 and k == min(10000, ncand) and (ncand < 10000 or (row.H * row.W == 10100 and k == 10000 and sel > k))
        elif c == 'fewer_candidates':
            assert 0 < ncand < 3 * area and k == ncand == sel
        elif c == 'exact_k':
            assert ncand == 3 * area == k == sel
        elif c == 'k_is_1':
            assert area == 1 and row.ratio == 1 and k == 1 < ncand
        elif c == 'one_candidate':
            assert ncand == 1 == k == sel and area > 0
        elif c == 'ties_straddle':
            assert below < k - 1 and k < upto
        elif c == 'ties_ends':
            assert below < k - 1 and upto == k
        elif c == 'ties_begins':
            assert below == k - 1 and upto > k
        elif c.startswith('saturated'):
            assert dc[k - 1] == K.SAT[('saturated_0', 'saturated_half', 'saturated_1').index(c)] and below < k < upto
        elif c == 'mask_values':
            assert set(np.unique(inp['neg'][b])) == {0, 1, 2} and bool(((inp['neg'][b] == 1) & (inp['pix'][b] == 1)).any())
        elif c == 'no_candidates':
            assert ncand == 0 and area > 0 and k == 0 and sel == 0
        elif c == 'nothing_at_all':
            assert ncand == 0 and area == 0 and np.isnan(ref['per_image'][b, :2]).all() and not np.isnan(ref['per_image'][b, 2:]).any()
            assert float(np.abs(ref['d1'][b]).max()) == 0.0
        elif c == 'links_all_1':
            assert ref['per_image'][b, 3] == 0.0 and ref['per_image'][b, 2] > 0
        elif c == 'links_all_0':
            assert ref['per_image'][b, 2] == 0.0 and ref['per_image'][b, 3] > 0
        elif c == 'posw_zero':
            assert ref['per_image'][b, 0] == 0.0 and ref['per_image'][b, 2] == ref['per_image'][b, 3] == 0.0 and float(np.abs(ref['d2'][b]).max()) == 0.0
        else:
            assert c == 'ordinary' and 0 < k < ncand
    assert np.isfinite(ref['d1']).all() and np.isfinite(ref['d2']).all()


def test_loss_rows_cover_the_issue():
    contents = {c for r in K.LOSS for c in r.contents}
    for H, W in K.SWITCH:                                            # the same content rule on both sides of the switch
        here = {c for r in K.LOSS if (r.H, r.W) == (H, W) for c in r.contents}
        assert here == contents
    assert {(r.H, r.W) for r in K.LOSS} == set(K.SORT_SIZES + K.SELECT_SIZES)
    assert any(r.B == 4 for r in K.LOSS)
    assert K.reference_defines_loss(0) and not all(K.reference_defines_loss(i) for i in range(len(K.LOSS)))


@pytest.mark.parametrize('mutant', ['lt', 'rank_plus_1', 'no_10000', 'mask_nonzero'])
def test_loss_mutant_fails_a_row(mutant):
    failed = []
    for i, row in enumerate(K.LOSS):
        ref = K.loss_reference(i)
        inp = ref['inp']
        d = inp['out1'][:, 0].astype(np.float64) - inp['out1'][:, 1].astype(np.float64)
        for b in range(row.B):
            m = K.mine(d[b], inp['neg'][b], inp['pix'][b], row.ratio, mutant)
            if not np.array_equal(m[0].reshape(row.H, row.W), ref['mask'][b]) or m[3] != ref['neg_area'][b]:
                failed.append(row.name)
    print(mutant, 'fails', len(failed), 'images')
    assert failed
    side = lambda n: {r.name: r.H * r.W <= K.PL_SORT for r in K.LOSS}[n]
    assert {side(n) for n in failed} == {True, False}                 # on both kernels


# ---- decode --------------------------------------------------------------------------------------------------------------------------------
RUN = [r for r in K.DECODE if not r.error]


@pytest.mark.parametrize('row', RUN, ids=[r.name for r in RUN])
def test_decode_row_is_fit(row):
    d = row.build()
    for b in range(len(d['ids'])):
        ids, labels = d['ids'][b], d['labels'][b]
        for v in np.unique(ids[ids > 0]):
            assert K.is_connected(ids == v), (row.name, b, int(v))
        assert int(labels.max()) == len(np.unique(ids[ids > 0])) and np.array_equal(labels > 0, ids > 0)
        first = [int(np.flatnonzero(labels.ravel() == c)[0]) for c in range(1, int(labels.max()) + 1)]
        assert first == sorted(first)                                 # numbered by the raster order of the first pixel
        assert np.array_equal(K.decode64(d['out1'][b], d['out2'][b], *row.thresholds), labels)
        if int((ids > 0).sum()) <= 2000:
            got = PO.decode_links(torch.from_numpy(d['out1'][b:b + 1]), torch.from_numpy(d['out2'][b:b + 1]), *row.thresholds)[0]
            assert np.array_equal(got, labels), (row.name, b)


def test_decode_rows_reach_their_branches():
    rows = {r.name: r for r in K.DECODE}
    count = lambda n: int(rows[n].build()['labels'].max())
    assert [count(f'table {c}') for c in (1023, 1024, 1025, 2813)] == [1023, 1024, 1025, 2813]
    assert rows['table 2813'].build()['ids'].shape[1:] == (75, 75) and rows['table 1025'].max_comps == (1, 512, 1024, 2048)
    for H, W in ((5, 7), (31, 33), (32, 32), (25, 41), (75, 75)):     # a root on each side of a thread's chunk boundary, and the last pixel
        lab = rows[f'rank_chunks {H}x{W}'].build()['labels'][0].ravel()
        per = -(-H * W // 1024)
        ts = [t for t in range(1, 1024) if per * t < H * W and lab[per * t - 1] and lab[per * t]]
        assert len(ts) >= 3 and lab[-1] and (per == {35: 1, 1023: 1, 1024: 1, 1025: 2, 5625: 6}[H * W])
    d = rows['one_direction'].build()
    lit = [(d['out2'][0, 2 * n + 1] > 0) for n in range(8)]
    assert all(int(l.sum()) == 2 for l in lit) and int(sum(l.sum() for l in lit)) == 16 == int(d['labels'].max())
    for k in range(16):                                               # one lit link per component; as the earlier and as the later pixel
        ys, xs = np.nonzero(d['labels'][0] == k + 1)
        assert sum(int(l[ys, xs].sum()) for l in lit) == 1
    # bars: every wave of 64 consecutive pixels holds at most one component; stripes: every full wave of the middle rows holds both
    bars = rows['stats_paths bars'].build()['labels'][0].ravel()
    assert all(len(set(bars[i:i + 64][bars[i:i + 64] > 0])) <= 1 for i in range(0, len(bars), 64)) and len(bars) > 1024
    st = rows['stats_paths stripes'].build()['labels'][0].ravel()
    assert sum(len(set(st[i:i + 64])) == 2 for i in range(0, len(st), 64)) >= len(st) // 64 - 4
    t1025 = rows['table 1025'].build()['labels'][0].ravel()
    assert any(0 < (w[w > 0].min() if w.any() else 0) <= K.PL_STAT_COMPS < w.max() for w in (t1025[i:i + 64] for i in range(0, len(t1025), 64)))
    th = rows['thresholds'].build()
    assert bool((th['out1'][0, 0] == th['out1'][0, 1]).any()) and bool((th['out2'][0, 0::2] == th['out2'][0, 1::2]).any())
    assert len(rows['batch'].build()['labels']) == 3 and int(rows['batch'].build()['labels'][1].max()) == 0


def test_score_levels_fit_the_summation_bound():
    """A one-pixel component's score sum is one fp32 number: the levels in use leave the bound count * 2^-24 * sum|score| room for it."""
    ratios = [K.score_level_ratio(j) for j in range(32)]
    assert all(ratios[j] <= 0.75 for j in K.SCORE_J) and ratios[0] <= 0.75          # (j = 0: the -+5 of every other row)
    assert sorted(j for j in range(32) if ratios[j] > 1.0) == [5, 7, 21] and len(K.SCORE_J) == 20
    for name in ('table 1023', 'table 2813', 'stats_paths bars'):
        o1 = {r.name: r for r in K.DECODE}[name].build()['out1'][0]
        assert len(np.unique(o1[0][o1[1] > 0])) > 10 and set(np.unique((o1[0][o1[1] > 0] + 5) * 8).astype(int)) <= set(K.SCORE_J)


@pytest.mark.parametrize('mutant', ['ge', 'no_clip', 'opp_n', 'drop_6'])
def test_decode_mutant_fails_a_row(mutant):
    failed = []
    for row in RUN:
        d = row.build()
        if d['ids'][0].size > 2000:
            continue
        for b in range(len(d['ids'])):
            if not np.array_equal(K.decode64(d['out1'][b], d['out2'][b], *row.thresholds, mutant=mutant), d['labels'][b]):
                failed.append(row.name)
    print(mutant, 'fails', sorted(set(failed)))
    assert failed
    want = {'ge': 'thresholds', 'no_clip': 'row_wrap 5x13', 'opp_n': 'one_direction', 'drop_6': 'late_merge both'}[mutant]
    assert want in failed
    if mutant == 'no_clip':
        assert 'row_wrap 13x5' in failed


# ---- cascade and final ---------------------------------------------------------------------------------------------------------------------
def _torch_interp(src, Hd, Wd):
    return F.interpolate(torch.from_numpy(src).double().permute(0, 3, 1, 2), size=(Hd, Wd), mode='bilinear', align_corners=True).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('r', K.INTERP, ids=K.interp_id)
def test_interp_restatement_is_torch(r):
    (Hs, Ws, Hd, Wd), C = r
    inp = K.interp_inputs(r)
    assert K.relerr(K.interp64(inp['src'], Hd, Wd), _torch_interp(inp['src'], Hd, Wd)) < 1e-13
    src = torch.from_numpy(inp['src']).double().permute(0, 3, 1, 2).requires_grad_()
    g = torch.from_numpy(inp['dout2']).double().permute(0, 3, 1, 2)
    (F.interpolate(src, size=(Hd, Wd), mode='bilinear', align_corners=True) * g).sum().backward()
    assert K.relerr(K.interp_bwd64(inp['dout2'], Hs, Ws), src.grad.permute(0, 2, 3, 1).numpy()) < 1e-13
    if (Hs, Ws) == (Hd, Wd):
        assert np.array_equal(K.interp64(inp['src'], Hd, Wd, dtype=np.float32), inp['src'])
    assert float(np.abs(inp['dsrc0']).min()) > 0 and float(np.abs(inp['dadd0']).min()) > 0 and bool((inp['dout'].reshape(K.INTERP_B, -1, C)[:, 0::2] == 0).all())


@pytest.mark.parametrize('mutant', ['swap_hw', 'scale_in_out'])
def test_interp_mutant_fails_a_row(mutant):
    failed = [K.interp_id(r) for r in K.INTERP
              if K.relerr(K.interp64(K.interp_inputs(r)['src'], r[0][2], r[0][3], mutant), K.interp64(K.interp_inputs(r)['src'], r[0][2], r[0][3])) > 1e-3]
    assert failed
    # ... and none of the square shapes the other tests use would notice a swap
    sq = np.random.default_rng(0).normal(size=(1, 19, 19, 2))
    assert mutant != 'swap_hw' or np.array_equal(K.interp64(sq, 38, 38, mutant), K.interp64(sq, 38, 38))


def test_final_rows_and_gates():
    assert {(f, n) for f, n, _, _ in K.FINAL} == {('final', n) for n in range(1, 5)} | {('final5', n) for n in range(1, 6)}
    assert {(B, HW) for _, _, B, HW in K.FINAL} == set(K.FINAL_SIZES) and (5, 50) in K.FINAL_SIZES
    assert K.final_masks(3) == [0, 7, 1, 2, 4]
    hit = False
    for r in K.FINAL:
        inp = K.final_inputs(r)
        masks = K.final_masks(r[1])
        r64 = K.final64(inp, masks[1])
        r32 = K.final32(inp, masks[1])
        # the allowance of every row stays below what test_final5_kernels allows
        for fam, e32 in (('final_fwd', max(K.relerr(r32['out1'], r64['out1']), K.relerr(r32['out2'], r64['out2']))),
                         ('final_dfeat', max(K.relerr(a, b) for a, b in zip(r32['g'], r64['g']))),
                         ('final_wgrad', max(K.relerr(r32['dw1'], r64['dw1']), K.relerr(r32['dw2'], r64['dw2'])))):
            assert K.bound(fam, e32) < K.EXISTING_BOUND[fam], (K.final_id(r), fam, e32)
        # the mistake: accumulate_mask ignored
        for m in masks[1:]:
            bad = K.final64(inp, m, mutant='ignore_acc')
            hit |= any(K.relerr(a, b) > 1e-3 for a, b in zip(bad['g'], K.final64(inp, m)['g']))
    assert hit
    for r in K.INTERP:
        (Hs, Ws, Hd, Wd), C = r
        inp = K.interp_inputs(r)
        g = inp['dout'].astype(np.float64) + inp['dout2']
        e32 = K.relerr(inp['dsrc0'] + K.interp_bwd64(g.astype(np.float32), Hs, Ws, dtype=np.float32), inp['dsrc0'] + K.interp_bwd64(g, Hs, Ws))
        assert K.bound('interp_bwd', e32) < K.EXISTING_BOUND['interp_bwd'], (K.interp_id(r), e32)
