"""The box-tail registry (tests/pixellink_box_cases.py) is fit for an exact comparison: with pixel_link/box_geometry.py alone, no row sits
on a rounding breakpoint or a filter threshold where two correct float64 evaluations could disagree, and the evaluation fixture of
tests/test_gpu_pixellink_boxes.py has no tied scores and a non-trivial expected AP.  No GPU."""
import numpy as np
import pytest

import pixellink_box_cases as R
from pixel_link import box_geometry as G

EPS = 1e-9


def _exact(rect):
    """An axis-aligned rectangle over integer points: every projection is an integer computed exactly."""
    c = rect['corners']
    return bool(np.all(c == np.round(c)) and all(float(s).is_integer() for s in rect['size']))


@pytest.mark.parametrize('row', R.all_rows(), ids=lambda r: r['name'])
def test_row_is_fit_for_exact_comparison(row):
    seen_kept = seen = 0
    for b in range(row['labels'].shape[0]):
        comps = R.host_components(row['labels'][b], row['dst'])
        assert int(row['labels'][b].max()) <= R.MAX_DET
        for _, rect, _, _ in comps:
            seen += 1
            w_, h_ = rect['size']
            for value, thr in ((min(w_, h_), row['min_height']), (rect['area'], row['min_area'])):
                # near a threshold only where rounding cannot decide: exact integer arithmetic, or a threshold of 0 (a size is a max
                # minus a min and an area the product of two sizes: never negative, so `value < 0` is false however it is rounded --
                # the 1e-16 height of the diagonal line under min_height = 0)
                assert value >= 0.0
                assert abs(value - thr) > EPS or _exact(rect) or thr <= 0, (row['name'], b, value, thr)
            if min(w_, h_) < row['min_height'] or rect['area'] < row['min_area']:
                continue
            seen_kept += 1
            # np.round(c, 6) then trunc: the integer changes where c crosses k - 0.5e-6
            c = np.asarray(rect['corners'], np.float64).ravel()
            dist = np.abs((c + 0.5e-6) - np.round(c + 0.5e-6))
            assert dist.min() > EPS, (row['name'], b, c[dist.argmin()])
    if row['name'] == 'empty':
        assert seen == 0
    elif row['name'] == 'cap_1024':
        assert seen == seen_kept == 1024
    elif row['name'] == 'identity_degenerate_cfgfilter':
        assert seen == 3 and seen_kept == 1                 # the pixel and the diagonal line are dropped, the block stays
    elif row['name'] == 'x2_filter_equalities':
        assert seen == 2 and seen_kept == 1                 # area 1 dropped, area 3 kept at equality
    else:
        assert seen_kept >= 1


def test_registry_reaches_the_branches_it_names():
    rows = {r['name']: r for r in R.hand_made_rows()}
    hulls = lambda row, b: [len(G.convex_hull(np.stack([xs, ys], 1))) for _, _, ys, xs in R.host_components(row['labels'][b], row['dst'])]
    assert hulls(rows['identity_degenerate_nofilter'], 0) == [1, 2, 4]
    assert hulls(rows['ties_identity'], 0) == [4, 4]
    assert max(hulls(rows['ties_x2_and_disc'], 1)) == 64 and hulls(rows['largest_map_80_edges'], 0) == [80]     # a full wave of edges; more than one
    down = rows['downscale']
    assert len(R.host_components(down['labels'][0], down['dst'])) == int(down['labels'].max()) - 2     # two components without destination pixels
    # filtered components between kept ones, and clamped corners
    boxes, _ = R.host_expected(rows['concave_and_order'])[0]
    assert len(boxes) < int(rows['concave_and_order']['labels'].max())
    clamp = rows['borders_and_clamp']
    raw = np.concatenate([rect['corners'].ravel() for _, rect, _, _ in R.host_components(clamp['labels'][1], clamp['dst'])])
    assert raw.min() < 0 and raw.max() > 59
    # closed forms (tests/test_pixellink_cpu.py)
    assert R.host_expected(rows['x4_closed_form'])[0][0] == [[80, 40, 99, 51], [160, 160, 163, 163], [28, 200, 31, 239]]
    assert R.host_expected(rows['x4_closed_form_minheight5'])[0][0] == [[80, 40, 99, 51]]


def test_evaluation_fixture_has_no_ties_and_a_real_ap():
    from oracle import eval_oracle as EO
    dets = []
    for o1, o2 in R.eval_batches():
        lab = R.oracle_labels(o1, o2, R.EVAL_THRESH)
        prob = R.host_prob(o1)
        for b in range(lab.shape[0]):
            boxes, scores = G.component_boxes(lab[b], prob[b], (R.EVAL_SIZE, R.EVAL_SIZE), R.CFG_FILTERS[0], R.CFG_FILTERS[1])
            dets.append([[s] + bx for s, bx in zip(scores, boxes)])
    assert [len(d) > 0 for d in dets] == [True, True, True, True, False]
    scores = np.sort(np.array([d[0] for img in dets for d in img], np.float64))
    assert np.diff(scores).min() > 2e-6 and np.abs(scores - R.EVAL_THRESH).min() > 2e-6
    assert len(dets[3]) == 1 and dets[3][0][0] < R.EVAL_THRESH and (scores > R.EVAL_THRESH).any()
    annos = R.eval_annotations(dets)
    k = max(len(d) for d in dets)
    det = np.zeros((len(dets), 2, k, 5), np.float32)
    for i, d in enumerate(dets):
        if d:
            det[i, 1, :len(d)] = np.asarray(d, np.float32)
    gts = [a[:, :-1] * R.EVAL_SIZE / R.EVAL_IMAGE if len(d) else np.zeros((0, 4)) for a, d in zip(annos, dets)]
    ap, iobb = EO.evaluate(det, np.ones((len(dets), 4), np.float32), gts, R.EVAL_THRESH, R.EVAL_AP, R.EVAL_IOBB, True)
    assert any(0.0 < v < 1.0 for v in ap + iobb), (ap, iobb)


def test_evaluate_hands_other_calls_to_test_ap_iobb(monkeypatch):
    """pixel_link.evaluate.test_net without use_pixel_link is test_ap_iobb.test_net with the same arguments."""
    import test_ap_iobb
    from pixel_link import evaluate
    seen = []
    monkeypatch.setattr(test_ap_iobb, 'test_net', lambda *a: seen.append(a) or ('ap', 'iobb'))
    out = evaluate.test_net('net', True, 'set', 'tf', 512, thresh=0.2, mode='v2', use_07_metric=False, ap_list=[0.3], iobb_list=[0.4],
                            visualize=True, output_path='o', model_name='m', batch_size=7)
    assert out == ('ap', 'iobb')
    assert seen == [('net', True, 'set', 'tf', 512, 0.2, 'v2', False, [0.3], [0.4], None, None, True, 'o', 'm', False, 7)]
