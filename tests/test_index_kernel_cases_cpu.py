"""The edge registry of the index kernels (tests/index_kernel_cases.py) on the CPU: the oracle against what the reference computed for
the fixture rows (tests/golden/index_edges.npz), every row's precondition on the oracle's result, the sensitivity of the rows to the
classic mistakes, and the argument checks of the three entry points (refused before any launch, so they run without a GPU).

Contracts, as everywhere in the suite: indices exact; Detect values within atol 3e-6 of the reference; losses within TOL."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_kernel_cases as K                        # noqa: E402
from gpu_common import TOL, rel                       # noqa: E402
from helpers import assert_mined_negatives_contract   # noqa: E402

CACHE = {}
WORST = {}


def oracle(family, row):
    """The oracle's result for a row, computed once and left unchanged."""
    key = (family, row.name)
    if key not in CACHE:
        inp = row.build()
        if family == 'detect':
            res = K.det_oracle(inp, row.params)
        elif family == 'nms':
            res = K.nms_oracle(inp, row.params)
        elif family == 'loss':
            res = K.loss_oracle(inp, row.params)
        else:
            res = {u: K.eval_oracle(inp, row.params, u) for u in (True, False)}
        CACHE[key] = (inp, res)
    return CACHE[key]


def worst(what, value):
    WORST[what] = max(WORST.get(what, 0.), float(value))
    print(f'worst {what}: {WORST[what]:.3g}')


@pytest.fixture(scope='module')
def fx(golden):
    g = golden('index_edges')
    return {p: K.unpack_rows(g, p) for p in ('detect', 'nms', 'loss', 'eval')}


ALL_ROWS = [(f, r) for f, rows in K.FAMILIES.items() for r in rows]
IDS = [f'{f}:{r.name}' for f, r in ALL_ROWS]


def test_registry_lists_what_it_should(fx):
    names = {f: [r.name for r in rows] for f, rows in K.FAMILIES.items()}
    for f, n in names.items():
        assert len(set(n)) == len(n), f
    for P in (1, 63, 64, 65, 255, 256, 257, 600):
        for C in (2, 3, 5):
            assert f'P_edges-P{P}-C{C}' in names['detect']
    for k in (1, 5, 64, 256):
        assert f'topk_edges-k{k}-n{k - 1}_{k}' in names['detect'] and f'topk_edges-k{k}-n{k + 1}_600' in names['detect']
    for C in (2, 3, 4, 5, 8):
        for P in (65, 1025):
            assert f'C_edges-C{C}-P{P}' in names['loss']
    assert {r.params['M'] for r in K.EVAL if 'M' in r.params} >= set(K.M_WANTED)
    assert all(r.name in names['detect'] for r in map(lambda n: K.by_name('detect', n), K.DIRTY_BUFFER_ROWS))
    # a row has a reference fixture exactly when the registry says so, and only with pairwise distinct scores
    assert set(fx['detect']) == {r.name for r in K.DETECT if r.fixture} and set(fx['nms']) == {r.name for r in K.NMS if r.fixture}
    assert set(fx['loss']) == {r.name for r in K.LOSS if r.name not in K.LOSS_ORACLE_ONLY}
    assert set(fx['eval']) == {r.name for r in K.EVAL if r.fixture}
    assert {r.name for r in K.LOSS if not r.fixture} == set(K.LOSS_TIE_ROWS) | set(K.LOSS_ORACLE_ONLY)


@pytest.mark.parametrize('family,row', ALL_ROWS, ids=IDS)
def test_fixture_rows_have_distinct_scores(family, row):
    if not row.fixture:
        return
    inp, res = oracle(family, row)
    if family == 'detect':
        assert K.det_distinct(inp, row.params)
    elif family == 'nms':
        assert np.unique(inp['scores']).size == inp['scores'].size
    elif family == 'loss':
        assert K.loss_distinct(inp, res)
    else:
        assert K.eval_distinct(inp, row.params)


@pytest.mark.parametrize('family,row', ALL_ROWS, ids=IDS)
def test_precondition(family, row):
    inp, res = oracle(family, row)
    if family == 'eval':
        assert row.pre(inp, res[True]) and row.pre(inp, res[False])
    else:
        assert row.pre(inp, res)


# ---- the oracle against the reference ----------------------------------------------------------------------------------------------------
def check_detect_fixture(out, keep, cnt, f, what):
    """``out[B, C, top_k, 5]``, ``keep[B, C, top_k]``, ``cnt[B, C]`` against a fixture row: counts and kept priors exact, the stored
    rows' values within 3e-6.  Returns the worst value difference."""
    assert np.array_equal(cnt, f['cnt']), what
    at_k = at_v = 0
    err = 0.
    for b in range(cnt.shape[0]):
        for cl in range(1, cnt.shape[1]):
            n = int(cnt[b, cl])
            if n == 0:
                continue
            assert np.array_equal(keep[b, cl, :n], f['keep'][at_k:at_k + n]), (what, b, cl)
            pos = K.sample_positions(n)
            ref = f['val'][at_v:at_v + pos.size]
            err = max(err, float(np.abs(out[b, cl, pos] - ref).max()))
            at_k, at_v = at_k + n, at_v + pos.size
    assert at_k == f['keep'].size and at_v == f['val'].shape[0] and err <= 3e-6, (what, err)
    return err


@pytest.mark.parametrize('row', [r for r in K.DETECT if r.fixture], ids=lambda r: r.name)
def test_detect_oracle_vs_reference(row, fx):
    inp, res = oracle('detect', row)
    B, C, top_k = res['out'].shape[:3]
    keep, cnt = K.keep_arrays(res['keeps'], B, C, top_k)
    worst('Detect oracle-reference abs', check_detect_fixture(res['out'], keep, cnt, fx['detect'][row.name], row.name))
    assert (res['out'][:, 0] == 0).all()


@pytest.mark.parametrize('row', K.NMS, ids=lambda r: r.name)
def test_nms_oracle_vs_reference(row, fx):
    _, res = oracle('nms', row)
    assert np.array_equal(res['keep'], fx['nms'][row.name]['keep'])


def check_loss_fixture(row, f, conf_t, pos, neg, num_neg, losses, loc_t, lca, what):
    """A loss result against a fixture row; ``lca`` are the oracle's mining scores (the contract of helpers.py is stated on them)."""
    B, P = conf_t.shape
    assert np.array_equal(conf_t, f['conf_t']), what
    assert np.array_equal(np.packbits(pos), f['pos']) and np.array_equal(num_neg, f['num_neg']), what
    err = max(rel(losses[0], f['losses'][0]), rel(losses[1], f['losses'][1]))
    assert err < TOL, (what, losses, f['losses'])
    if row.fixture:
        neg_ref = np.unpackbits(f['neg'])[:B * P].reshape(B, P).astype(bool)
        assert_mined_negatives_contract(neg, neg_ref, lca, pos.sum(1))
        ref = f['loc_t_pos']
        fin = np.isfinite(ref)
        assert np.allclose(loc_t[pos][fin], ref[fin], rtol=2e-6, atol=2e-6), what
    return err


@pytest.mark.parametrize('row', [r for r in K.LOSS if r.name not in K.LOSS_ORACLE_ONLY], ids=lambda r: r.name)
def test_loss_oracle_vs_reference(row, fx):
    _, res = oracle('loss', row)
    err = check_loss_fixture(row, fx['loss'][row.name], res['conf_t'], res['pos'], res['neg'], res['num_neg'], res['losses'], res['loc_t'],
                             res['loss_c_all'], row.name)
    worst('MultiBoxLoss oracle-reference rel', err)


@pytest.mark.parametrize('row', [r for r in K.EVAL if r.fixture], ids=lambda r: r.name)
def test_eval_oracle_vs_reference(row, fx):
    _, res = oracle('eval', row)
    for use07 in (True, False):
        got = np.array(list(res[use07]['ap']) + list(res[use07]['iobb']), np.float64)
        ref = fx['eval'][row.name][f'ap_{int(use07)}']
        assert np.array_equal(got, ref, equal_nan=True), (row.name, use07, got, ref)      # the same float64 steps: no difference at all
    if row.name == 'npos_zero':                                                           # the reference decides: 0 and NaN
        assert (fx['eval'][row.name]['ap_1'] == 0).all() and np.isnan(fx['eval'][row.name]['ap_0']).all()


# ---- sensitivity: the plain restatements, one switch per classic mistake -------------------------------------------------------------------
def same_detect(a, b):
    return np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and all(np.array_equal(a[1][k], b[1][k]) for k in b[1])


@pytest.mark.parametrize('row', K.DETECT, ids=lambda r: r.name)
def test_detect_plain_is_the_oracle(row):
    inp, res = oracle('detect', row)
    assert same_detect(K.detect_plain(inp, row.params), (res['out'], res['keeps']))


@pytest.mark.parametrize('switch', K.DETECT_SWITCHES)
def test_detect_rows_catch(switch):
    hit = []
    for family, rows in (('detect', K.DETECT), ('nms', K.NMS)):
        for row in rows:
            inp, res = oracle(family, row)
            if family == 'detect':
                if not same_detect(K.detect_plain(inp, row.params, **{switch: True}), (res['out'], res['keeps'])):
                    hit.append(row.name)
            elif switch in K.NMS_SWITCHES:
                k = K.nms_plain(inp['boxes'], inp['scores'], row.params['overlap'], row.params['top_k'], **{switch: True})
                assert np.array_equal(K.nms_plain(inp['boxes'], inp['scores'], row.params['overlap'], row.params['top_k']), res['keep'])
                if not np.array_equal(k, res['keep']):
                    hit.append(row.name)
    print(switch, 'changes', hit)
    assert hit, f'no Detect row notices "{switch}"'
    expected = dict(tie_high='ties_all', iou_lt='nms_exact-pair-at', thresh_ge='thresh_strict', topk_after='topk_edges-k64-n65_600',
                    dead_suppress='nms_exact-chain')[switch]
    assert expected in hit


def same_loss(a, res):
    return all(np.array_equal(a[k], res[k]) for k in ('conf_t', 'pos', 'neg', 'num_neg'))


@pytest.mark.parametrize('row', K.LOSS, ids=lambda r: r.name)
def test_loss_plain_is_the_oracle(row):
    inp, res = oracle('loss', row)
    assert same_loss(K.loss_plain(inp), res)


@pytest.mark.parametrize('switch', K.LOSS_SWITCHES)
def test_loss_rows_catch(switch):
    hit = [row.name for row in K.LOSS if not same_loss(K.loss_plain(oracle('loss', row)[0], **{switch: True}), oracle('loss', row)[1])]
    print(switch, 'changes', hit)
    expected = dict(first_twin='forced', last_max='forced', no_clip='clip', tie_high='ties_zero', keep_pos='C_edges-C5-P65')[switch]
    assert expected in hit


def same_eval(a, res):
    return np.array_equal(a['tp'], res['tp']) and (res['fp'] is None or np.array_equal(a['fp'], res['fp'])) \
        and np.array_equal(np.array(a['ap'] + a['iobb']), np.array(list(res['ap']) + list(res['iobb'])), equal_nan=True)


@pytest.mark.parametrize('row', K.EVAL, ids=lambda r: r.name)
def test_eval_plain_is_the_oracle(row):
    inp, res = oracle('eval', row)
    for use07 in (True, False):
        assert same_eval(K.eval_plain(inp, row.params, use07), res[use07])


@pytest.mark.parametrize('switch', K.EVAL_SWITCHES)
def test_eval_rows_catch(switch):
    hit = []
    for row in K.EVAL:
        inp, res = oracle('eval', row)
        if not same_eval(K.eval_plain(inp, row.params, True, **{switch: True}), res[True]):
            hit.append(row.name)
    print(switch, 'changes', hit)
    expected = dict(last_max='gt_edges', shared_used='metrics-8+0', ov_ge='thresh_strict-t0.25', score_ge='thresh_strict-t0.25',
                    ties_reversed='conf_ties', nogt_fp='gt_edges')[switch]
    assert expected in hit


# ---- argument checks: refused with GSSD_EINVAL before anything is launched -------------------------------------------------------------------
def host(n, dtype=np.float32):
    """A non-null, 64-byte aligned host buffer (never dereferenced: the calls below are refused first)."""
    raw = np.zeros(n * np.dtype(dtype).itemsize + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n * np.dtype(dtype).itemsize].view(dtype)


def test_argument_checks():
    from gssd._lib import lib
    bufs = [host(256) for _ in range(12)]
    p = [b.ctypes.data for b in bufs]
    assert all(a % 16 == 0 for a in p)

    def detect(B=1, P=8, C=2, top_k=4, conf_thresh=0.01, nms_thresh=0.45, loc=p[0]):
        return lib.gssd_detect(loc, p[1], p[2], B, P, C, top_k, conf_thresh, nms_thresh, 0.1, 0.2, 0, 0, p[3], p[4], p[5], None)
    for kw in (dict(top_k=257), dict(P=30001), dict(C=1), dict(nms_thresh=0.0), dict(conf_thresh=-0.5), dict(loc=p[0] + 4), dict(top_k=0),
               dict(B=0)):
        assert detect(**kw) == -1 and lib.gssd_last_error(), kw

    def match(N=1, top_k=4, stride=40, max_gt=2, n_iou=1, n_iobb=1):
        return lib.gssd_eval_match(p[0], stride, N, top_k, p[1], p[2], p[3], max_gt, 0.05, p[4], n_iou, n_iobb, p[5], p[6], None)
    for kw in (dict(n_iou=5, n_iobb=4), dict(n_iou=9, n_iobb=0), dict(max_gt=257), dict(stride=19), dict(n_iou=0, n_iobb=0)):
        assert match(**kw) == -1 and lib.gssd_last_error(), kw

    need = int(lib.gssd_multibox_loss_workspace_bytes(2))
    assert need >= 16 + 2 * 4

    def loss(B=2, P=8, C=2, ws_bytes=need, ws=p[11]):
        return lib.gssd_multibox_loss_forward_f32(p[0], p[1], p[2], p[3], p[4], B, P, C, 0.5, 0.1, 0.2, 3, p[5], p[6], p[7], p[8], p[9], p[10],
                                                  None, ws, ws_bytes, None)
    for kw in (dict(P=32768), dict(ws_bytes=need - 1), dict(C=1), dict(ws=p[11] + 4)):
        assert loss(**kw) == -1 and lib.gssd_last_error(), kw
