"""The index kernels at their edges: gssd_detect, the MultiBoxLoss forward (fused and four-launch) with gssd_loss_backward, and the AP /
IoBB evaluator, over the rows of tests/index_kernel_cases.py -- against the CPU oracle on every row and against what the reference
computed (tests/golden/index_edges.npz) on the rows whose scores are pairwise distinct.  Everything goes through gssd.ops, the drop-in
layers and the C ABI; no network runs.  tests/test_index_kernel_cases_cpu.py shows, without a GPU, that each row reaches the branch it
is named for and that the rows notice the classic mistakes.

Contracts (the suite's own): indices, counts and masks exact; Detect bit-equal to the oracle (same exp recipe) and within 3e-6 of the
reference; loc_t within 2e-6; mining scores within 4 ulp of their maximum; losses within TOL; gradients rtol 1e-4 / atol 1e-7; 11-point
AP bit-equal, area AP rtol 1e-13."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixtures dev / ops, rel, TOL)
import index_kernel_cases as K                # noqa: E402
from helpers import assert_mined_negatives_contract                                          # noqa: E402
from test_gpu_loss_fused import assert_same_state                                            # noqa: E402
from test_index_kernel_cases_cpu import check_detect_fixture, check_loss_fixture, oracle    # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx(golden):
    g = golden('index_edges')
    return {p: K.unpack_rows(g, p) for p in ('detect', 'nms', 'loss', 'eval')}


def i32(a):
    """fp32 -> its bits: NaN compares equal to NaN, -0 differs from +0, inf is a value."""
    a = a.cpu().numpy() if torch.is_tensor(a) else a
    return np.ascontiguousarray(a).view(np.int32)


# ==========================================================================================================================================
# Detect
# ==========================================================================================================================================
@pytest.mark.parametrize('row', K.DETECT, ids=lambda r: r.name)
def test_detect(dev, ops, fx, row):
    from layers.functions import Detect
    inp, res = oracle('detect', row)
    prm = row.params
    B, P, C = res['scores'].shape
    kw = dict(top_k=prm['top_k'], conf_thresh=prm['conf_thresh'], nms_thresh=prm['nms_thresh'], want_keep=True)
    loc, pri = torch.from_numpy(inp['loc']).to(dev), torch.from_numpy(K.priors(P)).to(dev)
    scores = torch.from_numpy(res['scores']).to(dev)
    out, keep, cnt = ops.detect(loc, scores, pri, C, **kw)
    keep_o, cnt_o = K.keep_arrays(res['keeps'], B, C, prm['top_k'])
    assert np.array_equal(cnt.cpu().numpy(), cnt_o), (cnt.cpu().numpy(), cnt_o)
    assert np.array_equal(keep.cpu().numpy(), keep_o)
    diff = i32(out) != i32(res['out'])
    print(row.name, 'kept', cnt_o[:, 1:].ravel(), 'words that differ from the oracle:', int(diff.sum()))
    assert not diff.any(), (np.argwhere(diff)[:5], out.cpu().numpy()[diff][:5], res['out'][diff][:5])
    if row.fixture:
        print('worst Detect kernel-reference abs:', check_detect_fixture(out.cpu().numpy(), keep_o, cnt_o, fx['detect'][row.name], row.name))
    # the reference's autograd.Function API
    out2 = Detect.apply(C, 0, prm['top_k'], prm['conf_thresh'], prm['nms_thresh'], loc, scores, pri)
    assert np.array_equal(i32(out2), i32(out))
    if 'logits' in inp:                 # the softmax inside the kernel: the same scores, so the same everything
        out3, keep3, cnt3 = ops.detect(loc, torch.from_numpy(inp['logits']).to(dev), pri, C, conf_is_logits=True, **kw)
        assert np.array_equal(i32(out3), i32(out)) and torch.equal(keep3, keep) and torch.equal(cnt3, cnt)


@pytest.mark.parametrize('row', K.NMS, ids=lambda r: r.name)
def test_nms_exact(dev, ops, fx, row):
    from layers import box_utils
    inp, res = oracle('nms', row)
    prm = row.params
    boxes, scores = torch.from_numpy(inp['boxes']).to(dev), torch.from_numpy(inp['scores']).to(dev)
    rows, keep, cnt = ops.detect_boxes(boxes, scores, prm['overlap'], prm['top_k'])
    n = int(cnt)
    k = keep[:n].cpu().numpy()
    assert n == res['keep'].shape[0] and np.array_equal(k, res['keep']), (k, res['keep'])
    assert np.array_equal(k, fx['nms'][row.name]['keep'])                                  # the reference
    assert (keep[n:] == -1).all() and (rows[n:] == 0).all()
    want = np.concatenate([inp['scores'][k, None], inp['boxes'][k]], 1)
    assert np.array_equal(i32(rows[:n]), i32(want))
    keep2, cnt2 = box_utils.nms(boxes, scores, prm['overlap'], prm['top_k'])
    assert cnt2 == n and np.array_equal(keep2[:n].cpu().numpy(), k) and (keep2[n:] == 0).all()


@pytest.mark.parametrize('name', K.DIRTY_BUFFER_ROWS)
def test_detect_dirty_buffers(dev, name):
    """gssd_detect promises to zero the rows past the count and the background rows and to set their keep to -1, whatever the buffers
    held: here they hold 7.0 / 12345 / -7, not zeros."""
    from gssd._lib import check, lib
    row = K.by_name('detect', name)
    inp, res = oracle('detect', row)
    prm = row.params
    B, P, C = res['scores'].shape
    top_k = prm['top_k']
    loc, pri = torch.from_numpy(inp['loc']).to(dev), torch.from_numpy(K.priors(P)).to(dev)
    lg = torch.from_numpy(inp['logits']).to(dev)
    out = torch.full((B, C, top_k, 5), 7.0, device=dev)
    keep = torch.full((B, C, top_k), 12345, device=dev, dtype=torch.int32)
    cnt = torch.full((B, C), -7, device=dev, dtype=torch.int32)
    check(lib.gssd_detect(loc.data_ptr(), lg.data_ptr(), pri.data_ptr(), B, P, C, top_k, prm['conf_thresh'], prm['nms_thresh'], 0.1, 0.2, 1, 0,
                          out.data_ptr(), keep.data_ptr(), cnt.data_ptr(), torch.cuda.current_stream().cuda_stream))
    keep_o, cnt_o = K.keep_arrays(res['keeps'], B, C, top_k)
    out, keep, cnt = out.cpu().numpy(), keep.cpu().numpy(), cnt.cpu().numpy()
    assert np.array_equal(cnt, cnt_o) and (cnt[:, 0] == 0).all()
    for b in range(B):
        for cl in range(C):
            n = int(cnt_o[b, cl])
            assert (i32(out[b, cl, n:]) == 0).all() and (keep[b, cl, n:] == -1).all(), (b, cl)
    assert (i32(out[:, 0]) == 0).all() and (keep[:, 0] == -1).all()
    assert np.array_equal(i32(out), i32(res['out'])) and np.array_equal(keep, keep_o)
    if name == 'one_class_empty':
        assert (cnt_o[:, 1:] == 0).any() and (cnt_o[2] == 0).all()      # an empty class beside the background; an empty image


# ==========================================================================================================================================
# MultiBoxLoss
# ==========================================================================================================================================
def backward_reference(inp, st, gl, gc):
    """float64 torch-CPU restatement of the backward: smooth-L1 sum over the positives and cross-entropy sum over the kernel's own selection,
    divided by N, times the incoming gradients."""
    sel = st['sel'].cpu()
    loc = torch.from_numpy(inp['loc']).double().requires_grad_()
    conf = torch.from_numpy(inp['conf']).double().requires_grad_()
    pos, s = (sel & 1).bool(), sel != 0
    N = float(st['n_total'].cpu())
    ll = torch.nn.functional.smooth_l1_loss(loc[pos], st['loc_t'].cpu().double()[pos], reduction='sum') / N
    lc = torch.nn.functional.cross_entropy(conf[s], st['conf_t'].cpu()[s], reduction='sum') / N
    (gl * ll + gc * lc).backward()
    return loc.grad.numpy(), conf.grad.numpy()


def check_backward(ops, dev, inp, st, f, settings):
    sel = st['sel'].cpu().numpy()
    for name, gl, gc in settings:
        dloc, dconf = ops.multibox_loss_backward(st, torch.tensor(gl, device=dev), None if gc is None else torch.tensor(gc, device=dev))
        dloc, dconf = dloc.cpu().numpy(), dconf.cpu().numpy()
        ref_l, ref_c = backward_reference(inp, st, gl, 0. if gc is None else gc)
        assert np.allclose(dloc, ref_l, rtol=1e-4, atol=1e-7) and np.allclose(dconf, ref_c, rtol=1e-4, atol=1e-7), name
        assert (i32(dloc[(sel & 1) == 0]) == 0).all() and (i32(dconf[sel == 0]) == 0).all(), name          # exactly 0 where nothing is selected
        if gc is None:
            assert (i32(dconf) == 0).all()
        if f is not None and f'dloc_{name}' in f:                                                          # the reference's own gradients
            assert np.allclose(dloc, f[f'dloc_{name}'], rtol=1e-4, atol=1e-7) and np.allclose(dconf, f[f'dconf_{name}'], rtol=1e-4, atol=1e-7), name
    dloc, dconf = ops.multibox_loss_backward(st, None, None)
    assert (i32(dloc) == 0).all() and (i32(dconf) == 0).all()


@pytest.mark.parametrize('row', K.LOSS, ids=lambda r: r.name)
def test_multibox_loss(dev, ops, fx, row):
    inp, res = oracle('loss', row)
    B, P, C = inp['conf'].shape
    pri = torch.from_numpy(K.priors(P)).to(dev)
    loc_d, conf_d = torch.from_numpy(inp['loc']).to(dev), torch.from_numpy(inp['conf']).to(dev)
    tgp, ngt = ops.pack_targets([torch.from_numpy(t) for t in inp['targets']], dev)
    st = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=True, fused=True)
    st_s = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=True, fused=False)
    assert_same_state(st, st_s, 'fused / four launches')
    st_n = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=False, fused=True)
    assert st_n['loss_c_all'] is None
    st_n['loss_c_all'] = st['loss_c_all']
    assert_same_state(st_n, st, 'without / with scores')
    # against the oracle
    sel, conf_t = st['sel'].cpu().numpy(), st['conf_t'].cpu().numpy()
    pos, neg = (sel & 1).astype(bool), (sel & 2).astype(bool)
    assert np.array_equal(conf_t, res['conf_t']) and np.array_equal(pos, res['pos'])
    loc_t = st['loc_t'].cpu().numpy()
    assert np.allclose(loc_t[pos], res['loc_t'][pos], rtol=2e-6, atol=2e-6)
    part = st['partial'].cpu().numpy()
    num_neg = part[:, 3].astype(np.int64)
    assert np.array_equal(num_neg, res['num_neg']) and np.array_equal(part[:, 2].astype(np.int64), res['num_pos'])
    assert_mined_negatives_contract(neg, res['neg'], res['loss_c_all'], res['num_pos'])
    lca = st['loss_c_all'].cpu().numpy()
    lca_err = np.abs(lca - res['loss_c_all']).max()
    assert lca_err <= 4 * np.spacing(np.float32(np.abs(res['loss_c_all']).max()))
    losses = st['losses'].cpu().numpy().astype(np.float64)
    err = max(rel(losses[0], res['losses'][0]), rel(losses[1], res['losses'][1]))
    print(row.name, 'losses', losses, 'rel err vs oracle', err, 'mining score err', lca_err, 'sel==3:', int((sel == 3).sum()))
    assert err < TOL and float(st['n_total']) == res['num_pos'].sum()
    # the selection logic itself is exact: the oracle's stable ranking of the kernel's own scores gives the same set
    order = np.argsort(-lca, axis=1, kind='stable')
    rank = np.argsort(order, axis=1, kind='stable')
    assert np.array_equal(neg, rank < num_neg[:, None])
    f = fx['loss'].get(row.name)
    if f is not None:
        print('worst MultiBoxLoss kernel-reference rel:', check_loss_fixture(row, f, conf_t, pos, neg, num_neg, losses, loc_t, res['loss_c_all'],
                                                                              row.name))
    check_backward(ops, dev, inp, st, f, K.GRADS if row.params.get('backward') else K.GRADS[1:2])


# ==========================================================================================================================================
# evaluator
# ==========================================================================================================================================
@pytest.mark.parametrize('row', K.EVAL, ids=lambda r: r.name)
def test_evaluator(dev, fx, row):
    from gssd.evaluator import DeviceEvaluator
    inp, res = oracle('eval', row)
    prm = row.params
    det, scales, gts = inp['det'], inp['scales'], inp['gts']
    na = len(prm['ap_list'])
    cuts = K.batch_splits(det.shape[0])
    assert len(set(np.diff(cuts))) > 1 or len(cuts) == 2
    for use07 in (True, False):
        ev = DeviceEvaluator(prm['thresh'], prm['ap_list'], prm['iobb_list'], use07)
        confs, flags = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            c, f = ev.add_batch(torch.from_numpy(det[a:b]).to(dev), scales[a:b], gts[a:b])
            confs.append(c.cpu().numpy())
            flags.append(f.cpu().numpy())
        ap, iobb = ev.result()
        got = np.array(list(ap) + list(iobb), np.float64)
        o = res[use07]
        want = np.array(list(o['ap']) + list(o['iobb']), np.float64)
        ref = fx['eval'][row.name][f'ap_{int(use07)}'] if row.fixture else want
        print(row.name, use07, got, 'abs err vs oracle', np.nanmax(np.abs(got - want), initial=0.))
        assert len(ap) == na and np.array_equal(np.isnan(got), np.isnan(want))
        if use07:
            assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got, ref, equal_nan=True)
        else:                                                                 # np.sum's pairwise order is not reproduced
            assert np.allclose(got, want, rtol=1e-13, atol=0, equal_nan=True) and np.allclose(got, ref, rtol=1e-13, atol=0, equal_nan=True)
        # TP / FP flags against the oracle's greedy loop (integer work: exact)
        conf, fl = np.concatenate(confs), np.concatenate(flags, axis=1)
        order = np.argsort(-conf, kind='stable')[:len(o['conf'])]
        assert np.array_equal(conf[order].astype(np.float64), o['conf']) and (conf == -np.inf).sum() == conf.size - len(o['conf'])
        assert np.array_equal(fl[:, order] == 1, o['tp'] == 1) and np.array_equal(fl[:, order] == 2, o['fp'] == 1)
        assert (fl[:, conf == -np.inf] == 0).all()
