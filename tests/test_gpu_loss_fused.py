"""The fused MultiBoxLoss forward (gssd_multibox_loss_forward_f32: two launches) and the one-launch heads reduce
(gssd_heads_reduce2_f32) against the launch sequences they replace.  The contract is IDENTITY, bit for bit, with the kernels that
tests/test_gpu_loss_detect.py pins to the reference and the oracle: there is no tolerance anywhere in this file.  Floats are compared
through integer views (loc_t holds -inf for images without boxes, the losses of a batch without boxes are inf / nan)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixtures dev / ops)
from gpu_common import O, ROOT                # noqa: E402,F401
from index_kernel_cases import FAR, prior_box_as_target, priors, rand_boxes      # noqa: E402  (shared with the edge registry)

pytestmark = pytest.mark.gpu


def scenario(name, P, B, C, seed):
    """-> (loc, conf, targets): what the issue's list of cases asks for, at any P / B / C."""
    rng = np.random.default_rng(seed)
    pri = priors(P)
    loc = rng.normal(0, 1.0, size=(B, P, 4)).astype(np.float32)
    conf = rng.normal(0, 2.0, size=(B, P, C)).astype(np.float32)
    if name == 'rand':              # an image without boxes between two with boxes (B = 3)
        counts = [3, 0, 1][:B]
        tg = [rand_boxes(rng, n, C) for n in counts]
    elif name == 'empty_all':       # N = 0: the losses are inf / nan
        tg = [np.zeros((0, 5), np.float32) for _ in range(B)]
    elif name == 'zeros':           # every score ties: the cut falls inside one tie group
        conf[:] = 0
        tg = [rand_boxes(rng, n, C) for n in [3, 1, 0][:B]]
    elif name == 'quant':           # many ties at the cut
        conf = (np.round(conf * 4) / 4).astype(np.float32)
        tg = [rand_boxes(rng, n, C) for n in [3, 1, 3][:B]]
    elif name == 'many64':          # 64 boxes; at small P 3 x positives exceeds P - 1 and the clip applies
        def many():
            if P > 65:
                return rand_boxes(rng, 64, C)
            # the priors themselves (each forces its own prior: 64 positives among 65 priors), with random labels
            t = np.concatenate([prior_box_as_target(pri, k % P) for k in range(64)], 0)
            t[:, 4] = rng.integers(0, C - 1, size=64)
            return t
        tg = [many(), rand_boxes(rng, 1, C), many()][:B]
    elif name == 'special':
        conf = (np.round(conf * 4) / 4).astype(np.float32)
        a = rand_boxes(rng, 1, C)
        a2 = a.copy()
        a2[0, 4] = C - 2            # two identical boxes: the later one wins the forced prior (and, with C = 3, its other label shows it)
        tg = [np.concatenate([a, a2, rand_boxes(rng, 1, C)], 0),
              np.concatenate([prior_box_as_target(pri, P // 2), FAR], 0),       # IoU exactly 1; a box that overlaps nothing
              FAR.copy()][:B]
    else:
        raise KeyError(name)
    return loc, conf, tg


def bits_equal(a, b, view):
    return torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def assert_same_state(st_f, st_s, what):
    assert bits_equal(st_f['loc_t'], st_s['loc_t'], torch.int32), f'{what}: loc_t'
    assert torch.equal(st_f['conf_t'], st_s['conf_t']), f'{what}: conf_t'
    assert torch.equal(st_f['sel'], st_s['sel']), f'{what}: sel'
    assert bits_equal(st_f['partial'], st_s['partial'], torch.int64), f'{what}: partial'
    assert bits_equal(st_f['losses'], st_s['losses'], torch.int32), f'{what}: losses {st_f["losses"]} {st_s["losses"]}'
    assert bits_equal(st_f['n_total'], st_s['n_total'], torch.int64), f'{what}: n_total'
    assert (st_f['loss_c_all'] is None) == (st_s['loss_c_all'] is None)
    if st_f['loss_c_all'] is not None:
        assert bits_equal(st_f['loss_c_all'], st_s['loss_c_all'], torch.int32), f'{what}: loss_c_all'


# P: 1 (P - 1 = 0 negatives), just over a wave, just over the 1024-thread block, no multiple of the slice count, the real prior count
CASES = [(P, B, C, 'rand') for P in (1, 65, 1025, 2500, 8732) for B, C in ((1, 2), (3, 3), (1, 3), (3, 2))]
CASES += [(P, 3, C, name) for P, C in ((1, 2), (65, 3), (1025, 2), (2500, 3), (8732, 2))
          for name in ('empty_all', 'zeros', 'quant', 'many64', 'special')]
CASES += [(8732, 3, 3, 'special'), (65, 1, 2, 'many64'), (8732, 1, 3, 'many64')]


@pytest.mark.parametrize('P,B,C,name', CASES)
def test_fused_loss_matches_launch_sequence(dev, ops, P, B, C, name):
    loc, conf, tg = scenario(name, P, B, C, seed=1000 + 7 * P + 3 * B + C)
    pri = torch.from_numpy(priors(P)).to(dev)
    loc_d, conf_d = torch.from_numpy(loc).to(dev), torch.from_numpy(conf).to(dev)
    tgp, ngt = ops.pack_targets([torch.from_numpy(t) for t in tg], dev)
    want = (B + C) % 2 == 1 or name != 'rand'        # loss_c_all is optional: both ways
    st_s = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=want, fused=False)
    st_f = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=want, fused=True)
    assert_same_state(st_f, st_s, 'first call')
    # the same workspace again: the ticket of the last-workgroup hand-over was left zero
    st_f2 = ops.multibox_loss_forward(loc_d, conf_d, pri, tgp, ngt, want_scores=want, fused=True)
    assert_same_state(st_f2, st_s, 'second call')
    if name == 'empty_all':
        assert not torch.isfinite(st_f['losses']).any() and float(st_f['n_total']) == 0.0
    if name == 'many64' and P == 65:
        assert (st_f['partial'][:, 3] == P - 1).any() and (st_f['partial'][:, 2] >= 64).any()      # 3 x positives > P - 1: num_neg clipped
    if name == 'special' and B == 3 and P > 1:
        ct = st_f['conf_t'].cpu().numpy()
        assert ct[1, P // 2] == 1 and ct[1, 0] == 1 and ct[2, 0] == 1 and (ct[2, 1:] == 0).all()
        if P == 8732:
            assert (ct[0] == C - 1).sum() >= 1                       # the later twin owns the forced prior


def test_heads_reduce2_matches_two_launches(dev):
    from gssd._lib import check, lib
    stream = torch.cuda.current_stream().cuda_stream
    B, P = 2, 37
    g = torch.Generator().manual_seed(11)
    for C in (4, 2):
        splits = torch.randint(1, 4, (P,), generator=g).to(torch.int8).to(dev)
        ws_loc = torch.randn(3, B, P, 4, generator=g).to(dev)
        ws_conf = torch.randn(3, B, P, C, generator=g).to(dev)
        ref_l, ref_c = torch.full((B, P, 4), 7., device=dev), torch.full((B, P, C), 7., device=dev)
        got_l, got_c = torch.full((B, P, 4), 9., device=dev), torch.full((B, P, C), 9., device=dev)
        check(lib.gssd_heads_reduce_f32(ws_loc.data_ptr(), splits.data_ptr(), ref_l.data_ptr(), B, P, 4, stream))
        check(lib.gssd_heads_reduce_f32(ws_conf.data_ptr(), splits.data_ptr(), ref_c.data_ptr(), B, P, C, stream))
        check(lib.gssd_heads_reduce2_f32(ws_loc.data_ptr(), ws_conf.data_ptr(), splits.data_ptr(), got_l.data_ptr(), got_c.data_ptr(),
                                         B, P, C, stream))
        assert bits_equal(got_l, ref_l, torch.int32) and bits_equal(got_c, ref_c, torch.int32), C
        # and the sum itself: slices 0 .. splits[p] - 1 in order
        exp = ws_conf[0].clone()
        for k in (1, 2):
            m = (splits.long() > k).view(1, P, 1)
            exp = torch.where(m, exp + ws_conf[k], exp)
        assert torch.equal(got_c, exp)


def test_module_fused_and_unfused_agree(dev, golden):
    from layers.modules import MultiBoxLoss
    g = golden('loss')
    pri_np = priors(8732)
    pri = torch.from_numpy(pri_np).to(dev)
    P = pri_np.shape[0]
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    for ci in range(3):
        rng = np.random.default_rng(int(g[f'seed{ci}']))
        loc = rng.normal(0, 1.0, size=(4, P, 4)).astype(np.float32)
        conf = rng.normal(0, 2.0, size=(4, P, 2)).astype(np.float32)
        tg = [torch.from_numpy(g[f'tg{ci}_{b}']) for b in range(4)]
        res = []
        for fused in (True, False):
            loc_d = torch.from_numpy(loc).to(dev).requires_grad_()
            conf_d = torch.from_numpy(conf).to(dev).requires_grad_()
            ll, lc = crit((loc_d, conf_d, pri), tg, fused=fused)
            (ll + lc).backward()
            res.append((ll.detach(), lc.detach(), loc_d.grad, conf_d.grad))
        for a, b in zip(*res):
            assert torch.equal(a, b), ci


def test_plan_heads_reduce_switch(tmp_path):
    """GSSD_FUSE_HEADS_REDUCE unset (one launch) and 0 (two launches): the same (loc, conf) from the train-mode forward of the gssd config."""
    outs = {}
    for tag, env in (('one', {}), ('two', {'GSSD_FUSE_HEADS_REDUCE': '0'})):
        path = str(tmp_path / f'{tag}.npz')
        e = {k: v for k, v in os.environ.items() if k != 'GSSD_FUSE_HEADS_REDUCE'}
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'heads_reduce_worker.py'), path], capture_output=True, text=True,
                           timeout=600, env=dict(e, **env))
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = np.load(path)
    assert (int(outs['one']['one']), int(outs['one']['two'])) == (1, 0) and (int(outs['two']['one']), int(outs['two']['two'])) == (0, 2)
    for k in ('loc', 'conf'):
        assert np.array_equal(outs['one'][k].view(np.int32), outs['two'][k].view(np.int32)), k
