"""Golden vectors for the index kernels at their edges: what the imported reference computes for the rows of
tests/index_kernel_cases.py whose scores are pairwise distinct (ties are not the reference's to define: see that file).

    Detect / NMS : Detect.apply and box_utils.decode + box_utils.nms per (image, class): kept prior indices whole, the five
                   values of a spread of kept rows
    MultiBoxLoss : box_utils.match, MultiBoxLoss(C, ...) and its mining restated with the reference's own ops; for the tie rows only
                   conf_t, the positives, num_neg and the two losses; for the backward rows the gradients
    evaluator    : test_net through a fake dataset / transform / network that replay the row's Detect output

Inputs are not stored: a row is rebuilt from its name and seed.  Nothing from the reference is copied.

    python tests/golden/make_golden_index_edges.py           # rewrites tests/golden/index_edges.npz  (build container only)
    python tests/golden/make_golden_index_edges.py --check   # regenerates and compares with the file: same entries, same contents
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference      # noqa: E402
import index_kernel_cases as K                # noqa: E402


def detect_rows(R):
    rows = {}
    for r in K.DETECT:
        if not r.fixture:
            continue
        inp, prm = r.build(), r.params
        sc = K.det_scores(inp)                # Detect's contract takes the softmaxed scores (detection_pytorch_ver_1point5.py:33)
        B, P, C = sc.shape
        pri = torch.from_numpy(K.priors(P))
        out = R.Detect.apply(C, 0, prm['top_k'], prm['conf_thresh'], prm['nms_thresh'], torch.from_numpy(inp['loc']),
                             torch.from_numpy(sc), pri).numpy()
        cnt, keep, pos, val = np.zeros((B, C), np.int16), [], [], []
        for b in range(B):
            boxes = R.box_utils.decode(torch.from_numpy(inp['loc'][b]), pri, [0.1, 0.2])
            for cl in range(1, C):
                s = torch.from_numpy(sc[b, :, cl])
                m = s.gt(prm['conf_thresh'])
                if int(m.sum()) == 0:
                    continue
                ids, n = R.box_utils.nms(boxes[m.unsqueeze(1).expand_as(boxes)].view(-1, 4), s[m], prm['nms_thresh'], prm['top_k'])
                k = torch.nonzero(m).view(-1)[ids[:n]].numpy()
                assert np.array_equal(out[b, cl, :n, 0], sc[b, k, cl]) and (out[b, cl, n:] == 0).all(), r.name
                cnt[b, cl] = n
                keep.append(k.astype(np.int16))
                at = K.sample_positions(int(n))
                pos.append(at.astype(np.int16))
                val.append(out[b, cl, at])
        assert (out[:, 0] == 0).all()
        rows[r.name] = dict(cnt=cnt, keep=np.concatenate(keep) if keep else np.zeros(0, np.int16),
                            val=np.concatenate(val) if val else np.zeros((0, 5), np.float32))
        print('detect', r.name, cnt[:, 1:].ravel())
    return rows


def nms_rows(R):
    rows = {}
    for r in K.NMS:
        inp, prm = r.build(), r.params
        ids, n = R.box_utils.nms(torch.from_numpy(inp['boxes']), torch.from_numpy(inp['scores']), prm['overlap'], prm['top_k'])
        rows[r.name] = dict(keep=ids[:n].numpy().astype(np.int16))
        print('nms', r.name, int(n))
    return rows


def loss_rows(R):
    rows = {}
    for r in K.LOSS:
        if r.name in K.LOSS_ORACLE_ONLY:
            continue
        inp, prm = r.build(), r.params
        B, P, C = inp['conf'].shape
        pri = torch.from_numpy(K.priors(P))
        crit = R.MultiBoxLoss(C, 0.5, True, 0, True, 3, 0.5, False, False)
        tg = [torch.from_numpy(t) for t in inp['targets']]
        loc_v, conf_v = torch.from_numpy(inp['loc']).requires_grad_(), torch.from_numpy(inp['conf']).requires_grad_()
        ll, lc = crit((loc_v, conf_v, pri), tg)
        # the reference's matching and mining with its own ops (multibox_loss.py:67-72, :91-106)
        conf_t, loc_t = torch.zeros(B, P, dtype=torch.long), torch.zeros(B, P, 4)
        for b in range(B):
            R.box_utils.match(0.5, tg[b][:, :-1], pri, [0.1, 0.2], tg[b][:, -1], loc_t, conf_t, b)
        bc = torch.from_numpy(inp['conf']).view(-1, C)
        lca = R.box_utils.log_sum_exp(bc) - bc.gather(1, conf_t.view(-1, 1))
        pos = conf_t > 0
        lca[pos.view(-1, 1)] = 0
        _, li = lca.view(B, -1).sort(1, descending=True)
        _, rk = li.sort(1)
        nneg = torch.clamp(3 * pos.long().sum(1, keepdim=True), max=P - 1)
        d = dict(losses=np.array([ll.item(), lc.item()], np.float64), conf_t=conf_t.numpy().astype(np.int8),
                 pos=np.packbits(pos.numpy()), num_neg=nneg[:, 0].numpy().astype(np.int32))
        if r.fixture:
            d['neg'] = np.packbits((rk < nneg).numpy())
            d['loc_t_pos'] = loc_t.numpy()[pos.numpy()]
        if prm.get('backward'):
            for name, gl, gc in K.GRADS:
                loc_g, conf_g = torch.from_numpy(inp['loc']).requires_grad_(), torch.from_numpy(inp['conf']).requires_grad_()
                l2, c2 = crit((loc_g, conf_g, pri), tg)
                (gl * l2 + (0. if gc is None else gc) * c2).backward()
                d[f'dloc_{name}'], d[f'dconf_{name}'] = loc_g.grad.numpy(), conf_g.grad.numpy()
        rows[r.name] = d
        print('loss', r.name, d['losses'], d['num_neg'])
    return rows


def eval_rows(R):
    import test_ap_iobb as T
    rows = {}
    for r in K.EVAL:
        if not r.fixture:
            continue
        inp, prm = r.build(), r.params
        det, gts, scales = inp['det'], inp['gts'], inp['scales']
        state = {'i': 0}

        class FakeSet:
            name = 'lesion_test_ap_synth'

            def __len__(self):
                return det.shape[0]

            def pull_image(self, idx):                       # test_net reads the scale off the image: (W, H) = shape[2], shape[1]
                return np.zeros((4, int(scales[idx][1]), int(scales[idx][0]), 3), np.uint8)

            def pull_anno(self, idx):
                return np.concatenate([gts[idx], np.zeros((gts[idx].shape[0], 1))], axis=1)

        def transform(img):
            return (np.zeros((4, 8, 8, 3), np.float32),)

        def net(x):
            i = state['i']
            state['i'] += 1
            return torch.from_numpy(det[i:i + 1])

        d = {}
        for use07 in (True, False):
            state['i'] = 0
            with warnings.catch_warnings(), np.errstate(all='ignore'):
                warnings.simplefilter('ignore')
                ap, iobb = T.test_net(net, False, FakeSet(), transform, 300, thresh=prm['thresh'], mode='v2', use_07_metric=use07,
                                      ap_list=list(prm['ap_list']), iobb_list=list(prm['iobb_list']))
            d[f'ap_{int(use07)}'] = np.array(list(ap) + list(iobb), np.float64)
        rows[r.name] = d
        print('eval', r.name, d)
    return rows


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    R = import_reference()
    out = {}
    for prefix, fn in (('detect', detect_rows), ('nms', nms_rows), ('loss', loss_rows), ('eval', eval_rows)):
        out.update(K.pack_rows(prefix, fn(R)))
    path = os.path.join(HERE, 'index_edges.npz')
    if '--check' in sys.argv:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(out), set(old.files) ^ set(out)
        for k in out:
            assert old[k].dtype == np.asarray(out[k]).dtype and np.array_equal(old[k].view(np.uint8) if old[k].dtype.kind == 'f' else old[k],
                                                                              np.asarray(out[k]).view(np.uint8) if old[k].dtype.kind == 'f' else out[k]), k
        print('index_edges.npz: same contents')
        return
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
