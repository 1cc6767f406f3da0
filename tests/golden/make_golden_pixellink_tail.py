"""Golden vectors for the PixelLink tail at its edges: what the imported reference computes for the rows of tests/pixellink_tail_cases.py that
it defines.

    loss   : criterion.PixelLinkLoss (pixel_loss + link_loss) for the rows with a candidate in every image and area + neg_area > 0 (its
             topk[-1] raises without a candidate, its means are NaN without a denominator): the four losses, neg_area, the mined mask
    decode : postprocess.func on masks thresholded with the reference's own ops (postprocess.py:97-115; mask_to_box itself needs cv2) for the
             rows with at most 255 components per image (func returns uint8): the label maps

Results only; inputs are not stored: a row is rebuilt from its name and seed.  Nothing from the reference is copied.

    python tests/golden/make_golden_pixellink_tail.py           # rewrites tests/golden/pixellink_tail.npz  (build container only)
    python tests/golden/make_golden_pixellink_tail.py --check   # regenerates and compares with the file: same entries, same contents
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import import_reference      # noqa: E402
import pixellink_tail_cases as K              # noqa: E402


def loss_rows(crit_mod):
    out = {}
    for i, row in enumerate(K.LOSS):
        if not K.reference_defines_loss(i):
            continue
        inp = K.loss_reference(i)['inp']
        t = lambda k: torch.from_numpy(inp[k])
        crit_mod.config.neg_pos_ratio = row.ratio
        crit = crit_mod.PixelLinkLoss()
        pp, pn = crit.pixel_loss(t('out1'), t('pix'), t('neg'), t('posw'))
        lp, ln = crit.link_loss(t('out2'), t('link'))
        crit_mod.config.neg_pos_ratio = K.NEG_POS_RATIO
        mask = crit.neg_pixel_weight.numpy().astype(bool)
        assert np.array_equal(mask, K.loss_reference(i)['mask']), row.name          # the rows leave no decision to rounding
        out[f'loss|{row.name}|vals'] = np.array([float(pp), float(pn), float(lp), float(ln)], np.float64)
        out[f'loss|{row.name}|neg_area'] = crit.neg_area.numpy().astype(np.int32)
        out[f'loss|{row.name}|mask'] = np.packbits(mask)
        print('loss', row.name, out[f'loss|{row.name}|vals'], out[f'loss|{row.name}|neg_area'])
    return out


def decode_rows(post_mod):
    import torch.nn as nn
    out = {}
    for row in K.DECODE:
        if row.error:
            continue
        d = row.build()
        if int(d['labels'].max()) > 255:
            continue
        pthr, lthr = row.thresholds
        o1, o2 = torch.from_numpy(d['out1']), torch.from_numpy(d['out2'])
        pixel_class = nn.Softmax2d()(o1)[:, 1] > pthr
        links = torch.zeros(o2.shape[0], 8, o2.shape[2], o2.shape[3], dtype=torch.uint8)
        for n in range(8):
            links[:, n] = nn.Softmax2d()(o2[:, [2 * n, 2 * n + 1]])[:, 1] > lthr
            links[:, n] = links[:, n] & pixel_class.byte()
        labels = np.stack([post_mod.func(pixel_class[b], links[b]) for b in range(o1.shape[0])])
        assert labels.dtype == np.uint8
        out[f'decode|{row.name}|labels'] = labels
        print('decode', row.name, [int(l.max()) for l in labels], 'as built' if np.array_equal(labels, d['labels']) else 'DIFFERS from the row')
    return out


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import_reference()
    from pixel_link import criterion as ref_crit, postprocess as ref_post
    assert 'reference' in ref_crit.__file__ or 'ssd_liverdet' in ref_crit.__file__, ref_crit.__file__
    out = {}
    out.update(loss_rows(ref_crit))
    out.update(decode_rows(ref_post))
    path = os.path.join(HERE, 'pixellink_tail.npz')
    if '--check' in sys.argv:
        old = np.load(path, allow_pickle=False)
        assert sorted(old.files) == sorted(out), set(old.files) ^ set(out)
        for k in out:
            a, b = old[k], np.asarray(out[k])
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8) if a.dtype.kind == 'f' else a,
                                                                                 b.view(np.uint8) if b.dtype.kind == 'f' else b), k
        print('pixellink_tail.npz: same contents')
        return
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
