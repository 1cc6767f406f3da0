"""Generates tests/golden/pixellink2s.npz from the IMPORTED reference with pixel_link_config.version = "2s" (run in the build container
only; the reference does not travel):  python tests/golden/make_pixellink2s_golden.py

  model_<v>_*  PixelLink forward (train mode, B = 1) on the seeded synthetic weights / image of gssd.synth for the variants of
               tests/pixellink2s_ref.py (plain: cascade_fuse + fuse + BN; sa: SA + SA-base; sapool: max_pool_factor 2; nocascade: no
               cascade, no fuse conv); cv2 is an empty import stub (not on a numeric path).  Full out_1 for plain / sa, every third row
               and column of it for the others; out_2 on every fifth row and column; the state-dict key:shape list in order; bn_fuse1's
               running mean; self_attn_list.0's theta weight_u.
  loss_*       criterion.PixelLinkLoss on pixellink2s_ref.loss_inputs(11) (150 x 150; an image without positives, exact ties at the
               OHEM threshold): the four losses, neg_area, the mined mask (bit-packed).
  dec_*        postprocess.func label maps on pixellink2s_ref.decode_inputs(21) (thresholded like mask_to_box; uint8 in the reference).
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG                     # noqa: E402  (import_reference: stubs + sys.path handling)
from gssd import synth                       # noqa: E402
import pixellink2s_ref as R2                 # noqa: E402

warnings.filterwarnings('ignore')


def main():
    MG.import_reference()
    import pixel_link.pixel_link_config as ref_config
    from pixel_link import model as ref_model, criterion as ref_crit, postprocess as ref_post
    assert "reference" in ref_model.__file__ and "reference" in ref_config.__file__, ref_model.__file__
    ref_config.version = "2s"
    out = {}
    for tag, (kw, mpf) in R2.VARIANTS.items():
        torch.manual_seed(7)
        net = ref_model.PixelLink(**kw, max_pool_factor=mpf)
        sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=2222)
        net.load_state_dict(sd)
        net.train()
        x = synth.synth_images(1, seed=300)
        with torch.no_grad():
            o1, o2 = net(x)
        full = tag in ('plain', 'sa')
        out[f'model_{tag}_out1'] = o1.numpy() if full else o1.numpy()[:, :, ::3, ::3]
        out[f'model_{tag}_out2s'] = o2.numpy()[:, :, ::5, ::5]
        out[f'model_{tag}_shape'] = np.array([list(o1.shape), list(o2.shape)], np.int64)
        after = net.state_dict()
        out[f'model_{tag}_keys'] = np.array([f'{k}:{"x".join(map(str, v.shape))}' for k, v in after.items()])
        if kw['use_fuseconv'] and kw['batch_norm']:
            out[f'model_{tag}_bn_fuse1_rm'] = after['bn_fuse1.running_mean'].numpy()
        if kw['use_self_attention']:
            out[f'model_{tag}_sa0_u'] = after['self_attn_list.0.snconv1x1_theta.weight_u'].numpy()
        print(tag, tuple(o1.shape), tuple(o2.shape), float(o1.abs().max()), float(o2.abs().max()))
    o1, o2, pix, neg, posw, link = R2.loss_inputs(11)
    crit = ref_crit.PixelLinkLoss()
    pp, pn = crit.pixel_loss(torch.from_numpy(o1), torch.from_numpy(pix), torch.from_numpy(neg), torch.from_numpy(posw))
    lp, ln = crit.link_loss(torch.from_numpy(o2), torch.from_numpy(link))
    out.update(loss_vals=np.array([float(pp), float(pn), float(lp), float(ln)], np.float64),
               loss_neg_weight_bits=np.packbits(crit.neg_pixel_weight.numpy().astype(bool)), loss_neg_area=crit.neg_area.numpy())
    print('loss', out['loss_vals'], out['loss_neg_area'])
    d1, d2 = R2.decode_inputs(21)
    t1, t2 = torch.from_numpy(d1), torch.from_numpy(d2)
    pixc = torch.softmax(t1, 1)[:, 1] > 0.2
    labels = []
    for b in range(d1.shape[0]):
        ln_ = torch.stack([(torch.softmax(t2[b:b + 1, 2 * n:2 * n + 2], 1)[0, 1] > 0.8) & pixc[b] for n in range(8)]).to(torch.uint8)
        labels.append(ref_post.func(pixc[b].to(torch.uint8), ln_).astype(np.uint8))
    out.update(dec_labels_u8=np.stack(labels))
    print('decode: max label (uint8)', [int(l.max()) for l in labels])
    np.savez_compressed(os.path.join(HERE, 'pixellink2s.npz'), **out)


if __name__ == '__main__':
    main()
