"""The PixelLink branch of the reference's evaluation entry point (ssd_liverdet/test_ap_iobb.py:231-328 ``test_net`` with
``use_pixel_link=True``, i.e. ``make_pred`` :99-111) on the device: the network's score maps are link-decoded and boxed on the MI355X
(``pixel_link.postprocess.mask_to_box_device``) and scored by ``gssd.evaluator.DeviceEvaluator``.

    from pixel_link.evaluate import test_net          # instead of: from test_ap_iobb import test_net
    ap, iobb = test_net(net, True, testset, transform, 300, thresh=0.5, mode='v2', use_pixel_link=True)

``test_net`` here takes the reference's arguments (plus ``batch_size``, like ``test_ap_iobb.test_net``); without ``use_pixel_link`` it hands
the call to ``test_ap_iobb.test_net`` unchanged, so a driver can import this one name for both model families.  Per batch it reads B integers
twice (the component counts and the detection counts): the reference skips an image without any detection BEFORE counting its ground truth."""
import numpy as np
import torch

from gssd._lib import GssdError
from gssd.evaluator import DeviceEvaluator
from pixel_link.postprocess import mask_to_box_device


def test_net(net, cuda, testset, transform, imsize=300, thresh=0.05, mode='v1', use_07_metric=True, ap_list=[0.5],
             iobb_list=[0.1], writer=None, iteration=None, visualize=False, output_path=None, model_name=None,
             use_pixel_link=False, batch_size=32):
    """Two quirks of the reference are kept: ``thresh`` is the pixel threshold of the decoding AND the later ``score > thresh`` filter; an
    image without any detection is skipped before its ground truth is counted (:107-108), one whose detections all fall below ``thresh``
    is not.  Boxes are in network pixels already, so the evaluator's scales are ones and the ground truth is brought to network pixels
    (annotation * s / img.shape[-2], :100)."""
    if not use_pixel_link:
        import test_ap_iobb
        return test_ap_iobb.test_net(net, cuda, testset, transform, imsize, thresh, mode, use_07_metric, ap_list, iobb_list, writer,
                                     iteration, visualize, output_path, model_name, False, batch_size)
    if visualize:                                       # the reference fails here with an unbound name (:122, :163): nothing is defined
        raise GssdError('test_net: visualize=True is not defined for use_pixel_link=True')
    ev = DeviceEvaluator(thresh, ap_list, iobb_list, use_07_metric)
    n = len(testset)
    for start in range(0, n, batch_size):
        idxs = range(start, min(n, start + batch_size))
        imgs = [testset.pull_image(i) for i in idxs]
        xs = [torch.as_tensor(transform(im)[0]) for im in imgs]                 # [4, s, s, 3] each (device or host)
        x = torch.stack(xs).cuda().float().permute(0, 1, 4, 2, 3)
        x = x.reshape(x.shape[0], -1, x.shape[3], x.shape[4]).contiguous()      # [B, 12, s, s]
        s = x.shape[-1]
        annos = [np.asarray(testset.pull_anno(i), np.float64) * s / im.shape[-2] for i, im in zip(idxs, imgs)]
        with torch.no_grad():
            pixel_pos, link_pos = net(x)
        # rows by descending score: the evaluator's greedy matching walks an image's rows in order, as the reference's global sort does
        det, ndet = mask_to_box_device(pixel_pos, link_pos, img_shape=(s, s), pixel_thres=thresh, by_score=True)
        found = ndet.cpu().numpy() > 0
        if mode == 'v1':
            gts = [a[2:3, :-1] for a in annos]                                  # portal-phase box only (:185)
        else:
            gts = [a[:, :-1] for a in annos]
        gts = [g if f else np.zeros((0, 4)) for g, f in zip(gts, found)]
        ev.add_batch(det, np.ones((len(imgs), 4), np.float32), gts)
    return ev.result()


test_net.__test__ = False        # a library entry point that keeps the reference's name, not a pytest case
