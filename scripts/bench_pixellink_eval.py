"""The box tail of PixelLink's evaluation at the evaluation batch (B = 32, 300 x 300 destination): device against host.

For 75 x 75 ("4s") and 150 x 150 ("2s") score maps, seeded like tests/pixellink2s_ref.decode_inputs (blobs of positives, links mostly on),
prints one JSON line with
  device_ms   `mask_to_box_device` (link decoding + gssd_pixellink_boxes_f32 + its one read of the component counts): device time, events
              around `--iters` back-to-back calls after `--warmup`,
  boxes_ms    of that, the box-tail launch alone (`component_boxes_device` on the decoded label maps),
  host_ms     the existing `mask_to_box` (the same decoding, then the numpy tail on the host): wall time of one call,
and the number of detections both return (the two lists are compared: same boxes, scores within 1e-6).

    python scripts/bench_pixellink_eval.py [--iters 300] [--warmup 10] [--batch 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'))
import numpy as np      # noqa: E402
import torch            # noqa: E402


def seeded_maps(seed, B, H):
    rng = np.random.default_rng(seed)
    d1 = rng.normal(0, 1.0, size=(B, 2, H, H)).astype(np.float32)
    blob = rng.random((B, H // 5, H // 5)) > 0.75                          # 5 x 5 blocks of positives
    d1[:, 1] += np.where(np.kron(blob, np.ones((5, 5), bool)), 3.0, -6.0).astype(np.float32)
    d2 = rng.normal(0, 2.5, size=(B, 16, H, H)).astype(np.float32)
    d2[:, 1::2] += 2.5                                                     # links mostly on
    return d1, d2


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    from pixel_link import postprocess
    dev = torch.device('cuda:0')
    out = {}
    for H in (75, 150):
        o1, o2 = (torch.from_numpy(t).to(dev) for t in seeded_maps(600 + H, a.batch, H))
        labels, _, ncomp = postprocess.decode(o1, o2)
        t_dev = timed(lambda: postprocess.mask_to_box_device(o1, o2), a.iters, a.warmup)
        t_box = timed(lambda: postprocess.component_boxes_device(labels, o1, ncomp=ncomp), a.iters, a.warmup)
        det, ndet = postprocess.mask_to_box_device(o1, o2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = postprocess.mask_to_box(o1, o2)
        t_host = (time.perf_counter() - t0) * 1e3
        det, ndet = det[:, 1].cpu().numpy(), ndet.cpu().numpy()
        for b, rows in enumerate(host):
            ref = np.asarray(rows, np.float64).reshape(-1, 5)
            assert int(ndet[b]) == len(ref) and np.array_equal(det[b, :len(ref), 1:], ref[:, 1:]), b
            assert len(ref) == 0 or np.abs(det[b, :len(ref), 0] - ref[:, 0]).max() <= 1e-6, b
        out[f'{H}x{H}'] = dict(device_ms=round(t_dev, 3), boxes_ms=round(t_box, 3), host_ms=round(t_host, 1),
                               components=int(ncomp.sum()), detections=int(ndet.sum()))
    print(json.dumps(dict(bench='pixellink_eval_box_tail', batch=a.batch, dst=[300, 300], maps=out)), flush=True)


if __name__ == '__main__':
    main()
