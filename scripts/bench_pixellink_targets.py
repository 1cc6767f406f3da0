"""Device PixelLink targets at the training geometry: B = 32 images of 0..20 random boxes, size 300, versions "4s" and "2s".

Prints one JSON line per version: the kernel's device time per 32-image batch (events around `--iters` back-to-back launches on
staged inputs, after `--warmup`), the device time of whole prepare_targets calls on device boxes (join + offsets upload + launch),
and the host wall time per prepare_targets call from CPU boxes (packing, pinned staging, upload, launch; no sync).  For comparison:
the reference's PreparePixelLinkTargets with the test fixture's stand-in raster took 38 ms ("4s") and 111 ms ("2s") of one
build-host core for the fixture's 32-image random batch (325 boxes), before the int64 masks are copied to the device.

    python scripts/bench_pixellink_targets.py [--iters 200] [--warmup 20]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'grouped-ssd-pytorch_amd'))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from gssd import pixellink_targets as PT      # noqa: E402


def boxes_batch(rng, B):
    out = []
    for _ in range(B):
        n = int(rng.integers(0, 21))
        cx, cy = rng.uniform(-0.1, 1.1, n), rng.uniform(-0.1, 1.1, n)
        w, h = rng.uniform(0.02, 0.4, n), rng.uniform(0.02, 0.4, n)
        out.append(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, np.zeros(n)], 1).astype(np.float32))
    return out


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    host = (time.perf_counter() - t0) / iters
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, host * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=300)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    boxes = boxes_batch(np.random.default_rng(0), a.batch)
    dev_boxes = [torch.from_numpy(b).to(dev) for b in boxes]
    packed, offs = PT.pack_boxes(boxes)
    buf, head = PT.staging(packed, offs)
    staged = torch.from_numpy(buf).to(dev)
    for v in ('4s', '2s'):
        kernel = lambda: PT.launch(staged.data_ptr() + head, staged.data_ptr(), a.batch, a.size, v, dev)   # noqa: E731
        from_dev = lambda: PT.prepare_targets(dev_boxes, a.size, v)                                       # noqa: E731
        from_cpu = lambda: PT.prepare_targets(boxes, a.size, v, device=dev)                              # noqa: E731
        for fn in (kernel, from_dev, from_cpu):
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        k_ms, _ = timed(kernel, a.iters)
        d_ms, d_host = timed(from_dev, a.iters)
        c_ms, c_host = timed(from_cpu, a.iters)
        M = PT.mask_side(a.size, v)
        out_mb = a.batch * M * M * (8 + 8 + 4 + 8 * 8) / 1e6
        print(json.dumps(dict(metric='pixellink_targets', version=v, batch=a.batch, size=a.size, M=M, boxes=int(packed.shape[0]),
                              iters=a.iters, kernel_us=round(k_ms * 1e3, 2), device_boxes_call_us=round(d_ms * 1e3, 2),
                              device_boxes_host_us=round(d_host * 1e3, 1), cpu_boxes_call_us=round(c_ms * 1e3, 2),
                              cpu_boxes_host_us=round(c_host * 1e3, 1), out_mb=round(out_mb, 2),
                              out_gbps=round(out_mb / 1e3 / (k_ms / 1e3), 1), gpu=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
