"""Device SSDAugmentation at the training geometry: B = 32 raw uint8 [4, 512, 512, 3] studies -> [32, 12, 300, 300] fp32.

Prints one JSON line: device ms per 32-study batch (events around `--iters` batches, each with fresh random draws, so every
batch has its own crop / expand / mirror geometry), the three passes' share, and the host planner's ms per batch (the only CPU
work left).  For comparison: the reference's per-study numpy / Pillow SSDAugmentation(0.01, 1.5, 300, [49] * 3,
use_normalize=True) measured 35 ms per study on one core of the build host (numpy 2.2, Pillow 12.2), i.e. about 1.1 s of
CPU per 32-study batch.

    python scripts/bench_augment.py [--iters 50] [--warmup 5]
"""
import argparse
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'grouped-ssd-pytorch_amd'))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from gssd import synth                                   # noqa: E402
from gssd.augment import DeviceSSDAugmentation, _as_studies  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    studies = [synth.synth_study_u8(900 + i, 4, 512) for i in range(4)]
    raw = torch.from_numpy(np.stack([studies[i % 4] for i in range(a.batch)])).to(dev)
    box = np.array([[0.30, 0.35, 0.55, 0.60, 1.], [0.45, 0.40, 0.70, 0.75, 1.]], np.float32)
    targets = [box] * a.batch
    aug = DeviceSSDAugmentation(0.01, 1.5, 300, (49, 49, 49), use_normalize=True)
    py, npr = random.Random(0), np.random.RandomState(0)
    out = torch.empty(a.batch, 12, 300, 300, device=dev)
    for _ in range(a.warmup):
        aug(raw, targets, out=out, py_rng=py, np_rng=npr)
    torch.cuda.synchronize()
    # host planner alone
    t0 = time.perf_counter()
    for _ in range(a.iters):
        aug.plan([(512, 512)] * a.batch, targets, py, npr)
    plan_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    # whole call (planner + descriptors + three launches), device time between events
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        aug(raw, targets, out=out, py_rng=py, np_rng=npr)
    host_ms = (time.perf_counter() - t0) * 1e3 / a.iters
    e1.record()
    torch.cuda.synchronize()
    call_ms = e0.elapsed_time(e1) / a.iters
    # device passes alone, on pre-made plans (no host gaps between batches)
    studies_t = _as_studies(raw)
    plans = [aug.plan([(512, 512)] * a.batch, targets, py, npr) for _ in range(a.iters)]
    aug.run(studies_t, plans[0], out)
    torch.cuda.synchronize()
    e0.record()
    for p in plans:
        aug.run(studies_t, p, out)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / a.iters
    print(json.dumps(dict(metric='augment_ms_per_batch', batch=a.batch, src=512, size=300, iters=a.iters,
                          device_ms=round(dev_ms, 4), call_ms=round(call_ms, 4), host_ms_per_call=round(host_ms, 3),
                          planner_ms=round(plan_ms, 3), ref_cpu_ms_per_batch_build_host=35.0 * a.batch,
                          gpu=torch.cuda.get_device_name(0))))


if __name__ == '__main__':
    main()
