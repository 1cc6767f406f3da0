"""PixelLink version "2s" at the reference driver's batch (B = 16, 300 x 300 inputs, 150 x 150 outputs).

Two configurations: "plain 2s" (cascade_fuse, fuse conv + BatchNorm, no Self_Attn) and "SA 2s" (Self_Attn + Self_Attn-base,
max_pool_factor 1: two 22 500-token attention blocks at stage 1).  For each, prints one JSON line with the device time (events around
`--iters` back-to-back calls after `--warmup`) of
  forward     a no-grad train-mode forward,
  loss_decode PixelLinkLoss (pixel + link, one launch) and the link decoding of the outputs,
  step        a full training step: grad-enabled forward, loss, backward,
and the peak allocation of one training step (torch.cuda.max_memory_allocated, the network's own tensors included).

    python scripts/bench_pixellink2s.py [--iters 5] [--warmup 2] [--batch 16]
"""
import argparse
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'))
import torch            # noqa: E402

import pixel_link.pixel_link_config as config      # noqa: E402
from gssd import synth                             # noqa: E402

CONFIGS = {
    'plain 2s': dict(cascade_fuse=True, use_fuseconv=True, batch_norm=True, use_self_attention=False, use_self_attention_base=False,
                     num_dcn_layers=0, groups_dcn=1, dcn_cat_sab=False, detach_sab=False),
    'SA 2s': dict(cascade_fuse=True, use_fuseconv=True, batch_norm=True, use_self_attention=True, use_self_attention_base=True,
                  num_dcn_layers=0, groups_dcn=1, dcn_cat_sab=False, detach_sab=False),
}


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
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    a = ap.parse_args()
    from pixel_link.model import PixelLink
    from pixel_link.criterion import PixelLinkLoss
    from pixel_link.postprocess import decode
    dev = torch.device('cuda:0')
    B = a.batch
    x = synth.synth_images(B, seed=500).to(dev)
    g = torch.Generator().manual_seed(1)
    pix = (torch.rand(B, 150, 150, generator=g) < 0.05).long().to(dev)
    neg = ((torch.rand(B, 150, 150, generator=g) < 0.9).to(dev) & (pix == 0)).to(torch.uint8)
    posw = (torch.rand(B, 150, 150, generator=g).to(dev) * pix.float()).contiguous()
    link = ((torch.rand(B, 8, 150, 150, generator=g) < 0.5).long().to(dev) * pix[:, None]).contiguous()
    for name, kw in CONFIGS.items():
        config.version = "2s"
        try:
            net = PixelLink(**kw)
        finally:
            config.version = "4s"
        net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=2222))
        net = net.to(dev).train()
        crit = PixelLinkLoss()

        def fwd():
            with torch.no_grad():
                return net(x)
        o1, o2 = fwd()

        def loss_decode():
            with torch.no_grad():
                crit.pixel_loss(o1, pix, neg, posw, link=(o2, link))
                crit.link_loss(o2, link)
                decode(o1, o2)

        def step():
            for p in net.parameters():
                p.grad = None
            q1, q2 = net(x)
            pp, pn = crit.pixel_loss(q1, pix, neg, posw, link=(q2, link))
            lp, ln = crit.link_loss(q2, link)
            (pp + pn + lp + ln).backward()
        t_fwd = timed(fwd, a.iters, a.warmup)
        t_ld = timed(loss_decode, a.iters, a.warmup)
        t_step = timed(step, a.iters, a.warmup)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        print(json.dumps(dict(config=name, batch=B, out_hw=list(o1.shape[2:]), forward_ms=round(t_fwd, 3), loss_decode_ms=round(t_ld, 3),
                              step_ms=round(t_step, 3), step_peak_gib=round(peak / 2 ** 30, 2))), flush=True)
        del net, crit, o1, o2
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
