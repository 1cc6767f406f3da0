"""Subprocess of tests/test_gpu_loss_fused.py: the train-mode forward of the plain GSSD config at batch 2 (no backward); writes loc and conf
to the .npz named by argv[1].  GSSD_FUSE_HEADS_REDUCE is read once per process, at import, so each setting needs a process of its own."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'grouped-ssd-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch
    from gssd import plan_common, synth
    from models.ssd_multiphase_custom_group import build_ssd
    args = (True, 4, 4, 1, True, False, False, 0, 1, False, False, 1)          # tests/gpu_common.py NETS['gssd']
    dev = torch.device('cuda:0')
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    x = synth.synth_images(2, seed=5).to(dev)
    with torch.no_grad():
        loc, conf, _ = net(x)
    fns = [st.fn.__name__ for st in net._engine._last_plan.steps]
    np.savez(sys.argv[1], loc=loc.float().cpu().numpy(), conf=conf.float().cpu().numpy(),
             one=np.int64(fns.count('gssd_heads_reduce2_f32')), two=np.int64(fns.count('gssd_heads_reduce_f32')),
             switch=np.int64(plan_common.FUSE_HEADS_REDUCE))


if __name__ == '__main__':
    main()
