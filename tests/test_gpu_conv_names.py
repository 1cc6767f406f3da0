"""The kernel-instance names of every conv launch, as gssd_conv2d_kernel_name (the dispatchers' own statement) gives them, against the
names the commit before it produced with a Python restatement of the dispatch (tests/data/conv_names_parent.json: layer, name, algorithmic
FLOPs and bytes of every tagged conv step, in plan order, dumped from that commit with collect() below).  bench.py and the committed
profiles match on these strings."""
import json
import os

import pytest
import torch

import pixel_link.pixel_link_config as pl_config
from gssd import _lib, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'data', 'conv_names_parent.json')
GSSD = (True, 4, 4, 1, True, False, False, 0, 1, False, False, 1)
GSSDPP = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)
PIXELLINK = dict(cascade_fuse=True, use_fuseconv=True, batch_norm=True, use_self_attention=True, use_self_attention_base=True,
                 num_dcn_layers=1, groups_dcn=4, dcn_cat_sab=True, detach_sab=False)
PIXELLINK_2S = dict(PIXELLINK, num_dcn_layers=0, groups_dcn=1, dcn_cat_sab=False)          # version "2s" is defined without DCN layers
CONFIGS = ('vanilla', 'gssd', 'gssdpp', 'gssdpp_bf16', 'pixellink4s', 'pixellink2s')      # BASELINE.json configs 0 - 4, PixelLink 4s / 2s
BATCHES = (4, 8, 24, 32)                                                                   # where tests/test_gpu_switches.py sees selection flip

# (config, batch, layer) -> the library's name, where the parent's restatement named a kernel that did not run.  Every entry
# needs the kernel symbol of a kernel trace of that configuration in the commit message that adds it; empty for default switches.
MIRROR_WAS_WRONG = {}


def build_net(config):
    if config == 'vanilla':
        from models.ssd import build_ssd
        net, seed = build_ssd('train', 300, 2), 1111
    elif config.startswith('pixellink'):
        from pixel_link.model import PixelLink
        pl_config.version = '2s' if config.endswith('2s') else '4s'
        try:
            net, seed = PixelLink(**(PIXELLINK_2S if config.endswith('2s') else PIXELLINK)), 2222
        finally:
            pl_config.version = '4s'
    else:
        from models.ssd_multiphase_custom_group import build_ssd
        net, seed = build_ssd('train', 300, 2, *(GSSD if config == 'gssd' else GSSDPP)), 1111
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=seed))
    net = net.cuda().train()
    if config.endswith('_bf16'):
        net.compute_dtype = 'bf16'
    return net


def collect(config, batch):
    """{'nograd' | 'grad': [[layer, name, flops, bytes] of every tagged conv step, in plan order]} of one train-mode forward each."""
    net = build_net(config)
    x = synth.synth_images(batch, seed=7, channels=3 if config == 'vanilla' else 12).cuda()
    out = {}
    for mode in ('nograd', 'grad'):
        with torch.set_grad_enabled(mode == 'grad'):
            net(x)
        plan = net._engine._last_plan
        out[mode] = [[st.tag.layer, st.tag[0], st.tag[1], st.tag[2]] for st in plan.steps
                     if st.fn in (_lib.lib.gssd_conv2d_nhwc_f32, _lib.lib.gssd_conv2d_nhwc_bf16)]
    del net, plan
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope='module')
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize('batch', BATCHES)
@pytest.mark.parametrize('config', CONFIGS)
def test_conv_names_match_parent(parent, config, batch):
    got = collect(config, batch)
    for mode in ('nograd', 'grad'):
        want = [list(r) for r in parent[f'{config}/{batch}/{mode}']]
        for r in want:
            r[1] = MIRROR_WAS_WRONG.get((config, batch, r[0]), r[1])
        assert len(got[mode]) == len(want) and len(want) > 10, (mode, len(got[mode]), len(want))
        diff = [(g, w) for g, w in zip(got[mode], want) if g != w]
        assert not diff, (mode, diff[:8])
