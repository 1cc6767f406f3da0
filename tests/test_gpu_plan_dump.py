"""Everything a forward launch plan will make the GPU do, against what the commit before the plan-constructor refactor built
(tests/data/plan_dump_parent.json: per case the step count and the SHA-256 of dump()'s canonical JSON, written by this file's __main__ on
a checkout of that commit).  dump() touches only what that commit also has, so the same file runs on both trees:

    python3 tests/test_gpu_plan_dump.py --out tests/data/plan_dump_parent.json [--text DIR]

``--text DIR`` also writes every full dump (one JSON file per case) so that a mismatch can be diffed; those texts are not committed."""
import ctypes as C
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == '__main__':
    for _p in (ROOT, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'), os.path.join(ROOT, 'tests')):
        if _p not in sys.path:
            sys.path.insert(0, _p)

from gssd import _lib, synth                                                    # noqa: E402
from test_gpu_conv_names import BATCHES, CONFIGS, build_net                     # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(ROOT, 'tests', 'data', 'plan_dump_parent.json')
CONV_FNS = ('gssd_conv2d_nhwc_f32', 'gssd_conv2d_nhwc_bf16')
PTR_FIELDS = {n for n, t in _lib.ConvDesc._fields_ if t is C.c_void_p}
ADDRESS = 1 << 40          # an integer argument this large is a device address: no shape or count of the project reaches it

# batch 4 only: (case, config or gpu_common.FLAG_NETS name)
EXTRA = ('gssdpp_eval', 'gssdpp_maps', 'nobn', 'nobn_plain')
CASES = [(c, b) for c in CONFIGS for b in BATCHES] + [(c, 4) for c in EXTRA]


class _Ordinals(dict):
    """Device address -> ordinal of its first appearance in the walk: keeps the aliasing structure, forgets the allocator."""

    def __call__(self, ptr):
        if not ptr:
            return 0
        return self.setdefault(int(ptr), len(self) + 1)


def _value(v):
    """A record value: the scalar itself, (shape, dtype) of a tensor, containers element by element, the type's name otherwise."""
    if v is None or isinstance(v, (bool, int, str)):
        return v
    if isinstance(v, float):
        return repr(v)
    if torch.is_tensor(v):
        return [list(v.shape), str(v.dtype)]
    if isinstance(v, (tuple, list)):
        return [_value(e) for e in v]
    return type(v).__name__


def dump(plan, mask_heads_out_f32=False):
    """Canonical, JSON-serialisable description of ``plan``: its steps in order (function, stream id, wait, tag, arguments, conv descriptor),
    its records, the engine's packed weights in registration order and the number of buffers.  ``mask_heads_out_f32``: see VANILLA_HEADS."""
    addr = _Ordinals()
    steps = []
    for st in plan.steps:
        name = st.fn.__name__
        tag = None if st.tag is None else [st.tag[0], repr(float(st.tag[1])), repr(float(st.tag[2])), st.tag.layer]
        args = []
        for a in st.args:
            if isinstance(a, bool) or a is None:
                args.append(a)
            elif isinstance(a, int):
                args.append(['@', addr(a)] if a >= ADDRESS else a)
            elif isinstance(a, float):
                args.append(repr(a))
            else:
                args.append('<' + type(a).__name__ + '>')          # byref(descriptor): the descriptor follows
        desc = None
        if name in CONV_FNS:
            d = st.keep[0] if isinstance(st.keep, tuple) else st.keep
            if not isinstance(d, _lib.ConvDesc):
                d = st.tag.desc
            desc = {}
            for f, _ in _lib.ConvDesc._fields_:
                v = getattr(d, f)
                desc[f] = ['@', addr(v)] if f in PTR_FIELDS else int(v)
            if mask_heads_out_f32 and d.out_mode == _lib.OUT_HEADS:
                desc['flags'] &= ~_lib.CONV_OUT_F32
        steps.append(dict(fn=name, sid=st.sid, wait=st.wait, tag=tag, args=args, desc=desc))
    rec = [[kind, r.get('sid'), [[k, _value(r[k])] for k in sorted(r)]] for kind, r in plan.rec]
    packed = [[k, list(t.shape), str(t.dtype)] for k, t in plan.eng._packed.items()]
    return dict(steps=steps, rec=rec, packed=packed, nbufs=len(plan.bufs))


# The one declared difference.  include/gssd_hip.h requires GSSD_CONV_OUT_F32 with GSSD_OUT_HEADS; the vanilla plan's six head descriptors
# used to omit it (the fp32 entry point never reads the bit) and carry it since they are built by the shared head emitter.  The bit is
# masked on exactly those descriptors, on both trees; their kernel names are part of the dump and must not change.
VANILLA_HEADS = ('vanilla',)


def _summary(d):
    text = json.dumps(d, sort_keys=True, separators=(',', ':'))
    return dict(steps=len(d['steps']), sha256=hashlib.sha256(text.encode()).hexdigest())


def _net_and_input(case, batch):
    from gpu_common import FLAG_NETS
    kw = {}
    if case in ('nobn', 'nobn_plain'):
        from models.ssd_multiphase_custom_group import build_ssd
        net = build_ssd('train', 300, 2, *FLAG_NETS[case][1])
        net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
        net = net.cuda().train()
    elif case == 'gssdpp_eval':
        net = build_net('gssdpp').eval()
    elif case == 'gssdpp_maps':
        net, kw = build_net('gssdpp'), dict(visualize=True)
    else:
        net = build_net(case)
    x = synth.synth_images(batch, seed=7, channels=3 if case == 'vanilla' else 12).cuda()
    return net, x, kw


def collect(case, batch):
    """{'<case>/<batch>/nograd' | '.../grad': dump of the plan of one forward each}."""
    net, x, kw = _net_and_input(case, batch)
    out = {}
    for mode in ('nograd', 'grad'):
        with torch.set_grad_enabled(mode == 'grad'):
            res = net(x, **kw)
        out[f'{case}/{batch}/{mode}'] = dump(net._engine._last_plan, mask_heads_out_f32=case in VANILLA_HEADS)
        del res
    del net
    torch.cuda.empty_cache()
    return out


def collect_self_attn():
    """A stand-alone Self_Attn block, as tests/test_gpu_kernels.py::test_self_attn_op builds it."""
    from gssd.engine import SelfAttnOp
    from gssd.modules import Self_Attn
    dev = torch.device('cuda:0')
    out = {}
    for mode in ('eval', 'train'):
        sa = Self_Attn(64)
        sa.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in sa.state_dict().items()}, seed=21))
        sa = sa.to(dev)
        op = SelfAttnOp(sa, 2, 6, mode == 'train', dev)
        op.run(torch.zeros(2, 6, 6, 64, device=dev))
        out[f'self_attn_op/2/{mode}'] = dump(op)
    return out


@pytest.fixture(scope='module')
def parent():
    with open(FIXTURE) as f:
        return json.load(f)


def _check(parent, got):
    assert got
    for key, d in got.items():
        s = _summary(d)
        print(key, s)
        assert s['steps'] == parent[key]['steps'], (key, s['steps'], parent[key]['steps'])
        assert s['sha256'] == parent[key]['sha256'], key


@pytest.mark.parametrize('case,batch', CASES)
def test_plan_dump_matches_parent(parent, case, batch):
    _check(parent, collect(case, batch))


def test_self_attn_op_dump_matches_parent(parent):
    _check(parent, collect_self_attn())


if __name__ == '__main__':
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=FIXTURE)
    ap.add_argument('--text', default=None, help='directory for the full dumps')
    a = ap.parse_args()
    summary = {}
    if a.text:
        os.makedirs(a.text, exist_ok=True)
    for job in [lambda c=c, b=b: collect(c, b) for c, b in CASES] + [collect_self_attn]:
        for key, d in job().items():
            summary[key] = _summary(d)
            print(key, summary[key], flush=True)
            if a.text:
                with open(os.path.join(a.text, key.replace('/', '_') + '.json'), 'w') as f:
                    json.dump(d, f, sort_keys=True, indent=0)
    with open(a.out, 'w') as f:
        json.dump(summary, f, sort_keys=True, indent=0)
        f.write('\n')
