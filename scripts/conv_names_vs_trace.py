"""Conv instance names of the GSSD++ plan at batch 32 (gssd_conv2d_kernel_name, the tags bench.py groups by) against the kernel symbols of a
`rocprofv3 --kernel-trace --stats` run of the benchmark's command:  python scripts/conv_names_vs_trace.py f32 STATS.csv  (GPU box; also bf16).
Per instance: launches per step the plan's tags name | launches per step the trace shows (calls / forwards; forwards = calls of the one
heads-reduce launch per step)."""
import collections, csv, os, re, sys
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd')); sys.path.insert(0, ROOT)
import torch
from gssd import synth, _lib
from models.ssd_multiphase_custom_group import build_ssd

dtype, stats = sys.argv[1], sys.argv[2]


def b(v):
    return v == 'true'


def instance(sym):
    """kernel symbol -> the instance name its launch site reports (None: not a kernel of the two conv entry points)"""
    m = re.search(r'::(conv_\w+_kernel|conv_igemm_kernel|gemm_slot_kernel)(?:<([^>]*)>)?\(', sym)
    if not m:
        return None
    k, a = m.group(1), [x.strip() for x in (m.group(2) or '').split(',')]
    sfx = lambda xf, pool: ('' if xf else '/plain') + ('/pool2' if pool else '')
    if k == 'conv_igemm_kernel': return f'conv_igemm<{a[0]}x{a[1]}>'
    if k == 'conv_bf16_kernel': return f'conv_bf16<{a[0]}x{a[1]}>'
    if k == 'gemm_slot_kernel': return f'gemm_slot<128x{a[0]}>'
    if k in ('conv_x6_kernel', 'conv_x6_v2_kernel'): return f'conv_x6<{a[0]}>'
    if k == 'conv_patch_x6_kernel': return 'conv_patch_x6<128>'
    if k == 'conv_thin_kernel': return f'conv_thin<{a[0]},{a[1]}>'
    if k == 'conv_thin_wino_kernel': return 'conv_thin_wino<16,16>'
    if k == 'conv_thin_x6_kernel': return f'conv_thin_x6<{a[0]},{a[1]}>' + sfx(b(a[2]), b(a[3]))
    if k == 'conv_wino_kernel': return f'conv_wino<{a[0]}>' + sfx(b(a[1]), a[3] == '2')
    if k == 'conv_wino_x6_kernel': return f'conv_wino_x6<{16 * int(a[0])}>' + sfx(b(a[1]), a[2] == '2')
    if k == 'conv_thin_bf16_kernel': return f'conv_thin_bf16<{a[0]},{a[1]}>' + ('/pool2' if b(a[4]) else '')
    if k == 'conv_flat_bf16_kernel': return f'conv_flat_bf16<{a[0]},{a[1]},{64 * int(a[4])}>'
    return None


traced, forwards = collections.Counter(), 0
for row in csv.DictReader(open(stats)):
    if 'heads_reduce' in row['Name']:
        forwards += int(row['Calls'])
    name = instance(row['Name'])
    if name:
        traced[name] += int(row['Calls'])

dev = torch.device('cuda:0')
net = build_ssd('train', 300, 2, True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)
net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
net = net.to(dev).train()
if dtype == 'bf16':
    net.compute_dtype = 'bf16'
with torch.no_grad():
    net(synth.synth_images(32, seed=100).to(dev))
tags = collections.Counter(st.tag[0] for st in net._engine._last_plan.steps
                           if st.fn in (_lib.lib.gssd_conv2d_nhwc_f32, _lib.lib.gssd_conv2d_nhwc_bf16))
print(f'GSSD++ {dtype}, batch 32, no-backward plan; trace: {os.path.basename(stats)}, {forwards} forwards')
print(f'{"instance":34s} {"tags / step":>11s} {"traced / step":>13s}')
bad = 0
for name in sorted(set(tags) | set(traced)):
    per = traced[name] / forwards if forwards else float('nan')
    ok = per == tags[name]
    bad += not ok
    print(f'{name:34s} {tags[name]:11d} {per:13.2f}{"" if ok else "   <-- differs"}')
print('every instance agrees' if not bad else f'{bad} instance(s) differ')
