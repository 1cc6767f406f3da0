"""The o conv of Self_Attn-base 0 writing slice_and_cat's result itself (csrc/conv_x6.hip, GSSD_CONV_OUT_GROUPCAT) against the two-launch form
it replaces in plans that no backward reads: the o conv with separate `out` (x + sigma o) / `out2` (sigma o) maps, then
gssd_slice_and_cat_f32.  The epilogue computes the same values and only stores them elsewhere, and no atomics are involved, so the
concatenated map must be equal BIT FOR BIT.  Plan level: GSSD_FUSE_CAT=0 (plan_common.FUSE_CAT) restores the copy launch (-1 step); plans whose
o conv the kernel declines (M = B * 38 * 38 < 4096), grad-enabled plans and the bf16 storage mode keep it."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'grouped-ssd-pytorch_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('B', [3, 32])
@pytest.mark.parametrize('f16', [False, True])
def test_o_conv_writes_the_group_concatenation(B, f16):
    """The bench shape (38 x 38 map, 256 -> 512 channels, 4 trunk groups) at a small batch and at batch 32; bf16- and fp16-plane forms."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    H, Cc, C2, G = 38, 512, 256, 4
    ga = Cc // G
    gen = torch.Generator(device='cpu').manual_seed(100 + B)
    ag = torch.randn(B, H, H, C2, generator=gen).to(dev)
    x = torch.randn(B, H, H, Cc, generator=gen).to(dev)
    w = (torch.randn(Cc, C2, generator=gen) * 0.1).to(dev)
    bias, alpha = torch.randn(Cc, generator=gen).to(dev), (torch.rand(Cc, generator=gen) + 0.5).to(dev)
    gate = torch.tensor([0.37], device=dev)
    bn = ops.x6_tile(Cc, 1, B * H * H)
    w6 = ops.x6_weight(w, 1, C2, 1, bn)
    kw = dict(B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, bias=bias, alpha=alpha, gate=gate, resid=x, wgt_x6=w6)
    fl = _lib.CONV_F16_OK if f16 else 0
    out = torch.full((B, H, H, Cc), float('nan'), device=dev)
    out2 = torch.full((B, H, H, Cc), float('nan'), device=dev)
    d0, _, _ = ops.make_conv_desc(ag, w, out, out2=out2, flags=fl, **kw)
    assert lib.gssd_conv_x6_takes(C.byref(d0)) == 1
    _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d0), st))
    ref = torch.full((B, H, H, 2 * Cc), float('nan'), device=dev)
    _lib.check(lib.gssd_slice_and_cat_f32(out.data_ptr(), out2.data_ptr(), ref.data_ptr(), B * H * H, Cc, Cc, G, st))
    xc = torch.full((B, H, H, 2 * Cc), float('nan'), device=dev)
    d1, _, _ = ops.make_conv_desc(ag, w, xc, out2=xc.view(-1)[ga:], out_stride=2 * Cc, split_n=ga, flags=fl | _lib.CONV_OUT_GROUPCAT, **kw)
    assert lib.gssd_conv_x6_takes(C.byref(d1)) == 1
    _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d1), st))
    torch.cuda.synchronize()
    assert torch.isfinite(ref).all() and torch.isfinite(xc).all()
    assert torch.equal(xc, ref), f'max |d| {float((xc - ref).abs().max()):.3e}'
    v = xc.view(B, H, H, G, 2, ga)
    assert torch.equal(v[:, :, :, :, 0].reshape(B, H, H, Cc), out) and torch.equal(v[:, :, :, :, 1].reshape(B, H, H, Cc), out2)


def test_groupcat_flag_is_refused_elsewhere():
    """A descriptor with the flag that csrc/conv_x6.hip declines (no packed planes; a slab that is no multiple of 8) is an error."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    B, H, Cc, C2 = 1, 38, 512, 256
    ag, x, xc = torch.zeros(B, H, H, C2, device=dev), torch.zeros(B, H, H, Cc, device=dev), torch.zeros(B, H, H, 2 * Cc, device=dev)
    w = torch.zeros(Cc, C2, device=dev)
    w6 = ops.x6_weight(w, 1, C2, 1, ops.x6_tile(Cc, 1, B * H * H))
    gate = torch.ones(1, device=dev)
    kw = dict(B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, gate=gate, resid=x, out_stride=2 * Cc, flags=_lib.CONV_OUT_GROUPCAT)
    for extra in (dict(split_n=128, out2=xc.view(-1)[128:]), dict(split_n=4, out2=xc.view(-1)[4:], wgt_x6=w6),
                  dict(split_n=128, out2=xc.view(-1)[128:], wgt_x6=w6, out_stride=Cc)):
        d, _, _ = ops.make_conv_desc(ag, w, xc, **{**kw, **extra})
        assert lib.gssd_conv_x6_takes(C.byref(d)) == 0
        assert lib.gssd_conv2d_nhwc_f32(C.byref(d), st) == -1
    torch.cuda.synchronize()


def _gssdpp(dev):
    from gssd import synth
    from models.ssd_multiphase_custom_group import build_ssd
    args = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)         # GSSD++
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    return net.to(dev).train()


def test_switch_restores_the_copy_launch(monkeypatch):
    from gssd import _lib, plan_common, synth
    lib = _lib.lib
    dev = torch.device('cuda:0')
    x = synth.synth_images(4, seed=9).to(dev)

    def ncat(plan):
        return sum(1 for s in plan.steps if s.fn is lib.gssd_slice_and_cat_f32)
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(plan_common, 'FUSE_CAT', fuse)
        net = _gssdpp(dev)
        with torch.no_grad():
            outs = [tuple(t.clone() for t in net(x)[:2]) for _ in range(4)]      # eager runs, then the captured graphs
        plan = net._engine._last_plan
        assert plan.nograd
        res[fuse] = (len(plan.steps), ncat(plan), outs)
    assert res[True][1] == 0 and res[False][1] == 1 and res[True][0] == res[False][0] - 1
    # no atomics between the o conv and the DCN: the same bits both ways wherever the rest of the step is run-to-run identical; the batch sums
    # of later BatchNorm layers are fp64 atomics, so allow their last-bit flips (tests/test_gpu_fused_pack.py's reasoning)
    for (l1, c1), (l0, c0) in zip(res[True][2], res[False][2]):
        dl = float((l1 - l0).abs().max() / l0.abs().max())
        dc = float((c1 - c0).abs().max() / c0.abs().max())
        print(f'fused vs copy launch, whole forward: loc {dl:.2e} conf {dc:.2e} (relative to the tensor max)')
        assert dl < 1e-5 and dc < 1e-5
    monkeypatch.setattr(plan_common, 'FUSE_CAT', True)
    net = _gssdpp(dev)
    with torch.no_grad():
        net(x[:2])                                     # M = 2 * 38 * 38 < 4096: the o conv stays with the implicit GEMM, the copy stays
    assert ncat(net._engine._last_plan) == 1
    net(x)                                             # a backward reads the separate maps
    assert not net._engine._last_plan.nograd and ncat(net._engine._last_plan) == 1
    net.compute_dtype = 'bf16'
    with torch.no_grad():
        net(x)
    assert ncat(net._engine._last_plan) == 1
