"""The merged theta | phi | g projection of a 38 x 38 Self_Attn block writing the attention core's bf16 planes itself (csrc/conv_x6.hip,
GSSD_CONV_OUT_X6PLANES) against the two-pass form it replaces in plans that no backward reads: the projection with fp32 outputs, then
gssd_self_attn_core_x6_f32, whose first pass splits them into the planes.  The epilogue computes the same values and splits them with the same
function, and no atomics are involved, so the planes -- the never-written zero key columns [N, Np32) and the images that straddle a row tile
included -- and the core's output must be equal BIT FOR BIT.  Plan level: GSSD_FUSE_SPLIT=0 (plan_common.FUSE_SPLIT) restores the two-pass
entry; grad-enabled, bf16, want_maps and small-M plans keep it."""
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


def _ws_views(ws, B, N, C4, C2):
    """(theta | phi planes [3][B][N][C4], g^T planes [3][B][C2][Np32]) of a workspace of 16-bit words."""
    Np32 = (N + 31) // 32 * 32
    ntp = 3 * B * N * C4
    return ws[:ntp].view(3, B, N, C4), ws[ntp:ntp + 3 * B * C2 * Np32].view(3, B, C2, Np32)


@pytest.mark.parametrize('B', [3, 32])
@pytest.mark.parametrize('f16', [False, True])
def test_projection_writes_the_core_planes(B, f16):
    """The bench shape (38 x 38 map, 512 -> 128 | 256 channels) at a small batch and at batch 32; bf16- and fp16-plane products of the projection."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    H, Cc = 38, 512
    N, C8, C4, C2 = H * H, Cc // 8, Cc // 4, Cc // 2
    Np32 = (N + 31) // 32 * 32
    assert N % 128 != 0 and N % 32 != 0                  # images straddle the 128-row tiles, their last 32-block is ragged
    gen = torch.Generator(device='cpu').manual_seed(300 + B)
    x = torch.randn(B, H, H, Cc, generator=gen).abs().to(dev)
    w = (torch.randn(C4 + C2, Cc, generator=gen) * 0.05).to(dev)
    bias, alpha = torch.randn(C4 + C2, generator=gen).to(dev), (torch.rand(C4 + C2, generator=gen) + 0.5).to(dev)
    bn = ops.x6_tile(C4 + C2, 1, B * N)
    w6 = ops.x6_weight(w, 1, Cc, 1, bn)
    fl = _lib.CONV_OUT_F32 | (_lib.CONV_F16_OK if f16 else 0)
    kw = dict(B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C4 + C2, bias=bias, alpha=alpha, wgt_x6=w6, out_mode=_lib.OUT_SPLIT_T, split_n=C4,
              out_stride=C4, in_batch_stride=N * Cc, out_batch_stride=N * C4)
    words = int(lib.gssd_self_attn_core_x6_ws_bytes(B, N, C8, C2)) // 2
    # reference: fp32 projection outputs, then the two-pass core
    tp = torch.full((B, N, C4), float('nan'), device=dev)
    gT = torch.zeros(B, C2, N, device=dev)
    d0, _, _ = ops.make_conv_desc(x, w, tp, out_b=gT, out_b_stride=N, outb_batch_stride=C2 * N, flags=fl, **kw)
    assert lib.gssd_conv_x6_takes(C.byref(d0)) == 1
    _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d0), st))
    ws0 = torch.full((words,), -1, device=dev, dtype=torch.int16)
    out0, lse0 = torch.full((B, N, C2), float('nan'), device=dev), torch.full((B, N), float('nan'), device=dev)
    _lib.check(lib.gssd_self_attn_core_x6_f32(tp.data_ptr(), gT.data_ptr(), out0.data_ptr(), B, N, N, C8, C2, ws0.data_ptr(), lse0.data_ptr(), st))
    # fused: planes from the projection's epilogue into a NaN-filled workspace (0x7fc0 = bf16 NaN) whose key tails are zero, as the plan leaves them
    ws1 = torch.full((words,), 0x7fc0, device=dev, dtype=torch.int16)
    _ws_views(ws1, B, N, C4, C2)[1][..., N:] = 0
    d1, _, _ = ops.make_conv_desc(x, w, ws1, out_b=ws1[3 * B * N * C4:], out_b_stride=Np32, outb_batch_stride=C2 * Np32,
                                  flags=fl | _lib.CONV_OUT_X6PLANES, **kw)
    assert lib.gssd_conv_x6_takes(C.byref(d1)) == 1
    _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d1), st))
    out1, lse1 = torch.full((B, N, C2), float('nan'), device=dev), torch.full((B, N), float('nan'), device=dev)
    _lib.check(lib.gssd_self_attn_core_x6_planes_f32(ws1.data_ptr(), out1.data_ptr(), B, N, C8, C2, lse1.data_ptr(), st))
    torch.cuda.synchronize()
    t0, g0 = _ws_views(ws0, B, N, C4, C2)
    t1, g1 = _ws_views(ws1, B, N, C4, C2)
    assert torch.equal(t1, t0), f'theta | phi planes differ in {int((t1 != t0).sum())} words'
    assert torch.equal(g1, g0), f'g^T planes differ in {int((g1 != g0).sum())} words'
    assert int(g1[..., N:].abs().max()) == 0
    assert torch.equal(ws1, ws0)
    assert torch.isfinite(out0).all() and torch.isfinite(out1).all()
    assert torch.equal(out1, out0), f'max |d| {float((out1 - out0).abs().max()):.3e}'
    assert torch.equal(lse1, lse0)


def test_x6planes_flag_is_refused_elsewhere():
    """A descriptor with the flag that csrc/conv_x6.hip declines (no packed planes; a split that is no tile multiple; key rows that are no
    whole 32-blocks; a residual) is an error."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    B, H, Cc = 1, 38, 512
    N, C8, C4, C2 = H * H, Cc // 8, Cc // 4, Cc // 2
    Np32 = (N + 31) // 32 * 32
    x, w = torch.zeros(B, H, H, Cc, device=dev), torch.zeros(C4 + C2, Cc, device=dev)
    w6 = ops.x6_weight(w, 1, Cc, 1, ops.x6_tile(C4 + C2, 1, B * N))
    ws = torch.zeros(int(lib.gssd_self_attn_core_x6_ws_bytes(B, N, C8, C2)) // 2, device=dev, dtype=torch.int16)
    resid = torch.zeros(B, N, C4 + C2, device=dev)
    kw = dict(B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C4 + C2, out_mode=_lib.OUT_SPLIT_T, split_n=C4, out_stride=C4, out_b=ws[3 * B * N * C4:],
              out_b_stride=Np32, outb_batch_stride=C2 * Np32, flags=_lib.CONV_OUT_F32 | _lib.CONV_OUT_X6PLANES, wgt_x6=w6)
    d, _, _ = ops.make_conv_desc(x, w, ws, **kw)
    assert lib.gssd_conv_x6_takes(C.byref(d)) == 1
    for extra in (dict(wgt_x6=None), dict(split_n=C4 - 32, out_stride=C4 - 32), dict(out_b_stride=N, outb_batch_stride=C2 * N), dict(resid=resid),
                  dict(out_mode=_lib.OUT_NHWC)):
        d, _, _ = ops.make_conv_desc(x, w, ws, **{**kw, **extra})
        assert lib.gssd_conv_x6_takes(C.byref(d)) == 0, extra
        assert lib.gssd_conv2d_nhwc_f32(C.byref(d), st) == -1, extra
    d, _, _ = ops.make_conv_desc(x, w, ws, **kw)
    assert lib.gssd_conv2d_nhwc_bf16(C.byref(d), st) == -1          # fp32 entry point only
    torch.cuda.synchronize()


def _gssdpp(dev):
    from gssd import synth
    from models.ssd_multiphase_custom_group import build_ssd
    args = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)         # GSSD++
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    return net.to(dev).train()


def test_switch_restores_the_two_pass_core(monkeypatch):
    from gssd import _lib, plan_common, synth
    lib = _lib.lib
    dev = torch.device('cuda:0')
    x = synth.synth_images(4, seed=9).to(dev)

    def cores(plan):
        return (sum(1 for s in plan.steps if s.fn is lib.gssd_self_attn_core_x6_planes_f32),
                sum(1 for s in plan.steps if s.fn is lib.gssd_self_attn_core_x6_f32))
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(plan_common, 'FUSE_SPLIT', fuse)
        net = _gssdpp(dev)
        with torch.no_grad():
            outs = [tuple(t.clone() for t in net(x)[:2]) for _ in range(4)]      # eager runs, then the captured graphs
        plan = net._engine._last_plan
        assert plan.nograd
        bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        res[fuse] = (len(plan.steps), cores(plan), outs, [(m.running_mean.clone(), m.running_var.clone()) for m in bns])
    # the two 38 x 38 blocks (Self_Attn-base 0, Self_Attn 0) switch entries; the launch list keeps its length (the split was inside the entry)
    assert res[True][1] == (2, 0) and res[False][1] == (0, 2) and res[True][0] == res[False][0]
    # the planes are the same bits both ways; the batch sums of later BatchNorm layers are fp64 atomics, so allow their last-bit flips
    # (tests/test_gpu_fused_pack.py's reasoning)
    for (l1, c1), (l0, c0) in zip(res[True][2], res[False][2]):
        dl = float((l1 - l0).abs().max() / l0.abs().max())
        dc = float((c1 - c0).abs().max() / c0.abs().max())
        print(f'fused vs two-pass core, whole forward: loc {dl:.2e} conf {dc:.2e} (relative to the tensor max)')
        assert dl < 1e-5 and dc < 1e-5
    for (m1, v1), (m0, v0) in zip(res[True][3], res[False][3]):      # running statistics after the 4 steps
        dm = float((m1 - m0).abs().max() / m0.abs().max().clamp_min(1e-30))
        dv = float((v1 - v0).abs().max() / v0.abs().max().clamp_min(1e-30))
        assert dm < 1e-5 and dv < 1e-5, (dm, dv)
    monkeypatch.setattr(plan_common, 'FUSE_SPLIT', True)
    net = _gssdpp(dev)
    with torch.no_grad():
        net(x[:2])                                     # M = 2 * 38 * 38 < 4096: the projection stays with the implicit GEMM
    assert cores(net._engine._last_plan)[0] == 0
    net(x)                                             # a backward reads the fp32 theta | phi and g^T
    assert not net._engine._last_plan.nograd and cores(net._engine._last_plan) == (0, 2)
    with torch.no_grad():
        net(x, visualize=True)                         # the attention map's logits GEMM reads the fp32 theta | phi
    assert net._engine._last_plan.want_maps and cores(net._engine._last_plan) == (0, 2)
    net.compute_dtype = 'bf16'
    with torch.no_grad():
        net(x)
    assert cores(net._engine._last_plan) == (0, 0)
