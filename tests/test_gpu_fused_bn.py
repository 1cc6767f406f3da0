"""BatchNorm + ReLU passes of a no-backward fp32 plan folded into the launches that read their output, against the pass + launch they replace:
  * conv4_3's pass -> Self_Attn-base 0: the projection reads the raw map through in_scale / in_shift (an existing form), the o conv's
    residual read through GSSD_CONV_RESID_XF (csrc/conv_x6.hip, plain and GSSD_CONV_OUT_GROUPCAT epilogues);
  * the passes behind the fuse convs with <= 512 channels -> their merged loc | conf head conv (in_scale / in_shift / in_pad together with the
    GSSD_OUT_HEADS epilogue: csrc/conv_wino_x6.hip on the 38 x 38 map, csrc/conv_igemm.hip with reduction slices elsewhere).
Scale and shift come from gssd_bn_finalize_f32, which computes them with the pass's expression, and every reader applies max(v * scale + shift, 0)
like the pass: the results must be equal BIT FOR BIT (the heads' reduction slices are plain stores).  Plan level: GSSD_FUSE_SA_BN=0 /
GSSD_FUSE_HEAD_BN=0 (plan_common) restore the passes (1 / 5 of them, each in place of a bn_finalize launch); grad-enabled, bf16, want_maps and small-M plans keep them."""
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


def _bn_both_ways(raw, gen, tail=True):
    """Train-mode BatchNorm + ReLU of the NHWC map ``raw`` both ways: (activated map from the pass, raw copy with the pad vector right behind it as
    the plan allocates it, scale, shift, pad)."""
    from gssd import _lib
    lib = _lib.lib
    dev, st = raw.device, torch.cuda.current_stream().cuda_stream
    B, H, W, Cc = raw.shape
    gamma = (torch.randn(Cc, generator=gen) * 0.5 + 1.0).to(dev)
    gamma[3], gamma[Cc - 5] = -0.7, -1.3
    beta = torch.randn(Cc, generator=gen).to(dev)
    rd = raw.double().view(-1, Cc)
    stats = torch.cat([rd.sum(0), (rd * rd).sum(0)]).contiguous()
    act = torch.full_like(raw, float('nan'))
    rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
    _lib.check(lib.gssd_bn_relu_pool_f32(raw.data_ptr(), act.data_ptr(), B, H, W, Cc, H, W, 0, 1, 0, stats.data_ptr(), float(B * H * W),
                                         gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, 1, 1, 1, st))
    flat = torch.empty(raw.numel() + Cc, device=dev)
    flat[:raw.numel()] = raw.reshape(-1)
    raw2, pd = flat[:raw.numel()].view(B, H, W, Cc), flat[raw.numel():]
    if not tail:
        pd = torch.empty(Cc, device=dev)
    sc, sh = torch.empty(Cc, device=dev), torch.empty(Cc, device=dev)
    rm2, rv2 = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
    _lib.check(lib.gssd_bn_finalize_f32(stats.data_ptr(), float(B * H * W), gamma.data_ptr(), beta.data_ptr(), rm2.data_ptr(), rv2.data_ptr(),
                                        0.1, 1e-5, 1, Cc, sc.data_ptr(), sh.data_ptr(), pd.data_ptr(), 1, st))
    torch.cuda.synchronize()
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2)      # one running-statistics update either way, the same one
    assert float((act == 0).float().mean()) > 0.1             # the ReLU clips
    return act, raw2, sc, sh, pd


@pytest.mark.parametrize('B', [3, 32])
@pytest.mark.parametrize('f16', [False, True])
@pytest.mark.parametrize('gcat', [False, True])
def test_o_conv_applies_bn_relu_to_its_residual(B, f16, gcat):
    """The bench shape (38 x 38 map, 256 -> 512 channels, 4 trunk groups): plain and grouped-concatenation epilogues, bf16- and fp16-plane forms."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    H, Cc, C2, G = 38, 512, 256, 4
    ga = Cc // G
    gen = torch.Generator(device='cpu').manual_seed(500 + B)
    ag = torch.randn(B, H, H, C2, generator=gen).to(dev)
    xr = (torch.randn(B, H, H, Cc, generator=gen) * 3.0 + 0.5).to(dev)
    w = (torch.randn(Cc, C2, generator=gen) * 0.1).to(dev)
    bias, alpha = torch.randn(Cc, generator=gen).to(dev), (torch.rand(Cc, generator=gen) + 0.5).to(dev)
    gate = torch.tensor([0.37], device=dev)
    act, raw, sc, sh, pd = _bn_both_ways(xr, gen)
    w6 = ops.x6_weight(w, 1, C2, 1, ops.x6_tile(Cc, 1, B * H * H))
    kw = dict(B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, bias=bias, alpha=alpha, gate=gate, wgt_x6=w6)
    fl = (_lib.CONV_F16_OK if f16 else 0) | (_lib.CONV_OUT_GROUPCAT if gcat else 0)
    res = []
    for resid, extra in ((act, {}), (raw, dict(in_scale=sc, in_shift=sh, in_pad=pd))):
        fx = fl | (_lib.CONV_RESID_XF if extra else 0)
        if gcat:
            xc = torch.full((B, H, H, 2 * Cc), float('nan'), device=dev)
            d, _, _ = ops.make_conv_desc(ag, w, xc, out2=xc.view(-1)[ga:], out_stride=2 * Cc, split_n=ga, resid=resid, flags=fx, **kw, **extra)
            outs = (xc,)
        else:
            out, out2 = torch.full((B, H, H, Cc), float('nan'), device=dev), torch.full((B, H, H, Cc), float('nan'), device=dev)
            d, _, _ = ops.make_conv_desc(ag, w, out, out2=out2, resid=resid, flags=fx, **kw, **extra)
            outs = (out, out2)
        assert lib.gssd_conv_x6_takes(C.byref(d)) == 1
        _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d), st))
        res.append(outs)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b), f'max |d| {float((a - b).abs().max()):.3e}'


def test_resid_transform_is_refused_elsewhere():
    """Only csrc/conv_x6.hip has the epilogue: a descriptor with GSSD_CONV_RESID_XF that it declines (no packed planes, no scale / shift, no
    residual, a transposed output) is an error, never a silently untransformed residual."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    B, H, Cc, C2 = 1, 38, 512, 256
    ag, x, out = torch.zeros(B, H, H, C2, device=dev), torch.zeros(B, H, H, Cc, device=dev), torch.zeros(B, H, H, Cc, device=dev)
    w = torch.zeros(Cc, C2, device=dev)
    w6 = ops.x6_weight(w, 1, C2, 1, ops.x6_tile(Cc, 1, B * H * H))
    sc, sh, pd = torch.ones(Cc, device=dev), torch.zeros(Cc, device=dev), torch.zeros(Cc, device=dev)
    xf = dict(in_scale=sc, in_shift=sh, in_pad=pd)
    kw = dict(B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, flags=_lib.CONV_RESID_XF)
    d, _, _ = ops.make_conv_desc(ag, w, out, resid=x, wgt_x6=w6, **kw, **xf)
    assert lib.gssd_conv_x6_takes(C.byref(d)) == 1
    for extra in (dict(resid=x, **xf), dict(resid=x, wgt_x6=w6), dict(wgt_x6=w6, **xf)):
        d, _, _ = ops.make_conv_desc(ag, w, out, **kw, **extra)
        assert lib.gssd_conv_x6_takes(C.byref(d)) == 0, list(extra)
        assert lib.gssd_conv2d_nhwc_f32(C.byref(d), st) == -1, list(extra)
    d, _, _ = ops.make_conv_desc(ag, w, out, resid=x, wgt_x6=w6, **kw, **xf)
    assert lib.gssd_conv2d_nhwc_bf16(C.byref(d), st) == -1
    torch.cuda.synchronize()


HEADS = [
    # B, H, Cs, anchors, Winograd (csrc/conv_wino_x6.hip) or implicit GEMM with reduction slices (csrc/conv_igemm.hip)
    (32, 38, 512, 4, True),      # the 38 x 38 head at the bench batch
    (4, 10, 512, 6, False),      # the 10 x 10 head
    (4, 3, 256, 4, False),       # a tail head: every output pixel touches the padding ring
]


@pytest.mark.parametrize('case', HEADS)
def test_head_applies_bn_relu_to_its_input(case):
    from gssd import ops, _lib
    lib = _lib.lib
    B, H, Cs, A, wino = case
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    nc = 2
    nloc, nconf, P = 4 * A, nc * A, H * H * A
    gen = torch.Generator(device='cpu').manual_seed(700 + H)
    xr = (torch.randn(B, H, H, Cs, generator=gen) * 2.0 + 0.3).to(dev)
    w = (torch.randn(nloc + nconf, Cs, 3, 3, generator=gen) * 0.05).to(dev)
    bias = torch.randn(nloc + nconf, generator=gen).to(dev)
    act, raw, sc, sh, pd = _bn_both_ways(xr, gen)
    wp = ops.pack_weight(w)
    K = wp.shape[1]
    U, split, fl = None, ops.auto_split_k(B * H * H, nloc + nconf, 1, K), _lib.CONV_OUT_F32 | _lib.CONV_HEADS_SLICES
    if wino:
        U, split, fl = ops.winograd_weight(wp, 1, Cs), 1, fl | _lib.CONV_F16_OK
    res = []
    for inp, extra in ((act, {}), (raw, dict(in_scale=sc, in_shift=sh, in_pad=pd))):
        loc = torch.full((split, B, P, 4), float('nan'), device=dev)
        conf = torch.full((split, B, P, nc), float('nan'), device=dev)
        d, _, _ = ops.make_conv_desc(inp, wp, loc, B=B, H=H, W=H, in_stride=Cs, cin_g=Cs, Cout=nloc + nconf, k=3, pad=1, bias=bias,
                                     out_mode=_lib.OUT_HEADS, out_b=conf, split_n=nloc, out_batch_stride=P * 4, outb_batch_stride=P * nc,
                                     split_k=split, wgt_wino=U, flags=fl, **extra)
        assert lib.gssd_conv_wino_x6_takes(C.byref(d)) == int(wino)
        _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d), st))
        res.append((loc, conf))
    torch.cuda.synchronize()
    assert split > 1 or wino
    for a, b in zip(*res):
        assert torch.isfinite(a).all() and torch.isfinite(b).all()
        assert torch.equal(a, b), f'{case}: max |d| {float((a - b).abs().max()):.3e}'


def _gssdpp(dev):
    from gssd import synth
    from models.ssd_multiphase_custom_group import build_ssd
    args = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)         # GSSD++
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    return net.to(dev).train()


@pytest.mark.parametrize('switch,removed', [('FUSE_SA_BN', 1), ('FUSE_HEAD_BN', 5)])
def test_switch_restores_the_bn_passes(monkeypatch, switch, removed):
    from gssd import _lib, plan_common, synth
    lib = _lib.lib
    dev = torch.device('cuda:0')
    x = synth.synth_images(4, seed=9).to(dev)

    def npass(plan):      # BatchNorm passes proper (stand-alone pools carry no statistics pointer)
        return sum(1 for s in plan.steps if s.fn is lib.gssd_bn_relu_pool_f32 and s.args[11] != 0)
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(plan_common, switch, fuse)
        net = _gssdpp(dev)
        with torch.no_grad():
            outs = [tuple(t.clone() for t in net(x)[:2]) for _ in range(3)]      # eager runs, then the captured graph
        plan = net._engine._last_plan
        assert plan.nograd
        bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        nfin = sum(1 for s in plan.steps if s.fn is lib.gssd_bn_finalize_f32)
        res[fuse] = (len(plan.steps), npass(plan), outs, [(m.running_mean.clone(), m.running_var.clone()) for m in bns], nfin)
    # every removed pass over a map leaves the layer's bn_finalize launch (C channels: scale / shift / pad and the running-statistics update)
    assert res[True][1] == res[False][1] - removed and res[True][4] == res[False][4] + removed and res[True][0] == res[False][0], \
        (res[True][:2], res[False][:2])
    # the folded forms are bit-identical launch by launch; the batch sums of later BatchNorm layers are fp64 atomics, so allow their last-bit
    # flips (tests/test_gpu_fused_pack.py's reasoning)
    for (l1, c1), (l0, c0) in zip(res[True][2], res[False][2]):
        dl = float((l1 - l0).abs().max() / l0.abs().max())
        dc = float((c1 - c0).abs().max() / c0.abs().max())
        print(f'{switch} on vs off, whole forward: loc {dl:.2e} conf {dc:.2e} (relative to the tensor max)')
        assert dl < 1e-5 and dc < 1e-5
    worst = 0.0
    for (m1, v1), (m0, v0) in zip(res[True][3], res[False][3]):      # running statistics after 3 steps: every momentum update happened once
        worst = max(worst, float((m1 - m0).abs().max() / m0.abs().max().clamp_min(1e-30)), float((v1 - v0).abs().max() / v0.abs().max()))
    print(f'{switch} on vs off, running statistics after 3 steps: {worst:.2e} (relative to the tensor max)')
    assert worst < 1e-5
    n_off = res[False][1]

    def seq(plan):        # the launch sequence: entry point of every step, and whether a conv carries a fused input transform
        return [(s.fn.__name__, bool(s.tag.desc.in_scale) if (s.tag is not None and getattr(s.tag, 'desc', None) is not None) else None)
                for s in plan.steps]

    def plans(fuse):      # the plans that must NOT fold: want_maps, grad-enabled, bf16 storage
        monkeypatch.setattr(plan_common, switch, fuse)
        net = _gssdpp(dev)
        out = {}
        with torch.no_grad():
            net(x, visualize=True)                     # want_maps: activated maps stay
        assert net._engine._last_plan.want_maps
        out['want_maps'] = net._engine._last_plan
        net(x)                                         # a backward reads the activated maps
        assert not net._engine._last_plan.nograd
        out['grad'] = net._engine._last_plan
        if fuse and switch == 'FUSE_SA_BN':
            with torch.no_grad():
                net(x[:2])                             # M = 2 * 38 * 38 < 4096: the block's launches stay with the implicit GEMM, the pass stays
            assert npass(net._engine._last_plan) == n_off
        net.compute_dtype = 'bf16'
        with torch.no_grad():
            net(x)
        assert net._engine._last_plan.bf16
        out['bf16'] = net._engine._last_plan
        return out
    on, off = plans(True), plans(False)
    for k in on:
        assert seq(on[k]) == seq(off[k]), k            # the same launches, the same fused input transforms: the switch changes nothing there
    n_none = n_off + (5 if switch == 'FUSE_SA_BN' else 1)      # neither kind folded (the other switch is at its default, on)
    assert npass(on['want_maps']) == n_none
    assert sum(1 for s in on['bf16'].steps if s.fn is lib.gssd_bn_relu_pool_bf16 and s.args[11] != 0) == \
        sum(1 for s in off['bf16'].steps if s.fn is lib.gssd_bn_relu_pool_bf16 and s.args[11] != 0)
