"""conv1_1 reading the caller's NCHW batch (csrc/conv_thin.hip, GSSD_CONV_IN_NCHW3) against the two-launch form it replaces in plans that no
backward reads: gssd_pack_input_nhwc + the same conv on the packed NHWC copy.

Kernel level: both forms put the same values into the same LDS patch and share the MFMA loop and the epilogue, so the raw output must be
equal BIT FOR BIT.  The batch sums are fp32 partial sums per tile (the same in both forms) added up with fp64 atomics, whose order differs from
launch to launch: each of the n_adds additions into a channel's sum rounds by at most 2^-53 of the running sum, so two launches may differ by
n_adds * 2^-53 * sum |y| (resp. sum y^2) -- that bound (from the number format, not from a run) is the gate for the sums, and the scale / shift
gssd_bn_finalize_f32 derives from them may differ by the fp32 rounding of such a perturbation (one unit in the last place of their terms).

Plan level: the switch GSSD_FUSE_PACK=0 (plan_common.FUSE_PACK) restores the pack launch (-1 step); grad-enabled and bf16 plans keep it."""
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

CASES = [
    # B, H, W            (12 -> 64 channels, 4 groups: conv1_1)
    (2, 300, 300),       # the bench shape at a small batch (300 = 37 * 8 + 4 = 18 * 16 + 12: ragged tiles on both edges)
    (32, 300, 300),      # the bench shape
    (3, 83, 91),         # odd, non-square map
]


@pytest.mark.parametrize('case', CASES)
def test_conv1_1_from_nchw_equals_pack_plus_conv(case):
    from gssd import ops, _lib
    lib = _lib.lib
    B, H, W = case
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device='cpu').manual_seed(B * 1000 + H)
    x = (torch.randn(B, 12, H, W, generator=gen) * 50.0 + 10.0).to(dev)
    w = (torch.randn(64, 3, 3, 3, generator=gen) * 0.2).to(dev)
    b = torch.randn(64, generator=gen).to(dev)
    gamma = (torch.randn(64, generator=gen) * 0.5 + 1.0).to(dev)
    gamma[3], gamma[17] = -0.7, 0.0
    beta = torch.randn(64, generator=gen).to(dev)
    wp = ops.pack_weight(w)
    kw = dict(B=B, H=H, W=W, in_stride=16, cin_g=4, Cout=64, groups=4, k=3, stride=1, pad=1, bias=b)

    def run(inp, flags):
        y = torch.full((B, H, W, 64), float('nan'), device=dev)
        stats = torch.zeros(128, dtype=torch.float64, device=dev)
        d, _, _ = ops.make_conv_desc(inp, wp, y, stats=stats, flags=flags, **kw)
        assert lib.gssd_conv_thin_nchw3_takes(C.byref(d)) == 1
        _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d), st))
        sc, sh, pd = (torch.empty(64, device=dev) for _ in range(3))
        rm, rv = torch.zeros(64, device=dev), torch.ones(64, device=dev)
        _lib.check(lib.gssd_bn_finalize_f32(stats.data_ptr(), float(B * H * W), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                            rv.data_ptr(), 0.1, 1e-5, 1, 64, sc.data_ptr(), sh.data_ptr(), pd.data_ptr(), 0, st))
        torch.cuda.synchronize()
        return y, stats, sc, sh, pd, rm, rv

    packed = ops.pack_input(x, 4, 4)
    assert packed.shape == (B, H, W, 16) and float(packed[..., 3::4].abs().max()) == 0.0
    y0, s0, sc0, sh0, pd0, rm0, rv0 = run(packed, 0)
    y1, s1, sc1, sh1, pd1, rm1, rv1 = run(x, _lib.CONV_IN_NCHW3)
    assert torch.isfinite(y1).all()
    assert torch.equal(y0, y1), f'raw conv1_1 output differs: max {float((y0 - y1).abs().max()):.3e}'
    # the sums against float64 sums of the (identical) raw output: fp32 partial sums per tile bound the kernel's own error
    yd = y1.double().view(-1, 64)
    exact = torch.cat([yd.sum(0), (yd * yd).sum(0)])
    mag = torch.cat([yd.abs().sum(0), (yd * yd).sum(0)])
    tiles = B * ((H + 7) // 8) * ((W + 15) // 16)
    n_adds = 4 * tiles + 768                       # per channel: one LDS add per wave and tile, one global add per workgroup
    bound = n_adds * 2.0 ** -53 * mag
    d01 = (s0 - s1).abs()
    print(f'{case}: batch sums fused vs packed: max |d| / bound {float((d01 / bound).max()):.3f}; vs float64 sums of the output '
          f'{float(((s1 - exact).abs() / mag).max()):.2e} relative')
    assert bool((d01 <= bound).all())
    assert float(((s1 - exact).abs() / mag).max()) < 32 * 2.0 ** -24          # 31 fp32 additions + the square, per tile and lane group
    # derived scale / shift / pad / running statistics: equal up to the fp32 rounding of that perturbation
    ulp = 2.0 ** -23
    mean = s1[:64] / (B * H * W)
    print(f'{case}: scale equal {bool(torch.equal(sc0, sc1))}, shift equal {bool(torch.equal(sh0, sh1))}')
    assert bool(((sc0 - sc1).abs() <= ulp * sc1.abs()).all())
    assert bool(((sh0 - sh1).abs().double() <= 2 * ulp * (beta.abs().double() + (mean * sc1.double()).abs())).all())
    assert torch.equal(pd0, pd1)
    assert bool(((rm0 - rm1).abs() <= ulp * rm1.abs()).all()) and bool(((rv0 - rv1).abs() <= ulp * rv1.abs()).all())


def test_nchw3_flag_is_refused_off_conv1_1():
    """Only the patch-staged kernel reads the layout: a descriptor with the flag that it declines is an error, never a wrong result."""
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(1, 12, 80, 80, device=dev)
    y = torch.zeros(1, 80, 80, 64, device=dev)
    wp = ops.pack_weight(torch.zeros(64, 3, 3, 3, device=dev))
    kw = dict(B=1, H=80, W=80, in_stride=16, cin_g=4, Cout=64, groups=4, k=3, stride=1, pad=1, flags=_lib.CONV_IN_NCHW3)
    for extra in (dict(relu=True), dict(in_scale=torch.ones(16, device=dev), in_shift=torch.zeros(16, device=dev),
                                        in_pad=torch.zeros(16, device=dev))):
        d, _, _ = ops.make_conv_desc(x, wp, y, **{**kw, **extra})
        assert lib.gssd_conv_thin_nchw3_takes(C.byref(d)) == 0
        assert lib.gssd_conv2d_nhwc_f32(C.byref(d), st) == -1
    d, _, _ = ops.make_conv_desc(x, wp, y, **kw)
    assert lib.gssd_conv2d_nhwc_bf16(C.byref(d), st) == -1
    torch.cuda.synchronize()


def _gssdpp(dev):
    from gssd import synth
    from models.ssd_multiphase_custom_group import build_ssd
    args = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)         # GSSD++
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    return net.to(dev).train()


def test_switch_restores_the_pack_launch(monkeypatch):
    from gssd import _lib, plan_common, synth
    lib = _lib.lib
    dev = torch.device('cuda:0')
    x = synth.synth_images(4, seed=7).to(dev)       # (batch 4: with 2 values per channel the 1 x 1 map's train-mode BatchNorm is ill-conditioned)
    res = {}
    for fuse in (True, False):
        monkeypatch.setattr(plan_common, 'FUSE_PACK', fuse)
        net = _gssdpp(dev)
        with torch.no_grad():
            outs = [tuple(t.clone() for t in net(x)[:2]) for _ in range(4)]      # eager runs, then the captured (zero-copy) graphs
        plan = net._engine._last_plan
        assert plan.nograd
        npack = sum(1 for s in plan.steps if s.fn is lib.gssd_pack_input_nhwc)
        res[fuse] = (len(plan.steps), npack, outs)
        c11 = next(s for s in plan.steps if s.tag is not None and s.tag.layer == 'vgg.0' and s.tag.desc is not None).tag.desc
        assert bool(c11.flags & _lib.CONV_IN_NCHW3) == fuse
    assert res[True][1] == 0 and res[False][1] == 1 and res[True][0] == res[False][0] - 1
    # the same network both ways: equal up to last-bit flips of a BatchNorm scale (fp64 atomic order of the batch sums, module docstring)
    for (l1, c1), (l0, c0) in zip(res[True][2], res[False][2]):
        dl = float((l1 - l0).abs().max() / l0.abs().max())
        dc = float((c1 - c0).abs().max() / c0.abs().max())
        print(f'fused vs pack launch, whole forward: loc {dl:.2e} conf {dc:.2e} (relative to the tensor max)')
        assert dl < 1e-5 and dc < 1e-5
    # a forward whose backward reads the packed copy (conv1_1's weight gradient), and the bf16 storage mode, keep the pack launch
    monkeypatch.setattr(plan_common, 'FUSE_PACK', True)
    net = _gssdpp(dev)
    net(x)
    plan = net._engine._last_plan
    assert not plan.nograd and sum(1 for s in plan.steps if s.fn is lib.gssd_pack_input_nhwc) == 1
    net.compute_dtype = 'bf16'
    with torch.no_grad():
        net(x)
    assert sum(1 for s in net._engine._last_plan.steps if s.fn is lib.gssd_pack_input_nhwc_bf16) == 1
