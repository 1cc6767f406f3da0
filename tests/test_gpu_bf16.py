"""GPU parity tests of the bf16 storage mode (BASELINE.json configs[4]: bf16 weights / activations, bf16 MFMA, fp32 accumulation /
BatchNorm statistics / softmax / offsets / loss / NMS), through the C ABI.

The reference has no bf16 mode.  The contract: the HIP bf16 path equals the CPU oracle evaluated with a
round-to-nearest-even bf16 rounding at every point where the HIP path STORES bf16 (oracle ``bf16=True``; weights rounded once,
fp32 accumulation), <= 1e-2 per tensor and <= 1e-3 on the loss; index work (matching, mining, NMS) stays bit-exact on identical
inputs.  Op level: against torch-CPU fp32 arithmetic on the bf16-rounded operands, within one bf16 ulp of the output.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gssd_oracle as O          # noqa: E402
from gssd import synth                       # noqa: E402
from gpu_common import assert_kernel         # noqa: E402

BF_ULP = 2.0 ** -8          # spacing of bf16 just below a power of two, relative to the value
BF_ULP_LOW = 2.0 ** -7      # ... just above a power of two: one ulp of the tensor's largest element can be this much of it


def rel(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def l2rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def q(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


# The last two elements of a case: the kernel instance of the launch with a bf16 output and of the launch with an fp32 output
# (GSSD_CONV_OUT_F32: the thin and flat-window kernels only store bf16, so that launch is always the generic kernel's), asserted before the
# launch.  The maps are small: B Ho Wo <= 4096 rows take the generic kernel's three-stage 64 x 64 tile (<= 512: 32 x 64) whatever cout_g
# is; all six of its tiles are run by tests/test_gpu_conv_leaves.py.
CASES = [
    # B, H, Cin, Cout, k, s, p, d, groups
    (2, 37, 32, 64, 3, 1, 1, 1, 4, 'conv_bf16<128x16>', 'conv_bf16<128x16>'),      # conv1_1-like: 8 ch / group (3 real + 5 pad), cout_g 16: single-tile lanes (8-byte stores)
    (2, 30, 64, 64, 3, 1, 1, 1, 4, 'conv_bf16<128x16>', 'conv_bf16<128x16>'),      # conv1_2 on a map below the thin kernels' 75 x 75
    (2, 21, 128, 128, 3, 1, 1, 1, 4, 'conv_bf16<128x32>', 'conv_bf16<128x32>'),    # cout_g = 32
    (2, 19, 256, 256, 3, 1, 1, 1, 4, 'conv_flat_bf16<64,64,128>', 'conv_bf16<64x64>'),        # cout_g = 64: the flat-window kernel; fp32 output: generic
    (2, 19, 512, 512, 3, 1, 1, 1, 4, 'conv_flat_bf16<128,128,128>', 'conv_bf16<64x64>'),      # cout_g = 128
    (2, 19, 512, 1024, 3, 1, 6, 6, 4, 'conv_flat_bf16<128,128,128>', 'conv_bf16<64x64>'),     # conv6: dilation 6
    (3, 19, 1024, 1024, 1, 1, 0, 1, 4, 'conv_bf16<64x64>', 'conv_bf16<64x64>'),    # conv7: grouped 1x1
    (2, 19, 256, 512, 3, 2, 1, 1, 4, 'conv_bf16<32x64>', 'conv_bf16<32x64>'),      # extras stride 2
    (5, 3, 128, 256, 3, 1, 0, 1, 4, 'conv_bf16<32x64>', 'conv_bf16<32x64>'),       # 3 -> 1
    (2, 10, 512, 512, 1, 1, 0, 1, 1, 'conv_bf16<32x64>', 'conv_bf16<32x64>'),      # dense 1x1 fuse
    (1, 83, 32, 64, 3, 1, 1, 1, 4, 'conv_thin_bf16<8,16>', 'conv_bf16<128x16>'),   # patch-staged thin kernels (maps >= 75 x 75, bf16 output): <8,16>, ragged 8 x 16 tiles
    (1, 83, 64, 64, 3, 1, 1, 1, 4, 'conv_thin_bf16<16,16>', 'conv_bf16<128x16>'),  # <16,16>
    (1, 80, 64, 128, 3, 1, 1, 1, 4, 'conv_thin_bf16<16,32>', 'conv_bf16<128x32>'),    # <16,32>
    (1, 77, 128, 128, 3, 1, 1, 1, 4, 'conv_thin_bf16<32,32>', 'conv_bf16<128x32>'),   # <32,32>
    (2, 77, 128, 256, 3, 1, 1, 1, 4, 'conv_flat_bf16<32,64,128>', 'conv_bf16<128x64>'),     # conv3_1 shape on a large map: flat <32, 64>; fp32 output: the generic kernel's 128-row tile
    (2, 75, 256, 256, 3, 1, 1, 1, 4, 'conv_flat_bf16<64,64,128>', 'conv_bf16<128x64>'),     # conv3_2 / conv3_3: flat-window kernel <64, 64> (csrc/conv_flat_bf16.hip), last tile ragged
    (3, 38, 256, 512, 3, 1, 1, 1, 4, 'conv_flat_bf16<64,128,128>', 'conv_bf16<128x64>'),    # conv4_1: flat <64, 128>
    (2, 38, 512, 512, 3, 1, 1, 1, 4, 'conv_flat_bf16<128,128,128>', 'conv_bf16<64x64>'),    # conv4_2 / conv4_3: flat <128, 128>, two staged channel halves
    (1, 12, 128, 256, 3, 1, 1, 1, 4, 'conv_flat_bf16<32,64,128>', 'conv_bf16<32x64>'),      # flat <32, 64> on a map of 144 pixels: one full tile + 16 pixels, windows mostly outside the image
    (2, 13, 512, 1024, 3, 1, 3, 3, 4, 'conv_flat_bf16<128,128,128>', 'conv_bf16<32x64>'),   # flat, dilation 3, two 128-channel tiles per group
]


@pytest.mark.parametrize('case', CASES)
def test_conv_bf16(dev, case):
    from gssd import ops, _lib
    import ctypes as C
    B, H, Cin, Cout, k, s, p, d, g, want_bf16, want_f32 = case
    rng = np.random.default_rng(hash(case[:9]) % (2 ** 31))
    x = q(torch.from_numpy(rng.normal(size=(B, Cin, H, H)).astype(np.float32)))
    w = q(torch.from_numpy(rng.normal(0, 0.1, size=(Cout, Cin // g, k, k)).astype(np.float32)))
    b = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    ref = torch.nn.functional.conv2d(x, w, b, s, p, d, g)
    xd = nhwc(x).to(dev).to(torch.bfloat16)
    wp = ops.pack_weight_bf16(w.to(dev))
    Ho = ref.shape[2]
    stats = torch.zeros(2 * Cout, dtype=torch.float64, device=dev)
    for f32 in (False, True):
        out = torch.empty(B, Ho, Ho, Cout, device=dev, dtype=torch.float32 if f32 else torch.bfloat16)
        stats.zero_()
        dsc, _, _ = ops.make_conv_desc(xd, wp, out, B=B, H=H, W=H, in_stride=Cin, cin_g=Cin // g, Cout=Cout, groups=g, k=k, stride=s,
                                       pad=p, dil=d, bias=b.to(dev), stats=stats, flags=_lib.CONV_OUT_F32 if f32 else 0)
        assert_kernel(dsc, want_f32 if f32 else want_bf16, bf16=True)
        _lib.check(_lib.lib.gssd_conv2d_nhwc_bf16(C.byref(dsc), torch.cuda.current_stream().cuda_stream))
        y = nchw(out.float())
        # fp32 accumulation of exact bf16 products; the bf16 output is that rounded once
        assert rel(y, ref) < (1e-5 if f32 else 1.01 * BF_ULP)
        if not f32:
            assert torch.equal(y.cpu(), q(y.cpu()))
            assert float((y.cpu() - q(ref)).abs().max()) <= float(ref.abs().max()) * BF_ULP   # at most one ulp off the rounded oracle
        # batch statistics come from the fp32 accumulators (before the rounding)
        n = ref.numel() / Cout
        assert rel(stats[:Cout] / n, ref.double().mean(dim=(0, 2, 3))) < 1e-5
        assert rel(stats[Cout:] / n, (ref.double() ** 2).mean(dim=(0, 2, 3))) < 1e-5


# (Cin, Cout, forced pixel tile) -> kernel instance <cin_g, output-channel tile, pixels>, with or without the fused input transform
FLAT_KERNELS = {
    (256, 256, 128): 'conv_flat_bf16<64,64,128>', (256, 256, 256): 'conv_flat_bf16<64,64,256>',
    (512, 512, 128): 'conv_flat_bf16<128,128,128>', (512, 512, 256): 'conv_flat_bf16<128,128,256>',
    (128, 256, 128): 'conv_flat_bf16<32,64,128>', (128, 256, 256): 'conv_flat_bf16<32,64,256>',
    (512, 1024, 128): 'conv_flat_bf16<128,128,128>', (512, 1024, 256): 'conv_flat_bf16<128,128,256>',
}


@pytest.mark.parametrize('Cin,Cout,H,W', [(256, 256, 21, 37), (512, 512, 9, 40), (128, 256, 33, 14), (512, 1024, 17, 23)])
@pytest.mark.parametrize('xf', [False, True])
@pytest.mark.parametrize('bm', [128, 256])
def test_conv_flat_bf16(dev, Cin, Cout, H, W, xf, bm):
    """csrc/conv_flat_bf16.hip (conv3_1 .. conv6 in bf16 mode): non-square maps (a row / column mix-up in the flat window cannot
    hide), tiles that start and end mid-row, the sideways-tap masks at both image borders, both staged channel halves, with and
    without the deferred producer BatchNorm + ReLU (zero padding AFTER the transform), bf16 output + batch statistics."""
    from gssd import ops, _lib
    import ctypes as C
    rng = np.random.default_rng(Cin + 7 * H + W)
    B, g = 3, 4
    x = q(torch.from_numpy(rng.normal(0.2, 1.0, size=(B, Cin, H, W)).astype(np.float32)))
    w = q(torch.from_numpy(rng.normal(0, 0.05, size=(Cout, Cin // g, 3, 3)).astype(np.float32)))
    b = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    act, sc, sh, pdv = x, None, None, None
    if xf:
        scv = torch.from_numpy(rng.uniform(-1.5, 1.5, size=Cin).astype(np.float32))
        shv = torch.from_numpy(rng.normal(size=Cin).astype(np.float32))
        act = q(torch.relu(torch.addcmul(shv.view(1, -1, 1, 1), x, scv.view(1, -1, 1, 1))))     # fma, like the kernel
        sc, sh = scv.to(dev), shv.to(dev)
        pdv = torch.zeros(Cin, device=dev, dtype=torch.bfloat16)          # (unused by the flat kernel: it stages zeros and skips them)
    ref = torch.nn.functional.conv2d(act, w, b, 1, 1, 1, g)
    wp = ops.pack_weight_bf16(w.to(dev))
    out = torch.empty(B, H, W, Cout, device=dev, dtype=torch.bfloat16)
    stats = torch.zeros(2 * Cout, dtype=torch.float64, device=dev)
    d, _, _ = ops.make_conv_desc(nhwc(x).to(dev).to(torch.bfloat16), wp, out, B=B, H=H, W=W, in_stride=Cin, cin_g=Cin // g, Cout=Cout,
                                 groups=g, k=3, stride=1, pad=1, bias=b.to(dev), stats=stats, in_scale=sc, in_shift=sh, in_pad=pdv)
    prev = _lib.lib.gssd_conv_flat_bf16_tile(bm)          # 128 pixels / 256 threads or 256 pixels / 512 threads per workgroup
    try:
        took = _lib.lib.gssd_conv_flat_bf16_takes(C.byref(d))
        assert took == bm                                     # the flat kernel, in the forced form
        assert_kernel(d, FLAT_KERNELS[(Cin, Cout, bm)], bf16=True)
        _lib.check(_lib.lib.gssd_conv2d_nhwc_bf16(C.byref(d), torch.cuda.current_stream().cuda_stream))
    finally:
        _lib.lib.gssd_conv_flat_bf16_tile(prev)
    y = nchw(out.float())
    # without the transform: exact bf16 products, fp32 accumulation, one rounding.  With it an activation can round the other way
    # (the oracle's fma is the kernel's fma, but ties at the bf16 boundary are hit by ~1e-3 of the elements)
    if not xf:
        assert rel(y, ref) < 1.01 * BF_ULP
        assert float((y.cpu() - q(ref)).abs().max()) <= float(ref.abs().max()) * BF_ULP
    else:
        assert rel(y, ref) < 2 * BF_ULP and l2rel(y, ref) < 0.6 * BF_ULP
    n = ref.numel() / Cout
    assert rel(stats[:Cout] / n, ref.double().mean(dim=(0, 2, 3))) < (1e-5 if not xf else 2e-3)
    assert rel(stats[Cout:] / n, (ref.double() ** 2).mean(dim=(0, 2, 3))) < (1e-5 if not xf else 2e-3)


@pytest.mark.parametrize('Cin,Cout,H', [(64, 64, 84), (128, 128, 78)])
@pytest.mark.parametrize('xf', [False, True])
def test_conv_thin_bf16_pooled_epilogue(dev, Cin, Cout, H, xf):
    """GSSD_CONV_POOL2 on the thin bf16 kernels (conv1_2 / conv2_2 of a no-backward forward): the launch stores the 2x2 max-pooled raw map
    where the BatchNorm weight is >= 0 and the min-pooled one where it is negative, with the batch sums of the FULL map; the consumer's
    deferred BatchNorm + ReLU of that map equals BatchNorm + ReLU + max-pool of the full map bit for bit (checked here on the stored
    values with both signs of gamma, ragged tiles, an odd-column border)."""
    from gssd import ops, _lib
    import ctypes as C
    rng = np.random.default_rng(Cin + H)
    B, g = 2, 4
    x = q(torch.from_numpy(rng.normal(0.2, 1.0, size=(B, Cin, H, H)).astype(np.float32)))
    w = q(torch.from_numpy(rng.normal(0, 0.08, size=(Cout, Cin // g, 3, 3)).astype(np.float32)))
    b = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    gamma = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))              # both signs
    gamma[3] = 0.0
    act, sc, sh, pdv = x, None, None, None
    if xf:
        scv = torch.from_numpy(rng.uniform(-1.5, 1.5, size=Cin).astype(np.float32))
        shv = torch.from_numpy(rng.normal(size=Cin).astype(np.float32))
        act = q(torch.relu(torch.addcmul(shv.view(1, -1, 1, 1), x, scv.view(1, -1, 1, 1))))
        sc, sh, pdv = scv.to(dev), shv.to(dev), torch.zeros(Cin, device=dev, dtype=torch.bfloat16)
    ref = torch.nn.functional.conv2d(act, w, b, 1, 1, 1, g)
    wp = ops.pack_weight_bf16(w.to(dev))
    Hp = (H + 1) // 2
    out = torch.full((B, Hp, Hp, Cout), float('nan'), device=dev, dtype=torch.bfloat16)
    full = torch.empty(B, H, H, Cout, device=dev, dtype=torch.bfloat16)
    stats, stats_full = torch.zeros(2 * Cout, dtype=torch.float64, device=dev), torch.zeros(2 * Cout, dtype=torch.float64, device=dev)
    gd_ = gamma.to(dev)
    kw = dict(B=B, H=H, W=H, in_stride=Cin, cin_g=Cin // g, Cout=Cout, groups=g, k=3, stride=1, pad=1, bias=b.to(dev), in_scale=sc,
              in_shift=sh, in_pad=pdv)
    d, _, _ = ops.make_conv_desc(nhwc(x).to(dev).to(torch.bfloat16), wp, out, stats=stats, flags=_lib.CONV_POOL2, pool_sign=gd_, **kw)
    d0, _, _ = ops.make_conv_desc(nhwc(x).to(dev).to(torch.bfloat16), wp, full, stats=stats_full, **kw)
    st_ = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.gssd_conv2d_nhwc_bf16(C.byref(d), st_))
    _lib.check(_lib.lib.gssd_conv2d_nhwc_bf16(C.byref(d0), st_))
    # exactly the pooled image of what the plain launch stores, and the same batch sums
    want = pool_by_sign(nchw(full.float().cpu()), gamma)
    assert torch.equal(nchw(out.float().cpu()), want)
    assert rel(stats, stats_full) < 1e-13                                  # the same fp32 additions in the same order (fp64 atomics: last bits)
    assert rel(nchw(out.float()), q(pool_by_sign(ref, gamma))) < (1.01 if not xf else 2.0) * BF_ULP
    # the identity the trick rests on: deferred BatchNorm + ReLU of the pooled map == max-pool(BatchNorm + ReLU(full map))
    scale = gamma * 0.7
    shift = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    f = lambda t: torch.relu(torch.addcmul(shift.view(1, -1, 1, 1), t, scale.view(1, -1, 1, 1)))
    assert torch.equal(f(want), torch.nn.functional.max_pool2d(f(nchw(full.float().cpu())), 2, 2, 0, ceil_mode=True))


FUSED_INPUT_KERNELS = {          # case -> kernel instance (fp32 output: always the generic kernel)
    (64, 64, 40, 3, 1, 1): 'conv_bf16<128x16>', (128, 128, 40, 3, 1, 1): 'conv_bf16<128x32>', (512, 512, 19, 3, 1, 1): 'conv_bf16<64x64>',
    (1024, 1024, 19, 1, 1, 0): 'conv_bf16<64x64>', (256, 512, 19, 3, 2, 1): 'conv_bf16<32x64>', (256, 256, 77, 3, 1, 1): 'conv_bf16<128x64>',
}


@pytest.mark.parametrize('Cin,Cout,H,k,st,pd', list(FUSED_INPUT_KERNELS))
def test_conv_bf16_fused_input_bn_relu(dev, Cin, Cout, H, k, st, pd):
    """Consumer-side BatchNorm + ReLU on bf16 raw input: conv2d(q(relu(q(x) * scale + shift))) with zero padding after the transform."""
    from gssd import ops, _lib
    import ctypes as C
    rng = np.random.default_rng(Cin + H)
    B, g = 2, 4
    x = q(torch.from_numpy(rng.normal(0.2, 1.0, size=(B, Cin, H, H)).astype(np.float32)))
    gm = torch.from_numpy(rng.uniform(-1.5, 1.5, size=Cin).astype(np.float32))
    bt = torch.from_numpy(rng.normal(size=Cin).astype(np.float32))
    w = q(torch.from_numpy(rng.normal(0, 0.1, size=(Cout, Cin // g, k, k)).astype(np.float32)))
    b = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    stats = torch.stack([x.double().sum(dim=(0, 2, 3)), (x.double() ** 2).sum(dim=(0, 2, 3))]).reshape(-1).to(dev)
    sc, sh = torch.empty(Cin, device=dev), torch.empty(Cin, device=dev)
    pdv = torch.empty(Cin, device=dev, dtype=torch.bfloat16)
    rm, rv = torch.zeros(Cin, device=dev), torch.ones(Cin, device=dev)
    st_ = torch.cuda.current_stream().cuda_stream
    gmd, btd = gm.to(dev), bt.to(dev)          # (named: a temporary's storage is recycled as soon as .data_ptr() returns)
    _lib.check(_lib.lib.gssd_bn_finalize_bf16(stats.data_ptr(), float(B * H * H), gmd.data_ptr(), btd.data_ptr(),
                                              rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, 1, Cin, sc.data_ptr(), sh.data_ptr(),
                                              pdv.data_ptr(), 0, st_))
    act = q(torch.relu(x * sc.cpu().view(1, -1, 1, 1) + sh.cpu().view(1, -1, 1, 1)))
    ref = torch.nn.functional.conv2d(act, w, b, st, pd, 1, g)
    wp = ops.pack_weight_bf16(w.to(dev))
    Ho = ref.shape[2]
    out = torch.empty(B, Ho, Ho, Cout, device=dev)
    d, _, _ = ops.make_conv_desc(nhwc(x).to(dev).to(torch.bfloat16), wp, out, B=B, H=H, W=H, in_stride=Cin, cin_g=Cin // g, Cout=Cout,
                                 groups=g, k=k, stride=st, pad=pd, bias=b.to(dev), in_scale=sc, in_shift=sh, in_pad=pdv,
                                 flags=_lib.CONV_OUT_F32)
    assert_kernel(d, FUSED_INPUT_KERNELS[(Cin, Cout, H, k, st, pd)], bf16=True)
    _lib.check(_lib.lib.gssd_conv2d_nhwc_bf16(C.byref(d), st_))
    # a bf16 rounding flip of an activation (fp32 fma vs mul + add) moves single outputs by ~1e-3 of the tensor's scale
    assert rel(nchw(out), ref) < 2e-3 and l2rel(nchw(out), ref) < 2e-4


def test_elementwise_bf16(dev):
    """BatchNorm + ReLU + pool, L2Norm and the input pack in bf16 storage: fp32 arithmetic on the stored values, one rounding."""
    from gssd import _lib
    lib, st = _lib.lib, torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(3)
    B, Cc, H = 3, 64, 19
    raw = q(torch.from_numpy(rng.normal(0.3, 1.2, size=(B, Cc, H, H)).astype(np.float32)))
    gm = torch.from_numpy(rng.uniform(0.5, 1.5, size=Cc).astype(np.float32))
    bt = torch.from_numpy(rng.normal(size=Cc).astype(np.float32))
    # statistics as the conv would deliver them (from an fp32 tensor whose bf16 copy is `raw`: here the same values)
    stats = torch.stack([raw.double().sum(dim=(0, 2, 3)), (raw.double() ** 2).sum(dim=(0, 2, 3))]).reshape(-1).to(dev)
    rawd, gmd, btd = nhwc(raw).to(dev).to(torch.bfloat16), gm.to(dev), bt.to(dev)
    for pool in (None, (2, 2, 0), (3, 1, 1)):
        Hp = H if pool is None else (H + 2 * pool[2] - pool[0]) // pool[1] + 1
        out = torch.empty(B, Hp, Hp, Cc, device=dev, dtype=torch.bfloat16)
        rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
        pk, ps, pp = pool if pool else (0, 1, 0)
        _lib.check(lib.gssd_bn_relu_pool_bf16(rawd.data_ptr(), out.data_ptr(), B, H, H, Cc, Hp, Hp, pk, ps,
                                              pp, stats.data_ptr(), float(B * H * H), gmd.data_ptr(), btd.data_ptr(),
                                              rm.data_ptr(), rv.data_ptr(), 0.1, 1e-5, 1, 1, 0, st))
        y = torch.relu(torch.nn.functional.batch_norm(raw, None, None, gm, bt, True, 0.1, 1e-5))
        if pool:
            y = torch.nn.functional.max_pool2d(y, pool[0], pool[1], pool[2])
        assert rel(nchw(out.float()), q(y)) < 1.01 * BF_ULP
    w = torch.from_numpy(rng.uniform(15, 25, size=Cc).astype(np.float32))
    out = torch.empty(B, H, H, Cc, device=dev, dtype=torch.bfloat16)
    wd = w.to(dev)
    _lib.check(lib.gssd_l2norm_bf16(rawd.data_ptr(), wd.data_ptr(), out.data_ptr(), B * H * H, Cc, 1e-10, st))
    assert rel(nchw(out.float()), q(O.l2norm(raw, w))) < 1.01 * BF_ULP
    x = torch.from_numpy(rng.uniform(0, 1, size=(2, 12, 9, 9)).astype(np.float32))
    y = torch.empty(2, 9, 9, 32, device=dev, dtype=torch.bfloat16)
    xd = x.to(dev)
    _lib.check(lib.gssd_pack_input_nhwc_bf16(xd.data_ptr(), y.data_ptr(), 2, 12, 9, 9, 4, st))
    yy = y.float().cpu().view(2, 9, 9, 4, 8)
    assert torch.equal(yy[..., :3].permute(0, 3, 4, 1, 2).reshape(2, 12, 9, 9), q(x)) and float(yy[..., 3:].abs().max()) == 0


@pytest.mark.parametrize('B,Cc,H,dg,Cout', [(2, 128, 9, 4, 32), (3, 128, 13, 1, 296), (5, 256, 11, 4, 512)])
def test_dcn_bf16(dev, B, Cc, H, dg, Cout):
    """bf16 fused deformable conv vs the oracle restatement on bf16-rounded operands with bf16-rounded sampled columns."""
    from gssd import _lib
    lib, st = _lib.lib, torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(18)
    x = q(torch.from_numpy(rng.normal(size=(B, Cc, H, H)).astype(np.float32)))
    om = torch.from_numpy(rng.normal(0, 2.5, size=(B, 27 * dg, H, H)).astype(np.float32))
    w = q(torch.from_numpy(rng.normal(0, 0.1, size=(Cout, Cc, 3, 3)).astype(np.float32)))
    bias = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
    o1, o2, m = torch.chunk(om, 3, dim=1)
    ref = O.dcn_v2_conv(x, torch.cat((o1, o2), 1), torch.sigmoid(m), w, bias, 1, 1, 1, dg, col_round=q)
    n = int(lib.gssd_dcn_packed_weight_elems_bf16(Cout, Cc))
    wp = torch.empty(n, device=dev, dtype=torch.bfloat16)
    wd, xd, omd, bd = w.to(dev), nhwc(x).to(dev).to(torch.bfloat16), nhwc(om).to(dev), bias.to(dev)
    _lib.check(lib.gssd_dcn_pack_weight_bf16(wd.data_ptr(), wp.data_ptr(), Cout, Cc, dg, st))
    out = torch.empty(B, H, H, Cout, device=dev, dtype=torch.bfloat16)
    _lib.check(lib.gssd_dcn_forward_bf16(xd.data_ptr(), omd.data_ptr(), wp.data_ptr(), bd.data_ptr(), out.data_ptr(), B, H, H, Cc, dg,
                                         27 * dg, Cout, st))
    # the blend's operation order differs from the oracle's (weights folded with the mask first): a few columns round the other
    # way; one output bf16 ulp + that
    assert rel(nchw(out.float()), ref) < 3 * BF_ULP and l2rel(nchw(out.float()), ref) < BF_ULP


def test_dcn_bf16_loader_wave_kernel_is_bit_identical(dev, tmp_path):
    """csrc/dcn_bf16.hip's opt-in round-5 kernel (GSSD_DCN_BF16_V3=1: eight matrix + four loader waves; the switch is read once per process,
    so it runs in a child process) against the default kernel: the same blend arithmetic and K order -> the same bits."""
    import os
    import subprocess
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import os, sys, torch
sys.path.insert(0, os.path.join(sys.argv[1], 'grouped-ssd-pytorch_amd'))
from gssd._lib import lib, check
dev = torch.device('cuda:0')
res = {}
for (B, H, Cc, dg, Cout) in ((3, 13, 128, 1, 296), (2, 19, 256, 4, 512), (1, 11, 128, 2, 40)):
    g = torch.Generator().manual_seed(B * 1000 + Cc)
    x = torch.randn(B, H, H, Cc, generator=g).to(dev).to(torch.bfloat16)
    om = (torch.randn(B, H, H, 27 * dg, generator=g) * 1.5).to(dev)
    w = (torch.randn(Cout, Cc, 3, 3, generator=g) * 0.05).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev)
    wp = torch.empty(int(lib.gssd_dcn_packed_weight_elems_bf16(Cout, Cc)), device=dev, dtype=torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    check(lib.gssd_dcn_pack_weight_bf16(w.data_ptr(), wp.data_ptr(), Cout, Cc, dg, s))
    out = torch.full((B, H, H, Cout), float('nan'), device=dev, dtype=torch.bfloat16)
    check(lib.gssd_dcn_forward_bf16(x.data_ptr(), om.data_ptr(), wp.data_ptr(), bias.data_ptr(), out.data_ptr(), B, H, H, Cc, dg, 27 * dg, Cout, s))
    torch.cuda.synchronize()
    res[(B, H, Cc, dg, Cout)] = out.cpu()
torch.save(res, sys.argv[2])
"""
    outs = []
    for v in ('0', '1'):
        f = str(tmp_path / f'dcnb_{v}.pt')
        env = dict(os.environ, GSSD_DCN_BF16_V3=v)
        r = subprocess.run([sys.executable, '-c', code, ROOT, f], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(torch.load(f))
    for k in outs[0]:
        assert torch.isfinite(outs[0][k].float()).all()
        assert torch.equal(outs[0][k], outs[1][k]), k


NETS = {
    'gssd': (dict(), (True, 4, 4, 1, True, False, False, 0, 1, False, False, 1)),
    'gssdpp': (dict(use_self_attention=True, use_self_attention_base=True, num_dcn_layers=1, groups_dcn=4, dcn_cat_sab=True),
               (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)),
}


def pool_by_sign(raw, gamma):
    """What a GSSD_CONV_POOL2 launch stores: 2x2 / stride-2 ceil-mode max-pool of the raw map where gamma >= 0, min-pool elsewhere."""
    F = torch.nn.functional
    mx = F.max_pool2d(raw, 2, 2, 0, ceil_mode=True)
    mn = -F.max_pool2d(-raw, 2, 2, 0, ceil_mode=True)
    return torch.where(gamma.view(1, -1, 1, 1) >= 0, mx, mn)


def _layer_local_checks(plan, net, name):
    """Teacher-forced parity at full network scale: every stage of the HIP bf16 plan is recomputed on the CPU FROM THE HIP PATH'S OWN
    STORED INPUT of that stage (so rounding flips do not cascade) and must agree within one bf16 ulp (a few for the sampled /
    attention stages whose fp32 operation order differs)."""
    F = torch.nn.functional
    worst = {}
    for kind, r in plan.rec:
        if kind == 'convbn':
            conv, bn = r['conv'], r['bn']
            x = r['x_in'].float().cpu()
            if r['in_xf'] is not None:
                sc, sh = r['in_xf'][0].cpu(), r['in_xf'][1].cpu()
                x = q(torch.relu(x * sc + sh))
            xin = nchw(x)
            if conv.weight.shape[1] * r['groups'] != xin.shape[1]:          # conv1_1: 3 real channels of 8 per phase
                xin = xin.view(xin.shape[0], r['groups'], -1, *xin.shape[2:])[:, :, :conv.weight.shape[1]].reshape(
                    xin.shape[0], -1, *xin.shape[2:])
            ref_raw = F.conv2d(xin, q(conv.weight.detach().cpu()), conv.bias.detach().cpu(), r['stride'], r['pad'], r['dil'], r['groups'])
            raw = nchw(r['raw'].float().cpu())
            if r.get('pooled'):          # GSSD_CONV_POOL2: max- / min-pooled raw map (by the sign of the BatchNorm weight), ceil mode
                ref_raw = pool_by_sign(ref_raw, bn.weight.detach().cpu())
            worst[r['name'] + '.raw'] = rel(raw, q(ref_raw))
            if r['xf'] is None:
                mean = ref_raw.mean(dim=(0, 2, 3))
                var = ref_raw.var(dim=(0, 2, 3), unbiased=False)
                scale = bn.weight.detach().cpu() / torch.sqrt(var + bn.eps)
                shift = bn.bias.detach().cpu() - mean * scale
                y = torch.relu(raw * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
                if r['pool']:
                    pk, ps, pp, ceil = r['pool']
                    y = F.max_pool2d(y, pk, ps, pp, ceil_mode=ceil)
                worst[r['name'] + '.act'] = rel(nchw(r['out'].float().cpu()), q(y))
        elif kind == 'l2norm':
            worst['l2norm'] = rel(nchw(r['out'].float().cpu()), q(O.l2norm(nchw(r['x_in'].float().cpu()), r['mod'].weight.detach().cpu())))
        elif kind == 'dcn':
            m, xin = r['mod'], nchw(r['x_in'].float().cpu())
            om_ref = F.conv2d(xin, q(m.conv_offset_mask.weight.detach().cpu()), m.conv_offset_mask.bias.detach().cpu(), 1, 1)
            om = nchw(r['om'].cpu())
            assert float(om[:, 27 * r['dg']:].abs().max()) == 0.0 if om.shape[1] > 27 * r['dg'] else True     # pad channels of the rows
            om = om[:, :27 * r['dg']]
            worst['dcn.om'] = rel(om, om_ref)
            o1, o2, mk = torch.chunk(om, 3, dim=1)                       # the HIP path's own offsets / mask logits
            ref = O.dcn_v2_conv(xin, torch.cat((o1, o2), 1), torch.sigmoid(mk), q(m.weight.detach().cpu()), m.bias.detach().cpu(), 1, 1, 1,
                                r['dg'], col_round=q)
            worst['dcn.out'] = rel(nchw(r['out'].float().cpu()), q(ref)) / 3
        elif kind == 'sa':
            sa, xin = r['mod'], nchw(r['x_in'].float().cpu())
            sd1 = {'p.' + k: v.detach().cpu() for k, v in sa.state_dict().items()}
            o_out, o_ag, _ = O.self_attn(xin, sd1, 'p', False, q=q)      # u / v already advanced by the HIP forward
            worst[f"sa{r['H']}.out"] = rel(nchw(r['out'].float().cpu()), o_out) / 2
    return worst


@pytest.mark.parametrize('name', list(NETS))
def test_bf16_end_to_end(dev, name):
    """configs[4] graph at batch 4.  Two bf16 implementations whose fp32 summation orders differ cannot agree to 1e-2 end to end:
    one rounding flip (1 bf16 ulp on ~1e-4 of the elements after the first block) perturbs ~9 x cout_g neighbours by ~1e-3, each of
    which flips with probability ~0.2 -- the set of differing elements grows 1e-4 -> 0.36 across the trunk (scripts/dbg_bf16_taps.py).
    So the contract is stated as
      (1) layer-local, teacher-forced: every stage recomputed from the HIP path's own stored input agrees within one bf16 ulp;
      (2) whole network: the distance to the bf16-rounded oracle is not larger than bf16's own distance to the fp32 oracle, and the
          loss agrees with the bf16 oracle's within 1e-2 (and the fp32 oracle's within 5e-2);
      (3) index work (matching, mining, NMS) is fp32 and bit-exact on the bf16 path's own outputs."""
    from models.ssd_multiphase_custom_group import build_ssd
    from layers.modules import MultiBoxLoss
    from gssd import ops
    flags, args = NETS[name]
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    net.compute_dtype = 'bf16'
    x = synth.synth_images(4, seed=5)
    tg = synth.synth_targets(4, seed=5)
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    with torch.no_grad():
        loc, conf, pri = net(x.to(dev))
        ll, lc = crit((loc, conf, pri), tg)
    assert loc.dtype == torch.float32 and conf.dtype == torch.float32
    # (1) layer-local
    worst = _layer_local_checks(net._engine._last_plan, net, name)
    bad = {k: v for k, v in worst.items() if v > 1.01 * BF_ULP_LOW}
    print(name, 'layer-local worst (units of max-abs):', {k: f'{v:.1e}' for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:6]})
    assert not bad, bad
    # (2) whole network
    with torch.no_grad():
        lo, co, upd = O.gssd_forward(sd, x, bf16=True, **flags)
        lo32, co32, _ = O.gssd_forward(sd, x, **flags)
    pri_np = O.prior_box()
    tgn = [t.numpy() for t in tg]
    rl, rc = O.multibox_loss(lo.numpy(), co.numpy(), pri_np, tgn)
    rl32, rc32 = O.multibox_loss(lo32.numpy(), co32.numpy(), pri_np, tgn)
    e = dict(loc=l2rel(loc, lo), conf=l2rel(conf, co), loc_bf16_vs_f32=l2rel(lo, lo32), conf_bf16_vs_f32=l2rel(co, co32),
             loss_l=rel(ll, rl), loss_c=rel(lc, rc), loss_l_f32=rel(ll, rl32), loss_c_f32=rel(lc, rc32))
    print(name, 'bf16 HIP vs oracles (relative L2 / loss)', {k: f'{v:.2e}' for k, v in e.items()})
    assert e['loc'] <= 1.2 * e['loc_bf16_vs_f32'] and e['conf'] <= 1.2 * e['conf_bf16_vs_f32'], e
    assert e['loss_l'] < 1e-2 and e['loss_c'] < 1e-2 and e['loss_l_f32'] < 5e-2 and e['loss_c_f32'] < 5e-2, e
    after = net.state_dict()
    for k in ('vgg.1.running_mean', 'vgg.1.running_var'):
        assert rel(after[k], upd[k]) < 1e-3, k
    # (3) index work on identical inputs
    rl2, rc2 = O.multibox_loss(loc.cpu().numpy(), conf.cpu().numpy(), pri.cpu().numpy(), tgn)
    assert rel(ll, rl2) < 1e-4 and rel(lc, rc2) < 1e-4
    det = ops.detect(loc, conf, pri, 2, conf_is_logits=True).cpu().numpy()
    ref = O.detect(2, 0, 200, 0.01, 0.45, loc.cpu().numpy(), O.softmax_scores(conf.cpu().numpy()), pri.cpu().numpy())
    assert np.array_equal(det, ref)
    # and the fp32 mode of the same module is untouched by the switch back
    net.compute_dtype = 'f32'
    net.load_state_dict(sd)
    with torch.no_grad():
        l32, c32, _ = net(x.to(dev))
    assert rel(l32, lo32) < 1e-4 and rel(c32, co32) < 1e-4


def _layer_local_checks_sampled(plan, imgs):
    """_layer_local_checks on a SAMPLE of the batch (full-size runs): convolutions, L2Norm, the deformable conv and the attention
    blocks are per-image operations, so the sampled images' stages are recomputed from the HIP path's own stored inputs; the
    BatchNorm + ReLU (+ pool) pass is checked with the batch statistics the HIP path itself accumulated (fp64 sums of the fp32
    accumulators), and those sums are checked against the stored raw tensor of the WHOLE batch."""
    F = torch.nn.functional
    worst = {}
    ii = torch.tensor(imgs, device=plan.dev)
    for kind, r in plan.rec:
        if kind == 'convbn':
            conv, bn = r['conv'], r['bn']
            x = r['x_in'][ii].float().cpu()
            if r['in_xf'] is not None:
                sc, sh = r['in_xf'][0].cpu(), r['in_xf'][1].cpu()
                x = q(torch.relu(x * sc + sh))
            xin = nchw(x)
            if conv.weight.shape[1] * r['groups'] != xin.shape[1]:
                xin = xin.view(xin.shape[0], r['groups'], -1, *xin.shape[2:])[:, :, :conv.weight.shape[1]].reshape(
                    xin.shape[0], -1, *xin.shape[2:])
            ref_raw = F.conv2d(xin, q(conv.weight.detach().cpu()), conv.bias.detach().cpu(), r['stride'], r['pad'], r['dil'], r['groups'])
            raw = nchw(r['raw'][ii].float().cpu())
            if r.get('pooled'):
                worst[r['name'] + '.raw'] = rel(raw, q(pool_by_sign(ref_raw, bn.weight.detach().cpu())))
                continue
            worst[r['name'] + '.raw'] = rel(raw, q(ref_raw))
            Cc = r['Cout']
            n = float(r['raw'].shape[0] * r['Ho'] * r['Ho'])
            st = r['stats'].cpu().view(max(r.get('stats_rep', 1), 1), 2 * Cc).sum(0)       # replicas of the batch sums add up
            mean, var = st[:Cc] / n, st[Cc:] / n - (st[:Cc] / n) ** 2
            full = r['raw'].float()                                        # whole batch, on the device (checker-side torch math)
            worst[r['name'] + '.mean'] = float(((full.mean(dim=(0, 1, 2)).double().cpu() - mean).abs() / (var.sqrt() + 1e-6)).max()) / 4
            if r['xf'] is None:
                scale = bn.weight.detach().cpu().double() / torch.sqrt(var + bn.eps)
                shift = bn.bias.detach().cpu().double() - mean * scale
                y = torch.relu(raw * scale.float().view(1, -1, 1, 1) + shift.float().view(1, -1, 1, 1))
                if r['pool']:
                    pk, ps, pp, ceil = r['pool']
                    y = F.max_pool2d(y, pk, ps, pp, ceil_mode=ceil)
                worst[r['name'] + '.act'] = rel(nchw(r['out'][ii].float().cpu()), q(y))
        elif kind == 'l2norm':
            worst['l2norm'] = rel(nchw(r['out'][ii].float().cpu()), q(O.l2norm(nchw(r['x_in'][ii].float().cpu()), r['mod'].weight.detach().cpu())))
        elif kind == 'dcn':
            m, xin = r['mod'], nchw(r['x_in'][ii].float().cpu())
            om = nchw(r['om'][ii].cpu())[:, :27 * r['dg']]
            om_ref = F.conv2d(xin, q(m.conv_offset_mask.weight.detach().cpu()), m.conv_offset_mask.bias.detach().cpu(), 1, 1)
            worst['dcn.om'] = rel(om, om_ref)
            o1, o2, mk = torch.chunk(om, 3, dim=1)
            ref = O.dcn_v2_conv(xin, torch.cat((o1, o2), 1), torch.sigmoid(mk), q(m.weight.detach().cpu()), m.bias.detach().cpu(), 1, 1, 1,
                                r['dg'], col_round=q)
            worst['dcn.out'] = rel(nchw(r['out'][ii].float().cpu()), q(ref)) / 3
        elif kind == 'sa':
            sa, xin = r['mod'], nchw(r['x_in'][ii].float().cpu())
            sd1 = {'p.' + k: v.detach().cpu() for k, v in sa.state_dict().items()}
            o_out, o_ag, _ = O.self_attn(xin, sd1, 'p', False, q=q)
            worst[f"sa{r['H']}.out"] = rel(nchw(r['out'][ii].float().cpu()), o_out) / 2
    return worst


@pytest.mark.parametrize('name', ['gssdpp'])
def test_full_size_properties_bf16(dev, name):
    """BASELINE.json configs[4] on one GPU at the BENCHMARKED size (batch 32, bf16 storage): the flat-window / thin / 256-pixel-tile
    kernels only take their full-size forms here.  Size-independent checks: every stage of two sampled images recomputed from the HIP
    path's own stored input within one bf16 ulp (layer-local contract of test_bf16_end_to_end), BatchNorm batch sums against the stored
    raw maps of the whole batch, the loss against the oracle on the same predictions, Detect bit-exact on the path's fp32 outputs,
    eval-mode image independence (image i of the batch-32 run == the same image in a batch of 2)."""
    from models.ssd_multiphase_custom_group import build_ssd
    from layers.modules import MultiBoxLoss
    from gssd import ops
    flags, args = NETS[name]
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    net.compute_dtype = 'bf16'
    x = synth.synth_images(32, seed=11).to(dev)
    tg = synth.synth_targets(32, seed=11)
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    with torch.no_grad():
        loc, conf, pri = net(x)
        ll, lc = crit((loc, conf, pri), tg)
    assert torch.isfinite(loc).all() and torch.isfinite(conf).all() and loc.dtype == torch.float32
    plan = net._engine._last_plan
    names = {st.tag[0] for st in plan.steps if st.tag is not None}
    assert any(n.startswith('conv_flat_bf16<') for n in names) and any(n.startswith('conv_thin_bf16<') for n in names), names
    worst = _layer_local_checks_sampled(plan, [7, 31])
    print(name, 'B=32 layer-local worst:', {k: f'{v:.1e}' for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]})
    bad = {k: v for k, v in worst.items() if v > 1.01 * BF_ULP_LOW}
    assert not bad, bad
    rl, rc = O.multibox_loss(loc.cpu().numpy(), conf.cpu().numpy(), pri.cpu().numpy(), [t.numpy() for t in tg])
    assert rel(ll, rl) < 1e-4 and rel(lc, rc) < 1e-4
    with torch.no_grad():
        net.eval()
        l32, c32, _ = net(x)
        l2, c2, _ = net(x[5:7])
    assert l2rel(l32[5:7], l2) < 1e-6 and l2rel(c32[5:7], c2) < 1e-6       # per-image work does not depend on the batch it sits in
    det, keep, cnt = ops.detect(l32, c32, pri, 2, conf_is_logits=True, want_keep=True)
    det = det.cpu().numpy()
    assert (np.diff(det[:, 1, :, 0], axis=1) <= 0).all() and (det[:, 0] == 0).all()
    b = 3
    ref = O.detect(2, 0, 200, 0.01, 0.45, l32[b:b + 1].cpu().numpy(), O.softmax_scores(c32[b:b + 1].cpu().numpy()), pri.cpu().numpy())
    assert np.array_equal(det[b:b + 1], ref)


@pytest.mark.parametrize('B,H,W,Cin,Cout,groups', [
    (2, 37, 37, 64, 64, 4),        # conv1_2: 16 -> 16 per group, a wave per phase group
    (2, 30, 41, 64, 128, 4),       # conv2_1: 16 -> 32
    (2, 21, 21, 128, 128, 4),      # conv2_2: 32 -> 32, 36 accumulator tiles per wave
    (2, 19, 26, 128, 256, 4),      # conv3_1: 32 -> 64
    (2, 19, 19, 256, 256, 4),      # conv3_2: 64 -> 64
    (1, 23, 17, 256, 512, 4),      # conv4_1: 64 -> 128, two output splits
    (2, 19, 19, 512, 512, 4),      # conv4_2 .. conv5_3: 128 -> 128, four output splits
    (1, 13, 9, 128, 96, 1),        # one group, 96 outputs: masked last split
    (3, 8, 16, 64, 64, 1),         # exactly one tile per image
    (2, 19, 19, 512, 112, 1),      # dense (the DCN offset / mask conv): four 128-channel input blocks feed the same 112 outputs
    (2, 10, 10, 256, 40, 1),       # dense, two input blocks, 40 outputs (heads with padded rows)
])
@pytest.mark.parametrize('xf', [False, True])
def test_conv_wgrad_bf16(dev, B, H, W, Cin, Cout, groups, xf, k=3):
    """gssd_conv2d_wgrad_bf16 (csrc/conv_wgrad_bf16.hip: LDS transpose reads feeding v_mfma_f32_16x16x32_bf16) against the float64 weight
    gradient of the conv over the SAME bf16 operands: the input after its deferred BatchNorm + ReLU rounded to bf16 (what the forward's
    MFMA saw), d(output) rounded to bf16.  Random operands with a distinct value everywhere: a wrong tap, transposed fragment or swizzle
    cannot pass.  The input sits at a channel offset inside wider rows."""
    from gssd import ops, _lib
    import ctypes as C
    rng = np.random.default_rng(B * 1000 + H * 10 + Cin + Cout)
    ld, off = Cin + 16, 8
    xs = q(torch.from_numpy(rng.normal(size=(B, H, W, ld)).astype(np.float32)))
    dy = q(torch.from_numpy(rng.normal(size=(B, H, W, Cout)).astype(np.float32)))
    # scale / shift on coarse binary grids: x * sc + sh is exact in fp32, fused or not, so the rounded operand is unambiguous
    sc = torch.from_numpy((np.round(rng.uniform(0.5, 1.5, size=ld) * 8) / 8).astype(np.float32))
    sh = torch.from_numpy((np.round(rng.normal(0, 0.5, size=ld) * 64) / 64).astype(np.float32))
    x = xs[..., off:off + Cin]
    if xf:
        x = q(torch.relu(x * sc[off:off + Cin] + sh[off:off + Cin]))
    xr = x.permute(0, 3, 1, 2).double().requires_grad_(False)
    w = torch.zeros(Cout, Cin // groups, k, k, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv2d(xr, w, None, 1, k // 2, 1, groups)
    (y * dy.permute(0, 3, 1, 2).double()).sum().backward()
    ref = w.grad
    xd, dyd = xs.to(dev).to(torch.bfloat16), dy.to(dev).to(torch.bfloat16)
    scd, shd = sc.to(dev), sh.to(dev)
    cg = Cin // groups
    d, _, _ = ops.make_conv_desc(xd, None, None, B=B, H=H, W=W, in_stride=ld, in_ch_off=off, cin_g=cg, Cout=Cout, groups=groups, k=k, pad=k // 2,
                                 in_scale=scd if xf else None, in_shift=shd if xf else None)
    assert _lib.lib.gssd_conv2d_wgrad_bf16_supported(C.byref(d)) == 1
    dwp = torch.zeros(Cout, k * k * cg, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(2):         # accumulates: two launches = twice the gradient
        _lib.check(_lib.lib.gssd_conv2d_wgrad_bf16(C.byref(d), dyd.data_ptr(), dwp.data_ptr(), st))
    got = (dwp.cpu().double() / 2).view(Cout, k * k, cg).permute(0, 2, 1).reshape(Cout, cg, k, k)
    assert rel(got, ref) < 2e-5, rel(got, ref)
    # not a supported shape: refused, no fallback
    d2, _, _ = ops.make_conv_desc(xd, None, None, B=B, H=H, W=W, in_stride=ld, in_ch_off=off, cin_g=cg, Cout=Cout, groups=groups, k=3, pad=1,
                                  stride=2)
    assert _lib.lib.gssd_conv2d_wgrad_bf16_supported(C.byref(d2)) == 0
    assert _lib.lib.gssd_conv2d_wgrad_bf16(C.byref(d2), dyd.data_ptr(), dwp.data_ptr(), st) == -1      # GSSD_EINVAL


@pytest.mark.parametrize('B,H,W,Cin,Cout,groups', [
    (1, 45, 16, 512, 384, 1),      # Self_Attn's merged projection: dense 1x1, four input blocks, six output splits
    (1, 23, 16, 256, 512, 1),      # the o conv
    (2, 19, 19, 1024, 1024, 4),    # conv7: grouped 1x1, two 128-channel blocks per group
    (1, 5, 16, 64, 24, 1),         # one 64-channel block, masked outputs
])
@pytest.mark.parametrize('xf', [False, True])
def test_conv_wgrad_bf16_1x1(dev, B, H, W, Cin, Cout, groups, xf):
    """The 1x1 form of csrc/conv_wgrad_bf16.hip (the tile is the patch): dense and grouped, input blocks inside a group."""
    test_conv_wgrad_bf16(dev, B, H, W, Cin, Cout, groups, xf, k=1)


@pytest.mark.parametrize('M,cin,cout,groups', [(4 * 19 * 19, 1152, 512, 1), (1000, 72, 40, 1), (777, 256, 512, 4), (64, 8, 8, 1)])
def test_wgrad_nt_bf16(dev, M, cin, cout, groups):
    """The bf16 storage mode's weight gradient dW[n][k] = sum_m dY[m][n] X[m][k] (gssd/backward.py::_wgrad_nt_bf16):
    gssd_transpose_cast_f32_bf16 is exact (a transposed round-to-nearest-even cast, strided source, ragged edges, pad columns untouched)
    and the split-K NT launch over the transposed operands equals the float64 product of the bf16-rounded operands."""
    from gssd import _lib
    import ctypes as C
    rng = np.random.default_rng(M + cin)
    ld_x = cin + 8
    x = torch.from_numpy(rng.normal(size=(M, ld_x)).astype(np.float32)).to(dev)
    dy = torch.from_numpy(rng.normal(size=(M, cout)).astype(np.float32)).to(dev)
    Mp = -(-M // 64) * 64
    xT = torch.full((cin, Mp), 7.0, device=dev, dtype=torch.bfloat16)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.gssd_transpose_cast_f32_bf16(x.data_ptr(), xT.data_ptr(), M, cin, ld_x, Mp, st))
    assert torch.equal(xT[:, :M], x[:, :cin].t().to(torch.bfloat16))
    assert bool((xT[:, M:] == 7.0).all())

    class Plan:                                   # the two members the helper touches
        pass
    from gssd.backward import BackwardPlan
    steps = []
    p = Plan()
    p.dev, p.keep = dev, []
    p._add = lambda fn, args, keep=None, leaf=None: steps.append((fn, args))
    dwp = torch.zeros(cout, cin // groups, device=dev)
    BackwardPlan._wgrad_nt_bf16(p, x, ld_x, cin, dy, cout, cout, M, dwp, cin // groups, groups=groups)
    for fn, args in steps:
        _lib.check(fn(*args, st))
    xq, dq = q(x[:, :cin].cpu()).double(), q(dy.cpu()).double()
    cg, ng = cin // groups, cout // groups
    ref = torch.cat([dq[:, g * ng:(g + 1) * ng].t() @ xq[:, g * cg:(g + 1) * cg] for g in range(groups)])
    assert rel(dwp.double().cpu(), ref) < 2e-5


@pytest.mark.parametrize('name', list(NETS))
def test_bf16_backward_gradients(dev, name):
    """configs[4] is a TRAINING config (train_lesion_multiphase_v2.py:242-253): the bf16 storage mode trains with a mixed-precision
    backward -- fp32 gradients of the fp32 graph evaluated AT the bf16-rounded activations the forward stored (gssd/backward.py::
    Bf16Shadow).  Arbiter: CPU autograd through the oracle's bf16 graph with straight-through rounding (bf16='ste').  Two bf16
    forwards whose fp32 summation orders differ disagree by a few per cent after the trunk (test_bf16_end_to_end), and so do their
    gradients; the contract mirrors the forward's:
      (1) per tensor, the HIP gradient is no farther from the bf16 oracle's than the bf16 oracle's is from the fp32 oracle's (x 1.2),
      (2) the head layers, which see no discontinuity downstream, agree to 2e-2 (their inputs are bf16 activations that differ),
      (3) every gradient points the way the bf16 oracle's does at least as well as the fp32 oracle's does (cosine, - 0.05)."""
    from models.ssd_multiphase_custom_group import build_ssd
    flags, args = NETS[name]
    net = build_ssd('train', 300, 2, *args)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    sd = synth.synth_state_dict(shapes, seed=1111)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    x = synth.synth_images(4, seed=9)
    rng = np.random.default_rng(0)
    r1 = torch.from_numpy(rng.normal(size=(4, 8732, 4)).astype(np.float32))
    r2 = torch.from_numpy(rng.normal(size=(4, 8732, 2)).astype(np.float32))
    r1[:, 8728:] = 0          # the 1x1 map's BatchNorm over 4 values has an ill-conditioned backward: keep it out
    r2[:, 8728:] = 0
    keys = ['vgg.0.weight', 'vgg.14.weight', 'vgg.31.weight', 'vgg.44.weight', 'extras.2.weight', 'fuse_11.weight', 'bn_fuse_21.bias',
            'loc.0.weight', 'conf.3.bias', 'L2Norm.weight']
    if name == 'gssdpp':
        keys += ['self_attn_list.0.snconv1x1_g.weight_orig', 'dcn_list.0.weight', 'dcn_list.0.conv_offset_mask.weight']

    def hip_grads(mode):
        net.load_state_dict(sd)
        net.compute_dtype = mode
        for p in net.parameters():
            p.grad = None
        loc, conf, _ = net(x.to(dev))
        ((loc * r1.to(dev)).sum() + (conf * r2.to(dev)).sum()).backward()
        return {k: p.grad.detach().double().cpu().clone() for k, p in net.named_parameters() if k in keys}
    g_bf = hip_grads('bf16')
    g_32 = hip_grads('f32')

    def oracle_grads(bf16):
        sdg = {k: (v.clone().requires_grad_() if (v.is_floating_point() and not k.endswith(('running_mean', 'running_var', 'weight_u',
                                                                                              'weight_v'))) else v)
               for k, v in sd.items()}
        lo, co, _ = O.gssd_forward(sdg, x, bf16=bf16, **flags)
        ((lo * r1).sum() + (co * r2).sum()).backward()
        return {k: sdg[k].grad.double() for k in keys}
    o_bf, o_32 = oracle_grads('ste'), oracle_grads(False)
    l2 = lambda a, b: float((a - b).norm() / b.norm())
    cos = lambda a, b: float((a * b).sum() / (a.norm() * b.norm()))
    e = {k: (l2(g_bf[k], o_bf[k]), l2(o_bf[k], o_32[k]), cos(g_bf[k], o_bf[k]), cos(o_32[k], o_bf[k]), cos(g_bf[k], g_32[k])) for k in keys}
    print(name, 'bf16 gradients: |HIP - bf16 oracle|, |bf16 oracle - fp32 oracle| (relative L2); cos(HIP, bf16 oracle), '
                'cos(fp32 oracle, bf16 oracle), cos(HIP bf16, HIP fp32)')
    for k, v in e.items():
        print(f'    {k:45s} {v[0]:.2e} {v[1]:.2e}   {v[2]:.4f} {v[3]:.4f} {v[4]:.4f}')
    for k, (a, b, c, c0, _) in e.items():
        assert a <= 1.2 * b + 2e-2, (k, a, b)
        assert c >= c0 - 0.05, (k, c, c0)
    assert e['loc.0.weight'][0] < 3e-2 and e['conf.3.bias'][0] < 3e-2
    net.compute_dtype = 'f32'


def test_bf16_training_steps_reduce_loss(dev):
    """Ten SGD steps of GSSD++ in bf16 storage mode (bf16 forward, mixed-precision backward) on one batch: the loss falls, every
    parameter gets a finite gradient, fp32 master weights move."""
    from models.ssd_multiphase_custom_group import build_ssd
    from layers.modules import MultiBoxLoss
    flags, args = NETS['gssdpp']
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    net.compute_dtype = 'bf16'
    x = synth.synth_images(4, seed=3).to(dev)
    tg = synth.synth_targets(4, seed=3)
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    w0 = net.vgg[0].weight.detach().clone()
    losses = []
    for _ in range(10):
        opt.zero_grad()
        ll, lc = crit(net(x), tg)
        (ll + lc).backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
        opt.step()
        losses.append(float((ll + lc).detach()))
    print('bf16 training losses', [round(v, 4) for v in losses])
    assert losses[-1] < 0.8 * losses[0] and float((net.vgg[0].weight.detach() - w0).abs().max()) > 0


@pytest.mark.parametrize('N,D,C2', [(38 * 38, 64, 256), (19 * 19, 128, 512), (100, 32, 128), (9, 32, 128), (1, 64, 256)])
def test_self_attn_core_bf16_values(dev, N, D, C2):
    """gssd_self_attn_core_bf16v (csrc/flash_attn.hip): fp32 logits, bf16 probabilities and values.  Checked against fp32
    arithmetic on the operands the kernel multiplies: softmax numerators rounded to bf16, g rounded to bf16 (oracle self_attn,
    q mode), within one bf16 ulp of the block's largest output; g^T handed over in the kernel's 32-token key order."""
    from gssd import _lib
    lib = _lib.lib
    B = 2
    gen = torch.Generator().manual_seed(5 + N)
    tp = torch.randn(B, N, 2 * D, generator=gen) * 0.9
    g = torch.randn(B, C2, N, generator=gen)
    Np = (N + 31) // 32 * 32
    m = torch.arange(Np)
    perm = (m & ~31) | (((m >> 2) & 3) << 3) | (((m >> 4) & 1) << 2) | (m & 3)
    gp = torch.zeros(B, C2, Np)
    gp[:, :, perm[:N]] = g
    d_tp, d_g = tp.to(dev), gp.to(dev).to(torch.bfloat16)
    out = torch.full((B, N, C2), float('nan'), device=dev, dtype=torch.bfloat16)
    lse = torch.full((B, N), float('nan'), device=dev)
    _lib.check(lib.gssd_self_attn_core_bf16v(d_tp.data_ptr(), d_g.data_ptr(), out.data_ptr(), B, N, Np, D, C2, lse.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    s = torch.bmm(tp[:, :, :D].double(), tp[:, :, D:].double().transpose(1, 2))
    assert float((lse.cpu().double() - torch.logsumexp(s, dim=-1)).abs().max()) < 2e-3      # (the denominator sums bf16-rounded probabilities) what the training step's backward reads
    p = q(torch.exp(s - s.max(dim=-1, keepdim=True).values).float()).double()
    ref = torch.bmm(p, q(g).double().transpose(1, 2)) / p.sum(dim=-1, keepdim=True)
    got = out.float().cpu().double()
    assert torch.isfinite(got).all()
    assert float((got - ref).abs().max() / ref.abs().max()) <= BF_ULP_LOW


@pytest.mark.parametrize('pool', [None, (2, 2, 0), (3, 1, 1)])
@pytest.mark.parametrize('dout_bf16', [False, True])
def test_bn_backward_mixed(dev, pool, dout_bf16):
    """gssd_bn_bwd_{reduce,apply}_mixed (the bf16 storage mode's BatchNorm backward: reads the forward's bf16 raw map, optionally a bf16
    d(out), writes d(pre-activation) in bf16 and / or fp32) against the fp32 entry points on fp32 copies of the SAME values: the fp32
    outputs, the sums and the parameter gradients are identical bit for bit up to the order of the atomics (1e-6), the bf16 output is
    the fp32 one rounded once."""
    from gssd import ops, _lib
    lib = _lib.lib
    rng = np.random.default_rng(5)
    B, H, Cc = 3, 20, 64
    raw = q(torch.from_numpy(rng.normal(size=(B, H, H, Cc)).astype(np.float32))).to(dev)
    pk, ps, pp = pool if pool else (0, 1, 0)
    Ho = (H + 2 * pp - pk) // ps + 1 if pool else H
    dout = torch.from_numpy(rng.normal(size=(B, Ho, Ho, Cc)).astype(np.float32))
    dout = (q(dout) if dout_bf16 else dout).to(dev)
    gm = torch.from_numpy(rng.uniform(0.5, 1.5, size=Cc).astype(np.float32)).to(dev)
    n = B * H * H
    stats = torch.cat([raw.double().sum((0, 1, 2)), (raw.double() ** 2).sum((0, 1, 2))]).contiguous()
    mean = stats[:Cc] / n
    inv = 1.0 / torch.sqrt(stats[Cc:] / n - mean * mean + 1e-5)
    sc = (gm.double() * inv).float()
    sh = (0.1 - mean * gm.double() * inv).float()
    ref_dz, ref_dg, ref_db, ref_cs = ops.bn_backward(dout, raw, stats, n, gm, sc, sh, pool=pool, want_colsum=True)
    if not pool:            # the plan's no-pool form: sums only, then the masked apply
        pass
    st = torch.cuda.current_stream().cuda_stream
    raw16 = raw.to(torch.bfloat16)
    d_in = dout.to(torch.bfloat16) if dout_bf16 else dout
    dz = torch.zeros_like(raw) if (pool and ps < pk) else torch.full_like(raw, float('nan'))
    dz16 = torch.full(raw.shape, float('nan'), device=dev, dtype=torch.bfloat16)
    sums = torch.zeros(2 * Cc, device=dev, dtype=torch.float64)
    _lib.check(lib.gssd_bn_bwd_reduce_mixed(d_in.data_ptr(), int(dout_bf16), raw16.data_ptr(), sc.data_ptr(), sh.data_ptr(),
                                            dz.data_ptr() if pool else 0, 0, sums.data_ptr(), B, H, H, Cc, Ho, Ho, pk, ps, pp, 1, st))
    ca, cb, cc, dg, db = (torch.empty(Cc, device=dev) for _ in range(5))
    _lib.check(lib.gssd_bn_bwd_finalize_f32(stats.data_ptr(), float(n), sums.data_ptr(), gm.data_ptr(), 1e-5, Cc, ca.data_ptr(), cb.data_ptr(),
                                            cc.data_ptr(), dg.data_ptr(), db.data_ptr(), 0, st))
    cs = torch.zeros(Cc, device=dev, dtype=torch.float64)
    _lib.check(lib.gssd_bn_bwd_apply_mixed(0 if pool else d_in.data_ptr(), int(dout_bf16), dz.data_ptr(), dz16.data_ptr(), raw16.data_ptr(),
                                           0 if pool else sc.data_ptr(), 0 if pool else sh.data_ptr(), 1, ca.data_ptr(), cb.data_ptr(),
                                           cc.data_ptr(), n, Cc, cs.data_ptr(), 1, st))
    assert rel(dz, ref_dz) < 1e-6 and rel(dg, ref_dg) < 1e-6 and rel(db, ref_db) < 1e-6
    # (the column sums of a BatchNorm backward vanish analytically: both are rounding noise of the same size)
    assert float((cs - ref_cs).abs().max()) < 1e-6 * float(dz.abs().sum(dim=(0, 1, 2)).max())
    assert torch.equal(dz16, dz.to(torch.bfloat16))
    if pool and ps >= pk and dout_bf16:
        # non-overlapping pool: the routed gradient handed over as a bf16 map (exact here: d(out) is bf16-representable) -- same results
        dzp = torch.full(raw.shape, float('nan'), device=dev, dtype=torch.bfloat16)
        sums2 = torch.zeros_like(sums)
        _lib.check(lib.gssd_bn_bwd_reduce_mixed(d_in.data_ptr(), 1, raw16.data_ptr(), sc.data_ptr(), sh.data_ptr(), 0, dzp.data_ptr(),
                                                sums2.data_ptr(), B, H, H, Cc, Ho, Ho, pk, ps, pp, 1, st))
        assert rel(sums2, sums) < 1e-6           # (fp32 per-thread partial sums, fp64 atomics in any order)
        dz3 = torch.full_like(raw, float('nan'))
        dz163 = torch.full(raw.shape, float('nan'), device=dev, dtype=torch.bfloat16)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(dzp.data_ptr(), 1, dz3.data_ptr(), dz163.data_ptr(), raw16.data_ptr(), 0, 0, 0, ca.data_ptr(),
                                               cb.data_ptr(), cc.data_ptr(), n, Cc, 0, 1, st))
        assert rel(dz3, ref_dz) < 1e-6 and torch.equal(dz163, dz3.to(torch.bfloat16))
    # store_f32 = 0 leaves dz alone (no-pool form)
    if not pool:
        dz2 = torch.full_like(raw, 7.0)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(d_in.data_ptr(), int(dout_bf16), dz2.data_ptr(), dz16.data_ptr(), raw16.data_ptr(), sc.data_ptr(),
                                               sh.data_ptr(), 1, ca.data_ptr(), cb.data_ptr(), cc.data_ptr(), n, Cc, 0, 0, st))
        assert bool((dz2 == 7.0).all()) and torch.equal(dz16, dz.to(torch.bfloat16))


def test_bf16_helpers_of_the_backward(dev):
    """gssd_cast_rows_f32_bf16 (rows widened with zero pad) and gssd_dcn_im2col_bf16 (the bf16 twin of gssd_dcn_im2col_f32: same sampling
    of the same bf16-representable map, interpolation in fp32, one rounding)."""
    from gssd import _lib
    lib = _lib.lib
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(11)
    x = torch.from_numpy(rng.normal(size=(77, 40)).astype(np.float32)).to(dev)
    y = torch.full((77, 40), float('nan'), device=dev, dtype=torch.bfloat16)
    _lib.check(lib.gssd_cast_rows_f32_bf16(x.data_ptr(), y.data_ptr(), 77, 36, 40, 40, st))
    assert torch.equal(y[:, :36], x[:, :36].to(torch.bfloat16)) and bool((y[:, 36:] == 0).all())
    B, H, Cc, dg = 2, 9, 128, 4
    OMC = 112
    xm = q(torch.from_numpy(rng.normal(size=(B, H, H, Cc)).astype(np.float32))).to(dev)
    om = torch.from_numpy(rng.normal(0, 1.5, size=(B, H, H, OMC)).astype(np.float32)).to(dev)
    cols = torch.empty(B * H * H, 9 * Cc, device=dev)
    cols16 = torch.full((B * H * H, 9 * Cc), float('nan'), device=dev, dtype=torch.bfloat16)
    _lib.check(lib.gssd_dcn_im2col_f32(xm.data_ptr(), om.data_ptr(), cols.data_ptr(), B, H, H, Cc, dg, OMC, st))
    _lib.check(lib.gssd_dcn_im2col_bf16(xm.to(torch.bfloat16).data_ptr(), om.data_ptr(), cols16.data_ptr(), B, H, H, Cc, dg, OMC, st))
    assert torch.equal(cols16, cols.to(torch.bfloat16))


@pytest.mark.parametrize('B,N,D,C2', [(2, 1444, 64, 256), (3, 361, 64, 256), (2, 100, 32, 128), (1, 65, 64, 256), (2, 9, 32, 128), (2, 361, 128, 512)])
def test_self_attn_flash_bwd(dev, B, N, D, C2):
    """gssd_self_attn_flash_bwd_bf16 (csrc/sa_flash_bwd.hip) against the float64 backward of attn_g = softmax(theta phi^T) g over the same
    operands: fp32 theta / phi, bf16-rounded g and d(attn_g); lse and D_i = <d(attn_g)_i, attn_g_i> are inputs, as the plan hands them
    over.  Inside, P and dS are rounded to bf16 before they are contracted (relative 2^-9 per element, uncorrelated): 5e-3 of the
    tensors' scale in L2.  Ragged N exercises the masked last blocks of both the owned and the streamed side.
    These are the workload sizes; every instance at its tile and block edges, per token: tests/test_gpu_attn_bwd.py::test_flash_bwd_bf16."""
    from gssd import _lib
    rng = np.random.default_rng(N + D)
    th = torch.from_numpy(rng.normal(0, 0.6, size=(B, N, D)).astype(np.float32))
    ph = torch.from_numpy(rng.normal(0, 0.6, size=(B, N, D)).astype(np.float32))
    g = q(torch.from_numpy(rng.normal(size=(B, N, C2)).astype(np.float32)))
    dag = q(torch.from_numpy(rng.normal(size=(B, N, C2)).astype(np.float32)))
    S = torch.bmm(th.double(), ph.double().transpose(1, 2))
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1))
    O = torch.bmm(P, g.double())
    Dv = (dag.double() * O).sum(-1)
    dP = torch.bmm(dag.double(), g.double().transpose(1, 2))
    dS = P * (dP - Dv.unsqueeze(-1))
    ref = torch.cat([torch.bmm(dS, ph.double()), torch.bmm(dS.transpose(1, 2), th.double()), torch.bmm(P.transpose(1, 2), dag.double())], dim=-1)
    tp = torch.cat([th, ph], dim=-1).contiguous().to(dev)
    out = torch.full((B, N, 2 * D + C2), float('nan'), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    tph, tpl = torch.empty_like(tp, dtype=torch.bfloat16), torch.empty_like(tp, dtype=torch.bfloat16)
    _lib.check(_lib.lib.gssd_cast_split_f32_bf16(tp.data_ptr(), tph.data_ptr(), tpl.data_ptr(), tp.numel(), st))
    assert torch.equal(tph, tp.to(torch.bfloat16)) and torch.equal(tpl, (tp - tph.float()).to(torch.bfloat16))
    assert _lib.lib.gssd_self_attn_flash_bwd_supported(D, C2) == 1 and _lib.lib.gssd_self_attn_flash_bwd_supported(256, 1024) == 0
    g16, dag16, lse32, dv32 = g.to(dev).to(torch.bfloat16), dag.to(dev).to(torch.bfloat16), lse.float().to(dev), Dv.float().to(dev)
    for form, lo in (('logits as hi.hi + hi.lo + lo.hi on bf16 MFMA', tpl.data_ptr()), ('logits on fp32 MFMA', 0)):
        out.fill_(float('nan'))
        _lib.check(_lib.lib.gssd_self_attn_flash_bwd_bf16(tp.data_ptr(), tph.data_ptr(), lo, g16.data_ptr(), dag16.data_ptr(), lse32.data_ptr(),
                                                          dv32.data_ptr(), out.data_ptr(), B, N, D, C2, st))
        got = out.double().cpu()
        assert bool(torch.isfinite(got).all())
        for name, sl in (('d theta', slice(0, D)), ('d phi', slice(D, 2 * D)), ('d g', slice(2 * D, None))):
            e = l2rel(got[..., sl], ref[..., sl])
            print(f'    flash backward N = {N}, {form}: {name} relative L2 {e:.2e}')
            assert e < 5e-3, (name, e)


def test_training_soak_batch32():
    """scripts/train_soak.py: 30 SGD steps of GSSD++ on one batch of 32 (the BENCHMARKED batch: every large-map kernel of the backward,
    the bf16 gradient maps, the flash-style attention backward at N = 1444) in fp32 and in the bf16 storage mode, in a process of its
    own -- both losses stay finite and at least halve (the script asserts it)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'train_soak.py'), '30'], capture_output=True, text=True, timeout=900)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stderr[-2000:]
    assert 'ratio bf16 / f32' in r.stdout


@pytest.mark.parametrize('name,flags,args', [
    ('g1', dict(groups_vgg=1, groups_extra=1), (True, 1, 1, 1, True, False, False, 0, 1, False, False, 1)),
    ('g2pp', dict(groups_vgg=2, groups_extra=2, use_self_attention=True, use_self_attention_base=True, num_dcn_layers=1, groups_dcn=4,
                  dcn_cat_sab=True), (True, 2, 2, 1, True, True, True, 1, 4, True, False, 1)),
    # --feature_scale 2 with Self_Attn / DCN: the (256, 1024) attention block as two launches of 512 g channels
    ('fs2pp', dict(feature_scale=2, use_self_attention=True, use_self_attention_base=True, num_dcn_layers=1, groups_dcn=4, dcn_cat_sab=True),
     (True, 4, 4, 2, True, True, True, 1, 4, True, False, 1))])
def test_bf16_group_counts(dev, name, flags, args):
    """--groups_vgg / --groups_extra 1 and 2 in the bf16 storage mode (the input pack writes 12 -> 16 / 6 -> 8 channels per group; every
    layer runs the generic bf16 kernels).  End to end at B = 2 the bf16 graph is far from the fp32 one (ill-conditioned small-batch
    BatchNorms, tests above): the HIP result must sit well inside that gap around the bf16 oracle."""
    from models.ssd_multiphase_custom_group import build_ssd
    net = build_ssd('train', 300, 2, *args)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    net.compute_dtype = 'bf16'
    x = synth.synth_images(2, seed=5)
    with torch.no_grad():
        loc, conf, _ = net(x.to(dev))
        lo, co, _ = O.gssd_forward(sd, x, bf16=True, **flags)
        lo32, co32, _ = O.gssd_forward(sd, x, **flags)
    assert torch.isfinite(loc).all() and torch.isfinite(conf).all()
    e, gap = max(rel(loc, lo), rel(conf, co)), max(rel(lo, lo32), rel(co, co32))
    print(name, f'bf16 HIP vs bf16 oracle {e:.3f}; bf16 oracle vs fp32 oracle {gap:.3f}')
    assert e < 0.6 * gap, (e, gap)

