"""The standalone DCNv2 operator (gssd/dcn_op.py, gssd.modules.DCN / DCNv2, layers/dcn_v2_custom.py) without a GPU: module state
against the reference's formulas (layers/dcn_v2_custom.py:18-77), the seeded init sequence of the engine's 3x3 DCN, the geometry
errors, the op's argument checks, no CPU fallback, and the test-local float64 restatement the GPU tests use for anisotropic cases."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gssd import _lib
from gssd.modules import DCN, DCNv2
from oracle import gssd_oracle as O


def dcn_v2_ref(x, offset, mask, weight, bias, stride, padding, dilation, dg):
    """float64 DCNv2 with separate (h, w) stride / padding / dilation (the oracle takes one of each): per tap, bilinear sample with
    the gate -1 < y < H, -1 < x < W and corners outside the map contributing 0; modulated; then the contraction."""
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    B, Cin, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    K = kh * kw
    Ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    cpg = Cin // dg
    xf = x.reshape(B, dg, cpg, H * W)
    off = offset.reshape(B, dg, K, 2, Ho, Wo)
    msk = mask.reshape(B, dg, K, Ho, Wo)
    ys = (torch.arange(Ho, dtype=x.dtype) * sh - ph).view(1, 1, Ho, 1)
    xs = (torch.arange(Wo, dtype=x.dtype) * sw - pw).view(1, 1, 1, Wo)
    cols = []
    for k in range(K):
        i, j = divmod(k, kw)
        py = ys + i * dh + off[:, :, k, 0]
        px = xs + j * dw + off[:, :, k, 1]
        gate = (py > -1) & (px > -1) & (py < H) & (px < W)
        y0, x0 = torch.floor(py), torch.floor(px)
        ly, lx = py - y0, px - x0
        val = 0
        for yy, xx, wt in ((y0, x0, (1 - ly) * (1 - lx)), (y0, x0 + 1, (1 - ly) * lx), (y0 + 1, x0, ly * (1 - lx)), (y0 + 1, x0 + 1, ly * lx)):
            inside = gate & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            lin = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(B, dg, 1, Ho * Wo).expand(B, dg, cpg, Ho * Wo)
            val = val + torch.gather(xf, 3, lin) * (wt * inside.to(x.dtype)).view(B, dg, 1, Ho * Wo)
        cols.append(val * msk[:, :, k].reshape(B, dg, 1, Ho * Wo))
    cols = torch.stack(cols, 3).reshape(B, Cin * K, Ho * Wo)               # (c, k) like weight.view(Cout, Cin*K)
    out = torch.matmul(weight.reshape(Cout, Cin * K), cols)
    if bias is not None:
        out = out + bias.view(1, Cout, 1)
    return out.view(B, Cout, Ho, Wo)


def ref_state(cin, cout, k, s, p, dg, with_offset_conv):
    """layers/dcn_v2_custom.py: state-dict shapes of DCNv2 / DCN for a geometry."""
    kh, kw = (k, k) if isinstance(k, int) else k
    st = {'weight': (cout, cin, kh, kw), 'bias': (cout,)}
    if with_offset_conv:
        st['conv_offset_mask.weight'] = (dg * 3 * kh * kw, cin, kh, kw)
        st['conv_offset_mask.bias'] = (dg * 3 * kh * kw,)
    return st


@pytest.mark.parametrize('cin,cout,k,s,p,dg', [(8, 4, 1, 1, 0, 1), (8, 6, 3, 2, 1, 2), (16, 8, 5, 1, 2, 4), (12, 4, 3, 1, 1, 4),
                                               (6, 3, 3, 2, 0, 2)])
def test_state_dict_matches_reference(cin, cout, k, s, p, dg):
    m = DCN(cin, cout, k, s, p, deformable_groups=dg)
    assert {n: tuple(t.shape) for n, t in m.state_dict().items()} == ref_state(cin, cout, k, s, p, dg, True)
    cm = m.conv_offset_mask
    assert cm.kernel_size == (k, k) and cm.stride == (s, s) and cm.padding == (p, p) and cm.dilation == (1, 1)
    assert not cm.weight.detach().any() and not cm.bias.detach().any() and not m.bias.detach().any()
    bound = 1.0 / math.sqrt(cin * k * k)
    assert float(m.weight.detach().abs().max()) <= bound
    v = DCNv2(cin, cout, k, s, p, deformable_groups=dg)
    assert {n: tuple(t.shape) for n, t in v.state_dict().items()} == ref_state(cin, cout, k, s, p, dg, False)


def test_dcnv2_rectangular_kernel_and_pairs():
    v = DCNv2(8, 4, (3, 1), (2, 1), (1, 0), dilation=(1, 2), deformable_groups=2)
    assert {n: tuple(t.shape) for n, t in v.state_dict().items()} == ref_state(8, 4, (3, 1), None, None, 2, False)
    assert (v.kernel_size, v.stride, v.padding, v.dilation) == ((3, 1), (2, 1), (1, 0), (1, 2))
    assert float(v.weight.detach().abs().max()) <= 1.0 / math.sqrt(8 * 3)


def test_engine_dcn_init_sequence_unchanged():
    """3/1/1/1: the same RNG draws in the same order as before (seeded build_ssd weights stay what they were)."""
    torch.manual_seed(1234)
    m = DCN(16, 8, 3, 1, 1, deformable_groups=4)
    after = torch.rand(3)
    torch.manual_seed(1234)
    w = torch.empty(8, 16, 3, 3).uniform_(-1.0 / math.sqrt(16 * 9), 1.0 / math.sqrt(16 * 9))
    b = torch.zeros(8)
    cm = torch.nn.Conv2d(16, 4 * 27, kernel_size=3, stride=1, padding=1, bias=True)
    want_after = torch.rand(3)
    assert torch.equal(m.weight.detach(), w) and torch.equal(m.bias.detach(), b) and torch.equal(after, want_after)
    assert tuple(m.conv_offset_mask.weight.shape) == tuple(cm.weight.shape)
    assert m.kernel_size == (3, 3) and m.stride == (1, 1) and m.padding == (1, 1) and m.dilation == (1, 1) and m.is_engine_geometry()
    assert not DCN(16, 8, 3, 2, 1).is_engine_geometry()


def test_dcn_geometry_errors():
    with pytest.raises(NotImplementedError):
        DCN(8, 4, (3, 1), 1, 1)
    with pytest.raises(NotImplementedError):
        DCN(8, 4, 3, (2, 1), 1)
    with pytest.raises(NotImplementedError):
        DCN(8, 4, 3, 1, (1, 0))
    m = DCN(8, 4, 3, 1, 1, dilation=2)                         # the reference's offset conv has no dilation: 5 x 5 against 3 x 3
    with pytest.raises(ValueError, match='dilation'):
        m(torch.zeros(1, 8, 5, 5))
    # k = 1: dilation does not change the size, so the check passes and the device check follows
    with pytest.raises(_lib.GssdError):
        DCN(8, 4, 1, 1, 0, dilation=2)(torch.zeros(1, 8, 5, 5))


def test_engine_refuses_non_engine_dcn_geometry():
    from gssd import plan_ops

    class Net:
        dcn_list = [DCN(8, 4, 3, 2, 1)]

    class Eng:
        net = Net()

    fake = type('F', (), {'eng': Eng(), 'B': 1})()
    with pytest.raises(_lib.GssdError, match='3x3 / stride 1'):
        plan_ops.PlanOpsMixin._dcn(fake, 0, None, 5, 8)


def test_op_checks_channels_and_device():
    from gssd.dcn_op import dcn_v2_conv
    x, w, b = torch.zeros(1, 8, 6, 6), torch.zeros(4, 8, 3, 3), torch.zeros(4)
    off, msk = torch.zeros(1, 2 * 2 * 9, 6, 6), torch.zeros(1, 2 * 9, 6, 6)
    with pytest.raises(ValueError, match='offset'):
        dcn_v2_conv(x, off[:, :-2], msk, w, b, 1, 1, 1, 2)
    with pytest.raises(ValueError, match='mask'):
        dcn_v2_conv(x, off, msk[:, :-1], w, b, 1, 1, 1, 2)
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        dcn_v2_conv(x, off, msk, w, b, 1, 1, 1, 2)
    from layers.dcn_v2_custom import DCN as LD
    with pytest.raises(_lib.GssdError):
        LD(8, 4, 3, 1, 1)(x)


def test_layers_exports():
    import layers.dcn_v2_custom as L
    from gssd import dcn_op
    assert L.dcn_v2_conv is dcn_op.dcn_v2_conv and L._DCNv2 is dcn_op._DCNv2 and issubclass(L.DCN, L.DCNv2)
    assert {'DCN', 'DCNv2', 'dcn_v2_conv', '_DCNv2'} <= set(L.__all__)


@pytest.mark.parametrize('B,Cc,H,W,Cout,dg,k,stride,pad,dil', [
    (1, 8, 11, 10, 3, 2, 3, 2, 1, 1), (1, 4, 10, 12, 3, 1, 3, 1, 2, 2), (1, 6, 9, 9, 2, 3, 3, 2, 2, 2), (2, 4, 6, 7, 3, 2, 1, 1, 0, 1)])
def test_local_restatement_agrees_with_oracle(B, Cc, H, W, Cout, dg, k, stride, pad, dil):
    rng = np.random.default_rng(B * 1000 + H * 10 + k)
    Ho = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    x = torch.from_numpy(rng.normal(size=(B, Cc, H, W)))
    off = torch.from_numpy(rng.normal(0, 2.5, size=(B, 2 * dg * k * k, Ho, Wo)))
    msk = torch.from_numpy(rng.uniform(0, 1, size=(B, dg * k * k, Ho, Wo)))
    w = torch.from_numpy(rng.normal(0, 0.2, size=(Cout, Cc, k, k)))
    b = torch.from_numpy(rng.normal(size=(Cout,)))
    a = dcn_v2_ref(x, off, msk, w, b, (stride, stride), (pad, pad), (dil, dil), dg)
    o = O.dcn_v2_conv(x, off, msk, w, b, stride, pad, dil, dg)
    assert torch.allclose(a, o, rtol=0, atol=1e-12)
    # integer offsets and a unit mask: an ordinary (anisotropic) conv
    s2, p2, d2 = (2, 1), (1, 0), (1, 2)
    Ho2 = (H + 2 * p2[0] - d2[0] * (k - 1) - 1) // s2[0] + 1
    Wo2 = (W + 2 * p2[1] - d2[1] * (k - 1) - 1) // s2[1] + 1
    z = torch.zeros(B, 2 * dg * k * k, Ho2, Wo2, dtype=torch.float64)
    one = torch.ones(B, dg * k * k, Ho2, Wo2, dtype=torch.float64)
    want = F.conv2d(x, w, b, s2, p2, d2)
    assert torch.allclose(dcn_v2_ref(x, z, one, w, b, s2, p2, d2, dg), want, rtol=0, atol=1e-12)
