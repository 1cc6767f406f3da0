"""The standalone DCNv2 operator on the MI355X (gssd/dcn_op.py over csrc/dcn_geo.hip + the existing 1x1 contraction): forward against
the two CPU restatements (float64 oracle, scalar C) for every geometry of tests/test_dcn_oracles.py and more, the exact border gates,
gradients against float64 autograd through the oracle, the DCN module with its offset conv, the engine's fused kernel on the shared
3x3 case, and batch chunking of the column workspace."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dcn_scalar
from oracle import gssd_oracle as O
from test_dcn_op_cpu import dcn_v2_ref

pytestmark = pytest.mark.gpu

TOL = 1e-4


def rel(a, b):
    a = a.detach().cpu().double() if torch.is_tensor(a) else torch.as_tensor(np.asarray(a, np.float64))
    b = b.detach().cpu().double() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b, np.float64))
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def case(seed, B, Cc, H, W, Cout, dg, kh, kw, stride, pad, dil, std):
    """fp32 inputs; offsets on a 1/256 grid shifted by 1/512 so no sample lies on a cell edge (fp32 and float64 take the same floor)."""
    (sh, sw), (ph, pw), (dh, dw) = stride, pad, dil
    rng = np.random.default_rng(seed)
    Ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    K = kh * kw
    x = rng.normal(size=(B, Cc, H, W)).astype(np.float32)
    off = (np.round(rng.normal(0, std, size=(B, 2 * K * dg, Ho, Wo)) * 256) / 256 + 1 / 512).astype(np.float32)
    msk = rng.uniform(0, 1, size=(B, K * dg, Ho, Wo)).astype(np.float32)
    w = rng.normal(0, 0.2, size=(Cout, Cc, kh, kw)).astype(np.float32)
    b = rng.normal(size=(Cout,)).astype(np.float32)
    return [torch.from_numpy(t) for t in (x, off, msk, w, b)]


def pair(v):
    return v if isinstance(v, tuple) else (v, v)


# (B, C, H, W, Cout, dg, k, stride, pad, dil, offset std): the seven geometries of test_two_restatements_agree, then more
GEOMS = [
    (2, 8, 7, 7, 5, 1, 3, 1, 1, 1, 2.5),
    (1, 8, 6, 9, 4, 2, 3, 1, 1, 1, 4.0),
    (2, 16, 9, 8, 6, 4, 3, 1, 1, 1, 1.0),
    (1, 8, 11, 10, 3, 2, 3, 2, 1, 1, 2.0),
    (1, 4, 10, 12, 3, 1, 3, 1, 2, 2, 2.0),
    (1, 6, 9, 9, 2, 3, 3, 2, 2, 2, 3.0),
    (1, 4, 5, 5, 2, 1, 3, 1, 0, 1, 0.7),
    (2, 8, 8, 9, 4, 2, (3, 1), 1, (1, 0), 1, 2.0),        # rectangular kernel
    (2, 6, 7, 6, 5, 2, 3, 1, 1, 1, 3.0),                  # C = 6, dg = 2: three channels per group, C not a multiple of 4
    (2, 8, 9, 11, 6, 2, 5, 1, 2, 1, 1.5),                 # 5 x 5
    (3, 12, 6, 7, 8, 4, 1, 1, 0, 1, 1.0),                 # 1 x 1
    (1, 160, 12, 10, 40, 2, 3, 1, 1, 1, 1.0),             # more than 64 channels per group
]


@pytest.mark.parametrize('g', GEOMS, ids=[f'g{i}' for i in range(len(GEOMS))])
def test_forward_matches_both_restatements(dev, g):
    from gssd.dcn_op import dcn_v2_conv
    B, Cc, H, W, Cout, dg, k, s, p, d, std = g
    kh, kw = pair(k)
    x, off, msk, w, b = case(B * 100 + H + Cc, B, Cc, H, W, Cout, dg, kh, kw, pair(s), pair(p), pair(d), std)
    out = dcn_v2_conv(x.to(dev), off.to(dev), msk.to(dev), w.to(dev), b.to(dev), s, p, d, dg)
    if kh == kw and isinstance(p, int):
        ref = O.dcn_v2_conv(x.double(), off.double(), msk.double(), w.double(), b.double(), s, p, d, dg)
        sc = dcn_scalar.dcn_v2_conv(x, off, msk, w, b, s, p, d, dg)
        assert out.shape == ref.shape and rel(out, sc) <= 1e-5
    else:
        ref = dcn_v2_ref(x.double(), off.double(), msk.double(), w.double(), b.double(), pair(s), pair(p), pair(d), dg)
    assert out.shape == ref.shape and rel(out, ref) <= 1e-5, rel(out, ref)


def test_forward_anisotropic(dev):
    from gssd.dcn_op import dcn_v2_conv
    s, p, d = (2, 1), (0, 2), (1, 2)
    x, off, msk, w, b = case(77, 2, 8, 11, 9, 6, 2, 3, 3, s, p, d, 2.5)
    out = dcn_v2_conv(x.to(dev), off.to(dev), msk.to(dev), w.to(dev), b.to(dev), s, p, d, 2)
    ref = dcn_v2_ref(x.double(), off.double(), msk.double(), w.double(), b.double(), s, p, d, 2)
    assert out.shape == ref.shape and rel(out, ref) <= 1e-5


def test_border_samples_exactly_on_the_gates(dev):
    """tests/test_dcn_oracles.py's exact border cases, through the HIP sampler."""
    from gssd.dcn_op import dcn_v2_conv
    H = W = 5
    x = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W).to(dev)
    w = torch.zeros(1, 1, 3, 3)
    w[0, 0, 1, 1] = 1.0
    w = w.to(dev)
    msk = torch.ones(1, 9, H, W, device=dev)
    for dy, dx, expect in [(-1.0, 0.0, 0.0), (-0.75, 0.0, 0.25 * 1.0), (4.0, 0.0, 21.0), (4.5, 0.0, 0.5 * 21.0), (5.0, 0.0, 0.0),
                           (0.0, -0.5, 0.5 * 1.0), (0.0, 4.5, 0.5 * 5.0)]:
        off = torch.zeros(1, 18, H, W)
        off[0, 8], off[0, 9] = dy, dx
        a = dcn_v2_conv(x, off.to(dev), msk, w, torch.zeros(1, device=dev), 1, 1, 1, 1)
        assert float(a[0, 0, 0, 0]) == np.float32(expect), (dy, dx, float(a[0, 0, 0, 0]))


GRAD_GEOMS = [(2, 8, 7, 7, 5, 2, 3, 1, 1, 1, 2.0), (1, 8, 11, 10, 6, 2, 3, 2, 1, 1, 2.0), (1, 4, 10, 12, 3, 1, 3, 1, 2, 2, 2.0),
              (2, 6, 7, 6, 5, 2, 1, 1, 0, 1, 1.5)]


@pytest.mark.parametrize('g', GRAD_GEOMS, ids=[f'g{i}' for i in range(len(GRAD_GEOMS))])
def test_gradients_vs_float64_autograd(dev, g):
    from gssd.dcn_op import dcn_v2_conv
    B, Cc, H, W, Cout, dg, k, s, p, d, std = g
    ts = case(B * 7 + H, B, Cc, H, W, Cout, dg, k, k, (s, s), (p, p), (d, d), std)
    gy = torch.randn(B, Cout, (H + 2 * p - d * (k - 1) - 1) // s + 1, (W + 2 * p - d * (k - 1) - 1) // s + 1, generator=torch.Generator().manual_seed(5))
    r = [t.double().requires_grad_() for t in ts]
    O.dcn_v2_conv(*r, s, p, d, dg).backward(gy.double())
    h = [t.to(dev).requires_grad_() for t in ts]
    dcn_v2_conv(*h, s, p, d, dg).backward(gy.to(dev))
    for name, a, b in zip(('input', 'offset', 'mask', 'weight', 'bias'), h, r):
        assert rel(a.grad, b.grad) <= TOL, (name, rel(a.grad, b.grad))
    # inputs that do not require grad get none (and the others are unchanged)
    h2 = [t.to(dev) for t in ts]
    h2[3].requires_grad_()
    h2[1].requires_grad_()
    dcn_v2_conv(*h2, s, p, d, dg).backward(gy.to(dev))
    assert h2[0].grad is None and h2[2].grad is None and h2[4].grad is None
    assert rel(h2[3].grad, r[3].grad) <= TOL and rel(h2[1].grad, r[1].grad) <= TOL


def dcn_module_ref(m, x):
    """float64 autograd through the reference's DCN.forward composition with the module's stride / padding."""
    w_om, b_om, w, b = (t.detach().cpu().double().requires_grad_() for t in (m.conv_offset_mask.weight, m.conv_offset_mask.bias, m.weight,
                                                                             m.bias))
    xr = x.detach().cpu().double().requires_grad_()
    om = F.conv2d(xr, w_om, b_om, m.stride, m.padding)
    o1, o2, mk = torch.chunk(om, 3, dim=1)
    offset = torch.cat((o1, o2), dim=1)
    out = O.dcn_v2_conv(xr, offset, torch.sigmoid(mk), w, b, m.stride[0], m.padding[0], m.dilation[0], m.deformable_groups)
    return out, offset, (xr, w_om, b_om, w, b)


@pytest.mark.parametrize('k,s,p,dg', [(3, 1, 1, 2), (3, 2, 1, 1), (1, 1, 0, 2)])
def test_dcn_module(dev, k, s, p, dg):
    from gssd.modules import DCN
    torch.manual_seed(k * 10 + s)
    B, Cc, H, W, Cout = 2, 8, 9, 8, 6
    m = DCN(Cc, Cout, k, s, p, deformable_groups=dg)
    x = torch.randn(B, Cc, H, W)
    xd = x.to(dev)
    # zero-initialised offset conv: offsets 0, mask 0.5 -> 0.5 * conv2d + b
    m.bias.data.normal_()
    md = m.to(dev)
    out, offset = md(xd)
    ident = 0.5 * F.conv2d(x.double(), m.weight.detach().cpu().double(), None, s, p) + m.bias.detach().cpu().double().view(1, -1, 1, 1)
    assert rel(out, ident) <= 1e-5 and not offset.detach().any()
    with torch.no_grad():
        m.conv_offset_mask.weight.normal_(0, 0.15)
        m.conv_offset_mask.bias.normal_(0, 0.5)
    m.zero_grad()
    xd = x.to(dev).requires_grad_()
    out, offset = md(xd)
    ro, roff, leaves = dcn_module_ref(md, x)
    assert rel(out, ro) <= 1e-5 and rel(offset, roff) <= 1e-5
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(1))
    go = torch.randn(offset.shape, generator=torch.Generator().manual_seed(2))
    (out * gy.to(dev)).sum().add_((offset * go.to(dev)).sum()).backward()
    ((ro * gy.double()).sum() + (roff * go.double()).sum()).backward()
    for name, a, b in zip(('x', 'conv_offset_mask.weight', 'conv_offset_mask.bias', 'weight', 'bias'),
                          (xd, md.conv_offset_mask.weight, md.conv_offset_mask.bias, md.weight, md.bias), leaves):
        assert rel(a.grad, b.grad) <= TOL, (name, rel(a.grad, b.grad))
    # a loss on the offsets alone reaches conv_offset_mask
    md.zero_grad()
    _, offset = md(x.to(dev))
    offset.sum().backward()
    assert md.conv_offset_mask.weight.grad.abs().max() > 0 and md.conv_offset_mask.bias.grad.abs().max() > 0
    assert md.weight.grad is None and md.bias.grad is None


def test_matches_engine_fused_kernel(dev):
    """The standalone 3 / 1 / 1 / 1 forward against ops.dcn_forward (csrc/dcn_fused.hip) on one small detector-like shape."""
    from gssd import ops
    from gssd.dcn_op import dcn_v2_conv
    torch.manual_seed(3)
    B, Cc, H, Cout, dg = 2, 128, 9, 32, 4
    x = torch.randn(B, Cc, H, H, device=dev)
    om = torch.randn(B, 27 * dg, H, H, device=dev) * 1.5
    w = torch.randn(Cout, Cc, 3, 3, device=dev) * 0.05
    b = torch.randn(Cout, device=dev)
    ref = ops.dcn_forward(x.permute(0, 2, 3, 1).contiguous(), om.permute(0, 2, 3, 1).contiguous(), w, b, dg).permute(0, 3, 1, 2)
    out = dcn_v2_conv(x, om[:, :18 * dg].contiguous(), torch.sigmoid(om[:, 18 * dg:]).contiguous(), w, b, 1, 1, 1, dg)
    assert rel(out, ref) <= 1e-5


def test_chunked_batch_is_the_unchunked_result(dev, monkeypatch):
    from gssd import dcn_op
    B, Cc, H, W, Cout, dg, k = 3, 8, 8, 8, 8, 2, 3
    ts = case(11, B, Cc, H, W, Cout, dg, k, k, (1, 1), (1, 1), (1, 1), 2.0)
    gy = torch.randn(B, Cout, H, W, generator=torch.Generator().manual_seed(4)).to(dev)

    def run():
        h = [t.to(dev).requires_grad_() for t in ts]
        out = dcn_op.dcn_v2_conv(*h, 1, 1, 1, dg)
        out.backward(gy)
        return [out.detach()] + [t.grad for t in h]
    whole = run()
    monkeypatch.setattr(dcn_op, 'WORKSPACE_BYTES', H * W * k * k * Cc * 4)       # one image per chunk: 3 chunks
    assert len(dcn_op._chunks(B, H * W * k * k * Cc * 4)) == 3
    part = run()
    names = ('out', 'input', 'offset', 'mask', 'weight', 'bias')
    for name, a, b in zip(names, part, whole):
        if name in ('offset', 'mask'):
            assert torch.equal(a, b), name
        else:
            assert rel(a, b) <= 1e-6, (name, rel(a, b))
