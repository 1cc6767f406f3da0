"""The standalone any-geometry DCNv2 op (gssd/dcn_op.py: csrc/dcn_geo.hip sampling + the existing 1x1 contraction), forward and
forward + backward, timed with device events after a warm-up.  Shapes: the detector's (B=32, 38x38, 1024 -> 512, dg 4, 3x3) next to the
engine's fused kernel gssd_dcn_forward_f32 on the same tensors, and one stride-2 downsampler."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'grouped-ssd-pytorch_amd'))
import torch  # noqa: E402
from gssd import ops  # noqa: E402
from gssd.dcn_op import dcn_v2_conv  # noqa: E402

dev = torch.device('cuda:0')
N = int(os.environ.get('N', 10))


def timed(fn, n=N):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def case(B, H, C, Cout, dg, k, s, p, oms=0.8):
    torch.manual_seed(0)
    Ho = (H + 2 * p - k) // s + 1
    x = torch.randn(B, C, H, H, device=dev)
    om = torch.randn(B, 3 * dg * k * k, Ho, Ho, device=dev) * oms
    off = om[:, :2 * dg * k * k].contiguous()
    msk = torch.sigmoid(om[:, 2 * dg * k * k:]).contiguous()
    w = torch.randn(Cout, C, k, k, device=dev) * 0.01
    b = torch.randn(Cout, device=dev)
    return x, om, off, msk, w, b, Ho


def bench(name, B, H, C, Cout, dg, k, s, p, fused=False):
    x, om, off, msk, w, b, Ho = case(B, H, C, Cout, dg, k, s, p)
    fl = 2.0 * B * Ho * Ho * Cout * k * k * C
    fwd = timed(lambda: dcn_v2_conv(x, off, msk, w, b, s, p, 1, dg))
    xs, offs, msks, ws, bs = (t.clone().requires_grad_() for t in (x, off, msk, w, b))
    gy = torch.randn(B, Cout, Ho, Ho, device=dev)
    fb = timed(lambda: dcn_v2_conv(xs, offs, msks, ws, bs, s, p, 1, dg).backward(gy))
    line = f'{name}: forward {fwd:.3f} ms ({fl / fwd / 1e9:.1f} TFLOP/s)  forward+backward {fb:.3f} ms'
    if fused:
        xh, omh = x.permute(0, 2, 3, 1).contiguous(), om.permute(0, 2, 3, 1).contiguous()
        wp = ops.dcn_pack_weight(w, dg)
        fz = timed(lambda: ops.dcn_forward(xh, omh, w, b, dg, w_packed=wp))
        line += f'  | engine gssd_dcn_forward_f32 (NHWC, packed weights) {fz:.3f} ms'
    print(line, flush=True)


bench('detector B=32 38x38 1024->512 dg4 3x3', int(os.environ.get('B', 32)), 38, 1024, 512, 4, 3, 1, 1, fused=True)
bench('stride-2 B=32 38x38 512->512 dg4 3x3 s2', int(os.environ.get('B', 32)), 38, 512, 512, 4, 3, 2, 1)
