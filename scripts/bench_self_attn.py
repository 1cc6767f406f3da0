"""The standalone Self_Attn module (gssd/self_attn_op.py: csrc/sa_any.hip under the existing convs), forward and forward + backward, timed
with device events after a warm-up, next to a few-line ATen restatement on the device (conv2d / bmm / softmax, as
tests/aten_shadow.py::_self_attn).  Shapes (B, C, H, max_pool_factor): (32, 512, 38, 1), (8, 128, 64, 1), (8, 128, 64, 2); module only at
(2, 128, 150, 1), where the ATen path would hold about 8 GB of maps.  At (32, 512, 38) the any-size forward entry is also timed against
the specialised gssd_self_attn_core_kv_f32 instance (64, 256) on the same buffers, the two alternating.  Prints one markdown table."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), '..', 'grouped-ssd-pytorch_amd'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from gssd._lib import check, lib  # noqa: E402
from gssd.modules import Self_Attn  # noqa: E402

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


def aten_self_attn(sa, x):
    """layers/self_attn.py:46-89 in eval mode (no power iteration), ATen only."""
    def w(m):
        wm = m.weight_orig.view(m.weight_orig.shape[0], -1)
        return m.weight_orig / torch.dot(m.weight_u, torch.mv(wm, m.weight_v))
    B, ch, h, _ = x.shape
    pool = max(int(h // sa.max_pool_factor), 1)
    theta = F.conv2d(x, w(sa.snconv1x1_theta), sa.snconv1x1_theta.bias).view(B, ch // 8, h * h)
    phi = F.adaptive_avg_pool2d(F.conv2d(x, w(sa.snconv1x1_phi), sa.snconv1x1_phi.bias), pool).view(B, ch // 8, -1)
    attn = torch.softmax(torch.bmm(theta.permute(0, 2, 1), phi), dim=-1)
    g = F.adaptive_avg_pool2d(F.conv2d(x, w(sa.snconv1x1_g), sa.snconv1x1_g.bias), pool).view(B, ch // 2, -1)
    attn_g = torch.bmm(g, attn.permute(0, 2, 1)).view(B, ch // 2, h, h)
    attn_g = F.conv2d(attn_g, w(sa.snconv1x1_attn), sa.snconv1x1_attn.bias)
    return x + sa.sigma * attn_g, sa.sigma * attn_g


def make(B, Cc, H, mpf):
    torch.manual_seed(0)
    m = Self_Attn(Cc, mpf)
    for n in ('theta', 'phi', 'g', 'attn'):                      # u / v converged, so the weights are normalised and the softmax is not saturated
        c = getattr(m, 'snconv1x1_' + n)
        wm = c.weight_orig.detach().view(c.out_channels, -1)
        u, v = c.weight_u, c.weight_v
        for _ in range(10):
            v = F.normalize(wm.t() @ u, dim=0)
            u = F.normalize(wm @ v, dim=0)
        c.weight_u.copy_(u)
        c.weight_v.copy_(v)
    with torch.no_grad():
        m.sigma.fill_(0.7)
    return m.to(dev).eval(), torch.randn(B, Cc, H, H, device=dev)


def fwd_bwd(fn, m, x):
    xg = x.clone().requires_grad_()

    def step():
        m.zero_grad(set_to_none=True)
        xg.grad = None
        out, o2 = fn(xg)
        (out.sum() + o2.sum()).backward()
    return step


def bench(B, Cc, H, mpf, aten=True):
    m, x = make(B, Cc, H, mpf)
    Nq, Nk = H * H, max(H // mpf, 1) ** 2
    row = [f'({B}, {Cc}, {H}, {mpf})']
    with torch.no_grad():
        f_mod = timed(lambda: m(x))
        f_at = timed(lambda: aten_self_attn(m, x)) if aten else None
        if aten:
            a, b = m(x), aten_self_attn(m, x)
            err = max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, b))
    fb_mod = timed(fwd_bwd(lambda t: m(t), m, x))
    fb_at = timed(fwd_bwd(lambda t: aten_self_attn(m, t), m, x)) if aten else None
    core = 2.0 * B * Nq * Nk * (Cc // 8 + Cc // 2)                # the two products of the attention core
    row += [f'{f_mod:.3f}', f'{f_at:.3f}' if aten else 'not run', f'{fb_mod:.3f}', f'{fb_at:.3f}' if aten else 'not run',
            f'{err:.1e}' if aten else '-', f'{core / 1e9:.1f}']
    print('| ' + ' | '.join(row) + ' |', flush=True)


def core_vs_specialised(B=32, H=38, D=64, C2=256):
    Nq = H * H
    Np = (Nq + 3) // 4 * 4
    torch.manual_seed(1)
    tp = torch.randn(B, Nq, 2 * D, device=dev) * D ** -0.25
    gT = torch.zeros(B, C2, Np, device=dev)
    gT[..., :Nq] = torch.randn(B, C2, Nq, device=dev)
    oa, ob = torch.empty(B, Nq, C2, device=dev), torch.empty(B, Nq, C2, device=dev)
    la, lb = torch.empty(B, Nq, device=dev), torch.empty(B, Nq, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    kp = tp[0, 0, D:].data_ptr()

    def any_():
        check(lib.gssd_self_attn_core_any_f32(tp.data_ptr(), kp, gT.data_ptr(), oa.data_ptr(), B, Nq, Nq, Np, D, C2, 2 * D, la.data_ptr(), s))

    def spec():
        check(lib.gssd_self_attn_core_kv_f32(tp.data_ptr(), kp, gT.data_ptr(), ob.data_ptr(), B, Nq, Nq, Np, D, C2, 2 * D, 0, lb.data_ptr(), s))
    ts = [(timed(any_, 20), timed(spec, 20)) for _ in range(3)]           # alternating, three rounds
    fl = 2.0 * B * Nq * Nq * (D + C2)
    ta, tb = min(t[0] for t in ts), min(t[1] for t in ts)
    print(f'\ncore at ({B}, {8 * D}, {H}): gssd_self_attn_core_any_f32 {ta * 1e3:.0f} us ({fl / ta / 1e9:.1f} TFLOP/s), '
          f'gssd_self_attn_core_kv_f32 (64, 256) {tb * 1e3:.0f} us ({fl / tb / 1e9:.1f} TFLOP/s); rounds (any, specialised) ms: '
          + ', '.join(f'({a:.3f}, {b:.3f})' for a, b in ts) + f'; outputs equal: {torch.equal(oa, ob) and torch.equal(la, lb)}', flush=True)


if __name__ == '__main__':
    print('| (B, C, H, max_pool_factor) | module fwd ms | ATen fwd ms | module fwd+bwd ms | ATen fwd+bwd ms | fwd max rel diff | core GFLOP (fwd) |')
    print('|---|---|---|---|---|---|---|')
    bench(32, 512, 38, 1)
    bench(8, 128, 64, 1)
    bench(8, 128, 64, 2)
    bench(2, 128, 150, 1, aten=False)
    core_vs_specialised()
