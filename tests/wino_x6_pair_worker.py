"""Subprocess of tests/test_gpu_wino_x6_pair.py: the forward launch forms of csrc/conv_wino_x6.hip that the paired form takes (plain + bias,
batch sums into 1 and 8 replicas, the fused producer BatchNorm + ReLU with both padding paths) on the shapes below, under the switches the
parent put into the environment (both read once per process: GSSD_WINO_X6_PAIR, GSSD_WINO_X6 = 2 every shape the kernel can take / 0 the
fp32-MFMA kernel).  Per launch: a hash of the raw output bytes, the error against a float64 convolution (test_gpu_wino_x6.py's measure), and
for the batch sums their error against a float64 sum over the kernel's OWN output.  Prints one JSON line."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'grouped-ssd-pytorch_amd')):
    sys.path.insert(0, p)
import numpy as np                      # noqa: E402
import torch                            # noqa: E402
import torch.nn.functional as F         # noqa: E402

CASES = [
    # B, H, W, Cin, Cout, groups, GSSD_CONV_F16_OK          (3x3 / stride 1 / pad 1)
    (1, 5, 7, 128, 512, 4, True),       # one partial item, one chunk
    (2, 9, 9, 192, 512, 4, True),       # cin_g 48: the 16-channel tail half of the last chunk
    (2, 38, 38, 256, 512, 4, True),     # several items per workgroup, ragged last item
    (1, 11, 6, 128, 1024, 4, True),     # four 64-channel blocks per group: two pairs
    (1, 6, 6, 128, 768, 4, True),       # three blocks per group: stays unpaired
    (3, 7, 7, 64, 128, 1, True),        # dense
    (40, 4, 4, 128, 512, 4, True),      # three items: the grid is cut to the items
    (1, 5, 7, 128, 512, 4, False),      # bf16 planes: stays unpaired
    (2, 92, 92, 128, 512, 4, True),     # 67 items over the paired grid's 64 workgroups per pair (the unpaired grid's 32): two and three items
                                        # per workgroup -- the one case in which the batch sums are grouped differently
]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.abs().max()), 1e-30))


def sum_err(stats, y, Cout, R):
    """Each channel's sum / sum of squares against a float64 sum over y, relative to the float64 sum of the magnitudes (the scale a summation's
    rounding error is proportional to); the maximum over the channels."""
    s = stats.view(R, 2 * Cout).sum(0).cpu()
    y64 = y.cpu().double().reshape(-1, Cout)
    e1 = ((s[:Cout] - y64.sum(0)).abs() / y64.abs().sum(0).clamp_min(1e-300)).max()
    e2 = ((s[Cout:] - (y64 * y64).sum(0)).abs() / (y64 * y64).sum(0).clamp_min(1e-300)).max()
    return [float(e1), float(e2)]


def main():
    from gssd import ops, _lib
    lib = _lib.lib
    dev = torch.device('cuda:0')
    st = torch.cuda.current_stream().cuda_stream
    res = []
    for ci, (B, H, W, Cin, Cout, g, f16ok) in enumerate(CASES):
        rng = np.random.default_rng(4000 + ci)
        cin_g = Cin // g
        x = torch.from_numpy(rng.normal(0.1, 1.0, size=(B, Cin, H, W)).astype(np.float32))
        w = torch.from_numpy(rng.normal(0, 0.1, size=(Cout, cin_g, 3, 3)).astype(np.float32))
        b = torch.from_numpy(rng.normal(size=(Cout,)).astype(np.float32))
        out = dict(case=[B, H, W, Cin, Cout, g, f16ok], forms={})
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
        wp = ops.pack_weight(w.to(dev))
        U = ops.winograd_weight(wp, g, cin_g)
        kw = dict(B=B, H=H, W=W, in_stride=Cin, cin_g=cin_g, Cout=Cout, groups=g, k=3, stride=1, pad=1, bias=b.to(dev), wgt_wino=U,
                  flags=_lib.CONV_F16_OK if f16ok else 0)

        def launch(name, inp, ref64, R=0, **extra):
            y = torch.full((B, H, W, Cout), float('nan'), device=dev)
            stats = torch.zeros(R * 2 * Cout, dtype=torch.float64, device=dev) if R else None
            if R:
                extra.update(stats=stats, stats_rep=R)
            d, _, _ = ops.make_conv_desc(inp, wp, y, **{**kw, **extra})
            takes = int(lib.gssd_conv_wino_x6_takes(C.byref(d)))
            _lib.check(lib.gssd_conv2d_nhwc_f32(C.byref(d), st))
            torch.cuda.synchronize()
            assert torch.isfinite(y).all(), (name, out['case'])
            f = dict(takes=takes, err=rel(y.cpu(), ref64), sha=hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest())
            if R:
                f['sum_err'] = sum_err(stats, y, Cout, R)
            out['forms'][name] = f

        ref = F.conv2d(x.double(), w.double(), b.double(), 1, 1, 1, g).permute(0, 2, 3, 1).contiguous()
        launch('plain', xd, ref)
        launch('sums_rep1', xd, ref, R=1)
        launch('sums_rep8', xd, ref, R=8)
        # fused producer BatchNorm + ReLU: |scale| >= 0.2, both signs; padding = a value the transform maps to 0
        scv = torch.from_numpy(rng.uniform(0.2, 1.5, size=Cin).astype(np.float32)) * torch.from_numpy(rng.choice([-1.0, 1.0], size=Cin).astype(np.float32))
        shv = torch.from_numpy(rng.normal(size=Cin).astype(np.float32))
        pdv = torch.where(scv > 0, torch.full_like(scv, -3.0e38), torch.full_like(scv, 3.0e38))
        act64 = torch.relu(torch.addcmul(shv.double().view(1, -1, 1, 1), x.double(), scv.double().view(1, -1, 1, 1)))
        refx = F.conv2d(act64, w.double(), b.double(), 1, 1, 1, g).permute(0, 2, 3, 1).contiguous()
        sc, sh, pd_sep = scv.to(dev), shv.to(dev), pdv.to(dev)
        launch('xf_select', xd, refx, in_scale=sc, in_shift=sh, in_pad=pd_sep)
        launch('xf_select_sums', xd, refx, R=1, in_scale=sc, in_shift=sh, in_pad=pd_sep)
        n = B * H * W * Cin
        buf = torch.empty(n + Cin, device=dev)                        # the engine's layout: the padding vector directly behind the dense map
        buf[:n] = xd.reshape(-1)
        buf[n:] = pd_sep
        launch('xf_address', buf[:n].view(B, H, W, Cin), refx, in_scale=sc, in_shift=sh, in_pad=buf[n:])
        launch('xf_address_sums', buf[:n].view(B, H, W, Cin), refx, R=8, in_scale=sc, in_shift=sh, in_pad=buf[n:])
        res.append(out)
    print('WINOX6PAIRJSON ' + json.dumps(dict(mode=os.environ.get('GSSD_WINO_X6', ''), pair=os.environ.get('GSSD_WINO_X6_PAIR', ''), results=res)))


if __name__ == '__main__':
    main()
