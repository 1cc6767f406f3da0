"""GPU parity of the generic conv kernels, one launch per row of tests/conv_leaf_cases.py: every tile of csrc/conv_igemm.hip and
csrc/conv_bf16.hip (and csrc/gemm_slot.hip) and every epilogue / operand form of the generic kernel, each pinned to the template instance
it runs (gssd_conv2d_kernel_name on the real descriptor, asserted before the launch) and held against a float64 restatement of the same
operation: F.conv2d in double -- a double bmm for per-image weight matrices -- with the epilogue restated in double.

What a row checks
  - the output against float64.  fp32 gate: e = max|y - ref64| / max|ref64| <= GATE * e_cpu32 + 1e-7 and e < TOL, where e_cpu32 is the same
    figure for torch's CPU fp32 evaluation of the restatement (a reference-only quantity; 3 - 8e-7 at these shapes).  GATE = 4 covers the
    other accumulation order and the split-K atomics, 1e-7 is the slack of the x6 comparisons; GATE * e_cpu32 + 1e-7 itself has to stay
    under 2e-5, the Winograd gate a direct fp32 kernel must beat.  bf16 gate: test_conv_bf16's -- bf16-rounded operands, 1e-5 for fp32
    outputs, 1.01 bf16 ulp and "one ulp off the rounded oracle" for bf16 outputs.
  - the batch sums against the double sums: 2e-7 * pixels * max|ref| (squared for the second half), test_conv_x6_matches_float64's form.
  - every float of every output buffer the launch has no business with: buffers are allocated larger than written and pre-filled; the
    channels outside [out_ch_off, out_ch_off + Cout), the floats between images, a guard block behind the last row, the other priors of
    the heads' buffers must be untouched, the pad columns of transposed rows exactly what include/gssd_hip.h documents (zeros up to the
    launch's row tile for per-image launches, untouched for the flat GSSD_OUT_SPLIT_T).
  - operands: input channels outside the window, the floats between images and the weight rows' padding [K, wgt_row_stride) are NaN -- a
    tile tail that reads them shows in the output.

Worst e / e_cpu32 per instance, from the MI355X run of this module (every row prints its own figures; GATE = 4 was never widened):
  conv_igemm<128x128>  1.79   per image nhwc 128x128 (e 6.14e-07, e_cpu32 3.42e-07)
  conv_igemm<128x64>   1.80   per image nhwc 361 of 364 columns (e 6.26e-07, e_cpu32 3.49e-07)
  conv_igemm<128x32>   1.01   128x32 (e 6.23e-07, e_cpu32 6.16e-07)
  conv_igemm<128x16>   1.00   128x16 (e 7.36e-07, e_cpu32 7.36e-07)
  conv_igemm<64x64>    1.72   xf 64x64 (e 3.91e-07, e_cpu32 2.28e-07)
  conv_igemm<32x64>    2.60   32x64 M 1 (e 4.15e-07, e_cpu32 1.59e-07: one pixel, 72 values)
  gemm_slot<128x128>   1.10   gemm_slot (e 3.51e-07, e_cpu32 3.19e-07)
The split-K rows are CLOSER to float64 than the CPU (0.29 - 0.62: shorter fp32 chains per slice).  bf16 rows: fp32 outputs 0.8 - 3.0e-07
(gate 1e-5), bf16 outputs 0.54 - 0.83 ulp (gate 1.01).  Batch sums: at most 1.1e-08 of pixels * max|ref| (gate 2e-7).
"""
import ctypes
import os
import sys
import zlib

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import TOL, assert_kernel, dev          # noqa: E402,F401
import conv_leaf_cases as R              # noqa: E402

pytestmark = pytest.mark.gpu

GATE = 4
BF_ULP = 2.0 ** -8
SENT = -7.0          # pre-fill of every output buffer (exact in bf16)
GUARD = 256          # floats behind the last row
_ref_cache = {}      # row id -> the float64 / fp32 restatement (computed once, read only)


def _q(t):
    return t.to(torch.bfloat16).to(torch.float32)


class Buf:
    """One output buffer: its expected image in double, which floats the launch writes and which of those are documented zeros."""

    def __init__(self, n, dtype):
        self.dtype = dtype
        self.exp = torch.zeros(n + GUARD, dtype=torch.float64)
        self.exp32 = torch.zeros(n + GUARD, dtype=torch.float32)
        self.written = torch.zeros(n + GUARD, dtype=torch.bool)
        self.zeros = torch.zeros(n + GUARD, dtype=torch.bool)

    def put(self, size, stride, offset, v64, v32):
        torch.as_strided(self.exp, size, stride, offset).copy_(v64)
        if v32 is not None:
            torch.as_strided(self.exp32, size, stride, offset).copy_(v32)
        torch.as_strided(self.written, size, stride, offset).fill_(True)

    def put_zeros(self, size, stride, offset):
        torch.as_strided(self.zeros, size, stride, offset).fill_(True)

    def initial(self, accumulate):
        """what the caller hands the launch: the pre-fill, zeros where a split-K launch accumulates"""
        init = torch.full(self.exp.shape, SENT, dtype=self.dtype)
        if accumulate:
            init[self.written] = 0
        return init


def geometry(kw):
    k, stride, pad, dil = kw.get('k', 1), kw.get('stride', 1), kw.get('pad', 0), kw.get('dil', 1)
    Ho = (kw['H'] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (kw['W'] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return k, stride, pad, dil, Ho, Wo


def operands(row):
    """CPU masters of a row's operands (fp32; bf16 rows: bf16-rounded) inside NaN-filled buffers, seeded by the row id."""
    rid, bf16, kw, _, _ = row
    g = torch.Generator().manual_seed(zlib.crc32(rid.encode()))
    rnd = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc          # noqa: E731
    o = type('Operands', (), {})()
    B, H, W, groups, cin_g, Cout = kw['B'], kw['H'], kw['W'], kw.get('groups', 1), kw['cin_g'], kw['Cout']
    k = kw.get('k', 1)
    Cin, K, ins, ico = groups * cin_g, k * k * cin_g, kw['in_stride'], kw.get('in_ch_off', 0)
    ibs = kw.get('in_batch_stride') or H * W * ins
    o.xbuf = torch.full((B * ibs + 8,), float('nan'))
    o.x = torch.as_strided(o.xbuf, (B, H, W, Cin), (ibs, W * ins, ins, 1), ico)
    o.x.copy_(rnd(B, H, W, Cin) + 0.1)
    wrs, wbs = kw.get('wgt_row_stride', K), kw.get('wgt_batch_stride', 0)
    o.nW = B if wbs else 1
    o.wbuf = torch.full((o.nW * max(wbs, Cout * wrs) + 8,), float('nan'))
    o.w = torch.as_strided(o.wbuf, (o.nW, Cout, K), (max(wbs, Cout * wrs), wrs, 1), 0)          # K-major rows, k = tap * cin_g + c
    o.w.copy_(rnd(o.nW, Cout, K, sc=0.1))
    if bf16:
        o.x.copy_(_q(o.x))
        o.w.copy_(_q(o.w))
    o.bias = rnd(Cout) if 'bias' in kw else None
    o.alpha = torch.rand(Cout, generator=g) + 0.5 if 'alpha' in kw else None
    o.gate = torch.tensor([0.37]) if 'gate' in kw else None
    o.sc = o.sh = o.pad = None
    if 'in_scale' in kw:          # per input channel of the whole row (the kernel indexes them with in_ch_off), both signs
        o.sc = (torch.rand(ins, generator=g) * 1.3 + 0.2) * (torch.randint(0, 2, (ins,), generator=g) * 2 - 1).float()
        o.sh = rnd(ins)
        o.pad = torch.where(o.sc > 0, torch.full_like(o.sc, -3.0e38), torch.full_like(o.sc, 3.0e38))
    o.resid_seed = zlib.crc32(rid.encode()) + 1
    return o


def restate(row, o, dt):
    """The row's operation up to the pre-activation value acc * alpha + bias, in dtype dt on the CPU: [B][Ho * Wo][Cout]."""
    _, _, kw, _, _ = row
    B, groups, Cout = kw['B'], kw.get('groups', 1), kw['Cout']
    k, stride, pad, dil, Ho, Wo = geometry(kw)
    ico, Cin = kw.get('in_ch_off', 0), groups * kw['cin_g']
    x = o.x.to(dt)
    if o.sc is not None:
        x = torch.relu(x * o.sc[ico:ico + Cin].to(dt) + o.sh[ico:ico + Cin].to(dt))          # zero padding applies AFTER the transform
    if o.nW == 1:
        w_oihw = o.w[0].to(dt).reshape(Cout, k, k, kw['cin_g']).permute(0, 3, 1, 2)
        acc = F.conv2d(x.permute(0, 3, 1, 2), w_oihw, None, stride, pad, dil, groups).permute(0, 2, 3, 1).reshape(B, Ho * Wo, Cout)
    else:
        assert k == 1 and groups == 1
        acc = torch.bmm(x.reshape(B, Ho * Wo, Cin), o.w.to(dt).transpose(1, 2))
    v = acc * o.alpha.to(dt) if o.alpha is not None else acc
    v = v + o.bias.to(dt) if o.bias is not None else v
    return v


def expected(row, flags):
    """The expected image of every output buffer (Buf), the pre-activation output in double, and what the resid buffer holds."""
    rid, bf16, kw, want, _ = row
    key = (rid, flags)
    if key in _ref_cache:
        return _ref_cache[key]
    o = operands(row)
    B, Cout = kw['B'], kw['Cout']
    _, _, _, _, Ho, Wo = geometry(kw)
    HW = Ho * Wo
    mode, mpi = kw.get('out_mode', R.OUT_NHWC), kw.get('m_per_image', False)
    os_, oco, split_n = kw.get('out_stride', Cout), kw.get('out_ch_off', 0), kw.get('split_n', 0)
    obs = kw.get('out_batch_stride') if (mpi or mode == R.OUT_HEADS) else HW * os_
    out_dt = torch.float32 if (not bf16 or flags & R.F32OUT) else torch.bfloat16
    BM = R.tile_rows(want)
    pad_to = lambda row_len: min(row_len, -(-HW // BM) * BM)          # noqa: E731  (per-image launches zero the pad columns their tiles cover)
    pre64, pre32 = restate(row, o, torch.float64), (None if bf16 else restate(row, o, torch.float32))
    bufs = {}
    resid = None

    def epilogue(pre, dt, layout):
        t, out2 = pre, None
        if o.gate is not None:
            t = t * o.gate.to(dt)
            out2 = t
        if 'resid' in kw:
            t = t + torch.as_strided(resid, *layout).to(dt)
        if kw.get('relu'):
            t = torch.relu(t)
        return t, out2

    if mode == R.OUT_NHWC:
        layout = ((B, HW, Cout), (obs, os_, 1), oco)
        n = (B - 1) * obs + HW * os_
        if 'resid' in kw:          # same geometry as out: every float of it is data, only the window is read
            resid = torch.randn(n + GUARD, generator=torch.Generator().manual_seed(o.resid_seed))
        (t64, o2_64), (t32, o2_32) = epilogue(pre64, torch.float64, layout), (epilogue(pre32, torch.float32, layout) if pre32 is not None else (None, None))
        bufs['out'] = Buf(n, out_dt)
        bufs['out'].put(*layout, t64, t32)
        if 'out2' in kw:
            bufs['out2'] = Buf(n, out_dt)
            bufs['out2'].put(*layout, o2_64, o2_32)
    elif mode == R.OUT_TRANSPOSED:
        t64 = torch.relu(pre64) if kw.get('relu') else pre64
        t32 = None if pre32 is None else (torch.relu(pre32) if kw.get('relu') else pre32)
        bufs['out'] = Buf((B - 1) * obs + Cout * os_, out_dt)
        bufs['out'].put((B, Cout, HW), (obs, os_, 1), 0, t64.transpose(1, 2), None if t32 is None else t32.transpose(1, 2))
        bufs['out'].put_zeros((B, Cout, pad_to(os_) - HW), (obs, os_, 1), HW)
    elif mode == R.OUT_HEADS:
        nb, obbs = Cout - split_n, kw['outb_batch_stride']
        bufs['out'] = Buf(B * obs, out_dt)
        bufs['out'].put((B, HW, split_n), (obs, split_n, 1), kw['out_off'], pre64[..., :split_n], None if pre32 is None else pre32[..., :split_n])
        bufs['out_b'] = Buf(B * obbs, out_dt)
        bufs['out_b'].put((B, HW, nb), (obbs, nb, 1), kw['outb_off'], pre64[..., split_n:], None if pre32 is None else pre32[..., split_n:])
    else:                          # GSSD_OUT_SPLIT_T
        nb, obst, obbs = Cout - split_n, kw['out_b_stride'], kw['outb_batch_stride']
        bufs['out'] = Buf((B - 1) * obs + HW * os_, out_dt)
        bufs['out'].put((B, HW, split_n), (obs, os_, 1), oco, pre64[..., :split_n], None if pre32 is None else pre32[..., :split_n])
        bufs['out_b'] = Buf((B - 1) * obbs + nb * obst, out_dt)
        bufs['out_b'].put((B, nb, HW), (obbs, obst, 1), 0, pre64[..., split_n:].transpose(1, 2), None if pre32 is None else pre32[..., split_n:].transpose(1, 2))
        if mpi:                    # flat launches leave the pad columns alone
            bufs['out_b'].put_zeros((B, nb, pad_to(obst) - HW), (obbs, obst, 1), HW)
    _ref_cache[key] = (o, bufs, pre64, resid)
    return _ref_cache[key]


def variants(row):
    """bf16 NHWC rows run with a bf16 and with an fp32 output"""
    _, bf16, kw, _, _ = row
    flags = kw.get('flags', 0)
    return [flags, flags | R.F32OUT] if bf16 and kw.get('out_mode', 0) == R.OUT_NHWC and not flags & R.F32OUT else [flags]


@pytest.mark.parametrize('row', R.ROWS, ids=R.row_id)
def test_conv_leaf_matches_float64(dev, row):
    from gssd import _lib, ops
    rid, bf16, kw, want, _ = row
    _, _, _, _, Ho, Wo = geometry(kw)
    Cout = kw['Cout']
    for flags in variants(row):
        o, bufs, pre64, resid = expected(row, flags)
        in_dt = torch.bfloat16 if bf16 else torch.float32
        devt = {'in': o.xbuf.to(in_dt).to(dev), 'wgt': o.wbuf.to(in_dt).to(dev)}
        for name, b in bufs.items():
            devt[name] = b.initial(kw.get('split_k', 1) > 1).to(dev)
        for name in ('bias', 'alpha', 'gate'):
            if getattr(o, name) is not None:
                devt[name] = getattr(o, name).to(dev)
        if o.sc is not None:
            devt.update(in_scale=o.sc.to(dev), in_shift=o.sh.to(dev), in_pad=o.pad.to(in_dt).to(dev))
        if resid is not None:
            devt['resid'] = resid.to(in_dt).to(dev)
        if 'stats' in kw:
            devt['stats'] = torch.cat([torch.zeros(2 * Cout, dtype=torch.float64), torch.full((8,), SENT, dtype=torch.float64)]).to(dev)
        d, _, _ = ops.make_conv_desc(devt['in'], devt['wgt'], devt['out'], **{**R.resolve(kw, lambda key: devt[key]), 'flags': flags})
        assert_kernel(d, want, bf16)
        fn = _lib.lib.gssd_conv2d_nhwc_bf16 if bf16 else _lib.lib.gssd_conv2d_nhwc_f32
        _lib.check(fn(ctypes.byref(d), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for name, b in bufs.items():
            got = devt[name].cpu()
            untouched = ~(b.written | b.zeros)
            assert torch.equal(got[untouched], torch.full_like(got[untouched], SENT)), f'{rid}: {name} written outside its window'
            assert int(b.zeros.sum()) == 0 or float(got[b.zeros].abs().max()) == 0.0, f'{rid}: {name} pad columns are not zero'
            y, ref = got[b.written].double(), b.exp[b.written]
            scale = float(ref.abs().max())
            e = float((y - ref).abs().max()) / scale
            if not bf16:
                e32 = float((b.exp32[b.written].double() - ref).abs().max()) / scale
                print(f'LEAF {want} | {rid} | {name}: e {e:.2e} e_cpu32 {e32:.2e} ratio {e / max(e32, 1e-30):.2f}')
                assert GATE * e32 + 1e-7 < 2e-5, (rid, name, e32)
                assert e <= GATE * e32 + 1e-7 and e < TOL, (rid, name, e, e32)
            elif b.dtype == torch.float32:
                print(f'LEAF {want} | {rid} | {name}: fp32 output e {e:.2e}')
                assert e < 1e-5, (rid, name, e)
            else:
                print(f'LEAF {want} | {rid} | {name}: bf16 output e {e:.2e} = {e / BF_ULP:.2f} ulp')
                assert e < 1.01 * BF_ULP, (rid, name, e)
                assert float((y - _q(ref.float()).double()).abs().max()) <= scale * BF_ULP, (rid, name)       # at most one ulp off the rounded oracle
        if 'stats' in kw:
            st = devt['stats'].cpu()
            assert torch.equal(st[2 * Cout:], torch.full((8,), SENT, dtype=torch.float64)), f'{rid}: batch sums written past 2 * Cout'
            s1, s2 = pre64.sum((0, 1)), (pre64 * pre64).sum((0, 1))
            n_px, scale = kw['B'] * Ho * Wo, float(pre64.abs().max())
            if bf16:          # test_conv_bf16's form
                assert float((st[:Cout] - s1).abs().max() / s1.abs().max()) < 1e-5 and float((st[Cout:2 * Cout] - s2).abs().max() / s2.abs().max()) < 1e-5, rid
            else:
                e1, e2 = float((st[:Cout] - s1).abs().max()) / (n_px * scale), float((st[Cout:2 * Cout] - s2).abs().max()) / (n_px * scale ** 2)
                print(f'LEAF {want} | {rid} | batch sums: {e1:.1e} {e2:.1e} of pixels * max|ref|')
                assert e1 < 2e-7 and e2 < 2e-7, (rid, e1, e2)
