"""Inputs and references of the rows of tests/dcn_kernel_cases.py.

Inputs (make_inputs; NCHW on the host, the GPU module lays them out NHWC).
  family 'exact': x holds integers in [-4, 4], the weights integers in [-2, 2], the bias integers in [-8, 8], d(out) integers in [-1, 1]
    (d(cols) = W^T d(out), integers: what the dgrad of the contraction hands to the sampling backward), the offsets come from
    EXACT_OFFSETS -- quarters, so every bilinear weight is a multiple of 1/16 -- and, for one coordinate in three, from whatever puts the
    sample on -1, on H - 1, on H - 1/2 or on H of its own row; the mask logits are -200, 0 and 200, whose fp32 sigmoid 1 / (1 + expf(-l)) is
    exactly 0, 1/2 and 1.  Every product and every partial sum of the forward is then a multiple of 1/32 far below 2^24 (of 1/64 in the
    backward), so fp32 kernels, bf16 / fp16 operand planes, bf16 columns (a blended sample is a multiple of 1/32 below 4: eight bits) and
    atomic sums in any order are all exact: the reference's numbers must come back bit for bit.  tests/test_dcn_kernel_cases_cpu.py proves
    that on the CPU -- float32 = float64 = oracle/dcn_scalar -- so the property is the inputs', not a kernel's.
  family 'random': x ~ N(0, 1), weights ~ N(0, 0.05), bias ~ N(0, 1) (tests/test_gpu_kernels.py::test_dcn_x6_matches_fused), mask logits
    ~ N(0, 2), offsets on a 1/256 grid shifted by 1/512 (tests/test_gpu_dcn_op.py::case: fp32 and float64 take the same floor).

References (reference; cached per row id, read only).
  out     oracle.gssd_oracle.dcn_v2_conv in float64 (and oracle/dcn_scalar on the 'exact' rows)
  cols    sample() below: the sampling written the way the kernels write it (gate, y0 >= 0, y0 + 1 <= H - 1, clamped reads), which is the
          oracle's column matrix -- the CPU module checks it against the identity-weight construction of test_dcn_col2im_backward where
          that weight fits in memory -- and which can be restated with the two conventions a kernel could get wrong
  dx, doff, dlogit   float64 autograd through O.dcn_v2_conv(x, offset, torch.sigmoid(logit), w, bias) with d(out)
  e_cpu32 the same quantities in float32 on the CPU against float64, max|a - b| / max|b|: a quantity of the reference alone
"""
import zlib

import numpy as np
import torch

from oracle import gssd_oracle as O

import dcn_kernel_cases as R

GATE = 4             # the project's gate (tests/test_gpu_conv_leaves.py): e <= GATE * e_cpu32 + 1e-7
# entry family -> twice its worst e / e_cpu32 over three runs of tests/test_gpu_dcn_kernels.py on the MI355X (the figures: that module's
# docstring): 6.63 dcn_fused on 'wide groups', 3.06 x6 (bf16 planes) on 'wide groups', 1.23 im2col f32 on 'mixed', 1.26 d(x) of col2im on
# 'overflow only'.  None would mean: the family's ceiling stands alone (the bf16 entries, which are not listed: their error is the rounding
# of the output type, four orders above e_cpu32)
GATES = {'fused': 13.26, 'x6': 6.12, 'im2col': 2.46, 'col2im': 2.52}
BF_ULP = 2.0 ** -8
_cache = {}


def bound(e32, gate):
    return gate * e32 + 1e-7


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def l2rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def q16(t):
    return t.to(torch.bfloat16).to(torch.float32)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def _bases(kw):
    """[2, 9, H, W]: the undeformed sampling position (h - 1 + i, w - 1 + j) of tap k = 3 i + j at pixel (h, w)"""
    H, W = kw['H'], kw['W']
    k = torch.arange(9)
    by = torch.arange(H).view(1, H, 1) - 1 + (k // 3).view(9, 1, 1)
    bx = torch.arange(W).view(1, 1, W) - 1 + (k % 3).view(9, 1, 1)
    return torch.stack([by.expand(9, H, W), bx.expand(9, H, W)]).float()


def _pick(values, shape, g):
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _exact_offsets(kw, g):
    """[B, dg, 9, 2, H, W]"""
    B, dg, H, W = kw['B'], kw['dg'], kw['H'], kw['W']
    base = _bases(kw).permute(1, 0, 2, 3).view(1, 1, 9, 2, H, W)
    kind = kw.get('offsets')
    if kind == 'closed':
        return _pick(R.CLOSED_OFFSETS, (B, dg, 9, 2, H, W), g)
    if kind == 'one pixel':
        tgt = torch.tensor(kw['target'], dtype=torch.float32).view(1, 1, 1, 2, 1, 1)
        return (tgt - base).expand(B, dg, 9, 2, H, W).contiguous()
    off = _pick(R.EXACT_OFFSETS, (B, dg, 9, 2, H, W), g)
    ext = torch.tensor([float(H), float(W)]).view(1, 1, 1, 2, 1, 1)
    # one coordinate in three lands on a gate or in a border strip of its own row: -1, ext - 1 (the last pixel), ext - 1/2, ext
    land = _pick((0.0,) * 8 + (1.0, 2.0, 3.0, 4.0), off.shape, g)          # 1: on -1; 2, 3, 4: ext - 1, ext - 1/2, ext; 0: keep
    tgt = torch.where(land == 1, torch.full_like(off, -1.0), ext - 1 + (land - 2) * 0.5)
    return torch.where(land >= 1, tgt - base, off)


def _grid(t):
    return torch.round(t * 256) / 256 + 1.0 / 512


def _random_offsets(kw, g):
    B, dg, H, W = kw['B'], kw['dg'], kw['H'], kw['W']
    shape = (B, dg, 9, 2, H, W)
    kind = kw['offsets']
    if kind == 'normal':
        return _grid(torch.randn(shape, generator=g) * kw['std'])
    if kind == 'uniform':          # |offset| <= lim after the grid shift
        lim = kw['lim'] - 1.0 / 128
        return _grid((torch.rand(shape, generator=g) * 2 - 1) * lim)
    assert kind == 'far'
    # every sample inside the map, |offset| >= lim, the (y0, x0) cell outside the col2im window of the pixel's tile: drawn as targets, the
    # misses redrawn
    base = _bases(kw).permute(1, 0, 2, 3).view(1, 1, 9, 2, H, W).expand(shape)
    ext = torch.tensor([float(H), float(W)]).view(1, 1, 1, 2, 1, 1)
    off = torch.zeros(shape)
    bad = torch.ones(B, dg, 9, H, W, dtype=torch.bool)
    for _ in range(400):
        tgt = _grid(torch.rand(shape, generator=g) * (ext - 1.5) + 0.25)
        new = tgt - base
        off = torch.where(bad.unsqueeze(3), new, off)
        inwin, contrib = window_units(off, kw)
        bad = inwin | ~contrib | (off.abs() < kw['lim']).any(3)
        if not bool(bad.any()):
            return off
    raise AssertionError('overflow-only offsets did not converge')


def make_inputs(row):
    """x [B, C, H, W], om [B, 27 dg, H, W] (18 dg offsets in (group, tap, y | x) order, then 9 dg mask logits), w [Cout, C, 3, 3], bias [Cout]
    or None, dout [B, Cout, H, W], dcols [B, C, 9, H, W] = W^T d(out) rounded to fp32 (exact on the 'exact' rows)."""
    rid, family, kw, _ = row
    key = ('in', rid)
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(zlib.crc32(rid.encode()))
    B, H, W, C, dg, Cout = (kw[k] for k in ('B', 'H', 'W', 'C', 'dg', 'Cout'))
    if family == 'random':
        x = torch.randn(B, C, H, W, generator=g)
        w = torch.randn(Cout, C, 3, 3, generator=g) * 0.05
        bias = torch.randn(Cout, generator=g)
        dout = torch.randn(B, Cout, H, W, generator=g)
        off = _random_offsets(kw, g)
        logit = torch.randn(B, 9 * dg, H, W, generator=g) * 2.0
    else:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()          # noqa: E731
        x, w, bias, dout = ri(-4, 4, B, C, H, W), ri(-2, 2, Cout, C, 3, 3), ri(-8, 8, Cout), ri(-1, 1, B, Cout, H, W)
        off = _exact_offsets(kw, g)
        logit = _pick(R.EXACT_LOGITS, (B, 9 * dg, H, W), g)
    om = torch.cat([off.reshape(B, 18 * dg, H, W), logit], 1).contiguous()
    o = dict(x=x, om=om, w=w, bias=bias if kw['bias'] else None, dout=dout)
    if 'im2col second item' not in row[3]:          # (that row is compared with the entry itself, image by image)
        dcols64 = torch.einsum('ockl,bohw->bcklhw', w.double(), dout.double()).reshape(B, C, 9, H, W)
        o.update(dcols=dcols64.float(), dcols64=dcols64)
    _cache[key] = o
    return o


def split_om(om, dg):
    return om[:, :18 * dg], om[:, 18 * dg:]


# ---- the sampling, written the way the kernels write it --------------------------------------------------------------------------------------
def positions(off, kw):
    """py, px [B, dg, 9, H, W] in off's dtype"""
    B, dg, H, W = kw['B'], kw['dg'], kw['H'], kw['W']
    o = off.reshape(B, dg, 9, 2, H, W)
    base = _bases(kw).to(off.dtype)
    return base[0].view(1, 1, 9, H, W) + o[:, :, :, 0], base[1].view(1, 1, 9, H, W) + o[:, :, :, 1]


def cells(off, kw, upper_closed=False):
    """(contributes, y0, x0, py, px): the gate -1 < p < extent (upper_closed: p <= extent, the mistake) and the floor of each sample"""
    H, W = kw['H'], kw['W']
    py, px = positions(off, kw)
    if upper_closed:
        valid = (py > -1) & (px > -1) & (py <= H) & (px <= W)
    else:
        valid = (py > -1) & (px > -1) & (py < H) & (px < W)
    return valid, torch.floor(py), torch.floor(px), py, px


def sample(x, off, mask, kw, upper_closed=False, far_at_extent=False):
    """cols [B, C, 9, H, W] in x's dtype.  A corner counts when the sample is inside the gate and y0 >= 0 (near) / y0 + 1 <= H - 1 (far) -- the
    near corner needs no upper test BECAUSE the gate is open at H; reads are clamped into the map.  upper_closed: the gate restated as
    p <= extent; far_at_extent: the far corner restated as y0 + 1 <= H.  Either one reads the last row / column where the rule says zero."""
    B, dg, H, W, C = kw['B'], kw['dg'], kw['H'], kw['W'], kw['C']
    cpg = C // dg
    valid, y0, x0, py, px = cells(off, kw, upper_closed)
    ly, lx = py - y0, px - x0
    hy, hx = 1 - ly, 1 - lx
    fy, fx = (H, W) if far_at_extent else (H - 1, W - 1)
    y0ok, y1ok, x0ok, x1ok = valid & (y0 >= 0), valid & (y0 + 1 <= fy), x0 >= 0, x0 + 1 <= fx
    xg = x.reshape(B, dg, cpg, 1, H * W).expand(B, dg, cpg, 9, H * W)
    m = mask.reshape(B, dg, 1, 9, H * W)
    val = x.new_zeros(B, dg, cpg, 9, H * W)
    for yy, xx, ok, wgt in ((y0, x0, y0ok & x0ok, hy * hx), (y0, x0 + 1, y0ok & x1ok, hy * lx),
                            (y0 + 1, x0, y1ok & x0ok, ly * hx), (y0 + 1, x0 + 1, y1ok & x1ok, ly * lx)):
        lin = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().reshape(B, dg, 1, 9, H * W)
        wv = torch.where(ok, wgt, torch.zeros((), dtype=x.dtype)).reshape(B, dg, 1, 9, H * W)
        val = val + torch.gather(xg, 4, lin.expand(B, dg, cpg, 9, H * W)) * wv
    return (val * m).reshape(B, C, 9, H, W)


def contract(cols, w, bias):
    """out [B, Cout, H, W] = W cols + bias"""
    B, C, _, H, W = cols.shape
    out = torch.einsum('ok,bkp->bop', w.reshape(w.shape[0], C * 9).to(cols.dtype), cols.reshape(B, C * 9, H * W))
    if bias is not None:
        out = out + bias.to(cols.dtype).view(1, -1, 1)
    return out.reshape(B, -1, H, W)


def window_units(off, kw):
    """(in the LDS window, contributes) [B, dg, 9, H, W] bool: csrc/dcn.hip::dc_geometry with the constants of tests/dcn_kernel_cases.py -- a
    contributing unit stays in dcn_col2im_kernel when its (y0, x0) cell and the far corners lie inside the window of the pixel's tile"""
    H, W = kw['H'], kw['W']
    valid, y0, x0, _, _ = cells(off.reshape(kw['B'], -1, H, W), kw)
    _, _, _, WH, WW = R.col2im_grid(kw)
    wy0 = (torch.arange(H) // R.TH * R.TH - R.DC_R).view(1, 1, 1, H, 1)
    wx0 = (torch.arange(W) // R.TW * R.TW - R.DC_R).view(1, 1, 1, 1, W)
    wy, wx = y0 - wy0, x0 - wx0
    return valid & (wy >= 0) & (wx >= 0) & (wy + 1 < WH) & (wx + 1 < WW), valid


def window_share(row):
    """the share of contributing col2im units that stay in the window kernel"""
    kw = row[2]
    off, _ = split_om(make_inputs(row)['om'], kw['dg'])
    inwin, contrib = window_units(off, kw)
    return float(inwin.sum()) / max(int(contrib.sum()), 1)


def sample_counts(row):
    """counts over the 2 x 9 x dg x B H W sample coordinates of a row: on -1 (y, x), on the extent (y, x), in the strips (-1, 0) and
    (extent - 1, extent), on integers inside the map, far outside (beyond two pixels from the map)"""
    kw = row[2]
    off, _ = split_om(make_inputs(row)['om'], kw['dg'])
    py, px = positions(off, kw)
    out = {}
    for name, p, ext in (('y', py, kw['H']), ('x', px, kw['W'])):
        out['on -1 ' + name] = int((p == -1).sum())
        out['on extent ' + name] = int((p == ext).sum())
        out['low strip ' + name] = int(((p > -1) & (p < 0)).sum())
        out['high strip ' + name] = int(((p > ext - 1) & (p < ext)).sum())
        out['integers ' + name] = int(((p >= 0) & (p <= ext - 1) & (p == torch.floor(p))).sum())
        out['far ' + name] = int(((p < -3) | (p > ext + 2)).sum())
    return out


# ---- references -----------------------------------------------------------------------------------------------------------------------------------
def autograd(o, kw, dt):
    """(out, dx, doff, dlogit) through the oracle in dtype dt"""
    dg = kw['dg']
    off, logit = split_om(o['om'], dg)
    x = o['x'].to(dt).clone().requires_grad_()          # (clones: the cached inputs stay leaves without a gradient)
    off, logit = off.to(dt).clone().requires_grad_(), logit.to(dt).clone().requires_grad_()
    bias = o['bias'] if o['bias'] is not None else torch.zeros(kw['Cout'])
    out = O.dcn_v2_conv(x, off, torch.sigmoid(logit), o['w'].to(dt), bias.to(dt), 1, 1, 1, dg)
    out.backward(o['dout'].to(dt))
    return out.detach(), x.grad, off.grad, logit.grad


def cols_of(o, kw, dt, **conv):
    off, logit = split_om(o['om'], kw['dg'])
    return sample(o['x'].to(dt), off.to(dt), torch.sigmoid(logit.to(dt)), kw, **conv)


def reference(row):
    """dict: out, cols, dx, doff, dlogit (float64), the same in float32 on the CPU under '32', e_cpu32 per quantity under 'e32'"""
    rid, family, kw, _ = row
    key = ('ref', rid)
    if key not in _cache:
        o = make_inputs(row)
        names = ('out', 'dx', 'doff', 'dlogit')
        r64 = dict(zip(names, autograd(o, kw, torch.float64)), cols=cols_of(o, kw, torch.float64))
        r32 = dict(zip(names, autograd(o, kw, torch.float32)), cols=cols_of(o, kw, torch.float32))
        r64['dom'] = torch.cat([r64['doff'], r64['dlogit']], 1)
        r32['dom'] = torch.cat([r32['doff'], r32['dlogit']], 1)
        r64['32'] = r32
        r64['e32'] = {k: relerr(r32[k], r64[k]) for k in ('out', 'cols', 'dx', 'dom')}
        _cache[key] = r64
    return _cache[key]


def reference_bf16(row):
    """The bf16 entries' reference (tests/test_gpu_bf16.py::test_dcn_bf16): the oracle in float32 on bf16-rounded x and weights with its
    sampled columns rounded to bf16; (out, cols), cols from sample() on the rounded x, rounded once."""
    rid, _, kw, _ = row
    key = ('bf16', rid)
    if key not in _cache:
        o = make_inputs(row)
        off, logit = split_om(o['om'], kw['dg'])
        x, w = q16(o['x']), q16(o['w'])
        bias = o['bias'] if o['bias'] is not None else torch.zeros(kw['Cout'])
        out = O.dcn_v2_conv(x, off.contiguous(), torch.sigmoid(logit), w, bias, 1, 1, 1, kw['dg'], col_round=q16)
        _cache[key] = (out, q16(sample(x, off, torch.sigmoid(logit), kw)))
    return _cache[key]


def scalar_out(row):
    """oracle/dcn_scalar on the row (float32 in, float64 accumulation, float32 out)"""
    from oracle import dcn_scalar
    o, kw = make_inputs(row), row[2]
    off, logit = split_om(o['om'], kw['dg'])
    sig = (1.0 / (1.0 + np.exp(-logit.numpy().astype(np.float64)))).astype(np.float32)
    bias = o['bias'].numpy() if o['bias'] is not None else None
    return torch.from_numpy(dcn_scalar.dcn_v2_conv(o['x'].numpy(), off.contiguous().numpy(), sig, o['w'].numpy(), bias, 1, 1, 1, kw['dg']))
