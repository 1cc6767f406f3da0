"""GPU parity of csrc/pixellink.hip at its edges, one test per row of tests/pixellink_tail_cases.py: PixelLinkLoss forward / backward through the
C entries and pixel_link.criterion.PixelLinkLoss, the link decoding through gssd_pixellink_decode_f32 and pixel_link.postprocess.decode, the
upsample-add cascade and the final 1x1 convs with their gradients through the C entries.

What a row checks
  - loss rows: the mined mask, area and neg_area EXACTLY (the rows leave no decision to rounding: tests/test_pixellink_tail_cases_cpu.py),
    also through PixelLinkLoss.neg_pixel_weight / .area / .neg_area; the four losses per image and as batch means at the project's 1e-5
    (max |got - ref| / max |ref| over the four, as test_loss_vs_reference_fixture) against the float64 restatement and, where the reference
    defines the row, the fixture; the gradients against float64 autograd with the mask constant, 1e-5 as a ceiling (worst figure printed).
    NaN exactly where area + neg_area == 0, and finite zeros in that image's d(out1).
  - decode rows: labels, ncomp, count and bounding box exactly, for every max_comp of the row; the score sum within count * 2^-24 * sum|score|
    of the float64 sum; rows beyond the table or beyond ncomp hold the empty pattern; on fixture rows also against postprocess.func's maps.
  - interp_add: forward against float64 F.interpolate at the project's 5e-6, same-size rows bit-equal; backward against float64 with the
    measured gate; d(addend) bit-equal to the one fp32 add it is; pad channels bit-identical.
  - final / final5: forward, d(features) and the weight gradients against float64 with the measured gates, every accumulate_mask x ld.
  - guards: every output lies in a larger buffer between sentinels that must come back bit-identical; every input has a guard behind its last
    element (NaN; for integer inputs a value that would change an exact result); an output the kernel must define completely starts as NaN
    (integers: -7777), one it accumulates into at the row's non-zero pre-fill.

Gates e <= GATE * e_cpu32 + 1e-7 (e = max |got - ref64| / max |ref64|, e_cpu32 = the same figure of the float32 restatement on the CPU;
pixellink_tail_cases.GATES).  Worst e / e_cpu32 per entry family over three MI355X runs of this module (every row prints its own figures):
  interp_bwd   3.73 / 3.82 / 3.73   19x10->38x19 C1, ld 3 'both' (e 3.41e-07, e_cpu32 8.92e-08; 3.73 with d_out2 NULL in every run).  The fp32
               atomics add up to eight contributions onto the pre-fill in whatever order they arrive, the float32 einsum of the restatement sums
               them first: the ratio is high where e_cpu32 is at its floor.  Every e of the family is below 3.5e-07.
  final_fwd    1.00 on every row, every run     final_dfeat  1.00     final_wgrad  1.00
               pixellink_tail_cases.final32 walks the kernels' own order (fma chains; 128-pixel passes summed in float64), and the device
               results equal it to the printed digits: e = e_cpu32 on all 54 rows x masks x ld (largest e: 6.3e-07, a weight gradient).
               The order of the fp64 atomics did not show in any figure.
The gates that stand: 7.64 for interp_bwd, 2.0 for the three final families = twice the worst measured ratio.  GATE * e_cpu32 + 1e-7 stays below
1.5e-06 (interp_bwd, against the 2e-6 of test_interp_add_backward), 8.0e-07 / 5.9e-07 (final forward / d(features), against the 1e-6 of
test_final5_kernels) and 1.4e-06 (weight gradients, against its 1e-5) on every row: asserted in the CPU module.
Other worst figures of one run: losses 4.5e-08 ('ties_straddle 5x7'), d(out1) 2.0e-07 ('no_positives 100x101'), d(out2) 1.9e-07
('ties_straddle 91x91') against the 1e-5 ceiling; score sums 0.68 of their bound ('table 1024': one-pixel components, where the bound is one
rounding wide -- which is why the varied score levels are chosen by pixellink_tail_cases.score_level_ratio); interp_add forward below 5e-6 on
every row.
What failed: nothing in csrc/pixellink.hip, pixel_link/criterion.py or pixel_link/postprocess.py -- every row passed on its first run on the
device, so no product code changed.  The behaviour the rows pin that nothing stated before: ncand == 0 mines nothing and divides by the area
alone; area + neg_area == 0 gives NaN pixel terms and finite zero gradients; both decode thresholds are strict (include/gssd_hip.h now says so).
The module takes 3.9 s on an MI355X (186 tests; the slowest, the first loss row with the library load, 0.5 s).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import dev          # noqa: E402,F401
import pixellink_tail_cases as K    # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -7.0
GUARD = 256
NAN = float('nan')
UNSET = -7777
U = 2.0 ** -24


def st():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """An output inside a larger device buffer: [SENT guard | values (prefilled) | SENT guard]"""

    def __init__(self, shape, dev, dtype=torch.float32, fill=NAN):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.n = int(np.prod(shape))
        self.host = torch.full((self.n + 2 * GUARD,), SENT, dtype=dtype)
        if torch.is_tensor(fill) or isinstance(fill, np.ndarray):
            self.host[GUARD:GUARD + self.n] = torch.as_tensor(fill).reshape(-1).to(dtype)
        else:
            self.host[GUARD:GUARD + self.n] = fill if dtype.is_floating_point else UNSET
        self.buf = self.host.to(dev)
        self.v = self.buf[GUARD:GUARD + self.n].view(shape)

    def ptr(self):
        return self.v.data_ptr()

    def check(self, what):
        got = self.buf.cpu()
        assert torch.equal(got[:GUARD], self.host[:GUARD]), f'{what}: written in front of the output'
        assert torch.equal(got[GUARD + self.n:], self.host[GUARD + self.n:]), f'{what}: written behind the output'
        return got[GUARD:GUARD + self.n].view(self.v.shape).numpy()

    def untouched(self, what):
        got = self.buf.cpu()
        same = (got == self.host) | ((got != got) & (self.host != self.host))
        assert bool(same.all()), f'{what}: values changed'


def inp(a, dev):
    """an input on the device with a guard behind its last element: NaN, or for integers a value that would change an exact result"""
    t = torch.as_tensor(a)
    g = NAN if t.dtype.is_floating_point else (255 if t.dtype == torch.uint8 else 1 << 40)
    buf = torch.cat([t.reshape(-1), torch.full((GUARD,), g, dtype=t.dtype)]).to(dev)
    return buf[:t.numel()].view(t.shape)


def rel4(got, ref):
    """max |got - ref| / max |ref| over the four losses, NaN positions equal"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    return K.relerr(np.nan_to_num(got), np.nan_to_num(ref))


# ------------------------------------------------------------------------------------------------------------------------------------------
# PixelLinkLoss
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(K.LOSS)), ids=[r.name for r in K.LOSS])
def test_loss_row(dev, golden, i):
    from gssd import _lib
    from pixel_link.criterion import PixelLinkLoss
    lib = _lib.lib
    row, ref = K.LOSS[i], K.loss_reference(i)
    src = ref['inp']
    B, H, W = row.B, row.H, row.W
    o1, o2, pix, neg, posw, link = (inp(src[k], dev) for k in ('out1', 'out2', 'pix', 'neg', 'posw', 'link'))
    res, nw = Out((B, 6), dev, torch.float64), Out((B, H, W), dev)
    _lib.check(lib.gssd_pixellink_loss_f32(o1.data_ptr(), o2.data_ptr(), pix.data_ptr(), neg.data_ptr(), posw.data_ptr(), link.data_ptr(),
                                           res.ptr(), nw.ptr(), B, H, W, row.ratio, st()))
    torch.cuda.synchronize()
    r, m = res.check('per_image'), nw.check('neg_weight_out')
    assert np.array_equal(r[:, 4], ref['area']) and np.array_equal(r[:, 5], ref['neg_area']), (r[:, 4:], ref['area'], ref['neg_area'])
    assert set(np.unique(m)) <= {0.0, 1.0}
    wrong = (m == 1) != ref['mask']
    assert not wrong.any(), f'{row.name}: {int(wrong.sum())} pixels of the mined mask differ ({m.reshape(B, -1).sum(1)} mined, {ref["mask"].reshape(B, -1).sum(1)} expected)'
    e_img = max(rel4(r[b, :4], ref['per_image'][b]) for b in range(B))
    with np.errstate(invalid='ignore'):
        e_mean = rel4(r[:, :4].mean(0), ref['per_image'].mean(0))
    # backward: the C entry on the forward's own outputs
    up = inp(np.asarray(K.UPSTREAM, np.float32), dev)
    d1, d2 = Out((B, 2, H, W), dev), Out((B, 16, H, W), dev)
    _lib.check(lib.gssd_pixellink_loss_bwd_f32(o1.data_ptr(), o2.data_ptr(), pix.data_ptr(), nw.ptr(), posw.data_ptr(), link.data_ptr(), res.ptr(),
                                               up.data_ptr(), d1.ptr(), d2.ptr(), B, H, W, st()))
    torch.cuda.synchronize()
    g1, g2 = d1.check('d_out1'), d2.check('d_out2')
    assert np.array_equal(res.check('per_image'), r, equal_nan=True) and np.array_equal(nw.check('neg_weight'), m), f'{row.name}: the backward wrote to its inputs'
    assert np.isfinite(g1).all() and np.isfinite(g2).all(), f'{row.name}: {int((~np.isfinite(g1)).sum())} + {int((~np.isfinite(g2)).sum())} non-finite gradients'
    e_g1, e_g2 = K.relerr(g1, ref['d1']), K.relerr(g2, ref['d2'])
    print(f'LOSS {row.name}: losses per image {e_img:.2e} batch {e_mean:.2e}  d_out1 {e_g1:.2e}  d_out2 {e_g2:.2e}')
    assert e_img < 1e-5 and e_mean < 1e-5
    assert e_g1 <= 1e-5 and e_g2 <= 1e-5
    for b, c in enumerate(row.contents):
        if c == 'nothing_at_all':
            assert np.isnan(r[b, :2]).all() and float(np.abs(g1[b]).max()) == 0.0
        if c == 'posw_zero':
            assert float(np.abs(g2[b]).max()) == 0.0
        if c == 'links_all_1':
            assert r[b, 3] == 0.0
        if c == 'links_all_0':
            assert r[b, 2] == 0.0
    for k, t in (('out1', o1), ('out2', o2), ('pix', pix), ('neg', neg), ('posw', posw), ('link', link)):
        assert np.array_equal(t.cpu().numpy(), src[k]), f'{row.name}: input {k} changed'
    g = golden('pixellink_tail')
    if f'loss|{row.name}|vals' in g.files:
        assert K.reference_defines_loss(i)
        assert np.array_equal(g[f'loss|{row.name}|neg_area'], r[:, 5]) and np.array_equal(np.unpackbits(g[f'loss|{row.name}|mask'])[:m.size], m.ravel())
        assert rel4(r[:, :4].mean(0), g[f'loss|{row.name}|vals']) < 1e-5
    else:
        assert not K.reference_defines_loss(i)
    if row.through_criterion:
        crit = PixelLinkLoss()
        h1, h2 = o1.clone().requires_grad_(), o2.clone().requires_grad_()
        pp, pn = crit.pixel_loss(h1, pix, neg, posw, link=(h2, link))
        lp, ln = crit.link_loss(h2, link)
        assert crit.neg_pixel_weight.dtype == torch.uint8 and np.array_equal(crit.neg_pixel_weight.cpu().numpy().astype(bool), ref['mask'])
        assert np.array_equal(crit.area.cpu().numpy(), ref['area']) and np.array_equal(crit.neg_area.cpu().numpy(), ref['neg_area'])
        assert rel4([float(pp), float(pn), float(lp), float(ln)], ref['per_image'].mean(0)) < 1e-5
        sum(w * t for w, t in zip(K.UPSTREAM, (pp, pn, lp, ln))).backward()
        assert K.relerr(h1.grad.cpu().numpy(), ref['d1']) <= 1e-5 and K.relerr(h2.grad.cpu().numpy(), ref['d2']) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------------------------------
# link decoding
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', K.DECODE, ids=[r.name for r in K.DECODE])
def test_decode_row(dev, golden, row):
    from gssd import _lib
    from pixel_link import postprocess
    lib = _lib.lib
    d = row.build()
    B, _, H, W = d['out1'].shape
    pthr, lthr = row.thresholds
    o1, o2 = inp(d['out1'], dev), inp(d['out2'], dev)
    if row.error:                                                     # the argument error, nothing launched or written
        lab, comps, ncomp = Out((B, 8), dev, torch.int32), Out((B, 4, 6), dev), Out((B,), dev, torch.int32)
        with pytest.raises(_lib.GssdError):
            _lib.check(lib.gssd_pixellink_decode_f32(o1.data_ptr(), o2.data_ptr(), lab.ptr(), comps.ptr(), ncomp.ptr(), B, H, W, pthr, lthr, 4, st()))
        torch.cuda.synchronize()
        for o, what in ((lab, 'labels'), (comps, 'comps'), (ncomp, 'ncomp')):
            o.untouched(what)
        with pytest.raises(_lib.GssdError):
            postprocess.decode(o1, o2)
        return
    stats = [K.component_stats(d['labels'][b], d['out1'][b]) for b in range(B)]
    worst = 0.0
    for mc in row.max_comps:
        lab, comps, ncomp = Out((B, H, W), dev, torch.int32), Out((B, mc, 6), dev), Out((B,), dev, torch.int32)
        _lib.check(lib.gssd_pixellink_decode_f32(o1.data_ptr(), o2.data_ptr(), lab.ptr(), comps.ptr(), ncomp.ptr(), B, H, W, pthr, lthr, mc, st()))
        torch.cuda.synchronize()
        L, C, N = lab.check('labels'), comps.check('comps'), ncomp.check('ncomp')
        for b in range(B):
            bad = L[b] != d['labels'][b]
            assert not bad.any(), f'{row.name} max_comp {mc} image {b}: {int(bad.sum())} labels differ, first at {tuple(np.argwhere(bad)[0])}; {int(L[b].max())} components, {int(d["labels"][b].max())} expected'
            box, ssum = stats[b]
            n = len(box)
            assert int(N[b]) == n
            have = min(n, mc, K.PL_STAT_COMPS)
            assert np.array_equal(C[b, :have, :5], box[:have].astype(np.float32)), f'{row.name} max_comp {mc} image {b}: count / bounding box'
            assert np.array_equal(C[b, have:], np.tile(np.asarray(K.EMPTY_COMP, np.float32), (mc - have, 1))), f'{row.name} max_comp {mc} image {b}: rows beyond'
            if have:
                ratio = np.abs(C[b, :have, 5].astype(np.float64) - ssum[:have]) / (box[:have, 0] * U * ssum[:have])
                worst = max(worst, float(ratio.max()))
    print(f'DECODE {row.name}: worst |score sum - float64| / (count 2^-24 sum|score|) {worst:.3f}')
    assert worst <= 1.0
    assert np.array_equal(o1.cpu().numpy(), d['out1']) and np.array_equal(o2.cpu().numpy(), d['out2'])
    g = golden('pixellink_tail')
    if f'decode|{row.name}|labels' in g.files:
        assert np.array_equal(g[f'decode|{row.name}|labels'].astype(np.int32), L)
    else:
        assert int(d['labels'].max()) > 255
    # the wrapper: the same maps; above the statistics table the box path refuses
    lw, cw, nw = postprocess.decode(o1, o2, pixel_thres=row.thr[0], link_thres=row.thr[1])
    assert np.array_equal(lw.cpu().numpy(), d['labels']) and np.array_equal(nw.cpu().numpy(), [len(s[0]) for s in stats]) and tuple(cw.shape) == (B, 512, 6)
    if row.name.startswith('table'):
        if int(d['labels'].max()) > K.PL_STAT_COMPS:
            with pytest.raises(_lib.GssdError):
                postprocess.mask_to_box_device(o1, o2)
        else:
            det, ndet = postprocess.mask_to_box_device(o1, o2)
            assert int(ndet[0]) <= int(d['labels'].max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# the cascade
# ------------------------------------------------------------------------------------------------------------------------------------------
def _torch_interp64(src, Hd, Wd):
    import torch.nn.functional as F
    return F.interpolate(torch.from_numpy(src).double().permute(0, 3, 1, 2), size=(Hd, Wd), mode='bilinear', align_corners=True).permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize('r', K.INTERP, ids=K.interp_id)
def test_interp_add_forward(dev, r):
    from gssd import _lib
    lib = _lib.lib
    (Hs, Ws, Hd, Wd), C = r
    B = K.INTERP_B
    src = K.interp_inputs(r)
    want = _torch_interp64(src['src'], Hd, Wd)
    s, a = inp(src['src'], dev), inp(src['addend'], dev)
    for with_add in (False, True):
        out, out2 = Out((B, Hd, Wd, C), dev), Out((B, Hd, Wd, C), dev)
        _lib.check(lib.gssd_interp_add_f32(s.data_ptr(), a.data_ptr() if with_add else None, out.ptr(), out2.ptr() if with_add else None, B, Hs, Ws,
                                           Hd, Wd, C, st()))
        torch.cuda.synchronize()
        o = out.check('out')
        e = K.relerr(o, want)
        assert e < 5e-6, (K.interp_id(r), e)
        if with_add:
            e2 = K.relerr(out2.check('out2'), want + src['addend'])
            assert e2 < 5e-6, (K.interp_id(r), e2)
            assert np.array_equal(out2.check('out2'), o + src['addend'])          # one fp32 add
        else:
            out2.untouched('out2 (no addend)')
        if (Hs, Ws) == (Hd, Wd):
            assert np.array_equal(o, src['src'])
    assert np.array_equal(s.cpu().numpy(), src['src']) and np.array_equal(a.cpu().numpy(), src['addend'])


@pytest.mark.parametrize('r', K.INTERP, ids=K.interp_id)
def test_interp_add_backward(dev, r):
    from gssd import _lib
    lib = _lib.lib
    (Hs, Ws, Hd, Wd), C = r
    B = K.INTERP_B
    src = K.interp_inputs(r)
    need = 0.0
    for ld in (C, C + 2):
        def pad(a, fill):                                             # NHWC with channel stride ld; the pad channels hold `fill`
            out = np.full(a.shape[:-1] + (ld,), fill, np.float32)
            out[..., :C] = a
            return out
        for form in K.INTERP_BWD_FORMS:
            use1, use2 = form != 'dout_null', form != 'dout2_null'
            go, go2 = inp(pad(src['dout'], NAN), dev), inp(pad(src['dout2'], NAN), dev)        # a pad channel that is read poisons the result
            dsrc, dadd = Out((B, Hs, Ws, ld), dev, fill=pad(src['dsrc0'], 3.5)), Out((B, Hd, Wd, ld), dev, fill=pad(src['dadd0'], -2.5))
            _lib.check(lib.gssd_interp_add_bwd_f32(go.data_ptr() if use1 else None, go2.data_ptr() if use2 else None, dsrc.ptr(), dadd.ptr(), B, Hs, Ws,
                                                   Hd, Wd, C, ld, st()))
            torch.cuda.synchronize()
            gs, ga = dsrc.check('d_src'), dadd.check('d_addend')
            what = f'{K.interp_id(r)} ld {ld} {form}'
            assert bool((gs[..., C:] == 3.5).all()) and bool((ga[..., C:] == -2.5).all()), f'{what}: pad channels written'
            g = (src['dout'].astype(np.float64) if use1 else 0.0) + (src['dout2'].astype(np.float64) if use2 else 0.0)
            g32 = ((src['dout'] if use1 else np.float32(0)) + (src['dout2'] if use2 else np.float32(0))).astype(np.float32)
            want = src['dsrc0'] + K.interp_bwd64(g, Hs, Ws)
            e32 = K.relerr(src['dsrc0'] + K.interp_bwd64(g32, Hs, Ws, dtype=np.float32), want)
            e = K.relerr(gs[..., :C], want)
            need = max(need, e / e32 if e32 > 0 else 0.0)
            print(f'INTERP_BWD {what}: e {e:.2e} e_cpu32 {e32:.2e} ratio {e / max(e32, 1e-30):.2f}')
            assert e <= K.bound('interp_bwd', e32), (what, e, e32)
            assert np.array_equal(ga[..., :C], src['dadd0'] + src['dout2'] if use2 else src['dadd0']), f'{what}: d_addend'
    print(f'GATE interp_bwd {K.interp_id(r)}: worst e / e_cpu32 {need:.2f}')


# ------------------------------------------------------------------------------------------------------------------------------------------
# final_1 / final_2
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', K.FINAL, ids=K.final_id)
def test_final_row(dev, r):
    from gssd import _lib
    lib = _lib.lib
    fam, nf, B, HW = r
    top = 4 if fam == 'final' else 5
    fwd, bwd = (lib.gssd_pixellink_final_f32, lib.gssd_pixellink_final_bwd_f32) if fam == 'final' else (lib.gssd_pixellink_final5_f32, lib.gssd_pixellink_final5_bwd_f32)
    src = K.final_inputs(r)
    feats = [inp(f, dev) for f in src['feats']]
    fp = [f.data_ptr() for f in feats] + [None] * (top - nf)
    w1, b1, w2, b2, d1, d2 = (inp(src[k], dev) for k in ('w1', 'b1', 'w2', 'b2', 'd1', 'd2'))
    need = dict(final_fwd=0.0, final_dfeat=0.0, final_wgrad=0.0)
    fails = []

    def gate(family, what, got, want, want32):
        e, e32 = K.relerr(got, want), K.relerr(want32, want)
        need[family] = max(need[family], e / e32 if e32 > 0 else 0.0)
        if not e <= K.bound(family, e32):
            fails.append((what, e, e32))
    o1, o2 = Out((B, 2, HW), dev), Out((B, 16, HW), dev)
    _lib.check(fwd(*fp, nf, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), o1.ptr(), o2.ptr(), B, HW, st()))
    torch.cuda.synchronize()
    r64, r32 = K.final64(src, 0), K.final32(src, 0)
    gate('final_fwd', 'out1', o1.check('out1'), r64['out1'], r32['out1'])
    gate('final_fwd', 'out2', o2.check('out2'), r64['out2'], r32['out2'])
    for ld in K.FINAL_LD:
        for mask in K.final_masks(nf):
            r64, r32 = K.final64(src, mask), K.final32(src, mask)
            gs = []
            for k in range(nf):                                       # a map the kernel defines starts as NaN, one it adds to at the pre-fill
                fill = np.full((B, HW, ld), 3.5, np.float32)
                fill[..., :18] = src['g0'][k] if (mask >> k) & 1 else NAN
                gs.append(Out((B, HW, ld), dev, fill=fill))
            gp = [g.ptr() for g in gs] + [None] * (top - nf)
            dw1, dw2 = Out(4 * nf + 2, dev, torch.float64, fill=src['dw1_0']), Out(256 * nf + 16, dev, torch.float64, fill=src['dw2_0'])
            _lib.check(bwd(d1.data_ptr(), d2.data_ptr(), *fp, nf, w1.data_ptr(), w2.data_ptr(), *gp, mask, dw1.ptr(), dw2.ptr(), B, HW, ld, st()))
            torch.cuda.synchronize()
            what = f'{K.final_id(r)} ld {ld} mask {mask}'
            for k in range(nf):
                got = gs[k].check(f'g{k}')
                assert bool((got[..., 18:] == 3.5).all()), f'{what}: pad channels of g{k} written'
                assert np.isfinite(got[..., :18]).all(), f'{what}: g{k} not defined everywhere'
                gate('final_dfeat', f'{what} g{k}', got[..., :18], r64['g'][k], r32['g'][k])
            gate('final_wgrad', f'{what} dw1', dw1.check('dw1'), r64['dw1'], r32['dw1'])
            gate('final_wgrad', f'{what} dw2', dw2.check('dw2'), r64['dw2'], r32['dw2'])
    print(f'GATE {K.final_id(r)}: worst e / e_cpu32 ' + '  '.join(f'{k} {v:.2f}' for k, v in need.items()))
    assert not fails, fails
    for t, k in zip(feats, src['feats']):
        assert np.array_equal(t.cpu().numpy(), k)
