"""Standalone, differentiable DCNv2 for any conv geometry: layers/dcn_v2_custom.py's ``dcn_v2_conv`` (= ``_DCNv2.apply``) and the
forward of its ``DCN`` module (offset / mask conv included), on HIP kernels only.

Forward: NHWC copies of the inputs (plumbing), the sampling kernel gssd_dcn_geo_im2col_f32 into a column matrix
[B*Ho*Wo][kh*kw*Cp] (Cp = C rounded up to 4), the existing 1x1 contraction gssd_conv2d_nhwc_f32 with bias (conv_x6 where
gssd_conv_x6_takes accepts the descriptor), NCHW out.  Backward: bias gradient by gssd_colsum_f32, weight gradient by
gssd_conv2d_wgrad_f32 over the rebuilt columns, d(cols) by the transposed-weight 1x1 conv, then gssd_dcn_geo_col2im_f32 for d(x),
d(offset) and d(mask).  Output channels are carried padded to a multiple of 4 (zero weight rows) because the GEMMs need it.

The column workspace is bounded by processing the batch in chunks of at most ``WORKSPACE_BYTES`` (forward columns; backward columns
plus d(cols)); a single image larger than the cap still runs as one chunk.  fp32 CUDA tensors only; no host synchronisation.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import DcnGeom, GssdError, check, lib
from .ops import _p, _stream, make_conv_desc, round_up

WORKSPACE_BYTES = 256 << 20


def _pair(v, name):
    t = tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v), int(v))
    if len(t) != 2:
        raise ValueError(f'{name}: an int or a pair, got {v!r}')
    return t


def _need_f32_cuda(**ts):
    for name, t in ts.items():
        if t is None:
            continue
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            what = 'a non-tensor' if not torch.is_tensor(t) else f'{t.dtype} on {t.device}'
            raise GssdError(f'dcn_v2_conv: {name} must be a float32 tensor on the MI355X (got {what}); there is no CPU fallback')


def _nhwc(t, stride=None):
    """NCHW -> contiguous NHWC [B][H][W][stride] (channels beyond the tensor's zero)."""
    B, Cc, H, W = t.shape
    if stride is None or stride == Cc:
        return t.detach().permute(0, 2, 3, 1).contiguous()
    out = torch.zeros(B, H, W, stride, device=t.device, dtype=torch.float32)
    out[..., :Cc].copy_(t.detach().permute(0, 2, 3, 1))
    return out


def _chunks(B, image_bytes):
    per = max(1, WORKSPACE_BYTES // max(1, image_bytes))
    return [(b0, min(B, b0 + per)) for b0 in range(0, B, per)]


class _Geo:
    """Shapes of one call and the gssd_dcn_geom handed to the sampling kernels."""

    def __init__(self, B, Cin, H, W, kh, kw, stride, padding, dilation, dg, off_stride, mask_stride, logit):
        (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
        self.B, self.C, self.H, self.W, self.kh, self.kw, self.dg = B, Cin, H, W, kh, kw, dg
        self.Ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
        self.Wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1
        if self.Ho <= 0 or self.Wo <= 0:
            raise ValueError(f'dcn_v2_conv: empty output ({self.Ho} x {self.Wo}) for a {H} x {W} input')
        self.K = kh * kw
        self.Cp = round_up(Cin, 4)
        self.Kc = self.K * self.Cp
        self.g = DcnGeom(B, H, W, Cin, self.Cp, self.Ho, self.Wo, kh, kw, sh, sw, ph, pw, dh, dw, dg, off_stride, mask_stride, int(logit))
        if self.Ho * self.Wo * self.Kc >= (1 << 31):
            raise GssdError(f'dcn_v2_conv: one image\'s column matrix ({self.Ho * self.Wo} x {self.Kc}) exceeds the 32-bit GEMM range')

    @property
    def rows(self):
        return self.Ho * self.Wo


def _conv1x1(inp, ld, cin, wp, cout, out, M, bias=None):
    """out[M][cout] = inp[M][ld, first cin] . wp[cout][cin]^T (+ bias): the existing 1x1 conv, on csrc/conv_x6.hip where it takes the
    descriptor."""
    d, _, _ = make_conv_desc(inp, wp, out, B=1, H=M, W=1, in_stride=ld, cin_g=cin, Cout=cout, bias=bias, wgt_x6=wp)
    if lib.gssd_conv_x6_takes(C.byref(d)) == 1:
        d.wgt_x6 = _p(ops.x6_weight(wp, 1, cin, 1, ops.x6_tile(cout, 1, M)))
    else:
        d.wgt_x6 = 0
    check(lib.gssd_conv2d_nhwc_f32(C.byref(d), _stream()))
    return d


def _pack_main(weight, geo, coutp):
    Cout = weight.shape[0]
    wp = torch.zeros(coutp, geo.Kc, device=weight.device, dtype=torch.float32)
    w = weight.detach().contiguous()
    check(lib.gssd_pack_conv_weight(_p(w), _p(wp), Cout, geo.C, geo.kh, geo.kw, geo.Cp, geo.Kc, _stream()))
    return wp


def _padded(v, n, device):
    out = torch.zeros(n, device=device, dtype=torch.float32)
    if v is not None:
        out[:v.numel()].copy_(v.detach().reshape(-1))
    return out


def sample_forward(xh, off, msk, wp, bp, coutp, geo):
    """NHWC out [B][Ho][Wo][coutp] = the deformable conv of xh (NHWC, stride Cp) with offsets / mask rows ``off`` / ``msk`` (pointers
    into NHWC maps with the strides of ``geo``)."""
    B, rows = geo.B, geo.rows
    out = torch.empty(B, geo.Ho, geo.Wo, coutp, device=xh.device, dtype=torch.float32)
    ch = _chunks(B, rows * geo.Kc * 4)
    cols = torch.empty((ch[0][1] - ch[0][0]) * rows, geo.Kc, device=xh.device, dtype=torch.float32)
    for b0, b1 in ch:
        check(lib.gssd_dcn_geo_im2col_f32(_p(xh), off, msk, _p(cols), C.byref(geo.g), b0, b1, _stream()))
        _conv1x1(cols, geo.Kc, geo.Kc, wp, coutp, out[b0:b1], (b1 - b0) * rows, bias=bp)
    return out


def sample_backward(dyp, xh, off, msk, wp, coutp, geo, need_w, need_b, dx, doff, dmsk):
    """Gradients of :func:`sample_forward` for the NHWC d(out) ``dyp`` [B*Ho*Wo][coutp]: returns (packed dW [coutp][Kc] or None,
    fp64 bias column sums [coutp] or None); ADDS d(x) into ``dx`` (NHWC, stride Cp; may be None) and WRITES d(offset) / d(mask) at the
    pointers ``doff`` / ``dmsk`` (0 = not wanted)."""
    B, rows, Kc, dev = geo.B, geo.rows, geo.Kc, xh.device
    dwp = torch.zeros(coutp, Kc, device=dev, dtype=torch.float32) if need_w else None
    cs = None
    if need_b:
        cs = torch.zeros(coutp, device=dev, dtype=torch.float64)
        check(lib.gssd_colsum_f32(_p(dyp), B * rows, coutp, coutp, _p(cs), _stream()))
    need_s = dx is not None or doff
    if not (need_w or need_s):
        return dwp, cs
    wt = None
    if need_s:
        wt = torch.empty(Kc, coutp, device=dev, dtype=torch.float32)
        check(lib.gssd_scaled_transpose_f32(_p(wp), None, _p(wt), coutp, Kc, _stream()))
    ch = _chunks(B, rows * Kc * 4 * (int(need_w) + int(bool(need_s))))
    n0 = (ch[0][1] - ch[0][0]) * rows
    cols = torch.empty(n0, Kc, device=dev, dtype=torch.float32) if need_w else None
    dcols = torch.empty(n0, Kc, device=dev, dtype=torch.float32) if need_s else None
    for b0, b1 in ch:
        M = (b1 - b0) * rows
        dy = dyp[b0 * rows:b1 * rows]
        if need_w:
            check(lib.gssd_dcn_geo_im2col_f32(_p(xh), off, msk, _p(cols), C.byref(geo.g), b0, b1, _stream()))
            d, _, _ = make_conv_desc(cols, None, None, B=1, H=M, W=1, in_stride=Kc, cin_g=Kc, Cout=coutp)
            check(lib.gssd_conv2d_wgrad_f32(C.byref(d), _p(dy), _p(dwp), _stream()))
        if need_s:
            _conv1x1(dy, coutp, coutp, wt, Kc, dcols, M)
            check(lib.gssd_dcn_geo_col2im_f32(_p(xh), off, msk, _p(dcols), _p(dx), doff or None, dmsk or None, C.byref(geo.g), b0, b1,
                                              _stream()))
    return dwp, cs


def _unpack_weight_grad(dwp, Cout, cin, kh, kw, cin_pad, Kc):
    g = torch.empty(Cout, cin, kh, kw, device=dwp.device, dtype=torch.float32)
    check(lib.gssd_unpack_conv_weight_grad(_p(dwp), _p(g), Cout, cin, kh, kw, cin_pad, Kc, 0, _stream()))
    return g


def _bias_grad(cs, n):
    g = torch.empty(n, device=cs.device, dtype=torch.float32)
    check(lib.gssd_cast_f64_f32(_p(cs), _p(g), n, 0, _stream()))
    return g


def _dy_padded(grad, coutp):
    """NCHW d(out) -> NHWC [B*Ho*Wo][coutp] (zero pad channels)."""
    B, Cout, Ho, Wo = grad.shape
    return _nhwc(grad, coutp).view(B * Ho * Wo, coutp)


def _nchw(t_nhwc, c):
    return t_nhwc[..., :c].permute(0, 3, 1, 2).contiguous()


class _DCNv2(torch.autograd.Function):
    """dcn_v2's ``_DCNv2``: apply(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
        _need_f32_cuda(input=input, offset=offset, mask=mask, weight=weight, bias=bias)
        stride, padding, dilation = _pair(stride, 'stride'), _pair(padding, 'padding'), _pair(dilation, 'dilation')
        dg = int(deformable_groups)
        B, Cin, H, W = input.shape
        Cout, cin_w, kh, kw = weight.shape
        K = kh * kw
        if cin_w != Cin or dg <= 0 or Cin % dg:
            raise ValueError(f'dcn_v2_conv: weight {tuple(weight.shape)} / deformable_groups {dg} do not fit {Cin} input channels')
        geo = _Geo(B, Cin, H, W, kh, kw, stride, padding, dilation, dg, 2 * dg * K, dg * K, False)
        if tuple(offset.shape) != (B, 2 * dg * K, geo.Ho, geo.Wo) or tuple(mask.shape) != (B, dg * K, geo.Ho, geo.Wo):
            raise ValueError(f'dcn_v2_conv: offset {tuple(offset.shape)} / mask {tuple(mask.shape)}: expected '
                             f'{(B, 2 * dg * K, geo.Ho, geo.Wo)} / {(B, dg * K, geo.Ho, geo.Wo)}')
        if bias is not None and bias.numel() != Cout:
            raise ValueError(f'dcn_v2_conv: bias of {bias.numel()} elements for {Cout} outputs')
        coutp = round_up(Cout, 4)
        xh, offh, mskh = _nhwc(input, geo.Cp), _nhwc(offset), _nhwc(mask)
        wp, bp = _pack_main(weight, geo, coutp), _padded(bias, coutp, input.device)
        out = sample_forward(xh, _p(offh), _p(mskh), wp, bp, coutp, geo)
        ctx.geo, ctx.coutp, ctx.Cout, ctx.has_bias = geo, coutp, Cout, bias is not None
        ctx.save_for_backward(xh, offh, mskh, wp)
        return _nchw(out, Cout)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        xh, offh, mskh, wp = ctx.saved_tensors
        geo, coutp, Cout = ctx.geo, ctx.coutp, ctx.Cout
        nx, noff, nmsk, nw, nb = ctx.needs_input_grad[:5]
        nb = nb and ctx.has_bias
        if not (nx or noff or nmsk or nw or nb):
            return (None,) * 9
        _need_f32_cuda(grad=grad)
        dyp = _dy_padded(grad, coutp)
        dev = xh.device
        dx = torch.zeros(geo.B, geo.H, geo.W, geo.Cp, device=dev, dtype=torch.float32) if nx else None
        doff = torch.empty_like(offh) if (noff or nmsk) else None
        dmsk = torch.empty_like(mskh) if (noff or nmsk) else None
        dwp, cs = sample_backward(dyp, xh, _p(offh), _p(mskh), wp, coutp, geo, nw, nb, dx, _p(doff), _p(dmsk))
        return (_nchw(dx, geo.C) if nx else None,
                _nchw(doff, doff.shape[-1]) if noff else None,
                _nchw(dmsk, dmsk.shape[-1]) if nmsk else None,
                _unpack_weight_grad(dwp, Cout, geo.C, geo.kh, geo.kw, geo.Cp, geo.Kc) if nw else None,
                _bias_grad(cs, Cout) if nb else None,
                None, None, None, None)


def dcn_v2_conv(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups):
    """Modulated deformable convolution (DCNv2), NCHW in / out, the reference's signature; ints or pairs for stride / padding /
    dilation.  ``mask`` is the modulation itself (no sigmoid)."""
    dg = int(deformable_groups)
    kh, kw = weight.shape[2], weight.shape[3]
    if offset.shape[1] != 2 * dg * kh * kw:
        raise ValueError(f'dcn_v2_conv: offset has {offset.shape[1]} channels, 2 * deformable_groups * kh * kw = {2 * dg * kh * kw}')
    if mask.shape[1] != dg * kh * kw:
        raise ValueError(f'dcn_v2_conv: mask has {mask.shape[1]} channels, deformable_groups * kh * kw = {dg * kh * kw}')
    _need_f32_cuda(input=input, offset=offset, mask=mask, weight=weight, bias=bias)
    return _DCNv2.apply(input, offset, mask, weight, bias, stride, padding, dilation, deformable_groups)


class _DCNFn(torch.autograd.Function):
    """layers/dcn_v2_custom.py DCN.forward: om = conv_offset_mask(x); offset = om[:, :2*dg*K]; mask = sigmoid(om[:, 2*dg*K:]);
    out = dcn_v2_conv(x, offset, mask, ...).  Returns (out, offset); both carry gradient.  The offset / mask conv is a square k,
    isotropic stride / padding conv (checked by gssd.modules.DCN); its output size equals the deformable conv's."""

    @staticmethod
    def forward(ctx, x, w_om, b_om, weight, bias, k, s, p, dilation, dg):
        ctx.set_materialize_grads(False)
        B, Cin, H, W = x.shape
        Cout = weight.shape[0]
        K = k * k
        OMC = 3 * dg * K
        OMCp = round_up(OMC, 4)
        geo = _Geo(B, Cin, H, W, k, k, (s, s), (p, p), dilation, dg, OMCp, OMCp, True)
        Cp = geo.Cp
        xh = _nhwc(x, Cp)
        # offset / mask conv on the existing HIP conv (rows padded to OMCp output channels, zero weights / bias there)
        wpo = torch.zeros(OMCp, geo.Kc, device=x.device, dtype=torch.float32)
        check(lib.gssd_pack_conv_weight(_p(w_om.detach().contiguous()), _p(wpo), OMC, Cin, k, k, Cp, geo.Kc, _stream()))
        bpo = _padded(b_om, OMCp, x.device)
        om = torch.empty(B, geo.Ho, geo.Wo, OMCp, device=x.device, dtype=torch.float32)
        d, Ho, Wo = make_conv_desc(xh, wpo, om, B=B, H=H, W=W, in_stride=Cp, cin_g=Cp, Cout=OMCp, k=k, stride=s, pad=p, bias=bpo)
        assert (Ho, Wo) == (geo.Ho, geo.Wo), ((Ho, Wo), (geo.Ho, geo.Wo))
        ops.run_conv(d)
        coutp = round_up(Cout, 4)
        wp, bp = _pack_main(weight, geo, coutp), _padded(bias, coutp, x.device)
        out = sample_forward(xh, _p(om), _p(om) + 4 * 2 * dg * K, wp, bp, coutp, geo)
        ctx.geo, ctx.coutp, ctx.Cout, ctx.k, ctx.s, ctx.p, ctx.OMC, ctx.OMCp = geo, coutp, Cout, k, s, p, OMC, OMCp
        ctx.has_bias = (bias is not None, b_om is not None)
        ctx.save_for_backward(xh, om, wp, w_om)
        return _nchw(out, Cout), _nchw(om, 2 * dg * K)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_off):
        xh, om, wp, w_om = ctx.saved_tensors
        geo, coutp, Cout, k, s, p, OMC, OMCp = ctx.geo, ctx.coutp, ctx.Cout, ctx.k, ctx.s, ctx.p, ctx.OMC, ctx.OMCp
        nx, nwo, nbo, nw, nb = ctx.needs_input_grad[:5]
        nb, nbo = nb and ctx.has_bias[0], nbo and ctx.has_bias[1]
        dev, B, H, W, Cp = xh.device, geo.B, geo.H, geo.W, geo.Cp
        rows = B * geo.rows
        need_om = nx or nwo or nbo                   # d(om) feeds all three
        none = (None,) * 5
        if g_out is None and g_off is None:
            return (None,) * 10
        dom = torch.zeros(B, geo.Ho, geo.Wo, OMCp, device=dev, dtype=torch.float32) if need_om else None
        dx = torch.zeros(B, H, W, Cp, device=dev, dtype=torch.float32) if nx else None
        gw = gb = None
        if g_out is not None:
            _need_f32_cuda(grad=g_out)
            dyp = _dy_padded(g_out, coutp)
            off = _p(om)
            dwp, cs = sample_backward(dyp, xh, off, off + 4 * 2 * geo.dg * geo.K, wp, coutp, geo, nw, nb, dx,
                                      _p(dom), _p(dom) + 4 * 2 * geo.dg * geo.K if dom is not None else 0)
            gw = _unpack_weight_grad(dwp, Cout, geo.C, k, k, Cp, geo.Kc) if nw else None
            gb = _bias_grad(cs, Cout) if nb else None
        if need_om and g_off is not None:
            _need_f32_cuda(grad=g_off)
            go = _nhwc(g_off, OMCp)
            check(lib.gssd_axpby_f32(_p(go), _p(dom), _p(dom), dom.numel(), 1.0, 1.0, _stream()))
        gwo = gbo = None
        if need_om and (g_out is not None or g_off is not None):
            if nwo:
                d, _, _ = make_conv_desc(xh, None, None, B=B, H=H, W=W, in_stride=Cp, cin_g=Cp, Cout=OMCp, k=k, stride=s, pad=p)
                dwo = torch.zeros(OMCp, geo.Kc, device=dev, dtype=torch.float32)
                check(lib.gssd_conv2d_wgrad_f32(C.byref(d), _p(dom), _p(dwo), _stream()))
                gwo = _unpack_weight_grad(dwo, OMC, geo.C, k, k, Cp, geo.Kc)
            if nbo:
                cs = torch.zeros(OMCp, device=dev, dtype=torch.float64)
                check(lib.gssd_colsum_f32(_p(dom), rows, OMCp, OMCp, _p(cs), _stream()))
                gbo = _bias_grad(cs, OMC)
            if nx:
                # d(x) += the offset conv's data gradient: a stride-1 conv of d(om) (zeros inserted between its pixels for stride > 1)
                # with the flipped, transposed weights and padding k - 1 - p (bwd_ops._dgrad)
                wpad = torch.zeros(OMCp, Cp, k, k, device=dev, dtype=torch.float32)
                wpad[:OMC, :geo.C].copy_(w_om)
                wd = torch.empty(Cp, k * k * OMCp, device=dev, dtype=torch.float32)
                check(lib.gssd_pack_conv_weight_dgrad(_p(wpad), _p(wd), OMCp, 1, Cp, k, k, _stream()))
                Lh, Lw = H + 2 * p - k + 1, W + 2 * p - k + 1
                src = dom
                if s != 1:
                    src = torch.empty(B, Lh, Lw, OMCp, device=dev, dtype=torch.float32)
                    check(lib.gssd_upsample_insert_f32(_p(dom), _p(src), B, geo.Ho, geo.Wo, Lh, Lw, OMCp, s, _stream()))
                d, Hd, Wd = make_conv_desc(src, wd, dx, B=B, H=Lh, W=Lw, in_stride=OMCp, cin_g=OMCp, Cout=Cp, k=k, pad=k - 1 - p,
                                           resid=dx)
                assert (Hd, Wd) == (H, W), ((Hd, Wd), (H, W))
                ops.run_conv(d)
        return (_nchw(dx, geo.C) if nx else None, gwo, gbo, gw, gb) + none


def dcn_forward(module, x):
    """``DCN.forward`` of gssd.modules: (out, offset)."""
    _need_f32_cuda(input=x, weight=module.weight, bias=module.bias, conv_offset_mask_weight=module.conv_offset_mask.weight,
                   conv_offset_mask_bias=module.conv_offset_mask.bias)
    cm = module.conv_offset_mask
    return _DCNFn.apply(x, cm.weight, cm.bias, module.weight, module.bias, module.kernel_size[0], module.stride[0], module.padding[0],
                        module.dilation, module.deformable_groups)
