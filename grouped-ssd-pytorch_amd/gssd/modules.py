"""Parameter containers that mirror the reference's module tree (names, shapes, state-dict keys)
so checkpoints load strictly in both directions.  Inside build_ssd / PixelLink they hold weights only; the arithmetic runs in
the HIP engine (``gssd/engine.py``).

Key compatibility (probed against the reference):
  * ``Self_Attn``: ``snconv1x1_{theta,phi,g,attn}.{bias,weight_orig,weight_u,weight_v}``, ``sigma``
    (layers/self_attn.py:29-44 + layers/spectral_norm.py:126-139)
  * ``DCN``: ``weight``, ``bias``, ``conv_offset_mask.{weight,bias}`` (layers/dcn_v2_custom.py:18-77)
  * ``L2Norm``: ``weight`` (layers/modules/l2norm.py:7-17)
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.nn.init as init


class L2Norm(nn.Module):
    """layers/modules/l2norm.py: learnable per-channel scale (init ``scale``), eps 1e-10 after sqrt."""

    def __init__(self, n_channels, scale):
        super().__init__()
        self.n_channels = n_channels
        self.gamma = scale or None
        self.eps = 1e-10
        self.weight = nn.Parameter(torch.empty(n_channels))
        init.constant_(self.weight, self.gamma)

    def forward(self, x):
        """NCHW in / NCHW out, HIP kernel underneath."""
        from . import ops
        xh = x.permute(0, 2, 3, 1).contiguous()
        return ops.l2norm(xh, self.weight.detach(), self.eps).permute(0, 3, 1, 2)


class SNConv1x1(nn.Module):
    """A spectral-normed 1x1 conv's state: ``weight_orig``, ``bias`` (parameters), ``weight_u``,
    ``weight_v`` (buffers, unit vectors) -- layers/spectral_norm.py:111-139."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        w = torch.empty(out_channels, in_channels, 1, 1)
        init.kaiming_uniform_(w, a=math.sqrt(5))            # nn.Conv2d default
        self.weight_orig = nn.Parameter(w)
        bound = 1.0 / math.sqrt(in_channels)
        self.bias = nn.Parameter(torch.empty(out_channels).uniform_(-bound, bound))
        self.register_buffer('weight_u', F.normalize(torch.randn(out_channels), dim=0, eps=1e-12))
        self.register_buffer('weight_v', F.normalize(torch.randn(in_channels), dim=0, eps=1e-12))


class Self_Attn(nn.Module):
    """layers/self_attn.py:29-89.  Inside build_ssd / PixelLink ``GssdEngine`` runs it; ``forward`` is the standalone, differentiable
    block (gssd/self_attn_op.py) for any ``in_channels`` that is a multiple of 8 up to 2048, any square map and any
    ``max_pool_factor``."""

    def __init__(self, in_channels, max_pool_factor=1):
        super().__init__()
        self.in_channels = in_channels
        self.snconv1x1_theta = SNConv1x1(in_channels, in_channels // 8)
        self.snconv1x1_phi = SNConv1x1(in_channels, in_channels // 8)
        self.snconv1x1_g = SNConv1x1(in_channels, in_channels // 2)
        self.snconv1x1_attn = SNConv1x1(in_channels // 2, in_channels)
        self.sigma = nn.Parameter(torch.zeros(1))
        self.max_pool_factor = max_pool_factor

    def forward(self, x, return_attn_map=False):
        """NCHW fp32 on the device in; (out, sigma * attn_g) or, with ``return_attn_map``, (out, sigma * attn_g, attn) with attn
        [B, H*H, Nk], Nk = max(H // max_pool_factor, 1) ** 2.  ``attn`` is not differentiable (nothing in the reference differentiates
        its map); in train mode one power iteration updates ``weight_u`` / ``weight_v`` in place, also under ``torch.no_grad()``."""
        from .self_attn_op import self_attn_forward
        return self_attn_forward(self, x, return_attn_map)


def _pair(v):
    return tuple(int(a) for a in v) if isinstance(v, (tuple, list)) else (int(v), int(v))


class DCNv2(nn.Module):
    """layers/dcn_v2_custom.py:18-55: modulated deformable conv with caller-supplied offsets and mask; any geometry.  ``forward`` runs
    gssd.dcn_op.dcn_v2_conv (HIP sampling kernels + the HIP 1x1 contraction; fp32 CUDA tensors only)."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), _pair(dilation)
        self.deformable_groups = deformable_groups
        kh, kw = self.kernel_size
        stdv = 1.0 / math.sqrt(in_channels * kh * kw)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, kh, kw).uniform_(-stdv, stdv))
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def forward(self, input, offset, mask):
        from .dcn_op import dcn_v2_conv
        return dcn_v2_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation,
                           self.deformable_groups)


class DCN(DCNv2):
    """layers/dcn_v2_custom.py:58-89: DCNv2 whose offsets and mask come from ``conv_offset_mask`` (zero-initialised).  The engine
    (build_ssd, PixelLink) reads its weights and runs only 3x3 / stride 1 / pad 1 / dilation 1; ``forward`` (the standalone module)
    takes any square kernel with isotropic stride and padding -- the offset conv runs on the engine's conv descriptor, which has one
    kernel size, one stride and one padding."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, padding, dilation=1, deformable_groups=1):
        kh, kw = _pair(kernel_size)
        (sh, sw), (ph, pw) = _pair(stride), _pair(padding)
        if kh != kw or sh != sw or ph != pw:
            raise NotImplementedError(f'DCN: kernel {(kh, kw)}, stride {(sh, sw)}, padding {(ph, pw)}: the offset / mask conv runs on '
                                      f'a conv with one square kernel, one stride and one padding (DCNv2 / dcn_v2_conv take any)')
        if ph > kh - 1:
            raise NotImplementedError(f'DCN: padding {ph} > kernel_size - 1: the offset conv\'s data gradient has no such form here')
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, deformable_groups)
        self.conv_offset_mask = nn.Conv2d(in_channels, deformable_groups * 3 * kh * kw, kernel_size=self.kernel_size, stride=self.stride,
                                          padding=self.padding, bias=True)
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def is_engine_geometry(self):
        """The geometry of the detector's DCN layers, the only one the engine's fused kernels run."""
        return (self.kernel_size, self.stride, self.padding, self.dilation) == ((3, 3), (1, 1), (1, 1), (1, 1))

    def forward(self, input):
        """(out, offset) as the reference: offset = the first 2*dg*kh*kw channels of conv_offset_mask(input), mask = sigmoid of
        the rest (applied inside the sampling kernel)."""
        k, s, p = self.kernel_size[0], self.stride[0], self.padding[0]
        (dh, dw) = self.dilation
        H, W = input.shape[2], input.shape[3]
        om_size = ((H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1)
        size = ((H + 2 * p - dh * (k - 1) - 1) // s + 1, (W + 2 * p - dw * (k - 1) - 1) // s + 1)
        if om_size != size:
            raise ValueError(f'DCN: dilation {self.dilation} makes the deformable conv\'s output {size} differ from the offset conv\'s '
                             f'{om_size} (the reference\'s offset conv has no dilation)')
        from .dcn_op import dcn_forward
        return dcn_forward(self, input)
