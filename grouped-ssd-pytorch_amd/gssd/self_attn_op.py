"""Standalone, differentiable Self_Attn for any channel count (layers/self_attn.py:46-89 + layers/spectral_norm.py:69-89): the
``forward`` of gssd.modules.Self_Attn, on HIP kernels only.

Forward: one gssd_spectral_norm_f32 launch over the four matrices (train mode: one power iteration, in place, also under
``torch.no_grad()``), the merged theta | phi | g projection (gssd_conv2d_nhwc_f32, alpha = 1 / sigma_sn), P x P average pooling of the
keys / values for ``max_pool_factor`` > 1 (gssd_sa_pool_kv_f32), the flash-style core gssd_self_attn_core_any_f32 (csrc/sa_any.hip; keeps
the rows' log-sum-exp and no map), the output conv with the ``sigma`` gate and the residual.  Backward: the order of
gssd/bwd_ops.py::_sa / _sa_tail with the map-free MFMA backward gssd_self_attn_flash_bwd_any_f32 in place of the explicit maps.
u, v of the power iteration are constants of the graph (the backward uses the copies its own forward made, as the reference's
clones do: two forwards followed by one backward work); sigma_sn = u^T W v is differentiated through W (gssd_sn_weight_grad_f32).

D = C / 8 theta | phi channels are carried padded to a multiple of 4 (zero weight rows, zero bias, zero 1 / sigma_sn: the pad channels
are exactly 0); C2 = C / 2 always is one.  ``attn`` (only with ``return_attn_map=True``) is exp(S - lse) from gssd_bgemm_ex_f32 mode 1, the
only [B, N, Nk] allocation of the op, and is NOT differentiable: the reference's map is, but nothing in the reference differentiates it.
fp32 CUDA tensors only; no host synchronisation once the module's spectral-norm table exists (built on the first call); current stream.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops
from ._lib import GssdError, check, lib
from .ops import _p, _stream, make_conv_desc, round_up

MAX_CHANNELS = 2048
_CONVS = ('theta', 'phi', 'g', 'attn')


def _conv1x1(inp, w, out, M, cin, cout, **kw):
    """out[M][cout] = inp[M][cin] . w[cout][cin]^T with the descriptor's epilogue (alpha, bias, gate, resid, out2): the existing 1x1
    conv, on csrc/conv_x6.hip for the launches the engine hands it (ops.x6_wanted: wide, long-K GEMMs over at least 4096 tokens)."""
    d, _, _ = make_conv_desc(inp, w, out, B=1, H=M, W=1, in_stride=cin, cin_g=cin, Cout=cout, wgt_x6=w, **kw)
    xw = None
    if ops.x6_wanted(1, cin, cout, 1, M) and lib.gssd_conv_x6_takes(C.byref(d)) == 1:
        xw = ops.x6_weight(w[:cout], 1, cin, 1, ops.x6_tile(cout, 1, M))      # (w may hold more rows: the merged projection's g part)
    d.wgt_x6 = _p(xw)
    check(lib.gssd_conv2d_nhwc_f32(C.byref(d), _stream()))


def _wgrad(inp, M, cin, dy, cout):
    """dW[cout][cin] = dy[M][cout]^T . inp[M][cin]"""
    dw = torch.zeros(cout, cin, device=inp.device, dtype=torch.float32)
    d, _, _ = make_conv_desc(inp, None, None, B=1, H=M, W=1, in_stride=cin, cin_g=cin, Cout=cout)
    check(lib.gssd_conv2d_wgrad_f32(C.byref(d), _p(dy), _p(dw), _stream()))
    return dw


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


class _Shape:
    def __init__(self, B, Cc, H, mpf):
        self.B, self.C, self.H, self.N = B, Cc, H, H * H
        self.D, self.Dp, self.C2 = Cc // 8, round_up(Cc // 8, 4), Cc // 2
        self.CT = 2 * self.Dp + self.C2                    # theta | phi | g rows of the merged projection
        self.Np = round_up(self.N, 4)
        self.P = max(H // int(mpf), 1)
        self.pooled = self.P != H
        self.Nk = self.P * self.P
        self.Nkp = round_up(self.Nk, 4)
        self.rows = ((0, self.D), (self.Dp, self.D), (2 * self.Dp, self.C2))      # (first row, rows) of theta, phi, g


def _sn_state(module, s):
    """The module's spectral-norm table (gssd_sn_item[4] on the device) and the 1 / sigma_sn vectors it writes; rebuilt when a tensor
    of the module has moved."""
    ts = []
    for k in _CONVS:
        m = getattr(module, 'snconv1x1_' + k)
        ts += [m.weight_orig, m.weight_u, m.weight_v]
    key = tuple(t.data_ptr() for t in ts)
    st = module.__dict__.get('_sn_state')
    if st is None or st[0] != key:
        dev = ts[0].device
        a_tpg = torch.zeros(s.CT, device=dev, dtype=torch.float32)
        a_o = torch.zeros(s.C, device=dev, dtype=torch.float32)
        outs = [a_tpg[r0:r0 + n] for r0, n in s.rows] + [a_o]
        items = [(ts[3 * i].detach(), ts[3 * i + 1], ts[3 * i + 2], outs[i]) for i in range(4)]
        st = (key, ops.sn_items_tensor(items, dev), a_tpg, a_o)
        module.__dict__['_sn_state'] = st
    return st


class _SelfAttnFn(torch.autograd.Function):
    """apply(x, sigma, w_theta, w_phi, w_g, w_attn, b_theta, b_phi, b_g, b_attn, a_tpg, a_o, uv, shape, want_map): (out, sigma * attn_g
    [, attn]).  a_tpg / a_o: 1 / sigma_sn per output channel, uv: the (u, v) of the four convs -- this call's own copies."""

    @staticmethod
    def forward(ctx, x, sigma, wt, wp, wg, wo, bt, bp, bg, bo, a_tpg, a_o, uv, s, want_map):
        ctx.set_materialize_grads(False)
        dev, f32 = x.device, torch.float32
        B, Cc, H, N, Dp, C2, CT, Np = s.B, s.C, s.H, s.N, s.Dp, s.C2, s.CT, s.Np
        M = B * N
        xh = _nhwc(x)
        w_tpg = torch.zeros(CT, Cc, device=dev, dtype=f32)
        b_tpg = torch.zeros(CT, device=dev, dtype=f32)
        for (r0, n), w, b in zip(s.rows, (wt, wp, wg), (bt, bp, bg)):
            w_tpg[r0:r0 + n].copy_(w.detach().view(n, Cc))
            b_tpg[r0:r0 + n].copy_(b.detach())
        w_o = wo.detach().view(Cc, C2)
        # theta | phi token-major, g channel-major (tokens contiguous, pad columns zero)
        tp = torch.empty(B, N, 2 * Dp, device=dev, dtype=f32)
        gT = torch.zeros(B, C2, Np, device=dev, dtype=f32)
        _conv1x1(xh, w_tpg, tp, M, Cc, 2 * Dp, bias=b_tpg, alpha=a_tpg)
        d, _, _ = make_conv_desc(xh, w_tpg[2 * Dp:], gT, B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C2, bias=b_tpg[2 * Dp:],
                                 alpha=a_tpg[2 * Dp:], out_mode=_lib.OUT_TRANSPOSED, out_stride=Np, m_per_image=True,
                                 in_batch_stride=N * Cc, out_batch_stride=C2 * Np)
        check(lib.gssd_conv2d_nhwc_f32(C.byref(d), _stream()))
        kp = gTp = None
        keys, krow, vals = tp[0, 0, Dp:], 2 * Dp, gT
        if s.pooled:                       # layers/self_attn.py:57-59, 67, 76: keys / values average-pooled to a P x P grid
            kp = torch.empty(B, s.Nk, Dp, device=dev, dtype=f32)
            gTp = torch.zeros(B, C2, s.Nkp, device=dev, dtype=f32)
            check(lib.gssd_sa_pool_kv_f32(_p(tp), _p(gT), _p(kp), _p(gTp), B, H, s.P, Dp, C2, Np, s.Nkp, _stream()))
            keys, krow, vals = kp, Dp, gTp
        ag = torch.empty(B, N, C2, device=dev, dtype=f32)
        lse = torch.empty(B, N, device=dev, dtype=f32)
        check(lib.gssd_self_attn_core_any_f32(_p(tp), _p(keys), _p(vals), _p(ag), B, N, s.Nk, s.Nkp, Dp, C2, krow, _p(lse), _stream()))
        out = torch.empty(B, H, H, Cc, device=dev, dtype=f32)
        out2 = torch.empty(B, H, H, Cc, device=dev, dtype=f32)
        _conv1x1(ag, w_o, out, M, C2, Cc, bias=bo.detach(), alpha=a_o, gate=sigma.detach(), resid=xh, out2=out2)
        ctx.s, ctx.uv = s, uv
        ctx.save_for_backward(xh, tp, gT, kp, gTp, ag, lse, w_tpg, a_tpg, a_o, sigma, wt, wp, wg, wo, bo)
        res = (_nchw(out), _nchw(out2))
        if want_map:
            A = torch.empty(B, N, s.Nkp, device=dev, dtype=f32)
            check(lib.gssd_bgemm_ex_f32(_p(tp), _p(keys), _p(A), N, s.Nk, Dp, 2 * Dp, krow, s.Nkp, 0, 1, N * 2 * Dp, s.Nk * krow,
                                        N * s.Nkp, B, 1.0, 1, _p(lse), None, _stream()))
            A = A[..., :s.Nk]
            ctx.mark_non_differentiable(A)
            res += (A,)
        return res

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_out2, *_):
        none = (None,) * 15
        if g_out is None and g_out2 is None:
            return none
        xh, tp, gT, kp, gTp, ag, lse, w_tpg, a_tpg, a_o, sigma, wt, wp, wg, wo, bo = ctx.saved_tensors
        s, uv = ctx.s, ctx.uv
        nx, nsig, nwt, nwp, nwg, nwo, nbt, nbp, nbg, nbo = ctx.needs_input_grad[:10]
        nw, nb = (nwt, nwp, nwg), (nbt, nbp, nbg)
        need_core = nx or any(nw) or any(nb)               # everything behind the attention core
        if not (need_core or nsig or nwo or nbo):
            return none
        dev, f32, f64 = xh.device, torch.float32, torch.float64
        B, Cc, H, N, Dp, C2, CT = s.B, s.C, s.H, s.N, s.Dp, s.C2, s.CT
        M, st = B * N, _stream()
        for g in (g_out, g_out2):
            if g is not None and (not g.is_cuda or g.dtype != f32):
                raise GssdError(f'Self_Attn backward: gradients must be float32 on the MI355X (got {g.dtype} on {g.device})')
        go = _nhwc(g_out) if g_out is not None else None
        T = go                                              # T = d(out) + d(sigma * attn_g)
        if g_out2 is not None:
            T = _nhwc(g_out2)
            if go is not None:
                check(lib.gssd_axpby_f32(_p(go), _p(T), _p(T), M * Cc, 1.0, 1.0, st))
        w_o = wo.view(Cc, C2)
        grads = [None] * 10
        # d(ag)' = T W_o^T / sigma_sn; everything below is linear in d(ag) = sigma d(ag)', sigma is applied where the chains end
        dag = None
        if need_core or nsig:
            wd_o = torch.empty(C2, Cc, device=dev, dtype=f32)
            check(lib.gssd_scaled_transpose_f32(_p(w_o), _p(a_o), _p(wd_o), Cc, C2, st))
            dag = torch.empty(B, N, C2, device=dev, dtype=f32)
            _conv1x1(T, wd_o, dag, M, Cc, C2)
        if nsig or nbo:
            csT = torch.zeros(Cc, device=dev, dtype=f64)
            check(lib.gssd_colsum_f32(_p(T), M, Cc, Cc, _p(csT), st))
            if nsig:                                        # d sigma = <d(ag)', ag> + <b_o, colsum T>
                dot = torch.zeros(1, device=dev, dtype=f64)
                check(lib.gssd_dot_f32(_p(dag), _p(ag), M * C2, _p(dot), st))
                grads[1] = torch.empty_like(sigma)
                check(lib.gssd_sa_sigma_grad_f32(_p(dot), _p(csT), _p(bo), Cc, _p(grads[1]), st))
            if nbo:
                grads[9] = torch.empty(Cc, device=dev, dtype=f32)
                check(lib.gssd_scale_cast_f64_f32(_p(csT), _p(sigma), _p(grads[9]), Cc, st))
        sndot = torch.zeros(4, device=dev, dtype=f64)       # <dW_eff, W> of the four convs
        if nwo:
            dwo = _wgrad(ag, M, C2, T, Cc)
            grads[5] = torch.empty_like(wo)
            check(lib.gssd_sn_weight_grad_f32(_p(dwo), C2, _p(w_o), _p(uv[3][0]), _p(uv[3][1]), _p(a_o), _p(sigma), _p(sndot[3:]),
                                              _p(grads[5]), Cc, C2, st))
        if not need_core:
            return tuple(grads) + (None,) * 5
        # [d theta | d keys | d values] without a map
        dvec = torch.empty(B, N, device=dev, dtype=f32)
        check(lib.gssd_rowdot_f32(_p(dag), _p(ag), _p(dvec), M, C2, st))
        dtpg = torch.empty(B, N, CT, device=dev, dtype=f32)
        if s.pooled:
            CW = Dp + C2
            dkg = torch.empty(B, s.Nk, CW, device=dev, dtype=f32)           # d(pooled phi) | d(pooled g) per cell
            keys, krow, vals, dk, dv, ld_kv = kp, Dp, gTp, dkg, dkg[0, 0, Dp:], CW
        else:
            keys, krow, vals, dk, dv, ld_kv = tp[0, 0, Dp:], 2 * Dp, gT, dtpg[0, 0, Dp:], dtpg[0, 0, 2 * Dp:], CT
        check(lib.gssd_self_attn_flash_bwd_any_f32(_p(tp), 2 * Dp, _p(keys), krow, _p(vals), s.Nkp, _p(dag), _p(lse), _p(dvec), _p(dtpg),
                                                   CT, _p(dk), _p(dv), ld_kv, B, N, s.Nk, Dp, C2, st))
        if s.pooled:
            check(lib.gssd_sa_unpool_f32(_p(dkg), _p(dtpg[0, 0, Dp:]), B, H, s.P, CW, CT, st))
        # projection weights / biases (gssd/bwd_ops.py::_sa_tail)
        if any(nw):
            dwp = _wgrad(xh, M, Cc, dtpg, CT)
            for i, ((r0, n), w) in enumerate(zip(s.rows, (wt, wp, wg))):
                if nw[i]:
                    grads[2 + i] = torch.empty_like(w)
                    check(lib.gssd_sn_weight_grad_f32(_p(dwp[r0:]), Cc, _p(w), _p(uv[i][0]), _p(uv[i][1]), _p(a_tpg[r0:]), _p(sigma),
                                                      _p(sndot[i:]), _p(grads[2 + i]), n, Cc, st))
        if any(nb):
            csP = torch.zeros(CT, device=dev, dtype=f64)
            check(lib.gssd_colsum_f32(_p(dtpg), M, CT, CT, _p(csP), st))
            for i, (r0, n) in enumerate(s.rows):
                if nb[i]:
                    grads[6 + i] = torch.empty(n, device=dev, dtype=f32)
                    check(lib.gssd_scale_cast_f64_f32(_p(csP[r0:]), _p(sigma), _p(grads[6 + i]), n, st))
        if nx:                                              # dx = d(out) + sigma [d theta | d phi | d g] W_tpg / sigma_sn
            wd_p = torch.empty(Cc, CT, device=dev, dtype=f32)
            check(lib.gssd_scaled_transpose_f32(_p(w_tpg), _p(a_tpg), _p(wd_p), CT, Cc, st))
            dx = torch.empty(B, H, H, Cc, device=dev, dtype=f32)
            _conv1x1(dtpg, wd_p, dx, M, CT, Cc, gate=sigma, resid=go)
            grads[0] = _nchw(dx)
        return tuple(grads) + (None,) * 5


def self_attn_forward(module, x, return_attn_map=False):
    """``Self_Attn.forward`` of gssd.modules: (out, sigma * attn_g) or (out, sigma * attn_g, attn)."""
    Cc = int(module.in_channels)
    if not torch.is_tensor(x) or x.dim() != 4:
        raise ValueError(f'Self_Attn: a [B, C, H, W] tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    B, ch, h, w = x.shape
    if Cc % 8 != 0 or Cc < 8:
        raise ValueError(f'Self_Attn: in_channels {Cc} is not a positive multiple of 8 (input {tuple(x.shape)})')
    if Cc > MAX_CHANNELS:
        raise ValueError(f'Self_Attn: in_channels {Cc} > {MAX_CHANNELS} (input {tuple(x.shape)})')
    if ch != Cc:
        raise ValueError(f'Self_Attn: input {tuple(x.shape)} has {ch} channels, the module {Cc}')
    if h != w or h == 0 or B == 0:
        raise ValueError(f'Self_Attn: a square, non-empty map is needed, got {tuple(x.shape)}')
    ps = [module.sigma]
    for k in _CONVS:
        m = getattr(module, 'snconv1x1_' + k)
        ps += [m.weight_orig, m.bias, m.weight_u, m.weight_v]
    for t in [x] + ps:
        if not t.is_cuda or t.dtype != torch.float32:
            raise GssdError(f'Self_Attn: the input and the module must be float32 on the MI355X (got {t.dtype} on {t.device}); '
                            'there is no CPU fallback')
    s = _Shape(B, Cc, h, module.max_pool_factor)
    _, items, a_tpg, a_o = _sn_state(module, s)
    ops.spectral_norm(items, 4, module.training)        # train: updates weight_u / weight_v in place before the weights are used
    cv = [getattr(module, 'snconv1x1_' + k) for k in _CONVS]
    uv = [(m.weight_u.clone(), m.weight_v.clone()) for m in cv]
    return _SelfAttnFn.apply(x, module.sigma, cv[0].weight_orig, cv[1].weight_orig, cv[2].weight_orig, cv[3].weight_orig, cv[0].bias,
                             cv[1].bias, cv[2].bias, cv[3].bias, a_tpg.clone(), a_o.clone(), uv, s, bool(return_attn_map))
