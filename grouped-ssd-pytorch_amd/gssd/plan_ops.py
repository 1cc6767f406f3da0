"""Per-op emitters of the forward launch plan: conv + BatchNorm (+ ReLU / pool), stand-alone pools, the merged loc | conf heads, spectral
norm, Self_Attn (layers/self_attn.py:46-89) and the deformable conv (layers/dcn_v2_custom.py:79-89).  Each appends its launches to the
plan and a record for the backward.  Mixin of engine._PlanBase."""
import ctypes as C
import os
import torch
from . import _lib, ops
from ._lib import lib
from . import plan_common
from .plan_common import DCN_X6, HEAD_OFF, MBOX, SN_STREAM, USE_CONV_X6, USE_FLASH_X6, USE_HEADS_WINO, USE_PATCH_X6, USE_WINOGRAD


def bn_arena(dev, modules, replicated):
    """The fp64 batch-sum arena of the BatchNorm layers among ``modules``: (sum, sum of squares) per channel of each, ``replicated`` (ids) in
    R = max(1, min(32, 2048 // channels)) replicas.  Returns (arena, {id: its slice}, {id: replicas}, the num_batches_tracked counters)."""
    uniq = list({id(m): m for m in modules if isinstance(m, torch.nn.BatchNorm2d)}.values())
    rep = {id(m): (max(1, min(32, 2048 // m.num_features)) if id(m) in replicated else 1) for m in uniq}
    stats = torch.zeros(max(sum(2 * m.num_features * rep[id(m)] for m in uniq), 2), device=dev, dtype=torch.float64)
    stat_of, off = {}, 0
    for m in uniq:
        n = 2 * m.num_features * rep[id(m)]
        stat_of[id(m)] = stats[off:off + n]
        off += n
    return stats, stat_of, rep, [m.num_batches_tracked for m in uniq]


class PlanOpsMixin:
    @property
    def f16_ok(self):
        """_lib.CONV_F16_OK for the forward launches of an fp32-mode, TRAIN-mode network, else 0: train-mode BatchNorm (batch statistics) bounds every
        activation map by |gamma| sqrt(n) + |beta|, far inside fp16's range, so the split-operand kernels may use their fp16 planes (three MFMAs per
        product).  Eval mode normalises with running statistics, which bound nothing, and so does a graph built with batch_norm=False (tests/test_gpu_pixellink.py's synthetic eval graph reaches
        1e12): those launches keep the bf16 planes (include/gssd_hip.h: GSSD_CONV_F16_OK)."""
        bn = bool(getattr(self.eng.net, 'batch_norm', False))          # (a graph without BatchNorm -- batch_norm=False, the vanilla SSD -- bounds nothing either)
        return _lib.CONV_F16_OK if (bn and not self.bf16 and self.training) else 0

    def _weight_forms(self, name, groups, cin_g, wino=False, x6_tile=0, taps=9):
        """Register the derived forms of the packed weight ``name``.w BEHIND it (pack jobs run in registration order, so they are refreshed after
        it): ``name``.U, the Winograd F(2x2,3x3) transform (``wino``), and ``name``.x6@tile, csrc/conv_x6.hip's three-plane layout for column tile
        ``x6_tile`` (the tile is part of the layout, so part of the key).  Returns (U, X6), None where not asked for."""
        eng, key = self.eng, name + '.w'
        U = X6 = None
        if wino:
            U = eng._pack(name + '.U', lambda out: ops.winograd_weight(eng._packed[key], groups, cin_g, out))
        if x6_tile:
            X6 = eng._pack(name + f'.x6@{x6_tile}', lambda out: ops.x6_weight(eng._packed[key], groups, cin_g, taps, x6_tile, out))
        return U, X6

    def _conv_bias(self, name, conv, x, H, Cin, groups=1, *, relu=False, in_xf=None, forms=False, weight=None, rec=()):
        """(grouped) conv + bias in ONE fp32 launch, ``relu`` in its epilogue or left to the reader: every conv without BatchNorm.  ``in_xf`` =
        (scale, shift, pad) of a transform applied on read; ``forms``: also the Winograd / x6 weight forms where the shape wants them;
        ``weight``: the caller's own pack job for ``name``.w (the vanilla conv1_1's channel pad); ``rec``: what the caller's 'convrelu'
        record carries beyond the common keys (the backward reads them)."""
        B = self.B
        k, s, p, dl = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        Cout = conv.out_channels
        cin_g, cout_g = Cin // groups, Cout // groups
        wp = self.eng._pack(name + '.w', weight) if weight else self._packed_conv(name, conv)
        Ho = (H + 2 * p - dl * (k - 1) - 1) // s + 1
        wino = bool(forms and USE_WINOGRAD and ops.winograd_eligible(k, s, p, dl, cin_g, cout_g, groups))
        x6 = forms and USE_CONV_X6 and ops.x6_wanted(k, cin_g, cout_g, groups, B * Ho * Ho, winograd=wino)
        U, X6 = self._weight_forms(name, groups, cin_g, wino, ops.x6_tile(cout_g, groups, B * Ho * Ho) if x6 else 0, k * k)
        out = self._buf(B, Ho, Ho, Cout)
        d, _, _ = ops.make_conv_desc(x, wp, out, B=B, H=H, W=H, in_stride=Cin, cin_g=cin_g, Cout=Cout, groups=groups, k=k,
                                     stride=s, pad=p, dil=dl, bias=conv.bias.detach(), relu=relu, wgt_wino=U, wgt_x6=X6, **ops.xf_kw(in_xf))
        self._add(lib.gssd_conv2d_nhwc_f32, (C.byref(d),), keep=(d, in_xf) if in_xf else d)
        self.rec.append(('convrelu', dict(name=name, conv=conv, x_in=x, out=out, H=H, Cin=Cin, Ho=Ho, Cout=Cout, desc=d, k=k,
                                          stride=s, pad=p, dil=dl, **dict(rec))))
        return out, Ho, Cout

    def _conv_act(self, name, conv, x, H, Cin, groups):
        """(grouped) conv + bias + ReLU in ONE launch (ReLU in the conv epilogue): the batch_norm=False layers."""
        return self._conv_bias(name, conv, x, H, Cin, groups, relu=True, rec=dict(groups=groups))

    def _head(self, i, s, Hs, Cs, in_xf=None):
        """loc[i] / conf[i] (models/...group.py:375-380) as ONE merged 3x3 conv writing straight into the concatenated fp32
        loc [B,8732,4] / conf [B,8732,C] at this source's prior offset.  ``in_xf`` = (scale, shift, pad) of the fuse conv's deferred
        BatchNorm + ReLU when ``s`` is its raw map."""
        eng, net, B, dev, f32 = self.eng, self.eng.net, self.B, self.dev, torch.float32
        off = HEAD_OFF[i]
        A = MBOX[i]
        nloc, nconf = A * 4, A * self.nc
        lw, cw = net.loc[i], net.conf[i]
        cin_pad, K = ops.packed_k(Cs, 3, 3)

        def build_w(out, lw=lw, cw=cw, nloc=nloc, nconf=nconf, K=K):
            if out is None:
                out = torch.empty(nloc + nconf, K, device=dev, dtype=self.adt)
            pk = ops.pack_weight_bf16 if self.bf16 else ops.pack_weight
            pk(lw.weight, out, 0)
            pk(cw.weight, out, nloc)
            return out

        def build_b(out, lw=lw, cw=cw, nloc=nloc):
            if out is None:
                out = torch.empty(nloc + cw.bias.numel(), device=dev, dtype=f32)
            ops.copy_into(out[:nloc], lw.bias)
            ops.copy_into(out[nloc:], cw.bias)
            return out
        wp = eng._pack(f'heads.{i}.w', build_w)
        bp = eng._pack(f'heads.{i}.b', build_b)
        split = (ops.auto_split_k(B * Hs * Hs, nloc + nconf, 1, K, target_blocks=256, max_split=8)
                 if self.bf16 else ops.auto_split_k(B * Hs * Hs, nloc + nconf, 1, K))
        U = None
        if (self.f16_ok and USE_WINOGRAD and USE_HEADS_WINO and nloc % 4 == 0 and nconf % 4 == 0 and B * ((Hs + 1) // 2) ** 2 >= 8192
                and ops.winograd_eligible(3, 1, 1, 1, Cs, nloc + nconf, 1)):
            # train-mode fp32 forward, large map (38 x 38 at batch >= 23): Winograd on fp16 planes with the heads' two-destination epilogue
            # (csrc/conv_wino_x6.hip: 95 us against 173 us for the implicit GEMM and its two reduction slices); one slice
            U, _ = self._weight_forms(f'heads.{i}', 1, Cs, wino=True)
            split = 1
        d, _, _ = ops.make_conv_desc(s, wp, None, B=B, H=Hs, W=Hs, in_stride=Cs, cin_g=Cs, Cout=nloc + nconf, k=3,
                                     pad=1, bias=bp, out_mode=_lib.OUT_HEADS, out_b=None, split_n=nloc,
                                     out_batch_stride=self.P * 4, outb_batch_stride=self.P * self.nc,
                                     out_off=off * 4, outb_off=off * self.nc, split_k=split, wgt_wino=U, **ops.xf_kw(in_xf),
                                     flags=_lib.CONV_OUT_F32 | (self.f16_ok if U is not None else 0))
        self.head_descs.append(d)
        self._add(self.conv_fn, (C.byref(d),), keep=d)
        self.rec.append(('head', dict(i=i, src=s, H=Hs, C=Cs, A=A, off=off, loc=lw, conf=cw, K=K)))

    def _setup_spectral_norm(self, lists):
        """layers/spectral_norm.py:74-89 for every Self_Attn conv of ``lists`` = [(list name, ModuleList)]: ONE launch that
        (training) runs the power iteration in place and writes 1/sigma per output channel (the convs' ``alpha`` vectors)."""
        for lst_name, lst in lists:
            for i, sa in enumerate(lst):
                Cc = sa.in_channels
                a_tpg = self._buf(Cc // 4 + Cc // 2)         # 1/sigma per output channel of the merged theta|phi|g projection
                a_o = self._buf(Cc)
                self.sn_items += [
                    (sa.snconv1x1_theta.weight_orig, sa.snconv1x1_theta.weight_u, sa.snconv1x1_theta.weight_v, a_tpg[:Cc // 8]),
                    (sa.snconv1x1_phi.weight_orig, sa.snconv1x1_phi.weight_u, sa.snconv1x1_phi.weight_v, a_tpg[Cc // 8:Cc // 4]),
                    (sa.snconv1x1_g.weight_orig, sa.snconv1x1_g.weight_u, sa.snconv1x1_g.weight_v, a_tpg[Cc // 4:]),
                    (sa.snconv1x1_attn.weight_orig, sa.snconv1x1_attn.weight_u, sa.snconv1x1_attn.weight_v, a_o),
                ]
                self.sa_state[(lst_name, i)] = (a_tpg, a_o)
        if self.sn_items:
            self.sn_dev = ops.sn_items_tensor([(w.detach(), u, v, s) for (w, u, v, s) in self.sn_items], self.dev)
            # one workgroup per matrix (48 of 256 CUs, ~180 us): on its own stream beside conv1_1 .. conv4_3 inside the graph; the
            # first Self_Attn launch joins it (every later one forks from the trunk after that point)
            with self._on_stream(SN_STREAM):
                self._add(lib.gssd_spectral_norm_f32, (self.sn_dev.data_ptr(), len(self.sn_items), int(self.training), 1e-12))
            self._sn_unjoined = True

    def _packed_conv(self, name, conv):
        eng = self.eng

        def build(out, conv=conv):
            if self.bf16:
                return ops.pack_weight_bf16(conv.weight, out)
            return ops.pack_weight(conv.weight, out)
        return eng._pack(name + '.w', build)

    def _conv_bn(self, name, conv, bn, x, H, Cin, groups, relu=True, pool=None, in_xf=None, defer_bn=False):
        """conv (raw output + fp64 batch sums) -> BN + ReLU (+ max-pool).  ``in_xf`` = (scale, shift, pad) of a producer
        whose BN + ReLU this conv applies on the fly; ``defer_bn`` leaves this layer's own BN + ReLU to its consumer and
        returns (raw, H, C, (scale, shift, pad))."""
        with self._in_layer(name):
            return self._conv_bn_steps(name, conv, bn, x, H, Cin, groups, relu, pool, in_xf, defer_bn)

    def _conv_bn_steps(self, name, conv, bn, x, H, Cin, groups, relu, pool, in_xf, defer_bn):
        B = self.B
        k, s, p, dl = conv.kernel_size[0], conv.stride[0], conv.padding[0], conv.dilation[0]
        Cout = conv.out_channels
        cin_g, cout_g = Cin // groups, Cout // groups
        if defer_bn and cout_g > 512:
            defer_bn = False        # the consumer (same group count) would read more than 512 channels per group: the conv kernels' fused
            #                         input transform keeps at most 512 scale / shift pairs (ungrouped conv6 -> conv7 at groups_vgg = 1)
        wp = self._packed_conv(name, conv)
        Ho = (H + 2 * p - dl * (k - 1) - 1) // s + 1
        wino = bool(not self.bf16 and USE_WINOGRAD and ops.winograd_eligible(k, s, p, dl, cin_g, cout_g, groups))
        x6 = not self.bf16 and USE_CONV_X6 and ops.x6_wanted(k, cin_g, cout_g, groups, B * Ho * Ho, winograd=wino, forward=bool(self.f16_ok))
        U, X6 = self._weight_forms(name, groups, cin_g, wino, ops.x6_tile(cout_g, groups, B * Ho * Ho) if x6 else 0, k * k)
        st = self.eng_stat(bn)
        srep = self.stat_rep.get(id(bn), 0) if self.training else 0
        common = dict(B=B, H=H, W=H, in_stride=Cin, cin_g=cin_g, Cout=Cout, groups=groups, k=k, stride=s, pad=p, dil=dl, bias=conv.bias.detach(),
                      wgt_wino=U, stats=st if self.training else None, stats_rep=srep, **ops.xf_kw(in_xf))
        rec = dict(name=name, conv=conv, bn=bn, x_in=x, in_xf=in_xf, H=H, Cin=Cin, groups=groups, Ho=Ho, Cout=Cout, stats=st, stats_rep=srep,
                   pool=pool, relu=relu, k=k, stride=s, pad=p, dil=dl)
        # Pooled trunk layers of a no-backward forward (conv1_2, conv2_2, conv3_3): max-pooling commutes with the monotone BatchNorm +
        # ReLU, and the direction of monotonicity is the sign of the BatchNorm weight, known before the launch.  The conv's epilogue
        # writes max- (gamma >= 0) or min- (gamma < 0) pooled RAW outputs, a quarter of the map, with the batch sums of the full map;
        # the separate BatchNorm + ReLU + pool pass disappears and the next conv applies the deferred BatchNorm + ReLU to the pooled
        # raw map on read: bit-identical activations (include/gssd_hip.h: GSSD_CONV_POOL2), the full-resolution raw map is never
        # written or re-read (conv1_2 in bf16: 369 MB written + 369 MB re-read + 92 MB written become 92 MB written).
        pooled = (self.nograd and relu and pool is not None and pool[:3] == (2, 2, 0) and (pool[3] or Ho % 2 == 0) and k == 3 and s == 1
                  and p == 1 and dl == 1 and groups == 4 and
                  (wino if not self.bf16 else ((cin_g, cout_g) in ((16, 16), (32, 32)) and Ho % 2 == 0 and Ho * Ho >= 75 * 75)))
        if pooled:
            Hp = ops.pool_out_size(Ho, 2, 2, 0, pool[3])
            raw, pd = self._abuf_tail(Cout, B, Hp, Hp, Cout)
            d, _, _ = ops.make_conv_desc(x, wp, raw, flags=_lib.CONV_POOL2 | self.f16_ok, pool_sign=bn.weight.detach(), **common)
            self._add(self.conv_fn, (C.byref(d),), keep=d)
            xf = self._bn_finalize(st, B * Ho * Ho, bn, Cout, pd, srep)
            self.rec.append(('convbn', dict(rec, raw=raw, desc=d, out=raw, Hp=Hp, xf=xf, pooled=True)))
            return raw, Hp, Cout, xf
        raw, pd = self._abuf_tail(Cout, B, Ho, Ho, Cout) if defer_bn else (self._abuf(B, Ho, Ho, Cout), None)
        # (fp32 mode, train-mode network: forward launches on activation maps may use the x6 kernels' fp16 planes)
        d, _, _ = ops.make_conv_desc(x, wp, raw, wgt_x6=X6, flags=self.f16_ok, **common)
        self._add(self.conv_fn, (C.byref(d),), keep=d)
        rec.update(raw=raw, desc=d)
        self.rec.append(('convbn', rec))
        if defer_bn:
            assert pool is None and relu
            xf = self._bn_finalize(st, B * Ho * Ho, bn, Cout, pd, srep)
            rec.update(out=raw, Hp=Ho, xf=xf)
            return raw, Ho, Cout, xf
        if pool:
            pk, ps, pp, ceil = pool
            Hp = ops.pool_out_size(Ho, pk, ps, pp, ceil)
        else:
            pk, ps, pp, Hp = 0, 1, 0, Ho
        act = self._abuf(B, Hp, Hp, Cout)
        self._add(lib.gssd_bn_relu_pool_bf16 if self.bf16 else lib.gssd_bn_relu_pool_f32,
                  (raw.data_ptr(), act.data_ptr(), B, Ho, Ho, Cout, Hp, Hp, pk, ps, pp, st.data_ptr(), float(B * Ho * Ho),
                   bn.weight.data_ptr(), bn.bias.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
                   float(bn.momentum), float(bn.eps), int(self.training), int(relu), srep), tag=self._pool_tag(Cout, Ho, Hp))
        rec.update(out=act, Hp=Hp, xf=None)
        return act, Hp, Cout, None

    def _bn_finalize(self, st, count, bn, Cout, pd, srep):
        """The launch that turns a layer's batch sums ``st`` (or its running statistics) into the (scale, shift, padding value) vectors its
        consumer applies on read, and updates the running statistics; returns (scale, shift, pad)."""
        sc, sh = self._buf(Cout), self._buf(Cout)
        self._add(lib.gssd_bn_finalize_bf16 if self.bf16 else lib.gssd_bn_finalize_f32,
                  (st.data_ptr(), float(count), bn.weight.data_ptr(), bn.bias.data_ptr(),
                   bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.momentum), float(bn.eps),
                   int(self.training), Cout, sc.data_ptr(), sh.data_ptr(), pd.data_ptr(), srep))
        return sc, sh, pd

    def _pool_tag(self, Cc, H, Hp):
        return ('bn_relu_pool_bf16' if self.bf16 else 'bn_relu_pool', 0.0, (2.0 if self.bf16 else 4.0) * self.B * Cc * (H * H + Hp * Hp))

    def eng_stat(self, bn):
        return self.stat_of[id(bn)]

    def _identity_pool(self, x, out, H, Cc, Hp, k, s, p, relu=False, tag=True):
        """The BatchNorm + ReLU + pool pass with the identity affine (no statistics: scale 1, shift 0): a bare max-pool and / or ReLU."""
        self._add(lib.gssd_bn_relu_pool_bf16 if self.bf16 else lib.gssd_bn_relu_pool_f32,
                  (x.data_ptr(), out.data_ptr(), self.B, H, H, Cc, Hp, Hp, k, s, p, 0, 1.0, 0, 0, 0, 0, 0.1, 1e-5, 0, int(relu), 0),
                  tag=self._pool_tag(Cc, H, Hp) if tag else None)

    def _pool_only(self, x, H, Cc, k, s, p, ceil=False, tag=True):
        Hp = ops.pool_out_size(H, k, s, p, ceil)
        out = self._abuf(self.B, Hp, Hp, Cc)
        self._identity_pool(x, out, H, Cc, Hp, k, s, p, tag=tag)
        self.rec.append(('pool', dict(x_in=x, out=out, H=H, C=Cc, k=k, s=s, p=p, Hp=Hp)))
        return out, Hp

    def _sa_on_x6(self, H, Cc):
        """(projection, o conv): which of a Self_Attn block's two GEMMs the engine hands to csrc/conv_x6.hip -- the ONE statement of the shape rules,
        read by _self_attn and by plan_graph._sa_base_reads_raw."""
        M, C4, C2 = self.B * H * H, Cc // 4, Cc // 2
        on = not self.bf16 and USE_CONV_X6
        return (bool(on and ops.x6_wanted(1, Cc, C4 + C2, 1, M) and C4 % ops.x6_tile(C4 + C2, 1, M) == 0),
                bool(on and ops.x6_wanted(1, C2, Cc, 1, M)))

    def _self_attn(self, lst_name, idx, x, H, Cc, need_out2, want_map=False, cat_groups=0, in_xf=None):
        """layers/self_attn.py:46-89 as three launches: ONE pass over x for the theta | phi | g projections (K9; g written
        transposed), the flash-style core theta^T phi -> softmax -> . g (K10, csrc/flash_attn.hip: the [N, N] map never exists),
        and the o conv with the sigma-gated residual epilogue.  ``want_map`` (visualize=True, op-level tests) additionally
        materialises the attention map with two extra launches; the output path does not read it.  ``cat_groups`` > 0 (with need_out2): the
        caller's only use of the two outputs is slice_and_cat over that many groups; when csrc/conv_x6.hip takes the o conv with the
        grouped destination remap the block writes the concatenation itself and returns (xc [B,H,H,2C], None).  ``in_xf`` = (scale, shift,
        pad): ``x`` is its producer's RAW map (conv4_3, plan_graph._sa_base_reads_raw) and both readers -- the projection and the o conv's
        residual (GSSD_CONV_RESID_XF) -- apply the deferred BatchNorm + ReLU on read; csrc/conv_x6.hip must take both launches."""
        eng, B = self.eng, self.B
        sa = getattr(eng.net, lst_name)[idx]
        a_tpg, a_o = self.sa_state[(lst_name, idx)]
        if self._sn_unjoined:
            self._sn_unjoined, self._pending_wait = False, SN_STREAM          # the next launch added (this block's projection) waits for the 1/sigma vectors
        N = H * H
        Np = ops.round_up(N, 4)
        C8, C2, C4 = Cc // 8, Cc // 2, Cc // 4
        dev, f32 = self.dev, torch.float32
        name = f'{lst_name}.{idx}'

        def build_w(out):
            if out is None:
                out = torch.empty(C4 + C2, Cc, device=dev, dtype=self.adt)
            ops.copy_into(out[:C8], sa.snconv1x1_theta.weight_orig)                     # (rounds to bf16 in bf16 mode)
            ops.copy_into(out[C8:C4], sa.snconv1x1_phi.weight_orig)
            ops.copy_into(out[C4:], sa.snconv1x1_g.weight_orig)
            return out

        def build_wo(out):
            if out is None:
                out = torch.empty(Cc, C2, device=dev, dtype=self.adt)
            ops.copy_into(out, sa.snconv1x1_attn.weight_orig)
            return out

        def build_b(out):
            if out is None:
                out = torch.empty(C4 + C2, device=dev, dtype=f32)
            ops.copy_into(out[:C8], sa.snconv1x1_theta.bias)
            ops.copy_into(out[C8:C4], sa.snconv1x1_phi.bias)
            ops.copy_into(out[C4:], sa.snconv1x1_g.bias)
            return out
        w_tpg = eng._pack(name + '.tpg.w', build_w)
        b_tpg = eng._pack(name + '.tpg.b', build_b)
        # the o conv's weight is already K-major rows; bf16 mode keeps a rounded copy
        w_o = eng._pack(name + '.o.w', build_wo) if self.bf16 else sa.snconv1x1_attn.weight_orig.detach().view(Cc, C2)
        if self.bf16:                          # g^T bf16, rows in the key order of the bf16-value core (csrc/flash_attn.hip)
            Np = ops.round_up(N, 32)
        ag = self._abuf(B, N, C2)
        out = self._abuf(B, H, H, Cc)
        out2 = self._abuf(B, H, H, Cc) if need_out2 else None
        mk = ops.make_conv_desc
        # fp32, N % 4 == 0 (38 x 38): all images as ONE M range -- 361 full row tiles instead of 12 per image with a ragged last one,
        # and the plain-GEMM dispatch (slot stream) instead of the per-image one
        flat = not self.bf16 and N % 4 == 0 and Np == N
        xin = ops.xf_kw(in_xf)
        rxf = _lib.CONV_RESID_XF if in_xf else 0       # the o conv: in_scale / in_shift are its RESIDUAL's (include/gssd_hip.h)
        tpg_on_x6, o_on_x6 = self._sa_on_x6(H, Cc)
        x6_tpg = None
        if tpg_on_x6:
            _, x6_tpg = self._weight_forms(name + '.tpg', 1, Cc, x6_tile=ops.x6_tile(C4 + C2, 1, B * N), taps=1)
        # No backward, fp32, the three-plane core (38 x 38 blocks): the projection's epilogue writes the core's bf16 planes itself where
        # csrc/conv_x6.hip takes the flagged descriptor (GSSD_CONV_OUT_X6PLANES) -- no split pass, and the fp32 theta | phi / g^T arrays do not
        # exist (the record's tp / gT are None).  GSSD_FUSE_SPLIT=0, want_map (its logits GEMM reads the fp32 theta | phi), pooled keys and the
        # opt-in fp16-plane core keep the two-pass entry.
        d1 = ws_planes = tp = gT = None
        if (plan_common.FUSE_SPLIT and self.nograd and not want_map and x6_tpg is not None and flat and C4 % 64 == 0
                and max(H // int(sa.max_pool_factor), 1) == H and USE_FLASH_X6 and N >= 1024 and C8 == 64
                and lib.gssd_self_attn_core_x6_supported(C8, C2) and os.environ.get('GSSD_FLASH_X6_F16', '0') != '1'):
            Np32 = ops.round_up(N, 32)
            ws = torch.zeros(int(lib.gssd_self_attn_core_x6_ws_bytes(B, N, C8, C2)) // 2, device=dev, dtype=torch.int16)   # (the key columns [N, Np32) stay zero)
            dp, _, _ = mk(x, w_tpg, ws, B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C4 + C2, bias=b_tpg, alpha=a_tpg, wgt_x6=x6_tpg,
                          out_mode=_lib.OUT_SPLIT_T, out_b=ws[3 * B * N * C4:], split_n=C4, out_stride=C4, out_b_stride=Np32,
                          in_batch_stride=N * Cc, out_batch_stride=N * C4, outb_batch_stride=C2 * Np32,
                          flags=_lib.CONV_OUT_F32 | self.f16_ok | _lib.CONV_OUT_X6PLANES, **xin)
            if lib.gssd_conv_x6_takes(C.byref(dp)) == 1:
                d1, ws_planes = dp, ws
                self.bufs.append(ws)
        if d1 is None:
            tp = self._buf(B, N, C4)           # theta | phi stay fp32 in both modes: the logits and the softmax are fp32
            gT = self._abuf(B, C2, Np) if self.bf16 else self._buf(B, C2, Np)
            if x6_tpg is not None:
                gT.zero_()                     # csrc/conv_x6.hip never writes the row tails [N, Np) of g^T (conv_igemm zero-fills them)
            d1, _, _ = mk(x, w_tpg, tp, B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C4 + C2, bias=b_tpg, alpha=a_tpg, wgt_x6=x6_tpg,
                          out_mode=_lib.OUT_SPLIT_T, out_b=gT, split_n=C4, out_stride=C4, out_b_stride=Np, m_per_image=not flat,
                          in_batch_stride=N * Cc, out_batch_stride=N * C4, outb_batch_stride=C2 * Np,
                          flags=_lib.CONV_OUT_F32 | (_lib.CONV_OUTB_BF16_PERM32 if self.bf16 else self.f16_ok), **xin)
        x6_o = None
        if o_on_x6:
            def build_x6o(out, bn=ops.x6_tile(Cc, 1, B * N)):
                return ops.x6_weight(sa.snconv1x1_attn.weight_orig.detach().view(Cc, C2), 1, C2, 1, bn, out)
            x6_o = eng._pack(name + f'.o.x6@{ops.x6_tile(Cc, 1, B * N)}', build_x6o)
        d5, _, _ = mk(ag, w_o, out, B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, bias=sa.snconv1x1_attn.bias.detach(),
                      alpha=a_o, gate=sa.sigma.detach(), resid=x, out2=out2, wgt_x6=x6_o, flags=self.f16_ok | rxf, **xin)
        xc = None
        if cat_groups and need_out2 and x6_o is not None and Cc % cat_groups == 0:
            ga = Cc // cat_groups
            xc = self._abuf(B, H, H, 2 * Cc)
            dc, _, _ = mk(ag, w_o, xc, B=B, H=H, W=H, in_stride=C2, cin_g=C2, Cout=Cc, bias=sa.snconv1x1_attn.bias.detach(),
                          alpha=a_o, gate=sa.sigma.detach(), resid=x, out2=xc.view(-1)[ga:], wgt_x6=x6_o, out_stride=2 * Cc, split_n=ga,
                          flags=self.f16_ok | _lib.CONV_OUT_GROUPCAT | rxf, **xin)
            if lib.gssd_conv_x6_takes(C.byref(dc)) == 1:
                d5 = dc
                self.bufs[:] = [t for t in self.bufs if t is not out and t is not out2]      # the separate maps are never written
                v = xc.view(B, H, H, cat_groups, 2, ga)       # the separate outputs, as views (records / debugging)
                out, out2 = v[:, :, :, :, 0], v[:, :, :, :, 1]
            else:
                self.bufs[:] = [t for t in self.bufs if t is not xc]
                xc = None
        fn = self.conv_fn
        if in_xf and (want_map or C4 % 64 != 0 or lib.gssd_conv_x6_takes(C.byref(d1)) != 1 or lib.gssd_conv_x6_takes(C.byref(d5)) != 1):
            raise _lib.GssdError(f'{name}: the block was handed a raw input map, but csrc/conv_x6.hip does not take its projection and o conv')
        if C4 % 64 == 0:
            self._add(fn, (C.byref(d1),), keep=(d1, w_tpg, b_tpg))
        else:
            if self.bf16:
                raise _lib.GssdError('bf16 mode: Self_Attn needs >= 64 theta|phi channels (in_channels >= 256)')
            # narrow blocks (fewer than 64 theta|phi channels: not on the detector's path, op-level tests only): the merged
            # launch's column split needs whole 64-channel tiles, so theta|phi and g go out as two launches over the same weights
            d1a, _, _ = mk(x, w_tpg, tp, B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C4, bias=b_tpg, alpha=a_tpg)
            d1b, _, _ = mk(x, w_tpg[C4:], gT, B=B, H=H, W=H, in_stride=Cc, cin_g=Cc, Cout=C2, bias=b_tpg[C4:], alpha=a_tpg[C4:],
                           out_mode=_lib.OUT_TRANSPOSED, out_stride=Np, m_per_image=True, in_batch_stride=N * Cc,
                           out_batch_stride=C2 * Np)
            self._add(fn, (C.byref(d1a),), keep=(d1a, w_tpg, b_tpg))
            self._add(fn, (C.byref(d1b),), keep=d1b)
        # training keeps the rows' log-sum-exp: the backward rebuilds the probabilities from it in a GEMM epilogue
        lse = self._buf(B, N) if self.training else None
        # max_pool_factor > 1 (layers/self_attn.py:57-59, 67, 76): keys / values average-pooled to a P x P grid before the core
        P = max(H // int(sa.max_pool_factor), 1)
        pooled = P != H
        Nk, Nkp, kp, gTp = N, Np, None, None
        if pooled:
            if self.bf16:
                raise _lib.GssdError('bf16 storage mode is built for max_pool_factor = 1 (BASELINE.json configs[4])')
            Nk, Nkp = P * P, ops.round_up(P * P, 4)
            kp, gTp = self._buf(B, Nk, C8), self._buf(B, C2, Nkp)
            self._add(lib.gssd_sa_pool_kv_f32, (tp.data_ptr(), gT.data_ptr(), kp.data_ptr(), gTp.data_ptr(), B, H, P, C8, C2, Np, Nkp))
            self._add(lib.gssd_self_attn_core_kv_f32, (tp.data_ptr(), kp.data_ptr(), gTp.data_ptr(), ag.data_ptr(), B, N, Nk, Nkp, C8, C2,
                                                       C8, 0, lse.data_ptr() if lse is not None else 0),
                      tag=(f'flash_attn<{C8},{C2}>', 2.0 * B * N * Nk * (C8 + C2), 4.0 * B * (N * C8 + Nk * C8 + C2 * Nkp + N * C2)))
        elif self.bf16:
            self._add(lib.gssd_self_attn_core_bf16v, (tp.data_ptr(), gT.data_ptr(), ag.data_ptr(), B, N, Np, C8, C2,
                                                      lse.data_ptr() if lse is not None else 0),
                      tag=(f'flash_attn_bf16v<{C8},{C2}>', 2.0 * B * N * N * (C8 + C2), B * (4.0 * N * C4 + 2.0 * C2 * Np + 2.0 * N * C2)))
        elif ws_planes is not None:
            self._add(lib.gssd_self_attn_core_x6_planes_f32, (ws_planes.data_ptr(), ag.data_ptr(), B, N, C8, C2,
                                                              lse.data_ptr() if lse is not None else 0),
                      tag=(f'flash_attn_x6<{C8},{C2}>', 2.0 * B * N * N * (C8 + C2), 2.0 * 3 * B * (N * C4 + C2 * Np) + 4.0 * B * N * C2))
        elif USE_FLASH_X6 and N >= 1024 and C8 == 64 and lib.gssd_self_attn_core_x6_supported(C8, C2):
            # both products of the core on the bf16 matrix cores over three-plane operands (csrc/flash_attn_x6.hip): fp32-equivalent results at
            # 6 / 16 of the fp32 instruction's matrix-pipe time; the planes of theta | phi and g^T live in a scratch buffer of the plan
            ws = self._buf(int(lib.gssd_self_attn_core_x6_ws_bytes(B, N, C8, C2)) // 4)
            self._add(lib.gssd_self_attn_core_x6_f32, (tp.data_ptr(), gT.data_ptr(), ag.data_ptr(), B, N, Np, C8, C2, ws.data_ptr(),
                                                       lse.data_ptr() if lse is not None else 0),
                      tag=(f'flash_attn_x6<{C8},{C2}>', 2.0 * B * N * N * (C8 + C2), 4.0 * B * (N * C4 + C2 * Np + N * C2)))
        else:
            self._add(lib.gssd_self_attn_core_kv_f32, (tp.data_ptr(), tp[0, 0, C8:].data_ptr(), gT.data_ptr(), ag.data_ptr(), B, N, N, Np,
                                                       C8, C2, C4, 0, lse.data_ptr() if lse is not None else 0),
                      tag=(f'flash_attn<{C8},{C2}>', 2.0 * B * N * N * (C8 + C2), 4.0 * B * (N * C4 + C2 * Np + N * C2)))
        S = None
        if want_map:
            # attn[b,i,j] = softmax_j(sum_c theta[b,i,c] * phi[b,j,c])   (no 1/sqrt(d) scaling, self_attn.py:71-72)
            S = self._buf(B, N, Nkp)
            keys, krow = (kp, C8) if pooled else (tp[0, 0, C8:], C4)
            d3, _, _ = mk(tp, keys, S, B=B, H=H, W=H, in_stride=C4, cin_g=C8, Cout=Nk, out_stride=Nkp, m_per_image=True,
                          in_batch_stride=N * C4, wgt_batch_stride=Nk * krow, out_batch_stride=N * Nkp, wgt_row_stride=krow)
            self._add(lib.gssd_conv2d_nhwc_f32, (C.byref(d3),), keep=d3)        # fp32 operands in both modes
            self._add(lib.gssd_softmax_rows_f32, (S.data_ptr(), B * N, Nk, Nkp))
        self._add(fn, (C.byref(d5),), keep=d5)
        self.attn_maps[(lst_name, idx)] = (S, Nk, Nkp)
        self.rec.append(('sa', dict(mod=sa, name=name, x_in=x, out=out, out2=out2, H=H, C=Cc, tp=tp, gT=gT, ag=ag, N=N, Np=Np,
                                    inv_sigma=(a_tpg, a_o), P=P, Nk=Nk, Nkp=Nkp, kp=kp, gTp=gTp, lse=lse)))
        if xc is not None:
            return xc, None
        return out, out2

    def _dcn(self, li, x, H, Cin):
        """layers/dcn_v2_custom.py:79-89: offset/mask conv, then ONE fused kernel for the modulated bilinear sampling and the
        9*Cin-deep contraction (csrc/dcn_fused.hip) -- no column buffer."""
        eng, B = self.eng, self.B
        m = eng.net.dcn_list[li]
        if not m.is_engine_geometry():
            raise _lib.GssdError(f'dcn_list.{li}: the engine runs 3x3 / stride 1 / pad 1 / dilation 1 DCN layers only (kernel '
                                 f'{m.kernel_size}, stride {m.stride}, padding {m.padding}, dilation {m.dilation})')
        dg, Cout = m.deformable_groups, m.out_channels
        w_om = self._packed_conv(f'dcn_list.{li}.om', m.conv_offset_mask)

        def build_w(out, m=m, Cin=Cin, dg=dg):
            elems = lib.gssd_dcn_packed_weight_elems_bf16 if self.bf16 else lib.gssd_dcn_packed_weight_elems_x6 if DCN_X6 else lib.gssd_dcn_packed_weight_elems
            pack = lib.gssd_dcn_pack_weight_bf16 if self.bf16 else lib.gssd_dcn_pack_weight_x6 if DCN_X6 else lib.gssd_dcn_pack_weight_f32
            if out is None:
                n = int(elems(m.out_channels, Cin))
                if n <= 0:
                    raise _lib.GssdError(f'deformable conv: unsupported shape Cin {Cin}, Cout {m.out_channels}')
                out = torch.empty(n, device=self.dev, dtype=torch.bfloat16 if (DCN_X6 and not self.bf16) else self.adt)
            _lib.check(pack(m.weight.detach().contiguous().data_ptr(), out.data_ptr(), m.out_channels, Cin, dg,
                            torch.cuda.current_stream().cuda_stream))
            return out
        w_main = eng._pack(f'dcn_list.{li}.wt' + ('.x6' if (DCN_X6 and not self.bf16) else ''), build_w)
        # offsets / mask logits stay fp32 in both modes; rows padded to a multiple of 4 channels (27 * dg is one only for dg = 4, 8, ..):
        # the weight-gradient and data-gradient kernels of the offset conv want 16-byte aligned channel vectors
        # (bf16 mode: a multiple of 8 -- the training step's bf16 data / weight gradients of the offset conv read 16-byte bf16 rows)
        OMC = ops.round_up(27 * dg, 8 if self.bf16 else 4)
        om = self._buf(B, H, H, OMC)
        if OMC != 27 * dg:
            om.zero_()
        out = self._abuf(B, H, H, Cout)
        u_om = None
        if not self.bf16 and USE_WINOGRAD and ops.winograd_eligible(3, 1, 1, 1, Cin, 27 * dg, 1):
            u_om, _ = self._weight_forms(f'dcn_list.{li}.om', 1, Cin, wino=True)
        p_om = None
        if self.f16_ok and USE_PATCH_X6 and lib.gssd_conv_patch_x6_weight_elems(27 * dg, Cin) > 0:
            # train-mode fp32 forward: the patch-staged direct conv on fp16 planes (csrc/conv_patch_x6.hip: 1024 -> 108 channels, 483 -> 398 us)
            def build_p(out, key=f'dcn_list.{li}.om.w', cin=Cin):
                return ops.patch_x6_weight(eng._packed[key], cin, out)
            p_om = eng._pack(f'dcn_list.{li}.om.px6', build_p)
        d1, _, _ = ops.make_conv_desc(x, w_om, om, B=B, H=H, W=H, in_stride=Cin, cin_g=Cin, Cout=27 * dg, k=3, pad=1, out_stride=OMC,
                                      bias=m.conv_offset_mask.bias.detach(), wgt_wino=u_om, wgt_patch=p_om,
                                      flags=_lib.CONV_OUT_F32 | self.f16_ok)
        self._add(self.conv_fn, (C.byref(d1),), keep=d1)
        M = B * H * H
        esz = 2.0 if self.bf16 else 4.0
        self._add(lib.gssd_dcn_forward_bf16 if self.bf16 else lib.gssd_dcn_forward_x6_ex if DCN_X6 else lib.gssd_dcn_forward_f32,
                  (x.data_ptr(), om.data_ptr(), w_main.data_ptr(), m.bias.data_ptr(), out.data_ptr(), B, H, H, Cin, dg, OMC, Cout) +
                  ((self.f16_ok,) if DCN_X6 and not self.bf16 else ()),
                  keep=w_main, tag=('dcn_bf16<128x256>' if self.bf16 else 'dcn_x6<128x256>' if DCN_X6 else 'dcn_fused<128x256>', 2.0 * M * Cout * 9 * Cin,
                                    esz * (M * (Cin + Cout) + Cout * 9 * Cin) + 4.0 * M * 27 * dg))
        if not self.bf16 and not DCN_X6:
            # the stream-K form keeps a flag / slab region per output buffer: released with the plan (engine._PlanBase.__del__)
            self._sk_outs.append(out.data_ptr())
        self.offsets.append((om, H, dg))
        self.rec.append(('dcn', dict(mod=m, x_in=x, out=out, H=H, Cin=Cin, Cout=Cout, om=om, d_om=d1, dg=dg, li=li, omc=OMC)))
        return out, Cout
