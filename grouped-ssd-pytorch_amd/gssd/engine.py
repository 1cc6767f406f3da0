"""Forward engine of the GSSD / GSSD++ detector on MI355X.

``GssdEngine`` turns the module tree built by ``build_ssd`` into a flat launch plan: a list of
(C-ABI function, prebuilt argument tuple) pairs over preallocated NHWC buffers.  Running the plan
is a tight loop of ctypes calls on the current HIP stream -- no tensor ops, no allocation (≈2.5 ms of host time per
GSSD step against 6.5 ms on the GPU, scripts/host_overhead.py).

Dataflow restated from models/ssd_multiphase_custom_group.py:217-400:

  x[B,12,300,300] -> pack NHWC(16 ch: 3->4 per phase) -> grouped VGG (conv -> raw + batch stats; BN+ReLU(+pool))
  conv4_3 -> [SA-base0] -> [slice_and_cat] -> [DCN]* -> x ; s = L2Norm(x) -> [SA0] -> fuse_11+BN+ReLU = source0
  pool4 -> conv5_x -> pool5 -> conv6(dil 6) -> conv7 -> [SA-base1] ; -> [SA1] -> fuse_21 = source1
  extras (conv+BN+ReLU)x8, every second one: [SA-base] ; [SA] -> fuse -> source2..5
  heads: one merged (loc|conf) 3x3 conv per source writing straight into loc[B,8732,4] / conf[B,8732,C]

Weights are re-packed (OIHW -> K-major rows) only when a parameter's version counter changed.
"""
import contextlib
import os

import torch

from . import _lib, ops
from ._lib import lib
from .plan_common import (VGG_CFG, EXTRAS_CFG, MBOX, SRC_HW, HEAD_OFF, FUSE_NAMES, USE_CONV_X6, USE_WINOGRAD, DCN_X6, USE_GRAPH, USE_FLASH_X6, USE_BRANCH_STREAMS, SN_STREAM, ALL_STREAMS, Tag, _Step, conv_tag)      # noqa: F401 (re-exported: backward.py, pixellink.py, bench.py)
from .plan_exec import PlanExecMixin
from .plan_graph import PlanGraphMixin
from .plan_ops import PlanOpsMixin, bn_arena


class GssdEngine:
    def __init__(self, net):
        self.net = net
        self._plans = {}
        self._packed = {}        # name -> packed weight tensor
        self._pack_jobs = []     # (callable) refreshers
        self._pack_table = None  # (device table, items, kept tensors, jobs that stay individual launches): see _refresh_packed
        self._versions = None
        self._ptrs = None
        self._param_list = None
        self._ptr_list = None
        self._bn_list = None

    # ------------------------------------------------------------------------------------------
    def _state(self):
        """(version counters of the parameters, storage pointers of every parameter AND buffer).  The launch plans hold raw
        device pointers of all of them (BN gamma / beta / running stats, conv biases, L2Norm weight, spectral-norm u / v,
        sigma, ...): a changed pointer (``p.data = ...``, a replaced head, ``bn.running_mean = ...``) rebuilds the plans, a
        changed version only re-runs the weight pack jobs.  The module tree is walked once (nn.Module traversal costs
        ~0.5 ms per call on this net); a module that gains or loses parameters after the first forward must call
        invalidate()."""
        if self._param_list is None:
            self._param_list = list(self.net.parameters())
            self._ptr_list = self._param_list + list(self.net.buffers())
            self._bn_list = [m for m in self.net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        return tuple([p._version for p in self._param_list]), tuple([t.data_ptr() for t in self._ptr_list])

    def invalidate(self):
        for plans in self._plans.values():
            for pl in plans:
                pl.generation += 1        # a backward still holding one of these plans must not use it
        self._plans.clear()
        self._packed.clear()
        self._pack_jobs = []
        self._pack_table = None
        self._versions = None
        self._ptrs = None
        self._param_list = None
        self._ptr_list = None
        self._bn_list = None

    # ------------------------------------------------------------------------------------------
    MAX_PLANS_IN_FLIGHT = 4

    def forward_plan(self, x, training, events=None, want_maps=False, need_backward=True):
        """Run one forward; returns (loc, conf, plan).  A plan whose last grad-enabled forward still awaits its backward is busy
        (gssd/autograd.py) and is never reused: the call takes (or builds) another instance with its own buffers."""
        net = self.net
        if not x.is_cuda:
            raise _lib.GssdError('GSSD HIP engine: input must live on the MI355X (cuda/ROCm tensor); there is no '
                                 'CPU fallback')
        vers, ptrs = self._state()
        if self._ptrs is not None and ptrs != self._ptrs:
            self.invalidate()              # some parameter / buffer storage moved (.cuda(), p.data = ..., new head ...)
            vers, ptrs = self._state()
        p0 = self._param_list[0]
        if p0.device != x.device:
            raise _lib.GssdError(f'model is on {p0.device}, input on {x.device}')
        B = x.shape[0]
        cin = 3 if getattr(net, 'vanilla', False) else 12
        if tuple(x.shape[1:]) != (cin, 300, 300):
            raise _lib.GssdError(f'expected input [B,{cin},300,300], got {tuple(x.shape)}')
        bn_cfg = tuple((m.momentum, m.eps) for m in self._bn_list)
        # a forward no backward will follow (torch.no_grad(): evaluation, the fwd + loss metric) takes a plan whose pooled trunk layers
        # never write their full-resolution raw maps (GSSD_CONV_POOL2, _Plan._conv_bn); net.pooled_raw = False keeps one plan form
        nograd = (not need_backward) and bool(getattr(net, 'pooled_raw', True))
        key = (B, bool(training), x.device.index, hash(bn_cfg), bool(want_maps), getattr(net, 'compute_dtype', 'f32'), nograd)
        plans = self._plans.setdefault(key, [])
        plan = next((pl for pl in plans if not pl.busy), None)
        if plan is None:
            if len(plans) >= self.MAX_PLANS_IN_FLIGHT:
                raise _lib.GssdError(f'{len(plans)} forwards of batch {B} are still waiting for their backward; free their '
                                     f'outputs (or call backward) before running more')
            plan = self._build(B, bool(training), x.device, bool(want_maps), nograd)
            plans.append(plan)
            vers, ptrs = self._state()
        self._ptrs = ptrs
        if vers != self._versions:
            self._refresh_packed(x.device)
            self._versions = vers
        self._last_plan = plan
        loc, conf = plan.run(x, events)
        return loc, conf, plan

    def forward(self, x, training, events=None, want_maps=False):
        loc, conf, _ = self.forward_plan(x, training, events, want_maps, need_backward=False)
        return loc, conf

    # ------------------------------------------------------------------------------------------
    def _pack(self, name, build):
        """Register a packed weight: ``build(out_or_None) -> tensor`` fills/refreshes it in place.  The cache is per storage mode
        (a module switched between fp32 and bf16 keeps both sets of packed weights)."""
        if getattr(self.net, 'compute_dtype', 'f32') == 'bf16':
            name = name + '@bf16'
        if name not in self._packed:
            t = build(None)
            self._packed[name] = t
            self._pack_jobs.append(lambda: build(self._packed[name]))
            self._pack_table = None
        return self._packed[name]

    def _refresh_packed(self, dev):
        """Re-derive every packed weight from the (changed) parameters.  Jobs made only of ops.pack_weight / ops.copy_into from the
        parameters' own storage are recorded ONCE into a device table and from then on refreshed by a single launch
        (gssd_pack_conv_weights_batched: ~130 launches of 5-8 us after every optimizer step otherwise); the rest -- Winograd
        transforms of packed weights, the DCN layout, bf16 rounding -- run after it, in registration order."""
        if self._pack_table is None:
            rec, rest = ops.PackRecorder(), []
            for job in self._pack_jobs:
                n0, k0 = len(rec.items), len(rec.keep)
                ops.recorder = rec
                try:
                    job()
                except ops.PackRecorder.Unstable:
                    del rec.items[n0:], rec.keep[k0:]
                    rest.append(job)
                finally:
                    ops.recorder = None
                if len(rec.items) == n0 and job not in rest:
                    rest.append(job)               # recorded nothing: a job of other launches only
            table = ops.pack_table(rec, dev) if rec.items else None
            self._pack_table = (table, len(rec.items), rec.keep, rest)
        table, n, _, rest = self._pack_table
        if n:
            ops.run_pack_table(table, n)
        for job in rest:
            job()

    def _build(self, B, training, dev, want_maps=False, nograd=False):
        drain_sk_releases()
        if getattr(self.net, 'vanilla', False):
            return _PlanVanilla(self, B, training, dev)
        return _Plan(self, B, training, dev, want_maps, nograd)


_SK_PENDING = []          # (device index, output pointer) of dropped plans whose stream-K regions await their release


def drain_sk_releases():
    """Free the stream-K regions queued by _PlanBase.__del__: only when no stream of this thread is capturing, each on its own device."""
    if not _SK_PENDING or torch.cuda.is_current_stream_capturing():
        return 0
    n = 0
    while _SK_PENDING:
        di, ptr = _SK_PENDING.pop()
        with torch.cuda.device(di):
            n += max(0, int(lib.gssd_dcn_streamk_release(ptr)))
    return n


class _RecList(list):
    """The forward graph records; append() notes which branch (stream id of the launch plan, 0 = trunk) the record belongs to."""

    def __init__(self, plan):
        super().__init__()
        self._plan = plan

    def append(self, item):
        item[1].setdefault('sid', self._plan._sid)
        super().append(item)


class _PlanBase(PlanGraphMixin, PlanOpsMixin, PlanExecMixin):
    """What every forward launch plan is made of: the state the emitters (plan_ops.PlanOpsMixin), the step placement and head helpers
    (plan_graph.PlanGraphMixin) and eager / hipGraph execution (plan_exec.PlanExecMixin) read, all of it set by ONE constructor, plus the
    step / buffer helpers.  A subclass calls the constructor, then emits its own graph."""
    generation = 0        # bumped by every run(): a backward checks it ran against the forward that produced it
    busy = False          # a grad-enabled forward awaits its backward (gssd/autograd.py::_Lease)
    _bwd = None

    def __init__(self, eng, B, training, dev, *, bf16=False, nograd=False, want_maps=False):
        self.eng, self.B, self.training, self.dev = eng, B, bool(training), dev
        self.nograd = nograd                       # no backward will read this plan's activations
        self.want_maps = want_maps                 # visualize=True: also materialise the attention maps
        # BASELINE.json configs[4]: bf16 NHWC activations + bf16 packed weights + bf16 MFMA, fp32 accumulation / BatchNorm
        # statistics / softmax / offsets / loc + conf / loss / NMS (net.compute_dtype = 'bf16'; parameters stay fp32 masters)
        self.bf16 = bf16
        self.adt = torch.bfloat16 if bf16 else torch.float32
        self.conv_fn = lib.gssd_conv2d_nhwc_bf16 if bf16 else lib.gssd_conv2d_nhwc_f32
        self.cpad = 8 if bf16 else 4               # stored channels per group of the packed input: whole 16-byte pieces
        self.steps, self.bufs, self.head_descs = [], [], []
        self.rec = _RecList(self)   # forward graph records, consumed by gssd/backward.py (each tagged with its branch stream id)
        self.P, self.nc = 0, 0      # prior boxes, classes (the detector plans)
        # emitter state: the stream id / layer the next launches belong to, a join the next launch carries, the spectral-norm launch's open join
        self._sid, self._layer, self._pending_wait, self._sn_unjoined = 0, None, None, False
        self.sn_items, self.sa_state, self.attn_maps, self.offsets = [], {}, {}, []
        self.sources, self.sources_xf = [], {}
        self._sk_outs = []          # deformable-conv outputs with a stream-K region (GSSD_DCN_X6=0), released with the plan
        self._mark_conv7 = self._pack_step = self._in_desc = None
        self._reduce_steps = ()
        self.stats, self.stat_of, self.stat_rep, self.nbt = bn_arena(dev, (), ())
        # execution state (plan_exec)
        self._runs, self._side_streams, self._node_events = 0, {}, {}
        self._graphs = self._last_in_ptr = self._gx = None          # (_graphs: None until the first capture, then {key: segments})

    def __del__(self):
        # csrc/dcn_fused.hip's stream-K regions belong to this plan's deformable-conv outputs (GSSD_DCN_X6=0 only).  The release frees device
        # memory (it synchronises) and the collector may drop a plan at any time -- inside another plan's open hipGraph capture, or with another
        # device current -- so the pointers are only QUEUED here, with their device; drain_sk_releases() frees them at the next plan build
        # that finds no capture open.
        try:
            outs = self.__dict__.get('_sk_outs', ())          # (guarded: the constructor may have raised)
            if outs:
                _SK_PENDING.extend((self.dev.index if self.dev.index is not None else torch.cuda.current_device(), ptr) for ptr in outs)
        except Exception:        # noqa: BLE001 -- interpreter teardown
            pass

    def backward_plan(self):
        if self.nograd:
            raise _lib.GssdError('this forward plan was built for a forward without backward (its pooled layers kept no raw maps)')
        if self._bwd is None:
            from .backward import BackwardPlan, Bf16Shadow
            # bf16 storage mode: the fp32 backward plan over fp32 copies of the stored bf16 activations (mixed precision)
            self._bwd = BackwardPlan(Bf16Shadow(self) if self.bf16 else self)
        return self._bwd

    # ------------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def _on_stream(self, sid):
        """The launches and records emitted inside belong to stream ``sid`` of the captured graph."""
        prev, self._sid = self._sid, sid
        try:
            yield
        finally:
            self._sid = prev

    @contextlib.contextmanager
    def _in_layer(self, name):
        """The launches emitted inside belong to layer ``name`` (Tag.layer: bench.py sums a layer's launches)."""
        prev, self._layer = self._layer, name
        try:
            yield
        finally:
            self._layer = prev

    def _add(self, fn, args, keep=None, tag=None):
        d = None
        if tag is None and fn in (lib.gssd_conv2d_nhwc_f32, lib.gssd_conv2d_nhwc_bf16):
            d = keep[0] if isinstance(keep, tuple) else keep
            tag = (None, 0.0, 0.0)                   # a conv: named by _name_convs() once the plan's descriptors are final
        if tag is not None:
            tag = Tag(tag)
            tag.layer = self._layer
            tag.desc = d
        self.steps.append(_Step(fn, args, keep, tag, self._sid, self._pending_wait))
        self._pending_wait = None

    def _name_convs(self):
        """Last step of a plan build: every conv step gets its (kernel instance, FLOPs, bytes) from the library's dispatcher
        (plan_common.conv_tag), now that the heads have their outputs and conv1_1 its final input form.  A descriptor the
        entry point would refuse raises GssdError here, not at the first launch."""
        for st in self.steps:
            if st.tag is not None and st.tag[0] is None:
                tag = Tag(conv_tag(st.tag.desc, bf16=st.fn is lib.gssd_conv2d_nhwc_bf16))
                tag.layer, tag.desc = st.tag.layer, st.tag.desc
                st.tag = tag

    def _abuf(self, *shape):
        """Activation buffer in the plan's storage type (fp32, or bf16 in configs[4] mode)."""
        t = torch.empty(*shape, device=self.dev, dtype=self.adt)
        self.bufs.append(t)
        return t

    def _buf(self, *shape):
        t = torch.empty(*shape, device=self.dev, dtype=torch.float32)
        self.bufs.append(t)
        return t

    def _abuf_tail(self, tail, *shape):
        """Activation buffer with ``tail`` more elements stored right behind it (one allocation): a raw conv output whose deferred
        BatchNorm's padding vector sits at ``map + numel`` -- the fp32 Winograd kernel then fetches the padding value of an out-of-image
        patch position through the load ADDRESS (32-bit offset from the map) instead of selecting it per loaded element
        (include/gssd_hip.h: in_pad).  Returns (map, tail view)."""
        if self.bf16:
            return self._abuf(*shape), self._abuf(tail)          # (only the fp32 Winograd kernel uses the layout)
        n = 1
        for v in shape:
            n *= v
        flat = torch.empty(n + tail, device=self.dev, dtype=self.adt)
        self.bufs.append(flat)
        return flat[:n].view(*shape), flat[n:]


class _Plan(_PlanBase):
    """The launch plan of one (batch size, mode) of the grouped detector: the walk over its graph (plan_graph.PlanGraphMixin)."""

    def __init__(self, eng, B, training, dev, want_maps=False, nograd=False):
        net = eng.net
        super().__init__(eng, B, training, dev, bf16=getattr(net, 'compute_dtype', 'f32') == 'bf16', nograd=nograd, want_maps=want_maps)
        g = net.groups_vgg
        # channels per group of the packed input: 12 / groups_vgg real ones (3 per CT phase at the default 4 groups), zero-padded to whole
        # 16-byte pieces (fp32: 4 channels, bf16: 8)
        self.cpad = ops.round_up(12 // g, self.cpad)
        self.P, self.nc = 8732, net.num_classes
        # The trunk's batch sums are kept in R replicas (include/gssd_hip.h: gssd_conv_desc::stats_rep): device-scope fp64 atomics on one
        # cache line are served serially, and the persistent trunk kernels flush every workgroup's sums at the END of the launch (conv2_1
        # in bf16: 131 k atomics on 16 lines = 60 of its 140 us, profiles/r04_thin_knockout_before.txt).  R * C <= 2048 (at most 32): every
        # trunk layer spreads its sums over 256 lines; the consumers add the replicas up in a fixed order.
        # bf16 storage mode only: the fp32 trunk kernels are compute-bound, their workgroups finish spread out and the tail is not
        # there to remove (scripts/thin_f32_probe.py: conv1_1 248 us with one array, 260 with 32 replicas, 224 without batch sums)
        trunk_bn = ({id(m) for m in net.vgg if isinstance(m, torch.nn.BatchNorm2d)}
                    if (self.bf16 and os.environ.get('GSSD_STATS_REP', '1') != '0') else set())
        self.stats, self.stat_of, self.stat_rep, self.nbt = bn_arena(dev, net.modules(), trunk_bn)
        self._setup_spectral_norm([(n, getattr(net, n)) for n in ('self_attn_base_list', 'self_attn_list')
                                   if getattr(net, n, None) is not None])

        # ---- input pack ------------------------------------------------------------------------------
        x16 = self._abuf(B, 300, 300, self.cpad * g)
        self._pack_step = len(self.steps)
        if self.bf16:
            self._add(lib.gssd_pack_input_nhwc_bf16, [0, x16.data_ptr(), B, 12, 300, 300, g])
        else:
            self._add(lib.gssd_pack_input_nhwc, [0, x16.data_ptr(), B, 12, 300, 300, g, self.cpad])

        if not net.batch_norm:
            if self.bf16:
                raise _lib.GssdError('bf16 storage mode is built for the batch_norm=True graph (BASELINE.json configs[4])')
            self._build_plain_graph(x16)
        else:
            self._build_bn_graph(x16)
        assert len(self.head_descs) == 6
        self._finish_heads()
        self._place_sn_step()
        self._place_branch0()
        self._fuse_input_pack()
        self._name_convs()


class _PlanVanilla(_PlanBase):
    """models/ssd.py:48-108: dense VGG-SSD300 without BatchNorm (BASELINE.json configs[0]).  conv + ReLU is one launch
    (ReLU in the conv epilogue); pools are the identity-affine pool pass."""

    def __init__(self, eng, B, training, dev):
        super().__init__(eng, B, training, dev)
        net = eng.net
        self.P, self.nc = 8732, net.num_classes
        x4 = self._buf(B, 300, 300, 4)
        self._pack_step = 0
        self._add(lib.gssd_pack_input_nhwc, [0, x4.data_ptr(), B, 3, 300, 300, 1, 4])
        cur, H, Cc = x4, 300, 4
        sources = []
        mods = list(net.vgg)
        i = 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, torch.nn.Conv2d):
                cur, H, Cc = self._conv_relu(f'vgg.{i}', m, cur, H, Cc)
                i += 2                                   # conv + ReLU
                if i - 2 == 21:                          # conv4_3 (+ReLU at 22): L2Norm source (ssd.py:73-77)
                    s = self._buf(B, H, H, Cc)
                    self._add(lib.gssd_l2norm_f32, (cur.data_ptr(), net.L2Norm.weight.data_ptr(), s.data_ptr(), B * H * H, Cc,
                                                    float(net.L2Norm.eps)))
                    self.rec.append(('l2norm', dict(x_in=cur, out=s, H=H, C=Cc, mod=net.L2Norm)))
                    sources.append((s, H, Cc))
            else:                                        # MaxPool2d
                cur, H = self._pool_only(cur, H, Cc, m.kernel_size, m.stride, m.padding, m.ceil_mode, tag=False)
                i += 1
        sources.append((cur, H, Cc))                     # conv7
        for k, m in enumerate(net.extras):
            cur, H, Cc = self._conv_relu(f'extras.{k}', m, cur, H, Cc)
            if k % 2 == 1:
                sources.append((cur, H, Cc))
        self.sources = sources
        for i, (s, Hs, Cs) in enumerate(sources):
            self._head(i, s, Hs, Cs)
        self._finish_heads()
        self._name_convs()

    def _conv_relu(self, name, conv, x, H, Cin):
        def build(out, conv=conv, Cin=Cin):
            w = conv.weight
            if w.shape[1] != Cin:                        # conv1_1: 3 input channels stored in 4 (zero pad)
                w = torch.nn.functional.pad(w.detach(), (0, 0, 0, 0, 0, Cin - w.shape[1]))
            return ops.pack_weight(w, out)
        return self._conv_bias(name, conv, x, H, Cin, relu=True, weight=build)


class SelfAttnOp(_PlanBase):
    """ONE Self_Attn block (layers/self_attn.py:46-89) as its own launch plan -- the op-level entry the parity tests use:
    x NHWC [B,H,H,C] -> (x + sigma*o, sigma*o, attention map [B,N,N]).  ``training`` runs the spectral-norm power iteration
    first (and mutates weight_u / weight_v in place), like the reference's forward pre-hook."""

    def __init__(self, sa, B, H, training, dev):
        holder = torch.nn.Module()
        holder.self_attn_list = torch.nn.ModuleList([sa])
        super().__init__(GssdEngine(holder), B, training, dev)
        Cc = sa.in_channels
        self.H, self.C = H, Cc
        self.x = self._buf(B, H, H, Cc)
        self._setup_spectral_norm([('self_attn_list', holder.self_attn_list)])
        self.out, self.out2 = self._self_attn('self_attn_list', 0, self.x, H, Cc, need_out2=True, want_map=True)
        self._name_convs()

    def run(self, x_nhwc):
        self.generation += 1
        self.x.copy_(x_nhwc)
        self._run_steps(torch.cuda.current_stream().cuda_stream)
        S, N, Np = self.attn_maps[('self_attn_list', 0)]
        return self.out, self.out2, S[:, :, :N]
