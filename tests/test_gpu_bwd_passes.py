"""GPU parity of the streaming backward passes of csrc/backward.hip, one test per row of tests/bwd_pass_cases.py, the C entries called
directly: BatchNorm(train) + ReLU + max-pool backward in the sequences gssd/bwd_ops.py and gssd/ops.py::bn_backward launch (fp32 and mixed
entries), gssd_colsum_f32, gssd_l2norm_bwd_f32, gssd_upsample_insert_f32, gssd_heads_gather_f32.

What a row checks
  - BatchNorm rows: d(raw), d(gamma), d(beta) and the device's fp64 sums array against tests/bwd_pass_ref.py's float64 restatement with the
    decisions (ReLU mask, first maximum of each window) the kernel takes on z = fma(raw, scale, shift) with the scale / shift that
    gssd_bn_finalize_f32 wrote on the device -- asserted equal to the ones the cached reference was built with.  The inputs leave no decision
    to rounding (tests/test_bwd_pass_ref_cpu.py).  Gate: e = max|got - ref64| / max|ref64| <= GATE * e_cpu32 + 1e-7 with e_cpu32 the same
    figure for the restatement in float32 on the CPU; that allowance is itself below test_bn_relu_pool_backward's 2e-4 / 1e-4 on every row
    (asserted in the CPU module).  All sequences of a row are held against the one reference.
  - the column sums of d(raw): against the float64 sum of the kernel's own d(raw) within the summation bound (n_t + ceil(1024 / C4) + 2)
    2^-24 sum|draw[:, c]| (thread chain, LDS adds of a workgroup, conversion), and against 0 -- they vanish analytically -- within that plus
    pixels x the row's allowance x max|draw|.
  - gssd_colsum_f32: |err| <= (n_t + ceil(1024 / C) + 2) 2^-24 sum_rows|x[:, c]| per channel, n_t = ceil(total / gstride).
  - gssd_l2norm_bwd_f32: float64 autograd of the oracle's l2norm, the same gate, 1e-5 as a ceiling.
  - the copy passes and the scale = shift = NULL forms of the reduce pass: bit-exact.
  - guards: every output lies in a larger buffer between sentinels that must come back bit-identical; every input has a NaN guard behind
    its last element; a dz the pass must define completely starts as NaN (no pool, pools whose windows cover the map), one it accumulates
    into or leaves gaps in as zeros (overlapping windows; 'pool floor odd': gssd.ops.pool_leaves_gaps, what every caller asks); scale,
    shift and the coefficients have NaN behind C; the helper's own torch.empty buffer is handed a NaN-filled block of the allocator.

Worst e / e_cpu32 per entry family and output over three MI355X runs of this module (every row prints its own figures; the order of the
fp32 LDS atomics and the fp64 device atomics makes the sums, and with them d(gamma) and d(beta), vary from run to run; draw gave the
same figures every time):
  bn_f32 (reduce_f32 -> finalize -> apply_f32 / apply_masked_f32, and ops.bn_backward)
    draw    2.16   pool ceil odd (e 1.15e-07, e_cpu32 5.32e-08)
    dgamma  4.00   unrolled + tail, plan/no-pool (e 4.17e-07, e_cpu32 1.04e-07; 3.05 in another run)
    dbeta   4.03   pool overlap, helper (e 2.56e-07, e_cpu32 6.37e-08; 2.07 in the plan sequence of the same row and run)
    sums    3.17   unrolled + tail (e 4.52e-07, e_cpu32 1.42e-07; 2.28 in another run)
  bn_mixed (reduce_mixed -> finalize -> apply_mixed, with and without the bf16 hand-over)
    draw    1.49   mixed idle threads bf16        dgamma  2.54   mixed unrolled + tail (1.46 in another run)
    dbeta   3.03   mixed pool overlap (1.89)      sums    3.12   mixed unrolled + tail (1.63 in another run)
  l2norm    dx 1.42 (C 4), dw 0.78 (C 512 dx_add)
  colsum    worst |err| / bound 0.007 (700 x 27 stride 32)
The gate that stands.  GATE = 4 for l2norm.  The BatchNorm passes: 8.06 = twice their worst measured ratio (tests/bwd_pass_ref.py::GATES;
the fp32 and the mixed entries are one family -- the same two kernel templates with the same accumulation -- and the mixed rows' sums moved
by a factor of two between the runs just as the fp32 rows' did).  The 4.03 is d(beta) = s1 of a 70-pixel row whose float32 CPU sum is
within one ulp of float64 (e_cpu32 6.4e-08) while the kernel adds the partial sums of a channel's 341 threads one after the other in LDS
(2.6e-07, four ulp of the largest channel): the ratio is high where e_cpu32 is at its floor, not where e is out of line -- every e of the
module is below 7e-07 (largest: d(beta) of 'mixed unrolled + tail', 6.26e-07 at ratio 2.41 in one run, 3.60e-07 in another; d(gamma) of
'pool grid', 5.85e-07 at ratio 3.57 in one run, 2.71e-07 in another).  gate * e_cpu32 + 1e-7 stays below 3e-06 on every row, against the
2e-4 / 1e-4 of test_bn_relu_pool_backward (asserted in the CPU module).
'pool floor odd' with ops.bn_backward as it stood (a torch.empty routed-gradient buffer): 176 NaN of 560 values of d(raw) -- the 22
pixels of the last row and column of both images.  The plan sequences of the same row, whose buffer the test zeroes by the rule the
callers now share, passed before and after.
test_plan_handlers_zero_what_the_windows_leave_out was written after the fix and has only run with it.
The module takes 5.3 s on an MI355X (44 tests; the slowest, 'pool grid', 1.0 s).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import dev, O          # noqa: E402,F401
import bwd_pass_cases as R             # noqa: E402
import bwd_pass_ref as ref             # noqa: E402

pytestmark = pytest.mark.gpu

SENT = -7.0
GUARD = 256          # elements; a multiple of 16 bytes in every dtype used
NAN = float('nan')
U = 2.0 ** -24


def st():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """An output inside a larger device buffer: [SENT guard | values (prefilled) | back guard (SENT, or NaN for vectors a kernel also reads)]"""

    def __init__(self, shape, dev, dtype=torch.float32, fill=NAN, back=SENT):
        self.n = 1
        for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)):
            self.n *= s
        self.host = torch.full((self.n + 2 * GUARD,), SENT, dtype=dtype)
        self.host[GUARD:GUARD + self.n] = fill.reshape(-1).to(dtype) if torch.is_tensor(fill) else fill
        self.host[GUARD + self.n:] = back
        self.buf = self.host.to(dev)
        self.v = self.buf[GUARD:GUARD + self.n].view(shape)
        self.back_nan = back != back

    def ptr(self):
        return self.v.data_ptr()

    def check(self, what):
        got = self.buf.cpu()
        assert torch.equal(got[:GUARD], self.host[:GUARD]), f'{what}: written in front of the output'
        tail = got[GUARD + self.n:]
        assert bool(torch.isnan(tail).all()) if self.back_nan else torch.equal(tail, self.host[GUARD + self.n:]), f'{what}: written behind the output'
        return got[GUARD:GUARD + self.n].view(self.v.shape)

    def untouched(self, what):
        assert torch.equal(self.check(what).reshape(-1), self.host[GUARD:GUARD + self.n]), f'{what}: values changed'


def inp(t, dev, dtype=None):
    """an input on the device with a NaN guard behind its last element"""
    t = t.to(dtype) if dtype is not None else t
    buf = torch.cat([t.reshape(-1), torch.full((GUARD,), NAN, dtype=t.dtype)]).to(dev)
    return buf[:t.numel()].view(t.shape)


gate_of = ref.gate_of


def dz_fill(kw):
    """what a routed-gradient buffer starts as: zeros where the pass accumulates or leaves gaps, NaN where it must define every element"""
    if kw['pool'] and (kw['pool'][1] < kw['pool'][0] or R.uncovered(kw) > 0):
        return 0.0
    return NAN


class BnSetup:
    """A BatchNorm row on the device: guarded inputs, scale / shift from gssd_bn_finalize_f32, the decisions they imply checked against the
    cached reference's."""

    def __init__(self, row, dev):
        from gssd import _lib
        self.rid, self.kind, self.kw, self.feats = row
        kw = self.kw
        self.o, (mask, idx), self.r64, self.e32 = ref.reference(self.rid, kw)
        o = self.o
        self.B, self.H, self.W, self.C = kw['B'], kw['H'], kw['W'], kw['C']
        self.Ho, self.Wo = R.out_extent(kw)
        self.n = self.B * self.H * self.W
        self.pk, self.ps, self.pp = kw['pool'][:3] if kw['pool'] else (0, 1, 0)
        self.relu = int(kw['relu'])
        self.dev = dev
        self.stats_h = ref.batch_stats(o['raw'])
        self.stats, self.gamma, self.beta = inp(self.stats_h, dev), inp(o['gamma'], dev), inp(o['beta'], dev)
        self.raw, self.dout = inp(o['raw'], dev), inp(o['dout'], dev)
        C = self.C
        self.sc, self.sh = Out(C, dev, back=NAN), Out(C, dev, back=NAN)
        pad, rm, rv = Out(C, dev), Out(C, dev, fill=0.0), Out(C, dev, fill=1.0)
        _lib.check(_lib.lib.gssd_bn_finalize_f32(self.stats.data_ptr(), float(self.n), self.gamma.data_ptr(), self.beta.data_ptr(), rm.ptr(), rv.ptr(),
                                                 0.1, ref.EPS, 2, C, self.sc.ptr(), self.sh.ptr(), pad.ptr(), 0, st()))
        torch.cuda.synchronize()
        sc, sh = self.sc.check('scale'), self.sh.check('shift')
        rm.untouched('running_mean')
        rv.untouched('running_var')
        sc_h, sh_h = ref.finalize_f32(self.stats_h, self.n, o['gamma'], o['beta'])
        if not (torch.equal(sc, sc_h) and torch.equal(sh, sh_h)):          # another rounding of scale / shift: the decisions must still be the same
            m2, i2 = ref.decisions(o['raw'], sc, sh, kw['pool'], kw['relu'])
            assert (mask is None or torch.equal(mask, m2)) and (idx is None or torch.equal(idx, i2)), f'{self.rid}: the device scale / shift decide differently'

    def coefs(self):
        d = self.dev
        return [Out(self.C, d, back=NAN) for _ in range(3)] + [Out(self.C, d), Out(self.C, d)]

    def finalize(self, sums, co):
        from gssd import _lib
        _lib.check(_lib.lib.gssd_bn_bwd_finalize_f32(self.stats.data_ptr(), float(self.n), sums.ptr(), self.gamma.data_ptr(), ref.EPS, self.C,
                                                     co[0].ptr(), co[1].ptr(), co[2].ptr(), co[3].ptr(), co[4].ptr(), 0, st()))

    def inputs_intact(self, raw=None, dout=None):
        raw, dout = self.raw if raw is None else raw, self.dout if dout is None else dout
        assert torch.equal(raw.float().cpu(), self.o['raw']) and torch.equal(dout.float().cpu(), self.o['dout']), f'{self.rid}: an input changed'

    def check(self, seq, family, draw, dg, db, sums, cs, r64=None, e32=None, vanishes=True):
        """draw / dg / db / sums (or None) / cs are CPU tensors; vanishes: the column sums of draw are analytically zero"""
        rid = self.rid
        r64, e32 = r64 or self.r64, e32 or self.e32
        gate = gate_of(family)
        got = dict(draw=draw, dgamma=dg, dbeta=db)
        want = dict(r64)
        if sums is not None:
            got['sums'], want['sums'] = sums, torch.cat([r64['s1'], r64['s2']])
        fig = {}
        for k, v in got.items():
            n_nan = int(torch.isnan(v).sum())
            e = ref.relerr(v, want[k]) if n_nan == 0 else NAN
            fig[k] = (e, e32[k], n_nan)
        print(f'BWD {family} | {rid} | {seq}: ' + '  '.join(f'{k} e {e:.2e} e_cpu32 {b:.2e} ratio {e / max(b, 1e-30):.2f}' + (f' ({n} NaN)' if n else '')
                                                               for k, (e, b, n) in fig.items()))
        for k, (e, b, n_nan) in fig.items():
            assert n_nan == 0, f'{rid} | {seq}: {n_nan} NaN of {got[k].numel()} in {k} -- unwritten routed gradient or a guard was read'
            assert e <= ref.bound(b, gate), (rid, seq, k, e, b)
        if cs is not None:
            C4 = self.C // 4
            n_t = R.bn_grids(self.kw)[1][4]
            absum = draw.double().abs().reshape(-1, self.C).sum(0)
            summ = (n_t + -(-R.WIDE // C4) + 2) * U * absum
            err = (cs.double() - draw.double().reshape(-1, self.C).sum(0)).abs()
            assert bool((err <= summ).all()), (rid, seq, 'colsum vs the sum of draw', float((err / summ.clamp_min(1e-300)).max()))
            zero = summ + self.n * ref.bound(e32['draw'], gate) * float(r64['draw'].abs().max())
            assert not vanishes or bool((cs.double().abs() <= zero).all()), (rid, seq, 'colsum does not vanish', float((cs.double().abs() / zero).max()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward, fp32 entries
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.of_kind('bn'), ids=R.row_id)
def test_bn_backward_sequences(dev, row):
    from gssd import _lib, ops
    lib = _lib.lib
    s = BnSetup(row, dev)
    kw, C, n = s.kw, s.C, s.n
    shape = (s.B, s.H, s.W, C)
    # ---- the sequence gssd/bwd_ops.py::_convbn launches ----
    sums, co, cs = Out(2 * C, dev, torch.float64, fill=0.0), s.coefs(), Out(C, dev, torch.float64, fill=0.0)
    if not kw['pool']:
        seq = 'plan/no-pool'
        draw = Out(shape, dev)
        _lib.check(lib.gssd_bn_bwd_reduce_f32(s.dout.data_ptr(), s.raw.data_ptr(), s.sc.ptr(), s.sh.ptr(), 0, sums.ptr(), s.B, s.H, s.W, C, s.H, s.W,
                                              0, 1, 0, s.relu, st()))
        s.finalize(sums, co)
        _lib.check(lib.gssd_bn_bwd_apply_masked_f32(s.dout.data_ptr(), s.raw.data_ptr(), s.sc.ptr(), s.sh.ptr(), s.relu, co[0].ptr(), co[1].ptr(),
                                                    co[2].ptr(), draw.ptr(), n, C, cs.ptr(), st()))
    else:
        seq = 'plan/pool'
        draw = Out(shape, dev, fill=dz_fill(kw))
        _lib.check(lib.gssd_bn_bwd_reduce_f32(s.dout.data_ptr(), s.raw.data_ptr(), s.sc.ptr(), s.sh.ptr(), draw.ptr(), sums.ptr(), s.B, s.H, s.W, C,
                                              s.Ho, s.Wo, s.pk, s.ps, s.pp, s.relu, st()))
        s.finalize(sums, co)
        _lib.check(lib.gssd_bn_bwd_apply_f32(draw.ptr(), s.raw.data_ptr(), co[0].ptr(), co[1].ptr(), co[2].ptr(), n, C, cs.ptr(), st()))
    assert seq in s.feats
    torch.cuda.synchronize()
    s.inputs_intact()                                       # (plan/no-pool: d(out) comes back bit-identical)
    for c, name in zip(co, ('coef_a', 'coef_b', 'coef_c', 'dgamma', 'dbeta')):
        c.check(f'{s.rid}: {name}')
    s.check(seq, 'bn_f32', draw.check(f'{s.rid}: draw'), co[3].check('dgamma'), co[4].check('dbeta'), sums.check(f'{s.rid}: sums'), cs.check(f'{s.rid}: colsum'))
    # ---- gssd/ops.py::bn_backward: it allocates its routed-gradient buffer itself; the allocator's next block of that size is full of NaN ----
    poison = torch.full(shape, NAN, device=dev)
    del poison
    d2, dg2, db2, cs2 = ops.bn_backward(s.dout, s.raw, s.stats, n, s.gamma, s.sc.v, s.sh.v, kw['pool'][:3] if kw['pool'] else None, bool(s.relu),
                                        want_colsum=True)
    torch.cuda.synchronize()
    s.inputs_intact()
    s.check('helper', 'bn_f32', d2.cpu(), dg2.cpu(), db2.cpu(), None, cs2.cpu())


@pytest.mark.parametrize('row', R.of_kind('noaffine'), ids=R.row_id)
def test_reduce_without_affine_is_exact(dev, row):
    """scale = shift = NULL, sums = NULL: the mask on the stored map (bwd_ops._convrelu), the stand-alone pool (_pool), ReLU + pool (_relupool)."""
    from gssd import _lib
    rid, _, kw, feats = row
    o = ref.make_plain_inputs(rid, kw)
    mask, idx = ref.decide(o['raw'], kw['pool'], kw['relu'])
    want = ref.route(o['dout'], mask, idx, o['raw'].shape)
    raw, dout = inp(o['raw'], dev), inp(o['dout'], dev)
    dz = Out(o['raw'].shape, dev, fill=dz_fill(kw))
    Ho, Wo = R.out_extent(kw)
    pk, ps, pp = kw['pool'][:3] if kw['pool'] else (0, 1, 0)
    _lib.check(_lib.lib.gssd_bn_bwd_reduce_f32(dout.data_ptr(), raw.data_ptr(), 0, 0, dz.ptr(), 0, kw['B'], kw['H'], kw['W'], kw['C'], Ho, Wo, pk, ps, pp,
                                               int(kw['relu']), st()))
    torch.cuda.synchronize()
    got = dz.check(rid)
    assert torch.equal(raw.cpu(), o['raw']) and torch.equal(dout.cpu(), o['dout']), rid
    assert not bool(torch.isnan(got).any()), f'{rid}: {int(torch.isnan(got).sum())} elements left unwritten'
    assert torch.equal(got, want), (rid, int((got != want).sum()))


@pytest.mark.parametrize('kind,relu', [('pool', 0), ('relupool', 1)])
def test_plan_handlers_zero_what_the_windows_leave_out(dev, kind, relu):
    """gssd/bwd_ops.py::_pool / _relupool on a 7 x 7 map under MaxPool2d(2, 2) -- 3 x 3 windows, the last row and column in none.  The
    engine itself only builds the SSD graphs, whose pools cover their maps, so the handlers run here on a stand-in for backward.BackwardPlan
    that keeps its contract (_buf: an uninitialised buffer, zeroed before a run only with zero_each_run) and hands out NaN for
    'uninitialised'.  Bit-exact against the routing of tests/bwd_pass_ref.py."""
    from gssd import _lib
    from gssd.bwd_ops import BackwardOpsMixin

    class Plan(BackwardOpsMixin):
        def __init__(self, B):
            self.B, self.dev, self.steps, self.zero_list, self.gbuf = B, dev, [], [], {}

        def _buf(self, *shape, dtype=torch.float32, zero_each_run=False):
            t = torch.full(shape, NAN, device=dev, dtype=dtype)
            if zero_each_run:
                self.zero_list.append(t)
            return t

        def _add(self, fn, args, keep=None, leaf=None):
            self.steps.append((fn, args))

        def _grad_of(self, t):
            return self.gbuf.get(t.data_ptr())

    kw = R.BN(2, 7, 7, 8, (2, 2, 0, False), relu=bool(relu))
    o = ref.make_plain_inputs(f'handler {kind}', kw)
    x_in, out, dout = inp(o['raw'], dev), torch.empty(2, 3, 3, 8, device=dev), inp(o['dout'], dev)
    plan = Plan(2)
    plan.gbuf[out.data_ptr()] = dout
    r = dict(H=7, C=8, Hp=3, k=2, s=2, p=0, relu=relu, x_in=x_in, out=out)
    (plan._pool if kind == 'pool' else plan._relupool)(r)
    for t in plan.zero_list:
        t.zero_()
    for fn, args in plan.steps:
        _lib.check(fn(*args, st()))
    torch.cuda.synchronize()
    got = plan.gbuf[x_in.data_ptr()].cpu()
    mask, idx = ref.decide(o['raw'], kw['pool'], kw['relu'])
    assert not bool(torch.isnan(got).any()), f'{kind}: {int(torch.isnan(got).sum())} elements of the gradient left unwritten'
    assert torch.equal(got, ref.route(o['dout'], mask, idx, o['raw'].shape))


# ------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm backward, mixed entries (bf16 raw, fp32 or bf16 d(out))
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.of_kind('mixed'), ids=R.row_id)
def test_bn_backward_mixed_sequences(dev, row):
    from gssd import _lib
    lib = _lib.lib
    s = BnSetup(row, dev)
    kw, C, n, o = s.kw, s.C, s.n, s.o
    b16 = int(kw['dout_bf16'])
    shape = (s.B, s.H, s.W, C)
    raw16 = inp(o['raw'], dev, torch.bfloat16)
    d_in = inp(o['dout'], dev, torch.bfloat16) if b16 else s.dout
    geo = (s.B, s.H, s.W, C, s.Ho, s.Wo, s.pk, s.ps, s.pp, s.relu)
    sums, co, cs = Out(2 * C, dev, torch.float64, fill=0.0), s.coefs(), Out(C, dev, torch.float64, fill=0.0)
    dz16 = Out(shape, dev, torch.bfloat16)
    if not kw['pool']:          # sums only; the apply pass re-derives dz from d(out)
        dz = Out(shape, dev)
        _lib.check(lib.gssd_bn_bwd_reduce_mixed(d_in.data_ptr(), b16, raw16.data_ptr(), s.sc.ptr(), s.sh.ptr(), 0, 0, sums.ptr(), *geo, st()))
        s.finalize(sums, co)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(d_in.data_ptr(), b16, dz.ptr(), dz16.ptr(), raw16.data_ptr(), s.sc.ptr(), s.sh.ptr(), s.relu, co[0].ptr(),
                                               co[1].ptr(), co[2].ptr(), n, C, cs.ptr(), 1, st()))
    else:                       # dz routed by the reduce pass in fp32 (what overlapping pools always take)
        dz = Out(shape, dev, fill=dz_fill(kw))
        _lib.check(lib.gssd_bn_bwd_reduce_mixed(d_in.data_ptr(), b16, raw16.data_ptr(), s.sc.ptr(), s.sh.ptr(), dz.ptr(), 0, sums.ptr(), *geo, st()))
        s.finalize(sums, co)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(0, 0, dz.ptr(), dz16.ptr(), raw16.data_ptr(), 0, 0, 0, co[0].ptr(), co[1].ptr(), co[2].ptr(), n, C,
                                               cs.ptr(), 1, st()))
    torch.cuda.synchronize()
    s.inputs_intact(raw16, d_in)
    draw = dz.check(f'{s.rid}: dz')
    s.check('mixed', 'bn_mixed', draw, co[3].check('dgamma'), co[4].check('dbeta'), sums.check('sums'), cs.check('colsum'))
    assert torch.equal(dz16.check(f'{s.rid}: dz16'), draw.to(torch.bfloat16)), f'{s.rid}: dz16 is not the fp32 result rounded once'
    if 'store_f32 = 0' in s.feats:          # only the bf16 map is written
        dz2, dz16b = Out(shape, dev, fill=7.0), Out(shape, dev, torch.bfloat16)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(d_in.data_ptr(), b16, dz2.ptr(), dz16b.ptr(), raw16.data_ptr(), s.sc.ptr(), s.sh.ptr(), s.relu, co[0].ptr(),
                                               co[1].ptr(), co[2].ptr(), n, C, 0, 0, st()))
        torch.cuda.synchronize()
        dz2.untouched(f'{s.rid}: dz with store_f32 = 0')
        assert torch.equal(dz16b.check(f'{s.rid}: dz16, store_f32 = 0'), draw.to(torch.bfloat16)), s.rid
    if 'dz_bf16 hand-over' in s.feats:
        # non-overlapping pool: the routed gradient travels to the apply pass as a bf16 map; the sums are taken before that rounding.  The
        # reference: the same coefficients on the routed gradient rounded to bf16 (no rounding at all when d(out) is bf16 already)
        q = lambda t: t.float().to(torch.bfloat16).to(t.dtype)          # noqa: E731
        mask, idx = ref.decisions(o['raw'], s.sc.v.cpu(), s.sh.v.cpu(), kw['pool'], kw['relu'])
        r32 = ref.bn_backward(o['raw'], o['dout'], o['gamma'], mask, idx, torch.float32)
        h64 = dict(s.r64, draw=s.r64['A'] * q(s.r64['dz']) + s.r64['B'] * o['raw'].double() + s.r64['C'])
        h32 = r32['A'] * q(r32['dz']) + r32['B'] * o['raw'] + r32['C']
        e32 = dict(s.e32, draw=ref.relerr(h32, h64['draw']))
        assert not b16 or torch.equal(h64['draw'], s.r64['draw'])
        dzp = Out(shape, dev, torch.bfloat16, fill=dz_fill(kw))
        sums2, co2, cs2 = Out(2 * C, dev, torch.float64, fill=0.0), s.coefs(), Out(C, dev, torch.float64, fill=0.0)
        dz3, dz163 = Out(shape, dev), Out(shape, dev, torch.bfloat16)
        _lib.check(lib.gssd_bn_bwd_reduce_mixed(d_in.data_ptr(), b16, raw16.data_ptr(), s.sc.ptr(), s.sh.ptr(), 0, dzp.ptr(), sums2.ptr(), *geo, st()))
        s.finalize(sums2, co2)
        _lib.check(lib.gssd_bn_bwd_apply_mixed(dzp.ptr(), 1, dz3.ptr(), dz163.ptr(), raw16.data_ptr(), 0, 0, 0, co2[0].ptr(), co2[1].ptr(), co2[2].ptr(),
                                               n, C, cs2.ptr(), 1, st()))
        torch.cuda.synchronize()
        routed = dzp.check(f'{s.rid}: dz_bf16')
        assert not bool(torch.isnan(routed).any()), f'{s.rid}: the hand-over map has unwritten elements'
        assert torch.equal(routed.float(), q(ref.route(o['dout'], mask, idx, shape))), f'{s.rid}: the hand-over map'
        draw3 = dz3.check(f'{s.rid}: dz after the hand-over')
        # (a fp32 d(out) rounded on the way: the sums were taken before the rounding, so the column sums of draw no longer cancel)
        s.check('mixed hand-over', 'bn_mixed', draw3, co2[3].check('dgamma'), co2[4].check('dbeta'), sums2.check('sums'), cs2.check('colsum'), h64, e32,
                vanishes=bool(b16))
        assert torch.equal(dz163.check(f'{s.rid}: dz16 after the hand-over'), draw3.to(torch.bfloat16)), s.rid


# ------------------------------------------------------------------------------------------------------------------------------------------
# column sums, L2Norm, the copy passes
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('row', R.of_kind('colsum'), ids=R.row_id)
def test_colsum(dev, row):
    from gssd import _lib
    rid, _, kw, _ = row
    rows, C, stride = kw['rows'], kw['C'], kw['stride']
    g = torch.Generator().manual_seed(rows * 4099 + C)
    x = torch.full((rows, stride), NAN)
    x[:, :C] = torch.randn(rows, C, generator=g) + 0.25
    xd = inp(x, dev)
    out = Out(C, dev, torch.float64, fill=0.0)
    _lib.check(_lib.lib.gssd_colsum_f32(xd.data_ptr(), rows, C, stride, out.ptr(), st()))
    torch.cuda.synchronize()
    got = out.check(rid)
    assert not bool(torch.isnan(got).any()), f'{rid}: a pad column or the guard was read'
    _, gstride, _, n_t = R.wide_grid(rows * C, C, R.COLSUM_MAX_WG)
    bound = (n_t + -(-R.WIDE // C) + 2) * U * x[:, :C].double().abs().sum(0)
    err = (got - x[:, :C].double().sum(0)).abs()
    print(f'BWD colsum | {rid}: worst err / bound {float((err / bound).max()):.3f} (n_t {n_t})')
    assert bool((err <= bound).all()), (rid, float((err / bound).max()))


@pytest.mark.parametrize('row', R.of_kind('l2norm'), ids=R.row_id)
def test_l2norm_backward(dev, row):
    from gssd import _lib
    rid, _, kw, _ = row
    B, H, W, C = kw['B'], kw['H'], kw['W'], kw['C']
    g = torch.Generator().manual_seed(B * 1000003 + H * 1009 + C)
    x, dy = torch.randn(B, H, W, C, generator=g), torch.randn(B, H, W, C, generator=g)
    w = torch.rand(C, generator=g) * 10 + 15
    add = torch.randn(B, H, W, C, generator=g) if kw['dx_add'] else None

    def grads(dt):
        xx, ww = x.to(dt).permute(0, 3, 1, 2).contiguous().requires_grad_(), w.to(dt).requires_grad_()
        O.l2norm(xx, ww).backward(dy.to(dt).permute(0, 3, 1, 2))
        dx = xx.grad.permute(0, 2, 3, 1)
        return (dx + add.to(dt) if add is not None else dx), ww.grad
    (dx64, dw64), (dx32, dw32) = grads(torch.float64), grads(torch.float32)
    xd, dyd, wd = inp(x, dev), inp(dy, dev), inp(w, dev)
    addd = inp(add, dev) if add is not None else None
    dx, dw = Out((B, H, W, C), dev), Out(C, dev, torch.float64, fill=0.0)
    _lib.check(_lib.lib.gssd_l2norm_bwd_f32(xd.data_ptr(), wd.data_ptr(), dyd.data_ptr(), dx.ptr(), addd.data_ptr() if add is not None else 0, dw.ptr(),
                                            B * H * W, C, 1e-10, st()))
    torch.cuda.synchronize()
    gate = gate_of('l2norm')
    for name, got, r64, r32 in (('dx', dx.check(rid), dx64, dx32), ('dw', dw.check(rid), dw64, dw32)):
        assert not bool(torch.isnan(got).any()), (rid, name)
        e, e32 = ref.relerr(got, r64), ref.relerr(r32, r64)
        print(f'BWD l2norm | {rid} | {name}: e {e:.2e} e_cpu32 {e32:.2e} ratio {e / max(e32, 1e-30):.2f}')
        assert e <= ref.bound(e32, gate) and e < 1e-5, (rid, name, e, e32)


@pytest.mark.parametrize('row', R.of_kind('upsample'), ids=R.row_id)
def test_upsample_insert(dev, row):
    from gssd import _lib
    rid, _, kw, _ = row
    B, Ho, Wo, s, H, W, C = (kw[k] for k in ('B', 'Ho', 'Wo', 's', 'H', 'W', 'C'))
    dy = torch.randn(B, Ho, Wo, C, generator=torch.Generator().manual_seed(H * 131 + W))
    want = torch.zeros(B, H, W, C)
    want[:, 0:(Ho - 1) * s + 1:s, 0:(Wo - 1) * s + 1:s] = dy
    dyd, u = inp(dy, dev), Out((B, H, W, C), dev)
    _lib.check(_lib.lib.gssd_upsample_insert_f32(dyd.data_ptr(), u.ptr(), B, Ho, Wo, H, W, C, s, st()))
    torch.cuda.synchronize()
    assert torch.equal(u.check(rid), want), rid


@pytest.mark.parametrize('row', R.of_kind('gather'), ids=R.row_id)
def test_heads_gather(dev, row):
    from gssd import _lib
    rid, _, kw, _ = row
    B, HW, A, nc, P, off = (kw[k] for k in ('B', 'HW', 'A', 'nc', 'P', 'off'))
    g = torch.Generator().manual_seed(P + A)
    dloc, dconf = torch.randn(B, P, 4, generator=g), torch.randn(B, P, nc, generator=g)
    want = torch.cat([dloc[:, off:off + HW * A].reshape(B, HW, A * 4), dconf[:, off:off + HW * A].reshape(B, HW, A * nc)], 2)
    dl, dc, out = inp(dloc, dev), inp(dconf, dev), Out((B, HW, A * (4 + nc)), dev)
    _lib.check(_lib.lib.gssd_heads_gather_f32(dl.data_ptr(), dc.data_ptr(), out.ptr(), B, HW, A, nc, P, off, st()))
    torch.cuda.synchronize()
    assert torch.equal(out.check(rid), want), rid
