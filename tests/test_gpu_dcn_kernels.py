"""GPU parity of the engine's deformable-conv kernels, one test per (row of tests/dcn_kernel_cases.py, entry form the launcher accepts it
for), the C entries called directly: gssd_dcn_im2col_f32 / _bf16, gssd_dcn_forward_f32, gssd_dcn_forward_x6_ex with flags 0 and with
GSSD_CONV_F16_OK, gssd_dcn_forward_bf16, gssd_dcn_col2im_f32.  One further test re-runs the 'exact' x6 tests in a child process with
GSSD_DCN_X6_SPLITK=0, so the one-part form also sees dg 2 and dg 4.

What a row checks
  - 'exact' rows: the result is bit-identical to the reference of tests/dcn_kernel_ref.py rounded once to the output type (fp32; bf16 for
    the two bf16 entries).  No tolerance: the inputs make every product and partial sum exact in every precision and summation order
    (proved on the CPU in tests/test_dcn_kernel_cases_cpu.py).  col2im: d(x) starts as a dyadic non-zero preload and comes back as
    preload + gradient exactly (the entry ADDS); d(om) starts at zero.
  - 'random' rows: e = max|got - ref64| / max|ref64| per quantity under the project's ceilings, never raised -- TOL = 1e-4 for dcn_fused,
    im2col f32 and col2im; e < 2e-6 + 2 e_fused and rel(x6, fused) < 1e-5 for x6 (test_dcn_x6_matches_fused); 3 BF_ULP max and BF_ULP l2
    against the col_round reference for the bf16 entries (test_dcn_bf16) -- and, below the ceiling, under the gate
    e <= G * e_cpu32 + 1e-7 (tests/dcn_kernel_ref.py::GATES) with e_cpu32 the same figure for the reference in float32 on the CPU.
  - 'im2col second item': the launch whose first waves take a second item against the same entry run image by image, bit for bit.
  - guards: every output lies in a larger buffer between sentinels that must come back bit-identical (the Cout tail, the last ragged row
    tile); every input has a NaN block behind its last element; out / cols start as NaN (the entries define them completely); the padding
    columns of om hold NaN and those of d(om) stay zero; the inputs come back unchanged.
  - eligibility: an entry returns GSSD_OK for every row dcn_kernel_cases.eligible accepts (each test) and the argument error, with nothing
    written, for the row it refuses (test_refused_row_writes_nothing).

Worst e / e_cpu32 per entry family over three MI355X runs of this module (every random row prints its own figures; the forward entries and
im2col gave the same figures every time, the atomics of col2im moved d(x) of 'overflow only' between 1.15 and 1.26 and d(om) of 'wide
groups' between 0.61 and 0.70):
  fused    out   6.63  wide groups (e 2.07e-06, e_cpu32 3.12e-07; K = 9216 products per output on the fp32 MFMA); 4.45 window only, 3.75 three
                       chunks, 2.87 mixed, 1.47 overflow only
  x6       out   3.06  wide groups, bf16 planes (e 9.52e-07, e_cpu32 3.12e-07; fp16 planes 1.97); 2.70 three chunks (fp16 planes 2.45)
  im2col   cols  1.23  mixed (e 1.46e-07, e_cpu32 1.18e-07)
  col2im   dx    1.26  overflow only (e 3.30e-07, e_cpu32 2.61e-07)          dom   0.90  overflow only (e 1.44e-07, e_cpu32 1.60e-07)
  bf16 entries (no gate, see below)   forward: max 0.80 BF_ULP, l2 0.44 BF_ULP;  im2col bf16: max 0.09 BF_ULP
The gates that stand (tests/dcn_kernel_ref.py::GATES), twice the worst ratio: fused 13.26, x6 6.12, im2col 2.46, col2im 2.52.  Each sits
below its ceiling on every row: G * e_cpu32 + 1e-7 is at most 4.3e-06 for dcn_fused, 1.4e-06 for col2im and 4.7e-07 for im2col against
TOL = 1e-4, and at most 2.1e-06 for x6 against 2e-6 + 2 e_fused = 6.1e-06 on the same row.  The bf16 entries keep their ceilings alone: their
error is the rounding of the bf16 columns and of the bf16 output (1e-3 of the output scale), four orders above e_cpu32, so a multiple of
e_cpu32 says nothing about them.
No row was red: every 'exact' check was bit-exact on the first run, in the two-part and in the one-part form of x6, and no kernel was changed.
The module takes 8.5 s on an MI355X (107 tests; the slowest, the child process of test_one_part_per_tile_on_the_exact_rows, 4.8 s; the
slowest row, 'im2col second item', 0.3 s).
"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import dev, TOL                            # noqa: E402,F401
from test_gpu_bwd_passes import Out, inp, st, NAN          # noqa: E402
import dcn_kernel_cases as R                               # noqa: E402
import dcn_kernel_ref as ref                               # noqa: E402

pytestmark = pytest.mark.gpu

BF_ULP = ref.BF_ULP
_fused = {}          # row id -> dcn_fused's output on the row (host): what the x6 forms are also held against


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def cols_layout(t):
    """[B, C, 9, H, W] -> the kernels' [pixel][tap][C]"""
    B, C, _, H, W = t.shape
    return t.permute(0, 3, 4, 2, 1).reshape(B * H * W, 9 * C).contiguous()


def om_layout(om, kw, fill=NAN):
    """[B, 27 dg, H, W] -> NHWC rows of om_stride floats, the padding columns filled"""
    B, H, W = kw['B'], kw['H'], kw['W']
    t = torch.full((B, H, W, kw['om_stride']), fill, dtype=om.dtype)
    t[..., :27 * kw['dg']] = nhwc(om)
    return t


class Inputs:
    """A row's operands on the device, every one with a NaN block behind its last element"""

    def __init__(self, row, dev, bf16=False):
        self.row, self.kw, self.bf16 = row, row[2], bf16
        o = self.o = ref.make_inputs(row)
        self.x_h = nhwc(ref.q16(o['x']) if bf16 else o['x'])
        self.om_h = om_layout(o['om'], self.kw)
        self.x = inp(self.x_h, dev, torch.bfloat16 if bf16 else None)
        self.om = inp(self.om_h, dev)
        self.bias = inp(o['bias'], dev) if o['bias'] is not None else None
        self.w = ref.q16(o['w']) if bf16 else o['w']

    def geo(self):
        kw = self.kw
        return kw['B'], kw['H'], kw['W'], kw['C'], kw['dg'], kw['om_stride']

    def intact(self):
        n = 27 * self.kw['dg']
        assert torch.equal(self.x.float().cpu(), self.x_h), f'{self.row[0]}: x changed'
        om = self.om.cpu()
        assert torch.equal(om[..., :n], self.om_h[..., :n]) and bool(torch.isnan(om[..., n:]).all()), f'{self.row[0]}: om changed'


def packed_weight(entry, w, kw, dev):
    """the entry's packed weights (a 16-byte dummy for a shape its packer refuses: the forward entry has to refuse it too)"""
    from gssd import _lib
    lib = _lib.lib
    Cout, C, dg = kw['Cout'], kw['C'], kw['dg']
    elems, pack, dt = {'fused': (lib.gssd_dcn_packed_weight_elems, lib.gssd_dcn_pack_weight_f32, torch.float32),
                       'bf16': (lib.gssd_dcn_packed_weight_elems_bf16, lib.gssd_dcn_pack_weight_bf16, torch.bfloat16)}.get(
                           entry, (lib.gssd_dcn_packed_weight_elems_x6, lib.gssd_dcn_pack_weight_x6, torch.bfloat16))
    n = int(elems(Cout, C))
    if n <= 0 or not R.eligible(entry, kw):
        return torch.zeros(64, device=dev, dtype=dt)
    wp = torch.empty(n, device=dev, dtype=dt)
    wd = inp(w, dev)
    _lib.check(pack(wd.data_ptr(), wp.data_ptr(), Cout, C, dg, st()))
    return wp


def run_forward(entry, s, dev, fill=NAN):
    """(rc, out) of a forward entry on the inputs s"""
    from gssd import _lib
    lib = _lib.lib
    kw = s.kw
    wp = packed_weight(entry, s.w, kw, dev)
    out = Out((kw['B'], kw['H'], kw['W'], kw['Cout']), dev, torch.bfloat16 if entry == 'bf16' else torch.float32, fill=fill)
    b = s.bias.data_ptr() if s.bias is not None else 0
    args = (s.x.data_ptr(), s.om.data_ptr(), wp.data_ptr(), b, out.ptr(), *s.geo(), kw['Cout'])
    if entry in ('x6', 'x6_f16'):
        rc = lib.gssd_dcn_forward_x6_ex(*args, _lib.CONV_F16_OK if entry == 'x6_f16' else 0, st())
    else:
        rc = getattr(lib, R.SYMBOL[entry])(*args, st())
    torch.cuda.synchronize()
    return rc, out


def run_im2col(entry, s, dev, fill=NAN, images=None):
    from gssd import _lib
    kw = s.kw
    B, H, W, C, dg, stride = s.geo()
    x, om = (s.x, s.om) if images is None else (s.x[images:images + 1], s.om[images:images + 1])
    nb = B if images is None else 1
    cols = Out((nb * H * W, 9 * C), dev, torch.bfloat16 if entry == 'im2col_bf16' else torch.float32, fill=fill)
    rc = getattr(_lib.lib, R.SYMBOL[entry])(x.data_ptr(), om.data_ptr(), cols.ptr(), nb, H, W, C, dg, stride, st())
    torch.cuda.synchronize()
    return rc, cols


def run_col2im(s, dev, preload):
    from gssd import _lib
    kw = s.kw
    dcols = inp(cols_layout(s.o['dcols']), dev)
    dx = Out(s.x_h.shape, dev, fill=preload)
    dom = Out(s.om_h.shape, dev, fill=0.0)
    rc = _lib.lib.gssd_dcn_col2im_f32(s.x.data_ptr(), s.om.data_ptr(), dcols.data_ptr(), dx.ptr(), dom.ptr(), *s.geo(), st())
    torch.cuda.synchronize()
    assert torch.equal(dcols.cpu(), cols_layout(s.o['dcols'])), f'{s.row[0]}: d(cols) changed'
    return rc, dx, dom


def figures(tag, rid, entry, **es):
    """print the figures of a random row (e, e_cpu32, ratio) and return them"""
    print(f'DCN {tag} | {rid} | {entry}: ' + '  '.join(f'{k} e {e:.2e} e_cpu32 {b:.2e} ratio {e / max(b, 1e-30):.2f}' for k, (e, b) in es.items()))
    return es


def gated(family, rid, entry, es):
    g = ref.GATES[family]
    for k, (e, b) in es.items():
        assert e == e, (rid, entry, k, 'NaN')
        assert g is None or e <= ref.bound(b, g), (rid, entry, k, e, b, g)


def no_nan(t, what):
    n = int(torch.isnan(t.float()).sum())
    assert n == 0, f'{what}: {n} NaN of {t.numel()} -- an element left unwritten, or a guard or a padding column was read'


def fused_out(row, dev):
    rid = row[0]
    if rid not in _fused:
        s = Inputs(row, dev)
        rc, out = run_forward('fused', s, dev)
        assert rc == 0, rid
        _fused[rid] = out.check(f'{rid}: fused')
    return _fused[rid]


# ------------------------------------------------------------------------------------------------------------------------------------------
# the forward entries
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.cases('exact', 'random', entries=R.FORWARD), ids=R.case_id)
def test_forward(dev, case):
    from gssd import _lib
    row, entry = case
    rid, family, kw, feats = row
    r = ref.reference(row)
    s = Inputs(row, dev, bf16=entry == 'bf16')
    rc, out = run_forward(entry, s, dev)
    _lib.check(rc)
    got = out.check(f'{rid} | {entry}')
    s.intact()
    no_nan(got, f'{rid} | {entry}')
    want = nhwc(r['out'])
    if family == 'exact':
        want = want.to(got.dtype)
        assert torch.equal(got, want), (rid, entry, int((got != want).sum()), float((got.double() - want.double()).abs().max()))
        return
    if entry == 'bf16':
        want = nhwc(ref.reference_bf16(row)[0])
        e, l2 = ref.relerr(got, want), ref.l2rel(got, want)
        print(f'DCN bf16 | {rid} | {entry}: max {e / BF_ULP:.2f} BF_ULP  l2 {l2 / BF_ULP:.2f} BF_ULP')
        assert e < 3 * BF_ULP and l2 < BF_ULP, (rid, e, l2)
        return
    e, e32 = ref.relerr(got, want), r['e32']['out']
    if entry == 'fused':
        es = figures('fused', rid, entry, out=(e, e32))
        assert e < TOL, (rid, e)
        gated('fused', rid, entry, es)
        return
    f = fused_out(row, dev)
    e_f, x6_f = ref.relerr(f, want), ref.relerr(got, f)
    es = figures('x6', rid, entry, out=(e, e32))
    print(f'DCN x6 | {rid} | {entry}: fused vs float64 {e_f:.2e}  x6 vs fused {x6_f:.2e}')
    assert e < 2e-6 + 2 * e_f and x6_f < 1e-5, (rid, entry, e, e_f, x6_f)
    gated('x6', rid, entry, es)


def test_one_part_per_tile_on_the_exact_rows():
    """GSSD_DCN_X6_SPLITK=0: the x6 tests of the 'exact' rows in a child process (the switch is read once), so the one-part form also sees
    dg 2 and dg 4 -- the pattern and the time limit of tests/test_gpu_kernels.py::test_dcn_x6_one_part_per_tile."""
    env = dict(os.environ, GSSD_DCN_X6_SPLITK='0')
    r = subprocess.run([sys.executable, '-m', 'pytest', '-q', '-x', os.path.abspath(__file__), '-k', 'test_forward and exact and x6'],
                       capture_output=True, text=True, timeout=600, env=env)
    n = 2 * sum(1 for row, e in R.cases('exact', entries=('x6',)))
    assert r.returncode == 0 and f'{n} passed' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------------------------------
# im2col
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.cases('exact', 'random', entries=('im2col_f32', 'im2col_bf16')), ids=R.case_id)
def test_im2col(dev, case):
    from gssd import _lib
    row, entry = case
    rid, family, kw, feats = row
    bf = entry == 'im2col_bf16'
    s = Inputs(row, dev, bf16=bf)
    rc, cols = run_im2col(entry, s, dev)
    _lib.check(rc)
    got = cols.check(f'{rid} | {entry}')
    s.intact()
    no_nan(got, f'{rid} | {entry}')
    if 'im2col second item' in feats:
        HW = kw['H'] * kw['W']
        for b in range(kw['B']):
            rc, one = run_im2col(entry, s, dev, images=b)
            _lib.check(rc)
            assert torch.equal(one.check(f'{rid} | {entry} | image {b}'), got[b * HW:(b + 1) * HW]), (rid, entry, b)
        return
    r = ref.reference(row)
    if family == 'exact':
        want = cols_layout(r['cols']).to(got.dtype)
        assert torch.equal(got, want), (rid, entry, int((got != want).sum()), float((got.double() - want.double()).abs().max()))
    elif bf:
        want = cols_layout(ref.reference_bf16(row)[1])
        e, l2 = ref.relerr(got, want), ref.l2rel(got, want)
        print(f'DCN bf16 | {rid} | {entry}: max {e / BF_ULP:.2f} BF_ULP  l2 {l2 / BF_ULP:.2f} BF_ULP')
        assert e < 3 * BF_ULP and l2 < BF_ULP, (rid, e, l2)
    else:
        e = ref.relerr(got, cols_layout(r['cols']))
        es = figures('im2col', rid, entry, cols=(e, r['e32']['cols']))
        assert e < TOL, (rid, e)
        gated('im2col', rid, entry, es)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the sampling backward
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.cases('exact', 'random', entries=('col2im',)), ids=R.case_id)
def test_col2im(dev, case):
    from gssd import _lib
    row, entry = case
    rid, family, kw, feats = row
    r = ref.reference(row)
    s = Inputs(row, dev)
    n = 27 * kw['dg']
    g = torch.Generator().manual_seed(len(rid))
    preload = torch.randint(-3, 4, s.x_h.shape, generator=g).float() + 0.5 if family == 'exact' else torch.zeros(s.x_h.shape)
    rc, dx, dom = run_col2im(s, dev, preload)
    _lib.check(rc)
    s.intact()
    got_dx, got_dom = dx.check(f'{rid}: dx'), dom.check(f'{rid}: dom')
    no_nan(got_dx, f'{rid}: dx')
    no_nan(got_dom, f'{rid}: dom')
    assert not bool(got_dom[..., n:].any()), f'{rid}: the padding columns of d(om) were written'
    want_dx, want_dom = nhwc(r['dx']), nhwc(r['dom'])
    if family == 'exact':
        want_dx = (want_dx + preload.double()).float()
        assert torch.equal(got_dx, want_dx), (rid, 'dx', int((got_dx != want_dx).sum()), float((got_dx - want_dx).abs().max()))
        want_dom = want_dom.float()
        assert torch.equal(got_dom[..., :n], want_dom), (rid, 'dom', int((got_dom[..., :n] != want_dom).sum()), float((got_dom[..., :n] - want_dom).abs().max()))
        return
    es = figures('col2im', rid, entry, dx=(ref.relerr(got_dx, want_dx), r['e32']['dx']), dom=(ref.relerr(got_dom[..., :n], want_dom), r['e32']['dom']))
    assert all(e < TOL for e, _ in es.values()), (rid, es)
    gated('col2im', rid, entry, es)


# ------------------------------------------------------------------------------------------------------------------------------------------
# eligibility
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry', R.ENTRIES)
def test_refused_row_writes_nothing(dev, entry):
    """The row dcn_kernel_cases.eligible refuses for every entry: the argument error, the failed condition named, the outputs untouched.
    (col2im also refuses 'three chunks, Cout tail', whose 96 channels per group the forward entries take.)"""
    from gssd import _lib
    lib = _lib.lib
    rows = R.of_family('refused') + ([R.by_id('three chunks, Cout tail')] if entry == 'col2im' else [])
    for row in rows:
        assert not R.eligible(entry, row[2]), (row[0], entry)
        s = Inputs(row, dev, bf16=entry in ('bf16', 'im2col_bf16'))
        if entry in R.FORWARD:
            rc, out = run_forward(entry, s, dev, fill=5.0)
            outs = [out]
        elif entry == 'col2im':
            rc, dx, dom = run_col2im(s, dev, torch.full(s.x_h.shape, 5.0))
            outs = [dx, dom]
        else:
            rc, cols = run_im2col(entry, s, dev, fill=5.0)
            outs = [cols]
        err = lib.gssd_last_error().decode()
        assert rc == -1 and 'invalid argument' in err and R.refused_text(entry) in err, (row[0], entry, rc, err)
        for o in outs:
            o.untouched(f'{row[0]} | {entry}')
