"""CPU half of the deformable-conv kernel tests (tests/dcn_kernel_cases.py, tests/dcn_kernel_ref.py; GPU half:
tests/test_gpu_dcn_kernels.py).  Every feature a row claims is recomputed from the registry's launch constants, and those constants are the
ones the sources state; the rows land their samples where they say (gates, strips, window shares); on every 'exact' row float32 equals
float64 equals oracle/dcn_scalar for the output, the columns and the three gradients -- the bit-exact gate of the GPU module is a property
of the inputs, not of a kernel; the reference moves when the sampling rule is restated with one of the two mistakes the 'gates' rows are
there for; the launchers refuse the shape the registry says they refuse before they touch a device."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gssd_oracle as O      # noqa: E402
import dcn_kernel_cases as R             # noqa: E402
import dcn_kernel_ref as ref             # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'grouped-ssd-pytorch_amd', 'gssd', 'csrc')
SMALL = [r for r in R.of_family('exact', 'random') if 'im2col second item' not in r[3]]
EXACT = R.of_family('exact')
_ADDR = torch.zeros(64, dtype=torch.float32)          # any 16-byte aligned host address: a refused call dereferences nothing


def test_constants_are_the_sources():
    """The registry's constants against the lines of csrc/ that define them."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()
    for name in ('dcn_fused.hip', 'dcn_x6.hip', 'dcn_bf16.hip'):
        m = re.search(r'constexpr int BM = (\d+), BN = (\d+), BKC = (\d+);', src(name))
        assert m and tuple(map(int, m.groups())) == (R.BM, R.BN, R.BKC), name
    d = src('dcn.hip')
    assert int(re.search(r'constexpr int DC_R = (\d+);', d).group(1)) == R.DC_R
    assert tuple(map(int, re.search(r'constexpr int TH = (\d+), TW = (\d+);', d).groups())) == (R.TH, R.TW)
    assert f'(C / dg) % {R.SLICE} == 0' in d and f'const int slices = C / {R.SLICE};' in d
    assert tuple(map(int, re.search(r'IM_UN = sizeof\(T\) == 2 \? (\d+) : (\d+);', d).groups())) == (R.IM_UN_BF16, R.IM_UN_F32)
    assert d.count(f'if (blocks > {R.IM_MAX_WG}) blocks = {R.IM_MAX_WG};') == 2 and d.count(f'(units + {R.IM_THREADS - 1}) / {R.IM_THREADS}') == 2
    assert f'base += nwaves * {R.IM_WAVE}' in d


def test_registry_features_recomputed():
    ids = [r[0] for r in R.ROWS]
    assert len(set(ids)) == len(ids)
    for rid, family, kw, feats in R.ROWS:
        f = set(feats)
        assert f <= set(R.FEATURES), (rid, f - set(R.FEATURES))
        if family == 'refused':
            assert not any(R.eligible(e, kw) for e in R.ENTRIES), rid
            continue
        M, mt, ntn, last, chunks = R.forward_tiles(kw)
        if 'im2col second item' not in f:
            assert ('ragged row tile' in f) == (M % R.BM != 0) and ('tiles cross images' in f) == R.tiles_cross_images(kw), rid
            assert ('second column tile' in f) == (ntn > 1) and ('x6 two parts' in f) == (R.x6_parts(kw) == 2), rid
            assert ('x6 one part' in f) == (R.x6_parts(kw) == 1), rid
            assert ('slices share scalars' in f) == (R.col2im_grid(kw)[2] > 1), rid
            share = ref.window_share(R.by_id(rid))
            assert ('window only' in f) == (share == 1.0 and family == 'random') and ('overflow only' in f) == (share == 0.0 and family == 'random'), (rid, share)
            if 'window mixed' in f:
                assert 0.0 < share < 1.0, (rid, share)
            assert kw['H'] != kw['W'], rid                                                    # a swapped extent shows
        units, per_pass, tail = R.im2col_walk(kw)
        assert ('im2col second item' in f) == (units > per_pass) and per_pass <= R.IM_MAX_WG * R.IM_THREADS, (rid, units, per_pass)
        assert ('im2col ragged walk' in f) == (tail % R.IM_UN_F32 != 0 or tail % R.IM_UN_BF16 != 0), (rid, tail)
        assert ('thin' in f) == (kw['H'] == 1 or kw['W'] == 1) and ('bias NULL' in f) == (not kw['bias']), rid
        assert ('om_stride padded' in f) == (kw['om_stride'] > 27 * kw['dg']), rid
        assert ('all closed' in f) == (kw.get('offsets') == 'closed') and ('one pixel' in f) == (kw.get('offsets') == 'one pixel'), rid
    for feat in R.FEATURES:
        assert any(feat in r[3] for r in R.ROWS), f'no row carries {feat!r}'
    # the figures the registry's docstring quotes
    for rid, (M, mt, last, chunks, slices) in R.FIGURES.items():
        kw = R.by_id(rid)[2]
        assert R.forward_tiles(kw)[0:2] == (M, mt) and R.forward_tiles(kw)[3:] == (last, chunks), rid
        assert slices is None or R.col2im_grid(kw)[2] == slices, rid
    kw = R.by_id('gates cross images')[2]
    assert R.BM - kw['H'] * kw['W'] == 51 and R.x6_parts(kw) == 1            # the second row tile starts at pixel 51 of image 1
    assert R.x6_parts(R.by_id('gates shared scalars')[2]) == 2 and R.by_id('gates shared scalars')[2]['dg'] // 2 == 2
    assert R.col2im_grid(R.by_id('mixed')[2]) == (3, 2, 1, 9, 13)
    units, per_pass, _ = R.im2col_walk(R.by_id('im2col second item')[2])
    kw = R.by_id('im2col second item')[2]
    assert per_pass == 16384 * 256 < units and units // kw['B'] < per_pass          # one image alone stays below the cap


def test_every_entry_has_its_rows():
    for e in R.ENTRIES:
        n_exact = sum(R.eligible(e, r[2]) for r in R.of_family('exact'))
        n_random = sum(1 for r, ee in R.cases('random', entries=(e,)))
        assert n_exact >= 3 and n_random >= 2, (e, n_exact, n_random)
    tail = R.by_id('three chunks, Cout tail')[2]
    assert not R.eligible('col2im', tail) and all(R.eligible(e, tail) for e in R.ENTRIES if e != 'col2im')
    assert {e for r, e in R.cases('random') if 'im2col second item' in r[3]} == {'im2col_f32', 'im2col_bf16'}


@pytest.mark.parametrize('row', EXACT + R.of_family('random')[:5], ids=R.row_id)
def test_rows_put_their_samples_where_they_say(row):
    rid, family, kw, feats = row
    n = ref.sample_counts(row)
    share = ref.window_share(row)
    print(f'{rid}: {n}  window share {share:.3f}')
    total = kw['B'] * kw['H'] * kw['W'] * 9 * kw['dg']
    if 'gates' in feats:
        for gate in ('on -1 y', 'on -1 x', 'on extent y', 'on extent x'):
            assert n[gate] >= 20, (rid, gate, n[gate])
        for strip in ('low strip y', 'low strip x', 'high strip y', 'high strip x'):
            assert n[strip] >= 10, (rid, strip, n[strip])
        assert min(n['integers y'], n['integers x'], n['far y'], n['far x']) >= 100, rid
    if 'thin' in feats:          # both gates and the far strip of the one-pixel extent: the far corner is never valid there
        a = 'y' if kw['H'] == 1 else 'x'
        assert n['on -1 ' + a] >= 10 and n['on extent ' + a] >= 10 and n['low strip ' + a] + n['high strip ' + a] >= 10, (rid, n)
    if 'all closed' in feats:
        assert n['far y'] == n['far x'] == total and share == 0.0, rid
    if 'one pixel' in feats:
        py, px = ref.positions(ref.split_om(ref.make_inputs(row)['om'], kw['dg'])[0], kw)
        assert bool((py == kw['target'][0]).all()) and bool((px == kw['target'][1]).all()) and 0.2 < share < 0.8, (rid, share)
    if family == 'random':
        off = ref.split_om(ref.make_inputs(row)['om'], kw['dg'])[0]
        assert torch.equal(off * 512 % 2, torch.ones_like(off)), f'{rid}: offsets off the shifted grid'          # odd multiples of 1/512
        py, px = ref.positions(off.double(), kw)
        p32 = ref.positions(off, kw)
        assert torch.equal(torch.floor(py), torch.floor(p32[0]).double()) and torch.equal(torch.floor(px), torch.floor(p32[1]).double()), rid
    if rid == 'mixed':
        assert 0.2 < share < 0.8, share
    if rid == 'window only':
        assert share == 1.0 and float(ref.split_om(ref.make_inputs(row)['om'], kw['dg'])[0].abs().max()) <= 0.9
    if rid == 'overflow only':
        off = ref.split_om(ref.make_inputs(row)['om'], kw['dg'])[0]
        assert share == 0.0 and float(off.abs().min()) >= 4.0 and bool(ref.window_units(off, kw)[1].all()), rid
        assert n['far y'] == n['far x'] == 0


@pytest.mark.parametrize('row', EXACT, ids=R.row_id)
def test_exact_rows_are_exact_in_every_precision(row):
    """float32 = float64 = dcn_scalar, the float64 results rounded once: the output, the columns, d(x), d(offset), d(logit)."""
    rid, _, kw, feats = row
    o, r = ref.make_inputs(row), ref.reference(row)
    for k in ('out', 'cols', 'dx', 'doff', 'dlogit'):
        assert torch.equal(r['32'][k], r[k].float()), (rid, k, int((r['32'][k] != r[k].float()).sum()))
        assert torch.equal(r[k].float().double() * 64, torch.round(r[k].float().double() * 64)), (rid, k)          # multiples of 1/64
    assert torch.equal(ref.scalar_out(row), r['out'].float()), rid
    assert torch.equal(o['dcols'].double(), o['dcols64']), rid
    # bf16 holds the operands and the blended columns exactly, and the mask the kernels compute is 0, 1/2 or 1
    assert torch.equal(ref.q16(r['cols'].float()), r['cols'].float()) and torch.equal(ref.q16(o['x']), o['x']) and torch.equal(ref.q16(o['w']), o['w']), rid
    logit = ref.split_om(o['om'], kw['dg'])[1]
    m = 1.0 / (1.0 + torch.exp(-logit))
    assert set(m.unique().tolist()) <= {0.0, 0.5, 1.0} and torch.equal(m, torch.sigmoid(logit)), rid
    if 'all closed' in feats:
        assert torch.equal(r['out'], o['bias'].double().view(1, -1, 1, 1).expand_as(r['out'])), rid
        assert not bool(r['cols'].any()) and not bool(r['dx'].any()) and not bool(r['dom'].any()), rid
    else:
        assert all(bool(r[k].any()) for k in ('cols', 'dx', 'doff', 'dlogit')), rid
    if 'one pixel' in feats:
        ty, tx = kw['target']
        dx = r['dx'].clone()
        assert bool(dx[:, :, ty, tx].any())
        dx[:, :, ty, tx] = 0
        assert not bool(dx.any()), rid


@pytest.mark.parametrize('row', SMALL, ids=R.row_id)
def test_sample_is_the_oracles_column_matrix(row):
    """W cols + bias of sample() is the oracle's output on every row; where the identity weight of test_dcn_col2im_backward fits in memory
    (C <= 128) the columns themselves are the oracle's."""
    rid, family, kw, _ = row
    o, r = ref.make_inputs(row), ref.reference(row)
    out = ref.contract(r['cols'], o['w'].double(), o['bias'])
    assert ref.relerr(out, r['out']) < 1e-13, rid
    if kw['C'] <= 128:
        C = kw['C']
        off, logit = ref.split_om(o['om'], kw['dg'])
        eye = torch.eye(C * 9, dtype=torch.float64).view(C * 9, C, 3, 3)
        cols = O.dcn_v2_conv(o['x'].double(), off.double(), torch.sigmoid(logit.double()), eye, torch.zeros(C * 9, dtype=torch.float64), 1, 1, 1, kw['dg'])
        assert torch.equal(cols.view(r['cols'].shape), r['cols']), rid


def test_gates_sit_below_the_ceilings():
    """G * e_cpu32 + 1e-7 of every random row is far below TOL = 1e-4 (the x6 ceiling depends on dcn_fused's own error: the GPU module
    asserts both); the exact rows leave float32 nothing to round, so they have no allowance at all."""
    for row in [r for r in R.of_family('random') if 'im2col second item' not in r[3]]:
        e32 = ref.reference(row)['e32']
        assert 1e-8 < min(e32.values()) and max(e32.values()) < 1e-6, (row[0], e32)
        for fam, k in (('fused', 'out'), ('x6', 'out'), ('im2col', 'cols'), ('col2im', 'dx'), ('col2im', 'dom')):
            assert ref.bound(e32[k], ref.GATES[fam]) < 5e-6, (row[0], fam, k)
    for row in EXACT:
        assert max(ref.reference(row)['e32'].values()) < 1e-80, row[0]


@pytest.mark.parametrize('row', [r for r in EXACT if 'gates' in r[3]], ids=R.row_id)
def test_reference_tells_the_conventions_apart(row):
    """Restated with p <= H for the gate (the near corner then reads the clamped last row with weight 1), or with the far corner taken at H,
    the reference changes outputs of every 'gates' row.  (About the reference alone: no project code is made wrong.)"""
    rid, _, kw, _ = row
    o, r = ref.make_inputs(row), ref.reference(row)
    for conv in (dict(upper_closed=True), dict(far_at_extent=True)):
        cols = ref.cols_of(o, kw, torch.float64, **conv)
        out = ref.contract(cols, o['w'].double(), o['bias'])
        n_cols, n_out = int((cols != r['cols']).sum()), int((out.float() != r['out'].float()).sum())
        print(f'{rid} {conv}: {n_cols} columns and {n_out} outputs change')
        assert n_cols >= 20 and n_out >= 1, (rid, conv, n_cols, n_out)


@pytest.mark.parametrize('entry', R.ENTRIES)
def test_refused_shape_touches_no_device(entry):
    """The 'refused' row comes back GSSD_EINVAL with the failed condition named -- on a host without a GPU: the argument checks stand in
    front of every HIP call.  (The GPU module repeats the call with real buffers and finds them untouched.)"""
    from gssd import _lib
    lib, a = _lib.lib, _ADDR.data_ptr()
    kw = R.of_family('refused')[0][2]
    assert not R.eligible(entry, kw)
    geo = (kw['B'], kw['H'], kw['W'], kw['C'], kw['dg'], kw['om_stride'])
    if entry.startswith('im2col'):
        rc = getattr(lib, R.SYMBOL[entry])(a, a, a, *geo, None)
    elif entry == 'col2im':
        rc = lib.gssd_dcn_col2im_f32(a, a, a, a, a, *geo, None)
    elif entry in ('x6', 'x6_f16'):
        rc = lib.gssd_dcn_forward_x6_ex(a, a, a, a, a, *geo, kw['Cout'], _lib.CONV_F16_OK if entry == 'x6_f16' else 0, None)
    else:
        rc = getattr(lib, R.SYMBOL[entry])(a, a, a, a, a, *geo, kw['Cout'], None)
    err = lib.gssd_last_error().decode()
    assert rc == -1 and 'invalid argument' in err and R.refused_text(entry) in err, (entry, rc, err)
