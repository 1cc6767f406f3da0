"""CPU half of the backward-pass tests (tests/bwd_pass_cases.py, tests/bwd_pass_ref.py; GPU half: tests/test_gpu_bwd_passes.py).  The
float64 restatement the GPU rows are held against equals float64 autograd, and is sensitive to the two mistakes the rows are there for; the
registry closes over every entry point and form and its launch arithmetic holds; the input recipe leaves no decision ambiguous; the
entry points refuse bad arguments before they touch a device; gssd.ops.pool_leaves_gaps agrees with a pixel-by-pixel count."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd_pass_cases as R          # noqa: E402
import bwd_pass_ref as ref          # noqa: E402

BN_ROWS = R.of_kind('bn')
_ADDR = torch.zeros(64, dtype=torch.float32)          # any 16-byte aligned host address: a refused call dereferences nothing


def f64_decisions(o, kw, last=False):
    n = o['raw'].numel() // kw['C']
    sc, sh, _, _ = ref.finalize_f64(ref.batch_stats(o['raw']), n, o['gamma'], o['beta'])
    return ref.decide(o['raw'].double() * sc + sh, kw['pool'], kw['relu'], last)


@pytest.mark.parametrize('row', BN_ROWS, ids=R.row_id)
def test_restatement_equals_float64_autograd(row):
    rid, _, kw, _ = row
    o, (mask, idx), r64, e32 = ref.reference(rid, kw)
    m64, i64 = f64_decisions(o, kw)
    assert torch.equal(mask, m64) and (idx is None or torch.equal(idx, i64)), rid          # the forced decisions ARE float64's own
    draw, dg, db = ref.autograd_f64(o['raw'], o['dout'], o['gamma'], o['beta'], kw['pool'], kw['relu'])
    e = (ref.relerr(r64['draw'], draw), ref.relerr(r64['dgamma'], dg), ref.relerr(r64['dbeta'], db))
    print(f'{rid}: restatement vs autograd {e[0]:.1e} {e[1]:.1e} {e[2]:.1e}')
    assert max(e) < 1e-12, (rid, e)
    # the bound the GPU row applies is never looser than tests/test_gpu_kernels.py::test_bn_relu_pool_backward's
    g = max(ref.gate_of('bn_f32'), ref.gate_of('bn_mixed'))
    assert ref.bound(e32['draw'], g) < 2e-4 and ref.bound(e32['dgamma'], g) < 1e-4 and ref.bound(e32['dbeta'], g) < 1e-4, (rid, e32)


@pytest.mark.parametrize('row', [r for r in BN_ROWS if set(r[3]) & set(R.SENSITIVE)], ids=R.row_id)
def test_restatement_is_sensitive(row):
    """Made wrong in the way the row is there for, the restatement leaves autograd by more than 100 x the GPU row's allowance.  (About the
    reference alone: no project code is made wrong.)"""
    rid, _, kw, feats = row
    o, _, _, e32 = ref.reference(rid, kw)
    draw, _, _ = ref.autograd_f64(o['raw'], o['dout'], o['gamma'], o['beta'], kw['pool'], kw['relu'])
    if 'sensitive: last maximum' in feats:
        mask, idx = f64_decisions(o, kw, last=True)
        wrong = ref.bn_backward(o['raw'], o['dout'], o['gamma'], mask, idx, torch.float64)
    else:
        mask, idx = f64_decisions(o, kw)
        wrong = ref.bn_backward(o['raw'], o['dout'], o['gamma'], mask, idx, torch.float64, uncovered_value=1.0, pool=kw['pool'])
    assert ref.relerr(wrong['draw'], draw) > 100 * ref.bound(e32['draw'], ref.gate_of('bn_f32')), rid


@pytest.mark.parametrize('row', R.of_kind('bn', 'mixed'), ids=R.row_id)
def test_inputs_leave_no_decision_ambiguous(row):
    rid, _, kw, feats = row
    o = ref.make_inputs(rid, kw)
    assert o['ambiguous'] == 0 and o['rounds'] <= 8, (rid, o['ambiguous'], o['rounds'])
    assert not bool(ref.ambiguous(o['raw'], o['gamma'], o['beta'], kw['pool'], kw['relu']).any()), rid
    a = o['gamma'].abs()
    assert 0.2 <= float(a.min()) and float(a.max()) <= 1.5 and bool((o['gamma'] > 0).any()) and bool((o['gamma'] < 0).any()), rid
    if 'dout_bf16' in kw:
        assert torch.equal(o['raw'], o['raw'].to(torch.bfloat16).float()), rid
        assert not kw['dout_bf16'] or torch.equal(o['dout'], o['dout'].to(torch.bfloat16).float()), rid
    if kw.get('ties'):          # the planted duplicates survived the redraws somewhere: a window with two equal maxima exists
        first, last = f64_decisions(o, kw)[1], f64_decisions(o, kw, last=True)[1]
        assert bool((first != last).any()), rid


def test_registry_closes_over_entries_and_forms():
    ids = [r[0] for r in R.ROWS]
    assert len(set(ids)) == len(ids) and len(R.ENTRIES) == len(set(R.ENTRIES)) == 10
    known = set(R.FORMS) | set(R.GRID) | set(R.SENSITIVE)
    for rid, kind, kw, feats in R.ROWS:
        assert set(feats) <= known, (rid, set(feats) - known)
    called = {e for r in R.ROWS for e in R.entries_of(r)}
    assert called == set(R.ENTRIES), set(R.ENTRIES) ^ called
    for f in R.FORMS + R.GRID + R.SENSITIVE:
        assert any(f in r[3] for r in R.ROWS), f'no row carries {f!r}'
    # the three sequences of a BatchNorm row: a pooled row runs plan/pool, an unpooled one plan/no-pool, both the helper
    for rid, kind, kw, feats in BN_ROWS:
        assert ('plan/pool' in feats) == bool(kw['pool']) and ('plan/no-pool' in feats) == (not kw['pool']) and 'helper' in feats, rid
    # mixed rows: the five shapes, each with fp32 and with bf16 d(out); the hand-over on every non-overlapping pool and on no other row
    mixed = R.of_kind('mixed')
    shapes = {tuple(sorted((k, v) for k, v in r[2].items() if k != 'dout_bf16')) for r in mixed}
    assert len(shapes) == 5 and len(mixed) == 10
    for rid, _, kw, feats in mixed:
        assert ('bf16 dout' in feats) == kw['dout_bf16'] and ('fp32 dout' in feats) != kw['dout_bf16'], rid
        nonoverlap = bool(kw['pool']) and kw['pool'][1] >= kw['pool'][0]
        assert ('dz_bf16 hand-over' in feats) == nonoverlap and ('store_f32 = 0' in feats) == (not kw['pool']) and 'dz16' in feats, rid
    for want in ('idle threads', 'unrolled + tail', 'pool even', 'pool floor odd', 'pool overlap'):
        assert any(want in r[3] for r in mixed), want


def test_registry_shapes_and_launch_arithmetic():
    """Every 'grid' feature recomputed from the launch constants named in tests/bwd_pass_cases.py."""
    for rid, kind, kw, feats in R.ROWS:
        f = set(feats)
        if kind in ('bn', 'mixed', 'noaffine'):
            assert kw['C'] % 4 == 0 and kw['C'] <= R.MAX_C, rid
            assert (kw['H'] != kw['W']) or (f & set(R.SQUARE_BY_SPEC)), rid                  # a swapped extent shows
            (rt, rwg, rs, ridle, rn), (at, awg, as_, aidle, an) = R.bn_grids(kw)
            launches = [(rt, rs, ridle)] if kind == 'noaffine' else [(rt, rs, ridle), (at, as_, aidle)]
            assert ('idle threads' in f) == all(i > 0 for _, _, i in launches), (rid, launches)
            assert ('C4 = 1' in f) == (kw['C'] == 4) and ('widest' in f) == (kw['C'] == R.MAX_C), rid
            if not kw['pool']:
                assert ('second item' in f) == (as_ < at <= R.BN_UNR * as_), (rid, at, as_)
                assert ('unrolled + tail' in f) == (R.BN_UNR * as_ < at < (R.BN_UNR + 1) * as_), (rid, at, as_)
            else:
                assert ('pool second item' in f) == (rs < rt < 2 * rs), (rid, rt, rs)
                k, s, p, ceil = kw['pool']
                Ho, Wo = R.out_extent(kw)
                assert ('pool overlap' in f) == (s < k) and ('pool stride 2 overlap' in f) == (s < k and s == 2), rid
                assert ('pool floor odd' in f) == (R.uncovered(kw) > 0), rid
                assert ('pool ceil odd' in f) == ((Ho - 1) * s - p + k > kw['H'] and (Wo - 1) * s - p + k > kw['W'] and s >= k), rid
                assert ('pool even' in f) == (s >= k and R.uncovered(kw) == 0 and 'pool ceil odd' not in f and 'pool second item' not in f), rid
            if 'pool floor odd' in f:
                assert R.out_extent(kw) == (3, 2) and R.uncovered(kw) == 7 * 5 - 6 * 4, rid
            if 'pool ceil odd' in f:
                assert R.out_extent(kw) == (4, 3), rid
            if kind == 'noaffine':
                assert ('relu, no pool' in f) == (kw['relu'] and not kw['pool']) and ('pool only' in f) == (bool(kw['pool']) and not kw['relu']), rid
                assert ('relu + pool' in f) == (bool(kw['pool']) and kw['relu']), rid
        elif kind == 'colsum':
            total = kw['rows'] * kw['C']
            wg, gs, idle, n = R.wide_grid(total, kw['C'], R.COLSUM_MAX_WG)
            assert ('colsum second item' in f) == (total > gs) and ('idle threads' in f) == (idle > 0), (rid, total, gs, idle)
            assert ('row stride' in f) == (kw['stride'] > kw['C']) and ('widest' in f) == (kw['C'] == R.MAX_C), rid
        elif kind == 'l2norm':
            pixels, C4 = kw['B'] * kw['H'] * kw['W'], kw['C'] // 4
            assert ('second pixel' in f) == (pixels > R.l2_waves(pixels)) and R.l2_waves(10 ** 6) == 4096, rid
            assert ('one lane' in f) == (C4 == 1) and ('lane loops twice' in f) == (C4 > R.WAVE) and ('dx_add' in f) == kw['dx_add'], rid
            assert kw['H'] != kw['W'] or 'second pixel' in f, rid
        elif kind == 'upsample':
            s, quads = kw['s'], kw['B'] * kw['H'] * kw['W'] * kw['C'] // 4
            assert kw['H'] >= (kw['Ho'] - 1) * s + 1 and kw['W'] >= (kw['Wo'] - 1) * s + 1 and kw['C'] % 4 == 0, rid
            assert ('exact fit' in f) == (kw['H'] == (kw['Ho'] - 1) * s + 1 or kw['W'] == (kw['Wo'] - 1) * s + 1), rid
            assert ('zero tail' in f) == (kw['H'] == kw['Ho'] * s or kw['W'] == kw['Wo'] * s), rid
            assert ('copy second item' in f) == (quads > R.copy_threads()) and ('s = 3' in f) == (s == 3), (rid, quads)
            assert kw['H'] != kw['W'] or 'copy second item' in f, rid
        else:
            assert kind == 'gather'
            n = kw['B'] * kw['HW'] * kw['A'] * (4 + kw['nc'])
            assert kw['off'] + kw['HW'] * kw['A'] <= kw['P'], rid
            assert ('copy second item' in f) == (n > R.copy_threads()), (rid, n)
            assert ('prior_off = 0' in f) == (kw['off'] == 0) and ('prior_off at end' in f) == (kw['off'] > 0 and kw['off'] + kw['HW'] * kw['A'] == kw['P']), rid
            assert ('nc 3' in f) == (kw['nc'] == 3) and ('A 6' in f) == (kw['A'] == 6), rid
    # the figures the registry's docstring quotes
    by = {r[0]: r[2] for r in R.ROWS}
    assert R.bn_grids(by['idle threads C 12'])[1][2:4] == (1023, 1) and R.bn_grids(by['idle threads C 100'])[1][2:4] == (2025, 23)
    assert R.bn_grids(by['second item'])[1][:3] == (720000, 512, 524288)
    assert R.bn_grids(by['unrolled + tail'])[1][:4] == (1058400, 512, 524286, 2) and 1058400 - 2 * 524286 == 9828
    assert R.bn_grids(by['pool grid'])[0][:3] == (529200, 512, 524286)
    assert R.bn_grids(by['widest'])[1][:4] == (9216, 9, 9216, 0)
    assert R.wide_grid(5776 * 24, 24, R.COLSUM_MAX_WG)[:3] == (128, 131064, 8)


def test_pool_leaves_gaps_counts_pixels():
    """gssd.ops.pool_leaves_gaps -- the one predicate behind every routed-gradient buffer (ops.bn_backward, bwd_ops._convbn / _pool /
    _relupool) -- against a pixel-by-pixel count, over every small pool geometry torch accepts."""
    from gssd import ops
    for k in (1, 2, 3):
        for s in (1, 2, 3, 4):
            for p in range(k // 2 + 1):
                for ceil in (False, True):
                    for H in range(k, 12):
                        for W in (H, H + 1, 9):
                            if W < k:
                                continue
                            kw = dict(H=H, W=W, pool=(k, s, p, ceil))
                            Ho, Wo = R.out_extent(kw)
                            assert ops.pool_out_size(H, k, s, p, ceil) == Ho
                            assert ops.pool_leaves_gaps(H, W, Ho, Wo, k, s, p) == (R.uncovered(kw) > 0), kw
    for rid, kind, kw, feats in R.ROWS:
        if kind in ('bn', 'mixed', 'noaffine') and kw['pool']:
            Ho, Wo = R.out_extent(kw)
            assert ops.pool_leaves_gaps(kw['H'], kw['W'], Ho, Wo, *kw['pool'][:3]) == ('pool floor odd' in feats), rid
    assert not ops.pool_leaves_gaps(5, 7, 5, 7, 0, 1, 0)                                       # no pool
    # the shipped graphs' pools cover their maps: nothing more is zeroed there than before
    for H, pool in ((300, (2, 2, 0, False)), (150, (2, 2, 0, False)), (75, (2, 2, 0, True)), (38, (2, 2, 0, False)), (19, (3, 1, 1, False))):
        Ho = ops.pool_out_size(H, pool[0], pool[1], pool[2], pool[3])
        assert not ops.pool_leaves_gaps(H, H, Ho, Ho, *pool[:3]), H


def test_refused_arguments_touch_no_device():
    """C % 4 != 0, C > 4096 and a bf16 hand-over with an overlapping pool come back GSSD_EINVAL with the failed condition named -- on a host
    without a GPU: the argument checks stand in front of every HIP call."""
    from gssd import _lib
    lib, a = _lib.lib, _ADDR.data_ptr()

    def refused(rc, text):
        err = lib.gssd_last_error().decode()
        assert rc == -1 and 'invalid argument' in err and text in err, (rc, err)
    for C, text in ((6, 'C % 4 == 0'), (4100, 'C <= 4096')):
        refused(lib.gssd_bn_bwd_reduce_f32(a, a, a, a, a, a, 1, 3, 2, C, 3, 2, 0, 1, 0, 1, None), text)
        refused(lib.gssd_bn_bwd_reduce_mixed(a, 0, a, a, a, a, 0, a, 1, 3, 2, C, 3, 2, 0, 1, 0, 1, None), text)
        refused(lib.gssd_bn_bwd_apply_f32(a, a, a, a, a, 6, C, 0, None), text)
        refused(lib.gssd_bn_bwd_apply_masked_f32(a, a, a, a, 1, a, a, a, a, 6, C, 0, None), text)
        refused(lib.gssd_bn_bwd_apply_mixed(a, 0, a, a, a, a, a, 1, a, a, a, 6, C, 0, 1, None), text)
        refused(lib.gssd_l2norm_bwd_f32(a, a, a, a, 0, a, 6, C, 1e-10, None), text)
    refused(lib.gssd_colsum_f32(a, 3, 4100, 4100, a, None), 'C <= 4096')
    refused(lib.gssd_colsum_f32(a, 3, 24, 20, a, None), 'row_stride >= C')
    refused(lib.gssd_bn_bwd_reduce_mixed(a, 0, a, a, a, 0, a, a, 2, 5, 7, 12, 5, 7, 3, 1, 1, 1, None), 'pool_s >= pool_k')
    refused(lib.gssd_bn_bwd_reduce_mixed(a, 0, a, a, a, 0, a, a, 2, 5, 7, 12, 5, 7, 0, 1, 0, 1, None), 'pool_k > 0')
    refused(lib.gssd_bn_bwd_reduce_f32(a, a, a, 0, a, a, 1, 3, 2, 4, 3, 2, 0, 1, 0, 1, None), '(scale == nullptr) == (shift == nullptr)')
    refused(lib.gssd_bn_bwd_reduce_f32(a, a, 0, 0, 0, 0, 1, 3, 2, 4, 3, 2, 0, 1, 0, 1, None), 'dz ||')          # nothing to write
    refused(lib.gssd_bn_bwd_reduce_f32(a, a, 0, 0, a, 0, 1, 3, 2, 4, 2, 2, 0, 1, 0, 1, None), 'Ho == H')
    refused(lib.gssd_upsample_insert_f32(a, a, 1, 4, 3, 9, 9, 4, 3, None), 'H >= (Ho - 1) * s + 1')
    refused(lib.gssd_upsample_insert_f32(a, a, 1, 4, 3, 10, 9, 6, 3, None), 'C % 4 == 0')
    refused(lib.gssd_heads_gather_f32(a, a, a, 2, 15, 6, 3, 150, 61, None), 'prior_off + HW * A <= P')
