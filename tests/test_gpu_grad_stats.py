"""gssd.optim.grad_stats / GradMonitor / utils.check_grad_norm on the MI355X (csrc/optim_stats.hip) against numpy float64 on host copies.

The yardstick of a row is ``np.sum(x.astype(np.float64) ** 2)``: n non-negative terms, each exact in fp64 (an fp32 square has 48
significand bits), so ANY summation order -- numpy's pairwise one, the kernel's per-thread / butterfly / strided one -- is within
(n - 1) 2^-53 relative of the true sum, and two such sums within n 2^-52 of each other.  Hence, per row with n = numel (the totals row:
all elements): sumsq within n 2^-52 relative, norm the same plus 2^-52 (two square roots), absmax and nonfinite EXACT, and a NaN / inf
in sumsq and norm of numpy's class.  Host data is generated once per module and never modified."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, NETS)
from gpu_common import synth                  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
EDGE_NUMELS = (1, 2, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 8195)
EDGE_SCALES = (1e-42, 1e-40, 1e-30, 1e-20, 1e-10, 1e-3, 1.0, 1e3, 1e10, 1e20, 1e25, 1e30)      # per item; the weights take them reversed
NAN, INF = float('nan'), float('inf')


# ----------------------------------------------------------------------------------------------
# the yardstick
# ----------------------------------------------------------------------------------------------
def want_cols(x):
    """(sumsq, norm, absmax, nonfinite) of a host fp32 array (None / empty: zeros) in float64."""
    if x is None or x.size == 0:
        return 0.0, 0.0, 0.0, 0.0
    d = x.astype(np.float64)
    with np.errstate(over='ignore', invalid='ignore'):
        ss = np.sum(d ** 2)
        norm = np.sqrt(ss)
    fin = np.isfinite(d)
    return float(ss), float(norm), float(np.abs(d[fin]).max()) if fin.any() else 0.0, float((~fin).sum())


def check_cols(got, x, what):
    n = 0 if x is None else x.size
    ss, norm, amax, nf = want_cols(x)
    worst = 0.0
    for name, g, w, tol in (('sumsq', got[0], ss, n * EPS), ('norm', got[1], norm, (n + 1) * EPS)):
        if np.isnan(w):
            assert np.isnan(g), f'{what}: {name} is {g}, numpy has NaN'
        elif np.isposinf(w):
            assert np.isposinf(g), f'{what}: {name} is {g}, numpy has inf'
        else:
            assert abs(g - w) <= tol * w, f'{what}: {name} {g!r} against {w!r}: off by {abs(g - w) / w:.3g} relative, bound {tol:.3g}'
            if w:
                worst = max(worst, abs(g - w) / w / tol)
    assert got[2] == amax, f'{what}: absmax {got[2]!r}, not {amax!r}'
    assert got[3] == nf, f'{what}: nonfinite {got[3]!r}, not {nf!r}'
    return worst


def check_table(table, ps, gs, what):
    """table: host [N + 1, 8]; ps / gs: per row the host array of the tensor / its gradient, or None where that side is not read."""
    assert table.shape == (len(gs) + 1, 8) and table.dtype == np.float64
    worst = 0.0
    for i, (p, g) in enumerate(zip(ps, gs)):
        worst = max(worst, check_cols(table[i, 0:4], g, f'{what}, row {i} gradient'), check_cols(table[i, 4:8], p, f'{what}, row {i} weights'))
    for side, arrs in ((0, gs), (4, ps)):
        arrs = [a.ravel() for a in arrs if a is not None and a.size]
        worst = max(worst, check_cols(table[-1, side:side + 4], np.concatenate(arrs) if arrs else None, f'{what}, totals {"gp"[side // 4]}'))
    return worst


def place(arrays, phases, dev):
    """Views of ONE flat device tensor: array i starts at an element offset that is phases[i] modulo 4, so 4 * phases[i] bytes modulo 16."""
    offs, o = [], 0
    for a, ph in zip(arrays, phases):
        o += (ph - o) % 4
        offs.append(o)
        o += a.size
    flat = np.zeros(o + 4, np.float32)
    for a, o in zip(arrays, offs):
        flat[o:o + a.size] = a
    d = torch.from_numpy(flat).to(dev)
    assert d.data_ptr() % 16 == 0
    return d, [d[o:o + a.size] for a, o in zip(arrays, offs)], offs


class TensorSet:
    """Parameters that are views of one flat tensor, gradients (where given) views of a second one, at the given 4-byte phases."""

    def __init__(self, dev, ps, gs, p_phases=None, g_phases=None):
        n = len(ps)
        self.ps, self.gs = ps, gs
        self.flat_p, views, self.p_offs = place(ps, p_phases or [0] * n, dev)
        self.params = [torch.nn.Parameter(v) for v in views]
        have = [i for i in range(n) if gs[i] is not None]
        self.flat_g, gviews, offs = place([gs[i] for i in have], [(g_phases or [0] * n)[i] for i in have], dev)
        self.g_offs = dict(zip(have, offs))
        for i, v in zip(have, gviews):
            self.params[i].grad = v
        for p, v in zip(self.params, views):
            assert p.data_ptr() == v.data_ptr()

    def named(self):
        return [(f't{i}', p) for i, p in enumerate(self.params)]


@functools.lru_cache(maxsize=None)
def edge_host():
    rng = np.random.default_rng(20261)
    with np.errstate(under='ignore'):
        gs = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in zip(EDGE_NUMELS, EDGE_SCALES)]
        ps = [(rng.standard_normal(n) * s).astype(np.float32) for n, s in zip(EDGE_NUMELS, reversed(EDGE_SCALES))]
        # fp32 squares would lose both ends: the subnormal items underflow to 0, the 1e30 ones overflow
        with np.errstate(over='ignore'):
            assert np.all(gs[0] * gs[0] == 0) and np.any(gs[0] != 0) and np.isinf(gs[-1] * gs[-1]).any()
    for a in gs + ps:
        a.setflags(write=False)
    return ps, gs


def edge_set(dev):
    ps, gs = edge_host()
    n = len(ps)
    s = TensorSet(dev, ps, gs, [i % 4 for i in range(n)], [(i + 1) % 4 for i in range(n)])
    assert {p.data_ptr() % 16 for p in s.params} == {0, 4, 8, 12} == {p.grad.data_ptr() % 16 for p in s.params}
    assert all(p.data_ptr() % 16 != p.grad.data_ptr() % 16 for p in s.params)
    return s


@pytest.fixture(scope='module')
def edge(dev):
    """The edge set on the device and its clean table (host copy); tests that plant values put the originals back."""
    from gssd import optim
    s = edge_set(dev)
    s.clean = optim.grad_stats(s.named()).table.cpu().numpy().copy()
    return s


# ----------------------------------------------------------------------------------------------
# 1. the edge table
# ----------------------------------------------------------------------------------------------
def test_edge_table(dev, edge):
    from gssd import optim
    stats = optim.grad_stats(edge.named())
    assert stats.names == [f't{i}' for i in range(len(EDGE_NUMELS))] and stats.without_grad == []
    assert stats.table.dtype == torch.float64 and stats.table.shape == (len(EDGE_NUMELS) + 1, 8) and stats.table.device == dev
    t = stats.table.cpu().numpy()
    print('edge table: worst error / bound', check_table(t, edge.ps, edge.gs, 'edge'))
    # the subnormal and the 1e30 rows carry real information
    assert 0 < t[0, 1] < 1e-40 and t[-2, 1] > 1e30 and 0 < t[-1, 5] < math.inf
    # the views are views of the same table and read nothing
    host = stats.to_host()
    assert list(host) == stats.names + ['total'] and host['t3'].grad_norm == t[3, 1] and host['total'].param_absmax == t[-1, 6]
    assert host['total']._fields[3] == 'grad_nonfinite'
    for view, col in ((stats.grad_norm, 1), (stats.grad_absmax, 2), (stats.grad_nonfinite, 3), (stats.param_norm, 5),
                      (stats.param_absmax, 6), (stats.param_nonfinite, 7)):
        assert view.shape == (len(EDGE_NUMELS),) and np.array_equal(view.cpu().numpy(), t[:-1, col])
    assert stats.total_norm.shape == () and float(stats.total_norm) == t[-1, 1] and float(stats.total_nonfinite) == 0.0


# ----------------------------------------------------------------------------------------------
# 2. non-finite values, one placement per case
# ----------------------------------------------------------------------------------------------
# (row, element).  Row 11 has 8195 elements: its gradient is 16-byte aligned (vector loads, the last chunk is a three-element tail), its
# weights are not (element loads).  Row 4 has five: its weights are aligned (one vector and a tail element), its gradient is not.
PLACES = [(11, 0), (11, 8194), (11, 4095), (11, 4096), (11, 8193), (4, 0), (4, 4), (4, 3)]


def planted(edge, row, plants):
    """Run with ``plants`` ({element: value}) written into row ``row`` of BOTH the gradients and the weights; returns the host table and
    the two host arrays as planted.  The device tensors get their values back."""
    from gssd import optim
    g, p = edge.gs[row].copy(), edge.ps[row].copy()
    for e, v in plants.items():
        g[e] = p[e] = v
    try:
        with torch.no_grad():
            edge.params[row].grad.copy_(torch.from_numpy(g))
            edge.params[row].copy_(torch.from_numpy(p))
        t = optim.grad_stats(edge.named()).table.cpu().numpy().copy()
    finally:
        with torch.no_grad():
            edge.params[row].grad.copy_(torch.from_numpy(edge.gs[row].copy()))
            edge.params[row].copy_(torch.from_numpy(edge.ps[row].copy()))
    return t, g, p


def check_planted(edge, row, plants, what):
    t, g, p = planted(edge, row, plants)
    ps, gs = list(edge.ps), list(edge.gs)
    ps[row], gs[row] = p, g
    check_table(t, ps, gs, what)
    n_bad = len(plants)
    assert t[row, 3] == t[row, 7] == t[-1, 3] == t[-1, 7] == n_bad
    keep = np.ones(len(g), bool)
    keep[list(plants)] = False
    assert t[row, 2] == np.abs(edge.gs[row][keep]).max() and t[row, 6] == np.abs(edge.ps[row][keep]).max()      # the FINITE maximum
    others = [i for i in range(len(EDGE_NUMELS)) if i != row]
    assert t[others].tobytes() == edge.clean[others].tobytes(), f'{what}: another row changed'


@pytest.mark.parametrize('row,elem', PLACES)
def test_nonfinite_placement(dev, edge, row, elem):
    assert 0 <= elem < EDGE_NUMELS[row]
    for v in (NAN, INF, -INF):
        check_planted(edge, row, {elem: v}, f'{v} at element {elem} of row {row}')
    # nothing stayed behind
    from gssd import optim
    assert optim.grad_stats(edge.named()).table.cpu().numpy().tobytes() == edge.clean.tobytes()


@pytest.mark.parametrize('row', [11, 4])
def test_nonfinite_all_three(dev, edge, row):
    n = EDGE_NUMELS[row]
    t, g, _ = planted(edge, row, {0: NAN, n // 2: INF, n - 1: -INF})
    check_planted(edge, row, {0: NAN, n // 2: INF, n - 1: -INF}, f'NaN, inf and -inf in row {row}')
    assert np.isnan(t[row, 0]) and np.isnan(t[row, 1]) and np.isnan(t[-1, 1]) and t[row, 3] == 3
    # inf without a NaN stays inf
    t, _, _ = planted(edge, row, {1 % n: -INF})
    assert np.isposinf(t[row, 0]) and np.isposinf(t[row, 1]) and np.isposinf(t[-1, 5])


def test_all_nonfinite_row_has_zero_absmax(dev):
    from gssd import optim
    g = np.array([NAN, INF, -INF, NAN, INF], np.float32)
    s = TensorSet(dev, [np.ones(5, np.float32)], [g])
    t = optim.grad_stats(s.params).table.cpu().numpy()
    check_table(t, s.ps, s.gs, 'all non-finite')
    assert t[0, 2] == 0.0 and t[0, 3] == 5 and t[0, 6] == 1.0 and t[0, 7] == 0


# ----------------------------------------------------------------------------------------------
# 3. shapes of the table
# ----------------------------------------------------------------------------------------------
def test_one_element(dev):
    from gssd import optim
    s = TensorSet(dev, [np.array([-3.0], np.float32)], [np.array([0.5], np.float32)])
    stats = optim.grad_stats(s.params)
    assert stats.names == ['0']
    t = stats.table.cpu().numpy()
    check_table(t, s.ps, s.gs, 'one element')
    assert t.shape == (2, 8) and t[:, (0, 2, 3, 4, 6, 7)].tolist() == [[0.25, 0.5, 0.0, 9.0, 3.0, 0.0]] * 2


def test_three_hundred_items(dev):
    from gssd import optim
    rng = np.random.default_rng(20262)
    numels = rng.integers(1, 9001, 300)
    numels[[17, 211]] = 0
    gs = [rng.standard_normal(n).astype(np.float32) for n in numels]
    ps = [rng.standard_normal(n).astype(np.float32) for n in numels]
    s = TensorSet(dev, ps, gs, list(rng.integers(0, 4, 300)), list(rng.integers(0, 4, 300)))
    stats = optim.grad_stats(s.params)
    t = stats.table.cpu().numpy()
    print('300 items: worst error / bound', check_table(t, ps, gs, '300 items'))
    assert not t[17].any() and not t[211].any() and stats.without_grad == [] and stats.names[299] == '299'


def test_more_chunks_than_sumsq_blocks(dev):
    """One item of 1025 chunks: the fold of a row (and of the totals) strides over more records than the clip's 1024 partial sums."""
    from gssd import _lib, optim
    n = 1025 * optim.CHUNK
    assert _lib.lib.gssd_optim_sumsq_blocks(1025) == 1024 < 1025
    rng = np.random.default_rng(20263)
    g, p = rng.standard_normal(n).astype(np.float32), np.array([2.0, -1.0], np.float32)
    s = TensorSet(dev, [np.zeros(n, np.float32), p], [g, p[::-1].copy()])
    t = optim.grad_stats(s.params).table.cpu().numpy()
    print('1025 chunks: worst error / bound', check_table(t, s.ps, s.gs, '1025 chunks'))
    assert t[0, 2] == np.abs(g).max() and t[0, 4] == 0.0 and t[-1, 4] == 5.0


def test_params_false_and_missing_gradient(dev):
    from gssd import optim
    ps, gs = edge_host()
    gs = list(gs)
    gs[2] = gs[9] = None
    s = TensorSet(dev, ps, gs, [i % 4 for i in range(len(ps))], [(i + 2) % 4 for i in range(len(ps))])
    assert s.params[2].grad is None and s.params[9].grad is None
    stats = optim.grad_stats(s.named())
    assert stats.without_grad == ['t2', 't9']
    t = stats.table.cpu().numpy().copy()
    check_table(t, ps, gs, 'two tensors without a gradient')
    assert not t[2, 0:4].any() and not t[9, 0:4].any() and t[2, 5] > 0 and t[9, 5] > 0
    stats = optim.grad_stats(s.named(), params=False)
    t2 = stats.table.cpu().numpy()
    check_table(t2, [None] * len(ps), gs, 'params=False')
    assert not t2[:, 4:8].any() and t2[:, 0:4].tobytes() == t[:, 0:4].tobytes() and stats.without_grad == ['t2', 't9']
    assert not t2[2].any()                              # neither side read: a row of zeros


# ----------------------------------------------------------------------------------------------
# 4. determinism, no read-back
# ----------------------------------------------------------------------------------------------
def test_bit_identical_and_reads_nothing_back(dev, edge):
    from gssd import optim
    a = optim.grad_stats(edge.named()).table.clone()
    b = optim.grad_stats(edge.named()).table.clone()
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == edge.clean.tobytes()
    mon = optim.GradMonitor(edge.named(), history=2)
    mon.record()                                        # the ring is allocated (and zero-filled) at the first record
    torch.cuda.set_sync_debug_mode('error')
    try:
        stats = optim.grad_stats(edge.named())
        mon.record()
        mon.record()
        views = stats.grad_norm, stats.total_norm, stats.param_nonfinite
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert stats.table.cpu().numpy().tobytes() == edge.clean.tobytes() and views[1].shape == ()
    steps, tables = mon.flush()
    assert steps.tolist() == [1, 2] and tables[0].tobytes() == tables[1].tobytes() == edge.clean.tobytes()


# ----------------------------------------------------------------------------------------------
# 5. the cached table
# ----------------------------------------------------------------------------------------------
def test_cache_follows_the_gradients_and_out(dev):
    from gssd import grad_stats as gs_mod, optim
    ps, gs = edge_host()
    s = edge_set(dev)
    first = optim.grad_stats(s.named())
    table = next(reversed(gs_mod._TABLES.values()))
    assert first.table is table.out
    optim.grad_stats(s.named())
    assert next(reversed(gs_mod._TABLES.values())) is table                     # same tensors: same table
    # one gradient moves to new storage with new values, another goes away
    gs = list(gs)
    gs[10] = (gs[10] * np.float32(3.0)).astype(np.float32)
    s.params[10].grad = torch.from_numpy(gs[10]).to(dev)
    s.params[5].grad = None
    gs[5] = None
    stats = optim.grad_stats(s.named())
    assert next(reversed(gs_mod._TABLES.values())) is not table and stats.without_grad == ['t5']
    owned = stats.table
    t = owned.cpu().numpy().copy()
    check_table(t, ps, gs, 'after the gradients changed')
    # out= writes where asked and leaves the owned buffer alone
    owned.fill_(-7.0)
    out = torch.full((len(ps) + 1, 8), -1.0, device=dev, dtype=torch.float64)
    stats = optim.grad_stats(s.named(), out=out)
    assert stats.table is out and out.cpu().numpy().tobytes() == t.tobytes() and bool((owned == -7.0).all())
    from gssd._lib import GssdError
    for bad in (torch.zeros(len(ps), 8, device=dev, dtype=torch.float64), torch.zeros(len(ps) + 1, 8, device=dev),
                torch.zeros(len(ps) + 1, 8, dtype=torch.float64)):
        with pytest.raises(GssdError):
            optim.grad_stats(s.named(), out=bad)
    # worst(): rows with non-finite gradients first, then by magnitude
    with torch.no_grad():
        s.params[3].grad[1] = NAN
        s.params[7].grad[0:2] = INF
    w = optim.grad_stats(s.named()).worst(3)
    assert [n for n, _ in w] == ['t7', 't3', 't11'] and w[0][1].grad_nonfinite == 2 and w[1][1].grad_nonfinite == 1


# ----------------------------------------------------------------------------------------------
# 6. agreement with the fused clip
# ----------------------------------------------------------------------------------------------
def test_total_norm_agrees_with_the_fused_clip(dev):
    from gssd import optim
    s = edge_set(dev)
    opt = optim.SGD(s.params, lr=0.0, max_grad_norm=1.0)
    opt.step()
    ours = np.float32(float(optim.grad_stats(s.named()).total_norm))
    theirs = np.float32(float(opt.grad_norm))
    print(f'total norm: fused clip {theirs!r}, grad_stats rounded to fp32 {ours!r}')
    assert np.isfinite(ours) and ours > 0
    assert abs(int(ours.view(np.int32)) - int(theirs.view(np.int32))) <= 1


# ----------------------------------------------------------------------------------------------
# 7. check_grad_norm on the engine's own gradients
# ----------------------------------------------------------------------------------------------
def test_check_grad_norm_on_the_engine(dev):
    from gssd import optim
    from layers.modules import MultiBoxLoss
    from models.ssd_multiphase_custom_group import build_ssd
    from utils.check_grad_norm import check_grad_norm
    net = build_ssd('train', 300, 2, *NETS['gssd'][1])
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    x = synth.synth_images(2, seed=21).to(dev)
    tg = [t.to(dev) for t in synth.synth_targets(2, seed=21)]
    ll, lc = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)(net(x), tg)
    (ll + lc).backward()
    names = [n for n, _ in net.named_parameters()]
    missing = [n for n, p in net.named_parameters() if p.grad is None]
    assert not missing, missing
    got = check_grad_norm(net)
    assert type(got) is float
    grads = [p.grad.cpu().numpy() for p in net.parameters()]
    n = sum(g.size for g in grads)
    want = math.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in grads))
    print(f'check_grad_norm {got!r}, float64 {want!r}: off by {abs(got - want) / want:.3g} relative, bound {(n + 1) * EPS:.3g} ({n} elements)')
    assert want > 0 and abs(got - want) <= (n + 1) * EPS * want
    stats = optim.grad_stats(net)
    host = stats.to_host()
    assert list(host) == names + ['total'] and len(names) == len(set(names))
    assert host['total'].grad_norm == got and host['total'].grad_nonfinite == 0 and host['total'].param_norm > 0
    i = max(range(len(grads)), key=lambda k: grads[k].size)
    check_cols(stats.table[i, 0:4].cpu().numpy(), grads[i], 'the largest gradient')
    p = net.get_parameter(names[3])
    p.grad = None
    with pytest.raises(AttributeError, match=names[3].replace('.', r'\.')):
        check_grad_norm(net)


# ----------------------------------------------------------------------------------------------
# 8. GradMonitor
# ----------------------------------------------------------------------------------------------
def test_monitor_ring(dev):
    from gssd import optim
    numels = [3, 4097, 0, 260]
    s = TensorSet(dev, [np.full(n, 2.0, np.float32) for n in numels], [np.zeros(n, np.float32) for n in numels], [1, 2, 0, 3], [3, 0, 0, 1])
    mon = optim.GradMonitor(s.named(), history=3)
    for step in range(5):
        for p in s.params:
            p.grad.fill_(float(step))
        got = mon.record()
        assert got.table.data_ptr() == mon.buffer[step % 3].data_ptr()
    steps, tables = mon.flush()
    assert steps.dtype == np.int64 and steps.tolist() == [2, 3, 4] and tables.shape == (3, 5, 8) and tables.dtype == np.float64
    for step, t in zip(steps, tables):
        check_table(t, s.ps, [np.full(n, float(step), np.float32) for n in numels], f'record {step}')
        assert t[:, 0].tolist() == [float(n) * step * step for n in numels + [sum(numels)]]        # small integers: exact
        assert t[:, 2].tolist() == [float(step) if n else 0.0 for n in numels] + [float(step)]
        assert t[:, 4].tolist() == [4.0 * n for n in numels + [sum(numels)]]
    steps, tables = mon.flush()
    assert steps.shape == (0,) and tables.shape == (0, 5, 8)
    for p in s.params:
        p.grad.fill_(9.0)
    mon.record()
    steps, tables = mon.flush()
    assert steps.tolist() == [5] and tables[0, 1, 2] == 9.0 and mon.n == 6
