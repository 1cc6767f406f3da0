"""Host logic of gssd.optim.GradAccumulator that needs no GPU: the ABI wiring of gssd_grad_accumulate_f32 and the layout of its item
struct, the launcher's refusals, the launch plan (which items are FIRST, which scale-only, which skipped) and its chunk list as pure
functions, the float64 model of tests/grad_accum_cases.py against a plain numpy restatement, and the bound of that module shown to hold
for an fp32 restatement of the rule and to REJECT three wrong results."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_accum_cases as GC                                   # noqa: E402
from test_optim_avg_cpu import HEADER, header_struct            # noqa: E402

CH = 16                                                         # the stand-in chunk size of the pure-function tests


def test_abi_carries_the_accumulate_entry_point():
    from gssd import _lib
    hdr = open(HEADER).read()
    n = 'gssd_grad_accumulate_f32'
    assert re.search(r'\bint\s+' + n + r'\s*\(', hdr) and n in _lib.SIGNATURES
    i = _lib.lib.gssd_plan_fn_index(n.encode())
    assert i >= 0 and _lib.lib.gssd_plan_fn_nargs(i) == len(_lib.SIGNATURES[n][1]) - 1 == 8
    decl = re.search(n + r'\s*\((.*?)\)\s*;', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S), flags=re.S).group(1)
    assert len(decl.split(',')) == len(_lib.SIGNATURES[n][1])
    assert _lib.lib.gssd_abi_version() == 8                    # additive, as the earlier optimizer entries were


def test_launcher_refuses_before_touching_a_device():
    from gssd import _lib, optim
    one = ctypes.c_void_p(16)                                   # never dereferenced: every call below is refused
    f = _lib.lib.gssd_grad_accumulate_f32
    for args in ((None, one, 1, 1.0, None, 0, one, one),        # no item table
                 (one, None, 1, 1.0, None, 0, one, one),        # no chunk list
                 (one, one, 0, 1.0, None, 0, one, one),         # no work
                 (one, one, -3, 1.0, None, 0, one, one),
                 (one, one, 1, -1.0, None, 0, one, one),        # a negative by-value weight
                 (one, one, 1, -1e-300, None, optim.ACCUM_FINALIZE, one, one),
                 (one, one, 1, float('nan'), None, 0, one, one),
                 (one, one, 1, 1.0, None, 0, None, one),        # no weight sum
                 (one, one, 1, 1.0, None, 0, one, None),        # no ticket word
                 (one, one, 1, 1.0, None, 8, one, one)):        # an unknown flag
        assert f(*args, None) == -1 and b'invalid argument' in _lib.lib.gssd_last_error(), args


def test_struct_layout_and_flags_agree():
    from gssd import optim, optim_table
    item, size = header_struct('gssd_accum_item')
    dt = optim_table._ACCUM_ITEM
    assert [n for n, _ in item] == ['dst', 'src', 'n', 'flags', 'reserved']
    assert size == dt.itemsize == 32 and item == [(n, dt.fields[n][1]) for n in dt.names]
    # gssd_avg_item's layout with `flags` where it has `kind`
    assert [(dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == \
        [(optim._AVG_ITEM.fields[n][1], optim._AVG_ITEM.fields[n][0].itemsize) for n in optim._AVG_ITEM.names]
    hdr = open(HEADER).read()
    for name, v in (('FIRST', optim.ACCUM_FIRST), ('W_F32', optim.ACCUM_W_F32), ('RESET', optim.ACCUM_RESET),
                    ('FINALIZE', optim.ACCUM_FINALIZE)):
        assert int(re.search(r'#define\s+GSSD_ACCUM_' + name + r'\s+(\d+)', hdr).group(1)) == v
    assert optim.ACCUM_FIRST == 1                               # flag bit 0 of an item


def test_launch_plan_of_a_mixed_set():
    from gssd.optim_table import ACCUM_ADD, ACCUM_FIRST, ACCUM_SCALE, accum_plan, build_chunks
    ns = GC.cpu_numels(CH)
    n = len(ns)
    empty = ns.index(0)
    pres = GC.present(3, n)
    seen = [False] * n
    # micro-batch 1: everything that has a gradient is FIRST; the empty parameter and the late one are not in the launch
    plan = accum_plan(ns, pres[0], seen, False)
    assert [i for i, _ in plan] == [i for i in range(n) if i not in (empty, n + GC.LATE)]
    assert all(kind == ACCUM_FIRST for _, kind in plan)
    seen = [s or p for s, p in zip(seen, pres[0])]
    # micro-batch 2: the late parameter is FIRST now, all others add
    plan = dict(accum_plan(ns, pres[1], seen, False))
    assert plan.pop(n + GC.LATE) == ACCUM_FIRST and empty not in plan and len(plan) == n - 2
    assert all(kind == ACCUM_ADD for kind in plan.values())
    seen = [s or p for s, p in zip(seen, pres[1])]
    # micro-batch 3 without the division: the early parameter brings nothing and is left out ...
    plan = dict(accum_plan(ns, pres[2], seen, False))
    assert n + GC.EARLY not in plan and empty not in plan and all(kind == ACCUM_ADD for kind in plan.values()) and len(plan) == n - 2
    # ... with the division it takes part scale-only
    plan = dict(accum_plan(ns, pres[2], seen, True))
    assert plan.pop(n + GC.EARLY) == ACCUM_SCALE and all(kind == ACCUM_ADD for kind in plan.values()) and len(plan) == n - 2
    # finish(): every seen parameter scale-only; one never seen stays out
    assert accum_plan(ns, [False] * n, seen, True) == [(i, ACCUM_SCALE) for i in range(n) if i != empty]
    assert accum_plan(ns, [False] * n, [False] * n, True) == [] and accum_plan(ns, [False] * n, seen, False) == []
    # the chunk list of such a plan: every element in exactly one chunk, no chunk across two items, partial chunks at the tails
    rows = [ns[i] for i, _ in accum_plan(ns, pres[1], seen, False)]
    item, off = build_chunks(rows, CH)
    covered = [np.zeros(m, np.int32) for m in rows]
    for it, o in zip(item, off):
        assert o % CH == 0 and o < rows[it]
        covered[it][o:min(o + CH, rows[it])] += 1
    assert all((c == 1).all() for c in covered) and len(item) == sum(-(-m // CH) for m in rows)


def _cpu_cycle(k, exact):
    ns = GC.cpu_numels(CH)
    flats = GC.host_grads(sum(ns), exact)
    offs = np.concatenate([[0], np.cumsum(ns)])
    pres = GC.present(k, len(ns))
    return ns, [[flats[j][offs[i]:offs[i + 1]] if pres[j][i] else None for j in range(k)] for i in range(len(ns))]


@pytest.mark.parametrize('row', GC.ROWS, ids=GC.ROW_IDS)
def test_model_agrees_with_numpy_and_the_bound_holds_for_fp32(row):
    k, _, weights, average, exact = row
    ns, grads = _cpu_cycle(k, exact)
    worst = 0.0
    for i, gs in enumerate(grads):
        m = GC.model64([None if g is None else torch.from_numpy(g) for g in gs], weights, average)
        if all(g is None for g in gs):
            assert m is None and GC.restate32(gs, weights, average) is None
            continue
        # numpy, written the plain way: a weighted sum over what arrived, divided by the sum of ALL weights
        num = np.zeros(ns[i], np.float64)
        mag = np.zeros(ns[i], np.float64)
        for w, g in zip(weights, gs):
            if g is not None:
                num += np.float64(w) * g.astype(np.float64)
                mag += abs(np.float64(w)) * np.abs(g.astype(np.float64))
        den = float(np.sum(np.asarray(weights, np.float64))) if average else 1.0
        assert np.allclose(m[0].numpy(), num / den, rtol=1e-14, atol=0) and np.allclose(m[1].numpy(), mag / den, rtol=1e-14, atol=0)
        assert m[2] == sum(g is not None for g in gs)
        got = torch.from_numpy(GC.restate32(gs, weights, average))
        worst = max(worst, GC.check(got, [None if g is None else torch.from_numpy(g) for g in gs], weights, average, exact, f'param {i}'))
    assert exact or k == 1 and not GC.inexact(weights) or worst > 0.0
    assert worst <= 1.0
    assert GC.weight_sum64(weights) == sum(float(np.float32(w)) for w in weights)


def test_the_bound_is_not_vacuous():
    """A result (i) whose last element of a partial chunk missed the last micro-batch, (ii) divided by k in place of the weight sum,
    (iii) with two micro-batches' weights swapped, is rejected -- for the count weights of the loss and for k = 2, 3 and 8."""
    for k, weights in ((2, GC._COUNTS[:2]), (3, GC._COUNTS[:3]), (8, GC._COUNTS), (3, GC._FRACS[:3])):
        ns, grads = _cpu_cycle(k, False)
        i = ns.index(CH + 1)                                   # one full chunk and a partial one of a single element
        gs = grads[i]
        tg = [torch.from_numpy(g) for g in gs]
        good = GC.restate32(gs, weights, True)
        GC.check(torch.from_numpy(good), tg, weights, True, False)
        inv = np.float32(1.0 / GC.weight_sum64(weights))
        tail = good.copy()                                      # (i)
        tail[-1] = GC.restate32([g[-1:] for g in gs[:-1]] + [None], weights, True)[0]
        with pytest.raises(AssertionError, match='err/bound'):
            GC.check(torch.from_numpy(tail), tg, weights, True, False)
        assert np.array_equal(tail[:-1], good[:-1])
        by_k = (GC.restate32(gs, weights, False) * np.float32(1.0 / k)).astype(np.float32)      # (ii)
        with pytest.raises(AssertionError, match='err/bound'):
            GC.check(torch.from_numpy(by_k), tg, weights, True, False)
        swapped = list(weights)                                 # (iii)
        swapped[0], swapped[1] = swapped[1], swapped[0]
        with pytest.raises(AssertionError, match='err/bound'):
            GC.check(torch.from_numpy(GC.restate32(gs, swapped, True)), tg, weights, True, False)
        assert inv > 0
    # an exact row rejects a single flipped bit
    ns, grads = _cpu_cycle(3, True)
    gs = grads[ns.index(CH + 1)]
    tg = [torch.from_numpy(g) for g in gs]
    good = GC.restate32(gs, [1.0, 2.0, 1.0], True)
    GC.check(torch.from_numpy(good), tg, [1.0, 2.0, 1.0], True, True)
    bad = good.copy()
    bad[3] = np.nextafter(bad[3], np.float32(1e9))
    with pytest.raises(AssertionError, match='bit for bit'):
        GC.check(torch.from_numpy(bad), tg, [1.0, 2.0, 1.0], True, True)


def test_constructor_and_weights_without_a_device():
    from gssd import optim
    from gssd._lib import GssdError
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    acc = optim.GradAccumulator(ps)
    assert acc.average is True and acc.launches == 0 and acc.params == ps
    assert optim.GradAccumulator([dict(params=ps[:1]), dict(params=ps[1:] + ps[:1], lr=0.1)], average=False).params == ps
    with pytest.raises(ValueError):
        optim.GradAccumulator([])
    for p in ps:
        p.grad = torch.ones_like(p)
    for bad in (-1.0, float('nan'), float('inf'), -0.5):
        with pytest.raises(ValueError, match='weight'):
            acc.add(weight=bad)
    for bad in ('1', [1.0], torch.ones(1), torch.ones(2)):
        with pytest.raises(GssdError, match='weight'):
            acc.add(weight=bad)
    with pytest.raises(GssdError, match='no CPU fallback'):        # CPU parameters: refused, nothing consumed
        acc.add()
    assert all(torch.equal(p.grad, torch.ones_like(p)) for p in ps) and acc.launches == 0
    with pytest.raises(GssdError, match='add\\(\\)'):
        acc.finish()
    for p in ps:
        p.grad = None
    with pytest.raises(GssdError, match='backward'):
        acc.add()
