"""GPU tests of gssd.optim.GradAccumulator (csrc/optim_accum.hip): the weighted mean / sum of micro-batch gradients, one launch per
micro-batch, against float64.

The parameter set is that of tests/test_gpu_optim.py (numels [1, 3, 4, 5, 63, 64, 65, CH-1, CH, CH+1, 3*CH+7, 0], gradients as slices of
ONE flat tensor laid end to end, so that most of them sit at a 4-byte but not 16-byte aligned address and take the element path, one
parameter without a gradient, one frozen) with four tensors appended (tests/grad_accum_cases.py: 2 CH + 3 and 257 CH + 1 elements, and
two small ones whose gradient is missing in the first / in the last micro-batch).  Every micro-batch has a flat gradient vector of
its own, generated once and never modified.

Yardstick: tests/grad_accum_cases.py holds the float64 model and the bound, derived there rounding by rounding; its exact rows
(integer gradients, weights 1, 2, 1) must match bit for bit.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, rel, TOL, NETS)
from gpu_common import synth                  # noqa: E402
import grad_accum_cases as GC                 # noqa: E402
import optim_lars_common as LC                # noqa: E402
import test_gpu_optim as TS                   # noqa: E402  (the SGD tests: their parameter set and bound, unchanged)
from test_gpu_optim import ParamSet, chunk    # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _host_flats(ch, exact):
    """K_MAX flat gradient vectors over the whole set (base set, then the appended tensors): generated once, never modified."""
    total = sum(p.numel() for p in ParamSet('cpu', ch).params) + sum(GC.numels(ch))
    return [torch.from_numpy(g) for g in GC.host_grads(total, exact)]


_DEVICE_FLATS = {}


def device_flats(dev, exact):
    key = (str(dev), chunk(), exact)
    if key not in _DEVICE_FLATS:
        _DEVICE_FLATS[key] = [g.to(dev) for g in _host_flats(chunk(), exact)]
    return _DEVICE_FLATS[key]


class AccumSet(ParamSet):
    """ParamSet with the tensors of GC.numels() appended; self.with_grad are the parameters that can get a gradient, in flat order."""

    def __init__(self, device, exact=False):
        super().__init__(device)
        rng = np.random.default_rng(GC.SEED + 7)
        self.extra = [torch.nn.Parameter(torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(device)) for n in GC.numels(chunk())]
        self.with_grad = self.params + self.extra
        self.all = self.with_grad + [self.nograd, self.frozen]
        for p in self.all:
            p.grad = None
        self.flats = device_flats(device, exact)
        self.offs = np.concatenate([[0], np.cumsum([p.numel() for p in self.with_grad])])

    def grad_of(self, j, i):
        """The gradient of with_grad[i] in micro-batch j: a slice of that micro-batch's flat vector."""
        p = self.with_grad[i]
        return self.flats[j][int(self.offs[i]):int(self.offs[i + 1])].view(p.shape)

    def backward(self, j, present):
        for i, p in enumerate(self.with_grad):
            p.grad = self.grad_of(j, i) if present[i] else None


def as_weight(kind, w, dev):
    if kind == 'none':
        assert w == 1.0
        return None
    if kind == 'float':
        return w
    return torch.tensor([w], dtype=torch.float64 if kind == 'f64' else torch.float32, device=dev)


def run_cycle(acc, ps, row, last):
    """One cycle of ``row``: k times backward + add, then finish().  Returns the per-parameter gradient lists the model takes."""
    k, kind, weights, _, _ = row
    pres = GC.present(k, len(ps.with_grad))
    for j in range(k):
        ps.backward(j, pres[j])
        acc.add(weight=as_weight(kind, weights[j], ps.flats[0].device), last=last and j == k - 1)
        assert all(p.grad is None for p in ps.all), 'every consumed gradient is set to None'
    acc.finish()
    return [[ps.grad_of(j, i) if pres[j][i] else None for j in range(k)] for i in range(len(ps.with_grad))]


@pytest.mark.parametrize('row', GC.ROWS, ids=GC.ROW_IDS)
def test_rows_match_float64(dev, row):
    from gssd import optim
    k, kind, weights, average, exact = row
    assert chunk() == 4096 or chunk() > 8
    res = {}
    worst = 0.0
    for last in (False, True):
        ps = AccumSet(dev, exact)
        keep_flats = [f.clone() for f in ps.flats[:k]]
        keep_params = [p.detach().clone() for p in ps.all]
        acc = optim.GradAccumulator(ps.all, average=average)
        grads = run_cycle(acc, ps, row, last)
        assert acc.launches == k + (1 if average and not last else 0), (acc.launches, k, last)
        assert all(torch.equal(a, b) for a, b in zip(ps.flats[:k], keep_flats)), 'the sources are only read'
        assert all(torch.equal(p.detach(), q) for p, q in zip(ps.all, keep_params)), 'the parameters are not touched'
        assert ps.nograd.grad is None and ps.frozen.grad is None
        out = []
        for i, (p, gs) in enumerate(zip(ps.with_grad, grads)):
            if all(g is None for g in gs):
                assert p.grad is None, f'parameter {i} never had a gradient'
                out.append(None)
                continue
            assert p.grad is not None and p.grad.shape == p.shape
            worst = max(worst, GC.check(p.grad, gs, weights, average, exact, f'{GC.ROW_IDS[GC.ROWS.index(row)]} last={last} param {i}'))
            out.append(p.grad.clone())
        assert acc.weight_sum.dtype == torch.float64 and acc.weight_sum.shape == (1,)
        assert float(acc.weight_sum) == GC.weight_sum64(weights)
        res[last] = out
    for a, b in zip(res[False], res[True]):
        assert (a is None and b is None) or torch.equal(a, b), 'last=True and finish() give the same bits'
    print(f'{GC.ROW_IDS[GC.ROWS.index(row)]}: worst error / bound {worst:.3f}')


def test_views_are_stable_slices_of_one_flat_tensor(dev):
    """After finish() every gradient has its parameter's shape, is 16-byte aligned and shares ONE 1-D base; the same tensors at the same
    addresses come back in every cycle, each cycle restarts the weight sum, and the launches add up."""
    from gssd import optim
    ps = AccumSet(dev)
    acc = optim.GradAccumulator([dict(params=ps.all[0::2]), dict(params=ps.all[1::2], lr=0.1)])
    assert len(acc.params) == len(ps.all)
    ptrs, base = None, None
    for cycle, i in enumerate((5, 9, 13)):
        row = GC.ROWS[i]
        assert row[3], 'rows with the division'
        grads = run_cycle(acc, ps, row, last=bool(cycle % 2))
        got = [p.grad for p in ps.with_grad if p.grad is not None]
        assert len(got) >= len(ps.with_grad) - 1
        for p in ps.with_grad:
            if p.grad is None:
                continue
            assert p.grad.shape == p.shape and p.grad.dtype == torch.float32 and p.grad.is_contiguous()
            assert p.grad.data_ptr() % 16 == 0 or p.numel() == 0
            assert p.grad._base is not None and p.grad._base.dim() == 1
            base = base if base is not None else p.grad._base
            assert p.grad._base is base
        now = [p.grad.data_ptr() for p in ps.with_grad[:-2]]
        assert ptrs is None or now == ptrs, 'the data pointers are the same in every cycle'
        ptrs = now
        for i2, (p, gs) in enumerate(zip(ps.with_grad, grads)):
            if p.grad is not None:
                GC.check(p.grad, gs, row[2], True, False, f'cycle {cycle} param {i2}')
        assert float(acc.weight_sum) == GC.weight_sum64(row[2]), 'the weight sum restarts with the cycle'
        for p in ps.all:                                        # optimizer.zero_grad()
            p.grad = None
    assert acc.launches == (2 + 1) + 3 + (8 + 1)


def test_deterministic(dev):
    from gssd import optim
    row = GC.ROWS[12]                                           # k = 8, Python-float weights that fp32 cannot hold
    res = []
    for _ in range(2):
        ps = AccumSet(dev)
        acc = optim.GradAccumulator(ps.all)
        run_cycle(acc, ps, row, last=False)
        res.append([p.grad.clone() for p in ps.with_grad] + [acc.weight_sum.clone()])
    assert len(res[0]) == len(res[1]) > 10 and all(torch.equal(a, b) for a, b in zip(res[0], res[1]))


def _same_sign_backward(ps, j):
    """Gradients for the optimizer test: micro-batch 0 is the base set's own flat gradient, micro-batch 1 has the same signs and other
    magnitudes (|g| rolled by one element)."""
    g0 = TS._host_data(chunk())[1].to(ps.flat.device)
    flat = g0 if j == 0 else torch.sign(g0) * g0.roll(1).abs()
    o = 0
    for p in ps.params:
        p.grad = flat[o:o + p.numel()].clone().view(p.shape) if p.numel() else flat[o:o].clone()
        o += p.numel()
    return flat


@pytest.mark.parametrize('algo', ['sgd', 'lamb'])
def test_step_after_finish(dev, algo):
    """SGD(max_grad_norm=...) and LAMB after finish(): the step is held, with those optimizers' own bounds (tests/test_gpu_optim.py,
    tests/optim_lars_common.py), against the same step taken from the FLOAT64 weighted mean of the two micro-batch gradients.

    The optimizers' bounds are relative to the gradient they are given (2^-21 of |c g| and the like), the accumulator's error to
    sum |w_j g_j| / W.  The two measure the same thing where the micro-batch gradients of an element have one sign, so the gradients
    here do: then the accumulated gradient is within (k + 2) 2^-24 = 2^-22 of the mean, relative, which is inside what either bound
    leaves for the gradient (2^-21 |c g| less three roundings; 2^-23 |c g| per moment plus 2^-22 (|m| + |c g|))."""
    from gssd import optim
    weights = [37.0, 5.0]                                       # counts: exact in fp32
    ps = ParamSet(dev)
    for p in ps.all:
        p.grad = None
    if algo == 'sgd':
        clip = 1.0
        opt = optim.SGD(ps.groups(1e-2), lr=1e-2, momentum=0.9, weight_decay=5e-4, max_grad_norm=clip)
    else:
        clip = None
        opt = optim.LAMB(ps.groups(1e-3), lr=1e-3, weight_decay=0.01)
    acc = optim.GradAccumulator(opt.param_groups)
    for step in range(2):                                       # the second step: momentum / moments in play, the accumulators reused
        flats = []
        for j in range(2):
            flats.append(_same_sign_backward(ps, j) * (1.0 if step == 0 else -0.5))
            if step:
                for p in ps.params:
                    p.grad.mul_(-0.5)
            acc.add(weight=torch.tensor([weights[j]], dtype=torch.float64, device=dev), last=j == 1)
        acc.finish()
        mean = (weights[0] * flats[0].double() + weights[1] * flats[1].double()) / sum(weights)
        o, mean_of = 0, {}
        for p in ps.params:
            mean_of[p] = mean[o:o + p.numel()].view(p.shape)
            o += p.numel()
            GC.check(p.grad, [flats[0][o - p.numel():o].view(p.shape), flats[1][o - p.numel():o].view(p.shape)], weights, True, False)
        c = 1.0 if clip is None else min(1.0, clip / (float(mean.pow(2).sum().sqrt()) + 1e-6))
        if algo == 'sgd':
            snap = [(p, g, p0, None if g0 is None else mean_of[p], b0) for p, g, p0, g0, b0 in TS.snapshot(opt)]
            opt.step()
            worst = TS.check_step(opt, snap, c, True, f'SGD after finish(), step {step}')
        else:
            snap = [(p, g, p0, None if g0 is None else mean_of[p], s0, n0) for p, g, p0, g0, s0, n0 in LC.snapshot('lamb', opt)]
            opt.step()
            worst, _ = LC.check_step('lamb', opt, snap, c, False, f'LAMB after finish(), step {step}')
        print(f'{algo} step {step}: worst error / bound {worst:.3f}')
        assert ps.nograd.grad is None
        opt.zero_grad()
    assert acc.launches == 4


def test_misuse(dev):
    from gssd import optim
    from gssd._lib import GssdError
    ps = AccumSet(dev)
    acc = optim.GradAccumulator(ps.all)
    pres = [True] * len(ps.with_grad)
    keep_params = [p.detach().clone() for p in ps.all]

    def unchanged(grads):
        assert all(torch.equal(p.detach(), q) for p, q in zip(ps.all, keep_params))
        assert all((p.grad is None and g is None) or p.grad is g for p, g in zip(ps.all, grads))
        assert torch.equal(ps.flats[0], _host_flats(chunk(), False)[0].to(dev))

    with pytest.raises(GssdError, match='backward'):            # no parameter has a gradient
        acc.add()
    with pytest.raises(GssdError, match='add\\(\\)'):           # finish() with no add() in the cycle
        acc.finish()
    ps.backward(0, pres)
    grads = [p.grad for p in ps.all]
    for bad in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='weight'):
            acc.add(weight=bad)
    for bad in (torch.ones(1), torch.ones(2, device=dev), torch.ones(1, device=dev, dtype=torch.float16),
                torch.ones(1, device=dev, dtype=torch.int64), '1', [1.0]):
        with pytest.raises(GssdError, match='weight'):
            acc.add(weight=bad)
    p = ps.with_grad[5]
    p.grad = None
    p.grad = torch.ones(128, device=dev)[::2]                                                  # not contiguous
    with pytest.raises(GssdError, match='parameter 5.*contiguous'):
        acc.add()
    p.grad = grads[5]
    unchanged(grads)
    assert acc.launches == 0
    # a cycle, then a backward without zero_grad(): autograd sums into the accumulator's own view
    acc.add(weight=2.0)
    acc.finish()
    own = [p.grad for p in ps.all]
    result = [None if g is None else g.clone() for g in own]
    with pytest.raises(GssdError, match='zero_grad'):
        acc.add()
    assert all((p.grad is None and g is None) or p.grad is g for p, g in zip(ps.all, own))
    assert all(g is None or torch.equal(g, r) for g, r in zip(own, result)) and acc.launches == 2
    # add(last=True) closes the cycle
    ps.backward(0, pres)
    acc.add(last=True)
    ps.backward(1, pres)
    with pytest.raises(GssdError, match='finish'):
        acc.add()
    acc.finish()
    # parameters on two devices
    with pytest.raises(GssdError, match='one accumulator per device'):
        optim.GradAccumulator([ps.params[0], torch.nn.Parameter(torch.ones(3))])


def test_on_the_engine(dev):
    """Two micro-batches of B = 2 through GSSD with N-weights: the second backward hands its slices of the plan's flat buffer out directly
    (no clone, no add_), num_pos is the number of matched priors, the accumulated gradient is (N1 g1 + N2 g2) / (N1 + N2) within the
    bound, and an SGD step on it makes the next forward run on new weights."""
    from gssd import optim, ops
    from layers.modules import MultiBoxLoss
    from models.ssd_multiphase_custom_group import build_ssd
    flags, args = NETS['gssd']
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    assert crit.num_pos is None
    params = list(net.parameters())
    acc = optim.GradAccumulator(params)
    opt = optim.SGD(params, lr=1e-2, momentum=0.9, weight_decay=5e-4)
    x0 = synth.synth_images(2, seed=21).to(dev)

    def eval_out():
        net.eval()
        with torch.no_grad():
            loc, conf, _ = net(x0)
        net.train()
        return loc.clone(), conf.clone()
    before = eval_out()
    g64, counts, bases = [], [], []
    for j, seed in enumerate((21, 22)):
        x = synth.synth_images(2, seed=seed).to(dev)
        tg = [t.to(dev) for t in synth.synth_targets(2, seed=seed)]
        out = net(x)
        ll, lc = crit(out, tg)
        (ll + lc).backward()
        n = crit.num_pos
        assert n.dtype == torch.float64 and n.shape == (1,) and n.device == x.device
        packed, off = ops.pack_targets(tg, dev)
        _, conf_t = ops.match_batch(packed, off, out[2][:out[0].size(1)].detach().to(dev).contiguous(), 0.5, (0.1, 0.2))
        counts.append(float(n))
        assert counts[-1] == float((conf_t > 0).sum()) > 0, 'num_pos is the number of matched priors'
        with_grad = [p for p in params if p.grad is not None]
        assert len(with_grad) > 50
        base = with_grad[0].grad._base
        assert base is not None and base.dim() == 1 and all(p.grad._base is base for p in with_grad), \
            'the gradients are the slices of the plan\'s flat tensor: the clone / add_ path did not run'
        bases.append(base)
        g64.append([None if p.grad is None else p.grad.double() for p in params])
        acc.add(weight=n)
        assert all(p.grad is None for p in params)
    assert bases[0] is bases[1] or bases[0].data_ptr() == bases[1].data_ptr()
    assert counts[0] != counts[1], 'two micro-batches with different normalisers'
    acc.finish()
    assert acc.launches == 3
    worst = 0.0
    for i, p in enumerate(params):
        gs = [None if g[i] is None else g[i].float() for g in g64]
        if all(g is None for g in gs):
            assert p.grad is None
            continue
        worst = max(worst, GC.check(p.grad, gs, counts, True, False, f'GSSD parameter {i} {tuple(p.shape)}'))
    print(f'N = {counts}, worst error / bound {worst:.3f}')
    assert float(acc.weight_sum) == sum(counts)
    opt.step()
    opt.zero_grad()
    after = eval_out()
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]), 'the forward ran on stale packed weights'
