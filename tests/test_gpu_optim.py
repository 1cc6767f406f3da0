"""GPU tests of gssd.optim (csrc/optim.hip): the fused clip_grad_norm_ + SGD step and the stand-alone clip, against float64.

Synthetic parameter set: numels [1, 3, 4, 5, 63, 64, 65, CH-1, CH, CH+1, 3*CH+7, 0] (CH = the kernels' chunk size), values
randn * 10^U(-3, 1), gradients randn * 10^U(-4, 1) as slices of ONE flat tensor laid end to end (so both the 16-byte vector path and
the element-wise path run, with full chunks, short chunks and tails), one more parameter without a gradient, one frozen, two param
groups with the second at lr * 0.1.

Yardstick (teacher-forced: the expected values are computed in float64 from the device's own fp32 p, buf, g before the step), with
S = |c g| + wd |p| + momentum |buf|:
    |buf - buf64| <= buf_tol = 2^-21 S (+ 4e-6 |c g| when clipping: the 1e-6 allowed on the norm)
    |p - p64|     <= 2^-23 |p64| + lr (2 buf_tol + 2^-22 (S + |buf64|)) + 1e-38
Each of the three fp32 operations rounds once; a factor 2 of margin.  torch.optim.SGD on fp32 CPU tensors stays within them (worst
error / bound 0.50); the same assertion runs on torch.optim.SGD on the device as a check of the yardstick itself.
"""
import copy
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, rel, TOL, NETS)
from gpu_common import synth                  # noqa: E402

pytestmark = pytest.mark.gpu

#        lr    wd    momentum dampening nesterov clip
ROWS = [(1e-3, 5e-4, 0.9, 0.0, False, None),
        (1e-2, 5e-4, 0.9, 0.0, False, 1.0),
        (1e-2, 0.0, 0.9, 0.0, True, 1.0),
        (1e-2, 5e-4, 0.5, 0.1, False, None),
        (1e-2, 5e-4, 0.0, 0.0, False, 0.5),
        (1e-4, 5e-4, 0.9, 0.0, False, 10.0)]


def chunk():
    from gssd import optim
    return optim.CHUNK


@functools.lru_cache(maxsize=None)
def _host_data(ch):
    """(parameter values, flat gradient, the two extra parameters' values): generated once, never modified (users clone)."""
    ns = [1, 3, 4, 5, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 7, 0]
    rng = np.random.default_rng(20260)

    def draw(n, lo):
        return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(lo, 1, n)).astype(np.float32))
    return [draw(n, -3) for n in ns], draw(sum(ns), -4), [draw(7, -3), draw(5, -3)], draw(7, -4)


class ParamSet:
    """The synthetic set on ``device``: params[0:12] with gradients (slices of self.flat), self.nograd (grad None), self.frozen."""

    def __init__(self, device, ch=None):
        vals, flat, extra, self.late_grad = _host_data(ch or chunk())
        self.params = [torch.nn.Parameter(v.clone().to(device)) for v in vals]
        self.flat = flat.clone().to(device)
        o = 0
        for p in self.params:
            p.grad = self.flat[o:o + p.numel()]
            o += p.numel()
        self.nograd = torch.nn.Parameter(extra[0].clone().to(device))
        self.frozen = torch.nn.Parameter(extra[1].clone().to(device), requires_grad=False)
        self.all = self.params + [self.nograd, self.frozen]

    def groups(self, lr):
        return [dict(params=self.params[0::2] + [self.nograd]), dict(params=self.params[1::2] + [self.frozen], lr=lr * 0.1)]


def norm64(params):
    return math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in params if p.grad is not None))


def coef64(params, clip):
    return 1.0 if clip is None else min(1.0, clip / (norm64(params) + 1e-6))


def snapshot(opt):
    """Per parameter of every group: (p, group, clones of p / g / buf or None) -- the fp32 state the step starts from."""
    snap = []
    for g in opt.param_groups:
        for p in g['params']:
            buf = opt.state[p].get('momentum_buffer') if p in opt.state else None
            snap.append((p, g, p.detach().clone(), None if p.grad is None else p.grad.clone(), None if buf is None else buf.clone()))
    return snap


def check_step(opt, snap, c, clip_on, tag='', twin=None):
    """The state after one step of ``opt`` against float64 from ``snap`` (hyperparameters as the groups hold them NOW); returns the
    worst error / bound ratio.  ``twin``: another optimizer of the same group structure that took the same step from the same state;
    its parameters and buffers must lie within the same bounds of ``opt``'s own."""
    twins = None if twin is None else [q for g in twin.param_groups for q in g['params']]
    worst = 0.0
    for i, (p, g, p0, g0, b0) in enumerate(snap):
        lr, wd, mom, damp, nest = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], g['nesterov']
        buf = opt.state[p].get('momentum_buffer') if p in opt.state else None
        if g0 is None or p0.numel() == 0:
            assert torch.equal(p.detach(), p0), f'{tag} param {i}: touched without a gradient'
            if g0 is None:
                assert (buf is None) if b0 is None else torch.equal(buf, b0), f'{tag} param {i}: state changed without a gradient'
            continue
        p64, g64 = p0.double(), g0.double()
        cg = c * g64
        d = cg + wd * p64
        S = cg.abs() + wd * p64.abs() + (mom * b0.double().abs() if (mom != 0 and b0 is not None) else 0)
        buf_tol = 2.0 ** -21 * S + (4e-6 * cg.abs() if clip_on else 0)
        if mom != 0:
            b64 = d if b0 is None else mom * b0.double() + (1 - damp) * d
            step = d + mom * b64 if nest else b64
            assert buf is not None and buf.shape == p.shape, f'{tag} param {i}: no momentum buffer'
            eb = (buf.double() - b64).abs()
            assert bool((eb <= buf_tol).all()), f'{tag} param {i} buf: err/bound {float((eb / buf_tol.clamp_min(1e-300)).max()):.3g}'
            worst = max(worst, float((eb / buf_tol.clamp_min(1e-300)).max()))
            if twins is not None:
                assert bool(((buf.double() - twin.state[twins[i]]['momentum_buffer'].double()).abs() <= buf_tol).all()), f'{tag} param {i} buf vs twin'
            b64a = b64.abs()
        else:
            step, b64a = d, 0
            assert buf is None, f'{tag} param {i}: momentum 0 keeps no buffer'
        e64 = p64 - lr * step
        p_tol = 2.0 ** -23 * e64.abs() + lr * (2 * buf_tol + 2.0 ** -22 * (S + b64a)) + 1e-38
        ep = (p.detach().double() - e64).abs()
        assert bool((ep <= p_tol).all()), f'{tag} param {i} ({p0.numel()} elements) p: err/bound {float((ep / p_tol).max()):.3g}'
        worst = max(worst, float((ep / p_tol).max()))
        if twins is not None:
            assert bool(((p.detach().double() - twins[i].detach().double()).abs() <= p_tol).all()), f'{tag} param {i} p vs twin'
    return worst


def make_opt(kind, groups, row):
    from gssd import optim
    lr, wd, mom, damp, nest, clip = row
    kw = dict(lr=lr, weight_decay=wd, momentum=mom, dampening=damp, nesterov=nest)
    return optim.SGD(groups, max_grad_norm=clip, **kw) if kind == 'gssd' else torch.optim.SGD(groups, **kw)


def do_step(kind, opt, ps, clip):
    """One step; torch: clip_grad_norm_ + step, with the gradients put back afterwards (gssd.optim.SGD leaves them unscaled itself)."""
    if kind == 'torch' and clip is not None:
        keep = ps.flat.clone()
        torch.nn.utils.clip_grad_norm_(ps.all, clip)
        opt.step()
        ps.flat.copy_(keep)
    else:
        opt.step()


@pytest.mark.parametrize('kind', ['gssd', 'torch'])
@pytest.mark.parametrize('row', ROWS, ids=[f'row{i}' for i in range(len(ROWS))])
def test_step_matches_float64(dev, row, kind):
    ps = ParamSet(dev)
    opt = make_opt(kind, ps.groups(row[0]), row)
    clip = row[5]
    worst = []
    for k in range(3):
        g_before = ps.flat.clone()
        snap = snapshot(opt)
        c = coef64(ps.all, clip)
        do_step(kind, opt, ps, clip)
        worst.append(check_step(opt, snap, c, clip is not None, f'{kind} step {k}'))
        assert torch.equal(ps.flat, g_before), 'the gradients are left unscaled'
        if kind == 'gssd' and clip is not None:
            n64 = norm64(ps.all)
            assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64
        ps.flat.mul_(-0.5)                                  # other gradients for the next step, same storage
    print(f'{kind} {row}: worst error / bound per step', [f'{w:.2f}' for w in worst])


@pytest.mark.parametrize('max_norm', [1.0, 1e9])
def test_clip_grad_norm(dev, max_norm):
    from gssd import optim
    ps = ParamSet(dev)
    g0 = ps.flat.clone()
    n64 = norm64(ps.all)
    assert n64 > 10.0                                       # max_norm 1.0 clips, 1e9 does not
    c64 = min(1.0, max_norm / (n64 + 1e-6))
    total = optim.clip_grad_norm_(ps.all, max_norm)
    assert total.shape == () and total.device == ps.flat.device and total.dtype == torch.float32
    assert abs(float(total) - n64) <= 1e-6 * n64
    want = (g0.double() * c64).float().double()
    err = (ps.flat.double() - want).abs()
    tol = 2.0 ** -23 * g0.double().abs() + (2e-6 * g0.double().abs() if c64 < 1.0 else 0)
    assert bool((err <= tol).all()), float((err / tol.clamp_min(1e-300)).max())
    if c64 < 1.0:
        assert not torch.equal(ps.flat, g0)
    # a one-parameter call (a tensor, not a list) and the same set again (the cached table): the norm is that of the scaled gradients
    again = optim.clip_grad_norm_(ps.all, 1e9)
    n1 = norm64(ps.all)
    assert abs(float(again) - n1) <= 1e-6 * n1
    one = optim.clip_grad_norm_(ps.params[10], 1e9)
    n1 = float(ps.params[10].grad.double().norm())
    assert abs(float(one) - n1) <= 1e-6 * n1


def test_deterministic(dev):
    row = ROWS[1]
    res = []
    for _ in range(2):
        ps = ParamSet(dev)
        opt = make_opt('gssd', ps.groups(row[0]), row)
        norms = []
        for k in range(3):
            opt.step()
            norms.append(opt.grad_norm.clone())
            ps.flat.mul_(-0.5)
        res.append(([p.detach() for p in ps.all], [opt.state[p]['momentum_buffer'] for p in ps.params[:11]], norms))
    for a, b in zip(res[0], res[1]):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_torch_semantics(dev):
    """grad None / frozen / empty parameters stay untouched and stateless; a learning rate edited in param_groups holds for the next
    step of that group alone; a gradient that appears later is picked up (with the first-step rule for its own buffer)."""
    row = (1e-2, 5e-4, 0.9, 0.1, False, 1.0)
    ps = ParamSet(dev)
    opt = make_opt('gssd', ps.groups(row[0]), row)
    keep = [ps.nograd.detach().clone(), ps.frozen.detach().clone()]

    def step(tag):
        snap = snapshot(opt)
        c = coef64([p for g in opt.param_groups for p in g['params']], row[5])
        versions = [p._version for p in ps.all]
        opt.step()
        check_step(opt, snap, c, True, tag)
        for p, v in zip(ps.all, versions):                  # the version counter moves with the data, and only then
            assert (p._version > v) == (p.grad is not None and p.numel() > 0), tag
    step('step 1')
    for p in (ps.nograd, ps.frozen, ps.params[11]):
        assert 'momentum_buffer' not in opt.state.get(p, {})
    assert torch.equal(ps.nograd.detach(), keep[0]) and torch.equal(ps.frozen.detach(), keep[1])
    opt.param_groups[1]['lr'] = 0.37
    step('step 2, new lr in group 1')                       # check_step reads the groups' current lr: 1e-2 and 0.37
    ps.nograd.grad = ps.late_grad.clone().to(dev)
    step('step 3, a gradient appeared')
    assert 'momentum_buffer' in opt.state[ps.nograd] and not torch.equal(ps.nograd.detach(), keep[0])
    ps.nograd.grad = None
    step('step 4, and went away')
    opt.add_param_group(dict(params=[torch.nn.Parameter(torch.full((9,), 2.0, device=dev))], lr=0.5, momentum=0.0))
    opt.param_groups[2]['params'][0].grad = torch.ones(9, device=dev)
    step('step 5, a third group without momentum')


@pytest.mark.parametrize('direction', ['gssd_to_torch', 'torch_to_gssd'])
def test_checkpoint_interop(dev, direction):
    row = (1e-2, 5e-4, 0.9, 0.0, False, None)
    src_kind, dst_kind = ('gssd', 'torch') if direction == 'gssd_to_torch' else ('torch', 'gssd')
    a, b = ParamSet(dev), ParamSet(dev)
    oa, ob = make_opt(src_kind, a.groups(row[0]), row), make_opt(dst_kind, b.groups(row[0]), row)
    for _ in range(2):
        oa.step()
        a.flat.mul_(-0.5)
    sd = copy.deepcopy(oa.state_dict())
    ob.load_state_dict(sd)
    for pa, pb in zip(a.all, b.all):
        pb.data.copy_(pa.detach())
    b.flat.copy_(a.flat)
    for pa, pb in zip(a.params[:11], b.params[:11]):
        assert torch.equal(oa.state[pa]['momentum_buffer'], ob.state[pb]['momentum_buffer'])
    snap_a, snap_b = snapshot(oa), snapshot(ob)
    oa.step()
    ob.step()
    check_step(oa, snap_a, 1.0, False, f'{direction}: {src_kind}', twin=ob)      # against float64, and the two against each other
    check_step(ob, snap_b, 1.0, False, f'{direction}: {dst_kind}')
    assert set(ob.state_dict()['param_groups'][0]) == set(sd['param_groups'][0])


def test_refusals(dev):
    from gssd import optim
    from gssd._lib import GssdError
    good = torch.nn.Parameter(torch.ones(8, device=dev))
    good.grad = torch.ones(8, device=dev)

    def bad_params():
        cpu = torch.nn.Parameter(torch.ones(8))
        cpu.grad = torch.ones(8)
        half = torch.nn.Parameter(torch.ones(8, device=dev, dtype=torch.float16))
        half.grad = torch.ones(8, device=dev, dtype=torch.float16)
        nc = torch.nn.Parameter(torch.ones(4, 6, device=dev).t())
        nc.grad = torch.ones(4, 6, device=dev).t()
        ncg = torch.nn.Parameter(torch.ones(6, 4, device=dev))
        ncg.grad = torch.ones(4, 6, device=dev).t()
        return dict(cpu=cpu, half=half, noncontiguous=nc, noncontiguous_grad=ncg)
    for name, p in bad_params().items():
        assert name == 'noncontiguous_grad' or not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous())
        opt = optim.SGD([good, p], lr=0.1, momentum=0.9, max_grad_norm=1.0)
        with pytest.raises(GssdError, match=r'params"\]\[1\]'):
            opt.step()
        with pytest.raises(GssdError, match='parameter 1'):
            optim.clip_grad_norm_([good, p], 1.0)
        # refused before any launch: the good parameter kept its value, its gradient and got no state
        assert torch.equal(good.detach(), torch.ones(8, device=dev)) and torch.equal(good.grad, torch.ones(8, device=dev)), name
        assert len(opt.state) == 0 and good._version == 0, name
    with pytest.raises(NotImplementedError):
        optim.SGD([good], lr=0.1, maximize=True)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_([good], 1.0, norm_type=1)
    assert torch.equal(good.grad, torch.ones(8, device=dev))


def test_engine_sees_the_update(dev):
    """The driver's step on GSSD with the fused optimizer: parameters match clip_grad_norm_ + torch.optim.SGD on a twin within the
    yardstick above, and the next forward runs on the NEW weights (the engine re-packs on the version counters this optimizer bumps)."""
    from gssd import optim
    from layers.modules import MultiBoxLoss
    from models.ssd_multiphase_custom_group import build_ssd
    flags, args = NETS['gssd']
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    twin = copy.deepcopy(net)
    x = synth.synth_images(2, seed=21).to(dev)
    tg = [t.to(dev) for t in synth.synth_targets(2, seed=21)]
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    ll, lc = crit(net(x), tg)
    (ll + lc).backward()
    twin.load_state_dict(net.state_dict())                   # the BatchNorm running statistics of net's forward included
    for p, q in zip(net.parameters(), twin.parameters()):
        q.grad = None if p.grad is None else p.grad.clone()

    def eval_out(m):
        m.eval()
        with torch.no_grad():
            loc, conf, _ = m(x)
        m.train()
        return loc.clone(), conf.clone()
    before = eval_out(net)
    n64 = norm64(list(net.parameters()))
    max_norm = 1.0
    c = min(1.0, max_norm / (n64 + 1e-6))
    print(f'gradient norm {n64:.4g}, clip coefficient {c:.4g}')
    kw = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)
    opt = optim.SGD(net.parameters(), max_grad_norm=max_norm, **kw)
    ref = torch.optim.SGD(twin.parameters(), **kw)
    snap, snap_ref = snapshot(opt), snapshot(ref)
    opt.step()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
    ref.step()
    assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64
    print('worst error / bound: fused', check_step(opt, snap, c, True, 'fused'), 'torch', check_step(ref, snap_ref, c, True, 'torch'))
    after, after_twin = eval_out(net), eval_out(twin)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]), 'the forward ran on stale packed weights'
    assert rel(after[0], after_twin[0]) < TOL and rel(after[1], after_twin[1]) < TOL
