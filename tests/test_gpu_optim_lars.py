"""GPU tests of gssd.optim.LARS / LAMB (csrc/optim_lars.hip): per-tensor trust ratios formed and consumed on the device, against float64.

The parameter set is that of tests/test_gpu_optim.py (numels [1, 3, 4, 5, 63, 64, 65, CH-1, CH, CH+1, 3*CH+7, 0], gradients as slices of
ONE flat tensor laid end to end, one parameter without a gradient, one frozen) with four tensors appended, their gradients slices of a
second flat tensor: exactly 2 CH elements (a record fold over full chunks only), 257 CH + 1 (more chunk records than a workgroup has
threads: the strided fold takes a second turn), one with an all-zero gradient and one all-zero weight (the fall-backs r = 1).

Yardstick: tests/optim_lars_common.py holds the float64 references and the bounds, derived there rounding by rounding, and its docstring
the formulae.  In short, teacher-forced from the device's own fp32 p, g, buf / m, v before the step, r64 from float64 norms:
    rel_r   = 2^-23 (+ 4e-6 when clipping) (+ ||tol_u||_2 / ||u64||_2 for LAMB);  0 where r is 1 by rule
    LARS    buf_tol = 2^-21 S + (2^-23 + rel_r) r S0 (+ 4e-6 r |c g| when clipping),  S0 = |c g| + wd |p|,  S = r S0 + mom |buf0|
            p_tol   = 2^-23 |p64| + lr (2 buf_tol + 2^-22 (S + |buf64|)) + 1e-38                 -- the SGD test's bounds with the factor r
    LAMB    tol_m, tol_v, tol_u: the Adam test's (decoupled form), u = (m / bc1) / den + wd p,  tol_u += 2^-21 wd |p|
            p_tol   = 2^-23 |p64| + lr r (tol_u + (rel_r + 2^-22) |u|) + 1e-38
Each bound is asserted over four consecutive steps.  The same assertion runs on an fp32 restatement of the rules in torch operations
(``Restated``, on the device here, on the CPU in tests/test_optim_lars_cpu.py) as a check of the yardstick itself: on this
parameter set its worst error / bound over all rows and steps is 0.58 for the tensors and 0.47 for the ratios, on CPU tensors and on the
device alike (the kernels: 0.58 and 0.47).
"""
import copy
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, rel, TOL, NETS)
from gpu_common import synth                  # noqa: E402
import optim_lars_common as LC                # noqa: E402
import test_gpu_optim as TS                   # noqa: E402  (the SGD tests: their parameter set and bound, unchanged)
import test_gpu_optim_adam as TA              # noqa: E402  (the Adam tests' bound)
from test_gpu_optim import ParamSet, chunk, coef64, norm64      # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _extra_data(ch):
    """(values, flat gradient) of the four appended tensors: generated once, never modified (users clone)."""
    ns = [2 * ch, 257 * ch + 1, 70, 33]
    rng = np.random.default_rng(20261)

    def draw(n, lo):
        return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(lo, 1, n)).astype(np.float32))
    vals, flat = [draw(n, -3) for n in ns], draw(sum(ns), -4)
    flat[ns[0] + ns[1]:ns[0] + ns[1] + ns[2]] = 0.0           # the all-zero gradient
    vals[3].zero_()                                           # the all-zero weight
    return vals, flat


class LarsSet(ParamSet):
    """ParamSet with the four tensors appended: self.extra = [2 CH, 257 CH + 1, zero gradient, zero weight], gradients in self.flat2."""

    def __init__(self, device):
        super().__init__(device)
        vals, flat2 = _extra_data(chunk())
        self.extra = [torch.nn.Parameter(v.clone().to(device)) for v in vals]
        self.flat2 = flat2.clone().to(device)
        o = 0
        for p in self.extra:
            p.grad = self.flat2[o:o + p.numel()]
            o += p.numel()
        self.zero_grad_p, self.zero_weight_p = self.extra[2], self.extra[3]
        self.with_grad = self.params + self.extra
        self.all = self.with_grad + [self.nograd, self.frozen]

    def layout(self, lr, layout):
        return LC.layout_groups(self.with_grad, lr, layout, tail=[self.nograd, self.frozen])

    def next_grads(self):
        """Other gradients for the next step, same storage."""
        self.flat.mul_(-0.5)
        self.flat2.mul_(-0.5)

    def grads(self):
        return torch.cat([self.flat, self.flat2])


def make_opt(algo, kind, groups, kw, clip):
    from gssd import optim
    if kind == 'torch':
        return LC.Restated(algo, groups, max_grad_norm=clip, **kw)
    return (optim.LARS if algo == 'lars' else optim.LAMB)(groups, max_grad_norm=clip, **kw)


def state_tensors(algo, opt, ps):
    return [opt.state[p][k] for p in ps if p in opt.state for k in LC.STATE[algo] if k in opt.state[p]]


@pytest.mark.parametrize('kind', ['gssd', 'torch'])
@pytest.mark.parametrize('algo,i', LC.ROWS, ids=[f'{a}{i}' for a, i in LC.ROWS])
def test_step_matches_float64(dev, algo, i, kind):
    from gssd import optim
    kw, clip, layout = LC.row_args(algo, i)
    ps = LarsSet(dev)
    groups = ps.layout(kw['lr'], layout)
    opt = make_opt(algo, kind, groups, kw, clip)
    worst, worst_r = [], []
    for k in range(4):
        g_before = ps.grads()
        snap = LC.snapshot(algo, opt)
        c = coef64(ps.all, clip)
        opt.step()
        w, ratios = LC.check_step(algo, opt, snap, c, clip is not None, f'{kind} {algo} row {i} step {k}')
        worst.append(w)
        worst_r.append(LC.check_ratios(opt.trust_ratio, ratios, f'{kind} {algo} row {i} step {k}'))
        assert torch.equal(ps.grads(), g_before), 'the gradients are left unscaled'
        if kind == 'gssd':
            if clip is not None:
                n64 = norm64(ps.all)
                assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64
            # launches: LARS 2, LAMB 2 (3 with the clip), one more per further eight groups
            assert opt.launches == (2 if algo == 'lars' else 2 + (clip is not None)) + (len(groups) > 8)
        ps.next_grads()
    if kind == 'gssd':
        assert (opt.grad_norm is None) == (clip is None)
        assert opt.trust_ratio.dtype == torch.float32 and opt.trust_ratio.device == ps.flat.device
        for t in state_tensors(algo, opt, ps.with_grad):
            assert t.data_ptr() % 16 == 0 and t.dtype == torch.float32
        if algo == 'lamb':
            for p in ps.with_grad[:11]:
                assert list(opt.state[p]) == ['step', 'exp_avg', 'exp_avg_sq'] and opt.state[p]['step'].device.type == 'cpu'
    print(f'{kind} {algo} row {i}: worst error / bound per step', [f'{w:.2f}' for w in worst], 'ratios', [f'{w:.2f}' for w in worst_r])


@pytest.mark.parametrize('algo', ['lars', 'lamb'])
def test_trust_ratio_vector(dev, algo):
    """opt.trust_ratio entry by entry against float64 norms: within rel_r for adapted tensors, exactly 1 for the group without
    adaptation and for the two fall-back tensors, exactly 0 for the grad-less, the frozen and the empty parameter.  LAMB runs without
    weight decay here: with it an all-zero gradient leaves u = wd w, whose ratio 1 / wd is no fall-back."""
    kw, clip, _ = LC.row_args(algo, 1)
    if algo == 'lamb':
        kw['weight_decay'] = 0.0
    ps = LarsSet(dev)
    groups = ps.layout(kw['lr'], 'three')
    if algo == 'lamb':
        groups[2].pop('weight_decay')
    opt = make_opt(algo, 'gssd', groups, kw, clip)
    order = [p for g in opt.param_groups for p in g['params']]
    slot = {id(p): i for i, p in enumerate(order)}
    for k in range(2):
        snap = LC.snapshot(algo, opt)
        c = coef64(ps.all, clip)
        opt.step()
        _, ratios = LC.check_step(algo, opt, snap, c, True, f'{algo} step {k}')
        tr = opt.trust_ratio.clone()
        assert tr.shape == (len(order),)
        LC.check_ratios(tr, ratios, f'{algo} step {k}')
        for p in (ps.zero_grad_p, ps.zero_weight_p)[:2 - k]:   # (after its first step the all-zero weight is no longer zero)
            assert float(tr[slot[id(p)]]) == 1.0, 'a norm that is exactly zero gives r = 1'
        for p in opt.param_groups[2]['params']:
            assert float(tr[slot[id(p)]]) == (0.0 if p.numel() == 0 else 1.0), 'no adaptation: r = 1'
        for p in (ps.nograd, ps.frozen, ps.params[11]):
            assert float(tr[slot[id(p)]]) == 0.0, 'not in the table: 0'
        adapted = [i for i, r in enumerate(ratios) if r is not None and r[1] > 0]
        assert len(adapted) >= 8 and all(float(tr[i]) != 1.0 for i in adapted)
        if algo == 'lars':                                   # the all-zero gradient: pure weight decay (the momentum buffer carries it)
            j = slot[id(ps.zero_grad_p)]
            assert ratios[j] == (1.0, 0.0)
        ps.next_grads()
    keep = opt.trust_ratio.clone()
    torch.cuda.synchronize()
    assert torch.equal(opt.trust_ratio, keep)                # it stands until the next step


def test_nonadapted_group_is_sgd(dev):
    """All groups with layer_adaptation=False: the step lies within the SGD test's own bound of gssd.optim.SGD from the same state."""
    from gssd import optim
    row = TS.ROWS[1]                                         # lr 1e-2, wd 5e-4, momentum 0.9, clip 1.0
    a, b = ParamSet(dev), ParamSet(dev)
    kw = dict(lr=row[0], weight_decay=row[1], momentum=row[2], dampening=row[3], nesterov=row[4])
    lars = optim.LARS(a.groups(row[0]), max_grad_norm=row[5], layer_adaptation=False, **kw)
    sgd = optim.SGD(b.groups(row[0]), max_grad_norm=row[5], **kw)
    for k in range(3):
        snap = TS.snapshot(lars)
        c = coef64(a.all, row[5])
        lars.step()
        sgd.step()
        TS.check_step(lars, snap, c, True, f'LARS without adaptation, step {k}', twin=sgd)
        for p, q in zip(a.params, b.params):                 # r = 1 makes the extra product exact: the same arithmetic, the same bits
            assert torch.equal(p.detach(), q.detach())
        assert torch.equal(lars.grad_norm, sgd.grad_norm)
        n = len(a.all)
        assert torch.equal(lars.trust_ratio, torch.tensor([float(p.grad is not None and p.numel() > 0) for g in lars.param_groups
                                                           for p in g['params']], device=dev)) and lars.trust_ratio.numel() == n
        a.flat.mul_(-0.5)
        b.flat.mul_(-0.5)


def test_nonadapted_group_is_adamw(dev):
    """All groups with layer_adaptation=False: w -= lr (m^ / den + wd w), AdamW's step up to where the decay enters -- the result lies
    within the Adam test's AdamW bound of gssd.optim.AdamW from the same state."""
    from gssd import optim
    row = (1e-3, 0.9, 0.999, 1e-6, 1e-2, False, True, 1.0)   # the Adam tests' row layout: decoupled, clip 1.0
    a, b = ParamSet(dev), ParamSet(dev)
    kw = dict(lr=row[0], betas=(row[1], row[2]), eps=row[3], weight_decay=row[4])
    lamb = optim.LAMB(a.groups(row[0]), max_grad_norm=row[7], layer_adaptation=False, **kw)
    adamw = optim.AdamW(b.groups(row[0]), max_grad_norm=row[7], **kw)
    for k in range(3):
        snap = TA.snapshot(adamw)
        c = coef64(b.all, row[7])
        lamb.step()
        adamw.step()
        TA.check_step(adamw, snap, c, True, f'AdamW and LAMB without adaptation, step {k}', twin=lamb)
        assert torch.equal(lamb.grad_norm, adamw.grad_norm)
        with torch.no_grad():                                # the next step starts from the same state again
            for p, q in zip(a.params[:11], b.params[:11]):
                p.copy_(q)
                for name in LC.STATE['lamb']:
                    lamb.state[p][name].copy_(adamw.state[q][name])
        a.flat.mul_(-0.5)
        b.flat.mul_(-0.5)


@pytest.mark.parametrize('algo', ['lars', 'lamb'])
def test_deterministic(dev, algo):
    """Two optimizers from equal state: bitwise equal parameters, state, trust_ratio and norms, with and without the clip."""
    for i in (0, 1):                                         # row 0: no clip; row 1: clip 1.0 and a group without adaptation
        kw, clip, layout = LC.row_args(algo, i)
        res = []
        for _ in range(2):
            ps = LarsSet(dev)
            opt = make_opt(algo, 'gssd', ps.layout(kw['lr'], layout), kw, clip)
            seen = []
            for k in range(3):
                opt.step()
                seen.append(opt.trust_ratio.clone())
                if clip is not None:
                    seen.append(opt.grad_norm.clone())
                ps.next_grads()
            res.append(([p.detach() for p in ps.all], state_tensors(algo, opt, ps.with_grad), seen))
        for a, b in zip(res[0], res[1]):
            assert len(a) == len(b) > 0 and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('direction', ['lars_to_torch', 'torch_to_lars', 'lamb_to_torch', 'torch_to_lamb'])
def test_checkpoint_interop(dev, direction):
    """LARS <-> torch.optim.SGD and LAMB <-> torch.optim.Adam: the state travels bit for bit, the extra group keys travel or are filled
    from the defaults, and a step after loading continues within the bounds (LARS / LAMB against float64; torch's optimizer against
    the SGD / Adam tests' own yardstick)."""
    from gssd import optim
    algo = 'lars' if 'lars' in direction else 'lamb'
    to_torch = direction.endswith('to_torch')
    a, b = ParamSet(dev), ParamSet(dev)
    if algo == 'lars':
        kw = dict(lr=1e-2, weight_decay=5e-4, momentum=0.9)
        ours, theirs = (lambda ps: optim.LARS(ps.groups(1e-2), **kw)), (lambda ps: torch.optim.SGD(ps.groups(1e-2), **kw))
    else:
        kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=1e-2)
        ours, theirs = (lambda ps: optim.LAMB(ps.groups(1e-3), **kw)), (lambda ps: torch.optim.Adam(ps.groups(1e-3), **kw))
    oa, ob = (ours(a), theirs(b)) if to_torch else (theirs(a), ours(b))
    for _ in range(2):
        oa.step()
        a.flat.mul_(-0.5)
    sd = copy.deepcopy(oa.state_dict())
    ob.load_state_dict(sd)
    for pa, pb in zip(a.all, b.all):
        pb.data.copy_(pa.detach())
    b.flat.copy_(a.flat)
    for pa, pb in zip(a.params[:11], b.params[:11]):
        names = LC.STATE[algo] + (('step',) if algo == 'lamb' else ())
        assert set(oa.state[pa]) == set(ob.state[pb]) == set(names)
        assert all(torch.equal(oa.state[pa][k], ob.state[pb][k].to(oa.state[pa][k].device)) for k in names)
    mine, torchs = (oa, ob) if to_torch else (ob, oa)
    snap = LC.snapshot(algo, mine)
    snap_t = TS.snapshot(torchs) if algo == 'lars' else TA.snapshot(torchs)
    oa.step()
    ob.step()
    LC.check_step(algo, mine, snap, 1.0, False, direction)
    (TS if algo == 'lars' else TA).check_step(torchs, snap_t, 1.0, False, direction + ': torch')
    extra = set(LC.EXTRA[algo])
    got, had = set(ob.state_dict()['param_groups'][0]), set(sd['param_groups'][0])
    assert got == had | extra and (extra <= had) == to_torch
    if algo == 'lamb':
        assert all(float(ob.state[pb]['step']) == 3 for pb in b.params[:11])
    if not to_torch:
        g = mine.param_groups[0]
        assert all(g[k] == mine.defaults[k] for k in extra)


@pytest.mark.parametrize('algo', ['lars', 'lamb'])
def test_torch_semantics(dev, algo):
    """grad None / frozen / empty parameters stay untouched and stateless with ratio 0; an lr edited in param_groups holds for the next
    step of that group alone and needs no new table; a gradient that appears later is picked up (LARS: first-step rule for its buffer;
    LAMB: its own bias correction from step 1); when it goes away its state and step count stand still; version counters move with
    the data."""
    kw, clip, _ = LC.row_args(algo, 1)
    if algo == 'lars':
        kw['dampening'] = 0.1
    ps = LarsSet(dev)
    opt = make_opt(algo, 'gssd', ps.layout(kw['lr'], 'two'), kw, clip)
    keep = [ps.nograd.detach().clone(), ps.frozen.detach().clone()]
    count = {}

    def step(tag):
        snap = LC.snapshot(algo, opt)
        c = coef64([p for g in opt.param_groups for p in g['params']], clip)
        versions = [(p, p._version) for g in opt.param_groups for p in g['params']]
        opt.step()
        _, ratios = LC.check_step(algo, opt, snap, c, True, tag)
        LC.check_ratios(opt.trust_ratio, ratios, tag)
        for p, v in versions:                               # the version counter moves with the data, and only then
            moved = p.grad is not None and p.numel() > 0
            assert (p._version > v) == moved, tag
            count[p] = count.get(p, 0) + moved
            if algo == 'lamb':
                assert (float(opt.state[p]['step']) if p in opt.state and opt.state[p] else 0) == count[p], tag
    step('step 1')
    for p in (ps.nograd, ps.frozen, ps.params[11]):
        assert p not in opt.state or len(opt.state[p]) == 0
    assert torch.equal(ps.nograd.detach(), keep[0]) and torch.equal(ps.frozen.detach(), keep[1])
    step('step 2')                                           # (LARS: the table without first-step flags is built here)
    table = opt._table
    opt.param_groups[1]['lr'] = 0.037
    step('step 3, new lr in group 1')                        # check_step reads the groups' current values
    assert opt._table is table, 'an lr edit needs no new table'
    assert opt.param_groups[0]['lr'] == kw['lr']
    ps.nograd.grad = ps.late_grad.clone().to(dev)
    step('step 4, a gradient appeared')
    assert opt._table is not table or algo == 'lars'
    assert count[ps.nograd] == 1 and count[ps.params[0]] == 4 and not torch.equal(ps.nograd.detach(), keep[0])
    step('step 5, the late one at its step 2')
    ps.nograd.grad = None
    frozen_state = {k: v.clone() for k, v in opt.state[ps.nograd].items()}
    step('step 6, and went away')
    assert all(torch.equal(opt.state[ps.nograd][k], v) for k, v in frozen_state.items()) and count[ps.nograd] == 2
    late = torch.nn.Parameter(torch.full((9,), 2.0, device=dev))
    opt.add_param_group(dict(params=[late], lr=0.5, layer_adaptation=False))
    late.grad = torch.linspace(-1, 1, 9, device=dev)
    step('step 7, a third group without adaptation')
    assert count[late] == 1 and float(opt.trust_ratio[-1]) == 1.0 and opt.trust_ratio.numel() == len(ps.all) + 1


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
        ncg = torch.nn.Parameter(torch.ones(6, 4, device=dev))
        ncg.grad = torch.ones(4, 6, device=dev).t()
        return dict(cpu=cpu, half=half, noncontiguous_grad=ncg)
    for cls in (optim.LARS, optim.LAMB):
        for name, p in bad_params().items():
            opt = cls([good, p], lr=0.1, max_grad_norm=1.0)
            with pytest.raises(GssdError, match=r'params"\]\[1\].*no CPU fallback'):
                opt.step()
            # refused before any launch: the good parameter kept its value, its gradient and got no state
            assert torch.equal(good.detach(), torch.ones(8, device=dev)) and torch.equal(good.grad, torch.ones(8, device=dev)), name
            assert len(opt.state) == 0 and good._version == 0 and opt.grad_norm is None and opt.trust_ratio is None, name
        with pytest.raises(NotImplementedError):
            cls([good], lr=torch.tensor(0.1))
        opt = cls([good], lr=0.1)
        opt.param_groups[0]['lr'] = torch.tensor(0.1, device=dev)
        with pytest.raises(NotImplementedError):
            opt.step()
        assert len(opt.state) == 0 and good._version == 0


def test_engine_sees_the_update(dev):
    """One LARS step on GSSD from real HIP-backward gradients (B = 2): every parameter against the teacher-forced rule, biases and
    BatchNorm weights in a group without adaptation, and the next forward runs on the NEW weights (the engine re-packs on the version
    counters this optimizer bumps)."""
    from gssd import optim
    from layers.modules import MultiBoxLoss
    from models.ssd_multiphase_custom_group import build_ssd
    flags, args = NETS['gssd']
    net = build_ssd('train', 300, 2, *args)
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111))
    net = net.to(dev).train()
    x = synth.synth_images(2, seed=21).to(dev)
    tg = [t.to(dev) for t in synth.synth_targets(2, seed=21)]
    crit = MultiBoxLoss(2, 0.5, True, 0, True, 3, 0.5, False, True)
    ll, lc = crit(net(x), tg)
    (ll + lc).backward()

    def eval_out(m):
        m.eval()
        with torch.no_grad():
            loc, conf, _ = m(x)
        m.train()
        return loc.clone(), conf.clone()
    before = eval_out(net)
    params = list(net.parameters())
    n64 = norm64(params)
    max_norm = 1.0
    c = min(1.0, max_norm / (n64 + 1e-6))
    groups = [dict(params=[p for p in params if p.dim() > 1]),
              dict(params=[p for p in params if p.dim() <= 1], layer_adaptation=False, weight_decay=0.0)]
    assert len(groups[0]['params']) > 10 and len(groups[1]['params']) > 10
    opt = optim.LARS(groups, lr=0.5, momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)
    snap = LC.snapshot('lars', opt)
    opt.step()
    assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64 and opt.launches == 2
    worst, ratios = LC.check_step('lars', opt, snap, c, True, 'LARS on GSSD')
    worst_r = LC.check_ratios(opt.trust_ratio, ratios, 'LARS on GSSD')
    print(f'gradient norm {n64:.4g}, clip coefficient {c:.4g}, worst error / bound {worst:.2f} (tensors) {worst_r:.2f} (ratios)')
    after = eval_out(net)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]), 'the forward ran on stale packed weights'
