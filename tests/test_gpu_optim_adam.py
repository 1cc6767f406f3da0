"""GPU tests of gssd.optim.Adam / AdamW (csrc/optim_adam.hip): torch's single-tensor Adam rule with the gradient-norm clip fused in,
against float64.

The parameter set is that of tests/test_gpu_optim.py: numels [1, 3, 4, 5, 63, 64, 65, CH-1, CH, CH+1, 3*CH+7, 0], gradients as slices
of ONE flat tensor laid end to end (with the 16-byte aligned state both the vector path and the element-wise path run, with full chunks,
short chunks and tails), one parameter without a gradient, one frozen, two param groups with the second at lr * 0.1.

Yardstick (teacher-forced: the expected values are computed in float64 from the device's own fp32 p, g, m, v, vmax before the step; c is
the clip coefficient, g' = c g (+ wd p when coupled), den = sqrt(vh) / sqrt(bc2) + eps, u = (lr / bc1) m / den):
    tol_g = 2^-22 (|c g| + wd |p|) coupled, 2^-23 |c g| decoupled            (+ 4e-6 |c g| when clipping: the 1e-6 allowed on the norm)
    tol_m = (1 - b1) tol_g + 2^-22 (|m0| + |g'|)
    tol_v = (1 - b2) 2 |g'| tol_g + 2^-22 (b2 v0 + (1 - b2) g'^2)              (the same bound for vmax)
    tol_r = min(tol_v / (2 sqrt(vh)), sqrt(tol_v))
    tol_d = tol_r / sqrt(bc2) + 2^-22 den
    tol_u = (lr / bc1) (tol_m / den + |m| tol_d / den^2) + 2^-21 |u|
    tol_p = 2^-23 |p'| + tol_u + 1e-38                                          (+ 2^-23 |p0| decoupled)
Each fp32 operation rounds once; a factor 2 of margin.  torch.optim.Adam / AdamW on fp32 CPU tensors stay within them (worst error /
bound 0.56 over these rows and four steps); the same assertion runs on torch's optimizers on the device as a check of the yardstick
itself.
"""
import copy
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, rel, TOL, NETS)
from gpu_common import synth                  # noqa: E402
from test_gpu_optim import ParamSet, coef64, norm64      # noqa: E402  (the SGD tests' parameter set, unchanged)

pytestmark = pytest.mark.gpu

#        lr    b1   b2     eps   wd    amsgrad decoupled clip
ROWS = [(1e-3, 0.9, 0.999, 1e-8, 0.0, False, False, None),
        (1e-3, 0.9, 0.999, 1e-8, 5e-4, False, False, 1.0),
        (1e-2, 0.9, 0.999, 1e-8, 1e-2, False, True, 1.0),
        (1e-3, 0.5, 0.9, 1e-6, 5e-4, True, False, None),
        (1e-4, 0.9, 0.99, 1e-8, 1e-2, True, True, 10.0),
        (1e-3, 0.0, 0.999, 1e-3, 0.0, False, False, 0.5)]
STATE = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def all_params(opt):
    return [p for g in opt.param_groups for p in g['params']]


def snapshot(opt):
    """Per parameter of every group: (p, group, clones of p / g or None, {state name: clone}, step count) -- what the step starts from."""
    snap = []
    for g in opt.param_groups:
        for p in g['params']:
            s = opt.state[p] if p in opt.state else {}
            snap.append((p, g, p.detach().clone(), None if p.grad is None else p.grad.clone(), {k: s[k].clone() for k in STATE if k in s},
                         int(float(s['step'])) if 'step' in s else 0))
    return snap


def check_step(opt, snap, c, clip_on, tag='', twin=None):
    """The state after one step of ``opt`` against float64 from ``snap`` (hyperparameters as the groups hold them NOW); returns the
    worst error / bound ratio.  ``twin``: another optimizer of the same group structure that took the same step from the same state;
    its parameters and moments must lie within the same bounds of ``opt``'s own."""
    twins = None if twin is None else all_params(twin)
    worst = 0.0

    def within(name, i, got, want, tol, other=None):
        nonlocal worst
        err = (got.double() - want).abs()
        ratio = float((err / tol.clamp_min(1e-300)).max())
        assert bool((err <= tol).all()), f'{tag} param {i} ({got.numel()} elements) {name}: err/bound {ratio:.3g}'
        worst = max(worst, ratio)
        if other is not None:
            assert bool(((got.double() - other.double()).abs() <= tol).all()), f'{tag} param {i} {name} vs twin'

    for i, (p, g, p0, g0, s0, step0) in enumerate(snap):
        lr, (b1, b2), eps, wd, ams = g['lr'], g['betas'], g['eps'], g['weight_decay'], g['amsgrad']
        dec = g['decoupled_weight_decay']
        s = opt.state[p] if p in opt.state else {}
        if g0 is None or p0.numel() == 0:
            assert torch.equal(p.detach(), p0), f'{tag} param {i}: touched without a gradient'
            if g0 is None:
                assert set(s) == (set(s0) | {'step'} if s0 else set()), f'{tag} param {i}: state appeared without a gradient'
                assert all(torch.equal(s[k], s0[k]) for k in s0) and (not s0 or int(float(s['step'])) == step0), \
                    f'{tag} param {i}: state changed without a gradient'
            continue
        step = step0 + 1
        assert int(float(s['step'])) == step, f'{tag} param {i}: step {float(s["step"])}, expected {step}'
        for k in STATE[:2 + bool(ams)]:
            assert k in s and s[k].shape == p.shape and s[k].dtype == torch.float32, f'{tag} param {i}: no {k}'
        assert ams or 'max_exp_avg_sq' not in s, f'{tag} param {i}: max_exp_avg_sq without amsgrad'
        tw = None if twins is None else twin.state[twins[i]]
        zero = torch.zeros_like(p0, dtype=torch.float64)
        p64, g64 = p0.double(), g0.double()
        m0, v0 = (s0[k].double() if k in s0 else zero for k in STATE[:2])
        x0 = s0['max_exp_avg_sq'].double() if 'max_exp_avg_sq' in s0 else zero
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        cg = c * g64
        if dec:
            gp, tol_g, p1 = cg, 2.0 ** -23 * cg.abs(), p64 * (1 - lr * wd)
        else:
            gp, tol_g, p1 = cg + wd * p64, 2.0 ** -22 * (cg.abs() + wd * p64.abs()), p64
        if clip_on:
            tol_g = tol_g + 4e-6 * cg.abs()
        m = b1 * m0 + (1 - b1) * gp
        tol_m = (1 - b1) * tol_g + 2.0 ** -22 * (m0.abs() + gp.abs())
        v = b2 * v0 + (1 - b2) * gp * gp
        tol_v = (1 - b2) * 2 * gp.abs() * tol_g + 2.0 ** -22 * (b2 * v0 + (1 - b2) * gp * gp)
        within('exp_avg', i, s['exp_avg'], m, tol_m, None if tw is None else tw['exp_avg'])
        within('exp_avg_sq', i, s['exp_avg_sq'], v, tol_v, None if tw is None else tw['exp_avg_sq'])
        vh = v
        if ams:
            vh = torch.maximum(x0, v)
            within('max_exp_avg_sq', i, s['max_exp_avg_sq'], vh, tol_v, None if tw is None else tw['max_exp_avg_sq'])
        tol_r = torch.minimum(tol_v / (2 * vh.sqrt()).clamp_min(1e-300), tol_v.sqrt())
        den = vh.sqrt() / math.sqrt(bc2) + eps
        tol_d = tol_r / math.sqrt(bc2) + 2.0 ** -22 * den
        u = (lr / bc1) * m / den
        tol_u = (lr / bc1) * (tol_m / den + m.abs() * tol_d / den ** 2) + 2.0 ** -21 * u.abs()
        e64 = p1 - u
        tol_p = 2.0 ** -23 * e64.abs() + tol_u + 1e-38 + (2.0 ** -23 * p64.abs() if dec else 0)
        within('p', i, p.detach(), e64, tol_p, None if twins is None else twins[i].detach())
    return worst


def make_opt(kind, groups, row):
    from gssd import optim
    lr, b1, b2, eps, wd, ams, dec, clip = row
    kw = dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=ams)
    if kind == 'gssd':
        return (optim.AdamW if dec else optim.Adam)(groups, max_grad_norm=clip, **kw)
    return (torch.optim.AdamW if dec else torch.optim.Adam)(groups, **kw)


def do_step(kind, opt, ps, clip):
    """One step; torch: clip_grad_norm_ + step, with the gradients put back afterwards (gssd.optim leaves them unscaled itself)."""
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
    assert opt.param_groups[1]['lr'] == row[0] * 0.1 and opt.param_groups[0]['decoupled_weight_decay'] == row[6]
    clip = row[7]
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
        for p in ps.params[:11]:
            assert float(opt.state[p]['step']) == k + 1
        ps.flat.mul_(-0.5)                                  # other gradients for the next step, same storage
    if kind == 'gssd':
        assert (opt.grad_norm is None) == (clip is None)
        for p in ps.params[:11]:                            # torch's state layout: a host step counter, moments shaped like p
            s = opt.state[p]
            assert list(s) == ['step', 'exp_avg', 'exp_avg_sq'] + ['max_exp_avg_sq'] * row[5]
            assert s['step'].device.type == 'cpu' and s['step'].dtype == torch.float32 and s['step'].shape == ()
            assert all(s[n].data_ptr() % 16 == 0 and s[n].device == p.device for n in list(s)[1:])
    print(f'{kind} {row}: worst error / bound per step', [f'{w:.2f}' for w in worst])


def test_torch_semantics(dev):
    """grad None / frozen / empty parameters stay untouched and stateless; an lr and betas edited in param_groups hold for the next step
    of that group alone; a gradient that appears at step 3 starts its own bias correction at step 1 while the others are at 3, and when
    it goes away again its state and step stand still; a third group added later works; version counters move with the data."""
    row = (1e-2, 0.9, 0.999, 1e-8, 5e-4, True, False, 1.0)
    ps = ParamSet(dev)
    opt = make_opt('gssd', ps.groups(row[0]), row)
    keep = [ps.nograd.detach().clone(), ps.frozen.detach().clone()]
    count = {}                                              # this test's own step counts

    def step(tag):
        snap = snapshot(opt)
        c = coef64(all_params(opt), row[7])
        versions = [(p, p._version) for p in all_params(opt)]
        opt.step()
        check_step(opt, snap, c, True, tag)                 # (bias corrections from the step counts in snap)
        for p, v in versions:                               # the version counter moves with the data, and only then
            moved = p.grad is not None and p.numel() > 0
            assert (p._version > v) == moved, tag
            count[p] = count.get(p, 0) + moved
            assert (float(opt.state[p]['step']) if p in opt.state else 0) == count[p], tag
    step('step 1')
    for p in (ps.nograd, ps.frozen, ps.params[11]):
        assert p not in opt.state or len(opt.state[p]) == 0
    assert torch.equal(ps.nograd.detach(), keep[0]) and torch.equal(ps.frozen.detach(), keep[1])
    opt.param_groups[1]['lr'] = 0.037
    opt.param_groups[1]['betas'] = (0.8, 0.95)
    step('step 2, new lr and betas in group 1')             # check_step reads the groups' current values
    assert opt.param_groups[0]['lr'] == 1e-2 and opt.param_groups[0]['betas'] == (0.9, 0.999)
    ps.nograd.grad = ps.late_grad.clone().to(dev)
    step('step 3, a gradient appeared')
    assert count[ps.nograd] == 1 and count[ps.params[0]] == 3 and not torch.equal(ps.nograd.detach(), keep[0])
    step('step 4, the late one at its step 2')
    assert count[ps.nograd] == 2 and count[ps.params[0]] == 4
    ps.nograd.grad = None
    frozen_state = {k: v.clone() for k, v in opt.state[ps.nograd].items()}
    step('step 5, and went away')
    assert all(torch.equal(opt.state[ps.nograd][k], v) for k, v in frozen_state.items()) and count[ps.nograd] == 2
    late = torch.nn.Parameter(torch.full((9,), 2.0, device=dev))
    opt.add_param_group(dict(params=[late], lr=0.5, amsgrad=False, weight_decay=0.0))
    late.grad = torch.linspace(-1, 1, 9, device=dev)
    step('step 6, a third group without amsgrad')
    assert count[late] == 1 and count[ps.params[0]] == 6 and 'max_exp_avg_sq' not in opt.state[late]


def test_more_groups_than_one_launch_takes(dev):
    """Nine groups (a launch carries eight) of one 5-element parameter each, distinct learning rates, with clipping."""
    from gssd import optim
    gen = torch.Generator().manual_seed(9)
    params = [torch.nn.Parameter(torch.randn(5, generator=gen).to(dev)) for _ in range(9)]
    for p in params:
        p.grad = (torch.randn(5, generator=gen) * 3).to(dev)
    opt = optim.Adam([dict(params=[p], lr=1e-3 * (i + 1)) for i, p in enumerate(params)], weight_decay=5e-4, max_grad_norm=1.0)
    for k in range(2):
        before = [p.detach().clone() for p in params]
        snap = snapshot(opt)
        n64 = norm64(params)
        assert n64 > 1.0
        opt.step()
        check_step(opt, snap, min(1.0, 1.0 / (n64 + 1e-6)), True, f'nine groups, step {k}')
        assert all(not torch.equal(p.detach(), b) for p, b in zip(params, before))
        assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64


def test_deterministic(dev):
    row = ROWS[4]
    res = []
    for _ in range(2):
        ps = ParamSet(dev)
        opt = make_opt('gssd', ps.groups(row[0]), row)
        norms = []
        for k in range(3):
            opt.step()
            norms.append(opt.grad_norm.clone())
            ps.flat.mul_(-0.5)
        res.append(([p.detach() for p in ps.all], [opt.state[p][k] for p in ps.params[:11] for k in STATE], norms))
    for a, b in zip(res[0], res[1]):
        assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('amsgrad', [False, True], ids=['plain', 'amsgrad'])
@pytest.mark.parametrize('direction', ['gssd_to_torch', 'torch_to_gssd'])
def test_checkpoint_interop(dev, direction, amsgrad):
    row = (1e-3, 0.9, 0.999, 1e-8, 1e-2, amsgrad, True, None)
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
        assert set(oa.state[pa]) == set(ob.state[pb]) == {'step'} | set(STATE[:2 + amsgrad])
        assert all(torch.equal(oa.state[pa][k], ob.state[pb][k].to(oa.state[pa][k].device)) for k in oa.state[pa])
    snap_a, snap_b = snapshot(oa), snapshot(ob)
    oa.step()
    ob.step()
    check_step(oa, snap_a, 1.0, False, f'{direction}: {src_kind}', twin=ob)      # against float64, and the two against each other
    check_step(ob, snap_b, 1.0, False, f'{direction}: {dst_kind}')
    assert all(float(ob.state[pb]['step']) == 3 for pb in b.params[:11])
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
    for cls in (optim.Adam, optim.AdamW):
        for name, p in bad_params().items():
            assert name == 'noncontiguous_grad' or not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous())
            opt = cls([good, p], lr=0.1, amsgrad=True, max_grad_norm=1.0)
            with pytest.raises(GssdError, match=r'params"\]\[1\].*no CPU fallback'):
                opt.step()
            # refused before any launch: the good parameter kept its value, its gradient and got no state
            assert torch.equal(good.detach(), torch.ones(8, device=dev)) and torch.equal(good.grad, torch.ones(8, device=dev)), name
            assert len(opt.state) == 0 and good._version == 0 and opt.grad_norm is None, name
        with pytest.raises(NotImplementedError):
            cls([good], lr=0.1, maximize=True)


def test_engine_sees_the_update(dev):
    """A training step on GSSD with the fused AdamW: parameters match clip_grad_norm_ + torch.optim.AdamW on a twin within the yardstick
    above, and the next forward runs on the NEW weights (the engine re-packs on the version counters this optimizer bumps)."""
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
    kw = dict(lr=1e-4, weight_decay=1e-2)
    opt = optim.AdamW(net.parameters(), max_grad_norm=max_norm, **kw)
    ref = torch.optim.AdamW(twin.parameters(), **kw)
    snap, snap_ref = snapshot(opt), snapshot(ref)
    opt.step()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), max_norm)
    ref.step()
    assert abs(float(opt.grad_norm) - n64) <= 1e-6 * n64
    print('worst error / bound: fused', check_step(opt, snap, c, True, 'fused', twin=ref), 'torch', check_step(ref, snap_ref, c, True, 'torch'))
    after, after_twin = eval_out(net), eval_out(twin)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1]), 'the forward ran on stale packed weights'
    assert rel(after[0], after_twin[0]) < TOL and rel(after[1], after_twin[1]) < TOL
