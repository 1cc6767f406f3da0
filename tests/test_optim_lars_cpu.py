"""Host logic of gssd.optim.LARS / LAMB that needs no GPU: the ABI wiring of csrc/optim_lars.hip's entry points and the layout of the two
hyperparameter structs, the torch.optim.Optimizer surface with the documented defaults and group keys, the table key, the refusals that
are decided before any launch, SGD- and Adam-format checkpoints, and the yardstick of tests/test_gpu_optim_lars.py itself: the float64
references of tests/optim_lars_common.py against an independent restatement of the rules in torch operations -- in float64 (the two must
agree to rounding) and in fp32 (the restatement must stay inside the bounds the device kernels are held to; worst error / bound on CPU
tensors over all rows and four steps: 0.52 for the tensors, 0.49 for the ratios)."""
import copy
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_lars_common as LC                                          # noqa: E402
from test_optim_adam_cpu import HEADER, header_struct                   # noqa: E402  (the header's struct parser, unchanged)


def test_abi_carries_the_entry_points():
    from gssd import _lib
    hdr = open(HEADER).read()
    for n, nargs in (('gssd_lars_step_f32', 13), ('gssd_lamb_step_f32', 14)):
        assert re.search(r'\bint\s+' + n + r'\s*\(', hdr) and n in _lib.SIGNATURES
        i = _lib.lib.gssd_plan_fn_index(n.encode())
        assert i >= 0 and _lib.lib.gssd_plan_fn_nargs(i) == len(_lib.SIGNATURES[n][1]) - 1 == nargs
    assert re.search(r'\blong long\s+gssd_lars_workspace_bytes\s*\(', hdr) and 'gssd_lars_workspace_bytes' in _lib.SIGNATURES
    assert _lib.lib.gssd_abi_version() == 8
    assert [_lib.lib.gssd_lars_workspace_bytes(n) for n in (-1, 0, 1, 1150)] == [0, 0, 16, 16 * 1150]
    # argument validation happens before anything touches a device
    one = ctypes.c_void_p(16)                  # never dereferenced: every call below is refused
    hy = (_lib.LarsHyper * 1)()
    lars = _lib.lib.gssd_lars_step_f32
    assert lars(None, None, 1, None, None, None, 1, None, None, 0, -1.0, None, None, None) == -1
    assert b'invalid argument' in _lib.lib.gssd_last_error()
    assert lars(None, one, 1, one, None, hy, 1, one, None, 0, -1.0, None, one, None) == -1            # no items
    assert lars(one, None, 1, one, None, hy, 1, one, None, 0, -1.0, None, one, None) == -1            # no chunks
    assert lars(one, one, 0, one, None, hy, 1, one, None, 0, -1.0, None, one, None) == -1             # no work
    assert lars(one, one, 1, None, None, hy, 1, one, None, 0, -1.0, None, one, None) == -1            # no chunk prefix
    assert lars(one, one, 1, one, None, None, 1, one, None, 0, -1.0, None, one, None) == -1           # no hyperparameters
    assert lars(one, one, 1, one, None, hy, 0, one, None, 0, -1.0, None, one, None) == -1             # no groups
    assert lars(one, one, 1, one, None, hy, 1, None, None, 0, -1.0, None, one, None) == -1            # no workspace
    assert lars(one, one, 1, one, None, hy, 1, ctypes.c_void_p(20), None, 0, -1.0, None, one, None) == -1   # ... misaligned
    assert lars(one, one, 1, one, None, hy, 1, one, None, 0, -1.0, None, None, None) == -1            # no ratio_out
    assert lars(one, one, 1, one, None, hy, 1, one, None, 1, 1.0, one, one, None) == -1               # clip without partial sums
    assert lars(one, one, 1, one, None, hy, 1, one, one, 2, 1.0, one, one, None) == -1                # ... of another length
    assert lars(one, one, 1, one, None, hy, 1, one, one, 1, 1.0, None, one, None) == -1               # clip without norm_out
    hy = (_lib.LambHyper * 1)()
    lamb = _lib.lib.gssd_lamb_step_f32
    assert lamb(None, one, 1, one, None, hy, 1, 1, one, None, 0, -1.0, None, one, None) == -1         # no items
    assert lamb(one, one, 0, one, None, hy, 1, 1, one, None, 0, -1.0, None, one, None) == -1          # no work
    assert lamb(one, one, 1, None, None, hy, 1, 1, one, None, 0, -1.0, None, one, None) == -1         # no chunk prefix
    assert lamb(one, one, 1, one, None, None, 1, 1, one, None, 0, -1.0, None, one, None) == -1        # no hyperparameters
    assert lamb(one, one, 1, one, None, hy, 1, 1, None, None, 0, -1.0, None, one, None) == -1         # no workspace
    assert lamb(one, one, 1, one, None, hy, 1, 1, one, None, 0, -1.0, None, None, None) == -1         # no ratio_out
    assert lamb(one, one, 1, one, None, hy, 1, 1, one, None, 0, 1.0, one, one, None) == -1            # clip without partial sums
    assert lamb(one, one, 1, one, None, hy, 1, 1, one, one, 1, 1.0, None, one, None) == -1            # clip without norm_out


def test_struct_layouts_agree():
    from gssd import _lib, optim
    C_DOUBLE = dict(lr=8, weight_decay=8, trust_coefficient=8, eps=8)
    hyper, size = header_struct('gssd_lars_hyper')
    assert [n for n, _ in hyper] == ['lr', 'weight_decay', 'trust_coefficient', 'eps', 'momentum', 'dampening', 'nesterov', 'adapt']
    assert size == ctypes.sizeof(_lib.LarsHyper) == 48
    assert hyper == [(n, getattr(_lib.LarsHyper, n).offset) for n, _ in _lib.LarsHyper._fields_]
    assert all(getattr(_lib.LarsHyper, n).size == s for n, s in C_DOUBLE.items())       # r is formed from them in fp64
    hyper, size = header_struct('gssd_lamb_hyper')
    assert [n for n, _ in hyper] == ['lr', 'beta1', 'beta2', 'one_minus_beta1', 'one_minus_beta2', 'eps', 'weight_decay',
                                     'bias_correction', 'adapt']
    assert size == ctypes.sizeof(_lib.LambHyper) == 48
    assert hyper == [(n, getattr(_lib.LambHyper, n).offset) for n, _ in _lib.LambHyper._fields_]
    # the tables are the SGD / Adam kernels': their structs are unchanged
    item, size = header_struct('gssd_sgd_item')
    assert size == optim._ITEM.itemsize and item == [(n, optim._ITEM.fields[n][1]) for n in optim._ITEM.names]
    item, size = header_struct('gssd_adam_item')
    assert size == optim._ADAM_ITEM.itemsize and item == [(n, optim._ADAM_ITEM.fields[n][1]) for n in optim._ADAM_ITEM.names]
    # what the groups hold is what the kernel gets
    p = torch.nn.Parameter(torch.zeros(2))
    opt = optim.LARS([dict(params=[p]), dict(params=[torch.nn.Parameter(torch.zeros(1))], layer_adaptation=False, eps=0.0)], lr=0.1,
                     momentum=0.9, weight_decay=5e-4, trust_coefficient=2e-3)
    h = opt._hyper()
    assert (h[0].lr, h[0].weight_decay, h[0].trust_coefficient, h[0].eps, h[0].adapt) == (0.1, 5e-4, 2e-3, 1e-8, 1)
    assert (h[1].eps, h[1].adapt, h[1].nesterov) == (0.0, 0, 0) and h[0].momentum == np.float32(0.9)
    h = optim.LAMB([p], betas=(0.9, 0.999), bias_correction=False)._hyper()[0]
    assert h.one_minus_beta2 == np.float32(1.0 - 0.999) != np.float32(1) - np.float32(0.999)
    assert (h.lr, h.beta1, h.beta2, h.bias_correction, h.adapt) == (1e-3, 0.9, 0.999, 0, 1)
    assert h.eps == np.float32(1e-6) and h.weight_decay == np.float32(0.01)
    # launches of a step: the hyperparameters travel by value, eight groups a launch
    assert [optim.step_launches(n) for n in (1, 8, 9, 16, 17)] == [1, 1, 2, 2, 3]


def test_are_torch_optimizers_with_the_documented_defaults():
    from gssd import optim
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    lars = optim.LARS([dict(params=ps[:1]), dict(params=ps[1:], layer_adaptation=False, lr=0.5)], max_grad_norm=1.0)
    sgd = torch.optim.SGD(ps)
    assert isinstance(lars, torch.optim.Optimizer) and isinstance(lars, optim.SGD)
    assert lars.defaults == dict(sgd.defaults, fused=None, trust_coefficient=1e-3, eps=1e-8, layer_adaptation=True)
    assert {k: v for k, v in lars.param_groups[0].items() if k != 'params'} == lars.defaults
    assert lars.param_groups[1]['layer_adaptation'] is False and lars.param_groups[1]['lr'] == 0.5
    assert lars.trust_ratio is None and lars.grad_norm is None and lars.max_grad_norm == 1.0 and lars.launches == 0
    lamb = optim.LAMB([dict(params=ps[:1]), dict(params=ps[1:], bias_correction=False)])
    adam = torch.optim.Adam(ps)
    assert isinstance(lamb, torch.optim.Optimizer) and isinstance(lamb, optim.Adam)
    assert lamb.defaults == dict(adam.defaults, eps=1e-6, weight_decay=0.01, bias_correction=True, layer_adaptation=True)
    assert (lamb.defaults['lr'], lamb.defaults['betas'], lamb.defaults['amsgrad']) == (1e-3, (0.9, 0.999), False)
    assert {k: v for k, v in lamb.param_groups[0].items() if k != 'params'} == lamb.defaults
    assert lamb.param_groups[1]['bias_correction'] is False and lamb.param_groups[1]['layer_adaptation'] is True
    assert lamb.trust_ratio is None and lamb.grad_norm is None and lamb.max_grad_norm is None
    late = torch.nn.Parameter(torch.zeros(1))
    lamb.add_param_group(dict(params=[late], layer_adaptation=False))           # a later group is filled the same way
    assert lamb.param_groups[2]['bias_correction'] is True and lamb.param_groups[2]['layer_adaptation'] is False
    # torch's argument checks, and the new keys'
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(nesterov=True), dict(trust_coefficient=-1e-3),
               dict(eps=-1e-8), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            optim.LARS(ps, **kw)
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.5)), dict(weight_decay=-1e-4),
               dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            optim.LAMB(ps, **kw)
    # ... also when they are edited in a group later (hyperparameters are read at every step)
    for key in ('trust_coefficient', 'eps'):
        opt = optim.LARS(ps)
        opt.param_groups[0][key] = -1.0
        with pytest.raises(ValueError, match=key):
            opt.step()


def test_what_is_not_implemented_says_so():
    from gssd import optim
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True), dict(lr=torch.tensor(0.1)),
               dict(trust_coefficient=torch.tensor(1e-3)), dict(eps=torch.tensor(1e-8))):
        with pytest.raises(NotImplementedError):
            optim.LARS(ps, **kw)
    for kw in (dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True), dict(capturable=True),
               dict(amsgrad=True), dict(lr=torch.tensor(1e-3)), dict(betas=(torch.tensor(0.9), torch.tensor(0.999)))):
        with pytest.raises(NotImplementedError):
            optim.LAMB(ps, **kw)
    # the group-level forms, at the step
    for cls, pairs in ((optim.LARS, (('maximize', True), ('foreach', True), ('fused', True), ('differentiable', True),
                                     ('lr', torch.tensor(0.1)), ('weight_decay', torch.tensor(0.1)),
                                     ('trust_coefficient', torch.tensor(1e-3)), ('eps', torch.tensor(1e-8)))),
                       (optim.LAMB, (('maximize', True), ('foreach', True), ('fused', True), ('capturable', True), ('amsgrad', True),
                                     ('decoupled_weight_decay', True), ('lr', torch.tensor(1e-3)), ('betas', (torch.tensor(0.9), 0.999)),
                                     ('eps', torch.tensor(1e-6))))):
        for key, v in pairs:
            q = torch.nn.Parameter(torch.zeros(3))
            q.grad = torch.ones(3)
            opt = cls([q])
            opt.param_groups[0][key] = v
            with pytest.raises(NotImplementedError):
                opt.step()
            assert len(opt.state) == 0 and opt.trust_ratio is None, (cls.__name__, key)


@pytest.mark.parametrize('name', ['LARS', 'LAMB'])
def test_table_key_follows_pointers_grads_and_state(name):
    from gssd import optim
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 2))
    kw = dict(momentum=0.9) if name == 'LARS' else {}
    opt = getattr(optim, name)([a, b], lr=1e-2, **kw)
    k0 = opt._table_key()
    assert k0 == opt._table_key() and len(opt.state) == 0          # asking creates no state
    a.grad = torch.zeros(3)
    k1 = opt._table_key()
    assert k1 != k0                                                 # a gradient appeared
    a.grad = torch.zeros(3)
    assert opt._table_key() != k1                                   # ... moved
    a.grad = None
    assert opt._table_key() == k0                                   # ... went away again
    b.data = torch.ones(5)
    k3 = opt._table_key()
    assert k3 != k0                                                 # the parameter's storage moved
    ref = torch.optim.SGD([a, b], lr=1e-2, momentum=0.9) if name == 'LARS' else torch.optim.Adam([a, b], lr=1e-2)
    b.grad = torch.ones(5)
    ref.step()
    b.grad = None
    opt.load_state_dict(ref.state_dict())
    k4 = opt._table_key()
    assert k4 != k3                                                 # loaded state
    moment = 'momentum_buffer' if name == 'LARS' else 'exp_avg_sq'
    opt.state[b][moment] = torch.zeros(5)
    assert opt._table_key() != k4                                   # one state tensor replaced
    k4 = opt._table_key()
    opt.add_param_group(dict(params=[c], lr=1e-3, layer_adaptation=False))
    k5 = opt._table_key()
    assert k5 != k4                                                 # a group was added
    opt.param_groups[1].update(lr=0.5, weight_decay=0.1, layer_adaptation=True)
    opt.param_groups[0].update(dict(trust_coefficient=0.1, eps=1e-3) if name == 'LARS' else dict(bias_correction=False, eps=1e-3))
    assert opt._table_key() == k5                                   # hyperparameters are not in the table


@pytest.mark.parametrize('name', ['LARS', 'LAMB'])
def test_refusals_need_no_device(name):
    from gssd import optim
    from gssd._lib import GssdError
    cls = getattr(optim, name)
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = cls([p], lr=1e-2, max_grad_norm=1.0)
    with pytest.raises(GssdError, match=r'params"\]\[0\].*no CPU fallback'):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(4)) and len(opt.state) == 0 and p._version == 0 and opt.grad_norm is None
    assert torch.equal(p.grad, torch.ones(4)) and opt.trust_ratio is None and opt.launches == 0
    # a step with nothing to do is a step: closure honoured, no table, no launch, no state
    q = torch.nn.Parameter(torch.zeros(4))
    calls = []
    opt = cls([q], lr=1e-2)
    assert opt.step(lambda: calls.append(torch.is_grad_enabled()) or 7.0) == 7.0 and calls == [True] and len(opt.state) == 0
    assert opt.trust_ratio is None and opt.launches == 0


def test_sgd_and_adam_checkpoints_load_with_the_extra_keys_filled():
    from gssd import optim
    ps = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]
    for p in ps:
        p.grad = torch.full_like(p, 0.5)
    groups = lambda: [dict(params=ps[:1]), dict(params=ps[1:], lr=0.01)]           # noqa: E731
    sgd = torch.optim.SGD(groups(), lr=0.1, momentum=0.9, weight_decay=5e-4)
    sgd.step()
    lars = optim.LARS(groups(), lr=0.3, trust_coefficient=2e-3, eps=1e-9, layer_adaptation=False)
    lars.load_state_dict(copy.deepcopy(sgd.state_dict()))
    for g, lr in zip(lars.param_groups, (0.1, 0.01)):                                # the checkpoint's values, the missing keys from defaults
        assert (g['lr'], g['momentum'], g['weight_decay']) == (lr, 0.9, 5e-4)
        assert (g['trust_coefficient'], g['eps'], g['layer_adaptation']) == (2e-3, 1e-9, False)
    assert all(torch.equal(lars.state[p]['momentum_buffer'], sgd.state[p]['momentum_buffer']) for p in ps)
    back = torch.optim.SGD(groups(), lr=0.7)
    back.load_state_dict(copy.deepcopy(lars.state_dict()))                           # and back: the extra keys travel, torch ignores them
    assert back.param_groups[0]['lr'] == 0.1 and back.param_groups[0]['trust_coefficient'] == 2e-3
    back.step()
    assert set(lars.state_dict()['param_groups'][0]) == set(sgd.state_dict()['param_groups'][0]) | set(LC.EXTRA['lars'])

    adam = torch.optim.Adam(groups(), lr=1e-3, betas=(0.8, 0.99), weight_decay=0.1)
    adam.step()
    lamb = optim.LAMB(groups(), lr=0.3, bias_correction=False)
    lamb.load_state_dict(copy.deepcopy(adam.state_dict()))
    for g, lr in zip(lamb.param_groups, (1e-3, 0.01)):
        assert (g['lr'], g['betas'], g['weight_decay'], g['eps']) == (lr, (0.8, 0.99), 0.1, 1e-8)
        assert (g['bias_correction'], g['layer_adaptation']) == (False, True)
    assert all(set(lamb.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'} and float(lamb.state[p]['step']) == 1 for p in ps)
    back = torch.optim.Adam(groups(), lr=0.7)
    back.load_state_dict(copy.deepcopy(lamb.state_dict()))
    assert back.param_groups[1]['lr'] == 0.01 and back.param_groups[0]['bias_correction'] is False
    back.step()
    assert all(float(back.state[p]['step']) == 2 for p in ps)
    assert set(lamb.state_dict()['param_groups'][0]) == set(adam.state_dict()['param_groups'][0]) | set(LC.EXTRA['lamb'])
    # a fresh LAMB's groups already carry every key torch.optim.Adam reads
    assert set(optim.LAMB(groups()).state_dict()['param_groups'][0]) == set(lamb.state_dict()['param_groups'][0])


# ---------------------------------------------------------------------------------------------- the yardstick
CH = 16            # a stand-in chunk size: the references know nothing of chunks, the sizes only have to be odd and uneven


def host_set(dtype):
    """Parameters with gradients on the CPU in ``dtype`` (values drawn as fp32, as the GPU tests' set): sizes around CH, one all-zero
    gradient, one all-zero weight, one parameter without a gradient."""
    rng = np.random.default_rng(2028)

    def draw(n, lo):
        return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(lo, 1, n)).astype(np.float32)).to(dtype)
    ns = [1, 3, 4, 5, CH - 1, CH, CH + 1, 3 * CH + 7, 2 * CH, 17 * CH + 1, 70, 33]
    ps = [torch.nn.Parameter(draw(n, -3)) for n in ns]
    for p in ps:
        p.grad = draw(p.numel(), -4)
    ps[-2].grad.zero_()
    with torch.no_grad():
        ps[-1].zero_()
    nograd = torch.nn.Parameter(draw(7, -3))
    return ps, nograd


def clip_coef(ps, clip):
    return 1.0 if clip is None else min(1.0, clip / (np.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps)) + 1e-6))


@pytest.mark.parametrize('algo,i', LC.ROWS, ids=[f'{a}{i}' for a, i in LC.ROWS])
def test_fp32_restatement_stays_inside_the_bounds(algo, i):
    """The check of the yardstick: the rules in plain fp32 torch operations, four steps, held to the bounds the kernels are held to."""
    kw, clip, layout = LC.row_args(algo, i)
    ps, nograd = host_set(torch.float32)
    opt = LC.Restated(algo, LC.layout_groups(ps, kw['lr'], layout, tail=[nograd]), max_grad_norm=clip, **kw)
    worst_t, worst_r = 0.0, 0.0
    for k in range(4):
        snap = LC.snapshot(algo, opt)
        c = clip_coef(ps, clip)
        opt.step()
        w, ratios = LC.check_step(algo, opt, snap, c, clip is not None, f'{algo} row {i} step {k}')
        worst_t, worst_r = max(worst_t, w), max(worst_r, LC.check_ratios(opt.trust_ratio, ratios, f'{algo} row {i} step {k}'))
        for p in ps:
            p.grad.mul_(-0.5)
    print(f'{algo} row {i}: worst error / bound {worst_t:.2f} (tensors) {worst_r:.2f} (ratios)')
    assert 0 < worst_t < 1


@pytest.mark.parametrize('algo,i', LC.ROWS, ids=[f'{a}{i}' for a, i in LC.ROWS])
def test_references_agree_with_the_restatement_in_float64(algo, i):
    """lars_ref / lamb_ref against the restatement run in float64: two statements of one rule, written apart, agree to rounding."""
    kw, clip, layout = LC.row_args(algo, i)
    ps, nograd = host_set(torch.float64)
    opt = LC.Restated(algo, LC.layout_groups(ps, kw['lr'], layout, tail=[nograd]), max_grad_norm=clip, **kw)
    for k in range(3):
        snap = LC.snapshot(algo, opt)
        c = clip_coef(ps, clip)
        opt.step()
        flat = [p for g in opt.param_groups for p in g['params']]
        for (p, g, p0, g0, s0, step0), r in zip(snap, opt.trust_ratio):
            if g0 is None:
                assert r is None and torch.equal(p.detach(), p0)
                continue
            if algo == 'lars':
                ref = LC.lars_ref(p0, g0, s0.get('momentum_buffer'), c, clip is not None, g)
                if g['momentum'] != 0:
                    torch.testing.assert_close(opt.state[p]['momentum_buffer'], ref['buf'], rtol=1e-12, atol=1e-300)
            else:
                ref = LC.lamb_ref(p0, g0, s0.get('exp_avg'), s0.get('exp_avg_sq'), step0 + 1, c, clip is not None, g)
                torch.testing.assert_close(opt.state[p]['exp_avg'], ref['m'], rtol=1e-12, atol=1e-300)
                torch.testing.assert_close(opt.state[p]['exp_avg_sq'], ref['v'], rtol=1e-12, atol=1e-300)
            assert abs(float(r) - ref['r']) <= 1e-12 * ref['r']
            scale = float(p0.abs().max()) + g['lr'] * ref['r'] * float(g0.abs().max() + 1)
            assert float((p.detach() - ref['p']).abs().max()) <= 1e-12 * scale
        assert len(flat) == len(opt.trust_ratio)
        for p in ps:
            p.grad.mul_(-0.5)


def test_zero_norms_fall_back_to_ratio_one():
    """||w|| = 0 and ||g|| = 0 (LAMB: ||u|| = 0, an all-zero gradient without weight decay) give r = 1 exactly, with no error allowed;
    an all-zero gradient under LARS leaves pure weight decay."""
    w, z = torch.tensor([0.5, -2.0, 3.0]), torch.zeros(3)
    g = torch.tensor([1e-2, 3e-2, -2e-2])
    kw, _, _ = LC.row_args('lars', 0)
    kw['momentum'] = 0.0
    for p0, g0 in ((w, z), (z, g)):
        ref = LC.lars_ref(p0, g0, None, 1.0, False, kw)
        assert ref['r'] == 1.0 and ref['rel_r'] == 0.0
        p = p0.clone()
        _, r = LC.lars_torch(p, g0.clone(), None, 1.0, kw)
        assert float(r) == 1.0
    ref = LC.lars_ref(w, z, None, 1.0, False, kw)
    assert torch.equal(ref['p'], w.double() * (1 - kw['lr'] * kw['weight_decay']))       # pure weight decay
    assert LC.lars_ref(w, g, None, 1.0, False, kw)['r'] != 1.0
    assert LC.lars_ref(w, g, None, 1.0, False, dict(kw, layer_adaptation=False))['r'] == 1.0
    kw, _, _ = LC.row_args('lamb', 2)
    assert kw['weight_decay'] == 0.0
    for p0, g0 in ((w, z), (z, g)):
        ref = LC.lamb_ref(p0, g0, None, None, 1, 1.0, False, kw)
        assert ref['r'] == 1.0 and ref['rel_r'] == 0.0
        p = p0.clone()
        assert float(LC.lamb_torch(p, g0.clone(), torch.zeros(3), torch.zeros(3), 1, 1.0, kw)) == 1.0
    assert torch.equal(LC.lamb_ref(w, z, None, None, 1, 1.0, False, kw)['p'], w.double())  # u = 0: nothing moves
    # with weight decay an all-zero gradient leaves u = wd w: the ratio is 1 / wd, not a fall-back
    ref = LC.lamb_ref(w, z, None, None, 1, 1.0, False, dict(kw, weight_decay=0.01))
    assert abs(ref['r'] - 100.0) < 1e-9 and ref['rel_r'] > 0
