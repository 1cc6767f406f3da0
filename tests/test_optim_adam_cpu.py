"""Host logic of gssd.optim.Adam / AdamW that needs no GPU: the ABI wiring of gssd_adam_step_f32 and the layout of its two structs, the
torch.optim.Optimizer surface against the installed torch's Adam / AdamW, the table key that decides when the device table is rebuilt,
and the refusals that are decided before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gssd_hip.h')

C_TYPES = {'float*': 8, 'const float*': 8, 'int64_t': 8, 'int32_t': 4, 'float': 4, 'double': 8}


def header_struct(name):
    """[(field, offset)] and the size of ``typedef struct name {...} name;`` in the header under the C layout rules (every member
    aligned to its own size, the struct to its largest member)."""
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef\s+struct\s+' + name + r'\s*\{(.*?)\}\s*' + name + r'\s*;', hdr, flags=re.S).group(1)
    fields, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        ctype, names = re.fullmatch(r'((?:const\s+)?\w+\s*\*?)\s*(.+)', decl, flags=re.S).groups()
        size = C_TYPES[re.sub(r'\s*\*', '*', ctype.strip())]
        for n in names.split(','):
            off = -(-off // size) * size
            fields.append((n.strip(), off))
            off += size
            align = max(align, size)
    return fields, -(-off // align) * align


def test_abi_carries_the_adam_entry_point():
    from gssd import _lib
    hdr = open(HEADER).read()
    n = 'gssd_adam_step_f32'
    assert re.search(r'\bint\s+' + n + r'\s*\(', hdr) and n in _lib.SIGNATURES
    i = _lib.lib.gssd_plan_fn_index(n.encode())
    assert i >= 0 and _lib.lib.gssd_plan_fn_nargs(i) == len(_lib.SIGNATURES[n][1]) - 1 == 10
    assert _lib.lib.gssd_abi_version() == 8
    # argument validation happens before anything touches a device
    hy = (_lib.AdamHyper * 1)()
    one = ctypes.c_void_p(16)                  # never dereferenced: every call below is refused
    assert _lib.lib.gssd_adam_step_f32(None, None, 1, None, 1, 1, None, 0, -1.0, None, None) == -1
    assert b'invalid argument' in _lib.lib.gssd_last_error()
    assert _lib.lib.gssd_adam_step_f32(None, one, 1, hy, 1, 1, None, 0, -1.0, None, None) == -1        # no items
    assert _lib.lib.gssd_adam_step_f32(one, None, 1, hy, 1, 1, None, 0, -1.0, None, None) == -1        # no chunks
    assert _lib.lib.gssd_adam_step_f32(one, one, 0, hy, 1, 1, None, 0, -1.0, None, None) == -1         # no work
    assert _lib.lib.gssd_adam_step_f32(one, one, 1, None, 1, 1, None, 0, -1.0, None, None) == -1       # no hyperparameters
    assert _lib.lib.gssd_adam_step_f32(one, one, 1, hy, 0, 1, None, 0, -1.0, None, None) == -1         # no groups
    assert _lib.lib.gssd_adam_step_f32(one, one, 1, hy, 1, 1, None, 0, 1.0, one, None) == -1           # clip without partial sums
    assert _lib.lib.gssd_adam_step_f32(one, one, 1, hy, 1, 1, one, 1, 1.0, None, None) == -1           # clip without norm_out


def test_struct_layouts_agree():
    from gssd import _lib, optim
    item, size = header_struct('gssd_adam_item')
    assert [n for n, _ in item] == ['p', 'g', 'm', 'v', 'vmax', 'n', 'group', 'flags', 't0']
    assert size == optim._ADAM_ITEM.itemsize == 64
    assert item == [(n, optim._ADAM_ITEM.fields[n][1]) for n in optim._ADAM_ITEM.names]
    assert [optim._ADAM_ITEM.fields[n][0].itemsize for n in optim._ADAM_ITEM.names] == [8, 8, 8, 8, 8, 8, 4, 4, 8]
    hyper, size = header_struct('gssd_adam_hyper')
    assert [n for n, _ in hyper] == ['lr', 'beta1', 'beta2', 'one_minus_beta1', 'one_minus_beta2', 'eps', 'weight_decay', 'amsgrad', 'decoupled']
    assert size == ctypes.sizeof(_lib.AdamHyper) == 48
    assert hyper == [(n, getattr(_lib.AdamHyper, n).offset) for n, _ in _lib.AdamHyper._fields_]
    # the chunk list is the SGD kernels': its struct is unchanged
    chunk, size = header_struct('gssd_sgd_chunk')
    assert size == optim._CHUNK.itemsize and chunk == [(n, optim._CHUNK.fields[n][1]) for n in optim._CHUNK.names]
    # 1 - beta is formed in double and rounded once: fp32 arithmetic on the rounded beta2 is 4.7e-5 off
    p = torch.nn.Parameter(torch.zeros(2))
    h = optim.Adam([p], betas=(0.9, 0.999))._hyper()[0]
    assert h.one_minus_beta2 == np.float32(1.0 - 0.999) != np.float32(1) - np.float32(0.999)
    assert h.one_minus_beta1 == np.float32(1.0 - 0.9) and h.beta2 == 0.999 and h.lr == 1e-3 and (h.amsgrad, h.decoupled) == (0, 0)
    assert optim.AdamW([p])._hyper()[0].decoupled == 1


def groups_of(ps):
    return [dict(params=ps[:1]), dict(params=ps[1:], lr=1e-4, betas=(0.5, 0.9), amsgrad=True)]


@pytest.mark.parametrize('name', ['Adam', 'AdamW'])
def test_is_a_torch_optimizer_with_torchs_defaults(name):
    from gssd import optim
    cls, ref_cls = getattr(optim, name), getattr(torch.optim, name)
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    for kw in (dict(), dict(lr=1e-2, betas=(0.8, 0.99), eps=1e-6, weight_decay=5e-4, amsgrad=True)):
        opt, ref = cls(groups_of(ps), max_grad_norm=1.0, **kw), ref_cls(groups_of(ps), **kw)
        assert isinstance(opt, torch.optim.Optimizer)
        assert opt.defaults == ref.defaults
        assert [{k: v for k, v in g.items() if k != 'params'} for g in opt.param_groups] == \
            [{k: v for k, v in g.items() if k != 'params'} for g in ref.param_groups]
        assert opt.state_dict() == ref.state_dict() and opt.grad_norm is None and opt.max_grad_norm == 1.0
    assert cls(ps).max_grad_norm is None
    # only __init__ and step are the classes' own
    public = {k for c in (optim.Adam, optim.AdamW) for k in vars(c) if not k.startswith('_')} | \
        {k for c in (optim.Adam, optim.AdamW) for k in vars(c) if k.startswith('__') and callable(vars(c)[k])}
    assert public == {'__init__', 'step'} and set(vars(optim.AdamW)) & {'__init__', 'step'} == {'__init__'}
    assert issubclass(optim.AdamW, optim.Adam)
    # torch's argument checks
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(-0.1, 0.999)), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)),
               dict(betas=(0.9, -0.5)), dict(weight_decay=-1e-4), dict(betas=(0, 0.999))):
        with pytest.raises(ValueError):
            cls(ps, **kw)
        with pytest.raises(ValueError):
            ref_cls(ps, **kw)
    with pytest.raises(ValueError):
        cls(ps, max_grad_norm=-1.0)


@pytest.mark.parametrize('name', ['Adam', 'AdamW'])
def test_what_is_not_implemented_says_so(name):
    from gssd import optim
    cls = getattr(optim, name)
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True), dict(capturable=True),
               dict(lr=torch.tensor(1e-3)), dict(betas=(torch.tensor(0.9), torch.tensor(0.999)))):
        with pytest.raises(NotImplementedError):
            cls(ps, **kw)
    # the group-level forms, at the step (hyperparameters are read from param_groups every time)
    for key, v in (('maximize', True), ('foreach', True), ('fused', True), ('differentiable', True), ('capturable', True),
                   ('lr', torch.tensor(1e-3)), ('betas', (torch.tensor(0.9), 0.999)), ('betas', (0.9, torch.tensor(0.999)))):
        opt = cls(ps)
        opt.param_groups[0][key] = v
        with pytest.raises(NotImplementedError):
            opt.step()
        assert len(opt.state) == 0


def test_table_key_follows_pointers_grads_state_and_groups():
    from gssd import optim
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 2))
    opt = optim.Adam([a, b], lr=1e-2)
    k0 = opt._table_key()
    assert k0 == opt._table_key() and len(opt.state) == 0          # asking creates no state
    a.grad = torch.zeros(3)
    k1 = opt._table_key()
    assert k1 != k0                                                 # a gradient appeared
    a.grad = torch.zeros(3)
    k2 = opt._table_key()
    assert k2 != k1                                                 # ... moved
    a.grad = None
    assert opt._table_key() == k0                                   # ... went away again
    b.data = torch.ones(5)
    k3 = opt._table_key()
    assert k3 != k0                                                 # the parameter's storage moved
    # loaded state: what torch.optim.Adam saved for the same parameters
    ref = torch.optim.Adam([a, b], lr=1e-2)
    b.grad = torch.ones(5)
    ref.step()
    b.grad = None
    opt.load_state_dict(ref.state_dict())
    k4 = opt._table_key()
    assert k4 != k3 and set(opt.state[b]) == {'step', 'exp_avg', 'exp_avg_sq'}
    opt.state[b]['exp_avg_sq'] = torch.zeros(5)
    k4b = opt._table_key()
    assert k4b != k4                                                # one moment tensor replaced
    opt.state[b]['step'] = torch.tensor(7.0)
    k4c = opt._table_key()
    assert k4c != k4b                                               # another step tensor: the items' t0 must be formed again
    opt.add_param_group(dict(params=[c], lr=1e-3))
    k5 = opt._table_key()
    assert k5 != k4c and len(k5) == len(k4c) + 2                    # a group was added
    c.grad = torch.zeros(2)
    k6 = opt._table_key()
    c.grad.data = torch.zeros(2, dtype=torch.float64)
    assert opt._table_key() != k6                                   # another dtype (the pointer may or may not have moved)
    c.grad = None
    opt.param_groups[1]['amsgrad'] = True
    assert opt._table_key() != k5                                   # amsgrad flipped: the group's items gain max_exp_avg_sq
    opt.param_groups[1]['amsgrad'] = False
    opt.param_groups[1].update(lr=0.5, betas=(0.5, 0.9), eps=1e-3, weight_decay=0.1)
    assert opt._table_key() == k5                                   # hyperparameters are not in the table


@pytest.mark.parametrize('name', ['Adam', 'AdamW'])
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
    assert torch.equal(p.grad, torch.ones(4))
    # a step with nothing to do is a step: closure honoured, no table, no launch, no state
    q = torch.nn.Parameter(torch.zeros(4))
    calls = []
    opt = cls([q], lr=1e-2)
    assert opt.step(lambda: calls.append(torch.is_grad_enabled()) or 7.0) == 7.0 and calls == [True] and len(opt.state) == 0
