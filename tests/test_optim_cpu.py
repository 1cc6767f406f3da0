"""Host logic of gssd.optim that needs no GPU: the chunk list, the table key that decides when the device table is rebuilt, the
torch.optim.Optimizer surface, the ABI wiring of the three entry points, and the refusals that are decided before any launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def numels(ch):
    return [1, 3, 4, 5, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 7, 0]


@pytest.mark.parametrize('chunk', [None, 64])
def test_chunks_cover_every_element_once(chunk):
    from gssd import optim
    ch = chunk or optim.CHUNK
    ns = numels(ch)
    item, off = optim.build_chunks(ns, chunk)
    assert item.dtype == np.int32 and off.dtype == np.int64 and len(item) == len(off) == sum(-(-n // ch) for n in ns)
    seen = [np.zeros(n, np.int32) for n in ns]
    for i, o in zip(item.tolist(), off.tolist()):
        assert 0 <= o < ns[i] and o % ch == 0             # inside its item (so an empty item has no chunk), on the chunk grid
        seen[i][o:min(o + ch, ns[i])] += 1                # [o, min(o + ch, n)): what the kernels touch -- never another item
    assert all((s == 1).all() for s in seen)
    assert 11 not in item.tolist() and np.array_equal(item, np.sort(item))
    assert optim.build_chunks([])[0].size == 0 and optim.build_chunks([0, 0])[0].size == 0


def test_chunk_size_and_partial_count_come_from_the_library():
    from gssd import _lib, optim
    lib = _lib.lib
    assert optim.CHUNK == lib.gssd_optim_chunk_elems() and optim.CHUNK % 1024 == 0
    assert lib.gssd_optim_sumsq_blocks(0) == 0 and lib.gssd_optim_sumsq_blocks(5) == 5
    cap = lib.gssd_optim_sumsq_blocks(10 ** 6)
    assert 0 < cap < 10 ** 6 and lib.gssd_optim_sumsq_blocks(cap + 1) == cap
    # table rows as numpy writes them == the header's structs under the C packing rules
    assert optim._ITEM.itemsize == 4 * 8 + 2 * 4 and optim._CHUNK.itemsize == 8 + 2 * 4
    assert [optim._ITEM.fields[k][1] for k in ('p', 'g', 'buf', 'n', 'group', 'flags')] == [0, 8, 16, 24, 32, 36]
    assert [optim._CHUNK.fields[k][1] for k in ('off', 'item')] == [0, 8]
    assert ctypes.sizeof(_lib.SgdHyper) == 20


def test_abi_carries_the_optimizer_entry_points():
    from gssd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read()
    names = ['gssd_grad_sumsq_f32', 'gssd_sgd_step_f32', 'gssd_grad_scale_clip_f32']
    for n in names:
        assert re.search(r'\bint\s+' + n + r'\s*\(', hdr) and n in _lib.SIGNATURES
        i = _lib.lib.gssd_plan_fn_index(n.encode())
        assert i >= 0 and _lib.lib.gssd_plan_fn_nargs(i) == len(_lib.SIGNATURES[n][1]) - 1
    assert _lib.lib.gssd_abi_version() == 8
    # argument validation happens before anything touches a device
    assert _lib.lib.gssd_grad_sumsq_f32(None, None, 0, None, None) == -1
    assert _lib.lib.gssd_sgd_step_f32(None, None, 1, None, 1, None, 0, -1.0, None, None) == -1
    assert _lib.lib.gssd_grad_scale_clip_f32(None, None, 1, None, 1, 1.0, None, None) == -1


def test_is_a_torch_optimizer_with_torchs_defaults():
    from gssd import optim
    ps = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(2, 2))]
    opt = optim.SGD([dict(params=ps[:1]), dict(params=ps[1:], lr=1e-3)], lr=1e-2, momentum=0.9, weight_decay=5e-4, max_grad_norm=1.0)
    ref = torch.optim.SGD([dict(params=ps[:1]), dict(params=ps[1:], lr=1e-3)], lr=1e-2, momentum=0.9, weight_decay=5e-4)
    assert isinstance(opt, torch.optim.Optimizer)
    assert opt.defaults == ref.defaults
    assert [{k: v for k, v in g.items() if k != 'params'} for g in opt.param_groups] == \
        [{k: v for k, v in g.items() if k != 'params'} for g in ref.param_groups]
    assert opt.state_dict() == ref.state_dict() and opt.grad_norm is None and opt.max_grad_norm == 1.0
    # only __init__ and step are this class's own
    for name in ('zero_grad', 'add_param_group', 'state_dict', 'load_state_dict'):
        assert name not in vars(optim.SGD)
    # torch's argument checks
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError):
            optim.SGD(ps, **{'lr': 1e-2, **kw})
        with pytest.raises(ValueError):
            torch.optim.SGD(ps, **{'lr': 1e-2, **kw})
    for kw in (dict(maximize=True), dict(foreach=True), dict(fused=True), dict(differentiable=True)):
        with pytest.raises(NotImplementedError):
            optim.SGD(ps, lr=1e-2, **kw)


def test_table_key_follows_pointers_grads_buffers_and_groups():
    from gssd import optim
    a, b, c = (torch.nn.Parameter(torch.zeros(n)) for n in (3, 5, 2))
    opt = optim.SGD([a, b], lr=1e-2, momentum=0.9)
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
    opt.state[b]['momentum_buffer'] = torch.zeros(5)
    k4 = opt._table_key()
    assert k4 != k3                                                 # a buffer appeared (load_state_dict)
    opt.add_param_group(dict(params=[c], lr=1e-3))
    k5 = opt._table_key()
    assert k5 != k4 and len(k5) == len(k4) + 2                      # a group was added
    c.grad = torch.zeros(2)
    k6 = opt._table_key()
    c.grad.data = torch.zeros(2, dtype=torch.float64)
    assert opt._table_key() != k6                                   # another dtype (the pointer may or may not have moved)
    c.grad = None
    opt.param_groups[1]['momentum'] = 0
    assert opt._table_key() != k5                                   # a group stopped keeping momentum: its items lose their buffers
    opt.param_groups[1]['momentum'] = 0.9
    opt.param_groups[1]['lr'] = 0.5
    assert opt._table_key() == k5                                   # hyperparameters are not in the table


def test_refusals_need_no_device():
    from gssd import optim
    from gssd._lib import GssdError
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    opt = optim.SGD([p], lr=1e-2, momentum=0.9)
    with pytest.raises(GssdError, match=r'params"\]\[0\].*no CPU fallback'):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(4)) and 'momentum_buffer' not in opt.state.get(p, {})
    with pytest.raises(GssdError, match='no CPU fallback'):
        optim.clip_grad_norm_([p], 1.0)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_([p], 1.0, norm_type=float('inf'))
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    assert torch.equal(p.grad, torch.ones(4))
    # a step with nothing to do is a step: closure honoured, no table, no launch
    q = torch.nn.Parameter(torch.zeros(4))
    calls = []
    assert optim.SGD([q], lr=1e-2).step(lambda: calls.append(torch.is_grad_enabled()) or 7.0) == 7.0 and calls == [True]
