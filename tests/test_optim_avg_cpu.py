"""Host logic of gssd.optim.AveragedModel / update_bn that needs no GPU: the ABI wiring of gssd_avg_update_f32 and the layout of its
item struct, the torch.optim.swa_utils.AveragedModel surface against the installed torch, the table key that decides when the device
table is rebuilt, the refusals that are decided before any launch, and the yardstick of tests/optim_avg_common.py held against torch's
own AveragedModel in fp32 on the CPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel as TorchAveragedModel, get_ema_multi_avg_fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from optim_avg_common import AvgSet, check_update, numels, repoint, snapshot      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gssd_hip.h')

C_TYPES = {'void*': 8, 'const void*': 8, 'float*': 8, 'const float*': 8, 'int64_t': 8, 'int32_t': 4, 'float': 4, 'double': 8}


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


class Small(torch.nn.Module):
    """Parameters, float buffers (a BatchNorm's and one of its own) and the BatchNorm's int64 counter."""

    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(3, 4)
        self.bn = torch.nn.BatchNorm1d(4)
        self.register_buffer('scale', torch.full((2,), 0.5))

    def forward(self, x):
        return self.bn(self.lin(x)) * self.scale[0]


def test_abi_carries_the_avg_entry_point():
    from gssd import _lib
    hdr = open(HEADER).read()
    n = 'gssd_avg_update_f32'
    assert re.search(r'\bint\s+' + n + r'\s*\(', hdr) and n in _lib.SIGNATURES
    i = _lib.lib.gssd_plan_fn_index(n.encode())
    assert i >= 0 and _lib.lib.gssd_plan_fn_nargs(i) == len(_lib.SIGNATURES[n][1]) - 1 == 6
    assert _lib.lib.gssd_abi_version() == 8
    # argument validation happens before anything touches a device
    one = ctypes.c_void_p(16)                  # never dereferenced: every call below is refused
    f = _lib.lib.gssd_avg_update_f32
    for args in ((None, one, 1, 0.5, one, one),        # no item table
                 (one, None, 1, 0.5, one, one),        # no chunk list
                 (one, one, 0, 0.5, one, one),         # no work
                 (one, one, 1, 1.5, one, one),         # w > 1
                 (one, one, 1, float(np.nextafter(np.float32(1), np.float32(2))), one, one),
                 (one, one, 1, float('nan'), one, one),
                 (one, one, 1, -1.0, None, one),       # no count
                 (one, one, 1, -1.0, one, None)):      # no ticket word
        assert f(*args, None) == -1 and b'invalid argument' in _lib.lib.gssd_last_error(), args


def test_struct_layout_agrees():
    from gssd import optim
    item, size = header_struct('gssd_avg_item')
    assert [n for n, _ in item] == ['dst', 'src', 'n', 'kind', 'reserved']
    assert size == optim._AVG_ITEM.itemsize == 32
    assert item == [(n, optim._AVG_ITEM.fields[n][1]) for n in optim._AVG_ITEM.names]
    assert [optim._AVG_ITEM.fields[n][0].itemsize for n in optim._AVG_ITEM.names] == [8, 8, 8, 4, 4]
    hdr = open(HEADER).read()
    for name, v in (('LERP', optim.AVG_LERP), ('COPY32', optim.AVG_COPY32), ('COPY64', optim.AVG_COPY64)):
        assert int(re.search(r'#define\s+GSSD_AVG_' + name + r'\s+(\d+)', hdr).group(1)) == v
    # the chunk list is the SGD kernels': its struct is unchanged
    chunk, size = header_struct('gssd_sgd_chunk')
    assert size == optim._CHUNK.itemsize and chunk == [(n, optim._CHUNK.fields[n][1]) for n in optim._CHUNK.names]


@pytest.mark.parametrize('use_buffers', [False, True])
def test_surface_is_torchs(use_buffers):
    from gssd import optim
    torch.manual_seed(3)
    model = Small()
    ours = optim.AveragedModel(model, use_buffers=use_buffers, ema_decay=0.99)
    ref = TorchAveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.99), use_buffers=use_buffers)
    assert isinstance(ours, torch.nn.Module) and ours.module is not model and isinstance(ours.module, Small)
    sd, sd_ref = ours.state_dict(), ref.state_dict()
    assert list(sd) == list(sd_ref) and list(sd)[0] == 'n_averaged'
    assert [(v.dtype, v.shape) for v in sd.values()] == [(v.dtype, v.shape) for v in sd_ref.values()]
    assert ours.n_averaged.dtype == torch.int64 and ours.n_averaged.shape == () and int(ours.n_averaged) == 0
    assert ours.n_averaged.device == model.lin.weight.device and ours.use_buffers == use_buffers
    # checkpoints go either way
    ref.update_parameters(model)
    with torch.no_grad():
        model.lin.weight.mul_(2.0)
    ref.update_parameters(model)
    ours.load_state_dict(ref.state_dict())
    assert int(ours.n_averaged) == 2 and all(torch.equal(a, b) for a, b in zip(ours.state_dict().values(), ref.state_dict().values()))
    with torch.no_grad():
        ours.module.lin.bias.add_(1.0)
        ours.n_averaged.add_(5)
    ref.load_state_dict(ours.state_dict())
    assert int(ref.n_averaged) == 7 and torch.equal(ref.module.lin.bias, ours.module.lin.bias)
    # forward delegates to the copy
    x = torch.randn(5, 3)
    ours.eval(), ref.eval()
    assert torch.equal(ours(x), ref(x)) and torch.equal(ours(x), ours.module(x))


def test_constructor_arguments():
    from gssd import optim
    model = Small()
    assert optim.AveragedModel(model).ema_decay is None and optim.AveragedModel(model)._weight() == -1.0       # torch's default: SWA
    for bad in (-0.1, 1.0001, float('nan')):
        with pytest.raises(ValueError):
            optim.AveragedModel(model, ema_decay=bad)
        if bad == bad:
            with pytest.raises(ValueError):
                get_ema_multi_avg_fn(bad)
    with pytest.raises(NotImplementedError):
        optim.AveragedModel(model, ema_decay=torch.tensor(0.9))
    with pytest.raises(NotImplementedError, match='ema_decay'):
        optim.AveragedModel(model, avg_fn=lambda a, b, n: a)
    with pytest.raises(NotImplementedError, match='ema_decay'):
        optim.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(0.9))
    assert optim.AveragedModel(model, device='cpu').n_averaged.device.type == 'cpu'
    assert optim.AveragedModel(model, device=torch.device('cpu')).module.lin.weight.device.type == 'cpu'
    with pytest.raises(ValueError, match='device'):
        optim.AveragedModel(model, device='cuda:0')
    # ema_decay is a plain attribute read at every update; the weight is 1 - decay formed in double and rounded once by the binding
    avg = optim.AveragedModel(model, ema_decay=0.999)
    assert avg._weight() == 1.0 - 0.999
    assert ctypes.c_float(avg._weight()).value == np.float32(1.0 - 0.999) != np.float32(1) - np.float32(0.999)
    avg.ema_decay = 0.5
    assert avg._weight() == 0.5
    avg.ema_decay = None
    assert avg._weight() == -1.0
    for bad, exc in ((1.5, ValueError), (-1e-9, ValueError), (torch.tensor(0.5), NotImplementedError)):
        avg.ema_decay = bad
        keep = snapshot(avg)
        with pytest.raises(exc):
            avg.update_parameters(model)
        assert all(torch.equal(a, b) for a, b in zip(snapshot(avg), keep))


@pytest.mark.parametrize('use_buffers', [False, True])
def test_cpu_model_is_refused_before_anything_is_written(use_buffers):
    from gssd import optim
    from gssd._lib import GssdError
    model = Small()
    avg = optim.AveragedModel(model, use_buffers=use_buffers, ema_decay=0.9)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    tensors = list(avg.parameters()) + list(avg.buffers())
    keep, versions = snapshot(avg), [t._version for t in tensors]
    with pytest.raises(GssdError, match='no CPU fallback'):
        avg.update_parameters(model)
    assert all(torch.equal(a, b) for a, b in zip(snapshot(avg), keep)) and int(avg.n_averaged) == 0
    assert [t._version for t in tensors] == versions


def test_mismatched_models_are_refused():
    from gssd import optim
    from gssd._lib import GssdError
    model = Small()
    avg = optim.AveragedModel(model)
    with pytest.raises(GssdError, match='parameters'):
        avg.update_parameters(torch.nn.Linear(3, 4))


def test_table_key_follows_storage_and_use_buffers():
    from gssd import optim
    model = Small()
    avg = optim.AveragedModel(model, ema_decay=0.9)
    k0 = avg._table_key(model)
    assert k0 == avg._table_key(model)
    avg.ema_decay = 0.5
    assert avg._table_key(model) == k0                              # the weight is a launch argument, not in the table
    avg.ema_decay = None
    assert avg._table_key(model) == k0
    model.lin.weight.data = torch.zeros(4, 3)
    k1 = avg._table_key(model)
    assert k1 != k0                                                 # a source storage moved
    avg.module.lin.bias.data = torch.zeros(4)
    k2 = avg._table_key(model)
    assert k2 != k1                                                 # an averaged storage moved
    model.bn.running_mean = torch.zeros(4)
    k3 = avg._table_key(model)
    assert k3 != k2                                                 # a buffer was replaced
    avg.use_buffers = True
    k4 = avg._table_key(model)
    assert k4 != k3 and len(k4) == len(k3)                          # float buffers turn from copies into averages
    kinds = [k for k, *_ in avg._pairs(model)]
    assert kinds == [optim.AVG_LERP] * 4 + [optim.AVG_LERP] * 3 + [optim.AVG_COPY64]      # (scale, running_mean, running_var; the counter)
    avg.use_buffers = False
    assert [k for k, *_ in avg._pairs(model)] == [optim.AVG_LERP] * 4 + [optim.AVG_COPY32] * 3 + [optim.AVG_COPY64]


def test_a_module_registered_twice_yields_one_item_per_tensor():
    from gssd import optim

    class Twice(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.BatchNorm1d(3)
            self.b = self.a                                         # as fuse_31 ... fuse_61 of the SSD are
            self.c = torch.nn.Linear(3, 3, bias=False)
    model = Twice()
    avg = optim.AveragedModel(model, use_buffers=True)
    pairs = avg._pairs(model)
    assert len(pairs) == 3 + 3 and len({id(a.untyped_storage()) for _, a, _, _ in pairs}) == 6
    assert avg.module.a is avg.module.b
    for _, a, b, _ in pairs:
        assert a.shape == b.shape and a.data_ptr() != b.data_ptr()
    # the pairing is that of parameters() and buffers(), on the real network too (fuse_31 ... fuse_61 are registered twice)
    from models.ssd_multiphase_custom_group import build_ssd
    for m in (model, Small(), build_ssd('train', 300, 2, True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)):
        ps, bs = optim._model_tensors(m)
        want_p, want_b = list(m.parameters()), list(m.buffers())
        assert len(ps) == len(want_p) and all(a is b for a, b in zip(ps, want_p))
        assert len(bs) == len(want_b) and all(a is b for a, b in zip(bs, want_b))


def test_update_bn_restores_momenta_and_mode_when_the_forward_raises():
    from gssd import optim
    from gssd._lib import GssdError
    from models.ssd_multiphase_custom_group import build_ssd
    net = build_ssd('train', 300, 2, True, 4, 4, 1, True, False, False, 0, 1, False, False, 1)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert len(bns) > 10
    for i, m in enumerate(bns):
        m.momentum = 0.05 + 0.001 * i
    net.eval()
    with pytest.raises(GssdError, match='no CPU fallback'):
        optim.update_bn([torch.zeros(1, 12, 300, 300)], net)
    assert not net.training and [m.momentum for m in bns] == [0.05 + 0.001 * i for i in range(len(bns))]
    net.train()
    with pytest.raises(GssdError):
        optim.update_bn([[torch.zeros(1, 12, 300, 300), 'labels']], net, device='cpu')
    assert net.training and [m.momentum for m in bns] == [0.05 + 0.001 * i for i in range(len(bns))]
    # a model without BatchNorm: nothing to do, the loader is not touched (torch's rule)
    assert optim.update_bn(iter(()), torch.nn.Linear(2, 2)) is None


@pytest.mark.parametrize('decay', [0.999, 0.5, None], ids=['ema0.999', 'ema0.5', 'swa'])
@pytest.mark.parametrize('use_buffers', [False, True])
def test_yardstick_holds_for_torch_on_the_cpu(decay, use_buffers):
    """torch's AveragedModel in fp32 on the CPU, counts 0 ... 4, on the GPU module's numels, stays within the bound."""
    from gssd import optim
    ch = optim.CHUNK
    assert numels(ch)[7:10] == [ch - 1, ch, ch + 1]
    src = AvgSet('cpu', ch)
    kw = dict(use_buffers=use_buffers) if decay is None else dict(use_buffers=use_buffers, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg = repoint_torch(TorchAveragedModel(src, **kw))
    n_par = len(list(src.parameters()))
    worst = 0.0
    for n in range(5):
        a0, b = snapshot(avg.module), snapshot(src)
        avg.update_parameters(src)
        a1 = snapshot(avg.module)
        for i, (x0, y, x1) in enumerate(zip(a0, b, a1)):
            if i < n_par or (use_buffers and x0.dtype == torch.float32):
                worst = max(worst, check_update(x0, y, x1, n, decay, f'count {n}, tensor {i}'))
            elif not use_buffers:
                assert torch.equal(x1, y)
        assert int(avg.n_averaged) == n + 1
        src.perturb()
    print(f'torch on the CPU, decay {decay}, use_buffers {use_buffers}: worst error / bound {worst:.3f}')
    assert worst > 0.0


def repoint_torch(avg):
    repoint(avg.module)
    return avg
