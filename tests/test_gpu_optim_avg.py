"""GPU tests of gssd.optim.AveragedModel / update_bn (csrc/optim_avg.hip): torch.optim.swa_utils.AveragedModel's update, EMA or the
equal SWA average, in one launch with the update count on the device, against float64.

The parameter set (tests/optim_avg_common.py) has the optimizer tests' numels [1, 3, 4, 5, 63, 64, 65, CH-1, CH, CH+1, 3*CH+7, 0], the
source tensors slices of one flat tensor laid end to end, the averaged ones re-pointed at slices of a second flat tensor that starts at
element 1 (aligned / misaligned and misaligned / misaligned pairs: the element path), float buffers of 1, 5 and CH+1 elements in
allocations of their own (aligned / aligned: the vector path with a full chunk and a tail) and a 0-dim int64 buffer.  A second layout
leaves the averaged parameters where deepcopy put them, each in its own allocation, so parameters take the vector path too.

Yardstick: optim_avg_common (one update, teacher-forced in float64 from the device's own fp32 a, b and the count before the launch).
A torch AveragedModel twin on the device takes the same updates from the same state (it is set to ours before every update: the bound
is that of ONE update) and must lie within the same bound of ours; the same assertion against float64 runs on the twin itself as a
check of the yardstick.
"""
import os
import sys

import pytest
import torch
from torch.optim.swa_utils import AveragedModel as TorchAveragedModel, get_ema_multi_avg_fn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev, rel, TOL, NETS)
from gpu_common import synth                  # noqa: E402
from optim_avg_common import AvgSet, check_update, lerp64, repoint, snapshot, weight64      # noqa: E402

pytestmark = pytest.mark.gpu

DECAYS = [0.999, 0.9, 0.5, 0.0, 1.0, None]    # None: the SWA rule


def chunk():
    from gssd import optim
    return optim.CHUNK


def make(dev, decay, use_buffers, repointed=True):
    """(source, ours, torch's twin), all starting from the same values."""
    from gssd import optim
    src = AvgSet(dev, chunk())
    ours = optim.AveragedModel(src, ema_decay=decay, use_buffers=use_buffers)
    kw = {} if decay is None else dict(multi_avg_fn=get_ema_multi_avg_fn(decay))
    if decay is None and use_buffers:
        # torch's default SWA function cannot take the int64 buffer on the device (its _foreach_addcdiv_ refuses integer division):
        # the twin gets the formula of torch's documentation as avg_fn, which handles every tensor by itself
        kw = dict(avg_fn=lambda averaged, current, num_averaged: averaged + (current - averaged) / (num_averaged + 1))
    twin = TorchAveragedModel(src, device=dev, use_buffers=use_buffers, **kw)
    if repointed:
        repoint(ours.module)
    return src, ours, twin


def lerped(module, use_buffers):
    """Per tensor of parameters() + buffers(): is it averaged (else: copied)?"""
    n_par = len(list(module.parameters()))
    return [True] * n_par + [use_buffers and b.dtype == torch.float32 for b in module.buffers()]


@torch.no_grad()
def sync_twin(twin, ours):
    for t, o in zip(list(twin.module.parameters()) + list(twin.module.buffers()), list(ours.module.parameters()) + list(ours.module.buffers())):
        t.copy_(o)
    twin.n_averaged.copy_(ours.n_averaged)


def one_update(src, ours, twin, n, decay, use_buffers, tag):
    """One update of ours (and of the twin, from ours' state) with the count ``n`` before it, checked; returns worst ratios (ours, twin)."""
    kinds = lerped(ours.module, use_buffers)
    tensors = list(ours.module.parameters()) + list(ours.module.buffers())
    a0, b = snapshot(ours.module), snapshot(src)
    versions = [t._version for t in tensors] + [ours.n_averaged._version]
    if twin is not None:
        sync_twin(twin, ours)
        twin.update_parameters(src)
    ours.update_parameters(src)
    a1 = snapshot(ours.module)
    t1 = snapshot(twin.module) if twin is not None else [None] * len(a1)
    assert all(torch.equal(x, y) for x, y in zip(snapshot(src), b)), f'{tag}: the source is only read'
    worst = [0.0, 0.0]
    for i, (x0, y, x1, z1, avg) in enumerate(zip(a0, b, a1, t1, kinds)):
        what = f'{tag}, tensor {i}'
        if not avg:
            assert torch.equal(x1, y) and x1.dtype == y.dtype, f'{what}: a copied tensor equals its source'
            continue
        worst[0] = max(worst[0], check_update(x0, y, x1, n, decay, what))
        if z1 is not None:
            worst[1] = max(worst[1], check_update(x0, y, z1, n, decay, what + ' (torch twin)'))
            if x0.numel() and n != 0 and decay not in (0.0, 1.0):
                w = weight64(decay, n)
                r = lerp64(x0.double(), y.double(), w)
                tol = 2.0 ** -23 * r.abs() + 2.0 ** -21 * w * (y.double() - x0.double()).abs() + 1e-38
                assert bool(((x1.double() - z1.double()).abs() <= tol).all()), f'{what}: ours vs torch twin'
            else:
                assert torch.equal(x1, z1), f'{what}: ours vs torch twin'
    for t, v in zip(tensors + [ours.n_averaged], versions):      # the version counter moves with the data, and only then
        assert (t._version > v) == (t.numel() > 0), tag
    return worst


@pytest.mark.parametrize('use_buffers', [False, True], ids=['sync_buffers', 'avg_buffers'])
@pytest.mark.parametrize('decay', DECAYS, ids=[f'ema{d}' if d is not None else 'swa' for d in DECAYS])
def test_update_matches_float64(dev, decay, use_buffers):
    src, ours, twin = make(dev, decay, use_buffers)
    pairs = ours._pairs(src)
    assert {(b.data_ptr() % 16 == 0, a.data_ptr() % 16 == 0) for _, a, b, _ in pairs if a.numel() > 4} == {(True, False), (False, False), (True, True)}
    counts, worst = [], []
    for n in range(4):
        worst.append(one_update(src, ours, twin, n, decay, use_buffers, f'decay {decay}, update {n}'))
        counts.append(ours.n_averaged.clone())
        src.perturb()
    assert torch.stack(counts).tolist() == [1, 2, 3, 4] and int(twin.n_averaged) == 4       # the one host read of the count
    print(f'decay {decay}, use_buffers {use_buffers}: worst error / bound per update (ours, torch)', [(f'{a:.2f}', f'{b:.2f}') for a, b in worst])


@pytest.mark.parametrize('decay', [0.9, None], ids=['ema0.9', 'swa'])
def test_vector_path_on_parameters(dev, decay):
    """The averaged parameters where deepcopy put them (16-byte aligned allocations): every source slice at a multiple of four elements
    makes an aligned / aligned pair, CH, CH + 1 and 64 among them."""
    src, ours, twin = make(dev, decay, True, repointed=False)
    both = [a.numel() for _, a, b, _ in ours._pairs(src) if a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0]
    ch = chunk()
    assert {64, 65, ch, ch + 1} <= set(both)
    for n in range(3):
        one_update(src, ours, twin, n, decay, True, f'aligned, decay {decay}, update {n}')
        src.perturb()
    assert int(ours.n_averaged) == 3


def test_count_lives_on_the_device(dev):
    """n_averaged.zero_() between two updates makes the next one a bitwise copy and leaves the count at 1; a count set by hand is the
    SWA rule's n.  No host mirror: the class never reads it."""
    src, ours, _ = make(dev, None, False)
    for n in range(3):
        one_update(src, ours, None, n, None, False, f'update {n}')
        src.perturb()
    ours.n_averaged.zero_()
    one_update(src, ours, None, 0, None, False, 'after zero_()')             # (n = 0: check_update asserts the bitwise copy)
    c1 = ours.n_averaged.clone()
    src.perturb()
    ours.n_averaged.fill_(9)
    one_update(src, ours, None, 9, None, False, 'count set to 9')            # w = 1 / 10
    assert int(c1) == 1 and int(ours.n_averaged) == 10
    # the same for the EMA rule: its first update is a copy whatever the decay
    src, ours, _ = make(dev, 0.999, True)
    one_update(src, ours, None, 0, 0.999, True, 'ema, first')
    src.perturb()
    one_update(src, ours, None, 1, 0.999, True, 'ema, second')
    ours.n_averaged.zero_()
    src.perturb()
    one_update(src, ours, None, 0, 0.999, True, 'ema, after zero_()')
    assert int(ours.n_averaged) == 1


def test_update_reads_nothing_back(dev):
    """With the table built (its upload is a host-to-device copy), an update under set_sync_debug_mode('error') raises nothing --
    a changed ema_decay included."""
    src, ours, _ = make(dev, 0.9, True)
    ours.update_parameters(src)
    src.perturb()
    a0, b = snapshot(ours.module), snapshot(src)
    torch.cuda.set_sync_debug_mode('error')
    try:
        ours.ema_decay = 0.75
        ours.update_parameters(src)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    for x0, y, x1, avg in zip(a0, b, snapshot(ours.module), lerped(ours.module, True)):
        if avg:
            check_update(x0, y, x1, 1, 0.75, 'under sync debug mode')
    assert int(ours.n_averaged) == 2


def test_table_follows_replaced_storage(dev):
    src, ours, _ = make(dev, 0.5, False)
    one_update(src, ours, None, 0, 0.5, False, 'first')
    table = ours._table[1]
    src.perturb()
    one_update(src, ours, None, 1, 0.5, False, 'second')
    assert ours._table[1] is table                                  # same storage: same table
    with torch.no_grad():
        src.ps[8].data = torch.full((chunk(),), 3.0, device=dev)    # a source parameter moves ...
        src.stat2 = torch.full_like(src.stat2, -2.0)                # ... a source buffer is replaced ...
        ours.module.ps[3].data = ours.module.ps[3].data.clone()     # ... and an averaged parameter moves
    one_update(src, ours, None, 2, 0.5, False, 'after the storage moved')      # (checks against the NEW tensors)
    assert ours._table[1] is not table and torch.equal(ours.module.stat2, src.stat2)
    ours.use_buffers = True
    src.perturb()
    table = ours._table[1]
    one_update(src, ours, None, 3, 0.5, True, 'use_buffers flipped')
    assert ours._table[1] is not table and int(ours.n_averaged) == 4


def test_refusals(dev):
    from gssd import optim
    from gssd._lib import GssdError

    def case(name):
        src = AvgSet(dev, 64)
        ours = optim.AveragedModel(src, ema_decay=0.5, use_buffers=True)
        with torch.no_grad():
            if name == 'half source':
                src.ps[2].data = src.ps[2].data.half()
            elif name == 'noncontiguous source':
                src.ps[5].data = torch.ones(64, 2, device=dev)[:, 0]
            elif name == 'cpu source':
                src.ps[1].data = src.ps[1].data.cpu()
            elif name == 'shape':
                src.ps[4].data = torch.ones(62, device=dev)
            elif name == 'int32 buffer':
                src.ticks = src.ticks.int()
            elif name == 'double averaged buffer':
                ours.module.stat1 = ours.module.stat1.double()
        return src, ours
    for name in ('half source', 'noncontiguous source', 'cpu source', 'shape', 'int32 buffer', 'double averaged buffer'):
        src, ours = case(name)
        src.perturb()
        tensors = list(ours.parameters()) + list(ours.buffers())
        keep, versions = snapshot(ours), [t._version for t in tensors]
        with pytest.raises(GssdError, match='shape' if name == 'shape' else 'no CPU fallback'):
            ours.update_parameters(src)
        assert all(torch.equal(a, b) for a, b in zip(snapshot(ours), keep)), name        # n_averaged among them
        assert [t._version for t in tensors] == versions, name


def build_net(dev, phase='train', sd=None):
    from models.ssd_multiphase_custom_group import build_ssd
    net = build_ssd(phase, 300, 2, *NETS['gssd'][1])
    if sd is None:
        sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=1111)
    net.load_state_dict(sd, strict=True)
    return net.to(dev)


def test_engine_sees_the_average(dev):
    """The averaged module's eval forward runs on the NEW averages (the engine re-packs on the version counters the update bumps): it
    equals the forward of a fresh net loaded with the averages computed in float64."""
    from gssd import optim
    net = build_net(dev).eval()
    avg = optim.AveragedModel(net, ema_decay=0.5, use_buffers=True)
    avg.update_parameters(net)                         # the first update is a copy; the one below averages
    x = synth.synth_images(1, seed=21).to(dev)

    def eval_out(m):
        m.eval()
        with torch.no_grad():
            loc, conf, _ = m(x)
        return loc.clone(), conf.clone()
    first = eval_out(avg.module)                       # the engine of the copy has packed its weights
    with torch.no_grad():
        for i, p in enumerate(net.parameters()):
            p.mul_(1.0 + 0.02 * (i % 5)).add_(1e-3)
        for b in net.buffers():
            if b.dtype == torch.float32:
                b.mul_(1.1)
    a0 = {k: v.clone() for k, v in avg.module.state_dict().items()}
    avg.update_parameters(net)
    want = {}
    for k, b in net.state_dict().items():
        want[k] = lerp64(a0[k].double(), b.double(), 0.5).float() if b.dtype == torch.float32 else b.clone()
    after = eval_out(avg.module)
    ref = eval_out(build_net(dev, sd=want))
    assert not torch.equal(after[0], first[0]) and not torch.equal(after[1], first[1]), 'the forward ran on stale packed weights'
    print('averaged forward vs fresh net: rel', rel(after[0], ref[0]), rel(after[1], ref[1]))
    assert rel(after[0], ref[0]) <= TOL and rel(after[1], ref[1]) <= TOL
    build_net(dev, 'test', sd=avg.module.state_dict())             # strict
    assert int(avg.n_averaged) == 2


def test_update_bn(dev):
    """Three batches of two: every BatchNorm ends with the mean over the batches of the per-batch statistics, which a separate
    train-mode forward per batch after reset_running_stats() gives at the default momentum as (running - 0.9 init) / 0.1."""
    from gssd import optim
    net = build_net(dev)
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert bns and all(m.momentum == 0.1 for m in bns)
    batches = [synth.synth_images(2, seed=s).to(dev) for s in (31, 32, 33)]
    mean = [torch.zeros_like(m.running_mean, dtype=torch.float64) for m in bns]
    var = [torch.zeros_like(m.running_var, dtype=torch.float64) for m in bns]
    net.train()
    for x in batches:
        for m in bns:
            m.reset_running_stats()
        with torch.no_grad():
            net(x)
        for i, m in enumerate(bns):
            mean[i] += (m.running_mean.double() - 0.9 * 0.0) / 0.1 / len(batches)
            var[i] += (m.running_var.double() - 0.9 * 1.0) / 0.1 / len(batches)

    def n_plans():
        return sum(len(v) for v in net._engine._plans.values())
    net.eval()
    plans = n_plans()
    optim.update_bn([(x, None) for x in batches], net)
    assert not net.training and all(m.momentum == 0.1 for m in bns)
    assert n_plans() == plans + 1                                   # the train-mode plan at momentum 1.0
    worst = 0.0
    for i, m in enumerate(bns):
        rm, rv = rel(m.running_mean, mean[i]), rel(m.running_var, var[i])
        worst = max(worst, rm, rv)
        assert rm <= TOL and rv <= TOL, f'BatchNorm {i} ({m.num_features} channels): rel {rm:.3g} (mean), {rv:.3g} (var)'
        assert int(m.num_batches_tracked) == 3
    print(f'update_bn over {len(bns)} BatchNorms: worst rel {worst:.3g}')
    net.train()
    optim.update_bn(iter(batches), net, device=dev)
    assert net.training and all(m.momentum == 0.1 for m in bns) and n_plans() == plans + 1      # no further plan
    for i, m in enumerate(bns):
        assert rel(m.running_mean, mean[i]) <= TOL and rel(m.running_var, var[i]) <= TOL and int(m.num_batches_tracked) == 3
