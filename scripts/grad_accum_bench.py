"""Time of one micro-batch's gradient accumulation on a synthetic gradient set with the shapes of GSSD++'s parameters (bench.py's
headline config; the model is built for its shapes only, nothing runs through it).  The gradients are 16-byte aligned slices of one
flat tensor, as the backward plan hands them out.  Forms, all on the same device in the same process:

    hand-out      p.grad = slice for every parameter, nothing else (what backward() does before any form below; host only)
    gssd add      hand-out + gssd.optim.GradAccumulator.add(weight=<fp64 device scalar>)                     (1 launch)
    accum kernel  the launch of that add() alone, over its cached table (where add()'s host time exceeds the kernel, the events
                  around `gssd add` show the host; this form shows the kernel)
    clone + add_  hand-out of the previous micro-batch, then p.grad = p.grad.clone(); p.grad.add_(g) per parameter: what
                  GssdTrainFn.backward does on the second micro-batch without the accumulator
    add_          p.grad.add_(g) per parameter into gradients that are already out of the way (third micro-batch onwards)
    foreach add_  torch._foreach_add_(grads, gs): the best case of the same
    avg kernel    AveragedModel.update_parameters' kernel (csrc/optim_avg.hip, EMA) over the same tensors: the same 12 bytes per element

The torch forms add with weight 1 (a weighted mean would cost them a multiplication more); `gssd add` multiplies by the weight it
reads from the device.  Per form and round: STEPS calls between two device events (GPU time per call: what the stream is busy for,
gaps included) and the host clock around the same loop before any synchronise (host time per call).  Rounds alternate the forms, each
round starting one form later; the table gives the median and the range over the rounds, which is the run-to-run spread to hold a difference against.

    python scripts/grad_accum_bench.py [--steps 50] [--rounds 7] [--out profiles/grad_accum.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'))
import torch                                                    # noqa: E402

GSSDPP = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)   # bench.py CONFIGS['gssdpp']
PEAK_HBM_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('grad_accum_bench: needs the MI355X (no device found)')
    from gssd import optim
    from models.ssd_multiphase_custom_group import build_ssd
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in build_ssd('train', 300, 2, *GSSDPP).parameters()]
    params = [torch.nn.Parameter(torch.empty(s, device=dev)) for s in shapes]
    n_el = sum(p.numel() for p in params)
    slices = optim.flat_views(params, dev)                      # this micro-batch's gradients, as the backward plan lays them out
    slices[0]._base.normal_()
    weight = torch.tensor([37.0], device=dev, dtype=torch.float64)

    def hand_out():
        for p, g in zip(params, slices):
            p.grad = g

    acc = optim.GradAccumulator(params)

    def gssd_add():
        hand_out()
        acc.add(weight=weight)

    gssd_add()                                                  # (the FIRST launch of the cycle; every later one adds)
    gssd_add()
    table, written = next(reversed(acc._tables.values()))       # the table of a steady-state add()
    w_ptr = weight.data_ptr()

    def accum_kernel():
        acc._launch(table, written, 0.0, w_ptr, 0)

    def clone_add():
        hand_out()
        for p, g in zip(params, slices):
            p.grad = p.grad.clone()
            p.grad.add_(g)

    foreign = [torch.zeros_like(g) for g in slices]             # gradients that are out of the way already

    def add_only():
        for t, g in zip(foreign, slices):
            t.add_(g)

    def foreach_add():
        torch._foreach_add_(foreign, slices)

    averaged = optim.flat_views(params, dev, zero=True)
    count = torch.ones((), device=dev, dtype=torch.int64)
    avg = optim._AvgTable([(optim.AVG_LERP, d, s, 'tensor') for d, s in zip(averaged, slices)], count)

    def avg_kernel():
        avg.launch(1e-3)

    forms = {'hand-out': hand_out, 'gssd add': gssd_add, 'accum kernel': accum_kernel, 'clone + add_': clone_add, 'add_': add_only, 'foreach add_': foreach_add,
             'avg kernel': avg_kernel}
    for f in forms.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    launches0 = acc.launches
    gpu = {k: [] for k in forms}
    host = {k: [] for k in forms}
    order = list(forms.items())
    for r in range(a.rounds):
        for k, f in order[r % len(order):] + order[:r % len(order)]:       # each round starts one form later: no form always follows the same one
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.steps):
                f()
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            gpu[k].append(1e3 * e0.elapsed_time(e1) / a.steps)
            host[k].append(1e6 * (t1 - t0) / a.steps)
    assert acc.launches - launches0 == 2 * a.rounds * a.steps, 'one launch per add() and per call of the kernel alone'

    n_bytes = 12 * n_el
    lines = [f'gradient accumulation of one micro-batch, GSSD++ shapes: {len(params)} parameters, {n_el} elements ({4 * n_el / 1e6:.1f} MB fp32), '
             f'{n_bytes / 1e6:.1f} MB to move per call (read acc, g; write acc), {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds x {a.steps} calls per form, forms alternating; median [min .. max] over the rounds, us per call',
             f'{"form":<14}{"GPU time (events)":>28}{"host time (enqueue)":>30}{"bytes / GPU time":>28}']
    med = {}
    for k in forms:
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        med[k] = (g, h)
        tail = ''
        if k != 'hand-out':
            gbs = n_bytes / (g * 1e-6) / 1e9
            tail = f'{gbs:>10.0f} GB/s = {100 * gbs / PEAK_HBM_GBS:>4.1f} % of peak'
        lines.append(f'{k:<14}{g:>9.1f} [{min(gpu[k]):>7.1f} .. {max(gpu[k]):>7.1f}]{h:>11.1f} [{min(host[k]):>7.1f} .. {max(host[k]):>7.1f}]{tail}')
    ours, ref = med['gssd add'], med['avg kernel']
    spread = max(gpu['avg kernel']) - min(gpu['avg kernel'])
    for k in ('accum kernel', 'gssd add'):
        lines.append(f'{k} against the avg kernel: GPU {med[k][0]:.1f} vs {ref[0]:.1f} us (difference {med[k][0] - ref[0]:+.1f} us; the avg '
                     f'kernel\'s own range over the rounds is {spread:.1f} us)')
    for k in ('clone + add_', 'add_', 'foreach add_'):
        lines.append(f'gssd add against {k}: GPU {ours[0]:.1f} vs {med[k][0]:.1f} us ({med[k][0] / ours[0]:.1f}x), '
                     f'host {ours[1]:.1f} vs {med[k][1]:.1f} us ({med[k][1] / ours[1]:.1f}x)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
