"""Time of AveragedModel.update_parameters on the GSSD++ model (bench.py's headline config), no forward.  Forms, each with its own
averaged copy of the same source model, all on the same device in the same process:

    torch ema   torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)).update_parameters()
    torch swa   torch.optim.swa_utils.AveragedModel().update_parameters()             (torch's default, the equal average)
    gssd  ema   gssd.optim.AveragedModel(ema_decay=d).update_parameters()             (1 launch)
    gssd  swa   gssd.optim.AveragedModel().update_parameters()                        (1 launch)

use_buffers is False (torch's default): parameters are averaged, buffers copied.  Per form and round: STEPS calls between two device
events (GPU time per call: what the stream is busy for, gaps included) and the host clock around the same loop before any synchronise
(host time per call; torch's forms read n_averaged back on every call, so their host time includes that wait).  Rounds alternate the
forms; the table gives the median and the range over the rounds.  `bytes` = what the update has to move: 12 per averaged element
(read a, b; write a), 8 per copied 4-byte element, 16 per copied int64; GB/s = bytes / GPU time, as a share of the 8 TB/s peak -- for
the gssd forms the kernel's own traffic, for the torch forms the same useful bytes (they move more).

    python scripts/optim_avg_bench.py [--steps 50] [--rounds 7] [--decay 0.999] [--out profiles/optim_avg.txt]
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
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_avg_bench: needs the MI355X (no device found)')
    from torch.optim.swa_utils import AveragedModel as TorchAveragedModel, get_ema_multi_avg_fn
    from gssd import optim
    from models.ssd_multiphase_custom_group import build_ssd
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = build_ssd('train', 300, 2, *GSSDPP).to(dev)
    params, buffers = list(net.parameters()), list(net.buffers())
    n_avg = sum(p.numel() for p in params)
    n_bytes = 12 * n_avg + sum(2 * b.numel() * b.element_size() for b in buffers)

    forms = {
        'torch ema': TorchAveragedModel(net, device=dev, multi_avg_fn=get_ema_multi_avg_fn(a.decay)),
        'torch swa': TorchAveragedModel(net, device=dev),
        'gssd  ema': optim.AveragedModel(net, ema_decay=a.decay),
        'gssd  swa': optim.AveragedModel(net),
    }
    for m in forms.values():
        for _ in range(a.warmup):
            m.update_parameters(net)
    torch.cuda.synchronize()
    gpu = {k: [] for k in forms}
    host = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, m in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            for _ in range(a.steps):
                m.update_parameters(net)
            e1.record()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            gpu[k].append(1e3 * e0.elapsed_time(e1) / a.steps)
            host[k].append(1e6 * (t1 - t0) / a.steps)
    counts = {k: int(m.n_averaged) for k, m in forms.items()}
    assert len(set(counts.values())) == 1, counts

    lines = [f'AveragedModel.update_parameters, GSSD++: {len(params)} parameters, {n_avg} elements ({4 * n_avg / 1e6:.1f} MB fp32) averaged, '
             f'{len(buffers)} buffers copied, {n_bytes / 1e6:.1f} MB to move per call, {torch.cuda.get_device_name(0)}',
             f'decay {a.decay}; {a.rounds} rounds x {a.steps} calls per form, forms alternating; median [min .. max] over the rounds, us per call',
             f'{"form":<12}{"GPU time (events)":>26}{"host time (enqueue)":>28}{"bytes / GPU time":>28}']
    med = {}
    for k in forms:
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        med[k] = (g, h)
        gbs = n_bytes / (g * 1e-6) / 1e9
        lines.append(f'{k:<12}{g:>9.1f} [{min(gpu[k]):>6.1f} .. {max(gpu[k]):>6.1f}]{h:>11.1f} [{min(host[k]):>6.1f} .. {max(host[k]):>6.1f}]'
                     f'{gbs:>10.0f} GB/s = {100 * gbs / PEAK_HBM_GBS:>4.1f} % of peak')
    for rule in ('ema', 'swa'):
        ours, theirs = med[f'gssd  {rule}'], med[f'torch {rule}']
        lines.append(f'gssd {rule} against torch {rule}: GPU {ours[0]:.1f} vs {theirs[0]:.1f} us ({theirs[0] / ours[0]:.1f}x), '
                     f'host {ours[1]:.1f} vs {theirs[1]:.1f} us ({theirs[1] / ours[1]:.1f}x)')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
