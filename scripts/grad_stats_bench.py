"""Time of the per-iteration gradient-norm check (train_lesion_multiphase_v2.py:250) on the GSSD++ model's parameter tensors with random
gradients, no forward.  Forms, all on the same tensors in the same process:

    (a) per-param    one torch.linalg.vector_norm and one .item() per parameter, squares added up on the host (what the helper does)
    (b) foreach      torch._foreach_norm + one stacked norm + one read
    (c) check_grad   utils.check_grad_norm.check_grad_norm(net): grad_stats(params=False) + one read of the total
    (d) grad_stats   gssd.optim.grad_stats(net, params=True), nothing read
    (e) monitor      gssd.optim.GradMonitor(net).record(), nothing read

Per form and round: STEPS calls between two device events (GPU time per call: what the stream is busy for, gaps included) and the host
clock around the same loop before any synchronise (host time per call; (a), (b) and (c) wait for their reads inside the loop, so their
host time includes the device's).  Rounds alternate the forms; the table gives the median and the range over the rounds.

    python scripts/grad_stats_bench.py [--steps 50] [--rounds 7] [--out profiles/grad_stats.txt]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('grad_stats_bench: needs the MI355X (no device found)')
    from gssd import optim
    from models.ssd_multiphase_custom_group import build_ssd
    from utils.check_grad_norm import check_grad_norm
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = build_ssd('train', 300, 2, *GSSDPP).to(dev)
    params = list(net.parameters())
    # gradients as the backward plan delivers them: slices of one flat tensor
    flat = torch.randn(sum(-(-p.numel() // 4) * 4 for p in params), device=dev) * 1e-2
    o = 0
    for p in params:
        p.grad = flat[o:o + p.numel()].view(p.shape)
        o += -(-p.numel() // 4) * 4
    n_elems = sum(p.numel() for p in params)
    monitor = optim.GradMonitor(net, history=100)

    def per_param():
        total = 0.0
        for p in net.parameters():
            total += torch.linalg.vector_norm(p.grad, 2).item() ** 2
        return total ** 0.5

    def foreach():
        return torch.linalg.vector_norm(torch.stack(torch._foreach_norm([p.grad for p in net.parameters()], 2.0)), 2).item()

    forms = {
        '(a) per-param': per_param,
        '(b) foreach': foreach,
        '(c) check_grad': lambda: check_grad_norm(net),
        '(d) grad_stats': lambda: optim.grad_stats(net, params=True),
        '(e) monitor': monitor.record,
    }
    values = {}
    for k, f in forms.items():
        for _ in range(a.warmup):
            values[k] = f()
    torch.cuda.synchronize()
    ref = values['(a) per-param']
    for k in ('(b) foreach', '(c) check_grad'):
        assert abs(values[k] - ref) <= 1e-5 * ref, (k, values[k], ref)
    assert abs(float(values['(d) grad_stats'].total_norm) - ref) <= 1e-5 * ref
    gpu = {k: [] for k in forms}
    host = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, f in forms.items():
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

    lines = [f'gradient-norm check, GSSD++: {len(params)} parameter tensors, {n_elems} elements ({4 * n_elems / 1e6:.1f} MB fp32 of gradients), '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds x {a.steps} calls per form, forms alternating; median [min .. max] over the rounds, us per call',
             f'{"form":<16}{"event span":>30}{"host time":>32}']
    med = {}
    for k in forms:
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        med[k] = (g, h)
        lines.append(f'{k:<16}{g:>10.1f} [{min(gpu[k]):>8.1f} .. {max(gpu[k]):>8.1f}]{h:>12.1f} [{min(host[k]):>8.1f} .. {max(host[k]):>8.1f}]')
    c, base = med['(c) check_grad'], med['(a) per-param']
    lines.append(f'(c) against (a): host {c[1]:.1f} vs {base[1]:.1f} us ({base[1] / c[1]:.1f}x), event span {c[0]:.1f} vs {base[0]:.1f} us '
                 f'({base[0] / c[0]:.1f}x); (c) is {"NOT slower" if c[1] <= base[1] else "SLOWER"} than (a) on the host clock')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
