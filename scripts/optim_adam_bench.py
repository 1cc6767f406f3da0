"""Time of the Adam step on the GSSD++ parameter set (bench.py's headline config), no forward: synthetic gradients as 16-byte aligned
slices of one flat tensor (the backward plan's layout), the driver's two param groups (dcn_list.* at lr * 0.1), weight decay 5e-4.
Forms, each on its own copy of the parameters and gradients:

    torch clip+adam   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step()    (torch's default form)
    torch adam        torch.optim.Adam.step()
    torch fused c+a   torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(fused=True).step()   (reported only)
    torch fused adam  torch.optim.Adam(fused=True).step()                          (reported only)
    gssd  clip+adam   gssd.optim.Adam(max_grad_norm=...).step()                    (2 launches)
    gssd  adam        gssd.optim.Adam.step()                                       (1 launch)

Per form and round: STEPS calls between two device events (GPU time per call: what the stream is busy for, gaps included) and the host
clock around the same loop before any synchronise (host time per call: the enqueue).  Rounds alternate the forms; the table gives the
median and the range over the rounds.  `HBM` = 7 x parameter bytes (read g, p, m, v; write p, m, v) over the GPU time, as a share of the
8 TB/s peak -- for the gssd forms the algorithm's own traffic, for the torch forms the same useful bytes (they move more).

The requirement, checked in the same run (exit status 1 when it does not hold): the median GPU time AND the median host time of
`gssd  clip+adam` are below those of `torch clip+adam`.

    python scripts/optim_adam_bench.py [--steps 50] [--rounds 7] [--out profiles/optim_adam_step.txt]
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
    ap.add_argument('--max-norm', type=float, default=5.0)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_adam_bench: needs the MI355X (no device found)')
    from gssd import optim
    from models.ssd_multiphase_custom_group import build_ssd
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = build_ssd('train', 300, 2, *GSSDPP)
    named = [(k, tuple(p.shape)) for k, p in net.named_parameters()]
    del net
    n_elems = sum(int(torch.Size(s).numel()) for _, s in named)

    def param_set():
        ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.05) for _, s in named]
        offs, o = [], 0
        for p in ps:
            offs.append(o)
            o += -(-p.numel() // 4) * 4
        flat = torch.randn(o, device=dev) * 1e-3
        for p, o in zip(ps, offs):
            p.grad = flat[o:o + p.numel()].view(p.shape)
        dcn = [p for (k, _), p in zip(named, ps) if k.startswith('dcn_list')]
        rest = [p for (k, _), p in zip(named, ps) if not k.startswith('dcn_list')]
        return ps, [dict(params=rest), dict(params=dcn, lr=1e-5)]

    kw = dict(lr=1e-4, weight_decay=5e-4)
    forms = {}
    ps, groups = param_set()
    opt = torch.optim.Adam(groups, **kw)
    forms['torch clip+adam'] = lambda ps=ps, opt=opt: (torch.nn.utils.clip_grad_norm_(ps, a.max_norm), opt.step())
    ps, groups = param_set()
    forms['torch adam'] = torch.optim.Adam(groups, **kw).step
    ps, groups = param_set()
    opt = torch.optim.Adam(groups, fused=True, **kw)
    forms['torch fused c+a'] = lambda ps=ps, opt=opt: (torch.nn.utils.clip_grad_norm_(ps, a.max_norm), opt.step())
    ps, groups = param_set()
    forms['torch fused adam'] = torch.optim.Adam(groups, fused=True, **kw).step
    ps, groups = param_set()
    forms['gssd  clip+adam'] = optim.Adam(groups, max_grad_norm=a.max_norm, **kw).step
    ps, groups = param_set()
    forms['gssd  adam'] = optim.Adam(groups, **kw).step

    for f in forms.values():
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
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

    lines = [f'Adam step, GSSD++ parameters: {len(named)} tensors, {n_elems} elements ({4 * n_elems / 1e6:.1f} MB fp32), '
             f'{torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds x {a.steps} calls per form, forms alternating; median [min .. max] over the rounds, us per call',
             f'{"form":<18}{"GPU time (events)":>26}{"host time (enqueue)":>28}{"HBM: 7 x param bytes / GPU time":>36}']
    med = {}
    for k in forms:
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        med[k] = (g, h)
        gbs = 7 * 4 * n_elems / (g * 1e-6) / 1e9
        lines.append(f'{k:<18}{g:>9.1f} [{min(gpu[k]):>6.1f} .. {max(gpu[k]):>6.1f}]{h:>11.1f} [{min(host[k]):>6.1f} .. {max(host[k]):>6.1f}]'
                     f'{gbs:>14.0f} GB/s = {100 * gbs / PEAK_HBM_GBS:>4.1f} % of peak')
    ours, theirs = med['gssd  clip+adam'], med['torch clip+adam']
    ok = ours[0] < theirs[0] and ours[1] < theirs[1]
    lines.append(f'gssd clip+adam below torch clip+adam (GPU {ours[0]:.1f} < {theirs[0]:.1f} us, host {ours[1]:.1f} < {theirs[1]:.1f} us): '
                 f'{"yes" if ok else "NO"}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
