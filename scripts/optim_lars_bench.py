"""Time of the LARS and LAMB steps on the GSSD++ parameter set (bench.py's headline config), no forward: synthetic gradients as 16-byte
aligned slices of one flat tensor (the backward plan's layout), three param groups -- the driver's two (dcn_list.* at lr * 0.1) for the
weights and one WITHOUT layer adaptation and weight decay for all 1-D parameters (biases, BatchNorm weights, sigma), the usual recipe.
Forms, each on its own copy of the parameters and gradients:

    torch lars / clip+lars   the rule restated with torch._foreach_norm / _foreach_* and no host read (the ratios stay on the device as
    torch lamb / clip+lamb   0-dim tensors), with and without torch.nn.utils.clip_grad_norm_ in front
    gssd  lars / clip+lars   gssd.optim.LARS(...).step()                        (2 launches, clip or no clip)
    gssd  lamb / clip+lamb   gssd.optim.LAMB(...).step()                        (2 launches, 3 with the clip)
    gssd  clip+sgd, clip+adam   gssd.optim.SGD / Adam with max_grad_norm        (the kernels the two are built beside: for context)

Per form and round: STEPS calls between two device events (GPU time per call: what the stream is busy for, gaps included) and the host
clock around the same loop before any synchronise (host time per call: the enqueue).  Rounds alternate the forms; the table gives the
median and the range over the rounds.  `launches` is what the optimizer counted in its own step (``opt.launches``), kernel launches per
call.  The traffic model: LARS makes 7 passes over the parameter bytes (read p, g | read g, p, buf; write p, buf) against 6 of SGD with
the clip; LAMB 10 (read g, p, m, v; write m, v | read p, m, v; write p) against 8 of Adam with the clip.  The last lines put the
measured ratios beside it.

The requirement, checked in the same run (exit status 1 when it does not hold): the median GPU time AND the median host time of each
of the four gssd LARS / LAMB forms are below those of its torch restatement.

    python scripts/optim_lars_bench.py [--steps 50] [--rounds 7] [--out profiles/optim_lars_step.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'))
import torch                                                    # noqa: E402

GSSDPP = (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)   # bench.py CONFIGS['gssdpp']


def ratios_on_device(num, den_extra, ok_norms, scale):
    """scale * num / (den_extra) where every norm in ok_norms is > 0, else 1 -- on stacked 0-dim norms, unbound again: no host read."""
    num_t, den_t = torch.stack(num), torch.stack(den_extra)
    ok = torch.ones_like(num_t, dtype=torch.bool)
    for n in ok_norms:
        ok &= torch.stack(n) > 0
    return torch.where(ok, scale * num_t / den_t, torch.ones_like(num_t))


class TorchLars:
    """LARS in foreach operations: per group norms of w and g', the ratio per tensor, then SGD's chain on the scaled gradient."""

    def __init__(self, groups, max_norm=None, **kw):
        self.groups = [dict(kw, **g) for g in groups]
        self.max_norm = max_norm
        self.all = [p for g in self.groups for p in g['params']]
        self.bufs = [[torch.zeros_like(p) for p in g['params']] for g in self.groups]

    @torch.no_grad()
    def step(self):
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.all, self.max_norm)
        for g, bufs in zip(self.groups, self.bufs):
            ps = g['params']
            grads = [p.grad for p in ps]
            d = torch._foreach_add(grads, ps, alpha=g['weight_decay']) if g['weight_decay'] != 0 else [x.clone() for x in grads]
            if g['layer_adaptation']:
                wn, gn = torch._foreach_norm(ps), torch._foreach_norm(grads)
                den = torch._foreach_mul(wn, g['weight_decay'])
                torch._foreach_add_(den, gn)
                torch._foreach_add_(den, g['eps'])
                torch._foreach_mul_(d, list(ratios_on_device(wn, den, (wn, gn), g['trust_coefficient']).unbind(0)))
            torch._foreach_mul_(bufs, g['momentum'])
            torch._foreach_add_(bufs, d, alpha=1 - g['dampening'])
            torch._foreach_add_(ps, bufs, alpha=-g['lr'])


class TorchLamb:
    """LAMB in foreach operations: Adam's moments, the update direction, per group norms of w and u, the ratio per tensor."""

    def __init__(self, groups, max_norm=None, **kw):
        self.groups = [dict(kw, **g) for g in groups]
        self.max_norm = max_norm
        self.all = [p for g in self.groups for p in g['params']]
        self.m = [[torch.zeros_like(p) for p in g['params']] for g in self.groups]
        self.v = [[torch.zeros_like(p) for p in g['params']] for g in self.groups]
        self.t = 0

    @torch.no_grad()
    def step(self):
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_(self.all, self.max_norm)
        self.t += 1
        for g, ms, vs in zip(self.groups, self.m, self.v):
            ps = g['params']
            grads = [p.grad for p in ps]
            b1, b2 = g['betas']
            bc1, bc2 = 1 - b1 ** self.t, 1 - b2 ** self.t
            torch._foreach_lerp_(ms, grads, 1 - b1)
            torch._foreach_mul_(vs, b2)
            torch._foreach_addcmul_(vs, grads, grads, value=1 - b2)
            den = torch._foreach_sqrt(vs)
            torch._foreach_div_(den, math.sqrt(bc2))
            torch._foreach_add_(den, g['eps'])
            u = torch._foreach_div(ms, bc1)
            torch._foreach_div_(u, den)
            if g['weight_decay'] != 0:
                torch._foreach_add_(u, ps, alpha=g['weight_decay'])
            if g['layer_adaptation']:
                wn, un = torch._foreach_norm(ps), torch._foreach_norm(u)
                torch._foreach_mul_(u, list(ratios_on_device(wn, un, (wn, un), g['lr']).unbind(0)))
                # (where the ratio falls back to 1 this form applies 1 instead of lr: it cannot happen with these tensors)
            else:
                torch._foreach_mul_(u, g['lr'])
            torch._foreach_sub_(ps, u)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--max-norm', type=float, default=5.0)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('optim_lars_bench: needs the MI355X (no device found)')
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
        flat_p = [p for p in ps if p.dim() <= 1]
        dcn = [p for (k, _), p in zip(named, ps) if k.startswith('dcn_list') and p.dim() > 1]
        rest = [p for (k, _), p in zip(named, ps) if not k.startswith('dcn_list') and p.dim() > 1]
        return [dict(params=rest), dict(params=dcn, lr_scale=0.1), dict(params=flat_p, layer_adaptation=False, weight_decay=0.0)]

    def groups(lr, extra=True):
        out = []
        for g in param_set():
            g = dict(g)
            scale = g.pop('lr_scale', 1.0)
            if scale != 1.0:
                g['lr'] = lr * scale
            if not extra:
                g.pop('layer_adaptation', None)
            out.append(g)
        return out

    lars_kw = dict(lr=0.1, momentum=0.9, dampening=0.0, weight_decay=5e-4, trust_coefficient=1e-3, eps=1e-8, layer_adaptation=True)
    lamb_kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, layer_adaptation=True)
    sgd_kw = dict(lr=1e-3, momentum=0.9, weight_decay=5e-4)
    adam_kw = dict(lr=1e-4, weight_decay=5e-4)
    forms, opts, pairs = {}, {}, []
    for clip, tag in ((None, ''), (a.max_norm, 'clip+')):
        forms[f'torch {tag}lars'] = TorchLars(groups(lars_kw['lr']), clip, **lars_kw).step
        forms[f'torch {tag}lamb'] = TorchLamb(groups(lamb_kw['lr']), clip, **lamb_kw).step
        for name, cls, kw in (('lars', optim.LARS, lars_kw), ('lamb', optim.LAMB, lamb_kw)):
            opt = cls(groups(kw['lr']), max_grad_norm=clip, **kw)
            opts[f'gssd  {tag}{name}'] = opt
            forms[f'gssd  {tag}{name}'] = opt.step
            pairs.append((f'gssd  {tag}{name}', f'torch {tag}{name}'))
    forms['gssd  clip+sgd'] = optim.SGD(groups(sgd_kw['lr'], extra=False), max_grad_norm=a.max_norm, **sgd_kw).step
    forms['gssd  clip+adam'] = optim.Adam(groups(adam_kw['lr'], extra=False), max_grad_norm=a.max_norm, **adam_kw).step

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

    n_flat = sum(1 for _, s in named if len(s) <= 1)
    lines = [f'LARS / LAMB step, GSSD++ parameters: {len(named)} tensors ({n_flat} of them 1-D, in the group without adaptation), '
             f'{n_elems} elements ({4 * n_elems / 1e6:.1f} MB fp32), {torch.cuda.get_device_name(0)}',
             f'{a.rounds} rounds x {a.steps} calls per form, forms alternating; median [min .. max] over the rounds, us per call',
             f'{"form":<18}{"GPU time (events)":>26}{"host time (enqueue)":>28}{"launches":>10}']
    med = {}
    for k in forms:
        g, h = statistics.median(gpu[k]), statistics.median(host[k])
        med[k] = (g, h)
        n = str(opts[k].launches) if k in opts else ('2' if k.startswith('gssd') else '-')
        lines.append(f'{k:<18}{g:>9.1f} [{min(gpu[k]):>6.1f} .. {max(gpu[k]):>6.1f}]{h:>11.1f} [{min(host[k]):>6.1f} .. {max(host[k]):>6.1f}]{n:>10}')
    ok = True
    for ours, theirs in pairs:
        (og, oh), (tg, th) = med[ours], med[theirs]
        good = og < tg and oh < th
        ok = ok and good
        lines.append(f'{" ".join(ours.split())} below {" ".join(theirs.split())} (GPU {og:.1f} < {tg:.1f} us, host {oh:.1f} < {th:.1f} us): {"yes" if good else "NO"}')
    for ours, base, model in (('gssd  clip+lars', 'gssd  clip+sgd', '7 / 6 = 1.17'), ('gssd  clip+lamb', 'gssd  clip+adam', '10 / 8 = 1.25')):
        lines.append(f'{" ".join(ours.split())} / {" ".join(base.split())}: GPU time x{med[ours][0] / med[base][0]:.2f}, the traffic model says {model}')
    text = '\n'.join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')
    sys.exit(0 if ok else 1)


if __name__ == '__main__':
    main()
