"""The steps whose results tests/golden/optim_steps.npz records, shared by tests/golden/make_golden_optim.py (which runs them at the
commit the fixture names) and tests/test_gpu_optim_golden.py (which runs them again and compares bit for bit).  Only this library runs
on the device: the kernels are bitwise reproducible, so a refactor of the optimizer core must leave every byte where it was.

Parameter set (CH = the kernels' chunk size), values randn * 10^U(-3, 1), gradients randn * 10^U(-4, 1), seed fixed:
    a[0:9]   numels [1, 3, 5, 64, CH-1, CH, CH+1, 2 CH+5, 0] laid end to end in ONE flat buffer (parameters and gradients alike): the
             one-element head leaves most of them off the 16-byte grid, so the vector path and the element-wise path both run
    b[0:9]   the same numels, every tensor allocated on its own (all aligned)
    nograd   7 elements, grad None;   big: 1025 CH + 1 elements (the record fold beyond 256 chunks, the partial sums beyond 1024 workgroups)
in NINE param groups -- group i holds a[i] and b[i], group 0 nograd, group 8 big -- with lr scaled by (1, 0.5, 0.1)[i % 3]: a step
takes a second launch and LAMB runs its <true, true> instance.  Group 3 has layer_adaptation=False (LARS, LAMB).  A case takes three
steps with fresh gradients in the same storage.

What a case leaves is a list of (name, array, in full?): norms, trust ratios and tables always in full, a tensor of up to full_max(case)
elements in full, a larger one as the SHA-256 of its bytes.  full_max is 8192 in FULL_CASES -- one case of each update rule, momentum
and moments, each with its trust ratio and the clip -- so that a mismatch there prints values of the chunk-sized tensors too, and 64 in
the others: every tensor of up to 8192 elements in full would be 6 MB over the 24 step cases, against 1 MiB for a committed file.  The
assertion is the same either way: equality of every byte.
"""
import functools
import hashlib

import numpy as np
import torch

FULL_CASES = ('LARS|clip', 'LAMB|clip')
STEPS = 3
N_GROUPS = 9


def numels(ch):
    return [1, 3, 5, 64, ch - 1, ch, ch + 1, 2 * ch + 5, 0]


@functools.lru_cache(maxsize=None)
def host_data(ch):
    """Values and per-step gradients on the host: generated once, never modified (users copy)."""
    rng = np.random.default_rng(20261)
    total, big = sum(numels(ch)), 1025 * ch + 1

    def draw(n, lo):
        return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(lo, 1, n)).astype(np.float32))
    return dict(a=draw(total, -3), b=draw(total, -3), nograd=draw(7, -3), big=draw(big, -3),
                ga=[draw(total, -4) for _ in range(STEPS)], gb=[draw(total, -4) for _ in range(STEPS)],
                gbig=[draw(big, -4) for _ in range(STEPS)])


class ParamSet:
    def __init__(self, dev, ch):
        self.h = h = host_data(ch)
        ns = numels(ch)
        self.spans = [(sum(ns[:i]), n) for i, n in enumerate(ns)]
        self.flat_p, self.flat_g = h['a'].clone().to(dev), torch.empty_like(h['a'], device=dev)
        self.a = [torch.nn.Parameter(self.flat_p[o:o + n]) for o, n in self.spans]
        for p, (o, n) in zip(self.a, self.spans):
            p.grad = self.flat_g[o:o + n]
        self.b = [torch.nn.Parameter(h['b'][o:o + n].clone().to(dev)) for o, n in self.spans]
        for p in self.b:
            p.grad = torch.empty_like(p)
        self.nograd = torch.nn.Parameter(h['nograd'].clone().to(dev))
        self.big = torch.nn.Parameter(h['big'].clone().to(dev))
        self.big.grad = torch.empty_like(self.big)
        self.all = self.a + self.b + [self.nograd, self.big]
        self.set_grads(0)

    def set_grads(self, k):
        """The gradients of step k, into the storage the gradients already have."""
        self.flat_g.copy_(self.h['ga'][k])
        gb = self.h['gb'][k].to(self.flat_g.device)
        for p, (o, n) in zip(self.b, self.spans):
            p.grad.copy_(gb[o:o + n])
        self.big.grad.copy_(self.h['gbig'][k])

    def groups(self, lr, adapt=False):
        out = []
        for i in range(N_GROUPS):
            g = dict(params=[self.a[i], self.b[i]], lr=lr * (1.0, 0.5, 0.1)[i % 3])
            if i == 0:
                g['params'].append(self.nograd)
            if i == N_GROUPS - 1:
                g['params'].append(self.big)
            if adapt and i == 3:
                g['layer_adaptation'] = False
            out.append(g)
        return out


#                        momentum dampening nesterov weight_decay max_grad_norm
MOMENTUM_ROWS = dict(plain=(0.9, 0.0, False, 5e-4, None), clip=(0.9, 0.0, False, 5e-4, 0.5), noclip=(0.9, 0.0, False, 5e-4, 1e6),
                     nesterov=(0.9, 0.0, True, 5e-4, None), dampening=(0.5, 0.1, False, 5e-4, None), nomomentum=(0.0, 0.0, False, 0.0, 0.5))
#                    amsgrad max_grad_norm
ADAM_ROWS = dict(plain=(False, None), clip=(False, 0.5), noclip=(False, 1e6), amsgrad=(True, None))
#                    bias_correction max_grad_norm
LAMB_ROWS = dict(plain=(True, None), clip=(True, 0.5), noclip=(True, 1e6), nobias=(False, None))

STEP_CASES = ([f'SGD|{r}' for r in MOMENTUM_ROWS] + [f'LARS|{r}' for r in MOMENTUM_ROWS] + [f'Adam|{r}' for r in ADAM_ROWS] +
              [f'AdamW|{r}' for r in ADAM_ROWS] + [f'LAMB|{r}' for r in LAMB_ROWS])
OTHER_CASES = ['clip_grad_norm|0.5', 'clip_grad_norm|1e6', 'averaged_model', 'grad_stats']
CASES = STEP_CASES + OTHER_CASES
STATE_KEYS = ('momentum_buffer', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


def _np(t):
    return t.detach().cpu().numpy()


def step_case(name, dev):
    from gssd import optim
    kind, row = name.split('|')
    ps = ParamSet(dev, optim.CHUNK)
    if kind in ('SGD', 'LARS'):
        mom, damp, nest, wd, clip = MOMENTUM_ROWS[row]
        opt = getattr(optim, kind)(ps.groups(1e-2, kind == 'LARS'), lr=1e-2, momentum=mom, dampening=damp, nesterov=nest, weight_decay=wd,
                                   max_grad_norm=clip)
    elif kind in ('Adam', 'AdamW'):
        ams, clip = ADAM_ROWS[row]
        opt = getattr(optim, kind)(ps.groups(1e-3), lr=1e-3, weight_decay=5e-4 if kind == 'Adam' else 1e-2, amsgrad=ams, max_grad_norm=clip)
    else:
        bias, clip = LAMB_ROWS[row]
        opt = optim.LAMB(ps.groups(1e-3, True), lr=1e-3, weight_decay=1e-2, bias_correction=bias, max_grad_norm=clip)
    out = []
    for k in range(STEPS):
        ps.set_grads(k)
        opt.step()
        if clip is not None:
            out.append((f'step {k} grad_norm', _np(opt.grad_norm), True))
        if kind in ('LARS', 'LAMB'):
            out.append((f'step {k} trust_ratio', _np(opt.trust_ratio), True))
            assert opt.launches == int(kind == 'LAMB' and clip is not None) + 1 + 2
    for i, p in enumerate(ps.all):
        out.append((f'p[{i}]', _np(p), False))
        for key in STATE_KEYS:
            if key in opt.state.get(p, {}):
                out.append((f'{key}[{i}]', _np(opt.state[p][key]), False))
    return out


def clip_case(name, dev):
    from gssd import optim
    ps = ParamSet(dev, optim.CHUNK)
    norm = optim.clip_grad_norm_(ps.all, float(name.split('|')[1]))
    return [('total_norm', _np(norm), True)] + [(f'grad[{i}]', _np(p.grad), False) for i, p in enumerate(ps.all) if p.grad is not None]


def _model(dev):
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 8, 3), torch.nn.BatchNorm2d(8))
    return m.to(dev)


def _fill(model, version):
    """Version ``version`` of the weights and statistics, in place: the same numbers in every run."""
    rng = np.random.default_rng(977 + version)
    with torch.no_grad():
        for k, t in model.state_dict().items():
            if t.dtype == torch.int64:
                t.fill_(5 * version + 1)
            else:
                v = rng.standard_normal(tuple(t.shape)).astype(np.float32)
                t.copy_(torch.from_numpy(np.abs(v) + 0.5 if k.endswith('running_var') else v))


def averaged_case(name, dev):
    from gssd import optim
    out = []
    for use_buffers in (False, True):
        for decay in (None, 0.9):
            model = _model(dev)
            _fill(model, 0)
            avg = optim.AveragedModel(model, use_buffers=use_buffers, ema_decay=decay)
            for version in range(3):                         # a first update (a copy) and two that average
                _fill(model, version)
                avg.update_parameters(model)
            tag = f'use_buffers={use_buffers} {"SWA" if decay is None else "EMA"}'
            out += [(f'{tag} {k}', _np(t), True) for k, t in avg.state_dict().items()]
    return out


def stats_case(name, dev):
    from gssd import optim
    ps = ParamSet(dev, optim.CHUNK)
    ps.a[5].grad[17] = float('inf')
    ps.big.grad[700 * optim.CHUNK + 3] = float('nan')
    st = optim.grad_stats([(f't{i}', p) for i, p in enumerate(ps.all)])
    assert st.without_grad == [f't{len(ps.all) - 2}']
    return [('table', _np(st.table), True)]


def run_case(name, dev):
    """[(entry name, array, stored in full?)] of one case, in a fixed order."""
    if name in STEP_CASES:
        return step_case(name, dev)
    return {'clip_grad_norm': clip_case, 'averaged_model': averaged_case, 'grad_stats': stats_case}[name.split('|')[0]](name, dev)


def full_max(name):
    return 8192 if name in FULL_CASES else 64


def pack(name, entries):
    """(full: the bytes of the entries stored in full, end to end; sha: uint8 [k, 32], the digests of the others), both in entry order."""
    full, sha, limit = [], [], full_max(name)
    for _, a, always in entries:
        a = np.ascontiguousarray(a)
        if always or a.size <= limit:
            full.append(a.reshape(-1).view(np.uint8))
        else:
            sha.append(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8))
    return (np.concatenate(full) if full else np.zeros(0, np.uint8)), (np.stack(sha) if sha else np.zeros((0, 32), np.uint8))


def compare(name, entries, full, sha):
    """Every entry of a replayed case against the fixture's ``full`` / ``sha`` of that case: the same bytes, entry by entry."""
    o, k, limit = 0, 0, full_max(name)
    for entry, a, always in entries:
        a = np.ascontiguousarray(a)
        if always or a.size <= limit:
            got = a.reshape(-1).view(np.uint8)
            want = full[o:o + got.size]
            o += got.size
            assert got.size == want.size and np.array_equal(got, want), \
                f'{name}: {entry} differs: now {a.reshape(-1)[:8]}, recorded {want.view(a.dtype)[:8] if want.size == got.size else "fewer bytes"}'
        else:
            assert k < len(sha) and np.array_equal(np.frombuffer(hashlib.sha256(a.tobytes()).digest(), np.uint8), sha[k]), \
                f'{name}: {entry} ({a.size} elements) differs from the recorded SHA-256'
            k += 1
    assert o == full.size and k == len(sha), f'{name}: the fixture holds more entries than the case left'
