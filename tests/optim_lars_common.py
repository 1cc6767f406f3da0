"""What tests/test_optim_lars_cpu.py and tests/test_gpu_optim_lars.py share: the float64 reference of one LARS / LAMB step of ONE tensor
with the bounds that go with it (``lars_ref`` / ``lamb_ref``), an independent restatement of the two rules in torch operations that runs
in the tensors' own dtype (``lars_torch`` / ``lamb_torch``; fp32: the check of the yardstick, float64: the check of the reference), a
minimal optimizer over the restatement (``Restated``) and the assertion itself (``snapshot`` / ``check_step``).  No device is needed to
import or to run any of it.

The rules (c: the clip coefficient, g' = c g, ||.||: the 2-norm over the tensor, in float64):
    LARS   r = adapt and ||w|| > 0 and ||g'|| > 0 ? tc ||w|| / (||g'|| + wd ||w|| + eps) : 1
           d = r (g' + wd w);  buf = first ? d : mom buf + (1 - damp) d;  step = nesterov ? d + mom buf : buf (mom 0: d);  w -= lr step
    LAMB   m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd w
           r = adapt and ||w|| > 0 and ||u|| > 0 ? ||w|| / ||u|| : 1;  w -= lr r u

The bounds (teacher-forced: expected values in float64 from the fp32 p, g, buf / m, v before the step; every fp32 operation rounds once,
2^-24 relative, and every budget below is the count of roundings with a factor 2 of margin, as in the SGD and Adam tests):
    rel_r  = 2^-23                                   r is formed in fp64 and rounded once
             + 4e-6 when clipping                    the 1e-6 allowed on the global norm
             + ||tol_u||_2 / ||u64||_2  (LAMB)       the triangle inequality on the fp32 u against the float64 u
             (0 where r is 1 by rule: no adaptation, or a norm that is exactly zero)
    LARS   S0 = |c g| + wd |p|,  S = r S0 + mom |buf0|
           buf_tol = 2^-21 S + (2^-23 + rel_r) r S0   (+ 4e-6 r |c g| when clipping)        the SGD bound, one more product, r's error
           p_tol   = 2^-23 |p64| + lr (2 buf_tol + 2^-22 (S + |buf64|)) + 1e-38             the SGD bound
           With r = 1 by rule the extra product is exact: buf_tol = 2^-21 S, the SGD test's bound itself.
    LAMB   tol_g = 2^-23 |c g| (+ 4e-6 |c g| when clipping)                                  the Adam test's decoupled form
           tol_m = (1 - b1) tol_g + 2^-22 (|m0| + |g'|)
           tol_v = (1 - b2) 2 |g'| tol_g + 2^-22 (b2 v0 + (1 - b2) g'^2)
           tol_s = min(tol_v / (2 sqrt(v)), sqrt(tol_v));  den = sqrt(v) / sqrt(bc2) + eps;  tol_d = tol_s / sqrt(bc2) + 2^-22 den
           q = (m / bc1) / den;  tol_u = (tol_m / den + |m| tol_d / den^2) / bc1 + 2^-21 (|q| + wd |p|)
           p_tol = 2^-23 |p64| + lr r (tol_u + (rel_r + 2^-22) |u|) + 1e-38                  lr r rounds once, the fma once
"""
import math

import torch

EXTRA = {'lars': ('trust_coefficient', 'eps', 'layer_adaptation'), 'lamb': ('bias_correction', 'layer_adaptation')}
STATE = {'lars': ('momentum_buffer',), 'lamb': ('exp_avg', 'exp_avg_sq')}


def norm64(t):
    return float(t.double().pow(2).sum().sqrt())


# ---------------------------------------------------------------------------------------------- float64 references
def lars_ref(p0, g0, b0, c, clip_on, g):
    """One LARS step of one tensor in float64 from fp32 p0, g0 and b0 (None: the buffer's first step, or momentum 0); ``g`` is the param
    group.  Returns dict(r, rel_r, buf, buf_tol, p, p_tol) -- buf / buf_tol None when momentum is 0."""
    lr, wd, mom, damp, nest = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], g['nesterov']
    p64, cg = p0.double(), c * g0.double()
    wn, gn = norm64(p64), norm64(cg)
    adapted = bool(g['layer_adaptation']) and wn > 0 and gn > 0
    r = g['trust_coefficient'] * wn / (gn + wd * wn + g['eps']) if adapted else 1.0
    rel_r = (2.0 ** -23 + (4e-6 if clip_on else 0.0)) if adapted else 0.0
    S0 = cg.abs() + wd * p64.abs()
    d = r * (cg + wd * p64)
    S = r * S0 + (mom * b0.double().abs() if (mom != 0 and b0 is not None) else 0)
    buf_tol = 2.0 ** -21 * S + ((2.0 ** -23 + rel_r) * r * S0 if adapted else 0) + (4e-6 * r * cg.abs() if clip_on else 0)
    if mom != 0:
        b64 = d if b0 is None else mom * b0.double() + (1 - damp) * d
        step, b64a = (d + mom * b64 if nest else b64), b64.abs()
    else:
        b64, step, b64a = None, d, 0
    e64 = p64 - lr * step
    p_tol = 2.0 ** -23 * e64.abs() + lr * (2 * buf_tol + 2.0 ** -22 * (S + b64a)) + 1e-38
    return dict(r=r, rel_r=rel_r, buf=b64, buf_tol=buf_tol if mom != 0 else None, p=e64, p_tol=p_tol)


def lamb_ref(p0, g0, m0, v0, step, c, clip_on, g):
    """One LAMB step of one tensor in float64 from fp32 p0, g0, m0, v0 (None: zeros); ``step`` is the tensor's count AFTER the step.
    Returns dict(r, rel_r, m, m_tol, v, v_tol, u, u_tol, p, p_tol)."""
    lr, (b1, b2), eps, wd = g['lr'], g['betas'], g['eps'], g['weight_decay']
    bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if g['bias_correction'] else (1.0, 1.0)
    p64, cg = p0.double(), c * g0.double()
    zero = torch.zeros_like(p64)
    m0, v0 = (zero if m0 is None else m0.double()), (zero if v0 is None else v0.double())
    tol_g = 2.0 ** -23 * cg.abs() + (4e-6 * cg.abs() if clip_on else 0)
    m = b1 * m0 + (1 - b1) * cg
    tol_m = (1 - b1) * tol_g + 2.0 ** -22 * (m0.abs() + cg.abs())
    v = b2 * v0 + (1 - b2) * cg * cg
    tol_v = (1 - b2) * 2 * cg.abs() * tol_g + 2.0 ** -22 * (b2 * v0 + (1 - b2) * cg * cg)
    tol_s = torch.minimum(tol_v / (2 * v.sqrt()).clamp_min(1e-300), tol_v.sqrt())
    den = v.sqrt() / math.sqrt(bc2) + eps
    tol_d = tol_s / math.sqrt(bc2) + 2.0 ** -22 * den
    q = (m / bc1) / den
    tol_u = (tol_m / den + m.abs() * tol_d / den ** 2) / bc1 + 2.0 ** -21 * (q.abs() + wd * p64.abs())
    u = q + wd * p64
    wn, un = norm64(p64), norm64(u)
    adapted = bool(g['layer_adaptation']) and wn > 0 and un > 0
    r = wn / un if adapted else 1.0
    rel_r = (2.0 ** -23 + (4e-6 if clip_on else 0.0) + norm64(tol_u) / un) if adapted else 0.0
    e64 = p64 - lr * r * u
    p_tol = 2.0 ** -23 * e64.abs() + lr * r * (tol_u + (rel_r + 2.0 ** -22) * u.abs()) + 1e-38
    return dict(r=r, rel_r=rel_r, m=m, m_tol=tol_m, v=v, v_tol=tol_v, u=u, u_tol=tol_u, p=e64, p_tol=p_tol)


# ---------------------------------------------------------------------------------------------- the rules again, in torch operations
def _ratio(ok, value, adapt, dtype):
    """The trust ratio ``value`` (a float64 0-dim tensor) where ``ok``, 1 elsewhere and without adaptation, rounded once to ``dtype``."""
    if not adapt:
        return torch.ones((), dtype=dtype, device=value.device)
    return torch.where(ok, value, torch.ones_like(value)).to(dtype)


def lars_torch(p, grad, buf, c, g):
    """One LARS step in p's dtype, in place on p and buf (None: first step -> a new buffer); returns (buf, r)."""
    lr, wd, mom, damp, nest = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], g['nesterov']
    gp = grad.mul(c) if c != 1.0 else grad.clone()
    wn = torch.linalg.vector_norm(p, dtype=torch.float64)
    gn = torch.linalg.vector_norm(gp, dtype=torch.float64)
    r = _ratio((wn > 0) & (gn > 0), g['trust_coefficient'] * wn / (gn + wd * wn + g['eps']), g['layer_adaptation'], p.dtype)
    d = gp.add(p, alpha=wd) if wd != 0 else gp
    d.mul_(r)
    step = d
    if mom != 0:
        buf = d.clone() if buf is None else buf.mul_(mom).add_(d, alpha=1 - damp)
        step = d.add(buf, alpha=mom) if nest else buf
    p.add_(step, alpha=-lr)
    return buf, r


def lamb_torch(p, grad, m, v, step, c, g):
    """One LAMB step in p's dtype, in place on p, m and v; ``step`` is the count after the step; returns r."""
    lr, (b1, b2), eps, wd = g['lr'], g['betas'], g['eps'], g['weight_decay']
    bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if g['bias_correction'] else (1.0, 1.0)
    gp = grad.mul(c) if c != 1.0 else grad
    m.lerp_(gp, 1 - b1)
    v.mul_(b2).addcmul_(gp, gp, value=1 - b2)
    u = m.div(bc1).div_(v.sqrt().div_(math.sqrt(bc2)).add_(eps)).add_(p, alpha=wd)
    wn = torch.linalg.vector_norm(p, dtype=torch.float64)
    un = torch.linalg.vector_norm(u, dtype=torch.float64)
    r = _ratio((wn > 0) & (un > 0), wn / un, g['layer_adaptation'], p.dtype)
    p.sub_(u.mul_((r.double() * lr).to(p.dtype)))
    return r


class Restated:
    """The two rules over param groups with the optimizers' state layout: ``param_groups``, ``state[p]`` (momentum_buffer, or step /
    exp_avg / exp_avg_sq), ``trust_ratio`` (a list of 0-dim tensors or None, in param_groups order).  The clip coefficient comes from
    the float64 norm of all gradients; the gradients are left unscaled."""

    def __init__(self, kind, groups, max_grad_norm=None, **defaults):
        self.kind, self.max_grad_norm, self.state = kind, max_grad_norm, {}
        self.param_groups = [dict(defaults, **g) for g in groups]
        self.trust_ratio = None

    def step(self):
        ps = [p for g in self.param_groups for p in g['params']]
        c = 1.0
        if self.max_grad_norm is not None:
            total = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps if p.grad is not None))
            c = min(1.0, self.max_grad_norm / (total + 1e-6))
        ratios = []
        with torch.no_grad():
            for g in self.param_groups:
                for p in g['params']:
                    if p.grad is None or p.numel() == 0:
                        ratios.append(None)
                        continue
                    s = self.state.setdefault(p, {})
                    if self.kind == 'lars':
                        buf, r = lars_torch(p, p.grad, s.get('momentum_buffer'), c, g)
                        if buf is not None:
                            s['momentum_buffer'] = buf
                    else:
                        if not s:
                            s.update(step=torch.tensor(0.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
                        s['step'] += 1
                        r = lamb_torch(p, p.grad, s['exp_avg'], s['exp_avg_sq'], int(s['step']), c, g)
                    ratios.append(r)
        self.trust_ratio = ratios


# ---------------------------------------------------------------------------------------------- the assertion
def snapshot(kind, opt):
    """Per parameter of every group: (p, group, clones of p / g or None, {state name: clone}, step count) -- what the step starts from."""
    snap = []
    for g in opt.param_groups:
        for p in g['params']:
            s = opt.state[p] if p in opt.state else {}
            snap.append((p, g, p.detach().clone(), None if p.grad is None else p.grad.clone(),
                         {k: s[k].clone() for k in STATE[kind] if k in s}, int(float(s['step'])) if 'step' in s else 0))
    return snap


def check_step(kind, opt, snap, c, clip_on, tag=''):
    """The state after one step of ``opt`` against float64 from ``snap`` (hyperparameters as the groups hold them NOW).  Returns
    (worst error / bound ratio, [(r64, rel_r) or None per parameter]) -- None where the step must not have touched the parameter."""
    worst, ratios = 0.0, []

    def within(name, i, got, want, tol):
        nonlocal worst
        err = (got.double() - want).abs()
        ratio = float((err / tol.clamp_min(1e-300)).max())
        assert bool((err <= tol).all()), f'{tag} param {i} ({got.numel()} elements) {name}: err/bound {ratio:.3g}'
        worst = max(worst, ratio)

    for i, (p, g, p0, g0, s0, step0) in enumerate(snap):
        s = opt.state[p] if p in opt.state else {}
        if g0 is None or p0.numel() == 0:
            ratios.append(None)
            assert torch.equal(p.detach(), p0), f'{tag} param {i}: touched without a gradient'
            if g0 is None:
                assert all(torch.equal(s[k], s0[k]) for k in s0) and all(k in s0 for k in STATE[kind] if k in s), \
                    f'{tag} param {i}: state changed without a gradient'
                assert not s0 or 'step' not in s or int(float(s['step'])) == step0, f'{tag} param {i}: counted without a gradient'
            continue
        if kind == 'lars':
            ref = lars_ref(p0, g0, s0.get('momentum_buffer'), c, clip_on, g)
            if g['momentum'] != 0:
                buf = s.get('momentum_buffer')
                assert buf is not None and buf.shape == p.shape, f'{tag} param {i}: no momentum buffer'
                within('buf', i, buf, ref['buf'], ref['buf_tol'])
            else:
                assert 'momentum_buffer' not in s, f'{tag} param {i}: momentum 0 keeps no buffer'
        else:
            assert int(float(s['step'])) == step0 + 1, f'{tag} param {i}: step {float(s["step"])}, expected {step0 + 1}'
            assert 'max_exp_avg_sq' not in s
            ref = lamb_ref(p0, g0, s0.get('exp_avg'), s0.get('exp_avg_sq'), step0 + 1, c, clip_on, g)
            within('exp_avg', i, s['exp_avg'], ref['m'], ref['m_tol'])
            within('exp_avg_sq', i, s['exp_avg_sq'], ref['v'], ref['v_tol'])
        within('p', i, p.detach(), ref['p'], ref['p_tol'])
        ratios.append((ref['r'], ref['rel_r']))
    return worst, ratios


def check_ratios(trust_ratio, ratios, tag=''):
    """``trust_ratio`` (the optimizer's vector, or Restated's list) entry by entry against check_step's float64 ratios: within rel_r,
    exactly 1 where the rule says 1, exactly 0 (None in the list) for a parameter the step did not touch.  Returns the worst ratio."""
    assert len(trust_ratio) == len(ratios), tag
    worst = 0.0
    for i, want in enumerate(ratios):
        got = trust_ratio[i]
        if want is None:
            assert got is None or float(got) == 0.0, f'{tag} entry {i}: {float(got)} for an untouched parameter'
            continue
        r64, rel = want
        err = abs(float(got) - r64)
        assert err <= rel * r64, f'{tag} entry {i}: {float(got)!r} vs {r64!r}, err/bound {err / max(rel * r64, 1e-300):.3g}'
        if rel:
            worst = max(worst, err / (rel * r64))
    return worst


# ---------------------------------------------------------------------------------------------- rows and group layouts of the step tests
#             lr    wd    momentum dampening nesterov clip  layout   trust_coefficient
LARS_ROWS = [(0.1, 5e-4, 0.9, 0.0, False, None, 'two', 1e-3),
             (0.1, 5e-4, 0.9, 0.0, False, 1.0, 'three', 1e-3),
             (0.1, 0.0, 0.9, 0.0, True, 1.0, 'two', 1e-3),
             (0.05, 5e-4, 0.5, 0.1, False, None, 'three', 1e-3),
             (0.1, 5e-4, 0.0, 0.0, False, 0.5, 'two', 1e-3),
             (0.02, 5e-4, 0.9, 0.0, False, 10.0, 'nine', 2e-3)]
#             lr    b1   b2     eps   wd    bias_correction clip  layout
LAMB_ROWS = [(1e-3, 0.9, 0.999, 1e-6, 0.01, True, None, 'two'),
             (1e-3, 0.9, 0.999, 1e-6, 0.01, True, 1.0, 'three'),
             (1e-2, 0.9, 0.999, 1e-6, 0.0, True, 1.0, 'two'),
             (1e-3, 0.5, 0.9, 1e-6, 5e-4, False, None, 'three'),
             (1e-3, 0.9, 0.99, 1e-8, 0.01, True, 10.0, 'nine'),
             (1e-3, 0.0, 0.999, 1e-3, 0.01, False, 0.5, 'two')]
ROWS = [('lars', i) for i in range(len(LARS_ROWS))] + [('lamb', i) for i in range(len(LAMB_ROWS))]


def row_args(algo, i):
    """(optimizer keywords with every group key spelled out, clip, layout) of row i."""
    if algo == 'lars':
        lr, wd, mom, damp, nest, clip, layout, tc = LARS_ROWS[i]
        return dict(lr=lr, weight_decay=wd, momentum=mom, dampening=damp, nesterov=nest, trust_coefficient=tc, eps=1e-8,
                    layer_adaptation=True), clip, layout
    lr, b1, b2, eps, wd, bias, clip, layout = LAMB_ROWS[i]
    return dict(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, bias_correction=bias, layer_adaptation=True), clip, layout


def layout_groups(params, lr, layout, tail=()):
    """Param groups over ``params``.  'two': even / odd positions, the second at lr * 0.1 (the SGD tests' layout); 'three': three of the
    parameters move to a group WITHOUT layer adaptation and without weight decay (the recipe for biases and BatchNorm weights); 'nine':
    nine groups round robin (a launch carries eight), each at its own lr, the fifth without adaptation.  ``tail``: parameters appended to
    the first groups one by one (the grad-less and the frozen one)."""
    if layout == 'two':
        groups = [dict(params=params[0::2]), dict(params=params[1::2], lr=lr * 0.1)]
    elif layout == 'three':
        plain = params[2:10:3]                               # (positions 2, 5, 8: the tensors appended behind stay adapted)
        rest = [p for p in params if not any(p is q for q in plain)]
        groups = [dict(params=rest[0::2]), dict(params=rest[1::2], lr=lr * 0.1),
                  dict(params=plain, layer_adaptation=False, weight_decay=0.0)]
    else:
        groups = [dict(params=params[k::9], lr=lr * (1 + 0.25 * k)) for k in range(9)]
        groups[4]['layer_adaptation'] = False
    for k, p in enumerate(tail):
        groups[k]['params'] = groups[k]['params'] + [p]
    return groups
