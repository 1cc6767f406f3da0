"""The optimizer step on the device: ``SGD`` (torch.optim.SGD's update rule and state layout, optionally with the gradient-norm clip
fused in) and a stand-alone ``clip_grad_norm_``, each two launches of csrc/optim.hip over a device table of tensors; ``Adam`` and
``AdamW`` (torch's rule, state names and checkpoints, the same optional clip) on the same tables and csrc/optim_adam.hip; ``LARS`` and
``LAMB`` (csrc/optim_lars.hip), the two with a per-tensor trust ratio that is formed and consumed on the device; and what a
training loop keeps next to its optimizer, ``AveragedModel`` (torch.optim.swa_utils.AveragedModel's layout and checkpoints: an EMA or
the equal SWA average of the weights, every tensor in ONE launch of csrc/optim_avg.hip, the update count on the device) with an
``update_bn`` that works on this engine (torch's sets ``momentum = None``, which the launch plans cannot take); ``grad_stats`` /
``GradMonitor`` (gssd/grad_stats.py, re-exported here): per-parameter norms, maxima and non-finite counts in two launches; and
``GradAccumulator``, the weighted mean of the gradients of k micro-batches in ONE launch of csrc/optim_accum.hip per micro-batch.

The reference driver's step (train_lesion_multiphase_v2.py:242-253) then runs on this library's kernels alone:

    optimizer = gssd.optim.SGD(groups, lr=..., momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)   # :603-626
    ...
    loss.backward(); optimizer.step()                                                                     # :251-253, clip included

The four optimizers are one core, ``_DeviceOptimizer``: it owns step() (closure, hyperparameters, table key, build, clip, launch, step
counts, version bump), the walk over the parameters with its validation and the refusals; a class adds its state tensors, its item rows,
its hyper struct and its one library call, and keeps what it built in a ``_Built``.  The device tables themselves -- item and chunk
layouts, their upload, the aligned slices of one flat tensor that fresh state lives in -- are gssd/optim_table.py, which
gssd/grad_stats.py shares.

Nothing here reads back to the host.  There is no CPU fallback: a parameter or gradient that is not a contiguous fp32 device tensor
raises GssdError.
"""
import copy
import itertools

import torch

from . import _lib
from ._lib import GssdError, check, lib
from .optim_table import (ACCUM_ADD, ACCUM_FIRST, ACCUM_SCALE, CHUNK, _ACCUM_ITEM, _ADAM_ITEM, _AVG_ITEM, _CHUNK, _ITEM,      # noqa: F401
                          _Table, _check_tensor, _stream, accum_plan, build_chunks, flat_views, item_chunk_prefix)
# per-parameter gradient / weight statistics on the same tables (gssd/grad_stats.py, csrc/optim_stats.hip), re-exported here: they sit
# in the training loop between backward() and step() like everything below
from .grad_stats import GradMonitor, GradStats, grad_stats      # noqa: F401

FIRST_STEP = 1
AVG_LERP, AVG_COPY32, AVG_COPY64 = 0, 1, 2     # gssd_avg_item.kind
ACCUM_W_F32, ACCUM_RESET, ACCUM_FINALIZE = 1, 2, 4     # launch flags of gssd_grad_accumulate_f32


_PLAIN = (float, int)
_NO_CLIP = (None, 0, -1.0, None)     # (partials, n_partials, max_norm, norm_out) as every step function takes them


def _holds_tensor(v):
    """Whether a hyperparameter is a tensor or (betas) a pair with one."""
    if isinstance(v, (tuple, list)):
        return isinstance(v[0], torch.Tensor) or isinstance(v[1], torch.Tensor)
    return isinstance(v, torch.Tensor)


class _Built:
    """What a step keeps from one call to the next, built for one ``key`` (the optimizer's ``_table_key()``): ``table``, the _Table of
    the parameters that take part (None: there are none); ``norm``, the gssd_sgd_item _Table of their gradients whose partial sums
    the clip reads (None without max_grad_norm); ``params``, those parameters; ``steps``, the one host tensor their step counts are
    views of (None: the rule keeps no count); ``device``; ``first``, whether the table carries first-step flags and so serves one step
    only; ``ratios``, the _Ratios of a trust-ratio rule (None otherwise); ``clip``, whether it was built for a clipping step."""
    __slots__ = ('key', 'clip', 'table', 'norm', 'params', 'steps', 'device', 'first', 'ratios')

    def __init__(self, params, device):
        self.key = self.clip = self.table = self.norm = self.steps = self.ratios = None
        self.params, self.device, self.first = params, device, False


class _DeviceOptimizer(torch.optim.Optimizer):
    """The core of the four optimizers: the step() skeleton, the walk over the parameters with its validation, the refusals of what the
    kernels do not implement, the clip and the version bump.  A subclass supplies what differs: ``_table_key()``, ``_state_tensors()``
    (the state a parameter brings along), ``_rows()`` (fresh state and the item rows), ``_fill()`` (one group's hyper struct) and
    ``_launch()`` (its one ``lib.gssd_*_step_f32`` call)."""
    _OFF = ()              # keys accepted for signature compatibility, in the constructor and in param_groups: they must stay off
    _NUMBERS = ()          # hyperparameters that must be Python numbers (a tensor would need a host read per step)
    _HYPER = None          # the ctypes struct of one group's hyperparameters
    _ITEM_DTYPE = _ITEM    # the item layout of the update kernel
    _OFF_NAME = None       # the class the flag refusals name (default: the class itself)
    _SUMSQ_LAUNCH = True   # the clip's norm takes gssd_grad_sumsq_f32, a launch of its own
    _CHUNK_PREFIX = False  # the table carries the items' chunk prefix

    def __init__(self, params, defaults, flags, max_grad_norm):
        self._refuse_flags(flags)
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f'Invalid max_grad_norm: {max_grad_norm}')
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self._launches = 0         # steps that reached the device: the kernels' `t`
        self._table = None         # the _Built of the last step
        super().__init__(params, defaults)

    def _refuse_flags(self, values, gi=None):
        name = self._OFF_NAME or type(self).__name__
        for k in self._OFF:
            if values.get(k):
                where = k if gi is None else f'param_groups[{gi}][{k!r}]'
                raise NotImplementedError(f'gssd.optim.{name}: {where}={values[k]!r} is not implemented')

    def _hyper(self):
        # (runs at every step: the two refusals cost a C-level pass over the names when there is nothing to refuse)
        arr = (self._HYPER * len(self.param_groups))()
        off, numbers, fill = self._OFF, self._NUMBERS, self._fill
        for gi, (h, g) in enumerate(zip(arr, self.param_groups)):
            if any(map(g.get, off)):
                self._refuse_flags(g, gi)
            for k in numbers:
                v = g[k]
                if v.__class__ not in _PLAIN and _holds_tensor(v):
                    raise NotImplementedError(f'gssd.optim.{type(self).__name__}: {k} must be a Python number')
            fill(h, g, gi)
        return arr

    def _ratios(self, table, params, device):
        return None

    def _build(self):
        todo, device = [], None
        for gi, g in enumerate(self.param_groups):
            for pi, p in enumerate(g['params']):
                if p.grad is None:
                    continue
                what = f'param_groups[{gi}]["params"][{pi}] (shape {tuple(p.shape)})'
                _check_tensor(p.detach(), what, device)
                device = p.device
                _check_tensor(p.grad, 'the gradient of ' + what, device)
                if p.grad.shape != p.shape:
                    raise GssdError(f'gssd.optim: the gradient of {what} has shape {tuple(p.grad.shape)}')
                if p.numel() == 0:
                    continue
                for label, t in self._state_tensors(g, p, what):
                    _check_tensor(t, f'{label} of ' + what, device)
                    if t.numel() != p.numel():
                        raise GssdError(f'gssd.optim: {label} of {what} has {t.numel()} elements')
                todo.append((gi, g, p))
        b = _Built([p for _, _, p in todo], device)
        rows = self._rows(todo, device, b)
        if rows:
            b.table = _Table(rows, device, self._ITEM_DTYPE, self._CHUNK_PREFIX)
            if self.max_grad_norm is not None:
                b.norm = b.table if self._ITEM_DTYPE is _ITEM else \
                    _Table([(0, p.grad.data_ptr(), 0, p.numel(), 0, 0) for p in b.params], device)
                if self.grad_norm is None:
                    self.grad_norm = torch.zeros((), device=device, dtype=torch.float32)
        b.ratios = self._ratios(b.table, b.params, device)
        b.key, b.clip = self._table_key(), self.max_grad_norm is not None
        return b

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hyper = self._hyper()
        clip = self.max_grad_norm is not None
        b = self._table
        if b is None or b.key != self._table_key() or b.clip != clip:      # (a max_grad_norm set or cleared later: the norm table)
            b = self._table = self._build()
        if b.table is None:
            return loss
        with torch.cuda.device(b.device):
            stream = _stream(b.device)
            if clip and self._SUMSQ_LAUNCH:
                b.norm.sumsq(stream)
            self._launch(b, hyper, (b.norm.partials.data_ptr(), b.norm.n_partials, self.max_grad_norm, self.grad_norm.data_ptr()) if clip
                         else _NO_CLIP, stream)
        self._launches += 1
        if b.steps is not None:
            b.steps.add_(1.0)
        torch.autograd.graph.increment_version(b.params)
        if b.first:
            self._table = None       # the table carries first-step flags: the next step builds one without them
        return loss


class SGD(_DeviceOptimizer):
    """torch.optim.SGD's constructor, update rule, ``param_groups`` and ``state[p]['momentum_buffer']`` -- checkpoints go either way --
    with the whole step in ONE launch of csrc/optim.hip for all parameters of all groups.

    ``max_grad_norm`` (extra keyword): when set, step() is ``clip_grad_norm_(all params, max_grad_norm)`` + the update in two launches.
    The clip coefficient is applied inside the update; the gradients themselves are left UNSCALED (read ``p.grad`` after step() and you
    see what backward wrote).  The total norm of the step is left in ``self.grad_norm``, a 0-dim device tensor that the next step
    overwrites (None without max_grad_norm).

    Momentum buffers are created on the first step as slices of one flat tensor (a gradient or group that appears later gets another);
    after ``load_state_dict`` they are whatever torch put there.

    ``maximize``, ``foreach``, ``fused`` and ``differentiable`` are accepted for signature compatibility and must keep their defaults.
    Hyperparameters are read from ``param_groups`` at every step (Python numbers), so editing ``param_groups[i]['lr']`` takes effect at
    once.  Parameters whose ``grad`` is None are skipped, as in torch.  After the launch every updated parameter's version counter is
    bumped: GssdEngine re-packs its weights on that signal."""

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False, foreach=None,
                 differentiable=False, fused=None, max_grad_norm=None):
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError('gssd.optim.SGD: lr must be a Python number (a tensor lr would need a host read per step)')
        if lr < 0.0:
            raise ValueError(f'Invalid learning rate: {lr}')
        if momentum < 0.0:
            raise ValueError(f'Invalid momentum value: {momentum}')
        if weight_decay < 0.0:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError('Nesterov momentum requires a momentum and zero dampening')
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, dict(maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused),
                         max_grad_norm)

    _OFF = ('maximize', 'foreach', 'differentiable', 'fused')
    _OFF_NAME = 'SGD'          # (LARS's refusals of SGD's flags name SGD)
    _NUMBERS = ('lr', 'weight_decay', 'momentum', 'dampening')
    _HYPER = _lib.SgdHyper

    # ------------------------------------------------------------------------------------------
    def _table_key(self):
        """Everything the device table depends on: per group whether it keeps momentum, per parameter the storage pointers of the
        parameter, its gradient and its momentum buffer (0: none), and the gradient's dtype and size (a new gradient that the allocator
        put at the old address must be validated again)."""
        key, state = [], self.state.get                 # (.get: asking creates no state entry)
        for g in self.param_groups:
            key.append(g['momentum'] != 0)
            for p in g['params']:
                s, grad = state(p), p.grad
                buf = s.get('momentum_buffer') if s else None
                if grad is None:
                    key.append((p.data_ptr(), 0, 0 if buf is None else buf.data_ptr()))
                else:
                    key.append((p.data_ptr(), grad.data_ptr(), 0 if buf is None else buf.data_ptr(), grad.dtype, grad.numel()))
        return tuple(key)

    def _state_tensors(self, g, p, what):
        buf = self.state[p].get('momentum_buffer') if g['momentum'] != 0 and p in self.state else None
        return [] if buf is None else [('the momentum buffer', buf)]

    def _rows(self, todo, device, built):
        # new momentum buffers: 16-byte aligned slices of one flat tensor.  All of them on the first step; a gradient or group that
        # appears later gets a flat tensor of its own
        fresh = [p for _, g, p in todo if g['momentum'] != 0 and self.state[p].get('momentum_buffer') is None]
        for p, buf in zip(fresh, flat_views(fresh, device)):
            self.state[p]['momentum_buffer'] = buf
        fresh = set(fresh)
        built.first = bool(fresh)
        return [(p.data_ptr(), p.grad.data_ptr(), self.state[p]['momentum_buffer'].data_ptr() if g['momentum'] != 0 else 0, p.numel(), gi,
                 FIRST_STEP if p in fresh else 0) for gi, g, p in todo]

    def _fill(self, h, g, gi):
        h.lr, h.weight_decay, h.momentum, h.dampening, h.nesterov = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], \
            bool(g['nesterov'])

    def _launch(self, b, hyper, clip, stream):
        check(lib.gssd_sgd_step_f32(*b.table.head, hyper, len(hyper), *clip, stream))


_ADAM_OFF = ('maximize', 'foreach', 'capturable', 'differentiable', 'fused')
_ADAM_STATE = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


class Adam(_DeviceOptimizer):
    """torch.optim.Adam's constructor, update rule (amsgrad and ``decoupled_weight_decay`` included), ``param_groups`` and state
    ``step`` / ``exp_avg`` / ``exp_avg_sq`` / ``max_exp_avg_sq`` -- checkpoints go either way -- with the whole step in ONE launch of
    csrc/optim_adam.hip for all parameters of all groups (one per eight groups beyond eight).

    ``max_grad_norm`` (extra keyword) is SGD's: when set, step() is ``clip_grad_norm_(all params, max_grad_norm)`` + the update in two
    launches, the coefficient is applied inside the update, ``p.grad`` is left UNSCALED and the total norm of the step is left in
    ``self.grad_norm``, a 0-dim device tensor that the next step overwrites (None without max_grad_norm).

    ``state[p]['step']`` is torch's default, a 0-dim float32 CPU tensor, counted on the host (the counts of one table are views of one
    host tensor, so a step is one add_ for all of them); the kernel gets the step of every parameter from one launch argument, the
    number of launches so far, and an offset in the table (a parameter whose gradient appears later starts at step 1, one whose gradient
    goes away stands still).  The moments are created on a parameter's first step as 16-byte aligned slices of flat ZERO tensors (zeros
    give torch's first step); after ``load_state_dict`` they are whatever torch put there.  A ``step`` that arrives as a DEVICE tensor
    (a checkpoint of torch's fused or capturable form) is read back ONCE, when the table is built, and lives on the host from then on.
    A group that turns ``amsgrad`` on later gets a zero ``max_exp_avg_sq``.

    ``maximize``, ``foreach``, ``capturable``, ``differentiable`` and ``fused`` are accepted for signature compatibility and must keep
    their defaults; ``lr`` and ``betas`` must be Python numbers.  Hyperparameters are read from ``param_groups`` at every step.
    Parameters whose ``grad`` is None are skipped, as in torch.  After the launch every updated parameter's version counter is bumped:
    GssdEngine re-packs its weights on that signal."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False, max_grad_norm=None):
        name = type(self).__name__
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError(f'gssd.optim.{name}: lr and betas must be Python numbers (a tensor would need a host read per step)')
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 0: {betas[0]}')
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f'Invalid beta parameter at index 1: {betas[1]}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if not (isinstance(betas[0], float) and isinstance(betas[1], float)):
            raise ValueError('betas must be either both floats or both Tensors')
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults, dict(maximize=maximize, foreach=foreach, capturable=capturable, differentiable=differentiable,
                                                fused=fused), max_grad_norm)

    _OFF = _ADAM_OFF
    _NUMBERS = ('lr', 'betas', 'eps', 'weight_decay')
    _HYPER = _lib.AdamHyper
    _ITEM_DTYPE = _ADAM_ITEM

    # ------------------------------------------------------------------------------------------
    def _table_key(self):
        """Everything the device table depends on: whether the step clips, per group whether it runs AMSGrad, per parameter the storage
        pointers of the parameter, its gradient and its three moment tensors (0: none), the identity of its step tensor, and the gradient's
        dtype and size (a new gradient that the allocator put at the old address must be validated again)."""
        key, state = [self.max_grad_norm is not None], self.state.get       # (.get: asking creates no state entry)
        for g in self.param_groups:
            key.append(bool(g['amsgrad']))
            for p in g['params']:
                s, grad = state(p), p.grad
                if s:
                    m, v, x = s.get('exp_avg'), s.get('exp_avg_sq'), s.get('max_exp_avg_sq')
                    s = (m is not None and m.data_ptr(), v is not None and v.data_ptr(), x is not None and x.data_ptr(), id(s.get('step')))
                else:
                    s = None
                if grad is None:
                    key.append((p.data_ptr(), s))
                else:
                    key.append((p.data_ptr(), s, grad.data_ptr(), grad.dtype, grad.numel()))
        return tuple(key)

    def _fill(self, h, g, gi):
        b1, b2 = g['betas']
        h.lr, h.beta1, h.beta2 = g['lr'], b1, b2
        h.one_minus_beta1, h.one_minus_beta2 = 1.0 - b1, 1.0 - b2            # formed in double, rounded once
        h.eps, h.weight_decay = g['eps'], g['weight_decay']
        self._fill_rule(h, g, gi)

    def _fill_rule(self, h, g, gi):
        h.amsgrad, h.decoupled = bool(g['amsgrad']), bool(g.get('decoupled_weight_decay', False))

    def _state_tensors(self, g, p, what):
        s = self.state.get(p) or {}
        for k in _ADAM_STATE:
            if k in s:
                yield k, s[k]
        if s and not ('step' in s and 'exp_avg' in s and 'exp_avg_sq' in s):
            raise GssdError(f'gssd.optim: the state of {what} holds {sorted(s)}, not step, exp_avg and exp_avg_sq')

    def _rows(self, todo, device, built):
        # new moments: 16-byte aligned slices of one flat ZERO tensor per kind.  All of them on the first step; a gradient or group that
        # appears later gets flat tensors of its own
        fresh = {k: [p for _, g, p in todo if k not in (self.state.get(p) or {}) and (g['amsgrad'] or k != 'max_exp_avg_sq')]
                 for k in _ADAM_STATE}
        # the step counts of the table's parameters move into ONE host tensor, state[p]['step'] becoming a 0-dim view of it, so that a
        # step counts them all with one add_ (253 host tensors incremented one by one cost more than the launch).  A count that arrives
        # as a device tensor is read back here, once
        built.steps = counts = torch.tensor([float(self.state[p]['step']) if self.state.get(p) else 0.0 for _, _, p in todo],
                                            dtype=torch.float32)
        for i, (_, _, p) in enumerate(todo):
            self.state[p]['step'] = counts[i]
        for k in _ADAM_STATE:                                                     # (torch's key order: step, exp_avg, exp_avg_sq, max_...)
            for p, t in zip(fresh[k], flat_views(fresh[k], device, zero=True)):
                self.state[p][k] = t
        rows = []
        for i, (gi, g, p) in enumerate(todo):
            s = self.state[p]
            rows.append((p.data_ptr(), p.grad.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr(),
                         s['max_exp_avg_sq'].data_ptr() if g['amsgrad'] else 0, p.numel(), gi, 0, self._launches - int(counts[i])))
        return rows

    def _launch(self, b, hyper, clip, stream):
        check(lib.gssd_adam_step_f32(*b.table.head, hyper, len(hyper), self._launches + 1, *clip, stream))


class AdamW(Adam):
    """torch.optim.AdamW: ``Adam`` with ``decoupled_weight_decay=True`` and weight_decay 1e-2 by default."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, decoupled_weight_decay=True, max_grad_norm=max_grad_norm)


# ----------------------------------------------------------------------------------------------
# layer-wise adaptive rates
# ----------------------------------------------------------------------------------------------
def step_launches(n_groups, cap=8):
    """Update launches of a step over ``n_groups`` param groups: one per ``cap`` groups (the hyperparameters travel by value)."""
    return max(1, -(-n_groups // cap))


class _Ratios:
    """What a trust-ratio step needs next to its table (which carries the items' chunk prefix): the items' slots in ``trust_ratio`` (the
    index of the parameter in ``param_groups`` order) and the per-chunk norm records -- owned by the table they were built for."""

    def __init__(self, table, params, slot_of, device):
        self.slot = torch.tensor([slot_of[id(p)] for p in params], dtype=torch.int32).to(device)
        self.workspace = torch.empty(lib.gssd_lars_workspace_bytes(table.n_chunks) // 8, device=device, dtype=torch.float64)


class _TrustRatio:
    """Shared by LARS and LAMB: the extra group keys (filled from the defaults in new groups and in loaded checkpoints that lack them)
    and ``trust_ratio``."""
    _CHUNK_PREFIX = True

    def add_param_group(self, param_group):
        self.defaults.update(self._extra_defaults)          # (torch fills a new group from self.defaults)
        super().add_param_group(param_group)

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:                         # a checkpoint of SGD / Adam has none of the extra keys
            for k, v in self._extra_defaults.items():
                g.setdefault(k, v)
        self._table = None

    def _ratios(self, table, params, device):
        """The _Ratios of a freshly built table, and ``trust_ratio`` zeroed (entries of parameters that left the table read 0)."""
        if table is None:
            return None
        order = [p for g in self.param_groups for p in g['params']]
        if self.trust_ratio is None or self.trust_ratio.numel() != len(order) or self.trust_ratio.device != device:
            self.trust_ratio = torch.zeros(len(order), device=device, dtype=torch.float32)
        else:
            self.trust_ratio.zero_()
        return _Ratios(table, params, {id(p): i for i, p in enumerate(order)}, device)


class LARS(_TrustRatio, SGD):
    """Layer-wise adaptive rate scaling (You et al. 2017) on ``SGD``'s state and checkpoint format: torch.optim.SGD's rule with the
    decayed gradient of every parameter TENSOR scaled by its trust ratio, the learning rate outside the momentum buffer --

        r    = layer_adaptation and ||w|| != 0 and ||g'|| != 0 ? trust_coefficient ||w|| / (||g'|| + weight_decay ||w|| + eps) : 1
        d    = r (g' + weight_decay w);   buf = first ? d : momentum buf + (1 - dampening) d
        step = nesterov ? d + momentum buf : buf   (momentum 0: step = d);   w -= lr step

    with g' = c g, c the clip coefficient of ``max_grad_norm`` (1 without), ||.|| the 2-norm over one tensor and ||w|| the norm BEFORE
    the update -- in TWO launches of csrc/optim_lars.hip for all parameters of all groups, clip or no clip (one more per eight groups
    beyond eight; ``self.launches`` holds the count of the last step).  Norms are summed in fp64 in a fixed order: a step is bitwise
    reproducible.  A norm that is exactly zero gives r = 1; a NaN or inf norm gives a NaN ratio, which propagates into that tensor as a
    NaN gradient does in SGD (there is no skip-on-non-finite step).

    Per-group keys next to SGD's: ``trust_coefficient`` (1e-3), ``eps`` (1e-8) and ``layer_adaptation`` (True; the usual recipe puts
    biases and BatchNorm weights in a group with False, which then takes SGD's step exactly).  They travel in ``param_groups``; a
    checkpoint of ``gssd.optim.SGD`` / ``torch.optim.SGD`` loads with them filled from the defaults, and a LARS checkpoint loads into
    those.

    ``self.trust_ratio``: an fp32 device vector with one entry per parameter in ``param_groups`` order, written by the step (None before
    the first): r for every updated parameter, 1 in a group without adaptation, 0 for a parameter the step did not touch.  The host
    never reads it; it stands until the next step overwrites it.  ``max_grad_norm`` / ``self.grad_norm`` and everything else are SGD's."""
    _NUMBERS = SGD._NUMBERS + ('trust_coefficient', 'eps')
    _HYPER = _lib.LarsHyper
    _SUMSQ_LAUNCH = False      # (the norm launch leaves the clip's partial sums)

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, trust_coefficient=1e-3, eps=1e-8,
                 layer_adaptation=True, maximize=False, foreach=None, differentiable=False, fused=None, max_grad_norm=None):
        for k, v in (('trust_coefficient', trust_coefficient), ('eps', eps)):
            if isinstance(v, torch.Tensor):
                raise NotImplementedError(f'gssd.optim.LARS: {k} must be a Python number')
            if not v >= 0.0:
                raise ValueError(f'Invalid {k} value: {v}')
        self._extra_defaults = dict(trust_coefficient=trust_coefficient, eps=eps, layer_adaptation=bool(layer_adaptation))
        self.trust_ratio = None
        self.launches = 0
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov, maximize=maximize, foreach=foreach,
                         differentiable=differentiable, fused=fused, max_grad_norm=max_grad_norm)

    def _fill(self, h, g, gi):
        for k in ('trust_coefficient', 'eps'):
            if not g[k] >= 0.0:
                raise ValueError(f'gssd.optim.{type(self).__name__}: param_groups[{gi}][{k!r}]={g[k]!r} is negative')
        super()._fill(h, g, gi)
        h.trust_coefficient, h.eps, h.adapt = g['trust_coefficient'], g['eps'], bool(g['layer_adaptation'])

    def _launch(self, b, hyper, clip, stream):
        rt = b.ratios
        check(lib.gssd_lars_step_f32(*b.table.head, b.table.chunk0.data_ptr(), rt.slot.data_ptr(), hyper, len(hyper), rt.workspace.data_ptr(),
                                     *clip, self.trust_ratio.data_ptr(), stream))
        self.launches = 1 + step_launches(len(hyper))


class LAMB(_TrustRatio, Adam):
    """LAMB (You et al. 2020) on ``Adam``'s state and checkpoint format (``step`` / ``exp_avg`` / ``exp_avg_sq``; there is no amsgrad):
    Adam's moments with a per-tensor trust ratio on the full update --

        m = b1 m + (1 - b1) g';   v = b2 v + (1 - b2) g'^2
        u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + weight_decay w        bc1 = 1 - b1^t, bc2 = 1 - b2^t (1 with bias_correction=False)
        r = layer_adaptation and ||w|| != 0 and ||u|| != 0 ? ||w|| / ||u|| : 1;   w -= lr r u

    with g' = c g, c the clip coefficient of ``max_grad_norm`` (1 without), ||.|| the 2-norm over one tensor and ||w|| the norm BEFORE
    the update -- in TWO launches of csrc/optim_lars.hip for all parameters of all groups, three with the clip (one more per eight
    groups beyond eight; ``self.launches`` holds the count of the last step).  The second launch forms u again from the stored moments
    instead of reading a stored copy: the same traffic, no fourth state tensor.  Norms are summed in fp64 in a fixed order: a step is
    bitwise reproducible.  A norm that is exactly zero gives r = 1; a NaN or inf norm gives a NaN ratio, which propagates into that tensor
    as a NaN gradient does in Adam.

    Defaults: lr 1e-3, betas (0.9, 0.999), eps 1e-6, weight_decay 0.01.  Per-group keys next to Adam's: ``bias_correction`` (True) and
    ``layer_adaptation`` (True; False for biases and BatchNorm weights).  They travel in ``param_groups``; a checkpoint of
    ``gssd.optim.Adam`` / ``torch.optim.Adam`` loads with them filled from the defaults, and a LAMB checkpoint loads into those (the
    groups carry Adam's keys, ``amsgrad`` and ``decoupled_weight_decay`` False).

    ``self.trust_ratio`` is LARS's: one fp32 device entry per parameter in ``param_groups`` order, r for every updated parameter, 1 in
    a group without adaptation, 0 for a parameter the step did not touch, never read by the host.  Step counts, ``max_grad_norm`` /
    ``self.grad_norm`` and everything else are Adam's."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, *, bias_correction=True, layer_adaptation=True,
                 amsgrad=False, foreach=None, maximize=False, capturable=False, differentiable=False, fused=None, max_grad_norm=None):
        if amsgrad:
            raise NotImplementedError('gssd.optim.LAMB: there is no amsgrad')
        self._extra_defaults = dict(bias_correction=bool(bias_correction), layer_adaptation=bool(layer_adaptation))
        self.trust_ratio = None
        self.launches = 0
        super().__init__(params, lr, betas, eps, weight_decay, False, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, max_grad_norm=max_grad_norm)

    _OFF = _ADAM_OFF + ('amsgrad', 'decoupled_weight_decay')
    _HYPER = _lib.LambHyper

    def _fill_rule(self, h, g, gi):
        h.bias_correction, h.adapt = bool(g['bias_correction']), bool(g['layer_adaptation'])

    def _launch(self, b, hyper, clip, stream):
        rt = b.ratios
        check(lib.gssd_lamb_step_f32(*b.table.head, b.table.chunk0.data_ptr(), rt.slot.data_ptr(), hyper, len(hyper), self._launches + 1,
                                     rt.workspace.data_ptr(), *clip, self.trust_ratio.data_ptr(), stream))
        self.launches = int(self.max_grad_norm is not None) + 1 + step_launches(len(hyper))


# (device, ((grad ptr, numel), ...)) -> _Table, the few most recent: building a table costs a host-to-device copy, and a training loop
# clips the same gradients every step.  Only the read-only item / chunk lists are shared; every call brings its own partial sums, so
# calls on several streams do not meet.  At most _CLIP_TABLES_MAX tables (~100 KB each for this network) outlive their model.
_CLIP_TABLES = {}
_CLIP_TABLES_MAX = 4


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False):
    """torch.nn.utils.clip_grad_norm_ (the driver's line 252) for contiguous fp32 device gradients, in two launches: the gradients are
    scaled in place by min(1, max_norm / (total_norm + 1e-6)), and the total norm comes back as a 0-dim device tensor.  Only the 2-norm;
    ``error_if_nonfinite`` would need a host read and is not implemented."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f'gssd.optim.clip_grad_norm_: norm_type={norm_type!r} (only 2)')
    if error_if_nonfinite:
        raise NotImplementedError('gssd.optim.clip_grad_norm_: error_if_nonfinite=True needs a host read of the norm')
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads, device = [], None
    for i, p in enumerate(parameters):
        if p.grad is None:
            continue
        _check_tensor(p.grad, f'the gradient of parameter {i} (shape {tuple(p.shape)})', device)
        device = p.grad.device
        if p.grad.numel():
            grads.append(p.grad)
    if not grads:
        if device is None:
            raise GssdError('gssd.optim.clip_grad_norm_: no parameter has a gradient (and so no device to put the norm on)')
        return torch.zeros((), device=device, dtype=torch.float32)
    key = (device, tuple((g.data_ptr(), g.numel()) for g in grads))
    table = _CLIP_TABLES.pop(key, None)
    if table is None:
        table = _Table([(0, g.data_ptr(), 0, g.numel(), 0, 0) for g in grads], device)
        while len(_CLIP_TABLES) >= _CLIP_TABLES_MAX:
            _CLIP_TABLES.pop(next(iter(_CLIP_TABLES)))
    _CLIP_TABLES[key] = table
    norm = torch.empty((), device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        stream = _stream(device)
        partials = torch.empty(table.n_partials, device=device, dtype=torch.float64)
        table.sumsq(stream, partials)
        check(lib.gssd_grad_scale_clip_f32(*table.head, partials.data_ptr(), table.n_partials, float(max_norm), norm.data_ptr(), stream))
    torch.autograd.graph.increment_version(grads)
    return norm


# ----------------------------------------------------------------------------------------------
# averaged weights
# ----------------------------------------------------------------------------------------------
def _avg_kind(a, lerp):
    if a.dtype == torch.float32:
        return AVG_LERP if lerp else AVG_COPY32
    return AVG_COPY64           # (anything that is not fp32 or int64 is refused by _AvgTable)


def _model_tensors(model):
    """list(model.parameters()), list(model.buffers()) -- the same tensors in the same order, duplicates removed by identity -- in ONE
    walk of the module tree: the two generator walks cost more host time on this network than everything else in an update."""
    ps, bs, seen = [], [], set()
    for m in model.modules():
        for t in m._parameters.values():
            if t is not None and id(t) not in seen:
                seen.add(id(t))
                ps.append(t)
        for t in m._buffers.values():
            if t is not None and id(t) not in seen:
                seen.add(id(t))
                bs.append(t)
    return ps, bs


def _avg_key(pairs):
    """Everything a table of (kind, dst, src, what) pairs depends on: kinds, storage pointers, sizes and dtypes (a new tensor that the
    allocator put at the old address must be validated again)."""
    return tuple((k, a.data_ptr(), b.data_ptr(), a.numel(), b.numel(), a.dtype, b.dtype) for k, a, b, _ in pairs)


class _AvgTable:
    """Device copies of gssd_avg_item[n] / gssd_sgd_chunk[m] for (kind, dst, src, what) pairs, the ticket word that goes with them, and the
    tensors one launch writes.  Every pair is validated before anything is built: nothing is written when one is refused."""

    def __init__(self, pairs, count):
        rows, self.written, device = [], [], None
        for i, (kind, a, b, what) in enumerate(pairs):
            what = f'{what} (pair {i} of the launch, shape {tuple(a.shape)})'
            dtype = torch.int64 if kind == AVG_COPY64 else torch.float32
            _check_tensor(a, 'the averaged ' + what, device, dtype)
            device = a.device
            _check_tensor(b, 'the source ' + what, device, dtype)
            if a.shape != b.shape:
                raise GssdError(f'gssd.optim: the averaged {what} has shape {tuple(a.shape)}, the source {tuple(b.shape)}')
            if a.numel():
                rows.append((a.data_ptr(), b.data_ptr(), a.numel(), kind, 0))
                self.written.append(a)
        _check_tensor(count, 'n_averaged', device, torch.int64)
        self.written.append(count)
        self.count, self.device = count, count.device
        self.table = _Table(rows, self.device, _AVG_ITEM) if rows else None
        self.ticket = torch.zeros(1, device=self.device, dtype=torch.int32)

    def launch(self, w):
        """One update with weight ``w`` of the source (negative: 1 / (count + 1)); without items only the count moves."""
        if self.table is None:
            self.count.add_(1)
            return
        with torch.cuda.device(self.device):
            check(lib.gssd_avg_update_f32(*self.table.head, w, self.count.data_ptr(), self.ticket.data_ptr(), _stream(self.device)))
        torch.autograd.graph.increment_version(self.written)


class AveragedModel(torch.nn.Module):
    """torch.optim.swa_utils.AveragedModel's layout -- ``module`` (a deep copy of the model), the 0-dim int64 buffer ``n_averaged``,
    ``forward`` delegating to ``module``, the same ``state_dict()`` keys, so checkpoints go either way -- with ``update_parameters`` as
    ONE launch of csrc/optim_avg.hip over all parameters and buffers.

    ``ema_decay`` (extra keyword): None gives torch's default, the equal (SWA) average ``a += (b - a) / (n_averaged + 1)``; a Python
    number in [0, 1] gives the EMA ``a = lerp(a, b, 1 - ema_decay)`` of ``get_ema_multi_avg_fn(ema_decay)``.  It is a plain attribute read
    at every update, so a warm-up schedule sets it per call; a tensor raises NotImplementedError (it would need a host read).  ``avg_fn``
    and ``multi_avg_fn`` must stay None: an arbitrary Python function cannot run inside the kernel -- use ``ema_decay``.  ``device`` must
    be None or the model's device; ``n_averaged`` lives on the model's device (torch leaves it on the CPU unless told otherwise).

    The first update (``n_averaged == 0``) copies the source, later ones average: parameters always, float buffers too with
    ``use_buffers=True``; with ``use_buffers=False`` every buffer is copied from the source (torch's rule).  The count is read and
    incremented ON THE DEVICE by the same launch and never read by the host: ``n_averaged.zero_()`` makes the next update a first one.
    Parameters are paired positionally and buffers positionally, duplicates removed by identity as ``parameters()`` / ``buffers()`` do;
    empty tensors are skipped.

    One deviation from torch: integer buffers (``num_batches_tracked``) are COPIED from the source in every mode.  torch passes them
    through the averaging function with ``use_buffers=True``, in float arithmetic truncated back to int64, which leaves a counter that
    counts nothing.

    Every tensor must be a contiguous fp32 (int64 for the copied counters) device tensor of the source's shape on one device: GssdError
    otherwise, before anything is written.  After the launch every written tensor's version counter is bumped: GssdEngine re-packs its
    weights on that signal."""

    def __init__(self, model, device=None, avg_fn=None, multi_avg_fn=None, use_buffers=False, *, ema_decay=None):
        super().__init__()
        if avg_fn is not None or multi_avg_fn is not None:
            raise NotImplementedError('gssd.optim.AveragedModel: avg_fn / multi_avg_fn cannot run inside the kernel; ema_decay=d gives '
                                      'get_ema_multi_avg_fn(d), ema_decay=None the equal SWA average')
        first = next(itertools.chain(model.parameters(), model.buffers()), None)
        model_device = torch.device('cpu') if first is None else first.device
        if device is not None:
            d = torch.device(device)
            if d.type != model_device.type or (d.index is not None and d.index != model_device.index):
                raise ValueError(f'gssd.optim.AveragedModel: device={device!r}, but the model is on {model_device} (move the model first)')
        self.module = copy.deepcopy(model)
        self.register_buffer('n_averaged', torch.tensor(0, dtype=torch.long, device=model_device))
        self.avg_fn = None
        self.multi_avg_fn = None
        self.use_buffers = use_buffers
        self.ema_decay = ema_decay
        self._weight()
        self._table = None         # (key, _AvgTable)

    def forward(self, *args, **kwargs):
        return self.module(*args, **kwargs)

    def _weight(self):
        """The kernel's ``w``: 1 - ema_decay formed in double (the binding rounds it once), or -1 for the SWA rule."""
        d = self.ema_decay
        if d is None:
            return -1.0
        if isinstance(d, torch.Tensor):
            raise NotImplementedError('gssd.optim.AveragedModel: ema_decay must be a Python number (a tensor would need a host read)')
        if not 0.0 <= d <= 1.0:
            raise ValueError(f'Invalid decay value {d} provided. Please provide a value in [0,1] range.')
        return 1.0 - d

    def _pairs(self, model):
        """(kind, averaged tensor, source tensor, what it is) in launch order: parameters, then buffers."""
        (pa, ba), (pb, bb) = _model_tensors(self.module), _model_tensors(model)
        if len(pa) != len(pb) or len(ba) != len(bb):
            raise GssdError(f'gssd.optim.AveragedModel: the source model has {len(pb)} parameters and {len(bb)} buffers, the averaged '
                            f'one {len(pa)} and {len(ba)}')
        lerp = self.use_buffers
        return [(AVG_LERP, a, b, 'parameter') for a, b in zip(pa, pb)] + [(_avg_kind(a, lerp), a, b, 'buffer') for a, b in zip(ba, bb)]

    def _table_key(self, model):
        return (self.n_averaged.data_ptr(),) + _avg_key(self._pairs(model))

    @torch.no_grad()
    def update_parameters(self, model):
        w = self._weight()
        pairs = self._pairs(model)
        key = (self.n_averaged.data_ptr(),) + _avg_key(pairs)
        if self._table is None or self._table[0] != key:
            self._table = (key, _AvgTable(pairs, self.n_averaged))
        self._table[1].launch(w)


# ----------------------------------------------------------------------------------------------
# gradient accumulation over micro-batches
# ----------------------------------------------------------------------------------------------
class GradAccumulator:
    """The weighted mean (``average=True``, the default) or sum of the gradients of k micro-batches, ONE launch of csrc/optim_accum.hip
    per micro-batch for all parameters:

        acc = gssd.optim.GradAccumulator(net.parameters())      # or optimizer.param_groups
        for x, t in micro_batches:
            ll, lc = criterion(net(x), t); (ll + lc).backward()
            acc.add(weight=criterion.num_pos)                   # acc (+)= w g for every parameter with a gradient; then p.grad = None
        acc.finish()                                            # acc /= sum of the weights;  p.grad = acc
        optimizer.step(); optimizer.zero_grad()

    ``add(weight=None, last=False)`` consumes every parameter whose ``grad`` is not None (a contiguous fp32 device tensor of the
    parameter's shape: GssdError otherwise, before anything is written) and sets it to None afterwards, so that the next ``backward()``
    hands its gradients out directly instead of adding into existing ones tensor by tensor.  ``weight``: None (1.0), a Python number
    (finite, >= 0: ValueError otherwise) or a 1-element fp32 / fp64 tensor on the parameters' device, such as ``MultiBoxLoss.num_pos`` --
    read by the kernel, never by the host.  It acts rounded to fp32: acc = w32 g for a parameter's first gradient of the cycle (which
    ones those are is host bookkeeping; the storage is not read, so nothing is zero-filled), acc = fmaf(w32, g, acc) afterwards.  A
    parameter without a gradient in some micro-batch is not in that launch and is still divided by the full weight sum, torch's
    "sum what arrived, divide by k".  ``last=True`` folds the division into this launch; otherwise ``finish()`` makes one scale-only
    launch.  Both give the same bits: acc * (float)(1 / W), W the fp64 sum of the fp32 weights, kept on the device in ``weight_sum`` (a
    1-element fp64 tensor; it restarts from 0 with every cycle).  ``W == 0`` gives inf / NaN as a division by zero does in torch.

    ``finish()`` sets ``p.grad`` of every parameter seen in the cycle to its accumulator and clears the cycle.  The accumulators are
    16-byte aligned slices of ONE flat fp32 tensor allocated once, the same tensor objects in every cycle: an optimizer's table is built
    once, ``gssd.dist.allreduce_grads`` reduces the flat base in place.  ``launches`` counts the launches so far.  The device tables are
    cached by (gradient pointers, first / later / scale-only pattern); a loop over one plan's gradients builds each of its patterns once.

    Everything runs on the current stream and nothing synchronises.  Launches of one accumulator must follow each other on one
    stream."""
    _TABLES_MAX = 8

    def __init__(self, params, average=True):
        params = list(params)
        if params and isinstance(params[0], dict):
            params = [p for g in params for p in g['params']]
        self.params, ids = [], set()
        for p in params:
            if not isinstance(p, torch.Tensor):
                raise TypeError(f'gssd.optim.GradAccumulator: parameters or param_groups, not {type(p).__name__}')
            if id(p) not in ids:
                ids.add(id(p))
                self.params.append(p)
        if not self.params:
            raise ValueError('gssd.optim.GradAccumulator: got an empty parameter list')
        devices = sorted({str(p.device) for p in self.params})
        if len(devices) > 1:
            raise GssdError(f'gssd.optim.GradAccumulator: the parameters are on {" and ".join(devices)}; make one accumulator per device')
        self.device = self.params[0].device
        self.average = bool(average)
        self.launches = 0
        self.weight_sum = None
        self._numels = [p.numel() for p in self.params]
        self._views = self._ptrs = self._ticket = None
        if self.device.type == 'cuda':
            self._views = flat_views(self.params, self.device)
            self._ptrs = [v.data_ptr() for v in self._views]
            self.weight_sum = torch.zeros(1, device=self.device, dtype=torch.float64)
            self._ticket = torch.zeros(1, device=self.device, dtype=torch.int32)
        self._tables = {}          # key -> (_Table, the accumulators it writes), the few most recent
        self._clear()

    def _clear(self):
        self._seen = [False] * len(self.params)
        self._launched = self._final = False       # this cycle: a launch has run; add(last=True) has closed it

    def _weight(self, weight):
        """(by-value weight, device pointer or None, launch flags)"""
        if weight is None:
            return 1.0, None, 0
        if isinstance(weight, torch.Tensor):
            if weight.layout != torch.strided or not weight.is_cuda or weight.device != self.device or weight.numel() != 1 or \
                    weight.dtype not in (torch.float32, torch.float64):
                raise GssdError(f'gssd.optim.GradAccumulator: a tensor weight must have one fp32 or fp64 element on {self.device} (got '
                                f'{weight.dtype}, {weight.device}, shape {tuple(weight.shape)}); pass a Python number otherwise')
            return 0.0, weight.data_ptr(), ACCUM_W_F32 if weight.dtype == torch.float32 else 0
        if isinstance(weight, (int, float)) and not isinstance(weight, bool):
            w = float(weight)
            if not (w >= 0.0 and w != float('inf')):
                raise ValueError(f'gssd.optim.GradAccumulator: weight={weight!r} must be finite and not negative')
            return w, None, 0
        raise GssdError(f'gssd.optim.GradAccumulator: weight must be None, a Python number or a 1-element device tensor, not '
                        f'{type(weight).__name__}')

    def _table(self, plan, grads, ptrs):
        """The cached (_Table, written accumulators) of a launch plan, by (gradient pointers, plan); the gradients are validated when a
        table is built.  torch itself holds an assigned ``grad`` to the parameter's shape, dtype and device, so a gradient at a known
        address can differ from the validated one in its strides alone: ``ptrs`` carries -1 for one that is not contiguous, which no
        cached key has."""
        key = (tuple(ptrs), tuple(plan))
        hit = self._tables.pop(key, None)
        if hit is None:
            for i, g in enumerate(grads):
                if g is None:
                    continue
                p = self.params[i]
                what = f'the gradient of parameter {i} (shape {tuple(p.shape)})'
                _check_tensor(g, what, self.device)
                if g.shape != p.shape:
                    raise GssdError(f'gssd.optim: {what} has shape {tuple(g.shape)}')
            rows = [(self._ptrs[i], 0 if kind == ACCUM_SCALE else ptrs[i], self._numels[i], int(kind == ACCUM_FIRST), 0) for i, kind in plan]
            hit = (_Table(rows, self.device, _ACCUM_ITEM), [self._views[i] for i, _ in plan])
            while len(self._tables) >= self._TABLES_MAX:
                self._tables.pop(next(iter(self._tables)))
        self._tables[key] = hit
        return hit

    def _launch(self, table, written, w, w_dev, flags):
        if not self._launched:
            flags |= ACCUM_RESET
        with torch.cuda.device(self.device):
            check(lib.gssd_grad_accumulate_f32(*table.head, w, w_dev, flags, self.weight_sum.data_ptr(), self._ticket.data_ptr(),
                                               _stream(self.device)))
        self.launches += 1
        self._launched = True
        torch.autograd.graph.increment_version(written)

    @torch.no_grad()
    def add(self, weight=None, last=False):
        w, w_dev, flags = self._weight(weight)
        if self._final:
            raise GssdError('gssd.optim.GradAccumulator: add(last=True) has closed this cycle; call finish() before the next add()')
        grads = [p.grad for p in self.params]
        has = [g is not None for g in grads]
        if True not in has:
            raise GssdError('gssd.optim.GradAccumulator.add(): no parameter has a gradient; call backward() before add()')
        ptrs = [0 if g is None else g.data_ptr() if g.is_contiguous() else -1 for g in grads]
        if self._ptrs is not None and True in map(int.__eq__, ptrs, self._ptrs):
            for i, (a, b) in enumerate(zip(ptrs, self._ptrs)):
                if a == b and self._numels[i]:
                    raise GssdError(f'gssd.optim.GradAccumulator.add(): the gradient of parameter {i} (shape {tuple(grads[i].shape)}) is '
                                    f'the accumulator itself, so autograd has summed into it; call optimizer.zero_grad() '
                                    f'(set_to_none=True) after the step that follows finish()')
        fin = bool(last) and self.average
        plan = accum_plan(self._numels, has, self._seen, fin)
        table, written = self._table(plan, grads, ptrs)
        if plan:
            self._launch(table, written, w, w_dev, flags | (ACCUM_FINALIZE if fin else 0))
        for i, p in enumerate(self.params):
            if has[i]:
                p.grad = None
                self._seen[i] = True
        self._final = bool(last)

    @torch.no_grad()
    def finish(self):
        if True not in self._seen:
            raise GssdError('gssd.optim.GradAccumulator.finish(): no add() since the last finish(); call add() after every backward()')
        if self.average and not self._final:
            plan = accum_plan(self._numels, [False] * len(self.params), self._seen, True)
            if plan:
                self._launch(*self._table(plan, [None] * len(self.params), [0] * len(self.params)), 0.0, None, ACCUM_FINALIZE)
        for p, v, s in zip(self.params, self._views, self._seen):
            if s:
                p.grad = v
        self._clear()


@torch.no_grad()
def update_bn(loader, model, device=None):
    """torch.optim.swa_utils.update_bn: one pass over ``loader`` that leaves in every BatchNorm of ``model`` the equal average of the
    batches' statistics (``momentum = None`` in torch's words) and ``num_batches_tracked`` at the number of batches.

    torch's own function sets ``momentum = None``, which the launch plans cannot take, and a different constant momentum per batch would
    build and keep a plan per value.  Here every momentum is the constant 1.0 during the pass, so that each train-mode forward leaves
    exactly ITS batch's statistics in ``running_mean`` / ``running_var``; one launch of csrc/optim_avg.hip per batch then folds them into
    fp32 accumulators by the SWA rule, acc += (stat - acc) / k with the count k on the device -- term for term torch's cumulative
    average -- and after the last batch one more launch copies the accumulators back.  Momenta and the training flag are restored on the
    way out, also when a forward raises.  Momentum 1.0 is one more plan key: the pass builds one extra train-mode plan per batch size,
    once; a second pass reuses it."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
    if not bns:
        return
    momenta = [m.momentum for m in bns]
    was_training = model.training
    for m in bns:
        m.reset_running_stats()
    stats = [t for m in bns for t in (m.running_mean, m.running_var) if t is not None]
    try:
        for m in bns:
            m.momentum = 1.0
        model.train()
        fold = unfold = None
        for input in loader:
            if isinstance(input, (list, tuple)):
                input = input[0]
            if device is not None:
                input = input.to(device)
            model(input)
            if not stats:
                continue
            key = _avg_key([(AVG_LERP, t, t, '') for t in stats])
            if fold is None or fold[0] != key:
                # the accumulators: 16-byte aligned slices of one flat tensor; a statistic whose storage moved keeps its accumulator
                if fold is None:
                    accs = flat_views(stats, stats[0].device, zero=True)
                    count = torch.zeros((), device=stats[0].device, dtype=torch.int64)
                fold = (key, _AvgTable([(AVG_LERP, a, t, 'running statistic') for a, t in zip(accs, stats)], count))
                unfold = _AvgTable([(AVG_COPY32, t, a, 'running statistic') for a, t in zip(accs, stats)], torch.zeros_like(count))
            fold[1].launch(-1.0)
        if unfold is not None:
            unfold.launch(-1.0)
    finally:
        for m, mom in zip(bns, momenta):
            m.momentum = mom
        model.train(was_training)
