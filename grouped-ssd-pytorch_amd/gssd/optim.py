"""The optimizer step on the device: ``SGD`` (torch.optim.SGD's update rule and state layout, optionally with the gradient-norm clip
fused in) and a stand-alone ``clip_grad_norm_``, each two launches of csrc/optim.hip over a device table of tensors; ``Adam`` and
``AdamW`` (torch's rule, state names and checkpoints, the same optional clip) on the same tables and csrc/optim_adam.hip; ``LARS`` and
``LAMB`` (csrc/optim_lars.hip), the two with a per-tensor trust ratio that is formed and consumed on the device; and what a
training loop keeps next to its optimizer, ``AveragedModel`` (torch.optim.swa_utils.AveragedModel's layout and checkpoints: an EMA or
the equal SWA average of the weights, every tensor in ONE launch of csrc/optim_avg.hip, the update count on the device) with an
``update_bn`` that works on this engine (torch's sets ``momentum = None``, which the launch plans cannot take); and ``grad_stats`` /
``GradMonitor`` (gssd/grad_stats.py, re-exported here): per-parameter norms, maxima and non-finite counts in two launches.

The reference driver's step (train_lesion_multiphase_v2.py:242-253) then runs on this library's kernels alone:

    optimizer = gssd.optim.SGD(groups, lr=..., momentum=0.9, weight_decay=5e-4, max_grad_norm=max_norm)   # :603-626
    ...
    loss.backward(); optimizer.step()                                                                     # :251-253, clip included

Nothing here reads back to the host.  There is no CPU fallback: a parameter or gradient that is not a contiguous fp32 device tensor
raises GssdError.
"""
import copy
import ctypes as C
import itertools

import numpy as np
import torch

from . import _lib
from ._lib import GssdError, check, lib

CHUNK = lib.gssd_optim_chunk_elems()      # elements per chunk (csrc/optim.hip)

_ITEM = np.dtype([('p', np.uint64), ('g', np.uint64), ('buf', np.uint64), ('n', np.int64), ('group', np.int32), ('flags', np.int32)])
_CHUNK = np.dtype([('off', np.int64), ('item', np.int32), ('reserved', np.int32)])
_ADAM_ITEM = np.dtype([('p', np.uint64), ('g', np.uint64), ('m', np.uint64), ('v', np.uint64), ('vmax', np.uint64), ('n', np.int64),
                       ('group', np.int32), ('flags', np.int32), ('t0', np.int64)])
_AVG_ITEM = np.dtype([('dst', np.uint64), ('src', np.uint64), ('n', np.int64), ('kind', np.int32), ('reserved', np.int32)])
FIRST_STEP = 1
AVG_LERP, AVG_COPY32, AVG_COPY64 = 0, 1, 2     # gssd_avg_item.kind


def build_chunks(numels, chunk=None):
    """The chunk list of a table whose item i has numels[i] elements: (item index, element offset) arrays, item by item, offsets
    0, chunk, 2 chunk, ... below numels[i].  Every element lies in exactly one chunk, no chunk crosses an item, an empty item has none."""
    chunk = chunk or CHUNK
    items, offs = [], []
    for i, n in enumerate(numels):
        k = -(-int(n) // chunk)
        items.append(np.full(k, i, np.int32))
        offs.append(np.arange(k, dtype=np.int64) * chunk)
    if not items:
        return np.zeros(0, np.int32), np.zeros(0, np.int64)
    return np.concatenate(items), np.concatenate(offs)


class _Table:
    """Device copies of gssd_sgd_item[n] (or gssd_adam_item[n]) / gssd_sgd_chunk[m] and the partial-sum workspace that goes with them."""

    def __init__(self, rows, device, dtype=_ITEM):
        # rows: (p ptr, g ptr, buf ptr, numel, group, flags), numel > 0 -- or the fields of ``dtype``, in order
        items = np.zeros(len(rows), dtype)
        for i, r in enumerate(rows):
            items[i] = r
        ci, co = build_chunks(items['n'])
        chunks = np.zeros(len(ci), _CHUNK)
        chunks['item'], chunks['off'] = ci, co
        self.n_chunks = len(ci)
        self.n_partials = lib.gssd_optim_sumsq_blocks(self.n_chunks)
        self.items = torch.from_numpy(items.view(np.uint8).copy()).to(device)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(device)
        self.partials = torch.empty(max(self.n_partials, 1), device=device, dtype=torch.float64)

    def sumsq(self, stream, partials=None):
        partials = self.partials if partials is None else partials
        check(lib.gssd_grad_sumsq_f32(self.items.data_ptr(), self.chunks.data_ptr(), self.n_chunks, partials.data_ptr(), stream))


def _check_tensor(t, what, device=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        d = f'{t.layout}, {t.device}, {t.dtype}, shape {tuple(t.shape)}, strides {t.stride() if t.layout == torch.strided else None}'
        name = 'fp32' if dtype == torch.float32 else str(dtype).replace('torch.', '')
        raise GssdError(f'gssd.optim: {what} must be a contiguous {name} tensor on the MI355X (got {d}); there is no CPU fallback')
    if device is not None and t.device != device:
        raise GssdError(f'gssd.optim: {what} is on {t.device}, the other tensors on {device}')


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class SGD(torch.optim.Optimizer):
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
        for name, v in (('maximize', maximize), ('foreach', foreach), ('differentiable', differentiable), ('fused', fused)):
            if v:
                raise NotImplementedError(f'gssd.optim.SGD: {name}={v!r} is not implemented')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f'Invalid max_grad_norm: {max_grad_norm}')
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=False,
                        foreach=None, differentiable=False, fused=None)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self._table = None         # (_Table, key, updated params, table holds first-step flags, device)
        super().__init__(params, defaults)

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

    def _build(self):
        todo, device = [], None
        for gi, g in enumerate(self.param_groups):
            for name in ('maximize', 'foreach', 'differentiable', 'fused'):
                if g.get(name):
                    raise NotImplementedError(f'gssd.optim.SGD: param_groups[{gi}][{name!r}]={g[name]!r} is not implemented')
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
                buf = None
                if g['momentum'] != 0:
                    buf = self.state[p].get('momentum_buffer') if p in self.state else None
                    if buf is not None:
                        _check_tensor(buf, 'the momentum buffer of ' + what, device)
                        if buf.numel() != p.numel():
                            raise GssdError(f'gssd.optim: the momentum buffer of {what} has {buf.numel()} elements')
                todo.append((gi, p, buf, g['momentum'] != 0))
        # new momentum buffers: 16-byte aligned slices of one flat tensor (the views keep it alive).  All of them on the first step; a
        # gradient or group that appears later gets a flat tensor of its own
        fresh = [p for _, p, buf, mom in todo if mom and buf is None]
        if fresh:
            flat = torch.empty(sum(-(-p.numel() // 4) * 4 for p in fresh), device=device, dtype=torch.float32)
            o = 0
            for p in fresh:
                self.state[p]['momentum_buffer'] = flat[o:o + p.numel()].view(p.shape)
                o += -(-p.numel() // 4) * 4
        fresh = set(fresh)
        rows, params = [], []
        for gi, p, buf, mom in todo:
            first = p in fresh
            if mom and buf is None:
                buf = self.state[p]['momentum_buffer']
            rows.append((p.data_ptr(), p.grad.data_ptr(), 0 if buf is None else buf.data_ptr(), p.numel(), gi, FIRST_STEP if first else 0))
            params.append(p)
        table = _Table(rows, device) if rows else None
        if table is not None and self.max_grad_norm is not None and self.grad_norm is None:
            self.grad_norm = torch.zeros((), device=device, dtype=torch.float32)
        return table, params, bool(fresh), device

    def _hyper(self):
        arr = (_lib.SgdHyper * len(self.param_groups))()
        for h, g in zip(arr, self.param_groups):
            for name in ('lr', 'weight_decay', 'momentum', 'dampening'):
                if isinstance(g[name], torch.Tensor):
                    raise NotImplementedError(f'gssd.optim.SGD: {name} must be a Python number')
            h.lr, h.weight_decay, h.momentum, h.dampening, h.nesterov = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], \
                bool(g['nesterov'])
        return arr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        key = self._table_key() if self._table is not None else None
        if self._table is None or self._table[1] != key:
            table, params, first, device = self._build()
            self._table = (table, self._table_key(), params, first, device)
        table, _, params, first, device = self._table
        if table is None:
            return loss
        hyper = self._hyper()
        clip = self.max_grad_norm is not None
        with torch.cuda.device(device):
            stream = _stream(device)
            if clip:
                table.sumsq(stream)
            check(lib.gssd_sgd_step_f32(table.items.data_ptr(), table.chunks.data_ptr(), table.n_chunks, hyper, len(hyper),
                                        table.partials.data_ptr(), table.n_partials, self.max_grad_norm if clip else -1.0,
                                        self.grad_norm.data_ptr() if clip else None, stream))
        torch.autograd.graph.increment_version(params)
        if first:
            self._table = None       # the table carries first-step flags: the next step builds one without them
        return loss


_ADAM_OFF = ('maximize', 'foreach', 'capturable', 'differentiable', 'fused')
_ADAM_STATE = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')


class Adam(torch.optim.Optimizer):
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
        for what, v in (('maximize', maximize), ('foreach', foreach), ('capturable', capturable), ('differentiable', differentiable),
                        ('fused', fused)):
            if v:
                raise NotImplementedError(f'gssd.optim.{name}: {what}={v!r} is not implemented')
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f'Invalid max_grad_norm: {max_grad_norm}')
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=decoupled_weight_decay)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.grad_norm = None
        self._launches = 0         # steps that reached the device: the kernel's `t`
        self._table = None         # (key, _Table, its gradients' _Table for the norm or None, params, their step counts, device)
        super().__init__(params, defaults)

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

    def _hyper(self):
        name = type(self).__name__
        arr = (_lib.AdamHyper * len(self.param_groups))()
        for gi, (h, g) in enumerate(zip(arr, self.param_groups)):
            for what in _ADAM_OFF:
                if g.get(what):
                    raise NotImplementedError(f'gssd.optim.{name}: param_groups[{gi}][{what!r}]={g[what]!r} is not implemented')
            b1, b2 = g['betas']
            for what, v in (('lr', g['lr']), ('betas', b1), ('betas', b2), ('eps', g['eps']), ('weight_decay', g['weight_decay'])):
                if isinstance(v, torch.Tensor):
                    raise NotImplementedError(f'gssd.optim.{name}: {what} must be a Python number')
            h.lr, h.beta1, h.beta2 = g['lr'], b1, b2
            h.one_minus_beta1, h.one_minus_beta2 = 1.0 - b1, 1.0 - b2            # formed in double, rounded once
            h.eps, h.weight_decay = g['eps'], g['weight_decay']
            h.amsgrad, h.decoupled = bool(g['amsgrad']), bool(g.get('decoupled_weight_decay', False))
        return arr

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
                s = self.state.get(p) or {}
                for k in _ADAM_STATE:
                    if k in s:
                        _check_tensor(s[k], f'{k} of ' + what, device)
                        if s[k].numel() != p.numel():
                            raise GssdError(f'gssd.optim: {k} of {what} has {s[k].numel()} elements')
                if s and not ('step' in s and 'exp_avg' in s and 'exp_avg_sq' in s):
                    raise GssdError(f'gssd.optim: the state of {what} holds {sorted(s)}, not step, exp_avg and exp_avg_sq')
                todo.append((gi, p, bool(g['amsgrad'])))
        # new moments: 16-byte aligned slices of one flat ZERO tensor per kind (the views keep it alive).  All of them on the first step; a
        # gradient or group that appears later gets flat tensors of its own
        pad = lambda p: -(-p.numel() // 4) * 4                                   # noqa: E731
        fresh = {k: [p for _, p, ams in todo if k not in (self.state.get(p) or {}) and (ams or k != 'max_exp_avg_sq')] for k in _ADAM_STATE}
        # the step counts of the table's parameters move into ONE host tensor, state[p]['step'] becoming a 0-dim view of it, so that a
        # step counts them all with one add_ (253 host tensors incremented one by one cost more than the launch).  A count that arrives
        # as a device tensor is read back here, once
        counts = torch.tensor([float(self.state[p]['step']) if self.state.get(p) else 0.0 for _, p, _ in todo], dtype=torch.float32)
        for i, (_, p, _) in enumerate(todo):
            self.state[p]['step'] = counts[i]
        for k in _ADAM_STATE:                                                     # (torch's key order: step, exp_avg, exp_avg_sq, max_...)
            if fresh[k]:
                flat = torch.zeros(sum(pad(p) for p in fresh[k]), device=device, dtype=torch.float32)
                o = 0
                for p in fresh[k]:
                    self.state[p][k] = flat[o:o + p.numel()].view(p.shape)
                    o += pad(p)
        rows, params = [], []
        for i, (gi, p, ams) in enumerate(todo):
            s = self.state[p]
            rows.append((p.data_ptr(), p.grad.data_ptr(), s['exp_avg'].data_ptr(), s['exp_avg_sq'].data_ptr(),
                         s['max_exp_avg_sq'].data_ptr() if ams else 0, p.numel(), gi, 0, self._launches - int(counts[i])))
            params.append(p)
        if not rows:
            return None, None, params, counts, device
        table, norm = _Table(rows, device, _ADAM_ITEM), None
        if self.max_grad_norm is not None:
            norm = _Table([(0, p.grad.data_ptr(), 0, p.numel(), 0, 0) for p in params], device)
            if self.grad_norm is None:
                self.grad_norm = torch.zeros((), device=device, dtype=torch.float32)
        return table, norm, params, counts, device

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hyper = self._hyper()
        if self._table is None or self._table[0] != self._table_key():
            built = self._build()
            self._table = (self._table_key(),) + built
        _, table, norm, params, steps, device = self._table
        if table is None:
            return loss
        clip = norm is not None
        with torch.cuda.device(device):
            stream = _stream(device)
            if clip:
                norm.sumsq(stream)
            check(lib.gssd_adam_step_f32(table.items.data_ptr(), table.chunks.data_ptr(), table.n_chunks, hyper, len(hyper),
                                         self._launches + 1, norm.partials.data_ptr() if clip else None, norm.n_partials if clip else 0,
                                         self.max_grad_norm if clip else -1.0, self.grad_norm.data_ptr() if clip else None, stream))
        self._launches += 1
        steps.add_(1.0)
        torch.autograd.graph.increment_version(params)
        return loss


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
    """What a trust-ratio step needs next to its item / chunk table: the items' chunk prefix, their slots in ``trust_ratio`` (the index
    of the parameter in ``param_groups`` order) and the per-chunk norm records -- all owned by the table they were built for."""

    def __init__(self, table, params, slot_of, device):
        from .grad_stats import item_chunk_prefix
        self.chunk0 = torch.from_numpy(item_chunk_prefix([p.numel() for p in params])).to(device)
        self.slot = torch.tensor([slot_of[id(p)] for p in params], dtype=torch.int32).to(device)
        self.workspace = torch.empty(lib.gssd_lars_workspace_bytes(table.n_chunks) // 8, device=device, dtype=torch.float64)


class _TrustRatio:
    """Shared by LARS and LAMB: the extra group keys (filled from the defaults in new groups and in loaded checkpoints that lack them)
    and ``trust_ratio``."""
    _EXTRA = ()

    def add_param_group(self, param_group):
        self.defaults.update(self._extra_defaults)          # (torch fills a new group from self.defaults)
        super().add_param_group(param_group)

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:                         # a checkpoint of SGD / Adam has none of the extra keys
            for k, v in self._extra_defaults.items():
                g.setdefault(k, v)
        self._table = None

    def _check_extra(self, gi, g):
        name = type(self).__name__
        for k in self._EXTRA:
            if isinstance(g[k], torch.Tensor):
                raise NotImplementedError(f'gssd.optim.{name}: {k} must be a Python number')
            if not g[k] >= 0.0:
                raise ValueError(f'gssd.optim.{name}: param_groups[{gi}][{k!r}]={g[k]!r} is negative')

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
    _EXTRA = ('trust_coefficient', 'eps')

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
        self._ratio = None         # the _Ratios of self._table
        super().__init__(params, lr, momentum, dampening, weight_decay, nesterov, maximize=maximize, foreach=foreach,
                         differentiable=differentiable, fused=fused, max_grad_norm=max_grad_norm)

    def _hyper(self):
        arr = (_lib.LarsHyper * len(self.param_groups))()
        for gi, (h, g) in enumerate(zip(arr, self.param_groups)):
            for name in ('lr', 'weight_decay', 'momentum', 'dampening'):
                if isinstance(g[name], torch.Tensor):
                    raise NotImplementedError(f'gssd.optim.LARS: {name} must be a Python number')
            self._check_extra(gi, g)
            h.lr, h.weight_decay, h.momentum, h.dampening, h.nesterov = g['lr'], g['weight_decay'], g['momentum'], g['dampening'], \
                bool(g['nesterov'])
            h.trust_coefficient, h.eps, h.adapt = g['trust_coefficient'], g['eps'], bool(g['layer_adaptation'])
        return arr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hyper = self._hyper()
        key = self._table_key() if self._table is not None else None
        if self._table is None or self._table[1] != key:
            table, params, first, device = self._build()
            self._ratio = self._ratios(table, params, device)
            self._table = (table, self._table_key(), params, first, device)
        table, _, params, first, device = self._table
        if table is None:
            return loss
        rt = self._ratio
        clip = self.max_grad_norm is not None
        with torch.cuda.device(device):
            check(lib.gssd_lars_step_f32(table.items.data_ptr(), table.chunks.data_ptr(), table.n_chunks, rt.chunk0.data_ptr(),
                                         rt.slot.data_ptr(), hyper, len(hyper), rt.workspace.data_ptr(), table.partials.data_ptr(),
                                         table.n_partials, self.max_grad_norm if clip else -1.0,
                                         self.grad_norm.data_ptr() if clip else None, self.trust_ratio.data_ptr(), _stream(device)))
        self.launches = 1 + step_launches(len(hyper))
        torch.autograd.graph.increment_version(params)
        if first:
            self._table = None       # the table carries first-step flags: the next step builds one without them
        return loss


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
        self._ratio = None         # the _Ratios of self._table
        super().__init__(params, lr, betas, eps, weight_decay, False, foreach=foreach, maximize=maximize, capturable=capturable,
                         differentiable=differentiable, fused=fused, max_grad_norm=max_grad_norm)

    def _hyper(self):
        arr = (_lib.LambHyper * len(self.param_groups))()
        for gi, (h, g) in enumerate(zip(arr, self.param_groups)):
            for what in _ADAM_OFF + ('amsgrad', 'decoupled_weight_decay'):
                if g.get(what):
                    raise NotImplementedError(f'gssd.optim.LAMB: param_groups[{gi}][{what!r}]={g[what]!r} is not implemented')
            b1, b2 = g['betas']
            for what, v in (('lr', g['lr']), ('betas', b1), ('betas', b2), ('eps', g['eps']), ('weight_decay', g['weight_decay'])):
                if isinstance(v, torch.Tensor):
                    raise NotImplementedError(f'gssd.optim.LAMB: {what} must be a Python number')
            h.lr, h.beta1, h.beta2 = g['lr'], b1, b2
            h.one_minus_beta1, h.one_minus_beta2 = 1.0 - b1, 1.0 - b2            # formed in double, rounded once
            h.eps, h.weight_decay = g['eps'], g['weight_decay']
            h.bias_correction, h.adapt = bool(g['bias_correction']), bool(g['layer_adaptation'])
        return arr

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        hyper = self._hyper()
        if self._table is None or self._table[0] != self._table_key():
            built = self._build()
            self._ratio = self._ratios(built[0], built[2], built[4])
            self._table = (self._table_key(),) + built
        _, table, norm, params, steps, device = self._table
        if table is None:
            return loss
        rt = self._ratio
        clip = norm is not None
        with torch.cuda.device(device):
            stream = _stream(device)
            if clip:
                norm.sumsq(stream)
            check(lib.gssd_lamb_step_f32(table.items.data_ptr(), table.chunks.data_ptr(), table.n_chunks, rt.chunk0.data_ptr(),
                                         rt.slot.data_ptr(), hyper, len(hyper), self._launches + 1, rt.workspace.data_ptr(),
                                         norm.partials.data_ptr() if clip else None, norm.n_partials if clip else 0,
                                         self.max_grad_norm if clip else -1.0, self.grad_norm.data_ptr() if clip else None,
                                         self.trust_ratio.data_ptr(), stream))
        self.launches = int(clip) + 1 + step_launches(len(hyper))
        self._launches += 1
        steps.add_(1.0)
        torch.autograd.graph.increment_version(params)
        return loss


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
        check(lib.gssd_grad_scale_clip_f32(table.items.data_ptr(), table.chunks.data_ptr(), table.n_chunks, partials.data_ptr(),
                                           table.n_partials, float(max_norm), norm.data_ptr(), stream))
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
        t = self.table
        with torch.cuda.device(self.device):
            check(lib.gssd_avg_update_f32(t.items.data_ptr(), t.chunks.data_ptr(), t.n_chunks, w, self.count.data_ptr(),
                                          self.ticket.data_ptr(), _stream(self.device)))
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
                    pad = lambda t: -(-t.numel() // 4) * 4                      # noqa: E731
                    flat = torch.zeros(sum(pad(t) for t in stats), device=stats[0].device, dtype=torch.float32)
                    count = torch.zeros((), device=stats[0].device, dtype=torch.int64)
                    accs, o = [], 0
                    for t in stats:
                        accs.append(flat[o:o + t.numel()].view(t.shape))
                        o += pad(t)
                fold = (key, _AvgTable([(AVG_LERP, a, t, 'running statistic') for a, t in zip(accs, stats)], count))
                unfold = _AvgTable([(AVG_COPY32, t, a, 'running statistic') for a, t in zip(accs, stats)], torch.zeros_like(count))
            fold[1].launch(-1.0)
        if unfold is not None:
            unfold.launch(-1.0)
    finally:
        for m, mom in zip(bns, momenta):
            m.momentum = mom
        model.train(was_training)


# per-parameter gradient / weight statistics on the same tables (gssd/grad_stats.py, csrc/optim_stats.hip), re-exported here: they sit
# in the training loop between backward() and step() like everything above
from .grad_stats import GradMonitor, GradStats, grad_stats      # noqa: E402,F401
