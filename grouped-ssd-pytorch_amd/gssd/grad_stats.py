"""Per-parameter statistics of the gradients (and weights) on the device: ``grad_stats`` leaves, for every tensor it is given, the
2-norm, the largest finite magnitude and the number of non-finite elements of its gradient and of the tensor itself in one fp64 table
``[N + 1, 8]`` (the last row: the totals), in two launches of csrc/optim_stats.hip over the optimizers' item / chunk tables.  Nothing is
read back: a training loop copies the table once per logging interval (``GradStats.to_host``, ``GradMonitor.flush``), not one norm per
tensor per step, and the table says WHICH tensor went non-finite.

The reference drivers' per-iteration ``check_grad_norm(net)`` (train_lesion_multiphase_v2.py:16, :250) is ``utils/check_grad_norm.py``
of this tree: the same name and signature on ``grad_stats`` and one read of the total.

There is no CPU fallback: a tensor or gradient that is not a contiguous fp32 device tensor raises GssdError.
"""
import collections

import numpy as np
import torch

from ._lib import GssdError, check, lib
from .optim_table import _Table, _check_tensor, _stream, item_chunk_prefix      # noqa: F401  (item_chunk_prefix: importable from here)

COLUMNS = ('grad_sumsq', 'grad_norm', 'grad_absmax', 'grad_nonfinite', 'param_sumsq', 'param_norm', 'param_absmax', 'param_nonfinite')
Row = collections.namedtuple('Row', COLUMNS)      # one row of the table on the host (GradStats.to_host)


def monitor_order(n, flushed, history):
    """Slot arithmetic of GradMonitor, on plain integers: with ``n`` records made so far, ``flushed`` of them already handed out (or
    overwritten and counted as such) and a ring of ``history`` slots, record s lives in slot s % history and a flush hands out
    (steps, slots) of the records max(flushed, n - history) .. n - 1, oldest first."""
    first = max(flushed, n - history, 0)
    steps = list(range(first, n))
    return steps, [s % history for s in steps]


def _entries(parameters):
    """[(name, tensor)] in iteration order from a Module (named_parameters()), an iterable of (name, tensor) or one of tensors."""
    if isinstance(parameters, torch.nn.Module):
        return list(parameters.named_parameters())
    if isinstance(parameters, torch.Tensor):
        return [('0', parameters)]
    out = []
    for i, e in enumerate(parameters):
        if isinstance(e, torch.Tensor):
            out.append((str(i), e))
        elif isinstance(e, (tuple, list)) and len(e) == 2 and isinstance(e[0], str) and isinstance(e[1], torch.Tensor):
            out.append((e[0], e[1]))
        else:
            raise TypeError(f'gssd.grad_stats: entry {i} is {type(e).__name__}, not a tensor or a (name, tensor) pair')
    return out


class _StatsTable:
    """The _Table (items, chunks, chunk prefix) of (name, tensor) entries, the 32 bytes of chunk records per chunk and the table's own
    output buffer.  Every tensor is validated before anything is built."""

    def __init__(self, entries, params):
        rows, device = [], None
        for i, (name, t) in enumerate(entries):
            what = f'parameter {name!r} (row {i}, shape {tuple(t.shape)})'
            _check_tensor(t.detach(), what, device)
            device = t.device
            g = t.grad
            if g is not None:
                _check_tensor(g, 'the gradient of ' + what, device)
                if g.numel() != t.numel():
                    raise GssdError(f'gssd.grad_stats: the gradient of {what} has shape {tuple(g.shape)}')
            rows.append((t.data_ptr() if params else 0, 0 if g is None else g.data_ptr(), 0, t.numel(), 0, 0))
        self.table = t = _Table(rows, device, prefix=True)
        self.device, self.n_items, self.n_chunks = device, t.n_items, t.n_chunks
        n_ws = lib.gssd_tensor_stats_workspace_bytes(self.n_chunks)
        self.workspace = torch.empty(n_ws // 8, device=device, dtype=torch.float64) if n_ws else None
        self.out = torch.zeros(self.n_items + 1, len(COLUMNS), device=device, dtype=torch.float64)

    def launch(self, out):
        t = self.table
        with torch.cuda.device(self.device):
            check(lib.gssd_tensor_stats_f32(t.items.data_ptr(), self.n_items, t.chunks.data_ptr() if self.n_chunks else None,
                                            self.n_chunks, t.chunk0.data_ptr(), self.workspace.data_ptr() if self.n_chunks else None,
                                            out.data_ptr(), _stream(self.device)))


# (params, ((data_ptr, grad data_ptr, numel, grad dtype), ...)) -> _StatsTable, the few most recent, as optim.clip_grad_norm_ keeps its
# tables: building one costs host-to-device copies, and a training loop asks about the same tensors every step.  A table owns its
# chunk records and its output buffer, so calls that share one must follow each other on one stream.
_TABLES = {}
_TABLES_MAX = 4


class GradStats:
    """What ``grad_stats`` returns.  ``names``: the rows' names; ``without_grad``: the names whose ``.grad`` was None (their gradient
    columns are zero); ``table``: the fp64 device tensor [N + 1, 8], columns ``COLUMNS``, last row the totals (sum / sqrt / max / sum).
    The attributes below are VIEWS of the table, which the next ``grad_stats`` call on the same tensors overwrites unless ``out=`` was
    given; none of them reads anything back.

    ``sumsq`` and ``norm`` follow IEEE: an inf among the elements makes them inf, a NaN makes them NaN.  ``absmax`` is the largest
    magnitude among the FINITE elements (0 if there is none) and ``nonfinite`` counts the others, so a row that went bad still says how
    bad."""

    def __init__(self, names, without_grad, table):
        self.names, self.without_grad, self.table = names, without_grad, table

    grad_norm = property(lambda self: self.table[:-1, 1])
    grad_absmax = property(lambda self: self.table[:-1, 2])
    grad_nonfinite = property(lambda self: self.table[:-1, 3])
    param_norm = property(lambda self: self.table[:-1, 5])
    param_absmax = property(lambda self: self.table[:-1, 6])
    param_nonfinite = property(lambda self: self.table[:-1, 7])
    total_norm = property(lambda self: self.table[-1, 1])
    total_nonfinite = property(lambda self: self.table[-1, 3])

    def to_host(self):
        """{name: Row} in row order plus ``'total'``, from ONE device-to-host copy of the table."""
        t = self.table.cpu().numpy()
        out = {n: Row(*(float(v) for v in r)) for n, r in zip(self.names, t)}
        out['total'] = Row(*(float(v) for v in t[-1]))
        return out

    def worst(self, k=5):
        """[(name, Row)]: the ``k`` rows with the most non-finite gradient elements, ties broken by the largest ``grad_absmax`` (then by
        row order); works on one host copy of the table."""
        t = self.table.cpu().numpy()[:-1]
        order = sorted(range(len(self.names)), key=lambda i: (-t[i, 3], -t[i, 2], i))
        return [(self.names[i], Row(*(float(v) for v in t[i]))) for i in order[:max(int(k), 0)]]


@torch.no_grad()
def grad_stats(parameters, params=True, out=None):
    """The statistics of ``parameters``: an ``nn.Module`` (rows named by ``named_parameters()``), an iterable of ``(name, tensor)`` or an
    iterable of tensors (names '0', '1', ...).  Every tensor given gets a row, in iteration order, empty ones included.  ``params=False``
    leaves the tensors themselves unread (their columns are zero); a tensor whose ``.grad`` is None gets zero gradient columns and is
    listed in ``GradStats.without_grad``.

    ``out``: an fp64 device tensor [N + 1, 8] to write into.  Without it the result lives in a buffer that belongs to the cached device
    table of these tensors and that the NEXT call on them overwrites (like ``optimizer.grad_norm``); clone what must outlive it.

    The device table is cached under the tensors' and gradients' storage pointers and sizes and rebuilt (one validation, four small
    uploads) when they change.  With the table built a call is two launches and reads nothing back."""
    entries = _entries(parameters)
    if not entries:
        raise GssdError('gssd.grad_stats: no tensor given (and so no device to put the table on)')
    names, without, key = [], [], []
    for name, t in entries:
        g = t.grad
        names.append(name)
        if g is None:
            without.append(name)
            key.append((t.data_ptr(), 0, t.numel()))
        else:
            key.append((t.data_ptr(), g.data_ptr(), t.numel(), g.dtype))
    key = (bool(params), tuple(key))
    table = _TABLES.pop(key, None)
    if table is None:
        table = _StatsTable(entries, bool(params))
        while len(_TABLES) >= _TABLES_MAX:
            _TABLES.pop(next(iter(_TABLES)))
    _TABLES[key] = table
    if out is None:
        out = table.out
    else:
        _check_tensor(out, 'out', table.device, torch.float64)
        if tuple(out.shape) != (table.n_items + 1, len(COLUMNS)):
            raise GssdError(f'gssd.grad_stats: out has shape {tuple(out.shape)}, the table {(table.n_items + 1, len(COLUMNS))}')
    table.launch(out)
    return GradStats(names, without, out)


class GradMonitor:
    """A ring of the last ``history`` tables of ``parameters`` on the device: ``record()`` after every ``loss.backward()`` is two launches
    and no read, ``flush()`` once per logging interval is one copy.

    ``parameters`` is what ``grad_stats`` takes; a Module is walked again at every record (its gradients may move), any other iterable
    is listed once, here.  The number of rows is fixed at construction."""

    def __init__(self, parameters, history=100, params=True):
        if int(history) < 1:
            raise ValueError(f'Invalid history: {history}')
        self._parameters = parameters if isinstance(parameters, torch.nn.Module) else _entries(parameters)
        entries = _entries(self._parameters)
        if not entries:
            raise GssdError('gssd.grad_stats.GradMonitor: no tensor given')
        self.names = [n for n, _ in entries]
        self.history, self.params = int(history), bool(params)
        self.buffer = None         # [history, N + 1, 8] fp64, on the device of the first record
        self.n = 0                 # records so far
        self._flushed = 0          # records already handed out

    def record(self):
        """``grad_stats`` into slot n % history of the ring (the slot is a pointer offset chosen on the host); returns its GradStats."""
        if self.buffer is None:
            device = _entries(self._parameters)[0][1].device
            self.buffer = torch.zeros(self.history, len(self.names) + 1, len(COLUMNS), device=device, dtype=torch.float64)
        stats = grad_stats(self._parameters, self.params, out=self.buffer[self.n % self.history])
        self.n += 1
        return stats

    def flush(self):
        """(steps int64 [k], tables float64 [k, N + 1, 8]) of the records since the last flush, oldest first, at most ``history`` of them
        (older ones were overwritten), from ONE device-to-host copy; the next flush starts behind them."""
        steps, slots = monitor_order(self.n, self._flushed, self.history)
        self._flushed = self.n
        if not steps:
            return np.zeros(0, np.int64), np.zeros((0, len(self.names) + 1, len(COLUMNS)), np.float64)
        if slots == list(range(slots[0], slots[0] + len(slots))):
            tables = self.buffer[slots[0]:slots[0] + len(slots)].cpu().numpy()       # the ring has not wrapped inside the range
        else:
            tables = self.buffer.cpu().numpy()[slots]
        return np.asarray(steps, np.int64), tables
