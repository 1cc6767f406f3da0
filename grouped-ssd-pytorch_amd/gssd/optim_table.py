"""The device tables of the optimizer kernels (csrc/optim*.hip), shared by gssd/optim.py and gssd/grad_stats.py: the item and chunk
layouts of include/gssd_hip.h, the chunk list and its per-item prefix, their upload, the validation of a tensor the kernels are to
touch, and the aligned slices of one flat tensor that fresh state lives in.  A leaf: it imports nothing of this package but ``_lib``.
"""
import numpy as np
import torch

from ._lib import GssdError, check, lib

CHUNK = lib.gssd_optim_chunk_elems()      # elements per chunk (csrc/optim_util.h)

_ITEM = np.dtype([('p', np.uint64), ('g', np.uint64), ('buf', np.uint64), ('n', np.int64), ('group', np.int32), ('flags', np.int32)])
_CHUNK = np.dtype([('off', np.int64), ('item', np.int32), ('reserved', np.int32)])
_ADAM_ITEM = np.dtype([('p', np.uint64), ('g', np.uint64), ('m', np.uint64), ('v', np.uint64), ('vmax', np.uint64), ('n', np.int64),
                       ('group', np.int32), ('flags', np.int32), ('t0', np.int64)])
_AVG_ITEM = np.dtype([('dst', np.uint64), ('src', np.uint64), ('n', np.int64), ('kind', np.int32), ('reserved', np.int32)])
_ACCUM_ITEM = np.dtype([('dst', np.uint64), ('src', np.uint64), ('n', np.int64), ('flags', np.int32), ('reserved', np.int32)])

ACCUM_ADD, ACCUM_FIRST, ACCUM_SCALE = 0, 1, 2     # what accum_plan() gives an item to do


def accum_plan(numels, has_grad, seen, finalize):
    """The items of one gssd_grad_accumulate_f32 launch, as (parameter index, ACCUM_*) in parameter order, for parameters of ``numels``
    elements of which ``has_grad[i]`` bring a gradient in this micro-batch and ``seen[i]`` brought one earlier in the cycle.  A gradient
    that is the parameter's first of the cycle is ACCUM_FIRST (the accumulator is written, not read), a later one ACCUM_ADD; a parameter
    without one is not in the launch -- unless the launch is the cycle's last (``finalize``) and the parameter was seen: then it is
    ACCUM_SCALE, an item without source that only takes the division.  Empty parameters are skipped."""
    plan = []
    for i, (n, g, s) in enumerate(zip(numels, has_grad, seen)):
        if n == 0:
            continue
        if g:
            plan.append((i, ACCUM_ADD if s else ACCUM_FIRST))
        elif s and finalize:
            plan.append((i, ACCUM_SCALE))
    return plan


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


def item_chunk_prefix(numels, chunk=None):
    """``item_chunk0`` of gssd_tensor_stats_f32 / gssd_lars_step_f32 for a table whose item i has numels[i] elements: int32 [n + 1], item i
    owns the chunks [prefix[i], prefix[i + 1]) of ``build_chunks(numels)``; an empty item owns none, the last entry is the number of chunks."""
    chunk = chunk or CHUNK
    counts = [-(-int(n) // chunk) for n in numels]
    total = sum(counts)
    if total >= 2 ** 31:
        raise GssdError(f'gssd.grad_stats: {total} chunks do not fit the 32-bit chunk index')
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(counts, np.int64))]).astype(np.int32)


class _Table:
    """Device copies of the items (gssd_sgd_item[n], or gssd_adam_item / gssd_avg_item / gssd_accum_item by ``dtype``) and their
    gssd_sgd_chunk[m], the partial-sum workspace that goes with them and, with ``prefix``, the items' chunk prefix ``chunk0`` (int32
    [n + 1])."""

    def __init__(self, rows, device, dtype=_ITEM, prefix=False):
        # rows: the fields of ``dtype``, in order -- (p ptr, g ptr, buf ptr, numel, group, flags) by default
        items = np.zeros(len(rows), dtype)
        for i, r in enumerate(rows):
            items[i] = r
        ci, co = build_chunks(items['n'])
        chunks = np.zeros(len(ci), _CHUNK)
        chunks['item'], chunks['off'] = ci, co
        self.n_items, self.n_chunks = len(rows), len(ci)
        self.n_partials = lib.gssd_optim_sumsq_blocks(self.n_chunks)
        self.items = torch.from_numpy(items.view(np.uint8).copy()).to(device)
        self.chunks = torch.from_numpy(chunks.view(np.uint8).copy()).to(device)
        self.chunk0 = torch.from_numpy(item_chunk_prefix(items['n'])).to(device) if prefix else None
        self.partials = torch.empty(max(self.n_partials, 1), device=device, dtype=torch.float64)
        self.head = (self.items.data_ptr(), self.chunks.data_ptr(), self.n_chunks)     # what every launch over the table begins with

    def sumsq(self, stream, partials=None):
        partials = self.partials if partials is None else partials
        check(lib.gssd_grad_sumsq_f32(*self.head, partials.data_ptr(), stream))


def _check_tensor(t, what, device=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or t.layout != torch.strided or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        d = f'{t.layout}, {t.device}, {t.dtype}, shape {tuple(t.shape)}, strides {t.stride() if t.layout == torch.strided else None}'
        name = 'fp32' if dtype == torch.float32 else str(dtype).replace('torch.', '')
        raise GssdError(f'gssd.optim: {what} must be a contiguous {name} tensor on the MI355X (got {d}); there is no CPU fallback')
    if device is not None and t.device != device:
        raise GssdError(f'gssd.optim: {what} is on {t.device}, the other tensors on {device}')


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def flat_views(like, device, zero=False):
    """One fp32 view per tensor of ``like``, of its shape: 16-byte aligned slices of ONE flat tensor (zeros with ``zero``), which the
    views keep alive."""
    if not like:
        return []
    pad = [-(-t.numel() // 4) * 4 for t in like]
    flat = (torch.zeros if zero else torch.empty)(sum(pad), device=device, dtype=torch.float32)
    views, o = [], 0
    for t, n in zip(like, pad):
        views.append(flat[o:o + t.numel()].view(t.shape))
        o += n
    return views
