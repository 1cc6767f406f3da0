"""Host side of gssd.optim.grad_stats / GradMonitor / utils.check_grad_norm that needs no GPU: the ABI wiring of the two
gssd_tensor_stats_* entry points, the refusals decided before anything touches a device, the chunk prefix the fold kernel walks, the
ring arithmetic of GradMonitor and the drivers' import."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gssd_hip.h')


def test_abi_carries_the_stats_entry_points():
    from gssd import _lib
    lib = _lib.lib
    hdr = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    ws = re.search(r'\blong\s+long\s+gssd_tensor_stats_workspace_bytes\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S)
    run = re.search(r'\bint\s+gssd_tensor_stats_f32\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S)
    assert ws and run
    n_ws, n_run = len(ws.group(1).split(',')), len(run.group(1).split(','))
    assert (n_ws, n_run) == (1, 8) and re.search(r'gssd_stream_t\s+\w+\s*$', run.group(1))
    assert len(_lib.SIGNATURES['gssd_tensor_stats_workspace_bytes'][1]) == n_ws
    assert len(_lib.SIGNATURES['gssd_tensor_stats_f32'][1]) == n_run
    assert _lib.SIGNATURES['gssd_tensor_stats_workspace_bytes'][0] is ctypes.c_longlong
    # both are in the library (the binding refuses to load without them) ...
    assert lib.gssd_tensor_stats_workspace_bytes(0) == 0 and lib.gssd_tensor_stats_workspace_bytes(1) == 32
    assert lib.gssd_tensor_stats_workspace_bytes(6151) == 32 * 6151 and lib.gssd_tensor_stats_workspace_bytes(2 ** 27) == 2 ** 32
    # ... and the launch is in the plan runner's table with the binding's argument count (the stream is not counted)
    i = lib.gssd_plan_fn_index(b'gssd_tensor_stats_f32')
    assert i >= 0 and lib.gssd_plan_fn_nargs(i) == n_run - 1 == 7
    assert lib.gssd_plan_fn_index(b'gssd_tensor_stats_workspace_bytes') == -1          # no stream: not a plan op
    assert lib.gssd_abi_version() == 8


def test_refusals_touch_no_device():
    from gssd import _lib
    f = _lib.lib.gssd_tensor_stats_f32
    one = ctypes.c_void_p(16)                  # never dereferenced: every call below is refused
    for args in ((None, 1, one, 1, one, one, one),         # no item table
                 (one, 1, None, 1, one, one, one),         # chunks to run and no chunk list
                 (one, 1, one, 1, None, one, one),         # no prefix
                 (one, 1, one, 1, one, None, one),         # chunks to run and nowhere to leave their records
                 (one, 1, one, 1, one, one, None),         # no output
                 (one, 0, one, 1, one, one, one),          # no rows
                 (one, -3, one, 1, one, one, one),
                 (one, 1, one, -1, one, one, one),         # a negative chunk count
                 (one, 1, None, 0, None, None, one),       # without chunks the list and the records may be null, the prefix may not
                 (one, 1, None, 0, one, None, None)):
        assert f(*args, None) == -1 and b'invalid argument' in _lib.lib.gssd_last_error(), args


def test_chunk_prefix_matches_the_chunk_list():
    from gssd import grad_stats as gs, optim
    assert optim.CHUNK == 4096
    numels = [1, 0, 4095, 4096, 4097, 0, 8195]
    items, offs = optim.build_chunks(numels)
    prefix = gs.item_chunk_prefix(numels)
    assert prefix.dtype == np.int32 and prefix.shape == (len(numels) + 1,)
    assert prefix.tolist() == [0, 1, 1, 2, 3, 5, 5, 8] and prefix[-1] == len(items) == len(offs)
    for i, n in enumerate(numels):
        own = np.arange(prefix[i], prefix[i + 1])
        assert (items[own] == i).all() and np.array_equal(np.flatnonzero(items == i), own)
        assert offs[own].tolist() == list(range(0, n, optim.CHUNK))
        assert (len(own) == 0) == (n == 0)
    # no tensors of any size, and only empty ones
    assert gs.item_chunk_prefix([]).tolist() == [0] and gs.item_chunk_prefix([0, 0]).tolist() == [0, 0, 0]
    assert gs.item_chunk_prefix([5, 9], chunk=4).tolist() == [0, 2, 5]
    # the re-exports are the same objects
    assert optim.grad_stats is gs.grad_stats and optim.GradStats is gs.GradStats and optim.GradMonitor is gs.GradMonitor
    assert gs.COLUMNS == ('grad_sumsq', 'grad_norm', 'grad_absmax', 'grad_nonfinite',
                          'param_sumsq', 'param_norm', 'param_absmax', 'param_nonfinite') == gs.Row._fields


def test_monitor_ring_order():
    from gssd.grad_stats import monitor_order
    assert monitor_order(0, 0, 3) == ([], [])
    assert monitor_order(2, 0, 3) == ([0, 1], [0, 1])                       # fewer than history
    assert monitor_order(3, 0, 3) == ([0, 1, 2], [0, 1, 2])                 # exactly history
    assert monitor_order(5, 0, 3) == ([2, 3, 4], [2, 0, 1])                 # wrapped once: the two oldest are gone
    assert monitor_order(8, 0, 3) == ([5, 6, 7], [2, 0, 1])                 # wrapped twice
    assert monitor_order(9, 0, 3) == ([6, 7, 8], [0, 1, 2])
    assert monitor_order(5, 5, 3) == ([], [])                               # a second flush
    assert monitor_order(6, 5, 3) == ([5], [2])                             # a flush, then further records
    assert monitor_order(7, 5, 3) == ([5, 6], [2, 0])
    assert monitor_order(12, 5, 3) == ([9, 10, 11], [0, 1, 2])              # ... more of them than the ring holds
    assert monitor_order(4, 0, 1) == ([3], [0])
    for n in range(0, 40):
        for flushed in range(0, n + 1):
            for history in (1, 2, 7, 100):
                steps, slots = monitor_order(n, flushed, history)
                assert steps == list(range(max(flushed, n - history), n)) and slots == [s % history for s in steps]
                assert len(set(slots)) == len(slots) <= history


def test_monitor_and_stats_host_logic():
    """What is decided on the host before a device is needed: the entry forms, a bad history, and the refusal of CPU tensors."""
    import torch
    from gssd import grad_stats as gs
    from gssd._lib import GssdError
    lin = torch.nn.Linear(3, 2)
    assert [n for n, _ in gs._entries(lin)] == ['weight', 'bias']
    assert [n for n, _ in gs._entries(lin.parameters())] == ['0', '1']
    assert [n for n, _ in gs._entries([('w', lin.weight), ('b', lin.bias)])] == ['w', 'b']
    assert [n for n, _ in gs._entries(lin.weight)] == ['0']
    with pytest.raises(TypeError):
        gs._entries([('w', 3.0)])
    with pytest.raises(ValueError):
        gs.GradMonitor(lin, history=0)
    mon = gs.GradMonitor(lin, history=4)
    assert mon.names == ['weight', 'bias'] and mon.n == 0
    steps, tables = mon.flush()
    assert steps.dtype == np.int64 and steps.shape == (0,) and tables.shape == (0, 3, 8)
    with pytest.raises(GssdError, match='no CPU fallback'):
        gs.grad_stats(lin)
    with pytest.raises(GssdError):
        gs.grad_stats([])


def test_drivers_import_works():
    """train_lesion_multiphase_v2.py:16 with the drop-in first on sys.path."""
    from utils.check_grad_norm import check_grad_norm
    params = list(inspect.signature(check_grad_norm).parameters.values())
    assert len(params) == 1 and params[0].kind in (inspect.Parameter.POSITIONAL_ONLY, inspect.Parameter.POSITIONAL_OR_KEYWORD)
    assert params[0].default is inspect.Parameter.empty
