"""CPU half of the generic conv kernels' leaf tests (tests/conv_leaf_cases.py): every registry row lands on the instance it names, and
the registry plus the written map of specialised kernels closes over every kernel name a production step launches
(tests/data/conv_names_parent.json).  Runs on a host without a GPU: gssd_conv2d_kernel_name only walks the dispatch."""
import ctypes
import json
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_leaf_cases as R          # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERIC = ('conv_igemm<', 'conv_bf16<', 'gemm_slot<')
_ADDR = torch.zeros(64, dtype=torch.float32)          # any 16-byte aligned host address: naming dereferences nothing
# the existing kernel-level tests that carry the expected instance name in their cases and assert it before the launch
PINNED = {'test_conv_igemm', 'test_conv_winograd', 'test_conv_winograd_pooled_epilogue', 'test_conv_bf16', 'test_conv_flat_bf16'}


def kernel_name(bf16, kw):
    from gssd import _lib, ops
    d, _, _ = ops.make_conv_desc(_ADDR, _ADDR, _ADDR, **R.resolve(kw, lambda key: _ADDR))
    buf = ctypes.create_string_buffer(64)
    rc = _lib.lib.gssd_conv2d_kernel_name(ctypes.byref(d), int(bf16), buf, 64)
    return rc, buf.value.decode(), _lib.lib.gssd_last_error().decode()


def fixture_names():
    with open(os.path.join(ROOT, 'tests', 'data', 'conv_names_parent.json')) as f:
        return {row[1] for rows in json.load(f).values() for row in rows}


def uncovered(rows, elsewhere):
    """fixture names that neither a registry row expects nor the map of specialised kernels lists"""
    return fixture_names() - {r[3] for r in rows} - set(elsewhere)


@pytest.mark.parametrize('row', R.ROWS, ids=R.row_id)
def test_registry_row_lands_on_its_instance(row):
    _, bf16, kw, want, _ = row
    rc, name, err = kernel_name(bf16, kw)
    assert (rc, name) == (0, want), err


def test_registry_ids_and_features():
    ids = [r[0] for r in R.ROWS]
    assert len(set(ids)) == len(ids)
    assert all(r[1] == r[3].startswith('conv_bf16<') for r in R.ROWS)
    assert all(set(r[4]) <= set(R.FEATURES) for r in R.ROWS)
    f32 = [r for r in R.ROWS if not r[1]]
    for feat in R.FEATURES:                            # every epilogue / operand form is on some fp32 row ...
        assert any(feat in r[4] for r in f32), feat
    for feat in R.THREE_STAGE_FEATURES:                # ... and where the kernel allows it on a three-stage tile (another K loop)
        assert any(feat in r[4] and r[3].endswith(tuple(t + '>' for t in R.THREE_STAGE_TILES)) for r in f32), feat
    for fam in ('conv_igemm', 'conv_bf16'):            # all six tiles of both kernels, from a row that asks for the tile
        tiles = {r[3] for r in R.ROWS if 'tile' in r[4] and r[3].startswith(fam)}
        assert tiles == {f'{fam}<{t}>' for t in ('128x128', '128x64', '128x32', '128x16', '64x64', '32x64')}, tiles


def test_fixture_names_are_closed_over():
    """Every kernel a production step launches is run at kernel level: the generic ones by a registry row that expects that name, the
    specialised ones by the existing test the map names."""
    names = fixture_names()
    generic = {n for n in names if n.startswith(GENERIC)}
    assert generic and generic <= {r[3] for r in R.ROWS}, generic - {r[3] for r in R.ROWS}
    assert not uncovered(R.ROWS, R.COVERED_ELSEWHERE)
    # dropping the rows of any generic name opens the closure again
    for n in sorted(generic):
        assert n in uncovered([r for r in R.ROWS if r[3] != n], R.COVERED_ELSEWHERE), n
    # the map speaks of the specialised families only, and of names the fixture has
    for n, test_id in R.COVERED_ELSEWHERE.items():
        assert n in names and not n.startswith(GENERIC) and n.split('<')[0].startswith(R.SPECIAL_FAMILIES), n
        path, fn = test_id.split('::')
        src = open(os.path.join(ROOT, path)).read()
        assert re.search(rf'^def {re.escape(fn)}\(', src, flags=re.M), test_id
        if fn in PINNED:
            assert f"'{n}'" in src, (n, test_id)       # the test asserts this very name before it launches

