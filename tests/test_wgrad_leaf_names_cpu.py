"""CPU half of the fp32 weight gradient's leaf tests (tests/wgrad_leaf_cases.py): every registry row lands on the instance it names, the
GPU rows close over all 18 template instances behind gssd_conv2d_wgrad_f32 and carry every operand form on the families that take it,
and the shape properties the rows are there for hold.  Runs on a host without a GPU: gssd_conv2d_wgrad_kernel_name only walks the dispatch."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wgrad_leaf_cases as R          # noqa: E402

_ADDR = torch.zeros(64, dtype=torch.float32)          # any 16-byte aligned host address: naming dereferences nothing


def kernel_name(kw, dy=None, dw=None, cap=64):
    """(code, what the buffer holds, gssd_last_error) for an ops.make_conv_desc(**kw) descriptor; the buffer starts as '?' * (cap - 1)"""
    from gssd import _lib, ops
    d, _, _ = ops.make_conv_desc(_ADDR, None, None, **R.resolve(kw, lambda key: _ADDR))
    buf = ctypes.create_string_buffer(b'?' * (max(cap, 1) - 1), max(cap, 1))
    dy, dw = (_ADDR.data_ptr() if p is None else p for p in (dy, dw))
    rc = _lib.lib.gssd_conv2d_wgrad_kernel_name(ctypes.byref(d), dy, dw, buf, cap)
    return rc, buf.value.decode(), _lib.lib.gssd_last_error().decode()


@pytest.mark.parametrize('row', R.ROWS, ids=R.row_id)
def test_registry_row_lands_on_its_instance(row):
    _, kw, want, _ = row
    rc, name, err = kernel_name(kw)
    assert (rc, name) == (0, want), err
    from gssd import ops
    d, _, _ = ops.make_conv_desc(_ADDR, None, None, **R.resolve(kw, lambda key: _ADDR))
    assert ops.conv_wgrad_kernel_name(d, _ADDR, _ADDR) == want


def test_registry_ids_features_and_shapes():
    ids = [r[0] for r in R.ROWS]
    assert len(set(ids)) == len(ids) and len(R.INSTANCES) == len(set(R.INSTANCES)) == 18
    for rid, kw, want, feats in R.ROWS:
        assert want in R.INSTANCES and set(feats) <= set(R.FORMS) | set(R.OTHER_FEATURES), rid
        assert kw['H'] != kw['W'], rid                                                      # a swapped extent shows
        assert ('in_scale' in kw) == ('xf' in feats or 'xf window' in feats) or 'name only' in feats, rid
        assert (kw.get('in_ch_off', 0) != 0) == ('window' in feats or 'xf window' in feats), rid
        k, stride, pad, dil, Ho, Wo = R.geometry(kw)
        M, groups = kw['B'] * Ho * Wo, kw['groups']
        assert ('stride' in feats) == (stride != 1) and ('dilation' in feats) == (dil != 1) and ('dilation 6' in feats) == (dil == 6), rid
        if kw.get('in_ch_off'):                                                             # the window sits inside wider rows
            assert kw['in_ch_off'] == 8 and kw['in_stride'] == groups * kw['cin_g'] + 24, rid
        if 'name only' in feats:
            continue
        if want.startswith('conv_wgrad<'):
            # two pixel slices, the second ending in a partial 32-pixel chunk; grouped; out of the slot and patch kernels' reach
            assert 'two slices' in feats and 513 <= M <= 1024 and M % 32 != 0 and groups >= 2 and kw['H'] * kw['W'] < 1444, rid
            assert ('1x1' in feats) == (k == 1) and ('pad 0' in feats) == (k == 3 and pad == 0), rid
            if 'dilation 6' in feats:
                assert (kw['H'], kw['W']) == (17, 19) and pad == 6, rid
        elif want.startswith('conv_thin_wgrad<'):
            assert R.patch_tiles(kw) > 512 and kw['H'] % 8 and kw['W'] % 16, rid           # more tiles than the grid's 512 workgroups, ragged
            assert ('cin 3 of 4' in feats) == (kw['cin_g'] == 4), rid
        elif want.startswith('conv_patch_wgrad<'):
            assert kw['H'] % 8 and kw['W'] % 16, rid
            if 'two tiles per workgroup' in feats:                                          # per_cu <= 4: at most 1024 / groups workgroups a group
                assert R.patch_tiles(kw) > 1024 // groups, rid
            if 'one tile per workgroup' in feats:                                           # per_cu >= 1: at least 256 / groups
                assert R.patch_tiles(kw) <= 256 // groups, rid
        else:
            assert M >= 4096 and M % 32 != 0 and groups == 1 and 'in_scale' not in kw, rid  # a partial last chunk of the reduction
    # the four generic tiles: ragged in rows and in columns
    for name, (bmw, bnw) in {'conv_wgrad<16x256>': (16, 256), 'conv_wgrad<32x128>': (32, 128), 'conv_wgrad<64x256>': (64, 256),
                             'conv_wgrad<128x128>': (128, 128)}.items():
        for rid, kw, want, feats in R.GPU_ROWS:
            if want == name:
                k = R.geometry(kw)[0]
                assert (kw['Cout'] // kw['groups']) % bmw and (k * k * kw['cin_g']) % bnw, rid
    assert any(kw['B'] * R.geometry(kw)[4] * R.geometry(kw)[5] >= 4096 and w == 'conv_wgrad<128x128>' for _, kw, w, f in R.ROWS if 'name only' in f)


def test_gpu_rows_close_over_instances_and_forms():
    assert not R.uncovered(R.ROWS)
    for n in R.INSTANCES:                              # dropping the rows of any one name opens the closure again
        assert R.uncovered([r for r in R.ROWS if r[2] != n]) == {n}
    assert R.uncovered([r for r in R.ROWS if 'name only' in r[3]]) == set(R.INSTANCES)          # name-only rows cover nothing
    for form, groups in R.FORMS.items():
        on = {r[2] for r in R.GPU_ROWS if form in r[3]}
        for grp in groups:                             # every family that accepts the form runs it ...
            assert on & set(grp), (form, grp)
        assert on <= {n for grp in groups for n in grp}, (form, on)          # ... and no other claims to


def test_refused_arguments_and_short_buffers():
    """What the launch refuses the query refuses with the launch's text; a short buffer is an error, never a truncated name.  GSSD_EINVAL,
    gssd_last_error set, the buffer left empty."""
    from gssd import _lib
    kw = R.GPU_ROWS[0][1]
    want = R.GPU_ROWS[0][2]
    n = len(want) + 1
    assert kernel_name(kw, cap=n)[:2] == (0, want)
    for cap in (n - 1, 8, 1):
        rc, name, err = kernel_name(kw, cap=cap)
        assert (rc, name) == (-1, '') and f'needs {n} bytes' in err, (cap, rc, name, err)
    long = 'conv_patch_wgrad<16,32>/plain'
    patch_kw = next(r[1] for r in R.ROWS if r[2] == long)
    assert kernel_name(patch_kw, cap=len(long))[:2] == (-1, '') and kernel_name(patch_kw, cap=len(long) + 1)[:2] == (0, long)
    # refused descriptors: the buffer comes back empty, the error names the failed condition
    for bad, text in ((dict(kw, cin_g=6, in_stride=12), 'cin_g % 4 == 0'), (dict(kw, Cout=26), '% 4 == 0'), (dict(kw, in_ch_off=2), 'in_ch_off % 4 == 0'),
                      (dict(kw, in_scale=R.P), 'in_scale == nullptr'), (dict(kw, m_per_image=True), 'm_per_image')):
        rc, name, err = kernel_name(bad)
        assert (rc, name) == (-1, '') and 'invalid argument' in err and text in err, (bad, rc, name, err)
    rc, name, err = kernel_name(kw, dy=_ADDR.data_ptr() + 4)                 # dy not 16-byte aligned
    assert (rc, name) == (-1, '') and 'dy % 16' in err, (rc, name, err)
    assert kernel_name(kw, dy=0)[:2] == (-1, '') and kernel_name(kw, dw=0)[:2] == (-1, '')
    d = _lib.ConvDesc()
    assert _lib.lib.gssd_conv2d_wgrad_kernel_name(ctypes.byref(d), _ADDR.data_ptr(), _ADDR.data_ptr(), None, 64) == -1
    assert _lib.lib.gssd_conv2d_wgrad_kernel_name(None, _ADDR.data_ptr(), _ADDR.data_ptr(), ctypes.create_string_buffer(8), 8) == -1
    # the launch itself answers the same for the same arguments, before it touches a device
    from gssd import ops
    d, _, _ = ops.make_conv_desc(_ADDR, None, None, **dict(kw, cin_g=6, in_stride=12))
    assert _lib.lib.gssd_conv2d_wgrad_f32(ctypes.byref(d), _ADDR.data_ptr(), _ADDR.data_ptr(), None) == -1 and b'cin_g % 4 == 0' in _lib.lib.gssd_last_error()
    # csrc/wgrad_slot.hip stores 16-byte quads: a packed gradient that is not 16-byte aligned stays on the generic kernel
    slot_kw, slot, generic = R.SLOT_SWITCH
    assert kernel_name(slot_kw)[:2] == (0, slot) and kernel_name(slot_kw, dw=_ADDR.data_ptr() + 4)[:2] == (0, generic)


@pytest.mark.parametrize('env,which', [({}, 1), ({'GSSD_NO_WGRAD_SLOT': '1'}, 2), ({'GSSD_NO_GEMM_SLOT': '1'}, 2)])
def test_name_follows_the_slot_switches(env, which):
    """The ablation switches are read once per process: a child each."""
    kw = R.SLOT_SWITCH[0]
    src = ('import torch\nfrom gssd import ops\na = torch.zeros(64)\n'
           f'd, _, _ = ops.make_conv_desc(a, None, None, **{kw!r})\nprint(ops.conv_wgrad_kernel_name(d, a, a))\n')
    base = {k: v for k, v in os.environ.items() if k not in ('GSSD_NO_WGRAD_SLOT', 'GSSD_NO_GEMM_SLOT')}
    r = subprocess.run([sys.executable, '-c', src], capture_output=True, text=True, timeout=120,
                       env=dict(base, PYTHONPATH=os.pathsep.join(sys.path), **env))
    assert r.returncode == 0 and r.stdout.strip() == R.SLOT_SWITCH[which], (r.stdout, r.stderr[-2000:])
