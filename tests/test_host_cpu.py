"""CPU-side checks of the product: the C-ABI library loads and exports every symbol include/gssd_hip.h
declares (no compute calls: there is no GPU here), and the host logic (PriorBox, module tree / state-dict
keys, pooling arithmetic, target packing) matches the reference-generated fixtures."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_exports_match_header():
    from gssd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read()
    declared = set(re.findall(r'\b(gssd_[a-z0-9_]+)\s*\(', hdr))
    declared -= {'gssd_conv_desc', 'gssd_sn_item', 'gssd_stream_t', 'gssd_plan_op'}
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert _lib.lib.gssd_abi_version() == 8 and _lib.lib.gssd_build_arch() == b'gfx950'
    # struct layout agrees with the header's field order / C packing rules
    assert ctypes.sizeof(_lib.ConvDesc) == 17 * 8 + 27 * 4 + 4 + 6 * 8 == _lib.lib.gssd_conv_desc_size()   # (17 pointers since wgt_patch; 27 ints + 4 bytes of padding)
    assert ctypes.sizeof(_lib.SnItem) == 4 * 8 + 2 * 4


def test_plan_runner_table_and_encoding():
    """csrc/plan_run.hip: the runner's function table is exactly the header's `int gssd_*(..., gssd_stream_t stream)`
    entry points, each with the parameter count of the binding; argument words are encoded as the header says; bad ops are refused with
    their index before anything touches a device."""
    import struct
    from gssd import _lib, planrun
    lib = _lib.lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read(), flags=re.S)
    want = {}
    for name, args in re.findall(r'\bint\s+(gssd_\w+)\s*\(([^;{]*?)\)\s*;', hdr, flags=re.S):
        a = [x.strip() for x in args.replace('\n', ' ').split(',')]
        if re.search(r'gssd_stream_t\s+\w+$', a[-1]):
            want[name] = len(a) - 1
    have = {lib.gssd_plan_fn_name(i).decode(): lib.gssd_plan_fn_nargs(i) for i in range(lib.gssd_plan_fn_count())}
    assert have == want and len(have) >= 85
    for name, n in have.items():
        assert len(_lib.SIGNATURES[name][1]) == n + 1 and planrun.fn_info(getattr(lib, name))[0] == lib.gssd_plan_fn_index(name.encode())
    assert lib.gssd_plan_fn_index(b'gssd_abi_version') == -1 and lib.gssd_plan_fn_nargs(10 ** 6) == -1
    assert max(have.values()) <= 24 and ctypes.sizeof(_lib.PlanOp) == 16 + 24 * 8 == lib.gssd_plan_op_size()
    # words: integers sign-extended, float / double as their bits, pointers by value, byref(struct) -> its address
    assert planrun.word(_lib.c_i, -1) == 2 ** 64 - 1 and planrun.word(_lib.c_i64, 1 << 40) == 1 << 40
    assert planrun.word(_lib.c_f, 0.5) == struct.unpack('<I', struct.pack('<f', 0.5))[0]
    assert planrun.word(_lib.c_d, -2.25) == struct.unpack('<Q', struct.pack('<d', -2.25))[0]
    d = _lib.ConvDesc()
    assert planrun.word(ctypes.POINTER(_lib.ConvDesc), ctypes.byref(d)) == ctypes.addressof(d) and planrun.word(_lib.c_fp, None) == 0
    # a program: a launch that the entry point itself refuses (null descriptor fields) -> its code and its index come back
    prog = planrun.Program([('wait', planrun.MAIN, planrun.MAIN), ('launch', lib.gssd_conv2d_nhwc_f32, (ctypes.byref(d),), planrun.MAIN)])
    with pytest.raises(_lib.GssdError, match=r'plan op 1 \(gssd_conv2d_nhwc_f32\)'):
        prog.run(0)
    ops_ = (_lib.PlanOp * 1)()
    ops_[0].kind, ops_[0].fn, ops_[0].stream = _lib.PLAN_LAUNCH, 10 ** 6, 0
    failed = ctypes.c_int(-7)
    streams = (_lib.c_fp * 1)()
    assert lib.gssd_plan_run(ops_, 1, streams, 1, ctypes.byref(failed)) == -1 and failed.value == 0
    ops_[0].fn, ops_[0].nargs = lib.gssd_plan_fn_index(b'gssd_conv2d_nhwc_f32'), 3                       # wrong argument count
    assert lib.gssd_plan_run(ops_, 1, streams, 1, ctypes.byref(failed)) == -1 and b'argument count' in lib.gssd_last_error()
    ops_[0].stream = 5
    assert lib.gssd_plan_run(ops_, 1, streams, 1, ctypes.byref(failed)) == -1 and b'stream index' in lib.gssd_last_error()


def test_argument_validation_without_gpu():
    """Entry points reject bad descriptors before touching the device."""
    from gssd import _lib
    d = _lib.ConvDesc()
    assert _lib.lib.gssd_conv2d_nhwc_f32(ctypes.byref(d), None) == -1
    assert b'invalid argument' in _lib.lib.gssd_last_error()
    assert _lib.lib.gssd_detect(None, None, None, 1, 8732, 2, 200, 0.01, 0.45, 0.1, 0.2, 0, 0, None, None, None, None) == -1


def test_conv_x6_host_rules():
    """Host side of csrc/conv_x6.hip (no device work): the tile rule, the size of the three-plane weight form, and which descriptors
    gssd_conv2d_nhwc_f32 hands to the kernel (gssd_conv_x6_takes)."""
    from gssd import _lib, ops
    lib = _lib.lib
    assert [lib.gssd_conv_x6_tile(c, 4, 46208) for c in (32, 64, 96, 128, 216, 256, 1024)] == [64, 64, 128, 128, 128, 128, 128]
    # (3 bf16 + 3 fp16 planes, round 6) x groups x ceil(cout_g / tile) x tile x taps x cin_g 16-bit elements; -1 for shapes the kernel does not take
    assert lib.gssd_conv_x6_weight_elems(1024, 4, 128, 9, 128) == 6 * 4 * 2 * 128 * 9 * 128
    assert lib.gssd_conv_x6_weight_elems(216, 1, 512, 9, 128) == 6 * 1 * 2 * 128 * 9 * 512          # 216 -> two 128-column tiles, zero rows
    assert lib.gssd_conv_x6_weight_elems(512, 1, 48, 1, 128) == -1                                    # cin_g % 32 != 0
    assert lib.gssd_conv_x6_weight_elems(512, 1, 64, 1, 96) == -1                                     # not a tile width
    assert lib.gssd_conv_x6_weight_elems(512, 1, 64, 1, 256) == -1                                    # nor is 256
    assert ops.x6_wanted(1, 512, 512, 1, 46208) and ops.x6_wanted(3, 128, 256, 4, 11552)
    assert not ops.x6_wanted(3, 128, 128, 4, 46208, winograd=True) and not ops.x6_wanted(1, 512, 64, 1, 46208) and not ops.x6_wanted(1, 512, 512, 1, 3200)
    # Winograd shapes: only forward launches on maps too small for conv_wino_x6 (conv5_x at batch 32), and only on the fp16 planes
    assert ops.x6_wanted(3, 128, 128, 4, 11552, winograd=True, forward=True) == ops.X6_F16
    assert not ops.x6_wanted(3, 128, 128, 4, 11552, winograd=True) and not ops.x6_wanted(3, 128, 128, 4, 46208, winograd=True, forward=True)
    buf = torch.zeros(64, dtype=torch.float32)             # any 16-byte aligned host address: takes() only inspects the descriptor

    def desc(**kw):
        args = dict(B=2, H=19, W=19, in_stride=256, cin_g=256, Cout=512)
        args.update(kw)
        d, _, _ = ops.make_conv_desc(buf, buf, buf, wgt_x6=args.pop('x6', buf), **args)
        return lib.gssd_conv_x6_takes(ctypes.byref(d))
    assert desc() == 1
    assert desc(x6=None) == 0                               # no three-plane weights: the fp32-MFMA kernels
    assert desc(alpha=buf, gate=buf, resid=buf, out2=buf, relu=True, stats=torch.zeros(8, dtype=torch.float64)) == 1
    assert desc(out2=buf) == 0                              # a second output only exists behind a gate
    assert desc(split_k=2) == 0 and desc(out_mode=_lib.OUT_TRANSPOSED, m_per_image=True, out_stride=364) == 0
    assert desc(cin_g=48, in_stride=48) == 0 and desc(Cout=24) == 0
    # the merged Self_Attn projection: split-transposed store, whole tiles on either side of split_n, flat or contiguous per-image batches
    sp = dict(Cout=384, out_mode=_lib.OUT_SPLIT_T, out_b=buf, split_n=128, out_stride=128, out_b_stride=364, flags=_lib.CONV_OUT_F32,
              in_batch_stride=361 * 256, out_batch_stride=361 * 128, outb_batch_stride=256 * 364)
    assert desc(**sp) == 1 and desc(m_per_image=True, **sp) == 1
    assert desc(**dict(sp, split_n=64, out_stride=64, out_batch_stride=361 * 64)) == 0
    assert desc(m_per_image=True, **dict(sp, in_batch_stride=400 * 256)) == 0


def _kernel_name(bf16=False, cap=64, **kw):
    """(code, name) of gssd_conv2d_kernel_name for an ops.make_conv_desc(**kw) descriptor over 16-byte aligned host addresses (nothing
    dereferences them); P in a keyword's value stands for such an address."""
    from gssd import _lib, ops
    kw = {k: (_ADDR if v is P else v) for k, v in kw.items()}
    d, _, _ = ops.make_conv_desc(_ADDR, _ADDR, _ADDR, **kw)
    buf = ctypes.create_string_buffer(b'?' * (max(cap, 1) - 1), max(cap, 1))
    return _lib.lib.gssd_conv2d_kernel_name(ctypes.byref(d), int(bf16), buf, cap), buf.value.decode()


P = object()
_ADDR = torch.zeros(64, dtype=torch.float32)
_POOL2, _F16, _F32OUT, _NCHW3, _GCAT, _PLANES, _RXF = 8, 32, 1, 64, 128, 256, 512          # GSSD_CONV_* flags (include/gssd_hip.h)
_XF = dict(in_scale=P, in_shift=P, in_pad=P)
# grouped 3x3 trunk layers (4 groups), dense 3x3 / 1x1 convs, the merged multibox head, the merged Self_Attn projection
_G4 = lambda ci, co, H, B=2, **kw: dict(dict(B=B, H=H, W=H, groups=4, cin_g=ci, in_stride=4 * ci, Cout=4 * co, k=3, pad=1), **kw)
_D3 = lambda ci, co, H, W, B=1, **kw: dict(dict(B=B, H=H, W=W, cin_g=ci, in_stride=ci, Cout=co, k=3, pad=1), **kw)
_D1 = lambda ci, co, H, W, B=1, **kw: dict(dict(B=B, H=H, W=W, cin_g=ci, in_stride=ci, Cout=co), **kw)
_HEAD = lambda B, **kw: _D3(512, 24, 38, 38, B, out_mode=2, out_b=P, split_n=16, out_batch_stride=8732 * 4, outb_batch_stride=8732 * 2, **kw)
_SPLIT = lambda sn, **kw: _D1(512, 384, 64, 64, 16, out_mode=3, out_b=P, split_n=sn, out_stride=sn, out_b_stride=4096,
                              outb_batch_stride=(384 - sn) * 4096, **kw)
_PLANES_D = lambda obs: _D1(256, 384, 20, 20, 2, wgt_x6=P, out_mode=3, out_b=P, split_n=128, out_stride=128, out_b_stride=obs,
                            outb_batch_stride=256 * obs, flags=_PLANES)
_BIG = dict(B=16, H=64, W=64)                # M = 65 536 rows = 512 row tiles: one full round of 128 x 128 workgroups

KERNEL_NAME_ROWS = [
    # ---- gssd_conv2d_nhwc_f32, in dispatch order: the flags only one kernel serves ----
    ('nchw3', False, _G4(4, 16, 300, flags=_NCHW3), 'conv_thin<4,16>'),
    ('nchw3 declined', False, _G4(4, 32, 300, flags=_NCHW3), "EINVAL GSSD_CONV_IN_NCHW3: not conv1_1's shape"),
    ('groupcat', False, _D1(256, 512, 19, 19, 2, wgt_x6=P, flags=_GCAT, split_n=128, out_stride=1024), 'conv_x6<128>'),
    ('groupcat declined', False, _D1(256, 512, 19, 19, 2, flags=_GCAT, split_n=128, out_stride=1024),
     'EINVAL GSSD_CONV_OUT_GROUPCAT: csrc/conv_x6.hip does not take this descriptor'),
    ('resid_xf', False, _D1(256, 512, 19, 19, 2, wgt_x6=P, flags=_RXF, resid=P, **_XF), 'conv_x6<128>'),
    ('resid_xf declined', False, _D1(256, 512, 19, 19, 2, wgt_x6=P, flags=_RXF, **_XF),
     'EINVAL GSSD_CONV_RESID_XF: csrc/conv_x6.hip does not take this descriptor'),
    ('x6planes', False, _PLANES_D(416), 'conv_x6<128>'),
    ('x6planes declined', False, _PLANES_D(400), 'EINVAL GSSD_CONV_OUT_X6PLANES: csrc/conv_x6.hip does not take this descriptor'),
    # ---- wgt_patch / wgt_x6 present and absent ----
    ('patch', False, _D3(512, 108, 38, 38, 2, wgt_patch=P, flags=_F16), 'conv_patch_x6<128>'),
    ('patch absent', False, _D3(512, 108, 38, 38, 2, flags=_F16), 'conv_igemm<64x64>'),
    ('x6', False, _D1(256, 512, 19, 19, 2, wgt_x6=P), 'conv_x6<128>'),
    ('x6 64 columns', False, _D1(256, 64, 19, 19, 2, wgt_x6=P), 'conv_x6<64>'),
    ('x6 absent', False, _D1(256, 512, 19, 19, 2), 'conv_igemm<64x64>'),
    # ---- the thin grouped layers: 75 x 75 against 74 x 74, fused input transform, pooled epilogue ----
    ('thin_x6', False, _G4(16, 16, 75), 'conv_thin_x6<16,16>/plain'),
    ('thin_x6 74', False, _G4(16, 16, 74), 'conv_igemm<128x16>'),
    ('thin_x6 xf', False, _G4(16, 16, 75, **_XF), 'conv_thin_x6<16,16>'),
    ('thin_x6 16,32', False, _G4(16, 32, 150), 'conv_thin_x6<16,32>/plain'),
    ('thin_x6 pool2', False, _G4(16, 16, 150, flags=_POOL2, pool_sign=P), 'conv_thin_x6<16,16>/plain/pool2'),
    ('thin_x6 xf pool2', False, _G4(32, 32, 150, flags=_POOL2, pool_sign=P, **_XF), 'conv_thin_x6<32,32>/pool2'),
    ('pool2 without pool_sign', False, _G4(16, 16, 150, flags=_POOL2), 'EINVAL GSSD_CONV_POOL2: no fp32 kernel with a pooled epilogue'),
    ('thin_x6 32,64 f16', False, _G4(32, 64, 75, flags=_F16), 'conv_thin_x6<32,64>/plain'),
    ('32,64 not flagged', False, _G4(32, 64, 75), 'conv_igemm<128x64>'),
    ('thin_wino', False, _G4(16, 16, 75, wgt_wino=P, wgt_row_stride=152), 'conv_thin_wino<16,16>'),       # (padded weight rows: not conv_thin_x6's)
    ('thin_wino absent', False, _G4(16, 16, 75, wgt_row_stride=152), 'conv_igemm<128x16>'),
    ('thin', False, _G4(4, 16, 300), 'conv_thin<4,16>'),
    ('thin 74', False, _G4(4, 16, 74), 'conv_igemm<128x16>'),
    # ---- Winograd: wgt_wino present and absent, the size gate of the three-plane form, the heads ----
    ('wino 32', False, _G4(32, 32, 38, wgt_wino=P), 'conv_wino<32>/plain'),
    ('wino absent', False, _G4(32, 32, 38), 'conv_igemm<128x32>'),
    ('wino 32 xf pool2', False, _G4(32, 32, 38, wgt_wino=P, flags=_POOL2, pool_sign=P, **_XF), 'conv_wino<32>/pool2'),
    ('wino pool2 without pool_sign', False, _G4(32, 32, 38, wgt_wino=P, flags=_POOL2), 'EINVAL GSSD_CONV_POOL2: no fp32 kernel with a pooled epilogue'),
    ('wino 64 small batch', False, _G4(32, 64, 75, wgt_wino=P), 'conv_wino<64>/plain'),
    ('wino_x6 64', False, _G4(32, 64, 75, B=8, wgt_wino=P), 'conv_wino_x6<64>/plain'),
    ('wino_x6 64 xf pool2', False, _G4(64, 64, 75, B=8, wgt_wino=P, flags=_POOL2, pool_sign=P, **_XF), 'conv_wino_x6<64>/pool2'),
    ('head on wino_x6', False, _HEAD(24, wgt_wino=P, flags=_F16), 'conv_wino_x6<32>/plain'),
    ('head small batch', False, _HEAD(8, wgt_wino=P, flags=_F16), 'conv_igemm<128x32>'),
    ('head not flagged', False, _HEAD(24, wgt_wino=P), 'conv_igemm<128x32>'),
    # ---- the slot-scheduled GEMM and the implicit-GEMM tiles: B Ho Wo at 512 / 513 and 4096 / 4097, per-image M at 128 / 129 ----
    ('gemm_slot', False, _D1(512, 512, 38, 38, 32), 'gemm_slot<128x128>'),
    ('M 512', False, _D3(64, 128, 16, 32), 'conv_igemm<32x64>'),
    ('M 513', False, _D3(64, 128, 27, 19), 'conv_igemm<64x64>'),
    ('M 4096', False, _D3(64, 128, 64, 64), 'conv_igemm<64x64>'),
    ('M 4097', False, _D3(64, 128, 17, 241), 'conv_igemm<128x64>'),
    ('per image M 128', False, _D3(64, 128, 8, 16, 8, m_per_image=True), 'conv_igemm<32x64>'),
    ('per image M 129', False, _D3(64, 128, 3, 43, 8, m_per_image=True), 'conv_igemm<64x64>'),
    # cout_g at 16 / 17, 32 / 33, 64 / 65 (M = 65 536: 65 channels fill one round of 128 x 128 workgroups)
    ('cout 16', False, _D3(64, 16, **_BIG), 'conv_igemm<128x16>'),
    ('cout 17', False, _D3(64, 17, **_BIG), 'conv_igemm<128x32>'),
    ('cout 32', False, _D3(64, 32, **_BIG), 'conv_igemm<128x32>'),
    ('cout 33', False, _D3(64, 33, **_BIG), 'conv_igemm<128x64>'),
    ('cout 64', False, _D3(64, 64, **_BIG), 'conv_igemm<128x64>'),
    ('cout 65', False, _D3(64, 65, **_BIG), 'conv_igemm<128x128>'),
    ('cout 128 wave quantisation', False, _D3(64, 128, 38, 38, 32), 'conv_igemm<128x64>'),       # 361 workgroups of 512 against 722 of 768
    # K at 256 / 260 (K = taps x cin_g, cin_g a multiple of 4; a fused input transform keeps gemm_slot out)
    ('K 256', False, _D1(256, 128, **_BIG, **_XF), 'conv_igemm<128x64>'),
    ('K 260', False, _D1(260, 128, **_BIG, **_XF), 'conv_igemm<128x128>'),
    # GSSD_OUT_SPLIT_T: split_n must be whole 128-column tiles for the wide tile (the Python restatement had no such term)
    ('split_t 64', False, _SPLIT(64, **_XF), 'conv_igemm<128x64>'),
    ('split_t 128', False, _SPLIT(128, **_XF), 'conv_igemm<128x128>'),
    ('split_t 192', False, _SPLIT(192, **_XF), 'conv_igemm<128x64>'),
    # conv_thin's own shape rule (the restatement tested the channel counts and the map only): a residual, padded weight rows
    ('thin with residual', False, _G4(4, 16, 300, resid=P), 'conv_igemm<128x16>'),
    ('thin padded rows', False, _G4(4, 16, 300, wgt_row_stride=44), 'conv_igemm<128x16>'),
    # ---- gssd_conv2d_nhwc_bf16 ----
    ('bf16 fp32-only flag', True, _G4(8, 16, 300, flags=_NCHW3), 'EINVAL invalid argument: !(d.flags & (GSSD_CONV_IN_NCHW3'),
    ('thin_bf16', True, _G4(8, 16, 300), 'conv_thin_bf16<8,16>'),
    ('thin_bf16 75', True, _G4(16, 16, 75), 'conv_thin_bf16<16,16>'),
    ('thin_bf16 74', True, _G4(16, 16, 74), 'conv_bf16<128x16>'),
    ('thin_bf16 pool2', True, _G4(32, 32, 150, flags=_POOL2, pool_sign=P, **_XF), 'conv_thin_bf16<32,32>/pool2'),
    ('bf16 pool2 without pool_sign', True, _G4(32, 32, 150, flags=_POOL2), 'EINVAL GSSD_CONV_POOL2: no bf16 kernel with a pooled epilogue'),
    ('thin_bf16 with gate', True, _G4(16, 16, 150, gate=P), 'conv_bf16<128x16>'),       # (the restatement left gssd_try_conv_thin_bf16's epilogue terms out)
    ('flat 64 channels', True, _G4(64, 64, 75), 'conv_flat_bf16<64,64,128>'),
    ('flat 64 channels, full tiles', True, _G4(64, 64, 75, B=32), 'conv_flat_bf16<64,64,256>'),
    ('flat 128 channels', True, _G4(128, 128, 38), 'conv_flat_bf16<128,128,128>'),
    ('flat dilated', True, _G4(128, 128, 19, B=32, pad=6, dil=6), 'conv_flat_bf16<128,128,128>'),
    ('bf16 M 512', True, _D3(64, 128, 16, 32), 'conv_bf16<32x64>'),
    ('bf16 M 513', True, _D3(64, 128, 27, 19), 'conv_bf16<64x64>'),
    ('bf16 M 4097', True, _D3(64, 128, 17, 241), 'conv_bf16<128x64>'),
    ('bf16 cout 16', True, _D3(64, 16, **_BIG), 'conv_bf16<128x16>'),
    ('bf16 cout 17', True, _D3(64, 17, **_BIG, flags=_F32OUT), 'conv_bf16<128x32>'),
    ('bf16 cout 33', True, _D3(64, 33, **_BIG, flags=_F32OUT), 'conv_bf16<128x64>'),
    ('bf16 cout 65', True, _D3(64, 65, **_BIG, flags=_F32OUT), 'conv_bf16<128x128>'),
    ('bf16 K 256', True, _D1(256, 128, **_BIG), 'conv_bf16<128x64>'),
    ('bf16 K 264', True, _D1(264, 128, **_BIG), 'conv_bf16<128x128>'),
    ('bf16 split_t 192', True, _SPLIT(192, m_per_image=True, flags=_F32OUT, in_batch_stride=4096 * 512, out_batch_stride=4096 * 192), 'conv_bf16<128x64>'),
    ('bf16 split_t 128', True, _SPLIT(128, m_per_image=True, flags=_F32OUT, in_batch_stride=4096 * 512, out_batch_stride=4096 * 128), 'conv_bf16<128x128>'),
]


@pytest.mark.parametrize('row', KERNEL_NAME_ROWS, ids=lambda r: ('bf16 ' if r[1] and not r[0].startswith('bf16') else '') + r[0])
def test_conv2d_kernel_name(row):
    """gssd_conv2d_kernel_name: one row per leaf of the two conv dispatchers and per boundary where the leaf changes -- the name the
    launch path itself arrives at, on a host without a GPU.  A descriptor the entry point refuses is GSSD_EINVAL with the launch's text."""
    from gssd import _lib
    _, bf16, kw, want = row
    rc, name = _kernel_name(bf16, **kw)
    if want.startswith('EINVAL '):
        assert rc == -1 and name == '' and want[7:] in _lib.lib.gssd_last_error().decode(), (rc, name, _lib.lib.gssd_last_error())
    else:
        assert (rc, name) == (0, want), _lib.lib.gssd_last_error()


def test_conv2d_kernel_name_buffer_and_takes():
    """A buffer too short for the name is an error, never a truncated name; gssd_conv_flat_bf16_takes reports the pixel tile of the same walk."""
    from gssd import _lib, ops
    kw = _G4(64, 64, 75, B=32)
    assert _kernel_name(True, cap=26, **kw) == (0, 'conv_flat_bf16<64,64,256>')             # 25 characters + NUL
    for cap in (25, 8, 1):
        rc, name = _kernel_name(True, cap=cap, **kw)
        assert rc == -1 and name == '' and b'needs 26 bytes' in _lib.lib.gssd_last_error()
    d, _, _ = ops.make_conv_desc(_ADDR, _ADDR, _ADDR, **kw)
    assert _lib.lib.gssd_conv2d_kernel_name(ctypes.byref(d), 1, None, 64) == -1 and _lib.lib.gssd_conv2d_kernel_name(None, 0, ctypes.create_string_buffer(8), 8) == -1
    assert _lib.lib.gssd_conv_flat_bf16_takes(ctypes.byref(d)) == 256
    d.B = 2
    assert _lib.lib.gssd_conv_flat_bf16_takes(ctypes.byref(d)) == 128
    d.gate = d.out
    assert _lib.lib.gssd_conv_flat_bf16_takes(ctypes.byref(d)) == 0


@pytest.mark.parametrize('env,bf16,kw,want', [
    # switches the Python restatement of the dispatch had lost or never had (they are read once per process: a child each)
    ({'GSSD_NO_GEMM_SLOT': '1'}, False, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=512)", 'conv_igemm<128x128>'),
    ({'GSSD_BF16_BIG_TILES': '1'}, True, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=512)", 'conv_bf16<256x128>'),
    ({'GSSD_BF16_BIG_TILES': '3'}, True, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=512)", 'conv_bf16<192x128>'),
    ({'GSSD_BF16_BIG_TILES': '5'}, True, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=256)", 'conv_bf16<128x128>'),
    ({'GSSD_NO_SMALL_TILES': '1'}, False, "dict(B=1, H=16, W=32, cin_g=64, in_stride=64, Cout=128, k=3, pad=1)", 'conv_igemm<128x64>'),
    ({'GSSD_CONV21_WINO': '0'}, False, "dict(B=2, H=150, W=150, groups=4, cin_g=16, in_stride=64, Cout=128, k=3, pad=1, wgt_wino=a, wgt_row_stride=144, relu=False, "
                                       "flags=0, out2=a)", 'conv_thin<16,32>'),
    # conv_x6's forced tile width: 64 or 128, anything else is ignored (the rule gives 512 channels in one group 128 columns)
    ({'GSSD_X6_BN': '64'}, False, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=512, wgt_x6=a)", 'conv_x6<64>'),
    ({'GSSD_X6_BN': '256'}, False, "dict(B=32, H=38, W=38, cin_g=512, in_stride=512, Cout=512, wgt_x6=a)", 'conv_x6<128>'),
])
def test_conv2d_kernel_name_follows_switches(env, bf16, kw, want):
    import subprocess
    import sys
    src = ('import ctypes, torch\nfrom gssd import _lib, ops\na = torch.zeros(64)\n'
           f'd, _, _ = ops.make_conv_desc(a, a, a, **{kw})\nbuf = ctypes.create_string_buffer(64)\n'
           f'assert _lib.lib.gssd_conv2d_kernel_name(ctypes.byref(d), {int(bf16)}, buf, 64) == 0, _lib.lib.gssd_last_error()\nprint(buf.value.decode())\n')
    r = subprocess.run([sys.executable, '-c', src], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path), **env))
    assert r.returncode == 0 and r.stdout.strip() == want, (r.stdout, r.stderr[-2000:])


def test_priorbox_bit_exact(golden):
    from layers.functions import PriorBox
    from data import v2, v2_512
    g = golden('priors')
    p = PriorBox(v2).forward()
    assert p.dtype == torch.float32 and np.array_equal(p.numpy(), g['v2'])
    p5 = PriorBox(v2_512).forward().numpy()
    assert p5.shape == (24564, 4) and np.array_equal(p5[g['v2_512_sample_idx']], g['v2_512_sample'])


@pytest.mark.parametrize('name,args', [
    ('gssd', (True, 4, 4, 1, True, False, False, 0, 1, False, False, 1)),
    ('gssd_sa', (True, 4, 4, 1, True, True, True, 0, 1, False, False, 1)),
    ('gssdpp', (True, 4, 4, 1, True, True, True, 1, 4, True, False, 1)),
])
def test_module_tree_matches_reference(golden, name, args):
    from models.ssd_multiphase_custom_group import build_ssd, weights_init
    g = golden('e2e')
    net = build_ssd('train', 300, 2, *args)
    sd = net.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in g[f'{name}.keys']]
    assert [str(tuple(sd[k].shape)) for k in sorted(sd.keys())] == [str(s) for s in g[f'{name}.shapes']]
    # the surface the driver touches (train_lesion_multiphase_v2.py:587-615)
    net.extras.apply(weights_init)
    net.loc.apply(weights_init)
    net.conf.apply(weights_init)
    twin = copy.deepcopy(net)
    assert twin._engine is not net._engine and twin._engine.net is twin
    test_net = build_ssd('test', 300, 2, *args)
    test_net.load_state_dict(net.state_dict())                 # strict, train -> test phase
    if name == 'gssdpp':
        assert any(n.startswith('dcn_list') for n, _ in net.named_parameters())
    assert net.priors.shape == (8732, 4)


def test_vanilla_module_tree(golden):
    from models.ssd import build_ssd
    g = golden('e2e')
    net = build_ssd('train', 300, 2)
    sd = net.state_dict()
    assert sorted(sd.keys()) == [str(k) for k in g['ssd.keys']]
    assert [str(tuple(sd[k].shape)) for k in sorted(sd.keys())] == [str(s) for s in g['ssd.shapes']]
    assert build_ssd('train', 512, 2) is None and build_ssd('x', 300, 2) is None


def test_build_ssd_rejects_like_reference(capsys):
    from models.ssd_multiphase_custom_group import build_ssd
    assert build_ssd('val', 300, 2, True) is None
    assert build_ssd('train', 512, 2, True) is None
    assert 'only SSD300' in capsys.readouterr().out
    with pytest.raises(AssertionError):
        build_ssd('train', 300, 2, True, 4, 4, 1, True, False, False, 1, 4, True, False, 1)   # cat_sab needs sab


def test_pool_and_pack_helpers():
    from gssd import ops
    for n, k, s, p, ceil in [(300, 2, 2, 0, False), (75, 2, 2, 0, True), (19, 3, 1, 1, False), (38, 2, 2, 0, False),
                             (5, 2, 2, 0, True), (7, 3, 2, 1, True)]:
        ref = torch.nn.functional.max_pool2d(torch.zeros(1, 1, n, n), k, s, p, ceil_mode=ceil).shape[-1]
        assert ops.pool_out_size(n, k, s, p, ceil) == ref
    tg = [torch.rand(2, 5), torch.rand(0, 5), torch.rand(3, 5)]
    flat, off = ops.pack_targets(tg, 'cpu')
    assert off.tolist() == [0, 2, 2, 5] and torch.equal(flat[2:], tg[2])
    assert ops.packed_k(3, 3, 3) == (4, 36)


def test_synth_is_deterministic():
    from gssd import synth
    a, b = synth.synth_images(2, seed=4), synth.synth_images(2, seed=4)
    assert torch.equal(a, b) and float(a.min()) == 0.0 and float(a.max()) == 1.0
    t = synth.synth_targets(4, seed=1)
    assert all(x.shape[1] == 5 and 1 <= x.shape[0] <= 3 for x in t)


def test_resample_coefficients_match_pillow_restatement():
    """Host half of the input stage (no GPU): the C library's fixed-point tables equal the oracle's (pinned on Pillow)."""
    from gssd import input_stage as IS
    from oracle import input_oracle as IO
    for a, b in ((512, 300), (64, 37), (20, 33), (300, 300), (513, 127)):
        for f in ('bicubic', 'bilinear'):
            bo, ko, ks = IO.resample_coeffs(a, b, f)
            bh, kh = IS.resample_tables(a, b, f)
            assert kh.shape[1] == ks and np.array_equal(bo, bh) and np.array_equal(ko, kh), (a, b, f)
    with pytest.raises(Exception):
        IS.resample_tables(0, 300)
    with pytest.raises(Exception):
        IS.DeviceInputStage(300)(torch.zeros(1, 4, 8, 8, 3, dtype=torch.uint8))      # CPU tensor: no fallback


def _run_bench(*args, env=None):
    import json
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    return r.returncode, [json.loads(ln) for ln in lines]


def test_bench_self_launch_refuses_missing_gpus_in_one_line():
    """`python bench.py --gpus N` on a host with fewer GPUs: one JSON error line, non-zero exit, nothing spawned."""
    ndev = torch.cuda.device_count()
    rc, lines = _run_bench('--gpus', str(ndev + 2))
    assert rc == 2 and len(lines) == 1 and lines[0]['devices_visible'] == ndev and 'error' in lines[0]


def test_bench_self_launch_two_ranks_rendezvous():
    """The self-launcher (no torch.distributed.run): two child ranks find each other on 127.0.0.1, rank 0 alone prints the line,
    the parent returns their code; a rank that dies ends the job with ITS code instead of hanging the others."""
    rc, lines = _run_bench('--gpus', '2', '--launch-probe')
    assert rc == 0 and len(lines) == 1
    assert lines[0]['ranks'] == [0.0, 1.0] and lines[0]['rccl_ranks'] == 2 and lines[0]['launcher'] == 'self'
    rc, lines = _run_bench('--gpus', '2', '--launch-probe', env={'GSSD_PROBE_FAIL_RANK': '1'})
    assert rc == 7 and lines == []


def test_bench_extra_legs_need_full():
    """A plain run times the headline only: asking for the training-step leg without --full is an error before anything starts."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--full-step', '2'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--full' in r.stderr and not r.stdout.strip()


def test_bench_dump_outputs_sample_is_fixed_and_bounded(tmp_path):
    """--dump-outputs: arrays as float32 .npy; past 64 MB in all, the same seeded sample of elements in every run."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    small = dict(loc=np.arange(12, dtype=np.float64).reshape(3, 4), loss_l=np.float32(1.5))
    bench.dump_outputs(small, str(tmp_path / 'a'))
    back = np.load(tmp_path / 'a' / 'loc.npy')
    assert back.dtype == np.float32 and np.array_equal(back, small['loc']) and np.load(tmp_path / 'a' / 'loss_l.npy') == 1.5
    big = dict(x=np.random.default_rng(1).standard_normal(20 << 20, dtype=np.float32), y=np.ones(3, np.float32))
    for d in ('b', 'c'):
        bench.dump_outputs(big, str(tmp_path / d))
    size = sum(os.path.getsize(tmp_path / 'b' / f) for f in os.listdir(tmp_path / 'b'))
    assert size <= bench.DUMP_LIMIT == 64 << 20 and size > 48 << 20
    xb, xc = np.load(tmp_path / 'b' / 'x.npy'), np.load(tmp_path / 'c' / 'x.npy')
    assert xb.dtype == np.float32 and xb.size < big['x'].size and np.array_equal(xb, xc)
    assert np.array_equal(np.load(tmp_path / 'b' / 'y.npy'), big['y'])


def test_bench_stdout_line_is_short_and_parses(tmp_path):
    """the driver keeps a bounded tail of stdout -- the ONE JSON line must stay under 8 KB (r04's 21.6 KB line left
    BENCH_r04.parsed = null).  Replays a full record of a real run (the committed round-4 detail, per-rank lists widened to 8 ranks)
    through bench.py's own line builder and through the CLI, and checks the contract's fields + roofline + cpu_baseline survive."""
    import json
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    import bench
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r04_h_gssdpp_b32_bench.json')))
    assert len(json.dumps(full)) > 2 * bench.LINE_LIMIT                      # the record itself is the long form
    for world in (1, 8):
        rec = json.loads(json.dumps(full))
        rec['n_gpus'] = rec['rccl_ranks'] = world
        rec['per_rank_ms_per_step'] = rec['per_rank_ms_per_step'] * world
        rec['host_enqueue_ms_per_step'] = rec['host_enqueue_ms_per_step'] * world
        rec['full_step']['host_enqueue_ms_per_step'] = rec['full_step']['host_enqueue_ms_per_step'] * world
        line = bench.compact_line(rec, 'gpurun_out/bench_detail.json')
        txt = json.dumps(line)
        assert len(txt) < bench.LINE_LIMIT == 8192, len(txt)
        back = json.loads(txt)
        for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline',
                  'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
            assert k in back, k
        assert 'workload' in back['config'] and 'model' not in back['config']
        for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
            assert k in back['roofline'], k
        for k in ('value', 'unit', 'cores', 'kind', 'sample'):
            assert k in back['cpu_baseline'], k
        assert 'kernels' not in back and 'trunk' not in back
    p = tmp_path / 'detail.json'
    p.write_text(json.dumps(full))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--replay-detail', str(p)], capture_output=True, text=True, timeout=300)
    last = r.stdout.strip().splitlines()[-1]
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == 1 and len(last) < 8192
    assert json.loads(last)['value'] == full['value']


def test_fp16_planes_are_flagged_only_for_train_mode_fp32_plans():
    """gssd/plan_ops.py::PlanOpsMixin.f16_ok: GSSD_CONV_F16_OK goes on forward launches of a train-mode, fp32-mode plan only (batch-statistics
    BatchNorm bounds the activations); eval mode, the bf16 storage mode and PixelLink's plan (a trunk without BatchNorm) never flag."""
    from gssd import _lib
    from gssd.plan_ops import PlanOpsMixin
    from gssd.pixellink import _PlanPixelLink

    import types

    class P(PlanOpsMixin):
        def __init__(self, training, bf16, batch_norm=True):
            self.training, self.bf16 = training, bf16
            self.eng = types.SimpleNamespace(net=types.SimpleNamespace(batch_norm=batch_norm))
    assert P(True, False).f16_ok == _lib.CONV_F16_OK == 32
    assert P(False, False).f16_ok == 0 and P(True, True).f16_ok == 0 and P(False, True).f16_ok == 0
    assert P(True, False, batch_norm=False).f16_ok == 0
    assert _PlanPixelLink.f16_ok == 0
    # the header documents the promise the flag makes
    hdr = open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read()
    assert '#define GSSD_CONV_F16_OK 32' in hdr and 'NEVER inferred' in hdr and 'gssd_dcn_forward_x6_ex' in hdr
