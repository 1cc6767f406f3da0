"""The generic conv kernels' case registry, shared by the CPU name test (tests/test_conv_leaf_names_cpu.py) and the GPU parity test
(tests/test_gpu_conv_leaves.py): one row per tile of csrc/conv_igemm.hip / csrc/conv_bf16.hip (and csrc/gemm_slot.hip) at the smallest
shape that selects it, and one per epilogue / operand form of the generic kernel on the widest tile it reaches plus a three-stage tile
(32x64 / 64x64: another K loop).  A row is

    (id, bf16, ops.make_conv_desc keywords, expected gssd_conv2d_kernel_name, features)

in the style of tests/test_host_cpu.py::KERNEL_NAME_ROWS.  P in a keyword's value stands for a pointer: the CPU test puts any aligned host
address there (nothing dereferences it), the GPU test a tensor it builds from the other keywords (tests/test_gpu_conv_leaves.py::build).
Every size is spelled out in the keywords, so both tests see the same descriptor.

Shapes.  D(cin, cout, H, W) is a dense 3x3 / pad 1 conv at B = 1.  36 input channels: K = 324 = 10 chunks of 32 + 4 (the fp32 K tail);
40 in bf16: K = 360 = 5 chunks of 64 + 40.  65 x 64 pixels: M = 4160 = 32 row tiles of 128 + 64, the first M past the 64-row tiles' 4096.
136 outputs = 128 + 8: the ragged second column tile of the 128-wide tiles.
"""

P = object()

OUT_NHWC, OUT_TRANSPOSED, OUT_HEADS, OUT_SPLIT_T = 0, 1, 2, 3          # GSSD_OUT_* (include/gssd_hip.h)
F32OUT = 1                                                             # GSSD_CONV_OUT_F32

# what the issue of this registry asks a row for; the CPU test checks every one is carried by a row, and by a three-stage row where marked
FEATURES = ('tile', 'bias', 'relu', 'stats', 'xf', 'gate', 'heads', 'window', 'split_k uneven', 'split_k empty', 'per image', 'transposed',
            'split_t flat', 'split_t per image', 'K<32', 'K tail', 'stride', 'dilation', 'groups')
THREE_STAGE_FEATURES = ('bias', 'relu', 'stats', 'xf', 'gate', 'window', 'per image', 'transposed', 'split_t per image', 'K<32')
THREE_STAGE_TILES = ('32x64', '64x64')


def D(cin, cout, H, W, B=1, k=3, pad=1, groups=1, **kw):
    """dense (or grouped: cin / cout per group) k x k conv; in_stride defaults to the channels the groups read"""
    d = dict(B=B, H=H, W=W, groups=groups, cin_g=cin, in_stride=groups * cin, Cout=groups * cout, k=k, pad=pad)
    d.update(kw)
    return d


def PER_IMAGE(tokens_hw, cin, cout, B, in_stride=None, wgt_row_stride=None, per_image_weights=True, **kw):
    """1x1 conv as a per-image GEMM (the attention bmm's): image b multiplies its [tokens][cin] rows with ITS OWN [cout][cin] matrix"""
    H, W = tokens_hw
    in_stride = in_stride or cin
    wrs = wgt_row_stride or cin
    d = dict(B=B, H=H, W=W, cin_g=cin, in_stride=in_stride, Cout=cout, m_per_image=True, in_batch_stride=H * W * in_stride + 8,
             wgt_row_stride=wrs, wgt_batch_stride=(cout * wrs + 16) if per_image_weights else 0)
    d.update(kw)
    return d


def _nhwc_pi(tokens, out_stride):          # per-image NHWC output: images a few floats further apart than their rows need
    return dict(out_stride=out_stride, out_batch_stride=tokens * out_stride + 16)


def _transposed(cout, row):                # per image [cout][row]
    return dict(out_mode=OUT_TRANSPOSED, out_stride=row, out_batch_stride=cout * row + 8)


def SPLIT_T(split_n, cout, tokens, row, per_image, **kw):
    """merged projection: channels [0, split_n) NHWC rows of split_n floats, the rest per image transposed [cout - split_n][row]"""
    d = dict(out_mode=OUT_SPLIT_T, out_b=P, split_n=split_n, out_stride=split_n, out_b_stride=row, outb_batch_stride=(cout - split_n) * row + 4,
             out_batch_stride=tokens * split_n)
    if per_image:
        d.update(m_per_image=True)
    d.update(kw)
    return d


XF = dict(in_scale=P, in_shift=P, in_pad=P)
GATE = dict(alpha=P, gate=P, resid=P, out2=P, bias=P)
BRS = dict(bias=P, relu=True, stats=P)
# 17 anchors x (4 box coordinates | 4 classes) = 68 | 68 columns: the ragged 128 + 8 again; this source starts at prior 100 of its image
_A, _OFF = 17, 100


def HEADS(H, W, tail=50):
    pri = _OFF + H * W * _A + tail
    return dict(out_mode=OUT_HEADS, out_b=P, split_n=4 * _A, out_batch_stride=4 * pri, outb_batch_stride=4 * pri, out_off=4 * _OFF, outb_off=4 * _OFF)


ROWS = [
    # ---- csrc/conv_igemm.hip: the six tiles at the smallest shape that selects each ----
    ('128x128 ragged M / N / K', False, D(36, 136, 65, 64, **BRS), 'conv_igemm<128x128>', ('tile', 'bias', 'relu', 'stats', 'K tail')),
    ('128x128 two groups', False, D(36, 136, 65, 64, groups=2, bias=P, stats=P), 'conv_igemm<128x128>', ('tile', 'groups', 'bias', 'stats', 'K tail')),
    ('128x64', False, D(36, 40, 65, 64, bias=P, stats=P), 'conv_igemm<128x64>', ('tile', 'bias', 'stats', 'K tail')),
    ('128x32', False, D(36, 20, 65, 64, bias=P, stats=P), 'conv_igemm<128x32>', ('tile', 'bias', 'stats', 'K tail')),
    ('128x16', False, D(36, 12, 65, 64, bias=P, stats=P), 'conv_igemm<128x16>', ('tile', 'bias', 'stats', 'K tail')),
    ('64x64 M 513', False, D(36, 72, 27, 19, **BRS), 'conv_igemm<64x64>', ('tile', 'bias', 'relu', 'stats', 'K tail')),
    ('64x64 M 4096', False, D(36, 72, 64, 64, bias=P, stats=P), 'conv_igemm<64x64>', ('tile', 'bias', 'stats', 'K tail')),
    ('32x64 M 512', False, D(36, 72, 16, 32, **BRS), 'conv_igemm<32x64>', ('tile', 'bias', 'relu', 'stats', 'K tail')),
    # (no batch sums on one pixel: the "sum" is the fp32 output itself, and the sums' bound -- 2e-7 x pixels of the largest output, the error of
    # adding fp32 values up -- is below one fp32 conv result's own rounding, which the output gate is for)
    ('32x64 M 1', False, D(36, 72, 3, 3, pad=0, bias=P, relu=True), 'conv_igemm<32x64>', ('tile', 'bias', 'relu', 'K tail')),
    ('128x128 stride 2', False, D(36, 136, 131, 129, stride=2, bias=P), 'conv_igemm<128x128>', ('stride', 'bias', 'K tail')),
    ('128x128 pad 6 dil 6', False, D(36, 136, 65, 64, pad=6, dil=6, bias=P), 'conv_igemm<128x128>', ('dilation', 'bias', 'K tail')),
    ('64x64 two groups pad 6 dil 6', False, D(36, 72, 27, 19, groups=2, pad=6, dil=6, bias=P), 'conv_igemm<64x64>', ('groups', 'dilation', 'bias', 'K tail')),
    # ---- epilogues and operand forms, each on the widest tile it reaches and on a three-stage tile ----
    ('xf 128x128', False, D(36, 136, 65, 64, bias=P, **XF), 'conv_igemm<128x128>', ('xf', 'bias', 'K tail')),
    ('xf 128x64 two groups', False, D(36, 40, 65, 64, groups=2, bias=P, stats=P, **XF), 'conv_igemm<128x64>', ('xf', 'groups', 'bias', 'stats', 'K tail')),
    ('xf 64x64', False, D(36, 72, 27, 19, bias=P, relu=True, **XF), 'conv_igemm<64x64>', ('xf', 'bias', 'relu', 'K tail')),
    ('xf 32x64 stride 2', False, D(36, 72, 31, 33, stride=2, bias=P, **XF), 'conv_igemm<32x64>', ('xf', 'stride', 'bias', 'K tail')),
    ('gate 128x128', False, D(36, 136, 65, 64, **GATE), 'conv_igemm<128x128>', ('gate', 'bias', 'K tail')),
    ('gate relu stats 64x64', False, D(36, 72, 27, 19, relu=True, stats=P, **GATE), 'conv_igemm<64x64>', ('gate', 'bias', 'relu', 'stats', 'K tail')),
    ('resid only 32x64', False, D(36, 72, 16, 32, resid=P, bias=P), 'conv_igemm<32x64>', ('gate', 'bias', 'K tail')),
    ('heads 128x128', False, D(36, 136, 65, 64, B=2, bias=P, **HEADS(65, 64)), 'conv_igemm<128x128>', ('heads', 'bias', 'K tail')),
    ('heads 64x64', False, D(36, 136, 27, 19, B=2, bias=P, **HEADS(27, 19)), 'conv_igemm<64x64>', ('heads', 'bias', 'K tail')),
    ('window 128x128', False, D(36, 136, 65, 64, in_stride=80, in_ch_off=8, out_stride=160, out_ch_off=12, **BRS), 'conv_igemm<128x128>',
     ('window', 'bias', 'relu', 'stats', 'K tail')),
    ('window two groups xf gate 64x64', False, D(36, 72, 27, 19, groups=2, in_stride=88, in_ch_off=12, out_stride=150, out_ch_off=5, **GATE, **XF),
     'conv_igemm<64x64>', ('window', 'groups', 'xf', 'gate', 'bias', 'K tail')),
    # split-K: 11 chunks over 3 slices = 4 + 4 + 3; over 16 slices = 11 x 1 and five EMPTY slices (ch_begin >= ch_end: no chunk is issued,
    # the accumulators stay zero and the epilogue adds 0.0 -- and the bias in slice 0 only); split_k > 1 never takes a three-stage tile
    ('split_k 3 of 11 chunks', False, D(36, 136, 65, 64, split_k=3, bias=P), 'conv_igemm<128x128>', ('split_k uneven', 'bias', 'K tail')),
    ('split_k 16 of 11 chunks', False, D(36, 136, 65, 64, split_k=16, bias=P), 'conv_igemm<128x128>', ('split_k empty', 'bias', 'K tail')),
    ('split_k 5 small map', False, D(36, 72, 16, 32, split_k=5, bias=P), 'conv_igemm<128x64>', ('split_k empty', 'bias', 'K tail')),
    ('split_k 4 heads', False, D(36, 136, 27, 19, B=2, split_k=4, bias=P, **HEADS(27, 19)), 'conv_igemm<128x128>', ('split_k uneven', 'heads', 'bias', 'K tail')),
    # per-image operands (the two attention bmm's): 361 tokens, K = 260 = 8 chunks + 4, each image with its own weight matrix
    ('per image nhwc 128x128', False, PER_IMAGE((19, 19), 260, 136, 12, in_stride=264, wgt_row_stride=268, bias=P, alpha=P, **_nhwc_pi(361, 140)),
     'conv_igemm<128x128>', ('per image', 'bias', 'K tail')),
    ('per image nhwc 361 of 364 columns', False, PER_IMAGE((19, 19), 260, 361, 12, in_stride=264, wgt_row_stride=268, bias=P, **_nhwc_pi(361, 364)),
     'conv_igemm<128x64>', ('per image', 'bias', 'K tail')),
    ('per image nhwc 64x64', False, PER_IMAGE((19, 19), 36, 72, 3, in_stride=40, wgt_row_stride=44, **BRS, **_nhwc_pi(361, 76)),
     'conv_igemm<64x64>', ('per image', 'bias', 'relu', 'stats', 'K tail')),
    ('transposed 361 of 364, 64x64', False, PER_IMAGE((19, 19), 36, 72, 3, bias=P, relu=True, stats=P, **_transposed(72, 364)),
     'conv_igemm<64x64>', ('per image', 'transposed', 'bias', 'relu', 'stats', 'K tail')),
    ('transposed 361 of 364, 128 rows', False, PER_IMAGE((19, 19), 260, 136, 12, bias=P, alpha=P, **_transposed(136, 364)),
     'conv_igemm<128x128>', ('per image', 'transposed', 'bias', 'K tail')),
    ('transposed 100 of 104, 32x64', False, PER_IMAGE((10, 10), 36, 72, 8, bias=P, **_transposed(72, 104)),
     'conv_igemm<32x64>', ('per image', 'transposed', 'bias', 'K tail')),
    # GSSD_OUT_SPLIT_T: flat (20 x 20 = 400 tokens in rows of 404) and per image (361 in rows of 364), split_n 64 and 128
    ('split_t flat 128', False, D(260, 136, 20, 20, B=11, k=1, pad=0, bias=P, **SPLIT_T(128, 136, 400, 404, False)), 'conv_igemm<128x128>',
     ('split_t flat', 'bias', 'K tail')),
    ('split_t flat 128, 128x64', False, D(260, 200, 20, 20, B=11, k=1, pad=0, bias=P, **SPLIT_T(128, 200, 400, 404, False)), 'conv_igemm<128x64>',
     ('split_t flat', 'bias', 'K tail')),
    ('split_t flat 64', False, D(36, 104, 20, 20, B=11, k=1, pad=0, bias=P, **SPLIT_T(64, 104, 400, 404, False)), 'conv_igemm<128x64>',
     ('split_t flat', 'bias', 'K tail')),
    ('split_t flat 64, 64x64', False, D(36, 104, 20, 20, B=3, k=1, pad=0, bias=P, **SPLIT_T(64, 104, 400, 404, False)), 'conv_igemm<64x64>',
     ('split_t flat', 'bias', 'K tail')),
    ('split_t per image 128', False, PER_IMAGE((19, 19), 260, 136, 12, per_image_weights=False, bias=P, alpha=P, **SPLIT_T(128, 136, 361, 364, True)),
     'conv_igemm<128x128>', ('split_t per image', 'per image', 'bias', 'K tail')),
    ('split_t per image 128, 128x64', False, PER_IMAGE((19, 19), 260, 200, 12, per_image_weights=False, bias=P, **SPLIT_T(128, 200, 361, 364, True)),
     'conv_igemm<128x64>', ('split_t per image', 'per image', 'bias', 'K tail')),
    ('split_t per image 64, 64x64', False, PER_IMAGE((19, 19), 36, 104, 3, per_image_weights=False, bias=P, **SPLIT_T(64, 104, 361, 364, True)),
     'conv_igemm<64x64>', ('split_t per image', 'per image', 'bias', 'K tail')),
    # K < 32: one chunk, most of it tail
    ('K 4, 64x64 two groups', False, D(4, 72, 27, 19, k=1, pad=0, groups=2, **BRS), 'conv_igemm<64x64>', ('K<32', 'groups', 'bias', 'relu', 'stats', 'K tail')),
    ('K 4, 128x128', False, D(4, 136, 65, 64, k=1, pad=0, bias=P), 'conv_igemm<128x64>', ('K<32', 'bias', 'K tail')),
    # ---- csrc/gemm_slot.hip: the smallest plain GEMM it takes (194 workgroups), ragged in M (96 x 128 + 33) and N (200 of 256) ----
    ('gemm_slot', False, D(96, 200, 111, 111, k=1, pad=0, **BRS), 'gemm_slot<128x128>', ('tile', 'bias', 'relu', 'stats')),
    # ---- csrc/conv_bf16.hip: the six tiles, a window, the transposed forms ----
    ('bf16 128x128', True, D(40, 136, 65, 64, bias=P, stats=P), 'conv_bf16<128x128>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 128x64', True, D(40, 40, 65, 64, bias=P, stats=P), 'conv_bf16<128x64>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 128x32', True, D(40, 24, 65, 64, bias=P, stats=P), 'conv_bf16<128x32>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 128x16', True, D(40, 16, 65, 64, bias=P, stats=P), 'conv_bf16<128x16>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 64x64', True, D(40, 72, 27, 19, bias=P, stats=P), 'conv_bf16<64x64>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 32x64', True, D(40, 72, 16, 32, bias=P, stats=P), 'conv_bf16<32x64>', ('tile', 'bias', 'stats', 'K tail')),
    ('bf16 window two groups 128x128', True, D(40, 136, 65, 64, groups=2, in_stride=96, in_ch_off=8, out_stride=288, out_ch_off=8, **BRS),
     'conv_bf16<128x128>', ('window', 'groups', 'bias', 'relu', 'stats', 'K tail')),
    ('bf16 transposed 361 of 364, 64x64', True, PER_IMAGE((19, 19), 40, 72, 3, bias=P, flags=F32OUT, **_transposed(72, 364)),
     'conv_bf16<64x64>', ('per image', 'transposed', 'bias', 'K tail')),
    ('bf16 split_t per image 128', True, PER_IMAGE((19, 19), 264, 136, 12, per_image_weights=False, bias=P, flags=F32OUT, **SPLIT_T(128, 136, 361, 364, True)),
     'conv_bf16<128x128>', ('split_t per image', 'per image', 'bias', 'K tail')),
]

# The other names of tests/data/conv_names_parent.json (what a production step launches): the specialised families, each with the existing
# kernel-level test that runs it against a reference.  The CPU closure test checks that every fixture name is a registry row's expected name
# or a key here, that only these families appear, and that the named test exists.
SPECIAL_FAMILIES = ('conv_x6', 'conv_patch_x6', 'conv_thin', 'conv_wino', 'conv_flat_bf16')
COVERED_ELSEWHERE = {
    'conv_x6<128>': 'tests/test_gpu_kernels.py::test_conv_x6_matches_float64',
    'conv_patch_x6<128>': 'tests/test_gpu_kernels.py::test_conv_patch_x6_matches_float64',
    'conv_thin<4,16>': 'tests/test_gpu_kernels.py::test_conv_igemm',
    'conv_thin_bf16<8,16>': 'tests/test_gpu_bf16.py::test_conv_bf16',
    'conv_thin_bf16<16,16>': 'tests/test_gpu_bf16.py::test_conv_bf16',
    'conv_thin_bf16<16,32>': 'tests/test_gpu_bf16.py::test_conv_bf16',
    'conv_thin_bf16<32,32>': 'tests/test_gpu_bf16.py::test_conv_bf16',
    'conv_thin_bf16<16,16>/pool2': 'tests/test_gpu_bf16.py::test_conv_thin_bf16_pooled_epilogue',
    'conv_thin_bf16<32,32>/pool2': 'tests/test_gpu_bf16.py::test_conv_thin_bf16_pooled_epilogue',
    'conv_thin_x6<16,16>': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<16,16>/pool2': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<16,32>': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<16,32>/plain': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<32,32>': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<32,32>/pool2': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_forms_vs_float64',
    'conv_thin_x6<32,64>': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_conv3_1_class',
    'conv_thin_x6<32,64>/plain': 'tests/test_gpu_thin_x6.py::test_conv_thin_x6_conv3_1_class',
    'conv_wino<64>': 'tests/test_gpu_kernels.py::test_conv_winograd',
    'conv_wino<64>/plain': 'tests/test_gpu_kernels.py::test_conv_winograd',
    'conv_wino<64>/pool2': 'tests/test_gpu_kernels.py::test_conv_winograd_pooled_epilogue',
    'conv_wino_x6<32>': 'tests/test_gpu_wino_x6.py::test_conv_winograd_x6_every_form_vs_float64_and_fp32_kernel',
    'conv_wino_x6<32>/plain': 'tests/test_gpu_kernels.py::test_conv_wino_x6_heads_epilogue',
    'conv_wino_x6<64>': 'tests/test_gpu_wino_x6.py::test_conv_winograd_x6_default_host_rule',
    'conv_wino_x6<64>/plain': 'tests/test_gpu_wino_x6.py::test_conv_winograd_x6_default_host_rule',
    'conv_wino_x6<64>/pool2': 'tests/test_gpu_wino_x6.py::test_conv_winograd_x6_every_form_vs_float64_and_fp32_kernel',
    'conv_flat_bf16<32,64,128>': 'tests/test_gpu_bf16.py::test_conv_flat_bf16',
    'conv_flat_bf16<32,64,256>': 'tests/test_gpu_bf16.py::test_conv_flat_bf16',
    'conv_flat_bf16<64,64,128>': 'tests/test_gpu_bf16.py::test_conv_flat_bf16',
    'conv_flat_bf16<64,64,256>': 'tests/test_gpu_bf16.py::test_conv_flat_bf16',
    'conv_flat_bf16<128,128,128>': 'tests/test_gpu_bf16.py::test_conv_flat_bf16',
    'conv_flat_bf16<64,128,128>': 'tests/test_gpu_bf16.py::test_conv_bf16',
}


def row_id(row):
    return row[0]


def resolve(kw, pointer):
    """the keywords with every P replaced by pointer(name)"""
    return {k: (pointer(k) if v is P else v) for k, v in kw.items()}


def tile_rows(name):
    """rows of the output tile of an instance name: conv_igemm<64x64> -> 64 (the rows a per-image transposed store pads with zeros to)"""
    return int(name[name.index('<') + 1:name.index('x', name.index('<'))])
