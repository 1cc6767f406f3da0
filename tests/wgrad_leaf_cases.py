"""The fp32 weight gradient's case registry, shared by the CPU name test (tests/test_wgrad_leaf_names_cpu.py) and the GPU parity test
(tests/test_gpu_wgrad_leaves.py): gssd_conv2d_wgrad_f32 (csrc/conv_wgrad.hip) tries csrc/conv_thin_wgrad.hip, csrc/conv_patch_wgrad.hip
and csrc/wgrad_slot.hip and then picks one of four tiles of its own kernel -- 18 template instances, INSTANCES below.  One row per
instance at the smallest shape at which it can still go wrong, and one per operand form on the families that take it.  A row is

    (id, ops.make_conv_desc keywords, expected gssd_conv2d_wgrad_kernel_name, features)

in the style of tests/conv_leaf_cases.py.  P in a keyword's value stands for a pointer: the CPU test puts any aligned host address there
(nothing dereferences it), the GPU test a tensor it builds from the other keywords.  Every map is non-square (a swapped extent shows).

Shapes.
  conv_wgrad<BMW x BNW> (output channels x im2col columns of a workgroup).  B Ho Wo = M with 513 <= M <= 1024 and M % 32 != 0: launch_wgrad
    makes two pixel slices and the second ends in a partial 32-pixel chunk ('two slices').  M < 4096 keeps csrc/wgrad_slot.hip away, H W <
    1444 (or channel counts it does not have) csrc/conv_patch_wgrad.hip.  2 x 17 x 19 = 646 output pixels; stride 2 from 35 x 39: 2 x 18 x
    20 = 720.  Channels per group (cout_g / cin_g, K = taps x cin_g):
      <16x256>   12 / 12, K 108   one ragged row tile, one ragged column tile
      <32x128>   36 / 20, K 180   32 + 4 rows, 128 + 52 columns; a wave's 64 columns cross tap boundaries (20, 40, ..) off the 16s
      <64x256>   68 / 32, K 288   64 + 4 rows, 256 + 32 columns
      <128x128> 132 / 20, K 180   128 + 4 rows, 128 + 52 columns
  conv_thin_wgrad<4 | 16>: groups 4, 16 outputs per group, 70 x 83 = 9 x 6 tiles of 8 x 16 (the last row of tiles 6 high, the last column 3
    wide).  54 tiles an image: B = 10 gives 540 tiles against the 512-workgroup grid, so 28 workgroups accumulate two tiles before the flush
    ('two tiles per workgroup').  <4> is the production case: 3 real input channels per group stored as 4 ('cin 3 of 4': the fourth is 0
    and gssd_unpack_conv_weight_grad drops its column).
  conv_patch_wgrad<ci,co>: 3x3 / stride 1 / pad 1 on 37 x 41 = 5 x 3 tiles, ragged both ways.  The grid is min(tiles, 256 per_cu / groups)
    workgroups per group with per_cu <= 4: groups 16 and B 5 give 75 tiles against at most 64 workgroups ('two tiles per workgroup'
    whatever the occupancy query answers).  B 1 ('one tile per workgroup') for <16,32> and <64,64>: the two extremes of how the four waves
    split output blocks against the (tap, ci tile) list -- two waves per block with 9 entries split 5 + 4, one wave per block with 36.
  wgrad_slot<gemm>: 1x1 on 67 x 63 = 4221 rows = 131 chunks of 32 + 29.  120 x 240: one tile, ragged both ways; 252 x 500: 2 x 2 tiles.
  wgrad_slot<conv>: dense 3x3, 120 outputs from 28 inputs (K 252): pad 1 and dilation 2 / pad 2 on 67 x 63; stride 2 from 131 x 129:
    66 x 65 = 4290 rows, just above the kernel's 4096.
  'window': the conv reads channels [8, 8 + groups cin_g) of rows 24 floats wider; the transform's vectors are indexed the same way.
"""

P = object()

# every template instance behind gssd_conv2d_wgrad_f32, as gssd_conv2d_wgrad_kernel_name spells it ("/plain": no fused input transform)
INSTANCES = (
    'conv_wgrad<128x128>', 'conv_wgrad<64x256>', 'conv_wgrad<32x128>', 'conv_wgrad<16x256>',
    'conv_thin_wgrad<4>', 'conv_thin_wgrad<4>/plain', 'conv_thin_wgrad<16>', 'conv_thin_wgrad<16>/plain',
    'conv_patch_wgrad<16,32>', 'conv_patch_wgrad<16,32>/plain', 'conv_patch_wgrad<32,32>', 'conv_patch_wgrad<32,32>/plain',
    'conv_patch_wgrad<32,64>', 'conv_patch_wgrad<32,64>/plain', 'conv_patch_wgrad<64,64>', 'conv_patch_wgrad<64,64>/plain',
    'wgrad_slot<gemm>', 'wgrad_slot<conv>',
)
_MT1, _MT4 = ('conv_wgrad<32x128>', 'conv_wgrad<16x256>'), ('conv_wgrad<128x128>', 'conv_wgrad<64x256>')      # scalar / b128 reads of dY
_THIN = tuple(n for n in INSTANCES if n.startswith('conv_thin_wgrad'))
_PATCH = tuple(n for n in INSTANCES if n.startswith('conv_patch_wgrad'))
# form -> groups of instances; a GPU row with the form sits on at least one instance of every group (and on no instance outside them)
FORMS = {
    'stride': (_MT1, _MT4, ('wgrad_slot<conv>',)),
    'dilation': (_MT1, _MT4, ('wgrad_slot<conv>',)),
    '1x1': (_MT1, _MT4, ('wgrad_slot<gemm>',)),
    'pad 0': (_MT1, _MT4),
    'xf': (_MT1, _MT4) + tuple((n,) for n in INSTANCES if n.startswith(('conv_thin', 'conv_patch')) and not n.endswith('/plain')),
    'window': (_MT1, _MT4, ('conv_patch_wgrad<32,64>/plain',), ('wgrad_slot<gemm>',)),
    'xf window': (_MT1, _MT4, ('conv_patch_wgrad<32,64>',)),
    'two slices': tuple((n,) for n in _MT1 + _MT4),
    'two tiles per workgroup': tuple((n,) for n in _THIN + _PATCH),
    'one tile per workgroup': (('conv_patch_wgrad<16,32>', 'conv_patch_wgrad<16,32>/plain'), ('conv_patch_wgrad<64,64>', 'conv_patch_wgrad<64,64>/plain')),
}
OTHER_FEATURES = ('name only', 'cin 3 of 4', 'dilation 6')


def G(cin, cout, H, W, B=2, groups=2, k=3, pad=1, **kw):
    """grouped k x k conv (cin / cout per group); in_stride defaults to the channels the groups read"""
    d = dict(B=B, H=H, W=W, groups=groups, cin_g=cin, in_stride=groups * cin, Cout=groups * cout, k=k, pad=pad)
    d.update(kw)
    return d


def WIN(groups, cin):
    return dict(in_ch_off=8, in_stride=groups * cin + 24)


XF = dict(in_scale=P, in_shift=P, in_pad=P)
_T16, _T32, _T64, _T128 = 'conv_wgrad<16x256>', 'conv_wgrad<32x128>', 'conv_wgrad<64x256>', 'conv_wgrad<128x128>'

ROWS = [
    # ---- csrc/conv_wgrad.hip: the four tiles, two pixel slices each ----
    ('16x256', G(12, 12, 17, 19), _T16, ('two slices',)),
    ('32x128', G(20, 36, 17, 19), _T32, ('two slices',)),
    ('64x256', G(32, 68, 17, 19), _T64, ('two slices',)),
    ('128x128', G(20, 132, 17, 19), _T128, ('two slices',)),
    # ---- its operand forms, each on a tile with scalar dY reads (MT = 1) and on one with b128 reads (MT = 4) ----
    ('32x128 stride 2', G(20, 36, 35, 39, stride=2), _T32, ('stride', 'two slices')),
    ('64x256 stride 2', G(32, 68, 35, 39, stride=2), _T64, ('stride', 'two slices')),
    ('16x256 dil 2', G(12, 12, 17, 19, pad=2, dil=2), _T16, ('dilation', 'two slices')),
    ('64x256 dil 2', G(32, 68, 17, 19, pad=2, dil=2), _T64, ('dilation', 'two slices')),
    # (dilation 6 on 17 x 19: most taps of most pixels are out of bounds)
    ('32x128 dil 6', G(20, 36, 17, 19, pad=6, dil=6), _T32, ('dilation', 'dilation 6', 'two slices')),
    ('128x128 dil 6', G(20, 132, 17, 19, pad=6, dil=6), _T128, ('dilation', 'dilation 6', 'two slices')),
    ('16x256 1x1', G(12, 12, 17, 19, k=1, pad=0), _T16, ('1x1', 'two slices')),
    ('128x128 1x1', G(20, 132, 17, 19, k=1, pad=0), _T128, ('1x1', 'two slices')),
    ('32x128 pad 0', G(20, 36, 19, 21, pad=0), _T32, ('pad 0', 'two slices')),
    ('64x256 pad 0', G(32, 68, 19, 21, pad=0), _T64, ('pad 0', 'two slices')),
    ('16x256 xf', G(12, 12, 17, 19, **XF), _T16, ('xf', 'two slices')),
    ('32x128 xf', G(20, 36, 17, 19, **XF), _T32, ('xf', 'two slices')),
    ('64x256 xf', G(32, 68, 17, 19, **XF), _T64, ('xf', 'two slices')),
    ('128x128 xf dil 6', G(20, 132, 17, 19, pad=6, dil=6, **XF), _T128, ('xf', 'dilation', 'dilation 6', 'two slices')),
    ('16x256 window', G(12, 12, 17, 19, **WIN(2, 12)), _T16, ('window', 'two slices')),
    ('64x256 window', G(32, 68, 17, 19, **WIN(2, 32)), _T64, ('window', 'two slices')),
    ('32x128 xf window', G(20, 36, 17, 19, **WIN(2, 20), **XF), _T32, ('xf window', 'two slices')),
    ('128x128 xf window', G(20, 132, 17, 19, **WIN(2, 20), **XF), _T128, ('xf window', 'two slices')),
    # name only: dense 3x3, 132 outputs, R = 4160 >= 4096.  K 180 is below the slot kernel's 192; K 216 reaches its tile-fill rule:
    # 132 / 256 x 216 / 256 = 0.44 < 0.7 -- both stay on the generic kernel
    ('128x128 dense K 180, R 4160', G(20, 132, 65, 64, B=1, groups=1), _T128, ('name only',)),
    ('128x128 dense K 216, R 4160: slot tile fill 0.44', G(24, 132, 65, 64, B=1, groups=1), _T128, ('name only',)),
    # ---- csrc/conv_thin_wgrad.hip ----
    ('thin 4 plain', G(4, 16, 70, 83, B=10, groups=4), 'conv_thin_wgrad<4>/plain', ('two tiles per workgroup', 'cin 3 of 4')),
    ('thin 4 xf', G(4, 16, 70, 83, B=10, groups=4, **XF), 'conv_thin_wgrad<4>', ('two tiles per workgroup', 'cin 3 of 4', 'xf')),
    ('thin 16 plain', G(16, 16, 70, 83, B=10, groups=4), 'conv_thin_wgrad<16>/plain', ('two tiles per workgroup',)),
    ('thin 16 xf', G(16, 16, 70, 83, B=10, groups=4, **XF), 'conv_thin_wgrad<16>', ('two tiles per workgroup', 'xf')),
    # ---- csrc/conv_patch_wgrad.hip: 75 tiles per group on at most 64 persistent workgroups ----
    ('patch 16,32 plain', G(16, 32, 37, 41, B=5, groups=16), 'conv_patch_wgrad<16,32>/plain', ('two tiles per workgroup',)),
    ('patch 16,32 xf', G(16, 32, 37, 41, B=5, groups=16, **XF), 'conv_patch_wgrad<16,32>', ('two tiles per workgroup', 'xf')),
    ('patch 32,32 plain', G(32, 32, 37, 41, B=5, groups=16), 'conv_patch_wgrad<32,32>/plain', ('two tiles per workgroup',)),
    ('patch 32,32 xf', G(32, 32, 37, 41, B=5, groups=16, **XF), 'conv_patch_wgrad<32,32>', ('two tiles per workgroup', 'xf')),
    ('patch 32,64 plain', G(32, 64, 37, 41, B=5, groups=16), 'conv_patch_wgrad<32,64>/plain', ('two tiles per workgroup',)),
    ('patch 32,64 xf', G(32, 64, 37, 41, B=5, groups=16, **XF), 'conv_patch_wgrad<32,64>', ('two tiles per workgroup', 'xf')),
    ('patch 64,64 plain', G(64, 64, 37, 41, B=5, groups=16), 'conv_patch_wgrad<64,64>/plain', ('two tiles per workgroup',)),
    ('patch 64,64 xf', G(64, 64, 37, 41, B=5, groups=16, **XF), 'conv_patch_wgrad<64,64>', ('two tiles per workgroup', 'xf')),
    ('patch 16,32 one tile each', G(16, 32, 37, 41, B=1, groups=4), 'conv_patch_wgrad<16,32>/plain', ('one tile per workgroup',)),
    ('patch 64,64 one tile each xf', G(64, 64, 37, 41, B=1, groups=4, **XF), 'conv_patch_wgrad<64,64>', ('one tile per workgroup', 'xf')),
    ('patch 32,64 window', G(32, 64, 37, 41, B=2, groups=4, **WIN(4, 32)), 'conv_patch_wgrad<32,64>/plain', ('window',)),
    ('patch 32,64 xf window', G(32, 64, 37, 41, B=2, groups=4, **WIN(4, 32), **XF), 'conv_patch_wgrad<32,64>', ('xf window',)),
    # name only: 37 x 38 = 1406 pixels are below the kernel's 1444; 16 -> 16 channels are not one of its four instances
    ('16,32 at 37 x 38', G(16, 32, 37, 38, B=5, groups=16), _T32, ('name only',)),
    ('32,32 at 37 x 38', G(32, 32, 37, 38, B=5, groups=16), _T32, ('name only',)),
    ('32,64 at 37 x 38', G(32, 64, 37, 38, B=5, groups=16), _T64, ('name only',)),
    ('64,64 at 37 x 38', G(64, 64, 37, 38, B=5, groups=16), _T64, ('name only',)),
    ('16,16 at 37 x 41', G(16, 16, 37, 41, B=5, groups=16), _T16, ('name only',)),
    # ---- csrc/wgrad_slot.hip ----
    ('slot gemm 120 x 240', G(240, 120, 67, 63, B=1, groups=1, k=1, pad=0), 'wgrad_slot<gemm>', ('1x1',)),
    ('slot gemm 252 x 500', G(500, 252, 67, 63, B=1, groups=1, k=1, pad=0), 'wgrad_slot<gemm>', ('1x1',)),
    ('slot gemm 120 x 240 window', G(240, 120, 67, 63, B=1, groups=1, k=1, pad=0, **WIN(1, 240)), 'wgrad_slot<gemm>', ('1x1', 'window')),
    ('slot conv pad 1', G(28, 120, 67, 63, B=1, groups=1), 'wgrad_slot<conv>', ()),
    ('slot conv stride 2', G(28, 120, 131, 129, B=1, groups=1, stride=2), 'wgrad_slot<conv>', ('stride',)),
    ('slot conv dil 2', G(28, 120, 67, 63, B=1, groups=1, pad=2, dil=2), 'wgrad_slot<conv>', ('dilation',)),
]

# One descriptor that is wgrad_slot<gemm> by default and a generic tile with GSSD_NO_WGRAD_SLOT=1 (the switch is read once per process: the
# CPU test asks a child process): (make_conv_desc keywords, default name, name with the switch)
SLOT_SWITCH = (G(240, 120, 67, 63, B=1, groups=1, k=1, pad=0), 'wgrad_slot<gemm>', 'conv_wgrad<64x256>')

GPU_ROWS = [r for r in ROWS if 'name only' not in r[3]]


def row_id(row):
    return row[0]


def resolve(kw, pointer):
    """the keywords with every P replaced by pointer(name)"""
    return {k: (pointer(k) if v is P else v) for k, v in kw.items()}


def geometry(kw):
    k, stride, pad, dil = kw.get('k', 1), kw.get('stride', 1), kw.get('pad', 0), kw.get('dil', 1)
    Ho = (kw['H'] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    Wo = (kw['W'] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    return k, stride, pad, dil, Ho, Wo


def patch_tiles(kw):
    """8 x 16 output tiles of a launch of the two patch-staged kernels"""
    return kw['B'] * (-(-kw['H'] // 8)) * (-(-kw['W'] // 16))


def uncovered(rows):
    """instances no GPU row expects"""
    return set(INSTANCES) - {r[2] for r in rows if 'name only' not in r[3]}
