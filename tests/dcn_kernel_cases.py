"""The case registry of the engine's deformable-conv kernels, shared by the CPU test (tests/test_dcn_kernel_cases_cpu.py) and the GPU test
(tests/test_gpu_dcn_kernels.py).  Seven entry forms implement one sampling rule -- the gate -1 < p < H, the per-corner validity, clamped
corner addresses, the table of a deformable group, the K loop over (group, channel chunk, tap) -- each with its own copy of that code:

    im2col_f32   gssd_dcn_im2col_f32                              csrc/dcn.hip
    im2col_bf16  gssd_dcn_im2col_bf16                             csrc/dcn.hip
    fused        gssd_dcn_forward_f32                             csrc/dcn_fused.hip
    x6           gssd_dcn_forward_x6_ex, flags 0                  csrc/dcn_x6.hip (three bf16 planes)
    x6_f16       gssd_dcn_forward_x6_ex, GSSD_CONV_F16_OK         csrc/dcn_x6.hip (fp16 planes)
    bf16         gssd_dcn_forward_bf16                            csrc/dcn_bf16.hip
    col2im       gssd_dcn_col2im_f32 (window + overflow kernel)   csrc/dcn.hip

A row is

    (id, family, shape keywords, features)

with the shape keywords B, H, W, C, dg, Cout, om_stride, bias (and, for the 'random' family, the offset recipe).  family 'exact': inputs for
which every kernel must return the reference's numbers bit for bit (tests/dcn_kernel_ref.py); 'random': offsets on a 1/256 grid shifted by
1/512, held against float64 within the project's ceilings; 'refused': a shape no entry accepts.

Launch arithmetic (the constants below restate the launchers; every feature a row claims is recomputed from them in the CPU module, so a
changed constant turns a row red instead of quietly emptying it).
  forward kernels (fused, x6, bf16): tiles of BM = 128 pixels x BN = 256 output channels over M = B H W flat pixels; the K loop walks, per
    deformable group, (C / dg) / BKC chunks of BKC = 32 channels x 9 taps.  x6 splits the groups over two workgroups per tile ('two parts')
    when dg is even and 2 x tiles fit the CUs -- every row here -- unless GSSD_DCN_X6_SPLITK=0.
      gates                2 x 5 x 9      M = 90: one ragged row tile; Cout 40; dg 2: two parts of one group
      gates cross images   3 x 7 x 11     M = 231 = 128 + 103: the second row tile starts at pixel 51 of image 1; Cout 264 = 256 + 8; dg 1: one part
      gates shared scalars 1 x 6 x 10     C 512, dg 4: four chunks per tap and group, two parts of two groups
      three chunks         1 x 9 x 17     C 96, dg 1: three chunks; M = 153 = 128 + 25; Cout 296 = 256 + 40
      wide groups          1 x 5 x 6      C 1024, dg 4: eight chunks per tap and group
  col2im: tiles of TH x TW = 4 x 8 pixels, an LDS window with halo DC_R = 2 ((TH + 2 DC_R + 1) x (TW + 2 DC_R + 1) corners), SLICE = 64
    channels per workgroup: a group's (C / dg) / 64 slices add into the same d(om) scalars.  A unit (pixel, tap) whose (y0, x0) corner cell
    leaves the window goes to the overflow kernel.
  im2col: a wave takes 64 consecutive units (pixel, tap, group), walked IM_UN = 4 (fp32) or 2 (bf16) at a time, at most IM_MAX_WG = 16384
    workgroups of 256 threads: a shape with more than 16384 x 256 units gives the first waves a second item.
"""

# ---- launch constants, named once ---------------------------------------------------------------------------------------------------------
BM, BN, BKC = 128, 256, 32               # csrc/dcn_fused.hip, dcn_x6.hip, dcn_bf16.hip
TH, TW, DC_R, SLICE = 4, 8, 2, 64        # csrc/dcn.hip: gssd_dcn_col2im_f32
IM_WAVE, IM_UN_F32, IM_UN_BF16 = 64, 4, 2
IM_MAX_WG, IM_THREADS = 16384, 256
NCU = 256                                # compute units of an MI355X: the x6 launcher's "2 x tiles <= CUs"

ENTRIES = ('im2col_f32', 'im2col_bf16', 'fused', 'x6', 'x6_f16', 'bf16', 'col2im')
FORWARD = ('fused', 'x6', 'x6_f16', 'bf16')
SYMBOL = {'im2col_f32': 'gssd_dcn_im2col_f32', 'im2col_bf16': 'gssd_dcn_im2col_bf16', 'fused': 'gssd_dcn_forward_f32',
          'x6': 'gssd_dcn_forward_x6_ex', 'x6_f16': 'gssd_dcn_forward_x6_ex', 'bf16': 'gssd_dcn_forward_bf16', 'col2im': 'gssd_dcn_col2im_f32'}

# the offsets of the 'exact' family (plus, per sample, whatever puts it on -1, H - 1, H - 1/2 and H of its own row: tests/dcn_kernel_ref.py)
EXACT_OFFSETS = (-1e4, -3.0, -2.0, -1.25, -1.0, -0.75, -0.25, 0.0, 0.25, 0.5, 1.0, 1.75, 2.0, 3.0, 4.0, 4.5, 5.0, 3e9)
EXACT_LOGITS = (-200.0, 0.0, 200.0)
CLOSED_OFFSETS = (-1e4, 1e4, -3e9, 3e9)

FEATURES = ('gates', 'ragged row tile', 'tiles cross images', 'second column tile', 'x6 two parts', 'x6 one part', 'slices share scalars',
            'thin', 'all closed', 'one pixel', 'bias NULL', 'om_stride padded', 'window only', 'overflow only', 'window mixed',
            'im2col second item', 'im2col ragged walk')


def S(B, H, W, C, dg, Cout, om_stride=None, bias=True, **kw):
    return dict(B=B, H=H, W=W, C=C, dg=dg, Cout=Cout, om_stride=27 * dg if om_stride is None else om_stride, bias=bias, **kw)


ROWS = [
    # ---- family 'exact': bit for bit ----
    ('gates', 'exact', S(2, 5, 9, 128, 2, 40), ('gates', 'ragged row tile', 'tiles cross images', 'x6 two parts')),
    ('gates cross images', 'exact', S(3, 7, 11, 64, 1, 264),
     ('gates', 'ragged row tile', 'tiles cross images', 'second column tile', 'x6 one part', 'im2col ragged walk')),
    ('gates shared scalars', 'exact', S(1, 6, 10, 512, 4, 8), ('gates', 'ragged row tile', 'slices share scalars', 'x6 two parts')),
    ('thin 1 x 13', 'exact', S(2, 1, 13, 64, 1, 16), ('thin', 'ragged row tile', 'tiles cross images', 'x6 one part', 'im2col ragged walk')),
    ('thin 9 x 1', 'exact', S(2, 9, 1, 64, 1, 16), ('thin', 'ragged row tile', 'tiles cross images', 'x6 one part', 'im2col ragged walk')),
    ('all closed', 'exact', S(2, 5, 9, 128, 2, 40, offsets='closed'), ('all closed', 'ragged row tile', 'tiles cross images', 'x6 two parts')),
    ('one pixel', 'exact', S(2, 8, 12, 64, 1, 16, offsets='one pixel', target=(2, 3)),
     ('one pixel', 'ragged row tile', 'tiles cross images', 'x6 one part', 'window mixed')),
    ('bias NULL', 'exact', S(1, 4, 6, 64, 1, 24, bias=False), ('bias NULL', 'ragged row tile', 'x6 one part')),
    ('om_stride 59', 'exact', S(2, 3, 7, 128, 2, 16, om_stride=27 * 2 + 5), ('om_stride padded', 'ragged row tile', 'tiles cross images', 'x6 two parts')),
    # ---- family 'random' ----
    # (std 3.0: with the 2.5 of test_dcn_col2im_backward 0.82 - 0.83 of the contributing units stay in the window on this map, outside the
    # 0.2 .. 0.8 this row is held to; 3.0 gives 0.76 - 0.77)
    ('mixed', 'random', S(2, 11, 13, 128, 2, 136, offsets='normal', std=3.0),
     ('ragged row tile', 'tiles cross images', 'x6 two parts', 'window mixed')),
    ('window only', 'random', S(2, 11, 13, 128, 2, 136, offsets='uniform', lim=0.9),
     ('ragged row tile', 'tiles cross images', 'x6 two parts', 'window only')),
    ('overflow only', 'random', S(1, 12, 16, 64, 1, 16, offsets='far', lim=4.0),
     ('ragged row tile', 'x6 one part', 'overflow only')),
    ('wide groups', 'random', S(1, 5, 6, 1024, 4, 16, offsets='normal', std=1.5),
     ('ragged row tile', 'slices share scalars', 'x6 two parts', 'window mixed')),
    ('three chunks, Cout tail', 'random', S(1, 9, 17, 96, 1, 296, offsets='normal', std=1.5),
     ('ragged row tile', 'second column tile', 'x6 one part', 'im2col ragged walk')),
    ('im2col second item', 'random', S(2, 300, 400, 8, 2, 8, offsets='normal', std=1.5), ('im2col second item',)),
    # ---- a shape every entry refuses: C / dg = 18 is no multiple of 4 (im2col), of 32 (forward) or of 64 (col2im) ----
    ('C 36 dg 2', 'refused', S(1, 3, 4, 36, 2, 16), ()),
]

# the figures the docstring quotes: row id -> (M, row tiles, channels of the last column tile, chunks per tap and group, col2im slices per group)
FIGURES = {
    'gates': (90, 1, 40, 2, 1),
    'gates cross images': (231, 2, 8, 2, 1),
    'gates shared scalars': (60, 1, 8, 4, 2),
    'three chunks, Cout tail': (153, 2, 40, 3, None),
    'wide groups': (30, 1, 16, 8, 4),
}


def row_id(row):
    return row[0]


def of_family(*families):
    return [r for r in ROWS if r[1] in families]


def by_id(rid):
    return next(r for r in ROWS if r[0] == rid)


def eligible(entry, kw):
    """The GSSD_CHECK_ARG lines of the entry's launcher, restated: True when the launcher accepts the shape."""
    C, dg, Cout = kw['C'], kw['dg'], kw['Cout']
    if kw['om_stride'] < 27 * dg:
        return False
    if entry in ('im2col_f32', 'im2col_bf16'):
        return C % (4 * dg) == 0 and kw['B'] * kw['H'] * kw['W'] * 9 * C < 2 ** 31
    if C % dg != 0:
        return False
    if entry == 'col2im':
        return (C // dg) % SLICE == 0
    ok = (C // dg) % BKC == 0
    if entry == 'fused':
        return ok
    assert entry in ('x6', 'x6_f16', 'bf16'), entry
    return ok and Cout % 8 == 0


def refused_text(entry):
    """a piece of the failed condition the launcher names when it refuses the 'refused' row"""
    return {'im2col_f32': 'C % (4 * dg) == 0', 'im2col_bf16': 'C % (4 * dg) == 0', 'col2im': '(C / dg) % 64 == 0'}.get(entry, '(C / dg) % BKC == 0')


def cases(*families, entries=ENTRIES):
    """(row, entry) for every entry form the launcher accepts the row for; 'im2col second item' is the im2col entries' alone"""
    out = []
    for r in of_family(*families):
        for e in entries:
            if eligible(e, r[2]) and ('im2col second item' not in r[3] or e.startswith('im2col')):
                out.append((r, e))
    return out


def case_id(c):
    row, entry = c
    return f'{row[1]}-{row[0]}-{entry}'.replace(' ', '_')


# ---- launch arithmetic ------------------------------------------------------------------------------------------------------------------------
def forward_tiles(kw):
    """(M, row tiles, column tiles, channels of the last column tile, chunks per tap and group)"""
    M = kw['B'] * kw['H'] * kw['W']
    ntn = -(-kw['Cout'] // BN)
    return M, -(-M // BM), ntn, kw['Cout'] - (ntn - 1) * BN, kw['C'] // kw['dg'] // BKC


def tiles_cross_images(kw):
    """a row tile holds pixels of two images"""
    M, mt, _, _, _ = forward_tiles(kw)
    HW = kw['H'] * kw['W']
    return any(k * BM // HW != (min((k + 1) * BM, M) - 1) // HW for k in range(mt))


def x6_parts(kw):
    M, mt, ntn, _, _ = forward_tiles(kw)
    return 2 if kw['dg'] % 2 == 0 and mt * ntn * 2 <= NCU else 1


def col2im_grid(kw):
    """(tiles_y, tiles_x, slices per group, window height, window width)"""
    return -(-kw['H'] // TH), -(-kw['W'] // TW), kw['C'] // kw['dg'] // SLICE, TH + 2 * DC_R + 1, TW + 2 * DC_R + 1


def im2col_walk(kw):
    """(units, units a launch covers in one pass, units of the last wave's item)"""
    units = kw['B'] * kw['H'] * kw['W'] * 9 * kw['dg']
    wg = min(-(-units // IM_THREADS), IM_MAX_WG)
    return units, wg * IM_THREADS, units % IM_WAVE or IM_WAVE
