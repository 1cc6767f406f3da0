"""The case registry of the streaming backward passes of csrc/backward.hip, shared by the CPU test (tests/test_bwd_pass_ref_cpu.py) and the
GPU test (tests/test_gpu_bwd_passes.py): BatchNorm(train) + ReLU + max-pool backward (gssd_bn_bwd_reduce_* -> gssd_bn_bwd_finalize_f32 ->
gssd_bn_bwd_apply_*), gssd_colsum_f32, gssd_l2norm_bwd_f32, gssd_upsample_insert_f32 and gssd_heads_gather_f32.  A row is

    (id, kind, shape and form keywords, features)

in the style of tests/wgrad_leaf_cases.py.  kind picks the sequence of entry points (SEQUENCES / ENTRIES_OF) the GPU test runs for the row.

Launch arithmetic (the constants below restate the launchers of csrc/backward.hip; every 'grid' feature is computed from them in
tests/test_bwd_pass_ref_cpu.py, so a changed cap turns a row red instead of quietly emptying it).
  BatchNorm passes: nblocks_wide = min(ceil(total / 1024), 512) workgroups of 1024 threads over total = pixels x C / 4 float4 items (the
    pooled reduce: pooled pixels); stride = floor(T / C4) C4 with T = workgroups x 1024, the T - stride threads behind it idle.  A thread
    runs the BN_UNR = 2 unrolled body when total > stride, the body and then the single-step tail when total > 2 stride.
      one quad        1 x 3 x 2 x 4       C4 = 1; 6 items
      idle threads    2 x 5 x 7 x 12      C4 = 3: 210 items, stride 1023 of 1024 threads;  x 100: C4 = 25, 1750 items, stride 2025 of 2048
      widest          1 x 3 x 3 x 4096    C4 = 1024 = one workgroup; LDS 2 x 4096 floats
      second item     2 x 150 x 150 x 64  720 000 items = 1.37 x 524 288: no unrolled pair, a tail step for the first 195 712 threads
      unrolled + tail 2 x 420 x 420 x 12  1 058 400 items = 2.019 x 524 286 (two idle threads): the unrolled pair, then the tail for the first 9 828
      pool grid       1 x 840 x 840 x 12, (2, 2, 0): 529 200 pooled items = 1.009 x 524 286: a second iteration of the pooled loop at C4 = 3
    (the 150, 420, 840, 3 and 50 maps are square because their item counts are what the row is for; every other map is non-square).
  Pools (k, s, p, ceil): (2, 2, 0) on 6 x 10 covers the map; on 7 x 5 with ceil the last windows hang over the border (4 x 3 outputs); on
    7 x 5 without ceil (3 x 2 outputs) the last row and the last column are in NO window: d there is 0, draw = B raw + C.  (3, 1, 1) and
    (3, 2, 1) on 5 x 7: overlapping windows cut by all four borders, atomics into a zeroed dz.
  gssd_colsum_f32: min(ceil(rows C / 1024), 128) workgroups, gstride = floor(T / C) C.  5776 x 24 (a 38 x 38 head at batch 4): 138 624
    elements = 1.058 x 131 064, 8 idle threads.
  gssd_l2norm_bwd_f32: one wave per pixel, at most 1024 workgroups of 4 waves = 4096 waves; lane l takes quads l, l + 64, ..
  gssd_upsample_insert_f32 / gssd_heads_gather_f32: at most 2048 workgroups of 256 threads = 524 288, one float4 / one float per item.
"""

# ---- launch constants of csrc/backward.hip, named once -------------------------------------------------------------------------------
WIDE = 1024              # threads of a workgroup of the BatchNorm passes and of gssd_colsum_f32
BN_MAX_WG = 512          # nblocks_wide(items): cap 2048 / 4
COLSUM_MAX_WG = 128      # nblocks_wide(items, 512): cap 512 / 4
COPY_MAX_WG, COPY_THREADS = 2048, 256          # nblocks(items): gssd_upsample_insert_f32, gssd_heads_gather_f32
L2_MAX_WG, L2_THREADS, WAVE = 1024, 256, 64    # nblocks(pixels * 64, 1024): gssd_l2norm_bwd_f32
BN_UNR = 2
MAX_C = 4096

ENTRIES = ('gssd_bn_bwd_reduce_f32', 'gssd_bn_bwd_reduce_mixed', 'gssd_bn_bwd_finalize_f32', 'gssd_bn_bwd_apply_f32',
           'gssd_bn_bwd_apply_masked_f32', 'gssd_bn_bwd_apply_mixed', 'gssd_colsum_f32', 'gssd_l2norm_bwd_f32',
           'gssd_upsample_insert_f32', 'gssd_heads_gather_f32')

# the forms of section "BatchNorm backward" / "Mixed entries": each sits on at least one row (test_registry_closes_over_entries_and_forms)
FORMS = ('plan/no-pool', 'plan/pool', 'helper', 'C4 = 1', 'widest', 'pool even', 'pool ceil odd', 'pool floor odd', 'pool overlap',
         'pool stride 2 overlap', 'no affine', 'relu, no pool', 'pool only', 'relu + pool', 'bf16 dout', 'fp32 dout', 'dz_bf16 hand-over',
         'store_f32 = 0', 'dz16', 'row stride', 'dx_add', 'zero tail', 'exact fit', 's = 3', 'prior_off = 0', 'prior_off at end', 'nc 3', 'A 6')
# properties of the launch arithmetic, recomputed from the constants above
GRID = ('second item', 'unrolled + tail', 'idle threads', 'pool second item', 'colsum second item', 'second pixel', 'lane loops twice',
        'one lane', 'copy second item')
SQUARE_BY_SPEC = ('second item', 'unrolled + tail', 'pool second item', 'widest', 'second pixel', 'copy second item')
# reference-sensitivity tags: the float64 restatement, made wrong in one way, must move by far more than the gate (CPU only)
SENSITIVE = ('sensitive: last maximum', 'sensitive: uncovered')


def BN(B, H, W, C, pool=None, relu=True, **kw):
    """pool = (k, s, p, ceil) or None"""
    return dict(B=B, H=H, W=W, C=C, pool=pool, relu=relu, **kw)


_P220, _P220C, _P311, _P321 = (2, 2, 0, False), (2, 2, 0, True), (3, 1, 1, False), (3, 2, 1, False)

ROWS = [
    # ---- BatchNorm backward, fp32 entries: every row runs its plan sequence and the helper against ONE reference ----
    ('one quad', 'bn', BN(1, 3, 2, 4), ('C4 = 1', 'plan/no-pool', 'helper')),
    ('idle threads C 12', 'bn', BN(2, 5, 7, 12), ('idle threads', 'plan/no-pool', 'helper')),
    ('idle threads C 100', 'bn', BN(2, 5, 7, 100), ('idle threads', 'plan/no-pool', 'helper')),
    ('widest', 'bn', BN(1, 3, 3, 4096), ('widest', 'plan/no-pool', 'helper')),
    ('second item', 'bn', BN(2, 150, 150, 64), ('second item', 'plan/no-pool', 'helper')),
    ('unrolled + tail', 'bn', BN(2, 420, 420, 12), ('unrolled + tail', 'idle threads', 'plan/no-pool', 'helper')),
    ('pool even', 'bn', BN(2, 6, 10, 12, _P220, ties=True), ('pool even', 'idle threads', 'plan/pool', 'helper', 'sensitive: last maximum')),
    ('pool ceil odd', 'bn', BN(1, 7, 5, 8, _P220C), ('pool ceil odd', 'plan/pool', 'helper')),
    ('pool floor odd', 'bn', BN(2, 7, 5, 8, _P220), ('pool floor odd', 'plan/pool', 'helper', 'sensitive: uncovered')),
    ('pool overlap', 'bn', BN(2, 5, 7, 12, _P311, ties=True), ('pool overlap', 'idle threads', 'plan/pool', 'helper', 'sensitive: last maximum')),
    ('pool overlap stride 2', 'bn', BN(2, 5, 7, 12, _P321), ('pool overlap', 'pool stride 2 overlap', 'idle threads', 'plan/pool', 'helper')),
    ('pool grid', 'bn', BN(1, 840, 840, 12, _P220), ('pool second item', 'idle threads', 'plan/pool', 'helper')),
    # ---- scale = shift = NULL, sums = NULL: gssd_bn_bwd_reduce_f32 as bwd_ops._convrelu / _pool / _relupool launch it (bit-exact) ----
    ('no affine relu', 'noaffine', BN(2, 5, 7, 12), ('no affine', 'relu, no pool', 'idle threads')),
    ('no affine relu C 100', 'noaffine', BN(2, 5, 7, 100), ('no affine', 'relu, no pool', 'idle threads')),
    ('no affine pool', 'noaffine', BN(1, 7, 5, 8, _P220C, relu=False), ('no affine', 'pool only', 'pool ceil odd')),
    ('no affine relu + pool', 'noaffine', BN(1, 7, 5, 8, _P220C), ('no affine', 'relu + pool', 'pool ceil odd')),
    ('no affine pool floor odd', 'noaffine', BN(2, 7, 5, 8, _P220, relu=False), ('no affine', 'pool only', 'pool floor odd')),
    # ---- gssd_bn_bwd_reduce_mixed / gssd_bn_bwd_apply_mixed on bf16-representable raw, fp32 and bf16 d(out) ----
    ('mixed idle threads', 'mixed', BN(2, 5, 7, 12, dout_bf16=False), ('idle threads', 'fp32 dout', 'dz16', 'store_f32 = 0')),
    ('mixed idle threads bf16', 'mixed', BN(2, 5, 7, 12, dout_bf16=True), ('idle threads', 'bf16 dout', 'dz16', 'store_f32 = 0')),
    ('mixed unrolled + tail', 'mixed', BN(2, 420, 420, 12, dout_bf16=False), ('unrolled + tail', 'idle threads', 'fp32 dout', 'dz16', 'store_f32 = 0')),
    ('mixed unrolled + tail bf16', 'mixed', BN(2, 420, 420, 12, dout_bf16=True), ('unrolled + tail', 'idle threads', 'bf16 dout', 'dz16', 'store_f32 = 0')),
    ('mixed pool even', 'mixed', BN(2, 6, 10, 12, _P220, dout_bf16=False), ('pool even', 'idle threads', 'fp32 dout', 'dz16', 'dz_bf16 hand-over')),
    ('mixed pool even bf16', 'mixed', BN(2, 6, 10, 12, _P220, dout_bf16=True), ('pool even', 'idle threads', 'bf16 dout', 'dz16', 'dz_bf16 hand-over')),
    ('mixed pool floor odd', 'mixed', BN(2, 7, 5, 8, _P220, dout_bf16=False), ('pool floor odd', 'fp32 dout', 'dz16', 'dz_bf16 hand-over')),
    ('mixed pool floor odd bf16', 'mixed', BN(2, 7, 5, 8, _P220, dout_bf16=True), ('pool floor odd', 'bf16 dout', 'dz16', 'dz_bf16 hand-over')),
    ('mixed pool overlap', 'mixed', BN(2, 5, 7, 12, _P311, dout_bf16=False), ('pool overlap', 'idle threads', 'fp32 dout', 'dz16')),
    ('mixed pool overlap bf16', 'mixed', BN(2, 5, 7, 12, _P311, dout_bf16=True), ('pool overlap', 'idle threads', 'bf16 dout', 'dz16')),
    # ---- gssd_colsum_f32: rows x C (row stride) ----
    ('colsum 5776 x 24', 'colsum', dict(rows=5776, C=24, stride=24), ('colsum second item', 'idle threads')),
    ('colsum 700 x 27 stride 32', 'colsum', dict(rows=700, C=27, stride=32), ('row stride', 'idle threads')),
    ('colsum 3 x 4096', 'colsum', dict(rows=3, C=4096, stride=4096), ('widest',)),
    ('colsum 1 x 1', 'colsum', dict(rows=1, C=1, stride=1), ()),
    # ---- gssd_l2norm_bwd_f32 ----
    ('l2norm C 4', 'l2norm', dict(B=2, H=3, W=5, C=4, dx_add=False), ('one lane',)),
    ('l2norm C 260', 'l2norm', dict(B=1, H=3, W=5, C=260, dx_add=False), ('lane loops twice',)),
    ('l2norm C 512 dx_add', 'l2norm', dict(B=2, H=3, W=5, C=512, dx_add=True), ('dx_add', 'lane loops twice')),
    ('l2norm 5000 pixels', 'l2norm', dict(B=2, H=50, W=50, C=8, dx_add=False), ('second pixel',)),
    # ---- gssd_upsample_insert_f32 (bit-exact) ----
    ('upsample exact fit', 'upsample', dict(B=2, Ho=5, Wo=7, s=2, H=9, W=13, C=8), ('exact fit',)),
    ('upsample zero tail', 'upsample', dict(B=2, Ho=5, Wo=7, s=2, H=10, W=14, C=8), ('zero tail',)),
    ('upsample s 3', 'upsample', dict(B=1, Ho=4, Wo=3, s=3, H=10, W=9, C=4), ('s = 3', 'C4 = 1', 'exact fit', 'zero tail')),
    ('upsample 720 000 quads', 'upsample', dict(B=2, Ho=75, Wo=75, s=2, H=150, W=150, C=64), ('copy second item', 'zero tail')),
    # ---- gssd_heads_gather_f32 (bit-exact) ----
    ('gather nc 2 A 4', 'gather', dict(B=2, HW=15, A=4, nc=2, P=100, off=0), ('prior_off = 0',)),
    ('gather nc 3 A 6', 'gather', dict(B=2, HW=15, A=6, nc=3, P=150, off=60), ('nc 3', 'A 6', 'prior_off at end')),
    ('gather 554 496 elements', 'gather', dict(B=16, HW=1444, A=4, nc=2, P=8732, off=0), ('copy second item', 'prior_off = 0')),
]

# the sequences of a 'bn' row, as gssd/bwd_ops.py::_convbn and gssd/ops.py::bn_backward launch them
SEQUENCES = {
    'plan/no-pool': ('gssd_bn_bwd_reduce_f32', 'gssd_bn_bwd_finalize_f32', 'gssd_bn_bwd_apply_masked_f32'),      # reduce: sums only, dz = NULL
    'plan/pool': ('gssd_bn_bwd_reduce_f32', 'gssd_bn_bwd_finalize_f32', 'gssd_bn_bwd_apply_f32'),                # reduce writes dz
    'helper': ('gssd_bn_bwd_reduce_f32', 'gssd_bn_bwd_finalize_f32', 'gssd_bn_bwd_apply_f32'),                   # ops.bn_backward
}
ENTRIES_OF = {
    'noaffine': ('gssd_bn_bwd_reduce_f32',),
    'mixed': ('gssd_bn_bwd_reduce_mixed', 'gssd_bn_bwd_finalize_f32', 'gssd_bn_bwd_apply_mixed'),
    'colsum': ('gssd_colsum_f32',), 'l2norm': ('gssd_l2norm_bwd_f32',), 'upsample': ('gssd_upsample_insert_f32',),
    'gather': ('gssd_heads_gather_f32',),
}


def row_id(row):
    return row[0]


def of_kind(*kinds):
    return [r for r in ROWS if r[1] in kinds]


def entries_of(row):
    _, kind, _, feats = row
    if kind == 'bn':
        return tuple(e for s in SEQUENCES if s in feats for e in SEQUENCES[s])
    return ENTRIES_OF[kind]


def pool_out(n, k, s, p, ceil):
    """output extent of a max-pool, torch's rule (the last window of ceil mode has to start inside the map or its left padding)"""
    if ceil:
        o = -(-(n + 2 * p - k) // s) + 1
        return o - 1 if (o - 1) * s >= n + p else o
    return (n + 2 * p - k) // s + 1


def out_extent(kw):
    if not kw['pool']:
        return kw['H'], kw['W']
    k, s, p, ceil = kw['pool']
    return pool_out(kw['H'], k, s, p, ceil), pool_out(kw['W'], k, s, p, ceil)


def uncovered(kw):
    """number of pixels of one image that lie in no pool window (0 without a pool)"""
    if not kw['pool']:
        return 0
    k, s, p, _ = kw['pool']
    Ho, Wo = out_extent(kw)
    ys = {y for o in range(Ho) for y in range(o * s - p, o * s - p + k) if 0 <= y < kw['H']}
    xs = {x for o in range(Wo) for x in range(o * s - p, o * s - p + k) if 0 <= x < kw['W']}
    return kw['H'] * kw['W'] - len(ys) * len(xs)


def wide_grid(total, C4, max_wg=BN_MAX_WG):
    """(workgroups, stride, idle threads, items of the busiest thread) of a nblocks_wide launch over ``total`` items in groups of C4"""
    wg = max(1, min(-(-total // WIDE), max_wg))
    stride = wg * WIDE // C4 * C4
    return wg, stride, wg * WIDE - stride, -(-total // stride)


def bn_grids(kw):
    """the launches of a BatchNorm row: (reduce, apply) as wide_grid tuples with their totals in front"""
    C4 = kw['C'] // 4
    Ho, Wo = out_extent(kw)
    red, app = kw['B'] * Ho * Wo * C4, kw['B'] * kw['H'] * kw['W'] * C4
    return (red,) + wide_grid(red, C4), (app,) + wide_grid(app, C4)


def copy_threads():
    return COPY_MAX_WG * COPY_THREADS


def l2_waves(pixels):
    return max(1, min(-(-pixels * WAVE // L2_THREADS), L2_MAX_WG)) * (L2_THREADS // WAVE)
