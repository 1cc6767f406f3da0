"""Constants, switches and the small value types shared by the forward engine's modules (gssd/engine.py and its mixins plan_graph / plan_ops /
plan_exec): the layer tables of models/ssd_multiphase_custom_group.py:434-490, the GSSD_* environment switches, the step / tag records."""
import ctypes as C
import os
from . import _lib
from ._lib import lib

VGG_CFG = [64, 64, 'M', 128, 128, 'M', 256, 256, 256, 'C', 512, 512, 512, 'M', 512, 512, 512]
EXTRAS_CFG = [256, 'S', 512, 128, 'S', 256, 128, 256, 128, 256]
MBOX = [4, 6, 6, 6, 4, 4]
SRC_HW = [38, 19, 10, 5, 3, 1]
HEAD_OFF = [sum(h * h * a for h, a in zip(SRC_HW[:i], MBOX[:i])) for i in range(6)]      # first prior of source i
FUSE_NAMES = ['11', '21', '31', '41', '51', '61']


# Winograd F(2x2,3x3) for the compute-bound 3x3 trunk layers (csrc/conv_wino.hip); GSSD_NO_WINOGRAD=1 keeps the direct
# implicit GEMM everywhere (ablation / cross-check).
USE_HEADS_WINO = os.environ.get('GSSD_HEADS_WINO', '1') != '0'  # the 38 x 38 multibox head of a train-mode fp32 forward on csrc/conv_wino_x6.hip
USE_PATCH_X6 = os.environ.get('GSSD_PATCH_X6', '1') != '0'    # csrc/conv_patch_x6.hip for the DCN offset conv of a train-mode fp32 forward
USE_CONV_X6 = os.environ.get('GSSD_CONV_X6', '1') != '0'      # csrc/conv_x6.hip for the launches ops.x6_wanted names (fp32 mode)
USE_WINOGRAD = os.environ.get('GSSD_NO_WINOGRAD', '0') != '1'
# fp32 mode: the deformable conv on the bf16 matrix cores with three-plane (fp32-equivalent) operands, csrc/dcn_x6.hip;
# GSSD_DCN_X6=0: the fp32-MFMA kernel csrc/dcn_fused.hip
DCN_X6 = os.environ.get('GSSD_DCN_X6', '1') != '0'
# GSSD_NO_GRAPH=1 keeps every forward an eager list of launches (debugging / ablation)
USE_GRAPH = os.environ.get('GSSD_NO_GRAPH', '0') != '1'
# GSSD_FLASH_X6=0: the fp32-MFMA attention core (csrc/flash_attn.hip) keeps every launch of the fp32 mode (ablation / A-B)
USE_FLASH_X6 = os.environ.get('GSSD_FLASH_X6', '1') != '0'
# GSSD_NO_BRANCH_STREAMS=1 captures the plan as one serial chain (ablation)
USE_BRANCH_STREAMS = os.environ.get('GSSD_NO_BRANCH_STREAMS', '0') != '1'
# conv1_1 of a no-backward fp32 plan reads the caller's NCHW batch itself (csrc/conv_thin.hip, GSSD_CONV_IN_NCHW3): no gssd_pack_input_nhwc
# launch and no packed copy; GSSD_FUSE_PACK=0 keeps the pack launch (A-B in the same build)
FUSE_PACK = os.environ.get('GSSD_FUSE_PACK', '1') != '0'
# the o conv of Self_Attn-base 0 in a no-backward fp32 plan writes its two outputs straight into the per-group concatenation the DCN reads
# (csrc/conv_x6.hip, GSSD_CONV_OUT_GROUPCAT): no gssd_slice_and_cat_f32 launch; GSSD_FUSE_CAT=0 keeps the copy pass
FUSE_CAT = os.environ.get('GSSD_FUSE_CAT', '1') != '0'
# the merged theta | phi | g projection of a 38 x 38 Self_Attn block in a no-backward fp32 plan stores the attention core's bf16 planes itself
# (csrc/conv_x6.hip, GSSD_CONV_OUT_X6PLANES) and the core runs its second pass only (gssd_self_attn_core_x6_planes_f32): no split_planes
# launches, no fp32 theta | phi / g^T arrays; GSSD_FUSE_SPLIT=0 keeps the two-pass entry
FUSE_SPLIT = os.environ.get('GSSD_FUSE_SPLIT', '1') != '0'
# conv4_3's BatchNorm + ReLU pass of a no-backward fp32 plan with Self_Attn-base on: its two readers -- the block's projection (in_scale / in_shift)
# and the residual read of the block's o conv (GSSD_CONV_RESID_XF, csrc/conv_x6.hip) -- apply it on read;
# GSSD_FUSE_SA_BN=0 keeps the pass
FUSE_SA_BN = os.environ.get('GSSD_FUSE_SA_BN', '1') != '0'
# the BatchNorm + ReLU passes behind the fuse convs with <= 512 output channels of a no-backward fp32 plan: each one's only reader is its merged
# loc | conf head conv, which applies it on read (in_scale / in_shift / in_pad); GSSD_FUSE_HEAD_BN=0 keeps the passes
FUSE_HEAD_BN = os.environ.get('GSSD_FUSE_HEAD_BN', '1') != '0'
# the split-K slices of the loc and the conf heads are added by ONE launch (csrc/elementwise.hip, gssd_heads_reduce2_f32: the same sums in the
# same order); GSSD_FUSE_HEADS_REDUCE=0 keeps one gssd_heads_reduce_f32 launch per head
FUSE_HEADS_REDUCE = os.environ.get('GSSD_FUSE_HEADS_REDUCE', '1') != '0'
SN_STREAM = 9               # stream id of the spectral-norm launch inside a captured graph
ALL_STREAMS = -1            # _Step.wait value: join every forked stream before this step

class Tag(tuple):
    """(kernel instance, algorithmic FLOPs, algorithmic bytes) of one launch; ``layer`` names the module it belongs to
    ('vgg.0' = conv1_1 ... 'vgg.40' = conv5_3) so bench.py can sum the trunk's launches -- convs AND their BatchNorm passes."""
    layer = None


class _Step:
    __slots__ = ('fn', 'args', 'keep', 'tag', 'sid', 'wait')

    def __init__(self, fn, args, keep=None, tag=None, sid=0, wait=None):
        # sid: stream id inside a captured graph (0 = trunk);  wait: a stream id whose work this step consumes (joined before it)
        self.fn, self.args, self.keep, self.tag, self.sid, self.wait = fn, args, keep, tag, sid, wait


def conv_cost(name, d):
    """(algorithmic FLOPs, algorithmic bytes) of the conv launch ``name`` runs for descriptor ``d``."""
    M = d.B * d.Ho * d.Wo
    if name.startswith('conv_patch_x6<'):
        return 2.0 * M * d.Cout * 9 * d.cin_g, 4.0 * (d.B * d.H * d.W * d.cin_g + M * d.Cout + d.Cout * 9 * d.cin_g)
    if name.startswith('conv_x6<'):
        return (2.0 * M * d.Cout * d.KH * d.KW * d.cin_g,
                4.0 * (d.B * d.H * d.W * d.cin_g * d.groups + M * d.Cout + d.Cout * d.KH * d.KW * d.cin_g))
    cin_g = 3 if (d.cin_g in (4, 8) and d.groups == 4 and d.H == 300) else d.cin_g       # conv1_1: 3 real channels per group in 4 / 8 stored
    esz = 2.0 if '_bf16<' in name else 4.0                                               # (every kernel of the bf16 entry point is named so)
    out_elems = M * d.Cout // 4 if (d.flags & _lib.CONV_POOL2) else M * d.Cout           # pooled raw output: a quarter of the map
    return 2.0 * M * d.Cout * d.KH * d.KW * cin_g, esz * (d.B * d.H * d.W * cin_g * d.groups + out_elems + d.Cout * d.KH * d.KW * cin_g)


def conv_tag(d, bf16=False):
    """(kernel instance, algorithmic FLOPs, algorithmic bytes) of one gssd_conv2d launch.  The name is the dispatcher's own statement
    (gssd_conv2d_kernel_name walks the launch path and names the template instance it arrives at; rocprofv3's kernel symbols carry the same
    arguments); a descriptor the entry point would refuse raises GssdError."""
    buf = C.create_string_buffer(64)
    _lib.check(lib.gssd_conv2d_kernel_name(C.byref(d), int(bf16), buf, len(buf)))
    name = buf.value.decode()
    return (name,) + conv_cost(name, d)
