"""Restatement of PixelLink.forward for pixel_link_config version "2s" (ssd_liverdet/pixel_link/model.py:189-383 with the 2s branches) and
the seeded inputs of the 2s loss / decoding fixtures.  TEST INFRASTRUCTURE ONLY.

``pixellink2s_forward`` runs in the dtype of its inputs (the tests call it in float64); it is pinned against the imported reference by
tests/golden/pixellink2s.npz (tests/test_pixellink2s_cpu.py).  It reuses the pinned operators of oracle/gssd_oracle.py (Self_Attn,
BatchNorm) and the trunk of oracle/pixellink_oracle.py.  Version "2s" is defined only without DCN layers: the reference fails there.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import gssd_oracle as O
from oracle import pixellink_oracle as PO

PLAIN = dict(cascade_fuse=True, use_fuseconv=True, batch_norm=True, use_self_attention=False, use_self_attention_base=False,
             num_dcn_layers=0, groups_dcn=1, dcn_cat_sab=False, detach_sab=False)
SA = dict(PLAIN, use_self_attention=True, use_self_attention_base=True)
VARIANTS = {
    'plain': (PLAIN, 1),
    'sa': (SA, 1),
    'sapool': (SA, 2),
    'nocascade': (dict(PLAIN, cascade_fuse=False, use_fuseconv=False, batch_norm=False), 1),
}


def pixellink2s_forward(sd, x, cascade_fuse=True, use_fuseconv=True, batch_norm=True, use_self_attention=False,
                        use_self_attention_base=False, num_dcn_layers=0, groups_dcn=1, dcn_cat_sab=False, detach_sab=False,
                        max_pool_factor=1, training=True):
    """-> (out_1 [B,2,150,150], out_2 [B,16,150,150], buffer updates)."""
    assert num_dcn_layers == 0, 'version "2s" is defined without DCN layers'
    updates = {}
    sab, sa = [0], [0]

    def sa_base(x):
        if not use_self_attention_base:
            return x
        out, _, _ = O.self_attn(x, sd, f'self_attn_base_list.{sab[0]}', training, max_pool_factor, updates)
        sab[0] += 1
        return out

    def stage_out(s, k):
        if use_self_attention:
            s, _, _ = O.self_attn(s, sd, f'self_attn_list.{sa[0]}', training, max_pool_factor, updates)
            sa[0] += 1
        if use_fuseconv:
            s = F.conv2d(s, sd[f'fuse{k}.weight'], sd[f'fuse{k}.bias'])
            if batch_norm:
                s = O._bn(s, sd, f'bn_fuse{k}', training, updates)
        return (F.conv2d(s, sd[f'out{k}_1.weight'], sd[f'out{k}_1.bias']),
                F.conv2d(s, sd[f'out{k}_2.weight'], sd[f'out{k}_2.bias']))

    for (n, _, _, _) in PO._STAGES[0]:
        x = PO._conv_relu(x, sd, n)
    x = F.max_pool2d(x, 2, ceil_mode=True)                                 # pool1
    for (n, _, _, _) in PO._STAGES[1]:
        x = PO._conv_relu(x, sd, n)
    x = sa_base(x)                                                         # :200-212 (2s): stage 1 on relu2_2, before pool2
    l1 = stage_out(x, 1)
    x = F.max_pool2d(x, 2, ceil_mode=True)                                 # pool2
    for (n, _, _, _) in PO._STAGES[2]:
        x = PO._conv_relu(x, sd, n)
    x = sa_base(x)                                                         # (no DCN after conv3_3 in 2s, :232)
    l2 = stage_out(x, 2)
    x = F.max_pool2d(x, 2, ceil_mode=True)                                 # pool3
    for (n, _, _, _) in PO._STAGES[3]:
        x = PO._conv_relu(x, sd, n)
    x = sa_base(x)
    l3 = stage_out(x, 3)
    x = F.max_pool2d(x, 2, ceil_mode=True)                                 # pool4
    for (n, _, _, _) in PO._STAGES[4]:
        x = PO._conv_relu(x, sd, n)
    x = sa_base(x)
    l4 = stage_out(x, 4)
    x = F.max_pool2d(x, 3, 1, 1, ceil_mode=True)                           # pool5
    x = PO._conv_relu(x, sd, 'conv6', pad=6, dil=6)
    x = PO._conv_relu(x, sd, 'conv7', pad=0)
    x = sa_base(x)
    l5 = stage_out(x, 5)
    outs = []
    for j, fin in ((0, 'final_1'), (1, 'final_2')):
        u1 = up(l5[j] + l4[j], l3[j].shape[2:])                            # :306-356 / :357-383
        u2 = up(u1 + l3[j], l2[j].shape[2:])
        u3 = up(u2 + l2[j], l1[j].shape[2:])
        logit = u3 + l1[j]
        if cascade_fuse:
            size = logit.shape[2:]
            feats = [up(l5[j], size), up(l5[j] + l4[j], size), up(u1 + l3[j], size), up(u2 + l2[j], size), logit]
            outs.append(F.conv2d(torch.cat(feats, 1), sd[fin + '.weight'], sd[fin + '.bias']))
        else:
            outs.append(F.conv2d(logit, sd[fin + '.weight'], sd[fin + '.bias']))
    return outs[0], outs[1], updates


def up(t, size):
    return F.interpolate(t, size=size, mode='bilinear', align_corners=True)


def loss_inputs(seed, B=3, H=150):
    """Seeded PixelLinkLoss inputs: boxes of positives, an image without any positive pixel (the r_pos == 0 branch), and exact ties at
    the OHEM threshold (logits on a coarse grid, so many background probabilities are equal)."""
    rng = np.random.default_rng(seed)
    out_1 = rng.normal(0, 2.0, size=(B, 2, H, H)).astype(np.float32)
    out_1[0] = np.round(out_1[0] * 2.0) / 2.0                             # image 0: logits on a 0.5 grid -> many equal probabilities
    out_2 = rng.normal(0, 2.0, size=(B, 16, H, H)).astype(np.float32)
    pix = np.zeros((B, H, H), np.int64)
    for b in range(B - 1):                                                 # the last image has no positive pixel
        for _ in range(3 + b):
            y, x, h, w = rng.integers(5, H - 25), rng.integers(5, H - 25), rng.integers(3, 20), rng.integers(3, 20)
            pix[b, y:y + h, x:x + w] = 1
    neg = ((pix == 0) & (rng.random((B, H, H)) > 0.1)).astype(np.uint8)
    posw = (pix * rng.uniform(0.5, 2.0, size=(B, H, H))).astype(np.float32)
    link = (rng.random((B, 8, H, H)) > 0.4).astype(np.int64) * pix[:, None]
    return out_1, out_2, pix, neg, posw, link


def decode_inputs(seed, B=3, H=150):
    """Seeded score maps for the link decoding: blobs of positives, links on / off at random."""
    rng = np.random.default_rng(seed)
    d1 = rng.normal(0, 1.0, size=(B, 2, H, H)).astype(np.float32)
    blob = rng.random((B, H // 10, H // 10)) > 0.75                        # 10 x 10 blocks: components of many pixels
    d1[:, 1] += np.where(np.kron(blob, np.ones((10, 10), bool)), 3.0, -6.0).astype(np.float32)
    d2 = rng.normal(0, 2.5, size=(B, 16, H, H)).astype(np.float32)
    d2[:, 1::2] += 2.5                                                     # links mostly on: fewer than 256 components per image (the
    return d1, d2                                                          # reference numbers them in uint8)
