"""CPU tests of PixelLink version "2s" (the fifth, 150 x 150 output stage): the module surface against the imported reference
(tests/golden/pixellink2s.npz, tests/golden/make_pixellink2s_golden.py), the construction rules, the C ABI declarations of the 2s
kernels, and the restatement tests/pixellink2s_ref.py against the reference fixture."""
import os
import re

import numpy as np
import pytest
import torch

import pixel_link.pixel_link_config as config
from gssd import synth
import pixellink2s_ref as R2
from test_pixellink_cpu import PLAIN as PLAIN4, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('gssd_pixellink_final5_f32', 'gssd_pixellink_final5_bwd_f32', 'gssd_self_attn_flash_bwd_f32',
               'gssd_self_attn_flash_bwd_f32_supported')


@pytest.fixture
def v2s():
    """pixel_link_config.version = "2s" for the test; "4s" again afterwards, whatever happens."""
    config.version = "2s"
    try:
        yield
    finally:
        config.version = "4s"


def build2s(kw, mpf=1):
    from pixel_link.model import PixelLink
    config.version = "2s"
    try:
        net = PixelLink(**kw, max_pool_factor=mpf)
    finally:
        config.version = "4s"
    net.load_state_dict(synth.synth_state_dict({k: tuple(v.shape) for k, v in net.state_dict().items()}, seed=2222))
    return net


def keys_of(net):
    return [f'{k}:{"x".join(map(str, v.shape))}' for k, v in net.state_dict().items()]


@pytest.mark.parametrize('tag', list(R2.VARIANTS))
def test_state_dict_matches_reference(golden, tag):
    """Keys (with the modules_except_dcn aliases) and shapes of the reference's 2s module, in its order of modules (inside one Self_Attn
    block the spectral-norm parameters are registered in another order than the reference's hooks leave them; load_state_dict does not
    care, and that order is the one "4s" has always had)."""
    g = golden('pixellink2s')
    kw, mpf = R2.VARIANTS[tag]
    mine, ref = keys_of(build2s(kw, mpf)), g[f'model_{tag}_keys'].tolist()
    assert sorted(mine) == sorted(ref)

    def modules(keys):
        out = []
        for k in keys:
            m = k.split(':')[0].rsplit('.', 1)[0]
            if not out or out[-1] != m:
                out.append(m)
        return out
    assert modules(mine) == modules(ref)


def test_reference_checkpoint_loads_strictly(golden):
    """A state dict in the reference's layout (every key of the fixture's list, synthetic values) loads with strict=True."""
    g = golden('pixellink2s')
    kw, mpf = R2.VARIANTS['sa']
    shapes = {}
    for e in g['model_sa_keys'].tolist():
        k, s = e.split(':')
        shapes[k] = tuple(int(d) for d in s.split('x')) if s else ()
    sd = synth.synth_state_dict(shapes, seed=5)
    net = build2s(kw, mpf)
    net.load_state_dict(sd, strict=True)
    assert torch.equal(net.out1_2.weight, sd['out1_2.weight']) and torch.equal(net.bn_fuse1.running_var, sd['bn_fuse1.running_var'])
    assert net.final_1.in_channels == 10 and net.final_2.in_channels == 80


def test_2s_with_dcn_raises(v2s):
    from pixel_link.model import PixelLink
    kw = dict(R2.SA, num_dcn_layers=1, groups_dcn=4, dcn_cat_sab=True)
    with pytest.raises(NotImplementedError, match='reference itself fails'):
        PixelLink(**kw)
    with pytest.raises(NotImplementedError):
        PixelLink(**dict(R2.PLAIN, num_dcn_layers=2, groups_dcn=1))


def test_other_settings_still_refused(v2s):
    from pixel_link.model import PixelLink
    for name, val in (('feature_scale', 2), ('dilation', False)):
        old = getattr(config, name)
        setattr(config, name, val)
        try:
            with pytest.raises(NotImplementedError):
                PixelLink(**R2.PLAIN)
        finally:
            setattr(config, name, old)
    config.version = "8s"
    with pytest.raises(NotImplementedError):
        PixelLink(**R2.PLAIN)


def test_version_captured_at_construction():
    net = build2s(R2.PLAIN)
    assert config.version == "4s" and net.version == "2s"
    assert net.out1_1.in_channels == 128 and net.fuse1.out_channels == 128 and net.final_2.in_channels == 80
    from pixel_link.model import PixelLink
    net4 = PixelLink(**PLAIN4)
    assert net4.version == "4s" and not hasattr(net4, 'out1_1') and net.version == "2s"


def test_4s_construction_unchanged(golden):
    """4s: the same modules in the same order (the 4s reference fixture's key list), and the same random draws: two builds from one seed
    agree, and the generator is left where a build of the same modules leaves it."""
    from pixel_link.model import PixelLink
    kw = dict(PLAIN4, use_self_attention=True, use_self_attention_base=True)
    torch.manual_seed(3)
    a = PixelLink(**kw)
    after_a = torch.rand(4)
    torch.manual_seed(3)
    config.version = "2s"
    try:
        PixelLink(**R2.SA)                                 # a 2s build in between does not change what "4s" builds
    finally:
        config.version = "4s"
    torch.manual_seed(3)
    b = PixelLink(**kw)
    assert torch.equal(torch.rand(4), after_a)
    assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    g = golden('pixellink')
    assert keys_of(PixelLink(**PLAIN4)) == g['model_plain_keys'].tolist()


def test_new_symbols_declared():
    from gssd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'gssd_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r'\b' + name + r'\(', hdr), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(_lib.lib, name)
    for name in NEW_SYMBOLS[:3]:                               # launches (last parameter: the stream) -> the plan-runner table
        idx = _lib.lib.gssd_plan_fn_index(name.encode())
        assert idx >= 0 and _lib.lib.gssd_plan_fn_nargs(idx) == len(_lib.SIGNATURES[name][1]) - 1
    assert _lib.lib.gssd_self_attn_flash_bwd_f32_supported(16, 64) == 1
    assert _lib.lib.gssd_self_attn_flash_bwd_f32_supported(8, 32) == 0 and _lib.lib.gssd_self_attn_flash_bwd_f32_supported(64, 256) == 0


# the unpooled SA variant's two 22 500-token attention maps take several GB in float64 on the CPU: tests/test_gpu_pixellink2s.py checks it
@pytest.mark.parametrize('tag', ['plain', 'sapool', 'nocascade'])
def test_restatement_vs_reference(golden, tag):
    g = golden('pixellink2s')
    kw, mpf = R2.VARIANTS[tag]
    net = build2s(kw, mpf)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in net.state_dict().items()}
    x = synth.synth_images(1, seed=300).double()
    with torch.no_grad():
        o1, o2, upd = R2.pixellink2s_forward(sd, x, max_pool_factor=mpf, training=True, **kw)
    assert tuple(o1.shape) == (1, 2, 150, 150) and tuple(o2.shape) == (1, 16, 150, 150)
    r1 = g[f'model_{tag}_out1']
    assert rel(o1 if r1.shape[2] == 150 else o1[:, :, ::3, ::3], r1) < 2e-5
    assert rel(o2[:, :, ::5, ::5], g[f'model_{tag}_out2s']) < 2e-5
    if kw['batch_norm'] and kw['use_fuseconv']:
        assert rel(upd['bn_fuse1.running_mean'], g[f'model_{tag}_bn_fuse1_rm']) < 1e-5
    if kw['use_self_attention']:
        assert rel(upd['self_attn_list.0.snconv1x1_theta.weight_u'], g[f'model_{tag}_sa0_u']) < 1e-5


def test_oracle_loss_and_decode_at_150(golden):
    """The loss / decoding oracles the GPU tests compare against reproduce the reference at 150 x 150, including an image with no
    positive pixel and exact ties at the OHEM threshold."""
    from oracle import pixellink_oracle as PO
    g = golden('pixellink2s')
    o1, o2, pix, neg, posw, link = (torch.from_numpy(a) for a in R2.loss_inputs(11))
    pp, pn, lp, ln, negw = PO.pixel_link_loss(o1, o2, pix, neg, posw, link)
    assert rel([pp, pn, lp, ln], g['loss_vals']) < 1e-6
    assert np.array_equal(np.packbits(negw.numpy().astype(bool)), g['loss_neg_weight_bits'])
    # ties: several candidates of image 0 share the threshold probability, and all of them are mined
    p0 = torch.softmax(o1[0], 0)[0]
    cand = p0[neg[0] == 1]
    thr = torch.sort(cand).values[int(g['loss_neg_area'][0]) - 1]
    assert int((cand == thr).sum()) > 1 and int(negw[0].sum()) > int(g['loss_neg_area'][0])
    d1, d2 = R2.decode_inputs(21)
    lab = PO.decode_links(torch.from_numpy(d1), torch.from_numpy(d2))
    assert np.array_equal(lab.astype(np.uint8), g['dec_labels_u8']) and lab.max() < 256
