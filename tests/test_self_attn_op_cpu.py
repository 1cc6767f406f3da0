"""The standalone Self_Attn (gssd/self_attn_op.py, gssd.modules.Self_Attn.forward) and its two any-size C entries (csrc/sa_any.hip)
without a GPU: the symbols and their declared argument types, the argument contract (GSSD_EINVAL before any launch, so no device is
touched), and the module's shape / device errors."""
import ctypes as C

import pytest
import torch

from gssd import _lib
from gssd.modules import Self_Attn

c_i, c_fp = C.c_int, C.c_void_p
FWD_ARGS = [c_fp, c_fp, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_fp, c_fp]
BWD_ARGS = [c_fp, c_i, c_fp, c_i, c_fp, c_i, c_fp, c_fp, c_fp, c_fp, c_i, c_fp, c_fp, c_i, c_i, c_i, c_i, c_i, c_i, c_fp]
EINVAL = -1


def test_symbols_exist_with_declared_types():
    raw = C.CDLL(_lib.LIB_PATH)
    for name, args in (('gssd_self_attn_core_any_f32', FWD_ARGS), ('gssd_self_attn_flash_bwd_any_f32', BWD_ARGS)):
        assert hasattr(raw, name), f'{name} is not exported by {_lib.LIB_PATH}'
        fn = getattr(_lib.lib, name)
        assert fn.restype is c_i and list(fn.argtypes) == args, name
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'gssd_hip.h')).read()
    assert 'int gssd_self_attn_core_any_f32(' in hdr and 'int gssd_self_attn_flash_bwd_any_f32(' in hdr


@pytest.fixture(scope='module')
def ptr():
    """A 16-byte aligned host address: the contract checks come before any launch, so it is never read."""
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) // 16 * 16
    yield p
    del buf


def fwd(p, tp=None, B=1, N=4, Nk=4, Nkp=4, D=8, C2=8, kstride=8, lse=None):
    tp = p if tp is None else tp
    return _lib.lib.gssd_self_attn_core_any_f32(tp, p, p, p, B, N, Nk, Nkp, D, C2, kstride, lse, None)


def bwd(p, dq=None, qstride=8, krow=8, Nkp=4, ld_q=8, ld_kv=16, B=1, N=4, Nk=4, D=8, C2=8):
    dq = p if dq is None else dq
    return _lib.lib.gssd_self_attn_flash_bwd_any_f32(p, qstride, p, krow, p, Nkp, p, p, p, dq, ld_q, p, p, ld_kv, B, N, Nk, D, C2, None)


@pytest.mark.parametrize('kw', [dict(D=6), dict(D=0), dict(D=260, kstride=260), dict(C2=6), dict(C2=1028), dict(C2=0), dict(kstride=4),
                                dict(kstride=10), dict(Nkp=5), dict(Nkp=2), dict(N=0), dict(B=0), dict(Nk=0)])
def test_forward_contract_is_checked_before_any_launch(ptr, kw):
    assert fwd(ptr, **kw) == EINVAL
    assert _lib.lib.gssd_last_error()


def test_forward_alignment_and_null(ptr):
    assert fwd(ptr, tp=ptr + 4) == EINVAL
    assert fwd(ptr, lse=ptr + 8) == EINVAL
    assert _lib.lib.gssd_self_attn_core_any_f32(None, ptr, ptr, ptr, 1, 4, 4, 4, 8, 8, 8, None, None) == EINVAL


def test_width_message_names_the_widths(ptr):
    assert fwd(ptr, D=6, C2=24) == EINVAL
    msg = _lib.lib.gssd_last_error().decode()
    assert '6' in msg and '24' in msg and 'multiples of 4' in msg
    assert bwd(ptr, D=260, C2=1040, qstride=260, krow=260, ld_q=260, ld_kv=1040) == EINVAL
    msg = _lib.lib.gssd_last_error().decode()
    assert '260' in msg and '1040' in msg


@pytest.mark.parametrize('kw', [dict(D=6), dict(D=260, qstride=260, krow=260, ld_q=260, ld_kv=260), dict(C2=10), dict(C2=1028, ld_kv=1028),
                                dict(qstride=4), dict(qstride=10), dict(krow=4), dict(krow=9), dict(Nkp=3), dict(Nkp=6), dict(ld_q=4),
                                dict(ld_q=9), dict(ld_kv=4), dict(ld_kv=18), dict(N=0), dict(Nk=0), dict(B=0)])
def test_backward_contract_is_checked_before_any_launch(ptr, kw):
    assert bwd(ptr, **kw) == EINVAL
    assert _lib.lib.gssd_last_error()


def test_backward_alignment(ptr):
    assert bwd(ptr, dq=ptr + 4) == EINVAL


def test_existing_entries_keep_their_predicates():
    lib = _lib.lib
    assert lib.gssd_self_attn_flash_bwd_f32_supported(16, 64) == 1 and lib.gssd_self_attn_flash_bwd_f32_supported(20, 68) == 0


def test_module_shape_errors_come_first():
    m = Self_Attn(16)
    with pytest.raises(ValueError, match=r'\(1, 16, 4, 5\)'):
        m(torch.zeros(1, 16, 4, 5))
    with pytest.raises(ValueError, match=r'\(1, 8, 4, 4\).*8 channels'):
        m(torch.zeros(1, 8, 4, 4))
    with pytest.raises(ValueError, match='multiple of 8'):
        Self_Attn(12)(torch.zeros(1, 12, 4, 4))
    with pytest.raises(ValueError, match='2056'):
        Self_Attn(2056)(torch.zeros(1, 2056, 2, 2))
    with pytest.raises(ValueError):
        m(torch.zeros(16, 4, 4))


def test_module_has_no_cpu_fallback():
    m = Self_Attn(16, max_pool_factor=2)
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        m(torch.zeros(1, 16, 4, 4))
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        m(torch.zeros(1, 16, 4, 4, dtype=torch.float64))
    with pytest.raises(_lib.GssdError, match='no CPU fallback'):
        m(torch.zeros(1, 16, 4, 4), return_attn_map=True)
    u = m.snconv1x1_g.weight_u.clone()
    with pytest.raises(_lib.GssdError):
        m.train()(torch.zeros(1, 16, 4, 4))
    assert torch.equal(u, m.snconv1x1_g.weight_u)              # a refused call leaves the power-iteration state alone


def test_layers_self_attn_is_the_same_class():
    import layers.self_attn as L
    assert L.Self_Attn is Self_Attn and callable(getattr(Self_Attn, 'forward'))
    sd = Self_Attn(24, 2).state_dict()
    assert tuple(sd['snconv1x1_theta.weight_orig'].shape) == (3, 24, 1, 1) and tuple(sd['snconv1x1_attn.weight_v'].shape) == (12,)
