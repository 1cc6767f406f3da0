"""The case table of the fixed-size attention cores (tests/attn_core_cases.py) on the CPU: that it reaches every template instance of
gssd_self_attn_core_kv_f32 and brackets every key block, that every row would notice a key mask one short or a key tile shifted by one
row (a condition on the inputs: a last key without weight would let such a kernel pass), and the argument checks of the entry points the
GPU module runs (refused before any launch, so they run without a GPU)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_core_cases as A               # noqa: E402
from gpu_common import TOL, rel           # noqa: E402

ROWS = [r for r in A.TABLE if r[3] > 1]


def test_table_reaches_every_instance():
    assert len(A.TABLE) == 70 and len(set(A.TABLE)) == 70
    for w in A.WIDTHS:
        assert A.instance_of(*w) == A.INSTANCES[w], w
    # the seven template instances of the dispatcher (the (256, 1024) width is two launches of one)
    assert {A.INSTANCES[w][:3] for w in A.WIDTHS} == {(64, 256, 64), (128, 512, 32), (256, 512, 32), (32, 128, 64), (16, 32, 64), (16, 64, 64)}
    assert {w for w in A.WIDTHS if A.INSTANCES[w][3] == 2} == {(256, 1024)} and A.batch_of(256, 1024) == 3 and A.batch_of(64, 256) == 2
    # zero-filled widths: every real width 4 ... 16 of the (<= 16, 32) instance, two of (<= 16, 64)
    assert {d for d, c2 in A.WIDTHS if c2 == 32} == {4, 8, 12, 16} and {d for d, c2 in A.WIDTHS if c2 == 64} == {8, 16}
    assert A.instance_of(48, 192) is None and A.instance_of(64, 128) is None and A.instance_of(20, 32) is None
    nks = {nk for _, nk in A.TOKENS}
    for BKV in (32, 64):
        tiles = {-(-nk // BKV) for nk in nks}                              # key tiles a row runs
        for blocks in (1, 2):
            assert blocks in tiles and blocks + 1 in tiles, (BKV, blocks)
    assert {31, 32, 33, 64, 65} <= nks and max(nks) > 128                  # tight at 32 and at 64 (= 2 x 32 and 1 x 64); 131 is beyond 2 x 64
    ns = {n for n, _ in A.TOKENS}
    assert {63, 64, 65} <= ns and max(ns) > 128 and 1 in ns
    assert sum(A.roundup(nk, 4) > nk for _, nk in A.TOKENS) >= 4
    assert all(t in A.TOKENS for t in A.BF16_TOKENS)


def test_pool_cases_overlap_where_they_should():
    for H, P in A.POOL:
        cs = A.pool_cells(H, P)
        overlap = any(cs[i][1] > cs[i + 1][0] for i in range(P - 1))
        assert overlap == ((H, P) in A.POOL_OVERLAPPING), (H, P)
        assert cs[0][0] == 0 and cs[-1][1] == H and all(b > a for a, b in cs)
    assert len(A.POOL_OVERLAPPING) == 3 and {(c8, c2) for c8, c2 in A.POOL_WIDTHS} == {(c8, c2) for c8 in (4, 16) for c2 in (32, 64)}


@pytest.mark.parametrize('d_real,C2,N,Nk', ROWS, ids=[A.case_id(*r) for r in ROWS])
def test_row_notices_a_wrong_key_mask_and_a_shifted_key_tile(d_real, C2, N, Nk):
    c = A.table_case(d_real, C2, N, Nk)
    BKV = A.INSTANCES[(d_real, C2)][2]
    e_drop = rel(A.without_last_key(c), c['out'])
    e_rot = rel(A.last_block_rotated(c, BKV), c['out'])
    print(f'{A.case_id(d_real, C2, N, Nk)}: last key dropped {e_drop:.2e}, last key tile rotated {e_rot:.2e}  (10 TOL = {10 * TOL:.0e})')
    assert e_drop > 10 * TOL and e_rot > 10 * TOL
    assert np.isfinite(c['out'].numpy()).all() and np.isfinite(c['lse'].numpy()).all()


# ---- argument checks: refused with GSSD_EINVAL before anything is launched -------------------------------------------------------------------
def host(n):
    """A non-null, 64-byte aligned host buffer (never dereferenced: the calls below are refused first)."""
    raw = np.zeros(4 * n + 64, np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + 4 * n].view(np.float32)


def refused(lib, rc, what, mentions):
    msg = lib.gssd_last_error()
    assert rc != 0 and msg, what
    assert mentions in msg.decode(), (what, msg)


def test_core_argument_checks():
    from gssd._lib import lib
    bufs = [host(256) for _ in range(6)]
    p = [b.ctypes.data for b in bufs]
    assert all(a % 16 == 0 for a in p)

    def kv(N=8, Nk=6, Nkp=8, D=64, C2=256, kstride=68, kp=p[1], out_bf16=0):
        return lib.gssd_self_attn_core_kv_f32(p[0], kp, p[2], p[3], 1, N, Nk, Nkp, D, C2, kstride, out_bf16, p[4], None)
    for kw, mentions in ((dict(Nkp=6), 'Nkp % 4'), (dict(Nkp=4), 'Nkp >= Nk'), (dict(kstride=60), 'kstride >= D'), (dict(kp=p[1] + 4), 'kp % 16'),
                         (dict(D=48, C2=192, kstride=48), 'unsupported'), (dict(D=64, C2=128), 'unsupported')):
        refused(lib, kv(**kw), kw, mentions)
    for w in A.WIDTHS + [(128, 512), (48, 192), (64, 128), (16, 32)]:
        assert lib.gssd_self_attn_core_x6_supported(*w) == (1 if w == (64, 256) else 0), w
    for B, N in ((1, 1), (2, 33), (3, 1024), (2, 1025), (32, 1444)):
        assert lib.gssd_self_attn_core_x6_ws_bytes(B, N, 64, 256) == 2 * 3 * (B * N * 2 * 64 + B * 256 * A.roundup(N, 32)), (B, N)
    for args in ((2, 33, 128, 512), (2, 33, 64, 128), (2, 33, 32, 128), (2, 0, 64, 256), (2, -5, 64, 256)):
        assert lib.gssd_self_attn_core_x6_ws_bytes(*args) == -1, args


def test_helper_argument_checks():
    from gssd._lib import lib
    bufs = [host(256) for _ in range(6)]
    p = [b.ctypes.data for b in bufs]

    def pool(H=4, P=2, Np=16, Nkp=4):
        return lib.gssd_sa_pool_kv_f32(p[0], p[1], p[2], p[3], 1, H, P, 4, 32, Np, Nkp, None)
    for kw, mentions in ((dict(P=5, Nkp=28), 'P <= H'), (dict(Np=15), 'Np >= H * H'), (dict(Nkp=3), 'Nkp >= P * P')):
        refused(lib, pool(**kw), kw, mentions)
    refused(lib, lib.gssd_sa_unpool_f32(p[0], p[1], 1, 4, 2, 36, 35, None), 'ld < CW', 'ld >= CW')

    def ex(mode, rowvec, aux):
        return lib.gssd_bgemm_ex_f32(p[0], p[1], p[2], 4, 4, 4, 4, 4, 4, 0, 1, 16, 16, 16, 1, 1.0, mode, rowvec, aux, None)
    refused(lib, ex(1, None, None), 'mode 1 without rowvec', 'mode == 1 && rowvec')
    refused(lib, ex(2, p[3], None), 'mode 2 without aux', 'mode == 2 && rowvec && aux')
    refused(lib, ex(3, p[3], p[4]), 'mode 3', 'mode')
