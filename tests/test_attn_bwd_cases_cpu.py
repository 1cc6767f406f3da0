"""The case tables of the attention backwards (tests/attn_bwd_cases.py) on the CPU: that they bracket the own tile and the streamed blocks
of every kernel, the gate tests/test_gpu_attn_bwd.py holds gssd_self_attn_flash_bwd_bf16 to and that the gate would catch a streamed mask
one short, the same for the fp32 rows, and the argument checks of the entry points (refused before any launch, so they run without a GPU).

The bf16 gate.  model() makes the kernel's stated roundings in float64; e_model = token_err(model, exact) is what they cost.  The kernel
makes the same roundings, accumulates in fp32 (2^-24 per term against 2^-9 per rounded factor) and, where __expf and exp differ in the
last fp32 bits, now and then rounds a P or dS to the other bf16 neighbour: token_err(kernel, exact) <= 2 e_model, the shape of gate the
three-plane forward core is held to (1.5 x its fp32 sibling plus a floor).  So that a slipped kernel cannot pass, each slip must move the
gradients it touches by at least 8 e_model in the same metric -- a condition on the inputs (a last token without weight would let such a
kernel pass), met by another seed in SEEDS where the default fails, never by a smaller factor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as K                # noqa: E402
import attn_core_cases as A               # noqa: E402
from gpu_common import TOL, rel           # noqa: E402

BF16_ROWS = [(d, c2, n) for d, c2 in K.FLASH_BF16_WIDTHS for n in K.FLASH_BF16_N if n > 1]
F32_ROWS = [(n, nk) for n, nk in K.FLASH_F32_TOKENS if nk > 1]
CHAIN_ROWS = [r for r in K.CHAIN_ROWS if r[3] > 1]


def test_tables_reach_what_they_say():
    assert K.FLASH_BF16_WIDTHS == [(32, 128), (64, 256), (128, 512)] and K.FLASH_BF16_N == [1, 31, 32, 33, 63, 64, 65, 97, 131] and K.B == 2
    assert len(K.FLASH_BF16_ROWS) == 54 and len(set(K.FLASH_BF16_ROWS)) == 54
    assert {f for _, _, _, f in K.FLASH_BF16_ROWS} == {'x3', 'f32mfma'} and dict(K.FLASH_BF16_FORMS) == {'x3': True, 'f32mfma': False}
    ns = set(K.FLASH_BF16_N)
    # one and two streamed blocks of 32, one and two own tiles of 64: a size below, at and above each edge
    for edge, step in ((K.STREAMED, K.STREAMED), (2 * K.STREAMED, K.STREAMED), (K.OWN, K.OWN)):
        assert {edge - 1, edge, edge + 1} <= ns, edge
        assert -(-(edge - 1) // step) == edge // step == -(-(edge + 1) // step) - 1
    assert (K.OWN, K.STREAMED) == (64, 32) and 1 in ns
    ragged = [n for n in ns if n % K.OWN and n % K.STREAMED and n > 2 * K.STREAMED + 1]
    assert {97, 131} <= set(ragged) and max(-(-n // K.OWN) for n in ns) == 3 and max(-(-n // K.STREAMED) for n in ns) == 5
    # the (16, 64) instance: the forward table's rows, fewer streamed rows than waves, a last block of one row, five key tiles
    assert K.FLASH_F32_TOKENS[:len(A.TOKENS)] == A.TOKENS and K.FLASH_F32_TOKENS[len(A.TOKENS):] == [(3, 2), (129, 129), (2, 257)]
    assert {(n, nk) for n, nk, f in K.FLASH_F32_ROWS if f == 'inplace'} == {(n, nk) for n, nk in K.FLASH_F32_TOKENS if n == nk} == {(1, 1), (129, 129)}
    assert sum(f == 'pooled' for _, _, f in K.FLASH_F32_ROWS) == len(K.FLASH_F32_TOKENS) == 10
    T, W = K.F32_TILE, K.F32_WAVES
    assert (T, W) == (64, 4)
    assert any(n < W and nk < W for n, nk in K.FLASH_F32_TOKENS if nk > 1)               # streamed rows with idle waves, in both launches
    assert any(n % T == 1 and nk % T == 1 and n > T for n, nk in K.FLASH_F32_TOKENS)     # a last streamed block of one row: wave 0 alone
    assert max(-(-nk // T) for _, nk in K.FLASH_F32_TOKENS) == 5
    for side in (0, 1):                                                                  # 64 and 65 own / streamed tokens on either side
        assert {T, T + 1} <= {t[side] for t in K.FLASH_F32_TOKENS}, side
    assert K.CHAIN_WIDTHS == [(4, 32), (64, 256)] and K.CHAIN_TOKENS == [(1, 1), (65, 31), (63, 33), (100, 65), (25, 131)] and len(K.CHAIN_ROWS) == 10
    assert sum(A.roundup(nk, 4) > nk for _, nk in K.CHAIN_TOKENS) == 5               # every row has pad columns [Nk, Nkp)
    assert K.SOFTMAX_BWD == [(1, 1, 4), (5, 63, 64), (4, 64, 64), (3, 65, 68), (9, 129, 132), (70000, 5, 8)]
    assert all(s >= n for _, n, s in K.SOFTMAX_BWD) and sum(s > n for _, n, s in K.SOFTMAX_BWD) == 5
    assert max(r for r, _, _ in K.SOFTMAX_BWD) > K.SOFTMAX_BWD_GRID_WAVES == 65536        # the grid-stride loop runs twice
    ids = [K.bf16_id(*r) for r in K.FLASH_BF16_ROWS] + [K.f32_id(*r) for r in K.FLASH_F32_ROWS] + [K.chain_id(*r) for r in K.CHAIN_ROWS] + \
        [K.softmax_id(*r) for r in K.SOFTMAX_BWD]
    assert len(set(ids)) == len(ids) == 54 + 12 + 10 + 6
    assert all(k in ids or k in {K.bf16_id(d, c2, n) for d, c2, n in BF16_ROWS} for k in K.SEEDS), 'a SEEDS key that names no row'


def test_supported_widths_agree_with_the_tables():
    from gssd._lib import lib
    widths = set(K.FLASH_BF16_WIDTHS) | set(A.WIDTHS) | set(K.CHAIN_WIDTHS) | {(48, 192), (64, 128), (128, 256), (16, 128)}
    for w in sorted(widths):
        assert lib.gssd_self_attn_flash_bwd_supported(*w) == (1 if w in K.FLASH_BF16_WIDTHS else 0), w
        assert lib.gssd_self_attn_flash_bwd_f32_supported(*w) == (1 if w == K.FLASH_F32_WIDTH else 0), w


def test_token_err_is_per_token():
    ref = torch.ones(2, 50, 4, dtype=torch.float64)
    got = ref.clone()
    got[1, 49] = 0                                                         # one token lost entirely: 1 % of the tensor's mass
    assert abs(K.token_err(got, ref) - 1.0) < 1e-12 and K.token_err(ref, ref) == 0


@pytest.mark.parametrize('D,C2,N', BF16_ROWS, ids=[K.bf16_id(*r) for r in BF16_ROWS])
def test_bf16_gate_and_that_each_slip_fails_it(D, C2, N):
    c = K.flash_bf16_case(D, C2, N)
    ex = K.exact(c)
    for form, x3 in K.FLASH_BF16_FORMS:
        e = K.e_model(D, C2, N, x3)
        assert all(np.isfinite(v) and 0 < v < 0.05 for v in e.values()), e        # two factors rounded to 2^-9 each: a few 1e-3, never 5 %
        for slip, moved in K.SLIPS.items():
            mo = K.model(c, x3, slip)
            for k in K.GRADS:
                if k not in moved:
                    assert torch.equal(mo[k], K.model(c, x3)[k]), (slip, k)
                    continue
                moves = K.token_err(mo[k], ex[k])
                print(f'{K.bf16_id(D, C2, N, form)} {k}: e_model {e[k]:.2e}, {slip} {moves:.2e} = {moves / e[k]:.1f} e_model (seed '
                      f'{K.SEEDS.get(K.bf16_id(D, C2, N), 0)})')
                assert moves >= 8 * e[k], (slip, k, moves / e[k])
                assert moves > 2 * e[k]                                      # the GPU gate: the slipped model fails it


@pytest.mark.parametrize('D,C2', K.FLASH_BF16_WIDTHS)
def test_bf16_single_token_bound(D, C2):
    """N = 1: exact() has d theta = d phi = 0 up to the rounding of D; the GPU test holds the kernel to single_token_bound, and model()
    itself stays inside it.  d g is gated by e_model like every other row."""
    c = K.flash_bf16_case(D, C2, 1)
    b_th, b_ph = K.single_token_bound(c)
    ex = K.exact(c)
    assert float(b_th.min()) > 0 and float(b_ph.min()) > 0
    for form, x3 in K.FLASH_BF16_FORMS:
        mo = K.model(c, x3)
        for got in (ex, mo):
            w_th, w_ph = got['dtheta'].abs().amax(dim=(1, 2)), got['dphi'].abs().amax(dim=(1, 2))
            print(f'{K.bf16_id(D, C2, 1, form)}: |d theta| {w_th.tolist()} <= {b_th.tolist()}, |d phi| {w_ph.tolist()} <= {b_ph.tolist()}')
            assert bool((w_th <= b_th).all()) and bool((w_ph <= b_ph).all())
        e = K.e_model(D, C2, 1, x3)['dg']
        assert e < 2.0 ** -9, e                                             # P = 1 +- the logits' error, rounded to bf16
        assert rel(ex['dg'], c['dag']) < 2.0 ** -9


@pytest.mark.parametrize('N,Nk', F32_ROWS, ids=[K.f32_id(n, nk, 'pooled') for n, nk in F32_ROWS])
def test_f32_row_notices_a_streamed_mask_one_short(N, Nk):
    notices(K.kv_case(*K.FLASH_F32_WIDTH, N, Nk, K.f32_id(N, Nk, 'pooled')), K.f32_id(N, Nk, 'pooled'))
    if N == Nk:
        notices(K.kv_case(*K.FLASH_F32_WIDTH, N, Nk, K.f32_id(N, Nk, 'inplace')), K.f32_id(N, Nk, 'inplace'))


@pytest.mark.parametrize('D,C2,N,Nk', CHAIN_ROWS, ids=[K.chain_id(*r) for r in CHAIN_ROWS])
def test_chain_row_notices_a_reduction_one_short(D, C2, N, Nk):
    """The chain's slips are the same sums one term short: K = Nk - 1 in the d theta GEMM, K = N - 1 in the two transA GEMMs."""
    notices(K.kv_case(D, C2, N, Nk, K.chain_id(D, C2, N, Nk)), K.chain_id(D, C2, N, Nk))


def notices(c, what):
    ref = K.kv_backward(c)
    for k in ('dq', 'dk', 'dv'):
        assert rel(ref[k], c[k]) < 1e-12                                   # kv_backward restates core_case
    for slip, moved in K.KV_SLIPS.items():
        got = K.kv_backward(c, slip)
        for k in moved:
            e = rel(got[k], ref[k])
            print(f'{what} {k}: {slip} moves it by {e:.2e}  (10 TOL = {10 * TOL:.0e}, seed {K.SEEDS.get(what, 0)})')
            assert e > 10 * TOL, (what, slip, k, e)


def test_softmax_bwd_reference():
    for rows, n, stride in K.SOFTMAX_BWD[:-1]:
        attn, dattn, ref = K.softmax_bwd_case(rows, n, stride)
        assert attn.shape == dattn.shape == (rows + 2, stride) and ref.shape == (rows, n) and ref.dtype == torch.float64
        assert bool(torch.isnan(attn[:, n:]).all()) and bool((dattn[:, n:] == K.SENT).all()) and bool((dattn[rows:] == K.SENT).all())
        assert float((attn[:, :n].double().sum(-1) - 1).abs().max()) < 1e-6
        assert float(ref.sum(-1).abs().max()) < 1e-5 * max(float(ref.abs().max()), 1e-30) + 1e-12       # softmax backward rows sum to zero
        a = attn[:rows, :n].double().requires_grad_()
        (torch.softmax(torch.log(a), -1) * dattn[:rows, :n].double()).sum().backward()               # softmax(log a) = a: d / d logits
        assert rel(a.grad * a.detach(), ref) < 1e-6 or n == 1


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


def test_flash_bwd_bf16_argument_checks():
    from gssd._lib import lib
    bufs = [host(256) for _ in range(8)]
    p = [b.ctypes.data for b in bufs]
    assert all(a % 16 == 0 for a in p)

    def call(tp=p[0], g16=p[3], dtpg=p[7], N=8, D=64, C2=256):
        return lib.gssd_self_attn_flash_bwd_bf16(tp, p[1], p[2], g16, p[4], p[5], p[6], dtpg, 1, N, D, C2, None)
    for kw, mentions in ((dict(tp=p[0] + 4), 'tp % 16'), (dict(dtpg=p[7] + 8), 'dtpg % 16'), (dict(g16=None), 'g_bf16'), (dict(N=0), 'N > 0'),
                         (dict(D=48, C2=192), 'unsupported'), (dict(D=64, C2=128), 'unsupported'), (dict(D=16, C2=64), 'unsupported')):
        refused(lib, call(**kw), kw, mentions)


def test_flash_bwd_f32_and_softmax_bwd_argument_checks():
    from gssd._lib import lib
    bufs = [host(256) for _ in range(9)]
    p = [b.ctypes.data for b in bufs]

    def call(qstride=32, krow=20, Nkp=8, ld_q=20, ld_kv=88, D=16, C2=64):
        return lib.gssd_self_attn_flash_bwd_f32(p[0], qstride, p[1], krow, p[2], Nkp, p[3], p[4], p[5], p[6], ld_q, p[7], p[8], ld_kv, 1, 8, 6, D, C2,
                                                None)
    for kw, mentions in ((dict(qstride=12), 'qstride >= D'), (dict(krow=15), 'krow >= D'), (dict(Nkp=5), 'Nkp >= Nk'), (dict(ld_q=8), 'ld_q >= D'),
                         (dict(ld_kv=12), 'ld_kv >= D'), (dict(D=16, C2=32), 'supported'), (dict(D=8, C2=64, krow=16), 'supported'),
                         (dict(D=64, C2=256, qstride=128, krow=68, ld_q=68), 'supported')):
        refused(lib, call(**kw), kw, mentions)
    refused(lib, lib.gssd_softmax_bwd_rows_f32(p[0], p[1], 4, 9, 8, None), 'row_stride < n', 'row_stride >= n')
