"""The fixed-size attention cores and the Self_Attn helpers on the MI355X, one kernel at a time through the C ABI, against float64 on the CPU.

gssd_self_attn_core_kv_f32 (csrc/flash_attn.hip -> flash_attn_kernel, csrc/flash_attn_core.h) over the whole table of
tests/attn_core_cases.py -- ten widths on the seven template instances, seven token shapes at the edges of the 64-query tile and of one
and two key blocks -- in three ways, each in the test's name so that a regression points at one instance:
  pooled keys (own buffer, kstride = d_real + 4 with NaN slack), lse given and NULL        test_kv_pooled_f32_lse_on_and_off
  the same with bf16 output                                                              test_kv_pooled_bf16_out
  keys in place (gssd_self_attn_core_f32: kp = tp + D, kstride = 2 D, Nk = N)            test_kv_in_place_f32
then the three-plane core (gssd_self_attn_core_x6_f32; its float64 parity at these sizes is test_self_attn_core_x6 of
tests/test_gpu_kernels.py), the adaptive average pooling of keys / values and its transpose (csrc/sa_pool.hip), gssd_rowdot_f32 and the
epilogue modes of gssd_bgemm_ex_f32 (csrc/sa_backward.hip).

Bounds.  Cores: TOL = 1e-4 (max-abs error over max-abs reference), outputs and log-sum-exp.  bf16 output: the bits of the fp32 output
rounded to nearest even (the same arithmetic, one rounding at the store).  lse = NULL, pass 2 alone: the same bits (no atomics).  Pooling:
a kernel adds at most n fp32 terms and divides once, so |err| <= 2 n 2^-24 max|input| with n the largest cell area; its transpose adds at
most 4 quotients: 2 * 8 * 2^-24 max|input| (the factor 2 covers the second-order terms).  rowdot and the GEMM epilogues: 1e-5 of
max|reference|, as test_sa_backward_building_blocks holds the fp32 helpers of the same file to.
"""
import os
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_core_cases as A                       # noqa: E402
from attn_core_cases import SENT                  # noqa: E402
from gpu_common import TOL, dev, rel              # noqa: E402,F401  (dev: fixture)
from gssd import _lib                             # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()


def worst(family, value):
    WORST[family] = max(WORST.get(family, 0.), float(value))
    print(f'worst so far, {family}: {WORST[family]:.3g}  ({time.time() - T0:.1f} s into the module)')


def stream():
    return torch.cuda.current_stream().cuda_stream


# --------------------------------------------------------------------------------------------------
# gssd_self_attn_core_kv_f32 / gssd_self_attn_core_f32: every instance
# --------------------------------------------------------------------------------------------------
IDS = [A.case_id(*r) for r in A.TABLE]
BF16_ROWS = [(d, c2, n, nk) for d, c2 in A.WIDTHS for n, nk in A.BF16_TOKENS]
IN_PLACE_ROWS = [(d, c2, n) for d, c2 in A.WIDTHS for n in A.IN_PLACE_N]


def run_pooled(c, d_real, C2, N, Nk, device, out_bf16=False, with_lse=True):
    """One call of the pooled-key form on sentinel-filled out [B N + 3][C2] / lse [B N + 3] -> (out, lse or None)."""
    B = A.batch_of(d_real, C2)
    tp, keys, krow, gT, Nkp = (t.to(device) if torch.is_tensor(t) else t for t in A.pooled_buffers(c, d_real, C2, N, Nk, B))
    assert Nkp % 4 == 0 and Nkp >= Nk and krow == d_real + 4 and bool(torch.isnan(keys[..., d_real:]).all())
    out = torch.full((B * N + 3, C2), SENT, device=device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    lse = torch.full((B * N + 3,), SENT, device=device) if with_lse else None
    _lib.check(_lib.lib.gssd_self_attn_core_kv_f32(tp.data_ptr(), keys.data_ptr(), gT.data_ptr(), out.data_ptr(), B, N, Nk, Nkp, d_real, C2, krow,
                                                   int(out_bf16), lse.data_ptr() if with_lse else None, stream()))
    torch.cuda.synchronize()
    return out, lse


def assert_out(out, c, B, N, C2, what):
    """rel(out, float64) < TOL; the two launches of the (256, 1024) width separately, so that a failure names the launch."""
    got, ref = out[:B * N].float().view(B, N, C2), c['out']
    assert bool(torch.isfinite(got).all()), what
    errs = []
    for lo in range(0, C2, 512):
        e = rel(got[..., lo:lo + 512], ref[..., lo:lo + 512])
        errs.append(e)
        assert e < TOL, f'{what}: channels [{lo}, {min(lo + 512, C2)}) off by {e:.3e}'
    assert bool((out[B * N:].float() == SENT).all()), f'{what}: rows beyond B N were written'
    return max(errs)


@pytest.mark.parametrize('d_real,C2,N,Nk', A.TABLE, ids=IDS)
def test_kv_pooled_f32_lse_on_and_off(dev, d_real, C2, N, Nk):
    B = A.batch_of(d_real, C2)
    c = A.table_case(d_real, C2, N, Nk)
    what = 'kv pooled ' + A.case_id(d_real, C2, N, Nk)
    out, lse = run_pooled(c, d_real, C2, N, Nk, dev)
    e_lse = rel(lse[:B * N].view(B, N), c['lse'])
    finite = bool(torch.isfinite(lse[:B * N]).all())
    e_out = assert_out(out, c, B, N, C2, what)
    print(f'{what} (instance {A.INSTANCES[(d_real, C2)]}): out {e_out:.2e} lse {e_lse:.2e}')
    assert finite and e_lse < TOL, (what, e_lse)
    assert bool((lse[B * N:] == SENT).all())
    worst('(a) kv pooled out', e_out)
    worst('(a) kv pooled lse', e_lse)
    # lse is optional, and the kernel has no atomics: the same bits
    out2, _ = run_pooled(c, d_real, C2, N, Nk, dev, with_lse=False)
    assert torch.equal(out2, out), f'{what}: lse = NULL changes {int((out2 != out).sum())} outputs'


@pytest.mark.parametrize('d_real,C2,N,Nk', BF16_ROWS, ids=[A.case_id(*r) for r in BF16_ROWS])
def test_kv_pooled_bf16_out(dev, d_real, C2, N, Nk):
    B = A.batch_of(d_real, C2)
    c = A.table_case(d_real, C2, N, Nk)
    what = 'kv pooled bf16 out ' + A.case_id(d_real, C2, N, Nk)
    out32, _ = run_pooled(c, d_real, C2, N, Nk, dev)
    assert_out(out32, c, B, N, C2, what + ' (fp32)')
    out16, lse = run_pooled(c, d_real, C2, N, Nk, dev, out_bf16=True)
    want = out32[:B * N].to(torch.bfloat16)                                # round to nearest even
    diff = out16[:B * N].view(torch.int16) != want.view(torch.int16)
    assert not bool(diff.any()), f'{what}: {int(diff.sum())} of {diff.numel()} bf16 outputs are not the rounded fp32 outputs'
    assert bool(torch.isfinite(out16.float()).all())
    # the tail rows still hold the sentinel as bf16 stores it (776)
    assert torch.equal(out16[B * N:], torch.full((3, C2), SENT, dtype=torch.bfloat16, device=dev)), f'{what}: rows beyond B N were written'
    assert rel(lse[:B * N].view(B, N), c['lse']) < TOL and bool((lse[B * N:] == SENT).all())


@pytest.mark.parametrize('d_real,C2,N', IN_PLACE_ROWS, ids=[f'd{d}-c{c2}-N{n}' for d, c2, n in IN_PLACE_ROWS])
def test_kv_in_place_f32(dev, d_real, C2, N):
    """Keys in place: tp rows are theta | phi, 2 d_real floats (8, 16 and 24 for the zero-filled widths 4, 8 and 12)."""
    B = A.batch_of(d_real, C2)
    c = A.table_case(d_real, C2, N, N)
    what = f'kv in place d{d_real}-c{C2}-N{N}'
    tp, gT, Np = A.in_place_buffers(c, d_real, C2, N, B)
    assert tp.shape == (B, N, 2 * d_real)
    tp, gT = tp.to(dev), gT.to(dev)
    out = torch.full((B * N + 3, C2), SENT, device=dev)
    _lib.check(_lib.lib.gssd_self_attn_core_f32(tp.data_ptr(), gT.data_ptr(), out.data_ptr(), B, N, Np, d_real, C2, 0, stream()))
    torch.cuda.synchronize()
    e = assert_out(out, c, B, N, C2, what)
    print(f'{what} (instance {A.INSTANCES[(d_real, C2)]}): out {e:.2e}')
    worst('(c) kv in place out', e)


# --------------------------------------------------------------------------------------------------
# gssd_self_attn_core_x6_f32: lse optional, pass 2 alone
# --------------------------------------------------------------------------------------------------
def x6_inputs(N, device, B=2, D=64, C2=256):
    """As test_self_attn_core_x6 (tests/test_gpu_kernels.py): logits of magnitude ~30."""
    rng = np.random.default_rng(N + D)
    Np = (N + 3) // 4 * 4
    tp = torch.from_numpy(rng.normal(0, 1.9, size=(B, N, 2 * D)).astype(np.float32))
    gT = torch.zeros(B, C2, Np)
    gT[:, :, :N] = torch.from_numpy(rng.normal(0, 1.0, size=(B, C2, N)).astype(np.float32))
    return tp.to(device), gT.to(device), Np


def x6_full(tp, gT, N, Np, device, with_lse, B=2, D=64, C2=256):
    lib = _lib.lib
    ws = torch.full((int(lib.gssd_self_attn_core_x6_ws_bytes(B, N, D, C2)) // 2,), 0x7fc0, device=device, dtype=torch.int16)     # bf16 NaN
    out = torch.full((B * N + 3, C2), SENT, device=device)
    lse = torch.full((B * N + 3,), SENT, device=device) if with_lse else None
    _lib.check(lib.gssd_self_attn_core_x6_f32(tp.data_ptr(), gT.data_ptr(), out.data_ptr(), B, N, Np, D, C2, ws.data_ptr(),
                                              lse.data_ptr() if with_lse else None, stream()))
    torch.cuda.synchronize()
    return out, lse, ws


@pytest.mark.parametrize('N', [33, 1025])
def test_self_attn_core_x6_without_lse(dev, N):
    """Both instances (4 waves up to N = 1024, 12 waves beyond): lse = NULL gives the same bits, rows beyond B N stay untouched."""
    B = 2
    tp, gT, Np = x6_inputs(N, dev)
    out, lse, _ = x6_full(tp, gT, N, Np, dev, True)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all())
    assert bool((out[B * N:] == SENT).all()) and bool((lse[B * N:] == SENT).all()) and not bool((lse[:B * N] == SENT).any())
    out2, _, _ = x6_full(tp, gT, N, Np, dev, False)
    assert torch.equal(out2, out), f'lse = NULL changes {int((out2 != out).sum())} outputs'


@pytest.mark.parametrize('N', [33, 1025])
def test_self_attn_core_x6_planes_on_the_filled_workspace(dev, N):
    """gssd_self_attn_core_x6_planes_f32 (pass 2 alone) on the workspace the full entry just filled returns the same bits."""
    B, D, C2 = 2, 64, 256
    tp, gT, Np = x6_inputs(N, dev)
    out, lse, ws = x6_full(tp, gT, N, Np, dev, True)
    out2, lse2 = torch.full((B * N + 3, C2), SENT, device=dev), torch.full((B * N + 3,), SENT, device=dev)
    _lib.check(_lib.lib.gssd_self_attn_core_x6_planes_f32(ws.data_ptr(), out2.data_ptr(), B, N, D, C2, lse2.data_ptr(), stream()))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out2).all())
    assert torch.equal(out2, out), f'pass 2 alone: {int((out2 != out).sum())} outputs differ'
    assert torch.equal(lse2, lse)


# --------------------------------------------------------------------------------------------------
# gssd_sa_pool_kv_f32 / gssd_sa_unpool_f32
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C8,C2', A.POOL_WIDTHS)
@pytest.mark.parametrize('H,P', A.POOL)
def test_sa_pool_kv(dev, H, P, C8, C2):
    B, N, Nk = 2, H * H, P * P
    Np, Nkp = A.roundup(N, 4), A.roundup(Nk, 4) + 4
    g = torch.Generator().manual_seed(H * 100 + P + C8)
    tp = torch.randn(B, N, 2 * C8, generator=g)
    gT = torch.zeros(B, C2, Np)
    gT[..., :N] = torch.randn(B, C2, N, generator=g)
    ref_k = F.adaptive_avg_pool2d(tp[..., C8:].double().transpose(1, 2).reshape(B, C8, H, H), P).reshape(B, C8, Nk).transpose(1, 2)
    ref_v = F.adaptive_avg_pool2d(gT[..., :N].double().reshape(B, C2, H, H), P).reshape(B, C2, Nk)
    kp = torch.full((B * Nk + 3, C8), SENT, device=dev)
    gTp = torch.full((B * C2 + 3, Nkp), float('nan'), device=dev)
    tpd, gTd = tp.to(dev), gT.to(dev)
    _lib.check(_lib.lib.gssd_sa_pool_kv_f32(tpd.data_ptr(), gTd.data_ptr(), kp.data_ptr(), gTp.data_ptr(), B, H, P, C8, C2, Np, Nkp, stream()))
    torch.cuda.synchronize()
    n = max(b - a for a, b in A.pool_cells(H, P)) ** 2                    # the largest cell area
    bound_k, bound_v = (2 * n * 2.0 ** -24 * float(t.abs().max()) for t in (tp[..., C8:], gT))
    e_k = float((kp[:B * Nk].view(B, Nk, C8).cpu().double() - ref_k).abs().max())
    e_v = float((gTp[:B * C2].view(B, C2, Nkp)[..., :Nk].cpu().double() - ref_v).abs().max())
    print(f'sa_pool_kv H {H} P {P} ({C8}, {C2}): largest cell {n}; keys {e_k:.2e} (bound {bound_k:.2e}) values {e_v:.2e} (bound {bound_v:.2e})')
    assert e_k <= bound_k and e_v <= bound_v
    pad = gTp[:B * C2, Nk:]
    assert pad.shape[1] >= 4 and bool((pad == 0).all()), 'the pad columns [P P, Nkp) are exactly 0'
    assert bool((kp[B * Nk:] == SENT).all()) and bool(torch.isnan(gTp[B * C2:]).all())
    worst('(e) pool forward err / bound', max(e_k / bound_k, e_v / bound_v))


@pytest.mark.parametrize('C8,C2', A.POOL_WIDTHS)
@pytest.mark.parametrize('H,P', A.POOL)
def test_sa_unpool(dev, H, P, C8, C2):
    B, N, Nk, CW = 2, H * H, P * P, C8 + C2
    ld = CW + 5
    g = torch.Generator().manual_seed(H * 100 + P + C8 + 7)
    dkg = torch.randn(B, Nk, CW, generator=g)
    x = torch.zeros(B, CW, H, H, dtype=torch.float64, requires_grad=True)
    F.adaptive_avg_pool2d(x, P).backward(dkg.double().transpose(1, 2).reshape(B, CW, P, P))
    ref = x.grad.reshape(B, CW, N).transpose(1, 2)
    dst = torch.full((B * N + 3, ld), SENT, device=dev)
    dkgd = dkg.to(dev)
    _lib.check(_lib.lib.gssd_sa_unpool_f32(dkgd.data_ptr(), dst.data_ptr(), B, H, P, CW, ld, stream()))
    torch.cuda.synchronize()
    bound = 2 * 8 * 2.0 ** -24 * float(dkg.abs().max())
    e = float((dst[:B * N, :CW].reshape(B, N, CW).cpu().double() - ref).abs().max())
    print(f'sa_unpool H {H} P {P} CW {CW}: {e:.2e} (bound {bound:.2e})')
    assert e <= bound
    assert bool((dst[:, CW:] == SENT).all()) and bool((dst[B * N:] == SENT).all())
    worst('(e) unpool err / bound', e / bound)


# --------------------------------------------------------------------------------------------------
# gssd_rowdot_f32, gssd_bgemm_ex_f32
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [4, 32, 260, 1024])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 1027])                      # four rows per workgroup
def test_rowdot(dev, rows, C):
    g = torch.Generator().manual_seed(rows * 2048 + C)
    a, b = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
    ref = (a.double() * b.double()).sum(-1)
    out = torch.full((rows + 3,), SENT, device=dev)
    ad, bd = a.to(dev), b.to(dev)
    _lib.check(_lib.lib.gssd_rowdot_f32(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), rows, C, stream()))
    torch.cuda.synchronize()
    e = rel(out[:rows], ref)
    print(f'rowdot rows {rows} C {C}: {e:.2e}  (max |ref| {float(ref.abs().max()):.3g}, max row sum |a b| {float((a * b).abs().sum(-1).max()):.3g})')
    assert e < 1e-5
    assert bool((out[rows:] == SENT).all())
    worst('(f) rowdot', e)


@pytest.mark.parametrize('transB', [0, 1])
@pytest.mark.parametrize('mode', [1, 2])
def test_bgemm_ex_epilogues(dev, mode, transB):
    """Mode 1: exp(alpha A B - rowvec[m]), rowvec the rows' true log-sum-exp, so the result is a softmax row in (0, 1].
    Mode 2: aux[m][n] (alpha A B - rowvec[m]).  transA = 0 with both transB: the forms self_attn_op.py and bwd_ops.py launch."""
    Bt, M, N, K, alpha = 3, 77, 50, 36, 0.5
    ldc = N + 3
    g = torch.Generator().manual_seed(40 + 2 * mode + transB)
    a = torch.randn(Bt, M, K, generator=g)
    b = torch.randn(*((Bt, N, K) if transB else (Bt, K, N)), generator=g)
    v = alpha * torch.matmul(a.double(), b.double().transpose(1, 2) if transB else b.double())
    aux = torch.full((Bt, M, ldc), float('nan'))
    if mode == 1:
        rowvec = torch.logsumexp(v, -1).float()
        ref = torch.exp(v - rowvec.double().unsqueeze(-1))
        assert float(ref.max()) <= 1.0 + 1e-6 and float(ref.min()) > 0
    else:
        rowvec = torch.randn(Bt, M, generator=g)
        aux[..., :N] = torch.randn(Bt, M, N, generator=g)
        ref = aux[..., :N].double() * (v - rowvec.double().unsqueeze(-1))
    c = torch.full((Bt * M + 3, ldc), 7.0, device=dev)                    # ldc > N: the slack columns must stay untouched
    ad, bd, rd, xd = a.to(dev), b.to(dev), rowvec.to(dev), aux.to(dev)
    _lib.check(_lib.lib.gssd_bgemm_ex_f32(ad.data_ptr(), bd.data_ptr(), c.data_ptr(), M, N, K, K, b.shape[2], ldc, 0, transB, M * K, b[0].numel(),
                                          M * ldc, Bt, alpha, mode, rd.data_ptr(), xd.data_ptr() if mode == 2 else None, stream()))
    torch.cuda.synchronize()
    got = c[:Bt * M].view(Bt, M, ldc)
    e = rel(got[..., :N], ref)
    print(f'bgemm_ex mode {mode} transB {transB}: {e:.2e}')
    assert bool(torch.isfinite(got).all()) and e < 1e-5
    assert bool((got[..., N:] == 7.0).all()) and bool((c[Bt * M:] == 7.0).all())
    worst('(g) bgemm_ex', e)
