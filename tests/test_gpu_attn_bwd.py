"""The three attention backwards on the MI355X, one kernel instance at a time through the C ABI, against float64 on the CPU, over the tables
of tests/attn_bwd_cases.py (tests/test_attn_bwd_cases_cpu.py derives the gates and shows that each row would notice a mask one short).

(a) test_flash_bwd_bf16      gssd_self_attn_flash_bwd_bf16 (csrc/sa_flash_bwd.hip): three widths x nine N around the 64-token own tile and
                             the 32-token streamed block x both logit forms; every call runs the own-keys and the own-queries instance.
                             Operands as gssd/bwd_ops.py hands them, each with three trailing NaN rows; the output has three sentinel
                             rows beyond B N.  Gate per gradient: token_err(kernel, exact) <= 2 e_model (N = 1: d theta, d phi inside
                             single_token_bound); bit-identical second call.
(b) test_flash_bwd_f32       gssd_self_attn_flash_bwd_f32 (csrc/sa_flash_bwd_f32.hip), the (16, 64) instance, in the pooled and the
                             keys-in-place calling form: rel < TOL per gradient, slack columns and trailing rows untouched, same bits twice.
(c) test_explicit_chain      the calls of _sa_explicit's lse branch in its order and with its strides (csrc/sa_backward.hip) over maps
                             whose pad columns [Nk, Nkp) hold NaN before and after: rel < TOL.
(d) test_softmax_bwd_rows    gssd_softmax_bwd_rows_f32: 1e-5 of max|reference|, pad columns zeroed, rows beyond untouched.

Measured on the MI355X (records for a later change to compare with, not gates; the tests print them again):
(a) worst token_err(kernel, exact) / e_model over the nine N and the three gradients (the gate is 2), and worst token_err(kernel, model):
        (32, 128)   x3 1.0001, 6.2e-4     f32mfma 1.0000, 1.9e-5
        (64, 256)   x3 1.0000, 6.0e-4     f32mfma 1.0000, 7.2e-4
        (128, 512)  x3 1.0000, 1.0e-3     f32mfma 1.0000, 6.1e-4
    over all 150 gated figures the ratio lies in [0.9999, 1.0001]: the kernel makes the model's roundings and hardly anything else; where it
    differs from the model at all (most rows: below 1e-5) a P or dS fell to the other bf16 neighbour.  x3 against f32mfma, worst token_err:
    2.5e-3, 9.0e-3, 9.2e-3 for the three widths.  N = 1: |d theta|, |d phi| at most 6.1e-4 of single_token_bound ((32, 128): exactly 0).
(b) worst rel 1.7e-6 in both calling forms.  (c) 2.7e-6 at (4, 32), 2.3e-6 at (64, 256).  (d) 2.3e-7.  The module: 82 tests in 3 s.
"""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_bwd_cases as K                        # noqa: E402
import attn_core_cases as A                       # noqa: E402
from attn_bwd_cases import SENT, roundup          # noqa: E402
from gpu_common import TOL, dev, rel              # noqa: E402,F401  (dev: fixture)
from gssd import _lib                             # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
T0 = time.time()
SPENT = {}                  # family -> seconds inside its tests so far
NAN = float('nan')


def worst(family, value):
    WORST[family] = max(WORST.get(family, 0.), float(value))
    print(f'worst so far, {family}: {WORST[family]:.5g}')


@pytest.fixture
def clock(request):
    """Prints the time spent in the test's family, (a) to (d), and into the module."""
    family = request.function.__doc__.split(':')[0]
    t = time.time()
    yield
    SPENT[family] = SPENT.get(family, 0.) + time.time() - t
    print(f'{family}: {SPENT[family]:.1f} s in this family, {time.time() - T0:.1f} s into the module')


def stream():
    return torch.cuda.current_stream().cuda_stream


def absmax(t):
    return float(t.abs().max())


def with_nan_rows(t, rows, device, dtype=torch.float32):
    """[B][N][C] or [B][N] float64 -> device [B N + 3][C] or [B N + 3] of dtype, the three rows beyond B N NaN."""
    flat = t.reshape(rows, -1).float()
    out = torch.full((rows + 3, flat.shape[1]), NAN)
    out[:rows] = flat
    out = out.to(dtype).to(device)
    return out.view(-1) if t.dim() == 2 else out


# --------------------------------------------------------------------------------------------------
# (a) gssd_self_attn_flash_bwd_bf16
# --------------------------------------------------------------------------------------------------
BF16_RESULTS = {}           # (D, C2, N) -> {form: the gradients, float64}: the two forms of a row are compared when the second has run


@pytest.mark.parametrize('D,C2,N,form', K.FLASH_BF16_ROWS, ids=[K.bf16_id(*r) for r in K.FLASH_BF16_ROWS])
def test_flash_bwd_bf16(dev, clock, D, C2, N, form):
    """(a): one row of FLASH_BF16_ROWS; the own-keys and the own-queries instance of its width and logit form."""
    lib = _lib.lib
    B, x3 = K.B, dict(K.FLASH_BF16_FORMS)[form]
    what = K.bf16_id(D, C2, N, form)
    c = K.flash_bf16_case(D, C2, N)
    ex, mo, gate = K.exact(c), K.model(c, x3), K.e_model(D, C2, N, x3)
    M, CT = B * N, 2 * D + C2
    assert lib.gssd_self_attn_flash_bwd_supported(D, C2) == 1
    tp = with_nan_rows(torch.cat((c['th'], c['ph']), -1), M, dev)
    tph, tpl = torch.empty_like(tp, dtype=torch.bfloat16), torch.empty_like(tp, dtype=torch.bfloat16)
    _lib.check(lib.gssd_cast_split_f32_bf16(tp.data_ptr(), tph.data_ptr(), tpl.data_ptr(), tp.numel(), stream()))
    assert torch.equal(tph[:M], tp[:M].to(torch.bfloat16)) and torch.equal(tpl[:M], (tp[:M] - tph[:M].float()).to(torch.bfloat16))
    assert bool(torch.isnan(tph[M:].float()).all()) and bool(torch.isnan(tpl[M:].float()).all())
    g16, dag16 = with_nan_rows(c['g'], M, dev, torch.bfloat16), with_nan_rows(c['dag'], M, dev, torch.bfloat16)
    assert torch.equal(g16[:M].double().cpu().view(B, N, C2), c['g'])                    # the table's g is bf16-representable
    lse, dvec = with_nan_rows(c['lse'], M, dev), with_nan_rows(c['dvec'], M, dev)
    assert tp.shape == (M + 3, 2 * D) and g16.shape == dag16.shape == (M + 3, C2) and lse.shape == dvec.shape == (M + 3,)

    def run():
        out = torch.full((M + 3, CT), SENT, device=dev)
        _lib.check(lib.gssd_self_attn_flash_bwd_bf16(tp.data_ptr(), tph.data_ptr(), tpl.data_ptr() if x3 else None, g16.data_ptr(), dag16.data_ptr(),
                                                     lse.data_ptr(), dvec.data_ptr(), out.data_ptr(), B, N, D, C2, stream()))
        torch.cuda.synchronize()
        return out
    out = run()
    assert bool(torch.isfinite(out[:M]).all()), f'{what}: {int((~torch.isfinite(out[:M])).sum())} non-finite gradients'
    assert not bool((out[:M] == SENT).any()), f'{what}: {int((out[:M] == SENT).sum())} gradients were never written'
    assert bool((out[M:] == SENT).all()), f'{what}: rows beyond B N were written'
    got = out[:M].double().cpu().view(B, N, CT)
    got = dict(dtheta=got[..., :D], dphi=got[..., D:2 * D], dg=got[..., 2 * D:])
    width = f'({D}, {C2}) {form}'
    for k in K.GRADS:
        if N == 1 and k != 'dg':
            bound = K.single_token_bound(c)[0 if k == 'dtheta' else 1]
            w = got[k].abs().amax(dim=(1, 2))
            print(f'{what} {k}: max |.| per image {w.tolist()}, bound {bound.tolist()}  (model: {mo[k].abs().amax(dim=(1, 2)).tolist()})')
            assert bool((w <= bound).all()), (what, k, w.tolist(), bound.tolist())
            worst(f'(a) {width}: N = 1 |d theta|, |d phi| / bound', float((w / bound).max()))
            continue
        e, e_mo = K.token_err(got[k], ex[k]), K.token_err(got[k], mo[k])
        print(f'{what} {k}: token_err(kernel, exact) {e:.3e}, e_model {gate[k]:.3e}, ratio {e / max(gate[k], 1e-300):.4f}; '
              f'token_err(kernel, model) {e_mo:.3e}')
        assert e <= 2 * gate[k], f'{what} {k}: token_err(kernel, exact) {e:.3e} > 2 e_model = {2 * gate[k]:.3e}'
        if gate[k] > 0:
            worst(f'(a) {width}: token_err(kernel, exact) / e_model', e / gate[k])
        worst(f'(a) {width}: token_err(kernel, model)', e_mo)
    # no atomics: the same bits again
    out2 = run()
    assert torch.equal(out2, out), f'{what}: a second call changes {int((out2 != out).sum())} values'
    # recorded, not gated: the two logit forms against each other
    other = BF16_RESULTS.setdefault((D, C2, N), {})
    other[form] = out[:M].double().cpu().view(B, N, CT)
    if len(other) == 2 and N > 1:
        a, b = other['x3'], other['f32mfma']
        d = max(K.token_err(a[..., lo:hi], b[..., lo:hi]) for lo, hi in ((0, D), (D, 2 * D), (2 * D, CT)))
        print(f'{K.bf16_id(D, C2, N)}: x3 against f32mfma, largest token_err {d:.3e}')
        worst(f'(a) ({D}, {C2}): x3 against f32mfma', d)


# --------------------------------------------------------------------------------------------------
# (b) gssd_self_attn_flash_bwd_f32
# --------------------------------------------------------------------------------------------------
def zero_aware(got, ref, largest):
    """rel(got, ref); where the reference is identically zero (a single key: P = 1, dS = 0) max |got| over the case's largest gradient."""
    if absmax(ref) <= 1e-9 * largest:
        return absmax(got) / largest
    return rel(got, ref)


@pytest.mark.parametrize('N,Nk,form', K.FLASH_F32_ROWS, ids=[K.f32_id(*r) for r in K.FLASH_F32_ROWS])
def test_flash_bwd_f32(dev, clock, N, Nk, form):
    """(b): one row of FLASH_F32_ROWS in the calling form of gssd/bwd_ops.py its id names."""
    lib = _lib.lib
    (D, C2), B = K.FLASH_F32_WIDTH, K.B
    what = K.f32_id(N, Nk, form)
    c = K.kv_case(D, C2, N, Nk, what)
    assert lib.gssd_self_attn_flash_bwd_f32_supported(D, C2) == 1
    dag, lse, dvec = c['dag'].float().to(dev), c['lse'].float().to(dev), c['dvec'].float().to(dev)
    if form == 'pooled':
        tp, keys, krow, gT, Nkp = (t.to(dev) if torch.is_tensor(t) else t for t in A.pooled_buffers(c, D, C2, N, Nk, B))
        assert krow == D + 4 and bool(torch.isnan(keys[..., D:]).all())
        ld_q, ld_kv = D + 4, D + C2 + 8
    else:
        assert N == Nk
        tp, gT, Nkp = A.in_place_buffers(c, D, C2, N, B)
        tp, gT = tp.to(dev), gT.to(dev)
        keys, krow = tp[0, 0, D:], 2 * D
        ld_q = ld_kv = 2 * D + C2

    def run():
        dq = torch.full((B * N + 3, ld_q), SENT, device=dev)
        if form == 'pooled':
            dkv = torch.full((B * Nk + 3, ld_kv), SENT, device=dev)
            dk, dv = dkv, dkv[0, D:]
        else:
            dkv = dq
            dk, dv = dq[0, D:], dq[0, 2 * D:]
        _lib.check(lib.gssd_self_attn_flash_bwd_f32(tp.data_ptr(), 2 * D, keys.data_ptr(), krow, gT.data_ptr(), Nkp, dag.data_ptr(), lse.data_ptr(),
                                                    dvec.data_ptr(), dq.data_ptr(), ld_q, dk.data_ptr(), dv.data_ptr(), ld_kv, B, N, Nk, D, C2,
                                                    stream()))
        torch.cuda.synchronize()
        return dq, dkv
    dq, dkv = run()
    k0 = 0 if form == 'pooled' else D
    got = dict(dq=dq[:B * N, :D].reshape(B, N, D), dk=dkv[:B * Nk, k0:k0 + D].reshape(B, Nk, D),
               dv=dkv[:B * Nk, k0 + D:k0 + D + C2].reshape(B, Nk, C2))
    largest = max(absmax(c[k]) for k in ('dq', 'dk', 'dv'))
    e = {k: zero_aware(got[k], c[k], largest) for k in ('dq', 'dk', 'dv')}
    print(f'{what}: dq {e["dq"]:.2e} dk {e["dk"]:.2e} dv {e["dv"]:.2e}')
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), what
    assert max(e.values()) < TOL, (what, e)
    # slack columns and trailing rows keep the sentinel
    assert bool((dq[B * N:] == SENT).all()) and bool((dkv[B * Nk:] == SENT).all()), f'{what}: rows beyond were written'
    if form == 'pooled':
        assert bool((dq[:, D:] == SENT).all()) and bool((dkv[:, D + C2:] == SENT).all()), f'{what}: slack columns were written'
    else:
        assert not bool((dq[:B * N] == SENT).any())
    dq2, dkv2 = run()
    assert torch.equal(dq2, dq) and torch.equal(dkv2, dkv), f'{what}: a second call gives other bits'
    worst(f'(b) flash_bwd_f32 {form}', max(e.values()))


# --------------------------------------------------------------------------------------------------
# (c) the explicit chain of gssd/bwd_ops.py::_sa_explicit, lse branch, pooled-key form
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,C2,N,Nk', K.CHAIN_ROWS, ids=[K.chain_id(*r) for r in K.CHAIN_ROWS])
def test_explicit_chain(dev, clock, D, C2, N, Nk):
    """(c): A = exp(theta keys^T - lse), D, dS, d theta, d keys, d values: six launches over NaN-prefilled maps."""
    lib = _lib.lib
    B = K.B
    what = K.chain_id(D, C2, N, Nk)
    c = K.kv_case(D, C2, N, Nk, what)
    C8, C4, CT, CW = D, 2 * D, 2 * D + C2, D + C2                       # the names of _sa_explicit
    tp, keys, krow, vals, Nkp = (t.to(dev) if torch.is_tensor(t) else t for t in A.pooled_buffers(c, D, C2, N, Nk, B))
    assert Nkp == roundup(Nk, 4) > Nk and krow == C8 + 4 and bool(torch.isnan(keys[..., C8:]).all())
    dag, ag, lse = c['dag'].float().to(dev), c['out'].float().to(dev), c['lse'].float().to(dev)
    Amap = torch.full((B, N, Nkp), NAN, device=dev)
    dA = torch.full((B, N, Nkp), NAN, device=dev)
    Dv = torch.full((B * N + 3,), SENT, device=dev)
    dtpg = torch.full((B * N + 3, CT), SENT, device=dev)
    dkg = torch.full((B * Nk + 3, CW), SENT, device=dev)
    s = stream()
    _lib.check(lib.gssd_bgemm_ex_f32(tp.data_ptr(), keys.data_ptr(), Amap.data_ptr(), N, Nk, C8, C4, krow, Nkp, 0, 1, N * C4, Nk * krow, N * Nkp, B, 1.0,
                                     1, lse.data_ptr(), None, s))
    _lib.check(lib.gssd_rowdot_f32(dag.data_ptr(), ag.data_ptr(), Dv.data_ptr(), B * N, C2, s))
    _lib.check(lib.gssd_bgemm_ex_f32(dag.data_ptr(), vals.data_ptr(), dA.data_ptr(), N, Nk, C2, C2, Nkp, Nkp, 0, 0, N * C2, C2 * Nkp, N * Nkp, B, 1.0,
                                     2, Dv.data_ptr(), Amap.data_ptr(), s))
    _lib.check(lib.gssd_bgemm_f32(dA.data_ptr(), keys.data_ptr(), dtpg.data_ptr(), N, C8, Nk, Nkp, krow, CT, 0, 0, N * Nkp, Nk * krow, N * CT, B, 1.0, 0,
                                  s))
    _lib.check(lib.gssd_bgemm_f32(dA.data_ptr(), tp.data_ptr(), dkg.data_ptr(), Nk, C8, N, Nkp, C4, CW, 1, 0, N * Nkp, N * C4, Nk * CW, B, 1.0, 0, s))
    _lib.check(lib.gssd_bgemm_f32(Amap.data_ptr(), dag.data_ptr(), dkg[0, C8:].data_ptr(), Nk, C2, N, Nkp, C2, CW, 1, 0, N * Nkp, N * C2, Nk * CW, B,
                                  1.0, 0, s))
    torch.cuda.synchronize()
    got = dict(dq=dtpg[:B * N, :C8].reshape(B, N, C8), dk=dkg[:B * Nk, :C8].reshape(B, Nk, C8), dv=dkg[:B * Nk, C8:].reshape(B, Nk, C2))
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), f'{what}: a pad column or a slack float was read'
    assert bool(torch.isfinite(Amap[..., :Nk]).all()) and bool(torch.isfinite(dA[..., :Nk]).all())
    largest = max(absmax(c[k]) for k in ('dq', 'dk', 'dv'))
    e = {k: zero_aware(got[k], c[k], largest) for k in ('dq', 'dk', 'dv')}
    e_map = rel(Amap[..., :Nk], torch.exp(c['th'] @ c['ks'].transpose(1, 2) - c['lse'].unsqueeze(-1)))
    print(f'{what}: dq {e["dq"]:.2e} dk {e["dk"]:.2e} dv {e["dv"]:.2e}  (A {e_map:.2e}, D {rel(Dv[:B * N].view(B, N), c["dvec"]):.2e})')
    assert max(e.values()) < TOL and e_map < TOL, (what, e, e_map)
    # nothing wrote the pad columns either, nor anything beyond the gradients
    assert bool(torch.isnan(Amap[..., Nk:]).all()) and bool(torch.isnan(dA[..., Nk:]).all()), f'{what}: pad columns [Nk, Nkp) were written'
    assert bool((dtpg[:, C8:] == SENT).all()) and bool((dtpg[B * N:] == SENT).all()) and bool((dkg[B * Nk:] == SENT).all())
    assert bool((Dv[B * N:] == SENT).all())
    worst(f'(c) explicit chain ({D}, {C2})', max(e.values()))


# --------------------------------------------------------------------------------------------------
# (d) gssd_softmax_bwd_rows_f32
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,n,stride', K.SOFTMAX_BWD, ids=[K.softmax_id(*r) for r in K.SOFTMAX_BWD])
def test_softmax_bwd_rows(dev, clock, rows, n, stride):
    """(d): dattn <- attn o (dattn - rowsum(attn o dattn)) in place, the path taken when no log-sum-exp was kept."""
    attn, dattn, ref = K.softmax_bwd_case(rows, n, stride)
    a, d = attn.to(dev), dattn.to(dev)
    _lib.check(_lib.lib.gssd_softmax_bwd_rows_f32(a.data_ptr(), d.data_ptr(), rows, n, stride, stream()))
    torch.cuda.synchronize()
    scale = max(absmax(ref), 1e-30)
    # a single column: A = 1 and the reference is identically zero -- held against the input instead
    e = float((d[:rows, :n].double().cpu() - ref).abs().max()) / (scale if n > 1 else absmax(dattn[:rows, :n]))
    print(f'{K.softmax_id(rows, n, stride)}: {e:.2e}')
    assert bool(torch.isfinite(d[:rows]).all()) and e < 1e-5
    assert bool((d[:rows, n:] == 0).all()), 'the pad columns [n, stride) come back zero'
    assert bool((d[rows:] == SENT).all()), 'rows beyond were written'
    assert torch.equal(a.cpu()[:, :n], attn[:, :n]) and bool(torch.isnan(a[:, n:]).all())
    worst('(d) softmax_bwd_rows', e)
