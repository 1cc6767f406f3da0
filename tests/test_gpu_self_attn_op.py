"""The standalone, differentiable Self_Attn (gssd.modules.Self_Attn.forward -> gssd/self_attn_op.py) and the two any-size kernels under it
(csrc/sa_any.hip) on the MI355X, against oracle.gssd_oracle.self_attn in float64 on the CPU (values) and float64 autograd through it
(gradients; loss = (out r1).sum() + (sigma_attn_g r2).sum() with fixed random r1, r2).

Inputs: sigma 0.7, weights uniform in +-1/sqrt(fan_in), x ~ N(0, 1) * scale, and u / v after 10 power iterations on the CPU, so sigma_sn is
the true spectral norm (with raw random u / v the normalised weights blow up and the softmax saturates).

Bounds.  Forward: TOL = 1e-4 (max-abs error over max-abs reference).  Gradients: max(1e-4, 8 e32), e32 = the deviation of CPU fp32
autograd through the same oracle on the same inputs, per tensor, computed here; the factor 8 allows for the different summation order of
MFMA reductions.  A gradient whose float64 reference is zero (phi's bias always: it shifts every logit of a query alike; all of theta and
phi with a single key) is compared absolutely: |grad| <= 1e-4 max|grad theta.bias| (phi's bias), or 1e-4 times the largest gradient of the
case where that one is zero too.  "Zero" = below 1e-9 of the case's largest gradient: float64 rounding noise sits at 1e-16, and a true
gradient that small is below the resolution of the fp32 result it would be compared with.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from attn_core_cases import SENT, core_buffers, core_case     # float64 cases of the cores, shared with tests/test_gpu_attn_cores.py
from gpu_common import TOL, dev, rel              # noqa: F401  (dev: fixture)
from gssd import _lib
from gssd.modules import Self_Attn
from oracle import gssd_oracle as O

pytestmark = pytest.mark.gpu

NAMES = ('theta', 'phi', 'g', 'attn')
PARAMS = [f'snconv1x1_{n}.{k}' for n in NAMES for k in ('weight_orig', 'bias')] + ['sigma']
CASES = [(8, 5, 2, 1, 1), (24, 9, 3, 1, 1), (40, 9, 2, 2, 1), (64, 13, 2, 1, 1), (64, 5, 2, 8, 1), (136, 9, 2, 1, 1), (264, 9, 1, 3, 1),
         (520, 9, 2, 1, 1), (2048, 5, 1, 1, 1), (64, 13, 2, 1, 6), (128, 17, 1, 1, 3)]          # (C, H, B, max_pool_factor, x scale)
MODES = ('train', 'eval')


def _ids(c):
    return 'C%d-H%d-B%d-mpf%d-x%d' % c


@functools.lru_cache(maxsize=None)
def make_inputs(Cc, H, B, scale, seed=0, n_x=1, sigma=0.7):
    """fp32-representable inputs (float32 tensors): state dict without prefix, and n_x inputs with their loss weights."""
    g = torch.Generator().manual_seed(1000 * Cc + 10 * H + B + seed)
    sd = {}
    for n, (co, ci) in zip(NAMES, ((Cc // 8, Cc), (Cc // 8, Cc), (Cc // 2, Cc), (Cc, Cc // 2))):
        bound = 1.0 / math.sqrt(ci)
        w = ((torch.rand(co, ci, 1, 1, generator=g, dtype=torch.float64) * 2 - 1) * bound).float()
        b = ((torch.rand(co, generator=g, dtype=torch.float64) * 2 - 1) * bound).float()
        wm = w.double().view(co, ci)
        u = F.normalize(torch.randn(co, generator=g, dtype=torch.float64), dim=0)
        v = F.normalize(torch.randn(ci, generator=g, dtype=torch.float64), dim=0)
        for _ in range(10):
            v = F.normalize(wm.t() @ u, dim=0, eps=1e-12)
            u = F.normalize(wm @ v, dim=0, eps=1e-12)
        p = f'snconv1x1_{n}.'
        sd[p + 'weight_orig'], sd[p + 'bias'], sd[p + 'weight_u'], sd[p + 'weight_v'] = w, b, u.float(), v.float()
    sd['sigma'] = torch.full((1,), sigma, dtype=torch.float32)
    xs = [(torch.randn(B, Cc, H, H, generator=g, dtype=torch.float64) * scale).float() for _ in range(n_x)]
    rs = [(torch.randn(B, Cc, H, H, generator=g, dtype=torch.float64).float(), torch.randn(B, Cc, H, H, generator=g, dtype=torch.float64).float())
          for _ in range(n_x)]
    return sd, xs, rs


def oracle_run(sd, xs, rs, mpf, training, dtype, x_grad=True):
    """The oracle on the CPU in ``dtype``: forwards over ``xs`` in order (train mode carries u / v from one to the next), one backward of
    the summed losses.  Returns (outputs per forward, gradients {name: tensor} with 'x<i>', u / v after-state)."""
    state = {'sa.' + k: v.to(dtype).clone() for k, v in sd.items()}
    for k in PARAMS:
        state['sa.' + k].requires_grad_(True)
    xl = [x.to(dtype).clone().requires_grad_(x_grad) for x in xs]
    loss, outs = 0, []
    for x, (r1, r2) in zip(xl, rs):
        upd = {}
        out, o2, attn = O.self_attn(x, state, 'sa', training, mpf, upd)
        state.update({k: v.detach() for k, v in upd.items()})
        loss = loss + (out * r1.to(dtype)).sum() + (o2 * r2.to(dtype)).sum()
        outs.append((out.detach(), o2.detach(), attn.detach()))
    loss.backward()
    grads = {k: state['sa.' + k].grad for k in PARAMS}
    for i, x in enumerate(xl):
        grads[f'x{i}'] = x.grad
    after = {k[3:]: v for k, v in state.items() if k.endswith(('weight_u', 'weight_v'))}
    return outs, grads, after


@functools.lru_cache(maxsize=None)
def reference(case, mode, n_x=1, sigma=0.7):
    Cc, H, B, mpf, scale = case
    sd, xs, rs = make_inputs(Cc, H, B, scale, n_x=n_x, sigma=sigma)
    r64 = oracle_run(sd, xs, rs, mpf, mode == 'train', torch.float64)
    r32 = oracle_run(sd, xs, rs, mpf, mode == 'train', torch.float32)
    return r64, r32


def build(case, mode, device, sigma=0.7, n_x=1):
    Cc, H, B, mpf, scale = case
    sd, xs, rs = make_inputs(Cc, H, B, scale, n_x=n_x, sigma=sigma)
    m = Self_Attn(Cc, mpf)
    m.load_state_dict(sd)
    m = m.to(device)
    m.train(mode == 'train')
    return m, [x.to(device) for x in xs], [(a.to(device), b.to(device)) for a, b in rs]


def device_grads(m, xs, rs, x_grad=True):
    xl = [x.clone().requires_grad_(x_grad) for x in xs]
    loss = 0
    for x, (r1, r2) in zip(xl, rs):
        out, o2 = m(x)
        loss = loss + (out * r1).sum() + (o2 * r2).sum()
    loss.backward()
    sdp = dict(m.named_parameters())
    grads = {k: sdp[k].grad for k in PARAMS}
    for i, x in enumerate(xl):
        grads[f'x{i}'] = x.grad
    return grads


def absmax(t):
    return float(t.detach().abs().max())


def check_grads(got, r64, r32, names=None, log=None):
    """The bound of the module docstring for every gradient in ``names`` (default: all of r64).  Returns the worst relative deviation."""
    names = list(r64) if names is None else names
    largest = max(absmax(v) for v in r64.values())
    tb = absmax(r64['snconv1x1_theta.bias'])
    worst = 0.0
    for k in names:
        ref, g = r64[k], got[k]
        assert g is not None, f'{k}: no gradient'
        assert tuple(g.shape) == tuple(ref.shape), k
        g = g.detach().cpu().double()
        if absmax(ref) <= 1e-9 * largest:
            scale = tb if (k == 'snconv1x1_phi.bias' and tb > 1e-9 * largest) else largest
            err = absmax(g) / scale
            print(f'  {k}: zero reference, |grad| / scale = {err:.2e}')
            assert err <= 1e-4, (k, err)
            continue
        e32 = absmax(r32[k].double() - ref) / absmax(ref)
        err = absmax(g - ref) / absmax(ref)
        print(f'  {k}: gpu {err:.2e}  cpu-fp32 {e32:.2e}')
        worst = max(worst, err)
        assert err <= max(1e-4, 8 * e32), (k, err, e32)
    if log is not None:
        print(f'{log}: worst gradient deviation {worst:.2e}')
    return worst


# --------------------------------------------------------------------------------------------------
# module
# --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_forward(dev, case, mode):
    (outs, _, after), _ = reference(case, mode)
    out_r, o2_r, attn_r = outs[0]
    m, xs, _ = build(case, mode, dev)
    before = {k: v.clone() for k, v in m.state_dict().items() if k.endswith(('weight_u', 'weight_v'))}
    with torch.no_grad():
        out, o2, attn = m(xs[0], return_attn_map=True)
        out_b, o2_b = m.eval()(xs[0]) if mode == 'eval' else (None, None)
    Cc, H, B, mpf, _ = case
    Nk = max(H // mpf, 1) ** 2
    assert tuple(out.shape) == tuple(o2.shape) == (B, Cc, H, H) and tuple(attn.shape) == (B, H * H, Nk)
    e = rel(out, out_r), rel(o2, o2_r), rel(attn, attn_r)
    print(f'{_ids(case)} {mode}: out {e[0]:.2e} sigma*attn_g {e[1]:.2e} attn {e[2]:.2e}')
    assert max(e) < TOL, e
    now = {k: v for k, v in m.state_dict().items() if k in before}
    if mode == 'train':
        for k in before:
            assert rel(now[k], after[k]) < TOL, k
    else:
        assert all(torch.equal(now[k], before[k]) for k in before)
        assert torch.equal(out, out_b) and torch.equal(o2, o2_b)        # without the map: the same values


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_gradients(dev, case, mode):
    (_, g64, _), (_, g32, _) = reference(case, mode)
    m, xs, rs = build(case, mode, dev)
    got = device_grads(m, xs, rs)
    check_grads(got, g64, g32, log=f'{_ids(case)} {mode}')


def test_wide_block_on_a_large_map(dev):
    """4096 tokens, 512 channels: the shapes at which the projection, the output conv and their data gradients go to csrc/conv_x6.hip
    (ops.x6_wanted); 64 pooled keys keep the float64 reference small.  Same bounds as every other case."""
    case = (512, 64, 1, 8, 1)
    (outs, g64, _), (_, g32, _) = reference(case, 'train')
    m, xs, rs = build(case, 'train', dev)
    with torch.no_grad():
        out, o2, attn = m.eval()(xs[0], return_attn_map=True)
    (outs_e, _, _), _ = reference(case, 'eval')
    e = rel(out, outs_e[0][0]), rel(o2, outs_e[0][1]), rel(attn, outs_e[0][2])
    print(f'{_ids(case)} eval: out {e[0]:.2e} sigma*attn_g {e[1]:.2e} attn {e[2]:.2e}')
    assert max(e) < TOL, e
    check_grads(device_grads(m.train(), xs, rs), g64, g32, log=f'{_ids(case)} train')


def test_default_sigma_zero(dev):
    case = (64, 13, 2, 1, 1)
    (_, g64, _), (_, g32, _) = reference(case, 'train', sigma=0.0)
    m, xs, rs = build(case, 'train', dev, sigma=0.0)
    x = xs[0].clone().requires_grad_(True)
    out, o2 = m(x)
    assert torch.equal(out.detach(), xs[0]) and not o2.detach().any()
    ((out * rs[0][0]).sum() + (o2 * rs[0][1]).sum()).backward()
    sdp = dict(m.named_parameters())
    check_grads({'sigma': sdp['sigma'].grad}, g64, g32, names=['sigma'])
    for k in PARAMS[:-1]:
        assert sdp[k].grad is not None and not sdp[k].grad.any(), k
    assert torch.equal(x.grad, rs[0][0])
    fresh = Self_Attn(64).to(dev)
    assert float(fresh.sigma.detach()) == 0.0 and torch.equal(fresh(xs[0])[0], xs[0])


def test_two_forwards_one_backward(dev):
    case = (40, 9, 2, 2, 1)
    (_, g64, after), (_, g32, _) = reference(case, 'train', n_x=2)
    m, xs, rs = build(case, 'train', dev, n_x=2)
    got = device_grads(m, xs, rs)
    check_grads(got, g64, g32, log='two forwards, one backward')
    for k, v in after.items():
        assert rel(m.state_dict()[k], v) < TOL, k


def test_train_mode_under_no_grad_updates_u_v(dev):
    case = (24, 9, 3, 1, 1)
    (_, _, after), _ = reference(case, 'train')
    m, xs, _ = build(case, 'train', dev)
    before = {k: v.clone() for k, v in m.state_dict().items() if k in after}
    with torch.no_grad():
        m(xs[0])
    for k, v in after.items():
        assert not torch.equal(m.state_dict()[k], before[k]) and rel(m.state_dict()[k], v) < TOL, k


def test_x_without_grad(dev):
    case = (136, 9, 2, 1, 1)
    (_, g64, _), (_, g32, _) = reference(case, 'eval')
    m, xs, rs = build(case, 'eval', dev)
    got = device_grads(m, xs, rs, x_grad=False)
    assert got['x0'] is None
    check_grads(got, g64, g32, names=PARAMS)


def test_frozen_parameters(dev):
    case = (24, 9, 3, 1, 1)
    (_, g64, _), (_, g32, _) = reference(case, 'eval')
    m, xs, rs = build(case, 'eval', dev)
    for p in m.snconv1x1_g.parameters():
        p.requires_grad_(False)
    got = device_grads(m, xs, rs)
    assert got['snconv1x1_g.weight_orig'] is None and got['snconv1x1_g.bias'] is None
    check_grads(got, g64, g32, names=[k for k in g64 if not k.startswith('snconv1x1_g.')])
    # nothing but sigma: the attention backward is not needed at all
    m2, xs, rs = build(case, 'eval', dev)
    for k, p in m2.named_parameters():
        p.requires_grad_(k == 'sigma')
    got = device_grads(m2, xs, rs, x_grad=False)
    check_grads(got, g64, g32, names=['sigma'])
    assert all(got[k] is None for k in PARAMS[:-1])


def test_noncontiguous_and_channels_last_input(dev):
    case = (40, 9, 2, 2, 1)
    m, xs, _ = build(case, 'eval', dev)
    x = xs[0]
    with torch.no_grad():
        want = m(x)
        cl = x.contiguous(memory_format=torch.channels_last)
        wide = torch.zeros(2, 40, 9, 12, device=dev)
        wide[..., 1:10] = x
        nc = wide[..., 1:10]
        assert not nc.is_contiguous() and not cl.is_contiguous()
        for y in (cl, nc):
            got = m(y)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_memory_stays_below_one_map(dev):
    """(C 64, H 64, B 4): one [4, 4096, 4096] fp32 map is 268 MB and the explicit path needs two."""
    torch.manual_seed(5)
    m = Self_Attn(64).to(dev).train()
    with torch.no_grad():
        m.sigma.fill_(0.7)
    x = torch.randn(4, 64, 64, 64, device=dev, requires_grad=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, o2 = m(x)
    (out.sum() + o2.sum()).backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print(f'forward + backward peak growth: {grew / 2 ** 20:.1f} MB')
    assert grew < 128 * 2 ** 20
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


# --------------------------------------------------------------------------------------------------
# kernels, through the C ABI
# --------------------------------------------------------------------------------------------------
WIDTHS = [(4, 4), (4, 16), (20, 68), (36, 132), (68, 260), (256, 1024)]
TOKENS = [(25, 25), (81, 16), (169, 169), (25, 1)]


@pytest.mark.parametrize('N,Nk', TOKENS)
@pytest.mark.parametrize('D,C2', WIDTHS)
def test_core_any_forward(dev, D, C2, N, Nk):
    B = 2
    c = core_case(D, C2, N, Nk)
    tp, keys, krow, gT, Nkp = core_buffers(c, D, C2, N, Nk, dev)
    out = torch.full((B * N + 3, C2), SENT, device=dev)
    lse = torch.full((B * N + 3,), SENT, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.lib.gssd_self_attn_core_any_f32(tp.data_ptr(), keys.data_ptr(), gT.data_ptr(), out.data_ptr(), B, N, Nk, Nkp, D, C2, krow,
                                                    lse.data_ptr(), s))
    e = rel(out[:B * N].view(B, N, C2), c['out']), rel(lse[:B * N].view(B, N), c['lse'])
    print(f'core_any ({D}, {C2}) N {N} Nk {Nk}: out {e[0]:.2e} lse {e[1]:.2e}')
    assert max(e) < TOL, e
    assert bool((out[B * N:] == SENT).all()) and bool((lse[B * N:] == SENT).all())
    # lse is optional
    out2 = torch.empty(B, N, C2, device=dev)
    _lib.check(_lib.lib.gssd_self_attn_core_any_f32(tp.data_ptr(), keys.data_ptr(), gT.data_ptr(), out2.data_ptr(), B, N, Nk, Nkp, D, C2, krow,
                                                    None, s))
    assert torch.equal(out2.view(-1, C2), out[:B * N])


def run_bwd(fn, c, D, C2, N, Nk, device, B=2):
    tp, keys, krow, gT, Nkp = core_buffers(c, D, C2, N, Nk, device)
    ld_q, ld_kv = D + 4, D + C2 + 8
    dag, lse, dvec = c['dag'].float().to(device), c['lse'].float().to(device), c['dvec'].float().to(device)
    dq = torch.full((B * N + 3, ld_q), SENT, device=device)
    dkv = torch.full((B * Nk + 3, ld_kv), SENT, device=device)
    _lib.check(fn(tp.data_ptr(), 2 * D, keys.data_ptr(), krow, gT.data_ptr(), Nkp, dag.data_ptr(), lse.data_ptr(), dvec.data_ptr(),
                  dq.data_ptr(), ld_q, dkv.data_ptr(), dkv[0, D:].data_ptr(), ld_kv, B, N, Nk, D, C2, torch.cuda.current_stream().cuda_stream))
    return dq, dkv


@pytest.mark.parametrize('N,Nk', TOKENS)
@pytest.mark.parametrize('D,C2', WIDTHS)
def test_flash_bwd_any(dev, D, C2, N, Nk):
    B = 2
    c = core_case(D, C2, N, Nk)
    fn = _lib.lib.gssd_self_attn_flash_bwd_any_f32
    dq, dkv = run_bwd(fn, c, D, C2, N, Nk, dev)
    # a single key makes P = 1 and dS = 0: dq and dk are zero, and are held absolutely against the case's largest gradient (module docstring)
    largest = max(absmax(c[k]) for k in ('dq', 'dk', 'dv'))

    def dev_of(got, ref):
        if absmax(ref) <= 1e-9 * largest:
            return absmax(got) / largest
        return rel(got, ref)
    e = (dev_of(dq[:B * N, :D].reshape(B, N, D), c['dq']), dev_of(dkv[:B * Nk, :D].reshape(B, Nk, D), c['dk']),
         dev_of(dkv[:B * Nk, D:D + C2].reshape(B, Nk, C2), c['dv']))
    print(f'flash_bwd_any ({D}, {C2}) N {N} Nk {Nk}: dq {e[0]:.2e} dk {e[1]:.2e} dv {e[2]:.2e}')
    assert max(e) < TOL, e
    # columns beyond D / C2 and rows beyond N / Nk come back untouched
    assert bool((dq[:, D:] == SENT).all()) and bool((dq[B * N:] == SENT).all())
    assert bool((dkv[:, D + C2:] == SENT).all()) and bool((dkv[B * Nk:] == SENT).all())
    dq2, dkv2 = run_bwd(fn, c, D, C2, N, Nk, dev)
    assert torch.equal(dq, dq2) and torch.equal(dkv, dkv2)            # no atomics: bit-reproducible


def test_generic_backward_agrees_with_the_16_64_instance(dev):
    D, C2, N, Nk = 16, 64, 169, 81
    c = core_case(D, C2, N, Nk)
    a = run_bwd(_lib.lib.gssd_self_attn_flash_bwd_any_f32, c, D, C2, N, Nk, dev)
    b = run_bwd(_lib.lib.gssd_self_attn_flash_bwd_f32, c, D, C2, N, Nk, dev)
    B = 2
    assert rel(a[0][:B * N, :D], b[0][:B * N, :D]) < TOL
    assert rel(a[1][:B * Nk, :D], b[1][:B * Nk, :D]) < TOL and rel(a[1][:B * Nk, D:D + C2], b[1][:B * Nk, D:D + C2]) < TOL
    assert rel(a[0][:B * N, :D].reshape(B, N, D), c['dq']) < TOL


def test_generic_forward_agrees_with_the_64_256_instance(dev):
    D, C2, N, Nk, B = 64, 256, 169, 169, 2
    c = core_case(D, C2, N, Nk)
    tp, keys, krow, gT, Nkp = core_buffers(c, D, C2, N, Nk, dev)
    s = torch.cuda.current_stream().cuda_stream
    out_a, out_b = torch.empty(B, N, C2, device=dev), torch.empty(B, N, C2, device=dev)
    lse_a, lse_b = torch.empty(B, N, device=dev), torch.empty(B, N, device=dev)
    _lib.check(_lib.lib.gssd_self_attn_core_any_f32(tp.data_ptr(), keys.data_ptr(), gT.data_ptr(), out_a.data_ptr(), B, N, Nk, Nkp, D, C2, krow,
                                                    lse_a.data_ptr(), s))
    _lib.check(_lib.lib.gssd_self_attn_core_kv_f32(tp.data_ptr(), keys.data_ptr(), gT.data_ptr(), out_b.data_ptr(), B, N, Nk, Nkp, D, C2, krow, 0,
                                                   lse_b.data_ptr(), s))
    assert rel(out_a, out_b) < TOL and rel(lse_a, lse_b) < TOL and rel(out_a, c['out']) < TOL
