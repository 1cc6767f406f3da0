"""Plain torch restatement of what csrc/backward.hip's BatchNorm passes differentiate,

    raw -> z = raw * scale + shift -> ReLU -> max-pool          (NHWC, BatchNorm in training mode: scale / shift from the batch statistics)

and of its backward written out -- route d(out) to each window's first maximum, apply the ReLU mask, s1 = sum dz, s2 = sum dz raw, the
finalize formulas of bn_bwd_finalize_kernel, draw = A dz + B raw + C -- evaluated in a given dtype with the DISCONTINUOUS decisions (ReLU
mask, window arg-max) passed in.  The decisions are taken the way tests/test_gpu_grad.py::hip_decisions takes them: from the fp32 scale and
shift of gssd_bn_finalize_f32 (finalize_f32 restates that kernel's float64 arithmetic) with z as the exact product and sum rounded once.

make_inputs draws a row's operands so that no decision depends on how z is rounded: the ReLU mask and every window's arg-max agree between
separately rounded fp32 (raw * scale, then + shift), fused fp32 (one rounding) and float64 with the unrounded scale / shift; offending raw
values are redrawn, at most 8 rounds, and the agreement is asserted -- a property of the inputs alone, checked on the CPU.
"""
import zlib

import torch

EPS = 1e-5
GATE = 4             # the project's gate (tests/test_gpu_conv_leaves.py): e <= GATE * e_cpu32 + 1e-7
# family -> its own gate where a correct kernel measured above GATE on the MI355X: twice its worst measured ratio (the figures:
# tests/test_gpu_bwd_passes.py).  The BatchNorm passes: 4.03 on d(beta) of 'pool overlap'; the fp32 and the mixed entries instantiate the
# same two kernel templates (bn_bwd_reduce_kernel, bn_bwd_apply_kernel) with the same accumulation, so they are one family
GATES = {'bn_f32': 8.06, 'bn_mixed': 8.06}
_cache = {}


def gate_of(family):
    return GATES.get(family, GATE)


def bound(e32, gate=GATE):
    return gate * e32 + 1e-7


# ---- BatchNorm scale / shift ----------------------------------------------------------------------------------------------------------
def batch_stats(raw):
    """[2 C] float64: per-channel sum | sum of squares -- what a conv's epilogue leaves for gssd_bn_finalize_f32"""
    r = raw.double().reshape(-1, raw.shape[-1])
    return torch.cat([r.sum(0), (r * r).sum(0)]).contiguous()


def finalize_f64(stats, count, gamma, beta, eps=EPS):
    """(scale, shift, mean, inv) in float64, csrc/elementwise.hip::bn_finalize_kernel's arithmetic before its roundings"""
    C = gamma.numel()
    mean = stats[:C] / count
    var = (stats[C:] / count - mean * mean).clamp_min(0.0)
    inv = 1.0 / torch.sqrt(var + eps)
    sc = gamma.double() * inv
    return sc, beta.double() - mean * sc, mean, inv


def finalize_f32(stats, count, gamma, beta, eps=EPS):
    sc, sh, _, _ = finalize_f64(stats, count, gamma, beta, eps)
    return sc.float(), sh.float()


# ---- decisions ------------------------------------------------------------------------------------------------------------------------
def z_forms(raw, sc32, sh32, sc64, sh64):
    """z three ways: separately rounded fp32, fused fp32 (exact product and sum, one rounding), float64 with the unrounded scale / shift"""
    fused = (raw.double() * sc32.double() + sh32.double()).float()
    return raw * sc32 + sh32, fused, raw.double() * sc64 + sh64


def window_argmax(a, pool, last=False):
    """[B, Ho, Wo, C] int64: flat index y W + x of each window's first (last = True: last) maximum of a [B, H, W, C] in scan order"""
    k, s, p, ceil = pool
    B, H, W, C = a.shape
    from bwd_pass_cases import pool_out
    Ho, Wo = pool_out(H, k, s, p, ceil), pool_out(W, k, s, p, ceil)
    best = torch.full((B, Ho, Wo, C), float('-inf'), dtype=a.dtype)
    bidx = torch.full((B, Ho, Wo, C), -1, dtype=torch.int64)
    for dy in range(k):
        yy = torch.arange(Ho) * s - p + dy
        for dx in range(k):
            xx = torch.arange(Wo) * s - p + dx
            ok = ((yy >= 0) & (yy < H)).view(1, Ho, 1, 1) & ((xx >= 0) & (xx < W)).view(1, 1, Wo, 1)
            v = a[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
            upd = ok & ((v >= best) if last else (v > best))
            best = torch.where(upd, v, best)
            bidx = torch.where(upd, (yy.clamp(0, H - 1).view(1, Ho, 1, 1) * W + xx.clamp(0, W - 1).view(1, 1, Wo, 1)).expand_as(bidx), bidx)
    assert int(bidx.min()) >= 0
    return bidx


def covered(H, W, pool):
    """[H, W] bool: pixels that lie in at least one pool window"""
    k, s, p, ceil = pool
    from bwd_pass_cases import pool_out
    cy, cx = torch.zeros(H, dtype=torch.bool), torch.zeros(W, dtype=torch.bool)
    for o in range(pool_out(H, k, s, p, ceil)):
        cy[max(o * s - p, 0):max(min(o * s - p + k, H), 0)] = True
    for o in range(pool_out(W, k, s, p, ceil)):
        cx[max(o * s - p, 0):max(min(o * s - p + k, W), 0)] = True
    return cy.view(H, 1) & cx.view(1, W)


def decide(z, pool, relu, last=False):
    """(ReLU mask or None, arg-max or None) of one evaluation of z"""
    mask = (z > 0) if relu else None
    idx = window_argmax(torch.relu(z) if relu else z, pool, last) if pool else None
    return mask, idx


def decisions(raw, sc32, sh32, pool, relu):
    """the decisions csrc/backward.hip takes on this map: z = fma(raw, scale, shift) in fp32"""
    return decide((raw.double() * sc32.double() + sh32.double()).float(), pool, relu)


def ambiguous(raw, gamma, beta, pool, relu):
    """[B, H, W, C] bool: raw values a decision of which differs between the three evaluations of z (all False: the inputs are clean)"""
    n = raw.numel() // raw.shape[-1]
    st = batch_stats(raw)
    sc64, sh64, _, _ = finalize_f64(st, n, gamma, beta)
    zs = z_forms(raw, sc64.float(), sh64.float(), sc64, sh64)
    bad = torch.zeros(raw.shape, dtype=torch.bool)
    d = [decide(z, pool, relu) for z in zs]
    if relu:
        bad |= (d[0][0] != d[1][0]) | (d[0][0] != d[2][0])
    if pool:
        w = (d[0][1] != d[1][1]) | (d[0][1] != d[2][1])          # [B, Ho, Wo, C]: windows whose arg-max differs -> the elements they chose
        if bool(w.any()):
            B, H, W, C = raw.shape
            hits = torch.zeros(B, H * W, C, dtype=torch.int32)
            for i in d:
                hits.scatter_add_(1, i[1].reshape(B, -1, C), w.reshape(B, -1, C).int())
            bad |= hits.view(B, H, W, C) > 0
    return bad


def make_inputs(rid, kw):
    """A row's operands (cached, read only): raw, dout, gamma, beta with every decision unambiguous; 'rounds' = redraw rounds it took."""
    if rid in _cache:
        return _cache[rid]
    g = torch.Generator().manual_seed(zlib.crc32(rid.encode()))
    from bwd_pass_cases import out_extent
    B, H, W, C = kw['B'], kw['H'], kw['W'], kw['C']
    Ho, Wo = out_extent(kw)
    q = (lambda t: t.to(torch.bfloat16).float()) if 'dout_bf16' in kw else (lambda t: t)      # mixed rows: bf16-representable raw
    raw = q(torch.randn(B, H, W, C, generator=g) * 1.5 + 0.3)
    if kw.get('ties'):          # exact duplicates inside the windows of image 0: 'first maximum wins' decides where d(out) goes
        raw[0, 1::2, 1::2] = raw[0, 0:-1:2, 0:-1:2]
    sign = 1.0 - 2.0 * ((torch.arange(C) + int(torch.randint(0, 2, (1,), generator=g))) % 2)          # both signs at every C
    gamma = (torch.rand(C, generator=g) * 1.3 + 0.2) * sign[torch.randperm(C, generator=g)]
    beta = torch.randn(C, generator=g) * 0.5
    dout = torch.randn(B, Ho, Wo, C, generator=g)
    if kw.get('dout_bf16'):
        dout = q(dout)
    rounds = 0
    for rounds in range(9):
        bad = ambiguous(raw, gamma, beta, kw['pool'], kw['relu'])
        n = int(bad.sum())
        if n == 0 or rounds == 8:
            break
        raw[bad] = q(torch.randn(n, generator=g) * 1.5 + 0.3)
    o = dict(raw=raw, dout=dout, gamma=gamma, beta=beta, rounds=rounds, ambiguous=n)
    _cache[rid] = o
    return o


def make_plain_inputs(rid, kw):
    """Operands of a scale = shift = NULL row: z IS the stored value, no rounding enters a decision.  relu without pool: a post-ReLU map
    (bwd_ops._convrelu masks on the stored output); pool only: distinct values; relu + pool: a signed map with exact zeros."""
    g = torch.Generator().manual_seed(zlib.crc32(rid.encode()))
    from bwd_pass_cases import out_extent
    B, H, W, C = kw['B'], kw['H'], kw['W'], kw['C']
    Ho, Wo = out_extent(kw)
    n = B * H * W * C
    if kw['pool'] and not kw['relu']:
        raw = ((torch.randperm(n, generator=g).float() - n // 2) / 64.0).view(B, H, W, C)
        assert raw.unique().numel() == n
    else:
        raw = torch.randn(B, H, W, C, generator=g)
        raw = torch.relu(raw) if not kw['pool'] else torch.where(torch.rand(raw.shape, generator=g) < 0.1, torch.zeros(()), raw)
    return dict(raw=raw, dout=torch.randn(B, Ho, Wo, C, generator=g))


# ---- the backward, written out ----------------------------------------------------------------------------------------------------------
def route(dout, mask, idx, shape, uncovered_value=0.0, pool=None):
    """dz [B, H, W, C]: d(out) sent to each window's arg-max (summed where windows overlap), zero elsewhere, then the ReLU mask"""
    B, H, W, C = shape
    if idx is None:
        d = dout.clone()
    else:
        d = torch.zeros(B, H * W, C, dtype=dout.dtype)
        d.scatter_add_(1, idx.reshape(B, -1, C), dout.reshape(B, -1, C))
        d = d.view(B, H, W, C)
        if uncovered_value != 0.0:
            d[:, ~covered(H, W, pool)] = uncovered_value
    return d * mask.to(d.dtype) if mask is not None else d


def bn_backward(raw, dout, gamma, mask, idx, dt, eps=EPS, uncovered_value=0.0, pool=None):
    """draw, dgamma, dbeta, s1, s2, dz of conv output -> BatchNorm(train) -> ReLU -> pool, all arithmetic in dtype dt"""
    raw, dout, g = raw.to(dt), dout.to(dt), gamma.to(dt)
    C = raw.shape[-1]
    n = raw.numel() // C
    mean = raw.reshape(-1, C).mean(0)
    var = ((raw - mean) ** 2).reshape(-1, C).mean(0)
    inv = 1.0 / torch.sqrt(var + eps)
    dz = route(dout, mask, idx, raw.shape, uncovered_value, pool)
    s1 = dz.reshape(-1, C).sum(0)
    s2 = (dz * raw).reshape(-1, C).sum(0)
    dg = inv * (s2 - mean * s1)
    A = g * inv
    Bc = -g * inv * inv * dg / n
    Cc = -g * inv * s1 / n + g * inv * inv * mean * dg / n
    return dict(draw=A * dz + Bc * raw + Cc, dgamma=dg, dbeta=s1, s1=s1, s2=s2, dz=dz, A=A, B=Bc, C=Cc)


def autograd_f64(raw, dout, gamma, beta, pool, relu, eps=EPS):
    """float64 autograd of max_pool2d(relu(batch_norm(x))) with its own decisions: (draw NHWC, dgamma, dbeta)"""
    import torch.nn.functional as F
    x = raw.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    gm, bt = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.batch_norm(x, None, None, gm, bt, True, 0.0, eps)
    if relu:
        y = torch.relu(y)
    if pool:
        y = F.max_pool2d(y, pool[0], pool[1], pool[2], ceil_mode=pool[3])
    y.backward(dout.double().permute(0, 3, 1, 2))
    return x.grad.permute(0, 2, 3, 1), gm.grad, bt.grad


def relerr(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def reference(rid, kw):
    """(inputs, decisions, float64 restatement, e_cpu32 per output) of a BatchNorm row, cached.  e_cpu32: the restatement in float32 on the
    CPU with the same decisions against float64 -- a quantity of the reference alone."""
    key = ('ref', rid)
    if key not in _cache:
        o = make_inputs(rid, kw)
        n = o['raw'].numel() // kw['C']
        sc, sh = finalize_f32(batch_stats(o['raw']), n, o['gamma'], o['beta'])
        mask, idx = decisions(o['raw'], sc, sh, kw['pool'], kw['relu'])
        r64 = bn_backward(o['raw'], o['dout'], o['gamma'], mask, idx, torch.float64)
        r32 = bn_backward(o['raw'], o['dout'], o['gamma'], mask, idx, torch.float32)
        e32 = {k: relerr(r32[k], r64[k]) for k in ('draw', 'dgamma', 'dbeta')}
        e32['sums'] = relerr(torch.cat([r32['s1'], r32['s2']]), torch.cat([r64['s1'], r64['s2']]))
        _cache[key] = (o, (mask, idx), r64, e32)
    return _cache[key]
