"""What tests/test_grad_accum_cpu.py and tests/test_gpu_grad_accum.py share: the rows, the float64 model of one accumulation cycle of
gssd.optim.GradAccumulator (csrc/optim_accum.hip), and the bound a result is held to, derived here rounding by rounding.

The rule, per element of one parameter, over the micro-batches j = 1 .. k in which the parameter HAS a gradient g_j (fp32), with
w32_j = fp32(w_j) the weight as the kernel uses it and W = sum over ALL micro-batches of the cycle of (double)w32_j:

    a_1 = fl(w32_1 g_1);   a_j = fl(fma(w32_j, g_j, a_(j-1)));   average: result = fl(a_k fl(1 / W))      sum: result = a_k

Model (float64, from the weights w_j as the caller gave them): r = sum_j w_j g_j / sum_j w_j (sum: the numerator alone).

Bound.  u = 2^-24 is the unit roundoff of fp32, t_j = w_j g_j, S = sum_j |t_j|.
  * w32_j = w_j (1 + d), |d| <= u, and d = 0 where w_j is an fp32 number (None = 1, counts below 2^24, an fp32 tensor): every term moves
    by at most u |t_j|, together dw u S with dw = 1 if any weight of the cycle is inexact, else 0.  W moves by at most dw u W likewise.
  * each of the k operations (the FIRST product, then k - 1 fused multiply-adds) rounds once, by at most u |a_j|, and |a_j| <= S (1 + k u):
    together k u S.  The products inside an fma are not rounded.
  * 1 / W is formed in fp64 (2^-53: nothing) and rounded to fp32 once: a relative u on the result.  The final product rounds once: u.
  So |result - r| <= (k + dw) u S / W + (2 + dw) u |r|, and with |r| <= S / W:

      average:  |result - r| <= (k + 2 + 2 dw) u S / W        sum:  |result - r| <= (k + dw) u S

  times (1 + 2^-10) for the second-order terms (k <= 8: (1 + u)^(k + 3) - 1 is below u (k + 3) (1 + 2^-20)), plus, for results in the
  subnormal range where a rounding is absolute, 2^-149 per operation: (k + 1) 2^-149 (1 + 1 / W).
It grows with k and is a small multiple of 2^-24 S / W, as the sum of k rounded terms must be.

Exact rows: integer-valued gradients of magnitude <= 32 and weights 1, 2, 1 (or one weight 1): every product, every partial sum and the
division by W = 4 (a power of two) are exact in fp32, so the result equals the model BIT FOR BIT.
"""
import numpy as np
import torch

SEED = 20262
U = 2.0 ** -24
K_MAX = 8


def numels(ch):
    """The appended tensors of the GPU set (the base set of tests/test_gpu_optim.py brings 1, 3, 4, 5, 63, 64, 65, ch - 1, ch, ch + 1,
    3 ch + 7 and 0 elements, laid end to end so that most gradients are only 4-byte aligned): two more chunk edges, and two small ones
    whose gradient is missing in the first / in the last micro-batch."""
    return [2 * ch + 3, 257 * ch + 1, 6, 9]


def cpu_numels(ch):
    """The CPU tests' stand-in (``ch`` small): every edge of the GPU set."""
    return [1, 3, 4, 5, ch - 1, ch, ch + 1, 2 * ch + 3, 0, 6, 9]


LATE, EARLY = -2, -1       # positions (from the end) of the two parameters with a missing gradient


def present(k, n_params):
    """present[j][i]: whether parameter i has a gradient in micro-batch j.  The second to last parameter misses the FIRST micro-batch
    (with k = 1 it never gets one), the last one misses the LAST micro-batch when k > 1."""
    rows = [[True] * n_params for _ in range(k)]
    rows[0][n_params + LATE] = False
    if k > 1:
        rows[k - 1][n_params + EARLY] = False
    return rows


# (k, kind of weight, weights as the caller gives them, average, exact).  Kinds: 'none' (weight=None), 'float' (a Python number),
# 'f64' / 'f32' (a 1-element device tensor).  Counts stand for MultiBoxLoss.num_pos; the float rows carry weights that fp32 cannot hold.
_COUNTS = [37.0, 5.0, 112.0, 1.0, 64.0, 23.0, 250.0, 9.0]
_FRACS = [0.3, 1.7, 0.011, 5.1, 2.9, 0.7, 1.1, 3.3]
_F32 = [float(np.float32(w)) for w in _FRACS]
ROWS = [
    (1, 'none', [1.0], True, False),
    (1, 'float', _FRACS[:1], True, False),
    (1, 'f64', _COUNTS[:1], False, False),
    (2, 'none', [1.0] * 2, True, False),
    (2, 'float', _FRACS[:2], False, False),
    (2, 'f64', _COUNTS[:2], True, False),
    (2, 'f32', _F32[:2], True, False),
    (3, 'none', [1.0] * 3, False, False),
    (3, 'float', _FRACS[:3], True, False),
    (3, 'f64', _FRACS[:3], True, False),             # a device double that fp32 cannot hold (N / world with global_normalizer)
    (3, 'f32', _F32[:3], False, False),
    (8, 'none', [1.0] * 8, True, False),
    (8, 'float', _FRACS, True, False),
    (8, 'f64', _COUNTS, True, False),
    (8, 'f32', _F32, True, False),
    (8, 'float', _COUNTS, False, False),
    (1, 'none', [1.0], True, True),
    (3, 'float', [1.0, 2.0, 1.0], True, True),
    (3, 'f64', [1.0, 2.0, 1.0], True, True),
    (3, 'f32', [1.0, 2.0, 1.0], True, True),
    (3, 'f64', [1.0, 2.0, 1.0], False, True),
]
ROW_IDS = [f'k{k}-{kind}-{"mean" if avg else "sum"}{"-exact" if exact else ""}-{i}' for i, (k, kind, _, avg, exact) in enumerate(ROWS)]


def host_grads(total, exact, seed=SEED):
    """K_MAX flat fp32 gradient vectors of ``total`` elements (numpy): randn * 10^U(-4, 1), or integers in [-32, 32] for the exact rows."""
    rng = np.random.default_rng(seed + int(exact))
    if exact:
        return [rng.integers(-32, 33, total).astype(np.float32) for _ in range(K_MAX)]
    return [(rng.standard_normal(total) * 10.0 ** rng.uniform(-4, 1, total)).astype(np.float32) for _ in range(K_MAX)]


def inexact(weights):
    return any(float(np.float32(w)) != float(w) for w in weights)


def weight_sum64(weights):
    """What the device keeps: the float64 sum, in order, of the weights rounded to fp32."""
    s = 0.0
    for w in weights:
        s += float(np.float32(w))
    return s


def model64(grads, weights, average):
    """(r, S / W or S, k) in float64 for one parameter: ``grads[j]`` is its fp32 gradient in micro-batch j or None, ``weights[j]`` the
    weight of micro-batch j as the caller gave it.  None when the parameter has no gradient in the whole cycle."""
    have = [(w, g.double()) for w, g in zip(weights, grads) if g is not None]
    if not have:
        return None
    r = sum(w * g for w, g in have)
    s = sum(abs(w) * g.abs() for w, g in have)
    if average:
        big_w = sum(float(w) for w in weights)
        r, s = r / big_w, s / big_w
    return r, s, len(have)


def bound(s, k, weights, average):
    """The bound derived above, per element: ``s`` is S / W (S for a sum) from model64, ``k`` the number of gradients that arrived."""
    dw = 1 if inexact(weights) else 0
    ops = (k + 2 + 2 * dw) if average else (k + dw)
    floor = (k + 1) * 2.0 ** -149 * ((1.0 + 1.0 / sum(float(w) for w in weights)) if average else 1.0)
    return ops * U * (1.0 + 2.0 ** -10) * s + floor


def check(result, grads, weights, average, exact, tag=''):
    """``result`` (fp32) of one parameter against model64 within bound(), or bit for bit in an exact row; returns error / bound (0 where
    the match is bitwise)."""
    m = model64(grads, weights, average)
    assert m is not None, f'{tag}: a parameter without any gradient has no result'
    r, s, k = m
    assert result.dtype == torch.float32 and result.shape == r.shape, f'{tag}: {result.dtype}, {tuple(result.shape)}'
    if result.numel() == 0:
        return 0.0
    if exact:
        assert torch.equal(result, r.float()) and torch.equal(r.float().double(), r), f'{tag}: an exact row must match bit for bit'
        return 0.0
    tol = bound(s, k, weights, average)
    err = (result.double() - r).abs()
    ratio = float((err / tol).max())
    assert bool((err <= tol).all()), f'{tag} ({result.numel()} elements, k = {k}): err/bound {ratio:.3g}'
    return ratio


def restate32(grads, weights, average):
    """The kernel's rule for one parameter in numpy fp32, operation by operation (the fma through float64: the product of two fp32
    numbers is exact there).  Returns an fp32 numpy array, or None when no gradient arrived."""
    acc = None
    for w, g in zip(weights, grads):
        if g is None:
            continue
        w32 = np.float32(w)
        g = np.asarray(g, np.float32)
        acc = (w32 * g).astype(np.float32) if acc is None else (np.float64(w32) * g.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    if acc is None or not average:
        return acc
    inv = np.float32(1.0 / weight_sum64(weights))
    return (acc * inv).astype(np.float32)
