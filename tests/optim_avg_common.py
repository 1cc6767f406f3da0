"""What tests/test_optim_avg_cpu.py and tests/test_gpu_optim_avg.py share: the synthetic module and the yardstick of ONE update of an
averaged model.

Yardstick (teacher-forced: expected values in float64 from the fp32 a, b and the integer count n as they were BEFORE the update).  With
w64 = 1 - decay (EMA) or 1 / (n + 1) (SWA), both in double, and r = lerp64(a, b, w64) in torch's two-branch form:

    |a' - r| <= 2^-23 |r| + 2^-21 w |b - a| + 1e-38

Sources: the subtraction b - a (2^-24 |b - a|), the product (2^-24), w itself (2^-24 for the rounded 1 - decay, at most 2^-22 for an
fp32 1 / (n + 1)), the final add (2^-24 |r|): at most 2^-24 |r| + 1.5 * 2^-22 w |b - a|, and some margin.  Where w >= 0.5 the product is
(b - a) (1 - w) and 1 - w carries the error of w; (1 - w) <= w there, so the same bound holds.
Bitwise instead: the first update (n == 0) gives b, w = 1 gives b, w = 0 leaves a, copied tensors equal their source.
"""
import numpy as np
import torch

SEED = 20261


def numels(ch):
    return [1, 3, 4, 5, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 7, 0]


def buffer_numels(ch):
    return [1, 5, ch + 1]


class AvgSet(torch.nn.Module):
    """Parameters of numels(ch) as slices of ONE flat tensor laid end to end (self.flat), float buffers of buffer_numels(ch) and one
    0-dim int64 buffer.  Values: randn * 10^U(-3, 1) from a fixed seed."""

    def __init__(self, device, ch, seed=SEED):
        super().__init__()
        rng = np.random.default_rng(seed)

        def draw(n):
            return torch.from_numpy((rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)).to(device)
        ns = numels(ch)
        self.flat = draw(sum(ns))
        self.ps = torch.nn.ParameterList()
        o = 0
        for n in ns:
            self.ps.append(torch.nn.Parameter(self.flat[o:o + n]))
            o += n
        for i, n in enumerate(buffer_numels(ch)):
            self.register_buffer(f'stat{i}', draw(n))
        self.register_buffer('ticks', torch.tensor(7, dtype=torch.int64, device=device))

    def forward(self, x):
        return x

    @torch.no_grad()
    def perturb(self):
        """Other values in the same storage: every source tensor changes, magnitudes stay spread over four decades."""
        self.flat.copy_(self.flat * 0.75 + self.flat.roll(1) * 0.5)
        for name, b in self.named_buffers():
            if b.dtype == torch.float32:
                b.mul_(-1.5).add_(1e-3)
        self.ticks.add_(3)


@torch.no_grad()
def repoint(module, first=1):
    """Move the parameters of an AvgSet (copy) onto slices of a second flat tensor laid end to end from element ``first``: with first = 1
    no averaged parameter has its source's alignment."""
    total = sum(p.numel() for p in module.ps)
    flat = torch.zeros(total + first, device=module.flat.device, dtype=torch.float32)
    o = first
    for p in module.ps:
        flat[o:o + p.numel()].copy_(p.data)
        p.data = flat[o:o + p.numel()]
        o += p.numel()
    module.flat = flat
    return module


def weight64(decay, n):
    """The weight of the source in double: 1 - decay, or 1 / (n + 1) for the SWA rule (decay None)."""
    return 1.0 / (n + 1) if decay is None else 1.0 - decay


def lerp64(a, b, w):
    return a + w * (b - a) if w < 0.5 else b - (b - a) * (1.0 - w)


def check_update(a0, b, a1, n, decay, tag=''):
    """``a1`` (after) against float64 from fp32 ``a0`` (before), ``b`` (source) and the count ``n`` before the update; returns the worst
    error / bound ratio (0 where the result must be, and is, bitwise)."""
    if a0.numel() == 0:
        assert a1.numel() == 0
        return 0.0
    if n == 0 or decay == 0.0:
        assert torch.equal(a1, b), f'{tag}: {"the first update" if n == 0 else "w = 1"} is a bitwise copy'
        return 0.0
    if decay == 1.0:
        assert torch.equal(a1, a0), f'{tag}: w = 0 leaves the averaged tensor as it is'
        return 0.0
    w = weight64(decay, n)
    a64, b64 = a0.double(), b.double()
    r = lerp64(a64, b64, w)
    tol = 2.0 ** -23 * r.abs() + 2.0 ** -21 * w * (b64 - a64).abs() + 1e-38
    err = (a1.double() - r).abs()
    ratio = float((err / tol).max())
    assert bool((err <= tol).all()), f'{tag} ({a0.numel()} elements): err/bound {ratio:.3g}'
    return ratio


def snapshot(module):
    """Clones of every parameter and buffer, in parameters() + buffers() order."""
    return [t.detach().clone() for t in list(module.parameters()) + list(module.buffers())]
