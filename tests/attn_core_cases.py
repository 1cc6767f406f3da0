"""The case table of the fixed-size fp32 attention core (flash_attn_kernel in csrc/flash_attn_core.h, launched by gssd_self_attn_core_kv_f32
in csrc/flash_attn.hip) and the float64 references its tests compare with.  Plain Python, no GPU: tests/test_attn_core_cases_cpu.py checks
the table itself, tests/test_gpu_attn_cores.py runs it, tests/test_gpu_self_attn_op.py shares core_case / core_buffers.

A width is (d_real, C2): theta / phi channels as the caller has them and g channels.  The dispatcher maps it to a template instance
<D, C2 per launch, BKV> (INSTANCES: what include/gssd_hip.h and the dispatcher state; instance_of restates the dispatcher's rule).  Each
instance has its own staging geometry -- rows per 1-KiB piece 64 / (D / 4) from 16 down to 1, XOR masks 3 / 7 / 15, key blocks of 32 or 64
-- so each can be wrong alone.

Token shapes (N, Nk): N brackets the 64-query tile, Nk brackets one and two key blocks for BKV = 32 and for BKV = 64, and
Nkp = roundup(Nk, 4) exceeds Nk in most rows.  Inputs as everywhere in this family: theta, keys ~ N(0, 1) D^-0.25 1.5 (logits of standard
deviation 2.25 at every width), values and d(attn_g) ~ N(0, 1), all fp32-representable float64 from a seeded generator."""
import functools

import torch

SENT = 777.0

# (d_real, C2) -> (D, C2 of one launch, BKV, launches)
INSTANCES = {
    (64, 256): (64, 256, 64, 1),
    (128, 512): (128, 512, 32, 1),
    (256, 1024): (256, 512, 32, 2),          # two launches of <256, 512, 32> with out_stride = g_batch_rows = 1024
    (32, 128): (32, 128, 64, 1),
    (16, 32): (16, 32, 64, 1), (12, 32): (16, 32, 64, 1), (8, 32): (16, 32, 64, 1), (4, 32): (16, 32, 64, 1),      # zero-filled to 16
    (16, 64): (16, 64, 64, 1), (8, 64): (16, 64, 64, 1),
}
WIDTHS = list(INSTANCES)
TOKENS = [(1, 1), (65, 31), (64, 32), (63, 33), (130, 64), (100, 65), (25, 131)]
BF16_TOKENS = [(65, 31), (100, 65)]
IN_PLACE_N = [1, 65, 131]


# gssd_sa_pool_kv_f32 / gssd_sa_unpool_f32 (csrc/sa_pool.hip): (H, P) -- (9, 4), (10, 3) and (19, 6) have overlapping cells -- and (C8, C2)
POOL = [(9, 4), (10, 3), (5, 1), (7, 7), (19, 6), (38, 19)]
POOL_OVERLAPPING = [(9, 4), (10, 3), (19, 6)]
POOL_WIDTHS = [(4, 32), (16, 64), (4, 64), (16, 32)]


def pool_cells(H, P):
    """F.adaptive_avg_pool2d's cells along one axis: cell o covers [floor(o H / P), ceil((o + 1) H / P))."""
    return [(o * H // P, -(-(o + 1) * H // P)) for o in range(P)]


def instance_of(d_real, C2):
    """The dispatcher's rule (gssd_self_attn_core_kv_f32), restated: None for a width it refuses."""
    if (d_real, C2) in ((64, 256), (32, 128)):
        return (d_real, C2, 64, 1)
    if (d_real, C2) == (128, 512):
        return (128, 512, 32, 1)
    if (d_real, C2) == (256, 1024):
        return (256, 512, 32, 2)
    if 0 < d_real <= 16 and d_real % 4 == 0 and C2 in (32, 64):
        return (16, C2, 64, 1)
    return None


def batch_of(d_real, C2):
    """B = 2; three images where a launch covers a slice of wider rows, so that a wrong g_batch_rows shows."""
    return 3 if INSTANCES[(d_real, C2)][3] > 1 else 2


def roundup(n, m):
    return (n + m - 1) // m * m


def case_id(d_real, C2, N, Nk):
    return f'd{d_real}-c{C2}-N{N}-Nk{Nk}'


TABLE = [(d, c2, n, nk) for d, c2 in WIDTHS for n, nk in TOKENS]
# rows whose default inputs would not notice a dropped last key or a shifted last key block: another seed (found on the CPU by
# tests/test_attn_core_cases_cpu.py; none needed so far)
SEEDS = {}


def attention(th, ks, v):
    """out = softmax(theta keys^T) values and the rows' log-sum-exp, in the dtype of the operands."""
    S = th @ ks.transpose(1, 2)
    lse = torch.logsumexp(S, dim=-1)
    return torch.exp(S - lse.unsqueeze(-1)) @ v, lse


@functools.lru_cache(maxsize=None)
def core_case(D, C2, N, Nk, B=2, seed=0):
    """float64 inputs (fp32-representable) and references of the attention core and its backward."""
    g = torch.Generator().manual_seed(D * 7919 + C2 * 31 + N * 3 + Nk + 1000003 * seed)
    f = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float().double()      # noqa: E731
    th, ks = f(B, N, D) * D ** -0.25 * 1.5, f(B, Nk, D) * D ** -0.25 * 1.5
    v, dag = f(B, Nk, C2), f(B, N, C2)
    S = th @ ks.transpose(1, 2)
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse.unsqueeze(-1))
    out = P @ v
    dvec = (dag * out).sum(-1)
    dP = dag @ v.transpose(1, 2)
    dS = P * (dP - dvec.unsqueeze(-1))
    return dict(th=th, ks=ks, v=v, dag=dag, lse=lse, out=out, dvec=dvec, dq=dS @ ks, dk=dS.transpose(1, 2) @ th, dv=P.transpose(1, 2) @ dag)


def table_case(d_real, C2, N, Nk):
    """The shared, unchanging reference of a table row (theta and keys are scaled by their real width)."""
    return core_case(d_real, C2, N, Nk, batch_of(d_real, C2), SEEDS.get((d_real, C2, N, Nk), 0))


def core_buffers(c, D, C2, N, Nk, device, B=2):
    """Device operands with strides wider than the widths: tp rows of 2 D (theta | noise), keys rows of D + 4, gT [B][C2][Nkp]."""
    Nkp = (Nk + 3) // 4 * 4
    krow = D + 4
    tp = torch.randn(B, N, 2 * D)
    tp[..., :D] = c['th'].float()
    keys = torch.randn(B, Nk, krow)
    keys[..., :D] = c['ks'].float()
    gT = torch.zeros(B, C2, Nkp)
    gT[..., :Nk] = c['v'].float().transpose(1, 2)
    return tp.to(device), keys.to(device), krow, gT.to(device), Nkp


def pooled_buffers(c, d_real, C2, N, Nk, B):
    """Host operands of the pooled-key form: tp [B][N][2 d_real] (theta, then finite filler), keys [B][Nk][d_real + 4] whose four slack
    floats are NaN (they lie beyond d_real: the kernel must never stage them), gT [B][C2][Nkp] with zero pad.  -> tp, keys, krow, gT, Nkp"""
    g = torch.Generator().manual_seed(d_real * 131 + C2 + N * 7 + Nk)
    Nkp = roundup(Nk, 4)
    krow = d_real + 4
    tp = torch.randn(B, N, 2 * d_real, generator=g)
    tp[..., :d_real] = c['th'].float()
    keys = torch.full((B, Nk, krow), float('nan'))
    keys[..., :d_real] = c['ks'].float()
    gT = torch.zeros(B, C2, Nkp)
    gT[..., :Nk] = c['v'].float().transpose(1, 2)
    return tp, keys, krow, gT, Nkp


def in_place_buffers(c, d_real, C2, N, B):
    """Host operands of the keys-in-place form (kp = tp + D, kstride = 2 D, Nk = N): tp [B][N][2 d_real] = theta | phi, gT [B][C2][Np]."""
    Np = roundup(N, 4)
    tp = torch.cat((c['th'], c['ks']), dim=-1).float().contiguous()
    gT = torch.zeros(B, C2, Np)
    gT[..., :N] = c['v'].float().transpose(1, 2)
    return tp, gT, Np


# ---- what a kernel's classic slips would compute: the table must tell them from the truth ----------------------------------------------------
def without_last_key(c):
    """The reference with the key mask one short (key Nk - 1 dropped)."""
    return attention(c['th'], c['ks'][:, :-1], c['v'][:, :-1])[0]


def last_block_rotated(c, BKV):
    """The reference with the rows of the last staged key tile rotated by one: the tile holds BKV rows, those beyond Nk zero-filled as the
    kernel stages them; row i takes what row i - 1 held and row 0 what the last row held (a zero row when the block is ragged).  The
    values keep their places, and the mask still ends at Nk."""
    ks = c['ks']
    B, Nk, D = ks.shape
    key0 = (Nk - 1) // BKV * BKV
    tile = torch.zeros(B, BKV, D, dtype=ks.dtype)
    tile[:, :Nk - key0] = ks[:, key0:]
    moved = ks.clone()
    moved[:, key0:] = torch.roll(tile, 1, dims=1)[:, :Nk - key0]
    return attention(c['th'], moved, c['v'])[0]
