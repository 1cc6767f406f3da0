"""The case tables of the three attention backwards and the float64 references their tests compare with.  Plain Python, no GPU:
tests/test_attn_bwd_cases_cpu.py checks the tables and derives the gates, tests/test_gpu_attn_bwd.py runs them.

  gssd_self_attn_flash_bwd_bf16 (csrc/sa_flash_bwd.hip): one template, twelve instances -- three widths (D, C2), own keys / own queries
      (both run in every call), logits as a three-term bf16 split ("x3") or on the fp32 matrix cores ("f32mfma").  The workgroup owns 64
      tokens and streams the other side in blocks of 32: FLASH_BF16_N brackets both, keys in place (Nk = N).
  gssd_self_attn_flash_bwd_f32 (csrc/sa_flash_bwd_f32.hip): the (16, 64) instance, 64 own tokens, streamed blocks of 64 split over four
      waves whose partial sums meet in LDS: FLASH_F32_TOKENS.
  the explicit chain of gssd/bwd_ops.py::_sa_explicit (csrc/sa_backward.hip) over [N][Nkp] maps with uninitialised pad columns:
      CHAIN_WIDTHS x CHAIN_TOKENS, and gssd_softmax_bwd_rows_f32 alone: SOFTMAX_BWD.

Inputs are attn_core_cases.core_case's (seeded, fp32-representable float64; logits of standard deviation 2.25 at every width).

The bf16 kernel against two float64 computations on the operands the plan hands it (fp32 theta | phi, bf16 g and d(attn_g), fp32 lse and
D_i = <d(attn_g)_i, attn_g_i>): exact() rounds nothing more; model() makes the kernel's stated roundings -- the logits' bf16 split when x3,
P and dS to bf16 after dS = P o (dP - D), bf16 theta / phi in the two dS contractions -- and nothing else.  token_err(model, exact) is
what those roundings cost; the kernel is held to twice that (tests/test_attn_bwd_cases_cpu.py says why)."""
import functools

import torch

from attn_core_cases import SENT, TOKENS, core_case, roundup           # noqa: F401  (SENT, roundup: shared with the GPU module)

FLASH_BF16_WIDTHS = [(32, 128), (64, 256), (128, 512)]
FLASH_BF16_N = [1, 31, 32, 33, 63, 64, 65, 97, 131]
FLASH_BF16_FORMS = [('x3', True), ('f32mfma', False)]
FLASH_BF16_ROWS = [(d, c2, n, form) for d, c2 in FLASH_BF16_WIDTHS for n in FLASH_BF16_N for form, _ in FLASH_BF16_FORMS]
OWN, STREAMED = 64, 32                        # csrc/sa_flash_bwd.hip: tokens a workgroup owns, tokens per streamed block
B = 2

FLASH_F32_WIDTH = (16, 64)
F32_TILE, F32_WAVES = 64, 4                   # csrc/sa_flash_bwd_f32.hip: own tokens = tokens per streamed block, waves that split a block's rows
FLASH_F32_TOKENS = TOKENS + [(3, 2), (129, 129), (2, 257)]
FLASH_F32_ROWS = [(n, nk, form) for n, nk in FLASH_F32_TOKENS for form in ('pooled', 'inplace') if form == 'pooled' or n == nk]

CHAIN_WIDTHS = [(4, 32), (64, 256)]
CHAIN_TOKENS = [(1, 1), (65, 31), (63, 33), (100, 65), (25, 131)]
CHAIN_ROWS = [(d, c2, n, nk) for d, c2 in CHAIN_WIDTHS for n, nk in CHAIN_TOKENS]

SOFTMAX_BWD = [(1, 1, 4), (5, 63, 64), (4, 64, 64), (3, 65, 68), (9, 129, 132), (70000, 5, 8)]          # (rows, n, row stride)
SOFTMAX_BWD_GRID_WAVES = 16384 * 4            # gssd_softmax_bwd_rows_f32: at most 16384 workgroups of four waves, one row per wave and turn

GRADS = ('dtheta', 'dphi', 'dg')
SLIPS = {'drop_last_streamed_query': ('dphi', 'dg'), 'drop_last_streamed_key': ('dtheta',)}        # slip -> the gradients it moves
KV_SLIPS = {'drop_last_streamed_query': ('dk', 'dv'), 'drop_last_streamed_key': ('dq',)}

# rows whose default inputs fail the CPU conditions of tests/test_attn_bwd_cases_cpu.py (a slip that moves a gradient by less than the
# factor asked there): another seed, by case id.  None needed so far.
SEEDS = {}


def bf16_id(D, C2, N, form=None):
    """form = None: the key of SEEDS (both logit forms run on the same operands)."""
    return f'flash_bwd_bf16-d{D}-c{C2}-N{N}' + (f'-{form}' if form else '')


def f32_id(N, Nk, form):
    return f'flash_bwd_f32-d16-c64-N{N}-Nk{Nk}-{form}'


def chain_id(D, C2, N, Nk):
    return f'explicit-d{D}-c{C2}-N{N}-Nk{Nk}'


def softmax_id(rows, n, stride):
    return f'softmax_bwd_rows-r{rows}-n{n}-s{stride}'


def bf16r(x):
    """Round to bf16, nearest even, through fp32 as the kernels do; back in float64."""
    return x.float().to(torch.bfloat16).double()


def f32r(x):
    return x.float().double()


def token_err(got, ref):
    """The largest per-token L2 error over (b, i), over the RMS of the reference's per-token L2 norms: one bad token cannot hide in a
    tensor-wide norm."""
    got, ref = got.double(), ref.double()
    scale = float(ref.norm(dim=-1).pow(2).mean().sqrt())
    return float((got - ref).norm(dim=-1).max()) / max(scale, 1e-300)


# ---- gssd_self_attn_flash_bwd_bf16 -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flash_bf16_case(D, C2, N):
    """The operands as the plan hands them, in float64: th, ph (fp32), g, dag (bf16), lse, dvec (fp32; D_i of the true forward over
    these operands)."""
    c = core_case(D, C2, N, N, B, SEEDS.get(bf16_id(D, C2, N), 0))
    th, ph, g, dag = c['th'], c['ks'], bf16r(c['v']), bf16r(c['dag'])
    P = torch.exp(th @ ph.transpose(1, 2) - c['lse'].unsqueeze(-1))
    dvec = (dag * (P @ g)).sum(-1)
    return dict(th=th, ph=ph, g=g, dag=dag, lse=f32r(c['lse']), dvec=f32r(dvec), D=D, C2=C2, N=N)


def _contract(c, P, dS, ph, th, slip):
    """d theta = dS ph, d phi = dS^T th, d g = P^T dag -- or what a launch whose streamed mask is one short would add up."""
    dag = c['dag']
    if slip == 'drop_last_streamed_key':                  # the own-queries launch streams the keys
        dth = dS[:, :, :-1] @ ph[:, :-1]
    else:
        dth = dS @ ph
    if slip == 'drop_last_streamed_query':                # the own-keys launch streams the queries
        dph, dg = dS[:, :-1].transpose(1, 2) @ th[:, :-1], P[:, :-1].transpose(1, 2) @ dag[:, :-1]
    else:
        dph, dg = dS.transpose(1, 2) @ th, P.transpose(1, 2) @ dag
    return dict(dtheta=dth, dphi=dph, dg=dg)


def exact(c, slip=None):
    """The float64 backward on the operands the kernel is handed."""
    assert slip is None or slip in SLIPS
    th, ph = c['th'], c['ph']
    P = torch.exp(th @ ph.transpose(1, 2) - c['lse'].unsqueeze(-1))
    dS = P * (c['dag'] @ c['g'].transpose(1, 2) - c['dvec'].unsqueeze(-1))
    return _contract(c, P, dS, ph, th, slip)


def model(c, x3, slip=None):
    """The same backward with the kernel's stated roundings and nothing else; everything else is float64."""
    assert slip is None or slip in SLIPS
    th, ph = c['th'], c['ph']
    th_hi, ph_hi = bf16r(th), bf16r(ph)
    if x3:
        th_lo, ph_lo = bf16r(th - th_hi), bf16r(ph - ph_hi)
        S = th_hi @ ph_hi.transpose(1, 2) + th_hi @ ph_lo.transpose(1, 2) + th_lo @ ph_hi.transpose(1, 2)
    else:
        S = th @ ph.transpose(1, 2)
    P = torch.exp(S - c['lse'].unsqueeze(-1))
    dS = P * (c['dag'] @ c['g'].transpose(1, 2) - c['dvec'].unsqueeze(-1))
    return _contract(c, bf16r(P), bf16r(dS), ph_hi, th_hi, slip)


@functools.lru_cache(maxsize=None)
def e_model(D, C2, N, x3):
    """{gradient: token_err(model, exact)}: what the stated roundings cost at this row (the GPU gate is twice this)."""
    c = flash_bf16_case(D, C2, N)
    ex, mo = exact(c), model(c, x3)
    return {k: token_err(mo[k], ex[k]) for k in GRADS}


def single_token_bound(c):
    """N = 1: P = 1 and dS = 0, d theta = d phi = 0 exactly.  What a kernel may leave: dS = P (dP - D) with dP an fp32 accumulation of C2
    terms and D its fp32-rounded exact value, |dP - D| <= C2 2^-24 sum_c |dag_c g_c|, times one operand; the factor 2 covers P = 1 +- 1e-3,
    the bf16 roundings (2^-9) and the second-order terms.  -> per image (bound on |d theta|, bound on |d phi|)."""
    assert c['N'] == 1
    s = 2 * c['C2'] * 2.0 ** -24 * (c['dag'] * c['g']).abs().sum(-1)[:, 0]
    return s * c['ph'].abs().amax(dim=(1, 2)), s * c['th'].abs().amax(dim=(1, 2))


# ---- the key / value form in float64: gssd_self_attn_flash_bwd_f32 and the explicit chain ---------------------------------------------------------
def kv_case(D, C2, N, Nk, what):
    """core_case at the row's seed (what: the row's case id)."""
    return core_case(D, C2, N, Nk, B, SEEDS.get(what, 0))


def kv_backward(c, slip=None):
    """dq, dk, dv of core_case, or what a kernel that drops the last streamed query (the sums over i of dk, dv) or the last streamed key
    (the sum over j of dq) would return."""
    assert slip is None or slip in KV_SLIPS
    th, ks, v, dag = c['th'], c['ks'], c['v'], c['dag']
    P = torch.exp(th @ ks.transpose(1, 2) - c['lse'].unsqueeze(-1))
    dS = P * (dag @ v.transpose(1, 2) - c['dvec'].unsqueeze(-1))
    dq = dS[:, :, :-1] @ ks[:, :-1] if slip == 'drop_last_streamed_key' else dS @ ks
    if slip == 'drop_last_streamed_query':
        return dict(dq=dq, dk=dS[:, :-1].transpose(1, 2) @ th[:, :-1], dv=P[:, :-1].transpose(1, 2) @ dag[:, :-1])
    return dict(dq=dq, dk=dS.transpose(1, 2) @ th, dv=P.transpose(1, 2) @ dag)


# ---- gssd_softmax_bwd_rows_f32 -----------------------------------------------------------------------------------------------------------------
def softmax_bwd_case(rows, n, stride):
    """attn [rows + 2][stride] fp32 (softmax rows; pad columns NaN: never read), dattn the same shape (pad columns and the two rows beyond
    hold SENT) and the float64 reference [rows][n]."""
    g = torch.Generator().manual_seed(rows * 131 + n * 7 + stride)
    attn = torch.full((rows + 2, stride), float('nan'))
    attn[:, :n] = torch.softmax(2.25 * torch.randn(rows + 2, n, generator=g, dtype=torch.float64), -1).float()
    dattn = torch.full((rows + 2, stride), SENT)
    dattn[:rows, :n] = torch.randn(rows, n, generator=g)
    a, d = attn[:rows, :n].double(), dattn[:rows, :n].double()
    return attn, dattn, a * (d - (a * d).sum(-1, keepdim=True))
