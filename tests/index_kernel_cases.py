"""Edge registry of the index kernels: csrc/detect.hip (gssd_detect), csrc/loss.hip (gssd_multibox_loss_forward_f32, the four-launch
path, gssd_loss_backward) and csrc/evaluator.hip (gssd_eval_match, gssd_eval_ap).  Plain numpy, seeded, no torch, no GPU.

Four families -- DETECT, NMS (the ``loc_is_boxes`` entry of Detect), LOSS, EVAL -- of ``Row(name, params, build, pre, fixture)``:

    build()          -> dict of inputs (numpy arrays), the same every time
    pre(inp, res)    -> True when the ORACLE's result ``res`` for the row proves that the row reaches the branch it is named for
    fixture          -> the row's scores are pairwise distinct, so tests/golden/index_edges.npz holds what the reference computes for it
                        (tests/golden/make_golden_index_edges.py).  Ties are not the reference's to define: torch's sort and
                        np.argsort(-confidence) give no order among equals; the project's contract is the oracle's (lower index first).

tests/test_index_kernel_cases_cpu.py runs the oracle over every row (against the fixture, the preconditions, the sensitivity of the rows
to the classic mistakes: ``*_plain`` below restate each family with a switch per mistake); tests/test_gpu_index_kernels.py runs the
kernels over the same rows.  The thresholds the sizes are chosen around: 64 (wave), 256 (detect.hip DT / MAXK), 1024 (loss.hip LT, the
chunks of eval_ap), 4 (register-held logits of hnm_fused_kernel), 64 (lanes per image in eval_match)."""
from collections import namedtuple

import numpy as np

from oracle import eval_oracle as EO
from oracle import gssd_oracle as O

f32 = np.float32
Row = namedtuple('Row', 'name params build pre fixture')
PRIORS = {}


def priors(P):
    """The first P rows of the SSD300 prior boxes (computed once)."""
    if 'all' not in PRIORS:
        PRIORS['all'] = O.prior_box().astype(np.float32)
    return PRIORS['all'][:P]


def rand_boxes(rng, n, C):
    c = rng.uniform(0.2, 0.8, size=(n, 2))
    wh = rng.uniform(0.05, 0.4, size=(n, 2))
    lab = rng.integers(0, C - 1, size=(n, 1)).astype(np.float64)
    return np.concatenate([c - wh / 2, c + wh / 2, lab], 1).astype(np.float32)


def prior_box_as_target(pri, k, label=0.):
    """Prior k in corner form, rounded as the kernel rounds it: its IoU with prior k is exactly 1."""
    cx, cy, w, h = (np.float32(v) for v in pri[k])
    hx, hy = w / np.float32(2), h / np.float32(2)
    return np.array([[cx - hx, cy - hy, cx + hx, cy + hy, label]], np.float32)


FAR = np.array([[5., 5., 6., 6., 0.]], np.float32)        # overlaps no prior (they lie in [0, 1]): every IoU is 0, the best prior is 0


def seed_of(name):
    return int(np.frombuffer(name.encode(), np.uint8).astype(np.int64).dot(np.arange(1, len(name) + 1)) % 100003) + 17


def bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


# ==========================================================================================================================================
# Detect
# ==========================================================================================================================================
CONF_THRESH, NMS_THRESH = 0.01, 0.45
DET_DEFAULTS = dict(top_k=200, conf_thresh=CONF_THRESH, nms_thresh=NMS_THRESH)


def det_scores(inp):
    """The class scores Detect thresholds: the row's own, or the oracle's softmax of its logits."""
    return inp['scores'] if 'scores' in inp else O.softmax_scores(inp['logits'])


def det_oracle(inp, prm):
    """-> dict(out, keeps, cand[B, C], scores): O.detect on the row."""
    sc = det_scores(inp)
    B, P, C = sc.shape
    with np.errstate(all='ignore'):
        out, keeps = O.detect(C, 0, prm['top_k'], prm['conf_thresh'], prm['nms_thresh'], inp['loc'], sc, priors(P), return_keep=True)
    cand = (sc > f32(prm['conf_thresh'])).sum(1)
    cand[:, 0] = 0
    return dict(out=out, keeps=keeps, cand=cand, scores=sc)


def keep_arrays(keeps, B, C, top_k):
    """The oracle's keeps as the kernel lays them out: keep[B, C, top_k] (-1 past the count), cnt[B, C]."""
    keep = np.full((B, C, top_k), -1, np.int32)
    cnt = np.zeros((B, C), np.int32)
    for (b, cl), k in keeps.items():
        keep[b, cl, :k.shape[0]] = k
        cnt[b, cl] = k.shape[0]
    return keep, cnt


def det_distinct(inp, prm):
    """Candidate scores pairwise distinct per (image, class): the condition for a reference fixture."""
    sc = det_scores(inp)
    for b in range(sc.shape[0]):
        for cl in range(1, sc.shape[2]):
            s = sc[b, :, cl]
            s = s[s > f32(prm['conf_thresh'])]
            if np.unique(s).size != s.size:
                return False
    return True


def _loc(rng, B, P):
    return rng.normal(0, 0.5, size=(B, P, 4)).astype(np.float32)


def _det_P_edges(P, C):
    name = f'P_edges-P{P}-C{C}'

    def build():
        rng = np.random.default_rng(seed_of(name))
        return dict(loc=_loc(rng, 2, P), logits=rng.normal(0, 1.5, size=(2, P, C)).astype(np.float32))

    def pre(inp, res):
        return res['out'].shape == (2, C, 200, 5) and (res['cand'][:, 1:] <= P).all() and res['cand'][:, 1:].sum() > 0
    return Row(name, dict(DET_DEFAULTS), build, pre, True)


def scattered_scores(rng, P, n_cand, lo=0.02, hi=1.0):
    """P scores: n_cand distinct ones above the threshold at random priors, the rest below it (and not zero)."""
    s = rng.uniform(0.001, 0.009, size=P)
    where = rng.permutation(P)[:n_cand]
    s[where] = lo + (hi - lo) * (rng.permutation(n_cand) + rng.uniform(0.1, 0.9, n_cand)) / max(n_cand, 1)
    return s.astype(np.float32)


def _det_topk_edges(top_k, counts):
    name = f'topk_edges-k{top_k}-n{counts[0]}_{counts[1]}'

    def build():
        rng = np.random.default_rng(seed_of(name))
        sc = np.zeros((2, 600, 2), np.float32)
        for b, n in enumerate(counts):
            sc[b, :, 1] = scattered_scores(rng, 600, n)
            sc[b, :, 0] = 1 - sc[b, :, 1]
        return dict(loc=_loc(rng, 2, 600), scores=sc)

    def pre(inp, res):
        return tuple(res['cand'][:, 1]) == tuple(counts)            # "candidates == top_k - 1 / top_k / top_k + 1 / 600"
    return Row(name, dict(DET_DEFAULTS, top_k=top_k), build, pre, True)


def _det_thresh_strict():
    name = 'thresh_strict'
    t = f32(CONF_THRESH)

    def build():
        rng = np.random.default_rng(seed_of(name))
        sc = np.zeros((2, 300, 2), np.float32)
        for b in range(2):
            s = scattered_scores(rng, 300, 40)
            at = rng.permutation(300)[:7]
            s[at[:6]] = t                                              # exactly conf_thresh: excluded (strict >)
            s[at[6]] = np.nextafter(t, f32(1))                         # the next float above: a candidate
            sc[b, :, 1], sc[b, :, 0] = s, 1 - s
        return dict(loc=_loc(rng, 2, 300), scores=sc)

    def pre(inp, res):
        s = inp['scores'][:, :, 1]
        return ((s == t).sum(1) >= 5).all() and ((s == np.nextafter(t, f32(1))).sum(1) == 1).all() \
            and np.array_equal(res['cand'][:, 1], (s > t).sum(1)) and np.array_equal(res['cand'][:, 1], (s >= t).sum(1) - (s == t).sum(1))
    return Row(name, dict(DET_DEFAULTS), build, pre, True)


def _det_one_class_empty():
    name = 'one_class_empty'

    def build():
        rng = np.random.default_rng(seed_of(name))
        lg = rng.normal(0, 1.5, size=(3, 257, 3)).astype(np.float32)
        lg[0, :, 1] = -20 + rng.normal(0, 0.1, 257)                    # image 0: class 1 has no candidate
        lg[1, :, 2] = -20 + rng.normal(0, 0.1, 257)                    # image 1: class 2 has none
        lg[2, :, 1:] = -20 + rng.normal(0, 0.1, (257, 2))              # image 2: empty altogether
        return dict(loc=_loc(rng, 3, 257), logits=lg.astype(np.float32))

    def pre(inp, res):
        c = res['cand']
        return c[0, 1] == 0 and c[0, 2] > 0 and c[1, 1] > 0 and c[1, 2] == 0 and c[2, 1] == 0 and c[2, 2] == 0
    return Row(name, dict(DET_DEFAULTS), build, pre, True)


def _det_radix_bytes(j):
    """Scores 0x3F000000 + k * 2^(8j): the candidates differ in byte j only, so radix pass j (of the four, from the top byte down) is the
    one that finds the cut.  k is a permutation, so the scores are distinct; j = 3 leaves 63 values below inf."""
    name = f'radix_bytes-j{j}'
    P, top_k = (256, 100) if j < 3 else (60, 20)

    def build():
        rng = np.random.default_rng(seed_of(name))
        sc = np.zeros((2, P, 2), np.float32)
        for b in range(2):
            sc[b, :, 1] = bits(0x3F000000 + (rng.permutation(P).astype(np.uint32) << np.uint32(8 * j)))
        return dict(loc=_loc(rng, 2, P), scores=sc)

    def pre(inp, res):
        u = inp['scores'][:, :, 1].view(np.uint32)
        others = np.uint32(0xFFFFFFFF) ^ (np.uint32(0xFF) << np.uint32(8 * j))
        return (((u ^ u[:, :1]) & others) == 0).all() and (res['cand'][:, 1] == P).all() and P > top_k   # "radix byte j decides this row"
    return Row(name, dict(DET_DEFAULTS, top_k=top_k), build, pre, True)


def _levels_to_inputs(level, use_logits, rng, B=2):
    """``level[P]``: 2 = one of the distinct scores above the tie value, 1 = the tie value, 0 = below the threshold.  As scores
    (tie = 0.5) or as two-class logits (class 0 logit 0: equal logits give equal softmax scores)."""
    P = level.shape[0]
    n_hi = int((level == 2).sum())
    if use_logits:
        v = np.where(level == 1, 0.0, -9.0)
        v[level == 2] = 1.0 + 0.01 * rng.permutation(n_hi)
        lg = np.zeros((B, P, 2), np.float32)
        lg[:, :, 1] = v
        return dict(loc=_loc(rng, B, P), logits=lg)
    v = np.where(level == 1, 0.5, 0.001)
    v[level == 2] = 0.6 + 0.3 * rng.permutation(n_hi) / max(n_hi, 1)
    sc = np.zeros((B, P, 2), np.float32)
    sc[:, :, 1] = v
    sc[:, :, 0] = 1 - sc[:, :, 1]
    return dict(loc=_loc(rng, B, P), scores=sc)


def _det_ties_all(use_logits):
    name = 'ties_all' + ('-logits' if use_logits else '')
    nms_t = 0.45 if use_logits else 1.0      # at 1.0 nothing is suppressed: the kept list IS the cut

    def build():
        return _levels_to_inputs(np.ones(600, np.int64), use_logits, np.random.default_rng(seed_of(name)))

    def pre(inp, res):
        ok = (res['cand'][:, 1] == 600).all() and np.unique(res['scores'][:, :, 1]).size == 1
        for b in range(2):
            k = res['keeps'][(b, 1)]
            ok = ok and k.size > 0 and (np.diff(k) > 0).all() and k.max() < 200           # survivors: priors 0..199 in index order
            if nms_t == 1.0:
                ok = ok and np.array_equal(k, np.arange(200))
        return ok
    return Row(name, dict(DET_DEFAULTS, nms_thresh=nms_t), build, pre, False)


def tie_group(s, top_k):
    """-> (indices of the priors that tie with the top_k-th candidate score, how many of them the cut takes)."""
    cand = np.sort(s[s > f32(CONF_THRESH)])[::-1]
    kth = cand[min(top_k, cand.size) - 1]
    return np.nonzero(s == kth)[0], min(top_k, cand.size) - int((s > kth).sum())


def _det_ties_straddle(use_logits):
    name = 'ties_straddle' + ('-logits' if use_logits else '')

    def build():
        rng = np.random.default_rng(seed_of(name))
        level = np.zeros(600, np.int64)
        level[70:401:3] = 1                                            # 111 ties: prior 70 (chunk 0, wave 1) .. 400 (chunk 1, wave 2)
        free = np.nonzero(level == 0)[0]
        level[rng.permutation(free)[:120]] = 2                         # 120 greater scores anywhere: the cut takes 80 of the ties
        return _levels_to_inputs(level, use_logits, rng)

    def pre(inp, res):
        ok = True
        for b in range(2):
            idx, need = tie_group(res['scores'][b, :, 1], 200)
            in0 = int((idx < 256).sum())
            ok = ok and 64 <= idx[0] < 128 and 256 + 128 <= idx[-1] < 256 + 192          # wave 1 of chunk 0 .. wave 2 of chunk 1
            ok = ok and in0 < need < idx.size and 256 <= idx[need - 1] < 512             # the cut is inside the group, in chunk 1
        return bool(ok)
    return Row(name, dict(DET_DEFAULTS), build, pre, False)


def _det_decode_overflow():
    name = 'decode_overflow'

    def build():
        rng = np.random.default_rng(seed_of(name))
        lg = rng.normal(0, 1.5, size=(2, 65, 2)).astype(np.float32)
        loc = _loc(rng, 2, 65)
        order = np.argsort(-O.softmax_scores(lg)[:, :, 1], axis=1)
        loc[0, order[0, 0], 2] = 500.       # exp(100) overflows fp32: w = inf, x1 = -inf, x2 = nan.  The top score: it is kept, and
        loc[0, order[0, 7], 0] = np.nan     # every IoU against it is NaN, which is not <= the threshold: nothing else survives
        loc[1, order[1, 5], 2] = 500.       # further down: their own IoU against the kept top box is NaN, so they are dropped
        loc[1, order[1, 9], 0] = np.nan
        return dict(loc=loc, logits=lg)

    def pre(inp, res):
        o = res['out'][:, 1]
        order = np.argsort(-res['scores'][1, :, 1])
        k1 = res['keeps'][(1, 1)]
        return bool(np.isnan(o[0, 0]).any() and np.isinf(o[0, 0]).any() and res['keeps'][(0, 1)].size == 1 and res['cand'][0, 1] > 10
                    and np.isfinite(o[1]).all() and k1.size > 3 and order[5] not in k1 and order[9] not in k1)
    return Row(name, dict(DET_DEFAULTS), build, pre, False)


DETECT = [_det_P_edges(P, C) for P in (1, 63, 64, 65, 255, 256, 257, 600) for C in (2, 3, 5)]
DETECT += [_det_topk_edges(k, c) for k in (1, 5, 64, 256) for c in ((k - 1, k), (k + 1, 600))]
DETECT += [_det_thresh_strict(), _det_one_class_empty()]
DETECT += [_det_radix_bytes(j) for j in range(4)]
DETECT += [_det_ties_all(False), _det_ties_all(True), _det_ties_straddle(False), _det_ties_straddle(True), _det_decode_overflow()]
DIRTY_BUFFER_ROWS = ('P_edges-P65-C3', 'one_class_empty')


# ---- the loc_is_boxes entry: ops.detect_boxes / layers.box_utils.nms ------------------------------------------------------------------
def nms_oracle(inp, prm):
    return dict(keep=O.nms(inp['boxes'], inp['scores'], prm['overlap'], prm['top_k']))


def _nms_row(name, boxes, scores, overlap, top_k, want=None, fixture=True):
    boxes, scores = np.asarray(boxes, np.float32).reshape(-1, 4), np.asarray(scores, np.float32)

    def pre(inp, res):
        return want is None or list(res['keep']) == list(want)
    return Row('nms_exact-' + name, dict(overlap=float(overlap), top_k=top_k), lambda: dict(boxes=boxes, scores=scores), pre, fixture)


def _nms_random(n, top_k):
    rng = np.random.default_rng(seed_of(f'nms{n}'))
    c = rng.uniform(0.2, 0.8, size=(n, 2))
    wh = rng.uniform(0.05, 0.3, size=(n, 2))
    sc = (0.02 + 0.97 * (rng.permutation(n) + 0.5) / n).astype(np.float32)
    return _nms_row(f'n{n}-k{top_k}', np.concatenate([c - wh / 2, c + wh / 2], 1), sc, 0.45, top_k)


HALF_BELOW = float(np.nextafter(np.float32(0.5), np.float32(0)))
PAIR = [[0, 0, 1, 1], [0, 0, 1, 2]]                                   # IoU = 1 / 2 exactly
CHAIN = [[0, 0, 10, 10], [3, 0, 13, 10], [6, 0, 16, 10]]              # a-b and b-c: 7/13; a-c: 4/16
NMS = [_nms_row('pair-at', PAIR, [.9, .8], 0.5, 200, want=[0, 1]),    # IoU == overlap is kept (<=)
       _nms_row('pair-below', PAIR, [.9, .8], HALF_BELOW, 200, want=[0]),
       _nms_row('identical', [[.1, .2, .5, .6]] * 3, [.7, .9, .8], 0.45, 200, want=[1]),
       _nms_row('chain', CHAIN, [.9, .8, .7], 0.5, 200, want=[0, 2]),  # a suppresses b; b, suppressed, does not suppress c
       _nms_row('n1', [[.1, .1, .3, .3]], [.5], 0.45, 1, want=[0]),    # (top_k < n cannot hold at n = 1: top_k > 0)
       _nms_random(257, 200), _nms_random(257, 256), _nms_random(257, 7)]


def pairwise_nms_iou(boxes):
    """iou[i, j] of candidate j against the picked box i, in box_utils.nms's association: inter / ((area_j - inter) + area_i)."""
    x1, y1, x2, y2 = (boxes[:, k] for k in range(4))
    area = (x2 - x1) * (y2 - y1)
    w = np.maximum(np.minimum(x2[None], x2[:, None]) - np.maximum(x1[None], x1[:, None]), f32(0))
    h = np.maximum(np.minimum(y2[None], y2[:, None]) - np.maximum(y1[None], y1[:, None]), f32(0))
    inter = w * h
    with np.errstate(all='ignore'):
        return inter / ((area[None] - inter) + area[:, None])


def nms_plain(boxes, scores, overlap, top_k, tie_high=False, iou_lt=False, topk_after=False, dead_suppress=False):
    """Greedy NMS as nested loops, with a switch per classic mistake (all off: the contract)."""
    boxes, scores = boxes.astype(f32), scores.astype(f32)
    order = sorted(range(scores.shape[0]), key=lambda i: (-float(scores[i]), -i if tie_high else i))
    if not topk_after:
        order = order[:top_k]
    iou = pairwise_nms_iou(boxes[order]) if order else None
    t = f32(overlap)
    alive, keep = [True] * len(order), []
    for a in range(len(order)):
        if alive[a]:
            keep.append(order[a])
        elif not dead_suppress:
            continue
        for b in range(a + 1, len(order)):
            ok = iou[a, b] < t if iou_lt else iou[a, b] <= t
            if not ok:
                alive[b] = False
    return np.asarray(keep[:top_k] if topk_after else keep, np.int64)


def detect_plain(inp, prm, thresh_ge=False, **nms_switches):
    """Detect as loops over (image, class) around nms_plain -> (out, keeps) like O.detect(return_keep=True)."""
    sc = det_scores(inp)
    B, P, C = sc.shape
    top_k, t = prm['top_k'], f32(prm['conf_thresh'])
    out, keeps = np.zeros((B, C, top_k, 5), f32), {}
    for b in range(B):
        with np.errstate(all='ignore'):
            boxes = O.decode(inp['loc'][b], priors(P), (0.1, 0.2))
        for cl in range(1, C):
            s = sc[b, :, cl]
            sel = np.nonzero(s >= t if thresh_ge else s > t)[0]
            keep = sel[nms_plain(boxes[sel], s[sel], prm['nms_thresh'], top_k, **nms_switches)] if sel.size else sel
            out[b, cl, :keep.size, 0], out[b, cl, :keep.size, 1:] = s[keep], boxes[keep]
            keeps[(b, cl)] = keep
    return out, keeps


DETECT_SWITCHES = ('tie_high', 'iou_lt', 'thresh_ge', 'topk_after', 'dead_suppress')
NMS_SWITCHES = ('tie_high', 'iou_lt', 'topk_after', 'dead_suppress')


# ==========================================================================================================================================
# MultiBoxLoss
# ==========================================================================================================================================
def loss_oracle(inp, prm):
    with np.errstate(all='ignore'):
        ll, lc, d = O.multibox_loss(inp['loc'], inp['conf'], priors(inp['loc'].shape[1]), inp['targets'], details=True)
    P = inp['loc'].shape[1]
    d['num_neg'] = np.minimum(3 * d['num_pos'], P - 1)
    d['losses'] = np.array([ll, lc], np.float64)
    return d


def loss_distinct(inp, res):
    """Mining scores pairwise distinct per image among the non-positives (positives are zeroed: they tie, and are selected anyway)."""
    for b in range(res['loss_c_all'].shape[0]):
        s = res['loss_c_all'][b][~res['pos'][b]]
        if np.unique(s).size != s.size:
            return False
    return True


def _loss_row(name, P, C, make_targets, pre, fixture=True, conf_kind='rand', B=3, extra=None, salt=0):
    def build():
        rng = np.random.default_rng(seed_of(name) + salt)
        loc = rng.normal(0, 1.0, size=(B, P, 4)).astype(np.float32)
        conf = rng.normal(0, 2.0, size=(B, P, C)).astype(np.float32)
        if conf_kind == 'zeros':
            conf[:] = 0
        elif conf_kind == 'quant':
            conf = np.clip(np.round(conf * 4) / 4, -1, 1).astype(np.float32)        # quarters in [-1, 1], every foreground logit the same:
            conf[:, :, 2:] = conf[:, :, 1:2]                                       # 81 different rows, so the mining scores tie in groups
        return dict(loc=loc, conf=conf, targets=make_targets(rng, priors(P)))
    return Row(name, dict(P=P, C=C, B=B, **(extra or {})), build, pre, fixture)


def near_prior_boxes(rng, pri, n, C):
    """n boxes, each a randomly chosen prior moved by about a tenth of its size: the first P priors cover a corner of the image only, and a
    box elsewhere overlaps none of them."""
    k = rng.integers(0, pri.shape[0], n)
    t = np.concatenate([prior_box_as_target(pri, i) for i in k], 0)
    t[:, :4] += rng.normal(0, 0.008, (n, 4)).astype(np.float32)
    t[:, 4] = rng.integers(0, C - 1, n)
    return t


def _counts_targets(C, counts=(3, 1, 2)):
    def make(rng, pri):
        tg = [near_prior_boxes(rng, pri, n, C) for n in counts]
        tg[0][-1, 4] = C - 2                 # a box forces its best prior (the last box wins it): the label C - 2 reaches conf_t as C - 1
        return tg
    return make


def _pre_top_label(C):
    def pre(inp, res):
        return bool((res['conf_t'] == C - 1).any() and res['pos'].any(1).all())         # "conf_t == C - 1 occurs"
    return pre


def _loss_clip():
    C, P = 5, 65

    def make(rng, pri):
        def many():          # 64 boxes: priors 0..55 themselves (each forces its own prior) and priors 0..7 again under another label; the
            t = np.concatenate([prior_box_as_target(pri, k % 56) for k in range(64)], 0)     # priors of the last two cells stay negative
            t[:, 4] = rng.integers(0, C - 1, size=64)
            return t
        return [many(), near_prior_boxes(rng, pri, 1, C), many()]

    def pre(inp, res):
        mined_pos = res['pos'] & res['neg']                                             # the kernel's sel == 3: "a prior is marked 3"
        n_negative = int((~res['pos'][0]).sum())
        return bool(res['num_pos'][0] >= 56 and res['num_neg'][0] == P - 1 and 3 * res['num_pos'][0] > P - 1 and n_negative > 0   # "num_neg == P - 1"
                    and mined_pos[0].sum() == P - 1 - n_negative and res['num_neg'][1] < P - 1)
    return _loss_row('clip', P, C, make, pre, fixture=False)


def _loss_forced():
    C, P = 5, 65

    def make(rng, pri):
        a, a2 = prior_box_as_target(pri, 32, 0.), prior_box_as_target(pri, 32, C - 2)   # identical boxes, different labels
        return [np.concatenate([a, a2, near_prior_boxes(rng, pri, 1, C)], 0),
                np.concatenate([prior_box_as_target(pri, P // 2), FAR], 0),             # IoU exactly 1; a box that overlaps nothing
                FAR.copy()]

    def pre(inp, res):
        ct = res['conf_t']
        twins = ct[0, 32] == C - 1 and (ct[0] == 1).sum() >= 1       # the later twin owns the forced prior, the earlier one its neighbours
        return bool(twins and ct[1, P // 2] == 1 and ct[1, 0] == 1 and ct[2, 0] == 1 and (ct[2, 1:] == 0).all())
    return _loss_row('forced', P, C, make, pre)


def _loss_no_box():
    def make(rng, pri):
        return [near_prior_boxes(rng, pri, 2, 5), np.zeros((0, 5), np.float32), near_prior_boxes(rng, pri, 1, 5)]

    def pre(inp, res):
        return res['num_pos'][1] == 0 and not res['neg'][1].any() and res['num_pos'][0] > 0 and res['num_pos'][2] > 0
    return _loss_row('no_box', 65, 5, make, pre, fixture=False)


def _pre_ties(every):
    """The cut falls inside a group of equal mining scores: in every image, or in one at least."""
    def pre(inp, res):
        hit = []
        for b in range(res['loss_c_all'].shape[0]):
            s = np.sort(res['loss_c_all'][b])[::-1]
            k = int(res['num_neg'][b])
            hit.append(0 < k < s.size and s[k - 1] == s[k])
        return bool(all(hit) if every else any(hit))
    return pre


GRADS = (('scaled', 0.5, -2.0), ('default', 1.0, 1.0), ('none_c', 1.0, None))      # (name, grad_l, grad_c) of the backward rows

LOSS = [_loss_row(f'C_edges-C{C}-P{P}', P, C, _counts_targets(C), _pre_top_label(C)) for C in (2, 3, 4, 5, 8) for P in (65, 1025)]
LOSS += [_loss_row(f'P_edges-P{P}', P, 5, _counts_targets(5), _pre_top_label(5), salt=P == 2500) for P in (1, 7, 2500)]   # (salt: distinct scores)
LOSS += [_loss_clip(),
         _loss_row('ties_zero', 1025, 5, _counts_targets(5), _pre_ties(True), fixture=False, conf_kind='zeros'),
         _loss_row('ties_quant', 1025, 5, _counts_targets(5, (3, 1, 3)), _pre_ties(True), fixture=False, conf_kind='quant'),
         _loss_forced(), _loss_no_box()]
LOSS += [_loss_row(f'backward-C{C}', 65, C, _counts_targets(C), _pre_top_label(C), extra=dict(backward=True)) for C in (2, 5)]
LOSS_TIE_ROWS = ('clip', 'ties_zero', 'ties_quant')      # the fixture holds conf_t, positives, num_neg and the losses only
LOSS_ORACLE_ONLY = ('no_box',)


def loss_plain(inp, first_twin=False, last_max=False, no_clip=False, tie_high=False, keep_pos=False):
    """Matching and mining as loops, with a switch per classic mistake -> dict(conf_t, pos, neg, num_neg)."""
    conf = inp['conf']
    B, P, C = conf.shape
    pri = priors(P)
    conf_t = np.zeros((B, P), np.int64)
    for b in range(B):
        t = np.asarray(inp['targets'][b], f32)
        if t.shape[0] == 0:
            continue
        ov = O.jaccard(t[:, :4], O.point_form(pri))                  # [n, P]
        best_truth, best_ov = np.zeros(P, np.int64), np.full(P, -np.inf, f32)
        for j in range(t.shape[0]):
            for p in range(P):
                if ov[j, p] > best_ov[p] or (last_max and ov[j, p] == best_ov[p]):
                    best_ov[p], best_truth[p] = ov[j, p], j
        forced = {}
        for j in range(t.shape[0]):
            bp = int(np.argmax(ov[j]))
            if not (first_twin and bp in forced):
                forced[bp] = j
        for p, j in forced.items():
            best_ov[p], best_truth[p] = 2, j
        conf_t[b] = np.where(best_ov < f32(0.5), 0, t[best_truth, 4].astype(np.int64) + 1)
    pos = conf_t > 0
    x_max = conf.max()
    with np.errstate(all='ignore'):
        lse = np.log(np.exp(conf - x_max).sum(axis=2, dtype=f32)) + x_max
    lca = (lse - np.take_along_axis(conf, conf_t[:, :, None], 2)[:, :, 0]).astype(f32)
    if not keep_pos:
        lca[pos] = 0
    num_neg = 3 * pos.sum(1)
    if not no_clip:
        num_neg = np.minimum(num_neg, P - 1)
    neg = np.zeros((B, P), bool)
    for b in range(B):
        order = sorted(range(P), key=lambda p: (-float(lca[b, p]), -p if tie_high else p))
        neg[b, order[:int(num_neg[b])]] = True
    return dict(conf_t=conf_t, pos=pos, neg=neg, num_neg=num_neg)


LOSS_SWITCHES = ('first_twin', 'last_max', 'no_clip', 'tie_high', 'keep_pos')


# ==========================================================================================================================================
# AP / IoBB evaluator
# ==========================================================================================================================================
def eval_oracle(inp, prm, use07):
    with np.errstate(all='ignore'):
        r = EO.evaluate(inp['det'], inp['scales'], inp['gts'], prm['thresh'], prm['ap_list'], prm['iobb_list'], use07, details=True)
    if len(r) == 2:                  # no detection at all
        return dict(ap=r[0], iobb=r[1], tp=np.zeros((len(prm['ap_list']) + len(prm['iobb_list']), 0)), fp=None, conf=np.zeros(0))
    return dict(ap=r[0], iobb=r[1], **r[2])


def eval_distinct(inp, prm):
    s = inp['det'][:, 1, :, 0].astype(np.float64)
    s = s[(s > 0) & (s > prm['thresh'])]
    return np.unique(s).size == s.size


def batch_splits(N):
    """Unequal add_batch sizes: [0, a, b, N]."""
    a = max(1, N // 4)
    return sorted({0, a, min(N, a + max(1, N // 2 + 1)), N})


def distinct_scores(rng, n, lo=0.06, hi=0.99):
    return (lo + (hi - lo) * (rng.permutation(n) + 0.5) / n).astype(np.float32)


def grid_gt(n, W, H):
    """n disjoint boxes on a 16 x 16 grid of a W x H image (pixels, float64)."""
    j = np.arange(n)
    cw, ch = W / 16., H / 16.
    x, y = (j % 16) * cw, (j // 16) * ch
    return np.stack([x + 0.125 * cw, y + 0.125 * ch, x + 0.75 * cw, y + 0.75 * ch], 1).astype(np.float64)


def pack_det(rows_per_image, top_k):
    """Lists of [score, x1, y1, x2, y2] (normalised) per image -> det[N, 2, top_k, 5]: descending score, zero rows behind, like Detect."""
    det = np.zeros((len(rows_per_image), 2, top_k, 5), np.float32)
    for n, rows in enumerate(rows_per_image):
        if len(rows):
            r = np.asarray(rows, np.float32).reshape(-1, 5)
            r = r[np.argsort(-r[:, 0], kind='stable')][:top_k]
            det[n, 1, :r.shape[0]] = r
    return det


def scales_of(sizes):
    return np.array([[w, h, w, h] for w, h in sizes], np.float32)


def jitter_rows(rng, g, W, H, n, sd=0.01):
    """n detections around ground-truth boxes g (pixels) picked at random, as normalised corner rows without a score."""
    pick = g[rng.integers(0, g.shape[0], n)] / np.array([W, H, W, H])
    return pick + rng.normal(0, sd, (n, 4))


def random_rows(rng, n):
    c, w = rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.03, 0.3, (n, 2))
    return np.concatenate([c - w / 2, c + w / 2], 1)


def with_scores(scores, boxes):
    return np.concatenate([np.asarray(scores, np.float64).reshape(-1, 1), boxes], 1)


def eval_overlaps(inp, prm):
    """(image, row, IoU[n_gt], IoBB[n_gt]) of every detection the evaluator keeps, from the inputs alone (float64, as test_net)."""
    for n in range(inp['det'].shape[0]):
        G = inp['gts'][n]
        for d, row in enumerate(inp['det'][n, 1]):
            if not (row[0] > 0 and float(row[0]) > prm['thresh']) or G.shape[0] == 0:
                continue
            bb = (row[1:] * inp['scales'][n]).astype(np.float64)
            iw = np.maximum(np.minimum(G[:, 2], bb[2]) - np.maximum(G[:, 0], bb[0]), 0.)
            ih = np.maximum(np.minimum(G[:, 3], bb[3]) - np.maximum(G[:, 1], bb[1]), 0.)
            area = (bb[2] - bb[0]) * (bb[3] - bb[1])
            with np.errstate(all='ignore'):
                yield n, d, iw * ih / (area + (G[:, 2] - G[:, 0]) * (G[:, 3] - G[:, 1]) - iw * ih), iw * ih / area


EV_DEFAULTS = dict(thresh=0.05, ap_list=(0.1, 0.5), iobb_list=(0.1, 0.5), top_k=200)
GT_COUNTS = (0, 1, 64, 65, 130, 256)
DUPS = ((5, 69), (0, 64), (3, 100))          # (j, j + 64): the same lane of eval_match; (3, 100): different lanes


def _ev_gt_edges():
    name = 'gt_edges'

    def build():
        rng = np.random.default_rng(seed_of(name))
        W = H = 512
        gts, rows = [], []
        for ng in GT_COUNTS:
            g = grid_gt(ng, W, H)
            hits = []
            for lo, hi in DUPS:
                if hi < ng:
                    g[hi] = g[lo]                                      # an exact IoU tie for whatever overlaps the pair
                    hits += [g[lo] / W, g[lo] / W + 0.002]             # two detections on the pair: the lower index takes the first,
            gts.append(g)                                              # and being used makes the second a false positive
            b = np.concatenate([np.asarray(hits).reshape(-1, 4), jitter_rows(rng, g, W, H, 12) if ng else np.zeros((0, 4)),
                                random_rows(rng, 6)], 0)
            rows.append(b)
        sc = distinct_scores(rng, sum(r.shape[0] for r in rows))
        off = np.cumsum([0] + [r.shape[0] for r in rows])
        det = pack_det([with_scores(sc[off[i]:off[i + 1]], r) for i, r in enumerate(rows)], 200)
        return dict(det=det, scales=scales_of([(W, H)] * len(gts)), gts=gts)

    def pre(inp, res):
        same_lane = cross_lane = False
        for n, d, iou, _ in eval_overlaps(inp, EV_DEFAULTS):
            top = np.nonzero(iou == iou.max())[0]
            if top.size >= 2 and iou.max() > 0.5:
                same_lane |= (top[1] - top[0]) % 64 == 0
                cross_lane |= (top[1] - top[0]) % 64 != 0
        counts = tuple(g.shape[0] for g in inp['gts'])
        no_gt_dets = (inp['det'][0, 1, :, 0] > 0.05).any()             # detections of the image without boxes: neither TP nor FP
        return counts == GT_COUNTS and same_lane and cross_lane and no_gt_dets
    return Row(name, dict(EV_DEFAULTS), build, pre, True)


def _ev_metrics(tag, ap_list, iobb_list):
    name = f'metrics-{tag}'

    def build():
        rng = np.random.default_rng(seed_of(name))
        W = H = 400
        gts, rows = [], []
        for n in range(5):
            g = np.array([[100., 100., 200., 200.], [250., 40., 330., 120.]])[:1 + n % 2]
            gts.append(g)
            weak = np.array([[100., 100., 150., 160.]]) / W           # detection 1: IoU 0.3 with box 0 (TP at 0.1 .. 0.2, FP above)
            good = np.array([[101., 101., 199., 199.]]) / W           # detection 2: IoU 0.96 with the same box, lower score
            rows.append(np.concatenate([weak, good, jitter_rows(rng, g, W, H, 4, 0.02), random_rows(rng, 3)], 0))
        sc = [np.concatenate([[0.9 - 0.01 * n, 0.8 - 0.01 * n], 0.1 + 0.6 * (rng.permutation(7) + n / 5.) / 7.]) for n in range(5)]
        det = pack_det([with_scores(s, r) for s, r in zip(sc, rows)], 16)
        return dict(det=det, scales=scales_of([(W, H)] * 5), gts=gts)

    def pre(inp, res):
        tp, fp = res['tp'], res['fp']
        nm = len(ap_list) + len(iobb_list)
        if tp.shape[0] != nm or nm == 1:
            return tp.shape[0] == nm
        lo, hi = ap_list.index(0.1), ap_list.index(0.5)
        first = ((tp[lo] == 1) & (fp[hi] == 1)).any()                 # detection 1: TP at 0.1, FP at 0.5 ...
        second = ((fp[lo] == 1) & (tp[hi] == 1)).any()                # ... detection 2: TP at 0.5 on the box that 0.1 has used up
        return bool(first and second)
    return Row(name, dict(EV_DEFAULTS, ap_list=ap_list, iobb_list=iobb_list, top_k=16), build, pre, True)


def _ev_M_edges(N, top_k, full=()):
    name = f'M_edges-N{N}-k{top_k}'

    def build():
        rng = np.random.default_rng(seed_of(name))
        W, H = 300, 300
        gts, rows = [], []
        for n in range(N):
            g = grid_gt(int(rng.integers(1, 4)), W, H) * 4             # 1-3 boxes of 42 x 42 pixels
            gts.append(g)
            nd = top_k if n in full or top_k == 1 else int(rng.integers(0, min(top_k, 12) + 1))
            rows.append(np.concatenate([jitter_rows(rng, g, W, H, nd - nd // 2, 0.02), random_rows(rng, nd // 2)], 0))
        sc = distinct_scores(rng, sum(r.shape[0] for r in rows))
        off = np.cumsum([0] + [r.shape[0] for r in rows])
        det = pack_det([with_scores(sc[off[i]:off[i + 1]], r) for i, r in enumerate(rows)], top_k)
        return dict(det=det, scales=scales_of([(W, H)] * N), gts=gts)

    def pre(inp, res):
        used = (inp['det'][:, 1, :, 0] > 0.05).sum(1)
        return inp['det'].shape[0] * inp['det'].shape[2] == N * top_k and all(used[n] == top_k for n in full) and res['tp'].sum() > 0
    return Row(name, dict(EV_DEFAULTS, top_k=top_k, M=N * top_k), build, pre, True)


def _ev_conf_ties():
    name = 'conf_ties'

    def build():
        rng = np.random.default_rng(seed_of(name))
        W = H = 512
        gts, rows = [], []
        for n in range(6):
            g = grid_gt(3, W, H) * 3
            gts.append(g)
            b = np.concatenate([jitter_rows(rng, g, W, H, 6, 0.02), random_rows(rng, 4)], 0)
            rows.append(with_scores(rng.choice([0.75, 0.5, 0.5, 0.25, 0.125], 10), b[rng.permutation(10)]))
        return dict(det=pack_det(rows, 200), scales=scales_of([(W, H)] * 6), gts=gts)

    def pre(inp, res):
        s = inp['det'][:, 1, :, 0]
        within = any(np.unique(r[r > 0]).size < (r > 0).sum() for r in s)
        across = np.intersect1d(s[0][s[0] > 0], s[1][s[1] > 0]).size > 0
        t = res['tp'][1] + 2 * res['fp'][1]
        mixed = any(np.unique(t[res['conf'] == v]).size > 1 for v in np.unique(res['conf']))     # the order among equals decides the curve
        return within and across and mixed
    return Row(name, dict(EV_DEFAULTS), build, pre, False)


def _ev_thresh_strict(thresh):
    """thresh = 0.25 is a float32: a score can equal it (excluded: strict >).  thresh = 0.05 is not: float32(0.05) lies above it in
    float64, where test_net compares (kept), and the float32 below it is excluded."""
    name = f'thresh_strict-t{thresh}'
    t32 = f32(thresh)
    edge = (t32, np.nextafter(t32, f32(1))) if float(t32) == thresh else (np.nextafter(t32, f32(0)), t32)      # (excluded, kept)

    def build():
        rng = np.random.default_rng(seed_of(name))
        W = H = 400
        gts, rows = [], []
        for n in range(4):
            g = np.array([[0., 0., 100., 100.], [200., 200., 300., 280.]])
            gts.append(g)
            b = np.concatenate([jitter_rows(rng, g, W, H, 5, 0.02), random_rows(rng, 3), jitter_rows(rng, g, W, H, 4, 0.02)], 0)
            sc = np.concatenate([thresh + 0.1 + 0.5 * (rng.permutation(8) + n / 4.) / 8., [edge[1] if n == 0 else thresh + 0.01 * (n + 1), edge[0]],
                                 thresh * np.array([.9, .5])])
            if n == 1:                                                 # IoU and IoBB exactly 0.5 with box 0: not above the 0.5 thresholds
                b[0], sc[0] = np.array([0., 0., 100., 200.]) / W, 0.95
            rows.append(with_scores(sc, b))
        return dict(det=pack_det(rows, 24), scales=scales_of([(W, H)] * 4), gts=gts)

    def pre(inp, res):
        s = inp['det'][:, 1, :, 0]
        at_half = any(iou.max() == 0.5 and iobb.max() == 0.5 for _, _, iou, iobb in eval_overlaps(inp, dict(thresh=thresh)))
        kept = int(((s > 0) & (s.astype(np.float64) > thresh)).sum())
        return (s == edge[0]).sum() == 4 and (s == edge[1]).sum() == 1 and ((s > 0) & (s < edge[0])).sum() == 8 and (s == 0).any() \
            and kept == 4 * 9 == res['conf'].shape[0] and at_half and float(edge[1]) > thresh >= float(edge[0])
    return Row(name, dict(EV_DEFAULTS, thresh=thresh, top_k=24), build, pre, True)


def _ev_degenerate():
    name = 'degenerate'

    def build():
        rng = np.random.default_rng(seed_of(name))
        W = H = 400
        gts, rows = [], []
        for n in range(3):
            g = np.array([[40., 40., 140., 140.], [200., 200., 300., 280.]])
            gts.append(g)
            b = np.concatenate([jitter_rows(rng, g, W, H, 4, 0.02), [[.2, .2, .2, .3]],          # zero area inside box 0: IoBB = 0 / 0
                                [[.8, .05, .95, .15]]], 0)                                      # overlaps no box
            rows.append(with_scores(0.1 + 0.8 * (rng.permutation(6) + n / 3.) / 6., b))
        return dict(det=pack_det(rows, 8), scales=scales_of([(W, H)] * 3), gts=gts)

    def pre(inp, res):
        nan_iobb = sum(bool(np.isnan(iobb).all()) for _, _, _, iobb in eval_overlaps(inp, EV_DEFAULTS))
        none = sum(bool((iou == 0).all()) for _, _, iou, _ in eval_overlaps(inp, EV_DEFAULTS))
        return nan_iobb == 3 and none >= 3
    return Row(name, dict(EV_DEFAULTS, top_k=8), build, pre, True)


def _ev_npos_zero():
    name = 'npos_zero'

    def build():
        rng = np.random.default_rng(seed_of(name))
        rows = [random_rows(rng, 5) for _ in range(3)]
        sc = distinct_scores(rng, 15)
        det = pack_det([with_scores(sc[5 * i:5 * i + 5], r) for i, r in enumerate(rows)], 8)
        return dict(det=det, scales=scales_of([(300, 300)] * 3), gts=[np.zeros((0, 4))] * 3)

    def pre(inp, res):
        return res['npos'] == 0 and res['conf'].shape[0] == 15 and res['tp'].sum() == 0 and res['fp'].sum() == 0
    return Row(name, dict(EV_DEFAULTS, top_k=8), build, pre, True)


def _ev_scales():
    name = 'scales'
    sizes = [(512, 300), (300, 512), (640, 480), (200, 333), (512, 512)]

    def build():
        rng = np.random.default_rng(seed_of(name))
        gts, rows = [], []
        for W, H in sizes:
            g = grid_gt(3, W, H) * 3
            gts.append(g)
            rows.append(np.concatenate([jitter_rows(rng, g, W, H, 6, 0.015), random_rows(rng, 3)], 0))
        sc = distinct_scores(rng, 45)
        det = pack_det([with_scores(sc[9 * i:9 * i + 9], r) for i, r in enumerate(rows)], 16)
        return dict(det=det, scales=scales_of(sizes), gts=gts)

    def pre(inp, res):
        s = inp['scales']
        return (s[:, 0] != s[:, 1]).any() and np.unique(s, axis=0).shape[0] == len(sizes) and res['tp'].sum() > 0
    return Row(name, dict(EV_DEFAULTS, top_k=16), build, pre, True)


EIGHT = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8)
EVAL = [_ev_gt_edges(),
        _ev_metrics('4+4', (0.1, 0.3, 0.5, 0.7), (0.1, 0.3, 0.5, 0.7)), _ev_metrics('8+0', EIGHT, ()), _ev_metrics('0+1', (), (0.1,)),
        _ev_M_edges(21, 1), _ev_M_edges(8, 128, full=(2,)), _ev_M_edges(5, 205, full=(1, 4)), _ev_M_edges(3, 683, full=(0,)),
        _ev_M_edges(3, 200, full=(0, 2)),
        _ev_conf_ties(), _ev_thresh_strict(0.25), _ev_thresh_strict(0.05), _ev_degenerate(), _ev_npos_zero(), _ev_scales()]
M_WANTED = (21, 1024, 1025, 2049)


def eval_plain(inp, prm, use07, last_max=False, shared_used=False, ov_ge=False, score_ge=False, ties_reversed=False, nogt_fp=False):
    """make_pred's filter, the global sort and test_net's greedy loop as plain loops, with a switch per classic mistake
    -> dict(tp, fp [n_metrics, nd] in sorted order, ap, iobb)."""
    thr = [('iou', t) for t in prm['ap_list']] + [('iobb', t) for t in prm['iobb_list']]
    dets = []
    for n in range(inp['det'].shape[0]):
        for d, row in enumerate(inp['det'][n, 1]):
            s = float(row[0])
            if row[0] > 0 and (s >= prm['thresh'] if score_ge else s > prm['thresh']):
                dets.append((s, n, d, (row[1:] * inp['scales'][n]).astype(np.float64)))
    dets.sort(key=lambda x: (-x[0], (-x[1], -x[2]) if ties_reversed else (x[1], x[2])))
    used = [[set() for _ in inp['gts']] for _ in thr]
    tp, fp = np.zeros((len(thr), len(dets))), np.zeros((len(thr), len(dets)))
    for i, (s, n, d, bb) in enumerate(dets):
        G = inp['gts'][n]
        if G.shape[0] == 0:
            fp[:, i] = 1. if nogt_fp else 0.
            continue
        area = (bb[2] - bb[0]) * (bb[3] - bb[1])
        ovs = {'iou': [], 'iobb': []}
        for g in G:
            inter = max(min(g[2], bb[2]) - max(g[0], bb[0]), 0.) * max(min(g[3], bb[3]) - max(g[1], bb[1]), 0.)
            with np.errstate(all='ignore'):
                ovs['iou'].append(np.float64(inter) / (area + (g[2] - g[0]) * (g[3] - g[1]) - inter))
                ovs['iobb'].append(np.float64(inter) / area)
        for m, (kind, t) in enumerate(thr):
            ov = ovs[kind]
            if any(np.isnan(v) for v in ov):
                fp[m, i] = 1.                                          # np.max is NaN: no comparison holds
                continue
            j = 0
            for q in range(1, len(ov)):
                if ov[q] > ov[j] or (last_max and ov[q] == ov[j]):
                    j = q
            u = used[0 if shared_used else m][n]
            if (ov[j] >= t if ov_ge else ov[j] > t) and j not in u:
                tp[m, i] = 1.
                u.add(j)
            else:
                fp[m, i] = 1.
    npos = sum(g.shape[0] for g in inp['gts'])
    out = []
    with np.errstate(all='ignore'):
        for m in range(len(thr)):
            f, t_ = np.cumsum(fp[m]), np.cumsum(tp[m])
            out.append(EO.voc_ap(t_ / float(npos), t_ / np.maximum(t_ + f, np.finfo(np.float64).eps), use07) if len(dets) else 0.)
    na = len(prm['ap_list'])
    return dict(tp=tp, fp=fp, ap=out[:na], iobb=out[na:])


EVAL_SWITCHES = ('last_max', 'shared_used', 'ov_ge', 'score_ge', 'ties_reversed', 'nogt_fp')

FAMILIES = dict(detect=DETECT, nms=NMS, loss=LOSS, eval=EVAL)


def by_name(family, name):
    return next(r for r in FAMILIES[family] if r.name == name)


# ==========================================================================================================================================
# tests/golden/index_edges.npz: what the reference computes for the fixture rows (make_golden_index_edges.py), packed per family
# ==========================================================================================================================================
def sample_positions(n, count=12):
    """Which of n kept rows have their five values stored (the indices are stored whole): evenly spread, both ends included."""
    return np.unique(np.linspace(0, n - 1, min(n, count)).astype(np.int64)) if n else np.zeros(0, np.int64)


def pack_rows(prefix, rows):
    """{row name: {key: array}} -> flat npz entries: per key one concatenated array and the shapes, plus the row names."""
    out = {f'{prefix}.names': np.array(list(rows))}
    keys = sorted({k for r in rows.values() for k in r})
    for k in keys:
        arrs = [np.asarray(r[k]) if k in r else None for r in rows.values()]
        some = next(a for a in arrs if a is not None)
        nd = max(a.ndim for a in arrs if a is not None)
        shape = np.full((len(arrs), nd + 1), -1, np.int32)       # column 0: number of dimensions, -1 = the row has no such key
        for i, a in enumerate(arrs):
            if a is not None:
                shape[i, 0] = a.ndim
                shape[i, 1:1 + a.ndim] = a.shape
        out[f'{prefix}.{k}'] = np.concatenate([a.ravel() for a in arrs if a is not None]).astype(some.dtype)
        out[f'{prefix}.{k}.shape'] = shape
    return out


def unpack_rows(g, prefix):
    names = [str(n) for n in g[f'{prefix}.names']]
    rows = {n: {} for n in names}
    for entry in g.files:
        if not entry.startswith(prefix + '.') or entry.endswith('.shape') or entry == f'{prefix}.names':
            continue
        k, flat, shape, at = entry[len(prefix) + 1:], g[entry], g[entry + '.shape'], 0
        for i, n in enumerate(names):
            if shape[i, 0] < 0:
                continue
            shp = tuple(int(v) for v in shape[i, 1:1 + shape[i, 0]])
            size = int(np.prod(shp, dtype=np.int64))
            rows[n][k] = flat[at:at + size].reshape(shp)
            at += size
    return rows
