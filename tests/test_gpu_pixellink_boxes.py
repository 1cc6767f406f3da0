"""GPU tests of the PixelLink++ evaluation path: the box-tail kernel (gssd_pixellink_boxes_f32) through the C entry against
pixel_link/box_geometry.py on every row of tests/pixellink_box_cases.py (tests/test_pixellink_box_cases_cpu.py proves the rows fit for an
exact comparison), ``mask_to_box_device`` against the host ``mask_to_box``, and ``pixel_link.evaluate.test_net(use_pixel_link=True)`` against the
evaluation oracle fed with the host detections."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pixellink_box_cases as R                       # noqa: E402

SCORE_TOL = 1e-6         # absolute, the tolerance of test_decode_vs_reference_fixture: a few fp32 ulps of a value below 1
SENT, ISENT = -7.25, -77


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


_EXPECTED = {}


def expected(row):
    if row['name'] not in _EXPECTED:
        _EXPECTED[row['name']] = R.host_expected(row)
    return _EXPECTED[row['name']]


class Launch:
    """One call of the C entry with ``det`` and ``ndet`` embedded between sentinels: a guard in front, the class-0 planes, one more image
    behind the last, and a guard element on either side of ``ndet``."""
    GUARD = 64

    def __init__(self, dev, labels, logits, max_det):
        self.B, self.max_det = labels.shape[0], max_det
        self.labels, self.logits = torch.from_numpy(labels).to(dev), torch.from_numpy(logits).to(dev)
        self.labels0, self.logits0 = self.labels.clone(), self.logits.clone()
        self.flat = torch.full((self.GUARD + (self.B + 1) * 2 * max_det * 5,), SENT, device=dev)
        self.det = self.flat[self.GUARD:].view(self.B + 1, 2, max_det, 5)
        self.nflat = torch.full((self.B + 2,), ISENT, device=dev, dtype=torch.int32)
        self.ncomp = torch.from_numpy(labels.reshape(self.B, -1).max(1).astype(np.int32)).to(dev)

    def __call__(self, dst, min_height, min_area, with_ncomp=True, h=None, w=None, max_det=None, stride=None, B=None, by_score=0):
        from gssd import _lib
        _, hh, ww = self.labels.shape
        rc = _lib.lib.gssd_pixellink_boxes_f32(self.labels.data_ptr(), self.logits.data_ptr(), self.ncomp.data_ptr() if with_ncomp else None,
                                               self.det[:, 1].data_ptr(), 2 * self.max_det * 5 if stride is None else stride,
                                               self.nflat[1:].data_ptr(), self.B if B is None else B, hh if h is None else h,
                                               ww if w is None else w, dst[0], dst[1], float(min_height), float(min_area),
                                               self.max_det if max_det is None else max_det, by_score, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.flat == SENT).all()) and bool((self.nflat == ISENT).all())

    def check_surroundings(self):
        assert bool((self.flat[:self.GUARD] == SENT).all()) and bool((self.det[:, 0] == SENT).all()) and bool((self.det[self.B] == SENT).all())
        assert int(self.nflat[0]) == ISENT and int(self.nflat[-1]) == ISENT
        assert torch.equal(self.labels, self.labels0) and torch.equal(self.logits, self.logits0)

    def results(self):
        return self.det[:self.B, 1].cpu().numpy(), self.nflat[1:-1].cpu().numpy()


def assert_matches(det, ndet, exp, name):
    for b, (boxes, scores) in enumerate(exp):
        n = len(boxes)
        assert int(ndet[b]) == n, (name, b, int(ndet[b]), n)
        assert np.array_equal(det[b, :n, 1:], np.asarray(boxes, np.float32).reshape(n, 4)), (name, b)
        err = np.abs(det[b, :n, 0].astype(np.float64) - np.asarray(scores, np.float64))
        print(name, 'image', b, 'components', n, 'max score error', float(err.max()) if n else 0.0)
        assert n == 0 or err.max() <= SCORE_TOL, (name, b, float(err.max()))
        assert not det[b, n:].any(), (name, b)


@pytest.mark.parametrize('row', R.all_rows(), ids=lambda r: r['name'])
def test_kernel_equals_the_definition(dev, row):
    """Integer boxes and ndet equal component_boxes exactly, scores to 1e-6; rows past ndet are zero; everything around det / ndet and the
    inputs come back untouched.  With the component counts given and with the kernel finding the largest label itself."""
    for with_ncomp in (True, False):
        run = Launch(dev, row['labels'], row['logits'], R.MAX_DET if row['labels'].max() > 16 else 16)
        assert run(row['dst'], row['min_height'], row['min_area'], with_ncomp) == 0
        run.check_surroundings()
        assert_matches(*run.results(), expected(row), row['name'])


def test_kernel_ignores_labels_beyond_max_det(dev):
    row = next(r for r in R.hand_made_rows() if r['name'] == 'concave_and_order')
    assert row['labels'].max() == 7
    cut = dict(row, name='cut', labels=np.where(row['labels'] <= 4, row['labels'], 0).astype(np.int32))
    for with_ncomp in (True, False):
        run = Launch(dev, row['labels'], row['logits'], 4)
        assert run(row['dst'], row['min_height'], row['min_area'], with_ncomp) == 0
        run.check_surroundings()
        assert_matches(*run.results(), R.host_expected(cut), 'max_det 4')


@pytest.mark.parametrize('name', ['concave_and_order', 'seeded150'])
def test_kernel_orders_by_score_on_request(dev, name):
    """by_score: each image's kept components by descending score, equal scores in label order."""
    row = next(r for r in R.all_rows() if r['name'] == name)
    run = Launch(dev, row['labels'], row['logits'], R.MAX_DET)
    assert run(row['dst'], row['min_height'], row['min_area'], by_score=1) == 0
    run.check_surroundings()
    by_label = Launch(dev, row['labels'], row['logits'], R.MAX_DET)
    assert by_label(row['dst'], row['min_height'], row['min_area']) == 0
    (det, ndet), (ref, nref) = run.results(), by_label.results()
    assert np.array_equal(ndet, nref) and int(nref.max()) > 2
    for b in range(len(ndet)):
        order = np.argsort(-ref[b, :nref[b], 0], kind='stable')
        assert np.array_equal(det[b, :nref[b]], ref[b, :nref[b]][order]) and not det[b, nref[b]:].any()
    assert not np.array_equal(det, ref)


def test_refused_arguments_write_nothing(dev):
    from gssd import _lib
    row = next(r for r in R.hand_made_rows() if r['name'] == 'ties_identity')
    run = Launch(dev, row['labels'], row['logits'], 16)
    f = (row['min_height'], row['min_area'])
    bad = [dict(h=164, w=163),                            # h * w beyond the decode's 26624
           dict(max_det=1025), dict(max_det=0), dict(h=0), dict(w=-1), dict(B=0), dict(stride=5 * 16 - 1)]
    for kw in bad:
        assert run(row['dst'], *f, **kw) == -1 and b'invalid argument' in _lib.lib.gssd_last_error(), kw
        assert run.untouched(), kw
    # non-positive; beyond 16-bit coordinates; more than 2^22 destination pixels; tables beyond the LDS (16 x 65536 pixels pass the count)
    for dst in ((0, 40), (40, 0), (65537, 40), (2048, 2049), (16, 65536)):
        assert run(dst, *f) == -1 and run.untouched(), dst
    assert run(row['dst'], *f) == 0 and not run.untouched()


@pytest.mark.parametrize('name', ['fixture75', 'seeded150'])
@pytest.mark.parametrize('B', [3, 1])
def test_mask_to_box_device_equals_mask_to_box(dev, name, B):
    from pixel_link import postprocess
    o1, o2 = (torch.from_numpy(np.ascontiguousarray(a[:B])).to(dev) for a in R.seeded_maps()[name])
    det, ndet = postprocess.mask_to_box_device(o1, o2)
    assert tuple(det.shape) == (B, 2, 1024, 5) and det.is_cuda and ndet.dtype == torch.int32 and not det[:, 0].any()
    host = postprocess.mask_to_box(o1, o2)
    exp = [([d[1:] for d in img], [d[0] for d in img]) for img in host]
    assert_matches(det[:, 1].cpu().numpy(), ndet.cpu().numpy(), exp, f'{name} B={B}')


def _isolated_pixels(dev, count):
    """Score maps [1, 2 / 16, 66, 64] that decode to ``count`` one-pixel components (every other row and column, no link on)."""
    o1 = torch.zeros(1, 2, 66, 64)
    o1[:, 0] = 6.0
    pos = [(y, x) for y in range(0, 66, 2) for x in range(0, 64, 2)][:count]
    for y, x in pos:
        o1[0, 0, y, x], o1[0, 1, y, x] = 0.0, 6.0
    o2 = torch.zeros(1, 16, 66, 64)
    o2[:, 0::2] = 6.0
    return o1.to(dev), o2.to(dev)


def test_component_cap(dev):
    """Exactly 1024 components work; one more raises instead of truncating."""
    from gssd import _lib
    from pixel_link import postprocess
    o1, o2 = _isolated_pixels(dev, 1024)
    det, ndet = postprocess.mask_to_box_device(o1, o2, img_shape=(256, 264))
    host = postprocess.mask_to_box(o1, o2, img_shape=(256, 264))
    assert len(host[0]) == 1024
    assert_matches(det[:, 1].cpu().numpy(), ndet.cpu().numpy(), [([d[1:] for d in host[0]], [d[0] for d in host[0]])], 'cap')
    o1, o2 = _isolated_pixels(dev, 1025)
    with pytest.raises(_lib.GssdError, match='1025'):
        postprocess.mask_to_box_device(o1, o2, img_shape=(256, 264))
    with pytest.raises(_lib.GssdError):
        postprocess.mask_to_box_device(o1.cpu(), o2.cpu())


class _Images:
    name = 'lesion_test_ap_synth'

    def __init__(self, annos):
        self.annos = annos

    def __len__(self):
        return len(self.annos)

    def pull_image(self, i):
        return np.zeros((4, R.EVAL_IMAGE, R.EVAL_IMAGE, 3), np.uint8)

    def pull_anno(self, i):
        return self.annos[i]


def test_test_net_pixel_link_vs_oracle(dev):
    """test_net(use_pixel_link=True) over two batches of registry maps (a stub network hands them out) equals the evaluation oracle fed
    with the HOST mask_to_box detections, the ground truth of the image without any detection removed (make_pred :107-108); the image
    whose only detection scores below thresh keeps its ground truth."""
    from pixel_link import evaluate as T
    from gssd import _lib
    from oracle import eval_oracle as EO
    from pixel_link import postprocess
    batches = [(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)) for a, b in R.eval_batches()]
    host = [img for o1, o2 in batches
            for img in postprocess.mask_to_box(o1, o2, img_shape=(R.EVAL_SIZE, R.EVAL_SIZE), pixel_thres=R.EVAL_THRESH)]
    assert [len(d) > 0 for d in host] == [True, True, True, True, False] and max(d[0] for d in host[3]) < R.EVAL_THRESH
    annos = R.eval_annotations(host)
    k = max(len(d) for d in host)
    det = np.zeros((len(host), 2, k, 5), np.float32)
    for i, d in enumerate(host):
        if d:
            det[i, 1, :len(d)] = np.asarray(d, np.float32)
    gts = [a[:, :-1] * R.EVAL_SIZE / R.EVAL_IMAGE if len(d) else np.zeros((0, 4)) for a, d in zip(annos, host)]

    class Net:
        calls = 0

        def __call__(self, x):
            o1, o2 = batches[self.calls]
            self.calls += 1
            assert tuple(x.shape) == (o1.shape[0], 12, R.EVAL_SIZE, R.EVAL_SIZE) and x.is_cuda and not torch.is_grad_enabled()
            return o1, o2
    transform = lambda im: (np.zeros((4, R.EVAL_SIZE, R.EVAL_SIZE, 3), np.float32),)
    for use07 in (True, False):
        net = Net()
        ap, iobb = T.test_net(net, True, _Images(annos), transform, R.EVAL_SIZE, thresh=R.EVAL_THRESH, mode='v2', use_07_metric=use07,
                              ap_list=list(R.EVAL_AP), iobb_list=list(R.EVAL_IOBB), use_pixel_link=True, batch_size=R.EVAL_BATCH)
        assert net.calls == 2
        ref_ap, ref_iobb = EO.evaluate(det, np.ones((len(host), 4), np.float32), gts, R.EVAL_THRESH, R.EVAL_AP, R.EVAL_IOBB, use07)
        print('use_07', use07, 'ap', ap, 'iobb', iobb, 'oracle', ref_ap, ref_iobb)
        assert any(0.0 < v < 1.0 for v in ref_ap + ref_iobb)
        if use07:
            assert ap == list(ref_ap) and iobb == list(ref_iobb)
        else:
            assert np.allclose(ap, ref_ap, rtol=1e-13, atol=0) and np.allclose(iobb, ref_iobb, rtol=1e-13, atol=0)
    # counting the empty image's ground truth would have given something else
    full = [a[:, :-1] * R.EVAL_SIZE / R.EVAL_IMAGE for a in annos]
    assert EO.evaluate(det, np.ones((len(host), 4), np.float32), full, R.EVAL_THRESH, R.EVAL_AP, R.EVAL_IOBB, True) != (list(ref_ap), list(ref_iobb))
    with pytest.raises(_lib.GssdError):
        T.test_net(Net(), True, _Images(annos), transform, R.EVAL_SIZE, use_pixel_link=True, visualize=True, output_path='.', model_name='m')


def test_test_net_pixel_link_real_network(dev):
    """A real PixelLink "4s" (synthetic weights, eval mode), 3 images in batches of 2, mode v1.  The area metric: the 11-point rule adds
    eleven times p / 11 like the reference, which is 1.0000000000000002 for a perfect ranking -- and the synthetic network's one big component
    does cover the box at IoU / IoBB 0.1."""
    from pixel_link import evaluate as T
    from data import BaseTransform
    from gssd import synth
    from test_pixellink_cpu import PLAIN, build
    net = build(PLAIN).to(dev).eval()

    class Set(_Images):
        def pull_image(self, i):
            return synth.synth_study_u8(40 + i, 4, 128)
    annos = [np.array([[20., 30., 60., 80., 0.]] * 4)] * 3
    ap, iobb = T.test_net(net, True, Set(annos), BaseTransform(300, (49., 49., 49.), use_normalize=True), 300, thresh=0.05, mode='v1',
                          use_07_metric=False, ap_list=[0.1, 0.5], iobb_list=[0.1, 0.5], use_pixel_link=True, batch_size=2)
    print('real network', ap, iobb)
    assert len(ap) == 2 and len(iobb) == 2 and all(0. <= v <= 1. for v in ap + iobb)
