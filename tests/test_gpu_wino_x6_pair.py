"""The paired form of csrc/conv_wino_x6.hip (one workgroup = 64 tiles x two adjacent 64-channel output blocks: the input transform once for
both) against the unpaired form on the same descriptors.  GSSD_WINO_X6_PAIR is read once per process, hence one worker process per switch
value (tests/wino_x6_pair_worker.py), started one after the other, each under its own timeout; a failed worker fails every test without a
further start.

* raw outputs: bit-identical (per output element the products, the chunk order and the fold order are the unpaired form's);
* against a float64 convolution: the measure and the gates of tests/test_gpu_wino_x6.py -- e < 2e-5 and e <= 1.5 e_fp32 + 1e-7 with e_fp32 the
  fp32-MFMA Winograd kernel's error on the same inputs (GSSD_WINO_X6=0, a third worker);
* batch sums (regrouped: a workgroup owns other items, a lane adds the sums of its tile pair): each channel's sum and sum of squares against
  a float64 sum over the kernel's own output, relative to the float64 sum of the magnitudes; paired <= 2 x unpaired on the same case;
* three blocks per group and bf16 planes run the unpaired kernel under either switch value and match as well.

Shapes: the smallest at which the paired code takes another path (see the worker)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from wino_x6_pair_worker import CASES          # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}


def run_worker(mode, pair):
    key = (mode, pair)
    if key not in _cache:
        if any(v is None for v in _cache.values()):
            pytest.fail('an earlier worker failed: no further GPU process is started')
        _cache[key] = None
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'wino_x6_pair_worker.py')], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, GSSD_WINO_X6=mode, GSSD_WINO_X6_PAIR=pair))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('WINOX6PAIRJSON ')][-1]
        res = json.loads(line[len('WINOX6PAIRJSON '):])
        assert res['mode'] == mode and res['pair'] == pair
        _cache[key] = res
    if _cache[key] is None:
        pytest.fail('this worker failed before')
    return _cache[key]


@pytest.mark.parametrize('ci', range(len(CASES)), ids=['x'.join(str(v) for v in c[:6]) + ('' if c[6] else '-bf16') for c in CASES])
def test_wino_x6_paired_matches_unpaired_and_float64(ci):
    paired, unpaired, fp32 = run_worker('2', '1')['results'][ci], run_worker('2', '0')['results'][ci], run_worker('0', '1')['results'][ci]
    case = paired['case']
    assert case == unpaired['case'] == fp32['case'] == list(CASES[ci])
    assert set(paired['forms']) == set(unpaired['forms']) == {'plain', 'sums_rep1', 'sums_rep8', 'xf_select', 'xf_select_sums', 'xf_address',
                                                             'xf_address_sums'}
    for name, fp in paired['forms'].items():
        fu, f3 = unpaired['forms'][name], fp32['forms'][name]
        line = f'{case} {name}: paired {fp["err"]:.2e} unpaired {fu["err"]:.2e} fp32 kernel {f3["err"]:.2e}'
        if 'sum_err' in fp:
            line += f' | batch sums paired {fp["sum_err"][0]:.2e} {fp["sum_err"][1]:.2e} unpaired {fu["sum_err"][0]:.2e} {fu["sum_err"][1]:.2e}'
        print(line)
        assert fp['takes'] == 1 and fu['takes'] == 1 and f3['takes'] == 0, line
        assert fp['sha'] == fu['sha'], line                                       # raw output: the same bits
        assert fp['err'] < 2e-5 and f3['err'] < 2e-5, line
        assert fp['err'] <= 1.5 * f3['err'] + 1e-7, line
        if 'sum_err' in fp:
            for k in range(2):
                assert fp['sum_err'][k] <= 2 * fu['sum_err'][k], line
    # the two padding paths of the fused producer transform: the same bits
    assert paired['forms']['xf_select']['sha'] == paired['forms']['xf_address']['sha']
    assert paired['forms']['plain']['sha'] == paired['forms']['sums_rep1']['sha'] == paired['forms']['sums_rep8']['sha']
