"""bench.py's plain run on the GPU: the headline only (no extra legs, no detail file), exactly --steps timed steps, and --dump-outputs writes
what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_step_outputs(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--batch', '4',
                        '--dump-outputs', str(out), '--detail', str(tmp_path / 'detail.json')], capture_output=True, text=True, timeout=600)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-3000:]
    ln = lines[0]
    assert ln['steps'] == 3 and ln['warmup'] == 1 and ln['full'] is False and ln['dtype'] == 'f32' and ln['higher_is_better'] is True
    assert ln['ms_per_step'] > 0 and ln['value'] > 0 and ln['unit'] == 'img/s'
    assert ln['cpu_baseline'] is None and ln['full_step'] is None and ln['roofline'] is None and ln['detail'] is None
    assert not (tmp_path / 'detail.json').exists()
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ['conf', 'loc', 'loss_c', 'loss_l', 'priors']
    assert got['loc'].shape == (4, 8732, 4) and got['conf'].shape == (4, 8732, 2) and got['priors'].shape == (8732, 4)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in got.values())
    assert got['loss_l'].size == got['loss_c'].size == 1
    assert np.allclose([got['loss_l'].item(), got['loss_c'].item()], ln['loss'], rtol=1e-4, atol=1e-5)
