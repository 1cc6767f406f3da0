"""gssd.optim against its own recorded results, bit for bit (tests/golden/optim_steps.npz, written by tests/golden/make_golden_optim.py
at the commit the fixture names): the optimizer kernels are bitwise reproducible, so a change to the optimizer core that is not meant to
move a result must leave every byte of every case of tests/optim_golden_common.py where it was.  There is no tolerance anywhere."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_common import *                      # noqa: E402,F401,F403  (fixture dev)
import optim_golden_common as K               # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'optim_steps.npz'), allow_pickle=False)


def test_fixture_lists_the_cases():
    g = golden()
    assert sorted(g.files) == sorted(['commit', 'device'] + [f'{c}|{k}' for c in K.CASES for k in ('full', 'sha')])
    assert len(str(g['commit'])) == 40


@pytest.mark.parametrize('case', K.CASES)
def test_same_bytes_as_recorded(dev, case):
    g = golden()
    K.compare(case, K.run_case(case, dev), g[case + '|full'], g[case + '|sha'])
