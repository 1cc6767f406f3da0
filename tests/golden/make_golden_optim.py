"""Golden vectors for gssd.optim: what the library's OWN optimizer kernels leave, bit for bit, at the commit the fixture names -- the
yardstick of a change that must not move a result (the kernels are documented as bitwise reproducible).  The cases are
tests/optim_golden_common.py: three steps of SGD / Adam / AdamW / LARS / LAMB in every variant over nine param groups,
clip_grad_norm_, AveragedModel and one grad_stats table.  Per case: ``<case>|full`` (the bytes of norms, trust ratios, tables and small
tensors, end to end) and ``<case>|sha`` (the SHA-256 of every larger tensor).  Needs the MI355X; nothing but this library runs on it.

    python tests/golden/make_golden_optim.py --commit $(git rev-parse HEAD)      # rewrites tests/golden/optim_steps.npz
    python tests/golden/make_golden_optim.py --check                             # replays and compares with the file
    (--out PATH writes elsewhere)
"""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'grouped-ssd-pytorch_amd'))
import optim_golden_common as K               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--commit', default=None, help='the commit of the tree that runs (default: git rev-parse HEAD)')
    ap.add_argument('--out', default=os.path.join(HERE, 'optim_steps.npz'))
    ap.add_argument('--check', action='store_true')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.check:
        old = np.load(a.out, allow_pickle=False)
        for name in K.CASES:
            K.compare(name, K.run_case(name, dev), old[name + '|full'], old[name + '|sha'])
        print(f'{a.out}: same contents (recorded at {old["commit"]})')
        return
    commit = a.commit or subprocess.run(['git', 'rev-parse', 'HEAD'], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    out = dict(commit=np.array(commit), device=np.array(torch.cuda.get_device_name(0)))
    for name in K.CASES:
        entries = K.run_case(name, dev)
        out[name + '|full'], out[name + '|sha'] = K.pack(name, entries)
        print(f'{name}: {len(entries)} entries, {out[name + "|full"].size} bytes in full, {len(out[name + "|sha"])} digests')
    np.savez_compressed(a.out, **out)
    print('wrote', a.out, os.path.getsize(a.out), 'bytes, commit', commit)


if __name__ == '__main__':
    main()
