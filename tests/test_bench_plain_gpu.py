"""GPU: what a plain `bench.py --gpus 1` run measures and what `--full` adds.  A plain run is the headline alone (set-up,
warm-up, the timed steps, --dump-outputs, the line); `--full` measures the rest after it, in the same process, so the
headline's steps and what they hand back are the same in both.  Narrow width: the point is the line, not the figure."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--gpus', '1', '--steps', '6', '--warmup', '2', '--n-hidden', '256', '--timing-every', '2']
FULL_ONLY = ('f32_mfma', 'f16x3_split', 'module_path', 'launch_floor', 'cpu_baseline')


def _bench(extra, dump):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + ARGS + ['--dump-outputs', dump] + extra,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.strip().split('\n') if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _bench([], str(tmp_path / 'plain'))
    assert plain['metric'] == 'epochs/sec' and plain['unit'] == 'epochs/s' and plain['higher_is_better'] is True
    assert plain['steps'] == 6 and plain['warmup'] == 2 and plain['ms_per_step'] > 0 and plain['value'] > 0
    assert plain['roofline']['frac'] > 0 and plain['roofline_spmm']['achieved'] > 0
    assert not [k for k in FULL_ONLY if k in plain] and 'unplanted_graph' not in plain
    assert 'peak_measured_copy' not in plain['roofline_spmm']
    full = _bench(['--full', '--no-unplanted-leg', '--cpu-steps', '2', '--cpu-budget', '20'], str(tmp_path / 'full'))
    assert all(k in full for k in FULL_ONLY) and 'unplanted_graph' not in full
    assert full['f32_mfma']['value'] > 0 and full['module_path']['value'] > 0 and full['cpu_baseline']['value'] > 0
    assert full['launch_floor']['launches_per_step'] > 0 and full['roofline_spmm']['peak_measured_copy'] > 0
    # the headline comes first: its steps, loss and updated parameters do not depend on --full
    assert (plain['loss_first'], plain['loss_last']) == (full['loss_first'], full['loss_last'])
    assert plain['dumped_outputs']['arrays'] == full['dumped_outputs']['arrays']
    for name in plain['dumped_outputs']['arrays']:
        a, b = np.load(str(tmp_path / 'plain' / (name + '.npy'))), np.load(str(tmp_path / 'full' / (name + '.npy')))
        assert np.array_equal(a, b), name
