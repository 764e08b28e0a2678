"""GPU: bench.py's plain run and its --dump-outputs (what the last timed step handed its caller), and that --full adds the legs a plain run
leaves out.  Small graphs, fresh processes as the driver starts them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(dataset, *argv, cwd=None):
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--dataset', dataset] + list(argv),
                       capture_output=True, text=True, timeout=600, cwd=cwd)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-1000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_step_and_repeats_it(tmp_path):
    """The plain run, started from a directory it may not write to (a checkout owned by another user), writes nothing there."""
    a, b, ro = tmp_path / 'a', tmp_path / 'b', tmp_path / 'read_only'
    ro.mkdir()
    ro.chmod(0o555)
    try:
        d = _bench('S-cora', '--steps', '4', '--warmup', '1', '--dump-outputs', str(a), cwd=ro)
        assert os.listdir(ro) == []
    finally:
        ro.chmod(0o755)
    assert d['steps'] == 4 and d['ms_per_step'] > 0 and d['value'] == pytest.approx(1e3 / d['ms_per_step'])
    assert d['metric'] == 'teachergnn_fullgraph_train_steps_per_sec' and d['unit'] == 'steps/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    for leg in ('dense_backward', 'all_rows_forward', 'cpu_baseline', 'epochs_per_sec_reference_epoch'):
        assert leg not in d, leg
    files = sorted(os.listdir(a))
    assert 'loss.npy' in files and any(f.startswith('param.') for f in files) and any(f.startswith('grad.') for f in files), files
    arrays = {f: np.load(a / f) for f in files}
    assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
    assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
    assert arrays['loss.npy'][0] == np.float32(d['final_loss'])
    # same arguments, same inputs: a second process computes the same step
    _bench('S-cora', '--steps', '4', '--warmup', '1', '--dump-outputs', 'b', cwd=tmp_path)      # (a relative DIR: under the caller's directory)
    assert sorted(os.listdir(b)) == files
    for f in files:
        np.testing.assert_allclose(np.load(b / f), arrays[f], rtol=1e-5, atol=1e-6, err_msg=f)


def test_full_run_adds_the_other_legs():
    """S-arxiv: large enough for the row-sparse backward, so the dense-backward restart runs as well."""
    d = _bench('S-arxiv', '--steps', '3', '--warmup', '1', '--full', '--pmc-traffic', '0', '--cpu-baseline-mode', 'sample', '--cpu-sample-nodes', '20000')
    assert d['steps'] == 3 and d['ms_per_step'] > 0
    assert d['dense_backward']['steps'] == 3 and d['dense_backward']['ms_per_step'] > 0
    assert d['cpu_baseline']['value'] > 0 and d['epochs_per_sec_reference_epoch'] > 0
