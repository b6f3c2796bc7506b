"""The plain `bench.py --gpus 1 --steps K --warmup W` run: headline only, K timed steps, and with --dump-outputs the last timed step's
outputs as float arrays that a second run with the same arguments reproduces (what two builds are compared by)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = dict(os.environ)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_PORT', 'MDX_BENCH_BACKEND'):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1', '--batch', '16',
                        '--dump-outputs', str(out_dir)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_run_reports_the_headline_and_dumps_reproducible_outputs(tmp_path):
    import bench
    line = _plain_run(tmp_path / 'a')
    assert line['steps'] == 4 and line['warmup'] == 1 and line['n_gpus'] == 1
    assert line['ms_per_step'] > 0 and line['higher_is_better'] is True and line['unit'] == 'molecules/sec'
    assert line['value'] == pytest.approx(16 / (line['ms_per_step'] * 1000 / 1e3), rel=1e-5)
    for k in ('configs', 'cpu_baseline', 'roofline_edge_b', 'segment_sum', 'gather_ms', 'sample_wall_s'):
        assert k not in line, k                                                  # --full only
    _, ph, _ = bench.build_workload(16, 0, None)
    N, Eh = int(ph['batch_node'].numel()), int(ph['batch_halfedge'].numel())
    shapes = {'pred_node': (N, 8), 'pred_pos': (N, 3), 'pred_halfedge': (Eh, 6), 'h_node': (N, 8), 'pos': (N, 3),
              'h_halfedge': (Eh, 6), 'log_node': (N, 8), 'log_halfedge': (Eh, 6)}
    assert sorted(os.listdir(tmp_path / 'a')) == sorted(k + '.npy' for k in shapes)
    a = {k: np.load(tmp_path / 'a' / (k + '.npy')) for k in shapes}
    for k, shp in shapes.items():
        assert a[k].dtype == np.float32 and a[k].shape == shp, (k, a[k].dtype, a[k].shape)
        assert np.isfinite(a[k]).all() or k.startswith('log_'), k
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert (a['h_node'].sum(-1) == 1).all() and (a['h_halfedge'].sum(-1) == 1).all()
    _plain_run(tmp_path / 'b')
    for k in shapes:
        assert np.array_equal(a[k], np.load(tmp_path / 'b' / (k + '.npy')), equal_nan=True), k
