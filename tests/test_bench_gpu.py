"""GPU: bench.py --dump-outputs on one GPU -- the last timed pair's outputs, written twice by two runs with the same
arguments, are the same arrays bit for bit, and the dumped relative pose is the one its dumped track() fields give."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(gpu, tmp_path):
    argv = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
            "--no-roofline", "--no-exact-leg", "--no-other-legs"]
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        r = subprocess.run(argv + ["--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert '"ms_per_step"' in r.stdout.strip().splitlines()[-1]
        dumps.append({f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert sorted(a) == sorted(b) and {"pose_rel", "pose_composed", "flow_fwd", "depth", "kp_ref", "track_status"} <= set(a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 10 ** 6
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["flow_fwd"].shape == (2, 376, 1241) and a["kp_ref"].shape == a["kp_cur"].shape and len(a["kp_ref"]) > 100
    assert int(a["track_n_kp"][0]) == len(a["kp_ref"])
    if int(a["track_status"][0]) == 0:  # E-tracked: R and t * scale (df-vo_amd/pipeline.py hybrid_pose)
        assert np.array_equal(a["pose_rel"][:3, :3], a["track_R"].reshape(3, 3))
        assert np.array_equal(a["pose_rel"][:3, 3], a["track_t"] * a["track_scale"][0])
