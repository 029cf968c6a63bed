"""bench.py on one GPU: a plain run prints the headline line only and, with
--dump-outputs, writes what its last timed step left; those arrays equal a
direct render of the same steps bit for bit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(native, tmp_path):
    steps, warmup, F = 2, 1, 2
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup), "--frames-per-step", str(F), "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["full"] is False
    assert out["unit"] == "Mpaths/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    # value is the paths of the timed steps over their wall time
    assert abs(out["value"] - out["config"]["paths_per_step"] / out["ms_per_step"] / 1e3) <= 2e-3 * out["value"]
    # nothing of the --full measurements ran
    for key in ("roofline", "interactive", "strong", "verify", "cpu_baseline"):
        assert key not in out
    assert out["build"]["matches_sources"]

    from vrenderer_pathtracer_amd import VRendererHIP, scenes
    sc = scenes.make_scene("C2")
    r = VRendererHIP(0)
    scenes.load_into(r, sc)
    for i in range(warmup + steps):
        r.render(frames=F, times=[sc["time"] + i * F + k for k in range(F)])
    want = {"accum": r.read_accum(), "rgba8": r.read_rgba8(), "depth8": r.read_depth8()}
    r.cleanUp()
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in want)
    total = 0
    for name, a in want.items():
        got = np.load(os.path.join(tmp_path, name + ".npy"))
        total += got.nbytes
        assert got.dtype == np.float32 and got.shape == (sc["width"] * sc["height"], 4)
        assert np.array_equal(got.view(np.uint32), a.reshape(-1, 4).astype(np.float32).view(np.uint32)), name
    assert total <= 64 * 1000 * 1000 and total == out["outputs"]["bytes"]
