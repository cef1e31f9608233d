"""bench.py's plain run on the GPU: exactly `--steps` timed steps, the headline fields only, and `--dump-outputs`
writing what the timed (graph-replayed) step computed -- the same in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--scenes", "2", "--views", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {p.stem: np.load(p) for p in out_dir.glob("*.npy")}


def test_plain_run_times_exactly_steps_and_dumps_outputs(hip_lib, tmp_path):
    out, got = _plain_run(tmp_path / "a")
    assert out["steps"] == 4 and out["timing"]["trials"] == 1 and len(out["trials_ms"]) == 1
    assert out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "Mpixels/s" and out["dtype"] == "f32"
    assert out["higher_is_better"] is True and out["config"]["launch"] == "hip-graph replay"
    assert not {"roofline", "cpu_baseline", "secondary", "stage_ms_per_step_warmup"} & set(out)
    names = {"loss", "color"} | {f"grad_{n}" for n in ("means", "scales", "rotations", "opacities", "harmonics",
                                                        "extrinsics")}
    assert set(got) == names and all(a.dtype == np.float32 for a in got.values())
    assert got["color"].shape == (2, 2, 3, 256, 256) and got["grad_extrinsics"].shape == (2, 2, 4, 4)
    assert all(np.isfinite(a).all() for a in got.values()) and float(got["loss"]) > 0
    assert float(np.abs(got["grad_means"]).max()) > 0
    # the same inputs again: the same outputs, up to the order of the backward's float atomics
    _, again = _plain_run(tmp_path / "b")
    for n in names:
        err = float(np.abs(again[n].astype(np.float64) - got[n]).max())
        assert err <= 1e-4 * float(np.abs(got[n]).max()) + 1e-12, (n, err)
