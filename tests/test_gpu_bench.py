"""GPU: bench.py's plain run prints the headline line only, times exactly --steps steps, and --dump-outputs writes the embeddings
of the timed path (checked against the CPU oracle on the bench's own seeded frames and weights), at a tiny geometry."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import vit as ovit
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump_outputs(tmp_path):
    name, frames = "ViT-tiny/14", 8
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", name, "--frames", str(frames),
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["dtype"] == "bf16" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["unit"] == "frame-embeddings/s"
    assert not {"roofline", "secondary_rooflines", "clock_probe", "cpu_baseline", "parity", "f16_same_workload", "student_train",
                "extras", "tfam_forward"} & set(line), "the measurements of --full ran in a plain run"

    y = np.load(tmp_path / "embeddings.npy")
    assert y.dtype == np.float32 and y.shape == (frames, synth.VIT_GEOMETRY[name][5])
    R, H = synth.VIT_GEOMETRY[name][0], synth.VIT_GEOMETRY[name][4]
    ref = ovit.vit_forward(synth.vit_state_dict(name, 2), ovit.normalize_u8(synth.randint_u8(1, "frames", (frames, 3, R, R))), H).numpy()
    err = float(np.abs(y - ref).max())
    assert err <= 8e-3 * max(1.0, float(np.abs(ref).max())), f"dumped embeddings differ from the oracle by {err}"
