"""bench.py's plain run on the GPU: the contract line, exactly --steps timed steps, no extra legs without --full, and the
outputs of the last timed step under --dump-outputs."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.gpu
def test_plain_run_dumps_outputs(tmp_path):
    d = tmp_path / "outputs"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "32",
                        "--seq-len", "20", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["unit"] == "sequences/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 2 and line["full"] is False
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(32 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    assert line["steady_state"] is None and line["roofline"] is None and line["cpu_baseline"] is None and "also" not in line
    files = {p.name: np.load(p) for p in d.iterdir()}
    assert {"loss.npy", "elbo_kf.npy", "elbo_vae_total.npy", "x_recon.npy", "grad_norm.npy"} <= set(files)
    assert any(n.startswith("param.") for n in files)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["x_recon.npy"].size == 32 * 20 * 32 * 32
    assert float(files["loss.npy"]) == pytest.approx(line["config"]["final_loss"], abs=1e-4)
