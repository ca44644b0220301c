"""``bench.py`` as the driver runs it: a plain run prints the headline line alone, and ``--dump-outputs``
writes what the timed forward computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_prints_the_headline_and_dumps_the_timed_output(dev, tmp_path):
    """8 x 48^2, 2 timed steps: the line carries the headline fields and none of ``--full``'s, and
    DIR/output.npy is, bit for bit, the forward of the same model on the same seeded inputs."""
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "8", "--size", "48", "--settle-s", "0", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "galaxies/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert "48x48" in rec["metric"] and rec["ms_per_step"] > 0
    # value = the galaxies of the timed steps / their wall time
    assert rec["value"] == pytest.approx(8 * 2 / (2 * rec["ms_per_step"] * 1e-3), rel=1e-9)
    for k in ("blocks", "kernels", "roofline", "graphed", "ingest", "end_to_end", "cpu_baseline", "configs1", "configs4"):
        assert k not in rec, k
    assert sorted(os.listdir(out)) == ["output.npy"]
    got = np.load(out / "output.npy")
    assert got.dtype == np.float32 and got.shape == (8, 1, 48, 48)

    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    from gdeconv.synth import make_batch
    obs, psf, alpha, _ = make_batch(8, 48, seed=20250307, device=dev)
    model = bench.build_model(8, "Gaussian", dev)
    model.Z = torch.nn.Identity()
    with torch.no_grad():
        want = model(obs, psf, alpha).cpu().numpy()
    assert np.array_equal(got, want)
