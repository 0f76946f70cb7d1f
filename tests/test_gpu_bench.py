"""`python bench.py --gpus 1` as the driver runs it: a plain run times exactly --steps steps and prints the headline
fields only (what takes runs of its own is behind --full), and `--dump-outputs DIR` writes the products of the last
timed step as float32 .npy files within 64 MB."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_with_dumped_outputs(tmp_path):
    out = str(tmp_path / "outputs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["kernels"] and all(len(k) for k in line["kernels"].values())
    for key in ("variants", "edge_dropped_step", "graph_construction", "model_steps", "cpu_baseline", "probes_GBps"):
        assert key not in line, key  # --full only
    files = sorted(glob.glob(os.path.join(out, "*.npy")))
    assert len(files) == len(line["kernels"]) == 8
    assert sum(os.path.getsize(f) for f in files) <= 64 << 20
    y = {os.path.basename(f)[:-4]: np.load(f) for f in files}
    for name, a in y.items():
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 128, (name, a.dtype, a.shape)
        assert np.isfinite(a).all() and np.abs(a).max() > 0, name
    # the step's forward and backward GCMC launches include two identical products (same graph, table and scalings)
    for a, b in (("gcmc_fwd_drug_to_disease", "gcmc_bwd_disease_to_drug"), ("gcmc_fwd_disease_to_drug", "gcmc_bwd_drug_to_disease")):
        np.testing.assert_allclose(y[a], y[b], rtol=1e-5, atol=1e-5 * float(np.abs(y[a]).max()))
