"""bench.py's plain run on a small configuration (-m gpu): one JSON line with the headline fields, exactly --steps timed steps, and
--dump-outputs writing the last step's descriptors and top-k lists -- the top-k lists equal to the CPU oracle's on those descriptors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    from cslam_amd import synthetic
    from oracle import pyoracle
    rows, dim, batch, k = 4096, 4096, 256, 5
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--bank-rows", str(rows), "--batch", str(batch), "--extract-chunk", "128", "--extract-lanes", "2",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "keyframes/sec" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - batch / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    assert "roofline" not in d and "cpu_baseline" not in d and "c2_cosplace" not in d      # behind --full
    assert sorted(os.listdir(out)) == ["descriptors.npy", "topk_count.npy", "topk_rows.npy", "topk_sims.npy"]
    desc = np.load(out / "descriptors.npy")
    idx, sims, cnt = (np.load(out / (n + ".npy")) for n in ("topk_rows", "topk_sims", "topk_count"))
    assert desc.dtype == np.float32 and desc.shape == (batch, dim)
    assert np.allclose(np.linalg.norm(desc, axis=1), 1.0, atol=1e-4)
    assert idx.shape == (batch, k) and sims.shape == (batch, k) and cnt.shape == (batch,)
    bank = synthetic.bank(0, rows, dim)
    q = desc[:32]
    oi, os_, oc = pyoracle.nns_search(bank, q, k)
    assert np.array_equal(idx[:32], oi.astype(np.float64)) and np.array_equal(cnt[:32], oc.astype(np.float64))
    assert np.max(np.abs(sims[:32] - os_)) < 1e-12
