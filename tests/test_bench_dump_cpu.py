"""bench.py --dump-outputs: the last step's arrays as <name>.npy in float32 / float64, within the 64 MB budget (a fixed seeded
sample of rows past it, the same rows in every array), integers exact as float64."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _step_outputs(n, dim, k=5, seed=0):
    g = torch.Generator().manual_seed(seed)
    desc = torch.randn((n, dim), generator=g)
    rows = torch.randint(0, 100_000, (n, k), generator=g)
    sims = torch.randn((n, k), generator=g, dtype=torch.float64)
    cnt = torch.full((n,), k, dtype=torch.int32)
    return desc, (rows, sims, cnt)


def test_dump_writes_every_array_in_float32_or_float64(tmp_path):
    b = _bench()
    desc, match = _step_outputs(64, 128)
    b.dump_outputs(str(tmp_path), desc, match)
    assert sorted(os.listdir(tmp_path)) == ["descriptors.npy", "topk_count.npy", "topk_rows.npy", "topk_sims.npy"]
    got = {n[:-4]: np.load(tmp_path / n) for n in os.listdir(tmp_path)}
    assert got["descriptors"].dtype == np.float32 and np.array_equal(got["descriptors"], desc.numpy())
    assert got["topk_rows"].dtype == np.float64 and np.array_equal(got["topk_rows"], match[0].numpy().astype(np.float64))
    assert got["topk_sims"].dtype == np.float64 and np.array_equal(got["topk_sims"], match[1].numpy())
    assert got["topk_count"].dtype == np.float64 and np.array_equal(got["topk_count"], match[2].numpy())


def test_dump_past_the_budget_is_a_fixed_sample_of_the_same_rows(tmp_path):
    b = _bench()
    desc, match = _step_outputs(600, 4096)
    b.DUMP_BUDGET_BYTES = 4 << 20                   # 9.8 MB of outputs against a 4 MB budget
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), desc, match)
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a"))
    assert total <= 4 << 20
    rows = np.load(tmp_path / "a" / "descriptors_sample_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 600 and np.all(np.diff(rows) > 0)
    for name, ref in (("descriptors", desc.numpy()), ("topk_rows", match[0].numpy()), ("topk_sims", match[1].numpy())):
        assert np.array_equal(np.load(tmp_path / "a" / (name + "_sample_rows.npy")), rows)
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), ref[rows])
    for n in os.listdir(tmp_path / "a"):                   # same inputs, same files
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
