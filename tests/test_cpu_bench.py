"""bench.py's --dump-outputs writer on host tensors shaped like a StackProcessor result: float32 / float64 files,
the size budget, seeded samples that are the same from call to call, and the rows they were taken from."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _result(m, n_assays, c=4, L=100, seed=0):
    rng = np.random.default_rng(seed)
    assay = np.sort(rng.integers(0, n_assays, m))
    table = np.zeros((m, 6 + 2 * c))
    table[:, 0] = assay
    table[:, 1:] = rng.integers(0, 4096, (m, 5 + 2 * c))
    out = {"roi": torch.from_numpy(rng.integers(0, 65536, (m, c, 1, L, L)).astype(np.uint16)),
           "fg": torch.from_numpy(rng.integers(0, 2, (m, L, L)).astype(np.uint8)),
           "bg": torch.from_numpy(rng.integers(0, 2, (m, L, L)).astype(np.uint8))}
    return out, torch.from_numpy(table)


def _load(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


def test_dump_outputs_budget_samples_and_determinism(tmp_path, monkeypatch):
    out, table = _result(300, 5)
    bench.dump_outputs(str(tmp_path / "a"), out, table, 6)
    a = _load(tmp_path / "a")
    assert sorted(a) == ["bg_sample", "fg_sample", "marker_table", "marker_table_index", "markers_per_assay",
                         "roi_sample", "roi_sample_index"]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in a) < 64 << 20
    np.testing.assert_array_equal(a["marker_table"], table.numpy())  # the whole table fits
    np.testing.assert_array_equal(a["markers_per_assay"], np.bincount(table[:, 0].numpy().astype(int), minlength=6))
    idx = a["roi_sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_MARKERS and len(set(idx)) == len(idx) and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(a["roi_sample"], out["roi"].numpy()[idx].astype(np.float32))
    np.testing.assert_array_equal(a["fg_sample"], out["fg"].numpy()[idx])
    np.testing.assert_array_equal(a["bg_sample"], out["bg"].numpy()[idx])

    bench.dump_outputs(str(tmp_path / "b"), out, table, 6)
    b = _load(tmp_path / "b")
    assert all(np.array_equal(a[n], b[n]) for n in a)

    # a table larger than its budget: a seeded sample of its rows, listed by index
    monkeypatch.setattr(bench, "DUMP_TABLE_BYTES", 100 * (8 * table.shape[1] + 8))
    bench.dump_outputs(str(tmp_path / "c"), out, table, 6)
    c = _load(tmp_path / "c")
    rows = c["marker_table_index"].astype(np.int64)
    assert len(rows) == 100 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(c["marker_table"], table.numpy()[rows])
    np.testing.assert_array_equal(c["markers_per_assay"], a["markers_per_assay"])


def test_dump_outputs_without_markers(tmp_path):
    out, table = _result(0, 3)
    bench.dump_outputs(str(tmp_path), out, table, 3)
    d = _load(tmp_path)
    assert d["marker_table"].shape == (0, 14) and d["markers_per_assay"].tolist() == [0, 0, 0]
    assert d["roi_sample"].shape == (0, 4, 1, 100, 100) and d["roi_sample_index"].shape == (0,)
