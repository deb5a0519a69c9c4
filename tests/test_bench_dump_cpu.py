"""``bench.py --dump-outputs DIR``: the output dict of the last timed step written as DIR/<name>.npy -- float32, at most 64 MB in all,
views that another dumped array already holds left out, a larger output as a fixed sample of its elements, the same files from run to run."""
import glob
import os

import numpy as np
import torch


def test_sample_indices_are_distinct_sorted_in_range_and_fixed():
    import bench
    for n, k in ((10, 10), (10, 3), (1000003, 1000), (81_100_800, 200_000), (7, 0)):
        idx = bench.dump_sample_indices(n, k).numpy()
        assert idx.shape == (k,) and idx.dtype == np.int64
        assert np.all(np.diff(idx) > 0) and (k == 0 or (idx[0] >= 0 and idx[-1] < n))      # sorted, hence distinct; in range
        assert np.array_equal(idx, bench.dump_sample_indices(n, k).numpy())
    assert np.array_equal(bench.dump_sample_indices(10, 10).numpy(), np.arange(10))            # k = n: every element
    big = bench.dump_sample_indices(81_100_800, 200_000).numpy()
    assert np.histogram(big, bins=16, range=(0, 81_100_800))[0].min() > 200_000 / 16 * 0.9   # spread over the whole array


def test_dump_outputs_budget_views_sample_and_repeatability(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    preds = torch.randn(8, 72, 100, 352, generator=g)               # 81 MB: over the budget, so everything is sampled
    single = torch.randn(8, 20, 100, 352, generator=g)
    out = {"cls_preds": preds[:, :8], "reg_preds": preds[:, 8:64], "dir_preds": preds[:, 64:], "preds_tensor": preds,
           "cls_preds_single": single[:, :2], "reg_preds_single": single[:, 2:16], "dir_preds_single": single[:, 16:], "not_an_array": None}
    a, b = tmp_path / "a", tmp_path / "b"
    written = bench.dump_outputs(out, str(a))
    assert bench.dump_outputs(out, str(b)) == written
    assert written["cls_preds"] == written["reg_preds"] == written["dir_preds"] == "in preds_tensor.npy"
    files = sorted(os.path.basename(f) for f in glob.glob(str(a / "*.npy")))
    assert files == ["cls_preds_single.npy", "dir_preds_single.npy", "preds_tensor.npy", "reg_preds_single.npy"]
    assert sum(os.path.getsize(a / f) for f in files) <= 64e6
    for f in files:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype == np.float32 and np.array_equal(x, y), f
    for name, full in (("preds_tensor", preds), ("reg_preds_single", single[:, 2:16])):
        shape, k = written[name]
        flat = full.contiguous().reshape(-1).numpy()                  # C order of the (possibly strided) view
        assert shape == list(full.shape) and flat.size // 2 < k < flat.size
        assert np.array_equal(np.load(a / (name + ".npy")), flat[bench.dump_sample_indices(flat.size, k).numpy()])


def test_dump_outputs_small_arrays_whole_and_float64_kept(tmp_path):
    import bench
    x = torch.arange(24, dtype=torch.float64).view(2, 3, 4)
    y = torch.arange(6, dtype=torch.float32).view(2, 3).t()
    written = bench.dump_outputs({"x": x, "y": y}, str(tmp_path))
    assert written == {"x": [[2, 3, 4], 24], "y": [[3, 2], 6]}
    assert np.load(tmp_path / "x.npy").dtype == np.float64 and np.array_equal(np.load(tmp_path / "x.npy"), x.numpy())
    assert np.array_equal(np.load(tmp_path / "y.npy"), y.numpy())
