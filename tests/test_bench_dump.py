"""bench.dump_outputs without a GPU: a stand-in renderer of the 4K size, whose
images exceed the dump budget, is written as the same seeded sample twice."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


class _Images:
    width, height = 3840, 2160

    def __init__(self):
        n = self.width * self.height
        self.index = np.arange(n, dtype=np.float32)          # exact in float32 below 2^24

    def read_accum(self):
        return np.repeat(self.index, 4).reshape(self.height, self.width, 4)

    def read_rgba8(self):
        return (np.repeat(self.index, 4).reshape(self.height, self.width, 4) % 251).astype(np.uint8)

    read_depth8 = read_rgba8


def test_dump_outputs_samples_large_images_reproducibly(tmp_path):
    import bench
    r = _Images()
    a = bench.dump_outputs(r, str(tmp_path / "a"))
    b = bench.dump_outputs(r, str(tmp_path / "b"))
    assert a["pixels"] == b["pixels"] < a["of_pixels"] == r.width * r.height and a["sample"]
    total = 0
    for name in ("accum", "rgba8", "depth8"):
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == (a["pixels"], 4) and np.array_equal(x, y)
        total += x.nbytes
    assert total == a["bytes"] <= 64 * 1000 * 1000
    # the arrays hold the same pixels: accum carries each pixel's index
    idx = np.load(tmp_path / "a" / "accum.npy")[:, 0]
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rgba8.npy")[:, 0], idx.astype(np.int64) % 251)
