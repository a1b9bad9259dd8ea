"""CPU: bench.py --dump-outputs writes every uint64 residue array as two exact float64 halves, under its size limit, with a fixed sample of
coefficient positions when the output is larger (the same positions in every run)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeCt:
    def __init__(self, a, level, scale):
        self.a, self.level, self.Scale = a, level, scale

    def download(self):
        return self.a

    def Level(self):
        return self.level


def load_u64(d, name):
    lo, hi = np.load(os.path.join(d, name + "_lo32.npy")), np.load(os.path.join(d, name + "_hi32.npy"))
    assert lo.dtype == hi.dtype == np.float64
    return (hi.astype(np.uint64) << np.uint64(32)) + lo.astype(np.uint64)


def test_dump_is_exact_below_the_limit(tmp_path):
    rng = np.random.default_rng(3)
    a = rng.integers(0, (1 << 61) - 1, (3, 4, 1024), dtype=np.uint64)
    b = rng.integers(0, (1 << 61) - 1, (3, 4, 1024), dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), [("ct0", FakeCt(a, 3, 2.0 ** 40)), ("ct1", FakeCt(b, 3, 2.0 ** 40))])
    assert (load_u64(tmp_path, "ct0") == a).all() and (load_u64(tmp_path, "ct1") == b).all()
    assert np.load(tmp_path / "ct0_level.npy").tolist() == [3.0] and np.load(tmp_path / "ct1_scale.npy").tolist() == [2.0 ** 40]
    assert not (tmp_path / "coeff_index.npy").exists()


def test_dump_samples_fixed_positions_above_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    a = np.random.default_rng(4).integers(0, (1 << 61) - 1, (2, 3, 4096), dtype=np.uint64)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), [("ct", FakeCt(a, 2, 1.0))])
    idx = np.load(tmp_path / "x" / "coeff_index.npy")
    assert (idx == np.load(tmp_path / "y" / "coeff_index.npy")).all()
    got = load_u64(tmp_path / "x", "ct")
    assert got.shape == (2, 3, len(idx)) and (got == a[..., idx.astype(np.int64)]).all()
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x") if f.startswith("ct_") and "32" in f) <= (1 << 16) + 512
