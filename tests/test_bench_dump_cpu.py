"""bench.py --dump-outputs without a GPU: what dump_outputs() writes for small and for large arrays."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_small_arrays_whole_and_large_ones_as_a_fixed_sample(tmp_path):
    big = torch.arange(bench.DUMP_ELEMENTS + 1000, dtype=torch.int32).to(torch.uint8)
    status = torch.tensor([0, -3, 7], dtype=torch.int32)
    u16 = torch.tensor([0, 1, 65535, 32768], dtype=torch.int32).to(torch.int16)         # uint16 pixels arrive as an int16 view
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"pixels": big, "status": status, "u16": u16})
    a, b = np.load(tmp_path / "a" / "pixels.npy"), np.load(tmp_path / "b" / "pixels.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_ELEMENTS,) and np.array_equal(a, b)
    idx = torch.randint(0, big.numel(), (bench.DUMP_ELEMENTS,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(a, big[idx].numpy().astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "status.npy"), np.array([0, -3, 7], np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "u16.npy"), np.array([0, 1, 65535, 32768], np.float32))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 << 20
