"""CPU tests for bench.py's --dump-outputs writer: float32 .npy files, one per
returned array, with a fixed seeded sample for arrays above the size cap."""
import numpy as np
import torch

import bench
from magi_attention.common.forward_meta import AttnForwardMeta


def _last(n, seed):
    g = torch.Generator().manual_seed(seed)
    out = torch.randn(n, 4, 8, generator=g).bfloat16()
    lse = torch.randn(n, 4, generator=g)
    grads = [torch.randn(n, 4, 8, generator=g).bfloat16() for _ in range(3)]
    return (out, AttnForwardMeta(lse=lse), *grads)


def test_dump_outputs_small_arrays_whole(tmp_path):
    last = _last(16, 0)
    bench.dump_outputs(last, str(tmp_path / "d"), rank=0, world=1)
    names = sorted(p.name for p in (tmp_path / "d").iterdir())
    assert names == ["dk.npy", "dq.npy", "dv.npy", "lse.npy", "out.npy"]
    out = np.load(tmp_path / "d" / "out.npy")
    assert out.dtype == np.float32
    assert np.array_equal(out, last[0].float().reshape(-1).numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "lse.npy"),
                          last[1].lse.reshape(-1).numpy())
    assert np.array_equal(np.load(tmp_path / "d" / "dv.npy"),
                          last[4].float().reshape(-1).numpy())


def test_dump_outputs_large_arrays_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 256)
    a, b = _last(64, 1), _last(64, 1)
    bench.dump_outputs(a, str(tmp_path / "a"), rank=0, world=1)
    bench.dump_outputs(b, str(tmp_path / "b"), rank=1, world=2)
    for name in ("out", "lse", "dq", "dk", "dv"):
        x = np.load(tmp_path / "a" / f"{name}.npy")
        y = np.load(tmp_path / "b" / f"{name}_rank1.npy")
        # lse has exactly 256 elements (kept whole); the others are sampled
        assert x.shape == (256,) and x.dtype == np.float32
        assert np.array_equal(x, y)  # same inputs -> same sample
    full = a[0].float().reshape(-1).numpy()
    assert np.isin(np.load(tmp_path / "a" / "out.npy"), full).all()
