"""bench.py --dump-outputs (host side): float32 / float64 files named after the outputs, the 64 MB cap, and a fixed sample of a
tensor that does not fit, drawn the same way in every run."""
import os

import numpy as np
import torch

import bench


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_dtypes_and_names(tmp_path):
    bench.dump_outputs(str(tmp_path), {"it0_coord_pos": torch.arange(6, dtype=torch.float32).reshape(2, 3),
                                       "loss": torch.tensor(1.5, dtype=torch.float64), "ids": torch.arange(4),
                                       "param_a/b": torch.ones(3, dtype=torch.float16)})
    a = np.load(tmp_path / "it0_coord_pos.npy")
    assert a.dtype == np.float32 and a.shape == (2, 3) and np.array_equal(a, np.arange(6).reshape(2, 3))
    assert np.load(tmp_path / "loss.npy").dtype == np.float64
    assert np.load(tmp_path / "ids.npy").dtype == np.float32
    assert np.load(tmp_path / "param_a_b.npy").dtype == np.float32


def test_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path):
    small = torch.full((1000,), 2.0)
    big = torch.arange(20 << 20, dtype=torch.float32)                    # 80 MB alone
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), {"small": small, "big": big})
        assert _total_bytes(tmp_path / sub) <= bench.DUMP_LIMIT_BYTES
        assert np.array_equal(np.load(tmp_path / sub / "small.npy"), small.numpy())
        idx = np.load(tmp_path / sub / "big.sample_index.npy")
        val = np.load(tmp_path / sub / "big.sample.npy")
        assert len(idx) > 0 and np.array_equal(val, big.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "big.sample_index.npy"), np.load(tmp_path / "b" / "big.sample_index.npy"))


def test_full_is_an_option_that_is_off_by_default():
    """A plain `bench.py --gpus 1 --steps N --warmup W` measures the headline figure only; everything else waits for --full."""
    ap = bench.build_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert plain.full is False and plain.steps == 5 and plain.warmup == 2 and plain.dump_outputs is None
    assert ap.parse_args(["--full"]).full is True
    assert ap.parse_args(["--train", "--full", "--no-cpu-baseline", "--no-b32", "--no-peaked", "--no-pmc"]).full is True
