"""GPU tier: deterministic mode against the float64 oracle, and the configurations it does not cover.

The oracle comparisons of test_gpu_backward.py — every shape of test_backward_matches_oracle_autograd (head dims 64, 128 and 256,
d up to 1024, unshared layers, ragged key and query counts, views smaller than one gather tile) with its bounds, and the ray-PE
backward with its bounds — run again under torch.use_deterministic_algorithms(True), i.e. through the fixed-order forms."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import test_gpu_backward as base  # noqa: E402
from parq_amd import synth  # noqa: E402
from gpu_util import make_decoder, scene_args  # noqa: E402

pytestmark = pytest.mark.gpu

_SHAPES = next(m for m in base.test_backward_matches_oracle_autograd.pytestmark if m.name == "parametrize").args


@pytest.fixture
def deterministic():
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


@pytest.mark.parametrize(*_SHAPES)
def test_deterministic_backward_matches_oracle_autograd(deterministic, B, V, h, w, Q, heads, dim, ffn, layers, shared):
    base.test_backward_matches_oracle_autograd(B, V, h, w, Q, heads, dim, ffn, layers, shared)


def test_deterministic_ray_pe_backward_matches_oracle_autograd(deterministic, monkeypatch):
    base.test_ray_pe_backward_matches_oracle_autograd(monkeypatch)


def _dh32():
    cfg = synth.decoder_cfg(dim=256, queries=32, heads=8, ffn=128, layers=2)        # head dim 32
    return make_decoder(cfg, synth.make_decoder_weights(cfg, 5)), synth.make_scene(6, 1, 2, 8, 10, 256)


def test_head_dim_32_inference_runs_in_deterministic_mode(deterministic):
    dec, sc = _dh32()
    with torch.no_grad():
        a = dec.eval()(*scene_args(sc))
        b = dec(*scene_args(sc))
    torch.cuda.synchronize()
    assert all(torch.equal(x[k], y[k]) for x, y in zip(a, b) for k in x)


def test_head_dim_32_training_refuses_in_deterministic_mode(deterministic):
    dec, sc = _dh32()
    with pytest.raises(RuntimeError, match="head dim 32"):
        dec.train().forward_train(*scene_args(sc))
    torch.use_deterministic_algorithms(True, warn_only=True)
    with pytest.warns(UserWarning, match="head dim 32"):
        dec.forward_train(*scene_args(sc))
    torch.cuda.synchronize()
