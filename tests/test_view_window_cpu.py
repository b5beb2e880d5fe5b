"""CPU tier: the parts of the streaming view window (parq_amd.ViewWindow, include/parq_hip.h parq_forward_views) that need no GPU —
the module imports, the dirty-set -> merged runs -> widened row ranges function against hand-written expectations, the argument
checks, and the entry point's declaration and ctypes signature."""
import ctypes as C
import os
import re

import pytest
import torch

import parq_amd
from parq_amd import _lib, synth
from parq_amd.view_window import ViewWindow, check_put_args, check_window_args, row_ranges, slot_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_importable_without_a_gpu_and_reachable_from_the_package_and_the_decoder():
    from parq_amd.decoder import PARQDecoder
    from parq_amd.module import PARQ
    assert parq_amd.ViewWindow is ViewWindow
    assert callable(PARQDecoder.view_window) and callable(PARQ.view_window)
    for name in ("put", "rebase", "forward", "close", "tokens", "camera", "dirty_slots"):
        assert hasattr(ViewWindow, name), name


def test_slot_runs_merges_adjacent_slots():
    assert slot_runs([2]) == [(2, 2)]
    assert slot_runs([3, 0]) == [(0, 0), (3, 3)]
    assert slot_runs([2, 1]) == [(1, 2)]
    assert slot_runs([0, 1, 2, 3]) == [(0, 3)]
    assert slot_runs([]) == []


@pytest.mark.parametrize("slots,hw,tile,want", [
    # h*w = 64: a view is one 64-row tile, half a 128-row tile
    ([2], 64, 64, [(128, 192)]),
    ([2], 64, 128, [(128, 256)]),                    # widened into slot 3
    ([1], 64, 128, [(0, 128)]),                      # widened into slot 0
    ([0, 3], 64, 64, [(0, 64), (192, 256)]),
    ([0, 3], 64, 128, [(0, 256)]),                   # [0, 128) and [128, 256) touch after widening: one range
    ([1, 2], 64, 64, [(64, 192)]),
    ([1, 2], 64, 128, [(0, 256)]),
    # h*w = 100, N = 400: no view starts on a tile
    ([2], 100, 64, [(192, 320)]),
    ([2], 100, 128, [(128, 384)]),
    ([0, 3], 100, 64, [(0, 128), (256, 400)]),       # the clamp at N
    ([0, 3], 100, 128, [(0, 128), (256, 400)]),
    ([1, 2], 100, 64, [(64, 320)]),
    ([1, 2], 100, 128, [(0, 384)]),
    ([3], 100, 128, [(256, 400)]),
    ([0, 2], 100, 128, [(0, 384)]),                  # two runs that touch after widening merge: [0, 128) + [128, 384)
    # h*w = 256: whole tiles, nothing to widen
    ([2], 256, 64, [(512, 768)]),
    ([2], 256, 128, [(512, 768)]),
    ([0, 3], 256, 128, [(0, 256), (768, 1024)]),
    ([1, 2], 256, 64, [(256, 768)]),
    ([0, 1, 2, 3], 256, 128, [(0, 1024)]),
    ([], 256, 64, []),
])
def test_row_ranges_against_hand_written_expectations(slots, hw, tile, want):
    assert row_ranges(slots, 4, hw, tile) == want
    assert sum(b - a for a, b in want) <= 4 * hw


def test_row_ranges_32_key_blocks_of_the_large_dim_kernel():
    assert row_ranges([1], 3, 64, 32) == [(64, 128)]
    assert row_ranges([0, 2], 3, 100, 32) == [(0, 128), (192, 300)]
    with pytest.raises(ValueError):
        row_ranges([3], 3, 64, 32)


def test_window_argument_errors_are_value_errors_before_the_gpu():
    T = torch.zeros(2, 12)
    for bad in (dict(B=0), dict(V=0), dict(h=1), dict(w=True), dict(dtype=torch.float64), dict(dtype=torch.int32)):
        a = dict(B=2, V=4, h=8, w=8, C_=256, T_world_local=T, dtype=torch.float32)
        a.update(bad)
        with pytest.raises(ValueError):
            check_window_args(**a)
    with pytest.raises(ValueError, match="T_world_local must be"):
        check_window_args(2, 4, 8, 8, 256, torch.zeros(3, 12), torch.float32)
    with pytest.raises(ValueError, match="lives on the GPU"):
        check_window_args(2, 4, 8, 8, 256, T, torch.float32)                 # a CPU tensor
    cfg = synth.decoder_cfg(dim=256, queries=32, heads=4, ffn=768, layers=2)
    from parq_amd.decoder import PARQDecoder
    with pytest.raises(ValueError, match="lives on the GPU"):
        PARQDecoder(cfg).view_window(2, 4, 8, 8, T)


def test_put_argument_errors_are_value_errors_before_the_gpu():
    B, V, h, w, Cd = 2, 4, 8, 8, 256
    gpu = torch.device("cuda", 0)
    tok = lambda n, dtype=torch.float32: torch.zeros(B, n * h * w, Cd, dtype=dtype)
    tabs = lambda n: (torch.zeros(B, n, 6), torch.zeros(B, n, 12), torch.zeros(B, n, 12))
    ok = lambda slot, t, tb, dtype=torch.float32, device=torch.device("cpu"): check_put_args(B, V, h, w, Cd, dtype, device, slot, t, *tb)
    slots, cam, T_cp, T_wp = ok([1, 3], tok(2), tabs(2))                       # (the checks themselves pass on matching devices)
    assert slots == [1, 3] and cam.shape == (B, 2, 6)
    assert ok(2, tok(1).view(B, 1, h * w, Cd), tabs(1))[0] == [2]
    for slot in (4, -1, [0, 4], [1, 1], [], "1", 1.0, True):
        with pytest.raises(ValueError, match="slot"):
            ok(slot, tok(1), tabs(1))
    with pytest.raises(ValueError, match="dtype"):
        ok(1, tok(1, torch.float16), tabs(1))
    with pytest.raises(ValueError, match="dtype"):
        ok(1, tok(1), tabs(1), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="must be"):
        ok(1, tok(2), tabs(1))                                                  # two views of tokens for one slot
    with pytest.raises(ValueError, match="must be"):
        ok(1, torch.zeros(B, h * w, Cd + 1), tabs(1))
    with pytest.raises(ValueError, match="camera must be"):
        ok([0, 1], tok(2), tabs(1))
    with pytest.raises(ValueError, match="T_world_pseudoCam must be"):
        ok(1, tok(1), tabs(1)[:2] + (torch.zeros(B, 1, 9),))
    with pytest.raises(ValueError, match="CPU tensor"):
        ok(1, tok(1), tabs(1), device=gpu)                                      # CPU tensors into a window on the GPU


def test_header_declares_the_entry_point_and_the_binding_types_it():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    m = re.search(r"\bint\s+\(?parq_forward_views\)?\s*\(([^;]*)\)\s*;", hdr)
    assert m, "include/parq_hip.h must declare parq_forward_views"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["h", "graph", "scene", "workspace", "workspace_bytes", "outs", "views", "n_views",
                                                           "rows_projected", "stream"]
    assert "const int32_t *views" in m.group(1) and "int64_t *rows_projected" in m.group(1)
    res, args = _lib.EXTRA_SYMBOLS["parq_forward_views"]
    assert res is C.c_int and len(args) == len(params)
    assert args[6] == C.POINTER(C.c_int32) and args[7] is C.c_int32 and args[8] == C.POINTER(C.c_int64)
    assert "parq_forward_views" not in _lib.SYMBOLS


def test_library_exports_the_entry_point():
    assert _lib.load().parq_forward_views.argtypes == _lib.EXTRA_SYMBOLS["parq_forward_views"][1]
