"""CPU tier: the deterministic-mode entry points (include/parq_hip.h parq_set_deterministic, parq_ray_pe_backward_flags,
parq_set_loss_flags) are declared, exported and typed; their setters check arguments; the training workspace grows, never shrinks."""
import ctypes as C
import os
import re

import pytest

from parq_amd import _lib, synth

ROOT = os.path.join(os.path.dirname(__file__), "..")
NEW = ("parq_set_deterministic", "parq_ray_pe_backward_workspace_bytes_flags", "parq_ray_pe_backward_flags",
       "parq_set_loss_scratch_bytes", "parq_set_loss_flags")


def _header():
    with open(os.path.join(ROOT, "include", "parq_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("name", NEW)
def test_declared_and_typed(name):
    assert re.search(r"\b%s\(" % name, _header()), name
    assert name in _lib.SYMBOLS
    assert getattr(_lib.load(), name) is not None


def test_flag_values_in_header():
    h = _header()
    assert re.search(r"PARQ_RAYPE_BWD_DETERMINISTIC = 1\b", h)
    assert re.search(r"PARQ_SETLOSS_DETERMINISTIC = 1\b", h)


def _handle(dim=256, heads=4):
    lib = _lib.load()
    cfg = synth.decoder_cfg(dim=dim, queries=64, heads=heads, ffn=512, layers=4)
    pc = _lib.ParqConfig(dim, 64, cfg.NUM_SEMCLS + 1, heads, 512, 4, 1, 10, (C.c_float * 6)(*cfg.TRANSFORMER.SCALE))
    h = C.c_void_p()
    _lib.check(lib.parq_create(C.byref(pc), C.byref(h)), "parq_create")
    return lib, h


def test_setter_checks_arguments():
    lib, h = _handle()
    try:
        assert lib.parq_set_deterministic(None, 1) == 1                    # PARQ_ERR_ARG
        assert lib.parq_set_deterministic(h, 2) == 1
        assert lib.parq_set_deterministic(h, -1) == 1
        assert lib.parq_set_deterministic(h, 1) == 0
        assert lib.parq_set_deterministic(h, 0) == 0
    finally:
        lib.parq_destroy(h)


@pytest.mark.parametrize("geo", [(2, 10, 60, 80), (1, 3, 8, 10)])
def test_training_workspace_grows_in_deterministic_mode(geo):
    lib, h = _handle()
    try:
        base = lib.parq_train_workspace_bytes(h, *geo)
        assert lib.parq_set_deterministic(h, 1) == 0
        det = lib.parq_train_workspace_bytes(h, *geo)
        assert lib.parq_set_deterministic(h, 0) == 0
        assert lib.parq_train_workspace_bytes(h, *geo) == base               # switching back restores the default carve
        assert det >= base > 0
    finally:
        lib.parq_destroy(h)


def test_flagged_sizes():
    lib = _lib.load()
    plain = lib.parq_ray_pe_backward_workspace_bytes(2, 3, 8, 10, 256, 64)
    assert lib.parq_ray_pe_backward_workspace_bytes_flags(2, 3, 8, 10, 256, 64, 0) == plain
    assert lib.parq_ray_pe_backward_workspace_bytes_flags(2, 3, 8, 10, 256, 64, 1) > plain
    assert lib.parq_ray_pe_backward_workspace_bytes_flags(2, 3, 8, 10, 256, 64, 2) == 0          # unknown bit
    assert lib.parq_set_loss_scratch_bytes(3, 2, 64, 10, 0) == 3 * 2 * 64 * 4
    assert lib.parq_set_loss_scratch_bytes(3, 2, 64, 10, 1) > 3 * 2 * 64 * 4
    assert lib.parq_set_loss_scratch_bytes(3, 2, 64, 10, 4) == 0


def test_flagged_entry_points_reject_unknown_flags():
    lib = _lib.load()
    one = C.c_void_p(16)                                   # never dereferenced: the flags are checked first
    f6 = (C.c_float * 6)(*[0.0] * 6)
    rc = lib.parq_ray_pe_backward_flags(one, one, one, one, one, f6, 0.25, 5.25, 64, 1, 1, 8, 10, 256, one, one, one, 1 << 30,
                                        one, one, one, one, None, 2, None)
    assert rc == 1
    w4 = (C.c_float * 4)(1, 1, 1, 1)
    rc = lib.parq_set_loss_flags(one, one, one, one, 1, 1, 8, 4, one, one, one, one, None, 2, None, None, 0, one, one, w4, one, one,
                                 one, one, one, one, 8, None)
    assert rc == 1
