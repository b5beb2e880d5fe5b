"""CPU tier: the token-type entry point of the C ABI (include/parq_hip.h parq_set_token_type) without a GPU — declared, exported and
typed, and its argument checks, including the training / view-sharded entry points that read fp32 tokens only."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handle():
    from parq_amd import _lib
    cfg = _lib.ParqConfig(256, 64, 10, 4, 768, 8, 1, 10, (C.c_float * 6)(-3, 3, -2, 0.5, 0.25, 5.25))
    h = C.c_void_p()
    assert _lib.load().parq_create(C.byref(cfg), C.byref(h)) == 0
    return h


def test_set_token_type_is_declared_exported_and_typed():
    from parq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    assert re.search(r"int parq_set_token_type\(parq_handle h, int32_t type\);", hdr)
    assert re.search(r"PARQ_TOKENS_F32 = 0, PARQ_TOKENS_F16 = 1, PARQ_TOKENS_BF16 = 2", hdr)
    res, args = _lib.SYMBOLS["parq_set_token_type"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32]
    assert _lib.load().parq_set_token_type is not None


def test_set_token_type_accepts_the_three_types_and_rejects_others():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        for t in (1, 2, 0):
            assert lib.parq_set_token_type(h, t) == 0, t
        for bad in (3, -1, 16):
            assert lib.parq_set_token_type(h, bad) == 1, bad
            assert b"token type" in lib.parq_last_error()
        assert lib.parq_set_token_type(None, 1) == 1
    finally:
        assert lib.parq_destroy(h) == 0


def test_training_and_sharded_entry_points_refuse_16_bit_tokens():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        sc = _lib.ParqScene(1, 2, 4, 4, 1, 1, 1, 1, 1)
        po = _lib.ParqOutputs(1, 1, 1, 1, 1, 1)
        pg = _lib.ParqOutputGrads(1, 1, 1, 1)
        assert lib.parq_set_token_type(h, 2) == 0
        assert lib.parq_forward_train(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), None) == 1
        assert b"fp32 tokens" in lib.parq_last_error()
        assert lib.parq_backward(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), C.byref(pg), C.c_void_p(1), None, None) == 1
        assert lib.parq_iterate_sharded(h, C.byref(sc), C.c_void_p(1), 16, 0, 0, None, C.byref(po), None, None,
                                        C.c_void_p(1), 1, None) == 1
        # the inference entry points take the type; call order is checked as before
        assert lib.parq_forward(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), None) == 3
        assert lib.parq_set_token_type(h, 0) == 0
        assert lib.parq_forward_train(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), None) == 3     # back to "pack first"
    finally:
        assert lib.parq_destroy(h) == 0


def test_decoder_token_type_map():
    from parq_amd.decoder import TOKEN_TYPES
    assert TOKEN_TYPES == {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def test_ray_pe_16_bit_output_is_an_inference_channels_last_flag():
    """parq_ray_pe's fp16 / bf16 token output (flags 8 / 16) needs the no-hidden flag (2), refuses the NCHW layout (1) and both types
    at once — checked before anything is enqueued."""
    from parq_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    scale = (C.c_float * 6)(-3, 3, -2, 0.5, 0.25, 5.25)
    for flags in (8, 16, 8 | 16 | 2, 8 | 1 | 2, 16 | 1 | 2):
        rc = lib.parq_ray_pe(p, p, p, p, p, p, p, p, scale, 0.25, 5.25, 64, 1, 1, 4, 4, 256, p, p, flags, p, 1 << 30, None)
        assert rc == 1, flags
        assert b"16-bit" in lib.parq_last_error()
