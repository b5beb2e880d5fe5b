"""CPU tier: the training token-type entry point of the C ABI (include/parq_hip.h parq_set_train_token_type) without a GPU — declared,
exported and typed, its argument checks, and the rule it sets: parq_forward_train / parq_backward run when the handle's token type
equals its training token type and refuse (with the message of the fp32-only days) otherwise."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _handle():
    from parq_amd import _lib
    cfg = _lib.ParqConfig(256, 64, 10, 4, 768, 8, 1, 10, (C.c_float * 6)(-3, 3, -2, 0.5, 0.25, 5.25))
    h = C.c_void_p()
    assert _lib.load().parq_create(C.byref(cfg), C.byref(h)) == 0
    return h


def _calls(lib, h):
    """(return code, message) of parq_forward_train and parq_backward on an unpacked handle with dummy pointers."""
    from parq_amd import _lib
    sc = _lib.ParqScene(1, 2, 4, 4, 1, 1, 1, 1, 1)
    po = _lib.ParqOutputs(1, 1, 1, 1, 1, 1)
    pg = _lib.ParqOutputGrads(1, 1, 1, 1)
    fwd = lib.parq_forward_train(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), None)
    fmsg = lib.parq_last_error()
    bwd = lib.parq_backward(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), C.byref(pg), C.c_void_p(1), None, None)
    return (fwd, fmsg), (bwd, lib.parq_last_error())


def test_set_train_token_type_is_declared_exported_and_typed():
    from parq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    assert re.search(r"int parq_set_train_token_type\(parq_handle h, int32_t type\);", hdr)
    res, args = _lib.SYMBOLS["parq_set_train_token_type"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int32]
    assert _lib.load().parq_set_train_token_type is not None
    assert len(_lib.SYMBOLS) == 71
    assert "71 entry points" in open(os.path.join(ROOT, "README.md")).read()


def test_set_train_token_type_accepts_the_three_types_and_rejects_others():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        for t in (1, 2, 0):
            assert lib.parq_set_train_token_type(h, t) == 0, t
        for bad in (3, -1):
            assert lib.parq_set_train_token_type(h, bad) == 1, bad
            assert b"token type" in lib.parq_last_error()
        assert lib.parq_set_train_token_type(None, 1) == 1
    finally:
        assert lib.parq_destroy(h) == 0


def test_training_runs_when_both_types_agree():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        for t in (2, 1, 0):
            assert lib.parq_set_token_type(h, t) == 0 and lib.parq_set_train_token_type(h, t) == 0
            (fwd, fmsg), (bwd, bmsg) = _calls(lib, h)
            # past the token check: the call order is checked next ("parq_pack_weights must be called first")
            assert fwd == 3 and b"parq_pack_weights" in fmsg, (t, fwd, fmsg)
            assert bwd == 3 and b"parq_pack_weights" in bmsg, (t, bwd, bmsg)
    finally:
        assert lib.parq_destroy(h) == 0


def test_training_refuses_when_the_types_differ():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        for tok, train in ((0, 2), (2, 0), (1, 2), (2, 1), (0, 1)):
            assert lib.parq_set_token_type(h, tok) == 0 and lib.parq_set_train_token_type(h, train) == 0
            (fwd, fmsg), (bwd, bmsg) = _calls(lib, h)
            assert fwd == 1 and b"fp32 tokens" in fmsg, (tok, train, fwd, fmsg)
            assert bwd == 1 and b"fp32 tokens" in bmsg, (tok, train, bwd, bmsg)
    finally:
        assert lib.parq_destroy(h) == 0


def test_view_sharding_keeps_refusing_16_bit_tokens():
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        sc = _lib.ParqScene(1, 2, 4, 4, 1, 1, 1, 1, 1)
        po = _lib.ParqOutputs(1, 1, 1, 1, 1, 1)
        assert lib.parq_set_token_type(h, 2) == 0 and lib.parq_set_train_token_type(h, 2) == 0
        assert lib.parq_iterate_sharded(h, C.byref(sc), C.c_void_p(1), 16, 0, 0, None, C.byref(po), None, None,
                                        C.c_void_p(1), 1, None) == 1
        assert b"fp32 tokens" in lib.parq_last_error()
    finally:
        assert lib.parq_destroy(h) == 0


def test_the_training_workspace_follows_the_token_type():
    """Attention mode 0 (fp32) carves the widened copy of 16-bit tokens (B*N*C floats); the cache modes carve nothing for them."""
    from parq_amd import _lib
    lib = _lib.load()
    h = _handle()
    try:
        B, V, hh, ww = 2, 3, 8, 8
        sizes = {}
        for mode in (0, 1):
            assert lib.parq_set_attention_mode(h, mode) == 0
            for t in (0, 1, 2):
                assert lib.parq_set_token_type(h, t) == 0 and lib.parq_set_train_token_type(h, t) == 0
                sizes[mode, t] = lib.parq_train_workspace_bytes(h, B, V, hh, ww)
        copy = B * V * hh * ww * 256 * 4
        assert sizes[0, 1] == sizes[0, 2] and copy <= sizes[0, 1] - sizes[0, 0] <= copy + 1024, sizes
        assert sizes[1, 0] == sizes[1, 1] == sizes[1, 2] > 0, sizes
    finally:
        assert lib.parq_destroy(h) == 0
