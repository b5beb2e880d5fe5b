"""Batch-invariant inference (include/parq_hip.h parq_set_batch_invariant), the part that needs no GPU: the entry point exists in the
header, the binding table and the built library, and the Python attribute is off by default and forwarded by PARQ."""
import ctypes as C
import os
import re
from types import SimpleNamespace as NS

from parq_amd import _lib, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_setter_and_the_built_library_exports_it():
    header = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    assert re.search(r"\bint\s+\(?parq_set_batch_invariant\)?\s*\(\s*parq_handle\s+h\s*,\s*int32_t\s+on\s*\)\s*;", header)
    assert _lib.EXTRA_SYMBOLS["parq_set_batch_invariant"] == (C.c_int, [C.c_void_p, C.c_int32])
    assert _lib.load().parq_set_batch_invariant is not None
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "parq_set_batch_invariant")
    lib.parq_set_batch_invariant.restype = C.c_int
    lib.parq_set_batch_invariant.argtypes = [C.c_void_p, C.c_int32]
    assert lib.parq_set_batch_invariant(None, 1) != 0, "a NULL handle is an error, not a crash"


def test_the_decoder_attribute_is_off_by_default():
    from parq_amd.decoder import PARQDecoder
    dec = PARQDecoder(synth.decoder_cfg(dim=256, queries=32, heads=4, ffn=256, layers=2))
    assert dec.batch_invariant is False
    assert dec._settings()[-1] is False
    dec.batch_invariant = True
    assert dec._settings()[-1] is True


def test_parq_forwards_the_attribute_to_its_decoder():
    from parq_amd import PARQ
    dcfg = synth.decoder_cfg(dim=256, queries=32, heads=4, ffn=256, layers=2)
    cfg = NS(MODEL=NS(TOKENIZER=NS(OUT_CHANNELS=256, RAY_POINTS_SCALE=dcfg.TRANSFORMER.SCALE, NUM_SAMPLES=64, MIN_DEPTH=0.25, MAX_DEPTH=5.25),
                      DECODER=dcfg))
    model = PARQ(cfg)
    assert model.batch_invariant is False and model.box3d_decoder.batch_invariant is False
    model.batch_invariant = True
    assert model.box3d_decoder.batch_invariant is True and model.batch_invariant is True
    model.box3d_decoder.batch_invariant = False
    assert model.batch_invariant is False
