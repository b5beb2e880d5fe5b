"""CPU tier: the float64 truth the GPU attention-map tests compare against (tests/attn_map_util.py) IS the tensor the reference
computes and drops — ``F.multi_head_attention_forward(..., need_weights=True)`` (model/transformer_parq.py:377-380;
oracle/parq_oracle.py:176-179 restates the call) on the same inputs, in float64, to 1e-12 — and the new entry points are bound."""
import pytest
import torch
import torch.nn.functional as F

from parq_amd import _lib
from attn_map_util import Truth, build, decode_one_term_cache, k_bf16, k_fp16, k_split, k_stage8


@pytest.mark.parametrize("name,share", [("a", True), ("b", True), ("c", True), ("b", False)])
def test_truth_helper_is_the_reference_ops_attention_weights(name, share):
    cfg, W, sc = build(name, share_weights=share)
    tr = Truth(cfg, W, sc)
    H = cfg.TRANSFORMER.DEC_HEADS
    for k in (0, 2):
        in_w, in_b = tr.in_proj(k)
        q_in, mem = tr.query_input(k), tr.od.tokens
        C = q_in.shape[-1]
        for avg in (True, False):
            _, want = F.multi_head_attention_forward(
                q_in.transpose(0, 1), mem.transpose(0, 1), mem.transpose(0, 1), C, H, in_w, in_b, None, None, False, 0.0,
                torch.eye(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), training=False, need_weights=True,
                average_attn_weights=avg)
            got = tr.maps(k).mean(1) if avg else tr.maps(k)
            assert want.dtype == torch.float64 and got.shape == want.shape
            assert float((got - want).abs().max()) < 1e-12, (k, avg)
        assert float((tr.maps(k).sum(-1) - 1).abs().max()) < 1e-12


def test_cache_forms_round_keys_as_the_formats_do():
    k = torch.tensor([[[1.0 + 2.0 ** -12 + 2.0 ** -20, -3.1415926535, 1e-3, 0.0]]], dtype=torch.float64)
    k32 = k.float().double()
    assert float((k_split(k) - k32).abs().max()) <= 2.0 ** -21 * 4          # 22 significant bits
    assert float((k_stage8(k) - k32).abs().max()) <= 2.0 ** -14 * 4         # hi16 + a 4-bit residual
    assert float((k_stage8(k) - k32).abs().max()) > 0
    assert torch.equal(k_fp16(k), k.half().double()) and torch.equal(k_bf16(k), k.bfloat16().double())


def test_one_term_cache_decode_inverts_the_documented_layout():
    """Written element by element in the order csrc/kv_layout.hpp documents for a [K | V] block; ragged N, two heads."""
    Bn, H, N = 1, 2, 70
    K = torch.randn(Bn, H, N, 64, generator=torch.Generator().manual_seed(3)).bfloat16()
    nblk = (N + 31) // 32
    raw = torch.zeros(Bn, H, nblk, 4096, dtype=torch.bfloat16)
    for n in range(N):
        blk, key = divmod(n, 32)
        for c in range(8):
            kh, s = c >> 2, c & 3
            pos = c ^ ((key >> 1) & 7)
            for e in range(8):
                d = 32 * (s >> 1) + 16 * (s & 1) + 4 * kh + (e & 3) + 8 * (e >> 2)
                raw[:, :, blk, key * 64 + pos * 8 + e] = K[:, :, n, d]
    got = decode_one_term_cache(raw.view(-1).view(torch.float32), Bn, H, N, "bf16")
    assert torch.equal(got, K.double())


def test_entry_points_are_declared():
    assert "parq_attention_map" in _lib.SYMBOLS and "parq_attention_map_scratch_bytes" in _lib.SYMBOLS
    from parq_amd.decoder import PARQDecoder
    assert callable(PARQDecoder.cross_attention_map) and callable(PARQDecoder.cross_attention_view_mass)
