"""The oracle's attention (oracle/parq_oracle.py mha, reference_ops=False) against torch's own nn.MultiheadAttention arithmetic
(F.multi_head_attention_forward, the function nn.MultiheadAttention.forward calls) in float64, at every head dim the library
takes (32, 64, 128, 256): outputs and autograd gradients of the in / out projection weights and biases and of the inputs.

The golden vectors of oracle/make_golden.py are all at head dims 64 and 256; the float64 bounds of the GPU tests at head dims 32
and 128 (tests/test_gpu_head_dims.py) rest on this restatement, so it is pinned here first.  The call patterns are the decoder's:
self-attention with query is key and a separate value (transformer_parq.py:372-376), cross-attention with key is value, and three
separate inputs."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import parq_oracle as O

TOL = 1e-12


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _torch_mha(q, k, v, in_w, in_b, out_w, out_b, H):
    o, _ = F.multi_head_attention_forward(q.transpose(0, 1), k.transpose(0, 1), v.transpose(0, 1), q.shape[-1], H, in_w, in_b,
                                          None, None, False, 0.0, out_w, out_b, training=False, need_weights=True)
    return o.transpose(0, 1)


@pytest.mark.parametrize("pattern", ["self", "cross", "separate"])
@pytest.mark.parametrize("B,Lq,Lk,H,dh", [
    (2, 7, 61, 8, 32),       # ragged lengths, 8 heads of 32 (dim 256)
    (1, 300, 300, 4, 32),    # more than 256 keys, dim 128
    (3, 1, 5, 2, 32),        # one query, B = 3
    (3, 40, 160, 2, 64),
    (2, 7, 61, 2, 128),
    (1, 300, 300, 2, 128),
    (2, 33, 97, 1, 256),
    (1, 300, 300, 4, 256),   # the reference's shipped width (dim 1024)
])
def test_oracle_mha_matches_torch_multihead_attention_float64(B, Lq, Lk, H, dh, pattern):
    C = H * dh
    if pattern == "self":
        Lk = Lq
    g = torch.Generator().manual_seed(1000 * dh + 10 * Lq + Lk + B)
    rnd = lambda *s, std=1.0: (torch.randn(*s, generator=g, dtype=torch.float64) * std).requires_grad_(True)
    # weight scale such that the scores q.k / sqrt(dh) have a spread of a few units: softmax neither uniform nor one-hot
    in_w, in_b = rnd(3 * C, C, std=1.5 / math.sqrt(C)), rnd(3 * C, std=0.1)
    out_w, out_b = rnd(C, C, std=1.0 / math.sqrt(C)), rnd(C, std=0.1)
    xq, xk, xv = rnd(B, Lq, C), rnd(B, Lk, C), rnd(B, Lk, C)
    key = {"self": xq, "cross": xk, "separate": xk}[pattern]
    value = {"self": xv, "cross": xk, "separate": xv}[pattern]
    leaves = {"in_proj_weight": in_w, "in_proj_bias": in_b, "out_proj.weight": out_w, "out_proj.bias": out_b, "query": xq}
    leaves.update({"key": xk, "value": xv} if pattern == "separate" else {"key": xk} if pattern == "cross" else {"value": xv})
    cot = torch.randn(B, Lq, C, generator=g, dtype=torch.float64)

    def run(fn):
        out = fn(xq, key, value, in_w, in_b, out_w, out_b, H)
        grads = torch.autograd.grad((out * cot).sum(), list(leaves.values()))
        return out.detach(), dict(zip(leaves, grads))

    got, got_g = run(O.mha)
    want, want_g = run(_torch_mha)
    assert got.shape == want.shape == (B, Lq, C)
    errs = {"output": _rel(got, want)}
    errs.update({name: _rel(got_g[name], want_g[name]) for name in leaves})
    # (one key: the probabilities are 1 whatever the query, so the query's gradient is exactly 0 there)
    assert all(float(want_g[n].abs().max()) > 0 for n in leaves if not (n == "query" and Lk == 1))
    assert max(errs.values()) < TOL, errs
