"""Shared by tests/test_attention_map_cpu.py and tests/test_gpu_attention_map.py: the float64 truth of the cross-attention map

    P[b,h,q,n] = softmax_n( q_h[b,q] . k_h[b,n] / sqrt(dh) ),      map = mean_h P

built from the oracle's intermediates of an iteration (``x1 + pos`` is the query input of the layer's cross-attention,
oracle/parq_oracle.py OracleDecoder.layer), the tokens and the cross-attention in-projection, and the row-relative metric."""
import math

import torch
import torch.nn.functional as F

from parq_amd import synth
from oracle import parq_oracle as O
from emulate_attention_arithmetic import _e4, _h, _rtz16

# name -> (dim, heads, Q, V, h, w): B = 2 throughout
SHAPES = {
    "a": (256, 4, 40, 2, 8, 8),        # N = 128: whole 64-key stages, the mode-4 layout applies
    "b": (256, 4, 19, 3, 5, 7),        # N = 105, ragged Q and N: "split8" runs as "split"
    "c": (128, 4, 16, 3, 5, 7),        # head dim 32
    "d": (1024, 4, 16, 2, 4, 8),       # head dim 256
}
B = 2


def build(name, seed=300, share_weights=True, wq_scale=1.0, layers=3):
    dim, heads, Q, V, h, w = SHAPES[name]
    cfg = synth.decoder_cfg(dim=dim, queries=Q, heads=heads, ffn=64 if dim > 256 else 96, layers=layers, share_weights=share_weights)
    W = synth.make_decoder_weights(cfg, seed)
    if wq_scale != 1.0:                  # sharpened rows: the query rows of the cross-attention in-projection (bench.py peaked_workload)
        for li in range(1 if share_weights else layers):
            key = "parq_module.decoder.layers.%d.multihead_attn.in_proj_weight" % li
            wq = W[key].copy()
            wq[:dim] *= wq_scale
            W[key] = wq
    sc = synth.make_scene(seed + 1, B, V, h, w, dim, smooth=True)
    return cfg, W, sc


def per_head_map(q_in, tokens, in_w, in_b, H, k_transform=None, k_project=None):
    """float64 (B, H, Q, N) probabilities.  k_transform(k, head) -> k: replaces a head's (B, N, dh) keys (what a cache holds of them);
    k_project(tokens, Wk, bk) -> (B, N, C): replaces the K projection itself (the one-term modes round its operands too)."""
    Bn, L, C = q_in.shape
    S = tokens.shape[1]
    dh = C // H
    q = F.linear(q_in, in_w[:C], in_b[:C]).view(Bn, L, H, dh).transpose(1, 2)
    k = F.linear(tokens, in_w[C:2 * C], in_b[C:2 * C]) if k_project is None else k_project(tokens, in_w[C:2 * C], in_b[C:2 * C])
    k = k.view(Bn, S, H, dh).transpose(1, 2)
    if k_transform is not None:
        k = torch.stack([k_transform(k[:, hd], hd) for hd in range(H)], dim=1)
    return torch.softmax((q @ k.transpose(-1, -2)) / math.sqrt(dh), dim=-1)


class Truth:
    """The float64 oracle of a scene, free-running: refs[k] are the reference points iteration k starts from, and
    ``maps(k)`` the per-head cross-attention probabilities of iteration k (computed once, kept)."""

    def __init__(self, cfg, W, sc, iters=3, refs=None):
        self.cfg, self.H = cfg, cfg.TRANSFORMER.DEC_HEADS
        self.od = O.OracleDecoder(cfg, W, synth.SCANNET_MEAN_SIZES, dtype=torch.float64)
        self.od.prepare(sc["tokens"], sc["camera"], sc["T_camera_pseudoCam"], sc["T_world_pseudoCam"], sc["T_world_local"])
        self.refs, self.inter = [], []
        with torch.no_grad():
            ref = self.od.initial_ref()
            for k in range(iters):
                if refs is not None:
                    ref = torch.as_tensor(refs[k]).double()
                self.refs.append(ref)
                _, ref, inter = self.od.iterate(ref, k)
                self.inter.append(inter)
        self._maps = {}

    def in_proj(self, k):
        li = 0 if self.cfg.TRANSFORMER.SHARE_WEIGHTS else k
        p = "parq_module.decoder.layers.%d.multihead_attn." % li
        return self.od.W[p + "in_proj_weight"], self.od.W[p + "in_proj_bias"]

    def query_input(self, k):
        return self.inter[k]["x1"] + self.inter[k]["pos"]

    def maps(self, k, k_transform=None, k_project=None):
        if k_transform is not None or k_project is not None:
            return per_head_map(self.query_input(k), self.od.tokens, *self.in_proj(k), self.H, k_transform, k_project)
        if k not in self._maps:
            self._maps[k] = per_head_map(self.query_input(k), self.od.tokens, *self.in_proj(k), self.H)
        return self._maps[k]


def row_rel(p, ref):
    """max over rows of  max_n |p - p*| / max_n p*  (rows = all leading dims; no element excluded)."""
    ref = torch.as_tensor(ref).double().cpu()
    p = torch.as_tensor(p).double().cpu().reshape(ref.shape)       # (.., V, h, w) -> (.., N)
    return float(((p - ref).abs().amax(-1) / ref.amax(-1)).max())


# ---- what a K cache holds of a float64 key (the device's keys come out of an fp32-class projection: start from the fp32 value)
def k_split(k, _head=None):             # split layout: hi (toward zero) + fp16 lo
    k = k.float().double()
    hi = _rtz16(k)
    return hi + _rtz16(k - hi)


def k_stage8(k, _head=None):            # mode-4 stage: hi16 + e4m3 of the residual scaled by 2^10
    k = k.float().double()
    hi = _rtz16(k)
    return hi + _e4(k - hi, 1024.0)


def k_fp16(k, _head=None):
    return _h(k)


def k_bf16(k, _head=None):
    return k.float().bfloat16().double()


def k_one_term(kind):
    """The cache of the one-term modes "fp16" / "bf16": the K projection is ONE 16-bit product — tokens and weights rounded to nearest,
    fp32 accumulation, fp32 bias — and its result is rounded to nearest once more (kvproj_split.hip, TERMS = 1)."""
    r = k_fp16 if kind == "fp16" else k_bf16

    def project(tokens, w, b):
        acc = (r(tokens) @ r(w).t()).float()
        return r((acc + b.float()).double())
    return project


def one_term_sum_slack(kind, tokens, w, b):
    """How far two fp32 evaluations of the one-term projection's sum can be apart (any summation order): 2 (n + 1) 2^-24 sum |x| |w|."""
    r = k_fp16 if kind == "fp16" else k_bf16
    n = tokens.shape[-1]
    return 2 * (n + 1) * 2.0 ** -24 * (r(tokens).abs() @ r(w).abs().t() + b.abs())


def k_tiers(safe_mask):
    return lambda k, head: k_split(k) if (safe_mask >> head) & 1 else k_stage8(k)


def decode_one_term_cache(raw, Bn, heads, N, kind):
    """K of the one-term ("fp16" / "bf16") cache as the device holds it: (B, heads, N, 64) float64 from the raw workspace buffer
    "kv_cache16" of a handle with shared layers and head dim 64.  Layout (csrc/kv_layout.hpp, restated here independently): per (scene, head) 32-key blocks
    of 8 KB [K | V]; K = [32 keys][8 chunk positions][8 elements], chunk c = 4 kh + s sits at position c ^ ((key >> 1) & 7) and holds
    d = 32 (s >> 1) + 16 (s & 1) + 4 kh + (e & 3) + 8 (e >> 2)."""
    nblk = (N + 31) // 32
    bits = raw.detach().cpu().contiguous().view(torch.int16)[: Bn * heads * nblk * 4096].view(Bn, heads, nblk, 4096)[..., :2048]
    idx = torch.empty(32, 8, 8, dtype=torch.int64)
    for key in range(32):
        for pos in range(8):
            c = pos ^ ((key >> 1) & 7)
            kh, s_ = c >> 2, c & 3
            for e in range(8):
                idx[key, pos, e] = 32 * (s_ >> 1) + 16 * (s_ & 1) + 4 * kh + (e & 3) + 8 * (e >> 2)
    vals = bits.contiguous().view(torch.float16 if kind == "fp16" else torch.bfloat16).double().view(Bn, heads, nblk, 32, 64)
    k = torch.empty_like(vals).scatter_(-1, idx.view(32, 64).expand(Bn, heads, nblk, 32, 64), vals)
    return k.view(Bn, heads, nblk * 32, 64)[:, :, :N]
