"""CPU tier: host-side mirror (state-dict contract, wrappers, C-ABI surface, loud failure
without a GPU).  No compute call reaches the GPU here."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from parq_amd import synth, Pose, Camera
from oracle import parq_oracle as O
import golden_util as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_weights(dec, W):
    sd = dec.state_dict()
    for k in sd:
        src = k.replace("parq_module.decoder.mlp_heads.", "mlp_heads.")
        sd[k] = torch.from_numpy(W[src]).reshape(sd[k].shape)
    dec.load_state_dict(sd, strict=True)


@pytest.mark.parametrize("tag", ["shared_d256", "unshared_d128"])
def test_state_dict_keys_match_reference(tag):
    from parq_amd.decoder import PARQDecoder
    schema = json.load(open(os.path.join(G.GOLDEN_DIR, "state_dict_keys.json")))[tag]
    dec = PARQDecoder(synth.decoder_cfg(**schema["cfg"]))
    mine = {k: list(v.shape) for k, v in dec.state_dict().items()}
    assert mine == schema["keys"]
    # the duplicated head entries share storage, as in the reference (parq_decoder.py:66)
    sd = dec.state_dict()
    assert sd["mlp_heads.center_head.layers.0.weight"].data_ptr() == \
        sd["parq_module.decoder.mlp_heads.center_head.layers.0.weight"].data_ptr()


def test_synthetic_weights_cover_every_parameter():
    from parq_amd.decoder import PARQDecoder
    cfg = synth.decoder_cfg(dim=128, queries=16, heads=2, ffn=96, layers=3, share_weights=False)
    dec = PARQDecoder(cfg)
    _load_weights(dec, synth.make_decoder_weights(cfg, 3))
    names = {n for n, _ in dec.named_parameters()}
    assert names == set(synth.decoder_param_shapes(cfg))


def test_header_symbols_are_exported_and_typed():
    from parq_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(parq_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    lib = _lib.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert b"gfx950" in lib.parq_version()


def test_product_library_reads_no_environment():
    """VERDICT r02 #3 / ADVICE: the development knobs and the kernels-with-ingredients-removed probes (PARQ_FLASH_PROBE,
    PARQ_KVPROJ_PROBE, ... — "results wrong by construction") exist only in the -DPARQ_DEV_PROBES build.  The product library
    must not even import getenv and must not contain one PARQ_* variable name; the version string says which build it is."""
    from parq_amd import _lib
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"PARQ_FLASH_PROBE" not in blob and b"PARQ_KVPROJ_PROBE" not in blob
    assert re.search(rb"PARQ_[A-Z][A-Z_0-9]{3,}", blob) is None
    assert b"getenv" not in blob                                   # not in the dynamic symbol table, not anywhere
    assert b"dev" not in _lib.load().parq_version().split(b"(")[0]
    assert not hasattr(_lib.load(), "parq_dev_timeline_missing") and not _lib.is_dev_library()
    with pytest.raises(AttributeError):
        _lib.load().parq_dev_timeline                              # the development entry point is not exported


def test_development_switches_are_exactly_the_documented_ones():
    """Every environment variable the development library reads (dev_env("PARQ_...") in parq_amd/csrc/) is listed, with what it does,
    under "Development switches" in tools/README.md — and nothing is listed that the source no longer reads.  A settled A/B is
    retired from both (profiles/variant_retirement.txt)."""
    csrc = os.path.join(ROOT, "parq_amd", "csrc")
    read = set()
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".hpp")):
            read |= set(re.findall(r'dev_env\("(PARQ_[A-Z0-9_]+)"', open(os.path.join(csrc, name)).read()))
    text = open(os.path.join(ROOT, "tools", "README.md")).read()
    section = text.split("## Development switches", 1)[1].split("\n## ", 1)[0]
    listed = re.findall(r"^ {4}(PARQ_[A-Z0-9_]+) ", section, re.M)       # one indented line per switch: name, then what it does
    assert len(listed) == len(set(listed)), sorted(listed)
    assert read, "no dev_env() call found: the scan is broken"
    assert set(listed) == read, (sorted(read - set(listed)), sorted(set(listed) - read))


def test_create_validates_config_without_gpu():
    from parq_amd import _lib
    lib = _lib.load()

    def mk(**kw):
        base = dict(dim=256, num_queries=64, num_classes=10, num_heads=4, ffn_dim=768, num_layers=8,
                    share_weights=1, num_mean_sizes=10)
        base.update(kw)
        return _lib.ParqConfig(scale=(C.c_float * 6)(-3, 3, -2, 0.5, 0.25, 5.25), **base)
    h = C.c_void_p()
    assert lib.parq_create(C.byref(mk()), C.byref(h)) == 0
    assert lib.parq_packed_weights_bytes(h) > 4 * 1_300_000          # 1.36 M parameters at d=256
    # forward before pack_weights is a state error, reported through parq_last_error
    sc = _lib.ParqScene(1, 2, 4, 4, 1, 1, 1, 1, 1)
    po = _lib.ParqOutputs(1, 1, 1, 1, 1, 1)
    assert lib.parq_forward(h, C.byref(sc), C.c_void_p(1), 16, C.byref(po), None) == 3
    assert b"pack_weights" in lib.parq_last_error()
    assert lib.parq_destroy(h) == 0
    for bad in (dict(dim=250), dict(num_heads=3), dict(num_heads=16), dict(ffn_dim=100), dict(num_classes=1),
                dict(num_queries=0)):
        assert lib.parq_create(C.byref(mk(**bad)), C.byref(h)) == 1, bad
        assert lib.parq_last_error() != b""


def test_decoder_refuses_cpu_tensors():
    from parq_amd.decoder import PARQDecoder
    cfg = synth.decoder_cfg(dim=64, queries=8, heads=1, ffn=64, layers=1)
    dec = PARQDecoder(cfg).eval()
    sc = synth.make_scene(1, 1, 2, 4, 6, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec(torch.from_numpy(sc["tokens"]), Camera(sc["camera"]), Pose(sc["T_camera_pseudoCam"]),
            Pose(sc["T_world_pseudoCam"]), Pose(sc["T_world_local"]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # the training path has no CPU fallback either
        dec.train()(torch.from_numpy(sc["tokens"]), Camera(sc["camera"]), Pose(sc["T_camera_pseudoCam"]),
                    Pose(sc["T_world_pseudoCam"]), Pose(sc["T_world_local"]))


def test_wrappers_match_oracle_geometry():
    cam, T_cp, T_wp, T_wl = synth.make_geometry(9, 2, 3, 12, 16)
    P = lambda a: Pose(torch.from_numpy(a))
    T_cl = P(T_cp) @ (P(T_wp).inverse() @ P(T_wl))
    want = O.camera_local_poses(torch.from_numpy(T_cp), torch.from_numpy(T_wp), torch.from_numpy(T_wl))
    assert torch.allclose(T_cl._data, want, atol=1e-6)
    pts = torch.from_numpy(synth.uniform(2, "pts", (2, 1, 7, 3), -2, 4))
    pc = T_cl.transform(pts)
    assert torch.allclose(pc, O.pose_transform(want, pts), atol=1e-6)
    uv, valid = Camera(torch.from_numpy(cam)).project(pc)
    uv2, valid2 = O.camera_project(torch.from_numpy(cam), pc)
    assert torch.allclose(uv, uv2) and torch.equal(valid, valid2)
    c4 = Camera(torch.from_numpy(cam)).scale(0.25)
    assert torch.allclose(c4.c, (torch.from_numpy(cam)[..., 4:6] + 0.5) * 0.25 - 0.5)
    assert T_cl[0].shape == (3,) and T_cl[0, 1]._data.shape == (12,)
    assert torch.stack([T_cl[0], T_cl[1]])._data.shape == (2, 3, 12)


def test_synth_is_deterministic():
    a = synth.normal(5, "x", (4, 3))
    b = synth.normal(5, "x", (4, 3))
    assert np.array_equal(a, b)
    assert abs(float(synth.normal(1, "big", (20000,)).std()) - 1.0) < 0.02
    # fixed fingerprint: changing the generator would silently invalidate every golden
    assert float(synth.uniform(7, "fingerprint", (1,))[0]) == np.float32(0.2026161402463913)
    assert float(synth.normal(7, "fingerprint", (1,))[0]) == np.float32(0.4613424837589264)


def test_dropout_hash_spec_row_pairs_are_statistically_independent():
    """NumPy restatement of the counter-based dropout keep decision (parq_amd/csrc/common.hpp: drop_rowhash, drop_colhash,
    drop_keep_h): drop rate ~p and, over ALL pairs of 512 rows x 4096 columns, no pair shares more of its dropped columns
    than independent draws would (the bare xor-and-compare shared 62-100 % for 1/16 of the pairs)."""
    M = np.uint64(0xFFFFFFFF)
    u32 = lambda x: (x & M).astype(np.uint64)

    def mix(x):
        x = u32(x); x ^= x >> np.uint64(16); x = u32(x * np.uint64(0x7feb352d)); x ^= x >> np.uint64(15)
        x = u32(x * np.uint64(0x846ca68b)); x ^= x >> np.uint64(16)
        return x
    p = 0.1
    thr = np.uint64(int(np.ceil(p * 2 ** 24)) << 8)

    def dropped(rows, cols, seed):
        with np.errstate(over="ignore"):
            r = mix(np.uint64(seed) ^ u32(np.arange(rows, dtype=np.uint64) * np.uint64(0x9e3779b1)))[:, None]
            # drop_colhash: block hash ^ register constant (bits 0, 1, 3, 4 of the column) ^ a constant where bit 2 is set
            j = np.arange(cols, dtype=np.uint64)
            k = j & np.uint64(31)
            c = mix(u32((j >> np.uint64(5)) * np.uint64(0x85ebca77) + np.uint64(0x6a09e667)))
            c = c ^ mix(np.uint64(0x3c6ef372) + ((k & np.uint64(3)) | ((k >> np.uint64(3)) << np.uint64(2))))
            c = (c ^ np.where((k & np.uint64(4)) != 0, mix(np.uint64(0xa54ff53a) + np.zeros(1, np.uint64)), np.uint64(0)))[None, :]
            # drop_keep_h: 24-bit multiply, shift-xor, 24-bit multiply
            h = u32(((r ^ c) & np.uint64(0xffffff)) * np.uint64(0x9E3779)); h ^= h >> np.uint64(16)
            h = u32((h & np.uint64(0xffffff)) * np.uint64(0x85EBCB))
        return h < thr
    d = dropped(512, 4096, 12345).astype(np.float64)
    assert abs(d.mean() - p) < 0.003
    per = d.sum(1)
    share = (d @ d.T) / per[:, None]
    np.fill_diagonal(share, 0.0)
    sigma = (p * (1 - p) / per.min()) ** 0.5
    assert share.max() < p + 6 * sigma, share.max()
    # the same for pairs of COLUMNS (the columns of a 32-column block differ by fixed xor constants, in every block and row): no two
    # of 1024 columns share more of their dropped rows than independent draws, and the co-drop frequency of every in-block column
    # pair, pooled over 32 blocks x 16384 rows, is p^2 within five standard deviations (pooled over six seeds: within 1.7 %)
    d = dropped(16384, 1024, 7).astype(np.float32)
    perc = d.sum(0)
    share = (d.T @ d) / perc[:, None]
    np.fill_diagonal(share, 0.0)
    sigma = (p * (1 - p) / perc.min()) ** 0.5
    assert share.max() < p + 6 * sigma, share.max()
    d3 = d.reshape(16384, 32, 32)
    co = np.einsum("rbk,rbl->kl", d3, d3) / (16384 * 32)
    off = ~np.eye(32, dtype=bool)
    sd = (p * p * (1 - p * p) / (16384 * 32)) ** 0.5          # 1.4 % of p^2 at this sample size
    assert np.abs(co[off] - p * p).max() < 5 * sd, np.abs(co[off] / (p * p) - 1).max()


def test_layernorm_pushed_through_the_query_projection_is_an_identity():
    """The algebra behind chain.hip's seam_tile (api.hip build_derived_weights: qg_w, qo_w, qu_b, q_s, qv_b), in float64 on random
    data: the cross-attention query rows (norm1(xa) + pos) Wq^T + bq with xa = tgt + sa Wo^T + bo and pos = pe_h W2^T + b2
    (model/transformer_parq.py:375-377) equal rstd (U - mean s) + V, where U and V contract operands that exist BEFORE xa does."""
    rng = np.random.default_rng(5)
    M, C = 48, 256
    sa, tgt, peh = (rng.standard_normal((M, C)) for _ in range(3))
    tgt = tgt + 0.7                                           # a row mean that is not small against the spread
    Wo, Wq, W2 = (rng.standard_normal((C, C)) / 16 for _ in range(3))
    bo, bq, b2, gamma, beta = (rng.standard_normal(C) for _ in range(5))
    eps = 1e-5
    xa = tgt + sa @ Wo.T + bo
    mean, var = xa.mean(-1, keepdims=True), xa.var(-1, keepdims=True)
    want = (((xa - mean) / np.sqrt(var + eps)) * gamma + beta + (peh @ W2.T + b2)) @ Wq.T + bq
    # pack time
    qg = Wq * gamma                                           # Wq diag(gamma)
    qo = qg @ Wo
    qu_b = qg @ bo
    q_s = qg.sum(-1)
    cross_q_w2, cross_q_b2 = Wq @ W2, bq + Wq @ b2            # (the position MLP's last layer folded: round 3)
    qv_b = cross_q_b2 + Wq @ beta
    # launch: query tiles
    U = sa @ qo.T + tgt @ qg.T + qu_b
    V = peh @ cross_q_w2.T + qv_b
    # ... and their epilogue, with the statistics from partial row sums over four 64-column tiles of xa
    S = sum(xa[:, 64 * t: 64 * t + 64].sum(-1) for t in range(4))
    Q = sum((xa[:, 64 * t: 64 * t + 64] ** 2).sum(-1) for t in range(4))
    mu = S / C
    rstd = 1.0 / np.sqrt(Q / C - mu * mu + eps)
    got = rstd[:, None] * (U - mu[:, None] * q_s) + V
    assert np.abs(got - want).max() < 1e-10 * max(1.0, np.abs(want).max())


def test_inflight_helper_is_importable_without_a_gpu_and_finds_the_tensors_of_a_call():
    """parq_amd.InFlight (several forwards of one module in flight): the module imports on a CPU-only host, and its argument walker
    finds plain tensors, the package's wrappers and tensors inside containers — the ones it must hand to record_stream."""
    import torch
    import parq_amd
    from parq_amd import inflight, Pose
    assert parq_amd.InFlight is inflight.InFlight
    a, b, c = torch.zeros(2), torch.ones(1, 12), torch.zeros(3)
    found = list(inflight._tensors(((a, {"pose": Pose(b), "n": 3}), {"kw": [c, "text"]})))
    assert len(found) == 3 and found[0] is a and found[1].shape == (1, 12) and found[2] is c
