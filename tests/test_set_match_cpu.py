"""CPU tier of the device matcher (include/parq_hip.h parq_set_match): the NumPy statement of tests/set_match_cases.py against the
host matcher (HungarianMatcherModified and the loop of decoder_loss_batched) where no cap binds, the cap rule and its hash where
one does, the entry points' declaration and binding, and the argument checks that return before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from parq_amd import Obb3D, Pose, _lib
from parq_amd.loss import HungarianMatcherModified, decoder_loss_batched

import set_match_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("parq_set_match_workspace_bytes", "parq_set_match")


def _host_matcher(outs, targets):
    """HungarianMatcherModified per iteration: [[(p, g) per scene]], [[punish per scene]]."""
    matcher = HungarianMatcherModified(cost_class=2, cost_bbox=0.25)
    idx, pun = [], []
    for o in outs:
        i, p = matcher({k: torch.from_numpy(v) for k, v in o.items()}, targets)
        idx.append(i)
        pun.append([x.numpy() for x in p])
    return idx, pun


def _batched_loop(outs, obbs, T_wl, sym, monkeypatch):
    """The flat pairs [segment, query, box, scene] and the punish masks (I, B, Q) that decoder_loss_batched's loop hands its tail."""
    seen = []
    real = torch.from_numpy

    def spy(a):
        seen.append(np.array(a))
        return real(a)
    monkeypatch.setattr(torch, "from_numpy", spy)
    cw = torch.ones(10)
    cw[9] = 0.1
    decoder_loss_batched([{k: real(v) for k, v in o.items()} for o in outs], Obb3D(real(obbs)), Pose(real(T_wl)), real(sym),
                         matcher=HungarianMatcherModified(cost_class=2, cost_bbox=0.25), loss_weight=[5.0, 5.0, 5.0, 1.0], num_semcls=9,
                         class_weight=cw)
    monkeypatch.undo()
    packed = [a for a in seen if a.dtype == np.int64 and a.ndim == 2 and a.shape[0] == 4]
    punish = [a for a in seen if a.dtype == bool and a.ndim == 3]
    assert len(packed) == 1 and len(punish) == 1
    return packed[0], punish[0]


@pytest.mark.parametrize("seed", M.ROBUST_SEEDS)
def test_statement_equals_the_host_matcher_where_no_cap_binds(seed, monkeypatch):
    outs, obbs, T_wl, sym, targets = M.host_case(seed)
    m, near, counts = M.host_case_cost(outs, targets)
    I, B, Q = m.shape[:3]
    assert not M.over_full(near, counts, M.MAX_PADDING).any() and near.any()
    state = np.random.get_state()
    np.random.seed(77)
    st = M.match_statement(m, near, counts, seed=5, step=3)
    idx, pun = _host_matcher(outs, targets)
    packed, punish_loop = _batched_loop(outs, obbs, T_wl, sym, monkeypatch)
    assert np.random.random() == np.random.RandomState(77).random_sample()      # nobody drew a sample
    np.random.set_state(state)
    rng = np.random.RandomState(seed)
    at = 0
    for k in range(I):
        for b in range(B):
            n = counts[b]
            p, g = M.segment_pairs(st, k, b)
            assert np.array_equal(p, idx[k][b][0]) and np.array_equal(g, idx[k][b][1]), (k, b)
            assert np.array_equal(st["punish"][k, b], pun[k][b]) and np.array_equal(st["punish"][k, b], punish_loop[k, b])
            assert st["punish"][k, b].all()
            seg = packed[:, at:at + len(p)]
            at += len(p)
            assert (seg[0] == k * B + b).all() and (seg[3] == b).all() and np.array_equal(seg[1], p) and np.array_equal(seg[2], g)
            # robust: +-1e-5 on the cost leaves scipy's assignment, so the last bits of the device's expf cannot flip a match
            cost = -m[k, b, :, :n].astype(np.float64)
            rows, cols = linear_sum_assignment(cost)
            got = st["row_to_col"][k, b]
            assert np.array_equal(np.nonzero(got >= 0)[0], rows) and np.array_equal(got[rows], cols)
            for _ in range(20):
                r2, c2 = linear_sum_assignment(cost + rng.uniform(-1e-5, 1e-5, cost.shape))
                assert np.array_equal(r2, rows) and np.array_equal(c2, cols), (seed, k, b)
    assert at == packed.shape[1]
    # the constants of the loss, as _device_set_loss computes them from the host pairs
    cnt = np.bincount(packed[0], minlength=I * B).astype(np.float32)
    vbs = int((cnt > 0).sum())
    assert st["stats"].tolist() == cnt.astype(np.int32).tolist() + [vbs]
    assert np.array_equal(st["pair_coef"].reshape(I * B, Q)[:, 0], np.float32(1.0) / (cnt * np.float32(vbs)))
    pm = punish_loop.astype(np.float32)
    assert np.array_equal(st["row_weight"], (pm / pm.sum(-1, keepdims=True) * np.float32(1.0) / np.float32(vbs)).reshape(-1))


def test_cap_rule_on_over_full_boxes():
    outs, obbs, T_wl, sym, targets = M.host_case(1, capped=True)
    m, near, counts = M.host_case_cost(outs, targets)
    I, B, Q = m.shape[:3]
    over = M.over_full(near, counts, M.MAX_PADDING)
    assert over[:, 0, counts[0] - 1].all() and over[:, 1, 0].all() and over.sum() == 2 * I
    st = M.match_statement(m, near, counts, seed=9, step=0)
    other = M.match_statement(m, near, counts, seed=9, step=1)
    for k in range(I):
        for b in range(B):
            n = counts[b]
            ch, nr = st["chosen"][k, b, :, :n], near[k, b, :, :n]
            assert not (ch & ~nr).any()
            for j in range(n):                                               # exactly max_padding per over-full box, everyone otherwise
                assert ch[:, j].sum() == (M.MAX_PADDING if over[k, b, j] else nr[:, j].sum())
            r2c, g = st["row_to_col"][k, b], st["g"][k, b]
            assert (g[r2c >= 0] == r2c[r2c >= 0]).all()                      # a query assigned by the Hungarian step keeps its box
            for q in np.nonzero(r2c < 0)[0]:                                 # the lowest box wins among extras
                assert g[q] == (int(np.nonzero(ch[q])[0][0]) if ch[q].any() else -1)
            zeros = ~st["punish"][k, b]                                      # punish zeros: unchosen neighbours of the LAST box only
            assert np.array_equal(zeros, nr[:, n - 1] & ~ch[:, n - 1])
            assert zeros.sum() == (int(nr[:, n - 1].sum()) - M.MAX_PADDING if over[k, b, n - 1] else 0)
    assert (~st["punish"][:, 0]).any() and st["punish"][:, 1].all()
    assert not np.array_equal(st["chosen"], other["chosen"])                 # another step, another draw
    assert np.array_equal(st["row_to_col"], other["row_to_col"])
    pm = st["punish"].astype(np.float32)
    vbs = np.float32(st["stats"][-1])
    assert vbs == I * B
    assert np.array_equal(st["row_weight"], (pm / pm.sum(-1, keepdims=True) / vbs).reshape(-1))


def test_capped_draw_is_uniform_over_the_neighbours():
    """Over 2000 seeds each of c = 14 neighbours is kept with frequency max_padding / c within 4 binomial standard deviations (and so
    is each of 31 under another (step, iteration, scene, box))."""
    for c, qs, (step, k, b, j) in ((14, np.arange(3, 60, 4)[:14], (0, 0, 0, 0)), (31, np.arange(31) * 9 + 1, (7, 5, 3, 11))):
        n_seeds = 2000
        hits = np.zeros(c)
        for seed in range(n_seeds):
            keys = M.match_keys(seed * 0x100000001 + 17, step, k, b, j, qs)
            hits[np.lexsort((qs, keys))[:M.MAX_PADDING]] += 1
        p = M.MAX_PADDING / c
        sd = np.sqrt(n_seeds * p * (1 - p))
        assert np.abs(hits - n_seeds * p).max() <= 4 * sd, (c, hits)
    # the stated hash, once in plain integers
    def mix(h):
        h ^= h >> 16
        h = (h * 0x7FEB352D) & 0xFFFFFFFF
        h ^= h >> 15
        h = (h * 0x846CA68B) & 0xFFFFFFFF
        return h ^ (h >> 16)
    h = 0x9E3779B9
    for w in (0xDEADBEEF, 0x12345678, 41, 6, 2, 11, 299):
        h = mix(((h ^ w) + 0x9E3779B9) & 0xFFFFFFFF)
    assert int(M.match_keys(0x12345678DEADBEEF, 41, 6, 2, 11, [299])[0]) == h


def test_g10_matching_draws_no_random_number():
    """The reference golden g10 has no box with more than 10 neighbours (its fullest has exactly 10): its matching draws nothing from
    np.random, the statement gives the host matcher's pairs on it, and the device path is held to its terms (test_gpu_set_match.py)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from make_golden import LOSS_CASE, loss_case_inputs
    from parq_amd.loss import parse_target
    outs, obbs, T_wl, sym = loss_case_inputs(LOSS_CASE)
    targets = parse_target(Obb3D(torch.from_numpy(obbs)), Pose(torch.from_numpy(T_wl)))
    m, near, counts = M.host_case_cost(outs, targets)
    assert not M.over_full(near, counts, M.MAX_PADDING).any() and near.sum(2).max() == M.MAX_PADDING
    state = np.random.get_state()
    np.random.seed(77)
    idx, pun = _host_matcher(outs, targets)
    assert np.random.random() == np.random.RandomState(77).random_sample()
    np.random.set_state(state)
    st = M.match_statement(m, near, counts, seed=0, step=0)
    for k in range(m.shape[0]):
        for b in range(m.shape[1]):
            p, g = M.segment_pairs(st, k, b)
            assert np.array_equal(p, idx[k][b][0]) and np.array_equal(g, idx[k][b][1]) and np.array_equal(st["punish"][k, b], pun[k][b])


def test_kernel_cases_are_what_they_say():
    for shape in M.SHAPES:
        for variant in M.VARIANTS:
            c = M.kernel_case(shape, variant)
            m, near = M.cost_statement(c["logits"], c["coord"], c["t_center"], c["t_label"], c["t_count"])
            over = M.over_full(near, c["t_count"], c["max_padding"])
            n = c["t_count"]
            if variant == "none":
                assert not over.any() and near.any()
            elif variant == "last":
                assert all(over[:, b, n[b] - 1].all() for b in range(c["B"])) and over.sum() == c["I"] * c["B"]
            else:
                assert over[:, :, 0].all() and all(over[:, b, 1].all() for b in range(c["B"]) if n[b] >= 2)
                assert any((near[:, b, :, 0] & near[:, b, :, 1]).any() for b in range(c["B"]) if n[b] >= 2) or (n < 2).all()


def test_header_declares_the_entry_points_and_the_binding_types_them():
    hdr = open(os.path.join(ROOT, "include", "parq_hip.h")).read()
    want = {"parq_set_match_workspace_bytes": ["I", "B", "Q", "nmax"],
            "parq_set_match": ["pred_logits", "coord_pos", "I", "B", "Q", "num_classes", "t_center", "t_label", "t_count", "nmax", "cost_class",
                               "cost_bbox", "ratio", "max_padding", "seed_lo", "seed_hi", "step", "workspace", "workspace_bytes", "row_to_col",
                               "pairs", "pair_coef", "row_weight", "stats", "cost_out", "near_out", "stream"]}
    for name, names in want.items():
        m = re.search(r"\b(?:int|size_t)\s+\(%s\)\s*\(([^;]*)\)\s*;" % name, hdr)
        assert m, "include/parq_hip.h must declare %s" % name
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1).replace("\n", " ")).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == names, name
        assert name in _lib.MATCH_SYMBOLS and name not in _lib.SYMBOLS and name not in _lib.EXTRA_SYMBOLS
        res, args = _lib.MATCH_SYMBOLS[name]
        assert len(args) == len(names) and res is (C.c_size_t if name.endswith("bytes") else C.c_int)
        for p, a in zip(params, args):                                       # pointers as void *, scalars by their C type
            kind = C.c_void_p if "*" in p else {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "size_t": C.c_size_t,
                                                "parq_stream": C.c_void_p}[p.split()[0]]
            assert a is kind, (name, p)
    assert len(_lib.SYMBOLS) == 71 and len(_lib.EXTRA_SYMBOLS) == 17 and len(_lib.MATCH_SYMBOLS) == 2
    assert "87" in open(os.path.join(ROOT, "README.md")).read()


def test_library_exports_the_entry_points_and_sizes():
    lib = _lib.load()
    for name in NEW:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.MATCH_SYMBOLS[name][1] and fn.restype is _lib.MATCH_SYMBOLS[name][0]
    size = lib.parq_set_match_workspace_bytes
    S, Q, nmax = 6, 70, 5
    assert size(2, 3, Q, nmax) == (S * (Q + nmax) * 8 + S * 32 + S * Q * nmax * 5 + 15) // 16 * 16
    assert size(0, 3, Q, nmax) == 0 and size(8, 4, 2048, 2048) > 0
    for bad in ((-1, 1, 8, 8), (1, -1, 8, 8), (1, 1, 0, 8), (1, 1, 2049, 8), (1, 1, 8, 0), (1, 1, 8, 2049), (1 << 14, 1 << 14, 8, 8)):
        assert size(*bad) == 0, bad


def test_argument_errors_return_before_any_device_call():
    """PARQ_ERR_ARG (1) from checks made on the host: the pointers below are never dereferenced."""
    lib = _lib.load()
    p, odd = C.c_void_p(4096), C.c_void_p(4104)                              # non-NULL, never touched
    need = lib.parq_set_match_workspace_bytes(2, 2, 8, 4)

    def call(lg=p, cp=p, I=2, B=2, Q=8, ncls=4, tc=p, tl=p, tn=p, nmax=4, pad=10, ws=p, wsb=need, r2c=p, pairs=p, coef=p, rw=p, stats=p):
        return lib.parq_set_match(lg, cp, I, B, Q, ncls, tc, tl, tn, nmax, 2.0, 0.25, 0.2, pad, 1, 2, 3, ws, wsb, r2c, pairs, coef, rw, stats,
                                  None, None, None)
    assert call(I=0) == 0 and call(B=0, lg=None, ws=None) == 0               # no problem: valid, nothing launched
    for kw in (dict(I=-1), dict(B=-1), dict(pad=-1), dict(Q=0), dict(Q=2049), dict(nmax=0), dict(nmax=2049), dict(ncls=1), dict(lg=None),
               dict(cp=None), dict(tc=None), dict(tl=None), dict(tn=None), dict(ws=None), dict(r2c=None), dict(pairs=None), dict(coef=None),
               dict(rw=None), dict(stats=None), dict(wsb=need - 1), dict(ws=odd), dict(I=1 << 14, B=1 << 14)):
        assert call(**kw) == 1, kw
    assert b"parq_set_match" in lib.parq_last_error()
