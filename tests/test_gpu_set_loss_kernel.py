"""GPU tier: parq_set_loss_flags (parq_amd/csrc/setloss.hip: four loss terms and d term / d output) called directly with hand-built
pairs, against the float64 oracle of tests/tail_oracles.py (pinned to the reference's golden g10 by tests/test_tail_oracles_cpu.py).

Tolerance: the same oracle evaluated in float32 on the CPU has the error class of an fp32 evaluation of these formulas; the kernel
may differ from float64 by 4x that plus 1e-6 (a different summation order at equal precision, as for the fp16 x 3 tile in
test_gpu_kernels.py), per term and per gradient ROW relative to that row's norm - a whole-tensor norm lets one wrong row hide behind
hundreds of right ones, and a row a thousand times larger (|a| = 1e-3) hide all others.  Measured errors: profiles/tail_kernel_errors.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from parq_amd import _lib
from gpu_util import lib, sptr
from set_loss_cases import EDGE_EQUAL, EDGE_LARGE_A, EDGE_NEAR_PARALLEL, EDGE_SMALL_A, make_case
from tail_oracles import set_loss_oracle

pytestmark = pytest.mark.gpu
SHAPES = {"small": (3, 2, 48, 19, 10), "wide": (2, 3, 100, 10, 64)}           # I, B, Q, ncls, nmax
SEEDS = {"small": 911, "wide": 912}                                          # chosen on the CPU: see test_seeds_leave_few_pairs_out
GUARD, PATTERN = 64, 0x5A5A5A5A
NAMES = ("logits", "center", "size", "o6")


def run_kernel(case, flags=0, sym_on=True):
    """Arguments packed as _SetLossFn.forward packs them: pairs [4][P] | coef [P] | row_weight [I*B*Q] in one int32 buffer; the scratch
    is exactly parq_set_loss_scratch_bytes long with a guard behind it, which must come back untouched."""
    o, tg = case["outputs"], case["targets"]
    I, B, Q, ncls = o["logits"].shape
    nmax, P = tg["t_label"].shape[1], case["pairs"].shape[1]
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: cu(v) for k, v in list(o.items()) + list(tg.items())}
    packed = cu(np.concatenate([case["pairs"].astype(np.int32).reshape(-1), case["coef"].astype(np.float32).view(np.int32),
                                case["row_weight"].astype(np.float32).reshape(-1).view(np.int32)]))
    t_sym, cw = (cu(case["sym"].astype(np.int32)) if sym_on else None), cu(case["class_weight"].astype(np.float32))
    l = lib()
    nbytes = l.parq_set_loss_scratch_bytes(I, B, Q, P, flags)
    assert nbytes >= I * B * Q * 4 and nbytes % 4 == 0
    scratch = torch.full((nbytes // 4 + GUARD,), PATTERN, dtype=torch.int32, device="cuda")
    terms = torch.full((4,), float("nan"), device="cuda")
    g = [torch.full(o[k].shape, float("nan"), device="cuda") for k in NAMES]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    base = packed.data_ptr()
    w4 = (C.c_float * 4)(*[float(x) for x in case["w4"]])
    _lib.check(l.parq_set_loss_flags(p(d["logits"]), p(d["center"]), p(d["size"]), p(d["o6"]), I, B, Q, ncls, p(d["t_center"]), p(d["t_size"]),
                                     p(d["t_rot"]), p(d["t_label"]), p(t_sym), nmax, C.c_void_p(base) if P else None,
                                     C.c_void_p(base + 16 * P) if P else None, P, C.c_void_p(base + 20 * P), p(cw), w4, p(terms), p(g[0]), p(g[1]),
                                     p(g[2]), p(g[3]), p(scratch), flags, sptr()), "parq_set_loss_flags")
    assert (scratch[nbytes // 4:] == PATTERN).all(), "the kernel wrote behind its scratch"
    return terms.cpu().numpy(), [t.cpu().numpy() for t in g]


@functools.lru_cache(maxsize=None)
def _case(shape, P, sym_on=True, edges=True):
    case = make_case(*SHAPES[shape], P, SEEDS[shape], edges=edges, turn=sym_on)
    orc = lambda dt: set_loss_oracle(case["outputs"], case["targets"], case["pairs"], case["coef"], case["row_weight"], case["class_weight"],
                                     case["w4"], case["sym"] if sym_on else None, dtype=dt)
    return case, orc(torch.float64), orc(torch.float32)


def compare(tag, got_terms, got_grads, r64, r32, left_out=None, log=print):
    """Every term and every gradient row within 4 x (error of the float32 oracle) + 1e-6 of the float64 oracle; rows whose float64
    gradient is exactly zero must be exactly zero.  `left_out`: pairs' rows of the rotation gradient that are not judged."""
    assert np.isfinite(got_terms).all() and all(np.isfinite(g).all() for g in got_grads)
    worst = []
    for j, name in enumerate(("centre", "size", "rotation", "class")):
        den = max(1.0, abs(r64.terms[j]))
        ek, e32 = abs(float(got_terms[j]) - r64.terms[j]) / den, abs(r32.terms[j] - r64.terms[j]) / den
        log("%s term %-8s kernel %.3e fp32-oracle %.3e" % (tag, name, ek, e32))
        worst.append((ek <= 4 * e32 + 1e-6, "term " + name, ek, e32))
    for name, got, g64, g32 in zip(NAMES, got_grads, r64.grads, r32.grads):
        last = g64.shape[-1]
        got, g64, g32 = (np.asarray(a, np.float64).reshape(-1, last) for a in (got, g64, g32))
        n64 = np.linalg.norm(g64, axis=1)
        zero = n64 == 0
        assert (got[zero] == 0).all(), (tag, name, "a row whose gradient is exactly zero")
        judged = ~zero
        if name == "o6" and left_out is not None:
            judged &= ~left_out
        ek = np.linalg.norm(got - g64, axis=1)[judged] / n64[judged]
        e32 = np.linalg.norm(g32 - g64, axis=1)[judged] / n64[judged]
        if ek.size:
            i = int(np.argmax(ek - 4 * e32))
            log("%s grad %-8s rows %5d  kernel max %.3e  fp32-oracle max %.3e  worst row: kernel %.3e fp32-oracle %.3e"
                % (tag, name, ek.size, ek.max(), e32.max(), ek[i], e32[i]))
            worst.append((bool((ek <= 4 * e32 + 1e-6).all()), "grad " + name, float(ek[i]), float(e32[i])))
    bad = [w for w in worst if not w[0]]
    assert not bad, (tag, bad)


def rot_rows_left_out(case, r64):
    """Rows of the rotation gradient whose best and second-best symmetry candidate are closer than 1e-4 in the oracle: the minimum
    may fall on either, so their gradient is not judged.  At most 2 % of the pairs."""
    I, B, Q = case["outputs"]["logits"].shape[:3]
    close = r64.gap < 1e-4
    assert close.sum() <= 0.02 * max(1, close.size), int(close.sum())
    out = np.zeros(I * B * Q, bool)
    pr = case["pairs"][:, close].astype(np.int64)
    out[(pr[0] * B + pr[1]) * Q + pr[2]] = True
    return out


CASES = [(s, P) for s in SHAPES for P in (0, 1, 255, 256, 257, 600) if P <= np.prod(SHAPES[s][:3])]


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("shape,P", CASES)
def test_terms_and_gradient_rows_match_the_float64_oracle(shape, P, flags):
    """P = 0, 1 and both sides of one workgroup of pairs (255, 256, 257), 600 = three workgroups; symmetry classes 0..3 all present;
    edge rows (tests/set_loss_cases.py): a residual exactly zero, |a| = 1e-3 and 1e3, a and b 5 degrees apart, logits spread over
    +-80, an (iteration, scene) of weight 0, target labels -1 and ncls + 3."""
    case, r64, r32 = _case(shape, P)
    terms, grads = run_kernel(case, flags)
    compare("%s P=%d flags=%d" % (shape, P, flags), terms, grads, r64, r32, rot_rows_left_out(case, r64))
    I, B, Q, ncls, nmax = SHAPES[shape]
    if P == 0:
        assert (terms[:3] == 0).all() and all((g == 0).all() for g in grads[1:])
        assert r64.terms[3] > 0
    assert (grads[0][I - 1, B - 1] == 0).all()                               # rows of weight 0: exactly 0, not NaN
    lg, cls, rw = case["outputs"]["logits"].astype(np.float64), r64.cls, case["row_weight"].astype(np.float64)
    srt = np.sort(lg, -1)
    sat = (srt[..., -1] - srt[..., -2] > 30) & (rw > 0)                      # saturated rows: -s at the target, +s at the maximum
    assert sat.sum() > 10
    s = rw * case["w4"][3] * case["class_weight"][cls]
    want = np.zeros_like(lg)
    np.put_along_axis(want, lg.argmax(-1)[..., None], s[..., None], -1)
    np.put_along_axis(want, cls[..., None], np.take_along_axis(want, cls[..., None], -1) - s[..., None], -1)
    assert np.abs(grads[0][sat] - want[sat]).max() <= 1e-5 * s[sat].max()
    if P > 8:
        k, b, q, g = case["pairs"][:, EDGE_EQUAL]
        assert grads[1][k, b, q, 0] == 0 and grads[2][k, b, q, 1] == 0
        assert (grads[1][k, b, q, 1:] != 0).all() and grads[2][k, b, q, 0] != 0
        na = lambda e: np.linalg.norm(grads[3][tuple(case["pairs"][:3, e])][:3])
        assert na(EDGE_SMALL_A) > 1e4 * na(EDGE_LARGE_A) > 0                 # d / d a scales with 1 / |a|
        assert set(np.unique(r64.cls[case["pairs"][0, 4:6], case["pairs"][1, 4:6], case["pairs"][2, 4:6]]).tolist()) == {ncls - 1}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_seeds_leave_few_pairs_out(shape):
    """The condition on the inputs, from the oracle alone: at the largest P of each shape at most 2 % of the pairs have their two best
    symmetry candidates within 1e-4, and every symmetry class occurs among the pairs."""
    P = max(p for s, p in CASES if s == shape)
    case, r64, _ = _case(shape, P)
    rot_rows_left_out(case, r64)
    assert set(case["sym"][case["pairs"][1], case["pairs"][3]].tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("shape,P", [("small", 257), ("wide", 600)])
def test_without_symmetry_classes(shape, P):
    """t_sym = NULL: every pair compares with its box's rotation alone."""
    case, r64, r32 = _case(shape, P, sym_on=False)
    terms, grads = run_kernel(case, 0, sym_on=False)
    assert np.isinf(r64.gap).all()
    compare("%s P=%d nosym" % (shape, P), terms, grads, r64, r32)


def test_two_classes():
    """num_classes = 2: one class and background."""
    I, B, Q, nmax, P = 2, 2, 70, 6, 257
    case = make_case(I, B, Q, 2, nmax, P, 913)
    args = (case["outputs"], case["targets"], case["pairs"], case["coef"], case["row_weight"], case["class_weight"], case["w4"], case["sym"])
    r64, r32 = set_loss_oracle(*args, dtype=torch.float64), set_loss_oracle(*args, dtype=torch.float32)
    for flags in (0, 1):
        terms, grads = run_kernel(case, flags)
        compare("two classes flags=%d" % flags, terms, grads, r64, r32, rot_rows_left_out(case, r64))
    assert set(np.unique(r64.cls).tolist()) == {0, 1}


def test_pairs_outside_the_tensors_are_skipped():
    """The documented skip: a pair with q = Q and one with g = nmax change no term and no gradient."""
    case, r64, r32 = _case("small", 255)
    I, B, Q, ncls, nmax = SHAPES["small"]
    more = dict(case)
    more["pairs"] = np.concatenate([case["pairs"][:, :100], np.array([[1, 0], [1, 0], [Q, 5], [2, nmax]], np.int32), case["pairs"][:, 100:]], 1)
    more["coef"] = np.concatenate([case["coef"][:100], np.float32([0.5, 0.25]), case["coef"][100:]])
    assert more["pairs"].shape[1] == 257
    o64 = set_loss_oracle(more["outputs"], more["targets"], more["pairs"], more["coef"], more["row_weight"], more["class_weight"], more["w4"],
                          more["sym"])
    assert o64.terms == r64.terms and all(np.array_equal(a, b) for a, b in zip(o64.grads, r64.grads))
    for flags in (0, 1):
        t0, g0 = run_kernel(case, flags)
        t1, g1 = run_kernel(more, flags)
        compare("skip flags=%d" % flags, t1, g1, r64, r32, rot_rows_left_out(case, r64))
        assert all(np.array_equal(a, b) for a, b in zip(g0, g1))
        if flags:
            assert np.array_equal(t0[3:], t1[3:])                            # (the pair terms' partials fall into other workgroups)


@pytest.mark.parametrize("shape,P", [("small", 257), ("wide", 600), ("wide", 0)])
def test_deterministic_flag_changes_only_the_summation_of_the_terms(shape, P):
    """Gradients bit-equal to the flag-off call (only the term sums differ), terms bit-identical between two flagged calls, and the
    guard behind the scratch of exactly parq_set_loss_scratch_bytes untouched (asserted by run_kernel in every call)."""
    case, r64, r32 = _case(shape, P)
    t0, g0 = run_kernel(case, 0)
    t1, g1 = run_kernel(case, 1)
    t2, g2 = run_kernel(case, 1)
    assert all(a.tobytes() == b.tobytes() == c.tobytes() for a, b, c in zip(g0, g1, g2))
    assert t1.tobytes() == t2.tobytes()
    compare("%s P=%d deterministic" % (shape, P), t1, g1, r64, r32, rot_rows_left_out(case, r64))
    I, B, Q = SHAPES[shape][:3]
    assert lib().parq_set_loss_scratch_bytes(I, B, Q, P, 1) == 4 * (I * B * Q + 3 * ((P + 255) // 256) + (I * B * Q + 255) // 256)
