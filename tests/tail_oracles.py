"""Float64 statements of the two kernels that turn decoder outputs into what a user reads: parse_pred + 3-D NMS
(parq_amd/csrc/postproc.hip) and the set loss with its output gradients (parq_amd/csrc/setloss.hip).  Plain NumPy / torch on the
CPU; tests/test_tail_oracles_cpu.py pins both to the goldens recorded from the reference (g11, g10)."""
import math
from collections import namedtuple

import numpy as np
import torch

ParsePred = namedtuple("ParsePred", "obbs mask margin pairs order label valid")
SetLoss = namedtuple("SetLoss", "terms grads gap cls")


def _cross(u, v):
    return np.stack((u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1],
                     u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]), -1)


def _norm(v):
    return np.maximum(np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]), 1e-8)[..., None]


def visit_order(score):
    """Visit order of the NMS over the candidates' scores: descending score, ties visit the higher index first, a NaN score
    sorts above every number (np.argsort puts NaN last) with the higher index first among NaNs."""
    return np.argsort(np.asarray(score, np.float64), kind="stable")[::-1]


def parse_pred_oracle(center, size, rot6, prob, track_scale, for_vis, enable_nms):
    """model/parq_decoder.py:372-424 with utils/nms.py:141-224 in float64 on the float32 inputs.  Returns the boxes (B, Q, 19), the
    keep mask, the smallest |IoU - threshold| over the pairs that were evaluated with both boxes alive, their number, the visit order
    of every scene, the labels and the validity flags."""
    c, s, o6 = (np.asarray(a, np.float32).astype(np.float64) for a in (center, size, rot6))
    prob = np.asarray(prob, np.float32)
    B, Q, ncls = prob.shape
    with np.errstate(invalid="ignore", divide="ignore"):
        x = o6[..., :3] / _norm(o6[..., :3])
        z = _cross(x, o6[..., 3:])
        z = z / _norm(z)
        y = _cross(z, x)
        R = np.stack((x, y, z), -1)                                        # columns x, y, z
        score = prob.max(-1)                                               # no arithmetic: the float32 values themselves
        label = prob.argmax(-1)                                            # first maximum
        obbs = np.concatenate([np.stack((-s[..., 0] / 2, s[..., 0] / 2, -s[..., 1] / 2, s[..., 1] / 2, -s[..., 2] / 2, s[..., 2] / 2), -1),
                               R.reshape(B, Q, 9), c, label[..., None].astype(np.float64)], -1)
        sign = np.array([[(1 if k & 1 else -1), (1 if k & 2 else -1), (1 if k & 4 else -1)] for k in range(8)], np.float64)
        corner = sign[None, None] * (s / 2)[:, :, None, :]                 # (B, Q, 8, 3) in the box frame
        pts = (corner[..., None, 0] * R[:, :, None, :, 0] + corner[..., None, 1] * R[:, :, None, :, 1]
               + corner[..., None, 2] * R[:, :, None, :, 2] + c[:, :, None, :])
        lo, hi = pts.min(2), pts.max(2)
    ts = [float(np.float32(t)) for t in track_scale]
    if for_vis:
        valid = np.ones((B, Q), bool)
    else:
        valid = (c[..., 0] > ts[0]) & (c[..., 0] < ts[1]) & (c[..., 2] > ts[4]) & (c[..., 2] < ts[5])
    thr = 0.2 if for_vis else 0.1
    picked = np.zeros((B, Q), bool)
    margin, pairs, orders = math.inf, 0, []
    for b in range(B):
        cand = np.nonzero(label[b] != ncls - 1)[0]
        order = cand[visit_order(score[b, cand])]
        orders.append(order)
        if not enable_nms:
            continue
        vol = (hi[b, :, 0] - lo[b, :, 0]) * (hi[b, :, 1] - lo[b, :, 1]) * (hi[b, :, 2] - lo[b, :, 2])
        alive = np.zeros(Q, bool)
        alive[cand] = True
        for pos, i in enumerate(order):
            if not alive[i]:
                continue
            picked[b, i] = True
            rest = order[pos + 1:]
            rest = rest[alive[rest]]
            if rest.size == 0:
                continue
            with np.errstate(invalid="ignore", divide="ignore"):
                ext = [np.maximum(0, np.minimum(hi[b, i, a], hi[b, rest, a]) - np.maximum(lo[b, i, a], lo[b, rest, a])) for a in range(3)]
                inter = ext[0] * ext[1] * ext[2]
                o = inter / (vol[i] + vol[rest] - inter)
                if for_vis:
                    o = o * (label[b, i] == label[b, rest])
                gap = np.abs(o - thr)
            if for_vis:                                                    # a pair of different classes has no IoU to compare
                gap = gap[label[b, i] == label[b, rest]]
            pairs += int(gap.size)
            if np.isfinite(gap).any():
                margin = min(margin, float(np.nanmin(gap)))
            with np.errstate(invalid="ignore"):
                alive[rest[o > thr]] = False
    mask = (picked & valid) if enable_nms else valid.copy()
    return ParsePred(obbs, mask, margin, pairs, orders, label, valid)


def _rotation(o6):
    """(n, 6) -> (n, 3, 3), columns x, y, z; both norms clamped at 1e-8 (utils/ortho6d_transforms.py:52-66)."""
    def unit(v):
        return v / torch.sqrt((v * v).sum(1)).clamp_min(1e-8).unsqueeze(1)

    def cross(u, v):
        return torch.stack((u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                            u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]), 1)
    x = unit(o6[:, 0:3])
    z = unit(cross(x, o6[:, 3:6]))
    return torch.stack((x, cross(z, x), z), 2)


def set_loss_oracle(outputs, targets, pairs, coef, row_weight, class_weight, w4, sym, dtype=torch.float64):
    """The formulas of the header of setloss.hip as a torch expression on leaves of `dtype`; gradients from autograd, one backward
    per term.  outputs: logits (I, B, Q, ncls), center, size (.., 3), o6 (.., 6).  targets: t_center, t_size (B, nmax, 3), t_rot
    (B, nmax, 3, 3), t_label (B, nmax).  pairs (4, P) = k, b, q, g; a pair with an index outside the tensors is skipped, a label
    outside [0, ncls) is background.  sym: (B, nmax) symmetry classes or None.  Returns the four terms (floats), the four gradients
    (logits, center, size, o6; float64 arrays), per kept-or-skipped pair the gap between the best and the second-best symmetry
    candidate's error (inf where there is one candidate or the pair is skipped), and the class targets."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)
    logits, ctr, siz, o6 = (t(outputs[k]).requires_grad_(True) for k in ("logits", "center", "size", "o6"))
    I, B, Q, ncls = logits.shape
    t_center, t_size, t_rot = t(targets["t_center"]), t(targets["t_size"]), t(targets["t_rot"])
    t_label = np.asarray(targets["t_label"]).astype(np.int64)
    nmax = t_label.shape[1]
    pairs = np.asarray(pairs, np.int64).reshape(4, -1)
    P = pairs.shape[1]
    keep = ((pairs[0] >= 0) & (pairs[0] < I) & (pairs[1] >= 0) & (pairs[1] < B) & (pairs[2] >= 0) & (pairs[2] < Q)
            & (pairs[3] >= 0) & (pairs[3] < nmax))
    k, b, q, g = (torch.from_numpy(pairs[j][keep]) for j in range(4))
    cf = t(np.asarray(coef, np.float64).reshape(-1)[:P][keep])
    w = [float(np.float32(x)) for x in w4]
    gap = np.full(P, np.inf)
    if int(keep.sum()):
        term_c = ((ctr[k, b, q] - t_center[b, g]).abs().mean(-1) * cf).sum() * w[0]
        term_s = ((siz[k, b, q] - t_size[b, g]).abs().mean(-1) * cf).sum() * w[1]
        R = _rotation(o6[k, b, q])
        T = t_rot[b, g]
        per = ((R - T) ** 2).mean(dim=(1, 2))
        if sym is not None:
            sy = torch.from_numpy(np.asarray(sym).astype(np.int64))[b, g]
            kept_idx = np.nonzero(keep)[0]
            for cls, m in ((1, 2), (2, 4), (3, 36)):
                sel = torch.nonzero(sy == cls).squeeze(1)
                if sel.numel() == 0:
                    continue
                ry = []
                for j in range(m):
                    th = (j * 2.0 / m) * math.pi
                    ry.append([[math.cos(th), 0.0, math.sin(th)], [0.0, 1.0, 0.0], [-math.sin(th), 0.0, math.cos(th)]])
                cand = T[sel].unsqueeze(1) @ torch.tensor(ry, dtype=torch.float64).to(dtype)          # (n, m, 3, 3)
                err = ((R[sel].unsqueeze(1) - cand) ** 2).mean(dim=(2, 3))
                per = per.index_put((sel,), err.min(dim=1).values)
                two = torch.sort(err.detach().double(), dim=1).values[:, :2]
                gap[kept_idx[sel.numpy()]] = (two[:, 1] - two[:, 0]).numpy()
        term_r = (per * cf).sum() * w[2]
    else:
        term_c, term_s, term_r = ctr.sum() * 0, siz.sum() * 0, o6.sum() * 0
    cls_t = torch.full((I, B, Q), ncls - 1, dtype=torch.int64)
    lab = torch.from_numpy(t_label)[b, g]
    cls_t[k, b, q] = torch.where((lab >= 0) & (lab < ncls), lab, torch.full_like(lab, ncls - 1))
    cw = t(class_weight)
    rw = t(np.asarray(row_weight, np.float64).reshape(I, B, Q))
    nll = torch.logsumexp(logits, -1) - torch.gather(logits, -1, cls_t.unsqueeze(-1)).squeeze(-1)
    term_k = (rw * w[3] * cw[cls_t] * nll).sum()
    terms = [term_c, term_s, term_r, term_k]
    grads = [torch.autograd.grad(term, leaf)[0].double().numpy() for term, leaf in zip((term_k, term_c, term_s, term_r), (logits, ctr, siz, o6))]
    return SetLoss([float(x.detach()) for x in terms], grads, gap, cls_t.numpy())
