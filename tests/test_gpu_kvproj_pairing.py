"""GPU tier: the persistent K/V projection kernel (kvproj_dma_kernel) after its column slices were rebalanced — each workgroup
of a slot projects the K and the V of two heads instead of all K heads or all V heads — and its epilogue got one range decision per
32-key block instead of a clamp and a compare per value.  Neither changes a single MFMA or a single stored byte, so the check is
bit equality (torch.equal on the raw words, NaN patterns included) of all six decoder outputs of every iteration, of the
workspace's range flag word and of the host's mirror words with tests/golden/kvproj_pairing.npz, recorded by
tools/make_golden_kvproj_pairing.py with the kernel as it was before.  Cases and shapes: tests/kvproj_pairing_cases.py."""
import functools
import os

import numpy as np
import pytest
import torch

import kvproj_pairing_cases as K

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", K.GOLDEN)) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize("case_id", K.case_ids())
def test_outputs_flag_and_mirror_equal_the_recording(case_id):
    want = {k[len(case_id) + 1:]: v for k, v in _golden().items() if k.startswith(case_id + "/")}
    got = K.run(case_id)
    assert sorted(got) == sorted(want) and len(want) == 2 * len(K.KEYS) + 3
    print("\n%s: flag %s, mirror max %d, state %s" % (case_id, got["flag"].tolist(), int(got["mirror"].max()), got["state"].tolist()))
    for name in ("flag", "mirror", "state"):
        assert torch.equal(_bits(got[name]), _bits(want[name])), (case_id, name, got[name], want[name])
    for name in sorted(want):
        assert got[name].shape == want[name].shape and torch.equal(_bits(got[name]), _bits(want[name])), (case_id, name)


def test_the_recording_holds_what_the_cases_are_about():
    """The range case raised the flag and the mirror in the recording and poisoned its outputs; the e4m3-range case and every plain
    case raised nothing and are finite."""
    g = _golden()
    for cid in K.case_ids():
        flagged = cid.startswith("range-")
        assert (int(g[cid + "/flag"][0]) & 1) == int(flagged), cid
        assert (int(g[cid + "/mirror"].max()) & 1) == int(flagged), cid
        assert bool(np.isnan(g[cid + "/it1.pred_logits"]).all()) == flagged, cid
