"""Records tests/golden/kvproj_pairing.npz: what the project's own decoder returns for the cases of tests/kvproj_pairing_cases.py
(outputs of every iteration, range flag word, mirror words) on the GPU, with the library built from the checkout this script runs in.
It was run at the commit before kvproj_dma_kernel's column slices were rebalanced and its epilogue got one range decision per
block; tests/test_gpu_kvproj_pairing.py compares later builds with that recording bit for bit.

    python tools/make_golden_kvproj_pairing.py [output.npz]

Run it from another checkout with that checkout's library built, and pass the path of the file to write."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kvproj_pairing_cases as K          # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", K.GOLDEN)
    # the range cases rest on these magnitudes (float64, CPU): checked before anything is recorded
    for scale, want in ((100.0, "head 1 beyond 60000, the others inside"), (1.0, "beyond 448, inside 60000")):
        k = np.abs(K.k_of_row(K.model(scale)[1], K.range_scene(1000.0), 70)).max(axis=1)
        print("K of the scaled row, max |.| per head (K rows of head 1 x %g): %s  [%s]" % (scale, np.round(k, 1), want))
        if scale == 100.0:
            assert k[1] > 1e5 and (np.delete(k, 1) < 3e4).all(), k
        else:
            assert (k > 900).any() and (k < 3e4).all(), k
    assert np.abs(K.range_scene(1000.0)["tokens"]).max() < 3e4
    blob = {}
    for cid in K.case_ids():
        rec = K.run(cid)
        print("%-24s flag %s mirror max %d state %s finite %s" % (cid, rec["flag"].tolist(), int(rec["mirror"].max()), rec["state"].tolist(),
                                                                  bool(np.isfinite(rec["it1.pred_logits"]).all())))
        for name, a in rec.items():
            blob[cid + "/" + name] = a
    np.savez_compressed(out, **blob)
    print("wrote %s: %d arrays, %d bytes" % (out, len(blob), os.path.getsize(out)))


if __name__ == "__main__":
    main()
