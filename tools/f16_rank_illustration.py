"""What float16 storage does to a real query (CPU only, the oracle's arithmetic): the reference's shipped features
(tests/golden/reference_features, 87 clips of DowntownBrooklynDrive_480p x 2 streams x 3 splits), its default query -- reference
clip 10, weights rgb 1.0 / warped_optical_flow 1.5, threshold 0.8 -- scored once on the fp64 values and once on the values rounded to
binary16.  Prints the figures quoted in DESIGN.md 3; they illustrate, they are no test threshold."""
import lzma
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import sim_oracle as so
from video_query_algorithms_amd.feature_store import open_store, store_from_csv_tree, to_float16

REF_CLIP, WEIGHTS, THRESHOLD = 10, [1.0, 1.5], 0.8


def main():
    src = os.path.join(ROOT, "tests", "golden", "reference_features", "stock-video-clips_features")
    with tempfile.TemporaryDirectory() as tmp:
        for dirpath, _dirs, files in os.walk(src):
            for fn in files:
                if fn.endswith(".xz"):
                    out = os.path.join(tmp, "tree", os.path.relpath(os.path.join(dirpath, fn[:-3]), src))
                    os.makedirs(os.path.dirname(out), exist_ok=True)
                    with lzma.open(os.path.join(dirpath, fn)) as f, open(out, "wb") as g:
                        g.write(f.read())
        _meta, feats, ids, present = open_store(store_from_csv_tree(os.path.join(tmp, "tree"), os.path.join(tmp, "store"), dtype=np.float64))
        x64 = np.array(feats)
    assert present is None
    x16 = to_float16(x64).astype(np.float64)
    row = int(np.flatnonzero(ids == REF_CLIP)[0])
    normal = x64 >= 2.0 ** -14                                              # below: subnormal halves, absolute error <= 2^-25
    rel = np.abs(x16 - x64)[normal] / x64[normal]
    print("%d clips x %d streams x %d splits x %d; values in [%g, %g], %.2f %% zeros, %.4f %% non-zero below 2^-14 (largest absolute error "
          "there %.3g, 2^-25 = %.3g); largest relative rounding error of the others %.3g (2^-11 = %.3g)"
          % (x64.shape + (x64.min(), x64.max(), 100.0 * (x64 == 0).mean(), 100.0 * ((x64 != 0) & ~normal).mean(),
                          np.abs(x16 - x64)[~normal].max(), 2.0 ** -25, rel.max(), 2.0 ** -11)))
    for name, query_from in (("query from the fp64 values", x64), ("query from the stored halves", x16)):
        t = np.stack([[so.scale_feature(query_from[row, s, e]) for e in range(x64.shape[2])] for s in range(x64.shape[1])])
        sc = {}
        for kind, x in (("fp64", x64), ("fp16", x16)):
            _, avg, _ = so.dense_similarities(x, t)
            sc[kind] = (avg, so.dense_scores(avg, WEIGHTS))
        d_avg = np.abs(sc["fp16"][0] - sc["fp64"][0])
        d_sc = np.abs(sc["fp16"][1] - sc["fp64"][1])
        r64, r16 = so.dense_topk(sc["fp64"][1], 50)[0], so.dense_topk(sc["fp16"][1], 50)[0]
        m64, m16 = set(np.flatnonzero(sc["fp64"][1] >= THRESHOLD)), set(np.flatnonzero(sc["fp16"][1] >= THRESHOLD))
        gaps = -np.diff(np.sort(sc["fp64"][1])[::-1][:50])
        print("%s: max |d avg similarity| %.3g (max relative %.3g), max |d score| %.3g; top-10 ranks that differ %d, top-50 %d; "
              "matches at %.1f: %d / %d, sets %s; smallest gap between neighbours of the fp64 top-50 %.3g"
              % (name, d_avg.max(), (d_avg / np.abs(sc["fp64"][0])).max(), d_sc.max(), int((r64[:10] != r16[:10]).sum()), int((r64 != r16).sum()),
                 THRESHOLD, len(m64), len(m16), "equal" if m64 == m16 else "differ by %d" % len(m64 ^ m16), gaps.min()))


if __name__ == "__main__":
    main()
