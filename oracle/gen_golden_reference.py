"""Record the reference's shipped data files that the CPU tests read, as fixtures under tests/golden/.

    python oracle/gen_golden_reference.py <reference checkout>

* tests/golden/reference_features/: feature CSVs of the reference's data/features tree (xz-compressed, byte-exact inside): the whole
  stock-video-clips tree (87 clips x 2 streams x 3 splits, numpy >= 1.14 number format) and one SHRP2 file written with the
  numpy < 1.14 '%.12g' rule.
* tests/golden/reference_prototxt.json: the two deploy prototxts of the reference as this package parses them
  (tsn.bn_inception.load_prototxt), pinned by a sha256 of the parsed layer list and the input shape -- nothing of the files
  themselves is kept.  TEST INFRASTRUCTURE ONLY."""
import dataclasses
import hashlib
import json
import lzma
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FEATURES = ["stock-video-clips_features/DowntownBrooklynDrive_480p/UCF101_split%d/%s_global_pool_features.csv" % (s, m)
            for s in (1, 2, 3) for m in ("rgb", "warped_optical_flow")]
FEATURES.append("SHRP2_Forward_clips_features/S06NDS_Sample_120406_1451_00186_Forward/UCF101_split2/warped_optical_flow_global_pool_features.csv")
PROTOTXT = "src/features_GPU_compute/models/ucf101/tsn_bn_inception_%s_deploy.prototxt"


def layers_digest(layers):
    """sha256 of a layer list (tsn.bn_inception.Layer) in a canonical JSON form."""
    text = json.dumps([dataclasses.asdict(layer) for layer in layers], sort_keys=True, separators=(",", ":"))
    return hashlib.sha256(text.encode()).hexdigest()


def main(ref):
    for rel in FEATURES:
        dst = os.path.join(GOLDEN, "reference_features", rel + ".xz")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(os.path.join(ref, "data", "features", rel), "rb") as f, lzma.open(dst, "wb", preset=9 | lzma.PRESET_EXTREME) as g:
            g.write(f.read())
    sys.path.insert(0, ROOT)
    from video_query_algorithms_amd.tsn import bn_inception as bi
    rec = {}
    for name in ("rgb", "flow"):
        g = bi.load_prototxt(os.path.join(ref, PROTOTXT % name))
        rec[name] = {"layers": len(g.layers), "layers_sha256": layers_digest(g.layers), "input_shape": list(g.input_shape)}
    with open(os.path.join(GOLDEN, "reference_prototxt.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
