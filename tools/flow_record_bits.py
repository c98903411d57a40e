"""Record what a build of the library gives on the cases of tests/_flow_bits_cases.py, as sha256 hashes and integer counts:
    VQ_AMD_LIB=<library> python tools/flow_record_bits.py <out directory> [--case A] [--no-cuts]
writes <out>/parent_bits.json (the hashes) and <out>/tile_cuts.json (Tvl1Flow.tile_cuts for 1..32 pairs on seven shapes, with the slot
count -- 2 x compute units -- it was recorded at).  Run it TWICE against a build of the commit whose bits are to be pinned and commit the
files under tests/golden/flow_plan/ only if the two runs agree.  --case runs one case alone (for a kernel trace) and writes nothing
unless an out directory is given."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import _flow_bits_cases as bc
    from video_query_algorithms_amd.tsn import flow
    args = sys.argv[1:]
    only = args[args.index("--case") + 1] if "--case" in args else None
    out_dir = args[0] if args and not args[0].startswith("--") else None
    bits = {name: bc.record(run(flow)) for name, run in bc.CASES.items() if only in (None, name)}
    for name, rec in bits.items():
        print(name, {k: v["sha256"][:12] for k, v in rec.items()})
    if out_dir is None:
        return 0
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "parent_bits.json"), "w") as f:
        json.dump(bits, f, indent=1, sort_keys=True)
    if "--no-cuts" not in args and only is None:
        import torch
        slots = 2 * torch.cuda.get_device_properties(0).multi_processor_count
        with open(os.path.join(out_dir, "tile_cuts.json"), "w") as f:
            json.dump({"slots": slots, "shapes": bc.tile_cuts(flow)}, f, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
