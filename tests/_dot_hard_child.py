"""Test program (GPU box): the hard rows of tests/_dot_cases.py through ONE forced instantiation of scan_kernel (``VQ_SCAN_LEAN`` is
read once per process: 0 streaming, 1 lean) for one storage type, at D = 1024 and the shapes 1 x 1, 2 x 3 and 2 x 5, every group of
the table, plain and masked, full scan and row view (tests/_dot_hard_run.py).  tests/test_dot_hard_gpu.py starts one of these at
a time.  Prints one line per (shape, group) with the worst |err| / bound per family, and ``ok``."""
import os
import sys

lean, dtype_name = sys.argv[1], sys.argv[2]
os.environ["VQ_SCAN_LEAN"] = lean
os.environ.setdefault("VQ_NO_TORCH", "1")

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import video_query_algorithms_amd as vqa
import _dot_cases as dc
from _dot_hard_run import SCAN_SHAPES, cell_line, one_query_path

if __name__ == "__main__":
    for s, e in SCAN_SHAPES:
        for group in dc.GROUPS:
            visit = one_query_path(vqa, dc.table(group, dtype_name, s, e, 1024))
            assert visit.scans == 4 and set(visit.worst) == set(dc.GROUP_FAMILIES[group])
            print("%s lean=%s %s %s" % (cell_line(s, e, group), lean, dtype_name, visit.line()), flush=True)
    print("ok", flush=True)
