"""GPU: every dot-product kernel of csrc/vq_sim.hip and csrc/vq_sim_batch.hip on the hard rows of tests/_dot_cases.py -- mixed signs, cancellation, storage-type
subnormals, values next to the largest finite one, 24 binades of range, signed zeros and single non-zeros at the lane, chunk and piece
boundaries, infinities and NaNs -- against the exact dot with the derived bound D 2^-53 sum|x_k t_k| (no measured constant), classes for
the non-finite rows, n_e exactly, scores bit for bit from the device's avg, a second run the same bits, row views bit for bit the full scan.
tests/test_dot_cases.py shows on the CPU that the same check tells seven wrong dots from three honest summation orders.

  * scan_kernel: tests/_dot_hard_child.py, one fresh process per (lean, dtype), one at a time;
  * scan_tiled_kernel, scan_generic_kernel, batch_fused_kernel (query_round_batch, scan_batch) and batch_view_kernel
    (query_round_batch_sets): below, in this process (tests/_dot_hard_run.py).

Every path runs plain and under a presence mask that declares every non-finite split absent: those stream means are then finite and
inside the bound; a (clip, stream) without a split stays NaN.

Worst |err| / bound per family as observed on the MI355X (1.0 is the bound, a worst case over D roundings that all go one way, so
honest kernels sit far below it at large D; float16 rows: 40-bit products, most sums exact).  ``zeros`` is 0 everywhere: one live
product, no rounding.  No kernel was outside the bound or reported a wrong class.

    path                                       signs  cancel subnormal extreme  range nonfinite
    scan_kernel, lean and streaming, 3 types   0.001   0.000     0.000   0.000  0.000     0.000
    scan_tiled_kernel 1 x 1                    0.002   0.000     0.001   0.000  0.000     0.000
    scan_tiled_kernel 2 x 5                    0.003   0.001     0.001   0.001  0.000     0.003
    scan_generic_kernel D = 4    f16           0.480   0.000     0.000   0.000  0.000     0.095
                                 f32, f64      0.493   0.000     0.000   0.288  0.303     0.266
    scan_generic_kernel D = 8    f16           0.250   0.000     0.000   0.000  0.000     0.175
                                 f32, f64      0.248   0.123     0.116   0.135  0.231     0.208
    scan_generic_kernel D = 252, 256, 260      0.005   0.001     0.001   0.002  0.002     0.004
    scan_generic_kernel D = 1024, 1028, 2048   0.001   0.000     0.000   0.000  0.000     0.000
    batched passes D = 256                     0.008   0.001     0.001   0.002  0.002     0.003
    batched passes D = 512, 768                0.007   0.001     0.001   0.000  0.001     0.003
    batched passes D = 1024, rows and tiled    0.002   0.000     0.000   0.000  0.001     0.001

The module's 48 tests took 14 s there, the slowest (a scan_kernel child process) 0.9 s.
"""
import os
import subprocess
import sys

import pytest

import _dot_cases as dc
from _dot_hard_run import SCAN_SHAPES, Visit, batched_path, cell_line, one_query_path

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TYPES = ("f16", "f32", "f64")
GENERIC = [(2, 3, D) for D in (4, 8, 252, 256, 260, 1028, 2048)] + [(3, 1, 1024), (2, 7, 1024)]      # no C_(s, e) entry at D = 1024 for the last two


@pytest.fixture(scope="module")
def vqa(gpu):
    import video_query_algorithms_amd as m
    return m


def covered(visit, scans_per_group):
    """every family of every group went through the bound, in the number of scans the path makes"""
    assert set(visit.worst) == set(dc.FAMILIES) and visit.scans == scans_per_group * len(dc.GROUPS) and max(visit.worst.values()) <= 1.0
    assert visit.classes > 0 and visit.finite > visit.classes


@pytest.mark.parametrize("lean", ["0", "1"])
@pytest.mark.parametrize("dtype_name", TYPES)
def test_scan_kernel_on_hard_rows(gpu, lean, dtype_name):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_dot_hard_child.py"), lean, dtype_name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-6000:]
    lines = r.stdout.splitlines()
    seen = set()
    for s, e in SCAN_SHAPES:                                   # no (shape, group) cell was skipped, and every family has a ratio
        for group in dc.GROUPS:
            mine = [line for line in lines if line.startswith(cell_line(s, e, group))]
            assert len(mine) == 1 and "(4 scans" in mine[0], (s, e, group)
            seen |= {f for f in dc.FAMILIES if " %s=" % f in mine[0]}
    assert seen == set(dc.FAMILIES)


@pytest.mark.parametrize("s,e", [(1, 1), (2, 5)])
def test_tiled_scan_on_hard_rows(vqa, s, e):
    """fp32, D = 1024; the view touches tiles in one clip only and leaves one out; the block reads back bit for bit in both layouts"""
    visit = Visit()
    for group in dc.GROUPS:
        tb = dc.table(group, "f32", s, e, 1024)
        visit.merge(one_query_path(vqa, tb, layout="tiled", view_rows=tb.tile_view_rows()))
    covered(visit, 4)
    print("tiled %d x %d f32: %s" % (s, e, visit.line()))


@pytest.mark.parametrize("s,e,D", GENERIC)
@pytest.mark.parametrize("dtype_name", TYPES)
def test_generic_scan_on_hard_rows(vqa, dtype_name, s, e, D):
    visit = Visit()
    for group in dc.GROUPS:
        visit.merge(one_query_path(vqa, dc.table(group, dtype_name, s, e, D)))
    covered(visit, 4)
    print("generic %d x %d D=%d %s: %s" % (s, e, D, dtype_name, visit.line()))


BATCHED = [(d, D, "rows") for d in TYPES for D in (256, 512, 768, 1024)] + [("f32", 1024, "tiled")]


@pytest.mark.parametrize("dtype_name,D,layout", BATCHED)
def test_batched_passes_on_hard_rows(vqa, dtype_name, D, layout):
    """Q in {1, 7, 16}: query_round_batch with avg, scan_batch (the round's scores bit for bit), query_round_batch_sets (bit for bit
    the round at each set's rows)"""
    visit = Visit()
    for group in dc.GROUPS:
        visit.merge(batched_path(vqa, dc.table(group, dtype_name, 2, 3, D), layout=layout))
    covered(visit, 2 * 2 * (1 + 7 + 16))                       # masks x (round, sets) x queries
    print("batched D=%d %s %s: %s" % (D, dtype_name, layout, visit.line()))
