"""CPU: Hyperparameter._pick_exact -- _pick_from with its squares written as products, the definition the device's pick
(FeatureDB.batch_round_update) is held to -- against _pick_from on a seeded table of fitted surfaces, and against a line-by-line
restatement on crafted surfaces that reach every branch."""
import logging

import numpy as np
import pytest

import _pick_cases as pc

import video_query_algorithms_amd as vqa

# The largest relative difference between _pick_from and _pick_exact this table shows (numpy 2.2.6: 122 of its 1963
# interior picks differ at all), and the bound the test holds other libm builds to: four times that.
OBSERVED = 2.72e-15
BOUND = 4 * OBSERVED


class _Warnings(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.WARNING)
        self.seen = 0

    def emit(self, record):
        self.seen += 1


def test_pick_exact_agrees_with_pick_from_on_fitted_surfaces():
    """2400 surfaces from raw_loss_surface over random labelled scores, L in 2 .. 60.  The discrete part -- the cell, whether it lies
    on the rim, whether the refinement fell back (which _pick_from only logs) -- is the same in every case; weights and threshold
    agree within BOUND = 4 x the observed 2.72e-15 relative (measured against _pick_from on this table; 0 in 94 % of the interior
    picks)."""
    hp = pc.make_hp(vqa)
    eps = pc.compute_eps()
    seen = _Warnings()
    logging.getLogger().addHandler(seen)
    worst, interior, differ = 0.0, 0, 0
    try:
        table = pc.fitted_surfaces(vqa)
        assert len(table) >= 2000 and {L for _s, L in table} == set(range(2, 61))
        for raw, L in table:
            surface = raw / L
            before = seen.seen
            weights, th = hp._pick_from(surface)
            fell_back_from = seen.seen > before
            exact, th_exact, iw, it, on_rim, fell_back = hp._pick_exact(surface)
            assert seen.seen == before + fell_back_from                   # _pick_exact itself logs nothing
            assert (iw, it) == tuple(int(v) for v in np.unravel_index(np.argmin(surface), surface.shape))
            assert on_rim == (iw in (0, 39) or it in (0, 30)) and fell_back == fell_back_from and not (on_rim and fell_back)
            assert list(weights) == list(exact) and weights[hp.streams[0]] == exact[hp.streams[0]] == 1.0
            got, want = np.array([exact[hp.streams[1]], th_exact]), np.array([weights[hp.streams[1]], th])
            if on_rim or fell_back:
                assert np.array_equal(got, want) and np.array_equal(got, [hp.weight_grid[iw], hp.threshold_grid[it] - eps])
                continue
            interior += 1
            rel = float((np.abs(got - want) / np.abs(want)).max())
            differ += rel > 0
            worst = max(worst, rel)
            assert rel <= BOUND, (rel, iw, it, L)
    finally:
        logging.getLogger().removeHandler(seen)
    print("interior picks: %d, differing: %d, largest relative difference: %.3g (bound %.3g)" % (interior, differ, worst, BOUND))
    assert interior >= 1500


@pytest.mark.parametrize("name", sorted(pc.crafted_surfaces()))
def test_pick_exact_is_the_restated_pick_on_crafted_surfaces(name):
    raw, L = pc.crafted_surfaces()[name]
    hp = pc.make_hp(vqa)
    got = pc.exact_pick(hp, raw, L)
    assert pc.same_pick(got, pc.restated_pick(hp.weight_grid, hp.threshold_grid, raw, L, pc.compute_eps())), got


def test_the_crafted_surfaces_reach_every_branch():
    hp = pc.make_hp(vqa)
    picks = {name: pc.exact_pick(hp, raw, L) for name, (raw, L) in pc.crafted_surfaces().items()}
    cells = {name: p[2:4] for name, p in picks.items()}
    assert [cells[n] for n in ("rim-north", "rim-south", "rim-west", "rim-east", "corner", "corner-00")] == \
        [(17, 30), (17, 0), (0, 12), (39, 12), (39, 30), (0, 0)] and all(picks[n][4] for n in cells if n.startswith(("rim", "corner")))
    assert cells["tie-first-wins"] == (9, 20) and cells["tie-earlier-row-wins"] == (3, 28) and cells["tie-made-by-the-division"] == (12, 4)
    assert cells["nan-first-nan-wins"] == (22, 7) and np.isnan(picks["nan-first-nan-wins"][:2]).all() and not picks["nan-first-nan-wins"][5]
    assert cells["nan-neighbour"] == (9, 21)
    assert cells["inf-cells"] == (9, 20) and np.isnan(picks["inf-cells"][1]) and not picks["inf-cells"][5]     # a NaN misfit is no fall-back
    assert picks["all-inf"][2:] == (0, 0, True, False) and picks["all-equal"][2:] == (0, 0, True, False)
    assert picks["cells-of-1e300"][2:] == (14, 14, False, True) and picks["overflowing-refinement"][5]
    assert picks["cells-of-1e300"][:2] == (hp.weight_grid[14], hp.threshold_grid[14] - pc.compute_eps())
    assert cells["tie-with-east"] == cells["tie-with-north"] == (9, 20) and not picks["tie-with-east"][4]
    assert abs(picks["tie-with-east"][0] - (hp.weight_grid[9] + hp.weight_grid[10]) / 2) < 1e-12     # the vertex lies between the two equal cells
    assert picks["interior"][2:] == (17, 12, False, False) and picks["interior"][0] != hp.weight_grid[17]
