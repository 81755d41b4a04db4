"""The float64 model of the alignment with a colour term (tests/align_color_independent.py) on the drawn wall, without a GPU: a flat textured
plane lets the geometric system slide in three of its six directions, and the colour term pins them.  The bounds are ten times what the model
gave when the feature was specified (1e-4 m after 3 to 5 iterations, cond(H) 308 at color_weight 1 and 81 at 4)."""
import numpy as np
import pytest

import align_color_independent as AC
import align_independent as A

MIN_WEIGHT = A.DEFAULTS["min_weight"]


@pytest.fixture(scope="module")
def wall():
    m = AC.wall_map()
    x, rgb, T = AC.wall_cloud()
    assert len(x) == 1200
    return dict(q=A.full_query(m.get_blocks, AC.WALL_VS, MIN_WEIGHT), cq=AC.full_color_query(m.get_blocks, AC.WALL_VS, 1e-4), x=x, rgb=rgb, T=T,
                starts=AC.wall_starts(T))


def test_the_wall_alone_is_degenerate(wall):
    for T0 in wall["starts"]:
        r = AC.run(wall["q"], None, wall["x"], wall["rgb"], T0, AC.WALL_VS)
        assert (r["status"], r["iterations"]) == (A.DEGENERATE, 1) and r["n_valid"] == 1200 and r["n_color"] == 0
        assert np.array_equal(r["T"], np.asarray(T0, np.float64))


@pytest.mark.parametrize("color_weight", [1.0, 4.0])
def test_the_colour_term_pins_the_pose_on_the_wall(wall, color_weight):
    for k, T0 in enumerate(wall["starts"]):
        r = AC.run(wall["q"], wall["cq"], wall["x"], wall["rgb"], T0, AC.WALL_VS, copts=dict(color_weight=color_weight))
        dt, ang, _ = A.pose_distance(r["T"], wall["T"])
        H = r["first"]["H"]
        print("start %d, weight %g: status %d after %d, %.3g m %.3g deg from the truth, cond(H) %.4g, n_color %d" % (
            k, color_weight, r["status"], r["iterations"], dt, np.rad2deg(ang), np.linalg.cond(H), r["n_color"]))
        assert r["status"] == A.CONVERGED and r["iterations"] <= 6, (k, r["status"], r["iterations"])
        assert dt <= 1e-3 and np.rad2deg(ang) <= 0.05, (k, dt, np.rad2deg(ang))
        assert r["n_color"] == r["n_valid"] == 1200


def test_a_grey_wall_stays_degenerate():
    m = AC.wall_map(grey=True)
    x, rgb, T = AC.wall_cloud(grey=True)
    q = A.full_query(m.get_blocks, AC.WALL_VS, MIN_WEIGHT); cq = AC.full_color_query(m.get_blocks, AC.WALL_VS, 1e-4)
    for T0 in AC.wall_starts(T):
        r = AC.run(q, cq, x, rgb, T0, AC.WALL_VS, copts=dict(color_weight=1.0))
        assert (r["status"], r["iterations"]) == (A.DEGENERATE, 1) and r["n_color"] == 1200
