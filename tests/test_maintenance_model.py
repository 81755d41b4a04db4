"""The model of decay and clearing (tests/maintenance_independent.py) and the drawn maps (tests/maintenance_cases.py) against the CPU checker, without
a GPU: block sets, every voxel and the cleared list after every call of cases A to D; that no case is vacuous, from the model alone; and the truth
the ESDF is held to after a deallocation (marks == the marking rule on the map's own TSDF, distances and parents == the brute force over that site
set), on the checker.  tests/test_gpu_maintenance_drawn.py puts the product through the same."""
import numpy as np
import pytest

import maintenance_cases as MC
import maintenance_independent as MM


def _M():
    from isaac_ros_nvblox_amd import mapper as M
    return M


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_case_is_not_vacuous_by_the_model_alone(name):
    case = MC.case_by_name(name)
    case.verify(MC.model_trace(case, MC.params(_M(), case)))


@pytest.mark.parametrize("name", MC.CASE_NAMES)
def test_model_equals_the_checker_on_the_drawn_cases(oracle_mod, name):
    case = MC.case_by_name(name)
    side = MC.CheckerSide(oracle_mod, MC.params(_M(), case))
    seen = {}

    def hook(state, before, cleared, read):
        seen["esdf"] = max(seen.get("esdf", 0), len(MM.layer_keys(before, "esdf")))
        seen["esdf_gone"] = seen.get("esdf_gone", 0) + len(set(MM.layer_keys(before, "esdf")) - set(MM.layer_keys(state, "esdf")))
    MC.run_case(case, side, after_hook=hook)
    if name[0] in "ABC":
        assert seen["esdf"] >= 20, "the update before the calls made ESDF blocks"
    if name[0] == "C":
        assert seen["esdf_gone"] >= 20, "there are ESDF blocks outside the radius"


def test_threshold_weights_are_found_by_stepping():
    for f, thr, _, _ in MC.DECAY_RUNS.values():
        exact, below = MC.threshold_weights(f, thr)
        assert all(np.float32(w * np.float32(f)) == np.float32(thr) for w in exact) and np.float32(below * np.float32(f)) < np.float32(thr)
        assert np.nextafter(below, np.float32(np.inf)) == exact[0]


@pytest.mark.parametrize("dims,r,op", [(2, r, op) for r in (2.5, 9) for op in MC.ESDF_OPS_2D] + [(2, 57, "radius_drops_esdf")] +
                         [(3, r, op) for r in (2.5, 8) for op in MC.ESDF_OPS_3D], ids=str)
def test_esdf_truth_after_deallocation_on_the_checker(oracle_mod, dims, r, op):
    """Operation 4 ("radius_drops_upper_tsdf") is the one radius clearing used to get wrong: the surviving ESDF block kept a site that no TSDF voxel
    backed any more (1 site at distance 0 where the column rule gives none)."""
    scene = MC.esdf_scene(_M(), op, r, dims)
    MC.run_esdf_scene(scene, MC.CheckerSide(oracle_mod, scene.params))


def test_radius_clearing_of_the_upper_row_with_neighbours_left(oracle_mod):
    """operation 4 again with a radius that leaves 3 x 3 columns of the lower row: the re-marked column's neighbours lose their parents too"""
    scene = MC.esdf_scene(_M(), "radius_drops_upper_tsdf", 9, 2, clear_radius_m=0.9)
    esdf = MC.run_esdf_scene(scene, MC.CheckerSide(oracle_mod, scene.params))
    assert len(esdf[0]) == 9
