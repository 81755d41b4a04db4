"""The independent model of rendering (tests/render_independent.py) against the CPU oracle's synthetic depth, at poses that were never
integrated and at three subsamplings.  No GPU."""
import numpy as np
import pytest

import render_cases as RC
import render_independent as R


@pytest.fixture(scope="module")
def oracle_and_volume():
    o = RC.oracle_map()
    return o, RC.oracle_volume(o, 1, RC.TSDF_FIELDS)      # (the TSDF is not written by the colour calls below: one volume serves all cases)


@pytest.mark.parametrize("s", RC.SUBSAMPLINGS)
@pytest.mark.parametrize("pose", sorted(RC.NOVEL_POSES))
def test_model_depth_equals_the_oracle(oracle_and_volume, pose, s):
    o, vol = oracle_and_volume
    T = RC.NOVEL_POSES[pose]
    ref = RC.oracle_depth_at(o, T, s)
    depth, hit = R.render_depth(vol, T, RC.CAM, s, **RC.march_params(o.params))
    assert depth.shape == ref.shape == (RC.CAM[5] // s, RC.CAM[4] // s)
    assert np.array_equal(hit, ref > 0), (pose, s, int((hit != (ref > 0)).sum()))
    diff = float(np.abs(depth - ref).max())
    # IEEE f32 on both sides in the same order: 0 is expected; 1e-4 is the project's TSDF tolerance
    assert diff <= 1e-4, "max |depth difference| = %g (pose %s, subsampling %d)" % (diff, pose, s)
    if pose == "out":
        assert not hit.any()                                # nothing was ever observed that way
    else:
        assert hit.mean() > 0.3, hit.mean()


def test_the_tsdf_is_untouched_by_the_oracle_colour_calls(oracle_and_volume):
    o, vol = oracle_and_volume
    again = RC.oracle_volume(o, 1, RC.TSDF_FIELDS)
    assert np.array_equal(again.keys, vol.keys)
    for f in RC.TSDF_FIELDS:
        assert again.data[f].tobytes() == vol.data[f].tobytes()
