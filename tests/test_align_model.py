"""CPU checks of the pose alignment's semantics: the float64 model (tests/align_independent.py, full driver) refines perturbed poses against
the oracle's map of the small room, and rank-deficient point sets fail the pivot rule.  Nothing here needs a GPU."""
import numpy as np
import pytest

import align_independent as A
import query_independent as Q

VS = 0.05


@pytest.fixture(scope="module")
def oracle_room(oracle_mod):
    """get_blocks over the oracle's TSDF of the ten map frames (host copies, the reference's voxel order)"""
    p = oracle_mod.default_params()
    o = oracle_mod.OracleMap(p)
    for i in A.MAP_FRAMES:
        d, _, T = A.room_frame(i)
        o.integrate_depth(d, T, A.SMALL_CAM)
    blocks = {tuple(int(v) for v in idx): o.get_block(oracle_mod.L_TSDF, idx) for idx in o.block_indices(oracle_mod.L_TSDF)}

    def get_blocks(layer, idx):
        assert layer == Q.LAYER_TSDF
        out = np.zeros((len(idx), 512), [("distance", "<f4"), ("weight", "<f4")]); found = np.zeros(len(idx), bool)
        for r, k in enumerate(map(tuple, np.asarray(idx))):
            b = blocks.get(tuple(int(v) for v in k))
            if b is not None:
                out[r]["distance"] = b["distance"]; out[r]["weight"] = b["weight"]; found[r] = True
        return out, found
    return get_blocks


@pytest.mark.parametrize("frame", A.ALIGN_FRAMES)
def test_perturbed_starts_converge_to_one_fixed_point_near_the_truth(oracle_room, frame):
    d, _, T_true = A.room_frame(frame)
    x = A.backproject(d, A.SMALL_CAM, subsampling=4)
    assert 1000 <= len(x) <= 1200
    q = A.full_query(oracle_room, VS, A.DEFAULTS["min_weight"])
    ends = []
    for T0 in A.starts(frame, T_true):
        dt, ang, _ = A.pose_distance(T0, T_true)
        assert abs(dt - 0.03) < 1e-4 and abs(np.rad2deg(ang) - 1.5) < 1e-2
        r = A.run(q, x, T0)
        assert r["status"] == A.CONVERGED and r["iterations"] <= 10, (r["status"], r["iterations"])
        assert r["last"]["cost"] < r["first"]["cost"]
        ends.append(r["T"])
        dt, ang, _ = A.pose_distance(r["T"], T_true)
        print("frame %d: %d iterations, n_valid %d, %.4f m %.3f deg from the truth, cond(H) %.1f" % (
            frame, r["iterations"], r["n_valid"], dt, np.rad2deg(ang), np.linalg.cond(r["last"]["H"])))
        assert dt <= 0.05 and np.rad2deg(ang) <= 0.5, (dt, np.rad2deg(ang))        # one voxel, half a degree
    for T in ends[1:]:
        dt, _, dr = A.pose_distance(T, ends[0])
        assert dt <= 1e-4 and dr <= 1e-4, (dt, dr)


@pytest.mark.parametrize("count", [3, 5])
def test_rank_deficient_point_sets_fail_the_pivot_rule(oracle_room, count):
    """3 points give at most rank 3, 5 points rank 5: a 6 x 6 system of either has a failing pivot under the default ratio"""
    d, _, T_true = A.room_frame(10)
    x = A.backproject(d, A.SMALL_CAM, subsampling=4)
    q = A.full_query(oracle_room, VS, A.DEFAULTS["min_weight"])
    Tf = np.asarray(T_true, np.float32)
    p = A.apply_rt_f32(Tf[:3, :3], Tf[:3, 3], x)
    valid = q(p)[2]
    pick = np.nonzero(valid)[0][np.linspace(0, valid.sum() - 1, count).astype(int)]
    r = A.run(q, x[pick], T_true, dict(min_valid=1))
    assert r["n_valid"] == count and r["status"] == A.DEGENERATE and r["iterations"] == 1
    assert np.array_equal(r["T"], np.asarray(T_true, np.float32).astype(np.float64))
    xi, ratio = A.solve(r["last"]["H"], r["last"]["b"])
    assert xi is None and ratio <= 1e-9, ratio
    full = A.run(q, x, T_true, dict(min_valid=1), linearize_only=True)
    assert full["status"] == A.LINEARIZED and A.solve(full["last"]["H"], full["last"]["b"])[1] >= 0.01


def test_too_few_points_apply_no_step(oracle_room):
    d, _, T_true = A.room_frame(10)
    x = A.backproject(d, A.SMALL_CAM, subsampling=4)[:20]
    r = A.run(A.full_query(oracle_room, VS, 1e-4), x, T_true)
    assert r["status"] == A.TOO_FEW and r["iterations"] == 1 and np.array_equal(r["T"], np.asarray(T_true, np.float64))
    r = A.run(A.full_query(oracle_room, VS, 1e-4), np.zeros((0, 3), np.float32), T_true)
    assert r["status"] == A.TOO_FEW and r["n_valid"] == 0
