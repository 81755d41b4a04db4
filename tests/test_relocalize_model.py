"""CPU checks of the relocalisation's semantics on the numpy model (tests/relocalize_independent.py, full driver) over the oracle's map of the
small room: the selection rule on constructed records, and the conditions the GPU tests (tests/test_gpu_relocalize.py) rely on for their
lattices -- a unique winner within one step of the truth from which the alignment's model converges near the truth.  Nothing here needs a GPU."""
import numpy as np
import pytest

import align_independent as A
import query_independent as Q
import relocalize_independent as RI

VS = 0.05
TRUNC_VOX = 4.0


@pytest.fixture(scope="module")
def oracle_room(oracle_mod):
    """get_blocks over the oracle's TSDF of the ten map frames (host copies, the reference's voxel order)"""
    p = oracle_mod.default_params()
    assert abs(p.voxel_size - VS) < 1e-9 and p.truncation_distance_vox == TRUNC_VOX
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


def S(inliers, conflicts, valid=None, points=1200, res=0):
    return RI.Score(points, inliers + conflicts if valid is None else valid, inliers, conflicts, res)


def test_selection_order_on_constructed_records():
    # the key decides, not the inlier count
    assert RI.select([S(300, 200), S(150, 10), S(140, 0)]) == (RI.OK, 1)
    # equal keys: more inliers
    assert RI.select([S(100, 0), S(120, 20), S(110, 10)]) == (RI.OK, 1)
    # equal keys and inliers: the lowest index, wherever the duplicates stand
    assert RI.select([S(10, 0), S(120, 20), S(120, 20), S(120, 20)]) == (RI.OK, 1)
    assert RI.select([S(120, 20), S(10, 0), S(120, 20)]) == (RI.OK, 0)
    # the residual and the valid count take no part
    assert RI.select([S(120, 20, valid=900, res=5), S(120, 20, valid=140, res=1)]) == (RI.OK, 0)
    # an invalid pose's record (key 0) beats a negative key; and then there is no candidate
    assert RI.select([S(60, 100), RI.INVALID]) == (RI.NO_CANDIDATE, 1)
    # the inlier floor looks at the winner only
    assert RI.select([S(49, 0), S(60, 30)]) == (RI.NO_CANDIDATE, 0)
    assert RI.select([S(49, 0), S(60, 30)], min_inliers=49) == (RI.OK, 0)
    assert RI.select([S(50, 0)]) == (RI.OK, 0) and RI.select([S(0, 0)]) == (RI.NO_CANDIDATE, 0)
    assert RI.winner_is_unique([S(100, 0), S(120, 20), S(110, 10)]) and not RI.winner_is_unique([S(120, 20), S(10, 0), S(120, 20)])


def test_records_of_simple_poses(oracle_room):
    """the true pose explains the frame; a pose 30 m away sees nothing; a non-finite or out-of-range pose is marked; special points are taken
    but never valid"""
    d, _, T_true = A.room_frame(10)
    x = RI.taken_pixels(d, A.SMALL_CAM, 4)
    assert np.array_equal(x, A.backproject(d, A.SMALL_CAM, 4)) and 1000 <= len(x) <= 1200
    q = RI.full_query(oracle_room, VS, 1e-4)
    far = np.asarray(T_true, np.float32).copy(); far[0, 3] += 30.0
    nan = np.asarray(T_true, np.float32).copy(); nan[1, 1] = np.nan
    out_of_range = np.asarray(T_true, np.float32).copy(); out_of_range[2, 3] = 5e5
    true, away, bad, oor = RI.score_poses(q, x, [T_true, far, nan, out_of_range], VS, TRUNC_VOX)
    # (a pixel on a depth edge may interpolate into free space even at the truth: conflicts are rare there, not absent)
    assert true.points == len(x) and true.valid > 0.8 * len(x) and true.inliers > 0.9 * true.valid and true.conflicts <= 0.01 * true.valid
    assert true.abs_residual_q20 < true.valid * 0.02 * (1 << 20)                  # mean |d| below 2 cm
    assert away == RI.Score(len(x), 0, 0, 0, 0) and bad == RI.INVALID and oor == RI.INVALID
    special = np.array([[np.nan, 0.5, 1.0], [0.1, np.inf, 1.0], [50.0, 50.0, 50.0]], np.float32)
    s, = RI.score_poses(q, np.concatenate([x[:10], special]), [T_true], VS, TRUNC_VOX)
    assert s.points == 13 and s.valid <= 10
    # thresholds: the defaults, and what replaces them
    mw, inl, con = RI.thresholds(VS, TRUNC_VOX)
    assert (mw, inl, con) == (np.float32(1e-4), np.float32(0.05), np.float32(0.5) * (np.float32(4.0) * np.float32(0.05)))
    assert RI.thresholds(VS, TRUNC_VOX, inlier_distance_m=0.02, conflict_distance_m=-1.0)[1:] == (np.float32(0.02), con)
    tight, = RI.score_poses(q, x, [T_true], VS, TRUNC_VOX, inlier_distance_m=0.005)
    assert tight.inliers < true.inliers and tight.valid == true.valid and tight.abs_residual_q20 == true.abs_residual_q20


@pytest.mark.parametrize("frame", A.ALIGN_FRAMES)
def test_the_lattice_search_meets_the_conditions_the_gpu_tests_rely_on(oracle_room, frame):
    d, _, T_true = A.room_frame(frame)
    x = RI.taken_pixels(d, A.SMALL_CAM, 4)
    T0 = RI.lattice_centre(T_true, frame)
    dt, ang, _ = A.pose_distance(T0, T_true)
    assert abs(dt - RI.OFFSET_M) < 1e-4 and abs(np.rad2deg(ang) - RI.OFFSET_DEG) < 1e-2
    q = RI.full_query(oracle_room, VS, 1e-4)
    # a start this far off is beyond what the alignment alone recovers to the bound below: the reason for the search
    poses = RI.lattice_poses(T0, **RI.LATTICE)
    scores = RI.score_poses(q, x, poses, VS, TRUNC_VOX)
    status, h = RI.select(scores)
    print("frame %d: winner %d %s key %d" % (frame, h, scores[h], scores[h].inliers - scores[h].conflicts))
    assert status == RI.OK and RI.winner_is_unique(scores)
    assert RI.within_one_step(poses[h], T_true, **RI.LATTICE)
    r = A.run(A.full_query(oracle_room, VS, 1e-4), x, poses[h])
    dt, ang, _ = A.pose_distance(r["T"], T_true)
    print("frame %d: from the winner %d iterations, %.4f m %.3f deg from the truth" % (frame, r["iterations"], dt, np.rad2deg(ang)))
    assert r["status"] == A.CONVERGED
    assert dt <= 0.05 and np.rad2deg(ang) <= 0.5                                   # test_end_to_end_refinement_reaches_the_models_fixed_point's bound
    refined, = RI.score_poses(q, x, [r["T"].astype(np.float32)], VS, TRUNC_VOX)
    assert refined.inliers >= scores[h].inliers


def test_a_lattice_far_from_the_map_has_no_candidate(oracle_room):
    d, _, T_true = A.room_frame(10)
    x = RI.taken_pixels(d, A.SMALL_CAM, 4)
    T0 = np.asarray(T_true, np.float32).copy(); T0[0, 3] += 30.0
    scores = RI.score_poses(RI.full_query(oracle_room, VS, 1e-4), x, RI.lattice_poses(T0, **dict(RI.LATTICE, steps=(3, 3, 1, 3))), VS, TRUNC_VOX)
    assert len(scores) == 27 and RI.select(scores) == (RI.NO_CANDIDATE, 0) and all(s == RI.Score(len(x), 0, 0, 0, 0) for s in scores)
