"""Relocalisation on the GPU (nvbx_score_poses_* / nvbx_relocalize_*; SEMANTICS.md "Relocalisation") against the numpy model of
tests/relocalize_independent.py in its hybrid driver (the interpolant is Mapper.query_tsdf's, so every record must agree bit for bit), against
the calls it chains (score_poses, search_lattice, align_depth / align_points) and against itself.
The map is the smoke-sized room of tests/test_gpu_align.py: a 160 x 120 camera, poses 0, 4, .., 36, block_capacity 1 << 13."""
import ctypes as C

import numpy as np
import pytest

import align_independent as A
import helpers as H
import relocalize_independent as RI

pytestmark = pytest.mark.gpu
VS = 0.05
TRUNC_VOX = 4.0
MIN_WEIGHT = 1e-4


def _mapper(**params):
    from isaac_ros_nvblox_amd import mapper as M
    return M.Mapper(M.default_params(**params), device=0, block_capacity=1 << 13)


@pytest.fixture(scope="module")
def room(hip_lib):
    m = _mapper()
    assert m.params.truncation_distance_vox == TRUNC_VOX and abs(m.params.voxel_size - VS) < 1e-9
    for i in A.MAP_FRAMES:
        d, _, T = A.room_frame(i)
        m.integrate_depth(d, T, A.SMALL_CAM)
    m.synchronize()
    return m


@pytest.fixture(scope="module")
def frames():
    """per alignment frame: (depth, true pose, the cloud of the pixels (4 r, 4 c), the lattice's centre)"""
    out = {}
    for f in A.ALIGN_FRAMES:
        d, _, T = A.room_frame(f)
        out[f] = (d, T, RI.taken_pixels(d, A.SMALL_CAM, 4), RI.lattice_centre(T, f))
    return out


def _np(t):
    return t.cpu().numpy()


def _gpu_records(counts, residual):
    return _np(counts).copy(), _np(residual).copy()


def _as_scores(counts, residual):
    return [RI.Score(*(int(v) for v in c), int(r)) for c, r in zip(counts, residual)]


def mixed_cloud(n, frame_cloud, T_true, seed=0):
    """n sensor-frame points: of every 20, 12 from the frame's back-projection, 5 uniform in the room's box (moved into the sensor frame: most lie
    in observed free space), 1 NaN / inf row, 2 far outside the map -- interleaved, so every prefix is mixed and point 0 is a surface point"""
    rng = np.random.default_rng([seed, n])
    T = np.asarray(T_true, np.float64)
    kind = np.arange(n) % 20
    pts = np.empty((n, 3), np.float32)
    surf = kind < 12; box = (kind >= 12) & (kind < 17); bad = kind == 17; far = kind >= 18
    pts[surf] = frame_cloud[rng.integers(0, len(frame_cloud), surf.sum())]
    pl = rng.uniform([-3.0, -2.5, 0.0], [3.0, 2.5, 3.0], (box.sum(), 3))
    pts[box] = ((pl - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    special = np.array([[np.nan, 0.5, 1.0], [0.1, np.inf, 1.0], [0.2, 0.3, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    pts[bad] = special[np.arange(bad.sum()) % 4]
    pts[far] = (rng.uniform(40.0, 60.0, (far.sum(), 3)) * rng.choice([-1.0, 1.0], (far.sum(), 3))).astype(np.float32)
    return pts


def mixed_poses(K, T_true, seed=0):
    """K poses: 0 the truth; the last (K >= 2) not finite; every 7th moves every point into unmapped space, every 11th lies out of range; the others
    are drawn up to 0.4 m and 20 degrees about z off the truth"""
    rng = np.random.default_rng([seed, K])
    T_true = np.asarray(T_true, np.float32)
    out = np.empty((K, 4, 4), np.float32)
    kinds = []
    for k in range(K):
        T = T_true.astype(np.float64).copy()
        if k == 0:
            kinds.append("true")
        elif k == K - 1:
            T[rng.integers(0, 3), rng.integers(0, 4)] = [np.nan, np.inf, -np.inf][k % 3]; kinds.append("bad")
        elif k % 7 == 3:
            T[:3, 3] += rng.choice([-1.0, 1.0], 3) * 30.0; kinds.append("far")
        elif k % 11 == 5:
            T[rng.integers(0, 3), 3] = 5e5; kinds.append("bad")
        else:
            yaw = rng.uniform(-1.0, 1.0) * np.deg2rad(20.0); c, s = np.cos(yaw), np.sin(yaw)
            T[:3, :3] = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) @ T[:3, :3]
            T[:3, 3] += rng.uniform(-0.4, 0.4, 3) * [1.0, 1.0, 0.25]; kinds.append("near")
        out[k] = T.astype(np.float32)
    return out, kinds


def check_against_model(room, x, poses, kinds, **options):
    """the GPU's records equal the hybrid model's, bit for bit, twice; -> (counts, residual)"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    c1, r1 = _gpu_records(*room.score_poses(xt, poses, **options))
    c2, r2 = _gpu_records(*room.score_poses(xt, poses, **options))
    mw = RI.thresholds(VS, TRUNC_VOX, **options)[0]
    mc, mr = RI.records(RI.score_poses(RI.hybrid_query(room, mw), x, poses, VS, TRUNC_VOX, **options))
    assert c1.dtype == np.int32 and r1.dtype == np.int64 and c1.shape == (len(poses), 4) and r1.shape == (len(poses),)
    assert np.array_equal(c1, mc), np.nonzero((c1 != mc).any(1))[0][:8]
    assert np.array_equal(r1, mr), np.nonzero(r1 != mr)[0][:8]
    assert c1.tobytes() == c2.tobytes() and r1.tobytes() == r2.tobytes()          # run to run
    for k, kind in enumerate(kinds):
        if kind == "bad":
            assert tuple(c1[k]) == (-1, 0, 0, 0) and r1[k] == 0, k
        elif kind == "far":
            assert tuple(c1[k]) == (len(x), 0, 0, 0) and r1[k] == 0, k
        else:
            assert c1[k, 0] == len(x) and c1[k, 1] >= max(c1[k, 2], c1[k, 3]), k
    return c1, r1


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1200])
def test_scores_are_the_models_bit_for_bit(room, frames, n, K):
    """(n: the wavefront, the workgroup, one point more than a workgroup, and the frame's cloud split over five workgroups; K: alone, with the
    non-finite pose, around 64 and past 256.  From n = 63 on the cloud holds all four kinds of points and the truth must show it.)"""
    d_img, T_true, _, _ = frames[10]
    x = mixed_cloud(n, A.backproject(d_img, A.SMALL_CAM), T_true)
    poses, kinds = mixed_poses(K, T_true)
    c, r = check_against_model(room, x, poses, kinds)
    if n >= 63:
        pts, valid, inl, conf = (int(v) for v in c[0])
        print("n %d: the truth has %d valid, %d inliers, %d conflicts, residual %d" % (n, valid, inl, conf, r[0]))
        assert 0.2 * n <= valid <= 0.99 * n and inl >= 0.4 * n and r[0] > 0        # (12 of 20 points lie on the surface, 3 of 20 are never valid)
        assert n < 257 or conf >= 1                                               # (64 and more points inside the room: some in observed free space)
    else:
        assert tuple(c[0]) == (1, 1, 1, 0)


def test_scores_on_the_other_launch_shapes(room, frames, monkeypatch):
    """Past 1 024 chunks of 256 points a lane takes a run of consecutive points: 262 444 points are 513 chunks of two points per lane.  And the A/B
    knob's shapes -- one workgroup per pose with five points per lane and plain stores, three chunks of two points per lane -- give the same bits as
    the launch's own five chunks.  K = 2 049: more poses than any of the other cases."""
    d_img, T_true, _, _ = frames[22]
    cloud = A.backproject(d_img, A.SMALL_CAM)
    poses, kinds = mixed_poses(3, T_true, seed=1)
    check_against_model(room, mixed_cloud(262444, cloud, T_true), poses, kinds)
    x = mixed_cloud(1200, cloud, T_true)
    poses, kinds = mixed_poses(2049, T_true, seed=1)
    c0, r0 = check_against_model(room, x, poses, kinds)
    try:         # (`room` is shared: a mapper keeps the knobs it last read)
        for chunks in ("1", "3"):
            monkeypatch.setenv("NVBX_SCORE_CHUNKS", chunks)
            room.reload_knobs()
            c, r = _gpu_records(*room.score_poses(x, poses))
            assert np.array_equal(c, c0) and np.array_equal(r, r0), chunks
    finally:
        monkeypatch.undo()
        room.reload_knobs()


def test_options_replace_the_thresholds(room, frames):
    d_img, T_true, _, _ = frames[34]
    x = mixed_cloud(1200, A.backproject(d_img, A.SMALL_CAM), T_true)
    poses, kinds = mixed_poses(9, T_true, seed=2)
    base, _ = check_against_model(room, x, poses, kinds)
    for kw in (dict(inlier_distance_m=0.01), dict(conflict_distance_m=0.02), dict(min_weight=2.5), dict(inlier_distance_m=-1.0, conflict_distance_m=0.0)):
        c, _ = check_against_model(room, x, poses, kinds, **kw)
        if "min_weight" in kw:           # (half of max_weight: a voxel few of the ten frames saw stays below it)
            assert c[0, 1] < base[0, 1]
        elif kw.get("inlier_distance_m", 0) > 0:
            assert c[0, 2] <= base[0, 2] and c[0, 1] == base[0, 1] and c[0, 3] == base[0, 3]
        elif kw.get("conflict_distance_m", 0) > 0:
            assert c[0, 3] >= base[0, 3] and c[0, 1] == base[0, 1] and c[0, 2] == base[0, 2]
        else:
            assert np.array_equal(c, base)
    # preallocated records: nothing is allocated, the views are the tensor's
    import torch
    out = torch.full((9, 3), -7, dtype=torch.int64, device="cuda")
    c, r = room.score_poses(x, poses, out=out)
    assert c.data_ptr() == out.data_ptr() and r.data_ptr() == out.data_ptr() + 16 and np.array_equal(_np(c), base)
    # no poses: nothing is launched, nothing is written
    c, r = room.score_poses(x, np.zeros((0, 4, 4), np.float32))
    assert tuple(c.shape) == (0, 4) and tuple(r.shape) == (0,)
    # no points: every finite pose has an all-zero record
    c, r = room.score_poses(np.zeros((0, 3), np.float32), poses)
    assert [tuple(v) for v in _np(c)] == [(-1, 0, 0, 0) if k == "bad" else (0, 0, 0, 0) for k in kinds] and not _np(r).any()


@pytest.mark.parametrize("s", [1, 3, 4])
def test_depth_is_points(room, frames, s):
    import torch
    d_img, T_true, _, _ = frames[22]
    depth = d_img.copy()
    depth[40:60, 50:90] = 0.0                                   # a hole; and the far part of the room lies beyond max_depth_m
    max_d = 2.5
    cloud = RI.taken_pixels(depth, A.SMALL_CAM, s, max_d)
    assert np.array_equal(cloud, A.backproject(depth, A.SMALL_CAM, s, max_d))
    assert len(cloud) > 200 and (depth[::s, ::s] > np.float32(max_d)).sum() > 50 and (depth[::s, ::s] == 0).sum() > 10
    poses, kinds = mixed_poses(9, T_true, seed=3)
    cd, rd = _gpu_records(*room.score_poses(torch.from_numpy(depth).cuda(), poses, cam=A.SMALL_CAM, subsampling=s, max_depth_m=max_d))
    cp, rp = check_against_model(room, cloud, poses, kinds)
    assert np.array_equal(cd, cp) and np.array_equal(rd, rp)
    # exactly those pixels: without the limit, and without the hole, more points are taken
    assert _np(room.score_poses(depth, poses[:1], cam=A.SMALL_CAM, subsampling=s)[0])[0, 0] > cp[0, 0]
    assert _np(room.score_poses(d_img, poses[:1], cam=A.SMALL_CAM, subsampling=s, max_depth_m=max_d)[0])[0, 0] > cp[0, 0]


@pytest.mark.parametrize("frame", A.ALIGN_FRAMES)
def test_selection_and_refinement(room, frames, frame):
    """The lattice of relocalize_independent.LATTICE (5 x 5 x 1 x 9 over +-0.4 m and +-20 degrees) centred 0.3 m and 15 degrees off the truth.
    The conditions the assertions rest on -- a unique winner within one step of the truth from which the alignment's model converges -- hold
    for all three frames with these parameters; they are asserted here on the hybrid model and in tests/test_relocalize_model.py on the oracle's map."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    d_img, T_true, x, T0 = frames[frame]
    dt = torch.from_numpy(d_img).cuda()
    res = room.relocalize_depth(dt, T0, A.SMALL_CAM, scores=True, **RI.LATTICE)
    again = room.relocalize_depth(dt, T0, A.SMALL_CAM, scores=True, **RI.LATTICE)
    assert _np(res.buffer).tobytes() == _np(again.buffer).tobytes()               # run to run
    # the lattice
    poses = room.search_lattice(T0, **RI.LATTICE)
    assert poses.dtype == np.float32 and np.array_equal(poses.view(np.uint32), RI.lattice_poses(T0, **RI.LATTICE).view(np.uint32))
    # its records: the model's, and score_poses' over the same poses
    model = RI.score_poses(RI.hybrid_query(room, MIN_WEIGHT), x, poses, VS, TRUNC_VOX)
    mc, mr = RI.records(model)
    lc, lr = _gpu_records(*res.scores)
    sc, sr = _gpu_records(*room.score_poses(dt, poses, cam=A.SMALL_CAM))
    assert np.array_equal(lc, mc) and np.array_equal(lr, mr) and np.array_equal(sc, mc) and np.array_equal(sr, mr)
    assert _np(again.scores[0]).tobytes() == lc.tobytes() and _np(again.scores[1]).tobytes() == lr.tobytes()
    # the conditions, on the model
    status, h = RI.select(model)
    assert status == RI.OK and RI.winner_is_unique(model) and RI.within_one_step(poses[h], T_true, **RI.LATTICE)
    mod = A.run(A.hybrid_query(room, MIN_WEIGHT), x, poses[h])
    assert mod["status"] == A.CONVERGED
    # the selection
    assert (res.status, res.best_index) == (M.RELOC_OK, h) and tuple(res.coarse) == tuple(model[h])
    assert np.array_equal(res.T_coarse.view(np.uint32), poses[h].view(np.uint32))
    # the refinement: align_depth from T_coarse, bit for bit
    ref = room.align_depth(dt, res.T_coarse, A.SMALL_CAM)
    assert _np(res.align.buffer).tobytes() == _np(ref.buffer).tobytes()
    assert res.align.status == M.ALIGN_CONVERGED == mod["status"]
    assert np.array_equal(res.T_L_S, ref.T_L_S)
    # the refined pose's record
    rc, rr = _gpu_records(*room.score_poses(dt, res.align.T_L_S[None], cam=A.SMALL_CAM))
    assert tuple(res.refined) == tuple(int(v) for v in rc[0]) + (int(rr[0]),)
    assert res.refined.inliers >= res.coarse.inliers
    # ... is as close to the truth as test_end_to_end_refinement_reaches_the_models_fixed_point asks of align_points from inside the band
    dtr, ang, _ = A.pose_distance(res.align.T64, T_true)
    print("frame %d: hypothesis %d %s -> %d iterations, %.4f m %.3f deg from the truth, refined %s" % (
        frame, h, tuple(res.coarse), res.align.iterations, dtr, np.rad2deg(ang), tuple(res.refined)))
    assert dtr <= 0.05 and np.rad2deg(ang) <= 0.5, (frame, dtr, np.rad2deg(ang))
    # the cloud form on the same points: the same selection, align_points' refinement; without `scores` the records stay inside the library
    pt = room.relocalize_points(x, T0, **RI.LATTICE)
    assert pt.scores is None and (pt.status, pt.best_index, tuple(pt.coarse)) == (res.status, h, tuple(res.coarse))
    assert _np(pt.align.buffer).tobytes() == _np(room.align_points(x, pt.T_coarse).buffer).tobytes()
    # options reach both parts: one iteration only, and a tighter inlier distance
    one = room.relocalize_depth(dt, T0, A.SMALL_CAM, min_inliers=1, align=dict(max_iterations=1), score=dict(inlier_distance_m=0.02), **RI.LATTICE)
    m2 = RI.score_poses(RI.hybrid_query(room, MIN_WEIGHT), x, poses, VS, TRUNC_VOX, inlier_distance_m=0.02)
    assert (one.status, one.best_index) == RI.select(m2, 1) == (RI.OK, one.best_index) and tuple(one.coarse) == tuple(m2[one.best_index])
    assert one.align.iterations == 1
    assert _np(one.align.buffer).tobytes() == _np(room.align_depth(dt, one.T_coarse, A.SMALL_CAM, max_iterations=1).buffer).tobytes()


def test_no_candidate(room, frames):
    from isaac_ros_nvblox_amd import mapper as M
    d_img, T_true, x, T0 = frames[10]
    far = T0.copy(); far[0, 3] += 30.0
    import torch
    out = torch.full((M.RELOC_RESULT_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    res = room.relocalize_depth(d_img, far, A.SMALL_CAM, scores=True, out=out, **RI.LATTICE)
    assert res.buffer.data_ptr() == out.data_ptr()
    K = int(np.prod(RI.LATTICE["steps"]))
    assert (res.status, res.best_index) == (M.RELOC_NO_CANDIDATE, 0) and tuple(res.coarse) == (len(x), 0, 0, 0, 0)
    assert np.array_equal(res.T_coarse.view(np.uint32), RI.lattice_poses(far, **RI.LATTICE)[0].view(np.uint32))
    assert res.align.iterations == 0 and res.align.status == 0 and tuple(res.refined) == (0, 0, 0, 0, 0)
    assert not _np(res.align.buffer).any()                                          # the whole alignment record is zero
    c, r = _gpu_records(*res.scores)
    assert c.shape == (K, 4) and (c == [len(x), 0, 0, 0]).all() and not r.any()
    # the inlier floor: the search that succeeds with the default fails with a floor above its winner's inliers, and says which hypothesis that was
    ok = room.relocalize_depth(d_img, T0, A.SMALL_CAM, **RI.LATTICE)
    hi = room.relocalize_depth(d_img, T0, A.SMALL_CAM, min_inliers=ok.coarse.inliers + 1, **RI.LATTICE)
    assert ok.status == M.RELOC_OK and (hi.status, hi.best_index, tuple(hi.coarse)) == (M.RELOC_NO_CANDIDATE, ok.best_index, tuple(ok.coarse))
    assert hi.align.iterations == 0 and tuple(hi.refined) == (0, 0, 0, 0, 0)
    at = room.relocalize_depth(d_img, T0, A.SMALL_CAM, min_inliers=ok.coarse.inliers, **RI.LATTICE)
    assert _np(at.buffer).tobytes() == _np(ok.buffer).tobytes()
    # the mapper's alignment state is its own again afterwards
    st = A.starts(10, T_true)[0]
    assert room.align_points(x, st).status == M.ALIGN_CONVERGED


def test_ties_go_to_more_inliers_then_to_the_lowest_index(room, frames):
    from isaac_ros_nvblox_amd import mapper as M
    d_img, T_true, x, T0 = frames[22]
    near, _ = mixed_poses(6, T_true, seed=4)
    a, b, c = np.asarray(T_true, np.float32), near[1], near[2]
    poses = np.stack([b, a, c, a, b, a])
    cnt, res = _gpu_records(*room.score_poses(x, poses))
    recs = _as_scores(cnt, res)
    assert recs[1] == recs[3] == recs[5] and recs[0] == recs[4] and recs[1] != recs[0]
    assert RI.select(recs) == (RI.OK, 1) and not RI.winner_is_unique(recs)
    assert RI.select(recs[::-1]) == (RI.OK, 0)
    # on the device: a lattice without extent is K times one pose -- the first wins; with the yaw axis alone spread, the centre does
    flat = room.relocalize_points(x, a, 0.0, 0.0, (3, 3, 1, 3), scores=True)
    fc, fr = _gpu_records(*flat.scores)
    assert (fc == fc[0]).all() and (fr == fr[0]).all() and (flat.status, flat.best_index) == (M.RELOC_OK, 0)
    yaw = room.relocalize_points(x, a, 0.0, float(np.deg2rad(10.0)), (3, 3, 1, 3), scores=True)
    yc, yr = _gpu_records(*yaw.scores)
    assert RI.select(_as_scores(yc, yr)) == (RI.OK, yaw.best_index) and yaw.best_index == 1          # (ix, iy, iz, iw) = (0, 0, 0, 1): the first of nine copies


def test_refusals_launch_nothing_and_leave_the_mapper_usable(room, frames):
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M
    d_img, T_true, x, T0 = frames[34]
    poses, kinds = mixed_poses(5, T_true, seed=5)
    before = _gpu_records(*room.score_poses(x, poses))
    nan = float("nan")
    rec = torch.full((5, 3), -7, dtype=torch.int64, device="cuda")
    buf = torch.full((M.RELOC_RESULT_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    lat = torch.full((int(np.prod(RI.LATTICE["steps"])), 3), -7, dtype=torch.int64, device="cuda")
    L = RI.LATTICE
    bad_T0 = T0.copy(); bad_T0[2, 3] = np.inf
    far_T0 = T0.copy(); far_T0[0, 3] = 5e5
    calls = [lambda kw=kw: room.score_poses(x, poses, out=rec, **kw) for kw in (
        dict(subsampling=0), dict(min_weight=nan), dict(inlier_distance_m=nan), dict(conflict_distance_m=nan), dict(max_depth_m=nan))]
    calls += [lambda: room.score_poses(d_img, poses, cam=(80.0, 80.0, 79.5, 59.5, 161, 120), out=rec),
              lambda: room.score_poses(d_img, poses, cam=A.SMALL_CAM, subsampling=-1, out=rec)]
    calls += [lambda kw=kw: room.relocalize_depth(d_img, T0, A.SMALL_CAM, scores="steps" not in kw and lat, out=buf, **dict(L, **kw)) for kw in (
        dict(steps=(0, 5, 1, 9)), dict(steps=(5, 65, 1, 9)), dict(steps=(64, 64, 64, 8)), dict(half_extent_m=(0.4, -0.1, 0.0)),
        dict(half_extent_m=(0.4, nan, 0.0)), dict(half_yaw_rad=float("inf")), dict(half_yaw_rad=-0.1))]
    calls += [lambda: room.relocalize_depth(d_img, bad_T0, A.SMALL_CAM, scores=lat, out=buf, **L),
              lambda: room.relocalize_points(x, far_T0, scores=lat, out=buf, **L),
              lambda: room.relocalize_depth(d_img, T0, (80.0, 80.0, 79.5, 59.5, 160, 121), scores=lat, out=buf, **L)]
    calls += [lambda kw=kw: room.relocalize_points(x, T0, scores=lat, out=buf, score=kw, **L) for kw in (dict(subsampling=0), dict(min_weight=nan))]
    calls += [lambda kw=kw: room.relocalize_points(x, T0, scores=lat, out=buf, align=kw, **L) for kw in (
        dict(max_iterations=0), dict(max_iterations=65), dict(min_valid=0), dict(damping=-1.0), dict(stop_translation_m=nan), dict(huber_delta_m=nan))]
    calls += [lambda: room.relocalize_depth(d_img, T0, A.SMALL_CAM, scores=lat, out=buf, align=dict(subsampling=0), **L)]
    for k, call in enumerate(calls):
        with pytest.raises(M.NvbxError):
            call()
        assert b"nvbx_" in room.lib.nvbx_last_error(), k
    # the raw entry points: NULL and misaligned pointers, negative counts
    xt = torch.from_numpy(x).cuda(); pt = torch.from_numpy(poses.reshape(-1, 16)).cuda(); dd = torch.from_numpy(d_img).cuda()
    px, pp, pd, pr, pb, pl = (C.c_void_p(t.data_ptr()) for t in (xt, pt, dd, rec, buf, lat))
    lib, h = room.lib, room._h
    cam = M.Camera(80.0, 80.0, 79.5, 59.5, 160, 120)
    T0c = np.ascontiguousarray(T0); pT = T0c.ctypes.data_as(C.c_void_p)
    sl = room._lattice(L["half_extent_m"], L["half_yaw_rad"], L["steps"]); psl = C.byref(sl)
    n = len(x)
    rcs = [lib.nvbx_score_poses_points(h, None, n, pp, 5, None, pr), lib.nvbx_score_poses_points(h, px, -1, pp, 5, None, pr),
           lib.nvbx_score_poses_points(h, px, n, None, 5, None, pr), lib.nvbx_score_poses_points(h, px, n, pp, -1, None, pr),
           lib.nvbx_score_poses_points(h, px, n, pp, 5, None, None), lib.nvbx_score_poses_points(h, px, n, pp, 5, None, C.c_void_p(rec.data_ptr() + 4)),
           lib.nvbx_score_poses_depth(h, None, 120, 160, C.byref(cam), pp, 5, None, pr), lib.nvbx_score_poses_depth(h, pd, 120, 160, None, pp, 5, None, pr),
           lib.nvbx_score_poses_depth(h, pd, 0, 160, C.byref(cam), pp, 5, None, pr), lib.nvbx_score_poses_depth(h, pd, 120, 160, C.byref(cam), None, 5, None, pr),
           lib.nvbx_relocalize_points(h, None, n, pT, psl, None, 0, None, pl, pb), lib.nvbx_relocalize_points(h, px, -1, pT, psl, None, 0, None, pl, pb),
           lib.nvbx_relocalize_points(h, px, n, None, psl, None, 0, None, pl, pb), lib.nvbx_relocalize_points(h, px, n, pT, None, None, 0, None, pl, pb),
           lib.nvbx_relocalize_points(h, px, n, pT, psl, None, 0, None, pl, None),
           lib.nvbx_relocalize_points(h, px, n, pT, psl, None, 0, None, pl, C.c_void_p(buf.data_ptr() + 4)),
           lib.nvbx_relocalize_points(h, px, n, pT, psl, None, 0, None, C.c_void_p(lat.data_ptr() + 4), pb),
           lib.nvbx_relocalize_depth(h, None, 120, 160, C.byref(cam), pT, psl, None, 0, None, pl, pb),
           lib.nvbx_relocalize_depth(h, pd, 120, 160, None, pT, psl, None, 0, None, pl, pb),
           lib.nvbx_relocalize_depth(h, pd, 120, 0, C.byref(cam), pT, psl, None, 0, None, pl, pb)]
    assert rcs == [-1] * len(rcs), rcs
    room.synchronize()
    # nothing was launched: no output changed
    assert (_np(rec) == -7).all() and (_np(lat) == -7).all() and (_np(buf) == 0xAB).all()
    # an occupancy mapper has no TSDF
    occ = _mapper(projective_layer_type=1)
    for call in (lambda: occ.score_poses(x, poses), lambda: occ.score_poses(d_img, poses, cam=A.SMALL_CAM),
                 lambda: occ.relocalize_points(x, T0, **L), lambda: occ.relocalize_depth(d_img, T0, A.SMALL_CAM, **L)):
        with pytest.raises(M.NvbxError):
            call()
    occ.integrate_depth(d_img, T_true, A.SMALL_CAM); occ.synchronize()
    assert occ.num_blocks(M.LAYER_OCCUPANCY) > 0                                  # the refused mapper stays usable
    # ... and so does the room's; options NULL are the defaults
    assert lib.nvbx_score_poses_points(h, px, n, pp, 5, None, pr) == 0
    room.synchronize()
    after = _gpu_records(*room.score_poses(x, poses))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(_np(rec.view(torch.int32).reshape(5, 6)[:, :4]), before[0]) and np.array_equal(_np(rec[:, 2]), before[1])
    # wrapper-side refusals: shapes and dtypes of poses and preallocated outputs
    for call in (lambda: room.score_poses(x, np.zeros((3, 5), np.float32)), lambda: room.score_poses(x, torch.zeros((2, 4, 4), dtype=torch.float64)),
                 lambda: room.score_poses(x, poses, out=torch.zeros((5, 4), dtype=torch.int64, device="cuda")),
                 lambda: room.score_poses(x, poses, out=torch.zeros((5, 3), dtype=torch.int32, device="cuda")),
                 lambda: room.relocalize_points(x, T0, out=torch.zeros(100, dtype=torch.uint8, device="cuda"), **L),
                 lambda: room.relocalize_points(x, T0, scores=torch.zeros((7, 3), dtype=torch.int64, device="cuda"), **L),
                 lambda: room.relocalize_points(x, T0, 0.1, 0.1, (1, 1, 1))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        room.score_poses(x, poses, no_such_option=1)


def test_relocalisation_leaves_the_map_and_held_back_work_alone(frames):
    """under colour deferral a colour frame and an updateEsdf are held back when the four calls run between two depth frames: the final layers are
    bit-identical to the same sequence without them"""
    d10, T_true, x, T0 = frames[10]
    poses = RI.lattice_poses(T0, **dict(RI.LATTICE, steps=(3, 3, 1, 3)))

    def sequence(relocalize):
        m = _mapper()
        m.set_color_deferral(True)
        results = []
        for k, i in enumerate((0, 4, 8, 12)):
            d, rgb, T = A.room_frame(i)
            m.integrate_depth(d, T, A.SMALL_CAM)
            m.integrate_color(rgb, T, A.SMALL_CAM)
            m.update_esdf()
            if relocalize and k == 1:
                results.append(_np(m.score_poses(x, poses)[0])[:, 1].max())
                results.append(m.relocalize_points(x, T0, **RI.LATTICE).coarse.valid)
            elif relocalize and k >= 2:
                results.append(_np(m.score_poses(d10, poses, cam=A.SMALL_CAM)[0])[:, 1].max())
                results.append(m.relocalize_depth(d10, T0, A.SMALL_CAM, **RI.LATTICE).coarse.valid)
        m.flush(); m.synchronize()
        return H.map_state(m), results
    plain, _ = sequence(False)
    with_calls, results = sequence(True)
    assert len(results) == 6 and all(r > 100 for r in results), results
    H.assert_same_map(plain, with_calls, "without and with the relocalisation calls")
