"""Pose alignment on the GPU (nvbx_align_points / nvbx_align_depth / nvbx_linearize_points; SEMANTICS.md "Pose alignment") against the calls it
fuses (nvbx_transform_pointcloud, query_tsdf), the float64 model of tests/align_independent.py in both of its drivers, and itself.
The map is the smoke-sized room: a 160 x 120 camera, poses 0, 4, .., 36, block_capacity 1 << 13."""
import ctypes as C

import numpy as np
import pytest

import align_independent as A
import helpers as H

pytestmark = pytest.mark.gpu
VS = 0.05
EPS = 2.0 ** -52
MIN_WEIGHT = A.DEFAULTS["min_weight"]


def _mapper(**params):
    from isaac_ros_nvblox_amd import mapper as M
    return M.Mapper(M.default_params(**params), device=0, block_capacity=1 << 13)


@pytest.fixture(scope="module")
def room(hip_lib):
    m = _mapper()
    for i in A.MAP_FRAMES:
        d, _, T = A.room_frame(i)
        m.integrate_depth(d, T, A.SMALL_CAM)
    m.synchronize()
    return m


@pytest.fixture(scope="module")
def frames():
    """per alignment frame: (depth, true pose, the 1 200-point cloud of the pixels (4 r, 4 c), the three starts)"""
    out = {}
    for f in A.ALIGN_FRAMES:
        d, _, T = A.room_frame(f)
        out[f] = (d, T, A.backproject(d, A.SMALL_CAM, subsampling=4), A.starts(f, T))
    return out


@pytest.fixture(scope="module")
def fixed_points(room, frames):
    """the full model's fixed point per frame, over the GPU map's own blocks: computed once"""
    q = A.full_query(room.get_blocks, VS, MIN_WEIGHT)
    out = {}
    for f, (_, _, x, st) in frames.items():
        r = A.run(q, x, st[0])
        assert r["status"] == A.CONVERGED
        out[f] = r["T"]
    return out


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint8)


def mixed_cloud(n, frame_cloud, T_true, seed=0):
    """n sensor-frame points: of every 20, 12 from the frame's back-projection, 5 uniform in the room's box (moved into the sensor frame),
    1 NaN / inf row, 2 far outside the map -- interleaved, so every prefix is mixed and point 0 is a surface point"""
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


def summation_bound(n, mag):
    return n * EPS * mag


def check_sums(sums_gpu, H_gpu, b_gpu, cost_gpu, p, t_f32, d, g, v, huber, n):
    """the result's sums against the numpy float64 sums of the same per-point values: identical terms, summation order only"""
    H, b, cost, nv, (mh, mb, mc) = A.sums(p, t_f32, d, g, v, huber)
    assert sums_gpu == nv
    assert (np.abs(H_gpu - H) <= summation_bound(n, mh)).all(), np.abs(H_gpu - H).max()
    assert (np.abs(b_gpu - b) <= summation_bound(n, mb)).all(), np.abs(b_gpu - b).max()
    assert abs(cost_gpu - cost) <= summation_bound(n, mc)
    return H, b, cost, nv


@pytest.mark.parametrize("huber,damping", [(0.0, 0.0), (0.02, 0.0), (0.0, 1e-3), (0.02, 1e-3)])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1200, 19200, 65537])
def test_linearization_is_the_composition(room, frames, n, huber, damping):
    """(n = 65 537: one more than the launch's 256 x 256 threads.  The valid-share property needs both kinds of points and is asserted from
    n = 63 on, n = 1 is one valid surface point; the two sides of the Huber threshold need more than 200 points and are asserted from n = 1 200 on.)"""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    d_img, T_true, _, st = frames[10]
    cloud = mixed_cloud(n, A.backproject(d_img, A.SMALL_CAM), T_true)
    T = st[0]
    x = torch.from_numpy(cloud).cuda()
    opts = dict(huber_delta_m=huber, damping=damping, min_valid=1)
    res, pl, r, g, v = room.linearize_points(x, T, **opts)
    res2, pl2, r2, g2, v2 = room.linearize_points(x, T, **opts)
    # the transform and the query it fuses, bit for bit
    ref_p = torch.empty_like(x)
    Tm = np.ascontiguousarray(np.asarray(T, np.float32))
    assert room.lib.nvbx_transform_pointcloud(room._h, Tm.ctypes.data_as(C.c_void_p), C.c_void_p(x.data_ptr()), n, C.c_void_p(ref_p.data_ptr())) == 0
    room.synchronize()
    rd, rg, rv = room.query_tsdf(ref_p, min_weight=MIN_WEIGHT, unknown_value=0.0)
    torch.cuda.synchronize()
    pl, r, g, v = _np(pl), _np(r), _np(g), _np(v)
    assert np.array_equal(_bits(pl), _bits(_np(ref_p)))
    assert np.array_equal(_bits(r), _bits(_np(rd))) and np.array_equal(_bits(g), _bits(_np(rg))) and np.array_equal(v, _np(rv))
    share = v.mean()
    print("n %d: valid share %.3f" % (n, share))
    if n >= 63:
        assert 0.2 <= share <= 0.99, share
    else:
        assert v.all()
    if huber > 0 and n >= 1200:
        assert (np.abs(r[v]) > np.float32(huber)).sum() > 100 and (np.abs(r[v]) <= np.float32(huber)).sum() > 100
    # the sums
    assert res.iterations == 1 and res.n_valid == int(v.sum()) == res.n_valid_first
    H, b, cost, nv = check_sums(res.n_valid, res.H, res.b, res.cost_last, pl, Tm[:3, 3], r, g, v, huber, n)
    assert np.array_equal(res.H, res.H_first) and np.array_equal(res.b, res.b_first) and res.cost_first == res.cost_last
    # the pose is the one handed over, no step is applied; the step is what the model's solve gives on these sums
    assert np.array_equal(_bits(res.T_L_S), _bits(Tm)) and np.array_equal(res.T64, Tm.astype(np.float64))
    xi, _ = A.solve(res.H, res.b, damping, A.DEFAULTS["min_pivot_ratio"])
    if xi is None:
        assert res.status == M.ALIGN_DEGENERATE and not res.step.any()
    else:
        assert res.status == M.ALIGN_LINEARIZED
        assert np.allclose(res.step, xi, rtol=1e-6, atol=1e-9), np.abs(res.step - xi).max()
    # bit-identical from run to run
    assert np.array_equal(_np(res.buffer), _np(res2.buffer))
    assert np.array_equal(_bits(pl), _bits(_np(pl2))) and np.array_equal(_bits(r), _bits(_np(r2))) and np.array_equal(_bits(g), _bits(_np(g2)))


def test_iterations_follow_the_hybrid_model(room, frames):
    from isaac_ros_nvblox_amd import mapper as M
    _, _, x, st = frames[10]
    q = A.hybrid_query(room, MIN_WEIGHT)
    for k in range(1, 7):
        res = room.align_points(x, st[0], max_iterations=k)
        mod = A.run(q, x, st[0], dict(max_iterations=k))
        dt, _, dr = A.pose_distance(res.T64, mod["T"])
        print("k %d: %s after %d, |dt| %.3g, max |dR| %.3g" % (k, res.status_name, res.iterations, dt, dr))
        assert dt <= 1e-6 and dr <= 1e-6, (k, dt, dr)
        assert (res.iterations, res.status, res.n_valid) == (mod["iterations"], mod["status"], mod["n_valid"]), k
        assert res.n_valid_first == mod["first"]["n_valid"]
        assert abs(res.cost_first - mod["first"]["cost"]) <= 1e-9 * mod["first"]["cost"]
        assert np.array_equal(res.T_L_S, res.T64.astype(np.float32))
    assert res.status == M.ALIGN_CONVERGED and res.rmse_last < res.rmse_first


def test_end_to_end_refinement_reaches_the_models_fixed_point(room, frames, fixed_points):
    from isaac_ros_nvblox_amd import mapper as M
    for f, (_, T_true, x, st) in frames.items():
        ends = []
        for T0 in st:
            res = room.align_points(x, T0)
            assert res.status == M.ALIGN_CONVERGED and res.iterations <= 10
            ends.append(res.T64)
            dt, ang, _ = A.pose_distance(res.T64, T_true)
            assert dt <= 0.05 and np.rad2deg(ang) <= 0.5, (f, dt, np.rad2deg(ang))
            dt, ang, _ = A.pose_distance(res.T64, fixed_points[f])
            print("frame %d: %d iterations, %.3g m %.3g rad from the full model's fixed point" % (f, res.iterations, dt, ang))
            assert dt <= 1e-3 and ang <= 1e-3, (f, dt, ang)
        for T in ends[1:]:
            dt, _, dr = A.pose_distance(T, ends[0])
            assert dt <= 1e-4 and dr <= 1e-4, (f, dt, dr)


@pytest.mark.parametrize("s", [1, 3, 4])
def test_depth_is_points(room, frames, s):
    import torch
    d_img, _, _, st = frames[22]
    depth = d_img.copy()
    depth[40:60, 50:90] = 0.0                                   # a hole; and the far part of the room lies beyond max_depth_m
    max_d = 2.5
    taken = np.zeros(depth.shape, bool); taken[::s, ::s] = True
    taken &= (depth > 0) & (depth <= np.float32(max_d))
    assert taken.sum() > 200 and (depth[::s, ::s] > np.float32(max_d)).sum() > 50 and (depth[::s, ::s] == 0).sum() > 10
    cloud = room.backproject_depth(np.where(taken, depth, np.float32(0.0)).astype(np.float32), A.SMALL_CAM, max_distance_m=max_d)
    assert len(cloud) == taken.sum()
    assert np.array_equal(np.sort(_bits(cloud).view(np.uint32), axis=0), np.sort(_bits(A.backproject(depth, A.SMALL_CAM, s, max_d)), axis=0))
    rd = room.align_depth(torch.from_numpy(depth).cuda(), st[1], A.SMALL_CAM, subsampling=s, max_depth_m=max_d)
    rp = room.align_points(cloud, st[1])
    assert (rd.n_valid_first, rd.n_valid, rd.status, rd.iterations) == (rp.n_valid_first, rp.n_valid, rp.status, rp.iterations)
    # at the guess both saw the same points: the sums differ by summation order only
    lin, pl, r, g, v = room.linearize_points(cloud, st[1])
    Tm = np.asarray(st[1], np.float32)
    for res in (rd, rp):
        check_sums(res.n_valid_first, res.H_first, res.b_first, res.cost_first, _np(pl), Tm[:3, 3], _np(r), _np(g), _np(v), 0.0, len(cloud))
    dt, _, dr = A.pose_distance(rd.T64, rp.T64)
    assert dt <= 1e-6 and dr <= 1e-6, (dt, dr)
    # exactly those pixels: without the limit, and without the hole, more points are valid
    assert room.align_depth(depth, st[1], A.SMALL_CAM, subsampling=s, max_iterations=1).n_valid_first > rd.n_valid_first
    assert room.align_depth(d_img, st[1], A.SMALL_CAM, subsampling=s, max_depth_m=max_d, max_iterations=1).n_valid_first > rd.n_valid_first


@pytest.mark.parametrize("s", [3, 7])
def test_depth_form_is_the_point_form_lane_for_lane(room, frames, s):
    """The depth form's pixel i = r cs + c sits in the lane and the workgroup of point i of an (rs cs, 3) cloud, and a non-finite point is never
    valid: with a NaN row where the pixel is not taken, the cloud leaves the depth form's result record byte for byte, and its score records but for
    `points`, which counts the NaN rows too.  (s = 3: 40 x 54 pixels, the columns leave a remainder; s = 7: 18 x 23, both sides do.)"""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    d_img, T_true, _, st = frames[22]
    depth = d_img.copy()
    depth[40:60, 50:90] = 0.0
    max_d = 2.5
    fu, fv, cu, cv = (np.float32(v) for v in A.SMALL_CAM[:4])
    d = depth[::s, ::s]
    rs, cs = d.shape
    assert (rs, cs) == {3: (40, 54), 7: (18, 23)}[s] and (rs - 1) * s < 120 and (cs - 1) * s < 160
    r = (np.arange(rs) * s).astype(np.float32); c = (np.arange(cs) * s).astype(np.float32)
    rx = ((c + np.float32(0.5)) - cu) / fu; ry = ((r + np.float32(0.5)) - cv) / fv                     # (align_independent.backproject's arithmetic)
    pts = np.stack([d * rx[None, :], d * ry[:, None], d], -1).astype(np.float32).reshape(-1, 3)
    take = ((d > 0) & (d <= np.float32(max_d))).reshape(-1)
    assert np.array_equal(_bits(pts[take]), _bits(A.backproject(depth, A.SMALL_CAM, s, max_d)))
    pts[~take] = np.nan
    n_taken = int(take.sum())
    assert n_taken == {3: 1912, 7: 370}[s] and (d == 0).sum() > 0 and (d > np.float32(max_d)).sum() > 0
    dt = torch.from_numpy(depth).cuda()
    rd = room.align_depth(dt, st[1], A.SMALL_CAM, subsampling=s, max_depth_m=max_d)
    rp = room.align_points(pts, st[1])
    bd, bp = _np(rd.buffer).tobytes(), _np(rp.buffer).tobytes()
    assert len(bd) == M.ALIGN_RESULT_BYTES == 712 and bd == bp
    assert rd.n_valid_first > 100 and rd.iterations > 1                          # (a real refinement, not a record both forms left untouched)
    poses = np.stack([np.asarray(T, np.float32) for T in [T_true] + list(st)])
    cd, qd = room.score_poses(dt, poses, cam=A.SMALL_CAM, subsampling=s, max_depth_m=max_d)
    cp, qp = room.score_poses(pts, poses)
    cd, qd, cp, qp = _np(cd), _np(qd), _np(cp), _np(qp)
    assert np.array_equal(cd[:, 1:], cp[:, 1:]) and np.array_equal(qd, qp) and cd[0, 1] > 100
    assert (cd[:, 0] == n_taken).all() and (cp[:, 0] == rs * cs).all()


def test_early_stop_and_failures(room, frames):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    _, T_true, x, st = frames[34]
    done = room.align_points(x, st[2])
    assert done.status == M.ALIGN_CONVERGED
    # a start at the fixed point: one iteration, and the launches enqueued behind it change nothing
    Tfix = done.T_L_S
    one = room.align_points(x, Tfix, max_iterations=1)
    many = room.align_points(x, Tfix, max_iterations=10)
    assert (many.status, many.iterations) == (M.ALIGN_CONVERGED, 1)
    assert np.array_equal(_np(one.buffer), _np(many.buffer))
    # too few valid points: no step, the guess comes back bit for bit
    guess = st[0]
    for cloud in (np.zeros((0, 3), np.float32), (x + np.float32(100.0)).astype(np.float32)):
        res = room.align_points(cloud, guess)
        assert (res.status, res.iterations, res.n_valid) == (M.ALIGN_TOO_FEW, 1, 0)
        assert np.array_equal(_bits(res.T_L_S), _bits(guess)) and np.array_equal(res.T64, guess.astype(np.float64)) and not res.step.any()
    # three valid points: a failing pivot
    _, _, _, _, v = room.linearize_points(x, guess)
    three = x[np.nonzero(_np(v))[0][[0, 400, 800]]]
    res = room.align_points(three, guess, min_valid=1)
    assert (res.status, res.iterations, res.n_valid) == (M.ALIGN_DEGENERATE, 1, 3)
    assert np.array_equal(_bits(res.T_L_S), _bits(guess)) and not res.step.any()
    assert room.align_points(three, guess).status == M.ALIGN_TOO_FEW              # (min_valid 50)
    # invalid arguments: NVBX_E_INVALID, nothing launched
    bad_pose = guess.copy(); bad_pose[0, 3] = np.nan
    for kw in (dict(max_iterations=0), dict(max_iterations=65), dict(min_valid=0), dict(damping=-1.0), dict(min_pivot_ratio=float("nan")),
               dict(stop_translation_m=-1.0), dict(stop_rotation_rad=-1.0), dict(min_weight=float("nan")), dict(huber_delta_m=float("nan")),
               dict(max_depth_m=float("nan")), dict(stop_translation_m=float("inf")), dict(stop_rotation_rad=float("inf")), dict(damping=float("inf"))):
        with pytest.raises(M.NvbxError):
            room.align_points(x, guess, **kw)
    with pytest.raises(M.NvbxError):
        room.align_points(x, bad_pose)
    with pytest.raises(M.NvbxError):
        room.linearize_points(x, bad_pose)
    d_img = frames[34][0]
    with pytest.raises(M.NvbxError):
        room.align_depth(d_img, guess, A.SMALL_CAM, subsampling=0)
    with pytest.raises(M.NvbxError):
        room.align_depth(d_img, guess, (80.0, 80.0, 79.5, 59.5, 161, 120))
    xt = torch.from_numpy(x).cuda(); buf = torch.empty(M.ALIGN_RESULT_BYTES + 8, dtype=torch.uint8, device="cuda")
    Tg = np.ascontiguousarray(guess); pT = Tg.ctypes.data_as(C.c_void_p); px = C.c_void_p(xt.data_ptr()); pb = C.c_void_p(buf.data_ptr())
    lib, h = room.lib, room._h
    cam = M.Camera(80.0, 80.0, 79.5, 59.5, 160, 120)
    dt = torch.from_numpy(d_img).cuda(); pd = C.c_void_p(dt.data_ptr())
    assert buf.data_ptr() % 8 == 0
    for rc in (lib.nvbx_align_points(None, px, len(x), pT, None, pb), lib.nvbx_align_points(h, None, len(x), pT, None, pb),
               lib.nvbx_align_points(h, px, -1, pT, None, pb), lib.nvbx_align_points(h, px, len(x), None, None, pb),
               lib.nvbx_align_points(h, px, len(x), pT, None, None), lib.nvbx_align_points(h, px, len(x), pT, None, C.c_void_p(buf.data_ptr() + 4)),
               lib.nvbx_linearize_points(h, None, len(x), pT, None, pb, None, None, None, None),
               lib.nvbx_linearize_points(h, px, len(x), pT, None, None, None, None, None, None),
               lib.nvbx_align_depth(h, None, 120, 160, pT, C.byref(cam), None, pb), lib.nvbx_align_depth(h, pd, 120, 160, pT, None, None, pb),
               lib.nvbx_align_depth(h, pd, 0, 160, pT, C.byref(cam), None, pb), lib.nvbx_align_depth(h, pd, 120, 160, None, C.byref(cam), None, pb),
               lib.nvbx_align_depth(h, pd, 120, 160, pT, C.byref(cam), None, None)):
        assert rc == -1, rc
    assert lib.nvbx_align_points(h, px, len(x), pT, None, pb) == 0                # options NULL: the defaults
    room.synchronize()
    occ = _mapper(projective_layer_type=1)
    for call in (lambda: occ.align_points(x, guess), lambda: occ.align_depth(d_img, guess, A.SMALL_CAM), lambda: occ.linearize_points(x, guess)):
        with pytest.raises(M.NvbxError):
            call()
    occ.integrate_depth(d_img, T_true, A.SMALL_CAM); occ.synchronize()
    assert occ.num_blocks(M.LAYER_OCCUPANCY) > 0                                  # the refused mapper stays usable
    again = room.align_points(x, st[2])                                           # ... and so does the room's
    assert np.array_equal(_np(again.buffer), _np(done.buffer))


def test_alignment_leaves_the_map_and_held_back_work_alone(frames):
    """under colour deferral a colour frame and an updateEsdf are held back when the alignment runs between two depth frames: the final layers are
    bit-identical to the same sequence without it"""
    _, _, x, st = frames[10]

    def sequence(align):
        m = _mapper()
        m.set_color_deferral(True)
        results = []
        for k, i in enumerate((0, 4, 8, 12)):
            d, rgb, T = A.room_frame(i)
            m.integrate_depth(d, T, A.SMALL_CAM)
            m.integrate_color(rgb, T, A.SMALL_CAM)
            m.update_esdf()
            if align and k >= 1:
                results.append(m.align_points(x, st[0]) if k == 1 else m.align_depth(frames[10][0], st[0], A.SMALL_CAM))
        m.flush(); m.synchronize()
        return H.map_state(m), results
    plain, _ = sequence(False)
    with_align, results = sequence(True)
    assert len(results) == 3 and all(r.n_valid > 100 for r in results)
    H.assert_same_map(plain, with_align, "without and with the alignment calls")
