"""The colour point query and the pose alignment with a colour term on the GPU (nvbx_query_colors, nvbx_align_points_color /
nvbx_align_depth_color / nvbx_linearize_points_color; SEMANTICS.md "Colour alignment and colour queries") against the calls they fuse, the
float64 model of tests/align_color_independent.py in both of its drivers, the plain alignment calls, and themselves.
The room is test_gpu_align.py's: a 160 x 120 camera, poses 0, 4, .., 36, depth and colour integrated, block_capacity 1 << 13."""
import ctypes as C

import numpy as np
import pytest

import align_color_independent as AC
import align_independent as A
import helpers as H

pytestmark = pytest.mark.gpu
VS = 0.05
EPS = 2.0 ** -52
MIN_WEIGHT = A.DEFAULTS["min_weight"]
MIN_COLOR_WEIGHT = AC.COLOR_DEFAULTS["min_color_weight"]
# tests/test_gpu_query.py holds the TSDF interpolant to 1e-5 (value) and 1e-4 per metre (gradient) against its float64 model, at corner magnitudes
# of the truncation distance 0.2 m.  The colour corners go through the same inline interpolant at magnitudes up to 255 levels: the bounds scale by
# 255 / 0.2, to 1.275e-2 and 0.1275, written with two digits.
Y_BOUND = 1.3e-2
G_BOUND = 0.13


def _mapper(**params):
    from isaac_ros_nvblox_amd import mapper as M
    return M.Mapper(M.default_params(**params), device=0, block_capacity=1 << 13)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint8)


def _bytes(res):
    return _np(res.buffer).tobytes()


@pytest.fixture(scope="module")
def room(hip_lib):
    m = _mapper()
    for i in A.MAP_FRAMES:
        d, rgb, T = A.room_frame(i)
        m.integrate_depth(d, T, A.SMALL_CAM)
        m.integrate_color(rgb, T, A.SMALL_CAM)
    m.flush(); m.synchronize()
    return m


@pytest.fixture(scope="module")
def frames():
    """per alignment frame: (depth, rgb, true pose, the 1 200-point cloud of the pixels (4 r, 4 c), its colours, the three starts)"""
    out = {}
    for f in A.ALIGN_FRAMES:
        d, rgb, T = A.room_frame(f)
        assert (d[::4, ::4] > 0).all()
        out[f] = (d, rgb, T, A.backproject(d, A.SMALL_CAM, subsampling=4), np.ascontiguousarray(rgb[::4, ::4].reshape(-1, 3)), A.starts(f, T))
    return out


def mixed_cloud(n, depth, rgb, T_true, seed=0):
    """test_gpu_align.mixed_cloud with colours: of every 20 points, 12 from the frame's back-projection (4 of them with a drawn colour, 8 with
    their pixel's), 5 uniform in the room's box, 1 NaN / inf row, 2 far outside the map -- interleaved; the rest carry drawn colours"""
    rng = np.random.default_rng([seed, n])
    T = np.asarray(T_true, np.float64)
    cloud = A.backproject(depth, A.SMALL_CAM); pix = np.ascontiguousarray(rgb.reshape(-1, 3))
    assert len(cloud) == len(pix)
    kind = np.arange(n) % 20
    pts = np.empty((n, 3), np.float32)
    col = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    surf = kind < 12; box = (kind >= 12) & (kind < 17); bad = kind == 17; far = kind >= 18
    pick = rng.integers(0, len(cloud), surf.sum())
    pts[surf] = cloud[pick]
    own = kind[surf] >= 4
    col[np.nonzero(surf)[0][own]] = pix[pick[own]]
    pl = rng.uniform([-3.0, -2.5, 0.0], [3.0, 2.5, 3.0], (box.sum(), 3))
    pts[box] = ((pl - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    special = np.array([[np.nan, 0.5, 1.0], [0.1, np.inf, 1.0], [0.2, 0.3, -np.inf], [np.nan, np.nan, np.nan]], np.float32)
    pts[bad] = special[np.arange(bad.sum()) % 4]
    pts[far] = (rng.uniform(40.0, 60.0, (far.sum(), 3)) * rng.choice([-1.0, 1.0], (far.sum(), 3))).astype(np.float32)
    return pts, col


def world_cloud(n, depth, rgb, T_true):
    """mixed_cloud's points in the map frame (for the point query)"""
    pts, _ = mixed_cloud(n, depth, rgb, T_true)
    T = np.asarray(T_true, np.float32)
    return A.apply_rt_f32(T[:3, :3], T[:3, 3], pts)


# ---- 1. query_color against the full model
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_query_color_against_the_model_on_the_room(room, frames, n):
    import torch
    d, rgb, T, _, _, _ = frames[10]
    p = world_cloud(n, d, rgb, T)
    pt = torch.from_numpy(p).cuda()
    c, y, g, v = (_np(t) for t in room.query_color(pt))
    c2, y2, g2, v2 = (_np(t) for t in room.query_color(pt))
    mc, my, mg, mv = AC.color_query(room.get_blocks, p, VS, MIN_COLOR_WEIGHT)
    assert np.array_equal(v, mv), (int(v.sum()), int(mv.sum()))
    ey, eg, ec = np.abs(y - my).max(), np.abs(g - mg).max(), np.abs(c - mc).max()
    print("n %d: %d valid, max |Y - model| %.3g, |gY - model| %.3g, |rgb - model| %.3g" % (n, int(v.sum()), ey, eg, ec))
    assert ey <= Y_BOUND and eg <= G_BOUND and ec <= Y_BOUND
    assert not y[~v].any() and not g[~v].any() and not c[~v].any()
    if n >= 63:
        assert 0.1 <= v.mean() <= 0.99 and np.abs(g[v]).max() > 1.0
    else:
        assert v.all()
    assert np.array_equal(_bits(y), _bits(y2)) and np.array_equal(_bits(g), _bits(g2)) and np.array_equal(_bits(c), _bits(c2)) and np.array_equal(v, v2)
    # a NULL output costs nothing and changes nothing; preallocated outputs
    n_, yo, go, vo = room.query_color(pt, rgb=False)
    assert n_ is None and np.array_equal(_bits(_np(yo)), _bits(y)) and np.array_equal(_bits(_np(go)), _bits(g)) and np.array_equal(_np(vo), v)
    vv = torch.empty(n, dtype=torch.bool, device="cuda")
    out = room.query_color(pt, out=(None, None, None, vv))
    assert out[3] is vv and np.array_equal(_np(vv), v)


# ---- 2. query_color on drawn blocks
def _drawn(case, rng):
    """eight blocks around the corner (0, 0, 0) with drawn colours; -> (tsdf indices, tsdf data, colour indices, colour data)"""
    idx = np.array([(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)], np.int32)
    tsdf = np.zeros((8, 512), AC.TSDF_DT); tsdf["distance"] = rng.uniform(-0.2, 0.2, (8, 512)).astype(np.float32); tsdf["weight"] = 1.0
    color = np.zeros((8, 512), AC.COLOR_DT)
    for ch in ("r", "g", "b"):
        color[ch] = rng.integers(0, 256, (8, 512))
    color["weight"] = rng.uniform(0.5, 4.0, (8, 512)).astype(np.float32)
    last = 7          # block (0, 0, 0): the one only the corners past a block face reach
    assert tuple(idx[last]) == (0, 0, 0)
    if case == "weight":
        color["weight"][last, 0] = 0.0          # voxel (0, 0, 0) of block (0, 0, 0)
    keep_t = np.ones(8, bool); keep_c = np.ones(8, bool)
    if case == "no_colour":
        keep_c[last] = False
    if case == "absent":
        keep_c[last] = keep_t[last] = False
    return idx[keep_t], tsdf[keep_t], idx[keep_c], color[keep_c]


@pytest.mark.parametrize("case", ["all", "weight", "no_colour", "absent"])
def test_query_color_on_drawn_blocks(hip_lib, case):
    """a base voxel with vx, vy or vz = 7 in every combination (the corners lie in 1, 2, 4 or 8 blocks); one corner's weight 0, one corner's
    block present in the TSDF but without colour, one corner's block absent"""
    from isaac_ros_nvblox_amd import mapper as M
    rng = np.random.default_rng(7)
    ti, td, ci, cd = _drawn(case, rng)
    m = _mapper()
    m.set_blocks(M.LAYER_TSDF, ti, td); m.set_blocks(M.LAYER_COLOR, ci, cd)
    model = AC.DrawnMap(ci, {AC.LAYER_COLOR: cd})
    base = np.array([(x, y, z) for x in (-1, -5) for y in (-1, -5) for z in (-1, -5)], np.float64)          # local 7 (crosses) or 3 (does not)
    p = ((base + 0.5 + np.array([0.3, 0.6, 0.45])) * VS).astype(np.float32)
    c, y, g, v = (_np(t) for t in m.query_color(p))
    mc, my, mg, mv = AC.color_query(model.get_blocks, p, VS, MIN_COLOR_WEIGHT)
    crosses_all = (base == -1).all(axis=1)
    assert np.array_equal(mv, ~crosses_all if case != "all" else np.ones(8, bool))          # (what the case is drawn for)
    assert np.array_equal(v, mv), (case, v, mv)
    assert np.abs(y - my).max() <= Y_BOUND and np.abs(g - mg).max() <= G_BOUND and np.abs(c - mc).max() <= Y_BOUND
    assert not y[~v].any() and not g[~v].any() and not c[~v].any()
    assert (y[v] > 0).all() and np.abs(g[v]).max() > 1.0
    # the map's own read-back tells the model the same
    _, _, _, mv2 = AC.color_query(m.get_blocks, p, VS, MIN_COLOR_WEIGHT)
    assert np.array_equal(mv2, mv)


# ---- 3. the linearization is the composition
def summation_bound(n, mag):
    return n * EPS * mag


@pytest.mark.parametrize("levels", [0.0, 20.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1200, 19200, 65537])
def test_linearization_is_the_composition(room, frames, n, levels):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    d_img, rgb, T_true, _, _, st = frames[10]
    cloud, col = mixed_cloud(n, d_img, rgb, T_true)
    T = st[0]
    x = torch.from_numpy(cloud).cuda(); ct = torch.from_numpy(col).cuda()
    opts = dict(color_huber_levels=levels, huber_delta_m=0.02, min_valid=1)
    res, pl, r, g, v, cy, cg, cv = room.linearize_points_color(x, ct, T, **opts)
    res2, pl2, r2, g2, v2, cy2, cg2, cv2 = room.linearize_points_color(x, ct, T, **opts)
    # the transform and the two queries it fuses, bit for bit
    ref_p = torch.empty_like(x)
    Tm = np.ascontiguousarray(np.asarray(T, np.float32))
    assert room.lib.nvbx_transform_pointcloud(room._h, Tm.ctypes.data_as(C.c_void_p), C.c_void_p(x.data_ptr()), n, C.c_void_p(ref_p.data_ptr())) == 0
    room.synchronize()
    rd, rg, rv = room.query_tsdf(ref_p, min_weight=MIN_WEIGHT, unknown_value=0.0)
    _, qy, qg, qv = room.query_color(ref_p, min_color_weight=MIN_COLOR_WEIGHT, rgb=False)
    torch.cuda.synchronize()
    pl, r, g, v, cy, cg, cv = (_np(t) for t in (pl, r, g, v, cy, cg, cv))
    assert np.array_equal(_bits(pl), _bits(_np(ref_p)))
    assert np.array_equal(_bits(r), _bits(_np(rd))) and np.array_equal(_bits(g), _bits(_np(rg))) and np.array_equal(v, _np(rv))
    assert np.array_equal(_bits(cy), _bits(_np(qy))) and np.array_equal(_bits(cg), _bits(_np(qg))) and np.array_equal(cv, _np(qv))
    both = v & cv
    Ys = AC.luminance(col)
    e = cy.astype(np.float64) - Ys
    share = cv.mean()
    near, far = int((np.abs(e[both]) <= levels).sum()), int((np.abs(e[both]) > levels).sum())
    print("n %d: colour-valid share %.3f, both %d, |e| <= %g: %d, above: %d" % (n, share, int(both.sum()), levels, near, far))
    if n >= 63:
        assert 0.1 <= share <= 0.99, share
    else:
        assert v.all()
    if levels > 0 and n >= 1200:
        assert near > 100 and far > 100, (near, far)
    # the sums: identical terms, summation order only
    cur, (mh, mb, mc, mcc) = AC.joint_sums(pl, Tm[:3, 3], r, g, v, cy, cg, Ys, cv, VS, 0.02, 1.0, levels)
    assert res.iterations == 1 and res.n_valid == cur["n_valid"] == int(v.sum()) and res.n_color == cur["n_color"] == int(both.sum())
    assert res.n_valid_first == res.n_valid and res.n_color_first == res.n_color
    assert (np.abs(res.H - cur["H"]) <= summation_bound(n, mh)).all(), np.abs(res.H - cur["H"]).max()
    assert (np.abs(res.b - cur["b"]) <= summation_bound(n, mb)).all(), np.abs(res.b - cur["b"]).max()
    assert abs(res.cost_last - cur["cost"]) <= summation_bound(n, mc)
    assert abs(res.color_cost_last - cur["color_cost"]) <= summation_bound(n, mcc)
    assert np.array_equal(res.H, res.H_first) and np.array_equal(res.b, res.b_first) and res.color_cost_first == res.color_cost_last
    if n >= 63:
        plain = A.sums(pl, Tm[:3, 3], r, g, v, 0.02)[0]
        assert np.abs(res.H - plain).max() > 1e-6          # (the colour term is in H)
    # no step is applied; the step is what the model's solve gives on these sums
    assert np.array_equal(_bits(res.T_L_S), _bits(Tm)) and np.array_equal(res.T64, Tm.astype(np.float64))
    xi, _ = A.solve(res.H, res.b, 0.0, A.DEFAULTS["min_pivot_ratio"])
    if xi is None:
        assert res.status == M.ALIGN_DEGENERATE and not res.step.any()
    else:
        assert res.status == M.ALIGN_LINEARIZED
        assert np.allclose(res.step, xi, rtol=1e-6, atol=1e-9), np.abs(res.step - xi).max()
    # bit-identical from run to run
    assert _bytes(res) == _bytes(res2) and len(_bytes(res)) == M.ALIGN_COLOR_RESULT_BYTES
    assert np.array_equal(_bits(cy), _bits(_np(cy2))) and np.array_equal(_bits(cg), _bits(_np(cg2))) and np.array_equal(cv, _np(cv2))
    assert np.array_equal(_bits(r), _bits(_np(r2))) and np.array_equal(_bits(g), _bits(_np(g2)))


# ---- 4. reduction to the plain call
def _reduction(m, frames):
    d, rgb, _, x, col, st = frames[22]
    opts = dict(huber_delta_m=0.02)
    pairs = [(m.align_points(x, st[0], **opts), m.align_points_color(x, col, st[0], color_weight=0.0, **opts)),
             (m.align_depth(d, st[1], A.SMALL_CAM, **opts), m.align_depth_color(d, rgb, st[1], A.SMALL_CAM, color_weight=0.0, **opts)),
             (m.linearize_points(x, st[2], **opts)[0], m.linearize_points_color(x, col, st[2], color_weight=0.0, **opts)[0])]
    for plain, colour in pairs:
        assert _bytes(plain) == _bytes(colour)[:712]
        assert plain.n_valid > 100
    return [c for _, c in pairs]


def test_weight_zero_is_the_plain_call(room, frames):
    for c in _reduction(room, frames):
        assert c.n_color > 100 and c.color_rmse_first > 0.0


def test_a_map_without_colour_gives_the_plain_call(hip_lib, frames):
    m = _mapper()
    for i in A.MAP_FRAMES:
        d, _, T = A.room_frame(i)
        m.integrate_depth(d, T, A.SMALL_CAM)
    for c in _reduction(m, frames):
        assert c.n_color == 0 and c.n_color_first == 0 and c.color_rmse_last == 0.0
    # ... at any weight: no point has a colour term
    d, rgb, _, x, col, st = frames[22]
    assert _bytes(m.align_points(x, st[0])) == _bytes(m.align_points_color(x, col, st[0], color_weight=4.0))[:712]


# ---- 5. the iterations follow the hybrid model
def test_iterations_follow_the_hybrid_model(room, frames):
    _, _, _, x, col, st = frames[10]
    q = A.hybrid_query(room, MIN_WEIGHT); cq = AC.hybrid_color_query(room, MIN_COLOR_WEIGHT)
    for k in range(1, 7):
        res = room.align_points_color(x, col, st[0], max_iterations=k)
        mod = AC.run(q, cq, x, col, st[0], VS, dict(max_iterations=k))
        dt, _, dr = A.pose_distance(res.T64, mod["T"])
        print("k %d: %s after %d, |dt| %.3g, max |dR| %.3g, n_color %d" % (k, res.status_name, res.iterations, dt, dr, res.n_color))
        assert dt <= 1e-6 and dr <= 1e-6, (k, dt, dr)
        assert (res.iterations, res.status, res.n_valid, res.n_color) == (mod["iterations"], mod["status"], mod["n_valid"], mod["n_color"]), k
        assert res.n_color_first == mod["first"]["n_color"] and res.n_color > 100
        assert abs(res.color_cost_first - mod["first"]["color_cost"]) <= 1e-9 * mod["first"]["color_cost"]
        assert np.array_equal(res.T_L_S, res.T64.astype(np.float32))


# ---- 6. the wall
@pytest.fixture(scope="module")
def wall(hip_lib):
    from isaac_ros_nvblox_amd import mapper as M
    idx, tsdf, color = AC.wall_blocks()
    m = _mapper()
    m.set_blocks(M.LAYER_TSDF, idx, tsdf); m.set_blocks(M.LAYER_COLOR, idx, color)
    x, col, T = AC.wall_cloud()
    depth, rgb, _ = AC.wall_frame()
    model = AC.wall_map()
    fixed = AC.run(A.full_query(model.get_blocks, VS, MIN_WEIGHT), AC.full_color_query(model.get_blocks, VS, MIN_COLOR_WEIGHT), x, col, AC.wall_starts(T)[0], VS)
    assert fixed["status"] == A.CONVERGED
    return dict(m=m, x=x, col=col, T=T, depth=depth, rgb=rgb, fixed=fixed["T"], starts=AC.wall_starts(T))


def test_the_wall_is_degenerate_without_colour_and_converges_with_it(wall):
    from isaac_ros_nvblox_amd import mapper as M
    m = wall["m"]
    for k, T0 in enumerate(wall["starts"]):
        plain = m.align_points(wall["x"], T0)
        assert (plain.status, plain.iterations, plain.n_valid) == (M.ALIGN_DEGENERATE, 1, 1200)
        for res in (m.align_points_color(wall["x"], wall["col"], T0), m.align_depth_color(wall["depth"], wall["rgb"], T0, A.SMALL_CAM)):
            dt, ang, _ = A.pose_distance(res.T64, wall["T"])
            ft, fa, _ = A.pose_distance(res.T64, wall["fixed"])
            print("start %d: %s after %d, %.3g m %.3g deg from the truth, %.3g m %.3g rad from the model's fixed point" % (
                k, res.status_name, res.iterations, dt, np.rad2deg(ang), ft, fa))
            assert res.status == M.ALIGN_CONVERGED and res.n_color == res.n_valid == 1200
            assert ft <= 1e-3 and fa <= 1e-3, (k, ft, fa)
            assert dt <= 1e-3 and np.rad2deg(ang) <= 0.05, (k, dt, np.rad2deg(ang))


def test_a_grey_wall_stays_degenerate(hip_lib):
    from isaac_ros_nvblox_amd import mapper as M
    idx, tsdf, color = AC.wall_blocks(grey=True)
    m = _mapper()
    m.set_blocks(M.LAYER_TSDF, idx, tsdf); m.set_blocks(M.LAYER_COLOR, idx, color)
    x, col, T = AC.wall_cloud(grey=True)
    for T0 in AC.wall_starts(T):
        res = m.align_points_color(x, col, T0)
        assert (res.status, res.iterations, res.n_valid, res.n_color) == (M.ALIGN_DEGENERATE, 1, 1200, 1200)
        assert np.array_equal(_bits(res.T_L_S), _bits(T0))


# ---- 7. the depth form is the point form lane for lane
@pytest.mark.parametrize("s", [3, 7])
def test_depth_form_is_the_point_form_lane_for_lane(room, frames, s):
    import torch
    d_img, rgb, _, _, _, st = frames[22]
    depth = d_img.copy()
    depth[40:60, 50:90] = 0.0
    max_d = 2.5
    fu, fv, cu, cv = (np.float32(v) for v in A.SMALL_CAM[:4])
    d = depth[::s, ::s]
    rs, cs = d.shape
    r = (np.arange(rs) * s).astype(np.float32); c = (np.arange(cs) * s).astype(np.float32)
    rx = ((c + np.float32(0.5)) - cu) / fu; ry = ((r + np.float32(0.5)) - cv) / fv
    pts = np.stack([d * rx[None, :], d * ry[:, None], d], -1).astype(np.float32).reshape(-1, 3)
    take = ((d > 0) & (d <= np.float32(max_d))).reshape(-1)
    pts[~take] = np.nan
    col = np.ascontiguousarray(rgb[::s, ::s].reshape(-1, 3))
    assert int(take.sum()) == {3: 1912, 7: 370}[s]
    rd = room.align_depth_color(torch.from_numpy(depth).cuda(), torch.from_numpy(rgb).cuda(), st[1], A.SMALL_CAM, subsampling=s, max_depth_m=max_d)
    rp = room.align_points_color(pts, col, st[1])
    assert _bytes(rd) == _bytes(rp) and len(_bytes(rd)) == 736
    assert rd.n_valid_first > 100 and rd.n_color_first > 100 and rd.iterations > 1


# ---- 8. held-back work and the map
def test_held_back_work_and_the_map(hip_lib, frames):
    from isaac_ros_nvblox_amd import mapper as M
    _, _, _, x, col, st = frames[10]
    d10, rgb10 = frames[10][0], frames[10][1]
    Aa, B, N, F = (_mapper() for _ in range(4))          # A: plain calls, B: colour calls, N: never aligned, F: flushed before the colour calls
    for m in (Aa, B, N, F):
        m.set_color_deferral(True); m.set_profiling(True)
    got = {}
    for k, i in enumerate((0, 4, 8, 12)):
        d, rgb, T = A.room_frame(i)
        for m in (Aa, B, N, F):
            m.integrate_depth(d, T, A.SMALL_CAM); m.integrate_color(rgb, T, A.SMALL_CAM); m.update_esdf()
        if k == 2:
            got["A"] = [Aa.align_points(x, st[0]), Aa.align_depth(d10, st[0], A.SMALL_CAM), Aa.linearize_points(x, st[0])[0]]
            F.flush()
            for m, tag in ((B, "B"), (F, "F")):
                got[tag] = [m.align_points_color(x, col, st[0]), m.align_depth_color(d10, rgb10, st[0], A.SMALL_CAM),
                            m.linearize_points_color(x, col, st[0])[0]]
    for m in (Aa, B, N, F):
        m.flush(); m.synchronize()
    # a held-back colour frame is carried out first: the same bytes as on the mapper that was flushed before the call
    for b, f in zip(got["B"], got["F"]):
        assert _bytes(b) == _bytes(f) and b.n_color > 100
    # the map and what was pending: as if no alignment had run
    never = H.map_state(N)
    for m, tag in ((Aa, "plain calls"), (B, "colour calls"), (F, "flushed, then colour calls")):
        H.assert_same_map(m, never, tag)
    # the plain calls leave held-back work held back: the launches of a run that never aligned
    launches = lambda m: {k: v["count"] for k, v in m.profile().items() if not k.startswith("_") and "k_align" not in k}      # noqa: E731
    assert launches(Aa) == launches(N), (launches(Aa), launches(N))
    assert Aa.counters() == N.counters()
    assert all(r.n_valid > 100 for r in got["A"])


# ---- 9. early stop and failures
def test_early_stop_and_failures(room, frames):
    from isaac_ros_nvblox_amd import mapper as M
    d_img, rgb, T_true, x, col, st = frames[34]
    done = room.align_points_color(x, col, st[2])
    assert done.status == M.ALIGN_CONVERGED
    # a start at the fixed point: one iteration, and the launches enqueued behind it change nothing
    Tfix = done.T_L_S
    one = room.align_points_color(x, col, Tfix, max_iterations=1)
    many = room.align_points_color(x, col, Tfix, max_iterations=10)
    assert (many.status, many.iterations) == (M.ALIGN_CONVERGED, 1)
    assert _bytes(one) == _bytes(many)
    # too few valid points: no step, the guess comes back bit for bit
    guess = st[0]
    for cloud, cc in ((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8)), ((x + np.float32(100.0)).astype(np.float32), col)):
        res = room.align_points_color(cloud, cc, guess)
        assert (res.status, res.iterations, res.n_valid, res.n_color) == (M.ALIGN_TOO_FEW, 1, 0, 0)
        assert np.array_equal(_bits(res.T_L_S), _bits(guess)) and np.array_equal(res.T64, guess.astype(np.float64)) and not res.step.any()
        assert res.color_cost_first == 0.0 and res.color_cost_last == 0.0
    # the wrapper's own checks, and the library's refusals through it
    with pytest.raises(ValueError):
        room.align_points_color(x, col[:-1], guess)
    with pytest.raises(ValueError):
        room.align_depth_color(d_img, rgb[:-1], guess, A.SMALL_CAM)
    with pytest.raises(TypeError):
        room.align_points_color(x, col, guess, colour_weight=1.0)
    for kw in (dict(color_weight=-1.0), dict(color_weight=float("nan")), dict(color_weight=float("inf")), dict(min_color_weight=float("nan")),
               dict(color_huber_levels=float("nan")), dict(max_iterations=0), dict(min_valid=0)):
        with pytest.raises(M.NvbxError):
            room.align_points_color(x, col, guess, **kw)
        with pytest.raises(M.NvbxError):
            room.align_depth_color(d_img, rgb, guess, A.SMALL_CAM, **kw)
        with pytest.raises(M.NvbxError):
            room.linearize_points_color(x, col, guess, **kw)
    with pytest.raises(M.NvbxError):
        room.query_color(x, min_color_weight=float("nan"))
    occ = _mapper(projective_layer_type=1)
    for call in (lambda: occ.align_points_color(x, col, guess), lambda: occ.align_depth_color(d_img, rgb, guess, A.SMALL_CAM),
                 lambda: occ.linearize_points_color(x, col, guess), lambda: occ.query_color(x)):
        with pytest.raises(M.NvbxError):
            call()
    again = room.align_points_color(x, col, st[2])                                # the room's mapper stays usable
    assert _bytes(again) == _bytes(done)
