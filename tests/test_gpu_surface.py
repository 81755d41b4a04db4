"""Surface points and map-to-map registration on the GPU (nvbx_surface_points / nvbx_align_map / nvbx_relocalize_map; SEMANTICS.md "Surface
points", "Registering two maps") against the numpy model of tests/surface_independent.py.  Maps are drawn with set_blocks (tests/surface_cases.py);
rows are compared with the model as SETS, bit for bit in position and colour; normals against query_tsdf's gradient normalised on the host by
the same two float32 operations, bit for bit.  The scan's tile is 256 slots (SF_TILE, csrc/surface.hip): the slot test crosses its borders.
One GPU: the refusal of mappers on different devices is not reached here."""
import ctypes as C

import numpy as np
import pytest

import align_independent as AI
import helpers as H
import surface_cases as SC
import surface_independent as SI

pytestmark = pytest.mark.gpu

VS = SC.VS
F32 = np.float32
SCAN_TILE = 256
E_INVALID = -1


def _mods():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def _mapper(cap=1 << 10, **params):
    M = _mods()
    return M.Mapper(M.default_params(voxel_size=VS, **params), device=0, block_capacity=cap)


def _upload(m, blocks):
    M = _mods()
    tk = [k for k in blocks if "d" in blocks[k]]
    if tk:
        v = np.zeros((len(tk), 512), M.TSDF_DT)
        for i, k in enumerate(tk):
            v[i]["distance"] = blocks[k]["d"].reshape(512); v[i]["weight"] = blocks[k]["w"].reshape(512)
        m.set_blocks(M.LAYER_TSDF, np.array(tk, np.int32), v)
    ck = [k for k in blocks if "rgb" in blocks[k]]
    if ck:
        v = np.zeros((len(ck), 512), M.COLOR_DT)
        for i, k in enumerate(ck):
            rgb = blocks[k]["rgb"].reshape(512, 3)
            v[i]["r"] = rgb[:, 0]; v[i]["g"] = rgb[:, 1]; v[i]["b"] = rgb[:, 2]; v[i]["weight"] = blocks[k]["cw"].reshape(512)
        m.set_blocks(M.LAYER_COLOR, np.array(ck, np.int32), v)
    m.synchronize()


def _read(m):
    """the mapper's TSDF and colour layers as the model's block dict"""
    M = _mods()
    out = {}
    for layer in (M.LAYER_TSDF, M.LAYER_COLOR):
        idx = m.block_indices(layer)
        if not len(idx):
            continue
        v, found = m.get_blocks(layer, idx)
        assert found.all()
        for i, b in enumerate(idx):
            e = out.setdefault(tuple(int(q) for q in b), {})
            if layer == M.LAYER_TSDF:
                e["d"] = v[i]["distance"].reshape(8, 8, 8).copy(); e["w"] = v[i]["weight"].reshape(8, 8, 8).copy()
            else:
                e["rgb"] = np.stack([v[i]["r"], v[i]["g"], v[i]["b"]], -1).reshape(8, 8, 8, 3).copy(); e["cw"] = v[i]["weight"].reshape(8, 8, 8).copy()
    return out


def _check(m, blocks, what="", min_rows=1, **opts):
    """surface_points with colours and normals against the model -> (points, colors, normals) as numpy, the model's rows"""
    want = SI.surface_rows(blocks, VS, min_weight=opts.get("min_weight", 1e-4), stride=opts.get("stride", 1), box=opts.get("box_min_max_vox"),
                           require_color=opts.get("require_color", False))
    p, c, n, count = m.surface_points(color=True, normals=True, **opts)
    p, c, n = p.cpu().numpy(), c.cpu().numpy(), n.cpu().numpy()
    assert count == len(want["t"]) == len(p) and count >= min_rows, (what, count, len(want["t"]), min_rows)
    got, exp = SI.row_set(p, c), SI.row_set(want["points"], want["colors"])
    assert len(exp) == count, (what, "the model's rows are not distinct")
    assert got == exp, (what, len(got - exp), len(exp - got))
    d, g, valid = m.query_tsdf(p, min_weight=opts.get("min_weight", 1e-4))
    nn = SI.unit_normals(g.cpu().numpy(), valid.cpu().numpy())
    assert n.tobytes() == nn.tobytes(), (what, "normals", int((n != nn).any(1).sum()))
    return (p, c, n), want


def _order_of(p, want):
    """for every GPU row the model's (block, t, axis), through the point's bits"""
    key = {bytes(r): i for i, r in enumerate(np.ascontiguousarray(want["points"]).view(np.uint32).reshape(-1, 3))}
    i = np.array([key[bytes(r)] for r in np.ascontiguousarray(p).view(np.uint32).reshape(-1, 3)])
    return want["block"][i], want["t"][i], want["axis"][i]


def _assert_order(p, want, what=""):
    blk, t, ax = _order_of(p, want)
    change = np.flatnonzero((blk[1:] != blk[:-1]).any(1)) + 1
    runs = np.split(np.arange(len(t)), change)
    assert len(runs) == len(set(map(tuple, blk.tolist()))), (what, "the rows of a block are not contiguous")
    for r in runs:
        k = t[r].astype(np.int64) * 4 + ax[r]
        assert (np.diff(k) > 0).all(), (what, "not ascending in (t, axis)", blk[r[0]].tolist())


# ---- 1. block borders
FIVE = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, -1)]


def test_block_borders_and_missing_or_layerless_neighbours(hip_lib):
    blocks = SC.random_blocks(FIVE, seed=3, color_keys=[(0, 0, 0), (0, 0, 1), (0, 1, 1)])      # (0, 1, 1): colour only -- no TSDF layer
    m = _mapper(cap=64)
    _upload(m, blocks)
    back = _read(m)
    assert sorted(back) == sorted(blocks) and "d" not in back[(0, 1, 1)]
    (p, c, n), want = _check(m, back, "five blocks", min_rows=1000)
    on = lambda k, a: ((want["block"] == k).all(1) & (want["axis"] == a) & ((want["t"] >> (6 - 3 * a)) & 7 == 7)).sum()      # noqa: E731
    assert on((0, 0, 0), 0) > 10 and on((0, 0, 0), 1) > 10 and on((0, 0, 0), 2) > 10          # across each of the three faces
    assert on((1, 0, 0), 0) == 0 and on((-1, -1, -1), 2) == 0                                  # an absent neighbour
    assert on((0, 1, 0), 2) == 0 and on((0, 0, 1), 1) == 0                                     # (0, 1, 1) carries no TSDF layer
    assert (n != 0).any(1).sum() > 100 and (c != 0).any(1).sum() > 100
    _assert_order(p, want, "five blocks")
    # two calls: identical bytes
    q = m.surface_points(color=True, normals=True)
    assert all(a.tobytes() == b.cpu().numpy().tobytes() for a, b in zip((p, c, n), q[:3]))
    m.close()


# ---- 2. the full prefix path
def test_checkerboard_takes_every_rank_through_the_wavefront_and_workgroup_prefixes(hip_lib):
    blocks = {(0, 0, 0): SC.checkerboard_block(0), (1, 0, 0): SC.checkerboard_block(0)}      # every edge crosses; +y and +z faces are open
    for i in range(5):
        blocks[(3 + 2 * i, 0, 0)] = SC.one_crossing_block(i)
    for i in range(3):
        blocks[(0, 3 + 2 * i, 0)] = {"d": np.full((8, 8, 8), 0.04, F32), "w": np.ones((8, 8, 8), F32)}
    m = _mapper(cap=64)
    _upload(m, blocks)
    (p, _, _), want = _check(m, blocks, "checkerboard")
    per = {k: int((want["block"] == k).all(1).sum()) for k in blocks}
    assert per[(0, 0, 0)] == 3 * 512 - 2 * 64 and per[(1, 0, 0)] == 3 * 512 - 3 * 64 and per[(3, 0, 0)] == 1 and per[(0, 3, 0)] == 0
    _assert_order(p, want, "checkerboard")
    m.close()


# ---- 3. slots and scan tiles
def test_holes_below_the_high_water_mark_and_every_tile_border(hip_lib):
    n = 700                                               # slots 0 .. 699: tiles 0, 1, 2 of SCAN_TILE slots
    blocks = {(2 * i, 0, 0): SC.one_crossing_block(i) for i in range(n)}
    m = _mapper(cap=1 << 10)
    _upload(m, blocks)
    assert m.surface_points()[3] == n
    centre = np.array([2 * 350 * 8 * VS, 0.2, 0.2], F32)
    m.clear_outside_radius(centre, 2 * 230 * 8 * VS)     # about 460 blocks stay: at most 240 holes, so every tile still holds blocks
    back = _read(m)
    assert 400 < len(back) < 520 and n - len(back) < SCAN_TILE
    (p, _, _), want = _check(m, back, "holes", min_rows=len(back))
    assert len(p) == len(back) > 2 * SCAN_TILE - (n - len(back))
    m.close()


# ---- 4. capacity
def test_capacity_below_the_count_counts_all_and_writes_no_further(hip_lib):
    import torch
    blocks = SC.random_blocks(FIVE[:4], seed=5)
    m = _mapper(cap=64)
    _upload(m, blocks)
    p, _, n, count = m.surface_points(normals=True)
    assert count > 1500
    k = 777
    big_p = torch.full((k + 64, 3), -7.0, dtype=torch.float32, device="cuda"); big_n = torch.full((k + 64, 3), -7.0, dtype=torch.float32, device="cuda")
    big_c = torch.full((k + 64, 3), 9, dtype=torch.uint8, device="cuda")
    q, c, qn, qcount = m.surface_points(out=(big_p[:k], big_c[:k], big_n[:k]))
    assert qcount == count and len(q) == k
    assert torch.equal(q, p[:k]) and qn.cpu().numpy().tobytes() == n[:k].cpu().numpy().tobytes()
    assert (big_p[k:] == -7.0).all() and (big_n[k:] == -7.0).all() and (big_c[k:] == 9).all()
    assert m.surface_points(capacity=0)[3] == count      # NULL arrays: counts only
    cnt = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    assert m.lib.nvbx_surface_points(m._h, None, None, None, None, 0, C.c_void_p(cnt.data_ptr())) == 0
    m.synchronize()
    assert int(cnt.item()) == count
    e = _mapper(cap=64)
    pe, _, _, ce = e.surface_points()
    assert ce == 0 and tuple(pe.shape) == (0, 3)
    e.close(); m.close()


# ---- 5. filters and contract
@pytest.fixture(scope="module")
def straddling(hip_lib):
    keys = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    blocks = SC.random_blocks(keys, seed=9, p_nan=0.0, color_keys=keys[::3])      # (no NaN: the map comparison of helpers.py takes none)
    m = _mapper(cap=64)
    _upload(m, blocks)
    yield m, _read(m)
    m.close()


@pytest.mark.parametrize("opts", [dict(stride=2), dict(stride=3), dict(box_min_max_vox=(-5, -8, -3, 4, 2, 7)), dict(box_min_max_vox=(-3, -3, -3, -3, -3, -3)),
                                  dict(min_weight=0.5e-4), dict(min_weight=1.5), dict(require_color=True), dict(stride=2, require_color=True, box_min_max_vox=(-8, -8, -8, 7, 7, 0))])
def test_filters(straddling, opts):
    m, blocks = straddling
    before = H.map_state(m, layers=(_mods().LAYER_TSDF, _mods().LAYER_COLOR))
    (p, _, _), want = _check(m, blocks, str(opts), min_rows=0)
    if "min_weight" not in opts or opts["min_weight"] < 1:
        assert len(p) > 0, opts
    _assert_order(p, want, str(opts))
    H.assert_same_map(before, m, "before and after surface_points")


def test_held_back_work_stays_held_back(hip_lib):
    """Two mappers with colour deferral on get the same frames; one of them asks for its surface points (no colour) between pipelined frames.
    Apart from the call's own kernels it has launched exactly the same kernels as often, and holds the same map."""
    from isaac_ros_nvblox_amd import synthetic as S
    M = _mods()
    sc = S.Scene()
    A = M.Mapper(M.default_params(), device=0, block_capacity=1 << 13); B = M.Mapper(M.default_params(), device=0, block_capacity=1 << 13)
    for m in (A, B):
        m.set_color_deferral(True); m.set_profiling(True)
    counts = []
    for k in range(4):
        T = S.trajectory_pose(3 * k)
        d, rgb = S.render(sc, T, H.SMALL_CAM)
        for m in (A, B):
            m.integrate_depth(d, T, H.SMALL_CAM); m.integrate_color(rgb, T, H.SMALL_CAM); m.update_esdf()
        if k in (1, 2):
            counts.append(A.surface_points(normals=True)[3])
    for m in (A, B):
        m.synchronize()
    assert counts[0] > 1000 and counts[1] >= counts[0]
    pa = {k: v["count"] for k, v in A.profile().items() if not k.startswith("_") and "k_surface" not in k}
    pb = {k: v["count"] for k, v in B.profile().items() if not k.startswith("_")}
    assert pa == pb, (pa, pb)
    assert any("k_integrate_tsdf_color" in k for k in pa), list(pa)[:20]
    assert {k for k in A.profile() if "k_surface" in k} == {"k_surface_count", "k_surface_tile_sums", "k_surface_scan_tiles", "k_surface_emit", "k_surface_normals"}
    H.assert_same_map(A, B, "against the mapper that never asked")
    A.close(); B.close()


# ---- 6. align_map and relocalize_map
@pytest.fixture(scope="module")
def rooms(hip_lib):
    first, second = SC.room_blocks(None), SC.room_blocks(SC.ROOM_T)
    a = _mapper(cap=256); b = _mapper(cap=256); a0 = _mapper(cap=256)
    _upload(a, first); _upload(b, second); _upload(a0, first)
    yield a, b, a0, first, second
    a.close(); b.close(); a0.close()


def _zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device="cuda")


def test_align_map_is_surface_points_then_align_points(rooms):
    M = _mods()
    a, b, _, _, second = rooms
    I = np.eye(4, dtype=F32)
    half = dict(box_min_max_vox=(-64, -64, -64, 63, 63, 3))      # the lower half of the room: the options reach the call
    p, c, _, count = b.surface_points(color=False, **half)
    assert 200 < count < b.surface_points()[3]
    x = a.align_points(p, I, out=_zeros(M.ALIGN_RESULT_BYTES), **SC.ROOM_ALIGN)
    y = a.align_map(b, I, surface=half, out=_zeros(M.ALIGN_RESULT_BYTES), **SC.ROOM_ALIGN)
    assert x.buffer.cpu().numpy().tobytes() == y.buffer.cpu().numpy().tobytes() and y.n_valid > 100
    # ... with a colour term: the crossings that have a colour
    b.set_blocks(M.LAYER_COLOR, np.array(sorted(second)[::2], np.int32), np.full((len(sorted(second)[::2]), 512), np.array((90, 120, 30, 0, 1.0), M.COLOR_DT), M.COLOR_DT))
    a.set_blocks(M.LAYER_COLOR, np.array(sorted(rooms[3]), np.int32), np.full((len(rooms[3]), 512), np.array((80, 110, 40, 0, 1.0), M.COLOR_DT), M.COLOR_DT))
    p, c, _, count = b.surface_points(color=True, require_color=True)
    assert 100 < count < b.surface_points()[3]
    x = a.align_points_color(p, c, I, out=_zeros(M.ALIGN_COLOR_RESULT_BYTES), color_weight=0.5, **SC.ROOM_ALIGN)
    y = a.align_map(b, I, color_weight=0.5, out=_zeros(M.ALIGN_COLOR_RESULT_BYTES), **SC.ROOM_ALIGN)
    assert x.buffer.cpu().numpy().tobytes() == y.buffer.cpu().numpy().tobytes() and y.n_color > 50
    # ... and relocalize_map against relocalize_points
    p, _, _, _ = b.surface_points()
    lat = (SC.ROOM_T, 0.1, 0.05, (3, 3, 3, 3))
    kw = dict(min_inliers=50, score=dict(subsampling=1), align=SC.ROOM_ALIGN, scores=True)
    x = a.relocalize_points(p, *lat, out=_zeros(M.RELOC_RESULT_BYTES), **kw)
    y = a.relocalize_map(b, *lat, out=_zeros(M.RELOC_RESULT_BYTES), **kw)
    assert x.buffer.cpu().numpy().tobytes() == y.buffer.cpu().numpy().tobytes() and y.status_name == "OK"
    assert all(np.array_equal(u.cpu().numpy(), v.cpu().numpy()) for u, v in zip(x.scores, y.scores))
    # no crossing at all: the point call with n = 0
    e = _mapper(cap=64)
    x = a.align_points(np.zeros((0, 3), F32), I, out=_zeros(M.ALIGN_RESULT_BYTES)); y = a.align_map(e, I, out=_zeros(M.ALIGN_RESULT_BYTES))
    assert x.buffer.cpu().numpy().tobytes() == y.buffer.cpu().numpy().tobytes() and y.status_name == x.status_name
    e.close()
    for m, blocks in ((a, rooms[3]), (b, second)):       # the colour blocks go again: the other tests see the rooms as drawn
        m.clear(); _upload(m, blocks)


def test_pose_recovery_and_the_pipeline_it_feeds(rooms):
    """The float64 model on the model's own points ends 9.4e-8 m and 4.8e-8 rad from the true pose (computed here again); the GPU's pose may be
    twice as far, for f32 against f64 evaluation of the interpolant.  Sub-voxel recovery -- 0.1 voxel, and that over the room's extent as an
    angle -- is asserted for both first."""
    a, b, a0, first, second = rooms
    model, (m_dt, m_ang), n_pts = SC.room_model_alignment()
    sub_t, sub_r = 0.1 * VS, 0.1 * VS / (2 * SC.ROOM_HALF)
    assert m_dt <= sub_t and m_ang <= sub_r and model["n_valid"] > 500
    res = a.align_map(b, np.eye(4, dtype=F32), **SC.ROOM_ALIGN)
    dt, ang, _ = AI.pose_distance(res.T64, SC.ROOM_T)
    print("align_map: %d points, %d valid, %d iterations, %s; |dt| %.3e m (model %.3e), angle %.3e rad (model %.3e)" % (
        n_pts, res.n_valid, res.iterations, res.status_name, dt, m_dt, ang, m_ang))
    assert res.n_valid > 500
    assert dt <= sub_t and ang <= sub_r
    assert dt <= 2 * m_dt and ang <= 2 * m_ang, (dt, m_dt, ang, m_ang)
    # the pipeline: merge under the pose found, then nothing has changed against the first map
    before = a0.surface_points()[3]
    mr = a.merge_from(b, res.T_L_S)
    assert mr.voxels_fused > 1000
    out = a.find_changes(a0, np.eye(4, dtype=F32))
    assert int(out[3].item()) == 0 and out[4].voxels_appeared == 0 and out[4].voxels_removed == 0 and out[4].voxels_compared > 1000
    assert a0.surface_points()[3] == before
    a.clear(); _upload(a, first)


def test_refusals_launch_nothing_and_leave_the_mappers_usable(rooms):
    import torch
    M = _mods()
    a, b, _, _, _ = rooms
    occ = _mapper(cap=64, projective_layer_type=1)
    a.synchronize(); b.synchronize()
    for m in (a, b):
        m.set_profiling(True)
    lib = a.lib
    T = (C.c_float * 16)(*np.eye(4, dtype=F32).reshape(-1).tolist())
    res = torch.zeros(1024, dtype=torch.uint8, device="cuda"); cnt = torch.full((1,), -3, dtype=torch.int64, device="cuda")
    pts = torch.zeros((8, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    r, c, pp = C.c_void_p(res.data_ptr()), C.c_void_p(cnt.data_ptr()), C.c_void_p(pts.data_ptr())
    so = lambda **kw: C.byref(a.surface_options(**kw))      # noqa: E731
    bad_box = a.surface_options(box_min_max_vox=(0, 0, 5, 7, 7, 4))
    cases = [lib.nvbx_surface_points(a._h, None, pp, None, None, 8, None), lib.nvbx_surface_points(a._h, None, pp, None, None, -1, c),
             lib.nvbx_surface_points(a._h, None, pp, None, None, (1 << 30) + 1, c), lib.nvbx_surface_points(a._h, None, None, None, None, 8, c),
             lib.nvbx_surface_points(a._h, so(stride=0), pp, None, None, 8, c), lib.nvbx_surface_points(a._h, so(min_weight=float("nan")), pp, None, None, 8, c),
             lib.nvbx_surface_points(a._h, C.byref(bad_box), pp, None, None, 8, c), lib.nvbx_surface_points(occ._h, None, pp, None, None, 8, c),
             lib.nvbx_align_map(a._h, a._h, T, None, None, None, r, None), lib.nvbx_align_map(a._h, occ._h, T, None, None, None, r, None),
             lib.nvbx_align_map(occ._h, b._h, T, None, None, None, r, None), lib.nvbx_align_map(a._h, b._h, None, None, None, None, r, None),
             lib.nvbx_align_map(a._h, b._h, T, so(stride=0), None, None, r, None), lib.nvbx_align_map(a._h, b._h, T, None, None, None, None, None),
             lib.nvbx_align_map(a._h, b._h, T, None, C.byref(a.align_options(max_iterations=0)), None, r, None),
             lib.nvbx_align_map(a._h, b._h, T, None, None, C.byref(a.align_color_options()), r, None),
             lib.nvbx_relocalize_map(a._h, a._h, T, None, None, None, 0, None, None, r), lib.nvbx_relocalize_map(a._h, b._h, T, None, None, None, 0, None, None, r),
             lib.nvbx_relocalize_map(a._h, occ._h, T, C.byref(M.Mapper._lattice(0.1, 0.1, (2, 2, 2, 2))), None, None, 0, None, None, r)]
    assert cases == [E_INVALID] * len(cases), cases
    assert lib.nvbx_last_error()
    a.synchronize(); b.synchronize()
    assert int(cnt.item()) == -3 and not res.any()
    for m in (a, b):
        assert not [k for k in m.profile() if not k.startswith("_")], list(m.profile())
        m.set_profiling(False)
    assert a.align_map(b, np.eye(4, dtype=F32)).n_valid > 500 and b.surface_points()[3] > 1000      # still usable
    occ.close()
