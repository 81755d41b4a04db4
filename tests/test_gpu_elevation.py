"""The elevation map and traversability on the GPU (nvbx_elevation_map / nvbx_traversability; SEMANTICS.md "Elevation and traversability")
against the numpy model of tests/elevation_independent.py: heights, steps, slopes and distances are compared as bytes, status and class as
arrays.  Maps are hand-built with set_blocks, images are handed in as arrays; the end-to-end tests run a drawn kerb scene through to a path and
two 80 x 60 frames of the synthetic room.  block_capacity at most 1 << 12."""
import ctypes as C

import numpy as np
import pytest

import elevation_independent as EI
import helpers as H
import plan_independent as PI

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
F32 = np.float32
VS = F32(EI.VS)
BS = VS * F32(8.0)
MW = EI.MIN_WEIGHT
E_INVALID = -1
SENTINEL = -77.0


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _mapper(cap=256, **params):
    M, _ = _mods()
    m = M.Mapper(M.default_params(**params), device=0, block_capacity=cap)
    assert F32(m.params.voxel_size) == VS
    return m


def _centre(gz):
    return (F32(gz >> 3) * BS + F32(gz & 7) * VS) + VS * F32(0.5)


def _check_map(m, box, what="", min_weight=MW, unknown_value=1000.0):
    """elevation_map on the GPU, the model on the layer read back: status equal, heights equal in every byte -> the model's (height, status)"""
    import torch
    M, _ = _mods()
    want_h, want_s = EI.elevation(EI.read_tsdf(m, M), box, min_weight, unknown_value, EI.VS)
    h, s = m.elevation_map(*box, min_weight=min_weight, unknown_value=unknown_value)
    assert h.dtype == torch.float32 and s.dtype == torch.uint8 and tuple(h.shape) == tuple(s.shape) == (box[2], box[3]), what
    h = h.cpu().numpy(); s = s.cpu().numpy()
    bad = np.argwhere(s != want_s)
    assert len(bad) == 0, (what, "status", len(bad), [(tuple(p), int(s[tuple(p)]), int(want_s[tuple(p)])) for p in bad[:5]])
    bad = np.argwhere(h.view(np.uint32) != want_h.view(np.uint32))
    assert len(bad) == 0, (what, "height", len(bad), [(tuple(p), float(h[tuple(p)]), float(want_h[tuple(p)])) for p in bad[:5]])
    return want_h, want_s


def _same_bytes(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32)) if got.dtype == np.float32 else np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), [(tuple(int(v) for v in p), got[tuple(p)].item(), want[tuple(p)].item()) for p in bad[:5]])


_STENCILS = {}


def _check_trav(m, h, st, what="", key=None, **kw):
    """traversability on the GPU against the model -> the model's result.  key: the stencil of an image is computed once and shared"""
    if key is None or key not in _STENCILS:
        sten = EI.stencil(h, st, EI.VS)
        if key is not None:
            _STENCILS[key] = sten
    else:
        sten = _STENCILS[key]
    o = EI.options(**kw)
    nk, step, slope2 = sten
    cls = EI.classes(st, nk, step, slope2, o)
    dist, mm = EI.distance(cls, o, EI.VS)
    got = m.traversability(h, st, step=True, slope=True, distance=True, **kw)
    assert sorted(got) == ["class", "distance", "slope2", "step"]
    _same_bytes(got["class"], cls, what + ": class")
    _same_bytes(got["step"], step, what + ": step")
    _same_bytes(got["slope2"], slope2, what + ": slope2")
    _same_bytes(got["distance"], dist, what + ": distance")
    return {"class": cls, "step": step, "slope2": slope2, "distance": dist, "m": mm}


def _staircase():
    """one block: column (vx, vy) is solid up to vz = vx and free above it (vx = 7: solid throughout); d0 = -0.01 vy, exactly 0 for vy = 0"""
    x, y, z = np.mgrid[0:8, 0:8, 0:8]
    return EI.block(np.where(z <= x, -0.01 * y, 0.03 + 0.001 * z).astype(F32))


# ---- 1. one block
def test_one_block_every_crossing_height(hip_lib):
    M, _ = _mods()
    b = (-2, 1, 3)
    box = (-16, 8, 8, 8, 20, 45)
    m = _mapper()
    EI.upload(m, M, {b: _staircase(), (b[0], b[1], b[2] + 1): EI.block(0.02)})
    h, st = _check_map(m, box, "staircase with the block above")
    assert (st == EI.SURFACE).all()
    for vx in range(8):
        assert h[0, vx] == _centre(24 + vx), vx                                # d0 == 0 exactly: the voxel centre, also across the block boundary
        assert (h[1:, vx] > _centre(24 + vx)).all() and (h[1:, vx] < _centre(24 + vx) + VS).all()
    m.close()
    m = _mapper()
    EI.upload(m, M, {b: _staircase()})
    h, st = _check_map(m, box, "staircase, the block above missing")
    assert (st[:, :7] == EI.SURFACE).all() and (st[:, 7] == EI.BLOCKED).all() and (h[:, 7] == F32(1000.0)).all()
    m.close()


# ---- 2. band edges
def test_band_edges(hip_lib):
    M, _ = _mods()
    m = _mapper()
    z = np.arange(8)[None, None, :]
    EI.upload(m, M, {(0, 0, 0): EI.block(np.where(z <= 3, -0.01, 0.02))})
    for band, want in (((0, 3), EI.BLOCKED), ((0, 4), EI.SURFACE), ((4, 7), EI.VOID), ((3, 3), EI.BLOCKED), ((5, 5), EI.VOID), ((9, 9), EI.UNKNOWN),
                       ((-3, 2), EI.BLOCKED), ((0, 1023), EI.SURFACE), ((-500, 523), EI.SURFACE), ((-1020, 3), EI.BLOCKED), ((-1019, 4), EI.SURFACE)):
        h, st = _check_map(m, (0, 0, 8, 8) + band, "band %s" % (band,))
        assert (st == want).all(), (band, want, np.unique(st))
        if want == EI.SURFACE:
            assert (h == _centre(3) + VS * (F32(0.01) / (F32(0.02) - F32(-0.01)))).all()
    m.close()
    # a band over three blocks, the middle one missing; in half of the columns an upper storey
    m = _mapper()
    x = np.arange(8)[:, None, None]
    EI.upload(m, M, {(0, 0, 0): EI.block(-0.01), (0, 0, 2): EI.block(np.where((x >= 4) & (z <= 1), -0.02, 0.02))})
    h, st = _check_map(m, (0, 0, 8, 8, 0, 23), "middle block missing")
    assert (st[:, :4] == EI.BLOCKED).all() and (st[:, 4:] == EI.SURFACE).all() and (h[:, 4:] == _centre(17) + VS * F32(0.5)).all()      # the upper one wins
    h, st = _check_map(m, (0, 0, 8, 8, 0, 17), "solid to the band's top above a floor")
    assert (st == EI.BLOCKED).all()
    m.close()


# ---- 3. the edge of "observed"
def test_observed_edge(hip_lib):
    M, _ = _mods()
    m = _mapper()
    x, y, z = np.mgrid[0:8, 0:8, 0:8]
    d = np.where(z <= 3, -0.01, 0.02).astype(F32)
    w = np.ones((8, 8, 8), F32)
    w[0] = F32(MW); w[1] = np.nextafter(F32(MW), F32(0)); w[2] = np.nan; w[5] = 0.0
    d[3, :, 4] = np.nan; d[4, :, 3] = np.nan
    color = np.zeros(512, M.COLOR_DT); color["weight"] = 1.0
    EI.upload(m, M, {(0, 0, 0): EI.block(d, w), (1, 0, 0): EI.block(-0.01, 0.0)})
    m.set_blocks(M.LAYER_COLOR, np.array([(2, 0, 0)], np.int32), color[None])
    assert (2, 0, 0) in H.idx_set(m.block_indices(M.LAYER_COLOR)) and (2, 0, 0) not in EI.read_tsdf(m, M)
    h, st = _check_map(m, (0, 0, 8, 32, 0, 9), "observed edge")
    assert st[0, :8].tolist() == [EI.SURFACE, EI.UNKNOWN, EI.UNKNOWN, EI.BLOCKED, EI.BLOCKED, EI.UNKNOWN, EI.SURFACE, EI.SURFACE]
    assert (st[:, 8:] == EI.UNKNOWN).all()                                     # weight 0; colour only; nothing
    h, st = _check_map(m, (0, 0, 8, 32, 0, 9), "min_weight 0", min_weight=0.0)
    assert (st[:, 8:16] == EI.BLOCKED).all() and (st[:, 16:] == EI.UNKNOWN).all() and st[0, 5] == EI.SURFACE      # the zeros of a block without the layer are not observed
    m.close()


# ---- 5. geometry
@pytest.fixture(scope="module")
def slope_map(hip_lib):
    """a tilted plane on negative and positive block indices, two blocks deep"""
    M, _ = _mods()
    m = _mapper()
    EI.upload(m, M, EI.heightfield_blocks(lambda X, Y: 0.11 * X - 0.07 * Y + 0.42, range(-2, 7), range(0, 2), range(0, 2)))
    yield m
    m.close()


@pytest.mark.parametrize("shape", ((1, 1), (7, 9), (8, 8), (9, 17), (64, 1), (1, 65)))
def test_unaligned_origin_and_image_sizes(slope_map, shape):
    import torch
    m = slope_map
    box = (-13, 5, shape[0], shape[1], 2, 13)
    want_h, want_s = _check_map(m, box, "%s at (-13, 5)" % (shape,))
    assert (want_s == EI.SURFACE).any()
    if shape == (64, 1):
        assert (want_s == EI.UNKNOWN).any()                                    # pixels over unallocated columns
    # preallocated outputs inside guard buffers: nothing outside rows x cols is written
    n = shape[0] * shape[1]; G = 300
    hb = torch.full((n + 2 * G,), SENTINEL, dtype=torch.float32, device="cuda"); sb = torch.full((n + 2 * G,), 99, dtype=torch.uint8, device="cuda")
    out = (hb[G:G + n].view(shape), sb[G:G + n].view(shape))
    got = m.elevation_map(*box, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    wrong = torch.zeros(shape, dtype=torch.int8, device="cuda")
    hb = hb.cpu().numpy(); sb = sb.cpu().numpy()
    assert hb[G:G + n].tobytes() == want_h.tobytes() and np.array_equal(sb[G:G + n].reshape(shape), want_s)
    assert (hb[:G] == SENTINEL).all() and (hb[G + n:] == SENTINEL).all() and (sb[:G] == 99).all() and (sb[G + n:] == 99).all()
    with pytest.raises(ValueError):
        m.elevation_map(*box, out=(out[0], wrong))
    with pytest.raises(ValueError):
        m.elevation_map(-13, 5, shape[0] + 1, shape[1], 2, 13, out=out)


def test_empty_map_is_all_unknown(hip_lib):
    m = _mapper(cap=64)
    h, st = _check_map(m, (-5, -5, 20, 70, -4, 30), "empty map", unknown_value=-3.5)
    assert (st == EI.UNKNOWN).all() and (h == F32(-3.5)).all()
    m.close()


# ---- 6. drawn maps
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_drawn_maps(hip_lib, seed):
    M, _ = _mods()
    m = _mapper()
    EI.upload(m, M, EI.drawn_map(seed))
    h, st = _check_map(m, EI.DRAWN_BOX, "drawn map %d" % seed)
    assert set(np.unique(st).tolist()) == {0, 1, 2, 3}
    m.close()


# ---- 7. traversability on drawn images
@pytest.fixture(scope="module")
def mp(hip_lib):
    m = _mapper(cap=64)
    yield m
    m.close()


def test_step_exactly_at_the_limit(mp):
    kw = dict(max_slope_tan=1000.0, min_known=1)
    for bump, want in ((F32(0.1), EI.T_OK), (np.nextafter(F32(0.1), F32(1)), EI.T_HAZARD)):
        h, st = EI.flat_image((3, 3), 0.0)
        h[1, 1] = bump
        t = _check_trav(mp, h, st, "step %r" % (bump,), **kw)
        assert (t["class"] == want).all() and (t["step"] == bump).all(), (bump, t["class"])


def test_ramp_exactly_at_the_limit(mp):
    kw = dict(min_known=1)
    for top, want in ((VS, EI.T_OK), (np.nextafter(VS, F32(1)), EI.T_HAZARD)):
        h, st = EI.flat_image((3, 3), 0.0)
        h[:, 1] = VS * F32(0.5); h[:, 2] = top
        t = _check_trav(mp, h, st, "ramp %r" % (top,), **kw)
        assert (t["slope2"][:, 0] == F32(0.25)).all() and (t["class"][:, 0] == EI.T_OK).all()      # one-sided at the border: exactly the limit
        assert (t["class"][:, 1] == want).all() and (t["class"][:, 2] == want).all(), (top, t["class"], t["slope2"])


def test_one_sided_differences_beside_unknown_pixels(mp):
    h = np.tile((F32(1.0) + F32(0.01) * np.arange(7, dtype=F32) ** 2)[None, :], (5, 1)).astype(F32)
    st = np.full((5, 7), EI.SURFACE, np.uint8)
    st[2, 3] = EI.UNKNOWN; st[0, 5] = EI.VOID; st[4, 1] = EI.BLOCKED
    h[st != EI.SURFACE] = F32(1000.0)                                          # never read: the status decides
    for kw in (dict(min_known=1), dict(min_known=1, void_is_hazard=1), {}):
        t = _check_trav(mp, h, st, "one-sided %r" % (kw,), **kw)
        assert t["class"][2, 3] == EI.T_UNKNOWN and t["class"][4, 1] == EI.T_HAZARD
        assert t["class"][0, 5] == (EI.T_HAZARD if kw.get("void_is_hazard") else EI.T_UNKNOWN)
        assert t["step"][2, 3] == 0 and t["slope2"][2, 3] == 0
    g = lambda a, b, d: (F32(a) - F32(b)) / d      # noqa: E731
    gl, gr = g(h[2, 2], h[2, 1], VS), g(h[2, 5], h[2, 4], VS)
    assert t["slope2"][2, 2] == gl * gl and t["slope2"][2, 4] == gr * gr      # left only, right only


@pytest.mark.parametrize("k", range(len(EI.IMAGE_SHAPES)))
def test_random_images_at_the_word_edges(mp, k):
    shape = EI.IMAGE_SHAPES[k]
    h, st = EI.random_image(shape, 20 + k)
    for kw in ({}, dict(min_known=1, void_is_hazard=1, distance_radius_px=1), dict(min_known=9, max_step_m=0.03, distance_radius_px=32)):
        t = _check_trav(mp, h, st, "%s %r" % (shape, kw), key=shape, **kw)
    if shape[0] > 3:
        assert set(np.unique(t["class"]).tolist()) == {0, 1, 2}


# ---- 8. distance
def test_one_hazard_in_the_middle_covers_every_distance(mp):
    import torch
    h, st = EI.flat_image((65, 65))
    st[32, 32] = EI.BLOCKED
    for R in (32, 15, 1, 0):
        t = _check_trav(mp, h, st, "R = %d" % R, key="middle", min_known=1, distance_radius_px=R)
        d = t["distance"]
        r, c = np.mgrid[0:65, 0:65]
        m2 = (r - 32) ** 2 + (c - 32) ** 2
        assert np.array_equal(t["m"][m2 <= R * R], m2[m2 <= R * R]) and (d[m2 > R * R] == VS * F32(R + 1)).all()
        if R:
            assert d[32, 32 + R] == VS * F32(R) and d[32 - R, 32] == VS * F32(R)                  # exactly R along an axis
        if R == 15:
            assert d[32 + 15, 32 + 1] == VS * F32(16) and d[32 - 1, 32 - 15] == VS * F32(16)      # dr^2 + dc^2 = R^2 + 1: out of reach
    assert len(np.unique(t["m"])) == 2 and d[32, 32] == 0
    # optional outputs left out: only what is asked for comes back, and through out= only what is handed in is written
    only = mp.traversability(h, st, distance=False, min_known=1)
    assert list(only) == ["class"] and np.array_equal(only["class"].cpu().numpy(), t["class"])
    cl = torch.full((65, 65), 9, dtype=torch.uint8, device="cuda"); sl = torch.full((65, 65), SENTINEL, dtype=torch.float32, device="cuda")
    got = mp.traversability(h, st, out=(cl, None, sl, None), min_known=1)
    assert sorted(got) == ["class", "slope2"] and got["class"] is cl and got["slope2"] is sl and (sl == 0).all().item()
    with pytest.raises(ValueError):
        mp.traversability(h, st, out=(cl, None, sl[:64], None))
    with pytest.raises(ValueError):
        mp.traversability(h, st[:64])


def test_hazards_in_the_corners_at_word_edges_and_none_at_all(mp):
    h, st = EI.flat_image((40, 130))
    t = _check_trav(mp, h, st, "no hazard", min_known=1, distance_radius_px=32)
    assert (t["distance"] == VS * F32(33)).all()
    for p in ((0, 0), (0, 129), (39, 0), (39, 129)):
        st[p] = EI.BLOCKED
    _check_trav(mp, h, st, "corners", min_known=1, distance_radius_px=32)
    _check_trav(mp, h, st, "corners, and the image's own with min_known 5", distance_radius_px=15)
    for col in (63, 64, 127, 128):
        h, st = EI.flat_image((3, 130))
        st[1, col] = EI.VOID
        t = _check_trav(mp, h, st, "column %d" % col, min_known=1, void_is_hazard=1, distance_radius_px=32)
        assert t["distance"][1, col - 32] == VS * F32(32) and t["distance"][1, col - 33] == VS * F32(33) and t["distance"][0, col + 1] == VS * np.sqrt(F32(2))


# ---- 9. end to end
def test_kerb_scene_from_the_map_to_a_path_over_the_ramp(hip_lib):
    M, _ = _mods()
    m = _mapper()
    EI.upload(m, M, EI.kerb_blocks())
    want_h, want_s = _check_map(m, EI.KERB_BOX, "kerb")
    want = EI.traversability(want_h, want_s)
    h, s = m.elevation_map(*EI.KERB_BOX)
    t = m.traversability(h, s)
    _same_bytes(t["class"], want["class"], "kerb: class")
    _same_bytes(t["distance"], want["distance"], "kerb: distance")
    src, start = np.array([[24, 4]], np.int32), np.array([[24, 44]], np.int32)
    G = m.cost_field(t["distance"], src, **EI.KERB_FIELD)
    o = PI.options(**EI.KERB_FIELD)
    want_G, n_acc = PI.field(want["distance"], src, o)
    assert n_acc == 1 and np.array_equal(G.cpu().numpy(), want_G)
    paths, lengths = m.trace_paths(t["distance"], G, start, 256, **EI.KERB_FIELD)
    want_path = PI.path(want["distance"], want_G, start[0], o)
    n = int(lengths.item())
    assert want_path and n == len(want_path) and n <= 256
    got = paths.cpu().numpy()[0, :n]
    assert np.array_equal(got, np.array(want_path, np.int32).reshape(n, 2)) and tuple(got[-1]) == (24, 4)
    on_ramp = got[np.isin(got[:, 1], EI.KERB_RAMP_COLS)]
    assert set(on_ramp[:, 1].tolist()) == set(EI.KERB_RAMP_COLS) and np.isin(on_ramp[on_ramp[:, 1] >= 29][:, 0], EI.KERB_RAMP_ROWS).all()      # it climbs the ramp
    assert want_G[24, 44] != PI.UNREACHED and (want["class"][12:31, 31] == EI.T_HAZARD).all()
    m.close()


def test_room_frames_map_unchanged_and_held_back_work_stays_held_back(hip_lib):
    """Two mappers with colour deferral on get the same frames; one of them makes both calls between pipelined frames.  Apart from the calls'
    own kernels it has launched exactly the same kernels as often, and its map is byte for byte the other's.  Over the slice's AABB the
    images have the slice image's shape."""
    M, S = _mods()
    sc = S.Scene()
    poses = [S.look_pose((1.0, 0.0, 1.5), np.pi, np.deg2rad(-10.0)), S.look_pose((-1.0, 0.0, 1.5), 0.0, np.deg2rad(-10.0))]
    A = _mapper(cap=1 << 12); B = _mapper(cap=1 << 12)
    own = ("k_elevation_scan", "k_terrain_classify", "k_terrain_distance")
    for m in (A, B):
        m.set_color_deferral(True); m.set_profiling(True)
    for k, T in enumerate(poses + poses[:1]):
        d, rgb = S.render(sc, T, CAM)
        for m in (A, B):
            m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM); m.update_esdf()
        if k == 1:
            h, s = A.elevation_map(-60, -60, 120, 120, -2, 40)
            A.traversability(h, s, step=True, slope=True)
    for m in (A, B):
        m.synchronize()
    pa = {k: v["count"] for k, v in A.profile().items() if not k.startswith("_") and not any(o in k for o in own)}
    pb = {k: v["count"] for k, v in B.profile().items() if not k.startswith("_")}
    assert pa == pb, (pa, pb)
    assert any(o in k for k in A.profile() for o in own)
    for m in (A, B):
        m.set_profiling(False)
    before = H.map_state(A)
    img, aabb = A.esdf_slice_image_device()
    box = A.elevation_box(aabb, -0.1, 2.0)                                      # (the room's floor is the plane z = 0: the band starts below it)
    assert box == EI.elevation_box(aabb, -0.1, 2.0, EI.VS) and (box[2], box[3]) == tuple(img.shape) and box[4] in (-3, -2) and box[5] == 40
    want_h, want_s = _check_map(A, box, "room")
    assert (want_s == EI.SURFACE).sum() > 500
    h, s = A.elevation_map(*box)
    t = A.traversability(h, s, step=True, slope=True)
    want = EI.traversability(want_h, want_s)
    for k in ("class", "step", "slope2", "distance"):
        _same_bytes(t[k], want[k], "room: " + k)
    assert tuple(t["distance"].shape) == tuple(img.shape)
    A.synchronize()
    H.assert_same_map(before, A, "before and after the two calls")
    H.assert_same_map(before, B, "against the mapper that never made them")
    A.close(); B.close()


# ---- 10. refusals
def test_refusals_launch_nothing_and_leave_the_mapper_usable(hip_lib):
    import torch
    M, _ = _mods()
    from isaac_ros_nvblox_amd import _lib
    m = _mapper(cap=64)
    z = np.arange(8)[None, None, :]
    EI.upload(m, M, {(0, 0, 0): EI.block(np.where(z <= 3, -0.01, 0.02))})
    m.synchronize(); m.set_profiling(True)
    lib, h = m.lib, m._h
    hgt = torch.zeros((8, 8), dtype=torch.float32, device="cuda"); st = torch.ones((8, 8), dtype=torch.uint8, device="cuda")
    cls = torch.zeros((8, 8), dtype=torch.uint8, device="cuda"); f1 = torch.zeros((8, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan = float("nan")
    L = 1 << 23

    def em(mapper=h, x0=0, y0=0, rows=8, cols=8, zlo=0, zhi=7, mw=1e-4, uv=1000.0, hd=p(hgt), sd=p(st)):
        return lib.nvbx_elevation_map(mapper, x0, y0, rows, cols, zlo, zhi, mw, uv, hd, sd)

    def tr(mapper=h, hd=p(hgt), sd=p(st), rows=8, cols=8, o=None, c=p(cls), a=p(f1), b=None, d=None, **kw):
        return lib.nvbx_traversability(mapper, hd, sd, rows, cols, C.byref(_lib.TerrainOptions(**EI.options(**kw))) if o is None else o, c, a, b, d)
    null_options = C.POINTER(_lib.TerrainOptions)()
    refused = [
        lambda: em(mapper=None), lambda: em(hd=None), lambda: em(sd=None),
        lambda: em(rows=0), lambda: em(cols=0), lambda: em(rows=-1), lambda: em(cols=-8), lambda: em(rows=2049, cols=2048), lambda: em(rows=1 << 16, cols=1 << 16),
        lambda: em(zlo=4, zhi=3), lambda: em(zlo=0, zhi=1024), lambda: em(zlo=-(1 << 31), zhi=(1 << 31) - 1),
        lambda: em(x0=-L - 1), lambda: em(x0=L - 7), lambda: em(y0=-L - 1), lambda: em(y0=L - 7), lambda: em(zlo=-L - 1, zhi=-L), lambda: em(zlo=L - 1, zhi=L),
        lambda: em(x0=(1 << 31) - 4), lambda: em(mw=nan), lambda: em(uv=nan),
        lambda: tr(mapper=None), lambda: tr(hd=None), lambda: tr(sd=None), lambda: tr(o=null_options), lambda: tr(c=None),
        lambda: tr(rows=0), lambda: tr(cols=0), lambda: tr(rows=-1), lambda: tr(cols=-8), lambda: tr(rows=2049, cols=2048), lambda: tr(rows=1 << 16, cols=1 << 16),
        lambda: tr(max_step_m=nan), lambda: tr(max_step_m=-0.01), lambda: tr(max_slope_tan=nan), lambda: tr(max_slope_tan=-0.5), lambda: tr(unknown_value=nan),
        lambda: tr(min_known=0), lambda: tr(min_known=10), lambda: tr(distance_radius_px=-1), lambda: tr(distance_radius_px=33),
    ]
    for i, call in enumerate(refused):
        assert call() == E_INVALID, "refusal %d" % i
        assert lib.nvbx_last_error(), "refusal %d" % i
    m.synchronize()
    assert not any(k.startswith("k_") for k in m.profile()), list(m.profile())        # nothing was launched
    m.set_profiling(False)
    # an occupancy mapper has no TSDF layer
    occ = _mapper(cap=64, projective_layer_type=1)
    assert lib.nvbx_elevation_map(occ._h, 0, 0, 8, 8, 0, 7, 1e-4, 1000.0, p(hgt), p(st)) == E_INVALID
    with pytest.raises(M.NvbxError):
        occ.elevation_map(0, 0, 8, 8, 0, 7)
    occ.close()
    # the limits themselves are not refusals
    assert em(x0=-L, y0=-L) == 0 and em(x0=L - 8, y0=L - 8) == 0 and em(zlo=-L, zhi=-L + 1023) == 0 and em(zlo=L - 1024, zhi=L - 1) == 0
    assert tr(a=None) == 0 and tr(d=p(f1), distance_radius_px=0) == 0 and tr(min_known=9, distance_radius_px=32, max_step_m=0.0, max_slope_tan=0.0) == 0
    with pytest.raises(M.NvbxError):
        m.traversability(hgt, st, min_known=12)
    with pytest.raises(TypeError):
        m.traversability(hgt, st, no_such_option=1)
    with pytest.raises(M.NvbxError):
        m.elevation_map(0, 0, 8, 8, 5, 4)
    h2, st2 = _check_map(m, (0, 0, 8, 8, 0, 7), "after the refusals")
    assert (st2 == EI.SURFACE).all()
    m.close()
