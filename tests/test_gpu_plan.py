"""The cost field and its paths on the GPU (nvbx_cost_field / nvbx_trace_paths; SEMANTICS.md "Cost field and paths") against the scipy model of
tests/plan_independent.py: fields and paths are compared exactly.  Images are handed in as tensors; the end-to-end test slices a map made of two
80 x 60 frames of the synthetic room.  block_capacity at most 1 << 12."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import plan_independent as PI

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05
F32 = np.float32
SENTINEL = -77
E_INVALID = -1
KNOBS = ("NVBX_PLAN_ROUNDS_PER_WAIT", "NVBX_PLAN_TILE_SWEEPS")


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


@pytest.fixture(scope="module")
def mp(hip_lib):
    M, _ = _mods()
    m = M.Mapper(M.default_params(), device=0, block_capacity=64)
    yield m
    m.close()


@pytest.fixture(scope="module")
def cases():
    return PI.random_cases()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _field(m, img, sources, **okw):
    """cost_field on the GPU -> (G numpy int32, accepted)"""
    import torch
    acc = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    G = m.cost_field(_dev(img), np.asarray(sources, np.int32).reshape(-1, 2), accepted=acc, **okw)
    assert G.dtype == torch.int32 and tuple(G.shape) == img.shape
    return G.cpu().numpy(), int(acc.item())


def _check_field(m, img, sources, what="", **okw):
    """the GPU's field and accepted count equal the model's, exactly -> the field"""
    want, n_acc = PI.field(img, sources, PI.options(**okw))
    got, acc = _field(m, img, sources, **okw)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:5]])
    assert acc == n_acc, (what, acc, n_acc)
    return got


def _check_paths(m, img, G, starts, capacity, what="", **okw):
    """trace_paths on the GPU against the model's walk: lengths, the pixels up to the capacity, and nothing written beyond a path's end"""
    import torch
    starts = np.asarray(starts, np.int32).reshape(-1, 2)
    paths = torch.full((len(starts), capacity, 2), SENTINEL, dtype=torch.int32, device="cuda")
    lengths = torch.full((len(starts),), SENTINEL, dtype=torch.int32, device="cuda")
    out = m.trace_paths(_dev(img), _dev(G), starts, capacity, out=(paths, lengths), **okw)
    assert out[0] is paths and out[1] is lengths
    paths = paths.cpu().numpy(); lengths = lengths.cpu().numpy()
    o = PI.options(**okw)
    for i, s in enumerate(starts):
        want = PI.path(img, G, s, o)
        assert int(lengths[i]) == (-1 if want is None else len(want)), (what, i, s.tolist(), int(lengths[i]), want if want is None else len(want))
        if want is None:
            continue
        k = min(len(want), capacity)
        assert np.array_equal(paths[i, :k], np.array(want[:k], np.int32).reshape(k, 2)), (what, i, s.tolist())
        assert (paths[i, k:] == SENTINEL).all(), (what, i, "written beyond the path's end or the capacity")
    return lengths


# ---- 1. sizes around the tile
@pytest.mark.parametrize("shape", PI.LINE_SHAPES)
def test_one_row_and_one_column_images(mp, shape):
    img, sources = PI.line_case(shape)
    G = _check_field(mp, img, sources, "line %s" % (shape,), **PI.CASE_OPTIONS)
    if img.size > 1:
        flat = G.reshape(-1)
        assert flat[96] == 640 and (flat[97:] == PI.UNREACHED).all() and flat[31] == flat[32] == 0      # the blocked pixel ends the line
        _check_paths(mp, img, G, [np.unravel_index(i, shape) for i in (96, 0, 64, 97, 129)], 80, "line", **PI.CASE_OPTIONS)
    else:
        assert G.tolist() == [[0]]
        assert _check_paths(mp, img, G, [(0, 0), (0, 1)], 4, "1 x 1", **PI.CASE_OPTIONS).tolist() == [1, 0]


@pytest.mark.parametrize("k", range(len(PI.RANDOM_SHAPES) * PI.SEEDS_PER_SHAPE))
def test_random_images_fields_and_paths(mp, cases, k):
    shape, seed, img, sources = cases[k]
    what = "%s seed %d" % (shape, seed)
    G = _check_field(mp, img, sources, what, **PI.CASE_OPTIONS)
    rng = np.random.default_rng(100 + k)
    reach = np.argwhere(G != PI.UNREACHED)
    starts = list(reach[rng.choice(len(reach), 16, replace=False)])
    starts += [np.argwhere(G == PI.UNREACHED)[0], (-1, 0), (0, -1), (shape[0], 0), (0, shape[1])]      # unreached, out of the image: 0
    lengths = _check_paths(mp, img, G, starts, 2 * (shape[0] + shape[1]), what, **PI.CASE_OPTIONS)
    assert (lengths[:16] >= 1).all() and (lengths[16:] == 0).all()


SOURCE_ON_THE_RIM = (      # (shape, blocked pixels, source, reached pixels, {pixel: cost}): figures from PI.field on the CPU
    ((33, 33), (), (32, 32), 1089, {(0, 0): 448, (31, 31): 14}),                          # the source is alone in its 1 x 1 tile
    ((65, 33), (), (32, 32), 2145, {}),                                                   # ... in a 1 x 32 tile: the control
    ((64, 64), ((30, 30), (30, 31), (31, 30)), (31, 31), 4093, {(32, 32): 14}),           # ... in a full tile that it can leave only across the rim
)


@pytest.mark.parametrize("shape,blocked,source,reached,values", SOURCE_ON_THE_RIM)
def test_a_source_wakes_the_tiles_that_hold_it_in_their_halo(mp, shape, blocked, source, reached, values):
    """A source's 0 is a value no relaxation stores: the classify launch has to wake the neighbouring tiles itself."""
    img = np.full(shape, F32(5.0))
    for p in blocked:
        img[p] = PI.BLOCKED
    what = "%s, source %s" % (shape, source)
    G = _check_field(mp, img, [source], what)
    assert int((G != PI.UNREACHED).sum()) == reached, what
    for p, v in values.items():
        assert G[p] == v, (what, p, int(G[p]), v)
    assert G[0, 0] == G[G != PI.UNREACHED].max(), what                                   # the far corner; its path crosses every tile boundary
    assert _check_paths(mp, img, G, [(0, 0)], shape[0] + shape[1], what)[0] >= 33


# ---- 2. many rounds, and the two knobs
def test_serpentine_under_every_knob_setting(mp):
    img, sources = PI.serpentine(96)
    want, _ = PI.field(img, sources, PI.options())
    assert int(want[want != PI.UNREACHED].max()) == 46550
    far = np.unravel_index(np.argmax(np.where(want == PI.UNREACHED, -1, want)), want.shape)
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for rounds, sweeps in (("1", None), ("64", None), ("1", "1"), ("64", "1"), (None, None)):
            for k, v in zip(KNOBS, (rounds, sweeps)):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
            mp.reload_knobs()
            G = _check_field(mp, img, sources, "serpentine, rounds per wait %s, tile sweeps %s" % (rounds, sweeps))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        mp.reload_knobs()
    assert _check_paths(mp, img, G, [far], 5000, "serpentine, ample").tolist() == [4656]
    assert _check_paths(mp, img, G, [far, (0, 5)], 10, "serpentine, capacity 10").tolist() == [4656, 6]      # the length is still reported


# ---- 3. no corner is cut
def test_corner_cutting(mp):
    img = np.full((9, 9), F32(0.9))
    img[:, 4] = PI.BLOCKED; img[4, :] = PI.BLOCKED      # four rooms
    img[4, 4] = F32(0.9)                                # the crossing is free: (3, 4)/(4, 3) and (5, 4)/(4, 5) still touch only diagonally
    G = _check_field(mp, img, [(0, 0)], "walled")
    assert G[4, 4] == PI.UNREACHED and (G[5:, 5:] == PI.UNREACHED).all() and G[3, 3] == 42
    two = np.full((5, 5), PI.BLOCKED); two[0:2, 0:2] = F32(0.9); two[2:4, 2:4] = F32(0.9)      # (1, 1) and (2, 2) touch diagonally, both edge pixels blocked
    G = _check_field(mp, two, [(0, 0)], "diagonal touch")
    assert G[1, 1] == 14 and (G[2:, 2:] == PI.UNREACHED).all()
    two[1, 2] = F32(0.9)                                                                        # one of the two edge pixels opens: connected, along the axes
    G = _check_field(mp, two, [(0, 0)], "one edge pixel open")
    assert G[2, 2] == 14 + 10 + 10 and G[3, 3] == 48
    _check_paths(mp, two, G, [(3, 3), (2, 2), (4, 4)], 8, "one edge pixel open")


# ---- 4. the edges of every class and penalty
@pytest.mark.parametrize("k", range(len(PI.EDGE_OPTIONS)))
def test_class_edges(mp, k):
    okw = PI.EDGE_OPTIONS[k]
    o = PI.options(**okw)
    v = PI.edge_values(o)
    img = np.full((3, len(v)), F32(5.0))      # a free corridor above, the edge values below it, a wall beneath them
    img[1] = v; img[2] = PI.BLOCKED
    G = _check_field(mp, img, [(0, 0)], "edges %r" % (okw,), **okw)
    trav, pen = PI.classify(v.reshape(1, -1), o)
    assert np.array_equal(G[1] != PI.UNREACHED, trav[0])
    assert trav[0, 0] == (o["robot_radius_m"] > 0) and not trav[0, 1]                           # v == robot_radius_m passes, one ulp below does not
    assert not trav[0, [3, 4, 5, 6, 8]].any() or o["unknown_value"] < 0                         # 0, -0, negative, NaN and -inf are not traversable
    if "unknown_value" not in okw:
        assert trav[0, 7] and np.array_equal(trav[0, 10:15], [bool(o["allow_unknown"])] * 3 + [True] * 2)      # within 1e-2 of unknown_value, and just outside
        if o["allow_unknown"]:
            assert G[1, 10] == G[0, 10] + 10 + o["unknown_penalty"]


# ---- 5. sources
def test_sources(mp, cases):
    import torch
    shape, seed, img, sources = cases[7]
    kw = PI.CASE_OPTIONS
    blocked = [tuple(int(v) for v in p) for p in np.argwhere(~PI.classify(img, PI.options(**kw))[0])[:3]]
    outside = [(-1, 0), (0, -1), (shape[0], 0), (0, shape[1]), (-2 ** 31, 5), (2 ** 31 - 1, 2 ** 31 - 1)]
    G, acc = _field(mp, img, np.zeros((0, 2), np.int32), **kw)
    assert acc == 0 and (G == PI.UNREACHED).all()                                               # none
    G, acc = _field(mp, img, blocked + outside, **kw)
    assert acc == 0 and (G == PI.UNREACHED).all()                                               # all rejected
    one = _check_field(mp, img, sources[:1], "one source", **kw)
    many = [tuple(sources[0])] * 5 + blocked + outside + [tuple(sources[0])]
    G, acc = _field(mp, img, many, **kw)
    assert acc == 6 and np.array_equal(G, one)                                                  # duplicates and rejected entries change nothing
    _check_field(mp, img, list(map(tuple, sources)) + outside + blocked, "all three", **kw)
    # a device tensor of sources and a preallocated field
    out = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
    assert mp.cost_field(_dev(img), _dev(sources[:1]), out=out, **kw) is out and np.array_equal(out.cpu().numpy(), one)


# ---- 6. a field that does not belong to the image
def test_a_foreign_field_gives_minus_one_not_an_error(mp, cases):
    (_, _, img_a, src_a), (_, _, img_b, _) = cases[3], cases[4]
    assert img_a.shape == img_b.shape
    Ga = _check_field(mp, img_a, src_a, **PI.CASE_OPTIONS)
    starts = np.argwhere(Ga != PI.UNREACHED)
    lengths = _check_paths(mp, img_b, Ga, starts, 4, "foreign field", **PI.CASE_OPTIONS)
    assert (lengths == -1).any()
    _check_field(mp, img_b, src_a, "after the foreign field", **PI.CASE_OPTIONS)              # the mapper is usable


# ---- 7. refusals
def test_refusals_launch_nothing_and_leave_the_mapper_usable(hip_lib):
    import torch
    M, _ = _mods()
    from isaac_ros_nvblox_amd import _lib
    m = M.Mapper(M.default_params(), device=0, block_capacity=64)
    m.synchronize(); m.set_profiling(True)
    lib, h = m.lib, m._h
    img = torch.full((8, 8), 0.9, dtype=torch.float32, device="cuda"); cost = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    rc2 = torch.zeros((2, 2), dtype=torch.int32, device="cuda"); acc = torch.zeros(1, dtype=torch.int32, device="cuda")
    paths = torch.zeros((2, 4, 2), dtype=torch.int32, device="cuda"); lens = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan = float("nan")

    def opt(**kw):
        return C.byref(_lib.CostOptions(**PI.options(**kw)))

    def cf(mapper=h, i=p(img), rows=8, cols=8, o=None, s=p(rc2), n=2, c=p(cost), a=p(acc), **kw):
        return lib.nvbx_cost_field(mapper, i, rows, cols, opt(**kw) if o is None else o, s, n, c, a)

    def tp(mapper=h, i=p(img), rows=8, cols=8, o=None, c=p(cost), s=p(rc2), n=2, pa=p(paths), cap=4, ln=p(lens), **kw):
        return lib.nvbx_trace_paths(mapper, i, rows, cols, opt(**kw) if o is None else o, c, s, n, pa, cap, ln)
    null_options = C.POINTER(_lib.CostOptions)()
    refused = []
    for f in (cf, tp):
        refused += [
            lambda f=f: f(mapper=None), lambda f=f: f(i=None), lambda f=f: f(o=null_options), lambda f=f: f(c=None),
            lambda f=f: f(rows=0), lambda f=f: f(cols=0), lambda f=f: f(rows=-1), lambda f=f: f(cols=-8), lambda f=f: f(rows=2049, cols=2048), lambda f=f: f(rows=1 << 16, cols=1 << 16),
            lambda f=f: f(robot_radius_m=nan), lambda f=f: f(robot_radius_m=-0.1), lambda f=f: f(inflation_radius_m=nan), lambda f=f: f(inflation_radius_m=-0.1),
            lambda f=f: f(penalty_per_m=nan), lambda f=f: f(penalty_per_m=-1.0), lambda f=f: f(unknown_value=nan),
            lambda f=f: f(max_penalty=-1), lambda f=f: f(max_penalty=201), lambda f=f: f(unknown_penalty=-1), lambda f=f: f(unknown_penalty=201),
            lambda f=f: f(n=-1), lambda f=f: f(s=None),
        ]
    refused += [lambda: tp(pa=None), lambda: tp(ln=None), lambda: tp(cap=-1)]
    for i, call in enumerate(refused):
        assert call() == E_INVALID, "refusal %d" % i
        assert lib.nvbx_last_error(), "refusal %d" % i
    m.synchronize()
    assert not any(k.startswith("k_") for k in m.profile()), list(m.profile())        # nothing was launched
    m.set_profiling(False)
    assert cf(a=None) == 0 and cf(s=None, n=0) == 0 and tp(s=None, pa=None, ln=None, n=0) == 0 and tp(cap=0) == 0      # not refusals
    with pytest.raises(M.NvbxError):
        m.cost_field(img, [(0, 0)], max_penalty=500)
    with pytest.raises(TypeError):
        m.cost_field(img, [(0, 0)], no_such_option=1)
    G = _check_field(m, np.full((8, 8), F32(0.9)), [(0, 0)], "after the refusals")
    assert G[7, 7] == 98
    m.close()


# ---- 8. end to end: from a mapped room to a priced goal and the way there
@pytest.fixture(scope="module")
def room(hip_lib):
    """two 80 x 60 frames that look at each other's standpoint, so each camera stands on floor the other one saw; ESDF updated"""
    M, S = _mods()
    m = M.Mapper(M.default_params(), device=0, block_capacity=1 << 12)
    sc = S.Scene()
    poses = [S.look_pose((1.0, 0.0, 1.5), np.pi, np.deg2rad(-10.0)), S.look_pose((-1.0, 0.0, 1.5), 0.0, np.deg2rad(-10.0))]
    for T in poses:
        d, rgb = S.render(sc, T, CAM)
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM)
    m.update_esdf()
    m.synchronize()
    yield m, poses
    m.close()


def test_end_to_end_from_the_map_to_a_priced_goal(room):
    import torch
    M, _ = _mods()
    m, poses = room
    kw = dict(robot_radius_m=0.10, inflation_radius_m=0.5)
    before = H.map_state(m)
    img_dev, aabb = m.esdf_slice_image_device()
    img = img_dev.cpu().numpy()
    src = m.slice_pixels(poses[1][:2, 3].reshape(1, 2), aabb)
    assert 0 <= src[0, 0] < img.shape[0] and 0 <= src[0, 1] < img.shape[1], (src, img.shape)
    acc = torch.zeros(1, dtype=torch.int32, device="cuda")
    G_dev = m.cost_field(img_dev, src, accepted=acc, **kw)
    G = G_dev.cpu().numpy()
    want, n_acc = PI.field(img, src, PI.options(**kw))
    assert n_acc == 1 and int(acc.item()) == 1, "the camera does not stand on traversable floor: v = %r" % (img[src[0, 0], src[0, 1]],)
    assert np.array_equal(G, want) and (G != PI.UNREACHED).sum() > 500
    # the frontier clusters' centroids, priced by a lookup
    comps = m.frontier_clusters(min_voxels=4)[4]
    goals = m.slice_pixels(comps.centroid_m.cpu().numpy()[:, :2], aabb)
    inside = (goals[:, 0] >= 0) & (goals[:, 0] < img.shape[0]) & (goals[:, 1] >= 0) & (goals[:, 1] < img.shape[1])
    goals = goals[inside]
    price = G[goals[:, 0], goals[:, 1]]
    assert (price != PI.UNREACHED).any(), (len(goals), "no frontier centroid is reachable")
    best = goals[int(np.argmin(price))]
    paths, lengths = m.trace_paths(img_dev, G_dev, best.reshape(1, 2), 1024, **kw)
    n = int(lengths.item())
    want_path = PI.path(img, want, best, PI.options(**kw))
    assert n == len(want_path) >= 1 and n <= 1024
    got = paths.cpu().numpy()[0, :n]
    assert np.array_equal(got, np.array(want_path, np.int32).reshape(n, 2)) and tuple(got[-1]) == tuple(src[0])      # it reaches the source
    m.synchronize()
    H.assert_same_map(before, m, "before and after the cost field and the paths")             # the calls write nothing to the map


def test_slice_pixels_puts_the_surface_voxels_on_the_pixels_with_v_at_most_zero(room):
    """Pins the metres -> pixel formula: the voxels of the slice plane that are sites or inside a surface (the room's walls, box and sphere: not
    symmetric under a swap or a flip of the axes), taken from the ESDF layer, land through slice_pixels on exactly the pixels with v <= 0."""
    M, _ = _mods()
    m, _ = room
    img, aabb = m.esdf_slice_image()
    idx = np.asarray(m.block_indices(M.LAYER_ESDF), np.int32).reshape(-1, 3)
    blocks, found = m.get_blocks(M.LAYER_ESDF, idx)
    assert np.all(found)
    kz = int(np.floor(F32(m.params.esdf_slice_height) / F32(VS)))
    centres = []
    for b, vox in zip(idx, np.asarray(blocks).reshape(len(idx), 512)):
        if b[2] != kz >> 3:
            continue
        plane = vox.reshape(8, 8, 8)[:, :, kz & 7]                                             # voxel z + 8 y + 64 x -> [x, y]
        on = (plane["observed"] != 0) & ((plane["squared_distance_vox"] == 0) | (plane["is_inside"] != 0))
        for vx, vy in np.argwhere(on):
            centres.append(((8 * b[0] + vx + 0.5) * VS, (8 * b[1] + vy + 0.5) * VS))
    assert len(centres) > 50
    px = m.slice_pixels(np.array(centres), aabb)
    assert len(set(map(tuple, px.tolist()))) == len(px)
    want = np.zeros(img.shape, bool)
    want[px[:, 0], px[:, 1]] = True
    assert np.array_equal(want, img <= 0), (int(want.sum()), int((img <= 0).sum()))
    # the AABB starts at a block's min corner: pixel (0, 0) is the voxel that holds it
    assert m.slice_pixels([(aabb[0] + 0.01, aabb[1] + 0.01), (aabb[0] - 0.01, aabb[1] + 0.06)], aabb).tolist() == [[0, 0], [1, -1]]
