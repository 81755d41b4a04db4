"""The cost volume and its 3-D paths on the GPU (nvbx_cost_volume / nvbx_trace_paths_3d; SEMANTICS.md "Cost volume and 3-D paths") against the
scipy model of tests/plan3d_independent.py: fields and paths are compared exactly.  Volumes are handed in as tensors; the end-to-end test takes
the dense ESDF box of a 3-D-mode map made of two 80 x 60 frames of the synthetic room.  block_capacity at most 1 << 12."""
import ctypes as C
import os

import numpy as np
import pytest

import helpers as H
import plan3d_independent as P3

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
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
    return P3.random_cases()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _field(m, vol, sources, **okw):
    """cost_volume on the GPU -> (G numpy int32, accepted)"""
    import torch
    acc = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    G = m.cost_volume(_dev(vol), np.asarray(sources, np.int32).reshape(-1, 3), accepted=acc, **okw)
    assert G.dtype == torch.int32 and tuple(G.shape) == vol.shape
    return G.cpu().numpy(), int(acc.item())


def _check_field(m, vol, sources, what="", **okw):
    """the GPU's field and accepted count equal the model's, exactly -> the field"""
    want, n_acc = P3.field(vol, sources, P3.options(**okw))
    got, acc = _field(m, vol, sources, **okw)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), [(tuple(int(v) for v in p), int(got[tuple(p)]), int(want[tuple(p)])) for p in bad[:5]])
    assert acc == n_acc, (what, acc, n_acc)
    return got


def _check_paths(m, vol, G, starts, capacity, what="", **okw):
    """trace_paths_3d on the GPU against the model's walk: lengths, the voxels up to the capacity, and nothing written beyond a path's end"""
    import torch
    starts = np.asarray(starts, np.int32).reshape(-1, 3)
    paths = torch.full((len(starts), capacity, 3), SENTINEL, dtype=torch.int32, device="cuda")
    lengths = torch.full((len(starts),), SENTINEL, dtype=torch.int32, device="cuda")
    out = m.trace_paths_3d(_dev(vol), _dev(G), starts, capacity, out=(paths, lengths), **okw)
    assert out[0] is paths and out[1] is lengths
    paths = paths.cpu().numpy(); lengths = lengths.cpu().numpy()
    o = P3.options(**okw)
    for i, s in enumerate(starts):
        want = P3.path(vol, G, s, o)
        assert int(lengths[i]) == (-1 if want is None else len(want)), (what, i, s.tolist(), int(lengths[i]), want if want is None else len(want))
        if want is None:
            continue
        k = min(len(want), capacity)
        assert np.array_equal(paths[i, :k], np.array(want[:k], np.int32).reshape(k, 3)), (what, i, s.tolist())
        assert (paths[i, k:] == SENTINEL).all(), (what, i, "written beyond the path's end or the capacity")
    return lengths


def _outside(shape):
    """a start beyond every face of the box"""
    return [(-1, 0, 0), (0, -1, 0), (0, 0, -1), (shape[0], 0, 0), (0, shape[1], 0), (0, 0, shape[2])]


# ---- 1. sizes around the tile
@pytest.mark.parametrize("shape", P3.LINE_SHAPES)
def test_single_voxel_and_lines_along_each_axis(mp, shape):
    vol, sources = P3.line_case(shape)
    G = _check_field(mp, vol, sources, "line %s" % (shape,), **P3.CASE_OPTIONS)
    if vol.size > 1:
        flat = G.reshape(-1)
        assert flat[119] == 550 and (flat[120:] == P3.UNREACHED).all() and flat[63] == flat[64] == 0 and flat[32] == 310      # the blocked voxel ends the line
        _check_paths(mp, vol, G, [np.unravel_index(i, shape) for i in (119, 0, 32, 90, 120, 129)], 80, "line", **P3.CASE_OPTIONS)
    else:
        assert G.tolist() == [[[0]]]
        assert _check_paths(mp, vol, G, [(0, 0, 0), (0, 0, 1)], 4, "1 x 1 x 1", **P3.CASE_OPTIONS).tolist() == [1, 0]


@pytest.mark.parametrize("k", range(len(P3.TILE_SHAPES)))
def test_shapes_on_beside_and_across_the_tile(mp, k):
    shape, vol, sources = P3.tile_cases()[k]
    G = _check_field(mp, vol, sources, "tile shape %s" % (shape,), **P3.CASE_OPTIONS)
    assert (G != P3.UNREACHED).sum() >= len(sources)
    reach = np.argwhere(G != P3.UNREACHED)
    _check_paths(mp, vol, G, list(reach[:: max(1, len(reach) // 8)]) + _outside(shape), 64, "tile shape %s" % (shape,), **P3.CASE_OPTIONS)
    empty = np.full(shape, F32(5.0))                                  # and the closed form, from the far corner
    far = tuple(s - 1 for s in shape)
    G = _check_field(mp, empty, [far], "empty %s" % (shape,))
    off = np.sort(np.stack(np.meshgrid(*[s - 1 - np.arange(s) for s in shape], indexing="ij"), -1), -1)
    assert np.array_equal(G, 17 * off[..., 0] + 14 * (off[..., 1] - off[..., 0]) + 10 * (off[..., 2] - off[..., 1]))


# ---- 2. random volumes: fields and paths
@pytest.mark.parametrize("k", range(len(P3.RANDOM_SHAPES) * P3.SEEDS_PER_SHAPE))
def test_random_volumes_fields_and_paths(mp, cases, k):
    shape, seed, vol, sources = cases[k]
    what = "%s seed %d" % (shape, seed)
    G = _check_field(mp, vol, sources, what, **P3.CASE_OPTIONS)
    rng = np.random.default_rng(100 + k)
    reach = np.argwhere(G != P3.UNREACHED)
    starts = list(reach[rng.choice(len(reach), 16, replace=False)])
    starts += [np.argwhere(G == P3.UNREACHED)[0]] + _outside(shape)                             # unreached, out of the box on every face: 0
    lengths = _check_paths(mp, vol, G, starts, 2 * sum(shape), what + ", ample", **P3.CASE_OPTIONS)
    assert (lengths[:16] >= 1).all() and (lengths[16:] == 0).all() and lengths.max() <= 2 * sum(shape)
    small = _check_paths(mp, vol, G, starts, 3, what + ", capacity 3", **P3.CASE_OPTIONS)      # the lengths are still reported
    assert np.array_equal(small, lengths) and lengths.max() > 3


# ---- 3. no corner is cut: every subset of the voxels between, for the space diagonal and the three face diagonals
def test_corner_rule_exhaustive(mp):
    vol, sources, cells = P3.corner_cells()
    G = _check_field(mp, vol, sources, "corner cells")
    want, _ = P3.field(vol, sources, P3.options())
    for low, far, shut, d in cells:
        assert G[far] == want[far], (low, shut)
        if sum(d) == 3:
            assert (G[far] == 17) == (len(shut) == 0), (low, shut, int(G[far]))
        else:
            assert int(G[far]) == (14, 20, P3.UNREACHED)[len(shut)], (low, shut, int(G[far]))
    _check_paths(mp, vol, G, [far for _, far, _, _ in cells], 8, "corner cells")


# ---- 4. many rounds through every tile, and the two knobs
def test_serpentine_under_every_knob_setting(mp):
    vol, sources = P3.serpentine(24)
    want, _ = P3.field(vol, sources, P3.options())
    assert int(want[want != P3.UNREACHED].max()) == 4094 and want[23, 0, 0] == 4094
    saved = {k: os.environ.get(k) for k in KNOBS}
    fields = []
    try:
        for rounds, sweeps in (("1", None), ("64", None), ("1", "1"), ("64", "1"), (None, None)):
            for k, v in zip(KNOBS, (rounds, sweeps)):
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
            mp.reload_knobs()
            fields.append(_check_field(mp, vol, sources, "serpentine, rounds per wait %s, tile sweeps %s" % (rounds, sweeps)))
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        mp.reload_knobs()
    assert all(np.array_equal(f, fields[0]) for f in fields[1:])
    G = fields[-1]
    assert _check_paths(mp, vol, G, [(23, 0, 0)], 400, "serpentine, ample").tolist() == [300]
    assert _check_paths(mp, vol, G, [(23, 0, 0), (0, 5, 5)], 4, "serpentine, capacity 4").tolist() == [300, 6]


# ---- 5. options and stored values of every kind
@pytest.mark.parametrize("k", range(len(P3.OPTION_SETS)))
def test_options_and_special_values(mp, k):
    okw = P3.OPTION_SETS[k]
    vol, sources = P3.special_values_volume()
    assert np.isnan(vol).any() and np.isposinf(vol).any() and np.isneginf(vol).any() and (vol < 0).any()
    G = _check_field(mp, vol, sources, "options %r" % (okw,), **okw)
    trav, pen = P3.classify(vol, P3.options(**okw))
    assert (G[~trav] == P3.UNREACHED).all() and (G != P3.UNREACHED).sum() > vol.size // 4
    assert not trav[np.isnan(vol) | (vol < 0) | (vol == 0)].any() and trav[np.isposinf(vol)].all()
    if okw.get("allow_unknown"):
        unknown = np.abs(vol - P3.UNKNOWN) < 1e-6
        assert trav[unknown].all() and (pen[unknown] == okw["unknown_penalty"]).all() and (G[unknown] != P3.UNREACHED).any()
    if okw.get("penalty_per_m", 0) >= 1000.0:
        assert (pen[trav & np.isfinite(vol)] == 200).all()                                      # every finite traversable voxel sits on the clamp
    reach = np.argwhere(G != P3.UNREACHED)
    _check_paths(mp, vol, G, reach[:: len(reach) // 8][:8], sum(vol.shape), "options %r" % (okw,), **okw)


# ---- 6. sources
def test_sources(mp, cases):
    import torch
    shape, seed, vol, sources = cases[1]
    kw = P3.CASE_OPTIONS
    blocked = [tuple(int(v) for v in p) for p in np.argwhere(~P3.classify(vol, P3.options(**kw))[0])[:3]]
    outside = _outside(shape) + [(-2 ** 31, 5, 5), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    G, acc = _field(mp, vol, np.zeros((0, 3), np.int32), **kw)
    assert acc == 0 and (G == P3.UNREACHED).all()                                               # none
    G, acc = _field(mp, vol, blocked + outside, **kw)
    assert acc == 0 and (G == P3.UNREACHED).all()                                               # all rejected
    one = _check_field(mp, vol, sources[:1], "one source", **kw)
    many = [tuple(sources[0])] * 5 + blocked + outside + [tuple(sources[0])]
    G, acc = _field(mp, vol, many, **kw)
    assert acc == 6 and np.array_equal(G, one)                                                  # duplicates and rejected entries change nothing
    _check_field(mp, vol, list(map(tuple, sources)) + outside + blocked, "all three", **kw)
    # a device tensor of sources and a preallocated field
    out = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
    assert mp.cost_volume(_dev(vol), _dev(sources[:1]), out=out, **kw) is out and np.array_equal(out.cpu().numpy(), one)


# ---- 7. a field that does not belong to the volume
def test_a_foreign_field_gives_minus_one_not_an_error(mp, cases):
    (_, _, vol_a, src_a), (_, _, vol_b, _) = cases[0], cases[1]
    assert vol_a.shape == vol_b.shape
    Ga = _check_field(mp, vol_a, src_a, **P3.CASE_OPTIONS)
    starts = np.argwhere(Ga != P3.UNREACHED)[::7]
    lengths = _check_paths(mp, vol_b, Ga, starts, 4, "foreign field", **P3.CASE_OPTIONS)
    assert (lengths == -1).any()
    _check_field(mp, vol_b, src_a, "after the foreign field", **P3.CASE_OPTIONS)              # the mapper is usable


# ---- 8. refusals
def test_refusals_launch_nothing_and_leave_the_mapper_usable(hip_lib):
    import torch
    M, _ = _mods()
    from isaac_ros_nvblox_amd import _lib
    m = M.Mapper(M.default_params(), device=0, block_capacity=64)
    m.synchronize(); m.set_profiling(True)
    lib, h = m.lib, m._h
    vol = torch.full((4, 4, 4), 0.9, dtype=torch.float32, device="cuda"); cost = torch.full((4, 4, 4), SENTINEL, dtype=torch.int32, device="cuda")
    xyz2 = torch.zeros((2, 3), dtype=torch.int32, device="cuda"); acc = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    paths = torch.full((2, 4, 3), SENTINEL, dtype=torch.int32, device="cuda"); lens = torch.full((2,), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan = float("nan")

    def opt(**kw):
        return C.byref(_lib.CostOptions(**P3.options(**kw)))

    def cv(mapper=h, v=p(vol), nx=4, ny=4, nz=4, o=None, s=p(xyz2), n=2, c=p(cost), a=p(acc), **kw):
        return lib.nvbx_cost_volume(mapper, v, nx, ny, nz, opt(**kw) if o is None else o, s, n, c, a)

    def tp(mapper=h, v=p(vol), nx=4, ny=4, nz=4, o=None, c=p(cost), s=p(xyz2), n=2, pa=p(paths), cap=4, ln=p(lens), **kw):
        return lib.nvbx_trace_paths_3d(mapper, v, nx, ny, nz, opt(**kw) if o is None else o, c, s, n, pa, cap, ln)
    null_options = C.POINTER(_lib.CostOptions)()
    refused = []
    for f in (cv, tp):
        refused += [
            lambda f=f: f(mapper=None), lambda f=f: f(v=None), lambda f=f: f(o=null_options), lambda f=f: f(c=None),
            lambda f=f: f(nx=0), lambda f=f: f(ny=0), lambda f=f: f(nz=0), lambda f=f: f(nx=-1), lambda f=f: f(ny=-4), lambda f=f: f(nz=-(2 ** 31)),
            lambda f=f: f(nx=(1 << 22) + 1, ny=1, nz=1), lambda f=f: f(nx=1, ny=(1 << 22) + 1, nz=1), lambda f=f: f(nx=1, ny=1, nz=(1 << 22) + 1),      # sizes only: refused before any read
            lambda f=f: f(nx=1 << 11, ny=1 << 11, nz=2), lambda f=f: f(nx=2 ** 31 - 1, ny=2 ** 31 - 1, nz=2 ** 31 - 1), lambda f=f: f(nx=1 << 16, ny=1 << 16, nz=1 << 16),
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
    for t in (cost, acc, paths, lens):
        assert (t == SENTINEL).all()                                                    # and nothing was written
    assert cv(a=None) == 0 and cv(s=None, n=0) == 0 and tp(s=None, pa=None, ln=None, n=0) == 0 and tp(cap=0) == 0      # not refusals
    with pytest.raises(M.NvbxError):
        m.cost_volume(vol, [(0, 0, 0)], max_penalty=500)
    with pytest.raises(TypeError):
        m.cost_volume(vol, [(0, 0, 0)], no_such_option=1)
    with pytest.raises(ValueError):
        m.cost_volume(vol[0], [(0, 0, 0)])
    G = _check_field(m, np.full((4, 4, 4), F32(0.9)), [(0, 0, 0)], "after the refusals")
    assert G[3, 3, 3] == 51
    m.close()


# ---- 9. end to end: from a mapped room to the price of a flight and the way
@pytest.fixture(scope="module")
def room(hip_lib):
    """two 80 x 60 frames that look at each other's standpoint, 3-D ESDF updated"""
    M, S = _mods()
    m = M.Mapper(M.default_params(esdf_mode=1), device=0, block_capacity=1 << 12)
    sc = S.Scene()
    poses = [S.look_pose((1.0, 0.0, 1.5), np.pi, np.deg2rad(-10.0)), S.look_pose((-1.0, 0.0, 1.5), 0.0, np.deg2rad(-10.0))]
    for T in poses:
        d, _ = S.render(sc, T, CAM)
        m.integrate_depth(d, T, CAM)
    m.update_esdf()
    m.synchronize()
    yield m, poses
    m.close()


def test_end_to_end_from_the_map_to_a_priced_flight(room):
    import torch
    M, _ = _mods()
    m, poses = room
    kw = dict(robot_radius_m=0.10, inflation_radius_m=0.5, allow_unknown=1)
    before = H.map_state(m)
    idx = np.asarray(m.block_indices(M.LAYER_ESDF), np.int32).reshape(-1, 3)
    assert len(idx) > 8
    mn = idx.min(0) * 8
    size = (idx.max(0) + 1) * 8 - mn
    assert int(np.prod(size.astype(np.int64))) <= 1 << 22, size
    vol_dev = m.esdf_dense_grid_device(mn, size, 1000.0)
    assert vol_dev.is_cuda and vol_dev.dtype == torch.float32 and tuple(vol_dev.shape) == tuple(int(v) for v in size)
    vol = vol_dev.cpu().numpy()
    assert np.array_equal(vol, m.esdf_dense_grid(mn, size, 1000.0))
    out = torch.full_like(vol_dev, float(SENTINEL))
    assert m.esdf_dense_grid_device(mn, size, 1000.0, out=out) is out and np.array_equal(out.cpu().numpy(), vol)
    src = m.volume_voxels(poses[0][:3, 3].reshape(1, 3), mn)
    assert np.all(src >= 0) and np.all(src < size), (src, size)
    acc = torch.zeros(1, dtype=torch.int32, device="cuda")
    G_dev = m.cost_volume(vol_dev, src, accepted=acc, **kw)
    G = G_dev.cpu().numpy()
    want, n_acc = P3.field(vol, src, P3.options(**kw))
    assert n_acc == 1 and int(acc.item()) == 1, "the camera does not stand in traversable space: v = %r" % (vol[tuple(src[0])],)
    assert np.array_equal(G, want) and (G != P3.UNREACHED).sum() > 5000
    known = np.argwhere((G != P3.UNREACHED) & (np.abs(vol - 1000.0) > 1.0))
    assert len(known) > 500                                                                    # the field reaches observed free space, not only the unknown
    rng = np.random.default_rng(3)
    starts = known[rng.choice(len(known), 16, replace=False)].astype(np.int32)
    paths, lengths = m.trace_paths_3d(vol_dev, G_dev, starts, 512, **kw)
    paths = paths.cpu().numpy(); lengths = lengths.cpu().numpy()
    o = P3.options(**kw)
    for i, s in enumerate(starts):
        w = P3.path(vol, want, s, o)
        assert w and int(lengths[i]) == len(w) <= 512, (i, s.tolist(), int(lengths[i]))
        assert np.array_equal(paths[i, :len(w)], np.array(w, np.int32)) and tuple(paths[i, len(w) - 1]) == tuple(src[0])      # it reaches the source
    m.synchronize()
    H.assert_same_map(before, m, "before and after the cost volume and the paths")             # the calls write nothing to the map
