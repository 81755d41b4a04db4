"""The feature layer on the GPU (features.hip; SEMANTICS.md "Feature layer") against the independent model of tests/feature_independent.py -- exactly:
the set of voxels with weight > 0, the weights and the fp16 bit patterns of every channel -- and against the colour layer, slot reuse, pool growth,
the rest of the mapper, the refusals and the two readers."""
import numpy as np
import pytest

import feature_independent as FI
import helpers as H

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _rules(p):
    occ = None if p.color_occlusion_threshold_vox < 0 else p.color_occlusion_threshold_vox * p.voxel_size
    return FI.Rules(p.voxel_size, p.max_integration_distance_m, p.max_weight, p.truncation_distance_vox, occ, max(1, p.sphere_tracing_subsampling))


def _tsdf_blocks(M, m, rules):
    idx = m.block_indices(M.LAYER_TSDF)
    if len(idx) == 0:
        return idx, np.zeros(0, bool)
    v, found = m.get_blocks(M.LAYER_TSDF, idx)
    assert found.all()
    return idx, FI.in_band(v["distance"], v["weight"], rules.trunc).any(axis=1)


def _model_frame(M, m, state, feat, T, stride, cam=CAM):
    """The model's step for the frame the mapper is about to integrate: its inputs are read from the mapper through other entry points."""
    rules = _rules(m.params)
    idx, band = _tsdf_blocks(M, m, rules)
    synth = m.render(T, cam, subsampling=rules.sub, color=False)[0].cpu().numpy()
    return FI.integrate(state, rules, idx, band, synth, T, cam, stride, feat)


def _expected(state, idx, C):
    f = np.zeros((len(idx), 512, C), np.float16); w = np.zeros((len(idx), 512), np.float32); has = np.zeros(len(idx), bool)
    for i, b in enumerate(idx):
        s = state.get(tuple(int(q) for q in b))
        if s is not None:
            f[i], w[i], has[i] = s[0], s[1], True
    return f, w, has


def _assert_layer_is(M, m, state, C, what=""):
    idx = m.block_indices(M.LAYER_TSDF)
    f, w, found = m.feature_blocks(idx)
    ef, ew, eh = _expected(state, idx, C)
    assert set(state) <= {tuple(int(q) for q in b) for b in idx}, what
    assert np.array_equal(found, eh), what
    assert np.array_equal(w > 0, ew > 0), what
    assert np.array_equal(w.view(np.uint32), ew.view(np.uint32)), what
    bad = f.view(np.uint16) != ef.view(np.uint16)
    assert not bad.any(), "%s: %d of %d values differ from the model" % (what, int(bad.sum()), bad.size)
    fl = m.block_indices(M.LAYER_FEATURE)
    assert {tuple(int(q) for q in b) for b in fl} == set(state), what
    return idx, f, w


def _frames(S, n=3, step=9):
    sc = S.Scene()
    out = []
    for i in range(n):
        T = S.trajectory_pose(i * step)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


@pytest.fixture(scope="module")
def room_frames():
    _, S = _mods()
    return _frames(S)


# ---- 1. against the model, exactly
@pytest.mark.parametrize("C,stride", [(8, 1), (8, 4), (40, 1), (40, 4)])
def test_three_frames_equal_the_model_bit_for_bit(room_frames, C, stride):
    M, _ = _mods()
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    for d, _, T in room_frames:
        m.integrate_depth(d, T, CAM)
    m.enable_features(C)
    rng = np.random.default_rng(100 * C + stride)
    state = {}
    for k, (_, _, T) in enumerate(room_frames):
        feat = rng.standard_normal((CAM[5] // stride, CAM[4] // stride, C)).astype(np.float16)
        _model_frame(M, m, state, feat, T, stride)
        m.integrate_features(feat, T, CAM, stride)
        _, f, w = _assert_layer_is(M, m, state, C, "frame %d" % k)
    assert (w == 3).any() and (w == 1).any() and len(state) > 50       # the frames overlap, and the layer is not trivially empty
    m.close()


# ---- 2. against colour, sharing no model
def test_weights_equal_the_colour_layers(room_frames):
    M, _ = _mods()
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.set_color_deferral(False)
    m.enable_features(8)
    for d, _, T in room_frames:
        m.integrate_depth(d, T, CAM)
    for _, rgb, T in room_frames:
        feat = np.zeros((CAM[5], CAM[4], 8), np.float16); feat[:, :, :3] = rgb
        m.integrate_color(rgb, T, CAM)
        m.integrate_features(feat, T, CAM, 1)
    idx = m.block_indices(M.LAYER_TSDF)
    col, _ = m.get_blocks(M.LAYER_COLOR, idx)
    _, w, _ = m.feature_blocks(idx)
    assert np.array_equal(col["weight"].view(np.uint32), w.view(np.uint32))
    assert (w > 0).sum() > 10000 and (w == 3).any()
    m.close()


def test_weights_equal_the_colour_layers_on_an_odd_image():
    """The same identity where the tracing launches' ray numbering has its edge cases: a 37 x 29 camera at sphere_tracing_subsampling 4 gives a
    9 x 7 synthetic image -- no multiple of the 8 x 4 ray patch on either side, and its four patches are fewer than the eight bands of the
    numbering, so partial patches and workgroups without a patch run on the colour path and on the feature path."""
    M, S = _mods()
    cam = (18.5, 18.5, 18.0, 14.0, 37, 29)      # CAM's field of view
    p = M.default_params()
    assert p.sphere_tracing_subsampling == 4
    m = M.Mapper(p, block_capacity=1 << 12)
    m.set_color_deferral(False)
    m.enable_features(8)
    sc = S.Scene()
    frames = []
    for i in range(3):
        T = S.trajectory_pose(i * 9)
        d, rgb = S.render(sc, T, cam)
        frames.append((rgb, T))
        m.integrate_depth(d, T, cam)
    for rgb, T in frames:
        feat = np.zeros((cam[5], cam[4], 8), np.float16); feat[:, :, :3] = rgb
        m.integrate_color(rgb, T, cam)
        m.integrate_features(feat, T, cam, 1)
    assert m.synthetic_depth().shape == (7, 9)
    idx = m.block_indices(M.LAYER_TSDF)
    col, _ = m.get_blocks(M.LAYER_COLOR, idx)
    _, w, _ = m.feature_blocks(idx)
    assert np.array_equal(col["weight"].view(np.uint32), w.view(np.uint32))
    # not trivially empty: the occlusion test passes only inside the synthetic image's interior (8 x 6 of its 9 x 7 pixels, about 3/4 of the
    # view), where each of the ~1 000 depth pixels of a frame has at least one voxel of the truncation band behind it
    assert (w > 0).sum() > 500 and (w == 3).any()
    m.close()


# ---- hand-made walls (set_blocks): a one-sided wall at x = 1 and, behind it, a two-sided slab at x = 2.2
def _wall_blocks(M, plane_x, two_sided, y_rng, z_rng, extra_bx=()):
    """TSDF blocks (weight 1) around the plane x = plane_x; extra_bx: further block columns of observed space beside it (the sphere tracer steps
    a whole truncation distance through unobserved space, and would step into a thin slab)."""
    idx, data = [], []
    t = np.arange(512)
    for bx in (int(np.floor(plane_x / 0.4)),) + tuple(extra_bx):
      for by in range(*y_rng):
        for bz in range(*z_rng):
            x = (bx * 8 + (t >> 6) + 0.5) * VS
            d = (np.abs(x - plane_x) - 0.05) if two_sided else (plane_x - x)
            v = np.zeros(512, M.TSDF_DT)
            v["distance"] = np.clip(d, -0.2, 0.2); v["weight"] = 1.0
            idx.append((bx, by, bz)); data.append(v)
    return np.array(idx, np.int32), np.stack(data)


def _look(S, pos, yaw):
    return S.look_pose(np.array(pos, float), yaw, 0.0)


# ---- 3. occlusion
def test_a_wall_hidden_behind_another_gets_features_only_from_its_own_side():
    M, S = _mods()
    m = M.Mapper(M.default_params(), block_capacity=256)
    i1, d1 = _wall_blocks(M, 1.0, False, (-3, 3), (0, 4))
    i2, d2 = _wall_blocks(M, 2.2, True, (-1, 1), (1, 2), extra_bx=(6,))
    m.set_blocks(M.LAYER_TSDF, i1, d1); m.set_blocks(M.LAYER_TSDF, i2, d2)
    m.enable_features(8)
    feat = np.ones((15, 20, 8), np.float16)
    front, back = _look(S, (0.0, 0.0, 0.6), 0.0), _look(S, (3.2, 0.0, 0.6), np.pi)
    state = _model_frame(M, m, {}, feat, front, 4)
    m.integrate_features(feat, front, CAM, 4)
    _assert_layer_is(M, m, state, 8, "front")
    _, w1, _ = m.feature_blocks(i1); _, w2, found2 = m.feature_blocks(i2)
    assert (w1 == 1).sum() > 500 and not found2.any() and (w2 == 0).all()          # the hidden wall's band keeps weight 0
    _model_frame(M, m, state, feat, back, 4)
    m.integrate_features(feat, back, CAM, 4)
    _assert_layer_is(M, m, state, 8, "back")
    _, w1b, _ = m.feature_blocks(i1); _, w2b, found2 = m.feature_blocks(i2)
    assert found2.all() and (w2b == 1).sum() > 300 and w2b.max() == 1
    assert np.array_equal(w1b, w1)                                                  # and the front wall, hidden from behind, is left alone
    m.close()


# ---- 4. layout and C
@pytest.mark.parametrize("C", [8, 16, 40, 256])
def test_layout_at_every_chunk_count(C):
    M, S = _mods()
    m = M.Mapper(M.default_params(), block_capacity=256)
    idx, data = _wall_blocks(M, 1.0, False, (-2, 2), (0, 3))
    m.set_blocks(M.LAYER_TSDF, idx, data)
    m.enable_features(C)
    rows_f, cols_f, stride = 7, 10, 8
    code = np.arange(rows_f * cols_f * C, dtype=np.uint16).reshape(rows_f, cols_f, C)
    feat = (code + np.uint16(0x0400)).view(np.float16)        # (i, j, c) -> its own positive normal fp16 value, every one different
    assert np.isfinite(feat).all() and len(np.unique(feat)) == feat.size
    T = _look(S, (0.0, 0.0, 0.6), 0.0)
    state = _model_frame(M, m, {}, feat, T, stride)
    m.integrate_features(feat, T, CAM, stride)
    idx_all, f, w = _assert_layer_is(M, m, state, C)
    assert (w > 0).sum() > 500
    # the point reader at every voxel centre
    t = np.arange(512)
    off = np.stack([t >> 6, (t >> 3) & 7, t & 7], 1)
    pts = ((idx_all[:, None, :].astype(np.float64) * 8 + off[None] + 0.5) * VS).reshape(-1, 3).astype(np.float32)
    qf, qw = m.query_features(pts)
    assert np.array_equal(qf.cpu().numpy().view(np.uint16).reshape(f.shape), f.view(np.uint16))
    assert np.array_equal(qw.cpu().numpy().reshape(w.shape), w)
    m.close()


# ---- 5. slot reuse (lazy invalidation)
@pytest.mark.parametrize("how", ["radius", "decay", "clear"])
def test_a_reused_slot_starts_empty(how):
    M, S = _mods()
    sc = S.Scene()
    Ta, Tb = S.trajectory_pose(0), S.trajectory_pose(100)       # opposite sides of the circle, looking away from each other
    da, _ = S.render(sc, Ta, CAM); db, _ = S.render(sc, Tb, CAM)
    p = M.default_params(tsdf_decay_factor=0.1)
    scout = M.Mapper(p, block_capacity=1 << 12)
    scout.integrate_depth(da, Ta, CAM); ia = scout.block_indices(M.LAYER_TSDF)
    scout.clear(); scout.integrate_depth(db, Tb, CAM); ib = scout.block_indices(M.LAYER_TSDF)
    scout.close()
    na, nb = len(ia), len(ib)
    cap = max(na, nb) + 64
    assert min(na, nb) > 64        # so that na + nb > cap: the second region cannot fit beside the first without reusing slots
    m = M.Mapper(p, block_capacity=cap, max_block_capacity=cap)
    C = 16
    m.enable_features(C)
    rng = np.random.default_rng(5)
    feat = rng.standard_normal((15, 20, C)).astype(np.float16)
    m.integrate_depth(da, Ta, CAM)
    state = _model_frame(M, m, {}, feat, Ta, 4)
    m.integrate_features(feat, Ta, CAM, 4)
    _assert_layer_is(M, m, state, C, "before")
    assert len(state) > 20
    if how == "radius":
        m.clear_outside_radius((100.0, 100.0, 100.0), 0.2)
    elif how == "decay":
        for _ in range(8):
            m.decay_tsdf(exclude_last_view=False)
    else:
        m.clear()
    assert m.num_blocks(M.LAYER_TSDF) == 0 and m.num_blocks(M.LAYER_FEATURE) == 0 and m.counters()["blocks_allocated"] == 0
    m.integrate_depth(db, Tb, CAM)
    c = m.counters()
    idx = m.block_indices(M.LAYER_TSDF)
    assert c["capacity_overflow"] == 0 and len(idx) == nb and m.capacity == cap and na + len(idx) > cap       # at least na + nb - cap slots are reused
    f, w, found = m.feature_blocks(idx)
    assert not found.any() and not w.any() and not f.view(np.uint16).any()
    pts = ((idx.astype(np.float64) * 8 + 3.5) * VS).astype(np.float32)
    qf, qw = m.query_features(pts)
    assert not qw.cpu().numpy().any() and not qf.cpu().numpy().view(np.uint16).any()
    feat2 = rng.standard_normal((15, 20, C)).astype(np.float16)
    state = _model_frame(M, m, {}, feat2, Tb, 4)            # the model started from empty
    m.integrate_features(feat2, Tb, CAM, 4)
    _assert_layer_is(M, m, state, C, "after")
    assert len(state) > 20
    m.close()


# ---- 6. growth
def test_pool_growth_carries_the_layer():
    M, S = _mods()
    sc = S.Scene()
    m = M.Mapper(M.default_params(), block_capacity=1 << 9, max_block_capacity=1 << 13)
    C = 16
    m.enable_features(C)
    rng = np.random.default_rng(6)
    state, caps = {}, [m.capacity]
    for k in range(6):
        T = S.trajectory_pose(k * 25)
        d, _ = S.render(sc, T, CAM)
        m.integrate_depth(d, T, CAM)
        caps.append(m.capacity)
        feat = rng.standard_normal((15, 20, C)).astype(np.float16)
        _model_frame(M, m, state, feat, T, 4)
        m.integrate_features(feat, T, CAM, 4)
        _assert_layer_is(M, m, state, C, "frame %d at %d blocks" % (k, m.capacity))
    grew = [k for k in range(1, len(caps)) if caps[k] > caps[k - 1]]
    assert grew and grew[0] > 1 and grew[-1] < len(caps) - 1, caps       # feature frames before the first growth and after the last
    assert m.profile()["_feature_pool_bytes"]["count"] == m.capacity * (1024 * C + 2048)
    m.close()


# ---- 7. nothing else moves
def _other_outputs(M, m):
    """what the map comparison does not hold: the synthetic depth image, the last colour view, the mesh's sizes and the counters"""
    out = {}
    out["synth"] = m.synthetic_depth().view(np.uint32)
    out["color_view"] = m.last_color_view()
    mesh = m.mesh()
    out["mesh"] = np.array([len(mesh), sum(len(v["vertices"]) for v in mesh.values()), sum(len(v["triangles"]) for v in mesh.values())])
    c = m.counters()
    out["counters"] = np.array([c[k] for k in sorted(c)])
    return out


@pytest.mark.parametrize("deferral", [False, True])
def test_a_mapper_with_features_computes_everything_else_as_one_without(deferral):
    M, S = _mods()
    sc = S.Scene()
    rng = np.random.default_rng(7)
    ops = []
    for k in range(24):
        ops.append((rng.choice(["depth", "depth", "color", "color", "esdf", "mesh", "decay"]), int(rng.integers(0, 60)), rng.random() < 0.5, int(rng.integers(0, 1 << 30))))
    ops += [("depth", 3, True, 1), ("color", 3, True, 2), ("esdf", 0, False, 3), ("mesh", 0, False, 4)]
    snaps = []
    for with_features in (False, True):
        m = M.Mapper(M.default_params(), block_capacity=1 << 12)
        m.set_color_deferral(deferral)
        if with_features:
            m.enable_features(8)
        else:
            assert "_feature_pool_bytes" not in m.profile()
        for op, i, sprinkle, seed in ops:
            T = S.trajectory_pose(i)
            if op in ("depth", "color"):
                d, rgb = S.render(sc, T, CAM)
                m.integrate_depth(d, T, CAM) if op == "depth" else m.integrate_color(rgb, T, CAM)
            elif op == "esdf":
                m.update_esdf()
            elif op == "mesh":
                m.update_color_mesh()
            else:
                m.decay_tsdf()
            if with_features and sprinkle:
                r2 = np.random.default_rng(seed)
                if seed & 1:
                    m.integrate_features(r2.standard_normal((15, 20, 8)).astype(np.float16), T, CAM, 4)
                else:
                    m.query_features(r2.uniform(-3, 3, (256, 3)).astype(np.float32))
        if with_features:
            assert m.num_blocks(M.LAYER_FEATURE) > 0 and "_feature_pool_bytes" in m.profile()
        else:
            assert "_feature_pool_bytes" not in m.profile() and m.num_blocks(M.LAYER_FEATURE) == 0      # nothing was ever allocated for features
        snaps.append((H.map_state(m, slice=True), _other_outputs(M, m)))
        m.close()
    (sa, a), (sb, b) = snaps
    H.assert_same_map(sa, sb, "without and with features", min_blocks={M.LAYER_TSDF: 101, M.LAYER_COLOR: 51, M.LAYER_ESDF: 11})
    assert a["mesh"][2] > 1000
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 8. refusals
def test_refusals_leave_the_mapper_usable(room_frames):
    M, _ = _mods()
    d, _, T = room_frames[0]
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.integrate_depth(d, T, CAM)
    feat = np.ones((15, 20, 8), np.float16)

    def refused(fn, code=-1):
        with pytest.raises(M.NvbxError) as e:
            fn()
        assert ("nvbx error %d" % code) in str(e.value) or "channels" in str(e.value), str(e.value)

    refused(lambda: m.integrate_features(feat, T, CAM, 4))                     # before enable
    refused(lambda: m.query_features(np.zeros((4, 3), np.float32)))
    refused(lambda: m.enable_features(12))
    refused(lambda: m.enable_features(264))
    refused(lambda: m.enable_features(0))
    m.enable_features(8)
    m.enable_features(8)                                                       # the same C again: a no-op
    refused(lambda: m.enable_features(16))
    refused(lambda: m.integrate_features(np.ones((16, 20, 8), np.float16), T, CAM, 4))       # 16 * 4 > 60 rows
    refused(lambda: m.integrate_features(np.ones((15, 21, 8), np.float16), T, CAM, 4))       # 21 * 4 > 80 columns
    refused(lambda: m.integrate_features(np.ones((15, 20, 16), np.float16), T, CAM, 4))      # channel count
    refused(lambda: m.integrate_features(feat, T, CAM, 0))
    Tn = T.copy(); Tn[0, 3] = np.nan
    refused(lambda: m.integrate_features(feat, Tn, CAM, 4))
    occ = M.Mapper(M.default_params(projective_layer_type=1), block_capacity=256)
    refused(lambda: occ.enable_features(8))
    occ.integrate_depth(d, T, CAM); assert occ.num_blocks(M.LAYER_OCCUPANCY) > 0
    occ.close()
    # the mapper still works, and no refused call left anything behind
    assert m.num_blocks(M.LAYER_FEATURE) == 0
    state = _model_frame(M, m, {}, feat, T, 4)
    m.integrate_features(feat, T, CAM, 4)
    _assert_layer_is(M, m, state, 8)
    # points that are not finite or outside the addressable range: weight 0, not an error
    lim = float(1 << 20) * 8 * VS
    pts = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [lim, 0, 0], [0, -lim - 1.0, 0], [3e38, 3e38, 3e38], [50.0, 50.0, 50.0]], np.float32)
    qf, qw = m.query_features(pts)
    assert not qw.cpu().numpy().any() and not qf.cpu().numpy().view(np.uint16).any()
    m.close()


# ---- 9. readers agree
def test_point_reader_equals_a_gather_from_the_block_reader(room_frames):
    M, _ = _mods()
    C = 24
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.enable_features(C)
    rng = np.random.default_rng(9)
    for d, _, T in room_frames:
        m.integrate_depth(d, T, CAM)
        m.integrate_features(rng.standard_normal((15, 20, C)).astype(np.float16), T, CAM, 4)
    idx = m.block_indices(M.LAYER_TSDF)
    f, w, _ = m.feature_blocks(idx)
    # 4 096 points: half anywhere in a box around the room (most of them outside the map), half inside voxels that hold features (the band is thin);
    # none within 1e-4 voxel of a voxel face (float32 p / vs and float64 p / vs then floor alike)
    bi, ti = np.nonzero(w > 0)
    pick = rng.integers(0, len(bi), 8192)
    cells = idx[bi[pick]].astype(np.float64) * 8 + np.stack([ti[pick] >> 6, (ti[pick] >> 3) & 7, ti[pick] & 7], 1)
    pts = np.zeros((0, 3), np.float32)
    for q in (rng.uniform([-4.0, -3.5, -0.5], [4.0, 3.5, 3.5], (8192, 3)), (cells + rng.uniform(0.0, 1.0, cells.shape)) * VS):
        q = q.astype(np.float32)
        fr = q.astype(np.float64) / VS
        keep = (np.abs(fr - np.round(fr)) > 1e-4).all(axis=1)
        assert keep.sum() >= 2048
        pts = np.concatenate([pts, q[keep][:2048]])
    where = {tuple(int(q) for q in b): i for i, b in enumerate(idx)}
    bl, t = FI.voxel_of(pts, VS)
    ef = np.zeros((len(pts), C), np.float16); ew = np.zeros(len(pts), np.float32)
    for k in range(len(pts)):
        i = where.get(tuple(int(q) for q in bl[k]))
        if i is not None:
            ef[k], ew[k] = f[i, t[k]], w[i, t[k]]
    qf, qw = m.query_features(pts)
    assert np.array_equal(qw.cpu().numpy(), ew) and np.array_equal(qf.cpu().numpy().view(np.uint16), ef.view(np.uint16))
    assert len(pts) == 4096 and (ew > 0).sum() > 1500 and (ew == 0).sum() > 1500
    m.close()
