"""Edge cases of the hot path on the GPU (empty / ragged inputs, capacity limits, idle updates), each against the oracle
or against an invariant -- the inputs the reference's callers can legally hand over (nvblox_node.cpp drops frames but
never validates image content)."""
import numpy as np
import pytest

import helpers as H
from isaac_ros_nvblox_amd import synthetic as S

pytestmark = pytest.mark.gpu


def pair(oracle_mod, cap=1 << 13, **kw):
    from isaac_ros_nvblox_amd import mapper as M
    pg = M.default_params(**kw); po = H.copy_params(pg, oracle_mod.OrcParams)
    return M, M.Mapper(pg, block_capacity=cap), oracle_mod.OracleMap(po)


def test_all_invalid_depth_allocates_nothing(oracle_mod, hip_lib):
    M, g, o = pair(oracle_mod)
    d = np.zeros((120, 160), np.float32); T = S.trajectory_pose(0)
    g.integrate_depth(d, T, H.SMALL_CAM); o.integrate_depth(d, T, H.SMALL_CAM)
    assert g.num_blocks(M.LAYER_TSDF) == 0 == o.num_blocks(oracle_mod.L_TSDF)
    assert len(g.last_view()) == 0
    g.update_esdf(); g.update_color_mesh()                       # idle updates on an empty map
    img, aabb = g.esdf_slice_image()
    assert img.size == 0
    assert g.mesh() == {}
    c = g.counters()
    assert c["blocks_allocated"] == 0 and c["capacity_overflow"] == 0
    rgb = np.zeros((120, 160, 3), np.uint8)
    g.integrate_color(rgb, T, H.SMALL_CAM)                        # colour on an empty map
    assert g.num_blocks(M.LAYER_COLOR) == 0


@pytest.mark.parametrize("shape", [(113, 157), (9, 11), (64, 64)])
def test_ragged_image_sizes(oracle_mod, hip_lib, shape):
    """Image sizes that are not multiples of the 8x8 tile / the sub-sampling factor."""
    rows, cols = shape
    cam = (cols / 2.0, cols / 2.0, cols / 2.0 - 0.5, rows / 2.0 - 0.5, cols, rows)
    M, g, o = pair(oracle_mod)
    sc = S.Scene()
    for i in range(2):
        T = S.trajectory_pose(i * 11)
        d, rgb = S.render(sc, T, cam)
        g.integrate_depth(d, T, cam); o.integrate_depth(d, T, cam)
        assert H.idx_set(g.last_view()) == H.idx_set(o.last_view())
        if rows >= 8:
            g.integrate_color(rgb, T, cam); o.integrate_color(rgb, T, cam)
            assert np.abs(g.synthetic_depth() - o.synthetic_depth()).max() <= 1e-4
    ig = g.block_indices(M.LAYER_TSDF); io = o.block_indices(oracle_mod.L_TSDF)
    assert np.array_equal(ig, io) and len(io) > 0
    bg, _ = g.get_blocks(M.LAYER_TSDF, ig)
    for k, idx in enumerate(io):
        bo = o.get_block(oracle_mod.L_TSDF, idx)
        assert np.abs(bg[k]["distance"] - bo["distance"]).max() <= 1e-4 and np.abs(bg[k]["weight"] - bo["weight"]).max() <= 1e-4


def test_block_pool_exhaustion_is_reported_not_fatal(oracle_mod, hip_lib):
    """FIXED pools (max capacity = capacity) and more blocks in view than they hold: the sticky overflow flag is raised, allocated
    blocks stay consistent, and the mapper keeps working after clear()."""
    M, g, o = pair(oracle_mod, cap=128)
    g.set_max_capacity(128)
    d, rgb, T = H.frames(1, H.SMALL_CAM, color=False)[0]
    g.integrate_depth(d, T, H.SMALL_CAM)
    c = g.counters()
    assert c["capacity_overflow"] != 0
    assert g.num_blocks(M.LAYER_TSDF) <= 128 and g.capacity == 128
    g.update_esdf(); g.update_color_mesh(); g.synchronize()      # must not hang or fault
    g.clear()
    assert g.num_blocks(M.LAYER_TSDF) == 0


def test_pools_grow_on_demand_without_data_loss(oracle_mod, hip_lib):
    """The reference allocates blocks on demand; here the pools double before they run out (nvbx_mapper_set_max_capacity).  A map that
    ends up 3x larger than the initial pools == the oracle's, with ESDF / mesh / colour state carried across every doubling."""
    M, g, o = pair(oracle_mod, cap=1024)
    caps = [g.capacity]
    for k, (d, rgb, T) in enumerate(H.frames(10, H.SMALL_CAM, color=True, stride=17)):
        g.integrate_depth(d, T, H.SMALL_CAM); o.integrate_depth(d, T, H.SMALL_CAM)
        assert H.idx_set(g.last_view()) == H.idx_set(o.last_view())
        g.integrate_color(rgb, T, H.SMALL_CAM); o.integrate_color(rgb, T, H.SMALL_CAM)
        g.update_esdf(); o.update_esdf()                  # (the distance transform stays held back across a growth)
        if k % 3 == 2:
            g.update_color_mesh(); o.update_mesh()        # (and so does the last mesh update's arena content)
        caps.append(g.capacity)
    assert caps[-1] >= 4096 and caps[0] == 1024 and sorted(caps) == caps
    assert g.counters()["capacity_overflow"] == 0
    from helpers import compare_layer
    n, _ = compare_layer(M, g, o, M.LAYER_TSDF, oracle_mod.L_TSDF, fields_tol=("distance", "weight"))
    assert n > 1200
    compare_layer(M, g, o, M.LAYER_COLOR, oracle_mod.L_COLOR, fields_tol=("weight",), lsb_fields=("r", "g", "b"))
    compare_layer(M, g, o, M.LAYER_ESDF, oracle_mod.L_ESDF, fields_exact=H.ESDF_FIELDS)
    g.update_color_mesh(full=True); o.update_mesh(full=True)
    mg = g.mesh()
    for idx in o.block_indices(oracle_mod.L_TSDF):
        assert np.array_equal(mg[tuple(idx)]["triangles"], o.mesh_block(idx)["triangles"])


def test_mesh_of_the_last_update_survives_a_growth(oracle_mod, hip_lib):
    M, g, o = pair(oracle_mod, cap=1024)
    fr = H.frames(4, H.SMALL_CAM, color=False, stride=23)
    g.integrate_depth(fr[0][0], fr[0][2], H.SMALL_CAM)
    g.update_color_mesh()
    before = g.mesh()
    cap0 = g.capacity
    for d, rgb, T in fr[1:]:
        g.integrate_depth(d, T, H.SMALL_CAM); g.synchronize()
    assert g.capacity > cap0
    after = g.mesh()                                           # still the FIRST update's mesh (no update since), re-based into the wider arenas
    assert set(before) == set(after) and len(before) > 50
    for k in before:
        assert np.array_equal(before[k]["vertices"], after[k]["vertices"]) and np.array_equal(before[k]["triangles"], after[k]["triangles"])


def test_explicit_allocation_grows_the_pools(hip_lib):
    """allocateBlockAtIndex / loadMap through nvbx_set_blocks: room is made for the whole batch."""
    from isaac_ros_nvblox_amd import mapper as M
    g = M.Mapper(M.default_params(), block_capacity=256)
    idx = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij"), -1).reshape(-1, 3).astype(np.int32)    # 1728 blocks
    data = np.zeros((len(idx), 512), M.TSDF_DT); data["distance"] = 0.1; data["weight"] = 1.0
    g.set_blocks(M.LAYER_TSDF, idx, data)
    assert g.num_blocks(M.LAYER_TSDF) == 1728 and g.capacity >= 2048 and g.counters()["capacity_overflow"] == 0
    b, found = g.get_blocks(M.LAYER_TSDF, idx[::97])
    assert found.all() and (b["weight"] == 1.0).all()


def test_clear_then_reuse_matches_fresh_mapper(oracle_mod, hip_lib):
    M, g, o = pair(oracle_mod)
    fr = H.frames(2, H.SMALL_CAM, color=False, stride=9)
    for d, rgb, T in fr:
        g.integrate_depth(d, T, H.SMALL_CAM)
    g.update_esdf()
    g.clear()
    for d, rgb, T in fr:
        g.integrate_depth(d, T, H.SMALL_CAM); o.integrate_depth(d, T, H.SMALL_CAM)
    g.update_esdf(); o.update_esdf()
    assert np.array_equal(g.block_indices(M.LAYER_TSDF), o.block_indices(oracle_mod.L_TSDF))
    sg, _ = g.esdf_slice_image(); so, _ = o.esdf_slice_image()
    assert sg.shape == so.shape and np.abs(sg - so).max() <= 1e-4


def test_esdf_update_without_new_data_is_idempotent(oracle_mod, hip_lib):
    M, g, o = pair(oracle_mod)
    for d, rgb, T in H.frames(2, H.SMALL_CAM, color=False, stride=9):
        g.integrate_depth(d, T, H.SMALL_CAM)
    g.update_esdf()
    a, _ = g.esdf_slice_image()
    g.update_esdf()                                              # nothing dirty: empty window
    b, _ = g.esdf_slice_image()
    assert np.array_equal(a, b)
    assert g.counters()["esdf_columns_marked"] == 0


def test_camera_facing_unmapped_space_then_back(oracle_mod, hip_lib):
    """Depth beyond max_integration_distance almost everywhere: rays are clipped at 1 m, mostly free space is carved."""
    M, g, o = pair(oracle_mod, max_integration_distance_m=1.0)
    d, rgb, T = H.frames(1, H.SMALL_CAM, color=False)[0]
    g.integrate_depth(d, T, H.SMALL_CAM); o.integrate_depth(d, T, H.SMALL_CAM)
    ig = g.block_indices(M.LAYER_TSDF); io = o.block_indices(oracle_mod.L_TSDF)
    assert np.array_equal(ig, io) and len(io) > 0
    bg, _ = g.get_blocks(M.LAYER_TSDF, ig)
    for k, idx in enumerate(io):
        bo = o.get_block(oracle_mod.L_TSDF, idx)
        assert np.abs(bg[k]["distance"] - bo["distance"]).max() <= 1e-4 and np.abs(bg[k]["weight"] - bo["weight"]).max() <= 1e-4
    assert (bg["distance"][bg["weight"] > 0] > 0).mean() > 0.9     # nearly everything within 1 m is free space
    g.update_color_mesh(); o.update_mesh()
    assert sum(len(v["triangles"]) for v in g.mesh().values()) == sum(len(o.mesh_block(i)["triangles"]) for i in io)


def test_esdf_layer_changes_only_in_update_esdf(oracle_mod, hip_lib):
    """The ESDF site marking rides in the colour-integration launch and the distance transform may be held back until the
    next call -- but what the API shows must behave like the reference: the ESDF layer changes in
    updateEsdf and nowhere else, and every query sees completed updates."""
    M, g, o = pair(oracle_mod, cap=1 << 14)
    fr = H.frames(4, H.SMALL_CAM, color=True, stride=9)
    for d, rgb, T in fr[:2]:
        g.integrate_depth(d, T, H.SMALL_CAM); g.integrate_color(rgb, T, H.SMALL_CAM)
        o.integrate_depth(d, T, H.SMALL_CAM); o.integrate_color(rgb, T, H.SMALL_CAM)
    g.update_esdf(); o.update_esdf()
    before = H.map_state(g, layers=(M.LAYER_ESDF,), slice=True)
    idx0 = before["layers"][M.LAYER_ESDF][0]
    assert np.array_equal(idx0, o.block_indices(oracle_mod.L_ESDF))
    # new depth + colour: marking happens inside the colour launch, but nothing observable may change
    for d, rgb, T in fr[2:]:
        g.integrate_depth(d, T, H.SMALL_CAM); g.integrate_color(rgb, T, H.SMALL_CAM)
        o.integrate_depth(d, T, H.SMALL_CAM); o.integrate_color(rgb, T, H.SMALL_CAM)
        H.assert_same_map(before, g, "the ESDF between two updates")
    # ... until updateEsdf, after which every query path sees the completed update (held-back EDT included)
    g.update_esdf(); o.update_esdf()
    img2, _ = g.esdf_slice_image(); ref, _ = o.esdf_slice_image()
    assert img2.shape == ref.shape and np.abs(img2 - ref).max() <= 1e-4 and not np.array_equal(img2.shape, ()) 
    g.update_esdf(); o.update_esdf()                              # nothing dirty: held back again, then read through another path
    idx2 = g.block_indices(M.LAYER_ESDF)
    assert np.array_equal(idx2, o.block_indices(oracle_mod.L_ESDF)) and len(idx2) >= len(idx0)
    blk2, _ = g.get_blocks(M.LAYER_ESDF, idx2)
    for k, i in enumerate(idx2):
        bo = o.get_block(oracle_mod.L_ESDF, i)
        for f_ in H.ESDF_FIELDS:
            assert np.array_equal(blk2[k][f_], bo[f_]), (f_, i)


def test_save_and_load_map_round_trip(oracle_mod, hip_lib, tmp_path):
    """Mapper::saveLayerCake / loadMap (nvblox_node.cpp:1668,1703): all three layers survive the file bit-for-bit, ESDF and
    mesh regenerate identically from the loaded TSDF, and a bad file leaves the map untouched."""
    from isaac_ros_nvblox_amd import mapper as M
    a = M.Mapper(M.default_params(), block_capacity=1 << 13)
    for d, rgb, T in H.frames(4, H.SMALL_CAM, color=True, stride=11):
        a.integrate_depth(d, T, H.SMALL_CAM); a.integrate_color(rgb, T, H.SMALL_CAM)
    a.update_esdf(); a.update_color_mesh()
    path = tmp_path / "map.nvbxmap"
    a.save_map(path)
    assert path.stat().st_size > a.num_blocks(M.LAYER_TSDF) * 4096
    b = M.Mapper(M.default_params(), block_capacity=1 << 13)
    d0, rgb0, T0 = H.frames(1, H.SMALL_CAM, start=100)[0]
    b.integrate_depth(d0, T0, H.SMALL_CAM)                       # content that the load must replace
    b.load_map(path)
    saved = H.map_state(a, slice=True, mesh=True)
    H.assert_same_map(saved, H.map_state(b, slice=True), "the loaded map", min_blocks=11)
    # loaded TSDF blocks are dirty: the ESDF / mesh recomputed from them equal the saved mapper's
    b.update_esdf(); b.update_color_mesh()
    H.assert_same_map(saved, b, "ESDF and mesh recomputed from the loaded map", layers=(M.LAYER_TSDF, M.LAYER_COLOR))
    ma, mb = a.mesh(), b.mesh()
    assert len(ma) > 10 and all(np.array_equal(ma[k]["colors"], mb[k]["colors"]) for k in ma)
    # both mappers keep integrating identically
    d1, rgb1, T1 = H.frames(1, H.SMALL_CAM, start=60)[0]
    a.integrate_depth(d1, T1, H.SMALL_CAM); b.integrate_depth(d1, T1, H.SMALL_CAM)
    H.assert_same_map(a, b, "one further frame", layers=(M.LAYER_TSDF,))
    # error behaviour: missing file, garbage file, wrong voxel size -> error, map untouched
    n_before = b.num_blocks(M.LAYER_TSDF)
    bad = tmp_path / "bad.nvbxmap"; bad.write_bytes(b"not a map file at all" * 10)
    for p in (tmp_path / "missing.nvbxmap", bad):
        with pytest.raises(RuntimeError):
            b.load_map(p)
    c = M.Mapper(M.default_params(voxel_size=0.1), block_capacity=1 << 10)
    with pytest.raises(RuntimeError):
        c.load_map(path)
    trunc = tmp_path / "trunc.nvbxmap"; trunc.write_bytes(path.read_bytes()[: path.stat().st_size // 2])
    with pytest.raises(RuntimeError):
        b.load_map(trunc)
    assert b.num_blocks(M.LAYER_TSDF) == n_before


def test_backproject_depth_and_transform(hip_lib):
    """DepthImageBackProjector::backProjectOnGPU + transformPointcloudOnGPU (nvblox_node.cpp:1128-1131, fuser_node.cpp:294-297)."""
    from isaac_ros_nvblox_amd import mapper as M
    g = M.Mapper(M.default_params(), block_capacity=1 << 10)
    cam = H.SMALL_CAM
    d, _, T = H.frames(1, cam, color=False)[0]
    d = d.copy(); d[:10, :] = 0.0; d[50, 60] = -1.0                   # invalid pixels are dropped
    for max_d in (0.0, 3.0):
        pts = g.backproject_depth(d, cam, max_d)
        valid = (d > 0) & ((d <= max_d) if max_d > 0 else True)
        assert len(pts) == int(valid.sum()) > 1000
        v, u = np.nonzero(valid)
        want = np.stack([((u + 0.5 - cam[2]) / cam[0]) * d[v, u], ((v + 0.5 - cam[3]) / cam[1]) * d[v, u], d[v, u]], -1).astype(np.float32)
        order = lambda a: a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))]
        assert np.abs(order(pts) - order(want)).max() <= 1e-5
    # in the layer frame the points lie on the analytic scene surface
    from test_oracle_ground_truth import scene_sdf
    pl = g.backproject_depth(d, cam, 0.0, T_L_C=T)
    assert np.abs(scene_sdf(pl.astype(np.float64))).max() < 2e-3
    with pytest.raises(RuntimeError):
        g.lib.nvbx_backproject_depth  # symbol exists
        import ctypes as C, torch
        dd = torch.from_numpy(d).cuda(); out = torch.empty((10, 3), device="cuda"); n = C.c_int64()
        g._check(g.lib.nvbx_backproject_depth(g._h, C.c_void_p(dd.data_ptr()), d.shape[0], d.shape[1], C.byref(g._cam(cam)), 0.0,
                                              C.c_void_p(out.data_ptr()), 10, C.byref(n)))       # capacity too small -> NVBX_E_CAPACITY


def test_combined_slice_of_two_mappers(oracle_mod, hip_lib):
    """EsdfSlicer::sliceLayersToCombinedDistanceImage (nvblox_node.cpp:836-840): union AABB, min of the observed distances."""
    from isaac_ros_nvblox_amd import mapper as M
    a = M.Mapper(M.default_params(), block_capacity=1 << 13); b = M.Mapper(M.default_params(), block_capacity=1 << 13)
    fa = H.frames(3, H.SMALL_CAM, color=False, stride=10); fb = H.frames(3, H.SMALL_CAM, color=False, start=35, stride=10)
    for d, _, T in fa: a.integrate_depth(d, T, H.SMALL_CAM)
    for d, _, T in fb: b.integrate_depth(d, T, H.SMALL_CAM)
    a.update_esdf(); b.update_esdf()
    ia, aa = a.esdf_slice_image(1000.0); ib, ab = b.esdf_slice_image(1000.0)
    ic, ac = a.esdf_slice_image_combined(b, 1000.0)
    x0, y0 = min(aa[0], ab[0]), min(aa[1], ab[1]); x1, y1 = max(aa[3], ab[3]), max(aa[4], ab[4])
    assert np.allclose(ac[[0, 1, 3, 4]], [x0, y0, x1, y1], atol=1e-5)
    W, Hh = int(round((x1 - x0) / 0.05)), int(round((y1 - y0) / 0.05))
    assert ic.shape == (Hh, W)
    def big(img, ab_):
        o = np.full((Hh, W), 1000.0, np.float32)
        r0, c0 = int(round((ab_[1] - y0) / 0.05)), int(round((ab_[0] - x0) / 0.05))
        o[r0:r0 + img.shape[0], c0:c0 + img.shape[1]] = img
        return o
    A, B = big(ia, aa), big(ib, ab)
    ka, kb = A < 999.0, B < 999.0
    want = np.where(ka & kb, np.minimum(A, B), np.where(ka, A, np.where(kb, B, 1000.0))).astype(np.float32)
    assert (ka & kb).sum() > 100 and (ka ^ kb).sum() > 100
    assert np.array_equal(ic, want)
    # a mapper combined with itself is its own slice
    ii, _ = a.esdf_slice_image_combined(a, 1000.0)
    assert np.array_equal(ii, ia)


def test_layer_type_and_esdf_mode_are_fixed_once_the_map_has_content(hip_lib):
    from isaac_ros_nvblox_amd import mapper as M
    g = M.Mapper(M.default_params(), block_capacity=1 << 10)
    g.set_params(M.default_params(esdf_mode=1)); g.set_params(M.default_params())          # empty map: allowed
    d, _, T = H.frames(1, H.SMALL_CAM, color=False)[0]
    g.integrate_depth(d, T, H.SMALL_CAM)
    for kw in (dict(projective_layer_type=1), dict(esdf_mode=1), dict(voxel_size=0.1)):
        with pytest.raises(RuntimeError):
            g.set_params(M.default_params(**kw))
    g.set_params(M.default_params(max_integration_distance_m=3.0))                        # ordinary knobs: any time
    g.clear()
    g.set_params(M.default_params(projective_layer_type=1))                               # empty again
    g.integrate_depth(d, T, H.SMALL_CAM)
    assert g.num_blocks(M.LAYER_OCCUPANCY) > 10 and g.num_blocks(M.LAYER_TSDF) == 0


def test_camera_model_must_describe_the_image(hip_lib):
    """A camera whose width/height differ from the image's cols/rows (or with a non-positive focal length) is refused before
    any launch -- the kernels bound projections by the model and address pixels by the image; absent blocks read as zeros."""
    from isaac_ros_nvblox_amd import mapper as M
    g = M.Mapper(M.default_params(), block_capacity=1 << 10)
    d, rgb, T = H.frames(1, H.SMALL_CAM, color=True)[0]
    for cam in ((80.0, 80.0, 79.5, 59.5, 320, 240), (80.0, 80.0, 79.5, 59.5, 120, 160), (0.0, 80.0, 79.5, 59.5, 160, 120)):
        with pytest.raises(M.NvbxError, match="camera"):
            g.integrate_depth(d, T, cam)
        with pytest.raises(M.NvbxError, match="camera"):
            g.integrate_color(rgb, T, cam)
    assert g.num_blocks(M.LAYER_TSDF) == 0
    g.integrate_depth(d, T, H.SMALL_CAM)
    have = g.block_indices(M.LAYER_TSDF)[:1]
    idx = np.concatenate([have, np.array([[1000, 1000, 1000]], np.int32)])
    vox, found = g.get_blocks(M.LAYER_TSDF, idx)
    assert list(found) == [1, 0] and not np.asarray(vox[1]).view(np.uint8).any() and np.asarray(vox[0]).view(np.uint8).any()


def test_poses_outside_the_addressable_range_are_refused(hip_lib):
    """Hash keys hold 21 bits per axis: a non-finite pose, or one further out than 2^20 blocks, is an error, not an alias."""
    from isaac_ros_nvblox_amd import mapper as M
    g = M.Mapper(M.default_params(), block_capacity=1 << 10)
    d, rgb, T = H.frames(1, H.SMALL_CAM, color=True)[0]
    far = np.array(T, np.float32); far[0, 3] = 5.0e5
    nan = np.array(T, np.float32); nan[1, 1] = np.nan
    for bad in (far, nan):
        with pytest.raises(M.NvbxError, match="addressable"):
            g.integrate_depth(d, bad, H.SMALL_CAM)
        with pytest.raises(M.NvbxError, match="addressable"):
            g.integrate_color(rgb, bad, H.SMALL_CAM)
    with pytest.raises(M.NvbxError):
        g.set_blocks(M.LAYER_TSDF, [[1 << 20, 0, 0]], np.zeros((1, 512), M._DT[M.LAYER_TSDF]))
    assert g.num_blocks(M.LAYER_TSDF) == 0
    ok = np.array(T, np.float32); ok[0, 3] += 4.0e5          # 400 km out: fine
    g.integrate_depth(d, ok, H.SMALL_CAM)
    assert g.num_blocks(M.LAYER_TSDF) > 10


@pytest.mark.parametrize("kw", [dict(max_integration_distance_m=0.0), dict(lidar_max_integration_distance_m=float("inf")),
                                dict(truncation_distance_vox=-1.0), dict(projective_layer_type=3), dict(esdf_mode=2),
                                dict(projective_layer_type=1, free_region_occupancy_probability=1.0)])
def test_parameter_values_the_kernels_rely_on_are_checked(hip_lib, kw):
    """Values that bound the kernels' ray walks and address arithmetic are refused at creation and in set_params."""
    from isaac_ros_nvblox_amd import mapper as M
    with pytest.raises(M.NvbxError):
        M.Mapper(M.default_params(**kw), block_capacity=1 << 10)
    g = M.Mapper(M.default_params(), block_capacity=1 << 10)
    with pytest.raises(M.NvbxError):
        g.set_params(M.default_params(**kw))
    g.set_params(M.default_params(max_integration_distance_m=4.0))
