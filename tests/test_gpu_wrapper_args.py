"""The path the mapper's arguments take (isaac_ros_nvblox_amd/_args.py) and the shared refusals of the C-ABI (nvbx::refuse, tsdf_reader_refused,
nvbx_camera_valid, seg_check, nvbx_camera_frame_refused).  What the calls compute is checked by the suites of each call.
Reader calls, on one tiny map (a 64 x 48 depth frame of a wall, 8 feature channels, one feature frame): preallocated outputs give what the
allocating call gives and allocate nothing, an empty input gives empty tensors, and a refused call leaves the error text it always left.
Writer and converter calls, on one or two 160 x 120 frames of synthetic.Scene: every form an input may take (numpy array, device tensor,
strided device view, prepared tuple, ColorFrame, bgra8, u16 millimetres) gives the same map or the same result, byte for byte; bad input is
refused with ValueError and leaves the mapper usable; the camera-frame entry points leave the error texts they always left."""
import ctypes as C

import numpy as np
import pytest

import helpers as H
from isaac_ros_nvblox_amd import synthetic as S

pytestmark = pytest.mark.gpu

CAM = (32.0, 32.0, 31.5, 23.5, 64, 48)
STRIDE = 4
CH = 8
N = 257           # points and rays: odd, more than one workgroup of 256
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def wall(hip_lib):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(voxel_size=0.05), device=0, block_capacity=1 << 11)
    m.integrate_depth(np.full((CAM[5], CAM[4]), 2.0, np.float32), EYE, CAM)
    m.enable_features(CH)
    rng = np.random.default_rng(7)
    m.integrate_features(rng.standard_normal((CAM[5] // STRIDE, CAM[4] // STRIDE, CH)).astype(np.float16), EYE, CAM, STRIDE)
    pts = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(1.85, 2.15, N)], 1).astype(np.float32)
    dirs = np.stack([rng.uniform(-0.5, 0.5, N), rng.uniform(-0.4, 0.4, N), np.ones(N)], 1)
    dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    poses = np.stack([EYE, EYE]); poses[1, 0, 3] = 0.4
    dev = {"pts": torch.from_numpy(pts).cuda(), "origins": torch.zeros((N, 3), dtype=torch.float32, device="cuda"), "dirs": torch.from_numpy(dirs).cuda(),
           "poses": torch.from_numpy(poses.reshape(2, 16)).cuda(), "queries": torch.from_numpy(rng.standard_normal((3, CH)).astype(np.float16)).cuda()}
    yield M, torch, m, dev
    m.close()


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _same(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (what, k)
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and _bytes(x) == _bytes(y), "%s: output %d differs" % (what, k)


def _no_alloc(torch, call):
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    r = call()
    assert torch.cuda.memory_allocated() == before, "the call with out= allocated device memory"
    return r


def _by_block(idx, *vols):
    """the entries of a sparse volume come in no particular order: sorted by block index"""
    i = idx.cpu().numpy()
    order = np.lexsort((i[:, 2], i[:, 1], i[:, 0]))
    return [i[order].tobytes()] + [v.cpu().numpy()[order].tobytes() for v in vols]


def test_preallocated_outputs_match_and_allocate_nothing(wall):
    M, torch, m, dev = wall
    like = lambda ts: tuple(torch.empty_like(t) if t is not None else None for t in ts)      # noqa: E731

    # per-point and per-ray calls: the same shapes, the same bits
    for what, call in (("query_tsdf", lambda out: m.query_tsdf(dev["pts"], out=out)),
                       ("cast_rays", lambda out: m.cast_rays(dev["origins"], dev["dirs"], out=out)),
                       ("query_features", lambda out: m.query_features(dev["pts"], out=out)),
                       ("match_points", lambda out: m.match_points(dev["pts"], dev["queries"], out=out))):
        first = call(None)
        out = like(first)
        second = _no_alloc(torch, lambda: call(out))
        assert all(a is b for a, b in zip(second, out)), what
        _same(first, second, what)
    t, hit, _, _ = m.cast_rays(dev["origins"], dev["dirs"])
    assert hit.dtype == torch.bool and bool(hit.any()) and float(t.max()) > 1.9          # (the wall is there)
    assert float(m.query_features(dev["pts"])[1].max()) > 0.0                             # (and carries features)

    g1 = m.view_gain(dev["poses"], CAM)
    g2 = torch.empty_like(g1)
    assert _no_alloc(torch, lambda: m.view_gain(dev["poses"], CAM, out=g2)) is g2
    _same((g1,), (g2,), "view_gain")
    assert int(g1[0, 0]) > 0                                                              # (rays were walked)

    # capacity-sized calls: the same capacity, the same entries (in no particular order)
    idx, lab, sc, al = m.match_features(dev["queries"])
    n = int(idx.shape[0])
    assert n > 0 and al is None
    out = like((idx, lab, sc)) + (None, torch.empty(1, dtype=torch.int64, device="cuda"))
    got = _no_alloc(torch, lambda: m.match_features(dev["queries"], out=out))
    assert all(a is b for a, b in zip(got, out)) and int(out[4].item()) == n
    assert _by_block(idx, lab, sc) == _by_block(*out[:3]), "match_features"

    fi, fl, fs, fc = m.find_frontiers()
    nf = int(fi.shape[0])
    assert nf > 0 and int(fc.item()) == nf
    out = like((fi, fl, fs, fc))
    got = _no_alloc(torch, lambda: m.find_frontiers(out=out))
    assert all(a is b for a, b in zip(got, out)) and int(out[3].item()) == nf
    assert _by_block(fi, fl, fs) == _by_block(*out[:3]), "find_frontiers"

    # components: the table's rows come in no particular order -- the same background, the same records, every voxel in the same record
    ids, comps = m.label_components(idx, lab, sc)
    nc = int(comps.label.shape[0])
    assert nc > 0
    out = (torch.empty_like(ids), m.component_records(nc), torch.empty(1, dtype=torch.int64, device="cuda"))
    ids2, rec2, cnt2 = _no_alloc(torch, lambda: m.label_components(idx, lab, sc, out=out))
    assert ids2 is out[0] and rec2 is out[1] and int(cnt2.item()) == nc
    a, b = ids.cpu().numpy(), ids2.cpu().numpy()
    assert np.array_equal(a < 0, b < 0)

    def table(c):      # the record table back from its fields, as int32 words
        cols = [c.label[:, None], c.voxels[:, None], c.min_xyz, c.max_xyz, c.sum_xyz.contiguous().view(torch.int32),
                c.peak_score.contiguous().view(torch.int32)[:, None], c.peak_xyz]
        return torch.cat([x.contiguous() for x in cols], 1).cpu().numpy()
    t1, t2 = table(comps), table(m.components_view(rec2, nc))
    assert np.array_equal(t2, rec2[:nc].cpu().numpy())
    assert t1.shape == (nc, M.COMPONENT_WORDS) and sorted(map(bytes, t1)) == sorted(map(bytes, t2))
    assert np.array_equal(t1[a[a >= 0]], t2[b[b >= 0]])


def test_empty_inputs_give_empty_tensors(wall):
    M, torch, m, dev = wall
    for empty in (np.zeros((0, 3), np.float32), torch.zeros((0, 3), dtype=torch.float32, device="cuda")):
        d, g, v = m.query_tsdf(empty)
        assert (tuple(d.shape), tuple(g.shape), tuple(v.shape)) == ((0,), (0, 3), (0,)) and v.dtype == torch.bool
        t, h, c, nr = m.cast_rays(empty, empty, color=True, normals=True)
        assert (tuple(t.shape), tuple(h.shape), tuple(c.shape), tuple(nr.shape)) == ((0,), (0,), (0, 3), (0, 3))
        f, w = m.query_features(empty)
        assert (tuple(f.shape), f.dtype, tuple(w.shape)) == ((0, CH), torch.float16, (0,))
        s, w = m.match_points(empty, dev["queries"])
        assert (tuple(s.shape), tuple(w.shape)) == ((0, 3), (0,))
    for empty in (np.zeros((0, 4, 4), np.float32), torch.zeros((0, 16), dtype=torch.float32, device="cuda")):
        g = m.view_gain(empty, CAM)
        assert tuple(g.shape) == (0, 4) and g.dtype == torch.int32
    assert g.is_cuda and d.is_cuda


def test_refusal_texts(wall):
    """The error a refused call leaves (nvbx_last_error), against the texts of the source before the refusals were brought together."""
    M, torch, m, dev = wall

    def refused(call, text, exc=None):
        with pytest.raises(exc or M.NvbxError):
            call()
        assert m.lib.nvbx_last_error().decode() == text

    occ = M.Mapper(M.default_params(voxel_size=0.05, projective_layer_type=1), device=0, block_capacity=256)
    other = M.Mapper(M.default_params(voxel_size=0.05), device=0, block_capacity=256)
    try:
        refused(lambda: occ.render(EYE, CAM), "nvbx_render_view: an occupancy mapper has no TSDF layer")
        refused(lambda: occ.cast_rays(dev["origins"], dev["dirs"]), "nvbx_cast_rays: an occupancy mapper has no TSDF layer")
        refused(lambda: occ.view_gain(dev["poses"], CAM), "nvbx_view_gain: an occupancy mapper has no TSDF layer")
        refused(lambda: occ.align_points(dev["pts"], EYE), "nvbx_align_points: an occupancy mapper has no TSDF layer")
        refused(lambda: occ.find_frontiers(), "nvbx_find_frontiers: an occupancy mapper has no TSDF layer")
        refused(lambda: occ.query_tsdf(dev["pts"]), "nvbx_query_points: an occupancy mapper has no TSDF layer")

        bad_cam = (0.0,) + CAM[1:]
        refused(lambda: m.render(EYE, bad_cam), "nvbx_render_view: invalid camera")
        refused(lambda: m.view_gain(dev["poses"], bad_cam), "nvbx_view_gain: invalid camera")
        refused(lambda: m.integrate_features(np.zeros((CAM[5] // STRIDE, CAM[4] // STRIDE, CH), np.float16), EYE, bad_cam, STRIDE),
                "nvbx_integrate_features: camera sides 1 .. 32768, focal lengths > 0")
        refused(lambda: m.render(EYE, CAM, subsampling=32), "nvbx_render_view: image too small for the subsampling")
        refused(lambda: m.view_gain(dev["poses"], CAM, subsampling=32), "nvbx_view_gain: image too small for the subsampling")
        refused(lambda: m.cast_rays(dev["origins"], dev["dirs"], max_ray_length_m=float("inf")), "nvbx_cast_rays: max_ray_length_m is not finite")
        refused(lambda: m.cast_rays(dev["origins"], dev["dirs"], max_ray_length_m=1e9),
                "nvbx_cast_rays: max_ray_length_m reaches beyond the addressable block range (+-2^20 blocks)")

        refused(lambda: m.align_points(dev["pts"], EYE, max_iterations=0), "nvbx_align_points: max_iterations must be 1 .. 64")
        T_nan = EYE.copy(); T_nan[0, 3] = np.nan
        refused(lambda: m.align_points(dev["pts"], T_nan), "nvbx_align_points: the pose is not finite or out of range")
        refused(lambda: m.merge_from(other, T_nan), "nvbx_merge_map: the pose is not finite or out of range")
        refused(lambda: other.match_points(dev["pts"], dev["queries"]), "nvbx_match_points: call nvbx_enable_features first")

        # the two chained calls, at the C-ABI (the wrapper refuses these values before the library sees them): nothing is launched, the counts stay
        q = dev["queries"]
        counts = torch.full((2,), -77, dtype=torch.int64, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
        rc = m.lib.nvbx_frontier_clusters(m._h, 1e-4, 0.05, 1, None, 5, 1, None, None, None, None, 0, p(counts[0:1]), None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_frontier_clusters: connectivity must be 6 or 26"
        idx = torch.empty((1, 3), dtype=torch.int32, device="cuda"); lab = torch.empty((1, 512), dtype=torch.int32, device="cuda")
        rc = m.lib.nvbx_frontier_clusters(m._h, 1e-4, 0.05, 1, None, 26, 1, p(idx), p(lab), None, None, 1, p(counts[0:1]), None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_frontier_clusters: component_id_dev is required with capacity_blocks > 0"
        rc = m.lib.nvbx_frontier_clusters(m._h, 1e-4, 0.05, 7, None, 5, 0, None, None, None, None, 0, p(counts[0:1]), None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_frontier_clusters: min_unknown_neighbours must be 1 .. 6"      # the scan's refusals come first
        rc = m.lib.nvbx_segment_features(m._h, p(q), 3, 1, 1.0, None, 6, 0, None, None, None, None, 0, p(counts[0:1]), None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_segment_features: min_voxels must be >= 1"
        rc = m.lib.nvbx_segment_features(m._h, p(q), 3, 1, 1.0, None, 6, 1, p(idx), p(lab), None, None, 1, p(counts[0:1]), None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_segment_features: block_idx_dev, label_dev and component_id_dev are required"
        rc = m.lib.nvbx_label_components(m._h, None, None, None, (1 << 22) + 1, None, 6, 1, None, None, 0, p(counts[1:2]))
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_label_components: the number of blocks must be 0 .. 2^22"
        rc = m.lib.nvbx_label_components(m._h, None, None, None, 0, None, 6, 1, None, p(idx), 1, None)
        assert rc == -1 and m.lib.nvbx_last_error().decode() == "nvbx_label_components: the component count pointer is required"
        assert counts.tolist() == [-77, -77]
    finally:
        occ.close(); other.close()


# ------------------------------------------------------------------------------------------------ writer and converter calls
SCAM = H.SMALL_CAM
ROWS, COLS = SCAM[5], SCAM[4]


@pytest.fixture(scope="module")
def scene_frames():
    """Two frames of synthetic.Scene: (depth in whole millimetres u16, the same depth f32, rgb with three different channels, pose).
    Whole millimetres: the u16 image decodes to exactly the float32 one ((float)mm * (1.0f / 1000.0f) in the kernels)."""
    sc = S.Scene(); out = []
    for i in (0, 9):
        T = S.trajectory_pose(i)
        d, rgb = S.render(sc, T, SCAM)
        d_mm = np.round(d * 1000.0).astype(np.uint16)
        d_f32 = d_mm.astype(np.float32) * np.float32(1 / 1000)
        rgb = rgb.copy(); rgb[..., 1] //= 2; rgb[..., 2] = 255 - rgb[..., 2]      # (the scene is grey: now the channel order matters)
        out.append((d_mm, d_f32, np.ascontiguousarray(rgb), np.asarray(T, np.float32)))
    assert out[0][0].max() >= 1000 and (out[0][0] > 0).sum() > ROWS * COLS // 2
    return out


def _fresh(M, stream=None, **params):
    return M.Mapper(M.default_params(**params), device=0, block_capacity=1 << 13, stream=stream)


def _mapped(M, torch, *calls, **params):
    """A fresh mapper, fed by calls(m) in order, then update_esdf: -> its layers.  Torch's current stream is the mapper's for the duration, so
    an upload or a copy the wrapper makes is ordered ahead of the launches that read it."""
    m = _fresh(M, **params)
    try:
        with torch.cuda.stream(m.torch_stream()):
            keep = [c(m) for c in calls]      # (a prepared tuple lives until the map has been read)
            m.update_esdf()
            got = H.map_state(m)
        del keep
        return got
    finally:
        m.close()


def _strided(torch, t, dim):
    """a non-contiguous device view that holds t: every second element along `dim` of a tensor twice as long there"""
    shape = list(t.shape); shape[dim] *= 2
    wide = torch.zeros(shape, dtype=t.dtype, device=t.device)
    view = wide[(slice(None),) * dim + (slice(None, None, 2),)]
    view.copy_(t)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _prepared(prepare, *args):
    def call(m):
        a = getattr(m, prepare)(*args); m.integrate_prepared(a)
        return a
    return call


def test_input_forms_give_one_map(hip_lib, scene_frames):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    d_mm, d, rgb, T = scene_frames[0]
    assert ((d_mm.astype(np.float32) * np.float32(1 / 1000)) == d).all()
    d_t = torch.from_numpy(d).cuda(); rgb_t = torch.from_numpy(rgb).cuda()
    bgra = np.ascontiguousarray(np.concatenate([rgb[..., ::-1], np.full((ROWS, COLS, 1), 255, np.uint8)], 2))
    frame = M.ColorFrame(ROWS, COLS, 3).write(rgb)
    torch.cuda.synchronize()
    depth_forms = {
        "numpy": lambda m: m.integrate_depth(d, T, SCAM),
        "tensor": lambda m: m.integrate_depth(d_t, T, SCAM),
        "strided": lambda m: m.integrate_depth(_strided(torch, d_t, 1), T, SCAM),
        "prepared": _prepared("prepare_depth", d_t, T, SCAM),
        "u16 numpy": lambda m: m.integrate_depth(d_mm, T, SCAM),
        "i16 tensor": lambda m: m.integrate_depth(torch.from_numpy(d_mm.view(np.int16)).cuda(), T, SCAM),
    }
    color_forms = {
        "numpy": lambda m: m.integrate_color(rgb, T, SCAM),
        "tensor": lambda m: m.integrate_color(rgb_t, T, SCAM),
        "strided": lambda m: m.integrate_color(_strided(torch, rgb_t, 1), T, SCAM),
        "prepared": _prepared("prepare_color", rgb_t, T, SCAM),
        "ColorFrame": lambda m: m.integrate_color(frame, T, SCAM),
        "bgra8": lambda m: m.integrate_color(bgra, T, SCAM),
    }
    want = _mapped(M, torch, depth_forms["numpy"], color_forms["numpy"])
    for (dn, df), (cn, cf) in list(zip(depth_forms.items(), color_forms.items()))[1:]:
        H.assert_same_map(want, _mapped(M, torch, df, cf), "the numpy forms vs depth as %s, colour as %s" % (dn, cn),
                          min_blocks={M.LAYER_TSDF: 21, M.LAYER_COLOR: 1, M.LAYER_ESDF: 1})          # (all three layers hold blocks)
    frame.close()


def test_batch_and_pair_forms_give_one_map(hip_lib, scene_frames):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    ds = [f[1] for f in scene_frames]; Ts = [f[3] for f in scene_frames]
    want = _mapped(M, torch, lambda m: m.integrate_depth_batch(ds, Ts, SCAM))

    def prepared(m):
        a = m.prepare_depth_batch(ds, Ts, SCAM); m.integrate_prepared_batch(a)
        return a
    H.assert_same_map(want, _mapped(M, torch, prepared), "the batch vs the prepared batch")

    # the pair: the left half of the frame into one mapper, the right half into the other
    da = ds[0].copy(); da[:, COLS // 2:] = 0.0
    db = ds[0].copy(); db[:, :COLS // 2] = 0.0

    stream = torch.cuda.Stream()      # both mappers on it, and torch for the duration: the uploads are ordered ahead of either mapper's launches

    def pair(a_img, b_img):
        a = _fresh(M, stream.cuda_stream); b = _fresh(M, stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                a.integrate_depth_pair(a_img, b, b_img, Ts[0], SCAM)
                a.update_esdf(); b.update_esdf()
                return H.map_state(a, (M.LAYER_TSDF, M.LAYER_ESDF)), H.map_state(b, (M.LAYER_TSDF, M.LAYER_ESDF))
        finally:
            a.close(); b.close()
    da_t = torch.from_numpy(da).cuda(); db_t = torch.from_numpy(db).cuda()
    torch.cuda.synchronize()
    want_a, want_b = pair(da_t, db_t)
    with pytest.raises(AssertionError):
        H.assert_same_map(want_a, want_b)                              # (the two halves are different maps)
    got_a, got_b = pair(da, db)
    H.assert_same_map(want_a, got_a, "pair: first mapper, tensors vs numpy", min_blocks={M.LAYER_TSDF: 1})
    H.assert_same_map(want_b, got_b, "pair: second mapper, tensors vs numpy", min_blocks={M.LAYER_TSDF: 1})


def test_converters_take_numpy_and_device_tensors_alike(hip_lib, scene_frames):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    _, d, rgb, T = scene_frames[0]
    rng = np.random.default_rng(11)
    mask = (rng.random((ROWS, COLS)) < 0.3).astype(np.uint8)
    lidar = (64, 16, 0.1, -0.4, 0.4)
    cloud = np.ascontiguousarray((S.lidar_beam_dirs(lidar)[::2, ::3] * rng.uniform(1.0, 5.0, (8, 22, 1))).reshape(-1, 3).astype(np.float32))
    times = np.linspace(0.0, 100.0, len(cloud)).astype(np.float32)
    T1 = T.copy(); T1[0, 3] += 0.2
    cuda = lambda a: torch.from_numpy(a).cuda()      # noqa: E731
    rows_sorted = lambda p: np.ascontiguousarray(p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))])      # noqa: E731  (the points come in no particular order)
    m = _fresh(M, projective_layer_type=2)            # (TSDF + freespace: what detect_dynamics reads)
    try:
        with torch.cuda.stream(m.torch_stream()):
            m.integrate_depth(d, T, SCAM)
            calls = {
                "detect_dynamics": lambda dev: (m.detect_dynamics(dev(d), T, SCAM, 4.0),),
                "split_depth_by_mask": lambda dev: m.split_depth_by_mask(dev(d), dev(mask), np.eye(4, dtype=np.float32), SCAM, SCAM, 0.25, overlay=True),
                "split_color_by_mask": lambda dev: m.split_color_by_mask(dev(rgb), dev(mask)),
                "backproject_depth": lambda dev: (torch.from_numpy(rows_sorted(m.backproject_depth(dev(d), SCAM, 4.0, T))),),
                "depth_image_from_pointcloud": lambda dev: (m.depth_image_from_pointcloud(dev(cloud), lidar),),
                "motion_compensate_pointcloud": lambda dev: (m.motion_compensate_pointcloud(dev(cloud), dev(times), T, T1, 100.0),),
            }
            for what, call in calls.items():
                host = call(lambda a: a); dev = call(cuda)
                _same(host, dev, what)
                assert all(t.numel() > 0 for t in host), what
            un, ma, ov = calls["split_depth_by_mask"](cuda)
            assert float(un.max()) > 0.0 and float(ma.max()) > 0.0                          # (the mask splits the frame)
            assert float(calls["depth_image_from_pointcloud"](cuda)[0].max()) > 1.0         # (the cloud lands in the image)
    finally:
        m.close()


def test_bad_input_is_refused_with_valueerror_and_the_mapper_goes_on(hip_lib, scene_frames):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    _, d, rgb, T = scene_frames[0]
    m = _fresh(M); other = _fresh(M)
    try:
        refusals = (
            lambda: m.integrate_depth(torch.zeros((ROWS, COLS), dtype=torch.uint8, device="cuda"), T, SCAM),      # a uint8 tensor as depth
            lambda: m.integrate_color(np.zeros((ROWS, COLS, 2), np.uint8), T, SCAM),                              # a 2-channel colour image
            lambda: m.integrate_depth_pair(d, other, d[:-1], T, SCAM),                                            # two shapes in one pair
            lambda: m.set_block(M.LAYER_TSDF, (0, 0, 0), np.zeros(511, M.TSDF_DT)),                               # 511 voxels
        )
        for k, call in enumerate(refusals):
            with pytest.raises(ValueError):
                call()
            m.integrate_depth(d, T, SCAM); m.integrate_color(rgb, T, SCAM); m.update_esdf()
            assert m.num_blocks(M.LAYER_TSDF) > 0, k
            v = m.invariant_violations()
            assert v is None or not any(v), (k, v)
    finally:
        m.close(); other.close()


def test_camera_frame_refusal_texts(hip_lib):
    """The two refusals every camera-frame entry point shares, called at the C-ABI: a NULL image, and a camera one pixel wider than the image."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    a = _fresh(M); b = _fresh(M)
    try:
        k = M.Camera(80.0, 80.0, 79.5, 59.5, COLS, ROWS); wide = M.Camera(80.0, 80.0, 79.5, 59.5, COLS + 1, ROWS)
        ks = (M.Camera * 1)(k); wides = (M.Camera * 1)(wide)
        T = np.eye(4, dtype=np.float32); Tp = T.ctypes.data_as(C.c_void_p)
        img = torch.zeros((ROWS, COLS, 4), dtype=torch.uint8, device="cuda")      # (as many bytes as any of the images; never read)
        p = C.c_void_p(img.data_ptr())
        imgs = (C.c_void_p * 1)(img.data_ptr()); null_imgs = (C.c_void_p * 1)(None)
        blocks = torch.empty((4, M.Mapper.MEAS_BLOCK_BYTES), dtype=torch.uint8, device="cuda"); count = torch.zeros(1, dtype=torch.int32, device="cuda")
        pb, pc = C.c_void_p(blocks.data_ptr()), C.c_void_p(count.data_ptr())
        L = hip_lib
        cases = (
            (lambda: L.nvbx_integrate_depth(a._h, None, ROWS, COLS, Tp, C.byref(k)), "nvbx_integrate_depth: invalid argument (image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_depth(a._h, p, ROWS, COLS, Tp, C.byref(wide)),
             "nvbx_integrate_depth: camera width/height must equal the image's cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_depth_u16mm(a._h, None, ROWS, COLS, Tp, C.byref(k)), "nvbx_integrate_depth_u16mm: invalid argument (image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_depth_u16mm(a._h, p, ROWS, COLS, Tp, C.byref(wide)),
             "nvbx_integrate_depth_u16mm: camera width/height must equal the image's cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_depth_batch(a._h, 1, None, ROWS, COLS, Tp, ks), "nvbx_integrate_depth_batch: invalid argument (1 <= n <= 8, image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_depth_batch(a._h, 1, null_imgs, ROWS, COLS, Tp, ks),
             "nvbx_integrate_depth_batch: every camera's width/height must equal the images' cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_depth_batch(a._h, 1, imgs, ROWS, COLS, Tp, wides),
             "nvbx_integrate_depth_batch: every camera's width/height must equal the images' cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_depth_pair(a._h, None, b._h, p, ROWS, COLS, Tp, C.byref(k)),
             "nvbx_integrate_depth_pair: invalid argument (two different mappers, image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_depth_pair(a._h, p, b._h, p, ROWS, COLS, Tp, C.byref(wide)),
             "nvbx_integrate_depth_pair: camera width/height must equal the image's cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_color(a._h, None, ROWS, COLS, Tp, C.byref(k)), "nvbx_integrate_color: invalid argument (image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_color(a._h, p, ROWS, COLS, Tp, C.byref(wide)),
             "nvbx_integrate_color: camera width/height must equal the image's cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_color_bgra8(a._h, None, ROWS, COLS, Tp, C.byref(k)), "nvbx_integrate_color_bgra8: invalid argument"),
            (lambda: L.nvbx_integrate_color_bgra8(a._h, C.c_void_p(img.data_ptr() + 1), ROWS, COLS, Tp, C.byref(k)), "nvbx_integrate_color_bgra8: invalid argument"),
            (lambda: L.nvbx_integrate_color_bgra8(a._h, p, ROWS, COLS, Tp, C.byref(wide)),
             "nvbx_integrate_color_bgra8: camera width/height must equal the image's cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_color_batch(a._h, 1, None, ROWS, COLS, Tp, ks), "nvbx_integrate_color_batch: invalid argument (1 <= n <= 8, image sides 1 .. 32768)"),
            (lambda: L.nvbx_integrate_color_batch(a._h, 1, null_imgs, ROWS, COLS, Tp, ks),
             "nvbx_integrate_color_batch: every camera's width/height must equal the images' cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_integrate_color_batch(a._h, 1, imgs, ROWS, COLS, Tp, wides),
             "nvbx_integrate_color_batch: every camera's width/height must equal the images' cols/rows, focal lengths > 0"),
            (lambda: L.nvbx_measure_depth(a._h, None, ROWS, COLS, Tp, C.byref(k), pb, pc, 4), "nvbx_measure_depth: invalid argument"),
            (lambda: L.nvbx_measure_depth(a._h, p, ROWS, COLS, Tp, C.byref(wide), pb, pc, 4),
             "nvbx_measure_depth: camera width/height must equal the image's cols/rows, focal lengths > 0"),
        )
        for k_, (call, text) in enumerate(cases):
            assert call() == -1, (k_, text)
            assert L.nvbx_last_error().decode() == text, k_
        assert a.num_blocks(M.LAYER_TSDF) == 0 and b.num_blocks(M.LAYER_TSDF) == 0          # (nothing was integrated)
    finally:
        a.close(); b.close()
