"""The reader calls of mapper.py on one tiny map (a 64 x 48 depth frame of a wall, 8 feature channels, one feature frame): preallocated
outputs give what the allocating call gives and allocate nothing, an empty input gives empty tensors, and a refused call leaves the error
text it always left.  What the calls compute is checked by the suites of each call; this one is about the path their arguments take
(isaac_ros_nvblox_amd/_args.py) and the shared refusals of the C-ABI (nvbx::refuse, tsdf_reader_refused, nvbx_camera_valid, seg_check)."""
import ctypes as C

import numpy as np
import pytest

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
