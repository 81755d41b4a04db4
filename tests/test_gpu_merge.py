"""Map merging on the GPU (nvbx_merge_map / Mapper.merge_from; SEMANTICS.md "Map merging") against the numpy model of tests/merge_independent.py
-- block sets, result records and voxels exactly, bit for bit -- against an analytic plane, and against the rest of the mapper afterwards.
80 x 60 frames of the synthetic room, at most four frames per mapper, block_capacity at most 1 << 12."""
import numpy as np
import pytest

import helpers as H
import merge_independent as MI

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05
F32 = np.float32
pose = MI.pose

TRANSFORMS = {
    "identity": pose([0, 0, 1], 0.0, [0, 0, 0]),
    "whole_blocks": pose([0, 0, 1], 0.0, np.array([2, -1, 1]) * 8 * VS),
    "sub_voxel": pose([0, 0, 1], 0.0, np.array([0.5, -0.25, 0.125]) * VS),
    "z45_negative": pose([0, 0, 1], 45.0, [-6.3, -5.1, -2.2]),
    "general_30": pose([1, 2, 3], 30.0, [0.37, -0.21, 0.13]),
}


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _mapper(cap=1 << 12, **params):
    M, _ = _mods()
    return M.Mapper(M.default_params(**params), device=0, block_capacity=cap)


def _trunc(p):
    return F32(p.truncation_distance_vox) * F32(p.voxel_size)


def _integrate(m, frames, color=True):
    for d, rgb, T in frames:
        m.integrate_depth(d, T, CAM)
        if color:
            m.integrate_color(rgb, T, CAM)


def _blocks_of(m):
    """({block: tsdf[512]}, {block: color[512]}): the form the merge model takes"""
    M, _ = _mods()
    return MI.read_layers(m, M)


def _tsdf_color_state(m):
    M, _ = _mods()
    return H.map_state(m, layers=(M.LAYER_TSDF, M.LAYER_COLOR))


def _merge_and_check(dst, src, T, what="", **options):
    """merge on the GPU, the model on the layers read before it; everything compared exactly.  -> (model result, GPU result, layers after)"""
    dt, dc = _blocks_of(dst); st, sc = _blocks_of(src)
    src_before = _tsdf_color_state(src)
    p = dst.params
    r = MI.merge(dt, dc, st, sc, T, p.voxel_size, _trunc(p), p.max_weight, **{**{k: MI.DEFAULTS[k] for k in MI.DEFAULTS}, **options})
    res = dst.merge_from(src, T, **options)
    at, ac = _blocks_of(dst)
    assert set(at) == set(r["tsdf"]) == set(dt) | set(r["candidates"]), what
    assert (res.source_blocks, res.candidate_blocks, res.blocks_allocated, res.voxels_fused, res.color_voxels_fused, res.status) == \
        (r["source_blocks"], r["candidate_blocks"], r["blocks_allocated"], r["voxels_fused"], r["color_voxels_fused"], r["status"]), (what, res)
    for k, v in r["tsdf"].items():
        bad = (at[k]["distance"].view(np.uint32) != v["distance"].view(np.uint32)) | (at[k]["weight"].view(np.uint32) != v["weight"].view(np.uint32))
        assert not bad.any(), "%s: %d TSDF voxels of block %r differ from the model" % (what, int(bad.sum()), k)
        if k in dt and k not in r["fused"]:
            assert at[k].tobytes() == dt[k].tobytes(), what                     # a block the merge did not go over
    assert set(ac) == set(r["color"]), what
    for k, v in r["color"].items():
        assert ac[k].tobytes() == v.tobytes(), "%s: colour block %r differs from the model" % (what, k)
    H.assert_same_map(src_before, src, what + " (src is not modified)")
    return r, res, (at, ac)


@pytest.fixture(scope="module")
def room_frames():
    _, S = _mods()
    sc = S.Scene()
    out = []
    for i in (0, 9, 18, 4, 13, 27):
        T = S.trajectory_pose(i)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


@pytest.fixture(scope="module")
def src_room(hip_lib, room_frames):
    m = _mapper()
    _integrate(m, room_frames[:3])
    m.synchronize()
    return m


# ---- 1. against the model
@pytest.mark.parametrize("name", list(TRANSFORMS))
@pytest.mark.parametrize("dst_case", ["empty", "overlapping"])
def test_merge_equals_the_model(src_room, room_frames, dst_case, name):
    dst = _mapper()
    if dst_case == "overlapping":
        _integrate(dst, room_frames[3:5])
    r, res, _ = _merge_and_check(dst, src_room, TRANSFORMS[name], "%s %s" % (dst_case, name))
    assert res.status_name == "OK" and r["voxels_fused"] > 10000 and r["color_voxels_fused"] > 1000
    if dst_case == "overlapping" and name in ("identity", "sub_voxel", "general_30"):
        assert r["blocks_allocated"] < r["candidate_blocks"]                 # some candidates existed: both paths of the enumeration ran
    dst.close()


# ---- 2. hand-made blocks
def _blocks(rng, keys, weights=(1.0,), dist=0.15, color=False):
    t, c = {}, {}
    for k in keys:
        b = np.zeros(512, MI.TSDF_DT)
        b["distance"] = rng.uniform(-dist, dist, 512).astype(F32); b["weight"] = rng.choice(np.asarray(weights, F32), 512)
        t[tuple(k)] = b
        if color:
            q = np.zeros(512, MI.COLOR_DT)
            for ch in "rgb":
                q[ch] = rng.integers(0, 256, 512)
            q["weight"] = rng.choice(np.array([0.0, 1.0, 2.5], F32), 512)
            c[tuple(k)] = q
    return t, c


def _upload(m, tsdf, color=None):
    M, _ = _mods()
    if tsdf:
        ks = sorted(tsdf)
        m.set_blocks(M.LAYER_TSDF, np.array(ks, np.int32), np.stack([tsdf[k] for k in ks]))
    if color:
        ks = sorted(color)
        m.set_blocks(M.LAYER_COLOR, np.array(ks, np.int32), np.stack([color[k] for k in ks]))


def _cube(origin, n):
    return [(origin[0] + x, origin[1] + y, origin[2] + z) for x in range(n) for y in range(n) for z in range(n)]


def test_a_single_block_under_the_general_rotation(hip_lib):
    rng = np.random.default_rng(1)
    src = _mapper(1 << 8); dst = _mapper(1 << 8)
    t, c = _blocks(rng, [(3, -2, 1)], color=True)
    _upload(src, t, c)
    r, res, _ = _merge_and_check(dst, src, TRANSFORMS["general_30"], "single block")
    assert 1 <= res.candidate_blocks <= 27 and res.candidate_blocks == len(MI.candidates(TRANSFORMS["general_30"], [(3, -2, 1)], VS))
    assert res.voxels_fused > 0                                            # the block's own interior samples are valid
    src.close(); dst.close()


def test_one_weak_corner_invalidates_exactly_the_samples_that_use_it(hip_lib):
    rng = np.random.default_rng(2)
    T = TRANSFORMS["general_30"]
    keys = _cube((0, 0, 0), 2)
    t, _ = _blocks(rng, keys)
    weak = {k: v.copy() for k, v in t.items()}
    weak[(0, 0, 0)]["weight"][7 + 8 * 7 + 64 * 7] = F32(5e-5)             # voxel (7, 7, 7) of block 0: a corner of samples in all eight blocks
    out = []
    for blocks in (t, weak):
        src = _mapper(1 << 8); dst = _mapper(1 << 8)
        _upload(src, blocks)
        r, _, _ = _merge_and_check(dst, src, T, "weak corner")
        out.append(r)
        src.close(); dst.close()
    full, holed = out
    cand = np.array(full["candidates"])
    b, _, ok = MI.base_voxels(MI.sample_positions(T, cand, VS), VS)
    uses = ok & ((b <= 7) & (b >= 6)).all(axis=-1)                         # base voxel in {6, 7}^3: the weak voxel (7, 7, 7) is one of its corners
    lost = 0
    for i, k in enumerate(full["candidates"]):
        want = full["fused"][k] & ~uses[i]
        assert np.array_equal(holed["fused"][k], want), k
        lost += int((full["fused"][k] & uses[i]).sum())
    assert lost > 0 and full["voxels_fused"] - holed["voxels_fused"] == lost


def test_two_blocks_adjacent_across_a_face_and_the_options(hip_lib):
    """corners from two slots (a z face: the pair load splits, an x face: it does not); dst near max_weight; weight_scale 0.25; merge_color 0"""
    rng = np.random.default_rng(3)
    for axis in (0, 2):
        other = [0, 0, 0]; other[axis] = 1
        st, sc = _blocks(rng, [(0, 0, 0), tuple(other)], weights=(0.5, 1.0, 3.0), color=True)
        dt, dc = _blocks(rng, _cube((-1, -1, -1), 3), weights=(0.0, 4.6, 4.99, 5.0), color=True)
        for T, opts in ((TRANSFORMS["sub_voxel"], {}), (pose([1, 0, 0], 3.0, [0.01, 0.02, -0.015]), {"weight_scale": 0.25}),
                        (TRANSFORMS["sub_voxel"], {"merge_color": 0}), (TRANSFORMS["identity"], {"min_weight": 0.75})):
            src = _mapper(1 << 8); dst = _mapper(1 << 8)
            _upload(src, st, sc); _upload(dst, dt, dc)
            r, res, (at, ac) = _merge_and_check(dst, src, T, "axis %d %r" % (axis, opts), **opts)
            assert res.voxels_fused > 0
            w = np.concatenate([at[k]["weight"] for k in r["candidates"]])
            assert (w <= F32(5.0)).all() and (w == F32(5.0)).any()        # the clamp was reached
            if opts.get("merge_color", 1) == 0:
                assert res.color_voxels_fused == 0
                assert set(ac) == set(dc) and all(ac[k].tobytes() == dc[k].tobytes() for k in dc), "merge_color = 0 leaves dst's colour layer alone"
            else:
                assert res.color_voxels_fused > 0
            src.close(); dst.close()


def test_a_source_without_colour_blocks(hip_lib):
    rng = np.random.default_rng(4)
    st, _ = _blocks(rng, _cube((0, 0, 0), 2))
    src = _mapper(1 << 8); dst = _mapper(1 << 8)
    _upload(src, st)
    r, res, (_, ac) = _merge_and_check(dst, src, TRANSFORMS["general_30"], "no colour")
    assert res.voxels_fused > 0 and res.color_voxels_fused == 0 and ac == {}
    src.close(); dst.close()


# ---- 3. an analytic plane (shares nothing with the model)
def test_a_plane_stays_the_plane(hip_lib):
    """d = n . p + c in src, weight 1 inside the truncation band, 0 outside.  Every fused voxel of dst must read n' . p_D + c' of the transformed
    plane within 2e-5 m: positions up to 4 m are rounded a few times by at most 2.4e-7 m each (the centre, three products and three sums of the
    transform: about 4e-6 m in all), the interpolation of values below 0.2 m rounds by about 1e-8 m per operation; 2e-5 m is four times the sum."""
    M, _ = _mods()
    n = np.array([0.36, -0.48, 0.8]); c0 = -3.12                           # the plane passes through (1.2, -1.6, 2.4), the middle of the patch; all within +-4 m
    centre_blk = np.array([3, -4, 6])
    keys = _cube(tuple(centre_blk - 3), 6)
    trunc = 0.2
    t = {}
    for k in keys:
        g = 8 * np.array(k) + MI.LANE_XYZ
        p = (g + 0.5) * float(F32(VS))
        d = p @ n + c0
        b = np.zeros(512, MI.TSDF_DT)
        b["distance"] = np.clip(d, -trunc, trunc).astype(F32); b["weight"] = (np.abs(d) < trunc - 1e-6).astype(F32)
        t[k] = b
    assert max(abs((8 * np.array(k) + 8) * VS).max() for k in keys) < 4.0
    src = _mapper(1 << 9); dst = _mapper(1 << 12)
    _upload(src, t)
    T = TRANSFORMS["general_30"]
    res = dst.merge_from(src, T)
    assert res.status_name == "OK"
    at, _ = _blocks_of(dst)
    T64 = T.astype(np.float64)
    n2 = T64[:3, :3] @ n; c2 = c0 - n2 @ T64[:3, 3]
    Tinv = np.linalg.inv(T64)
    lo = (8 * (centre_blk - 3) + 2) * VS; hi = (8 * (centre_blk + 3) - 2) * VS      # the source patch less two voxels: every corner of a sample in there exists
    worst, fused_total, crossed, crossed_fused = 0.0, 0, 0, 0
    for k, blk in at.items():
        pD = (8 * np.array(k) + MI.LANE_XYZ + 0.5) * float(F32(VS))
        want = pD @ n2 + c2
        f = blk["weight"] > 0
        fused_total += int(f.sum())
        if f.any():
            worst = max(worst, float(np.abs(blk["distance"][f].astype(np.float64) - want[f]).max()))
            assert (blk["weight"][f] == F32(1.0)).all()
        pS = pD @ Tinv[:3, :3].T + Tinv[:3, 3]
        inside = ((pS > lo) & (pS < hi)).all()
        if inside and (np.abs(want) < trunc / 2).any():                     # the band crosses the block well inside the patch: a voxel there has all its corners in the band
            crossed += 1; crossed_fused += int(f.any())
    assert fused_total == res.voxels_fused > 5000
    assert crossed > 8 and crossed_fused == crossed
    assert worst <= 2e-5, worst
    src.close(); dst.close()


# ---- 4. the rest of the mapper afterwards
def test_the_mapper_afterwards_behaves_as_after_set_blocks(src_room, room_frames, tmp_path):
    M, _ = _mods()
    dst = _mapper()
    _integrate(dst, room_frames[3:5])
    res = dst.merge_from(src_room, TRANSFORMS["general_30"])
    assert res.status_name == "OK"
    at, ac = _blocks_of(dst)
    merged = _tsdf_color_state(dst)
    twin = _mapper()
    _upload(twin, at, ac)
    H.assert_same_map(merged, twin, "the twin holds the merged layers")
    dst.save_map(str(tmp_path / "merged.nvblx"))
    loaded = _mapper(); loaded.load_map(str(tmp_path / "merged.nvblx"))
    H.assert_same_map(merged, loaded, "save_map / load_map")
    loaded.close()
    for m in (dst, twin):
        m.update_esdf(); m.update_color_mesh()
    sa, ba = dst.esdf_slice_image(); sb, bb = twin.esdf_slice_image()
    assert sa.shape == sb.shape and np.array_equal(sa, sb) and np.array_equal(ba, bb)
    ma, mb = dst.mesh(), twin.mesh()
    assert set(ma) == set(mb) and sum(len(v["triangles"]) for v in ma.values()) > 1000
    for k in ma:
        assert np.array_equal(ma[k]["triangles"], mb[k]["triangles"]), k
        assert ma[k]["vertices"].shape == mb[k]["vertices"].shape and np.abs(ma[k]["vertices"] - mb[k]["vertices"]).max(initial=0.0) <= 1e-4, k
        assert np.array_equal(ma[k]["colors"], mb[k]["colors"]), k
    # one further frame: the colour integration decides per block from the band flags the merge (or set_blocks) left
    d, rgb, T = room_frames[5]
    for m in (dst, twin):
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM); m.update_esdf()
    H.assert_same_map(_tsdf_color_state(dst), twin, "one further depth + colour frame")
    assert np.array_equal(dst.esdf_slice_image()[0], twin.esdf_slice_image()[0])
    # and the flags agree with in_band over the voxels: a colour frame over a map whose flags were recomputed from scratch (set_params does so
    # when the truncation distance changes -- here it is uploaded afresh) gives the same colours
    fresh = _mapper()
    t2, c2 = _blocks_of(dst)
    _upload(fresh, t2, c2)
    for m in (dst, fresh):
        m.integrate_color(room_frames[4][1], room_frames[4][2], CAM)
    H.assert_same_map(_tsdf_color_state(dst), fresh, "colour frame over the merged map's band flags")
    dst.close(); twin.close(); fresh.close()


# ---- 5. ordering and pipelining
def _pipelined_pair(room_frames, deferral, sync):
    """src and dst each with a held-back colour frame and ESDF update, the merge, then at once another depth frame into src"""
    src = _mapper(); dst = _mapper()
    for m in (src, dst):
        m.set_color_deferral(deferral)
    _integrate(src, room_frames[:2]); src.update_esdf()
    _integrate(dst, room_frames[3:5]); dst.update_esdf()
    if sync:
        src.synchronize(); dst.synchronize()
    res = dst.merge_from(src, TRANSFORMS["general_30"])
    if sync:
        src.synchronize(); dst.synchronize()
    src.integrate_depth(room_frames[2][0], room_frames[2][2], CAM)
    if sync:
        src.synchronize(); dst.synchronize()
    out = (_tsdf_color_state(dst), _tsdf_color_state(src), (res.candidate_blocks, res.voxels_fused, res.color_voxels_fused, res.status))
    src.close(); dst.close()
    return out


def test_held_back_work_and_a_following_source_frame(hip_lib, room_frames):
    ref = _pipelined_pair(room_frames, False, True)
    assert ref[2][1] > 10000 and ref[2][2] > 1000
    for deferral, sync in ((True, False), (True, True), (False, False)):
        got = _pipelined_pair(room_frames, deferral, sync)
        what = "deferral %r, synchronised %r" % (deferral, sync)
        assert got[2] == ref[2], what
        H.assert_same_map(got[0], ref[0], what + ": dst"); H.assert_same_map(got[1], ref[1], what + ": src")


# ---- 6. growth and capacity
def test_a_small_destination_grows(src_room):
    dst = _mapper(64)
    _merge_and_check(dst, src_room, TRANSFORMS["general_30"], "growth from 64 blocks")
    assert dst.capacity > 64
    dst.close()


def test_capacity_error_leaves_the_destination_unchanged(src_room):
    M, _ = _mods()
    rng = np.random.default_rng(6)
    dst = _mapper(64)
    dst.set_max_capacity(64)
    t, c = _blocks(rng, _cube((0, 0, 0), 2), color=True)
    _upload(dst, t, c)
    before = _tsdf_color_state(dst)
    with pytest.raises(M.NvbxError, match=r"error -3: nvbx_merge_map"):
        dst.merge_from(src_room, TRANSFORMS["identity"])
    assert dst.capacity == 64
    H.assert_same_map(before, dst, "after the capacity error")
    # and the mapper is usable: a merge that fits goes through
    small = _mapper(1 << 8)
    _upload(small, *_blocks(rng, [(0, 0, 0)]))
    assert dst.merge_from(small, TRANSFORMS["identity"]).status_name in ("OK", "NO_OVERLAP")
    small.close(); dst.close()


# ---- 7. refusals
def test_refusals_name_the_call_and_change_nothing(hip_lib):
    import torch
    M, _ = _mods()
    rng = np.random.default_rng(7)
    t, c = _blocks(rng, _cube((0, 0, 0), 2), color=True)
    src = _mapper(1 << 8); dst = _mapper(1 << 8)
    _upload(src, t, c); _upload(dst, *_blocks(rng, [(0, 0, 1), (5, 5, 5)], color=True))
    before = _tsdf_color_state(dst)
    I = TRANSFORMS["identity"]
    other_vs = _mapper(1 << 8, voxel_size=0.1)
    occ = _mapper(1 << 8, projective_layer_type=1)
    free = _mapper(1 << 8, projective_layer_type=2)
    bad_T = {}
    T = I.copy(); T[0, 3] = np.nan; bad_T["nan"] = T
    T = I.copy(); T[1, 1] = np.inf; bad_T["inf"] = T
    T = I.copy(); T[2, 3] = 1e9; bad_T["out of range"] = T
    T = I.copy(); T[:3, :3] *= F32(1.001); bad_T["scaled"] = T
    T = I.copy(); T[2, 2] = -1.0; bad_T["mirrored"] = T
    cases = [("same", dst, dst, I, {}), ("voxel size", dst, other_vs, I, {}), ("occupancy src", dst, occ, I, {}), ("occupancy dst", occ, src, I, {}),
             ("freespace src", dst, free, I, {}), ("freespace dst", free, src, I, {})]
    cases += [(k, dst, src, v, {}) for k, v in bad_T.items()]
    cases += [("min_weight nan", dst, src, I, {"min_weight": float("nan")})]
    cases += [("weight_scale %r" % w, dst, src, I, {"weight_scale": w}) for w in (0.0, -1.0, float("inf"), float("nan"))]
    if torch.cuda.device_count() > 1:
        far = M.Mapper(M.default_params(), device=1, block_capacity=1 << 8)
        cases.append(("devices", dst, far, I, {}))
    for what, d, s, T, opts in cases:
        with pytest.raises(M.NvbxError, match=r"error -1: nvbx_merge_map: "):
            d.merge_from(s, T, **opts)
        H.assert_same_map(before, dst, what)
    buf = torch.empty(M.MERGE_RESULT_BYTES + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        dst.merge_from(src, I, out=buf[4:4 + M.MERGE_RESULT_BYTES])
    with pytest.raises(TypeError):
        dst.merge_from(src, I, no_such_option=1)
    # after all of it the merge itself still works
    _merge_and_check(dst, src, I, "after the refusals")
    for m in (src, dst, other_vs, occ, free):
        m.close()


# ---- 8. empty and disjoint
def test_empty_source_and_no_overlap(hip_lib):
    M, _ = _mods()
    rng = np.random.default_rng(8)
    src = _mapper(1 << 8); dst = _mapper(1 << 8)
    res = dst.merge_from(src, TRANSFORMS["whole_blocks"])
    assert (res.status_name, res.source_blocks, res.candidate_blocks, res.blocks_allocated, res.voxels_fused) == ("EMPTY_SOURCE", 0, 0, 0, 0)
    assert dst.num_blocks(M.LAYER_TSDF) == 0 and dst.counters()["blocks_allocated"] == 0
    t, _ = _blocks(rng, _cube((1, 1, 1), 2))
    for b in t.values():
        b["weight"] = F32(5e-5)
    _upload(src, t)
    r, res, (at, ac) = _merge_and_check(dst, src, TRANSFORMS["whole_blocks"], "no overlap")
    assert res.status_name == "NO_OVERLAP" and res.candidate_blocks == res.blocks_allocated == len(at) > 0 and res.voxels_fused == 0
    for b in at.values():
        assert (b["weight"] == 0).all() and (b["distance"] == 0).all()
    assert ac == {}
    src.close(); dst.close()
