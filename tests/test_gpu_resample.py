"""Resampling on the GPU (nvbx_resample_map / Mapper.resample_from / Mapper.coarsened; SEMANTICS.md "Resampling") against the numpy model of
tests/resample_independent.py -- candidate block sets, result records, TSDF and colour voxels exactly, bit for bit -- against merge_from at
one voxel size and one tap, and against the rest of the mapper afterwards.  Every source the model goes over holds at most 64 blocks; the
ordering test, which compares GPU runs with each other, integrates two 40 x 30 frames into its source."""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import merge_independent as MI
import resample_independent as RI

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CAM = (20.0, 20.0, 19.5, 14.5, 40, 30)
VS = 0.05
VD = {1.0: 0.05, 1.5: 0.075, 2.0: 0.1, 4.0: 0.2}
RN = [(2.0, 2), (4.0, 4), (4.0, 1), (1.5, 2), (1.0, 3), (1.0, 1)]
F32 = np.float32
pose = MI.pose


def transform(name, vd):
    """the five transforms of the cases; a whole-block translation is one of dst's blocks"""
    return {"identity": None,
            "whole_blocks": pose([0, 0, 1], 0.0, np.array([2, -1, 1]) * 8 * float(F32(vd))),
            "small": pose([1, 2, 3], 1.5, [0.02, -0.02, 0.01]),                 # 3 cm, 1.5 degrees about a general axis
            "z90": pose([0, 0, 1], 90.0, [0.11, -0.07, 0.05]),
            "general": pose([3, -1, 2], 130.0, [0.37, -0.21, 0.13])}[name]


TRANSFORM_NAMES = ("identity", "whole_blocks", "small", "z90", "general")


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _mapper(cap=1 << 10, **params):
    M, _ = _mods()
    return M.Mapper(M.default_params(**params), device=0, block_capacity=cap)


def _trunc(p):
    return F32(p.truncation_distance_vox) * F32(p.voxel_size)


def _blocks_of(m):
    M, _ = _mods()
    return MI.read_layers(m, M)


def _state(m):
    M, _ = _mods()
    return H.map_state(m, layers=(M.LAYER_TSDF, M.LAYER_COLOR))


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


def _blocks(rng, keys, weights=(1.0,), dist=0.15, color=False, weak=0.0):
    t, c = {}, {}
    for k in keys:
        b = np.zeros(512, MI.TSDF_DT)
        b["distance"] = rng.uniform(-dist, dist, 512).astype(F32); b["weight"] = rng.choice(np.asarray(weights, F32), 512)
        if weak:
            b["weight"][rng.random(512) < weak] = F32(5e-5)                     # under min_weight
        t[tuple(k)] = b
        if color:
            q = np.zeros(512, MI.COLOR_DT)
            for ch in "rgb":
                q[ch] = rng.integers(0, 256, 512)
            q["weight"] = rng.choice(np.array([0.0, 1.0, 2.5], F32), 512)
            c[tuple(k)] = q
    return t, c


def hand_source(rng, n):
    """n x n x n blocks around the origin (negative indices), holes: a block missing (n = 3), 3 % of the voxels under min_weight, two TSDF blocks
    without their colour block"""
    keys = _cube((-2, -1, -2), n)
    if n == 3:
        keys.remove((-1, 0, -1))
    t, c = _blocks(rng, keys, weights=(0.5, 1.0, 3.0), color=True, weak=0.03)
    del c[keys[0]]; del c[keys[-1]]
    return t, c


def prefilled(rng):
    return _blocks(rng, _cube((-1, -1, -1), 2), weights=(0.0, 4.6, 4.99, 5.0), color=True)


def _resample_and_check(dst, src, T, what="", **options):
    """resample on the GPU, the model on the layers read before it; everything compared exactly.  -> (model result, GPU result, layers after)"""
    dt, dc = _blocks_of(dst); st, sc = _blocks_of(src)
    src_before = _state(src)
    p = dst.params
    r = RI.resample(dt, dc, st, sc, T, src.params.voxel_size, p.voxel_size, _trunc(p), p.max_weight, **{**RI.DEFAULTS, **options})
    res = dst.resample_from(src, T, **options)
    at, ac = _blocks_of(dst)
    assert set(at) == set(r["tsdf"]) == set(dt) | set(r["candidates"]), what
    assert (res.source_blocks, res.candidate_blocks, res.blocks_allocated, res.voxels_fused, res.color_voxels_fused, res.status) == \
        (r["source_blocks"], r["candidate_blocks"], r["blocks_allocated"], r["voxels_fused"], r["color_voxels_fused"], r["status"]), (what, res)
    for k, v in r["tsdf"].items():
        bad = (at[k]["distance"].view(np.uint32) != v["distance"].view(np.uint32)) | (at[k]["weight"].view(np.uint32) != v["weight"].view(np.uint32))
        assert not bad.any(), "%s: %d TSDF voxels of block %r differ from the model" % (what, int(bad.sum()), k)
        if k in dt and k not in r["fused"]:
            assert at[k].tobytes() == dt[k].tobytes(), what                     # a block the call did not go over
    assert set(ac) == set(r["color"]), what
    for k, v in r["color"].items():
        assert ac[k].tobytes() == v.tobytes(), "%s: colour block %r differs from the model" % (what, k)
    H.assert_same_map(src_before, src, what + " (src is not modified)")
    return r, res, (at, ac)


# ---- 1. hand-made sources against the model
@pytest.fixture(scope="module")
def hand_sources(hip_lib):
    """(mapper, tsdf, colour) per block-cube size: 2 (for r < 2: the candidates are as many as the source blocks) and 3"""
    out = {}
    for n in (2, 3):
        t, c = hand_source(np.random.default_rng(40 + n), n)
        m = _mapper()
        _upload(m, t, c); m.synchronize()
        out[n] = (m, t, c)
    yield out
    for m, _, _ in out.values():
        m.close()


@pytest.mark.parametrize("name", TRANSFORM_NAMES)
@pytest.mark.parametrize("r,n", RN)
def test_resample_into_a_prefilled_map_equals_the_model(hand_sources, r, n, name):
    src = hand_sources[2 if r < 2 else 3][0]
    dst = _mapper(voxel_size=VD[r])
    _upload(dst, *prefilled(np.random.default_rng(5)))
    m, res, _ = _resample_and_check(dst, src, transform(name, VD[r]), "r %g n %d %s" % (r, n, name), taps=n)
    assert res.status_name == "OK" and m["voxels_fused"] > 0
    if name in ("identity", "small"):
        assert m["blocks_allocated"] < m["candidate_blocks"] and m["color_voxels_fused"] > 0      # some candidates existed already
    dst.close()


@pytest.mark.parametrize("r,n", RN)
def test_resample_into_an_empty_map_equals_the_model(hand_sources, r, n):
    src = hand_sources[2 if r < 2 else 3][0]
    dst = _mapper(64, voxel_size=VD[r])
    m, res, (at, _) = _resample_and_check(dst, src, transform("small", VD[r]), "empty r %g n %d" % (r, n), taps=n, weight_scale=0.5)
    assert res.status_name == "OK" and res.blocks_allocated == res.candidate_blocks == len(at) and res.voxels_fused > 0
    dst.close()


def test_the_default_tap_count_follows_the_ratio(hand_sources):
    src = hand_sources[3][0]
    for r in (1.5, 2.0, 4.0):
        dst = _mapper(voxel_size=VD[r])
        m, _, _ = _resample_and_check(dst, src, transform("small", VD[r]), "default taps, r %g" % r)
        assert m["taps"] == {1.5: 2, 2.0: 2, 4.0: 4}[r]
        dst.close()


# ---- 2. a dozen room frames
@pytest.fixture(scope="module")
def room_frames():
    _, S = _mods()
    sc = S.Scene()
    out = []
    for i in (0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 33):
        T = S.trajectory_pose(i)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


@pytest.fixture(scope="module")
def src_room(hip_lib, room_frames):
    """twelve 40 x 30 frames of the synthetic room; the 64 TSDF blocks nearest to the middle of the band of the map, with their colour"""
    M, _ = _mods()
    full = _mapper(1 << 12)
    for d, rgb, T in room_frames:
        full.integrate_depth(d, T, CAM); full.integrate_color(rgb, T, CAM)
    t, c = _blocks_of(full)
    full.close()
    band = [k for k in sorted(t) if MI.band_bits(t[k], 0.2)]
    assert len(band) >= 64
    mid = np.median(np.array(band), axis=0)
    keep = sorted(band, key=lambda k: (float(np.abs(np.array(k) - mid).sum()), k))[:64]
    m = _mapper()
    _upload(m, {k: t[k] for k in keep}, {k: c[k] for k in keep if k in c})
    m.synchronize()
    assert m.num_blocks(M.LAYER_TSDF) == 64 and m.num_blocks(M.LAYER_COLOR) > 8
    yield m
    m.close()


@pytest.mark.parametrize("r,n,name", [(2.0, 2, "identity"), (2.0, 2, "small"), (4.0, 4, "small"), (1.5, 2, "general")])
def test_room_frames_equal_the_model(src_room, r, n, name):
    dst = _mapper(voxel_size=VD[r])
    m, res, _ = _resample_and_check(dst, src_room, transform(name, VD[r]), "room r %g n %d %s" % (r, n, name), taps=n)
    assert res.status_name == "OK" and m["voxels_fused"] > (500 if r < 4 else 30) and m["color_voxels_fused"] > 20
    dst.close()


# ---- 3. one voxel size, one tap: the merge
@pytest.mark.parametrize("name", ["identity", "small", "general"])
def test_with_one_voxel_size_and_one_tap_the_result_is_merge_froms(src_room, hand_sources, name):
    T = transform(name, VS)
    I = pose([0, 0, 1], 0.0, [0, 0, 0])
    for src in (src_room, hand_sources[2][0]):
        a = _mapper(); b = _mapper()
        for m in (a, b):
            _upload(m, *prefilled(np.random.default_rng(9)))
        ra = a.resample_from(src, T, taps=1)
        rb = b.merge_from(src, I if T is None else T)
        assert bytes(ra.buffer.cpu().numpy()) == bytes(rb.buffer.cpu().numpy()), (ra, rb)
        assert ra.voxels_fused > 500 and ra.color_voxels_fused > 50
        H.assert_same_map(_state(a), b, "resample_from(taps=1) against merge_from, %s" % name)
        a.close(); b.close()


# ---- 4. the rest of the mapper afterwards
def _same_esdf_slice_and_mesh(a, b):
    for m in (a, b):
        m.update_esdf(); m.update_color_mesh()
    sa, ba = a.esdf_slice_image(); sb, bb = b.esdf_slice_image()
    assert sa.shape == sb.shape and np.array_equal(sa, sb) and np.array_equal(ba, bb)
    ma, mb = a.mesh(), b.mesh()
    assert set(ma) == set(mb)
    for k in ma:
        assert np.array_equal(ma[k]["triangles"], mb[k]["triangles"]), k
        assert ma[k]["vertices"].shape == mb[k]["vertices"].shape and np.abs(ma[k]["vertices"] - mb[k]["vertices"]).max(initial=0.0) <= 1e-4, k
        assert np.array_equal(ma[k]["colors"], mb[k]["colors"]), k
    return sa, sum(len(v["triangles"]) for v in ma.values())


def test_the_mapper_afterwards_behaves_as_after_set_blocks(src_room, room_frames, tmp_path):
    dst = _mapper(voxel_size=0.1)
    for d, rgb, T in room_frames[:2]:
        dst.integrate_depth(d, T, CAM); dst.integrate_color(rgb, T, CAM)
    res = dst.resample_from(src_room, transform("small", 0.1))
    assert res.status_name == "OK" and res.voxels_fused > 500 and res.blocks_allocated < res.candidate_blocks
    at, ac = _blocks_of(dst)
    after = _state(dst)
    twin = _mapper(voxel_size=0.1)
    _upload(twin, at, ac)
    H.assert_same_map(after, twin, "the twin holds the resampled layers")
    dst.save_map(str(tmp_path / "coarse.nvblx"))
    loaded = _mapper(voxel_size=0.1); loaded.load_map(str(tmp_path / "coarse.nvblx"))
    H.assert_same_map(after, loaded, "save_map / load_map")
    loaded.close()
    _, triangles = _same_esdf_slice_and_mesh(dst, twin)
    assert triangles > 300
    # one further frame: the colour integration decides per block from the band flags the call (or set_blocks) left
    d, rgb, T = room_frames[5]
    for m in (dst, twin):
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM); m.update_esdf()
    H.assert_same_map(_state(dst), twin, "one further depth + colour frame")
    assert np.array_equal(dst.esdf_slice_image()[0], twin.esdf_slice_image()[0])
    dst.close(); twin.close()


def test_coarsened_feeds_the_cost_volume(src_room):
    M, _ = _mods()
    st, sc = _blocks_of(src_room)
    fine = _mapper(esdf_mode=1)
    _upload(fine, st, sc)
    coarse, res = fine.coarsened(2)
    assert coarse.params.voxel_size == F32(0.1) and coarse.params.esdf_mode == 1 and coarse.device == fine.device
    assert coarse.params.truncation_distance_vox == fine.params.truncation_distance_vox and coarse.params.max_weight == fine.params.max_weight
    want = RI.resample({}, {}, st, sc, None, VS, 0.1, _trunc(coarse.params), coarse.params.max_weight)
    assert (res.status_name, res.source_blocks, res.candidate_blocks, res.voxels_fused, res.color_voxels_fused) == \
        ("OK", 64, want["candidate_blocks"], want["voxels_fused"], want["color_voxels_fused"])
    at, ac = _blocks_of(coarse)
    assert set(at) == set(want["tsdf"]) and all(at[k].tobytes() == want["tsdf"][k].tobytes() for k in at)
    assert set(ac) == set(want["color"]) and all(ac[k].tobytes() == want["color"][k].tobytes() for k in ac)
    twin = _mapper(voxel_size=0.1, esdf_mode=1)
    _upload(twin, at, ac)
    out = []
    for m in (coarse, twin):
        m.update_esdf()
        idx = np.asarray(m.block_indices(M.LAYER_ESDF), np.int32).reshape(-1, 3)
        assert len(idx) > 4
        mn = idx.min(0) * 8; size = (idx.max(0) + 1) * 8 - mn
        assert int(np.prod(size.astype(np.int64))) <= 1 << 22
        vol = m.esdf_dense_grid_device(mn, size, 1000.0)
        v = vol.cpu().numpy()
        far = np.array(np.unravel_index(int(np.argmax(np.where(np.abs(v - 1000.0) > 1.0, v, -np.inf))), v.shape), np.int32).reshape(1, 3)
        G = m.cost_volume(vol, far, robot_radius_m=0.0, inflation_radius_m=0.3, allow_unknown=1)      # from the known voxel farthest from a surface
        out.append((mn, size, vol.cpu().numpy(), G.cpu().numpy()))
    (mn_a, size_a, vol_a, G_a), (mn_b, size_b, vol_b, G_b) = out
    assert np.array_equal(mn_a, mn_b) and np.array_equal(size_a, size_b) and np.array_equal(vol_a, vol_b) and np.array_equal(G_a, G_b)
    assert (np.abs(vol_a - 1000.0) > 1.0).sum() > 100 and (G_a != M.COST_UNREACHED).sum() > 100
    with pytest.raises(M.NvbxError, match=r"error -1: nvbx_resample_map: "):
        fine.coarsened(5)
    with pytest.raises(M.NvbxError, match=r"error -1: nvbx_resample_map: "):
        fine.coarsened(0.5)
    other, res2 = fine.coarsened(4.0, block_capacity=64, taps=2, merge_color=0)
    assert other.params.voxel_size == F32(0.2) and res2.status_name == "OK" and res2.color_voxels_fused == 0 and other.num_blocks(M.LAYER_COLOR) == 0
    for m in (fine, coarse, twin, other):
        m.close()


# ---- 5. refusals, capacity, empty and disjoint
def test_refusals_name_the_call_and_change_nothing(hip_lib):
    import torch
    M, _ = _mods()
    rng = np.random.default_rng(7)
    t, c = _blocks(rng, _cube((0, 0, 0), 2), color=True)
    src = _mapper(1 << 8); dst = _mapper(1 << 8, voxel_size=0.1)
    _upload(src, t, c); _upload(dst, *_blocks(rng, [(0, 0, 1), (5, 5, 5)], color=True))
    before = _state(dst)
    I = pose([0, 0, 1], 0.0, [0, 0, 0])
    finer = _mapper(1 << 8, voxel_size=0.2)                 # as a source for dst: r = 0.5
    tiny = _mapper(1 << 8, voxel_size=0.02)                 # r = 5
    just_over = _mapper(1 << 8, voxel_size=0.0249)          # r = 4.016
    occ = _mapper(1 << 8, projective_layer_type=1); occ_d = _mapper(1 << 8, projective_layer_type=1, voxel_size=0.1)
    free = _mapper(1 << 8, projective_layer_type=2); free_d = _mapper(1 << 8, projective_layer_type=2, voxel_size=0.1)
    bad_T = {}
    T = I.copy(); T[0, 3] = np.nan; bad_T["nan"] = T
    T = I.copy(); T[1, 1] = np.inf; bad_T["inf"] = T
    T = I.copy(); T[2, 3] = 1e9; bad_T["out of range"] = T
    T = I.copy(); T[:3, :3] *= F32(1.001); bad_T["scaled"] = T
    T = I.copy(); T[2, 2] = -1.0; bad_T["mirrored"] = T
    cases = [("same", dst, dst, I, {}), ("r < 1", dst, finer, I, {}), ("r > 4", dst, tiny, I, {}), ("r just over 4", dst, just_over, None, {}),
             ("taps 5", dst, src, I, {"taps": 5}), ("taps -1", dst, src, None, {"taps": -1}),
             ("occupancy src", dst, occ, I, {}), ("occupancy dst", occ_d, src, I, {}), ("freespace src", dst, free, I, {}), ("freespace dst", free_d, src, I, {})]
    cases += [(k, dst, src, v, {}) for k, v in bad_T.items()]
    cases += [("min_weight nan", dst, src, I, {"min_weight": float("nan")})]
    cases += [("weight_scale %r" % w, dst, src, I, {"weight_scale": w}) for w in (0.0, -1.0, float("inf"), float("nan"))]
    if torch.cuda.device_count() > 1:
        far = M.Mapper(M.default_params(), device=1, block_capacity=1 << 8)
        cases.append(("devices", dst, far, I, {}))
    for what, d, s, T, opts in cases:
        with pytest.raises(M.NvbxError, match=r"error -1: nvbx_resample_map: "):
            d.resample_from(s, T, **opts)
        H.assert_same_map(before, dst, what)
    buf = torch.empty(M.MERGE_RESULT_BYTES + 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        dst.resample_from(src, I, out=buf[4:4 + M.MERGE_RESULT_BYTES])
    with pytest.raises(TypeError):
        dst.resample_from(src, I, no_such_option=1)
    with pytest.raises(TypeError):
        dst.resample_from("not a mapper")
    H.assert_same_map(before, dst, "python-side refusals")
    # after all of it the call itself still works, into a preallocated record
    out = buf[8:8 + M.MERGE_RESULT_BYTES]
    _resample_and_check(dst, src, I, "after the refusals")
    assert dst.resample_from(src, None, out=out).buffer is out
    for m in (src, dst, finer, tiny, just_over, occ, occ_d, free, free_d):
        m.close()


def test_capacity_error_leaves_the_destination_unchanged(src_room):
    M, _ = _mods()
    rng = np.random.default_rng(6)
    dst = _mapper(64)
    dst.set_max_capacity(64)
    _upload(dst, *_blocks(rng, _cube((0, 0, 0), 2), color=True))
    before = _state(dst)
    with pytest.raises(M.NvbxError, match=r"error -3: nvbx_resample_map"):
        dst.resample_from(src_room, None, taps=2)
    assert dst.capacity == 64
    H.assert_same_map(before, dst, "after the capacity error")
    small = _mapper(1 << 8)
    _upload(small, *_blocks(rng, [(0, 0, 0)]))
    assert dst.resample_from(small, None).status_name in ("OK", "NO_OVERLAP")      # the mapper is usable: a call that fits goes through
    small.close(); dst.close()


def test_a_small_destination_grows(src_room):
    dst = _mapper(64)
    _resample_and_check(dst, src_room, transform("small", VS), "growth from 64 blocks", taps=2)
    assert dst.capacity > 64
    dst.close()


def test_empty_source_and_no_overlap(hip_lib):
    M, _ = _mods()
    rng = np.random.default_rng(8)
    src = _mapper(1 << 8); dst = _mapper(1 << 8, voxel_size=0.1)
    res = dst.resample_from(src, transform("whole_blocks", 0.1))
    assert (res.status_name, res.source_blocks, res.candidate_blocks, res.blocks_allocated, res.voxels_fused) == ("EMPTY_SOURCE", 0, 0, 0, 0)
    assert dst.num_blocks(M.LAYER_TSDF) == 0 and dst.counters()["blocks_allocated"] == 0
    t, _ = _blocks(rng, _cube((1, 1, 1), 2))
    for b in t.values():
        b["weight"] = F32(5e-5)
    _upload(src, t)
    r, res, (at, ac) = _resample_and_check(dst, src, transform("whole_blocks", 0.1), "no overlap")
    assert res.status_name == "NO_OVERLAP" and res.candidate_blocks == res.blocks_allocated == len(at) > 0 and res.voxels_fused == 0
    for b in at.values():
        assert (b["weight"] == 0).all() and (b["distance"] == 0).all()
    assert ac == {}
    src.close(); dst.close()


# ---- 6. the grid cap
def test_the_grid_cap_changes_no_voxel(hip_lib, tmp_path):
    """NVBX_RESAMPLE_GRID is read when a mapper is created: 1, 7 and the default in a fresh process each, the same maps bit for bit"""
    procs = {}
    for s in ("1", "7", None):
        env = {k: v for k, v in os.environ.items() if k != "NVBX_RESAMPLE_GRID"}
        if s:
            env["NVBX_RESAMPLE_GRID"] = s
        procs[s] = subprocess.Popen([sys.executable, os.path.join(HERE, "resample_grid_child.py"), str(tmp_path / ("g%s.npz" % s))], env=env,
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = {}
    for s, p in procs.items():
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, (s, log[-3000:])
        out[s] = np.load(str(tmp_path / ("g%s.npz" % s)))
    ref = out[None]
    assert int(ref["candidates_a"]) > 7 and int(ref["fused_a"]) > 1000 and int(ref["fused_b"]) > 0      # (a: more blocks than workgroups under both caps)
    for s in ("1", "7"):
        assert sorted(out[s].files) == sorted(ref.files)
        for k in ref.files:
            assert out[s][k].tobytes() == ref[k].tobytes(), (s, k)


# ---- 7. ordering
def _pipelined_pair(room_frames, deferral, sync):
    """src and dst each with a held-back colour frame and ESDF update, the call, then at once another depth frame into src"""
    src = _mapper(1 << 12); dst = _mapper(1 << 12, voxel_size=0.1)
    for m in (src, dst):
        m.set_color_deferral(deferral)
    for d, rgb, T in room_frames[:2]:
        src.integrate_depth(d, T, CAM); src.integrate_color(rgb, T, CAM)
    src.update_esdf()
    for d, rgb, T in room_frames[3:5]:
        dst.integrate_depth(d, T, CAM); dst.integrate_color(rgb, T, CAM)
    dst.update_esdf()
    if sync:
        src.synchronize(); dst.synchronize()
    res = dst.resample_from(src, transform("small", 0.1))
    if sync:
        src.synchronize(); dst.synchronize()
    src.integrate_depth(room_frames[2][0], room_frames[2][2], CAM)
    if sync:
        src.synchronize(); dst.synchronize()
    out = (_state(dst), _state(src), (res.candidate_blocks, res.voxels_fused, res.color_voxels_fused, res.status))
    src.close(); dst.close()
    return out


def test_held_back_work_and_a_following_source_frame(hip_lib, room_frames):
    ref = _pipelined_pair(room_frames, False, True)
    assert ref[2][1] > 1000 and ref[2][2] > 100
    for deferral, sync in ((True, False), (True, True), (False, False)):
        got = _pipelined_pair(room_frames, deferral, sync)
        what = "deferral %r, synchronised %r" % (deferral, sync)
        assert got[2] == ref[2], what
        H.assert_same_map(got[0], ref[0], what + ": dst"); H.assert_same_map(got[1], ref[1], what + ": src")
