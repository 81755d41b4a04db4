"""Feature merging on the GPU (nvbx_merge_features / Mapper.merge_features_from, nvbx_set_feature_blocks / Mapper.set_feature_blocks; SEMANTICS.md
"Feature merging") against the numpy model of tests/feature_merge_independent.py -- result records, flagged blocks, weights and the fp16 bits
of every channel exactly -- and against the rest of the mapper afterwards.  Maps are drawn through set_blocks + set_feature_blocks: 3 x 3 x 3
blocks straddling the origin with values that are a hash of (block, voxel, channel); frames are rendered in the twin and ordering tests only."""
import numpy as np
import pytest

import feature_merge_independent as FM
import helpers as H

pytestmark = pytest.mark.gpu

VS = 0.05
F32, F16 = np.float32, np.float16
CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
pose = FM.pose

TRANSFORMS = {
    "identity": pose([0, 0, 1], 0.0, [0, 0, 0]),
    "whole_blocks": pose([0, 0, 1], 0.0, np.array([2, -1, 1]) * 8 * VS),
    "sub_voxel": pose([0, 0, 1], 0.0, np.array([0.5, -0.25, 0.125]) * VS),
    "small": pose([1, 2, 3], 1.5, [0.03, 0.0, 0.0]),                # 3 cm / 1.5 degrees about a general axis
    "z90": pose([0, 0, 1], 90.0, [0.11, -0.27, 0.4]),
    "general_45": pose([1, 2, 3], 45.0, [0.37, -0.21, 0.13]),      # where a block reaches 3 x 3 x 3 source blocks
}
SRC_KEYS = [(x, y, z) for x in (-2, -1, 0) for y in (-2, -1, 0) for z in (-1, 0, 1)]      # straddles the origin


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _mapper(C=None, cap=1 << 11, **params):
    M, _ = _mods()
    m = M.Mapper(M.default_params(**params), device=0, block_capacity=cap)
    if C:
        m.enable_features(C)
    return m


def _mix(h):
    h = (h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    h = (h ^ (h >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    return h ^ (h >> np.uint64(15))


def _hash_features(keys, C, seed=0, weights=(0.0, 0.5, 1.0, 2.0, 3.0)):
    """{block: (f [512, C] f16, w [512] f32)}: the value of (block, voxel, channel) is a hash of the three rounded to fp16 in [-4, 4), the
    weight a hash of (block, voxel) into `weights` -- a wrong block, voxel or chunk cannot go unnoticed"""
    out = {}
    v = np.arange(512, dtype=np.uint64)[:, None]; c = np.arange(C, dtype=np.uint64)[None, :]
    for k in keys:
        b = np.uint64(((k[0] + 1024) * 73856093) ^ ((k[1] + 1024) * 19349663) ^ ((k[2] + 1024) * 83492791) ^ (seed * 2654435761)) & np.uint64(0xFFFFFFFF)
        h = _mix(b ^ (v * np.uint64(40503)) ^ (c * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF))
        f = ((h & np.uint64(0xFFFF)).astype(np.float64) * (8.0 / 65536.0) - 4.0).astype(F16)
        hw = _mix(b ^ (v[:, 0] * np.uint64(3266489917)) & np.uint64(0xFFFFFFFF))
        w = np.asarray(weights, F32)[(hw % np.uint64(len(weights))).astype(np.int64)]
        out[tuple(k)] = (f, w)
    return out


def _tsdf_blocks(m, keys):
    """TSDF blocks without features (set_blocks): a plane z = 0.02 m seen with weight 2, so that merge_from has something to fuse everywhere"""
    M, _ = _mods()
    keys = sorted(tuple(k) for k in keys)
    if not keys:
        return
    data = np.zeros((len(keys), 512), M.TSDF_DT)
    for i, k in enumerate(keys):
        z = (8 * k[2] + FM.LANE_XYZ[:, 2] + 0.5) * VS
        data[i]["distance"] = np.clip(z - 0.02, -0.2, 0.2).astype(F32); data[i]["weight"] = 2.0
    m.set_blocks(M.LAYER_TSDF, np.array(keys, np.int32), data)


def _put_features(m, feat):
    keys = sorted(feat)
    return m.set_feature_blocks(np.array(keys, np.int32).reshape(-1, 3), np.stack([feat[k][0] for k in keys]), np.stack([feat[k][1] for k in keys]))


def _source(C, keys=SRC_KEYS, seed=0, without=(), **params):
    """a mapper holding `keys` as TSDF blocks, all but `without` with hashed features"""
    m = _mapper(C, **params)
    _tsdf_blocks(m, keys)
    feat = _hash_features([k for k in keys if k not in without], C, seed)
    assert _put_features(m, feat).all()
    return m, feat


def _layer_counts(m):
    M, _ = _mods()
    return [m.num_blocks(l) for l in (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF, M.LAYER_MESH)]


def _merge_and_check(dst, src, T, what="", **options):
    """the call on the GPU, the model on the layers read before it; everything compared exactly.  -> (model result, GPU result)"""
    M, _ = _mods()
    have = H.idx_set(dst.block_indices(M.LAYER_TSDF))
    dfeat = FM.read_features(dst, M); sfeat = FM.read_features(src, M)
    counts = _layer_counts(dst)
    r = FM.merge_features(have, dfeat, sfeat, T, dst.params.voxel_size, dst.params.max_weight, **{**FM.DEFAULTS, **options})
    res = dst.merge_features_from(src, T, **options)
    got = (res.source_blocks, res.candidate_blocks, res.blocks_flagged, res.voxels_fused, res.status)
    print("%s: model %s, library %s" % (what, (r["source_blocks"], r["candidate_blocks"], r["blocks_flagged"], r["voxels_fused"], r["status"]), got))
    assert got == (r["source_blocks"], r["candidate_blocks"], r["blocks_flagged"], r["voxels_fused"], r["status"]), (what, res)
    after = FM.read_features(dst, M)
    assert set(after) == set(r["feat"]), (what, sorted(set(after) ^ set(r["feat"]))[:5])
    assert set(after) - set(dfeat) == set(r["flagged"]), what
    for k, (f, w) in r["feat"].items():
        gf, gw = after[k]
        bad = gw.view(np.uint32) != w.view(np.uint32)
        assert not bad.any(), "%s: %d weights of block %r differ from the model" % (what, int(bad.sum()), k)
        bad = gf.view(np.uint16) != f.view(np.uint16)
        assert not bad.any(), "%s: %d values of block %r differ from the model (first voxel %d)" % (what, int(bad.sum()), k, int(np.argmax(bad.any(1))))
    assert _layer_counts(dst) == counts and H.idx_set(dst.block_indices(M.LAYER_TSDF)) == have, what      # nothing is allocated
    assert FM.read_features(src, M).keys() == sfeat.keys()
    return r, res


def _positive(feat):
    return int(sum(int((w > 0).sum()) for _, w in feat.values()))


# ---- 1. against the model, in every transform
@pytest.mark.parametrize("name", list(TRANSFORMS))
@pytest.mark.parametrize("C", [8, 40])
def test_merge_equals_the_model(hip_lib, C, name):
    """dst prepared by merge_from with the same pose, one extra block far away; the centre block of src has TSDF but no features"""
    T = TRANSFORMS[name]
    src, sfeat = _source(C, without=[(-1, -1, 0)])
    dst = _mapper(C)
    dst.merge_from(src, T)
    _tsdf_blocks(dst, [(40, 40, 40)])
    r, res = _merge_and_check(dst, src, T, "C %d %s" % (C, name))
    assert res.status_name == "OK" and r["source_blocks"] == 26
    assert 2 * r["voxels_fused"] >= _positive(sfeat)                 # not a vacuous pass
    assert (40, 40, 40) not in r["feat"]                             # a block no source voxel reaches is not flagged
    assert any(not p.all() for p in r["fused"].values())             # first touch: voxels nothing contributed to, written as zeros
    if name == "general_45":
        assert int(FM.reach(T, np.array(r["candidates"]), VS).prod(1).max()) == 27
    # again, now into blocks that carry features: blended, scaled, clamped at max_weight
    r2, _ = _merge_and_check(dst, src, T, "C %d %s, blended" % (C, name), weight_scale=4.0, min_weight=0.75)
    assert r2["blocks_flagged"] == 0 and 0 < r2["voxels_fused"] < r["voxels_fused"]      # min_weight above some weights
    assert any((w == F32(dst.params.max_weight)).any() for _, w in r2["feat"].values())
    r3, _ = _merge_and_check(dst, src, T, "C %d %s, half" % (C, name), weight_scale=0.5)
    assert r3["voxels_fused"] == r["voxels_fused"]
    # a dst that lacks every other candidate: those are skipped, not allocated (_merge_and_check compares the block counts of every layer)
    cands = sorted(FM.candidates(T, sorted(sfeat), VS))
    half = _mapper(C)
    _tsdf_blocks(half, cands[::2])
    rh, _ = _merge_and_check(half, src, T, "C %d %s, every other candidate" % (C, name))
    assert rh["candidate_blocks"] == len(cands[::2]) < len(cands) and rh["voxels_fused"] > 0
    src.close(); dst.close(); half.close()


def test_merge_equals_the_model_at_256_channels(hip_lib):
    T = TRANSFORMS["general_45"]
    keys = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    src, sfeat = _source(256, keys=keys, cap=1 << 9)
    dst = _mapper(256, cap=1 << 9)
    dst.merge_from(src, T)
    r, _ = _merge_and_check(dst, src, T, "C 256")
    assert 2 * r["voxels_fused"] >= _positive(sfeat)
    _merge_and_check(dst, src, T, "C 256, blended", weight_scale=0.5)
    src.close(); dst.close()


def test_empty_source_and_no_overlap(hip_lib):
    M, _ = _mods()
    src = _mapper(8); dst = _mapper(8)
    _tsdf_blocks(dst, SRC_KEYS[:4])
    _tsdf_blocks(src, SRC_KEYS[:4])                                  # TSDF, no feature block
    r, res = _merge_and_check(dst, src, TRANSFORMS["identity"], "empty source")
    assert res.status_name == "EMPTY_SOURCE" and res.candidate_blocks == 0
    assert _put_features(src, _hash_features(SRC_KEYS[:4], 8)).all()
    r, res = _merge_and_check(dst, src, pose([0, 0, 1], 0.0, [30.0, 0, 0]), "far away")
    assert res.status_name == "NO_OVERLAP" and res.candidate_blocks == 0 and dst.num_blocks(M.LAYER_FEATURE) == 0
    r, res = _merge_and_check(dst, src, TRANSFORMS["identity"], "min_weight above all", min_weight=10.0)
    assert res.status_name == "NO_OVERLAP" and res.candidate_blocks == 4 and dst.num_blocks(M.LAYER_FEATURE) == 0
    assert dst.merge_features_from(src).status_name == "OK"          # None: the identity
    src.close(); dst.close()


# ---- 2. slot reuse: a stale payload behind a cleared flag is never read, on either side
def test_a_stale_payload_is_never_read(hip_lib):
    M, _ = _mods()
    C = 16
    T = TRANSFORMS["sub_voxel"]
    src, _ = _source(C, seed=1)
    dst, _ = _source(C, seed=2)
    # src: cleared, the same blocks again without features, then features in a few
    src.clear()
    _tsdf_blocks(src, SRC_KEYS)
    assert src.num_blocks(M.LAYER_FEATURE) == 0
    few = _hash_features(SRC_KEYS[5:9], C, seed=3)
    assert _put_features(src, few).all()
    # dst: everything outside a small radius far away goes, the same blocks again without features
    dst.clear_outside_radius([100.0, 100.0, 100.0], 0.5)
    assert dst.num_blocks(M.LAYER_TSDF) == 0
    _tsdf_blocks(dst, SRC_KEYS)
    assert dst.num_blocks(M.LAYER_FEATURE) == 0
    r, res = _merge_and_check(dst, src, T, "reused slots")
    assert res.source_blocks == 4 and 0 < res.blocks_flagged < 27 and res.voxels_fused > 0
    src.close(); dst.close()


# ---- 3. the writer
def test_set_feature_blocks_round_trip(hip_lib):
    M, _ = _mods()
    C = 24
    m = _mapper(C)
    _tsdf_blocks(m, SRC_KEYS[:10])
    keys = SRC_KEYS[:10] + [(50, 0, 0), (-50, 3, 1)]                # the last two: no TSDF block
    feat = _hash_features(keys, C, seed=4)
    before = H.map_state(m, (M.LAYER_TSDF,)), m.counters(), m.last_view()
    written = _put_features(m, feat)
    order = sorted(feat)
    assert [bool(w) for w in written] == [k in SRC_KEYS[:10] for k in order]
    f, w, found = m.feature_blocks(np.array(order, np.int32))
    assert np.array_equal(found, written)
    for i, k in enumerate(order):
        if written[i]:
            assert np.array_equal(f[i].view(np.uint16), feat[k][0].view(np.uint16)) and np.array_equal(w[i].view(np.uint32), feat[k][1].view(np.uint32))
        else:
            assert not f[i].any() and not w[i].any()
    assert H.idx_set(m.block_indices(M.LAYER_FEATURE)) == set(SRC_KEYS[:10]) and m.num_blocks(M.LAYER_TSDF) == 10
    H.assert_same_map(before[0], m, "set_feature_blocks touches the two feature pools and the flag only")
    assert before[1] == m.counters() and np.array_equal(before[2], m.last_view())
    # a second write replaces all 512 voxels
    again = _hash_features(SRC_KEYS[:1], C, seed=5)
    assert _put_features(m, again).all()
    f, w, _ = m.feature_blocks(np.array(SRC_KEYS[:1], np.int32))
    assert np.array_equal(f[0].view(np.uint16), again[SRC_KEYS[0]][0].view(np.uint16)) and np.array_equal(w[0], again[SRC_KEYS[0]][1])
    m.close()


def test_refusals(hip_lib):
    M, _ = _mods()
    a, feat = _source(8, keys=SRC_KEYS[:2]); b = _mapper(8); c16 = _mapper(16); plain = _mapper(); coarse = _mapper(8, voxel_size=0.1)
    _tsdf_blocks(b, SRC_KEYS[:2])
    T = TRANSFORMS["identity"]

    def refused(fn, text):
        with pytest.raises(M.NvbxError) as e:
            fn()
        assert text in str(e.value), str(e.value)
    refused(lambda: b.merge_features_from(plain, T), "nvbx_merge_features: both mappers need the feature layer")
    refused(lambda: plain.merge_features_from(a, T), "nvbx_merge_features: both mappers need the feature layer")
    refused(lambda: c16.merge_features_from(a, T), "nvbx_merge_features: the mappers' feature channel counts differ")
    refused(lambda: coarse.merge_features_from(a, T), "nvbx_merge_features: the mappers' voxel sizes differ")
    refused(lambda: b.merge_features_from(b, T), "nvbx_merge_features: src and dst are the same mapper")
    refused(lambda: b.merge_features_from(a, T, min_weight=-1.0), "nvbx_merge_features: min_weight is negative")
    refused(lambda: b.merge_features_from(a, T, min_weight=float("nan")), "nvbx_merge_features: min_weight is not a number")
    refused(lambda: b.merge_features_from(a, T, weight_scale=0.0), "nvbx_merge_features: weight_scale")
    bad = np.eye(4, dtype=F32); bad[0, 0] = 1.01
    refused(lambda: b.merge_features_from(a, bad), "nvbx_merge_features: the upper-left 3 x 3")
    with pytest.raises(TypeError):
        b.merge_features_from(a, T, merge_color=1)
    assert b.num_blocks(M.LAYER_FEATURE) == 0                        # dst unchanged
    k = np.array(SRC_KEYS[:1], np.int32); f = np.zeros((1, 512, 8), F16); w = np.ones((1, 512), F32)
    refused(lambda: plain.set_feature_blocks(k, f, w), "nvbx_set_feature_blocks: call nvbx_enable_features first")
    for v in (-1.0, float("nan")):
        w2 = w.copy(); w2[0, 77] = v
        refused(lambda: b.set_feature_blocks(k, f, w2), "nvbx_set_feature_blocks: a weight is negative or not a number")
    assert b.num_blocks(M.LAYER_FEATURE) == 0
    assert len(b.set_feature_blocks(np.zeros((0, 3), np.int32), np.zeros((0, 512, 8), F16), np.zeros((0, 512), F32))) == 0
    for m in (a, b, c16, plain, coarse):
        m.close()


# ---- 4. the rest of both maps
@pytest.fixture(scope="module")
def room_frames():
    _, S = _mods()
    sc = S.Scene()
    out = []
    for i in (0, 9, 4):
        T = S.trajectory_pose(i)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


def _room(frames, C, esdf=True):
    M, _ = _mods()
    m = _mapper(C, cap=1 << 12)
    for d, rgb, T in frames:
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM)
    if esdf:
        m.update_esdf(); m.update_color_mesh()
    return m


def test_only_the_feature_layer_of_dst_changes_and_src_does_not(hip_lib, room_frames):
    import torch
    M, _ = _mods()
    C = 16
    src = _room(room_frames[:2], C); dst = _room(room_frames[1:], C)
    keys = [tuple(k) for k in src.block_indices(M.LAYER_TSDF).tolist()]
    assert _put_features(src, _hash_features(keys, C, seed=7, weights=(0.0, 1.0, 2.0))).all()
    dkeys = [tuple(k) for k in dst.block_indices(M.LAYER_TSDF).tolist()][::3]
    assert _put_features(dst, _hash_features(dkeys, C, seed=8, weights=(1.0,))).all()
    dst.integrate_depth(room_frames[0][0], room_frames[0][2], CAM)      # dirty lists and a view list that are not empty

    def rest(m):
        idx = torch.full((m.capacity, 3), -1, dtype=torch.int32, device="cuda:0"); cnt = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        m.esdf_dirty_list(idx, cnt); m.synchronize()
        n = int(cnt.item())
        return (sorted(map(tuple, idx[:n].cpu().numpy().tolist())), sorted(map(tuple, m.last_view().tolist())), m.counters(),
                sorted(map(tuple, m.block_indices(M.LAYER_MESH).tolist())))
    layers = (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF)
    d_before = H.map_state(dst, layers, slice=True, mesh=True), rest(dst)
    s_before = H.map_state(src, layers + (M.LAYER_FEATURE,), slice=True, mesh=True), rest(src)
    assert len(d_before[1][0]) > 0 and len(d_before[1][1]) > 0
    r, res = _merge_and_check(dst, src, TRANSFORMS["small"], "room")
    assert res.status_name == "OK" and res.blocks_flagged > 0 and res.blocks_flagged < res.candidate_blocks
    H.assert_same_map(d_before[0], dst, "dst but for its features", min_blocks={M.LAYER_TSDF: 101, M.LAYER_COLOR: 51, M.LAYER_ESDF: 5})
    assert rest(dst) == d_before[1]
    H.assert_same_map(s_before[0], src, "src", min_blocks={M.LAYER_FEATURE: 101})
    assert rest(src) == s_before[1]
    src.close(); dst.close()


# ---- 5. downstream
def test_the_readers_answer_on_the_merged_map_as_on_the_source(hip_lib, room_frames):
    M, _ = _mods()
    C = 16
    src = _room(room_frames[:2], C, esdf=False)
    keys = [tuple(k) for k in src.block_indices(M.LAYER_TSDF).tolist()]
    feat = _hash_features(keys, C, seed=9, weights=(0.0, 1.0, 2.0))
    for f, w in feat.values():
        f[w == 0] = 0                                                # as integration leaves a voxel it never reached (the merge writes such voxels as zeros)
    assert _put_features(src, feat).all()
    dst = _mapper(C, cap=1 << 12)
    dst.merge_from(src, TRANSFORMS["identity"])
    res = dst.merge_features_from(src)
    assert res.status_name == "OK" and res.blocks_flagged == len(keys) == res.source_blocks
    fs, fd = FM.read_features(src, M), FM.read_features(dst, M)
    assert fs.keys() == fd.keys() and all(fs[k][0].tobytes() == fd[k][0].tobytes() and fs[k][1].tobytes() == fd[k][1].tobytes() for k in fs)
    rng = np.random.default_rng(12)
    q = rng.standard_normal((5, C)).astype(F16)

    def by_block(idx, *arrays):
        idx = idx.cpu().numpy()
        return {tuple(int(v) for v in b): tuple(a[i].cpu().numpy().tobytes() for a in arrays) for i, b in enumerate(idx)}
    a = src.match_features(q, "cosine", 1.0); b = dst.match_features(q, "cosine", 1.0)
    ma, mb = by_block(a[0], a[1], a[2]), by_block(b[0], b[1], b[2])
    assert len(ma) == len(keys) and ma == mb
    pts = rng.uniform(-3, 3, (2000, 3)).astype(F32)
    fa, wa = src.query_features(pts); fb, wb = dst.query_features(pts)
    assert (wa > 0).sum() > 20 and np.array_equal(wa.cpu().numpy(), wb.cpu().numpy())
    assert np.array_equal(fa.cpu().numpy().view(np.uint16), fb.cpu().numpy().view(np.uint16))
    sa = src.segment_features(q, "cosine", 1.0, min_score=0.2); sb = dst.segment_features(q, "cosine", 1.0, min_score=0.2)
    assert by_block(sa[0], sa[1], sa[2]) == by_block(sb[0], sb[1], sb[2])

    def comps(c):
        return sorted(zip(c.label.cpu().tolist(), c.voxels.cpu().tolist(), map(tuple, c.min_xyz.cpu().tolist()), map(tuple, c.max_xyz.cpu().tolist()),
                          map(tuple, c.sum_xyz.cpu().tolist())))
    assert len(comps(sa[4])) > 0 and comps(sa[4]) == comps(sb[4])
    src.close(); dst.close()


def _feature_image(rng, C):
    return rng.standard_normal((CAM[5] // 4, CAM[4] // 4, C)).astype(F16)


def test_two_merged_single_frame_mappers_against_one_that_integrated_both(hip_lib, room_frames):
    """weights add, so they equal the twin's; the values are the model's (the blend of a blend is not the twin's, bit for bit)"""
    M, _ = _mods()
    C = 8
    rng = np.random.default_rng(14)
    feats = [_feature_image(rng, C) for _ in range(2)]
    twin = _room(room_frames[:2], C, esdf=False)
    singles = [_room(room_frames[:2], C, esdf=False) for _ in range(2)]
    for k in range(2):
        twin.integrate_features(feats[k], room_frames[k][2], CAM, 4)
        singles[k].integrate_features(feats[k], room_frames[k][2], CAM, 4)
    dst = _room(room_frames[:2], C, esdf=False)
    for k in range(2):
        r, res = _merge_and_check(dst, singles[k], TRANSFORMS["identity"], "single %d" % k)
        assert res.status_name == "OK" and res.voxels_fused > 1000
    ft, fd = FM.read_features(twin, M), FM.read_features(dst, M)
    assert set(ft) == set(fd) and len(ft) > 20
    assert all(np.array_equal(ft[k][1].view(np.uint32), fd[k][1].view(np.uint32)) for k in ft)
    assert any((ft[k][1] == 2).any() for k in ft)
    for m in [twin, dst] + singles:
        m.close()


# ---- 6. ordering
def test_the_call_runs_behind_work_enqueued_on_src(hip_lib, room_frames):
    """issued right after a feature frame enqueued on src's stream, without a synchronize: as after one"""
    M, _ = _mods()
    C = 8
    feat = _feature_image(np.random.default_rng(15), C)
    results = []
    for wait in (True, False):
        src = _room(room_frames[:2], C, esdf=False); dst = _room(room_frames[:2], C, esdf=False)
        src.synchronize(); dst.synchronize()
        src.integrate_features(feat, room_frames[0][2], CAM, 4)
        if wait:
            src.synchronize()
        res = dst.merge_features_from(src, TRANSFORMS["small"])
        # work enqueued on src afterwards runs behind the call's reads: src is cleared at once
        src.clear()
        results.append((FM.read_features(dst, M), (res.source_blocks, res.candidate_blocks, res.blocks_flagged, res.voxels_fused, res.status)))
        src.close(); dst.close()
    (fa, ra), (fb, rb) = results
    assert ra == rb and ra[3] > 1000 and fa.keys() == fb.keys()
    assert all(fa[k][0].tobytes() == fb[k][0].tobytes() and fa[k][1].tobytes() == fb[k][1].tobytes() for k in fa)
