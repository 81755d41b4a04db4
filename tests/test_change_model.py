"""The numpy model of change detection (tests/change_independent.py) against restatements that share nothing with it: plain array compares of
two dense volumes (identity, nearest sampling), the shifted array (whole-voxel translations, trilinear sampling), and the analytic room whose
sphere was moved -- fused by the CPU oracle from the same few 80 x 60 frames, under the identity and with the reference map in a frame of its
own -- where every labelled voxel must lie near the sphere it belongs to.  Also: the drawn block sets of the GPU test yield enough voxels of
both labels.  No GPU, no library."""
import numpy as np
import pytest

import change_cases as CC
import change_independent as CI
import merge_independent as MI

F32 = np.float32


def dense_volume(rng, shape, vs, origin=(0, 0, 0), holes=0.3):
    """-> (distance, weight [X, Y, Z] float32, {block: TSDF_DT[512]}) of a dense volume of whole blocks from block `origin`; `holes`: the
    share of voxels with weight 0"""
    d = rng.uniform(-3 * vs, 3 * vs, shape).astype(F32)
    w = rng.choice(np.array([0.5, 2.0], F32), shape)
    if holes:
        w[rng.random(shape) < holes] = F32(0.0)
    blocks = {}
    for bx in range(shape[0] // 8):
        for by in range(shape[1] // 8):
            for bz in range(shape[2] // 8):
                v = np.zeros(512, CI.TSDF_DT)
                sl = (slice(8 * bx, 8 * bx + 8), slice(8 * by, 8 * by + 8), slice(8 * bz, 8 * bz + 8))
                v["distance"] = d[sl].reshape(512); v["weight"] = w[sl].reshape(512)
                blocks[(origin[0] + bx, origin[1] + by, origin[2] + bz)] = v
    return d, w, blocks


def dense_of(per_block, shape, origin, dtype):
    out = np.zeros(shape, dtype)
    for k, v in per_block.items():
        b = np.asarray(k) - np.asarray(origin)
        out[8 * b[0]:8 * b[0] + 8, 8 * b[1]:8 * b[1] + 8, 8 * b[2]:8 * b[2] + 8] = np.asarray(v).reshape(8, 8, 8)
    return out


@pytest.mark.parametrize("vs", [0.0625, 0.05])
@pytest.mark.parametrize("shape,origin", [((16, 8, 24), (0, 0, 0)), ((8, 16, 8), (-2, 3, -1))])
def test_identity_and_nearest_sampling_equal_plain_array_compares(vs, shape, origin):
    rng = np.random.default_rng(3)
    dm, wm, m = dense_volume(rng, shape, vs, origin)
    dr, wr, ref = dense_volume(rng, shape, vs, origin)
    mw, rmw, fd, od = 0.4, 1.0, float(F32(vs)), 0.0
    r = CI.changes(m, ref, np.eye(4, dtype=F32), vs, mw, rmw, None, od, CI.NEAREST)
    obs = wm >= F32(mw); seen = wr >= F32(rmw)
    appeared = obs & (dm <= F32(od)) & seen & (dr > F32(fd))
    removed = obs & (dm > F32(fd)) & seen & (dr <= F32(od))
    want = np.where(appeared, 0, np.where(removed, 1, -1)).astype(np.int32)
    labels = dense_of({k: r["volume"][k][0] if k in r["volume"] else np.full(512, -1, np.int32) for k in m}, shape, origin, np.int32)
    assert np.array_equal(labels, want) and appeared.sum() > 20 and removed.sum() > 20      # (not vacuous on the smaller volume, 1024 voxels, either)
    score = dense_of({k: r["volume"][k][1] if k in r["volume"] else np.zeros(512, F32) for k in m}, shape, origin, F32)
    assert np.array_equal(score, np.where(want >= 0, np.abs(dm - dr), F32(0)).astype(F32))
    assert (r["voxels_compared"], r["voxels_appeared"], r["voxels_removed"]) == (int((obs & seen).sum()), int(appeared.sum()), int(removed.sum()))
    assert r["blocks_scanned"] == len(m) and r["blocks_changed"] == len(r["volume"]) and r["status"] == CI.OK
    assert set(r["volume"]) == {k for k in m if (dense_of({k: np.ones(512, bool)}, shape, origin, bool) & (want >= 0)).any()}


@pytest.mark.parametrize("shift", [(0, 0, 0), (3, 0, 0), (0, -5, 0), (0, 0, 9), (-8, 8, 0), (2, -11, 7)])
def test_whole_voxel_translations_sample_the_shifted_array(shift):
    """voxel size 2^-4: every position and quotient is exact, the fractions are 0, the interpolant is its first corner"""
    vs, shape = 0.0625, (16, 16, 16)
    rng = np.random.default_rng(7)
    dm, wm, m = dense_volume(rng, shape, vs, holes=0)
    dr, wr, ref = dense_volume(rng, shape, vs, holes=0.04)
    s = np.asarray(shift)
    T = MI.pose([0, 0, 1], 0.0, s * vs)                        # p_M = p_R + shift: voxel g of m samples voxel g - shift of ref
    r = CI.changes(m, ref, T, vs, 1e-4, 0.25, None, 0.0, CI.TRILINEAR)
    valid = dense_of(r["valid"], shape, (0, 0, 0), bool); d_ref = dense_of(r["d_ref"], shape, (0, 0, 0), F32)
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1)
    want_valid = np.ones(shape, bool)
    for q in range(8):
        c = g - s + ((q & 1), (q >> 1) & 1, q >> 2)
        inside = np.all((c >= 0) & (c < np.asarray(shape)), axis=-1)
        cc = np.clip(c, 0, np.asarray(shape) - 1)
        want_valid &= inside & (wr[cc[..., 0], cc[..., 1], cc[..., 2]] >= F32(0.25))
    assert np.array_equal(valid, want_valid) and want_valid.sum() > 100
    c = np.clip(g - s, 0, np.asarray(shape) - 1)
    assert np.array_equal(d_ref[want_valid], dr[c[..., 0], c[..., 1], c[..., 2]][want_valid])
    # ... and nearest sampling reads that voxel alone
    rn = CI.changes(m, ref, T, vs, 1e-4, 0.25, None, 0.0, CI.NEAREST)
    inside = np.all((g - s >= 0) & (g - s < np.asarray(shape)), axis=-1)
    near_valid = inside & (wr[c[..., 0], c[..., 1], c[..., 2]] >= F32(0.25))
    assert np.array_equal(dense_of(rn["valid"], shape, (0, 0, 0), bool), near_valid)
    assert rn["voxels_compared"] == int(near_valid.sum()) >= r["voxels_compared"] == int(want_valid.sum())


def test_statuses_box_and_nan():
    vs = 0.05
    rng = np.random.default_rng(1)
    _, _, m = dense_volume(rng, (8, 8, 8), vs)
    I = np.eye(4, dtype=F32)
    assert CI.changes({}, m, I, vs)["status"] == CI.EMPTY_MAP and CI.changes({}, {}, I, vs)["status"] == CI.EMPTY_MAP
    assert CI.changes(m, {}, I, vs)["status"] == CI.EMPTY_REFERENCE
    far = {(40, 0, 0): next(iter(m.values()))}
    r = CI.changes(m, far, I, vs)
    assert r["status"] == CI.NO_OVERLAP and r["voxels_compared"] == 0 and r["blocks_scanned"] == 1 and not r["volume"]
    # a NaN on either side is neither free nor occupied; a box keeps what lies inside
    a = np.zeros(512, CI.TSDF_DT); a["weight"] = 1; a["distance"] = -0.1
    b = np.zeros(512, CI.TSDF_DT); b["weight"] = 1; b["distance"] = 0.2
    r = CI.changes({(0, 0, 0): a}, {(0, 0, 0): b}, I, vs, sampling=CI.NEAREST)
    assert r["voxels_appeared"] == 512 and r["voxels_removed"] == 0
    assert CI.changes({(0, 0, 0): b}, {(0, 0, 0): a}, I, vs, sampling=CI.NEAREST)["voxels_removed"] == 512
    an = a.copy(); an["distance"][:100] = np.nan
    bn = b.copy(); bn["distance"][50:150] = np.nan
    r = CI.changes({(0, 0, 0): an}, {(0, 0, 0): bn}, I, vs, sampling=CI.NEAREST)
    assert r["voxels_appeared"] == 512 - 150 and r["voxels_compared"] == 512 and (r["volume"][(0, 0, 0)][0][:150] == -1).all()
    r = CI.changes({(0, 0, 0): a}, {(0, 0, 0): b}, I, vs, sampling=CI.NEAREST, box_vox=(2, 0, 0, 3, 7, 7))
    assert r["voxels_appeared"] == r["voxels_compared"] == 128 and (r["volume"][(0, 0, 0)][0].reshape(8, 8, 8)[2:4] == 0).all()
    # exactly at the thresholds: d == free_distance is not free, d == occupied_distance is occupied
    e = b.copy(); e["distance"] = F32(vs)
    assert CI.changes({(0, 0, 0): a}, {(0, 0, 0): e}, I, vs, sampling=CI.NEAREST)["voxels_appeared"] == 0
    z = a.copy(); z["distance"] = 0.0
    assert CI.changes({(0, 0, 0): z}, {(0, 0, 0): b}, I, vs, sampling=CI.NEAREST)["voxels_appeared"] == 512


@pytest.mark.parametrize("sampling", [CI.TRILINEAR, CI.NEAREST])
def test_every_drawn_case_yields_both_labels(sampling):
    """what tests/test_gpu_change.py relies on: at least 32 voxels of each label per drawn case, and every sampling path is reached"""
    m, ref = CC.drawn_maps(5)
    assert min(min(k) for k in m) < 0 and len(m) == 8 and len(ref) == 63
    for name, T in CC.drawn_transforms():
        r = CI.changes(m, ref, T, CC.VS, sampling=sampling)
        assert r["voxels_appeared"] >= 32 and r["voxels_removed"] >= 32, (name, r["voxels_appeared"], r["voxels_removed"])
        assert 0 < r["voxels_compared"] < 8 * 512 and r["status"] == CI.OK
    # the sub-voxel shift: base voxels with local index 7 on each axis alone and on all three at once, with valid samples among them
    T = dict(CC.drawn_transforms())["sub-voxel shift"]
    karr = np.array(sorted(m))
    b, _, ok = MI.base_voxels(MI.sample_positions(T, karr, CC.VS), CC.VS)
    valid = np.stack([CI.changes(m, ref, T, CC.VS)["valid"][k] for k in sorted(m)])
    l7 = (b & 7) == 7
    for sel in (l7[..., 0] & ~l7[..., 1] & ~l7[..., 2], ~l7[..., 0] & l7[..., 1] & ~l7[..., 2], ~l7[..., 0] & ~l7[..., 1] & l7[..., 2], l7.all(-1)):
        assert (sel & ok & valid).sum() > 0


@pytest.fixture(scope="module")
def room(oracle_mod):
    """({block: voxels} of the reference room, of the room now, the truncation distance), fused by the CPU oracle from the same frames"""
    out = []
    p = oracle_mod.default_params(**CC.PARAMS)
    for scene in CC.scenes():
        o = oracle_mod.OracleMap(p)
        for d, T in CC.frames(scene):
            o.integrate_depth(d, T, CC.CAM)
        out.append({tuple(int(q) for q in b): np.array(o.get_block(oracle_mod.L_TSDF, b), CI.TSDF_DT).reshape(512) for b in o.block_indices(oracle_mod.L_TSDF)})
    return out[0], out[1], float(p.truncation_distance_vox) * CC.VS


@pytest.mark.parametrize("frame", ["identity", "general"])
def test_the_moved_sphere_is_found_where_it_was_and_where_it_is(room, frame):
    ref, now, trunc = room
    if frame == "identity":
        T = np.eye(4, dtype=F32)
    else:                                                      # the reference map in a frame of its own: p_R = T^-1 p_M, resampled by the merge model
        T = CC.T_GENERAL
        ref = CI.move_blocks(ref, np.linalg.inv(T.astype(np.float64)).astype(F32), CC.VS, trunc)
    r = CI.changes(now, ref, T, CC.VS)
    assert r["status"] == CI.OK and r["voxels_compared"] > 10000
    CC.check_room(r["volume"], trunc, frame)
    comps, _ = CI.clusters(r["volume"], 26, 8)
    labels = sorted(c[0] for c in comps.values())
    assert labels.count(CI.APPEARED) >= 1 and labels.count(CI.REMOVED) >= 1, labels
    assert comps == CI.clusters(r["volume"], 26, 8, scipy=False)[0]
    # the largest component of each label is the sphere's visible shell: its centroid lies inside the sphere it belongs to
    for label, centre in ((CI.APPEARED, CC.NEW_C), (CI.REMOVED, CC.OLD_C)):
        big = max((c for c in comps.values() if c[0] == label), key=lambda c: c[1])
        centroid = (np.asarray(big[4], np.float64) / big[1] + 0.5) * CC.VS
        assert np.linalg.norm(centroid - np.asarray(centre)) < CC.SPHERE_R + CC.margin(trunc), (label, centroid)
