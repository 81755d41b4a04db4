"""Frontiers and view gain on the GPU (nvbx_find_frontiers / nvbx_frontier_clusters / nvbx_view_gain; SEMANTICS.md "Frontiers and view gain")
against the numpy model of tests/frontier_independent.py: entry sets as sets, label and score volumes bit for bit, records as sets of tuples.
Maps are hand-built with set_blocks or come from two 80 x 60 frames of the synthetic room; block_capacity at most 1 << 12."""
import ctypes as C

import numpy as np
import pytest

import frontier_independent as FI
import helpers as H
import segment_independent as SI

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05
F32 = np.float32
MIN_W = 1e-4
SENTINEL = -77
E_INVALID = -1


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


def _mapper(cap=1 << 12, **params):
    M, _ = _mods()
    return M.Mapper(M.default_params(**params), device=0, block_capacity=cap)


def _block(distance=0.2, weight=1.0):
    v = np.zeros(512, FI.TSDF_DT)
    v["distance"] = distance; v["weight"] = weight
    return v


def _upload(m, tsdf):
    M, _ = _mods()
    ks = sorted(tsdf)
    m.set_blocks(M.LAYER_TSDF, np.array(ks, np.int32), np.stack([tsdf[k] for k in ks]))


def _as_dict(idx, lab, sc):
    idx = idx.cpu().numpy(); lab = lab.cpu().numpy(); sc = sc.cpu().numpy()
    out = {tuple(int(q) for q in b): (lab[i], sc[i]) for i, b in enumerate(idx)}
    assert len(out) == len(idx), "a block appears in two entries"
    return out


def _same(got, want, what=""):
    assert set(got) == set(want), (what, sorted(set(got) ^ set(want))[:8])
    for k in want:
        assert got[k][0].dtype == np.int32 and got[k][1].dtype == np.float32
        assert np.array_equal(got[k][0], want[k][0]), "%s: labels of block %r differ" % (what, k)
        assert got[k][1].tobytes() == want[k][1].tobytes(), "%s: scores of block %r differ" % (what, k)


def _check(m, what="", min_weight=MIN_W, free_distance_m=None, min_unknown=1, box_m=None):
    """find_frontiers on the GPU, the model on the layer read back: compared exactly.  -> the model's result"""
    M, _ = _mods()
    fd = VS if free_distance_m is None else free_distance_m
    want = FI.frontiers(FI.read_tsdf(m, M), min_weight, fd, min_unknown, None if box_m is None else FI.box_from_metres(box_m, VS))
    idx, lab, sc, cnt = m.find_frontiers(min_weight=min_weight, free_distance_m=free_distance_m, min_unknown=min_unknown, box_m=box_m)
    assert int(cnt.item()) == len(want) == len(idx), (what, int(cnt.item()), len(want))
    _same(_as_dict(idx, lab, sc), want, what)
    return want


# ---- 1. one block alone in the void
def test_one_free_block_alone(hip_lib):
    m = _mapper()
    b = (-3, 2, 5)
    _upload(m, {b: _block()})
    fr = _check(m, "alone")
    lab, sc = fr[b]
    assert (lab == 0).sum() == 296                                           # 512 - 6^3: the surface
    assert ((sc == 3).sum(), (sc == 2).sum(), (sc == 1).sum(), (sc == 0).sum()) == (8, 72, 216, 216)
    on_border = ((FI.OFF == 0) | (FI.OFF == 7)).sum(1)
    assert np.array_equal(sc, on_border.astype(F32))                         # corners 3, edges 2, faces 1
    # min_unknown 1, 2, 3, 6
    for k, n in ((1, 296), (2, 80), (3, 8), (6, 0)):
        fr = _check(m, "min_unknown %d" % k, min_unknown=k)
        assert sum(int((v[0] == 0).sum()) for v in fr.values()) == n
    m.close()


# ---- 2. block pairs: the halo's face addressing
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [-1, 1])
def test_block_pairs(hip_lib, axis, sign):
    base = (-1, 0, -2)
    nb = tuple(base[k] + (sign if k == axis else 0) for k in range(3))
    face = FI.OFF[:, axis] == (7 if sign > 0 else 0)                         # the base block's voxels that face the neighbour
    rng = np.random.default_rng(10 * axis + sign + 1)
    holes = _block(); holes["weight"] = rng.choice(np.array([0.0, 1.0], F32), 512)
    holes_base = _block(); holes_base["weight"] = rng.choice(np.array([0.0, 1.0], F32), 512)
    for case, other in (("free", _block()), ("weight_0", _block(0.2, 0.0)), ("occupied", _block(-0.02, 1.0)), ("holes", holes)):
        m = _mapper(cap=64)
        _upload(m, {base: holes_base if case == "holes" else _block(), nb: other})
        fr = _check(m, "%s axis %d sign %d" % (case, axis, sign))
        if case == "holes":
            m.close()
            continue
        lab, sc = fr[base]
        inner_face = face & (((FI.OFF == 0) | (FI.OFF == 7)).sum(1) == 1)       # the 36 voxels of the face that touch nothing else
        if case == "weight_0":                                               # allocated, never observed: unknown, the faces are frontier again
            assert (lab[inner_face] == 0).all() and (sc[inner_face] == 1).all() and (lab == 0).sum() == 296 and nb not in fr
        else:                                                                # free or occupied: known, the facing faces stop being frontier
            assert (lab[inner_face] == -1).all() and (lab == 0).sum() == 296 - 36
            assert (nb in fr) == (case == "free")
        m.close()


# ---- 3. the box
def test_box_cuts_the_block(hip_lib):
    m = _mapper(cap=64)
    _upload(m, {(0, 0, 0): _block(), (1, 0, 0): _block()})
    n_all = sum(int((v[0] == 0).sum()) for v in _check(m, "no box").values())
    cut = _check(m, "interior plane", box_m=((-1.0, -1.0, -1.0), (0.19, 1.0, 1.0)))          # x <= 3
    assert set(cut) == {(0, 0, 0)} and (cut[(0, 0, 0)][0].reshape(8, 8, 8)[4:] == -1).all() and (cut[(0, 0, 0)][0] == 0).sum() == 4 * 64 - 3 * 36
    border = _check(m, "block border", box_m=((0.0, 0.0, 0.0), (0.39, 0.39, 0.39)))           # exactly block (0, 0, 0)
    assert set(border) == {(0, 0, 0)} and (border[(0, 0, 0)][0] == 0).sum() == n_all // 2
    one = _check(m, "one voxel", box_m=((0.41, 0.01, 0.36), (0.41, 0.01, 0.36)))               # voxel (8, 0, 7): a corner of block (1, 0, 0) ...
    assert set(one) == {(1, 0, 0)} and (one[(1, 0, 0)][0] == 0).sum() == 1 and one[(1, 0, 0)][1].max() == 2      # ... on the face shared with (0, 0, 0)
    assert not _check(m, "outside", box_m=((2.0, 2.0, 2.0), (3.0, 3.0, 3.0)))
    m.close()


# ---- 4. the two thresholds, exactly at a stored value
def test_free_distance_and_min_weight_at_a_stored_value(hip_lib):
    m = _mapper(cap=64)
    d = float(F32(0.1)); w = float(F32(0.3))
    v = _block(d, w)
    v["distance"][:64] = np.nextafter(F32(0.1), F32(1.0))                     # the slab x = 0: one ulp above
    _upload(m, {(0, 0, 0): v})
    fr = _check(m, "d == free_distance", min_weight=MIN_W, free_distance_m=d)              # strict >: only the slab is free
    assert (fr[(0, 0, 0)][0] == 0).sum() == 64
    fr = _check(m, "below", min_weight=MIN_W, free_distance_m=float(np.nextafter(F32(0.1), F32(0.0))))
    assert (fr[(0, 0, 0)][0] == 0).sum() == 296
    fr = _check(m, "w == min_weight", min_weight=w, free_distance_m=0.0)                    # >=: observed
    assert (fr[(0, 0, 0)][0] == 0).sum() == 296
    assert not _check(m, "w < min_weight", min_weight=float(np.nextafter(F32(0.3), F32(1.0))), free_distance_m=0.0)
    m.close()


# ---- 5. capacity, count-only call, empty map
def test_capacity_and_count_only(hip_lib):
    import torch
    m = _mapper(cap=64)
    empty_cnt = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    z = lambda *s, dt=torch.int32: torch.empty(s, dtype=dt, device="cuda")      # noqa: E731
    m.find_frontiers(out=(z(0, 3), z(0, 512), z(0, 512, dt=torch.float32), empty_cnt))
    assert int(empty_cnt.item()) == 0                                         # an empty map writes a count of 0
    keys = [(2 * i, -i, 1) for i in range(5)]
    _upload(m, {k: _block() for k in keys})
    want = _check(m, "five blocks")
    assert len(want) == 5
    # count only: capacity 0, NULL arrays
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.find_frontiers(out=(z(0, 3), z(0, 512), None, cnt))
    assert int(cnt.item()) == 5
    # capacity 2: the count in full, two valid entries, nothing behind them
    idx = torch.full((4, 3), SENTINEL, dtype=torch.int32, device="cuda")
    lab = torch.full((4, 512), SENTINEL, dtype=torch.int32, device="cuda")
    sc = torch.full((4, 512), float(SENTINEL), dtype=torch.float32, device="cuda")
    m.find_frontiers(out=(idx[:2], lab[:2], sc[:2], cnt))
    assert int(cnt.item()) == 5
    got = _as_dict(idx[:2], lab[:2], sc[:2])
    assert len(got) == 2 and set(got) <= set(want)
    _same(got, {k: want[k] for k in got}, "capacity 2")
    assert (idx[2:] == SENTINEL).all() and (lab[2:] == SENTINEL).all() and (sc[2:] == float(SENTINEL)).all()
    # the clusters call under the same capacity: the labelling reads min(count, capacity) entries
    ids = torch.full((4, 512), SENTINEL, dtype=torch.int32, device="cuda")
    rec = m.component_records(8); bcnt = torch.zeros(1, dtype=torch.int64, device="cuda"); ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.frontier_clusters(connectivity=6, out=(idx[:2], lab[:2], sc[:2], ids[:2], bcnt, rec, ccnt))
    assert int(bcnt.item()) == 5 and int(ccnt.item()) == 2 and (ids[2:] == SENTINEL).all() and (lab[2:] == SENTINEL).all()
    m.close()


# ---- 6. the room
@pytest.fixture(scope="module")
def room(hip_lib):
    M, S = _mods()
    m = _mapper()
    sc = S.Scene()
    for i in (0, 9):
        T = S.trajectory_pose(i)
        d, _ = S.render(sc, T, CAM, color=False)
        m.integrate_depth(d, T, CAM)
    m.synchronize()
    tsdf = FI.read_tsdf(m, M)
    yield m, tsdf
    m.close()


def _records(rec):
    return rec.cpu().numpy().view(SI.COMPONENT_DT).reshape(-1)


def _clusters_raw(m, conn, mv, **kw):
    """frontier_clusters into preallocated buffers -> numpy (idx, lab, sc, ids, records, count), trimmed to the block count"""
    import torch
    M, _ = _mods()
    cap = m.num_blocks(M.LAYER_TSDF)
    idx = torch.empty((cap, 3), dtype=torch.int32, device="cuda"); lab = torch.empty((cap, 512), dtype=torch.int32, device="cuda")
    sc = torch.empty((cap, 512), dtype=torch.float32, device="cuda"); ids = torch.empty((cap, 512), dtype=torch.int32, device="cuda")
    rec = m.component_records(cap * 512 // mv)
    bcnt = torch.zeros(1, dtype=torch.int64, device="cuda"); ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.frontier_clusters(connectivity=conn, min_voxels=mv, out=(idx, lab, sc, ids, bcnt, rec, ccnt), **kw)
    nb, nc = int(bcnt.item()), int(ccnt.item())
    assert nb <= cap and nc <= len(rec)
    return idx[:nb].cpu().numpy(), lab[:nb].cpu().numpy(), sc[:nb].cpu().numpy(), ids[:nb].cpu().numpy(), _records(rec)[:nc], nc


def test_room_frontiers_equal_the_model(room):
    m, tsdf = room
    want = _check(m, "room")
    assert len(want) > 50 and sum(int((v[0] == 0).sum()) for v in want.values()) > 2000
    assert len(_check(m, "room, two unknown neighbours, a box", min_unknown=2, box_m=((-1.0, -2.0, 0.0), (2.5, 1.0, 1.6)))) > 5


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("mv", [1, 5])
def test_room_clusters_equal_the_model(room, conn, mv):
    m, tsdf = room
    want = FI.frontiers(tsdf, MIN_W, VS, 1)
    exp_c, exp_k = FI.clusters(want, conn, mv)
    idx, lab, sc, ids, recs, count = _clusters_raw(m, conn, mv)
    _same({tuple(int(q) for q in b): (lab[i], sc[i]) for i, b in enumerate(idx)}, want, "clusters' volume")
    assert count == len(exp_c) > 0
    got_c, got_k = SI.canonical(idx, lab, ids, recs, count)
    order = {tuple(b): i for i, b in enumerate(idx.tolist())}
    perm = [order[k] for k in sorted(want)]                                   # the model's keys are in sorted block order
    # (keys are linear indices in the bounding box of the listed blocks: the same box for both lists)
    assert np.array_equal(got_k[perm], exp_k), "the partition differs at %d voxels" % int((got_k[perm] != exp_k).sum())
    assert got_c == exp_c
    # the wrapper's trimmed form
    i2, l2, s2, ids2, comps = m.frontier_clusters(connectivity=conn, min_voxels=mv)
    assert len(comps.voxels) == count and sorted(comps.voxels.cpu().tolist()) == sorted(c[1] for c in exp_c.values())
    cm = comps.centroid_m.cpu().numpy()
    assert cm.shape == (count, 3) and np.isfinite(cm).all()


def test_clusters_equal_find_then_label(room):
    m, _ = room
    idx, lab, sc, ids, recs, count = _clusters_raw(m, 26, 3, min_unknown=2)
    fi, fl, fs, fc = m.find_frontiers(min_unknown=2)
    ids2, comps = m.label_components(fi, fl, fs, connectivity=26, min_voxels=3)
    recs2 = np.zeros(len(comps.voxels), SI.COMPONENT_DT)
    for f in SI.COMPONENT_DT.names:
        recs2[f] = getattr(comps, f).cpu().numpy()
    a_c, a_k = SI.canonical(idx, lab, ids, recs, count)
    b_c, b_k = SI.canonical(fi.cpu().numpy(), fl.cpu().numpy(), ids2.cpu().numpy(), recs2, len(recs2))
    assert count == len(recs2) > 0 and a_c == b_c
    oa = np.lexsort(idx.T[::-1]); ob = np.lexsort(fi.cpu().numpy().T[::-1])
    assert np.array_equal(idx[oa], fi.cpu().numpy()[ob]) and np.array_equal(a_k[oa], b_k[ob])


# ---- 7. view gain
def test_view_gain_equals_the_model(room):
    M, S = _mods()
    m, tsdf = room
    poses = [S.trajectory_pose(i) for i in (0, 9, 40)] + [S.look_pose((0.3, -0.2, 1.2), 2.0, 0.4)]
    bad = poses[0].copy(); bad[2, 2] = np.inf
    far = poses[1].copy(); far[0, 3] = 4.2e5
    poses = np.stack(poses + [bad, far]).astype(F32)
    got = m.view_gain(poses, CAM, subsampling=4, max_range_m=4.0).cpu().numpy()
    want = FI.view_gain(tsdf, poses, CAM, 4, 4.0, VS, MIN_W, VS)
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), (got.tolist(), want.tolist())
    assert (got[:4, 0] == 300).all() and (got[:4, 1] > 0).all() and (got[:2, 2] > 0).all() and (got[:2, 3] > 0).all()
    assert got[4:].tolist() == [[-1, 0, 0, 0], [-1, 0, 0, 0]]                # never an error
    # other thresholds and the default subsampling / range (the mapper's sphere_tracing_* parameters)
    got = m.view_gain(poses[:2], CAM, min_weight=2.0, free_distance_m=0.1).cpu().numpy()
    p = m.params
    want = FI.view_gain(tsdf, poses[:2], CAM, max(1, p.sphere_tracing_subsampling), p.sphere_tracing_max_ray_length_m, VS, 2.0, 0.1)
    assert got.tolist() == want.tolist()
    assert m.view_gain(np.zeros((0, 4, 4), F32), CAM).shape == (0, 4)


def test_view_gain_wall_and_empty_map(hip_lib):
    M, S = _mods()
    # a wall 0.5 m ahead: free space in front of it, every ray ends on it
    m = _mapper(cap=256)
    tsdf = {}
    for bx in range(0, 2):
        for by in range(-2, 2):
            for bz in range(-2, 2):
                v = _block()
                v["distance"] = np.where(8 * bx + FI.OFF[:, 0] >= 10, -0.02, 0.2).astype(F32)
                tsdf[(bx, by, bz)] = v
    _upload(m, tsdf)
    T = np.eye(4, dtype=F32)
    T[:3, 0] = (0, -1, 0); T[:3, 1] = (0, 0, -1); T[:3, 2] = (1, 0, 0); T[:3, 3] = (0.01, 0.012, 0.013)      # looks along +x
    got = m.view_gain(T[None], CAM, subsampling=4, max_range_m=3.0).cpu().numpy()
    assert got.tolist() == FI.view_gain(tsdf, T[None], CAM, 4, 3.0, VS, MIN_W, VS).tolist()
    assert got[0, 0] == 300 and got[0, 3] == got[0, 0] and got[0, 1] == 0 and got[0, 2] >= 10 * 300
    m.close()
    # an empty mapper: every sample is unknown, t_k < 1.0 for k = 0 .. 19
    e = _mapper(cap=64)
    got = e.view_gain(T[None], CAM, subsampling=4, max_range_m=1.0).cpu().numpy()
    assert got.tolist() == [[300, 300 * 20, 0, 0]]
    e.close()


# ---- 8. nothing is written to the map, held-back work stays held back
def test_map_unchanged_and_held_back_work_stays_held_back(hip_lib):
    """Two mappers with colour deferral on get the same frames; one of them runs the three calls between pipelined frames.  Its map is byte for
    byte the other's and, apart from the calls' own kernels, it has launched exactly the same kernels as often: the held-back colour frame and
    ESDF update were still carried by the next depth frame's fused launches."""
    M, S = _mods()
    sc = S.Scene()
    frames = []
    for i in range(6):
        T = S.trajectory_pose(3 * i)
        d, rgb = S.render(sc, T, CAM)
        frames.append((d, rgb, T))
    A = _mapper(); B = _mapper()
    own = ("k_find_frontiers", "k_view_gain", "k_seg_", "k_frontier_classes")
    for m in (A, B):
        m.set_color_deferral(True); m.set_profiling(True)
    results = []
    for k, (d, rgb, T) in enumerate(frames):
        for m in (A, B):
            m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM); m.update_esdf()
        if k in (2, 4):
            results.append(A.find_frontiers()[3])
            A.frontier_clusters(connectivity=6, min_voxels=2)
            results.append(A.view_gain(np.stack([T, frames[0][2]]), CAM, subsampling=4, max_range_m=3.0))
    for m in (A, B):
        m.synchronize()
    assert int(results[0].item()) > 10 and int(results[1][0, 0]) == 300
    pa = {k: v["count"] for k, v in A.profile().items() if not k.startswith("_") and not any(o in k for o in own)}
    pb = {k: v["count"] for k, v in B.profile().items() if not k.startswith("_")}
    assert pa == pb, (pa, pb)
    assert any("k_integrate_tsdf_color" in k for k in pa), list(pa)[:20]     # the pipelined path has run: colour frames were carried, not flushed
    before = H.map_state(A)
    A.find_frontiers(); A.frontier_clusters(); A.view_gain(np.stack([f[2] for f in frames]), CAM, subsampling=4, max_range_m=3.0)
    H.assert_same_map(before, A, "before and after the three calls")
    H.assert_same_map(before, B, "against the mapper that never made them")
    A.close(); B.close()


# ---- 9. refusals
def test_refusals_launch_nothing_and_leave_the_mapper_usable(hip_lib):
    import torch
    M, _ = _mods()
    m = _mapper(cap=64)
    _upload(m, {(0, 0, 0): _block()})
    m.synchronize(); m.set_profiling(True)
    lib, h = m.lib, m._h
    idx = torch.zeros((4, 3), dtype=torch.int32, device="cuda"); lab = torch.zeros((4, 512), dtype=torch.int32, device="cuda")
    sc = torch.zeros((4, 512), dtype=torch.float32, device="cuda"); ids = torch.zeros((4, 512), dtype=torch.int32, device="cuda")
    rec = m.component_records(16); cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    gains = torch.zeros((2, 4), dtype=torch.int32, device="cuda"); poses = torch.eye(4, device="cuda").reshape(1, 16).repeat(2, 1).contiguous()
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan = float("nan")
    box_bad = (C.c_int32 * 6)(0, 0, 5, 7, 7, 4)
    cam = M.Mapper._cam(CAM)
    small = M.Mapper._cam((40.0, 40.0, 1.0, 1.0, 4, 4))
    nocam = M.Mapper._cam((0.0, 40.0, 1.0, 1.0, 80, 60))

    def ff(mw=1e-4, fd=0.05, mu=1, box=None, i=p(idx), l=p(lab), s=p(sc), cap=4, c=p(cnt)):
        return lib.nvbx_find_frontiers(h, mw, fd, mu, box, i, l, s, cap, c)

    def fc(mu=1, conn=6, mv=1, i=p(idx), l=p(lab), d=p(ids), cap=4, bc=p(cnt), r=p(rec), rcap=16, cc=C.c_void_p(cnt.data_ptr() + 8)):
        return lib.nvbx_frontier_clusters(h, 1e-4, 0.05, mu, None, conn, mv, i, l, p(sc), d, cap, bc, r, rcap, cc)

    def vg(T=p(poses), n=2, k=cam, s=4, rng=3.0, mw=1e-4, fd=0.05, g=p(gains)):
        return lib.nvbx_view_gain(h, T, n, C.byref(k) if k is not None else None, s, rng, mw, fd, g)
    refused = [
        lambda: ff(mu=0), lambda: ff(mu=7), lambda: ff(mw=nan), lambda: ff(fd=nan), lambda: ff(cap=-1), lambda: ff(cap=(1 << 22) + 1),
        lambda: ff(c=None), lambda: ff(i=None), lambda: ff(l=None), lambda: ff(box=box_bad),
        lambda: fc(mu=0), lambda: fc(conn=18), lambda: fc(mv=0), lambda: fc(d=None), lambda: fc(bc=None), lambda: fc(cc=None), lambda: fc(r=None),
        lambda: fc(r=C.c_void_p(rec.data_ptr() + 4)), lambda: fc(rcap=-1), lambda: fc(i=None),
        lambda: vg(n=-1), lambda: vg(T=None), lambda: vg(g=None), lambda: vg(k=None), lambda: vg(s=-1), lambda: vg(k=small), lambda: vg(k=nocam),
        lambda: vg(rng=float("inf")), lambda: vg(mw=nan), lambda: vg(fd=nan),
    ]
    for i, call in enumerate(refused):
        assert call() == E_INVALID, "refusal %d" % i
        assert lib.nvbx_last_error(), "refusal %d" % i
    m.synchronize()
    assert not any(k.startswith("k_") for k in m.profile()), list(m.profile())        # nothing was launched
    assert vg(n=0) == 0 and ff(cap=0, i=None, l=None, s=None) == 0                     # not refusals: no views; count only
    # an occupancy mapper has no TSDF layer
    occ = _mapper(cap=64, projective_layer_type=1)
    assert lib.nvbx_find_frontiers(occ._h, 1e-4, 0.05, 1, None, p(idx), p(lab), p(sc), 4, p(cnt)) == E_INVALID
    assert lib.nvbx_frontier_clusters(occ._h, 1e-4, 0.05, 1, None, 6, 1, p(idx), p(lab), p(sc), p(ids), 4, p(cnt), p(rec), 16, C.c_void_p(cnt.data_ptr() + 8)) == E_INVALID
    assert lib.nvbx_view_gain(occ._h, p(poses), 2, C.byref(cam), 4, 3.0, 1e-4, 0.05, p(gains)) == E_INVALID
    with pytest.raises(M.NvbxError):
        occ.find_frontiers()
    occ.close()
    # the mapper is still usable
    m.set_profiling(False)
    fr = _check(m, "after the refusals")
    assert (fr[(0, 0, 0)][0] == 0).sum() == 296
    assert m.view_gain(np.eye(4, dtype=F32)[None], CAM, subsampling=4, max_range_m=1.0).cpu().numpy()[0, 0] == 300
    m.close()
