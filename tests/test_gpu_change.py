"""Change detection on the GPU (nvbx_find_changes / nvbx_change_clusters; SEMANTICS.md "Change detection") against the numpy model of
tests/change_independent.py: entries sorted by block index, labels, scores and every field of the result record bit for bit, component records
as sets of tuples against scipy.ndimage.label.  Maps are hand-built with set_blocks (tests/change_cases.py draws them) or are the two rooms of
tests/test_change_model.py, fused on the GPU from the same 80 x 60 frames; block_capacity at most 1 << 12.  One GPU: the refusal of mappers on
different devices is not reached here."""
import ctypes as C
import os

import numpy as np
import pytest

import change_cases as CC
import change_independent as CI
import helpers as H
import segment_independent as SI

pytestmark = pytest.mark.gpu

VS = CC.VS
F32 = np.float32
SENTINEL = -77
E_INVALID = -1
SAMPLING = {"trilinear": CI.TRILINEAR, "nearest": CI.NEAREST}
OFF_T = CI.MI.pose([0.3, -0.2, 1.0], 1.5, [0.03, -0.01, 0.02])      # 3 cm and 1.5 degrees off


def _mods():
    from isaac_ros_nvblox_amd import mapper as M
    return M


def _mapper(cap=1 << 12, **params):
    M = _mods()
    return M.Mapper(M.default_params(**dict(CC.PARAMS, **params)), device=0, block_capacity=cap)


def _upload(m, tsdf):
    M = _mods()
    ks = sorted(tsdf)
    m.set_blocks(M.LAYER_TSDF, np.array(ks, np.int32), np.stack([tsdf[k] for k in ks]))


def _read(m):
    M = _mods()
    idx = m.block_indices(M.LAYER_TSDF)
    if not len(idx):
        return {}
    v, found = m.get_blocks(M.LAYER_TSDF, idx)
    assert found.all()
    return {tuple(int(q) for q in b): v[i].copy() for i, b in enumerate(idx)}


def _as_dict(idx, lab, sc):
    idx = idx.cpu().numpy(); lab = lab.cpu().numpy(); sc = sc.cpu().numpy()
    out = {tuple(int(q) for q in b): (lab[i], sc[i]) for i, b in enumerate(idx)}
    assert len(out) == len(idx), "a block appears in two entries"
    return out


def _same(got, want, what=""):
    assert sorted(got) == sorted(want), (what, sorted(set(got) ^ set(want))[:8])
    for k in sorted(want):
        assert got[k][0].dtype == np.int32 and got[k][1].dtype == np.float32
        assert np.array_equal(got[k][0], want[k][0]), "%s: labels of block %r differ at %s" % (what, k, np.flatnonzero(got[k][0] != want[k][0])[:6])
        assert got[k][1].tobytes() == want[k][1].tobytes(), "%s: scores of block %r differ" % (what, k)


def _same_result(res, want, what=""):
    got = {f: getattr(res, f) for f in CI.RESULT_FIELDS}
    assert got == {f: want[f] for f in CI.RESULT_FIELDS}, (what, got, {f: want[f] for f in CI.RESULT_FIELDS})
    assert res.status_name == _mods().CHANGE_STATUS_NAMES[want["status"]]


def _check(m, ref, T, m_tsdf, ref_tsdf, what="", box_m=None, **opts):
    """find_changes on the GPU, the model on the layers as they were read back: compared exactly.  -> the model's result"""
    sampling = opts.pop("sampling", "trilinear")
    box = None if box_m is None else tuple(int(v) for v in np.floor(np.asarray(box_m, F32).reshape(2, 3) / F32(VS)).astype(np.int64).reshape(6))
    want = CI.changes(m_tsdf, ref_tsdf, T, VS, sampling=SAMPLING[sampling], box_vox=box, **opts)
    idx, lab, sc, cnt, res = m.find_changes(ref, T, sampling=sampling, box_m=box_m, **opts)
    assert int(cnt.item()) == len(want["volume"]) == len(idx), (what, int(cnt.item()), len(want["volume"]))
    _same(_as_dict(idx, lab, sc), want["volume"], what)
    _same_result(res, want, what)
    return want


# ---- 1. hand-made blocks: every path of the sampling
@pytest.fixture(scope="module")
def drawn(hip_lib):
    m_tsdf, ref_tsdf = CC.drawn_maps(5)
    m = _mapper(cap=256); ref = _mapper(cap=256)
    _upload(m, m_tsdf); _upload(ref, ref_tsdf)
    m_back, ref_back = _read(m), _read(ref)
    for a, b in ((m_tsdf, m_back), (ref_tsdf, ref_back)):      # NaN distances and all: the maps hold the drawn bits
        assert sorted(a) == sorted(b) and all(a[k].tobytes() == b[k].tobytes() for k in a)
    yield m, ref, m_back, ref_back
    m.close(); ref.close()


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
@pytest.mark.parametrize("case", [0, 1, 2, 3])
def test_drawn_blocks_equal_the_model(drawn, case, sampling):
    m, ref, m_tsdf, ref_tsdf = drawn
    name, T = CC.drawn_transforms()[case]
    want = _check(m, ref, T, m_tsdf, ref_tsdf, "%s, %s" % (name, sampling), sampling=sampling)
    assert want["voxels_appeared"] >= 32 and want["voxels_removed"] >= 32, (name, sampling, want["voxels_appeared"], want["voxels_removed"])
    # ... with other thresholds and weights, one of them a stored value
    _check(m, ref, T, m_tsdf, ref_tsdf, "%s, %s, thresholds" % (name, sampling), sampling=sampling, min_weight=1.0, ref_min_weight=3.0,
           free_distance_m=0.1, occupied_distance_m=-0.05)


# ---- 2. the rooms
@pytest.fixture(scope="module")
def rooms(hip_lib):
    out = []
    for scene in CC.scenes():
        m = _mapper()
        for d, T in CC.frames(scene):
            m.integrate_depth(d, T, CC.CAM)
        m.synchronize()
        out.append(m)
    ref, now = out
    yield now, ref, _read(now), _read(ref)
    now.close(); ref.close()


@pytest.mark.parametrize("sampling", ["trilinear", "nearest"])
def test_room_changes_equal_the_model(rooms, sampling):
    now, ref, now_tsdf, ref_tsdf = rooms
    I = np.eye(4, dtype=F32)
    want = _check(now, ref, I, now_tsdf, ref_tsdf, "room, identity", sampling=sampling)
    assert want["status"] == CI.OK and want["blocks_scanned"] >= 20 and want["voxels_appeared"] > 200 and want["voxels_removed"] > 200
    CC.check_room(want["volume"], float(now.params.truncation_distance_vox) * VS, "the GPU's rooms, " + sampling)
    _check(now, ref, OFF_T, now_tsdf, ref_tsdf, "room, 3 cm and 1.5 degrees off", sampling=sampling)


def test_room_box_cuts_through_blocks(rooms):
    now, ref, now_tsdf, ref_tsdf = rooms
    I = np.eye(4, dtype=F32)
    box_m = ((1.02, -1.63, 0.11), (1.93, -0.57, 0.83))                          # inside the new sphere's blocks, on no block border
    full = CI.changes(now_tsdf, ref_tsdf, I, VS)
    cut = _check(now, ref, I, now_tsdf, ref_tsdf, "room, a box", box_m=box_m)
    assert 0 < cut["voxels_appeared"] < full["voxels_appeared"] and cut["voxels_removed"] == 0 and cut["voxels_compared"] < full["voxels_compared"]
    assert any(0 < int((cut["volume"][k][0] >= 0).sum()) < int((full["volume"][k][0] >= 0).sum()) for k in cut["volume"])      # a block is cut
    far = _check(now, ref, I, now_tsdf, ref_tsdf, "room, a box outside", box_m=((40.0, 40.0, 40.0), (41.0, 41.0, 41.0)))
    assert far["status"] == CI.NO_OVERLAP and not far["volume"]


def _records(rec):
    return rec.cpu().numpy().view(SI.COMPONENT_DT).reshape(-1)


@pytest.mark.parametrize("conn,mv", [(26, 8), (6, 1)])
def test_room_clusters_equal_the_model(rooms, conn, mv):
    import torch
    M = _mods()
    now, ref, now_tsdf, ref_tsdf = rooms
    I = np.eye(4, dtype=F32)
    want = CI.changes(now_tsdf, ref_tsdf, I, VS)
    exp_c, exp_k = CI.clusters(want["volume"], conn, mv)
    cap = len(now_tsdf)
    idx = torch.empty((cap, 3), dtype=torch.int32, device="cuda"); lab = torch.empty((cap, 512), dtype=torch.int32, device="cuda")
    sc = torch.empty((cap, 512), dtype=torch.float32, device="cuda"); ids = torch.empty((cap, 512), dtype=torch.int32, device="cuda")
    rec = now.component_records(cap * 512 // mv)
    bcnt = torch.zeros(1, dtype=torch.int64, device="cuda"); ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    rbuf = torch.zeros(M.CHANGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    out = now.change_clusters(ref, I, connectivity=conn, min_voxels=mv, out=(idx, lab, sc, ids, bcnt, rec, ccnt, rbuf))
    assert out[0] is idx and out[5] is rec and out[7].buffer is rbuf                  # the out= form hands back what it was given
    nb, count = int(bcnt.item()), int(ccnt.item())
    assert nb == len(want["volume"]) and count == len(exp_c) > 0
    idx, lab, sc, ids = (t[:nb].cpu().numpy() for t in (idx, lab, sc, ids))
    _same({tuple(int(q) for q in b): (lab[i], sc[i]) for i, b in enumerate(idx)}, want["volume"], "clusters' volume")
    _same_result(out[7], want, "clusters' result")
    got_c, got_k = SI.canonical(idx, lab, ids, _records(rec)[:count], count)
    order = {tuple(b): i for i, b in enumerate(idx.tolist())}
    perm = [order[k] for k in sorted(want["volume"])]                               # the model's keys are in sorted block order
    assert np.array_equal(got_k[perm], exp_k), "the partition differs at %d voxels" % int((got_k[perm] != exp_k).sum())
    assert got_c == exp_c
    labels = [c[0] for c in exp_c.values()]
    assert CI.APPEARED in labels and CI.REMOVED in labels
    # the wrapper's trimmed form
    i2, l2, s2, ids2, comps, res = now.change_clusters(ref, I, connectivity=conn, min_voxels=mv)
    assert len(i2) == nb and len(comps.voxels) == count and sorted(comps.voxels.cpu().tolist()) == sorted(c[1] for c in exp_c.values())
    _same_result(res, want, "the wrapper's result")
    cm = comps.centroid_m.cpu().numpy()
    assert cm.shape == (count, 3) and np.isfinite(cm).all()


def test_room_capacity_count_only_and_out_form(rooms):
    import torch
    M = _mods()
    now, ref, now_tsdf, ref_tsdf = rooms
    I = np.eye(4, dtype=F32)
    want = CI.changes(now_tsdf, ref_tsdf, I, VS)
    n = len(want["volume"])
    assert n > 6
    z = lambda *s, dt=torch.int32: torch.empty(s, dtype=dt, device="cuda")      # noqa: E731
    # capacity 0 with NULL arrays only counts; the record is complete
    cnt = torch.full((1,), 99, dtype=torch.int64, device="cuda")
    rbuf = torch.zeros(M.CHANGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
    out = now.find_changes(ref, I, out=(z(0, 3), z(0, 512), None, cnt, rbuf))
    assert int(cnt.item()) == n
    _same_result(out[4], want, "count only")
    # capacity 4 < count: the count in full, four valid entries, the canaries behind them untouched
    idx = torch.full((8, 3), SENTINEL, dtype=torch.int32, device="cuda")
    lab = torch.full((8, 512), SENTINEL, dtype=torch.int32, device="cuda")
    sc = torch.full((8, 512), float(SENTINEL), dtype=torch.float32, device="cuda")
    out = now.find_changes(ref, I, out=(idx[:4], lab[:4], sc[:4], cnt, None))
    assert out[4] is None and int(cnt.item()) == n
    got = _as_dict(idx[:4], lab[:4], sc[:4])
    assert len(got) == 4 and set(got) <= set(want["volume"])
    _same(got, {k: want["volume"][k] for k in got}, "capacity 4")
    assert (idx[4:] == SENTINEL).all() and (lab[4:] == SENTINEL).all() and (sc[4:] == float(SENTINEL)).all()
    # no scores wanted: labels alone
    lab2 = torch.full((n, 512), SENTINEL, dtype=torch.int32, device="cuda")
    idx2 = z(n, 3)
    now.find_changes(ref, I, out=(idx2, lab2, None, cnt, None))
    got = {tuple(int(q) for q in b): l for b, l in zip(idx2.cpu().numpy(), lab2.cpu().numpy())}
    assert sorted(got) == sorted(want["volume"]) and all(np.array_equal(got[k], want["volume"][k][0]) for k in got)
    # the clusters call under capacity 4: the labelling reads min(count, capacity) entries
    ids = torch.full((8, 512), SENTINEL, dtype=torch.int32, device="cuda")
    rec = now.component_records(64); bcnt = torch.zeros(1, dtype=torch.int64, device="cuda"); ccnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    now.change_clusters(ref, I, connectivity=26, min_voxels=1, out=(idx[:4], lab[:4], sc[:4], ids[:4], bcnt, rec, ccnt, None))
    assert int(bcnt.item()) == n and int(ccnt.item()) >= 1 and (ids[4:] == SENTINEL).all() and (lab[4:] == SENTINEL).all()
    with pytest.raises(ValueError):
        now.find_changes(ref, I, out=(idx, lab, sc, cnt))                      # the result entry is part of out
    with pytest.raises(ValueError):
        now.find_changes(ref, I, sampling="cubic")
    with pytest.raises(TypeError):
        now.find_changes(None, I)


# ---- 3. the grid is launch geometry only
def test_result_does_not_depend_on_the_grid(rooms):
    now, ref, now_tsdf, ref_tsdf = rooms
    assert len(now_tsdf) >= 20
    a = now.find_changes(ref, OFF_T)
    old = os.environ.get("NVBX_CHANGE_GRID")
    os.environ["NVBX_CHANGE_GRID"] = "3"
    try:
        now.reload_knobs()
        b = now.find_changes(ref, OFF_T)
    finally:
        if old is None:
            del os.environ["NVBX_CHANGE_GRID"]
        else:
            os.environ["NVBX_CHANGE_GRID"] = old
        now.reload_knobs()
    _same(_as_dict(*b[:3]), _as_dict(*a[:3]), "NVBX_CHANGE_GRID=3")
    assert {f: getattr(a[4], f) for f in CI.RESULT_FIELDS} == {f: getattr(b[4], f) for f in CI.RESULT_FIELDS} and a[4].voxels_appeared > 0


# ---- 4. neither map is written, held-back work does not change the answer
def test_maps_untouched_and_held_back_colour_stays_out_of_it(rooms):
    from isaac_ros_nvblox_amd import synthetic as S
    now, ref, now_tsdf, ref_tsdf = rooms
    I = np.eye(4, dtype=F32)
    before_now, before_ref = H.map_state(now), H.map_state(ref)
    now.find_changes(ref, I); now.change_clusters(ref, OFF_T, sampling="nearest"); ref.find_changes(now, I)
    H.assert_same_map(before_now, now, "the scanned map"); H.assert_same_map(before_ref, ref, "the reference")
    # a mapper in the pipelined order with a colour frame and an ESDF update held back: the same answer as after flush()
    a = _mapper()
    a.set_color_deferral(True)
    scene = CC.scenes()[1]
    for T in CC.poses():
        d, rgb = S.render(scene, T, CC.CAM)
        a.integrate_depth(d, T, CC.CAM); a.integrate_color(rgb, T, CC.CAM); a.update_esdf()
    held = a.find_changes(ref, OFF_T)
    as_ref = ref.find_changes(a, OFF_T)                                            # ... and as the reference of another mapper's scan
    a.flush()
    flushed = a.find_changes(ref, OFF_T)
    as_ref_flushed = ref.find_changes(a, OFF_T)
    for x, y, what in ((held, flushed, "scanned"), (as_ref, as_ref_flushed, "as the reference")):
        _same(_as_dict(*x[:3]), _as_dict(*y[:3]), "held back against flushed, " + what)
        assert {f: getattr(x[4], f) for f in CI.RESULT_FIELDS} == {f: getattr(y[4], f) for f in CI.RESULT_FIELDS}
    assert held[4].voxels_appeared > 0
    _same(_as_dict(*flushed[:3]), CI.changes(_read(a), ref_tsdf, OFF_T, VS)["volume"], "the flushed mapper against the model")
    a.close()


# ---- 5. statuses
def test_the_four_statuses(hip_lib):
    M = _mods()
    I = np.eye(4, dtype=F32)
    blk = np.zeros(512, CI.TSDF_DT); blk["distance"] = -0.1; blk["weight"] = 1.0
    other = blk.copy(); other["distance"] = 0.2
    m = _mapper(cap=64); ref = _mapper(cap=64)
    assert m.find_changes(ref, I)[4].status == M.CHANGE_EMPTY_MAP                  # both empty: the map's emptiness comes first
    _upload(ref, {(0, 0, 0): other})
    res = m.find_changes(ref, I)[4]
    assert (res.status, res.status_name, res.blocks_scanned) == (M.CHANGE_EMPTY_MAP, "EMPTY_MAP", 0)
    res = ref.find_changes(m, I)[4]
    assert (res.status, res.status_name, res.blocks_scanned, res.voxels_compared) == (M.CHANGE_EMPTY_REFERENCE, "EMPTY_REFERENCE", 1, 0)
    _upload(m, {(9, 0, 0): blk})
    for sampling in ("trilinear", "nearest"):
        _check(m, ref, I, _read(m), _read(ref), "far apart", sampling=sampling)
    assert m.find_changes(ref, I)[4].status == M.CHANGE_NO_OVERLAP
    T = CI.MI.pose([0, 0, 1], 0.0, [9 * 8 * VS, 0, 0])                             # brings the reference's block under the map's
    want = _check(m, ref, T, _read(m), _read(ref), "brought together", sampling="nearest")
    assert want["status"] == CI.OK and want["voxels_appeared"] == 512
    assert "OK" in repr(m.find_changes(ref, T, sampling="nearest")[4])
    m.close(); ref.close()


# ---- 6. refusals
def test_refusals_launch_nothing_and_leave_the_mappers_usable(hip_lib):
    import torch
    M = _mods()
    from isaac_ros_nvblox_amd import _lib
    blk = np.zeros(512, CI.TSDF_DT); blk["distance"] = -0.1; blk["weight"] = 1.0
    other = blk.copy(); other["distance"] = 0.2
    m = _mapper(cap=64); ref = _mapper(cap=64)
    _upload(m, {(0, 0, 0): blk}); _upload(ref, {(0, 0, 0): other})
    coarse = _mapper(cap=64, voxel_size=0.1); occ = _mapper(cap=64, projective_layer_type=1)
    for x in (m, ref):
        x.synchronize(); x.set_profiling(True)
    lib = m.lib
    idx = torch.zeros((4, 3), dtype=torch.int32, device="cuda"); lab = torch.zeros((4, 512), dtype=torch.int32, device="cuda")
    sc = torch.zeros((4, 512), dtype=torch.float32, device="cuda"); ids = torch.zeros((4, 512), dtype=torch.int32, device="cuda")
    rec = m.component_records(16); cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    rbuf = torch.zeros(M.CHANGE_RESULT_BYTES + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    nan, inf = float("nan"), float("inf")
    I = np.eye(4, dtype=F32)

    def pose(**kw):
        T = I.copy()
        for k, v in kw.items():
            T[int(k[1]), int(k[2])] = v
        return T
    box_bad = (C.c_int32 * 6)(0, 0, 5, 7, 7, 4)

    def opts(**kw):
        o = _lib.ChangeOptions()
        lib.nvbx_default_change_options(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def fc(a=m, b=ref, T=I, o=None, box=None, i=p(idx), l=p(lab), cap=4, c=p(cnt), r=p(rbuf)):
        T = None if T is None else np.ascontiguousarray(T, np.float32)
        return lib.nvbx_find_changes(a._h if a is not None else None, b._h if b is not None else None, None if T is None else T.ctypes.data_as(C.c_void_p),
                                     C.byref(o) if o is not None else None, box, i, l, p(sc), cap, c, r)

    def cc(o=None, conn=26, mv=8, i=p(idx), d=p(ids), cap=4, bc=p(cnt), rc=p(rec), rcap=16, ccn=C.c_void_p(cnt.data_ptr() + 8), r=p(rbuf)):
        return lib.nvbx_change_clusters(m._h, ref._h, I.ctypes.data_as(C.c_void_p), C.byref(o) if o is not None else None, None, conn, mv, i, p(lab), p(sc), d, cap,
                                        bc, rc, rcap, ccn, r)
    refused = [
        lambda: fc(b=m), lambda: fc(a=None), lambda: fc(b=None), lambda: fc(T=None),                      # ref == m; a missing mapper or pose
        lambda: fc(b=coarse), lambda: fc(a=coarse), lambda: fc(b=occ), lambda: fc(a=occ),                   # voxel sizes; a non-TSDF mapper on either side
        lambda: fc(T=pose(t03=nan)), lambda: fc(T=pose(t11=inf)), lambda: fc(T=pose(t03=4.2e5)),           # not finite; out of range
        lambda: fc(T=pose(t00=1.001)), lambda: fc(T=pose(t22=-1.0)),                                        # no rotation: scaled; a reflection
        lambda: fc(o=opts(min_weight=nan)), lambda: fc(o=opts(ref_min_weight=nan)), lambda: fc(o=opts(free_distance_m=nan)),
        lambda: fc(o=opts(occupied_distance_m=nan)),
        lambda: fc(o=opts(occupied_distance_m=0.06)),                                                        # above the default free distance, one voxel size
        lambda: fc(o=opts(free_distance_m=0.1, occupied_distance_m=0.2)),
        lambda: fc(o=opts(sampling=2)), lambda: fc(o=opts(sampling=-1)),
        lambda: fc(cap=-1), lambda: fc(cap=(1 << 22) + 1), lambda: fc(c=None), lambda: fc(i=None), lambda: fc(l=None), lambda: fc(box=box_bad),
        lambda: fc(r=C.c_void_p(rbuf.data_ptr() + 4)),
        lambda: cc(o=opts(sampling=5)), lambda: cc(conn=18), lambda: cc(mv=0), lambda: cc(d=None), lambda: cc(bc=None), lambda: cc(ccn=None), lambda: cc(rc=None),
        lambda: cc(rc=C.c_void_p(rec.data_ptr() + 4)), lambda: cc(rcap=-1), lambda: cc(i=None), lambda: cc(r=C.c_void_p(rbuf.data_ptr() + 4)),
    ]
    for i, call in enumerate(refused):
        assert call() == E_INVALID, "refusal %d" % i
        assert lib.nvbx_last_error(), "refusal %d" % i
    for x in (m, ref):
        x.synchronize()
        assert not any(k.startswith("k_") for k in x.profile()), list(x.profile())        # nothing was launched
    # not refusals: no result record; count only; occupied == free
    assert fc(r=None) == 0 and fc(cap=0, i=None, l=None) == 0 and fc(o=opts(free_distance_m=0.1, occupied_distance_m=0.1)) == 0
    with pytest.raises(M.NvbxError):
        m.find_changes(occ, I)
    with pytest.raises(M.NvbxError):
        m.find_changes(m, I)
    # the mappers are still usable
    for x in (m, ref):
        x.set_profiling(False)
    want = _check(m, ref, I, _read(m), _read(ref), "after the refusals", sampling="nearest")
    assert want["voxels_appeared"] == 512
    assert _check(ref, m, I, _read(ref), _read(m), "the other way round")["voxels_removed"] > 0
    for x in (m, ref, coarse, occ):
        x.close()
