"""Feature segmentation on the GPU (segment.hip; SEMANTICS.md "Feature segmentation") against the model of tests/segment_independent.py.
The index order of the components is unspecified, everything else is bit-specified: results are compared in canonical form -- the partition of
the voxels, and every record field after keying the components by their lowest voxel."""
import ctypes as C

import numpy as np
import pytest

import feature_match_independent as FM
import helpers as H
import segment_independent as SI

pytestmark = pytest.mark.gpu

ORIGIN = (-2, -2, -2)      # 3 x 3 x 3 blocks at -2 .. 0 per axis: negative and zero indices
SENTINEL = -77


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


@pytest.fixture(scope="module")
def mapper():
    """a mapper with no frame integrated at all: label_components reads nothing from the map"""
    M, _ = _mods()
    m = M.Mapper(M.default_params(), block_capacity=256)
    yield m
    m.close()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(m, fn):
    """a direct library call between torch's stream (which filled the buffers, and reads them next) and the mapper's"""
    import torch
    torch.cuda.synchronize()
    rc = fn()
    m.synchronize()
    return rc


def _records(rec):
    return rec.cpu().numpy().view(SI.COMPONENT_DT).reshape(-1)


def _label(m, bidx, lab, sc, conn, mv=1, capacity=None):
    """label_components into sentinel-filled buffers -> (ids, records, count) as numpy"""
    import torch
    n = len(bidx)
    cap = n * 512 if capacity is None else capacity
    ids = torch.full((n, 512), SENTINEL, dtype=torch.int32, device="cuda")
    rec = m.component_records(cap); rec.fill_(SENTINEL)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    out = m.label_components(bidx, lab, sc, conn, mv, out=(ids, rec, cnt))
    assert out[0] is ids and out[1] is rec and out[2] is cnt
    return ids.cpu().numpy(), _records(rec), int(cnt.item())


def _assert_equals_model(bidx, lab, sc, conn, mv, ids, recs, count):
    exp_c, exp_k = SI.model(bidx, lab, sc, conn, mv)
    assert count == len(exp_c), (count, len(exp_c))
    got_c, got_k = SI.canonical(bidx, lab, ids, recs, count)
    assert np.array_equal(got_k, exp_k), "the partition differs at %d voxels" % int((got_k != exp_k).sum())
    if len(recs) >= count:
        assert got_c == exp_c, [(k, got_c.get(k), exp_c.get(k)) for k in sorted(set(got_c) | set(exp_c)) if got_c.get(k) != exp_c.get(k)][:5]
    else:
        assert all(exp_c[k] == v for k, v in got_c.items()) and len(got_c) == len(recs)
    return exp_c


def _check(m, bidx, lab, sc, conn, mv=1):
    ids, recs, count = _label(m, bidx, lab, sc, conn, mv)
    assert (recs[count:].view(np.int32) == SENTINEL).all()          # nothing behind the last record is written
    return _assert_equals_model(bidx, lab, sc, conn, mv, ids, recs, count)


# ---- 1. one block
ONE_BLOCK = {
    "empty": lambda: np.full((8, 8, 8), -1, np.int32),
    "full": lambda: np.zeros((8, 8, 8), np.int32),
    "checkerboard": SI.checkerboard,
    "z_planes": SI.z_planes,
    "serpentine": SI.serpentine,
}


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("name", sorted(ONE_BLOCK))
def test_one_block(mapper, name, conn):
    bidx, lab, _ = SI.cut(ONE_BLOCK[name](), origin_block=(-1, 3, -7))
    c = _check(mapper, bidx, lab, None, conn)
    want = {"empty": 0, "full": 1, "checkerboard": 256 if conn == 6 else 1, "z_planes": 8 if conn == 6 else 8, "serpentine": 1}[name]
    assert len(c) == want


# ---- 2. 27 blocks, drawn
DRAWN = {"serpentine": lambda: SI.serpentine(24), "u": SI.u_shape, "contacts": SI.contacts, "side_by_side": SI.side_by_side}


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("middle", ["whole", "no_middle"])
@pytest.mark.parametrize("name", sorted(DRAWN))
def test_27_blocks_drawn(mapper, name, middle, conn):
    bidx, lab, _ = SI.cut(DRAWN[name](), origin_block=ORIGIN, drop=[(1, 1, 1)] if middle == "no_middle" else [], seed=11)
    assert len(bidx) == (27 if middle == "whole" else 26) and (bidx < 0).any() and (bidx == 0).any()
    c = _check(mapper, bidx, lab, None, conn)
    if middle == "whole":
        assert len(c) == {"serpentine": 1, "u": 1, "contacts": 10 if conn == 6 else 5, "side_by_side": 2}[name]


# ---- 3. 27 blocks of noise
@pytest.fixture(scope="module")
def noise27():
    L, s, sq = SI.noise((24, 24, 24))
    bidx, lab, sc = SI.cut(L, s, origin_block=ORIGIN, seed=7)
    _, _, scq = SI.cut(L, sq, origin_block=ORIGIN, seed=7)
    return bidx, lab, sc, scq


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("scores", ["random", "quantised", "none"])
@pytest.mark.parametrize("mv", [1, 2, 5])
def test_27_blocks_of_noise(mapper, noise27, mv, scores, conn):
    bidx, lab, sc, scq = noise27
    c = _check(mapper, bidx, lab, {"random": sc, "quantised": scq, "none": None}[scores], conn, mv)
    if conn == 6 and mv == 1:
        assert len(c) == 431 + 488                                  # what the model test prints for this seed
    if conn == 26:
        assert len(c) <= 3


def test_returned_components_view_the_records(mapper, noise27):
    """out=None: trimmed results; the named tuple's fields are the records', centroid_m = (sum / voxels + 0.5) voxel_size in float64"""
    bidx, lab, sc, _ = noise27
    ids, comps = mapper.label_components(bidx, lab, sc, connectivity=6, min_voxels=5)
    exp_c, _ = SI.model(bidx, lab, sc, 6, 5)
    n = len(exp_c)
    assert tuple(ids.shape) == (27, 512) and all(len(f) == n for f in comps)
    recs = np.zeros(n, SI.COMPONENT_DT)
    for f in SI.COMPONENT_DT.names:
        recs[f] = getattr(comps, f).cpu().numpy()
    _assert_equals_model(bidx, lab, sc, 6, 5, ids.cpu().numpy(), recs, n)
    cm = comps.centroid_m.cpu().numpy()
    assert cm.dtype == np.float64
    assert np.array_equal(cm, (recs["sum_xyz"].astype(np.float64) / recs["voxels"].astype(np.float64)[:, None] + 0.5) * float(mapper.params.voxel_size))


# ---- 4. 128 blocks, a device count below the list's length
@pytest.mark.parametrize("conn", [6, 26])
def test_128_blocks_with_a_device_count_of_100(mapper, conn):
    import torch
    m = mapper
    L, s, _ = SI.noise((64, 64, 16), seed=5)
    bidx, lab, sc = SI.cut(L, s, origin_block=(-3, -4, -1), seed=13)
    n, used = 128, 100
    assert len(bidx) == n
    d_idx, d_lab, d_sc = (torch.from_numpy(a).cuda() for a in (bidx, lab, sc))
    ids = torch.full((n, 512), SENTINEL, dtype=torch.int32, device="cuda")
    rec = m.component_records(n * 512); rec.fill_(SENTINEL)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    n_dev = torch.tensor([used], dtype=torch.int64, device="cuda")
    assert _raw(m, lambda: m.lib.nvbx_label_components(m._h, P(d_idx), P(d_lab), P(d_sc), n, P(n_dev), conn, 1, P(ids), P(rec), n * 512, P(cnt))) == 0
    ids = ids.cpu().numpy(); count = int(cnt.item()); recs = _records(rec)
    assert (ids[used:] == SENTINEL).all()                           # entries behind the device count are not written ...
    assert (recs[count:].view(np.int32) == SENTINEL).all()
    _assert_equals_model(bidx[:used], lab[:used], sc[:used], conn, 1, ids[:used], recs, count)      # ... nor read: the model sees 100 blocks
    # a device count above the list's length reads the list's length
    n_dev.fill_(1 << 40); ids2 = torch.full((n, 512), SENTINEL, dtype=torch.int32, device="cuda")
    assert _raw(m, lambda: m.lib.nvbx_label_components(m._h, P(d_idx), P(d_lab), P(d_sc), used, P(n_dev), conn, 1, P(ids2), P(rec), n * 512, P(cnt))) == 0
    assert (ids2[used:] == SENTINEL).all().item()
    _assert_equals_model(bidx[:used], lab[:used], sc[:used], conn, 1, ids2[:used].cpu().numpy(), _records(rec), int(cnt.item()))


# ---- 5. capacity
@pytest.mark.parametrize("conn", [6, 26])
def test_capacity_below_the_count(mapper, noise27, conn):
    import torch
    m = mapper
    bidx, lab, sc, _ = noise27
    full = len(SI.model(bidx, lab, sc, conn, 1)[0])
    cap = max(1, full // 2)
    # the table given to the call ends at `cap`: the 7 records behind it stay as they were
    ids_t = torch.full((27, 512), SENTINEL, dtype=torch.int32, device="cuda")
    rec = m.component_records(cap + 7); rec.fill_(SENTINEL)
    cnt = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    m.label_components(bidx, lab, sc, conn, 1, out=(ids_t, rec[:cap], cnt))
    count = int(cnt.item()); recs = _records(rec)
    assert count == full                                            # the full number
    assert (recs[cap:].view(np.int32) == SENTINEL).all()
    ids = ids_t.cpu().numpy()
    if full > cap:
        assert ids.max() == full - 1                                # the ids above the capacity are in the volume
    _assert_equals_model(bidx, lab, sc, conn, 1, ids, recs[:cap], count)
    # capacity 0 with a NULL table: counts and labels
    ids_t.fill_(SENTINEL); cnt.fill_(SENTINEL)
    m.label_components(bidx, lab, sc, conn, 1, out=(ids_t, None, cnt))
    assert int(cnt.item()) == full
    _assert_equals_model(bidx, lab, sc, conn, 1, ids_t.cpu().numpy(), recs[:0], full)


# ---- 6. refusals
def test_refusals_leave_the_mapper_usable(mapper):
    import torch
    m = mapper
    bidx, lab, sc = SI.cut(SI.serpentine(8), np.zeros((8, 8, 8), np.float32))
    d_idx, d_lab, d_sc = (torch.from_numpy(a).cuda() for a in (bidx, lab, sc))
    ids = torch.zeros((1, 512), dtype=torch.int32, device="cuda"); rec = m.component_records(512)
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    INVALID = -1

    def call(idx_=d_idx, lab_=d_lab, sc_=d_sc, n=1, n_dev=None, conn=6, mv=1, ids_=ids, rec_=rec, cap=512, cnt_=cnt):
        return _raw(m, lambda: m.lib.nvbx_label_components(m._h, P(idx_), P(lab_), P(sc_), n, P(n_dev), conn, mv, P(ids_),
                                                            rec_ if isinstance(rec_, C.c_void_p) else P(rec_), cap, P(cnt_)))

    def fine():
        cnt.fill_(SENTINEL)
        assert call() == 0
        assert int(cnt.item()) == 1
    fine()
    misaligned = C.c_void_p(rec.data_ptr() + 4)
    for bad in (dict(conn=0), dict(conn=18), dict(conn=-6), dict(mv=0), dict(mv=-3), dict(n=-1), dict(n=(1 << 22) + 1), dict(idx_=None), dict(lab_=None),
                dict(ids_=None), dict(cnt_=None), dict(cnt_=None, n=0), dict(rec_=None), dict(cap=-1), dict(rec_=misaligned)):
        assert call(**bad) == INVALID, bad
        assert m.lib.nvbx_last_error()
        fine()
    assert call(sc_=None) == 0 and call(rec_=None, cap=0) == 0      # scores and, with capacity 0, the table are optional
    cnt.fill_(SENTINEL)
    assert call(idx_=None, lab_=None, sc_=None, ids_=None, rec_=None, cap=0, n=0) == 0      # n_blocks == 0: a count of 0, nothing else is required
    assert int(cnt.item()) == 0
    for kw in (dict(connectivity=18), dict(min_voxels=0)):
        with pytest.raises(ValueError):
            m.label_components(bidx, lab, None, **kw)
    ids0, comps0 = m.label_components(np.zeros((0, 3), np.int32), np.zeros((0, 512), np.int32))
    assert tuple(ids0.shape) == (0, 512) and len(comps0.label) == 0 and tuple(comps0.centroid_m.shape) == (0, 3)
    fine()


def test_a_repeated_block_index_gives_a_valid_partition_without_a_fault(mapper):
    bidx, lab, _ = SI.cut(SI.serpentine(24), origin_block=ORIGIN, seed=11)
    bidx = np.concatenate([bidx, bidx[:5]]); lab = np.concatenate([lab, lab[:5]])
    import torch
    m = mapper
    ids = torch.full((len(bidx), 512), SENTINEL, dtype=torch.int32, device="cuda"); cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.label_components(torch.from_numpy(bidx).cuda(), torch.from_numpy(lab).cuda(), None, 6, 1, out=(ids, None, cnt))
    ids = ids.cpu().numpy(); count = int(cnt.item())
    # Which copy the neighbours see is unspecified, and a copy they do not see joins only what lies in its own positive directions: the path may
    # come in pieces.  What holds: exactly the foreground is labelled, the ids are 0 .. count - 1, and a block-local piece is never split.
    assert 1 <= count <= 1 + 5 * 512
    assert ((ids >= 0) == (lab >= 0)).all() and np.array_equal(np.unique(ids[ids >= 0]), np.arange(count))
    for e in range(len(bidx)):
        _, local = SI.model(bidx[e:e + 1], lab[e:e + 1], None, 6)
        for k in np.unique(local[local >= 0]):
            assert len(np.unique(ids[e][local[0] == k])) == 1


# ---- 7. / 8. on a feature map (the fixture of tests/test_gpu_feature_match.py)
CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
STRIDE = 4


@pytest.fixture(scope="module")
def room_frames():
    _, S = _mods()
    sc = S.Scene()
    out = []
    for i in range(3):
        T = S.trajectory_pose(i * 9)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


def _feature_image(rng, Cn):
    return rng.standard_normal((CAM[5] // STRIDE, CAM[4] // STRIDE, Cn)).astype(np.float16)


@pytest.fixture(scope="module")
def feature_map(room_frames):
    M, _ = _mods()
    Cn = 8
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.set_color_deferral(False)
    m.enable_features(Cn)
    rng = np.random.default_rng(1000 + Cn)
    for d, rgb, T in room_frames:
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM)
        m.integrate_features(_feature_image(rng, Cn), T, CAM, STRIDE)
    yield m, Cn
    m.close()


def _queries(Cn, Q):
    return np.random.default_rng(77 * Cn + Q).standard_normal((Q, Cn)).astype(np.float16)


def test_both_calls_leave_the_map_bit_identical(feature_map, noise27):
    M, _ = _mods()
    m, Cn = feature_map

    layers = (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF, M.LAYER_FEATURE)
    before = H.map_state(m, layers), m.block_indices(M.LAYER_MESH), m.counters()
    bidx, lab, sc, _ = noise27
    for conn in (6, 26):
        m.label_components(bidx, lab, sc, conn, 2)
        for metric in ("dot", "cosine"):
            m.segment_features(_queries(Cn, 5), metric, 1.0, 0.0, conn, 2)
    H.assert_same_map(before[0], m, "before and after the calls", min_blocks={M.LAYER_TSDF: 101, M.LAYER_COLOR: 51, M.LAYER_FEATURE: 51})
    assert np.array_equal(before[1], m.block_indices(M.LAYER_MESH)) and before[2] == m.counters()


def _thresholds(best, lab, bound, Q):
    """Per query the midpoint of the widest gap between consecutive sorted best scores within the 40th .. 60th percentile; the window widens until
    that gap is at least 8 times the score error bound, so that no voxel sits at its threshold."""
    thr = np.full(Q, np.nan, np.float32)
    for q in range(Q):
        s = np.sort(best[lab == q].astype(np.float64))
        assert len(s) >= 20, "query %d is the best of %d voxels only" % (q, len(s))
        bq = float(bound[lab == q].max())
        for half in (10, 20, 30, 40, 50):
            lo, hi = int(len(s) * (50 - half) / 100), max(int(len(s) * (50 + half) / 100), 2)
            gaps = np.diff(s[lo:hi])
            k = int(np.argmax(gaps))
            if gaps[k] >= 8 * bq:
                break
        print("query %d: %d voxels, gap %.3g = %.1f bounds in the %d .. %d percentile window" % (q, len(s), gaps[k], gaps[k] / bq, 50 - half, 50 + half))
        assert gaps[k] >= 8 * bq, (q, gaps[k], bq)
        t = np.float32(0.5 * (s[lo + k] + s[lo + k + 1]))
        assert s[lo + k] < t < s[lo + k + 1]
        thr[q] = t
    return thr


@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_segment_features_end_to_end(feature_map, metric, conn):
    M, _ = _mods()
    m, Cn = feature_map
    Q = 5
    q = _queries(Cn, Q)
    idx0, lab0, sc0 = (t.cpu().numpy() for t in m.match_features(q, metric, 1.0)[:3])
    f, _, found = m.feature_blocks(idx0)
    assert found.all()
    bound = np.take_along_axis(FM.bound(f, q, metric), np.maximum(lab0, 0)[..., None].astype(np.int64), -1)[..., 0]
    thr = _thresholds(sc0, lab0, bound, Q)
    where = {tuple(b): i for i, b in enumerate(idx0.tolist())}

    def run(min_score, thr_model, mv):
        idx, lab, sc, ids, comps = m.segment_features(q, metric, 1.0, min_score, conn, mv)
        idx, lab, sc, ids = (t.cpu().numpy() for t in (idx, lab, sc, ids))
        got = [tuple(b) for b in idx.tolist()]
        assert len(got) == len(set(got)) == len(where) and set(got) == set(where)
        perm = np.array([where[g] for g in got])
        exp_lab, exp_sc = (lab0[perm], sc0[perm]) if thr_model is None else SI.threshold(lab0[perm], sc0[perm], thr_model)
        assert np.array_equal(lab, exp_lab) and np.array_equal(sc.view(np.uint32), exp_sc.view(np.uint32))      # bit for bit
        n = len(comps.label)
        recs = np.zeros(n, SI.COMPONENT_DT)
        for name in SI.COMPONENT_DT.names:
            recs[name] = getattr(comps, name).cpu().numpy()
        c = _assert_equals_model(idx, exp_lab, exp_sc, conn, mv, ids, recs, n)
        return exp_lab, c
    kept, c = run(thr, thr, 3)
    assert 0 < (kept >= 0).sum() < (lab0 >= 0).sum() and len(c) > 0                # the threshold drops some voxels and keeps some
    run(None, None, 1)                                                             # no threshold
    mid = np.float32(np.median(thr))
    if not (np.abs(sc0[lab0 >= 0].astype(np.float64) - float(mid)) >= 8 * bound[lab0 >= 0]).all():      # a scalar for all queries, clear of every score
        cand = np.sort(sc0[lab0 >= 0].astype(np.float64)); k = len(cand) // 2
        gaps = np.diff(cand[k - len(cand) // 4:k + len(cand) // 4]); j = int(np.argmax(gaps)) + k - len(cand) // 4
        assert cand[j + 1] - cand[j] >= 8 * float(bound.max())
        mid = np.float32(0.5 * (cand[j] + cand[j + 1]))
    run(float(mid), np.full(Q, mid, np.float32), 1)


def test_segment_features_into_given_buffers_and_its_refusals(feature_map):
    import torch
    M, _ = _mods()
    m, Cn = feature_map
    Q = 5
    q = torch.from_numpy(_queries(Cn, Q)).cuda()
    n = m.num_blocks(M.LAYER_FEATURE)
    cap = n + 3
    idx = torch.full((cap, 3), SENTINEL, dtype=torch.int32, device="cuda"); lab = torch.full((cap, 512), SENTINEL, dtype=torch.int32, device="cuda")
    sc = torch.full((cap, 512), float(SENTINEL), device="cuda"); ids = torch.full((cap, 512), SENTINEL, dtype=torch.int32, device="cuda")
    bc = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda"); cc = torch.full((1,), SENTINEL, dtype=torch.int64, device="cuda")
    rec = m.component_records(cap * 512); rec.fill_(SENTINEL)
    thr = torch.zeros(Q, device="cuda")
    out = m.segment_features(q, "cosine", 1.0, thr, 26, 2, out=(idx, lab, sc, ids, bc, rec, cc))
    assert out[0] is idx and out[5] is rec and len(out) == 7
    assert int(bc.item()) == n
    for t in (idx, lab, sc, ids):
        assert (t[n:] == SENTINEL).all()                            # behind the block count nothing is written
    lab_n, sc_n, ids_n = lab[:n].cpu().numpy(), sc[:n].cpu().numpy(), ids[:n].cpu().numpy()
    assert ((lab_n >= 0) | (sc_n == 0)).all() and (sc_n[lab_n >= 0] >= 0).all()
    _assert_equals_model(idx[:n].cpu().numpy(), lab_n, sc_n, 26, 2, ids_n, _records(rec), int(cc.item()))

    def call(conn=6, mv=1, nq=Q, metric=1, idx_=idx, lab_=lab, sc_=sc, ids_=ids, bc_=bc, rec_=rec, ccap=cap * 512, cc_=cc, bcap=cap, q_=q):
        return _raw(m, lambda: m.lib.nvbx_segment_features(m._h, P(q_), nq, metric, 1.0, P(thr), conn, mv, P(idx_), P(lab_), P(sc_), P(ids_), bcap, P(bc_),
                                                            P(rec_), ccap, P(cc_)))

    def fine():
        bc.fill_(SENTINEL)
        assert call() == 0 and int(bc.item()) == n
    fine()
    for bad in (dict(conn=7), dict(mv=0), dict(nq=0), dict(nq=129), dict(metric=2), dict(q_=None), dict(idx_=None), dict(lab_=None), dict(sc_=None),
                dict(ids_=None), dict(bc_=None), dict(cc_=None), dict(rec_=None), dict(bcap=-1), dict(bcap=(1 << 22) + 1), dict(ccap=-1)):
        assert call(**bad) == -1, bad
        assert m.lib.nvbx_last_error()
        fine()
    cc.fill_(SENTINEL); bc.fill_(SENTINEL)
    assert call(idx_=None, lab_=None, sc_=None, ids_=None, rec_=None, ccap=0, bcap=0) == 0      # capacity 0: the block count, and no components
    assert int(bc.item()) == n and int(cc.item()) == 0
    e = M.Mapper(M.default_params(), block_capacity=256)                                        # before enable_features
    with pytest.raises(M.NvbxError):
        e.segment_features(q, "cosine")
    e.close()
