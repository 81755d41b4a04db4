"""Feature matching on the GPU (feature_match.hip; SEMANTICS.md "Feature matching") against the float64 model of tests/feature_match_independent.py.
The expected values are computed from what feature_blocks returns: the stored fp16 values are the truth, the integration rounding is not under test.
One-hot queries check the matrix instruction's lane map exactly; random queries are held to the derived float32 error bounds."""
import ctypes as C

import numpy as np
import pytest

import feature_match_independent as FM
import helpers as H

pytestmark = pytest.mark.gpu

CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
VS = 0.05
STRIDE = 4
T512 = np.arange(512)
OFF = np.stack([T512 >> 6, (T512 >> 3) & 7, T512 & 7], 1)      # voxel t = vx 64 + vy 8 + vz


def _mods():
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    return M, S


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


def _feature_image(rng, C, positive=False):
    f = rng.standard_normal((CAM[5] // STRIDE, CAM[4] // STRIDE, C)).astype(np.float16)
    return np.abs(f) if positive else f


def _read_layer(M, m):
    idx = m.block_indices(M.LAYER_FEATURE)
    f, w, found = m.feature_blocks(idx)
    assert found.all()
    return idx, f, w


@pytest.fixture(scope="module")
def maps(room_frames):
    """(C, positive) -> a mapper with three overlapping feature frames and what feature_blocks returns of it; built once, left unchanged"""
    M, _ = _mods()
    cache = {}

    def get(C, positive=False):
        key = (C, positive)
        if key not in cache:
            m = M.Mapper(M.default_params(), block_capacity=1 << 12)
            for d, _, T in room_frames:
                m.integrate_depth(d, T, CAM)
            m.enable_features(C)
            rng = np.random.default_rng(1000 + C)
            for _, _, T in room_frames:
                m.integrate_features(_feature_image(rng, C, positive), T, CAM, STRIDE)
            idx, f, w = _read_layer(M, m)
            assert len(idx) > 50 and (w == 3).any() and (w == 1).any()
            cache[key] = dict(m=m, idx=idx, f=f, w=w, ref={})
        return cache[key]
    yield get
    for v in cache.values():
        v["m"].close()


def _order(returned_idx, idx):
    """positions in `idx` of the returned entries; the returned set is exactly `idx`, each index once"""
    where = {tuple(b): i for i, b in enumerate(np.asarray(idx).tolist())}
    got = [tuple(b) for b in np.asarray(returned_idx).tolist()]
    assert len(got) == len(set(got)) == len(where) and set(got) == set(where)
    return np.array([where[g] for g in got], np.int64)


def _np(*ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def _queries(C, Q, seed=0, negative=False):
    q = np.random.default_rng(77 * C + Q + seed).standard_normal((Q, C)).astype(np.float16)
    return -np.abs(q) - np.float16(0.01) if negative else q


def _assert_uncounted_are_blank(cnt, lab, sc, al):
    assert (lab[~cnt] == -1).all() and (sc[~cnt] == 0).all()
    if al is not None:
        assert (al[~cnt] == 0).all()


def _assert_one_hot_exact(M, m, C, min_weight=1.0):
    """Query q is one-hot at channel q, dot metric: every score equals the stored value as a float (-0 == +0); a stored fp16 subnormal may come
    back as itself or as 0.  -> (subnormals compared, how many of them came back as 0)"""
    idx, f, w = _read_layer(M, m)
    ri, lab, sc, al = _np(*m.match_features(np.eye(C, dtype=np.float16), "dot", min_weight, all_scores=True))
    perm = _order(ri, idx)
    f, w = f[perm], w[perm]
    cnt = FM.counts(w, min_weight)
    assert cnt.sum() > 1000
    exp = f.astype(np.float32)
    sub = FM.is_subnormal(f) & cnt[..., None]
    good = (al == exp) | (sub & (al == 0))
    assert good[cnt].all(), "%d of %d scores differ from the stored value" % (int((~good[cnt]).sum()), good[cnt].size)
    assert sub.sum() < 1e-3 * cnt.sum() * C
    _assert_uncounted_are_blank(cnt, lab, sc, al)
    assert np.array_equal(lab[cnt], np.argmax(al[cnt], -1))                 # the tie rule, on these exact scores
    assert np.array_equal(sc[cnt].view(np.uint32), np.take_along_axis(al[cnt], lab[cnt][:, None].astype(np.int64), -1)[:, 0].view(np.uint32))
    return int(sub.sum()), int((sub & (al == 0) & (exp != 0)).sum())


# ---- 1. the lane map, exactly
@pytest.mark.parametrize("C", [8, 24, 64])
def test_one_hot_queries_return_the_stored_values_exactly(maps, C):
    M, _ = _mods()
    n_sub, n_zero = _assert_one_hot_exact(M, maps(C)["m"], C)
    print("C = %d: %d stored fp16 subnormals among the compared values, %d of them scored 0" % (C, n_sub, n_zero))


# ---- 2. random queries against float64
def _reference(mp, C, Q, metric):
    key = (Q, metric)
    if key not in mp["ref"]:
        q = _queries(C, Q)
        mp["ref"][key] = (q, FM.scores(mp["f"], q, metric), FM.bound(mp["f"], q, metric))
    return mp["ref"][key]


def _assert_within_bounds(s64, bnd, cnt, Q, lab, sc, al, what):
    err = np.abs(al.astype(np.float64) - s64)
    if not cnt.any():
        return
    print("%s: max error / bound = %.3g over %d scores" % (what, float((err[cnt] / np.maximum(bnd[cnt], 1e-300)).max()), err[cnt].size))
    assert (err[cnt] <= bnd[cnt]).all(), "%s: %d scores outside the bound, worst %.3g x" % (what, int((err[cnt] > bnd[cnt]).sum()), float((err[cnt] / bnd[cnt]).max()))
    if lab is None:
        return
    _assert_uncounted_are_blank(cnt, lab, sc, al)
    L = lab[cnt].astype(np.int64)
    assert ((L >= 0) & (L < Q)).all()
    best = np.argmax(s64[cnt], -1)
    s_l = np.take_along_axis(s64[cnt], L[:, None], -1)[:, 0]; s_b = np.take_along_axis(s64[cnt], best[:, None], -1)[:, 0]
    b_l = np.take_along_axis(bnd[cnt], L[:, None], -1)[:, 0]; b_b = np.take_along_axis(bnd[cnt], best[:, None], -1)[:, 0]
    assert (s_l >= s_b - (b_l + b_b)).all(), what            # (b_l + b_b <= 2 max bound)
    assert np.array_equal(sc[cnt].view(np.uint32), np.take_along_axis(al[cnt], L[:, None], -1)[:, 0].view(np.uint32)), what


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("C,Q", [(8, 1), (24, 5), (40, 33), (64, 128)])
def test_random_queries_stay_within_the_float32_bound(maps, C, Q, metric, min_weight):
    mp = maps(C)
    q, s64, bnd = _reference(mp, C, Q, metric)
    ri, lab, sc, al = _np(*mp["m"].match_features(q, metric, min_weight, all_scores=True))
    perm = _order(ri, mp["idx"])
    w = mp["w"][perm]
    cnt = FM.counts(w, min_weight)
    if min_weight == 2.0:
        assert ((w > 0) & ~cnt).sum() > 100 and cnt.sum() > 100        # some voxels are masked by 2, some are not
    else:
        assert np.array_equal(cnt, w > 0)
    _assert_within_bounds(s64[perm], bnd[perm], cnt, Q, lab, sc, al, "C %d Q %d %s" % (C, Q, metric))
    # without the score matrix: the same labels and scores
    ri2, lab2, sc2, none = _np(*mp["m"].match_features(q, metric, min_weight))
    assert none is None
    back = np.argsort(_order(ri2, mp["idx"]))[perm]
    assert np.array_equal(lab2[back], lab) and np.array_equal(sc2[back].view(np.uint32), sc.view(np.uint32))


# ---- 3. padding never wins
@pytest.mark.parametrize("metric", ["dot", "cosine"])
@pytest.mark.parametrize("Q", [1, 33])
def test_padding_rows_never_win(maps, Q, metric):
    mp = maps(8, positive=True)
    assert (mp["f"] >= 0).all()
    q = _queries(8, Q, negative=True)
    assert (q < 0).all()
    ri, lab, sc, al = _np(*mp["m"].match_features(q, metric, 1.0, all_scores=True))
    cnt = mp["w"][_order(ri, mp["idx"])] > 0
    assert cnt.sum() > 1000
    assert ((lab[cnt] >= 0) & (lab[cnt] < Q)).all() and (sc[cnt] < 0).all() and (al[cnt] < 0).all() and al.shape[-1] == Q
    _assert_uncounted_are_blank(cnt, lab, sc, al)


# ---- 4. points
def _special_points(M, mp):
    m = mp["m"]
    feat = {tuple(b) for b in mp["idx"].tolist()}
    bare = [b for b in m.block_indices(M.LAYER_TSDF).tolist() if tuple(b) not in feat]
    assert bare, "the map has no TSDF block without features"
    return np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [1e9, 0.0, 0.0], (np.array(bare[0]) * 8 + 3.5) * VS], np.float32)


def _points(M, mp, n, rng):
    """voxel centres drawn from feature blocks (half of them from voxels that hold features), and among them the four special points"""
    bi, ti = np.nonzero(mp["w"] > 0)
    k = rng.integers(0, len(bi), n)
    b, t = bi[k], ti[k]
    anyw = rng.random(n) < 0.5
    b = np.where(anyw, rng.integers(0, len(mp["idx"]), n), b); t = np.where(anyw, rng.integers(0, 512, n), t)
    pts = ((mp["idx"][b].astype(np.float64) * 8 + OFF[t] + 0.5) * VS).astype(np.float32)
    src = np.stack([b, t], 1)
    if n >= 4:
        at = rng.choice(n, 4, replace=False)
        pts[at] = _special_points(M, mp); src[at] = -1
    return pts, src


def _assert_points(M, mp, C, pts, src, q, metric, exact):
    m = mp["m"]
    s, wts = _np(*m.match_points(pts, q, metric))
    _, qw = _np(*m.query_features(pts))
    assert s.shape == (len(pts), len(q)) and np.array_equal(wts.view(np.uint32), qw.view(np.uint32))
    assert (s[wts == 0] == 0).all()
    real = src[:, 0] >= 0
    assert (wts[~real] == 0).all()
    f = mp["f"][src[real, 0], src[real, 1]]; w = mp["w"][src[real, 0], src[real, 1]]
    assert np.array_equal(wts[real], w)
    cnt = w > 0
    if exact:
        exp = f.astype(np.float32)
        sub = FM.is_subnormal(f)
        assert ((s[real] == exp) | (sub & (s[real] == 0)))[cnt].all()
    else:
        _assert_within_bounds(FM.scores(f, q, metric), FM.bound(f, q, metric), cnt, len(q), None, None, s[real], "points %d %s" % (len(pts), metric))
    return int(cnt.sum())


@pytest.mark.parametrize("n", [1, 63, 1000])
def test_points_score_as_their_voxels(maps, n):
    M, _ = _mods()
    C = 24
    mp = maps(C)
    rng = np.random.default_rng(40 + n)
    if n == 1:        # one point of every kind, one call each
        bi, ti = np.nonzero(mp["w"] > 0)
        centre = ((mp["idx"][bi[7]].astype(np.float64) * 8 + OFF[ti[7]] + 0.5) * VS).astype(np.float32)[None]
        cases = [(centre, np.array([[bi[7], ti[7]]]))] + [(p[None], np.array([[-1, -1]])) for p in _special_points(M, mp)]
    else:
        cases = [_points(M, mp, n, rng)]
    hits = 0
    for pts, src in cases:
        assert len(pts) == n
        hits += _assert_points(M, mp, C, pts, src, np.eye(C, dtype=np.float16), "dot", True)
        for metric in ("dot", "cosine"):
            _assert_points(M, mp, C, pts, src, _queries(C, 5), metric, False)
        _assert_points(M, mp, C, pts, src, _queries(C, 33), "cosine", False)
    assert hits >= min(n, 20) // 2
    s, w = mp["m"].match_points(np.zeros((0, 3), np.float32), _queries(C, 5))          # n == 0 launches nothing
    assert tuple(s.shape) == (0, 5) and tuple(w.shape) == (0,)


# ---- 5. capacity
def test_capacity_below_the_block_count_counts_all_and_writes_no_further(maps):
    import torch
    M, _ = _mods()
    C, Q = 24, 5
    mp = maps(C)
    m = mp["m"]
    n = len(mp["idx"]); half = n // 2
    q = _queries(C, Q)
    idx = torch.full((n, 3), -77, dtype=torch.int32, device="cuda"); lab = torch.full((n, 512), -77, dtype=torch.int32, device="cuda")
    sc = torch.full((n, 512), -77.0, device="cuda"); al = torch.full((n, 512, Q), -77.0, device="cuda")
    cnt = torch.full((1,), -77, dtype=torch.int64, device="cuda")
    out = m.match_features(q, "dot", 1.0, out=(idx[:half], lab[:half], sc[:half], al[:half], cnt))
    assert len(out) == 5 and out[4] is cnt
    assert int(cnt.item()) == n                                                   # the full number
    for t in (idx, lab, sc, al):
        assert (t[half:] == -77).all()                                            # the sentinel-filled tail behind every output buffer is untouched
    ri, lb, s, a = _np(idx[:half], lab[:half], sc[:half], al[:half])
    where = {tuple(b): i for i, b in enumerate(mp["idx"].tolist())}
    got = [tuple(b) for b in ri.tolist()]
    assert len(set(got)) == half and set(got) <= set(where)                       # distinct, members of the layer
    perm = np.array([where[g] for g in got])
    _, s64, bnd = _reference(mp, C, Q, "dot")
    _assert_within_bounds(s64[perm], bnd[perm], mp["w"][perm] > 0, Q, lb, s, a, "first half")
    # capacity 0 with NULL outputs: the count alone
    qd = torch.from_numpy(q).cuda()
    cnt.fill_(-77)
    rc = m.lib.nvbx_match_features(m._h, C_ptr(qd), Q, 0, 1.0, None, None, None, None, 0, C_ptr(cnt))
    assert rc == 0 and int(cnt.item()) == n
    # features enabled, nothing integrated: count 0
    e = M.Mapper(M.default_params(), block_capacity=256)
    e.enable_features(C)
    r = e.match_features(q, "dot", 1.0, all_scores=True)
    assert tuple(r[0].shape) == (0, 3) and tuple(r[1].shape) == (0, 512) and tuple(r[3].shape) == (0, 512, Q)
    cnt.fill_(-77)
    assert e.match_features(q, "dot", 1.0, out=(idx, lab, sc, None, cnt))[4] is cnt and int(cnt.item()) == 0
    e.close()


def C_ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- 6. the map is untouched
def test_matching_leaves_the_map_bit_identical(room_frames):
    M, _ = _mods()
    Cn = 16
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.set_color_deferral(False)
    m.enable_features(Cn)
    rng = np.random.default_rng(6)
    for d, rgb, T in room_frames:
        m.integrate_depth(d, T, CAM); m.integrate_color(rgb, T, CAM)
        m.integrate_features(_feature_image(rng, Cn), T, CAM, STRIDE)

    layers = (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF, M.LAYER_FEATURE)
    before = H.map_state(m, layers), m.block_indices(M.LAYER_MESH), m.counters()
    q = _queries(Cn, 33)
    for metric in ("dot", "cosine"):
        m.match_features(q, metric, 1.0, all_scores=True)
        m.match_points(rng.uniform(-3, 3, (500, 3)).astype(np.float32), q, metric)
    H.assert_same_map(before[0], m, "before and after the calls", min_blocks={M.LAYER_TSDF: 101, M.LAYER_COLOR: 51, M.LAYER_FEATURE: 51})
    assert np.array_equal(before[1], m.block_indices(M.LAYER_MESH)) and before[2] == m.counters()
    m.close()


# ---- 7. lifetime and growth
def test_the_scan_follows_removed_blocks_reused_slots_and_grown_pools():
    M, S = _mods()
    sc = S.Scene()
    C8 = 8
    m = M.Mapper(M.default_params(), block_capacity=1 << 9, max_block_capacity=1 << 13)
    m.enable_features(C8)
    rng = np.random.default_rng(8)
    caps = [m.capacity]

    def frame(k):
        T = S.trajectory_pose(k)
        d, _ = S.render(sc, T, CAM)
        m.integrate_depth(d, T, CAM)
        m.integrate_features(_feature_image(rng, C8), T, CAM, STRIDE)
        caps.append(m.capacity)
    for k in (0, 25, 50):
        frame(k)
    n0 = m.num_blocks(M.LAYER_FEATURE)
    _assert_one_hot_exact(M, m, C8)
    centres = (m.block_indices(M.LAYER_FEATURE).astype(np.float64) + 0.5) * 8 * VS
    mid = centres.mean(0)
    m.clear_outside_radius(tuple(mid), float(np.median(np.linalg.norm(centres - mid, axis=1))))      # removes part of the map
    n1 = m.num_blocks(M.LAYER_FEATURE)
    assert 0 < n1 < n0
    _assert_one_hot_exact(M, m, C8)                                                     # (lists exactly block_indices(LAYER_FEATURE), each once)
    for k in (75, 100, 125):                                                            # freed slots are reused, and the pools grow
        frame(k)
    assert m.num_blocks(M.LAYER_FEATURE) > n1 and caps[-1] > caps[0], caps
    _assert_one_hot_exact(M, m, C8)
    m.close()


# ---- 8. refusals
def test_refusals_leave_the_mapper_usable(room_frames):
    import torch
    M, _ = _mods()
    C8, Q = 8, 5
    d, _, T = room_frames[0]
    m = M.Mapper(M.default_params(), block_capacity=1 << 12)
    m.integrate_depth(d, T, CAM)
    qh = np.zeros((130, C8), np.float16); qh[:Q] = _queries(C8, Q)
    qd = torch.from_numpy(qh).cuda()
    pts = torch.zeros((4, 3), device="cuda"); s4 = torch.zeros((4, Q), device="cuda"); w4 = torch.zeros(4, device="cuda")
    CAP = 1 << 12
    idx = torch.zeros((CAP, 3), dtype=torch.int32, device="cuda"); lab = torch.zeros((CAP, 512), dtype=torch.int32, device="cuda")
    sc = torch.zeros((CAP, 512), device="cuda"); cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = C_ptr

    def feats(q=None, nq=Q, metric=1, idx_=idx, lab_=lab, sc_=sc, cnt_=cnt, cap=1 << 12):
        return m.lib.nvbx_match_features(m._h, P(qd) if q is None else q, nq, metric, 1.0, P(idx_) if idx_ is not None else None, P(lab_) if lab_ is not None else None,
                                         P(sc_) if sc_ is not None else None, None, cap, P(cnt_) if cnt_ is not None else None)

    def points(q=None, nq=Q, metric=1, s_=s4, w_=w4, p_=pts, n=4):
        return m.lib.nvbx_match_points(m._h, P(p_) if p_ is not None else None, n, P(qd) if q is None else q, nq, metric, P(s_) if s_ is not None else None,
                                       P(w_) if w_ is not None else None)
    INVALID = -1
    assert feats() == INVALID and points() == INVALID                          # before nvbx_enable_features
    assert b"nvbx_enable_features" in m.lib.nvbx_last_error()
    with pytest.raises(M.NvbxError):
        m.match_features(qh[:Q])
    with pytest.raises(M.NvbxError):
        m.match_points(np.zeros((4, 3), np.float32), qh[:Q])
    m.enable_features(C8)
    m.integrate_features(np.ones((15, 20, C8), np.float16), T, CAM, STRIDE)
    n = m.num_blocks(M.LAYER_FEATURE)
    assert 0 < n <= CAP

    def fine():
        cnt.zero_()
        assert feats() == 0 and points() == 0
        assert int(cnt.item()) == n
    fine()
    misaligned = C.c_void_p(qd.data_ptr() + 2)
    for bad in (dict(nq=0), dict(nq=129), dict(nq=-1), dict(metric=2), dict(metric=-1), dict(q=C.c_void_p(None)), dict(q=misaligned)):
        assert feats(**bad) == INVALID, bad
        assert m.lib.nvbx_last_error()
        fine()
        assert points(**bad) == INVALID, bad
        fine()
    for bad in (dict(idx_=None), dict(lab_=None), dict(sc_=None), dict(cnt_=None), dict(cnt_=None, cap=0), dict(cap=-1)):
        assert feats(**bad) == INVALID, bad
        fine()
    for bad in (dict(s_=None), dict(w_=None), dict(p_=None), dict(n=-1)):
        assert points(**bad) == INVALID, bad
        fine()
    assert points(s_=None, w_=None, p_=None, n=0) == 0                         # n == 0: nothing is required
    with pytest.raises(ValueError):
        m.match_features(qh[:Q], metric="l2")
    with pytest.raises(M.NvbxError):
        m.match_features(np.zeros((Q, 16), np.float16))                        # channel count
    r = m.match_features(qh[:Q])
    assert len(r[0]) == n
    m.close()
