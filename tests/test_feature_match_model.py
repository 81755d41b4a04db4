"""The feature-matching model (tests/feature_match_independent.py) on hand-made cases whose answer is known in closed form.  No GPU."""
import numpy as np

import feature_match_independent as FM

H = np.float16


def block(C, seed=0):
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((1, 512, C)).astype(H)
    w = np.ones((1, 512), np.float32)
    return f, w


def test_one_hot_queries_read_the_channels_back():
    f, w = block(24)
    q = np.eye(24, dtype=H)
    lab, best, s = FM.match(f, w, q, FM.DOT, 1.0)
    assert np.array_equal(s, f.astype(np.float64))
    assert np.array_equal(lab, np.argmax(f.astype(np.float64), -1))
    assert np.array_equal(best, f.astype(np.float64).max(-1))
    assert (FM.bound(f, q, FM.DOT) >= 0).all()


def test_cosine_of_orthogonal_parallel_and_opposite_vectors():
    f = np.zeros((4, 8), H)
    f[0, 0] = 3.0                      # along e0
    f[1, 1] = 0.5                      # along e1
    f[2, :2] = (2.0, 2.0)              # the diagonal
    f[3, 0] = -7.0                     # against e0
    q = np.zeros((2, 8), H)
    q[0, 0] = 5.0; q[1, :2] = (1.0, 1.0)
    s = FM.scores(f, q, FM.COSINE)
    r = np.sqrt(0.5)
    assert np.allclose(s, [[1.0, r], [0.0, r], [r, 1.0], [-1.0, -r]], atol=1e-15)
    assert np.array_equal(FM.scores(f, q, FM.DOT), [[15.0, 3.0], [0.0, 0.5], [10.0, 4.0], [-35.0, -7.0]])


def test_a_zero_norm_scores_zero():
    f = np.zeros((2, 8), H); f[1, 3] = 1.0
    q = np.zeros((2, 8), H); q[1, 3] = 2.0
    s = FM.scores(f, q, FM.COSINE)
    assert np.array_equal(s, [[0.0, 0.0], [0.0, 1.0]]) and np.isfinite(s).all()
    # a voxel that counts, all of whose scores are 0: the tie goes to query 0
    lab, best, _ = FM.match(f[None], np.ones((1, 2), np.float32), q, FM.COSINE, 1.0)
    assert lab.tolist() == [[0, 1]] and best.tolist() == [[0.0, 1.0]]


def test_a_tie_goes_to_the_lowest_query_index():
    f = np.ones((1, 1, 8), H)
    q = np.zeros((4, 8), H)
    q[0, 0] = 1.0; q[1, 1] = 2.0; q[2, 2] = 2.0; q[3, 3] = 2.0
    lab, best, s = FM.match(f, np.ones((1, 1), np.float32), q, FM.DOT, 1.0)
    assert s.tolist() == [[[1.0, 2.0, 2.0, 2.0]]] and lab.tolist() == [[1]] and best.tolist() == [[2.0]]


def test_min_weight_and_label_minus_one():
    f, _ = block(8, seed=3)
    w = np.zeros((1, 512), np.float32)
    w[0, :100] = 1.0; w[0, 100:200] = 2.0; w[0, 200:300] = 0.5
    q = np.random.default_rng(4).standard_normal((5, 8)).astype(H)
    for mw, n in ((0.0, 300), (0.5, 300), (1.0, 200), (2.0, 100), (3.0, 0)):
        lab, best, s = FM.match(f, w, q, FM.DOT, mw)
        cnt = FM.counts(w, mw)
        assert cnt.sum() == n
        assert (lab[~cnt] == -1).all() and (best[~cnt] == 0).all() and (s[~cnt] == 0).all()
        assert ((lab[cnt] >= 0) & (lab[cnt] < 5)).all()
    assert not FM.counts(np.zeros(3, np.float32), 0.0).any() and not FM.counts(np.zeros(3, np.float32), -1.0).any()      # weight 0 never counts


def test_the_bound_covers_float32_summation_in_any_order_and_dropped_subnormals():
    rng = np.random.default_rng(5)
    C = 64
    f = rng.standard_normal((256, C)).astype(H)
    f[:, 5] = H(3e-6)                                       # an fp16 subnormal in every vector
    q = rng.standard_normal((7, C)).astype(H)
    assert FM.is_subnormal(f).sum() >= 256
    ref = FM.scores(f, q, FM.DOT); b = FM.bound(f, q, FM.DOT)
    f32, q32 = f.astype(np.float32), q.astype(np.float32)
    for order in (np.arange(C), np.arange(C)[::-1], rng.permutation(C)):
        acc = np.zeros((256, 7), np.float32)
        for c in order:
            acc = (acc + f32[:, c, None] * q32[None, :, c]).astype(np.float32)
        assert (np.abs(acc - ref) <= b).all()
    f0 = f.copy(); f0[FM.is_subnormal(f)] = 0
    assert (np.abs(FM.scores(f0, q, FM.DOT) - ref) <= b).all()
    assert (FM.bound(f, q, FM.COSINE) == (C + 16) * 2.0 ** -23).all()
