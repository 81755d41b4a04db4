"""An independent float64 model of feature matching (SEMANTICS.md "Feature matching"): both metrics, the counting rule, the tie rule, label -1,
and the per-voxel error bound a float32 implementation has to keep.  Its input is the public block layout (what feature_blocks returns:
features [n, 512, C] float16, weights [n, 512] float32); it imports nothing from the product or the oracle."""
import numpy as np

DOT, COSINE = "dot", "cosine"
F16_MIN_NORMAL = 2.0 ** -14
ULP32 = 2.0 ** -23


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float16, a.dtype
    return a.astype(np.float64)


def scores(f, q, metric):
    """f [..., C] float16, q [Q, C] float16 -> [..., Q] float64.  dot: sum_c f_c q_c; cosine: dot / sqrt(|f|^2 |q|^2), 0 where either norm is 0."""
    f64, q64 = _f64(f), _f64(q)
    assert q64.ndim == 2 and f64.shape[-1] == q64.shape[1]
    d = f64 @ q64.T
    if metric == DOT:
        return d
    assert metric == COSINE, metric
    nf = (f64 * f64).sum(-1)[..., None]
    nq = (q64 * q64).sum(-1)
    den = np.sqrt(nf * nq)
    out = np.zeros_like(d)
    np.divide(d, den, out=out, where=den > 0)
    return out


def counts(w, min_weight):
    """A voxel counts when its weight is above 0 and at least min_weight."""
    w = np.asarray(w)
    return (w > 0) & (w >= min_weight)


def labels_of(s, cnt):
    """The query with the highest score, the lowest index on a tie (numpy's argmax returns the first maximum); -1 where the voxel does not count."""
    return np.where(cnt, np.argmax(s, axis=-1), -1).astype(np.int32)


def match(f, w, q, metric, min_weight):
    """-> (labels [...] int32, score [...] float64, all [..., Q] float64); a voxel that does not count: label -1, score 0, all scores 0."""
    cnt = counts(w, min_weight)
    s = np.where(cnt[..., None], scores(f, q, metric), 0.0)
    lab = labels_of(s, cnt)
    best = np.where(cnt, np.take_along_axis(s, np.maximum(lab, 0)[..., None].astype(np.int64), -1)[..., 0], 0.0)
    return lab, best, s


def is_subnormal(a):
    a = np.abs(_f64(a))
    return (a > 0) & (a < F16_MIN_NORMAL)


def bound(f, q, metric):
    """[..., Q] float64: how far a float32 implementation may be from scores().
    The fp16 products are exact in float32; at most C additions are each off by at most one float32 ulp of a partial sum, and every partial sum is
    bounded by sum_c |f_c q_c|.  Hardware may take an fp16 subnormal operand as 0: those products may be missing altogether.
      dot:    C 2^-23 sum_c |f_c q_c| + sum_{c: f_c or q_c subnormal} |f_c q_c|
      cosine: (C + 16) 2^-23 -- by Cauchy-Schwarz the dot bound over the norms is at most C 2^-23; 16 covers the two norm sums, the root, the division."""
    f64, q64 = np.abs(_f64(f)), np.abs(_f64(q))
    C = q64.shape[1]
    if metric == COSINE:
        return np.full(f64.shape[:-1] + (q64.shape[0],), (C + 16) * ULP32)
    assert metric == DOT, metric
    fs, qs = is_subnormal(f), is_subnormal(q)
    # sum over subnormal pairs: |f| on f's subnormals against all |q|, plus |f| elsewhere against q's subnormals
    sub = (f64 * fs) @ q64.T + (f64 * ~fs) @ (q64 * qs).T
    return C * ULP32 * (f64 @ q64.T) + sub
