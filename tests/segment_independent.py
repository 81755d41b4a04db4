"""An independent model of feature segmentation (SEMANTICS.md "Feature segmentation"): connected components of a labelled sparse voxel volume
with their records, by scipy.ndimage.label on a dense volume, cross-checked by a scipy-free union-find in numpy; the threshold rule of
segment_features; the canonical form in which a result is compared (the index order of the components is unspecified); and the drawn volumes
the tests share.  It imports nothing from the product or the oracle."""
import numpy as np

T512 = np.arange(512)
OFF = np.stack([T512 >> 6, (T512 >> 3) & 7, T512 & 7], 1)      # voxel t = vx 64 + vy 8 + vz

# nvbx_component as the header lays it out (72 bytes; offsets 0 4 8 20 32 56 60)
COMPONENT_DT = np.dtype({"names": ["label", "voxels", "min_xyz", "max_xyz", "sum_xyz", "peak_score", "peak_xyz"],
                         "formats": ["<i4", "<i4", ("<i4", (3,)), ("<i4", (3,)), ("<i8", (3,)), "<f4", ("<i4", (3,))],
                         "offsets": [0, 4, 8, 20, 32, 56, 60], "itemsize": 72})


def threshold(label, score, min_score):
    """segment_features' threshold in float32: where score < min_score[label] the voxel becomes background (label -1, score 0).
    A voxel AT its threshold stays; a NaN threshold drops nothing."""
    label = np.asarray(label, np.int32); score = np.asarray(score, np.float32)
    thr = np.asarray(min_score, np.float32)[np.maximum(label, 0)]
    drop = (label >= 0) & (score < thr)
    return np.where(drop, -1, label).astype(np.int32), np.where(drop, np.float32(0), score).astype(np.float32)


def _order_scores(score):
    """the order the peaks are taken in: floats, -0 as +0, a NaN as -infinity"""
    s = np.asarray(score, np.float32).copy()
    s[np.isnan(s)] = -np.inf
    return s + np.float32(0)


class Dense:
    """the blocks of a list scattered into a dense volume over their bounding box; an absent block is background"""

    def __init__(self, block_idx, label, score=None):
        self.bidx = np.asarray(block_idx, np.int64).reshape(-1, 3)
        n = len(self.bidx)
        assert len({tuple(b) for b in self.bidx.tolist()}) == n, "block indices must be distinct"
        self.lab = np.asarray(label, np.int32).reshape(n, 512)
        self.sc = _order_scores(np.zeros((n, 512), np.float32) if score is None else np.asarray(score, np.float32).reshape(n, 512))
        self.lo = self.bidx.min(0) * 8 if n else np.zeros(3, np.int64)
        self.shape = tuple(((self.bidx.max(0) + 1) * 8 - self.lo).tolist()) if n else (0, 0, 0)
        # global voxel coordinates of every listed voxel [n, 512, 3], their positions in the box and the linear (= lexicographic) index
        self.g = self.bidx[:, None, :] * 8 + OFF[None]
        self.pos = self.g - self.lo
        self.lin = np.ravel_multi_index(tuple(self.pos[..., k] for k in range(3)), self.shape) if n else np.zeros((0, 512), np.int64)
        self.L = np.full(self.shape, -1, np.int32); self.S = np.zeros(self.shape, np.float32)
        if n:
            self.L.ravel()[self.lin] = np.where(self.lab >= 0, self.lab, -1); self.S.ravel()[self.lin] = self.sc

    def voxel_of(self, lin):
        return tuple((np.array(np.unravel_index(int(lin), self.shape)) + self.lo).tolist())


def _records(d, roots_dense, min_voxels):
    """roots_dense: per voxel of the box the linear index of its component's lowest voxel, -1 for background
    -> (components: {lowest global voxel: (label, voxels, min, max, sum, peak_score, peak_xyz)}, keys [n, 512]: that lowest voxel's linear index per
    listed voxel, -1 for background and for components below min_voxels)"""
    flat = roots_dense.ravel()
    where = np.flatnonzero(flat >= 0)                    # rising linear index = lexicographic order
    comps = {}
    keep = np.zeros(flat.size + 1, bool)
    if where.size:
        order = np.argsort(flat[where], kind="stable")
        w = where[order]; r = flat[w]
        starts = np.flatnonzero(np.r_[True, r[1:] != r[:-1]]); ends = np.r_[starts[1:], len(r)]
        S = d.S.ravel(); L = d.L.ravel()
        for s, e in zip(starts, ends):
            if e - s < min_voxels:
                continue
            vox = w[s:e]                                   # rising
            assert vox[0] == r[s]
            xyz = np.stack(np.unravel_index(vox, d.shape), 1) + d.lo
            sc = S[vox]
            p = int(np.argmax(sc))                         # the first maximum: the lexicographically lowest voxel of the best score
            keep[r[s]] = True
            comps[tuple(xyz[0].tolist())] = (int(L[vox[0]]), int(e - s), tuple(xyz.min(0).tolist()), tuple(xyz.max(0).tolist()),
                                             tuple(int(v) for v in xyz.sum(0)), np.float32(sc[p]).view(np.uint32).item(), tuple(xyz[p].tolist()))
    roots_listed = flat[d.lin] if len(d.bidx) else np.zeros((0, 512), np.int64)
    keys = np.where(keep[roots_listed], roots_listed, -1)
    return comps, keys


def model(block_idx, label, score, connectivity, min_voxels=1):
    """scipy.ndimage.label per distinct label on the dense volume -> (components, keys), see _records"""
    from scipy import ndimage
    assert connectivity in (6, 26)
    d = Dense(block_idx, label, score)
    st = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    roots = np.full(d.shape, -1, np.int64)
    lin_all = np.arange(int(np.prod(d.shape)), dtype=np.int64).reshape(d.shape)
    for lab in np.unique(d.L[d.L >= 0]):
        cc, k = ndimage.label(d.L == lab, structure=st)
        if k:
            low = ndimage.minimum(lin_all, cc, np.arange(1, k + 1)).astype(np.int64)
            m = cc > 0
            roots[m] = low[cc[m] - 1]
    return _records(d, roots, min_voxels)


def model_union_find(block_idx, label, score, connectivity, min_voxels=1):
    """the same result without scipy: minimum propagation along the equal-label edges of the voxel grid with pointer jumping, until quiet"""
    assert connectivity in (6, 26)
    d = Dense(block_idx, label, score)
    size = int(np.prod(d.shape))
    parent = np.where(d.L.ravel() >= 0, np.arange(size, dtype=np.int64), -1)
    offs = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
            if (dx, dy, dz) > (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1)]
    assert len(offs) == (13 if connectivity == 26 else 3)
    ea, eb = [], []
    lin = np.arange(size, dtype=np.int64).reshape(d.shape) if size else np.zeros(d.shape, np.int64)
    for o in offs:
        sa = tuple(slice(max(0, -k), d.shape[i] - max(0, k)) for i, k in enumerate(o))
        sb = tuple(slice(max(0, k), d.shape[i] - max(0, -k)) for i, k in enumerate(o))
        same = (d.L[sa] == d.L[sb]) & (d.L[sa] >= 0)
        ea.append(lin[sa][same]); eb.append(lin[sb][same])
    ea = np.concatenate(ea) if ea else np.zeros(0, np.int64); eb = np.concatenate(eb) if eb else np.zeros(0, np.int64)
    for _ in range(size + 1):
        before = parent.copy()
        m = np.minimum(parent[ea], parent[eb])
        np.minimum.at(parent, ea, m); np.minimum.at(parent, eb, m)
        fg = parent >= 0
        parent[fg] = parent[parent[fg]]
        if np.array_equal(parent, before):
            break
    else:
        raise AssertionError("no fixed point")
    return _records(d, parent.reshape(d.shape), min_voxels)


def canonical(block_idx, label, ids, records, count):
    """What a product call returned, in the model's form.  ids [n, 512] int32, records: COMPONENT_DT array of at least min(count, its length)
    rows.  Checks on the way: ids lie in [-1, count), every index below count is used, and the ids of one component share one label.
    -> (components of the records that exist, keys [n, 512])"""
    d = Dense(block_idx, label, None)
    ids = np.asarray(ids, np.int64).reshape(len(d.bidx), 512)
    assert ids.min(initial=-1) >= -1 and ids.max(initial=-1) < count, (int(ids.min(initial=-1)), int(ids.max(initial=-1)), count)
    fg = ids >= 0
    assert np.array_equal(np.unique(ids[fg]), np.arange(count)), "the ids in the volume are not exactly 0 .. count - 1"
    low = np.full(count, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(low, ids[fg], d.lin[fg])
    keys = np.where(fg, np.r_[low, -1][np.where(fg, ids, count)], -1)
    comps = {}
    for i in range(min(count, len(records))):
        r = records[i]
        comps[d.voxel_of(low[i])] = (int(r["label"]), int(r["voxels"]), tuple(r["min_xyz"].tolist()), tuple(r["max_xyz"].tolist()),
                                     tuple(int(v) for v in r["sum_xyz"]), np.float32(r["peak_score"]).view(np.uint32).item(), tuple(r["peak_xyz"].tolist()))
    return comps, keys


# ---- drawn volumes: dense int32 label volumes over a cube of blocks, cut into a shuffled block list
def cut(dense_label, dense_score=None, origin_block=(0, 0, 0), drop=(), seed=0):
    """dense [8 bx, 8 by, 8 bz] -> (block_idx [n, 3] int32, label [n, 512] int32, score [n, 512] float32 | None), the blocks in `drop` (positions
    inside the cube) left out, the entries shuffled with `seed`"""
    L = np.asarray(dense_label, np.int32)
    nb = [s // 8 for s in L.shape]
    assert all(s % 8 == 0 for s in L.shape)

    def blocks(a):
        return a.reshape(nb[0], 8, nb[1], 8, nb[2], 8).transpose(0, 2, 4, 1, 3, 5).reshape(-1, 512)
    pos = np.stack(np.meshgrid(*[np.arange(k) for k in nb], indexing="ij"), -1).reshape(-1, 3)
    keep = np.array([tuple(p) not in {tuple(x) for x in drop} for p in pos.tolist()])
    order = np.random.default_rng(seed).permutation(int(keep.sum()))
    bidx = (pos[keep] + np.asarray(origin_block)).astype(np.int32)[order]
    lab = blocks(L)[keep][order]
    sc = blocks(np.asarray(dense_score, np.float32))[keep][order] if dense_score is not None else None
    return np.ascontiguousarray(bidx), np.ascontiguousarray(lab), None if sc is None else np.ascontiguousarray(sc)


def checkerboard(n=8):
    x, y, z = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    return np.where((x + y + z) % 2 == 0, 0, -1).astype(np.int32)


def z_planes(n=8):
    """two labels interleaved in z planes"""
    return np.broadcast_to((np.arange(n) % 2).astype(np.int32), (n, n, n)).copy()


def serpentine(n=8):
    """One 6-connected path through the cube: in every other x plane the rows y = 0, 2, .. run along all of z and are joined at alternating ends
    by one voxel in the rows between; the planes are joined through one voxel in the plane between, at alternating ends (y = n - 2, then 0)."""
    L = np.full((n, n, n), -1, np.int32)
    for x in range(0, n, 2):
        L[x, 0::2, :] = 0
        for y in range(1, n - 1, 2):
            L[x, y, n - 1 if (y // 2) % 2 == 0 else 0] = 0
        if x + 2 < n:
            L[x + 1, n - 2 if (x // 2) % 2 == 0 else 0, 0] = 0
    return L


def u_shape():
    """24^3: two arms along x in the block columns (by, bz) = (0, 0) and (2, 0), joined only at x = 23 (the farthest blocks from the lowest voxel)"""
    L = np.full((24, 24, 24), -1, np.int32)
    L[:, 3, 3] = 2; L[:, 19, 3] = 2; L[23, 3:20, 3] = 2
    return L


def contacts():
    """24^3: pairs of voxels that touch only across a block edge or a block corner, in the all-positive and in mixed-sign directions"""
    L = np.full((24, 24, 24), -1, np.int32)
    for a, b in [((7, 7, 3), (8, 8, 3)), ((15, 15, 15), (16, 16, 16)), ((15, 16, 3), (16, 15, 3)), ((7, 8, 16), (8, 7, 15)), ((3, 7, 20), (3, 8, 21))]:
        L[a] = 0; L[b] = 0
    return L


def side_by_side():
    """24^3: two labels that meet along the block face x = 8"""
    L = np.full((24, 24, 24), -1, np.int32)
    L[2:8, 4:20, 4:20] = 0; L[8:14, 4:20, 4:20] = 1
    return L


def noise(shape, seed=5):
    """labels from {-1, 0, 1} with probabilities (0.2, 0.4, 0.4): above the 6-connected percolation density.  -> (labels, random scores, scores
    quantised to 4 levels so that peaks tie)"""
    rng = np.random.default_rng(seed)
    L = rng.choice(np.array([-1, 0, 1], np.int32), size=shape, p=[0.2, 0.4, 0.4]).astype(np.int32)
    s = rng.standard_normal(shape).astype(np.float32)
    return L, s, (np.floor(rng.random(shape) * 4) / 4 - 0.5).astype(np.float32)
