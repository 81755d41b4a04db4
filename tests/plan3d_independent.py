"""The cost volume and its 3-D paths (SEMANTICS.md "Cost volume and 3-D paths") as a model that shares no code with the product: the 26 moves
generated from the rule, the graph as an explicit sparse matrix with the no-corner-cutting rule, scipy's Dijkstra over it (integer weights are
exact in its float64), the path rule as a plain walk.  The voxel classes and penalties are those of the 2-D field by specification, so
`classify` and `options` come from tests/plan_independent.py.  Imports nothing from the product and nothing from oracle/.  Also the drawn and
random cases tests/test_plan3d_model.py (CPU) and tests/test_gpu_plan3d.py share, with the condition every random case must meet."""
import itertools

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

from plan_independent import classify, options, F32, UNREACHED, BLOCKED, UNKNOWN      # noqa: F401  (re-exported for the tests)

BASE = {1: 10, 2: 14, 3: 17}
_RANK = {1: 0, 0: 1, -1: 2}      # each component is ordered +1, 0, -1


def _k(d):
    return sum(1 for c in d if c)


# by the number of nonzero components, then lexicographically by (dx, dy, dz)
MOVES = tuple(sorted((d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)), key=lambda d: (_k(d),) + tuple(_RANK[c] for c in d)))
assert len(MOVES) == 26 and MOVES[:6] == ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (0, -1, 0), (-1, 0, 0))


def between(d):
    """the voxels p + e a move d must find traversable besides its two ends: e_i in {0, d_i}, e != 0, e != d (none, two or six)"""
    out = [e for e in itertools.product(*[(0, c) if c else (0,) for c in d]) if any(e) and e != tuple(d)]
    assert len(out) == {1: 0, 2: 2, 3: 6}[_k(d)]
    return out


def _shift(a, d, fill):
    """b[p] = a[p + d], `fill` where p + d lies outside"""
    b = np.full_like(a, fill)
    dst, src = [], []
    for n, c in zip(a.shape, d):
        lo, hi = max(0, -c), min(n, n - c)
        if lo >= hi:
            return b
        dst.append(slice(lo, hi)); src.append(slice(lo + c, hi + c))
    b[tuple(dst)] = a[tuple(src)]
    return b


def allowed(trav, d):
    """where the move d may start: both ends traversable and no corner cut"""
    ok = trav & _shift(trav, d, False)
    for e in between(d):
        ok &= _shift(trav, e, False)
    return ok


def graph(trav, pen):
    """the moves as a sparse matrix: entry (p, q) = c(p, q), voxels numbered (x * ny + y) * nz + z"""
    ids = np.arange(trav.size).reshape(trav.shape)
    src, dst, w = [], [], []
    for d in MOVES:
        ok = allowed(trav, d)
        q = _shift(ids, d, -1)
        cost = BASE[_k(d)] + pen + _shift(pen, d, 0)
        src.append(ids[ok]); dst.append(q[ok]); w.append(cost[ok])
    n = trav.size
    return sp.csr_matrix((np.concatenate(w).astype(np.float64), (np.concatenate(src), np.concatenate(dst))), shape=(n, n))


def accepted_sources(trav, sources):
    s = np.asarray(sources, np.int64).reshape(-1, 3)
    inside = np.all((s >= 0) & (s < np.array(trav.shape)), axis=1)
    ok = inside.copy()
    ok[inside] = trav[s[inside, 0], s[inside, 1], s[inside, 2]]
    return s[ok]


def field(vol, sources, o):
    """-> (G int32 [nx, ny, nz], the number of accepted source entries)"""
    trav, pen = classify(vol, o)
    acc = accepted_sources(trav, sources)
    G = np.full(trav.size, UNREACHED, np.int64)
    if len(acc):
        d = dijkstra(graph(trav, pen), directed=True, indices=np.unique(np.ravel_multi_index(acc.T, trav.shape)), min_only=True)
        G = np.where(np.isfinite(d), d, UNREACHED).astype(np.int64)
    assert G.max() <= UNREACHED
    return G.reshape(trav.shape).astype(np.int32), len(acc)


def _inside(shape, p):
    return all(0 <= c < n for c, n in zip(p, shape))


def path(vol, G, start, o):
    """the path rule: -> the list of (x, y, z) from `start` to the first voxel with G = 0; [] for a start outside the box or UNREACHED; None
    where no neighbour satisfies the equation"""
    trav, pen = classify(vol, o)
    shape = trav.shape
    p = tuple(int(c) for c in start)
    if not _inside(shape, p) or int(G[p]) == UNREACHED:
        return []
    out = [p]
    while int(G[p]) != 0:
        if len(out) > trav.size or not trav[p] or int(G[p]) < 0:
            return None
        for d in MOVES:
            q = tuple(a + b for a, b in zip(p, d))
            if not _inside(shape, q) or not trav[q] or int(G[q]) == UNREACHED:
                continue
            mid = [tuple(a + b for a, b in zip(p, e)) for e in between(d)]
            if not all(_inside(shape, m) and trav[m] for m in mid):
                continue
            if int(G[q]) + BASE[_k(d)] + int(pen[p]) + int(pen[q]) == int(G[p]):
                p = q
                break
        else:
            return None
        out.append(p)
    return out


# ---- the cases the CPU and the GPU tests share
TILE = (8, 8, 8)                  # the relaxation's tile (csrc/plan3d.hip): the shapes below sit on it, beside it and across it
CASE_OPTIONS = dict(robot_radius_m=0.10, inflation_radius_m=0.6, penalty_per_m=100.0, max_penalty=200)
LINE_SHAPES = ((1, 1, 1), (130, 1, 1), (1, 130, 1), (1, 1, 130))
# the tile itself, one voxel more on each axis in turn and on all three, one voxel less and more mixed over several tiles
TILE_SHAPES = (TILE, (9, 8, 8), (8, 9, 8), (8, 8, 9), (9, 9, 9), (7, 7, 7), (9, 17, 7), (7, 9, 33), (17, 7, 9))
RANDOM_SHAPES = ((16, 16, 16), (17, 17, 33), (20, 25, 40))     # at least two tiles on every axis, at most 2^15 voxels
SEEDS_PER_SHAPE = 2


def line_case(shape):
    """a line of voxels along one axis, free but for ONE blocked voxel near the far end; sources at the first voxel and on both sides of the
    tile boundary at 64 (a boundary of every tile extent)"""
    vol = np.full(shape, F32(0.9))
    n = vol.size
    axis = int(np.argmax(shape))
    at = lambda i: tuple(i if a == axis else 0 for a in range(3))      # noqa: E731
    if n > 1:
        vol.reshape(-1)[120] = BLOCKED
    sources = np.array([at(0)] + ([at(64), at(63)] if n > 1 else []), np.int32)
    return vol, sources


def _corner_and_rim_voxels(shape):
    """corners of the box and the voxels either side of the first tile rim on every axis, inside the box"""
    n = np.array(shape)
    cand = [tuple(c) for c in itertools.product(*[(0, s - 1) for s in shape])]
    t = np.array(TILE)
    cand += [tuple(t - 1), tuple(t), (t[0] - 1, t[1], t[2] - 1), (t[0], t[1] - 1, t[2]), (shape[0] // 2, t[1] - 1, t[2]), (t[0], shape[1] // 2, t[2] - 1)]
    return [tuple(int(v) for v in p) for p in dict.fromkeys(cand) if np.all(np.array(p) < n)]


def draw_random(shape, seed):
    """20 % blocked, 5 % unknown, v uniform in (0, 1) m elsewhere; three sources from the corners and tile rims, their voxels made free"""
    rng = np.random.default_rng(seed)
    vol = rng.uniform(0.0, 1.0, shape).astype(F32)
    kind = rng.uniform(0.0, 1.0, shape)
    vol[kind < 0.20] = BLOCKED
    vol[(kind >= 0.20) & (kind < 0.25)] = UNKNOWN
    cand = _corner_and_rim_voxels(shape)
    sources = np.array([cand[i] for i in rng.choice(len(cand), min(3, len(cand)), replace=False)], np.int32).reshape(-1, 3)
    vol[sources[:, 0], sources[:, 1], sources[:, 2]] = F32(0.9)
    return vol, sources


def case_shares(vol, sources, o):
    """-> (blocked share, unknown share, accepted sources, reached share of the traversable voxels)"""
    G, acc = field(vol, sources, o)
    trav, _ = classify(vol, o)
    return (float((np.abs(vol - BLOCKED) < 1e-6).mean()), float((np.abs(vol - UNKNOWN) < 1e-6).mean()), acc,
            float((G != UNREACHED).sum()) / max(int(trav.sum()), 1))


def case_condition(vol, sources, o):
    """what every random case must meet: blocked share between 0.1 and 0.3, unknown share between 0.01 and 0.1, all three sources accepted, at
    least half of the traversable voxels reached"""
    blocked, unknown, acc, reached = case_shares(vol, sources, o)
    return 0.1 < blocked < 0.3 and 0.01 < unknown < 0.1 and acc == 3 and len(sources) == 3 and reached >= 0.5


def random_cases():
    """-> [(shape, seed, vol, sources)]: per shape the first SEEDS_PER_SHAPE seeds of 0, 1, 2, ... whose draw meets the condition"""
    o = options(**CASE_OPTIONS)
    out = []
    for shape in RANDOM_SHAPES:
        found = 0
        for seed in range(64):
            vol, sources = draw_random(shape, 10000 * shape[0] + 100 * shape[1] + shape[2] + 7919 * seed)
            if case_condition(vol, sources, o):
                out.append((shape, seed, vol, sources)); found += 1
                if found == SEEDS_PER_SHAPE:
                    break
        assert found == SEEDS_PER_SHAPE, (shape, found)
    return out


def tile_cases():
    """-> [(shape, vol, sources)]: one random draw per shape around the tile (no condition: some of them hold a few dozen voxels)"""
    return [(shape,) + draw_random(shape, 31 + 1000 * k) for k, shape in enumerate(TILE_SHAPES)]


def serpentine(n=24):
    """every odd x plane blocked except ONE voxel, in alternating corners of the (y, z) square: the best path crosses every free plane from
    corner to corner -> (vol, the source (0, 0, 0))"""
    vol = np.full((n, n, n), F32(0.9))
    for x in range(1, n, 2):
        vol[x] = BLOCKED
        c = n - 1 if (x // 2) % 2 == 0 else 0
        vol[x, c, c] = F32(0.9)
    return vol, np.array([[0, 0, 0]], np.int32)


# ---- the corner rule, every case: 2 x 2 x 2 cells in a blocked volume, a source in the low corner of each
CORNER_SHAPE = (12, 12, 18)
CORNER_ORIGIN = (1, 1, 1)         # cells at pitch 3 from here: the cells at 7..8 on every axis lie across a tile boundary, the z cells 16..17 begin a tile
CORNER_GRID = (4, 4, 6)
SPACE_BETWEEN = tuple(between((1, 1, 1)))
FACE_DIAGONALS = ((1, 1, 0), (1, 0, 1), (0, 1, 1))


def corner_cells():
    """-> (vol, sources [76, 3], cells): cells = [(low corner, far corner, the blocked ones of the voxels between, the diagonal)].  Cells 0 .. 63:
    the space diagonal with every subset of its six voxels between blocked; then per face diagonal the four subsets of its two, the cell's other
    layer blocked."""
    vol = np.full(CORNER_SHAPE, BLOCKED)
    spots = list(itertools.product(*[range(n) for n in CORNER_GRID]))
    jobs = [((1, 1, 1), [e for b, e in enumerate(SPACE_BETWEEN) if m >> b & 1]) for m in range(64)]
    jobs += [(d, [e for b, e in enumerate(between(d)) if m >> b & 1]) for d in FACE_DIAGONALS for m in range(4)]
    assert len(jobs) == 76 <= len(spots)
    cells, sources = [], []
    for (d, shut), spot in zip(jobs, spots):
        low = tuple(o + 3 * s for o, s in zip(CORNER_ORIGIN, spot))
        for e in itertools.product(*[(0, 1) if c else (0,) for c in d]):
            if e not in shut:
                vol[tuple(a + b for a, b in zip(low, e))] = F32(0.9)
        far = tuple(a + b for a, b in zip(low, d))
        assert all(0 <= c < n for c, n in zip(far, CORNER_SHAPE))
        cells.append((low, far, shut, d)); sources.append(low)
    return vol, np.array(sources, np.int32), cells


def special_values_volume():
    """a random case with NaN, +inf, -inf, negative values, zero and values on the penalty clamp strewn in"""
    vol, sources = draw_random((9, 17, 33), 424242)
    rng = np.random.default_rng(7)
    flat = vol.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, -1.0, -1e-30, 0.0, 0.1, np.nextafter(F32(0.1), F32(0)), 1e-30):
        flat[rng.choice(flat.size, 60, replace=False)] = F32(v)
    vol[sources[:, 0], sources[:, 1], sources[:, 2]] = F32(0.9)
    return vol, sources


OPTION_SETS = (
    dict(allow_unknown=1, unknown_penalty=0, **CASE_OPTIONS), dict(allow_unknown=1, unknown_penalty=200, **CASE_OPTIONS),
    dict(robot_radius_m=0.0, inflation_radius_m=0.0), dict(robot_radius_m=0.0, inflation_radius_m=5.0, penalty_per_m=1000.0, max_penalty=200),      # every penalty at the clamp
    dict(robot_radius_m=0.1, inflation_radius_m=0.6, penalty_per_m=400.0, max_penalty=200, allow_unknown=1, unknown_penalty=200),
)
