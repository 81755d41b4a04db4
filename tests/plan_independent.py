"""The cost field and its paths (SEMANTICS.md "Cost field and paths") as a model that shares no code with the product: pixel classes and
penalties in numpy float32, the moves as an explicit sparse graph, scipy's Dijkstra over it (integer weights are exact in its float64), the path
rule as a plain walk.  Imports nothing from the product and nothing from oracle/.  Also the drawn and random cases tests/test_plan_model.py
(CPU) and tests/test_gpu_plan.py share, with the condition every random case must meet."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import dijkstra

F32 = np.float32
UNREACHED = 0x7fffffff
MOVES = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))      # (drow, dcol), the order the path rule tries them in
DEFAULTS = dict(robot_radius_m=0.25, inflation_radius_m=0.75, penalty_per_m=100.0, unknown_value=1000.0, max_penalty=200, unknown_penalty=50,
                allow_unknown=0)


def options(**kw):
    assert not set(kw) - set(DEFAULTS), set(kw) - set(DEFAULTS)
    return dict(DEFAULTS, **kw)


def classify(img, o):
    """-> (traversable bool [rows, cols], penalty int64 [rows, cols]; 0 where not traversable)"""
    v = np.asarray(img, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        unknown = np.abs(v - F32(o["unknown_value"])) < F32(1e-2)
        trav = ~unknown & (v > F32(0)) & (v >= F32(o["robot_radius_m"]))
        t = F32(o["inflation_radius_m"]) - v
        u = F32(o["penalty_per_m"]) * t
        below = u < F32(o["max_penalty"])
        pen = np.where(t > F32(0), np.where(below, np.trunc(np.where(below, u, F32(0))), F32(o["max_penalty"])), F32(0)).astype(np.int64)
    if o["allow_unknown"]:
        trav = trav | unknown
    pen = np.where(unknown, np.int64(o["unknown_penalty"]), pen)
    return trav, np.where(trav, pen, 0)


def _shift(a, dr, dc, fill):
    """b[r, c] = a[r + dr, c + dc], `fill` outside"""
    rows, cols = a.shape
    b = np.full_like(a, fill)
    r0, r1 = max(0, -dr), min(rows, rows - dr)
    c0, c1 = max(0, -dc), min(cols, cols - dc)
    if r0 < r1 and c0 < c1:
        b[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return b


def graph(trav, pen):
    """the moves as a sparse matrix: entry (p, q) = c(p, q), pixels numbered row * cols + col"""
    rows, cols = trav.shape
    ids = np.arange(rows * cols).reshape(rows, cols)
    src, dst, w = [], [], []
    for dr, dc in MOVES:
        ok = trav & _shift(trav, dr, dc, False)
        if dr and dc:
            ok &= _shift(trav, dr, 0, False) & _shift(trav, 0, dc, False)      # no corner is cut
        q = _shift(ids, dr, dc, -1)
        cost = (14 if dr and dc else 10) + pen + _shift(pen, dr, dc, 0)
        src.append(ids[ok]); dst.append(q[ok]); w.append(cost[ok])
    n = rows * cols
    return sp.csr_matrix((np.concatenate(w).astype(np.float64), (np.concatenate(src), np.concatenate(dst))), shape=(n, n))


def accepted_sources(trav, sources):
    s = np.asarray(sources, np.int64).reshape(-1, 2)
    rows, cols = trav.shape
    inside = (s[:, 0] >= 0) & (s[:, 0] < rows) & (s[:, 1] >= 0) & (s[:, 1] < cols)
    ok = inside.copy()
    ok[inside] = trav[s[inside, 0], s[inside, 1]]
    return s[ok]


def field(img, sources, o):
    """-> (G int32 [rows, cols], the number of accepted source entries)"""
    trav, pen = classify(img, o)
    rows, cols = trav.shape
    acc = accepted_sources(trav, sources)
    G = np.full(rows * cols, UNREACHED, np.int64)
    if len(acc):
        d = dijkstra(graph(trav, pen), directed=True, indices=np.unique(acc[:, 0] * cols + acc[:, 1]), min_only=True)
        G = np.where(np.isfinite(d), d, UNREACHED).astype(np.int64)
    assert G.max() <= UNREACHED
    return G.reshape(rows, cols).astype(np.int32), len(acc)


def path(img, G, start, o):
    """the path rule: -> the list of (row, col) from `start` to the first pixel with G = 0; [] for a start outside the image or UNREACHED;
    None where no neighbour satisfies the equation"""
    trav, pen = classify(img, o)
    rows, cols = trav.shape
    r, c = int(start[0]), int(start[1])
    if not (0 <= r < rows and 0 <= c < cols) or int(G[r, c]) == UNREACHED:
        return []
    out = [(r, c)]
    while int(G[r, c]) != 0:
        if len(out) > rows * cols or not trav[r, c]:
            return None
        for dr, dc in MOVES:
            qr, qc = r + dr, c + dc
            if not (0 <= qr < rows and 0 <= qc < cols) or not trav[qr, qc] or int(G[qr, qc]) == UNREACHED:
                continue
            if dr and dc and not (trav[qr, c] and trav[r, qc]):
                continue
            if int(G[qr, qc]) + (14 if dr and dc else 10) + int(pen[r, c]) + int(pen[qr, qc]) == int(G[r, c]):
                r, c = qr, qc
                break
        else:
            return None
        out.append((r, c))
    return out


# ---- the cases the CPU and the GPU tests share
CASE_OPTIONS = dict(robot_radius_m=0.10, inflation_radius_m=0.6, penalty_per_m=100.0, max_penalty=200)
LINE_SHAPES = ((1, 1), (1, 130), (130, 1))
RANDOM_SHAPES = ((31, 33), (32, 32), (33, 65), (64, 64))
SEEDS_PER_SHAPE = 3
BLOCKED, UNKNOWN = F32(-0.05), F32(1000.0)


def line_case(shape):
    """a one-row or one-column image, free but for ONE blocked pixel behind the first tile; sources at the first pixel and just past the tile rim"""
    rows, cols = shape
    img = np.full(shape, F32(0.9))
    n = rows * cols
    flat = img.reshape(-1)
    if n > 1:
        flat[97] = BLOCKED
    at = (lambda i: (0, i)) if rows == 1 else (lambda i: (i, 0))
    sources = np.array([at(0)] + ([at(32), at(31)] if n > 1 else []), np.int32)
    return img, sources


def _corner_and_rim_pixels(shape):
    """corners of the image and the pixels either side of the first tile rim, inside the image"""
    rows, cols = shape
    cand = [(0, 0), (rows - 1, cols - 1), (0, cols - 1), (rows - 1, 0), (31, 31), (32, 32), (31, 32), (32, 31), (rows // 2, 31), (31, cols // 2)]
    return [p for p in dict.fromkeys(cand) if p[0] < rows and p[1] < cols]


def draw_random(shape, seed):
    """20 % blocked, 5 % unknown, v uniform in (0, 1) m elsewhere; three sources from the corners and tile rims, their pixels made free"""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.0, 1.0, shape).astype(F32)
    kind = rng.uniform(0.0, 1.0, shape)
    img[kind < 0.20] = BLOCKED
    img[(kind >= 0.20) & (kind < 0.25)] = UNKNOWN
    cand = _corner_and_rim_pixels(shape)
    sources = np.array([cand[i] for i in rng.choice(len(cand), 3, replace=False)], np.int32)
    img[sources[:, 0], sources[:, 1]] = F32(0.9)
    return img, sources


def case_condition(img, sources, o):
    """what every random case must meet: the model reaches at least a quarter of all pixels and leaves a traversable pixel unreached"""
    G, _ = field(img, sources, o)
    trav, _ = classify(img, o)
    reached = G != UNREACHED
    return 4 * int(reached.sum()) >= G.size and bool((trav & ~reached).any())


def random_cases():
    """-> [(shape, seed, img, sources)]: per shape the first SEEDS_PER_SHAPE seeds of 0, 1, 2, ... whose draw meets the condition"""
    o = options(**CASE_OPTIONS)
    out = []
    for shape in RANDOM_SHAPES:
        found = 0
        for seed in range(64):
            img, sources = draw_random(shape, 1000 * shape[0] + shape[1] + 7919 * seed)
            if case_condition(img, sources, o):
                out.append((shape, seed, img, sources)); found += 1
                if found == SEEDS_PER_SHAPE:
                    break
        assert found == SEEDS_PER_SHAPE, (shape, found)
    return out


def serpentine(n=96):
    """every odd row blocked except one end pixel, alternating sides: one corridor through the whole image -> (img, the source (0, 0));
    the far end is where the model's field is largest"""
    img = np.full((n, n), F32(0.9))
    for r in range(1, n, 2):
        img[r, :] = BLOCKED
        img[r, n - 1 if (r // 2) % 2 == 0 else 0] = F32(0.9)
    return img, np.array([[0, 0]], np.int32)


# ---- option sets and stored values on every edge of a class or a penalty
EDGE_OPTIONS = (
    dict(), dict(allow_unknown=1), dict(allow_unknown=1, unknown_penalty=0), dict(allow_unknown=1, unknown_penalty=200), dict(inflation_radius_m=0.0),
    dict(robot_radius_m=0.1, inflation_radius_m=0.6, penalty_per_m=100.0), dict(robot_radius_m=0.0, penalty_per_m=400.0, max_penalty=100),
    dict(max_penalty=0), dict(penalty_per_m=0.0, inflation_radius_m=float("inf")), dict(unknown_value=-1.0, allow_unknown=1),
)


def edge_values(o):
    r = F32(o["robot_radius_m"]); unk = F32(o["unknown_value"]); infl = F32(o["inflation_radius_m"])
    vals = [r, np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf)), 0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 1e-30, unk, unk + F32(0.009), unk - F32(0.009),
            unk + F32(0.011), unk - F32(0.011), infl, np.nextafter(infl, F32(0)), 5.0]
    if o["penalty_per_m"] > 0 and np.isfinite(infl):
        edge = infl - F32(o["max_penalty"]) / F32(o["penalty_per_m"])      # u lands on max_penalty, and either side of it
        vals += [edge, np.nextafter(edge, F32(np.inf)), np.nextafter(edge, F32(-np.inf)), edge + F32(0.01), edge - F32(0.01)]
    vals += list(np.linspace(-0.2, 1.2, 141))
    return np.array(vals, F32)
