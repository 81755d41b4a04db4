"""Masks drawn to break the fused dynamic-mask front end (nvbx_dynamic_depth_split, csrc/dynamics.hip), the model they are judged by, and the
recipe that makes the library compute exactly the drawn mask.  Plain numpy + scipy: nothing here imports the project.

THE MODEL.  filter_model = scipy.ndimage.label (8-connected) + bincount + size filter; split_model = the two depth images the cleaned mask
dictates for ONE camera and the identity transform (depth pixel i lands on mask pixel i).

THE RECIPE (steering).  A mapper with projective_layer_type = 2 and initialize_to_high_confidence_freespace = 1 integrates ONE depth frame of a
constant 4.0 m wall from the identity pose at time 0: every voxel of every block in view becomes high-confidence freespace.  A later depth
image that is 1.5 m where a pattern is set makes exactly those pixels dynamic; elsewhere it is 6.0 m (beyond max_distance_m = 5.0) or 0 (invalid).
tests/test_mask_patterns.py proves this on the CPU checker for every case below; tests/test_gpu_dynamic_masks.py relies on it.

THE GENERATORS know the lattice of k_dyn_detect_union: a workgroup owns 30 x 7 pixels of a 32 x 8 patch.  Each one asserts its own design with
the model (a serpentine IS one component of the expected size, pairs drawn apart ARE two components): a generator that degenerates at a small
image size fails here, on the CPU, instead of quietly testing nothing on the GPU.
"""
import functools

import numpy as np
import scipy.ndimage as ndi

OW, OH = 30, 7          # DYN_OW, DYN_OH of csrc/dynamics.hip: the owned region of a patch; its ring is the left + right column and the top row
STRUCT8 = np.ones((3, 3), np.int32)

# ------------------------------------------------------------------------------------------------ the model


def components(pattern, structure=STRUCT8):
    """(label image, sizes[1..n]) of the non-zero pixels."""
    lab, n = ndi.label(np.asarray(pattern) != 0, structure=structure)
    return lab, np.bincount(lab.ravel(), minlength=n + 1)[1:]


def component_sizes(pattern, structure=STRUCT8):
    return sorted(components(pattern, structure)[1].tolist())


def filter_model(pattern, min_size):
    """removeSmallConnectedComponents: 8-connected components with fewer than min_size pixels are erased (min_size <= 0: nothing is)."""
    p = np.asarray(pattern) != 0
    if min_size <= 0:
        return p.copy()
    lab, n = ndi.label(p, structure=STRUCT8)
    size = np.bincount(lab.ravel(), minlength=n + 1)
    size[0] = 0
    return p & (size[lab] >= min_size)


def split_model(depth, kept, invalid):
    """(unmasked, masked): a valid depth pixel under a kept mask pixel goes to `masked`, every other pixel stays in `unmasked`."""
    depth = np.asarray(depth, np.float32)
    m = np.asarray(kept, bool) & (depth > 0)
    inv = np.float32(invalid)
    return np.where(m, inv, depth).astype(np.float32), np.where(m, depth, inv).astype(np.float32)


def overlay_model(depth, masked_pixels):
    """(grey, red, red_is_decisive): the overlay's grey value floor(min(51 d, 255)), its red channel, and where red tells masked from unmasked."""
    d = np.asarray(depth, np.float32)
    gv = np.minimum(np.where(d > 0, d * np.float32(51.0), np.float32(0.0)), np.float32(255.0))
    grey = gv.astype(np.uint8)
    return grey, np.where(masked_pixels, np.uint8(255), grey), d * np.float32(51.0) < 255.0

# ------------------------------------------------------------------------------------------------ the steering recipe


WALL_M, DYNAMIC_M, FAR_M, MAX_DISTANCE_M, OCCLUSION_THRESHOLD_M = 4.0, 1.5, 6.0, 5.0, 0.25
STEER_PARAMS = dict(projective_layer_type=2, initialize_to_high_confidence_freespace=1)

# (fu, fv, cu, cv, cols, rows) by (rows, cols): focal length ~ half the longer side, principal point at the centre
CAMERAS = {
    (1, 1): (16.0, 16.0, 0.5, 0.5, 1, 1),
    (1, 64): (32.0, 32.0, 32.0, 0.5, 64, 1),
    (64, 1): (32.0, 32.0, 0.5, 32.0, 1, 64),
    (7, 30): (16.0, 16.0, 14.5, 3.5, 30, 7),
    (8, 31): (16.0, 16.0, 15.0, 3.5, 31, 8),
    (15, 61): (30.0, 30.0, 30.0, 7.0, 61, 15),
    (61, 15): (30.0, 30.0, 7.0, 30.0, 15, 61),
    (22, 90): (45.0, 45.0, 44.5, 10.5, 90, 22),
    (120, 160): (80.0, 80.0, 79.5, 59.5, 160, 120),
    (480, 640): (320.0, 320.0, 319.5, 239.5, 640, 480),
}


def wall_depth(rows, cols):
    return np.full((rows, cols), WALL_M, np.float32)


def steering_depth(pattern, background="far"):
    """The depth image that makes `pattern` the dynamic mask: 'far' = 6.0 m elsewhere, 'invalid' = 0 elsewhere, 'mixed' = 6.0 m on even rows."""
    p = np.asarray(pattern, bool)
    bg = np.full(p.shape, FAR_M, np.float32)
    if background == "invalid":
        bg[:] = 0.0
    elif background == "mixed":
        bg[1::2, :] = 0.0
    else:
        assert background == "far", background
    return np.where(p, np.float32(DYNAMIC_M), bg).astype(np.float32)

# ------------------------------------------------------------------------------------------------ the generators


def _img(rows, cols):
    return np.zeros((rows, cols), bool)


def random_mask(rows, cols, density, seed=0):
    """Independent pixels; 0.42 is about the 8-connected percolation threshold (long snaking components)."""
    return np.random.default_rng(1000 * seed + int(round(density * 100)) + 7 * rows + cols).random((rows, cols)) < density


def all_ones(rows, cols):
    p = np.ones((rows, cols), bool)
    assert component_sizes(p) == [rows * cols]
    return p


def all_zeros(rows, cols):
    return _img(rows, cols)


def single_pixels(rows, cols):
    """One pixel in each corner and one in the centre."""
    p = _img(rows, cols)
    spots = {(0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1), (rows // 2, cols // 2)}
    for r, c in spots:
        p[r, c] = True
    assert component_sizes(p) == [1] * len(spots), (rows, cols)
    return p


def serpentine(rows, cols):
    """Every second row full, joined alternately at the last and at the first column: ONE component, one pixel wide, through every patch."""
    assert rows >= 3 and cols >= 3, (rows, cols)
    p = _img(rows, cols)
    p[0::2, :] = True
    for k, r in enumerate(range(1, rows, 2)):
        p[r, cols - 1 if k % 2 == 0 else 0] = True
    n_full, n_join = (rows + 1) // 2, rows // 2
    assert component_sizes(p) == [n_full * cols + n_join] and component_sizes(p, None) == [n_full * cols + n_join]
    q = p.copy(); q[1, cols - 1] = False                      # (the joints are the only bridges)
    assert len(component_sizes(q)) == 2
    return p


def serpentine_columns(rows, cols):
    return np.ascontiguousarray(serpentine(cols, rows).T)


def spiral(rows, cols):
    """A square spiral, one pixel wide with one pixel between its arms: ONE component whose label chain winds inwards."""
    assert rows >= 5 and cols >= 5, (rows, cols)
    p = _img(rows, cols)
    l = 0
    while rows - 2 * l >= 1 and cols - 2 * l >= 1:
        t, b, le, ri = l, rows - 1 - l, l, cols - 1 - l
        if b - t >= 2 and ri - le >= 2:          # a ring, cut open under its top-left corner ...
            p[t, le:ri + 1] = True; p[b, le:ri + 1] = True; p[t:b + 1, le] = True; p[t:b + 1, ri] = True
            p[t + 1, le] = False
        else:                                    # (what is left in the middle: a line)
            p[t, le:ri + 1] = True
        if l > 0:
            p[t, le - 1] = True                  # ... and joined to the ring inside it along that ring's top row
        l += 2
    n = int(p.sum())
    assert n > rows + cols and component_sizes(p) == [n] and component_sizes(p, None) == [n], (rows, cols, n)
    assert not (p[:-1, :-1] & p[1:, :-1] & p[:-1, 1:] & p[1:, 1:]).any()          # one pixel wide
    return p


def staircase(rows, cols, direction, period=4):
    """Parallel diagonals `period` apart, 'nwse' or 'nesw': every link is diagonal (no 4-connected pair at all), every diagonal is one component,
    and together they cross the patch boundaries at every phase (the NW / NE ring links, the px == DYN_OW rule); one of them passes exactly
    through the first interior lattice corner (7, 30)."""
    assert period >= 3 and direction in ("nwse", "nesw")
    r, c = np.mgrid[0:rows, 0:cols]
    k, phase = ((c - r), OW - OH) if direction == "nwse" else ((c + r), OW + OH - 1)
    p = ((k - phase) % period) == 0
    want = sorted(np.bincount((k[p] - k.min()).ravel()).tolist())
    want = [s for s in want if s > 0]
    assert component_sizes(p) == want, (rows, cols, direction)
    assert component_sizes(p, None) == [1] * int(p.sum())                          # diagonal-only connectivity
    if rows > OH and cols > OW:
        assert (p[OH - 1, OW - 1] and p[OH, OW]) if direction == "nwse" else (p[OH - 1, OW] and p[OH, OW - 1])
    return p


def lattice_lines(rows, cols, which):
    """Full rows at r = 6 and r = 0 (mod 7), full columns at c = 29 and c = 0 (mod 30): the last and the first owned row / column of adjacent
    patches.  which: 'rows6' 'rows0' 'cols29' 'cols0' (one residue alone), 'rows' 'cols' (both residues), 'grid' (all four)."""
    p = _img(rows, cols)
    r6, r0 = list(range(OH - 1, rows, OH)), list(range(0, rows, OH))
    c29, c0 = list(range(OW - 1, cols, OW)), list(range(0, cols, OW))
    if which in ("rows6", "rows", "grid"): p[r6, :] = True
    if which in ("rows0", "rows", "grid"): p[r0, :] = True
    if which in ("cols29", "cols", "grid"): p[:, c29] = True
    if which in ("cols0", "cols", "grid"): p[:, c0] = True
    sizes = component_sizes(p)
    if which in ("rows6", "rows0"):
        n = len(r6 if which == "rows6" else r0)
        assert n >= 1 and sizes == [cols] * n, (rows, cols, which)
    elif which in ("cols29", "cols0"):
        n = len(c29 if which == "cols29" else c0)
        assert n >= 1 and sizes == [rows] * n, (rows, cols, which)
    elif which == "rows":
        lines = sorted(set(r6) | set(r0))
        groups = 1 + sum(1 for a, b in zip(lines, lines[1:]) if b - a > 1)          # rows 6 and 7 touch, rows 0 and 6 do not
        assert len(sizes) == groups and sum(sizes) == len(lines) * cols, (rows, cols)
    elif which == "cols":
        lines = sorted(set(c29) | set(c0))
        groups = 1 + sum(1 for a, b in zip(lines, lines[1:]) if b - a > 1)
        assert len(sizes) == groups and sum(sizes) == len(lines) * rows, (rows, cols)
    elif which == "grid":
        assert len(sizes) == 1, (rows, cols)
    assert p.any()
    return p


def comb(rows, cols, mirrored=False):
    """One comb per patch row.  Spine on the patch's LAST owned row (r = 6 mod 7), teeth on every second column rising through rows 1..5 of the
    patch: the teeth meet only through the spine, whose pixels are all `shared`.  Mirrored: spine on the FIRST owned row (r = 0 mod 7), teeth
    hanging down through rows 1..5.  A free row separates a comb from the next one."""
    assert rows >= OH and cols >= 3, (rows, cols)
    p = _img(rows, cols)
    n = 0
    for top in range(0, rows - OH + 1, OH):
        p[top + (0 if mirrored else OH - 1), :] = True
        p[top + 1:top + OH - 1, 0::2] = True
        n += 1
    each = cols + (OH - 2) * ((cols + 1) // 2)
    assert component_sizes(p) == [each] * n, (rows, cols, mirrored)
    q = p.copy(); q[(0 if mirrored else OH - 1), :] = False                       # without its spine the first comb is its teeth
    assert len(component_sizes(q)) == n - 1 + (cols + 1) // 2
    return p


ENCOUNTER_TAIL = 5
ENCOUNTER_MIN_SIZE = ENCOUNTER_TAIL + 1          # a merged pair (tail + single pixel) survives, a tail or a pixel alone does not


def encounters(rows, cols, direction, apart, at=(0, 0)):
    """At every lattice point (7 k + at[0], 30 j + at[1]) that has room: a horizontal tail of ENCOUNTER_TAIL pixels and a single pixel that touch
    ONLY diagonally across the point -- 'nwse': tail ending at (r - 1, c - 1), pixel at (r, c); 'nesw': pixel at (r - 1, c), tail ending at
    (r, c - 1).  at = (0, 0) is a patch corner, (3, 0) a vertical patch boundary in mid-patch, (0, 15) a horizontal one.  apart: the tail is
    moved one pixel away, so the two must NOT merge.  With min_size = ENCOUNTER_MIN_SIZE the outcome shows: merged pairs stay, all else goes."""
    assert direction in ("nwse", "nesw")
    L = ENCOUNTER_TAIL
    p = _img(rows, cols)
    n = 0
    for r in range(at[0], rows, OH):
        for c in range(at[1], cols, OW):
            end = c - 1 - (1 if apart else 0)
            if r < 1 or end - L + 1 < 0:
                continue
            if direction == "nwse":
                p[r - 1, end - L + 1:end + 1] = True; p[r, c] = True
            else:
                p[r, end - L + 1:end + 1] = True; p[r - 1, c] = True
            n += 1
    assert n >= 1, (rows, cols, at)
    assert component_sizes(p) == ([1] * n + [L] * n if apart else [L + 1] * n), (rows, cols, direction, apart, at)
    kept = filter_model(p, ENCOUNTER_MIN_SIZE)
    assert int(kept.sum()) == (0 if apart else (L + 1) * n)
    return p


BRIDGE_MIN_SIZE = ENCOUNTER_TAIL + 3


def bridges(rows, cols):
    """At every vertical patch boundary c = 30 j and row r = 7 k + 4 that has room: a horizontal tail in the LEFT patch ending on its last owned
    column at (r, c - 1), and in the RIGHT patch a three-pixel diagonal (r, c), (r - 1, c + 1), (r - 2, c + 2) whose root has a SMALLER index
    than the tail's end.  Their only contact is the W link of (r, c), and the tail's end is not the root of its own patch: if the right patch
    re-hangs it before the left patch links it to its tail, only a proper union keeps both links (the px == DYN_OW part of `shared`).  With
    min_size = BRIDGE_MIN_SIZE a lost link erases the whole figure."""
    L = ENCOUNTER_TAIL
    p = _img(rows, cols)
    n = 0
    for r in range(4, rows, OH):
        for c in range(OW, cols - 2, OW):
            p[r, c - L:c] = True
            p[r, c] = p[r - 1, c + 1] = p[r - 2, c + 2] = True
            n += 1
    assert n >= 1, (rows, cols)
    assert component_sizes(p) == [L + 3] * n
    q = p.copy(); q[4, OW - 1] = False                         # the tail's end IS the bridge
    assert sorted(component_sizes(q))[:2] == [3, L - 1]
    return p


def threshold_blobs(rows, cols, min_size):
    """Three isolated compact blobs of exactly min_size - 1, min_size and min_size + 1 pixels (the kernel's test is `<`)."""
    assert min_size >= 2
    p = _img(rows, cols)
    c0 = 1
    for s in (min_size - 1, min_size, min_size + 1):
        w = int(np.ceil(np.sqrt(s)))
        h = (s + w - 1) // w
        assert 1 + h <= rows and c0 + w <= cols, (rows, cols, min_size)
        blob = (np.arange(h * w) < s).reshape(h, w)
        p[1:1 + h, c0:c0 + w] = blob
        c0 += w + 2
    assert component_sizes(p) == [min_size - 1, min_size, min_size + 1]
    assert int(filter_model(p, min_size).sum()) == 2 * min_size + 1
    return p


def threshold_lines(rows, cols, min_size, axis):
    """The same three sizes as one-pixel lines that straddle a patch boundary: axis 'h' = horizontal lines across c = 30 on rows 1, 3, 5;
    'v' = vertical lines across r = 7 on columns 1, 3, 5."""
    assert min_size >= 3 and axis in ("h", "v")
    if axis == "v":
        return np.ascontiguousarray(_lines(cols, rows, min_size, OH).T)
    return _lines(rows, cols, min_size, OW)


def _lines(rows, cols, min_size, boundary):
    p = _img(rows, cols)
    for k, s in enumerate((min_size - 1, min_size, min_size + 1)):
        lo = boundary - s // 2
        assert lo >= 0 and lo + s <= cols and 1 + 2 * k < rows and lo < boundary < lo + s, (rows, cols, min_size)
        p[1 + 2 * k, lo:lo + s] = True
    assert component_sizes(p) == [min_size - 1, min_size, min_size + 1]
    assert int(filter_model(p, min_size).sum()) == 2 * min_size + 1
    return p

# ------------------------------------------------------------------------------------------------ the cases: pattern x size x thresholds


SIZES = [(1, 1), (1, 64), (64, 1), (7, 30), (8, 31), (15, 61), (61, 15), (22, 90), (120, 160)]
FULL_RES = (480, 640)
# 0, 1, 2, one value inside the component-size distribution, one larger than the image
THRESHOLDS = {(1, 1): (0, 1, 2), (1, 64): (0, 1, 2, 4, 65), (64, 1): (0, 1, 2, 4, 65), (7, 30): (0, 1, 2, 6, 211), (8, 31): (0, 1, 2, 6, 249),
              (15, 61): (0, 1, 2, 9, 916), (61, 15): (0, 1, 2, 9, 916), (22, 90): (0, 1, 2, 12, 1981), (120, 160): (0, 1, 2, 40, 19201)}
EDGE_MIN_SIZE = 9            # the threshold-edge cases' min_size (8, 9 and 10 pixels)


@functools.lru_cache(maxsize=None)
def cases(rows, cols):
    """[(name, pattern, background, thresholds)] for one image size: every generator whose design fits the size, at the size's thresholds;
    the encounter and threshold-edge patterns at the threshold they are designed for as well.  Patterns are read-only."""
    thr = THRESHOLDS[(rows, cols)]
    out = []

    def add(name, p, background="far", extra=()):
        p = np.ascontiguousarray(p, bool); p.setflags(write=False)
        assert p.shape == (rows, cols), (name, p.shape)
        out.append((name, p, background, tuple(sorted(set(thr) | set(extra)))))

    for k, density in enumerate((0.30, 0.42, 0.60)):
        add("random%.2f" % density, random_mask(rows, cols, density), ("far", "invalid", "mixed")[k])
    add("ones", all_ones(rows, cols)); add("zeros", all_zeros(rows, cols), "invalid")
    if rows * cols == 1 or (rows == 1 or rows >= 5) and (cols == 1 or cols >= 5):
        add("single_pixels", single_pixels(rows, cols), "mixed")
    if rows >= 3 and cols >= 3:
        add("serpentine", serpentine(rows, cols)); add("serpentine_columns", serpentine_columns(rows, cols), "invalid")
        for d in ("nwse", "nesw"):
            add("staircase_" + d, staircase(rows, cols, d)); add("staircase3_" + d, staircase(rows, cols, d, 3), "mixed")
    if rows >= 5 and cols >= 5:
        add("spiral", spiral(rows, cols))
    for which in ("rows6", "rows0", "cols29", "cols0", "rows", "cols", "grid"):
        if (which == "rows6" and rows < OH) or (which == "cols29" and cols < OW):
            continue
        add("lattice_" + which, lattice_lines(rows, cols, which))
    if rows >= OH and cols >= 3:
        add("comb", comb(rows, cols)); add("comb_mirrored", comb(rows, cols, True), "invalid")
    for at, tag in (((0, 0), "corner"), ((3, 0), "vertical"), ((0, 15), "horizontal")):
        if rows > (at[0] or OH) and cols > (at[1] or OW):
            for d in ("nwse", "nesw"):
                for apart in (False, True):
                    add("%s_%s_%s" % (tag, d, "apart" if apart else "touching"), encounters(rows, cols, d, apart, at), "far" if d == "nwse" else "mixed",
                        (ENCOUNTER_MIN_SIZE,))
    if rows > 4 and cols > OW + 2:
        add("bridges", bridges(rows, cols), "far", (BRIDGE_MIN_SIZE,))
    m = EDGE_MIN_SIZE
    if rows >= 5 and cols >= 16:
        add("threshold_blobs", threshold_blobs(rows, cols, m), "far", (m - 1, m, m + 1))
    if rows >= 6 and cols > OW + m:
        add("threshold_lines_h", threshold_lines(rows, cols, m, "h"), "mixed", (m - 1, m, m + 1))
    if cols >= 6 and rows > OH + m:
        add("threshold_lines_v", threshold_lines(rows, cols, m, "v"), "far", (m - 1, m, m + 1))
    return out


@functools.lru_cache(maxsize=None)
def full_res_cases():
    """480 x 640 once: the percolation-density random mask and the serpentine (a chain through all 1 518 patches), two thresholds each."""
    rows, cols = FULL_RES
    out = []
    for name, p, thr in (("random0.42", random_mask(rows, cols, 0.42), (40, 640)), ("serpentine", serpentine(rows, cols), (640, rows * cols + 1))):
        p = np.ascontiguousarray(p, bool); p.setflags(write=False)
        out.append((name, p, "far", thr))
    return out


def pattern(rows, cols, name):
    for n, p, _, _ in cases(rows, cols):
        if n == name:
            return p
    raise KeyError((rows, cols, name))
