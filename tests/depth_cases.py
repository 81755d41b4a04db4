"""Camera depth fusion on DRAWN frames: what tests/test_depth_model.py (CPU: the checker against the float64 model) and tests/test_gpu_depth_drawn.py
(GPU: the product against the model and the checker) share.

The rendered room frames of the other suites practically never put a voxel exactly onto a pixel centre, an image border, the range limit or a
weighting threshold.  Here every frame is drawn so that some voxels do.  The exact-lattice cases use voxel 1/16 m (block 0.5 m), truncation 4 voxels =
0.25 m, the identity or a signed axis permutation as rotation, the camera at (1/32, 1/32, 1/32) + a multiple of 1/16 -- so the camera-frame centre of
every voxel is a multiple of 1/16 -- and dyadic intrinsics.  For the voxel layers at camera depth 0.5, 1 and 2 m the quotients x / z, y / z, the pixel
coordinates, the bilinear weights (0 or 1/2), the interpolated depth and the sdf are then exact in float32: on those EXACT VOXELS (exact_mask) a float32
kernel and the float64 model take every decision alike with margin 0.  tests/test_depth_model.py proves the claim by evaluating both.

A case: name, family, parameter overrides, camera (fu, fv, cu, cv, cols, rows), one pose and one image per frame (float32 metres, or uint16
millimetres for the u16 entry point), optional prior blocks for set_blocks (indices [n, 3], voxels [n, 512] of {distance, weight}; an occupancy mapper
takes `distance` as its log-odds), the camera depths of its exact layers, the voxels it was drawn for (label -> mask over the report of the last frame,
and whether the count must be positive or zero) and the block capacity.  Families:

  border          u, v exactly at 0, 1/2, 1, cols - 1, cols - 1/2, cols (rows alike); bilinear with an invalid rim and decay on, and nearest
  centre-taps     a voxel exactly on a valid pixel's centre whose right / lower / diagonal neighbour is 0, -0, NaN, -1.5, -inf or +inf
  tap-values      patches of +0, -0, 1e-40, FLT_MIN, NaN, +inf, -inf, -1.5, 1e30, 65.535 over voxels observed free
  range           voxels exactly at max_integration_distance_m, a wall beyond the limit
  behind          the camera's own block and its neighbours pre-filled: voxels at camera depth 0 and below
  sdf-thresholds  stripes that put the layer at 1 m on sdf = -trunc, -voxel, 0, +trunc and beyond; six weighting modes x two formula sets x both
                  states of the -trunc switch, the frame fused twice; truncation of one voxel
  prior           weight at / one below max_weight, weight 0 with a distance, distance at +-trunc; both clamp orders
  step            half the image at 1 m, a quarter at 2 m, a quarter invalid; decay factors 0, 1/2, 1
  tiny            images of 1 x 1, 1 x 7, 2 x 2, 3 x 5; ray subsampling 1 and 4
  single-ray      one valid pixel: along an axis, a face diagonal, the space diagonal from a block corner; one general ray through negative blocks
  oblique         (not exact) yaw 37, pitch -21, roll 13 degrees from (-3.3, -2.7, -1.1): a tilted noisy plane with a checkerboard of invalid patches
  occupancy       border, centre-taps, tap-values, step and the stripes with projective_layer_type 1; voxels exactly at ds -+ the half width
  u16             border and step in whole millimetres through the u16 entry point; 0 and 65535 among the taps
"""
import collections

import numpy as np

import tsdf_independent as TI

F = np.float32
VOXEL = 0.0625
TRUNC = 0.25
ORIGIN = (1 / 32, 1 / 32, 1 / 32)
EXACT_DEPTHS = (0.5, 1.0, 2.0)
FREE_D, FREE_W = F(0.2), F(3.0)                  # "observed free"
TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
COLS, ROWS = 32, 24
CAM_CENTRE = (16.0, 16.0, 16.5, 12.5, COLS, ROWS)     # layer 1 m: u - 1/2 = k + 16, every voxel on a pixel centre (weights 0); layer 2 m: weights 0 or 1/2
CAM_CORNER = (16.0, 16.0, 16.0, 12.0, COLS, ROWS)     # layer 1 m: u = k + 16, every voxel on a pixel corner (weights 1/2); layer 2 m: u = k / 2 + 16
TAP_VALUES = [("+0", F(0.0)), ("-0", F(-0.0)), ("denormal", F(1e-40)), ("FLT_MIN", np.finfo(F).tiny), ("NaN", F(np.nan)), ("+inf", F(np.inf)),
              ("-inf", F(-np.inf)), ("-1.5", F(-1.5)), ("1e30", F(1e30)), ("65.535", F(65.535))]
INVALID_TAPS = [(n, v) for n, v in TAP_VALUES if not (v > 0 and np.isfinite(v))]

Case = collections.namedtuple("Case", "name family kw cam poses depths prior exact_depths targets capacity")
# the last frame of a case, voxel by voxel over the blocks in its view (arrays of one length)
Report = collections.namedtuple("Report", "block u v z rule exact taps ax ay ds prev_d prev_w new_d new_w")


def pose(t=ORIGIN, R=None):
    T = np.eye(4, dtype=F)
    if R is not None:
        T[:3, :3] = np.asarray(R, F)
    T[:3, 3] = np.asarray(t, F)
    return T


def prior_box(lo, hi, d=FREE_D, w=FREE_W):
    """blocks lo <= index < hi, every voxel {d, w}"""
    idx = np.stack(np.meshgrid(*[np.arange(a, b) for a, b in zip(lo, hi)], indexing="ij"), -1).reshape(-1, 3).astype(np.int32)
    vox = np.zeros((len(idx), 512), TSDF_DT); vox["distance"] = d; vox["weight"] = w
    return idx, vox


FRUSTUM_BOX = ((-7, -6, -1), (7, 6, 7))         # holds the view of the 32 x 24 cameras out to 3 m, and a shell of blocks around it


def as_metres(image):
    """the float32 image the kernels see: a u16 image is converted pixel by pixel as (float) mm * (1.0f / 1000.0f)"""
    image = np.asarray(image)
    return image.astype(F) * (F(1.0) / F(1000.0)) if image.dtype == np.uint16 else image.astype(F)


def is_plain(kw):
    """the compile-time instantiation of the update: constant weighting, clamp after the blend, no decay, no occupancy"""
    return (kw.get("weighting_mode", 0) == 0 and not kw.get("tsdf_weight_clamp_before_blend", 0) and not kw.get("invalid_depth_decay_factor", -1.0) >= 0.0
            and kw.get("projective_layer_type", 0) == 0)


CASES = []


def _case(name, family, kw, cam, depths, poses=None, prior=None, exact=EXACT_DEPTHS, targets=None, capacity=1 << 12):
    depths = [np.ascontiguousarray(d) for d in (depths if isinstance(depths, list) else [depths])]
    poses = poses or [pose()] * len(depths)
    base = dict(voxel_size=VOXEL, truncation_distance_vox=4.0, raycast_subsampling_factor=1, max_integration_distance_m=4.0)
    base.update(kw)
    for d in depths:
        assert d.shape == (cam[5], cam[4]) and d.shape[0] <= 48 and d.shape[1] <= 64
    CASES.append(Case(name, family, base, tuple(cam), poses, depths, prior, tuple(exact), dict(targets or {}), capacity))


def _const(value, cam=CAM_CENTRE):
    return np.full((cam[5], cam[4]), value, F)


# ---- target masks over a Report (r); "some" = the count must be positive, "none" = zero
def _on(r, u=None, v=None, z=None):
    m = r.exact.copy()
    for have, want in ((r.u, u), (r.v, v), (r.z, z)):
        if want is not None:
            m &= have == want
    return m


# ------------------------------------------------------------------------------------------------ border
def _border_targets(cols, rows, nearest, rim_decay):
    t = {}
    for name, u in (("0", 0.0), ("1/2", 0.5), ("1", 1.0), ("cols-1", cols - 1.0), ("cols-1/2", cols - 0.5), ("cols", float(cols))):
        t["u = " + name] = (lambda r, u=u: _on(r, u=u), "some")
    for name, v in (("0", 0.0), ("1/2", 0.5), ("1", 1.0), ("rows-1", rows - 1.0), ("rows-1/2", rows - 0.5), ("rows", float(rows))):
        t["v = " + name] = (lambda r, v=v: _on(r, v=v), "some")
    inner = lambda r: (r.v > 2) & (r.v < rows - 2)
    if nearest:
        t["u = cols is outside"] = (lambda r: _on(r, u=float(cols)) & inner(r) & (r.rule == TI.OUTSIDE), "some")
        t["u = cols touched"] = (lambda r: _on(r, u=float(cols)) & (r.rule != TI.OUTSIDE), "none")
        t["u = cols - 1 is inside"] = (lambda r: _on(r, u=cols - 1.0) & inner(r) & (r.rule == TI.FUSED), "some")
        t["u = 0 is inside"] = (lambda r: _on(r, u=0.0) & inner(r) & (r.rule == TI.FUSED), "some")
    else:
        hit = TI.INVALID if rim_decay else TI.FUSED
        t["u = 0 in the image, outside the taps"] = (lambda r: _on(r, u=0.0) & inner(r) & ((r.prev_w > 0) | (r.prev_d != 0)) & (r.rule == TI.OUTSIDE), "some")
        t["u = 1/2 updated with weight 0"] = (lambda r: _on(r, u=0.5) & inner(r) & (r.ax == 0) & (r.rule == hit), "some")
        t["u = cols - 1/2 not updated"] = (lambda r: _on(r, u=cols - 0.5) & (r.rule != TI.OUTSIDE), "none")
        t["u = cols - 1/2 seen"] = (lambda r: _on(r, u=cols - 0.5) & ((r.prev_w > 0) | (r.prev_d != 0)), "some")
    return t


def _rim(img, value):
    img = img.copy(); img[0, :] = value; img[-1, :] = value; img[:, 0] = value; img[:, -1] = value
    return img


_case("border-bilinear", "border", {}, CAM_CORNER, _const(2.5), prior=prior_box(*FRUSTUM_BOX), targets=_border_targets(COLS, ROWS, 0, False))
_case("border-bilinear-rim-decay", "border", dict(invalid_depth_decay_factor=0.5), CAM_CORNER, _rim(_const(2.5), 0.0), prior=prior_box(*FRUSTUM_BOX),
      targets=_border_targets(COLS, ROWS, 0, True))
_case("border-nearest", "border", dict(depth_interp_nearest=1), CAM_CORNER, _const(2.5), prior=prior_box(*FRUSTUM_BOX), targets=_border_targets(COLS, ROWS, 1, False))

# ------------------------------------------------------------------------------------------------ centre-taps
# single invalid pixels on a wall at 2.5 m, far enough apart that no voxel reads two of them; the layers at 1 m and 2 m read each as a right, a lower
# and a diagonal neighbour with bilinear weight 0
CENTRE_PIXELS = [(4 + 8 * (k // 3), 5 + 10 * (k % 3)) for k in range(6)]          # (row, col)


def _centre_image():
    img = _const(2.5)
    for (r, c), (_, val) in zip(CENTRE_PIXELS, INVALID_TAPS):
        img[r, c] = val
    return img


def _centre_targets():
    t = {}
    for (row, col), (name, _) in zip(CENTRE_PIXELS, INVALID_TAPS):
        for where, (dr, dc) in (("right", (0, 1)), ("lower", (1, 0)), ("diagonal", (1, 1))):
            # the voxel on the centre of pixel (row - dr, col - dc): u = col - dc + 1/2
            t["%s as the %s neighbour" % (name, where)] = (
                lambda r, uu=col - dc + 0.5, vv=row - dr + 0.5: _on(r, u=uu, v=vv) & (r.ax == 0) & (r.ay == 0) & TI.tap_valid(r.taps[0]) & (r.rule == TI.INVALID), "some")
    return t


_case("centre-taps", "centre-taps", {}, CAM_CENTRE, _centre_image(), prior=prior_box(*FRUSTUM_BOX), targets=_centre_targets())
_case("centre-taps-decay", "centre-taps", dict(invalid_depth_decay_factor=0.5), CAM_CENTRE, _centre_image(), prior=prior_box(*FRUSTUM_BOX), targets=_centre_targets())

# ------------------------------------------------------------------------------------------------ tap-values
PATCH_AT = [(3 + 13 * (k // 5), 1 + 6 * (k % 5)) for k in range(10)]             # top-left (row, col) of each 5 x 5 patch


def _patch_image(cam=CAM_CENTRE, background=1.5):
    img = _const(background, cam)
    for (r, c), (_, val) in zip(PATCH_AT, TAP_VALUES):
        img[r:r + 5, c:c + 5] = val
    return img


def _in_patch(r, k):
    """voxels all of whose taps lie inside patch k"""
    val = TAP_VALUES[k][1]
    same = (r.taps.view(np.uint64) == np.float64(val).view(np.uint64)) if not np.isnan(val) else np.isnan(r.taps)
    return r.exact & same.all(0) & (r.rule != TI.OUTSIDE)


def _patch_targets():
    t = {}
    for k, (name, val) in enumerate(TAP_VALUES):
        valid = bool(val > 0 and np.isfinite(val))
        t["patch %s is %s" % (name, "valid" if valid else "invalid")] = (lambda r, k=k, valid=valid: _in_patch(r, k) & ((r.rule != TI.INVALID) == valid), "some")
        t["patch %s otherwise" % name] = (lambda r, k=k, valid=valid: _in_patch(r, k) & ((r.rule != TI.INVALID) != valid), "none")
    t["weight 0 on an infinite tap"] = (lambda r: r.exact & (r.rule == TI.INVALID) & np.isposinf(r.taps).any(0) & TI.tap_valid(r.taps[0]) & (r.ax == 0) & (r.ay == 0), "some")
    t["observed free before"] = (lambda r: r.exact & (r.prev_w > 0) & (r.prev_d > 0), "some")
    return t


for _nearest, _mode, _cam in ((0, 0, CAM_CENTRE), (0, 2, CAM_CENTRE), (0, 2, CAM_CORNER), (1, 0, CAM_CENTRE), (1, 2, CAM_CENTRE)):
    _t = _patch_targets()
    if _nearest or _cam is CAM_CORNER:
        del _t["weight 0 on an infinite tap"]
    _case("tap-values-%s-mode%d%s" % ("nearest" if _nearest else "bilinear", _mode, "-corner" if _cam is CAM_CORNER else ""), "tap-values",
          dict(depth_interp_nearest=_nearest, weighting_mode=_mode), _cam, [_const(1.5, _cam), _patch_image(_cam)], prior=prior_box(*FRUSTUM_BOX), targets=_t)

# ------------------------------------------------------------------------------------------------ range
_case("range-wall-beyond", "range", dict(max_integration_distance_m=2.0), CAM_CENTRE, _const(3.0),
      targets={"at the limit, updated": (lambda r: _on(r, z=2.0) & (r.rule == TI.FUSED), "some"),
               "the next layer, untouched": (lambda r: (r.z == 2.0625) & (r.rule == TI.OUTSIDE), "some"),
               "beyond the limit, touched": (lambda r: (r.z > 2.0) & (r.rule != TI.OUTSIDE), "none")})
_case("range-nearest", "range", dict(max_integration_distance_m=2.0, depth_interp_nearest=1, weighting_mode=5, tsdf_weighting_variant=1), CAM_CORNER, _const(2.0),
      targets={"at the limit, updated": (lambda r: _on(r, z=2.0) & (r.rule == TI.FUSED), "some"),
               "beyond the limit, touched": (lambda r: (r.z > 2.0) & (r.rule != TI.OUTSIDE), "none")})

# ------------------------------------------------------------------------------------------------ behind
_case("behind", "behind", {}, CAM_CENTRE, _const(1.0), poses=[pose((1 / 32, 1 / 32, 5 / 32))], prior=prior_box((-1, -1, -1), (2, 2, 2)), exact=(0.0, -0.0625, -0.125, 0.5, 1.0),
      targets={"camera depth 0": (lambda r: _on(r, z=0.0) & (r.prev_w > 0) & (r.rule == TI.OUTSIDE), "some"),
               "camera depth < 0": (lambda r: r.exact & (r.z < 0) & (r.prev_w > 0) & (r.rule == TI.OUTSIDE), "some"),
               "not in front, touched": (lambda r: (r.z <= 0) & (r.rule != TI.OUTSIDE), "none")})

# ------------------------------------------------------------------------------------------------ sdf-thresholds
# stripes of four columns: the layer at 1 m meets sdf = -1/4 (-trunc), -1/8, -1/16 (-voxel), 0, +1/8, +1/4 (+trunc), +1/2, +1 (the second and the
# fifth are the occupancy thresholds ds +- 1/8)
STRIPES = (0.75, 0.875, 0.9375, 1.0, 1.125, 1.25, 1.5, 2.0)


def _stripe_image():
    img = _const(2.0)
    for k, d in enumerate(STRIPES):
        img[:, 4 * k:4 * k + 4] = d
    return img


def _sdf_targets(trunc, skip):
    at = lambda s: (lambda r, s=s: _on(r, z=1.0) & (r.ds - r.z == s) & (r.taps == r.taps[0]).all(0))
    t = {"sdf = -trunc": (lambda r: at(-trunc)(r) & ((r.rule == TI.REJECTED) if skip else (r.rule != TI.OUTSIDE)), "some"),
         "sdf = -voxel": (lambda r: at(-VOXEL)(r) & (r.rule != TI.OUTSIDE), "some"), "sdf = 0": (lambda r: at(0.0)(r) & (r.rule == TI.FUSED), "some"),
         "sdf = +trunc": (lambda r: at(trunc)(r) & (r.rule == TI.FUSED), "some"), "sdf beyond +trunc": (lambda r: at(1.0)(r) & (r.rule == TI.FUSED), "some"),
         "blended with a prior weight": (lambda r: r.exact & (r.rule == TI.FUSED) & (r.prev_w > 0), "some")}
    if skip:
        t["sdf = -trunc fused"] = (lambda r: at(-trunc)(r) & (r.rule == TI.FUSED), "none")
    return t


for _mode in range(6):
    for _variant in (0, 1):
        for _skip in (0, 1):
            _t = _sdf_targets(TRUNC, _skip)
            if not _skip and _mode in (1, 3) or (not _skip and _mode == 4 and _variant == 1):
                # the ramp is 0 at -trunc: a measurement of weight 0 onto a voxel of weight 0 leaves it alone (twice)
                _t["weight 0 onto weight 0"] = (lambda r: _on(r, z=1.0) & (r.ds - r.z == -TRUNC) & (r.rule == TI.REJECTED) & (r.prev_w == 0) & (r.new_w == 0), "some")
            _case("sdf-mode%d-set%s-skip%d" % (_mode, "AB"[_variant], _skip), "sdf-thresholds",
                  dict(weighting_mode=_mode, tsdf_weighting_variant=_variant, tsdf_skip_at_negative_truncation=_skip, depth_interp_nearest=_mode % 2, max_weight=1.75),
                  CAM_CENTRE, [_stripe_image()] * 2, targets=_t)
for _mode in (1, 3):
    _case("sdf-mode%d-setB-one-voxel-truncation" % _mode, "sdf-thresholds", dict(weighting_mode=_mode, tsdf_weighting_variant=1, truncation_distance_vox=1.0),
          CAM_CENTRE, [_stripe_image()] * 2,
          targets={"sdf = -trunc = -voxel": (lambda r: _on(r, z=1.0) & (r.ds - r.z == -VOXEL) & (r.rule != TI.OUTSIDE), "some"),
                   "sdf = 0": (lambda r: _on(r, z=1.0) & (r.ds == 1.0) & (r.rule == TI.FUSED), "some")})

# ------------------------------------------------------------------------------------------------ prior
PRIOR_ROWS = [("at max_weight", 0.125, 5.0), ("reaches max_weight", -0.0625, 4.0), ("weight 0 with a distance", 0.1, 0.0), ("at +trunc", 0.25, 2.0),
              ("at -trunc", -0.25, 2.0), ("over max_weight", 0.0, 7.0), ("fresh", 0.0, 0.0), ("light", 0.2, 0.5)]


def _prior_blocks():
    idx, vox = prior_box(*FRUSTUM_BOX)
    v = vox.reshape(len(idx), 8, 8, 8)                       # [x][y][z]
    for k, (_, d, w) in enumerate(PRIOR_ROWS):
        v["distance"][:, k] = d; v["weight"][:, k] = w        # voxel column x = k of every block
    return idx, vox


def _prior_targets():
    t = {}
    for _, d, w in PRIOR_ROWS:
        t["prior {%g, %g} fused" % (d, w)] = (lambda r, d=F(d), w=F(w): r.exact & (r.prev_d == d) & (r.prev_w == w) & (r.rule == TI.FUSED), "some")
    t["reaches max_weight exactly"] = (lambda r: r.exact & (r.prev_w == 4.0) & (r.new_w == 5.0), "some")
    return t


for _before in (0, 1):
    for _mode in (0, 2):
        _t = _prior_targets()
        if _mode:
            del _t["reaches max_weight exactly"]
        _case("prior-clamp%d-mode%d" % (_before, _mode), "prior", dict(tsdf_weight_clamp_before_blend=_before, weighting_mode=_mode, max_weight=5.0), CAM_CENTRE,
              _const(1.125), prior=_prior_blocks(), targets=_t)

# ------------------------------------------------------------------------------------------------ step
def _step_image(cam=CAM_CORNER, near=1.0, far=2.0, bad=0.0):
    img = _const(near, cam)
    img[:cam[5] // 2, cam[4] // 2:] = far
    img[cam[5] // 2:, cam[4] // 2:] = bad
    return img


def _step_targets():
    mixed = lambda r: r.exact & TI.tap_valid(r.taps).all(0) & (r.taps.max(0) != r.taps.min(0)) & (r.rule != TI.OUTSIDE)
    return {"taps straddle the 1 m / 2 m edge": (mixed, "some"),
            "straddles with real weights": (lambda r: mixed(r) & ((r.ax == 0.5) | (r.ay == 0.5)), "some"),
            "taps straddle an edge to invalid depth": (lambda r: r.exact & (r.rule == TI.INVALID) & TI.tap_valid(r.taps).any(0), "some"),
            "all taps invalid": (lambda r: r.exact & (r.rule == TI.INVALID) & ~TI.tap_valid(r.taps).any(0) & (r.prev_w > 0), "some")}


for _decay in (0.0, 0.5, 1.0):
    _case("step-decay%g" % _decay, "step", dict(invalid_depth_decay_factor=_decay), CAM_CORNER, _step_image(), prior=prior_box(*FRUSTUM_BOX), targets=_step_targets())
_case("step-no-decay-centre", "step", {}, CAM_CENTRE, _step_image(CAM_CENTRE, bad=np.nan), prior=prior_box(*FRUSTUM_BOX),
      targets={"taps straddle an edge to invalid depth": _step_targets()["taps straddle an edge to invalid depth"]})

# ------------------------------------------------------------------------------------------------ tiny
for _rows, _cols in ((1, 1), (1, 7), (2, 2), (3, 5)):
    for _sub in (1, 4):
        for _nearest in (0, 1):
            _cam = (2.0, 2.0, _cols / 2.0, _rows / 2.0, _cols, _rows)
            _fuses = _nearest or (_rows > 1 and _cols > 1)
            _case("tiny-%dx%d-sub%d-%s" % (_rows, _cols, _sub, "nearest" if _nearest else "bilinear"), "tiny",
                  dict(raycast_subsampling_factor=_sub, depth_interp_nearest=_nearest), _cam, np.full((_rows, _cols), 1.5, F),
                  targets={"fused": (lambda r: r.rule == TI.FUSED, "some" if _fuses else "none"), "exact and seen": (lambda r: r.exact & (r.u >= 0) & (r.u <= 8), "some")})

# ------------------------------------------------------------------------------------------------ single-ray
def _one_pixel(row, col, depth):
    img = np.zeros((3, 3), F); img[row, col] = depth
    return img


_RAY_CAM = (1.0, 1.0, 1.5, 1.5, 3, 3)              # the centre pixel looks along the axis, (1, 2) along a face diagonal, (2, 2) along the space diagonal
_FLIP = [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]        # looks along -z
for _name, _px, _t0, _R in (("axis", (1, 1), (0, 0, 0), None), ("face-diagonal", (1, 2), (0, 0, 0), None), ("space-diagonal", (2, 2), (0, 0, 0), None),
                            ("axis-from-negative-corner", (1, 1), (-1, -1, -1), None), ("general-negative", (0, 2), (-0.21875, -0.40625, -0.09375), _FLIP)):
    _case("single-ray-" + _name, "single-ray", dict(depth_interp_nearest=1), _RAY_CAM, _one_pixel(_px[0], _px[1], 1.75), poses=[pose(_t0, _R)], exact=(),
          targets={"fused": (lambda r: r.rule == TI.FUSED, "some")})

# ------------------------------------------------------------------------------------------------ oblique (not exact)
def _rot(yaw, pitch, roll):
    y, p, r = np.radians([yaw, pitch, roll])
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
    return Rz @ Ry @ Rx


def _oblique_image(cols=64, rows=48):
    rng = np.random.default_rng(37)
    c, r = np.meshgrid(np.arange(cols), np.arange(rows))
    img = 1.6 + 0.006 * (c - cols / 2) - 0.009 * (r - rows / 2) + rng.normal(0.0, 0.005, (rows, cols))      # a tilted plane, 5 mm noise
    for pr in range(4, rows - 3, 9):
        for pc in range(4 + 6 * ((pr // 9) % 2), cols - 3, 12):
            img[pr:pr + 3, pc:pc + 3] = 0.0                                                               # a checkerboard of invalid 3 x 3 patches
    return img.astype(F)


OBLIQUE_CAM = (44.0, 38.0, 31.25, 24.75, 64, 48)
for _kw in ({}, dict(invalid_depth_decay_factor=0.5, weighting_mode=3)):
    _case("oblique" + ("-decay-mode3" if _kw else ""), "oblique", dict(voxel_size=0.05, **_kw), OBLIQUE_CAM, [_oblique_image(), _oblique_image()[::-1, ::-1]],
          poses=[pose((-3.3, -2.7, -1.1), _rot(37, -21, 13))] * 2, exact=(),
          targets={"fused": (lambda r: r.rule == TI.FUSED, "some"), "invalid": (lambda r: r.rule == TI.INVALID, "some"), "rejected": (lambda r: r.rule == TI.REJECTED, "some")})

# ------------------------------------------------------------------------------------------------ occupancy
_OCC = dict(projective_layer_type=1, occupied_region_half_width_m=0.125)
_LOG_ODDS_BOX = prior_box(*FRUSTUM_BOX, d=F(0.375), w=F(0.0))
_case("occupancy-border", "occupancy", _OCC, CAM_CORNER, _rim(_const(2.5), 0.0), prior=_LOG_ODDS_BOX, targets=_border_targets(COLS, ROWS, 0, True))
_case("occupancy-centre-taps", "occupancy", _OCC, CAM_CENTRE, _centre_image(), prior=_LOG_ODDS_BOX, targets=_centre_targets())
_t = _patch_targets(); del _t["observed free before"]
_case("occupancy-tap-values", "occupancy", _OCC, CAM_CENTRE, [_const(1.5), _patch_image()], prior=_LOG_ODDS_BOX, targets=_t)
_case("occupancy-step", "occupancy", _OCC, CAM_CORNER, [_step_image(), _step_image()],
      targets={k: v for k, v in _step_targets().items() if k != "all taps invalid"})
_case("occupancy-thresholds", "occupancy", _OCC, CAM_CENTRE, [_stripe_image()] * 3,
      targets={"vd = ds - half width": (lambda r: _on(r, z=1.0) & (r.ds == 1.125) & (r.taps == r.taps[0]).all(0) & (r.new_d > r.prev_d), "some"),
               "vd = ds + half width": (lambda r: _on(r, z=1.0) & (r.ds == 0.875) & (r.taps == r.taps[0]).all(0) & (r.new_d > r.prev_d), "some"),
               "free": (lambda r: r.exact & (r.new_d < r.prev_d), "some"), "behind, unobserved": (lambda r: r.exact & (r.rule == TI.FUSED) & (r.new_d == r.prev_d), "some")})

# ------------------------------------------------------------------------------------------------ u16
def _mm(img):
    out = np.round(np.where(np.isfinite(img), img, 0.0) * 1000.0)
    return np.clip(out, 0, 65535).astype(np.uint16)


_u16_border = _mm(_rim(_const(2.5, CAM_CORNER), 0.0)); _u16_border[0, ::2] = 65535; _u16_border[::2, -1] = 65535
_case("u16-border", "u16", dict(invalid_depth_decay_factor=0.5), CAM_CORNER, _u16_border, prior=prior_box(*FRUSTUM_BOX),
      targets={"u = 1/2": (lambda r: _on(r, u=0.5) & (r.rule != TI.OUTSIDE), "some"), "a tap of 0": (lambda r: r.exact & (r.taps == 0).any(0) & (r.rule == TI.INVALID), "some"),
               "a tap of 65535": (lambda r: r.exact & (r.taps > 65.0).any(0) & (r.rule != TI.OUTSIDE), "some")})
_u16_step = _mm(_step_image()); _u16_step[2:5, 2:5] = 65535
_case("u16-step", "u16", dict(invalid_depth_decay_factor=0.5), CAM_CORNER, _u16_step, prior=prior_box(*FRUSTUM_BOX),
      targets={"taps straddle the edge": (lambda r: r.exact & TI.tap_valid(r.taps).all(0) & (r.taps.max(0) != r.taps.min(0)) & (r.rule != TI.OUTSIDE), "some"),
               "all taps 65535": (lambda r: r.exact & (r.taps > 65.0).all(0) & (r.rule == TI.FUSED), "some"),
               "a tap of 0": (lambda r: r.exact & (r.taps == 0).any(0) & (r.rule == TI.INVALID), "some")})

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FAMILIES = sorted({c.family for c in CASES})


# ------------------------------------------------------------------------------------------------ running a case
def params(M, case, **more):
    return M.default_params(**dict(case.kw, **more))


def frames_of(case):
    return list(zip(case.depths, case.poses))


def batch_partner(case):
    """the second frame of the batch-of-two launch: the same rotation from a pose one block to the side (exact layers stay exact layers), a plane at 1.25 m"""
    T = case.poses[-1].copy()
    T[:3, 3] += T[:3, :3] @ np.asarray([0.5, 0.0, 0.0], F)
    img = np.full(case.depths[-1].shape, 1.25, F)
    img[2::5, 3::7] = 0.0
    return (_mm(img) if case.depths[-1].dtype == np.uint16 else img), T


def exact_mask(case, key, frames):
    """the exact voxels of block `key`: on an exact layer of every frame, and wherever all four taps are valid they are equal or short dyadic numbers (so
    that the weights 0 and 1/2 blend them without rounding)"""
    if not case.exact_depths:
        return np.zeros(512, bool)
    m = np.ones(512, bool)
    vs = float(F(case.kw["voxel_size"]))
    for image, T in frames:
        pc, u, v = TI.voxel_geometry(key, T, case.cam, vs)
        _, taps, _, _ = TI.sample_depth(as_metres(image), u, v, int(case.kw.get("depth_interp_nearest", 0)))
        with np.errstate(invalid="ignore", over="ignore"):
            short = (np.abs(taps) < 64.0) & (taps * 4096.0 == np.round(taps * 4096.0))
            same = (taps == taps[0]).all(0)
        m &= np.isin(pc[:, 2], case.exact_depths) & (~TI.tap_valid(taps).all(0) | short.all(0) | same)
    return m


def stays_free(r):
    """voxels of a Report that were observed free and none of whose valid taps measures a surface at or in front of them: whatever the other taps hold,
    such a voxel cannot end with a negative distance"""
    with np.errstate(invalid="ignore"):
        return (r.prev_w > 0) & (r.prev_d > 0) & ~(TI.tap_valid(r.taps) & (r.taps <= r.z + TRUNC)).any(0)


def prior_map(case):
    if case.prior is None:
        return {}
    return {tuple(int(v) for v in i): (vox["distance"].astype(np.float64), vox["weight"].astype(np.float64)) for i, vox in zip(*case.prior)}


def run_model(case, p, frames, views):
    """The float64 model over `frames` in order, each applied to the blocks of its view (views[i]: what a view calculation named for frame i).
    -> (map {block: (distance, weight)}, robust {block: mask}, exact {block: mask}, Report of the last frame)"""
    model = prior_map(case); robust = {}; exact = {}
    rep = None
    for i, ((image, T), view) in enumerate(zip(frames, views)):
        img = as_metres(image)
        rows = []
        for key in sorted(view):
            pd_, pw_ = model.get(key, (np.zeros(512), np.zeros(512)))
            if key not in exact:
                exact[key] = exact_mask(case, key, frames)
            nd, nw, rule, rob = TI.update_block_rules(pd_, pw_, key, img, T, case.cam, p, exact=exact[key])
            model[key] = (nd, nw); robust[key] = robust.get(key, np.ones(512, bool)) & rob
            if i == len(frames) - 1:
                pc, u, v = TI.voxel_geometry(key, T, case.cam, float(p.voxel_size))
                nearest = int(p.depth_interp_nearest)
                _, taps, ds, _ = TI.sample_depth(img, u, v, nearest)
                ax = np.zeros(512) if nearest else (u - 0.5) - np.floor(u - 0.5); ay = np.zeros(512) if nearest else (v - 0.5) - np.floor(v - 0.5)
                rows.append((np.repeat(np.asarray([key]), 512, 0), u, v, pc[:, 2], rule, exact[key], taps, ax, ay, ds, pd_, pw_, nd, nw))
        if rows:
            cat = lambda k: np.concatenate([r[k] for r in rows], 1 if k == 6 else 0)
            rep = Report(*[cat(k) for k in range(14)])
    return model, robust, exact, rep


def run_checker(oracle_mod, H, case, p, frames):
    """the CPU checker over the same frames -> (OracleMap, [view of frame i as a set of tuples], its map {block: voxels [512]} before the last frame)"""
    o = oracle_mod.OracleMap(H.copy_params(p, oracle_mod.OrcParams))
    if case.prior is not None:
        for i, vox in zip(*case.prior):
            o.set_block(oracle_mod.L_TSDF, i, vox)
    views = []
    for k, (image, T) in enumerate(frames):
        if k == len(frames) - 1:
            before = checker_map(oracle_mod, o)
        o.integrate_depth(as_metres(image), T, case.cam)
        views.append({tuple(int(v) for v in r) for r in np.asarray(o.last_view()).reshape(-1, 3)})
    return o, views, before


def checker_map(oracle_mod, o):
    return {tuple(int(v) for v in i): o.get_block(oracle_mod.L_TSDF, i).copy() for i in np.asarray(o.block_indices(oracle_mod.L_TSDF)).reshape(-1, 3)}
