"""The feature layer's independent model (tests/feature_independent.py) on hand-made cases whose answer is known in closed form.  No GPU."""
import numpy as np

import feature_independent as FI

F = np.float32
CAM = (40.0, 40.0, 39.5, 29.5, 80, 60)
EYE = np.eye(4, dtype=np.float32)      # camera frame = layer frame: z forward
BLOCK = (0, 0, 2)                      # z from 0.8 to 1.2 m in front of the camera, x and y from 0 to 0.4 m: inside the image
WALL_Z = 1.0                           # between two voxel centres: every voxel of the block is within 0.175 m of it


def frame(state, rules, feat, stride, synth_depth=WALL_Z, band=True):
    sub = rules.sub
    synth = np.full((CAM[5] // sub, CAM[4] // sub), synth_depth, np.float32)
    return FI.integrate(state, rules, np.array([BLOCK]), [band], synth, EYE, CAM, stride, feat)


def voxel_depths():
    t = np.arange(512)
    return (F(0.8) + (t & 7).astype(F) * F(0.05) + F(0.025)).astype(F)


def test_constant_image_gives_the_constant_and_weight_k():
    rules = FI.Rules(max_weight=100.0)
    feat = np.full((15, 20, 8), 0.5, np.float16)
    state = {}
    for k in range(1, 5):
        frame(state, rules, feat, 4)
        vals, w = state[BLOCK]
        assert (w == k).all()             # every voxel of the block lies within the truncation distance of the wall and inside the grid
        assert (vals == np.float16(0.5)).all()


def test_a_voxel_beyond_the_occlusion_threshold_is_untouched():
    rules = FI.Rules(occlusion_threshold_m=0.06)
    feat = np.full((15, 20, 8), 2.0, np.float16)
    state = frame({}, rules, feat, 4)
    vals, w = state[BLOCK]
    near = np.abs(voxel_depths() - F(WALL_Z)) < 0.05       # depths 0.975 and 1.025 (0.025 m off); the next ones are 0.075 m off
    assert near.sum() == 2 * 64
    assert (w[near] == 1).all() and (vals[near] == 2).all()
    assert (w[~near] == 0).all() and (vals[~near] == 0).all()
    # no synthetic depth at all (nothing was hit): nothing is reached, the block does not join the layer
    assert frame({}, rules, feat, 4, synth_depth=0.0) == {}
    # a block outside the truncation band is no candidate
    assert frame({}, rules, feat, 4, band=False) == {}


def test_taps_on_the_last_row_or_column_are_accepted_and_one_past_it_is_refused():
    rows_f, cols_f, stride = 15, 20, 4
    # u = 78: uf = 19 -> taps 19, 20 (one past the last column 19); u = 77.9: taps 18, 19
    ok, x0, y0, ax, ay = FI.feature_taps([78.0, 77.9, 74.0, 10.0, 10.0, 10.0, 1.9, 2.0], [10.0, 10.0, 10.0, 58.0, 57.9, 54.0, 10.0, 10.0], stride, rows_f, cols_f)
    assert ok.tolist() == [False, True, True, False, True, True, False, True]
    assert x0[1] == 18 and x0[2] == 18 and ax[2] == 0 and y0[4] == 13 and y0[5] == 13 and ay[5] == 0 and x0[7] == 0 and ax[7] == 0
    # the accepted tap really reads the last column / row: an image that is 1 there and 0 elsewhere
    feat = np.zeros((rows_f, cols_f, 8), np.float32); feat[:, cols_f - 1] = 1.0
    f = FI.bilinear(ax[1], ay[1], feat[y0[1], x0[1]], feat[y0[1], x0[1] + 1], feat[y0[1] + 1, x0[1]], feat[y0[1] + 1, x0[1] + 1])
    assert np.allclose(f, ax[1]) and ax[1] > 0.9


def test_stride_one_with_x0_on_the_last_column_is_refused():
    ok, x0, _, _, _ = FI.feature_taps([79.5, 79.4, 80.0], [10.0, 10.0, 10.0], 1, 60, 80)
    assert x0.tolist() == [79, 78, 79] and ok.tolist() == [False, True, False]
    ok, _, y0, _, _ = FI.feature_taps([10.0, 10.0], [59.5, 59.4], 1, 60, 80)
    assert y0.tolist() == [59, 58] and ok.tolist() == [False, True]


def test_max_weight_clamp():
    rules = FI.Rules(max_weight=2.0)
    state = {}
    for v in (1.0, 3.0, 9.0):
        frame(state, rules, np.full((15, 20, 8), v, np.float16), 4)
    vals, w = state[BLOCK]
    assert (w == 2).all()
    # 1 -> (1 + 3) / 2 = 2 -> weight clamped at 2 -> 2 * (2 / 3) + 9 * (1 / 3): 4.3333 in f32, 4.332 in fp16
    assert (vals == np.float16(F(2) * (F(2) / F(3)) + F(9) * (F(1) / F(3)))).all()
    assert vals[0, 0] == np.float16(4.332)


def test_a_blend_exactly_between_two_fp16_values_rounds_to_even():
    ulp = 2.0 ** -10      # fp16 spacing in [1, 2)
    # w0 = 1: v = (old + f) / 2, exact in f32
    for old, f, want in ((1.0, 1.0 + ulp, 1.0),                           # 1 + ulp / 2: between mantissa 0 (even) and 1
                         (1.0 + ulp, 1.0 + 2 * ulp, 1.0 + 2 * ulp),       # 1 + 1.5 ulp: between 1 and 2 (even)
                         (1.0 + 2 * ulp, 1.0 + 3 * ulp, 1.0 + 2 * ulp),   # 1 + 2.5 ulp: between 2 (even) and 3
                         (-1.0 - 2 * ulp, -1.0 - 3 * ulp, -1.0 - 2 * ulp)):
        v, w = FI.blend(np.float16([old]), F(1), F(f), 5.0)
        assert F(0.5) * F(old) + F(0.5) * F(f) == F((old + f) / 2)       # the tie is exact in f32
        assert v[0] == np.float16(want) and w == 2, (old, f, v)
    # through a whole frame: a constant image lands on the tie in the voxels whose horizontal and vertical tap weights are exact
    rules = FI.Rules()
    state = frame({}, rules, np.full((15, 20, 8), 1.0, np.float16), 4)
    frame(state, rules, np.full((15, 20, 8), 1.0 + ulp, np.float16), 4)
    vals, w = state[BLOCK]
    assert (w == 2).all() and set(np.unique(vals).tolist()) <= {1.0, 1.0 + ulp}
    assert (vals == 1.0).any()
