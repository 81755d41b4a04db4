"""The drawn masks of tests/mask_patterns.py on the CPU checker: for every pattern x size x threshold that tests/test_gpu_dynamic_masks.py feeds to
the fused dynamic-mask front end, (1) the steering recipe makes OracleMap.detect_dynamics return the drawn pattern bit for bit, (2) the checker's
remove_small_components equals scipy's 8-connected size filter and (3) its split equals the split the cleaned mask dictates.  So the inputs do what
the GPU test assumes, and the checker itself has met the adversarial shapes (until now it had met scipy on random masks only)."""
import os
import re

import numpy as np
import pytest

import mask_patterns as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)

# the call sequences of the GPU file: (pattern, min_component_size) on ONE mapper at SEQUENCE_SIZE, then image sizes in turn on one mapper
SEQUENCE_SIZE = (120, 160)
SEQUENCE = (("random0.60", 40), ("zeros", 40), ("serpentine", 40), ("random0.42", 0), ("random0.60", 40), ("corner_nwse_touching", P.ENCOUNTER_MIN_SIZE))
RESIZE_SEQUENCE = (((15, 61), "staircase_nesw", 9), ((61, 15), "random0.42", 9), ((61, 15), "serpentine", 2), ((120, 160), "random0.42", 40),
                   ((15, 61), "corner_nesw_touching", P.ENCOUNTER_MIN_SIZE), ((15, 61), "random0.60", 9))
RESIZE_SIZES = ((15, 61), (61, 15), (120, 160))


def masked_depth_invalid():
    """NVBX_MASKED_DEPTH_INVALID as include/nvblox_hip.h documents it."""
    with open(os.path.join(ROOT, "include", "nvblox_hip.h")) as f:
        m = re.search(r"#define\s+NVBX_MASKED_DEPTH_INVALID\s+\(?\s*(-?[0-9.]+)f?\s*\)?", f.read())
    return float(m.group(1))


_checkers = {}


def checker(oracle_mod, sizes, params=None):
    """An OracleMap steered for the cameras of `sizes`: one 4.0 m wall frame each from the identity pose at time 0 (shared, never changed again:
    detect_dynamics only reads it)."""
    key = tuple(sizes)
    if key not in _checkers:
        o = oracle_mod.OracleMap(params or oracle_mod.default_params(**P.STEER_PARAMS))
        o.set_time_ms(0)
        for rows, cols in key:
            o.integrate_depth(P.wall_depth(rows, cols), EYE, P.CAMERAS[(rows, cols)])
        _checkers[key] = o
    return _checkers[key]


def check_case(oracle_mod, o, size, name, pattern, background, thresholds):
    cam = P.CAMERAS[size]
    invalid = masked_depth_invalid()
    depth = P.steering_depth(pattern, background)
    raw = o.detect_dynamics(depth, EYE, cam, P.MAX_DISTANCE_M)
    assert np.array_equal(raw, pattern.astype(np.uint8)), (size, name, "steering", int(raw.sum()), int(pattern.sum()))
    for thr in thresholds:
        want = P.filter_model(pattern, thr)
        cleaned = oracle_mod.remove_small_components(raw, thr)
        assert np.array_equal(cleaned, want.astype(np.uint8)), (size, name, thr, "filter", int(cleaned.sum()), int(want.sum()))
        un, ma = oracle_mod.split_depth_by_mask(depth, cleaned, EYE, cam, cam, P.OCCLUSION_THRESHOLD_M)
        wu, wm = P.split_model(depth, want, invalid)
        assert np.array_equal(un, wu) and np.array_equal(ma, wm), (size, name, thr, "split")
        assert np.array_equal(ma > 0, want) and np.array_equal(un[~want], depth[~want])


def test_invalid_depth_value_is_the_documented_one():
    assert masked_depth_invalid() == -1.0


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_steering_reproduces_the_pattern_and_the_checker_equals_scipy(oracle_mod, size):
    o = checker(oracle_mod, (size,))
    cs = P.cases(*size)
    assert len(cs) >= 11
    for name, pattern, background, thresholds in cs:
        check_case(oracle_mod, o, size, name, pattern, background, thresholds)


def test_full_resolution_cases(oracle_mod):
    o = checker(oracle_mod, (P.FULL_RES,))
    for name, pattern, background, thresholds in P.full_res_cases():
        check_case(oracle_mod, o, P.FULL_RES, name, pattern, background, thresholds)


def test_call_sequences_use_cases_of_the_table():
    """Every step of the GPU file's call sequences is a (pattern, threshold) pair the table holds, i.e. one the tests above have checked."""
    for size, name, thr in [(SEQUENCE_SIZE, n, t) for n, t in SEQUENCE] + list(RESIZE_SEQUENCE):
        hits = [c for c in P.cases(*size) if c[0] == name]
        assert len(hits) == 1 and thr in hits[0][3], (size, name, thr)


def test_one_map_steered_for_three_cameras(oracle_mod):
    """The size-change sequence runs on ONE mapper: wall frames of all three cameras, then each camera's patterns come out as drawn."""
    o = checker(oracle_mod, RESIZE_SIZES)
    for size, name, thr in RESIZE_SEQUENCE:
        c = [c for c in P.cases(*size) if c[0] == name][0]
        check_case(oracle_mod, o, size, name, c[1], c[2], (thr,))
