"""The fused dynamic-mask front end (nvbx_dynamic_depth_split: k_dyn_detect_union -> k_cc_count -> k_dyn_filter_split, csrc/dynamics.hip) on masks
DRAWN to break it.  The call computes its own mask, so the mask is steered (tests/mask_patterns.py: a mapper that has seen one 4.0 m wall holds
high-confidence freespace everywhere in view; a depth image of 1.5 m on a pattern makes exactly the pattern dynamic -- proven on the CPU checker
for every case used here by tests/test_mask_patterns.py).  Mapper `a` makes the three separate calls, mapper `b` the fused one; for every case

    b == a == scipy model == CPU checker, bit for bit: cleaned mask, unmasked and masked depth image

at the smallest image sizes at which each rule of the 30 x 7 patch lattice can go wrong, at 480 x 640 once, and over call sequences that
exercise the parity double-buffering of the label / size / nearest-depth arrays (which can only be wrong on the call after next)."""
import numpy as np
import pytest

import helpers as H
import mask_patterns as P
import test_mask_patterns as C

pytestmark = pytest.mark.gpu

EYE = C.EYE


class Pair:
    """Two steered mappers (a: three calls, b: fused) and the steered checker for the cameras of `sizes`."""

    def __init__(self, oracle_mod, sizes):
        import torch
        from isaac_ros_nvblox_amd import mapper as M
        self.torch, self.oracle_mod, self.dev = torch, oracle_mod, torch.device("cuda", 0)
        pg = M.default_params(**P.STEER_PARAMS)
        self.a = M.Mapper(pg, block_capacity=1 << 13); self.b = M.Mapper(pg, block_capacity=1 << 13)
        po = H.copy_params(pg, oracle_mod.OrcParams)
        self.o = C.checker(oracle_mod, tuple(sizes), po)
        assert bytes(self.o.params) == bytes(po)                  # (the shared checker was made with the same parameters)
        for m_ in (self.a, self.b):
            m_.set_time_ms(0)
            for rows, cols in sizes:
                m_.integrate_depth(P.wall_depth(rows, cols), EYE, P.CAMERAS[(rows, cols)])
            m_.synchronize()
        self.invalid = C.masked_depth_invalid()

    def _outputs(self, shape):
        t = self.torch
        return (t.empty(shape, dtype=t.uint8, device=self.dev), t.empty(shape, dtype=t.float32, device=self.dev), t.empty(shape, dtype=t.float32, device=self.dev))

    def three_calls(self, d_dev, cam, thr, m_=None):
        m_ = m_ or self.a
        mk, un, ma = self._outputs(tuple(d_dev.shape))
        m_.detect_dynamics_into(d_dev, EYE, cam, P.MAX_DISTANCE_M, mk)
        m_.remove_small_components_inplace(mk, thr)
        m_.split_depth_by_mask_into(d_dev, mk, EYE, cam, cam, P.OCCLUSION_THRESHOLD_M, un, ma)
        m_.synchronize()
        return mk.cpu().numpy(), un.cpu().numpy(), ma.cpu().numpy()

    def fused(self, d_dev, cam, thr, overlay=False, m_=None):
        m_ = m_ or self.b
        t = self.torch
        mk, un, ma = self._outputs(tuple(d_dev.shape))
        ov = t.empty(tuple(d_dev.shape) + (3,), dtype=t.uint8, device=self.dev) if overlay else None
        m_.dynamic_depth_split_into(d_dev, EYE, cam, P.MAX_DISTANCE_M, thr, P.OCCLUSION_THRESHOLD_M, mk, un, ma, ov)
        m_.synchronize()
        return mk.cpu().numpy(), un.cpu().numpy(), ma.cpu().numpy(), (ov.cpu().numpy() if overlay else None)

    def model(self, pattern, depth, thr):
        kept = P.filter_model(pattern, thr)
        un, ma = P.split_model(depth, kept, self.invalid)
        return kept.astype(np.uint8), un, ma

    def check(self, size, name, pattern, background, thr, overlay=False, checker=True, fused_on=None, repeats=1):
        """One case through both paths, the model and the checker; returns the fused outputs."""
        cam = P.CAMERAS[size]
        depth = P.steering_depth(pattern, background)
        d_dev = self.torch.from_numpy(depth).to(self.dev)
        want = self.model(pattern, depth, thr)
        tag = (size, name, thr)
        for rep in range(repeats):
            got_b = self.fused(d_dev, cam, thr, overlay, fused_on)
            for k, what in enumerate(("mask", "unmasked", "masked")):
                assert np.array_equal(got_b[k], want[k]), tag + ("fused != model", what, rep, int((got_b[k] != want[k]).sum()))
        got_a = self.three_calls(d_dev, cam, thr)
        for k, what in enumerate(("mask", "unmasked", "masked")):
            assert np.array_equal(got_a[k], want[k]), tag + ("three calls != model", what, int((got_a[k] != want[k]).sum()))
            assert np.array_equal(got_b[k], got_a[k]), tag + ("fused != three calls", what)
        if thr == 0:
            assert np.array_equal(got_b[0], pattern.astype(np.uint8)), tag + ("raw mask != drawn pattern",)
        if checker:
            raw = self.o.detect_dynamics(depth, EYE, cam, P.MAX_DISTANCE_M)
            mo = self.oracle_mod.remove_small_components(raw, thr)
            uo, mao = self.oracle_mod.split_depth_by_mask(depth, mo, EYE, cam, cam, P.OCCLUSION_THRESHOLD_M)
            for k, ref in enumerate((mo, uo, mao)):
                assert np.array_equal(got_b[k], ref), tag + ("fused != checker", k)
        if overlay:
            grey, red, decisive = P.overlay_model(depth, want[2] > 0)
            ov = got_b[3]
            assert np.array_equal(ov[..., 1], grey) and np.array_equal(ov[..., 2], grey), tag + ("overlay grey",)
            assert np.array_equal(ov[..., 0][decisive], red[decisive]), tag + ("overlay red",)
            assert np.array_equal((ov[..., 0] == 255) & decisive, (want[2] > 0) & decisive), tag + ("overlay red == 255 exactly on the masked pixels",)
        return got_b


_pairs = {}


def pair(oracle_mod, sizes):
    key = tuple(sizes)
    if key not in _pairs:
        _pairs[key] = Pair(oracle_mod, key)
    return _pairs[key]


@pytest.mark.parametrize("size", P.SIZES, ids=lambda s: "%dx%d" % s)
def test_drawn_masks_fused_equals_three_calls_model_and_checker(oracle_mod, hip_lib, size):
    """Every pattern of the table at every threshold of the size (0, 1, 2, one inside the size distribution, one above the image, and the
    thresholds the encounter / threshold-edge patterns are drawn for); the overlay on every third call."""
    pr = pair(oracle_mod, (size,))
    n = 0
    for name, pattern, background, thresholds in P.cases(*size):
        for thr in thresholds:
            pr.check(size, name, pattern, background, thr, overlay=(n % 3 == 0))
            n += 1
    assert n >= 33


def test_full_resolution_once(oracle_mod, hip_lib):
    """480 x 640: the percolation-density random mask and the serpentine (one label chain through all 1 518 patches) at two thresholds, each
    submitted five times: the union is racy by design, its result must not be."""
    pr = pair(oracle_mod, (P.FULL_RES,))
    for name, pattern, background, thresholds in P.full_res_cases():
        for k, thr in enumerate(thresholds):
            pr.check(P.FULL_RES, name, pattern, background, thr, overlay=(k == 0), repeats=5)


@pytest.mark.parametrize("overlay_on", [(), (1, 2, 5)], ids=["no_overlay", "overlay_on_some_calls"])
def test_six_fused_calls_in_a_row_on_one_mapper(oracle_mod, hip_lib, overlay_on):
    """dense -> empty -> serpentine -> filter off (no k_cc_count) -> dense -> corner encounters on ONE mapper, twice over (twelve consecutive
    calls, so each pattern meets both parities): what a call leaves in the arrays of its parity is cleared by the NEXT call and met by the one
    after that."""
    size = C.SEQUENCE_SIZE
    pr = Pair(oracle_mod, (size,))
    table = {c[0]: c for c in P.cases(*size)}
    for rnd in range(2):
        for k, (name, thr) in enumerate(C.SEQUENCE):
            _, pattern, background, _ = table[name]
            pr.check(size, name, pattern, background, thr, overlay=(k in overlay_on), checker=False)
    # an odd number of calls more, so that the sequence also runs with the parities swapped
    pr.check(size, "zeros", table["zeros"][1], "far", 40, checker=False)
    for k, (name, thr) in enumerate(C.SEQUENCE):
        pr.check(size, name, table[name][1], table[name][2], thr, overlay=(k in overlay_on), checker=False)


def test_image_size_changes_on_one_mapper(oracle_mod, hip_lib):
    """15 x 61 then 61 x 15 on the same mapper: the pixel count is the same, so the scratch arrays are NOT re-initialised (their resting state
    must not depend on the shape); then 120 x 160 and back to 15 x 61, which does re-initialise."""
    pr = pair(oracle_mod, C.RESIZE_SIZES)
    for rnd in range(2):
        for size, name, thr in C.RESIZE_SEQUENCE:
            _, pattern, background, _ = [c for c in P.cases(*size) if c[0] == name][0]
            pr.check(size, name, pattern, background, thr, overlay=(rnd == 1))


def test_separate_component_filter_interleaved_with_fused_calls(oracle_mod, hip_lib):
    """nvbx_remove_small_components (k_cc_union, its own scratch arrays and parity) between fused calls on the SAME mapper: neither disturbs
    the other."""
    size = (22, 90)
    pr = Pair(oracle_mod, (size,))
    table = {c[0]: c for c in P.cases(*size)}
    steps = (("random0.42", 12, "lattice_grid"), ("serpentine", 2, "random0.60"), ("lattice_grid", 12, "staircase_nesw"), ("zeros", 12, "random0.42"),
             ("corner_nesw_touching", P.ENCOUNTER_MIN_SIZE, "serpentine_columns"), ("random0.60", 0, "comb"), ("comb_mirrored", 12, "spiral"))
    for name, thr, other in steps:
        other = table[other]
        for thr2 in (thr, 9):
            got = pr.a.remove_small_components(other[1].astype(np.uint8), thr2).cpu().numpy()
            assert np.array_equal(got, P.filter_model(other[1], thr2).astype(np.uint8)), (other[0], thr2)
            pr.check(size, name, table[name][1], table[name][2], thr, checker=False, fused_on=pr.a)


@pytest.mark.parametrize("size", [(15, 61), (120, 160)], ids=lambda s: "%dx%d" % s)
def test_same_input_five_times_gives_five_identical_outputs(oracle_mod, hip_lib, size):
    pr = pair(oracle_mod, (size,))
    table = {c[0]: c for c in P.cases(*size)}
    for name in ("random0.42", "serpentine", "serpentine_columns", "spiral", "lattice_grid", "staircase_nwse", "staircase_nesw", "comb", "corner_nesw_touching", "bridges"):
        thr = P.BRIDGE_MIN_SIZE if name == "bridges" else P.THRESHOLDS[size][3]
        first = pr.check(size, name, table[name][1], table[name][2], thr, checker=False)
        for rep in range(4):
            again = pr.fused(pr.torch.from_numpy(P.steering_depth(table[name][1], table[name][2])).to(pr.dev), P.CAMERAS[size], thr)
            for k in range(3):
                assert np.array_equal(first[k], again[k]), (size, name, rep, k)
