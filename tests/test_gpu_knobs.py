"""The NVBX_* knobs belong to a mapper: read when it is created, read again by reload_knobs (nvbx_mapper_reload_knobs), and never
frozen for the process.  Two mappers of one process run under different settings and hold the same map bit for bit; a reload changes the launch
structure of a live mapper and changes it back; the variables that shape a mapper at creation are not re-applied to a live one.  The launch
structure is read off the profile: the fused TSDF + colour launch, k_integrate_tsdf_color<..>, runs only with NVBX_FUSE_COLC on and a colour
frame held back."""
import pytest

import helpers as H

pytestmark = pytest.mark.gpu
CAM = H.SMALL_CAM
SETTING = {"NVBX_FUSE_COLC": "0", "NVBX_INTEG_GRID": "8", "NVBX_DECAY_GRID": "1", "NVBX_MARK_RIDERS": "8"}


@pytest.fixture(scope="module")
def frames():
    return H.frames(8, CAM, stride=25)      # (half of the 200-pose loop in four frames: 113 ESDF blocks, the smallest layer, after the decay)


@pytest.fixture
def unset(monkeypatch):
    for name in tuple(SETTING) + ("NVBX_COLOR_DEFERRAL",):
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def new_mapper():
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(tsdf_decay_factor=0.8, tsdf_decayed_weight_threshold=0.05), block_capacity=1 << 13)
    m.set_profiling(True)
    return m


def feed(m, frames):
    for d, rgb, T in frames:
        m.integrate_depth(d, T, CAM)
        m.integrate_color(rgb, T, CAM)
        m.update_esdf()


def fused_launches(m):
    return sum(v["count"] for k, v in m.profile().items() if "k_integrate_tsdf_color<" in k)


def test_each_mapper_keeps_the_knobs_it_was_created_under_and_a_reload_replaces_them(hip_lib, frames, unset):
    a = new_mapper()
    for name, value in SETTING.items():
        unset.setenv(name, value)
    b = new_mapper()
    for name in SETTING:
        unset.delenv(name)
    c = new_mapper()                                       # (as a, and never reloaded)
    for m in (a, b, c):
        feed(m, frames[:4]); m.decay_tsdf(True)
    H.assert_same_map(a, b, "created under other knobs", min_blocks=101, slice=True)
    n_a = fused_launches(a)
    assert n_a == 3 and fused_launches(b) == 0 and fused_launches(c) == 3      # (frames 2 .. 4 each carry the colour frame before them)
    # reload: the fused launch goes away and comes back on the live mapper
    unset.setenv("NVBX_FUSE_COLC", "0")
    a.reload_knobs()
    feed(a, frames[4:6])
    assert fused_launches(a) == n_a
    unset.delenv("NVBX_FUSE_COLC")
    a.reload_knobs()
    feed(a, frames[6:8])
    assert fused_launches(a) == n_a + 1                    # (the reload carried frame 6's colour out: frame 8 carries frame 7's)
    feed(c, frames[4:8])
    assert fused_launches(c) == n_a + 3                    # (the decay carried frame 4's colour out: frames 6 .. 8 carry)
    feed(b, frames[4:8])
    assert fused_launches(b) == 0                          # (b never saw the environment change)
    for m in (a, b, c):
        m.update_esdf()
    H.assert_same_map(a, c, "reloaded twice against never reloaded", min_blocks=101, slice=True)
    H.assert_same_map(b, c, "other knobs to the end", min_blocks=101, slice=True)
    assert a.counters()["capacity_overflow"] == 0


def test_a_reload_does_not_reapply_what_shapes_a_mapper_at_creation(hip_lib, frames, unset):
    kept = new_mapper()                                    # creation left colour deferral on
    off = new_mapper(); off.set_color_deferral(False)      # the setter switched it off
    unset.setenv("NVBX_COLOR_DEFERRAL", "0")
    kept.reload_knobs()
    feed(kept, frames[:2])
    assert fused_launches(kept) == 1                       # frame 1's colour was still held back: frame 2's depth carried it in the fused launch
    unset.setenv("NVBX_COLOR_DEFERRAL", "2")
    off.reload_knobs()
    feed(off, frames[:2])
    assert fused_launches(off) == 0
    unset.setenv("NVBX_COLOR_DEFERRAL", "0")
    created_off = new_mapper()                             # (the variable does reach a mapper created under it)
    feed(created_off, frames[:2])
    assert fused_launches(created_off) == 0
    H.assert_same_map(kept, off, "deferral on and off", slice=True)
