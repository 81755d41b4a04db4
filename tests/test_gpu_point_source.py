"""The point source of the calls that read a sensor cloud against the map (csrc/nvbx_point_source.h): the refusals the seven entry points share --
nvbx_align_points / _depth, nvbx_linearize_points, nvbx_score_poses_points / _depth, nvbx_relocalize_points / _depth -- by their exact text and in
their order, on the raw C-ABI.  The map is a corner of the smoke-sized room: a 160 x 120 camera, two frames, block_capacity 1 << 13."""
import ctypes as C

import numpy as np
import pytest

import align_independent as A

pytestmark = pytest.mark.gpu

ENTRIES = {      # the arguments behind the mapper, by the names of `good` below
    "nvbx_align_points": ("pts", "n", "T", "ao", "res"),
    "nvbx_align_depth": ("depth", "rows", "cols", "T", "cam", "ao", "res"),
    "nvbx_linearize_points": ("pts", "n", "T", "ao", "res", "out_p", "out_r", "out_g", "out_v"),
    "nvbx_score_poses_points": ("pts", "n", "poses", "k", "so", "rec"),
    "nvbx_score_poses_depth": ("depth", "rows", "cols", "cam", "poses", "k", "so", "rec"),
    "nvbx_relocalize_points": ("pts", "n", "T", "lat", "so", "min_inliers", "ao", "lrec", "rbuf"),
    "nvbx_relocalize_depth": ("depth", "rows", "cols", "cam", "T", "lat", "so", "min_inliers", "ao", "lrec", "rbuf"),
}
DEPTH = [e for e in ENTRIES if e.endswith("_depth")]
POINTS = [e for e in ENTRIES if not e.endswith("_depth")]
NO_IMAGE = ": the depth image and the camera are required"
BAD_IMAGE = ": the depth image and a camera of its size are required"
SUBSAMPLING = ": subsampling must be >= 1"
NO_POINTS = ": n points need points_xyz_dev"


def test_refusals_by_text_and_order(hip_lib):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(), device=0, block_capacity=1 << 13)
    for i in A.MAP_FRAMES[:2]:
        d, _, T = A.room_frame(i)
        m.integrate_depth(d, T, A.SMALL_CAM)
    d_img, _, T_true = A.room_frame(4)
    x = A.backproject(d_img, A.SMALL_CAM, subsampling=4)
    K = 5
    lat = m._lattice(0.2, 0.2, (3, 3, 1, 3))
    # every output holds a sentinel
    res = torch.full((M.ALIGN_RESULT_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    rbuf = torch.full((M.RELOC_RESULT_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
    rec = torch.full((K, 3), -7, dtype=torch.int64, device="cuda")
    lrec = torch.full((27, 3), -7, dtype=torch.int64, device="cuda")
    out_p = torch.full((len(x), 3), -7.0, dtype=torch.float32, device="cuda"); out_g = out_p.clone()
    out_r = torch.full((len(x),), -7.0, dtype=torch.float32, device="cuda")
    out_v = torch.full((len(x),), 0xAB, dtype=torch.uint8, device="cuda")
    outputs = (res, rbuf, rec, lrec, out_p, out_g, out_r, out_v)
    before = [t.clone() for t in outputs]
    xt = torch.from_numpy(x).cuda(); dt = torch.from_numpy(d_img).cuda()
    pt = torch.from_numpy(np.repeat(np.asarray(T_true, np.float32).reshape(1, 16), K, 0)).cuda()
    Tc = np.ascontiguousarray(T_true, np.float32)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cam = M.Camera(80.0, 80.0, 79.5, 59.5, 160, 120)
    wide = M.Camera(80.0, 80.0, 79.5, 59.5, 161, 120)
    good = dict(pts=ptr(xt), n=len(x), depth=ptr(dt), rows=120, cols=160, cam=C.byref(cam), T=Tc.ctypes.data_as(C.c_void_p), ao=None, so=None,
                res=ptr(res), out_p=ptr(out_p), out_r=ptr(out_r), out_g=ptr(out_g), out_v=ptr(out_v), poses=ptr(pt), k=K, rec=ptr(rec),
                lat=C.byref(lat), min_inliers=0, lrec=ptr(lrec), rbuf=ptr(rbuf))
    ao_s0 = C.byref(m.align_options(subsampling=0)); ao_it0 = C.byref(m.align_options(max_iterations=0)); so_s0 = C.byref(m.score_options(subsampling=0))
    assert res.data_ptr() % 8 == 0 and rbuf.data_ptr() % 8 == 0

    def call(entry, **replaced):
        args = dict(good, **replaced)
        return getattr(m.lib, entry)(m._h, *[args[name] for name in ENTRIES[entry]])

    table = []
    for e in DEPTH:
        table += [(e, dict(depth=None), NO_IMAGE), (e, dict(cam=None), NO_IMAGE), (e, dict(cam=C.byref(wide)), BAD_IMAGE), (e, dict(rows=0), BAD_IMAGE)]
    for e in POINTS:
        table += [(e, dict(n=-1), NO_POINTS), (e, dict(pts=None), NO_POINTS)]
    # subsampling = 0, in the options that feed the entry.  (The alignment looks at it in the depth form only, the scoring always.)
    table += [("nvbx_align_depth", dict(ao=ao_s0), SUBSAMPLING), ("nvbx_relocalize_depth", dict(ao=ao_s0), SUBSAMPLING)]
    table += [(e, dict(so=so_s0), SUBSAMPLING) for e in ENTRIES if "score" in e or "relocalize" in e]
    # two things wrong at once: which one the entry names
    table += [("nvbx_align_depth", dict(cam=C.byref(wide), ao=ao_s0), BAD_IMAGE),
              ("nvbx_score_poses_depth", dict(cam=C.byref(wide), so=so_s0), SUBSAMPLING),
              ("nvbx_relocalize_depth", dict(so=so_s0, ao=ao_it0), SUBSAMPLING),
              ("nvbx_relocalize_depth", dict(cam=C.byref(wide), ao=ao_s0), BAD_IMAGE)]
    # a side above 32768, with a camera of that size: refused before anything reads the (small) image
    long_cam = M.Camera(80.0, 80.0, 16384.0, 0.0, 32769, 1)
    table += [("nvbx_align_depth", dict(rows=1, cols=32769, cam=C.byref(long_cam)), BAD_IMAGE)]
    assert len(table) == 12 + 8 + 2 + 4 + 4 + 1
    for k, (entry, replaced, why) in enumerate(table):
        assert call(entry, **replaced) == -1, (k, entry)
        assert m.lib.nvbx_last_error() == (entry + why).encode(), (k, entry, m.lib.nvbx_last_error())
    m.synchronize(); torch.cuda.synchronize()
    for t, b in zip(outputs, before):                            # nothing was launched: no output changed
        assert torch.equal(t, b)
    # the good call of every entry, and the point form with an alignment subsampling of 0, which it does not look at
    for entry in ENTRIES:
        assert call(entry) == 0, (entry, m.lib.nvbx_last_error())
    for entry in ("nvbx_align_points", "nvbx_linearize_points", "nvbx_relocalize_points"):
        assert call(entry, ao=ao_s0) == 0, (entry, m.lib.nvbx_last_error())
    m.synchronize()
    assert not torch.equal(res, before[0]) and not torch.equal(rbuf, before[1]) and not torch.equal(rec, before[2]) and not torch.equal(lrec, before[3])
