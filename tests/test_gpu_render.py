"""Rendering and ray casts (nvbx_render_view / nvbx_cast_rays, Mapper.render / cast_rays, nvblox::SphereTracer) against the colour frame's own
synthetic depth, the CPU oracle at poses that were never integrated, the independent model (tests/render_independent.py), the point query and
the analytic room scene.  Small shapes throughout: the 160 x 120 camera and a five-frame map."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import render_cases as RC
import render_independent as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CAM = RC.CAM


def _np(t):
    return None if t is None else t.cpu().numpy()


def _mapper(frames, deferral=None, color=True, **kw):
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(**kw), block_capacity=1 << 13)
    if deferral is not None:
        m.set_color_deferral(deferral)
    for d, rgb, T in frames:
        m.integrate_depth(d, T, CAM)
        if color:
            m.integrate_color(rgb, T, CAM)
    return m


@pytest.fixture(scope="module")
def small(hip_lib):
    m = _mapper(RC.map_frames())
    m.synchronize()
    return m


@pytest.fixture(scope="module")
def oracle_small():
    return RC.oracle_map()


@pytest.fixture(scope="module")
def small_volume(small):
    from isaac_ros_nvblox_amd import mapper as M
    return RC.product_volume(small, M.LAYER_TSDF, RC.TSDF_FIELDS)


# ---- 1
@pytest.mark.gpu
def test_same_pose_equals_the_synthetic_depth(small):
    T_last = RC.map_frames()[-1][2]
    sd = small.synthetic_depth(); view = small.last_color_view()
    depth, color, normals = small.render(T_last, CAM, subsampling=small.params.sphere_tracing_subsampling, color=False)
    assert color is None and normals is None
    assert np.array_equal(_np(depth), sd) and (sd > 0).mean() > 0.3
    assert np.array_equal(small.synthetic_depth(), sd) and np.array_equal(small.last_color_view(), view)
    d0 = small.render(T_last, CAM, subsampling=None, color=False)[0]          # None: the mapper's subsampling
    assert np.array_equal(_np(d0), sd)


# ---- 2
@pytest.mark.gpu
@pytest.mark.parametrize("s", RC.SUBSAMPLINGS)
@pytest.mark.parametrize("pose", sorted(RC.NOVEL_POSES))
def test_any_pose_equals_the_oracle(small, oracle_small, pose, s):
    T = RC.NOVEL_POSES[pose]
    ref = RC.oracle_depth_at(oracle_small, T, s)
    depth = _np(small.render(T, CAM, subsampling=s, color=False)[0])
    assert depth.shape == ref.shape
    assert np.array_equal(depth > 0, ref > 0), int(((depth > 0) != (ref > 0)).sum())
    diff = float(np.abs(depth - ref).max())
    print("pose %s s %d: max |depth - oracle| = %g, hits %d" % (pose, s, diff, int((ref > 0).sum())))
    assert diff <= 1e-4, diff
    if pose == "out":
        assert not depth.any() and not ref.any()            # nothing was ever observed that way: all zeros, on both sides
    else:
        assert (depth > 0).mean() > 0.3


# ---- 3
@pytest.mark.gpu
@pytest.mark.parametrize("w,h,s", [(37, 23, 1), (37, 23, 2), (8, 8, 4)])
def test_odd_sizes(small, small_volume, w, h, s):
    cam = (20.0, 20.0, w / 2.0 - 0.5, h / 2.0 - 0.5, w, h)
    T = RC.NOVEL_POSES["along"]
    depth, color, normals = (_np(x) for x in small.render(T, cam, subsampling=s, color=True, normals=True))
    assert depth.shape == (h // s, w // s) and color.shape == depth.shape + (3,) and normals.shape == depth.shape + (3,)
    md, mh = R.render_depth(small_volume, T, cam, s, **RC.march_params(small.params))
    assert np.array_equal(depth > 0, mh) and mh.any()
    assert float(np.abs(depth - md).max()) <= 1e-4
    assert (color[~mh] == 0).all() and (normals[~mh] == 0).all()


@pytest.mark.gpu
def test_too_small_an_image_is_refused(small):
    from isaac_ros_nvblox_amd import mapper as M
    with pytest.raises(M.NvbxError, match="too small"):
        small.render(RC.NOVEL_POSES["along"], (20.0, 20.0, 3.0, 3.0, 7, 7), subsampling=4)


# ---- 4
@pytest.mark.gpu
def test_ray_list_equals_the_view(small):
    import torch
    T = RC.NOVEL_POSES["off30"]
    depth = _np(small.render(T, CAM, subsampling=1, color=False)[0]).reshape(-1)
    o, d, dcz, _ = R.view_rays(T, CAM, 1)                    # numpy f32, in the kernel's order of operations
    t, hit, _, _ = small.cast_rays(o, d)
    t, hit = _np(t), _np(hit)
    assert np.array_equal(hit, depth > 0) and hit.mean() > 0.3
    assert np.array_equal((t * dcz).astype(np.float32), depth)
    for n in (1, 7, 64, 65, 513):                            # partial groups, partial wavefronts, more than one workgroup
        tn, hn, cn, nn = small.cast_rays(torch.from_numpy(o[:n]).cuda(), d[:n], color=True, normals=True)
        assert np.array_equal(_np(tn), t[:n]) and np.array_equal(_np(hn), hit[:n]), n
        assert cn.shape == (n, 3) and nn.shape == (n, 3)
    # the first rays of a long list and the last rays of it, the colour and normal outputs included
    full = [_np(x) for x in small.cast_rays(o, d, color=True, normals=True)]
    head = [_np(x) for x in small.cast_rays(o[:513], d[:513], color=True, normals=True)]
    tail = [_np(x) for x in small.cast_rays(o[-513:], d[-513:], color=True, normals=True)]
    for f, a, b in zip(full, head, tail):
        assert np.array_equal(f[:513], a) and np.array_equal(f[-513:], b)


# ---- 5
def _random_rays(n, seed):
    from isaac_ros_nvblox_amd import synthetic as S
    rng = np.random.default_rng(seed)
    sc = S.Scene()
    k = n // 3

    def unit(v):
        v = v.astype(np.float32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
    free = []
    for _, _, T in RC.map_frames():                          # observed free space: on the frames' own rays, in front of the surface
        T = T.astype(np.float64)
        rays = S.pixel_rays(CAM).reshape(-1, 3) @ T[:3, :3].T
        t = sc.raycast(T[:3, 3], rays)
        j = rng.integers(0, len(rays), k // 5 + 1)
        free.append(T[:3, 3] + rays[j] * (t[j] * rng.uniform(0.2, 0.9, len(j)))[:, None])
    free = np.concatenate(free)[:k]
    th = rng.uniform(0, 2 * np.pi, k); rad = rng.uniform(0, 0.7, k)         # never observed: inside the circle the cameras look out of
    unobserved = np.stack([rad * np.cos(th), rad * np.sin(th), rng.uniform(0.5, 2.5, k)], 1)
    m = n - 2 * k
    dirs_out = unit(rng.normal(size=(m, 3)))
    outside = np.array([0.0, 0.0, 1.5]) + 8.0 * dirs_out                    # outside the map, aimed at a point of the room
    target = np.stack([rng.uniform(-3, 3, m), rng.uniform(-2.5, 2.5, m), rng.uniform(0, 3, m)], 1)
    o = np.concatenate([free, unobserved, outside]).astype(np.float32)
    d = np.concatenate([unit(rng.normal(size=(2 * k, 3))), unit(target - outside)])
    return o, d


@pytest.mark.gpu
def test_ray_list_equals_the_independent_model(small, small_volume):
    o, d = _random_rays(2000, 3)
    hand_o = np.array([[0.0, 0.0, 50.0],       # pointing away from everything
                       [3.1, 0.0, 1.5],        # starts behind the wall x = 3: the first samples are negative, nothing positive was seen
                       [1.0, 0.0, 1.5],        # looks at that wall from 2 m
                       [1.0, 0.0, 1.5],        # zero direction
                       [1.0, 0.0, 1.5]], np.float32)   # not finite
    hand_d = np.array([[0, 0, 1], [-1, 0, 0], [1, 0, 0], [0, 0, 0], [np.nan, 0, 1]], np.float32)
    o = np.concatenate([o, hand_o]); d = np.concatenate([d, hand_d])
    mp = RC.march_params(small.params)
    t, hit, _, _ = small.cast_rays(o, d)
    t, hit = _np(t), _np(hit)
    mt, mh = R.cast(small_volume, o, d, **mp)
    assert np.array_equal(hit, mh), np.nonzero(hit != mh)[0][:10]
    diff = float(np.abs(t - mt).max())
    print("max |t - model| = %g over %d rays, %d hits" % (diff, len(o), int(mh.sum())))
    assert diff <= 1e-4, diff
    k = 2000 // 3
    assert mh[:k].sum() > 50 and mh[2 * k:2000].sum() > 20                  # free-space and outside-in rays do find the surface
    assert list(mh[-5:]) == [False, False, True, False, False] and (t[~mh] == 0).all()
    # the ray at the wall again, stopped by max_ray_length just before the surface (samples at 0, 0.2, .. 1.6 m; the next would be at 1.8)
    t2, h2, _, _ = small.cast_rays(o[-3:-2], d[-3:-2], max_ray_length_m=1.7)
    mt2, mh2 = R.cast(small_volume, o[-3:-2], d[-3:-2], **dict(mp, max_len=np.float32(1.7)))
    assert not mh2[0] and not _np(h2)[0] and _np(t2)[0] == 0.0 and 1.8 < t[-3] < 2.2


# ---- 6
@pytest.mark.gpu
def test_colour_is_the_voxel_at_the_hit_point(hip_lib):
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    m = _mapper(RC.map_frames())
    T_extra = RC._pose(60, 0.0)                               # one depth frame without its colour frame: surface that has no colour
    m.integrate_depth(S.render(S.Scene(), T_extra, CAM)[0], T_extra, CAM)
    T = RC._pose(48, 0.0)                                     # sees both
    depth, color, _ = (_np(x) for x in m.render(T, CAM, subsampling=1, color=True))
    cv = RC.product_volume(m, M.LAYER_COLOR, RC.COLOR_FIELDS)
    o, d, dcz, shape = R.view_rays(T, CAM, 1)
    t, hit, c2, _ = (_np(x) for x in m.cast_rays(o, d, color=True))          # t itself (the view reports t * dcz)
    assert np.array_equal(hit.reshape(shape), depth > 0) and np.array_equal(c2.reshape(shape + (3,)), color)
    ref = R.colors(cv, o, d, t, hit, np.float32(m.params.voxel_size))
    assert np.array_equal(c2, ref), int((c2 != ref).any(axis=1).sum())
    found, v = cv.lookup(R._voxel_of(R.hit_points(o, d, t), np.float32(m.params.voxel_size)))
    has = found & (v["weight"] > 0)
    assert (hit & has).sum() > 500 and (hit & ~has).sum() > 500               # both kinds of hit occur
    assert (c2[hit & ~has] == 127).all() and (c2[~hit] == 0).all()


# ---- 7
@pytest.mark.gpu
def test_normals_are_the_normalised_query_gradient(small):
    import torch
    T = RC.NOVEL_POSES["along"]
    o, d, dcz, shape = R.view_rays(T, CAM, 1)
    t, hit, _, nr = (_np(x) for x in small.cast_rays(o, d, normals=True))
    view_n = _np(small.render(T, CAM, subsampling=1, color=False, normals=True)[2])
    assert np.array_equal(view_n.reshape(-1, 3), nr)                          # the view and the ray list run one epilogue
    P = R.hit_points(o, d, t)
    dist, g, valid = (_np(x) for x in small.query_tsdf(torch.from_numpy(P).cuda(), min_weight=1e-4))
    g = g.astype(np.float64); ln = np.linalg.norm(g, axis=1)
    use = hit & valid & (ln > 0)
    assert use.sum() > 5000 and (hit & ~valid).sum() > 0
    err = float(np.abs(nr[use] - g[use] / ln[use, None]).max())
    print("max |normal - g / |g|| = %g over %d hits" % (err, int(use.sum())))
    assert err <= 1e-6, err
    assert (nr[~use] == 0).all()


# Tolerance of the wall test.  Measured on the CPU: the independent model (render_independent.normals) on the ORACLE's map of the same ten frames
# gives max |normal - (-1, 0, 0)| = 0.0 over the 7277 wall pixels of RC.wall_pixels() (the frames look at the wall head-on, so the TSDF does not
# vary along y and z there and the interpolant's gradient is exactly along x).  Bound = 1.2 x 0.0 + 1e-6, the 1e-6 being the f32 normalisation
# allowance of the test above.
WALL_NORMAL_TOLERANCE = 1.2 * 0.0 + 1e-6


@pytest.mark.gpu
def test_wall_normals_agree_with_the_analytic_scene(hip_lib):
    """The wall x = 3 of the room scene seen head-on by ten frames: rendered normals of the wall pixels against the wall's analytic normal
    (-1, 0, 0).  Tolerance WALL_NORMAL_TOLERANCE = 1e-6: the model on the oracle's map of this scene measures 0.0 (CPU, see above)."""
    m = _mapper(RC.wall_frames())
    depth, _, nr = (_np(x) for x in m.render(RC.WALL_POSE, CAM, subsampling=1, color=False, normals=True))
    mask = RC.wall_pixels()
    assert mask.sum() > 5000 and (depth[mask] > 0).all()
    err = RC.wall_normal_error(nr, mask)
    print("max |normal - analytic| on %d wall pixels = %g" % (int(mask.sum()), err))
    assert err <= WALL_NORMAL_TOLERANCE, err


# ---- 8
@pytest.mark.gpu
def test_held_back_work(hip_lib):
    from isaac_ros_nvblox_amd import mapper as M
    fr = RC.map_frames()
    T = RC.NOVEL_POSES["along"]
    # a render with colour shows what classic order shows
    res = []
    for on in (True, False):
        m = M.Mapper(block_capacity=1 << 13); m.set_color_deferral(on)
        for d, rgb, Tf in fr:
            m.integrate_depth(d, Tf, CAM); m.integrate_color(rgb, Tf, CAM); m.update_esdf()
        res.append([_np(x) for x in m.render(T, CAM, subsampling=2, color=True, normals=True)])
    for a, b in zip(*res):
        assert a.tobytes() == b.tobytes()
    assert (res[0][0] > 0).mean() > 0.3 and (res[0][1] != 127).any()
    # in the middle of a pipelined sequence: without colour the held-back frame stays held back (same launches as a run that never rendered,
    # same map); with colour it is carried out first (same map)
    A, B, N = (M.Mapper(block_capacity=1 << 13) for _ in range(3))
    for m in (A, B, N):
        m.set_color_deferral(True); m.set_profiling(True)
    mid = []
    for k, (d, rgb, Tf) in enumerate(fr):
        for m in (A, B, N):
            m.integrate_depth(d, Tf, CAM); m.integrate_color(rgb, Tf, CAM); m.update_esdf()
        if k == 2:
            mid = [_np(A.render(T, CAM, subsampling=2, color=False)[0]), _np(B.render(T, CAM, subsampling=2, color=True)[0])]
    for m in (A, B, N):
        m.synchronize()
    assert np.array_equal(mid[0], mid[1]) and (mid[0] > 0).any()
    never = H.map_state(N)
    H.assert_same_map(A, never, "rendered without colour"); H.assert_same_map(B, never, "rendered with colour")
    launches = lambda m: {k: v["count"] for k, v in m.profile().items() if not k.startswith("_") and "k_render" not in k}      # noqa: E731
    assert launches(A) == launches(N), (launches(A), launches(N))
    assert sum(v["count"] for k, v in A.profile().items() if "k_render" in k) == 1
    assert A.counters() == N.counters()


# ---- 9
@pytest.mark.gpu
def test_errors(small):
    import torch
    from isaac_ros_nvblox_amd import mapper as M, _lib
    lib = small.lib
    T = np.ascontiguousarray(RC.NOVEL_POSES["along"], np.float32); k = _lib.Camera(*[float(v) for v in CAM[:4]], int(CAM[4]), int(CAM[5]))
    r, c = C.c_int32(), C.c_int32()
    Tp = T.ctypes.data_as(C.c_void_p)
    buf = torch.zeros(CAM[4] * CAM[5], dtype=torch.float32, device="cuda")
    p = C.c_void_p(buf.data_ptr())
    assert lib.nvbx_render_view(small._h, Tp, C.byref(k), 4, 0.0, None, None, None, 0, C.byref(r), C.byref(c)) == -3       # NVBX_E_CAPACITY ...
    assert (r.value, c.value) == (30, 40)                                                                              # ... and the sizes
    assert lib.nvbx_render_view(small._h, Tp, C.byref(k), 4, 0.0, p, None, None, 30 * 40 - 1, C.byref(r), C.byref(c)) == -3
    assert lib.nvbx_render_view(small._h, Tp, C.byref(k), 4, 0.0, None, None, None, 30 * 40, C.byref(r), C.byref(c)) == -1   # depth is required
    assert lib.nvbx_render_view(small._h, None, C.byref(k), 4, 0.0, p, None, None, 30 * 40, C.byref(r), C.byref(c)) == -1
    assert lib.nvbx_render_view(small._h, Tp, None, 4, 0.0, p, None, None, 30 * 40, C.byref(r), C.byref(c)) == -1
    assert lib.nvbx_render_view(small._h, Tp, C.byref(k), -1, 0.0, p, None, None, 30 * 40, C.byref(r), C.byref(c)) == -1
    assert lib.nvbx_render_view(small._h, Tp, C.byref(k), 4, 0.0, p, None, None, 30 * 40, C.byref(r), C.byref(c)) == 0
    assert lib.nvbx_cast_rays(small._h, None, None, 0, 0.0, None, None, None, None) == 0                                  # n = 0: a no-op
    assert lib.nvbx_cast_rays(small._h, None, None, -1, 0.0, None, None, None, None) == -1
    assert lib.nvbx_cast_rays(small._h, p, None, 4, 0.0, p, None, None, None) == -1
    assert lib.nvbx_cast_rays(small._h, p, p, 4, 0.0, None, None, None, None) == -1
    assert b"nvbx_cast_rays" in lib.nvbx_last_error()
    assert lib.nvbx_cast_rays(small._h, p, p, 4, 1e30, p, None, None, None) == -1      # no origin could be addressed with such a reach
    assert b"max_ray_length_m" in lib.nvbx_last_error()
    t, hit, col, nr = small.cast_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), color=True, normals=True)
    assert t.numel() == 0 and hit.numel() == 0 and col.shape == (0, 3) and nr.shape == (0, 3)
    occ = M.Mapper(M.default_params(projective_layer_type=1), block_capacity=1 << 10)
    with pytest.raises(M.NvbxError, match="occupancy"):
        occ.render(T, CAM)
    with pytest.raises(M.NvbxError, match="occupancy"):
        occ.cast_rays(np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32))
    with pytest.raises(ValueError):
        small.render(T, CAM, subsampling=4, out=(torch.zeros((5, 5), device="cuda"), None, None))
    # out=: the caller's tensors are written, nothing else
    d = torch.full((30, 40), -1.0, device="cuda"); col = torch.zeros((30, 40, 3), dtype=torch.uint8, device="cuda")
    got = small.render(T, CAM, subsampling=4, out=(d, col, None))
    assert got[0] is d and got[1] is col and got[2] is None
    ref = small.render(T, CAM, subsampling=4, color=True)
    assert torch.equal(d, ref[0]) and torch.equal(col, ref[1])
    small.synchronize()


# ---- 10
FACADE_SRC = r'''
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>
#include "nvblox/nvblox.h"
#include "nvblox/rays/sphere_tracer.h"
int main(int argc, char** argv) {
  nvblox::Mapper mapper(0.05f, nvblox::MemoryType::kDevice);
  if (!mapper.loadMap(argv[1])) return 2;
  float Trm[16];
  { std::ifstream in(argv[2], std::ios::binary); in.read((char*)Trm, sizeof(Trm)); }
  const nvblox::Transform T = nvblox::Transform::fromRowMajor(Trm);
  const nvblox::Camera cam(80.0f, 80.0f, 79.5f, 59.5f, 160, 120);
  nvbx_mapper* h = mapper.tsdf_layer().c_handle();
  nvbx_mapper_params before, after;
  nvbx_mapper_get_params(h, &before);
  const float trunc = before.truncation_distance_vox * before.voxel_size;
  nvblox::SphereTracer tracer;
  nvblox::DepthImage depth, depth_short, depth_bad;
  nvblox::ColorImage color;
  if (!tracer.renderRgbdImageOnGPU(cam, T, mapper.tsdf_layer(), mapper.color_layer(), trunc, &depth, &color, nvblox::MemoryType::kDevice, 2)) return 3;
  tracer.maximum_steps(3);
  if (!tracer.renderImageOnGPU(cam, T, mapper.tsdf_layer(), trunc, &depth_short, nvblox::MemoryType::kHost, 2)) return 4;
  const bool refused = !tracer.renderImageOnGPU(cam, T, mapper.tsdf_layer(), trunc * 2.0f, &depth_bad);
  nvbx_synchronize(h);
  nvbx_mapper_get_params(h, &after);
  const int n = depth.numel();
  std::vector<float> d(n), ds(n); std::vector<unsigned char> c(3 * n);
  hipMemcpy(d.data(), depth.dataConstPtr(), n * sizeof(float), hipMemcpyDeviceToHost);
  hipMemcpy(c.data(), color.dataConstPtr(), 3 * n, hipMemcpyDeviceToHost);
  std::memcpy(ds.data(), depth_short.dataConstPtr(), n * sizeof(float));
  std::ofstream out(argv[3], std::ios::binary);
  out.write((const char*)d.data(), n * sizeof(float)); out.write((const char*)c.data(), 3 * n); out.write((const char*)ds.data(), n * sizeof(float));
  std::printf("{\"rows\": %d, \"cols\": %d, \"short_rows\": %d, \"params_unchanged\": %d, \"refused\": %d, \"steps\": %d}\n", depth.rows(), depth.cols(),
              depth_short.rows(), (int)(std::memcmp(&before, &after, sizeof(before)) == 0), (int)refused, tracer.maximum_steps());
  return 0;
}
'''


@pytest.mark.gpu
def test_sphere_tracer_facade_equals_the_c_call(small, tmp_path):
    from isaac_ros_nvblox_amd import mapper as M
    src = tmp_path / "tracer.cpp"; src.write_text(FACADE_SRC)
    exe = tmp_path / "tracer"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unused-result", "-D__HIP_PLATFORM_AMD__", "-I" + INC, "-I/opt/rocm/include",
                           str(src), "-o", str(exe), "-L" + os.path.join(ROOT, "isaac_ros_nvblox_amd"), "-lnvblox_hip", "-L/opt/rocm/lib", "-lamdhip64",
                           "-Wl,-rpath," + os.path.join(ROOT, "isaac_ros_nvblox_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    path = str(tmp_path / "small.nvbx")
    small.save_map(path)
    T = np.ascontiguousarray(RC.NOVEL_POSES["off30"], np.float32)
    (tmp_path / "pose.bin").write_bytes(T.tobytes())
    r = subprocess.run([str(exe), path, str(tmp_path / "pose.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info == {"rows": 60, "cols": 80, "short_rows": 60, "params_unchanged": 1, "refused": 1, "steps": 3}
    m = M.Mapper(block_capacity=1 << 13); m.load_map(path)
    depth, color, _ = (_np(x) for x in m.render(T, CAM, subsampling=2, max_ray_length_m=15.0, color=True))
    raw = (tmp_path / "out.bin").read_bytes(); n = 60 * 80
    fd = np.frombuffer(raw, np.float32, n, 0).reshape(60, 80); fc = np.frombuffer(raw, np.uint8, 3 * n, 4 * n).reshape(60, 80, 3)
    fs = np.frombuffer(raw, np.float32, n, 7 * n).reshape(60, 80)
    assert fd.tobytes() == depth.tobytes() and fc.tobytes() == color.tobytes() and (fd > 0).mean() > 0.3
    # three steps of at most the truncation distance reach 0.6 m: shorter rays, so far fewer hits, and those that remain are unchanged
    assert 0 <= (fs > 0).sum() < 0.2 * (fd > 0).sum()
    assert np.array_equal(fs[fs > 0], fd[fs > 0])
