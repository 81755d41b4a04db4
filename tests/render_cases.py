"""Shared by tests/test_render_model.py (CPU) and tests/test_gpu_render.py: the small map, the poses that were never integrated, and the
adapters that hand a map's blocks to the independent model (tests/render_independent.py)."""
import functools

import numpy as np

import helpers as H
import render_independent as R
from isaac_ros_nvblox_amd import synthetic as S

CAM = H.SMALL_CAM
STRIDE = 9                       # frames 0, 9, .. 36 of the 200-frame circle: yaw 0 .. 65 degrees
SUBSAMPLINGS = (1, 3, 4)


@functools.lru_cache(maxsize=None)
def map_frames():
    return H.frames(5, CAM, stride=STRIDE)


def _pose(index, yaw_off_deg):
    th = 2.0 * np.pi * index / 200.0
    pos = np.array([np.cos(th), np.sin(th), 1.5])
    return S.look_pose(pos, th + np.deg2rad(yaw_off_deg), np.deg2rad(-10.0))


# never integrated: between two frames of the trajectory; ~30 degrees off it; turned round, towards space no frame has looked at
NOVEL_POSES = {"along": _pose(14, 0.0), "off30": _pose(20, 30.0), "out": _pose(18, 180.0)}


def march_params(p):
    """(voxel_size, trunc, eps_m, max_steps, max_len) of a parameter struct, in f32 as the library forms them"""
    vs = np.float32(p.voxel_size)
    return dict(voxel_size=vs, trunc=np.float32(p.truncation_distance_vox) * vs, eps_m=np.float32(p.sphere_tracing_surface_eps_vox) * vs,
                max_steps=int(p.sphere_tracing_max_steps), max_len=np.float32(p.sphere_tracing_max_ray_length_m))


def oracle_volume(o, layer, fields):
    import oracle
    assert layer in (oracle.L_TSDF, oracle.L_COLOR)
    return R.Volume({tuple(int(v) for v in i): o.get_block(layer, i) for i in o.block_indices(layer)}, fields)


def product_volume(m, layer, fields):
    idx = m.block_indices(layer)
    blocks, found = m.get_blocks(layer, idx)
    assert found.all()
    return R.Volume({tuple(int(v) for v in i): blocks[k] for k, i in enumerate(idx)}, fields)


TSDF_FIELDS = ("distance", "weight")
COLOR_FIELDS = ("r", "g", "b", "weight")


def oracle_map():
    import oracle
    o = oracle.OracleMap(oracle.default_params())
    for d, rgb, T in map_frames():
        o.integrate_depth(d, T, CAM); o.integrate_color(rgb, T, CAM)
    return o


def oracle_depth_at(o, T, subsampling):
    """the oracle's synthetic depth at pose T and `subsampling`: its colour integration renders it and does not write the TSDF"""
    import oracle
    p = oracle.default_params()
    for name, _ in oracle.OrcParams._fields_:
        setattr(p, name, getattr(o.params, name))
    p.sphere_tracing_subsampling = subsampling
    o.set_params(p)
    o.integrate_color(np.zeros((CAM[5], CAM[4], 3), np.uint8), T, CAM)
    return o.synthetic_depth()


# ---- the analytic room's wall x = 3 seen head-on by ten frames (normals against the wall's analytic normal)
WALL_NORMAL = np.array([-1.0, 0.0, 0.0], np.float32)      # the TSDF grows towards the camera: its gradient points out of the wall


def wall_frames():
    sc = S.Scene()
    out = []
    for y in np.linspace(-0.45, 0.45, 10):
        T = S.look_pose(np.array([0.0, y, 1.5]), 0.0, 0.0)
        d, rgb = S.render(sc, T, CAM)
        out.append((d, rgb, T))
    return out


WALL_POSE = S.look_pose(np.array([0.2, 0.07, 1.5]), 0.0, 0.0)


def wall_pixels():
    """mask [rows, cols] of the pixels of WALL_POSE whose ray, and every ray within 10 pixels, ends on the wall x = 3"""
    sc = S.Scene()
    T = WALL_POSE.astype(np.float64)
    rays = S.pixel_rays(CAM) @ T[:3, :3].T
    t = sc.raycast(T[:3, 3], rays)
    x = T[0, 3] + rays[..., 0] * t
    on = np.isfinite(t) & (np.abs(x - sc.room_max[0]) < 1e-9)
    keep = on.copy()
    for dr in range(-10, 11):
        for dc in range(-10, 11):
            sh = np.zeros_like(on)
            r0, r1 = max(0, dr), on.shape[0] + min(0, dr)
            c0, c1 = max(0, dc), on.shape[1] + min(0, dc)
            sh[r0:r1, c0:c1] = on[r0 - dr:r1 - dr, c0 - dc:c1 - dc]
            keep &= sh
    return keep


def wall_normal_error(normals, mask):
    """largest absolute component difference between the rendered normals of the wall pixels and the wall's analytic normal"""
    n = np.asarray(normals, np.float32).reshape(mask.shape + (3,))[mask]
    return float(np.abs(n - WALL_NORMAL).max())
