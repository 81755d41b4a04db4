"""Child process of tests/test_gpu_render_lanes.py: NVBX_RENDER_LANES is read when a mapper is created; every lanes-per-ray setting renders the
same cases in a process of its own (a fault under one setting stays there) and saves what it got.  Usage: python render_lanes_child.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)

import render_cases as RC          # noqa: E402
import render_independent as R     # noqa: E402

BIG_CAM = (160.0, 160.0, 159.5, 119.5, 320, 240)       # 76 800 rays: the by-count choice takes 4 lanes per ray
TILES = 7                                              # 7 x 19 200 = 134 400 rays: the by-count choice takes 2
STRIDE_WORKGROUPS = 8192                               # the ray list's grid cap (render.hip): more workgroups' worth of rays repeat the loop


def main(out):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    m = M.Mapper(M.default_params(), block_capacity=1 << 13)
    for d, rgb, T in RC.map_frames():
        m.integrate_depth(d, T, RC.CAM); m.integrate_color(rgb, T, RC.CAM)
    res = {}
    np_ = lambda t: t.cpu().numpy()      # noqa: E731
    res["synthetic"] = m.synthetic_depth()
    res["same_pose"] = np_(m.render(RC.map_frames()[-1][2], RC.CAM, subsampling=m.params.sphere_tracing_subsampling, color=False)[0])
    for name, cam, pose in (("view", RC.CAM, "off30"), ("big", BIG_CAM, "off30")):
        d, c, n = m.render(RC.NOVEL_POSES[pose], cam, subsampling=1, color=True, normals=True)
        res[name + "_depth"], res[name + "_color"], res[name + "_normal"] = np_(d), np_(c), np_(n)
    o, d, _, _ = R.view_rays(RC.NOVEL_POSES["off30"], RC.CAM, 1)
    for name, reps in (("rays", 1), ("tiled", TILES)):
        t, h, c, n = m.cast_rays(np.tile(o, (reps, 1)), np.tile(d, (reps, 1)), color=True, normals=True)
        res[name + "_t"], res[name + "_hit"], res[name + "_color"], res[name + "_normal"] = np_(t), np_(h), np_(c), np_(n)
    # the gradient of the point query at the hit points of the ray list (the normals' reference)
    P = R.hit_points(o, d, res["rays_t"])
    _, g, v = m.query_tsdf(torch.from_numpy(P).cuda(), min_weight=1e-4)
    res["query_grad"], res["query_valid"] = np_(g), np_(v)
    if os.environ.get("NVBX_RENDER_LANES") == "1":
        # one lane per ray: 256 rays per workgroup, so 8192 * 256 rays fill the grid and the rest take the loop's second trip
        n_rays = STRIDE_WORKGROUPS * 256 + 513
        reps = -(-n_rays // len(o))
        oo = torch.from_numpy(np.tile(o, (reps, 1))[:n_rays]).cuda(); dd = torch.from_numpy(np.tile(d, (reps, 1))[:n_rays]).cuda()
        t, h, c, n = m.cast_rays(oo, dd, color=True, normals=True)
        idx = torch.arange(n_rays, device="cuda") % len(o)
        ref = [torch.from_numpy(res["rays_" + k]).cuda()[idx] for k in ("t", "hit", "color", "normal")]
        res["stride_rays"] = np.int64(n_rays)
        res["stride_equal"] = np.array([bool(torch.equal(a, b)) for a, b in zip((t, h, c, n), ref)])
    m.synchronize()
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
