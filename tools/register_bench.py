"""Time of the surface points and of map-to-map registration (nvbx_surface_points / nvbx_align_map) beside the two compositions a
caller has without them, in the same run by the same clock:
  (a) block_indices + get_blocks, the blocks uploaded again, the crossings of the three axes (faces through a sorted key search) in torch on the
      device;
  (b) update_color_mesh(full) + mesh(): the mesh's vertices as the surface cloud.
Scenario: the room map of the 640x480 loop (every fourth pose of the 200, depth and colour) and a copy of it built 3 cm / 1.5 degrees off (the same
frames integrated under T_off^-1 T).  Reported: us of the surface launches by the library's per-launch event spans (set_profiling), the least
bytes they can move -- two reads of every TSDF block and its three neighbour faces, 2 x (4096 + 3 x 512) B, plus the rows written -- and that
over the spans' sum as a share of the 8 TB/s HBM peak, ms of the whole surface_points call (count, wait, emit, wait) by a host clock around call
+ synchronize (the first call warms up), ms of align_map at stride 1 and 2 with the distance of its pose from the true one, ms of (a) and (b),
and whether (a) gives the same set of points.
One JSON object per line.  Usage: python tools/register_bench.py [--calls 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32
HBM_PEAK = 8.0e12


def host_ms(fn, sync, calls):
    """mean and spread (ms) of fn() + sync() by the host clock; the first call warms up"""
    times = []
    for i in range(calls + 1):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.mean(times)), 3), round(float(np.min(times)), 3), round(float(np.max(times)), 3)]


def offset_pose(axis, angle_deg, t):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def pose_distance(Ta, Tb):
    dR = Ta[:3, :3] @ Tb[:3, :3].T
    sk = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.linalg.norm(Ta[:3, 3] - Tb[:3, 3])), float(np.arctan2(np.linalg.norm(sk), (np.trace(dR) - 1.0) / 2.0))


# (the rule below restates what csrc/nvbx_surface_math.h and tests/surface_independent.py have too: on purpose -- a tool imports nothing from
#  tests/, and a composition must not call the code it is compared with)
def compose_torch(torch, m, M, min_weight=1e-4):
    """(a) -> points [n, 3] f32 on the device, in no particular order"""
    vs = float(F32(m.params.voxel_size))
    idx_h = np.asarray(m.block_indices(M.LAYER_TSDF), np.int32).reshape(-1, 3)
    vox, _ = m.get_blocks(M.LAYER_TSDF, idx_h)
    dev = m._cuda
    d = torch.from_numpy(np.ascontiguousarray(vox["distance"])).to(dev).reshape(-1, 8, 8, 8)
    w = torch.from_numpy(np.ascontiguousarray(vox["weight"])).to(dev).reshape(-1, 8, 8, 8)
    idx = torch.from_numpy(idx_h).to(dev).to(torch.int64)
    B = 1 << 21
    key = ((idx[:, 0] + (B >> 1)) * B + (idx[:, 1] + (B >> 1))) * B + (idx[:, 2] + (B >> 1))
    skey, order = torch.sort(key)
    obs = (w >= min_weight) & (d == d)
    v = torch.arange(8, device=dev, dtype=torch.float32)
    out = []
    for ax in range(3):
        step = torch.zeros(3, dtype=torch.int64, device=dev); step[ax] = 1
        n = idx + step
        nkey = ((n[:, 0] + (B >> 1)) * B + (n[:, 1] + (B >> 1))) * B + (n[:, 2] + (B >> 1))
        pos = torch.searchsorted(skey, nkey).clamp(max=len(skey) - 1)
        has = skey[pos] == nkey
        nb = order[pos]
        face_d = torch.where(has[:, None, None, None], d[nb].narrow(1 + ax, 0, 1), torch.full_like(d.narrow(1 + ax, 0, 1), float("nan")))
        face_o = has[:, None, None, None] & obs[nb].narrow(1 + ax, 0, 1)
        d1 = torch.cat([d.narrow(1 + ax, 1, 7), face_d], 1 + ax); o1 = torch.cat([obs.narrow(1 + ax, 1, 7), face_o], 1 + ax)
        cross = obs & o1 & ((d <= 0) != (d1 <= 0))
        b, x, y, z = torch.nonzero(cross, as_tuple=True)
        loc = (x, y, z)
        p = [((idx[b, i].to(torch.float32) * (8.0 * vs) + v[loc[i]] * vs) + vs * 0.5) for i in range(3)]
        p[ax] = p[ax] + vs * ((-d[b, x, y, z]) / (d1[b, x, y, z] - d[b, x, y, z]))
        out.append(torch.stack(p, 1))
    return torch.cat(out)


def compose_mesh(m):
    """(b) -> the number of mesh vertices"""
    m.update_color_mesh(full=True)
    return sum(len(b["vertices"]) for b in m.mesh().values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    T_off = offset_pose([0.3, -0.2, 1.0], 1.5, [0.02, -0.015, 0.0166])      # p_first = T_off p_second
    inv = np.linalg.inv(T_off)
    first = M.Mapper(M.default_params()); second = M.Mapper(M.default_params())
    sc = S.Scene()
    for i in range(0, 200, 4):
        T = S.trajectory_pose(i, 200)
        d, rgb = S.render(sc, T, cam)
        dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(rgb).cuda()
        for m, Tm in ((first, T), (second, (inv @ T).astype(F32))):
            m.integrate_depth(dd, Tm, cam); m.integrate_color(cc, Tm, cam)
    for m in (first, second):
        m.flush(); m.synchronize()
    lines = []

    def emit(r):
        line = json.dumps({"lib": os.path.basename(_lib.LIB_PATH), **r}); print(line, flush=True); lines.append(line)

    m = second
    n_blocks = int(m.num_blocks(M.LAYER_TSDF))
    count = m.surface_points(capacity=0)[3]
    dev = m._cuda
    P = torch.empty((count, 3), dtype=torch.float32, device=dev); Cc = torch.empty((count, 3), dtype=torch.uint8, device=dev); N = torch.empty((count, 3), dtype=torch.float32, device=dev)
    forms = (("points", (P, None, None), 12), ("points_colors", (P, Cc, None), 15), ("points_colors_normals", (P, Cc, N), 27))
    for name, out, row_bytes in forms:
        call_ms = host_ms(lambda: m.surface_points(out=out), m.synchronize, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            m.surface_points(out=out)
        m.synchronize()
        spans = {k: round(v["total_ms"] * 1e3 / v["count"], 2) for k, v in m.profile().items() if k.startswith("k_surface")}
        m.set_profiling(False)
        least = n_blocks * 2 * (4096 + 3 * 512) + count * row_bytes
        total_us = sum(spans.values())
        emit({"case": "surface_" + name, "tsdf_blocks": n_blocks, "points": count, "span_us_per_launch": spans, "spans_sum_us": round(total_us, 2),
              "least_bytes": least, "share_of_hbm_peak": round(least / HBM_PEAK / (total_us * 1e-6), 4), "out_call_ms_mean_min_max": call_ms, "calls": a.calls})
    whole = host_ms(lambda: m.surface_points(color=True, normals=True), m.synchronize, a.calls)
    comp_a = host_ms(lambda: compose_torch(torch, m, M), torch.cuda.synchronize, max(a.calls // 3, 2))
    pa = compose_torch(torch, m, M)
    as_set = lambda t: set(map(bytes, t.cpu().numpy().view(np.uint32)))      # noqa: E731
    same = as_set(pa) == as_set(m.surface_points()[0])
    comp_b = host_ms(lambda: compose_mesh(m), m.synchronize, max(a.calls // 3, 2))
    emit({"case": "surface_call_and_compositions", "points": count, "surface_points_count_then_emit_ms_mean_min_max": whole,
          "a_get_blocks_torch_crossings_ms_mean_min_max": comp_a, "a_points": int(pa.shape[0]), "a_same_set_of_points": bool(same),
          "b_update_color_mesh_full_then_mesh_ms_mean_min_max": comp_b, "b_vertices": int(compose_mesh(m)),
          "a_over_surface_points": round(comp_a[0] / whole[0], 1), "b_over_surface_points": round(comp_b[0] / whole[0], 1)})
    for stride in (1, 2):
        ms = host_ms(lambda: first.align_map(second, np.eye(4, dtype=F32), surface=dict(stride=stride)), first.synchronize, a.calls)
        res = first.align_map(second, np.eye(4, dtype=F32), surface=dict(stride=stride))
        dt, ang = pose_distance(res.T64, T_off)
        emit({"case": "align_map_stride_%d" % stride, "points": second.surface_points(capacity=0, stride=stride)[3], "n_valid": res.n_valid, "iterations": res.iterations,
              "status": res.status_name, "ms_mean_min_max": ms, "translation_error_m": round(dt, 6), "rotation_error_rad": round(ang, 6),
              "rmse_first_last_m": [round(res.rmse_first, 6), round(res.rmse_last, 6)]})
    first.close(); second.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
