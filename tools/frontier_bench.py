"""Time of the frontier scan, the frontier clusters and the view gain (nvbx_find_frontiers / nvbx_frontier_clusters / nvbx_view_gain; DESIGN.md
2.18) on the bench's room map, beside the composition a caller builds from the calls the library already had.

The room map of the 640x480 loop (every second pose of the 200, depth only: the calls read TSDF voxels) is built once.  Reported:
  - us per launch of the scan (k_find_frontiers) by the
    library's own per-launch event spans (set_profiling), the least bytes the scan has to move -- every TSDF block read once, the six facing
    faces (3 KiB) of every block that holds a free voxel, 4 KiB + 12 B written per entry -- and that over the span as a share of the 8 TB/s HBM peak;
  - ms of find_frontiers, frontier_clusters and view_gain (64 poses, subsampling 4) by a host clock around the call + synchronize, into
    preallocated buffers;
  - in the same run, by the same clock, today's composition: block_indices + get_blocks, classification and the six-neighbour count on a dense
    numpy volume, scipy.ndimage.label; for the view gain a numpy walk of the same samples through that dense volume (there is no call to compose).
One JSON object per line.  Usage: python tools/frontier_bench.py [--calls 10] [--scan-only] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
MIN_W = 1e-4
F32 = np.float32


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


# (the classification and the ray walk restate rules that csrc/frontier.hip and tests/frontier_independent.py have too: on purpose -- a tool imports
#  nothing from tests/, and the composition must not call the code it is compared with)
def dense_classes(M, m, free_d):
    """block_indices + get_blocks + classification: -> (unknown [X, Y, Z] bool, free [X, Y, Z] bool, lo: the box's lowest voxel, keys)"""
    keys = m.block_indices(M.LAYER_TSDF)
    blocks, _ = m.get_blocks(M.LAYER_TSDF, keys)
    lo = keys.min(0); nb = keys.max(0) - lo + 1
    obs = np.zeros(tuple(8 * nb), bool); free = np.zeros(tuple(8 * nb), bool)
    o = blocks["weight"] >= F32(MIN_W)
    f = o & (blocks["distance"] > F32(free_d))
    p = keys - lo
    ov = obs.reshape(nb[0], 8, nb[1], 8, nb[2], 8); fv = free.reshape(nb[0], 8, nb[1], 8, nb[2], 8)
    ov[p[:, 0], :, p[:, 1], :, p[:, 2], :] = o.reshape(-1, 8, 8, 8)
    fv[p[:, 0], :, p[:, 1], :, p[:, 2], :] = f.reshape(-1, 8, 8, 8)
    return ~obs, free, 8 * lo, keys


def compose_frontiers(M, m, free_d, label):
    from scipy import ndimage
    unk, free, lo, keys = dense_classes(M, m, free_d)
    u = np.pad(unk, 1, constant_values=True).astype(np.int8)
    nu = u[:-2, 1:-1, 1:-1] + u[2:, 1:-1, 1:-1] + u[1:-1, :-2, 1:-1] + u[1:-1, 2:, 1:-1] + u[1:-1, 1:-1, :-2] + u[1:-1, 1:-1, 2:]
    fr = free & (nu >= 1)
    n_comp = 0
    if label:
        cc, n_comp = ndimage.label(fr, structure=ndimage.generate_binary_structure(3, 3))
        if n_comp:
            ndimage.center_of_mass(fr, cc, np.arange(1, n_comp + 1))
    return int(fr.sum()), int(n_comp), unk, free, lo, keys


def compose_view_gain(unk, free, lo, poses, cam, s, max_range, vs):
    fu, fv, cu, cv, w, h = cam
    rows, cols = h // s, w // s
    c, r = np.meshgrid((np.arange(cols) * s).astype(F32), (np.arange(rows) * s).astype(F32))
    rx = ((c + F32(0.5)) - F32(cu)) / F32(fu); ry = ((r + F32(0.5)) - F32(cv)) / F32(fv)
    n = np.sqrt((rx * rx + ry * ry) + F32(1.0))
    dc = np.stack([rx / n, ry / n, F32(1.0) / n], -1).reshape(-1, 3)
    shape = np.array(unk.shape)
    out = np.zeros((len(poses), 4), np.int64)
    for i, T in enumerate(poses):
        d = np.stack([(T[j, 0] * dc[:, 0] + T[j, 1] * dc[:, 1]) + T[j, 2] * dc[:, 2] for j in range(3)], -1); o = T[:3, 3]      # (the kernels' order of the sum)
        alive = np.ones(len(d), bool)
        k = 0
        while alive.any():
            t = (F32(k) + F32(0.5)) * F32(vs)
            if not t < F32(max_range):
                break
            g = np.floor((o[None] + t * d[alive]) / F32(vs)).astype(np.int64) - lo
            inside = np.all((g >= 0) & (g < shape), axis=1)
            gi = np.where(inside[:, None], g, 0)
            u = ~inside | unk[gi[:, 0], gi[:, 1], gi[:, 2]]
            f = inside & free[gi[:, 0], gi[:, 1], gi[:, 2]]
            hit = ~u & ~f
            out[i, 1] += int(u.sum()); out[i, 2] += int(f.sum()); out[i, 3] += int(hit.sum())
            alive[np.flatnonzero(alive)[hit]] = False
            k += 1
        out[i, 0] = len(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scan-only", action="store_true", help="the scan's spans and host time only (the A/B of a build variant)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    scene = S.Scene()
    m = M.Mapper(M.default_params())
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i, 200)
        d, _ = S.render(scene, T, cam, color=False)
        m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
    m.synchronize()
    vs = float(m.params.voxel_size)
    n_tsdf = m.num_blocks(M.LAYER_TSDF)
    dev = torch.device("cuda", 0)
    idx = torch.empty((n_tsdf, 3), dtype=torch.int32, device=dev); lab = torch.empty((n_tsdf, 512), dtype=torch.int32, device=dev)
    sc = torch.empty((n_tsdf, 512), dtype=torch.float32, device=dev); ids = torch.empty((n_tsdf, 512), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    rec = m.component_records(1 << 16)
    lines = []

    def emit(r):
        r = {"lib": os.path.basename(_lib.LIB_PATH), **r}
        line = json.dumps(r); print(line, flush=True); lines.append(line)

    # ---- the scan
    scan = lambda: m.find_frontiers(out=(idx, lab, sc, cnt[0:1]))      # noqa: E731
    call = host_ms(scan, m.synchronize, a.calls)
    n_entries = int(cnt[0].item())
    n_voxels = int((lab[:n_entries] == 0).sum().item())
    spans = {}
    m.set_profiling(True)
    for _ in range(a.calls):
        scan()
    m.synchronize()
    for k, v in m.profile().items():
        if "frontier" in k:
            spans[k] = round(v["total_ms"] * 1e3 / max(v["count"], 1), 2)
    m.set_profiling(False)
    n_found, _, unk, free, lo, keys = compose_frontiers(M, m, vs, False)
    has_free = free.reshape(free.shape[0] // 8, 8, free.shape[1] // 8, 8, free.shape[2] // 8, 8).any(axis=(1, 3, 5))
    n_free_blocks = int(has_free.sum())
    least = n_tsdf * 4096 + n_free_blocks * 6 * 64 * 8 + n_entries * (4096 + 12)
    span_us = round(sum(spans.values()), 2)
    emit({"case": "frontier_scan_room_640x480", "form": "single_pass", "tsdf_blocks": n_tsdf,
          "blocks_with_a_free_voxel": n_free_blocks, "frontier_blocks": n_entries, "frontier_voxels": n_voxels, "span_us": spans, "scan_span_us": span_us,
          "least_bytes": least, "share_of_hbm_peak": round(least / HBM_PEAK / (span_us * 1e-6), 4) if span_us else None,
          "call_ms_mean_min_max": call, "composition_frontier_voxels": n_found, "calls": a.calls})
    assert n_found == n_voxels, (n_found, n_voxels)
    if not a.scan_only:
        comp = host_ms(lambda: compose_frontiers(M, m, vs, False), m.synchronize, max(a.calls // 3, 2))
        emit({"case": "frontier_scan_vs_composition", "call_ms_mean_min_max": call, "composition_ms_mean_min_max": comp, "composition_over_call": round(comp[0] / call[0], 1)})
        # ---- the clusters, connectivity 26
        clusters = lambda: m.frontier_clusters(connectivity=26, min_voxels=5, out=(idx, lab, sc, ids, cnt[0:1], rec, cnt[1:2]))      # noqa: E731
        call_c = host_ms(clusters, m.synchronize, a.calls)
        n_comp = int(cnt[1].item())
        comp_c = host_ms(lambda: compose_frontiers(M, m, vs, True), m.synchronize, max(a.calls // 3, 2))
        emit({"case": "frontier_clusters_room_640x480", "connectivity": 26, "min_voxels": 5, "components": n_comp, "call_ms_mean_min_max": call_c,
              "composition_ms_mean_min_max": comp_c, "composition_over_call": round(comp_c[0] / call_c[0], 1), "calls": a.calls})
        # ---- the view gain: 64 poses on two circles, subsampling 4, 5 m
        poses = np.stack([S.trajectory_pose(i, 64, radius=1.0 if i % 2 else 2.0, height=1.2, pitch_deg=-5.0, yaw_offset_deg=37.0) for i in range(64)]).astype(F32)
        pd = torch.from_numpy(poses).cuda(); gains = torch.zeros((64, 4), dtype=torch.int32, device=dev)
        gain = lambda: m.view_gain(pd, cam, subsampling=4, max_range_m=5.0, out=gains)      # noqa: E731
        call_g = host_ms(gain, m.synchronize, a.calls)
        g = gains.cpu().numpy()
        m.set_profiling(True)
        for _ in range(a.calls):
            gain()
        m.synchronize()
        gspan = [round(v["total_ms"] * 1e3 / max(v["count"], 1), 2) for k, v in m.profile().items() if "k_view_gain" in k]
        m.set_profiling(False)
        t0 = time.perf_counter()
        unk, free, lo, _ = dense_classes(M, m, vs)
        want = compose_view_gain(unk, free, lo, poses, cam, 4, 5.0, vs)
        comp_g = (time.perf_counter() - t0) * 1e3
        emit({"case": "view_gain_room_640x480", "views": 64, "subsampling": 4, "max_range_m": 5.0, "rays": int(g[:, 0].sum()), "unknown_samples": int(g[:, 1].sum()),
              "free_samples": int(g[:, 2].sum()), "rays_hit": int(g[:, 3].sum()), "span_us": gspan[0] if gspan else None, "call_ms_mean_min_max": call_g,
              "composition_ms": round(comp_g, 1), "composition_over_call": round(comp_g / call_g[0], 1), "composition_agrees": bool(np.array_equal(want, g.astype(np.int64))),
              "calls": a.calls})
    m.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
