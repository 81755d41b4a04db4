"""Time of change detection (nvbx_find_changes / nvbx_change_clusters) on the bench's room map against the same room with its
sphere moved, beside the composition a caller builds from the calls the library already had.

Both rooms are fused from every fourth pose of the 640x480 loop (depth only: the calls read TSDF voxels).  Per transform (the identity; 3 cm and
1.5 degrees off) and sampling mode, reported:
  - us per launch of the scan (k_find_changes + k_change_result) by the library's own per-launch event spans (set_profiling), the least bytes
    the scan has to move -- 4 KiB per TSDF block of the scanned map, 4 KiB per distinct block of the reference its samples reach, 4 KiB + 12 B
    (8 KiB + 12 B with scores) written per entry -- and that over the span as a share of the 8 TB/s HBM peak;
  - ms of find_changes and of the whole change_clusters call by a host clock around the call + synchronize, into preallocated buffers;
  - in the same process, by the same clock, today's composition (trilinear only: there is no nearest query to compose): block_indices +
    get_blocks of the scanned map, query_tsdf of the reference at every voxel centre, torch compares, a gather of the changed blocks,
    label_components.
One JSON object per line.  Usage: python tools/change_bench.py [--calls 10] [--stride 4] [--out FILE]"""
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
MOVED = (1.5, -1.0, 0.6)


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


def small_pose(axis, angle_deg, t):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a); th = np.deg2rad(angle_deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K); T[:3, 3] = t
    return T.astype(F32)


def inverse_pair(T):
    """{R_RM, t_RM} as the library forms them: the transpose, and -(R^T t) summed in float64 and rounded once"""
    R = T[:3, :3].T.copy()
    return R, (-(R.astype(np.float64) @ T[:3, 3].astype(np.float64))).astype(F32)


# (the classes and the sample positions restate rules that csrc/change.hip and tests/change_independent.py have too: on purpose -- a tool imports
#  nothing from tests/, and the composition must not call the code it is compared with)
def compose(torch, M, m, ref, T, vs, label):
    """-> (appeared voxels, removed voxels, changed blocks, components) through the calls the library had before"""
    keys = m.block_indices(M.LAYER_TSDF)
    blocks, _ = m.get_blocks(M.LAYER_TSDF, keys)
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(np.ascontiguousarray(blocks["distance"])).to(dev); w = torch.from_numpy(np.ascontiguousarray(blocks["weight"])).to(dev)
    t = torch.arange(512, device=dev)
    lane = torch.stack([t >> 6, (t >> 3) & 7, t & 7], 1)
    g = (8 * torch.from_numpy(keys.astype(np.int64)).to(dev)[:, None, :] + lane[None]).to(torch.float32)
    p = (g + 0.5) * F32(vs)
    R, tr = inverse_pair(T)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    pr = torch.stack([((float(R[i, 0]) * x + float(R[i, 1]) * y) + float(R[i, 2]) * z) + float(tr[i]) for i in range(3)], -1).reshape(-1, 3).contiguous()
    dr, _, valid = ref.query_tsdf(pr, min_weight=MIN_W)
    dr = dr.reshape(-1, 512); valid = valid.reshape(-1, 512).bool()
    obs = w >= MIN_W
    appeared = obs & (d <= 0.0) & valid & (dr > F32(vs)); removed = obs & (d > F32(vs)) & valid & (dr <= 0.0)
    lab = torch.where(appeared, 0, torch.where(removed, 1, -1)).to(torch.int32)
    sc = torch.where(lab >= 0, (d - dr).abs(), torch.zeros_like(d))
    changed = (lab >= 0).any(1)
    n_comp = 0
    if label and bool(changed.any()):
        idx = torch.from_numpy(keys.astype(np.int32)).to(dev)[changed].contiguous()
        _, comps = m.label_components(idx, lab[changed].contiguous(), sc[changed].contiguous(), connectivity=26, min_voxels=8)
        n_comp = len(comps.voxels)
    return int(appeared.sum()), int(removed.sum()), int(changed.sum()), n_comp


def reached_blocks(M, m, ref, T, vs):
    """distinct TSDF blocks of `ref` that the trilinear corners of m's observed voxels fall into (host arithmetic: a byte estimate)"""
    keys = m.block_indices(M.LAYER_TSDF)
    blocks, _ = m.get_blocks(M.LAYER_TSDF, keys)
    t = np.arange(512)
    lane = np.stack([t >> 6, (t >> 3) & 7, t & 7], 1)
    g = (8 * keys.astype(np.int64)[:, None, :] + lane[None])[blocks["weight"] >= F32(MIN_W)]
    R, tr = inverse_pair(T)
    pr = ((g + 0.5) * vs) @ R.astype(np.float64).T + tr
    b = np.floor(pr / vs - 0.5).astype(np.int64)
    have = {tuple(k) for k in ref.block_indices(M.LAYER_TSDF).tolist()}
    seen = set()
    for o in range(8):
        c = (b + ((o & 1), (o >> 1) & 1, o >> 2)) >> 3
        seen |= {tuple(k) for k in np.unique(c, axis=0).tolist()}
    return len(seen & have)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--stride", type=int, default=4, help="every stride-th pose of the 200 is fused")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    maps = []
    for scene in (S.Scene(), S.Scene(sphere_c=MOVED)):
        m = M.Mapper(M.default_params())
        for i in range(0, 200, a.stride):
            T = S.trajectory_pose(i, 200)
            d, _ = S.render(scene, T, cam, color=False)
            m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
        m.synchronize()
        maps.append(m)
    ref, now = maps
    vs = float(now.params.voxel_size)
    n_tsdf = now.num_blocks(M.LAYER_TSDF)
    dev = torch.device("cuda", 0)
    idx = torch.empty((n_tsdf, 3), dtype=torch.int32, device=dev); lab = torch.empty((n_tsdf, 512), dtype=torch.int32, device=dev)
    sc = torch.empty((n_tsdf, 512), dtype=torch.float32, device=dev); ids = torch.empty((n_tsdf, 512), dtype=torch.int32, device=dev)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    rbuf = torch.zeros(M.CHANGE_RESULT_BYTES, dtype=torch.uint8, device=dev)
    rec = now.component_records(1 << 16)
    lines = []

    def emit(r):
        r = {"lib": os.path.basename(_lib.LIB_PATH), "grid_cap": os.environ.get("NVBX_CHANGE_GRID", "default"), **r}
        line = json.dumps(r); print(line, flush=True); lines.append(line)

    sync = lambda: (now.synchronize(), ref.synchronize())      # noqa: E731
    for name, T in (("identity", np.eye(4, dtype=F32)), ("3cm_1.5deg_off", small_pose([0.3, -0.2, 1.0], 1.5, [0.03, -0.01, 0.02]))):
        reached = reached_blocks(M, now, ref, T, vs)
        for sampling in ("trilinear", "nearest"):
            scan = lambda: now.find_changes(ref, T, sampling=sampling, out=(idx, lab, sc, cnt[0:1], rbuf))      # noqa: E731
            call = host_ms(scan, sync, a.calls)
            res = scan()[4]
            n_entries = res.blocks_changed
            spans = {}
            now.set_profiling(True)
            for _ in range(a.calls):
                scan()
            sync()
            for k, v in now.profile().items():
                if "change" in k:
                    spans[k] = round(v["total_ms"] * 1e3 / max(v["count"], 1), 2)
            now.set_profiling(False)
            least = n_tsdf * 4096 + reached * 4096 + n_entries * (8192 + 12)
            span_us = round(sum(spans.values()), 2)
            clusters = lambda: now.change_clusters(ref, T, sampling=sampling, connectivity=26, min_voxels=8,      # noqa: E731
                                                   out=(idx, lab, sc, ids, cnt[0:1], rec, cnt[1:2], rbuf))
            call_c = host_ms(clusters, sync, a.calls)
            row = {"case": "change_scan_room_640x480", "transform": name, "sampling": sampling, "tsdf_blocks": n_tsdf, "ref_blocks_reached": reached,
                   "status": res.status_name, "voxels_compared": res.voxels_compared, "voxels_appeared": res.voxels_appeared, "voxels_removed": res.voxels_removed,
                   "blocks_changed": n_entries, "components": int(cnt[1].item()), "span_us": spans, "scan_span_us": span_us, "least_bytes": least,
                   "share_of_hbm_peak": round(least / HBM_PEAK / (span_us * 1e-6), 4) if span_us else None, "find_changes_ms_mean_min_max": call,
                   "change_clusters_ms_mean_min_max": call_c, "calls": a.calls}
            if sampling == "trilinear":
                comp = host_ms(lambda: compose(torch, M, now, ref, T, vs, True), sync, max(a.calls // 3, 2))
                got = compose(torch, M, now, ref, T, vs, True)
                row.update({"composition_ms_mean_min_max": comp, "composition_over_change_clusters": round(comp[0] / call_c[0], 1),
                            "composition_appeared_removed_blocks_components": list(got),
                            "composition_agrees": got[:3] == (res.voxels_appeared, res.voxels_removed, n_entries)})
            emit(row)
    now.close(); ref.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
