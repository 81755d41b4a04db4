"""Time of a map merge (nvbx_merge_map) on the bench's room map, beside the composition a caller builds from the calls the
library already had.

The room map of the 640x480 loop (every second pose of the 200, depth and colour) is built once in `src`.  It is merged into an empty mapper
and into a copy of itself (the same blocks, uploaded through set_blocks), under the identity and under a transform 3 cm and 1.5 degrees off
about a general axis:
  - us per launch (k_transfer_count<Box>, k_transfer_index<Box>, k_merge_fuse, k_transfer_result: the enumeration and the result record are
    csrc/nvbx_map_transfer.h's) by the library's own per-launch event spans (set_profiling);
  - ms of the whole call by a host clock around merge_from + synchronize (the call waits on the host twice, so the host clock is the honest one);
    the empty destination is cleared before every call, outside the timed window;
  - the least bytes the fuse launch has to move, from the call's own counts -- every candidate block's TSDF read once, 8 bytes written per
    fused voxel, 16 per blended colour voxel, every source TSDF and colour block read once -- and that over the span as a share of the
    8 TB/s HBM peak (a bandwidth bound: the arithmetic is a few dozen operations per voxel);
  - in the same run, by the same clock, today's composition: block_indices of src, the candidate blocks and their voxel centres on the host,
    query_tsdf on src, get_blocks of dst, a blend in torch, set_blocks back.  It carries no weights (query_tsdf has none: a valid sample
    counts as weight 1) and no colour, so it does less than the fused call.
One JSON object per line.  Usage: python tools/merge_bench.py [--calls 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
VS = 0.05


# (the rotation and the candidate boxes restate formulas that csrc/nvbx_merge_math.h and tests/merge_independent.py have too: on purpose -- a
#  tool imports nothing from tests/, and the composition must not call the code it is compared with)
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def candidate_blocks(T, keys, vs):
    R = T[:3, :3].astype(np.float64); t = T[:3, 3].astype(np.float64)
    s = np.asarray(keys, np.float64)
    corners = np.stack([(8.0 * s + np.where(np.array([(q >> a) & 1 for a in range(3)]), 8.5, 0.5)) * vs for q in range(8)])      # [8, n, 3]
    pd = corners @ R.T + t
    kl = np.ceil((pd.min(0) - 0.01 * vs) / vs - 0.5).astype(np.int64) >> 3
    kh = np.floor((pd.max(0) + 0.01 * vs) / vs - 0.5).astype(np.int64) >> 3
    out = set()
    for l, h in zip(kl, kh):
        for x in range(l[0], h[0] + 1):
            for y in range(l[1], h[1] + 1):
                for z in range(l[2], h[2] + 1):
                    out.add((x, y, z))
    return np.array(sorted(out), np.int32)


def host_ms(fn, sync, calls, before=None):
    """mean and spread (ms) of fn() + sync() by the host clock; before(): untimed preparation of every call"""
    times = []
    for i in range(calls + 1):
        if before:
            before()
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i:                                   # (the first call warms up: code objects, scratch buffers, pool growth)
            times.append((time.perf_counter() - t0) * 1e3)
    return float(np.mean(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    scene = S.Scene()
    src = M.Mapper(M.default_params())
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i, 200)
        d, rgb = S.render(scene, T, cam)
        src.integrate_depth(torch.from_numpy(d).cuda(), T, cam); src.integrate_color(torch.from_numpy(rgb).cuda(), T, cam)
    src.synchronize()
    idx_t = src.block_indices(M.LAYER_TSDF); idx_c = src.block_indices(M.LAYER_COLOR)
    tsdf, _ = src.get_blocks(M.LAYER_TSDF, idx_t); color, _ = src.get_blocks(M.LAYER_COLOR, idx_c)
    rng = np.random.default_rng(1)
    Tg = np.eye(4)
    ax = rng.normal(size=3); Tg[:3, :3] = rodrigues(ax, np.deg2rad(1.5))
    dt = rng.normal(size=3); Tg[:3, 3] = dt * 0.03 / np.linalg.norm(dt)
    transforms = {"identity": np.eye(4, dtype=np.float32), "3cm_1.5deg_general_axis": Tg.astype(np.float32)}
    trunc = float(src.params.truncation_distance_vox * src.params.voxel_size); max_w = float(src.params.max_weight)
    lanes = np.arange(512); lane_xyz = np.stack([lanes >> 6, (lanes >> 3) & 7, lanes & 7], 1)
    lines = []
    for dst_case in ("empty", "copy"):
        dst = M.Mapper(M.default_params())

        def refill():
            dst.clear()
            if dst_case == "copy":
                dst.set_blocks(M.LAYER_TSDF, idx_t, tsdf); dst.set_blocks(M.LAYER_COLOR, idx_c, color)
        for tname, T in transforms.items():
            refill()
            buf = torch.empty(M.MERGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
            res = dst.merge_from(src, T, out=buf)
            counts = {k: getattr(res, k) for k in ("source_blocks", "candidate_blocks", "blocks_allocated", "voxels_fused", "color_voxels_fused")}
            status = res.status_name
            before = refill if dst_case == "empty" else None      # (a copy stays a copy of the block set: merged again as it is)
            call = host_ms(lambda: dst.merge_from(src, T, out=buf), dst.synchronize, a.calls, before)
            spans = {}
            for _ in range(a.calls):                              # spans in calls of their own: profiling adds event records around every launch
                if before:
                    before()
                dst.set_profiling(True)
                dst.merge_from(src, T, out=buf); dst.synchronize()
                p = dst.profile(); dst.set_profiling(False)
                for k, v in p.items():
                    if "k_merge" in k or "k_transfer" in k:
                        s = spans.setdefault(k, [0.0, 0]); s[0] += v["total_ms"] * 1e3; s[1] += v["count"]
            span_us = {k: round(v[0] / max(v[1], 1), 2) for k, v in spans.items()}
            fuse_us = next((v for k, v in span_us.items() if "k_merge_fuse" in k), None)
            least = counts["candidate_blocks"] * 4096 + counts["voxels_fused"] * 8 + counts["color_voxels_fused"] * 16 + (len(idx_t) + len(idx_c)) * 4096

            # the composition from the entry points the library already had
            def composition():
                keys = src.block_indices(M.LAYER_TSDF)
                cand = candidate_blocks(T, keys, VS)
                centres = ((8 * cand[:, None, :] + lane_xyz[None]).astype(np.float32) + np.float32(0.5)) * np.float32(VS)
                Ti = np.linalg.inv(T.astype(np.float64))
                ps = (centres.reshape(-1, 3).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
                d, _, v = src.query_tsdf(torch.from_numpy(ps).cuda(), min_weight=1e-4, unknown_value=0.0)
                blocks, _ = dst.get_blocks(M.LAYER_TSDF, cand)
                cur = torch.from_numpy(blocks.view(np.float32).reshape(-1, 2)).cuda()
                wd = cur[:, 1]; w = wd + 1.0
                fused = torch.clamp((d + cur[:, 0] * wd) / w, -trunc, trunc)
                out = torch.stack([torch.where(v, fused, cur[:, 0]), torch.where(v, torch.clamp(w, max=max_w), wd)], 1)
                dst.set_blocks(M.LAYER_TSDF, cand, out.cpu().numpy().view(M.TSDF_DT).reshape(len(cand), 512))
                return len(cand), int(v.sum())
            if before:
                before()
            n_cand, n_valid = composition()
            comp = host_ms(composition, dst.synchronize, max(a.calls // 2, 2), before)
            rec = {"case": "merge_room_640x480", "dst": dst_case, "transform": tname, "status": status, **counts,
                   "source_color_blocks": int(len(idx_c)), "span_us": span_us, "call_ms": round(call[0], 3), "call_ms_min_max": [round(call[1], 3), round(call[2], 3)],
                   "fuse_least_bytes": int(least), "fuse_share_of_hbm_peak": round(least / HBM_PEAK / (fuse_us * 1e-6), 4) if fuse_us else None,
                   "composition_ms": round(comp[0], 3), "composition_ms_min_max": [round(comp[1], 3), round(comp[2], 3)],
                   "composition_candidates": n_cand, "composition_valid_samples": n_valid,
                   "composition_over_call": round(comp[0] / call[0], 2), "calls": a.calls}
            line = json.dumps(rec); print(line, flush=True); lines.append(line)
        dst.close()
    src.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
