"""Time of a map resampling (nvbx_resample_map) on the bench's room map, beside merge_from at one voxel size and beside the
composition a caller builds from the calls the library already had.

The room map of the 640x480 loop (every second pose of the 200, depth and colour) is built once in `src` at 0.05 m.  It is resampled into an
empty mapper (cleared before every call, outside the timed window) at 0.10 m with 2 taps per axis, at 0.20 m with 4 taps and with 1 tap, and
at 0.05 m with 1 tap -- next to merge_from into the same kind of mapper, in the same run -- each under the identity and under a transform
3 cm and 1.5 degrees off about a general axis:
  - us per launch (count, index, fuse, result: k_transfer_count<Box>, k_transfer_index<Box>, the call's fuse kernel, k_transfer_result) by the
    library's own per-launch event spans (set_profiling);
  - ms of the whole call by a host clock around the call + synchronize (the call waits on the host twice, so the host clock is the honest one);
  - the least bytes the fuse launch has to move, from the call's own counts -- every candidate block's TSDF read once, 8 bytes written per
    fused voxel, 16 per blended colour voxel, every source TSDF and colour block read once -- and that over the span as a share of the
    8 TB/s HBM peak;
  - in the same run, by the same clock, the composition: block_indices of src, the candidate blocks and the tap positions on the host,
    query_tsdf on src, the mean over the valid taps in torch (at least half of them valid), set_blocks.  It has no allocation rule of its
    own, carries no weights (a fused voxel gets the share of valid taps) and no colour, so it does less than the fused call.
One JSON object per line.  Usage: python tools/resample_bench.py [--calls 5] [--out FILE]"""
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
CASES = (("0.05->0.10 n=2", 0.10, 2), ("0.05->0.20 n=4", 0.20, 4), ("0.05->0.20 n=1", 0.20, 1), ("0.05->0.05 n=1", 0.05, 1))


# (the rotation and the candidate boxes restate formulas that csrc/nvbx_resample_math.h and tests/resample_independent.py have too: on purpose --
#  a tool imports nothing from tests/, and the composition must not call the code it is compared with)
def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def candidate_blocks(T, keys, vs, vd, n):
    R = T[:3, :3].astype(np.float64); t = T[:3, 3].astype(np.float64)
    s = np.asarray(keys, np.float64)
    corners = np.stack([(8.0 * s + np.where(np.array([(q >> a) & 1 for a in range(3)]), 8.5, 0.5)) * vs for q in range(8)])      # [8, m, 3]
    pd = corners @ R.T + t
    pad = 0.01 * vs + 0.5 * vd * (1.0 - 1.0 / n)
    kl = np.ceil((pd.min(0) - pad) / vd - 0.5).astype(np.int64) >> 3
    kh = np.floor((pd.max(0) + pad) / vd - 0.5).astype(np.int64) >> 3
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
    n_t = src.num_blocks(M.LAYER_TSDF); n_c = src.num_blocks(M.LAYER_COLOR)
    rng = np.random.default_rng(1)
    Tg = np.eye(4)
    ax = rng.normal(size=3); Tg[:3, :3] = rodrigues(ax, np.deg2rad(1.5))
    dt = rng.normal(size=3); Tg[:3, 3] = dt * 0.03 / np.linalg.norm(dt)
    transforms = {"identity": np.eye(4, dtype=np.float32), "3cm_1.5deg_general_axis": Tg.astype(np.float32)}
    lanes = np.arange(512); lane_xyz = np.stack([lanes >> 6, (lanes >> 3) & 7, lanes & 7], 1)
    lines = []

    def measure(dst, call_fn, fuse_kernel):
        """-> (result record of one call, host ms, us per launch) of call_fn(out) into the cleared dst"""
        buf = torch.empty(M.MERGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
        dst.clear()
        res = call_fn(buf)
        counts = {k: getattr(res, k) for k in ("source_blocks", "candidate_blocks", "blocks_allocated", "voxels_fused", "color_voxels_fused")}
        status = res.status_name
        call = host_ms(lambda: call_fn(buf), dst.synchronize, a.calls, dst.clear)
        spans = {}
        for _ in range(a.calls):                              # spans in calls of their own: profiling adds event records around every launch
            dst.clear()
            dst.set_profiling(True)
            call_fn(buf); dst.synchronize()
            p = dst.profile(); dst.set_profiling(False)
            for k, v in p.items():
                if fuse_kernel in k or "k_transfer" in k:      # (the enumeration and the result record: csrc/nvbx_map_transfer.h)
                    s = spans.setdefault(k, [0.0, 0]); s[0] += v["total_ms"] * 1e3; s[1] += v["count"]
        span_us = {k: round(v[0] / max(v[1], 1), 2) for k, v in spans.items()}
        return status, counts, call, span_us

    for cname, vd, taps in CASES:
        dst = M.Mapper(M.default_params(voxel_size=vd))
        trunc = float(dst.params.truncation_distance_vox * dst.params.voxel_size)
        for tname, T in transforms.items():
            status, counts, call, span_us = measure(dst, lambda buf: dst.resample_from(src, T, out=buf, taps=taps), "k_resample_fuse")
            fuse_us = next((v for k, v in span_us.items() if "k_resample_fuse" in k), None)
            least = counts["candidate_blocks"] * 4096 + counts["voxels_fused"] * 8 + counts["color_voxels_fused"] * 16 + (n_t + n_c) * 4096
            rec = {"case": "resample_room_640x480", "what": cname, "voxel_size_dst": vd, "taps": taps, "transform": tname, "status": status, **counts,
                   "source_color_blocks": int(n_c), "span_us": span_us, "call_ms": round(call[0], 3), "call_ms_min_max": [round(call[1], 3), round(call[2], 3)],
                   "fuse_least_bytes": int(least), "fuse_share_of_hbm_peak": round(least / HBM_PEAK / (fuse_us * 1e-6), 4) if fuse_us else None,
                   "grid_cap": os.environ.get("NVBX_RESAMPLE_GRID", "default"), "calls": a.calls}
            if vd == VS and taps == 1:                        # the merge in the same run, into the same kind of mapper
                m_status, m_counts, m_call, m_span = measure(dst, lambda buf: dst.merge_from(src, T, out=buf), "k_merge_fuse")
                rec.update({"merge_call_ms": round(m_call[0], 3), "merge_call_ms_min_max": [round(m_call[1], 3), round(m_call[2], 3)], "merge_span_us": m_span,
                            "merge_counts_equal": m_counts == counts and m_status == status})

            # the composition from the entry points the library already had
            def composition():
                keys = src.block_indices(M.LAYER_TSDF)
                cand = candidate_blocks(T, keys, VS, vd, taps)
                off = (np.arange(taps, dtype=np.float32) + np.float32(0.5)) / np.float32(taps) - np.float32(0.5)
                o = np.stack(np.meshgrid(off, off, off, indexing="ij"), -1).reshape(-1, 3)                       # [n^3, 3], x outer
                g = (8 * cand[:, None, :] + lane_xyz[None]).astype(np.float32) + np.float32(0.5)                 # [m, 512, 3]
                pd = (g[:, :, None, :] + o[None, None]) * np.float32(vd)
                Ti = np.linalg.inv(T.astype(np.float64))
                ps = (pd.reshape(-1, 3).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
                d, _, v = src.query_tsdf(torch.from_numpy(ps).cuda(), min_weight=1e-4, unknown_value=0.0)
                d = d.reshape(-1, taps ** 3); v = v.reshape(-1, taps ** 3)
                c = v.sum(1)
                fuse = 2 * c >= taps ** 3
                mean = torch.clamp((d * v).sum(1) / torch.clamp(c, min=1), -trunc, trunc)
                out = torch.stack([torch.where(fuse, mean, torch.zeros_like(mean)), torch.where(fuse, c / float(taps ** 3), torch.zeros_like(mean))], 1)
                dst.set_blocks(M.LAYER_TSDF, cand, out.cpu().numpy().astype(np.float32).view(M.TSDF_DT).reshape(len(cand), 512))
                return len(cand), int(fuse.sum())
            dst.clear()
            n_cand, n_fused = composition()
            comp = host_ms(composition, dst.synchronize, max(a.calls // 2, 2), dst.clear)
            rec.update({"composition_ms": round(comp[0], 3), "composition_ms_min_max": [round(comp[1], 3), round(comp[2], 3)],
                        "composition_candidates": n_cand, "composition_voxels_fused": n_fused, "composition_over_call": round(comp[0] / call[0], 2)})
            line = json.dumps(rec); print(line, flush=True); lines.append(line)
        dst.close()
    src.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
