"""Time of a feature merge (nvbx_merge_features) on the bench's room map, beside the composition a caller builds from
feature_blocks / set_feature_blocks and beside the TSDF merge's fuse launch on the same map.

The room map of the 640x480 loop (every second pose of the 200, depth and colour, and a feature frame per pose at stride 16) is built once
per channel count (C = 32 and 64) in `src`.  `dst` is a merge_from copy of it with the feature layer on; src's features are merged into it
under the identity and under a transform 3 cm and 1.5 degrees off about a general axis.  The first call of a case flags dst's blocks; the
timed calls after it blend into blocks that carry features -- the steady state: dst read and written, src read.
  - us per launch (k_feature_merge_index, k_feature_merge_fuse, k_feature_merge_result) by the library's own per-launch event spans
    (set_profiling), next to an empty event pair; k_merge_fuse of merge_from on the same pair of maps, by the same spans, in the same run;
  - ms of the whole call by a host clock around merge_features_from + synchronize (the call waits on the host once, for src's block count);
  - the least bytes the fuse launch has to move, from the call's own count: per fused voxel its C halfs and its weight, read from src, read
    from dst and written to dst -- and that over the span as a share of the 8 TB/s HBM peak;
  - in the same run, by the same clock, the composition: feature_blocks of src and of dst's blocks (to the host, the public layout), the
    containing voxel, a gather and the blend in torch on the device, set_feature_blocks back.
One JSON object per line.  Usage: python tools/feature_merge_bench.py [--channels 32 64] [--calls 5] [--out FILE]"""
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
STRIDE = 16


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


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
    return float(np.mean(times)), float(np.min(times)), float(np.max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    scene = S.Scene()
    frames = []
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i, 200)
        d, rgb = S.render(scene, T, cam)
        frames.append((torch.from_numpy(d).cuda(), torch.from_numpy(rgb).cuda(), T))
    rng = np.random.default_rng(1)
    Tg = np.eye(4)
    Tg[:3, :3] = rodrigues(rng.normal(size=3), np.deg2rad(1.5))
    dt = rng.normal(size=3); Tg[:3, 3] = dt * 0.03 / np.linalg.norm(dt)
    transforms = {"identity": np.eye(4, dtype=np.float32), "3cm_1.5deg_general_axis": Tg.astype(np.float32)}
    lanes = torch.arange(512, device="cuda")
    lane_xyz = torch.stack([lanes >> 6, (lanes >> 3) & 7, lanes & 7], 1)
    lines = []
    for C in a.channels:
        src = M.Mapper(M.default_params()); src.set_color_deferral(False)
        src.enable_features(C)
        frng = np.random.default_rng(C)
        for d, rgb, T in frames:
            src.integrate_depth(d, T, cam); src.integrate_color(rgb, T, cam)
            feat = torch.from_numpy(frng.standard_normal((cam[5] // STRIDE, cam[4] // STRIDE, C)).astype(np.float16)).cuda()
            src.integrate_features(feat, T, cam, STRIDE)
        src.synchronize()
        max_w = float(src.params.max_weight)
        for tname, T in transforms.items():
            dst = M.Mapper(M.default_params())
            dst.enable_features(C)
            mbuf = torch.empty(M.MERGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
            dst.merge_from(src, T, out=mbuf)
            buf = torch.empty(M.FEATURE_MERGE_RESULT_BYTES, dtype=torch.uint8, device="cuda")
            first = dst.merge_features_from(src, T, out=buf)           # flags dst's blocks
            first_counts = {k: getattr(first, k) for k in ("source_blocks", "candidate_blocks", "blocks_flagged", "voxels_fused")}
            res = dst.merge_features_from(src, T, out=buf)
            counts = {k: getattr(res, k) for k in ("source_blocks", "candidate_blocks", "blocks_flagged", "voxels_fused")}
            status = res.status_name
            call = host_ms(lambda: dst.merge_features_from(src, T, out=buf), dst.synchronize, a.calls)
            spans = {}
            pair_us = None
            for _ in range(a.calls):                                  # spans in calls of their own: profiling adds event records around every launch
                dst.set_profiling(True)
                dst.merge_features_from(src, T, out=buf); dst.synchronize()
                p = dst.profile(); dst.set_profiling(False)
                for k, v in p.items():
                    if "k_feature_merge" in k:
                        s = spans.setdefault(k, [0.0, 0]); s[0] += v["total_ms"] * 1e3; s[1] += v["count"]
                if "_empty_event_pair" in p and p["_empty_event_pair"]["count"]:
                    pair_us = p["_empty_event_pair"]["total_ms"] * 1e3 / p["_empty_event_pair"]["count"]
            span_us = {k: round(v[0] / max(v[1], 1), 2) for k, v in spans.items()}
            fuse_us = next((v for k, v in span_us.items() if "k_feature_merge_fuse" in k), None)
            least = counts["voxels_fused"] * (2 * C + 4) * 3
            # the TSDF merge's fuse launch on the same pair of maps
            tsdf_spans = [0.0, 0]
            for _ in range(a.calls):
                dst.set_profiling(True)
                dst.merge_from(src, T, out=mbuf); dst.synchronize()
                p = dst.profile(); dst.set_profiling(False)
                for k, v in p.items():
                    if "k_merge_fuse" in k:
                        tsdf_spans[0] += v["total_ms"] * 1e3; tsdf_spans[1] += v["count"]
            mres = M.MergeResult(mbuf)

            # the composition: whole blocks through the host in the public layout, the blend in torch on the device
            Ti = np.linalg.inv(T.astype(np.float64))
            R = torch.from_numpy(Ti[:3, :3].astype(np.float32)).cuda(); t = torch.from_numpy(Ti[:3, 3].astype(np.float32)).cuda()

            def composition():
                skeys = src.block_indices(M.LAYER_FEATURE)
                sf, sw, _ = src.feature_blocks(skeys)
                dkeys = dst.block_indices(M.LAYER_TSDF)
                df, dw, _ = dst.feature_blocks(dkeys)
                sf_d = torch.from_numpy(sf).cuda(); sw_d = torch.from_numpy(sw).cuda(); df_d = torch.from_numpy(df).cuda(); dw_d = torch.from_numpy(dw).cuda()
                sk = torch.from_numpy(skeys.astype(np.int64)).cuda() + (1 << 20)
                skey = (sk[:, 0] << 42) | (sk[:, 1] << 21) | sk[:, 2]
                skey, order = torch.sort(skey)
                dk = torch.from_numpy(dkeys.astype(np.int64)).cuda()
                centres = ((8 * dk[:, None, :] + lane_xyz[None]).float() + 0.5) * VS
                n = torch.floor((centres @ R.T + t) / VS).long()
                nb = (n >> 3) + (1 << 20)
                key = (nb[..., 0] << 42) | (nb[..., 1] << 21) | nb[..., 2]
                pos = torch.searchsorted(skey, key).clamp(max=len(skey) - 1)
                found = skey[pos] == key
                blk = order[pos]
                lin = (n[..., 2] & 7) + 8 * (n[..., 1] & 7) + 64 * (n[..., 0] & 7)
                ws = torch.where(found, sw_d[blk, lin], torch.zeros((), device="cuda"))
                ok = ws > 0
                f = sf_d[blk, lin].float()
                tw = dw_d + ws
                safe = torch.where(ok, tw, torch.ones((), device="cuda"))
                v = df_d.float() * (dw_d / safe)[..., None] + f * (ws / safe)[..., None]
                out_f = torch.where(ok[..., None], v.half(), df_d); out_w = torch.where(ok, torch.clamp(tw, max=max_w), dw_d)
                dst.set_feature_blocks(dkeys, out_f.cpu().numpy(), out_w.cpu().numpy())
                return len(dkeys), int(ok.sum())
            n_blocks, n_ok = composition()
            comp = host_ms(composition, dst.synchronize, max(a.calls // 2, 2))
            rec = {"case": "merge_features_room_640x480_stride16", "channels": C, "transform": tname, "status": status, **counts,
                   "first_call": first_counts, "span_us": span_us, "empty_event_pair_us": round(pair_us, 2) if pair_us is not None else None,
                   "call_ms": round(call[0], 3), "call_ms_min_max": [round(call[1], 3), round(call[2], 3)],
                   "fuse_least_bytes": int(least), "fuse_GBps": round(least / (fuse_us * 1e-6) / 1e9, 1) if fuse_us else None,
                   "fuse_share_of_hbm_peak": round(least / HBM_PEAK / (fuse_us * 1e-6), 4) if fuse_us else None,
                   "tsdf_merge_fuse_us": round(tsdf_spans[0] / max(tsdf_spans[1], 1), 2), "tsdf_merge_candidate_blocks": mres.candidate_blocks,
                   "tsdf_merge_voxels_fused": mres.voxels_fused,
                   "composition_ms": round(comp[0], 3), "composition_ms_min_max": [round(comp[1], 3), round(comp[2], 3)],
                   "composition_blocks": n_blocks, "composition_voxels_blended": n_ok, "composition_over_call": round(comp[0] / call[0], 2), "calls": a.calls}
            line = json.dumps(rec); print(line, flush=True); lines.append(line)
            dst.close()
        src.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
