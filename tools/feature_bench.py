"""Time of a feature frame (nvbx_integrate_features) on the bench's room map.

The room map of the 640x480 loop (synthetic.sequence, every second pose of the 200) is built once per channel count; then, at one pose of the loop,
640 x 480 camera, stride 16 (a 30 x 40 feature grid), for C = 32 and 64: us per integrate_features by the library's own per-launch event spans
(set_profiling), split into its two launches -- trace (k_feature_trace) and update (k_integrate_features) -- and the update's algorithmic bytes
(blocks the frame updates x (values read + written + weights read + written)) with their share of the HBM peak.  Beside it the yardstick: the colour
launch (k_integrate_color, classic order) of a colour frame at the same pose on the same mapper, in the same units.
One JSON object per line.  Usage: python tools/feature_bench.py [--channels 32 64] [--calls 200] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12
POSE_INDEX = 38
STRIDE = 16


def span_us(p, needle):
    ks = [k for k in p if needle in k]
    n = sum(p[k]["count"] for k in ks)
    return (sum(p[k]["total_ms"] for k in ks) * 1e3 / n if n else float("nan")), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    frames = [(torch.from_numpy(d).cuda(), torch.from_numpy(rgb).cuda(), T) for d, rgb, T in
              (x for i, x in enumerate(S.sequence(200, n_frames_in_loop=200)) if i % 2 == 0)]
    T = S.trajectory_pose(POSE_INDEX)
    rgb = torch.from_numpy(S.render(S.Scene(), T, cam)[1]).cuda()
    lines = []
    for C in a.channels:
        m = M.Mapper(M.default_params()); m.set_color_deferral(False)
        for d, c, Tf in frames:
            m.integrate_depth(d, Tf, cam); m.integrate_color(c, Tf, cam)
        m.enable_features(C)
        feat = torch.from_numpy(np.random.default_rng(C).standard_normal((cam[5] // STRIDE, cam[4] // STRIDE, C)).astype(np.float16)).cuda()
        for _ in range(5):
            m.integrate_features(feat, T, cam, STRIDE)
        blocks = m.num_blocks(M.LAYER_FEATURE)          # (one pose so far: the blocks a frame at this pose updates)
        m.set_profiling(True)
        for _ in range(a.calls):
            m.integrate_features(feat, T, cam, STRIDE)
        p = m.profile(); m.set_profiling(False)
        trace_us, _ = span_us(p, "k_feature_trace"); upd_us, n = span_us(p, "k_integrate_features")
        empty = p["_empty_event_pair"]; pair_us = empty["total_ms"] * 1e3 / empty["count"]
        ab = blocks * (2 * 512 * C * 2 + 2 * 2048)
        # the yardstick: the colour launch of a colour frame at the same pose
        m.set_profiling(True)
        for _ in range(a.calls):
            m.integrate_color(rgb, T, cam)
        pc = m.profile(); m.set_profiling(False)
        col_us, _ = span_us(pc, "k_integrate_color")
        col_blocks = m.counters()["color_blocks_updated"]
        cb = col_blocks * 2 * 4096
        rec = {"case": "integrate_features_640x480_stride16", "channels": C, "calls": n, "tsdf_blocks": m.num_blocks(M.LAYER_TSDF), "blocks_updated": blocks,
               "us_per_call": round(trace_us + upd_us, 2), "trace_us": round(trace_us, 2), "update_us": round(upd_us, 2), "empty_event_pair_us": round(pair_us, 2),
               "update_algorithmic_bytes": ab, "update_GBps": round(ab / (upd_us * 1e-6) / 1e9, 1), "update_share_of_hbm_peak": round(ab / (upd_us * 1e-6) / HBM_BPS, 4),
               "color_launch_us": round(col_us, 2), "color_blocks_updated": col_blocks, "color_algorithmic_bytes": cb, "color_GBps": round(cb / (col_us * 1e-6) / 1e9, 1),
               "update_over_color_bytes_per_s": round((ab / upd_us) / (cb / col_us), 2)}
        line = json.dumps(rec); print(line, flush=True); lines.append(line)
        m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
