"""Time of a feature segmentation (nvbx_segment_features) on the bench's room map, beside what the caller had before it.

The room map of the 640x480 loop (synthetic.sequence, every second pose of the 200) is built once and feature frames (C = 64, stride 16, a 30 x 40
grid) are integrated at every eighth of those poses.  Then, for Q = 32 random queries, cosine metric, one threshold for all queries at the median
best score, connectivity 6 and 26, min_voxels 1:
  - us per launch of segment_features by the library's own event spans (set_profiling): the match, the threshold and the seven labelling launches;
  - us per segment_features(out=...) call by events on torch's stream around many calls;
  - us per match_features(out=...) call the same way: what the library could do before;
  - the composition a caller had: match_features, then labels and scores copied to the host (timed on their own), then the threshold,
    a dense volume and scipy.ndimage.label per label with the components' sizes, boxes and centres on the CPU (host clock around a synchronise).
One JSON object per line.  Usage: python tools/segment_bench.py [--calls 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STRIDE = 16
CHANNELS = 64
QUERIES = 32
LAUNCHES = ("k_match_features", "k_seg_threshold", "k_seg_local", "k_seg_border", "k_seg_count", "k_seg_compact", "k_seg_records", "k_seg_peak", "k_seg_finish")


def span_us(p, needle):
    ks = [k for k in p if needle in k]
    n = sum(p[k]["count"] for k in ks)
    return (sum(p[k]["total_ms"] for k in ks) * 1e3 / n if n else float("nan")), n


def event_us(torch, fn, calls):
    """mean us of fn() by events on torch's current stream (the mapper's calls are ordered behind and ahead of it)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a = torch.cuda.Event(enable_timing=True); b = torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def host_components(idx, lab, sc, thr, connectivity):
    """the CPU side of the composition: threshold, dense volume, scipy.ndimage.label per label, sizes / boxes / centres -> number of components"""
    from scipy import ndimage
    lab = np.where((lab >= 0) & (sc < thr), -1, lab)
    lo = idx.min(0); nb = idx.max(0) - lo + 1
    dense = np.full(tuple(nb) + (8, 8, 8), -1, np.int32)
    p = idx - lo
    dense[p[:, 0], p[:, 1], p[:, 2]] = lab.reshape(-1, 8, 8, 8)
    dense = dense.transpose(0, 3, 1, 4, 2, 5).reshape(nb[0] * 8, nb[1] * 8, nb[2] * 8)
    st = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    n = 0
    for q in np.unique(lab[lab >= 0]):
        cc, k = ndimage.label(dense == q, structure=st)
        if k:
            ndimage.find_objects(cc); ndimage.center_of_mass(cc > 0, cc, np.arange(1, k + 1)); np.bincount(cc.ravel())
        n += k
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    frames = [(torch.from_numpy(d).cuda(), T) for d, _, T in (x for i, x in enumerate(S.sequence(200, n_frames_in_loop=200)) if i % 2 == 0)]
    C, Q = CHANNELS, QUERIES
    m = M.Mapper(M.default_params())
    for d, Tf in frames:
        m.integrate_depth(d, Tf, cam)
    m.enable_features(C)
    rng = np.random.default_rng(C)
    for _, Tf in frames[::8]:
        feat = torch.from_numpy(rng.standard_normal((cam[5] // STRIDE, cam[4] // STRIDE, C)).astype(np.float16)).cuda()
        m.integrate_features(feat, Tf, cam, STRIDE)
    n = m.num_blocks(M.LAYER_FEATURE)
    q = torch.from_numpy(rng.standard_normal((Q, C)).astype(np.float16)).cuda()
    dev = "cuda"
    idx = torch.empty((n, 3), dtype=torch.int32, device=dev); lab = torch.empty((n, 512), dtype=torch.int32, device=dev)
    sc = torch.empty((n, 512), dtype=torch.float32, device=dev); ids = torch.empty((n, 512), dtype=torch.int32, device=dev)
    bc = torch.empty(1, dtype=torch.int64, device=dev); cc = torch.empty(1, dtype=torch.int64, device=dev)
    rec = m.component_records(n * 512)
    m.match_features(q, "cosine", 1.0, out=(idx, lab, sc, None, bc))
    best = sc[lab >= 0]
    median = float(best.median().item())
    thr = torch.full((Q,), median, dtype=torch.float32, device=dev)
    lines = []
    for conn in (6, 26):
        def segment():
            m.segment_features(q, "cosine", 1.0, thr, conn, 1, out=(idx, lab, sc, ids, bc, rec, cc))

        def match():
            m.match_features(q, "cosine", 1.0, out=(idx, lab, sc, None, bc))
        segment()                                        # (the first call allocates the scratch)
        seg_call_us = event_us(torch, segment, a.calls)
        match_call_us = event_us(torch, match, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            segment()
        p = m.profile(); m.set_profiling(False)
        spans = {k: round(span_us(p, k)[0], 2) for k in LAUNCHES}
        segment(); torch.cuda.synchronize()
        n_comp = int(cc.item()); kept = int((lab >= 0).sum().item())
        # the composition: match, copy, host labelling (each part by the host clock around a synchronise; the copy goes through pageable memory as a
        # caller's .cpu() does)
        t_match, t_copy, t_host, n_host = [], [], [], 0
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            match(); torch.cuda.synchronize(); t1 = time.perf_counter()
            h_idx, h_lab, h_sc = idx.cpu().numpy(), lab.cpu().numpy(), sc.cpu().numpy(); t2 = time.perf_counter()
            n_host = host_components(h_idx, h_lab, h_sc, np.float32(median), conn); t3 = time.perf_counter()
            t_match.append(t1 - t0); t_copy.append(t2 - t1); t_host.append(t3 - t2)
        assert n_host == n_comp, (n_host, n_comp)
        rec_line = {"case": "segment_features_room_640x480", "channels": C, "queries": Q, "metric": "cosine", "connectivity": conn, "min_voxels": 1,
                    "feature_blocks": n, "workgroups_per_labelling_launch": n, "min_score_median": round(median, 5), "voxels_kept": kept,
                    "components": n_comp, "calls": a.calls, "span_us": spans, "labelling_spans_sum_us": round(sum(v for k, v in spans.items() if k.startswith("k_seg_") and k != "k_seg_threshold"), 2),
                    "segment_call_us": round(seg_call_us, 2), "match_call_us": round(match_call_us, 2),
                    "composition_match_sync_us": round(min(t_match) * 1e6, 1), "composition_copy_to_host_us": round(min(t_copy) * 1e6, 1),
                    "composition_host_label_us": round(min(t_host) * 1e6, 1),
                    "composition_us": round((min(t_match) + min(t_copy) + min(t_host)) * 1e6, 1), "copied_bytes": int(n * (12 + 4096))}
        line = json.dumps(rec_line); print(line, flush=True); lines.append(line)
    m.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
