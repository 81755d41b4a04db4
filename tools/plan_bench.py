"""Time of the cost field and the path walk (nvbx_cost_field / nvbx_trace_paths) beside the two compositions a caller has without
them, in the same run by the same clock:
  (a) the slice image copied to the host, the moves as a sparse graph, scipy's Dijkstra;
  (b) a torch pull-relaxation on the device: eight shifted minima per sweep over the whole image until a sweep changes nothing.
Two images: the ESDF slice of the room map of the 640x480 loop (every second pose of the 200, depth only), source = the first camera's pixel with
allow_unknown (the camera stands where it never looked), and a 1024 x 1024 synthetic image, a grid of 64-pixel rooms with doors, source in a
corner room.  Reported per image: us of the classify launch and of all relaxation launches of one call by the library's per-launch event spans
(set_profiling), the rounds launched, ms of the whole call and of trace_paths for 64 starts by a host clock around call + synchronize (the
first call warms up), ms of (a) and (b), and once that (a), (b) and the call give the same field.
One JSON object per line.  Usage: python tools/plan_bench.py [--calls 10] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32
UNREACHED = 0x7fffffff
MOVES = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, -1), (-1, 1))


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


# (the classification restates rules that csrc/nvbx_plan_math.h and tests/plan_independent.py have too: on purpose -- a tool imports nothing from
#  tests/, and a composition must not call the code it is compared with)
def classify(xp, v, o):
    """xp: numpy or torch -> (traversable, penalty) of the image v"""
    unknown = xp.abs(v - o["unknown_value"]) < 1e-2
    trav = ~unknown & (v > 0) & (v >= o["robot_radius_m"])
    t = o["inflation_radius_m"] - v
    u = o["penalty_per_m"] * t
    pen = xp.where(t > 0, xp.where(u < o["max_penalty"], xp.trunc(xp.where(u < o["max_penalty"], u, xp.zeros_like(u))), xp.full_like(u, o["max_penalty"])), xp.zeros_like(u))
    if o["allow_unknown"]:
        trav = trav | unknown
    pen = xp.where(unknown, xp.full_like(pen, o["unknown_penalty"]), pen)
    return trav, xp.where(trav, pen, xp.zeros_like(pen))


def shifted(xp, a, dr, dc, fill):
    """b[r, c] = a[r + dr, c + dc], `fill` outside"""
    rows, cols = a.shape
    b = xp.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(rows, rows - dr), max(0, -dc), min(cols, cols - dc)
    b[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return b


def compose_scipy(img_dev, src, o):
    """(a): the image to the host, a sparse graph of the moves, scipy's Dijkstra"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    img = img_dev.cpu().numpy()
    of = {k: (F32(v) if isinstance(v, float) else v) for k, v in o.items()}
    trav, pen = classify(np, img, of)
    pen = pen.astype(np.int64)
    rows, cols = img.shape
    ids = np.arange(rows * cols).reshape(rows, cols)
    s, d, w = [], [], []
    for dr, dc in MOVES:
        ok = trav & shifted(np, trav, dr, dc, False)
        if dr and dc:
            ok &= shifted(np, trav, dr, 0, False) & shifted(np, trav, 0, dc, False)
        s.append(ids[ok]); d.append(shifted(np, ids, dr, dc, -1)[ok]); w.append(((14 if dr and dc else 10) + pen + shifted(np, pen, dr, dc, 0))[ok])
    g = sp.csr_matrix((np.concatenate(w).astype(np.float64), (np.concatenate(s), np.concatenate(d))), shape=(rows * cols, rows * cols))
    acc = [r * cols + c for r, c in src if 0 <= r < rows and 0 <= c < cols and trav[r, c]]
    dist = dijkstra(g, directed=True, indices=acc, min_only=True)
    return np.where(np.isfinite(dist), dist, UNREACHED).astype(np.int32).reshape(rows, cols)


def compose_torch(torch, img_dev, src, o):
    """(b): whole-image pull sweeps on the device; one host read per sweep decides whether to go on -> (field, sweeps)"""
    trav, pen = classify(torch, img_dev, o)
    pen = pen.to(torch.int32)
    G = torch.full(img_dev.shape, UNREACHED, dtype=torch.int32, device=img_dev.device)
    for r, c in src:
        if 0 <= r < G.shape[0] and 0 <= c < G.shape[1] and bool(trav[r, c]):
            G[r, c] = 0
    moves = []
    for dr, dc in MOVES:
        ok = trav & shifted(torch, trav, dr, dc, False)
        if dr and dc:
            ok &= shifted(torch, trav, dr, 0, False) & shifted(torch, trav, 0, dc, False)
        moves.append((dr, dc, ok, (14 if dr and dc else 10) + pen + shifted(torch, pen, dr, dc, 0)))
    big = torch.full_like(G, UNREACHED)
    for sweep in range(1, G.numel() + 2):
        new = G
        for dr, dc, ok, cost in moves:
            gq = shifted(torch, G, dr, dc, UNREACHED)
            new = torch.minimum(new, torch.where(ok & (gq != UNREACHED), gq + cost, big))
        if bool(torch.equal(new, G)):
            return G, sweep
        G = new
    raise RuntimeError("no fixed point")


def room_grid(n=1024, room=64, door=6):
    """n x n image: rooms `room` pixels wide, walls one pixel thick (v < 0) with a door of `door` pixels in every wall; elsewhere the Euclidean
    distance to the nearest wall pixel at 0.05 m per pixel, capped at 1 m"""
    from scipy import ndimage
    r = np.arange(n)
    on_line = r % room == 0
    in_door = (r % room >= room // 2 - door // 2) & (r % room < room // 2 + door // 2)
    wall = (on_line[:, None] & ~in_door[None, :]) | (on_line[None, :] & ~in_door[:, None])
    img = np.minimum(ndimage.distance_transform_edt(~wall) * 0.05, 1.0).astype(F32)
    img[wall] = F32(-0.05)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    scene = S.Scene()
    m = M.Mapper(M.default_params())
    T0 = S.trajectory_pose(0, 200)
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i, 200)
        d, _ = S.render(scene, T, cam, color=False)
        m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
    m.update_esdf()
    room_img, aabb = m.esdf_slice_image_device()
    m.synchronize()
    lines = []

    def emit(r):
        r = {"lib": os.path.basename(_lib.LIB_PATH), **r}
        line = json.dumps(r); print(line, flush=True); lines.append(line)

    grid_img = torch.from_numpy(room_grid()).cuda()
    images = (("room_640x480_slice", room_img, m.slice_pixels(T0[:2, 3].reshape(1, 2), aabb), dict(robot_radius_m=0.15, inflation_radius_m=0.6, allow_unknown=1)),
              ("rooms_with_doors_1024x1024", grid_img, np.array([[32, 32]], np.int32), dict(robot_radius_m=0.10, inflation_radius_m=0.5)))
    for name, img, src, kw in images:
        o = {f: getattr(m.cost_options(**kw), f) for f, _ in _lib.CostOptions._fields_ if f != "pad"}
        src_dev = torch.from_numpy(src).cuda()
        cost = torch.empty(img.shape, dtype=torch.int32, device=img.device); acc = torch.zeros(1, dtype=torch.int32, device=img.device)
        field = lambda: m.cost_field(img, src_dev, out=cost, accepted=acc, **kw)      # noqa: E731
        call = host_ms(field, m.synchronize, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            field()
        m.synchronize()
        prof = {k: v for k, v in m.profile().items() if k.startswith("k_plan")}
        m.set_profiling(False)
        spans = {k: round(v["total_ms"] * 1e3 / a.calls, 2) for k, v in prof.items()}
        rounds = prof.get("k_plan_relax", {}).get("count", 0) // a.calls
        G = cost.cpu().numpy()
        reach = np.argwhere(G != UNREACHED)
        starts = torch.from_numpy(reach[np.linspace(0, len(reach) - 1, 64).astype(np.int64)].astype(np.int32)).cuda()
        cap = 4 * (img.shape[0] + img.shape[1])
        paths = torch.empty((64, cap, 2), dtype=torch.int32, device=img.device); lengths = torch.empty(64, dtype=torch.int32, device=img.device)
        trace = host_ms(lambda: m.trace_paths(img, cost, starts, cap, out=(paths, lengths), **kw), m.synchronize, a.calls)
        src_list = [tuple(int(v) for v in p) for p in src]
        n_a, n_b = max(a.calls // 5, 2), max(a.calls // 3, 2)
        comp_a = host_ms(lambda: compose_scipy(img, src_list, o), m.synchronize, n_a)
        sweeps = []
        comp_b = host_ms(lambda: sweeps.append(compose_torch(torch, img, src_list, o)[1]), torch.cuda.synchronize, n_b)
        same_a = bool(np.array_equal(compose_scipy(img, src_list, o), G))
        same_b = bool(np.array_equal(compose_torch(torch, img, src_list, o)[0].cpu().numpy(), G))
        emit({"case": "cost_field_" + name, "rows": int(img.shape[0]), "cols": int(img.shape[1]), "accepted": int(acc.item()), "reached_pixels": int(len(reach)),
              "largest_cost": int(G[G != UNREACHED].max()) if len(reach) else None, "span_us_per_call": spans, "rounds_launched": int(rounds),
              "rounds_per_wait": int(os.environ.get("NVBX_PLAN_ROUNDS_PER_WAIT", 16)), "call_ms_mean_min_max": call,
              "trace_64_starts_ms_mean_min_max": trace, "longest_path_pixels": int(lengths.max().item()),
              "a_host_scipy_ms_mean_min_max": comp_a, "b_torch_pull_ms_mean_min_max": comp_b, "b_sweeps": sweeps[-1],
              "a_over_call": round(comp_a[0] / call[0], 1), "b_over_call": round(comp_b[0] / call[0], 1), "a_agrees": same_a, "b_agrees": same_b, "calls": a.calls})
        assert same_a and same_b, (name, same_a, same_b)
    m.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
