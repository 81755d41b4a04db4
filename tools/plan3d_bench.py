"""Time of the cost volume and the 3-D path walk (nvbx_cost_volume / nvbx_trace_paths_3d) beside the two compositions a caller
has without them, in the same run by the same clock:
  (a) the volume copied to the host, the 26 moves as a sparse graph with the corner rule, scipy's Dijkstra;
  (b) a torch pull-relaxation on the device: 26 shifted minima per sweep over the whole volume until a sweep changes nothing.
Two volumes: the dense ESDF box over the allocated blocks of the room map of the 640x480 loop in 3-D ESDF mode (every second pose of the 200,
depth only), source = the first camera's voxel with allow_unknown, and a drawn 256 x 256 x 64 volume, two storeys of 32-voxel rooms with doors in
the walls and hatches in the floors, source in a corner room.  Reported per volume: us of the classify launch and of all relaxation launches of
one call by the library's per-launch event spans (set_profiling), the rounds launched, ms of the whole call and of trace_paths_3d for 64 starts
by a host clock around call + synchronize (the first call warms up), ms of (a) and (b), once that (a), (b) and the call give the same field,
and the bytes the relaxation would move if every tile were active in every round (an upper bound) as a share of the HBM peak.
One JSON object per line.  Usage: python tools/plan3d_bench.py [--calls 10] [--out FILE] [--skip-large-scipy]"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32 = np.float32
UNREACHED = 0x7fffffff
MOVES = [d for d in itertools.product((1, 0, -1), repeat=3) if any(d)]      # (the order does not matter to a field)
BASE = {1: 10, 2: 14, 3: 17}
TILE = (8, 8, 8)                                    # csrc/plan3d.hip
HALO_CELLS = (TILE[0] + 2) * (TILE[1] + 2) * (TILE[2] + 2)
TILE_VOXELS = TILE[0] * TILE[1] * TILE[2]
ROUND_BYTES = 2 * 4 * HALO_CELLS + 4 * TILE_VOXELS  # the least an active tile moves in a round: class and cost words of tile + halo in, every voxel's cost out
HBM_PEAK = 8.0e12                                   # bytes per second, the MI355X's specified peak


def host_ms(fn, sync, calls, warm=True):
    """mean and spread (ms) of fn() + sync() by the host clock; with warm the first call is discarded"""
    times = []
    for i in range(calls + int(warm)):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i or not warm:
            times.append((time.perf_counter() - t0) * 1e3)
    return [round(float(np.mean(times)), 3), round(float(np.min(times)), 3), round(float(np.max(times)), 3)]


# (the classification restates rules that csrc/nvbx_plan_math.h and tests/plan_independent.py have too: on purpose -- a tool imports nothing from
#  tests/, and a composition must not call the code it is compared with)
def classify(xp, v, o):
    """xp: numpy or torch -> (traversable, penalty) of the volume v"""
    unknown = xp.abs(v - o["unknown_value"]) < 1e-2
    trav = ~unknown & (v > 0) & (v >= o["robot_radius_m"])
    t = o["inflation_radius_m"] - v
    u = o["penalty_per_m"] * t
    pen = xp.where(t > 0, xp.where(u < o["max_penalty"], xp.trunc(xp.where(u < o["max_penalty"], u, xp.zeros_like(u))), xp.full_like(u, o["max_penalty"])), xp.zeros_like(u))
    if o["allow_unknown"]:
        trav = trav | unknown
    pen = xp.where(unknown, xp.full_like(pen, o["unknown_penalty"]), pen)
    return trav, xp.where(trav, pen, xp.zeros_like(pen))


def shifted(xp, a, d, fill):
    """b[p] = a[p + d], `fill` outside"""
    b = xp.full_like(a, fill)
    dst, src = [], []
    for n, c in zip(a.shape, d):
        lo, hi = max(0, -c), min(n, n - c)
        if lo >= hi:
            return b
        dst.append(slice(lo, hi)); src.append(slice(lo + c, hi + c))
    b[tuple(dst)] = a[tuple(src)]
    return b


def between(d):
    return [e for e in itertools.product(*[(0, c) if c else (0,) for c in d]) if any(e) and e != tuple(d)]


def allowed(xp, trav, d):
    ok = trav & shifted(xp, trav, d, False)
    for e in between(d):
        ok = ok & shifted(xp, trav, e, False)
    return ok


def compose_scipy(vol_dev, src, o):
    """(a): the volume to the host, a sparse graph of the moves, scipy's Dijkstra"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    vol = vol_dev.cpu().numpy()
    of = {k: (F32(v) if isinstance(v, float) else v) for k, v in o.items()}
    trav, pen = classify(np, vol, of)
    pen = pen.astype(np.int32)
    ids = np.arange(vol.size, dtype=np.int32).reshape(vol.shape)
    s, t, w = [], [], []
    for d in MOVES:
        ok = allowed(np, trav, d)
        s.append(ids[ok]); t.append(shifted(np, ids, d, -1)[ok]); w.append((BASE[sum(map(abs, d))] + pen + shifted(np, pen, d, 0))[ok].astype(np.float64))
    g = sp.csr_matrix((np.concatenate(w), (np.concatenate(s), np.concatenate(t))), shape=(vol.size, vol.size))
    acc = [int(np.ravel_multi_index(p, vol.shape)) for p in src if all(0 <= c < n for c, n in zip(p, vol.shape)) and trav[p]]
    dist = dijkstra(g, directed=True, indices=acc, min_only=True)
    return np.where(np.isfinite(dist), dist, UNREACHED).astype(np.int32).reshape(vol.shape)


def compose_torch(torch, vol_dev, src, o):
    """(b): whole-volume pull sweeps on the device; one host read per sweep decides whether to go on -> (field, sweeps)"""
    trav, pen = classify(torch, vol_dev, o)
    pen = pen.to(torch.int32)
    G = torch.full(vol_dev.shape, UNREACHED, dtype=torch.int32, device=vol_dev.device)
    for p in src:
        if all(0 <= c < n for c, n in zip(p, G.shape)) and bool(trav[p]):
            G[p] = 0
    moves = [(d, allowed(torch, trav, d), BASE[sum(map(abs, d))] + pen + shifted(torch, pen, d, 0)) for d in MOVES]
    big = torch.full_like(G, UNREACHED)
    for sweep in range(1, G.numel() + 2):
        new = G
        for d, ok, cost in moves:
            gq = shifted(torch, G, d, UNREACHED)
            new = torch.minimum(new, torch.where(ok & (gq != UNREACHED), gq + cost, big))
        if bool(torch.equal(new, G)):
            return G, sweep
        G = new
    raise RuntimeError("no fixed point")


def storeys(nx=256, ny=256, nz=64, room=32, door=6):
    """nx x ny x nz volume: rooms `room` voxels wide on two storeys; walls and floors one voxel thick (v < 0), a door `door` voxels wide and 20
    high in every wall, a hatch of door x door voxels in every room's floor; elsewhere the Euclidean distance to the nearest wall voxel at
    0.05 m per voxel, capped at 1 m"""
    from scipy import ndimage
    x, y, z = np.arange(nx), np.arange(ny), np.arange(nz)
    mid = lambda r: (r % room >= room // 2 - door // 2) & (r % room < room // 2 + door // 2)      # noqa: E731
    low = (z % room >= 1) & (z % room <= 20)
    wall_x = (x % room == 0)[:, None, None] & ~(mid(y)[None, :, None] & low[None, None, :])
    wall_y = (y % room == 0)[None, :, None] & ~(mid(x)[:, None, None] & low[None, None, :])
    floor = (z % room == 0)[None, None, :] & ~(mid(x)[:, None, None] & mid(y)[None, :, None])
    wall = wall_x | wall_y | floor
    vol = np.minimum(ndimage.distance_transform_edt(~wall) * 0.05, 1.0).astype(F32)
    vol[wall] = F32(-0.05)
    return vol


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-large-scipy", action="store_true", help="no composition (a) on the drawn volume (it builds a graph of about 10^8 edges)")
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    scene = S.Scene()
    m = M.Mapper(M.default_params(esdf_mode=1))
    T0 = S.trajectory_pose(0, 200)
    for i in range(0, 200, 2):
        T = S.trajectory_pose(i, 200)
        d, _ = S.render(scene, T, cam, color=False)
        m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
    m.update_esdf()
    idx = np.asarray(m.block_indices(M.LAYER_ESDF), np.int32).reshape(-1, 3)
    mn = idx.min(0) * 8
    size = (idx.max(0) + 1) * 8 - mn
    room_vol = m.esdf_dense_grid_device(mn, size, 1000.0)
    m.synchronize()
    lines = []

    def emit(r):
        r = {"lib": os.path.basename(_lib.LIB_PATH), **r}
        line = json.dumps(r); print(line, flush=True); lines.append(line)

    drawn = torch.from_numpy(storeys()).cuda()
    volumes = (("room_640x480_esdf_box", room_vol, m.volume_voxels(T0[:3, 3].reshape(1, 3), mn), dict(robot_radius_m=0.15, inflation_radius_m=0.6, allow_unknown=1), True),
               ("storeys_256x256x64", drawn, np.array([[16, 16, 10]], np.int32), dict(robot_radius_m=0.10, inflation_radius_m=0.5), not a.skip_large_scipy))
    for name, vol, src, kw, with_a in volumes:
        shape = tuple(int(v) for v in vol.shape)
        o = {f: getattr(m.cost_options(**kw), f) for f, _ in _lib.CostOptions._fields_ if f != "pad"}
        src_dev = torch.from_numpy(src).cuda()
        cost = torch.empty(shape, dtype=torch.int32, device=vol.device); acc = torch.zeros(1, dtype=torch.int32, device=vol.device)
        field = lambda: m.cost_volume(vol, src_dev, out=cost, accepted=acc, **kw)      # noqa: E731
        call = host_ms(field, m.synchronize, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            field()
        m.synchronize()
        prof = {k: v for k, v in m.profile().items() if k.startswith("k_plan3d")}
        m.set_profiling(False)
        spans = {k: round(v["total_ms"] * 1e3 / a.calls, 2) for k, v in prof.items()}
        rounds = prof.get("k_plan3d_relax", {}).get("count", 0) // a.calls
        G = cost.cpu().numpy()
        reach = np.argwhere(G != UNREACHED)
        starts = torch.from_numpy(reach[np.linspace(0, len(reach) - 1, 64).astype(np.int64)].astype(np.int32)).cuda()
        cap = 4 * sum(shape)
        paths = torch.empty((64, cap, 3), dtype=torch.int32, device=vol.device); lengths = torch.empty(64, dtype=torch.int32, device=vol.device)
        trace = host_ms(lambda: m.trace_paths_3d(vol, cost, starts, cap, out=(paths, lengths), **kw), m.synchronize, a.calls)
        src_list = [tuple(int(v) for v in p) for p in src]
        sweeps = []
        comp_b = host_ms(lambda: sweeps.append(compose_torch(torch, vol, src_list, o)), torch.cuda.synchronize, max(a.calls // 5, 1))
        same_b = bool(np.array_equal(sweeps[-1][0].cpu().numpy(), G))
        comp_a, same_a = None, None
        if with_a:      # (no warm-up call, and on a large volume one call only: the graph is built from scratch every time, there is nothing to warm)
            got = []
            comp_a = host_ms(lambda: got.append(compose_scipy(vol, src_list, o)), m.synchronize, 1 if vol.numel() > 1 << 20 else 2, warm=False)
            same_a = bool(np.array_equal(got[-1], G))
        ntiles = int(np.prod([-(-s // t) for s, t in zip(shape, TILE)]))
        relax_us = spans.get("k_plan3d_relax", 0.0)
        bound = rounds * ntiles * ROUND_BYTES
        emit({"case": "cost_volume_" + name, "shape": list(shape), "voxels": int(vol.numel()), "tiles": ntiles, "accepted": int(acc.item()), "reached_voxels": int(len(reach)),
              "largest_cost": int(G[G != UNREACHED].max()) if len(reach) else None, "span_us_per_call": spans, "rounds_launched": int(rounds),
              "rounds_per_wait": int(os.environ.get("NVBX_PLAN_ROUNDS_PER_WAIT", 16)), "call_ms_mean_min_max": call,
              "trace_64_starts_ms_mean_min_max": trace, "longest_path_voxels": int(lengths.max().item()),
              "a_host_scipy_ms_mean_min_max": comp_a, "b_torch_pull_ms_mean_min_max": comp_b, "b_sweeps": sweeps[-1][1],
              "a_over_call": round(comp_a[0] / call[0], 1) if comp_a else None, "b_over_call": round(comp_b[0] / call[0], 1), "a_agrees": same_a, "b_agrees": same_b,
              "least_bytes_per_active_tile_round": ROUND_BYTES, "bytes_if_every_tile_were_active_every_round": bound,
              "hbm_peak_share_at_most": round(bound / (relax_us * 1e-6) / HBM_PEAK, 4) if relax_us else None, "calls": a.calls})
        assert same_b and same_a is not False, (name, same_a, same_b)
    m.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
