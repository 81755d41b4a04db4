"""Time of the elevation map and of traversability (nvbx_elevation_map / nvbx_traversability) beside the compositions a caller
has without them, in the same run by the same clock:
  (a) for the elevation map: block_indices + get_blocks, the band's voxels gathered into a dense [x, y, z] volume on the host, the column rule in
      numpy;
  (b) for traversability: the 3 x 3 stencil as shifted torch tensors on the device and the distance as one shifted minimum per offset of the disc.
Three maps: the room map of the 640x480 loop and the same loop in the 14 x 12 x 3 m hall (every second pose of the 200, depth only), elevation
over the slice's AABB and the band 0 .. 2 m, and a drawn terrain of 1024 x 1024 columns uploaded with set_blocks (heights from a fixed formula,
two to three blocks deep).  Reported per map: us of the scan, classify and distance launches by the library's per-launch event spans
(set_profiling), ms of the two calls by a host clock around call + synchronize (the first call warms up), the bytes of every TSDF block of the
band under the image plus the 5 bytes written per pixel -- what the scan reads if no column ends early -- and that over the span as a share of
the 8 TB/s HBM peak, ms of (a) and (b), and whether they give the same images.
One JSON object per line.  Usage: python tools/elevation_bench.py [--calls 10] [--out FILE]"""
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
UNKNOWN, SURFACE, BLOCKED, VOID = 0, 1, 2, 3
T_UNKNOWN, T_OK, T_HAZARD = 0, 1, 2


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


# (the rules below restate what csrc/nvbx_terrain_math.h and tests/elevation_independent.py have too: on purpose -- a tool imports nothing from
#  tests/, and a composition must not call the code it is compared with)
def compose_elevation(m, M, box, min_weight, unknown_value):
    """(a): every TSDF block to the host, the band under the image as a dense volume, the column rule in numpy -> (height, status)"""
    x0, y0, rows, cols, z_lo, z_hi = box
    vs = F32(m.params.voxel_size)
    idx = np.asarray(m.block_indices(M.LAYER_TSDF), np.int64).reshape(-1, 3)
    bx0, by0, bz0 = x0 >> 3, y0 >> 3, z_lo >> 3
    nbx, nby, nbz = ((x0 + cols - 1) >> 3) - bx0 + 1, ((y0 + rows - 1) >> 3) - by0 + 1, (z_hi >> 3) - bz0 + 1
    rel = idx - np.array([bx0, by0, bz0])
    keep = np.all((rel >= 0) & (rel < np.array([nbx, nby, nbz])), axis=1)
    D = np.zeros((nbx, nby, nbz, 8, 8, 8), F32); O = np.zeros((nbx, nby, nbz, 8, 8, 8), bool)
    if keep.any():
        vox, found = m.get_blocks(M.LAYER_TSDF, idx[keep].astype(np.int32))
        d = vox["distance"].reshape(-1, 8, 8, 8); w = vox["weight"].reshape(-1, 8, 8, 8)
        r = rel[keep]
        D[r[:, 0], r[:, 1], r[:, 2]] = d
        with np.errstate(invalid="ignore"):
            O[r[:, 0], r[:, 1], r[:, 2]] = (w >= F32(min_weight)) & (d == d)
    D = D.transpose(0, 3, 1, 4, 2, 5).reshape(nbx * 8, nby * 8, nbz * 8); O = O.transpose(0, 3, 1, 4, 2, 5).reshape(nbx * 8, nby * 8, nbz * 8)
    xs, ys, zs = x0 - 8 * bx0, y0 - 8 * by0, z_lo - 8 * bz0
    n = z_hi - z_lo + 1
    D = D[xs:xs + cols, ys:ys + rows, zs:zs + n]; O = O[xs:xs + cols, ys:ys + rows, zs:zs + n]
    solid = O & (D <= 0)
    has = solid.any(2)
    k = n - 1 - np.argmax(solid[:, :, ::-1], axis=2)                         # the topmost solid voxel where there is one
    k1 = np.minimum(k + 1, n - 1)
    take = lambda a, i: np.take_along_axis(a, i[:, :, None], 2)[:, :, 0]      # noqa: E731
    surface = has & (k + 1 < n) & take(O, k1)
    d0, d1 = take(D, k), take(D, k1)
    zt = z_lo + k
    centre = ((zt >> 3).astype(F32) * (vs * F32(8.0)) + (zt & 7).astype(F32) * vs) + vs * F32(0.5)
    with np.errstate(all="ignore"):
        h = centre + vs * ((-d0) / (d1 - d0))
    status = np.where(surface, SURFACE, np.where(has, BLOCKED, np.where(O.any(2), VOID, UNKNOWN))).astype(np.uint8)
    height = np.where(surface, h, F32(unknown_value)).astype(F32)
    return np.ascontiguousarray(height.T), np.ascontiguousarray(status.T)


def shifted(torch, a, dr, dc, fill):
    """b[r, c] = a[r + dr, c + dc], `fill` outside"""
    rows, cols = a.shape
    b = torch.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(rows, rows - dr), max(0, -dc), min(cols, cols - dc)
    if r1 > r0 and c1 > c0:
        b[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return b


def compose_terrain(torch, h, st, o, vs):
    """(b): the stencil and the distance as whole-image torch operations -> (class, step, slope2, distance)"""
    known = st == SURFACE
    zero = torch.zeros_like(h)
    nk = torch.zeros(h.shape, dtype=torch.int32, device=h.device)
    step = zero.clone()
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            kq = shifted(torch, known, dr, dc, False)
            nk += kq.to(torch.int32)
            if dr or dc:
                step = torch.maximum(step, torch.where(kq & known, (h - shifted(torch, h, dr, dc, 0.0)).abs(), zero))

    def grad(dr, dc):
        km, kp = shifted(torch, known, -dr, -dc, False), shifted(torch, known, dr, dc, False)
        hm, hp = shifted(torch, h, -dr, -dc, 0.0), shifted(torch, h, dr, dc, 0.0)
        return torch.where(km & kp, (hp - hm) / (2.0 * vs), torch.where(kp, (hp - h) / vs, torch.where(km, (h - hm) / vs, zero)))
    gx, gy = grad(0, 1), grad(1, 0)
    slope2 = torch.where(known, gx * gx + gy * gy, zero)
    lim = float(F32(o["max_slope_tan"]) * F32(o["max_slope_tan"]))
    bad = ~(step <= o["max_step_m"]) | ~(slope2 <= lim) | (nk < o["min_known"])
    cls = torch.where(known, torch.where(bad, T_HAZARD, T_OK), torch.where((st == BLOCKED) | ((st == VOID) & bool(o["void_is_hazard"])), T_HAZARD, T_UNKNOWN)).to(torch.uint8)
    haz = cls == T_HAZARD
    R = o["distance_radius_px"]
    none = R * R + 1
    mm = torch.full(h.shape, none, dtype=torch.int32, device=h.device)
    for dr in range(-R, R + 1):
        for dc in range(-R, R + 1):
            s = dr * dr + dc * dc
            if s <= R * R:
                mm = torch.where(shifted(torch, haz, dr, dc, False), torch.clamp(mm, max=s), mm)
    dist = torch.where(mm < none, vs * torch.sqrt(mm.to(torch.float32)), torch.full_like(h, float(F32(vs) * F32(R + 1))))
    dist = torch.where(haz, zero, torch.where(cls == T_UNKNOWN, torch.full_like(h, o["unknown_value"]), dist))
    return cls, torch.where(known, step, zero), slope2, dist


def terrain_height(X, Y):
    """the drawn terrain: rolling ground between 0.45 and 1.25 m with a kerb of 0.15 m every 6.4 m along x"""
    return 0.85 + 0.25 * np.sin(X / 3.1) * np.cos(Y / 2.3) + 0.15 * (np.floor(X / 6.4) % 2)


def draw_terrain(m, M, n_blocks=128, chunk=16):
    """n_blocks x n_blocks block columns with d = voxel centre z - terrain_height(x, y), from one block below the column's lowest height to one above
    its highest -> the number of blocks uploaded"""
    vs = float(m.params.voxel_size)
    v = (np.arange(8) + 0.5) * vs
    total = 0
    for bx_base in range(0, n_blocks, chunk):
        ids, data = [], []
        for bx in range(bx_base, bx_base + chunk):
            for by in range(n_blocks):
                X, Y = np.meshgrid(bx * 8 * vs + v, by * 8 * vs + v, indexing="ij")
                H = terrain_height(X, Y)
                for bz in range(int(np.floor((H.min() - 0.2) / (8 * vs))), int(np.floor((H.max() + 0.2) / (8 * vs))) + 1):
                    blk = np.zeros((8, 8, 8), M.TSDF_DT)
                    blk["distance"] = ((bz * 8 * vs + v)[None, None, :] - H[:, :, None]).astype(F32); blk["weight"] = 1.0
                    ids.append((bx, by, bz)); data.append(blk.reshape(512))
        m.set_blocks(M.LAYER_TSDF, np.array(ids, np.int32), np.stack(data))
        total += len(ids)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--terrain-blocks", type=int, default=128, help="block columns per side of the drawn terrain (128: 1024 x 1024 columns)")
    a = ap.parse_args()
    import torch
    from isaac_ros_nvblox_amd import _lib, mapper as M, synthetic as S
    cam = S.REPLICA_LIKE_CAM
    lines = []

    def emit(r):
        r = {"lib": os.path.basename(_lib.LIB_PATH), **r}
        line = json.dumps(r); print(line, flush=True); lines.append(line)

    def scanned(scene):
        m = M.Mapper(M.default_params())
        for i in range(0, 200, 2):
            T = S.trajectory_pose(i, 200)
            d, _ = S.render(scene, T, cam, color=False)
            m.integrate_depth(torch.from_numpy(d).cuda(), T, cam)
        m.update_esdf()
        _, aabb = m.esdf_slice_image_device()
        return m, m.elevation_box(aabb, 0.0, 2.0)

    def drawn():
        m = M.Mapper(M.default_params(), block_capacity=a.terrain_blocks * a.terrain_blocks * 4)
        draw_terrain(m, M, a.terrain_blocks)
        return m, (0, 0, 8 * a.terrain_blocks, 8 * a.terrain_blocks, 0, 40)

    cases = (("room_640x480_loop", lambda: scanned(S.Scene())), ("hall_640x480_loop", lambda: scanned(S.Scene(room_min=(-7.0, -6.0, 0.0), room_max=(7.0, 6.0, 3.0)))),
             ("drawn_terrain_%dx%d" % (8 * a.terrain_blocks, 8 * a.terrain_blocks), drawn))
    for name, make in cases:
        m, box = make()
        m.synchronize()
        x0, y0, rows, cols, z_lo, z_hi = box
        dev = m._cuda
        o = {f: getattr(m.terrain_options(), f) for f, _ in _lib.TerrainOptions._fields_ if f != "pad"}
        vs = float(F32(m.params.voxel_size))
        hgt = torch.empty((rows, cols), dtype=torch.float32, device=dev); st = torch.empty((rows, cols), dtype=torch.uint8, device=dev)
        outs = (torch.empty((rows, cols), dtype=torch.uint8, device=dev),) + tuple(torch.empty((rows, cols), dtype=torch.float32, device=dev) for _ in range(3))
        scan = lambda: m.elevation_map(*box, out=(hgt, st))      # noqa: E731
        trav = lambda: m.traversability(hgt, st, out=outs)       # noqa: E731
        scan_ms = host_ms(scan, m.synchronize, a.calls)
        trav_ms = host_ms(trav, m.synchronize, a.calls)
        m.set_profiling(True)
        for _ in range(a.calls):
            scan(); trav()
        m.synchronize()
        prof = {k: v for k, v in m.profile().items() if k.startswith("k_elevation") or k.startswith("k_terrain")}
        m.set_profiling(False)
        spans = {k: round(v["total_ms"] * 1e3 / a.calls, 2) for k, v in prof.items()}
        idx = np.asarray(m.block_indices(M.LAYER_TSDF), np.int64).reshape(-1, 3)
        under = ((idx[:, 0] >= x0 >> 3) & (idx[:, 0] <= (x0 + cols - 1) >> 3) & (idx[:, 1] >= y0 >> 3) & (idx[:, 1] <= (y0 + rows - 1) >> 3) &
                 (idx[:, 2] >= z_lo >> 3) & (idx[:, 2] <= z_hi >> 3))
        band_bytes = int(under.sum()) * 4096 + rows * cols * 5
        span = spans.get("k_elevation_scan", 0.0)
        n_a, n_b = max(a.calls // 5, 2), max(a.calls // 5, 2)
        comp_a = host_ms(lambda: compose_elevation(m, M, box, 1e-4, 1000.0), m.synchronize, n_a)
        comp_b = host_ms(lambda: compose_terrain(torch, hgt, st, o, vs), torch.cuda.synchronize, n_b)
        ha, sa = compose_elevation(m, M, box, 1e-4, 1000.0)
        h_host, s_host = hgt.cpu().numpy(), st.cpu().numpy()
        same_a = bool(np.array_equal(sa, s_host) and ha.tobytes() == h_host.tobytes())
        cb = compose_terrain(torch, hgt, st, o, vs)
        same_b = {k: bool(torch.equal(x, y)) for k, x, y in zip(("class", "step", "slope2", "distance"), cb, outs)}
        counts = lambda x, n: [int(v) for v in np.bincount(x.reshape(-1), minlength=n)[:n]]      # noqa: E731
        emit({"case": "elevation_" + name, "rows": rows, "cols": cols, "band_vox": [z_lo, z_hi], "tsdf_blocks": int(len(idx)), "blocks_of_the_band_under_the_image": int(under.sum()),
              "status_unknown_surface_blocked_void": counts(s_host, 4), "class_unknown_ok_hazard": counts(outs[0].cpu().numpy(), 3),
              "span_us_per_call": spans, "elevation_map_ms_mean_min_max": scan_ms, "traversability_ms_mean_min_max": trav_ms,
              "band_bytes": band_bytes, "share_of_hbm_peak": round(band_bytes / HBM_PEAK / (span * 1e-6), 4) if span else None,
              "a_blocks_to_host_numpy_ms_mean_min_max": comp_a, "b_torch_stencil_distance_ms_mean_min_max": comp_b,
              "a_over_elevation_map": round(comp_a[0] / scan_ms[0], 1), "b_over_traversability": round(comp_b[0] / trav_ms[0], 1),
              "a_agrees": same_a, "b_agrees": same_b, "calls": a.calls})
        assert same_a, name
        m.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
