"""Independent float64 model of the colour integrator's per-voxel rule (ProjectiveColorIntegrator as DESIGN.md / SEMANTICS.md restate it): numpy only,
no code shared with the product or with oracle/nvblox_oracle.c.  Per voxel centre of a block in the colour view: layer -> camera frame, pinhole
projection, occlusion test against the synthetic depth (bilinear with validity at 1/sphere_tracing_subsampling resolution, |synthetic - voxel depth| <=
truncation distance), bilinear colour at (u, v), weight-1 blend rounded to u8, weight clamp at max_weight.  The synthetic depth and the colour view are
the caller's (the map under test reports them); everything else is restated here.  A per-voxel "robust" mask leaves out voxels whose DECISIONS hang on
the last bits of a float32 evaluation; it is accumulated over frames (a voxel once decided on a knife edge stays out)."""
import numpy as np

_LIN = np.arange(512)
_VX, _VY, _VZ = _LIN // 64, (_LIN // 8) % 8, _LIN % 8


def decode(image):
    """uint8 [rows, cols, 3] rgb8, or [rows, cols, 4] bgra8 (alpha ignored) -> float64 [rows, cols, 3] in r, g, b order."""
    a = np.asarray(image)
    assert a.ndim == 3 and a.shape[2] in (3, 4), a.shape
    if a.shape[2] == 4:
        a = a[..., [2, 1, 0]]
    return a.astype(np.float64)


def _key(idx):
    return tuple(int(v) for v in idx)


def update(state, block_indices, synth, rgb_f64, T, cam, params):
    """One integrateColor: `block_indices` [n, 3] the colour view, `synth` the synthetic depth [srows, scols] of this frame, `rgb_f64` [rows, cols, 3]
    (decode), T the 4x4 T_L_C, cam (fu, fv, cu, cv, w, h), params anything with voxel_size, truncation_distance_vox, sphere_tracing_subsampling,
    max_integration_distance_m, max_weight.  state: {block key: (colour [512, 3], weight [512], robust [512])}, updated in place and returned."""
    fu, fv, cu, cv, w, h = cam
    vs = float(params.voxel_size); bs = 8 * vs; trunc = float(params.truncation_distance_vox) * vs; f = int(params.sphere_tracing_subsampling)
    max_dist = float(params.max_integration_distance_m); max_w = float(params.max_weight)
    synth = np.asarray(synth, np.float64); srows, scols = synth.shape
    Tm = np.asarray(T, np.float64).reshape(4, 4); R = Tm[:3, :3]; t = Tm[:3, 3]
    img = np.asarray(rgb_f64, np.float64); rows, cols = img.shape[:2]
    for idx in np.asarray(block_indices).reshape(-1, 3):
        key = _key(idx)
        c0, w0, rob_acc = state.get(key, (np.zeros((512, 3)), np.zeros(512), np.ones(512, bool)))
        pl = np.stack([idx[0] * bs + _VX * vs + vs / 2, idx[1] * bs + _VY * vs + vs / 2, idx[2] * bs + _VZ * vs + vs / 2], 1)
        pc = (pl - t) @ R; z = pc[:, 2]; zs = np.where(z > 0, z, 1.0)
        u = fu * pc[:, 0] / zs + cu; v = fv * pc[:, 1] / zs + cv
        ok = (z > 0) & (u >= 0) & (v >= 0) & (u <= w) & (v <= h) & (z <= max_dist)
        # synthetic depth, bilinear with validity at (u / f, v / f)
        us, vs_ = u / f - 0.5, v / f - 0.5
        x0 = np.floor(us).astype(np.int64); y0 = np.floor(vs_).astype(np.int64)
        inb = (x0 >= 0) & (y0 >= 0) & (x0 + 1 <= scols - 1) & (y0 + 1 <= srows - 1)
        xs = np.clip(x0, 0, scols - 2); ys = np.clip(y0, 0, srows - 2)
        s00, s10, s01, s11 = synth[ys, xs], synth[ys, xs + 1], synth[ys + 1, xs], synth[ys + 1, xs + 1]
        sval = (s00 > 0) & (s10 > 0) & (s01 > 0) & (s11 > 0)
        ax, ay = us - np.floor(us), vs_ - np.floor(vs_)
        sd = (1 - ay) * ((1 - ax) * s00 + ax * s10) + ay * ((1 - ax) * s01 + ax * s11)
        occl_ok = np.abs(sd - z) <= trunc
        # colour, bilinear at (u, v)
        uc, vc = u - 0.5, v - 0.5
        cx0 = np.floor(uc).astype(np.int64); cy0 = np.floor(vc).astype(np.int64)
        cin = (cx0 >= 0) & (cy0 >= 0) & (cx0 + 1 <= cols - 1) & (cy0 + 1 <= rows - 1)
        cxs = np.clip(cx0, 0, cols - 2); cys = np.clip(cy0, 0, rows - 2)
        bx, by = (uc - np.floor(uc))[:, None], (vc - np.floor(vc))[:, None]
        col = (1 - by) * ((1 - bx) * img[cys, cxs] + bx * img[cys, cxs + 1]) + by * ((1 - bx) * img[cys + 1, cxs] + bx * img[cys + 1, cxs + 1])
        upd = ok & inb & sval & occl_ok & cin
        blended = np.floor((c0 * (w0 / (w0 + 1))[:, None] + col * (1 / (w0 + 1))[:, None]) + 0.5).clip(0, 255)
        c1 = np.where(upd[:, None], blended, c0); w1 = np.where(upd, np.minimum(w0 + 1, max_w), w0)
        spread = np.maximum.reduce([s00, s10, s01, s11]) - np.minimum.reduce([s00, s10, s01, s11])
        rob = ((np.minimum.reduce([np.abs(u), np.abs(v), np.abs(u - w), np.abs(v - h)]) > 0.02) & (np.abs(z - max_dist) > 1e-3) &
               (np.minimum(np.abs(us - np.round(us)), np.abs(vs_ - np.round(vs_))) > 0.01) & (np.minimum(np.abs(uc - np.round(uc)), np.abs(vc - np.round(vc))) > 0.01) &
               (np.abs(np.abs(sd - z) - trunc) > 2e-3) & ((spread < 0.3) | ~sval) & (z > 0.05))
        state[key] = (c1, w1, rob_acc & rob)
    return state


def compare(state, block_indices, get_blocks):
    """The colour layer of a map against the model.  block_indices [n, 3]: every block the map's colour layer holds; get_blocks(indices) -> [n, 512]
    voxels with fields r, g, b, weight.  Blocks of the model: colour within `worst` on robust voxels, weights exactly equal there.  Every other block
    (never in a colour view): uncoloured.  -> {worst, bad_weight: [keys], coloured_outside: [keys], n_cmp, n_col, n_blocks, n_outside}"""
    idx = np.asarray(block_indices, np.int32).reshape(-1, 3)
    res = dict(worst=0, bad_weight=[], coloured_outside=[], n_cmp=0, n_col=0, n_blocks=0, n_outside=0)
    if len(idx) == 0:
        return res
    blocks = get_blocks(idx)
    for k, i in enumerate(idx):
        key = _key(i); b = blocks[k]
        if key not in state:
            res["n_outside"] += 1
            if (b["weight"] > 0).any():
                res["coloured_outside"].append(key)
            continue
        c1, w1, rob = state[key]
        res["n_blocks"] += 1
        got = np.stack([b["r"], b["g"], b["b"]], 1).astype(np.int64)
        if not np.array_equal(b["weight"][rob].astype(np.float64), w1[rob]):
            res["bad_weight"].append(key)
        res["worst"] = max(res["worst"], int(np.abs(got[rob] - c1[rob]).max(initial=0)))
        res["n_cmp"] += int(rob.sum()); res["n_col"] += int((w1[rob] > 0).sum())
    return res
