"""Decay and clearing on DRAWN maps: the model the maintenance kernels (csrc/maintenance.hip: k_decay<OCC>, k_clear_outside, k_clear_shapes and
the hash rebuild) and the CPU checker are judged by.  Plain numpy, single float32 operations; nothing here imports the project or its checker
(tests/test_maintenance_model.py validates it on the CPU against the checker).  Written from SEMANTICS.md, "Decay / clearing" and the occupancy
paragraph.

THE STATE.  A dict from block index (bx, by, bz) to a dict of that block's layers: "tsdf" (TSDF_DT[512]) or "occ" (float32[512] log-odds),
"color" (COLOR_DT[512]), each None where the block does not carry the layer, and "esdf" (bool: the block carries an ESDF block, whose voxels
are not the model's business).  A block with no layer left is not in the dict.  Voxel order z + 8 y + 64 x.  Every operation returns
(new state, cleared): the input is not modified, `cleared` is the sorted unique [n, 3] int32 list of the blocks that lost their projective layer.

THE RULES, each one float32 operation per step (the product is built without contraction, so results compare bit for bit):
  decay_tsdf            w = float32(w0 * factor); a block none of whose voxels has `not (w < thr)` is deallocated with its colour (its ESDF
                        block stays) unless decay_deallocate_decayed_blocks is 0 -- written this way round so that a NaN weight keeps the block;
                        with tsdf_set_free_distance_on_decayed a voxel with w < thr and w0 > 0 becomes (float32(free_vox) * float32(voxel_size), thr);
                        spared blocks and colour-only blocks are untouched.
  decay_occupancy       v > 0: v += step_occ (negative), and stops at 0 unless occupancy_decay_to_free; v < 0 (not with to_free): v += step_free,
                        stops at 0; a block that is all 0 afterwards is deallocated unless the keep-blocks switch is set.
  clear_outside_radius  a block of any layer goes iff d2 > float32(r * r), d2 = (dx * dx + dy * dy) + dz * dz, dx = (float32(ix) * bs + bs * 0.5) - cx.
  clear_shapes          a voxel becomes (0, 0) iff its centre ((float32(bi) * bs + float32(vi) * vs) + vs * 0.5) lies in a sphere (d2 <= r * r, the
                        sum associated as above) or in a box (inclusive on both faces).
"""
import math

import numpy as np

TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
COLOR_DT = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad", "u1"), ("weight", "<f4")])
F = np.float32
_LIN = np.arange(512)
VOX = np.stack([_LIN // 64, (_LIN // 8) % 8, _LIN % 8], 1)          # (vx, vy, vz) of voxel z + 8 y + 64 x


def make_block(tsdf=None, occ=None, color=None, esdf=False):
    assert tsdf is None or occ is None
    return {"tsdf": None if tsdf is None else np.array(tsdf, TSDF_DT).reshape(512), "occ": None if occ is None else np.array(occ, F).reshape(512),
            "color": None if color is None else np.array(color, COLOR_DT).reshape(512), "esdf": bool(esdf)}


def _copy(b):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def _alive(b):
    return b["tsdf"] is not None or b["occ"] is not None or b["color"] is not None or b["esdf"]


def _cleared(keys):
    a = np.asarray(sorted(set(keys)), np.int32).reshape(-1, 3)
    return a


def layer_keys(state, layer):
    """sorted keys of the blocks that carry `layer` ("tsdf", "occ", "color", "esdf")"""
    return sorted(k for k, b in state.items() if (b[layer] if layer == "esdf" else b[layer] is not None))


def log_odds(p):
    """float32 logit of a probability held in float32 (the product evaluates it once on the host)"""
    p = F(p)
    return F(math.log(float(p / (F(1.0) - p))))


# ------------------------------------------------------------------------------------------------ decay


def decay_tsdf(state, spared, params):
    f = F(params.tsdf_decay_factor); thr = F(params.tsdf_decayed_weight_threshold)
    free_d = F(params.tsdf_decayed_free_distance_vox) * F(params.voxel_size)
    keep_blocks = int(params.decay_deallocate_decayed_blocks) == 0
    to_free = int(params.tsdf_set_free_distance_on_decayed) != 0
    spared = {tuple(int(v) for v in k) for k in np.asarray(spared, np.int64).reshape(-1, 3)} if len(spared) else set()
    out = {}; gone = []
    for key, b in state.items():
        b = _copy(b)
        if b["tsdf"] is not None and key not in spared:
            w0 = b["tsdf"]["weight"]
            with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                w = (w0 * f).astype(F)
                below = w < thr
                survives = bool((~below).any()) or keep_blocks
                if survives:
                    if to_free:
                        sel = below & (w0 > 0)
                        b["tsdf"]["distance"] = np.where(sel, free_d, b["tsdf"]["distance"]).astype(F)
                        w = np.where(sel, thr, w).astype(F)
                    b["tsdf"]["weight"] = w
                else:
                    b["tsdf"] = None; b["color"] = None; gone.append(key)
        if _alive(b):
            out[key] = b
    return out, _cleared(gone)


def decay_occupancy(state, params):
    step_free = log_odds(params.free_region_decay_probability); step_occ = log_odds(params.occupied_region_decay_probability)
    keep_blocks = int(params.decay_deallocate_decayed_blocks) == 0
    to_free = int(params.occupancy_decay_to_free) != 0
    out = {}; gone = []
    for key, b in state.items():
        b = _copy(b)
        if b["occ"] is not None:
            v = b["occ"]
            pos = v > 0; neg = v < 0
            with np.errstate(invalid="ignore", over="ignore"):
                vp = (v + step_occ).astype(F)
                if not to_free:
                    vp = np.where(vp < 0, F(0), vp)
                vn = (v + step_free).astype(F)
                vn = np.where(vn > 0, F(0), vn)
            new = np.where(pos, vp, np.where(neg & (not to_free), vn, v)).astype(F)
            if bool((new != 0).any()) or keep_blocks:
                b["occ"] = new
            else:
                b["occ"] = None; gone.append(key)
        if _alive(b):
            out[key] = b
    return out, _cleared(gone)


# ------------------------------------------------------------------------------------------------ clearing


def block_d2(idx, c, voxel_size):
    """float32 squared distance of the centres of the blocks `idx` [n, 3] from c, as the rule associates it"""
    bs = F(voxel_size) * F(8.0)
    half = bs * F(0.5)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    d = [((idx[:, a].astype(F) * bs).astype(F) + half).astype(F) - F(c[a]) for a in range(3)]
    d = [x.astype(F) for x in d]
    return (((d[0] * d[0]).astype(F) + (d[1] * d[1]).astype(F)).astype(F) + (d[2] * d[2]).astype(F)).astype(F)


def clear_outside_radius(state, c, r, voxel_size):
    r2 = F(F(r) * F(r))
    keys = list(state)
    if not keys:
        return {}, _cleared([])
    goes = block_d2(keys, c, voxel_size) > r2
    out = {}; gone = []
    for key, g in zip(keys, goes):
        b = state[key]
        if g:
            if b["tsdf"] is not None or b["occ"] is not None:
                gone.append(key)
        else:
            out[key] = _copy(b)
    return out, _cleared(gone)


def voxel_centres(key, voxel_size):
    """[512, 3] float32 centres of a block's voxels"""
    vs = F(voxel_size); bs = vs * F(8.0); half = vs * F(0.5)
    cols = [(((F(key[a]) * bs) + (VOX[:, a].astype(F) * vs).astype(F)).astype(F) + half).astype(F) for a in range(3)]
    return np.stack(cols, 1)


def shape_mask(key, shapes, voxel_size):
    """[512] bool: the voxels of block `key` whose centre lies in one of `shapes` (("sphere", centre, radius) / ("aabb", min corner, max corner))"""
    c = voxel_centres(key, voxel_size)
    inside = np.zeros(512, bool)
    for sh in shapes:
        a = np.asarray(sh[1], F)
        if sh[0] == "sphere":
            rad = F(sh[2])
            d = [(c[:, k] - a[k]).astype(F) for k in range(3)]
            d2 = (((d[0] * d[0]).astype(F) + (d[1] * d[1]).astype(F)).astype(F) + (d[2] * d[2]).astype(F)).astype(F)
            inside |= d2 <= F(rad * rad)
        else:
            hi = np.asarray(sh[2], F)
            inside |= (c >= a).all(1) & (c <= hi).all(1)
    return inside


def clear_shapes(state, shapes, voxel_size):
    """(new state, cleared = empty: shape clearing deallocates nothing)"""
    out = {}
    for key, b in state.items():
        b = _copy(b)
        proj = b["tsdf"] if b["tsdf"] is not None else b["occ"]
        if proj is not None and len(shapes):
            m = shape_mask(key, shapes, voxel_size)
            if m.any():
                if b["tsdf"] is not None:
                    b["tsdf"]["distance"][m] = 0; b["tsdf"]["weight"][m] = 0
                else:
                    b["occ"][m] = 0
        out[key] = b
    return out, _cleared([])


def shape_touched(state, shapes, voxel_size):
    """sorted keys of the projective blocks with a voxel centre in one of the shapes (the blocks shape clearing dirties), and the voxel count"""
    keys = [k for k, b in state.items() if (b["tsdf"] is not None or b["occ"] is not None) and len(shapes)]
    masks = {k: shape_mask(k, shapes, voxel_size) for k in keys}
    return sorted(k for k in keys if masks[k].any()), int(sum(m.sum() for m in masks.values()))


# ------------------------------------------------------------------------------------------------ comparing a state with a read-back


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_floats(a, b):
    """bit for bit, except that a NaN equals any NaN"""
    a = np.ascontiguousarray(a, F); b = np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def assert_state_equals(tag, state, read):
    """`read`: {"tsdf" | "occ" | "color": (indices [n, 3], voxels [n, 512]), "esdf": indices} as read back from a map.  Per layer the same
    duplicate-free block set, and every voxel of every block bit for bit (a NaN as "is NaN")."""
    for layer in ("tsdf", "occ", "color", "esdf"):
        if layer not in read:
            assert not layer_keys(state, layer), (tag, layer, "the model holds blocks of a layer that was not read back")
            continue
        idx = read[layer] if layer == "esdf" else read[layer][0]
        got = [tuple(int(v) for v in i) for i in np.asarray(idx).reshape(-1, 3)]
        assert len(got) == len(set(got)), (tag, layer, "a block is listed twice")
        want = layer_keys(state, layer)
        assert sorted(got) == want, (tag, layer, "block sets differ: only read %s, only model %s" % (sorted(set(got) - set(want))[:5], sorted(set(want) - set(got))[:5]))
        if layer == "esdf":
            continue
        vox = read[layer][1]
        for k, key in enumerate(got):
            m = state[key][layer]
            if layer == "occ":
                ok = same_floats(vox[k], m)
                assert ok, (tag, layer, key, "log-odds differ at voxels", _first_diff(vox[k], m))
            elif layer == "tsdf":
                for f in ("weight", "distance"):
                    assert same_floats(vox[k][f], m[f]), (tag, layer, key, f, _first_diff(vox[k][f], m[f]))
            else:
                assert np.ascontiguousarray(vox[k]).tobytes() == np.ascontiguousarray(m).tobytes(), (tag, layer, key)


def _first_diff(a, b):
    a = np.asarray(a, F); b = np.asarray(b, F)
    bad = (bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))
    v = np.nonzero(bad)[0][:4]
    return v.tolist(), a[v].tolist(), b[v].tolist()
