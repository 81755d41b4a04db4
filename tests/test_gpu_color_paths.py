"""Colour through every path the product has for it, and the depth pair when BOTH of its mappers hold colour.

* The colour layer against the float64 colour model (tests/color_independent.py, no code shared with the product or the checker) on each path a colour
  frame can take -- classic order, held back and carried by the fused two-launch form, carried by nvbx_integrate_depth_pair on mapper a, on mapper b --
  in each encoding: rgb8 and bgra8 tensors (staged), a library-owned frame of 3 bytes per pixel (retained) and one of 4 (nvbx_integrate_color_owned).
  The colours carry real colour information (r != b, per-pixel noise, random alpha in bgra8), so a channel swap or a 3- against 4-byte stride shows up.
  The model is advanced from the product's own synthetic depth and colour view, read right after the call that consumed the colour frame.
* nvbx_integrate_depth_pair against the two nvbx_integrate_depth calls it is defined by, every layer bit for bit, when both mappers hold colour frames in
  every pair of encodings, and with per-mapper settings that differ.  Each test computes from its own schedule how many pair calls must share the pair
  launches and how many must fall back (both mappers hold colour in different encodings), and checks those counts in the first mapper's profile."""
import ctypes as C

import numpy as np
import pytest

import color_independent as CI
import helpers as H
from isaac_ros_nvblox_amd import synthetic as S

pytestmark = pytest.mark.gpu

ENCODINGS = ("rgb8", "bgra8", "owned3", "owned4")
KIND = {"rgb8": 0, "owned3": 0, "bgra8": 1, "owned4": 1}       # the pixel type the library decodes: 3 or 4 bytes per pixel
PATHS = ("classic", "fused", "pair_a", "pair_b")


def colourise(rgb_grey, rng):
    """The synthetic scene's grey checker (64 / 192) -> rgb8 with real colour: r and b differ by ~100 everywhere, per-pixel noise in every channel."""
    g = rgb_grey[..., 0].astype(np.float64)
    base = np.stack([0.75 * g + 40.0, 0.4 * g + 90.0, 250.0 - 0.9 * g], -1)
    return np.clip(np.rint(base + rng.integers(-24, 25, size=base.shape)), 0, 255).astype(np.uint8)


def to_bgra(rgb, rng):
    alpha = rng.integers(0, 255, size=rgb.shape[:2]).astype(np.uint8)          # (never 255: a decoder that reads it as a colour channel shows)
    return np.ascontiguousarray(np.concatenate([rgb[..., ::-1], alpha[..., None]], -1))


class Feeder:
    """integrate_color of one image in one of the four encodings; keeps what the asynchronous uploads read alive until the test ends."""

    def __init__(self, lib, M, torch, dev):
        self.lib, self.M, self.torch, self.dev = lib, M, torch, dev
        self.keep = []

    def __call__(self, m, enc, rgb, bgra, T, cam):
        M, torch, lib = self.M, self.torch, self.lib
        rows, cols = rgb.shape[:2]
        if enc == "rgb8":
            m.integrate_color(torch.from_numpy(rgb).to(self.dev), T, cam)
        elif enc == "bgra8":
            m.integrate_color(torch.from_numpy(bgra).to(self.dev), T, cam)
        elif enc == "owned3":                   # a ColorFrame the mapper retains (nvbx_integrate_color on a frame pointer)
            src = torch.from_numpy(rgb).to(self.dev); self.keep.append(src)
            f = M.ColorFrame(rows, cols, 3)
            f.write(src, stream=m.stream_handle())
            m.integrate_color(f, T, cam)
            f.close()
        else:                                   # the converter's frame, ownership passed with the call
            assert enc == "owned4"
            q = C.c_void_p()
            assert lib.nvbx_color_image_acquire(m._h, rows, cols, 4, C.byref(q)) == 0
            self.keep.append(bgra)
            assert lib.nvbx_frame_upload(q, bgra.ctypes.data_as(C.c_void_p), bgra.nbytes, C.c_void_p(m.stream_handle())) == 0
            Tm = np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4)); self.keep.append(Tm)
            k = M.Camera(*[float(v) for v in cam[:4]], int(cam[4]), int(cam[5]))
            assert lib.nvbx_integrate_color_owned(m._h, q, 4, rows, cols, Tm.ctypes.data_as(C.c_void_p), C.byref(k)) == 0


def _kernel_counts(m):
    names = {}
    for k_, v in m.profile().items():
        names[H.short(k_)] = names.get(H.short(k_), 0) + v["count"]
    return names


def _model_step(M, g, model, img, T, cam, p, tag):
    """Advance the model by the colour frame the last call consumed (the product's own synthetic depth and colour view), then compare the whole layer."""
    CI.update(model, g.last_color_view(), g.synthetic_depth(), img, T, cam, p)
    # (every TSDF block too: one that was never in a colour view must have no colour, whether or not the layer holds a block for it)
    idx = np.unique(np.concatenate([g.block_indices(M.LAYER_TSDF), g.block_indices(M.LAYER_COLOR)]).reshape(-1, 3), axis=0)
    st = CI.compare(model, idx, lambda i: g.get_blocks(M.LAYER_COLOR, i)[0])
    assert not st["coloured_outside"], (tag, "coloured outside every colour view", st["coloured_outside"][:5])
    assert not st["bad_weight"], (tag, "weights differ from the model", st["bad_weight"][:5])
    assert st["worst"] <= 1, (tag, "colour differs from the model", st["worst"])
    return st


def _colour_path_case(hip_lib, path, enc, cam, n_colour):
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    cols = cam[4]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rng = np.random.default_rng(40 + 4 * PATHS.index(path) + ENCODINGS.index(enc))
    pg = M.default_params(max_weight=2.5)           # (colour weights 1, 2, 2.5, 2.5, ...: the clamp and a blend with a fractional weight)
    po = M.default_params(projective_layer_type=1)
    fr = H.frames(n_colour + 1, cam, stride=7, color=True)
    feed = Feeder(hip_lib, M, torch, dev)
    with torch.cuda.stream(stream):
        g = M.Mapper(pg, block_capacity=1 << 13, stream=stream.cuda_stream)
        other = M.Mapper(po, block_capacity=1 << 12, stream=stream.cuda_stream) if path.startswith("pair") else None
        if path == "classic":
            g.set_color_deferral(False)
        g.set_profiling(True)
        if other is not None:
            other.set_profiling(True)
        model = {}; pending = None; st = None
        for i, (d, grey, T) in enumerate(fr):
            fg = d.copy(); fg[:, : cols // 2] = 0.0            # (the occupancy mapper's half)
            if path == "pair_a":
                g.integrate_depth_pair(d, other, fg, T, cam)
            elif path == "pair_b":
                other.integrate_depth_pair(fg, g, d, T, cam)
            else:
                g.integrate_depth(d, T, cam)
            if pending is not None:                           # this depth call carried the held-back colour frame
                st = _model_step(M, g, model, pending[0], pending[1], cam, pg, (path, enc, i))
                pending = None
            if i == n_colour:
                break
            rgb = colourise(grey, rng); bgra = to_bgra(rgb, rng)
            feed(g, enc, rgb, bgra, T, cam)
            img = CI.decode(bgra if KIND[enc] else rgb)
            if path == "classic":
                st = _model_step(M, g, model, img, T, cam, pg, (path, enc, i))
            else:
                pending = (img, T)
        g.synchronize()
        names = _kernel_counts(g)
        if path == "classic":
            assert names.get("k_integrate_color", 0) == n_colour and not {"k_integrate_tsdf_color", "k_integrate_tsdf_color_pair"} & set(names), names
        elif path == "fused":
            assert names.get("k_integrate_tsdf_color", 0) == n_colour and "k_integrate_color" not in names, names
        else:
            first = _kernel_counts(g if path == "pair_a" else other)
            assert first.get("k_integrate_tsdf_color_pair", 0) == n_colour + 1 and first.get("k_mark_view_pair", 0) == n_colour + 1, first
            assert "k_integrate_color" not in names and "k_integrate_tsdf_color" not in names, names
        print("colour model: %s %s %dx%d worst %d compared %d coloured %d blocks %d (+%d outside)" % (
            path, enc, cam[4], cam[5], st["worst"], st["n_cmp"], st["n_col"], st["n_blocks"], st["n_outside"]))
        for m_ in (g, other):
            if m_ is not None:
                m_.close()
    return st


@pytest.mark.parametrize("enc", ENCODINGS)
@pytest.mark.parametrize("path", PATHS)
def test_colour_layer_against_the_model_on_every_path(hip_lib, path, enc):
    """Five colour frames (160x120) through one path in one encoding; the whole colour layer against the model after each."""
    st = _colour_path_case(hip_lib, path, enc, H.SMALL_CAM, 5)
    # measured on every path and encoding: worst 1, 137 177 voxels compared, 43 616 of them coloured, 356 blocks; 171 TSDF blocks outside every
    # colour view (classic order), 211 (held back: one depth frame more)
    assert st["n_cmp"] > 120000 and st["n_col"] > 38000 and st["n_outside"] > 150, st


def test_colour_layer_against_the_model_pair_b_640x480(hip_lib):
    """The foreground-mapper half of the pair at the metric's image size, bgra8."""
    st = _colour_path_case(hip_lib, "pair_b", "bgra8", S.REPLICA_LIKE_CAM, 3)
    # measured: worst 1, 114 362 voxels compared, 39 515 coloured, 267 blocks; 231 TSDF blocks outside every colour view
    assert st["n_cmp"] > 100000 and st["n_col"] > 35000 and st["n_outside"] > 200, st


# ------------------------------------------------------------------------------------------------ the pair against the two calls, both mappers with colour
def _layers_of(M, p):
    if p.projective_layer_type == 1:
        return (M.LAYER_OCCUPANCY, M.LAYER_ESDF)
    return (M.LAYER_TSDF, M.LAYER_COLOR, M.LAYER_ESDF)


def _pair_vs_two_calls(hip_lib, pa, pb, schedule, seed, cam=H.SMALL_CAM, disrupt=True, model_check=False):
    """schedule: one (encoding of a, encoding of b) per pair call, "none" = that mapper holds no colour frame at the call.  Per step: [decay / clearing /
    a slice query / a mesh update -- they carry out whatever is held back] -> the colour frames of the step -> ESDF updates (held back behind them) ->
    the pair (A, B) against the two calls (RA, RB).  Layers compared bit for bit now and then and at the end; the pair and fallback counts from
    A's profile.  model_check: B's colour layer (and A's) against the colour model after every pair call as well."""
    import torch
    from isaac_ros_nvblox_amd import mapper as M
    cols = cam[4]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    rng = np.random.default_rng(seed)
    feed = Feeder(hip_lib, M, torch, dev)
    la, lb = _layers_of(M, pa), _layers_of(M, pb)
    n_fused = n_fallback = 0
    with torch.cuda.stream(stream):
        A = M.Mapper(pa, block_capacity=1 << 13, stream=stream.cuda_stream); B = M.Mapper(pb, block_capacity=1 << 13, stream=stream.cuda_stream)
        RA = M.Mapper(pa, block_capacity=1 << 13, stream=stream.cuda_stream); RB = M.Mapper(pb, block_capacity=1 << 13, stream=stream.cuda_stream)
        A.set_profiling(True)
        fr = H.frames(10, cam, color=True, stride=7)
        models = {id(A): {}, id(B): {}}
        for step, (ea, eb) in enumerate(schedule):
            d, grey, T = fr[int(rng.integers(len(fr)))]
            cut = int(rng.integers(cols // 4, cols)) if rng.random() < 0.85 else cols
            bg = d.copy(); bg[:, cut:] = 0.0
            fg = d.copy(); fg[:, :cut] = 0.0
            if disrupt:
                r = rng.random()
                if r < 0.10:
                    for m_, p_ in ((A, pa), (RA, pa)):
                        m_.decay_occupancy() if p_.projective_layer_type == 1 else m_.decay_tsdf(True)
                elif r < 0.20:
                    for m_, p_ in ((B, pb), (RB, pb)):
                        m_.decay_occupancy() if p_.projective_layer_type == 1 else m_.decay_tsdf(True)
                elif r < 0.27:
                    c = (float(T[0, 3]), float(T[1, 3]), 1.0)
                    for m_ in (A, B, RA, RB):
                        m_.clear_outside_radius(c, 2.5)
                elif r < 0.37:
                    for x, y in ((A, RA), (B, RB)):
                        ix, _ = x.esdf_slice_image(); iy, _ = y.esdf_slice_image()
                        assert ix.shape == iy.shape and np.array_equal(ix, iy), (seed, step)
                elif r < 0.44:
                    for x, y, p_ in ((A, RA, pa), (B, RB, pb)):
                        if p_.projective_layer_type != 1:
                            x.update_color_mesh(); y.update_color_mesh()
            rgb = colourise(grey, rng); bgra = to_bgra(rgb, rng)
            for x, y, e in ((A, RA, ea), (B, RB, eb)):
                if e != "none":
                    feed(x, e, rgb, bgra, T, cam); feed(y, e, rgb, bgra, T, cam)
            if rng.random() < 0.6:
                A.update_esdf(); RA.update_esdf()
            if rng.random() < 0.5:
                B.update_esdf(); RB.update_esdf()
            A.integrate_depth_pair(bg, B, fg, T, cam)
            RA.integrate_depth(bg, T, cam); RB.integrate_depth(fg, T, cam)
            if ea != "none" and eb != "none" and KIND[ea] != KIND[eb]:
                n_fallback += 1
            else:
                n_fused += 1
            if model_check:
                for x, e, p_ in ((A, ea, pa), (B, eb, pb)):
                    if e != "none":
                        _model_step(M, x, models[id(x)], CI.decode(bgra if KIND[e] else rgb), T, cam, p_, ("pair", "a" if x is A else "b", e, step))
            if rng.random() < 0.15:
                H.assert_same_map(A, RA, ("a", seed, step), layers=la); H.assert_same_map(B, RB, ("b", seed, step), layers=lb)
        for m_ in (A, B, RA, RB):
            m_.synchronize()
        H.assert_same_map(A, RA, ("a, end", seed), layers=la); H.assert_same_map(B, RB, ("b, end", seed), layers=lb)
        names = _kernel_counts(A)
        for m_ in (A, B, RA, RB):
            m_.close()
    print("pair: %d calls, %d in the pair launches, %d by the two calls" % (len(schedule), n_fused, n_fallback))
    # the pair launches on exactly the frames the schedule says can share them; the others are the two calls (A's own view-marking launch)
    assert names.get("k_mark_view_pair", 0) == n_fused and names.get("k_integrate_tsdf_color_pair", 0) == n_fused, (n_fused, n_fallback, names)
    assert names.get("k_mark_view", 0) == n_fallback, (n_fused, n_fallback, names)
    return n_fused, n_fallback


ALL = ("none",) + ENCODINGS


def _schedule(rng, n, enc_a=ALL, enc_b=ALL):
    """every (a, b) combination once, then random ones up to n, shuffled"""
    combos = [(a, b) for a in enc_a for b in enc_b]
    extra = [combos[int(rng.integers(len(combos)))] for _ in range(max(0, n - len(combos)))]
    s = combos + extra
    return [s[k] for k in rng.permutation(len(s))]


@pytest.mark.parametrize("seed", [1, 2])
def test_pair_with_colour_on_both_mappers_in_every_pair_of_encodings(hip_lib, seed):
    """Both mappers TSDF + colour; 36 frames whose schedule reaches all 25 (a, b) combinations of {none, rgb8, bgra8, owned-3, owned-4} at a pair call;
    decay, clearing, slice queries, mesh updates and ESDF updates mixed in.  Mixed encodings (8 of the 16 colour-on-both combinations) fall back."""
    from isaac_ros_nvblox_amd import mapper as M
    rng = np.random.default_rng(200 + seed)
    sched = _schedule(rng, 36)
    assert {(a, b) for a in ENCODINGS for b in ENCODINGS} <= set(sched)
    p = M.default_params(tsdf_decay_factor=0.8, tsdf_decayed_weight_threshold=0.3)
    n_fused, n_fallback = _pair_vs_two_calls(hip_lib, p, p, sched, 300 + seed)
    assert n_fallback >= 8 and n_fused >= 17, (n_fused, n_fallback)


@pytest.mark.parametrize("a_enc,b_enc", [("rgb8", "bgra8"), ("bgra8", "rgb8"), ("owned3", "owned4"), ("owned4", "owned3"),
                                         ("bgra8", "owned4"), ("owned3", "rgb8")])
def test_pair_with_colour_on_both_mappers_against_the_model(hip_lib, a_enc, b_enc):
    """Both mappers hold a colour frame at every pair call, in fixed encodings: both colour layers against the colour model after every call, both maps
    against the two calls.  Same pixel type: the pair launches every time; rgb8 against bgra8: the two calls every time."""
    from isaac_ros_nvblox_amd import mapper as M
    p = M.default_params(max_weight=2.5)
    n_fused, n_fallback = _pair_vs_two_calls(hip_lib, p, p, [(a_enc, b_enc)] * 5, 17, disrupt=False, model_check=True)
    assert (n_fused, n_fallback) == ((5, 0) if KIND[a_enc] == KIND[b_enc] else (0, 5))


CASES = ("voxel_size", "truncation_max_weight", "weighting_mode_a", "weighting_mode_b", "roles_swapped")


@pytest.mark.parametrize("case", CASES)
def test_pair_with_per_mapper_settings(hip_lib, case):
    """Each half of the pair reads its own mapper's settings: b at 0.10 m voxels against 0.05; b with another truncation distance and max_weight; a
    non-constant weighting mode on ONE mapper (its frame is not "plain", the other's is); the roles swapped (a occupancy, b TSDF + colour)."""
    from isaac_ros_nvblox_amd import mapper as M
    rng = np.random.default_rng(500 + CASES.index(case))
    pa = M.default_params(); pb = M.default_params()
    enc_a = enc_b = ALL
    if case == "voxel_size":
        pb = M.default_params(voxel_size=0.10)
    elif case == "truncation_max_weight":
        pb = M.default_params(truncation_distance_vox=2.5, max_weight=3.0)
    elif case == "weighting_mode_a":
        pa = M.default_params(weighting_mode=3)
    elif case == "weighting_mode_b":
        pb = M.default_params(weighting_mode=3)
    else:
        pa = M.default_params(projective_layer_type=1, free_region_decay_probability=0.6, occupied_region_decay_probability=0.35)
        enc_a = ("none",)
    sched = _schedule(rng, 30, enc_a, enc_b)
    n_fused, n_fallback = _pair_vs_two_calls(hip_lib, pa, pb, sched, 600 + CASES.index(case))
    assert n_fused >= 17 and (n_fallback >= 8 or case == "roles_swapped"), (n_fused, n_fallback)


def test_colour_batch_refuses_a_bgra8_frame(hip_lib):
    """nvbx_integrate_color_batch takes rgb8 only: a 4-channel ColorFrame is an error before anything is launched, not an image decoded as rgb8."""
    from isaac_ros_nvblox_amd import mapper as M
    cam = H.SMALL_CAM
    g = M.Mapper(M.default_params(), block_capacity=1 << 12)
    g.set_profiling(True)
    f = M.ColorFrame(cam[5], cam[4], 4)
    T = np.eye(4, dtype=np.float32)
    with pytest.raises(ValueError):
        g.integrate_color_batch([f, f], [T, T], cam)
    g.synchronize()
    assert not [k for k in g.profile() if H.short(k).startswith("k_")], g.profile()
    f.close(); g.close()
