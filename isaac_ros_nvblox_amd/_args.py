"""Argument coercion and output buffers of the mapper's calls (mapper.py): one coercion per kind of input, one tensor -> pointer conversion (`ptr`),
ValueError on bad input.  Writers, converters and exporters: `image` / `depth_image` for what a call is fed, `pose` / `pose_block`, `camera` /
`lidar`, and `frame` for the C argument group of an image with its pose and intrinsics.  Reader calls: `points3` / `poses16` / `pixels2` / `voxels3` and `outputs`.
Pure functions: the target torch.device is an argument, nothing here touches the library or a stream, so they run with torch.device("cpu")
on a machine without a GPU (tests/test_wrapper_args.py).  A call adds no coercion code of its own ("Host language").
"""
import ctypes as C
import numpy as np
import torch

from ._lib import Camera, Lidar

F32, F16, I32, I64, U8 = (torch.float32,), (torch.float16,), (torch.int32,), (torch.int64,), (torch.uint8,)
FLAG = (torch.bool, torch.uint8)      # what a `valid` / `hit` output may be: the kernels write one byte, 0 or 1


def image(a, dev, dtype, what="image", dims=None, channels=None, convert=True):
    """-> a contiguous tensor of `dtype` on `dev`; with dims (the shape in words: "(rows, cols)" for depth, range and mask images, "(rows, cols, 3)"
    for colour) of that many dimensions, the last one of `channels` where given.  A tensor is moved and made contiguous, never converted;
    anything else goes through numpy and is uploaded -- where an array of another dtype IS converted (a float64 depth image, a bool mask:
    what Mapper._dev always did) unless convert=False."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a))
        a = a.to(dtype) if convert else a
    t = (a if a.device == dev else a.to(dev)).contiguous()
    if t.dtype != dtype or (dims and t.dim() != dims.count(",") + 1) or (channels and t.shape[-1] not in channels):
        raise ValueError("%s must be a %s%s array, got %s %s" % (what, dims + " " if dims else "", str(dtype)[6:], tuple(t.shape), t.dtype))
    return t


def depth_image(a, dev, what="depth"):
    """-> ((rows, cols) tensor, "f32" | "u16mm").  THE rule for a depth image in u16 millimetres: a torch.int16 tensor (torch has no uint16
    arithmetic; the kernels read the bits as uint16) or an array numpy calls uint16, whose bits go into an int16 tensor unchanged.  Anything
    else is float32 metres."""
    u16 = a.dtype == torch.int16 if isinstance(a, torch.Tensor) else np.asarray(a).dtype == np.uint16
    if u16 and not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(a).view(np.int16))
    return image(a, dev, torch.int16 if u16 else torch.float32, what, "(rows, cols)"), "u16mm" if u16 else "f32"


def pose(T):      # -> a contiguous float32 (4, 4) numpy array from anything that holds 16 numbers, row-major
    return np.ascontiguousarray(np.asarray(T, np.float32).reshape(4, 4))


def pose_block(poses):      # n poses -> one contiguous float32 (n, 16) numpy array
    return np.ascontiguousarray(np.stack([pose(T) for T in poses]).reshape(len(poses), 16))


def camera(cam):      # a Camera, or (fu, fv, cu, cv, width, height) -> Camera
    return cam if isinstance(cam, Camera) else Camera(float(cam[0]), float(cam[1]), float(cam[2]), float(cam[3]), int(cam[4]), int(cam[5]))


def lidar(lidar):      # a Lidar, or (azimuth divisions, elevation divisions, min range, min elevation, max elevation) -> Lidar
    return lidar if isinstance(lidar, Lidar) else Lidar(int(lidar[0]), int(lidar[1]), float(lidar[2]), float(lidar[3]), float(lidar[4]))


def np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def frame(img, T, model, collapse=True):
    """THE C argument group of an image with its pose and intrinsics: -> ((pointer, rows, cols, pose pointer, byref(model)), keep).
    img: a device tensor (rows, cols[, channels]), or a library-owned frame with .ptr, .rows and .cols (ColorFrame); model: a Camera or a
    Lidar.  keep = (img, pose array, model): what the pointers point into, to be held for as long as the group is in use."""
    T = pose(T)
    p, rows, cols = (ptr(img, collapse), img.shape[0], img.shape[1]) if isinstance(img, torch.Tensor) else (C.c_void_p(img.ptr), img.rows, img.cols)
    return (p, rows, cols, np_ptr(T), C.byref(model)), (img, T, model)


def _rows(a, dev, w, dtype, of, what):
    """-> a contiguous (n, w) tensor of `dtype` on `dev`; `of`: what a row holds, for the message.  A tensor is moved and made contiguous, never
    converted or reshaped; anything else goes through numpy (converted to `dtype`, reshaped to (-1, w)) and is uploaded."""
    if isinstance(a, torch.Tensor):
        p = (a if a.device == dev else a.to(dev)).contiguous()
    else:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(a, getattr(np, str(dtype)[6:])).reshape(-1, w))).to(dev)
    if p.dtype != dtype or p.dim() != 2 or p.shape[1] != w:
        raise ValueError("%s must be an (n, %d) %s array%s, got %s %s" % (what, w, str(dtype)[6:], of, tuple(p.shape), p.dtype))
    return p


def points3(a, dev, what="points"):
    """-> a contiguous (n, 3) float32 tensor on `dev`; moved, converted and reshaped as _rows says."""
    return _rows(a, dev, 3, torch.float32, "", what)


def colors3(a, dev, what="colors"):
    """-> a contiguous (n, 3) uint8 tensor of (r, g, b) on `dev`; moved, converted and reshaped as _rows says."""
    return _rows(a, dev, 3, torch.uint8, " of (r, g, b)", what)


def pixels2(a, dev, what="pixels"):
    """-> a contiguous (n, 2) int32 tensor of (row, col) on `dev`; moved, converted and reshaped as _rows says."""
    return _rows(a, dev, 2, torch.int32, " of (row, col)", what)


def voxels3(a, dev, what="voxels"):
    """-> a contiguous (n, 3) int32 tensor of (x, y, z) on `dev`; moved, converted and reshaped as _rows says."""
    return _rows(a, dev, 3, torch.int32, " of (x, y, z)", what)


def poses16(a, dev, what="poses"):
    """-> a contiguous (n, 16) float32 tensor on `dev` from (n, 4, 4) or (n, 16) row-major poses.  A tensor is moved and made contiguous, never
    converted; anything else goes through numpy (converted to float32) and is uploaded."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 16)))
    if a.dtype != torch.float32 or a.numel() % 16 or (a.dim() and a.shape[-1] not in (4, 16)):
        raise ValueError("%s must be (n, 4, 4) float32, got %s %s" % (what, tuple(a.shape), a.dtype))
    return (a if a.device == dev else a.to(dev)).reshape(-1, 16).contiguous()


def score_records(out, n, dev):
    """The records of score_poses / relocalize_*: `out`, checked, or a new one -- a contiguous int64 [n, 3] tensor on `dev` (24 bytes per pose) --
    and its two views: -> (records, counts int32 [n, 4]: points, valid, inliers, conflicts; abs_residual_q20 int64 [n])."""
    rec, = outputs(None if out is None else (out,), (("score records", (n, 3), I64, True, True),), dev)
    return rec, rec.view(torch.int32).reshape(n, 6)[:, :4], rec[:, 2]


def outputs(out, spec, dev):
    """Allocate a call's outputs, or check the caller's.  spec: rows (name, shape, dtypes, required, wanted).
    out=None: -> a tensor of dtypes[0] per wanted row, None for the others.  Otherwise `out` holds one entry per row: a None in a required
    row is refused, every tensor must lie on `dev`, have the row's shape, one of its dtypes and be contiguous; -> tuple(out)."""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtypes[0], device=dev) if wanted else None for _, shape, dtypes, _, wanted in spec)
    out = tuple(out)
    if len(out) != len(spec):
        raise ValueError("out must hold %d entries (%s), got %d" % (len(spec), ", ".join(row[0] for row in spec), len(out)))
    for t, (name, shape, dtypes, required, _) in zip(out, spec):
        if t is None:
            if required:
                raise ValueError("out needs a %s tensor" % name)
        elif t.device != dev or tuple(t.shape) != tuple(shape) or t.dtype not in dtypes or not t.is_contiguous():
            raise ValueError("out tensor for %s must be contiguous %s %s on %s, got %s %s" % (name, tuple(shape), dtypes[0], dev, tuple(t.shape), t.dtype))
    return out


def sparse_volume(out, dev, count_blocks, scores_required=True, all_queries=None, want_all=False, record_words=0, min_voxels=1):
    """THE spec of the sparse voxel volume (match_features, segment_features, find_frontiers, frontier_clusters), over `outputs`:
    indices [cap, 3] i32, labels [cap, 512] i32, scores [cap, 512] f32 (optional unless scores_required), then with all_queries = Q the score
    matrix [cap, 512, Q] f32 (optional; allocated if want_all), then with record_words > 0 the component ids [cap, 512] i32, then the block
    count (one int64), then with record_words > 0 the record table [any, record_words] i32 (optional) and the component count (one int64).
    out=None: cap = count_blocks() (which may wait), the table holds the worst case cap 512 / min_voxels records.  Otherwise cap is
    out[0]'s and the table's capacity its own.  -> (the tensors in that order, cap, counts); counts, out=None only, is the tensor to wait
    for once: the block count, or with records the two-element tensor that both counts view."""
    if out is None:
        cap = int(count_blocks()); rcap = cap * 512 // min_voxels
    else:
        out = tuple(out)
        if not out or out[0] is None:
            raise ValueError("out needs an indices tensor")
        cap = int(out[0].shape[0])
        rcap = int(out[-2].shape[0]) if record_words and len(out) > 1 and out[-2] is not None else 0
    spec = [("indices", (cap, 3), I32, True, True), ("labels", (cap, 512), I32, True, True), ("scores", (cap, 512), F32, scores_required, True)]
    if all_queries is not None:
        spec.append(("all scores", (cap, 512, all_queries), F32, False, want_all))
    if record_words:
        spec.append(("ids", (cap, 512), I32, True, True))
    spec.append(("block count" if record_words else "count", (1,), I64, True, not record_words))
    if record_words:
        spec += [("components", (rcap, record_words), I32, False, True), ("count", (1,), I64, True, False)]
    t = list(outputs(out, spec, dev))
    if out is not None:
        return tuple(t), cap, None
    counts = t[-1]
    if record_words:      # one tensor for both counts: one wait
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        t[-3], t[-1] = counts[0:1], counts[1:2]
    return tuple(t), cap, counts


def ptr(x, collapse=True):
    """THE tensor -> c_void_p conversion: None and an empty tensor become NULL.  Every entry point the reader calls use takes NULL where
    the count or capacity that sizes the tensor is 0 (its first check reads `n > 0 && !pointer`), and NULL for an optional output means
    'not wanted', which is what an empty one is; the writers' entry points refuse NULL and a zero size in one check, with one text.
    collapse=False: an empty tensor keeps its address -- for an entry point that refuses NULL before it looks at the size, or takes size 0."""
    return C.c_void_p(x.data_ptr()) if x is not None and (x.numel() or not collapse) else None


def result_buffer(out, nbytes, dev):
    """The device record an alignment or a merge writes its result into: `out`, checked, or a new one -- a contiguous, 8-byte aligned
    uint8 tensor of nbytes on `dev`."""
    if out is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if out.device != dev or out.dtype != torch.uint8 or out.numel() != nbytes or not out.is_contiguous() or out.data_ptr() % 8:
        raise ValueError("the result buffer must be a contiguous 8-byte aligned uint8 tensor of %d bytes on %s" % (nbytes, dev))
    return out


def struct_options(struct, defaults_fn, kw, what):
    """-> struct() filled by defaults_fn(byref(it)), then the fields `kw` names replaced; a name that is no field: TypeError.
    A field called merge_color is a flag (any truthy value: 1)."""
    o = struct()
    defaults_fn(C.byref(o))
    names = [f for f, _ in struct._fields_ if f != "pad"]
    for k, v in kw.items():
        if k not in names:
            raise TypeError("unknown %s option %r" % (what, k))
        setattr(o, k, int(bool(v)) if k == "merge_color" else v)
    return o


def subsampling_arg(subsampling):
    """render / view_gain: None -> 0 (the mapper's sphere_tracing_subsampling), else an int >= 1"""
    s = int(subsampling) if subsampling is not None else 0
    if s < 0 or (subsampling is not None and s < 1):
        raise ValueError("subsampling must be >= 1")
    return s
