"""isaac_ros_nvblox_amd/_args.py: the argument coercion of all the mapper's calls and the output-buffer path of its reader calls, on the CPU.
The functions take the target device as an argument and touch neither the library nor a stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from isaac_ros_nvblox_amd import _args as A

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ points3
def test_points3_accepts_list_array_strided_and_empty():
    p = A.points3([[1, 2, 3], [4, 5, 6]], CPU)
    assert p.dtype == torch.float32 and tuple(p.shape) == (2, 3) and p.is_contiguous()
    assert p.tolist() == [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]

    a64 = np.arange(12, dtype=np.float64).reshape(4, 3) * 0.5
    p = A.points3(a64, CPU)
    assert p.dtype == torch.float32 and tuple(p.shape) == (4, 3)
    assert np.array_equal(p.numpy(), a64.astype(np.float32))

    strided = torch.arange(24, dtype=torch.float32).reshape(4, 6)[:, ::2]
    assert not strided.is_contiguous()
    p = A.points3(strided, CPU)
    assert p.is_contiguous() and torch.equal(p, strided)

    same = torch.zeros((5, 3), dtype=torch.float32)
    assert A.points3(same, CPU).data_ptr() == same.data_ptr()          # already right: no copy

    for empty in (np.zeros((0, 3), np.float32), torch.zeros((0, 3), dtype=torch.float32), []):
        p = A.points3(empty, CPU)
        assert p.dtype == torch.float32 and tuple(p.shape) == (0, 3)


def test_points3_refuses_wrong_dtype_and_shape():
    with pytest.raises(ValueError, match=r"points must be an \(n, 3\) float32 array"):
        A.points3(torch.zeros((4, 3), dtype=torch.int32), CPU)
    with pytest.raises(ValueError, match=r"\(4, 2\)"):
        A.points3(torch.zeros((4, 2), dtype=torch.float32), CPU)
    with pytest.raises(ValueError, match="origins"):                   # the message names the argument
        A.points3(torch.zeros(3, dtype=torch.float32), CPU, "origins")


# ------------------------------------------------------------------------------------------------ image, depth_image
DEPTH = dict(dtype=torch.float32, what="depth", dims="(rows, cols)")
COLOR = dict(dtype=torch.uint8, what="rgb", dims="(rows, cols, 3 or 4)", channels=(3, 4))


def test_image_accepts_list_array_strided_empty_and_device_tensor():
    t = A.image([[1, 2], [3, 4]], CPU, **DEPTH)
    assert t.dtype == torch.float32 and t.tolist() == [[1.0, 2.0], [3.0, 4.0]] and t.is_contiguous()

    a = np.arange(12 * 16, dtype=np.float32).reshape(12, 16)
    assert np.array_equal(A.image(a, CPU, **DEPTH).numpy(), a)
    view = a[:, ::2]                                                    # every second column
    assert not view.flags.c_contiguous
    t = A.image(view, CPU, **DEPTH)
    assert t.is_contiguous() and tuple(t.shape) == (12, 8) and np.array_equal(t.numpy(), view)
    tv = torch.from_numpy(a)[:, ::2]
    t = A.image(tv, CPU, **DEPTH)
    assert t.is_contiguous() and torch.equal(t, tv)

    for empty in (np.zeros((0, 16), np.float32), np.zeros((0, 0), np.float32), torch.zeros((0, 16), dtype=torch.float32)):
        t = A.image(empty, CPU, **DEPTH)
        assert t.dtype == torch.float32 and tuple(t.shape) == tuple(empty.shape)
    assert tuple(A.image(np.zeros((0, 4, 3), np.uint8), CPU, **COLOR).shape) == (0, 4, 3)

    same = torch.zeros((12, 16), dtype=torch.float32)
    assert A.image(same, CPU, **DEPTH).data_ptr() == same.data_ptr()     # already right: no copy
    rgb = torch.zeros((4, 5, 3), dtype=torch.uint8)
    assert A.image(rgb, CPU, **COLOR).data_ptr() == rgb.data_ptr()
    assert tuple(A.image(np.zeros((4, 5, 4), np.uint8), CPU, **COLOR).shape) == (4, 5, 4)


def test_image_converts_arrays_but_never_tensors():
    t = A.image(np.array([[1.5, 2.5]], np.float64), CPU, **DEPTH)        # an array of another dtype is converted, as Mapper._dev always did
    assert t.dtype == torch.float32 and t.tolist() == [[1.5, 2.5]]
    assert A.image(np.array([[True, False]]), CPU, torch.uint8, "mask", "(rows, cols)").tolist() == [[1, 0]]
    with pytest.raises(ValueError, match=r"depth must be a \(rows, cols\) float32 array, got \(1, 2\) torch.float64"):
        A.image(torch.zeros((1, 2), dtype=torch.float64), CPU, **DEPTH)
    with pytest.raises(ValueError, match="depth"):
        A.image(torch.zeros((4, 4), dtype=torch.uint8), CPU, **DEPTH)   # a uint8 image is no depth image
    with pytest.raises(ValueError, match="feat must be a"):             # convert=False: nor is an array converted
        A.image(np.zeros((2, 2, 8), np.float32), CPU, torch.float16, "feat", "(rows_f, cols_f, C)", convert=False)
    assert A.image(np.zeros((2, 2, 8), np.float16), CPU, torch.float16, "feat", "(rows_f, cols_f, C)", convert=False).dtype == torch.float16


def test_image_refuses_wrong_rank_and_channel_count():
    with pytest.raises(ValueError, match=r"depth must be a \(rows, cols\) float32 array, got \(5,\)"):
        A.image(np.zeros(5, np.float32), CPU, **DEPTH)                  # 1-D where 2-D is needed
    with pytest.raises(ValueError, match="depth"):
        A.image(torch.zeros((2, 3, 1), dtype=torch.float32), CPU, **DEPTH)
    for ch in (2, 5):
        with pytest.raises(ValueError, match=r"rgb must be a \(rows, cols, 3 or 4\) uint8 array, got \(4, 5, %d\)" % ch):
            A.image(np.zeros((4, 5, ch), np.uint8), CPU, **COLOR)
        with pytest.raises(ValueError, match="rgb"):
            A.image(torch.zeros((4, 5, ch), dtype=torch.uint8), CPU, **COLOR)
    with pytest.raises(ValueError, match="rgb"):
        A.image(np.zeros((4, 5), np.uint8), CPU, **COLOR)
    assert A.image(torch.zeros(7, dtype=torch.int32), CPU, torch.int32).dim() == 1      # no dims given: any rank (Mapper._dev)


def test_depth_image_kinds():
    mm = np.array([[0, 1000, 32768, 65535]], np.uint16)
    t, kind = A.depth_image(mm, CPU)
    assert kind == "u16mm" and t.dtype == torch.int16 and tuple(t.shape) == (1, 4)
    assert t.numpy().view(np.uint16).tolist() == [[0, 1000, 32768, 65535]]          # the bits of a value >= 32768 are kept
    assert t.tolist() == [[0, 1000, -32768, -1]]
    i16 = torch.from_numpy(mm.view(np.int16))
    t, kind = A.depth_image(i16, CPU)
    assert kind == "u16mm" and t.data_ptr() == i16.data_ptr()
    f = torch.full((3, 4), 1.5)
    t, kind = A.depth_image(f, CPU)
    assert kind == "f32" and t.data_ptr() == f.data_ptr()
    for other in (np.full((3, 4), 1.5, np.float32), np.full((3, 4), 1.5), [[1.5, 2.0]], np.array([[1, 2]], np.int16)):      # numpy's int16 is no u16 image
        t, kind = A.depth_image(other, CPU)
        assert kind == "f32" and t.dtype == torch.float32
    for bad in (torch.zeros((3, 4), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.float64), np.zeros(4, np.uint16), torch.zeros(4, dtype=torch.int16)):
        with pytest.raises(ValueError, match="depth"):
            A.depth_image(bad, CPU)


# ------------------------------------------------------------------------------------------------ pose, pose_block, camera, lidar, frame
def test_pose_and_pose_block():
    T = (np.arange(16, dtype=np.float64) * 0.25 - 1.0).reshape(4, 4)
    forms = [A.pose(T.tolist()), A.pose(T.reshape(16)), A.pose(T), A.pose(torch.from_numpy(T))]
    for p in forms:
        assert p.dtype == np.float32 and p.shape == (4, 4) and p.flags.c_contiguous and p.tobytes() == T.astype(np.float32).tobytes()
    assert A.pose(T.T).flags.c_contiguous and np.array_equal(A.pose(T.T), T.T.astype(np.float32))
    with pytest.raises(ValueError):
        A.pose(np.zeros(12))
    block = A.pose_block([T, T.tolist(), T.reshape(16) + 1.0])
    assert block.dtype == np.float32 and block.shape == (3, 16) and block.flags.c_contiguous
    assert block[0].tobytes() == forms[0].tobytes() and block[1].tobytes() == forms[0].tobytes()
    assert np.array_equal(block[2], (T.reshape(16) + 1.0).astype(np.float32))


def test_camera_and_lidar_from_tuple_or_struct():
    from isaac_ros_nvblox_amd._lib import Camera, Lidar
    k = A.camera((80, 81.5, 79.5, 59.5, 160.0, 120))
    assert isinstance(k, Camera) and (k.fu, k.fv, k.cu, k.cv, k.width, k.height) == (80.0, 81.5, 79.5, 59.5, 160, 120)
    assert A.camera(k) is k
    k2 = A.camera(Camera(80.0, 81.5, 79.5, 59.5, 160, 120))
    assert all(getattr(k, f) == getattr(k2, f) for f, _ in Camera._fields_)
    ld = A.lidar((1024.0, 64, 0.1, -0.4, 0.4))
    assert isinstance(ld, Lidar) and A.lidar(ld) is ld
    ld2 = Lidar(1024, 64, 0.1, -0.4, 0.4)
    assert all(getattr(ld, f) == getattr(ld2, f) for f, _ in Lidar._fields_)
    assert (ld.num_azimuth_divisions, ld.num_elevation_divisions) == (1024, 64)


def test_frame_argument_group():
    img = torch.zeros((12, 16, 3), dtype=torch.uint8)
    k = A.camera((8.0, 8.0, 7.5, 5.5, 16, 12))
    T = np.eye(4, dtype=np.float64)
    (p, rows, cols, Tp, kref), keep = A.frame(img, T, k)
    assert p.value == img.data_ptr() and (rows, cols) == (12, 16)
    assert keep[0] is img and keep[2] is k and keep[1].dtype == np.float32 and Tp.value == keep[1].ctypes.data
    assert kref._obj is k
    empty = torch.zeros((12, 16), dtype=torch.float32)[:0]               # an empty view of memory that exists
    assert A.frame(empty, T, k)[0][:3] == (None, 0, 16)
    assert A.frame(empty, T, k, collapse=False)[0][0].value == C.c_void_p(empty.data_ptr()).value      # (the address torch reports for it)

    class Owned:                                                        # what a ColorFrame looks like: an address and its sides
        ptr, rows, cols = 4096, 12, 16
    (p, rows, cols, _, _), keep = A.frame(Owned, T, A.lidar((16, 12, 0.1, -0.4, 0.4)))
    assert (p.value, rows, cols) == (4096, 12, 16) and keep[0] is Owned


# ------------------------------------------------------------------------------------------------ outputs
def _spec(n, want_color=False):
    return (("t", (n,), A.F32, True, True), ("hit", (n,), A.FLAG, False, True), ("color", (n, 3), A.U8, False, want_color))


def test_outputs_allocates_exactly_the_wanted_rows():
    t, h, c = A.outputs(None, _spec(7), CPU)
    assert tuple(t.shape) == (7,) and t.dtype == torch.float32 and t.device == CPU
    assert tuple(h.shape) == (7,) and h.dtype == torch.bool          # the first dtype of the row
    assert c is None
    t, h, c = A.outputs(None, _spec(7, want_color=True), CPU)
    assert tuple(c.shape) == (7, 3) and c.dtype == torch.uint8
    assert all(x.numel() == 0 for x in A.outputs(None, _spec(0, True), CPU))


def test_outputs_passes_a_valid_out_through():
    t = torch.empty(7, dtype=torch.float32); h = torch.empty(7, dtype=torch.uint8)
    got = A.outputs((t, h, None), _spec(7, want_color=True), CPU)      # `out` decides, the wanted flag is not looked at
    assert got[0] is t and got[1] is h and got[2] is None
    got = A.outputs([t, None, None], _spec(7), CPU)                    # an optional row may be None
    assert got[0] is t and got[1] is None


def test_outputs_flag_row_accepts_bool_and_uint8_only():
    t = torch.empty(7, dtype=torch.float32)
    for dt in (torch.bool, torch.uint8):
        assert A.outputs((t, torch.empty(7, dtype=dt), None), _spec(7), CPU)[1].dtype == dt
    with pytest.raises(ValueError, match="hit"):
        A.outputs((t, torch.empty(7, dtype=torch.int8), None), _spec(7), CPU)


def test_outputs_refusals():
    t = torch.empty(7, dtype=torch.float32); h = torch.empty(7, dtype=torch.bool)
    with pytest.raises(ValueError, match="out needs a t tensor"):     # a required row
        A.outputs((None, h, None), _spec(7), CPU)
    with pytest.raises(ValueError, match=r"t must be contiguous \(7,\) torch.float32"):      # shape: names the argument, the shape and the dtype
        A.outputs((torch.empty(8, dtype=torch.float32), h, None), _spec(7), CPU)
    with pytest.raises(ValueError, match="color"):                    # shape of an optional row
        A.outputs((t, h, torch.empty((7, 4), dtype=torch.uint8)), _spec(7), CPU)
    with pytest.raises(ValueError, match="t must be"):                # dtype
        A.outputs((torch.empty(7, dtype=torch.float64), h, None), _spec(7), CPU)
    with pytest.raises(ValueError, match="t must be"):                # contiguity
        A.outputs((torch.empty(14, dtype=torch.float32)[::2], h, None), _spec(7), CPU)
    with pytest.raises(ValueError, match="color"):
        A.outputs((t, h, torch.empty((7, 6), dtype=torch.uint8)[:, ::2]), _spec(7), CPU)
    with pytest.raises(ValueError, match="3 entries"):                # the tuple's length
        A.outputs((t, h), _spec(7), CPU)
    with pytest.raises(ValueError, match="t must be"):                # another device
        A.outputs((torch.empty(7, dtype=torch.float32, device="meta"), h, None), _spec(7), CPU)


# ------------------------------------------------------------------------------------------------ the sparse-volume family
def test_sparse_volume_allocates_from_the_block_count():
    calls = []
    (idx, lab, sc, cnt), cap, counts = A.sparse_volume(None, CPU, lambda: calls.append(1) or 5, scores_required=False)
    assert cap == 5 and calls == [1]
    assert (tuple(idx.shape), idx.dtype) == ((5, 3), torch.int32) and (tuple(lab.shape), lab.dtype) == ((5, 512), torch.int32)
    assert (tuple(sc.shape), sc.dtype) == ((5, 512), torch.float32) and (tuple(cnt.shape), cnt.dtype) == ((1,), torch.int64)
    assert counts is cnt

    vol, cap, counts = A.sparse_volume(None, CPU, lambda: 3, all_queries=4, want_all=True)
    assert len(vol) == 5 and tuple(vol[3].shape) == (3, 512, 4)
    vol, _, _ = A.sparse_volume(None, CPU, lambda: 3, all_queries=4)
    assert vol[3] is None


def test_sparse_volume_with_components_shares_one_count_tensor():
    vol, cap, counts = A.sparse_volume(None, CPU, lambda: 2, record_words=18, min_voxels=4)
    idx, lab, sc, ids, bcnt, rec, ccnt = vol
    assert tuple(ids.shape) == (2, 512) and tuple(rec.shape) == (2 * 512 // 4, 18) and rec.dtype == torch.int32
    assert tuple(counts.shape) == (2,) and counts.dtype == torch.int64
    counts[0] = 11; counts[1] = 22                                     # both counts view it: one wait reads both
    assert int(bcnt) == 11 and int(ccnt) == 22 and tuple(bcnt.shape) == (1,) and tuple(ccnt.shape) == (1,)


def test_sparse_volume_checks_out_at_its_own_capacity():
    i32 = lambda *s: torch.empty(s, dtype=torch.int32)      # noqa: E731
    cnt = torch.empty(1, dtype=torch.int64)
    never = lambda: pytest.fail("out= must not count blocks")      # noqa: E731
    out = (i32(9, 3), i32(9, 512), None, cnt)
    vol, cap, counts = A.sparse_volume(out, CPU, never, scores_required=False)
    assert cap == 9 and counts is None and all(a is b for a, b in zip(vol, out))
    with pytest.raises(ValueError, match="scores"):                   # ... which match_features requires
        A.sparse_volume(out, CPU, never, all_queries=None)
    with pytest.raises(ValueError, match="labels"):                   # every row at the capacity of the first
        A.sparse_volume((i32(9, 3), i32(8, 512), None, cnt), CPU, never, scores_required=False)
    rec = i32(40, 18)
    out = (i32(9, 3), i32(9, 512), None, i32(9, 512), cnt, rec, torch.empty(1, dtype=torch.int64))
    vol, cap, _ = A.sparse_volume(out, CPU, never, scores_required=False, record_words=18)
    assert cap == 9 and vol[5] is rec                                  # the table has a capacity of its own
    vol, _, _ = A.sparse_volume(out[:5] + (None,) + out[6:], CPU, never, scores_required=False, record_words=18)
    assert vol[5] is None
    with pytest.raises(ValueError, match="components"):
        A.sparse_volume(out[:5] + (i32(40, 17),) + out[6:], CPU, never, scores_required=False, record_words=18)
    with pytest.raises(ValueError, match="count"):
        A.sparse_volume(out[:6] + (torch.empty(2, dtype=torch.int64),), CPU, never, scores_required=False, record_words=18)


# ------------------------------------------------------------------------------------------------ ptr, result_buffer, struct_options, subsampling
def test_ptr_null_for_none_and_empty():
    assert A.ptr(None) is None
    assert A.ptr(torch.empty((0, 3), dtype=torch.float32)) is None
    assert A.ptr(torch.empty(8, dtype=torch.float32)[3:3]) is None      # an empty view of memory that exists
    t = torch.zeros(4, dtype=torch.float32)
    p = A.ptr(t)
    assert isinstance(p, C.c_void_p) and p.value == t.data_ptr()
    # collapse=False: whatever address torch reports for the empty tensor (recent versions report 0 themselves)
    assert A.ptr(t[3:3], collapse=False).value == C.c_void_p(t[3:3].data_ptr()).value and A.ptr(None, collapse=False) is None


def test_result_buffer():
    b = A.result_buffer(None, 64, CPU)
    assert b.dtype == torch.uint8 and b.numel() == 64 and b.data_ptr() % 8 == 0
    assert A.result_buffer(b, 64, CPU) is b
    with pytest.raises(ValueError, match="64 bytes"):
        A.result_buffer(torch.empty(63, dtype=torch.uint8), 64, CPU)
    big = torch.empty(72, dtype=torch.uint8)
    assert big.data_ptr() % 8 == 0
    with pytest.raises(ValueError, match="8-byte aligned"):
        A.result_buffer(big[1:65], 64, CPU)                            # right size, misaligned
    with pytest.raises(ValueError):
        A.result_buffer(big[1:], 64, CPU)                              # misaligned and too long
    with pytest.raises(ValueError):
        A.result_buffer(torch.empty(64, dtype=torch.int8), 64, CPU)
    with pytest.raises(ValueError):
        A.result_buffer(torch.empty(128, dtype=torch.uint8)[::2], 64, CPU)


class _Opts(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("iterations", C.c_int32), ("merge_color", C.c_int32), ("pad", C.c_int32)]


def _defaults(ref):
    o = ref._obj
    o.min_weight = 0.5; o.iterations = 10; o.merge_color = 1; o.pad = 0


def test_struct_options():
    o = A.struct_options(_Opts, _defaults, {}, "test")
    assert (o.min_weight, o.iterations, o.merge_color) == (0.5, 10, 1)
    o = A.struct_options(_Opts, _defaults, {"iterations": 3, "merge_color": []}, "test")
    assert (o.min_weight, o.iterations, o.merge_color) == (0.5, 3, 0)
    assert A.struct_options(_Opts, _defaults, {"merge_color": 7}, "test").merge_color == 1      # a flag: int(bool(v))
    with pytest.raises(TypeError, match="unknown test option 'iteration'"):
        A.struct_options(_Opts, _defaults, {"iteration": 3}, "test")
    with pytest.raises(TypeError):
        A.struct_options(_Opts, _defaults, {"pad": 1}, "test")          # padding is no option


def test_subsampling_arg():
    assert A.subsampling_arg(None) == 0 and A.subsampling_arg(1) == 1 and A.subsampling_arg(4) == 4
    for bad in (0, -1):
        with pytest.raises(ValueError, match="subsampling must be >= 1"):
            A.subsampling_arg(bad)
