"""Host-side mirror of nvblox::Mapper / MultiMapper / EsdfSlicer for tests and bench.py (thin ctypes over the C-ABI).

Method names follow the reference call sites (nvblox_ros/src/lib/nvblox_node.cpp:781,1062,1264;
layer_publishing.cpp:686-689).  Images are torch CUDA tensors (device memory, like the reference's
MemoryType::kDevice images) or numpy arrays (uploaded first).
"""
import collections
import ctypes as C
import os
import numpy as np

from . import _args, _lib
from ._args import F16, F32, FLAG, I32, I64, U8, np_ptr as _np_ptr, ptr
from ._lib import BoundingShape, Camera, Counters, Index3D, Lidar, Params

LAYER_TSDF, LAYER_COLOR, LAYER_ESDF, LAYER_MESH, LAYER_OCCUPANCY, LAYER_FREESPACE = 1, 2, 4, 8, 16, 32
LAYER_FEATURE = 64

# nvbx_component (label_components / segment_features): the fields of a record table as tensors that view it, one row per component; centroid_m is
# derived -- (sum_xyz / voxels + 0.5) voxel_size, float64 metres.  A record is COMPONENT_WORDS int32 words (72 bytes).
Components = collections.namedtuple("Components", "label voxels min_xyz max_xyz sum_xyz peak_score peak_xyz centroid_m")
COMPONENT_WORDS = C.sizeof(_lib.Component) // 4

# nvbx_align_result.status (align_points / align_depth / linearize_points)
ALIGN_CONVERGED, ALIGN_MAX_ITERATIONS, ALIGN_TOO_FEW, ALIGN_DEGENERATE, ALIGN_LINEARIZED = 1, 2, 3, 4, 5
ALIGN_STATUS_NAMES = {1: "CONVERGED", 2: "MAX_ITERATIONS", 3: "TOO_FEW", 4: "DEGENERATE", 5: "LINEARIZED"}
ALIGN_RESULT_BYTES = C.sizeof(_lib.AlignResult)

# nvbx_relocalize_result.status (relocalize_points / relocalize_depth); one pose's record of score_poses
RELOC_OK, RELOC_NO_CANDIDATE = 0, 1
RELOC_STATUS_NAMES = {0: "OK", 1: "NO_CANDIDATE"}
RELOC_RESULT_BYTES = C.sizeof(_lib.RelocalizeResult)
PoseScore = collections.namedtuple("PoseScore", "points valid inliers conflicts abs_residual_q20")

# nvbx_merge_result.status (merge_from)
MERGE_OK, MERGE_EMPTY_SOURCE, MERGE_NO_OVERLAP = 0, 1, 2
MERGE_STATUS_NAMES = {0: "OK", 1: "EMPTY_SOURCE", 2: "NO_OVERLAP"}
MERGE_RESULT_BYTES = C.sizeof(_lib.MergeResult)
FEATURE_MERGE_RESULT_BYTES = C.sizeof(_lib.FeatureMergeResult)      # (merge_features_from; its status values are the merge's)
# nvbx_change_result.status (find_changes / change_clusters); the labels of their volume; nvbx_change_options.sampling
CHANGE_OK, CHANGE_EMPTY_MAP, CHANGE_EMPTY_REFERENCE, CHANGE_NO_OVERLAP = 0, 1, 2, 3
CHANGE_STATUS_NAMES = {0: "OK", 1: "EMPTY_MAP", 2: "EMPTY_REFERENCE", 3: "NO_OVERLAP"}
CHANGE_RESULT_BYTES = C.sizeof(_lib.ChangeResult)
CHANGE_APPEARED, CHANGE_REMOVED = 0, 1
CHANGE_SAMPLING = {"trilinear": 0, "nearest": 1}
COST_UNREACHED = 0x7fffffff     # NVBX_COST_UNREACHED: cost_field's value where no move sequence leads
ELEV_UNKNOWN, ELEV_SURFACE, ELEV_BLOCKED, ELEV_VOID = 0, 1, 2, 3      # NVBX_ELEV_*: elevation_map's status
TERRAIN_UNKNOWN, TERRAIN_OK, TERRAIN_HAZARD = 0, 1, 2                 # NVBX_TERRAIN_*: traversability's class

TSDF_DT = np.dtype([("distance", "<f4"), ("weight", "<f4")])
COLOR_DT = np.dtype([("r", "u1"), ("g", "u1"), ("b", "u1"), ("pad", "u1"), ("weight", "<f4")])
ESDF_DT = np.dtype([("squared_distance_vox", "<f4"), ("parent_direction", "<i4", (3,)),
                    ("is_inside", "u1"), ("observed", "u1"), ("is_site", "u1"), ("pad", "u1")])
OCCUPANCY_DT = np.dtype([("log_odds", "<f4")])
FREESPACE_DT = np.dtype([("last_occupied_timestamp_ms", "<i8"), ("consecutive_occupancy_duration_ms", "<i8"),
                         ("is_high_confidence_freespace", "u1"), ("initialized", "u1"), ("pad", "u1", (6,))])
_DT = {LAYER_TSDF: TSDF_DT, LAYER_COLOR: COLOR_DT, LAYER_ESDF: ESDF_DT, LAYER_OCCUPANCY: OCCUPANCY_DT, LAYER_FREESPACE: FREESPACE_DT}


def default_params(**kw):
    """fuser.yaml values (nvblox_examples_bringup/config/nvblox/fuser.yaml:24-42) + nvblox_base.yaml:87,103-107."""
    p = Params(
        voxel_size=0.05, max_integration_distance_m=8.0, truncation_distance_vox=4.0, max_weight=5.0,
        weighting_mode=0, raycast_subsampling_factor=4,
        esdf_min_weight=0.1, esdf_max_site_distance_vox=2.0, esdf_max_distance_m=2.0,
        esdf_slice_height=0.09, esdf_slice_min_height=0.09, esdf_slice_max_height=0.65,
        mesh_min_weight=0.1, mesh_weld_vertices=1,
        sphere_tracing_subsampling=4, sphere_tracing_max_steps=100,
        sphere_tracing_max_ray_length_m=15.0, sphere_tracing_surface_eps_vox=0.1,
        tsdf_decay_factor=0.95, tsdf_decayed_weight_threshold=0.001,
        esdf_site_rule=0, depth_interp_nearest=0,
        lidar_max_integration_distance_m=10.0,
        lidar_linear_interpolation_max_allowable_difference_vox=2.0,
        lidar_nearest_interpolation_max_allowable_dist_to_ray_vox=0.5, invalid_depth_decay_factor=-1.0,
        projective_layer_type=0, free_region_occupancy_probability=0.45, occupied_region_occupancy_probability=0.55,
        unobserved_region_occupancy_probability=0.5, occupied_region_half_width_m=0.1,
        free_region_decay_probability=0.55, occupied_region_decay_probability=0.30, esdf_mode=0,
        max_tsdf_distance_for_occupancy_m=0.15, max_unobserved_to_keep_consecutive_occupancy_ms=200,
        min_duration_since_occupied_for_freespace_ms=1000, min_consecutive_occupancy_duration_for_reset_ms=2000,
        check_neighborhood=1, initialize_to_high_confidence_freespace=0,
        tsdf_weighting_variant=0, tsdf_skip_at_negative_truncation=0, tsdf_weight_clamp_before_blend=0,
        color_occlusion_threshold_vox=-1.0, esdf_propagation=0, mesh_ambiguity_rule=0, mesh_normal_rule=0,
        decay_deallocate_decayed_blocks=1, tsdf_set_free_distance_on_decayed=0, tsdf_decayed_free_distance_vox=4.0, occupancy_decay_to_free=0)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class NvbxError(RuntimeError):
    pass


# NVBX_CHECK_ON_CLOSE=1 with the -DNVBX_CHECK_INVARIANTS variant of the library: what the mappers closed so far reported (tests/test_gpu_invariants.py)
INVARIANT_REPORT = {"mappers_checked": 0, "violations": []}


def frame_pool_stats():
    """(held, free, bytes, created, waits, syncs) of the library's frame pool (nvbx_frame_pool_stats)."""
    out = (C.c_int64 * 6)()
    _lib.load().nvbx_frame_pool_stats(out)
    return tuple(int(v) for v in out)


class ColorFrame:
    """A colour image in a library-owned, reference-counted device frame (nvbx_frame_acquire, include/nvblox_hip.h): what nvblox::Image<Color>
    device memory is in the C++ facade.  A mapper that holds integrate_color back RETAINS the frame instead of copying the image; `write` first makes
    sure nobody else holds the frame and continues in another one if a mapper does (rotation) -- the node's one re-used colour buffer
    (nvblox_node.hpp:484-488) without the staging copy."""

    def __init__(self, rows, cols, channels=3, device=0):
        self.lib = _lib.load()
        self.rows, self.cols, self.channels, self.device = int(rows), int(cols), int(channels), int(device)
        self.nbytes = self.rows * self.cols * self.channels
        self._p = C.c_void_p()
        self._acquire(_lib.STREAM_UNKNOWN)

    def _acquire(self, stream):
        p = C.c_void_p()
        if self.lib.nvbx_frame_acquire(self.device, self.nbytes, stream, C.byref(p)) != 0:
            raise NvbxError("nvbx_frame_acquire: %s" % self.lib.nvbx_last_error().decode())
        self._p = p

    @property
    def ptr(self):
        return self._p.value

    def shared(self):
        return self.lib.nvbx_frame_refcount(self._p) > 1

    def write(self, src, stream=None):
        """Overwrite the image from a torch CUDA tensor / numpy array of rows x cols x channels uint8: asynchronously on `stream` (a raw hipStream_t),
        or with a blocking copy (stream=None: a writer the library knows nothing about).  Continues in another frame first when a mapper still holds
        this one, or its launches may still be reading it."""
        s = C.c_void_p(stream) if stream else _lib.STREAM_UNKNOWN
        if self.lib.nvbx_frame_writable(self._p, s) == 0:      # a mapper holds it, or its launches may still be reading it (and not on this stream)
            old = self._p
            self._acquire(s)
            self.lib.nvbx_frame_release(old)
        if hasattr(src, "data_ptr"):
            assert src.is_contiguous() and src.numel() * src.element_size() == self.nbytes
            sp = ptr(src)
        else:
            a = np.ascontiguousarray(src, np.uint8); assert a.nbytes == self.nbytes
            self._host_keep = a; sp = _np_ptr(a)
        if self.lib.nvbx_frame_upload(self._p, sp, self.nbytes, s) != 0:
            raise NvbxError("nvbx_frame_upload: %s" % self.lib.nvbx_last_error().decode())
        return self

    def close(self):
        if getattr(self, "_p", None) is not None and self._p.value:
            self.lib.nvbx_frame_release(self._p); self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AlignResult:
    """What an alignment call left behind: `buffer` is the nvbx_align_result record on the device (a uint8 tensor, written by the launches);
    the first field that is read copies it to the host once (torch's current stream is ordered behind the launches by then)."""

    def __init__(self, buffer):
        self.buffer = buffer
        self._host = None

    def _r(self):
        if self._host is None:
            self._host = _lib.AlignResult.from_buffer_copy(self.buffer.cpu().numpy().tobytes())
        return self._host

    @staticmethod
    def _full(tri):
        H = np.zeros((6, 6)); H[np.triu_indices(6)] = np.array(tri, np.float64)
        return H + np.triu(H, 1).T

    @staticmethod
    def _rmse(sums):
        return float(np.sqrt(sums.cost / sums.n_valid)) if sums.n_valid > 0 else 0.0

    T_L_S = property(lambda self: np.array(self._r().T_L_S, np.float32).reshape(4, 4), doc="the refined pose, f32")
    T64 = property(lambda self: np.array(self._r().T64, np.float64).reshape(4, 4), doc="the refined pose, f64")
    step = property(lambda self: np.array(self._r().step, np.float64), doc="the last step solved for, (v, omega)")
    iterations = property(lambda self: int(self._r().iterations))
    status = property(lambda self: int(self._r().status))
    status_name = property(lambda self: ALIGN_STATUS_NAMES.get(int(self._r().status), "?"))
    n_valid = property(lambda self: int(self._r().last.n_valid), doc="valid points of the last linearization")
    n_valid_first = property(lambda self: int(self._r().first.n_valid))
    cost_first = property(lambda self: float(self._r().first.cost))
    cost_last = property(lambda self: float(self._r().last.cost))
    rmse_first = property(lambda self: self._rmse(self._r().first), doc="sqrt(cost / n_valid) at the guess")
    rmse_last = property(lambda self: self._rmse(self._r().last), doc="... at the last linearization")
    H = property(lambda self: self._full(self._r().last.H), doc="6 x 6 normal matrix of the last linearization")
    b = property(lambda self: np.array(self._r().last.b, np.float64))
    H_first = property(lambda self: self._full(self._r().first.H))
    b_first = property(lambda self: np.array(self._r().first.b, np.float64))

    def __repr__(self):
        return "AlignResult(%s, iterations=%d, n_valid=%d, rmse %.4g -> %.4g)" % (self.status_name, self.iterations, self.n_valid, self.rmse_first, self.rmse_last)


ALIGN_COLOR_RESULT_BYTES = ALIGN_RESULT_BYTES + C.sizeof(_lib.AlignColorResult)


class AlignColorResult(AlignResult):
    """What an alignment with a colour term left behind: `buffer` holds the nvbx_align_result record (the AlignResult view: `buffer[:712]` is
    byte for byte what the plain call writes) and the nvbx_align_color_result record behind it; ALIGN_COLOR_RESULT_BYTES bytes."""

    def _c(self):
        self._r()
        return self._color

    def _r(self):
        if self._host is None:
            raw = self.buffer.cpu().numpy().tobytes()
            self._host = _lib.AlignResult.from_buffer_copy(raw[:ALIGN_RESULT_BYTES])
            self._color = _lib.AlignColorResult.from_buffer_copy(raw[ALIGN_RESULT_BYTES:])
        return self._host

    @staticmethod
    def _crmse(cost, n):
        return float(np.sqrt(cost / n)) if n > 0 else 0.0

    n_color = property(lambda self: int(self._c().n_color_last), doc="points with a colour term in the last linearization")
    n_color_first = property(lambda self: int(self._c().n_color_first))
    color_cost_first = property(lambda self: float(self._c().color_cost_first))
    color_cost_last = property(lambda self: float(self._c().color_cost_last))
    color_rmse_first = property(lambda self: self._crmse(self._c().color_cost_first, self._c().n_color_first), doc="sqrt(color_cost / n_color) at the guess, in levels")
    color_rmse_last = property(lambda self: self._crmse(self._c().color_cost_last, self._c().n_color_last), doc="... at the last linearization")

    def __repr__(self):
        return "AlignColorResult(%s, iterations=%d, n_valid=%d, n_color=%d, rmse %.4g -> %.4g m, colour %.4g -> %.4g levels)" % (
            self.status_name, self.iterations, self.n_valid, self.n_color, self.rmse_first, self.rmse_last, self.color_rmse_first, self.color_rmse_last)


class RelocalizeResult:
    """What relocalize_points / relocalize_depth left behind: `buffer` is the nvbx_relocalize_result record on the device (a uint8 tensor, written
    by the launches); the first field that is read copies it to the host once.  `align` is an AlignResult over the record's alignment part,
    `scores` the lattice's records (counts int32 [K, 4], abs_residual_q20 int64 [K]; device tensors) where the call was asked for them."""

    def __init__(self, buffer, scores=None):
        self.buffer = buffer
        self.scores = scores
        self.align = AlignResult(buffer[_lib.RelocalizeResult.align.offset:])
        self._host = None

    def _r(self):
        if self._host is None:
            self._host = _lib.RelocalizeResult.from_buffer_copy(self.buffer.cpu().numpy().tobytes())
        return self._host

    @staticmethod
    def _score(s):
        return PoseScore(int(s.points), int(s.valid), int(s.inliers), int(s.conflicts), int(s.abs_residual_q20))

    status = property(lambda self: int(self._r().status))
    status_name = property(lambda self: RELOC_STATUS_NAMES.get(int(self._r().status), "?"))
    best_index = property(lambda self: int(self._r().best_index), doc="h of the selected hypothesis")
    coarse = property(lambda self: self._score(self._r().coarse), doc="its record")
    T_coarse = property(lambda self: np.array(self._r().T_coarse, np.float32).reshape(4, 4), doc="its pose")
    refined = property(lambda self: self._score(self._r().refined), doc="the record of align.T_L_S")
    T_L_S = property(lambda self: self.align.T_L_S, doc="the refined pose, f32 (T_coarse's refinement; meaningless with NO_CANDIDATE)")

    def __repr__(self):
        return "RelocalizeResult(%s, hypothesis %d: %d inliers, %d conflicts -> %s, %d inliers)" % (
            self.status_name, self.best_index, self.coarse.inliers, self.coarse.conflicts, self.align.status_name, self.refined.inliers)


class MergeResult:
    """What merge_from left behind: `buffer` is the nvbx_merge_result record on the device (a uint8 tensor, written by the call's last launch);
    the first field that is read copies it to the host once."""

    def __init__(self, buffer):
        self.buffer = buffer
        self._host = None

    def _r(self):
        if self._host is None:
            self._host = _lib.MergeResult.from_buffer_copy(self.buffer.cpu().numpy().tobytes())
        return self._host

    source_blocks = property(lambda self: int(self._r().source_blocks), doc="TSDF blocks of the source")
    candidate_blocks = property(lambda self: int(self._r().candidate_blocks), doc="blocks of this map the merge went over")
    blocks_allocated = property(lambda self: int(self._r().blocks_allocated), doc="... of which it did not have before")
    voxels_fused = property(lambda self: int(self._r().voxels_fused))
    color_voxels_fused = property(lambda self: int(self._r().color_voxels_fused))
    status = property(lambda self: int(self._r().status))
    status_name = property(lambda self: MERGE_STATUS_NAMES.get(int(self._r().status), "?"))

    def __repr__(self):
        return "MergeResult(%s, %d source blocks -> %d candidates (%d new), %d voxels, %d colour voxels)" % (
            self.status_name, self.source_blocks, self.candidate_blocks, self.blocks_allocated, self.voxels_fused, self.color_voxels_fused)


class FeatureMergeResult:
    """What merge_features_from left behind: `buffer` is the nvbx_feature_merge_result record on the device (a uint8 tensor, written by the
    call's last launch); the first field that is read copies it to the host once."""

    def __init__(self, buffer):
        self.buffer = buffer
        self._host = None

    def _r(self):
        if self._host is None:
            self._host = _lib.FeatureMergeResult.from_buffer_copy(self.buffer.cpu().numpy().tobytes())
        return self._host

    source_blocks = property(lambda self: int(self._r().source_blocks), doc="feature blocks of the source")
    candidate_blocks = property(lambda self: int(self._r().candidate_blocks), doc="distinct blocks of this map the call went over")
    blocks_flagged = property(lambda self: int(self._r().blocks_flagged), doc="... of which it gave the feature layer")
    voxels_fused = property(lambda self: int(self._r().voxels_fused))
    status = property(lambda self: int(self._r().status))
    status_name = property(lambda self: MERGE_STATUS_NAMES.get(int(self._r().status), "?"))

    def __repr__(self):
        return "FeatureMergeResult(%s, %d source blocks -> %d candidates (%d flagged), %d voxels)" % (
            self.status_name, self.source_blocks, self.candidate_blocks, self.blocks_flagged, self.voxels_fused)


class ChangeResult:
    """What find_changes / change_clusters left behind: `buffer` is the nvbx_change_result record on the device (a uint8 tensor, written by the
    scan's last launch); the first field that is read copies it to the host once."""

    def __init__(self, buffer):
        self.buffer = buffer
        self._host = None

    def _r(self):
        if self._host is None:
            self._host = _lib.ChangeResult.from_buffer_copy(self.buffer.cpu().numpy().tobytes())
        return self._host

    blocks_scanned = property(lambda self: int(self._r().blocks_scanned), doc="TSDF blocks of this map")
    voxels_compared = property(lambda self: int(self._r().voxels_compared), doc="in the box, observed here, with a valid sample of the reference")
    voxels_appeared = property(lambda self: int(self._r().voxels_appeared))
    voxels_removed = property(lambda self: int(self._r().voxels_removed))
    blocks_changed = property(lambda self: int(self._r().blocks_changed), doc="blocks with a labelled voxel")
    status = property(lambda self: int(self._r().status))
    status_name = property(lambda self: CHANGE_STATUS_NAMES.get(int(self._r().status), "?"))

    def __repr__(self):
        return "ChangeResult(%s, %d blocks scanned, %d voxels compared: %d appeared, %d removed in %d blocks)" % (
            self.status_name, self.blocks_scanned, self.voxels_compared, self.voxels_appeared, self.voxels_removed, self.blocks_changed)


class Mapper:
    def __init__(self, params=None, device=0, block_capacity=1 << 15, stream=None, max_block_capacity=None):
        import torch
        if not torch.cuda.is_available():
            raise NvbxError("no HIP device visible: the product path has no CPU fallback")
        self._torch = torch
        self.lib = _lib.load()
        self.params = params or default_params()
        self.device = device
        self._h = C.c_void_p()
        torch.cuda.set_device(device)
        s = C.c_void_p(stream) if stream else None
        self._check(self.lib.nvbx_mapper_create(device, s, C.byref(self.params), block_capacity, C.byref(self._h)))
        self._capacity0 = block_capacity
        self._stream0 = stream          # (coarsened() creates its mapper with the same stream setting)
        self._keep = []
        if max_block_capacity is not None:
            self.set_max_capacity(max_block_capacity)

    @property
    def capacity(self):
        """Current block capacity of the HBM pools (they double on demand up to max_block_capacity)."""
        return int(self.lib.nvbx_mapper_capacity(self._h))

    def set_max_capacity(self, max_blocks):
        self._check(self.lib.nvbx_mapper_set_max_capacity(self._h, int(max_blocks)))

    def set_color_deferral(self, enable, staged=True):
        """Hold integrateColor (and an updateEsdf behind it) back until the next integrateDepth carries them out in pipelined order (two
        launches per frame instead of four; include/nvblox_hip.h nvbx_mapper_set_color_deferral).  A NEW mapper does so in the staged form
        (enable=True, staged=True: the mapper copies a held-back frame into its own memory first, nothing observable changes but the time).
        staged=False (opt-in, zero-copy): the colour image handed to integrate_color must then stay valid and unchanged until the next call into
        the mapper has returned.  enable=False: the classic order, every call launches its own kernels.
        (staged=True is the default here as in C and C++ -- ADVICE r04.)  An image in a ColorFrame is never copied, in either form."""
        self._check(self.lib.nvbx_mapper_set_color_deferral(self._h, (2 if staged else 1) if enable else 0))

    def reload_knobs(self):
        """Read the library's NVBX_* environment variables again for this mapper (they are read at creation and kept per mapper).
        Held-back work is carried out first, under the old settings.  NVBX_MAX_BLOCKS, NVBX_COLOR_DEFERRAL and NVBX_DEFER_EDT
        apply at creation only."""
        self._check(self.lib.nvbx_mapper_reload_knobs(self._h))

    # -- ground plane (MultiMapper::ground_plane_estimator())
    def tsdf_zero_crossings(self, min_z_m, max_z_m):
        """xyz [N, 3] float32 of the TSDF's upward zero crossings with height in [min_z_m, max_z_m], sorted by (x, y, z)."""
        n = self._check(self.lib.nvbx_tsdf_zero_crossings(self._h, float(min_z_m), float(max_z_m), None, 0))
        out = np.zeros((max(n, 1), 3), np.float32)
        n2 = self._check(self.lib.nvbx_tsdf_zero_crossings(self._h, float(min_z_m), float(max_z_m), _np_ptr(out), out.shape[0]))
        return out[:min(n, n2)]

    def fit_plane_ransac(self, points, distance_threshold_m, iterations, seed=1):
        """-> (plane [nx, ny, nz, d] float32, inliers); host only"""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3); plane = np.zeros(4, np.float32)
        n = self._check(self.lib.nvbx_fit_plane_ransac(_np_ptr(p), len(p), float(distance_threshold_m), int(iterations), int(seed), _np_ptr(plane)))
        return plane, n

    def _check(self, rc):
        if rc < 0:
            raise NvbxError("nvbx error %d: %s" % (rc, self.lib.nvbx_last_error().decode()))
        return rc

    def invariant_violations(self, selftest=False):
        """-DNVBX_CHECK_INVARIANTS variant of the library only (NVBX_LIB=...; tools/build_variant.sh inv): (I1, I3, I4, writers still running, I8) as
        the kernels and the host counted them; None with the product library, which compiles the checks to nothing."""
        try:
            fn = self.lib.nvbx_debug_invariants
        except AttributeError:
            return None
        fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        out = (C.c_int64 * 5)()
        self._check(fn(self._h, out, int(bool(selftest))))
        return tuple(int(v) for v in out)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            if os.environ.get("NVBX_CHECK_ON_CLOSE") == "1":        # (tests/test_gpu_invariants.py: every mapper of a test run answers for its launches)
                v = self.invariant_violations()
                if v is not None:
                    INVARIANT_REPORT["mappers_checked"] += 1
                    if any(v):          # (recorded as well as raised: most mappers are closed by __del__, which swallows exceptions)
                        INVARIANT_REPORT["violations"].append(v)
                        self.lib.nvbx_mapper_destroy(self._h); self._h = C.c_void_p()
                        raise NvbxError("invariant violations (I1, I3, I4, writers running, I8) = %r" % (v,))
            self.lib.nvbx_mapper_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers
    def _hold(self, slot, tensors):
        """Keep the device images of the call that has just been enqueued alive (`slot`: "_keep" depth / range images, "_keep_c" colour) and let go
        of the previous call's.  The kernels that read them run on the MAPPER's stream, which torch's caching allocator knows nothing about: a
        block it takes back could be handed out again and overwritten by the next upload (on torch's current stream) while kernels queued behind
        a slow launch -- a first launch loads its code object, ~0.5 ms -- still read it (found as garbage view rays in tests/test_gpu_pipeline.py).
        So before the old images are dropped, torch's current stream is made to wait for everything queued on the mapper's stream so far."""
        old = getattr(self, slot, None)
        if old:
            torch = self._torch
            cur = torch.cuda.current_stream(self.device); ms = self.torch_stream()
            if ms.cuda_stream != cur.cuda_stream:
                cur.wait_stream(ms)
        setattr(self, slot, tensors)

    # -- Argument coercion and output buffers live in _args.py, for every call: a call adds no coercion code of its own and hands tensors to the
    #    library through `ptr`; a reader call declares its outputs as a spec of (name, shape, dtypes, required, wanted) rows ("Host language")
    @property
    def _cuda(self):
        return self._torch.device("cuda", self.device)

    def _dev(self, a, dtype):
        return _args.image(a, self._cuda, dtype)

    _T = staticmethod(_args.pose)
    _cam = staticmethod(_args.camera)
    _lidar = staticmethod(_args.lidar)

    def _image(self, a, what="depth", dtype=None):      # a (rows, cols) image: float32 (depth, range) unless dtype says otherwise (uint8: a mask)
        return _args.image(a, self._cuda, dtype or self._torch.float32, what, "(rows, cols)")

    def _frame(self, fn, img, T, model):
        """-> the prepared call of an image with its pose and intrinsics: (fn, pointer, rows, cols, pose pointer, byref(model), keep), keep[0] = img"""
        group, keep = _args.frame(img, T, model)
        return (fn,) + group + (keep,)

    def _run(self, a, slot):      # a prepared call, now; its device image is kept alive in `slot` until the next call (stream-ordered use)
        self._check(a[0](self._h, *a[1:6]))
        if slot:
            self._hold(slot, [a[6][0]])

    def set_params(self, params):
        self._check(self.lib.nvbx_mapper_set_params(self._h, C.byref(params)))
        self.params = params

    def synchronize(self):
        self._check(self.lib.nvbx_synchronize(self._h))

    def wait_for(self, producer):
        """This mapper's stream waits for everything enqueued so far on `producer`'s stream (two mappers on two streams; nvbx_mapper_wait_for)."""
        self._check(self.lib.nvbx_mapper_wait_for(self._h, producer._h))

    def stream_handle(self):
        """The raw hipStream_t of the mapper (int)."""
        h = C.c_void_p()
        self._check(self.lib.nvbx_get_stream(self._h, C.byref(h)))
        return h.value or 0

    def torch_stream(self):
        """The mapper's stream as a torch stream object (for event ordering against work on torch's streams)."""
        if getattr(self, "_tstream", None) is None:
            self._tstream = self._torch.cuda.ExternalStream(self.stream_handle(), device="cuda:%d" % self.device)
        return self._tstream

    def flush(self):
        """Enqueue held-back work (the EDT of the last update_esdf) without waiting."""
        self._check(self.lib.nvbx_flush(self._h))

    def clear(self):
        self._check(self.lib.nvbx_mapper_clear(self._h))

    # -- integration (async)
    def integrate_depth(self, depth, T_L_C, cam):
        """depth [rows, cols]: float32 metres, or u16 millimetres (a numpy uint16 array / a torch.int16 tensor holding those bits)"""
        self._run(self.prepare_depth(depth, T_L_C, cam), "_keep")

    def integrate_lidar_depth(self, range_image, T_L_C, lidar):
        """range image [elevation divisions, azimuth divisions] f32 metres; lidar = (cols, rows, min_range, min_el, max_el)."""
        self._run(self.prepare_lidar(range_image, T_L_C, lidar), "_keep")

    def prepare_lidar(self, range_image, T_L_C, lidar):
        return self._frame(self.lib.nvbx_integrate_lidar_depth, self._image(range_image, "range_image"), T_L_C, _args.lidar(lidar))

    def motion_compensate_pointcloud(self, points, rel_time_ms, T_L_S_start, T_L_S_end, scan_duration_ms):
        """LiDAR motion compensation: points [n, 3] measured at rel_time_ms [n] within the scan -> sensor frame at scan start (device tensor)."""
        p = _args.points3(points, self._cuda); t = _args.image(rel_time_ms, self._cuda, self._torch.float32, "rel_time_ms")
        out = self._torch.empty_like(p)
        self._check(self.lib.nvbx_motion_compensate_pointcloud(self._h, ptr(p), ptr(t), p.shape[0], _np_ptr(self._T(T_L_S_start)),
                                                               _np_ptr(self._T(T_L_S_end)), float(scan_duration_ms), ptr(out)))
        self.synchronize()
        return out

    def depth_image_from_pointcloud(self, points, lidar):
        p = _args.points3(points, self._cuda); k = _args.lidar(lidar)
        img = self._torch.zeros((k.num_elevation_divisions, k.num_azimuth_divisions), dtype=self._torch.float32, device=p.device)
        # (a non-collapsing pointer: the entry takes an empty cloud, but not a NULL one)
        self._check(self.lib.nvbx_depth_image_from_pointcloud(self._h, ptr(p, collapse=False), p.shape[0], C.byref(k), ptr(img)))
        self.synchronize()
        return img

    def integrate_color(self, rgb, T_L_C, cam):
        """rgb8 [rows, cols, 3] or bgra8 [rows, cols, 4] (the two encodings image_conversions.cpp:170-176 accepts)."""
        self._run(self._color(rgb, T_L_C, cam, (3, 4)), None if isinstance(rgb, ColorFrame) else "_keep_c")

    # -- pre-marshalled calls: the reference hands ready C++ objects to integrateDepth/Color; this keeps Python's per-call
    #    argument marshalling (tensor checks, numpy pose copy, struct construction) out of a measured loop
    def prepare_depth(self, depth, T_L_C, cam):
        d, kind = _args.depth_image(depth, self._cuda)
        return self._frame(self.lib.nvbx_integrate_depth_u16mm if kind == "u16mm" else self.lib.nvbx_integrate_depth, d, T_L_C, _args.camera(cam))

    def _color(self, rgb, T_L_C, cam, channels):
        """the prepared call of a colour image (a ColorFrame, or what `image` takes) with one of `channels` channels: 4 = bgra8"""
        if not isinstance(rgb, ColorFrame):
            rgb = _args.image(rgb, self._cuda, self._torch.uint8, "rgb", "(rows, cols, %s)" % " or ".join(map(str, channels)), channels)
        elif rgb.channels not in channels:
            raise ValueError("the ColorFrame has %d channels, not one of %s" % (rgb.channels, channels))
        ch = rgb.channels if isinstance(rgb, ColorFrame) else rgb.shape[2]
        return self._frame(self.lib.nvbx_integrate_color_bgra8 if ch == 4 else self.lib.nvbx_integrate_color, rgb, T_L_C, _args.camera(cam))

    def prepare_color(self, rgb, T_L_C, cam):
        return self._color(rgb, T_L_C, cam, (3,))

    # -- camera batches (nvbx_integrate_depth_batch / _color_batch): n frames of one image size in ONE launch set
    def _batch(self, fn, imgs, coerce, poses, cams):
        n = len(imgs)
        d = [i if isinstance(i, ColorFrame) else coerce(i) for i in imgs]
        ptrs = (C.c_void_p * n)(*[t.ptr if isinstance(t, ColorFrame) else t.data_ptr() for t in d])      # (raw addresses: the elements of an array)
        T = _args.pose_block(poses)
        if not isinstance(cams, (list, tuple)) or not isinstance(cams[0], (list, tuple, Camera)):
            cams = [cams] * n
        ks = (Camera * n)(*[_args.camera(k) for k in cams])
        rows, cols = (d[0].rows, d[0].cols) if isinstance(d[0], ColorFrame) else d[0].shape[:2]
        return (fn, n, ptrs, rows, cols, _np_ptr(T), ks, (d, T))

    def prepare_depth_batch(self, depths, poses, cams):
        return self._batch(self.lib.nvbx_integrate_depth_batch, depths, self._image, poses, cams)

    def prepare_color_batch(self, rgbs, poses, cams):
        # (nvbx_integrate_color_batch takes rgb8 only: a bgra8 frame would be decoded as rgb8)
        if any(isinstance(i, ColorFrame) and i.channels != 3 for i in rgbs):
            raise ValueError("integrate_color_batch: rgb8 frames only (3 channels)")
        rgb8 = lambda i: _args.image(i, self._cuda, self._torch.uint8, "rgb", "(rows, cols, 3)", (3,))      # noqa: E731
        return self._batch(self.lib.nvbx_integrate_color_batch, rgbs, rgb8, poses, cams)

    def integrate_prepared_batch(self, a):
        rc = a[0](self._h, a[1], a[2], a[3], a[4], a[5], a[6])
        if rc < 0:
            self._check(rc)

    def integrate_depth_batch(self, depths, poses, cams):
        a = self.prepare_depth_batch(depths, poses, cams); self.integrate_prepared_batch(a); self._hold("_keep", [a])

    def integrate_color_batch(self, rgbs, poses, cams):
        a = self.prepare_color_batch(rgbs, poses, cams); self.integrate_prepared_batch(a); self._hold("_keep_c", [a])

    def integrate_depth_pair(self, depth_a, other, depth_b, T_L_C, cam):
        """nvbx_integrate_depth_pair: self.integrate_depth(depth_a) followed by other.integrate_depth(depth_b) -- the background / foreground mappers of a
        MultiMapper's dynamic and human mapping types, fed the two halves of one mask-split depth frame -- in two launches instead of four (both mappers on
        one stream; anything else falls back to the two calls).  Same maps, bit for bit."""
        da = self._image(depth_a, "depth_a"); db = self._image(depth_b, "depth_b")
        if da.shape != db.shape:
            raise ValueError("depth_a %s and depth_b %s differ in shape" % (tuple(da.shape), tuple(db.shape)))
        (pa, rows, cols, T, k), keep = _args.frame(da, T_L_C, _args.camera(cam))
        self._check(self.lib.nvbx_integrate_depth_pair(self._h, pa, other._h, ptr(db), rows, cols, T, k))
        self._hold("_keep", [da, db]); other._hold("_keep", [db])

    def integrate_prepared(self, a):
        rc = a[0](self._h, a[1], a[2], a[3], a[4], a[5])
        if rc < 0:
            self._check(rc)

    def update_esdf(self):
        self._check(self.lib.nvbx_update_esdf(self._h))

    def update_color_mesh(self, full=False):
        self._check(self.lib.nvbx_update_color_mesh(self._h, int(full)))

    update_mesh = update_color_mesh

    def decay_tsdf(self, exclude_last_view=True):
        self._check(self.lib.nvbx_decay_tsdf(self._h, int(exclude_last_view)))

    def set_time_ms(self, t):
        """update_time_ms of the next integrate_depth (freespace layer of a projective_layer_type 2 mapper)."""
        self._check(self.lib.nvbx_set_time_ms(self._h, int(t)))

    def detect_dynamics(self, depth, T_L_C, cam, max_distance_m=0.0):
        """DynamicsDetection::computeDynamics: uint8 device tensor [rows, cols], 1 = the pixel's point lies in high-confidence freespace."""
        d = self._image(depth)
        mask = self._torch.empty(d.shape, dtype=self._torch.uint8, device=d.device)
        self.detect_dynamics_into(d, T_L_C, cam, max_distance_m, mask)
        self.synchronize()
        return mask

    # -- no-sync forms for a stream-ordered caller (outputs pre-allocated on the mapper's device; the caller's tensors must live on
    #    the mapper's stream or be ordered against it)
    def detect_dynamics_into(self, depth_dev, T_L_C, cam, max_distance_m, mask_out):
        group, keep = _args.frame(depth_dev, T_L_C, _args.camera(cam))
        self._check(self.lib.nvbx_detect_dynamics(self._h, *group, float(max_distance_m), ptr(mask_out)))

    def remove_small_components_inplace(self, mask_dev, min_size):
        """(asynchronous on the mapper's stream)"""
        self._check(self.lib.nvbx_remove_small_components(self._h, ptr(mask_dev), mask_dev.shape[0], mask_dev.shape[1], int(min_size)))

    def split_depth_by_mask_into(self, depth_dev, mask_dev, T_CM_CD, depth_cam, mask_cam, occlusion_threshold_m, unmasked_out, masked_out):
        self._split_depth(depth_dev, mask_dev, T_CM_CD, depth_cam, mask_cam, occlusion_threshold_m, unmasked_out, masked_out, None)

    def _split_depth(self, d, mk, T_CM_CD, depth_cam, mask_cam, occlusion_threshold_m, un, ma, ov):
        (pd, rows, cols, T, dc), keep = _args.frame(d, T_CM_CD, _args.camera(depth_cam))
        self._check(self.lib.nvbx_split_depth_by_mask(self._h, pd, rows, cols, ptr(mk), mk.shape[0], mk.shape[1], T, dc, C.byref(_args.camera(mask_cam)),
                                                      float(occlusion_threshold_m), ptr(un), ptr(ma), ptr(ov)))

    def dynamic_depth_split_into(self, depth_dev, T_L_C, cam, max_distance_m, min_component_size, occlusion_threshold_m, mask_out, unmasked_out, masked_out, overlay_out=None):
        """The dynamic-mapping frame's front end in one call (three launches): detect_dynamics -> remove_small_components -> split_depth_by_mask."""
        group, keep = _args.frame(depth_dev, T_L_C, _args.camera(cam))
        self._check(self.lib.nvbx_dynamic_depth_split(self._h, *group, float(max_distance_m), int(min_component_size), float(occlusion_threshold_m),
                                                      ptr(mask_out), ptr(unmasked_out), ptr(masked_out), ptr(overlay_out)))

    def remove_small_components(self, mask, min_size):
        torch = self._torch
        mk = self._image(mask, "mask", torch.uint8).clone()
        torch.cuda.current_stream(mk.device).synchronize()      # the clone ran on torch's stream, the library works on the mapper's
        self.remove_small_components_inplace(mk, min_size)
        self.synchronize()          # (the call is asynchronous on the mapper's stream; the tensor goes back to torch's)
        return mk

    def decay_occupancy(self):
        """Mapper::decayOccupancyAllVoxels (nvblox_node.cpp:925-929); occupancy mappers only."""
        self._check(self.lib.nvbx_decay_occupancy(self._h))

    def clear_outside_radius(self, center, radius):
        c = np.asarray(center, np.float32)
        self._check(self.lib.nvbx_clear_outside_radius(self._h, _np_ptr(c), float(radius)))

    def take_cleared_blocks(self):
        """Mapper::getClearedBlocks (layer_publishing.cpp:716): blocks deallocated by decay / radius clearing since the last call."""
        out = np.zeros((self.capacity, 3), np.int32)
        n = self._check(self.lib.nvbx_take_cleared_blocks(self._h, _np_ptr(out), out.shape[0]))
        return out[:n].copy()

    def clear_tsdf_inside_shapes(self, shapes):
        """shapes: list of ("sphere", centre, radius) / ("aabb", min_corner, max_corner)."""
        arr = (BoundingShape * max(1, len(shapes)))()
        for i, sh in enumerate(shapes):
            if sh[0] == "sphere":
                arr[i].kind = 0; arr[i].a[:] = [float(v) for v in sh[1]]; arr[i].b[:] = [float(sh[2]), 0.0, 0.0]
            else:
                arr[i].kind = 1; arr[i].a[:] = [float(v) for v in sh[1]]; arr[i].b[:] = [float(v) for v in sh[2]]
        self._check(self.lib.nvbx_clear_tsdf_inside_shapes(self._h, C.cast(arr, C.c_void_p), len(shapes)))

    # -- queries (synchronise)
    def counters(self):
        c = Counters()
        self._check(self.lib.nvbx_get_counters(self._h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Counters._fields_}

    def num_blocks(self, layer=LAYER_TSDF):
        return self._check(self.lib.nvbx_num_blocks(self._h, layer))

    def block_indices(self, layer=LAYER_TSDF):
        n = self.num_blocks(layer)
        out = np.zeros((max(n, 1), 3), np.int32)
        n2 = self._check(self.lib.nvbx_block_indices(self._h, layer, _np_ptr(out), out.shape[0]))
        return out[:min(n, n2)]

    def last_view(self):
        out = np.zeros((self.capacity, 3), np.int32)
        n = self._check(self.lib.nvbx_last_depth_view(self._h, _np_ptr(out), out.shape[0]))
        return out[:n].copy()

    def last_color_view(self):
        out = np.zeros((self.capacity, 3), np.int32)
        n = self._check(self.lib.nvbx_last_color_view(self._h, _np_ptr(out), out.shape[0]))
        return out[:n].copy()

    def get_blocks(self, layer, indices):
        idx = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3))
        out = np.zeros((idx.shape[0], 512), _DT[layer])
        found = np.zeros(idx.shape[0], np.int32)
        self._check(self.lib.nvbx_get_blocks(self._h, layer, _np_ptr(idx), idx.shape[0], _np_ptr(out), _np_ptr(found)))
        return out, found.astype(bool)

    def get_block(self, layer, idx):
        out, found = self.get_blocks(layer, [idx])
        return out[0] if found[0] else None

    def set_block(self, layer, idx, data):
        data = np.ascontiguousarray(data, _DT[layer])
        if data.size != 512:
            raise ValueError("data must hold the 512 voxels of a block, got %d" % data.size)
        self._check(self.lib.nvbx_set_block(self._h, layer, Index3D(int(idx[0]), int(idx[1]), int(idx[2])), _np_ptr(data)))

    def set_blocks(self, layer, indices, data):
        idx = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3))
        data = np.ascontiguousarray(data, _DT[layer])
        if data.size != 512 * idx.shape[0]:
            raise ValueError("data must hold 512 voxels for each of the %d blocks, got %d" % (idx.shape[0], data.size))
        self._check(self.lib.nvbx_set_blocks(self._h, layer, _np_ptr(idx), idx.shape[0], _np_ptr(data)))

    def save_map(self, path):
        """Mapper::saveLayerCake (nvblox_node.cpp:1668): TSDF + colour + ESDF layers to one file."""
        self._check(self.lib.nvbx_save_map(self._h, str(path).encode()))

    def load_map(self, path):
        """Mapper::loadMap (nvblox_node.cpp:1703): replaces the map with the file's layers."""
        self._check(self.lib.nvbx_load_map(self._h, str(path).encode()))

    def synthetic_depth(self):
        r, c = C.c_int32(), C.c_int32()
        self._check(self.lib.nvbx_get_synthetic_depth(self._h, None, 0, C.byref(r), C.byref(c)))
        if r.value == 0:
            return None
        out = np.zeros((r.value, c.value), np.float32)
        self._check(self.lib.nvbx_get_synthetic_depth(self._h, _np_ptr(out), out.size, C.byref(r), C.byref(c)))
        return out

    def esdf_slice_image(self, unknown_value=1000.0):
        """EsdfSlicer::sliceLayerToDistanceImage for a host caller: ONE wait for the device (nvbx_esdf_slice_to_host sizes the image on the device);
        the buffer it is written into is kept and grows when the layer outgrows it."""
        r, c = C.c_int32(), C.c_int32()
        aabb = np.zeros(6, np.float32)
        buf = getattr(self, "_slice_buf", None)
        if buf is None:
            buf = self._slice_buf = np.empty(256 * 256, np.float32)
        rc = self.lib.nvbx_esdf_slice_to_host(self._h, unknown_value, _np_ptr(buf), buf.size, C.byref(r), C.byref(c), _np_ptr(aabb))
        if rc == -3:          # NVBX_E_CAPACITY: rows / cols are reported
            buf = self._slice_buf = np.empty(int(r.value * c.value * 1.5), np.float32)
            rc = self.lib.nvbx_esdf_slice_to_host(self._h, unknown_value, _np_ptr(buf), buf.size, C.byref(r), C.byref(c), _np_ptr(aabb))
        self._check(rc)
        return buf[:r.value * c.value].reshape(r.value, c.value).copy(), aabb

    def esdf_slice_image_device(self, unknown_value=1000.0):
        torch = self._torch
        r, c = C.c_int32(), C.c_int32()
        aabb = np.zeros(6, np.float32)
        self._check(self.lib.nvbx_esdf_slice_size(self._h, C.byref(r), C.byref(c), _np_ptr(aabb)))
        img = torch.empty((r.value, c.value), dtype=torch.float32, device="cuda:%d" % self.device)
        if img.numel():
            self._check(self.lib.nvbx_esdf_slice_to_image(self._h, unknown_value, ptr(img), img.numel(), C.byref(r), C.byref(c), _np_ptr(aabb)))
        return img, aabb

    def occupancy_grid_from_slice(self, img_dev, unknown_value=1000.0):
        grid = self._torch.empty(img_dev.shape, dtype=self._torch.int8, device=img_dev.device)
        self._check(self.lib.nvbx_occupancy_grid_from_slice(self._h, ptr(img_dev), img_dev.shape[0], img_dev.shape[1], unknown_value, ptr(grid)))
        self.synchronize()
        return grid

    def pointcloud_from_slice(self, img_dev, aabb, slice_height, unknown_value=1000.0):
        pts = self._torch.empty((img_dev.numel(), 4), dtype=self._torch.float32, device=img_dev.device)
        n = C.c_int32(); a = np.ascontiguousarray(aabb, np.float32)
        self._check(self.lib.nvbx_pointcloud_from_slice(self._h, ptr(img_dev), img_dev.shape[0], img_dev.shape[1], _np_ptr(a), float(slice_height), unknown_value, ptr(pts), C.byref(n)))
        return pts[:n.value]

    def esdf_slice_image_combined(self, other, unknown_value=1000.0):
        """EsdfSlicer::sliceLayersToCombinedDistanceImage (nvblox_node.cpp:836-840) of this mapper and `other`; host image."""
        import torch
        r, c = C.c_int32(), C.c_int32(); aabb = (C.c_float * 6)()
        self._check(self.lib.nvbx_esdf_slice_combined_size(self._h, other._h, C.byref(r), C.byref(c), aabb))
        if r.value == 0:
            return np.zeros((0, 0), np.float32), np.array(list(aabb), np.float32)
        img = torch.empty((r.value, c.value), dtype=torch.float32, device="cuda:%d" % self.device)
        self._check(self.lib.nvbx_esdf_slice_combined_to_image(self._h, other._h, unknown_value, ptr(img), img.numel(), C.byref(r), C.byref(c), aabb))
        self.synchronize()
        return img.cpu().numpy(), np.array(list(aabb), np.float32)

    def backproject_depth(self, depth, cam, max_distance_m=0.0, T_L_C=None):
        """DepthImageBackProjector::backProjectOnGPU (+ transformPointcloudOnGPU if T_L_C is given): [n, 3] float32 host array."""
        d = self._image(depth); rows, cols = d.shape
        pts = self._torch.empty((rows * cols, 3), dtype=self._torch.float32, device=d.device); n = C.c_int64()
        self._check(self.lib.nvbx_backproject_depth(self._h, ptr(d), rows, cols, C.byref(_args.camera(cam)), max_distance_m, ptr(pts), rows * cols, C.byref(n)))
        pts = pts[:n.value]
        if T_L_C is not None and n.value:
            self._check(self.lib.nvbx_transform_pointcloud(self._h, _np_ptr(self._T(T_L_C)), ptr(pts), n.value, ptr(pts)))
            self.synchronize()
        return pts.cpu().numpy()

    def split_depth_by_mask(self, depth, mask, T_CM_CD, depth_cam, mask_cam, occlusion_threshold_m=0.25, overlay=False):
        """ImageMasker::splitImageOnGPU (MultiMapper::integrateDepth with a mask): device tensors (unmasked, masked[, overlay])."""
        torch = self._torch
        d = self._image(depth); mk = self._image(mask, "mask", torch.uint8)
        un = torch.empty_like(d); ma = torch.empty_like(d)
        ov = torch.empty(d.shape + (3,), dtype=torch.uint8, device=d.device) if overlay else None
        self._split_depth(d, mk, T_CM_CD, depth_cam, mask_cam, occlusion_threshold_m, un, ma, ov)
        self.synchronize()       # (the outputs are torch tensors: torch's stream is not the mapper's)
        return (un, ma, ov) if overlay else (un, ma)

    def split_color_by_mask(self, rgb, mask):
        torch = self._torch
        c = _args.image(rgb, self._cuda, torch.uint8, "rgb", "(rows, cols, channels)"); mk = self._image(mask, "mask", torch.uint8)
        un = torch.empty_like(c); ma = torch.empty_like(c)
        self._check(self.lib.nvbx_split_color_by_mask(self._h, ptr(c), c.shape[0], c.shape[1], ptr(mk), ptr(un), ptr(ma)))
        self.synchronize()
        return un, ma

    def device_view(self):
        """nvbx_device_view for the caller's own kernels (include/nvblox_hip_device.h)."""
        from ._lib import DeviceView
        v = DeviceView()
        self._check(self.lib.nvbx_get_device_view(self._h, C.byref(v)))
        return v

    def esdf_dense_grid(self, min_vox, size_vox, default_value):
        mn = np.asarray(min_vox, np.int32); sz = np.asarray(size_vox, np.int32)
        out = self._torch.empty(tuple(int(s) for s in sz), dtype=self._torch.float32, device=self._cuda)
        self._check(self.lib.nvbx_esdf_dense_grid(self._h, _np_ptr(mn), _np_ptr(sz), default_value, ptr(out)))
        self.synchronize()
        return out.cpu().numpy()

    # -- Reader calls, from the point queries down to view_gain: ordered against torch's current stream on both sides, outputs by spec (see "helpers")
    def _around_torch_stream(self, call, order=True):
        """`call` enqueues on the mapper's stream, ordered behind torch's current stream (which produced the inputs) and ahead of it (which reads
        the results): no host synchronisation either way.  order=False: a call that launches nothing."""
        torch = self._torch
        cur = torch.cuda.current_stream(self.device); ms = self.torch_stream()
        other = order and ms.cuda_stream != cur.cuda_stream
        if other:
            ms.wait_stream(cur)
        self._check(call())
        if other:
            cur.wait_stream(ms)

    def _trim(self, counts, cap, volume, records=None):
        """The tail of a call that allocated its own sparse volume: ONE wait, for `counts` (the block count, or the two-element tensor of block and
        component count) -> the volume's tensors cut to min(block count, cap) blocks and, with a record table, its first min(component count,
        its capacity) records as Components."""
        c = counts.tolist()
        n = min(c[0], cap)
        cut = tuple(t[:n] if t is not None else None for t in volume)
        return cut if records is None else cut + (self.components_view(records, min(c[-1], int(records.shape[0]))),)

    # -- interpolated point queries (nvbx_query_points; SEMANTICS.md "Point queries")
    def query_tsdf(self, points, min_weight=None, unknown_value=1000.0, out=None):
        """Trilinear TSDF distance and its gradient per metre at `points` ((n, 3) float32 torch tensor or numpy array, metres):
        -> (distance [n] f32, gradient [n, 3] f32, valid [n] bool) on the mapper's device.  A corner counts with weight >= min_weight
        (default: the mapper's mesh_min_weight).  out=(distance, gradient, valid): preallocated tensors, nothing is allocated."""
        mw = self.params.mesh_min_weight if min_weight is None else min_weight
        return self._query(LAYER_TSDF, points, mw, unknown_value, out)

    def query_esdf(self, points, unknown_value=1000.0, out=None):
        """Interpolated ESDF distance and gradient (trilinear in 3-D mode; bilinear in the slice plane in 2-D mode, z ignored);
        same shapes and rules as query_tsdf."""
        return self._query(LAYER_ESDF, points, 0.0, unknown_value, out)

    def _query(self, layer, points, min_weight, unknown_value, out):
        """Runs on the mapper's stream, ordered behind torch's current stream (which produced the points) and ahead of it (which
        reads the results): no host synchronisation either way."""
        dev = self._cuda
        p = _args.points3(points, dev); n = p.shape[0]
        d, g, v = _args.outputs(out, (("distance", (n,), F32, True, True), ("gradient", (n, 3), F32, False, True), ("valid", (n,), FLAG, False, True)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_query_points(self._h, layer, ptr(p), n, float(min_weight), float(unknown_value), ptr(d), ptr(g), ptr(v)),
                                  order=n > 0)
        self._hold("_keep_q", [p])      # (the kernel reads the points: they, and an uploaded copy, live until the next query)
        return d, g, v

    # -- pose alignment (nvbx_align_points / nvbx_align_depth / nvbx_linearize_points; SEMANTICS.md "Pose alignment")
    def align_options(self, **kw):
        """nvbx_align_options: the library's defaults with the given fields replaced (max_iterations, subsampling, min_weight, huber_delta_m,
        damping, min_pivot_ratio, stop_translation_m, stop_rotation_rad, min_valid, max_depth_m)."""
        return _args.struct_options(_lib.AlignOptions, self.lib.nvbx_default_align_options, kw, "alignment")

    def align_points(self, points, T_L_S_guess, out=None, **options):
        """Refine the pose of a sensor-frame cloud ((n, 3) float32 torch tensor or numpy array) against the TSDF, from T_L_S_guess: -> AlignResult.
        Every launch is enqueued at once on the mapper's stream, nothing waits on the host.  options: see align_options.
        out: a preallocated result buffer (uint8 tensor of ALIGN_RESULT_BYTES bytes), nothing is allocated."""
        p = _args.points3(points, self._cuda); T = self._T(T_L_S_guess); o = self.align_options(**options)
        buf = _args.result_buffer(out, ALIGN_RESULT_BYTES, self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_align_points(self._h, ptr(p), p.shape[0], _np_ptr(T), C.byref(o), ptr(buf)))
        self._hold("_keep_a", [p])      # (the launches read the points: they, and an uploaded copy, live until the next alignment)
        return AlignResult(buf)

    def align_depth(self, depth, T_L_C_guess, cam, out=None, **options):
        """Refine a camera pose from a float32 depth image (metres; torch tensor or numpy array): the pixels (r s, c s) with
        0 < depth <= max_depth_m are back-projected inside the launch, no point buffer is written.  -> AlignResult; out as for align_points."""
        d, k = self._point_source(depth, cam)
        T = self._T(T_L_C_guess); o = self.align_options(**options)
        buf = _args.result_buffer(out, ALIGN_RESULT_BYTES, self._cuda)
        # (a non-collapsing pointer: nvbx_align_depth refuses a NULL image before it looks at its size)
        self._around_torch_stream(lambda: self.lib.nvbx_align_depth(self._h, C.c_void_p(d.data_ptr()), d.shape[0], d.shape[1], _np_ptr(T), C.byref(k),
                                                                    C.byref(o), ptr(buf)))
        self._hold("_keep_a", [d])
        return AlignResult(buf)

    def linearize_points(self, points, T_L_S, per_point=True, out=None, **options):
        """One linearization at T_L_S, no step applied: -> (AlignResult, points_L [n, 3] f32, residual [n] f32, gradient [n, 3] f32, valid [n] bool)
        on the mapper's device; the per-point tensors are None with per_point=False.  They are bit for bit nvbx_transform_pointcloud and
        query_tsdf(unknown_value=0) at those points.  out=(buffer | None, points_L | None, residual | None, gradient | None, valid | None):
        preallocated tensors, `out` then decides what is written (a None per-point entry is not) and per_point is not looked at."""
        dev = self._cuda
        p = _args.points3(points, dev); n = p.shape[0]
        T = self._T(T_L_S); o = self.align_options(**options)
        buf_out, rest = (None, None) if out is None else (out[0], out[1:])
        buf = _args.result_buffer(buf_out, ALIGN_RESULT_BYTES, dev)
        pl, r, g, v = _args.outputs(rest, (("points_L", (n, 3), F32, False, per_point), ("residual", (n,), F32, False, per_point),
                                           ("gradient", (n, 3), F32, False, per_point), ("valid", (n,), FLAG, False, per_point)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_linearize_points(self._h, ptr(p), n, _np_ptr(T), C.byref(o), ptr(buf), ptr(pl), ptr(r), ptr(g), ptr(v)))
        self._hold("_keep_a", [p])
        return AlignResult(buf), pl, r, g, v

    # -- colour point queries and pose alignment with a colour term (nvbx_query_colors / nvbx_*_color; SEMANTICS.md "Colour alignment and colour queries")
    def query_color(self, points, min_color_weight=1e-4, rgb=True, out=None):
        """The colour layer at `points` ((n, 3) float32, metres), trilinear over the TSDF query's lattice: -> (rgb [n, 3] f32 | None, luminance [n]
        f32 in levels, its gradient [n, 3] f32 per metre, valid [n] bool) on the mapper's device; zeros at an invalid point.  A corner counts
        with colour weight >= min_color_weight.  rgb=False: no rgb output.  out=(rgb | None, luminance | None, gradient | None, valid):
        preallocated tensors, nothing is allocated and `rgb` is not looked at."""
        dev = self._cuda
        p = _args.points3(points, dev); n = p.shape[0]
        c, y, g, v = _args.outputs(out, (("rgb", (n, 3), F32, False, rgb), ("luminance", (n,), F32, False, True), ("gradient", (n, 3), F32, False, True),
                                         ("valid", (n,), FLAG, True, True)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_query_colors(self._h, ptr(p), n, float(min_color_weight), ptr(c), ptr(y), ptr(g), ptr(v)), order=n > 0)
        self._hold("_keep_q", [p])
        return c, y, g, v

    def align_color_options(self, **kw):
        """nvbx_align_color_options: the library's defaults with the given fields replaced (color_weight, min_color_weight, color_huber_levels)."""
        return _args.struct_options(_lib.AlignColorOptions, self.lib.nvbx_default_align_color_options, kw, "colour alignment")

    def _align_color_setup(self, T, out, options):
        """-> (pose, align options, colour options, result buffer, pointer to its colour record); `options` mixes the fields of both structs"""
        names = [f for f, _ in _lib.AlignColorOptions._fields_]
        co = self.align_color_options(**{k: v for k, v in options.items() if k in names})
        o = self.align_options(**{k: v for k, v in options.items() if k not in names})
        buf = _args.result_buffer(out, ALIGN_COLOR_RESULT_BYTES, self._cuda)
        return self._T(T), o, co, buf, C.c_void_p(buf.data_ptr() + ALIGN_RESULT_BYTES)

    def align_points_color(self, points, colors, T_L_S_guess, out=None, **options):
        """align_points with a colour term: `colors` = (n, 3) uint8 rgb, one per point.  -> AlignColorResult.  options: the fields of
        align_options and align_color_options.  out: a preallocated uint8 tensor of ALIGN_COLOR_RESULT_BYTES bytes."""
        p = _args.points3(points, self._cuda); c = _args.colors3(colors, self._cuda)
        if c.shape[0] != p.shape[0]:
            raise ValueError("colors must hold one (r, g, b) per point: %d points, %d colours" % (p.shape[0], c.shape[0]))
        T, o, co, buf, cbuf = self._align_color_setup(T_L_S_guess, out, options)
        self._around_torch_stream(lambda: self.lib.nvbx_align_points_color(self._h, ptr(p), ptr(c), p.shape[0], _np_ptr(T), C.byref(o), C.byref(co), ptr(buf), cbuf))
        self._hold("_keep_a", [p, c])
        return AlignColorResult(buf)

    def align_depth_color(self, depth, rgb, T_L_C_guess, cam, out=None, **options):
        """align_depth with a colour term: `rgb` = the (rows, cols, 3) uint8 image registered with the depth image; the colour of a point is its
        depth pixel's.  -> AlignColorResult; options and out as for align_points_color."""
        d, k = self._point_source(depth, cam)
        c = _args.image(rgb, self._cuda, self._torch.uint8, "rgb", "(rows, cols, 3)", (3,))
        if tuple(c.shape[:2]) != tuple(d.shape):
            raise ValueError("rgb must have the depth image's size %s, got %s" % (tuple(d.shape), tuple(c.shape[:2])))
        T, o, co, buf, cbuf = self._align_color_setup(T_L_C_guess, out, options)
        self._around_torch_stream(lambda: self.lib.nvbx_align_depth_color(self._h, C.c_void_p(d.data_ptr()), C.c_void_p(c.data_ptr()), d.shape[0], d.shape[1],
                                                                          _np_ptr(T), C.byref(k), C.byref(o), C.byref(co), ptr(buf), cbuf))
        self._hold("_keep_a", [d, c])
        return AlignColorResult(buf)

    def linearize_points_color(self, points, colors, T_L_S, per_point=True, out=None, **options):
        """linearize_points with a colour term: -> (AlignColorResult, points_L, residual, gradient, valid, luminance [n] f32, color_gradient [n, 3] f32,
        color_valid [n] bool); the last three are bit for bit query_color at points_L.  per_point and out (the buffer and the seven per-point
        tensors, each may be None) as for linearize_points."""
        dev = self._cuda
        p = _args.points3(points, dev); n = p.shape[0]
        c = _args.colors3(colors, dev)
        if c.shape[0] != n:
            raise ValueError("colors must hold one (r, g, b) per point: %d points, %d colours" % (n, c.shape[0]))
        buf_out, rest = (None, None) if out is None else (out[0], out[1:])
        T, o, co, buf, cbuf = self._align_color_setup(T_L_S, buf_out, options)
        pl, r, g, v, cy, cg, cv = _args.outputs(rest, (("points_L", (n, 3), F32, False, per_point), ("residual", (n,), F32, False, per_point),
                                                       ("gradient", (n, 3), F32, False, per_point), ("valid", (n,), FLAG, False, per_point),
                                                       ("luminance", (n,), F32, False, per_point), ("color_gradient", (n, 3), F32, False, per_point),
                                                       ("color_valid", (n,), FLAG, False, per_point)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_linearize_points_color(self._h, ptr(p), ptr(c), n, _np_ptr(T), C.byref(o), C.byref(co), ptr(buf), cbuf,
                                                                               ptr(pl), ptr(r), ptr(g), ptr(v), ptr(cy), ptr(cg), ptr(cv)))
        self._hold("_keep_a", [p, c])
        return AlignColorResult(buf), pl, r, g, v, cy, cg, cv

    # -- relocalisation (nvbx_score_poses_* / nvbx_relocalize_*; SEMANTICS.md "Relocalisation")
    def score_options(self, **kw):
        """nvbx_score_options: the library's defaults with the given fields replaced (min_weight, inlier_distance_m, conflict_distance_m,
        max_depth_m, subsampling).  A threshold <= 0 selects its default: one voxel size, half the truncation distance, 1e-4."""
        return _args.struct_options(_lib.ScoreOptions, self.lib.nvbx_default_score_options, kw, "score")

    def _point_source(self, points_or_depth, cam):
        """The points of an alignment, scoring or relocalisation call -> (device tensor, Camera | None): cam None: an (n, 3) cloud for the _points
        entries; else a (rows, cols) depth image for the _depth ones"""
        if cam is None:
            p = _args.points3(points_or_depth, self._cuda)
            return p, None
        d = self._dev(points_or_depth, self._torch.float32)
        if d.dim() != 2:
            raise ValueError("depth must be a (rows, cols) image")
        return d, self._cam(cam)

    def score_poses(self, points_or_depth, poses, cam=None, out=None, **options):
        """How well each of K candidate sensor poses ((K, 4, 4) or (K, 16) float32, torch device tensor or numpy array) explains a sensor-frame cloud
        ((n, 3) float32; cam=None) or a float32 depth image (with `cam`: the pixels (r s, c s) with 0 < depth <= max_depth_m): one launch.
        -> (counts int32 [K, 4]: points, valid, inliers, conflicts; abs_residual_q20 int64 [K]: sum of |d| in 2^-20 m over the valid points) on the
        mapper's device, two views of one int64 [K, 3] tensor of 24-byte records.  A pose that is not finite or out of range has points = -1 and
        zeros.  options: see score_options.  out: that preallocated int64 [K, 3] tensor, nothing is allocated."""
        src, k = self._point_source(points_or_depth, cam)
        T = _args.poses16(poses, self._cuda); n = int(T.shape[0])
        o = self.score_options(**options)
        rec, counts, residual = _args.score_records(out, n, self._cuda)
        if k is None:
            call = lambda: self.lib.nvbx_score_poses_points(self._h, ptr(src), src.shape[0], ptr(T), n, C.byref(o), ptr(rec))
        else:      # (a non-collapsing pointer: the entry refuses a NULL image before it looks at its size)
            call = lambda: self.lib.nvbx_score_poses_depth(self._h, C.c_void_p(src.data_ptr()), src.shape[0], src.shape[1], C.byref(k), ptr(T), n,
                                                           C.byref(o), ptr(rec))
        self._around_torch_stream(call, order=n > 0)
        self._hold("_keep_sp", [src, T])      # (the kernel reads the points and the poses: they live until the next call)
        return counts, residual

    @staticmethod
    def _lattice(half_extent_m, half_yaw_rad, steps):
        he = np.broadcast_to(np.asarray(half_extent_m, np.float32), (3,)); st = [int(s) for s in steps]
        if len(st) != 4:
            raise ValueError("steps must be (nx, ny, nz, nyaw)")
        return _lib.SearchLattice((C.c_float * 3)(*he.tolist()), float(half_yaw_rad), (C.c_int32 * 4)(*st))

    def search_lattice(self, T0, half_extent_m, half_yaw_rad, steps):
        """The poses relocalize_* score around T0: -> (K, 4, 4) float32 numpy array, K = nx ny nz nyaw, hypothesis
        h = ((ix ny + iy) nz + iz) nyaw + iw at t0 + (dx[ix], dy[iy], dz[iz]) with Rz(yaw[iw]) R0; step i of s covers -half .. +half evenly
        (0 for s = 1).  half_extent_m: one number or (x, y, z).  Host only."""
        lat = self._lattice(half_extent_m, half_yaw_rad, steps); T = self._T(T0)
        K = 1
        for s in lat.steps:
            K *= max(int(s), 0)
        out = np.zeros((max(min(K, 1 << 20), 1), 4, 4), np.float32)
        K = self._check(self.lib.nvbx_search_lattice_poses(_np_ptr(T), C.byref(lat), _np_ptr(out)))
        return out[:K]

    def _relocalize(self, src, k, T0, half_extent_m, half_yaw_rad, steps, min_inliers, score, align, scores, out):
        lat = self._lattice(half_extent_m, half_yaw_rad, steps); T = self._T(T0)
        so = self.score_options(**(score or {})); ao = self.align_options(**(align or {}))
        buf = _args.result_buffer(out, RELOC_RESULT_BYTES, self._cuda)
        views = None
        rec = None
        if scores is not None and scores is not False:
            K = int(np.prod([int(s) for s in lat.steps]))
            rec, counts, residual = _args.score_records(None if scores is True else scores, K, self._cuda)
            views = (counts, residual)
        mi = int(min_inliers) if min_inliers is not None else 0
        if k is None:
            call = lambda: self.lib.nvbx_relocalize_points(self._h, ptr(src), src.shape[0], _np_ptr(T), C.byref(lat), C.byref(so), mi, C.byref(ao),
                                                           ptr(rec), ptr(buf))
        else:
            call = lambda: self.lib.nvbx_relocalize_depth(self._h, C.c_void_p(src.data_ptr()), src.shape[0], src.shape[1], C.byref(k), _np_ptr(T),
                                                          C.byref(lat), C.byref(so), mi, C.byref(ao), ptr(rec), ptr(buf))
        self._around_torch_stream(call)
        self._hold("_keep_a", [src])
        return RelocalizeResult(buf, views)

    def relocalize_points(self, points, T0, half_extent_m, half_yaw_rad, steps, min_inliers=None, score=None, align=None, scores=None, out=None):
        """Find a sensor-frame cloud's pose in the map from a guess that may be far outside the truncation band: the lattice search_lattice(T0,
        half_extent_m, half_yaw_rad, steps) is scored as by score_poses, the hypothesis with the most inliers - conflicts (ties: more inliers, then
        the lower index) is refined with align_points' iterations, and the refined pose is scored once more -- all enqueued at once on the mapper's
        stream, nothing waits on the host.  -> RelocalizeResult.  With fewer than min_inliers (default 50) inliers at the best hypothesis the
        status is NO_CANDIDATE and no refinement runs.  score / align: dicts of score_options / align_options fields.  scores: True, or a
        preallocated int64 [K, 3] tensor: the lattice's records are kept (result.scores).  out: a preallocated result buffer (uint8 tensor of
        RELOC_RESULT_BYTES bytes)."""
        src, _ = self._point_source(points, None)
        return self._relocalize(src, None, T0, half_extent_m, half_yaw_rad, steps, min_inliers, score, align, scores, out)

    def relocalize_depth(self, depth, T0, cam, half_extent_m, half_yaw_rad, steps, min_inliers=None, score=None, align=None, scores=None, out=None):
        """relocalize_points for a float32 depth image: scoring takes the pixels (r s, c s) of the score options' subsampling and max_depth_m, the
        refinement those of the align options', both back-projected inside the launches."""
        src, k = self._point_source(depth, cam)
        return self._relocalize(src, k, T0, half_extent_m, half_yaw_rad, steps, min_inliers, score, align, scores, out)

    # -- map merging (nvbx_merge_map; SEMANTICS.md "Map merging")
    def merge_options(self, **kw):
        """nvbx_merge_options: the library's defaults with the given fields replaced (min_weight, weight_scale, merge_color)."""
        return _args.struct_options(_lib.MergeOptions, self.lib.nvbx_default_merge_options, kw, "merge")

    def merge_from(self, other, T_D_S, out=None, **options):
        """Bring `other`'s TSDF and colour into this map under p_D = T_D_S p_S (row-major 4 x 4): -> MergeResult.  Missing blocks are allocated
        (the pools grow; NvbxError with code -3 if max_block_capacity cannot hold them, this map then unchanged); `other` is not modified.
        The launches run on this mapper's stream behind everything enqueued on `other`'s.  options: see merge_options.
        out: a preallocated result buffer (uint8 tensor of MERGE_RESULT_BYTES bytes)."""
        if not isinstance(other, Mapper):
            raise TypeError("merge_from needs a Mapper")
        T = self._T(T_D_S); o = self.merge_options(**options)
        buf = _args.result_buffer(out, MERGE_RESULT_BYTES, self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_merge_map(self._h, other._h, _np_ptr(T), C.byref(o), ptr(buf)))
        return MergeResult(buf)

    # -- feature merging (nvbx_merge_features; SEMANTICS.md "Feature merging")
    def feature_merge_options(self, **kw):
        """nvbx_feature_merge_options: the library's defaults with the given fields replaced (min_weight, weight_scale)."""
        if "reserved" in kw:
            raise TypeError("unknown feature merge option 'reserved'")
        return _args.struct_options(_lib.FeatureMergeOptions, self.lib.nvbx_default_feature_merge_options, kw, "feature merge")

    def merge_features_from(self, other, T_D_S=None, out=None, **options):
        """Bring `other`'s feature layer into this map under p_D = T_D_S p_S (row-major 4 x 4; None: the identity): -> FeatureMergeResult.
        Meant to follow merge_from with the same pose: only blocks this map already has are written, nothing is allocated; a voxel takes
        the voxel of `other` that contains its centre.  `other` is not modified.  The launches run on this mapper's stream behind everything
        enqueued on `other`'s.  options: see feature_merge_options.  out: a preallocated result buffer (uint8 tensor of
        FEATURE_MERGE_RESULT_BYTES bytes)."""
        if not isinstance(other, Mapper):
            raise TypeError("merge_features_from needs a Mapper")
        T = self._T(np.eye(4, dtype=np.float32) if T_D_S is None else T_D_S); o = self.feature_merge_options(**options)
        buf = _args.result_buffer(out, FEATURE_MERGE_RESULT_BYTES, self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_merge_features(self._h, other._h, _np_ptr(T), C.byref(o), ptr(buf)))
        return FeatureMergeResult(buf)

    # -- resampling (nvbx_resample_map; SEMANTICS.md "Resampling")
    def resample_options(self, **kw):
        """nvbx_resample_options: the library's defaults with the given fields replaced (min_weight, weight_scale, merge_color, taps)."""
        return _args.struct_options(_lib.ResampleOptions, self.lib.nvbx_default_resample_options, kw, "resample")

    def resample_from(self, other, T_D_S=None, out=None, **options):
        """Bring `other`'s TSDF and colour into this map, whose voxel size is 1 to 4 times `other`'s, under p_D = T_D_S p_S (row-major 4 x 4;
        None: the identity): -> MergeResult.  Every voxel averages taps x taps x taps sub-samples of `other` and fuses when at least half of
        them are valid; the rest is merge_from's.  options: see resample_options.  out: as for merge_from."""
        if not isinstance(other, Mapper):
            raise TypeError("resample_from needs a Mapper")
        T = None if T_D_S is None else self._T(T_D_S)
        o = self.resample_options(**options)
        buf = _args.result_buffer(out, MERGE_RESULT_BYTES, self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_resample_map(self._h, other._h, None if T is None else _np_ptr(T), C.byref(o), ptr(buf)))
        return MergeResult(buf)

    def coarsened(self, factor=2.0, block_capacity=None, **options):
        """-> (Mapper, MergeResult): a new mapper on this one's device and stream setting, with this one's params except voxel_size * factor
        (1 <= factor <= 4), holding this map resampled under the identity.  block_capacity: the new mapper's (default: this one's initial
        capacity; it grows on demand).  options: see resample_options."""
        p = Params.from_buffer_copy(bytes(self.params))
        p.voxel_size = float(np.float32(self.params.voxel_size) * np.float32(factor))
        m = Mapper(p, device=self.device, block_capacity=self._capacity0 if block_capacity is None else int(block_capacity), stream=self._stream0)
        try:
            res = m.resample_from(self, None, **options)
        except Exception:
            m.close()
            raise
        return m, res

    # -- surface points and map-to-map registration (nvbx_surface_points / nvbx_align_map / nvbx_relocalize_map; SEMANTICS.md "Surface points")
    def surface_options(self, **kw):
        """nvbx_surface_options: the library's defaults with the given fields replaced (min_weight, stride, require_color, and
        box_min_max_vox = (min x, y, z, max x, y, z) in global voxel coordinates, inclusive, which also sets use_box)."""
        kw = dict(kw)
        box = kw.pop("box_min_max_vox", None)
        if "require_color" in kw:
            kw["require_color"] = int(bool(kw["require_color"]))
        o = _args.struct_options(_lib.SurfaceOptions, self.lib.nvbx_default_surface_options, kw, "surface")
        if box is not None:
            b = [int(v) for v in np.asarray(box).reshape(-1)]
            if len(b) != 6:
                raise ValueError("box_min_max_vox must hold (min x, y, z, max x, y, z)")
            o.box_min_max_vox = (C.c_int32 * 6)(*b)
            if "use_box" not in kw:
                o.use_box = 1
        return o

    def surface_points(self, color=False, normals=False, capacity=None, out=None, **options):
        """The TSDF's zero crossings as a point cloud on the mapper's device: -> (points [n, 3] f32, colors [n, 3] u8 | None, normals [n, 3] f32
        | None, count), in the order (pool slot of the origin block, voxel, axis); two calls on an unchanged mapper give identical tensors.
        count is the number of crossings, n = min(count, capacity).  capacity=None: a first call counts (one wait), a second one emits.
        out=(points, colors | None, normals | None): preallocated tensors of one row count, the capacity; color and normals are then not
        looked at.  Both forms wait once more, for the count the tensors are trimmed to.  options: see surface_options."""
        dev = self._cuda; torch = self._torch
        o = self.surface_options(**options)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        if out is not None:
            if not out or out[0] is None:
                raise ValueError("out needs a points tensor")
            capacity = int(out[0].shape[0])
        elif capacity is None:
            self._around_torch_stream(lambda: self.lib.nvbx_surface_points(self._h, C.byref(o), None, None, None, 0, ptr(count)))
            capacity = int(count.item())
        cap = int(capacity)
        p, c, nr = _args.outputs(out, (("points", (cap, 3), F32, True, True), ("colors", (cap, 3), U8, False, color),
                                       ("normals", (cap, 3), F32, False, normals)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_surface_points(self._h, C.byref(o), ptr(p), ptr(c), ptr(nr), cap, ptr(count)))
        total = int(count.item())
        n = min(total, cap)
        return p[:n], (c[:n] if c is not None else None), (nr[:n] if nr is not None else None), total

    def _surface_of(self, other, surface, what):
        if not isinstance(other, Mapper):
            raise TypeError("%s needs a Mapper" % what)
        return other.surface_options(**(surface or {}))

    def align_map(self, other, T_D_S_guess, color_weight=None, surface=None, out=None, **options):
        """Refine the pose T_D_S of `other`'s map in this one (p_D = T_D_S p_S: merge_from's argument) from a guess inside the truncation band:
        `other`'s surface points (surface: a dict of surface_options fields, e.g. stride) are aligned against this map's TSDF by align_points'
        launches -> AlignResult; with color_weight (a number) by align_points_color's, over the crossings that have a colour ->
        AlignColorResult.  Runs on this mapper's stream behind `other`'s; waits once on the host, for the point count.  options: the fields of
        align_options and, with color_weight, of align_color_options.  out: as for align_points / align_points_color."""
        so = self._surface_of(other, surface, "align_map")
        if color_weight is None:
            T = self._T(T_D_S_guess); o = self.align_options(**options)
            buf = _args.result_buffer(out, ALIGN_RESULT_BYTES, self._cuda)
            self._around_torch_stream(lambda: self.lib.nvbx_align_map(self._h, other._h, _np_ptr(T), C.byref(so), C.byref(o), None, ptr(buf), None))
            return AlignResult(buf)
        T, o, co, buf, cbuf = self._align_color_setup(T_D_S_guess, out, dict(options, color_weight=float(color_weight)))
        self._around_torch_stream(lambda: self.lib.nvbx_align_map(self._h, other._h, _np_ptr(T), C.byref(so), C.byref(o), C.byref(co), ptr(buf), cbuf))
        return AlignColorResult(buf)

    def relocalize_map(self, other, T0, half_extent_m, half_yaw_rad, steps, min_inliers=None, surface=None, score=None, align=None, scores=None, out=None):
        """Find the pose of `other`'s map in this one from a guess that may be far outside the truncation band: relocalize_points over `other`'s
        surface points (surface: a dict of surface_options fields).  -> RelocalizeResult; its align.T is T_D_S.  Stream order and the one host
        wait as for align_map; the other arguments as for relocalize_points."""
        so = self._surface_of(other, surface, "relocalize_map")
        lat = self._lattice(half_extent_m, half_yaw_rad, steps); T = self._T(T0)
        sc = self.score_options(**(score or {})); ao = self.align_options(**(align or {}))
        buf = _args.result_buffer(out, RELOC_RESULT_BYTES, self._cuda)
        views = None
        rec = None
        if scores is not None and scores is not False:
            K = int(np.prod([int(s) for s in lat.steps]))
            rec, counts, residual = _args.score_records(None if scores is True else scores, K, self._cuda)
            views = (counts, residual)
        mi = int(min_inliers) if min_inliers is not None else 0
        self._around_torch_stream(lambda: self.lib.nvbx_relocalize_map(self._h, other._h, _np_ptr(T), C.byref(lat), C.byref(so), C.byref(sc), mi,
                                                                       C.byref(ao), ptr(rec), ptr(buf)))
        return RelocalizeResult(buf, views)

    # -- rendering and ray casts (nvbx_render_view / nvbx_cast_rays; SEMANTICS.md "Rendering and ray casts")
    def render(self, T_L_C, cam, subsampling=None, max_ray_length_m=None, color=True, normals=False, out=None):
        """The map seen from camera `cam` at pose T_L_C: -> (depth [rows/s, cols/s] f32, color [.., 3] u8 | None, normals [.., 3] f32 | None) on the
        mapper's device.  depth 0 = no surface.  subsampling / max_ray_length_m None: the mapper's sphere_tracing_* parameters.
        out=(depth, color | None, normals | None): preallocated tensors, nothing is allocated; `out` then decides what is computed (a None
        entry is not) and the color / normals flags are not looked at."""
        k = self._cam(cam); T = self._T(T_L_C)
        s = _args.subsampling_arg(subsampling)
        s_eff = s if s > 0 else max(1, self.params.sphere_tracing_subsampling)
        rows, cols = k.height // s_eff, k.width // s_eff
        d, c, nr = _args.outputs(out, (("depth", (rows, cols), F32, True, True), ("color", (rows, cols, 3), U8, False, color),
                                       ("normals", (rows, cols, 3), F32, False, normals)), self._cuda)
        r_, c_ = C.c_int32(), C.c_int32()
        self._around_torch_stream(lambda: self.lib.nvbx_render_view(
            self._h, _np_ptr(T), C.byref(k), s, float(max_ray_length_m) if max_ray_length_m is not None else 0.0, ptr(d), ptr(c), ptr(nr), d.numel(),
            C.byref(r_), C.byref(c_)))
        assert (r_.value, c_.value) == (rows, cols)
        return d, c, nr

    def cast_rays(self, origins, directions, max_ray_length_m=None, color=False, normals=False, out=None):
        """Cast n rays (origins, directions: (n, 3) float32 torch tensors or numpy arrays, map-frame metres, directions of unit length):
        -> (t [n] f32 metres, 0 = no hit; hit [n] bool; color [n, 3] u8 | None; normals [n, 3] f32 | None) on the mapper's device.
        out=(t, hit | None, color | None, normals | None): preallocated tensors, nothing is allocated; `out` then decides what is computed
        (a None entry is not) and the color / normals flags are not looked at."""
        dev = self._cuda
        o = _args.points3(origins, dev, "origins"); dr = _args.points3(directions, dev, "directions")
        if o.shape != dr.shape:
            raise ValueError("origins %s and directions %s differ in shape" % (tuple(o.shape), tuple(dr.shape)))
        n = o.shape[0]
        t, h, c, nr = _args.outputs(out, (("t", (n,), F32, True, True), ("hit", (n,), FLAG, False, True), ("color", (n, 3), U8, False, color),
                                          ("normals", (n, 3), F32, False, normals)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_cast_rays(
            self._h, ptr(o), ptr(dr), n, float(max_ray_length_m) if max_ray_length_m is not None else 0.0, ptr(t), ptr(h), ptr(c), ptr(nr)))
        self._hold("_keep_r", [o, dr])      # (the kernel reads the rays: they, and an uploaded copy, live until the next cast)
        return t, h, c, nr

    # -- feature layer (nvbx_enable_features / nvbx_integrate_features / nvbx_query_features; SEMANTICS.md "Feature layer")
    def enable_features(self, channels):
        """Turn the feature layer on with `channels` fp16 values per voxel (a multiple of 8, 8 .. 256).  Again with the same value: no-op."""
        self._check(self.lib.nvbx_enable_features(self._h, int(channels)))
        self.feature_channels = int(channels)

    def integrate_features(self, feat, T_L_C, cam, stride):
        """Average a feature image into the voxels the frame sees.  feat: (rows_f, cols_f, C) torch.float16 device tensor or numpy float16 array;
        `cam` is the full-resolution camera the features were computed from, feature pixel (i, j) is centred on its pixel coordinate
        ((j + 0.5) stride, (i + 0.5) stride)."""
        f = _args.image(feat, self._cuda, self._torch.float16, "feat", "(rows_f, cols_f, C)", convert=False)
        ch = getattr(self, "feature_channels", 0)      # (0: not enabled -- the library refuses the call)
        if ch and f.shape[2] != ch:
            raise NvbxError("integrate_features: the image has %d channels, the layer %d (enable_features)" % (f.shape[2], ch))
        # (a non-collapsing pointer: nvbx_integrate_features refuses a NULL image before it looks at its size)
        (pf, rows, cols, T, k), keep = _args.frame(f, T_L_C, _args.camera(cam), collapse=False)
        self._around_torch_stream(lambda: self.lib.nvbx_integrate_features(self._h, pf, rows, cols, int(stride), T, k))
        self._hold("_keep_f", [f])      # (the kernel reads the image: it, and an uploaded copy, live until the next feature frame)

    def query_features(self, points, out=None):
        """The feature voxel that contains each of `points` ((n, 3) float32 torch tensor or numpy array, metres): -> (features [n, C] f16,
        weights [n] f32) on the mapper's device; weight 0 and zeros where the map holds no features (never an error).
        out=(features, weights): preallocated tensors, nothing is allocated."""
        dev = self._cuda
        p = _args.points3(points, dev); n = p.shape[0]; ch = getattr(self, "feature_channels", 0)
        f, w = _args.outputs(out, (("features", (n, ch), F16, True, True), ("weights", (n,), F32, True, True)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_query_features(self._h, ptr(p), n, ptr(f), ptr(w)), order=n > 0)
        self._hold("_keep_fq", [p])
        return f, w

    def feature_blocks(self, indices):
        """Whole feature blocks: -> (features [n, 512, C] f16, weights [n, 512] f32, found [n] bool) as numpy arrays; voxel t = vx 64 + vy 8 + vz."""
        idx = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3))
        ch = getattr(self, "feature_channels", 0)
        f = np.zeros((idx.shape[0], 512, max(ch, 1)), np.float16); w = np.zeros((idx.shape[0], 512), np.float32)
        found = np.zeros(idx.shape[0], np.int32)
        self._check(self.lib.nvbx_get_feature_blocks(self._h, _np_ptr(idx), idx.shape[0], _np_ptr(f), _np_ptr(w), _np_ptr(found)))
        return f, w, found.astype(bool)

    def set_feature_blocks(self, indices, features, weights):
        """Whole feature blocks, the layout of feature_blocks: features [n, 512, C] float16, weights [n, 512] float32 (numpy arrays) -> written
        [n] bool.  A block is written -- all 512 voxels replaced -- only where this map has it with its TSDF layer; nothing else of the map
        changes.  The indices are distinct."""
        idx = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3)); n = idx.shape[0]
        ch = getattr(self, "feature_channels", 0)      # (0: not enabled -- the library refuses the call)
        f = np.ascontiguousarray(np.asarray(features, np.float16)); w = np.ascontiguousarray(np.asarray(weights, np.float32))
        if (ch and f.shape != (n, 512, ch)) or w.shape != (n, 512):
            raise ValueError("features must be (%d, 512, %d) and weights (%d, 512), got %s and %s" % (n, ch, n, f.shape, w.shape))
        written = np.zeros(n, np.int32)
        self._check(self.lib.nvbx_set_feature_blocks(self._h, _np_ptr(idx), n, _np_ptr(f), _np_ptr(w), _np_ptr(written)))
        return written.astype(bool)

    # -- feature matching (nvbx_match_features / nvbx_match_points; SEMANTICS.md "Feature matching")
    _METRICS = {"dot": 0, "cosine": 1}

    def _queries(self, queries, metric):
        """-> (fp16 [Q, C] tensor on the mapper's device, Q, metric id)"""
        torch = self._torch
        if metric not in self._METRICS:
            raise ValueError("metric must be 'dot' or 'cosine', got %r" % (metric,))
        if not isinstance(queries, torch.Tensor):
            queries = np.asarray(queries)
        if queries.dtype not in (torch.float16, np.float16) or len(queries.shape) != 2:
            raise ValueError("queries must be a (Q, C) float16 array, got %s %s" % (tuple(queries.shape), queries.dtype))
        q = self._dev(queries, torch.float16)
        ch = getattr(self, "feature_channels", 0)      # (0: not enabled -- the library refuses the call)
        if ch and q.shape[1] != ch:
            raise NvbxError("queries have %d channels, the layer %d (enable_features)" % (q.shape[1], ch))
        return q, int(q.shape[0]), self._METRICS[metric]

    def match_features(self, queries, metric="cosine", min_weight=1.0, all_scores=False, out=None):
        """Score every feature voxel of the map against `queries` ((Q, C) torch.float16 device tensor or numpy float16 array, Q <= 128):
        -> (indices [n, 3] i32, labels [n, 512] i32, scores [n, 512] f32, all [n, 512, Q] f32 | None) on the mapper's device, one entry per feature
        block in no particular order, voxel t = vx 64 + vy 8 + vz.  label = the best query of a voxel whose weight is > 0 and >= min_weight (a tie:
        the lowest index), score = its score; -1 and 0 elsewhere.  Buffers are sized from block_indices(LAYER_FEATURE); the call waits once for the count.
        out=(indices, labels, scores, all | None, count): preallocated tensors of any capacity n_cap (count: one int64), nothing is allocated and
        nothing waited for: -> (indices, labels, scores, all | None, count) untrimmed; count (a device tensor) may exceed n_cap, entries from n_cap on
        are not written; `out` then decides whether the score matrix is computed and the all_scores flag is not looked at."""
        q, nq, mid = self._queries(queries, metric)
        (idx, lab, sc, al, cnt), cap, counts = _args.sparse_volume(out, self._cuda, lambda: self.num_blocks(LAYER_FEATURE), all_queries=nq, want_all=all_scores)
        self._around_torch_stream(lambda: self.lib.nvbx_match_features(self._h, ptr(q), nq, mid, float(min_weight), ptr(idx), ptr(lab), ptr(sc), ptr(al), cap, ptr(cnt)))
        self._hold("_keep_mq", [q])      # (the kernel reads the queries: they, and an uploaded copy, live until the next match)
        return (idx, lab, sc, al, cnt) if out is not None else self._trim(counts, cap, (idx, lab, sc, al))

    def match_points(self, points, queries, metric="cosine", out=None):
        """Score the feature voxel that contains each of `points` ((n, 3) float32 torch tensor or numpy array, metres) against `queries`:
        -> (scores [n, Q] f32, weights [n] f32) on the mapper's device; weight 0 and zero scores where query_features would return weight 0.
        out=(scores, weights): preallocated tensors, nothing is allocated."""
        dev = self._cuda
        q, nq, mid = self._queries(queries, metric)
        p = _args.points3(points, dev); n = p.shape[0]
        s, w = _args.outputs(out, (("scores", (n, nq), F32, True, True), ("weights", (n,), F32, True, True)), dev)
        self._around_torch_stream(lambda: self.lib.nvbx_match_points(self._h, ptr(p), n, ptr(q), nq, mid, ptr(s), ptr(w)), order=n > 0)
        self._hold("_keep_mp", [p, q])
        return s, w

    # -- feature segmentation (nvbx_label_components / nvbx_segment_features; SEMANTICS.md "Feature segmentation")
    def component_records(self, capacity):
        """An uninitialised table of `capacity` nvbx_component records for out=: an int32 [capacity, 18] device tensor (72 bytes a record)."""
        return self._torch.empty((int(capacity), COMPONENT_WORDS), dtype=self._torch.int32, device=self._cuda)

    def components_view(self, records, n=None, centroid=True):
        """The fields of a record table (component_records) as device tensors viewing it, trimmed to the first n records: -> Components.  centroid_m
        = (sum / voxels + 0.5) voxel_size in float64 is the one field that is computed (and allocated), None with centroid=False."""
        torch = self._torch
        r = records if n is None else records[:n]
        sums = r[:, 8:14].view(torch.int64)
        voxels = r[:, 1]
        cm = (sums.double() / voxels.double()[:, None] + 0.5) * float(self.params.voxel_size) if centroid else None
        return Components(r[:, 0], voxels, r[:, 2:5], r[:, 5:8], sums, r[:, 14:15].view(torch.float32)[:, 0], r[:, 15:18], cm)

    def _volume(self, a, dtype, what):
        """-> a contiguous [n, 512] tensor of `dtype` on the mapper's device"""
        torch = self._torch
        if not isinstance(a, torch.Tensor):
            a = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        if a.dtype != dtype or a.dim() != 2 or a.shape[1] != 512:
            raise ValueError("%s must be an (n, 512) %s array, got %s %s" % (what, dtype, tuple(a.shape), a.dtype))
        return self._dev(a, dtype)

    @staticmethod
    def _segment_options(connectivity, min_voxels):
        if connectivity not in (6, 26):
            raise ValueError("connectivity must be 6 or 26, got %r" % (connectivity,))
        if int(min_voxels) < 1:
            raise ValueError("min_voxels must be >= 1, got %r" % (min_voxels,))
        return int(connectivity), int(min_voxels)

    def label_components(self, indices, labels, scores=None, connectivity=6, min_voxels=1, out=None):
        """Connected components of a labelled sparse voxel volume of the shape match_features returns: indices (n, 3) int32 distinct block indices,
        labels (n, 512) int32 (< 0: background), scores (n, 512) float32 or None -- torch device tensors or numpy arrays, voxel t = vx 64 + vy 8 + vz.
        Voxels are adjacent across faces (connectivity 6) or faces, edges and corners (26) of the GLOBAL voxel grid, block borders included; a block
        that is not listed separates its sides.  -> (ids [n, 512] i32: the component's row in the table, -1 for background and for components of fewer
        than min_voxels voxels; Components, one row per kept component in no particular order) on the mapper's device.  The table is sized for the
        worst case (n 512 / min_voxels records of 72 bytes), the call waits once for the count.  Reads nothing from the map.
        out=(ids, records | None, count): preallocated tensors (records: component_records(capacity), count: one int64), nothing is allocated and
        nothing waited for: -> (ids, records, count) as given; count (a device tensor) may exceed the capacity, records from the capacity on are
        not written (ids still name them); components_view(records) gives the fields."""
        torch = self._torch
        conn, mv = self._segment_options(connectivity, min_voxels)
        if not isinstance(indices, torch.Tensor):
            indices = torch.from_numpy(np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1, 3)))
        if indices.dtype != torch.int32 or indices.dim() != 2 or indices.shape[1] != 3:
            raise ValueError("indices must be an (n, 3) int32 array, got %s %s" % (tuple(indices.shape), indices.dtype))
        idx = self._dev(indices, torch.int32)
        lab = self._volume(labels, torch.int32, "labels")
        sc = self._volume(scores, torch.float32, "scores") if scores is not None else None
        n = int(idx.shape[0])
        if lab.shape[0] != n or (sc is not None and sc.shape[0] != n):
            raise ValueError("indices, labels and scores differ in their number of blocks")
        if out is None:
            cap = n * 512 // mv
        else:
            cap = int(out[1].shape[0]) if len(out) > 1 and out[1] is not None else 0
        ids, rec, cnt = _args.outputs(out, (("ids", (n, 512), I32, True, True), ("components", (cap, COMPONENT_WORDS), I32, False, True),
                                            ("count", (1,), I64, True, True)), self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_label_components(self._h, ptr(idx), ptr(lab), ptr(sc), n, None, conn, mv, ptr(ids), ptr(rec), cap, ptr(cnt)))
        self._hold("_keep_lc", [idx, lab, sc])      # (the kernels read the volume: it, and an uploaded copy, live until the next call)
        return (ids, rec, cnt) if out is not None else (ids,) + self._trim(cnt, 0, (), rec)

    def segment_features(self, queries, metric="cosine", min_weight=1.0, min_score=None, connectivity=6, min_voxels=1, out=None):
        """From query embeddings to 3-D objects in one call: match_features without the score matrix, then a threshold (where score <
        min_score[label] the voxel becomes background: label -1, score 0; min_score: None, a float for all queries, or a length-Q float32 array /
        device tensor; a NaN drops nothing), then label_components over the result.  -> (indices [n, 3] i32, labels [n, 512] i32, scores [n, 512] f32,
        ids [n, 512] i32, Components) on the mapper's device, trimmed; buffers are sized from block_indices(LAYER_FEATURE) and the worst-case
        component count, the call waits once for the two counts.
        out=(indices, labels, scores, ids, block_count, records | None, component_count): preallocated tensors of any capacities (the counts: one
        int64 each), nothing is allocated -- give min_score as a device tensor -- and nothing waited for: -> the same tuple, untrimmed."""
        torch = self._torch
        dev = self._cuda
        conn, mv = self._segment_options(connectivity, min_voxels)
        q, nq, mid = self._queries(queries, metric)
        if min_score is None:
            thr = None
        elif isinstance(min_score, torch.Tensor):
            thr = self._dev(min_score.reshape(-1), torch.float32)
        else:
            thr = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(min_score, np.float32).reshape(-1), (nq,)))).to(dev)
        if thr is not None and tuple(thr.shape) != (nq,):
            raise ValueError("min_score must be a number or hold one value per query (%d), got %s" % (nq, tuple(thr.shape)))
        vol, cap, counts = _args.sparse_volume(out, dev, lambda: self.num_blocks(LAYER_FEATURE), record_words=COMPONENT_WORDS, min_voxels=mv)
        idx, lab, sc, ids, bcnt, rec, ccnt = vol
        self._around_torch_stream(lambda: self.lib.nvbx_segment_features(
            self._h, ptr(q), nq, mid, float(min_weight), ptr(thr), conn, mv, ptr(idx), ptr(lab), ptr(sc), ptr(ids), cap, ptr(bcnt), ptr(rec),
            int(rec.shape[0]) if rec is not None else 0, ptr(ccnt)))
        self._hold("_keep_sq", [q, thr])      # (the kernels read the queries and thresholds: they live until the next call)
        return vol if out is not None else self._trim(counts, cap, (idx, lab, sc, ids), rec)

    # -- frontiers and view gain (nvbx_find_frontiers / nvbx_frontier_clusters / nvbx_view_gain; SEMANTICS.md "Frontiers and view gain")
    def _frontier_options(self, min_weight, free_distance_m, min_unknown, box_m):
        """-> (min_weight, free_distance_m, min_unknown, box | None); box_m = ((x0, y0, z0), (x1, y1, z1)) in metres, inclusive: the
        voxels that contain the two corners, floor(p / voxel_size) in float32, bound the box (six int32, _box_ptr makes the argument of them)"""
        fd = float(self.params.voxel_size) if free_distance_m is None else float(free_distance_m)
        if int(min_unknown) < 1 or int(min_unknown) > 6:
            raise ValueError("min_unknown must be 1 .. 6, got %r" % (min_unknown,))
        box = None
        if box_m is not None:
            b = np.asarray(box_m, np.float32).reshape(2, 3)
            box = np.ascontiguousarray(np.floor(b / np.float32(self.params.voxel_size)).astype(np.int32).reshape(6))
            if np.any(box[:3] > box[3:]):
                raise ValueError("box_m has min > max on an axis: %r" % (box_m,))
        return float(min_weight), fd, int(min_unknown), box

    @staticmethod
    def _box_ptr(box):
        return box.ctypes.data_as(C.POINTER(C.c_int32)) if box is not None else None

    def _frontier_count(self, mw, fd, mu, box):
        """the number of blocks that hold a frontier voxel: a counting scan (capacity 0), waited for"""
        cnt = self._torch.empty(1, dtype=self._torch.int64, device=self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_find_frontiers(self._h, mw, fd, mu, self._box_ptr(box), None, None, None, 0, ptr(cnt)))
        return int(cnt.item())

    def find_frontiers(self, min_weight=1e-4, free_distance_m=None, min_unknown=1, box_m=None, out=None):
        """The frontier voxels of the TSDF layer: free voxels (weight >= min_weight, distance > free_distance_m; None: one voxel size) with at
        least min_unknown unknown voxels among their six face neighbours, inside box_m (((x0, y0, z0), (x1, y1, z1)) metres; None: everywhere).
        -> (indices [n, 3] i32, labels [n, 512] i32: 0 on a frontier voxel, -1 elsewhere; scores [n, 512] f32: the number of unknown neighbours, 0
        elsewhere; count: one int64) on the mapper's device, one entry per block that holds a frontier voxel in no particular order, voxel
        t = vx 64 + vy 8 + vz -- the shape label_components takes.  Buffers are sized by a counting scan first (the call scans twice and waits once
        for the count; unlike num_blocks that leaves held-back work held back).
        out=(indices, labels, scores | None, count): preallocated tensors of any capacity n_cap, nothing is allocated and nothing waited for:
        -> the same tuple untrimmed; count may exceed n_cap, entries from n_cap on are not written."""
        mw, fd, mu, box = self._frontier_options(min_weight, free_distance_m, min_unknown, box_m)
        vol, cap, counts = _args.sparse_volume(out, self._cuda, lambda: self._frontier_count(mw, fd, mu, box), scores_required=False)
        idx, lab, sc, cnt = vol
        self._around_torch_stream(lambda: self.lib.nvbx_find_frontiers(self._h, mw, fd, mu, self._box_ptr(box), ptr(idx), ptr(lab), ptr(sc), cap, ptr(cnt)))
        return vol if out is not None else self._trim(counts, cap, (idx, lab, sc)) + (cnt,)

    def frontier_clusters(self, min_weight=1e-4, free_distance_m=None, min_unknown=1, box_m=None, connectivity=26, min_voxels=1, out=None):
        """From the map to exploration goals in one call: find_frontiers, then label_components over the result.  -> (indices [n, 3] i32,
        labels [n, 512] i32, scores [n, 512] f32, ids [n, 512] i32, Components) on the mapper's device, trimmed, as segment_features returns: a
        component's centroid_m is a goal, voxels the frontier's size, peak_score / peak_xyz its most open voxel.  Buffers are sized by a counting
        scan first and for the worst-case component count; the call waits for that count and once for the two counts of the result.
        out=(indices, labels, scores | None, ids, block_count, records | None, component_count): preallocated tensors of any capacities (the counts:
        one int64 each), nothing is allocated and nothing waited for: -> the same tuple, untrimmed."""
        conn, mv = self._segment_options(connectivity, min_voxels)
        mw, fd, mu, box = self._frontier_options(min_weight, free_distance_m, min_unknown, box_m)
        vol, cap, counts = _args.sparse_volume(out, self._cuda, lambda: self._frontier_count(mw, fd, mu, box), scores_required=False,
                                               record_words=COMPONENT_WORDS, min_voxels=mv)
        idx, lab, sc, ids, bcnt, rec, ccnt = vol
        self._around_torch_stream(lambda: self.lib.nvbx_frontier_clusters(
            self._h, mw, fd, mu, self._box_ptr(box), conn, mv, ptr(idx), ptr(lab), ptr(sc), ptr(ids), cap, ptr(bcnt), ptr(rec),
            int(rec.shape[0]) if rec is not None else 0, ptr(ccnt)))
        return vol if out is not None else self._trim(counts, cap, (idx, lab, sc, ids), rec)

    def view_gain(self, poses, cam, subsampling=None, max_range_m=None, min_weight=1e-4, free_distance_m=None, out=None):
        """How much unseen space each candidate pose would look into: poses (n, 4, 4) or (n, 16) float32 T_L_C (torch device tensor or numpy
        array), the rays of render() for `cam` at `subsampling`, walked one voxel size per sample up to max_range_m (None: the mapper's
        sphere_tracing_* parameters).  -> int32 [n, 4] on the mapper's device: rays, unknown_samples, free_samples, rays_hit per pose; a pose
        that is not finite or out of range has rays = -1 and zeros.  Samples count voxels along rays, not distinct voxels.
        out: a preallocated int32 [n, 4] tensor, nothing is allocated."""
        torch = self._torch
        k = self._cam(cam)
        if not isinstance(poses, torch.Tensor):
            poses = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 16)))
        if poses.dtype != torch.float32 or poses.numel() % 16:
            raise ValueError("poses must be (n, 4, 4) float32, got %s %s" % (tuple(poses.shape), poses.dtype))
        p = self._dev(poses.reshape(-1, 16), torch.float32)
        n = int(p.shape[0])
        s = _args.subsampling_arg(subsampling)
        mw, fd, _, _ = self._frontier_options(min_weight, free_distance_m, 1, None)
        g, = _args.outputs(None if out is None else (out,), (("gains", (n, 4), I32, True, True),), self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_view_gain(
            self._h, ptr(p), n, C.byref(k), s, float(max_range_m) if max_range_m is not None else 0.0, mw, fd, ptr(g)), order=n > 0)
        self._hold("_keep_vg", [p])      # (the kernel reads the poses: they, and an uploaded copy, live until the next call)
        return g

    # -- change detection (nvbx_find_changes / nvbx_change_clusters; SEMANTICS.md "Change detection")
    def _change_options(self, ref, T_M_R, min_weight, ref_min_weight, free_distance_m, occupied_distance_m, sampling, box_m):
        """-> (pose array, nvbx_change_options, box | None); free_distance_m None: 0, the library's "one voxel size"; box_m as find_frontiers takes it"""
        if not isinstance(ref, Mapper):
            raise TypeError("the reference must be a Mapper")
        if sampling not in CHANGE_SAMPLING:
            raise ValueError("sampling must be 'trilinear' or 'nearest', got %r" % (sampling,))
        o = _args.struct_options(_lib.ChangeOptions, self.lib.nvbx_default_change_options, dict(
            min_weight=float(min_weight), ref_min_weight=float(ref_min_weight), free_distance_m=0.0 if free_distance_m is None else float(free_distance_m),
            occupied_distance_m=float(occupied_distance_m), sampling=CHANGE_SAMPLING[sampling]), "change")
        _, _, _, box = self._frontier_options(min_weight, None, 1, box_m)
        return self._T(T_M_R), o, box

    def _change_count(self, ref, T, o, box):
        """the number of blocks that hold a labelled voxel: a counting scan (capacity 0, no result record), waited for"""
        cnt = self._torch.empty(1, dtype=self._torch.int64, device=self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_find_changes(self._h, ref._h, _np_ptr(T), C.byref(o), self._box_ptr(box), None, None, None, 0, ptr(cnt), None))
        return int(cnt.item())

    @staticmethod
    def _change_out(out, n):
        """out=(the n tensors of the volume ..., result buffer | None) -> (the volume's tensors, the result buffer)"""
        if out is None:
            return None, None
        out = tuple(out)
        if len(out) != n + 1:
            raise ValueError("out must hold %d entries (the volume's %d tensors and a result buffer or None), got %d" % (n + 1, n, len(out)))
        return out[:n], out[n]

    def find_changes(self, ref, T_M_R, min_weight=1e-4, ref_min_weight=1e-4, free_distance_m=None, occupied_distance_m=0.0, sampling="trilinear",
                     box_m=None, out=None):
        """What differs between this map ("now") and `ref` ("before") under p_M = T_M_R p_R (row-major 4 x 4).  A voxel here is observed with
        weight >= min_weight, free with distance > free_distance_m (None: one voxel size), occupied with distance <= occupied_distance_m; its
        sample of `ref` ("trilinear": the point query's rule over eight corners of weight >= ref_min_weight; "nearest": the voxel that holds the
        position) is classified by the same thresholds.  Label 0 (CHANGE_APPEARED): occupied here, free there; label 1 (CHANGE_REMOVED): free
        here, occupied there; inside box_m (as find_frontiers takes it; None: everywhere).
        -> (indices [n, 3] i32, labels [n, 512] i32: 0 / 1 / -1, scores [n, 512] f32: |d - d_ref| on a labelled voxel, count: one int64,
        ChangeResult) on the mapper's device, one entry per block with a labelled voxel in no particular order -- the shape label_components
        takes.  Buffers are sized by a counting scan first (the call scans twice and waits once for the count).  Neither map is written; the
        launches run on this mapper's stream behind everything enqueued on `ref`'s.
        out=(indices, labels, scores | None, count, result | None): preallocated tensors of any capacity n_cap (result: a uint8 tensor of
        CHANGE_RESULT_BYTES bytes), nothing is allocated and nothing waited for: -> the same tensors untrimmed and the ChangeResult (None
        without a buffer); count may exceed n_cap, entries from n_cap on are not written."""
        T, o, box = self._change_options(ref, T_M_R, min_weight, ref_min_weight, free_distance_m, occupied_distance_m, sampling, box_m)
        vout, rbuf = self._change_out(out, 4)
        vol, cap, counts = _args.sparse_volume(vout, self._cuda, lambda: self._change_count(ref, T, o, box), scores_required=False)
        idx, lab, sc, cnt = vol
        buf = _args.result_buffer(rbuf, CHANGE_RESULT_BYTES, self._cuda) if out is None or rbuf is not None else None
        self._around_torch_stream(lambda: self.lib.nvbx_find_changes(
            self._h, ref._h, _np_ptr(T), C.byref(o), self._box_ptr(box), ptr(idx), ptr(lab), ptr(sc), cap, ptr(cnt), ptr(buf)))
        res = ChangeResult(buf) if buf is not None else None
        return vol + (res,) if out is not None else self._trim(counts, cap, (idx, lab, sc)) + (cnt, res)

    def change_clusters(self, ref, T_M_R, min_weight=1e-4, ref_min_weight=1e-4, free_distance_m=None, occupied_distance_m=0.0, sampling="trilinear",
                        box_m=None, connectivity=26, min_voxels=8, out=None):
        """From two maps to the objects that appeared and the objects that are gone in one call: find_changes, then label_components over the
        result.  -> (indices [n, 3] i32, labels [n, 512] i32, scores [n, 512] f32, ids [n, 512] i32, Components, ChangeResult) on the mapper's
        device, trimmed, as frontier_clusters returns: a component of label 0 is an object that appeared, one of label 1 an object that is
        gone, peak_score its largest distance change.  Buffers are sized by a counting scan first and for the worst-case component count.
        out=(indices, labels, scores | None, ids, block_count, records | None, component_count, result | None): preallocated tensors of any
        capacities, nothing is allocated and nothing waited for: -> the same tensors untrimmed and the ChangeResult (None without a buffer)."""
        conn, mv = self._segment_options(connectivity, min_voxels)
        T, o, box = self._change_options(ref, T_M_R, min_weight, ref_min_weight, free_distance_m, occupied_distance_m, sampling, box_m)
        vout, rbuf = self._change_out(out, 7)
        vol, cap, counts = _args.sparse_volume(vout, self._cuda, lambda: self._change_count(ref, T, o, box), scores_required=False,
                                               record_words=COMPONENT_WORDS, min_voxels=mv)
        idx, lab, sc, ids, bcnt, rec, ccnt = vol
        buf = _args.result_buffer(rbuf, CHANGE_RESULT_BYTES, self._cuda) if out is None or rbuf is not None else None
        self._around_torch_stream(lambda: self.lib.nvbx_change_clusters(
            self._h, ref._h, _np_ptr(T), C.byref(o), self._box_ptr(box), conn, mv, ptr(idx), ptr(lab), ptr(sc), ptr(ids), cap, ptr(bcnt), ptr(rec),
            int(rec.shape[0]) if rec is not None else 0, ptr(ccnt), ptr(buf)))
        res = ChangeResult(buf) if buf is not None else None
        return vol + (res,) if out is not None else self._trim(counts, cap, (idx, lab, sc, ids), rec) + (res,)

    # -- cost field and paths (nvbx_cost_field / nvbx_trace_paths; SEMANTICS.md "Cost field and paths")
    def cost_options(self, **kw):
        """nvbx_cost_options: the library's defaults with the given fields replaced (robot_radius_m, inflation_radius_m, penalty_per_m,
        unknown_value, max_penalty, unknown_penalty, allow_unknown)."""
        return _args.struct_options(_lib.CostOptions, self.lib.nvbx_default_cost_options, kw, "cost")

    def _cost_to_go(self, fn, grid, coerce, sources, name, out, accepted, options):
        """cost_field / cost_volume: fn = the library's call, grid = the image or volume, checked; coerce = the coercer of `sources`, called `name`"""
        torch = self._torch
        shape = tuple(int(v) for v in grid.shape)
        o = self.cost_options(**options)
        src = coerce(sources, self._cuda, name)
        cost, acc = _args.outputs((out, accepted) if out is not None or accepted is not None else None,
                                  (("cost", shape, I32, False, True), ("accepted", (1,), I32, False, False)), self._cuda)
        if cost is None:
            cost = torch.empty(shape, dtype=torch.int32, device=self._cuda)
        self._around_torch_stream(lambda: fn(self._h, ptr(grid, collapse=False), *shape, C.byref(o), ptr(src), int(src.shape[0]), ptr(cost, collapse=False), ptr(acc)))
        return cost

    def _descend(self, fn, grid, word, dims, field, coerce, starts, name, capacity, out, options, slot):
        """trace_paths / trace_paths_3d: as _cost_to_go; word and dims = what messages call the grid and its shape, slot = where _hold keeps the inputs"""
        shape = tuple(int(v) for v in grid.shape)
        o = self.cost_options(**options)
        f = _args.image(field, self._cuda, self._torch.int32, "field", dims, convert=False)
        if tuple(f.shape) != shape:
            raise ValueError("field must have the %s's shape %s, got %s" % (word, shape, tuple(f.shape)))
        st = coerce(starts, self._cuda, name)
        n, cap = int(st.shape[0]), int(capacity)
        if cap < 0:
            raise ValueError("capacity must be >= 0")
        paths, lengths = _args.outputs(out, (("paths", (n, cap, len(shape)), I32, True, True), ("lengths", (n,), I32, True, True)), self._cuda)
        self._around_torch_stream(lambda: fn(self._h, ptr(grid, collapse=False), *shape, C.byref(o), ptr(f, collapse=False), ptr(st), n, ptr(paths, collapse=False), cap, ptr(lengths)),
                                  order=n > 0)
        self._hold(slot, [grid, f, st])      # (the kernel reads them: they, and uploaded copies, live until the next call)
        return paths, lengths

    def cost_field(self, image_dev, sources_rc, out=None, accepted=None, **options):
        """The integer cost-to-go field over a distance image (esdf_slice_image_device, esdf_slice_image_combined, or any (rows, cols) float32
        image of that form) from the source pixels sources_rc ((n, 2) int32 (row, col), torch device tensor or numpy array; slice_pixels makes
        them from metres): -> int32 [rows, cols] on the mapper's device, 0 at an accepted source, COST_UNREACHED where no move sequence leads
        and on every pixel that is not traversable.  A source outside the image or on such a pixel is ignored.  options: see cost_options --
        unknown_value must be the one the image was sliced with.  The call waits for the device (between batches of relaxation rounds) and
        returns with the field complete; it reads the image only.  out: a preallocated int32 [rows, cols] tensor; accepted: an int32 [1]
        device tensor that receives the number of accepted sources."""
        return self._cost_to_go(self.lib.nvbx_cost_field, self._image(image_dev, "image"), _args.pixels2, sources_rc, "sources_rc", out, accepted, options)

    def trace_paths(self, image_dev, field, starts_rc, capacity, out=None, **options):
        """The paths that descend `field` (cost_field of this image and these options) from the pixels starts_rc ((n, 2) int32 (row, col)):
        -> (paths int32 [n, capacity, 2] of (row, col), lengths int32 [n]) on the mapper's device.  A path runs from its start to the first
        pixel of cost 0, both included; lengths[i] is its number of pixels, also beyond `capacity` (pixels from the capacity on are not
        written; rows past a path's end are left as they were), 0 for a start outside the image or unreached, -1 where the field does not
        belong to the image.  Asynchronous.  out=(paths, lengths): preallocated tensors, nothing is allocated."""
        return self._descend(self.lib.nvbx_trace_paths, self._image(image_dev, "image"), "image", "(rows, cols)", field, _args.pixels2, starts_rc, "starts_rc",
                             capacity, out, options, "_keep_tp")

    def slice_pixels(self, points_xy, aabb):
        """Metres -> pixels of the ESDF slice image that came with `aabb` (esdf_slice_image_device / esdf_slice_image / ..._combined):
        points_xy (n, 2) or (n, 3) (z ignored) -> int32 numpy [n, 2] of (row, col); col = floor(x / voxel_size) - lrint(aabb[0] / voxel_size),
        row likewise with y and aabb[1], in float32 (the slice's AABB starts at a block's min corner, so the second term is a whole number of
        voxels).  A point outside the image gives a pixel outside it, which cost_field and trace_paths ignore.  No kernel, host only."""
        p = np.asarray(points_xy, np.float32)
        p = p.reshape(-1, p.shape[-1] if p.ndim > 1 else 2)
        if p.shape[1] not in (2, 3):
            raise ValueError("points_xy must be (n, 2) or (n, 3), got %s" % (p.shape,))
        vs = np.float32(self.params.voxel_size)
        a = np.asarray(aabb, np.float32).reshape(-1)
        col = np.floor(p[:, 0] / vs).astype(np.int64) - np.int64(np.rint(a[0] / vs))
        row = np.floor(p[:, 1] / vs).astype(np.int64) - np.int64(np.rint(a[1] / vs))
        return np.stack([row, col], 1).astype(np.int32)

    # -- cost volume and 3-D paths (nvbx_cost_volume / nvbx_trace_paths_3d; SEMANTICS.md "Cost volume and 3-D paths")
    def esdf_dense_grid_device(self, min_vox, size_vox, default_value, out=None):
        """The device-tensor form of esdf_dense_grid: the ESDF distances of the voxel box min_vox .. min_vox + size_vox (global voxel
        coordinates) -> float32 [nx, ny, nz] on the mapper's device, default_value where nothing is stored: the volume cost_volume takes, with
        default_value = its unknown_value.  No host copy and no synchronise: ordered on the streams like the other reader calls.
        out: a preallocated float32 [nx, ny, nz] tensor, nothing is allocated."""
        mn = np.ascontiguousarray(np.asarray(min_vox, np.int32).reshape(3)); sz = np.ascontiguousarray(np.asarray(size_vox, np.int32).reshape(3))
        if (sz <= 0).any():
            raise ValueError("size_vox must be > 0 on every axis, got %s" % (sz.tolist(),))
        grid, = _args.outputs(None if out is None else (out,), (("grid", tuple(int(v) for v in sz), F32, True, True),), self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_esdf_dense_grid(self._h, _np_ptr(mn), _np_ptr(sz), float(default_value), ptr(grid)))
        return grid

    def _dense_volume(self, volume_dev):
        return _args.image(volume_dev, self._cuda, self._torch.float32, "volume", "(nx, ny, nz)")

    def cost_volume(self, volume_dev, sources_xyz, out=None, accepted=None, **options):
        """The integer cost-to-go field over a distance volume (esdf_dense_grid_device with default_value = unknown_value, or any (nx, ny, nz)
        float32 volume of that form) over 26-connected moves from the source voxels sources_xyz ((n, 3) int32 (x, y, z) offsets in the box,
        torch device tensor or numpy array; volume_voxels makes them from metres): -> int32 [nx, ny, nz] on the mapper's device, 0 at an
        accepted source, COST_UNREACHED where no move sequence leads and on every voxel that is not traversable.  A source outside the box or
        on such a voxel is ignored.  options: see cost_options.  The call waits for the device (between batches of relaxation rounds) and
        returns with the field complete; it reads the volume only.  out: a preallocated int32 [nx, ny, nz] tensor; accepted: an int32 [1]
        device tensor that receives the number of accepted sources."""
        return self._cost_to_go(self.lib.nvbx_cost_volume, self._dense_volume(volume_dev), _args.voxels3, sources_xyz, "sources_xyz", out, accepted, options)

    def trace_paths_3d(self, volume_dev, field, starts_xyz, capacity, out=None, **options):
        """The paths that descend `field` (cost_volume of this volume and these options) from the voxels starts_xyz ((n, 3) int32 (x, y, z)):
        -> (paths int32 [n, capacity, 3] of (x, y, z), lengths int32 [n]) on the mapper's device.  A path runs from its start to the first
        voxel of cost 0, both included; lengths[i] is its number of voxels, also beyond `capacity` (voxels from the capacity on are not
        written; rows past a path's end are left as they were), 0 for a start outside the box or unreached, -1 where the field does not
        belong to the volume.  Asynchronous.  out=(paths, lengths): preallocated tensors, nothing is allocated."""
        return self._descend(self.lib.nvbx_trace_paths_3d, self._dense_volume(volume_dev), "volume", "(nx, ny, nz)", field, _args.voxels3, starts_xyz, "starts_xyz",
                             capacity, out, options, "_keep_tp3")

    def volume_voxels(self, points_xyz, min_vox):
        """Metres -> voxels of the box that starts at min_vox (esdf_dense_grid_device's): points_xyz (n, 3) -> int32 numpy [n, 3] of (x, y, z)
        offsets; per axis floor(p / voxel_size) - min_vox, in float32.  A point outside the box gives a voxel outside it, which cost_volume and
        trace_paths_3d ignore.  No kernel, host only."""
        p = np.asarray(points_xyz, np.float32).reshape(-1, 3)
        vs = np.float32(self.params.voxel_size)
        return (np.floor(p / vs).astype(np.int64) - np.asarray(min_vox, np.int64).reshape(1, 3)).astype(np.int32)

    # -- elevation and traversability (nvbx_elevation_map / nvbx_traversability; SEMANTICS.md "Elevation and traversability")
    def terrain_options(self, **kw):
        """nvbx_terrain_options: the library's defaults with the given fields replaced (max_step_m, max_slope_tan, unknown_value, min_known,
        void_is_hazard, distance_radius_px)."""
        return _args.struct_options(_lib.TerrainOptions, self.lib.nvbx_default_terrain_options, kw, "terrain")

    def elevation_box(self, aabb, z_min_m, z_max_m, rows=None, cols=None):
        """The voxel box of an elevation image over `aabb` ((min x, y, z, max x, y, z) metres, as the slice calls return it) and the band
        z_min_m .. z_max_m: -> (x0, y0, rows, cols, z_lo, z_hi) for elevation_map, x0 = lrint(aabb[0] / voxel_size), y0 likewise with
        aabb[1], rows = lrint(aabb[4] / voxel_size) - y0 and cols = lrint(aabb[3] / voxel_size) - x0 unless given, z = floor(z_m /
        voxel_size), all in float32.  Over a slice's AABB the image lies pixel for pixel on the slice image's grid (the AABB runs from a
        block's min corner to a block's max corner), and slice_pixels serves both.  No kernel, host only."""
        vs = np.float32(self.params.voxel_size)
        a = np.asarray(aabb, np.float32).reshape(-1)
        if a.size != 6:
            raise ValueError("aabb must hold (min x, y, z, max x, y, z), got %d numbers" % a.size)
        x0, y0 = int(np.rint(a[0] / vs)), int(np.rint(a[1] / vs))
        rows = int(np.rint(a[4] / vs)) - y0 if rows is None else int(rows)
        cols = int(np.rint(a[3] / vs)) - x0 if cols is None else int(cols)
        z_lo, z_hi = (int(np.floor(np.float32(z) / vs)) for z in (z_min_m, z_max_m))
        return x0, y0, rows, cols, z_lo, z_hi

    def elevation_map(self, x0, y0, rows, cols, z_lo, z_hi, min_weight=1e-4, unknown_value=1000.0, out=None):
        """Per-column ground height and status of the TSDF layer over the voxel columns gx = x0 + col, gy = y0 + row and the band
        z_lo <= gz <= z_hi (global voxel coordinates; elevation_box makes them from metres): -> (height float32 [rows, cols], status uint8
        [rows, cols]) on the mapper's device.  status: ELEV_UNKNOWN (nothing observed in the band), ELEV_SURFACE (the topmost solid voxel
        has an observed, free voxel above it inside the band: height = the interpolated zero crossing in metres), ELEV_BLOCKED (solid up to
        the band's top or with unobserved space above), ELEV_VOID (observed, nothing solid); height is unknown_value wherever the status is
        not SURFACE.  Asynchronous, reads TSDF voxels only, held-back work stays held back.  out=(height, status): preallocated tensors,
        nothing is allocated."""
        rows, cols = int(rows), int(cols)
        h, s = _args.outputs(out, (("height", (max(rows, 0), max(cols, 0)), F32, True, True), ("status", (max(rows, 0), max(cols, 0)), U8, True, True)), self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_elevation_map(self._h, int(x0), int(y0), rows, cols, int(z_lo), int(z_hi), float(min_weight),
                                                                      float(unknown_value), ptr(h, collapse=False), ptr(s, collapse=False)))
        return h, s

    def traversability(self, height, status, step=False, slope=False, distance=True, out=None, **options):
        """Classes and the distance to the nearest hazard from a height / status image pair (elevation_map's, or any float32 / uint8 pair of
        one shape): -> dict of tensors [rows, cols] on the mapper's device: "class" uint8 (TERRAIN_UNKNOWN / TERRAIN_OK / TERRAIN_HAZARD),
        and where asked for "step" float32 (the largest height difference to a known 8-neighbour, metres), "slope2" float32 (the squared
        gradient, tan^2) and "distance" float32 (metres to the nearest HAZARD pixel within distance_radius_px; voxel_size x (radius + 1)
        if there is none, 0 on a hazard, unknown_value on an UNKNOWN pixel: the image cost_field takes).  options: see terrain_options.
        Asynchronous; the map is not read.  out=(class, step | None, slope2 | None, distance | None): preallocated tensors decide what is
        written (the three flags are not looked at), nothing is allocated."""
        torch = self._torch
        h = self._image(height, "height")
        s = self._image(status, "status", torch.uint8)
        rows, cols = int(h.shape[0]), int(h.shape[1])
        if tuple(s.shape) != (rows, cols):
            raise ValueError("status must have the height image's shape %s, got %s" % ((rows, cols), tuple(s.shape)))
        o = self.terrain_options(**options)
        cl, st, sl, di = _args.outputs(out, (("class", (rows, cols), U8, True, True), ("step", (rows, cols), F32, False, bool(step)),
                                             ("slope2", (rows, cols), F32, False, bool(slope)), ("distance", (rows, cols), F32, False, bool(distance))), self._cuda)
        self._around_torch_stream(lambda: self.lib.nvbx_traversability(self._h, ptr(h, collapse=False), ptr(s, collapse=False), rows, cols, C.byref(o),
                                                                       ptr(cl, collapse=False), ptr(st), ptr(sl), ptr(di)))
        self._hold("_keep_tr", [h, s])      # (the kernels read them: they, and uploaded copies, live until the next call)
        return {k: v for k, v in (("class", cl), ("step", st), ("slope2", sl), ("distance", di)) if v is not None}

    def mesh(self):
        """Mesh of the last update_color_mesh: dict block index tuple -> dict(vertices, normals, colors, triangles)."""
        nb, nv, nt = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.nvbx_mesh_sizes(self._h, C.byref(nb), C.byref(nv), C.byref(nt)))
        nb, nv, nt = nb.value, nv.value, nt.value
        idx = np.zeros((max(nb, 1), 3), np.int32); vo = np.zeros(nb + 1, np.int32); to = np.zeros(nb + 1, np.int32)
        v = np.zeros((max(nv, 1), 3), np.float32); n = np.zeros((max(nv, 1), 3), np.float32)
        c = np.zeros((max(nv, 1), 4), np.uint8); t = np.zeros((max(nt, 1), 3), np.int32)
        self._check(self.lib.nvbx_mesh_copy(self._h, _np_ptr(idx), _np_ptr(vo), _np_ptr(to), _np_ptr(v), _np_ptr(n), _np_ptr(c), _np_ptr(t)))
        out = {}
        for i in range(nb):
            out[tuple(int(q) for q in idx[i])] = dict(vertices=v[vo[i]:vo[i + 1]], normals=n[vo[i]:vo[i + 1]],
                                                      colors=c[vo[i]:vo[i + 1]], triangles=t[to[i]:to[i + 1]])
        return out

    # -- multi-GPU, one fused map: measurement exchange (nvbx_measure_depth / nvbx_apply_measurements; dist.MeasurementFusion)
    MEAS_BLOCK_BYTES = 4112

    def measure_depth(self, depth, T_L_C, cam, out_blocks, out_count):
        """This rank's camera -> measurement records into caller-owned device tensors: out_blocks uint8 [capacity, 4112], out_count int32 [1]."""
        d = self._image(depth)
        group, keep = _args.frame(d, T_L_C, _args.camera(cam))
        self._check(self.lib.nvbx_measure_depth(self._h, *group, ptr(out_blocks), ptr(out_count), int(out_blocks.shape[0])))
        self._hold("_keep", [d])

    def apply_measurements(self, gathered, counts, owner_mod=0, owner_rank=0):
        """gathered uint8 [world, stride, 4112], counts int32 [world] (device): every camera's measurements applied in rank order."""
        self._check(self.lib.nvbx_apply_measurements(self._h, ptr(gathered), ptr(counts), int(gathered.shape[0]), int(gathered.shape[1]),
                                                     int(owner_mod), int(owner_rank)))

    # -- multi-GPU hooks
    def esdf_dirty_list(self, idx_out, count_out):
        """Write the Index3D list [cap,3] int32 + count [1] int32 of TSDF blocks dirtied since the last updateEsdf
        into caller-owned device tensors (async)."""
        self._check(self.lib.nvbx_esdf_dirty_list(self._h, ptr(idx_out), ptr(count_out), int(idx_out.shape[0])))

    def set_view_export(self, packed_tensor):
        """Register (or, with None, unregister) an int32 device tensor [1 + cap, 3]: every following integrate_depth writes the indices
        of the blocks it updates into it (row 0 = count) from inside its own launch.  The tensor must stay alive while registered."""
        self._check(self.lib.nvbx_set_view_export(self._h, ptr(packed_tensor), int(packed_tensor.shape[0]) - 1 if packed_tensor is not None else 0))
        self._view_export = packed_tensor      # (the one it replaces is let go of only now: it stayed registered until the call)

    def mark_esdf_dirty(self, idx_tensor, count_tensor, max_count):
        # (a non-collapsing pointer: the entry takes max_count 0 with an empty list, but not a NULL one)
        self._check(self.lib.nvbx_mark_esdf_dirty(self._h, ptr(idx_tensor, collapse=False), ptr(count_tensor), int(max_count)))

    def mark_esdf_dirty_gathered(self, gathered, world, self_rank, max_count, deferred=False):
        """gathered: int32 device tensor [world, 1 + max_count, 3] (row 0 = count); one launch for all peers -- or, deferred,
        no launch at all: the next integrate_color carries it (the tensor must stay alive and unchanged until then)."""
        fn = self.lib.nvbx_mark_esdf_dirty_gathered_deferred if deferred else self.lib.nvbx_mark_esdf_dirty_gathered
        self._check(fn(self._h, ptr(gathered), int(world), int(self_rank), int(max_count)))

    # -- instrumentation
    def set_profiling(self, enable):
        self._check(self.lib.nvbx_set_profiling(self._h, int(enable)))

    def profile(self):
        import json
        buf = C.create_string_buffer(1 << 16)
        self._check(self.lib.nvbx_get_profile(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())
