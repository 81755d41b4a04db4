/*
 * nvblox_hip.h -- C-ABI of libnvblox_hip.so, the MI355X (gfx950) implementation of the nvblox_core hot path
 * that isaac_ros_nvblox reaches through nvblox::MultiMapper / nvblox::Mapper / nvblox::EsdfSlicer.
 *
 * Every entry point names the reference call site it serves (paths relative to the reference root).  The C++ classes
 * in include/nvblox/ are inline wrappers over these functions, so nvblox_ros links against this library unchanged at
 * the call-expression level (INTEGRATION.md shows the CMake swap).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.  `*_dev` pointers are device (HBM) addresses on the mapper's
 *     GPU, everything else is host memory.
 *   - all work is enqueued on the mapper's stream (the reference is single-caller, stream-ordered:
 *     nvblox_ros/src/lib/nvblox_node.cpp:99,456-459).  Functions that return host-visible results synchronise that
 *     stream; the integrate / update calls do not.  (One piece of work may be enqueued one call late: see nvbx_update_esdf.)
 *   - return value: 0 = ok, negative = error (NVBX_E_*).  Nothing throws across the boundary; device faults are
 *     reported through nvbx_last_error().  (Reference convention: bool for I/O, CHECK/abort for programmer errors,
 *     checkCudaErrors -> exit(99): nvblox_ros_common/src/check_cuda_errors.cpp:24-32.)
 *   - transforms are row-major 4x4 float (T_L_C: camera -> layer/world), cameras are (fu,fv,cu,cv,width,height) as in
 *     conversions/image_conversions.cpp:27-32.
 *   - voxel blocks are 8x8x8, block copies use the reference's voxel structs and its linear order z + 8*y + 64*x
 *     (nvblox_ros/src/lib/layer_publishing.cpp:335,501).
 */
#ifndef NVBLOX_HIP_H_
#define NVBLOX_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NVBX_OK 0
#define NVBX_E_INVALID (-1)   /* bad argument */
#define NVBX_E_DEVICE (-2)    /* HIP runtime error, see nvbx_last_error() */
#define NVBX_E_CAPACITY (-3)  /* block pool / arena / window capacity exceeded */
#define NVBX_E_NOTFOUND (-4)
#define NVBX_E_IO (-5)        /* file could not be opened / read / written, or is not a map file */

/* layer selectors (bit mask), mirrors the reference's LayerType usage in layer_publishing.cpp:675-826 */
#define NVBX_LAYER_TSDF 1u
#define NVBX_LAYER_COLOR 2u
#define NVBX_LAYER_ESDF 4u
#define NVBX_LAYER_MESH 8u
#define NVBX_LAYER_OCCUPANCY 16u   /* occupancy mappers only; shares the projective voxel pool with TSDF */
#define NVBX_LAYER_FREESPACE 32u   /* projective_layer_type 2 only */
#define NVBX_LAYER_FEATURE 64u     /* after nvbx_enable_features; listed by nvbx_block_indices, read by nvbx_get_feature_blocks / nvbx_query_features */

typedef struct nvbx_mapper nvbx_mapper; /* replaces nvblox::Mapper (one per GPU / stream) */

typedef struct { int32_t x, y, z; } nvbx_index3d;                      /* nvblox::Index3D; addressable range [-2^20, 2^20) per axis (419 km at 0.05 m voxels): poses / indices beyond it are refused with NVBX_E_INVALID */
typedef struct { float fu, fv, cu, cv; int32_t width, height; } nvbx_camera; /* nvblox::Camera */

/* Voxel structs as the reference's consumers read them. */
typedef struct { float distance, weight; } nvbx_tsdf_voxel;            /* layer_publishing.cpp:111,179 */
/* FreespaceVoxel: layer_publishing.cpp:129-137,158-165 (consecutive_occupancy_duration_ms, is_high_confidence_freespace) */
typedef struct { int64_t last_occupied_timestamp_ms; int64_t consecutive_occupancy_duration_ms; uint8_t is_high_confidence_freespace; uint8_t initialized; uint8_t pad[6]; } nvbx_freespace_voxel;
typedef struct { float log_odds; } nvbx_occupancy_voxel;                /* layer_publishing.cpp:140-154 (OccupancyVoxel::log_odds) */
typedef struct { uint8_t r, g, b, pad; float weight; } nvbx_color_voxel; /* layer_publishing.cpp:62-76; Color = 3 x u8 */
typedef struct {                                                        /* esdf_and_gradients_conversions.cu:33-44 */
  float squared_distance_vox; int32_t parent_direction[3]; uint8_t is_inside, observed, is_site, pad;
} nvbx_esdf_voxel;

/* WeightingFunctionType, nvblox_ros/src/lib/mapper_initialization.cpp:31-42 */
enum {
  NVBX_WEIGHT_CONSTANT = 0, NVBX_WEIGHT_CONSTANT_DROPOFF = 1, NVBX_WEIGHT_INVERSE_SQUARE = 2,
  NVBX_WEIGHT_INVERSE_SQUARE_DROPOFF = 3, NVBX_WEIGHT_INVERSE_SQUARE_TSDF_DISTANCE_PENALTY = 4,
  NVBX_WEIGHT_LINEAR_WITH_MAX = 5
};

/* The MapperParams fields that reach this path (mapper_initialization.cpp:231-466, values fuser.yaml:24-42). */
typedef struct {
  float voxel_size;                       /* node param voxel_size, node_params.hpp:84 */
  float max_integration_distance_m;       /* projective_integrator_max_integration_distance_m */
  float truncation_distance_vox;          /* projective_integrator_truncation_distance_vox */
  float max_weight;                       /* projective_integrator_max_weight */
  int32_t weighting_mode;                 /* projective_integrator_weighting_mode */
  int32_t raycast_subsampling_factor;     /* raycast_subsampling_factor */
  float esdf_min_weight;                  /* esdf_integrator_min_weight */
  float esdf_max_site_distance_vox;       /* esdf_integrator_max_site_distance_vox */
  float esdf_max_distance_m;              /* esdf_integrator_max_distance_m: the ESDF cut-off radius.  esdf_max_distance_m / voxel_size (in float) must
                                             be below 64 voxels: nvbx_update_esdf fails with NVBX_E_INVALID otherwise, in both ESDF modes, and leaves the
                                             map as it is.  Below one voxel only the sites themselves have a distance (0); every other voxel reads the
                                             cut-off value (esdf_max_distance_m / voxel_size)^2 -- SEMANTICS.md "Limits of the cut-off radius" */
  float esdf_slice_height;                /* esdf_slice_height */
  float esdf_slice_min_height;            /* esdf_slice_min_height */
  float esdf_slice_max_height;            /* esdf_slice_max_height */
  float mesh_min_weight;                  /* mesh_integrator_min_weight */
  int32_t mesh_weld_vertices;             /* mesh_integrator_weld_vertices */
  int32_t sphere_tracing_subsampling;     /* colour integrator synthetic-depth subsampling (4) */
  int32_t sphere_tracing_max_steps;       /* 100 */
  float sphere_tracing_max_ray_length_m;  /* 15 */
  float sphere_tracing_surface_eps_vox;   /* 0.1 */
  float tsdf_decay_factor;                /* tsdf_decay_factor */
  float tsdf_decayed_weight_threshold;    /* tsdf_decayed_weight_threshold */
  int32_t esdf_site_rule;                 /* 0: inside && |d| <= max_site_distance (default); 1: |d| <= max_site_distance */
  int32_t depth_interp_nearest;           /* 0: bilinear with validity (default); 1: nearest */
  float lidar_max_integration_distance_m; /* lidar_projective_integrator_max_integration_distance_m (mapper_initialization.cpp:271-276) */
  float lidar_linear_interpolation_max_allowable_difference_vox;    /* [U] 2.0: bilinear taps must agree within this */
  float lidar_nearest_interpolation_max_allowable_dist_to_ray_vox;  /* [U] 0.5: nearest-beam fallback acceptance */
  int32_t workspace_bounds_type;          /* 0 unbounded, 1 height_bounds, 2 bounding_box (mapper_initialization.cpp:62-80,337-358) */
  float workspace_bounds_min_corner_m[3]; /* workspace_bounds_min_corner_{x,y}_m, workspace_bounds_min_height_m */
  float workspace_bounds_max_corner_m[3]; /* workspace_bounds_max_corner_{x,y}_m, workspace_bounds_max_height_m */
  int32_t do_depth_preprocessing;         /* do_depth_preprocessing (mapper_initialization.cpp:238-243; false in every shipped config) */
  int32_t depth_preprocessing_num_dilations; /* depth_preprocessing_num_dilations: invalid-depth regions grow by this many pixels */
  float invalid_depth_decay_factor;       /* projective_tsdf_integrator_invalid_depth_decay_factor (mapper_initialization.cpp:294-300;
                                             -1 = off, nvblox_base.yaml:80; 0.8 in nvblox_dynamics.yaml:11) */
  /* -- occupancy mappers: Mapper(voxel_size, memory_type, ProjectiveLayerType::kOccupancy) -- mapping_type static_occupancy
   *    (nvblox_base.yaml:9) and the dynamic / human mapper (specializations/nvblox_segmentation.yaml:9-22) */
  int32_t projective_layer_type;          /* 0 = TSDF (default), 1 = occupancy (log-odds), 2 = TSDF with a freespace layer */
  float free_region_occupancy_probability;      /* mapper_initialization.cpp:309-312; 0.45 nvblox_base.yaml:82 */
  float occupied_region_occupancy_probability;  /* :315-317; 0.55 */
  float unobserved_region_occupancy_probability;/* :320-322; 0.5 */
  float occupied_region_half_width_m;           /* :327; 0.1 */
  float free_region_decay_probability;          /* occupancy decay, :416; 0.55 */
  float occupied_region_decay_probability;      /* :421; 0.30 in the shipped configs */
  int32_t esdf_mode;                      /* node param esdf_mode, node_params.hpp:90: 0 = "2d" (default, the slice), 1 = "3d" (every voxel
                                             of every updated block; MultiMapper(voxel_size, mapping_type, EsdfMode::k3D, ...), nvblox_node.cpp:187-190) */
  /* -- freespace integrator of a projective_layer_type 2 mapper (MappingType::kDynamic's static mapper = TSDF with freespace,
   *    layer_publishing.cpp:747; parameters mapper_initialization.cpp:430-462, values nvblox_dynamics.yaml:12-18) */
  float max_tsdf_distance_for_occupancy_m;                    /* 0.15 */
  int32_t max_unobserved_to_keep_consecutive_occupancy_ms;    /* 200 */
  int32_t min_duration_since_occupied_for_freespace_ms;       /* 1000 (250 in nvblox_dynamics.yaml) */
  int32_t min_consecutive_occupancy_duration_for_reset_ms;    /* 2000 */
  int32_t check_neighborhood;                                 /* 1 */
  int32_t initialize_to_high_confidence_freespace;            /* 0 */
  /* -- [U] open choices (SURVEY.md 8a "open choices the oracle must expose as switches"): the arithmetic lives in the absent
   *    nvblox core, so every recollection that could be wrong is a switch implemented on BOTH sides (these kernels and
   *    oracle/nvblox_oracle.c) and parity-tested in both positions -- pinning to the real core is then a flag flip.
   *    0 is always the default behaviour documented in DESIGN.md section 3. */
  int32_t tsdf_weighting_variant;          /* formulas of the four non-trivial WeightingFunctionType modes: 0 = set A, 1 = set B */
  int32_t tsdf_skip_at_negative_truncation;/* voxel exactly at sdf == -truncation: 0 = integrated (skip iff sdf < -trunc), 1 = skipped (skip iff sdf <= -trunc) */
  int32_t tsdf_weight_clamp_before_blend;  /* 0 = blend with the unclamped sum, then w = min(w + w_m, max_weight); 1 = sum clamped first,
                                              distance blended as a running average over the clamped sum */
  float color_occlusion_threshold_vox;     /* colour occlusion test |synthetic depth - voxel depth| <= this (voxels); < 0 = the truncation distance */
  int32_t esdf_propagation;                /* 0 = exact Euclidean distance transform; 1 = synchronous 4-neighbour parent propagation to its fixed
                                              point, restricted to allocated ESDF blocks (the reference's sweep / propagate loop class) */
  int32_t mesh_ambiguity_rule;             /* marching-cubes ambiguous faces: 0 = inside corners cut off separately, 1 = inside corners joined,
                                              2 = complement-symmetric table (rule 0 for <= 4 inside corners, else rule 1: the classic table's behaviour) */
  int32_t mesh_normal_rule;                /* welded vertex normal: 0 = normal of the first triangle referencing it, 1 = area-weighted mean of the
                                              block's triangles referencing it */
  /* -- decay integrator switches (mapper_initialization.cpp:383-428; nvblox_base.yaml:103-107).  [U] semantics, DESIGN.md 3 */
  int32_t decay_deallocate_decayed_blocks; /* decay_integrator_deallocate_decayed_blocks (1): 0 = a fully decayed block stays allocated with its decayed voxels */
  int32_t tsdf_set_free_distance_on_decayed; /* tsdf_set_free_distance_on_decayed (0): 1 = an observed voxel whose weight falls below the threshold
                                              becomes FREE instead of fading to unknown: distance = tsdf_decayed_free_distance_vox voxels, weight = the threshold */
  float tsdf_decayed_free_distance_vox;    /* tsdf_decayed_free_distance_vox (4.0) */
  int32_t occupancy_decay_to_free;         /* occupancy_decay_to_free (0): 1 = occupied voxels decay past unknown into free and stay there; free voxels are not decayed */
  /* -- ground-plane-relative 2-D slice (mapper_initialization.cpp:136,257-260; [U] semantics).  With esdf_use_ground_plane the z
   *    band a column (x, y) of the slice looks at is [h + slice_height_above_plane_m, h + slice_height_above_plane_m + slice_height_thickness_m],
   *    h = the height of esdf_ground_plane {nx, ny, nz, d: n . p + d = 0, nz > 0} at the column's centre, instead of the fixed
   *    [esdf_slice_min_height, esdf_slice_max_height]; the output plane stays esdf_slice_height.  nvblox::MultiMapper sets plane and switch from its
   *    ground-plane estimator before every updateEsdf when multi_mapper.experimental_use_ground_plane_estimation is on. */
  float slice_height_above_plane_m;        /* slice_height_above_plane_m (0) */
  float slice_height_thickness_m;          /* slice_height_thickness_m (0) */
  int32_t esdf_use_ground_plane;           /* (0) */
  float esdf_ground_plane[4];
} nvbx_mapper_params;

/* nvblox::Lidar(num_azimuth_divisions, num_elevation_divisions, min_valid_range_m, vertical_fov_rad) or
 * (…, min_angle_below_zero_elevation_rad, max_angle_above_zero_elevation_rad) -- nvblox_node.cpp:1315-1323.
 * Elevations are signed here: min_elevation_rad < 0 below the horizon (vfov form: -vfov/2, +vfov/2). */
typedef struct {
  int32_t num_azimuth_divisions, num_elevation_divisions;
  float min_valid_range_m, min_elevation_rad, max_elevation_rad;
} nvbx_lidar;

/* Per-frame work counters (bench.py turns them into algorithmic bytes). */
typedef struct {
  int64_t blocks_allocated;     /* live hash entries */
  int64_t tsdf_blocks_in_view;  /* N_v of the last integrateDepth */
  int64_t color_blocks_updated; /* N_c of the last integrateColor */
  int64_t esdf_columns_marked;  /* N_u columns re-marked by the last updateEsdf */
  int64_t esdf_blocks_swept;    /* N_e ESDF blocks rewritten by the last updateEsdf */
  int64_t esdf_window_voxels;   /* voxels of the EDT working window (incl. halo) */
  int64_t mesh_blocks_updated;  /* N_m of the last updateColorMesh */
  int64_t mesh_vertices;        /* V written by the last updateColorMesh */
  int64_t mesh_triangles;       /* T (triangles) written by the last updateColorMesh */
  int64_t capacity_overflow;    /* != 0 if any pool / arena / window overflowed since creation */
  int64_t lidar_blocks_beam_centric; /* blocks in view of the last LiDAR scan that the beam-centric far-field launch updated (the dense launch took the rest) */
} nvbx_counters;

/* ---- lifetime --------------------------------------------------------------------------------------------------
 * nvblox::MultiMapper(voxel_size, MappingType, EsdfMode, MemoryType::kDevice, shared_ptr<CudaStream>)
 *   nvblox_ros/src/lib/nvblox_node.cpp:187-190, fuser_node.cpp:85-89.  `hip_stream` may be NULL (library-owned stream).
 * block_capacity = number of 8^3 blocks the HBM pools are sized for initially (3 x 4 KiB per block), 64 .. 2^24, or 0 = automatic
 * (about 4 % of the free HBM, 2^16 .. 2^20 blocks); the pools grow on demand, see nvbx_mapper_set_max_capacity.
 * Parameter values the kernels' loop bounds rely on are checked here and in nvbx_mapper_set_params (NVBX_E_INVALID, reason in
 * nvbx_last_error): voxel_size, both integration distances, truncation distance and max_weight > 0 and finite,
 * projective_layer_type in 0..2, esdf_mode in 0..1, occupancy probabilities strictly inside (0, 1). */
int nvbx_mapper_create(int device, void* hip_stream, const nvbx_mapper_params* params, int64_t block_capacity,
                       nvbx_mapper** out);
int nvbx_mapper_destroy(nvbx_mapper* m);
/* Pool growth.  The reference's layers allocate blocks on demand (Layer::allocateBlockAtIndex -- test_esdf_and_gradient_conversions.cpp:87);
 * here `block_capacity` is the INITIAL size of the HBM pools: before a frame is enqueued the integrate calls look at the number of free
 * slots the GPU last reported (pinned host memory, no synchronisation) and, below half, double every pool (contents kept, hash rebuilt
 * on the device; the call synchronises once) up to max_block_capacity (default 2^22, NVBX_MAX_BLOCKS in the environment; at most 2^24).
 * max_block_capacity <= the current capacity: fixed pools -- an allocation beyond them is dropped and reported through
 * nvbx_counters::capacity_overflow, never fatal.  Device pointers handed out by nvbx_get_device_view are valid until the next call
 * that can allocate, or that decays the map (the hash table of the surviving blocks is built in a second buffer: nvblox_hip_device.h).  nvbx_mapper_capacity = the current capacity. */
int nvbx_mapper_set_max_capacity(nvbx_mapper* m, int64_t max_block_capacity);
int64_t nvbx_mapper_capacity(nvbx_mapper* m);
/* the offline fuser's parameter values (nvblox_examples_bringup/config/nvblox/fuser.yaml:24-42; decay / workspace values from
 * nvblox_base.yaml:87-107) = the benchmark configuration; pure host function */
void nvbx_default_params(nvbx_mapper_params* out);
/* MultiMapper::setMapperParams  -- nvblox_node.cpp:203, fuser_node.cpp:94 */
int nvbx_mapper_set_params(nvbx_mapper* m, const nvbx_mapper_params* params);
int nvbx_mapper_get_params(const nvbx_mapper* m, nvbx_mapper_params* out);
/* CudaStream::synchronize -- conversions/esdf_slice_conversions.cu:107-108 */
int nvbx_synchronize(nvbx_mapper* m);
/* Enqueue everything the mapper holds back (the distance transform of the last nvbx_update_esdf, see there) on its stream
 * WITHOUT waiting: for callers that order their own work behind the mapper's with stream events instead of a host sync. */
int nvbx_flush(nvbx_mapper* m);
/* Colour deferral (cross-frame pipelining).  enable = 2, the DEFAULT of a new mapper since round 4: nvbx_integrate_color / _bgra8 of a single frame
 * is HELD BACK -- the image is copied into staging memory the mapper owns (one launch on the mapper's stream, ~0.9 MB at 640x480), the other arguments
 * are remembered -- and so is an nvbx_update_esdf that follows it.  The next single-frame nvbx_integrate_depth / _u16mm (for a held-back
 * nvbx_integrate_color_batch of n > 1 frames: the next nvbx_integrate_depth_batch of n > 1 frames) carries them out in pipelined order, two launches per
 * depth + colour + ESDF frame instead of four: {view marking of the new depth frame || sphere tracing, candidate-block discovery and ESDF site marking of
 * the held-back frame}, then {TSDF update of the new frame || colour integration and distance transform of the held-back frame} (three launches where the
 * mapper does not run the exact 2-D ESDF, or has integrated a LiDAR scan).  The overlapped parts are independent (DESIGN.md 2.8, table of invariants).
 * EVERY other entry point (queries, synchronize / flush, batches, LiDAR, mesh, decay, clearing, another integrate_color, ...) first carries the held-back
 * calls out exactly as they would have run at call time, so results -- map contents, ESDF, views, every query -- are bit-identical to the undeferred
 * sequence (tests/test_gpu_pipeline.py; the whole GPU suite runs with this default), and the caller may overwrite or free its colour image as soon as
 * nvbx_integrate_color has returned: nothing a host can observe through this header differs from enable = 0, except the time.  (What CAN tell the
 * difference: a kernel of the caller's own that reads the colour layer or the ESDF through include/nvblox_hip_device.h without calling nvbx_flush first.)
 * An nvbx_update_esdf that follows a depth frame WITHOUT a colour frame in between is held back the same way and carried out by the next camera depth
 * frame.  Argument errors are still reported by the call that made them.
 * enable = 1 (opt-in, zero-copy): no staging copy -- and a CONTRACT instead: the colour image passed to nvbx_integrate_color must stay valid and UNCHANGED
 * until the next call into this mapper has returned that either consumes or flushes the frame -- any call except nvbx_detect_dynamics,
 * nvbx_remove_small_components, nvbx_split_depth_by_mask, nvbx_dynamic_depth_split and nvbx_set_time_ms, which leave held-back work alone (the
 * dynamic-mapping frame starts with them).  nvblox_ros re-uses ONE colour buffer per node (nvblox_node.hpp:485-488) and fills it right before
 * integrateColor, after the depth frame -- compatible with the contract for the depth -> colour -> updateEsdf order of NvbloxNode::tick(); a node that
 * fills the colour buffer BEFORE calling integrateDepth must not use it.
 * enable = 0: the classic order, every call launches its own kernels (four launches per frame).  NVBX_COLOR_DEFERRAL=0|1|2 in the environment sets the
 * default of mappers created afterwards. */
int nvbx_mapper_set_color_deferral(nvbx_mapper* m, int32_t enable);
/* The NVBX_* environment variables of the library (launch geometry and A/B switches; none changes a result) are read when a mapper is
 * created and kept per mapper.  nvbx_mapper_reload_knobs reads them again for this mapper: held-back work is carried out first, under the old
 * settings; the calls that follow use the new ones.  Three variables shape a mapper at creation and are NOT re-applied to a live one: NVBX_MAX_BLOCKS
 * (nvbx_mapper_set_max_capacity keeps what it last set), NVBX_COLOR_DEFERRAL (likewise nvbx_mapper_set_color_deferral)
 * and NVBX_DEFER_EDT.  NVBX_FRAME_POOL_MAX belongs to the process-wide frame pool, not to a mapper, and is read whenever the pool would grow. */
int nvbx_mapper_reload_knobs(nvbx_mapper* m);
/* ---- Library-owned device frames: OWNERSHIP TRANSFER of input images (csrc/frames.hip).
 * Replaces the node-owned, re-used device image buffers of the reference (nvblox_node.hpp:484-488: color_image_, filled by the conversion on the
 * mapper's stream right before integrateColor, nvblox_node.cpp:1237-1263, conversions/image_conversions_thrust.cu:68-84) for a library that may hold a
 * colour frame back (nvbx_mapper_set_color_deferral above): an image that lives in a frame of nvbx_frame_acquire is RETAINED by the mapper instead of
 * copied (no k_stage_color launch, in either deferral form), and let go of when the launches that read it are enqueued.  A writer asks for "a frame
 * nobody else holds" before it writes: nvblox::Image<T> does so in its non-const dataPtr() / copyFromAsync / resize (include/nvblox/sensors/image.h) and
 * rotates to another frame while the mapper still holds the last one.
 *   nvbx_frame_acquire(device, bytes, writer_stream, &ptr): a device buffer of >= bytes, reference count 1 (the caller's).  Never hands out memory
 *     that launches of a mapper may still read: a frame a mapper has let go of is given to a writer only when those launches are known to have
 *     finished, or when `writer_stream` is the very stream they were enqueued on (stream order does the rest); otherwise another frame is taken, the
 *     pool grows (NVBX_FRAME_POOL_MAX frames per size, default 8) or -- pool full -- the call waits for the oldest.  writer_stream: the stream the
 *     caller will write the frame on, or NVBX_STREAM_UNKNOWN (host writes, any stream).
 *   nvbx_frame_retain / nvbx_frame_release: reference counting; at 0 the frame returns to the pool -- and is handed out again only after the work that
 *     may still use it: the release that brings the count to 0 records an event on every stream the library knows on the frame's device (the streams
 *     of live mappers and the legacy default stream), and nvbx_frame_acquire skips the frame until those events are reached (hipFree, which the
 *     reference's image buffers end in, waits for the device instead).  Only work on a non-blocking stream that no live mapper runs on is the
 *     caller's to order (or to name: nvbx_frame_release_on).  nvbx_frame_release_on(ptr, stream): the same for a caller that knows
 *     the ONE stream its work on the frame was enqueued on (one event; NVBX_STREAM_UNKNOWN = nvbx_frame_release).  A holder that lets go while others
 *     still hold the frame records nothing: its writes precede the others' reads by its own ordering, as with any shared buffer.
 *     nvbx_frame_refcount: > 1 = somebody else (a mapper) holds it too; -1 = not a frame.  nvbx_frame_device: the device the frame lives on (-1 = not a frame).
 *     nvbx_frame_writable: the question a writer asks before it overwrites a frame it holds (below).
 *   nvbx_frame_pool_trim(device | -1): hipFree every frame nobody holds; returns how many.  nvbx_frame_pool_stats: {held, free, bytes, created, waits, syncs}.
 *   nvbx_frame_upload: hipMemcpyAsync into a frame on `hip_stream` (NVBX_STREAM_UNKNOWN: a blocking hipMemcpy) -- for hosts without a HIP binding of
 *     their own (the ctypes mirror).
 *   nvbx_color_image_acquire(m, rows, cols, 3 | 4, &ptr) = nvbx_frame_acquire(device of m, rows * cols * bytes_per_pixel, stream of m, &ptr): for the
 *     converter that runs on the mapper's stream.  nvbx_integrate_color_owned(m, frame, 3 | 4, ...) = nvbx_integrate_color / _bgra8 + the caller's
 *     reference passes to the mapper (released for the caller; on NVBX_E_INVALID the caller keeps it). */
#define NVBX_STREAM_UNKNOWN ((void*)(intptr_t)-1)
int nvbx_frame_acquire(int device, size_t bytes, void* writer_stream, void** dev_ptr_out);
int nvbx_frame_retain(void* dev_ptr);
int nvbx_frame_release(void* dev_ptr);
int nvbx_frame_release_on(void* dev_ptr, void* last_stream);
int32_t nvbx_frame_device(const void* dev_ptr);
int32_t nvbx_frame_refcount(const void* dev_ptr);
/* 1 = the caller is the only holder AND no launch of a mapper (nor work recorded at an earlier release) can still be using the frame (finished, or enqueued on `writer_stream` itself): write in
 * place; 0 = take another frame (nvbx_frame_acquire) and let go of this one; -1 = not a live frame. */
int32_t nvbx_frame_writable(const void* dev_ptr, void* writer_stream);
int nvbx_frame_pool_trim(int device);
int nvbx_frame_pool_stats(int64_t out[6]);
int nvbx_frame_upload(void* dev_ptr, const void* src, size_t bytes, void* hip_stream);
int nvbx_color_image_acquire(nvbx_mapper* m, int32_t rows, int32_t cols, int32_t bytes_per_pixel, void** dev_ptr_out);
int nvbx_integrate_color_owned(nvbx_mapper* m, void* frame, int32_t bytes_per_pixel, int32_t rows, int32_t cols, const float T_L_C[16], const nvbx_camera* camera);
/* The hipStream_t all of the mapper's work is enqueued on (the one handed to nvbx_mapper_create, or the library-owned one):
 * implicit conversion of nvblox::CudaStream to cudaStream_t -- conversions/esdf_slice_conversions.cu:107-108.  A caller that
 * reads / writes buffers it shares with the mapper on ANOTHER stream (e.g. an RCCL collective on the framework's stream) orders
 * the two with events on this handle. */
int nvbx_get_stream(nvbx_mapper* m, void** hip_stream_out);
/* Stream order between two mappers on DIFFERENT streams of one device (no reference counterpart: nvblox::MultiMapper hands both of its mappers one
 * CudaStream, nvblox_node.cpp:187-190; a host that creates its mappers on streams of their own -- stream = NULL at nvbx_mapper_create -- and passes
 * device images from one to the other, e.g. the split depth image of nvbx_dynamic_depth_split, orders them with this instead of a host
 * synchronisation): work enqueued on `waiter`'s stream after this call starts only when
 * everything ENQUEUED on `producer`'s stream before it has finished (held-back calls of `producer` are not enqueued yet and are not waited for).
 * Asynchronous; a no-op when both run on one stream. */
int nvbx_mapper_wait_for(nvbx_mapper* waiter, nvbx_mapper* producer);
const char* nvbx_last_error(void);
/* Arithmetic self-test (no reference counterpart; test infrastructure of the boundary): evaluates the library's own division and
 * square-root sequences (csrc/nvbx_arith.h: the compiler's IEEE sequences without their range-scaling steps) on device arrays --
 * quot[i] = a[i] / b[i], root[i] = sqrt(|a[i]|) -- on the current device's null stream and waits.  tests/test_gpu_arith.py compares
 * the results with IEEE float division / square root bit for bit: the CPU oracle uses the plain operators. */
int nvbx_selftest_arith(const float* a_dev, const float* b_dev, float* quot_dev, float* root_dev, int64_t n);
/* Mapper::clear / fresh map (load_map path re-creates the mapper: nvblox_node.cpp:1698-1703) */
int nvbx_mapper_clear(nvbx_mapper* m);

/* ---- integration (asynchronous on the mapper stream) --------------------------------------------------------------
 * Argument checks (NVBX_E_INVALID, nothing launched): the camera's width / height must equal the image's cols / rows and its
 * focal lengths be > 0; image sides are 1 .. 32768 (pixel indices are 31-bit on the device); T_L_C must be finite and keep everything within the integration distance inside the addressable block
 * range (nvbx_index3d).  Every entry point makes the mapper's device the calling thread's current device and leaves it so.
 * MultiMapper::integrateDepth(const DepthImage&, const Transform& T_L_C, const Camera&, Time) -- nvblox_node.cpp:1062 */
int nvbx_integrate_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                         const nvbx_camera* camera);
/* Same, depth given as uint16 millimetres: fuses conversions::depthImageFromNitrosViewAsync's DivideBy1000
 * (conversions/image_conversions_thrust.cu:39-45,140-142) into the integrator's depth read. */
int nvbx_integrate_depth_u16mm(nvbx_mapper* m, const uint16_t* depth_mm_dev, int32_t rows, int32_t cols,
                               const float T_L_C[16], const nvbx_camera* camera);
/* MultiMapper::integrateDepth(const Pointcloud&, const Transform&, const Lidar&, ...) -- nvblox_node.cpp:1382-1384, after
 * the point cloud has been rendered to a range image (nvbx_depth_image_from_pointcloud; the reference exposes that image
 * as getLastDepthFrameFromPointcloud(), nvblox_node.cpp:1397).  range_dev: rows = elevation divisions, cols = azimuth
 * divisions, metres along the beam, <= 0 invalid.  Uses lidar_max_integration_distance_m. */
int nvbx_integrate_lidar_depth(nvbx_mapper* m, const float* range_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                               const nvbx_lidar* lidar);
/* depthImageFromPointcloudKernel (conversions/pointcloud_conversions.cu:118-150): points (x,y,z f32, sensor frame) ->
 * range image; NaN points and points outside the model are skipped; several points in one pixel: one of them wins. */
int nvbx_depth_image_from_pointcloud(nvbx_mapper* m, const float* points_xyz_dev, int64_t n_points, const nvbx_lidar* lidar,
                                     float* range_dev);
/* [U] LiDAR motion compensation (use_lidar_motion_compensation, nvblox_node.cpp:1339-1384): every point carries its time within the
 * scan (rel_time_ms, 0 = scan start = the time T_L_S_start refers to); the sensor pose at that time is interpolated between
 * T_L_S_start and T_L_S_end (translation linearly, rotation by normalised quaternion interpolation) and the point is re-expressed
 * in the sensor frame at scan start.  Out may alias in.  Asynchronous.  Feed the result to nvbx_depth_image_from_pointcloud. */
int nvbx_motion_compensate_pointcloud(nvbx_mapper* m, const float* points_in_dev, const float* rel_time_ms_dev, int64_t n_points,
                                      const float T_L_S_start[16], const float T_L_S_end[16], float scan_duration_ms, float* points_out_dev);
/* MultiMapper::integrateColor(const ColorImage&, const Transform&, const Camera&) -- nvblox_node.cpp:1264.
 * rgb_dev: rows*cols*3 bytes, nvblox::Color order r,g,b (image_conversions.cpp:100-101). */
int nvbx_integrate_color(nvbx_mapper* m, const uint8_t* rgb_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                         const nvbx_camera* camera);
/* Same, colour given as bgra8 (4 bytes per pixel): fuses conversions::colorImageFromNitrosViewAsync's ToRgba<Bgra>
 * channel reorder (conversions/image_conversions_thrust.cu:60-65, image_conversions.cpp:170-176) into the integrator's
 * colour fetch (one aligned 4-byte load per tap). */
int nvbx_integrate_color_bgra8(nvbx_mapper* m, const uint8_t* bgra_dev, int32_t rows, int32_t cols, const float T_L_C[16],
                               const nvbx_camera* camera);
/* ---- camera batches: the reference's multi-camera mode (up to four cameras feed ONE mapper through one queue, an integrateDepth /
 * integrateColor call per camera frame: nvblox_ros/include/nvblox_ros/nvblox_node.hpp:298-332, nvblox_node.cpp:247-292) as ONE launch
 * set.  n (1 .. NVBX_MAX_BATCH) frames of the same image size; depth_dev / rgb_dev = n device image pointers (host array), T_L_C =
 * n x 16 floats, cameras = n structs.  DEFINED as equal to the n separate calls in order 0 .. n-1 -- map contents bit for bit, the
 * "last view" queries (nvbx_last_depth_view / _color_view, decayTsdfExcludeLastView, nvbx_get_synthetic_depth) report camera n-1's --
 * but with one view-marking + one TSDF-update launch (depth) and one sphere-tracing + one colour launch for all n cameras: at
 * 640x480 a frame is launch / latency bound, so a batch of 8 costs far less than 8 frames.  Mappers with a freespace layer and depth
 * dilation fall back to the separate calls. */
#define NVBX_MAX_BATCH 8
int nvbx_integrate_depth_batch(nvbx_mapper* m, int32_t n, const float* const* depth_dev, int32_t rows, int32_t cols, const float* T_L_C,
                               const nvbx_camera* cameras);
int nvbx_integrate_color_batch(nvbx_mapper* m, int32_t n, const uint8_t* const* rgb_dev, int32_t rows, int32_t cols, const float* T_L_C,
                               const nvbx_camera* cameras);
/* ---- a PAIR of mappers, one depth frame each: MultiMapper::integrateDepth of the dynamic and the human mapping types (nvblox_node.cpp:1057-1062:
 * the depth image is split by a mask; the unmasked part goes to the background mapper, the masked part to the foreground occupancy mapper, one
 * integrateDepth each).  DEFINED as equal to nvbx_integrate_depth(ma, depth_a, ...) followed by nvbx_integrate_depth(mb, depth_b, ...) -- both maps, the
 * held-back calls each of them carries, "last view" queries: bit for bit -- but the two view-marking launches share one grid and so do the two
 * TSDF-update launches (k_mark_view_pair, k_integrate_tsdf_color_pair): two launches instead of four; the maps share nothing, so nothing else changes.
 * Needs both mappers on one device and one stream (what nvblox::MultiMapper hands out); whatever the pair cannot express -- different streams, depth
 * dilation, a held-back colour BATCH, held-back colour frames of BOTH mappers in different encodings (one rgb8, the other bgra8), the ESDF side
 * stream -- falls back to the two calls.  NVBX_DEPTH_PAIR=0 in the environment: always the two calls. */
int nvbx_integrate_depth_pair(nvbx_mapper* ma, const float* depth_a_dev, nvbx_mapper* mb, const float* depth_b_dev, int32_t rows, int32_t cols,
                              const float T_L_C[16], const nvbx_camera* camera);
/* MultiMapper::updateEsdf() (EsdfMode::k2D) -- nvblox_node.cpp:781.
 * Scheduling note: the site-marking half runs at once (or already ran inside the preceding nvbx_integrate_color launch);
 * the distance-transform half may be HELD BACK until the next entry point of this mapper: nvbx_integrate_depth[_u16mm]
 * runs it inside its first launch, beside the view marking it does not interact with; every other entry point -- all
 * queries, nvbx_synchronize, colour / LiDAR integration, mesh, maintenance -- enqueues it first.  Results observed through
 * this API are therefore always those of the completed update; a caller that only synchronises the raw stream and calls
 * nothing else leaves the transform un-enqueued until its next call.  NVBX_DEFER_EDT=0 in the environment disables this. */
int nvbx_update_esdf(nvbx_mapper* m);
/* Mapper::updateColorMesh(UpdateFullLayer) -- layer_publishing.cpp:686-689, nvblox_node.cpp:1611 */
int nvbx_update_color_mesh(nvbx_mapper* m, int32_t update_full_layer);
/* Mapper::decayTsdfExcludeLastView<Camera>() / decayTsdf -- nvblox_node.cpp:931-936 */
int nvbx_decay_tsdf(nvbx_mapper* m, int32_t exclude_last_view);
/* Mapper::decayOccupancyAllVoxels() -- nvblox_node.cpp:925-929 (occupancy mappers): log-odds move towards 0 (unknown) by the
 * log-odds of free_region_decay_probability / occupied_region_decay_probability and stop there; all-unknown blocks are deallocated */
int nvbx_decay_occupancy(nvbx_mapper* m);
/* Mapper::clearOutsideRadius(center, radius) -- nvblox_node.cpp:1566-1583 */
int nvbx_clear_outside_radius(nvbx_mapper* m, const float center[3], float radius);

/* Mapper::getClearedBlocks(layer_types) -- layer_publishing.cpp:716,804: Index3D (sorted, unique) of the projective-layer (TSDF /
 * occupancy) blocks that decayTsdf / decayOccupancyAllVoxels / clearOutsideRadius deallocated since the last call; the list is
 * emptied.  Returns their number n; if n > capacity nothing is written and the list is kept (call again with room for n);
 * synchronises. */
int64_t nvbx_take_cleared_blocks(nvbx_mapper* m, nvbx_index3d* out, int64_t capacity);

/* Mapper::clearTsdfInsideShapes(std::vector<BoundingShape>) -- nvblox_node.cpp:1834 (the EsdfAndGradients service's
 * clearing request, conversions/esdf_and_gradients_conversions.cu:127-180).  A shape is a sphere (kind 0: centre, radius)
 * or an axis-aligned box (kind 1: min corner, max corner); TSDF voxels whose centre lies inside any shape are reset to
 * unobserved (distance 0, weight 0) and their blocks become ESDF / mesh dirty. */
typedef struct { int32_t kind; float a[3]; float b[3]; } nvbx_bounding_shape;   /* sphere: a = centre, b[0] = radius; box: a = min, b = max */
int nvbx_clear_tsdf_inside_shapes(nvbx_mapper* m, const nvbx_bounding_shape* shapes_host, int32_t n_shapes);

/* ---- ESDF slice (EsdfSlicer) ------------------------------------------------------------------------------------
 * EsdfSlicer::sliceLayerToDistanceImage(esdf_layer, slice_height, unknown_value, &aabb, &Image<float>) --
 * nvblox_node.cpp:836-844.  Two-step like Image<float> allocation: query the size, then fill a device image
 * (row = y, col = x, row-major; origin aabb[0..2]; conversions/esdf_slice_conversions.cu:60-64). */
int nvbx_esdf_slice_size(nvbx_mapper* m, int32_t* rows, int32_t* cols, float aabb_min_max[6]);
int nvbx_esdf_slice_to_image(nvbx_mapper* m, float unknown_value, float* image_dev, int64_t capacity_elems,
                             int32_t* rows, int32_t* cols, float aabb_min_max[6]);
/* EsdfSliceConverter::distanceMapSliceMsgFromSliceImage's D2H (esdf_slice_conversions.cu:81-109) in one call -- and ONE wait for the device: the
 * slicing launch reads the layer's AABB itself and writes size + image into pinned host memory (no size query first; round 5).  NVBX_E_CAPACITY
 * (image_host null or capacity_elems too small): *rows / *cols / aabb report what is needed, nothing is copied. */
int nvbx_esdf_slice_to_host(nvbx_mapper* m, float unknown_value, float* image_host, int64_t capacity_elems,
                            int32_t* rows, int32_t* cols, float aabb_min_max[6]);
/* EsdfSlicer::sliceLayersToCombinedDistanceImage(layer_1, layer_2, height_1, height_2, unknown, &aabb, &image) --
 * nvblox_node.cpp:836-840 (static + dynamic mapper in one costmap): the image covers the union of the two layers' AABBs,
 * a pixel is the smaller of the two signed distances where both are observed, the observed one where only one is, else
 * unknown_value.  Both mappers must live on the same device; the work is enqueued on m1's stream behind everything
 * enqueued on m2's (event).  aabb z range = m1's slice block. */
int nvbx_esdf_slice_combined_size(nvbx_mapper* m1, nvbx_mapper* m2, int32_t* rows, int32_t* cols, float aabb_min_max[6]);
int nvbx_esdf_slice_combined_to_image(nvbx_mapper* m1, nvbx_mapper* m2, float unknown_value, float* image_dev, int64_t capacity_elems,
                                      int32_t* rows, int32_t* cols, float aabb_min_max[6]);
/* EsdfSlicer::occupancyGridFromSliceImage(img, int8_t*, unknown) -- nvblox_node.cpp:917-919:
 * 100 where distance <= 0 (inside), 0 where observed free, -1 where unknown. */
int nvbx_occupancy_grid_from_slice(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols,
                                   float unknown_value, int8_t* grid_dev);
/* conversions::EsdfSliceConverter::pointcloudFromSliceImage kernel (esdf_slice_conversions.cu:33-73,138-159):
 * compacts observed pixels to {x,y,z,intensity} float4; returns the count through *n_points (synchronises). */
int nvbx_pointcloud_from_slice(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols,
                               const float aabb_min_max[6], float slice_height, float unknown_value,
                               float* points_xyzi_dev, int32_t* n_points);
/* voxelLayerToDenseVoxelGridInAABBAsync<SignedDistanceFunctor> (esdf_and_gradients_conversions.cu:88-125):
 * out[x*(Ny*Nz) + y*Nz + z] = signed metres or default_value; AABB given in global voxel indices. */
int nvbx_esdf_dense_grid(nvbx_mapper* m, const int32_t min_vox[3], const int32_t size_vox[3], float default_value,
                         float* grid_dev);
/* [U] Interpolator::interpolateOnGPU(points_L, layer, &distances, &success_flags) (nvblox/interpolation/interpolation_3d.h) with
 * gradients: distance, gradient and validity at n arbitrary points (SEMANTICS.md "Point queries").  layer = NVBX_LAYER_TSDF or
 * NVBX_LAYER_ESDF (exactly one).  Per axis u = p / voxel_size - 0.5, b = floor(u), t = u - b; the corners are the voxels b + {0, 1}.
 * Valid when every corner's block carries the layer and the voxel passes the layer's test (TSDF: weight >= min_weight; ESDF: observed,
 * value +-sqrt(squared_distance_vox) * voxel_size as nvbx_esdf_dense_grid): distance = the trilinear interpolant, gradient = its
 * analytic gradient per metre.  Otherwise distance = unknown_value, gradient = 0, valid = 0 -- also for a point whose corners leave
 * the addressable range.  ESDF of a 2-D mapper (esdf_mode 0): bilinear over the plane z = floor(esdf_slice_height / voxel_size),
 * p.z ignored, gradient z = 0.  min_weight is ignored by ESDF queries; a TSDF query on an occupancy mapper is NVBX_E_INVALID.
 * points_xyz_dev[n][3], distance_dev[n], gradient_xyz_dev[n][3] (NULL: not written), valid_dev[n] (NULL: not written).
 * Asynchronous on the mapper's stream; n == 0 launches nothing.  An ESDF query carries held-back work out first; a TSDF query
 * leaves it held back (it reads nothing that work writes).  The same arithmetic for callers' kernels: nvbx_dev_interpolate_tsdf /
 * nvbx_dev_interpolate_esdf in nvblox_hip_device.h, bit-identical. */
int nvbx_query_points(nvbx_mapper* m, uint32_t layer, const float* points_xyz_dev, int64_t n, float min_weight, float unknown_value,
                      float* distance_dev, float* gradient_xyz_dev, uint8_t* valid_dev);
/* [U] The colour layer at n arbitrary points (SEMANTICS.md "Colour alignment and colour queries"): the lattice and the trilinear interpolant of
 * the TSDF query above, over the colour voxels.  A corner counts when its block carries the colour layer and its voxel's weight is
 * >= min_color_weight; the point is valid when all eight corners count.  Corner luminance Yc = (77 r + 150 g + 29 b) / 256 (levels, exact in
 * f32); luminance_dev[n] = Y(p), gradient_xyz_dev[n][3] = dY/dp per metre, rgb_dev[n][3] = the same interpolant per channel of the raw u8
 * values; all 0 at an invalid point.  rgb_dev, luminance_dev, gradient_xyz_dev: NULL = not written; valid_dev[n] is required when n > 0.
 * One launch, asynchronous on the mapper's stream; n == 0 launches nothing.  Held-back colour work is carried out first (the call reads the
 * colour layer).  NVBX_E_INVALID: a NULL mapper, points or valid pointer (n > 0); n < 0; an occupancy mapper; a min_color_weight that is not a
 * number. */
int nvbx_query_colors(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, float min_color_weight, float* rgb_dev, float* luminance_dev,
                      float* gradient_xyz_dev, uint8_t* valid_dev);

/* ---- rendering and ray casts ([U] SphereTracer::renderImageOnGPU / renderRgbdImageOnGPU / castOnGPU, nvblox/rays/sphere_tracer.h) -----
 * The map seen along rays (SEMANTICS.md "Rendering and ray casts"): the sphere tracing of integrateColor's occlusion image -- nearest voxel,
 * step = voxel distance, the truncation distance through unobserved space until something positive has been seen, hit when an observed
 * sample is < sphere_tracing_surface_eps_vox * voxel_size after a positive one, stop at sphere_tracing_max_steps or the ray length -- from
 * any pose, at any subsampling, into the caller's buffers.  One launch, read-only on the map, asynchronous on the mapper's stream.
 * nvbx_render_view: ray (r, c) of the rows / s x cols / s image goes through the centre of full-resolution pixel (r s, c s) of `camera` at
 *   pose T_L_C (row-major 4 x 4, camera -> layer).  depth = z of the hit in the camera frame (t * direction z), 0 = no surface.
 * nvbx_cast_rays: origins / directions [n][3] in layer-frame metres, directions of unit length (the caller's contract); t_dev[n] = ray parameter of
 *   the hit in metres, 0 = no hit; hit_dev[n] = 1 / 0.  A direction that is not finite or all-zero, or an origin that is not finite or
 *   outside the addressable block range, reports no hit.
 * Optional outputs of both (NULL: not computed, no loads spent): color_rgb_dev [..][3] = the colour voxel that contains the hit point
 *   P = o + t d (grey 127 where that voxel has no colour, the mesh's rule; 0 0 0 on a miss); normal_xyz_dev [..][3] = the gradient of the trilinear
 *   TSDF interpolant at P (nvbx_query_points with min_weight 1e-4), normalised; 0 0 0 on a miss, where a corner is missing or the gradient is 0.
 * subsampling 0 / max_ray_length_m <= 0: the mapper's sphere_tracing_subsampling / sphere_tracing_max_ray_length_m.
 * Errors: NVBX_E_INVALID (occupancy mapper, NULL required pointer, n < 0, rows / s < 2 or cols / s < 2, pose out of range, a ray length that
 * reaches beyond the addressable block range from every origin); NVBX_E_CAPACITY when
 * capacity_pixels < rows_out * cols_out, which are filled in (call with capacity 0 to size the buffers).  n == 0 launches nothing.
 * Held-back work (nvbx_mapper_set_color_deferral): a call without a colour output leaves it held back (it reads TSDF voxels only), a call with
 * one carries it out first (a held-back integrateColor writes the colour layer). */
int nvbx_render_view(nvbx_mapper* m, const float T_L_C[16], const nvbx_camera* camera,
                     int32_t subsampling,          /* >= 1; 0: the mapper's sphere_tracing_subsampling */
                     float max_ray_length_m,       /* <= 0: the mapper's sphere_tracing_max_ray_length_m */
                     float* depth_dev,             /* [rows/s][cols/s], 0 = no surface */
                     uint8_t* color_rgb_dev,       /* [rows/s][cols/s][3] or NULL */
                     float* normal_xyz_dev,        /* [rows/s][cols/s][3], map frame, or NULL */
                     int64_t capacity_pixels, int32_t* rows_out, int32_t* cols_out);
int nvbx_cast_rays(nvbx_mapper* m, const float* origins_xyz_dev, const float* directions_xyz_dev, int64_t n,
                   float max_ray_length_m, float* t_dev, uint8_t* hit_dev /* or NULL */,
                   uint8_t* color_rgb_dev /* or NULL */, float* normal_xyz_dev /* or NULL */);
/* The same two calls with a tracer's own step limit and surface threshold instead of the mapper's parameters, which are left as they are
 * (nvblox::SphereTracer keeps its own): max_steps <= 0 / surface_distance_epsilon_vox < 0 = the mapper's value; options NULL = both. */
typedef struct { int32_t max_steps; float surface_distance_epsilon_vox; } nvbx_render_options;
int nvbx_render_view_with(nvbx_mapper* m, const nvbx_render_options* options, const float T_L_C[16], const nvbx_camera* camera, int32_t subsampling,
                          float max_ray_length_m, float* depth_dev, uint8_t* color_rgb_dev, float* normal_xyz_dev, int64_t capacity_pixels,
                          int32_t* rows_out, int32_t* cols_out);
int nvbx_cast_rays_with(nvbx_mapper* m, const nvbx_render_options* options, const float* origins_xyz_dev, const float* directions_xyz_dev, int64_t n,
                        float max_ray_length_m, float* t_dev, uint8_t* hit_dev, uint8_t* color_rgb_dev, float* normal_xyz_dev);

/* ---- feature layer ([U] upstream's FeatureLayer / projective feature integrator; SEMANTICS.md "Feature layer") -----------------------
 * A vision backbone emits a coarse grid of C-channel fp16 vectors per colour frame; the mapper averages them into the voxels the frame
 * sees, and the caller reads them back at 3-D points.  The rules are the colour integrator's, item by item.
 * nvbx_enable_features: turns the layer on.  channels = a multiple of 8, 8 .. 256 (else NVBX_E_INVALID); again with the same value: no-op,
 *   with another: NVBX_E_INVALID; an occupancy mapper: NVBX_E_INVALID; pools that do not fit in free device memory: NVBX_E_DEVICE, the mapper
 *   stays usable.  Pools: capacity x 512 x C x 2 B of values + capacity x 2048 B of weights, carried by pool growth.  A mapper that never calls
 *   this allocates nothing for features and behaves bit for bit as without the layer.
 * nvbx_integrate_features: feat_dev = rows_f x cols_f x C fp16, row-major HWC, 16-byte aligned device memory; `camera` = the full-resolution
 *   camera the features were computed from; stride >= 1: feature pixel (i, j) is centred on full-resolution pixel coordinate
 *   ((j + 0.5) stride, (i + 0.5) stride); cols_f stride <= camera.width and rows_f stride <= camera.height (else NVBX_E_INVALID).
 *   Candidate blocks, synthetic depth (sphere-traced at sphere_tracing_subsampling into a scratch image of this call's own:
 *   nvbx_get_synthetic_depth, nvbx_last_color_view and color_blocks_updated stay the last colour frame's) and the per-voxel projection and
 *   occlusion test are nvbx_integrate_color's.  Feature taps: uf = u / stride - 0.5, vf = v / stride - 0.5, x0 = floor(uf), y0 = floor(vf),
 *   all four taps inside [0, cols_f - 1] x [0, rows_f - 1] or the voxel is skipped; per channel f = bilinear in f32 (top, bottom, then
 *   vertical, no contraction).  Blend: w0 = stored weight, tw = w0 + 1, v = old (w0 / tw) + f (1 / tw), rounded to fp16 to nearest even;
 *   weight = min(w0 + 1, max_weight).  A voxel that fails a test is not written.  The mesh is not marked dirty, no work list is touched.
 *   A block carries features while its slot has NVBX_LAYER_FEATURE: the first feature frame that reaches a voxel of a block without it
 *   treats the whole block as empty (unreached voxels: weight 0, zero values); whatever deallocates the block's TSDF (decay, radius
 *   clearing, nvbx_mapper_clear) takes its features with it.
 * nvbx_query_features: the voxel that contains p (floor(p / voxel_size) per axis); feat_out_dev [n][C] fp16 (16-byte aligned), weight_out_dev [n].
 *   Weight 0 and zero values -- never an error -- where the block is absent or carries no features, p is not finite, or p lies outside the
 *   addressable range.  Chained behind nvbx_cast_rays / nvbx_render_view it gives a feature image of the map from any pose.
 * nvbx_get_feature_blocks: whole blocks in the public layout -- voxel t = vx 64 + vy 8 + vz, C contiguous halfs per voxel: feat_out [n][512][C]
 *   fp16, weight_out [n][512] f32, found_out [n] (NULL: not written); pointer conventions of nvbx_get_blocks (host memory, synchronous).
 * nvbx_set_feature_blocks: its mirror -- feat_in [n][512][C] fp16 and weight_in [n][512] f32 in the same public layout; pointer conventions
 *   of nvbx_set_blocks (host memory, synchronous).  Block i is written only if its slot carries the TSDF layer (features do not keep a block
 *   alive: an orphan would be unreachable); any other block is skipped, written_out[i] = 0 (written_out may be NULL).  A write replaces all 512
 *   voxels, stores the weights as given and sets NVBX_LAYER_FEATURE; it touches nothing but the two feature pools and that flag: no dirty
 *   list, no view list, no mesh.  The indices of one call are distinct.  NVBX_E_INVALID (nothing written): a weight that is negative or not
 *   a number; NULL pointers with n > 0.  With it a caller puts features back into a loaded map (nvbx_load_map starts without them).
 * All of them carry held-back work out first (as nvbx_flush) and run in classic order on the mapper's stream; integrate and query are
 * asynchronous.  Before nvbx_enable_features they return NVBX_E_INVALID.  Not covered: map files, mesh vertices, multi-GPU exchange,
 * batches, LiDAR, nvbx_device_view.  Scoring the layer against query embeddings: "feature matching" below; bringing another mapper's
 * layer into this one: "feature merging". */
int nvbx_enable_features(nvbx_mapper* m, int32_t channels);
int nvbx_integrate_features(nvbx_mapper* m, const void* feat_dev, int32_t rows_f, int32_t cols_f, int32_t stride, const float T_L_C[16],
                            const nvbx_camera* camera);
int nvbx_query_features(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, void* feat_out_dev, float* weight_out_dev);
int nvbx_get_feature_blocks(nvbx_mapper* m, const nvbx_index3d* idx, int64_t n, void* feat_out, float* weight_out, int32_t* found_out);
int nvbx_set_feature_blocks(nvbx_mapper* m, const nvbx_index3d* idx, int64_t n, const void* feat_in, const float* weight_in, int32_t* written_out);

/* ---- feature matching (open-vocabulary search over the feature layer; SEMANTICS.md "Feature matching") -------------------------------
 * Scores feature voxels against Q query embeddings on the matrix cores, without moving the layer anywhere.
 * Common to both calls: queries_dev = [Q][C] fp16, row-major, 16-byte aligned device memory, C = the layer's channel count, 1 <= Q <= 128.
 *   NVBX_MATCH_DOT:    s(v, q) = sum_c f_v[c] q[c] -- the fp16 products are exact in f32, the sum is in f32 in the order the matrix instruction takes it.
 *   NVBX_MATCH_COSINE: dot / sqrt(|f_v|^2 |q|^2), the norms summed in f32; 0 where either norm is 0.
 *   Scores are NOT bit-specified (the library's only such output).  The contract is an error bound against exact arithmetic on the stored fp16
 *   values: dot within C 2^-23 sum_c |f_c q_c| (+ the products that have an fp16-subnormal factor, which the hardware may take as 0), cosine within
 *   (C + 16) 2^-23.
 *   Both carry held-back work out first (as nvbx_flush), run in classic order on the mapper's stream, are asynchronous and write nothing to the map.
 *   NVBX_E_INVALID (nvbx_last_error set, the mapper stays usable): before nvbx_enable_features; Q outside 1 .. 128; an unknown metric; a NULL or
 *   misaligned queries_dev; a NULL required output while capacity_blocks / n is above 0 (count_dev is always required).
 * nvbx_match_features: every block that carries features, one entry per block, entry order unspecified.  block_idx_dev[e] = the block's index;
 *   label_dev[e][512], score_dev[e][512] in the public voxel order t = vx 64 + vy 8 + vz.  A voxel counts when its weight is > 0 and >= min_weight:
 *   label = the query with the highest score (a tie: the lowest query index), score = that score; a voxel that does not count: label -1, score 0.
 *   all_scores_dev: NULL, or [e][512][Q] f32 (0 for voxels that do not count).  *count_dev = the number of feature blocks in the map, also when it
 *   exceeds capacity_blocks; entries at capacity_blocks and beyond are written nowhere; capacity_blocks 0 with NULL outputs only counts.
 * nvbx_match_points: the voxel that contains each point (nvbx_query_features' rule: floor(p / voxel_size) per axis); scores_dev [n][Q],
 *   weight_dev [n] = nvbx_query_features' weight.  Weight 0 and zero scores -- never an error -- where nvbx_query_features returns weight 0.
 *   n == 0 launches nothing.  Chained behind nvbx_cast_rays / nvbx_render_view it gives a relevance image of the map from any pose. */
#define NVBX_MATCH_DOT    0
#define NVBX_MATCH_COSINE 1
int nvbx_match_features(nvbx_mapper* m, const void* queries_dev, int32_t n_queries, int32_t metric, float min_weight,
                        nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev, float* all_scores_dev,
                        int64_t capacity_blocks, int64_t* count_dev);
int nvbx_match_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const void* queries_dev, int32_t n_queries,
                      int32_t metric, float* scores_dev, float* weight_dev);

/* ---- feature segmentation (from matched voxels to a table of 3-D objects; SEMANTICS.md "Feature segmentation") ----------------------
 * nvbx_label_components: connected components of a labelled sparse voxel volume of the shape nvbx_match_features returns -- one entry per
 *   block, distinct block indices in any order, label_dev[e][512] / score_dev[e][512] in the public voxel order t = vx 64 + vy 8 + vz; a label
 *   < 0 is background.  Two voxels are adjacent when their GLOBAL voxel coordinates g = 8 block + v differ by at most 1 on every axis
 *   (connectivity 26) or by exactly 1 on exactly one axis (6), across block borders too; a block that is not in the list separates what lies on
 *   either side of it.  A component is a maximal set of voxels of one label >= 0 connected through adjacent voxels of that label.
 *   component_id_dev[e][512] = the component's index in [0, *count_dev) for every voxel of a component of at least min_voxels voxels, -1 for
 *   background and for smaller components; components_dev[index] = its record.  Index order is unspecified; volume and table agree.
 *   *count_dev = the number of kept components, also when it exceeds capacity_components; records from the capacity on are written nowhere
 *   (the id volume still carries their indices); capacity 0 with a NULL table only counts and labels.  Every record field is an integer, or a
 *   maximum / comparison of stored floats: apart from the index order the result is bit-specified.  Scores compare as floats (-0 as +0, a NaN
 *   as -infinity); without scores (NULL) every score is 0 and peak_xyz is the component's lowest voxel.
 *   n_blocks_dev: NULL, or a device count -- min(n_blocks, *n_blocks_dev) entries are read, the entries behind them neither read nor written.
 *   The call reads nothing from the map, carries out no held-back work and is asynchronous on the mapper's stream.  Its scratch (about 4.1 KiB
 *   per entry) belongs to the mapper and grows on demand: the first call and every call with more entries than any before allocate (and wait
 *   for the stream once).  NVBX_E_INVALID (nvbx_last_error set, nothing launched, the mapper stays usable): connectivity other than 6 / 26;
 *   min_voxels < 1; n_blocks < 0 or > 2^22 (voxel ids are int32); a NULL block_idx_dev / label_dev / component_id_dev while n_blocks > 0; a
 *   NULL count_dev; capacity_components < 0, or > 0 with a NULL or not 8-byte aligned components_dev.  n_blocks == 0 writes a count of 0 and
 *   launches nothing else.  A repeated block index is a precondition violation: the result is still a valid partition, which copy the
 *   neighbours see is unspecified.  Record fields of blocks outside the addressable index range (nvbx_index3d) are unspecified.
 * nvbx_segment_features: queries in, objects out -- nvbx_match_features without the score matrix, then the threshold, then
 *   nvbx_label_components over min(*block_count_dev, capacity_blocks) entries (read on the device), all in stream order without a host wait.
 *   Threshold, in place: where score < min_score_dev[label] (f32; a NaN threshold drops nothing) label becomes -1 and score 0;
 *   min_score_dev: [Q] device floats, or NULL for no threshold.  Refusals: those of both calls (capacity_blocks takes n_blocks' part);
 *   held-back work is handled as in nvbx_match_features. */
typedef struct {
  int32_t label;          /* the common label of its voxels, >= 0 */
  int32_t voxels;         /* how many */
  int32_t min_xyz[3];     /* box in global voxel coordinates g = 8 block + v, inclusive */
  int32_t max_xyz[3];
  int64_t sum_xyz[3];     /* sum of g over its voxels: centroid = (sum / voxels + 0.5) voxel_size */
  float   peak_score;     /* highest score among its voxels (0 without scores) */
  int32_t peak_xyz[3];    /* global voxel of that score; a tie: the lexicographically lowest (x, then y, then z) */
} nvbx_component;         /* 72 bytes, 8-byte aligned; offsets 0 4 8 20 32 56 60 */
int nvbx_label_components(nvbx_mapper* m, const nvbx_index3d* block_idx_dev, const int32_t* label_dev, const float* score_dev,
                          int64_t n_blocks, const int64_t* n_blocks_dev, int32_t connectivity, int32_t min_voxels,
                          int32_t* component_id_dev, nvbx_component* components_dev, int64_t capacity_components, int64_t* count_dev);
int nvbx_segment_features(nvbx_mapper* m, const void* queries_dev, int32_t n_queries, int32_t metric, float min_weight,
                          const float* min_score_dev, int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev,
                          int32_t* label_dev, float* score_dev, int32_t* component_id_dev, int64_t capacity_blocks,
                          int64_t* block_count_dev, nvbx_component* components_dev, int64_t capacity_components,
                          int64_t* component_count_dev);

/* ---- frontiers and view gain (exploration; SEMANTICS.md "Frontiers and view gain") -------------------------------------------------
 * Where known free space ends and the unseen begins, and how much unseen space a pose would look into.  A voxel with stored {d, w} is
 * OBSERVED iff its block carries the TSDF layer and w >= min_weight, FREE iff observed and d > free_distance_m (a NaN d is not free),
 * OCCUPIED iff observed and not free, UNKNOWN otherwise -- every voxel of a block that is not allocated or lies outside the addressable
 * block range included.  All three calls are for TSDF mappers (an occupancy mapper: NVBX_E_INVALID), read TSDF voxels only, leave held-back
 * work held back (as a TSDF nvbx_query_points does), write nothing to the map and are asynchronous on the mapper's stream.  On a refusal
 * (NVBX_E_INVALID, nvbx_last_error set) nothing is launched and the mapper stays usable.
 * nvbx_find_frontiers: a frontier voxel is a free voxel with nu >= min_unknown_neighbours (1 .. 6), nu = the number of unknown voxels among
 *   its six face neighbours in GLOBAL voxel coordinates g = 8 block + v (across block borders), that lies inside box_min_max_vox = {min x, y, z,
 *   max x, y, z} (host memory, inclusive, global voxel coordinates; NULL: unbounded).  The output has the shape nvbx_match_features returns and
 *   feeds nvbx_label_components unchanged: one entry per TSDF block with at least one frontier voxel, entry order unspecified;
 *   block_idx_dev[e] = the block's index; label_dev[e][512] = 0 for a frontier voxel, -1 otherwise; score_dev[e][512] (NULL: not written) =
 *   (float)nu for a frontier voxel, 0 otherwise; voxel order t = vx 64 + vy 8 + vz.  *count_dev = the number of such blocks, also when it
 *   exceeds capacity_blocks; entries from the capacity on are written nowhere; capacity_blocks 0 with NULL arrays only counts; an empty map
 *   writes a count of 0.  Apart from the entry order the result is bit-specified.  Refused: min_unknown_neighbours outside 1 .. 6; a NaN
 *   min_weight or free_distance_m; capacity_blocks < 0 or > 2^22; a NULL count_dev; a NULL block_idx_dev or label_dev with capacity_blocks > 0;
 *   a box with min > max on an axis.
 * nvbx_frontier_clusters: nvbx_find_frontiers, then nvbx_label_components over min(*block_count_dev, capacity_blocks) entries (read on the
 *   device), in stream order without a host wait (the labelling's scratch grows as documented there).  A component's centroid is an
 *   exploration goal, `voxels` the frontier's size, peak_score / peak_xyz its most open voxel.  Refusals: those of both calls.
 * nvbx_view_gain: for each of n_views poses T_L_C_dev[n_views][16] (DEVICE memory, row-major 4 x 4, camera -> layer) the rays of
 *   nvbx_render_view for `camera` at `subsampling` are walked in steps of one voxel size: sample k = 0, 1, ... lies at t_k = (k + 0.5) voxel_size
 *   while t_k < max_range_m, in the voxel that contains o + t_k d (floor(p / voxel_size) per axis, f32).  An unknown sample counts one
 *   unknown_samples, a free one one free_samples, an occupied one ends the ray and counts one rays_hit.  The samples count voxels ALONG RAYS,
 *   not distinct voxels: neighbouring rays may count one voxel twice, and a ray may count a voxel it crosses diagonally more than once.
 *   gains_dev[v] = the sums over the view's rays, rays = rows / s x cols / s.  A pose that is not finite or out of range (nvbx_render_view's
 *   rule) is never an error: its record is all zero with rays = -1.  subsampling 0 / max_range_m <= 0: the mapper's sphere_tracing_subsampling
 *   / sphere_tracing_max_ray_length_m.  Refused: what nvbx_render_view refuses of camera, subsampling and range; n_views < 0; a NULL
 *   T_L_C_dev or gains_dev with n_views > 0; a NaN min_weight or free_distance_m.  n_views == 0 launches nothing. */
typedef struct { int32_t rays, unknown_samples, free_samples, rays_hit; } nvbx_gain;      /* 16 bytes; offsets 0 4 8 12 */
int nvbx_find_frontiers(nvbx_mapper* m, float min_weight, float free_distance_m, int32_t min_unknown_neighbours,
                        const int32_t box_min_max_vox[6], nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev,
                        int64_t capacity_blocks, int64_t* count_dev);
int nvbx_frontier_clusters(nvbx_mapper* m, float min_weight, float free_distance_m, int32_t min_unknown_neighbours,
                           const int32_t box_min_max_vox[6], int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev,
                           int32_t* label_dev, float* score_dev, int32_t* component_id_dev, int64_t capacity_blocks,
                           int64_t* block_count_dev, nvbx_component* components_dev, int64_t capacity_components,
                           int64_t* component_count_dev);
int nvbx_view_gain(nvbx_mapper* m, const float* T_L_C_dev, int32_t n_views, const nvbx_camera* camera, int32_t subsampling,
                   float max_range_m, float min_weight, float free_distance_m, nvbx_gain* gains_dev);

/* ---- cost field and paths (which goal can be reached, and how far is the drive; SEMANTICS.md "Cost field and paths") -----------------
 * Over a distance image image_dev[rows][cols] (DEVICE memory, f32, row = y, col = x) as nvbx_esdf_slice_to_image and
 * nvbx_esdf_slice_combined_to_image write it, with their unknown_value -- or any image of that form.  `options` is host memory.  A pixel with
 * stored value v is UNKNOWN iff fabsf(v - unknown_value) < 1e-2f (nvbx_occupancy_grid_from_slice's test), TRAVERSABLE iff it is not unknown,
 * v > 0 and v >= robot_radius_m (a NaN v is not), and with allow_unknown != 0 an unknown pixel is traversable too.  A traversable pixel's
 * penalty: t = inflation_radius_m - v; 0 if !(t > 0); else u = penalty_per_m * t and max_penalty if !(u < (float)max_penalty), else
 * (int32_t)u; a traversable unknown pixel's is unknown_penalty.  A move goes from a traversable pixel p to a traversable 8-neighbour q inside
 * the image, diagonally only if both pixels that share an edge with p and q are traversable, and costs B + pen(p) + pen(q), B = 10 along an
 * axis, 14 diagonally.  Both calls read the image only and write their outputs only: the map is untouched, held-back work stays held back.
 * On a refusal (NVBX_E_INVALID, nvbx_last_error set) nothing is launched and the mapper stays usable.  Refused by both: a NULL mapper, image,
 * options or field; rows or cols <= 0 or rows x cols > 2^22; a NaN or negative robot_radius_m, inflation_radius_m or penalty_per_m; a NaN
 * unknown_value; max_penalty or unknown_penalty outside 0 .. 200 (a step then costs at most 414, and 414 x 2^22 < 2^31: no sum overflows).
 * nvbx_cost_field: cost_dev[rows][cols] = the least total cost of a move sequence from any accepted source to the pixel: 0 at a source,
 *   NVBX_COST_UNREACHED where there is none and at every pixel that is not traversable.  sources_rc_dev[n_sources][2] = (row, col), DEVICE
 *   memory; one outside the image or on a pixel that is not traversable is ignored, duplicates are harmless, none accepted: all UNREACHED.
 *   *accepted_dev (NULL: not wanted) = the number of accepted entries.  The field is the unique fixed point of an integer relaxation and
 *   bit-specified.  The call enqueues relaxation rounds in batches on the mapper's stream and WAITS for the device after each batch to read
 *   one counter: it returns with the field complete (everything enqueued on the stream before it has then run as well).  NVBX_E_DEVICE with
 *   a message if rows x cols rounds did not reach the fixed point, which the algorithm excludes.  Also refused: n_sources < 0; a NULL
 *   sources_rc_dev with n_sources > 0.
 * nvbx_trace_paths: for each of n_starts pixels starts_rc_dev[i] = (row, col) the path that descends cost_dev, a field of this image and
 *   these options: it begins at the start; at p with 0 < G(p) < UNREACHED the next pixel is the FIRST allowed neighbour q in the order (drow,
 *   dcol) = (0,1) (1,0) (0,-1) (-1,0) (1,1) (1,-1) (-1,-1) (-1,1) with G(q) + c(p, q) == G(p); it ends at the first pixel with G = 0, which
 *   is included.  path_rc_dev[i][capacity][2] receives the pixels, length_dev[i] their number -- also when it exceeds `capacity`; pixels from
 *   the capacity on are written nowhere -- 0 for a start outside the image or UNREACHED, -1 if no neighbour satisfies the equation (the field
 *   is not one of this image and these options; never an error code).  One lane per start, at most rows x cols steps, asynchronous on the
 *   mapper's stream.  Also refused: n_starts < 0; capacity < 0; a NULL starts_rc_dev, path_rc_dev or length_dev with n_starts > 0.
 *   n_starts == 0 launches nothing. */
#define NVBX_COST_UNREACHED 0x7fffffff
typedef struct {
  float robot_radius_m;        /* 0.25 */
  float inflation_radius_m;    /* 0.75 */
  float penalty_per_m;         /* 100 */
  float unknown_value;         /* 1000: what the slice call was given */
  int32_t max_penalty;         /* 200 */
  int32_t unknown_penalty;     /* 50 */
  int32_t allow_unknown;       /* 0 */
  int32_t pad;
} nvbx_cost_options;            /* 32 bytes; offsets 0 4 8 12 16 20 24 28 */
void nvbx_default_cost_options(nvbx_cost_options* options);
int nvbx_cost_field(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                    const int32_t* sources_rc_dev, int32_t n_sources, int32_t* cost_dev, int32_t* accepted_dev);
int nvbx_trace_paths(nvbx_mapper* m, const float* image_dev, int32_t rows, int32_t cols, const nvbx_cost_options* options,
                     const int32_t* cost_dev, const int32_t* starts_rc_dev, int32_t n_starts, int32_t* path_rc_dev, int32_t capacity,
                     int32_t* length_dev);

/* ---- cost volume and 3-D paths (which goal can be reached through free space, and what does the flight cost; SEMANTICS.md "Cost volume
 *      and 3-D paths") ----------------------------------------------------------------------------------------------------------------------
 * The cost field over a distance VOLUME volume_dev[nx][ny][nz] (DEVICE memory, f32, element (x, y, z) at (x * ny + y) * nz + z): exactly
 * what nvbx_esdf_dense_grid writes for size_vox = {nx, ny, nz} with default_value = the options' unknown_value -- or any volume of that
 * form.  `options` is host memory; the voxel classes and penalties are those of the cost field above, unchanged (UNKNOWN iff fabsf(v -
 * unknown_value) < 1e-2f; TRAVERSABLE iff not unknown, v > 0 and v >= robot_radius_m; a negative v and a NaN are not; allow_unknown makes
 * unknown voxels traversable with unknown_penalty).  There are 26 moves d = (dx, dy, dz), components in {-1, 0, 1}, not all 0.  With k =
 * the number of nonzero components, a move from a traversable p to a traversable q = p + d inside the volume costs B_k + pen(p) + pen(q),
 * B_1 = 10, B_2 = 14, B_3 = 17, and is allowed iff every voxel p + e is traversable, for each e with e_i in {0, d_i}, e != 0, e != d: the
 * two voxels beside a face diagonal, the six around a space diagonal; a voxel outside the volume is not traversable.  Nothing squeezes
 * between two blocked voxels that touch along an edge or at a corner.  ORDER of the moves: by k, then lexicographically by (dx, dy, dz)
 * with each component ordered +1, 0, -1 -- (1,0,0) (0,1,0) (0,0,1) (0,0,-1) (0,-1,0) (-1,0,0), then (1,1,0) (1,0,1) (1,0,-1) (1,-1,0)
 * (0,1,1) (0,1,-1) (0,-1,1) (0,-1,-1) (-1,1,0) (-1,0,1) (-1,0,-1) (-1,-1,0), then (1,1,1) (1,1,-1) (1,-1,1) (1,-1,-1) (-1,1,1) (-1,1,-1)
 * (-1,-1,1) (-1,-1,-1).  Both calls read the volume only and write their outputs only: the map is untouched, held-back work stays held
 * back.  On a refusal (NVBX_E_INVALID, nvbx_last_error set) nothing is launched and the mapper stays usable.  Refused by both: a NULL mapper,
 * volume, options or field; nx, ny or nz <= 0 or nx x ny x nz > 2^22 (a step costs at most 17 + 2 x 200 = 417, and 417 x 2^22 < 2^31: no
 * sum overflows); the options the cost field refuses.
 * nvbx_cost_volume: cost_dev[nx][ny][nz], int32 in the volume's layout = the least total cost of a move sequence from any accepted source
 *   to the voxel: 0 at a source, NVBX_COST_UNREACHED where there is none and at every voxel that is not traversable.
 *   sources_xyz_dev[n_sources][3] = (x, y, z) offsets in the box, DEVICE memory; one outside the box or on a voxel that is not traversable
 *   is ignored, duplicates are harmless, none accepted: all UNREACHED.  *accepted_dev (NULL: not wanted) = the number of accepted entries.
 *   The field is the unique fixed point of an integer relaxation and bit-specified.  The call enqueues relaxation rounds in batches on the
 *   mapper's stream and WAITS for the device after each batch to read one counter: it returns with the field complete.  NVBX_E_DEVICE with
 *   a message if nx x ny x nz rounds plus one batch did not reach the fixed point, which the algorithm excludes.  Also refused:
 *   n_sources < 0; a NULL sources_xyz_dev with n_sources > 0.
 * nvbx_trace_paths_3d: for each of n_starts voxels starts_xyz_dev[i] = (x, y, z) the path that descends cost_dev, a field of this volume
 *   and these options: it begins at the start; at p with 0 < G(p) < UNREACHED the next voxel is the FIRST allowed neighbour q in the order
 *   above with G(q) + c(p, q) == G(p); it ends at the first voxel with G = 0, which is included.  path_xyz_dev[i][capacity][3] receives
 *   the voxels, length_dev[i] their number -- also when it exceeds `capacity`; voxels from the capacity on are written nowhere -- 0 for a
 *   start outside the box or UNREACHED, -1 if no neighbour satisfies the equation (the field is not one of this volume and these options;
 *   never an error code).  One lane per start, at most nx x ny x nz steps, asynchronous on the mapper's stream.  Also refused:
 *   n_starts < 0; capacity < 0; a NULL starts_xyz_dev, path_xyz_dev or length_dev with n_starts > 0.  n_starts == 0 launches nothing. */
int nvbx_cost_volume(nvbx_mapper* m, const float* volume_dev, int32_t nx, int32_t ny, int32_t nz, const nvbx_cost_options* options,
                     const int32_t* sources_xyz_dev, int32_t n_sources, int32_t* cost_dev, int32_t* accepted_dev);
int nvbx_trace_paths_3d(nvbx_mapper* m, const float* volume_dev, int32_t nx, int32_t ny, int32_t nz, const nvbx_cost_options* options,
                        const int32_t* cost_dev, const int32_t* starts_xyz_dev, int32_t n_starts, int32_t* path_xyz_dev,
                        int32_t capacity, int32_t* length_dev);

/* ---- elevation and traversability (how high is the ground here, can the robot stand here, how far is the next place where it cannot;
 *      SEMANTICS.md "Elevation and traversability") -------------------------------------------------------------------------------------
 * Per-column products of the TSDF layer, pixel-aligned with the slice image: pixel (r, c) is the voxel column gx = x0 + c, gy = y0 + r in
 * global voxel coordinates g = 8 block + v (row = y, col = x), the band is gz in [z_lo, z_hi], both included.  All image pointers are
 * DEVICE memory, row-major [rows][cols]; `options` is host memory.  Both calls are for TSDF mappers, read only, asynchronous on the
 * mapper's stream with no host wait inside, and leave held-back work held back.  On a refusal (NVBX_E_INVALID, nvbx_last_error set)
 * nothing is launched and the mapper stays usable.
 * nvbx_elevation_map: a voxel with stored {d, w} is OBSERVED iff its block is allocated and carries the TSDF layer, w >= min_weight and
 *   d == d (a NaN weight or distance is not observed), SOLID iff observed and d <= 0, FREE iff observed and d > 0, all in f32.  With zt =
 *   the largest gz of the band whose voxel is solid, status_dev = NVBX_ELEV_UNKNOWN: no observed voxel in the band; NVBX_ELEV_SURFACE: zt
 *   exists, zt + 1 <= z_hi and voxel zt + 1 is observed (then free); NVBX_ELEV_BLOCKED: zt exists without that (the solid reaches the
 *   band's top, or what lies above it is unobserved); NVBX_ELEV_VOID: observed voxels, none solid.  height_dev of a SURFACE pixel, with
 *   d0 = d(zt), d1 = d(zt + 1) and vs the voxel size: (((float)bz * (8 vs) + (float)vz * vs) + vs * 0.5f) + vs * (-d0 / (d1 - d0)), bz =
 *   zt >> 3, vz = zt & 7, in f32 in this order without contraction (nvbx_tsdf_zero_crossings' expression); of every other pixel:
 *   unknown_value.  Both images are fully written and bit-specified; an empty map gives all UNKNOWN.  Refused: a NULL mapper or output;
 *   an occupancy mapper; rows or cols <= 0 or rows x cols > 2^22; z_hi < z_lo or z_hi - z_lo >= 1024; a box that leaves [-2^23, 2^23)
 *   voxels on an axis (the addressable blocks times 8); a NaN min_weight or unknown_value.
 * nvbx_traversability: over such a pair of images (of this call or drawn by the caller; the map is not read).  A pixel is KNOWN iff its
 *   status is SURFACE -- the status decides, no test on the height.  All arithmetic f32 in the order written, vs = the mapper's voxel
 *   size.  n_known(p) = the known pixels among the 3 x 3 around p inside the image, p included.  step(p), p known = the largest
 *   fabsf(h(p) - h(q)) over the known 8-neighbours q (none: 0).  gx(p), p known = (h(r, c+1) - h(r, c-1)) / (2.0f * vs) if both are
 *   known, else (h(r, c+1) - h(p)) / vs if the right one is, else (h(p) - h(r, c-1)) / vs if the left one is, else 0; gy(p) likewise
 *   along rows; slope2 = gx * gx + gy * gy.  step and slope2 of a pixel that is not known are 0.  class_dev = NVBX_TERRAIN_UNKNOWN:
 *   status UNKNOWN, and VOID with void_is_hazard == 0; NVBX_TERRAIN_HAZARD: status BLOCKED, VOID with void_is_hazard != 0, a known pixel
 *   with !(step <= max_step_m) or !(slope2 <= max_slope_tan * max_slope_tan) or n_known < min_known; NVBX_TERRAIN_OK: every other known
 *   pixel.  distance_dev, R = distance_radius_px: unknown_value on an UNKNOWN pixel, 0 on a HAZARD pixel; an OK pixel takes m = the least
 *   dr * dr + dc * dc over the HAZARD pixels inside the image with dr * dr + dc * dc <= R * R and gets vs * sqrtf((float)m), or
 *   vs * (float)(R + 1) if there is none (m is an integer minimum and the root correctly rounded: bit-specified whatever the order of
 *   the search).  The distance image has the form nvbx_cost_field reads.  (With a distance image the first call, and any with more
 *   rows x ceil(cols / 64) than every earlier one, grows a mapper-owned scratch buffer and waits for the stream once while it does.)  step_dev, slope2_dev and distance_dev may be NULL: not
 *   wanted.  Refused: a NULL mapper, height_dev, status_dev, options or class_dev; rows / cols as above; a NaN or negative max_step_m
 *   or max_slope_tan; a NaN unknown_value; min_known outside 1 .. 9; distance_radius_px outside 0 .. 32. */
#define NVBX_ELEV_UNKNOWN 0
#define NVBX_ELEV_SURFACE 1
#define NVBX_ELEV_BLOCKED 2
#define NVBX_ELEV_VOID 3
#define NVBX_TERRAIN_UNKNOWN 0
#define NVBX_TERRAIN_OK 1
#define NVBX_TERRAIN_HAZARD 2
typedef struct {
  float max_step_m;            /* 0.10 */
  float max_slope_tan;         /* 0.5 */
  float unknown_value;         /* 1000: what nvbx_cost_field will be told */
  int32_t min_known;           /* 5 */
  int32_t void_is_hazard;      /* 0 */
  int32_t distance_radius_px;  /* 15 */
  int32_t pad[2];
} nvbx_terrain_options;         /* 32 bytes; offsets 0 4 8 12 16 20 24 */
void nvbx_default_terrain_options(nvbx_terrain_options* options);
int nvbx_elevation_map(nvbx_mapper* m, int32_t x0, int32_t y0, int32_t rows, int32_t cols, int32_t z_lo, int32_t z_hi, float min_weight,
                       float unknown_value, float* height_dev, uint8_t* status_dev);
int nvbx_traversability(nvbx_mapper* m, const float* height_dev, const uint8_t* status_dev, int32_t rows, int32_t cols,
                        const nvbx_terrain_options* options, uint8_t* class_dev, float* step_dev, float* slope2_dev, float* distance_dev);

/* ---- map file (Mapper::saveLayerCake(path) -> bool, loadMap(path) -> bool: nvblox_node.cpp:1663-1668,1698-1703) -----------------
 * A path ending in .nvblx is written as an SQLITE database, like the reference's layer cake: table layers(layer_type, voxel_size,
 * block_size, voxel_bytes, num_blocks) + one table <layer_type>_blocks(index_x, index_y, index_z, data BLOB) per layer (tsdf_layer,
 * color_layer, esdf_layer, occupancy_layer; data = 512 reference voxel structs).  [U] The schema is a guess at upstream's (the
 * serializer lives in the absent core): files open with any sqlite3 tool, interoperability with upstream's reader is unverified.
 * libsqlite3 is loaded at run time; any other path (or no libsqlite3) uses a compact little-endian container of our own.  load
 * recognises either by its magic and replaces the map: it is cleared first, the file's voxel size must equal the mapper's, loaded TSDF
 * blocks are ESDF- and mesh-dirty.  Errors: NVBX_E_IO, NVBX_E_INVALID (voxel size), NVBX_E_CAPACITY; a file that fails validation
 * leaves the current map untouched. */
int nvbx_save_map(nvbx_mapper* m, const char* path);
int nvbx_load_map(nvbx_mapper* m, const char* path);

/* ---- sensor-side conversions next to the path -----------------------------------------------------------------------
 * DepthImageBackProjector::backProjectOnGPU(depth, camera, &pointcloud_C, max_back_projection_distance) --
 * nvblox_node.cpp:1128-1130, fuser_node.cpp:294-296: every pixel with 0 < depth <= max_distance_m (max <= 0: no limit)
 * becomes the point ((u + 0.5 - cu) / fu * d, (v + 0.5 - cv) / fv * d, d) of the camera frame; the points are compacted
 * (order unspecified) into points_xyz_dev[capacity_points][3]; *n_points = their number (synchronises). */
int nvbx_backproject_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const nvbx_camera* camera,
                           float max_distance_m, float* points_xyz_dev, int64_t capacity_points, int64_t* n_points);
/* transformPointcloudOnGPU(T_L_C, pointcloud_C, &pointcloud_L) -- nvblox_node.cpp:1131, fuser_node.cpp:297 (in place if
 * out == in; asynchronous on the mapper's stream) */
int nvbx_transform_pointcloud(nvbx_mapper* m, const float T_L_C[16], const float* points_in_dev, int64_t n_points, float* points_out_dev);

/* ---- pose alignment ([U] frame-to-model refinement against the TSDF; SEMANTICS.md "Pose alignment") ---------------------------------
 * Refines a sensor pose so that the sensor's points lie on the TSDF's zero level: Gauss-Newton on sum w r^2 with r = the trilinear TSDF
 * interpolant of nvbx_query_points at T x and its analytic gradient.  A refinement from a guess within the truncation band, not a
 * relocalisation.  The pose is held in f64 on the device; every iteration is an accumulate launch (one lane per point, 29 f64 sums, a
 * fixed reduction order: bit-identical from run to run) and a one-workgroup solve launch (6 x 6 Cholesky, exponential map, pose update,
 * status).  All launches of a call are enqueued at once on the mapper's stream: no host wait, the launches behind a final status
 * return at once.  The calls read TSDF voxels only and leave held-back work held back (as a TSDF nvbx_query_points does).
 * One linearization at T, over the n sensor-frame points x: Tf = T rounded to f32; p = Tf x in nvbx_transform_pointcloud's f32
 * arithmetic; (d, g, valid) = nvbx_query_points(TSDF, min_weight) at p; then in f64 r = d, q = p - Tf.t, J = [g, q x g],
 * w = 1 if huber_delta_m <= 0 or |r| <= huber_delta_m else huber_delta_m / |r|; over the valid points H += (w J) J^T (upper triangle,
 * row-major: 21 numbers), b += (w J) r, cost += (w r) r, n_valid += 1.
 * One step: (H + damping diag(H)) xi = -b by Cholesky, xi = (v, omega); R <- exp([omega]x) R, t <- t + V(omega) v.
 * Status: NVBX_ALIGN_TOO_FEW when n_valid < min_valid, NVBX_ALIGN_DEGENERATE when a pivot is <= min_pivot_ratio x max diag(H) -- neither
 * applies a step, a failure in the first iteration returns the guess bit for bit; NVBX_ALIGN_CONVERGED after an applied step with
 * |v| <= stop_translation_m and |omega| <= stop_rotation_rad; NVBX_ALIGN_MAX_ITERATIONS after max_iterations linearizations. */
#define NVBX_ALIGN_CONVERGED      1
#define NVBX_ALIGN_MAX_ITERATIONS 2
#define NVBX_ALIGN_TOO_FEW        3
#define NVBX_ALIGN_DEGENERATE     4
#define NVBX_ALIGN_LINEARIZED     5   /* nvbx_linearize_points: one linearization, a solvable system, no step applied */
typedef struct {
  int32_t max_iterations;       /* 1 .. 64 linearizations */
  int32_t subsampling;          /* nvbx_align_depth: pixels (r s, c s); >= 1 */
  float   min_weight;           /* a TSDF corner counts with weight >= this */
  float   huber_delta_m;        /* <= 0: plain least squares */
  double  damping;              /* >= 0: (H + damping diag(H)) */
  double  min_pivot_ratio;      /* >= 0 */
  double  stop_translation_m;
  double  stop_rotation_rad;
  int32_t min_valid;            /* >= 1 */
  float   max_depth_m;          /* nvbx_align_depth: pixels with 0 < depth <= this; <= 0: no limit */
} nvbx_align_options;           /* 56 bytes; offsets 0 4 8 12 16 24 32 40 48 52 */
typedef struct {
  double  H[21];                /* upper triangle, row-major */
  double  b[6];
  double  cost;                 /* sum w r^2 */
  int32_t n_valid;
  int32_t pad;
} nvbx_align_sums;              /* 232 bytes */
typedef struct {
  float   T_L_S[16];            /* the refined pose, row-major 4 x 4, rounded to f32 */
  double  T64[16];              /* the same in f64 */
  double  step[6];              /* the last step solved for, (v, omega); 0 where none was */
  nvbx_align_sums first;        /* the sums of the first linearization (at the guess) ... */
  nvbx_align_sums last;         /* ... and of the last one (the pose it was taken at: T64 before the last applied step) */
  int32_t iterations;           /* linearizations carried out */
  int32_t status;               /* NVBX_ALIGN_* */
} nvbx_align_result;            /* 712 bytes, 8-byte aligned DEVICE memory; offsets 0 64 192 240 472 704 708 */
/* defaults: 10 iterations, subsampling 4, min_weight 1e-4, huber 0, damping 0, min_pivot_ratio 1e-9, stop 1e-5 m / 1e-5 rad, min_valid 50, no depth limit */
void nvbx_default_align_options(nvbx_align_options* options);
/* nvbx_align_points: any sensor-frame cloud points_xyz_dev[n][3] (LiDAR included), from T_L_S_guess (row-major 4 x 4, host memory).
 * nvbx_align_depth: the pixels (r s, c s) of depth_dev[rows][cols] with 0 < depth <= max_depth_m, back-projected with
 *   nvbx_backproject_depth's arithmetic inside the launch; no point buffer is written.
 * nvbx_linearize_points: one linearization at T_L_S, no step is applied (result: T = T_L_S, step = what the solve gives, first = last,
 *   iterations 1, status TOO_FEW / DEGENERATE / LINEARIZED); optional per-point outputs (NULL: not written): points_L_dev[n][3],
 *   residual_dev[n], gradient_dev[n][3], valid_dev[n] -- bit for bit nvbx_transform_pointcloud and nvbx_query_points (unknown_value 0).
 * options NULL: the defaults.  result_dev: 8-byte aligned device memory, written by the launches.  Asynchronous on the mapper's stream.
 * n == 0: NVBX_ALIGN_TOO_FEW, the accumulate launch is skipped.  NVBX_E_INVALID (nvbx_last_error set, nothing launched, the mapper stays
 * usable): an occupancy mapper; a NULL mapper, pose, result or (n > 0) point / depth pointer; n < 0; a misaligned result_dev; a pose that is
 * not finite or out of range; image sides outside 1 .. 32768; a camera that does not match the image; max_iterations outside 1 .. 64;
 * subsampling < 1; min_valid < 1;
 * damping / min_pivot_ratio / a stop threshold negative or not finite; min_weight, huber_delta_m or max_depth_m not a number. */
int nvbx_align_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T_L_S_guess[16], const nvbx_align_options* options,
                      nvbx_align_result* result_dev);
int nvbx_align_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C_guess[16], const nvbx_camera* camera,
                     const nvbx_align_options* options, nvbx_align_result* result_dev);
int nvbx_linearize_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T_L_S[16], const nvbx_align_options* options,
                          nvbx_align_result* result_dev, float* points_L_dev, float* residual_dev, float* gradient_dev, uint8_t* valid_dev);

/* ---- pose alignment with a colour term ([U]; SEMANTICS.md "Colour alignment and colour queries") ----------------------------------------
 * The calls above with a photometric term beside the geometric one, for frames whose geometry lets the pose slide (a wall, a floor).  Every
 * point carries an rgb8 colour: colors_rgb_dev[n][3] beside a cloud, color_rgb_dev[rows][cols][3] (the depth's pixels) beside a depth image;
 * Ys = its luminance (77 r + 150 g + 29 b) / 256.  For a point whose geometric term is valid and whose colour query
 * (Y, gY, valid) = nvbx_query_colors(min_color_weight) at the same p is valid, in f64: e = Y - Ys (levels), kappa = voxel_size / 255,
 * r_c = kappa e, J_c = kappa [gY, q x gY], w_c = 1 if color_huber_levels <= 0 or |e| <= color_huber_levels else color_huber_levels / |e|;
 * H += (color_weight w_c J_c) J_c^T, b += (color_weight w_c J_c) r_c -- added to the same H and b after the point's geometric products --
 * color_cost += (w_c e) e, n_color += 1.  A full-range intensity step across one voxel has |kappa gY| = 1, the TSDF gradient's magnitude:
 * color_weight 1 weighs such an edge like a surface.  cost and n_valid of nvbx_align_sums stay the geometric ones; the solve, its statuses and
 * the 712-byte result record are the plain calls', over the joint system.  With color_weight 0 the result record is the plain call's bit for
 * bit.  The calls read the colour layer: held-back colour work is carried out first.
 * Refused: what the plain calls refuse, in their order; then a NULL colour pointer (n > 0, or an image); a NULL or misaligned
 * color_result_dev; a color_weight that is negative or not finite; a min_color_weight / color_huber_levels that is not a number. */
typedef struct {
  float   color_weight;         /* lambda >= 0 */
  float   min_color_weight;     /* a colour corner counts with weight >= this */
  float   color_huber_levels;   /* <= 0: plain least squares */
  int32_t pad;
} nvbx_align_color_options;     /* 16 bytes; offsets 0 4 8 12 */
typedef struct {
  double  color_cost_first, color_cost_last;      /* sum w_c e^2 (levels^2) of the first and of the last linearization */
  int32_t n_color_first, n_color_last;            /* points with a colour term */
} nvbx_align_color_result;      /* 24 bytes, 8-byte aligned DEVICE memory; offsets 0 8 16 20 */
/* defaults: color_weight 1, min_color_weight 1e-4, no Huber weighting */
void nvbx_default_align_color_options(nvbx_align_color_options* options);
int nvbx_align_points_color(nvbx_mapper* m, const float* points_xyz_dev, const uint8_t* colors_rgb_dev, int64_t n, const float T_L_S_guess[16],
                            const nvbx_align_options* options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                            nvbx_align_color_result* color_result_dev);
int nvbx_align_depth_color(nvbx_mapper* m, const float* depth_dev, const uint8_t* color_rgb_dev, int32_t rows, int32_t cols, const float T_L_C_guess[16],
                           const nvbx_camera* camera, const nvbx_align_options* options, const nvbx_align_color_options* color_options,
                           nvbx_align_result* result_dev, nvbx_align_color_result* color_result_dev);
/* the per-point outputs (each NULL: not written) of nvbx_linearize_points, and luminance_dev[n], color_gradient_dev[n][3], color_valid_dev[n]:
 * bit for bit nvbx_query_colors at points_L_dev */
int nvbx_linearize_points_color(nvbx_mapper* m, const float* points_xyz_dev, const uint8_t* colors_rgb_dev, int64_t n, const float T_L_S[16],
                                const nvbx_align_options* options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                                nvbx_align_color_result* color_result_dev, float* points_L_dev, float* residual_dev, float* gradient_dev,
                                uint8_t* valid_dev, float* luminance_dev, float* color_gradient_dev, uint8_t* color_valid_dev);

/* ---- relocalisation ([U] scoring pose hypotheses against the TSDF; SEMANTICS.md "Relocalisation") ----------------------------------------
 * Where nvbx_align_* refine a guess within the truncation band, these calls find such a guess: they score many sensor poses against the
 * TSDF in one launch, and nvbx_relocalize_* score a lattice of poses around T0, select the best and refine it with the alignment's own
 * iterations, without a host wait in between.
 * One pose, one taken point x (nvbx_score_poses_points: all n points; nvbx_score_poses_depth: the pixels (r s, c s) with
 * 0 < depth <= max_depth_m, back-projected with nvbx_backproject_depth's arithmetic inside the launch): p = T x in
 * nvbx_transform_pointcloud's f32 arithmetic with the pose's f32 entries; (d, valid) = nvbx_query_points(TSDF, min_weight) at p, bit for
 * bit (a non-finite point or a missing corner is not valid).  The record of the pose, all integers, so that every summation order gives the
 * same bits: points = the taken points, valid = the valid ones, inliers = valid with |d| <= inlier_distance_m, conflicts = valid with
 * d > conflict_distance_m (a measured surface point in observed free space: evidence against the pose), abs_residual_q20 = the sum over
 * the valid points of (int64)rintf(|d| * 1048576.0f) (round to even).
 * A pose that is not finite or out of range (nvbx_render_view's rule) is never an error: its record is all zero with points = -1.
 * Options: a threshold <= 0 selects its default -- inlier_distance_m one voxel size, conflict_distance_m half the truncation distance,
 * min_weight 1e-4; max_depth_m <= 0: no limit; options NULL: the defaults.  n_poses == 0 launches nothing.  Asynchronous on the mapper's
 * stream; TSDF voxels are read, nothing is written to the map, held-back work stays held back.
 * NVBX_E_INVALID (nvbx_last_error set, nothing launched, the mapper stays usable): an occupancy mapper; a NULL mapper, or a NULL point /
 * depth, pose or score pointer that a count > 0 needs; n < 0 or n_poses < 0; a misaligned scores_dev; subsampling < 1; a camera that does
 * not match the image; an option that is not a number. */
typedef struct { int32_t points, valid, inliers, conflicts; int64_t abs_residual_q20; } nvbx_pose_score;   /* 24 bytes, 8-byte aligned; offsets 0 4 8 12 16 */
typedef struct { float min_weight, inlier_distance_m, conflict_distance_m, max_depth_m; int32_t subsampling; } nvbx_score_options;   /* 20 bytes; offsets 0 4 8 12 16 */
/* defaults: the three thresholds 0 (= their defaults, above), no depth limit, subsampling 4 */
void nvbx_default_score_options(nvbx_score_options* options);
/* T_L_S_dev / T_L_C_dev: [n_poses][16] f32, row-major 4 x 4, DEVICE memory; scores_dev[n_poses]: 8-byte aligned device memory */
int nvbx_score_poses_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float* T_L_S_dev, int32_t n_poses,
                            const nvbx_score_options* options, nvbx_pose_score* scores_dev);
int nvbx_score_poses_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const nvbx_camera* camera, const float* T_L_C_dev,
                           int32_t n_poses, const nvbx_score_options* options, nvbx_pose_score* scores_dev);
/* The lattice around T0 (row-major 4 x 4, host memory): steps[0..3] = (nx, ny, nz, nyaw), each 1 .. 64, product K <= 2^20.  Hypothesis
 * h = ((ix ny + iy) nz + iz) nyaw + iw has t_h = t0 + (dx[ix], dy[iy], dz[iz]) (three f32 additions; offsets along the layer's axes) and
 * R_h = Rz(yaw[iw]) R0 (about the layer's z through the sensor origin).  Offset i of s steps over +-half: 0 for s == 1, else
 * -half + (2 half i) / (s - 1) in f64, rounded once to f32 for the translations.  R_h in f64 from R0's f32 entries, c = cos(yaw), s = sin(yaw):
 * row 0 = c R0[0] - s R0[1], row 1 = s R0[0] + c R0[1], row 2 = R0[2], rounded once to f32.  The tables are made on the host
 * (csrc/nvbx_relocalize_math.h); the device only picks entries and adds.  nvbx_search_lattice_poses writes the K poses [K][16] into host
 * memory and returns K, or NVBX_E_INVALID for a lattice or T0 the relocalisation would refuse (but for the range of T0). */
typedef struct { float half_extent_m[3]; float half_yaw_rad; int32_t steps[4]; } nvbx_search_lattice;   /* 32 bytes; offsets 0 12 16 */
#define NVBX_RELOC_OK           0
#define NVBX_RELOC_NO_CANDIDATE 1
typedef struct {
  int32_t status;               /* NVBX_RELOC_* */
  int32_t best_index;           /* h of the selected hypothesis */
  nvbx_pose_score coarse;       /* its record */
  float   T_coarse[16];         /* its pose */
  nvbx_pose_score refined;      /* the record of align.T_L_S; zero with NVBX_RELOC_NO_CANDIDATE */
  nvbx_align_result align;      /* what nvbx_align_* from T_coarse leaves; zero with NVBX_RELOC_NO_CANDIDATE */
} nvbx_relocalize_result;       /* 832 bytes, 8-byte aligned DEVICE memory; offsets 0 4 8 32 96 120 */
/* nvbx_relocalize_points / _depth: four steps enqueued at once.  (1) The lattice is scored as above (score_options), into scores_dev[K]
 * if that is not NULL.  (2) Selection: the hypothesis with the largest key = inliers - conflicts; ties go to more inliers, then to the
 * lowest h.  If its inliers < min_inliers (<= 0: the default 50) the status is NVBX_RELOC_NO_CANDIDATE, best_index / coarse / T_coarse
 * still describe it, refined and align are zero and nothing further runs.  (3) The iterations of nvbx_align_points / _depth
 * (align_options) from T_coarse, read on the device: `align` is bit for bit what that call leaves with T_coarse as the host guess.
 * (4) One scoring launch of align.T_L_S into `refined`.  Refused: what scoring and alignment refuse; steps outside 1 .. 64 or a product
 * above 2^20; a half-extent that is negative or not finite; a T0 that is not finite or out of range; a NULL or misaligned result_dev. */
int nvbx_search_lattice_poses(const float T0[16], const nvbx_search_lattice* lattice, float* T_out_host);
int nvbx_relocalize_points(nvbx_mapper* m, const float* points_xyz_dev, int64_t n, const float T0[16], const nvbx_search_lattice* lattice,
                           const nvbx_score_options* score_options, int32_t min_inliers, const nvbx_align_options* align_options,
                           nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev);
int nvbx_relocalize_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const nvbx_camera* camera, const float T0[16],
                          const nvbx_search_lattice* lattice, const nvbx_score_options* score_options, int32_t min_inliers,
                          const nvbx_align_options* align_options, nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev);

/* ---- map merging ([U] submap fusion under a rigid transform; SEMANTICS.md "Map merging") ----------------------------------------------
 * Brings the TSDF and colour of `src` into `dst` under p_D = T_D_S p_S: every voxel of every candidate block of dst (the blocks whose voxel
 * centres can fall into the sampling cube of a TSDF block of src; missing ones are allocated) samples src at R_SD p_D + t_SD with the rule of
 * the TSDF point query (eight corners, each with weight >= min_weight), the weights interpolated the same way and multiplied by
 * weight_scale; a valid sample is fused as a weighted mean, clamped to +-truncation and dst's max_weight; an invalid one leaves the voxel
 * untouched.  With merge_color the nearest source colour voxel is blended into dst's.  Band flags, ESDF-dirty and mesh-dirty lists of dst
 * are kept as by any TSDF writer; src is not modified.  Both mappers: TSDF mappers (projective_layer_type 0) on one device with one
 * voxel_size.  ESDF, occupancy and freespace are not merged; feature voxels by a call of their own (nvbx_merge_features below).
 * Launches run on dst's stream, ordered behind everything enqueued on src's so far; work enqueued on src afterwards is ordered behind the
 * merge's reads.  A maintenance call: it waits on the host for src's block count and, once, between enumerating the candidates and
 * allocating them (dst's pools grow if they must).  NVBX_E_CAPACITY (dst unchanged): dst's max_capacity cannot hold the candidates.
 * NVBX_E_INVALID (nvbx_last_error set, dst unchanged): src == dst; different devices or voxel sizes; an occupancy or freespace mapper; a
 * pose that is not finite, out of range or no rotation (|R^T R - I| > 1e-5 or det <= 0); min_weight not a number; weight_scale not finite
 * or <= 0; a NULL or misaligned result_dev. */
#define NVBX_MERGE_OK           0
#define NVBX_MERGE_EMPTY_SOURCE 1   /* src has no TSDF block: nothing is allocated */
#define NVBX_MERGE_NO_OVERLAP   2   /* no voxel fused (the candidates stay allocated) */
typedef struct {
  float   min_weight;           /* a source corner counts with weight >= this */
  float   weight_scale;         /* the sampled TSDF weight is multiplied by this; finite, > 0 */
  int32_t merge_color;          /* != 0: colour is merged too */
  int32_t pad;
} nvbx_merge_options;           /* 16 bytes; offsets 0 4 8 12 */
typedef struct {
  int64_t source_blocks;        /* TSDF blocks of src */
  int64_t candidate_blocks;     /* blocks of dst the merge went over */
  int64_t blocks_allocated;     /* ... of which dst did not have before */
  int64_t voxels_fused;
  int64_t color_voxels_fused;
  int32_t status;               /* NVBX_MERGE_* */
  int32_t pad[5];
} nvbx_merge_result;            /* 64 bytes, 8-byte aligned DEVICE memory; offsets 0 8 16 24 32 40 44 */
/* defaults: min_weight 1e-4, weight_scale 1, merge_color 1 */
void nvbx_default_merge_options(nvbx_merge_options* options);
/* T_D_S: row-major 4 x 4, host memory.  options NULL: the defaults.  result_dev: written by the last launch, not waited for. */
int nvbx_merge_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_merge_options* options, nvbx_merge_result* result_dev);

/* ---- feature merging (the feature layer of one map brought into another; SEMANTICS.md "Feature merging") --------------------------------
 * A call of its own, meant to follow nvbx_merge_map with the same pose p_D = T_D_S p_S.  For every block of src that carries features, the
 * blocks of dst whose voxel centres can fall into it are candidates -- those dst HAS with its TSDF layer: this call allocates nothing and
 * never grows a pool.  Every voxel of a candidate takes the source voxel that CONTAINS R_SD p_D + t_SD (floor(p / voxel_size) per axis,
 * nvbx_query_features' rule: features are never interpolated); it contributes iff its block carries features in src and its stored weight
 * w_s satisfies w_s > 0 and w_s >= min_weight, with w_1 = w_s weight_scale.  Blend, per channel: w_0 = dst's stored weight (0 in a block
 * that carried no features when the call began), tw = w_0 + w_1, v = old (w_0 / tw) + f (w_1 / tw) rounded to fp16 to nearest even; weight
 * = min(tw, dst's max_weight) -- the feature integrator's blend with w_1 in place of 1.  A candidate without features in which a voxel
 * contributes is flagged and written whole (weight 0 and zero values where nothing contributed); one in which none does is neither.
 * Only dst's feature pools and NVBX_LAYER_FEATURE flags change: TSDF, colour, ESDF, every other flag, the dirty lists, the view list,
 * nvbx_last_depth_view, counters and mesh stay bit for bit; src is not modified.
 * Launches run on dst's stream, ordered behind everything enqueued on src's so far; work enqueued on src afterwards is ordered behind the
 * call's reads; both mappers' held-back work is carried out first.  The only host wait is the one for src's block count, which sizes the
 * scratch: nothing waits between enumerating and fusing.
 * NVBX_E_INVALID (nvbx_last_error names the call, dst unchanged): what nvbx_merge_map refuses of its mappers, pose, weight_scale and
 * result_dev; different voxel sizes; the feature layer off on either side; different channel counts; min_weight negative or not a number. */
typedef struct {
  float   min_weight;           /* a source voxel counts with weight > 0 and >= this */
  float   weight_scale;         /* its weight is multiplied by this; finite, > 0 */
  int32_t reserved[6];          /* 0 */
} nvbx_feature_merge_options;   /* 32 bytes; offsets 0 4 8 */
typedef struct {
  int64_t source_blocks;        /* feature blocks of src */
  int64_t candidate_blocks;     /* distinct blocks of dst the call went over */
  int64_t blocks_flagged;       /* ... of which it gave the feature layer */
  int64_t voxels_fused;
  int32_t status;               /* NVBX_MERGE_*: OK, EMPTY_SOURCE (src has no feature block), NO_OVERLAP (no voxel fused) */
  int32_t pad[7];
} nvbx_feature_merge_result;    /* 64 bytes, 8-byte aligned DEVICE memory; offsets 0 8 16 24 32 36 */
/* defaults: min_weight 0, weight_scale 1 */
void nvbx_default_feature_merge_options(nvbx_feature_merge_options* options);
/* T_D_S: row-major 4 x 4, host memory.  options NULL: the defaults.  result_dev: written by the last launch, not waited for. */
int nvbx_merge_features(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_feature_merge_options* options,
                        nvbx_feature_merge_result* result_dev);

/* ---- resampling ([U] a map brought into a mapper of a coarser voxel size; SEMANTICS.md "Resampling") ----------------------------------
 * nvbx_merge_map with two voxel sizes: reads `src` at its voxel size vs_s and writes `dst` at vs_d, r = (double)vs_d / (double)vs_s in
 * [1, 4], under p_D = T_D_S p_S.  Every voxel of every candidate block of dst takes n x n x n sub-samples (taps) on a lattice symmetric
 * about its centre, offsets ((float)i + 0.5f) / n - 0.5f voxels of dst per axis, each sampled from src by the merge's rule (eight corners
 * with weight >= min_weight).  With c valid taps the voxel fuses iff 2 c >= n^3: the sample distance is the mean over the valid taps, the
 * sample weight the sum of their weights over n^3 (a half-seen voxel gets half the weight) times weight_scale, fused, clamped and flagged as
 * by the merge.  With merge_color the source colour voxel nearest to the voxel's CENTRE is blended in; colour bytes are never averaged.
 * taps: n, 1 .. 4; 0 = min(4, ceil(r)).  With vs_d == vs_s and taps 1 the map and the result record are the merge's, bit for bit.
 * The result record is nvbx_merge_result with the merge's status values.  Ordering, the two host waits, growth and NVBX_E_CAPACITY (dst
 * unchanged) are the merge's, and so are its refusals (NVBX_E_INVALID, dst unchanged) but the one on voxel sizes: refused are r < 1
 * (upsampling), r > 4 and taps outside 0 .. 4.  T_D_S NULL: the identity.  Feature voxels, ESDF, occupancy and freespace are not resampled. */
typedef struct {
  float   min_weight;           /* a source corner counts with weight >= this */
  float   weight_scale;         /* the sample weight is multiplied by this; finite, > 0 */
  int32_t merge_color;          /* != 0: colour is brought over too */
  int32_t taps;                 /* sub-samples per axis, 1 .. 4; 0 = min(4, ceil(r)) */
} nvbx_resample_options;        /* 16 bytes; offsets 0 4 8 12 */
/* defaults: min_weight 1e-4, weight_scale 1, merge_color 1, taps 0 */
void nvbx_default_resample_options(nvbx_resample_options* options);
/* T_D_S: row-major 4 x 4, host memory, or NULL.  options NULL: the defaults.  result_dev: written by the last launch, not waited for. */
int nvbx_resample_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S[16], const nvbx_resample_options* options, nvbx_merge_result* result_dev);

/* ---- change detection ([U] what differs between two maps; SEMANTICS.md "Change detection") --------------------------------------------
 * Compares mapper `m` ("now") with a reference mapper `ref` ("before") under p_M = T_M_R p_R.  A voxel of a TSDF block of m with stored
 * {d, w}, inside box_min_max_vox (inclusive, global voxel coordinates of m as in nvbx_find_frontiers; NULL: unbounded), is OBSERVED iff
 * w >= min_weight, FREE iff observed and d > free_distance_m, OCCUPIED iff observed and d <= occupied_distance_m, NEAR otherwise (a NaN d
 * is neither free nor occupied).  Its sample of ref lies at p_R = R_RM p_M + t_RM, p_M = ((float)(8 b + v) + 0.5f) voxel_size per axis and
 * {R_RM, t_RM} the inverse pair of nvbx_merge_map.  sampling 0 (trilinear): the rule of the merge and of the TSDF point query -- all eight
 * corners in TSDF blocks of ref with weight >= ref_min_weight, d_ref = the trilinear interpolant.  sampling 1 (nearest): the voxel
 * floor(p_R / voxel_size) per axis in f32, valid iff its block carries the TSDF layer and its weight >= ref_min_weight, d_ref = its
 * distance.  A valid sample is FREE / OCCUPIED / NEAR by the same two thresholds; an invalid one, or one outside the addressable block
 * range, is UNKNOWN.  label 0 (APPEARED): m OCCUPIED and ref FREE; label 1 (REMOVED): m FREE and ref OCCUPIED; -1 otherwise;
 * score = fabsf(d - d_ref) on a labelled voxel, 0 elsewhere.
 * nvbx_find_changes writes the sparse volume of nvbx_find_frontiers: one entry per TSDF block of m with at least one labelled voxel, entry
 *   order unspecified; label_dev[e][512], score_dev[e][512] (NULL: not written), t = vx 64 + vy 8 + vz; *count_dev = the number of such
 *   blocks, also beyond capacity_blocks; entries from the capacity on are written nowhere; capacity_blocks 0 with NULL arrays only counts.
 *   Apart from the entry order the result is bit-specified.  result_dev (may be NULL): written by the last launch, not waited for.
 * nvbx_change_clusters: the same, then nvbx_label_components over min(*block_count_dev, capacity_blocks) entries (read on the device), with
 *   the argument tail of nvbx_frontier_clusters; its refusals are checked before anything is launched.  A component of label 0 is an
 *   object that appeared, one of label 1 an object that is gone, peak_score the largest distance change.
 * Launches run on m's stream, behind everything enqueued on ref's stream so far; work enqueued on ref afterwards is ordered behind the
 * reads (as nvbx_merge_map).  No host wait, no allocation; held-back colour / ESDF work of both mappers stays held back; neither map is
 * written.  NVBX_E_INVALID (nvbx_last_error set, nothing launched): ref == m; different devices or voxel sizes; an occupancy mapper on
 * either side; a pose that is not finite, out of range or no rotation; a NaN weight or distance option; occupied_distance_m >
 * free_distance_m; sampling outside 0 / 1; the capacity, pointer and box refusals of nvbx_find_frontiers; a misaligned result_dev. */
#define NVBX_CHANGE_OK              0
#define NVBX_CHANGE_EMPTY_MAP       1   /* m has no TSDF block */
#define NVBX_CHANGE_EMPTY_REFERENCE 2   /* ref has no TSDF block */
#define NVBX_CHANGE_NO_OVERLAP      3   /* voxels_compared == 0 */
#define NVBX_CHANGE_TRILINEAR 0
#define NVBX_CHANGE_NEAREST   1
typedef struct {
  float   min_weight;           /* a voxel of m is observed with weight >= this */
  float   ref_min_weight;       /* a voxel of ref counts with weight >= this */
  float   free_distance_m;      /* FREE: distance > this; 0 = one voxel size */
  float   occupied_distance_m;  /* OCCUPIED: distance <= this */
  int32_t sampling;             /* NVBX_CHANGE_TRILINEAR / NVBX_CHANGE_NEAREST */
  int32_t pad;
} nvbx_change_options;          /* 24 bytes; offsets 0 4 8 12 16 20 */
typedef struct {
  int64_t blocks_scanned;       /* TSDF blocks of m */
  int64_t voxels_compared;      /* in the box, observed in m, with a valid sample of ref */
  int64_t voxels_appeared;      /* label 0 */
  int64_t voxels_removed;       /* label 1 */
  int64_t blocks_changed;       /* blocks with a labelled voxel (*count_dev) */
  int32_t status;               /* NVBX_CHANGE_*, checked in the order EMPTY_MAP, EMPTY_REFERENCE, NO_OVERLAP */
  int32_t pad[5];
} nvbx_change_result;           /* 64 bytes, 8-byte aligned DEVICE memory; offsets 0 8 16 24 32 40 44 */
/* defaults: min_weight 1e-4, ref_min_weight 1e-4, free_distance_m 0 (one voxel size), occupied_distance_m 0, sampling 0 */
void nvbx_default_change_options(nvbx_change_options* options);
/* T_M_R: row-major 4 x 4, host memory.  options NULL: the defaults. */
int nvbx_find_changes(nvbx_mapper* m, nvbx_mapper* ref, const float T_M_R[16], const nvbx_change_options* options,
                      const int32_t box_min_max_vox[6], nvbx_index3d* block_idx_dev, int32_t* label_dev, float* score_dev,
                      int64_t capacity_blocks, int64_t* count_dev, nvbx_change_result* result_dev);
int nvbx_change_clusters(nvbx_mapper* m, nvbx_mapper* ref, const float T_M_R[16], const nvbx_change_options* options,
                         const int32_t box_min_max_vox[6], int32_t connectivity, int32_t min_voxels, nvbx_index3d* block_idx_dev,
                         int32_t* label_dev, float* score_dev, int32_t* component_id_dev, int64_t capacity_blocks,
                         int64_t* block_count_dev, nvbx_component* components_dev, int64_t capacity_components,
                         int64_t* component_count_dev, nvbx_change_result* result_dev);

/* ---- surface points and map-to-map registration (SEMANTICS.md "Surface points", "Registering two maps") ----------------
 * [U] nvbx_surface_points: the TSDF's zero crossings as a point cloud in DEVICE memory, with colour and normals, asynchronous on the mapper's
 * stream.  A voxel {d, w} is OBSERVED iff its block is allocated with a TSDF layer, w >= min_weight and d == d.  The edge from an ORIGIN voxel
 * g to g + e_a (a = 0, 1, 2; across block borders) holds a crossing iff both voxels are observed and (d0 <= 0) != (d1 <= 0); a neighbour in a
 * block that is missing, has no TSDF layer or is not addressable gives none.  The point: along axis a
 *   (((float)b_a * (8 vs) + (float)v_a * vs) + vs * 0.5f) + vs * (-d0 / (d1 - d0)),   on the other two axes the voxel centre (the first term).
 * Filters: the origin voxel inside box_min_max_vox (inclusive, global voxel coordinates, only with use_box != 0) and g_x, g_y, g_z all
 * multiples of stride (mathematical modulo); require_color != 0: only crossings with a colour (below).
 * Outputs, each may be NULL: points_dev[capacity][3] f32; colors_dev[capacity][3] u8 = the stored r, g, b of the colour voxel of the edge's
 * endpoint nearer the surface (|d0| <= |d1|: the origin) where its block carries colour and its colour weight is > 0, else 0, 0, 0;
 * normals_dev[capacity][3] f32 = nvbx_query_points' TSDF gradient at the point (same min_weight) divided by its length, 0 where the query is
 * invalid or the gradient zero.  *count_dev (required) = the number of crossings, also beyond capacity; rows from capacity on are not written.
 * ORDER: ascending pool slot of the origin block, then t = vx 64 + vy 8 + vz, then axis -- a function of the mapper's state alone: two calls
 * write identical bytes.  TSDF mappers only; reads the map only; a call without colour output leaves held-back colour / ESDF work held back,
 * one with colors_dev or require_color carries it out first (as nvbx_query_colors).
 * Refused: NULL mapper or count_dev, capacity < 0 or > 2^30, capacity > 0 without points_dev, stride < 1, a NaN min_weight, a used box with
 * min > max on an axis, an occupancy mapper. */
typedef struct {
  float min_weight;             /* 1e-4 */
  int32_t stride;               /* 1 */
  int32_t use_box;              /* 0 */
  int32_t require_color;        /* 0 */
  int32_t box_min_max_vox[6];   /* min x y z, max x y z */
} nvbx_surface_options;         /* 40 bytes; offsets 0 4 8 12 16 */
void nvbx_default_surface_options(nvbx_surface_options* options);
int nvbx_surface_points(nvbx_mapper* m, const nvbx_surface_options* options, float* points_dev, uint8_t* colors_dev, float* normals_dev,
                        int64_t capacity, int64_t* count_dev);
/* nvbx_align_map: the pose T_D_S (p_D = T_D_S p_S, nvbx_merge_map's argument) of map src in map dst, refined from a guess: src's surface
 * points (surface_options; NULL: defaults) go into scratch of dst, then exactly the launches of nvbx_align_points over them against dst's TSDF
 * -- or, with color_options != NULL, of nvbx_align_points_color with the points' colours (require_color is then forced on and
 * color_result_dev is required).  Runs on dst's stream behind what src's stream holds; later work on src is ordered behind the reads.
 * ONE host wait: for the 8-byte point count, which sizes the scratch and the alignment's grid; everything after it is enqueued without
 * waiting.  No crossing: as nvbx_align_points with n = 0.  The voxel sizes may differ.  Every refusal of either half comes before the first
 * launch; refused as well: dst == src, different devices, an occupancy mapper on either side.
 * nvbx_relocalize_map: the same in front of nvbx_relocalize_points' launches (its lattice, options, scores_dev and result record). */
int nvbx_align_map(nvbx_mapper* dst, nvbx_mapper* src, const float T_D_S_guess[16], const nvbx_surface_options* surface_options,
                   const nvbx_align_options* align_options, const nvbx_align_color_options* color_options, nvbx_align_result* result_dev,
                   nvbx_align_color_result* color_result_dev);
int nvbx_relocalize_map(nvbx_mapper* dst, nvbx_mapper* src, const float T0[16], const nvbx_search_lattice* lattice,
                        const nvbx_surface_options* surface_options, const nvbx_score_options* score_options, int32_t min_inliers,
                        const nvbx_align_options* align_options, nvbx_pose_score* scores_dev, nvbx_relocalize_result* result_dev);

/* ---- mask splitting (human / people-segmentation mapping) ------------------------------------------------------------
 * [U] ImageMasker::splitImageOnGPU as used by MultiMapper::integrateDepth(depth, mask, T_L_CD, T_CM_CD, depth_cam, mask_cam) --
 * nvblox_node.cpp:1018-1060: every valid depth pixel is lifted to 3-D, moved into the mask camera (T_CM_CD = T_L_CM^-1 T_L_CD)
 * and projected; it is MASKED if it lands on a non-zero mask pixel and is not occluded there (its depth in the mask camera is
 * within occlusion_threshold_m of the nearest depth pixel that landed on the same mask pixel).  depth_unmasked gets the pixel
 * if it is not masked, depth_masked if it is; the other image gets NVBX_MASKED_DEPTH_INVALID (-1, an invalid depth for the
 * integrators).  overlay_rgb (may be NULL): grey depth with masked pixels tinted red (debug image).  Asynchronous. */
#define NVBX_MASKED_DEPTH_INVALID (-1.0f)
int nvbx_split_depth_by_mask(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const uint8_t* mask_dev,
                             int32_t mask_rows, int32_t mask_cols, const float T_CM_CD[16], const nvbx_camera* depth_camera,
                             const nvbx_camera* mask_camera, float occlusion_threshold_m, float* depth_unmasked_dev,
                             float* depth_masked_dev, uint8_t* overlay_rgb_dev);
/* MultiMapper::integrateColor(color, mask, T_L_C, camera) -- nvblox_node.cpp:1261-1262 (mask and colour share the camera):
 * [U] masked pixels are black in rgb_unmasked and the only non-black ones in rgb_masked (either output may be NULL). */
int nvbx_split_color_by_mask(nvbx_mapper* m, const uint8_t* rgb_dev, int32_t rows, int32_t cols, const uint8_t* mask_dev,
                             uint8_t* rgb_unmasked_dev, uint8_t* rgb_masked_dev);

/* ---- dynamic mapping (MappingType::kDynamic, nvblox_dynamics.yaml) -----------------------------------------------------------
 * update_time_ms of MultiMapper::integrateDepth(depth, T_L_C, camera, update_time_ms) (nvblox_node.cpp:1062): host state, read by the
 * next nvbx_integrate_depth of a projective_layer_type 2 mapper, which then also updates the freespace layer of the blocks in view
 * ([U] FreespaceIntegrator, semantics in DESIGN.md 3). */
int nvbx_set_time_ms(nvbx_mapper* m, int64_t update_time_ms);
/* [U] DynamicsDetection::computeDynamics: mask_dev[rows][cols] (u8) = 1 where a valid depth pixel (<= max_distance_m if > 0) lies in a
 * high-confidence-freespace voxel, else 0.  Asynchronous. */
int nvbx_detect_dynamics(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C[16], const nvbx_camera* camera,
                         float max_distance_m, uint8_t* mask_dev);
/* [U] removeSmallConnectedComponents (multi_mapper connected_mask_component_size_threshold, mapper_initialization.cpp:130): erases the
 * 8-connected components of non-zero pixels smaller than min_size.  In place; asynchronous on the mapper's stream (lock-free union-find). */
int nvbx_remove_small_components(nvbx_mapper* m, uint8_t* mask_dev, int32_t rows, int32_t cols, int32_t min_size);
/* The front end of MultiMapper::integrateDepth(depth, T_L_C, camera) in MappingType::kDynamic (nvblox_node.cpp:1062; its outputs are read at
 * :1098,1108) as ONE call: nvbx_detect_dynamics -> nvbx_remove_small_components(min_component_size; <= 0: not removed) ->
 * nvbx_split_depth_by_mask with the depth camera as the mask camera (T_CM_CD = identity).  Same results as the three calls, bit for bit
 * (mask_dev = the cleaned mask; overlay_rgb_dev may be NULL), in three launches and no memset instead of six and one.  Like
 * nvbx_detect_dynamics it leaves held-back work (colour deferral) alone.  Asynchronous. */
int nvbx_dynamic_depth_split(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C[16], const nvbx_camera* camera,
                             float max_distance_m, int32_t min_component_size, float occlusion_threshold_m,
                             uint8_t* mask_dev, float* depth_unmasked_dev, float* depth_masked_dev, uint8_t* overlay_rgb_dev);

/* ---- device-side view for the caller's own kernels (GPULayerView / gpu_indexing.cuh: esdf_slice_conversions.cu:18,
 * esdf_and_gradients_conversions.cu:19-23).  Accessors: include/nvblox_hip_device.h. */
typedef struct {
  const void* table; uint32_t table_mask, table_shift;    /* open-addressing hash: 16-byte entries {key64, slot32, stamp32} */
  const uint32_t* slot_flags;                              /* per slot: NVBX_LAYER_* bits in the low byte */
  const int32_t* slot_index;                               /* per slot: block index x, y, z */
  const void* tsdf; const void* color; const void* esdf;   /* voxel pools, 512 x 8 bytes per slot */
  float voxel_size; uint32_t block_capacity;
} nvbx_device_view;
int nvbx_get_device_view(nvbx_mapper* m, nvbx_device_view* out);

/* ---- layer access (Layer<VoxelBlock> accessors; synchronise) ----------------------------------------------------
 * layer.numAllocatedBlocks(), getAllBlockIndices(), getBlockAtIndex(), allocateBlockAtIndex(),
 * callFunctionOnAllVoxels -- test_esdf_and_gradient_conversions.cpp:85-92,114,118 */
int64_t nvbx_num_blocks(nvbx_mapper* m, uint32_t layer);
int64_t nvbx_block_indices(nvbx_mapper* m, uint32_t layer, nvbx_index3d* out, int64_t capacity);
int nvbx_get_block(nvbx_mapper* m, uint32_t layer, nvbx_index3d idx, void* voxels_out /* 512 reference structs */);
int nvbx_set_block(nvbx_mapper* m, uint32_t layer, nvbx_index3d idx, const void* voxels_in);
/* batched allocateBlockAtIndex + whole-block write: voxels_in[n][512] reference structs (TSDF blocks become ESDF- and mesh-dirty) */
int nvbx_set_blocks(nvbx_mapper* m, uint32_t layer, const nvbx_index3d* idx, int64_t n, const void* voxels_in);
/* batched getBlockAtIndex: n blocks into voxels_out[n][512]; found_out[i] = 1 if block i exists (may be NULL) */
int nvbx_get_blocks(nvbx_mapper* m, uint32_t layer, const nvbx_index3d* idx, int64_t n, void* voxels_out, int32_t* found_out);
/* blocks touched by the last integrateDepth / integrateColor (what Mapper records as "blocks to update") */
int64_t nvbx_last_depth_view(nvbx_mapper* m, nvbx_index3d* out, int64_t capacity);
int64_t nvbx_last_color_view(nvbx_mapper* m, nvbx_index3d* out, int64_t capacity);
int nvbx_get_synthetic_depth(nvbx_mapper* m, float* out_host, int64_t capacity, int32_t* rows, int32_t* cols);
int nvbx_get_counters(nvbx_mapper* m, nvbx_counters* out);

/* ---- mesh output (SerializedColorMeshLayer accessors, conversions/mesh_conversions.cpp:62-104) -------------------
 * Flat arrays + per-block offsets for the blocks meshed by the last nvbx_update_color_mesh: vertices (x,y,z f32),
 * normals (f32 x3), colours (rgba u8), triangle indices (int32, local to the block). */
int nvbx_mesh_sizes(nvbx_mapper* m, int64_t* n_blocks, int64_t* n_vertices, int64_t* n_triangles);
int nvbx_mesh_copy(nvbx_mapper* m, nvbx_index3d* block_indices, int32_t* vertex_offsets /* n_blocks+1 */,
                   int32_t* triangle_offsets /* n_blocks+1 */, float* vertices, float* normals, uint8_t* colors,
                   int32_t* triangles);

/* The exchange message without an export launch: once a buffer is registered (host state only), every nvbx_integrate_depth /
 * _lidar_depth also writes the Index3D of the blocks it updates into it -- int32 [1 + capacity][3], row 0 = {count, 0, 0} -- from
 * inside its TSDF-update launch.  (The blocks of THIS depth frame; nvbx_esdf_dirty_list also covers decay / clearing / set_block.)
 * NULL unregisters.  The buffer must stay valid while registered. */
int nvbx_set_view_export(nvbx_mapper* m, int32_t* packed_dev, int64_t capacity);
/* ---- multi-GPU (one camera per GPU, all-gather of updated block indices before the ESDF sweep) -----
 * nvbx_esdf_dirty_list writes the Index3D of the TSDF blocks dirtied since the last updateEsdf into caller-owned
 * device buffers (indices int32[capacity][3], count int32[1], clamped to capacity) -- asynchronous, no host copy.
 * The caller all-gathers both over RCCL and feeds every peer's list back with nvbx_mark_esdf_dirty (count is read
 * on the device; max_count bounds it). */
int nvbx_esdf_dirty_list(nvbx_mapper* m, int32_t* indices_dev_out, int32_t* count_dev_out, int64_t capacity);
int nvbx_mark_esdf_dirty(nvbx_mapper* m, const int32_t* indices_dev, const int32_t* count_dev, int64_t max_count);
/* The same for the whole all-gathered buffer in ONE launch: gathered_dev is int32 [world][1 + max_count][3], row 0 of
 * each rank = (count, -, -), rows 1.. = block indices (the packed layout isaac_ros_nvblox_amd/dist.py all-gathers);
 * rank `self_rank`'s own list is skipped. */
int nvbx_mark_esdf_dirty_gathered(nvbx_mapper* m, const int32_t* gathered_dev, int32_t world, int32_t self_rank, int64_t max_count);
/* The same union step, held back -- no launch of its own.  WHEN it runs, and how long `gathered_dev` must stay valid and unchanged:
 *   classic launch order: extra workgroups of the next nvbx_integrate_color launch perform it beside the marking of the mapper's own
 *     dirty blocks; the peers' blocks reach the ESDF with the NEXT nvbx_update_esdf (one update after the frame that produced them).
 *   pipelined order (colour deferral, the default): it rides in the fused TSDF-update launch of the next nvbx_integrate_depth, where it only
 *     sets the blocks ESDF-dirty for the marking pass AFTER that -- the peers' blocks reach the ESDF TWO updates after the frame that produced
 *     them, and the buffer is read one nvbx_integrate_depth later than in classic order.
 *   any other entry point that comes first performs it at once (its own launch).
 * A caller that refills gathered buffers in rotation therefore needs THREE sets (filling / in flight in the collective / being read here):
 * nvblox::BlockIndexExchange (include/nvblox/mapper/block_index_exchange.h) and dist.PipelinedDirtyBlockExchange do exactly that; two sets race
 * with the rider.  Under option (A) of SURVEY.md 8e (replicas + index union) the extra update of delay changes no voxel: a peer's block only
 * re-marks a column from the local, unchanged TSDF. */
int nvbx_mark_esdf_dirty_gathered_deferred(nvbx_mapper* m, const int32_t* gathered_dev, int32_t world, int32_t self_rank, int64_t max_count);

/* ---- multi-GPU, one fused map (SURVEY.md 8e option B, made exact): measurement exchange ---------------------------------------------
 * One camera per GPU.  nvbx_measure_depth runs the view calculation and the per-voxel projection / depth sampling of THIS rank's camera
 * -- the expensive, sharded part of integrateDepth -- and writes, per block in view, a record {Index3D, 512 x {measured depth, voxel
 * depth}} (voxel depth < 0: voxel not touched; measured depth < 0: it projects onto invalid depth) plus the record count, into
 * caller-owned device buffers (asynchronous, no host copy).  The caller all-gathers the buffers (RCCL over xGMI; isaac_ros_nvblox_amd/
 * dist.py MeasurementFusion) and hands the gathered array [world][stride_blocks] + counts [world] to nvbx_apply_measurements on every
 * rank, which applies every camera's measurements to the local map in RANK ORDER with the integrator's own per-voxel update: every rank
 * then holds the SAME map, bit-identical to ONE mapper integrating the cameras in rank order (nvbx_integrate_depth_batch) -- which
 * exchanging already-fused {distance, weight} blocks cannot give (the clamps do not commute with a weighted mean).  owner_mod > 1: only
 * blocks with Index3DHash(block) mod owner_mod == owner_rank are applied (the rank's shard of that map; the other blocks stay empty).
 * world <= NVBX_MAX_BATCH.  Two launches per apply, whatever the world size. */
typedef struct { int32_t x, y, z, rank; float ds_vd[512][2]; } nvbx_measurement_block;     /* 4112 bytes */
int nvbx_measure_depth(nvbx_mapper* m, const float* depth_dev, int32_t rows, int32_t cols, const float T_L_C[16], const nvbx_camera* camera,
                       nvbx_measurement_block* out_dev, int32_t* count_dev, int64_t capacity_blocks);
int nvbx_apply_measurements(nvbx_mapper* m, const nvbx_measurement_block* gathered_dev, const int32_t* counts_dev, int32_t world, int64_t stride_blocks,
                            int32_t owner_mod, int32_t owner_rank);

/* ---- ground plane (MultiMapper::ground_plane_estimator(), nvblox_node.cpp:1456,1474; parameters mapper_initialization.cpp:133-153) ------
 * [U] GroundPlaneEstimator restated.  nvbx_tsdf_zero_crossings: the upward zero crossings of the TSDF -- vertically adjacent observed voxels
 * with d(z) <= 0 < d(z + 1), interpolated linearly along z -- whose height lies in [min_z_m, max_z_m] (ground_points_candidates_min/max_z_m),
 * as xyz triples in HOST memory sorted by (x, y, z); returns the count (> capacity: nothing written, come back with room); synchronises.
 * nvbx_fit_plane_ransac (host only, no mapper): `iterations` (num_ransac_iterations) sampled triples, inliers within distance_threshold_m
 * (ransac_distance_threshold_m), normal turned upwards; plane_out = {nx, ny, nz, d} with n . p + d = 0; returns the inlier count of the winner
 * (0 = no plane).  The sampling sequence is fixed by `seed`, so the estimate is a pure function of its inputs. */
int64_t nvbx_tsdf_zero_crossings(nvbx_mapper* m, float min_z_m, float max_z_m, float* points_xyz_host, int64_t capacity);
int64_t nvbx_fit_plane_ransac(const float* points_xyz_host, int64_t n, float distance_threshold_m, int32_t iterations, uint32_t seed, float plane_out[4]);

/* ---- instrumentation (timing::Timer analogue for the per-kernel roofline line of bench.py) -----------------------
 * While enabled every kernel launch is bracketed by a hipEvent pair on the mapper stream. nvbx_get_profile returns a
 * JSON object {"kernel": {"count": n, "total_ms": t}}; the entry "_empty_event_pair" is the span of event pairs with nothing between
 * them = what the instrumentation itself adds to the span of one launch (subtract it once per launch). */
int nvbx_set_profiling(nvbx_mapper* m, int32_t enable);
int nvbx_get_profile(nvbx_mapper* m, char* json_out, int64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* NVBLOX_HIP_H_ */
