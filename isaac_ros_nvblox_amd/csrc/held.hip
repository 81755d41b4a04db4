// held.hip -- work the mapper has accepted but not launched yet (nvbx_mapper::held), and the one place that decides when it is carried out.
// WHAT can be held back:
//   * the distance transform (EDT) of an updateEsdf (held.edt_pending + edt_args; NVBX_DEFER_EDT=0 disables): it rides in the view-marking launch of the
//     next depth frame, or in the fused TSDF-update launch, instead of being a launch of its own;
//   * the union step of the multi-GPU exchange (held.import_pending + its arguments, nvbx_mark_esdf_dirty_gathered_deferred): it rides in the next
//     integrateColor launch beside the marking of the mapper's own dirty blocks, or in the fused TSDF-update launch;
//   * with colour deferral (nvbx_mapper_set_color_deferral) an integrateColor (held.color_pending: arguments remembered, nothing launched)
//     and an updateEsdf that follows it, or that comes with no colour at all (held.esdf_update_pending).  Contract: the colour image stays valid and
//     unchanged until the next call into the mapper has returned -- or, staged (the default), is copied when it is held back.
// WHO carries it out: the next camera integrateDepth, in PIPELINED order (tsdf.hip depth_step_*) -- view marking of the new depth frame || sphere tracing
//   of the held-back colour frame, colour integration + ESDF marking, TSDF update of the new frame: three launches per frame instead of four, two in the
//   fused form (a depth batch carries a colour batch, one frame one frame; what a call cannot carry it replays first).
// EVERYONE ELSE passes begin_call() as the first thing it does, which carries everything out as the calls would have run at call time, IN THIS ORDER:
//   replay_deferred (integrateColor, then updateEsdf -- which may arm a new EDT), flush_edt, flush_import (esdf.hip) -- so the API observes call order.
//   begin_call_keeping_held() skips exactly that, for the entry point that touches nothing the held-back work does: nvbx_detect_dynamics (TSDF + freespace
//   reads only; the dynamic-mapping frame starts with it) and the camera integrateDepth that carries the work out itself (tsdf.hip cameras_prepare).
// Two modes switch parts of this off while they last (nvbx_mapper::ModeScope): `replaying` (the replayed calls must not be held back again, nor replay)
//   and `pipelined_order` (the carried-out calls run inside integrateDepth: no replay, and the marking pass empties its list itself -- EsdfArgs).
#include "nvbx_mapper.h"
#include "nvbx_color_worker.h"      // with_color_types
using namespace nvbx;

__global__ void k_reset_esdf_dirty_list(DMap m) { if (threadIdx.x < NSH) *shc_at(m, S_LIST_ESDF_DIRTY, threadIdx.x, 0) = 0; }
int nvbx_mapper::reset_consumed_list() {
  if (premark_consumed) { NVBX_LAUNCH(this, k_reset_esdf_dirty_list, dim3(1), dim3(64), d); premark_consumed = false; }
  return NVBX_OK;
}
int nvbx_mapper::begin_call(bool carry_out_held) {
  enqueue_seq++;                     // (an entry point runs: host copies of device counters are stale from here on, esdf.hip nvbx_esdf_slice_to_image)
  zc_valid = false;                  // (whatever follows may change the TSDF: the kept zero-crossing list is dropped)
  // every entry point passes here before its first HIP call: make this mapper's device current (hosts with one mapper per GPU in
  // one process); a thread-local read when it already is
  { int cur = -1; if (hipGetDevice(&cur) != hipSuccess || cur != device) NVBX_HIP(hipSetDevice(device)); }
  if (carry_out_held) {
    if (!replaying && !pipelined_order && replay_deferred()) return NVBX_E_DEVICE;      // held-back integrateColor / updateEsdf: carried out first, in call order
    if (flush_edt() || flush_import()) return NVBX_E_DEVICE;
  }
  return NVBX_OK;
}
// the held-back calls of colour deferral, carried out as they would have been at call time: the entry point of each kind of colour call (with_color_types)
static int replay_color(nvbx_mapper* m, const nvbx_mapper::ColorPending& c, PixRgb8, std::integral_constant<int, 1>) { return nvbx_integrate_color(m, (const uint8_t*)c.imgs[0], c.rows, c.cols, c.T, &c.cams[0]); }
static int replay_color(nvbx_mapper* m, const nvbx_mapper::ColorPending& c, PixBgra8, std::integral_constant<int, 1>) { return nvbx_integrate_color_bgra8(m, (const uint8_t*)c.imgs[0], c.rows, c.cols, c.T, &c.cams[0]); }
static int replay_color(nvbx_mapper* m, const nvbx_mapper::ColorPending& c, PixRgb8, std::integral_constant<int, MAX_BATCH>) { return nvbx_integrate_color_batch(m, c.n, reinterpret_cast<const uint8_t* const*>(c.imgs), c.rows, c.cols, c.T, c.cams); }
int nvbx_mapper::replay_deferred() {
  if (!held.color_pending.on && !held.esdf_update_pending) return NVBX_OK;
  ModeScope mode(replaying);
  int rc = NVBX_OK;
  if (replay_pair_applies()) { rc = replay_pair(); return rc == NVBX_OK ? NVBX_OK : NVBX_E_DEVICE; }
  if (held.color_pending.on) {
    const ColorPending c = take_pending();
    rc = with_color_types(c.enc, c.n, [&](auto pix, auto nb) { return replay_color(this, c, pix, nb); });
  }
  if (rc == NVBX_OK && held.esdf_update_pending) { held.esdf_update_pending = false; rc = nvbx_update_esdf(this); }
  held.esdf_update_pending = false;
  mode.leave();
  release_consumed_frames();
  return rc == NVBX_OK ? NVBX_OK : NVBX_E_DEVICE;
}
extern "C" int nvbx_mapper_set_color_deferral(nvbx_mapper* m, int32_t enable) {
  if (!m) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;          // (anything held back under the old setting is carried out)
  if (enable < 0 || enable > 2) { set_error("nvbx_mapper_set_color_deferral: 0 = off, 1 = on (the caller keeps the image valid), 2 = on with a staged copy"); return NVBX_E_INVALID; }
  m->color_deferral = enable != 0; m->color_staging = enable == 2;
  return NVBX_OK;
}
extern "C" int nvbx_flush(nvbx_mapper* m) {
  if (!m) return NVBX_E_INVALID;
  NVBX_HIP(hipSetDevice(m->device));
  return m->begin_call();
}
