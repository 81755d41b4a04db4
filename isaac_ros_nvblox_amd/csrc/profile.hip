// profile.hip -- optional per-kernel timing: a hipEvent pair around every launch (NVBX_LAUNCH*) while nvbx_set_profiling is on.
#include <cstdio>
#include <cstring>
#include "nvbx_mapper.h"
using namespace nvbx;

hipEvent_t nvbx_mapper::get_event() {
  if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
  hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
void nvbx_mapper::span_begin(const char* name, hipStream_t st) {
  Span s{name, get_event(), get_event()};
  (void)hipEventRecord(s.a, st);
  spans.push_back(s);
}
void nvbx_mapper::span_end(hipStream_t st) { (void)hipEventRecord(spans.back().b, st); }
extern "C" int nvbx_set_profiling(nvbx_mapper* m, int32_t enable) {
  if (!m) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;
  NVBX_HIP(hipStreamSynchronize(m->stream));
  for (auto& s : m->spans) { m->event_pool.push_back(s.a); m->event_pool.push_back(s.b); }
  m->spans.clear();
  m->profiling = enable != 0;
  return NVBX_OK;
}

// JSON object {"kernel": {"count": n, "total_ms": t}, ...} of every launch since nvbx_set_profiling(m, 1).
extern "C" int nvbx_get_profile(nvbx_mapper* m, char* json_out, int64_t capacity) {
  if (!m || !json_out || capacity < 4) return NVBX_E_INVALID;
  if (m->begin_call()) return NVBX_E_DEVICE;
  NVBX_HIP(hipStreamSynchronize(m->stream));
  struct Acc { const char* name; int64_t n; double ms; double max_ms; };
  std::vector<Acc> acc;
  for (auto& s : m->spans) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) continue;
    bool hit = false;
    for (auto& a : acc) if (!strcmp(a.name, s.name)) { a.n++; a.ms += ms; if (ms > a.max_ms) a.max_ms = ms; hit = true; break; }
    if (!hit) acc.push_back({s.name, 1, ms, ms});
  }
  // what a hipEvent pair adds to the span of ONE launch: pairs with nothing between them, on the same (now idle) stream
  {
    const int kPairs = 32; double ms_sum = 0.0; int n_ok = 0;
    std::vector<hipEvent_t> ev;
    for (int i = 0; i < 2 * kPairs; i++) { ev.push_back(m->get_event()); (void)hipEventRecord(ev.back(), m->stream); }
    NVBX_HIP(hipStreamSynchronize(m->stream));
    for (int i = 0; i < kPairs; i++) { float ms = 0.0f; if (hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]) == hipSuccess) { ms_sum += ms; n_ok++; } }
    for (hipEvent_t e : ev) m->event_pool.push_back(e);
    if (n_ok) acc.push_back({"_empty_event_pair", n_ok, ms_sum, 0.0});
  }
  // a mapper with a feature layer (features.hip) reports its pools: count = bytes allocated.  No entry: nothing was ever allocated for features
  if (m->feat_val) acc.push_back({"_feature_pool_bytes", (int64_t)m->capacity * (1024 * (int64_t)m->feat_channels + 2048), 0.0, 0.0});
  std::string out = "{";
  for (size_t i = 0; i < acc.size(); i++) {
    char buf[256];
    std::string nm = acc[i].name;
    for (char& c : nm) if (c == '(' || c == ')' ) c = ' ';
    snprintf(buf, sizeof(buf), "%s\"%s\": {\"count\": %lld, \"total_ms\": %.6f, \"max_ms\": %.6f}", i ? ", " : "", nm.c_str(), (long long)acc[i].n, acc[i].ms, acc[i].max_ms);
    out += buf;
  }
  out += "}";
  if ((int64_t)out.size() + 1 > capacity) return NVBX_E_CAPACITY;
  memcpy(json_out, out.c_str(), out.size() + 1);
  return NVBX_OK;
}
