// The tuning knobs of libgdsm: one row per gdsm_tune key (include/gdsm.h lists them). A knob is
// set by gdsm_tune at any time, or by its environment variable, read once when the library loads;
// the launchers read it through knob(). What each value selects is described where it is used.
#include "gdsm_launch.h"

#include <stdlib.h>
#include <string.h>

#include <atomic>

namespace gdsm {

namespace {

struct KnobRow {
  const char* key;
  const char* env;  // nullptr: no variable
  int lo;           // accepted: lo + i for every set bit i of `ok`
  uint64_t ok;
  int dflt;
  std::atomic<int> v{0};

  bool accepts(int64_t x) const {
    const uint64_t i = (uint64_t)x - (uint64_t)(int64_t)lo;  // (x < lo wraps to a large i)
    return i < 64 && ((ok >> i) & 1u);
  }
};
constexpr uint64_t first(unsigned n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

#ifdef GDSM_MEASURE  // 4-7: the fold's measurement arms (output invalid); 3 was the four-pass path
constexpr uint64_t kCohVariantsOk = 0xF7;
#else
constexpr uint64_t kCohVariantsOk = 0x07;
#endif

// In the order of enum Knob.
KnobRow g_knobs[] = {
    {"diff_variant", "GDSM_DIFF_VARIANT", 0, first(9), 0},
    {"apply_variant", "GDSM_APPLY_VARIANT", 0, first(9), 0},
    {"diff_solo_max", "GDSM_DIFF_SOLO_MAX", 0, first(kSoloUnits + 1), 0},
    {"diff_chain", "GDSM_DIFF_CHAIN", 0, first(5), 2},
    {"coh_variant", "GDSM_COH_VARIANT", 0, kCohVariantsOk, 0},
    {"coh_chain", "GDSM_COH_CHAIN", 0, first(2), 1},
    {"coh_span", "GDSM_COH_SPAN", 1, 0xB /* 1, 2, 4 */, 4},
    {"rounds_xcd", "GDSM_ROUNDS_XCD", -1, first(3), -1},
    {"rounds_lds", "GDSM_ROUNDS_LDS", -1, first(3), -1},
    {"rounds_lds_wg", "GDSM_ROUNDS_LDS_WG", 0, first(kRoundsLdsMaxWGs + 1), 0},
#ifdef GDSM_MEASURE
    {"diff_skip", nullptr, 0, first(64), 0},
#endif
};
static_assert(sizeof(g_knobs) / sizeof(g_knobs[0]) == kKnobs, "one row per Knob");

// At load: the default, or the variable's value when it is a number the knob accepts.
[[maybe_unused]] const bool g_knobs_loaded = [] {
  for (KnobRow& r : g_knobs) {
    int v = r.dflt;
    if (const char* e = r.env ? getenv(r.env) : nullptr) {
      char* end;
      const long x = strtol(e, &end, 10);
      if (end != e && r.accepts(x)) v = (int)x;
    }
    r.v.store(v, std::memory_order_relaxed);
  }
  return true;
}();

}  // namespace

int knob(Knob k) { return g_knobs[k].v.load(std::memory_order_relaxed); }

int tune(const char* key, int64_t value) {
  for (KnobRow& r : g_knobs) {
    if (strcmp(key, r.key)) continue;
    if (!r.accepts(value)) return -1;
    r.v.store((int)value, std::memory_order_relaxed);
    return 0;
  }
  return -1;
}

}  // namespace gdsm
