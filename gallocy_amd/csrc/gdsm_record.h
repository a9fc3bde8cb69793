// Device-side validation of one SPEC §3 record (the rules gdsm_apply refuses by, SPEC §4), shared
// by the apply kernels (gdsm_pages.hip) and the merge kernels (gdsm_merge.hip). Internal header.
#pragma once
#include "gdsm_common.h"

namespace gdsm {

// A group is one 16-lane DPP row (kW = 16) or the whole wave (kW = 64).
template <uint32_t kW>
__device__ __forceinline__ uint32_t grp_incl_sum(uint32_t x) {
  return kW == 16 ? row_incl_sum(x) : wave_incl_sum(x);
}
template <uint32_t kW>
__device__ __forceinline__ uint32_t grp_incl_max(uint32_t x) {
  return kW == 16 ? row_incl_max(x) : wave_incl_max(x);
}
template <uint32_t kW>
__device__ __forceinline__ uint32_t grp_last(uint32_t x) {
  return kW == 16 ? row_last(x) : lane_bcast(x, 63);
}
template <uint32_t kW>
__device__ __forceinline__ uint32_t grp_prev(uint32_t x) {
  return kW == 16 ? row_prev(x) : from_prev_lane(x);
}

// Validates every header of the group's record (`size` bytes at rec32; `has` false for a group
// without a record), a lane per run, kW runs per step: every run non-empty and inside the page,
// runs sorted and non-overlapping, and the size equal to what the headers imply. nr = the run
// count the caller read and bounded (as record_check below does), bad = its verdict so far. Returns
// true in the lanes of a group whose record is malformed.
template <uint32_t kW, typename P32>
__device__ __forceinline__ bool record_runs_check(P32 rec32, uint32_t size, bool has, uint32_t nr,
                                                  bool bad) {
  static_assert(kW == 16 || kW == 64, "a DPP row or the wave");
  const uint32_t lane = lane_id(), lr = lane & (kW - 1);
  const uint32_t nit = lane_bcast(wave_incl_max((nr + kW - 1) / kW), 63);
  uint32_t pay = 0, prev_end = 0, lbad = 0;
  for (uint32_t it = 0; it < nit; ++it) {
    const uint32_t r = it * kW + lr;
    const bool v = r < nr;
    const uint32_t h = v ? rec32[1 + r] : 0u;
    const uint32_t off = h & 0xFFFFu, len = h >> 16, end = v ? off + len : 0u;
    uint32_t pe = grp_prev<kW>(end);
    if (lr == 0) pe = prev_end;
    if (v && (len == 0 || end > kPage || off < pe)) lbad = 1;
    pay += grp_last<kW>(grp_incl_sum<kW>(v ? len : 0u));
    prev_end = grp_last<kW>(end);
  }
  if (grp_last<kW>(grp_incl_max<kW>(lbad))) bad = true;
  if (has && !bad && size != 4u + 4u * nr + ((pay + 3u) & ~3u)) bad = true;
  return bad;
}

// The whole check: nruns in 1..2048 and its headers inside `size` (so no header past the record
// is ever read), then record_runs_check. nr = the run count, 0 for a malformed record.
template <uint32_t kW, typename P32>
__device__ __forceinline__ bool record_check(P32 rec32, uint32_t size, bool has, uint32_t& nr) {
  nr = has ? rec32[0] : 0u;
  bool bad = has && (nr == 0 || nr > kMaxRuns || size < 4u + 4u * nr);
  if (bad) nr = 0;
  bad = record_runs_check<kW>(rec32, size, has, nr, bad);
  if (bad) nr = 0;
  return bad;
}

}  // namespace gdsm
