// The page table by page list (SPEC §15): gdsm_coh_clean clears the dirty bit of the listed pages
// that `node` owns; gdsm_coh_lookup reads a field of the listed pages' words. Entry i works on
// table page p = ids[i] - base (ids NULL: p = i).
//
// One launch each, no workspace. The list is only 4-B aligned, so entries are counted from the
// 16-B boundary at or before ids: position q = i + lead, lead = the 0..3 list elements between that
// boundary and ids[0]. A lane takes the 4 positions [4 t, 4 t + 4), a workgroup of 256 lanes 1024
// positions. A lane whose 4 positions are all entries (the body) gets its ids with one 16-B load;
// the first lane (lead != 0) and the last one take their entries singly, each guarded by the list.
// The 4 table loads of a lane are unconditional (an entry that is no entry, or whose id is out of
// range, reads table page 0 and ignores it), so all of them are in flight before the first use.
// clean: the status comes from the loaded word; only a lane whose word is owned and dirty issues
// the 32-bit atomic AND on the state half, and the old value says whether it was the one that
// cleaned (repeats in the list: exactly one of them). The faults half is never written. The four
// counts are ballots per wave, kept in scalar registers over the workgroup's tiles and summed over
// the workgroup in LDS at the end: one atomic per counter and workgroup, and none for a counter
// that is 0. Every workgroup's atomics hit the same 32 bytes of stats and are served one after the
// other (about 9 ns each, derived from one run: DESIGN §4t), so the clean grid is capped at kCleanBlocks
// workgroups (8 waves per SIMD on 256 CUs) which stride over the tiles; lookup, which counts
// nothing, launches a workgroup per tile. A lane's 4 status bytes are one 4-B store and its 4 out
// words one 16-B store where the output pointer allows, else single stores.
#include "gdsm_common.h"
#include "gdsm_launch.h"

namespace gdsm {

namespace {

constexpr uint32_t kPer = 4;             // entries of a lane
// positions of a workgroup; tests/test_gpu_cohlist.py has it as T (list lengths T - 1, T, T + 1) and
// kCleanBlocks as CLEAN_BLOCKS (a list of more tiles than workgroups): change them together
constexpr uint32_t kTile = 256 * kPer;
constexpr uint32_t kDirtyBit = 1u << 18;
constexpr uint64_t kCleanBlocks = 2048;  // workgroups of a clean at most

// The lane's 4 entries: i0 = the entry of its first position (negative in the first lane where
// lead != 0); in[k]: position k is an entry; p[k]: its table page, 0 where !ok[k]; ok[k]: an entry
// with a page inside the table; returns whether any entry's id was out of range.
__device__ __forceinline__ bool load_entries(const uint32_t* __restrict__ ids, uint64_t n,
                                             uint32_t lead, uint64_t base, uint64_t n_pages,
                                             uint64_t t, int64_t& i0, bool (&in)[kPer],
                                             bool (&ok)[kPer], uint64_t (&p)[kPer]) {
  const uint64_t q0 = t * kPer;
  i0 = (int64_t)q0 - (int64_t)lead;
  const bool body = q0 >= lead && q0 + kPer <= n + lead;
  uint32_t id[kPer] = {0, 0, 0, 0};
  if (body) {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) in[k] = true;
    if (ids) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(ids + i0);  // 16-B aligned by lead
      id[0] = v.x;
      id[1] = v.y;
      id[2] = v.z;
      id[3] = v.w;
    }
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      const int64_t i = i0 + (int64_t)k;
      in[k] = i >= 0 && (uint64_t)i < n;
      if (ids && in[k]) id[k] = ids[i];
    }
  }
  bool bad = false;
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint64_t page = ids ? (uint64_t)id[k] - base : (uint64_t)(i0 + (int64_t)k);
    const bool inside = ids ? (id[k] >= base && page < n_pages) : true;  // (host: n <= n_pages)
    ok[k] = in[k] && inside;
    bad |= in[k] && !inside;
    p[k] = ok[k] ? page : 0;
  }
  return bad;
}

// Every word of w is needed here: keeps the compiler from sinking a lane's table loads into the
// branches that use them one by one (a dependent round trip each); it costs no instruction.
__device__ __forceinline__ void all_loaded(uint32_t (&w)[kPer]) {
  asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
}

}  // namespace

// ------------------------------------------------------------------------- clean
namespace {

// One tile: the workgroup's 256 lanes take its 1024 positions; c += the wave's counts (wave-uniform).
__device__ __forceinline__ void clean_tile(uint64_t* __restrict__ pt,
                                           const uint32_t* __restrict__ ids, uint64_t n,
                                           uint32_t lead, uint64_t base, uint64_t n_pages,
                                           uint32_t node, uint64_t tile,
                                           uint8_t* __restrict__ status_out, bool count,
                                           uint32_t* __restrict__ err, uint32_t (&c)[4]) {
  const uint64_t t = tile * 256 + threadIdx.x;
  int64_t i0;
  bool in[kPer], ok[kPer];
  uint64_t p[kPer];
  const bool bad = load_entries(ids, n, lead, base, n_pages, t, i0, in, ok, p);
  uint32_t w[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) w[k] = *reinterpret_cast<const uint32_t*>(pt + p[k]);
  all_loaded(w);
  // the status the loaded word gives; 0 = "owned and dirty": the atomic decides
  uint32_t st[kPer];
  bool need[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const uint32_t o = (w[k] >> 8) & 0xFFu, s = (w[k] >> 16) & 3u;
    st[k] = !ok[k] ? 4u : s == 0 ? 3u : o != node ? 2u : (w[k] & kDirtyBit) ? 0u : 1u;
    need[k] = st[k] == 0;
  }
  uint32_t old[kPer];  // (the loaded word where no atomic is issued: not looked at)
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) old[k] = w[k];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k)
    if (need[k]) old[k] = atomicAnd(reinterpret_cast<uint32_t*>(pt + p[k]), ~kDirtyBit);
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k)
    if (need[k] && !(old[k] & kDirtyBit)) st[k] = 1;  // another entry of this page cleaned it
  if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(err, kErrIds);
  if (status_out) {
    if (in[0] && in[3] && ((reinterpret_cast<uintptr_t>(status_out) + (uint64_t)i0) & 3) == 0) {
      *reinterpret_cast<uint32_t*>(status_out + i0) =
          st[0] | (st[1] << 8) | (st[2] << 16) | (st[3] << 24);
    } else {
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k)
        if (in[k]) status_out[i0 + (int64_t)k] = (uint8_t)st[k];
    }
  }
  if (count) {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k) {
      c[0] += (uint32_t)__popcll(__ballot(in[k] && st[k] == 0));
      c[1] += (uint32_t)__popcll(__ballot(in[k] && st[k] == 1));
      c[2] += (uint32_t)__popcll(__ballot(in[k] && st[k] == 2));
      c[3] += (uint32_t)__popcll(__ballot(in[k] && st[k] >= 3));
    }
  }
}

}  // namespace

// Workgroup b takes tiles b, b + gridDim.x, ...
__global__ __launch_bounds__(256) void coh_clean_kernel(uint64_t* __restrict__ pt,
                                                        const uint32_t* __restrict__ ids,
                                                        uint64_t n, uint32_t lead, uint64_t base,
                                                        uint64_t n_pages, uint32_t node,
                                                        uint64_t tiles,
                                                        uint8_t* __restrict__ status_out,
                                                        unsigned long long* __restrict__ stats,
                                                        uint32_t* __restrict__ err) {
  __shared__ uint32_t s_cnt[4][4];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t c[4] = {0, 0, 0, 0};  // at most 256 per tile: 2^32 entries on 2048 workgroups fit
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x)
    clean_tile(pt, ids, n, lead, base, n_pages, node, tile, status_out, stats != nullptr, err, c);
  if (!stats) return;  // (kernel argument: the whole grid returns)
  if (lane == 0) {
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) s_cnt[wave][j] = c[j];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const uint32_t j = threadIdx.x;
    const uint32_t sum = s_cnt[0][j] + s_cnt[1][j] + s_cnt[2][j] + s_cnt[3][j];
    if (sum) atomicAdd(stats + j, (unsigned long long)sum);
  }
}

// ------------------------------------------------------------------------- lookup
template <bool kFaults>
__global__ __launch_bounds__(256) void coh_lookup_kernel(const uint64_t* __restrict__ pt,
                                                         const uint32_t* __restrict__ ids,
                                                         uint64_t n, uint32_t lead, uint64_t base,
                                                         uint64_t n_pages, uint32_t shift,
                                                         uint32_t mask, uint32_t* __restrict__ out,
                                                         uint32_t* __restrict__ faults_out,
                                                         uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t i0;
  bool in[kPer], ok[kPer];
  uint64_t p[kPer];
  const bool bad = load_entries(ids, n, lead, base, n_pages, t, i0, in, ok, p);
  uint32_t w[kPer], f[kPer];
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    if constexpr (kFaults) {
      const uint64_t e = pt[p[k]];
      w[k] = (uint32_t)e;
      f[k] = (uint32_t)(e >> 32);
    } else {
      w[k] = *reinterpret_cast<const uint32_t*>(pt + p[k]);
      f[k] = 0;
    }
  }
  all_loaded(w);
#pragma unroll
  for (uint32_t k = 0; k < kPer; ++k) {
    const bool live = ok[k] && ((w[k] >> 16) & 3u) != 0;
    w[k] = live ? (w[k] >> shift) & mask : 0u;
    f[k] = ok[k] ? f[k] : 0u;
  }
  if (__ballot(bad) && lane == 0) atomicOr(err, kErrIds);
  const bool whole = in[0] && in[3];
  if (whole && (reinterpret_cast<uintptr_t>(out + i0) & 15) == 0) {
    *reinterpret_cast<u32x4*>(out + i0) = u32x4{w[0], w[1], w[2], w[3]};
  } else {
#pragma unroll
    for (uint32_t k = 0; k < kPer; ++k)
      if (in[k]) out[i0 + (int64_t)k] = w[k];
  }
  if constexpr (kFaults) {
    if (whole && (reinterpret_cast<uintptr_t>(faults_out + i0) & 15) == 0) {
      *reinterpret_cast<u32x4*>(faults_out + i0) = u32x4{f[0], f[1], f[2], f[3]};
    } else {
#pragma unroll
      for (uint32_t k = 0; k < kPer; ++k)
        if (in[k]) faults_out[i0 + (int64_t)k] = f[k];
    }
  }
}

// ------------------------------------------------------------------------- launchers
namespace {

// The list elements between the 16-B boundary at or before ids and ids[0].
inline uint32_t lead_of(const uint32_t* ids) {
  return (uint32_t)((reinterpret_cast<uintptr_t>(ids) & 15) / 4);
}

}  // namespace

hipError_t launch_coh_clean(uint64_t* pt, uint64_t n_pages, uint32_t node, const uint32_t* ids,
                            uint64_t n, uint64_t base, uint8_t* status_out, uint64_t* stats,
                            uint32_t* err, hipStream_t s) {
  // a refused call enqueues nothing; a table of 0 pages has no page 0 for the kernel to fall back on
  if (n > (1ull << 32) || (n && n_pages == 0) || (!ids && n > n_pages))
    return hipErrorInvalidValue;
  if (stats) {
    hipError_t e = hipMemsetAsync(stats, 0, 32, s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) return hipSuccess;
  const uint32_t lead = lead_of(ids);
  const uint64_t tiles = (n + lead + kTile - 1) / kTile;
  const uint64_t blocks = tiles < kCleanBlocks ? tiles : kCleanBlocks;
  hipLaunchKernelGGL(coh_clean_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pt, ids, n, lead,
                     base, n_pages, node, tiles, status_out,
                     reinterpret_cast<unsigned long long*>(stats), err);
  return hipGetLastError();
}

hipError_t launch_coh_lookup(const uint64_t* pt, uint64_t n_pages, const uint32_t* ids, uint64_t n,
                             uint64_t base, uint32_t shift, uint32_t mask, uint32_t* out,
                             uint32_t* faults_out, uint32_t* err, hipStream_t s) {
  if (n == 0) return hipSuccess;
  if (n > (1ull << 32) || n_pages == 0 || shift > 31 || !out || (!ids && n > n_pages))
    return hipErrorInvalidValue;
  const uint32_t lead = lead_of(ids);
  const uint64_t blocks = (n + lead + kTile - 1) / kTile;
  if (faults_out)
    hipLaunchKernelGGL(coh_lookup_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, pt, ids,
                       n, lead, base, n_pages, shift, mask, out, faults_out, err);
  else
    hipLaunchKernelGGL(coh_lookup_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, pt, ids,
                       n, lead, base, n_pages, shift, mask, out, faults_out, err);
  return hipGetLastError();
}

}  // namespace gdsm
