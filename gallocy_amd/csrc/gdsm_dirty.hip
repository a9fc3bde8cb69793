// Dirty scan (SPEC §12): which listed pages differ between two arenas, as a compacted page list
// in list order, with the count and an upper bound of the diff stream of those pages. The GPU
// counterpart of gdsm_track_dirty for a writer that takes no faults.
//
// Three launches on the stream, ordered by their boundaries alone (no workgroup ever waits for
// another):
//   1. dirty_flag_kernel: the only one that touches the arenas. A workgroup takes a tile of 64
//      consecutive list entries, each of its 4 waves 16 of them, a wave per page in the layout of
//      load_page (gdsm_list.h): four 16-B loads per lane and arena, the two arenas' interleaved
//      (load_pair). The next entry's eight loads are
//      issued before the current entry is reduced, so a wave always has loads in flight; there is
//      no early exit inside a page (a clean page has to be read whole, and clean pages are the
//      common case). Lane l holds the 16-B chunks l + 64 q: XOR / OR to one "differs" bit per
//      chunk, a ballot and a popcount per quarter give C, the page's differing chunks. A wave
//      writes its 16 flag bits (a quarter of the tile's u64 flag word) and the sum of its dirty
//      pages' min(10244, 4 + 48 C).
//   2. dirty_sum_kernel: one workgroup; exclusive scan of the tiles' dirty counts (the popcount
//      of the flag word), the totals of counts and bounds into stats.
//   3. dirty_emit_kernel: a wave per flag word, lane = entry; its rank inside the word is
//      ballot_rank of the word.
// Flags, bounds and offsets are 32 B per 64 entries, next to the 512 KiB those entries read.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"

namespace gdsm {

namespace {

constexpr uint32_t kTile = 64;      // entries per workgroup = bits of a flag word
constexpr uint32_t kPerWave = 16;   // entries per wave
constexpr uint32_t kMaxRecord = 10244;  // SPEC §3's largest record

struct Pair {
  u32x4 a[4], b[4];
};

__device__ __forceinline__ void load_pair(const uint8_t* __restrict__ a,
                                          const uint8_t* __restrict__ b, uint64_t p, uint32_t lane,
                                          Pair& v) {
  const u32x4* pa = reinterpret_cast<const u32x4*>(a + p * kPage) + lane;
  const u32x4* pb = reinterpret_cast<const u32x4*>(b + p * kPage) + lane;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    v.a[q] = __builtin_nontemporal_load(pa + 64 * q);
    v.b[q] = __builtin_nontemporal_load(pb + 64 * q);
  }
}

// The 16-B chunks of the page in which the two copies differ (wave-uniform).
__device__ __forceinline__ uint32_t chunks_differing(const Pair& v) {
  uint32_t c = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const u32x4 x = v.a[q] ^ v.b[q];
    c += (uint32_t)__popcll(__ballot(((x.x | x.y) | (x.z | x.w)) != 0));
  }
  return c;
}

}  // namespace

// Workspace of a scan of n entries, T = ceil(n / 64) tiles: off[T] (u64: dirty entries before the
// tile), flags[T] (u64: bit e = entry 64 t + e is dirty), bound[4 T] (u32: one per wave).
uint64_t dirty_workspace_bytes(uint64_t n) {
  const uint64_t T = (n + kTile - 1) / kTile;
  return 32 * T + 64;
}

// ------------------------------------------------------------------------- flags and bounds
// Entry i = page ids[i] (NULL: page i). An id >= n_pages is not dirty (err |= 8; raw callers:
// n_pages = ~0, err = NULL). Every wave of the grid writes its 16 flag bits and its bound, also
// the waves past the list (zeros), so the workspace needs no clearing.
//
// A wave with all 16 entries (every wave but a list's last ones) runs straight-line code, two
// register sets in turn: entry j + 1 is issued before entry j is reduced. There is no branch
// between a load and its use: where paths with and without a pending load meet, the compiler
// waits for every load, and the loads kept in flight would be drained. So an id out of range
// loads page 0 (the arenas always hold it) and its result is dropped. The last waves of a list
// take their entries one at a time.
__global__ __launch_bounds__(256) void dirty_flag_kernel(const uint8_t* __restrict__ a,
                                                         const uint8_t* __restrict__ b,
                                                         const uint32_t* __restrict__ ids,
                                                         uint64_t n, uint64_t n_pages,
                                                         uint16_t* __restrict__ flags,
                                                         uint32_t* __restrict__ bound,
                                                         uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t slot = (uint64_t)blockIdx.x * 4 + wave;
  const uint64_t first = slot * kPerWave;
  const uint32_t cnt = first >= n ? 0u : (n - first < kPerWave ? (uint32_t)(n - first) : kPerWave);
  uint32_t mask = 0, bnd = 0, n_bad = 0;  // wave-uniform, as everything below but the loads
  if (cnt) {
    // the wave's ids, entry j in lanes j, j + 16, ... (past the list: its last entry again)
    uint32_t my_id = 0;
    if (ids) {
      const uint64_t i = first + (lane & (kPerWave - 1));
      my_id = ids[i < n ? i : n - 1];
    }
    auto issue = [&](uint32_t j, Pair& v) -> bool {
      const uint64_t p = ids ? (uint64_t)lane_bcast(my_id, (int)j) : first + j;
      const bool ok = p < n_pages;
      load_pair(a, b, ok ? p : 0, lane, v);
      return ok;
    };
    auto reduce = [&](uint32_t j, bool ok, const Pair& v) {
      const uint32_t c = ok ? chunks_differing(v) : 0u;
      const uint32_t r = 4u + 48u * c;
      mask |= (c ? 1u : 0u) << j;
      bnd += c ? (r < kMaxRecord ? r : kMaxRecord) : 0u;
      n_bad += ok ? 0u : 1u;
    };
    if (cnt == kPerWave) {
      Pair v[2];
      bool ok[2];
      ok[0] = issue(0, v[0]);
#pragma unroll
      for (uint32_t j = 0; j < kPerWave; ++j) {
        if (j + 1 < kPerWave) ok[(j + 1) & 1] = issue(j + 1, v[(j + 1) & 1]);
        reduce(j, ok[j & 1], v[j & 1]);
      }
    } else {
      for (uint32_t j = 0; j < cnt; ++j) {
        Pair v;
        const bool ok = issue(j, v);
        reduce(j, ok, v);
      }
    }
  }
  if (lane == 0) {
    flags[slot] = (uint16_t)mask;
    bound[slot] = bnd;
    if (n_bad && err) atomicOr(err, kErrIds);
  }
}

// ------------------------------------------------------------------------- tile counts -> offsets
// One workgroup: off[t] = the dirty entries before tile t; stats (may be NULL) = {their total, the
// sum of the bounds}.
__global__ __launch_bounds__(256) void dirty_sum_kernel(const uint64_t* __restrict__ flags,
                                                        const uint32_t* __restrict__ bound,
                                                        uint64_t T, uint64_t* __restrict__ off,
                                                        uint64_t* __restrict__ stats) {
  __shared__ uint64_t wbnd[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t bsum = 0;
  const uint64_t carry = block_excl_scan<uint64_t>(
      T,
      [&](uint64_t t) {
        const uint32_t dirty = (uint32_t)__popcll(flags[t]);
        bsum += (uint64_t)bound[4 * t] + bound[4 * t + 1] + bound[4 * t + 2] + bound[4 * t + 3];
        return dirty;
      },
      [&](uint64_t t, uint64_t before) { off[t] = before; });
  bsum = wave_sum64(bsum);
  if (lane == 0) wbnd[wave] = bsum;
  __syncthreads();
  if (threadIdx.x == 0 && stats) {
    stats[0] = carry;
    stats[1] = wbnd[0] + wbnd[1] + wbnd[2] + wbnd[3];
  }
}

// ------------------------------------------------------------------------- emit
// A wave per flag word, lane e = entry 64 t + e: the k-th dirty entry of the list goes to
// pages_out[k] / pos_out[k] (either may be NULL), k = off[t] + the set bits below e; entries at
// or past cap are dropped (stats[0] still counts them).
__global__ __launch_bounds__(256) void dirty_emit_kernel(const uint64_t* __restrict__ flags,
                                                         const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ ids,
                                                         uint64_t T, uint32_t* __restrict__ pages_out,
                                                         uint32_t* __restrict__ pos_out,
                                                         uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;  // wave-uniform
  const uint64_t w = flags[t];
  if (w == 0) return;  // wave-uniform: most words of a sparse interval
  if (!((w >> lane) & 1ull)) return;
  const uint64_t k = off[t] + ballot_rank(w);
  if (k >= cap) return;
  const uint64_t i = t * kTile + lane;
  if (pages_out) pages_out[k] = ids ? ids[i] : (uint32_t)i;
  if (pos_out) pos_out[k] = (uint32_t)i;
}

// ------------------------------------------------------------------------- launcher
hipError_t launch_dirty_scan(const uint8_t* a, const uint8_t* b, const uint32_t* ids, uint64_t n,
                             uint64_t n_pages, uint32_t* pages_out, uint32_t* pos_out,
                             uint64_t cap, uint64_t* stats, uint32_t* err, uint8_t* ws,
                             uint64_t ws_bytes, hipStream_t s) {
  if (n == 0) return stats ? hipMemsetAsync(stats, 0, 16, s) : hipSuccess;
  if (n > (1ull << 32) || ws_bytes < dirty_workspace_bytes(n)) return hipErrorInvalidValue;
  const uint64_t T = (n + kTile - 1) / kTile;
  uint64_t* off = reinterpret_cast<uint64_t*>(ws);
  uint64_t* flags = off + T;
  uint32_t* bound = reinterpret_cast<uint32_t*>(flags + T);
  hipLaunchKernelGGL(dirty_flag_kernel, dim3((unsigned)T), dim3(256), 0, s, a, b, ids, n, n_pages,
                     reinterpret_cast<uint16_t*>(flags), bound, err);
  hipLaunchKernelGGL(dirty_sum_kernel, dim3(1), dim3(256), 0, s, flags, bound, T, off, stats);
  if (cap && (pages_out || pos_out))
    hipLaunchKernelGGL(dirty_emit_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, s, flags, off,
                       ids, T, pages_out, pos_out, cap);
  return hipGetLastError();
}

}  // namespace gdsm
