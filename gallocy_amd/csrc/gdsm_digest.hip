// Page digest (SPEC §10) and the kernels behind gdsm_fetch_changed (SPEC §11): a fetch that moves
// only the pages whose digest at the requester differs from the home copy's. The transfers are in
// gdsm_exchange.cpp.
//
// The digest of a page is two u64 sums (S0, S1) over its 1024 u32 words, the NH construction of
// UMAC with two Toeplitz-shifted key rows: S_t = sum over the 512 word pairs of
// (x[2i] + K[2i + 4t]) * (x[2i+1] + K[2i+1 + 4t]), the adds mod 2^32, the sum mod 2^64. It is not
// a MAC: the keys are public, two unrelated pages collide with probability about 2^-64, a chosen
// pair can be made to collide.
//
// Shape, as every page move (load_page, gdsm_list.h): a wave per 4 KiB page, four 16-B loads per
// lane, all in flight before the arithmetic. Lane l always holds the words 4 (l + 64 q) .. + 3, q = 0 .. 3,
// so its keys are lane constants: 32 of them (8 per q: row 1's keys are row 0's four words on),
// computed once per wave and kept in registers over the wave's pages. Per page and lane that
// leaves 16 multiply-adds 32 x 32 -> 64 and 32 adds; the two u64 are then summed over the wave on
// DPP (no LDS) and lane 0 stores them.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"

namespace gdsm {

namespace {

// K[4 g + c], c = 0 .. 7, for the lane's 16-B units g = lane + 64 q (SPEC §10: K[j] = mix64(j + 1)
// >> 32).
struct LaneKeys {
  uint32_t k[4][8];
};
__device__ __forceinline__ void lane_keys(uint32_t lane, LaneKeys& K) {
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q)
#pragma unroll
    for (uint32_t c = 0; c < 8; ++c)
      K.k[q][c] = (uint32_t)(mix64(4ull * (lane + 64 * q) + c + 1) >> 32);
}

// (S0, S1) of the page held in v, in every lane.
__device__ __forceinline__ void digest_of(const u32x4 (&v)[4], const LaneKeys& K, uint64_t& s0,
                                          uint64_t& s1) {
  uint64_t a = 0, b = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t* k = K.k[q];
    a += (uint64_t)(v[q].x + k[0]) * (uint64_t)(v[q].y + k[1]);
    a += (uint64_t)(v[q].z + k[2]) * (uint64_t)(v[q].w + k[3]);
    b += (uint64_t)(v[q].x + k[4]) * (uint64_t)(v[q].y + k[5]);
    b += (uint64_t)(v[q].z + k[6]) * (uint64_t)(v[q].w + k[7]);
  }
  s0 = wave_sum64(a);
  s1 = wave_sum64(b);
}

__device__ __forceinline__ bool pages_differ(const u32x4 (&a)[4], const u32x4 (&b)[4]) {
  uint32_t d = 0;
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q)
    d |= (a[q].x ^ b[q].x) | (a[q].y ^ b[q].y) | (a[q].z ^ b[q].z) | (a[q].w ^ b[q].w);
  return __ballot(d != 0) != 0;
}

// The waves of a launch take list entries wave0, wave0 + stride, ...
__device__ __forceinline__ uint64_t wave0() { return (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }
__device__ __forceinline__ uint64_t wave_stride() { return (uint64_t)gridDim.x * 4; }

}  // namespace

// ------------------------------------------------------------------------- gdsm_digest
// out[2i], out[2i+1] = (S0, S1) of page ids[i] (NULL: page i) of `arena`; an id >= n_pages gets
// (0, 0) and err |= 8 (raw callers: n_pages = ~0, err = NULL, the list is theirs to get right).
__global__ __launch_bounds__(256) void digest_kernel(const uint8_t* __restrict__ arena,
                                                     const uint32_t* __restrict__ ids, uint64_t n,
                                                     uint64_t n_pages, uint64_t* __restrict__ out,
                                                     uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t i = wave0();
  if (i >= n) return;  // wave-uniform: no keys for a wave without a page
  LaneKeys K;
  lane_keys(lane, K);
  for (; i < n; i += wave_stride()) {
    const uint64_t p = ids ? ids[i] : i;
    if (p >= n_pages) {  // wave-uniform
      if (lane == 0) {
        out[2 * i] = 0;
        out[2 * i + 1] = 0;
        if (err) atomicOr(err, kErrIds);
      }
      continue;
    }
    u32x4 v[4];
    load_page(arena + p * kPage, lane, v);
    uint64_t s0, s1;
    digest_of(v, K, s0, s1);
    if (lane == 0) {
      out[2 * i] = s0;
      out[2 * i + 1] = s1;
    }
  }
}

// ------------------------------------------------------------------------- requester: offer
// dig[2k], dig[2k+1] = the digest of the requester's copy, page dst(i) of arena a, for its k-th
// entry homed elsewhere (entry i = k before skip_at, k + skip from there on, as
// fetch_place_kernel). A destination that is no longer valid offers (0, 0) (err bit 8).
__global__ __launch_bounds__(256) void fetchc_offer_kernel(const uint8_t* __restrict__ a,
                                                           const uint32_t* __restrict__ pages,
                                                           const uint32_t* __restrict__ dst_ids,
                                                           uint64_t skip_at, uint64_t skip,
                                                           uint64_t cnt, uint64_t n_pages,
                                                           uint64_t* __restrict__ dig,
                                                           uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t k = wave0();
  if (k >= cnt) return;
  LaneKeys K;
  lane_keys(lane, K);
  for (; k < cnt; k += wave_stride()) {
    const uint64_t i = k < skip_at ? k : k + skip;
    const uint64_t d = dst_ids ? dst_ids[i] : pages[i];
    uint64_t s0 = 0, s1 = 0;
    if (d < n_pages) {  // wave-uniform
      u32x4 v[4];
      load_page(a + d * kPage, lane, v);
      digest_of(v, K, s0, s1);
    } else if (lane == 0) {
      atomicOr(err, kErrIds);
    }
    if (lane == 0) {
      dig[2 * k] = s0;
      dig[2 * k + 1] = s1;
    }
  }
}

// ------------------------------------------------------------------------- home: verify
// flags[j] = 1 when the home copy of request j (page req[j] - base of src) does not have the
// digest the requester offered (dig[2j], dig[2j+1]), else 0. A request outside the home's block
// gets 0, so nothing is sent for it (err bit 8).
__global__ __launch_bounds__(256) void fetchc_verify_kernel(const uint8_t* __restrict__ src,
                                                            const uint32_t* __restrict__ req,
                                                            const uint64_t* __restrict__ dig,
                                                            uint64_t n, uint64_t base,
                                                            uint64_t block,
                                                            uint32_t* __restrict__ flags,
                                                            uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t j = wave0();
  if (j >= n) return;
  LaneKeys K;
  lane_keys(lane, K);
  for (; j < n; j += wave_stride()) {
    const uint64_t p = req[j];
    if (p < base || p - base >= block) {  // wave-uniform
      if (lane == 0) {
        flags[j] = 0;
        atomicOr(err, kErrIds);
      }
      continue;
    }
    u32x4 v[4];
    load_page(src + (p - base) * kPage, lane, v);
    uint64_t s0, s1;
    digest_of(v, K, s0, s1);
    if (lane == 0) flags[j] = (s0 != dig[2 * j] || s1 != dig[2 * j + 1]) ? 1u : 0u;
  }
}

// ------------------------------------------------------------------------- flags -> positions
// pos[i] = the number of set flags before entry i, pos[m] = their total: the slot of a changed
// page in the compacted staging, at the home (over all requesters' slices, so a slice's pages sit
// together, in request order) and at the requester (over its remote entries). 256 flags per block:
// kEmit = false counts a block's set flags, the scan turns the counts into offsets, kEmit = true
// writes the positions.
template <bool kEmit>
__global__ __launch_bounds__(256) void fetchc_pos_kernel(const uint32_t* __restrict__ flags,
                                                         uint64_t m, uint32_t* __restrict__ blk,
                                                         const uint32_t* __restrict__ blk_off,
                                                         uint32_t* __restrict__ pos) {
  __shared__ uint32_t wcnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool set = i < m && flags[i] != 0;
  uint64_t B;
  const uint32_t rank = ballot_rank(set, B);
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(B);
  __syncthreads();
  if (!kEmit) {
    if (threadIdx.x == 0) blk[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return;
  }
  if (i >= m) return;
  uint32_t at = blk_off[blockIdx.x] + rank;
  for (uint32_t w = 0; w < wave; ++w) at += wcnt[w];
  pos[i] = at;
}

// One workgroup: exclusive scan of the block counts and their total.
__global__ __launch_bounds__(256) void fetchc_scan_kernel(const uint32_t* __restrict__ blk,
                                                          uint64_t nblk,
                                                          uint32_t* __restrict__ blk_off,
                                                          uint32_t* __restrict__ total) {
  const uint32_t sum = block_excl_scan<uint32_t>(
      nblk, [&](uint64_t b) { return blk[b]; }, [&](uint64_t b, uint32_t off) { blk_off[b] = off; });
  if (threadIdx.x == 0) *total = sum;
}

// counts[p] = the changed pages of requester p's slice [off[p], off[p+1]) of the home's requests.
__global__ __launch_bounds__(256) void fetchc_slice_kernel(const uint32_t* __restrict__ pos,
                                                           const uint64_t* __restrict__ off,
                                                           uint32_t G,
                                                           uint64_t* __restrict__ counts) {
  const uint32_t t = threadIdx.x;
  if (t < G) counts[t] = pos[off[t + 1]] - pos[off[t]];
}

// ------------------------------------------------------------------------- home: gather
// staging[pos[j]] := page req[j] - base of src for the requests whose flag is set (the verify
// kernel sets none outside the block).
__global__ __launch_bounds__(256) void fetchc_gather_kernel(const uint8_t* __restrict__ src,
                                                            const uint32_t* __restrict__ req,
                                                            const uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ pos,
                                                            uint64_t n, uint64_t base,
                                                            uint64_t block,
                                                            uint8_t* __restrict__ staging) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t j = wave0(); j < n; j += wave_stride()) {
    const uint64_t p = req[j];
    if (flags[j] == 0 || p < base || p - base >= block) continue;  // wave-uniform
    u32x4 v[4];
    load_page(src + (p - base) * kPage, lane, v);
    store_page(staging + (uint64_t)pos[j] * kPage, lane, v);
  }
}

// ------------------------------------------------------------------------- requester: place
// Entry i of the list into a0 (the arena whose copy was offered) and, when not NULL, a1, at
// dst(i); changed[i] (when not NULL) = 1 when a0's page was replaced; stats (when not NULL) counts
// the replaced and the kept entries, one add per wave and counter.
// kLocal: entries [first, first + cnt), homed at this rank: a0's page is compared with the home
// copy (`from`, page pages[i] - base) byte for byte and stored only when it differs; a1 gets the
// home copy in either case (which is a0's page when they are equal). stats[2], stats[3].
// !kLocal: the cnt entries homed elsewhere (entry k before skip_at, k + skip from there on). With
// flags[k] set the page is at slot pos[k] of the staging (`from`) and goes to a0 and a1; otherwise
// a0 keeps its page and a1 becomes a copy of it. stats[0], stats[1].
// The list was validated by the split; an entry that changed since then moves nothing (err bit 8).
template <bool kLocal>
__global__ __launch_bounds__(256) void fetchc_place_kernel(const uint8_t* __restrict__ from,
                                                           const uint32_t* __restrict__ pages,
                                                           const uint32_t* __restrict__ dst_ids,
                                                           const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ pos,
                                                           uint64_t first, uint64_t skip_at,
                                                           uint64_t skip, uint64_t cnt,
                                                           uint64_t base, uint64_t block,
                                                           uint64_t n_pages,
                                                           uint8_t* __restrict__ a0,
                                                           uint8_t* __restrict__ a1,
                                                           uint32_t* __restrict__ changed,
                                                           uint64_t* __restrict__ stats,
                                                           uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  uint64_t n_new = 0, n_kept = 0;
  for (uint64_t k = wave0(); k < cnt; k += wave_stride()) {
    const uint64_t i = kLocal ? first + k : (k < skip_at ? k : k + skip);
    const uint64_t p = pages[i];
    const uint64_t d = dst_ids ? dst_ids[i] : p;
    if (d >= n_pages || (kLocal && (p < base || p - base >= block))) {  // wave-uniform
      if (lane == 0) atomicOr(err, kErrIds);
      continue;
    }
    bool differs;
    u32x4 v[4];
    if (kLocal) {
      u32x4 mine[4];
      load_page(from + (p - base) * kPage, lane, v);
      load_page(a0 + d * kPage, lane, mine);
      differs = pages_differ(v, mine);
      if (differs) store_page(a0 + d * kPage, lane, v);
      if (a1) store_page(a1 + d * kPage, lane, v);
    } else {
      differs = flags[k] != 0;  // wave-uniform
      if (differs) {
        load_page(from + (uint64_t)pos[k] * kPage, lane, v);
        store_page(a0 + d * kPage, lane, v);
        if (a1) store_page(a1 + d * kPage, lane, v);
      } else if (a1) {
        load_page(a0 + d * kPage, lane, v);
        store_page(a1 + d * kPage, lane, v);
      }
    }
    if (changed && lane == 0) changed[i] = differs ? 1u : 0u;
    n_new += differs ? 1 : 0;
    n_kept += differs ? 0 : 1;
  }
  if (stats && lane == 0) {
    unsigned long long* st = reinterpret_cast<unsigned long long*>(stats) + (kLocal ? 2 : 0);
    if (n_new) atomicAdd(st, (unsigned long long)n_new);
    if (n_kept) atomicAdd(st + 1, (unsigned long long)n_kept);
  }
}

// ------------------------------------------------------------------------- launchers
// Memory-bound, a wave per page: at most 2048 workgroups (8 per CU), the rest by the waves'
// stride, which also spreads a wave's key set-up over its pages.
static inline unsigned page_grid(uint64_t pages) { return grid_for(pages, 4, 2048); }

hipError_t launch_digest(const uint8_t* arena, const uint32_t* ids, uint64_t n, uint64_t n_pages,
                         uint64_t* out, uint32_t* err, hipStream_t s, Prof* prof) {
  if (n == 0) return hipSuccess;
  ProfScope ps(prof, GDSM_PROF_DIGEST, s);
  hipLaunchKernelGGL(digest_kernel, dim3(page_grid(n)), dim3(256), 0, s, arena, ids, n, n_pages,
                     out, err);
  return hipGetLastError();
}

hipError_t launch_fetchc_offer(const uint8_t* a, const uint32_t* pages, const uint32_t* dst_ids,
                               uint64_t skip_at, uint64_t skip, uint64_t cnt, uint64_t n_pages,
                               uint64_t* dig, uint32_t* err, hipStream_t s) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(fetchc_offer_kernel, dim3(page_grid(cnt)), dim3(256), 0, s, a, pages, dst_ids,
                     skip_at, skip, cnt, n_pages, dig, err);
  return hipGetLastError();
}

hipError_t launch_fetchc_verify(const uint8_t* src, const uint32_t* req, const uint64_t* dig,
                                uint64_t n, uint64_t base, uint64_t block, uint32_t* flags,
                                uint32_t* err, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fetchc_verify_kernel, dim3(page_grid(n)), dim3(256), 0, s, src, req, dig, n,
                     base, block, flags, err);
  return hipGetLastError();
}

uint64_t fetchc_pos_blocks(uint64_t m) { return (m + 255) / 256; }

hipError_t launch_fetchc_pos(const uint32_t* flags, uint64_t m, uint32_t* blk, uint32_t* blk_off,
                             uint32_t* pos, hipStream_t s) {
  const uint64_t nb = fetchc_pos_blocks(m);
  if (nb == 0) return hipMemsetAsync(pos, 0, 4, s);
  hipLaunchKernelGGL(fetchc_pos_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, flags, m, blk,
                     nullptr, nullptr);
  hipLaunchKernelGGL(fetchc_scan_kernel, dim3(1), dim3(256), 0, s, blk, nb, blk_off, pos + m);
  hipLaunchKernelGGL(fetchc_pos_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, flags, m,
                     nullptr, blk_off, pos);
  return hipGetLastError();
}

hipError_t launch_fetchc_slices(const uint32_t* pos, const uint64_t* off, uint32_t G,
                                uint64_t* counts, hipStream_t s) {
  if (G > kFetchMaxRanks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fetchc_slice_kernel, dim3(1), dim3(256), 0, s, pos, off, G, counts);
  return hipGetLastError();
}

hipError_t launch_fetchc_gather(const uint8_t* src, const uint32_t* req, const uint32_t* flags,
                                const uint32_t* pos, uint64_t n, uint64_t base, uint64_t block,
                                uint8_t* staging, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fetchc_gather_kernel, dim3(page_grid(n)), dim3(256), 0, s, src, req, flags,
                     pos, n, base, block, staging);
  return hipGetLastError();
}

hipError_t launch_fetchc_place(const uint8_t* staging, const uint32_t* pages,
                               const uint32_t* dst_ids, const uint32_t* flags, const uint32_t* pos,
                               uint64_t skip_at, uint64_t skip, uint64_t cnt, uint64_t n_pages,
                               uint8_t* a0, uint8_t* a1, uint32_t* changed, uint64_t* stats,
                               uint32_t* err, hipStream_t s) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(fetchc_place_kernel<false>, dim3(page_grid(cnt)), dim3(256), 0, s, staging,
                     pages, dst_ids, flags, pos, 0ull, skip_at, skip, cnt, 0ull, 0ull, n_pages, a0,
                     a1, changed, stats, err);
  return hipGetLastError();
}

hipError_t launch_fetchc_local(const uint8_t* src, const uint32_t* pages, const uint32_t* dst_ids,
                               uint64_t first, uint64_t cnt, uint64_t base, uint64_t block,
                               uint64_t n_pages, uint8_t* a0, uint8_t* a1, uint32_t* changed,
                               uint64_t* stats, uint32_t* err, hipStream_t s) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(fetchc_place_kernel<true>, dim3(page_grid(cnt)), dim3(256), 0, s, src, pages,
                     dst_ids, nullptr, nullptr, first, 0ull, 0ull, cnt, base, block, n_pages, a0,
                     a1, changed, stats, err);
  return hipGetLastError();
}

}  // namespace gdsm
