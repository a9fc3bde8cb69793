// Page fetch (SPEC §9): the kernels behind gdsm_fetch (pages from their home copies to the nodes)
// and gdsm_notices_fetch_list (a node's notices -> the list of pages it has to fetch). The
// transfers themselves are in gdsm_exchange.cpp.
//
// This is the "copy over the latest contents" step of the reference's description of a fault
// (resources/NUTSHELL.md:61-69), which it would carry over its HTTP fan-out
// (gallocy/http/client.cpp:39-91); none of it is implemented there.
//
// Page moves are pure bandwidth (no arithmetic): a wave per 4 KiB page, four 16-B loads per lane,
// all in flight before the stores (load_page / store_page, gdsm_list.h, which twin_kernel of
// gdsm_pages.hip uses too). Plain cached loads and stores:
// on this part nontemporal loads and/or stores measured 0.3-4.5 % slower for the same wave-per-page
// copy (launch_twin), and an `nt` store keeps its line in L2 like a plain one
// (MI355X_MICROARCH.md, stores of each flavour), so the hint buys nothing here. With both
// destination arenas named the source is read once and stored twice.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"

namespace gdsm {

// ------------------------------------------------------------------------- requester: split
// Validates a rank's request list (strictly ascending, page < total_pages, destination < n_pages)
// and finds each home's slice by binary search: bounds[d] = first entry of a page >= d * per,
// counts[d] = its length (u64, the all-to-all input). bad |= 1 on any invalid entry (the call is
// then refused); the bounds are made non-decreasing whatever the list holds, so the counts always
// sum to n.
__global__ __launch_bounds__(256) void fetch_split_kernel(const uint32_t* __restrict__ pages,
                                                          const uint32_t* __restrict__ dst_ids,
                                                          uint64_t n, uint64_t total_pages,
                                                          uint64_t per, uint32_t G,
                                                          uint64_t n_pages,
                                                          uint64_t* __restrict__ counts,
                                                          uint64_t* __restrict__ bounds,
                                                          uint32_t* __restrict__ bad) {
  uint32_t v = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t p = pages[i];
    if (p >= total_pages) v = 1;
    if (i + 1 < n && pages[i + 1] <= p) v = 1;
    const uint64_t d = dst_ids ? dst_ids[i] : p;
    if (d >= n_pages) v = 1;
  }
  if (__ballot(v) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
  if (blockIdx.x != 0) return;  // block-uniform
  __shared__ uint64_t b[kFetchMaxRanks + 1];
  const uint32_t t = threadIdx.x;
  if (t <= G) {
    const uint64_t first = (uint64_t)t * per;
    uint64_t lo = 0, hi = n;
    if (t == G || first >= total_pages) {
      lo = n;
    } else {
      while (lo < hi) {  // first index with pages >= first
        const uint64_t mid = (lo + hi) >> 1;
        if (pages[mid] < first) lo = mid + 1; else hi = mid;
      }
    }
    b[t] = lo;
  }
  __syncthreads();
  if (t == 0)  // (an unsorted list: searches may disagree; the list is refused, the counts stay sane)
    for (uint32_t k = 1; k <= G; ++k)
      if (b[k] < b[k - 1]) b[k] = b[k - 1];
  __syncthreads();
  if (t <= G) bounds[t] = b[t];
  if (t < G) counts[t] = b[t + 1] - b[t];
}

// ------------------------------------------------------------------------- page moves
// Home side: staging[j] := page req[j] - base of the home's source arena, for the n requests
// received. An id outside the home's block [base, base + block) copies nothing and sets err bit 8
// (the next gdsm_sync reports -EINVAL); it never addresses outside the arena.
__global__ __launch_bounds__(256) void fetch_gather_kernel(const uint8_t* __restrict__ src,
                                                           const uint32_t* __restrict__ req,
                                                           uint64_t n, uint64_t base,
                                                           uint64_t block,
                                                           uint8_t* __restrict__ staging,
                                                           uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t j = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); j < n;
       j += (uint64_t)gridDim.x * 4) {
    const uint64_t p = req[j];
    if (p < base || p - base >= block) {  // wave-uniform: one page per wave step
      if (lane == 0) atomicOr(err, kErrIds);
      continue;
    }
    u32x4 v[4];
    load_page(src + (p - base) * kPage, lane, v);
    store_page(staging + j * kPage, lane, v);
  }
}

// Requester side: list entry i's page into the destination arenas a0 and (when not NULL) a1 at
// dst(i) = dst_ids ? dst_ids[i] : pages[i], read once.
// kLocal: entries [first, first + cnt), homed at this rank, straight from its source arena
// (`from`, page pages[i] - base of the block [base, base + block)).
// !kLocal: the cnt entries homed elsewhere, from the staging the homes filled (`from`, page k for
// the k-th such entry: entry k before skip_at, entry k + skip from there on, where [skip_at,
// skip_at + skip) are the local entries).
// The list was validated by the split; an entry that changed since then copies nothing (err bit 8).
template <bool kLocal>
__global__ __launch_bounds__(256) void fetch_place_kernel(const uint8_t* __restrict__ from,
                                                          const uint32_t* __restrict__ pages,
                                                          const uint32_t* __restrict__ dst_ids,
                                                          uint64_t first, uint64_t skip_at,
                                                          uint64_t skip, uint64_t cnt,
                                                          uint64_t base, uint64_t block,
                                                          uint64_t n_pages,
                                                          uint8_t* __restrict__ a0,
                                                          uint8_t* __restrict__ a1,
                                                          uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint64_t k = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); k < cnt;
       k += (uint64_t)gridDim.x * 4) {
    const uint64_t i = kLocal ? first + k : (k < skip_at ? k : k + skip);
    const uint64_t p = pages[i];
    const uint64_t d = dst_ids ? dst_ids[i] : p;
    if (d >= n_pages || (kLocal && (p < base || p - base >= block))) {  // wave-uniform
      if (lane == 0) atomicOr(err, kErrIds);
      continue;
    }
    u32x4 v[4];
    load_page(from + (kLocal ? p - base : k) * kPage, lane, v);
    store_page(a0 + d * kPage, lane, v);
    if (a1) store_page(a1 + d * kPage, lane, v);
  }
}

// ------------------------------------------------------------------------- notices -> fetch list
// A notice (SPEC §5b) names a page this node must fetch: no access before, and the access after is
// one `want` selects (bit 0: read, bit 1: write). An upgrade 1 -> 2 needs no contents.
__device__ __forceinline__ bool fetch_wanted(uint64_t x, uint32_t want) {
  const uint32_t before = (uint32_t)(x >> 32) & 3u, after = (uint32_t)(x >> 34) & 3u;
  return before == 0 && (after == 1 || after == 2) && ((want >> (after - 1)) & 1u);
}

// One notice per thread, 256 per block. kEmit = false: the block's count of wanted notices.
// kEmit = true: their pages at blk_off[block] + their rank inside the block (notice order, so the
// list stays ascending); entries past cap are dropped (the call then reports -ENOSPC).
template <bool kEmit>
__global__ __launch_bounds__(256) void fetch_list_kernel(const uint64_t* __restrict__ notices,
                                                         uint64_t n, uint32_t want,
                                                         uint32_t* __restrict__ blk,
                                                         const uint64_t* __restrict__ blk_off,
                                                         uint32_t* __restrict__ out,
                                                         uint64_t cap) {
  __shared__ uint32_t wcnt[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t x = i < n ? notices[i] : 0;
  const bool keep = i < n && fetch_wanted(x, want);
  uint64_t B;
  const uint32_t rank = ballot_rank(keep, B);
  if (lane == 0) wcnt[wave] = (uint32_t)__popcll(B);
  __syncthreads();
  if (!kEmit) {
    if (threadIdx.x == 0) blk[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    return;
  }
  if (!keep) return;
  uint64_t at = blk_off[blockIdx.x] + rank;
  for (uint32_t w = 0; w < wave; ++w) at += wcnt[w];
  if (at < cap) out[at] = (uint32_t)x;
}

// One workgroup: exclusive scan of the block counts (blk -> blk_off) and their total.
__global__ __launch_bounds__(256) void fetch_list_scan_kernel(const uint32_t* __restrict__ blk,
                                                              uint64_t nblk,
                                                              uint64_t* __restrict__ blk_off,
                                                              uint64_t* __restrict__ total) {
  const uint64_t sum = block_excl_scan<uint64_t>(
      nblk, [&](uint64_t b) { return blk[b]; }, [&](uint64_t b, uint64_t off) { blk_off[b] = off; });
  if (threadIdx.x == 0) *total = sum;
}

// ------------------------------------------------------------------------- launchers
hipError_t launch_fetch_split(const uint32_t* pages, const uint32_t* dst_ids, uint64_t n,
                              uint64_t total_pages, uint64_t per, uint32_t G, uint64_t n_pages,
                              uint64_t* counts, uint64_t* bounds, uint32_t* bad, hipStream_t s) {
  if (G > kFetchMaxRanks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fetch_split_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, pages,
                     dst_ids, n, total_pages, per, G, n_pages, counts, bounds, bad);
  return hipGetLastError();
}

hipError_t launch_fetch_gather(const uint8_t* src, const uint32_t* req, uint64_t n, uint64_t base,
                               uint64_t block, uint8_t* staging, uint32_t* err, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(fetch_gather_kernel, dim3(grid_for(n, 4, 16384)), dim3(256), 0, s, src, req, n,
                     base, block, staging, err);
  return hipGetLastError();
}

hipError_t launch_fetch_scatter(const uint8_t* staging, const uint32_t* pages,
                                const uint32_t* dst_ids, uint64_t skip_at, uint64_t skip,
                                uint64_t cnt, uint64_t n_pages, uint8_t* a0, uint8_t* a1,
                                uint32_t* err, hipStream_t s) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(fetch_place_kernel<false>, dim3(grid_for(cnt, 4, 16384)), dim3(256), 0, s,
                     staging, pages, dst_ids, 0ull, skip_at, skip, cnt, 0ull, 0ull, n_pages, a0, a1,
                     err);
  return hipGetLastError();
}

hipError_t launch_fetch_local(const uint8_t* src, const uint32_t* pages, const uint32_t* dst_ids,
                              uint64_t first, uint64_t cnt, uint64_t base, uint64_t block,
                              uint64_t n_pages, uint8_t* a0, uint8_t* a1, uint32_t* err,
                              hipStream_t s) {
  if (cnt == 0) return hipSuccess;
  hipLaunchKernelGGL(fetch_place_kernel<true>, dim3(grid_for(cnt, 4, 16384)), dim3(256), 0, s, src,
                     pages, dst_ids, first, 0ull, 0ull, cnt, base, block, n_pages, a0, a1, err);
  return hipGetLastError();
}

uint64_t fetch_list_blocks(uint64_t n) { return (n + 255) / 256; }

hipError_t launch_fetch_list(const uint64_t* notices, uint64_t n, uint32_t want, uint32_t* blk,
                             uint64_t* blk_off, uint64_t* total, uint32_t* out, uint64_t cap,
                             hipStream_t s) {
  const uint64_t nb = fetch_list_blocks(n);
  if (nb == 0) return hipMemsetAsync(total, 0, 8, s);
  hipLaunchKernelGGL(fetch_list_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, notices, n,
                     want, blk, nullptr, nullptr, 0ull);
  hipLaunchKernelGGL(fetch_list_scan_kernel, dim3(1), dim3(256), 0, s, blk, nb, blk_off, total);
  hipLaunchKernelGGL(fetch_list_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, notices, n,
                     want, nullptr, blk_off, out, cap);
  return hipGetLastError();
}

}  // namespace gdsm
