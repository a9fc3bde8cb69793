// Workgroup- and list-level building blocks shared by the list kernels (gfx950, wave64). Internal
// header; the lane-level primitives are in gdsm_common.h. Contracts: DESIGN.md, "Shared blocks".
#pragma once
#include "gdsm_common.h"

namespace gdsm {

// ---- a wave moves one 4 KiB page: four 16-B accesses per lane (lane l: chunks l + 64 q), every
// load in flight before the first use. kNT: nontemporal access (each call site keeps the form it
// was measured with).
template <bool kNT = false>
__device__ __forceinline__ void load_page(const uint8_t* __restrict__ src, uint32_t lane,
                                          u32x4 (&v)[4]) {
  const u32x4* s = reinterpret_cast<const u32x4*>(src);
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q)
    v[q] = kNT ? __builtin_nontemporal_load(s + lane + 64 * q) : s[lane + 64 * q];
}
template <bool kNT = false>
__device__ __forceinline__ void store_page(uint8_t* __restrict__ dst, uint32_t lane,
                                           const u32x4 (&v)[4]) {
  u32x4* d = reinterpret_cast<u32x4*>(dst);
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    if (kNT)
      __builtin_nontemporal_store(v[q], d + lane + 64 * q);
    else
      d[lane + 64 * q] = v[q];
  }
}

// ---- one workgroup of exactly 256 threads scans n u32 counts exclusively, 256 per step with a
// carry of type Acc: store(i, the sum of load(j) over j < i) for every i < n; returns the total in
// every thread. Contains __syncthreads(): every thread of the workgroup must call it, with the
// same n. load(i) is called once per i < n, by one thread.
template <typename Acc, typename Load, typename Store>
__device__ __forceinline__ Acc block_excl_scan(uint64_t n, Load load, Store store) {
  __shared__ uint32_t wtot[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Acc carry = 0;
  for (uint64_t c0 = 0; c0 < n; c0 += 256) {
    const uint64_t i = c0 + threadIdx.x;
    uint32_t v = 0;
    if (i < n) v = load(i);
    const uint32_t inc = wave_incl_sum(v);
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    Acc pre = carry;
    for (uint32_t w = 0; w < wave; ++w) pre += wtot[w];
    if (i < n) store(i, pre + inc - v);
    carry += (Acc)wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  return carry;
}

// ---- one report per wave that found something: when any lane's v is not 0, report(the OR of v
// over the wave) is called in one lane, the first whose v is not 0 (so a report's atomics are one
// per wave, not one per lane).
template <typename Report>
__device__ __forceinline__ void wave_report(uint32_t v, Report report) {
  const uint64_t any = __ballot(v != 0);
  if (!any) return;
  uint32_t w = v;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) w |= __shfl_xor(w, d, 64);
  if ((threadIdx.x & 63) == (uint32_t)__builtin_ctzll(any)) report(w);
}

}  // namespace gdsm
