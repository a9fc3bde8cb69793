// gdsm_runs_split for gfx950 (docs/SPEC.md §13): one diff stream taken apart into one stream per
// destination, a stable multi-way partition of its records. Record i goes to the destinations its
// mask names (mask form: any subset of G <= 8, so a record may be copied several times) or to the
// home of its page (home form: ids[i] / per, the page rewritten to the home's REPLICA index).
// Records are opaque: they are copied byte for byte, never parsed.
//
// Five launches and one 4-B memset on one stream, ordered by their boundaries alone (no wave ever
// waits for another, no host read in between):
//   split_check_kernel  the input's offsets (from 0, non-decreasing, 4-aligned, inside the
//                       capacity: the rules merge_check_kernel applies) before anything is read
//                       through them;
//                       a failure sets the `fatal` word, which empties everything after it
//   split_count_kernel  a workgroup per tile of 256 records, a thread per record: the record's
//                       destinations (a bit >= G or a home >= G is fatal too) and size, reduced to
//                       the tile's {records, bytes} per destination (ballots and wave sums: no
//                       atomics, so the counts do not depend on the scheduling order)
//   split_scan_kernel   one workgroup, a wave per (destination, records | bytes): the exclusive
//                       scan of the tile sums in place (256 tiles a step), the totals into
//                       `counts`, and the last offset rec_off[c_d] = b_d of every output
//   split_index_kernel  the count kernel's geometry again: the record's rank and byte offset in
//                       each of its destinations (tile prefix + the recount inside the tile), the
//                       output's rec_off entry and page id
//   split_copy_kernel   the bytes. A persistent grid walks fixed 16 KiB spans of the INPUT data, so
//                       the work is balanced by bytes whatever the records' sizes. A workgroup
//                       stages its span in LDS with aligned 16-B loads: every input byte is read
//                       from memory once, however many destinations it has. The span's first record
//                       is found by a 64-ary search of rec_off; its position in every output is the
//                       scanned tile prefix plus a recount of its tile's records before it (256
//                       masks and offsets, from L2), so no n x G table of positions exists. The
//                       span's records are then taken 256 at a time: a block scan per destination of
//                       the bytes each record has inside the span gives, in LDS, where they lie in
//                       that destination, which is one contiguous range (the split is stable). The
//                       range is walked in 16-B chunks aligned on the DESTINATION address: a lane
//                       finds its chunk's record by binary search in the LDS prefix, gathers four
//                       dwords from the staged span (LDS reads at any 4-B alignment, so the 0 / 4 /
//                       8 / 12 offset between source and destination costs nothing in memory
//                       traffic) and stores 16 B. Dword stores only where a chunk is not whole: the
//                       two edges of a span's range in a destination, and at a capacity.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"

namespace gdsm {

namespace {

constexpr uint32_t kTile = kSplitTile;  // records per tile = threads of a workgroup
constexpr uint32_t kSpan = 16384;       // input bytes per work item of the copy
constexpr uint32_t kMaxG = 8;
constexpr uint32_t kScanPer = 4;        // tiles per lane and step of the scan of the tile sums

// The destinations of record i as a mask (bit d = out[d]) and the page id written for it. A mask
// with a bit >= G or a home >= G returns bad (the caller makes it fatal).
struct Dest {
  uint32_t mask;
  uint32_t page;
  bool bad;
};
__device__ __forceinline__ Dest record_dest(const SplitArgs& a, uint64_t i, uint64_t size) {
  Dest r{0u, 0u, false};
  const uint32_t id = a.ids ? a.ids[i] : (uint32_t)i;
  if (a.dest) {
    const uint32_t m = a.dest[i];
    r.bad = (m >> a.G) != 0;
    r.mask = m;
    r.page = id;
  } else {
    const uint64_t d = a.per <= 0xFFFFFFFFull ? (uint64_t)(id / (uint32_t)a.per) : 0ull;
    r.bad = d >= a.G;
    r.mask = 1u << (uint32_t)(d & 7u);
    r.page = id - (uint32_t)(d * a.per);
  }
  if (r.bad || ((a.flags & 1u) && size == 0)) r.mask = 0;
  return r;
}

// ------------------------------------------------------------------------- check
__global__ __launch_bounds__(256) void split_check_kernel(const uint64_t* __restrict__ ro,
                                                          uint64_t n, uint64_t cap,
                                                          uint32_t* __restrict__ fatal,
                                                          uint32_t* __restrict__ err) {
  const uint64_t st = (uint64_t)gridDim.x * blockDim.x;
  uint32_t v = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += st) {
    const uint64_t o = ro[i];
    if ((o & 3u) || (i == 0 && o != 0)) v = 1;
    if (i < n) {
      if (ro[i + 1] < o) v = 1;
    } else if (o > cap) {
      v = 1;
    }
  }
  wave_report(v, [&](uint32_t) {
    atomicOr(fatal, 1u);
    if (err) atomicOr(err, kErrStream);
  });
}

// ------------------------------------------------------------------------- tile sums
// tsum[(2 d) T + t] = the records of tile t that go to d, tsum[(2 d + 1) T + t] = their bytes (T
// tiles; one row per scanned sequence, so the scan's loads and stores are contiguous).
__global__ __launch_bounds__(256) void split_count_kernel(SplitArgs a, uint64_t* __restrict__ tsum,
                                                          uint32_t* __restrict__ fatal,
                                                          uint32_t* __restrict__ err) {
  __shared__ uint64_t wcnt[4][kMaxG], wbytes[4][kMaxG];
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t size = 0;
  Dest ds{0u, 0u, false};
  if (i < a.n) {
    size = a.rec_off[i + 1] - a.rec_off[i];  // (garbage under a fatal check: dropped by the scan)
    ds = record_dest(a, i, size);
  }
  const uint64_t bad = __ballot(ds.bad);
  if (bad && lane == (uint32_t)__builtin_ctzll(bad)) {
    atomicOr(fatal, 1u);
    if (err) atomicOr(err, kErrIds);
  }
  for (uint32_t d = 0; d < a.G; ++d) {
    const bool sel = (ds.mask >> d) & 1u;
    const uint64_t c = (uint64_t)__popcll(__ballot(sel));
    const uint64_t b = lane_bcast64(wave_incl_sum64(sel ? size : 0ull), 63);
    if (lane == 0) {
      wcnt[wave][d] = c;
      wbytes[wave][d] = b;
    }
  }
  __syncthreads();
  if (threadIdx.x < a.G) {
    const uint32_t d = threadIdx.x;
    const uint64_t T = gridDim.x;
    tsum[(2ull * d) * T + blockIdx.x] = wcnt[0][d] + wcnt[1][d] + wcnt[2][d] + wcnt[3][d];
    tsum[(2ull * d + 1) * T + blockIdx.x] = wbytes[0][d] + wbytes[1][d] + wbytes[2][d] + wbytes[3][d];
  }
}

// ------------------------------------------------------------------------- scan
// Wave w = 2 d + which scans row w of tsum over t in place (exclusive); counts[2 d +
// which] = the total (0 under fatal); then rec_off[c_d] = b_d of every output (rec_off[0] = 0
// under fatal), where it is within the record capacity.
__global__ __launch_bounds__(1024) void split_scan_kernel(SplitArgs a, uint64_t* __restrict__ tsum,
                                                          uint64_t T,
                                                          const uint32_t* __restrict__ fatal,
                                                          uint64_t* __restrict__ counts) {
  __shared__ uint64_t tot[2 * kMaxG];
  const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
  const bool dead = *fatal != 0;
  uint64_t carry = 0;
  if (!dead) {
    // a lane takes kScanPer consecutive tiles of its row: a step's loads are issued together, a
    // wave reads 2 KiB in a piece, and a step covers 256 tiles
    uint64_t* const row = tsum + (uint64_t)w * T;
    for (uint64_t b = 0; b < T; b += 64 * kScanPer) {
      const uint64_t t0 = b + (uint64_t)lane * kScanPer;
      uint64_t v[kScanPer], sum = 0;
#pragma unroll
      for (uint32_t j = 0; j < kScanPer; ++j) {
        v[j] = t0 + j < T ? row[t0 + j] : 0;
        sum += v[j];
      }
      const uint64_t inc = wave_incl_sum64(sum);
      uint64_t pre = carry + inc - sum;
#pragma unroll
      for (uint32_t j = 0; j < kScanPer; ++j) {
        if (t0 + j < T) row[t0 + j] = pre;
        pre += v[j];
      }
      carry += lane_bcast64(inc, 63);
    }
  }
  if (lane == 0) {
    tot[w] = carry;
    counts[w] = carry;
  }
  __syncthreads();
  if (threadIdx.x < a.G) {
    const uint32_t d = threadIdx.x;
    const uint64_t c = tot[2 * d], b = tot[2 * d + 1];
    if (c <= a.out_n_cap[d]) a.out_rec_off[d][c] = b;
  }
}

// ------------------------------------------------------------------------- offsets and ids
__global__ __launch_bounds__(256) void split_index_kernel(SplitArgs a,
                                                          const uint64_t* __restrict__ tsum,
                                                          const uint32_t* __restrict__ fatal) {
  __shared__ uint64_t wcnt[4][kMaxG], wbytes[4][kMaxG];
  if (*fatal) return;  // written by an earlier launch: the whole grid reads the same word
  const uint32_t lane = lane_id(), wave = threadIdx.x >> 6;
  const uint64_t i = (uint64_t)blockIdx.x * kTile + threadIdx.x;
  uint64_t size = 0;
  Dest ds{0u, 0u, false};
  if (i < a.n) {
    size = a.rec_off[i + 1] - a.rec_off[i];
    ds = record_dest(a, i, size);
  }
  uint64_t rank[kMaxG], pre[kMaxG];  // inside the wave, exclusive
#pragma unroll
  for (uint32_t d = 0; d < kMaxG; ++d) {
    if (d >= a.G) break;
    const bool sel = (ds.mask >> d) & 1u;
    uint64_t bal;
    rank[d] = ballot_rank(sel, bal);
    const uint64_t v = sel ? size : 0ull;
    const uint64_t inc = wave_incl_sum64(v);
    pre[d] = inc - v;
    if (lane == 63) {
      wcnt[wave][d] = (uint64_t)__popcll(bal);
      wbytes[wave][d] = inc;
    }
  }
  __syncthreads();
#pragma unroll
  for (uint32_t d = 0; d < kMaxG; ++d) {
    if (d >= a.G) break;
    if (!((ds.mask >> d) & 1u)) continue;
    const uint64_t T = gridDim.x;
    uint64_t j = tsum[(2ull * d) * T + blockIdx.x] + rank[d];
    uint64_t off = tsum[(2ull * d + 1) * T + blockIdx.x] + pre[d];
    for (uint32_t q = 0; q < wave; ++q) {
      j += wcnt[q][d];
      off += wbytes[q][d];
    }
    if (j <= a.out_n_cap[d]) a.out_rec_off[d][j] = off;
    if (j < a.out_n_cap[d] && a.out_ids[d]) a.out_ids[d][j] = ds.page;
  }
}

// ------------------------------------------------------------------------- copy
// The last record r <= n - 1 with ro[r] <= x (ro[0] = 0 <= x < ro[n]): the record holding input
// byte x. The wave probes 64 points a step, as find_id of gdsm_merge.hip does for its lower bound
// with an equality test; this is an upper bound over offsets, so the two stay apart.
__device__ __forceinline__ uint64_t find_record(const uint64_t* __restrict__ ro, uint64_t n,
                                                uint64_t x) {
  const uint32_t lane = lane_id();
  uint64_t lo = 0, hi = n;  // ro[lo] <= x, ro[hi] > x
  while (hi - lo > 1) {
    const uint64_t st = (hi - lo + 63) / 64;
    const uint64_t idx = lo + (uint64_t)(lane + 1) * st;
    const bool le = idx < hi && ro[idx] <= x;
    const uint32_t c = (uint32_t)__popcll(__ballot(le));  // probes are monotone: a prefix of lanes
    const uint64_t nlo = lo + (uint64_t)c * st;
    const uint64_t nhi = lo + (uint64_t)(c + 1) * st;
    hi = nhi < hi ? nhi : hi;
    lo = nlo;
  }
  return lo;
}

struct CopyLds {
  uint32_t data[kSpan / 4];     // the staged span
  uint32_t pre[kMaxG][kTile];   // per destination: the batch's bytes before record j (exclusive)
  uint32_t src[kTile];          // where record j's part of the span starts, in data (bytes)
  uint32_t len[kTile];          // the bytes record j has inside the span
  uint64_t wsum[4][kMaxG];
  uint64_t base[kMaxG];         // where the batch's first byte for d lies in out[d]
  uint32_t more;
};

__global__ __launch_bounds__(256) void split_copy_kernel(SplitArgs a,
                                                         const uint64_t* __restrict__ tsum,
                                                         const uint32_t* __restrict__ fatal) {
  __shared__ __attribute__((aligned(16))) CopyLds L;
  if (*fatal) return;
  const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
  const uint64_t total = a.rec_off[a.n];
  const uint64_t T = (a.n + kTile - 1) / kTile;
  const bool src16 = (reinterpret_cast<uintptr_t>(a.data) & 15u) == 0;
  for (uint64_t s0 = (uint64_t)blockIdx.x * kSpan; s0 < total; s0 += (uint64_t)gridDim.x * kSpan) {
    const uint64_t s1 = s0 + kSpan < total ? s0 + kSpan : total;
    // stage the span: 16 B a lane where the whole chunk lies inside the buffer
#pragma unroll
    for (uint32_t q = 0; q < kSpan / 16 / 256; ++q) {
      const uint32_t c = (q * 256 + tid) * 16;
      const uint64_t o = s0 + c;
      if (o >= s1) continue;
      if (src16 && o + 16 <= a.cap) {
        *reinterpret_cast<u32x4*>(&L.data[c / 4]) =
            __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a.data + o));
      } else {
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e)
          if (o + 4 * e < s1)
            L.data[c / 4 + e] = *reinterpret_cast<const uint32_t*>(a.data + o + 4 * e);
      }
    }
    // the span's first record and where its first byte lies in every output
    const uint64_t r0 = find_record(a.rec_off, a.n, s0);
    const uint64_t t0 = r0 / kTile;
    {
      const uint64_t i = t0 * kTile + tid;
      uint64_t sz = 0, full = 0;
      Dest ds{0u, 0u, false};
      if (i <= r0) {
        const uint64_t o0 = a.rec_off[i], o1 = a.rec_off[i + 1];
        full = o1 - o0;
        sz = (o1 < s0 ? o1 : s0) - o0;  // whole records before r0, r0's bytes before the span
        ds = record_dest(a, i, full);
      }
      for (uint32_t d = 0; d < a.G; ++d) {
        const uint64_t b = lane_bcast64(wave_incl_sum64(((ds.mask >> d) & 1u) ? sz : 0ull), 63);
        if (lane == 0) L.wsum[wave][d] = b;
      }
      __syncthreads();
      if (tid < a.G)
        L.base[tid] = tsum[(2ull * tid + 1) * T + t0] + L.wsum[0][tid] + L.wsum[1][tid] +
                      L.wsum[2][tid] + L.wsum[3][tid];
      __syncthreads();
    }
    // the span's records, 256 at a time
    for (uint64_t rb = r0;; rb += kTile) {
      const uint64_t i = rb + tid;
      uint32_t len = 0, src = 0, mask = 0;
      uint64_t o1 = 0;
      if (i < a.n) {
        const uint64_t o0 = a.rec_off[i];
        o1 = a.rec_off[i + 1];
        const uint64_t c0 = o0 < s0 ? s0 : (o0 > s1 ? s1 : o0);
        const uint64_t c1 = o1 < s0 ? s0 : (o1 > s1 ? s1 : o1);
        len = (uint32_t)(c1 - c0);
        src = (uint32_t)(c0 - s0);
        mask = len ? record_dest(a, i, o1 - o0).mask : 0u;
      }
      L.src[tid] = src;
      L.len[tid] = len;
      if (tid == kTile - 1) L.more = (i + 1 < a.n && o1 < s1) ? 1u : 0u;
      uint32_t inc[kMaxG];
#pragma unroll
      for (uint32_t d = 0; d < kMaxG; ++d) {
        if (d >= a.G) break;
        inc[d] = wave_incl_sum(((mask >> d) & 1u) ? len : 0u);
        if (lane == 63) L.wsum[wave][d] = inc[d];
      }
      __syncthreads();
#pragma unroll
      for (uint32_t d = 0; d < kMaxG; ++d) {
        if (d >= a.G) break;
        uint32_t p = inc[d] - (((mask >> d) & 1u) ? len : 0u);
        for (uint32_t q = 0; q < wave; ++q) p += (uint32_t)L.wsum[q][d];
        L.pre[d][tid] = p;
      }
      __syncthreads();
      for (uint32_t d = 0; d < a.G; ++d) {
        const uint32_t tot = (uint32_t)(L.wsum[0][d] + L.wsum[1][d] + L.wsum[2][d] + L.wsum[3][d]);
        if (tot == 0) continue;
        const uint64_t w0 = L.base[d];  // the range [w0, w0 + tot) of out[d]
        uint8_t* const out = a.out_data[d];
        const uint64_t cap = a.out_cap[d];
        const uint32_t ph = (uint32_t)((reinterpret_cast<uintptr_t>(out) + w0) & 15u);
        const uint32_t nch = (ph + tot + 15u) / 16u;
        const uint32_t* const pre = L.pre[d];
        for (uint32_t c = tid; c < nch; c += 256) {
          // chunk c covers the range's bytes [16 c - ph, 16 c - ph + 16)
          uint32_t v[4];
          uint32_t have = 0;
          uint32_t k = 0, kb = 0, ke = 0;  // the record found last: pre[k] = kb, its end ke
          int64_t x0 = (int64_t)16 * c - ph;
#pragma unroll
          for (uint32_t e = 0; e < 4; ++e) {
            const int64_t xs = x0 + 4 * e;
            if (xs < 0 || xs >= (int64_t)tot) continue;
            const uint32_t x = (uint32_t)xs;
            if (x >= ke) {
              uint32_t lo = 0, hi = kTile;  // the last j with pre[j] <= x has the byte
              while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (pre[mid] <= x)
                  lo = mid;
                else
                  hi = mid;
              }
              k = lo;
              kb = pre[k];
              ke = kb + L.len[k];
            }
            v[e] = L.data[(L.src[k] + (x - kb)) >> 2];
            have |= 1u << e;
          }
          const uint64_t p = w0 + x0;  // (meaningful for the dwords in `have` only)
          if (have == 0xFu && p + 16 <= cap) {
            *reinterpret_cast<u32x4*>(out + p) = (u32x4){v[0], v[1], v[2], v[3]};
          } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
              if (((have >> e) & 1u) && p + 4 * e + 4 <= cap)
                *reinterpret_cast<uint32_t*>(out + p + 4 * e) = v[e];
          }
        }
      }
      __syncthreads();
      if (tid < a.G)
        L.base[tid] += L.wsum[0][tid] + L.wsum[1][tid] + L.wsum[2][tid] + L.wsum[3][tid];
      const bool more = L.more != 0;
      __syncthreads();
      if (!more) break;
    }
  }
}

}  // namespace

// Workspace: the header (kSplitHeader bytes: the fatal word; the rest is the caller's, the context
// keeps its private error word and the counts there) and the tile sums, 16 B per tile and
// destination.
uint64_t split_workspace_bytes(uint64_t n, uint32_t G) {
  const uint64_t T = (n + kTile - 1) / kTile;
  return kSplitHeader + 16ull * G * T;
}

hipError_t launch_runs_split(const SplitArgs& a, uint64_t* counts, uint32_t* err, uint8_t* ws,
                             uint64_t ws_bytes, hipStream_t s) {
  if (a.G == 0 || a.G > kMaxG || a.n > (1ull << 32) || ws_bytes < split_workspace_bytes(a.n, a.G))
    return hipErrorInvalidValue;
  uint32_t* fatal = reinterpret_cast<uint32_t*>(ws);
  uint64_t* tsum = reinterpret_cast<uint64_t*>(ws + kSplitHeader);
  const uint64_t T = (a.n + kTile - 1) / kTile;
  hipError_t e = hipMemsetAsync(ws, 0, 4, s);
  if (e != hipSuccess) return e;
  const uint64_t cb = (a.n + 1 + 255) / 256;
  hipLaunchKernelGGL(split_check_kernel, dim3((unsigned)(cb < 4096 ? cb : 4096)), dim3(256), 0, s,
                     a.rec_off, a.n, a.cap, fatal, err);
  if (T) hipLaunchKernelGGL(split_count_kernel, dim3((unsigned)T), dim3(256), 0, s, a, tsum, fatal, err);
  hipLaunchKernelGGL(split_scan_kernel, dim3(1), dim3(128 * a.G), 0, s, a, tsum, T, fatal, counts);
  if (T) {
    hipLaunchKernelGGL(split_index_kernel, dim3((unsigned)T), dim3(256), 0, s, a, tsum, fatal);
    const uint64_t spans = (a.cap + kSpan - 1) / kSpan;
    if (spans)
      hipLaunchKernelGGL(split_copy_kernel, dim3((unsigned)(spans < 2048 ? spans : 2048)),
                         dim3(256), 0, s, a, tsum, fatal);
  }
  return hipGetLastError();
}

}  // namespace gdsm
