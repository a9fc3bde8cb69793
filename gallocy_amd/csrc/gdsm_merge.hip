// gdsm_merge for gfx950 (docs/SPEC.md §8): K diff streams of several writers, in priority order
// and joined by page id, composed into one canonical stream, with the bytes where the inputs
// overlapped and where they disagreed counted.
//
// The multiple-writer step of a twin/diff DSM at the home (resources/NUTSHELL.md:59-69 describes
// the single-writer flow only; the reference has no counterpart): the writers' diffs of one
// interval become one stream to apply, forward or log, and a byte two writers wrote is reported.
//
// Five launches (six with the totals) on one stream, no wave ever waits for another:
//   merge_check_kernel  every input's offsets (from 0, non-decreasing, 4-aligned, inside its
//                       capacity) and every page list (strictly ascending), before any record is
//                       dereferenced; a failure sets the `fatal` word, which empties the output
//   merge_size_kernel   a wave per out page: the union of the streams' coverage from their
//                       HEADERS alone (payloads are not read) -> the out record's size
//   merge_scan_kernels  exclusive scan of the sizes (4096-page tiles, then the tile sums)
//   merge_emit_kernel   a wave per out page: lane k locates stream k's record, the records are
//                       staged in LDS together (LDS-DMA, 16 B a lane, one wait), each payload is
//                       laid into a 4 KiB LDS page image in priority order (compared with what is
//                       there first, where coverage exists: the conflict bits), then the out
//                       record is assembled in LDS and stored once, 16 B a lane
//   merge_stats_kernel  the totals from the per-page counts the emit launch left
// Lane l of a page's wave owns byte positions [64 l, 64 l + 64): coverage and overlap masks are one
// uint64_t per lane each. The byte-moving passes run over the covered dwords as work items spread
// over all lanes (publish_blocks), not over each lane's own positions.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"
#include "gdsm_record.h"

namespace gdsm {

namespace {

// Largest record gdsm_apply accepts: 2048 abutting runs covering the whole page (not canonical).
constexpr uint32_t kMergeMaxIn = 4u + 4u * kMaxRuns + kPage;
// Staging / out-record buffer of a wave: the largest input at any position inside its first 16-B
// line, and one line of slack (a payload dword read at the record's end stays inside the buffer).
constexpr uint32_t kMergeBufWords = (kMergeMaxIn + 12u + 15u) / 16u * 4u + 4u;
constexpr uint32_t kTile = 4096;  // out pages per scan tile

struct WaveLds {
  uint32_t img[kPage / 4];    // the page image
  uint32_t buf[kMergeBufWords];
  uint64_t sbits[64], ebits[64];  // run starts / last positions of the record being read
  // the work items of a lay / gather pass (publish_blocks): per 64-position block its coverage,
  // the coverage accumulated before this stream, the payload offset of its first covered byte,
  // and the list of covered blocks; cnf: the conflict bits of the page (64 x 2 dwords)
  uint64_t cmask[64], amask[64];
  uint32_t cpre[64], list[64], cnf[128];
};

// Byte mask of a 4-bit byte-enable nibble.
__device__ __forceinline__ uint32_t nib_mask(uint32_t nib) {
  return ((nib * 0x00204081u) & 0x01010101u) * 0xFFu;
}
// Bit j set iff byte j of x is non-zero.
__device__ __forceinline__ uint32_t nz4(uint32_t x) {
  const uint32_t y = ((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u) >> 7;
  return ((y * 0x00204081u) >> 21) & 0xFu;
}

__device__ __forceinline__ uint32_t popc64(uint64_t v) { return (uint32_t)__popcll(v); }

// Bit 63 of the previous lane's mask (lane 0: 0) / bit 0 of the next lane's (lane 63: 0).
__device__ __forceinline__ uint64_t prev_top(uint64_t m) {
  return (uint64_t)from_prev_lane((uint32_t)(m >> 63));
}
__device__ __forceinline__ uint64_t next_low(uint64_t m) {
  return (uint64_t)from_next_lane((uint32_t)(m & 1u));
}

// Where out page p's record sits in a stream with the page list ids[0..n) (ascending): the index,
// or n when the stream has no such page. The wave probes 64 points a step (4 steps for 16 M ids).
__device__ __forceinline__ uint64_t find_id(const uint32_t* __restrict__ ids, uint64_t n,
                                            uint32_t p) {
  const uint32_t lane = lane_id();
  uint64_t lo = 0, hi = n;  // the first index with ids[idx] >= p lies in [lo, hi]
  while (hi > lo) {
    const uint64_t st = (hi - lo + 63) / 64;
    const uint64_t idx = lo + (uint64_t)lane * st;
    const bool lt = idx < hi && ids[idx] < p;
    const uint32_t c = popc64(__ballot(lt));
    if (c == 0) {
      hi = lo;
      break;
    }
    const uint64_t nlo = lo + (uint64_t)(c - 1) * st + 1;
    hi = min(lo + (uint64_t)c * st, hi);
    lo = nlo;
  }
  return (lo < n && ids[lo] == p) ? lo : n;
}

// Out entry i's record in stream k: rec (NULL: none) and its size. A record whose offsets are
// unusable (the check kernel has then flagged the stream) or larger than any record gdsm_apply
// accepts counts as malformed: `bad`, nothing of it is read.
struct Located {
  const uint8_t* rec;
  uint32_t size;
  bool bad;
};
__device__ __forceinline__ Located locate(const MergeIn& in, uint32_t k, const uint32_t* out_ids,
                                          uint64_t n_out, uint64_t i, uint32_t page) {
  Located L{nullptr, 0u, false};
  const uint32_t* ids = in.ids[k];
  const uint64_t n = in.n[k];
  uint64_t r = i;
  if (ids && !(ids == out_ids && n == n_out)) r = find_id(ids, n, page);
  if (r >= n) return L;
  const uint64_t o0 = in.rec_off[k][r], o1 = in.rec_off[k][r + 1];
  if (o1 == o0) return L;
  if (o1 < o0 || ((o0 | o1) & 3u) || o1 > in.cap[k] || o1 - o0 > kMergeMaxIn) {
    L.bad = true;
    return L;
  }
  L.rec = in.data[k] + o0;
  L.size = (uint32_t)(o1 - o0);
  return L;
}

// This lane's 64 positions of a validated record's coverage (nr runs, headers at rec32[1..]): a
// lane per run ORs the run's first and last position into two LDS bitmaps; the coverage is then
// the running parity of the toggles "a run starts here" ^ "a run ended just before here".
template <typename P32>
__device__ __forceinline__ uint64_t record_cov(P32 rec32, uint32_t nr, uint64_t* sbits,
                                               uint64_t* ebits) {
  const uint32_t lane = lane_id();
  sbits[lane] = 0;
  ebits[lane] = 0;
  wave_lds_sync();
  uint32_t* s32 = reinterpret_cast<uint32_t*>(sbits);
  uint32_t* e32 = reinterpret_cast<uint32_t*>(ebits);
  for (uint32_t r = lane; r < nr; r += 64) {
    const uint32_t h = rec32[1 + r];
    const uint32_t off = h & 0xFFFFu, last = off + (h >> 16) - 1u;  // validated: both < 4096
    atomicOr(&s32[off >> 5], 1u << (off & 31u));
    atomicOr(&e32[last >> 5], 1u << (last & 31u));
  }
  wave_lds_sync();
  const uint64_t s = sbits[lane], e = ebits[lane];
  uint64_t t = s ^ ((e << 1) | prev_top(e));
  const uint32_t tinc = wave_incl_sum(popc64(t));
  const bool carry = ((tinc - popc64(t)) & 1u) != 0;  // covered on entering this lane
  t ^= t << 1;
  t ^= t << 2;
  t ^= t << 4;
  t ^= t << 8;
  t ^= t << 16;
  t ^= t << 32;
  wave_lds_sync();  // (the bitmaps are reused by the next record)
  return carry ? ~t : t;
}

// Run count and record size of a page's coverage.
__device__ __forceinline__ uint32_t cov_size(uint64_t cov, uint32_t& nruns, uint32_t& paybytes) {
  const uint64_t starts = cov & ~((cov << 1) | prev_top(cov));
  nruns = wave_sum(popc64(starts));
  paybytes = wave_sum(popc64(cov));
  return nruns ? 4u + 4u * nruns + ((paybytes + 3u) & ~3u) : 0u;
}

// ------------------------------------------------------------------------- check
__global__ __launch_bounds__(256) void merge_check_kernel(MergeIn in, const uint32_t* out_ids,
                                                          uint64_t n_out,
                                                          uint32_t* __restrict__ fatal,
                                                          uint32_t* __restrict__ err) {
  const uint64_t st = (uint64_t)gridDim.x * blockDim.x;
  const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t v = 0;
  for (uint32_t k = 0; k < in.K; ++k) {
    const uint64_t* ro = in.rec_off[k];
    const uint32_t* ids = in.ids[k];
    const uint64_t n = in.n[k];
    for (uint64_t i = t0; i <= n; i += st) {
      const uint64_t o = ro[i];
      if ((o & 3u) || (i == 0 && o != 0)) v |= kErrStream;
      if (i < n) {
        if (ro[i + 1] < o) v |= kErrStream;
        if (ids && i + 1 < n && ids[i + 1] <= ids[i]) v |= kErrIds;
      } else if (o > in.cap[k]) {
        v |= kErrStream;
      }
    }
  }
  if (out_ids)
    for (uint64_t i = t0; i + 1 < n_out; i += st)
      if (out_ids[i + 1] <= out_ids[i]) v |= kErrIds;
  wave_report(v, [&](uint32_t w) {
    atomicOr(fatal, 1u);
    if (err) atomicOr(err, w);
  });
}

// ------------------------------------------------------------------------- sizes
__global__ __launch_bounds__(256) void merge_size_kernel(MergeIn in, const uint32_t* out_ids,
                                                         uint64_t n_out,
                                                         const uint32_t* __restrict__ fatal,
                                                         uint32_t* __restrict__ sizes,
                                                         uint32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) uint64_t bits_all[4][2][64];
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t i = (uint64_t)blockIdx.x * 4 + wv;
  if (i >= n_out) return;
  if (*fatal) {  // written by the previous launch: every wave reads the same word
    if (lane == 0) sizes[i] = 0;
    return;
  }
  const uint32_t page = out_ids ? out_ids[i] : (uint32_t)i;
  uint64_t cov = 0;
  bool any_bad = false;
  for (uint32_t k = 0; k < in.K; ++k) {
    const Located L = locate(in, k, out_ids, n_out, i, page);
    any_bad |= L.bad;
    if (!L.rec) continue;
    const uint32_t* rec32 = reinterpret_cast<const uint32_t*>(L.rec);
    uint32_t nr;
    if (record_check<64>(rec32, L.size, true, nr)) {
      any_bad = true;
      continue;
    }
    cov |= record_cov(rec32, nr, bits_all[wv][0], bits_all[wv][1]);
  }
  uint32_t nruns, pay;
  const uint32_t size = cov_size(cov, nruns, pay);
  if (lane == 0) {
    sizes[i] = size;
    if (any_bad && err) atomicOr(err, kErrRecord);
  }
}

// ------------------------------------------------------------------------- scan
// Tile t: local[i] = the exclusive prefix of sizes inside the tile, tsum[t] = the tile's total.
__global__ __launch_bounds__(256) void merge_scan_tile_kernel(const uint32_t* __restrict__ sizes,
                                                              uint64_t n_out,
                                                              uint32_t* __restrict__ local,
                                                              uint64_t* __restrict__ tsum) {
  __shared__ uint32_t wsum[4];
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t base = (uint64_t)blockIdx.x * kTile + (uint64_t)threadIdx.x * 16;
  uint32_t v[16], t = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    v[j] = base + j < n_out ? sizes[base + j] : 0u;
    t += v[j];
  }
  const uint32_t inc = wave_incl_sum(t);
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t pre = inc - t;
  for (uint32_t q = 0; q < wv; ++q) pre += wsum[q];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (base + j < n_out) local[base + j] = pre;
    pre += v[j];
  }
  if (threadIdx.x == 255) tsum[blockIdx.x] = pre;
}

// One wave: tsum[0..nt) := its exclusive prefix, tsum[nt] := the total.
__global__ __launch_bounds__(64) void merge_scan_top_kernel(uint64_t* __restrict__ tsum,
                                                            uint64_t nt) {
  const uint32_t lane = lane_id();
  uint64_t carry = 0;
  for (uint64_t b = 0; b < nt; b += 64) {
    const uint64_t x = b + lane < nt ? tsum[b + lane] : 0;
    const uint64_t inc = wave_incl_sum64(x);
    if (b + lane < nt) tsum[b + lane] = carry + inc - x;
    carry += shfl64(inc, 63);
  }
  if (lane == 0) tsum[nt] = carry;
}

// ------------------------------------------------------------------------- emit
// 16-B coalesced store of the wave's LDS record (words) to data + off, every store below cap.
__device__ __forceinline__ void store_record(const uint32_t* __restrict__ buf, uint32_t words,
                                             uint8_t* __restrict__ data, uint64_t off,
                                             uint64_t cap) {
  const uint32_t lane = lane_id();
  // head: the dwords before the first 16-B boundary of the destination
  const uint32_t head = min(words, (uint32_t)((16u - (off & 15u)) & 15u) >> 2);
  if (lane < head && off + 4ull * lane + 4 <= cap)
    *reinterpret_cast<uint32_t*>(data + off + 4ull * lane) = buf[lane];
  const uint32_t n16 = (words - head) >> 2;
  for (uint32_t q = lane; q < n16; q += 64) {
    const uint32_t j = head + 4 * q;
    const uint64_t o = off + 4ull * j;
    if (o + 16 <= cap) {
      *reinterpret_cast<u32x4*>(data + o) = (u32x4){buf[j], buf[j + 1], buf[j + 2], buf[j + 3]};
    } else {
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e)
        if (o + 4ull * e + 4 <= cap) *reinterpret_cast<uint32_t*>(data + o + 4ull * e) = buf[j + e];
    }
  }
  const uint32_t j = head + 4 * n16 + lane;
  if (j < words && off + 4ull * j + 4 <= cap)
    *reinterpret_cast<uint32_t*>(data + off + 4ull * j) = buf[j];
}

// The blocks (64 positions = 16 dwords each, block b = lane b's positions) that `mask` covers, as
// work items of one dword each, spread evenly over the lanes whatever the coverage looks like (a
// 64-B cluster is one lane's whole block: lane-owned loops left 58 lanes idle on it). Publishes
// each lane's mask, the payload byte offset of its first covered byte and the list of covered
// blocks; returns the item count (16 per covered block).
__device__ __forceinline__ uint32_t publish_blocks(WaveLds& w, uint64_t mask, uint32_t pay_base) {
  const uint32_t lane = lane_id();
  const uint64_t m = __ballot(mask != 0);
  const uint32_t c = popc64(mask);
  w.cmask[lane] = mask;
  w.cpre[lane] = pay_base + wave_incl_sum(c) - c;
  if (mask) w.list[popc64(m & ((1ull << lane) - 1ull))] = lane;
  return 16u * popc64(m);
}

__global__ __launch_bounds__(256) void merge_emit_kernel(
    MergeIn in, const uint32_t* out_ids, uint64_t n_out, const uint32_t* __restrict__ fatal,
    uint32_t* sizes, uint32_t* local, const uint64_t* __restrict__ tsum, uint64_t* __restrict__ out_rec_off,
    uint8_t* __restrict__ out_data, uint64_t out_cap, uint32_t* __restrict__ conflicts,
    uint64_t* __restrict__ stats, uint32_t* __restrict__ err) {
  __shared__ __attribute__((aligned(16))) WaveLds lds[4];
  const uint32_t wv = threadIdx.x >> 6, lane = lane_id();
  const uint64_t i = (uint64_t)blockIdx.x * 4 + wv;
  if (i >= n_out) return;
  const uint32_t want = sizes[i];
  const uint64_t off = tsum[i / kTile] + local[i];
  if (lane == 0) {
    out_rec_off[i] = off;
    if (i + 1 == n_out) out_rec_off[n_out] = off + want;
  }
  if (*fatal) {  // (every size is 0: the offsets above are all zero)
    if (lane == 0 && conflicts) conflicts[i] = 0;
    return;
  }
  WaveLds& w = lds[wv];
  const uint32_t page = out_ids ? out_ids[i] : (uint32_t)i;
  // ---- every stream's pair of offsets is loaded before any is used (one round trip for the K
  // streams; a stream with a page list of its own is searched by the whole wave first); lane k
  // then holds stream k's record
  uint64_t o0[8], o1[8];
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    o0[k] = o1[k] = 0;
    if (k < in.K) {
      const uint32_t* ids = in.ids[k];
      uint64_t r = i;
      if (ids && !(ids == out_ids && in.n[k] == n_out)) r = find_id(ids, in.n[k], page);
      if (r < in.n[k]) {
        o0[k] = in.rec_off[k][r];
        o1[k] = in.rec_off[k][r + 1];
      }
    }
  }
  uint64_t my_rec = 0;
  uint32_t my_size = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8; ++k) {
    // (unusable offsets or an over-long record: malformed, flagged by the size launch)
    if (k < in.K && lane == k && o1[k] > o0[k] && !((o0[k] | o1[k]) & 3u) &&
        o1[k] <= in.cap[k] && o1[k] - o0[k] <= kMergeMaxIn) {
      my_rec = reinterpret_cast<uint64_t>(in.data[k] + o0[k]);
      my_size = (uint32_t)(o1[k] - o0[k]);
    }
  }
  w.cnf[lane] = 0;
  w.cnf[lane + 64] = 0;
  uint64_t cov = 0, ovl = 0;
  uint32_t k = 0;
  while (k < in.K) {
    // ---- the next records that fit the staging buffer together -> LDS, 16 B a lane by LDS-DMA,
    // every load of the group in flight at once
    uint32_t ke = k, used = 0;
    // (the previous group's LDS reads are done before the DMA may overwrite the buffer)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    while (ke < in.K) {
      const uint32_t size = lane_bcast(my_size, (int)ke);
      const uint64_t rec = lane_bcast64(my_rec, (int)ke);
      // the record keeps its position inside a 16-B line: its slot starts on a line and the
      // record (rec & 15) bytes into it, so every 16-B piece is aligned on both sides; the dwords
      // before the first and after the last whole line go singly (nothing outside the record is
      // read)
      const uint32_t lead = (uint32_t)rec & 15u;
      const uint32_t slot = (lead + size + 15u) & ~15u;
      if (used + slot > 4u * (kMergeBufWords - 4u)) break;  // (one record always fits)
      if (size) {
        typedef __attribute__((address_space(1))) void* gptr;
        typedef __attribute__((address_space(3))) void* lptr;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(rec);
        uint32_t* dst = w.buf + (used + lead) / 4;
        const uint32_t words = size >> 2;
        const uint32_t head = min(words, ((16u - lead) & 15u) >> 2), n16 = (words - head) >> 2;
        if (lane < head) __builtin_amdgcn_global_load_lds((gptr)(src + lane), (lptr)dst, 4, 0, 0);
        for (uint32_t q0 = 0; q0 < 4 * n16; q0 += 256) {
          const uint32_t q = q0 / 4 + lane;
          if (q < n16)
            __builtin_amdgcn_global_load_lds((gptr)(src + head + 4 * q), (lptr)(dst + head + q0),
                                             16, 0, 0);
        }
        const uint32_t qt = head + 4 * n16 + lane;
        if (qt < words)
          __builtin_amdgcn_global_load_lds((gptr)(src + qt), (lptr)(dst + head + 4 * n16), 4, 0, 0);
      }
      used += slot;
      ++ke;
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the group has landed
    wave_lds_sync();
    uint32_t base = 0;
    for (; k < ke; ++k) {
      const uint32_t size = lane_bcast(my_size, (int)k);
      if (!size) continue;
      const uint32_t lead = (uint32_t)lane_bcast64(my_rec, (int)k) & 15u;
      const uint32_t* rec32 = w.buf + (base + lead) / 4;
      base += (lead + size + 15u) & ~15u;
      uint32_t nr;
      if (record_check<64>(rec32, size, true, nr)) continue;  // contributes nothing
      const uint64_t ck = record_cov(rec32, nr, w.sbits, w.ebits);
      if (!__ballot(ck != 0)) continue;
      const bool have_prev = __ballot(cov != 0) != 0;  // (never with K = 1: no compare path)
      ovl |= ck & cov;
      w.amask[lane] = cov;
      // the payload is the covered bytes in position order
      const uint32_t items = publish_blocks(w, ck, 4u + 4u * nr);
      wave_lds_sync();
      for (uint32_t j = lane; j < items; j += 64) {
        const uint32_t blk = w.list[j >> 4], wd = j & 15u;
        const uint64_t mk = w.cmask[blk];
        const uint32_t nib = (uint32_t)(mk >> (4 * wd)) & 0xFu;
        if (!nib) continue;
        const uint32_t q = w.cpre[blk] + popc64(mk & ((1ull << (4 * wd)) - 1ull));
        // the next 4 payload bytes (two aligned dwords and a funnel shift), spread to nib's bytes
        const uint32_t sh = (q & 3u) * 8u;
        uint32_t src = rec32[q >> 2];
        if (sh) src = __builtin_amdgcn_alignbit(rec32[(q >> 2) + 1], src, sh);
        uint32_t val = src;
        if (nib != 0xFu) {
          val = 0;
#pragma unroll
          for (uint32_t b = 0; b < 4; ++b)
            if ((nib >> b) & 1u) {
              val |= (src & 0xFFu) << (8 * b);
              src >>= 8;
            }
        }
        const uint32_t at = 16u * blk + wd;
        if (have_prev) {
          const uint32_t pn = (uint32_t)(w.amask[blk] >> (4 * wd)) & nib;
          const uint32_t old = w.img[at];
          const uint32_t c = nz4(old ^ val) & pn;
          if (c) atomicOr(&w.cnf[2 * blk + (wd >> 3)], c << ((4 * wd) & 31u));
          const uint32_t m8 = nib_mask(nib);
          val = (old & ~m8) | (val & m8);
        }
        w.img[at] = val;
      }
      cov |= ck;
      wave_lds_sync();  // (the bitmaps and the block list are reused by the next record)
    }
  }
  // conflicts are counted where any two covering streams disagree: a byte once in conflict stays
  // so even when a later stream restores agreement with the newest value
  wave_lds_sync();
  const uint64_t cnf = (uint64_t)w.cnf[2 * lane] | ((uint64_t)w.cnf[2 * lane + 1] << 32);
  const uint32_t n_ovl = wave_sum(popc64(ovl)), n_cnf = wave_sum(popc64(cnf));
  if (lane == 0) {
    if (conflicts) conflicts[i] = n_cnf;
    // the page's counts take the place of its size and offset, which only this wave read; the
    // stats launch sums them (an atomic add per wave on the two totals serialised in one L2
    // line: 7.5 of 12.9 ms at 1 M pages)
    if (stats) {
      sizes[i] = n_ovl;
      local[i] = n_cnf;
    }
  }
  uint32_t nruns, paybytes;
  const uint32_t size = cov_size(cov, nruns, paybytes);
  if (size != want) {  // the inputs changed between the launches: nothing is written
    if (lane == 0 && err) atomicOr(err, kErrRecord);
    return;
  }
  if (size == 0) return;
  // ---- the out record in LDS: count, headers, payload
  const uint64_t starts = cov & ~((cov << 1) | prev_top(cov));
  const uint64_t ends = cov & ~((cov >> 1) | (next_low(cov) << 63));
  if (lane == 0) w.buf[0] = nruns;
  {
    uint64_t s = starts;
    uint32_t rr = wave_incl_sum(popc64(starts)) - popc64(starts);
    while (s) {
      w.buf[1 + rr++] = 64u * lane + (uint32_t)__builtin_ctzll(s);
      s &= s - 1;
    }
  }
  for (uint32_t j = 1 + nruns + lane; j < size / 4; j += 64) w.buf[j] = 0;
  const uint32_t items = publish_blocks(w, cov, 4u + 4u * nruns);
  wave_lds_sync();
  {
    uint64_t e = ends;  // the r-th end closes the r-th start
    uint32_t rr = wave_incl_sum(popc64(ends)) - popc64(ends);
    while (e) {
      const uint32_t last = 64u * lane + (uint32_t)__builtin_ctzll(e);
      const uint32_t o = w.buf[1 + rr];
      w.buf[1 + rr] = o | ((last + 1u - o) << 16);
      ++rr;
      e &= e - 1;
    }
  }
  for (uint32_t j = lane; j < items; j += 64) {
    const uint32_t blk = w.list[j >> 4], wd = j & 15u;
    const uint64_t mk = w.cmask[blk];
    const uint32_t nib = (uint32_t)(mk >> (4 * wd)) & 0xFu;
    if (!nib) continue;
    const uint32_t q = w.cpre[blk] + popc64(mk & ((1ull << (4 * wd)) - 1ull));
    const uint32_t src = w.img[16u * blk + wd];
    uint32_t c = src;
    if (nib != 0xFu) {
      uint32_t cnt = 0;
      c = 0;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b)
        if ((nib >> b) & 1u) c |= ((src >> (8 * b)) & 0xFFu) << (8 * cnt++);
    }
    // the bytes land at byte offset q of the zeroed payload: an OR per dword touched (items share
    // the dwords at their edges)
    const uint64_t v = (uint64_t)c << ((q & 3u) * 8u);
    if ((uint32_t)v) atomicOr(&w.buf[q >> 2], (uint32_t)v);
    if ((uint32_t)(v >> 32)) atomicOr(&w.buf[(q >> 2) + 1], (uint32_t)(v >> 32));
  }
  wave_lds_sync();
  store_record(w.buf, size / 4, out_data, off, out_cap);
}

// stats += the sums of the per-page counts the emit launch left: a tile per workgroup, one atomic
// add per wave and total.
__global__ __launch_bounds__(256) void merge_stats_kernel(const uint32_t* __restrict__ ovl,
                                                          const uint32_t* __restrict__ cnf,
                                                          uint64_t n_out,
                                                          uint64_t* __restrict__ stats) {
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  uint32_t a = 0, b = 0;  // (a tile's sums stay below 2^32: 4096 pages x 4096 bytes)
  for (uint32_t j = threadIdx.x; j < kTile && base + j < n_out; j += 256) {
    a += ovl[base + j];
    b += cnf[base + j];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane_id() == 0) {
    if (a) atomicAdd(reinterpret_cast<unsigned long long*>(stats), (unsigned long long)a);
    if (b) atomicAdd(reinterpret_cast<unsigned long long*>(stats) + 1, (unsigned long long)b);
  }
}

inline uint64_t up256(uint64_t v) { return (v + 255) & ~255ull; }
inline uint64_t n_tiles(uint64_t n_out) { return (n_out + kTile - 1) / kTile; }

}  // namespace

// [0, 256): the fatal word | sizes u32[n_out] | local u32[n_out] | tile sums u64[tiles + 1]
uint64_t merge_workspace_bytes(uint64_t n_out) {
  return 256 + 2 * up256(4 * n_out) + up256(8 * (n_tiles(n_out) + 1));
}

hipError_t launch_merge(const MergeIn& in, const uint32_t* out_ids, uint64_t n_out,
                        uint64_t* out_rec_off, uint8_t* out_data, uint64_t out_cap,
                        uint32_t* conflicts, uint64_t* stats, uint32_t* err, uint8_t* ws,
                        uint64_t ws_bytes, hipStream_t s, Prof* prof) {
  if (ws_bytes < merge_workspace_bytes(n_out)) return hipErrorInvalidValue;
  ProfScope ps(prof, GDSM_PROF_MERGE, s);
  hipError_t e;
  if (stats && (e = hipMemsetAsync(stats, 0, 16, s)) != hipSuccess) return e;
  if (n_out == 0) return hipMemsetAsync(out_rec_off, 0, 8, s);
  uint32_t* fatal = reinterpret_cast<uint32_t*>(ws);
  uint32_t* sizes = reinterpret_cast<uint32_t*>(ws + 256);
  uint32_t* local = reinterpret_cast<uint32_t*>(ws + 256 + up256(4 * n_out));
  uint64_t* tsum = reinterpret_cast<uint64_t*>(ws + 256 + 2 * up256(4 * n_out));
  if ((e = hipMemsetAsync(fatal, 0, 256, s)) != hipSuccess) return e;
  uint64_t longest = n_out;
  for (uint32_t k = 0; k < in.K; ++k) longest = longest > in.n[k] + 1 ? longest : in.n[k] + 1;
  const unsigned cgrid = (unsigned)(longest / 256 + 1 < 4096 ? longest / 256 + 1 : 4096);
  const unsigned pgrid = (unsigned)((n_out + 3) / 4);
  hipLaunchKernelGGL(merge_check_kernel, dim3(cgrid), dim3(256), 0, s, in, out_ids, n_out, fatal,
                     err);
  hipLaunchKernelGGL(merge_size_kernel, dim3(pgrid), dim3(256), 0, s, in, out_ids, n_out, fatal,
                     sizes, err);
  hipLaunchKernelGGL(merge_scan_tile_kernel, dim3((unsigned)n_tiles(n_out)), dim3(256), 0, s, sizes,
                     n_out, local, tsum);
  hipLaunchKernelGGL(merge_scan_top_kernel, dim3(1), dim3(64), 0, s, tsum, n_tiles(n_out));
  hipLaunchKernelGGL(merge_emit_kernel, dim3(pgrid), dim3(256), 0, s, in, out_ids, n_out, fatal,
                     sizes, local, tsum, out_rec_off, out_data, out_cap, conflicts, stats, err);
  if (stats)
    hipLaunchKernelGGL(merge_stats_kernel, dim3((unsigned)n_tiles(n_out)), dim3(256), 0, s, sizes,
                       local, n_out, stats);
  return hipGetLastError();
}

}  // namespace gdsm
