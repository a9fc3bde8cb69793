// Page-table sweeps (SPEC §14): gdsm_coh_retire takes a node out of every copyset and hands the
// pages it owned to their heirs; gdsm_coh_select lists the pages whose word matches (mask, value).
// One bandwidth-bound pass over table pages [first, first + n) with an ordered compaction, in the
// shape of the dirty scan (gdsm_dirty.hip).
//
// Three launches on the stream, ordered by their boundaries alone (no workgroup ever waits for
// another):
//   1. sweep_flag_kernel: the only one that touches the table. Positions are counted from the even
//      page a0 = first & ~1, so that the two table words of a lane are one aligned 16-B load. A
//      workgroup takes a tile of 2048 positions, each of its 4 waves 512 of them in 4 steps of 128,
//      every load of a wave issued before the first is used. A wave whose 512 positions lie inside
//      the range (the body) loads 16 B per lane; the waves at the two ends of the range take their
//      words singly, each guarded by the range. One ballot per 64 positions gives the flag words,
//      a pair per step: the step's even positions, then its odd ones (bit l = lane l's), as the
//      lanes hold them. retire: a `moved` and an `orphan` pair, and the state halves that change
//      are stored back (4-B stores: the faults half of a table word is never written; nothing is
//      stored in the dry form). select: one pair. The workgroup also writes the tile's counts.
//   2. sweep_sum_kernel: one workgroup; exclusive scan of the tiles' counts, 16 tiles per thread
//      and step, the totals into stats / count.
//   3. sweep_emit_kernel: a workgroup per tile, a wave per 4 pairs of flag words, lane l = the
//      pair's positions 2 l and 2 l + 1; a page's rank is the tile's offset, the set bits of the
//      tile's earlier pairs and the set bits of its own pair below it in page order.
// Flags, counts and offsets are 532 B per tile, next to the 16 KiB of table the tile reads.
#include "gdsm_common.h"
#include "gdsm_launch.h"
#include "gdsm_list.h"

namespace gdsm {

namespace {

constexpr uint32_t kStep = 128;                 // positions of a wave's step: two per lane
constexpr uint32_t kSteps = 4;                  // steps of a wave
constexpr uint32_t kWave = kStep * kSteps;      // positions per wave
constexpr uint32_t kTile = 4 * kWave;           // positions per workgroup
constexpr uint32_t kTileWords = kTile / 64;     // flag words per tile
constexpr uint32_t kWaveWords = kWave / 64;     // flag words per wave
static_assert(kWaveWords <= 64 && kTileWords <= 64, "a lane per flag word");

// What a sweep does with one state word (SPEC §14).
struct Retire {
  uint32_t x, heir, n_nodes, per;  // per: min(per, 2^32 - 1), the same homes for pages < 2^28
  uint64_t base;
  uint32_t dry;
};
struct Select {
  uint32_t mask, value;
};

// retire(x) of the word w of table page `page` (base not yet added): the new word; moved, orphan
// and held as §14 counts them.
__device__ __forceinline__ uint32_t retire_word(const Retire& r, uint32_t w, uint64_t page,
                                                bool& moved, bool& orphan, bool& held) {
  // no branch on the word: every lane computes both outcomes and selects
  const uint32_t c = w & 0xFFu, o = (w >> 8) & 0xFFu, s = (w >> 16) & 3u;
  const bool live = s != 0;
  const uint32_t c1 = c & ~(1u << r.x);
  held = live && c != c1;
  moved = live && o == r.x;
  uint32_t h = r.heir;
  if (r.per) {  // wave-uniform
    h = (uint32_t)(r.base + page) / r.per;  // base + page < 2^28
    h = (h >= r.n_nodes || h == r.x) ? r.heir : h;
  }
  const uint32_t c2 = c1 | (1u << h);
  const uint32_t s2 = c2 == (1u << h) ? 2u : 1u;
  orphan = moved && s == 2 && ((w >> 18) & 1u);
  const uint32_t gone = (w & ~0x3FFFFu) | c2 | (h << 8) | (s2 << 16);
  const uint32_t kept = (w & ~0xFFu) | c1;
  return live ? (moved ? gone : kept) : w;
}

}  // namespace

// Workspace of a sweep of n pages, NT = ceil((n + 1) / 2048) tiles (+ 1: the position before an
// odd `first`), NTp = NT rounded up to 16: ca[NTp], cb[NTp], ch[NTp] (u32 per tile: the set bits
// of its fa and fb words, retire's held pages), off[NT] (u64: flagged pages before the tile),
// fa[32 NT] and fb[32 NT] (u64 flag words; fb: retire's orphans). 16-byte aligned.
constexpr uint64_t kGroup = 16;  // tiles a thread of the sum kernel takes per step
inline uint64_t padded_tiles(uint64_t NT) { return (NT + kGroup - 1) / kGroup * kGroup; }
uint64_t sweep_workspace_bytes(uint64_t n) {
  const uint64_t NT = (n + 1 + kTile - 1) / kTile;
  return 12 * padded_tiles(NT) + NT * (8 + 16 * kTileWords) + 64;
}

// ------------------------------------------------------------------------- flags and counts
// Position q is table page a0 + q; it is swept iff first <= a0 + q < end. Every wave of the grid
// writes its 8 flag words (both arrays for retire), every workgroup its counts, also where no
// position is swept (zeros), so the workspace needs no clearing.
template <bool kRetire, typename Op>
__global__ __launch_bounds__(256) void sweep_flag_kernel(uint64_t* __restrict__ pt, uint64_t a0,
                                                         uint64_t first, uint64_t end, Op op,
                                                         uint64_t* __restrict__ fa,
                                                         uint64_t* __restrict__ fb,
                                                         uint32_t* __restrict__ ca,
                                                         uint32_t* __restrict__ cb,
                                                         uint32_t* __restrict__ ch) {
  __shared__ uint32_t s_cnt[4][3];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t slot = (uint64_t)blockIdx.x * 4 + wave;
  const uint64_t p0 = a0 + slot * kWave;  // the wave's first table page (even)
  const bool body = p0 >= first && p0 + kWave <= end;  // wave-uniform
  // The range guard: a position outside [first, end) is never loaded and its word reads as 0.
  // retire needs no more: 0 is INVALID, which it leaves alone, counts nowhere and never stores.
  // select matches words against (mask, value), 0 included, so it also keeps `in` per position.
  uint32_t w[kSteps][2];
  bool in[kSteps][2];
  if (body) {
#pragma unroll
    for (uint32_t j = 0; j < kSteps; ++j) {
      const u32x4 v = *reinterpret_cast<const u32x4*>(pt + p0 + j * kStep + 2 * lane);
      w[j][0] = v.x;
      w[j][1] = v.z;
      if constexpr (!kRetire) in[j][0] = in[j][1] = true;
    }
  } else {
#pragma unroll
    for (uint32_t j = 0; j < kSteps; ++j) {
#pragma unroll
      for (uint32_t k = 0; k < 2; ++k) {
        const uint64_t p = p0 + j * kStep + 2 * lane + k;
        const bool inside = p >= first && p < end;
        w[j][k] = inside ? (uint32_t)pt[p] : 0u;
        if constexpr (!kRetire) in[j][k] = inside;
      }
    }
  }
  // Flag words stay as the ballots give them: the emit kernel ranks the even and the odd
  // positions of a pair, so nothing is interleaved here.
  uint64_t my_a = 0, my_b = 0;  // lane i < 8: the wave's flag word i
  uint32_t n_a = 0, n_b = 0;    // wave-uniform
  uint32_t my_held = 0;         // per lane
#pragma unroll
  for (uint32_t j = 0; j < kSteps; ++j) {
    bool a[2], b[2] = {false, false};
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
      if constexpr (kRetire) {
        const uint64_t p = p0 + j * kStep + 2 * lane + k;
        bool held;
        const uint32_t nw = retire_word(op, w[j][k], p, a[k], b[k], held);
        my_held += held ? 1u : 0u;
        if (nw != w[j][k] && !op.dry) *reinterpret_cast<uint32_t*>(pt + p) = nw;
      } else {
        a[k] = in[j][k] && (w[j][k] & op.mask) == op.value;
      }
    }
    const uint64_t ea = __ballot(a[0]), oa = __ballot(a[1]);
    n_a += (uint32_t)(__popcll(ea) + __popcll(oa));
    my_a = lane == 2 * j ? ea : lane == 2 * j + 1 ? oa : my_a;
    if constexpr (kRetire) {
      const uint64_t eb = __ballot(b[0]), ob = __ballot(b[1]);
      n_b += (uint32_t)(__popcll(eb) + __popcll(ob));
      my_b = lane == 2 * j ? eb : lane == 2 * j + 1 ? ob : my_b;
    }
  }
  const uint32_t n_held = kRetire ? wave_sum(my_held) : 0u;
  if (lane < kWaveWords) {
    fa[slot * kWaveWords + lane] = my_a;
    if constexpr (kRetire) fb[slot * kWaveWords + lane] = my_b;
  }
  // the tile's counts: one word each, so that the sum kernel reads 4 B per tile
  if (lane == 0) {
    s_cnt[wave][0] = n_a;
    s_cnt[wave][1] = n_b;
    s_cnt[wave][2] = n_held;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ca[blockIdx.x] = s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0];
    if constexpr (kRetire) {
      cb[blockIdx.x] = s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1];
      ch[blockIdx.x] = s_cnt[0][2] + s_cnt[1][2] + s_cnt[2][2] + s_cnt[3][2];
    }
  }
}

// ------------------------------------------------------------------------- tile counts -> offsets
// One workgroup: off[t] = the flagged pages before tile t; out (may be NULL) = retire's {held,
// moved, orphaned} or select's count. A step of the scan has a dependent load and two barriers,
// about 1 us whatever it carries, so a thread takes 16 tiles per step (four 16-B loads in flight):
// 4096 tiles a step, 2 steps for a 16 M-page table.
namespace {

// c[j] = cnt[t0 + j] for the tiles below NT (0 past them); returns their sum.
__device__ __forceinline__ uint32_t load_group(const uint32_t* __restrict__ cnt, uint64_t t0,
                                               uint64_t NT, uint32_t (&c)[kGroup]) {
  if (t0 + kGroup <= NT) {  // (the arrays are padded to whole groups and 16-B aligned)
    const u32x4* v = reinterpret_cast<const u32x4*>(cnt + t0);
#pragma unroll
    for (uint32_t q = 0; q < kGroup / 4; ++q) {
      const u32x4 x = v[q];
      c[4 * q] = x.x;
      c[4 * q + 1] = x.y;
      c[4 * q + 2] = x.z;
      c[4 * q + 3] = x.w;
    }
  } else {
#pragma unroll
    for (uint32_t j = 0; j < kGroup; ++j) c[j] = t0 + j < NT ? cnt[t0 + j] : 0u;
  }
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t j = 0; j < kGroup; ++j) sum += c[j];
  return sum;
}

}  // namespace

template <bool kRetire>
__global__ __launch_bounds__(256) void sweep_sum_kernel(const uint32_t* __restrict__ ca,
                                                        const uint32_t* __restrict__ cb,
                                                        const uint32_t* __restrict__ ch,
                                                        uint64_t NT, uint64_t* __restrict__ off,
                                                        uint64_t* __restrict__ out) {
  __shared__ uint64_t wsum[4][2];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t orphans = 0, held = 0;
  uint32_t c[kGroup];  // the group's counts, from load to store of the same step
  const uint64_t carry = block_excl_scan<uint64_t>(
      (NT + kGroup - 1) / kGroup,
      [&](uint64_t g) {
        if (kRetire) {
          orphans += load_group(cb, g * kGroup, NT, c);
          held += load_group(ch, g * kGroup, NT, c);
        }
        return load_group(ca, g * kGroup, NT, c);
      },
      [&](uint64_t g, uint64_t before) {
#pragma unroll
        for (uint32_t j = 0; j < kGroup; ++j) {
          if (g * kGroup + j < NT) off[g * kGroup + j] = before;
          before += c[j];
        }
      });
  if (kRetire) {
    orphans = wave_sum64(orphans);
    held = wave_sum64(held);
    if (lane == 0) {
      wsum[wave][0] = orphans;
      wsum[wave][1] = held;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0 && out) {
    if (kRetire) {
      out[0] = wsum[0][1] + wsum[1][1] + wsum[2][1] + wsum[3][1];
      out[1] = carry;
      out[2] = wsum[0][0] + wsum[1][0] + wsum[2][0] + wsum[3][0];
    } else {
      out[0] = carry;
    }
  }
}

// ------------------------------------------------------------------------- emit
// A workgroup per tile, a wave per 4 of its 16 pairs of flag words (the pairs a wave of the flag
// kernel wrote), one pair (e, o) at a time: lane l has the pair's positions 2 l (bit l of e) and
// 2 l + 1 (bit l of o). The k-th flagged page of the range goes to out[k]; for position 2 l,
// k = off[tile] + the set bits of the tile's earlier pairs + the bits of e and of o below l, and
// position 2 l + 1 follows it. Entries at or past cap are dropped (the counts still hold them).
// Every wave loads the tile's 32 words once, a lane each, and scans their popcounts. page0 = base
// + a0. retire: bit 31 = the page's orphan flag.
template <bool kRetire>
__global__ __launch_bounds__(256) void sweep_emit_kernel(const uint64_t* __restrict__ fa,
                                                         const uint64_t* __restrict__ fb,
                                                         const uint64_t* __restrict__ off,
                                                         uint64_t page0,
                                                         uint32_t* __restrict__ out, uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t w0 = (uint64_t)blockIdx.x * kTileWords;
  const uint64_t mine = lane < kTileWords ? fa[w0 + lane] : 0ull;
  const uint32_t pc = (uint32_t)__popcll(mine);
  const uint32_t incl = wave_incl_sum(pc);
  if (lane_bcast(incl, 63) == 0) return;  // wave-uniform: most tiles of a sparse answer
  const uint64_t k0 = off[blockIdx.x];
  if (k0 >= cap) return;  // wave-uniform
  uint64_t mine_b = 0;
  if (kRetire) mine_b = lane < kTileWords ? fb[w0 + lane] : 0ull;
  for (uint32_t j = 0; j < kSteps; ++j) {
    const int i = (int)(2 * (wave * kSteps + j));  // the pair's first word in the tile
    const uint64_t e = lane_bcast64(mine, i), o = lane_bcast64(mine, i + 1);
    if ((e | o) == 0) continue;  // wave-uniform
    const bool has_e = (e >> lane) & 1ull, has_o = (o >> lane) & 1ull;
    const uint64_t k = k0 + (lane_bcast(incl, i) - lane_bcast(pc, i)) + ballot_rank(e) + ballot_rank(o);
    const uint32_t page = (uint32_t)(page0 + (w0 + i) * 64 + 2 * lane);
    uint32_t orph_e = 0, orph_o = 0;
    if (kRetire) {
      orph_e = (uint32_t)((lane_bcast64(mine_b, i) >> lane) & 1ull) << 31;
      orph_o = (uint32_t)((lane_bcast64(mine_b, i + 1) >> lane) & 1ull) << 31;
    }
    if (has_e && k < cap) out[k] = page | orph_e;
    if (has_o && k + has_e < cap) out[k + has_e] = (page + 1) | orph_o;
  }
}

// ------------------------------------------------------------------------- launchers
namespace {

template <bool kRetire, typename Op>
hipError_t launch_sweep(uint64_t* pt, const Op& op, uint64_t base, uint64_t first, uint64_t n,
                        uint32_t* out, uint64_t cap, uint64_t* totals, uint8_t* ws,
                        uint64_t ws_bytes, hipStream_t s) {
  if (n == 0) return totals ? hipMemsetAsync(totals, 0, kRetire ? 24 : 8, s) : hipSuccess;
  if (n > (1ull << 28) || ws_bytes < sweep_workspace_bytes(n)) return hipErrorInvalidValue;
  const uint64_t a0 = first & ~1ull, end = first + n;
  const uint64_t NT = (end - a0 + kTile - 1) / kTile, W = NT * kTileWords;
  const uint64_t NTp = padded_tiles(NT);
  uint32_t* ca = reinterpret_cast<uint32_t*>(ws);  // first: the 16-B loads need ws's alignment
  uint32_t* cb = ca + NTp;
  uint32_t* ch = cb + NTp;
  uint64_t* off = reinterpret_cast<uint64_t*>(ch + NTp);
  uint64_t* fa = off + NT;
  uint64_t* fb = fa + W;
  hipLaunchKernelGGL((sweep_flag_kernel<kRetire, Op>), dim3((unsigned)NT), dim3(256), 0, s, pt, a0,
                     first, end, op, fa, fb, ca, cb, ch);
  hipLaunchKernelGGL(sweep_sum_kernel<kRetire>, dim3(1), dim3(256), 0, s, ca, cb, ch, NT, off,
                     totals);
  if (cap && out)
    hipLaunchKernelGGL(sweep_emit_kernel<kRetire>, dim3((unsigned)NT), dim3(256), 0, s, fa, fb, off,
                       base + a0, out, cap);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_coh_retire(uint64_t* pt, uint32_t n_nodes, uint32_t node, uint32_t heir,
                             uint64_t base, uint64_t per, uint64_t first, uint64_t n,
                             uint32_t* moved_out, uint64_t cap, uint64_t* stats, bool dry,
                             uint8_t* ws, uint64_t ws_bytes, hipStream_t s) {
  Retire r;
  r.x = node;
  r.heir = heir;
  r.n_nodes = n_nodes;
  r.per = per > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)per;
  r.base = base;
  r.dry = dry ? 1u : 0u;
  return launch_sweep<true>(pt, r, base, first, n, moved_out, cap, stats, ws, ws_bytes, s);
}

hipError_t launch_coh_select(const uint64_t* pt, uint32_t mask, uint32_t value, uint64_t base,
                             uint64_t first, uint64_t n, uint32_t* pages_out, uint64_t cap,
                             uint64_t* count, uint8_t* ws, uint64_t ws_bytes, hipStream_t s) {
  const Select q{mask, value};
  return launch_sweep<false>(const_cast<uint64_t*>(pt), q, base, first, n, pages_out, cap, count,
                             ws, ws_bytes, s);
}

}  // namespace gdsm
