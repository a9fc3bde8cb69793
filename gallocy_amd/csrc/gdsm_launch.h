// Host-side launchers for the gdsm kernels (internal; the public ABI is include/gdsm.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "gdsm_prof.h"

namespace gdsm {

// Workspace of one diff of n list entries (ticket counter + one look-back granule per unit).
uint64_t diff_workspace_bytes(uint64_t n);
// Tuning knobs (gdsm_tune.cpp: one table row each, with its key, environment variable, accepted
// values and default). tune returns -1 for an unknown key or a value the knob does not accept.
enum Knob {
  kDiffVariant,
  kApplyVariant,
  kDiffSoloMax,
  kDiffChain,
  kCohVariant,
  kCohChain,
  kCohSpan,
  kRoundsXcd,
  kRoundsLds,
  kRoundsLdsWg,
#ifdef GDSM_MEASURE
  kDiffSkip,  // the chained release's kSkip
#endif
  kKnobs
};
int knob(Knob k);
int tune(const char* key, int64_t value);
constexpr uint32_t kSoloUnits = 16;  // pages of the one-workgroup release (gdsm_pages.hip, kSolo)

// Bits of the device error word (gdsm_ctx::err), set by the kernels and read by gdsm_sync.
constexpr uint32_t kErrRecord = 1;          // malformed record (apply, merge)
constexpr uint32_t kErrEvents = 2;          // coherence batch not sorted / out of range
constexpr uint32_t kErrNw = 4;              // GPU NW input out of range
constexpr uint32_t kErrIds = 8;             // page id / index out of range
constexpr uint32_t kErrStream = 16;         // stream with malformed offsets
constexpr uint32_t kErrOverBudget = 32;     // fixed-budget exchanged stream over its budget
constexpr uint32_t kErrRoundsBarrier = 64;  // gdsm_rounds: a persistent grid's barrier never completed
constexpr uint32_t kErrRoundsWrites = 128;  // ... a round's writes not 8-B aligned or outside its pages

// Workgroups of a launch: ceil(work / per_block), at most cap, at least 1.
inline unsigned grid_for(uint64_t work, unsigned per_block, unsigned cap) {
  uint64_t g = (work + per_block - 1) / per_block;
  if (g > cap) g = cap;
  return g ? (unsigned)g : 1u;
}

hipError_t launch_gen_pages(uint8_t* twin, uint8_t* cur, uint8_t* replica, uint64_t n,
                            uint64_t first_global, uint64_t stride, uint64_t seed, int mode,
                            uint32_t ppm, hipStream_t s);
// With a caller list, n_pages / err guard it in the kernel (ids >= n_pages -> the guard page
// n_pages, err |= 8); the defaults leave the list unchecked (raw entry points).
hipError_t launch_twin(uint8_t* twin, const uint8_t* cur, const uint32_t* ids, uint64_t n,
                       hipStream_t s, Prof* prof = nullptr, uint64_t n_pages = ~0ull,
                       uint32_t* err = nullptr);
// Full diff of n pages in one pass: rec_off[n+1], data[cap]. With `target`, the runs are also
// applied to target by the same kernel, page tids[i] for list entry i (tids NULL: the same page
// ids). bpp_hint: stream bytes per page the caller saw last time (0 = unknown); it only picks
// the geometry.
// Caller page-id lists checked by the diff launch itself (in the launch that zeroes its
// workspace): safe_ids[i] = ids[i] if < n_pages, else n_pages (the guard page), the same for
// tids, err |= 8 when any id was out of range. A null list is not checked.
struct IdGuard {
  const uint32_t* ids;
  const uint32_t* tids;
  uint32_t* safe_ids;
  uint32_t* safe_tids;
  uint64_t n_pages;
  uint32_t* err;
};
// A context's chain of zero-free diff launches: lists of at most kDiffChainUnits pages (one-page
// units) take one launch, no workspace-zeroing launch before it. ws (diff_chain_bytes(), device)
// holds two ticket counters and one epoch-tagged look-back granule per unit; it is zeroed once
// (epoch 0: by the next launch, then epoch 1). Launch E draws its tickets from counter E & 1 and
// zeroes counter (E + 1) & 1 for launch E + 1; a granule counts only when it carries E. Not for
// graph capture (a replayed launch would repeat its epoch).
constexpr uint64_t kDiffChainUnits = 2048;
struct DiffChain {
  uint64_t* ws = nullptr;
  uint32_t epoch = 0;  // the next launch's epoch, 1 .. 2^30 - 1; 0 = zero ws first
};
uint64_t diff_chain_bytes();
// The geometry the calling thread's last diff launch took (gdsm_debug_last_diff_variant):
// variant 1 .. 8 (gdsm_pages.hip's table) | form << 8; 0 before any launch on this thread.
enum DiffForm { kFormGrid = 0, kFormSolo = 1, kFormChainPage = 2, kFormChainWave = 3 };
int last_diff_variant();
// With `guard`, the kernel reads guard->safe_ids / safe_tids in place of ids / tids.
hipError_t launch_diff(const uint8_t* twin, const uint8_t* cur, const uint32_t* ids, uint64_t n,
                       uint64_t* rec_off, uint8_t* data, uint64_t cap, uint8_t* ws,
                       uint64_t ws_bytes, hipStream_t s, Prof* prof = nullptr,
                       uint8_t* target = nullptr, uint32_t bpp_hint = 0,
                       const uint32_t* tids = nullptr, const IdGuard* guard = nullptr,
                       uint8_t* retwin = nullptr, DiffChain* chain = nullptr);
// retwin (gdsm_release's GDSM_RELEASE_RETWIN; must be the `twin` arena): after the diff, TWIN :=
// CURRENT for every listed page whose record fits the capacity (inside the one-workgroup kernel
// of a short release, by a second launch otherwise).
// The diff kernel's output streams: list entries [first[d], first[d+1]) go to stream d (record
// i of stream d = entry first[d] + i); ustart: the first work unit of each stream (set by the
// launcher). One launch serves them all, each stream with its own look-back chain.
constexpr uint32_t kMaxSplit = 8;
struct DiffSplit {
  uint64_t* rec_off[kMaxSplit];
  uint8_t* data[kMaxSplit];
  uint64_t cap[kMaxSplit];
  uint64_t first[kMaxSplit + 1];
  uint64_t ustart[kMaxSplit + 1];
  uint32_t G;
  uint32_t epoch;  // a DiffChain launch's epoch (set by the launcher)
};
// One diff launch over arena pages [first[0], first[G]) (ids = identity) into sp's G streams.
hipError_t launch_copy_batch(const uint64_t* desc, uint64_t n, hipStream_t s);
// DSM rounds on the device (gdsm_rounds): the page-data side, one persistent launch of `grid`
// workgroups: per round the release of list entries [off[r], off[r+1]) of ids (home indices tids
// into target, re-twin) with its copy descriptors [doff[r], doff[r+1]) of desc laid onto the
// pages, then a grid barrier. off / doff on the device; look-back granules in chain_ws
// (DiffChain layout) with epochs epoch0 + r; bar: kRoundsBarBytes zeroed by the launcher.
// xcd: the rounds run on a one-XCD team of the grid (xcd_team: about grid / 8 members).
hipError_t launch_rounds_data(const uint8_t* twin, const uint8_t* cur, const uint32_t* ids,
                              const uint32_t* tids, const int64_t* off, const uint64_t* desc,
                              const int64_t* doff, uint32_t n_rounds, uint32_t grid,
                              uint64_t* rec_off, uint8_t* data, uint64_t cap, uint64_t* chain_ws,
                              uint8_t* target, uint64_t n_pages, uint32_t* err, uint32_t epoch0,
                              uint32_t* bar, bool xcd, hipStream_t s, Prof* prof = nullptr);
const void* rounds_data_kernel_ptr(bool xcd);  // (for the occupancy query)
constexpr uint64_t kRoundsBarBytes = 256;      // a rounds grid's barrier and team words
hipError_t launch_diff_split(const uint8_t* twin, const uint8_t* cur, DiffSplit sp, uint8_t* ws,
                             uint64_t ws_bytes, hipStream_t s, Prof* prof, uint32_t bpp_hint);
hipError_t launch_apply(uint8_t* target, const uint32_t* ids, uint64_t n,
                        const uint64_t* rec_off, const uint8_t* data, uint32_t* err,
                        hipStream_t s, Prof* prof = nullptr);
// gdsm_merge (SPEC §8; gdsm_merge.hip): K <= 8 input streams in priority order, each with its
// offsets, data, capacity, record count and page list (NULL: record i is out entry i).
struct MergeIn {
  const uint64_t* rec_off[8];
  const uint8_t* data[8];
  const uint32_t* ids[8];
  uint64_t n[8];
  uint64_t cap[8];
  uint32_t K;
};
uint64_t merge_workspace_bytes(uint64_t n_out);
// The merged stream of out entries out_ids[0..n_out) (NULL: the identity) into out_rec_off[n_out+1]
// / out_data[out_cap]; conflicts (n_out x u32) and stats (2 x u64) may be NULL. err |= 1 for a
// malformed record (it contributes nothing), 16 / 8 for malformed offsets / an unsorted page list
// (the output is then empty). Five launches and two small memsets on s, no host synchronisation.
hipError_t launch_merge(const MergeIn& in, const uint32_t* out_ids, uint64_t n_out,
                        uint64_t* out_rec_off, uint8_t* out_data, uint64_t out_cap,
                        uint32_t* conflicts, uint64_t* stats, uint32_t* err, uint8_t* ws,
                        uint64_t ws_bytes, hipStream_t s, Prof* prof = nullptr);
// A stream about to be applied by gdsm_exchange: checked whole (offsets from 0, non-decreasing,
// 4-aligned, rec_off[n] <= budget; page indices < n_pages, copied to safe[n]). A rejected stream
// has every offset zeroed (nothing applied); err |= 16 (malformed offsets), 32 (over budget),
// 8 (bad page index). `verdict` is one device word of scratch.
hipError_t launch_xchg_guard(uint64_t* rec_off, const uint32_t* ids, uint64_t n, uint64_t budget,
                             uint64_t n_pages, uint32_t* safe, uint32_t* verdict, uint32_t* err,
                             hipStream_t s);
// err |= 32 when rec_off[n] > budget (a fixed-budget stream its sender shipped over budget).
hipError_t launch_budget_check(const uint64_t* rec_off, uint64_t n, uint64_t budget,
                               uint32_t* err, hipStream_t s);
// Caller page-id lists at the context level: safe[i] = ids[i] if < n_pages, else n_pages (the
// arenas' guard page), and err |= 8 when any id was out of range.
hipError_t launch_check_ids(const uint32_t* ids, uint64_t n, uint64_t n_pages, uint32_t* safe,
                            uint32_t* err, hipStream_t s);

// Coherence (SPEC §5).
uint64_t coh_workspace_bytes(uint64_t n_events);
// Page table: one u64 per page, state | faults << 32.
hipError_t launch_coh_init(uint64_t* pt, uint64_t n_pages, uint32_t n_nodes, hipStream_t s);
// A context's chain of zero-free small coherence batches (as DiffChain): ws (coh_chain_bytes(),
// device) holds two sets of ticket counters, totals rows and completion counters, then
// epoch-tagged status granules; zeroed once (epoch 0: by the next launch). Not for graph capture.
struct CohChainState {
  uint64_t* ws = nullptr;
  uint32_t epoch = 0;
};
uint64_t coh_chain_bytes();
// Events naming a page >= n_pages or a node >= n_nodes reject the batch (err |= 2).
hipError_t launch_coherence(uint64_t* pt, uint64_t n_pages, uint32_t n_nodes,
                            const uint64_t* events, uint64_t n_events, uint64_t* totals,
                            uint8_t* ws, uint64_t ws_bytes, uint32_t* err, hipStream_t s,
                            Prof* prof = nullptr, CohChainState* chain = nullptr);
// DSM rounds on the device (gdsm_rounds): the page-table side, one persistent launch of `grid`
// workgroups over n_rounds rounds (eoff: device, n_rounds + 1 event offsets; totals: 10 u64 per
// round). Uses the chain's ws with epochs of its own; the chain restarts (zeroed) afterwards.
// bar: kRoundsBarBytes zeroed by the launcher; xcd: a one-XCD team (as launch_rounds_data).
// lds: instead `grid` workgroups (<= kRoundsLdsMaxWGs) with the page table in LDS slices of
// ceil(n_pages / grid) <= kRoundsLdsPages pages (every round <= kRoundsLdsEvents events, n_rounds
// <= kRoundsLdsRounds; chain and bar unused).
constexpr uint64_t kRoundsLdsPages = 8192;    // 64 KiB of page-table words per workgroup
constexpr uint32_t kRoundsLdsMaxWGs = 16;     // workgroups (page-table slices) of the LDS form
constexpr uint64_t kRoundsLdsWGEvents = 4096; // a round's events per workgroup the host aims at
constexpr uint64_t kRoundsLdsEvents = 16384;  // 64 KiB of a round's staged events
constexpr uint32_t kRoundsLdsRounds = 2048;   // 16 KiB of event offsets
// (gdsm_rounds takes the LDS form whenever it fits: config 5, same box, against the grid fold,
// 1 / 2 / 4 / 8 nodes on 1 / 1 / 2 / 4 workgroups: +12 % / tied / +12 % / +5 %; one workgroup
// alone at 4 and 8 nodes was the slower form, -10 % / -25 %, profiles/r06_rounds_lds_ab.txt)
hipError_t launch_rounds_fold(uint64_t* pt, uint64_t n_pages, uint32_t n_nodes,
                              const uint64_t* events, const int64_t* eoff, uint32_t n_rounds,
                              uint32_t grid, uint64_t* totals, uint32_t* err, CohChainState* chain,
                              uint32_t* bar, bool xcd, bool lds, hipStream_t s,
                              Prof* prof = nullptr);
const void* rounds_fold_kernel_ptr(bool xcd);  // (for the occupancy query)
hipError_t launch_gen_events(uint64_t* events, const uint64_t* offsets, uint64_t first_page,
                             uint64_t n, uint64_t seed, uint32_t n_nodes, uint32_t write_pct,
                             hipStream_t s);

// Coherence across GPUs (SPEC §5b; gdsm_route.hip).
// A node's stamped events: validation (bad |= 1), per-home bounds[G+1] and counts[G] (u64).
hipError_t launch_route_split(const uint64_t* ev, uint64_t n, uint64_t total_pages, uint64_t per,
                              uint32_t G, uint64_t* counts, uint64_t* bounds, uint32_t* bad,
                              hipStream_t s);
// G sorted runs (host offsets off[G+1] into `runs`) merged into one page-sorted local batch.
hipError_t launch_route_merge(const uint64_t* runs, const uint64_t* off, uint32_t G, uint64_t base,
                              uint64_t* out, hipStream_t s);
uint64_t notice_blocks(uint64_t n);
// pre[i] = the page-table word at each page's first event; *heads = the batch's distinct pages.
hipError_t launch_notice_pre(const uint64_t* pt, uint64_t n_pages, const uint64_t* batch,
                             uint64_t n, uint32_t* pre, uint64_t* heads, hipStream_t s);
// blk: notice_blocks(n) x 8 u32; blk_off the same in u64; dest_total / dest_base: G u64 each.
hipError_t launch_notice_count(const uint64_t* pt, uint64_t n_pages, const uint64_t* batch,
                               uint64_t n, const uint32_t* pre, uint32_t G, uint32_t* blk,
                               uint64_t* blk_off, uint64_t* dest_total, uint64_t* dest_base,
                               hipStream_t s);
hipError_t launch_notice_emit(const uint64_t* pt, uint64_t n_pages, const uint64_t* batch,
                              uint64_t n, const uint32_t* pre, uint32_t G, uint64_t base,
                              const uint64_t* blk_off, const uint64_t* dest_base, uint64_t* out,
                              hipStream_t s);

// Page fetch (SPEC §9; gdsm_fetch.hip).
constexpr uint32_t kFetchMaxRanks = 255;  // the split finds every home's slice in one workgroup
// A rank's request list: validation (bad |= 1: not strictly ascending, a page >= total_pages, a
// destination >= n_pages), per-home bounds[G+1] and counts[G] (u64; they always sum to n).
hipError_t launch_fetch_split(const uint32_t* pages, const uint32_t* dst_ids, uint64_t n,
                              uint64_t total_pages, uint64_t per, uint32_t G, uint64_t n_pages,
                              uint64_t* counts, uint64_t* bounds, uint32_t* bad, hipStream_t s);
// Home: staging[j] := page req[j] - base of src for the n received requests; an id outside
// [base, base + block) copies nothing (err |= 8).
hipError_t launch_fetch_gather(const uint8_t* src, const uint32_t* req, uint64_t n, uint64_t base,
                               uint64_t block, uint8_t* staging, uint32_t* err, hipStream_t s);
// Requester: the cnt list entries outside [skip_at, skip_at + skip), in order, from staging pages
// 0 .. cnt - 1 into a0 / a1 (a1 may be NULL) at dst_ids[i] (NULL: pages[i]).
hipError_t launch_fetch_scatter(const uint8_t* staging, const uint32_t* pages,
                                const uint32_t* dst_ids, uint64_t skip_at, uint64_t skip,
                                uint64_t cnt, uint64_t n_pages, uint8_t* a0, uint8_t* a1,
                                uint32_t* err, hipStream_t s);
// Requester and home at once: list entries [first, first + cnt) from src page pages[i] - base.
hipError_t launch_fetch_local(const uint8_t* src, const uint32_t* pages, const uint32_t* dst_ids,
                              uint64_t first, uint64_t cnt, uint64_t base, uint64_t block,
                              uint64_t n_pages, uint8_t* a0, uint8_t* a1, uint32_t* err,
                              hipStream_t s);
// Notices -> fetch list: blk (u32) and blk_off (u64) hold fetch_list_blocks(n) entries each;
// *total = the wanted notices, of which the first cap pages are written to out.
uint64_t fetch_list_blocks(uint64_t n);
hipError_t launch_fetch_list(const uint64_t* notices, uint64_t n, uint32_t want, uint32_t* blk,
                             uint64_t* blk_off, uint64_t* total, uint32_t* out, uint64_t cap,
                             hipStream_t s);

// Page digest (SPEC §10; gdsm_digest.hip): out[2i], out[2i+1] = (S0, S1) of page ids[i] (NULL:
// page i) of arena; an id >= n_pages gets (0, 0) and err |= 8 (err may be NULL when n_pages is ~0:
// raw callers). No workspace, one launch.
hipError_t launch_digest(const uint8_t* arena, const uint32_t* ids, uint64_t n, uint64_t n_pages,
                         uint64_t* out, uint32_t* err, hipStream_t s, Prof* prof = nullptr);

// Conditional fetch (SPEC §11; gdsm_digest.hip). List arguments as the fetch launchers above.
// Requester: dig[2k], dig[2k+1] = the digest of a's page dst(i) for its k-th entry homed elsewhere.
hipError_t launch_fetchc_offer(const uint8_t* a, const uint32_t* pages, const uint32_t* dst_ids,
                               uint64_t skip_at, uint64_t skip, uint64_t cnt, uint64_t n_pages,
                               uint64_t* dig, uint32_t* err, hipStream_t s);
// Home: flags[j] = 1 when src's page req[j] - base does not have the digest dig[2j], dig[2j+1];
// 0 for a request outside [base, base + block) (err |= 8).
hipError_t launch_fetchc_verify(const uint8_t* src, const uint32_t* req, const uint64_t* dig,
                                uint64_t n, uint64_t base, uint64_t block, uint32_t* flags,
                                uint32_t* err, hipStream_t s);
// pos[i] = the set flags before entry i, pos[m] = their total (m + 1 words); blk and blk_off hold
// fetchc_pos_blocks(m) u32 each.
uint64_t fetchc_pos_blocks(uint64_t m);
hipError_t launch_fetchc_pos(const uint32_t* flags, uint64_t m, uint32_t* blk, uint32_t* blk_off,
                             uint32_t* pos, hipStream_t s);
// counts[p] = pos[off[p+1]] - pos[off[p]] for the G slices off[G+1] (device) of the home's requests.
hipError_t launch_fetchc_slices(const uint32_t* pos, const uint64_t* off, uint32_t G,
                                uint64_t* counts, hipStream_t s);
// Home: staging[pos[j]] := page req[j] - base of src for the requests with flags[j] set.
hipError_t launch_fetchc_gather(const uint8_t* src, const uint32_t* req, const uint32_t* flags,
                                const uint32_t* pos, uint64_t n, uint64_t base, uint64_t block,
                                uint8_t* staging, hipStream_t s);
// Requester: its cnt entries homed elsewhere; with flags[k] set, staging page pos[k] into a0 / a1,
// otherwise a1 (when not NULL) := a0's page. changed (n entries) and stats (4 u64: [0] += the
// entries replaced, [1] += the entries kept) may be NULL.
hipError_t launch_fetchc_place(const uint8_t* staging, const uint32_t* pages,
                               const uint32_t* dst_ids, const uint32_t* flags, const uint32_t* pos,
                               uint64_t skip_at, uint64_t skip, uint64_t cnt, uint64_t n_pages,
                               uint8_t* a0, uint8_t* a1, uint32_t* changed, uint64_t* stats,
                               uint32_t* err, hipStream_t s);
// Requester and home at once: entries [first, first + cnt) compared byte for byte with src's page
// pages[i] - base; a0 is stored when it differs, a1 (when not NULL) always. stats[2] / [3].
hipError_t launch_fetchc_local(const uint8_t* src, const uint32_t* pages, const uint32_t* dst_ids,
                               uint64_t first, uint64_t cnt, uint64_t base, uint64_t block,
                               uint64_t n_pages, uint8_t* a0, uint8_t* a1, uint32_t* changed,
                               uint64_t* stats, uint32_t* err, hipStream_t s);

// Dirty scan (SPEC §12; gdsm_dirty.hip): the entries i of the list ids[0..n) (NULL: the identity)
// whose page differs between arenas a and b, compacted in list order: pages_out[k] = the page,
// pos_out[k] = i (either may be NULL), the first cap of them; stats (2 x u64, may be NULL) = their
// number and the sum of min(10244, 4 + 48 x differing 16-B chunks) over them. An id >= n_pages is
// not dirty and err |= 8 (err may be NULL when n_pages is ~0: raw callers). ws: 8-byte aligned,
// dirty_workspace_bytes(n), its contents need not be kept. Three launches on s (n == 0: one
// memset), no host synchronisation.
uint64_t dirty_workspace_bytes(uint64_t n);
hipError_t launch_dirty_scan(const uint8_t* a, const uint8_t* b, const uint32_t* ids, uint64_t n,
                             uint64_t n_pages, uint32_t* pages_out, uint32_t* pos_out,
                             uint64_t cap, uint64_t* stats, uint32_t* err, uint8_t* ws,
                             uint64_t ws_bytes, hipStream_t s);

// Page-table sweeps (SPEC §14; gdsm_sweep.hip) over table pages [first, first + n) of pt (u64 =
// state | faults << 32; first + n within the table, base + first + n <= 2^28). Retire: node out of
// every copyset, the pages it owned to their heirs (per ? home : heir; a home >= n_nodes or == node
// gives heir); stats (3 x u64, may be NULL) = {held, moved, orphaned}; moved_out[k] = (base + p) |
// orphaned << 31 of the k-th moved page, ascending, the first cap of them; dry: the table is only
// read. Select: pages_out[k] = base + p of the k-th page with (word & mask) == value, the first cap;
// count (1 x u64, may be NULL). The counts are the true ones whatever cap is; a list may be NULL
// (nothing emitted). ws: 16-byte aligned, sweep_workspace_bytes(n), its contents need not be kept.
// Three launches on s (two without a list; n == 0: one memset), no host synchronisation.
uint64_t sweep_workspace_bytes(uint64_t n);
hipError_t launch_coh_retire(uint64_t* pt, uint32_t n_nodes, uint32_t node, uint32_t heir,
                             uint64_t base, uint64_t per, uint64_t first, uint64_t n,
                             uint32_t* moved_out, uint64_t cap, uint64_t* stats, bool dry,
                             uint8_t* ws, uint64_t ws_bytes, hipStream_t s);
hipError_t launch_coh_select(const uint64_t* pt, uint32_t mask, uint32_t value, uint64_t base,
                             uint64_t first, uint64_t n, uint32_t* pages_out, uint64_t cap,
                             uint64_t* count, uint8_t* ws, uint64_t ws_bytes, hipStream_t s);

// The page table by page list (SPEC §15; gdsm_cohlist.hip): entry i of the device list ids (n
// entries, 4-B aligned; NULL: table pages 0 .. n-1, n <= n_pages) works on table page ids[i] - base
// of pt (n_pages >= 1 u64 words). Clean: the dirty bit of the pages `node` owns dirty is cleared
// with a 32-bit atomic on the state half; status_out (n bytes, may be NULL): 0 cleaned, 1 already
// clean, 2 owned by another node, 3 INVALID, 4 out of range; stats (4 x u64, may be NULL; zeroed
// by a memset node ahead of the launch) = {cleaned, already, stale, skipped (3 and 4)}. Lookup:
// out[i] = INVALID or out of range ? 0 : (word >> shift) & mask; faults_out[i] (may be NULL) = the
// page's faults, 0 out of range. An id out of range sets kErrIds in *err. One launch on s, no
// workspace, no host synchronisation; n == 0: only the memset of stats. hipErrorInvalidValue, with
// nothing enqueued: n > 2^32, n > 0 with n_pages == 0, ids NULL with n > n_pages, lookup's n > 0
// with out NULL or shift > 31.
hipError_t launch_coh_clean(uint64_t* pt, uint64_t n_pages, uint32_t node, const uint32_t* ids,
                            uint64_t n, uint64_t base, uint8_t* status_out, uint64_t* stats,
                            uint32_t* err, hipStream_t s);
hipError_t launch_coh_lookup(const uint64_t* pt, uint64_t n_pages, const uint32_t* ids, uint64_t n,
                             uint64_t base, uint32_t shift, uint32_t mask, uint32_t* out,
                             uint32_t* faults_out, uint32_t* err, hipStream_t s);

// Stream split (SPEC §13; gdsm_split.hip): the stream rec_off[n+1] / data[cap] partitioned stably
// into G streams. dest (n masks, bit d = stream d) or, with dest NULL, the home ids[i] / per with
// the page rewritten to ids[i] - home x per (ids NULL: page i); flags: GDSM_SPLIT_DROP_EMPTY. Every
// write is guarded: out_rec_off[d][j] for j <= out_n_cap[d], out_ids[d][j] (an entry may be NULL)
// for j < out_n_cap[d], data below out_cap[d] in whole dwords.
constexpr uint32_t kSplitTile = 256;     // records per tile of the counts and their scan
constexpr uint64_t kSplitHeader = 256;   // workspace bytes before the tile sums; [0, 4) the fatal word
struct SplitArgs {
  const uint64_t* rec_off;
  const uint8_t* data;
  uint64_t cap;
  const uint32_t* ids;
  const uint32_t* dest;
  uint64_t per;
  uint64_t n;
  uint32_t G;
  uint32_t flags;
  uint64_t* out_rec_off[8];
  uint8_t* out_data[8];
  uint64_t out_cap[8];
  uint64_t out_n_cap[8];
  uint32_t* out_ids[8];
};
uint64_t split_workspace_bytes(uint64_t n, uint32_t G);
// counts (device, 2G u64): {records, bytes} per stream, the true values whatever the capacities;
// err |= 16 for malformed input offsets, 8 for a destination >= G (err may be NULL): the outputs are
// then empty (counts 0, rec_off[0] = 0, no data written). ws: 8-byte aligned,
// split_workspace_bytes(n, G); the launcher uses its first 4 bytes and the tile sums, the rest of
// the header is the caller's. Five launches and a memset on s, no host synchronisation.
hipError_t launch_runs_split(const SplitArgs& a, uint64_t* counts, uint32_t* err, uint8_t* ws,
                             uint64_t ws_bytes, hipStream_t s);

// GPU NW alignment (legacy diff()): workspace per pair and the fill + trace launches.
uint64_t nw_pair_ws_bytes(uint32_t max_len);
hipError_t launch_nw(const uint8_t* a, const uint64_t* a_off, const uint8_t* b,
                     const uint64_t* b_off, uint64_t n, uint32_t max_len, uint8_t* out1,
                     uint8_t* out2, uint64_t* out_len, uint8_t* ws, uint64_t ws_bytes,
                     uint32_t* err, hipStream_t s, Prof* prof = nullptr);

// Diff wire format (SPEC §7).
uint64_t wire_frame_bytes(uint64_t n, uint64_t data_bytes);
hipError_t launch_wire_sum(const uint8_t* frame, uint64_t F, uint64_t* sum, hipStream_t s);
// dst[i] = i for i < n (identity page-id lists on the device).
hipError_t launch_iota(uint32_t* dst, uint64_t n, hipStream_t s);
hipError_t launch_b64_encode(const uint8_t* frame, uint64_t F, uint8_t* text, hipStream_t s);
hipError_t launch_b64_decode(const uint8_t* text, uint64_t T, uint32_t pad, uint8_t* frame,
                             uint64_t F, uint32_t* err, hipStream_t s);
hipError_t launch_wire_check(const uint32_t* ids, const uint64_t* rec_off, uint64_t n,
                             uint64_t D, uint64_t n_pages, uint32_t* err, hipStream_t s);

}  // namespace gdsm
