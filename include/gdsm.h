/*
 * gdsm — MI355X-native engine for gallocy's DSM hot path (page twin / run diff / apply /
 * batched coherence). C ABI: plain pointers and sizes, no torch or HIP types in signatures.
 * Semantics are frozen in docs/SPEC.md.
 *
 * Where each entry point sits in the reference (/root/reference, gallocy 0.0.438):
 *   - The reference has no plugin or operator registry; its hot-path "interface" is the leaf
 *     utility `int diff(const char*, size_t, char*&, const char*, size_t, char*&)`
 *     (gallocy/include/gallocy/utils/diff.h:9-11, gallocy/utils/diff.cpp:73-167) plus the
 *     page-tracking hooks of the allocator stack that were never written:
 *     `PageTableHeap<Super>` (gallocy/include/gallocy/heaplayers/pagetableheap.h:12-29, only a
 *     LOG_DEBUG) and the per-page record `ApplicationMemory`
 *     (gallocy/include/gallocy/models.h:171-213, declared, never defined).
 *   - gdsm_diff / gdsm_apply / gdsm_twin replace the twin/diff/apply steps of the
 *     fault → negotiate → "copy over the latest contents" flow that the reference describes but
 *     does not implement (resources/NUTSHELL.md:59-69, resources/IMPLEMENTATION.md:246-249);
 *     the run record is the (offset, bytes) edit of print_diff (gallocy/utils/diff.cpp:43-70).
 *   - gdsm_coh_* replace the ApplicationMemory table (`dirty, owner, permissions, faults`,
 *     models.h:171-213) and the missing page-table application step of Raft's `try_apply`
 *     (gallocy/consensus/state.cpp:308-316).
 *   - gdsm_nw_diff is the reference diff() with the alignment length returned (the reference
 *     drops it, diff.h:9-11); the unchanged legacy C++ symbol `diff` is declared at the bottom.
 *   - The allocator hooks gdsm_set_allocator mirror internal_malloc/internal_free
 *     (gallocy/include/gallocy/allocators/internal.h:75-82), which own diff()'s outputs.
 *
 * Conventions: every function returns 0 or a negative errno (-EINVAL -22, -ENOMEM -12,
 * -EIO -5 for a HIP failure, -ENOSPC -28, -ENODEV -19, -EOVERFLOW -75 for a fixed-budget exchange
 * stream over its budget, -ETIMEDOUT -110 for a loopback rank that never arrived) and never
 * aborts. Device work is
 * enqueued on the context's HIP stream and is asynchronous unless the comment says it
 * synchronises. One context per host thread, or external synchronisation.
 */
#ifndef GDSM_H_
#define GDSM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDSM_PAGE_SZ 4096u
#define GDSM_MAX_RUNS 2048u
#define GDSM_MAX_NODES 8u
/* Largest page table gdsm_coh_init accepts: page ids of coherence events fit 28 bits (1 TiB of
 * 4 KiB pages, beyond any one GPU's HBM). */
#define GDSM_MAX_COH_PAGES (1ull << 28)
/* Largest record: 4 + 4*2048 + 2048 (alternating bytes), SPEC §3. */
#define GDSM_MAX_RECORD 10244u

enum gdsm_arena_kind { GDSM_TWIN = 0, GDSM_CURRENT = 1, GDSM_REPLICA = 2 };
enum gdsm_gen_mode { GDSM_GEN_UNIFORM = 0, GDSM_GEN_CLUSTERED = 1 };
/* gdsm_init flags: which arenas the context allocates (all three when 0). */
enum gdsm_init_flags {
  GDSM_WANT_TWIN = 1u << 0,
  GDSM_WANT_CURRENT = 1u << 1,
  GDSM_WANT_REPLICA = 1u << 2,
  GDSM_NO_ARENAS = 1u << 31, /* page-table-only context */
};
/* Per-kernel stages timed by gdsm_prof_* (HIP events on the context stream). */
enum gdsm_prof_stage {
  GDSM_PROF_DIFF = 0,   /* diff_single_kernel: the dominant kernel of the hot path */
  GDSM_PROF_APPLY,      /* apply_kernel */
  GDSM_PROF_TWIN,       /* twin_kernel */
  GDSM_PROF_COH_FOLD,   /* coh_fold_kernel: the coherence batch */
  GDSM_PROF_COH_REDUCE, /* the batch totals */
  GDSM_PROF_NW_FILL,    /* GPU diff(): DP fill */
  GDSM_PROF_NW_TRACE,   /* GPU diff(): traceback + alignment strings */
  GDSM_PROF_EXCHANGE,   /* gdsm_exchange: the transfer of the record streams (RCCL group) */
  GDSM_PROF_ROUTE,      /* gdsm_route_events / gdsm_coherence_notify: the transfers */
  GDSM_PROF_EXCHANGE_WAIT, /* gdsm_exchange: the transfer plus the wait for the peers' streams */
  GDSM_PROF_MERGE,      /* gdsm_merge: its check, size, scan and emit launches together */
  GDSM_PROF_FETCH,      /* gdsm_fetch: its two transfer groups and the gather / scatter launches */
  GDSM_PROF_DIGEST,     /* gdsm_digest: digest_kernel */
  GDSM_PROF_STAGES
};

typedef struct gdsm_ctx gdsm_ctx;

/* A diff stream (SPEC §3). All pointers are device pointers. */
typedef struct gdsm_runs {
  uint64_t n;        /* records in the stream (set by gdsm_diff) */
  uint64_t* rec_off; /* n + 1 */
  uint8_t* data;     /* cap bytes */
  uint64_t cap;      /* data capacity in bytes */
  uint64_t n_cap;    /* record capacity: rec_off holds n_cap + 1 entries */
  uint32_t owned;    /* 1 if allocated by gdsm_runs_alloc */
  uint32_t _pad;
} gdsm_runs;

/* ---- context ------------------------------------------------------------------------- */
int gdsm_device_count(int* count);
/* Allocates the arenas (n_pages × 4 KiB each) on `device` and one HIP stream. */
int gdsm_init(gdsm_ctx** out, int device, uint64_t n_pages, uint32_t flags);
int gdsm_fini(gdsm_ctx* ctx);
int gdsm_arena(gdsm_ctx* ctx, int which, void** dev_ptr);
uint64_t gdsm_n_pages(const gdsm_ctx* ctx);
/* The context's hipStream_t, as an opaque pointer. */
void* gdsm_stream(gdsm_ctx* ctx);
/* Waits for all enqueued work; reports a device-side failure recorded since the last sync. */
int gdsm_sync(gdsm_ctx* ctx);
/* Synchronous host <-> arena copies of pages [first, first+n). */
int gdsm_upload(gdsm_ctx* ctx, int which, uint64_t first, uint64_t n, const void* host);
int gdsm_download(gdsm_ctx* ctx, int which, uint64_t first, uint64_t n, void* host);
/* Pre-sizes the context's diff and coherence workspaces so later calls never reallocate (a
 * reallocation synchronises the device). */
int gdsm_reserve(gdsm_ctx* ctx, uint64_t diff_pages, uint64_t coh_events);
/* Device scratch owned by the context (freed by gdsm_fini). */
int gdsm_dev_alloc(gdsm_ctx* ctx, uint64_t bytes, void** dev_ptr);
int gdsm_dev_free(gdsm_ctx* ctx, void* dev_ptr);
int gdsm_memcpy_h2d(gdsm_ctx* ctx, void* dev, const void* host, uint64_t bytes);
int gdsm_memcpy_d2h(gdsm_ctx* ctx, void* host, const void* dev, uint64_t bytes);
/* Asynchronous device-to-device copy on the context stream. */
int gdsm_memcpy_d2d(gdsm_ctx* ctx, void* dst, const void* src, uint64_t bytes);
/* n device-to-device copies in one launch on the context stream: desc (device, 3n u64) holds
 * (dst, src, bytes) per copy; the copies must not overlap each other. E.g. the application
 * writes of one DSM round replayed at once (gallocy_amd/replay.py). */
int gdsm_memcpy_batch(gdsm_ctx* ctx, const uint64_t* desc, uint64_t n);

/* HIP graphs: record a launch-bound sequence once and replay it with one launch.
 * - Between gdsm_capture_begin(ctx) and gdsm_capture_end(ctx, &g), the asynchronous calls on ctx
 *   are recorded, not run: gdsm_twin, gdsm_diff, gdsm_apply, gdsm_memcpy_d2d / _batch,
 *   gdsm_coherence_batch_async and the generators.
 * - gdsm_capture_join(ctx, other) adds a second context on the same device. Its asynchronous
 *   calls are recorded into the same graph, ordered after what ctx had recorded when it joined.
 *   ctx's recording waits for them at gdsm_capture_end.
 * - Size the workspaces beforehand with gdsm_reserve: a call that would grow one fails with
 *   -EBUSY, and so does gdsm_sync on a recording context. Other calls that synchronise the host
 *   fail too.
 * - gdsm_graph_launch enqueues the whole graph on ctx's stream; gdsm_sync reports its
 *   device-side failures as usual. Every recorded pointer must stay valid while the graph
 *   lives.
 * - A caller may also capture gdsm_stream(ctx) itself (hipStreamBeginCapture): every call checks
 *   hipStreamIsCapturing and then records the forms that replay correctly (a zeroing launch
 *   before each short diff / small coherence batch instead of the one-launch chained forms,
 *   whose per-launch epoch a replay would repeat). The same sizing rule applies. */
typedef struct gdsm_graph gdsm_graph;
int gdsm_capture_begin(gdsm_ctx* ctx);
int gdsm_capture_join(gdsm_ctx* ctx, gdsm_ctx* other);
int gdsm_capture_end(gdsm_ctx* ctx, gdsm_graph** out);
int gdsm_graph_launch(gdsm_ctx* ctx, const gdsm_graph* g);
int gdsm_graph_destroy(gdsm_graph* g);

/* Per-kernel timing: when enabled, every kernel the context launches is bracketed by HIP events
 * on its stream; gdsm_prof_read synchronises and returns the summed milliseconds and launch
 * counts per stage (arrays of GDSM_PROF_STAGES), then clears them. */
int gdsm_prof_enable(gdsm_ctx* ctx, int on);
int gdsm_prof_read(gdsm_ctx* ctx, double* ms, uint64_t* launches);

/* Box ceilings (measurement support for bench.py, gdsm_probe.hip; no reference counterpart): how
 * fast this GPU streams given page arenas, `reps` launches timed by HIP events on ctx's stream
 * (best and median ms per launch). GDSM_PROBE_READ: arenas a and b (n_pages each) read once, the
 * diff's input pattern; GDSM_PROBE_COPY: dst := a over n_pages pages (dst is overwritten), the
 * fastest of three copy shapes (`reps` launches each). */
#define GDSM_PROBE_READ 0
#define GDSM_PROBE_COPY 1
int gdsm_probe_ceiling(gdsm_ctx* ctx, int kind, const void* a, const void* b, void* dst,
                       uint64_t n_pages, int reps, float* best_ms, float* median_ms);

/* ---- DSM rounds on the device ------------------------------------------------------------
 * n_rounds release rounds of one DSM run, each: a coherence batch of fault events on `pt`'s page
 * table (as gdsm_coherence_batch_async, totals row r = totals + 10 r), the application's writes
 * of the round on `data` (copy descriptors as gdsm_memcpy_batch) and the release of the pages
 * written (as gdsm_release with GDSM_RELEASE_RETWIN: diff of list entries ids, applied to
 * REPLICA at home, TWIN := CURRENT), round after round. Instead of three calls per round, ONE
 * persistent launch per context: the page-table rounds on pt's stream, the page-data rounds on
 * data's stream, a device-wide barrier between rounds where the launches had their boundaries.
 * Round r = events [ev_off[r], ev_off[r+1]), list entries [id_off[r], id_off[r+1]) of ids / home,
 * descriptors [desc_off[r], desc_off[r+1]) of desc (3 u64 each). The offset arrays are HOST
 * arrays of n_rounds + 1 entries from 0 (copied to the device by the call); events, totals, ids,
 * home, desc are device pointers. A round's writes are laid onto its released pages by the
 * release itself (no separate copy step), so they must be 8-B aligned (dst, src and bytes) and lie
 * inside the pages that round releases, each page listed once per round; otherwise gdsm_sync on
 * data reports -EINVAL. One round's descriptors must not overlap each other (a word two of them
 * cover is also reported as -EINVAL by gdsm_sync). A descriptor's source must not lie in data's
 * arenas or in any memory written during the call (runs' buffers, totals): the sources are read
 * with no ordering against the call's own stores, and this is NOT checked. Limits: <= 2048 pages
 * and <= 2^20 events per round; runs sized for the largest round, in records (n_cap) and in bytes:
 * runs->cap >= (pages of the largest round) * GDSM_MAX_RECORD, else -EINVAL from the call before
 * anything runs (a round whose stream overflowed cap would leave its pages dirty unreported); data
 * and pt distinct contexts of one device. runs ends holding the last round's stream. Asynchronous on both streams; gdsm_sync on each reports failures (-ETIMEDOUT: a device
 * barrier gave up, never expected). Replaces gallocy_amd/native/replay.cpp's per-round
 * calls for config 5 (test/test_mmult.cpp:51-64's rounds). */
int gdsm_rounds(gdsm_ctx* data, gdsm_ctx* pt, uint32_t n_rounds, const uint64_t* events,
                const int64_t* ev_off, uint64_t* totals, const uint32_t* ids,
                const uint32_t* home, const int64_t* id_off, const uint64_t* desc,
                const int64_t* desc_off, gdsm_runs* runs);

/* ---- synthetic inputs (SPEC §6) ------------------------------------------------------- */
/* Fills the arenas named in `arenas` (bit 1<<GDSM_TWIN | 1<<GDSM_CURRENT | 1<<GDSM_REPLICA,
 * 0 = all) for every page; arena page i has global id first_global + i * stride (stride 0 = 1).
 * REPLICA gets the page's TWIN content. */
int gdsm_gen_pages(gdsm_ctx* ctx, uint32_t arenas, uint64_t first_global, uint64_t stride,
                   uint64_t seed, int mode, uint32_t ppm);
int gdsm_gen_pages_raw(uint8_t* twin, uint8_t* cur, uint8_t* replica, uint64_t n,
                       uint64_t first_global, uint64_t stride, uint64_t seed, int mode,
                       uint32_t ppm, void* stream);

/* ---- twin / diff / apply (SPEC §2-4) ------------------------------------------------- */
/* `ids` is a device array of n page ids, or NULL for the identity range [0, n). */
int gdsm_twin(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n);
/* Allocates a stream for n records with `cap` data bytes (cap 0: worst case n*10244). */
int gdsm_runs_alloc(gdsm_ctx* ctx, uint64_t n, uint64_t cap, gdsm_runs* out);
int gdsm_runs_free(gdsm_ctx* ctx, gdsm_runs* runs);
/* Diffs TWIN against CURRENT for the listed pages into `out` (n <= out->n_cap; out->n is set
 * to n). Asynchronous; use gdsm_runs_total to learn the size. */
int gdsm_diff(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n, gdsm_runs* out);
/* gdsm_diff, and the same runs applied to arena `target` (GDSM_REPLICA: a home copy on this
 * GPU, indexed by the same ids) by the same kernel: each dirty 16-B chunk's changed bytes, which
 * are exactly the bytes its runs cover (SPEC §4), are stored from the registers that found them,
 * so the stream is not read back. Equivalent to gdsm_diff + gdsm_apply(ctx, target, ids, out),
 * except that every page is applied even when the stream overflows out->cap (-ENOSPC from
 * gdsm_runs_total). Replaces the local-home half of gallocy's described release
 * (resources/NUTSHELL.md:59-69): the home applies what the writer diffed. */
int gdsm_diff_apply(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n, gdsm_runs* out, int target);
/* gdsm_diff_apply with the home copy indexed differently: list entry i (page ids[i] of TWIN and
 * CURRENT) is applied to page target_ids[i] of arena `target` (device, n entries; out-of-range
 * ids are reported by the next gdsm_sync and write nothing). For writers whose pages sit at other
 * indices than their home copies on the same GPU (e.g. several nodes' views of one zone, each
 * at its own offset, and one home copy of it). */
int gdsm_diff_apply_ids(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n, gdsm_runs* out,
                        int target, const uint32_t* target_ids);
/* A whole release of a writer's pages on this GPU: gdsm_diff of the listed pages into `out`;
 * with target >= 0 the runs are applied to arena `target` as gdsm_diff_apply_ids does
 * (target_ids NULL: the same page ids); with GDSM_RELEASE_RETWIN, TWIN := CURRENT afterwards for
 * every listed page whose record fit out->cap (a page whose record did not fit stays dirty, so
 * redoing the release with a larger stream ships it), i.e. the next interval's diff starts clean
 * without a gdsm_twin step. ids must be unique. A short release (<= 16 pages) is one kernel
 * launch, re-twin included. Replaces the twin taken at the next write fault
 * (resources/NUTSHELL.md:52-69: twin on the first write, diff at release). */
#define GDSM_RELEASE_RETWIN 1u
int gdsm_release(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n, gdsm_runs* out, int target,
                 const uint32_t* target_ids, uint32_t flags);
/* One diff launch for a release with several destinations: arena pages [bounds[d],
 * bounds[d+1]) are diffed into out[d] (G <= 8 streams, each with its own buffers; record i of
 * out[d] is page bounds[d] + i; out[d].n is set). Every stream is exactly what gdsm_diff of that
 * range would write, but the G ranges share one launch instead of G (gdsm_exchange's per-home
 * streams). */
int gdsm_diff_split(gdsm_ctx* ctx, const uint64_t* bounds, uint32_t G, gdsm_runs* out);
/* Synchronises, returns rec_off[n] in *total; -ENOSPC if it exceeded runs->cap. */
int gdsm_runs_total(gdsm_ctx* ctx, const gdsm_runs* runs, uint64_t* total);
/* Applies `in` to arena `target` (normally GDSM_REPLICA) for the listed pages (ids unique). */
int gdsm_apply(gdsm_ctx* ctx, int target, const uint32_t* ids, const gdsm_runs* in);
/* As gdsm_apply, on the context's second stream: it runs concurrently with the gdsm_diff calls
 * that follow (double-buffered releases: diff k+1 overlaps apply k). A later gdsm_diff into the
 * same `in` waits for this apply; every other call on the context is ordered after it.
 * Malformed records are reported by the next gdsm_sync. */
int gdsm_apply_async(gdsm_ctx* ctx, int target, const uint32_t* ids, const gdsm_runs* in);

/* ---- merge: the diff streams of several writers as one (docs/SPEC.md §8) -------------------
 * The multiple-writer step at a home (no reference counterpart: resources/NUTSHELL.md:59-69
 * describes one writer per page): K streams in[0..K), 1 <= K <= GDSM_MAX_NODES, in priority order
 * (in[k] is "applied after" in[k-1]) become the one stream `out` that gdsm_apply applies with the
 * same result, restricted to the out pages; where two writers covered the same byte is counted.
 *   in_ids[k]  (device, in[k].n entries, strictly ascending) the pages of stream k's records;
 *              NULL (or in_ids itself NULL): record i is out entry i, and in[k].n == n_out;
 *   out_ids    (device, n_out entries, strictly ascending) the pages of the out records; a stream
 *              contributes the record whose id equals the page, pages not listed here are ignored
 *              (pass the union for everything); NULL = the identity, every in_ids[k] NULL too.
 * Per out page the record's runs are the MAXIMAL ranges of the positions any stream covers (runs
 * that abut fuse), each byte from the highest k covering it; with K = 1 and a canonical input the
 * output equals the input byte for byte, and merging is associative byte for byte.
 *   conflicts  (device, n_out x u32, may be NULL) per out page, the positions covered by at least
 *              two streams that do not all carry the same byte there;
 *   stats      (device, 2 x u64, may be NULL) {overlapped bytes (covered by >= 2 streams),
 *              conflicting bytes} over all out pages.
 * Capacity as gdsm_diff: rec_off is written in full, data only below out->cap (in whole dwords),
 * gdsm_runs_total reports -ENOSPC. A record gdsm_apply would refuse contributes nothing (the out
 * record is built from the other streams) and the next gdsm_sync reports -EINVAL; input offsets
 * that do not start at 0, decrease, are not 4-aligned or end past the stream's cap, or a page list
 * that is not strictly ascending, are found before any record is read: the out stream is then
 * empty (every offset 0, no data written) and the next gdsm_sync reports -EINVAL.
 * Asynchronous on the context stream, no host synchronisation; sets out->n = n_out. Immediate
 * -EINVAL: K == 0 or > 8, a NULL ctx / in / out, n_out > out->n_cap, out sharing data or rec_off
 * with an input, in_ids[k] == NULL with in[k].n != n_out, a list with out_ids == NULL. -EBUSY on
 * a recording context whose merge workspace would have to grow (merge once before recording). */
int gdsm_merge(gdsm_ctx* ctx, uint32_t K, const gdsm_runs* in, const uint32_t* const* in_ids,
               const uint32_t* out_ids, uint64_t n_out, gdsm_runs* out, uint32_t* conflicts,
               uint64_t* stats);

/* ---- raw entry points (caller-owned device memory, e.g. tensors; stream = hipStream_t) ---- */
uint64_t gdsm_diff_workspace_bytes(uint64_t n);
int gdsm_diff_raw(const uint8_t* twin, const uint8_t* cur, const uint32_t* ids, uint64_t n,
                  uint64_t* rec_off, uint8_t* data, uint64_t cap, void* workspace,
                  uint64_t workspace_bytes, void* stream);
int gdsm_diff_apply_raw(const uint8_t* twin, const uint8_t* cur, uint8_t* target,
                        const uint32_t* ids, uint64_t n, uint64_t* rec_off, uint8_t* data,
                        uint64_t cap, void* workspace, uint64_t workspace_bytes, void* stream);
/* err: caller-owned device word, OR-ed with 1 on a malformed record (NULL: not reported). */
int gdsm_apply_raw(uint8_t* target, const uint32_t* ids, uint64_t n, const uint64_t* rec_off,
                   const uint8_t* data, uint32_t* err, void* stream);
int gdsm_twin_raw(uint8_t* twin, const uint8_t* cur, const uint32_t* ids, uint64_t n,
                  void* stream);
/* gdsm_merge on caller-owned buffers: K arrays of offsets, data, capacities, page lists (in_ids or
 * an entry NULL as above) and record counts; err as gdsm_apply_raw's (OR-ed with 1 for a malformed
 * record, 16 / 8 for malformed offsets / an unsorted list; NULL: not reported); workspace of
 * gdsm_merge_workspace_bytes(n_out) device bytes, its contents need not be kept. */
uint64_t gdsm_merge_workspace_bytes(uint64_t n_out);
int gdsm_merge_raw(uint32_t K, const uint64_t* const* rec_off, const uint8_t* const* data,
                   const uint64_t* caps, const uint32_t* const* in_ids, const uint64_t* in_n,
                   const uint32_t* out_ids, uint64_t n_out, uint64_t* out_rec_off,
                   uint8_t* out_data, uint64_t out_cap, uint32_t* conflicts, uint64_t* stats,
                   uint32_t* err, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- batched coherence (SPEC §5) ------------------------------------------------------- */
/* Allocates and initialises the page table (state + faults) for n_nodes <= 8; -EINVAL for a
 * context of more than GDSM_MAX_COH_PAGES pages. */
int gdsm_coh_init(gdsm_ctx* ctx, uint32_t n_nodes);
/* Applies one batch of page-sorted events (device array). Synchronises and writes
 * totals[10] = {invalidations, transfers, node_faults[8]}; -EINVAL if the batch is not sorted
 * by page or names a page/node out of range (the page table is then unspecified). */
int gdsm_coherence_batch(gdsm_ctx* ctx, const uint64_t* events, uint64_t n_events,
                         uint64_t* totals);
/* Asynchronous variant: totals stay on the device (10 x u64, written at the end). */
int gdsm_coherence_batch_async(gdsm_ctx* ctx, const uint64_t* events, uint64_t n_events,
                               uint64_t* totals_dev);
int gdsm_coh_download(gdsm_ctx* ctx, uint32_t* state, uint32_t* faults);
int gdsm_coh_upload(gdsm_ctx* ctx, const uint32_t* state, const uint32_t* faults);
/* Fills events from per-page counts: offsets is a device array of n+1 exclusive-scan offsets. */
int gdsm_gen_events(gdsm_ctx* ctx, uint64_t* events, const uint64_t* offsets, uint64_t first_page,
                    uint64_t n, uint64_t seed, uint32_t n_nodes, uint32_t write_pct);

/* ---- reference diff() (NW alignment), CPU ----------------------------------------------- */
/* out1/out2 are allocated with the installed allocator (default malloc); *len = alignment
 * length, which the legacy symbol cannot return. */
int gdsm_nw_diff(const char* mem1, size_t mem1_len, char** out1, const char* mem2,
                 size_t mem2_len, char** out2, size_t* len);
/* Installs the allocator used for diff()/gdsm_nw_diff outputs: gallocy passes
 * internal_malloc/internal_free so callers keep freeing with internal_free. */
int gdsm_set_allocator(void* (*alloc_fn)(size_t), void (*free_fn)(void*));

/* ---- reference diff() on the GPU: batched NW alignment --------------- */
/* Aligns n pairs (a_i, b_i) exactly like diff() / gdsm_nw_diff (same scores, tie-break and
 * traceback, gallocy/utils/diff.cpp:73-167), on the context's GPU. Device pointers: a and b hold
 * the concatenated inputs, a_off/b_off[n+1] their exclusive offsets; every |a_i|, |b_i| must be
 * <= max_len (-EINVAL otherwise). Pair i's alignment (L_i bytes + NUL) is written at
 * out1/out2 + a_off[i] + b_off[i] + i, so each output buffer needs a_off[n] + b_off[n] + n
 * bytes; out_len[i] = L_i. Synchronises (it checks the device error word). */
int gdsm_nw_diff_batch(gdsm_ctx* ctx, const uint8_t* a, const uint64_t* a_off, const uint8_t* b,
                       const uint64_t* b_off, uint64_t n, uint32_t max_len, uint8_t* out1,
                       uint8_t* out2, uint64_t* out_len);
/* Routes the legacy diff() symbol (and gdsm_nw_diff) through gdsm_nw_diff_batch on ctx when
 * mem1_len * mem2_len >= min_cells; ctx == NULL restores the CPU path (the default). Outputs
 * still come from the installed allocator. The caller keeps ctx alive while it is installed and
 * does not use it for other work meanwhile: offloaded calls stage through its stream and buffers
 * (concurrent diff() calls are serialised on an internal lock; the CPU path stays reentrant). */
int gdsm_set_diff_device(gdsm_ctx* ctx, uint64_t min_cells);

/* ---- Host write-fault capture (the step before the diff). The reference
 * describes protecting shared pages and faulting on access (resources/NUTSHELL.md:52-69,
 * resources/IMPLEMENTATION.md:246-249) but never implements it; its only mprotect use is the
 * thread-stack guard (gallocy/threads.cpp:53-58). A tracker protects a page-aligned host region
 * read-only; the first write to a page in an interval is caught by a SIGSEGV handler, which
 * copies the page to the tracker's twin and makes it writable. CPU only (no GPU needed) except
 * gdsm_track_diff. Faults outside every tracked region go to the previously installed handler. */
typedef struct gdsm_tracker gdsm_tracker;
int gdsm_track_begin(gdsm_tracker** out, void* base, uint64_t n_pages);
/* Sorted ids of the pages written since begin / the last rearm; *n_out = their count. With
 * ids == NULL only the count is returned; -ENOSPC if cap < count. */
int gdsm_track_dirty(gdsm_tracker* t, uint32_t* ids, uint64_t cap, uint64_t* n_out);
/* The twin buffer (n_pages x 4 KiB; page p valid while p is dirty): p's contents before the
 * interval's first write to it. */
int gdsm_track_twin(gdsm_tracker* t, const void** twin);
/* Write faults taken so far (all intervals). */
int gdsm_track_faults(gdsm_tracker* t, uint64_t* faults);
/* Release point: re-protects the dirty pages and empties the dirty list. No thread may write
 * the region during the call. */
int gdsm_track_rearm(gdsm_tracker* t);
/* Unprotects the region and frees the tracker once no fault handler is still inside it. Only
 * write faults are claimed by a tracker; any other fault goes to the previous handler. */
int gdsm_track_end(gdsm_tracker* t);
/* Packs the dirty pages' twin and current contents, uploads them (synchronous w.r.t. the host
 * region: it may be written again once this returns) and diffs them on the GPU into `out`, one
 * record per dirty page in id order; ids_dev (>= count entries, device) receives the sorted ids,
 * so gdsm_apply(ctx, GDSM_REPLICA, ids_dev, out) applies the interval to a replica indexed by
 * page id. *n_out = count. */
int gdsm_track_diff(gdsm_ctx* ctx, gdsm_tracker* t, gdsm_runs* out, uint32_t* ids_dev,
                    uint64_t* n_out);

/* ---- diff wire format (docs/SPEC.md §7): a diff stream as a Raft log command text --------
 * The step after the diff: gallocy replicates Command{string}
 * (gallocy/include/gallocy/consensus/log.h:18-27) inside append-entries JSON
 * (consensus/client.cpp:133-142) and applies committed entries in try_apply
 * (consensus/state.cpp:308-316). The text is "GDSM1:" + base64(frame): printable, no NUL, no
 * JSON escapes. Framing, checksum and base64 run on the GPU. */
/* Length of the command text (without its NUL) for n records carrying data_bytes. */
uint64_t gdsm_wire_size(uint64_t n, uint64_t data_bytes);
/* Encodes the stream `runs` of pages ids[0..runs->n) (device; NULL = pages 0..n-1) into `out`
 * (host, cap bytes including the NUL); *len = text length. -ENOSPC (and *len = the length
 * needed) when cap is too small. Synchronises. */
int gdsm_wire_encode(gdsm_ctx* ctx, const uint32_t* ids, const gdsm_runs* runs, char* out,
                     uint64_t cap, uint64_t* len);
/* Decodes and verifies a command text (host, len bytes, no NUL needed) into device ids_out
 * (>= n entries) and `out` (n <= out->n_cap, data <= out->cap); *n_out = n. -EINVAL for any
 * malformed text (SPEC §7), -ENOSPC when out is too small. Synchronises. */
int gdsm_wire_decode(gdsm_ctx* ctx, const char* text, uint64_t len, uint32_t* ids_out,
                     gdsm_runs* out, uint64_t* n_out);
/* Follower side of try_apply: decodes, verifies (including page ids < the arena's pages) and
 * applies the command's records to arena `target`; nothing is applied when the text is rejected
 * (-EINVAL); a malformed record inside a well-formed frame fails during the apply (SPEC §7).
 * *n_out = records applied. Synchronises. */
int gdsm_wire_apply(gdsm_ctx* ctx, int target, const char* text, uint64_t len, uint64_t* n_out);

/* ---- multi-GPU diff propagation over RCCL / xGMI -------------------------------
 * One process and one context per GPU; pages are sharded by home rank. At a release, each rank
 * diffs the pages it wrote, grouped by home rank d, into one stream per destination (send[d]);
 * gdsm_exchange ships every stream to its home and applies what arrives to the home's arena.
 * This replaces the reference's page-update transport, an HTTP POST per peer fanned out with
 * std::async (gallocy/http/client.cpp:39-91, driven by gallocy/consensus/client.cpp:15-42).
 * RCCL is bound at run time (the librccl already loaded in the process, e.g. by torch, else
 * librccl.so.1); without it gdsm_comm_* return -ENOSYS. */
typedef struct gdsm_comm gdsm_comm;
#define GDSM_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on ONE rank and hand the 128 bytes to every rank (Raft, HTTP, env). */
int gdsm_comm_unique_id(uint8_t* id);
/* Collective over the nranks processes (ncclCommInitRank on ctx's device). */
int gdsm_comm_init(gdsm_comm** out, gdsm_ctx* ctx, int nranks, int rank, const uint8_t* id);
int gdsm_comm_fini(gdsm_comm* comm);
int gdsm_comm_size(const gdsm_comm* comm, int* nranks, int* rank);
/* Test transport: nranks communicators over nranks contexts of ONE process (normally all on one
 * GPU), comms[r] bound to ctxs[r] and driven by its own host thread. Every collective below makes
 * the same calls at the same points as over RCCL; the moves become device-to-device copies on
 * the contexts' streams, ordered by HIP events (a receiver copies after the sender's stream
 * reached the send; the sender's stream continues after every receiver copied). It lets the
 * multi-rank code paths run on a one-GPU box. RCCL stays the transport of gdsm_comm_init. */
int gdsm_comm_init_loopback(gdsm_comm** comms, gdsm_ctx* const* ctxs, int nranks);
/* Collective, synchronous (after the work enqueued on ctx): *value becomes the maximum of every
 * rank's *value. The ranks' agreement on what to do next, e.g. whether to redo a release whose
 * fixed budget overflowed (-EOVERFLOW on some rank, below). */
int gdsm_comm_agree(gdsm_comm* comm, gdsm_ctx* ctx, uint64_t* value);

/* gdsm_exchange flags */
enum gdsm_exchange_flags {
  /* No host synchronisation: every record count and byte count is fixed by the caller.
   * send[d] ships exactly send[d].n records and send[d].cap data bytes (cap is the byte budget:
   * the stream's real size, rec_off[n], must not exceed it; the bytes past it are padding);
   * recv[s].n and recv[s].cap must equal what rank s ships here. A stream found larger than its
   * budget is not applied (its offsets are zeroed) and the next gdsm_sync of the home AND of the
   * sender reports -EOVERFLOW (when nothing else went wrong). Nothing of the release is lost
   * that the same release redone without the flag does not restore: gdsm_comm_agree on the
   * verdict, then re-diff and exchange with exact sizes (diff streams are idempotent). Without
   * the flag the library learns the sizes with one device all-to-all of (records, bytes) and
   * one host read, and agrees on capacity with every rank (all return -ENOSPC when any stream
   * is too small). */
  GDSM_XCHG_FIXED = 1u << 0,
  /* Measurement: before the transfer, a device-side barrier (a one-word all-to-all on the
   * exchange stream), so the transfer starts once every rank's streams are ready. With profiling
   * on, GDSM_PROF_EXCHANGE then times the RCCL group alone (the link) and
   * GDSM_PROF_EXCHANGE_WAIT the group plus the wait for the peers; without the flag both time the
   * group from when this rank's own streams are ready. */
  GDSM_XCHG_TIMED = 1u << 1,
};
/* Collective: every rank of `comm` calls it with arrays of nranks entries.
 *   send[d], send_ids[d]: this rank's stream for home rank d and, per record, the page's index
 *                         in rank d's arena `target` (device, send[d].n entries);
 *   recv[s], recv_ids[s]: where the stream from rank s lands (capacity recv[s].n_cap records,
 *                         recv[s].cap bytes; recv_ids[s] >= that many entries); recv[s].n is set.
 *                         recv[rank] / recv_ids[rank] are unused: the own stream is applied in
 *                         place from send[rank].
 * Runs on the context's second stream after everything enqueued on the main stream (the diffs
 * that produced send[]); it overlaps the gdsm_diff calls that follow, and a later gdsm_diff into
 * one of the send streams waits for it (as gdsm_apply_async). Every stream (the own one too) is
 * checked whole before it is applied: offsets from 0, non-decreasing, 4-aligned, within the
 * budget, every page index < the arena's pages; a stream failing any check is not applied at
 * all and the next gdsm_sync reports -EINVAL (-EOVERFLOW when the budget was the only fault);
 * a malformed record inside a well-formed stream is caught by the apply (SPEC §4). */
int gdsm_exchange(gdsm_ctx* ctx, gdsm_comm* comm, const gdsm_runs* send,
                  const uint32_t* const* send_ids, gdsm_runs* recv, uint32_t* const* recv_ids,
                  int target, uint32_t flags);

/* ---- coherence across GPUs (docs/SPEC.md §5b) ----------------------------------
 * Rank r of the communicator is DSM node r and the home of the page block
 * [r * per, (r+1) * per), per = ceil(total_pages / nranks) (SPEC §5's initial home); its page-table
 * context holds that block (local page = global page - base). A batch of faults is handled in two
 * collective, host-synchronising steps (every rank calls both, in this order, with its own data):
 *   1. gdsm_route_events: each node's fault events go to their pages' homes, where the sources'
 *      lists are merged into one page-sorted batch;
 *   2. gdsm_coherence_notify: each home folds its batch into its page-table shard (SPEC §5) and
 *      sends every node whose access to a page changed a notice, the "negotiate access / copy over
 *      the latest contents / update protections" step of resources/NUTSHELL.md:61-69 that the
 *      reference only describes (its transport would be gallocy/http/client.cpp:39-91).
 * The shards then equal the sequential fold of all nodes' events in (page, seq) order. */
#define GDSM_STAMP_PAGE_SHIFT 36
/* A node's fault event, stamped: (page << 36) | (seq << 4) | (node << 1) | rw, page < 2^28 the
 * GLOBAL page, seq < 2^32 the event's position in the batch's global order (a logical clock; unique
 * per page), node = the calling rank. A node's list is sorted ascending (by page, then seq). */
/* Routes this node's n stamped events (device) to the homes; on return *n_batch events of this
 * rank's home block, from every node, merged by (page, seq) and packed as SPEC §5 events with the
 * LOCAL page, are being written to `batch` (device, cap entries) on ctx's stream. All ranks return
 * -EINVAL if any node's list is unsorted or names a page >= total_pages or a node >= nranks, and
 * -ENOSPC if any home's cap is too small; nothing moves then. A rank whose own step fails after
 * the arguments were accepted (a workspace it cannot allocate, a launch error) returns that error
 * and every other rank -ECANCELED, together; nothing moves either. */
int gdsm_route_events(gdsm_ctx* ctx, gdsm_comm* comm, const uint64_t* events, uint64_t n,
                      uint64_t total_pages, uint64_t* batch, uint64_t cap, uint64_t* n_batch);
/* Home side: folds `batch` (n events, local pages, e.g. from gdsm_route_events) into ctx's page
 * table (gdsm_coh_init'd, pages [base, base + n_pages)) with its totals into totals_dev (10 x u64,
 * as gdsm_coherence_batch_async), then sends each node its notices. On return *n_notices notices
 * for THIS rank as a node, from every home, sorted by page, are being written to `notices`
 * (device, cap entries) on ctx's stream. A notice (u64) for page p and node d:
 *   bits 0-31 global page | 32-33 d's access before the batch | 34-35 d's access after |
 *   40-47 owner before | 48-55 owner after
 * with access 0 none, 1 read (d in the copyset), 2 write (EXCLUSIVE and d the owner); d gets one
 * iff its access changed or it is the old or the new owner of a page whose owner changed, so a
 * node never gets more notices than there are distinct pages in all homes' batches: every rank
 * returns -ENOSPC, before any page table changes, when some node's cap is below that count. All
 * ranks return -EINVAL if any home's batch was rejected by the fold (that page table is then
 * unspecified, as after a rejected gdsm_coherence_batch). A rank whose own step fails (a workspace
 * it cannot allocate, a launch error) returns that error and every other rank -ECANCELED,
 * together: before the fold (every workspace is sized then) no page table changes; a launch
 * failure of the fold itself leaves the page tables unspecified, as above. Only this fold's
 * rejection counts: an error bit an earlier unsynchronised batch left is kept for gdsm_sync. */
int gdsm_coherence_notify(gdsm_ctx* ctx, gdsm_comm* comm, const uint64_t* batch, uint64_t n,
                          uint64_t base, uint64_t* totals_dev, uint64_t* notices, uint64_t cap,
                          uint64_t* n_notices);

/* ---- page fetch: contents from the home copies to the nodes (docs/SPEC.md §9) ---------------
 * The other direction of a home-based DSM. gdsm_diff / gdsm_exchange / gdsm_merge take a writer's
 * changes to the page's home copy (REPLICA at the home rank); gdsm_fetch takes a page's contents
 * from its home to a node that gained access to it: the "copy over the latest contents" step of
 * resources/NUTSHELL.md:61-69, which the reference only describes (its transport would be
 * gallocy/http/client.cpp:39-91). Contents ALWAYS come from the home copy, rank p / per with per =
 * ceil(total_pages / nranks) as in §5b above: the page table's `owner` names the last writer, not
 * the holder of the data, and the last writer's release (gdsm_exchange) is what brings the home
 * copy up to date.
 *
 * Collective: every rank of `comm` calls it, also a rank that wants nothing (n = 0).
 *   pages      device, n GLOBAL page ids, strictly ascending, each < total_pages
 *              (total_pages <= GDSM_MAX_COH_PAGES);
 *   dst_ids    device, n entries: where entry i lands in THIS rank's arenas (NULL: at pages[i]);
 *              every destination < gdsm_n_pages(ctx); the destinations of one call must be
 *              distinct (with duplicates, which entry's contents stay is unspecified);
 *   src        the arena the homes serve from, normally GDSM_REPLICA; page p is page p - home * per
 *              of its home's arena, and a home's context must hold at least its block,
 *              min(total_pages, (r+1) * per) - min(total_pages, r * per) pages (possibly none);
 *   dst_arenas bit 1<<GDSM_CURRENT and/or 1<<GDSM_TWIN, 0 = both; src may not be one of them.
 * Effect: for every entry i and every arena named, arena[dst(i)] := the home copy of pages[i],
 * byte for byte. With both arenas the page arrives clean (TWIN == CURRENT: its next diff is
 * empty). No other page of any arena changes on any rank; src is only read. Pages homed at the
 * calling rank are copied arena to arena on the device: no staging buffer, no transfer.
 *
 * Runs on the context's main stream after everything enqueued on it and after pending
 * gdsm_exchange / gdsm_apply_async work (no gdsm_sync needed in between). It synchronises the host
 * (one read of the per-home counts), so on a recording context it fails with -EBUSY; the page
 * moves themselves are still being written on ctx's stream when it returns.
 *
 * Memory: the call stages whole pages in buffers the communicator keeps (they only grow): at a home
 * 4 KiB + 4 B per page it serves to OTHER ranks in this call, at a requester 4 KiB per page it asks
 * of OTHER ranks. A fetch is not chunked: size the lists accordingly.
 *
 * Refusals are collective, before anything moves: every rank returns -EINVAL if any rank's list is
 * not strictly ascending or names a page >= total_pages or a destination >= its n_pages, or if any
 * home's context is smaller than its block. A rank whose own step fails (staging it cannot
 * allocate, a launch error) returns that error and every other rank -ECANCELED, together.
 * Immediate -EINVAL (the same on every rank by construction): NULL ctx or comm, n without pages,
 * a bad src or dst_arenas, an arena the context lacks, total_pages 0 or over the limit, more than
 * 255 ranks, a comm on another device. A request id a home receives that is outside its block
 * (only a corrupted transfer can produce one) copies nothing and the home's next gdsm_sync reports
 * -EINVAL. With profiling on, GDSM_PROF_FETCH times the transfers and the page moves. */
int gdsm_fetch(gdsm_ctx* ctx, gdsm_comm* comm, const uint32_t* pages, const uint32_t* dst_ids,
               uint64_t n, uint64_t total_pages, int src, uint32_t dst_arenas);
/* From notices to a fetch list. Filters this node's n notices (device, as gdsm_coherence_notify
 * wrote them: sorted by page, at most one per page): keeps those whose access before is 0 and
 * whose access after `want` selects (bit 0: gained for reading, 0 -> 1; bit 1: gained for writing,
 * 0 -> 2) and writes their global pages to pages_out (device, cap entries) in order, so the list
 * is strictly ascending, ready for gdsm_fetch. An upgrade 1 -> 2 needs no contents and is never
 * listed. Synchronises and sets *n_out; -ENOSPC, with *n_out = the count needed, when cap is too
 * small (the first cap pages are written). ctx may be the page-table context that received the
 * notices: the list is a plain device array that the data context's gdsm_fetch then reads.
 * -EINVAL for a NULL ctx or n_out, n without notices, cap without pages_out, want outside 1..3,
 * n > GDSM_MAX_COH_PAGES; -EBUSY on a recording context. */
int gdsm_notices_fetch_list(gdsm_ctx* ctx, const uint64_t* notices, uint64_t n, uint32_t want,
                            uint32_t* pages_out, uint64_t cap, uint64_t* n_out);

/* ---- page digest (docs/SPEC.md §10) -----------------------------------------------------------
 * A page's identity in 16 bytes: two u64 (S0, S1) over its 1024 little-endian u32 words x[],
 *   S_t = sum_{i < 512} ((x[2i] + K[2i + 4t]) mod 2^32) * ((x[2i+1] + K[2i+1 + 4t]) mod 2^32) mod 2^64,
 * t = 0, 1, with the public keys K[j] = mix64(j + 1) >> 32 (SPEC §6's mix64): the NH construction of
 * UMAC with two Toeplitz-shifted key rows. It is a sum, so the bits do not depend on the reduction
 * order. Like the wire checksum (§7) it is NOT a MAC: two unrelated pages collide with probability
 * about 2^-64, a colliding pair can be constructed. Use it to learn that two copies are equal
 * without moving them (gdsm_fetch_changed below; a Raft follower's REPLICA against its leader's).
 *
 * out (device, 2n u64): (S0, S1) of page ids[i] (NULL: page i) of arena `which`. Asynchronous on the
 * context stream, no host synchronisation, no workspace (may be recorded into a graph). ids may
 * repeat. An id >= gdsm_n_pages(ctx) gets (0, 0) and the next gdsm_sync reports -EINVAL.
 * Immediate -EINVAL: NULL ctx, a bad `which`, an arena the context lacks, n without out. n == 0 is
 * a no-op. With profiling on, GDSM_PROF_DIGEST times the launch. */
int gdsm_digest(gdsm_ctx* ctx, int which, const uint32_t* ids, uint64_t n, uint64_t* out);
/* The same on a caller's arena and stream, ids unchecked (NULL: pages 0 .. n-1). */
int gdsm_digest_raw(const uint8_t* arena, const uint32_t* ids, uint64_t n, uint64_t* out,
                    void* stream);

/* ---- conditional fetch: move only the stale pages (docs/SPEC.md §11) --------------------------
 * gdsm_fetch with the question "do you already have it?" asked first. Arguments, list rules, home
 * mapping, ordering (after pending gdsm_exchange / gdsm_apply_async work, no gdsm_sync needed),
 * -EBUSY on a recording context and every immediate and collective refusal are gdsm_fetch's.
 * Postcondition on the arenas: gdsm_fetch's, provided no digest collides: every named arena at
 * dst(i) equals the home copy of pages[i], nothing else changes anywhere, src is only read.
 *
 * What travels differs. The requester's existing copy is arena A at dst(i), A = CURRENT when it is
 * named, else TWIN.
 *   entries homed at another rank: the requester sends the 4-B id and the 16-B digest of A[dst(i)];
 *     the home digests its own page and answers one u32 flag per entry plus the 4 KiB pages of the
 *     entries whose digests differ, compacted in request order. A matching entry moves no page;
 *     with both arenas named the other arena is made equal by a device-local copy of A[dst(i)], so
 *     the page still arrives clean.
 *   entries homed at the caller: compared byte for byte with the home copy on the device (exact, no
 *     digest), copied arena to arena when they differ.
 *   changed    device, n u32, may be NULL: changed[i] = 1 when entry i's contents in A were
 *              replaced, 0 when they were found equal (exactly for local entries, by digest for
 *              remote ones);
 *   stats      device, 4 u64, may be NULL, over this rank's list: [0] remote entries transferred,
 *              [1] remote entries skipped, [2] local entries that differed, [3] local entries found
 *              equal. Written (zeroed, then counted) only when the call is not refused.
 * Sending only what changed costs a second host synchronisation: the homes' changed counts go
 * all-to-all and are read back before the pages move (gdsm_fetch reads the host once).
 * Memory: the staging buffers of gdsm_fetch, sized for the worst case (every page changed) plus
 * about 32 B per served request at a home and per remote entry at a requester. */
int gdsm_fetch_changed(gdsm_ctx* ctx, gdsm_comm* comm, const uint32_t* pages,
                       const uint32_t* dst_ids, uint64_t n, uint64_t total_pages, int src,
                       uint32_t dst_arenas, uint32_t* changed, uint64_t* stats);

/* ---- dirty scan: which pages did this interval change? (docs/SPEC.md §12) --------------------
 * The device counterpart of gdsm_track_dirty, for a writer that takes no faults (a kernel storing
 * into CURRENT): the list of pages that gdsm_diff / gdsm_release / gdsm_exchange / gdsm_merge take
 * from their caller, made by comparing two arenas of the context.
 *   a, b       two different arena kinds the context holds; the usual pair is GDSM_TWIN,
 *              GDSM_CURRENT (GDSM_REPLICA, GDSM_CURRENT: "which pages differ from my home copy");
 *   ids        device, n page ids, or NULL for pages 0 .. n-1; need not be sorted, may repeat, each
 *              entry is judged on its own;
 *   pages_out  device, cap u32, may be NULL: the pages of the dirty entries, in list order (a
 *              stable compaction: strictly ascending when the list is, or with no list);
 *   pos_out    device, cap u32, may be NULL: the list positions i of the same entries (to gather
 *              gdsm_release's target_ids);
 *   stats      device, 2 u64, may be NULL: [0] the number of dirty entries, also when it exceeds
 *              cap (then only the first cap are written and nothing at or past [cap]); [1] an upper
 *              bound of rec_off[count] of the diff (a -> b) of the dirty entries, the sum over them
 *              of min(10244, 4 + 48 C), C = the 16-B chunks of the page in which a and b differ:
 *              the capacity to give gdsm_runs_alloc in place of count x 10244.
 * Entry i is dirty iff page ids[i] of a and of b differ in at least one byte. cap == 0 with both
 * outputs NULL is the count-only form. An id >= gdsm_n_pages(ctx) is not dirty, contributes nothing
 * and the next gdsm_sync reports -EINVAL. Both arenas are only read. n == 0 writes stats = {0, 0}
 * and nothing else.
 * Asynchronous on the context's stream, no host synchronisation: read stats after gdsm_sync. The
 * workspace (at most 1 B per entry plus a constant) is the context's and only grows; a recording
 * context that would have to grow it gets -EBUSY (scan once before recording, as gdsm_merge),
 * otherwise the call can be recorded, and a replay reads the arenas again. Not timed by a
 * gdsm_prof_stage.
 * Immediate -EINVAL: NULL ctx, a == b, a bad kind, an arena the context lacks, n > 2^32, cap > 0
 * with both outputs NULL. */
int gdsm_dirty_scan(gdsm_ctx* ctx, int a, int b, const uint32_t* ids, uint64_t n,
                    uint32_t* pages_out, uint32_t* pos_out, uint64_t cap, uint64_t* stats);
/* The same on a caller's arenas, workspace (8-byte aligned, at least
 * gdsm_dirty_scan_workspace_bytes(n) device bytes, contents need not be kept) and stream; ids are
 * not checked. -EINVAL also for a NULL arena and a workspace that is NULL, misaligned or too small. */
uint64_t gdsm_dirty_scan_workspace_bytes(uint64_t n);
int gdsm_dirty_scan_raw(const uint8_t* a, const uint8_t* b, const uint32_t* ids, uint64_t n,
                        uint32_t* pages_out, uint32_t* pos_out, uint64_t cap, uint64_t* stats,
                        void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- stream split: one diff stream into one per destination (docs/SPEC.md §13) ---------------
 * The joint between a stream and the calls that want one stream per destination: gdsm_exchange's
 * send[] (a sparse release: gdsm_dirty_scan -> gdsm_diff of the list -> split by home -> exchange)
 * and a home forwarding a merged stream to the nodes that hold copies of its pages. A stable
 * multi-way partition of the n = in->n records of `in`; records are opaque here (copied byte for
 * byte, not validated: the apply at the destination does that as usual).
 *   ids      device, n u32: the page of record i; NULL = page i;
 *   out      HOST array of G streams, 1 <= G <= GDSM_MAX_NODES, each with its own buffers;
 *   out_ids  HOST array of G device arrays, out_ids[d] of at least out[d].n_cap entries: the pages
 *            of out[d]'s records. The array or single entries may be NULL (not written).
 * Mask form (dest != NULL, per == 0): dest is a device array of n u32; record i goes to every
 * out[d] with bit d of dest[i] set (0: nowhere; several bits: several copies); the page written is
 * ids[i]. Home form (dest == NULL, per > 0): record i goes to d = ids[i] / per only and the page
 * written is ids[i] - d * per, the REPLICA index at home d of SPEC §5b / §9, so out[] and out_ids[]
 * are gdsm_exchange's send[] and send_ids[] as they stand. With GDSM_SPLIT_DROP_EMPTY a 0-byte
 * record goes nowhere in either form.
 * Result: record j of out[d] is the j-th selected record in input order, equal to it byte for byte;
 * rec_off[0 .. c_d] of out[d] is written from 0; ascending input ids give ascending ids in every
 * output (an output can be one of gdsm_merge's inputs); in the home form with ascending ids and no
 * flag the outputs' data concatenated in d order is the input's data.
 * Runs on the context stream after what was enqueued, synchronises once at the end (one host read
 * of the counts, as gdsm_notices_fetch_list) and sets out[d].n = c_d. counts: HOST array of 2G u64,
 * {records, bytes} per destination, may be NULL.
 *   -ENOSPC  some c_d > out[d].n_cap or b_d > out[d].cap: counts holds what is needed, every
 *            out[d].n is 0, no buffer was written at or past its capacity;
 *   -EINVAL  the input offsets do not start at 0, decrease, are not 4-aligned or end past in->cap
 *            (checked before any record is read, as the merge does), a mask has a bit >= G, or a
 *            page's home is >= G: nothing is written to any output's data, every out[d].n is 0 and
 *            the counts are 0. Only this call's own checks decide its return: an error bit an
 *            earlier unsynchronised call left stays for gdsm_sync (as gdsm_coherence_notify);
 *   -EBUSY   on a recording context.
 * Immediate -EINVAL: NULL ctx, in or out; G of 0 or more than 8; both or neither of dest and per;
 * unknown flags; n > 2^32; an output sharing data or rec_off with the input or with another output;
 * a data pointer (the input's or an output's) that is not 4-byte aligned: records move in dwords
 * (16-byte aligned buffers, as gdsm_runs_alloc makes them, take the 16-byte loads).
 * n == 0 writes rec_off[0] = 0 of every output and zero counts. The workspace is the context's and
 * only grows. Not timed by a gdsm_prof_stage. */
#define GDSM_SPLIT_DROP_EMPTY 1u
int gdsm_runs_split(gdsm_ctx* ctx, const gdsm_runs* in, const uint32_t* ids,
                    const uint32_t* dest, uint64_t per, uint32_t G, gdsm_runs* out,
                    uint32_t* const* out_ids, uint64_t* counts, uint32_t flags);
/* The same result on caller-owned memory, asynchronous on `stream` with no host synchronisation.
 * counts is a DEVICE array of 2G u64 and always holds the true values (0 when the input is
 * refused). Writes are guarded on the device: out_rec_off[d][j] only for j <= out_n_caps[d],
 * out_ids[d][j] for j < out_n_caps[d], data only below out_caps[d], in whole dwords. err (device
 * word, NULL: not reported) is OR-ed with 16 for malformed offsets and with 8 for a destination out
 * of range; in either case no output data is written. workspace: 8-byte aligned, at least
 * gdsm_runs_split_workspace_bytes(n, G) device bytes, contents need not be kept; -EINVAL for one
 * that is NULL, misaligned or short, and for NULL counts. */
uint64_t gdsm_runs_split_workspace_bytes(uint64_t n, uint32_t G);
int gdsm_runs_split_raw(const uint64_t* rec_off, const uint8_t* data, uint64_t cap,
                        const uint32_t* ids, const uint32_t* dest, uint64_t per, uint64_t n,
                        uint32_t G, uint64_t* const* out_rec_off, uint8_t* const* out_data,
                        const uint64_t* out_caps, const uint64_t* out_n_caps,
                        uint32_t* const* out_ids, uint64_t* counts, uint32_t* err,
                        uint32_t flags, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- page-table sweeps: a node leaves; questions to the table (docs/SPEC.md §14) --------------
 * Two passes over the page table of gdsm_coh_init that need no event batch and no download. Both
 * work on table pages [first, first + n) and report page `base + p`, base = the shard's first
 * global page as in gdsm_coherence_notify. The word layout is SPEC §5's (copyset bits 0-7, owner
 * 8-15, state 16-17, dirty 18); `faults` is never touched.
 *
 * gdsm_coh_retire: node `node` leaves (a committed Raft configuration change). Per page p with word
 * (c, o, s, d):
 *   s == INVALID   unchanged, nothing counted;
 *   c1 = c & ~bit(node); `held` counts the pages with c != c1;
 *   o != node      the word becomes (c1, o, s, d): the state is kept (SHARED with only the owner
 *                  left is legal; the §5 rules treat it conservatively);
 *   o == node      the new owner is o' = heir(p): h = per ? (base + p) / per : heir, and h = heir
 *                  when h >= n_nodes or h == node (§5's home where that home survives: a home
 *                  always holds the home copy, which is why it may enter the copyset);
 *                  c' = c1 | bit(o'), s' = EXCLUSIVE if c' == bit(o') else SHARED, d kept; `moved`
 *                  counts it, and `orphaned` too when s == EXCLUSIVE and d is set: `node` held the
 *                  only copy and had written it, so what it had not released is gone and the home
 *                  copy is the newest that survives.
 *   stats      device, 3 u64, may be NULL: {held, moved, orphaned};
 *   moved_out  device, cap u32, may be NULL: (base + p) | orphaned << 31 per moved page, ascending.
 * With GDSM_RETIRE_DRY the table is left as it is; stats and moved_out are what the wet call would
 * give. Retiring is idempotent (a second call changes nothing and counts {0, 0, 0}), keeps
 * "owner in copyset" and "EXCLUSIVE => copyset == {owner}" where they held, leaves `node` in no
 * copyset and owning nothing, and is not a ban: later events of `node` are ordinary events, which
 * is how a node rejoins.
 *
 * gdsm_coh_select: the pages p of the range with (word & mask) == value, as base + p, ascending,
 * into pages_out (device, cap u32, may be NULL), and their number into count (device, 1 u64, may be
 * NULL). mask 1 << d, value 1 << d: the pages node d holds, a valid list for gdsm_fetch.
 *
 * Capacity: the counts are always the true ones; only the first cap list entries are written and
 * nothing at or past [cap]; a wet retire updates the whole range whatever cap is. A caller who
 * cannot size cap = n runs GDSM_RETIRE_DRY (or a count-only select) first to learn the count.
 * cap == 0 with a NULL list is the count-only form. n == 0 writes zero counts and nothing else.
 * Asynchronous on the context's stream, after what was enqueued and after pending async applies;
 * no host synchronisation: read stats / count after gdsm_sync. The workspace is the context's and
 * only grows; a recording context that would have to grow it gets -EBUSY (sweep once before
 * recording), otherwise the call can be recorded. Not timed by a gdsm_prof_stage.
 * Immediate -EINVAL: NULL ctx; no page table (gdsm_coh_init not called); node or heir >= n_nodes;
 * heir == node; unknown flags; first + n > gdsm_n_pages; base + first + n > GDSM_MAX_COH_PAGES (bit
 * 31 stays free); cap > 0 with a NULL list. */
#define GDSM_RETIRE_DRY 1u /* compute stats and moved_out, leave the table as it is */
int gdsm_coh_retire(gdsm_ctx* ctx, uint32_t node, uint32_t heir, uint64_t base, uint64_t per,
                    uint64_t first, uint64_t n, uint32_t* moved_out, uint64_t cap,
                    uint64_t* stats /* device, 3 u64, may be NULL */, uint32_t flags);
int gdsm_coh_select(gdsm_ctx* ctx, uint32_t mask, uint32_t value, uint64_t base,
                    uint64_t first, uint64_t n, uint32_t* pages_out, uint64_t cap,
                    uint64_t* count /* device, 1 u64, may be NULL */);

/* ---- the page table by page list: clean after a release, look fields up (docs/SPEC.md §15) ----
 * Where the sweeps take a range of the table, these two take a device list of page ids, the form
 * every other call speaks in (gdsm_release, gdsm_dirty_scan, gdsm_exchange's send_ids / recv_ids,
 * gdsm_fetch). ids[i] is a GLOBAL page; entry i works on table page p = ids[i] - base, base = the
 * shard's first global page as in the sweeps (0 for recv_ids / send_ids, which are local). ids ==
 * NULL means table pages 0 .. n-1. The list needs no order, only 4-byte alignment, and may repeat
 * pages. The word layout is SPEC §5's; bits 19-31 of a word and `faults` are never written.
 *
 * gdsm_coh_clean: a release of `node` reached the home, so the dirty bit of the pages it shipped is
 * cleared. Per entry, with word (c, o, s, d) of page p:
 *   status 0 CLEANED  s != INVALID, o == node, d == 1: d := 0, nothing else in the word changes
 *                     (state and copyset kept);                                   stats[0]
 *   status 1 ALREADY  s != INVALID, o == node, d == 0: no effect;                 stats[1]
 *   status 2 STALE    s != INVALID, o != node: no effect (somebody wrote the page after `node`
 *                     did; that writer's own release will clean it);              stats[2]
 *   status 3 SKIPPED  s == INVALID: no effect;                                    stats[3]
 *   status 4 SKIPPED  ids[i] < base or p >= gdsm_n_pages: no effect, and the next gdsm_sync
 *                     reports -EINVAL (as gdsm_digest does for such an id);       stats[3]
 *   status_out  device, n bytes, may be NULL: the status of entry i;
 *   stats       device, 4 u64, may be NULL: {cleaned, already, stale, skipped}; they sum to n. The
 *               call zeroes and then counts them itself. n == 0 writes four zeros and nothing else.
 * A page listed more than once is cleaned, and counted as cleaned, exactly once; its other entries
 * report ALREADY, and which entry reports CLEANED is unspecified. The call is idempotent, keeps
 * every invariant the sweeps keep, leaves a valid input of the SPEC §5 fold, and a later write
 * event sets the bit again. After cleaning the list that gdsm_coh_select(owns dirty, d) returned,
 * with node = d, that select returns nothing and gdsm_coh_retire(d) reports orphaned == 0.
 *
 * gdsm_coh_lookup: out[i] = (s == INVALID) ? 0 : (word >> shift) & mask, and, where faults_out is
 * given, faults_out[i] = faults[p]. An id out of range gives 0 / 0 and the next gdsm_sync reports
 * -EINVAL. shift 0, mask 0xFF & ~bit(writer) & ~bit(home): the `dest` array of gdsm_runs_split's
 * mask form as it stands (the copyset of each record's page, without the two nodes that have the
 * bytes already); shift 8, mask 0xFF: the owners; shift 0, mask ~0u: the words. The table is only
 * read.
 *
 * Both are asynchronous on the context's stream, after what was enqueued and after pending async
 * applies; no host synchronisation and no workspace, so both can always be recorded, and a replay
 * reads the table and the list again. Read stats, status_out and out after gdsm_sync. Where the
 * page table lives in a context of its own, synchronise the data context that produced the list
 * (gdsm_sync, or an event the table's stream waits for) before the call: the two streams are not
 * ordered otherwise. Not timed by a gdsm_prof_stage.
 * Immediate -EINVAL: NULL ctx; no page table (gdsm_coh_init not called); node >= n_nodes; flags
 * != 0; shift > 31; n > 2^32; base > GDSM_MAX_COH_PAGES; ids == NULL with n > gdsm_n_pages;
 * n > 0 on a table of 0 pages; n > 0 with a NULL out (lookup). */
int gdsm_coh_clean(gdsm_ctx* ctx, uint32_t node, const uint32_t* ids, uint64_t n, uint64_t base,
                   uint8_t* status_out /* device, n bytes, may be NULL */,
                   uint64_t* stats /* device, 4 u64, may be NULL */, uint32_t flags /* 0 */);
int gdsm_coh_lookup(gdsm_ctx* ctx, const uint32_t* ids, uint64_t n, uint64_t base,
                    uint32_t shift, uint32_t mask, uint32_t* out /* device, n u32 */,
                    uint32_t* faults_out /* device, n u32, may be NULL */);

const char* gdsm_version(void);
/* Process-wide knobs that choose a kernel variant or launch form, for measurement and tests (every
 * value produces the same results). Key, accepted values, (default):
 *   "diff_variant"   0..8 (0)    diff geometry
 *   "apply_variant"  0..8 (0)    apply geometry
 *   "diff_solo_max"  0..16 (0)   short lists: pages up to which the one-workgroup form is taken
 *   "diff_chain"     0..4 (2)    short lists: the chained (zero-free) form
 *   "coh_variant"    0..2 (0)    automatic / streaming fold / single-pass fold
 *   "coh_chain"      0|1 (1)     small coherence batches without the zeroing launch
 *   "coh_span"       1|2|4 (4)   their span, in 64-event chunks
 *   "rounds_xcd"     -1|0|1 (-1) gdsm_rounds: automatic / the whole grid / a one-XCD team
 *   "rounds_lds"     -1|0|1 (-1) gdsm_rounds' page-table side: automatic / the persistent grid /
 *                                LDS slices (1 where they do not fit: gdsm_rounds returns -EINVAL)
 *   "rounds_lds_wg"  0..16 (0)   workgroups of the LDS form, 0 = automatic
 * Each key is also the environment variable GDSM_<KEY> (upper case), read once when the library
 * loads; a value that is not accepted there leaves the default. Returns 0, or -EINVAL for an
 * unknown key or a value that is not accepted. */
int gdsm_tune(const char* key, int64_t value);
/* Test hook: the nth next growth of one of ctx's internal workspaces fails with -ENOMEM (0 = off).
 * Used to show that a collective call refuses on every rank together when one rank fails. */
int gdsm_debug_fail_alloc(gdsm_ctx* ctx, int nth);
/* Test hook: the geometry the calling thread's last diff launch took (gdsm_diff, gdsm_diff_apply*,
 * gdsm_release, gdsm_diff_split, gdsm_diff_raw, ...): variant | form << 8, the variant 1 .. 8 as
 * the "diff_variant" key counts them (the one the automatic choice resolved to), the form 0 = the
 * grid with its zeroing launch, 1 = one workgroup, 2 = chained, a page per workgroup, 3 = chained,
 * a page per wave. 0 before any diff launch on this thread. */
int gdsm_debug_last_diff_variant(void);

#ifdef __cplusplus
}  /* extern "C" */

/* Legacy drop-in, C++ linkage, mangled _Z4diffPKcmRPcS0_mS2_ exactly like
 * gallocy/include/gallocy/utils/diff.h:9-11. Bit-exact with the reference for
 * mem1_len, mem2_len <= 1180 (the reference crashes beyond). Always returns 0. */
int diff(const char* mem1, size_t mem1_len, char*& mem1_alignment, const char* mem2,
         size_t mem2_len, char*& mem2_alignment);
#endif

#endif /* GDSM_H_ */
