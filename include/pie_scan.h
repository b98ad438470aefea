/*
 * pie_scan.h — C ABI of the MI355X session-scan -> per-user feed path (libpie_hip.so).
 *
 * The reference (sphereisaiahmin-dev/sph-pie) is a pure Node.js app with no FFI seam; the seams this ABI
 * sits behind are the CommonJS exports of three modules and one HTTP route.  Each entry
 * point below names the reference interface it replaces (paths relative to /root/reference).  The Node
 * binding (raw N-API, sph-pie_amd/csrc/pie_napi.c) and the ctypes binding (sph-pie_amd/binding.py) wrap
 * exactly these symbols; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions: plain pointers and sizes, caller-owned host buffers, no exceptions across the boundary,
 * int status return (0 = ok, negative = PIE_E_*), text of the last failure via pie_last_error().
 * A context is bound to one GPU and is used from one host thread at a time (the reference is a
 * single-threaded event loop: server/index.js, no worker threads).  There is NO CPU fallback: without a
 * HIP device pie_ctx_create() fails with PIE_E_NODEVICE.
 */
#ifndef PIE_SCAN_H
#define PIE_SCAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIE_ABI_VERSION 1

enum {
    PIE_OK = 0,
    PIE_E_INVAL = -1,    /* bad argument (null pointer, negative size, n >= 2^31, user id out of range) */
    PIE_E_NODEVICE = -2, /* no HIP device / HIP runtime error at init */
    PIE_E_HIP = -3,      /* HIP runtime error during the call; see pie_last_error() */
    PIE_E_NOMEM = -4,    /* device or host allocation failed */
    PIE_E_CAPACITY = -5, /* caller buffer too small (idx_cap < M): *m_out holds the needed size */
    PIE_E_STATE = -6     /* call out of order (scan before load, fetch before scan, ...) */
};

/* synthetic-corpus flags; identical meaning in oracle/pie_oracle.h */
#define PIE_GEN_INTERVAL  1u /* end = start + uniform[15 min, 12 h]; default end = start + SESSION_TTL_MS */
#define PIE_GEN_CLUSTERED 2u /* rows of one user contiguous; default uniform random users */
#define PIE_GEN_TIME_ORDERED 4u /* rows in order of creation (start ascending with the row index), as a session store appends
                                   them: the live rows sit together at the end of the table; default random order */

/* sentinel for "no end" (calendarFeed.js:74 endTs === null) and for tombstoned rows: never live */
#define PIE_END_NONE INT64_MIN

typedef struct pie_ctx pie_ctx;

typedef struct pie_stats {
    uint32_t struct_size;  /* set by caller to sizeof(pie_stats) */
    uint32_t n_profiled;   /* scans whose events were resolved into the sums below */
    uint64_t rows;         /* N of the resident table */
    uint64_t users;        /* U */
    uint64_t selected;     /* M of the last scan */
    uint64_t alg_bytes;    /* 24 * N: algorithmic bytes of one scan */
    double k1_ms_sum;      /* sum of predicate+compaction kernel durations (HIP events, scan stream) */
    double scan_ms_sum;    /* sum of first-kernel-start -> last-kernel-end durations */
    uint32_t max_bucket;   /* largest per-user bucket of the last scan */
    uint32_t n_segments;   /* block-sorted segments of the last scan */
    uint32_t n_big;        /* buckets that needed the multi-pass merge in the last scan */
    uint32_t k1_blocks;    /* grid of the scan kernel */
    uint32_t k1_variant;   /* form of the scan kernel used by the last scan (bit0 nt loads, bit1 late user, bit2 liveness-first,
                              0x400 keyed: streams the 2-byte liveness key instead of the `end` column, 0x800 the 1-byte key,
                              0x1000 batched: the last finished call was a batch, `selected` sums its queries, `max_bucket` is the
                              largest UNION bucket,
                              0x2000 ordered run: 0x2003 dense form, 0x2400 / 0x2C00 keyed form on the 2- / 1-byte key,
                              0x3400 / 0x3C00 a batch on the ordered run) */
    uint32_t key_ambiguous; /* keyed form: rows of the last scan whose key equalled the query's and needed the full compare (saturating) */
    uint64_t live;         /* rows with end > now seen by the last scan */
    uint64_t candidates;   /* keyed form: rows whose key was >= the query's, i.e. payload records the table pass gathered */
    /* fields below were added with the bucket-order route counters: a caller that sets struct_size to the size without them gets
       the rest.  They describe the last single scan answered by the general path (0 after a batch, an ordered-run scan or the
       partitioned path). */
    uint32_t n_small;      /* buckets of 17..512 rows (and the 1..16-row buckets of hot users): ordered by one wave each */
    uint32_t n_over;       /* listed buckets with staged records: outgrew the direct slots, belong to a hot user, or no slots exist */
    uint32_t n_hot;        /* users the scan reported for the next scan's hot set (bucket > 1/256 of the previous M), at most 32 */
    uint32_t direct_shift; /* log2 of the direct-slot capacity per user the scan ran with (4 .. 9; 0: no direct slots) */
} pie_stats;

/* ---- lifecycle ------------------------------------------------------------------------------------- */
int pie_abi_version(void);
int pie_device_count(void);
/* One context per GPU, one process per GPU.  device_id is the HIP ordinal. */
int pie_ctx_create(int device_id, pie_ctx **ctx_out);
int pie_ctx_destroy(pie_ctx *ctx);
/* ctx may be NULL: returns the last error of a failed pie_ctx_create on this thread. */
const char *pie_last_error(const pie_ctx *ctx);
/* Run the scan's main-stream kernels (K1, K2) on a caller stream (a hipStream_t, e.g. torch's current stream).
 * NULL = ctx-owned stream. */
int pie_ctx_set_stream(pie_ctx *ctx, void *hip_stream);
/* The stream on which scan results are produced and on which every result copy / pack is enqueued (today the
 * context's one stream).  A caller that consumes results on another stream records an event here
 * (e.g. torch.cuda.ExternalStream(ptr)). */
int pie_ctx_aux_stream(pie_ctx *ctx, void **hip_stream_out);

/* ---- session table: replaces the in-process `sessions` Map (server/sessionStore.js:6,17) -------------
 * Columns are SoA: start = createdAt, end = expiresAt (int64 ms), user = dense index of the userId string,
 * disc = index into DISCIPLINES (server/disciplineConfig.js:35).  Host arrays stay caller-owned. */
int pie_load_columns(pie_ctx *ctx, const int64_t *start, const int64_t *end, const int32_t *user,
                     const int32_t *disc, size_t n, int32_t n_users);
/* createSession (server/sessionStore.js:12-19): append k rows behind the resident ones (device capacity grows
 * geometrically).  n_users may grow, never shrink. */
int pie_append_rows(pie_ctx *ctx, const int64_t *start, const int64_t *end, const int32_t *user, const int32_t *disc,
                    size_t k, int32_t n_users);
/* Fill the table on the device with rows [row0, row0+n) of the deterministic synthetic corpus. */
int pie_gen_synthetic(pie_ctx *ctx, uint64_t seed, int64_t n_total, int64_t row0, int64_t n, int32_t n_users,
                      int32_t n_disc, uint32_t flags);
/* Same corpus with skewed users (the "Zipf(1.1)" variant of SURVEY.md §8d): user = first k with r0 < cdf[k], cdf =
 * n_users ascending 64-bit thresholds floor(CDF_k * 2^64) computed by the caller. */
int pie_gen_synthetic_cdf(pie_ctx *ctx, uint64_t seed, int64_t n_total, int64_t row0, int64_t n, int32_t n_users,
                          int32_t n_disc, uint32_t flags, const uint64_t *cdf);
/* Flat column files: <dir>/{start.i64,end.i64,user.i32,disc.i32} + header.json; the table survives a
 * restart (the reference keeps sessions in memory only, server/sessionStore.js:6).  Load mmaps the files and uploads. */
int pie_save_columns(pie_ctx *ctx, const char *dir);
int pie_load_columns_dir(pie_ctx *ctx, const char *dir);
/* Copy the resident columns back (any pointer may be NULL). */
int pie_read_columns(pie_ctx *ctx, int64_t *start, int64_t *end, int32_t *user, int32_t *disc, size_t n);
/* touchSession (server/sessionStore.js:37-45): end[row] = new_end.  deleteSession (:47-53): new_end = PIE_END_NONE.
 * A call that names a row more than once behaves as its elements applied in array order, as two touches or deletes of one token
 * run one after the other in the reference: the last occurrence's value is the row's `end`, and every derived structure (both
 * liveness keys, the hot index, the ordered run) agrees with that value.  The repeats are resolved on the host before the
 * rows are staged (scratch sized by k, never by the table); the call stays queued and un-waited where it was.
 * Finished results under a later mutation: pie_set_end / pie_shard_set_end leave the results of a finished scan or batch as
 * they were: every reader (pie_read_results, pie_read_user_feed, pie_batch_read_results, pie_batch_read_user_feed, the union
 * readers, the device pointers) keeps answering for the table as the scan saw it; only the `end` column that
 * pie_batch_fetch_requests returns beside the rows is the table's own, read when it is called.  pie_append_rows /
 * pie_shard_append_rows that add a row or a user to the context end them: until the next finish every reader of a scan's or a
 * batch's result returns PIE_E_STATE. */
int pie_set_end(pie_ctx *ctx, const int32_t *rows, const int64_t *new_end, size_t k);
/* Host only, no context, no GPU: the reduction pie_set_end applies to its call.  keep_out[i] = 1 iff element i is the last
 * occurrence of rows[i] in rows[0, k), else 0 (any int32 is a row here; k = 0 is allowed).  For tests. */
int pie_set_end_last_writers(const int32_t *rows, size_t k, uint8_t *keep_out);
/* deleteSessionsForUser (server/sessionStore.js:55-64): tombstone every live row with user == u (strict match;
 * unknown ids are a no-op like the falsy-id guard :56-58).  rows_out (may be NULL) receives the tombstoned row
 * indices in ascending order so the host can drop their token-map entries; *n_deleted their number. */
int pie_delete_user(pie_ctx *ctx, int32_t user, int32_t *rows_out, size_t cap, size_t *n_deleted);
/* deleteSessionsForUser for a whole set of users in one call: afterwards the table and everything derived from it (both liveness
 * keys, the payload column, the hot index and its delta, the ordered run's mirror, what the token index sees as live) are what
 * k calls pie_delete_user(ctx, users[i], ...) in array order would have left, after two passes over the user column whatever k
 * is (membership is a bit test in a bitmap of n_users bits; `end` is read only for rows whose user is in the set) and at most
 * two waits.  rows_out (may be NULL) receives ALL tombstoned rows in ascending row order, the sorted union of the k single
 * lists, *n_deleted their number; a cap too small tombstones the rows all the same, fills *n_deleted and per_user_out and
 * returns PIE_E_CAPACITY.  per_user_out[i] (may be NULL) = rows tombstoned for users[i]: an id named more than once has its
 * count at its FIRST occurrence and 0 at the later ones (the second of two deleteSessionsForUser calls finds nothing), ids < 0
 * or >= n_users have 0 and are a no-op; the counts add up to *n_deleted.  k = 0: PIE_OK, nothing changes.  users = NULL with
 * k > 0: PIE_E_INVAL.  PIE_E_STATE while a scan or batch is in flight (nothing changes).  Queued appends and touches are
 * ordered in front; slot 0's finished result and the held queue go as under pie_delete_user. */
int pie_delete_users(pie_ctx *ctx, const int32_t *users, size_t k, int32_t *rows_out, size_t cap, size_t *n_deleted,
                     int32_t *per_user_out /* [k] */);
/* Host only, no context, no GPU: what pie_delete_users uploads.  bits_out[(n_users + 63) / 64] = membership bitmap of the valid
 * ids (0 <= id < n_users; bit id % 64 of word id / 64; bits at and above n_users are 0), first_out[i] = 1 iff users[i] is valid
 * and is the first occurrence of its value, else 0.  k = 0 and n_users <= 0 are allowed.  For tests. */
int pie_delete_users_plan(const int32_t *users, size_t k, int32_t n_users, uint64_t *bits_out, uint8_t *first_out /* [k] */);

/* _pruneCalendarEvents (server/storage/sqlProvider.js:956-968): tombstone every row with start < cutoff (the
 * complement of the scan's window predicate); rows_out / n_pruned as in pie_delete_user. */
int pie_prune_before(pie_ctx *ctx, int64_t cutoff, int32_t *rows_out, size_t cap, size_t *n_pruned);

/* Retention purge with calendar-month arithmetic (server/storage/sqlProvider.js:863-890 _purgeExpiredArchives, :991-1009
 * _isArchiveExpired / _addMonths; ARCHIVE_RETENTION_MONTHS = 2, :10): tombstone every row with
 * now >= addMonths(start, months), where addMonths is JS `setMonth(getMonth() + months)` on a local-time Date (day
 * overflow rolls into the next month) and local time = UTC + tz_offset_ms (a fixed offset of whole minutes; zones with
 * daylight saving: pie_retention_purge_tz).  rows_out / n_purged as in pie_delete_user. */
int pie_retention_purge(pie_ctx *ctx, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t *rows_out, size_t cap,
                        size_t *n_purged);
/* The same under a REAL time zone (the reference's Date is local: daylight saving moves the result by the hour the clocks
 * move).  The zone travels as the transition table the host builds from its own zone rules (sph-pie_amd/host/tzTable.js,
 * binding.tz_table): offsets_ms[0] applies before transitions_utc_ms[0], offsets_ms[i + 1] from transitions_utc_ms[i] on
 * (n_transitions + 1 offsets; local = UTC + offset).  The device follows ECMA-262 exactly: offset in force at the UTC instant,
 * month shift on the local fields, and a resulting local time that is skipped or repeated at a transition is read with the
 * offset before the transition.  Instants outside the table's span use its first / last offset.  n_transitions = 0 is the
 * fixed-offset form.  Pinned by tests/golden/addmonths_zones.json (JS engine vectors under seven zones). */
int pie_retention_purge_tz(pie_ctx *ctx, int64_t now, int32_t months, const int64_t *transitions_utc_ms, const int64_t *offsets_ms,
                           int32_t n_transitions, int32_t *rows_out, size_t cap, size_t *n_purged);

/* ---- discipline predicate table: replaces findDiscipline() lookups (server/disciplineConfig.js:88-97) -
 * bit d of mask = rows of discipline d are wanted; bits >= n_disc are ignored. n_disc <= 64. */
int pie_set_disciplines(pie_ctx *ctx, uint64_t mask, int32_t n_disc);

/* ---- the scan: replaces the per-request loops (server/sessionStore.js:59-63,68-72;
 * server/storage/sqlProvider.js:284 window filter, :276 ORDER BY start_ts ASC) -------------------------
 * Row i is selected iff end[i] > now && start[i] >= cutoff && bit(mask, disc[i]).  Feed(u) = selected rows
 * of user u ordered by (start asc, row index asc).  Outputs: counts[U], offsets[U+1], idx[M]. */
int pie_scan(pie_ctx *ctx, int64_t now, int64_t cutoff, int32_t *counts_out, int64_t *offsets_out,
             int32_t *idx_out, size_t idx_cap, size_t *m_out);
/* Same scan, results left in device memory (for the multi-GPU gather and for benchmarking). */
int pie_scan_device(pie_ctx *ctx, int64_t now, int64_t cutoff, size_t *m_out);
/* The same scan in two halves for callers that overlap host work with it: begin enqueues the table pass and returns at
 * once; finish waits for the scan's summary (M), enqueues what is left (scatter + order of buckets that outgrew their
 * direct slots, the rare big-bucket merge passes) and returns M.  Up to two scans may be in flight: with begin(i+1)
 * called before finish(i), the offsets + order kernel of scan i runs inside the launch of scan i+1's table pass, so
 * a steady stream of scans costs one kernel launch each — and the summary of scan i arrives while scan i+1 runs (a
 * caller that wants it sooner calls finish(i) first).  Results of a finished scan end at the next begin. */
int pie_scan_begin(pie_ctx *ctx, int64_t now, int64_t cutoff);
int pie_scan_finish(pie_ctx *ctx, size_t *m_out);
/* The same pair for the exchange step of a sharded table: the scan also produces its result message
 * [ off[0..u_pad] | M | rows[0..min(M, idx_cap)) ] (int32 words, the layout of pie_pack_results_device) in caller-owned
 * device memory dst_i32 (u_pad + 2 + idx_cap words, which must stay valid until the matching finish).
 * pie_scan_finish_packed: *ready_out = 1 when the message was complete in device memory before the call returned (the
 * scan's own kernels wrote it: a consumer on any stream, or a peer GPU, may read it at once); 0 when a pack kernel was
 * enqueued on the context's stream to write it (order the consumer after that stream, e.g. with an event). */
int pie_scan_begin_packed(pie_ctx *ctx, int64_t now, int64_t cutoff, void *dst_i32, size_t u_pad, size_t idx_cap);
int pie_scan_finish_packed(pie_ctx *ctx, size_t *m_out, int *ready_out);
/* pie_scan_begin_packed with a second destination: counts_dst_i32 (n_users words, may be NULL) receives counts[U].  Both
 * destinations are device-visible memory; they may be MAPPED PINNED HOST memory (pie_host_alloc): the scan's own kernels
 * then deliver offsets / counts / rows to the host with no copy node behind the scan ("D2H of
 * counts/offsets included"), complete when pie_scan_finish_packed returns with *ready_out = 1 or, with 0, after
 * pie_synchronize. */
int pie_scan_begin_packed2(pie_ctx *ctx, int64_t now, int64_t cutoff, void *dst_i32, size_t u_pad, size_t idx_cap,
                           void *counts_dst_i32);
/* Pinned host memory mapped into the device's address space: *host_out is the CPU address, *dev_out the address a
 * kernel (or pie_scan_begin_packed*) uses for the same bytes. */
int pie_host_alloc(pie_ctx *ctx, size_t bytes, void **host_out, void **dev_out);
int pie_host_free(pie_ctx *ctx, void *host_ptr);
/* ---- batched scan: many feed requests, one table pass (SURVEY.md section 7 "batch many queries per launch"; the
 * north_star's "calendarFeed per-request loop -> batched GPU scan").  Every query has its own `now` (the request's clock,
 * server/sessionStore.js:67 samples one per scan), `cutoff` (server/calendarFeed.js:33-38) and discipline mask
 * (server/disciplineConfig.js:88-97; bits >= n_disc of pie_set_disciplines are ignored).  Up to three batches per lane (see
 * pie_set_batch_lanes) may be in flight (begin(i+1), begin(i+2) before finish(i): the tail of batch i rides in the launch of the
 * next batch of its lane, and with a third batch queued the GPU never waits for the host to react to a summary); single scans
 * and batches do not mix in flight.
 *
 * The PRIMARY result of a batch is the UNION of its queries' selections: per user the rows that ANY query selected, in
 * (start, row) order, with a query mask per row —
 *     uoff[U+1] (int64) | rows[Mu] (int32) | mask[Mu] (bit q = query q selected the row)
 *     Feed(q, u) = the rows of rows[uoff[u] : uoff[u+1]] whose mask has bit q, in that order
 * (requests that arrive together select almost the same rows: the union is little longer than one query's list, whatever Q).
 * pie_scan_batch_finish reports every query's M; pie_batch_read_user_feed answers a request straight from the union.  The
 * per-query form of a result — counts[U], offsets[U+1], idx[M], bit for bit those of n_q separate pie_scan calls — is
 * materialised from the union only when asked for (pie_batch_read_results, pie_batch_result_device_ptrs, the per-query
 * messages).  A query the batched pass cannot hold (a dense query, a user with more than 64 union rows) is rerun inside
 * pie_scan_batch_finish on the general path; such a batch has per-query results only (no union: pie_batch_union_device_ptrs
 * returns NULL pointers). */
#define PIE_BATCH_MAX 64
typedef struct pie_query {
    int64_t now, cutoff;
    uint64_t mask;
} pie_query;
int pie_scan_batch_begin(pie_ctx *ctx, const pie_query *queries, int n_q);
/* m_out: n_q selected-row counts (may be NULL) */
int pie_scan_batch_finish(pie_ctx *ctx, size_t *m_out);
/* begin + finish */
int pie_scan_batch(pie_ctx *ctx, const pie_query *queries, int n_q, size_t *m_out);
/* The union of the last finished batch: device pointers (valid until three more batches have begun; NULL when the batch has
 * no union, see above), or host copies (masks_out: one 64-bit mask per union row; PIE_E_CAPACITY if cap < Mu, PIE_E_STATE if
 * the batch has no union). */
int pie_batch_union_device_ptrs(pie_ctx *ctx, void **uoff_dev /* int64[U+1] */, void **rows_dev /* int32[Mu] */,
                                void **mask_lo_dev /* uint32[Mu]: queries 0..31 */, void **mask_hi_dev /* uint32[Mu]: 32..63, NULL for n_q <= 32 */,
                                size_t *mu_out);
int pie_batch_read_union(pie_ctx *ctx, int64_t *uoff_out, int32_t *rows_out, uint64_t *masks_out, size_t cap, size_t *mu_out);
/* ---- WIDE batches: 1..PIE_WIDE_MAX queries, one table pass.  The same pie_query records and the same semantics as the batch
 * above: Feed(q, u) is bit for bit what pie_scan with query q's (now, cutoff, mask) gives.  Wide and ordinary batches share the
 * context's lanes, slots and FIFO (pie_batch_room counts both; finish order is begin order).  pie_scan_batch_finish[_packed]
 * return PIE_E_STATE and consume nothing when the oldest batch in flight is wide; pie_scan_wide_finish finishes the oldest batch
 * of either kind (m_out: n_q counts; PIE_E_CAPACITY if m_cap < n_q, nothing consumed).  After a wide batch the readers that take
 * a query index (pie_batch_read_results, pie_batch_result_device_ptrs, pie_batch_read_user_feed, pie_batch_fetch_requests) accept
 * every qi < n_q; the 32/64-bit union readers (pie_batch_union_device_ptrs, pie_batch_read_union, pie_batch_pack_union_device)
 * return PIE_E_STATE.  A wide batch whose queries fall back (dense queries, a user whose union outgrows 64 slots, bad rows), on a
 * table whose batches take the ordered run unless pie_set_wide_ordered is on, or on a table that cannot run the batched pass,
 * has exact per-query results and no union: the wide union readers return PIE_E_STATE.  The wide state (mask words, host
 * summaries) is allocated by the first wide batch of a context.
 * With pie_set_wide_ordered(ctx, 1) a wide batch on a table whose batches take the ordered run (skewed users, mode 2 of
 * pie_set_ordered_run, a table the general pass gave up on) is ONE pass over the run's key column and keeps its union like any
 * other: per user the rows any query selects in (start, row) order with no 64-row bound per user, bounded only by the union
 * result arrays (max(16 rows per user of capacity, rows / 16 + 4096)).  A union that outgrows them reruns every query (exact
 * results, no union) and sends the context's later wide batches back to the per-query path until the table is loaded anew.
 * The run holds no row whose user id lies outside [0, users) (its build leaves them out), so on a table that has such rows
 * this pass simply never selects them, as the ordinary batch on the run does, where the general wide pass returns PIE_E_INVAL. */
#define PIE_WIDE_MAX 512
int pie_scan_wide_begin(pie_ctx *ctx, const pie_query *queries, int n_q);
int pie_scan_wide_finish(pie_ctx *ctx, size_t *m_out, size_t m_cap, int *n_q_out);
/* The union of the last finished wide batch: words = ceil(n_q / 64) uint64 mask words per union row, bit q of row r =
 * masks[r * words + q / 64] >> (q % 64) & 1.  Device pointers are valid until three more batches have begun on the lane. */
int pie_batch_union_wide_device_ptrs(pie_ctx *ctx, void **uoff_dev /* int64[U+1] */, void **rows_dev /* int32[Mu] */,
                                     void **masks_dev /* uint64[Mu][words] */, int *words_out, size_t *mu_out);
int pie_batch_read_union_wide(pie_ctx *ctx, int64_t *uoff_out, int32_t *rows_out, uint64_t *masks_out /* [cap][words] */, size_t cap,
                              int *words_out, size_t *mu_out);
/* The exchange message of the wide union into device memory, enqueued on the context's stream:
 * [ uoff[0..u_pad] | Mu | rows[0..cap) | masks[0..cap) as 2 * words int32 words per row ] (rows beyond cap are cut). */
int pie_batch_pack_union_wide_device(pie_ctx *ctx, void *dst_i32, size_t u_pad, size_t cap);
/* A wide batch that writes that exchange message itself (the wide counterpart of pie_scan_batch_begin_union): the launch that
 * orders the union buckets also stores the message words, so no pack launch follows.  Layout as above with words =
 * ceil(n_q / 64): u_pad + 2 + cap * (1 + 2 * words) int32 words; uoff[u] = Mu for u >= users; rows beyond cap are cut, Mu
 * still says how many there are.  msg_i32 is device-visible memory (device or mapped host, pie_host_alloc) that stays valid
 * until the matching finish; u_pad >= users.
 * pie_scan_wide_finish_packed finishes the oldest batch of either kind, as pie_scan_wide_finish does.  *ready_out = 1: the
 * batch kept its union and the message was complete when the call returned.  *ready_out = 0: the batch has no union (queries
 * fell back, the table is on the ordered run unless pie_set_wide_ordered is on, or cannot run the batched pass, the slot masks
 * exceed the direct bound); the
 * header — uoff[0..u_pad] and the Mu word, all -1 — is written on the context's stream (order the consumer behind
 * pie_ctx_aux_stream); the per-query results stay exact and readable through the readers above.  The first wide batch on a
 * table normally overflows its 16 union slots per user and reruns on the general path while the slot capacity grows, so it
 * reports ready = 0 / Mu = -1: a caller repeats the batch.  pie_scan_wide_finish also finishes a batch begun here; the
 * message is then ordered on the context's stream, as with ready = 0. */
int pie_scan_wide_begin_union(pie_ctx *ctx, const pie_query *queries, int n_q, void *msg_i32, size_t u_pad, size_t cap);
int pie_scan_wide_finish_packed(pie_ctx *ctx, size_t *m_out, size_t m_cap, int *n_q_out, int *ready_out);
/* Batch LANES.  A batch over a shard-sized table (a tenth of 10^8 rows) is one launch of ~20 us that occupies a fraction of
 * the chip: its time is latency, not bytes, and that floor is what would cap an 8-GPU split of the table at 2.5x.  A context
 * therefore deals its batches to up to four lanes — independent pipelines, each with its own HIP stream, three batch slots and
 * spans — whose launches run SIDE BY SIDE on the chip; pie_scan_batch_begin picks the lane (round robin),
 * pie_scan_batch_finish returns batches in the order they were begun, so callers do not change: with n lanes up to 3 n batches
 * may be in flight.  n_lanes 1..4 pins the number, 0 (default; PIE_BATCH_LANES) chooses by table size: 4 up to 2^25 rows, 3
 * above.  Batches on the ordered run and batches that only fall back stay on lane 0.  Reading a finished batch's arrays
 * on the context's stream is ordered behind the lane by the library; the messages of pie_scan_batch_begin_union are complete
 * when finish says ready, as before.  There is no counterpart in the reference (one request at a time,
 * server/index.js:293-302). */
int pie_set_batch_lanes(pie_ctx *ctx, int n_lanes);
int pie_batch_lanes(pie_ctx *ctx); /* lanes in use now */
/* Batches pie_scan_batch_begin would take right now (0: finish one first): three per lane less those in flight; a table whose
 * batches run on the ordered run uses lane 0 only, whatever the lane count.  A pipelined caller asks this instead of counting. */
int pie_batch_room(pie_ctx *ctx);
/* The end of a burst: no further begin is coming for now.  The tail of a batch normally rides in its lane's next launch and,
 * for a lane's last batch, is queued when that batch is finished — one after the other as the caller works through them.
 * pie_scan_batch_flush queues the waiting tails of all lanes at once (they run side by side); optional, results unchanged; a
 * begin after it simply carries no tail. */
int pie_scan_batch_flush(pie_ctx *ctx);
/* A batch that also writes the multi-GPU exchange message as it goes — ONE union message for the whole batch:
 *   msg (int32 words) = [ uoff[0..u_pad] | Mu | rows[0..cap) | mask_lo[0..cap) | mask_hi[0..cap) (only when n_q > 32) ]
 * u_pad + 2 + 2 * cap words (3 * cap for n_q > 32); uoff[u] = Mu for u >= users; rows beyond cap are dropped (Mu says how many
 * there are).  msg is device-visible memory (device or mapped host) that stays valid until the matching finish.
 * pie_scan_batch_finish_packed: *ready_out = 1 when the message was complete when the call returned (the batch's own kernels
 * wrote it); 0 when it was packed afterwards on the context's stream (order the consumer behind pie_ctx_aux_stream) — then
 * Mu = -1 means a user's merged union exceeds 32 rows or the batch holds more than 32 queries: use the per-query messages. */
int pie_scan_batch_begin_union(pie_ctx *ctx, const pie_query *queries, int n_q, void *msg_i32, size_t u_pad, size_t cap);
/* The per-query form of the exchange: one result message per query (layout of pie_pack_results_device) written to
 * msg_i32 + q * msg_stride_words and, optionally, counts[U] to counts_i32 + q * counts_stride_words; both device-visible.
 * The lists are materialised from the union and packed at finish (*ready_out = 0: order the consumer behind the context's
 * stream). */
int pie_scan_batch_begin_packed(pie_ctx *ctx, const pie_query *queries, int n_q, void *msg_i32, size_t msg_stride_words,
                                size_t u_pad, size_t idx_cap, void *counts_i32, size_t counts_stride_words);
int pie_scan_batch_finish_packed(pie_ctx *ctx, size_t *m_out, int *ready_out);
/* Results of query `qi` of the last finished batch (as pie_read_results / pie_result_device_ptrs): materialised on first use. */
int pie_batch_read_results(pie_ctx *ctx, int qi, int32_t *counts_out, int64_t *offsets_out, int32_t *idx_out, size_t idx_cap,
                           size_t *m_out);
int pie_batch_result_device_ptrs(pie_ctx *ctx, int qi, void **counts_dev, void **offsets_dev, void **idx_dev);
/* The union message (layout above) of the last finished batch into caller memory, whatever path the batch took; enqueued on
 * the context's stream (pie_ctx_aux_stream). */
int pie_batch_pack_union_device(pie_ctx *ctx, void *dst_i32, size_t u_pad, size_t cap);
/* One user's feed of query `qi` of the last finished batch (as pie_read_user_feed): the per-request read of a server that
 * answers the requests of one event-loop turn with one batch (/root/reference/server/index.js:293-302).  Read from the union
 * (two small copies + a filter on the host); no per-query list is built for it. */
int pie_batch_read_user_feed(pie_ctx *ctx, int qi, int32_t user, int32_t *idx_out, size_t idx_cap, size_t *k_out);

/* The requests of one event-loop turn, fetched together: request i asks for Feed(qi[i], user[i]) of the last finished batch.
 * req_off_out[n_req + 1] (exclusive offsets into the arrays below), then for every request its rows in feed order and the
 * columns the host serialises (start, end, disc: the event object of server/calendarFeed.js:66-79) — two device round trips
 * for the whole batch instead of three small copies per request.  A user outside [0, U) has an empty feed.  PIE_E_CAPACITY if
 * the feeds hold more than cap_rows rows (*total_out says how many). */
int pie_batch_fetch_requests(pie_ctx *ctx, const int32_t *qi, const int32_t *user, size_t n_req, size_t cap_rows, int64_t *req_off_out,
                             int32_t *idx_out, int64_t *start_out, int64_t *end_out, int32_t *disc_out, size_t *total_out);

/* Copy the last finished scan's results to host arrays (what pie_scan does after scanning); any pointer may be NULL. */
int pie_read_results(pie_ctx *ctx, int32_t *counts_out, int64_t *offsets_out, int32_t *idx_out, size_t idx_cap,
                     size_t *m_out);
/* One user's feed of the last finished scan: rows idx[offsets[user] .. offsets[user+1]) into idx_out (two small copies
 * instead of the whole result: the per-request read behind GET /api/calendar, /root/reference/server/index.js:293-302).
 * *k_out = the feed's length; PIE_E_CAPACITY if it exceeds idx_cap; a user outside [0, U) has an empty feed. */
int pie_read_user_feed(pie_ctx *ctx, int32_t user, int32_t *idx_out, size_t idx_cap, size_t *k_out);
/* Device pointers of the last finished scan's results: complete in stream order (pie_ctx_aux_stream) or after
 * pie_synchronize; valid until the next pie_scan_begin. */
int pie_result_device_ptrs(pie_ctx *ctx, void **counts_dev, void **offsets_dev, void **idx_dev);
/* Copy the last scan's results into caller-owned DEVICE buffers (e.g. torch tensors that feed an RCCL
 * all-gather), asynchronously on the context's stream.  Any pointer may be NULL; idx copies min(M, idx_cap). */
int pie_copy_results_device(pie_ctx *ctx, void *counts_dst, void *offsets_dst, void *idx_dst, size_t idx_cap);
/* Pack the last scan's results into ONE int32 message in caller-owned device memory, one launch on the context's
 * stream: [off[0..u_pad] (exclusive offsets, = M past the last user) | M | idx[0 .. min(M, idx_cap))], u_pad+2+cap
 * words — the unit of the multi-GPU all-gather; Feed(u) = idx[off[u] : off[u+1]]. */
int pie_pack_results_device(pie_ctx *ctx, void *dst_i32, size_t u_pad, size_t idx_cap);
/* Gather the rows named by idx (host array of m row indices) for host-side serialisation
 * (the event object of server/calendarFeed.js:66-79).  Output pointers may be NULL. */
int pie_fetch_rows(pie_ctx *ctx, const int32_t *idx, size_t m, int64_t *start, int64_t *end, int32_t *user,
                   int32_t *disc);

/* ---- "next" row: newly-expired change predicate -> ordered dispatch queue -----------
 * queue = ascending row indices with prev_now < end <= now  (dead per server/sessionStore.js:69 at `now`,
 * not yet dead at `prev_now`); order = the sequential-await order of server/storage/sqlProvider.js:834-861. */
int pie_expired_queue(pie_ctx *ctx, int64_t prev_now, int64_t now, int32_t *queue_out, size_t cap, size_t *q_out);

/* The reference's own archive chain (server/storage/sqlProvider.js:758-816 _archiveDailyShows), [DERIVED] onto the
 * session table with the user column as the group key: a group's earliest = min(start) over its (non-tombstoned)
 * rows; it qualifies iff now - earliest >= window_ms (:798, AUTO_ARCHIVE_WINDOW_MS :9); every row of a qualifying
 * group is queued, groups in order of first appearance (Map insertion order), rows in table order inside a group —
 * the order in which :834-861 dispatches them.  Entirely on the device: one pass for the group statistics, the threshold and
 * the first-appearance ranks per group, an order-preserving selection pass, a stable sort of the queued rows by group rank. */
int pie_archive_queue(pie_ctx *ctx, int64_t now, int64_t window_ms, int32_t *queue_out, size_t cap, size_t *q_out);
/* Measurement of the archive chain: with pie_set_profiling on, the device time (first kernel start -> end of the last sort) of
 * the chains since pie_stats_reset and their number; the algorithmic bytes of the last one: 20 B/row for the group statistics
 * (start, end, user) + 12 B/row for the selection (end, user) + 4 B per queued row. */
int pie_archive_stats(pie_ctx *ctx, double *ms_sum_out, uint32_t *calls_out, uint64_t *alg_bytes_out);
/* The queue the last pie_expired_queue / pie_archive_queue left on the device, for the cross-shard merge (pie_comm_*_queue).
 * pie_queue_info: kind 1 = expired, 2 = archive (0: none — a scan, batch or table change since forgot it), its rows, and for
 * the archive queue its groups.  PIE_E_STATE when there is none, or when the table holds rows its shard map does not cover
 * (appended after pie_shard_table: they have no global row).
 * What forgets it: every scan begin, and a batch that stages in the scan slots' workspace; every call that answers with a row
 * list (prune, purge, delete_user(s), the two queue calls themselves, one that fails for capacity included); a load, generate,
 * shard or compaction; and every call that adds rows or writes `end` through the table's own mutators — pie_append_rows,
 * pie_set_end, their pie_shard_* and pie_token_* forms and a turn that logs in — whether it ran in place or had to grow the
 * table.  A queue of row indices from before such a change is never handed out.  (pie_expired_queue_begin / _finish and a token
 * turn that only touches or deletes leave it alone.)
 * pie_queue_pack_device: pack it into ONE int32 message in caller-owned device memory, one launch on the context's stream:
 *   [ n_rows | n_groups | global rows (cap_rows) | local rows (cap_rows) | group offsets (cap_groups + 1) ]
 * global row = the shard map's entry (the row itself on a context that was never sharded); group offsets = the exclusive
 * scan of the group sizes in group order, closed by n_rows (expired: n_groups = 0).  2 + 2 cap_rows + cap_groups + 1 words;
 * PIE_E_CAPACITY if the queue has more rows or groups than that, PIE_E_STATE as pie_queue_info. */
int pie_queue_info(pie_ctx *ctx, int32_t *kind_out, size_t *rows_out, size_t *groups_out);
int pie_queue_pack_device(pie_ctx *ctx, void *dst_i32, size_t cap_rows, size_t cap_groups);

/* ---- measurement ------------------------------------------------------------------------------------- */
/* Pin the form of the table pass (the codes of pie_stats.k1_variant, DESIGN.md section 8: 0x01 reads every byte of the
 * four columns, 0x03 the streaming form, 0xC85 the keyed form ...); form < 0 returns to the adaptive choice.  A tuning /
 * measurement switch: every form produces identical results.  Not while a scan is in flight. */
int pie_set_scan_form(pie_ctx *ctx, int form);
typedef struct pie_table_info {
    uint32_t struct_size;     /* set by caller to sizeof(pie_table_info) */
    uint32_t has_keys;        /* 1: the derived liveness-key / payload columns exist and are in step */
    uint64_t rows, users;
    uint64_t table_bytes;     /* 24 * capacity rows: the four caller-visible columns */
    uint64_t derived_bytes;   /* derived columns (2-byte key, 1-byte key, 16-byte payload record) */
    uint64_t workspace_bytes; /* per-scan workspace of the two slots + histogram spans */
    double index_build_ms;    /* host wall time of the last full build of the derived columns (kernels + syncs) */
    uint64_t ordered_rows;    /* rows the ordered run holds (0: there is none, or it was invalidated) */
    uint64_t ordered_bytes;   /* device memory of the ordered run (27 B per position + 4 B per row of capacity + small arrays) */
    double ordered_build_ms;  /* host wall time of its last build (one all-selecting scan + a gather) */
    uint64_t ordered_builds;  /* times it was built for this context */
    uint64_t ordered_positions; /* positions a scan of the run visits: its rows + the spare slots of every user's segment */
    uint64_t ordered_respreads; /* times appends filled a segment and the run was moved into fresh segments (a linear pass) */
    uint64_t hot_rows;        /* rows the end-ordered hot index holds, its delta aside (0: there is none, or it was dropped) */
    uint64_t hot_bytes;       /* device memory of the hot index (32 B per entry and delta slot + 4 B per row of capacity + build scratch) */
    uint64_t hot_builds;      /* times it was built for this context */
    /* fields below were added with pie_compact_rows: a caller that sets struct_size to the size without them gets the rest */
    uint64_t compact_bytes;   /* device memory of the two maps of the last compaction (0: there are none) */
    uint64_t compactions;     /* pie_compact_rows calls that succeeded on this context */
    double compact_count_ms;  /* device time (HIP events around the two kernels) of the last compaction's count pass and prefix ... */
    double compact_write_ms;  /* ... and of its write pass */
    /* fields below were added with the slot-ordered hot index, under the same rule */
    double hot_build_ms;      /* device time of the hot index's last build (count, scan, and the scatter or keys + sort + gather) */
    uint32_t hot_order;       /* records inside a bin of the index: 0 ascending row, 1 by histogram slot (the order of the index
                               * that stands; with none, the order the next build will try: PIE_HOT_ORDER) */
    uint32_t hot_slot_bits;   /* bits of a histogram slot in the sort key at the present user count */
    /* fields below were added with the token index (pie_token_*), under the same rule */
    uint64_t token_rows;      /* rows the token column covers (0: there is none) */
    uint64_t token_bytes;     /* device memory of the token column (16 B per row of capacity), its index (4 B per slot) and the lookup staging */
    uint64_t token_builds;    /* times the index was built from the column (pie_token_set, growth, compaction) */
    double token_build_ms;    /* device time of the last such build (HIP events around the fill and the insert pass) */
    /* fields below were added with the in-flight expired queue (pie_expired_queue_begin), under the same rule */
    uint64_t expired_inflight_bytes; /* device memory of its scratch (one count and one offset per unit) and its queue buffer */
    double expired_inflight_ms;      /* device time of the last pass that has run (HIP events on its own stream) */
} pie_table_info;
int pie_table_info_get(pie_ctx *ctx, pie_table_info *out);
/* The hot index's layout, for tests and tools (host-only readers; not while a scan is in flight).  The index groups the rows
 * whose `end` reaches the fine key's base by fine-key bin 1..127; off[k] is the first record of bin k, off[128] = n_main.
 * Inside a bin the records stand by ascending sort key, rows ascending among equal keys, where
 *     key = (bin << pie_hot_slot_bits(n_users)) | histogram slot of the record's user
 * at the user count of the build (PIE_HOT_ORDER=slot, the default; hot_order = 1), or by ascending row (PIE_HOT_ORDER=row, or a
 * slot build that found no scratch memory or no room for bin and slot in 32 bits; hot_order = 0).  The order is a locality
 * hint for the pass's histogram atomics and reaches no result; appends that add users leave it stale until the next build.
 * pie_hot_layout: off[129] and *n_main; user / row / bin of the n_main main records when any of the three is given (cap = room
 * in each, PIE_E_CAPACITY when n_main is larger); pos[n_pos] = the record of rows 0 .. n_pos - 1, -1 for a row the index does
 * not hold.  Every pointer may be NULL.  PIE_E_STATE when there is no index.
 * pie_hot_order_key, pie_hot_slot_bits: pure host functions, no context. */
int pie_hot_layout(pie_ctx *ctx, int64_t *off, int64_t *n_main, int32_t *user, int32_t *row, int32_t *bin, size_t cap,
                   int32_t *pos, size_t n_pos);
uint64_t pie_hot_order_key(uint32_t bin, int32_t user, uint32_t n_users);
uint32_t pie_hot_slot_bits(uint32_t n_users);
/* The ordered run (sph-pie_amd/csrc/pie_ordered.h): the table's rows a second time, in (user, start, row) order — the order
 * of every answer — so that a query is a filter over positions: no histogram atomics, no per-bucket sort, no dependence on
 * how rows are spread over users.  There is no counterpart in the reference (its Map is scanned per request,
 * server/sessionStore.js:55-73); results are identical to the general path's.  mode 0: never (frees it); 1 (default):
 * built and used when the general path is weak — a query selecting more than 1/24 of the rows, or skewed users — the second
 * time in a row such a query arrives; 2: always (built at the next scan).  Touches and deletes keep it in step, and so do
 * appends: a new row is inserted at its place in its user's segment, which ends in spare slots — for a session store's
 * createSession that place is the end; a row a little late shifts the few behind it; a full segment moves the run into
 * fresh segments (a linear pass).  Loads, sharding and back-fills (a row more than 256 rows back in its segment) invalidate
 * it (queries run on the general path until it is rebuilt).  A turn that logs in (pie_session_turn and its shard forms, a
 * PIE_TURN_CREATE among the ops) drops it too, unless pie_set_turn_ordered is on: then the rows the turn creates are inserted
 * as an append's rows are.  PIE_ORDERED=0|1|2 sets the mode a context starts with. */
int pie_set_ordered_run(pie_ctx *ctx, int mode);
/* Wide batches on the ordered run (see pie_scan_wide_begin).  0 (default): a wide batch on a table whose batches take the
 * ordered run reruns every query as a single scan and keeps no union.  1: it runs one pass over the run and keeps its union
 * (and writes the message of pie_scan_wide_begin_union, ready = 1).  A table that does not take the ordered run is not
 * affected.  PIE_E_STATE while a scan or batch is in flight, PIE_E_INVAL for any other value.  PIE_WIDE_ORDERED=1 sets the
 * value a context starts with. */
int pie_set_wide_ordered(pie_ctx *ctx, int on);
/* Turns that log in on a table with a valid ordered run (pie_session_turn, pie_shard_session_turn, pie_comm_session_turn: set it
 * on every shard's context, pie_comm_ctx).  0 (default): a turn in which the context keeps at least one PIE_TURN_CREATE drops the
 * run.  1: such a turn keeps the run where pie_append_rows would keep it — the run is valid and covers every row, the context
 * keeps at most 4096 creates, its user count after the turn is within the users the run has segments for, the key columns are in
 * step, and the table does not have to grow.  Behind the turn's kernel the created rows are read back from the table (with the
 * `end` the turn's later ops left them) and inserted into their users' segments; a full segment re-spreads the run; a row more
 * than 256 rows back in its segment, or a row the run does not hold that the turn brought back to life, drops it.  Results,
 * the table and every index are the same with 0 and 1: only whether the run survives differs.  Create-free turns, pie_token_turn
 * and the turns begun in flight (pie_token_turn_begin) are not affected.  PIE_E_INVAL for a NULL context or any other value;
 * PIE_E_STATE while a scan or batch is in flight or a turn is begun and not finished.  PIE_TURN_ORDERED=1 sets the value a
 * context starts with. */
int pie_set_turn_ordered(pie_ctx *ctx, int on);
/* 0: off.  n >= 1: every n-th scan carries HIP events around K1 and around the whole scan (an event between two
 * kernels costs a few microseconds of pipeline drain, so a benchmark samples). */
int pie_set_profiling(pie_ctx *ctx, int enabled);
int pie_stats_get(pie_ctx *ctx, pie_stats *out);  /* resolves pending events (synchronises the stream) */
int pie_stats_reset(pie_ctx *ctx);
int pie_synchronize(pie_ctx *ctx);
/* user-hash sharding rule: shard = splitmix64(user) mod n_shards.  Pure host function. */
int32_t pie_shard_of(int32_t user, int32_t n_shards);
/* Shard the RESIDENT table on the device: keep only the rows whose user hashes to `rank` of `world` (pie_shard_of), in table
 * order, users re-numbered densely in ascending global id (a shard with no user keeps n_users = 1).  Every rank loads or
 * generates the same whole table and calls this with its own rank; nothing crosses PCIe.  *n_rows_out / *n_users_out = the
 * shard's size.  pie_shard_maps copies the maps back: rows_global_out[i] = the global row of local row i (n_rows),
 * users_global_out[k] = the global id of local user k (n_users); either may be NULL. */
int pie_shard_table(pie_ctx *ctx, int32_t rank, int32_t world, size_t *n_rows_out, int32_t *n_users_out);
int pie_shard_maps(pie_ctx *ctx, int32_t *rows_global_out, int32_t *users_global_out);

/* ---- a LIVE sharded table: createSession / touchSession / deleteSession / deleteSessionsForUser (server/sessionStore.js:12-19,
 * 37-64) by GLOBAL id.  A context that pie_shard_table left remembers its rank, the world, and the size of the WHOLE table
 * (N_g rows, U_g users).  Every shard is given the same call with the same arrays and keeps what is its own; nothing is
 * exchanged.  The calls keep the shards in step with the unsharded table: a shard's rows are the whole table's rows of its
 * users in ascending global row (less what its own compactions dropped), its row map ascends and covers every local row, its
 * user map is the ascending list of ALL ids in [0, U_g) that hash to the rank.  New users always have ids at or above the old
 * U_g, new rows global ids above all earlier ones, so both maps grow at their ends only and no local id ever moves; global
 * row ids are never reused (pie_compact_rows keeps reporting the original ones).  Rows appended this way HAVE a global row:
 * pie_queue_info, pie_queue_pack_device and the pie_comm_*_queue calls keep working.
 * All of them return PIE_E_STATE on a context that was never sharded (or whose table was loaded or generated anew since), on
 * one whose row map does not cover its rows (plain pie_append_rows added some), and while a scan or batch is in flight.
 * Everything is checked before anything is staged or changed.  The device maps have room for the table's capacity and grow
 * with it; the context keeps a host copy of the user map (4 B per local user) and none of the row map. */
int pie_shard_info(pie_ctx *ctx, int32_t *rank_out, int32_t *world_out, int64_t *rows_global_out /* N_g */,
                   int32_t *users_global_out /* U_g */, uint64_t *map_bytes_out /* device bytes of the two maps */);
/* The k rows are rows [N_g, N_g + k) of the unsharded table, in array order; user_global[] holds GLOBAL ids in
 * [0, n_users_global), n_users_global >= U_g (PIE_E_INVAL otherwise, and when N_g + k >= 2^31 - 1).  The shard keeps the rows
 * whose user hashes to it; N_g grows by k and U_g to n_users_global on every shard whether or not it kept a row (k = 0 only
 * raises U_g).  *first_row_out = N_g before the call, *n_kept_out = rows kept.  Queued and un-waited where pie_append_rows is. */
int pie_shard_append_rows(pie_ctx *ctx, const int64_t *start, const int64_t *end, const int32_t *user_global, const int32_t *disc,
                          size_t k, int32_t n_users_global, int32_t *first_row_out, size_t *n_kept_out);
/* end[row] = new_end by GLOBAL row in [0, N_g) (PIE_E_INVAL outside).  The shard applies the elements whose row it holds; rows
 * of other shards and rows its compactions dropped are skipped.  Repeats: the last element wins, as in pie_set_end.  A touch of a
 * row appended by the call before finds that row (stream order), with no wait in between. */
int pie_shard_set_end(pie_ctx *ctx, const int32_t *rows_global, const int64_t *new_end, size_t k);
/* pie_delete_user by GLOBAL user id: a no-op (n_deleted = 0) on the shards the user does not hash to and for ids outside
 * [0, U_g); rows_global_out (may be NULL) receives GLOBAL rows, ascending. */
int pie_shard_delete_user(pie_ctx *ctx, int32_t user_global, int32_t *rows_global_out, size_t cap, size_t *n_deleted);
/* pie_delete_users by GLOBAL user ids: ids outside [0, U_g), ids that hash to another shard and ids this shard's user map does
 * not hold are skipped (count 0); rows_global_out receives GLOBAL rows, ascending (translated on the device). */
int pie_shard_delete_users(pie_ctx *ctx, const int32_t *users_global, size_t k, int32_t *rows_global_out, size_t cap,
                           size_t *n_deleted, int32_t *per_user_out /* [k] */);
/* pie_prune_before / pie_retention_purge / pie_retention_purge_tz (_pruneCalendarEvents, server/storage/sqlProvider.js:956-968;
 * _purgeExpiredArchives / _isArchiveExpired / _addMonths, :863-890, 991-1009) on a shard, answered in GLOBAL rows: each call
 * tombstones and lists exactly the local rows the plain call would on the same context, and rows_global_out (may be NULL)
 * receives their ORIGINAL global rows, ascending (the row map ascends, so local order is global order).  The write pass stores
 * row_map[row] itself: no translation pass follows.  Everything the plain calls maintain stays in step as under them (both
 * keys, the hot index, the ordered run's mirror, the held queue, slot 0's result).  PIE_E_STATE on a context that is not
 * sharded or whose row map does not cover its rows; all other rules are the plain calls': a cap too small tombstones the rows
 * all the same and returns PIE_E_CAPACITY with *n_out set. */
int pie_shard_prune_before(pie_ctx *ctx, int64_t cutoff, int32_t *rows_global_out, size_t cap, size_t *n_out);
int pie_shard_retention_purge(pie_ctx *ctx, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t *rows_global_out, size_t cap,
                              size_t *n_out);
int pie_shard_retention_purge_tz(pie_ctx *ctx, int64_t now, int32_t months, const int64_t *transitions_utc_ms, const int64_t *offsets_ms,
                                 int32_t n_transitions, int32_t *rows_global_out, size_t cap, size_t *n_out);
/* k global rows -> local rows in place (-1: not held by this shard); k local rows -> global rows in place (-1: outside the
 * map).  One small launch each, for hosts that hold a few rows of a huge table (the shape of pie_compact_translate); with
 * them the per-shard lists of pie_prune_before / pie_retention_purge* become global rows. */
int pie_shard_rows_to_local(pie_ctx *ctx, int32_t *rows_inout, size_t k);
int pie_shard_rows_to_global(pie_ctx *ctx, int32_t *rows_inout, size_t k);
/* Host only, no context, no GPU: the routing pie_shard_append_rows applies.  keep_out[i] = 1 iff pie_shard_of(user_global[i],
 * world) == rank (any int32 is routed: routing is not validation), *n_kept_out their number; new_users_out (cap entries, may be
 * NULL with cap 0) = the ascending ids in [users_before, users_after) that hash to rank, *n_new_out their number;
 * PIE_E_CAPACITY (with *n_new_out set) when that exceeds cap.  For tests. */
int pie_shard_route(const int32_t *user_global, size_t k, int32_t rank, int32_t world, uint8_t *keep_out, size_t *n_kept_out,
                    int32_t users_before, int32_t users_after, int32_t *new_users_out, size_t cap, size_t *n_new_out);

/* ---- compaction: the table's counterpart of `sessions.delete()` (server/sessionStore.js:47-53,66-73) ---------------------
 * Every mutator above appends rows or tombstones them; pie_compact_rows is what removes rows from the device table.
 * Keep, in table order, exactly the rows with end > dead_before; drop the rest.  dead_before = PIE_END_NONE drops
 * tombstones only; dead_before = T also drops sessions that expired at or before T (e.g. the `now` of the last purge
 * that reported them).  Users are NOT renumbered; n_users is unchanged.  *n_kept_out = new row count.  Row order is
 * kept, so under the tie rule (start asc, row index asc) every feed is the old one with its rows renumbered.
 *   PIE_E_STATE with no table, or while a scan or batch is in flight; queued asynchronous appends and touches land first.
 *   Afterwards the four columns hold the kept rows in their old order; the 2-byte key, 1-byte key and payload records are
 *   rebuilt and in step (has_keys unchanged); the hot index is dropped and rebuilt by the next batch that can use it, the
 *   ordered run is invalid and comes back under its mode's rule, what the scans had learned about the table is forgotten —
 *   all as after a load.  The last scan / batch results and the queue of pie_queue_info are forgotten (kind 0).
 *   Without PIE_COMPACT_SHRINK capacity and workspace stay: the kept rows are written into fresh columns of the same capacity,
 *   which then replace the old ones (no second copy).  With it the table and its workspace are re-sized to the kept rows,
 *   as pie_shard_table does: pie_table_info.table_bytes and workspace_bytes fall to those of a load of the kept rows.
 *   Every row dropped leaves a valid empty table (0 rows, capacity >= 1): scans answer empty, appends work.
 *   On a sharded context the local row -> global row map is gathered with the columns: pie_shard_maps, pie_queue_pack_device
 *   and the pie_comm_*_queue calls keep reporting the ORIGINAL global rows; the user map is untouched.
 *   When nothing is dropped the columns and everything derived from them are left alone; the maps are the identity.
 *   Memory: the kept rows are written out of place, so while the call runs the device holds a second set of columns — 24 B x
 *   capacity without PIE_COMPACT_SHRINK, 24 B x kept rows with it — beside the two maps (4 B per old row + 4 B per kept row,
 *   which stay: pie_table_info.compact_bytes).  PIE_E_NOMEM before anything was moved leaves the table as it was; with
 *   PIE_COMPACT_SHRINK a failure while the right-sized workspace is allocated leaves the context without a table, as a failed
 *   pie_shard_table does. */
#define PIE_COMPACT_SHRINK 1u   /* also re-size the table and its workspace to the kept rows (as pie_shard_table does) */
int pie_compact_rows(pie_ctx *ctx, int64_t dead_before, uint32_t flags, size_t *n_kept_out);
/* Maps of the last compaction, resident on the device until the next table change that renumbers rows (load, gen,
 * shard, compact):  new_of_old[n_old] (-1 = dropped), old_of_new[n_kept] (ascending).  Host copies (either may be NULL);
 * PIE_E_STATE when there are none. */
int pie_compact_maps(pie_ctx *ctx, int32_t *new_of_old_out, int32_t *old_of_new_out, size_t *n_old_out, size_t *n_kept_out);
/* ... their device pointers (int32 arrays, valid as long as the maps are) ... */
int pie_compact_map_device_ptrs(pie_ctx *ctx, void **new_of_old_dev, void **old_of_new_dev, size_t *n_old_out, size_t *n_kept_out);
/* ... and k old row indices rewritten in place to their new ones (-1 = dropped; an index outside [0, n_old) -> -1):
 * one small gather, for a host that holds only a few rows of a huge table. */
int pie_compact_translate(pie_ctx *ctx, int32_t *rows_inout, size_t k);
/* How the two passes would cut a table of n rows: rows a wave takes per step, rows the waves of a block take per step, rows of
 * the contiguous unit every wave owns, blocks of the grid (any output may be NULL).  For tests that straddle the boundaries. */
int pie_compact_geometry(pie_ctx *ctx, size_t n, int32_t *rows_per_wave_step_out, int32_t *rows_per_block_step_out,
                         int64_t *rows_per_unit_out, int32_t *blocks_out);

/* ---- token index: getSession / touchSession / deleteSession BY TOKEN (server/sessionStore.js:21-53) -----------------------
 * The reference keys its Map by sha256(token) (sessionStore.js:8-10, :17).  The table carries that key as a column of its own:
 * the FIRST 16 BYTES of the digest as two little-endian uint64 per row, tok[row][2] (128 bits of a cryptographic hash: at 10^8
 * rows the probability that any two sessions collide is below 10^-22).  The device never hashes a token; the host does
 * (binding.token_key, host/tokenKeys.js).  From the column the library derives an open-addressing index — int32 slot_row[slots],
 * -1 empty, slots = pie_token_slots_for(covered) so it is at most half full, home slot = the top log2(slots) bits of a 64-bit mix
 * of the key (pie_token_homes), linear probing that wraps; a slot holds the row only, a probe compares against tok[row] — and a
 * batched lookup answers all the requests of one event-loop turn in one launch.
 * The column covers a PREFIX of the table, rows [0, covered): rows appended with pie_append_rows are not findable until
 * pie_token_append gives them keys.  There is no deleted state: tombstoned and expired rows stay findable and report live = 0
 * (all that `sessions.delete(hash)` on an expired lookup achieves, :30-33); an entry leaves when pie_compact_rows drops its row.
 * Of several rows under one key (a caller error in the reference: tokens are 48 random bytes) the LARGEST row answers.
 * Everything is queued on the context's stream, where pie_append_rows and pie_set_end queue their work: a lookup sees every
 * append, touch and pie_token_append issued before it with no host wait in between, and waits once, for its results.
 * What renumbers or replaces the table drops the column and index (pie_load_columns, pie_load_columns_dir, pie_gen_synthetic*,
 * pie_shard_table).  pie_compact_rows that drops rows carries them over: the keys of the kept covered rows are gathered (they are
 * a prefix again: covered = the kept rows whose old row was covered) and the index is rebuilt; the column keeps its capacity
 * under PIE_COMPACT_SHRINK; if that step runs out of memory the compaction stands and the column is dropped.
 * A SHARDED context (after pie_shard_table) takes its column by GLOBAL row through pie_shard_token_* below; pie_token_set
 * returns PIE_E_STATE there.
 * PIE_E_STATE: no table; no token column (all but pie_token_set); while a scan or batch is in flight (every call that takes a
 * context).  PIE_E_INVAL: NULL tok with k > 0.  PIE_E_HIP "probe bound exhausted": a probe loop ran its bound of `slots` steps
 * (an index out of step with its column — never seen; reported by the lookup or build that follows it).
 * Memory: 16 B per row of capacity + 4 B per slot (8 .. 16 B per covered row). */
/* keys for rows [0, n), n <= rows; replaces any earlier column; builds the index (replaces `sessions.set(hash, ...)`, :17) */
int pie_token_set(pie_ctx *ctx, const uint64_t *tok /* [n][2] */, size_t n);
/* createSession's `sessions.set` (:17) for rows appended since: keys for rows [covered, covered + k); PIE_E_INVAL if
 * covered + k > rows; queued, un-waited.  An append that would make covered > slots / 2 first rebuilds the index into
 * pie_token_slots_for(new covered) slots (the new table is allocated first: on PIE_E_NOMEM nothing has changed). */
int pie_token_append(pie_ctx *ctx, const uint64_t *tok, size_t k);
/* getSession for k tokens (sessionStore.js:21-35): row_out[i] = row or -1; live_out[i] = found && end > now;
 * user/start/end of found rows (undefined for -1).  Every output pointer may be NULL.  k = 0 is allowed. */
int pie_token_lookup(pie_ctx *ctx, const uint64_t *tok, size_t k, int64_t now, int32_t *row_out, uint8_t *live_out,
                     int32_t *user_out, int64_t *start_out, int64_t *end_out);
/* touchSession / deleteSession by token (:37-53): for every element whose key is found with end > now, end[row] = new_end[i],
 * through pie_set_end's own path (repeats: last element wins; both keys, hot index and ordered run stay in step).
 * rows_out[i] (may be NULL) = the row written or -1.  now = PIE_END_NONE applies to every found row that is not a tombstone. */
int pie_token_set_end(pie_ctx *ctx, const uint64_t *tok, const int64_t *new_end, size_t k, int64_t now, int32_t *rows_out);
/* tests and tools: *covered_out, *slots_out; slot_row_out[cap] (PIE_E_CAPACITY if cap < slots); tok_out[covered][2]; any may be NULL */
int pie_token_layout(pie_ctx *ctx, size_t *covered_out, size_t *slots_out, int32_t *slot_row_out, size_t cap, uint64_t *tok_out);
/* host only, no context, no GPU: the smallest power of two >= max(1024, 2 * covered); home_out[i] = the home slot of key i in
 * a table of 2^log2_slots slots (log2_slots <= 32, PIE_E_INVAL otherwise) — the rule the device applies */
size_t pie_token_slots_for(size_t covered);
int pie_token_homes(const uint64_t *tok, size_t k, uint32_t log2_slots, uint32_t *home_out);

/* ---- a whole event-loop TURN by token: an ORDERED list of getSession / touchSession / deleteSession calls
 * (server/sessionStore.js:21-53), each with its own clock, in one upload, one kernel, one download and one wait.  The results
 * equal the calls made one by one: a touch changes what the next get of the same token returns, a delete makes the following
 * touch a no-op, a get after a touch sees the new end.
 * A key's row is the one pie_token_lookup finds: the largest row under the key, or -1.  Let e be that row's `end`.  The ops are
 * applied in array order; ops with different keys never interact (distinct keys have distinct rows).
 *     op      condition                     live_out              end_out        effect
 *     GET     always                        found && e > now      e              none
 *     TOUCH   found && e > now              1                     new_end        e := new_end
 *     TOUCH   otherwise                     0                     e              none
 *     DELETE  found && e != PIE_END_NONE    0                     PIE_END_NONE   e := PIE_END_NONE (liveness not consulted, :47-53)
 *     DELETE  otherwise                     0                     e              none
 * row_out = the row, or -1 when the key is not found; for DELETE also -1 when the row was already a tombstone (the rule of
 * pie_token_set_end's rows_out under now = PIE_END_NONE).  user_out and start_out as in pie_token_lookup (undefined for -1);
 * end_out of a key that is not found is PIE_END_NONE.
 * A get or touch that finds its row expired writes nothing: expired rows stay findable and report live = 0, the rule of the
 * whole token index.  That equals the reference's `sessions.delete(hash)` on an expired lookup (:30-33) whenever the clocks of
 * one key's ops do not decrease within the turn: a row found expired at `now` is expired at every later clock.
 * Every write of `end` goes through the path pie_set_end's kernel takes, once per row that ends the turn with another value
 * than it began with: both keys, the hot index and the ordered run stay in step.
 * Cost: one lane per key; the ops of one key are applied by that lane one after another, so a turn in which every op names
 * one token costs k serial steps.
 * Every output pointer may be NULL.  k = 0 is allowed.  Like the other synchronous token calls a turn sees every append, touch
 * and pie_token_append queued before it with no host wait in between; it waits once, bounded by PIE_WAIT_DEADLINE_MS.
 * PIE_E_STATE: no table; no token column; a scan or batch in flight (a turn mutates).  PIE_E_INVAL: NULL ops with k > 0;
 * k >= 2^31; an unknown kind; reserved != 0 — nothing is changed. */
#define PIE_TURN_GET    0
#define PIE_TURN_TOUCH  1
#define PIE_TURN_DELETE 2
typedef struct pie_turn_op {   /* 40 bytes, no padding */
    uint64_t tok[2];           /* key as in pie_token_* */
    int64_t  now;              /* the call's own clock */
    int64_t  new_end;          /* TOUCH only */
    int32_t  kind, reserved;   /* reserved = 0 */
} pie_turn_op;
/* host only, no context, no GPU: the chains the device walks.  next_out[i] = the index of the next op with op i's key, or -1;
 * head_out[i] = 1 iff no earlier op has that key.  One pass through an open-addressed table sized by k.  PIE_E_INVAL: a NULL
 * pointer with k > 0; k >= 2^31.  Kinds and reserved words are not looked at. */
int pie_token_turn_plan(const pie_turn_op *ops, size_t k, int32_t *next_out /* [k] */, uint8_t *head_out /* [k] */);
int pie_token_turn(pie_ctx *ctx, const pie_turn_op *ops, size_t k, int32_t *row_out, uint8_t *live_out, int32_t *user_out,
                   int64_t *start_out, int64_t *end_out);

/* ---- a turn that LOGS IN: createSession (server/sessionStore.js:12-19) joins get / touch / delete as a fourth kind, and the
 * whole ordered list is still one upload, one kernel, one download and one wait.  Only pie_session_turn and its shard and
 * communicator forms (pie_shard_session_turn, pie_comm_session_turn) take the kind: pie_token_turn, pie_token_turn_begin,
 * pie_shard_token_turn, pie_shard_token_turn_begin and pie_comm_token_turn keep refusing it with PIE_E_INVAL.
 * GET, TOUCH and DELETE follow the table above exactly.  A CREATE op carries the key `tok`, start = now, end = new_end, and
 * user[i] / disc[i] (the two arrays are read at CREATE ops only; both may be NULL in a turn without one).
 *     op      condition   row_out        live_out        end_out    start_out  user_out   effect
 *     CREATE  always      the new row    new_end > now   new_end    now        user[i]    a row is appended, its key indexed
 * The j-th CREATE of the array, counting from 0, becomes row rows + j of the table (the host computes it; no device atomic).
 * From that op on the key's row is the new row — the largest row under a key answers — so later ops of the same key in the turn
 * act on the new row, with e = new_end; earlier ops acted on whatever row the key had before, or on none.  A change earlier ops
 * left in the old row's `end` is stored (pie_set_end's path) before the chain moves to the new row.  Two CREATEs of one key
 * both get rows; the later one answers afterwards.  A CREATE with new_end <= now answers live 0 and is findable.
 * The defining equivalence: the table, the token column and index, both keys, the payload, the hot index, later scan results and
 * every output equal those of the calls made one by one, where a CREATE is pie_append_rows of one row followed by
 * pie_token_append of its key and every other op is a pie_token_turn of one op.
 * Room: when the rows, the users (n_users, which may only grow, as in pie_append_rows), the key columns, the token column or
 * the slots (token_rows + creates > slots / 2) have no room in place, the call first makes room the way pie_append_rows and
 * pie_token_append do — a larger table, a key build, a longer column, a rebuild into pie_token_slots_for(new covered) slots —
 * and may wait there; lookups begun in flight land first.  PIE_E_NOMEM there changes nothing.  After that the turn is one
 * upload, one kernel, one download and one wait bounded by PIE_WAIT_DEADLINE_MS.
 * Ordered run: a turn with at least one CREATE drops a valid ordered run (later scans rebuild it or take the general path),
 * unless pie_set_turn_ordered is on and the run can take the rows as it takes an append's (see there); a turn without one treats
 * the run as pie_token_turn does.  A turn without a CREATE is pie_token_turn, plus the growth of the
 * user count to n_users as pie_append_rows(k = 0) does it.  k = 0 is allowed.  Every output pointer may be NULL.
 * PIE_E_STATE: no table; no token column; a sharded context; a scan or batch in flight; a turn begun and not finished; a CREATE
 * while the column does not cover every row (the column is a prefix).  PIE_E_INVAL: NULL context; NULL ops with k > 0;
 * k >= 2^31; a kind outside 0..3; reserved != 0; n_users below the context's user count; a CREATE with NULL user or disc, or
 * with user[i] outside [0, n_users) (checked on the host before anything is staged); a row count reaching 2^31 - 1.
 * On any error nothing is changed. */
#define PIE_TURN_CREATE 3
int pie_session_turn(pie_ctx *ctx, const pie_turn_op *ops, size_t k, const int32_t *user /* [k] */, const int32_t *disc /* [k] */,
                     int32_t n_users, int32_t *row_out, uint8_t *live_out, int32_t *user_out, int64_t *start_out, int64_t *end_out);
/* host only, no context, no GPU: pie_token_turn_plan's chains (next_out, head_out) plus the row every CREATE gets on a table of
 * row0 rows: new_row_out[i] = row0 + j for the j-th CREATE, -1 for every other op; *n_create_out = the number of CREATEs.
 * PIE_E_INVAL: a NULL array with k > 0; k >= 2^31; row0 < 0; a kind outside 0..3 or reserved != 0; row0 + CREATEs reaching
 * 2^31 - 1.  Nothing is written then.  n_create_out may be NULL. */
int pie_session_turn_plan(const pie_turn_op *ops, size_t k, int64_t row0, int32_t *next_out /* [k] */, uint8_t *head_out /* [k] */,
                          int32_t *new_row_out /* [k] */, size_t *n_create_out);

/* ---- the token column of a SHARDED context, by GLOBAL row.  Every shard is given the same call with the same arrays and keeps
 * what is its own; nothing is exchanged (the rule of pie_shard_append_rows / pie_shard_set_end).
 * Coverage: the context remembers covered_g — keys have been given for the global rows [0, covered_g), covered_g <= N_g — and
 * holds the keys of its local rows whose global row lies below it.  The row map ascends, so these are a prefix [0, covered_l) of
 * the local rows, covered_l = lower_bound(row map, local rows, covered_g).  Rows of other shards, and rows this shard's
 * compactions dropped, are skipped silently.  covered_g grows on every shard alike, whether or not the shard kept a key.
 * Slots: the index is sized by the shard's row count, which the host knows (covered_l only the device's row map knows):
 * slots >= pie_token_slots_for(local rows) after every set and append, so it is at most half full; the token append that
 * follows the row count passing half the slots rebuilds it into the next size — the one place an append waits.  Home slot,
 * linear probing, the claim by compare-and-swap and the bounded probe loops with the status word are those of the plain index.
 * pie_compact_rows that drops rows carries the column over as on a plain context: the keys of the kept covered local rows are
 * gathered, covered_g stays, covered_l follows from the new row map, the index is rebuilt; out of memory in that step drops the
 * column and the compaction stands.  Loads, generated tables and pie_shard_table drop the column.
 * The plain calls on a sharded context that has a column: pie_token_append returns PIE_E_STATE (it would break covered_g);
 * pie_token_lookup, pie_token_set_end and pie_token_layout run unchanged, in LOCAL ids.  pie_table_info.token_rows is covered_l.
 * A key held by two shards (the same token given to sessions of users on different shards — a caller error in the reference):
 * each shard answers for itself; pie_comm_token_lookup resolves it.
 * PIE_E_STATE: a context that is not sharded, or whose row map does not cover its rows; no table; no column (all but
 * pie_shard_token_set); a scan or batch in flight.  PIE_E_INVAL: NULL tok with k > 0; keys past N_g. */
/* keys for the global rows [0, n), n <= N_g; replaces any earlier column.  Defined as: an empty column, then
 * pie_shard_token_append of the n keys in chunks of at most 2^20 (no shard needs a device buffer of 16 n bytes).  May wait. */
int pie_shard_token_set(pie_ctx *ctx, const uint64_t *tok /* [n][2] */, size_t n);
/* keys for the global rows [covered_g, covered_g + k); PIE_E_INVAL if that passes N_g.  Queued and un-waited like
 * pie_token_append, except when the column or the slot table must grow. */
int pie_shard_token_append(pie_ctx *ctx, const uint64_t *tok, size_t k);
/* pie_token_lookup with the row and the user as GLOBAL ids (read through the two maps); a key this shard does not hold answers
 * -1 / live 0; of several local rows under one key the largest answers.  Every output pointer may be NULL.  k = 0 is allowed. */
int pie_shard_token_lookup(pie_ctx *ctx, const uint64_t *tok, size_t k, int64_t now, int32_t *row_global_out, uint8_t *live_out,
                           int32_t *user_global_out, int64_t *start_out, int64_t *end_out);
/* one lookup, then pie_set_end's own path on the local rows found live (exactly how pie_token_set_end composes: repeats, both
 * keys, the hot index and the ordered run stay in step).  rows_global_out[i] (may be NULL) = the global row written or -1. */
int pie_shard_token_set_end(pie_ctx *ctx, const uint64_t *tok, const int64_t *new_end, size_t k, int64_t now, int32_t *rows_global_out);
/* pie_token_turn on this shard's column: the same rules and the same single launch, the row and the user answered as GLOBAL ids
 * (read through the two maps, as pie_shard_token_lookup reads them).  A key this shard does not hold answers -1 / live 0 /
 * PIE_END_NONE for every op of its chain, and the chain changes nothing. */
int pie_shard_token_turn(pie_ctx *ctx, const pie_turn_op *ops, size_t k, int32_t *row_global_out, uint8_t *live_out,
                         int32_t *user_global_out, int64_t *start_out, int64_t *end_out);
/* pie_session_turn on this shard of a sharded table: the turn that LOGS IN, given to every shard with the same arrays (GLOBAL user
 * ids in user_global[], read at CREATE ops only; n_users_global may only grow).  GET, TOUCH and DELETE answer as
 * pie_shard_token_turn.  The j-th CREATE of the array, counting from 0, becomes GLOBAL row N_g + j on every shard; the shard with
 * pie_shard_of(user, world) == rank keeps the row, as LOCAL row local rows + (the CREATEs it kept before that one).  All of this
 * is host arithmetic (pie_shard_session_turn_plan); there is no device atomic and nothing is exchanged.
 *     op      on the shard that      row_global_out   live_out        end_out       start_out  user_global_out
 *     CREATE  keeps the row          N_g + j          new_end > now   new_end       now        user_global[i]
 *     CREATE  does not keep it       -1               0               PIE_END_NONE  0          -1
 * On the shard that keeps it, later ops of the key act on the new row, and a change earlier ops left in the old row's `end` is
 * stored first (pie_session_turn's rule).  On a shard that does not, the chain goes on with whatever row the key had there: the
 * rule for a key held by two shards above.
 * The defining equivalence, per shard: every output, the table, the row map, the user map, the token column (covered_g,
 * covered_l, keys, slots), both key columns, the payload, the hot index and later scans equal those of the same ops made one by
 * one on that shard, where a CREATE is pie_shard_append_rows of one row (n_users_global) followed by pie_shard_token_append of its
 * key and every other op is a pie_shard_token_turn of one op.  Afterwards N_g and covered_g have grown by the number of CREATEs
 * on every shard alike.
 * Room, with the shard's own sizes: local rows + kept CREATEs against the capacity of the columns; its users, after the new ones
 * it owns, against the capacity of the user arrays (both maps grow with the table); a longer token column; the slots
 * (local rows + kept > slots / 2) rebuilt into pie_token_slots_for of that count.  Lookups begun in flight land first; the call
 * may wait there.  The shard's new users go behind the device user map in stream order, ahead of the kernel.  After that the
 * turn is one upload, one kernel, one download and one wait bounded by PIE_WAIT_DEADLINE_MS — also on a shard that keeps no
 * CREATE and holds none of the keys, which still runs its chains.  With k = 0, or no CREATE and no new user, the call is
 * pie_shard_token_turn; a turn without a CREATE that grows n_users_global is pie_shard_append_rows(k = 0) followed by the turn.
 * Ordered run: a turn in which the shard keeps a CREATE drops its valid ordered run (with pie_set_turn_ordered on for the shard's
 * context: keeps it where an append of those rows would, in the shard's own LOCAL numbers); any other turn keeps it in step.
 * PIE_E_STATE: a context that is not sharded, or whose row map does not cover its rows; no table; no column; a scan or batch in
 * flight; a turn begun and not finished; a CREATE while covered_g < N_g.  PIE_E_INVAL: NULL context; NULL ops with k > 0;
 * k >= 2^31; a kind outside 0..3; reserved != 0; n_users_global below the table's; a CREATE with NULL user_global or disc, or with
 * a user outside [0, n_users_global) (checked on the host before anything is staged); N_g + CREATEs reaching 2^31 - 1.  On any
 * error nothing is changed.  Every output pointer may be NULL.  pie_session_turn keeps refusing sharded contexts, and
 * pie_shard_token_turn, pie_shard_token_turn_begin and pie_comm_token_turn keep refusing the kind. */
int pie_shard_session_turn(pie_ctx *ctx, const pie_turn_op *ops, size_t k, const int32_t *user_global /* [k] */,
                           const int32_t *disc /* [k] */, int32_t n_users_global, int32_t *row_global_out, uint8_t *live_out,
                           int32_t *user_global_out, int64_t *start_out, int64_t *end_out);
/* host only, no context, no GPU: pie_token_turn_plan's chains plus the rows every CREATE gets on shard `rank` of `world`, on a
 * table of rows_global0 rows of which the shard holds rows_local0: new_row_global_out[i] = rows_global0 + j for the j-th CREATE,
 * new_row_local_out[i] = rows_local0 + (the CREATEs before it that the shard keeps) when pie_shard_of(user_global[i], world) ==
 * rank, -1 otherwise and for every other op.  *n_create_out = the CREATEs, *n_kept_out = those the shard keeps (either may be
 * NULL).  PIE_E_INVAL: a NULL array with k > 0 (user_global only when there is a CREATE); k >= 2^31; a negative row count or
 * rows_local0 > rows_global0; rank outside [0, world); a kind outside 0..3 or reserved != 0; rows_global0 + CREATEs reaching
 * 2^31 - 1.  Nothing is written then. */
int pie_shard_session_turn_plan(const pie_turn_op *ops, size_t k, const int32_t *user_global /* [k] */, int64_t rows_global0,
                                int64_t rows_local0, int32_t rank, int32_t world, int32_t *next_out /* [k] */,
                                uint8_t *head_out /* [k] */, int32_t *new_row_global_out /* [k] */,
                                int32_t *new_row_local_out /* [k] */, size_t *n_create_out, size_t *n_kept_out);
/* tests and tools: covered_g, covered_l, slots; slot_row_out[cap] (local rows; PIE_E_CAPACITY if cap < slots);
 * tok_out[covered_l][2]; any may be NULL.  Waits. */
int pie_shard_token_layout(pie_ctx *ctx, size_t *covered_global_out, size_t *covered_local_out, size_t *slots_out,
                           int32_t *slot_row_out, size_t cap, uint64_t *tok_out);

/* ---- token lookups WHILE SCANS AND BATCHES ARE IN FLIGHT.  A lookup only reads (the token column, the slots, end, start, user);
 * scans and batches only read the table; every mutator is refused while they are in flight.  So these calls are allowed whenever
 * the context has a table and a token column, whatever is in flight: single scans, batches on any lane, wide batches, batches on
 * the ordered run, or nothing.  pie_token_lookup and the other synchronous calls keep their rules (PIE_E_STATE in flight).
 * Up to 4 lookups may be begun and not finished; they finish in the order they were begun.  Each owns a slot: pinned and device
 * staging and status words of its own, so the probe-bound report of one lookup is neither raised nor cleared by another call.
 * Clock: now[i] belongs to key i (the requests of a turn carry their own Date.now()): live_out[i] = found && end[row] > now[i].
 * What a lookup sees: the table after every append, touch, delete and pie_token_append queued on the context before its begin,
 * with no host wait in between.  A mutator issued between its begin and its finish does not change its answer: that mutator's
 * device work is ordered behind the lookup.  Calls that replace or free what a lookup reads (pie_load_columns*,
 * pie_gen_synthetic*, pie_shard_table, pie_compact_rows, pie_token_set / pie_shard_token_set, an index rebuild or a longer
 * column in pie_token_append / pie_shard_token_append, capacity growth in pie_append_rows / pie_shard_append_rows,
 * pie_ctx_destroy) first wait on the host for the lookups begun; the results stay readable by finish, in the ids of the table
 * the lookup was begun on.
 * Waiting: the lookup runs on a stream of its own, ordered behind the context's stream only by an event recorded at begin.
 * Neither call synchronises the context's stream or a lane's; finish polls the lookup's own event, bounded by
 * PIE_WAIT_DEADLINE_MS like the wait on a scan summary (PIE_E_HIP past it; the slot is returned).
 * PIE_E_STATE: no table; no token column; a fifth begin with four unfinished; finish with none begun, or by the other form
 * than the begin; the shard form on a context that is not sharded.  PIE_E_INVAL: NULL tok or NULL now with k > 0; k >= 2^31.
 * PIE_E_CAPACITY: cap < k — *k_out is set and the lookup stays finishable with a larger buffer.  k = 0 takes and returns a
 * slot like any other lookup.  *k_out (may be NULL) = keys of the lookup; every output pointer may be NULL. */
int pie_token_lookup_begin(pie_ctx *ctx, const uint64_t *tok /* [k][2] */, const int64_t *now /* [k] */, size_t k);
int pie_token_lookup_finish(pie_ctx *ctx, int32_t *row_out, uint8_t *live_out, int32_t *user_out, int64_t *start_out,
                            int64_t *end_out, size_t cap, size_t *k_out);
/* lookups pie_token_lookup_begin (either form) would take now: 4 less those unfinished */
int pie_token_lookup_room(pie_ctx *ctx);
/* the same on a sharded context's column: rows and users answered as GLOBAL ids, as pie_shard_token_lookup answers them */
int pie_shard_token_lookup_begin(pie_ctx *ctx, const uint64_t *tok /* [k][2] */, const int64_t *now /* [k] */, size_t k);
int pie_shard_token_lookup_finish(pie_ctx *ctx, int32_t *row_global_out, uint8_t *live_out, int32_t *user_global_out,
                                  int64_t *start_out, int64_t *end_out, size_t cap, size_t *k_out);

/* ---- token TURNS WHILE SCANS AND BATCHES ARE IN FLIGHT: touchSession on every authenticated request (server/sessionStore.js:
 * 37-45) without draining the pipeline.  The ops, the results and the effect on the table are exactly pie_token_turn's (the
 * table at PIE_TURN_GET / TOUCH / DELETE above); the shard form answers rows and users as GLOBAL ids, as pie_shard_token_turn.
 * Allowed whenever the context has a table and a token column, whatever is in flight: single scans, batches on any lane, batches
 * whose union tail still rides, wide batches, in-flight lookups, the in-flight expired queue, or nothing.
 * Slots: up to 4 turns may be begun and not finished; they finish in the order they were begun.  Each owns its pinned and device
 * staging, its status words and its event; nothing is shared with pie_token_turn or pie_token_lookup.  The staging of a slot grows
 * only when a begin brings more ops than the slot has held before.
 * Visibility is QUEUE ORDER, not the moment of finish:
 *   - a scan, batch or wide batch begun before pie_token_turn_begin answers for the table before the turn;
 *   - one begun after it sees every write of the turn; two turns apply in begin order;
 *   - pie_token_lookup_begin / pie_expired_queue_begin issued after it see it, those issued before it do not;
 *   - the exception: a query that a batch's finish reruns on the general path (a dense query, a union bucket that outgrew its
 *     slots: see pie_scan_batch_begin) is answered for the table as it stands at that finish.
 * How: the turn's kernel runs on the context's stream.  Begin first launches every union tail that still waits for a launch
 * (what pie_scan_batch_flush does: a tail rebuilds the masks from the table), makes the context's stream wait for an event on
 * every lane that has a batch in flight, queues the turn, and records one event behind it that every lane's next begin waits for
 * once.  There is no host wait in begin.  The lanes stand still for the length of the turn's kernel.
 * Waiting: finish waits once, for the turn's own event, bounded by PIE_WAIT_DEADLINE_MS (PIE_E_HIP past it; the slot is
 * returned).  It never waits on the context's stream or a lane's.
 * The ordered run: on a context whose ordered run is valid begin returns PIE_E_STATE.  The host sees the run's stale flag (a row
 * outside the run came back to life) only at a wait, so a batch begun between begin and finish could read a stale run.
 * pie_token_turn keeps serving such a table.
 * The other calls: pie_token_turn, pie_token_set, pie_token_append, pie_token_set_end, pie_append_rows, pie_set_end,
 * pie_delete_user(s), pie_prune_before, pie_retention_purge*, pie_expired_queue and every pie_shard_* call that checks the
 * shard's state return PIE_E_STATE while a turn is begun and not finished, besides their rule for scans and batches.  Calls
 * that replace or free the table, the token column or a shard's maps (loads, pie_gen_synthetic*, pie_shard_table,
 * pie_compact_rows, pie_ctx_destroy) first wait on the host for the turns begun; their results stay readable by finish, in the
 * ids of the table they were begun on.
 * PIE_E_STATE: no table; no token column; an ordered run that is valid; a fifth begin with four unfinished (no slot is taken);
 * finish with none begun, or by the other form than the begin; the shard form on a context that is not sharded or whose row map
 * does not cover its rows.  PIE_E_INVAL: pie_token_turn's cases (NULL context; NULL ops with k > 0; k >= 2^31; an unknown kind;
 * reserved != 0) — nothing is changed.  PIE_E_CAPACITY: cap < k at finish — *k_out is set and the turn stays begun.  *k_out (may
 * be NULL) = ops of the turn; every output pointer may be NULL.  k = 0 takes and returns a slot and queues nothing.
 * pie_token_turn_room: turns a begin (either form) would take now, 4 less those unfinished; PIE_E_INVAL for a NULL context.
 * There is no pie_comm_* form. */
int pie_token_turn_begin(pie_ctx *ctx, const pie_turn_op *ops, size_t k);
int pie_token_turn_finish(pie_ctx *ctx, int32_t *row_out, uint8_t *live_out, int32_t *user_out, int64_t *start_out,
                          int64_t *end_out, size_t cap, size_t *k_out);
int pie_token_turn_room(pie_ctx *ctx);
int pie_shard_token_turn_begin(pie_ctx *ctx, const pie_turn_op *ops, size_t k);
int pie_shard_token_turn_finish(pie_ctx *ctx, int32_t *row_global_out, uint8_t *live_out, int32_t *user_global_out,
                                int64_t *start_out, int64_t *end_out, size_t cap, size_t *k_out);

/* ---- the expired queue WHILE SCANS AND BATCHES ARE IN FLIGHT.  pie_expired_queue borrows the scan slots' workspace and is
 * refused in flight; this form has a stream, scratch, a queue buffer and a summary of its own, and only reads the table.  So the
 * calls are allowed whenever the context has a table, whatever is in flight: single scans, batches on any lane, wide batches,
 * batches on the ordered run, token lookups, or nothing.  pie_expired_queue keeps its rules.
 * Result: exactly the queue pie_expired_queue(prev_now, now) returns on the same table — ascending rows with
 * prev_now < end <= now (prev_now >= now: empty).  The shard form answers in GLOBAL rows through the shard's row map.
 * One queue may be begun and not finished.  It touches neither the scan slots, nor the finished scan's or batch's result and its
 * readers, nor the queue pie_queue_info / pie_queue_pack_device / pie_comm_*_queue know, nor the profiling ring, nor pie_stats.
 * What it sees: the table after every append, touch and delete queued on the context before its begin, with no host wait.  A
 * mutator issued between begin and finish does not change the answer: its device work is ordered behind the pass.  Calls that
 * replace or free what the pass reads (pie_load_columns*, pie_gen_synthetic*, pie_shard_table, pie_compact_rows, capacity growth
 * in pie_append_rows / pie_shard_append_rows, a rebuild of the key columns, pie_ctx_destroy) first wait on the host for it; the
 * result stays readable by finish, in the ids of the table it was begun on.
 * Buffer: the pass writes into a device buffer of its own, cap_rows x 4 B, kept between calls and reallocated only when a begin
 * asks for more.  cap_rows = 0 counts only.  *q_out (may be NULL) is always the true length.
 *   finish with queue_out != NULL and cap < the begin's cap_rows: PIE_E_INVAL, nothing consumed.
 *   a queue longer than cap_rows (> 0): its first cap_rows rows are copied — a true ascending prefix — and finish returns
 *   PIE_E_CAPACITY with *q_out set; the pass is consumed, the caller begins again with room.
 * Waiting: the pass runs on a stream of its own, ordered behind the context's stream only by an event recorded at begin.
 * Neither call synchronises the context's stream or a lane's; finish polls the pass's summary word, bounded by
 * PIE_WAIT_DEADLINE_MS (PIE_E_HIP past it; the pass is consumed).
 * PIE_E_STATE: no table; a second begin; finish with none begun, or by the other form than the begin; the shard form on a
 * context that is not sharded or whose row map does not cover its rows.  PIE_E_INVAL: NULL context; cap_rows >= 2^31.
 * An empty table gives PIE_OK and an empty queue. */
int pie_expired_queue_begin(pie_ctx *ctx, int64_t prev_now, int64_t now, size_t cap_rows);
int pie_expired_queue_finish(pie_ctx *ctx, int32_t *queue_out, size_t cap, size_t *q_out);
/* queues pie_expired_queue_begin (either form) would take now: 1 or 0; PIE_E_INVAL for a NULL context */
int pie_expired_queue_room(pie_ctx *ctx);
int pie_shard_expired_queue_begin(pie_ctx *ctx, int64_t prev_now, int64_t now, size_t cap_rows);
int pie_shard_expired_queue_finish(pie_ctx *ctx, int32_t *rows_global_out, size_t cap, size_t *q_out);
/* Host only, for tests: how the pass cuts a table of n rows on this context's device — the rows a wave reads per step, the rows
 * of a unit (the contiguous range one wave walks alone; the pass has ceil(n / rows_per_unit) of them) and the blocks of its
 * grid (four waves each, units taken grid-stride).  Any output may be NULL.  PIE_E_INVAL: NULL context, n >= 2^31 - 1. */
int pie_expired_inflight_geometry(pie_ctx *ctx, size_t n, int32_t *rows_per_wave_step_out, int64_t *rows_per_unit_out,
                                  int32_t *blocks_out);

/* Host only, no context, no GPU: what the batched pass stores per selected row. A row's 64-bit query mask is
 * live[r] & win[w] & disc[d] (r: queries whose `now` lies below the row's end, w: queries whose cutoff is <= its start, d: its
 * discipline), so the pass keeps the 20-bit code r | w << 7 | d << 14 in the row's bucket slot and the tail expands it through
 * the batch's tables.  For every given row: code_out = that code, mask_out = the code expanded through the tables the host
 * builds for these queries (bit q = query q selects the row; queries marked in fallback[], which may be NULL, are left out of
 * the tables).  Either output may be NULL.  For tests. */
int pie_batch_mask_codes(const pie_query *queries, int n_q, const uint8_t *fallback, int32_t n_disc, const int64_t *start,
                         const int64_t *end, const int32_t *disc, size_t n_rows, uint32_t *code_out, uint64_t *mask_out);

/* ---- communicator: the sharded table behind the C ABI (SURVEY.md 8b "pie_ctx_create(device_ids[], n, ...)", 8e) --------
 * A pie_comm owns one scan context per GPU and one RCCL communicator; the session table is sharded by user hash
 * (pie_shard_of) and the cross-user reassembly — every rank receives every rank's per-user offsets and row lists — is an
 * all-gather done as grouped ncclSend / ncclRecv over the point-to-point xGMI links.  This is what lets a host that is not
 * Python (the Node addon) use more than one GPU.  RCCL is opened at run time; without it pie_comm_create fails with
 * PIE_E_NODEVICE.  Two ways to build one:
 *   pie_comm_create        one process drives all n GPUs of the node (ncclCommInitAll): the Node host;
 *   pie_comm_create_rank   one process per GPU (ncclCommInitRank): rank 0 makes the 128-byte id with pie_comm_unique_id
 *                          and hands it to the other ranks by whatever channel the host has. */
typedef struct pie_comm pie_comm;
int pie_comm_create(const int32_t *device_ids, int32_t n, pie_comm **comm_out);
int pie_comm_unique_id(void *id_out_128);
int pie_comm_create_rank(const void *id_128, int32_t rank, int32_t world, int32_t device_id, pie_comm **comm_out);
int pie_comm_destroy(pie_comm *comm);
/* comm may be NULL: the last error of a failed pie_comm_create* on this thread */
const char *pie_comm_last_error(const pie_comm *comm);
int32_t pie_comm_world(const pie_comm *comm);
int32_t pie_comm_local_ranks(const pie_comm *comm);
/* The scan context of shard `rank` (NULL when that rank lives in another process): load / shard / touch / scan it through
 * the ordinary entry points.  Owned by the communicator. */
pie_ctx *pie_comm_ctx(pie_comm *comm, int32_t rank);
/* Every local shard generates the synthetic corpus on its own GPU and keeps the rows of its users (pie_gen_synthetic +
 * pie_shard_table): the sharded form of BASELINE.json configs[3]. */
int pie_comm_gen_synthetic_sharded(pie_comm *comm, uint64_t seed, int64_t n_total, int32_t n_users, int32_t n_disc, uint32_t flags);
/* One synchronous step, per-query lists: every local shard runs ONE batched scan of the n_q queries and leaves its n_q result
 * messages ([off[0..u_pad] | M | rows], pie_pack_results_device's layout); the messages are exchanged (direct pattern: one
 * send and one receive per peer inside one ncclGroup); returns when every local rank holds all world x n_q messages.
 * u_pad: 0 in a single-process communicator (the largest shard's user count is used); in a process-per-GPU communicator
 * the value every rank agreed on, with the row capacity reserved beforehand (pie_comm_reserve) — the message length must be
 * the same everywhere.  m_out (may be NULL): local_ranks x n_q selected-row counts.
 * The exchange always runs (a list longer than the capacity is truncated, M stays in its header); the capacity check is made
 * on the gathered headers, so EVERY rank returns PIE_E_CAPACITY together: reserve pie_comm_needed_cap() and repeat. */
int pie_comm_scan_batch_gather(pie_comm *comm, const pie_query *queries, int32_t n_q, int32_t u_pad, size_t *m_out);
int pie_comm_reserve(pie_comm *comm, int32_t n_q, int32_t u_pad, size_t idx_cap);
/* Rows to reserve after PIE_E_CAPACITY (the largest list / union any rank reported, with headroom): the same on every rank. */
size_t pie_comm_needed_cap(const pie_comm *comm);
/* The gathered messages as rank `at_rank` holds them: device pointer and strides (words), or one message copied to the host. */
int pie_comm_gathered_device_ptr(pie_comm *comm, int32_t at_rank, void **base_out, size_t *rank_stride_words,
                                 size_t *query_stride_words, size_t *u_pad_out);
int pie_comm_read_gathered(pie_comm *comm, int32_t at_rank, int32_t src_rank, int32_t qi, int32_t *offsets_out /* u_pad + 1 */,
                           int32_t *idx_out, size_t idx_cap, size_t *m_out);
/* Cross-shard dispatch queues: every local shard computes its own queue (pie_expired_queue / pie_archive_queue), packs it
 * (pie_queue_pack_device's layout), the messages are exchanged (direct pattern) and merged on every rank's device into the
 * one queue of the unsharded table: the ascending global rows with prev_now < end <= now, or the archive queue (groups = users,
 * each on one rank, ordered by the global row of their first queued row; rows in table order).  Two header words per rank
 * (rows, groups) are exchanged first and size the messages; a rank whose local step failed sends {-1, status} and EVERY rank
 * returns that status (the lowest failing rank's), with nothing left waiting in ncclSend / ncclRecv.  PIE_E_STATE while
 * pipelined steps are uncollected.  Every rank of a process-per-GPU communicator makes the same calls in the same order.
 * queue_out (may be NULL) receives the global rows as the first local rank holds them; *q_out = the total on every rank;
 * PIE_E_CAPACITY (with *q_out set) if cap is below it.  The merged queue stays with the communicator until the next call:
 * pie_comm_queue_read copies it as a local rank holds it (global row, source rank, source local row; any output may be NULL),
 * pie_comm_queue_device_ptrs hands out the device arrays. */
int pie_comm_expired_queue(pie_comm *comm, int64_t prev_now, int64_t now, int32_t *queue_out, size_t cap, size_t *q_out);
int pie_comm_archive_queue(pie_comm *comm, int64_t now, int64_t window_ms, int32_t *queue_out, size_t cap, size_t *q_out);
int pie_comm_queue_read(pie_comm *comm, int32_t at_rank, int32_t *rows_out, int32_t *src_rank_out, int32_t *src_row_out,
                        size_t cap, size_t *q_out);
int pie_comm_queue_device_ptrs(pie_comm *comm, int32_t at_rank, void **rows_dev, void **src_rank_dev, void **src_row_dev,
                               size_t *q_out);
/* Device time of the phases of the last queue call on the first local rank's stream (ms): [0] local queue + header exchange,
 * [1] pack, [2] payload exchange, [3] merge.  After pie_comm_prune_before / pie_comm_retention_purge* (kind
 * PIE_COMM_QUEUE_MAINT): [0] the shards' list passes, [1] the copies of lists held on other devices, [2] 0 (nothing is
 * exchanged), [3] the merge kernel. */
int pie_comm_queue_timing(pie_comm *comm, float *ms_out_4);
/* Which call left the merged queue the readers above answer from. */
#define PIE_COMM_QUEUE_NONE    0
#define PIE_COMM_QUEUE_EXPIRED 1 /* pie_comm_expired_queue */
#define PIE_COMM_QUEUE_ARCHIVE 2 /* pie_comm_archive_queue */
#define PIE_COMM_QUEUE_MAINT   3 /* pie_comm_prune_before / pie_comm_retention_purge / pie_comm_retention_purge_tz: the rows the call
                                    tombstoned; held by the FIRST local rank only (the readers refuse another at_rank: PIE_E_STATE) */
int pie_comm_queue_kind(const pie_comm *comm);

/* ---- a live sharded table behind the communicator: pie_shard_append_rows / pie_shard_set_end / pie_shard_delete_user on every
 * local shard, with GLOBAL ids throughout.  Nothing is exchanged: every process of a process-per-GPU communicator makes the
 * same call with the same arrays.  Every local shard checks the call before any is changed, so a refused call changes none.
 * PIE_E_STATE while pipelined steps of either kind are uncollected, and when the local shards disagree on the table's size.
 * pie_comm_append_rows: *first_row_out = the table's row count before the call.  n_users may grow; that can raise the largest
 * shard's user count, and the reservations of pie_comm_step_reserve / pie_comm_wide_step_reserve are then the caller's to renew,
 * as after any table change (u_pad = 0 in pie_comm_scan_batch_gather follows by itself).
 * pie_comm_delete_user: rows_out / *n_deleted are filled by the process that drives the owning rank; *owner_rank_out =
 * pie_shard_of(user, world) (-1 for an id outside [0, users)); other processes report n_deleted = 0.
 * pie_comm_table_size: rows and users of the whole table. */
int pie_comm_append_rows(pie_comm *comm, const int64_t *start, const int64_t *end, const int32_t *user, const int32_t *disc, size_t k,
                         int32_t n_users, int32_t *first_row_out);
int pie_comm_set_end(pie_comm *comm, const int32_t *rows, const int64_t *new_end, size_t k);
int pie_comm_delete_user(pie_comm *comm, int32_t user, int32_t *rows_out, size_t cap, size_t *n_deleted, int32_t *owner_rank_out);
/* pie_shard_delete_users with the whole id list on every local shard: rows_out = the per-shard lists merged into ONE ascending
 * list of global rows, per_user_out[i] summed over the local shards, owner_rank_out[i] (may be NULL) = pie_shard_of(users[i],
 * world), -1 for an id outside [0, users).  A process reports what its own shards held, as pie_comm_delete_user. */
int pie_comm_delete_users(pie_comm *comm, const int32_t *users, size_t k, int32_t *rows_out, size_t cap, size_t *n_deleted,
                          int32_t *per_user_out /* [k] */, int32_t *owner_rank_out /* [k] */);
int pie_comm_table_size(pie_comm *comm, int64_t *rows_global_out, int32_t *users_global_out);
/* A sharded table that ages: _pruneCalendarEvents (server/storage/sqlProvider.js:956-968), _purgeExpiredArchives /
 * _isArchiveExpired / _addMonths (:863-890, 991-1009) and the removal of dead rows (`sessions.delete()`, server/sessionStore.js:
 * 47-53) behind the communicator.  The rules above hold: PIE_E_STATE while pipelined steps of either kind are uncollected or the
 * local shards disagree on the table's size; every local shard checks the call before any is changed; nothing is exchanged, and
 * in a process-per-GPU communicator every process makes the same call and reports what its own shards held.  Token lookups and
 * an expired queue begun on a shard's side stream land as under the shard's own calls.
 * The three lists: every local shard runs its shard form (pie_shard_prune_before ...) with the list left on its device; the
 * lists are merged ON THE DEVICE of the first local rank (lists held on other devices are copied over first) into ONE ascending
 * list of global rows.  rows_out (may be NULL) receives it, *n_out its length; a cap below it returns PIE_E_CAPACITY with *n_out
 * set, the rows tombstoned all the same.  Either way the merged list stays with the communicator as a queue of kind
 * PIE_COMM_QUEUE_MAINT: pie_comm_queue_read / pie_comm_queue_device_ptrs (at_rank = the first local rank) give global row,
 * source rank and source local row, pie_comm_queue_timing its device times.
 * pie_comm_compact_rows: pie_compact_rows(dead_before, flags) on every local shard; *kept_total_out = the kept rows of the local
 * shards, kept_local_out[i] (may be NULL) those of the i-th local shard.  Global rows are NOT renumbered: the table keeps its
 * N_g, the next pie_comm_append_rows starts there, every pie_comm_* call keeps naming and reporting the original global rows,
 * and a global row that was dropped behaves as a row no shard holds (pie_comm_set_end skips it, token lookups answer -1; token
 * columns are carried over as pie_compact_rows does).  A merged queue the communicator held is forgotten (its source rows named
 * the old numbering).  Reservations of pie_comm_step_reserve / pie_comm_wide_step_reserve are the caller's to renew afterwards,
 * as after any table change.  If a shard fails part-way (PIE_E_NOMEM), that status is returned and the shards before it stay
 * compacted: that is a valid table, because global ids do not move; *kept_total_out and kept_local_out cover the shards done. */
int pie_comm_prune_before(pie_comm *comm, int64_t cutoff, int32_t *rows_out, size_t cap, size_t *n_out);
int pie_comm_retention_purge(pie_comm *comm, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t *rows_out, size_t cap,
                             size_t *n_out);
int pie_comm_retention_purge_tz(pie_comm *comm, int64_t now, int32_t months, const int64_t *transitions_utc_ms, const int64_t *offsets_ms,
                                int32_t n_transitions, int32_t *rows_out, size_t cap, size_t *n_out);
int pie_comm_compact_rows(pie_comm *comm, int64_t dead_before, uint32_t flags, size_t *kept_total_out,
                          size_t *kept_local_out /* [local ranks], may be NULL */);
/* The token column behind the communicator (pie_shard_token_* on every local shard; the rules above hold: PIE_E_STATE while
 * pipelined steps are uncollected, every local shard checks a call before any is staged or changed).
 * pie_comm_token_lookup queues the lookup on every local shard, then waits for each, and merges on the host: per key the answer
 * with the LARGEST global row (-1 / live 0 if no local shard holds the key) with its live / user / start / end (global ids);
 * owner_rank_out[i] (may be NULL) = the rank that answered, -1 if none.  This is the unsharded table's answer, a key held by
 * two shards included.  In a process-per-GPU communicator a process reports what its own shards hold, as pie_comm_delete_user.
 * pie_comm_token_set_end: that lookup, then ONE pie_comm_set_end by global row of the elements whose winner is live under `now`
 * (PIE_END_NONE: every winner that is not a tombstone) — the unsharded pie_token_set_end's result, repeats included.
 * rows_out[i] (may be NULL) = the global row written or -1. */
int pie_comm_token_set(pie_comm *comm, const uint64_t *tok /* [n][2] */, size_t n);
int pie_comm_token_append(pie_comm *comm, const uint64_t *tok, size_t k);
int pie_comm_token_lookup(pie_comm *comm, const uint64_t *tok, size_t k, int64_t now, int32_t *row_out, uint8_t *live_out,
                          int32_t *user_out, int64_t *start_out, int64_t *end_out, int32_t *owner_rank_out);
int pie_comm_token_set_end(pie_comm *comm, const uint64_t *tok, const int64_t *new_end, size_t k, int64_t now, int32_t *rows_out);
/* pie_token_turn across the local shards: every local shard is given the same turn (pie_shard_token_turn); all are checked before
 * any is changed and all are queued before any is waited for.  Per op the answer comes from the shard with the LARGEST global row
 * (pie_comm_token_lookup's merge), owner_rank_out[i] (may be NULL) = its rank, -1 if no local shard holds the key.  With every
 * key held by one shard — tokens are 48 random bytes — this is the unsharded pie_token_turn's result.  A key held by two shards
 * (a caller error in the reference) has its chain applied by each shard to its own latest row.  PIE_E_STATE while pipelined steps
 * are uncollected; PIE_E_INVAL as pie_token_turn. */
int pie_comm_token_turn(pie_comm *comm, const pie_turn_op *ops, size_t k, int32_t *row_out, uint8_t *live_out,
                        int32_t *owner_rank_out, int32_t *user_out, int64_t *start_out, int64_t *end_out);
/* pie_session_turn across the local shards: every local shard is given the same turn (pie_shard_session_turn), user[] and n_users
 * in GLOBAL ids.  All local shards are checked before any is changed, room is made on all of them before any is queued, and all
 * are queued before any is waited for.  Per op the answer comes from the shard with the largest global row (pie_comm_token_turn's
 * merge), owner_rank_out likewise; a CREATE is kept by one shard, which answers it.  With every key held by one shard this is the
 * unsharded pie_session_turn's result; afterwards the table is N_g + CREATEs rows long on every shard.  In place of the three
 * calls a login cost before (pie_comm_append_rows of one row, pie_comm_token_append of its key, pie_comm_token_turn of the rest).
 * PIE_E_STATE while pipelined steps of either kind are uncollected, when the local shards disagree on N_g, and as
 * pie_shard_session_turn; PIE_E_INVAL as pie_shard_session_turn.  An error changes no shard. */
int pie_comm_session_turn(pie_comm *comm, const pie_turn_op *ops, size_t k, const int32_t *user /* [k] */, const int32_t *disc /* [k] */,
                          int32_t n_users, int32_t *row_out, uint8_t *live_out, int32_t *owner_rank_out, int32_t *user_out,
                          int64_t *start_out, int64_t *end_out);

/* ---- the pipelined exchange: ONE union message per step (layout: pie_scan_batch_begin_union), written by each shard's own
 * batch kernels; the exchange of step i runs on a side stream while the shards scan steps i+1, i+2.  Order of calls:
 *     step_reserve;  begin(0); begin(1); finish(0); begin(2); collect(0); finish(1); begin(3); collect(1); ...
 * at most three steps per batch lane of the shards (pie_set_batch_lanes: 3 .. 12) begun and unfinished, at most sixteen
 * uncollected (rotating buffer sets).  Every rank of a process-per-GPU communicator makes the same calls in the same order.
 * These rules hold for the ordinary steps here and for the wide steps below alike (one engine runs both):
 *   - geometry: u_pad, union_cap and the words per row of a reservation belong to the kind of step alone.  Neither the other
 *     kind's reservation nor the synchronous path (pie_comm_reserve, pie_comm_scan_batch_gather) moves them; they change only
 *     in step_reserve, and only while no step of the kind is in flight (PIE_E_STATE otherwise).
 *   - begin: if a local shard cannot begin after others began, every step in flight on this process is finished and marked
 *     failed (its collect returns PIE_E_STATE) together with what this call began; the step is not counted.
 *   - waits: collect waits for the side stream at most PIE_WAIT_DEADLINE_MS (20 000 ms by default), then fails with PIE_E_HIP.
 *   - a step that failed on this process (a shard's finish, the exchange, the wait) says so at its collect (PIE_E_STATE, or the
 *     wait's own status), and its gathered buffers are never handed out.
 *   - buffer lifetime: the gathered messages of a collected step stay valid until as many further steps have BEGUN as there
 *     are buffer sets — sixteen here, eight for wide steps; gathered_ptr / read_gathered return PIE_E_STATE before the step's
 *     collect, after that point, and for a failed step.  A step whose collect returned PIE_E_CAPACITY is not a failed step.
 * step_reserve: u_pad as in pie_comm_scan_batch_gather; union_cap = rows per message.
 * step_finish:  waits for the oldest begun step's summaries on every local shard (m_out: local_ranks x n_q, may be NULL),
 *               then queues its exchange; does not wait for it.
 * step_collect: waits for the oldest queued exchange (side stream only); *step_out = its step number (0, 1, 2, ...).
 *               PIE_E_CAPACITY — on every rank alike, from the gathered Mu words — when a union outgrew union_cap (reserve
 *               pie_comm_needed_cap() once nothing is in flight, repeat) or could not be formed at all (Mu = -1). */
int pie_comm_step_reserve(pie_comm *comm, int32_t n_q, int32_t u_pad, size_t union_cap);
int pie_comm_step_begin(pie_comm *comm, const pie_query *queries, int32_t n_q);
int pie_comm_step_finish(pie_comm *comm, size_t *m_out);
int pie_comm_step_collect(pie_comm *comm, int64_t *step_out);
/* The gathered union messages of a collected step as rank `at_rank` holds them (valid until sixteen more steps have begun):
 * message of rank r at base + r * rank_stride_words; or one message copied to the host (masks_out: 64-bit mask per row; Mu comes
 * from the words collect already holds, no extra copy). */
int pie_comm_step_gathered_ptr(pie_comm *comm, int32_t at_rank, int64_t step, void **base_out, size_t *rank_stride_words,
                               size_t *u_pad_out, size_t *cap_out);
int pie_comm_step_read_gathered(pie_comm *comm, int32_t at_rank, int32_t src_rank, int64_t step, int32_t *uoff_out /* u_pad + 1 */,
                                int32_t *rows_out, uint64_t *masks_out, size_t cap, size_t *mu_out);

/* ---- the pipelined WIDE exchange: the same pipeline for steps of 1..PIE_WIDE_MAX queries.  One wide union message per step
 * and shard (layout: pie_scan_wide_begin_union), written by the shard's own wide tail; entry points, counters, buffer sets and
 * u_pad of its own — a reservation here never moves the geometry of pie_comm_step_* and the reverse.  The rules stated above
 * for both kinds (geometry, a shard that cannot begin, bounded waits, failed steps, buffer lifetime) apply.  Order of calls as above:
 *     wide_step_reserve;  begin(0); begin(1); finish(0); begin(2); collect(0); finish(1); ...
 * The two kinds do not mix in flight: pie_comm_wide_step_begin returns PIE_E_STATE while ordinary steps are uncollected;
 * pie_comm_step_begin, pie_comm_scan_batch_gather and the queue calls return PIE_E_STATE while wide steps are uncollected.
 * Limits: steps begun and unfinished — what the shards' batch slots hold (pie_batch_room) and at most 6; steps uncollected —
 * the EIGHT rotating buffer sets.  Device memory per set and local rank:
 *     4 B x (u_pad + 2 + cap x (1 + 2 x words_max)) x (1 + world),   words_max = ceil(n_q_max / 64).
 * wide_step_reserve: n_q_max 1..PIE_WIDE_MAX fixes the message length; u_pad as in pie_comm_scan_batch_gather; union_cap =
 *               rows per message.  PIE_E_STATE if the geometry would change while wide steps are in flight.
 * wide_step_begin:  pie_scan_wide_begin_union on every local shard into the step's buffer set.
 * wide_step_finish: waits (bounded) for the oldest begun step's batches; m_out (may be NULL): local_ranks x n_q counts,
 *               PIE_E_CAPACITY with nothing consumed if m_cap is below that.  Queues the exchange on the side streams, which
 *               wait for a context's stream only where its shard said ready = 0.  Only the prefix the step uses is exchanged:
 *               u_pad + 2 + cap x (1 + 2 x ceil(n_q / 64)) words — every rank knows n_q.
 * wide_step_collect: waits (bounded by PIE_WAIT_DEADLINE_MS) for the oldest queued exchange; *step_out = its number.
 *               PIE_E_CAPACITY on every rank alike, from the gathered Mu words, when a union outgrew union_cap (reserve
 *               pie_comm_needed_cap() once nothing is in flight, repeat) or when some rank's Mu is -1.
 * wide_step_status: the gathered Mu word of every rank (mu_out: world values) of a collected step; -1: that rank kept no
 *               union.  This tells "re-reserve" from "rerun the batch": the first wide batch on a table normally overflows
 *               its 16 union slots per user and reruns on the general path while the slot capacity grows, so that step reports
 *               Mu = -1 — the caller REPEATS the step.  A caller whose queries really are dense (they keep falling back) uses
 *               pie_comm_scan_batch_gather in groups of at most PIE_BATCH_MAX.
 * The gathered messages of a collected step as rank at_rank holds them are valid until eight more steps have begun: message of
 * rank r at base + r * rank_stride_words, its masks as 2 x *words_out int32 per row behind rows[*cap_out];
 * wide_step_read_gathered copies one to the host (masks_out: [cap][words] uint64; PIE_E_CAPACITY if cap < min(Mu, union_cap));
 * wide_step_read_feed reads ONE user's feed of query qi straight from a gathered message (a few small copies and a filter on the
 * host, like pie_batch_read_user_feed); local_user and the rows are src_rank's local ids (pie_shard_maps).
 * Like the ordinary steps, this has run against a one-GPU stand-in for RCCL and a 1-rank RCCL communicator only. */
int pie_comm_wide_step_reserve(pie_comm *comm, int32_t n_q_max, int32_t u_pad, size_t union_cap);
int pie_comm_wide_step_begin(pie_comm *comm, const pie_query *queries, int32_t n_q);
int pie_comm_wide_step_finish(pie_comm *comm, size_t *m_out, size_t m_cap);
int pie_comm_wide_step_collect(pie_comm *comm, int64_t *step_out);
int pie_comm_wide_step_status(pie_comm *comm, int64_t step, int32_t *mu_out /* world */);
int pie_comm_wide_step_gathered_ptr(pie_comm *comm, int32_t at_rank, int64_t step, void **base_out, size_t *rank_stride_words,
                                    size_t *u_pad_out, size_t *cap_out, int *words_out);
int pie_comm_wide_step_read_gathered(pie_comm *comm, int32_t at_rank, int32_t src_rank, int64_t step, int32_t *uoff_out /* u_pad + 1 */,
                                     int32_t *rows_out, uint64_t *masks_out /* [cap][words] */, size_t cap, int *words_out, size_t *mu_out);
int pie_comm_wide_step_read_feed(pie_comm *comm, int32_t at_rank, int32_t src_rank, int64_t step, int32_t qi, int32_t local_user,
                                 int32_t *idx_out, size_t idx_cap, size_t *k_out);

/* ---- token lookups and the purge tick WHILE STEPS ARE IN FLIGHT: pie_shard_token_lookup_begin / _finish and
 * pie_shard_expired_queue_begin / _finish on every local shard.  A multi-GPU server answers getSession (server/index.js:84,
 * server/sessionStore.js:21-35) and computes its purge queue (server/sessionStore.js:66-73) without collecting the steps it keeps
 * in flight.  pie_comm_token_lookup and pie_comm_expired_queue keep their rule (PIE_E_STATE while steps are uncollected).
 * Both families:
 *   - allowed whenever every local shard has a table (lookups: and a token column), whatever is in flight: ordinary steps, wide
 *     steps, the synchronous gather's batches, or nothing;
 *   - no RCCL call; neither the exchange streams nor a step buffer set is touched; no context's stream or lane is synchronised:
 *     each shard's pass runs on its own side stream, and every host wait is bounded by PIE_WAIT_DEADLINE_MS (PIE_E_HIP past it);
 *   - in a process-per-GPU communicator a process reports what its own shards hold, as pie_comm_token_lookup and
 *     pie_comm_delete_users do;
 *   - begin asks every local shard before it begins on any.  If a shard still refuses after others began, what was begun is
 *     finished and discarded: every shard's room is what it was before the call;
 *   - the communicator counts what it has begun.  A shard whose own room does not match that count (pie_shard_* was used on a
 *     context from pie_comm_ctx directly): begin returns PIE_E_STATE and takes no slot anywhere;
 *   - pie_comm_destroy lands whatever was begun and not finished.
 * Token lookup: up to 4 begun and unfinished, finished in begin order; now[i] belongs to key i.  Per key the local shard with the
 * LARGEST global row answers, with its live / user / start / end in global ids; owner_rank_out[i] = the rank that answered, -1 if
 * none: pie_comm_token_lookup's merge, the unsharded table's answer, a key held by two shards included.  cap < k:
 * PIE_E_CAPACITY with *k_out set, the lookup stays finishable.  k = 0 takes and returns a slot.  Every output may be NULL.
 * pie_comm_token_lookup_room: the smallest room any local shard has left (4 less the lookups begun and unfinished).
 * Expired queue: one begun and unfinished.  Result: the ascending global rows with prev_now < end <= now that the local shards
 * hold — what pie_comm_expired_queue returns on the same table in a single-process communicator; owner_rank_out[i] = the rank
 * that holds row i (pie_shard_of of its user).  Every shard's pass is begun with cap_rows; finish waits (bounded) for each and
 * merges the shards' ascending lists ON THE DEVICE of the first local rank, on that shard's pass stream: one element per lane,
 * placed by co-rank (its index plus a lower bound in every other list), read from the shards' own queue buffers; lists held on
 * other devices are first copied over device to device, asynchronously, behind their pass.  *q_out (may be NULL) is always the
 * true total.  cap_rows = 0 counts only.  A total above cap_rows: the first cap_rows merged rows — a true ascending prefix,
 * since they only ever come from the first cap_rows rows of each list — are returned with PIE_E_CAPACITY; the queue is consumed.
 * rows_out or owner_rank_out != NULL with cap below the begin's cap_rows: PIE_E_INVAL, nothing consumed.
 * The merged list stays with the communicator until the next begin: pie_comm_inflight_queue_device_ptrs hands out the device
 * arrays on the first local rank's device (*n_out rows held = min(total, cap_rows); *q_out the total; PIE_E_STATE before a finish).
 * PIE_E_STATE: a shard without a table / a token column / whose row map does not cover its rows; a fifth lookup, a second queue;
 * finish with none begun.  PIE_E_INVAL: NULL communicator; NULL tok or now with k > 0; k or cap_rows >= 2^31.
 * Like the steps, this has run against a one-GPU stand-in for RCCL only, never across GPUs. */
int pie_comm_token_lookup_begin(pie_comm *comm, const uint64_t *tok /* [k][2] */, const int64_t *now /* [k] */, size_t k);
int pie_comm_token_lookup_finish(pie_comm *comm, int32_t *row_out, uint8_t *live_out, int32_t *user_out, int64_t *start_out,
                                 int64_t *end_out, int32_t *owner_rank_out, size_t cap, size_t *k_out);
int pie_comm_token_lookup_room(pie_comm *comm);
int pie_comm_expired_queue_begin(pie_comm *comm, int64_t prev_now, int64_t now, size_t cap_rows);
int pie_comm_expired_queue_finish(pie_comm *comm, int32_t *rows_out, int32_t *owner_rank_out, size_t cap, size_t *q_out);
int pie_comm_expired_queue_room(pie_comm *comm);
int pie_comm_inflight_queue_device_ptrs(pie_comm *comm, void **rows_dev, void **owner_rank_dev, size_t *n_out, size_t *q_out);

#ifdef __cplusplus
}
#endif
#endif /* PIE_SCAN_H */
