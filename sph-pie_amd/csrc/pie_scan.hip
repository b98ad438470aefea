// pie_scan.hip — C ABI (include/pie_scan.h) over the HIP kernels of pie_kernels.h.  gfx950 only.
// There is no CPU path in this library: every entry point either runs on the GPU or returns an error.
//
// One stream, two slots.  A scan is one bandwidth-bound kernel (K1, the table pass) followed by short latency-bound
// work (K2: offsets + the order of every small bucket; K3 scatter / K4 order only for buckets that outgrew their 16
// direct slots), all on ONE stream: co-running the tail with the next table pass on other streams was measured and
// rejected (its dependent loads crawl under a saturated HBM and every cross-queue dependency costs ~15 us:
// profiles/r01_d_two_stream_timeline.txt).
// The big per-scan buffers exist twice (two SLOTS) and the small histogram "spans" three times, rotating: K2 of
// every scan zeroes the span the scan AFTER THE NEXT will use (its last user is two launches old), so no memset and no
// event sits between kernels — a marker packet between two kernels costs ~6 us here, a plain kernel boundary ~0.
// pie_scan_begin enqueues K1+K2 and returns; pie_scan_finish spins on the summary that K2's last block writes to
// mapped host memory, then enqueues K3/K4 sized from it if any bucket needs them.  With begin(i+1) called before
// finish(i) the stream always holds the next table pass, so the host's round trip is off the critical path:
//   stream:  K1(i) | K1(i+1)+K2(i) in one launch | [K3(i) K4(i)] consumers(i) | K1(i+2)+K2(i+1) | ...
// (K2 of a scan rides in the first blocks of the next scan's table-pass launch; a scan nobody follows gets its K2 from
// pie_scan_finish).
// The table carries three derived columns (2-byte and 1-byte liveness keys, 16-byte payload records; pie_kernels.h)
// that every writer of `end` keeps in step; the scan form is chosen per scan from what the previous scan observed
// (live fraction, ambiguous keys, hot buckets) — see scan_begin.
#include "../../include/pie_scan.h"
#include "pie_kernels.h"
#include "pie_ordered.h"
#include "pie_token.h"
#include "pie_turn_plan.h"
#include "pie_expq.h"
#include "pie_wait.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <rocprim/device/device_radix_sort.hpp> // the archive chain's two sorts and its scan (pie_archive_queue)
#include <rocprim/device/device_scan.hpp>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace pie;

namespace {

thread_local char g_create_error[256] = "";

struct ScanEvents {
    hipEvent_t e0, e1, e2; // before K1, after K1, after the last kernel of the tail
};

constexpr int kEventRing = 2048;
constexpr size_t kDirectMaxBytes = (size_t)2 << 30; // direct bucket slots (256 B per user) are carried up to 8 M users

// everything one scan owns
struct Slot {
    int* counts = nullptr;         // the span this scan uses: histogram (transposed user order, see hist_index) | tile_pub[] | ScanCtl | Summary
    int* counts_ord = nullptr;     // per-user counts in user order, written by K2: what every consumer after K2 reads
    unsigned long long* tile_pub = nullptr;
    ScanCtl* ctl = nullptr;
    Summary* sum = nullptr;
    HostSummary* h_sum = nullptr;     // mapped pinned memory: written by K2's last block
    HostSummary* h_sum_dev = nullptr; // the same memory as the device sees it
    unsigned long long seq = 0;       // value h_sum->seq takes when this slot's scan has its summary
    long long* offsets = nullptr;
    SelRec* sel = nullptr;
    int* sel_rank = nullptr;
    int* blk_count = nullptr;
    BktRec* bkt = nullptr;
    BktRec* direct = nullptr;      // kTinyMax direct bucket slots per user (nullptr: user table too large, staged route only)
    int* blk_hot_base = nullptr;   // per (K1 block, hot user): the base its block-level histogram atomic returned
    int* hot_list = nullptr;       // K2's output: users whose bucket exceeded the hot threshold (<= kHotMax kept)
    int* over_list = nullptr;      // K2's output: buckets with staged records (user id, or -1 when nothing sits in its direct slots)
    HotSet hot{};                  // hot users of THIS scan (K1 and K3 must agree)
    bool k2_pending = false;       // K1 is queued, K2 is not yet: it rides in the next scan's launch or is launched by finish
    int4* zero_span = nullptr;     // the histogram span this scan's K2 zeroes (the one the scan after the next will use)
    int* msg = nullptr;            // this scan's result message (caller-owned device memory), or nullptr
    int msg_u_pad = 0;
    long long msg_cap = 0;
    int* msg_counts = nullptr;     // optional second destination: the per-user counts (pie_scan_begin_packed2)
    bool msg_by_k2 = false;        // K2 wrote the message (fused route)
    int* out_idx = nullptr;
    Segment* seg_list = nullptr;
    Segment* small_list = nullptr;
    int* part_cursor = nullptr;   // in the span: cursors of the partitioned fast path
    SelRec* part_rec = nullptr;   // kPartMax x kPartCap records
    bool fast = false;            // this scan ran on the partitioned fast path
    bool ordered = false;         // this scan ran on the ordered run (pie_ordered.h): nothing left to launch at finish
    long long q_now = 0, q_cutoff = 0; // the query, kept for a rerun on the general path
    int* big_list = nullptr;
    // per-scan host state
    bool in_flight = false;
    bool have_result = false;
    Summary last{};
    int k1_blocks = 0;
    long long rows_per_block = 0;
    int variant = 0;
    int dshift = 0;    // log2 of the direct-slot capacity this scan ran with (0: no direct slots), for pie_stats
    int ev_index = -1; // index into the event ring, -1 = not profiled
};

// Batches in flight: three.  With two, begin(i + 2) has to wait for finish(i), whose summary arrives half-way through launch i + 1
// (the tail of batch i rides there): the host then has the second half of ONE launch to prepare and queue the next, and every
// microsecond it is late the GPU idles (8 - 12 us per 54 us launch at 64 queries per batch, rocprofv3 timeline).  With three
// the next launch is always queued before the host waits.
constexpr int kBatchSlots = 3;
constexpr int kLaneMax = 4;     // batch lanes of a context (pie_set_batch_lanes): independent streams, kBatchSlots batches in flight on each
constexpr long long kHotDeltaMin = 1 << 16; // delta entries of the hot index at least (an eighth of its entries where that is more)

// what a batch slot needs for a WIDE batch (pie_kernels.h "wide batches"), allocated the first time the slot runs one
struct WideSlot {
    int dshift = -1;                        // the bucket capacity the arrays below were sized for
    unsigned long long* dmask = nullptr;    // bucket-slot masks: kWideWords words per slot
    unsigned long long* umask = nullptr;    // union masks: `words` words per union row, for up to (cap_users << dshift) rows
    int umask_words = 0;                    // mask words per row umask was sized for
    size_t umask_rows = 0;                  // ... and union rows
    char* d_sum = nullptr;                  // a wide batch on the run: its summary + kWideMax per-query totals (k_ord_wide_publish), copied to h_sum
    WideQuery* d_wq = nullptr;              // the batch's queries as the lanes hold them
    WideQuery* h_wq = nullptr;              // pinned staging of d_wq
    Summary* h_sum = nullptr;               // pinned: the pass's summary, then kWideMax per-query totals
    hipEvent_t done = nullptr;              // the summary has landed
    int words = 0;
    std::vector<pie_query> q;
    std::vector<unsigned char> fallback;
    std::vector<unsigned long long> m;      // selected rows per query
    // per-query lists: the fallback queries' (built at finish) and the ones somebody asked for (not every query of the batch)
    struct List { int* counts = nullptr; long long* offsets = nullptr; int* idx = nullptr; long long idx_cap = 0; bool ok = false; };
    std::vector<List> lists;
};

// everything one batch of queries owns (see pie_kernels.h "batched scan").  The primary result of a batch on the general pass
// is the UNION (uoff / urows / umlo / umhi); per-query lists are materialised from it on request, or produced directly by the
// paths that work per query (fallback scans on the general path, a batch on the ordered run).
struct BatchSlot {
    int n_q = 0;
    bool in_flight = false, k2_pending = false, have_result = false;
    int dshift = 4;                    // union bucket capacity (log2) the batch ran with
    bool ordered = false;              // this batch ran on the ordered run (pie_ordered.h "batched form"): no tail, nothing rides
    bool unsupported = false;          // this table cannot run the batched pass (no key columns / no direct slots): every query falls back
    bool fine_key = false;
    bool hot = false;                  // the pass read the hot index (pie_ctx::HotIndex) instead of the 1-byte key column
    unsigned long long seq = 0;
    char* span = nullptr;              // this batch's span (histogram | tile granules | ctl | summary + row statistics | mq slots)
    char* zero_span = nullptr;         // the span its tail zeroes
    BktRec* direct = nullptr;          // union bucket slots: [cap_users << bdshift]; BktRec::pad = the row's mask code (mask_code)
    unsigned long long* mtab = nullptr; // [kMaskTabWords] the tables that expand the codes: written by this batch's pass, read by its tail
    long long* uoff = nullptr;         // the union result: [cap_users + 1]
    int* urows = nullptr;              // [cap_users << bdshift]
    unsigned* umlo = nullptr;
    unsigned* umhi = nullptr;
    bool union_ok = false;             // the union arrays hold every query of the finished batch
    bool union_part = false;           // ... the queries that did not fall back
    unsigned long long mu = 0;         // union rows
    BatchHost* bh = nullptr;           // mapped pinned: the tail's summary + per-query totals
    BatchHost* bh_dev = nullptr;
    int lists_q = 0;                   // queries the per-query list storage below holds (0: not allocated)
    int* counts_ord = nullptr;         // [lists_q][users_stride]
    long long* offsets = nullptr;      // [lists_q][users_stride]
    int* out_idx = nullptr;            // [lists_q][out_stride]
    bool list_ok[kBatchMax];           // query q's counts / offsets / row list are in the list storage
    pie_query q[kBatchMax];
    bool fallback[kBatchMax];          // rerun on the general path (dense query, outgrown bucket, bad rows)
    Summary last[kBatchMax];
    int* over_idx[kBatchMax] = {};     // row list of a query that outgrew out_stride
    long long over_cap[kBatchMax] = {};
    int* idx_of[kBatchMax] = {};       // where query q's row list lives (valid with list_ok[q])
    int msg_kind = 0;                  // 0: none; 1: one message per query (lists); 2: ONE union message
    int* msg = nullptr;                // caller-owned device-visible memory
    long long msg_stride = 0, msg_cap = 0;
    int msg_u_pad = 0;
    int* msg_counts = nullptr;
    long long msg_counts_stride = 0;
    int k1_blocks = 0;
    int ev_index = -1;
    int lane = 0;                      // the lane (stream) the batch ran on
    hipStream_t stream = nullptr;
    bool main_ordered = true;          // the context's main stream is ordered behind the batch's kernels (see order_after_batch)
    bool wide = false;                 // a wide batch (pie_scan_wide_begin): its queries and results live in *w, not above
    WideSlot* w = nullptr;
};

// the ordered run of the resident table (pie_ordered.h)
constexpr int kOrdAppendMax = 4096; // rows of one append the run takes in place (a larger append drops the run)
// the run's own staging block for the rows of a turn: [start | end | user | disc] of up to kOrdAppendMax rows, and the 64 ints
// k_ord_append's long-chain path may read past the user column
constexpr size_t kOrdTurnStageBytes = (size_t)kOrdAppendMax * 24 + 64 * 4 + 64;

struct OrderedRun {
    int grid_mult = 12;      // PIE_ORD_GRID: blocks per CU of the key-stream kernels on the 1-byte key
    int mode = 1;            // PIE_ORDERED: 0 = never, 1 = when the general path is weak (dense / skewed queries), 2 = always
    bool valid = false;
    long long n = 0;         // positions (= rows the all-selecting scan returned)
    long long rows = 0;      // table rows the run covers (built from, plus the appends it took)
    long long held = 0;      // rows it holds (the selectable ones of those)
    long long cap = 0;       // positions the arrays hold
    int cap_users = 0;
    OrdRec* pay = nullptr;
    long long* end = nullptr;
    lkey_t* key = nullptr;
    fkey_t* fkey = nullptr;
    int* pos = nullptr;
    long long* uoff = nullptr;               // [users + 1] first position of every user's segment (rows, then spare slots)
    int* ufill = nullptr;                    // [users] rows in the segment
    int* pend = nullptr;                     // [users] rows of an append that found their segment full (re-spread)
    int* bhead = nullptr;                    // [users] head of the user's chain of rows in the append in progress (-1 between appends)
    int* bnext = nullptr;                    // [kOrdAppendMax] the chains: the row of the same user that came before this one, or -1
    int* placed = nullptr;                   // [2][4096] outcome per row of the append in progress (+ the copy pass 2 reads)
    char* tstage = nullptr;                  // the rows a turn created, gathered from the table for k_ord_append (k_ord_stage_rows)
    OrdRec* alt_pay = nullptr;               // the arrays a re-spread moves the run into (allocated at the first one), then swapped
    long long* alt_end = nullptr;
    lkey_t* alt_key = nullptr;
    fkey_t* alt_fkey = nullptr;
    long long* alt_uoff = nullptr;
    unsigned long long respreads = 0;
    // batched form: per query unit counts / prefixes / group sums, one summary set per batch slot
    int* bq_local = nullptr;
    long long* bq_gsum = nullptr;
    long long* bq_gbase = nullptr;
    OrdCtl* bq_ctl = nullptr;
    char* bq_sum[2] = {nullptr, nullptr};
    // wide batches on the run (pie_ordered.h OrdWidePool): scratch between the pass and its emit, one set (chains run one after the other)
    int* wp_rows = nullptr;
    unsigned long long* wp_mask = nullptr;
    size_t wp_cap = 0;
    int wp_words = 0;
    int users = 0;                           // users that have a segment (>= n_users: room for users yet to come)
    long long pos_cap = 0;                   // positions the arrays hold
    int* unit_count[2] = {nullptr, nullptr}; // alternate: the finish kernel of one ordered scan zeroes the other buffer
    int uc_next = 0;
    long long units_cap = 0;
    int* unit_local = nullptr;               // exclusive prefix of the unit counts inside their group of 1024
    long long* group_sum = nullptr;
    long long* group_base = nullptr;
    unsigned long long* tile_ballot = nullptr;
    unsigned int* tile_prefix = nullptr;
    unsigned int* h_stale = nullptr;         // mapped pinned: rows outside the run that a writer of `end` brought back to life
    unsigned int* stale = nullptr;           // ... as the device sees it
    bool no_room = false;                    // the arrays did not fit: not tried again for this table
    char* sum[2] = {nullptr, nullptr};       // per scan slot: Summary + row-statistics slots + OrdCtl
    unsigned wanted = 0;     // consecutive scans that wanted the run while it was not there
    unsigned need = 2;       // ... and how many of them it takes to build it: 2, more after a run that did not live long
    unsigned long long built_at = 0; // scans_begun when it was last built
    unsigned long long builds = 0;
    double build_ms = 0;
};

// A side pass runs beside scans and batches on a stream of its own: the token lookups and the expired queue in flight (side_open
// ... side_release below).  It is fenced against the context's stream both ways, once per begin (SideFence); a block it outgrew is
// only set aside, because hipFree and hipHostFree wait for the whole device, the lanes' kernels included.
struct SidePass {
    hipStream_t stream = nullptr; // non-blocking, created at the first begin
    bool stale = false;           // a wait gave up or a begin failed half-way: the next begin drains the stream first
    std::vector<std::pair<void*, void*>> retired; // (pinned, device) blocks a begin outgrew, until side_release
};
struct SideFence {
    hipEvent_t order = nullptr; // recorded on the context's stream at begin: the pass runs behind the mutations queued so far
    hipEvent_t done = nullptr;  // recorded on the side stream behind the pass; the context's stream waits for it
};

} // namespace

struct pie_ctx {
    int device = -1;
    int n_cus = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr; // main stream (own_stream or the caller's)
    unsigned long long seq_counter = 0;
    char err[512] = "";

    // resident table
    long long n = 0;
    int n_users = 0;
    long long cap_rows = 0;
    long long sel_cap = 0;      // records the staging arrays (sel, sel_rank) of each slot hold: see ensure_sel
    int cap_users = 0;
    long long *d_start = nullptr, *d_end = nullptr;
    int *d_user = nullptr, *d_disc = nullptr;
    // derived liveness-key column (see pie_kernels.h): 2 B/row, kept in step with d_end by every writer
    lkey_t* d_key = nullptr;
    PayRec* d_pay = nullptr;    // derived payload column (start, user, disc) per row: immutable after a row is written
    fkey_t* d_fkey = nullptr;   // 7-bit key of the top of the `end` range (1 B/row), see pie_kernels.h
    long long fkey_base = 0;
    int fkey_shift = 0;
    bool fkey_poor = false;     // a fine-keyed scan found too many ambiguous rows: use the 15-bit key
    unsigned int* d_hist = nullptr;
    std::vector<unsigned int> key_hist;  // host copy of the key histogram of the last full key build (8 keys per bin)
    std::vector<unsigned long long> key_hist_above; // key_hist_above[b] = rows in bins b .. end (what every begin asks for, per query)
    long long key_hist_rows = 0;         // rows it covers
    long long key_base = 0;
    int key_shift = 0;
    bool key_ok = false;        // d_key covers rows [0, n) under (key_base, key_shift)
    bool key_dirty = false;     // rows were appended / re-ended since the column was built: a rebuild may fit better
    bool key_poor = false;      // a keyed scan found too many ambiguous rows and a rebuild would not help: use the `end` column
    bool key_rebuild = false;   // ... and a rebuild may help: done at the next pie_scan_begin with nothing in flight
    bool keyed_enabled = true;  // PIE_K1_KEYED=0 turns the keyed form off
    int order_block = 512;       // threads (= users) per block of the fused K2 + order kernel (PIE_ORDER_BLOCK: 256 / 512 / 1024)
    bool no_ride = false;        // PIE_K2_RIDE=0: K2 never rides in the next scan's launch (A/B runs)
    bool no_fused_order = false; // PIE_FUSED_ORDER=0: K2 and the tiny-bucket order as two kernels (A/B runs)
    int k1_keyed = 0xC85;       // keyed liveness-first form (bit 0x400; 0x800: the 1-byte fine key where the query allows), unroll 8
    long long* d_range = nullptr;
    char* h_stage = nullptr;       // pinned host + device staging of the small mutations (append, touch): grown, never per call
    char* d_stage = nullptr;
    size_t stage_bytes = 0;
    bool expired_copy_total = false; // PIE_EXPIRED_COPY_TOTAL=1: the queue's length by a copy behind the gather, as before round 3 (A/B runs)
    // Appends and touches that need nothing back from the device (no ordered run to keep in step: its spare-slot bookkeeping is
    // read by the host) do not wait for it: the rows are validated on the host, staged in one of two pinned areas and queued; the
    // next scan runs behind them in stream order.  A server's turn — logins, touches, one feed scan — is then ONE wait, not three.
    struct AsyncStage { char* h = nullptr; char* d = nullptr; size_t bytes = 0; hipEvent_t ev = nullptr; bool pending = false; } astage[2];
    int astage_next = 0;
    bool async_mutations = true;   // PIE_ASYNC_MUTATIONS=0: every append / touch waits for its kernel (A/B runs)
    std::vector<uint8_t> set_end_keep;   // pie_set_end: which elements of the call are the last on their row; sized by the call
    std::vector<size_t> set_end_slots;   // ... and the scratch that finds them (set_end_last_writers)
    int* d_shard_rows = nullptr;   // pie_shard_table: local row -> global row
    int* d_shard_users = nullptr;  // ... local user -> global user
    long long shard_rows_n = 0;
    int shard_users_n = 0;
    // What pie_shard_table knew, for the mutators that take global ids (pie_shard_append_rows ...): the shard's place, the size of
    // the WHOLE table (rows and users ever handed out: N_g, U_g), the room of the two device maps (entries; they grow with
    // cap_rows / cap_users) and a host copy of the user map (4 B per local user; the row map has none).  A new table forgets it.
    bool shard_on = false;
    int shard_rank = 0, shard_world = 1;
    long long shard_rows_global = 0;
    int shard_users_global = 0;
    long long shard_rows_cap = 0;
    int shard_users_cap = 0;
    std::vector<int32_t> shard_users_h;
    std::vector<uint8_t> shard_keep;     // pie_shard_append_rows: which rows of the call this shard keeps; sized by the call
    // pie_compact_rows: the maps of the last compaction (old row -> new row or -1, new row -> old row), until rows are renumbered again
    int* d_cmp_new_of_old = nullptr;
    int* d_cmp_old_of_new = nullptr;
    long long cmp_n_old = 0, cmp_n_kept = 0;
    bool cmp_valid = false;
    long long *adopt_start = nullptr, *adopt_end = nullptr; // set by pie_compact_rows around its ensure_capacity call only: columns the
    int *adopt_user = nullptr, *adopt_disc = nullptr;       // re-allocated table takes over instead of allocating its own
    unsigned long long compactions = 0;
    // The token column and its index (pie_token.h): absent (tok == nullptr) until pie_token_set; dropped by whatever renumbers or
    // replaces the table; pie_compact_rows carries it over (`hold` keeps it through that call's ensure_capacity).
    struct TokenIndex {
        TokKey* tok = nullptr;      // [cap] keys of the rows [0, covered)
        long long cap = 0, covered = 0;
        // A sharded context's column (pie_shard_token_*): keys were given for the GLOBAL rows [0, covered_g); the shard holds those of
        // its local rows below that, a prefix [0, covered_l) only the device's row map knows (shard_token_covered reads it back, in
        // calls that wait anyway).  `covered` stays 0 then.
        bool sharded = false;
        long long covered_g = 0;
        int* slot_row = nullptr;    // [1 << log2_slots]
        unsigned log2_slots = 0;
        unsigned int* status = nullptr; // [kTokStatusWords], device
        char* h_stage = nullptr;    // pinned host + device staging of a lookup: keys in, results and the status words out
        char* d_stage = nullptr;
        size_t stage_bytes = 0;
        hipEvent_t ev[2] = {};      // around the last rebuild (build_ms)
        hipEvent_t turn_done = nullptr;     // behind a turn's download (pie_token_turn): what its one wait polls
        std::vector<int32_t> turn_slots;    // scratch of the turn's plan (pie_turn_plan.h), kept between calls
        // a sharded turn that logs in (pie_shard_session_turn), from its queue phase to its wait: the creates and the new users
        // that shaped its staging block (turn_stage_of)
        size_t turn_creates = 0, turn_new_users = 0;
        // a turn whose created rows went into the ordered run (pie_set_turn_ordered), from its launch to its wait: how many rows,
        // the first of them, and the user count the insert ran with; 0 rows: the run was not kept, or the turn created nothing
        size_t turn_ord_k = 0;
        long long turn_ord_row0 = 0;
        int turn_ord_users = 0;
        int turn_late_rc = 0;               // ... and what failed behind its launch (the wait phase reports it)
        bool timed = false;
        bool hold = false;
        double build_ms = 0;
        unsigned long long builds = 0;
        // What a lookup or a turn begun beside scans and batches holds until its finish: its own pinned and device staging
        // (lookup_flight_stage_of / turn_flight_stage_of: inputs and ITS zeroed status words in, the status words and the
        // results out), which only ever grows (slot_stage_room).
        struct FlightSlot {
            char* h = nullptr;
            char* d = nullptr;
            size_t bytes = 0, k = 0;
            bool landed = false;    // its `done` event was waited for (flight_slot_landed): the results are in h
            bool global = false;    // begun by the shard form: rows and users are GLOBAL ids
        };
        // Lookups that run beside scans and batches (pie_token_lookup_begin / _finish): one side pass and kTokLookups slots
        // handed out and returned in order.  A slot owns its fence: `done` sits behind the results' copy.
        struct Lookup : FlightSlot {
            SideFence fence;
            hipEvent_t done_event() const { return fence.done; }
            static constexpr const char *noun = "lookup", *unit = "keys", *subject = "token lookup";
        } lk[kTokLookups];
        SidePass side;              // stale: a finish returned its slot without having seen `done`
        int lk_head = 0, lk_n = 0;  // the oldest unfinished lookup; how many are unfinished
        // Turns begun beside scans and batches (pie_token_turn_begin / _finish): kTokTurns slots handed out and returned in
        // order.  The turn runs on the CONTEXT's stream (it mutates: see turn_fence); a slot owns the event behind its
        // download, the one thing its finish waits for.  A block a slot outgrew goes to side.retired.
        struct Turn : FlightSlot {
            hipEvent_t done = nullptr;
            hipEvent_t done_event() const { return done; }
            static constexpr const char *noun = "turn", *unit = "ops", *subject = "the turn";
        } tn[kTokTurns];
        int tn_head = 0, tn_n = 0;  // the oldest unfinished turn; how many are unfinished
        bool tn_stale = false;      // a finish returned its slot without having seen `done`: the next begin drains the stream first
    } tokx;
    // The expired queue that runs beside scans and batches (pie_expired_queue_begin / _finish): a side pass with scratch (one
    // count and one offset per unit, pie_expq_plan.h), a queue buffer and a mapped summary of its own, all created at the first
    // begin.  `done` sits behind its last kernel, `t0` ahead of its first (the device time of the pass).  One pass may be begun
    // and not finished.
    struct ExpiredFlight {
        SidePass side;
        SideFence fence;             // `done` keeps its timing: t0 .. done is the pass
        hipEvent_t t0 = nullptr;
        char* d_scratch = nullptr;
        int* d_buf = nullptr;
        size_t buf_rows = 0;
        HostSummary* h_sum = nullptr;
        HostSummary* h_sum_dev = nullptr;
        unsigned long long seq = 0;  // of the pass begun last
        size_t cap_rows = 0;         // what its begin asked for
        bool begun = false;
        bool launched = false;       // it has kernels (not an empty table or an empty window)
        bool landed = false;         // its summary was seen (expq_land): nothing of it reads the table any more
        bool global = false;         // begun by the shard form: the buffer holds GLOBAL rows
        bool timed = false;          // t0 / done of a pass whose time has not been read yet
        double ms = 0;
        int blocks_per_cu = kExpqBlocksPerCu;
        int max_blocks = 0;          // PIE_EXPQ_MAX_BLOCKS: a cap on the grid (0: none)
    } expq;
    double cmp_count_ms = 0;       // ... of its count pass and prefix alone
    double cmp_write_ms = 0;       // ... of its write pass (HIP events)

    // predicate table
    unsigned long long disc_mask = ~0ull;
    int n_disc = 64;

    // scan plans: [0] streaming form, [1] liveness-first form, [2] keyed liveness-first form, [3] the same on the 1-byte key
    int plan_blocks[4] = {0, 0, 0, 0};
    long long plan_rows[4] = {0, 0, 0, 0};
    int n_tiles = 0;
    int k1_variant = 0x03;    // streaming form: nontemporal loads + late user materialisation
    int k1_live_first = 0x85; // liveness-first form (unroll 8, nontemporal), chosen when few rows are live
    bool k1_pinned = false;   // PIE_K1_VARIANT given: no adaptation
    double live_frac = -1;    // live fraction seen by the last finished scan of this table (-1: none yet)
    int dshift = 4;           // log2 of the direct-slot capacity per user (16 .. kSmallMax); grown when scans outgrow it
    int dshift_want = 4;      // capacity the last finished scan asked for (applied at the next pie_scan_begin with nothing in flight)
    bool hot_bucket = false;  // the last finished scan had one bucket with > 1/64 of the selected rows
    bool clustered = false;   // the last streaming scan found most selected rows next to a row of the same user
    HotSet hot{};             // users whose buckets were "big" in a recent scan: block-level histogram in the aggregated forms
    unsigned hot_seen = 0;    // size of the hot list the set was read from
    unsigned hot_age = 0;     // finished scans since the set was read
    long long last_m = -1;    // M of the last finished feed scan of this table (-1: none yet)
    int part_shift = -1;      // users per partition = 1 << part_shift (-1: too many users for the fast path)
    int n_parts = 0;
    bool fast_enabled = false; // the partitioned path is opt-in (PIE_FAST_PATH=1): measured at parity with the general
    bool fast_env = false;     // path (0.179 vs 0.177 ms/step), so the simpler path stays the default; an overflow turns it off for the table

    UnionRow* d_union = nullptr;   // pie_batch_pack_union_device: per user kUnionMax union rows
    int* d_union_cnt = nullptr;    // ... their counts, padded with zeros to whole groups of 1024 (the two-level prefix reads groups)
    int* d_union_local = nullptr;  // ... prefix inside the group
    long long* d_union_off = nullptr; // ... group sums | group bases | a Summary the prefix kernel writes M into | the overflow flag
    int union_users = 0;
    OrderedRun ord;
    bool ord_building = false;  // the scan being begun is the ordered run's build
    // The end-ordered hot index (pie_kernels.h HotRec): where the 1-byte batched pass would stream the key column, a batch reads
    // the index's suffix for its smallest key(now) and the delta instead.  Built at the first batch begin that can use it with
    // nothing in flight; dropped by every key build or refit (build_keys).  Writers keep it exact in place (hot_mirror_of) and
    // never wait for it: the delta's cursor lives on the device, and the host bounds it by the rows its writers could move there
    // (delta_bound: the k of every set_end / append since the build), dropping the index before that bound passes delta_cap.
    struct HotIndex {
        HotRec* rec = nullptr;    // [n_main) grouped by bin | [delta_cap) delta
        long long rec_cap = 0;
        int* pos = nullptr;       // [pos_cap] row -> entry (-1: not held)
        long long pos_cap = 0;
        unsigned* cnt = nullptr;  // build scratch: 128 x segments counts / offsets
        long long cnt_cap = 0;
        long long* d_off = nullptr; // [129] bin offsets, device
        unsigned* delta_n = nullptr;
        long long off[129] = {};  // host copy: off[k] = first entry of bin k, off[128] = n_main
        long long n_main = 0, delta_cap = 0, delta_bound = 0;
        bool valid = false;
        bool enabled = true;      // PIE_HOT_INDEX=0: never built (A/B runs)
        int order = 1;            // PIE_HOT_ORDER: records inside a bin by row (0) or by histogram slot (1, see k_hot_keys)
        int recs_per_thread = 2;  // records of the pass per thread of its launch (PIE_HOT_RECS=1|2|4, a measurement switch)
        int built_order = 0;      // what the last build produced: the slot build falls back to row order (hot_build)
        hipEvent_t ev[2] = {};    // around the last build's work on the stream (build_ms)
        bool timed = false;
        double build_ms = 0;
        unsigned long long builds = 0;
    } hix;
    Slot slot[2];
    // Batch lanes.  A batch over a SHARD-sized table (a tenth of cfg3) is one launch of ~20 us that fills a fraction of the chip:
    // its time is latency (key load -> candidate gather -> atomic -> store; then the tail's prefix chain), not bytes.  Lanes are
    // independent pipelines — own stream, own three slots, own spans — so batches of different lanes run SIDE BY SIDE on the chip;
    // begin deals batches to the lanes round robin, finish returns them in the order they were begun (profiles/r03_zg_lanes.txt:
    // 1.25 x 10^7 rows, 64 queries: 20.9 us per batch on one lane, 7.8 on four).  Lane 0 is the context's main stream.
    BatchSlot bslot[kLaneMax * kBatchSlots]; // lane l: slots [l * kBatchSlots, (l + 1) * kBatchSlots)
    char* bspan[kLaneMax * 3] = {};          // lane l: rotating batch spans [3 l, 3 l + 3) (batch_span_bytes each)
    hipStream_t lane_stream[kLaneMax] = {};  // [0] unused (= stream); the others are created with the lane
    hipEvent_t lane_event[kLaneMax][2] = {}; // per lane: [0] orders the lane behind the main stream (idle_epoch), [1] the main stream behind the lane (order_after_batch)
    int n_lanes = 1;                         // lanes begin deals to (pie_set_batch_lanes / PIE_BATCH_LANES; 0 there = by table size)
    int lanes_want = 0;                      // what the caller asked for (0: automatic)
    int lane_rr = 0;                         // lane the next begin tries first
    int lane_flight[kLaneMax] = {};          // batches in flight per lane
    int lane_next[kLaneMax] = {};            // slot (0..kBatchSlots) the lane's next begin uses
    int lane_span_next[kLaneMax] = {};
    bool lane_alloc[kLaneMax] = {};          // the lane's slot arrays and spans exist
    unsigned char fifo[kLaneMax * kBatchSlots] = {}; // lanes of the batches in flight, in the order they were begun
    int fifo_head = 0;
    // Table changes (loads, appends, touches, key builds) are queued on the MAIN stream and only happen while no batch is in
    // flight; some return with kernels still queued (the fine key of a load).  A lane's stream knows nothing of the main
    // stream, so the first batch a lane begins after the context was idle waits for what the main stream holds.
    unsigned long long idle_epoch = 1;                // bumped whenever the last batch in flight leaves
    unsigned long long lane_epoch[kLaneMax] = {};     // the idle epoch the lane's stream was last ordered behind the main stream in
    // A turn begun with batches in flight (pie_token_turn_begin) mutates on the main stream between two fences: the main stream
    // first waits for every lane that has a batch in flight, and `mut_event` is recorded behind the turn's kernel.  A lane's next
    // launch waits for that event once (lane_after_mutation): the mutation epoch of its last wait against the context's.
    hipEvent_t mut_event = nullptr;
    unsigned long long mut_epoch = 0;                 // bumped by every turn begun in flight
    unsigned long long lane_mut_epoch[kLaneMax] = {}; // the mutation epoch the lane's stream last waited for
    long long* d_mat_tile = nullptr;   // materialisation scratch: [kBatchMax][tiles + 1] tile sums / prefixes
    unsigned int* d_mat_qmax = nullptr; // ... [kBatchMax] largest per-user count
    int mat_tiles = 0;
    int b_flight = 0;           // batches begun and not finished, all lanes
    BatchSlot* bres = nullptr;  // last finished batch
    int bdshift = 4;            // log2 of the union bucket capacity of the batched pass (16 .. 64 slots per user)
    int bdshift_want = 4;       // capacity the last finished batch asked for (applied at the next begin with nothing in flight)
    int run_shift = 0;          // chunk interleave of the keyed / batched table pass: 0 = fully interleaved (dense stretches of
                                // live rows, the safe default), 3 = eight consecutive chunks per wave (live rows spread evenly: a few
                                // per cent faster); follows the densest-chunk statistic of the last pass, see choose_run_shift
    bool batch_poor = false;    // union buckets overflowed at their largest capacity (skewed users): batches run as single scans
    bool ord_lists_only = false; // a batch's union on the ordered run outgrew the result arrays: its batches take the per-query chain
    bool wide_ordered = false;   // pie_set_wide_ordered / PIE_WIDE_ORDERED: a wide batch on a table whose batches take the ordered run runs one pass there
    bool turn_ordered = false;   // pie_set_turn_ordered / PIE_TURN_ORDERED: a turn that logs in keeps a valid ordered run where an append would
    bool wide_ord_off = false;   // ... until the union of one outgrew the result arrays: later wide batches rerun their queries, as with the switch off
    bool run_shift_pinned = false; // PIE_RUN_SHIFT=0..3 pins it (A/B runs)
    bool last_was_batch = false; // pie_stats_get describes the last finished batch rather than the last single scan
    unsigned long long bseq_counter = 0;
    char* span[3] = {nullptr, nullptr, nullptr}; // rotating histogram spans (see counts_span)
    int span_next = 0;
    int profile_every = 1;   // with profiling on, every n-th scan carries timing events
    double index_build_ms = 0;         // pie_table_info: last full build of the derived columns
    double wait_deadline_ms = 20000.0; // bound of every wait on a scan summary (PIE_WAIT_DEADLINE_MS)
    unsigned long long scans_begun = 0;
    int next_slot = 0;   // slot the next pie_scan_begin uses
    int n_flight = 0;    // scans begun and not finished (0..2)
    Slot* res = nullptr; // last finished scan (results)
    const unsigned char* d_qual = nullptr; // group-qualified scan form (k_scan_compact<.., GQ>): per-user flag
    char* d_arch = nullptr;                // pie_archive_queue: per-group scratch
    size_t arch_bytes = 0;
    char* d_arch_tmp = nullptr;            // ... temporary storage of its sorts / scan
    size_t arch_tmp_bytes = 0;
    unsigned long long arch_alg_bytes = 0; // algorithmic bytes of the last archive queue (32 B/row + 4 B per queued row)
    double arch_ms_sum = 0;                // with profiling on: device time of the archive chains (first kernel -> last sort)
    unsigned arch_calls = 0;
    // the queue the last pie_expired_queue / pie_archive_queue left on the device (pie_queue_info, pie_queue_pack_device); any
    // call that reuses the slots' workspace or changes the table forgets it (queue_forget)
    int q_kind = 0;                        // 0: none, 1: expired, 2: archive
    long long q_rows = 0;                  // its length
    int q_groups = 0;                      // archive: qualifying groups
    const int* q_dev = nullptr;            // the queue (local rows)
    const unsigned int* q_goff = nullptr;  // archive: exclusive scan of the group sizes, in group order

    // shared scratch
    long long* d_blk_off = nullptr;
    Summary* d_summary = nullptr; // table-maintenance calls
    Summary* h_summary = nullptr; // pinned

    // profiling
    bool profiling = false;
    std::vector<ScanEvents> ring;
    int ring_used = 0;
    double k1_ms_sum = 0, scan_ms_sum = 0;
    unsigned n_profiled = 0;
};

namespace {

int fail(pie_ctx* c, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (c) vsnprintf(c->err, sizeof c->err, fmt, ap);
    else vsnprintf(g_create_error, sizeof g_create_error, fmt, ap);
    va_end(ap);
    return code;
}

// Host-time profile of the batched begin / finish (builds with -DPIE_HOST_PROF only: tools/host_prof.sh); totals go to stderr
// when a context is destroyed.
#ifdef PIE_HOST_PROF
struct HostProf {
    double acc[16] = {0};
    unsigned long long n[16] = {0};
    timespec last{};
    void start() { clock_gettime(CLOCK_MONOTONIC, &last); }
    void tick(int i)
    {
        timespec t{};
        clock_gettime(CLOCK_MONOTONIC, &t);
        acc[i] += (double)(t.tv_sec - last.tv_sec) * 1e6 + (double)(t.tv_nsec - last.tv_nsec) * 1e-3;
        n[i]++;
        last = t;
    }
    void report() const
    {
        static const char* names[16] = {"begin: checks + dense test", "begin: slot / span set-up", "begin: tables", "begin: launch", "begin: rest",
                                        "finish: k2 launch", "finish: wait", "finish: rest", "", "", "", "", "", "", "", ""};
        for (int i = 0; i < 8; ++i)
            if (n[i]) fprintf(stderr, "[pie host prof] %-28s %8.3f us x %llu\n", names[i], acc[i] / (double)n[i], n[i]);
    }
};
HostProf g_prof;
#define PIE_PROF_START() g_prof.start()
#define PIE_PROF_TICK(i) g_prof.tick(i)
#else
#define PIE_PROF_START() ((void)0)
#define PIE_PROF_TICK(i) ((void)0)
#endif

#define PIE_HIP(c, call)                                                                              \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail((c), e_ == hipErrorOutOfMemory ? PIE_E_NOMEM : PIE_E_HIP, "%s: %s (%s:%d)", #call, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

template <class T>
void dfree(T*& p)
{
    if (p) (void)hipFree(p);
    p = nullptr;
}

DirectSlots direct_of(const pie_ctx* c, const Slot& sl);

// scans in flight are the last n_flight slots handed out; this is the older one
Slot* oldest_in_flight(pie_ctx* c)
{
    if (c->n_flight == 0) return nullptr;
    return &c->slot[c->n_flight == 2 ? c->next_slot : (c->next_slot ^ 1)];
}

void queue_forget(pie_ctx* c)
{
    c->q_kind = 0;
    c->q_rows = 0;
    c->q_groups = 0;
    c->q_dev = nullptr;
    c->q_goff = nullptr;
}

void free_slots(pie_ctx* c)
{
    queue_forget(c);
    for (Slot& s : c->slot) {
        s.counts = nullptr; s.sum = nullptr;
        s.tile_pub = nullptr; s.ctl = nullptr;
        dfree(s.offsets); dfree(s.counts_ord); dfree(s.sel); dfree(s.sel_rank); dfree(s.blk_count);
        dfree(s.bkt); dfree(s.direct); dfree(s.blk_hot_base); dfree(s.hot_list); dfree(s.over_list); dfree(s.out_idx); dfree(s.seg_list); dfree(s.small_list); dfree(s.big_list); dfree(s.part_rec); s.part_cursor = nullptr;
        s.in_flight = s.have_result = false;
    }
    for (char*& sp : c->span) dfree(sp);
    c->span_next = 0;
    c->sel_cap = 0;
    c->res = nullptr;
    c->n_flight = 0;
    c->next_slot = 0;
}

void free_batch(pie_ctx* c)
{
    for (BatchSlot& b : c->bslot) {
        dfree(b.counts_ord); dfree(b.offsets); dfree(b.direct); dfree(b.out_idx);
        dfree(b.mtab); dfree(b.uoff); dfree(b.urows); dfree(b.umlo); dfree(b.umhi);
        b.lists_q = 0;
        for (int q = 0; q < kBatchMax; ++q) { dfree(b.over_idx[q]); b.over_cap[q] = 0; b.idx_of[q] = nullptr; b.list_ok[q] = false; }
        b.in_flight = b.k2_pending = b.have_result = b.union_ok = b.union_part = false;
        b.n_q = 0;
        b.wide = false;
        if (WideSlot* w = b.w) {
            dfree(w->dmask); dfree(w->umask); dfree(w->d_wq); dfree(w->d_sum);
            if (w->h_wq) (void)hipHostFree(w->h_wq);
            if (w->h_sum) (void)hipHostFree(w->h_sum);
            if (w->done) (void)hipEventDestroy(w->done);
            for (WideSlot::List& l : w->lists) { dfree(l.counts); dfree(l.offsets); dfree(l.idx); }
            delete w;
            b.w = nullptr;
        }
    }
    for (char*& sp : c->bspan) dfree(sp);
    dfree(c->d_mat_tile); dfree(c->d_mat_qmax);
    c->mat_tiles = 0;
    for (int l = 0; l < kLaneMax; ++l) {
        c->lane_flight[l] = c->lane_next[l] = c->lane_span_next[l] = 0;
        c->lane_alloc[l] = false;
    }
    c->fifo_head = 0;
    c->lane_rr = 0;
    c->b_flight = 0;
    c->bres = nullptr;
}

void ord_free(pie_ctx* c)
{
    OrderedRun& o = c->ord;
    dfree(o.pay); dfree(o.end); dfree(o.key); dfree(o.fkey); dfree(o.pos); dfree(o.uoff); dfree(o.ufill); dfree(o.pend); dfree(o.placed); dfree(o.bhead); dfree(o.bnext); dfree(o.tstage);
    dfree(o.alt_pay); dfree(o.alt_end); dfree(o.alt_key); dfree(o.alt_fkey); dfree(o.alt_uoff);
    dfree(o.bq_local); dfree(o.bq_gsum); dfree(o.bq_gbase); dfree(o.bq_ctl); dfree(o.bq_sum[0]); dfree(o.bq_sum[1]);
    dfree(o.wp_rows); dfree(o.wp_mask);
    o.wp_cap = 0; o.wp_words = 0;
    dfree(o.unit_count[0]); dfree(o.unit_count[1]); dfree(o.unit_local); dfree(o.group_sum); dfree(o.group_base); dfree(o.tile_ballot); dfree(o.tile_prefix);
    dfree(o.sum[0]); dfree(o.sum[1]);
    o.valid = false;
    o.no_room = false;
    o.cap = 0; o.cap_users = 0; o.units_cap = 0; o.n = 0; o.rows = 0; o.wanted = 0; o.need = 2;
}

// The run no longer describes the table.  new_table: a load / re-shard — nothing is known about what comes.  Otherwise a row
// arrived that the run could not take (out of time order, no room even after a re-spread) or one it does not hold came back
// to life: a run that lived for fewer than 64 scans was not worth its build, so the next one takes four times as many
// consecutive dense / skewed queries to come about (2, 8, 32, ... 4096); one that lived longer starts over at 2.
void ord_invalidate(pie_ctx* c, bool new_table = false, bool out_of_order = false)
{
    OrderedRun& o = c->ord;
    if (new_table) {
        o.need = 2;
        o.wanted = 0;
    } else if (o.valid) {
        // rows that arrive out of time order are how this table is fed: the run cannot live on it, one build was enough to learn that
        if (out_of_order && c->scans_begun - o.built_at < 64) o.need = 4096u;
        else o.need = c->scans_begun - o.built_at < 64 ? (o.need * 4 < 4096u ? o.need * 4 : 4096u) : 2u;
        o.wanted = 0;
    }
    o.valid = false;
}

// spare slots every segment gets on top of a sixteenth of its rows: 16 where that costs under a quarter of the rows
// (a user with a handful of rows then takes a few hundred appends' worth of new sessions before anything has to move), else 4
int ord_spare(const pie_ctx* c) { return (long long)16 * c->cap_users <= c->cap_rows / 4 ? 16 : 4; }

HotMirror hot_mirror_of(const pie_ctx* c)
{
    HotMirror m{};
    if (c->hix.valid) {
        m.pos = c->hix.pos;
        m.rec = c->hix.rec;
        m.delta_n = c->hix.delta_n;
        m.n_main = c->hix.n_main;
        m.delta_cap = (unsigned)c->hix.delta_cap;
        m.pay = c->d_pay;
    }
    return m;
}

// a writer about to move up to k rows into the delta: the index stays only while the host's bound says they fit
void hot_reserve(pie_ctx* c, long long k)
{
    if (!c->hix.valid) return;
    if (c->hix.delta_bound + k > c->hix.delta_cap) c->hix.valid = false;
    else c->hix.delta_bound += k;
}

void hot_free(pie_ctx* c)
{
    pie_ctx::HotIndex& h = c->hix;
    dfree(h.rec); dfree(h.pos); dfree(h.cnt); dfree(h.d_off); dfree(h.delta_n);
    h.rec_cap = h.pos_cap = h.cnt_cap = 0;
    h.valid = false;
    for (hipEvent_t& e : h.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    h.timed = false;
}

OrdMirror ord_mirror_of(const pie_ctx* c)
{
    OrdMirror m{};
    if (c->ord.valid) {
        m.pos = c->ord.pos;
        m.end = c->ord.end;
        m.key = c->ord.key;
        m.fkey = c->ord.fkey;
        m.stale = c->ord.stale;
    }
    return m;
}

// ---- the waits (pie_wait.h): nothing below polls a query or a mapped word itself.  hipSuccess is kProbeDone.
int probe_of(hipError_t e) { return e == hipErrorNotReady ? kProbeNotReady : (int)e; }
// for a summary word in mapped host memory to take the value `want`; `query` says how the stream or event behind it fares
template <class Query>
WaitResult word_wait(pie_ctx* c, const volatile unsigned long long* word, unsigned long long want, Query query, double drained_grace_ms, WaitPace pace)
{
    return bounded_wait([=] { return *word == want; }, [&] { return probe_of(query()); }, c->wait_deadline_ms, drained_grace_ms, pace);
}

// for an event: the one query per spin is both the thing waited for and the probe
WaitResult event_wait(pie_ctx* c, hipEvent_t ev)
{
    hipError_t e = hipSuccess;
    return bounded_wait([&] { return (e = hipEventQuery(ev)) == hipSuccess; }, [&] { return probe_of(e); }, c->wait_deadline_ms, kNoGraceLimit, kPaceEvent);
}

// ---- side passes (SidePass, SideFence).  The caller has set the device.
int side_open(pie_ctx* c, SidePass& sp)
{
    if (!sp.stream) PIE_HIP(c, hipStreamCreateWithFlags(&sp.stream, hipStreamNonBlocking));
    if (sp.stale) PIE_HIP(c, hipStreamSynchronize(sp.stream)); // what a given-up wait left there may still use what the next pass touches
    sp.stale = false;
    return PIE_OK;
}

// the pass runs behind the appends, touches and deletes queued on the context's stream so far, and behind nothing that comes later
int side_enter(pie_ctx* c, SidePass& sp, SideFence& f, unsigned done_flags)
{
    if (!f.order) PIE_HIP(c, hipEventCreateWithFlags(&f.order, hipEventDisableTiming));
    if (!f.done) PIE_HIP(c, hipEventCreateWithFlags(&f.done, done_flags));
    PIE_HIP(c, hipEventRecord(f.order, c->stream));
    PIE_HIP(c, hipStreamWaitEvent(sp.stream, f.order, 0));
    return PIE_OK;
}

// whatever is queued on the context's stream from here on (a touch, a delete, an append) runs behind the pass's reads
hipError_t side_leave(pie_ctx* c, SidePass& sp, SideFence& f)
{
    const hipError_t e = hipEventRecord(f.done, sp.stream);
    return e == hipSuccess ? hipStreamWaitEvent(c->stream, f.done, 0) : e;
}

// a block the pass outgrew, its replacement already allocated: set aside until side_release (false: out of host memory)
bool side_retire(SidePass& sp, void* host_ptr, void* dev_ptr) try {
    if (host_ptr || dev_ptr) sp.retired.push_back({host_ptr, dev_ptr});
    return true;
} catch (...) {
    return false;
}

// called where the context has been drained anyway (the frees wait for the device)
void side_release(SidePass& sp)
{
    for (auto& p : sp.retired) {
        if (p.first) (void)hipHostFree(p.first);
        if (p.second) (void)hipFree(p.second);
    }
    sp.retired.clear();
}

void side_close(SidePass& sp)
{
    if (sp.stream) (void)hipStreamSynchronize(sp.stream);
    side_release(sp);
    if (sp.stream) (void)hipStreamDestroy(sp.stream); // pie_ctx_destroy, ahead of freeing what the pass owns
}

// the one wait of a lookup or a turn begun beside scans and batches: on its own event, never on the context's stream or a lane's
template <class Slot>
int flight_slot_landed(pie_ctx* c, Slot& sl, const char* what)
{
    if (sl.landed) return PIE_OK;
    const WaitResult w = event_wait(c, sl.done_event());
    if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "%s: %s failed: %s", what, Slot::subject, hipGetErrorString((hipError_t)w.err));
    if (w.end != WaitEnd::Ready)
        return fail(c, PIE_E_HIP, "%s: %s not finished within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", what, Slot::subject, w.waited_ms);
    sl.landed = true;
    return PIE_OK;
}

// Every lookup begun and not finished has run: its results are in its slot's pinned staging, where its finish reads them, in the
// ids of the table it was begun on.  Whatever replaces or frees something such a lookup reads (the columns, the token column, the
// slots, a shard's maps) calls this first; with none begun it costs nothing.
// The turns begun beside scans and batches (pie_token_turn_begin) land with them: a turn reads and writes what a lookup reads;
// past this the table holds their writes.
int token_lookups_land(pie_ctx* c, const char* what)
{
    pie_ctx::TokenIndex& t = c->tokx;
    for (int i = 0; i < t.lk_n; ++i) {
        int rc = flight_slot_landed(c, t.lk[(t.lk_head + i) % kTokLookups], what);
        if (rc) return rc;
    }
    for (int i = 0; i < t.tn_n; ++i) {
        int rc = flight_slot_landed(c, t.tn[(t.tn_head + i) % kTokTurns], what);
        if (rc) return rc;
    }
    return PIE_OK;
}

// ---- the staging layouts of the token calls (pie_token_*, further down).  Every form brings its results back in one order, [end 8 k | start 8 k | row 4 k | user 4 k | live k]
// from some base; `row` holds the GLOBAL row wherever a shard form has only one row to give.
struct TokResults {
    size_t end, start, row, user, live, past; // past: the first byte behind `live`
    explicit TokResults(size_t base = 0, size_t k = 0)
        : end(base), start(base + k * 8), row(base + k * 16), user(base + k * 20), live(base + k * 24), past(base + k * 25) {}
};

// what the caller asked for, out of the pinned block h (any pointer may be NULL)
void token_results_out(const char* h, const TokResults& r, size_t k, int32_t* row_out, uint8_t* live_out, int32_t* user_out,
                              int64_t* start_out, int64_t* end_out)
{
    if (row_out) memcpy(row_out, h + r.row, k * 4);
    if (live_out) memcpy(live_out, h + r.live, k);
    if (user_out) memcpy(user_out, h + r.user, k * 4);
    if (start_out) memcpy(start_out, h + r.start, k * 8);
    if (end_out) memcpy(end_out, h + r.end, k * 8);
}

// A staging block: the keys (16 k) or the ops (40 k) at 0, the form's other inputs, the results, the status words; [0, up) goes
// up.  The synchronous forms (tokx.h_stage) keep the status words last and fill them from the context's (token_stage_download).
// The in-flight forms (a slot's block) send their own up, zeroed, and keep them right ahead of the results: one copy of
// [status, bytes) brings both back.
struct TokStage {
    size_t now = 0;                        // in-flight lookup: a clock per key
    size_t next = 0, cuser = 0, cdisc = 0; // turn: the chains; the users and disciplines of its creates
    size_t crow = 0, newu = 0;             // sharded turn that logs in: the LOCAL row of every create (-1: another shard's); the new users
    size_t grow = 0;                       // synchronous shard lookup: the GLOBAL rows, beside the local ones in res.row
    size_t up = 0;
    TokResults res;
    size_t status = 0, bytes = 0;
};
constexpr size_t kTokStatusBytes = kTokStatusWords * sizeof(unsigned int);
size_t pad16(size_t x) { return (x + 15) / 16 * 16; }

// a lookup: [keys 16 k | results | pad | status]; the sharded lookup adds the GLOBAL rows (4 k) between live and the status words
TokStage lookup_stage_of(size_t k, bool global = false)
{
    TokStage o;
    o.up = k * 16;
    o.res = TokResults(o.up, k);
    o.grow = (o.res.past + 3) / 4 * 4;
    o.status = pad16(global ? o.grow + k * 4 : o.res.past);
    o.bytes = o.status + kTokStatusBytes;
    return o;
}

// a turn: [ops 40 k | next 4 k | cuser 4 n_create | cdisc 4 n_create | crow 4 n_create | newu 4 n_new | pad | results | pad |
// status]; only a turn that logs in (pie_session_turn) has creates, and only its shard form (pie_shard_session_turn) has crow and
// the new users of its user map
TokStage turn_stage_of(size_t k, size_t n_create = 0, bool shard = false, size_t n_new = 0)
{
    TokStage o;
    o.next = k * 40;
    o.cuser = k * 44;
    o.cdisc = o.cuser + n_create * 4;
    o.crow = o.cdisc + n_create * 4;
    o.newu = o.crow + (shard ? n_create * 4 : 0);
    o.up = o.newu + (shard ? n_new * 4 : 0);
    o.res = TokResults(pad16(o.up), k);
    o.status = pad16(o.res.past);
    o.bytes = o.status + kTokStatusBytes;
    return o;
}

TokStage flight_stage_of(size_t status, size_t k)
{
    TokStage o;
    o.status = status;
    o.res = TokResults(status + kTokStatusBytes, k);
    o.up = o.res.end;
    o.bytes = pad16(o.res.past);
    return o;
}

// a lookup's slot: [keys 16 k | now 8 k | status | results]
TokStage lookup_flight_stage_of(size_t k)
{
    TokStage o = flight_stage_of(k * 24, k);
    o.now = k * 16;
    return o;
}

// a turn's slot: [ops 40 k | next 4 k | pad | status | results]
TokStage turn_flight_stage_of(size_t k)
{
    TokStage o = flight_stage_of(pad16(k * 44), k);
    o.next = k * 40;
    return o;
}

template <class T>
T* stage_at(char* block, size_t offset) { return reinterpret_cast<T*>(block + offset); }

// The finish of the oldest lookup or turn of a ring of slots: the form it was begun by, the caller's room, the one wait, then the
// slot's own status words and the results.  The slot is returned whatever the wait said; if it failed, the slot's download may
// still be pending, and `stale` makes the next begin drain the stream before it touches a slot.
template <class Slot, int N>
int flight_finish(pie_ctx* c, Slot (&ring)[N], int& head, int& n, bool& stale, TokStage (*stage_of)(size_t), int32_t* row_out,
                         uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out, size_t cap, size_t* k_out, bool global,
                         const char* what)
{
    if (n == 0) return fail(c, PIE_E_STATE, "%s: no %s was begun", what, Slot::noun);
    Slot& sl = ring[head];
    if (sl.global != global) return fail(c, PIE_E_STATE, "%s: the oldest %s was begun by the %s form", what, Slot::noun, sl.global ? "shard" : "plain");
    const size_t k = sl.k;
    if (k_out) *k_out = k;
    if (cap < k) return fail(c, PIE_E_CAPACITY, "%s: %zu %s, room for %zu", what, k, Slot::unit, cap);
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = flight_slot_landed(c, sl, what);
    head = (head + 1) % N;
    n--;
    if (rc) stale = true;
    if (rc || k == 0) return rc;
    const TokStage o = stage_of(k);
    const unsigned int* st = stage_at<const unsigned int>(sl.h, o.status);
    if (st[0] || st[1])
        return fail(c, PIE_E_HIP, "%s: probe bound exhausted (a lookup ran %llu steps without meeting an empty slot)", what, 1ull << c->tokx.log2_slots);
    token_results_out(sl.h, o.res, k, row_out, live_out, user_out, start_out, end_out);
    return PIE_OK;
}

// every synchronous mutator is refused while a turn is begun and not finished (the turn's results belong to its queue position)
bool turns_begun(const pie_ctx* c) { return c->tokx.tn_n > 0; }

// The one wait of the expired queue begun beside scans and batches: on ITS summary word (and its own event, for a failure), never
// on the context's stream or a lane's.  Past it nothing of the pass reads the table.
int expq_land(pie_ctx* c, const char* what)
{
    pie_ctx::ExpiredFlight& x = c->expq;
    if (!x.begun || x.landed) return PIE_OK;
    const WaitResult w = word_wait(c, &x.h_sum->seq, x.seq, [&] { return hipEventQuery(x.fence.done); }, 0.0, kPaceSideSummary);
    if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "%s: expired queue in flight failed: %s", what, hipGetErrorString((hipError_t)w.err));
    if (w.end == WaitEnd::Drained) return fail(c, PIE_E_HIP, "%s: expired queue in flight ended without its summary", what);
    if (w.end == WaitEnd::Deadline)
        return fail(c, PIE_E_HIP, "%s: expired queue in flight not finished within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", what, w.waited_ms);
    x.landed = true;
    return PIE_OK;
}

// both side passes have run: for whatever replaces something that both read (the columns, a shard's maps, the row numbering)
int side_passes_land(pie_ctx* c, const char* what)
{
    const int rc = token_lookups_land(c, what);
    return rc ? rc : expq_land(c, what);
}

// the token column and its index go (no-op when there is none); the status array, the staging and the counters stay
void token_drop(pie_ctx* c)
{
    pie_ctx::TokenIndex& t = c->tokx;
    t.hold = false;
    if (!t.tok && !t.slot_row) return;
    (void)token_lookups_land(c, "token column");
    (void)hipStreamSynchronize(c->stream);
    side_release(t.side);
    dfree(t.tok);
    dfree(t.slot_row);
    t.cap = t.covered = t.covered_g = 0;
    t.sharded = false;
    t.log2_slots = 0;
}

void cmp_forget(pie_ctx* c)
{
    dfree(c->d_cmp_new_of_old);
    dfree(c->d_cmp_old_of_new);
    c->cmp_n_old = c->cmp_n_kept = 0;
    c->cmp_valid = false;
}

void free_table(pie_ctx* c)
{
    for (int l = 1; l < kLaneMax; ++l) // nothing of a lane's may still be running when its arrays go
        if (c->lane_stream[l]) (void)hipStreamSynchronize(c->lane_stream[l]);
    side_release(c->expq.side);
    dfree(c->d_union); dfree(c->d_union_cnt); dfree(c->d_union_local); dfree(c->d_union_off);
    c->union_users = 0;
    ord_free(c);
    hot_free(c);
    free_batch(c);
    dfree(c->d_start); dfree(c->d_end); dfree(c->d_user); dfree(c->d_disc); dfree(c->d_key); dfree(c->d_pay); dfree(c->d_fkey);
    dfree(c->d_arch);
    c->arch_bytes = 0;
    dfree(c->d_arch_tmp);
    c->arch_tmp_bytes = 0;
    c->key_ok = false;
    dfree(c->d_blk_off);
    free_slots(c);
    c->cap_rows = 0; c->cap_users = 0; c->n = 0; c->n_users = 0;
}

DirectSlots direct_of(const pie_ctx* c, const Slot& sl)
{
    DirectSlots d;
    d.p = sl.direct;
    d.shift = c->dshift;
    return d;
}

int sync_all(pie_ctx* c)
{
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    for (int l = 1; l < kLaneMax; ++l)
        if (c->lane_stream[l]) PIE_HIP(c, hipStreamSynchronize(c->lane_stream[l]));
    return PIE_OK;
}

// Grid of the scan kernel: every block owns a contiguous, tile-aligned row range.  Two plans, measured on
// cfg3 (profiles/r01_c_*): the streaming form likes many short blocks (short tail), the liveness-first form likes
// fewer, longer blocks (each wave ends with one partial drain of its live-row ring, amortised over more rows).
// PIE_K1_BLOCKS / PIE_K1_BLOCKS_LIVE override for tuning.
void plan_one(pie_ctx* c, int which, long long want, const char* env)
{
    if (const char* e = getenv(env)) {
        long long v = atoll(e);
        if (v > 0) want = v;
    }
    // a whole number of wave-tiles for every unroll (the keyed form reads 512 rows per wave per load)
    const long long block_tile_rows = which == 3 ? (long long)kFineKeyRowsPerLoad * 8 * kK1Waves
                                     : which == 2 ? (long long)kKeyRowsPerLoad * 8 * kK1Waves : (long long)kUnitRows * 8 * kK1Waves;
    long long tiles = (c->n + block_tile_rows - 1) / block_tile_rows;
    if (tiles < 1) tiles = 1;
    if (want > tiles) want = tiles;
    if (want < 1) want = 1;
    const long long tiles_per_block = (tiles + want - 1) / want;
    c->plan_rows[which] = tiles_per_block * block_tile_rows;
    c->plan_blocks[which] = (int)((c->n + c->plan_rows[which] - 1) / c->plan_rows[which]);
    if (c->plan_blocks[which] < 1) c->plan_blocks[which] = 1;
}

// Lanes of the batched scan (see pie_ctx::bslot): as many as the caller pinned, else by the size of the table — a batch over a
// small table is latency, and several side by side fill the chip; over the whole of cfg3 one batch already does
// (profiles/r03_zg_lanes.txt).
void choose_lanes(pie_ctx* c)
{
    if (c->lanes_want > 0) c->n_lanes = c->lanes_want;
    else c->n_lanes = c->n <= (1LL << 25) ? 4 : 3; // (10^8 rows: 53 / 42.5 / 41.5 / 41.6 us per 64-query batch on 1 / 2 / 3 / 4 lanes)
}

void plan_k1(pie_ctx* c)
{
    choose_lanes(c);
    plan_one(c, 0, (long long)c->n_cus * 48, "PIE_K1_BLOCKS");
    plan_one(c, 1, (long long)c->n_cus * 16, "PIE_K1_BLOCKS_LIVE");
    plan_one(c, 2, (long long)c->n_cus * 32, "PIE_K1_BLOCKS_KEYED");
    plan_one(c, 3, (long long)c->n_cus * 16, "PIE_K1_BLOCKS_FINE");
}

// The staging arrays give block b of a table pass the private region [b * rows_per_block, (b + 1) * rows_per_block): a
// block never stages more records than it reads, and since the keyed pass deals rows in interleaved chunks EVERY block,
// the last one too, reads up to rows_per_block rows — so the arrays must hold blocks x rows_per_block records of the
// largest plan (up to one block's worth beyond n), not n.  (Found by the differential fuzz: a dense query on the keyed
// form overran the arrays by most of a block and trampled the neighbouring allocation.)
int ensure_sel(pie_ctx* c)
{
    long long need = c->cap_rows + 256;
    for (int k = 0; k < 4; ++k) {
        const long long span = (long long)c->plan_blocks[k] * c->plan_rows[k] + 256;
        if (span > need) need = span;
    }
    if (need <= c->sel_cap && c->slot[0].sel) return PIE_OK;
    queue_forget(c);
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    for (Slot& s : c->slot) {
        dfree(s.sel);
        dfree(s.sel_rank);
    }
    c->sel_cap = 0;
    need += need / 16 + 65536; // room for the plans of a table that grows inside its capacity
    for (Slot& s : c->slot) {
        PIE_HIP(c, hipMalloc(&s.sel, (size_t)need * sizeof(SelRec)));
        PIE_HIP(c, hipMalloc(&s.sel_rank, (size_t)need * 4));
    }
    c->sel_cap = need;
    return PIE_OK;
}

// layout of a slot's span (all parts 128-byte aligned, total a multiple of 16 bytes so K2 can zero it as int4)
size_t span_counts_bytes(const pie_ctx* c) { return ((((size_t)c->cap_users + 32) * 4 + 127) / 128) * 128; } // +32: the transposed histogram rounds U up to a multiple of 32
size_t span_tiles_bytes(const pie_ctx* c) { return ((((size_t)c->cap_users / 256 + 2) * 8 + 127) / 128) * 128; } // sized for the smallest tile shape
size_t span_parts_bytes() { return (size_t)kPartMax * 4; }
size_t span_stats_bytes() { return (size_t)kSummaryBytes + (size_t)kStatSlots * sizeof(StatSlot); } // Summary (padded) + the K1 row-statistics slots
size_t counts_span(const pie_ctx* c) { return span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes() + 128 + span_stats_bytes(); }

// everything that depends on the number of users of the resident table (within the allocated capacity)
void set_user_count(pie_ctx* c, int n_users)
{
    c->n_users = n_users;
    c->n_tiles = (n_users + kScanTile - 1) / kScanTile;
    c->part_shift = -1;
    for (int sh = 0; (1 << sh) <= kPartRange; ++sh) {
        if ((((long long)n_users - 1) >> sh) + 1 <= kPartMax) { c->part_shift = sh; break; }
    }
    c->n_parts = c->part_shift >= 0 ? (int)((((long long)n_users - 1) >> c->part_shift) + 1) : 0;
}

// Make room for n rows / n_users users.  keep_rows > 0: the first keep_rows rows of the resident columns survive
// a re-allocation (append path; capacity grows geometrically so appends are amortised O(1) per row).
int ensure_capacity(pie_ctx* c, long long n, int n_users, long long keep_rows = 0)
{
    if (n < 0 || n >= (1LL << 31) - 1) return fail(c, PIE_E_INVAL, "row count %lld outside [0, 2^31 - 1)", n);
    if (n_users < 1) return fail(c, PIE_E_INVAL, "n_users must be >= 1 (got %d)", n_users);
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "table change while a scan is in flight");
    int rc = PIE_OK;
    // a new table, or columns that are about to move: the token lookups and the expired queue begun on the old ones land first
    if (keep_rows == 0 || n > c->cap_rows || n_users > c->cap_users) rc = side_passes_land(c, "table change");
    if (rc) return rc;
    rc = sync_all(c);
    if (rc) return rc;
    queue_forget(c); // a new table, or rows about to be added: the held queue is of the table as it was
    ord_invalidate(c, keep_rows == 0);
    if (keep_rows == 0) cmp_forget(c); // a new table (load, gen, shard, compact) renumbers the rows: the last compaction's maps go
    if (keep_rows == 0 && !c->tokx.hold) token_drop(c); // ... the token keys name the old rows (pie_compact_rows carries them over itself)
    if (keep_rows == 0) c->shard_on = false; // ... and it is no shard of anything until pie_shard_table says so (pie_compact_rows restores it)
    long long rows = n > 0 ? n : 1;
    if (rows > c->cap_rows || n_users > c->cap_users) {
        int users = n_users;
        if (keep_rows > 0) { // geometric growth for the append path
            if (rows > c->cap_rows) rows = rows > 2 * c->cap_rows ? rows : 2 * c->cap_rows;
            else rows = c->cap_rows;
            if (n_users > c->cap_users) users = n_users > 2 * c->cap_users ? n_users : 2 * c->cap_users;
            else users = c->cap_users;
            if (rows >= (1LL << 31)) rows = (1LL << 31) - 1;
        }
        long long *old_s = c->d_start, *old_e = c->d_end;
        int *old_u = c->d_user, *old_d = c->d_disc;
        if (keep_rows > 0) { c->d_start = c->d_end = nullptr; c->d_user = c->d_disc = nullptr; }
        else old_s = old_e = nullptr, old_u = old_d = nullptr;
        free_table(c);
        if (c->adopt_start) { // pie_compact_rows hands over columns of exactly `rows` rows that already hold the table
            c->d_start = c->adopt_start; c->d_end = c->adopt_end; c->d_user = c->adopt_user; c->d_disc = c->adopt_disc;
            c->adopt_start = c->adopt_end = nullptr;
            c->adopt_user = c->adopt_disc = nullptr;
        } else {
            PIE_HIP(c, hipMalloc(&c->d_start, rows * 8));
            PIE_HIP(c, hipMalloc(&c->d_end, rows * 8));
            PIE_HIP(c, hipMalloc(&c->d_user, rows * 4));
            PIE_HIP(c, hipMalloc(&c->d_disc, rows * 4));
        }
        // derived columns, rebuilt by build_keys after every (re)allocation; a table too large to carry them (19 B/row)
        // simply runs without the keyed form
        if (hipMalloc(&c->d_key, rows * sizeof(lkey_t) + 64) != hipSuccess || hipMalloc(&c->d_pay, rows * sizeof(PayRec)) != hipSuccess ||
            hipMalloc(&c->d_fkey, rows * sizeof(fkey_t) + 64) != hipSuccess) {
            (void)hipGetLastError();
            dfree(c->d_key);
            dfree(c->d_pay);
            dfree(c->d_fkey);
        }
        if (keep_rows > 0 && old_s) {
            PIE_HIP(c, hipMemcpyAsync(c->d_start, old_s, keep_rows * 8, hipMemcpyDeviceToDevice, c->stream));
            PIE_HIP(c, hipMemcpyAsync(c->d_end, old_e, keep_rows * 8, hipMemcpyDeviceToDevice, c->stream));
            PIE_HIP(c, hipMemcpyAsync(c->d_user, old_u, keep_rows * 4, hipMemcpyDeviceToDevice, c->stream));
            PIE_HIP(c, hipMemcpyAsync(c->d_disc, old_d, keep_rows * 4, hipMemcpyDeviceToDevice, c->stream));
            PIE_HIP(c, hipStreamSynchronize(c->stream));
            (void)hipFree(old_s); (void)hipFree(old_e); (void)hipFree(old_u); (void)hipFree(old_d);
        }
        const long long max_blocks = rows / (kUnitRows * 8 * kK1Waves) + 2;
        PIE_HIP(c, hipMalloc(&c->d_blk_off, (max_blocks * kK1Waves + 8) * 8)); // per-wave prefix of the expired queue
        c->cap_users = users; // counts_span() below reads it
        for (Slot& s : c->slot) {
            PIE_HIP(c, hipMalloc(&s.offsets, ((size_t)users + 1) * 8));
            PIE_HIP(c, hipMalloc(&s.counts_ord, ((size_t)users + 1) * 4));
            // +256: K3 fetches a region's first 256 records before it knows the count
            PIE_HIP(c, hipMalloc(&s.blk_count, (max_blocks * kK1Waves + 8) * 4));
            PIE_HIP(c, hipMalloc(&s.blk_hot_base, (size_t)(max_blocks + 8) * kHotMax * 4));
            PIE_HIP(c, hipMalloc(&s.hot_list, (size_t)kHotMax * 4));
            PIE_HIP(c, hipMalloc(&s.over_list, ((size_t)users + 16) * 4));
            PIE_HIP(c, hipMalloc(&s.bkt, rows * sizeof(BktRec)));
            if ((size_t)users * kTinyMax * sizeof(BktRec) <= kDirectMaxBytes) PIE_HIP(c, hipMalloc(&s.direct, (size_t)users * kTinyMax * sizeof(BktRec)));
            c->dshift = c->dshift_want = 4;
            PIE_HIP(c, hipMalloc(&s.out_idx, rows * 4));
            PIE_HIP(c, hipMalloc(&s.seg_list, ((size_t)users + rows / kSegMax + 16) * sizeof(Segment)));
            PIE_HIP(c, hipMalloc(&s.small_list, ((size_t)users + 16) * sizeof(Segment)));
            PIE_HIP(c, hipMalloc(&s.big_list, ((size_t)users + 16) * 4));
            PIE_HIP(c, hipMalloc(&s.part_rec, (size_t)kPartMax * kPartCap * sizeof(SelRec)));
        }
        for (char*& sp : c->span) PIE_HIP(c, hipMalloc(&sp, counts_span(c)));
        c->cap_rows = rows;
    }
    c->n = n;
    c->n_users = n_users;
    c->n_tiles = (n_users + kScanTile - 1) / kScanTile;
    if (keep_rows == 0) {
        // a new table: nothing is known about it.  An append keeps what the last scans observed (live fraction, skew,
        // clustering): a few new rows do not change the picture, and one scan corrects it if they do
        c->live_frac = -1;
        c->batch_poor = false;
        c->ord_lists_only = false;
        c->wide_ord_off = false;
        if (!c->run_shift_pinned) c->run_shift = 0;
        c->hot_bucket = false;
        c->clustered = false;
        c->hot.n = 0;
        c->hot_seen = 0;
        c->hot_age = 0;
        c->last_m = -1;
    }
    c->fast_enabled = c->fast_env;
    set_user_count(c, n_users);
    c->res = nullptr;
    for (Slot& s : c->slot) s.have_result = false;
    // all three spans start clean; from here on every K2 zeroes the span of the scan after it
    for (char* sp : c->span) PIE_HIP(c, hipMemsetAsync(sp, 0, counts_span(c), c->stream));
    c->span_next = 0;
    plan_k1(c);
    return ensure_sel(c);
}

// pinned host + device staging blocks of at least `bytes` (one pair per context; the context is used by one thread)
int ensure_stage(pie_ctx* c, size_t bytes)
{
    if (bytes <= c->stage_bytes) return PIE_OK;
    size_t want = c->stage_bytes ? c->stage_bytes : (size_t)64 << 10;
    while (want < bytes) want *= 2;
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    dfree(c->d_stage);
    c->h_stage = nullptr;
    c->stage_bytes = 0;
    PIE_HIP(c, hipHostMalloc(&c->h_stage, want, hipHostMallocDefault));
    PIE_HIP(c, hipMalloc(&c->d_stage, want));
    c->stage_bytes = want;
    return PIE_OK;
}

// one of the two staging areas of the queued mutations, free to be written: *out
int async_stage(pie_ctx* c, size_t bytes, pie_ctx::AsyncStage** out)
{
    pie_ctx::AsyncStage& a = c->astage[c->astage_next];
    c->astage_next ^= 1;
    if (a.pending) { // the copy out of it was queued two mutations ago
        PIE_HIP(c, hipEventSynchronize(a.ev));
        a.pending = false;
    }
    if (!a.ev) PIE_HIP(c, hipEventCreateWithFlags(&a.ev, hipEventDisableTiming));
    if (bytes > a.bytes) {
        size_t want = a.bytes ? a.bytes : (size_t)64 << 10;
        while (want < bytes) want *= 2;
        if (a.h) (void)hipHostFree(a.h);
        if (a.d) { PIE_HIP(c, hipStreamSynchronize(c->stream)); (void)hipFree(a.d); } // a kernel queued earlier may still read it
        a.h = nullptr; a.d = nullptr; a.bytes = 0;
        PIE_HIP(c, hipHostMalloc(&a.h, want, hipHostMallocDefault));
        PIE_HIP(c, hipMalloc(&a.d, want));
        a.bytes = want;
    }
    *out = &a;
    return PIE_OK;
}

int validate_users(pie_ctx* c, long long row0 = 0)
{
    if (c->n - row0 <= 0) return PIE_OK;
    PIE_HIP(c, hipMemsetAsync(c->d_summary, 0, sizeof(Summary), c->stream));
    const int grid = c->n_cus * 8;
    hipLaunchKernelGGL(k_validate_users, dim3(grid), dim3(256), 0, c->stream, c->d_user + row0, c->n - row0, c->n_users,
                       &c->d_summary->bad_rows);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(Summary), hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    if (c->h_summary->bad_rows)
        return fail(c, PIE_E_INVAL, "%u rows carry a user id outside [0, %d)", c->h_summary->bad_rows, c->n_users);
    return PIE_OK;
}

// Liveness-key column for rows [row0, n).  row0 == 0, a re-allocated table, or `rebuild` re-derive (base, shift) from the
// range of the live `end` values and key every row; otherwise the appended rows are keyed under the current parameters
// (out-of-range values clamp; the column stays exact, only less selective).
int build_keys(pie_ctx* c, long long row0, bool rebuild = false)
{
    c->hix.valid = false; // its bins are the fine key's
    if (!c->d_key || !c->d_pay || !c->d_fkey) { c->key_ok = false; return PIE_OK; }
    const bool write_pay = !(rebuild && c->key_ok); // a refit of the key leaves the (immutable) payload alone
    if (c->n == 0) { c->key_ok = true; c->key_base = 0; c->key_shift = 0; c->key_dirty = false; return PIE_OK; }
    hipStream_t s = c->stream;
    const int grid = c->n_cus * 8;
    const bool full_build = row0 == 0 || !c->key_ok || rebuild;
    // the ordered run carries copies of both keys: a refit of the table's keys refits them from its copy of `end` (below);
    // a first build means a new table, whose run went with the old one
    if (full_build && !(rebuild && c->key_ok && c->ord.valid && c->ord.rows == c->n)) ord_invalidate(c);
    timespec tb0{};
    if (full_build) { // index_build_ms of pie_table_info: everything from here to the last key kernel's completion
        const int land_rc = expq_land(c, "key build"); // an expired queue in flight reads the keys under the old parameters
        if (land_rc) return land_rc;
        PIE_HIP(c, hipStreamSynchronize(s));
        clock_gettime(CLOCK_MONOTONIC, &tb0);
    }
    if (row0 == 0 || !c->key_ok || rebuild) {
        const long long init[2] = {INT64_MAX, INT64_MIN};
        long long got[2];
        PIE_HIP(c, hipMemcpyAsync(c->d_range, init, sizeof init, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_end_range, dim3(grid), dim3(256), 0, s, c->d_end, c->n, c->d_range);
        PIE_HIP(c, hipGetLastError());
        PIE_HIP(c, hipMemcpyAsync(got, c->d_range, sizeof got, hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipStreamSynchronize(s));
        c->key_base = 0;
        c->key_shift = 0;
        if (got[0] <= got[1]) {
            c->key_base = got[0];
            const unsigned long long span = (unsigned long long)got[1] - (unsigned long long)got[0];
            while (c->key_shift < 63 && (span >> c->key_shift) >= (unsigned long long)(kKeyMax - 1u)) c->key_shift++;
        }
        row0 = 0;
        c->key_dirty = false;
        c->key_poor = false;
        c->key_rebuild = false;
    } else {
        c->key_dirty = true;
    }
    hipLaunchKernelGGL(k_build_key, dim3(grid), dim3(256), 0, s, c->d_end, row0, c->n, c->key_base, c->key_shift, c->d_key,
                       c->d_start, c->d_user, c->d_disc, write_pay ? c->d_pay : (PayRec*)nullptr);
    PIE_HIP(c, hipGetLastError());
    if (row0 == 0) {
        // fine key: base = lower edge of the histogram bin that holds the 90th percentile of the 15-bit keys (tombstones
        // and rows below the base count as key 0), shift = smallest that keeps the largest `end` under the clamp
        std::vector<unsigned int> hist(kKeyHistBins);
        PIE_HIP(c, hipMemsetAsync(c->d_hist, 0, kKeyHistBins * sizeof(unsigned int), s));
        hipLaunchKernelGGL(k_key_hist, dim3(c->n_cus), dim3(1024), 0, s, c->d_key, c->n, c->d_hist);
        PIE_HIP(c, hipGetLastError());
        PIE_HIP(c, hipMemcpyAsync(hist.data(), c->d_hist, kKeyHistBins * sizeof(unsigned int), hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipStreamSynchronize(s));
        c->key_hist = hist;
        c->key_hist_rows = c->n;
        c->key_hist_above.assign((size_t)kKeyHistBins + 1, 0ull);
        for (int b = kKeyHistBins - 1; b >= 0; --b) c->key_hist_above[(size_t)b] = c->key_hist_above[(size_t)b + 1] + hist[(size_t)b];
        unsigned long long cum = 0;
        int bin = 0, top_bin = 0;
        for (int b = 0; b < kKeyHistBins; ++b)
            if (hist[b]) top_bin = b;
        const unsigned long long want = (unsigned long long)((double)c->n * 0.9);
        for (bin = 0; bin < kKeyHistBins - 1; ++bin) {
            if (cum + hist[bin] > want) break;
            cum += hist[bin];
        }
        if (bin > top_bin) bin = top_bin;
        // key k >= 1 covers [base + ((k-1) << shift), base + (k << shift)); bin b holds keys 8b .. 8b+7
        c->fkey_base = bin == 0 ? c->key_base : (long long)((unsigned long long)c->key_base + (((unsigned long long)bin * 8ull - 1ull) << c->key_shift));
        const unsigned long long top_edge = (unsigned long long)c->key_base + (((unsigned long long)top_bin * 8ull + 8ull) << c->key_shift);
        const unsigned long long fspan = top_edge - (unsigned long long)c->fkey_base;
        c->fkey_shift = 0;
        while (c->fkey_shift < 63 && (fspan >> c->fkey_shift) >= (unsigned long long)(kFineKeyMax - 1u)) c->fkey_shift++;
        c->fkey_poor = false;
    }
    hipLaunchKernelGGL(k_build_fine_key, dim3(grid), dim3(256), 0, s, c->d_end, row0, c->n, c->fkey_base, c->fkey_shift, c->d_fkey);
    PIE_HIP(c, hipGetLastError());
    if (rebuild && c->ord.valid) { // filler positions hold end = 0 (or below every base): key 0 under any parameters
        hipLaunchKernelGGL(k_build_key, dim3(grid), dim3(256), 0, s, c->ord.end, 0LL, c->ord.n, c->key_base, c->key_shift, c->ord.key,
                           (const long long*)nullptr, (const int*)nullptr, (const int*)nullptr, (PayRec*)nullptr);
        hipLaunchKernelGGL(k_build_fine_key, dim3(grid), dim3(256), 0, s, c->ord.end, 0LL, c->ord.n, c->fkey_base, c->fkey_shift, c->ord.fkey);
        PIE_HIP(c, hipGetLastError());
    }
    c->key_ok = true;
    if (full_build) {
        PIE_HIP(c, hipStreamSynchronize(s));
        timespec tb1{};
        clock_gettime(CLOCK_MONOTONIC, &tb1);
        c->index_build_ms = (double)(tb1.tv_sec - tb0.tv_sec) * 1e3 + (double)(tb1.tv_nsec - tb0.tv_nsec) * 1e-6;
    }
    return PIE_OK;
}

// Bits of a histogram slot: the padded histogram of hist_index has 32 * ceil(U / 32) counters.
int hot_slot_bits(unsigned long long n_users)
{
    const unsigned long long pad = ((n_users + 31) >> 5) * 32;
    int b = 0;
    while ((1ull << b) < pad) ++b;
    return b;
}

// The slot-ordered records of a build whose counts and offsets stand (h.cnt, h.n_main): keys, one stable radix sort over the
// bits in use, gather.  The scratch (two key and two row arrays and the sort's own) is transient: allocated here, freed before
// returning, never part of workspace_bytes.  -> false with nothing written: no scratch, or bin and slot do not fit 32 bits.
static bool hot_fill_by_slot(pie_ctx* c, long long blocks, long long seg_len)
{
    pie_ctx::HotIndex& h = c->hix;
    hipStream_t s = c->stream;
    const int slot_bits = hot_slot_bits((unsigned long long)c->n_users);
    if (slot_bits + 7 > 32 || h.n_main > 0x7FFFFFFFLL) return false;
    if (h.n_main == 0) return true;
    const size_t m = (size_t)h.n_main, arr = (m * 4 + 255) & ~(size_t)255;
    size_t need = 0;
    unsigned* kz = nullptr;
    int* vz = nullptr;
    if (rocprim::radix_sort_pairs(nullptr, need, kz, kz, vz, vz, m, 0u, (unsigned)(slot_bits + 7), s) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    char* scratch = nullptr;
    if (hipMalloc(&scratch, 4 * arr + need + 256) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    unsigned* k_in = reinterpret_cast<unsigned*>(scratch);
    unsigned* k_out = reinterpret_cast<unsigned*>(scratch + arr);
    int* v_in = reinterpret_cast<int*>(scratch + 2 * arr);
    int* v_out = reinterpret_cast<int*>(scratch + 3 * arr);
    void* tmp = scratch + 4 * arr;
    hipLaunchKernelGGL(k_hot_keys, dim3((unsigned)blocks), dim3(256), 0, s, c->d_fkey, c->d_pay, c->n, seg_len, h.cnt, c->n_users, slot_bits, k_in, v_in);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = rocprim::radix_sort_pairs(tmp, need, k_in, k_out, v_in, v_out, m, 0u, (unsigned)(slot_bits + 7), s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_hot_gather, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, k_out, v_out, h.n_main, slot_bits, c->d_end, c->d_pay, h.rec, h.pos);
        e = hipGetLastError();
    }
    const hipError_t e2 = hipStreamSynchronize(s); // the scratch goes only when nothing reads it any more
    (void)hipFree(scratch);
    if (e != hipSuccess || e2 != hipSuccess) { // pos[] may be half written: the caller's row-order scatter rewrites all of it
        (void)hipGetLastError();
        return false;
    }
    return true;
}

// k_hot_scan's work for the slot build: a device-wide exclusive scan of the (bin, segment) counts into transient scratch,
// off[] from it, the prefix copied back over the counts.  -> the scratch, to be freed once the stream has run; nullptr with
// nothing launched when it cannot be had (the caller runs k_hot_scan).
static void* hot_scan_wide(pie_ctx* c, long long S)
{
    pie_ctx::HotIndex& h = c->hix;
    hipStream_t s = c->stream;
    const size_t total = (size_t)(128 * S), arr = (total * 4 + 255) & ~(size_t)255;
    size_t need = 0;
    unsigned* z = nullptr;
    if (rocprim::exclusive_scan(nullptr, need, z, z, 0u, total, rocprim::plus<unsigned int>(), s) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    char* scratch = nullptr;
    if (hipMalloc(&scratch, arr + need + 256) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    unsigned* out = reinterpret_cast<unsigned*>(scratch);
    if (rocprim::exclusive_scan(scratch + arr, need, h.cnt, out, 0u, total, rocprim::plus<unsigned int>(), s) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(s);
        (void)hipFree(scratch);
        return nullptr;
    }
    hipLaunchKernelGGL(k_hot_offsets, dim3(1), dim3(192), 0, s, out, h.cnt, S, h.d_off);
    (void)hipMemcpyAsync(h.cnt, out, total * 4, hipMemcpyDeviceToDevice, s);
    return scratch;
}

// The hot index of the current fine key (see pie_ctx::HotIndex), on the main stream with nothing in flight; waits for the
// bin offsets.  Device memory it cannot get leaves the batches on the key stream.  Inside a bin the records stand in slot
// order (k_hot_keys) unless PIE_HOT_ORDER=row asks for row order, or the slot build cannot run: then in row order.
int hot_build(pie_ctx* c)
{
    pie_ctx::HotIndex& h = c->hix;
    hipStream_t s = c->stream;
    const long long blocks = (long long)c->n_cus * 16, S = blocks * 4; // one segment per wave
    const long long seg_len = ((c->n + S - 1) / S + kWave - 1) / kWave * kWave;
    auto grow = [&](auto*& p, long long& cap, long long want, size_t elem) {
        if (cap >= want) return true;
        dfree(p);
        cap = 0;
        if (hipMalloc(&p, (size_t)want * elem) != hipSuccess) { (void)hipGetLastError(); return false; }
        cap = want;
        return true;
    };
    long long one = 0;
    if (!h.d_off) grow(h.d_off, one, 129, sizeof(long long));
    one = 0;
    if (!h.delta_n) grow(h.delta_n, one, 1, sizeof(unsigned));
    if (!h.d_off || !h.delta_n || !grow(h.pos, h.pos_cap, c->cap_rows, sizeof(int)) || !grow(h.cnt, h.cnt_cap, 128 * S, sizeof(unsigned))) {
        h.enabled = false;
        return PIE_OK;
    }
    for (hipEvent_t& e : h.ev)
        if (!e) PIE_HIP(c, hipEventCreate(&e));
    h.timed = false;
    PIE_HIP(c, hipEventRecord(h.ev[0], s));
    PIE_HIP(c, hipMemsetAsync(h.pos, 0xFF, (size_t)c->cap_rows * sizeof(int), s));
    hipLaunchKernelGGL(k_hot_count, dim3((unsigned)blocks), dim3(256), 0, s, c->d_fkey, c->n, seg_len, h.cnt);
    void* scan_scratch = h.order == 1 ? hot_scan_wide(c, S) : nullptr;
    if (!scan_scratch) hipLaunchKernelGGL(k_hot_scan, dim3(1), dim3(1024), 0, s, h.cnt, S, h.d_off);
    hipError_t e_scan = hipGetLastError();
    if (e_scan == hipSuccess) e_scan = hipMemcpyAsync(h.off, h.d_off, sizeof h.off, hipMemcpyDeviceToHost, s);
    if (e_scan == hipSuccess) e_scan = hipStreamSynchronize(s);
    if (scan_scratch) (void)hipFree(scan_scratch);
    PIE_HIP(c, e_scan);
    h.n_main = h.off[128];
    h.delta_cap = h.n_main / 8 > kHotDeltaMin ? h.n_main / 8 : kHotDeltaMin;
    if (!grow(h.rec, h.rec_cap, h.n_main + h.delta_cap, sizeof(HotRec))) {
        h.enabled = false;
        return PIE_OK;
    }
    h.built_order = h.order == 1 && hot_fill_by_slot(c, blocks, seg_len) ? 1 : 0;
    if (h.built_order == 0) {
        hipLaunchKernelGGL(k_hot_scatter, dim3((unsigned)blocks), dim3(256), 0, s, c->d_fkey, c->d_end, c->d_pay, c->n, seg_len, h.cnt, h.rec, h.pos);
        PIE_HIP(c, hipGetLastError());
    }
    PIE_HIP(c, hipMemsetAsync(h.delta_n, 0, sizeof(unsigned), s));
    PIE_HIP(c, hipEventRecord(h.ev[1], s));
    h.timed = true;
    h.delta_bound = 0;
    h.valid = true;
    h.builds++;
    return PIE_OK;
}

unsigned host_key_of(const pie_ctx* c, long long e)
{
    if (e < c->key_base) return 0u;
    const unsigned long long k = ((unsigned long long)e - (unsigned long long)c->key_base) >> c->key_shift;
    return k >= (unsigned long long)(kKeyMax - 1u) ? kKeyMax : (unsigned)k + 1u;
}

// rows whose 15-bit key lies in the histogram bin of key(now) or above: an upper bound on the rows live at `now`
// (valid while the histogram describes the table: !key_dirty && key_hist_rows == n)
unsigned long long rows_keyed_at_or_above(const pie_ctx* c, long long now)
{
    const size_t bin = (size_t)(host_key_of(c, now) >> 3);
    return bin < c->key_hist_above.size() ? c->key_hist_above[bin] : 0ull;
}

unsigned host_fine_key_of(const pie_ctx* c, long long e)
{
    if (e < c->fkey_base) return 0u;
    const unsigned long long k = ((unsigned long long)e - (unsigned long long)c->fkey_base) >> c->fkey_shift;
    return k >= (unsigned long long)(kFineKeyMax - 1u) ? kFineKeyMax : (unsigned)k + 1u;
}

int resolve_events(pie_ctx* c)
{
    if (c->ring_used == 0) return PIE_OK;
    if (c->n_flight) return PIE_OK; // events of scans in flight are not closed yet; resolved on a later call
    int rc = sync_all(c);
    if (rc) return rc;
    for (int i = 0; i < c->ring_used; ++i) {
        float k1 = 0, all = 0;
        PIE_HIP(c, hipEventElapsedTime(&k1, c->ring[i].e0, c->ring[i].e1));
        PIE_HIP(c, hipEventElapsedTime(&all, c->ring[i].e0, c->ring[i].e2));
        c->k1_ms_sum += k1;
        c->scan_ms_sum += all;
        c->n_profiled++;
    }
    c->ring_used = 0;
    return PIE_OK;
}

// K1 forms.  Variant code: bit0 nontemporal loads, bit1 late user materialisation, bit2 liveness-first form
// (streams only `end`, gathers the other columns for live rows); bits 4,5,7 = unroll (0 -> 4, 0x20 -> 2, 0x80 -> 8);
// bit6 (0x40, liveness-first only) = wave-aggregated histogram atomics for skewed users.
// PIE_K1_VARIANT pins one form (tuning / A-B runs); otherwise the form follows the live fraction that the
// previous scan on this table observed: liveness-first below kLiveFirstBelow, the streaming form above.
constexpr double kLiveFirstBelow = 0.10; // measured crossover ~0.16 live (profiles/r01_c_live_fraction_crossover.txt)

void launch_k1(pie_ctx* c, Slot& sl, hipStream_t s, long long now, long long cutoff, unsigned long long mask)
{
#define PIE_K1(UN, NT, LU)                                                                                          \
    hipLaunchKernelGGL((k_scan_compact<UN, NT, LU>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start, c->d_end, \
                       c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, sl.counts, sl.sel, \
                       sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl))
#define PIE_K1L(UN, NT)                                                                                             \
    if (sl.variant & 0x40)                                                                                          \
        hipLaunchKernelGGL((k_scan_live_first<UN, NT, true>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start, c->d_end, \
                           c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, sl.counts, sl.sel, \
                           sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl), sl.hot, sl.blk_hot_base);          \
    else                                                                                                            \
        hipLaunchKernelGGL((k_scan_live_first<UN, NT, false>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start, c->d_end, \
                       c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, sl.counts, sl.sel, \
                       sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl), sl.hot, sl.blk_hot_base)
    if (sl.variant & 0x400) { // keyed liveness-first form
#define PIE_K1K3(UN, AG, NT, PP)                                                                                     \
        do {                                                                                                        \
            if (sl.variant & 0x800)                                                                                 \
                hipLaunchKernelGGL((k_scan_keyed<UN, AG, NT, fkey_t, PP>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_pay, \
                                   c->d_end, c->d_fkey, c->n, sl.rows_per_block, now, host_fine_key_of(c, now), cutoff, mask, \
                                   c->n_users, sl.counts, sl.sel, sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl), \
                                   sl.hot, sl.blk_hot_base, c->run_shift);                                          \
            else                                                                                                    \
                hipLaunchKernelGGL((k_scan_keyed<UN, AG, NT, lkey_t, PP>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_pay, \
                                   c->d_end, c->d_key, c->n, sl.rows_per_block, now, host_key_of(c, now), cutoff, mask,       \
                                   c->n_users, sl.counts, sl.sel, sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl), \
                                   sl.hot, sl.blk_hot_base, c->run_shift);                                          \
        } while (0)
#define PIE_K1K(UN, AG, NT)                                                                                          \
        do {                                                                                                        \
            if (sl.variant & 0x10) PIE_K1K3(UN, AG, NT, true);                                                       \
            else PIE_K1K3(UN, AG, NT, false);                                                                        \
        } while (0)
#define PIE_K1K2(UN)                                                                                                 \
        do {                                                                                                        \
            if (sl.variant & 0x40) { if (sl.variant & 1) PIE_K1K(UN, true, true); else PIE_K1K(UN, true, false); }   \
            else { if (sl.variant & 1) PIE_K1K(UN, false, true); else PIE_K1K(UN, false, false); }                   \
        } while (0)
        switch (sl.variant & 0xA0) {
        case 0x20: PIE_K1K2(2); break;
        case 0x80: PIE_K1K2(8); break;
        default: PIE_K1K2(4); break;
        }
#undef PIE_K1K2
#undef PIE_K1K3
#undef PIE_K1K
        return;
    }
    if (sl.variant == 0x101) { // group-qualified form, used only by pie_archive_queue
        hipLaunchKernelGGL((k_scan_compact<4, true, false, true>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start,
                           c->d_end, c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, sl.counts,
                           sl.sel, sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl), c->d_qual);
        return;
    }
    if (sl.variant == 0x43) { // streaming form with wave-aggregated histogram atomics (rows clustered by user)
        hipLaunchKernelGGL((k_scan_compact<4, true, true, false, true>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start,
                           c->d_end, c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, sl.counts,
                           sl.sel, sl.sel_rank, sl.blk_count, sl.sum, direct_of(c, sl));
        return;
    }
    switch (sl.variant & ~0x40) {
    case 0x00: PIE_K1(4, false, false); break;
    case 0x01: PIE_K1(4, true, false); break;
    case 0x02: PIE_K1(4, false, true); break;
    case 0x03: PIE_K1(4, true, true); break;
    case 0x04: PIE_K1L(4, false); break;
    case 0x05: PIE_K1L(4, true); break;
    case 0x24: PIE_K1L(2, false); break;
    case 0x25: PIE_K1L(2, true); break;
    case 0x84: PIE_K1L(8, false); break;
    case 0x85: PIE_K1L(8, true); break;
    case 0x20: PIE_K1(2, false, false); break;
    case 0x21: PIE_K1(2, true, false); break;
    case 0x22: PIE_K1(2, false, true); break;
    case 0x23: PIE_K1(2, true, true); break;
    case 0x80: PIE_K1(8, false, false); break;
    case 0x81: PIE_K1(8, true, false); break;
    case 0x82: PIE_K1(8, false, true); break;
    case 0x83: PIE_K1(8, true, true); break;
    default: sl.variant = 0x03; PIE_K1(4, true, true); break;
    }
#undef PIE_K1
#undef PIE_K1L
}

// per-bucket order of the buckets of <= kTinyMax rows; with direct slots it depends on K2 only (not on K3, not on the
// host), so it is queued right behind K2
void launch_sort_tiny(pie_ctx* c, Slot& sl, hipStream_t s)
{
    const int tiny_blocks = (c->n_users + 255) / 256;
    hipLaunchKernelGGL(k_sort_tiny, dim3(tiny_blocks), dim3(256), 0, s, sl.counts_ord, sl.offsets, c->n_users, sl.bkt, direct_of(c, sl), sl.out_idx, sl.hot);
}

// K2 (+ the order of the tiny buckets).  Three shapes: fused (one user per thread; offsets and tiny-bucket order in one
// kernel) when buckets have direct slots and the tile count suits the all-predecessors look-back; otherwise the
// 2048-user tiles, followed by the tiny-bucket kernel right away (direct slots) or after K3 (staged route).
constexpr int kOrderMaxTiles = 2048; // fused form: few enough tiles for the all-predecessors look-back

// a bucket is "hot" when it holds more than 1/256 of the rows the previous scan selected (and enough of them that
// same-address histogram atomics hurt): such users are reported for the next scan's hot set
int hot_threshold(const pie_ctx* c)
{
    return (c->last_m >= 65536 && !c->d_qual) ? (int)std::min<long long>(c->last_m / 256, 0x7FFFFFFF) : 0;
}

void launch_k2(pie_ctx* c, Slot& sl, hipStream_t s, int4* zero_span, long long zero_vec16)
{
    if (!zero_span) zero_vec16 = 0; // a scan outside the span rotation (the ordered run's build) zeroes nothing
    const int hot_thr = hot_threshold(c);
    const int ob = c->order_block;
    const int order_tiles = (c->n_users + ob - 1) / ob;
    if (sl.direct && order_tiles <= kOrderMaxTiles && !c->no_fused_order) {
#define PIE_K2O(B)                                                                                                          \
    hipLaunchKernelGGL((k_offsets<1, true, B>), dim3(order_tiles), dim3(B), 0, s, sl.counts, sl.counts_ord, c->n_users, sl.tile_pub, sl.ctl,   \
                       sl.offsets, sl.seg_list, sl.small_list, sl.big_list, sl.sum, sl.h_sum_dev, sl.seq, zero_span, zero_vec16, \
                       direct_of(c, sl), sl.bkt, sl.out_idx, sl.msg, sl.msg_u_pad, sl.msg_cap, sl.msg_counts, sl.hot, hot_thr, sl.hot_list, sl.over_list)
        if (ob == 256) PIE_K2O(256);
        else if (ob == 512) PIE_K2O(512);
        else PIE_K2O(1024);
#undef PIE_K2O
        sl.msg_by_k2 = sl.msg != nullptr;
        return;
    }
    hipLaunchKernelGGL((k_offsets<8, false, 256>), dim3(c->n_tiles), dim3(256), 0, s, sl.counts, sl.counts_ord, c->n_users, sl.tile_pub, sl.ctl,
                       sl.offsets, sl.seg_list, sl.small_list, sl.big_list, sl.sum, sl.h_sum_dev, sl.seq, zero_span, zero_vec16,
                       direct_of(c, sl), sl.bkt, (int*)nullptr, (int*)nullptr, 0, 0LL, (int*)nullptr, sl.hot, hot_thr, sl.hot_list, sl.over_list);
    sl.msg_by_k2 = false;
    if (sl.direct) launch_sort_tiny(c, sl, s);
}

// K2 of `tail` can ride in another scan's launch: fused form (direct slots), few enough 256-user tiles.  (Beside a
// table pass K2 takes about twice as long, so a caller that wants a scan's summary early should not begin the next scan
// first; the exchange driver in shard.py does its host work in that window instead.)
bool tail_can_ride(const pie_ctx* c, const Slot& tail)
{
    const int tiles = (c->n_users + kK1Threads - 1) / kK1Threads;
    return tail.direct != nullptr && tiles <= kOrderMaxTiles && !c->no_fused_order && !c->no_ride && !tail.fast && !c->d_qual;
}

// the default keyed forms (unroll 8, nontemporal loads, with or without wave aggregation; no pipelining) exist with a tail
bool keyed_can_carry(const pie_ctx* c, const Slot& sl)
{
    (void)c;
    return (sl.variant & ~0x840) == 0x485;
}

// ... and so do the plain streaming forms (nontemporal loads, unroll 4, with or without late user materialisation): the
// every-byte scan and dense queries on tables without an ordered run.  PIE_STREAM_RIDE=0 turns it off (A/B runs).
bool stream_can_carry(const pie_ctx* c, const Slot& sl)
{
    if (c->d_qual || !(sl.variant == 0x01 || sl.variant == 0x03)) return false;
    const char* v = getenv("PIE_STREAM_RIDE"); // read per scan (only on this rare form): in-process A/B runs flip it
    return !(v && atoi(v) == 0);
}

void launch_keyed_with_tail(pie_ctx* c, Slot& sl, Slot& tail, hipStream_t s, long long now, long long cutoff, unsigned long long mask)
{
    OffsetsArgs t;
    t.counts = tail.counts; t.counts_ord = tail.counts_ord; t.n_users = c->n_users; t.tile_pub = tail.tile_pub; t.ctl = tail.ctl;
    t.offsets = tail.offsets; t.seg_list = tail.seg_list; t.small_list = tail.small_list; t.big_list = tail.big_list;
    t.summary = tail.sum; t.host = tail.h_sum_dev; t.seq = tail.seq; t.zero_span = tail.zero_span;
    t.zero_vec16 = (long long)(counts_span(c) / 16); t.direct = direct_of(c, tail); t.bkt = tail.bkt; t.out_idx = tail.out_idx;
    t.msg = tail.msg; t.u_pad = tail.msg_u_pad; t.msg_cap = tail.msg_cap; t.msg_counts = tail.msg_counts; t.hot = tail.hot; t.hot_thr = hot_threshold(c);
    t.hot_list = tail.hot_list; t.over_list = tail.over_list;
    t.n_tail = (c->n_users + kK1Threads - 1) / kK1Threads;
    tail.msg_by_k2 = tail.msg != nullptr;
    const unsigned grid = (unsigned)(sl.k1_blocks + t.n_tail);
    if (!(sl.variant & 0x400)) { // a streaming form carries the tail
        StreamArgs a;
        a.start = c->d_start; a.end = c->d_end; a.user = c->d_user; a.disc = c->d_disc; a.n = c->n; a.rows_per_block = sl.rows_per_block;
        a.now = now; a.cutoff = cutoff; a.mask = mask; a.n_users = c->n_users; a.counts = sl.counts; a.sel = sl.sel; a.sel_rank = sl.sel_rank;
        a.blk_count = sl.blk_count; a.summary = sl.sum; a.direct = direct_of(c, sl);
        if (sl.variant & 2) hipLaunchKernelGGL((k_scan_compact_with_tail<true>), dim3(grid), dim3(kK1Threads), 0, s, a, t);
        else hipLaunchKernelGGL((k_scan_compact_with_tail<false>), dim3(grid), dim3(kK1Threads), 0, s, a, t);
        return;
    }
#define PIE_RIDE(KT, KEYPTR, NOWKEY)                                                                                     \
    do {                                                                                                                \
        KeyedArgs<KT> a;                                                                                                \
        a.pay = c->d_pay; a.end = c->d_end; a.key = KEYPTR; a.n = c->n; a.rows_per_block = sl.rows_per_block; a.now = now; \
        a.now_key = NOWKEY; a.cutoff = cutoff; a.mask = mask; a.n_users = c->n_users; a.counts = sl.counts; a.sel = sl.sel;  \
        a.sel_rank = sl.sel_rank; a.blk_count = sl.blk_count; a.summary = sl.sum; a.direct = direct_of(c, sl); a.hot = sl.hot; \
        a.blk_hot_base = sl.blk_hot_base; a.run_shift = c->run_shift;                                                   \
        if (sl.variant & 0x40) hipLaunchKernelGGL((k_scan_keyed_with_tail<8, true, KT, true>), dim3(grid), dim3(kK1Threads), 0, s, a, t);  \
        else hipLaunchKernelGGL((k_scan_keyed_with_tail<8, true, KT, false>), dim3(grid), dim3(kK1Threads), 0, s, a, t);   \
    } while (0)
    if (sl.variant & 0x800) PIE_RIDE(fkey_t, c->d_fkey, host_fine_key_of(c, now));
    else PIE_RIDE(lkey_t, c->d_key, host_key_of(c, now));
#undef PIE_RIDE
}

// Head of a scan: K1 and K2 on the stream (plus the tiny-bucket order kernel when buckets have direct slots).  No host wait.
// ------------------------------------------------------------------------------------------------ the ordered run (pie_ordered.h)

int scan_begin(pie_ctx* c, long long now, long long cutoff, int* msg, int msg_u_pad, long long msg_cap, int* msg_counts);
int scan_finish(pie_ctx* c, Slot* which = nullptr);

size_t ord_sum_bytes() { return span_stats_bytes() + 128; } // Summary + row-statistics slots, then OrdCtl

// arrays for the table's current capacity; no room is not an error (the general path serves every query)
int ord_alloc(pie_ctx* c)
{
    OrderedRun& o = c->ord;
    if (o.pay && o.cap >= c->cap_rows && o.cap_users >= c->cap_users) return PIE_OK;
    ord_free(c);
    // positions: every row of capacity, a sixteenth more and four per user as spare slots; then whole chunks of zero keys
    const size_t positions = (size_t)c->cap_rows + (size_t)c->cap_rows / 16 + (size_t)ord_spare(c) * (size_t)c->cap_users + 64;
    const size_t padded = ((positions + 1023) / 1024) * 1024 + 1024;
    if (padded + kOrdTile >= ((size_t)1 << 31)) { // positions are 31-bit (ring entries, staging records, pos[])
        o.no_room = true;
        return PIE_OK;
    }
    // a scan stages one 4-byte entry per position in the slot's record staging (sel): a table with far more users than rows
    // (four spare slots each) does not fit there, and has no use for the run anyway
    if ((padded + kOrdTile) * 4 > (size_t)c->sel_cap * sizeof(SelRec)) {
        o.no_room = true;
        return PIE_OK;
    }
    const size_t units = ((padded / 512 + 8 + 1023) / 1024) * 1024;              // the smallest unit is a 512-position chunk; whole groups
    const size_t tiles = padded / kOrdTile + 2;
    const bool ok = hipMalloc(&o.pay, padded * sizeof(OrdRec)) == hipSuccess && hipMalloc(&o.end, padded * 8) == hipSuccess &&
                    hipMalloc(&o.key, padded * sizeof(lkey_t)) == hipSuccess && hipMalloc(&o.fkey, padded * sizeof(fkey_t)) == hipSuccess &&
                    hipMalloc(&o.pos, (size_t)c->cap_rows * 4 + 64) == hipSuccess &&
                    hipMalloc(&o.uoff, ((size_t)c->cap_users + 1) * 8) == hipSuccess &&
                    hipMalloc(&o.ufill, ((size_t)c->cap_users + 1) * 4) == hipSuccess &&
                    hipMalloc(&o.pend, ((size_t)c->cap_users + 1) * 4) == hipSuccess && hipMalloc(&o.placed, 2 * (size_t)kOrdAppendMax * 4) == hipSuccess &&
                    hipMalloc(&o.bhead, ((size_t)c->cap_users + 1) * 4) == hipSuccess && hipMalloc(&o.bnext, (size_t)kOrdAppendMax * 4) == hipSuccess &&
                    hipMalloc(&o.tstage, kOrdTurnStageBytes) == hipSuccess &&
                    hipMalloc(&o.unit_count[0], units * 4) == hipSuccess && hipMalloc(&o.unit_count[1], units * 4) == hipSuccess &&
                    hipMalloc(&o.unit_local, units * 4) == hipSuccess && hipMalloc(&o.group_sum, (units / 1024 + 2) * 8) == hipSuccess &&
                    hipMalloc(&o.group_base, (units / 1024 + 2) * 8) == hipSuccess &&
                    hipMalloc(&o.tile_ballot, tiles * kOrdSlices * 8) == hipSuccess &&
                    hipMalloc(&o.tile_prefix, tiles * kOrdSlices * 4) == hipSuccess &&
                    hipMalloc(&o.sum[0], ord_sum_bytes()) == hipSuccess && hipMalloc(&o.sum[1], ord_sum_bytes()) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        ord_free(c);
        o.no_room = true;
        return PIE_OK;
    }
    o.cap = c->cap_rows;
    o.pos_cap = (long long)positions;
    o.cap_users = c->cap_users;
    o.units_cap = (long long)units;
    return PIE_OK;
}

// Build the run: ONE all-selecting scan on the general path (every row that any query can ever select: end above
// INT64_MIN, discipline inside the table) gives the rows in (user, start, row) order and the per-user segment starts;
// a gather makes the run's columns from them.  Nothing the scan learns about the table is kept: it is not a query.
int build_ordered(pie_ctx* c)
{
    OrderedRun& o = c->ord;
    if (c->n_flight > 1) return fail(c, PIE_E_STATE, "ordered run: two scans are in flight");
    hipStream_t s = c->stream;
    PIE_HIP(c, hipStreamSynchronize(s));
    timespec t0{};
    clock_gettime(CLOCK_MONOTONIC, &t0);
    int rc = ord_alloc(c);
    if (rc || !o.pay) return rc;
    struct Keep {
        unsigned long long mask; int n_disc, variant, dshift_want, next_slot, mode, run_shift, bdshift_want;
        bool pinned, fast, hot_bucket, clustered, key_poor, fkey_poor, profiling, last_was_batch, batch_poor;
        double live_frac; long long last_m; HotSet hot; unsigned hot_seen, hot_age; Slot* res;
    } k{c->disc_mask, c->n_disc, c->k1_variant, c->dshift_want, c->next_slot, o.mode, c->run_shift, c->bdshift_want,
        c->k1_pinned, c->fast_enabled, c->hot_bucket, c->clustered, c->key_poor, c->fkey_poor, c->profiling, c->last_was_batch, c->batch_poor,
        c->live_frac, c->last_m, c->hot, c->hot_seen, c->hot_age, c->res};
    c->disc_mask = ~0ull;
    c->n_disc = 64;
    c->k1_pinned = true;
    c->k1_variant = 0x43; // streaming, histogram atomics aggregated per wave: bounded whatever the row order (a user-clustered
                          // table would otherwise send 64 lanes to one counter, 10^8 times)
    c->fast_enabled = false;
    c->profiling = false;
    o.mode = 0;           // the scan below must not come back here
    // The build's scan stands OUTSIDE the span rotation.  A caller's scan may be in flight: its tail (launched at its finish,
    // i.e. after everything queued here) still reads its span, which a regular scan's K2 would zero for the scan after the
    // next.  So this scan zeroes nothing, its own span is wiped when it is done, and the rotation continues where it was.
    const int keep_span_next = c->span_next;
    c->ord_building = true;
    // one scan of the caller's may be in flight (a pipelined caller always has one): the build takes the free slot, and
    // finishes THAT slot; the caller's scan stays the oldest in flight
    Slot* built = &c->slot[c->next_slot];
    rc = scan_begin(c, INT64_MIN, INT64_MIN, nullptr, 0, 0, nullptr);
    if (rc == PIE_OK) rc = scan_finish(c, built);
    c->ord_building = false;
    (void)hipMemsetAsync(c->span[keep_span_next], 0, counts_span(c), s);
    c->span_next = keep_span_next;
    c->disc_mask = k.mask; c->n_disc = k.n_disc; c->k1_pinned = k.pinned; c->k1_variant = k.variant; c->fast_enabled = k.fast;
    c->profiling = k.profiling; o.mode = k.mode; c->dshift_want = k.dshift_want; c->hot_bucket = k.hot_bucket; c->clustered = k.clustered;
    c->key_poor = k.key_poor; c->fkey_poor = k.fkey_poor; c->live_frac = k.live_frac; c->last_m = k.last_m; c->hot = k.hot;
    c->hot_seen = k.hot_seen; c->hot_age = k.hot_age; c->last_was_batch = k.last_was_batch; c->run_shift = k.run_shift;
    c->bdshift_want = k.bdshift_want; c->batch_poor = k.batch_poor;
    if (rc) { // the caller's last result and slot order are as they were; the failed scan left nothing in flight of its own
        built->have_result = false;
        c->res = (k.res && k.res != built) ? k.res : nullptr;
        c->next_slot = k.next_slot;
        return rc;
    }
    const long long m = (long long)built->last.m;
    // segments: user u's rows, then spare slots for the rows to come (k_ord_append); users that do not exist yet get four
    const int seg_users = c->cap_users;
    std::vector<int> cnt((size_t)seg_users + 1, 0);
    PIE_HIP(c, hipMemcpyAsync(cnt.data(), built->counts_ord, (size_t)c->n_users * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    std::vector<long long> seg((size_t)seg_users + 1);
    long long total = 0;
    const int spare = ord_spare(c);
    for (int u = 0; u < seg_users; ++u) {
        seg[(size_t)u] = total;
        total += (long long)cnt[(size_t)u] + cnt[(size_t)u] / 16 + spare;
    }
    seg[(size_t)seg_users] = total;
    if (total > o.pos_cap) { o.no_room = true; return PIE_OK; } // cannot happen by ord_alloc's sizing; stay on the general path
    const size_t padded = (((size_t)o.pos_cap + 1023) / 1024) * 1024 + 1024;
    PIE_HIP(c, hipMemcpyAsync(o.uoff, seg.data(), ((size_t)seg_users + 1) * 8, hipMemcpyHostToDevice, s));
    PIE_HIP(c, hipMemcpyAsync(o.ufill, cnt.data(), ((size_t)seg_users + 1) * 4, hipMemcpyHostToDevice, s));
    PIE_HIP(c, hipMemsetAsync(o.pend, 0, ((size_t)seg_users + 1) * 4, s));
    PIE_HIP(c, hipMemsetAsync(o.bhead, 0xFF, ((size_t)seg_users + 1) * 4, s));
    PIE_HIP(c, hipMemsetAsync(o.pos, 0xFF, (size_t)o.cap * 4, s));
    PIE_HIP(c, hipMemsetAsync(o.pay, 0xFF, padded * sizeof(OrdRec), s)); // filler: discipline -1, never selected
    hipLaunchKernelGGL(k_fill_ll, dim3(c->n_cus * 8), dim3(256), 0, s, o.end, (long long)padded, (long long)INT64_MIN);
    PIE_HIP(c, hipMemsetAsync(o.key, 0, padded * sizeof(lkey_t), s));
    PIE_HIP(c, hipMemsetAsync(o.fkey, 0, padded * sizeof(fkey_t), s));
    PIE_HIP(c, hipMemsetAsync(o.unit_count[0], 0, (size_t)o.units_cap * 4, s));
    PIE_HIP(c, hipMemsetAsync(o.unit_count[1], 0, (size_t)o.units_cap * 4, s));
    PIE_HIP(c, hipMemsetAsync(o.sum[0], 0, ord_sum_bytes(), s));
    PIE_HIP(c, hipMemsetAsync(o.sum[1], 0, ord_sum_bytes(), s));
    if (m > 0) {
        hipLaunchKernelGGL(k_ord_gather, dim3(c->n_cus * 16), dim3(256), 0, s, built->out_idx, m, built->offsets, o.uoff, c->d_pay, c->d_end,
                           c->key_base, c->key_shift, c->fkey_base, c->fkey_shift, o.pay, o.end, o.key, o.fkey, o.pos);
        PIE_HIP(c, hipGetLastError());
    }
    PIE_HIP(c, hipStreamSynchronize(s));
    o.h_stale[0] = o.h_stale[1] = 0;
    // the build's scan is not a result: the caller's last one (in the other slot) stays readable, and the next scan takes
    // the slot it would have taken
    built->have_result = false;
    c->res = (k.res && k.res != built) ? k.res : nullptr;
    c->next_slot = k.next_slot;
    o.n = total;
    o.held = m;
    o.users = seg_users;
    o.rows = c->n;
    o.uc_next = 0;
    o.valid = true;
    o.wanted = 0;
    o.built_at = c->scans_begun;
    o.builds++;
    timespec t1{};
    clock_gettime(CLOCK_MONOTONIC, &t1);
    o.build_ms = (double)(t1.tv_sec - t0.tv_sec) * 1e3 + (double)(t1.tv_nsec - t0.tv_nsec) * 1e-6;
    return PIE_OK;
}

// stage: the device block that holds the k rows as [start k | end k | user k | disc k]: the append's own staging block, or the
// run's (ord.tstage) for the rows of a turn
void launch_ord_append(pie_ctx* c, hipStream_t s, const char* stage, size_t k, long long row0, int n_users, int pass)
{
    OrderedRun& o = c->ord;
    const unsigned grid = (unsigned)((k + 255) / 256);
    const int* st_user = reinterpret_cast<const int*>(stage + k * 16);
    if (pass == 2) (void)hipMemcpyAsync(o.placed + kOrdAppendMax, o.placed, k * 4, hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(k_ord_append_mark, dim3(grid), dim3(256), 0, s, st_user, (int)k, n_users, o.placed + kOrdAppendMax, pass, o.bhead, o.bnext);
    hipLaunchKernelGGL(k_ord_append, dim3(grid), dim3(256), 0, s, reinterpret_cast<const long long*>(stage),
                       reinterpret_cast<const long long*>(stage + k * 8), st_user, reinterpret_cast<const int*>(stage + k * 20), (int)k,
                       row0, n_users, c->key_base, c->key_shift, c->fkey_base, c->fkey_shift, o.uoff, o.ufill, o.pay, o.end, o.key, o.fkey,
                       o.pos, o.stale, o.placed + kOrdAppendMax, o.placed, pass == 1 ? o.pend : (int*)nullptr, pass, o.bhead, o.bnext);
}

// Segments are full: give every user fresh spare slots (its rows, the rows of this append still waiting, a sixteenth more,
// four) and move the run there — a linear pass, no sort.  Then the waiting rows of the append (still in the staging block
// `stage`, as launch_ord_append read them in pass 1) take their places.  Returns with the run valid, or invalid when it no longer
// fits / the second pass failed too.
int ord_respread(pie_ctx* c, const char* stage, size_t k, long long row0, int n_users)
{
    OrderedRun& o = c->ord;
    hipStream_t s = c->stream;
    const size_t padded = (((size_t)o.pos_cap + 1023) / 1024) * 1024 + 1024;
    if (!o.alt_pay) {
        const bool ok = hipMalloc(&o.alt_pay, padded * sizeof(OrdRec)) == hipSuccess && hipMalloc(&o.alt_end, padded * 8) == hipSuccess &&
                        hipMalloc(&o.alt_key, padded * sizeof(lkey_t)) == hipSuccess && hipMalloc(&o.alt_fkey, padded * sizeof(fkey_t)) == hipSuccess &&
                        hipMalloc(&o.alt_uoff, ((size_t)o.cap_users + 1) * 8) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            dfree(o.alt_pay); dfree(o.alt_end); dfree(o.alt_key); dfree(o.alt_fkey); dfree(o.alt_uoff);
            ord_invalidate(c);
            return PIE_OK;
        }
    }
    const int seg_users = o.users;
    std::vector<int> fill((size_t)seg_users + 1), pend((size_t)seg_users + 1);
    PIE_HIP(c, hipMemcpyAsync(fill.data(), o.ufill, (size_t)seg_users * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipMemcpyAsync(pend.data(), o.pend, (size_t)seg_users * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipMemsetAsync(o.pend, 0, ((size_t)seg_users + 1) * 4, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    std::vector<long long> seg((size_t)seg_users + 1);
    long long total = 0;
    for (int u = 0; u < seg_users; ++u) {
        seg[(size_t)u] = total;
        const long long rows = (long long)fill[(size_t)u] + pend[(size_t)u];
        total += rows + rows / 16 + ord_spare(c);
    }
    seg[(size_t)seg_users] = total;
    if (total > o.pos_cap) { // the table has outgrown what the run's arrays were sized for: a rebuild re-allocates
        ord_free(c);
        return PIE_OK;
    }
    PIE_HIP(c, hipMemcpyAsync(o.alt_uoff, seg.data(), ((size_t)seg_users + 1) * 8, hipMemcpyHostToDevice, s));
    PIE_HIP(c, hipMemsetAsync(o.alt_pay, 0xFF, padded * sizeof(OrdRec), s));
    hipLaunchKernelGGL(k_fill_ll, dim3(c->n_cus * 8), dim3(256), 0, s, o.alt_end, (long long)padded, (long long)INT64_MIN);
    PIE_HIP(c, hipMemsetAsync(o.alt_key, 0, padded * sizeof(lkey_t), s));
    PIE_HIP(c, hipMemsetAsync(o.alt_fkey, 0, padded * sizeof(fkey_t), s));
    hipLaunchKernelGGL(k_ord_respread, dim3(c->n_cus * 16), dim3(256), 0, s, o.n, seg_users, o.uoff, o.ufill, o.alt_uoff, o.pay, o.end, o.key,
                       o.fkey, o.alt_pay, o.alt_end, o.alt_key, o.alt_fkey, o.pos);
    PIE_HIP(c, hipGetLastError());
    std::swap(o.pay, o.alt_pay);
    std::swap(o.end, o.alt_end);
    std::swap(o.key, o.alt_key);
    std::swap(o.fkey, o.alt_fkey);
    std::swap(o.uoff, o.alt_uoff);
    o.n = total;
    o.respreads++;
    o.h_stale[0] = o.h_stale[1] = 0;
    launch_ord_append(c, s, stage, k, row0, n_users, 2);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipStreamSynchronize(s));
    if (*(volatile unsigned int*)&o.h_stale[0] || *(volatile unsigned int*)&o.h_stale[1]) {
        o.h_stale[0] = o.h_stale[1] = 0;
        ord_invalidate(c);
    }
    return PIE_OK;
}

long long batch_users_stride(const pie_ctx* c);
long long batch_out_stride(const pie_ctx* c);
size_t batch_ucap(const pie_ctx* c);
size_t batch_mq_bytes();

// the batched form's per-query arrays (allocated at the first ordered batch)
int ord_batch_alloc(pie_ctx* c)
{
    OrderedRun& o = c->ord;
    if (o.bq_local) return PIE_OK;
    const size_t units = (size_t)o.units_cap, groups = units / 1024 + 2;
    const bool ok = hipMalloc(&o.bq_local, units * 4) == hipSuccess && hipMalloc(&o.bq_gsum, groups * 8) == hipSuccess &&
                    hipMalloc(&o.bq_gbase, groups * 8) == hipSuccess && hipMalloc(&o.bq_ctl, sizeof(OrdCtl)) == hipSuccess &&
                    hipMalloc(&o.bq_sum[0], ord_sum_bytes() + batch_mq_bytes()) == hipSuccess &&
                    hipMalloc(&o.bq_sum[1], ord_sum_bytes() + batch_mq_bytes()) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        dfree(o.bq_local); dfree(o.bq_gsum); dfree(o.bq_gbase); dfree(o.bq_ctl); dfree(o.bq_sum[0]); dfree(o.bq_sum[1]);
        return PIE_E_NOMEM;
    }
    PIE_HIP(c, hipMemsetAsync(o.bq_ctl, 0, sizeof(OrdCtl), c->stream));
    PIE_HIP(c, hipMemsetAsync(o.bq_sum[0], 0, ord_sum_bytes() + batch_mq_bytes(), c->stream));
    PIE_HIP(c, hipMemsetAsync(o.bq_sum[1], 0, ord_sum_bytes() + batch_mq_bytes(), c->stream));
    return PIE_OK;
}

// can this batch run on the ordered run?  (a table whose batches the general pass cannot hold: skewed users)
bool ordered_batch_wanted(const pie_ctx* c)
{
    const OrderedRun& o = c->ord;
    if (o.mode == 0 || !o.valid || o.rows != c->n || c->d_qual || !c->key_ok || c->key_poor) return false;
    if (!(o.mode == 2 || c->batch_poor || c->hot_bucket)) return false;
    // union staging records (8 B per position) live in the scan slots' record staging
    const size_t padded = (((size_t)o.pos_cap + 1023) / 1024) * 1024 + 1024;
    return (padded + kOrdTile) * sizeof(OrdUnion) <= (size_t)c->sel_cap * sizeof(SelRec);
}

void fill_batch_tables(const pie_ctx* c, const BatchSlot& b, const pie_query* qs, const unsigned* nk, BatchTables& t);
void fill_batch_tables(int n_disc, int n_q, const bool* fallback, const pie_query* qs, const unsigned* nk, BatchTables& t);

// a batch on the ordered run (up to 64 queries): scan, ONE prefix, emit, publish — see pie_ordered.h "the UNION form"
void launch_ordered_union(pie_ctx* c, BatchSlot& b, hipStream_t s, const pie_query* qs, bool fine)
{
    OrderedRun& o = c->ord;
    const int bi = (int)(&b - c->bslot) & 1; // scratch (staging, device summary) of two sets: chains run one after the other in the stream
    char* sums = o.bq_sum[bi];
    int* uc = o.unit_count[o.uc_next];
    int* uc_other = o.unit_count[o.uc_next ^ 1];
    o.uc_next ^= 1;
    OrdUnion* ustage = reinterpret_cast<OrdUnion*>(c->slot[bi].sel);
    const unsigned impossible = fine ? 0xFFu : 0xFFFFu; // (a query that falls back is not in the tables)
    unsigned mk = impossible, nk[kBatchMax];
    for (int q = 0; q < b.n_q; ++q) {
        nk[q] = fine ? host_fine_key_of(c, qs[q].now) : host_key_of(c, qs[q].now);
        if (!b.fallback[q] && nk[q] < mk) mk = nk[q];
    }
    BatchTables tab;
    fill_batch_tables(c, b, qs, nk, tab);
    const int chunk_shift = 9;
    const long long n_chunks = (o.n + (1 << chunk_shift) - 1) >> chunk_shift;
    Summary* sum0 = reinterpret_cast<Summary*>(sums);
    unsigned int* mq_slots = reinterpret_cast<unsigned int*>(sums + ord_sum_bytes()); // behind the summary: its own, zero between batches
    if (fine) {
        const int gm = o.grid_mult;
        long long grid = (n_chunks + 3) / 4 < (long long)c->n_cus * gm ? (n_chunks + 3) / 4 : (long long)c->n_cus * gm;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL((k_ord_batch_scan_t<fkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.fkey, o.n, n_chunks, mk, tab, ustage, uc, sum0);
    } else {
        long long grid = (n_chunks + 3) / 4 < (long long)c->n_cus * 6 ? (n_chunks + 3) / 4 : (long long)c->n_cus * 6;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL((k_ord_batch_scan_t<lkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.key, o.n, n_chunks, mk, tab, ustage, uc, sum0);
    }
    if (b.ev_index >= 0) (void)hipEventRecord(c->ring[b.ev_index].e1, s);
    long long n_groups = (n_chunks + kOrdGroup - 1) >> kOrdGroupShift;
    if (n_groups < 1) n_groups = 1;
    const unsigned pre_grid = (unsigned)(n_groups < (long long)c->n_cus ? n_groups : (long long)c->n_cus);
    hipLaunchKernelGGL(k_ord_prefix, dim3(pre_grid), dim3(256), 0, s, uc, n_chunks, o.bq_local, o.bq_gsum, o.bq_gbase, o.bq_ctl, sum0, 0LL, 0LL, 0LL);
    const int copy_blocks = c->n_cus * 8;
    const int user_blocks = (int)(((long long)c->n_users + 1 + 254) / 255);
    const unsigned egrid = (unsigned)(copy_blocks + user_blocks);
    if (b.n_q > 32)
        hipLaunchKernelGGL((k_ord_union_emit<true>), dim3(egrid), dim3(256), 0, s, o.uoff, c->n_users, o.n, chunk_shift, n_chunks, b.n_q, tab, ustage, uc, o.bq_local,
                           o.bq_gbase, b.uoff, b.urows, b.umlo, b.umhi, (long long)batch_ucap(c), copy_blocks, sum0, mq_slots, uc_other, o.units_cap);
    else
        hipLaunchKernelGGL((k_ord_union_emit<false>), dim3(egrid), dim3(256), 0, s, o.uoff, c->n_users, o.n, chunk_shift, n_chunks, b.n_q, tab, ustage, uc, o.bq_local,
                           o.bq_gbase, b.uoff, b.urows, b.umlo, b.umhi, (long long)batch_ucap(c), copy_blocks, sum0, mq_slots, uc_other, o.units_cap);
    hipLaunchKernelGGL(k_ord_union_publish, dim3(1), dim3(256), 0, s, sum0, mq_slots, b.n_q, (long long)batch_ucap(c), b.bh_dev, b.seq);
}

// should this query run on the ordered run?  (mode 1: where the general path is weak)
bool ordered_wanted(const pie_ctx* c)
{
    if (c->ord.mode == 2) return true;
    if (c->ord.mode == 0) return false;
    return c->hot_bucket || c->batch_poor || (c->last_m >= 0 && c->last_m * 24 > c->n);
}

// keyed (sparse) or dense form: an upper bound on the candidate rows — the key histogram while it describes the
// table, else the live fraction of the last scan
bool ordered_keyed_form(const pie_ctx* c, long long now)
{
    if (c->key_poor) return false;
    double frac = c->live_frac >= 0 ? c->live_frac : 1.0;
    if (!c->key_dirty && c->key_hist_rows == c->n && c->n > 0) {
        frac = (double)rows_keyed_at_or_above(c, now) / (double)c->n;
    }
    return frac < 0.08;
}

// scan kernel, prefix, emit, publish: four launches, nothing to do at pie_scan_finish but read the summary
void launch_ordered(pie_ctx* c, Slot& sl, hipStream_t s, long long now, long long cutoff, unsigned long long mask)
{
    OrderedRun& o = c->ord;
    const int si = (int)(&sl - c->slot);
    Summary* sum = reinterpret_cast<Summary*>(o.sum[si]);
    sl.sum = sum; // what a later pack of this slot's result reads M from
    OrdCtl* ctl = reinterpret_cast<OrdCtl*>(o.sum[si] + span_stats_bytes());
    int* uc = o.unit_count[o.uc_next];
    int* uc_other = o.unit_count[o.uc_next ^ 1];
    o.uc_next ^= 1;
    unsigned int* stage = reinterpret_cast<unsigned int*>(sl.sel);
    const bool keyed = ordered_keyed_form(c, now);
    const bool fine = keyed && (c->k1_keyed & 0x800) && !c->fkey_poor && now >= c->fkey_base;
    long long n_units;
    int unit_shift;
    if (!keyed) {
        unit_shift = kOrdTileShift;
        n_units = (o.n + kOrdTile - 1) >> kOrdTileShift;
        long long grid = n_units < (long long)c->n_cus * 8 ? n_units : (long long)c->n_cus * 8;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL(k_ord_scan_dense, dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.key, o.n, now, host_key_of(c, now),
                           cutoff, mask, stage, uc, o.tile_ballot, o.tile_prefix, sum);
        sl.variant = 0x2003;
    } else if (fine) {
        unit_shift = 9;
        n_units = (o.n + 511) >> 9;
        const int gm = o.grid_mult; // blocks per CU (profiles/r02_ze_ord_keyed_grid_unroll_sweep.txt: 12 beats 4 .. 10; the unroll does not matter)
        long long grid = (n_units + 3) / 4 < (long long)c->n_cus * gm ? (n_units + 3) / 4 : (long long)c->n_cus * gm;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL((k_ord_scan_keyed<fkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.fkey, o.n, n_units, now,
                           host_fine_key_of(c, now), cutoff, mask, stage, uc, sum);
        sl.variant = 0x2C00;
    } else {
        unit_shift = 9;
        n_units = (o.n + 511) >> 9;
        long long grid = (n_units + 3) / 4 < (long long)c->n_cus * 8 ? (n_units + 3) / 4 : (long long)c->n_cus * 8;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL((k_ord_scan_keyed<lkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.key, o.n, n_units, now,
                           host_key_of(c, now), cutoff, mask, stage, uc, sum);
        sl.variant = 0x2400;
    }
    sl.k1_blocks = 0;
    if (sl.ev_index >= 0) (void)hipEventRecord(c->ring[sl.ev_index].e1, s);
    long long n_groups = (n_units + kOrdGroup - 1) >> kOrdGroupShift;
    if (n_groups < 1) n_groups = 1;
    const unsigned pre_grid = (unsigned)(n_groups < (long long)c->n_cus * 4 ? n_groups : (long long)c->n_cus * 4);
    hipLaunchKernelGGL(k_ord_prefix, dim3(pre_grid), dim3(256), 0, s, uc, n_units, o.unit_local, o.group_sum, o.group_base, ctl, sum, 0LL, 0LL, 0LL);
    const int fin_blocks = (int)(((long long)c->n_users + 1 + 254) / 255);
    if (keyed) {
        const int copy_blocks = c->n_cus * 8;
        hipLaunchKernelGGL(k_ord_emit<true>, dim3((unsigned)(copy_blocks + fin_blocks)), dim3(256), 0, s, o.uoff, c->n_users, o.n, unit_shift,
                           uc, o.unit_local, o.group_base, n_units, stage, o.pay, o.tile_ballot, o.tile_prefix, sl.out_idx, sl.offsets,
                           sl.counts_ord, copy_blocks, sum, uc_other, o.units_cap);
    } else {
        long long copy_blocks = n_units < (long long)c->n_cus * 16 ? n_units : (long long)c->n_cus * 16;
        if (copy_blocks < 1) copy_blocks = 1;
        hipLaunchKernelGGL(k_ord_emit<false>, dim3((unsigned)(copy_blocks + fin_blocks)), dim3(256), 0, s, o.uoff, c->n_users, o.n, unit_shift,
                           uc, o.unit_local, o.group_base, n_units, stage, o.pay, o.tile_ballot, o.tile_prefix, sl.out_idx, sl.offsets,
                           sl.counts_ord, (int)copy_blocks, sum, uc_other, o.units_cap);
    }
    hipLaunchKernelGGL(k_ord_publish, dim3(1), dim3(64), 0, s, sum, sl.h_sum_dev, sl.seq, 0LL);
}

int scan_begin(pie_ctx* c, long long now, long long cutoff, int* msg = nullptr, int msg_u_pad = 0, long long msg_cap = 0,
               int* msg_counts = nullptr);
int scan_begin(pie_ctx* c, long long now, long long cutoff, int* msg, int msg_u_pad, long long msg_cap, int* msg_counts)
{
    queue_forget(c); // the slots' workspace is about to be reused
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (c->n_flight >= 2) return fail(c, PIE_E_STATE, "two scans are already in flight: call pie_scan_finish first");
    if (c->key_rebuild && c->n_flight == 0) {
        int rc = build_keys(c, 0, true);
        if (rc) return rc;
    }
    if (c->dshift_want > c->dshift && c->n_flight == 0 && c->slot[0].direct) {
        // larger direct slots for every user: both slots' arrays are replaced (their contents are per-scan)
        int rc = sync_all(c);
        if (rc) return rc;
        BktRec* fresh[2] = {nullptr, nullptr};
        const size_t bytes = ((size_t)c->cap_users << c->dshift_want) * sizeof(BktRec);
        if (hipMalloc(&fresh[0], bytes) == hipSuccess && hipMalloc(&fresh[1], bytes) == hipSuccess) {
            for (int k = 0; k < 2; ++k) {
                (void)hipFree(c->slot[k].direct);   // scratch of finished scans only: their results live in out_idx / offsets / counts
                c->slot[k].direct = fresh[k];
            }
            c->dshift = c->dshift_want;
        } else {
            (void)hipGetLastError();
            if (fresh[0]) (void)hipFree(fresh[0]);
            c->dshift_want = c->dshift; // no room: stay with what there is
        }
    }
    // The ordered run serves the queries the general path is weak at (dense, skewed users).  It is built the second time
    // in a row such a query arrives with nothing in flight and the table unchanged (a first dense query may be the only one).
    bool ord_route = false;
    if (!c->d_qual && !c->k1_pinned && c->key_ok && !c->ord.no_room && ordered_wanted(c)) {
        if (!c->ord.valid && c->n_flight <= 1 && (c->ord.mode == 2 || ++c->ord.wanted >= c->ord.need)) {
            int rc = build_ordered(c);
            if (rc) return rc;
        }
        ord_route = c->ord.valid && c->ord.rows == c->n;
    } else c->ord.wanted = 0;
    Slot& sl = c->slot[c->next_slot];
    hipStream_t s = c->stream;
    sl.dshift = sl.direct ? c->dshift : 0;
    sl.ev_index = -1;
    if (c->profiling && (c->scans_begun % (unsigned long long)c->profile_every) == 0) {
        if (c->ring_used == kEventRing) {
            int rc = resolve_events(c);
            if (rc) return rc;
        }
        if (c->ring_used < kEventRing) {
            if ((int)c->ring.size() <= c->ring_used) {
                ScanEvents e{};
                PIE_HIP(c, hipEventCreate(&e.e0));
                PIE_HIP(c, hipEventCreate(&e.e1));
                PIE_HIP(c, hipEventCreate(&e.e2));
                c->ring.push_back(e);
            }
            sl.ev_index = c->ring_used++;
        }
    }
    const unsigned long long mask = c->n_disc >= 64 ? c->disc_mask : (c->disc_mask & ((1ull << c->n_disc) - 1ull));
    sl.variant = c->k1_variant;
    if (c->d_qual) sl.variant = 0x101;
    else if (!c->k1_pinned && c->live_frac >= 0) {
        sl.variant = c->live_frac < kLiveFirstBelow ? c->k1_live_first : c->k1_variant;
        // few candidates: stream the 2-byte liveness key instead of the 8-byte `end` column
        if ((sl.variant & 4) && c->keyed_enabled && c->key_ok && !c->key_poor) {
            sl.variant = c->k1_keyed & ~0x800;
            // queries above the fine key's base (every query that few rows survive) stream 1 B/row instead of 2
            if ((c->k1_keyed & 0x800) && !c->fkey_poor && now >= c->fkey_base) sl.variant |= 0x800;
        }
    }
    else if (!c->k1_pinned && !c->d_qual && c->live_frac < 0 && c->keyed_enabled && c->key_ok && !c->key_dirty &&
             c->key_hist_rows == c->n && c->n > 0) {
        // first scan of a table: no scan has counted live rows yet, but the key histogram taken when the key columns were
        // built bounds them: rows whose key bin lies at or above the bin of key(now) (an upper bound on the live rows)
        if ((double)rows_keyed_at_or_above(c, now) < kLiveFirstBelow * (double)c->n) {
            sl.variant = c->k1_keyed & ~0x800;
            if ((c->k1_keyed & 0x800) && now >= c->fkey_base) sl.variant |= 0x800;
        }
    }
    if ((sl.variant & 0x400) && !c->key_ok) sl.variant = c->k1_live_first; // pinned keyed form without a key column
    // rows clustered by user + a dense query: the streaming form aggregates its histogram atomics per wave
    if (!c->k1_pinned && !c->d_qual && sl.variant == 0x03 && c->clustered) sl.variant = 0x43;
    // skewed users (one bucket held > 1/64 of the last scan's selected rows): aggregate the histogram atomics per wave
    if (!c->k1_pinned && !c->d_qual && (sl.variant & 4) && c->hot_bucket) sl.variant |= 0x40;
    sl.hot.n = 0;
    if ((sl.variant & 0x44) == 0x44 && !c->d_qual) sl.hot = c->hot; // aggregated forms only; K1 and K3 of this scan share it
    const int plan = (sl.variant & 0x800) ? 3 : (sl.variant & 0x400) ? 2 : (sl.variant & 4) ? 1 : 0;
    sl.k1_blocks = c->plan_blocks[plan];
    sl.rows_per_block = c->plan_rows[plan];
    sl.have_result = false;
    if (c->res == &sl) c->res = nullptr;
    sl.msg = msg;
    sl.msg_u_pad = msg_u_pad;
    sl.msg_cap = msg_cap;
    sl.msg_counts = msg_counts;
    sl.msg_by_k2 = false;
    sl.ordered = false;

    if (ord_route) {
        {
            Slot& prev = c->slot[c->next_slot ^ 1];
            if (c->n_flight == 1 && prev.in_flight && prev.k2_pending) { // nothing carries it along: it goes first
                launch_k2(c, prev, s, prev.zero_span, (long long)(counts_span(c) / 16));
                prev.k2_pending = false;
            }
            sl.ordered = true;
            sl.fast = false;
            sl.k2_pending = false;
            sl.hot.n = 0;
            c->scans_begun++;
            sl.q_now = now;
            sl.q_cutoff = cutoff;
            sl.seq = ++c->seq_counter;
            if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e0, s));
            launch_ordered(c, sl, s, now, cutoff, mask);
            PIE_HIP(c, hipGetLastError());
            if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e2, s));
            sl.in_flight = true;
            c->n_flight++;
            c->next_slot ^= 1;
            return PIE_OK;
        }
    }

    // this scan's histogram span (zeroed by the previous scan's K2, or by the load) and the one K2 will zero
    {
        char* base = c->span[c->span_next];
        sl.counts = reinterpret_cast<int*>(base);
        sl.tile_pub = reinterpret_cast<unsigned long long*>(base + span_counts_bytes(c));
        sl.part_cursor = reinterpret_cast<int*>(base + span_counts_bytes(c) + span_tiles_bytes(c));
        sl.ctl = reinterpret_cast<ScanCtl*>(base + span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes());
        sl.sum = reinterpret_cast<Summary*>(base + span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes() + 128);
        c->span_next = (c->span_next + 1) % 3;
    }
    // K2 (or the fast path's tail) zeroes the span of the scan AFTER the next one: every span is clean again before its
    // next user starts, and K2 of this scan may run beside the next scan's table pass, which uses span_next
    int4* zero_span = reinterpret_cast<int4*>(c->span[(c->span_next + 1) % 3]);
    if (c->ord_building) zero_span = nullptr; // see build_ordered: this scan stands outside the rotation
    sl.zero_span = zero_span;
    c->scans_begun++;
    sl.q_now = now;
    sl.q_cutoff = cutoff;
    sl.seq = ++c->seq_counter;
    // Partitioned fast path: the query is sparse (liveness-first form chosen), the previous scan's M says a user
    // range of 1 << part_shift users holds far fewer than kPartCap selected rows, and no partition ever overflowed
    // on this table.  Two launches, no host round trip: K1P, then the one-wave-per-partition tail.
    sl.fast = false;
    if (!c->k1_pinned && !c->d_qual && c->fast_enabled && (sl.variant & 4) && c->part_shift >= 0 && c->last_m >= 0) {
        const double mean = (double)c->last_m / (double)c->n_parts;
        sl.fast = mean + 6.0 * __builtin_sqrt(mean) + 16.0 <= (double)kPartCap;
    }
    if (sl.fast) {
        // the fast path's tail zeroes the span the scan in flight still needs for its K2: that K2 goes first
        Slot& prev = c->slot[c->next_slot ^ 1];
        if (c->n_flight == 1 && prev.in_flight && prev.k2_pending) {
            launch_k2(c, prev, s, prev.zero_span, (long long)(counts_span(c) / 16));
            prev.k2_pending = false;
        }
        sl.variant = 0x285;
        sl.k1_blocks = c->plan_blocks[1];
        sl.rows_per_block = c->plan_rows[1];
        if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e0, s));
        hipLaunchKernelGGL((k_scan_live_first_part<8, true>), dim3(sl.k1_blocks), dim3(kK1Threads), 0, s, c->d_start, c->d_end,
                           c->d_user, c->d_disc, c->n, sl.rows_per_block, now, cutoff, mask, c->n_users, c->part_shift,
                           sl.part_cursor, sl.part_rec, sl.sum);
        if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e1, s));
        const unsigned tail_waves = kTailThreads / 64;
        unsigned tail_blocks = (unsigned)((c->n_parts + tail_waves - 1) / tail_waves);
        if (tail_blocks > (unsigned)c->n_cus) tail_blocks = (unsigned)c->n_cus;
        hipLaunchKernelGGL(k_tail_partitions, dim3(tail_blocks), dim3(kTailThreads), 0, s, sl.part_cursor, sl.part_rec, c->n_parts,
                           c->part_shift, c->n_users, sl.counts_ord, sl.offsets, sl.out_idx, sl.sum,
                           reinterpret_cast<unsigned int*>(sl.blk_count), zero_span, (long long)(counts_span(c) / 16));
        hipLaunchKernelGGL(k_publish_summary, dim3(1), dim3(256), 0, s, sl.sum, reinterpret_cast<unsigned int*>(sl.blk_count),
                           (int)tail_blocks, sl.h_sum_dev, sl.seq);
        PIE_HIP(c, hipGetLastError());
        if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e2, s));
        sl.in_flight = true;
        c->n_flight++;
        c->next_slot ^= 1;
        return PIE_OK;
    }
    // K2 of the scan already in flight (if it is still pending) rides in this scan's launch when both fit the fused
    // kernel; otherwise it goes first, on its own
    Slot& other = c->slot[c->next_slot ^ 1];
    const bool ride = c->n_flight == 1 && other.in_flight && other.k2_pending && tail_can_ride(c, other) &&
                      (keyed_can_carry(c, sl) || stream_can_carry(c, sl));
    if (c->n_flight == 1 && other.in_flight && other.k2_pending && !ride) {
        launch_k2(c, other, s, other.zero_span, (long long)(counts_span(c) / 16));
        other.k2_pending = false;
    }
    if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e0, s));
    if (ride) {
        launch_keyed_with_tail(c, sl, other, s, now, cutoff, mask);
        other.k2_pending = false;
    } else {
        launch_k1(c, sl, s, now, cutoff, mask);
    }
    if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e1, s));
    sl.k2_pending = true; // launched by the next pie_scan_begin (riding) or by pie_scan_finish, whichever comes first
    PIE_HIP(c, hipGetLastError());
    sl.in_flight = true;
    c->n_flight++;
    c->next_slot ^= 1;
    return PIE_OK;
}

// Chunk interleave of the next keyed / batched pass, from what the last one saw: `chunk_max` = candidates in its densest
// chunk (1024 or 512 rows), `cand` = all candidates.  Live rows spread evenly (the synthetic corpus of SURVEY.md 8d: a
// chunk holds a handful) -> eight consecutive chunks per wave; a chunk that is an eighth full while the average chunk
// is nearly empty (a session table in creation order: every live row at its end; a login burst) -> fully interleaved.
void choose_run_shift(pie_ctx* c, unsigned long long cand, unsigned chunk_max, bool fine_key)
{
    if (c->run_shift_pinned) return;
    const double rows_per_chunk = fine_key ? (double)kFineKeyRowsPerLoad : (double)kKeyRowsPerLoad;
    const double chunks = (double)c->n / rows_per_chunk;
    if (chunks < 1.0) return;
    const double mean = (double)cand / chunks;
    const bool dense_stretch = (double)chunk_max >= rows_per_chunk / 8.0 && (double)chunk_max > 8.0 * (mean + 1.0);
    c->run_shift = dense_stretch ? 0 : 3;
}

// Tail of the oldest scan in flight: launch its K2 if no later scan took it along, wait for its summary, then — only for
// buckets that outgrew their direct slots — scatter + per-bucket order (plus the merge passes of big buckets, sized from
// the summary).  Also where the adaptive choices for the next scans are made (scan form, key fit, hot set, slot capacity).
// `which`: finish THIS slot's scan although an older one is still in flight (the ordered run's build, which must not
// consume the caller's scan); everything a finish launches works on its own slot's arrays, in stream order
int scan_finish(pie_ctx* c, Slot* which)
{
    Slot* slp = which ? which : oldest_in_flight(c);
    if (!slp) return fail(c, PIE_E_STATE, "pie_scan_finish without pie_scan_begin");
    Slot& sl = *slp;
    hipStream_t a = c->stream;
    const bool e2_recorded = sl.k2_pending && sl.ev_index >= 0;
    if (sl.k2_pending) { // no later scan took it along
        launch_k2(c, sl, a, sl.zero_span, (long long)(counts_span(c) / 16));
        PIE_HIP(c, hipGetLastError());
        sl.k2_pending = false;
        // "last kernel end" of a scan whose buckets all fit their slots is the end of K2: the event goes in right behind it,
        // not after the host has woken up on the summary (a scan that needs K3 / K4 records it again behind those)
        if (sl.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e2, a));
    }
    // wait for K2's last block to publish the summary in mapped host memory (no copy node, no event wait).  The wait is
    // bounded (PIE_WAIT_DEADLINE_MS, default 20 s): a kernel that never finishes must not hang the caller — in the Node
    // host that is the JS main thread.  The slot stays in flight until its summary has been read, so an error return
    // leaves the context consistent: the failed scan is dropped (no result), the stream is left to drain.  Drained: the stream
    // has drained but the mapped write is not visible; the device copy is read instead (the ordered run has none and waits on).
    {
        const WaitResult w = word_wait(c, &sl.h_sum->seq, sl.seq, [&] { return hipStreamQuery(c->stream); }, sl.ordered ? kNoGraceLimit : 0.0, kPaceSummary);
        if (w.end == WaitEnd::Failed || w.end == WaitEnd::Deadline) {
            sl.in_flight = false;
            sl.have_result = false;
            c->n_flight--;
            if (c->res == &sl) c->res = nullptr;
            if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "scan failed: %s", hipGetErrorString((hipError_t)w.err));
            return fail(c, PIE_E_HIP, "scan summary not published within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", c->wait_deadline_ms);
        }
        if (w.end == WaitEnd::Drained) {
            // K2 writes live / amb only to the host copy: take every other field from the device Summary and the row
            // statistics from their slots (the same sum K2's last block makes)
            std::vector<unsigned char> raw(span_stats_bytes());
            hipError_t e = hipMemcpy(raw.data(), sl.sum, raw.size(), hipMemcpyDeviceToHost);
            if (e != hipSuccess) {
                sl.in_flight = false;
                c->n_flight--;
                return fail(c, PIE_E_HIP, "summary read-back: %s", hipGetErrorString(e));
            }
            Summary dev;
            memcpy(&dev, raw.data(), sizeof dev);
            dev.live = dev.amb = dev.cand = 0;
            dev.chunk_max = 0;
            for (int k = 0; k < kStatSlots; ++k) {
                StatSlot st;
                memcpy(&st, raw.data() + kSummaryBytes + (size_t)k * sizeof(StatSlot), sizeof st);
                dev.live += st.live;
                dev.amb += st.amb;
                dev.cand += st.cand;
                dev.chunk_max = st.chunk_max > dev.chunk_max ? (unsigned)st.chunk_max : dev.chunk_max;
            }
            sl.h_sum->s = dev;
        }
    }
    sl.in_flight = false;
    c->n_flight--;
    sl.last = sl.h_sum->s;
    if (sl.ordered) {
        // idx, offsets and counts are complete; what the scan saw of the table steers the next one like any other scan's
        c->last_m = (long long)sl.last.m;
        c->live_frac = c->ord.n > 0 ? (double)sl.last.live / (double)c->n : 0.0;
        c->hot_bucket = sl.last.m > 4096 && (unsigned long long)sl.last.max_count * 64ull > sl.last.m;
        if ((sl.variant & 0x400) && sl.last.amb > 4096 && sl.last.amb > (unsigned long long)c->n / 64) {
            if (c->key_dirty) c->key_rebuild = true;
            else if (sl.variant & 0x800) c->fkey_poor = true;
            else c->key_poor = true;
        }
        sl.have_result = true;
        c->res = &sl;
        c->last_was_batch = false;
        return PIE_OK;
    }
    if (sl.fast) {
        if (sl.last.pad & 1u) {
            // a partition overflowed (skewed users): everything this attempt wrote is discarded and the same query
            // reruns on the general path, here and now; the fast path stays off for this table
            c->fast_enabled = false;
            int rc = sync_all(c);
            if (rc) return rc;
            const unsigned long long mask = c->n_disc >= 64 ? c->disc_mask : (c->disc_mask & ((1ull << c->n_disc) - 1ull));
            PIE_HIP(c, hipMemsetAsync(sl.counts, 0, counts_span(c), a));
            sl.fast = false;
            sl.variant = c->k1_live_first;
            sl.ev_index = -1; // the events of the discarded attempt stay as they are (they timed real launches)
            sl.seq = ++c->seq_counter;
            launch_k1(c, sl, a, sl.q_now, sl.q_cutoff, mask);
            launch_k2(c, sl, a, (int4*)nullptr, 0LL);
            PIE_HIP(c, hipGetLastError());
            PIE_HIP(c, hipStreamSynchronize(a));
            sl.last = sl.h_sum->s;
        } else {
            // nothing left to launch: the tail ran right behind the table pass
            c->live_frac = c->n > 0 ? (double)sl.last.live / (double)c->n : 0.0;
            c->hot_bucket = sl.last.m > 4096 && (unsigned long long)sl.last.max_count * 64ull > sl.last.m;
            c->last_m = (long long)sl.last.m;
            sl.have_result = true;
            c->res = &sl;
            if (sl.last.bad_rows)
                return fail(c, PIE_E_INVAL, "%u selected rows carry a user id outside [0, %d)", sl.last.bad_rows, c->n_users);
            return PIE_OK;
        }
    }
    if ((sl.variant & 0x400) && !c->d_qual) choose_run_shift(c, sl.last.cand, sl.last.chunk_max, (sl.variant & 0x800) != 0);
    if ((sl.variant & 0x400) && sl.last.amb > 4096 && sl.last.amb > (unsigned long long)c->n / 64) {
        // the key column separated this query badly (e.g. `now` beyond the range it was built for)
        if (c->key_dirty) c->key_rebuild = true;
        else if (sl.variant & 0x800) c->fkey_poor = true;
        else c->key_poor = true;
    }
    if (!c->d_qual) {
        c->last_m = (long long)sl.last.m;
        c->live_frac = c->n > 0 ? (double)sl.last.live / (double)c->n : 0.0;
        c->hot_bucket = sl.last.m > 4096 && (unsigned long long)sl.last.max_count * 64ull > sl.last.m;
        // buckets outgrew the direct slots: ask for a capacity that holds the largest one (up to what one wave orders),
        // within the memory budget; applied at the next begin with nothing in flight
        if (sl.direct && sl.last.n_over > 0 && sl.last.max_count > (1u << c->dshift)) {
            int want = c->dshift;
            while (want < 9 && (1u << want) < sl.last.max_count) ++want;
            while (want > c->dshift && ((size_t)c->cap_users << want) * sizeof(BktRec) > kDirectMaxBytes) --want;
            if (want > c->dshift_want) c->dshift_want = want;
        }
        // streaming forms report how many selected rows sat next to (0x03) / shared an atomic with (0x43) a row of the same user
        if (sl.variant == 0x03 || sl.variant == 0x43) c->clustered = sl.last.m > 4096 && sl.last.amb * 2 > sl.last.m;
        // hot set = the users K2 reported (bucket > 1/256 of the previous M), re-read only when their number changed
        // or every 64 scans (the read waits for the stream, so it must stay rare); a stale set is still exact
        const unsigned n_hot = sl.last.n_hot < (unsigned)kHotMax ? sl.last.n_hot : (unsigned)kHotMax;
        c->hot_age++;
        if (n_hot == 0) { c->hot.n = 0; c->hot_seen = 0; }
        else if (n_hot != c->hot_seen || c->hot_age >= 64) {
            PIE_HIP(c, hipMemcpyAsync(c->hot.user, sl.hot_list, (size_t)n_hot * 4, hipMemcpyDeviceToHost, a));
            PIE_HIP(c, hipStreamSynchronize(a));
            c->hot.n = (int)n_hot;
            c->hot_seen = n_hot;
            c->hot_age = 0;
        }
    }

    // Without direct slots every record was staged: scatter, then order the tiny buckets.  With them only the buckets K2
    // counted in n_over (outgrew the slot capacity, or belong to a hot user) have staged records.
    const bool staged = sl.direct ? (sl.last.n_over > 0) : (sl.last.m > 0);
    if (sl.last.m > 0) {
        if (staged) {
            int scat_blocks = sl.k1_blocks;
            if (scat_blocks > c->n_cus * 16) scat_blocks = c->n_cus * 16;
            hipLaunchKernelGGL(k_scatter, dim3(scat_blocks), dim3(256), 0, a, sl.sel, sl.sel_rank, sl.blk_count, sl.k1_blocks,
                               sl.rows_per_block, sl.offsets, sl.bkt, sl.hot, sl.blk_hot_base);
            if (sl.direct) {
                unsigned cp_blocks = (sl.last.n_over + 3) / 4;
                if (cp_blocks > (unsigned)c->n_cus * 8) cp_blocks = (unsigned)c->n_cus * 8;
                hipLaunchKernelGGL(k_copy_direct, dim3(cp_blocks), dim3(256), 0, a, sl.over_list, sl.sum, direct_of(c, sl), sl.offsets, sl.bkt);
            }
        }
        if (!sl.direct) launch_sort_tiny(c, sl, a);
        if (sl.last.n_seg > 0) {
            const unsigned seg_blocks = sl.last.n_seg < (unsigned)(c->n_cus * 3) ? sl.last.n_seg : (unsigned)(c->n_cus * 3);
            hipLaunchKernelGGL(k_sort_segments, dim3(seg_blocks), dim3(1024), 0, a, sl.seg_list, sl.sum, sl.bkt, sl.out_idx);
        }
        if (sl.last.n_small > 0) {
            unsigned small_blocks = (sl.last.n_small + 3) / 4;
            if (small_blocks > (unsigned)c->n_cus * 8) small_blocks = (unsigned)c->n_cus * 8;
            hipLaunchKernelGGL(k_sort_small, dim3(small_blocks), dim3(256), 0, a, sl.small_list, sl.sum, sl.bkt, direct_of(c, sl), sl.out_idx);
        }
    }
    if (sl.last.n_big > 0) {
        // big buckets: tiles of kSegMax were sorted in place by K4; merge passes ping-pong between the bucket
        // arrays and scratch carved out of this slot's (now consumed) record staging; the last pass lands in out_idx.
        BktRec* tmp = reinterpret_cast<BktRec*>(sl.sel); // same 16-B records, n of them
        // up to kMergeWays-way passes (one launch merges a bucket of up to 16 tiles); every pass takes as many ways as it
        // needs to finish, at most kMergeWays
        int passes = 0;
        for (long long w = kSegMax; w < (long long)sl.last.max_count; w *= kMergeWays) ++passes;
        bool in_bkt = true; // which buffer holds the current runs
        long long w = kSegMax;
        for (int p = 0; p < passes; ++p) {
            long long need = ((long long)sl.last.max_count + w - 1) / w; // runs of the largest bucket
            const int ways = need < 2 ? 2 : (need > kMergeWays ? kMergeWays : (int)need);
            const BktRec* src = in_bkt ? sl.bkt : tmp;
            BktRec* dst = in_bkt ? tmp : sl.bkt;
            int* idx_only = (p == passes - 1) ? sl.out_idx : nullptr;
            const unsigned gx = (unsigned)((sl.last.max_count + 255u) / 256u);
            const unsigned gy = sl.last.n_big < 65535u ? sl.last.n_big : 65535u;
            hipLaunchKernelGGL(k_merge_pass, dim3(gx < 4096u ? gx : 4096u, gy), dim3(256), 0, a, sl.big_list,
                               (int)sl.last.n_big, sl.counts_ord, sl.offsets, w, ways, src, dst, idx_only);
            in_bkt = !in_bkt;
            w *= ways;
        }
    }
    PIE_HIP(c, hipGetLastError());
    // kernels were queued behind K2 (or K2 rode in a later scan's launch: the event has not been recorded at all)
    const bool more = (sl.last.m > 0 && (staged || !sl.direct || sl.last.n_seg > 0 || sl.last.n_small > 0)) || sl.last.n_big > 0;
    if (sl.ev_index >= 0 && (more || !e2_recorded)) PIE_HIP(c, hipEventRecord(c->ring[sl.ev_index].e2, a));
    sl.have_result = true;
    c->res = &sl;
    c->last_was_batch = false;
    if (sl.last.bad_rows)
        return fail(c, PIE_E_INVAL, "%u selected rows carry a user id outside [0, %d)", sl.last.bad_rows, c->n_users);
    return PIE_OK;
}

int run_scan(pie_ctx* c, long long now, long long cutoff)
{
    if (c->n_flight) return fail(c, PIE_E_STATE, "a scan is in flight: finish it first");
    int rc = scan_begin(c, now, cutoff);
    if (rc) return rc;
    return scan_finish(c);
}

// ---------------------------------------------------------------------------------------------- synchronous row lists
// The calls that walk the table once and answer with an ordered list of rows (run_row_list, delete_users_run,
// pie_expired_queue, pie_archive_queue) enter and leave through the three helpers below.

// What a call does on entry, in this order: forget the device-side queue; refuse "no table loaded"; report an empty table
// (*empty: the caller returns PIE_OK in its own way); refuse "a scan is in flight"; [kRefuseTurns] refuse a begun token turn;
// select the device; [kSyncAll] wait for every stream of the context; [kDropSlot0 / kDropSlots] give up the scan result whose
// workspace the list is about to use (drop_results).  kChecksOnly stops before the device is selected.
//
//   call                             kRefuseTurns  kSyncAll  results given up
//   run_row_list (row_list)          yes           yes       slot 0 (kDropSlot0); slot 1 later, when local rows are wanted
//   delete_users_run                 yes           yes       slot 0 (kDropSlot0)
//   pie_expired_queue                no            no        slots 0 and 1 (kDropSlots)
//   pie_expired_queue, two-pass arm  kChecksOnly, then row_list's own entry
//   pie_archive_queue                no            yes       slots 0 and 1, by itself after its allocations (drop_results)
enum ListEnter : unsigned { kChecksOnly = 0, kRefuseTurns = 1, kSyncAll = 2, kDropSlot0 = 4, kDropSlots = 8 };

// both = false: slot 0's result, and the context's current result only if it was that one; both = true: both slots', and the
// current result whichever it was
void drop_results(pie_ctx* c, bool both)
{
    c->slot[0].have_result = false;
    if (both) c->slot[1].have_result = false;
    if (both || c->res == &c->slot[0]) c->res = nullptr;
}

int list_enter(pie_ctx* c, unsigned flags, bool* empty)
{
    *empty = false;
    queue_forget(c);
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (c->n == 0) { *empty = true; return PIE_OK; }
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    if (flags == kChecksOnly) return PIE_OK;
    if ((flags & kRefuseTurns) && turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    PIE_HIP(c, hipSetDevice(c->device));
    if (flags & kSyncAll) { // the workspace is shared with the scans' tails, the staging block with appends / touches
        const int rc = sync_all(c);
        if (rc) return rc;
    }
    if (flags & (kDropSlot0 | kDropSlots)) drop_results(c, (flags & kDropSlots) != 0);
    return PIE_OK;
}

// the list's length: what the prefix kernel left in d_summary->m, behind everything queued on s
int list_total(pie_ctx* c, hipStream_t s, size_t* m)
{
    PIE_HIP(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(Summary), hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    *m = (size_t)c->h_summary->m;
    return PIE_OK;
}

// m rows of the device-side list -> out (may be NULL: nothing is copied).  A list longer than `cap` is refused here, AFTER
// the write pass: the rows are tombstoned all the same, and PIE_E_CAPACITY tells the count the caller has already stored.
int list_copy_out(pie_ctx* c, const int* dev, size_t m, int32_t* out, size_t cap, const char* what)
{
    if (out && m > cap) return fail(c, PIE_E_CAPACITY, "%s cap %zu < %zu", what, cap, m);
    if (out && m) {
        PIE_HIP(c, hipMemcpyAsync(out, dev, m * 4, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
    }
    return PIE_OK;
}

// ordered list of the rows matching a one-column predicate (expired queue / user match), through slot 0's
// workspace: blk_count + blk_off for the per-block prefix, out_idx as the device-side list
// MAPPED: the context is a shard whose row map covers its rows (the caller checked); the list holds GLOBAL rows, stored by the
// write pass itself.  want_local (MAPPED only): the local rows go beside them into slot 1's out_idx, whose result is given up.
template <ListMode MODE, bool MAPPED = false>
int run_row_list(pie_ctx* c, long long a, long long b, int32_t* out, size_t cap, size_t* k_out, bool want_local = false)
{
    if (k_out) *k_out = 0;
    bool empty;
    int rc = list_enter(c, kRefuseTurns | kSyncAll | kDropSlot0, &empty);
    if (rc || empty) return rc;
    hipStream_t s = c->stream;
    Slot& sl = c->slot[0];
    const int blocks = c->plan_blocks[0];
    const long long rpb = c->plan_rows[0];
    hipLaunchKernelGGL(k_list_count<MODE>, dim3(blocks), dim3(256), 0, s, c->d_end, c->d_user, c->d_start, c->n, rpb, a, b, sl.blk_count);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, sl.blk_count, blocks, c->d_blk_off, &c->d_summary->m);
    const int* row_map = nullptr;
    int* local_q = nullptr;
    if constexpr (MAPPED) {
        row_map = c->d_shard_rows;
        if (want_local) {
            c->slot[1].have_result = false;
            c->res = nullptr;
            local_q = c->slot[1].out_idx;
        }
    }
    hipLaunchKernelGGL((k_list_write<MODE, MAPPED>), dim3(blocks), dim3(256), 0, s, c->d_end, c->d_user, c->d_start, c->n, rpb, a, b,
                       c->d_blk_off, sl.out_idx, c->cap_rows, c->d_key, c->d_fkey, ord_mirror_of(c), hot_mirror_of(c), row_map, local_q);
    PIE_HIP(c, hipGetLastError());
    size_t k = 0;
    rc = list_total(c, s, &k);
    if (rc) return rc;
    if (k_out) *k_out = k;
    return list_copy_out(c, sl.out_idx, k, out, cap, "list"); // after the write pass: see list_copy_out
}

// The one way in: which instantiation a (mode, mapped) pair runs.  Shards answer the three maintenance lists in global rows;
// the expired queue and the one-user delete have no mapped form.
int row_list(pie_ctx* c, ListMode mode, bool mapped, long long a, long long b, int32_t* out, size_t cap, size_t* k_out, bool want_local)
{
    switch (mode) {
    case kExpired: return run_row_list<kExpired>(c, a, b, out, cap, k_out);
    case kOneUser: return run_row_list<kOneUser>(c, a, b, out, cap, k_out);
    case kPrune: return mapped ? run_row_list<kPrune, true>(c, a, b, out, cap, k_out, want_local) : run_row_list<kPrune>(c, a, b, out, cap, k_out);
    case kRetention: return mapped ? run_row_list<kRetention, true>(c, a, b, out, cap, k_out, want_local) : run_row_list<kRetention>(c, a, b, out, cap, k_out);
    case kRetentionTz: return mapped ? run_row_list<kRetentionTz, true>(c, a, b, out, cap, k_out, want_local) : run_row_list<kRetentionTz>(c, a, b, out, cap, k_out);
    }
    return fail(c, PIE_E_INVAL, "unknown list mode %d", (int)mode);
}


// ---------------------------------------------------------------------------------------------- batched scans
// Q <= 64 queries in one table pass (pie_kernels.h "batched scan").  The pass and its tail produce the UNION of the selections
// (per user the rows any query selected, ordered, with a query mask per row): that is the batch's result.  Per-query counts /
// offsets / row lists live in list storage that is allocated and filled only when somebody asks for them
// (pie_batch_read_results, per-query messages) or when a path produces them anyway (fallback scans, the ordered run).

long long batch_users_stride(const pie_ctx* c) { return (((long long)c->cap_users + 1 + 31) / 32) * 32; }
long long batch_out_stride(const pie_ctx* c) { return (long long)c->cap_users * kTinyMax; }
size_t batch_mq_bytes() { return (size_t)kMqSlots * kBatchMax * 4; }
size_t batch_span_bytes(const pie_ctx* c) { return counts_span(c) + batch_mq_bytes(); }

bool batch_supported(const pie_ctx* c)
{
    const int tiles = (c->n_users + kK1Threads - 1) / kK1Threads;
    return c->key_ok && c->d_key && c->d_fkey && c->d_pay && c->slot[0].direct != nullptr && tiles <= kOrderMaxTiles && c->n > 0 &&
           (long long)c->cap_users * kTinyMax < (1LL << 31);
}

// the arrays of the batched pass: union bucket slots + the union result per batch slot, three rotating spans
// entries of the union result arrays: the bucket slots of the general pass, or a sixteenth of the rows (a batch on the ordered
// run has no slot bound: a head user's union is as long as its live rows)
size_t batch_ucap(const pie_ctx* c)
{
    const size_t slots = (size_t)c->cap_users << c->bdshift, rows16 = (size_t)c->cap_rows / 16 + 4096;
    return slots > rows16 ? slots : rows16;
}

bool any_lane_alloc(const pie_ctx* c)
{
    for (bool a : c->lane_alloc)
        if (a) return true;
    return false;
}

hipStream_t lane_stream_of(const pie_ctx* c, int lane) { return lane == 0 ? c->stream : c->lane_stream[lane]; }

// the slot arrays and spans of one lane (and, for lanes above 0, its stream)
int ensure_batch(pie_ctx* c, int lane)
{
    if (c->lane_alloc[lane]) return PIE_OK;
    if (lane > 0 && !c->lane_stream[lane]) PIE_HIP(c, hipStreamCreateWithFlags(&c->lane_stream[lane], hipStreamNonBlocking));
    for (hipEvent_t& e : c->lane_event[lane])
        if (!e) PIE_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const size_t slots = (size_t)c->cap_users << c->bdshift;
    const size_t ucap = batch_ucap(c);
    for (int i = 0; i < kBatchSlots; ++i) {
        BatchSlot& b = c->bslot[lane * kBatchSlots + i];
        PIE_HIP(c, hipMalloc(&b.direct, slots * sizeof(BktRec)));
        PIE_HIP(c, hipMalloc(&b.mtab, kMaskTabWords * 8));
        PIE_HIP(c, hipMalloc(&b.uoff, ((size_t)c->cap_users + 2) * 8));
        PIE_HIP(c, hipMalloc(&b.urows, ucap * 4));
        PIE_HIP(c, hipMalloc(&b.umlo, ucap * 4));
        PIE_HIP(c, hipMalloc(&b.umhi, ucap * 4));
    }
    for (int i = 0; i < 3; ++i) {
        char*& sp = c->bspan[lane * 3 + i];
        PIE_HIP(c, hipMalloc(&sp, batch_span_bytes(c)));
        PIE_HIP(c, hipMemsetAsync(sp, 0, batch_span_bytes(c), lane_stream_of(c, lane)));
    }
    c->lane_span_next[lane] = 0;
    c->lane_alloc[lane] = true;
    return PIE_OK;
}

// per-query list storage of a batch slot for at least n_q queries (16 / 32 / 64); growing it drops what it held, so it is
// sized before anything of the batch is written to it
int ensure_lists(pie_ctx* c, BatchSlot& b, int n_q)
{
    const int want = n_q <= 16 ? 16 : n_q <= 32 ? 32 : kBatchMax;
    if (b.lists_q >= want) return PIE_OK;
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    dfree(b.counts_ord); dfree(b.offsets); dfree(b.out_idx);
    b.lists_q = 0;
    for (int q = 0; q < kBatchMax; ++q) b.list_ok[q] = false;
    const size_t us = (size_t)batch_users_stride(c), os = (size_t)batch_out_stride(c);
    PIE_HIP(c, hipMalloc(&b.counts_ord, (size_t)want * us * 4));
    PIE_HIP(c, hipMalloc(&b.offsets, (size_t)want * us * 8));
    PIE_HIP(c, hipMalloc(&b.out_idx, (size_t)want * (os > 0 ? os : 1) * 4));
    b.lists_q = want;
    return PIE_OK;
}

// batches finish in the order they were begun, whatever lane they ran on
BatchSlot* oldest_batch(pie_ctx* c)
{
    if (c->b_flight == 0) return nullptr;
    const int lane = c->fifo[c->fifo_head];
    return &c->bslot[lane * kBatchSlots + (c->lane_next[lane] + kBatchSlots - c->lane_flight[lane]) % kBatchSlots];
}

// bookkeeping of a batch that has been begun on `lane` in slot lane_next[lane]
void batch_begun(pie_ctx* c, int lane)
{
    c->fifo[(c->fifo_head + c->b_flight) % (kLaneMax * kBatchSlots)] = (unsigned char)lane;
    c->b_flight++;
    c->lane_flight[lane]++;
    c->lane_next[lane] = (c->lane_next[lane] + 1) % kBatchSlots;
}

// ... and of the oldest batch leaving the flight
void batch_left(pie_ctx* c, BatchSlot& b)
{
    b.in_flight = false;
    c->fifo_head = (c->fifo_head + 1) % (kLaneMax * kBatchSlots);
    c->b_flight--;
    c->lane_flight[b.lane]--;
    if (c->b_flight == 0) c->idle_epoch++;
}

// Work about to be queued on the context's MAIN stream reads what batch b's kernels wrote on a lane's stream.  The host has
// seen b's summary, but the launch that carried b's tail (the next table pass of that lane rides in it) may still be running,
// and plain stores sit in the XCDs' L2s until a kernel ends: the main stream waits for what the lane has queued so far.
int order_after_batch(pie_ctx* c, BatchSlot& b)
{
    if (b.main_ordered || b.stream == c->stream || !b.stream) { b.main_ordered = true; return PIE_OK; }
    if (!c->lane_event[b.lane][1]) PIE_HIP(c, hipEventCreateWithFlags(&c->lane_event[b.lane][1], hipEventDisableTiming));
    PIE_HIP(c, hipEventRecord(c->lane_event[b.lane][1], b.stream));
    PIE_HIP(c, hipStreamWaitEvent(c->stream, c->lane_event[b.lane][1], 0));
    b.main_ordered = true;
    return PIE_OK;
}

void fill_tail_args(pie_ctx* c, BatchSlot& b, UnionTailArgs& t)
{
    t.n_q = b.n_q;
    t.n_users = c->n_users;
    t.tiles = (c->n_users + kK1Threads - 1) / kK1Threads;
    t.dshift = b.dshift;
    t.span = b.span;
    t.tiles_off = (long long)span_counts_bytes(c);
    t.ctl_off = (long long)(span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes());
    t.summary_off = t.ctl_off + 128;
    t.mq_off = (long long)counts_span(c);
    t.zero_span = b.zero_span;   // the next-but-one batch's span
    t.zero_total16 = (long long)(batch_span_bytes(c) / 16);
    t.direct = b.direct;
    t.mtab = b.mtab;
    t.uoff = b.uoff; t.urows = b.urows; t.umlo = b.umlo; t.umhi = b.umhi;
    t.host = b.bh_dev;
    t.seq = b.seq;
    t.msg = b.msg_kind == 2 ? b.msg : nullptr;
    t.u_pad = b.msg_u_pad;
    t.msg_cap = b.msg_cap;
}

// the predicate tables of a batch (pie_kernels.h BatchTables) over the queries that take part in the pass
void fill_batch_tables(const pie_ctx* c, const BatchSlot& b, const pie_query* qs, const unsigned* nk, BatchTables& t)
{
    fill_batch_tables(c->n_disc, b.n_q, b.fallback, qs, nk, t);
}

// ... of n_q queries, those marked in fallback[] left out, over a table of n_disc disciplines
void fill_batch_tables(int n_disc, int n_q, const bool* fallback, const pie_query* qs, const unsigned* nk, BatchTables& t)
{
    int by_now[kBatchMax], by_cut[kBatchMax], nb = 0;
    for (int q = 0; q < n_q; ++q)
        if (!fallback[q]) { by_now[nb] = q; by_cut[nb] = q; ++nb; }
    std::stable_sort(by_now, by_now + nb, [&](int x, int y) { return qs[x].now < qs[y].now; });
    std::stable_sort(by_cut, by_cut + nb, [&](int x, int y) { return qs[x].cutoff < qs[y].cutoff; });
    unsigned long long lv = 0, wn = 0;
    t.live[0] = 0;
    t.win[0] = 0;
    for (int i = 0; i < kBatchMax; ++i) {
        if (i < nb) {
            t.now[i] = qs[by_now[i]].now;
            t.nk[i] = nk[by_now[i]];
            t.cutoff[i] = qs[by_cut[i]].cutoff;
            lv |= 1ull << by_now[i];
            wn |= 1ull << by_cut[i];
        } else {
            t.now[i] = INT64_MAX;
            t.nk[i] = ~0u;
            t.cutoff[i] = INT64_MAX;
        }
        t.live[i + 1] = lv;
        t.win[i + 1] = wn;
    }
    for (int d = 0; d < 64; ++d) t.disc[d] = 0;
    const unsigned long long table = n_disc >= 64 ? ~0ull : ((1ull << n_disc) - 1ull);
    for (int i = 0; i < nb; ++i) { // every set bit of every query's mask, once
        const int q = by_now[i];
        for (unsigned long long m = qs[q].mask & table; m; m &= m - 1) t.disc[__builtin_ctzll(m)] |= 1ull << q;
    }
}

void launch_batch_k2(pie_ctx* c, BatchSlot& b, hipStream_t s)
{
    UnionTailArgs t;
    fill_tail_args(c, b, t);
    if (t.n_q > 32) hipLaunchKernelGGL(k_union_tail<true>, dim3((unsigned)t.tiles), dim3(kK1Threads), 0, s, t);
    else hipLaunchKernelGGL(k_union_tail<false>, dim3((unsigned)t.tiles), dim3(kK1Threads), 0, s, t);
    b.k2_pending = false;
}

// ---- admission of a batch to a lane's slot, the steps batch_begin and wide_begin share; the callers put them in order

// A table is loaded, the batch holds 1..max_q queries (`what` names the caller's kind of batch) and no single scan is in
// flight; then the keys are rebuilt if that is due.
int begin_checks(pie_ctx* c, const pie_query* qs, int n_q, int max_q, const char* what)
{
    queue_forget(c); // the ordered run's union stages in the slots' workspace
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (!qs || n_q < 1 || n_q > max_q) return fail(c, PIE_E_INVAL, "%s holds 1..%d queries (got %d)", what, max_q, n_q);
    if (c->n_flight) return fail(c, PIE_E_STATE, "a single scan is in flight: finish it before beginning a batch");
    if (c->key_rebuild && c->b_flight == 0) return build_keys(c, 0, true);
    return PIE_OK;
}

// Dense queries (the key histogram bounds their live rows above a tenth of the table) do not belong in a batch: they would
// make every row a candidate for all queries; they run on the general path.  Marks them in dense[n_q] and says in *fine
// whether the pass can read the 1-byte key.  False when nothing is left to batch (every query is dense): then there is no
// table pass at all — a pass whose smallest key is the impossible one would still make nearly every row a candidate.
bool classify_queries(const pie_ctx* c, const pie_query* qs, int n_q, unsigned char* dense, bool* fine)
{
    const bool hist_ok = !c->key_dirty && c->key_hist_rows == c->n;
    int n_batched = 0;
    *fine = (c->k1_keyed & 0x800) && !c->fkey_poor;
    for (int q = 0; q < n_q; ++q) {
        dense[q] = hist_ok && (double)rows_keyed_at_or_above(c, qs[q].now) >= kLiveFirstBelow * (double)c->n;
        if (!dense[q]) {
            ++n_batched;
            if (qs[q].now < c->fkey_base) *fine = false;
        }
    }
    return n_batched > 0;
}

// Batches are dealt round robin over `lanes` lanes: the first one from lane_rr on with a free slot.  Nothing moves when all are full.
int pick_lane(pie_ctx* c, int lanes, int* lane_out)
{
    int lane = lanes > 1 ? c->lane_rr % lanes : 0, tried = 0;
    while (tried < lanes && c->lane_flight[lane] >= kBatchSlots) { lane = (lane + 1) % lanes; ++tried; }
    if (tried == lanes)
        return fail(c, PIE_E_STATE, "%d batches are already in flight (%d per lane, %d lane%s): finish one first", c->b_flight, kBatchSlots, lanes,
                    lanes > 1 ? "s" : "");
    if (lanes > 1) c->lane_rr = (lane + 1) % lanes;
    *lane_out = lane;
    return PIE_OK;
}

// Larger union buckets for every user (a finished batch found one that outgrew its slots), taken once no batch is in flight:
// every slot's arrays are replaced; their contents are per-batch scratch.
int regrow_union_buckets(pie_ctx* c)
{
    if (c->bdshift_want <= c->bdshift || c->b_flight != 0 || !any_lane_alloc(c)) return PIE_OK;
    int rc = sync_all(c);
    if (rc) return rc;
    const size_t slots = (size_t)c->cap_users << c->bdshift_want;
    if (slots * sizeof(BktRec) <= kDirectMaxBytes) {
        c->bdshift = c->bdshift_want;
        for (BatchSlot& x : c->bslot) {
            dfree(x.direct); dfree(x.mtab); dfree(x.uoff); dfree(x.urows); dfree(x.umlo); dfree(x.umhi);
            x.have_result = false;
        }
        for (char*& sp : c->bspan) dfree(sp);
        c->bres = nullptr;
        for (bool& a : c->lane_alloc) a = false;
    } else {
        c->bdshift_want = c->bdshift;
    }
    return PIE_OK;
}

// the slot the lane's next batch takes (back = 0), or the one of the batch begun `back` batches before it
BatchSlot& lane_slot(pie_ctx* c, int lane, int back = 0)
{
    return c->bslot[lane * kBatchSlots + (c->lane_next[lane] + kBatchSlots - back) % kBatchSlots];
}

// The slot is claimed for a batch of n_q queries: what an earlier batch left in it is dropped, the message request and the
// lane's stream are noted.  msg_kind as BatchSlot::msg_kind, 0 without a message.
void claim_slot(pie_ctx* c, BatchSlot& b, int lane, int n_q, bool unsupported, int msg_kind, int* msg, long long msg_stride, int u_pad,
                long long msg_cap, int* msg_counts, long long msg_counts_stride)
{
    b.lane = lane;
    b.n_q = n_q;
    b.have_result = false;
    b.union_ok = b.union_part = false;
    b.mu = 0;
    if (c->bres == &b) c->bres = nullptr;
    b.msg_kind = msg ? msg_kind : 0;
    b.msg = msg; b.msg_stride = msg_stride; b.msg_u_pad = u_pad; b.msg_cap = msg_cap;
    b.msg_counts = msg_counts; b.msg_counts_stride = msg_counts_stride;
    b.ev_index = -1;
    b.ordered = false;
    b.unsupported = unsupported;
    b.stream = lane_stream_of(c, lane);
    b.main_ordered = lane == 0;
}

// a batch none of whose queries takes a pass is in flight with nothing on the lane's stream: finish runs every query on the
// general path
void begin_fallback_only(pie_ctx* c, BatchSlot& b)
{
    b.in_flight = true;
    b.k2_pending = false;
    b.main_ordered = true;
    batch_begun(c, b.lane);
}

// a lane above 0 that has queued nothing since the context was last idle goes behind the main stream (see idle_epoch)
int order_lane_after_main(pie_ctx* c, int lane)
{
    if (lane == 0 || c->lane_epoch[lane] == c->idle_epoch) return PIE_OK;
    PIE_HIP(c, hipEventRecord(c->lane_event[lane][0], c->stream));
    PIE_HIP(c, hipStreamWaitEvent(lane_stream_of(c, lane), c->lane_event[lane][0], 0));
    c->lane_epoch[lane] = c->idle_epoch;
    return PIE_OK;
}

// a lane above 0 whose stream has not yet waited for the last turn begun in flight (turn_fence_leave) does so before its next
// launch: that launch reads the table the turn left
int lane_after_mutation(pie_ctx* c, int lane)
{
    if (lane == 0 || c->lane_mut_epoch[lane] == c->mut_epoch) return PIE_OK;
    PIE_HIP(c, hipStreamWaitEvent(lane_stream_of(c, lane), c->mut_event, 0));
    c->lane_mut_epoch[lane] = c->mut_epoch;
    return PIE_OK;
}

// spans (the lane's own three, in rotation): this batch's, and the one it zeroes for the batch after the next
void take_spans(pie_ctx* c, BatchSlot& b)
{
    char** const lane_spans = c->bspan + b.lane * 3;
    b.span = lane_spans[c->lane_span_next[b.lane]];
    c->lane_span_next[b.lane] = (c->lane_span_next[b.lane] + 1) % 3;
    b.zero_span = lane_spans[(c->lane_span_next[b.lane] + 1) % 3];
}

// the batch begun just before the next one on this lane, if its union tail still waits for a launch (tails run in the order of
// their batches); null otherwise
BatchSlot* waiting_tail(pie_ctx* c, int lane)
{
    BatchSlot& prev = lane_slot(c, lane, 1);
    return c->lane_flight[lane] >= 1 && prev.in_flight && prev.k2_pending && !prev.ordered ? &prev : nullptr;
}

int batch_begin(pie_ctx* c, const pie_query* qs, int n_q, int msg_kind, int* msg, long long msg_stride, int u_pad, long long msg_cap,
                int* msg_counts, long long msg_counts_stride)
{
    PIE_PROF_START();
    int rc = begin_checks(c, qs, n_q, kBatchMax, "a batch");
    if (rc) return rc;
    const bool ord_batch = batch_supported(c) && ordered_batch_wanted(c) && !c->ord_lists_only;
    bool unsupported = !ord_batch && (!batch_supported(c) || c->key_poor || c->batch_poor);
    unsigned char dense_q[kBatchMax];
    bool fine = false;
    if (!unsupported && !classify_queries(c, qs, n_q, dense_q, &fine)) unsupported = true;
    // a batch on the ordered run (its staging is the scan slots') stays on lane 0 (one that only falls back queues nothing here:
    // any lane's slot will do)
    int lane = 0;
    rc = pick_lane(c, ord_batch ? 1 : c->n_lanes, &lane);
    if (rc) return rc;
    BatchSlot& b = lane_slot(c, lane);
    claim_slot(c, b, lane, n_q, unsupported, msg_kind, msg, msg_stride, u_pad, msg_cap, msg_counts, msg_counts_stride);
    b.wide = false;
    for (int q = 0; q < n_q; ++q) { b.q[q] = qs[q]; b.fallback[q] = unsupported || dense_q[q]; b.idx_of[q] = nullptr; b.list_ok[q] = false; }
    hipStream_t s = b.stream;
    PIE_PROF_TICK(0);
    if (unsupported) {
        begin_fallback_only(c, b);
        return PIE_OK;
    }
    rc = regrow_union_buckets(c);
    if (rc) return rc;
    rc = ord_batch ? PIE_OK : ensure_batch(c, lane);
    if (rc) return rc;
    // the 1-byte pass reads the hot index instead of the key column; built here, on the main stream, the first time it can be
    if (fine && !ord_batch && c->hix.enabled && !c->hix.valid && c->b_flight == 0) {
        rc = hot_build(c);
        if (rc) return rc;
    }
    rc = order_lane_after_main(c, lane);
    if (rc) return rc;
    rc = lane_after_mutation(c, lane);
    if (rc) return rc;
    b.fine_key = fine;
    b.hot = fine && !ord_batch && c->hix.valid;
    b.dshift = c->bdshift;
    if (c->profiling && (c->scans_begun % (unsigned long long)c->profile_every) == 0) {
        if (c->ring_used == kEventRing) {
            rc = resolve_events(c);
            if (rc) return rc;
        }
        if (c->ring_used < kEventRing) {
            if ((int)c->ring.size() <= c->ring_used) {
                ScanEvents e{};
                PIE_HIP(c, hipEventCreate(&e.e0));
                PIE_HIP(c, hipEventCreate(&e.e1));
                PIE_HIP(c, hipEventCreate(&e.e2));
                c->ring.push_back(e);
            }
            b.ev_index = c->ring_used++;
        }
    }
    BatchSlot* const other = waiting_tail(c, lane);
    if (ord_batch) {
        // the table's batches do not fit the general pass (skewed users): ONE pass over the run's key column for the batch (pie_ordered.h, the batched union form)
        rc = ord_batch_alloc(c);
        if (rc) return rc;
        rc = ensure_batch(c, 0);
        if (rc) return rc;
        if (other) launch_batch_k2(c, *other, s); // nothing carries it along
        b.seq = ++c->bseq_counter;
        c->scans_begun++;
        if (b.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[b.ev_index].e0, s));
        launch_ordered_union(c, b, s, qs, fine);
        PIE_HIP(c, hipGetLastError());
        b.ordered = true;
        b.k2_pending = false;
        b.in_flight = true;
        batch_begun(c, lane);
        return PIE_OK;
    }
    take_spans(c, b);
    b.seq = ++c->bseq_counter;
    const int plan = fine ? 3 : 2;
    b.k1_blocks = c->plan_blocks[plan];
    c->scans_begun++;
    const bool ride = other && !c->no_ride;
    if (other && !ride) launch_batch_k2(c, *other, s);
    if (b.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[b.ev_index].e0, s));
    PIE_PROF_TICK(1);
#define PIE_BATCH_RIDE(KT, HI)                                                                                          \
    hipLaunchKernelGGL((k_scan_batch_with_tail<8, true, KT, HI>), dim3((unsigned)(b.k1_blocks + t.tiles)), dim3(kK1Threads), 0, s, a, t)
#define PIE_BATCH(KT, KEYPTR, KEYFN, IMPOSSIBLE)                                                                         \
    do {                                                                                                                \
        BatchScanArgs<KT> a;                                                                                            \
        a.pay = c->d_pay; a.end = c->d_end; a.key = KEYPTR; a.n = c->n; a.rows_per_block = c->plan_rows[plan];          \
        a.n_users = c->n_users; a.n_q = n_q; a.dshift = c->bdshift;                                                     \
        a.counts = reinterpret_cast<int*>(b.span);                                                                      \
        a.summary = reinterpret_cast<Summary*>(b.span + span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes() + 128); \
        a.direct = b.direct; a.mtab = b.mtab; a.run_shift = c->run_shift;                                               \
        unsigned nk[kBatchMax];                                                                                         \
        unsigned mk = IMPOSSIBLE;                                                                                       \
        for (int q = 0; q < n_q; ++q) {                                                                                 \
            nk[q] = KEYFN(c, qs[q].now);                                                                                \
            if (!b.fallback[q] && nk[q] < mk) mk = nk[q];                                                               \
        }                                                                                                               \
        a.min_key = mk;                                                                                                 \
        a.hot = nullptr; a.hot_lo = a.hot_main = 0; a.hot_delta_n = nullptr; a.hot_delta_cap = 0;                       \
        if (b.hot && mk >= 1 && mk <= kFineKeyMax) { /* the suffix of bin mk and the delta, a wave per 2 x 64 records */ \
            a.hot = c->hix.rec; a.hot_lo = c->hix.off[mk]; a.hot_main = c->hix.n_main;                                  \
            a.hot_delta_n = c->hix.delta_n; a.hot_delta_cap = (unsigned)c->hix.delta_cap;                               \
            const long long recs = a.hot_main - a.hot_lo + c->hix.delta_bound;                                          \
            const long long per = (long long)c->hix.recs_per_thread * kK1Threads;                                      \
            const long long want = (recs + per - 1) / per;                                                              \
            b.k1_blocks = (int)(want < 1 ? 1 : want < b.k1_blocks ? want : b.k1_blocks);                                \
        }                                                                                                               \
        fill_batch_tables(c, b, qs, nk, a.tab);                                                                         \
        PIE_PROF_TICK(2);                                                                                               \
        if (ride) {                                                                                                     \
            UnionTailArgs t;                                                                                            \
            fill_tail_args(c, *other, t);                                                                               \
            if (t.n_q > 32) PIE_BATCH_RIDE(KT, true);                                                                   \
            else PIE_BATCH_RIDE(KT, false);                                                                             \
            other->k2_pending = false;                                                                                  \
        } else {                                                                                                        \
            hipLaunchKernelGGL((k_scan_batch<8, true, KT>), dim3((unsigned)b.k1_blocks), dim3(kK1Threads), 0, s, a);    \
        }                                                                                                               \
    } while (0)
    // a query that falls back is not in the tables: it selects nothing here
    if (fine) PIE_BATCH(fkey_t, c->d_fkey, host_fine_key_of, 0xFFu);
    else PIE_BATCH(lkey_t, c->d_key, host_key_of, 0xFFFFu);
#undef PIE_BATCH
#undef PIE_BATCH_RIDE
    PIE_PROF_TICK(3);
    PIE_HIP(c, hipGetLastError());
    if (b.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[b.ev_index].e1, s));
    b.k2_pending = true;
    b.in_flight = true;
    batch_begun(c, lane);
    PIE_PROF_TICK(4);
    return PIE_OK;
}

// where query q's row list of `m` rows lives in the list storage: its strided region, or a buffer of its own when it is longer
int batch_list_dst(pie_ctx* c, BatchSlot& b, int q, long long m, int** dst_out)
{
    int* dst = b.out_idx ? b.out_idx + (long long)q * batch_out_stride(c) : nullptr;
    if (!dst || m > batch_out_stride(c)) {
        if (b.over_cap[q] < m || !b.over_idx[q]) {
            PIE_HIP(c, hipStreamSynchronize(c->stream)); // an earlier copy may still be reading the old buffer's neighbours: keep it simple
            dfree(b.over_idx[q]);
            b.over_cap[q] = 0;
            PIE_HIP(c, hipMalloc(&b.over_idx[q], (size_t)(m > 0 ? m : 1) * 4));
            b.over_cap[q] = m > 0 ? m : 1;
        }
        dst = b.over_idx[q];
    }
    *dst_out = dst;
    return PIE_OK;
}

// per-query message [off[0..u_pad] | M | rows] of a query whose lists are in the list storage
void batch_pack_list_msg(pie_ctx* c, BatchSlot& b, int q)
{
    const long long m = (long long)b.last[q].m;
    const long long total = (long long)b.msg_u_pad + 2 + (m < b.msg_cap ? m : b.msg_cap);
    unsigned blocks = (unsigned)((total + 255) / 256);
    if (blocks > (unsigned)c->n_cus * 8) blocks = (unsigned)c->n_cus * 8;
    hipLaunchKernelGGL(k_pack_lists, dim3(blocks ? blocks : 1u), dim3(256), 0, c->stream, b.offsets + (long long)q * batch_users_stride(c), c->n_users,
                       b.msg_u_pad, m, b.idx_of[q], b.msg_cap, b.msg + (long long)q * b.msg_stride);
}

// Queries of a batch on the general path, two scans in flight (the offsets kernel of one rides in the next one's table
// pass); every result is copied into the batch's list storage in stream order, one wait at the end.
int batch_fallback_copy(pie_ctx* c, BatchSlot& b, int q)
{
    Slot& sl = *c->res;
    hipStream_t s = c->stream;
    const long long us = batch_users_stride(c);
    PIE_HIP(c, hipMemcpyAsync(b.counts_ord + (long long)q * us, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDeviceToDevice, s));
    PIE_HIP(c, hipMemcpyAsync(b.offsets + (long long)q * us, sl.offsets, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToDevice, s));
    const long long m = (long long)sl.last.m;
    int* dst = nullptr;
    int rc = batch_list_dst(c, b, q, m, &dst);
    if (rc) return rc;
    if (m) PIE_HIP(c, hipMemcpyAsync(dst, sl.out_idx, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
    b.idx_of[q] = dst;
    b.list_ok[q] = true;
    if (b.msg_kind == 1) {
        rc = pie_pack_results_device(c, b.msg + (long long)q * b.msg_stride, (size_t)b.msg_u_pad, (size_t)b.msg_cap);
        if (rc) return rc;
    }
    if (b.msg_counts)
        PIE_HIP(c, hipMemcpyAsync(b.msg_counts + (long long)q * b.msg_counts_stride, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDefault, s));
    b.last[q] = sl.last;
    return PIE_OK;
}

int batch_fallback_many(pie_ctx* c, BatchSlot& b, const int* list, int n_list)
{
    if (n_list == 0) return PIE_OK;
    const unsigned long long keep_mask = c->disc_mask;
    auto begin = [&](int q) {
        c->disc_mask = b.q[q].mask;
        return scan_begin(c, b.q[q].now, b.q[q].cutoff);
    };
    int rc = begin(list[0]);
    for (int i = 0; i < n_list && rc == PIE_OK; ++i) {
        if (i + 1 < n_list) rc = begin(list[i + 1]);
        if (rc == PIE_OK) rc = scan_finish(c);
        if (rc == PIE_OK) rc = batch_fallback_copy(c, b, list[i]);
    }
    c->disc_mask = keep_mask;
    if (rc != PIE_OK) { // leave no scan in flight behind an error
        while (c->n_flight) (void)scan_finish(c);
        return rc;
    }
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    for (Slot& sl : c->slot) sl.have_result = false; // implementation details of the batch, not feed results of their own
    c->res = nullptr;
    return PIE_OK;
}

// counts / offsets / row lists of the listed queries out of the batch's union (k_mat_*); returns with the lists complete in
// stream order and, for sync = true, the per-query maxima read back
int batch_materialize(pie_ctx* c, BatchSlot& b, const int* list, int n_list)
{
    if (n_list == 0) return PIE_OK;
    if (!b.union_part) return fail(c, PIE_E_STATE, "the batch has no union to take query lists from");
    int rc = ensure_lists(c, b, b.n_q);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const int tiles = (c->n_users + 255) / 256;
    if (c->mat_tiles < tiles || !c->d_mat_tile) {
        PIE_HIP(c, hipStreamSynchronize(s));
        dfree(c->d_mat_tile); dfree(c->d_mat_qmax);
        const int cap_tiles = (c->cap_users + 255) / 256 + 1;
        PIE_HIP(c, hipMalloc(&c->d_mat_tile, (size_t)kBatchMax * ((size_t)cap_tiles + 1) * 8));
        PIE_HIP(c, hipMalloc(&c->d_mat_qmax, (size_t)kBatchMax * 4));
        c->mat_tiles = cap_tiles;
    }
    MatArgs a;
    a.n_users = c->n_users; a.tiles = tiles; a.n_list = n_list;
    a.uoff = b.uoff; a.urows = b.urows; a.umlo = b.umlo; a.umhi = b.n_q > 32 ? b.umhi : nullptr;
    a.counts = b.counts_ord; a.offsets = b.offsets; a.users_stride = batch_users_stride(c);
    a.tile_sum = c->d_mat_tile; a.qmax = c->d_mat_qmax;
    for (int i = 0; i < n_list; ++i) {
        const int q = list[i];
        int* dst = nullptr;
        rc = batch_list_dst(c, b, q, (long long)b.last[q].m, &dst);
        if (rc) return rc;
        a.q_of[i] = (unsigned char)q;
        a.out[i] = dst;
        a.out_cap[i] = (long long)b.last[q].m;
        b.idx_of[q] = dst;
    }
    PIE_HIP(c, hipMemsetAsync(c->d_mat_qmax, 0, (size_t)kBatchMax * 4, s));
    hipLaunchKernelGGL(k_mat_count, dim3((unsigned)tiles, (unsigned)n_list), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_mat_prefix, dim3((unsigned)n_list), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_mat_write, dim3((unsigned)tiles, (unsigned)n_list), dim3(256), 0, s, a);
    PIE_HIP(c, hipGetLastError());
    unsigned int qmax[kBatchMax];
    PIE_HIP(c, hipMemcpyAsync(qmax, c->d_mat_qmax, (size_t)n_list * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < n_list; ++i) {
        b.last[list[i]].max_count = qmax[i];
        b.list_ok[list[i]] = true;
    }
    return PIE_OK;
}

// the lists of query qi of a finished batch, materialised if need be
int batch_need_list(pie_ctx* c, BatchSlot& b, int qi)
{
    if (b.list_ok[qi]) return PIE_OK;
    return batch_materialize(c, b, &qi, 1);
}

int batch_pack_union(pie_ctx* c, BatchSlot& b, void* dst_i32, size_t u_pad, size_t cap);

int batch_finish(pie_ctx* c, int* ready_out)
{
    if (ready_out) *ready_out = 0;
    BatchSlot* bp = oldest_batch(c);
    if (!bp) return fail(c, PIE_E_STATE, "pie_scan_batch_finish without pie_scan_batch_begin");
    if (bp->wide) return fail(c, PIE_E_STATE, "the oldest batch in flight is wide: finish it with pie_scan_wide_finish");
    BatchSlot& b = *bp;
    hipStream_t s = b.stream ? b.stream : c->stream; // the lane the batch runs on
    bool all_ready = true;
    PIE_PROF_START();
    if (!b.unsupported) {
        if (b.k2_pending) {
            launch_batch_k2(c, b, s);
            PIE_HIP(c, hipGetLastError());
        }
        PIE_PROF_TICK(5);
        // wait for the batch's summary (mapped host memory, seq last); bounded like the single-scan wait
        const WaitResult w = word_wait(c, &b.bh->seq, b.seq, [&] { return hipStreamQuery(s); }, 1000.0, kPaceSummary);
        if (w.end != WaitEnd::Ready) {
            batch_left(c, b);
            if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "batched scan failed: %s", hipGetErrorString((hipError_t)w.err));
            return fail(c, PIE_E_HIP, "batch summary not published within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", w.waited_ms);
        }
        PIE_PROF_TICK(6);
        bool overflow = false;
        {
            const Summary us = b.bh->s;
            b.mu = us.m;
            // a union bucket outgrew its slots (the general pass) / the union its arrays (the ordered run): rows were dropped, and
            // nothing says which queries they belonged to, so every query of the batch is rerun on the general path
            overflow = us.n_over > 0 || us.bad_rows > 0;
            for (int q = 0; q < b.n_q; ++q) {
                b.last[q] = us;                       // cand, chunk_max, bad_rows, n_over: the pass's; max_count: the union's
                b.last[q].m = b.bh->mq[q];
                if (overflow) b.fallback[q] = true;
            }
            if (us.n_over > 0 && b.ordered) c->ord_lists_only = true; // the union outgrew its arrays on the run: its batches run as single scans from now on
            else if (us.n_over > 0) {
                if (c->bdshift < kUnionShiftMax) c->bdshift_want = c->bdshift + 1;
                else c->batch_poor = true; // a user's rows do not fit 64 slots: this table's batches go straight to the general path
            }
            b.union_part = !overflow;
            b.union_ok = !overflow;
            for (int q = 0; q < b.n_q; ++q) b.union_ok = b.union_ok && !b.fallback[q];
            if (!b.ordered && !b.hot) choose_run_shift(c, us.cand, us.chunk_max, b.fine_key);
        }
        if (b.ev_index >= 0) PIE_HIP(c, hipEventRecord(c->ring[b.ev_index].e2, s));
    }
    batch_left(c, b);
    {
        int list[kBatchMax], n_list = 0;
        for (int q = 0; q < b.n_q; ++q)
            if (b.fallback[q]) list[n_list++] = q;
        if (n_list) {
            all_ready = false;
            int rc = order_after_batch(c, b); // what follows runs on the main stream
            if (rc) return rc;
            rc = ensure_lists(c, b, b.n_q);
            if (rc) return rc;
            rc = batch_fallback_many(c, b, list, n_list);
            if (rc) return rc;
        }
    }
    b.have_result = true;
    c->bres = &b;
    c->last_was_batch = true;
    for (int q = 0; q < b.n_q; ++q)
        if (b.last[q].bad_rows) return fail(c, PIE_E_INVAL, "query %d: %u selected rows carry a user id outside [0, %d)", q, b.last[q].bad_rows, c->n_users);
    if (b.msg_kind == 1 || b.msg_counts) {
        // per-query messages of a batch on the general pass: the lists are materialised from the union, then packed
        all_ready = false;
        int list[kBatchMax], n_list = 0;
        for (int q = 0; q < b.n_q; ++q)
            if (!b.list_ok[q]) list[n_list++] = q;
        int rc = order_after_batch(c, b);
        if (rc) return rc;
        rc = batch_materialize(c, b, list, n_list);
        if (rc) return rc;
        for (int i = 0; i < n_list; ++i) {
            const int q = list[i];
            if (b.msg_kind == 1) batch_pack_list_msg(c, b, q);
            if (b.msg_counts)
                PIE_HIP(c, hipMemcpyAsync(b.msg_counts + (long long)q * b.msg_counts_stride, b.counts_ord + (long long)q * batch_users_stride(c),
                                          (size_t)c->n_users * 4, hipMemcpyDefault, s));
        }
        PIE_HIP(c, hipGetLastError());
    }
    if (b.msg_kind == 2 && (!b.union_ok || b.ordered)) {
        // no tail wrote the message (the batch ran on the ordered run: copied from its union; or queries fell back: merged from the lists)
        all_ready = false;
        int rc = order_after_batch(c, b);
        if (rc) return rc;
        rc = batch_pack_union(c, b, b.msg, (size_t)b.msg_u_pad, (size_t)b.msg_cap);
        if (rc) return rc;
    }
    if (ready_out) *ready_out = b.msg_kind ? (all_ready ? 1 : 0) : 1;
    PIE_PROF_TICK(7);
    return PIE_OK;
}

// The union message of a finished batch into caller memory, enqueued on the context's stream.  A batch whose union the tail
// produced: one copy kernel.  Otherwise (queries fell back, the ordered run) the per-query lists are merged per user
// (k_union_collect): 32 query bits, 32 union rows per user — beyond either the message says Mu = -1 (use the lists).
int batch_pack_union(pie_ctx* c, BatchSlot& b, void* dst_i32, size_t u_pad, size_t cap)
{
    hipStream_t s = c->stream;
    if (b.union_ok) {
        size_t total = u_pad + 2 + (size_t)(b.mu < cap ? b.mu : cap);
        size_t grid = (total + 255) / 256;
        if (grid > (size_t)c->n_cus * 8) grid = (size_t)c->n_cus * 8;
        hipLaunchKernelGGL(k_union_pack, dim3((unsigned)(grid ? grid : 1)), dim3(256), 0, s, c->n_users, (int)u_pad, b.uoff, b.urows, b.umlo,
                           b.n_q > 32 ? b.umhi : (const unsigned*)nullptr, (long long)cap, (int*)dst_i32);
        PIE_HIP(c, hipGetLastError());
        return PIE_OK;
    }
    {   // every query's list is needed: the ones still only in the (partial) union are materialised
        int list[kBatchMax], n_list = 0;
        for (int q = 0; q < b.n_q; ++q)
            if (!b.list_ok[q]) list[n_list++] = q;
        int rc = batch_materialize(c, b, list, n_list);
        if (rc) return rc;
    }
    const size_t padded = (((size_t)c->cap_users + 1023) / 1024 + 1) * 1024, groups = padded / 1024 + 2;
    if (c->union_users < c->cap_users || !c->d_union) {
        if ((size_t)c->cap_users * kUnionMax * sizeof(UnionRow) > ((size_t)4 << 30)) return fail(c, PIE_E_NOMEM, "union scratch for %d users exceeds 4 GiB", c->cap_users);
        PIE_HIP(c, hipStreamSynchronize(s));
        dfree(c->d_union); dfree(c->d_union_cnt); dfree(c->d_union_local); dfree(c->d_union_off);
        PIE_HIP(c, hipMalloc(&c->d_union, (size_t)c->cap_users * kUnionMax * sizeof(UnionRow)));
        PIE_HIP(c, hipMalloc(&c->d_union_cnt, padded * 4));
        PIE_HIP(c, hipMalloc(&c->d_union_local, padded * 4));
        PIE_HIP(c, hipMalloc(&c->d_union_off, 2 * groups * 8 + 256 + 64));
        PIE_HIP(c, hipMemsetAsync(c->d_union_cnt, 0, padded * 4, s)); // entries behind the users stay zero for good
        PIE_HIP(c, hipMemsetAsync(c->d_union_off, 0, 2 * groups * 8 + 256 + 64, s)); // incl. the prefix kernel's block counter
        c->union_users = c->cap_users;
    }
    long long* gsum = c->d_union_off;
    long long* gbase = c->d_union_off + groups;
    Summary* usum = reinterpret_cast<Summary*>(reinterpret_cast<char*>(c->d_union_off + 2 * groups));
    int* over = reinterpret_cast<int*>(reinterpret_cast<char*>(usum) + 256);
    OrdCtl* uctl = reinterpret_cast<OrdCtl*>(reinterpret_cast<char*>(usum) + 256 + 16); // its counter returns to 0 by itself
    if (b.n_q > 32) { // the merged form carries 32 query bits
        const int one = 1;
        PIE_HIP(c, hipMemcpyAsync(over, &one, 4, hipMemcpyHostToDevice, s));
        PIE_HIP(c, hipStreamSynchronize(s));
    } else {
        PIE_HIP(c, hipMemsetAsync(over, 0, 4, s));
    }
    UnionLists lists{};
    for (int q = 0; q < b.n_q && q < 32; ++q) lists.idx[q] = b.idx_of[q];
    const unsigned ublocks = (unsigned)((c->n_users + kUnionThreads - 1) / kUnionThreads);
    hipLaunchKernelGGL(k_union_collect, dim3(ublocks ? ublocks : 1u), dim3(kUnionThreads), 0, s, b.n_q < 32 ? b.n_q : 32, c->n_users, b.offsets, batch_users_stride(c),
                       lists, c->d_start, c->d_union, c->d_union_cnt, over);
    long long n_groups = ((long long)c->n_users + 1023) >> 10;
    if (n_groups < 1) n_groups = 1;
    const unsigned pre_grid = (unsigned)(n_groups < (long long)c->n_cus * 4 ? n_groups : (long long)c->n_cus * 4);
    // a hundred groups at most: the one-launch form (the block that finishes last scans the group sums)
    hipLaunchKernelGGL(k_ord_prefix, dim3(pre_grid), dim3(256), 0, s, c->d_union_cnt, (long long)c->n_users, c->d_union_local, gsum, gbase,
                       uctl, usum, 0LL, 0LL, 0LL);
    unsigned wblocks = (unsigned)((u_pad + 2 + 255) / 256);
    if (wblocks > (unsigned)c->n_cus * 8) wblocks = (unsigned)c->n_cus * 8;
    hipLaunchKernelGGL(k_union_write, dim3(wblocks), dim3(256), 0, s, c->n_users, (int)u_pad, c->d_union_local, gbase, c->d_union_cnt, c->d_union, over,
                       (long long)cap, (int*)dst_i32);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}


// ---- wide batches (pie_scan_wide_begin; pie_kernels.h "wide batches").  A wide batch takes a slot of a lane like any batch and
// shares the FIFO; its pass and its union tail (two small launches) are queued at begin — no tail rides in a later launch — and
// the summary with the per-query totals is copied to pinned host memory behind them.  Queries that fall back run on the general
// path at finish for their counts only; their lists are produced again when somebody asks for them, so list storage grows with
// the queries asked for, not with the batch.

// the wide pass's device arrays of a slot: bucket-slot masks (kWideWords words per slot) and union masks (`words` words per
// union row; a union row holds a bucket slot, so (cap_users << dshift) rows bound it)
size_t wide_slot_bytes(const pie_ctx* c) { return ((size_t)c->cap_users << c->bdshift) * kWideWords * 8; }

// `ordered`: a wide batch on the run has no bucket slots; its union is bounded by the result arrays (batch_ucap), not by the slots
int ensure_wide(pie_ctx* c, BatchSlot& b, bool ordered = false)
{
    WideSlot& w = *b.w;
    if (!w.done) PIE_HIP(c, hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    if (!w.h_sum) PIE_HIP(c, hipHostMalloc(&w.h_sum, (size_t)kSummaryBytes + (size_t)kWideMax * 4, hipHostMallocDefault));
    if (!w.h_wq) PIE_HIP(c, hipHostMalloc(&w.h_wq, (size_t)kWideMax * sizeof(WideQuery), hipHostMallocDefault));
    if (!w.d_wq) PIE_HIP(c, hipMalloc(&w.d_wq, (size_t)kWideMax * sizeof(WideQuery)));
    const size_t slots = (size_t)c->cap_users << c->bdshift;
    if (!ordered && (w.dshift != c->bdshift || !w.dmask)) {
        dfree(w.dmask);
        PIE_HIP(c, hipMalloc(&w.dmask, slots * kWideWords * 8));
        w.dshift = c->bdshift;
    }
    const size_t rows = ordered ? batch_ucap(c) : slots;
    if (w.umask_words < w.words || w.umask_rows < rows) {
        dfree(w.umask);
        w.umask_words = 0;
        w.umask_rows = 0;
        PIE_HIP(c, hipMalloc(&w.umask, rows * (size_t)w.words * 8));
        w.umask_words = w.words;
        w.umask_rows = rows;
    }
    if (ordered) {
        if (!w.d_sum) PIE_HIP(c, hipMalloc(&w.d_sum, (size_t)kSummaryBytes + (size_t)kWideMax * 4));
        OrderedRun& o = c->ord;
        if (o.wp_cap < rows || o.wp_words < w.words) {
            dfree(o.wp_rows); dfree(o.wp_mask);
            o.wp_cap = 0; o.wp_words = 0;
            PIE_HIP(c, hipMalloc(&o.wp_rows, rows * 4));
            PIE_HIP(c, hipMalloc(&o.wp_mask, rows * (size_t)w.words * 8));
            o.wp_cap = rows;
            o.wp_words = w.words;
        }
    }
    return PIE_OK;
}

// a wide batch on the ordered run: scan, ONE prefix, emit, publish, then the union message where one was asked for — see
// pie_ordered.h "wide batches on the run".  Scratch as launch_ordered_union: the scan slots' record staging and two summary sets.
int launch_ordered_wide(pie_ctx* c, BatchSlot& b, hipStream_t s, bool fine, unsigned mk)
{
    OrderedRun& o = c->ord;
    WideSlot& w = *b.w;
    const int bi = (int)(&b - c->bslot) & 1;
    char* sums = o.bq_sum[bi];
    int* uc = o.unit_count[o.uc_next];
    int* uc_other = o.unit_count[o.uc_next ^ 1];
    o.uc_next ^= 1;
    OrdWide* ustage = reinterpret_cast<OrdWide*>(c->slot[bi].sel);
    const long long n_chunks = (o.n + 511) >> 9;
    Summary* sum0 = reinterpret_cast<Summary*>(sums);
    unsigned* mq = reinterpret_cast<unsigned*>(sums + ord_sum_bytes()); // the set's mq area: kWideMax totals, then the pool cursor; zero between batches
    const long long ucap = (long long)batch_ucap(c);
    const OrdWidePool pool{o.wp_rows, o.wp_mask, w.words, ucap};
    // 38 / 42 KiB of LDS per block: four / three blocks fit a CU
    long long grid = (long long)c->n_cus * (fine ? 4 : 3);
    if (grid > (n_chunks + 3) / 4) grid = (n_chunks + 3) / 4;
    if (grid < 1) grid = 1;
    b.k1_blocks = (int)grid;
    if (fine) hipLaunchKernelGGL((k_ord_wide_scan<fkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.fkey, o.n, n_chunks, mk, w.d_wq, ustage, uc, pool, mq, sum0);
    else hipLaunchKernelGGL((k_ord_wide_scan<lkey_t>), dim3((unsigned)grid), dim3(256), 0, s, o.pay, o.end, o.key, o.n, n_chunks, mk, w.d_wq, ustage, uc, pool, mq, sum0);
    long long n_groups = (n_chunks + kOrdGroup - 1) >> kOrdGroupShift;
    if (n_groups < 1) n_groups = 1;
    const unsigned pre_grid = (unsigned)(n_groups < (long long)c->n_cus ? n_groups : (long long)c->n_cus);
    hipLaunchKernelGGL(k_ord_prefix, dim3(pre_grid), dim3(256), 0, s, uc, n_chunks, o.bq_local, o.bq_gsum, o.bq_gbase, o.bq_ctl, sum0, 0LL, 0LL, 0LL);
    const int copy_blocks = c->n_cus * 8;
    const int user_blocks = (int)(((long long)c->n_users + 1 + 254) / 255);
    hipLaunchKernelGGL(k_ord_wide_emit, dim3((unsigned)(copy_blocks + user_blocks)), dim3(256), 0, s, o.uoff, c->n_users, o.n, n_chunks, ustage, uc, o.bq_local,
                       o.bq_gbase, pool, b.uoff, b.urows, w.umask, copy_blocks, sum0, uc_other, o.units_cap);
    hipLaunchKernelGGL(k_ord_wide_publish, dim3(1), dim3(kWideMax), 0, s, sum0, mq, ucap, w.d_sum);
    if (b.msg) { // the message of pie_scan_wide_begin_union, complete when the batch's event has passed
        const size_t total = (size_t)b.msg_u_pad + 2 + (size_t)(b.msg_cap < ucap ? b.msg_cap : ucap) * (1 + 2 * (size_t)w.words);
        size_t pgrid = (total + 255) / 256;
        if (pgrid > (size_t)c->n_cus * 8) pgrid = (size_t)c->n_cus * 8;
        hipLaunchKernelGGL(k_wide_pack, dim3((unsigned)(pgrid ? pgrid : 1)), dim3(256), 0, s, c->n_users, b.msg_u_pad, (const long long*)b.uoff,
                           (const int*)b.urows, (const unsigned long long*)w.umask, w.words, b.msg_cap, b.msg);
    }
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(w.h_sum, w.d_sum, (size_t)kSummaryBytes + (size_t)b.n_q * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipEventRecord(w.done, s));
    return PIE_OK;
}

int wide_begin(pie_ctx* c, const pie_query* qs, int n_q, int* msg = nullptr, int u_pad = 0, long long msg_cap = 0)
{
    int rc = begin_checks(c, qs, n_q, kWideMax, "a wide batch");
    if (rc) return rc;
    // a table whose batches take the ordered run, or that cannot run the batched pass: every query falls back
    // (with pie_set_wide_ordered on, the former runs ONE pass over the run's key column: launch_ordered_wide)
    const bool ord_table = batch_supported(c) && ordered_batch_wanted(c) && !c->ord_lists_only;
    const bool ord_wide = ord_table && c->wide_ordered && !c->wide_ord_off;
    bool unsupported = !ord_wide && (ord_table || !batch_supported(c) || c->key_poor || c->batch_poor);
    std::vector<unsigned char> dense((size_t)n_q, 0);
    bool fine = false;
    if (!unsupported && !classify_queries(c, qs, n_q, dense.data(), &fine)) unsupported = true;
    int lane = 0;
    rc = pick_lane(c, ord_table ? 1 : c->n_lanes, &lane);
    if (rc) return rc;
    if (!unsupported && !ord_wide) { // (a wide batch on the run has no union buckets)
        rc = regrow_union_buckets(c);
        if (rc) return rc;
    }
    // the bucket-slot masks are four times the bucket records: the same bound as the direct slots
    if (!unsupported && !ord_wide && wide_slot_bytes(c) > kDirectMaxBytes) unsupported = true;
    BatchSlot& b = lane_slot(c, lane);
    if (!b.w) b.w = new WideSlot();
    WideSlot& w = *b.w;
    w.words = (n_q + 63) / 64;
    if (!unsupported) {
        if (ord_wide) {
            rc = ord_batch_alloc(c);
            if (rc) return rc;
        }
        rc = ensure_batch(c, lane);
        if (rc) return rc;
        rc = ensure_wide(c, b, ord_wide);
        if (rc) return rc;
    }
    claim_slot(c, b, lane, n_q, unsupported, 2, msg, 0, u_pad, msg_cap, nullptr, 0); // (2: the tail writes the wide union message, pie_scan_wide_begin_union)
    b.wide = true;
    b.k2_pending = false;
    w.q.assign(qs, qs + n_q);
    w.fallback.assign((size_t)n_q, 0);
    w.m.assign((size_t)n_q, 0);
    if ((int)w.lists.size() < n_q) w.lists.resize((size_t)n_q);
    for (WideSlot::List& l : w.lists) l.ok = false;
    for (int q = 0; q < n_q; ++q) w.fallback[q] = unsupported ? 1 : dense[q];
    if (unsupported) {
        begin_fallback_only(c, b);
        return PIE_OK;
    }
    hipStream_t s = b.stream;
    rc = order_lane_after_main(c, lane);
    if (rc) return rc;
    rc = lane_after_mutation(c, lane);
    if (rc) return rc;
    b.fine_key = fine;
    b.dshift = c->bdshift;
    if (!ord_wide) take_spans(c, b);
    b.seq = ++c->bseq_counter;
    if (!ord_wide) b.k1_blocks = c->plan_blocks[fine ? 3 : 2]; // (launch_ordered_wide sets its own grid)
    c->scans_begun++;
    if (BatchSlot* prev = waiting_tail(c, lane)) launch_batch_k2(c, *prev, s);
    // the queries as the lanes hold them: a query that falls back has mask 0 and selects nothing here
    const unsigned long long table = c->n_disc >= 64 ? ~0ull : ((1ull << c->n_disc) - 1ull);
    unsigned mk = fine ? 0xFFu : 0xFFFFu;
    for (int i = 0; i < kWideMax; ++i) {
        WideQuery& x = w.h_wq[i];
        x.pad = 0;
        if (i < n_q && !w.fallback[i]) {
            x.now = qs[i].now;
            x.cutoff = qs[i].cutoff;
            x.mask = qs[i].mask & table;
            x.nk = fine ? host_fine_key_of(c, qs[i].now) : host_key_of(c, qs[i].now);
            if (x.nk < mk) mk = x.nk;
        } else {
            x.now = INT64_MAX;
            x.cutoff = INT64_MAX;
            x.mask = 0;
            x.nk = ~0u;
        }
    }
    PIE_HIP(c, hipMemcpyAsync(w.d_wq, w.h_wq, (size_t)kWideMax * sizeof(WideQuery), hipMemcpyHostToDevice, s));
    if (ord_wide) {
        rc = launch_ordered_wide(c, b, s, fine, mk);
        if (rc) return rc;
        b.ordered = true;
        b.in_flight = true;
        batch_begun(c, lane);
        return PIE_OK;
    }
    char* const sp = b.span;
    Summary* const sum = reinterpret_cast<Summary*>(sp + span_counts_bytes(c) + span_tiles_bytes(c) + span_parts_bytes() + 128);
    unsigned* const mq = reinterpret_cast<unsigned*>(sp + counts_span(c));
#define PIE_WIDE(KT, KEYPTR)                                                                                            \
    do {                                                                                                                \
        WideScanArgs<KT> a;                                                                                             \
        a.pay = c->d_pay; a.end = c->d_end; a.key = KEYPTR; a.n = c->n; a.n_users = c->n_users;                         \
        a.dshift = c->bdshift; a.run_shift = c->run_shift; a.min_key = mk;                                              \
        a.counts = reinterpret_cast<int*>(sp); a.summary = sum; a.direct = b.direct; a.dmask = w.dmask; a.mq = mq;      \
        a.wq = w.d_wq;                                                                                                  \
        hipLaunchKernelGGL((k_scan_wide<8, true, KT>), dim3((unsigned)b.k1_blocks), dim3(kK1Threads), 0, s, a);       \
    } while (0)
    if (fine) PIE_WIDE(fkey_t, c->d_fkey);
    else PIE_WIDE(lkey_t, c->d_key);
#undef PIE_WIDE
    WideTailArgs t;
    t.n_users = c->n_users;
    t.dshift = c->bdshift;
    t.words = w.words;
    t.counts = reinterpret_cast<const int*>(sp);
    t.tile_sum = reinterpret_cast<long long*>(sp + span_counts_bytes(c));
    t.summary = sum;
    t.direct = b.direct;
    t.dmask = w.dmask;
    t.uoff = b.uoff;
    t.urows = b.urows;
    t.umask = w.umask;
    const unsigned tiles = (unsigned)((c->n_users + 255) / 256);
    hipLaunchKernelGGL(k_wide_tiles, dim3(tiles), dim3(256), 0, s, t);
    if (b.msg) hipLaunchKernelGGL(k_wide_order_msg, dim3(tiles), dim3(256), 0, s, t, WideMsgArgs{b.msg, b.msg_u_pad, b.msg_cap});
    else hipLaunchKernelGGL(k_wide_order, dim3(tiles), dim3(256), 0, s, t);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(w.h_sum, sum, sizeof(Summary), hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipMemcpyAsync(reinterpret_cast<char*>(w.h_sum) + kSummaryBytes, mq, (size_t)n_q * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipEventRecord(w.done, s));
    // the span of the batch before this one on the lane (done in stream order) is zeroed for the batch after the next
    PIE_HIP(c, hipMemsetAsync(b.zero_span, 0, batch_span_bytes(c), s));
    b.in_flight = true;
    batch_begun(c, lane);
    return PIE_OK;
}

// query q's lists of a wide batch in its per-query storage (idx sized for m rows)
int wide_list_alloc(pie_ctx* c, WideSlot& w, int q, long long m)
{
    WideSlot::List& l = w.lists[q];
    if (!l.counts) PIE_HIP(c, hipMalloc(&l.counts, ((size_t)c->cap_users + 1) * 4));
    if (!l.offsets) PIE_HIP(c, hipMalloc(&l.offsets, ((size_t)c->cap_users + 1) * 8));
    if (!l.idx || l.idx_cap < m) {
        PIE_HIP(c, hipStreamSynchronize(c->stream)); // an earlier copy may still read the old buffer
        dfree(l.idx);
        l.idx_cap = 0;
        PIE_HIP(c, hipMalloc(&l.idx, (size_t)(m > 0 ? m : 1) * 4));
        l.idx_cap = m > 0 ? m : 1;
    }
    return PIE_OK;
}

// the listed queries of a wide batch on the general path, two scans in flight (as batch_fallback_many): their counts, and with
// `keep` their lists too
int wide_rerun(pie_ctx* c, BatchSlot& b, const int* list, int n_list, bool keep, unsigned* bad_out)
{
    if (n_list == 0) return PIE_OK;
    WideSlot& w = *b.w;
    const unsigned long long keep_mask = c->disc_mask;
    auto begin = [&](int q) {
        c->disc_mask = w.q[q].mask;
        return scan_begin(c, w.q[q].now, w.q[q].cutoff);
    };
    int rc = begin(list[0]);
    for (int i = 0; i < n_list && rc == PIE_OK; ++i) {
        if (i + 1 < n_list) rc = begin(list[i + 1]);
        if (rc == PIE_OK) rc = scan_finish(c);
        if (rc != PIE_OK) break;
        const int q = list[i];
        Slot& sl = *c->res;
        const long long m = (long long)sl.last.m;
        w.m[q] = (unsigned long long)m;
        if (bad_out && sl.last.bad_rows > *bad_out) *bad_out = sl.last.bad_rows;
        if (keep) {
            rc = wide_list_alloc(c, w, q, m);
            if (rc) break;
            WideSlot::List& l = w.lists[q];
            hipStream_t s = c->stream;
            PIE_HIP(c, hipMemcpyAsync(l.counts, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDeviceToDevice, s));
            PIE_HIP(c, hipMemcpyAsync(l.offsets, sl.offsets, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToDevice, s));
            if (m) PIE_HIP(c, hipMemcpyAsync(l.idx, sl.out_idx, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
            l.ok = true;
        }
    }
    c->disc_mask = keep_mask;
    if (rc != PIE_OK) {
        while (c->n_flight) (void)scan_finish(c);
        return rc;
    }
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    for (Slot& sl : c->slot) sl.have_result = false;
    c->res = nullptr;
    return PIE_OK;
}

// query q's counts / offsets / row list of the last finished (wide) batch, produced on first use
int wide_need_list(pie_ctx* c, BatchSlot& b, int q)
{
    WideSlot& w = *b.w;
    if (w.lists[q].ok) return PIE_OK;
    if (w.fallback[q] || !b.union_part) return fail(c, PIE_E_STATE, "query %d of the wide batch has no list", q); // built at finish
    int rc = wide_list_alloc(c, w, q, (long long)w.m[q]);
    if (rc) return rc;
    WideSlot::List& l = w.lists[q];
    hipStream_t s = c->stream;
    const unsigned tiles = (unsigned)((c->n_users + 255) / 256);
    hipLaunchKernelGGL(k_wide_mat_count, dim3(tiles ? tiles : 1u), dim3(256), 0, s, c->n_users, (const long long*)b.uoff,
                       (const unsigned long long*)w.umask, w.words, q, l.counts);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, (const int*)l.counts, c->n_users, l.offsets, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_wide_mat_write, dim3(tiles ? tiles : 1u), dim3(256), 0, s, c->n_users, (const long long*)b.uoff, (const int*)b.urows,
                       (const unsigned long long*)w.umask, w.words, q, (const long long*)l.offsets, l.idx, l.idx_cap);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipStreamSynchronize(s));
    l.ok = true;
    return PIE_OK;
}

int wide_finish(pie_ctx* c, size_t* m_out, size_t m_cap, int* n_q_out, int* ready_out = nullptr)
{
    if (ready_out) *ready_out = 0;
    BatchSlot* bp = oldest_batch(c);
    if (!bp) return fail(c, PIE_E_STATE, "pie_scan_wide_finish without a batch in flight");
    if (n_q_out) *n_q_out = bp->n_q;
    if (m_out && m_cap < (size_t)bp->n_q) return fail(c, PIE_E_CAPACITY, "m_cap %zu < %d queries", m_cap, bp->n_q);
    if (!bp->wide) { // an ordinary batch is the oldest: finished as pie_scan_batch_finish does
        int rc = batch_finish(c, ready_out);
        if (rc) return rc;
        if (m_out)
            for (int q = 0; q < c->bres->n_q; ++q) m_out[q] = (size_t)c->bres->last[q].m;
        return PIE_OK;
    }
    BatchSlot& b = *bp;
    WideSlot& w = *b.w;
    if (!b.unsupported) {
        // wait for the summary's copy, bounded like batch_finish's wait (PIE_WAIT_DEADLINE_MS)
        const WaitResult wr = event_wait(c, w.done);
        if (wr.end != WaitEnd::Ready) {
            batch_left(c, b);
            if (wr.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "wide batch failed: %s", hipGetErrorString((hipError_t)wr.err));
            return fail(c, PIE_E_HIP, "wide batch not finished within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", wr.waited_ms);
        }
        const Summary us = *w.h_sum;
        const unsigned* mq = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(w.h_sum) + kSummaryBytes);
        b.mu = us.m;
        // a bucket outgrew its slots or a selected row has a bad user id: every query is rerun on the general path
        const bool overflow = us.n_over > 0 || us.bad_rows > 0;
        for (int q = 0; q < b.n_q; ++q) {
            w.m[q] = mq[q];
            if (overflow) w.fallback[q] = 1;
        }
        if (us.n_over > 0 && b.ordered) c->wide_ord_off = true; // the union outgrew the result arrays on the run: later wide batches rerun their queries
        else if (us.n_over > 0) {
            if (c->bdshift < kUnionShiftMax) c->bdshift_want = c->bdshift + 1;
            else c->batch_poor = true;
        }
        b.last[0] = us; // the pass's statistics (pie_stats_get)
        b.union_part = !overflow;
        b.union_ok = !overflow;
        for (int q = 0; q < b.n_q; ++q) b.union_ok = b.union_ok && !w.fallback[q];
        if (!b.ordered) choose_run_shift(c, us.cand, us.chunk_max, b.fine_key);
    }
    batch_left(c, b);
    unsigned bad = 0;
    {
        std::vector<int> list;
        for (int q = 0; q < b.n_q; ++q)
            if (w.fallback[q]) list.push_back(q);
        if (!list.empty()) {
            int rc = order_after_batch(c, b);
            if (rc) return rc;
            // their lists are built now, as batch_fallback_many does: a snapshot of the table as the batch saw it
            rc = wide_rerun(c, b, list.data(), (int)list.size(), true, &bad);
            if (rc) return rc;
        }
    }
    b.have_result = true;
    c->bres = &b;
    c->last_was_batch = true;
    if (b.msg_kind == 2) {
        // the tail wrote the message (complete: its event has passed) unless the batch kept no union: then the header says so
        // (Mu = -1, uoff all -1), written on the context's stream behind the batch
        const bool kept = !b.unsupported && b.union_ok;
        if (!kept || !ready_out) {
            int rc = order_after_batch(c, b);
            if (rc) return rc;
        }
        if (!kept) {
            unsigned grid = (unsigned)((b.msg_u_pad + 2 + 255) / 256);
            if (grid > (unsigned)c->n_cus * 8) grid = (unsigned)c->n_cus * 8;
            hipLaunchKernelGGL(k_wide_msg_none, dim3(grid), dim3(256), 0, c->stream, b.msg, b.msg_u_pad);
            PIE_HIP(c, hipGetLastError());
        }
        if (ready_out) *ready_out = kept ? 1 : 0;
    } else if (ready_out) *ready_out = 1; // no message to wait for (as pie_scan_batch_finish_packed)
    if (bad) return fail(c, PIE_E_INVAL, "%u selected rows carry a user id outside [0, %d)", bad, c->n_users);
    if (m_out)
        for (int q = 0; q < b.n_q; ++q) m_out[q] = (size_t)w.m[q];
    return PIE_OK;
}

// the last finished batch, when it is wide and kept its union
int wide_union_of(pie_ctx* c, BatchSlot** out)
{
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (!c->bres->wide) return fail(c, PIE_E_STATE, "the last finished batch is not wide: use the batch union readers");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o;
    if (!c->bres->union_ok)
        return fail(c, PIE_E_STATE, "this wide batch has no union result (queries fell back to the general path): read the per-query results");
    *out = c->bres;
    return PIE_OK;
}

} // namespace

extern "C" {

int pie_abi_version(void) { return PIE_ABI_VERSION; }

int pie_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* pie_last_error(const pie_ctx* ctx) { return ctx ? ctx->err : g_create_error; }

int pie_ctx_create(int device_id, pie_ctx** ctx_out)
{
    if (!ctx_out) return fail(nullptr, PIE_E_INVAL, "ctx_out is NULL");
    *ctx_out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, PIE_E_NODEVICE, "no HIP device (%s); this library has no CPU path",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, PIE_E_INVAL, "device %d outside [0, %d)", device_id, n);
    if ((e = hipSetDevice(device_id)) != hipSuccess)
        return fail(nullptr, PIE_E_NODEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    pie_ctx* c = new (std::nothrow) pie_ctx();
    if (!c) return fail(nullptr, PIE_E_NOMEM, "out of host memory");
    c->device = device_id;
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
        delete c;
        return fail(nullptr, PIE_E_NODEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    }
    c->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    bool ok = (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) == hipSuccess;
    // the lanes' streams right behind the main one: the runtime deals its (four) hardware queues to streams in the order they
    // first appear, and a lane that ends up sharing a queue with another lane runs behind it, not beside it
    for (int l = 1; l < kLaneMax && ok; ++l) ok = (e = hipStreamCreateWithFlags(&c->lane_stream[l], hipStreamNonBlocking)) == hipSuccess;
    ok = ok &&
              (e = hipMalloc(&c->d_summary, sizeof(Summary))) == hipSuccess &&
              (e = hipMalloc(&c->d_range, 16)) == hipSuccess &&
              (e = hipMalloc(&c->d_hist, kKeyHistBins * sizeof(unsigned int))) == hipSuccess &&
              (e = hipHostMalloc(&c->h_summary, sizeof(Summary), hipHostMallocDefault)) == hipSuccess;
    for (Slot& s : c->slot) {
        ok = ok && (e = hipHostMalloc(&s.h_sum, sizeof(HostSummary), hipHostMallocMapped)) == hipSuccess &&
             (e = hipHostGetDevicePointer((void**)&s.h_sum_dev, s.h_sum, 0)) == hipSuccess;
        if (ok) memset(s.h_sum, 0, sizeof(HostSummary));
    }
    ok = ok && (e = hipHostMalloc(&c->ord.h_stale, 64, hipHostMallocMapped)) == hipSuccess &&
         (e = hipHostGetDevicePointer((void**)&c->ord.stale, c->ord.h_stale, 0)) == hipSuccess;
    if (ok) memset(c->ord.h_stale, 0, 64);
    for (BatchSlot& b : c->bslot) {
        ok = ok && (e = hipHostMalloc(&b.bh, sizeof(BatchHost), hipHostMallocMapped)) == hipSuccess &&
             (e = hipHostGetDevicePointer((void**)&b.bh_dev, b.bh, 0)) == hipSuccess;
        if (ok) memset(b.bh, 0, sizeof(BatchHost));
    }
    if (!ok) {
        fail(nullptr, PIE_E_NODEVICE, "context setup: %s", hipGetErrorString(e));
        delete c; // the few handles created so far go with the process: it has no usable GPU anyway
        return PIE_E_NODEVICE;
    }
    c->stream = c->own_stream;
    if (const char* v = getenv("PIE_K1_VARIANT")) { c->k1_variant = (int)strtol(v, nullptr, 0); c->k1_pinned = true; }
    if (const char* v = getenv("PIE_K1_LIVE_FIRST")) c->k1_live_first = (int)strtol(v, nullptr, 0);
    if (const char* v = getenv("PIE_FAST_PATH")) c->fast_env = atoi(v) != 0;
    if (const char* v = getenv("PIE_FUSED_ORDER")) c->no_fused_order = atoi(v) == 0;
    if (const char* v = getenv("PIE_K2_RIDE")) c->no_ride = atoi(v) == 0;
    if (const char* v = getenv("PIE_EXPIRED_COPY_TOTAL")) c->expired_copy_total = atoi(v) != 0;
    if (const char* v = getenv("PIE_ASYNC_MUTATIONS")) c->async_mutations = atoi(v) != 0;
    if (const char* v = getenv("PIE_HOT_INDEX")) c->hix.enabled = atoi(v) != 0;
    if (const char* v = getenv("PIE_HOT_RECS")) { const int r = atoi(v); if (r == 1 || r == 2 || r == 4) c->hix.recs_per_thread = r; }
    if (const char* v = getenv("PIE_HOT_ORDER")) { if (!strcmp(v, "row")) c->hix.order = 0; else if (!strcmp(v, "slot")) c->hix.order = 1; }
    if (const char* v = getenv("PIE_BATCH_LANES")) { const int l = atoi(v); if (l >= 0 && l <= kLaneMax) c->lanes_want = l; }
    if (const char* v = getenv("PIE_ORDER_BLOCK")) { const int b = atoi(v); if (b == 256 || b == 512 || b == 1024) c->order_block = b; }
    if (const char* v = getenv("PIE_RUN_SHIFT")) { const int r = atoi(v); if (r >= 0 && r <= 3) { c->run_shift = r; c->run_shift_pinned = true; } }
    if (const char* v = getenv("PIE_ORDERED")) { const int m = atoi(v); if (m >= 0 && m <= 2) c->ord.mode = m; }
    if (const char* v = getenv("PIE_WIDE_ORDERED")) c->wide_ordered = atoi(v) == 1;
    if (const char* v = getenv("PIE_TURN_ORDERED")) c->turn_ordered = atoi(v) == 1;
    if (const char* v = getenv("PIE_ORD_GRID")) { const int g = atoi(v); if (g >= 1 && g <= 64) c->ord.grid_mult = g; }
    if (const char* v = getenv("PIE_WAIT_DEADLINE_MS")) { const double d = atof(v); if (d > 0) c->wait_deadline_ms = d; }
    if (const char* v = getenv("PIE_EXPQ_BLOCKS_PER_CU")) { const int g = atoi(v); if (g >= 1 && g <= 16) c->expq.blocks_per_cu = g; }
    if (const char* v = getenv("PIE_EXPQ_MAX_BLOCKS")) { const int g = atoi(v); if (g >= 1) c->expq.max_blocks = g; }
    if (const char* v = getenv("PIE_K1_KEYED")) {
        const int k = (int)strtol(v, nullptr, 0);
        c->keyed_enabled = k != 0;
        if (k & 0x400) c->k1_keyed = k;
    }
    *ctx_out = c;
    return PIE_OK;
}

int pie_ctx_destroy(pie_ctx* c)
{
    if (!c) return PIE_OK;
#ifdef PIE_HOST_PROF
    g_prof.report();
#endif
    (void)hipSetDevice(c->device);
    (void)side_passes_land(c, "pie_ctx_destroy");
    (void)hipStreamSynchronize(c->stream);
    free_table(c);
    dfree(c->d_shard_rows);
    dfree(c->d_shard_users);
    cmp_forget(c);
    token_drop(c);
    dfree(c->tokx.status);
    dfree(c->tokx.d_stage);
    if (c->tokx.h_stage) (void)hipHostFree(c->tokx.h_stage);
    if (c->tokx.turn_done) (void)hipEventDestroy(c->tokx.turn_done);
    for (hipEvent_t e : c->tokx.ev)
        if (e) (void)hipEventDestroy(e);
    side_close(c->tokx.side);
    for (auto& l : c->tokx.lk) {
        if (l.h) (void)hipHostFree(l.h);
        dfree(l.d);
        for (hipEvent_t e : {l.fence.order, l.fence.done})
            if (e) (void)hipEventDestroy(e);
    }
    for (auto& u : c->tokx.tn) {
        if (u.h) (void)hipHostFree(u.h);
        dfree(u.d);
        if (u.done) (void)hipEventDestroy(u.done);
    }
    if (c->mut_event) (void)hipEventDestroy(c->mut_event);
    side_close(c->expq.side);
    dfree(c->expq.d_scratch);
    dfree(c->expq.d_buf);
    if (c->expq.h_sum) (void)hipHostFree(c->expq.h_sum);
    for (hipEvent_t e : {c->expq.fence.order, c->expq.t0, c->expq.fence.done})
        if (e) (void)hipEventDestroy(e);
    dfree(c->d_stage);
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    for (auto& a : c->astage) {
        if (a.h) (void)hipHostFree(a.h);
        if (a.d) (void)hipFree(a.d);
        if (a.ev) (void)hipEventDestroy(a.ev);
    }
    for (auto& e : c->ring) {
        (void)hipEventDestroy(e.e0); (void)hipEventDestroy(e.e1); (void)hipEventDestroy(e.e2);
    }
    for (Slot& s : c->slot) {
        if (s.h_sum) (void)hipHostFree(s.h_sum);
    }
    for (BatchSlot& b : c->bslot) {
        if (b.bh) (void)hipHostFree(b.bh);
    }
    if (c->ord.h_stale) (void)hipHostFree(c->ord.h_stale);
    if (c->d_summary) (void)hipFree(c->d_summary);
    if (c->d_range) (void)hipFree(c->d_range);
    if (c->d_hist) (void)hipFree(c->d_hist);
    if (c->h_summary) (void)hipHostFree(c->h_summary);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    for (int l = 1; l < kLaneMax; ++l)
        if (c->lane_stream[l]) (void)hipStreamDestroy(c->lane_stream[l]);
    for (auto& pair : c->lane_event)
        for (hipEvent_t e : pair)
            if (e) (void)hipEventDestroy(e);
    delete c;
    return PIE_OK;
}

// Lanes of the batched scan: 1..4 pins the number, 0 chooses by the size of the resident table (whenever it changes).  May be
// called at any time: a batch in flight stays on the lane it was begun on.
int pie_set_batch_lanes(pie_ctx* c, int n_lanes)
{
    if (!c) return PIE_E_INVAL;
    if (n_lanes < 0 || n_lanes > kLaneMax) return fail(c, PIE_E_INVAL, "lanes outside 0..%d", kLaneMax);
    c->lanes_want = n_lanes;
    choose_lanes(c);
    return PIE_OK;
}

int pie_batch_lanes(pie_ctx* c) { return c ? c->n_lanes : 0; }

// how many more batches pie_scan_batch_begin would take right now
int pie_batch_room(pie_ctx* c)
{
    if (!c || c->n_flight) return 0;
    const bool ord_batch = batch_supported(c) && ordered_batch_wanted(c) && !c->ord_lists_only;
    const int lanes = ord_batch ? 1 : c->n_lanes;
    int room = 0;
    for (int l = 0; l < lanes; ++l) room += kBatchSlots - c->lane_flight[l];
    return room;
}

int pie_ctx_set_stream(pie_ctx* c, void* hip_stream)
{
    if (!c) return PIE_E_INVAL;
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    int rc = sync_all(c);
    if (rc) return rc;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return PIE_OK;
}

int pie_ctx_aux_stream(pie_ctx* c, void** hip_stream_out)
{
    if (!c || !hip_stream_out) return PIE_E_INVAL;
    *hip_stream_out = (void*)c->stream;
    return PIE_OK;
}

int pie_load_columns(pie_ctx* c, const int64_t* start, const int64_t* end, const int32_t* user, const int32_t* disc,
                     size_t n, int32_t n_users)
{
    if (!c) return PIE_E_INVAL;
    if (n > 0 && (!start || !end || !user || !disc)) return fail(c, PIE_E_INVAL, "NULL column pointer");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = ensure_capacity(c, (long long)n, n_users);
    if (rc) return rc;
    if (n > 0) {
        PIE_HIP(c, hipMemcpyAsync(c->d_start, start, n * 8, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_end, end, n * 8, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_user, user, n * 4, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_disc, disc, n * 4, hipMemcpyHostToDevice, c->stream));
    }
    rc = validate_users(c);
    if (rc) { c->n = 0; plan_k1(c); return rc; }
    return build_keys(c, 0);
}

// ---- the small mutations (append, touch), plain and by global id: one staging helper, one launch site per kernel
//
// A mutation that needs nothing back from the device is queued, not waited for (see AsyncStage).  Queued and waited forms stage,
// upload and launch alike; they differ in what follows the launch (queued: the area's event; waited: the read-back and the wait)
// and in the bad_rows memset the waited appends put in front of it.
static bool mutation_queued(const pie_ctx* c) { return c->async_mutations && !c->ord.valid; }

// blocks of a grid-stride kernel over k elements: one per 256, at most 8 per CU
static unsigned capped_grid(const pie_ctx* c, size_t k)
{
    return (unsigned)((k + 255) / 256) < (unsigned)c->n_cus * 8 ? (unsigned)((k + 255) / 256) : (unsigned)c->n_cus * 8;
}

// The staging block of one mutation: pinned host memory to fill, the device block it is uploaded to, and the AsyncStage it
// belongs to when the mutation is queued (NULL: the context's own pair, and the mutation is waited for).
struct Staged {
    char* h;
    char* d;
    pie_ctx::AsyncStage* a;
};
static int stage_mutation(pie_ctx* c, size_t bytes, bool queued, Staged* st)
{
    pie_ctx::AsyncStage* a = nullptr;
    int rc = queued ? async_stage(c, bytes, &a) : ensure_stage(c, bytes);
    if (rc) return rc;
    *st = queued ? Staged{a->h, a->d, a} : Staged{c->h_stage, c->d_stage, nullptr};
    return PIE_OK;
}
// a queued mutation is in the stream: its area is busy until the event behind it
static int stage_queued(pie_ctx* c, const Staged& st)
{
    PIE_HIP(c, hipEventRecord(st.a->ev, c->stream));
    st.a->pending = true;
    return PIE_OK;
}

static void drop_results(pie_ctx* c)
{
    c->res = nullptr;
    for (Slot& sl : c->slot) sl.have_result = false;
    c->bres = nullptr;
}

// a failed append on a path that moved c->n (ensure_capacity) takes it back
static int append_rollback(pie_ctx* c, long long old_n, int rc)
{
    c->n = old_n;
    plan_k1(c);
    return rc;
}

// the end of every append that added rows (n_users: the context's own, local, user count after the call)
static int append_finish(pie_ctx* c, int n_users)
{
    if (n_users > c->n_users) set_user_count(c, n_users);
    c->key_dirty = true;
    queue_forget(c); // the held queue names groups as the table was before the rows came
    drop_results(c);
    plan_k1(c);
    return ensure_sel(c);
}

// What follows the append kernel of the in-place path.  Queued form: nothing is read back, the table's size moves at once.
static int append_queued_tail(pie_ctx* c, const Staged& st, long long old_n, size_t k, int n_users)
{
    int rc = stage_queued(c, st);
    if (rc) return rc;
    c->n = old_n + (long long)k;
    ord_invalidate(c);
    return append_finish(c, n_users);
}

// Waited form: the kernel's count of bad user ids and the ordered run's bookkeeping are read once the stream has drained.
static int append_waited_tail(pie_ctx* c, long long old_n, size_t k, int n_users, bool ord_kept, bool global_ids)
{
    hipStream_t s = c->stream;
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(Summary), hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    if (c->h_summary->bad_rows) { // the rows were written beyond n: the table itself is unchanged (the hot index is not)
        c->hix.valid = false;
        if (ord_kept) { // ... but some of them may sit in the run's spare slots
            ord_invalidate(c);
            c->ord.h_stale[0] = c->ord.h_stale[1] = 0;
        }
        if (global_ids) return fail(c, PIE_E_INVAL, "%u rows carry a user id the shard's user map does not hold", c->h_summary->bad_rows);
        return fail(c, PIE_E_INVAL, "%u rows carry a user id outside [0, %d)", c->h_summary->bad_rows, n_users);
    }
    c->n = old_n + (long long)k;
    if (ord_kept) {
        volatile unsigned int* st = c->ord.h_stale; // [0] rows out of time order, [1] rows whose segment was full
        if (st[0] == 0 && st[1] != 0) {
            int rc2 = ord_respread(c, c->d_stage, k, old_n, n_users);
            if (rc2) return rc2;
        } else if (st[0] != 0) ord_invalidate(c, false, true);
        c->ord.h_stale[0] = c->ord.h_stale[1] = 0;
        if (c->ord.valid) {
            c->ord.rows = c->n;
            c->ord.held += (long long)k;
        }
    } else ord_invalidate(c);
    return append_finish(c, n_users);
}

// What a sharded append adds to a plain one: k_call rows went to all shards (this one keeps k of them), n_new users join the
// shard's user map, and the maps are committed once the kernel is queued (shard_append_commit, defined with the sharded calls).
struct ShardAppend {
    size_t k_call, n_new;
    int32_t n_users_global;
};
static int append_launch(pie_ctx* c, const Staged& st, size_t k, long long row0, int n_users, const ShardAppend* sh, bool with_keys);
static int append_in_place(pie_ctx* c, const Staged& st, size_t k, int n_users, const ShardAppend* sh);

int pie_append_rows(pie_ctx* c, const int64_t* start, const int64_t* end, const int32_t* user, const int32_t* disc,
                    size_t k, int32_t n_users)
{
    if (!c) return PIE_E_INVAL;
    if (k > 0 && (!start || !end || !user || !disc)) return fail(c, PIE_E_INVAL, "NULL column pointer");
    if (n_users < c->n_users) return fail(c, PIE_E_INVAL, "n_users may only grow (%d < %d)", n_users, c->n_users);
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    PIE_HIP(c, hipSetDevice(c->device));
    const long long old_n = c->n;
    if (k > 0 && old_n > 0 && old_n + (long long)k <= c->cap_rows && n_users <= c->cap_users && c->key_ok && k <= ((size_t)1 << 24)) {
        // In-place path (room for the rows and the users, key columns in step): ONE staged upload, ONE kernel that writes the
        // four columns, both keys and the payload record of every new row and validates the user ids, and ONE wait or none.  A
        // login burst costs tens of microseconds, not the half-dozen blocking calls of the general path below.
        if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "table change while a scan is in flight");
        if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
        if (old_n + (long long)k >= (1LL << 31) - 1) return fail(c, PIE_E_INVAL, "row count outside [0, 2^31 - 1)");
        hot_reserve(c, (long long)k);
        const bool queued = mutation_queued(c);
        if (queued) { // nothing will be read back: the user ids are checked here
            unsigned bad = 0;
            for (size_t i = 0; i < k; ++i) bad += (unsigned)user[i] >= (unsigned)n_users ? 1u : 0u;
            if (bad) return fail(c, PIE_E_INVAL, "%u rows carry a user id outside [0, %d)", bad, n_users);
        }
        Staged st{};
        int rc0 = stage_mutation(c, k * 24 + 64, queued, &st);
        if (rc0) return rc0;
        memcpy(st.h, start, k * 8);
        memcpy(st.h + k * 8, end, k * 8);
        memcpy(st.h + k * 16, user, k * 4);
        memcpy(st.h + k * 20, disc, k * 4);
        return append_in_place(c, st, k, n_users, nullptr);
    }
    int rc = ensure_capacity(c, old_n + (long long)k, n_users, old_n > 0 ? old_n : 1);
    if (rc) return rc;
    if (k > 0) {
        PIE_HIP(c, hipMemcpyAsync(c->d_start + old_n, start, k * 8, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_end + old_n, end, k * 8, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_user + old_n, user, k * 4, hipMemcpyHostToDevice, c->stream));
        PIE_HIP(c, hipMemcpyAsync(c->d_disc + old_n, disc, k * 4, hipMemcpyHostToDevice, c->stream));
    }
    rc = validate_users(c, old_n);
    if (rc) return append_rollback(c, old_n, rc);
    return build_keys(c, old_n);
}

int pie_gen_synthetic(pie_ctx* c, uint64_t seed, int64_t n_total, int64_t row0, int64_t n, int32_t n_users,
                      int32_t n_disc, uint32_t flags)
{
    if (!c) return PIE_E_INVAL;
    if (n < 0 || row0 < 0 || n_total < row0 + n || n_disc < 1 || n_disc > 64)
        return fail(c, PIE_E_INVAL, "bad synthetic-corpus shape");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = ensure_capacity(c, n, n_users);
    if (rc) return rc;
    if (n > 0) {
        hipLaunchKernelGGL(k_gen, dim3(c->n_cus * 8), dim3(256), 0, c->stream, seed, (long long)n_total, (long long)row0,
                           (long long)n, n_users, n_disc, flags, c->d_start, c->d_end, c->d_user, c->d_disc);
        PIE_HIP(c, hipGetLastError());
    }
    rc = build_keys(c, 0);
    if (rc) return rc;
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

int pie_gen_synthetic_cdf(pie_ctx* c, uint64_t seed, int64_t n_total, int64_t row0, int64_t n, int32_t n_users,
                          int32_t n_disc, uint32_t flags, const uint64_t* cdf)
{
    if (!c) return PIE_E_INVAL;
    if (!cdf) return fail(c, PIE_E_INVAL, "cdf is NULL");
    int rc = pie_gen_synthetic(c, seed, n_total, row0, n, n_users, n_disc, flags & ~2u);
    if (rc || n == 0) return rc;
    unsigned long long* d_cdf = nullptr;
    PIE_HIP(c, hipMalloc(&d_cdf, (size_t)n_users * 8));
    hipError_t e = hipMemcpyAsync(d_cdf, cdf, (size_t)n_users * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gen_users_cdf, dim3(c->n_cus * 8), dim3(256), 0, c->stream, seed, (long long)row0, (long long)n,
                           n_users, d_cdf, c->d_user);
        e = hipGetLastError();
    }
    hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(d_cdf);
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(c, PIE_E_HIP, "pie_gen_synthetic_cdf: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    c->key_ok = false; // the user column was rewritten: the payload column has to follow
    rc = build_keys(c, 0);
    if (rc) return rc;
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

// ---- on-disk column format: <dir>/start.i64, end.i64, user.i32, disc.i32 (raw little-endian arrays) and
// <dir>/header.json {"format":"pie-columns","version":1,"rows":N,"users":U}.  Contrast: the reference exports its whole
// SQLite image after every mutation (/root/reference/server/storage/sqlProvider.js:737-744) and keeps sessions in memory
// only (/root/reference/server/sessionStore.js:6).
namespace {
int write_file(pie_ctx* c, const std::string& path, const void* data, size_t bytes)
{
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return fail(c, PIE_E_INVAL, "cannot create %s", path.c_str());
    const char* p = static_cast<const char*>(data);
    size_t left = bytes;
    while (left) {
        const ssize_t w = write(fd, p, left > (1u << 30) ? (1u << 30) : left);
        if (w <= 0) { close(fd); return fail(c, PIE_E_INVAL, "short write to %s", path.c_str()); }
        p += w;
        left -= (size_t)w;
    }
    close(fd);
    return PIE_OK;
}
} // namespace

int pie_save_columns(pie_ctx* c, const char* dir)
{
    if (!c || !dir) return PIE_E_INVAL;
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    PIE_HIP(c, hipSetDevice(c->device));
    (void)mkdir(dir, 0755);
    const size_t n = (size_t)c->n;
    std::vector<char> host(n * 8 + 8);
    const std::string base(dir);
    struct { const char* name; const void* dev; size_t width; } cols[4] = {
        {"/start.i64", c->d_start, 8}, {"/end.i64", c->d_end, 8}, {"/user.i32", c->d_user, 4}, {"/disc.i32", c->d_disc, 4}};
    for (auto& col : cols) {
        if (n) PIE_HIP(c, hipMemcpy(host.data(), col.dev, n * col.width, hipMemcpyDeviceToHost));
        int rc = write_file(c, base + col.name, host.data(), n * col.width);
        if (rc) return rc;
    }
    char hdr[256];
    const int len = snprintf(hdr, sizeof hdr, "{\"format\":\"pie-columns\",\"version\":1,\"rows\":%lld,\"users\":%d}\n", c->n, c->n_users);
    return write_file(c, base + "/header.json", hdr, (size_t)len);
}

int pie_load_columns_dir(pie_ctx* c, const char* dir)
{
    if (!c || !dir) return PIE_E_INVAL;
    const std::string base(dir);
    FILE* f = fopen((base + "/header.json").c_str(), "r");
    if (!f) return fail(c, PIE_E_INVAL, "no header.json under %s", dir);
    char hdr[512] = {0};
    const size_t got = fread(hdr, 1, sizeof hdr - 1, f);
    fclose(f);
    (void)got;
    long long rows = -1;
    int users = -1, version = -1;
    const char* pr = strstr(hdr, "\"rows\":");
    const char* pu = strstr(hdr, "\"users\":");
    const char* pv = strstr(hdr, "\"version\":");
    if (!strstr(hdr, "\"pie-columns\"") || !pr || !pu || !pv) return fail(c, PIE_E_INVAL, "%s/header.json is not a pie-columns header", dir);
    rows = atoll(pr + 7);
    users = atoi(pu + 8);
    version = atoi(pv + 10);
    if (version != 1 || rows < 0 || users < 1) return fail(c, PIE_E_INVAL, "unsupported header in %s (version %d)", dir, version);
    const size_t n = (size_t)rows;
    const char* names[4] = {"/start.i64", "/end.i64", "/user.i32", "/disc.i32"};
    const size_t width[4] = {8, 8, 4, 4};
    void* maps[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = PIE_OK;
    for (int k = 0; k < 4 && rc == PIE_OK; ++k) {
        const int fd = open((base + names[k]).c_str(), O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0 || (size_t)st.st_size != n * width[k]) {
            if (fd >= 0) close(fd);
            rc = fail(c, PIE_E_INVAL, "%s%s missing or not %zu bytes", dir, names[k], n * width[k]);
            break;
        }
        if (n) {
            maps[k] = mmap(nullptr, n * width[k], PROT_READ, MAP_PRIVATE, fd, 0);
            if (maps[k] == MAP_FAILED) { maps[k] = nullptr; rc = fail(c, PIE_E_NOMEM, "mmap of %s%s failed", dir, names[k]); }
        }
        close(fd);
    }
    if (rc == PIE_OK)
        rc = pie_load_columns(c, (const int64_t*)maps[0], (const int64_t*)maps[1], (const int32_t*)maps[2], (const int32_t*)maps[3], n, users);
    for (int k = 0; k < 4; ++k)
        if (maps[k]) munmap(maps[k], n * width[k]);
    return rc;
}

int pie_read_columns(pie_ctx* c, int64_t* start, int64_t* end, int32_t* user, int32_t* disc, size_t n)
{
    if (!c) return PIE_E_INVAL;
    if ((long long)n > c->n) return fail(c, PIE_E_INVAL, "asked for %zu rows, table has %lld", n, c->n);
    PIE_HIP(c, hipSetDevice(c->device));
    if (n) {
        if (start) PIE_HIP(c, hipMemcpyAsync(start, c->d_start, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (end) PIE_HIP(c, hipMemcpyAsync(end, c->d_end, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (user) PIE_HIP(c, hipMemcpyAsync(user, c->d_user, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (disc) PIE_HIP(c, hipMemcpyAsync(disc, c->d_disc, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

// pie_set_end applies its elements in array order, so of the elements that name one row only the last one counts.  k_set_end
// gives every element a thread of its own and orders nothing between them: the repeats are resolved here, on the host, and the
// kernel only ever sees distinct rows.  keep[i] = 1 iff no later element names rows[i].  A call whose rows strictly ascend or
// strictly descend has no repeats (one pass, no memory); any other goes through an open-addressed table of positions, at
// most half full, sized by k alone (`slots` is scratch the caller keeps between calls).  -> false: out of memory.
static bool set_end_last_writers(const int32_t* rows, size_t k, uint8_t* keep, std::vector<size_t>& slots)
{
    if (k == 0) return true;
    size_t up = 0, down = 0; // counted, not tested element by element: the loop has no branch and vectorises
    for (size_t i = 1; i < k; ++i) {
        up += rows[i - 1] < rows[i] ? 1 : 0;
        down += rows[i - 1] > rows[i] ? 1 : 0;
    }
    memset(keep, 1, k);
    if (up == k - 1 || down == k - 1) return true;
    int bits = 4;
    while (bits < 62 && ((size_t)1 << bits) < 2 * k) ++bits;
    const size_t n_slots = (size_t)1 << bits, mask = n_slots - 1, none = ~(size_t)0;
    try {
        slots.assign(n_slots, none);
    } catch (...) {
        return false;
    }
    size_t* const tab = slots.data();
    for (size_t i = 0; i < k; ++i) {
        const int32_t r = rows[i];
        size_t at = (size_t)(((uint64_t)(uint32_t)r * 0x9E3779B97F4A7C15ULL) >> (64 - bits));
        while (tab[at] != none && rows[tab[at]] != r) at = (at + 1) & mask;
        if (tab[at] != none) keep[tab[at]] = 0; // an earlier element on the same row: this one overrides it
        tab[at] = i;
    }
    return true;
}

int pie_set_end_last_writers(const int32_t* rows, size_t k, uint8_t* keep_out)
{
    if (k && (!rows || !keep_out)) return PIE_E_INVAL;
    std::vector<size_t> slots;
    return set_end_last_writers(rows, k, keep_out, slots) ? PIE_OK : PIE_E_NOMEM;
}

// [new_end kept | rows kept] of the elements with keep[i] set, in array order, into a staging area; -> their number
static size_t set_end_stage(char* dst, const int32_t* rows, const int64_t* new_end, size_t k, const uint8_t* keep, size_t n_kept)
{
    if (n_kept == k) {
        memcpy(dst, new_end, k * 8);
        memcpy(dst + k * 8, rows, k * 4);
        return k;
    }
    int64_t* e = reinterpret_cast<int64_t*>(dst);
    int32_t* r = reinterpret_cast<int32_t*>(dst + n_kept * 8);
    size_t j = 0;
    for (size_t i = 0; i < k; ++i)
        if (keep[i]) {
            e[j] = new_end[i];
            r[j] = rows[i];
            ++j;
        }
    return j;
}

// pie_set_end and pie_shard_set_end behind their own checks: ids[] are local rows, or (global) global rows the kernel looks up
// in the row map.  Equal global rows are equal local rows, so the repeats are resolved over the ids as they come: a row named
// more than once takes the value of its last element (the header's rule), the others are left out here.
static int set_end_apply(pie_ctx* c, const int32_t* ids, const int64_t* new_end, size_t k_given, bool global)
{
    try {
        c->set_end_keep.resize(k_given);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu touches", k_given);
    }
    const uint8_t* keep = c->set_end_keep.data();
    if (!set_end_last_writers(ids, k_given, c->set_end_keep.data(), c->set_end_slots)) return fail(c, PIE_E_NOMEM, "no memory for %zu touches", k_given);
    size_t k = 0;
    for (size_t i = 0; i < k_given; ++i) k += keep[i];
    PIE_HIP(c, hipSetDevice(c->device));
    queue_forget(c); // a touch or a tombstone can move a row into or out of the held queue
    hot_reserve(c, (long long)k_given); // the bound counts every element: never less than the rows that can move to the delta
    // staged like the append path: one upload of [new_end k | ids k], one kernel (end + both keys + mirrors), one wait or none
    Staged st{};
    int rc = stage_mutation(c, k * 12 + 64, mutation_queued(c), &st);
    if (rc) return rc;
    set_end_stage(st.h, ids, new_end, k_given, keep, k);
    hipStream_t s = c->stream;
    PIE_HIP(c, hipMemcpyAsync(st.d, st.h, k * 12, hipMemcpyHostToDevice, s));
    const int* d_ids = reinterpret_cast<const int*>(st.d + k * 8);
    const long long* d_new_end = reinterpret_cast<const long long*>(st.d);
    const dim3 grid((unsigned)((k + 255) / 256)); // a thread per element
    if (global)
        hipLaunchKernelGGL(k_shard_set_end, grid, dim3(256), 0, s, c->d_end, d_ids, d_new_end, (long long)k, (const int*)c->d_shard_rows, c->n,
                           c->d_key, c->key_base, c->key_shift, c->d_fkey, c->fkey_base, c->fkey_shift, ord_mirror_of(c), hot_mirror_of(c));
    else
        hipLaunchKernelGGL(k_set_end, grid, dim3(256), 0, s, c->d_end, d_ids, d_new_end, (long long)k, c->n, c->d_key, c->key_base,
                           c->key_shift, c->d_fkey, c->fkey_base, c->fkey_shift, ord_mirror_of(c), hot_mirror_of(c));
    PIE_HIP(c, hipGetLastError());
    c->key_dirty = true;
    if (st.a) return stage_queued(c, st); // the ids were checked by the caller: nothing to read back
    PIE_HIP(c, hipStreamSynchronize(s));
    if (c->ord.h_stale && *(volatile unsigned int*)c->ord.h_stale) { // a row the run does not hold is live again
        *c->ord.h_stale = 0;
        ord_invalidate(c);
    }
    return PIE_OK;
}

int pie_set_end(pie_ctx* c, const int32_t* rows, const int64_t* new_end, size_t k_given)
{
    if (!c) return PIE_E_INVAL;
    if (k_given == 0) return PIE_OK;
    if (!rows || !new_end) return fail(c, PIE_E_INVAL, "NULL pointer");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "table change while a scan is in flight");
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    for (size_t i = 0; i < k_given; ++i)
        if (rows[i] < 0 || rows[i] >= c->n) return fail(c, PIE_E_INVAL, "row %d outside the table", rows[i]);
    return set_end_apply(c, rows, new_end, k_given, false);
}

int pie_delete_user(pie_ctx* c, int32_t user, int32_t* rows_out, size_t cap, size_t* n_deleted)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    if (c->n == 0 || user < 0 || user >= c->n_users) return PIE_OK; // unknown / falsy id: no-op (sessionStore.js:56-58)
    // the rows are tombstoned even when rows_out is too small to list them (PIE_E_CAPACITY then tells the count)
    return row_list(c, kOneUser, false, (long long)user, 0, rows_out, cap, n_deleted, false);
}

int pie_delete_users_plan(const int32_t* users, size_t k, int32_t n_users, uint64_t* bits_out, uint8_t* first_out)
{
    if (k && (!users || !first_out)) return PIE_E_INVAL;
    if (n_users > 0 && !bits_out) return PIE_E_INVAL;
    const size_t words = n_users > 0 ? ((size_t)n_users + 63) / 64 : 0;
    for (size_t w = 0; w < words; ++w) bits_out[w] = 0;
    for (size_t i = 0; i < k; ++i) {
        const int32_t u = users[i];
        first_out[i] = 0;
        if (u < 0 || u >= n_users) continue;
        const uint64_t bit = 1ull << (u & 63);
        if (bits_out[u >> 6] & bit) continue; // named before: the earlier element has the count
        bits_out[u >> 6] |= bit;
        first_out[i] = 1;
    }
    return PIE_OK;
}

// pie_delete_users / pie_shard_delete_users behind their own checks: users[] are the context's own (local) ids, anything outside
// [0, n_users) is skipped.  Leaves the ascending list in slot 0's out_idx (as global rows if to_global) and its length in
// *m_out; per_user_out was zeroed by the caller.  Host side as run_row_list<1>: same workspace, same waits.
static int delete_users_run(pie_ctx* c, const int32_t* users, size_t k, bool to_global, size_t* m_out, int32_t* per_user_out)
{
    *m_out = 0;
    const size_t words = ((size_t)c->n_users + 63) / 64;
    std::vector<uint64_t> bits;
    std::vector<uint8_t> first;
    std::vector<int32_t> ids;
    try {
        bits.resize(words);
        first.resize(k);
        if (pie_delete_users_plan(users, k, c->n_users, bits.data(), first.data()) != PIE_OK) return fail(c, PIE_E_INVAL, "bad user list");
        for (size_t w = 0; w < words; ++w) // the distinct valid ids, ascending
            for (uint64_t b = bits[w]; b; b &= b - 1) ids.push_back((int32_t)(w * 64 + (size_t)__builtin_ctzll(b)));
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu user ids", k);
    }
    const size_t d = ids.size();
    if (d == 0) return PIE_OK; // no id the table knows: as k calls that each found the falsy-id guard
    bool empty; // never: both callers return before this on a table of no rows
    int rc = list_enter(c, kRefuseTurns | kSyncAll | kDropSlot0, &empty);
    if (rc || empty) return rc;
    hipStream_t s = c->stream;
    Slot& sl = c->slot[0];
    // one upload of [bitmap | distinct ids], the per-id counters behind them
    const size_t bits_bytes = words * 8, ids_bytes = d * 4;
    Staged st{};
    rc = stage_mutation(c, bits_bytes + 2 * ids_bytes, false, &st);
    if (rc) return rc;
    memcpy(st.h, bits.data(), bits_bytes);
    memcpy(st.h + bits_bytes, ids.data(), ids_bytes);
    PIE_HIP(c, hipMemcpyAsync(st.d, st.h, bits_bytes + ids_bytes, hipMemcpyHostToDevice, s));
    const unsigned int* d_bits = reinterpret_cast<const unsigned int*>(st.d); // little-endian: bit u of the 64-bit words = bit u of these
    const int* d_ids = reinterpret_cast<const int*>(st.d + bits_bytes);
    unsigned int* d_cnt = reinterpret_cast<unsigned int*>(st.d + bits_bytes + ids_bytes);
    if (per_user_out) PIE_HIP(c, hipMemsetAsync(d_cnt, 0, ids_bytes, s));
    const int blocks = c->plan_blocks[0];
    const long long rpb = c->plan_rows[0]; // a multiple of the streaming tile: every wave's quarter starts 16-byte aligned
    const int n_waves = blocks * kK1Waves;
    hipLaunchKernelGGL(k_users_pass<false>, dim3(blocks), dim3(kK1Threads), 0, s, c->d_end, (const int*)c->d_user, c->n, rpb, d_bits, c->n_users,
                       sl.blk_count, (const long long*)nullptr, (int*)nullptr, 0LL, (lkey_t*)nullptr, (fkey_t*)nullptr, OrdMirror{}, HotMirror{});
    hipLaunchKernelGGL(k_block_prefix_wide, dim3(1), dim3(1024), 0, s, sl.blk_count, n_waves, c->d_blk_off, &c->d_summary->m,
                       (HostSummary*)nullptr, 0ull);
    hipLaunchKernelGGL(k_users_pass<true>, dim3(blocks), dim3(kK1Threads), 0, s, c->d_end, (const int*)c->d_user, c->n, rpb, d_bits, c->n_users,
                       (int*)nullptr, (const long long*)c->d_blk_off, sl.out_idx, c->cap_rows, c->d_key, c->d_fkey, ord_mirror_of(c), hot_mirror_of(c));
    if (per_user_out)
        hipLaunchKernelGGL(k_users_tally, dim3(capped_grid(c, (size_t)c->n)), dim3(256), 0, s, (const int*)sl.out_idx,
                           (const unsigned long long*)&c->d_summary->m, c->cap_rows, (const int*)c->d_user, d_ids, (int)d, d_cnt);
    PIE_HIP(c, hipGetLastError());
    char* h_cnt = st.h + bits_bytes + ids_bytes;
    if (per_user_out) PIE_HIP(c, hipMemcpyAsync(h_cnt, d_cnt, ids_bytes, hipMemcpyDeviceToHost, s)); // list_total waits for it too
    size_t m = 0;
    rc = list_total(c, s, &m);
    if (rc) return rc;
    *m_out = m;
    if (per_user_out) { // an id's count goes to its first occurrence; the later ones keep their 0
        const unsigned int* cnt = reinterpret_cast<const unsigned int*>(h_cnt);
        for (size_t i = 0; i < k; ++i)
            if (first[i]) per_user_out[i] = (int32_t)cnt[std::lower_bound(ids.begin(), ids.end(), users[i]) - ids.begin()];
    }
    if (to_global && m) {
        hipLaunchKernelGGL(k_shard_rows_to_global, dim3(capped_grid(c, m)), dim3(256), 0, s, (const int*)sl.out_idx, sl.out_idx, (long long)m,
                           (const int*)c->d_shard_rows, c->n);
        PIE_HIP(c, hipGetLastError());
    }
    return PIE_OK;
}

// the list delete_users_run left on the device -> rows_out (m entries; more than `cap` are refused, tombstoned all the same)
static int delete_users_copy(pie_ctx* c, int32_t* rows_out, size_t cap, size_t m)
{
    return list_copy_out(c, c->slot[0].out_idx, m, rows_out, cap, "list");
}

int pie_delete_users(pie_ctx* c, const int32_t* users, size_t k, int32_t* rows_out, size_t cap, size_t* n_deleted, int32_t* per_user_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    if (k == 0) return PIE_OK;
    if (!users) return fail(c, PIE_E_INVAL, "NULL user list");
    if (per_user_out) memset(per_user_out, 0, k * 4);
    if (c->n == 0) return PIE_OK;
    size_t m = 0;
    int rc = delete_users_run(c, users, k, false, &m, per_user_out);
    if (rc) return rc;
    if (n_deleted) *n_deleted = m;
    // the rows are tombstoned even when rows_out is too small to list them (PIE_E_CAPACITY then tells the count)
    return delete_users_copy(c, rows_out, cap, m);
}

// The three maintenance lists behind their plain and their shard entries.  `mapped`: the context is a shard whose row map
// covers its rows (the entry checked that): the list holds GLOBAL rows; want_local as in run_row_list.
static int prune_impl(pie_ctx* c, int64_t cutoff, int32_t* rows_out, size_t cap, size_t* n_pruned, bool mapped, bool want_local)
{
    if (n_pruned) *n_pruned = 0;
    if (c->n == 0) return PIE_OK;
    return row_list(c, kPrune, mapped, (long long)cutoff, 0, rows_out, cap, n_pruned, want_local);
}

static int retention_check(pie_ctx* c, int32_t months, int64_t tz_offset_ms)
{
    if (months < -32768 || months > 32767) return fail(c, PIE_E_INVAL, "months outside int16");
    if (tz_offset_ms % 60000 != 0 || tz_offset_ms > 86400000LL || tz_offset_ms < -86400000LL)
        return fail(c, PIE_E_INVAL, "tz offset must be whole minutes within a day");
    return PIE_OK;
}

static int retention_impl(pie_ctx* c, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t* rows_out, size_t cap, size_t* n_purged,
                          bool mapped, bool want_local)
{
    if (n_purged) *n_purged = 0;
    const int rc = retention_check(c, months, tz_offset_ms);
    if (rc) return rc;
    if (c->n == 0) return PIE_OK;
    return row_list(c, kRetention, mapped, (long long)now, retention_pack(months, tz_offset_ms / 60000), rows_out, cap, n_purged, want_local);
}

static int retention_tz_check(pie_ctx* c, int32_t months, const int64_t* transitions_utc_ms, const int64_t* offsets_ms, int32_t n_transitions)
{
    if (months < -32768 || months > 32767) return fail(c, PIE_E_INVAL, "months outside int16");
    if (n_transitions < 0 || n_transitions > 65536 || !offsets_ms || (n_transitions > 0 && !transitions_utc_ms))
        return fail(c, PIE_E_INVAL, "bad transition table");
    const int n = n_transitions;
    for (int i = 0; i <= n; ++i)
        if (offsets_ms[i] > 2 * 86400000LL || offsets_ms[i] < -2 * 86400000LL) return fail(c, PIE_E_INVAL, "offset %d outside two days", i);
    // transitions ascending, and ascending on the old offset's local clock too (what the local -> UTC search relies on)
    for (int i = 1; i < n; ++i)
        if (transitions_utc_ms[i] <= transitions_utc_ms[i - 1] || transitions_utc_ms[i] + offsets_ms[i] <= transitions_utc_ms[i - 1] + offsets_ms[i - 1])
            return fail(c, PIE_E_INVAL, "transitions must ascend (entry %d)", i);
    return PIE_OK;
}

static int retention_tz_impl(pie_ctx* c, int64_t now, int32_t months, const int64_t* transitions_utc_ms, const int64_t* offsets_ms,
                             int32_t n_transitions, int32_t* rows_out, size_t cap, size_t* n_purged, bool mapped, bool want_local);

int pie_prune_before(pie_ctx* c, int64_t cutoff, int32_t* rows_out, size_t cap, size_t* n_pruned)
{
    if (!c) return PIE_E_INVAL;
    return prune_impl(c, cutoff, rows_out, cap, n_pruned, false, false);
}

int pie_retention_purge(pie_ctx* c, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t* rows_out, size_t cap,
                        size_t* n_purged)
{
    if (!c) return PIE_E_INVAL;
    return retention_impl(c, now, months, tz_offset_ms, rows_out, cap, n_purged, false, false);
}

int pie_retention_purge_tz(pie_ctx* c, int64_t now, int32_t months, const int64_t* transitions_utc_ms, const int64_t* offsets_ms,
                           int32_t n_transitions, int32_t* rows_out, size_t cap, size_t* n_purged)
{
    if (!c) return PIE_E_INVAL;
    return retention_tz_impl(c, now, months, transitions_utc_ms, offsets_ms, n_transitions, rows_out, cap, n_purged, false, false);
}

static int retention_tz_impl(pie_ctx* c, int64_t now, int32_t months, const int64_t* transitions_utc_ms, const int64_t* offsets_ms,
                             int32_t n_transitions, int32_t* rows_out, size_t cap, size_t* n_purged, bool mapped, bool want_local)
{
    if (n_purged) *n_purged = 0;
    int rc = retention_tz_check(c, months, transitions_utc_ms, offsets_ms, n_transitions);
    if (rc) return rc;
    const int n = n_transitions;
    if (c->n == 0) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    // the table on the device: [n, months, T[n], L[n], off[n + 1]] through the context's staging block
    const size_t words = 2 + (size_t)n * 2 + (size_t)n + 1;
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    rc = sync_all(c); // the staging block is shared with appends / touches
    if (rc) return rc;
    rc = ensure_stage(c, words * 8);
    if (rc) return rc;
    long long* h = reinterpret_cast<long long*>(c->h_stage);
    h[0] = n;
    h[1] = months;
    for (int i = 0; i < n; ++i) {
        h[2 + i] = transitions_utc_ms[i];
        h[2 + n + i] = transitions_utc_ms[i] + offsets_ms[i];
    }
    for (int i = 0; i <= n; ++i) h[2 + 2 * n + i] = offsets_ms[i];
    PIE_HIP(c, hipMemcpyAsync(c->d_stage, c->h_stage, words * 8, hipMemcpyHostToDevice, c->stream));
    const long long zone_table = (long long)(uintptr_t)c->d_stage; // kRetentionTz's `b` is a device address (list_match reads it back)
    return row_list(c, kRetentionTz, mapped, (long long)now, zone_table, rows_out, cap, n_purged, want_local);
}

int pie_set_disciplines(pie_ctx* c, uint64_t mask, int32_t n_disc)
{
    if (!c) return PIE_E_INVAL;
    if (n_disc < 0 || n_disc > 64) return fail(c, PIE_E_INVAL, "n_disc %d outside [0, 64]", n_disc);
    c->disc_mask = mask;
    c->n_disc = n_disc;
    return PIE_OK;
}

int pie_scan_device(pie_ctx* c, int64_t now, int64_t cutoff, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = run_scan(c, now, cutoff);
    if (m_out) *m_out = c->res ? (size_t)c->res->last.m : 0;
    return rc;
}

int pie_scan_begin(pie_ctx* c, int64_t now, int64_t cutoff)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    PIE_HIP(c, hipSetDevice(c->device));
    return scan_begin(c, now, cutoff);
}

int pie_scan_finish(pie_ctx* c, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = scan_finish(c);
    if (m_out) *m_out = c->res ? (size_t)c->res->last.m : 0;
    return rc;
}

int pie_scan_begin_packed(pie_ctx* c, int64_t now, int64_t cutoff, void* dst_i32, size_t u_pad, size_t idx_cap)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    if (!dst_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad message destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    return scan_begin(c, now, cutoff, (int*)dst_i32, (int)u_pad, (long long)idx_cap);
}

int pie_scan_begin_packed2(pie_ctx* c, int64_t now, int64_t cutoff, void* dst_i32, size_t u_pad, size_t idx_cap, void* counts_dst_i32)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    if (!dst_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad message destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    return scan_begin(c, now, cutoff, (int*)dst_i32, (int)u_pad, (long long)idx_cap, (int*)counts_dst_i32);
}

int pie_scan_finish_packed(pie_ctx* c, size_t* m_out, int* ready_out)
{
    if (!c) return PIE_E_INVAL;
    if (ready_out) *ready_out = 0;
    PIE_HIP(c, hipSetDevice(c->device));
    Slot* slp = oldest_in_flight(c);
    if (!slp) return fail(c, PIE_E_STATE, "pie_scan_finish_packed without pie_scan_begin_packed");
    if (!slp->msg) return fail(c, PIE_E_STATE, "the oldest scan in flight was not begun with pie_scan_begin_packed");
    int rc = scan_finish(c);
    if (rc) return rc;
    Slot& sl = *c->res;
    if (m_out) *m_out = (size_t)sl.last.m;
    // K2 wrote the whole message iff it ran the fused form and no bucket outgrew the direct slots
    if (sl.msg_by_k2 && sl.last.n_small + sl.last.n_seg == 0) {
        if (ready_out) *ready_out = 1;
        return PIE_OK;
    }
    // the unfused K2 wrote neither destination; the fused one wrote the counts but not the rows of the outgrown buckets
    if (sl.msg_counts && !sl.msg_by_k2)
        PIE_HIP(c, hipMemcpyAsync(sl.msg_counts, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDefault, c->stream));
    return pie_pack_results_device(c, sl.msg, (size_t)sl.msg_u_pad, (size_t)sl.msg_cap);
}

int pie_scan_batch_begin(pie_ctx* c, const pie_query* queries, int n_q)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    return batch_begin(c, queries, n_q, 0, nullptr, 0, 0, 0, nullptr, 0);
}

int pie_scan_batch_begin_packed(pie_ctx* c, const pie_query* queries, int n_q, void* msg_i32, size_t msg_stride_words, size_t u_pad,
                                size_t idx_cap, void* counts_i32, size_t counts_stride_words)
{
    if (!c) return PIE_E_INVAL;
    if (!msg_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u || msg_stride_words < u_pad + 2 + idx_cap)
        return fail(c, PIE_E_INVAL, "bad message destination / u_pad < n_users / stride below u_pad + 2 + idx_cap");
    if (counts_i32 && counts_stride_words < (size_t)c->n_users) return fail(c, PIE_E_INVAL, "counts stride below n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    return batch_begin(c, queries, n_q, 1, (int*)msg_i32, (long long)msg_stride_words, (int)u_pad, (long long)idx_cap, (int*)counts_i32,
                       (long long)counts_stride_words);
}

int pie_scan_batch_begin_union(pie_ctx* c, const pie_query* queries, int n_q, void* msg_i32, size_t u_pad, size_t cap)
{
    if (!c) return PIE_E_INVAL;
    if (!msg_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad union destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    return batch_begin(c, queries, n_q, 2, (int*)msg_i32, 0, (int)u_pad, (long long)cap, nullptr, 0);
}

// No further begin is coming for now: the tails that were waiting for a ride in their lane's next launch are queued at once,
// side by side, instead of one by one as their batches are finished (the end of a burst: 20 batches on three lanes drained
// through three tail launches in a row).
int pie_scan_batch_flush(pie_ctx* c)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    // Oldest first, every batch of the lane whose tail still waits — not only the youngest: a batch that only falls back queues no
    // launch, so the batch before it keeps its tail until its finish, and tails must run in the order of their batches (a tail
    // zeroes the span of the batch after the next: found by the differential fuzz, which flushed the third batch of a lane
    // while the first one's tail was still waiting behind such a batch).
    for (int lane = 0; lane < kLaneMax; ++lane) {
        for (int age = c->lane_flight[lane]; age >= 1; --age) {
            BatchSlot& b = c->bslot[lane * kBatchSlots + (c->lane_next[lane] + kBatchSlots - age) % kBatchSlots];
            if (b.in_flight && b.k2_pending && !b.ordered && !b.unsupported) launch_batch_k2(c, b, b.stream ? b.stream : c->stream);
        }
    }
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

int pie_scan_batch_finish_packed(pie_ctx* c, size_t* m_out, int* ready_out)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = batch_finish(c, ready_out);
    if (rc) return rc;
    if (m_out)
        for (int q = 0; q < c->bres->n_q; ++q) m_out[q] = (size_t)c->bres->last[q].m;
    return PIE_OK;
}

int pie_scan_batch_finish(pie_ctx* c, size_t* m_out) { return pie_scan_batch_finish_packed(c, m_out, nullptr); }

int pie_scan_batch(pie_ctx* c, const pie_query* queries, int n_q, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    int rc = pie_scan_batch_begin(c, queries, n_q);
    if (rc) return rc;
    return pie_scan_batch_finish(c, m_out);
}

int pie_scan_wide_begin(pie_ctx* c, const pie_query* queries, int n_q)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    return wide_begin(c, queries, n_q);
}

int pie_scan_wide_finish(pie_ctx* c, size_t* m_out, size_t m_cap, int* n_q_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_q_out) *n_q_out = 0;
    PIE_HIP(c, hipSetDevice(c->device));
    return wide_finish(c, m_out, m_cap, n_q_out);
}

int pie_scan_wide_begin_union(pie_ctx* c, const pie_query* queries, int n_q, void* msg_i32, size_t u_pad, size_t cap)
{
    if (!c) return PIE_E_INVAL;
    if (!msg_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad union destination / u_pad < n_users");
    if (cap > ((size_t)1 << 40)) return fail(c, PIE_E_INVAL, "cap %zu is not a row capacity", cap);
    PIE_HIP(c, hipSetDevice(c->device));
    return wide_begin(c, queries, n_q, (int*)msg_i32, (int)u_pad, (long long)cap);
}

int pie_scan_wide_finish_packed(pie_ctx* c, size_t* m_out, size_t m_cap, int* n_q_out, int* ready_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_q_out) *n_q_out = 0;
    int ready = 0;
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = wide_finish(c, m_out, m_cap, n_q_out, &ready);
    if (ready_out) *ready_out = rc == PIE_OK ? ready : 0;
    return rc;
}

int pie_batch_union_wide_device_ptrs(pie_ctx* c, void** uoff_dev, void** rows_dev, void** masks_dev, int* words_out, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    if (uoff_dev) *uoff_dev = nullptr;
    if (rows_dev) *rows_dev = nullptr;
    if (masks_dev) *masks_dev = nullptr;
    if (words_out) *words_out = 0;
    if (mu_out) *mu_out = 0;
    BatchSlot* b = nullptr;
    if (int rc = wide_union_of(c, &b)) return rc;
    if (uoff_dev) *uoff_dev = b->uoff;
    if (rows_dev) *rows_dev = b->urows;
    if (masks_dev) *masks_dev = b->w->umask;
    if (words_out) *words_out = b->w->words;
    if (mu_out) *mu_out = (size_t)b->mu;
    return PIE_OK;
}

int pie_batch_read_union_wide(pie_ctx* c, int64_t* uoff_out, int32_t* rows_out, uint64_t* masks_out, size_t cap, int* words_out, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    if (mu_out) *mu_out = 0;
    if (words_out) *words_out = 0;
    PIE_HIP(c, hipSetDevice(c->device));
    BatchSlot* b = nullptr;
    if (int rc = wide_union_of(c, &b)) return rc;
    hipStream_t a = c->stream;
    const size_t mu = (size_t)b->mu, words = (size_t)b->w->words;
    if (mu_out) *mu_out = mu;
    if (words_out) *words_out = (int)words;
    if ((rows_out || masks_out) && mu > cap) return fail(c, PIE_E_CAPACITY, "cap %zu < union rows %zu", cap, mu);
    if (uoff_out) PIE_HIP(c, hipMemcpyAsync(uoff_out, b->uoff, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToHost, a));
    if (rows_out && mu) PIE_HIP(c, hipMemcpyAsync(rows_out, b->urows, mu * 4, hipMemcpyDeviceToHost, a));
    if (masks_out && mu) PIE_HIP(c, hipMemcpyAsync(masks_out, b->w->umask, mu * words * 8, hipMemcpyDeviceToHost, a));
    PIE_HIP(c, hipStreamSynchronize(a));
    return PIE_OK;
}

int pie_batch_pack_union_wide_device(pie_ctx* c, void* dst_i32, size_t u_pad, size_t cap)
{
    if (!c) return PIE_E_INVAL;
    if (!dst_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad union destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    BatchSlot* b = nullptr;
    if (int rc = wide_union_of(c, &b)) return rc;
    const size_t words = (size_t)b->w->words;
    const size_t k = (size_t)b->mu < cap ? (size_t)b->mu : cap;
    const size_t total = u_pad + 2 + k * (1 + 2 * words);
    size_t grid = (total + 255) / 256;
    if (grid > (size_t)c->n_cus * 8) grid = (size_t)c->n_cus * 8;
    hipLaunchKernelGGL(k_wide_pack, dim3((unsigned)(grid ? grid : 1)), dim3(256), 0, c->stream, c->n_users, (int)u_pad, (const long long*)b->uoff,
                       (const int*)b->urows, (const unsigned long long*)b->w->umask, (int)words, (long long)cap, (int*)dst_i32);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

int pie_batch_union_device_ptrs(pie_ctx* c, void** uoff_dev, void** rows_dev, void** mask_lo_dev, void** mask_hi_dev, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    if (uoff_dev) *uoff_dev = nullptr;
    if (rows_dev) *rows_dev = nullptr;
    if (mask_lo_dev) *mask_lo_dev = nullptr;
    if (mask_hi_dev) *mask_hi_dev = nullptr;
    if (mu_out) *mu_out = 0;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (c->bres->wide) return fail(c, PIE_E_STATE, "the last batch is wide: use pie_batch_union_wide_device_ptrs");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    const BatchSlot& b = *c->bres;
    if (!b.union_ok) return PIE_OK; // queries fell back / the batch ran on the ordered run: per-query lists only
    if (uoff_dev) *uoff_dev = b.uoff;
    if (rows_dev) *rows_dev = b.urows;
    if (mask_lo_dev) *mask_lo_dev = b.umlo;
    if (mask_hi_dev) *mask_hi_dev = b.n_q > 32 ? b.umhi : nullptr;
    if (mu_out) *mu_out = (size_t)b.mu;
    return PIE_OK;
}

int pie_batch_read_union(pie_ctx* c, int64_t* uoff_out, int32_t* rows_out, uint64_t* masks_out, size_t cap, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    if (mu_out) *mu_out = 0;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (c->bres->wide) return fail(c, PIE_E_STATE, "the last batch is wide: use pie_batch_read_union_wide");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    const BatchSlot& b = *c->bres;
    if (!b.union_ok) return fail(c, PIE_E_STATE, "this batch has no union result (queries fell back to the general path, or it ran on the ordered run): read the per-query results");
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t a = c->stream;
    const size_t mu = (size_t)b.mu;
    if (mu_out) *mu_out = mu;
    if (uoff_out) PIE_HIP(c, hipMemcpyAsync(uoff_out, b.uoff, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToHost, a));
    if ((rows_out || masks_out) && mu > cap) {
        PIE_HIP(c, hipStreamSynchronize(a));
        return fail(c, PIE_E_CAPACITY, "cap %zu < union rows %zu", cap, mu);
    }
    if (rows_out && mu) PIE_HIP(c, hipMemcpyAsync(rows_out, b.urows, mu * 4, hipMemcpyDeviceToHost, a));
    std::vector<uint32_t> lo, hi;
    if (masks_out && mu) {
        lo.resize(mu);
        PIE_HIP(c, hipMemcpyAsync(lo.data(), b.umlo, mu * 4, hipMemcpyDeviceToHost, a));
        if (b.n_q > 32) {
            hi.resize(mu);
            PIE_HIP(c, hipMemcpyAsync(hi.data(), b.umhi, mu * 4, hipMemcpyDeviceToHost, a));
        }
    }
    PIE_HIP(c, hipStreamSynchronize(a));
    if (masks_out)
        for (size_t i = 0; i < mu; ++i) masks_out[i] = (uint64_t)lo[i] | (hi.empty() ? 0ull : ((uint64_t)hi[i] << 32));
    return PIE_OK;
}

int pie_batch_result_device_ptrs(pie_ctx* c, int qi, void** counts_dev, void** offsets_dev, void** idx_dev)
{
    if (!c) return PIE_E_INVAL;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    if (qi < 0 || qi >= c->bres->n_q) return fail(c, PIE_E_INVAL, "query %d outside the batch of %d", qi, c->bres->n_q);
    PIE_HIP(c, hipSetDevice(c->device));
    if (c->bres->wide) {
        int rc = wide_need_list(c, *c->bres, qi);
        if (rc) return rc;
        const WideSlot::List& l = c->bres->w->lists[qi];
        if (counts_dev) *counts_dev = l.counts;
        if (offsets_dev) *offsets_dev = l.offsets;
        if (idx_dev) *idx_dev = l.idx;
        return PIE_OK;
    }
    int rc = batch_need_list(c, *c->bres, qi);
    if (rc) return rc;
    const long long us = batch_users_stride(c);
    if (counts_dev) *counts_dev = c->bres->counts_ord + (long long)qi * us;
    if (offsets_dev) *offsets_dev = c->bres->offsets + (long long)qi * us;
    if (idx_dev) *idx_dev = c->bres->idx_of[qi];
    return PIE_OK;
}

int pie_batch_read_user_feed(pie_ctx* c, int qi, int32_t user, int32_t* idx_out, size_t idx_cap, size_t* k_out)
{
    if (!c) return PIE_E_INVAL;
    if (k_out) *k_out = 0;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    BatchSlot& b = *c->bres;
    if (qi < 0 || qi >= b.n_q) return fail(c, PIE_E_INVAL, "query %d outside the batch of %d", qi, b.n_q);
    if (user < 0 || user >= c->n_users) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    if (b.wide && b.union_part && !b.w->fallback[qi] && !b.w->lists[qi].ok) {
        // straight from the wide union: the user's (<= 64) union rows and their mask words, filtered by the query's bit
        const WideSlot& w = *b.w;
        long long off[2] = {0, 0};
        PIE_HIP(c, hipMemcpyAsync(off, b.uoff + user, sizeof off, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
        const size_t ku = (size_t)(off[1] - off[0]);
        if (ku == 0) return PIE_OK;
        std::vector<int> rows(ku);
        std::vector<unsigned long long> masks(ku * (size_t)w.words);
        PIE_HIP(c, hipMemcpyAsync(rows.data(), b.urows + off[0], ku * 4, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipMemcpyAsync(masks.data(), w.umask + (size_t)off[0] * w.words, ku * w.words * 8, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
        auto hit = [&](size_t i) { return ((masks[i * w.words + (qi >> 6)] >> (qi & 63)) & 1ull) != 0; };
        size_t k = 0;
        for (size_t i = 0; i < ku; ++i) k += hit(i) ? 1 : 0;
        if (k_out) *k_out = k;
        if (k == 0) return PIE_OK;
        if (!idx_out || k > idx_cap) return fail(c, PIE_E_CAPACITY, "idx_cap %zu < feed length %zu", idx_cap, k);
        size_t at = 0;
        for (size_t i = 0; i < ku; ++i)
            if (hit(i)) idx_out[at++] = rows[i];
        return PIE_OK;
    }
    if (!b.wide && b.union_ok && !b.list_ok[qi]) {
        // straight from the union: the user's (few) union rows, filtered by the query's bit — no per-query list is ever built
        long long off[2] = {0, 0};
        PIE_HIP(c, hipMemcpyAsync(off, b.uoff + user, sizeof off, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
        const size_t ku = (size_t)(off[1] - off[0]);
        if (ku == 0) return PIE_OK;
        int rows_s[1 << kUnionShiftMax];
        unsigned masks_s[1 << kUnionShiftMax];
        std::vector<int> rows_h;
        std::vector<unsigned> masks_h;
        int* rows = rows_s;
        unsigned* masks = masks_s;
        if (ku > (size_t)(1 << kUnionShiftMax)) { // a batch on the ordered run: a head user's union is as long as its live rows
            rows_h.resize(ku);
            masks_h.resize(ku);
            rows = rows_h.data();
            masks = masks_h.data();
        }
        PIE_HIP(c, hipMemcpyAsync(rows, b.urows + off[0], ku * 4, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipMemcpyAsync(masks, (qi >= 32 ? b.umhi : b.umlo) + off[0], ku * 4, hipMemcpyDeviceToHost, c->stream));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
        size_t k = 0;
        for (size_t i = 0; i < ku; ++i) k += (masks[i] >> (qi & 31)) & 1u;
        if (k_out) *k_out = k;
        if (k == 0) return PIE_OK;
        if (!idx_out || k > idx_cap) return fail(c, PIE_E_CAPACITY, "idx_cap %zu < feed length %zu", idx_cap, k);
        size_t at = 0;
        for (size_t i = 0; i < ku; ++i)
            if ((masks[i] >> (qi & 31)) & 1u) idx_out[at++] = rows[i];
        return PIE_OK;
    }
    void *dc = nullptr, *dof = nullptr, *di = nullptr;
    int rc = pie_batch_result_device_ptrs(c, qi, &dc, &dof, &di);
    if (rc) return rc;
    long long off[2] = {0, 0};
    PIE_HIP(c, hipMemcpyAsync(off, static_cast<long long*>(dof) + user, sizeof off, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    const size_t k = (size_t)(off[1] - off[0]);
    if (k_out) *k_out = k;
    if (k == 0) return PIE_OK;
    if (!idx_out || k > idx_cap) return fail(c, PIE_E_CAPACITY, "idx_cap %zu < feed length %zu", idx_cap, k);
    PIE_HIP(c, hipMemcpyAsync(idx_out, static_cast<int*>(di) + off[0], k * 4, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

int pie_batch_fetch_requests(pie_ctx* c, const int32_t* qi, const int32_t* user, size_t n_req, size_t cap_rows, int64_t* req_off_out,
                             int32_t* idx_out, int64_t* start_out, int64_t* end_out, int32_t* disc_out, size_t* total_out)
{
    if (!c) return PIE_E_INVAL;
    if (total_out) *total_out = 0;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    if (n_req == 0) return PIE_OK;
    if (!qi || !user || !req_off_out || n_req > (size_t)1 << 24) return fail(c, PIE_E_INVAL, "bad request list");
    BatchSlot& b = *c->bres;
    for (size_t i = 0; i < n_req; ++i)
        if (qi[i] < 0 || qi[i] >= b.n_q) return fail(c, PIE_E_INVAL, "request %zu: query %d outside the batch of %d", i, qi[i], b.n_q);
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (b.wide || !b.union_ok || !c->d_pay) {
        // a wide batch, a batch without a union (queries fell back, the ordered run) or a table without the payload column: request by request
        size_t total = 0;
        std::vector<int32_t> tmp;
        for (size_t i = 0; i < n_req; ++i) {
            req_off_out[i] = (int64_t)total;
            size_t k = 0;
            int rc = pie_batch_read_user_feed(c, qi[i], user[i], nullptr, 0, &k);
            if (rc != PIE_OK && rc != PIE_E_CAPACITY) return rc;
            if (k && idx_out && total + k <= cap_rows) {
                rc = pie_batch_read_user_feed(c, qi[i], user[i], idx_out + total, k, &k);
                if (rc) return rc;
                rc = pie_fetch_rows(c, idx_out + total, k, start_out ? start_out + total : nullptr, end_out ? end_out + total : nullptr, nullptr,
                                    disc_out ? disc_out + total : nullptr);
                if (rc) return rc;
            }
            total += k;
        }
        req_off_out[n_req] = (int64_t)total;
        if (total_out) *total_out = total;
        if (idx_out && total > cap_rows) return fail(c, PIE_E_CAPACITY, "cap_rows %zu < %zu rows", cap_rows, total);
        return PIE_OK;
    }
    // device staging: [qi n | user n | cnt n | off (n + 1) x 8 | idx cap | disc cap | start cap x 8 | end cap x 8]
    const size_t n4 = ((n_req + 3) / 4) * 4, cap4 = ((cap_rows + 3) / 4) * 4;
    const size_t bytes = n4 * 12 + (n4 + 4) * 8 + cap4 * 24 + 64;
    int rc = ensure_stage(c, bytes);
    if (rc) return rc;
    char* h = c->h_stage;
    char* d = c->d_stage;
    memcpy(h, qi, n_req * 4);
    memcpy(h + n4 * 4, user, n_req * 4);
    PIE_HIP(c, hipMemcpyAsync(d, h, n4 * 8, hipMemcpyHostToDevice, s));
    int* d_qi = reinterpret_cast<int*>(d);
    int* d_us = reinterpret_cast<int*>(d + n4 * 4);
    int* d_cnt = reinterpret_cast<int*>(d + n4 * 8);
    long long* d_off = reinterpret_cast<long long*>(d + n4 * 12);
    int* d_idx = reinterpret_cast<int*>(d + n4 * 12 + (n4 + 4) * 8);
    int* d_disc = d_idx + cap4;
    long long* d_start = reinterpret_cast<long long*>(d_disc + cap4);
    long long* d_end = d_start + cap4;
    const unsigned blocks = (unsigned)((n_req + 255) / 256);
    const unsigned* hi = b.n_q > 32 ? b.umhi : b.umlo;
    hipLaunchKernelGGL(k_req_count, dim3(blocks), dim3(256), 0, s, (int)n_req, d_qi, d_us, c->n_users, b.uoff, b.umlo, hi, d_cnt);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, d_cnt, (int)n_req, d_off, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_req_write, dim3(blocks), dim3(256), 0, s, (int)n_req, d_qi, d_us, c->n_users, b.uoff, b.urows, b.umlo, hi, d_off, c->d_pay,
                       c->d_end, (long long)cap_rows, d_idx, d_start, d_end, d_disc);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(req_off_out, d_off, (n_req + 1) * 8, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    const size_t total = (size_t)req_off_out[n_req];
    if (total_out) *total_out = total;
    if (idx_out && total > cap_rows) return fail(c, PIE_E_CAPACITY, "cap_rows %zu < %zu rows", cap_rows, total);
    if (total && idx_out) {
        PIE_HIP(c, hipMemcpyAsync(idx_out, d_idx, total * 4, hipMemcpyDeviceToHost, s));
        if (disc_out) PIE_HIP(c, hipMemcpyAsync(disc_out, d_disc, total * 4, hipMemcpyDeviceToHost, s));
        if (start_out) PIE_HIP(c, hipMemcpyAsync(start_out, d_start, total * 8, hipMemcpyDeviceToHost, s));
        if (end_out) PIE_HIP(c, hipMemcpyAsync(end_out, d_end, total * 8, hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipStreamSynchronize(s));
    }
    return PIE_OK;
}

int pie_batch_read_results(pie_ctx* c, int qi, int32_t* counts_out, int64_t* offsets_out, int32_t* idx_out, size_t idx_cap, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    void *dc = nullptr, *dof = nullptr, *di = nullptr;
    int rc = pie_batch_result_device_ptrs(c, qi, &dc, &dof, &di);
    if (rc) return rc;
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t a = c->stream;
    const size_t m = c->bres->wide ? (size_t)c->bres->w->m[qi] : (size_t)c->bres->last[qi].m;
    if (m_out) *m_out = m;
    if (counts_out) PIE_HIP(c, hipMemcpyAsync(counts_out, dc, (size_t)c->n_users * 4, hipMemcpyDeviceToHost, a));
    if (offsets_out) PIE_HIP(c, hipMemcpyAsync(offsets_out, dof, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToHost, a));
    if (idx_out && m > idx_cap) {
        PIE_HIP(c, hipStreamSynchronize(a));
        return fail(c, PIE_E_CAPACITY, "idx_cap %zu < selected rows %zu", idx_cap, m);
    }
    if (idx_out && m) PIE_HIP(c, hipMemcpyAsync(idx_out, di, m * 4, hipMemcpyDeviceToHost, a));
    PIE_HIP(c, hipStreamSynchronize(a));
    return PIE_OK;
}

int pie_read_results(pie_ctx* c, int32_t* counts_out, int64_t* offsets_out, int32_t* idx_out, size_t idx_cap, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    if (!c->res || !c->res->have_result) return fail(c, PIE_E_STATE, "no scan result on this context");
    PIE_HIP(c, hipSetDevice(c->device));
    Slot& sl = *c->res;
    hipStream_t a = c->stream;
    const size_t m = (size_t)sl.last.m;
    if (m_out) *m_out = m;
    if (counts_out) PIE_HIP(c, hipMemcpyAsync(counts_out, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDeviceToHost, a));
    if (offsets_out) PIE_HIP(c, hipMemcpyAsync(offsets_out, sl.offsets, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToHost, a));
    if (idx_out && m > idx_cap) {
        PIE_HIP(c, hipStreamSynchronize(a));
        return fail(c, PIE_E_CAPACITY, "idx_cap %zu < selected rows %zu", idx_cap, m);
    }
    if (idx_out && m) PIE_HIP(c, hipMemcpyAsync(idx_out, sl.out_idx, m * 4, hipMemcpyDeviceToHost, a));
    PIE_HIP(c, hipStreamSynchronize(a));
    return PIE_OK;
}

int pie_read_user_feed(pie_ctx* c, int32_t user, int32_t* idx_out, size_t idx_cap, size_t* k_out)
{
    if (!c) return PIE_E_INVAL;
    if (k_out) *k_out = 0;
    if (!c->res || !c->res->have_result) return fail(c, PIE_E_STATE, "no scan result on this context");
    if (user < 0 || user >= c->n_users) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    Slot& sl = *c->res;
    long long off[2] = {0, 0};
    PIE_HIP(c, hipMemcpyAsync(off, sl.offsets + user, sizeof off, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    const size_t k = (size_t)(off[1] - off[0]);
    if (k_out) *k_out = k;
    if (k == 0) return PIE_OK;
    if (!idx_out || k > idx_cap) return fail(c, PIE_E_CAPACITY, "idx_cap %zu < feed length %zu", idx_cap, k);
    PIE_HIP(c, hipMemcpyAsync(idx_out, sl.out_idx + off[0], k * 4, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

int pie_scan(pie_ctx* c, int64_t now, int64_t cutoff, int32_t* counts_out, int64_t* offsets_out, int32_t* idx_out,
             size_t idx_cap, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    if (c->b_flight) return fail(c, PIE_E_STATE, "a batch is in flight: finish it first");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = run_scan(c, now, cutoff);
    if (m_out) *m_out = c->res ? (size_t)c->res->last.m : 0;
    if (rc) return rc;
    return pie_read_results(c, counts_out, offsets_out, idx_out, idx_cap, m_out);
}

int pie_result_device_ptrs(pie_ctx* c, void** counts_dev, void** offsets_dev, void** idx_dev)
{
    if (!c) return PIE_E_INVAL;
    if (!c->res || !c->res->have_result) return fail(c, PIE_E_STATE, "no scan result on this context");
    if (counts_dev) *counts_dev = c->res->counts_ord;
    if (offsets_dev) *offsets_dev = c->res->offsets;
    if (idx_dev) *idx_dev = c->res->out_idx;
    return PIE_OK;
}

int pie_copy_results_device(pie_ctx* c, void* counts_dst, void* offsets_dst, void* idx_dst, size_t idx_cap)
{
    if (!c) return PIE_E_INVAL;
    if (!c->res || !c->res->have_result) return fail(c, PIE_E_STATE, "no scan result on this context");
    PIE_HIP(c, hipSetDevice(c->device));
    Slot& sl = *c->res;
    hipStream_t a = c->stream;
    if (counts_dst) PIE_HIP(c, hipMemcpyAsync(counts_dst, sl.counts_ord, (size_t)c->n_users * 4, hipMemcpyDeviceToDevice, a));
    if (offsets_dst)
        PIE_HIP(c, hipMemcpyAsync(offsets_dst, sl.offsets, ((size_t)c->n_users + 1) * 8, hipMemcpyDeviceToDevice, a));
    size_t m = (size_t)sl.last.m;
    if (m > idx_cap) m = idx_cap;
    if (idx_dst && m) PIE_HIP(c, hipMemcpyAsync(idx_dst, sl.out_idx, m * 4, hipMemcpyDeviceToDevice, a));
    return PIE_OK;
}

int pie_pack_results_device(pie_ctx* c, void* dst_i32, size_t u_pad, size_t idx_cap)
{
    if (!c) return PIE_E_INVAL;
    if (!c->res || !c->res->have_result) return fail(c, PIE_E_STATE, "no scan result on this context");
    if (!dst_i32 || u_pad < (size_t)c->n_users) return fail(c, PIE_E_INVAL, "bad pack destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    Slot& sl = *c->res;
    const size_t total = u_pad + 2 + ((size_t)sl.last.m < idx_cap ? (size_t)sl.last.m : idx_cap);
    size_t grid = (total + 255) / 256;
    if (grid > (size_t)c->n_cus * 8) grid = (size_t)c->n_cus * 8;
    hipLaunchKernelGGL(k_pack_results, dim3((unsigned)grid), dim3(256), 0, c->stream, sl.offsets, c->n_users, (int)u_pad,
                       sl.sum, sl.out_idx, (long long)idx_cap, (int*)dst_i32);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

int pie_batch_pack_union_device(pie_ctx* c, void* dst_i32, size_t u_pad, size_t cap)
{
    if (!c) return PIE_E_INVAL;
    if (!c->bres || !c->bres->have_result) return fail(c, PIE_E_STATE, "no batch result on this context");
    if (c->bres->wide) return fail(c, PIE_E_STATE, "the last batch is wide: use pie_batch_pack_union_wide_device");
    if (int rc_o = order_after_batch(c, *c->bres)) return rc_o; // the batch may have run on another lane's stream
    if (!dst_i32 || u_pad < (size_t)c->n_users || u_pad > 0x7FFFFFF0u) return fail(c, PIE_E_INVAL, "bad union destination / u_pad < n_users");
    PIE_HIP(c, hipSetDevice(c->device));
    return batch_pack_union(c, *c->bres, dst_i32, u_pad, cap);
}

int pie_fetch_rows(pie_ctx* c, const int32_t* idx, size_t m, int64_t* start, int64_t* end, int32_t* user, int32_t* disc)
{
    if (!c) return PIE_E_INVAL;
    if (m == 0) return PIE_OK;
    if (!idx) return fail(c, PIE_E_INVAL, "idx is NULL");
    if (c->n == 0) return fail(c, PIE_E_STATE, "no table loaded");
    PIE_HIP(c, hipSetDevice(c->device));
    // device scratch: [start m*8][end m*8][user m*4][disc m*4][idx m*4]
    char* d = nullptr;
    const size_t bytes = m * 28 + 64;
    PIE_HIP(c, hipMalloc(&d, bytes));
    long long* o_s = reinterpret_cast<long long*>(d);
    long long* o_e = o_s + m;
    int* o_u = reinterpret_cast<int*>(o_e + m);
    int* o_d = o_u + m;
    int* d_idx = o_d + m;
    hipError_t e = hipMemcpyAsync(d_idx, idx, m * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_fetch_rows, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, d_idx, (long long)m,
                           c->n, c->d_start, c->d_end, c->d_user, c->d_disc, o_s, o_e, o_u, o_d);
        e = hipGetLastError();
    }
    if (e == hipSuccess && start) e = hipMemcpyAsync(start, o_s, m * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && end) e = hipMemcpyAsync(end, o_e, m * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && user) e = hipMemcpyAsync(user, o_u, m * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && disc) e = hipMemcpyAsync(disc, o_d, m * 4, hipMemcpyDeviceToHost, c->stream);
    hipError_t e2 = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess || e2 != hipSuccess)
        return fail(c, PIE_E_HIP, "pie_fetch_rows: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return PIE_OK;
}

int pie_expired_queue(pie_ctx* c, int64_t prev_now, int64_t now, int32_t* queue_out, size_t cap, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    if (q_out) *q_out = 0;
    const bool two_pass = getenv("PIE_EXPIRED_TWO_PASS") != nullptr; // the count / prefix / write form, kept for A-B runs
    bool empty;
    int rc = list_enter(c, two_pass ? kChecksOnly : kDropSlots, &empty);
    if (rc) return rc;
    if (empty) { c->q_kind = 1; return PIE_OK; } // an empty queue: nothing on the device to read
    if (two_pass) {
        size_t k = 0;
        rc = row_list(c, kExpired, false, (long long)prev_now, (long long)now, queue_out, cap, &k, false);
        if (rc == PIE_OK || rc == PIE_E_CAPACITY) { c->q_kind = 1; c->q_rows = (long long)k; c->q_dev = c->slot[0].out_idx; }
        if (q_out) *q_out = k;
        return rc;
    }
    hipStream_t s = c->stream;
    // workspace: slot 0's out_idx is the device-side queue, slot 1's out_idx the per-wave staging, slot 0's
    // blk_count the per-wave counts (4 per block of the liveness-first plan: <= the streaming plan's block count)
    Slot& q = c->slot[0];
    Slot& st = c->slot[1];
    const int blocks = c->plan_blocks[1];
    const long long rpb = c->plan_rows[1];
    const int n_waves = blocks * kK1Waves;
    const bool prof = c->profiling && c->ring_used < kEventRing;
    if (prof && (int)c->ring.size() <= c->ring_used) {
        ScanEvents e{};
        PIE_HIP(c, hipEventCreate(&e.e0));
        PIE_HIP(c, hipEventCreate(&e.e1));
        PIE_HIP(c, hipEventCreate(&e.e2));
        c->ring.push_back(e);
    }
    if (prof) PIE_HIP(c, hipEventRecord(c->ring[c->ring_used].e0, s));
    if (c->key_ok && c->keyed_enabled && !getenv("PIE_EXPIRED_ON_END"))
        hipLaunchKernelGGL(k_expired_stage_keyed<2>, dim3(blocks), dim3(kK1Threads), 0, s, c->d_key, c->d_end, c->n, rpb,
                           (long long)prev_now, (long long)now, host_key_of(c, prev_now), host_key_of(c, now), st.out_idx, q.blk_count);
    else
        hipLaunchKernelGGL(k_expired_stage<8>, dim3(blocks), dim3(kK1Threads), 0, s, c->d_end, c->n, rpb, (long long)prev_now,
                           (long long)now, st.out_idx, q.blk_count);
    if (prof) PIE_HIP(c, hipEventRecord(c->ring[c->ring_used].e1, s));
    // the prefix kernel hands the queue's length to the host itself (mapped memory, seq last): no copy, no stream drain
    const unsigned long long seq = ++c->seq_counter;
    hipLaunchKernelGGL(k_block_prefix_wide, dim3(1), dim3(1024), 0, s, q.blk_count, n_waves, c->d_blk_off, &c->d_summary->m,
                       c->expired_copy_total ? (HostSummary*)nullptr : q.h_sum_dev, seq);
    hipLaunchKernelGGL(k_expired_gather, dim3(blocks < c->n_cus * 8 ? blocks : c->n_cus * 8), dim3(256), 0, s, st.out_idx,
                       q.blk_count, c->d_blk_off, n_waves, rpb / kK1Waves, q.out_idx, c->cap_rows);
    PIE_HIP(c, hipGetLastError());
    if (prof) {
        PIE_HIP(c, hipEventRecord(c->ring[c->ring_used].e2, s));
        c->ring_used++;
    }
    size_t k = 0;
    if (c->expired_copy_total) {
        rc = list_total(c, s, &k);
        if (rc) return rc;
    } else {
        // bounded wait like a scan's; the gather behind the prefix kernel may still run when the length is known (everything that
        // reads the queue afterwards is queued on this stream, behind it)
        const WaitResult w = word_wait(c, &q.h_sum->seq, seq, [&] { return hipStreamQuery(s); }, 1000.0, kPaceSummary);
        if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "expired queue failed: %s", hipGetErrorString((hipError_t)w.err));
        if (w.end != WaitEnd::Ready)
            return fail(c, PIE_E_HIP, "expired-queue length not published within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", w.waited_ms);
        k = (size_t)q.h_sum->s.m;
    }
    c->q_kind = 1;
    c->q_rows = (long long)k;
    c->q_dev = q.out_idx;
    if (q_out) *q_out = k;
    return list_copy_out(c, q.out_idx, k, queue_out, cap, "queue");
}

// The reference's archive chain on the device: group stats -> threshold on the host (U values) -> group-qualified
// scan (buckets per group, rows in table order) -> groups laid out in first-appearance order.
// The reference's archive chain entirely on the device (round 3; the threshold and the group order used to go through the
// host, the selection through the general scan path with its histogram atomics and per-bucket order):
//   1. k_arch_flag        one pass over (start, end): which groups hold a live row with start <= now - window            16 B/row
//                         (<=> now - min(start) >= window, sqlProvider.js:798) — a bitmap; `user` only for rows that pass
//   2. k_arch_select x 2  the selection, order-preserving (count per block, prefix, write): (group, row) pairs in table
//                         order, the bitmap looked up in LDS                                                          2 x 12 B/row
//   3. stable radix sort of the M pairs by group: the rows of a group stay in table order, and the head of its run IS its
//      first row — the first-appearance order (Map insertion order, :769-789) costs no per-row work
//   4. per group: key = first row; radix sort of the U (key, group) pairs; sizes in that order; exclusive scan; gather of
//      every group's run into its place in the queue
// The sorts and the scan are rocPRIM's (plain library primitives, as hipBLASLt would be for a plain GEMM); everything that
// touches the table is above.  Algorithmic bytes: 20 B/row (start, end, user: the group statistics) + 12 B/row (end, user:
// the selection) + 4 B per queued row.
int pie_archive_queue(pie_ctx* c, int64_t now, int64_t window_ms, int32_t* queue_out, size_t cap, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    if (q_out) *q_out = 0;
    bool empty;
    int rc = list_enter(c, kSyncAll, &empty); // the slots' results are given up below, once nothing can fail for want of memory
    if (rc) return rc;
    if (empty) { c->q_kind = 2; return PIE_OK; } // an empty queue: nothing on the device to read
    rc = ensure_sel(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const size_t U = (size_t)c->n_users;
    // per-group scratch: carved from one allocation kept with the context
    const size_t u4 = ((U + 63) / 64) * 64;
    const int words = (int)((U + 31) / 32);
    const size_t grp_bytes = u4 * 4 * 9 + 256;
    if (c->arch_bytes < grp_bytes) {
        dfree(c->d_arch);
        c->arch_bytes = 0;
        PIE_HIP(c, hipMalloc(&c->d_arch, grp_bytes));
        c->arch_bytes = grp_bytes;
    }
    char* p = c->d_arch;
    auto carve = [&](size_t bytes) { char* q = p; p += bytes; return q; };
    unsigned int* d_bits = reinterpret_cast<unsigned int*>(carve(u4 * 4)); // (words <= u4)
    int* d_ghead = reinterpret_cast<int*>(carve(u4 * 4));
    int* d_gfirst = reinterpret_cast<int*>(carve(u4 * 4));
    int* d_glast = reinterpret_cast<int*>(carve(u4 * 4));
    unsigned int* d_key[2] = {reinterpret_cast<unsigned int*>(carve(u4 * 4)), reinterpret_cast<unsigned int*>(carve(u4 * 4))};
    int* d_val[2] = {reinterpret_cast<int*>(carve(u4 * 4)), reinterpret_cast<int*>(carve(u4 * 4))};
    unsigned int* d_size = reinterpret_cast<unsigned int*>(carve(u4 * 4));
    unsigned int* d_nqual = reinterpret_cast<unsigned int*>(carve(256));
    Slot& sl = c->slot[0];
    Slot& other = c->slot[1];
    drop_results(c, true);
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (c->profiling) {
        PIE_HIP(c, hipEventCreate(&ev0));
        PIE_HIP(c, hipEventCreate(&ev1));
        PIE_HIP(c, hipEventRecord(ev0, s));
    }
    // now - earliest >= window  <=>  earliest <= now - window, in 128 bits (JS numbers do not wrap)
    const __int128 lim128 = (__int128)now - (__int128)window_ms;
    const bool none = lim128 < (__int128)INT64_MIN;
    const long long limit = lim128 > (__int128)INT64_MAX ? INT64_MAX : (none ? INT64_MIN : (long long)lim128);
    PIE_HIP(c, hipMemsetAsync(d_bits, 0, (size_t)words * 4, s));
    PIE_HIP(c, hipMemsetAsync(d_nqual, 0, 4, s));
    hipLaunchKernelGGL(k_arch_flag, dim3(c->n_cus * 16), dim3(256), 0, s, c->d_start, c->d_end, c->d_user, c->n, c->n_users, limit, none, d_bits);
    hipLaunchKernelGGL(k_arch_popc, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, d_bits, words, d_nqual);
    // the selection: (group, row) pairs in table order
    const int blocks = c->plan_blocks[0];
    const long long rpb = c->plan_rows[0]; // a multiple of the streaming tile: even
    const bool lds_bits = (size_t)words * 4 <= (size_t)48 * 1024; // up to 393 216 groups; beyond: the bitmap is read through the caches
    const size_t lds = lds_bits ? (size_t)words * 4 : 0;
    if (lds_bits) hipLaunchKernelGGL((k_arch_select<false, true>), dim3(blocks), dim3(256), lds, s, c->d_end, c->d_user, c->n, rpb, d_bits, words, c->n_users, sl.blk_count, (const long long*)nullptr, (unsigned int*)nullptr, (int*)nullptr);
    else hipLaunchKernelGGL((k_arch_select<false, false>), dim3(blocks), dim3(256), 0, s, c->d_end, c->d_user, c->n, rpb, d_bits, words, c->n_users, sl.blk_count, (const long long*)nullptr, (unsigned int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, sl.blk_count, blocks, c->d_blk_off, &c->d_summary->m);
    PIE_HIP(c, hipGetLastError());
    unsigned int n_qual = 0;
    PIE_HIP(c, hipMemcpyAsync(&n_qual, d_nqual, 4, hipMemcpyDeviceToHost, s)); // list_total waits for it too
    size_t q = 0;
    rc = list_total(c, s, &q);
    if (rc) return rc;
    if (q_out) *q_out = q;
    c->arch_alg_bytes = 32ull * (unsigned long long)c->n + 4ull * q;
    if (queue_out && q > cap) return fail(c, PIE_E_CAPACITY, "queue cap %zu < %zu", cap, q);
    if (q) {
        // pair arrays in slot 0's record staging (16 B per row of capacity: four 4-byte arrays of q <= n entries); the
        // sorts' temporary storage and the queue in slot 1's
        unsigned int* k_in = reinterpret_cast<unsigned int*>(sl.sel);
        unsigned int* k_out = k_in + q;
        int* v_in = reinterpret_cast<int*>(k_out + q);
        int* v_out = v_in + q;
        int* d_queue = reinterpret_cast<int*>(other.sel);
        size_t need = 0;
        // temporary storage of the library primitives: a buffer of its own, grown to what they ask for (a table of a handful of
        // rows and 600 000 users wants more for the per-group sort than the table's record staging holds: found by the fuzz)
        auto tmp_for = [&](size_t bytes) -> void* {
            if (bytes > c->arch_tmp_bytes) {
                if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
                dfree(c->d_arch_tmp);
                c->arch_tmp_bytes = 0;
                if (hipMalloc(&c->d_arch_tmp, bytes + bytes / 4 + 4096) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
                c->arch_tmp_bytes = bytes + bytes / 4 + 4096;
            }
            return c->d_arch_tmp;
        };
        void* tmp = nullptr;
        if (lds_bits) hipLaunchKernelGGL((k_arch_select<true, true>), dim3(blocks), dim3(256), lds, s, c->d_end, c->d_user, c->n, rpb, d_bits, words, c->n_users, (int*)nullptr, c->d_blk_off, k_in, v_in);
        else hipLaunchKernelGGL((k_arch_select<true, false>), dim3(blocks), dim3(256), 0, s, c->d_end, c->d_user, c->n, rpb, d_bits, words, c->n_users, (int*)nullptr, c->d_blk_off, k_in, v_in);
        unsigned g_bits = 1;
        while (g_bits < 32 && (1ull << g_bits) < (unsigned long long)U) ++g_bits;
        PIE_HIP(c, rocprim::radix_sort_pairs(nullptr, need, k_in, k_out, v_in, v_out, q, 0u, g_bits, s));
        if (!(tmp = tmp_for(need))) return fail(c, PIE_E_NOMEM, "sort scratch of %zu bytes", need);
        PIE_HIP(c, rocprim::radix_sort_pairs(tmp, need, k_in, k_out, v_in, v_out, q, 0u, g_bits, s));
        unsigned hb = (unsigned)((q + 255) / 256);
        if (hb > (unsigned)c->n_cus * 16) hb = (unsigned)c->n_cus * 16;
        hipLaunchKernelGGL(k_arch_heads, dim3(hb), dim3(256), 0, s, k_out, v_out, (long long)q, d_ghead, d_gfirst, d_glast);
        hipLaunchKernelGGL(k_arch_group_keys, dim3((unsigned)((U + 255) / 256)), dim3(256), 0, s, d_bits, d_gfirst, c->n_users, d_key[0], d_val[0]);
        PIE_HIP(c, rocprim::radix_sort_pairs(nullptr, need, d_key[0], d_key[1], d_val[0], d_val[1], U, 0u, 32u, s));
        if (!(tmp = tmp_for(need))) return fail(c, PIE_E_NOMEM, "sort scratch of %zu bytes", need);
        PIE_HIP(c, rocprim::radix_sort_pairs(tmp, need, d_key[0], d_key[1], d_val[0], d_val[1], U, 0u, 32u, s));
        hipLaunchKernelGGL(k_arch_sizes, dim3((unsigned)((n_qual + 255) / 256)), dim3(256), 0, s, d_val[1], d_nqual, d_ghead, d_glast, d_size);
        unsigned int* d_off = d_key[0]; // free again
        PIE_HIP(c, rocprim::exclusive_scan(nullptr, need, d_size, d_off, 0u, (size_t)n_qual, rocprim::plus<unsigned int>(), s));
        if (!(tmp = tmp_for(need))) return fail(c, PIE_E_NOMEM, "scan scratch of %zu bytes", need);
        PIE_HIP(c, rocprim::exclusive_scan(tmp, need, d_size, d_off, 0u, (size_t)n_qual, rocprim::plus<unsigned int>(), s));
        const unsigned gb = n_qual < (unsigned)c->n_cus * 16 ? n_qual : (unsigned)c->n_cus * 16;
        hipLaunchKernelGGL(k_arch_gather, dim3(gb ? gb : 1u), dim3(256), 0, s, d_val[1], d_nqual, d_ghead, d_size, d_off, v_out, d_queue);
        PIE_HIP(c, hipGetLastError());
        if (ev1) PIE_HIP(c, hipEventRecord(ev1, s));
        if (queue_out) PIE_HIP(c, hipMemcpyAsync(queue_out, d_queue, q * 4, hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipStreamSynchronize(s));
        c->q_dev = d_queue;
        c->q_goff = d_off;
        c->q_groups = (int)n_qual;
    } else if (ev1) {
        PIE_HIP(c, hipEventRecord(ev1, s));
        PIE_HIP(c, hipStreamSynchronize(s));
    }
    c->q_kind = 2;
    c->q_rows = (long long)q;
    if (ev0) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) { c->arch_ms_sum += ms; c->arch_calls++; }
        (void)hipEventDestroy(ev0);
        (void)hipEventDestroy(ev1);
    }
    return PIE_OK;
}

int pie_archive_stats(pie_ctx* c, double* ms_sum_out, uint32_t* calls_out, uint64_t* alg_bytes_out)
{
    if (!c) return PIE_E_INVAL;
    if (ms_sum_out) *ms_sum_out = c->arch_ms_sum;
    if (calls_out) *calls_out = c->arch_calls;
    if (alg_bytes_out) *alg_bytes_out = c->arch_alg_bytes;
    return PIE_OK;
}

int pie_queue_info(pie_ctx* c, int32_t* kind_out, size_t* rows_out, size_t* groups_out)
{
    if (!c) return PIE_E_INVAL;
    if (kind_out) *kind_out = c->q_kind;
    if (rows_out) *rows_out = (size_t)c->q_rows;
    if (groups_out) *groups_out = (size_t)c->q_groups;
    if (c->q_kind == 0) return fail(c, PIE_E_STATE, "no queue on the device: pie_expired_queue / pie_archive_queue first");
    if (c->d_shard_rows && c->n > c->shard_rows_n)
        return fail(c, PIE_E_STATE, "%lld rows were added after pie_shard_table: they have no global row", c->n - c->shard_rows_n);
    return PIE_OK;
}

int pie_queue_pack_device(pie_ctx* c, void* dst_i32, size_t cap_rows, size_t cap_groups)
{
    if (!c) return PIE_E_INVAL;
    int rc = pie_queue_info(c, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (!dst_i32) return fail(c, PIE_E_INVAL, "dst is NULL");
    if (cap_rows > 0x3FFFFFF0u || cap_groups > 0x3FFFFFF0u) return fail(c, PIE_E_INVAL, "cap_rows / cap_groups above 2^30");
    if ((size_t)c->q_rows > cap_rows || (size_t)c->q_groups > cap_groups)
        return fail(c, PIE_E_CAPACITY, "queue of %lld rows / %d groups above cap %zu / %zu", c->q_rows, c->q_groups, cap_rows, cap_groups);
    PIE_HIP(c, hipSetDevice(c->device));
    const long long work = 2 + c->q_rows + (long long)c->q_groups + 1;
    long long grid = (work + 255) / 256;
    if (grid > (long long)c->n_cus * 8) grid = (long long)c->n_cus * 8;
    hipLaunchKernelGGL(k_queue_pack, dim3((unsigned)grid), dim3(256), 0, c->stream, c->q_dev, c->q_rows, c->q_goff, c->q_groups,
                       (const int*)c->d_shard_rows, (long long)cap_rows, (int*)dst_i32);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

int pie_set_scan_form(pie_ctx* c, int form)
{
    if (!c) return PIE_E_INVAL;
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    if (form < 0) {
        c->k1_pinned = false;
        c->k1_variant = 0x03;
    } else {
        c->k1_pinned = true;
        c->k1_variant = form;
    }
    return PIE_OK;
}

static int token_info(pie_ctx* c, pie_table_info* out);

int pie_table_info_get(pie_ctx* c, pie_table_info* out)
{
    if (!c || !out) return PIE_E_INVAL;
    // the struct grows at its end: a caller built against the form without the compaction fields gets the fields it knows
    const uint32_t caller_size = out->struct_size;
    if (caller_size != sizeof(pie_table_info) && caller_size != offsetof(pie_table_info, expired_inflight_bytes) &&
        caller_size != offsetof(pie_table_info, token_rows) && caller_size != offsetof(pie_table_info, hot_build_ms) &&
        caller_size != offsetof(pie_table_info, compact_bytes))
        return fail(c, PIE_E_INVAL, "pie_table_info.struct_size mismatch");
    pie_table_info full{};
    pie_table_info* const caller = out;
    out = &full;
    const size_t rows = (size_t)c->cap_rows, users = (size_t)c->cap_users;
    out->has_keys = (c->key_ok && c->d_key && c->d_pay && c->d_fkey) ? 1u : 0u;
    out->rows = (uint64_t)c->n;
    out->users = (uint64_t)c->n_users;
    out->table_bytes = (uint64_t)rows * 24u;
    out->derived_bytes = (c->d_key && c->d_pay && c->d_fkey) ? (uint64_t)rows * (sizeof(lkey_t) + sizeof(fkey_t) + sizeof(PayRec)) + 128u : 0u;
    // mirrors ensure_capacity(): per slot sel + sel_rank + bkt + out_idx (row-sized), the direct slots, the per-user arrays
    uint64_t per_slot = 0;
    if (rows) {
        per_slot += (uint64_t)c->sel_cap * (sizeof(SelRec) + 4) + (uint64_t)rows * (sizeof(BktRec) + 4);
        per_slot += (uint64_t)users * (8 + 4 + 4 + sizeof(Segment) * 2 + 4) + (uint64_t)(rows / kSegMax) * sizeof(Segment);
        if (c->slot[0].direct) per_slot += ((uint64_t)users << c->dshift) * sizeof(BktRec);
        per_slot += (uint64_t)kPartMax * kPartCap * sizeof(SelRec);
    }
    out->workspace_bytes = rows ? 2 * per_slot + 3 * (uint64_t)counts_span(c) : 0;
    for (bool alloc : c->lane_alloc) // batched scans, per lane: three slots (union bucket slots 16 B each, the mask tables, the union result 12 B per entry, 8 per user), three spans
        if (alloc)
            out->workspace_bytes += kBatchSlots * (((uint64_t)users << c->bdshift) * sizeof(BktRec) + kMaskTabWords * 8u + (uint64_t)batch_ucap(c) * 12 + ((uint64_t)users + 2) * 8) +
                                    3 * (uint64_t)batch_span_bytes(c);
    for (const BatchSlot& b : c->bslot) // per-query list storage, where somebody asked for lists
        out->workspace_bytes += (uint64_t)b.lists_q * ((uint64_t)batch_users_stride(c) * 12 + (uint64_t)batch_out_stride(c) * 4);
    for (const BatchSlot& b : c->bslot) { // the wide state of slots that ran wide batches
        if (!b.w) continue;
        if (b.w->dmask) out->workspace_bytes += ((uint64_t)c->cap_users << b.w->dshift) * kWideWords * 8;
        if (b.w->umask) out->workspace_bytes += (uint64_t)b.w->umask_rows * (uint64_t)b.w->umask_words * 8;
        if (b.w->d_wq) out->workspace_bytes += (uint64_t)kWideMax * sizeof(WideQuery);
        for (const WideSlot::List& l : b.w->lists)
            if (l.counts) out->workspace_bytes += ((uint64_t)c->cap_users + 1) * 12 + (uint64_t)l.idx_cap * 4;
    }
    if (c->ord.wp_rows) out->workspace_bytes += (uint64_t)c->ord.wp_cap * (4 + (uint64_t)c->ord.wp_words * 8); // the pool of wide batches on the run
    out->index_build_ms = c->index_build_ms;
    out->ordered_rows = c->ord.valid ? (uint64_t)c->ord.held : 0u;
    out->ordered_positions = c->ord.valid ? (uint64_t)c->ord.n : 0u;
    // the run's columns (record 16 + end 8 + keys 3 per position, row -> position 4 per row) and its small per-unit arrays
    out->ordered_bytes = c->ord.pay ? (uint64_t)c->ord.pos_cap * (sizeof(OrdRec) + 8 + sizeof(lkey_t) + sizeof(fkey_t)) + (uint64_t)c->ord.cap * 4 +
                                          (uint64_t)c->ord.units_cap * 12 + ((uint64_t)c->ord.pos_cap / kOrdTile + 2) * kOrdSlices * 12 +
                                          ((uint64_t)c->ord.cap_users + 1) * 12
                                    : 0u;
    out->ordered_build_ms = c->ord.build_ms;
    out->ordered_builds = c->ord.builds;
    out->ordered_respreads = c->ord.respreads;
    out->hot_rows = c->hix.valid ? (uint64_t)c->hix.n_main : 0u;
    out->hot_bytes = (uint64_t)c->hix.rec_cap * sizeof(HotRec) + (uint64_t)c->hix.pos_cap * 4 + (uint64_t)c->hix.cnt_cap * 4 + (c->hix.d_off ? 129 * 8 + 4 : 0);
    out->hot_builds = c->hix.builds;
    if (c->hix.timed) { // the last build's device time, read once it has run
        float ms = 0.f;
        if (hipEventSynchronize(c->hix.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, c->hix.ev[0], c->hix.ev[1]) == hipSuccess) c->hix.build_ms = ms;
        else (void)hipGetLastError();
        c->hix.timed = false;
    }
    out->hot_build_ms = c->hix.build_ms;
    out->hot_order = (uint32_t)(c->hix.valid ? c->hix.built_order : c->hix.order);
    out->hot_slot_bits = (uint32_t)hot_slot_bits((unsigned long long)c->n_users);
    out->compact_bytes = c->cmp_valid ? (uint64_t)(c->cmp_n_old > 0 ? c->cmp_n_old : 1) * 4 + (uint64_t)(c->cmp_n_kept > 0 ? c->cmp_n_kept : 1) * 4 : 0u;
    out->compactions = c->compactions;
    out->compact_count_ms = c->cmp_count_ms;
    out->compact_write_ms = c->cmp_write_ms;
    {
        pie_ctx::ExpiredFlight& x = c->expq;
        out->expired_inflight_bytes = (x.d_scratch ? (uint64_t)expq_scratch_of().bytes : 0u) + (uint64_t)x.buf_rows * 4;
        if (x.timed && !(x.begun && !x.landed)) { // the last pass's device time, read once it has run
            float ms = 0.f;
            if (hipEventSynchronize(x.fence.done) == hipSuccess && hipEventElapsedTime(&ms, x.t0, x.fence.done) == hipSuccess) x.ms = ms;
            else (void)hipGetLastError();
            x.timed = false;
        }
        out->expired_inflight_ms = x.ms;
    }
    const int token_rc = token_info(c, out); // a sharded column reads covered_l back: that can fail
    if (token_rc) return token_rc;
    full.struct_size = caller_size;
    memcpy(caller, &full, caller_size);
    return PIE_OK;
}

uint64_t pie_hot_order_key(uint32_t bin, int32_t user, uint32_t n_users)
{
    const unsigned long long t = ((unsigned long long)n_users + 31) >> 5, pad = t * 32;
    const unsigned long long u = (unsigned long long)(uint32_t)user;
    const unsigned long long slot = u < pad ? (u & 31) * t + (u >> 5) : 0; // hist_index (pie_kernels.h)
    return ((uint64_t)bin << hot_slot_bits(n_users)) | slot;
}

uint32_t pie_hot_slot_bits(uint32_t n_users) { return (uint32_t)hot_slot_bits(n_users); }

int pie_hot_layout(pie_ctx* c, int64_t* off, int64_t* n_main, int32_t* user, int32_t* row, int32_t* bin, size_t cap, int32_t* pos, size_t n_pos)
{
    if (!c) return PIE_E_INVAL;
    if (!c->hix.valid) return fail(c, PIE_E_STATE, "there is no hot index");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = sync_all(c);
    if (rc) return rc;
    const pie_ctx::HotIndex& h = c->hix;
    if (off) for (int k = 0; k <= 128; ++k) off[k] = h.off[k];
    if (n_main) *n_main = h.n_main;
    if (user || row || bin) {
        if ((long long)cap < h.n_main) return fail(c, PIE_E_CAPACITY, "the hot index holds %lld main records, room for %zu", h.n_main, cap);
        std::vector<HotRec> rec((size_t)h.n_main);
        if (h.n_main) PIE_HIP(c, hipMemcpy(rec.data(), h.rec, rec.size() * sizeof(HotRec), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < rec.size(); ++i) {
            if (user) user[i] = rec[i].user;
            if (row) row[i] = rec[i].row;
            if (bin) bin[i] = rec[i].bin;
        }
    }
    if (pos) {
        if ((long long)n_pos > c->n) return fail(c, PIE_E_INVAL, "asked for %zu rows, table has %lld", n_pos, c->n);
        if (n_pos) PIE_HIP(c, hipMemcpy(pos, h.pos, n_pos * 4, hipMemcpyDeviceToHost));
    }
    return PIE_OK;
}

int pie_set_ordered_run(pie_ctx* c, int mode)
{
    if (!c) return PIE_E_INVAL;
    if (mode < 0 || mode > 2) return fail(c, PIE_E_INVAL, "ordered-run mode must be 0 (never), 1 (adaptive) or 2 (always)");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    c->ord.mode = mode;
    c->ord.wanted = 0;
    if (mode == 0) {
        PIE_HIP(c, hipSetDevice(c->device));
        PIE_HIP(c, hipStreamSynchronize(c->stream));
        ord_free(c);
    }
    return PIE_OK;
}

int pie_set_wide_ordered(pie_ctx* c, int on)
{
    if (!c) return PIE_E_INVAL;
    if (on != 0 && on != 1) return fail(c, PIE_E_INVAL, "pie_set_wide_ordered takes 0 (off) or 1 (on)");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    c->wide_ordered = on == 1;
    return PIE_OK;
}

int pie_set_turn_ordered(pie_ctx* c, int on)
{
    if (!c) return PIE_E_INVAL;
    if (on != 0 && on != 1) return fail(c, PIE_E_INVAL, "pie_set_turn_ordered takes 0 (off) or 1 (on)");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    c->turn_ordered = on == 1;
    return PIE_OK;
}

int pie_host_alloc(pie_ctx* c, size_t bytes, void** host_out, void** dev_out)
{
    if (!c || !host_out || !dev_out || bytes == 0) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    void* h = nullptr;
    void* d = nullptr;
    PIE_HIP(c, hipHostMalloc(&h, bytes, hipHostMallocMapped));
    hipError_t e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) { (void)hipHostFree(h); return fail(c, PIE_E_HIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e)); }
    memset(h, 0, bytes);
    *host_out = h;
    *dev_out = d;
    return PIE_OK;
}

int pie_host_free(pie_ctx* c, void* host_ptr)
{
    if (!c) return PIE_E_INVAL;
    if (!host_ptr) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    PIE_HIP(c, hipStreamSynchronize(c->stream)); // a scan may still be writing it
    PIE_HIP(c, hipHostFree(host_ptr));
    return PIE_OK;
}

int pie_set_profiling(pie_ctx* c, int enabled)
{
    if (!c) return PIE_E_INVAL;
    c->profiling = enabled != 0;
    c->profile_every = enabled > 1 ? enabled : 1;
    return PIE_OK;
}

int pie_stats_get(pie_ctx* c, pie_stats* out)
{
    if (!c || !out) return PIE_E_INVAL;
    // the struct grows at its end (as pie_table_info does): a caller built against the form without the route counters gets the
    // fields it knows
    const uint32_t caller_size = out->struct_size;
    if (caller_size != sizeof(pie_stats) && caller_size != offsetof(pie_stats, n_small)) return fail(c, PIE_E_INVAL, "pie_stats.struct_size mismatch");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = resolve_events(c);
    if (rc) return rc;
    pie_stats full{};
    pie_stats* const caller = out;
    out = &full;
    const Slot* sl = c->res;
    out->n_profiled = c->n_profiled;
    out->rows = (uint64_t)c->n;
    out->users = (uint64_t)c->n_users;
    out->selected = sl ? sl->last.m : 0;
    out->alg_bytes = 24ull * (uint64_t)c->n;
    out->k1_ms_sum = c->k1_ms_sum;
    out->scan_ms_sum = c->scan_ms_sum;
    out->max_bucket = sl ? sl->last.max_count : 0;
    out->n_segments = sl ? sl->last.n_seg : 0;
    out->n_big = sl ? sl->last.n_big : 0;
    out->k1_blocks = sl ? (uint32_t)sl->k1_blocks : 0;
    out->k1_variant = sl ? (uint32_t)sl->variant : 0;
    out->key_ambiguous = (c->res && (c->res->variant & 0x400)) ? (uint32_t)(c->res->last.amb > 0xFFFFFFFFull ? 0xFFFFFFFFull : c->res->last.amb) : 0u;
    out->live = sl ? sl->last.live : 0;
    out->candidates = (sl && (sl->variant & 0x400)) ? sl->last.cand : 0;
    // the K2 route counters: words of the summary record the scan published anyway, and the capacity the host chose
    const bool k2_route = sl && !sl->ordered && !sl->fast;
    out->n_small = k2_route ? sl->last.n_small : 0;
    out->n_over = k2_route ? sl->last.n_over : 0;
    out->n_hot = k2_route ? (sl->last.n_hot < (unsigned)kHotMax ? sl->last.n_hot : (unsigned)kHotMax) : 0;
    out->direct_shift = k2_route ? (uint32_t)sl->dshift : 0;
    if (c->last_was_batch && c->bres && c->bres->have_result) {
        // the last finished thing was a batch: selected = rows over all its queries, form = keyed | 0x1000 (batched)
        const BatchSlot& b = *c->bres;
        uint64_t m = 0;
        uint32_t mx = 0;
        if (b.wide) {
            for (int q = 0; q < b.n_q; ++q) m += b.w->m[q];
            mx = b.unsupported ? 0u : b.last[0].max_count;
        } else {
            for (int q = 0; q < b.n_q; ++q) { m += b.last[q].m; mx = mx > b.last[q].max_count ? mx : b.last[q].max_count; }
        }
        out->selected = m;
        out->max_bucket = mx;
        out->n_segments = out->n_big = 0;
        out->n_small = out->n_over = out->n_hot = out->direct_shift = 0;
        out->k1_blocks = (uint32_t)b.k1_blocks;
        out->k1_variant = b.unsupported ? 0u : b.ordered ? (0x3400u | (b.fine_key ? 0x800u : 0u)) : (0x1485u | (b.fine_key ? 0x800u : 0u));
        out->key_ambiguous = 0;
        out->live = 0;
        out->candidates = b.unsupported ? 0 : b.last[0].cand;
    }
    full.struct_size = caller_size;
    memcpy(caller, &full, caller_size);
    return PIE_OK;
}

int pie_stats_reset(pie_ctx* c)
{
    if (!c) return PIE_E_INVAL;
    int rc = resolve_events(c);
    c->k1_ms_sum = c->scan_ms_sum = 0;
    c->arch_ms_sum = 0;
    c->arch_calls = 0;
    c->n_profiled = 0;
    return rc;
}

int pie_synchronize(pie_ctx* c)
{
    if (!c) return PIE_E_INVAL;
    PIE_HIP(c, hipSetDevice(c->device));
    return sync_all(c);
}

int pie_shard_table(pie_ctx* c, int32_t rank, int32_t world, size_t* n_rows_out, int32_t* n_users_out)
{
    if (!c) return PIE_E_INVAL;
    if (world < 1 || rank < 0 || rank >= world) return fail(c, PIE_E_INVAL, "rank %d outside [0, %d)", rank, world);
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = expq_land(c, "pie_shard_table"); // an expired queue begun on the whole table keeps its answer
    if (rc) return rc;
    rc = sync_all(c);
    if (rc) return rc;
    hipStream_t s = c->stream;
    const long long n = c->n;
    const int U = c->n_users;
    int *d_flag = nullptr, *d_local = nullptr, *d_users = nullptr, *d_blk = nullptr, *o_user = nullptr, *o_disc = nullptr, *o_row = nullptr;
    long long *d_uoff = nullptr, *d_boff = nullptr, *o_start = nullptr, *o_end = nullptr;
    auto cleanup = [&]() {
        dfree(d_flag); dfree(d_local); dfree(d_blk); dfree(d_uoff); dfree(d_boff);
        dfree(o_start); dfree(o_end); dfree(o_user); dfree(o_disc);
    };
#define PIE_TRY(call)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            cleanup();                                                                                \
            dfree(d_users);                                                                           \
            dfree(o_row);                                                                             \
            return fail(c, e_ == hipErrorOutOfMemory ? PIE_E_NOMEM : PIE_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                             \
    } while (0)
    // 1. which users stay, and their local ids
    const unsigned ub = (unsigned)((U + 255) / 256);
    PIE_TRY(hipMalloc(&d_flag, (size_t)U * 4));
    PIE_TRY(hipMalloc(&d_local, (size_t)U * 4));
    PIE_TRY(hipMalloc(&d_users, (size_t)U * 4));
    PIE_TRY(hipMalloc(&d_uoff, ((size_t)U + 1) * 8));
    hipLaunchKernelGGL(k_shard_user_flags, dim3(ub), dim3(256), 0, s, U, (int)rank, (int)world, d_flag);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, d_flag, U, d_uoff, (unsigned long long*)nullptr);
    hipLaunchKernelGGL(k_shard_user_ids, dim3(ub), dim3(256), 0, s, U, d_flag, d_uoff, d_local, d_users);
    PIE_TRY(hipGetLastError());
    long long u_local = 0;
    PIE_TRY(hipMemcpyAsync(&u_local, d_uoff + U, 8, hipMemcpyDeviceToHost, s));
    // 2. rows: per-block counts -> prefix -> order-preserving compaction into fresh columns
    const long long rpb = 256LL * 64;
    const int blocks = (int)((n + rpb - 1) / rpb) > 0 ? (int)((n + rpb - 1) / rpb) : 1;
    PIE_TRY(hipMalloc(&d_blk, (size_t)blocks * 4));
    PIE_TRY(hipMalloc(&d_boff, ((size_t)blocks + 1) * 8));
    hipLaunchKernelGGL(k_shard_row_count, dim3(blocks), dim3(256), 0, s, c->d_user, n, rpb, d_local, U, d_blk);
    hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, d_blk, blocks, d_boff, (unsigned long long*)nullptr);
    PIE_TRY(hipGetLastError());
    long long n_local = 0;
    PIE_TRY(hipMemcpyAsync(&n_local, d_boff + blocks, 8, hipMemcpyDeviceToHost, s));
    PIE_TRY(hipStreamSynchronize(s));
    const size_t rows = (size_t)(n_local > 0 ? n_local : 1);
    PIE_TRY(hipMalloc(&o_start, rows * 8));
    PIE_TRY(hipMalloc(&o_end, rows * 8));
    PIE_TRY(hipMalloc(&o_user, rows * 4));
    PIE_TRY(hipMalloc(&o_disc, rows * 4));
    PIE_TRY(hipMalloc(&o_row, rows * 4));
    if (n > 0) {
        hipLaunchKernelGGL(k_shard_row_write, dim3(blocks), dim3(256), 0, s, c->d_start, c->d_end, c->d_user, c->d_disc, n, rpb, d_local, U,
                           d_boff, o_start, o_end, o_user, o_disc, o_row);
        PIE_TRY(hipGetLastError());
        PIE_TRY(hipStreamSynchronize(s));
    }
    // 3. a right-sized table takes the shard (the whole-table buffers and their workspace are released first)
    free_table(c);
    const int users_new = u_local > 0 ? (int)u_local : 1;
    rc = ensure_capacity(c, n_local, users_new);
    if (rc) { cleanup(); dfree(d_users); dfree(o_row); return rc; }
    if (n_local > 0) {
        PIE_TRY(hipMemcpyAsync(c->d_start, o_start, (size_t)n_local * 8, hipMemcpyDeviceToDevice, s));
        PIE_TRY(hipMemcpyAsync(c->d_end, o_end, (size_t)n_local * 8, hipMemcpyDeviceToDevice, s));
        PIE_TRY(hipMemcpyAsync(c->d_user, o_user, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s));
        PIE_TRY(hipMemcpyAsync(c->d_disc, o_disc, (size_t)n_local * 4, hipMemcpyDeviceToDevice, s));
        PIE_TRY(hipStreamSynchronize(s));
    }
#undef PIE_TRY
    cleanup();
    dfree(c->d_shard_rows);
    dfree(c->d_shard_users);
    c->d_shard_rows = o_row;
    c->d_shard_users = d_users;
    c->shard_rows_n = n_local;
    c->shard_users_n = (int)u_local;
    c->shard_rows_cap = (long long)rows;
    c->shard_users_cap = U;
    c->shard_rank = rank;
    c->shard_world = world;
    c->shard_rows_global = n;
    c->shard_users_global = U;
    c->shard_on = false;
    try {
        c->shard_users_h.assign((size_t)u_local, 0);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for the user map of %lld users", u_local);
    }
    if (u_local > 0) {
        PIE_HIP(c, hipMemcpyAsync(c->shard_users_h.data(), d_users, (size_t)u_local * 4, hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipStreamSynchronize(s));
    }
    c->shard_on = true;
    if (n_rows_out) *n_rows_out = (size_t)n_local;
    if (n_users_out) *n_users_out = users_new;
    rc = build_keys(c, 0);
    if (rc) return rc;
    PIE_HIP(c, hipStreamSynchronize(s));
    return PIE_OK;
}

int pie_shard_maps(pie_ctx* c, int32_t* rows_global_out, int32_t* users_global_out)
{
    if (!c) return PIE_E_INVAL;
    if (!c->d_shard_rows || !c->d_shard_users) return fail(c, PIE_E_STATE, "pie_shard_maps without pie_shard_table");
    PIE_HIP(c, hipSetDevice(c->device));
    if (rows_global_out && c->shard_rows_n)
        PIE_HIP(c, hipMemcpyAsync(rows_global_out, c->d_shard_rows, (size_t)c->shard_rows_n * 4, hipMemcpyDeviceToHost, c->stream));
    if (users_global_out && c->shard_users_n)
        PIE_HIP(c, hipMemcpyAsync(users_global_out, c->d_shard_users, (size_t)c->shard_users_n * 4, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return PIE_OK;
}

// ---- mutators by GLOBAL id on a sharded context (createSession / touchSession / deleteSession / deleteSessionsForUser,
// server/sessionStore.js:12-19,37-64, on the sharded form of the table).  Every shard is given the same call and keeps what is
// its own; nothing is exchanged.  The context stays in step with the unsharded table: its row map ascends and covers every
// local row, its user map is the ascending list of all global ids that hash to the rank (new ids are larger than all earlier
// ones, so both maps only ever grow at their ends and no local id moves).

// the table a call by GLOBAL id needs, in flight or not: both maps, the row map covering every local row
static int shard_table_ready(pie_ctx* c, const char* what)
{
    if (!c->shard_on || !c->d_shard_rows || !c->d_shard_users)
        return fail(c, PIE_E_STATE, "%s: the context holds no sharded table (pie_shard_table)", what);
    if (c->n != c->shard_rows_n)
        return fail(c, PIE_E_STATE, "%s: %lld rows were added after pie_shard_table: they have no global row", what, c->n - c->shard_rows_n);
    return PIE_OK;
}

static int shard_ready(pie_ctx* c, const char* what)
{
    int rc = shard_table_ready(c, what);
    if (rc) return rc;
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "%s while a scan is in flight", what);
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "a token turn is begun and not finished (pie_token_turn_finish)");
    return PIE_OK;
}

// Both device maps as large as the table's capacity (they grow with it, geometrically as it does).  The copy is waited for: an
// earlier queued touch may still read the old map, and this happens once per growth of the table.
static int shard_maps_reserve(pie_ctx* c, long long rows, long long users)
{
    hipStream_t s = c->stream;
    if (rows > c->shard_rows_cap || users > c->shard_users_cap) { // a token lookup begun earlier reads the maps that go
        const int rc = side_passes_land(c, "map growth"); // ... and the shard form of the expired queue in flight reads the row map
        if (rc) return rc;
    }
    if (rows > c->shard_rows_cap) {
        int* p = nullptr;
        PIE_HIP(c, hipMalloc(&p, (size_t)rows * 4));
        hipError_t e = c->shard_rows_n ? hipMemcpyAsync(p, c->d_shard_rows, (size_t)c->shard_rows_n * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(p); return fail(c, PIE_E_HIP, "row map growth: %s", hipGetErrorString(e)); }
        dfree(c->d_shard_rows);
        c->d_shard_rows = p;
        c->shard_rows_cap = rows;
    }
    if (users > c->shard_users_cap) {
        int* p = nullptr;
        PIE_HIP(c, hipMalloc(&p, (size_t)users * 4));
        hipError_t e = c->shard_users_n ? hipMemcpyAsync(p, c->d_shard_users, (size_t)c->shard_users_n * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hipFree(p); return fail(c, PIE_E_HIP, "user map growth: %s", hipGetErrorString(e)); }
        dfree(c->d_shard_users);
        c->d_shard_users = p;
        c->shard_users_cap = (int)users;
    }
    return PIE_OK;
}

static size_t shard_route_rows(const int32_t* user_global, size_t k, int32_t rank, int32_t world, uint8_t* keep)
{
    size_t n_kept = 0;
    for (size_t i = 0; i < k; ++i) {
        keep[i] = pie_shard_of(user_global[i], world) == rank ? 1 : 0;
        n_kept += keep[i];
    }
    return n_kept;
}

int pie_shard_route(const int32_t* user_global, size_t k, int32_t rank, int32_t world, uint8_t* keep_out, size_t* n_kept_out,
                    int32_t users_before, int32_t users_after, int32_t* new_users_out, size_t cap, size_t* n_new_out)
{
    if (n_kept_out) *n_kept_out = 0;
    if (n_new_out) *n_new_out = 0;
    if (world < 1 || rank < 0 || rank >= world || users_before < 0) return PIE_E_INVAL;
    if (k && (!user_global || !keep_out)) return PIE_E_INVAL;
    const size_t n_kept = shard_route_rows(user_global, k, rank, world, keep_out);
    if (n_kept_out) *n_kept_out = n_kept;
    size_t n_new = 0;
    for (int32_t u = users_before; u < users_after; ++u)
        if (pie_shard_of(u, world) == rank) {
            if (new_users_out && n_new < cap) new_users_out[n_new] = u;
            ++n_new;
        }
    if (n_new_out) *n_new_out = n_new;
    return n_new > cap ? PIE_E_CAPACITY : PIE_OK;
}

int pie_shard_info(pie_ctx* c, int32_t* rank_out, int32_t* world_out, int64_t* rows_global_out, int32_t* users_global_out, uint64_t* map_bytes_out)
{
    if (!c) return PIE_E_INVAL;
    if (!c->shard_on) return fail(c, PIE_E_STATE, "pie_shard_info: the context holds no sharded table (pie_shard_table)");
    if (rank_out) *rank_out = c->shard_rank;
    if (world_out) *world_out = c->shard_world;
    if (rows_global_out) *rows_global_out = c->shard_rows_global;
    if (users_global_out) *users_global_out = c->shard_users_global;
    if (map_bytes_out) *map_bytes_out = ((uint64_t)c->shard_rows_cap + (uint64_t)c->shard_users_cap) * 4u;
    return PIE_OK;
}

} // extern "C"

// What the calls below refuse, checked without staging or changing anything: the communicator asks every local shard first,
// so that a refused call changes none of them.
namespace pie_internal {
int shard_check_append(pie_ctx* c, const int32_t* user_global, size_t k, int32_t n_users_global)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_ready(c, "pie_shard_append_rows");
    if (rc) return rc;
    if (k > 0 && !user_global) return fail(c, PIE_E_INVAL, "NULL column pointer");
    if (n_users_global < c->shard_users_global)
        return fail(c, PIE_E_INVAL, "n_users_global may only grow (%d < %d)", n_users_global, c->shard_users_global);
    if (c->shard_rows_global + (long long)k >= (1LL << 31) - 1 || k >= ((size_t)1 << 31))
        return fail(c, PIE_E_INVAL, "global row count outside [0, 2^31 - 1)");
    for (size_t i = 0; i < k; ++i)
        if ((uint32_t)user_global[i] >= (uint32_t)n_users_global)
            return fail(c, PIE_E_INVAL, "row %zu carries a user id outside [0, %d)", i, n_users_global);
    return PIE_OK;
}

int shard_check_set_end(pie_ctx* c, const int32_t* rows_global, const int64_t* new_end, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_ready(c, "pie_shard_set_end");
    if (rc) return rc;
    if (k > 0 && (!rows_global || !new_end)) return fail(c, PIE_E_INVAL, "NULL pointer");
    for (size_t i = 0; i < k; ++i)
        if (rows_global[i] < 0 || (long long)rows_global[i] >= c->shard_rows_global)
            return fail(c, PIE_E_INVAL, "global row %d outside [0, %lld)", rows_global[i], c->shard_rows_global);
    return PIE_OK;
}
} // namespace pie_internal

extern "C" {

// the staging block of an append: [start kept | end kept | GLOBAL user kept | disc kept | global row kept | new users]
static void shard_append_stage(char* h, const int64_t* start, const int64_t* end, const int32_t* user_global, const int32_t* disc, size_t k,
                               const uint8_t* keep, size_t n_kept, long long first_row, int32_t users_before, int32_t users_after,
                               int32_t rank, int32_t world)
{
    int64_t* hs = reinterpret_cast<int64_t*>(h);
    int64_t* he = reinterpret_cast<int64_t*>(h + n_kept * 8);
    int32_t* hu = reinterpret_cast<int32_t*>(h + n_kept * 16);
    int32_t* hd = reinterpret_cast<int32_t*>(h + n_kept * 20);
    int32_t* hg = reinterpret_cast<int32_t*>(h + n_kept * 24);
    int32_t* hn = reinterpret_cast<int32_t*>(h + n_kept * 28);
    size_t j = 0;
    for (size_t i = 0; i < k; ++i)
        if (keep[i]) {
            hs[j] = start[i];
            he[j] = end[i];
            hu[j] = user_global[i];
            hd[j] = disc[i];
            hg[j] = (int32_t)(first_row + (long long)i);
            ++j;
        }
    j = 0;
    for (int32_t u = users_before; u < users_after; ++u)
        if (pie_shard_of(u, world) == rank) hn[j++] = u;
}

// Upload an append's block, extend the device user map by a sharded append's new users, zero the count a waited append reads
// back, and run the kernel on rows [row0, row0 + k).  with_keys false (the growth path of a sharded append): the four columns
// and the row map only, build_keys follows.
static int append_launch(pie_ctx* c, const Staged& st, size_t k, long long row0, int n_users, const ShardAppend* sh, bool with_keys)
{
    hipStream_t s = c->stream;
    PIE_HIP(c, hipMemcpyAsync(st.d, st.h, sh ? k * 28 + sh->n_new * 4 : k * 24, hipMemcpyHostToDevice, s));
    if (sh && sh->n_new)
        PIE_HIP(c, hipMemcpyAsync(c->d_shard_users + c->shard_users_n, st.d + k * 28, sh->n_new * 4, hipMemcpyDeviceToDevice, s));
    if (!st.a) PIE_HIP(c, hipMemsetAsync(&c->d_summary->bad_rows, 0, sizeof(unsigned int), s));
    if (k == 0) return PIE_OK;
    const long long *d_start = reinterpret_cast<const long long*>(st.d), *d_end = reinterpret_cast<const long long*>(st.d + k * 8);
    int* d_user = reinterpret_cast<int*>(st.d + k * 16);
    const int *d_disc = reinterpret_cast<const int*>(st.d + k * 20), *d_grow = reinterpret_cast<const int*>(st.d + k * 24);
    lkey_t* key = with_keys ? c->d_key : nullptr;
    fkey_t* fkey = with_keys ? c->d_fkey : nullptr;
    PayRec* pay = with_keys ? c->d_pay : nullptr;
    const HotMirror hot = with_keys ? hot_mirror_of(c) : HotMirror{};
    if (sh)
        hipLaunchKernelGGL(k_shard_append_rows, dim3(capped_grid(c, k)), dim3(256), 0, s, d_start, d_end, d_user, d_disc, d_grow, (long long)k, row0,
                           (const int*)c->d_shard_users, c->shard_users_n + (int)sh->n_new, c->d_start, c->d_end, c->d_user, c->d_disc,
                           c->d_shard_rows, key, c->key_base, c->key_shift, fkey, c->fkey_base, c->fkey_shift, pay, &c->d_summary->bad_rows, hot);
    else
        hipLaunchKernelGGL(k_append_rows, dim3(capped_grid(c, k)), dim3(256), 0, s, d_start, d_end, (const int*)d_user, d_disc, (long long)k, row0,
                           n_users, c->d_start, c->d_end, c->d_user, c->d_disc, key, c->key_base, c->key_shift, fkey, c->fkey_base,
                           c->fkey_shift, pay, &c->d_summary->bad_rows, hot);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

// The kernel is queued: the maps cover rows [0, old_n + n_kept) and the new users, the whole table is k rows longer.  This
// stands BEFORE the steps that move c->n and can still fail late (the ordered run's re-spread, the staging arrays, the key
// build), so that c->n and the map never part; a step that fails with c->n unmoved takes it back (shard_append_undo).
struct ShardUndo {
    long long rows_n, rows_global;
    int users_n, users_global;
    size_t users_h;
};
static int shard_append_commit(pie_ctx* c, const char* h, long long old_n, size_t n_kept, size_t n_new, size_t k, int32_t n_users_global,
                               ShardUndo* u)
{
    const int32_t* hn = reinterpret_cast<const int32_t*>(h + n_kept * 28);
    *u = ShardUndo{c->shard_rows_n, c->shard_rows_global, c->shard_users_n, c->shard_users_global, c->shard_users_h.size()};
    try {
        c->shard_users_h.insert(c->shard_users_h.end(), hn, hn + n_new);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for the user map");
    }
    c->shard_rows_n = old_n + (long long)n_kept;
    c->shard_users_n += (int)n_new;
    c->shard_rows_global += (long long)k;
    c->shard_users_global = n_users_global;
    return PIE_OK;
}
static void shard_append_undo(pie_ctx* c, const ShardUndo& u)
{
    c->shard_rows_n = u.rows_n;
    c->shard_rows_global = u.rows_global;
    c->shard_users_n = u.users_n;
    c->shard_users_global = u.users_global;
    c->shard_users_h.resize(u.users_h);
}

// The in-place path of pie_append_rows and pie_shard_append_rows from the filled staging block on: the kernel, the ordered run's
// append (waited form only: it reads the context's own staging block, where the sharded kernel has left LOCAL user ids), the
// shard's commit, then the queued or the waited tail.
static int append_in_place(pie_ctx* c, const Staged& st, size_t k, int n_users, const ShardAppend* sh)
{
    const long long old_n = c->n;
    int rc = append_launch(c, st, k, old_n, n_users, sh, true);
    if (rc) return rc;
    // the ordered run takes rows that arrive in time order into the spare slots of their users' segments
    bool ord_kept = false;
    if (c->ord.valid && c->ord.rows == old_n && k <= (size_t)kOrdAppendMax && n_users <= c->ord.users && c->key_ok) {
        launch_ord_append(c, c->stream, c->d_stage, k, old_n, n_users, 1); // pend[] is all zero between appends (build and re-spread leave it so)
        ord_kept = true;
    }
    ShardUndo undo{};
    if (sh) {
        rc = shard_append_commit(c, st.h, old_n, k, sh->n_new, sh->k_call, sh->n_users_global, &undo);
        if (rc) { // the kernels fed the hot index and the run rows the table will not hold
            c->hix.valid = false;
            if (ord_kept) ord_invalidate(c);
            return rc;
        }
    }
    rc = st.a ? append_queued_tail(c, st, old_n, k, n_users) : append_waited_tail(c, old_n, k, n_users, ord_kept, sh != nullptr);
    if (rc && sh && c->n == old_n) shard_append_undo(c, undo);
    return rc;
}

int pie_shard_append_rows(pie_ctx* c, const int64_t* start, const int64_t* end, const int32_t* user_global, const int32_t* disc,
                          size_t k, int32_t n_users_global, int32_t* first_row_out, size_t* n_kept_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_kept_out) *n_kept_out = 0;
    if (k > 0 && (!start || !end || !user_global || !disc)) return fail(c, PIE_E_INVAL, "NULL column pointer");
    int rc = pie_internal::shard_check_append(c, user_global, k, n_users_global);
    if (rc) return rc;
    PIE_HIP(c, hipSetDevice(c->device));
    const int32_t rank = c->shard_rank, world = c->shard_world, users_before = c->shard_users_global;
    const long long first_row = c->shard_rows_global, old_n = c->n;
    if (first_row_out) *first_row_out = (int32_t)first_row;
    // the host routes: pure arithmetic, so the number of rows kept is known with nothing read back
    try {
        c->shard_keep.resize(k);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu rows", k);
    }
    const uint8_t* keep = c->shard_keep.data();
    const size_t n_kept = shard_route_rows(user_global, k, rank, world, c->shard_keep.data());
    size_t n_new = 0;
    for (int32_t u = users_before; u < n_users_global; ++u) n_new += pie_shard_of(u, world) == rank ? 1 : 0;
    if (n_kept_out) *n_kept_out = n_kept;
    const long long users_after = (long long)c->shard_users_n + (long long)n_new;
    const int local_users = users_after > 0 ? (int)users_after : 1; // a shard with no user keeps n_users = 1
    if (n_kept == 0 && n_new == 0) { // nothing of this call is this shard's: the whole table still grew
        c->shard_rows_global += (long long)k;
        c->shard_users_global = n_users_global;
        return PIE_OK;
    }
    const size_t bytes = n_kept * 28 + n_new * 4 + 64;
    const ShardAppend sh{k, n_new, n_users_global};
    const bool in_place = n_kept > 0 && old_n > 0 && old_n + (long long)n_kept <= c->cap_rows && c->key_ok && n_kept <= ((size_t)1 << 24);
    Staged st{};
    if ((n_kept == 0 || in_place) && local_users <= c->cap_users) {
        rc = shard_maps_reserve(c, c->cap_rows, c->cap_users);
        if (rc) return rc;
        if (in_place) hot_reserve(c, (long long)n_kept);
        // rows and no wait where pie_append_rows has none; users alone are always queued (nothing of them is ever read back)
        rc = stage_mutation(c, bytes, !in_place || mutation_queued(c), &st);
        if (rc) return rc;
        shard_append_stage(st.h, start, end, user_global, disc, k, keep, n_kept, first_row, users_before, n_users_global, rank, world);
        if (in_place) return append_in_place(c, st, n_kept, local_users, &sh);
        // Only the user map grows: the new ids go behind it in stream order.  Not the n_kept == 0 case of append_in_place: no row
        // changed, so the keys stay clean and the plans stand, and the ordered run goes only when it has no room for the users.
        rc = append_launch(c, st, 0, old_n, local_users, &sh, true);
        if (rc == PIE_OK) rc = stage_queued(c, st);
        ShardUndo undo{};
        if (rc == PIE_OK) rc = shard_append_commit(c, st.h, old_n, 0, n_new, k, n_users_global, &undo);
        if (rc) return rc;
        if (local_users > c->n_users) { // as an in-place append that brings users and no row would leave the context
            if (c->ord.valid && local_users > c->ord.users) ord_invalidate(c);
            set_user_count(c, local_users);
            drop_results(c);
        }
        if (!c->async_mutations) PIE_HIP(c, hipStreamSynchronize(c->stream));
        return PIE_OK;
    }
    // growth path, as pie_append_rows: a larger table first (the maps with it), the rows behind the resident ones, then the keys
    rc = ensure_capacity(c, old_n + (long long)n_kept, local_users, old_n > 0 ? old_n : 1);
    if (rc == PIE_OK) rc = shard_maps_reserve(c, c->cap_rows, c->cap_users);
    if (rc == PIE_OK) rc = stage_mutation(c, bytes, false, &st);
    if (rc) return append_rollback(c, old_n, rc);
    shard_append_stage(st.h, start, end, user_global, disc, k, keep, n_kept, first_row, users_before, n_users_global, rank, world);
    rc = append_launch(c, st, n_kept, old_n, local_users, &sh, false);
    if (rc) return append_rollback(c, old_n, rc);
    PIE_HIP(c, hipMemcpyAsync(c->h_summary, c->d_summary, sizeof(Summary), hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    if (c->h_summary->bad_rows)
        return append_rollback(c, old_n, fail(c, PIE_E_INVAL, "%u rows carry a user id the shard's user map does not hold", c->h_summary->bad_rows));
    ShardUndo undo{};
    rc = shard_append_commit(c, st.h, old_n, n_kept, n_new, k, n_users_global, &undo);
    if (rc) return append_rollback(c, old_n, rc);
    return build_keys(c, old_n); // c->n and the map already agree, whatever this returns
}

int pie_shard_set_end(pie_ctx* c, const int32_t* rows_global, const int64_t* new_end, size_t k_given)
{
    if (!c) return PIE_E_INVAL;
    int rc = pie_internal::shard_check_set_end(c, rows_global, new_end, k_given);
    if (rc || k_given == 0) return rc;
    return set_end_apply(c, rows_global, new_end, k_given, true);
}

int pie_shard_delete_user(pie_ctx* c, int32_t user_global, int32_t* rows_global_out, size_t cap, size_t* n_deleted)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    int rc = shard_ready(c, "pie_shard_delete_user");
    if (rc) return rc;
    // unknown ids and other shards' users: a no-op, like the falsy-id guard (sessionStore.js:56-58)
    if (user_global < 0 || user_global >= c->shard_users_global || pie_shard_of(user_global, c->shard_world) != c->shard_rank) return PIE_OK;
    const std::vector<int32_t>& um = c->shard_users_h;
    const auto it = std::lower_bound(um.begin(), um.end(), user_global);
    if (it == um.end() || *it != user_global || c->n == 0) return PIE_OK;
    size_t k = 0;
    rc = row_list(c, kOneUser, false, (long long)(it - um.begin()), 0, nullptr, 0, &k, false); // the list stays in slot 0's out_idx
    if (rc) return rc;
    if (n_deleted) *n_deleted = k;
    if (!rows_global_out || k == 0) return PIE_OK;
    if (k > cap) return fail(c, PIE_E_CAPACITY, "list cap %zu < %zu", cap, k); // the rows are tombstoned all the same
    hipStream_t s = c->stream;
    int* list = c->slot[0].out_idx;
    const unsigned grid = capped_grid(c, k);
    hipLaunchKernelGGL(k_shard_rows_to_global, dim3(grid), dim3(256), 0, s, (const int*)list, list, (long long)k, (const int*)c->d_shard_rows, c->n);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(rows_global_out, list, k * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    return PIE_OK;
}

} // extern "C"

// pie_shard_delete_users in the pieces the communicator needs: the check, the run that leaves the ascending list of GLOBAL rows
// on the device (its length in *m_out), and the copy of that list.
namespace pie_internal {
int shard_check_delete_users(pie_ctx* c, const int32_t* users_global, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_ready(c, "pie_shard_delete_users");
    if (rc) return rc;
    if (k > 0 && !users_global) return fail(c, PIE_E_INVAL, "NULL user list");
    return PIE_OK;
}

int shard_delete_users_run(pie_ctx* c, const int32_t* users_global, size_t k, size_t* m_out, int32_t* per_user_out)
{
    *m_out = 0;
    int rc = shard_check_delete_users(c, users_global, k);
    if (rc || k == 0) return rc;
    if (per_user_out) memset(per_user_out, 0, k * 4);
    if (c->n == 0) return PIE_OK;
    // unknown ids, other shards' users and ids the map does not hold: skipped (-1), like the falsy-id guard (sessionStore.js:56-58)
    const std::vector<int32_t>& um = c->shard_users_h;
    std::vector<int32_t> local;
    try {
        local.assign(k, -1);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu user ids", k);
    }
    for (size_t i = 0; i < k; ++i) {
        const int32_t g = users_global[i];
        if (g < 0 || g >= c->shard_users_global || pie_shard_of(g, c->shard_world) != c->shard_rank) continue;
        const auto it = std::lower_bound(um.begin(), um.end(), g);
        if (it != um.end() && *it == g) local[i] = (int32_t)(it - um.begin());
    }
    return delete_users_run(c, local.data(), k, true, m_out, per_user_out);
}

int shard_delete_users_copy(pie_ctx* c, int32_t* rows_global_out, size_t m) { return delete_users_copy(c, rows_global_out, m, m); }
} // namespace pie_internal

extern "C" {

int pie_shard_delete_users(pie_ctx* c, const int32_t* users_global, size_t k, int32_t* rows_global_out, size_t cap, size_t* n_deleted,
                           int32_t* per_user_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    size_t m = 0;
    int rc = pie_internal::shard_delete_users_run(c, users_global, k, &m, per_user_out);
    if (rc) return rc;
    if (n_deleted) *n_deleted = m;
    return delete_users_copy(c, rows_global_out, cap, m); // refuses a list above cap; the rows are tombstoned all the same
}

// ---- pruneCalendarEvents / purgeExpiredArchives (server/storage/sqlProvider.js:956-968, 863-890, 991-1009) on a shard, answered
// in GLOBAL rows: the plain call's passes on the same table, the write pass storing row_map[row] (k_list_write<MODE, true>)
int pie_shard_prune_before(pie_ctx* c, int64_t cutoff, int32_t* rows_global_out, size_t cap, size_t* n_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_out) *n_out = 0;
    const int rc = shard_ready(c, "pie_shard_prune_before");
    if (rc) return rc;
    return prune_impl(c, cutoff, rows_global_out, cap, n_out, true, false);
}

int pie_shard_retention_purge(pie_ctx* c, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t* rows_global_out, size_t cap, size_t* n_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_out) *n_out = 0;
    const int rc = shard_ready(c, "pie_shard_retention_purge");
    if (rc) return rc;
    return retention_impl(c, now, months, tz_offset_ms, rows_global_out, cap, n_out, true, false);
}

int pie_shard_retention_purge_tz(pie_ctx* c, int64_t now, int32_t months, const int64_t* transitions_utc_ms, const int64_t* offsets_ms,
                                 int32_t n_transitions, int32_t* rows_global_out, size_t cap, size_t* n_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_out) *n_out = 0;
    const int rc = shard_ready(c, "pie_shard_retention_purge_tz");
    if (rc) return rc;
    return retention_tz_impl(c, now, months, transitions_utc_ms, offsets_ms, n_transitions, rows_global_out, cap, n_out, true, false);
}

} // extern "C"

// The three shard forms in the pieces the communicator needs: what a call would refuse, checked with nothing changed; the run
// that leaves the ascending GLOBAL rows in slot 0's out_idx and the LOCAL rows beside them in slot 1's; and where they are.
// kind 2: prune (a = cutoff), 3: retention under a fixed offset (a = now, tz_offset_ms), 4: under a zone table (a = now).
namespace pie_internal {
int shard_check_row_list(pie_ctx* c, int kind, int32_t months, int64_t tz_offset_ms, const int64_t* transitions, const int64_t* offsets,
                         int32_t n_transitions)
{
    if (!c) return PIE_E_INVAL;
    const char* what = kind == 2 ? "pie_shard_prune_before" : kind == 3 ? "pie_shard_retention_purge" : "pie_shard_retention_purge_tz";
    int rc = shard_ready(c, what);
    if (rc) return rc;
    if (kind == 3) return retention_check(c, months, tz_offset_ms);
    if (kind == 4) return retention_tz_check(c, months, transitions, offsets, n_transitions);
    return PIE_OK;
}

int shard_row_list_run(pie_ctx* c, int kind, int64_t a, int32_t months, int64_t tz_offset_ms, const int64_t* transitions, const int64_t* offsets,
                       int32_t n_transitions, size_t* m_out, const int32_t** rows_global_dev, const int32_t** rows_local_dev)
{
    *m_out = 0;
    int rc = shard_check_row_list(c, kind, months, tz_offset_ms, transitions, offsets, n_transitions);
    if (rc) return rc;
    if (kind == 2) rc = prune_impl(c, a, nullptr, 0, m_out, true, true);
    else if (kind == 3) rc = retention_impl(c, a, months, tz_offset_ms, nullptr, 0, m_out, true, true);
    else rc = retention_tz_impl(c, a, months, transitions, offsets, n_transitions, nullptr, 0, m_out, true, true);
    *rows_global_dev = c->slot[0].out_idx;
    *rows_local_dev = c->slot[1].out_idx;
    return rc;
}

// what pie_compact_rows would refuse before it moves anything, on a shard of a live sharded table
int shard_check_compact(pie_ctx* c, uint32_t flags)
{
    if (!c) return PIE_E_INVAL;
    const int rc = shard_ready(c, "pie_compact_rows");
    if (rc) return rc;
    if (flags & ~PIE_COMPACT_SHRINK) return fail(c, PIE_E_INVAL, "unknown compaction flags 0x%x", flags);
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    return PIE_OK;
}
} // namespace pie_internal

extern "C" {

static int shard_translate(pie_ctx* c, int32_t* rows_inout, size_t k, bool to_local, const char* what)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_ready(c, what);
    if (rc) return rc;
    if (k == 0) return PIE_OK;
    if (!rows_inout) return fail(c, PIE_E_INVAL, "NULL row list");
    PIE_HIP(c, hipSetDevice(c->device));
    rc = ensure_stage(c, k * 4);
    if (rc) return rc;
    hipStream_t s = c->stream;
    memcpy(c->h_stage, rows_inout, k * 4);
    PIE_HIP(c, hipMemcpyAsync(c->d_stage, c->h_stage, k * 4, hipMemcpyHostToDevice, s));
    int* d = reinterpret_cast<int*>(c->d_stage);
    const unsigned grid = capped_grid(c, k);
    if (to_local) hipLaunchKernelGGL(k_shard_rows_to_local, dim3(grid), dim3(256), 0, s, d, (long long)k, (const int*)c->d_shard_rows, c->n);
    else hipLaunchKernelGGL(k_shard_rows_to_global, dim3(grid), dim3(256), 0, s, (const int*)d, d, (long long)k, (const int*)c->d_shard_rows, c->n);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(c->h_stage, c->d_stage, k * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    memcpy(rows_inout, c->h_stage, k * 4);
    return PIE_OK;
}

int pie_shard_rows_to_local(pie_ctx* c, int32_t* rows_inout, size_t k) { return shard_translate(c, rows_inout, k, true, "pie_shard_rows_to_local"); }
int pie_shard_rows_to_global(pie_ctx* c, int32_t* rows_inout, size_t k) { return shard_translate(c, rows_inout, k, false, "pie_shard_rows_to_global"); }

// Rows per unit (= per wave) and the grid of the two compaction passes: every wave of every block owns one contiguous unit, a
// whole number of 128-row steps; the grid comes from the chip (8 blocks per CU: the passes are streams, and a wave keeps one
// step in flight), a small table gets as many units as it has steps.
static int token_after_compact(pie_ctx* c, long long n_old);

static void compact_plan(const pie_ctx* c, long long n, int* blocks_out, long long* rows_per_unit_out)
{
    long long blocks = (n + kCmpBlockRows - 1) / kCmpBlockRows;
    const long long most = (long long)(c->n_cus > 0 ? c->n_cus : 1) * 8;
    if (blocks > most) blocks = most;
    if (blocks < 1) blocks = 1;
    const long long units = blocks * kK1Waves;
    long long rpu = (n + units - 1) / units;
    rpu = (rpu + kCmpWaveRows - 1) / kCmpWaveRows * kCmpWaveRows;
    if (rpu < kCmpWaveRows) rpu = kCmpWaveRows;
    *blocks_out = (int)blocks;
    *rows_per_unit_out = rpu;
}

int pie_compact_geometry(pie_ctx* c, size_t n, int32_t* rows_per_wave_step_out, int32_t* rows_per_block_step_out, int64_t* rows_per_unit_out,
                         int32_t* blocks_out)
{
    if (!c) return PIE_E_INVAL;
    int blocks = 0;
    long long rpu = 0;
    compact_plan(c, (long long)n, &blocks, &rpu);
    if (rows_per_wave_step_out) *rows_per_wave_step_out = kCmpWaveRows;
    if (rows_per_block_step_out) *rows_per_block_step_out = kCmpBlockRows;
    if (rows_per_unit_out) *rows_per_unit_out = rpu;
    if (blocks_out) *blocks_out = blocks;
    return PIE_OK;
}

int pie_compact_rows(pie_ctx* c, int64_t dead_before, uint32_t flags, size_t* n_kept_out)
{
    if (!c) return PIE_E_INVAL;
    if (flags & ~PIE_COMPACT_SHRINK) return fail(c, PIE_E_INVAL, "unknown compaction flags 0x%x", flags);
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "no table loaded");
    if (c->n_flight || c->b_flight) return fail(c, PIE_E_STATE, "a scan is in flight");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = side_passes_land(c, "pie_compact_rows"); // token lookups and the expired queue begun on this numbering keep their answers
    if (rc) return rc;
    rc = sync_all(c); // queued appends and touches land first
    if (rc) return rc;
    hipStream_t s = c->stream;
    const long long n = c->n;
    const int users = c->n_users;
    const bool shrink = (flags & PIE_COMPACT_SHRINK) != 0;
    const bool sharded = c->d_shard_rows != nullptr;
    const bool shard_on = c->shard_on; // ensure_capacity below takes the compacted rows for a new table: it stays the shard it was
    int blocks = 0;
    long long rpu = 0;
    compact_plan(c, n, &blocks, &rpu);
    const int units = blocks * kK1Waves;
    int *d_cnt = nullptr, *m_new = nullptr, *m_old = nullptr, *o_user = nullptr, *o_disc = nullptr, *o_row = nullptr;
    long long *d_off = nullptr, *o_start = nullptr, *o_end = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto cleanup = [&]() {
        dfree(d_cnt); dfree(d_off); dfree(m_new); dfree(m_old);
        dfree(o_start); dfree(o_end); dfree(o_user); dfree(o_disc); dfree(o_row);
        for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    };
#define PIE_TRY(call)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            cleanup();                                                                                \
            return fail(c, e_ == hipErrorOutOfMemory ? PIE_E_NOMEM : PIE_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
        }                                                                                             \
    } while (0)
    for (hipEvent_t& e : ev) PIE_TRY(hipEventCreate(&e));
    // 1. how many rows every unit keeps -> where its rows go
    PIE_TRY(hipMalloc(&d_cnt, (size_t)units * 4));
    PIE_TRY(hipMalloc(&d_off, ((size_t)units + 1) * 8));
    PIE_TRY(hipMalloc(&m_new, (size_t)(n > 0 ? n : 1) * 4));
    PIE_TRY(hipEventRecord(ev[0], s));
    hipLaunchKernelGGL(k_compact_count, dim3(blocks), dim3(256), 0, s, c->d_end, n, rpu, (long long)dead_before, d_cnt);
    // one block's sweep holds a few thousand counts; beyond that the two-level form (a chunk per thread, one block-wide scan)
    if (units <= 4096) hipLaunchKernelGGL(k_block_prefix, dim3(1), dim3(256), 0, s, d_cnt, units, d_off, (unsigned long long*)nullptr);
    else hipLaunchKernelGGL(k_block_prefix_wide, dim3(1), dim3(1024), 0, s, d_cnt, units, d_off, (unsigned long long*)nullptr, (HostSummary*)nullptr, 0ull);
    PIE_TRY(hipGetLastError());
    PIE_TRY(hipEventRecord(ev[1], s)); // the count pass ends here: the copy, the wait and the allocations below are host time
    long long kept = 0;
    PIE_TRY(hipMemcpyAsync(&kept, d_off + units, 8, hipMemcpyDeviceToHost, s));
    PIE_TRY(hipStreamSynchronize(s));
    if (kept < 0 || kept > n) { cleanup(); return fail(c, PIE_E_HIP, "compaction counted %lld kept rows of %lld", kept, n); }
    const size_t rows_kept = (size_t)(kept > 0 ? kept : 1);
    PIE_TRY(hipMalloc(&m_old, rows_kept * 4));
    const bool same = kept == n && !(shrink && c->cap_rows > (long long)rows_kept);
    long long shard_kept = 0;
    float ms_count = 0, ms_write = 0;
    if (same) {
        // nothing to move: the columns, their keys and everything derived from them stay as they are
        PIE_TRY(hipEventRecord(ev[2], s));
        if (n > 0) hipLaunchKernelGGL(k_compact_identity, dim3(c->n_cus * 8), dim3(256), 0, s, n, m_new, m_old);
        PIE_TRY(hipGetLastError());
        PIE_TRY(hipEventRecord(ev[3], s));
        PIE_TRY(hipStreamSynchronize(s));
    } else {
        // 2. the kept rows into fresh columns: of the table's capacity (swapped in below), or of the kept rows (a right-sized table)
        const size_t rows_out = shrink ? rows_kept : (size_t)c->cap_rows;
        PIE_TRY(hipMalloc(&o_start, rows_out * 8));
        PIE_TRY(hipMalloc(&o_end, rows_out * 8));
        PIE_TRY(hipMalloc(&o_user, rows_out * 4));
        PIE_TRY(hipMalloc(&o_disc, rows_out * 4));
        if (sharded) PIE_TRY(hipMalloc(&o_row, rows_kept * 4));
        PIE_TRY(hipEventRecord(ev[2], s));
        if (n > 0) hipLaunchKernelGGL(k_compact_write, dim3(blocks), dim3(256), 0, s, c->d_start, c->d_end, c->d_user, c->d_disc,
                                      (const int*)c->d_shard_rows, c->shard_rows_n, n, rpu, (long long)dead_before, d_off, o_start, o_end, o_user,
                                      o_disc, o_row, m_new, m_old);
        PIE_TRY(hipGetLastError());
        PIE_TRY(hipEventRecord(ev[3], s));
        PIE_TRY(hipStreamSynchronize(s));
        if (sharded) {
            // rows appended after pie_shard_table have no global row and sit behind the mapped ones, before and after: the map
            // now covers the kept rows among the first shard_rows_n, i.e. the new rows whose old row lies below shard_rows_n
            if (c->shard_rows_n >= n) shard_kept = kept;
            else {
                hipLaunchKernelGGL(k_compact_lower_bound, dim3(1), dim3(1), 0, s, (const int*)m_old, kept, c->shard_rows_n, d_off);
                PIE_TRY(hipGetLastError());
                PIE_TRY(hipMemcpyAsync(&shard_kept, d_off, 8, hipMemcpyDeviceToHost, s));
                PIE_TRY(hipStreamSynchronize(s));
            }
        }
    }
    PIE_TRY(hipEventElapsedTime(&ms_count, ev[0], ev[1]));
    PIE_TRY(hipEventElapsedTime(&ms_write, ev[2], ev[3]));
#undef PIE_TRY
    if (!same) {
        // 3. the table takes the new columns: as a new table of the same users (what the last scans learned is forgotten, the
        // ordered run is invalid, results and queues are gone), in the old capacity or a right-sized one
        c->tokx.hold = c->tokx.tok != nullptr; // the token column outlives the ensure_capacity below: token_after_compact renumbers it
        if (shrink) {
            // the kept rows already sit in right-sized columns: the new table is built around them (as in pie_shard_table, a
            // failure past this point leaves the context without a table)
            free_table(c);
            c->adopt_start = o_start; c->adopt_end = o_end; c->adopt_user = o_user; c->adopt_disc = o_disc;
            o_start = o_end = nullptr;
            o_user = o_disc = nullptr;
            rc = ensure_capacity(c, kept, users);
            dfree(c->adopt_start); dfree(c->adopt_end); dfree(c->adopt_user); dfree(c->adopt_disc); // taken (null by now) unless it failed early
            if (rc) { token_drop(c); cleanup(); return rc; }
        } else {
            rc = ensure_capacity(c, kept, users);
            if (rc) { token_drop(c); cleanup(); return rc; }
            dfree(c->d_start); dfree(c->d_end); dfree(c->d_user); dfree(c->d_disc);
            c->d_start = o_start; c->d_end = o_end; c->d_user = o_user; c->d_disc = o_disc;
            o_start = o_end = nullptr;
            o_user = o_disc = nullptr;
        }
        if (sharded) {
            dfree(c->d_shard_rows);
            c->d_shard_rows = o_row;
            o_row = nullptr;
            c->shard_rows_n = shard_kept;
            c->shard_rows_cap = (long long)rows_kept;
        }
        c->shard_on = shard_on;
    } else {
        cmp_forget(c);
    }
    // results name rows by index, and so does a dispatch queue: whatever is left of earlier calls is forgotten
    queue_forget(c);
    c->res = nullptr;
    for (Slot& sl : c->slot) sl.have_result = false;
    c->bres = nullptr;
    for (BatchSlot& b : c->bslot) b.have_result = false;
    c->d_cmp_new_of_old = m_new;
    c->d_cmp_old_of_new = m_old;
    m_new = m_old = nullptr;
    c->cmp_n_old = n;
    c->cmp_n_kept = kept;
    c->cmp_valid = true;
    c->compactions++;
    c->cmp_write_ms = (double)ms_write;
    c->cmp_count_ms = (double)ms_count;
    cleanup();
    if (n_kept_out) *n_kept_out = (size_t)kept;
    if (same) return PIE_OK;
    rc = build_keys(c, 0);
    if (rc) { token_drop(c); return rc; }
    PIE_HIP(c, hipStreamSynchronize(s));
    return token_after_compact(c, n);
}

int pie_compact_maps(pie_ctx* c, int32_t* new_of_old_out, int32_t* old_of_new_out, size_t* n_old_out, size_t* n_kept_out)
{
    if (!c) return PIE_E_INVAL;
    if (!c->cmp_valid) return fail(c, PIE_E_STATE, "no compaction maps: the rows were renumbered since, or never compacted");
    PIE_HIP(c, hipSetDevice(c->device));
    if (new_of_old_out && c->cmp_n_old)
        PIE_HIP(c, hipMemcpyAsync(new_of_old_out, c->d_cmp_new_of_old, (size_t)c->cmp_n_old * 4, hipMemcpyDeviceToHost, c->stream));
    if (old_of_new_out && c->cmp_n_kept)
        PIE_HIP(c, hipMemcpyAsync(old_of_new_out, c->d_cmp_old_of_new, (size_t)c->cmp_n_kept * 4, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    if (n_old_out) *n_old_out = (size_t)c->cmp_n_old;
    if (n_kept_out) *n_kept_out = (size_t)c->cmp_n_kept;
    return PIE_OK;
}

int pie_compact_map_device_ptrs(pie_ctx* c, void** new_of_old_dev, void** old_of_new_dev, size_t* n_old_out, size_t* n_kept_out)
{
    if (!c) return PIE_E_INVAL;
    if (!c->cmp_valid) return fail(c, PIE_E_STATE, "no compaction maps: the rows were renumbered since, or never compacted");
    if (new_of_old_dev) *new_of_old_dev = c->d_cmp_new_of_old;
    if (old_of_new_dev) *old_of_new_dev = c->d_cmp_old_of_new;
    if (n_old_out) *n_old_out = (size_t)c->cmp_n_old;
    if (n_kept_out) *n_kept_out = (size_t)c->cmp_n_kept;
    return PIE_OK;
}

int pie_compact_translate(pie_ctx* c, int32_t* rows_inout, size_t k)
{
    if (!c) return PIE_E_INVAL;
    if (!c->cmp_valid) return fail(c, PIE_E_STATE, "no compaction maps: the rows were renumbered since, or never compacted");
    if (k == 0) return PIE_OK;
    if (!rows_inout) return fail(c, PIE_E_INVAL, "NULL row list");
    PIE_HIP(c, hipSetDevice(c->device));
    int rc = ensure_stage(c, k * 4);
    if (rc) return rc;
    hipStream_t s = c->stream;
    memcpy(c->h_stage, rows_inout, k * 4);
    PIE_HIP(c, hipMemcpyAsync(c->d_stage, c->h_stage, k * 4, hipMemcpyHostToDevice, s));
    const unsigned grid = capped_grid(c, k);
    hipLaunchKernelGGL(k_compact_translate, dim3(grid), dim3(256), 0, s, reinterpret_cast<int*>(c->d_stage), (long long)k,
                       (const int*)c->d_cmp_new_of_old, c->cmp_n_old);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(c->h_stage, c->d_stage, k * 4, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    memcpy(rows_inout, c->h_stage, k * 4);
    return PIE_OK;
}

int pie_batch_mask_codes(const pie_query* queries, int n_q, const uint8_t* fallback, int32_t n_disc, const int64_t* start, const int64_t* end,
                         const int32_t* disc, size_t n_rows, uint32_t* code_out, uint64_t* mask_out)
{
    if (!queries || n_q < 1 || n_q > kBatchMax || n_disc < 1 || n_disc > 64 || (n_rows && (!start || !end || !disc))) return PIE_E_INVAL;
    bool fb[kBatchMax];
    unsigned nk[kBatchMax];
    for (int q = 0; q < kBatchMax; ++q) { fb[q] = q < n_q && fallback && fallback[q]; nk[q] = 0; }
    BatchTables t;
    fill_batch_tables(n_disc, n_q, fb, queries, nk, t);
    for (size_t i = 0; i < n_rows; ++i) {
        if ((uint32_t)disc[i] >= 64u) return PIE_E_INVAL;
        int r = 0, w = 0; // as the pass ranks a row: the queries with now < end, the queries with cutoff <= start
        for (int k = 0; k < kBatchMax; ++k) { r += t.now[k] < end[i] ? 1 : 0; w += t.cutoff[k] <= start[i] ? 1 : 0; }
        const int code = mask_code(r, w, disc[i]);
        if (code_out) code_out[i] = (uint32_t)code;
        if (mask_out) mask_out[i] = mask_of_code(t.live, code);
    }
    return PIE_OK;
}

int32_t pie_shard_of(int32_t user, int32_t n_shards) { return shard_of(user, n_shards); }

// ---- the token column and its index (pie_token.h): getSession / touchSession / deleteSession by token hash ------------------
// Everything is queued on the context's stream.  The host tracks `covered` and the slot count; the device tracks nothing but the
// status words, which a lookup brings back with its results (an exhausted probe bound of an earlier, un-waited insert included).

size_t pie_token_slots_for(size_t covered)
{
    size_t s = 1024;
    while (s / 2 < covered && (s << 1) != 0) s <<= 1;
    return s;
}

int pie_token_homes(const uint64_t* tok, size_t k, uint32_t log2_slots, uint32_t* home_out)
{
    if (log2_slots > 32 || (k && (!tok || !home_out))) return PIE_E_INVAL;
    for (size_t i = 0; i < k; ++i) home_out[i] = (uint32_t)token_home(tok[2 * i], tok[2 * i + 1], log2_slots);
    return PIE_OK;
}

static unsigned token_log2(size_t slots)
{
    unsigned b = 0;
    while (((size_t)1 << b) < slots) ++b;
    return b;
}

// the checks every pie_token_* call that takes a context begins with; idle = false: the call runs beside scans and batches
static int token_ready(pie_ctx* c, const char* what, bool need_column, bool idle = true)
{
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "%s: no table loaded", what);
    if (idle && (c->n_flight || c->b_flight)) return fail(c, PIE_E_STATE, "%s while a scan or batch is in flight", what);
    if (need_column && !c->tokx.tok) return fail(c, PIE_E_STATE, "%s: the table has no token column (pie_token_set gives it one)", what);
    return PIE_OK;
}

static int token_status_alloc(pie_ctx* c)
{
    if (c->tokx.status) return PIE_OK;
    PIE_HIP(c, hipMalloc(&c->tokx.status, kTokStatusWords * sizeof(unsigned int)));
    PIE_HIP(c, hipMemsetAsync(c->tokx.status, 0, kTokStatusWords * sizeof(unsigned int), c->stream));
    return PIE_OK;
}

// st[] = the status words as read back behind a waited call: set -> cleared on the device, PIE_E_HIP
static int token_status_check(pie_ctx* c, const unsigned int* st, const char* what)
{
    if (!st[0] && !st[1] && !st[2]) return PIE_OK;
    (void)hipMemsetAsync(c->tokx.status, 0, kTokStatusWords * sizeof(unsigned int), c->stream);
    if (st[2]) return fail(c, PIE_E_HIP, "%s: a create names a user the shard's user map does not hold", what);
    return fail(c, PIE_E_HIP, "%s: probe bound exhausted (%s ran %llu steps without meeting an empty slot)", what,
                st[0] ? "an insert" : "a lookup", 1ull << c->tokx.log2_slots);
}

static int token_status_wait(pie_ctx* c, const char* what)
{
    unsigned int st[kTokStatusWords] = {};
    PIE_HIP(c, hipMemcpyAsync(st, c->tokx.status, sizeof st, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return token_status_check(c, st, what);
}

static int token_insert(pie_ctx* c, long long row0, long long k)
{
    pie_ctx::TokenIndex& t = c->tokx;
    if (k <= 0) return PIE_OK;
    hipLaunchKernelGGL(k_token_insert, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, c->stream, (const TokKey*)t.tok, row0, k, t.slot_row,
                       t.log2_slots, t.status);
    PIE_HIP(c, hipGetLastError());
    return PIE_OK;
}

// every slot empty, then the rows [0, rows) inserted (the covered rows: `covered`, or a shard's covered_l); queued, timed by two
// events (pie_table_info.token_build_ms)
static int token_rebuild(pie_ctx* c, long long rows)
{
    pie_ctx::TokenIndex& t = c->tokx;
    for (hipEvent_t& e : t.ev)
        if (!e) PIE_HIP(c, hipEventCreate(&e));
    PIE_HIP(c, hipEventRecord(t.ev[0], c->stream));
    PIE_HIP(c, hipMemsetAsync(t.slot_row, 0xFF, (size_t)4 << t.log2_slots, c->stream));
    int rc = token_insert(c, 0, rows);
    if (rc) return rc;
    PIE_HIP(c, hipEventRecord(t.ev[1], c->stream));
    t.timed = true;
    t.builds++;
    return PIE_OK;
}

// Room for a plain column to cover `covered` rows (pie_token_append, pie_session_turn): a column as long as the table's capacity
// (the table grew) and slots that stay at most half full — a larger table of slots is rebuilt from the rows covered NOW, the
// caller inserts the rest.  Both free what a lookup begun earlier (pie_token_lookup_begin) reads: those land first.  May wait.
static int token_make_room(pie_ctx* c, long long covered, const char* what)
{
    pie_ctx::TokenIndex& t = c->tokx;
    hipStream_t s = c->stream;
    const bool longer = c->cap_rows > t.cap, grow = (unsigned long long)covered > ((1ull << t.log2_slots) >> 1);
    if (!longer && !grow) return PIE_OK;
    int rc = token_lookups_land(c, what);
    if (rc) return rc;
    // the allocations first: a failure leaves what was there
    TokKey* nt = nullptr;
    int* ns = nullptr;
    const unsigned log2_slots = grow ? token_log2(pie_token_slots_for((size_t)covered)) : t.log2_slots;
    if ((longer && hipMalloc(&nt, (size_t)c->cap_rows * sizeof(TokKey)) != hipSuccess) || (grow && hipMalloc(&ns, (size_t)4 << log2_slots) != hipSuccess)) {
        (void)hipGetLastError();
        dfree(nt);
        return fail(c, PIE_E_NOMEM, "%s: no device memory for %lld keys and %llu slots", what, c->cap_rows, 1ull << log2_slots);
    }
    hipError_t e = longer && t.covered ? hipMemcpyAsync(nt, t.tok, (size_t)t.covered * sizeof(TokKey), hipMemcpyDeviceToDevice, s) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(s); // the copy has run; inserts queued earlier still write the table of slots that goes
    if (e != hipSuccess) {
        dfree(nt);
        dfree(ns);
        return fail(c, PIE_E_HIP, "%s: %s", what, hipGetErrorString(e));
    }
    if (longer) {
        dfree(t.tok);
        t.tok = nt;
        t.cap = c->cap_rows;
    }
    if (!grow) return PIE_OK;
    dfree(t.slot_row);
    t.slot_row = ns;
    t.log2_slots = log2_slots;
    return token_rebuild(c, t.covered);
}

// A sharded column's covered_l = lower_bound(rows_map, mapped rows, covered_g): one thread on the device, read back and waited for.
static int shard_token_covered(pie_ctx* c, long long* covered_l)
{
    pie_ctx::TokenIndex& t = c->tokx;
    *covered_l = 0;
    if (c->shard_rows_n <= 0 || t.covered_g <= 0 || !c->d_shard_rows) return PIE_OK;
    hipStream_t s = c->stream;
    long long got = -1;
    hipLaunchKernelGGL(k_compact_lower_bound, dim3(1), dim3(1), 0, s, (const int*)c->d_shard_rows, c->shard_rows_n, t.covered_g, c->d_range);
    PIE_HIP(c, hipGetLastError());
    PIE_HIP(c, hipMemcpyAsync(&got, c->d_range, 8, hipMemcpyDeviceToHost, s));
    PIE_HIP(c, hipStreamSynchronize(s));
    if (got < 0 || got > c->shard_rows_n || got > t.cap) return fail(c, PIE_E_HIP, "token column: %lld covered rows of %lld", got, c->shard_rows_n);
    *covered_l = got;
    return PIE_OK;
}

static int token_info(pie_ctx* c, pie_table_info* out)
{
    pie_ctx::TokenIndex& t = c->tokx;
    long long covered = t.covered;
    if (t.tok && t.sharded) {
        PIE_HIP(c, hipSetDevice(c->device));
        int rc = shard_token_covered(c, &covered);
        if (rc) return rc;
    }
    out->token_rows = t.tok ? (uint64_t)covered : 0u;
    out->token_bytes = (uint64_t)t.cap * sizeof(TokKey) + (t.slot_row ? (uint64_t)4 << t.log2_slots : 0u) +
                       (t.status ? kTokStatusWords * sizeof(unsigned int) : 0u) + (uint64_t)t.stage_bytes;
    for (const auto& l : t.lk) out->token_bytes += (uint64_t)l.bytes;
    for (const auto& u : t.tn) out->token_bytes += (uint64_t)u.bytes;
    out->token_builds = t.builds;
    if (t.timed) { // the last build's device time, read once it has run
        float ms = 0.f;
        if (hipEventSynchronize(t.ev[1]) == hipSuccess && hipEventElapsedTime(&ms, t.ev[0], t.ev[1]) == hipSuccess) t.build_ms = ms;
        else (void)hipGetLastError();
        t.timed = false;
    }
    out->token_build_ms = t.build_ms;
    return PIE_OK;
}

int pie_token_set(pie_ctx* c, const uint64_t* tok, size_t n)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_set", false);
    if (rc) return rc;
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "%s: a token turn is begun and not finished (pie_token_turn_finish)", "pie_token_set");
    if (c->shard_on) return fail(c, PIE_E_STATE, "pie_token_set: a sharded context carries no token column");
    if (n > 0 && !tok) return fail(c, PIE_E_INVAL, "tok is NULL");
    if ((long long)n > c->n || n > (size_t)c->n) return fail(c, PIE_E_INVAL, "%zu keys for a table of %lld rows", n, c->n);
    PIE_HIP(c, hipSetDevice(c->device));
    rc = token_status_alloc(c);
    if (rc) return rc;
    pie_ctx::TokenIndex& t = c->tokx;
    // the new column and table first: a failure leaves what was there
    const unsigned log2_slots = token_log2(pie_token_slots_for(n));
    TokKey* nt = nullptr;
    int* ns = nullptr;
    if (hipMalloc(&nt, (size_t)c->cap_rows * sizeof(TokKey)) != hipSuccess || hipMalloc(&ns, (size_t)4 << log2_slots) != hipSuccess) {
        (void)hipGetLastError();
        dfree(nt);
        return fail(c, PIE_E_NOMEM, "pie_token_set: no device memory for %lld keys and %llu slots", c->cap_rows, 1ull << log2_slots);
    }
    token_drop(c);
    t.tok = nt;
    t.cap = c->cap_rows;
    t.slot_row = ns;
    t.log2_slots = log2_slots;
    t.covered = (long long)n;
    if (n > 0) PIE_HIP(c, hipMemcpyAsync(t.tok, tok, n * sizeof(TokKey), hipMemcpyHostToDevice, c->stream));
    rc = token_rebuild(c, t.covered);
    if (rc) return rc;
    return token_status_wait(c, "pie_token_set");
}

int pie_token_append(pie_ctx* c, const uint64_t* tok, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_append", true);
    if (rc) return rc;
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "%s: a token turn is begun and not finished (pie_token_turn_finish)", "pie_token_append");
    if (c->tokx.sharded) return fail(c, PIE_E_STATE, "pie_token_append: the column was given by global row (pie_shard_token_append)");
    if (k > 0 && !tok) return fail(c, PIE_E_INVAL, "tok is NULL");
    pie_ctx::TokenIndex& t = c->tokx;
    if (k > (size_t)(c->n - t.covered)) return fail(c, PIE_E_INVAL, "%zu keys behind %lld covered rows of a table of %lld", k, t.covered, c->n);
    if (k == 0) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const long long covered = t.covered + (long long)k;
    // everything that can fail comes first: the staging area, a longer column (the table grew), a larger table of slots
    const bool staged = k <= ((size_t)1 << 20);
    Staged st{};
    if (staged && (rc = stage_mutation(c, k * sizeof(TokKey), true, &st)) != PIE_OK) return rc;
    if ((rc = token_make_room(c, covered, "pie_token_append")) != PIE_OK) return rc;
    hipError_t e;
    if (staged) {
        memcpy(st.h, tok, k * sizeof(TokKey));
        e = hipMemcpyAsync(t.tok + t.covered, st.h, k * sizeof(TokKey), hipMemcpyHostToDevice, s);
    } else { // a bulk load (tools): straight from the caller's memory, waited for
        e = hipMemcpyAsync(t.tok + t.covered, tok, k * sizeof(TokKey), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
    if (e != hipSuccess) return fail(c, PIE_E_HIP, "pie_token_append: %s", hipGetErrorString(e));
    if (staged && (rc = stage_queued(c, st)) != PIE_OK) return rc;
    const long long row0 = t.covered;
    t.covered = covered;
    return token_insert(c, row0, (long long)k);
}

// rows the column can hold keys for: what keeps a probe's 16-byte load inside it
static long long token_bound(const pie_ctx* c)
{
    const pie_ctx::TokenIndex& t = c->tokx;
    if (!t.sharded) return t.covered;
    return c->n < t.cap ? c->n : t.cap;
}

// tokx.h_stage / d_stage hold at least `bytes` (they grow by doubling; growing waits for what still uses the old pair)
static int token_stage_room(pie_ctx* c, size_t bytes)
{
    pie_ctx::TokenIndex& t = c->tokx;
    if (bytes <= t.stage_bytes) return PIE_OK;
    size_t want = t.stage_bytes ? t.stage_bytes : (size_t)64 << 10;
    while (want < bytes) want *= 2;
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    if (t.h_stage) (void)hipHostFree(t.h_stage);
    dfree(t.d_stage);
    t.h_stage = nullptr;
    t.stage_bytes = 0;
    PIE_HIP(c, hipHostMalloc(&t.h_stage, want, hipHostMallocDefault));
    PIE_HIP(c, hipMalloc(&t.d_stage, want));
    t.stage_bytes = want;
    return PIE_OK;
}

// the results and the context's status words come back into tokx.h_stage: queued, not waited for
static int token_stage_download(pie_ctx* c, const TokStage& o)
{
    pie_ctx::TokenIndex& t = c->tokx;
    PIE_HIP(c, hipMemcpyAsync(t.h_stage + o.res.end, t.d_stage + o.res.end, o.status - o.res.end, hipMemcpyDeviceToHost, c->stream));
    PIE_HIP(c, hipMemcpyAsync(t.h_stage + o.status, t.status, kTokStatusBytes, hipMemcpyDeviceToHost, c->stream));
    return PIE_OK;
}

// The queue phase of a lookup: the keys go up, one launch for k keys, the results and the status words come back into
// tokx.h_stage (lookup_stage_of) — all queued on the stream, nothing waited for.  global: the sharded kernel, which also answers
// the global row and translates the user.
static int token_lookup_queue(pie_ctx* c, const uint64_t* tok, size_t k, long long now, bool want_user, bool want_start, bool global)
{
    pie_ctx::TokenIndex& t = c->tokx;
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const TokStage o = lookup_stage_of(k, global);
    int rc = token_stage_room(c, o.bytes);
    if (rc) return rc;
    char* d = t.d_stage;
    memcpy(t.h_stage, tok, o.up);
    PIE_HIP(c, hipMemcpyAsync(d, t.h_stage, o.up, hipMemcpyHostToDevice, s));
    const dim3 grid((unsigned)((k + 255) / 256));
    int* o_user = want_user ? stage_at<int>(d, o.res.user) : nullptr;
    long long* o_start = want_start ? stage_at<long long>(d, o.res.start) : nullptr;
    if (global)
        hipLaunchKernelGGL(k_shard_token_lookup, grid, dim3(256), 0, s, stage_at<const TokKey>(d, 0), (long long)k, (const int*)t.slot_row,
                           t.log2_slots, (const TokKey*)t.tok, token_bound(c), (const long long*)c->d_end, (const long long*)c->d_start,
                           (const int*)c->d_user, (const int*)c->d_shard_rows, c->shard_rows_n, (const int*)c->d_shard_users, c->shard_users_n, now,
                           stage_at<int>(d, o.res.row), stage_at<int>(d, o.grow), stage_at<unsigned char>(d, o.res.live), o_user, o_start,
                           stage_at<long long>(d, o.res.end), t.status);
    else
        hipLaunchKernelGGL(k_token_lookup, grid, dim3(256), 0, s, stage_at<const TokKey>(d, 0), (long long)k, (const int*)t.slot_row,
                           t.log2_slots, (const TokKey*)t.tok, token_bound(c), (const long long*)c->d_end, (const long long*)c->d_start,
                           (const int*)c->d_user, now, stage_at<int>(d, o.res.row), stage_at<unsigned char>(d, o.res.live), o_user, o_start,
                           stage_at<long long>(d, o.res.end), t.status);
    PIE_HIP(c, hipGetLastError());
    return token_stage_download(c, o);
}

// The wait phase: the one wait of a lookup; the results and the status words are in tokx.h_stage when it returns.
static int token_lookup_wait(pie_ctx* c, size_t k, bool global, const char* what)
{
    PIE_HIP(c, hipSetDevice(c->device));
    PIE_HIP(c, hipStreamSynchronize(c->stream));
    return token_status_check(c, stage_at<const unsigned int>(c->tokx.h_stage, lookup_stage_of(k, global).status), what);
}

static int token_lookup_run(pie_ctx* c, const uint64_t* tok, size_t k, long long now, bool want_user, bool want_start, const char* what)
{
    int rc = token_lookup_queue(c, tok, k, now, want_user, want_start, false);
    if (rc) return rc;
    return token_lookup_wait(c, k, false, what);
}

int pie_token_lookup(pie_ctx* c, const uint64_t* tok, size_t k, int64_t now, int32_t* row_out, uint8_t* live_out, int32_t* user_out,
                     int64_t* start_out, int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_lookup", true);
    if (rc) return rc;
    if (k == 0) return PIE_OK;
    if (!tok) return fail(c, PIE_E_INVAL, "tok is NULL");
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%zu keys in one lookup", k);
    rc = token_lookup_run(c, tok, k, (long long)now, user_out != nullptr, start_out != nullptr, "pie_token_lookup");
    if (rc) return rc;
    token_results_out(c->tokx.h_stage, lookup_stage_of(k).res, k, row_out, live_out, user_out, start_out, end_out);
    return PIE_OK;
}

// lookup, read the rows back, then pie_set_end's own path on the elements that qualify: no `end` kernel of its own
int pie_token_set_end(pie_ctx* c, const uint64_t* tok, const int64_t* new_end, size_t k, int64_t now, int32_t* rows_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_set_end", true);
    if (rc) return rc;
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "%s: a token turn is begun and not finished (pie_token_turn_finish)", "pie_token_set_end");
    if (k == 0) return PIE_OK;
    if (!tok || !new_end) return fail(c, PIE_E_INVAL, "NULL pointer");
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%zu keys in one call", k);
    rc = token_lookup_run(c, tok, k, (long long)now, false, false, "pie_token_set_end");
    if (rc) return rc;
    const TokStage o = lookup_stage_of(k);
    const int32_t* row = stage_at<const int32_t>(c->tokx.h_stage, o.res.row);
    const uint8_t* live = stage_at<const uint8_t>(c->tokx.h_stage, o.res.live);
    std::vector<int32_t> rows;
    std::vector<int64_t> ends;
    try {
        rows.reserve(k);
        ends.reserve(k);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu touches", k);
    }
    for (size_t i = 0; i < k; ++i) {
        const bool hit = live[i] != 0 && row[i] >= 0 && row[i] < c->n;
        if (rows_out) rows_out[i] = hit ? row[i] : -1;
        if (hit) {
            rows.push_back(row[i]);
            ends.push_back(new_end[i]);
        }
    }
    if (rows.empty()) return PIE_OK;
    return set_end_apply(c, rows.data(), ends.data(), rows.size(), false);
}

// ---- a whole turn in one launch (pie_token_turn, pie_shard_token_turn; include/pie_scan.h, k_token_turn in pie_token.h)

// What every form refuses beyond its state checks, with nothing staged or changed.  k > 0.
static int token_turn_args(pie_ctx* c, const pie_turn_op* ops, size_t k, const char* what)
{
    if (!ops) return fail(c, PIE_E_INVAL, "%s: ops is NULL", what);
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%s: %zu ops in one turn", what, k);
    const size_t bad = turn_first_bad(ops, k);
    if (bad < k) return fail(c, PIE_E_INVAL, "%s: op %zu has kind %d, reserved %d", what, bad, (int)ops[bad].kind, (int)ops[bad].reserved);
    return PIE_OK;
}

// A turn's inputs into the pinned block h as `o` lays them out: [ops | next | cuser | cdisc].  The plan (pie_turn_plan.h) goes
// straight in: next[] where the device reads it, the head flags (built where the `live` results will land) into the reserved word
// of the staged ops.  That word carries the head flag in bit 0 and above it the ordinal of a CREATE (its row is rows + ordinal),
// whose user and discipline go to the compact arrays; without a create it is the head flag alone, and user / disc are not read.
static int turn_stage_fill(pie_ctx* c, char* h, const TokStage& o, const pie_turn_op* ops, size_t k, const int32_t* user, const int32_t* disc,
                           const char* what)
{
    memcpy(h, ops, k * sizeof(pie_turn_op));
    pie_turn_op* staged = stage_at<pie_turn_op>(h, 0);
    uint8_t* head = stage_at<uint8_t>(h, o.res.live);
    if (!turn_plan(ops, k, stage_at<int32_t>(h, o.next), head, c->tokx.turn_slots)) return fail(c, PIE_E_NOMEM, "%s: no memory for %zu ops", what, k);
    int32_t* cuser = stage_at<int32_t>(h, o.cuser);
    int32_t* cdisc = stage_at<int32_t>(h, o.cdisc);
    uint32_t j = 0;
    for (size_t i = 0; i < k; ++i) {
        uint32_t word = head[i];
        if (ops[i].kind == PIE_TURN_CREATE) {
            word |= j << 1;
            cuser[j] = user[i];
            cdisc[j] = disc[i];
            ++j;
        }
        staged[i].reserved = (int32_t)word;
    }
    return PIE_OK;
}

// What a create-free turn queues on the context's stream: ONE upload of the block's inputs, ONE k_token_turn with a thread per op.
// `status` are the words the kernel reports into: the context's, or the ones inside the slot's block.  `ord` is the ordered run
// the kernel keeps in step: ord_mirror_of(c) for the synchronous turn, none for a turn begun beside scans and batches (which is
// refused on a table that has a run: the host would learn of a stale run only at a wait).
static int token_turn_launch(pie_ctx* c, const char* h, char* d, const TokStage& o, size_t k, bool global, unsigned int* status, OrdMirror ord)
{
    pie_ctx::TokenIndex& t = c->tokx;
    hot_reserve(c, (long long)k); // the bound counts every op: never less than the rows that can move to the delta
    PIE_HIP(c, hipMemcpyAsync(d, h, o.up, hipMemcpyHostToDevice, c->stream));
    ShardMaps maps{};
    if (global) maps = ShardMaps{(const int*)c->d_shard_rows, c->shard_rows_n, (const int*)c->d_shard_users, c->shard_users_n};
    hipLaunchKernelGGL(global ? k_token_turn<true> : k_token_turn<false>, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, c->stream,
                       stage_at<const TurnOp>(d, 0), stage_at<const int>(d, o.next), (long long)k, (const int*)t.slot_row, t.log2_slots,
                       (const TokKey*)t.tok, token_bound(c), c->d_end, (const long long*)c->d_start, (const int*)c->d_user, maps, c->d_key,
                       c->key_base, c->key_shift, c->d_fkey, c->fkey_base, c->fkey_shift, ord, hot_mirror_of(c), stage_at<int>(d, o.res.row),
                       stage_at<unsigned char>(d, o.res.live), stage_at<int>(d, o.res.user), stage_at<long long>(d, o.res.start),
                       stage_at<long long>(d, o.res.end), status);
    PIE_HIP(c, hipGetLastError());
    c->key_dirty = true;
    return PIE_OK;
}

// What the shard form of a turn that logs in knows beside the turn itself (pie_shard_session_turn): how many of the creates the
// shard keeps and how many of the call's new users it owns.
struct ShardTurn {
    size_t n_kept, n_new;
    int32_t n_users_global;
};

// ... and a turn that logs in (the room is behind the caller): ONE upload of [ops | next | cuser | cdisc], ONE k_session_turn.
// sh (a sharded context): the block also carries [crow | new users]; the new users go behind the device user map in stream order,
// before the kernel, as append_launch puts them there; the run goes only when the shard keeps a create.
// n_kept creates become the context's rows [c->n, c->n + n_kept); users_after is its own (local) user count after the turn.
// The ordered run: dropped before the kernel could mirror into it, or — pie_set_turn_ordered, under append_in_place's
// condition — kept: the kernel mirrors the stores to the rows from before the turn, and behind it the created rows are gathered
// from the TABLE (k_ord_stage_rows: a later op of the turn may have re-ended one) and inserted as an append's rows are.
// tokx.turn_ord_k tells the wait phase (turn_ord_tail) that it owes the run's bookkeeping.
static int session_turn_launch(pie_ctx* c, const TokStage& o, size_t k, size_t n_kept, int users_after, const ShardTurn* sh = nullptr)
{
    pie_ctx::TokenIndex& t = c->tokx;
    hot_reserve(c, (long long)k);           // every delta record of the turn is owed to an op of its own: a touch, a delete or a create
    const long long old_n = c->n;
    const bool ord_kept = c->turn_ordered && n_kept > 0 && c->ord.valid && c->ord.rows == old_n && n_kept <= (size_t)kOrdAppendMax &&
                          users_after <= c->ord.users && c->key_ok;
    if (n_kept && !ord_kept) ord_invalidate(c); // the run does not take the new rows: it goes before the kernel could mirror into it
    t.turn_ord_k = 0;
    char* d = t.d_stage;
    PIE_HIP(c, hipMemcpyAsync(d, t.h_stage, o.up, hipMemcpyHostToDevice, c->stream));
    if (sh && sh->n_new)
        PIE_HIP(c, hipMemcpyAsync(c->d_shard_users + c->shard_users_n, d + o.newu, sh->n_new * 4, hipMemcpyDeviceToDevice, c->stream));
    const bool keys = c->key_ok; // a table too large to carry the derived columns runs without them
    const dim3 grid((unsigned)((k + 255) / 256));
    if (sh) {
        const ShardMaps maps{(const int*)c->d_shard_rows, c->shard_rows_n, (const int*)c->d_shard_users, c->shard_users_n + (int)sh->n_new};
        hipLaunchKernelGGL(k_session_turn<true>, grid, dim3(256), 0, c->stream, stage_at<const TurnOp>(d, 0), stage_at<const int>(d, o.next),
                           (long long)k, stage_at<const int>(d, o.cuser), stage_at<const int>(d, o.cdisc), stage_at<const int>(d, o.crow),
                           c->shard_rows_global, t.slot_row, t.log2_slots, t.tok, token_bound(c), c->d_start, c->d_end, c->d_user, c->d_disc,
                           maps, c->d_shard_rows, keys ? c->d_key : nullptr, c->key_base, c->key_shift, keys ? c->d_fkey : nullptr,
                           c->fkey_base, c->fkey_shift, keys ? c->d_pay : nullptr, ord_mirror_of(c), hot_mirror_of(c),
                           stage_at<int>(d, o.res.row), stage_at<unsigned char>(d, o.res.live), stage_at<int>(d, o.res.user),
                           stage_at<long long>(d, o.res.start), stage_at<long long>(d, o.res.end), t.status);
    } else
        hipLaunchKernelGGL(k_session_turn<false>, grid, dim3(256), 0, c->stream, stage_at<const TurnOp>(d, 0), stage_at<const int>(d, o.next),
                           (long long)k, stage_at<const int>(d, o.cuser), stage_at<const int>(d, o.cdisc), (const int*)nullptr, c->n,
                           t.slot_row, t.log2_slots, t.tok, t.covered, c->d_start, c->d_end, c->d_user, c->d_disc, ShardMaps{}, (int*)nullptr,
                           keys ? c->d_key : nullptr, c->key_base, c->key_shift, keys ? c->d_fkey : nullptr, c->fkey_base, c->fkey_shift,
                           keys ? c->d_pay : nullptr, ord_mirror_of(c), hot_mirror_of(c), stage_at<int>(d, o.res.row),
                           stage_at<unsigned char>(d, o.res.live), stage_at<int>(d, o.res.user), stage_at<long long>(d, o.res.start),
                           stage_at<long long>(d, o.res.end), t.status);
    PIE_HIP(c, hipGetLastError());
    if (ord_kept) {
        OrderedRun& r = c->ord;
        t.turn_ord_k = n_kept; // from here on the run holds, or may hold, rows of the turn: the wait phase settles it
        t.turn_ord_row0 = old_n;
        t.turn_ord_users = users_after;
        hipLaunchKernelGGL(k_ord_stage_rows, dim3((unsigned)((n_kept + 255) / 256)), dim3(256), 0, c->stream, (const long long*)c->d_start,
                           (const long long*)c->d_end, (const int*)c->d_user, (const int*)c->d_disc, old_n, (int)n_kept,
                           reinterpret_cast<long long*>(r.tstage), reinterpret_cast<long long*>(r.tstage + n_kept * 8),
                           reinterpret_cast<int*>(r.tstage + n_kept * 16), reinterpret_cast<int*>(r.tstage + n_kept * 20));
        launch_ord_append(c, c->stream, r.tstage, n_kept, old_n, users_after, 1); // pend[] is all zero between appends
        PIE_HIP(c, hipGetLastError());
    }
    return PIE_OK;
}

// The queue phase (the checks are behind the caller, k > 0): the plan on the host, ONE upload, ONE kernel, ONE download of the
// results and the status words, and an event behind them.  Nothing is waited for.  n_create > 0: the turn logs in
// (pie_session_turn), user / disc name who, and users_after is the context's own (local) user count after the turn.
static int token_turn_queue(pie_ctx* c, const pie_turn_op* ops, size_t k, bool global, const char* what, const int32_t* user = nullptr,
                            const int32_t* disc = nullptr, size_t n_create = 0, const ShardTurn* sh = nullptr, int users_after = 0)
{
    pie_ctx::TokenIndex& t = c->tokx;
    PIE_HIP(c, hipSetDevice(c->device));
    const TokStage o = turn_stage_of(k, n_create, sh != nullptr, sh ? sh->n_new : 0);
    int rc = token_stage_room(c, o.bytes);
    if (rc) return rc;
    if (!t.turn_done) PIE_HIP(c, hipEventCreateWithFlags(&t.turn_done, hipEventDisableTiming));
    if ((rc = turn_stage_fill(c, t.h_stage, o, ops, k, user, disc, what)) != PIE_OK) return rc;
    if (sh) { // the shard's own part of the plan: the LOCAL row of every create it keeps, the users it gains
        int32_t* crow = stage_at<int32_t>(t.h_stage, o.crow);
        int32_t* per_op = stage_at<int32_t>(t.h_stage, o.res.row); // scratch: the results have not landed there yet
        shard_session_turn_rows(ops, k, user, c->shard_rows_global, c->n, c->shard_rank, c->shard_world, nullptr, per_op, nullptr);
        size_t j = 0;
        for (size_t i = 0; i < k; ++i)
            if (ops[i].kind == PIE_TURN_CREATE) crow[j++] = per_op[i];
        shard_new_users(c->shard_users_global, sh->n_users_global, c->shard_rank, c->shard_world, stage_at<int32_t>(t.h_stage, o.newu));
    }
    t.turn_ord_k = 0;
    rc = n_create ? session_turn_launch(c, o, k, sh ? sh->n_kept : n_create, users_after, sh)
                  : token_turn_launch(c, t.h_stage, t.d_stage, o, k, global, t.status, ord_mirror_of(c));
    if (rc == PIE_OK) rc = token_stage_download(c, o);
    if (rc == PIE_OK && hipEventRecord(t.turn_done, c->stream) != hipSuccess) rc = fail(c, PIE_E_HIP, "%s: hipEventRecord failed", what);
    if (rc && t.turn_ord_k) { // nobody will wait for the insert: the run may hold some of the turn's rows and not others
        t.turn_ord_k = 0;
        ord_invalidate(c);
    }
    return rc;
}

// Behind the wait of a turn whose created rows went into the ordered run (session_turn_launch): what append_waited_tail does with
// the run's two mapped words.  [0]: a row far out of time order, or a row the run does not hold that an op of the turn brought
// back to life — the run goes either way; [1] alone: a full segment — re-spread, then pass 2 from the run's own staging block.
// c->n already counts the turn's rows.  failed: the status words reported a slip, so a planned row may not have been written.
static int turn_ord_tail(pie_ctx* c, bool failed)
{
    pie_ctx::TokenIndex& t = c->tokx;
    const size_t kept = t.turn_ord_k;
    t.turn_ord_k = 0;
    int rc = PIE_OK;
    volatile unsigned int* st = c->ord.h_stale;
    // plain ord_invalidate, not append_waited_tail's out_of_order form: here word 0 also counts revived rows, which say nothing
    // about how the table is fed, so a run that dies this way raises `need` step by step instead of straight to 4 096
    if (failed || st[0] != 0) ord_invalidate(c);
    else if (st[1] != 0 && (rc = ord_respread(c, c->ord.tstage, kept, t.turn_ord_row0, t.turn_ord_users)) != PIE_OK) ord_invalidate(c);
    c->ord.h_stale[0] = c->ord.h_stale[1] = 0;
    if (c->ord.valid) {
        c->ord.rows = c->n;
        c->ord.held += (long long)kept;
    }
    return rc;
}

// The wait phase: the one wait of a turn, on its own event and bounded (pie_wait.h); then what set_end_apply does behind its
// wait (a row the ordered run does not hold came back to life: the run goes), the status words, and the results.
static int token_turn_wait(pie_ctx* c, size_t k, const char* what, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out,
                           int64_t* end_out, size_t n_create = 0, bool shard = false, size_t n_new = 0)
{
    pie_ctx::TokenIndex& t = c->tokx;
    PIE_HIP(c, hipSetDevice(c->device));
    const WaitResult w = event_wait(c, t.turn_done);
    if (w.end != WaitEnd::Ready && t.turn_ord_k) { // the insert's outcome will never be read: the run may miss rows of the turn
        t.turn_ord_k = 0;
        ord_invalidate(c);
    }
    if (w.end == WaitEnd::Failed) return fail(c, PIE_E_HIP, "%s: the turn failed: %s", what, hipGetErrorString((hipError_t)w.err));
    if (w.end != WaitEnd::Ready) return fail(c, PIE_E_HIP, "%s: not finished within %.0f ms (PIE_WAIT_DEADLINE_MS): kernel hung?", what, w.waited_ms);
    const TokStage o = turn_stage_of(k, n_create, shard, n_new);
    int rc = token_status_check(c, stage_at<const unsigned int>(t.h_stage, o.status), what);
    int rc_ord = PIE_OK;
    if (t.turn_ord_k) rc_ord = turn_ord_tail(c, rc != PIE_OK);
    else if (c->ord.h_stale && *(volatile unsigned int*)c->ord.h_stale) {
        *c->ord.h_stale = 0;
        ord_invalidate(c);
    }
    if (rc) return rc;
    token_results_out(t.h_stage, o.res, k, row_out, live_out, user_out, start_out, end_out);
    return rc_ord;
}

int pie_token_turn_plan(const pie_turn_op* ops, size_t k, int32_t* next_out, uint8_t* head_out)
{
    if (k >= ((size_t)1 << 31) || (k && (!ops || !next_out || !head_out))) return PIE_E_INVAL;
    std::vector<int32_t> slots;
    return turn_plan(ops, k, next_out, head_out, slots) ? PIE_OK : PIE_E_NOMEM;
}

int pie_token_turn(pie_ctx* c, const pie_turn_op* ops, size_t k, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out,
                   int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_turn", true);
    if (rc || k == 0) return rc;
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "%s: a token turn is begun and not finished (pie_token_turn_finish)", "pie_token_turn");
    if ((rc = token_turn_args(c, ops, k, "pie_token_turn")) != PIE_OK) return rc;
    if ((rc = token_turn_queue(c, ops, k, false, "pie_token_turn")) != PIE_OK) return rc;
    return token_turn_wait(c, k, "pie_token_turn", row_out, live_out, user_out, start_out, end_out);
}

// ---- a turn that logs in (pie_session_turn; include/pie_scan.h, k_session_turn in pie_token.h)

int pie_session_turn_plan(const pie_turn_op* ops, size_t k, int64_t row0, int32_t* next_out, uint8_t* head_out, int32_t* new_row_out,
                          size_t* n_create_out)
{
    if (k >= ((size_t)1 << 31) || row0 < 0 || (k && (!ops || !next_out || !head_out || !new_row_out))) return PIE_E_INVAL;
    if (session_turn_first_bad(ops, k) < k) return PIE_E_INVAL;
    if (row0 + (int64_t)session_turn_creates(ops, k) >= ((int64_t)1 << 31) - 1) return PIE_E_INVAL;
    std::vector<int32_t> slots;
    if (!turn_plan(ops, k, next_out, head_out, slots)) return PIE_E_NOMEM;
    const size_t n_create = session_turn_rows(ops, k, row0, new_row_out);
    if (n_create_out) *n_create_out = n_create;
    return PIE_OK;
}

int pie_session_turn(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user, const int32_t* disc, int32_t n_users, int32_t* row_out,
                     uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    const char* const what = "pie_session_turn";
    int rc = token_ready(c, what, true);
    if (rc) return rc;
    if (c->shard_on || c->tokx.sharded) return fail(c, PIE_E_STATE, "%s: a sharded context", what);
    if (turns_begun(c)) return fail(c, PIE_E_STATE, "%s: a token turn is begun and not finished (pie_token_turn_finish)", what);
    if (n_users < c->n_users) return fail(c, PIE_E_INVAL, "%s: n_users may only grow (%d < %d)", what, n_users, c->n_users);
    if (k > 0 && !ops) return fail(c, PIE_E_INVAL, "%s: ops is NULL", what);
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%s: %zu ops in one turn", what, k);
    const size_t bad = session_turn_first_bad(ops, k);
    if (bad < k) return fail(c, PIE_E_INVAL, "%s: op %zu has kind %d, reserved %d", what, bad, (int)ops[bad].kind, (int)ops[bad].reserved);
    const size_t n_create = session_turn_creates(ops, k);
    if (n_create == 0) { // pie_token_turn, behind the growth of the user count as an append of no rows does it
        if (n_users > c->n_users && (rc = pie_append_rows(c, nullptr, nullptr, nullptr, nullptr, 0, n_users)) != PIE_OK) return rc;
        if (k == 0) return PIE_OK;
        if ((rc = token_turn_queue(c, ops, k, false, what)) != PIE_OK) return rc;
        return token_turn_wait(c, k, what, row_out, live_out, user_out, start_out, end_out);
    }
    pie_ctx::TokenIndex& t = c->tokx;
    const long long old_n = c->n, creates = (long long)n_create;
    if (!user || !disc) return fail(c, PIE_E_INVAL, "%s: a create without %s", what, user ? "disc" : "user");
    for (size_t i = 0; i < k; ++i)
        if (ops[i].kind == PIE_TURN_CREATE && (unsigned)user[i] >= (unsigned)n_users)
            return fail(c, PIE_E_INVAL, "%s: op %zu carries user %d outside [0, %d)", what, i, user[i], n_users);
    if (t.covered < old_n) return fail(c, PIE_E_STATE, "%s: the token column covers %lld of %lld rows (pie_token_append the rest first)", what, t.covered, old_n);
    if (old_n + creates >= (1LL << 31) - 1) return fail(c, PIE_E_INVAL, "%s: row count outside [0, 2^31 - 1)", what);
    PIE_HIP(c, hipSetDevice(c->device));
    // Room, by the routines pie_append_rows and pie_token_append make it with; the table's size does not move here.
    if (old_n + creates > c->cap_rows || n_users > c->cap_users || !c->key_ok) {
        rc = append_rollback(c, old_n, ensure_capacity(c, old_n + creates, n_users, old_n > 0 ? old_n : 1));
        if (rc == PIE_OK) rc = build_keys(c, old_n); // every row: the columns moved, or were not keyed
        if (rc) return rc;
    }
    if ((rc = token_make_room(c, old_n + creates, what)) != PIE_OK) return rc;
    if ((rc = token_turn_queue(c, ops, k, false, what, user, disc, n_create, nullptr, n_users)) != PIE_OK) return rc;
    // the host's picture moves as an append moves it; the rows are in the stream behind everything queued so far
    c->n = old_n + creates;
    t.covered = c->n;
    rc = append_finish(c, n_users);
    const int rc_wait = token_turn_wait(c, k, what, row_out, live_out, user_out, start_out, end_out, n_create);
    return rc_wait ? rc_wait : rc;
}

// pie_token_layout and pie_shard_token_layout behind their checks; the covered rows are LOCAL ones (covered_l on a sharded column)
static int token_layout_read(pie_ctx* c, const char* what, size_t* covered_global_out, size_t* covered_out, size_t* slots_out,
                             int32_t* slot_row_out, size_t cap, uint64_t* tok_out)
{
    pie_ctx::TokenIndex& t = c->tokx;
    const size_t slots = (size_t)1 << t.log2_slots;
    if (slots_out) *slots_out = slots;
    if (covered_global_out) *covered_global_out = (size_t)t.covered_g;
    if (slot_row_out && cap < slots) return fail(c, PIE_E_CAPACITY, "%s: %zu slots, room for %zu", what, slots, cap);
    PIE_HIP(c, hipSetDevice(c->device));
    long long covered = t.covered;
    if (t.sharded) {
        int rc = shard_token_covered(c, &covered);
        if (rc) return rc;
    }
    if (covered_out) *covered_out = (size_t)covered;
    if (slot_row_out) PIE_HIP(c, hipMemcpyAsync(slot_row_out, t.slot_row, slots * 4, hipMemcpyDeviceToHost, c->stream));
    if (tok_out && covered) PIE_HIP(c, hipMemcpyAsync(tok_out, t.tok, (size_t)covered * sizeof(TokKey), hipMemcpyDeviceToHost, c->stream));
    return token_status_wait(c, what);
}

int pie_token_layout(pie_ctx* c, size_t* covered_out, size_t* slots_out, int32_t* slot_row_out, size_t cap, uint64_t* tok_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_ready(c, "pie_token_layout", true);
    if (rc) return rc;
    return token_layout_read(c, "pie_token_layout", nullptr, covered_out, slots_out, slot_row_out, cap, tok_out);
}

// pie_compact_rows dropped rows and the table stands in its new numbering (the maps of the compaction are resident): the keys of
// the kept covered rows move to their new rows — row order was kept, so they are a prefix again — and the index is rebuilt.
// Out of memory here drops the token column; the compaction stands either way.
static int token_after_compact(pie_ctx* c, long long n_old)
{
    pie_ctx::TokenIndex& t = c->tokx;
    t.hold = false;
    if (!t.tok) return PIE_OK;
    hipStream_t s = c->stream;
    const long long kept = c->cmp_n_kept;
    // a sharded column: the new row map holds the original global ids of the kept rows, so the kept covered rows are its entries
    // below covered_g — a prefix again; their old rows lay inside the old column
    const long long covered_old = t.sharded ? (n_old < t.cap ? n_old : t.cap) : t.covered;
    long long covered = t.covered >= n_old ? kept : 0;
    if (t.sharded) {
        int rc = shard_token_covered(c, &covered);
        if (rc == PIE_OK && covered > kept) rc = fail(c, PIE_E_HIP, "pie_compact_rows: token column: %lld covered rows of %lld kept", covered, kept);
        if (rc) {
            token_drop(c);
            return rc;
        }
    } else if (t.covered < n_old && t.covered > 0 && kept > 0) { // the entries of old_of_new below the old `covered`
        hipLaunchKernelGGL(k_compact_lower_bound, dim3(1), dim3(1), 0, s, (const int*)c->d_cmp_old_of_new, kept, t.covered, c->d_range);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&covered, c->d_range, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess || covered < 0 || covered > kept) {
            token_drop(c);
            return fail(c, PIE_E_HIP, "pie_compact_rows: token column: %s", hipGetErrorString(e));
        }
    }
    const unsigned log2_slots = token_log2(pie_token_slots_for((size_t)(t.sharded ? kept : covered))); // a shard sizes by its rows
    const long long cap = c->cap_rows > t.cap ? c->cap_rows : t.cap;
    TokKey* nt = nullptr;
    int* ns = nullptr;
    if (hipMalloc(&nt, (size_t)cap * sizeof(TokKey)) != hipSuccess || (log2_slots != t.log2_slots && hipMalloc(&ns, (size_t)4 << log2_slots) != hipSuccess)) {
        (void)hipGetLastError();
        dfree(nt);
        token_drop(c);
        return PIE_OK;
    }
    if (covered > 0) {
        hipLaunchKernelGGL(k_token_gather, dim3(capped_grid(c, (size_t)covered)), dim3(256), 0, s, (const TokKey*)t.tok,
                           (const int*)c->d_cmp_old_of_new, covered, covered_old, nt);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            dfree(nt);
            dfree(ns);
            token_drop(c);
            return fail(c, PIE_E_HIP, "pie_compact_rows: token column: %s", hipGetErrorString(e));
        }
    }
    dfree(t.tok);
    t.tok = nt;
    t.cap = cap;
    t.covered = t.sharded ? 0 : covered;
    if (ns) {
        dfree(t.slot_row);
        t.slot_row = ns;
        t.log2_slots = log2_slots;
    }
    int rc = token_rebuild(c, covered);
    if (rc) return rc;
    return token_status_wait(c, "pie_compact_rows");
}

// ---- the token column of a SHARDED context, by GLOBAL row (include/pie_scan.h, pie_shard_token_*).  Every shard is given the
// same call and keeps what is its own; nothing is exchanged.  The host knows covered_g, the shard's row count and the slot
// count; which local rows are covered only the device's row map knows.

// idle = false: the call runs beside scans, batches and begun turns, and asks for the sharded table alone
static int shard_token_ready(pie_ctx* c, const char* what, bool need_column, bool idle = true)
{
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "%s: no table loaded", what);
    int rc = idle ? shard_ready(c, what) : shard_table_ready(c, what);
    if (rc) return rc;
    if (need_column && !(c->tokx.tok && c->tokx.sharded))
        return fail(c, PIE_E_STATE, "%s: the table has no token column (pie_shard_token_set gives it one)", what);
    return PIE_OK;
}

} // extern "C"

// What pie_shard_token_set / pie_shard_token_append would refuse, checked with nothing staged or changed (the communicator asks
// every local shard first), and the two phases of a sharded lookup, which the communicator queues on every shard before it waits
// for any.
namespace pie_internal {
int shard_token_check(pie_ctx* c, const uint64_t* tok, size_t k, bool set)
{
    if (!c) return PIE_E_INVAL;
    const char* what = set ? "pie_shard_token_set" : "pie_shard_token_append";
    int rc = shard_token_ready(c, what, !set);
    if (rc) return rc;
    if (k > 0 && !tok) return fail(c, PIE_E_INVAL, "tok is NULL");
    const long long from = set ? 0 : c->tokx.covered_g;
    if (k > (size_t)(c->shard_rows_global - from))
        return fail(c, PIE_E_INVAL, "%s: %zu keys behind %lld covered rows of a table of %lld", what, k, from, c->shard_rows_global);
    return PIE_OK;
}

int shard_token_lookup_queue(pie_ctx* c, const uint64_t* tok, size_t k, int64_t now)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_token_ready(c, "pie_shard_token_lookup", true);
    if (rc || k == 0) return rc;
    if (!tok) return fail(c, PIE_E_INVAL, "tok is NULL");
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%zu keys in one lookup", k);
    return token_lookup_queue(c, tok, k, (long long)now, true, true, true);
}

// after shard_token_lookup_queue of the same k returned PIE_OK: waits, then copies what is asked for (any pointer may be NULL)
int shard_token_lookup_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                            int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    if (k == 0) return PIE_OK;
    int rc = token_lookup_wait(c, k, true, "pie_shard_token_lookup");
    if (rc) return rc;
    const TokStage o = lookup_stage_of(k, true);
    TokResults global = o.res; // this form alone has two rows to give: the caller gets the GLOBAL one
    global.row = o.grow;
    token_results_out(c->tokx.h_stage, global, k, row_global_out, live_out, user_global_out, start_out, end_out);
    return PIE_OK;
}

// The phases of pie_shard_token_turn, which the communicator runs shard by shard: every check with nothing staged or changed
// (k = 0 passes the state checks alone), the queue phase, the wait phase.
int shard_token_turn_check(pie_ctx* c, const pie_turn_op* ops, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_token_ready(c, "pie_shard_token_turn", true);
    if (rc || k == 0) return rc;
    return token_turn_args(c, ops, k, "pie_shard_token_turn");
}

int shard_token_turn_queue(pie_ctx* c, const pie_turn_op* ops, size_t k)
{
    return k == 0 ? PIE_OK : token_turn_queue(c, ops, k, true, "pie_shard_token_turn");
}

int shard_token_turn_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                          int64_t* end_out)
{
    return k == 0 ? PIE_OK : token_turn_wait(c, k, "pie_shard_token_turn", row_global_out, live_out, user_global_out, start_out, end_out);
}
} // namespace pie_internal

extern "C" {

int pie_shard_token_turn(pie_ctx* c, const pie_turn_op* ops, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out,
                         int64_t* start_out, int64_t* end_out)
{
    int rc = pie_internal::shard_token_turn_check(c, ops, k);
    if (rc || k == 0) return rc;
    if ((rc = pie_internal::shard_token_turn_queue(c, ops, k)) != PIE_OK) return rc;
    return pie_internal::shard_token_turn_wait(c, k, row_global_out, live_out, user_global_out, start_out, end_out);
}

// Room for a sharded column on a shard of `rows` local rows (pie_shard_token_append: the rows it holds; pie_shard_session_turn:
// with the creates it keeps): a column as long as the table's capacity (the table grew) and slots that stay at most half full —
// the shard's row count passed half of them: the index is rebuilt from the covered rows into pie_token_slots_for(rows).  Both
// free what a lookup begun earlier reads: those land first.  May wait.
static int shard_token_make_room(pie_ctx* c, long long rows, const char* what)
{
    pie_ctx::TokenIndex& t = c->tokx;
    hipStream_t s = c->stream;
    const bool longer = c->cap_rows > t.cap, grow = (unsigned long long)rows > ((1ull << t.log2_slots) >> 1);
    int rc = PIE_OK;
    if ((longer || grow) && (rc = token_lookups_land(c, what)) != PIE_OK) return rc;
    if (longer) {
        TokKey* nt = nullptr;
        PIE_HIP(c, hipMalloc(&nt, (size_t)c->cap_rows * sizeof(TokKey)));
        hipError_t e = t.cap ? hipMemcpyAsync(nt, t.tok, (size_t)t.cap * sizeof(TokKey), hipMemcpyDeviceToDevice, s) : hipSuccess;
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hipFree(nt);
            return fail(c, PIE_E_HIP, "%s: %s", what, hipGetErrorString(e));
        }
        dfree(t.tok);
        t.tok = nt;
        t.cap = c->cap_rows;
    }
    if (grow) {
        const unsigned log2_slots = token_log2(pie_token_slots_for((size_t)rows));
        long long covered_l = 0;
        rc = shard_token_covered(c, &covered_l); // waits: inserts queued earlier still write the table that goes
        if (rc) return rc;
        int* ns = nullptr;
        PIE_HIP(c, hipMalloc(&ns, (size_t)4 << log2_slots));
        dfree(t.slot_row);
        t.slot_row = ns;
        t.log2_slots = log2_slots;
        rc = token_rebuild(c, covered_l);
        if (rc) return rc;
    }
    return PIE_OK;
}

// One chunk (k <= 2^20 keys, checked by the caller) for the global rows [covered_g, covered_g + k): everything that can fail and
// everything that waits comes first — the staging area, a longer column (the table grew), a larger table of slots (the shard's
// row count passed half of them: the index is rebuilt from the covered rows) — then one upload and one launch, queued.
static int shard_token_chunk(pie_ctx* c, const uint64_t* tok, size_t k)
{
    pie_ctx::TokenIndex& t = c->tokx;
    hipStream_t s = c->stream;
    if (c->n == 0) { // nothing of any chunk can be this shard's
        t.covered_g += (long long)k;
        return PIE_OK;
    }
    Staged st{};
    int rc = stage_mutation(c, k * sizeof(TokKey), true, &st);
    if (rc) return rc;
    if ((rc = shard_token_make_room(c, c->n, "pie_shard_token_append")) != PIE_OK) return rc;
    memcpy(st.h, tok, k * sizeof(TokKey));
    PIE_HIP(c, hipMemcpyAsync(st.d, st.h, k * sizeof(TokKey), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_shard_token_place, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const TokKey*>(st.d), t.covered_g,
                       (long long)k, (const int*)c->d_shard_rows, c->shard_rows_n, t.tok, t.cap, t.slot_row, t.log2_slots, t.status);
    PIE_HIP(c, hipGetLastError());
    rc = stage_queued(c, st);
    if (rc) return rc;
    t.covered_g += (long long)k;
    return PIE_OK;
}

static int shard_token_chunks(pie_ctx* c, const uint64_t* tok, size_t k)
{
    const size_t most = (size_t)1 << 20;
    for (size_t done = 0; done < k;) {
        const size_t kk = k - done < most ? k - done : most;
        int rc = shard_token_chunk(c, tok + 2 * done, kk);
        if (rc) return rc;
        done += kk;
    }
    return PIE_OK;
}

int pie_shard_token_set(pie_ctx* c, const uint64_t* tok, size_t n)
{
    if (!c) return PIE_E_INVAL;
    int rc = pie_internal::shard_token_check(c, tok, n, true);
    if (rc) return rc;
    PIE_HIP(c, hipSetDevice(c->device));
    rc = token_status_alloc(c);
    if (rc) return rc;
    pie_ctx::TokenIndex& t = c->tokx;
    // the new column and table first: a failure leaves what was there.  Slots by the shard's row count, which the host knows.
    const unsigned log2_slots = token_log2(pie_token_slots_for((size_t)c->n));
    TokKey* nt = nullptr;
    int* ns = nullptr;
    if (hipMalloc(&nt, (size_t)c->cap_rows * sizeof(TokKey)) != hipSuccess || hipMalloc(&ns, (size_t)4 << log2_slots) != hipSuccess) {
        (void)hipGetLastError();
        dfree(nt);
        return fail(c, PIE_E_NOMEM, "pie_shard_token_set: no device memory for %lld keys and %llu slots", c->cap_rows, 1ull << log2_slots);
    }
    token_drop(c);
    t.tok = nt;
    t.cap = c->cap_rows;
    t.slot_row = ns;
    t.log2_slots = log2_slots;
    t.sharded = true;
    rc = token_rebuild(c, 0); // the empty column: every slot empty
    if (rc == PIE_OK) rc = shard_token_chunks(c, tok, n);
    if (rc) return rc;
    PIE_HIP(c, hipEventRecord(t.ev[1], c->stream)); // token_build_ms: the fill and every chunk
    return token_status_wait(c, "pie_shard_token_set");
}

int pie_shard_token_append(pie_ctx* c, const uint64_t* tok, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = pie_internal::shard_token_check(c, tok, k, false);
    if (rc || k == 0) return rc;
    PIE_HIP(c, hipSetDevice(c->device));
    return shard_token_chunks(c, tok, k);
}

int pie_shard_token_lookup(pie_ctx* c, const uint64_t* tok, size_t k, int64_t now, int32_t* row_global_out, uint8_t* live_out,
                           int32_t* user_global_out, int64_t* start_out, int64_t* end_out)
{
    int rc = pie_internal::shard_token_lookup_queue(c, tok, k, now);
    if (rc) return rc;
    return pie_internal::shard_token_lookup_wait(c, k, row_global_out, live_out, user_global_out, start_out, end_out);
}

// one lookup, then pie_set_end's own path on the LOCAL rows found live, as pie_token_set_end composes
int pie_shard_token_set_end(pie_ctx* c, const uint64_t* tok, const int64_t* new_end, size_t k, int64_t now, int32_t* rows_global_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_token_ready(c, "pie_shard_token_set_end", true);
    if (rc || k == 0) return rc;
    if (!tok || !new_end) return fail(c, PIE_E_INVAL, "NULL pointer");
    rc = pie_internal::shard_token_lookup_queue(c, tok, k, now);
    if (rc == PIE_OK) rc = token_lookup_wait(c, k, true, "pie_shard_token_set_end");
    if (rc) return rc;
    const TokStage o = lookup_stage_of(k, true);
    const int32_t* row = stage_at<const int32_t>(c->tokx.h_stage, o.res.row);
    const int32_t* grow = stage_at<const int32_t>(c->tokx.h_stage, o.grow);
    const uint8_t* live = stage_at<const uint8_t>(c->tokx.h_stage, o.res.live);
    std::vector<int32_t> rows;
    std::vector<int64_t> ends;
    try {
        rows.reserve(k);
        ends.reserve(k);
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "no memory for %zu touches", k);
    }
    for (size_t i = 0; i < k; ++i) {
        const bool hit = live[i] != 0 && row[i] >= 0 && row[i] < c->n;
        if (rows_global_out) rows_global_out[i] = hit ? grow[i] : -1;
        if (hit) {
            rows.push_back(row[i]);
            ends.push_back(new_end[i]);
        }
    }
    if (rows.empty()) return PIE_OK;
    return set_end_apply(c, rows.data(), ends.data(), rows.size(), false);
}

int pie_shard_token_layout(pie_ctx* c, size_t* covered_global_out, size_t* covered_local_out, size_t* slots_out, int32_t* slot_row_out,
                           size_t cap, uint64_t* tok_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = shard_token_ready(c, "pie_shard_token_layout", true);
    if (rc) return rc;
    return token_layout_read(c, "pie_shard_token_layout", covered_global_out, covered_local_out, slots_out, slot_row_out, cap, tok_out);
}

// ---- a turn that logs in on a sharded table (pie_shard_session_turn; include/pie_scan.h, k_session_turn<true> in pie_token.h).
// Every shard is given the same turn.  Which create is whose, the global and the local row of each and the users a shard gains
// are host arithmetic (pie_turn_plan.h); nothing is exchanged and nothing is counted on the device.

int pie_shard_session_turn_plan(const pie_turn_op* ops, size_t k, const int32_t* user_global, int64_t rows_global0, int64_t rows_local0,
                                int32_t rank, int32_t world, int32_t* next_out, uint8_t* head_out, int32_t* new_row_global_out,
                                int32_t* new_row_local_out, size_t* n_create_out, size_t* n_kept_out)
{
    if (k >= ((size_t)1 << 31) || rows_global0 < 0 || rows_local0 < 0 || rows_local0 > rows_global0 || world < 1 || rank < 0 || rank >= world)
        return PIE_E_INVAL;
    if (k && (!ops || !next_out || !head_out || !new_row_global_out || !new_row_local_out)) return PIE_E_INVAL;
    if (session_turn_first_bad(ops, k) < k) return PIE_E_INVAL;
    const size_t n_create = session_turn_creates(ops, k);
    if (n_create && !user_global) return PIE_E_INVAL;
    if (rows_global0 + (int64_t)n_create >= ((int64_t)1 << 31) - 1) return PIE_E_INVAL;
    std::vector<int32_t> slots;
    if (!turn_plan(ops, k, next_out, head_out, slots)) return PIE_E_NOMEM;
    size_t n_kept = 0;
    shard_session_turn_rows(ops, k, user_global, rows_global0, rows_local0, rank, world, new_row_global_out, new_row_local_out, &n_kept);
    if (n_create_out) *n_create_out = n_create;
    if (n_kept_out) *n_kept_out = n_kept;
    return PIE_OK;
}

} // extern "C"

// The phases of pie_shard_session_turn, which the communicator runs shard by shard: every check with nothing staged or changed;
// the room (the one phase that may wait or re-allocate); the queue phase; the wait phase.
namespace pie_internal {
int shard_session_turn_check(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, const int32_t* disc, int32_t n_users_global)
{
    if (!c) return PIE_E_INVAL;
    const char* const what = "pie_shard_session_turn";
    int rc = shard_token_ready(c, what, true);
    if (rc) return rc;
    if (n_users_global < c->shard_users_global)
        return fail(c, PIE_E_INVAL, "%s: n_users_global may only grow (%d < %d)", what, n_users_global, c->shard_users_global);
    if (k > 0 && !ops) return fail(c, PIE_E_INVAL, "%s: ops is NULL", what);
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%s: %zu ops in one turn", what, k);
    const size_t bad = session_turn_first_bad(ops, k);
    if (bad < k) return fail(c, PIE_E_INVAL, "%s: op %zu has kind %d, reserved %d", what, bad, (int)ops[bad].kind, (int)ops[bad].reserved);
    const size_t n_create = session_turn_creates(ops, k);
    if (n_create == 0) return PIE_OK;
    if (!user_global || !disc) return fail(c, PIE_E_INVAL, "%s: a create without %s", what, user_global ? "disc" : "user");
    for (size_t i = 0; i < k; ++i)
        if (ops[i].kind == PIE_TURN_CREATE && (uint32_t)user_global[i] >= (uint32_t)n_users_global)
            return fail(c, PIE_E_INVAL, "%s: op %zu carries user %d outside [0, %d)", what, i, user_global[i], n_users_global);
    if (c->tokx.covered_g < c->shard_rows_global)
        return fail(c, PIE_E_STATE, "%s: the token column covers %lld of %lld global rows (pie_shard_token_append the rest first)", what,
                    c->tokx.covered_g, c->shard_rows_global);
    if (c->shard_rows_global + (long long)n_create >= (1LL << 31) - 1) return fail(c, PIE_E_INVAL, "%s: global row count outside [0, 2^31 - 1)", what);
    return PIE_OK;
}

// what the turn means to this shard (behind shard_session_turn_check): the creates it keeps, the users it gains
static ShardTurn shard_turn_of(const pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, int32_t n_users_global)
{
    ShardTurn sh{};
    sh.n_kept = session_turn_creates(ops, k) ? shard_session_turn_kept(ops, k, user_global, c->shard_rank, c->shard_world) : 0;
    sh.n_new = shard_new_users(c->shard_users_global, n_users_global, c->shard_rank, c->shard_world);
    sh.n_users_global = n_users_global;
    return sh;
}

// the context's own (local) user count once the shard holds n_new more users; a shard with no user keeps n_users = 1
static int shard_local_users(const pie_ctx* c, size_t n_new)
{
    const long long users = (long long)c->shard_users_n + (long long)n_new;
    return users > 0 ? (int)users : 1;
}

// Room, by the routines pie_shard_append_rows and pie_shard_token_append make it with; neither the table's size nor the user
// count moves here: the communicator makes room on every shard before it changes any.  A turn without a create needs none
// ahead of time (its new users come in the queue phase, as pie_shard_append_rows(k = 0) brings them).
int shard_session_turn_room(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, int32_t n_users_global)
{
    const char* const what = "pie_shard_session_turn";
    const size_t n_create = session_turn_creates(ops, k);
    if (n_create == 0) return PIE_OK;
    PIE_HIP(c, hipSetDevice(c->device));
    const ShardTurn sh = shard_turn_of(c, ops, k, user_global, n_users_global);
    const long long old_n = c->n, rows = old_n + (long long)sh.n_kept;
    const int local_users = shard_local_users(c, sh.n_new);
    try {
        c->shard_users_h.reserve(c->shard_users_h.size() + sh.n_new); // the commit behind the launch cannot fail
    } catch (...) {
        return fail(c, PIE_E_NOMEM, "%s: no memory for the user map", what);
    }
    int rc = PIE_OK;
    if (rows > c->cap_rows || local_users > c->cap_users || !c->key_ok) {
        rc = append_rollback(c, old_n, ensure_capacity(c, rows, local_users, old_n > 0 ? old_n : 1));
        if (rc == PIE_OK) rc = build_keys(c, old_n); // every row: the columns moved, or were not keyed
        if (rc) return rc;
    }
    if ((rc = shard_maps_reserve(c, c->cap_rows, c->cap_users)) != PIE_OK) return rc;
    if ((rc = shard_token_make_room(c, rows, what)) != PIE_OK) return rc;
    return token_stage_room(c, turn_stage_of(k, n_create, true, sh.n_new).bytes);
}

// One upload, one kernel, one download, nothing waited for (an error means nothing was launched); then the host's picture moves as a sharded append and a token append
// move it: the maps, N_g and covered_g on every shard alike, the rows and the users this shard gained.
int shard_session_turn_queue(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, const int32_t* disc, int32_t n_users_global)
{
    const char* const what = "pie_shard_session_turn";
    pie_ctx::TokenIndex& t = c->tokx;
    const size_t n_create = session_turn_creates(ops, k);
    t.turn_creates = n_create;
    t.turn_new_users = 0;
    t.turn_late_rc = PIE_OK;
    if (n_create == 0) { // pie_shard_token_turn, behind the growth of the user count as an append of no rows does it
        if (n_users_global > c->shard_users_global) {
            const int rc = pie_shard_append_rows(c, nullptr, nullptr, nullptr, nullptr, 0, n_users_global, nullptr, nullptr);
            if (rc) return rc;
        }
        return k == 0 ? PIE_OK : token_turn_queue(c, ops, k, true, what);
    }
    const ShardTurn sh = shard_turn_of(c, ops, k, user_global, n_users_global);
    const TokStage o = turn_stage_of(k, n_create, true, sh.n_new);
    // token_turn_queue fails before its launch (the staging, the plan) or, behind it, where only the runtime itself can fail
    // (the download, the event): such a context has a device error pending and is not used further, as on the unsharded path.
    int rc = token_turn_queue(c, ops, k, true, what, user_global, disc, n_create, &sh, shard_local_users(c, sh.n_new));
    if (rc) return rc;
    t.turn_new_users = sh.n_new;
    const int32_t* newu = stage_at<const int32_t>(t.h_stage, o.newu);
    c->shard_users_h.insert(c->shard_users_h.end(), newu, newu + sh.n_new); // reserved by the room phase
    const long long old_n = c->n;
    c->shard_rows_n = old_n + (long long)sh.n_kept;
    c->shard_users_n += (int)sh.n_new;
    c->shard_rows_global += (long long)n_create;
    c->shard_users_global = n_users_global;
    t.covered_g += (long long)n_create;
    c->n = old_n + (long long)sh.n_kept;
    const int local_users = shard_local_users(c, 0);
    if (sh.n_kept) {
        t.turn_late_rc = append_finish(c, local_users);
        return PIE_OK;
    }
    c->key_dirty = true; // the touches and deletes of the turn, as token_turn_launch leaves it
    if (local_users > c->n_users) { // as pie_shard_append_rows leaves a context that gained users and no row
        if (c->ord.valid && local_users > c->ord.users) ord_invalidate(c);
        set_user_count(c, local_users);
        drop_results(c);
    }
    return PIE_OK;
}

int shard_session_turn_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                            int64_t* end_out)
{
    if (k == 0) return PIE_OK;
    const pie_ctx::TokenIndex& t = c->tokx;
    const int rc = token_turn_wait(c, k, "pie_shard_session_turn", row_global_out, live_out, user_global_out, start_out, end_out,
                                   t.turn_creates, t.turn_creates > 0, t.turn_new_users);
    return rc ? rc : t.turn_late_rc;
}
} // namespace pie_internal

extern "C" {

int pie_shard_session_turn(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, const int32_t* disc, int32_t n_users_global,
                           int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out, int64_t* end_out)
{
    int rc = pie_internal::shard_session_turn_check(c, ops, k, user_global, disc, n_users_global);
    if (rc) return rc;
    if ((rc = pie_internal::shard_session_turn_room(c, ops, k, user_global, n_users_global)) != PIE_OK) return rc;
    if ((rc = pie_internal::shard_session_turn_queue(c, ops, k, user_global, disc, n_users_global)) != PIE_OK) return rc;
    return pie_internal::shard_session_turn_wait(c, k, row_global_out, live_out, user_global_out, start_out, end_out);
}

// ---- lookups beside scans and batches (pie_token_lookup_begin / _finish, include/pie_scan.h).  A lookup only reads, and so do
// scans and batches; every mutator is refused while those are in flight.  So a lookup needs no empty pipeline, only a stream, a
// staging area and status words that are not the context's: tokx.lk.

// A slot's staging holds `bytes`.  This slot's staging alone grows (from 256 KiB, which hold 5 300 keys or 3 700 ops, by
// doubling); the lookups and turns in flight keep theirs, and the old blocks wait for the next call that has drained the context
// anyway (token_drop, pie_ctx_destroy).
static int slot_stage_room(pie_ctx* c, SidePass& side, pie_ctx::TokenIndex::FlightSlot& sl, size_t bytes, size_t k, const char* what,
                           const char* unit)
{
    if (bytes <= sl.bytes) return PIE_OK;
    size_t want = sl.bytes ? sl.bytes : (size_t)256 << 10;
    while (want < bytes) want *= 2;
    char *nh = nullptr, *nd = nullptr;
    PIE_HIP(c, hipHostMalloc(&nh, want, hipHostMallocDefault));
    if (hipMalloc(&nd, want) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipHostFree(nh);
        return fail(c, PIE_E_NOMEM, "%s: no device memory for the staging of %zu %s", what, k, unit);
    }
    if (!side_retire(side, sl.h, sl.d)) {
        (void)hipHostFree(nh);
        (void)hipFree(nd);
        return fail(c, PIE_E_NOMEM, "%s: out of host memory", what);
    }
    sl.h = nh;
    sl.d = nd;
    sl.bytes = want;
    return PIE_OK;
}

static int token_flight_ready(pie_ctx* c, const char* what, bool global)
{
    return global ? shard_token_ready(c, what, true, false) : token_ready(c, what, true, false);
}

static int token_flight_begin(pie_ctx* c, const uint64_t* tok, const int64_t* now, size_t k, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_flight_ready(c, what, global);
    if (rc) return rc;
    pie_ctx::TokenIndex& t = c->tokx;
    if (t.lk_n >= kTokLookups) return fail(c, PIE_E_STATE, "%s: %d lookups are begun and not finished", what, t.lk_n);
    if (k > 0 && (!tok || !now)) return fail(c, PIE_E_INVAL, "%s: NULL pointer", what);
    if (k >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%s: %zu keys in one lookup", what, k);
    PIE_HIP(c, hipSetDevice(c->device));
    if ((rc = side_open(c, t.side)) != PIE_OK) return rc;
    pie_ctx::TokenIndex::Lookup& l = t.lk[(t.lk_head + t.lk_n) % kTokLookups]; // free: lookups finish in the order they began
    const TokStage o = lookup_flight_stage_of(k);
    if ((rc = slot_stage_room(c, t.side, l, o.bytes, k, what, l.unit)) != PIE_OK) return rc;
    hipStream_t s = t.side.stream;
    if ((rc = side_enter(c, t.side, l.fence, hipEventDisableTiming)) != PIE_OK) return rc;
    if (k > 0) {
        memcpy(l.h, tok, k * sizeof(TokKey));
        memcpy(l.h + o.now, now, k * 8);
        memset(l.h + o.status, 0, kTokStatusBytes);
        PIE_HIP(c, hipMemcpyAsync(l.d, l.h, o.up, hipMemcpyHostToDevice, s));
        char* d = l.d;
        const dim3 grid((unsigned)((k + 255) / 256));
        if (global)
            hipLaunchKernelGGL(k_shard_token_lookup_now, grid, dim3(256), 0, s, stage_at<const TokKey>(d, 0), stage_at<const long long>(d, o.now),
                               (long long)k, (const int*)t.slot_row, t.log2_slots, (const TokKey*)t.tok, token_bound(c), (const long long*)c->d_end,
                               (const long long*)c->d_start, (const int*)c->d_user, (const int*)c->d_shard_rows, c->shard_rows_n,
                               (const int*)c->d_shard_users, c->shard_users_n, stage_at<int>(d, o.res.row), stage_at<unsigned char>(d, o.res.live),
                               stage_at<int>(d, o.res.user), stage_at<long long>(d, o.res.start), stage_at<long long>(d, o.res.end),
                               stage_at<unsigned int>(d, o.status));
        else
            hipLaunchKernelGGL(k_token_lookup_now, grid, dim3(256), 0, s, stage_at<const TokKey>(d, 0), stage_at<const long long>(d, o.now),
                               (long long)k, (const int*)t.slot_row, t.log2_slots, (const TokKey*)t.tok, token_bound(c), (const long long*)c->d_end,
                               (const long long*)c->d_start, (const int*)c->d_user, stage_at<int>(d, o.res.row),
                               stage_at<unsigned char>(d, o.res.live), stage_at<int>(d, o.res.user), stage_at<long long>(d, o.res.start),
                               stage_at<long long>(d, o.res.end), stage_at<unsigned int>(d, o.status));
        PIE_HIP(c, hipGetLastError());
        PIE_HIP(c, hipMemcpyAsync(l.h + o.status, d + o.status, o.bytes - o.status, hipMemcpyDeviceToHost, s));
    }
    PIE_HIP(c, side_leave(c, t.side, l.fence));
    l.k = k;
    l.landed = false;
    l.global = global;
    t.lk_n++;
    return PIE_OK;
}

static int token_flight_finish(pie_ctx* c, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out,
                               size_t cap, size_t* k_out, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    pie_ctx::TokenIndex& t = c->tokx;
    return flight_finish(c, t.lk, t.lk_head, t.lk_n, t.side.stale, lookup_flight_stage_of, row_out, live_out, user_out, start_out, end_out, cap,
                         k_out, global, what);
}

int pie_token_lookup_begin(pie_ctx* c, const uint64_t* tok, const int64_t* now, size_t k)
{
    return token_flight_begin(c, tok, now, k, false, "pie_token_lookup_begin");
}

int pie_token_lookup_finish(pie_ctx* c, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out, size_t cap,
                            size_t* k_out)
{
    return token_flight_finish(c, row_out, live_out, user_out, start_out, end_out, cap, k_out, false, "pie_token_lookup_finish");
}

int pie_token_lookup_room(pie_ctx* c) { return c ? kTokLookups - c->tokx.lk_n : 0; }

int pie_shard_token_lookup_begin(pie_ctx* c, const uint64_t* tok, const int64_t* now, size_t k)
{
    return token_flight_begin(c, tok, now, k, true, "pie_shard_token_lookup_begin");
}

int pie_shard_token_lookup_finish(pie_ctx* c, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                                  int64_t* end_out, size_t cap, size_t* k_out)
{
    return token_flight_finish(c, row_global_out, live_out, user_global_out, start_out, end_out, cap, k_out, true, "pie_shard_token_lookup_finish");
}

// ---- turns beside scans and batches (pie_token_turn_begin / _finish, include/pie_scan.h).  A turn MUTATES, and
// scans and batches read what it writes: `end`, both keys, the hot index.  Every single scan and every batch of lane 0 is queued
// on the context's stream, so stream order already puts the turn between them.  The other lanes are fenced by events: the
// context's stream waits for every lane that has a batch in flight (turn_fence_enter), the turn's kernel runs, an event is
// recorded behind it, and every lane's next begin waits for that event once (lane_after_mutation).  Nothing here waits on the host.

// What stands in front of the turn's kernel on the context's stream.  First every union tail that still waits for a launch: a
// tail rebuilds its batch's masks from the table, so it must run before `end` changes (what pie_scan_batch_flush does; a begin
// after it carries no tail).  Then the lanes above 0 that have a batch in flight: an event on each, and the context's stream
// waits for it.  A lane with nothing in flight has had its last summary read by the host: nothing of it reads the table any more.
// The side passes (lookups, the expired queue) fenced the context's stream behind themselves when they were begun (side_leave).
static int turn_fence_enter(pie_ctx* c)
{
    int rc = pie_scan_batch_flush(c);
    if (rc) return rc;
    for (int lane = 1; lane < kLaneMax; ++lane) {
        if (c->lane_flight[lane] == 0 || !c->lane_stream[lane]) continue;
        if (!c->lane_event[lane][1]) PIE_HIP(c, hipEventCreateWithFlags(&c->lane_event[lane][1], hipEventDisableTiming));
        PIE_HIP(c, hipEventRecord(c->lane_event[lane][1], c->lane_stream[lane]));
        PIE_HIP(c, hipStreamWaitEvent(c->stream, c->lane_event[lane][1], 0));
    }
    return PIE_OK;
}

// ... and behind it: the event the lanes' next launches wait for, under a new mutation epoch
static int turn_fence_leave(pie_ctx* c)
{
    PIE_HIP(c, hipEventRecord(c->mut_event, c->stream));
    c->mut_epoch++;
    return PIE_OK;
}

static int turn_flight_begin(pie_ctx* c, const pie_turn_op* ops, size_t k, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    int rc = token_flight_ready(c, what, global);
    if (rc) return rc;
    pie_ctx::TokenIndex& t = c->tokx;
    if (k > 0 && (rc = token_turn_args(c, ops, k, what)) != PIE_OK) return rc;
    // the host learns of a row the run does not hold coming back to life (the run's stale flag) only at a wait: a batch begun
    // between this begin and its finish could read a stale run
    if (c->ord.valid) return fail(c, PIE_E_STATE, "%s: the table has an ordered run (pie_token_turn keeps it in step; pie_set_ordered_run(0) drops it)", what);
    if (t.tn_n >= kTokTurns) return fail(c, PIE_E_STATE, "%s: %d turns are begun and not finished", what, t.tn_n);
    PIE_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    if (t.tn_stale) { // a finish gave up on its wait: that turn's download may still be on its way into a slot
        PIE_HIP(c, hipStreamSynchronize(s));
        t.tn_stale = false;
    }
    pie_ctx::TokenIndex::Turn& u = t.tn[(t.tn_head + t.tn_n) % kTokTurns]; // free: turns finish in the order they began
    const TokStage o = turn_flight_stage_of(k);
    if ((rc = slot_stage_room(c, t.side, u, o.bytes, k, what, u.unit)) != PIE_OK) return rc;
    if (!u.done) PIE_HIP(c, hipEventCreateWithFlags(&u.done, hipEventDisableTiming));
    if (!c->mut_event) PIE_HIP(c, hipEventCreateWithFlags(&c->mut_event, hipEventDisableTiming));
    if (k > 0) {
        if ((rc = turn_stage_fill(c, u.h, o, ops, k, nullptr, nullptr, what)) != PIE_OK) return rc;
        memset(u.h + o.status, 0, kTokStatusBytes);
        if ((rc = turn_fence_enter(c)) != PIE_OK) return rc;
        // Host-side state the synchronous turn moves too (token_turn_launch); both are flags, and what they set off waits for an
        // idle context: the hot index's delta bound (past it the index is given up: later batches read the key
        // column, which the kernel keeps in step) and key_dirty (the re-fit is gated on nothing in flight and runs on this stream).
        char* d = u.d;
        if ((rc = token_turn_launch(c, u.h, d, o, k, global, stage_at<unsigned int>(d, o.status), OrdMirror{})) != PIE_OK) return rc;
        if ((rc = turn_fence_leave(c)) != PIE_OK) return rc;
        PIE_HIP(c, hipMemcpyAsync(u.h + o.status, d + o.status, o.bytes - o.status, hipMemcpyDeviceToHost, s));
        PIE_HIP(c, hipEventRecord(u.done, s));
    }
    u.k = k;
    u.landed = k == 0;
    u.global = global;
    t.tn_n++;
    return PIE_OK;
}

static int turn_flight_finish(pie_ctx* c, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out,
                              size_t cap, size_t* k_out, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    pie_ctx::TokenIndex& t = c->tokx;
    return flight_finish(c, t.tn, t.tn_head, t.tn_n, t.tn_stale, turn_flight_stage_of, row_out, live_out, user_out, start_out, end_out, cap, k_out,
                         global, what);
}

int pie_token_turn_begin(pie_ctx* c, const pie_turn_op* ops, size_t k) { return turn_flight_begin(c, ops, k, false, "pie_token_turn_begin"); }

int pie_token_turn_finish(pie_ctx* c, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out, size_t cap,
                          size_t* k_out)
{
    return turn_flight_finish(c, row_out, live_out, user_out, start_out, end_out, cap, k_out, false, "pie_token_turn_finish");
}

int pie_token_turn_room(pie_ctx* c) { return c ? kTokTurns - c->tokx.tn_n : PIE_E_INVAL; }

int pie_shard_token_turn_begin(pie_ctx* c, const pie_turn_op* ops, size_t k)
{
    return turn_flight_begin(c, ops, k, true, "pie_shard_token_turn_begin");
}

int pie_shard_token_turn_finish(pie_ctx* c, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                                int64_t* end_out, size_t cap, size_t* k_out)
{
    return turn_flight_finish(c, row_global_out, live_out, user_global_out, start_out, end_out, cap, k_out, true, "pie_shard_token_turn_finish");
}

// ---- the expired queue beside scans and batches (pie_expired_queue_begin / _finish, include/pie_scan.h; kernels: pie_expq.h).
// pie_expired_queue is refused in flight only because it borrows the scan slots' workspace; this form owns what it writes
// (c->expq) and reads what scans and batches read.

// the table a begin needs (the shard form: one whose row map covers its rows)
static int expq_ready(pie_ctx* c, bool global, const char* what)
{
    if (c->cap_rows == 0) return fail(c, PIE_E_STATE, "%s: no table loaded", what);
    if (global) {
        if (!c->shard_on || !c->d_shard_rows) return fail(c, PIE_E_STATE, "%s: the context holds no sharded table (pie_shard_table)", what);
        if (c->n != c->shard_rows_n)
            return fail(c, PIE_E_STATE, "%s: %lld rows were added after pie_shard_table: they have no global row", what, c->n - c->shard_rows_n);
    }
    return PIE_OK;
}

static int expq_begin(pie_ctx* c, int64_t prev_now, int64_t now, size_t cap_rows, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    const int ready_rc = expq_ready(c, global, what);
    if (ready_rc) return ready_rc;
    pie_ctx::ExpiredFlight& x = c->expq;
    if (x.begun) return fail(c, PIE_E_STATE, "%s: an expired queue is begun and not finished", what);
    if (cap_rows >= ((size_t)1 << 31)) return fail(c, PIE_E_INVAL, "%s: cap_rows %zu", what, cap_rows);
    const ExpqPlan plan = expq_plan_of(c->n, c->n_cus, x.blocks_per_cu, x.max_blocks);
    if (plan.units < 0) return fail(c, PIE_E_INVAL, "%s: no plan for %lld rows", what, c->n);
    PIE_HIP(c, hipSetDevice(c->device));
    const ExpqScratch sc = expq_scratch_of();
    const int open_rc = side_open(c, x.side); // stale: what a given-up wait left on the stream may still write the buffer
    if (open_rc) return open_rc;
    if (!x.t0) PIE_HIP(c, hipEventCreate(&x.t0));
    if (!x.h_sum) {
        HostSummary* h = nullptr;
        PIE_HIP(c, hipHostMalloc(&h, sizeof(HostSummary), hipHostMallocMapped));
        memset(h, 0, sizeof(HostSummary));
        if (hipHostGetDevicePointer((void**)&x.h_sum_dev, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            return fail(c, PIE_E_HIP, "%s: no device view of the summary", what);
        }
        x.h_sum = h;
    }
    if (!x.d_scratch) {
        char* d = nullptr;
        if (hipMalloc(&d, sc.bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, PIE_E_NOMEM, "%s: no device memory for the scratch", what);
        }
        if (hipMemsetAsync(d + sc.ctl, 0, sc.bytes - sc.ctl, x.side.stream) != hipSuccess) { // the done counter; every pass leaves it at zero
            (void)hipGetLastError();
            (void)hipFree(d);
            return fail(c, PIE_E_HIP, "%s: cannot clear the scratch", what);
        }
        x.d_scratch = d;
    }
    if (cap_rows > x.buf_rows) {
        // the old buffer waits for the next call that has drained the context anyway (free_table, pie_ctx_destroy)
        const size_t rows = expq_buffer_rows(x.buf_rows, cap_rows);
        int* nb = nullptr;
        if (hipMalloc(&nb, rows * 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, PIE_E_NOMEM, "%s: no device memory for a queue of %zu rows", what, cap_rows);
        }
        if (!side_retire(x.side, nullptr, x.d_buf)) {
            (void)hipFree(nb);
            return fail(c, PIE_E_NOMEM, "%s: out of host memory", what);
        }
        x.d_buf = nb;
        x.buf_rows = rows;
    }
    x.launched = c->n > 0 && prev_now < now; // an empty table or an empty window: an empty queue, nothing to run
    if (x.launched) {
        hipStream_t s = x.side.stream;
        const int enter_rc = side_enter(c, x.side, x.fence, hipEventDefault); // `done` is timed
        if (enter_rc) return enter_rc;
        PIE_HIP(c, hipEventRecord(x.t0, s));
        int* d_count = reinterpret_cast<int*>(x.d_scratch + sc.counts);
        long long* d_off = reinterpret_cast<long long*>(x.d_scratch + sc.offsets);
        ExpqCtl* d_ctl = reinterpret_cast<ExpqCtl*>(x.d_scratch + sc.ctl);
        const bool keyed = c->key_ok && c->keyed_enabled && c->d_key && !getenv("PIE_EXPIRED_ON_END"); // pie_expired_queue's choice
        const unsigned kp = keyed ? host_key_of(c, prev_now) : 0u, kn = keyed ? host_key_of(c, now) : 0u;
        const int units = (int)plan.units;
        const int* map = global ? (const int*)c->d_shard_rows : (const int*)nullptr;
        const unsigned long long seq = x.seq + 1;
        const bool count_only = cap_rows == 0;
        const dim3 grid((unsigned)plan.blocks), block(256);
#define PIE_EXPQ_LAUNCH(KEYED, WRITE)                                                                                                    \
    hipLaunchKernelGGL((k_expq_pass<KEYED, WRITE>), grid, block, 0, s, (const lkey_t*)c->d_key, (const long long*)c->d_end, c->n,         \
                       plan.rows_per_unit, units, (long long)prev_now, (long long)now, kp, kn, d_count, (const long long*)d_off, x.d_buf, \
                       (long long)cap_rows, map, d_ctl, x.h_sum_dev, seq)
        if (keyed) PIE_EXPQ_LAUNCH(true, false);
        else PIE_EXPQ_LAUNCH(false, false);
        // a counting pass ends with the prefix kernel, which then hands the length to the host itself
        hipLaunchKernelGGL(k_block_prefix_wide, dim3(1), dim3(1024), 0, s, (const int*)d_count, units, d_off, (unsigned long long*)nullptr,
                           count_only ? x.h_sum_dev : (HostSummary*)nullptr, seq);
        if (!count_only) {
            if (keyed) PIE_EXPQ_LAUNCH(true, true);
            else PIE_EXPQ_LAUNCH(false, true);
        }
#undef PIE_EXPQ_LAUNCH
        const hipError_t le = hipGetLastError();
        // `done` and the context's wait for it are queued even behind a failed launch: what did start must not be overtaken
        const hipError_t we = side_leave(c, x.side, x.fence);
        if (le != hipSuccess || we != hipSuccess) {
            x.side.stale = true;
            return fail(c, PIE_E_HIP, "%s: %s", what, hipGetErrorString(le != hipSuccess ? le : we));
        }
        x.seq = seq;
        x.timed = true;
    }
    x.cap_rows = cap_rows;
    x.global = global;
    x.landed = !x.launched;
    x.begun = true;
    return PIE_OK;
}

static int expq_finish(pie_ctx* c, int32_t* queue_out, size_t cap, size_t* q_out, bool global, const char* what)
{
    if (!c) return PIE_E_INVAL;
    pie_ctx::ExpiredFlight& x = c->expq;
    if (!x.begun) return fail(c, PIE_E_STATE, "%s: no expired queue was begun", what);
    if (x.global != global) return fail(c, PIE_E_STATE, "%s: the queue was begun by the %s form", what, x.global ? "shard" : "plain");
    if (queue_out && cap < x.cap_rows) return fail(c, PIE_E_INVAL, "%s: room for %zu rows, the begin asked for %zu", what, cap, x.cap_rows);
    PIE_HIP(c, hipSetDevice(c->device));
    const int rc = expq_land(c, what);
    x.begun = false; // the pass is consumed whatever the wait said
    if (rc) {
        x.side.stale = true;
        return rc;
    }
    const size_t len = x.launched ? (size_t)x.h_sum->s.m : 0;
    if (q_out) *q_out = len;
    const size_t rows = len < x.cap_rows ? len : x.cap_rows;
    if (queue_out && rows) {
        const hipError_t ce = hipMemcpyAsync(queue_out, x.d_buf, rows * 4, hipMemcpyDeviceToHost, x.side.stream);
        const hipError_t se = ce == hipSuccess ? hipStreamSynchronize(x.side.stream) : ce; // the pass's own stream, nobody else's
        if (se != hipSuccess) {
            x.side.stale = true;
            return fail(c, PIE_E_HIP, "%s: %s", what, hipGetErrorString(se));
        }
    }
    if (x.cap_rows > 0 && len > x.cap_rows) return fail(c, PIE_E_CAPACITY, "%s: %zu rows, the begin asked for %zu", what, len, x.cap_rows);
    return PIE_OK;
}

int pie_expired_queue_begin(pie_ctx* c, int64_t prev_now, int64_t now, size_t cap_rows)
{
    return expq_begin(c, prev_now, now, cap_rows, false, "pie_expired_queue_begin");
}

int pie_expired_queue_finish(pie_ctx* c, int32_t* queue_out, size_t cap, size_t* q_out)
{
    return expq_finish(c, queue_out, cap, q_out, false, "pie_expired_queue_finish");
}

int pie_expired_queue_room(pie_ctx* c) { return c ? (c->expq.begun ? 0 : 1) : PIE_E_INVAL; }

int pie_shard_expired_queue_begin(pie_ctx* c, int64_t prev_now, int64_t now, size_t cap_rows)
{
    return expq_begin(c, prev_now, now, cap_rows, true, "pie_shard_expired_queue_begin");
}

int pie_shard_expired_queue_finish(pie_ctx* c, int32_t* rows_global_out, size_t cap, size_t* q_out)
{
    return expq_finish(c, rows_global_out, cap, q_out, true, "pie_shard_expired_queue_finish");
}

int pie_expired_inflight_geometry(pie_ctx* c, size_t n, int32_t* rows_per_wave_step_out, int64_t* rows_per_unit_out, int32_t* blocks_out)
{
    if (!c) return PIE_E_INVAL;
    if (n >= (size_t)kExpqMaxRows) return fail(c, PIE_E_INVAL, "pie_expired_inflight_geometry: %zu rows", n);
    const ExpqPlan p = expq_plan_of((long long)n, c->n_cus, c->expq.blocks_per_cu, c->expq.max_blocks);
    if (rows_per_wave_step_out) *rows_per_wave_step_out = p.rows_per_wave_step;
    if (rows_per_unit_out) *rows_per_unit_out = p.rows_per_unit;
    if (blocks_out) *blocks_out = p.blocks;
    return PIE_OK;
}

} // extern "C"

// What the communicator's in-flight calls (pie_comm_token_lookup_begin ..., pie_comm_expired_queue_begin ...) need of a shard
// beyond the pie_shard_* entry points: the checks of a begin with nothing begun, the newest lookup taken back, and the finished
// queue left where the pass wrote it.
namespace pie_internal {
int shard_token_flight_check(pie_ctx* c, const char* what) { return c ? token_flight_ready(c, what, true) : PIE_E_INVAL; }

int shard_expq_check(pie_ctx* c, const char* what) { return c ? expq_ready(c, true, what) : PIE_E_INVAL; }

// the lookup begun LAST is waited for (bounded) and its slot returned: a begin that went through here and failed on another shard
int shard_token_flight_drop_last(pie_ctx* c, const char* what)
{
    if (!c) return PIE_E_INVAL;
    pie_ctx::TokenIndex& t = c->tokx;
    if (t.lk_n == 0) return fail(c, PIE_E_STATE, "%s: no lookup was begun", what);
    if (hipSetDevice(c->device) != hipSuccess) (void)hipGetLastError();
    const int rc = flight_slot_landed(c, t.lk[(t.lk_head + t.lk_n - 1) % kTokLookups], what);
    t.lk_n--;
    if (rc) t.side.stale = true;
    return rc;
}

// pie_shard_expired_queue_finish without its copy: the bounded wait for the pass, which is consumed whatever the wait said.  The
// queue stays in the pass's own buffer (GLOBAL rows, the first min(*len_out, cap_rows) of them) until the shard's next begin;
// *stream_out is the pass's stream, *done_out the event behind its last kernel (nullptr: the pass had none).
int shard_expq_take(pie_ctx* c, const char* what, const int32_t** rows_dev_out, size_t* len_out, void** stream_out, void** done_out)
{
    if (!c) return PIE_E_INVAL;
    pie_ctx::ExpiredFlight& x = c->expq;
    if (!x.begun) return fail(c, PIE_E_STATE, "%s: no expired queue was begun", what);
    if (!x.global) return fail(c, PIE_E_STATE, "%s: the queue was begun by the plain form", what);
    PIE_HIP(c, hipSetDevice(c->device));
    const int rc = expq_land(c, what);
    x.begun = false;
    if (rc) {
        x.side.stale = true;
        return rc;
    }
    *rows_dev_out = x.d_buf;
    *len_out = x.launched ? (size_t)x.h_sum->s.m : 0;
    *stream_out = x.side.stream;
    *done_out = x.launched ? x.fence.done : nullptr;
    return PIE_OK;
}

// a reader of the pass's buffer on *stream_out gave up its wait: the shard's next begin drains that stream first
void shard_expq_stale(pie_ctx* c)
{
    if (c) c->expq.side.stale = true;
}
} // namespace pie_internal
