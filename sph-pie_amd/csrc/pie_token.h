// pie_token.h — the token column and its index: getSession (server/sessionStore.js:21-35) for a whole event-loop turn in one
// launch.  gfx950, wave64.  Included by pie_scan.hip behind pie_kernels.h; pie_scan.hip holds the host side (pie_token_*,
// pie_shard_token_*).
//
// Token key: the first 16 bytes of the sha256 the reference uses as its Map key (sessionStore.js:8-10), as two little-endian
// 64-bit words per row.  The device never hashes a token; the host does (binding.token_key, host/tokenKeys.js).
//
// Column:  tok[row] (16 B per row of capacity) for the rows [0, covered) — a prefix of the table.
// Index:   slot_row[slots] (int32; -1 empty, otherwise a row), slots a power of two >= max(1024, 2 x covered): at most half full.
//          home slot = the top log2(slots) bits of token_mix(key); linear probing, wrapping at the end of the table.
//          The key is NOT stored in the slot: a probe reads slot_row[s], then tok[row] as one 16-byte load.
//          There is no deleted state: an entry leaves only when compaction drops its row (the index is rebuilt then).
// Every probe loop runs at most `slots` steps; a lane that exhausts the bound sets a status word and stops.
#ifndef PIE_TOKEN_H
#define PIE_TOKEN_H

#include <hip/hip_runtime.h>

namespace pie {

typedef ulonglong2 TokKey; // .x = bytes 0..7, .y = bytes 8..15 of the sha256, little endian

constexpr int kTokStatusWords = 4; // [0] an insert exhausted its probe bound, [1] a lookup did, [2] a sharded create's user is unknown
constexpr int kTokLookups = 4;     // lookups begun and not finished beside scans and batches (pie_token_lookup_begin)
constexpr int kTokTurns = 4;       // turns begun and not finished beside scans and batches (pie_token_turn_begin)

// 64-bit mix of a key: the splitmix64 finaliser (the one pie_shard_of applies to a user id) over k0 ^ rotl(k1, 32)
__host__ __device__ __forceinline__ unsigned long long token_mix(unsigned long long k0, unsigned long long k1)
{
    unsigned long long z = (k0 ^ ((k1 << 32) | (k1 >> 32))) + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__host__ __device__ __forceinline__ unsigned long long token_home(unsigned long long k0, unsigned long long k1, unsigned log2_slots)
{
    return log2_slots ? token_mix(k0, k1) >> (64 - log2_slots) : 0ull;
}

// Claim the first empty slot from the key's home for `row`.  Keys are never compared, so rows with equal keys all get in.  The
// claim is a relaxed agent-scope compare-and-swap: every reader is a later kernel on the stream.  At most `slots` steps; a lane
// that exhausts them sets status[0].
__device__ __forceinline__ void token_claim(TokKey key, int row, int* slot_row, unsigned log2_slots, unsigned int* status)
{
    const unsigned long long slots = 1ull << log2_slots, mask = slots - 1;
    unsigned long long s = token_home(key.x, key.y, log2_slots);
    unsigned long long step = 0;
    for (; step < slots; ++step) {
        int expected = -1;
        if (__hip_atomic_compare_exchange_strong(&slot_row[s], &expected, row, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        s = (s + 1) & mask;
    }
    if (step == slots) status[0] = 1u;
}

// One lane per row of [row0, row0 + k): token_claim for the row's key.
__global__ __launch_bounds__(256) void k_token_insert(const TokKey* __restrict__ tok, long long row0, long long k, int* __restrict__ slot_row,
                                                      unsigned log2_slots, unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const long long row = row0 + t;
    token_claim(tok[row], (int)row, slot_row, log2_slots, status);
}

// The probe every lookup runs: walk from the key's home slot to the first empty slot; among the slots whose row carries the key
// (both words) keep the largest row.  `bound` keeps the 16-byte load inside the column whatever the slot holds (always true for an
// index in step with its column).  At most `slots` steps; a lane that exhausts them sets status[1].  -> the row, or -1.
__device__ __forceinline__ int token_probe(TokKey key, const int* __restrict__ slot_row, unsigned log2_slots, const TokKey* __restrict__ tok,
                                           long long bound, unsigned int* __restrict__ status)
{
    const unsigned long long slots = 1ull << log2_slots, mask = slots - 1;
    unsigned long long s = token_home(key.x, key.y, log2_slots);
    int best = -1;
    unsigned long long step = 0;
    for (; step < slots; ++step) {
        const int r = slot_row[s];
        if (r < 0) break;
        if ((long long)r < bound) {
            const TokKey have = tok[r];
            if (have.x == key.x && have.y == key.y && r > best) best = r;
        }
        s = (s + 1) & mask;
    }
    if (step == slots) status[1] = 1u;
    return best;
}

// the two maps of a sharded context (kShard): rows and users are answered as GLOBAL ids, both reads bounded (best < n_local by the
// probe's bound, user < n_users; -1 otherwise)
struct ShardMaps {
    const int* rows;
    long long n_local;
    const int* users;
    int n_users;
};

// What every lookup answers for key t once its probe gave `best`: of several sessions under one key the latest (largest row) won.
// kShard: the row and the user as GLOBAL ids through the two maps.  kOptional: an output may be absent (NULL), and what it would
// have held is not read.  *now is the key's clock, read where `live` is decided.
template <bool kShard, bool kOptional>
__device__ __forceinline__ void token_answer(long long t, int best, const long long* now, const long long* end, const long long* start, const int* user,
                                             ShardMaps maps, int* o_row, unsigned char* o_live, int* o_user, long long* o_start, long long* o_end)
{
    const long long e = best >= 0 ? end[best] : INT64_MIN;
    if (!kOptional || o_row) o_row[t] = !kShard ? best : best >= 0 ? maps.rows[best] : -1;
    if (!kOptional || o_live) o_live[t] = (best >= 0 && e > *now) ? 1 : 0;
    if (!kOptional || o_end) o_end[t] = e;
    if (!kOptional || o_start) o_start[t] = best >= 0 ? start[best] : 0;
    if (!kOptional || o_user) {
        const int u = best >= 0 ? user[best] : -1;
        o_user[t] = !kShard ? u : (u >= 0 && u < maps.n_users) ? maps.users[u] : -1;
    }
}

// One lane per query key, one clock for all of them.  Outputs may be absent (NULL).
__global__ __launch_bounds__(256) void k_token_lookup(const TokKey* __restrict__ query, long long k, const int* __restrict__ slot_row, unsigned log2_slots,
                                                      const TokKey* __restrict__ tok, long long covered, const long long* __restrict__ end,
                                                      const long long* __restrict__ start, const int* __restrict__ user, long long now,
                                                      int* __restrict__ o_row, unsigned char* __restrict__ o_live, int* __restrict__ o_user,
                                                      long long* __restrict__ o_start, long long* __restrict__ o_end, unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int best = token_probe(query[t], slot_row, log2_slots, tok, covered, status);
    token_answer<false, true>(t, best, &now, end, start, user, ShardMaps{}, o_row, o_live, o_user, o_start, o_end);
}

// ---- the token column of a SHARDED context (pie_shard_token_*): keys are given by GLOBAL row; a shard keeps the keys of the rows
// its ascending row map holds (shard_lower_bound, pie_kernels.h) and indexes them by LOCAL row, exactly as above.

// pie_shard_token_append: one lane per key of the staged chunk, which belongs to the global rows [g0, g0 + k).  The lane whose
// global row the shard holds (local row r < n_local, inside the column's capacity) stores the key as one 16-byte store to tok[r]
// and claims a slot for r (token_claim).  The key a probe compares against is written by the lane that claims the slot, and
// every reader is a later kernel on the stream.
__global__ __launch_bounds__(256) void k_shard_token_place(const TokKey* __restrict__ staged, long long g0, long long k,
                                                           const int* __restrict__ rows_map, long long n_local, TokKey* __restrict__ tok,
                                                           long long cap, int* __restrict__ slot_row, unsigned log2_slots,
                                                           unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const long long g = g0 + t;
    if (g > 0x7fffffffLL) return;
    const long long r = shard_lower_bound(rows_map, n_local, (int)g);
    if (r >= n_local || r >= cap || (long long)rows_map[r] != g) return; // another shard's row, or one this shard's compactions dropped
    const TokKey key = staged[t];
    tok[r] = key;
    token_claim(key, (int)r, slot_row, log2_slots, status);
}

// pie_shard_token_lookup: k_token_lookup with the row (o_grow) and the user answered as GLOBAL ids; the LOCAL row, which only this
// form gives beside the global one, goes to o_row.  `bound` = the rows the column can hold keys for.
__global__ __launch_bounds__(256) void k_shard_token_lookup(const TokKey* __restrict__ query, long long k, const int* __restrict__ slot_row,
                                                            unsigned log2_slots, const TokKey* __restrict__ tok, long long bound,
                                                            const long long* __restrict__ end, const long long* __restrict__ start,
                                                            const int* __restrict__ user, const int* __restrict__ rows_map, long long n_local,
                                                            const int* __restrict__ users_map, int n_map, long long now, int* __restrict__ o_row,
                                                            int* __restrict__ o_grow, unsigned char* __restrict__ o_live, int* __restrict__ o_user,
                                                            long long* __restrict__ o_start, long long* __restrict__ o_end,
                                                            unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int best = token_probe(query[t], slot_row, log2_slots, tok, bound < n_local ? bound : n_local, status);
    if (o_row) o_row[t] = best;
    token_answer<true, true>(t, best, &now, end, start, user, ShardMaps{rows_map, n_local, users_map, n_map}, o_grow, o_live, o_user, o_start, o_end);
}

// ---- lookups that run beside scans and batches (pie_token_lookup_begin / _finish): the same probe and the same answer on a
// stream of the lookup's own.  Each key carries its own clock (now[t]: the requests of a turn were stamped one by one), every
// output is written, and `status` points at the status words of the lookup's slot, so the report of one lookup is nobody else's.
// One lane per key, a grid of ceil(k / 256) blocks that come and go (no persistent grid, no LDS, no barrier): a turn's worth of
// keys is a handful of waves for a few microseconds, which leaves the wave slots and the LDS of every CU to the batch lanes'
// kernels.
__global__ __launch_bounds__(256) void k_token_lookup_now(const TokKey* __restrict__ query, const long long* __restrict__ now, long long k,
                                                          const int* __restrict__ slot_row, unsigned log2_slots, const TokKey* __restrict__ tok,
                                                          long long covered, const long long* __restrict__ end,
                                                          const long long* __restrict__ start, const int* __restrict__ user,
                                                          int* __restrict__ o_row, unsigned char* __restrict__ o_live, int* __restrict__ o_user,
                                                          long long* __restrict__ o_start, long long* __restrict__ o_end,
                                                          unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int best = token_probe(query[t], slot_row, log2_slots, tok, covered, status);
    token_answer<false, false>(t, best, now + t, end, start, user, ShardMaps{}, o_row, o_live, o_user, o_start, o_end);
}

// the shard form: the row and the user answered as GLOBAL ids through the two maps
__global__ __launch_bounds__(256) void k_shard_token_lookup_now(const TokKey* __restrict__ query, const long long* __restrict__ now, long long k,
                                                                const int* __restrict__ slot_row, unsigned log2_slots,
                                                                const TokKey* __restrict__ tok, long long bound, const long long* __restrict__ end,
                                                                const long long* __restrict__ start, const int* __restrict__ user,
                                                                const int* __restrict__ rows_map, long long n_local,
                                                                const int* __restrict__ users_map, int n_map, int* __restrict__ o_grow,
                                                                unsigned char* __restrict__ o_live, int* __restrict__ o_user,
                                                                long long* __restrict__ o_start, long long* __restrict__ o_end,
                                                                unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    const int best = token_probe(query[t], slot_row, log2_slots, tok, bound < n_local ? bound : n_local, status);
    token_answer<true, false>(t, best, now + t, end, start, user, ShardMaps{rows_map, n_local, users_map, n_map}, o_grow, o_live, o_user, o_start, o_end);
}

// ---- a whole turn (pie_token_turn / pie_shard_token_turn, include/pie_scan.h): an ordered list of get / touch / delete ops, each
// with its own clock (sessionStore.js:21-53), answered and applied in one launch.
//
// The host has cut the turn into chains (pie_turn_plan.h): the ops that name one key, in array order, linked through next[].  One
// thread per op; a thread whose op is not the head of a chain returns.  A head thread probes the index once (token_probe: the
// bounded loop and the status word of every lookup), reads end / start / user of the row once, then walks its chain with `e`, the
// row's `end`, in a register: every op is judged against the `e` the ops before it left, and its results are written where the op
// stands in the array.  If `e` ends the walk with another value than the row had, touch_row stores it — once, and nowhere else:
// `end`, both keys, the ordered run's mirror and the hot index's mirror move together.
// Distinct keys have distinct rows (a key's row is the largest row that carries it), and all the ops of one key are walked by one
// thread: no two threads ever write the same row, and no thread reads an `end` another one writes.  So the kernel needs no atomic
// of its own, no barrier and no LDS, and nothing in it spins: the probe runs at most `slots` steps, the walk at most k (next[]
// ascends; an entry that does not is the end of the chain).  A chain is walked by ONE lane: a turn in which every op names one
// token costs k serial steps.
// The uploaded array is the caller's pie_turn_op array with the `reserved` word (0 in the ABI) carrying the head flag.
// `status` is whatever the host hands in: the context's words for pie_token_turn, the words inside the staging of its own slot for
// a turn begun beside scans and batches (pie_token_turn_begin).  The kernel only ever raises status[1] (token_probe), so a turn
// neither raises nor clears the report of another; the in-flight form needs no variant of the kernel.
struct alignas(8) TurnOp {
    unsigned long long k0, k1;
    long long now, new_end;
    int kind, head;
};
static_assert(sizeof(TurnOp) == 40, "TurnOp mirrors pie_turn_op");
constexpr int kTurnGet = 0, kTurnTouch = 1, kTurnDelete = 2, kTurnCreate = 3;

// One get / touch / delete op against its key's row, whose `end` is `e` (the rules of the table in include/pie_scan.h): `e` moves
// as the op says, `r` becomes -1 for a delete that wrote nothing.  -> live_out.  Shared by k_token_turn and k_session_turn.
__device__ __forceinline__ unsigned char turn_apply(const TurnOp& op, bool found, long long& e, int& r)
{
    if (op.kind == kTurnTouch) {
        if (found && e > op.now) {
            e = op.new_end;
            return 1;
        }
        return 0;
    }
    if (op.kind == kTurnDelete) {
        if (found && e != INT64_MIN) e = INT64_MIN;
        else r = -1;
        return 0;
    }
    return (found && e > op.now) ? 1 : 0;
}

template <bool kShard>
__global__ __launch_bounds__(256) void k_token_turn(const TurnOp* __restrict__ ops, const int* __restrict__ next, long long k,
                                                    const int* __restrict__ slot_row, unsigned log2_slots, const TokKey* __restrict__ tok,
                                                    long long bound, long long* __restrict__ end, const long long* __restrict__ start,
                                                    const int* __restrict__ user, ShardMaps maps, lkey_t* __restrict__ key, long long key_base,
                                                    int key_shift, fkey_t* __restrict__ fkey, long long fkey_base, int fkey_shift, OrdMirror ord,
                                                    HotMirror hot, int* __restrict__ o_row, unsigned char* __restrict__ o_live,
                                                    int* __restrict__ o_user, long long* __restrict__ o_start, long long* __restrict__ o_end,
                                                    unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    TurnOp op = ops[t];
    if (!op.head) return;
    TokKey want;
    want.x = op.k0;
    want.y = op.k1;
    const int best = token_probe(want, slot_row, log2_slots, tok, kShard && maps.n_local < bound ? maps.n_local : bound, status);
    const bool found = best >= 0;
    const long long e0 = found ? end[best] : INT64_MIN;
    const long long sv = found ? start[best] : 0;
    int uv = found ? user[best] : -1, rv = best;
    if (kShard) {
        rv = found ? maps.rows[best] : -1;
        uv = (uv >= 0 && uv < maps.n_users) ? maps.users[uv] : -1;
    }
    long long e = e0, j = t;
    for (long long step = 0; step < k; ++step) {
        int r = rv;
        const unsigned char live = turn_apply(op, found, e, r);
        o_row[j] = r;
        o_live[j] = live;
        o_end[j] = e;
        o_start[j] = sv;
        o_user[j] = uv;
        const long long nx = next[j];
        if (nx <= j || nx >= k) break;
        j = nx;
        op = ops[j];
    }
    if (e != e0) touch_row(best, e, end, key, key_base, key_shift, fkey, fkey_base, fkey_shift, ord, hot);
}

// ---- a turn that logs in (pie_session_turn, pie_shard_session_turn): k_token_turn's walk with a fourth kind, CREATE.  The plain
// form first; what kShard adds stands below it.
//
// The uploaded op's `head` word carries the head flag in bit 0 and, for a CREATE, the create's ordinal j in the bits above: the
// j-th create of the array becomes row row0 + j (the host counted; no device atomic) and takes user / disc from the compact
// arrays cuser[j] / cdisc[j].  The host has made room: row0 + creates <= the capacity of the columns, of tok[] and of the hot
// index's pos[], and the slots stay at most half full with every create in.
// A head lane probes ONCE, before anything its chain creates, and walks the chain as k_token_turn does, with the row it is on and
// that row's `end` in registers.  At a CREATE the lane
//   1. stores the change earlier ops left in the old row's `end` (touch_row),
//   2. writes the new row (append_row: four columns, both keys, the payload record, the hot mirror),
//   3. stores tok[new row] as one 16-byte store,
//   4. claims the first empty slot from the key's home (token_claim: exhaustion raises status[0]),
//   5. goes on with the new row's values in registers.  It does not probe again.
// The hazard: a lane probing for ANOTHER key can meet a slot claimed in this same launch, whose tok[] entry is not written yet
// (or not visible yet), and memory past the covered prefix can hold stale keys after a compaction.  So every probe of this kernel
// runs with `bound` = the rows covered BEFORE the turn: token_probe steps over a slot that names a newer row without reading tok.
// That is enough: (a) a key's pre-existing entries all lie between its home and the first slot that was empty at launch, and
// inserts only fill empty slots, so a probe that steps over new entries still reaches every old one, and one that reads a slot as
// still empty stops where it would have stopped before the launch; (b) all the ops of one key belong to one lane, so the rows a
// launch creates under a key matter to that lane alone, which has them in registers.  Readers of the new entries are later
// kernels on the stream.  No spin, no barrier, no LDS; the only atomics are the slot claim and the hot mirror's own.
// Rows: distinct keys have distinct rows and every new row belongs to one create, so no two lanes write one row.
//
// kShard (pie_shard_session_turn): the same walk on one shard of a sharded table.  row0 is N_g, the GLOBAL row count before the
// turn: the create of ordinal j is global row N_g + j on every shard.  crow[j] is the LOCAL row the shard gives it, or -1 when
// another shard keeps it; cuser[j] is the GLOBAL user, found in the user map by shard_lower_bound as k_shard_append_rows finds it
// (the new users of the call are behind the map in stream order).  A kept create also stores rows_map[local row] = N_g + j; the
// local rows ascend with the ordinal, so the map stays ascending.  A create the shard does not keep answers -1 / 0 / INT64_MIN /
// -1 and leaves the lane on whatever row the key had here; so does one whose user the map does not hold, which also raises
// status[2] (the host has checked every id: this keeps a slip from reaching an index).  Rows and users are answered as GLOBAL
// ids, as k_token_turn<true> answers them.  The argument about probes carries over with `bound` = min(bound, the local rows
// before the turn): all of them are covered, because the host refuses a create while covered_g < N_g.
template <bool kShard>
__global__ __launch_bounds__(256) void k_session_turn(const TurnOp* __restrict__ ops, const int* __restrict__ next, long long k,
                                                      const int* __restrict__ cuser, const int* __restrict__ cdisc,
                                                      const int* __restrict__ crow, long long row0, int* slot_row, unsigned log2_slots,
                                                      TokKey* tok, long long bound, long long* start, long long* end, int* user, int* disc,
                                                      ShardMaps maps, int* rows_map, lkey_t* key, long long key_base, int key_shift,
                                                      fkey_t* fkey, long long fkey_base, int fkey_shift, PayRec* pay, OrdMirror ord,
                                                      HotMirror hot, int* __restrict__ o_row, unsigned char* __restrict__ o_live,
                                                      int* __restrict__ o_user, long long* __restrict__ o_start,
                                                      long long* __restrict__ o_end, unsigned int* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= k) return;
    TurnOp op = ops[t];
    if (!(op.head & 1)) return;
    TokKey want;
    want.x = op.k0;
    want.y = op.k1;
    int row = token_probe(want, slot_row, log2_slots, tok, kShard && maps.n_local < bound ? maps.n_local : bound, status);
    bool found = row >= 0;
    long long e0 = found ? end[row] : INT64_MIN, sv = found ? start[row] : 0;
    int uv = found ? user[row] : -1, rv = row; // what the lane answers for its row and user: GLOBAL ids on a shard
    if (kShard) {
        rv = found ? maps.rows[row] : -1;
        uv = (uv >= 0 && uv < maps.n_users) ? maps.users[uv] : -1;
    }
    // the ordered run (ord, when the host keeps it through the turn) holds the rows from before the turn only: a row the turn itself
    // creates has no pos[] entry until the insert behind this kernel has run, so a store to one changes the table alone
    const long long first_new = kShard ? maps.n_local : row0;
    const OrdMirror no_ord{};
    long long e = e0, j = t;
    for (long long step = 0; step < k; ++step) {
        int r = rv;
        unsigned char live;
        bool kept = true;
        if (op.kind == kTurnCreate) {
            const long long c = (long long)((unsigned)op.head >> 1);
            long long nr = row0 + c;
            int lu = cuser[c]; // the user as the row stores it: the LOCAL id on a shard
            if (kShard) {
                nr = crow[c];
                kept = nr >= 0;
                if (kept) {
                    const long long p = shard_lower_bound(maps.users, (long long)maps.n_users, lu);
                    if (p < (long long)maps.n_users && maps.users[p] == lu) lu = (int)p;
                    else {
                        status[2] = 1u;
                        kept = false;
                    }
                }
            }
            if (kept) {
                if (found && e != e0)
                    touch_row(row, e, end, key, key_base, key_shift, fkey, fkey_base, fkey_shift, row < first_new ? ord : no_ord, hot);
                row = (int)nr;
                rv = r = kShard ? (int)(row0 + c) : row;
                found = true;
                sv = op.now;
                e = e0 = op.new_end;
                uv = cuser[c];
                append_row(row, sv, e, lu, cdisc[c], start, end, user, disc, key, key_base, key_shift, fkey, fkey_base, fkey_shift, pay, hot);
                if (kShard) rows_map[row] = rv;
                tok[row] = want;
                token_claim(want, row, slot_row, log2_slots, status);
            }
            live = kept && e > op.now ? 1 : 0;
        } else live = turn_apply(op, found, e, r);
        o_row[j] = kept ? r : -1;
        o_live[j] = live;
        o_end[j] = kept ? e : INT64_MIN;
        o_start[j] = kept ? sv : 0;
        o_user[j] = kept ? uv : -1;
        const long long nx = next[j];
        if (nx <= j || nx >= k) break;
        j = nx;
        op = ops[j];
    }
    if (found && e != e0) touch_row(row, e, end, key, key_base, key_shift, fkey, fkey_base, fkey_shift, row < first_new ? ord : no_ord, hot);
}

// the compaction hook: the keys of the kept covered rows, in their new places
__global__ __launch_bounds__(256) void k_token_gather(const TokKey* __restrict__ tok_old, const int* __restrict__ old_of_new, long long n_new,
                                                      long long covered_old, TokKey* __restrict__ tok_new)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_new; i += (long long)gridDim.x * blockDim.x) {
        const long long r = old_of_new[i];
        if (r >= 0 && r < covered_old) tok_new[i] = tok_old[r];
    }
}

} // namespace pie
#endif /* PIE_TOKEN_H */
