// pie_comm.hip — the multi-GPU exchange behind the C ABI (include/pie_scan.h, "communicator" section): user-hash shards
// of one session table on the GPUs of one node, one batched scan per shard, and the reassembly of cross-user feeds by
// RCCL over xGMI — callable from a host that is not Python (the Node addon binds these entry points).
//
// Built on the public ABI only (a pie_ctx per GPU) plus RCCL, which is opened at run time (dlopen "librccl.so.1": the
// scan library itself stays loadable on a box without RCCL; pie_comm_create then fails with PIE_E_NODEVICE).
// xGMI is point-to-point (7 links per GPU), so the exchange is the DIRECT pattern: inside one ncclGroupStart / End every
// rank posts one ncclSend per peer and one ncclRecv per peer — each shard's message crosses its own link to each peer
// once — rather than a ring that would bound the step by one link.
#include "../../include/pie_scan.h"
#include "pie_wait.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

// pie_scan.hip: what pie_shard_append_rows / pie_shard_set_end would refuse, checked with nothing staged or changed
namespace pie_internal {
int shard_check_append(pie_ctx* c, const int32_t* user_global, size_t k, int32_t n_users_global);
int shard_check_set_end(pie_ctx* c, const int32_t* rows_global, const int64_t* new_end, size_t k);
// ... what pie_shard_token_set / pie_shard_token_append would refuse, and the two phases of pie_shard_token_lookup
int shard_token_check(pie_ctx* c, const uint64_t* tok, size_t k, bool set);
int shard_token_lookup_queue(pie_ctx* c, const uint64_t* tok, size_t k, int64_t now);
int shard_token_lookup_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                            int64_t* end_out);
// ... the three phases of pie_shard_token_turn: the checks with nothing staged or changed, the queue phase, the wait phase
int shard_token_turn_check(pie_ctx* c, const pie_turn_op* ops, size_t k);
int shard_token_turn_queue(pie_ctx* c, const pie_turn_op* ops, size_t k);
int shard_token_turn_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                          int64_t* end_out);
int shard_session_turn_check(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, const int32_t* disc, int32_t n_users_global);
int shard_session_turn_room(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, int32_t n_users_global);
int shard_session_turn_queue(pie_ctx* c, const pie_turn_op* ops, size_t k, const int32_t* user_global, const int32_t* disc, int32_t n_users_global);
int shard_session_turn_wait(pie_ctx* c, size_t k, int32_t* row_global_out, uint8_t* live_out, int32_t* user_global_out, int64_t* start_out,
                            int64_t* end_out);
// ... and pie_shard_delete_users in three pieces: the check, the run that leaves the ascending list of global rows on the device,
// the copy of that list
int shard_check_delete_users(pie_ctx* c, const int32_t* users_global, size_t k);
int shard_delete_users_run(pie_ctx* c, const int32_t* users_global, size_t k, size_t* m_out, int32_t* per_user_out);
int shard_delete_users_copy(pie_ctx* c, int32_t* rows_global_out, size_t m);
// ... and what the in-flight calls need beyond pie_shard_token_lookup_* / pie_shard_expired_queue_*: a begin's checks with nothing
// begun, the newest lookup taken back, the finished queue left in the pass's own buffer (its bounded wait; the pass is consumed)
int shard_token_flight_check(pie_ctx* c, const char* what);
int shard_expq_check(pie_ctx* c, const char* what);
int shard_token_flight_drop_last(pie_ctx* c, const char* what);
int shard_expq_take(pie_ctx* c, const char* what, const int32_t** rows_dev_out, size_t* len_out, void** stream_out, void** done_out);
void shard_expq_stale(pie_ctx* c);
// ... and pie_shard_prune_before / pie_shard_retention_purge / _tz (kind 2 / 3 / 4) in two pieces: the check, and the run that
// leaves the ascending global rows and, beside them, the local rows on the device; what pie_compact_rows would refuse on a shard
int shard_check_row_list(pie_ctx* c, int kind, int32_t months, int64_t tz_offset_ms, const int64_t* transitions, const int64_t* offsets,
                         int32_t n_transitions);
int shard_row_list_run(pie_ctx* c, int kind, int64_t a, int32_t months, int64_t tz_offset_ms, const int64_t* transitions, const int64_t* offsets,
                       int32_t n_transitions, size_t* m_out, const int32_t** rows_global_dev, const int32_t** rows_local_dev);
int shard_check_compact(pie_ctx* c, uint32_t flags);
} // namespace pie_internal

namespace {

// the slice of the RCCL API this file uses (signatures of /opt/rocm/include/rccl/rccl.h)
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef int ncclResult_t;
constexpr int kNcclInt32 = 2;

struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};

Rccl g_rccl;

bool load_rccl(char* err, size_t errlen)
{
    if (g_rccl.handle) return true;
    // PIE_RCCL_LIB: another library with the same entry points (tests/stub_rccl.c: several "ranks" of ONE process on ONE GPU,
    // which RCCL itself refuses — the stand-in that lets the communicator's logic run with world > 1 on a one-GPU box)
    const char* names[] = {getenv("PIE_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) {
        if (!n || !*n) continue;
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) {
        snprintf(err, errlen, "RCCL not found (%s)", dlerror());
        return false;
    }
    Rccl r;
    r.handle = h;
#define PIE_SYM(field, name)                                            \
    *(void**)(&r.field) = dlsym(h, name);                               \
    if (!r.field) {                                                     \
        snprintf(err, errlen, "RCCL symbol %s missing", name);          \
        return false;                                                   \
    }
    PIE_SYM(GetUniqueId, "ncclGetUniqueId")
    PIE_SYM(CommInitRank, "ncclCommInitRank")
    PIE_SYM(CommInitAll, "ncclCommInitAll")
    PIE_SYM(CommDestroy, "ncclCommDestroy")
    PIE_SYM(Send, "ncclSend")
    PIE_SYM(Recv, "ncclRecv")
    PIE_SYM(GroupStart, "ncclGroupStart")
    PIE_SYM(GroupEnd, "ncclGroupEnd")
    PIE_SYM(GetErrorString, "ncclGetErrorString")
#undef PIE_SYM
    g_rccl = r;
    return true;
}

thread_local char g_comm_create_error[256] = "";

} // namespace

// One pipelined union exchange (the state of pie_comm_step_*, and again of pie_comm_wide_step_*): rotating buffer sets per local
// rank, a ready and a done event per set and rank, and the gathered Mu words in mapped host memory.  Step i lives in set
// i % sets (StepKind) from its begin until `sets` more steps have begun.
struct pie_steps {
    static constexpr int kMaxSets = 16;
    std::vector<int*> msg[kMaxSets], gath[kMaxSets];       // [set][local index]: this rank's union message [L] / the gathered ones [world][L]
    std::vector<hipEvent_t> ready[kMaxSets], done[kMaxSets];
    int* h_mu[kMaxSets] = {};      // mapped pinned: [local index][world] the Mu word of every gathered message
    int* h_mu_dev[kMaxSets] = {};
    long long u_pad = 0, cap = 0, L = 0;   // users per message, union rows per message, words per message (for words_max)
    int words_max = 0;             // mask words per union row the reservation holds
    long long begun = 0, finished = 0, collected = 0;  // steps begun / exchanges issued / exchanges collected
    int nq[kMaxSets] = {};
    int rc[kMaxSets] = {};         // a step that failed on this process before its exchange completed: its collect reports it
};

// One member per LOCAL rank: a single-process communicator (pie_comm_create) holds all ranks of the node, a
// process-per-GPU communicator (pie_comm_create_rank) holds one.
struct pie_comm {
    int world = 0;                 // ranks in the communicator
    int n_local = 0;               // ranks this process drives
    std::vector<int> rank_of;      // local index -> rank
    std::vector<int> device;       // local index -> HIP device
    std::vector<pie_ctx*> ctx;     // local index -> scan context (owned)
    std::vector<ncclComm_t> comm;
    std::vector<hipStream_t> stream;   // the context's stream: results are produced and exchanged in stream order
    std::vector<int*> msg;         // local index -> this rank's messages   [q_max][L]
    std::vector<int*> gath;        // local index -> gathered messages      [world][q_max][L]
    int q_max = 0;
    long long u_pad = 0, cap = 0, L = 0;
    int last_nq = 0;
    long long need = 0;            // row capacity the last exchange called for (the largest list / union any rank reported)
    std::vector<hipStream_t> xstream;  // local index -> exchange stream of the pipelined steps (both kinds: they never mix in flight)
    pie_steps ord, wide;               // pie_comm_step_* / pie_comm_wide_step_*: nothing shared, a reservation of one never moves the other's geometry
    // cross-shard dispatch queues (pie_comm_expired_queue / _archive_queue): buffers of their own, sized by the header exchange
    std::vector<int*> qh_msg, qh_gath;            // local index -> header words [2] / gathered headers [world][2]
    int* h_qhead = nullptr;                       // pinned: [local index][2] headers to send, then [world][2] as gathered
    std::vector<int*> q_msg, q_gath;              // local index -> queue message [QL] / gathered messages [world][QL]
    long long q_msg_words = 0;                    // words allocated per message
    std::vector<int*> q_rows, q_src_rank, q_src_row; // local index -> the merged queue
    long long q_out_cap = 0;
    long long q_total = -1;                       // length of the merged queue (-1: none)
    int q_kind = 0;                               // PIE_COMM_QUEUE_*: which call left it
    // the merged list of pie_comm_prune_before / pie_comm_retention_purge*: on the first local rank's device only
    int *mq_rows = nullptr, *mq_rank = nullptr, *mq_row = nullptr;
    long long mq_cap = 0;
    int* mq_stage = nullptr;                      // lists of shards on other devices, global rows then local rows, back to back
    long long mq_stage_cap = 0;
    void* mq_desc = nullptr;                      // the merge's descriptor on the device
    std::vector<hipEvent_t> q_ev;                 // local index -> completion of a queue phase
    hipEvent_t q_tev[5] = {};                     // timing of the last queue call on the first local rank's stream
    bool q_timed = false;
    double wait_deadline_ms = 20000.0;            // bound of every wait of the queue path and the steps (PIE_WAIT_DEADLINE_MS)
    // token lookups and the expired queue while steps are in flight (pie_comm_token_lookup_begin ..., pie_comm_expired_queue_begin
    // ...): what the communicator has begun on every local shard, and the merged queue on the first local rank's device
    static constexpr int kLookups = 4;            // a shard's own slots (pie_token_lookup_room of an idle shard)
    size_t lk_k[kLookups] = {};                   // keys of the lookups begun and unfinished, a ring from lk_head
    int lk_head = 0, lk_n = 0;
    bool xq_begun = false;
    bool xq_stage_all = false;                    // PIE_COMM_STAGE_ALL=1: every shard's list is brought over, same device or not (tests)
    size_t xq_cap_rows = 0;                       // of the begin
    int *xq_rows = nullptr, *xq_owner = nullptr;  // the merged list: global rows, owning ranks
    size_t xq_room = 0;
    int* xq_stage = nullptr;                      // lists brought over from other devices, back to back
    size_t xq_stage_room = 0;
    void* xq_desc = nullptr;                      // the merge's descriptor (MergeDesc) on the device
    char* xq_h = nullptr;                         // pinned: the descriptor going up, then rows and owners coming back
    hipEvent_t xq_ev = nullptr;
    long long xq_total = -1, xq_have = 0;         // of the last finish: the true total (-1: none), the rows the merged list holds
    std::vector<void*> xq_retired_dev, xq_retired_host; // blocks a begin outgrew: freed at destroy (a free waits for the whole device)
    char err[512] = "";
};

namespace {

int cfail(pie_comm* c, int code, const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    if (c) vsnprintf(c->err, sizeof c->err, fmt, ap);
    else vsnprintf(g_comm_create_error, sizeof g_comm_create_error, fmt, ap);
    va_end(ap);
    return code;
}

#define PIE_CHIP(c, call)                                                                                       \
    do {                                                                                                        \
        hipError_t e_ = (call);                                                                                 \
        if (e_ != hipSuccess)                                                                                   \
            return cfail((c), e_ == hipErrorOutOfMemory ? PIE_E_NOMEM : PIE_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define PIE_CNCCL(c, call)                                                                                      \
    do {                                                                                                        \
        ncclResult_t r_ = (call);                                                                               \
        if (r_ != 0) return cfail((c), PIE_E_HIP, "%s: %s", #call, g_rccl.GetErrorString(r_));                  \
    } while (0)
#define PIE_CCTX(c, k, call)                                                                                    \
    do {                                                                                                        \
        int rc_ = (call);                                                                                       \
        if (rc_ != PIE_OK) return cfail((c), rc_, "rank %d: %s", (c)->rank_of[k], pie_last_error((c)->ctx[k])); \
    } while (0)

void free_buffers(pie_comm* c)
{
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        if (k < (int)c->msg.size() && c->msg[k]) (void)hipFree(c->msg[k]);
        if (k < (int)c->gath.size() && c->gath[k]) (void)hipFree(c->gath[k]);
    }
    c->msg.assign((size_t)c->n_local, nullptr);
    c->gath.assign((size_t)c->n_local, nullptr);
    c->cap = c->L = 0;
}

int ensure_buffers(pie_comm* c, int n_q, long long u_pad, long long cap)
{
    if (c->msg.size() == (size_t)c->n_local && c->msg[0] && n_q <= c->q_max && u_pad == c->u_pad && cap <= c->cap) return PIE_OK;
    free_buffers(c);
    c->q_max = n_q > c->q_max ? n_q : c->q_max;
    c->u_pad = u_pad;
    c->cap = cap;
    c->L = u_pad + 2 + cap;
    const size_t words = (size_t)c->q_max * (size_t)c->L;
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        PIE_CHIP(c, hipMalloc(&c->msg[k], words * 4));
        PIE_CHIP(c, hipMalloc(&c->gath[k], words * 4 * (size_t)c->world));
        PIE_CHIP(c, hipMemset(c->msg[k], 0, words * 4));
    }
    return PIE_OK;
}

pie_comm* new_comm(int world, int n_local)
{
    pie_comm* c = new (std::nothrow) pie_comm();
    if (!c) return nullptr;
    c->world = world;
    c->n_local = n_local;
    c->rank_of.assign((size_t)n_local, 0);
    c->device.assign((size_t)n_local, 0);
    c->ctx.assign((size_t)n_local, nullptr);
    c->comm.assign((size_t)n_local, nullptr);
    c->stream.assign((size_t)n_local, nullptr);
    c->msg.assign((size_t)n_local, nullptr);
    c->gath.assign((size_t)n_local, nullptr);
    for (auto* v : {&c->qh_msg, &c->qh_gath, &c->q_msg, &c->q_gath, &c->q_rows, &c->q_src_rank, &c->q_src_row}) v->assign((size_t)n_local, nullptr);
    c->q_ev.assign((size_t)n_local, nullptr);
    if (const char* v = getenv("PIE_WAIT_DEADLINE_MS")) { const double d = atof(v); if (d > 0) c->wait_deadline_ms = d; }
    if (const char* v = getenv("PIE_COMM_STAGE_ALL")) c->xq_stage_all = atoi(v) != 0;
    return c;
}

void free_queue_buffers(pie_comm* c);

void free_step_buffers(pie_comm* c, pie_steps& st);

void inflight_close(pie_comm* c);

// the synchronous gather, the queues and the mutations stay out of the way of pipelined steps of either kind
int steps_idle(pie_comm* c)
{
    if (c->ord.begun != c->ord.collected) return cfail(c, PIE_E_STATE, "pipelined steps are in flight (pie_comm_step_*): collect them first");
    if (c->wide.begun != c->wide.collected) return cfail(c, PIE_E_STATE, "wide steps are in flight (pie_comm_wide_step_*): collect them first");
    return PIE_OK;
}

int local_index(const pie_comm* c, int rank)
{
    for (int k = 0; k < c->n_local; ++k)
        if (c->rank_of[k] == rank) return k;
    return -1;
}

} // namespace

extern "C" {

const char* pie_comm_last_error(const pie_comm* c) { return c ? c->err : g_comm_create_error; }

int pie_comm_create(const int32_t* device_ids, int32_t n, pie_comm** comm_out)
{
    if (!comm_out) return cfail(nullptr, PIE_E_INVAL, "comm_out is NULL");
    *comm_out = nullptr;
    if (!device_ids || n < 1 || n > 64) return cfail(nullptr, PIE_E_INVAL, "1..64 devices expected (got %d)", n);
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            if (device_ids[a] == device_ids[b] && !getenv("PIE_RCCL_LIB")) // (the test stand-in runs several shards on one GPU)
                return cfail(nullptr, PIE_E_INVAL, "device %d listed twice: one shard per GPU", device_ids[a]);
    char why[200];
    if (!load_rccl(why, sizeof why)) return cfail(nullptr, PIE_E_NODEVICE, "%s", why);
    pie_comm* c = new_comm(n, n);
    if (!c) return cfail(nullptr, PIE_E_NOMEM, "out of host memory");
    for (int k = 0; k < n; ++k) {
        c->rank_of[k] = k;
        c->device[k] = device_ids[k];
        int rc = pie_ctx_create(device_ids[k], &c->ctx[k]);
        if (rc != PIE_OK) {
            cfail(nullptr, rc, "shard %d on device %d: %s", k, device_ids[k], pie_last_error(nullptr));
            pie_comm_destroy(c);
            return rc;
        }
        void* s = nullptr;
        (void)pie_ctx_aux_stream(c->ctx[k], &s);
        c->stream[k] = (hipStream_t)s;
    }
    std::vector<int> devs(device_ids, device_ids + n);
    ncclResult_t r = g_rccl.CommInitAll(c->comm.data(), n, devs.data());
    if (r != 0) {
        cfail(nullptr, PIE_E_HIP, "ncclCommInitAll: %s", g_rccl.GetErrorString(r));
        for (auto& cm : c->comm) cm = nullptr;
        pie_comm_destroy(c);
        return PIE_E_HIP;
    }
    *comm_out = c;
    return PIE_OK;
}

int pie_comm_unique_id(void* id_out_128)
{
    if (!id_out_128) return cfail(nullptr, PIE_E_INVAL, "id_out is NULL");
    char why[200];
    if (!load_rccl(why, sizeof why)) return cfail(nullptr, PIE_E_NODEVICE, "%s", why);
    ncclUniqueId id;
    ncclResult_t r = g_rccl.GetUniqueId(&id);
    if (r != 0) return cfail(nullptr, PIE_E_HIP, "ncclGetUniqueId: %s", g_rccl.GetErrorString(r));
    memcpy(id_out_128, id.internal, sizeof id.internal);
    return PIE_OK;
}

int pie_comm_create_rank(const void* id_128, int32_t rank, int32_t world, int32_t device_id, pie_comm** comm_out)
{
    if (!comm_out) return cfail(nullptr, PIE_E_INVAL, "comm_out is NULL");
    *comm_out = nullptr;
    if (!id_128 || world < 1 || world > 64 || rank < 0 || rank >= world) return cfail(nullptr, PIE_E_INVAL, "bad id / rank %d of %d (1..64 ranks)", rank, world);
    char why[200];
    if (!load_rccl(why, sizeof why)) return cfail(nullptr, PIE_E_NODEVICE, "%s", why);
    pie_comm* c = new_comm(world, 1);
    if (!c) return cfail(nullptr, PIE_E_NOMEM, "out of host memory");
    c->rank_of[0] = rank;
    c->device[0] = device_id;
    int rc = pie_ctx_create(device_id, &c->ctx[0]);
    if (rc != PIE_OK) {
        cfail(nullptr, rc, "rank %d on device %d: %s", rank, device_id, pie_last_error(nullptr));
        pie_comm_destroy(c);
        return rc;
    }
    void* s = nullptr;
    (void)pie_ctx_aux_stream(c->ctx[0], &s);
    c->stream[0] = (hipStream_t)s;
    ncclUniqueId id;
    memcpy(id.internal, id_128, sizeof id.internal);
    if (hipSetDevice(device_id) != hipSuccess) {
        cfail(nullptr, PIE_E_NODEVICE, "hipSetDevice(%d) failed", device_id);
        pie_comm_destroy(c);
        return PIE_E_NODEVICE;
    }
    ncclResult_t r = g_rccl.CommInitRank(&c->comm[0], world, id, rank);
    if (r != 0) {
        cfail(nullptr, PIE_E_HIP, "ncclCommInitRank: %s", g_rccl.GetErrorString(r));
        c->comm[0] = nullptr;
        pie_comm_destroy(c);
        return PIE_E_HIP;
    }
    *comm_out = c;
    return PIE_OK;
}

int pie_comm_destroy(pie_comm* c)
{
    if (!c) return PIE_OK;
    inflight_close(c); // lookups and a queue begun and not finished land first (bounded waits)
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        if (c->stream[k]) (void)hipStreamSynchronize(c->stream[k]);
    }
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        if (k < (int)c->xstream.size() && c->xstream[k]) (void)hipStreamSynchronize(c->xstream[k]);
    }
    free_buffers(c);
    free_step_buffers(c, c->ord);
    free_step_buffers(c, c->wide);
    free_queue_buffers(c);
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        if (k < (int)c->xstream.size() && c->xstream[k]) (void)hipStreamDestroy(c->xstream[k]);
    }
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        if (c->comm[k] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm[k]);
        if (c->ctx[k]) (void)pie_ctx_destroy(c->ctx[k]);
    }
    delete c;
    return PIE_OK;
}

int32_t pie_comm_world(const pie_comm* c) { return c ? c->world : 0; }
int32_t pie_comm_local_ranks(const pie_comm* c) { return c ? c->n_local : 0; }

pie_ctx* pie_comm_ctx(pie_comm* c, int32_t rank)
{
    if (!c) return nullptr;
    const int k = local_index(c, rank);
    return k >= 0 ? c->ctx[k] : nullptr;
}

int pie_comm_gen_synthetic_sharded(pie_comm* c, uint64_t seed, int64_t n_total, int32_t n_users, int32_t n_disc, uint32_t flags)
{
    if (!c) return PIE_E_INVAL;
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CCTX(c, k, pie_gen_synthetic(c->ctx[k], seed, n_total, 0, n_total, n_users, n_disc, flags));
        size_t rows = 0;
        int32_t users = 0;
        PIE_CCTX(c, k, pie_shard_table(c->ctx[k], c->rank_of[k], c->world, &rows, &users));
    }
    return PIE_OK;
}

namespace {

// the Mu word of every gathered message (world of them, rank_stride words apart) into mapped host memory: no copy node behind
// the exchange (a 2-D copy call cost more host time than the whole step's launches)
__global__ __launch_bounds__(64) void k_pick_words(const int* __restrict__ gath, long long rank_stride, long long word, int world, int* __restrict__ out)
{
    const int r = (int)threadIdx.x;
    if (r < world) __hip_atomic_store(&out[r], gath[(long long)r * rank_stride + word], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// the direct exchange of one fixed-length message per rank: inside one group every local rank posts one send and one
// receive per peer (each message crosses its own xGMI link once); its own message is a local copy on the same stream
int exchange(pie_comm* c, const std::vector<int*>& msg, const std::vector<int*>& gath, size_t count, size_t rank_stride, const std::vector<hipStream_t>& streams)
{
    if (c->world > 1) {
        PIE_CNCCL(c, g_rccl.GroupStart());
        for (int k = 0; k < c->n_local; ++k) {
            const int me = c->rank_of[k];
            for (int p = 0; p < c->world; ++p) {
                if (p == me) continue;
                ncclResult_t r1 = g_rccl.Send(msg[k], count, kNcclInt32, p, c->comm[k], streams[k]);
                ncclResult_t r2 = g_rccl.Recv(gath[k] + (size_t)p * rank_stride, count, kNcclInt32, p, c->comm[k], streams[k]);
                if (r1 != 0 || r2 != 0) {
                    (void)g_rccl.GroupEnd();
                    return cfail(c, PIE_E_HIP, "ncclSend/ncclRecv: %s", g_rccl.GetErrorString(r1 != 0 ? r1 : r2));
                }
            }
        }
        PIE_CNCCL(c, g_rccl.GroupEnd());
    }
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        PIE_CHIP(c, hipMemcpyAsync(gath[k] + (size_t)c->rank_of[k] * rank_stride, msg[k], count * 4, hipMemcpyDeviceToDevice, streams[k]));
    }
    return PIE_OK;
}

// u_pad every rank uses: the largest shard's user count (single process), or the value the ranks agreed on
int resolve_u_pad(pie_comm* c, int32_t u_pad_in, long long* u_pad_out)
{
    long long u_pad = u_pad_in;
    for (int k = 0; k < c->n_local; ++k) {
        pie_stats st;
        st.struct_size = sizeof(pie_stats);
        PIE_CCTX(c, k, pie_stats_get(c->ctx[k], &st));
        if (u_pad_in <= 0 && (long long)st.users > u_pad) u_pad = (long long)st.users;
        if ((long long)st.users > u_pad) return cfail(c, PIE_E_INVAL, "rank %d holds %llu users, above u_pad %lld", c->rank_of[k], (unsigned long long)st.users, u_pad);
    }
    if (c->n_local != c->world && u_pad_in <= 0) return cfail(c, PIE_E_INVAL, "process-per-GPU communicator: pass the agreed u_pad");
    *u_pad_out = u_pad;
    return PIE_OK;
}

} // namespace

// One synchronous step, per-query lists.  The exchange ALWAYS runs once every local shard has finished its batch — the
// messages have the fixed length L and simply truncate a list that outgrew the capacity (M stays in the header) — and the
// capacity check is made on the GATHERED headers, which every rank sees alike: all ranks return PIE_E_CAPACITY together
// (pie_comm_needed_cap says what to reserve), none is left waiting inside ncclSend / ncclRecv for a peer that bailed out
// (ADVICE r02).  An error on one local shard still finishes the batches begun on the others before it is reported.
int pie_comm_scan_batch_gather(pie_comm* c, const pie_query* queries, int32_t n_q, int32_t u_pad_in, size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    if (!queries || n_q < 1 || n_q > PIE_BATCH_MAX) return cfail(c, PIE_E_INVAL, "a batch holds 1..%d queries (got %d)", PIE_BATCH_MAX, n_q);
    if (steps_idle(c)) return PIE_E_STATE;
    long long u_pad = 0;
    int rc = resolve_u_pad(c, u_pad_in, &u_pad);
    if (rc) return rc;
    std::vector<size_t> m((size_t)c->n_local * (size_t)n_q, 0);
    long long cap = c->cap > 0 ? c->cap : 1024;
    std::vector<int> heads((size_t)c->world * (size_t)n_q);
    for (int attempt = 0; attempt < 3; ++attempt) {
        rc = ensure_buffers(c, n_q, u_pad, cap);
        if (rc) return rc;
        // 1. every shard scans its batch and leaves its n_q messages back to back in msg[k]
        int begun = 0, first_rc = PIE_OK;
        for (int k = 0; k < c->n_local && first_rc == PIE_OK; ++k) {
            first_rc = pie_scan_batch_begin_packed(c->ctx[k], queries, n_q, c->msg[k], (size_t)c->L, (size_t)c->u_pad, (size_t)c->cap, nullptr, 0);
            if (first_rc == PIE_OK) ++begun;
            else cfail(c, first_rc, "rank %d: %s", c->rank_of[k], pie_last_error(c->ctx[k]));
        }
        for (int k = 0; k < begun; ++k) { // every batch that was begun is finished, whatever happened elsewhere
            int ready = 0;
            const int r2 = pie_scan_batch_finish_packed(c->ctx[k], &m[(size_t)k * n_q], &ready);
            if (r2 != PIE_OK && first_rc == PIE_OK) {
                first_rc = r2;
                cfail(c, r2, "rank %d: %s", c->rank_of[k], pie_last_error(c->ctx[k]));
            }
        }
        if (first_rc != PIE_OK) return first_rc; // a local failure (bad argument, HIP error): no rank of THIS process entered the exchange
        // 2. the exchange: always
        const size_t count = (size_t)n_q * (size_t)c->L;
        rc = exchange(c, c->msg, c->gath, count, (size_t)c->q_max * (size_t)c->L, c->stream);
        if (rc) return rc;
        // 3. every rank's M words, as gathered at the first local rank: the same numbers on every rank of the communicator
        PIE_CHIP(c, hipSetDevice(c->device[0]));
        for (int p = 0; p < c->world; ++p)
            PIE_CHIP(c, hipMemcpy2DAsync(&heads[(size_t)p * n_q], 4, c->gath[0] + (size_t)p * (size_t)c->q_max * (size_t)c->L + (size_t)c->u_pad + 1,
                                         (size_t)c->L * 4, 4, (size_t)n_q, hipMemcpyDeviceToHost, c->stream[0]));
        for (int k = 0; k < c->n_local; ++k) {
            PIE_CHIP(c, hipSetDevice(c->device[k]));
            PIE_CHIP(c, hipStreamSynchronize(c->stream[k]));
        }
        long long need = 0;
        for (int v : heads) need = v > need ? v : need;
        c->need = need;
        c->last_nq = n_q;
        if (need <= c->cap) break;
        if (c->n_local != c->world || attempt == 2)
            return cfail(c, PIE_E_CAPACITY, "a row list of %lld rows exceeds the reserved capacity %lld on some rank: every rank calls pie_comm_reserve(pie_comm_needed_cap) and repeats the step", need, c->cap);
        cap = need + need / 16 + 64; // a single process owns every rank: grow and run the step again
    }
    if (m_out) memcpy(m_out, m.data(), m.size() * sizeof(size_t));
    return PIE_OK;
}

size_t pie_comm_needed_cap(const pie_comm* c) { return c ? (size_t)(c->need + c->need / 16 + 64) : 0; }

int pie_comm_reserve(pie_comm* c, int32_t n_q, int32_t u_pad, size_t idx_cap)
{
    if (!c) return PIE_E_INVAL;
    if (n_q < 1 || n_q > PIE_BATCH_MAX || u_pad < 1) return cfail(c, PIE_E_INVAL, "bad reservation");
    return ensure_buffers(c, n_q, u_pad, (long long)idx_cap);
}

int pie_comm_gathered_device_ptr(pie_comm* c, int32_t at_rank, void** base_out, size_t* rank_stride_words, size_t* query_stride_words,
                                 size_t* u_pad_out)
{
    if (!c) return PIE_E_INVAL;
    const int k = local_index(c, at_rank);
    if (k < 0 || !c->gath[k]) return cfail(c, PIE_E_STATE, "rank %d is not local to this communicator or nothing was gathered yet", at_rank);
    if (base_out) *base_out = c->gath[k];
    if (rank_stride_words) *rank_stride_words = (size_t)c->q_max * (size_t)c->L;
    if (query_stride_words) *query_stride_words = (size_t)c->L;
    if (u_pad_out) *u_pad_out = (size_t)c->u_pad;
    return PIE_OK;
}

int pie_comm_read_gathered(pie_comm* c, int32_t at_rank, int32_t src_rank, int32_t qi, int32_t* offsets_out, int32_t* idx_out, size_t idx_cap,
                           size_t* m_out)
{
    if (!c) return PIE_E_INVAL;
    const int k = local_index(c, at_rank);
    if (k < 0 || !c->gath[k]) return cfail(c, PIE_E_STATE, "rank %d is not local to this communicator or nothing was gathered yet", at_rank);
    if (src_rank < 0 || src_rank >= c->world || qi < 0 || qi >= c->last_nq) return cfail(c, PIE_E_INVAL, "source rank / query outside the last exchange");
    PIE_CHIP(c, hipSetDevice(c->device[k]));
    const int* msg = c->gath[k] + ((size_t)src_rank * (size_t)c->q_max + (size_t)qi) * (size_t)c->L;
    int m32 = 0;
    PIE_CHIP(c, hipMemcpy(&m32, msg + c->u_pad + 1, 4, hipMemcpyDeviceToHost));
    if (m_out) *m_out = (size_t)m32;
    if (offsets_out) PIE_CHIP(c, hipMemcpy(offsets_out, msg, ((size_t)c->u_pad + 1) * 4, hipMemcpyDeviceToHost));
    if (idx_out) {
        if ((size_t)m32 > idx_cap) return cfail(c, PIE_E_CAPACITY, "idx_cap %zu < %d rows", idx_cap, m32);
        if (m32 > 0) PIE_CHIP(c, hipMemcpy(idx_out, msg + c->u_pad + 2, (size_t)m32 * 4, hipMemcpyDeviceToHost));
    }
    return PIE_OK;
}

} // extern "C"

// ---- cross-shard dispatch queues (pie_comm_expired_queue / pie_comm_archive_queue) ---------------------------------------
// Each shard's queue is packed on its device into one message of global rows (pie_queue_pack_device:
// [n_rows | n_groups | global rows (cap_rows) | local rows (cap_rows) | group offsets (cap_groups + 1)]), exchanged with the direct
// pattern and merged on every rank's device.  Global rows are unique across ranks and every shard's list is ascending in them
// (the shard maps are ascending), so an element's place in the merged order is its place in its own list plus, for every other
// rank, how many of that rank's keys are smaller (a lower bound): no sort, no atomics, the same result on every rank.
namespace {

constexpr int kMergeMaxLists = 64; // lists one merge takes: the ranks of a communicator (pie_comm_create: 1..64), one lane each in the archive merge

// what the co-rank merge reads: `count` ascending lists of GLOBAL rows (a gathered message's rows, a shard's own queue buffer, or
// its copy on the merging device), every list's kept length and rank, the lists' running lengths (pre[count] elements in all)
struct MergeDesc {
    const int* rows[kMergeMaxLists];
    const int* local[kMergeMaxLists];   // SRC_ROW only: every list's local rows, element for element
    long long pre[kMergeMaxLists + 1];
    int n[kMergeMaxLists];
    int rank[kMergeMaxLists];
    int count, pad;
};

// One lane per element, placed by co-rank: its index in its own list plus, for every other list, how many of that list's rows
// are smaller (a lower bound; global rows are unique across shards).  No atomics, no wave waits for another.  A position at or
// past out_cap is not written: the first out_cap merged rows only ever come from the first out_cap rows of each list.
// SRC_ROW: the element's local row on its shard goes with it.  `s` sits in LDS (every lane indexes it by its own list).
template <bool SRC_ROW>
__device__ __forceinline__ void merge_by_corank(const MergeDesc& s, long long out_cap, int* __restrict__ out_rows, int* __restrict__ out_rank,
                                                int* __restrict__ out_row)
{
    const int count = min(max(s.count, 0), kMergeMaxLists);
    const long long total = s.pre[count];
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        int r = 0;
        while (r + 1 < count && s.pre[r + 1] <= e) ++r;
        const long long i = e - s.pre[r];
        if (i >= s.n[r]) continue; // (a descriptor that does not add up reads nothing)
        const int v = s.rows[r][i];
        long long pos = i;
        for (int p = 0; p < count; ++p) {
            if (p == r) continue;
            const int* other = s.rows[p];
            int lo = 0, hi = s.n[p];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (other[mid] < v) lo = mid + 1;
                else hi = mid;
            }
            pos += lo;
        }
        if (pos < out_cap) {
            out_rows[pos] = v;
            out_rank[pos] = s.rank[r];
            if constexpr (SRC_ROW) out_row[pos] = s.local[r][i];
        }
    }
}

// rows / groups of every gathered message, clamped to the message's capacities (the kernels never read past a message)
__device__ void queue_heads(const int* __restrict__ gath, long long ql, long long cap_rows, long long cap_groups, int world, int* s_n, int* s_g,
                            long long* s_pre, bool by_groups)
{
    if (threadIdx.x == 0) {
        long long acc = 0;
        for (int r = 0; r < world; ++r) {
            const int* m = gath + (long long)r * ql;
            const long long n = min(max((long long)m[0], 0LL), cap_rows);
            const long long g = n > 0 ? min(max((long long)m[1], 0LL), cap_groups) : 0;
            s_n[r] = (int)n;
            s_g[r] = (int)g;
            s_pre[r] = acc;
            acc += by_groups ? g : n;
        }
        s_pre[world] = acc;
    }
    __syncthreads();
}

// expired queue: the co-rank merge of the gathered messages; list p is rank p's, its length clamped as queue_heads clamps it
__global__ __launch_bounds__(256) void k_merge_expired(const int* __restrict__ gath, long long ql, long long cap_rows, int world, long long out_cap,
                                                       int* __restrict__ out_rows, int* __restrict__ out_rank, int* __restrict__ out_row)
{
    __shared__ MergeDesc s;
    if (threadIdx.x == 0) {
        world = min(world, kMergeMaxLists);
        long long acc = 0;
        for (int p = 0; p < world; ++p) {
            const int* m = gath + (long long)p * ql;
            s.rows[p] = m + 2;
            s.local[p] = s.rows[p] + cap_rows;
            s.n[p] = (int)min(max((long long)m[0], 0LL), cap_rows);
            s.rank[p] = p;
            s.pre[p] = acc;
            acc += s.n[p];
        }
        s.pre[world] = acc;
        s.count = world;
    }
    __syncthreads();
    merge_by_corank<true>(s, out_cap, out_rows, out_rank, out_row);
}

// the lists of local shards, named by a descriptor in device memory: <false> the in-flight expired queue (rows and owners), <true>
// the lists of a prune / retention purge (the local row too)
template <bool SRC_ROW>
__global__ __launch_bounds__(256) void k_merge_shard_queues(const MergeDesc* __restrict__ desc, long long out_cap, int* __restrict__ out_rows,
                                                            int* __restrict__ out_rank, int* __restrict__ out_row)
{
    __shared__ MergeDesc s;
    for (int w = (int)threadIdx.x; w < (int)(sizeof(MergeDesc) / 4); w += (int)blockDim.x)
        reinterpret_cast<int*>(&s)[w] = reinterpret_cast<const int*>(desc)[w];
    __syncthreads();
    merge_by_corank<SRC_ROW>(s, out_cap, out_rows, out_rank, out_row);
}

// archive queue: one wave per group; lane p finds how many of rank p's groups have a smaller key (the global row of a group's first
// queued row) and contributes the rows they hold (their group offset); the wave then copies the group's rows to its place
__global__ __launch_bounds__(256) void k_merge_archive(const int* __restrict__ gath, long long ql, long long cap_rows, long long cap_groups, int world,
                                                       long long out_cap, int* __restrict__ out_rows, int* __restrict__ out_rank, int* __restrict__ out_row)
{
    __shared__ int s_n[kMergeMaxLists], s_g[kMergeMaxLists];
    __shared__ long long s_pre[kMergeMaxLists + 1];
    queue_heads(gath, ql, cap_rows, cap_groups, world, s_n, s_g, s_pre, true);
    const long long groups = s_pre[world];
    const int lane = (int)(threadIdx.x & 63);
    const long long waves = ((long long)gridDim.x * blockDim.x) >> 6;
    auto goff_at = [&](const int* goff, int j, int n) { return min(max(goff[j], 0), n); };
    for (long long f = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; f < groups; f += waves) { // wave-uniform
        int r = 0;
        while (s_pre[r + 1] <= f) ++r;
        const int j = (int)(f - s_pre[r]);
        const int* grow = gath + (long long)r * ql + 2;
        const int* lrow = grow + cap_rows;
        const int* goff = lrow + cap_rows;
        const int b = goff_at(goff, j, s_n[r]);
        const int e = max(goff_at(goff, j + 1, s_n[r]), b);
        const int key = b < s_n[r] ? grow[b] : 0x7FFFFFFF;
        int before = 0;
        if (lane < world && lane != r) {
            const int* g_p = gath + (long long)lane * ql + 2;
            const int* goff_p = g_p + 2 * cap_rows;
            const int n_p = s_n[lane];
            int lo = 0, hi = s_g[lane];
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (g_p[min(goff_at(goff_p, mid, n_p), n_p - 1)] < key) lo = mid + 1;
                else hi = mid;
            }
            before = goff_at(goff_p, lo, n_p);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
        const long long dst = (long long)b + before;
        for (int t = lane; t < e - b; t += 64) {
            const long long pos = dst + t;
            if (pos < out_cap) {
                out_rows[pos] = grow[b + t];
                out_rank[pos] = r;
                out_row[pos] = lrow[b + t];
            }
        }
    }
}

// a bounded wait for an event (PIE_WAIT_DEADLINE_MS): a peer that never sends must not hang the caller
int wait_event(pie_comm* c, int k, hipEvent_t ev, const char* what)
{
    PIE_CHIP(c, hipSetDevice(c->device[k]));
    hipError_t e = hipSuccess; // the one query per spin is both the thing waited for and the probe
    const pie::WaitResult w = pie::bounded_wait([&] { return (e = hipEventQuery(ev)) == hipSuccess; },
                                                [&] { return e == hipErrorNotReady ? pie::kProbeNotReady : (int)e; }, c->wait_deadline_ms,
                                                pie::kNoGraceLimit, pie::kPaceCommEvent);
    if (w.end == pie::WaitEnd::Ready) return PIE_OK;
    if (w.end == pie::WaitEnd::Failed) return cfail(c, PIE_E_HIP, "rank %d, %s: %s", c->rank_of[k], what, hipGetErrorString((hipError_t)w.err));
    return cfail(c, PIE_E_HIP, "rank %d: %s not complete within %.0f ms (PIE_WAIT_DEADLINE_MS): a peer never sent?", c->rank_of[k], what, w.waited_ms);
}

void free_queue_buffers(pie_comm* c)
{
    for (int k = 0; k < c->n_local; ++k) {
        (void)hipSetDevice(c->device[k]);
        for (auto* v : {&c->qh_msg, &c->qh_gath, &c->q_msg, &c->q_gath, &c->q_rows, &c->q_src_rank, &c->q_src_row})
            if (k < (int)v->size() && (*v)[k]) { (void)hipFree((*v)[k]); (*v)[k] = nullptr; }
        if (k < (int)c->q_ev.size() && c->q_ev[k]) { (void)hipEventDestroy(c->q_ev[k]); c->q_ev[k] = nullptr; }
    }
    if (c->n_local > 0) (void)hipSetDevice(c->device[0]);
    for (hipEvent_t& e : c->q_tev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (c->h_qhead) (void)hipHostFree(c->h_qhead);
    c->h_qhead = nullptr;
    c->q_msg_words = c->q_out_cap = 0;
    c->q_total = -1;
    c->q_kind = 0;
    for (void* p : {(void*)c->mq_rows, (void*)c->mq_rank, (void*)c->mq_row, (void*)c->mq_stage, c->mq_desc})
        if (p) (void)hipFree(p);
    c->mq_rows = c->mq_rank = c->mq_row = c->mq_stage = nullptr;
    c->mq_desc = nullptr;
    c->mq_cap = c->mq_stage_cap = 0;
}

// header buffers and events: once per communicator
int ensure_queue_heads(pie_comm* c)
{
    if (c->h_qhead) return PIE_OK;
    PIE_CHIP(c, hipHostMalloc(&c->h_qhead, (size_t)c->n_local * (size_t)(c->world + 1) * 8, hipHostMallocDefault));
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        PIE_CHIP(c, hipMalloc(&c->qh_msg[k], 8));
        PIE_CHIP(c, hipMalloc(&c->qh_gath[k], (size_t)c->world * 8));
        PIE_CHIP(c, hipEventCreateWithFlags(&c->q_ev[k], hipEventDisableTiming));
    }
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    for (hipEvent_t& e : c->q_tev) PIE_CHIP(c, hipEventCreate(&e));
    return PIE_OK;
}

// message and merged-queue buffers, grown to what the gathered headers call for (the message length is the same on every rank)
int ensure_queue_msgs(pie_comm* c, long long words, long long total)
{
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        if (words > c->q_msg_words) {
            if (c->q_msg[k]) { PIE_CHIP(c, hipFree(c->q_msg[k])); c->q_msg[k] = nullptr; }
            if (c->q_gath[k]) { PIE_CHIP(c, hipFree(c->q_gath[k])); c->q_gath[k] = nullptr; }
        }
        if (total > c->q_out_cap)
            for (auto* v : {&c->q_rows, &c->q_src_rank, &c->q_src_row})
                if ((*v)[k]) { PIE_CHIP(c, hipFree((*v)[k])); (*v)[k] = nullptr; }
    }
    const long long w = words > c->q_msg_words ? words + words / 16 + 64 : c->q_msg_words;
    const long long o = total > c->q_out_cap ? total + total / 16 + 64 : c->q_out_cap;
    c->q_msg_words = 0;
    c->q_out_cap = 0;
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        if (!c->q_msg[k]) PIE_CHIP(c, hipMalloc(&c->q_msg[k], (size_t)w * 4));
        if (!c->q_gath[k]) PIE_CHIP(c, hipMalloc(&c->q_gath[k], (size_t)w * 4 * (size_t)c->world));
        for (auto* v : {&c->q_rows, &c->q_src_rank, &c->q_src_row})
            if (!(*v)[k]) PIE_CHIP(c, hipMalloc(&(*v)[k], (size_t)o * 4));
    }
    c->q_msg_words = w;
    c->q_out_cap = o;
    return PIE_OK;
}

// kind 1: expired (a = prev_now, b = now), 2: archive (a = now, b = window_ms)
int comm_queue(pie_comm* c, int kind, int64_t a, int64_t b, int32_t* queue_out, size_t cap, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    if (q_out) *q_out = 0;
    if (c->world > kMergeMaxLists) return cfail(c, PIE_E_INVAL, "the queue merge takes at most %d ranks (world %d)", kMergeMaxLists, c->world);
    if (steps_idle(c)) return PIE_E_STATE;
    c->q_total = -1;
    c->q_kind = 0;
    c->q_timed = false;
    int rc = ensure_queue_heads(c);
    if (rc) return rc;
    int* h_send = c->h_qhead;                        // [n_local][2]
    int* h_recv = c->h_qhead + 2 * c->n_local;       // [n_local][world][2]
    // 1. every local shard's queue stays on its device; its header is {rows, groups}, or {-1, status} when the step failed
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    PIE_CHIP(c, hipEventRecord(c->q_tev[0], c->stream[0]));
    std::vector<int> local_rc((size_t)c->n_local, PIE_OK);
    std::vector<std::string> local_err((size_t)c->n_local);
    for (int k = 0; k < c->n_local; ++k) {
        size_t rows = 0, groups = 0;
        int r = kind == 1 ? pie_expired_queue(c->ctx[k], a, b, nullptr, 0, &rows) : pie_archive_queue(c->ctx[k], a, b, nullptr, 0, &rows);
        if (r == PIE_OK) r = pie_queue_info(c->ctx[k], nullptr, &rows, &groups);
        if (r != PIE_OK) local_err[k] = pie_last_error(c->ctx[k]);
        local_rc[k] = r;
        h_send[2 * k] = r == PIE_OK ? (int)rows : -1;
        h_send[2 * k + 1] = r == PIE_OK ? (int)groups : r;
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        PIE_CHIP(c, hipMemcpyAsync(c->qh_msg[k], h_send + 2 * k, 8, hipMemcpyHostToDevice, c->stream[k]));
    }
    // 2. the header exchange: the same path in a single-process and a process-per-GPU communicator
    rc = exchange(c, c->qh_msg, c->qh_gath, 2, 2, c->stream);
    if (rc) return rc;
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        PIE_CHIP(c, hipMemcpyAsync(h_recv + (size_t)k * 2 * c->world, c->qh_gath[k], (size_t)c->world * 8, hipMemcpyDeviceToHost, c->stream[k]));
        PIE_CHIP(c, hipEventRecord(c->q_ev[k], c->stream[k]));
    }
    for (int k = 0; k < c->n_local; ++k) {
        rc = wait_event(c, k, c->q_ev[k], "queue header exchange");
        if (rc) return rc;
    }
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    PIE_CHIP(c, hipEventRecord(c->q_tev[1], c->stream[0]));
    const int* hd = h_recv; // every rank holds the same world headers
    for (int p = 0; p < c->world; ++p) {
        if (hd[2 * p] >= 0) continue;
        int status = hd[2 * p + 1];
        if (status >= 0 || status < PIE_E_STATE) status = PIE_E_STATE;
        const int k = local_index(c, p);
        if (k >= 0 && !local_err[k].empty()) return cfail(c, status, "rank %d: %s", p, local_err[k].c_str());
        return cfail(c, status, "rank %d could not produce its queue (status %d): no rank merged", p, status);
    }
    long long cap_rows = 0, cap_groups = 0, total = 0;
    for (int p = 0; p < c->world; ++p) {
        cap_rows = hd[2 * p] > cap_rows ? hd[2 * p] : cap_rows;
        cap_groups = hd[2 * p + 1] > cap_groups ? hd[2 * p + 1] : cap_groups;
        total += hd[2 * p];
    }
    if (total >= 0x7FFFFFFFLL) return cfail(c, PIE_E_INVAL, "a merged queue of %lld rows does not fit int32", total);
    const long long ql = 2 + 2 * cap_rows + cap_groups + 1;
    rc = ensure_queue_msgs(c, ql, total);
    if (rc) return rc;
    // 3. pack (global rows through the shard map, on the device) and exchange the messages
    for (int k = 0; k < c->n_local; ++k) PIE_CCTX(c, k, pie_queue_pack_device(c->ctx[k], c->q_msg[k], (size_t)cap_rows, (size_t)cap_groups));
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    PIE_CHIP(c, hipEventRecord(c->q_tev[2], c->stream[0]));
    rc = exchange(c, c->q_msg, c->q_gath, (size_t)ql, (size_t)ql, c->stream);
    if (rc) return rc;
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    PIE_CHIP(c, hipEventRecord(c->q_tev[3], c->stream[0]));
    // 4. the merge, on every local rank's device
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        if (kind == 1) {
            const long long blocks = total > 0 ? (total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048 : 1;
            hipLaunchKernelGGL(k_merge_expired, dim3((unsigned)blocks), dim3(256), 0, c->stream[k], c->q_gath[k], ql, cap_rows, c->world, total,
                               c->q_rows[k], c->q_src_rank[k], c->q_src_row[k]);
        } else {
            long long groups = 0;
            for (int p = 0; p < c->world; ++p) groups += hd[2 * p + 1];
            const long long blocks = groups > 0 ? (groups + 3) / 4 < 2048 ? (groups + 3) / 4 : 2048 : 1;
            hipLaunchKernelGGL(k_merge_archive, dim3((unsigned)blocks), dim3(256), 0, c->stream[k], c->q_gath[k], ql, cap_rows, cap_groups, c->world,
                               total, c->q_rows[k], c->q_src_rank[k], c->q_src_row[k]);
        }
        PIE_CHIP(c, hipGetLastError());
        if (k == 0) PIE_CHIP(c, hipEventRecord(c->q_tev[4], c->stream[0]));
        PIE_CHIP(c, hipEventRecord(c->q_ev[k], c->stream[k]));
    }
    for (int k = 0; k < c->n_local; ++k) {
        rc = wait_event(c, k, c->q_ev[k], "queue merge");
        if (rc) return rc;
    }
    c->q_total = total;
    c->q_kind = kind == 1 ? PIE_COMM_QUEUE_EXPIRED : PIE_COMM_QUEUE_ARCHIVE;
    c->q_timed = true;
    if (q_out) *q_out = (size_t)total;
    if (queue_out && (size_t)total > cap) return cfail(c, PIE_E_CAPACITY, "queue cap %zu < %lld", cap, total);
    if (queue_out && total) {
        PIE_CHIP(c, hipSetDevice(c->device[0]));
        PIE_CHIP(c, hipMemcpy(queue_out, c->q_rows[0], (size_t)total * 4, hipMemcpyDeviceToHost));
    }
    return PIE_OK;
}

} // namespace

extern "C" {

int pie_comm_expired_queue(pie_comm* c, int64_t prev_now, int64_t now, int32_t* queue_out, size_t cap, size_t* q_out)
{
    return comm_queue(c, 1, prev_now, now, queue_out, cap, q_out);
}

int pie_comm_archive_queue(pie_comm* c, int64_t now, int64_t window_ms, int32_t* queue_out, size_t cap, size_t* q_out)
{
    return comm_queue(c, 2, now, window_ms, queue_out, cap, q_out);
}

int pie_comm_queue_device_ptrs(pie_comm* c, int32_t at_rank, void** rows_dev, void** src_rank_dev, void** src_row_dev, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    const int k = local_index(c, at_rank);
    if (k < 0) return cfail(c, PIE_E_INVAL, "rank %d is not local to this communicator", at_rank);
    if (c->q_total < 0) return cfail(c, PIE_E_STATE, "no merged queue: pie_comm_expired_queue / pie_comm_archive_queue first");
    if (c->q_kind == PIE_COMM_QUEUE_MAINT) { // merged on the first local rank's device only
        if (k != 0) return cfail(c, PIE_E_STATE, "the list of a prune / retention purge is held by the first local rank (%d) only", c->rank_of[0]);
        if (rows_dev) *rows_dev = c->q_total ? c->mq_rows : nullptr;
        if (src_rank_dev) *src_rank_dev = c->q_total ? c->mq_rank : nullptr;
        if (src_row_dev) *src_row_dev = c->q_total ? c->mq_row : nullptr;
        if (q_out) *q_out = (size_t)c->q_total;
        return PIE_OK;
    }
    if (rows_dev) *rows_dev = c->q_rows[k];
    if (src_rank_dev) *src_rank_dev = c->q_src_rank[k];
    if (src_row_dev) *src_row_dev = c->q_src_row[k];
    if (q_out) *q_out = (size_t)c->q_total;
    return PIE_OK;
}

int pie_comm_queue_read(pie_comm* c, int32_t at_rank, int32_t* rows_out, int32_t* src_rank_out, int32_t* src_row_out, size_t cap, size_t* q_out)
{
    void *rows = nullptr, *src_rank = nullptr, *src_row = nullptr;
    size_t q = 0;
    const int rc = pie_comm_queue_device_ptrs(c, at_rank, &rows, &src_rank, &src_row, &q);
    if (rc) return rc;
    if (q_out) *q_out = q;
    if ((rows_out || src_rank_out || src_row_out) && q > cap) return cfail(c, PIE_E_CAPACITY, "cap %zu < %zu queued rows", cap, q);
    if (!q) return PIE_OK;
    PIE_CHIP(c, hipSetDevice(c->device[local_index(c, at_rank)]));
    if (rows_out) PIE_CHIP(c, hipMemcpy(rows_out, rows, q * 4, hipMemcpyDeviceToHost));
    if (src_rank_out) PIE_CHIP(c, hipMemcpy(src_rank_out, src_rank, q * 4, hipMemcpyDeviceToHost));
    if (src_row_out) PIE_CHIP(c, hipMemcpy(src_row_out, src_row, q * 4, hipMemcpyDeviceToHost));
    return PIE_OK;
}

int pie_comm_queue_kind(const pie_comm* c) { return c && c->q_total >= 0 ? c->q_kind : PIE_COMM_QUEUE_NONE; }

int pie_comm_queue_timing(pie_comm* c, float* ms_out_4)
{
    if (!c || !ms_out_4) return PIE_E_INVAL;
    if (!c->q_timed) return cfail(c, PIE_E_STATE, "no completed queue call to time");
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    for (int i = 0; i < 4; ++i) PIE_CHIP(c, hipEventElapsedTime(&ms_out_4[i], c->q_tev[i], c->q_tev[i + 1]));
    return PIE_OK;
}

// ---- a live sharded table: the context-level calls by global id on every local shard, nothing exchanged

namespace {
// rows and users of the whole table, which every local shard must agree on
int table_size(pie_comm* c, int64_t* rows_out, int32_t* users_out)
{
    int64_t rows = 0;
    int32_t users = 0;
    for (int k = 0; k < c->n_local; ++k) {
        int64_t r = 0;
        int32_t u = 0;
        PIE_CCTX(c, k, pie_shard_info(c->ctx[k], nullptr, nullptr, &r, &u, nullptr));
        if (k > 0 && (r != rows || u != users))
            return cfail(c, PIE_E_STATE, "rank %d holds a table of %lld rows / %d users, rank %d one of %lld / %d", c->rank_of[k], (long long)r, u,
                         c->rank_of[0], (long long)rows, users);
        rows = r;
        users = u;
    }
    if (rows_out) *rows_out = rows;
    if (users_out) *users_out = users;
    return PIE_OK;
}

int mutate_ready(pie_comm* c, int64_t* rows_out, int32_t* users_out)
{
    if (steps_idle(c)) return PIE_E_STATE;
    return table_size(c, rows_out, users_out);
}
} // namespace

int pie_comm_table_size(pie_comm* c, int64_t* rows_global_out, int32_t* users_global_out)
{
    if (!c) return PIE_E_INVAL;
    return table_size(c, rows_global_out, users_global_out);
}

int pie_comm_append_rows(pie_comm* c, const int64_t* start, const int64_t* end, const int32_t* user, const int32_t* disc, size_t k, int32_t n_users,
                         int32_t* first_row_out)
{
    if (!c) return PIE_E_INVAL;
    if (k > 0 && (!start || !end || !user || !disc)) return cfail(c, PIE_E_INVAL, "NULL column pointer");
    int64_t rows = 0;
    int rc = mutate_ready(c, &rows, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_check_append(c->ctx[i], user, k, n_users));
    if (first_row_out) *first_row_out = (int32_t)rows;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_shard_append_rows(c->ctx[i], start, end, user, disc, k, n_users, nullptr, nullptr));
    return PIE_OK;
}

int pie_comm_set_end(pie_comm* c, const int32_t* rows, const int64_t* new_end, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_check_set_end(c->ctx[i], rows, new_end, k));
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_shard_set_end(c->ctx[i], rows, new_end, k));
    return PIE_OK;
}

int pie_comm_delete_user(pie_comm* c, int32_t user, int32_t* rows_out, size_t cap, size_t* n_deleted, int32_t* owner_rank_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    if (owner_rank_out) *owner_rank_out = -1;
    int32_t users = 0;
    int rc = mutate_ready(c, nullptr, &users);
    if (rc) return rc;
    if (user < 0 || user >= users) return PIE_OK;
    const int owner = pie_shard_of(user, c->world);
    if (owner_rank_out) *owner_rank_out = owner;
    const int i = local_index(c, owner);
    if (i < 0) return PIE_OK; // the owning rank lives in another process, which makes the same call
    PIE_CCTX(c, i, pie_shard_delete_user(c->ctx[i], user, rows_out, cap, n_deleted));
    return PIE_OK;
}

int pie_comm_delete_users(pie_comm* c, const int32_t* users, size_t k, int32_t* rows_out, size_t cap, size_t* n_deleted, int32_t* per_user_out,
                          int32_t* owner_rank_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_deleted) *n_deleted = 0;
    if (k > 0 && !users) return cfail(c, PIE_E_INVAL, "NULL user list");
    int32_t n_users = 0;
    int rc = mutate_ready(c, nullptr, &n_users);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_check_delete_users(c->ctx[i], users, k));
    if (per_user_out && k) memset(per_user_out, 0, k * 4);
    if (owner_rank_out)
        for (size_t j = 0; j < k; ++j) owner_rank_out[j] = (users[j] < 0 || users[j] >= n_users) ? -1 : pie_shard_of(users[j], c->world);
    if (k == 0) return PIE_OK;
    // every local shard gets the whole list; its own list (global rows, ascending) is merged behind the ones before it
    std::vector<int32_t> merged, per;
    try {
        if (per_user_out) per.resize(k);
        for (int i = 0; i < c->n_local; ++i) {
            size_t m = 0;
            PIE_CCTX(c, i, pie_internal::shard_delete_users_run(c->ctx[i], users, k, &m, per_user_out ? per.data() : nullptr));
            if (per_user_out)
                for (size_t j = 0; j < k; ++j) per_user_out[j] += per[j];
            if (n_deleted) *n_deleted += m;
            if (!rows_out || m == 0) continue;
            const size_t before = merged.size();
            merged.resize(before + m);
            PIE_CCTX(c, i, pie_internal::shard_delete_users_copy(c->ctx[i], merged.data() + before, m));
            std::inplace_merge(merged.begin(), merged.begin() + (std::ptrdiff_t)before, merged.end());
        }
    } catch (const std::bad_alloc&) {
        return cfail(c, PIE_E_NOMEM, "no memory for the merged list");
    }
    if (rows_out && merged.size() > cap) return cfail(c, PIE_E_CAPACITY, "list cap %zu < %zu", cap, merged.size()); // tombstoned all the same
    if (rows_out && !merged.empty()) memcpy(rows_out, merged.data(), merged.size() * 4);
    return PIE_OK;
}

// ---- the token column behind the communicator: pie_shard_token_* on every local shard, the lookup merged on the host

int pie_comm_token_set(pie_comm* c, const uint64_t* tok, size_t n)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_token_check(c->ctx[i], tok, n, true));
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_shard_token_set(c->ctx[i], tok, n));
    return PIE_OK;
}

int pie_comm_token_append(pie_comm* c, const uint64_t* tok, size_t k)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_token_check(c->ctx[i], tok, k, false));
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_shard_token_append(c->ctx[i], tok, k));
    return PIE_OK;
}

} // extern "C"

namespace {

// The per-key answer merge of the lookups and the turns: every local shard answers every key, per key the shard with the largest
// global row wins (a shard that does not hold the key answers -1).  One shard's answers land in the scratch, take() folds them
// into the caller's outputs (each may be NULL).
struct KeyMerge {
    int32_t* row_out;
    uint8_t* live_out;
    int32_t* user_out;
    int64_t *start_out, *end_out;
    int32_t* owner_rank_out;
    size_t k = 0;
    std::vector<int32_t> best, row, user;
    std::vector<uint8_t> live;
    std::vector<int64_t> start, end;

    bool alloc(size_t keys)
    {
        try {
            best.assign(keys, -1);
            row.resize(keys);
            user.resize(keys);
            live.resize(keys);
            start.resize(keys);
            end.resize(keys);
        } catch (...) {
            return false;
        }
        k = keys;
        return true;
    }
    // what a key no shard holds reads as; end_none: its end too (the turns), else end_out[j] is left as the caller had it
    void preset(bool end_none)
    {
        if (live_out && k) memset(live_out, 0, k);
        if (owner_rank_out) for (size_t j = 0; j < k; ++j) owner_rank_out[j] = -1;
        if (end_none && end_out) for (size_t j = 0; j < k; ++j) end_out[j] = PIE_END_NONE;
    }
    void take(int owner_rank)
    {
        // (locals: the byte stores to live_out may alias this object, not these)
        int32_t *const b = best.data(), *const uo = user_out, *const oo = owner_rank_out;
        uint8_t* const lo = live_out;
        int64_t *const so = start_out, *const eo = end_out;
        const int32_t *const r = row.data(), *const u = user.data();
        const uint8_t* const l = live.data();
        const int64_t *const s = start.data(), *const e = end.data();
        for (size_t j = 0, n = k; j < n; ++j) {
            if (r[j] <= b[j]) continue;
            b[j] = r[j];
            if (lo) lo[j] = l[j];
            if (uo) uo[j] = u[j];
            if (so) so[j] = s[j];
            if (eo) eo[j] = e[j];
            if (oo) oo[j] = owner_rank;
        }
    }
    void write_rows()
    {
        if (row_out && k) memcpy(row_out, best.data(), k * 4);
    }
};

// a shard's wait phase: shard_token_lookup_wait, shard_token_turn_wait, shard_session_turn_wait, shard_lookup_finish
typedef int (*ShardWait)(pie_ctx*, size_t, int32_t*, uint8_t*, int32_t*, int64_t*, int64_t*);

// pie_shard_token_lookup_finish as a wait phase: the oldest lookup in flight, which must be the one of k keys the communicator began
int shard_lookup_finish(pie_ctx* x, size_t k, int32_t* row, uint8_t* live, int32_t* user, int64_t* start, int64_t* end)
{
    size_t kk = 0;
    const int rc = pie_shard_token_lookup_finish(x, row, live, user, start, end, k, &kk);
    return rc == PIE_OK && kk != k ? PIE_E_STATE : rc;
}

// the first n local shards are waited for and their answers dropped: nothing is left writing a staging block
void wait_out(pie_comm* c, int n, size_t k, ShardWait wait)
{
    for (int i = 0; i < n; ++i) (void)wait(c->ctx[i], k, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// queue(ctx) on every local shard, so that the shards' launches and copies overlap: all are in their streams before the first
// wait.  A shard that refuses is reported once what was queued before it has been waited for.
template <class Queue>
int queue_all(pie_comm* c, size_t k, Queue queue, ShardWait wait)
{
    for (int i = 0; i < c->n_local; ++i) {
        const int rc = queue(c->ctx[i]);
        if (rc == PIE_OK) continue;
        wait_out(c, i, k, wait);
        PIE_CCTX(c, i, rc);
    }
    return PIE_OK;
}

// every local shard is waited for, whatever the ones before it returned; those that succeeded are merged, the first that failed
// is reported; row_out is written only when none failed
int wait_and_merge(pie_comm* c, KeyMerge& m, ShardWait wait)
{
    int first_rc = PIE_OK, first_bad = -1;
    for (int i = 0; i < c->n_local; ++i) {
        const int rc = wait(c->ctx[i], m.k, m.row.data(), m.live.data(), m.user.data(), m.start.data(), m.end.data());
        if (rc == PIE_OK) m.take(c->rank_of[i]);
        else if (first_rc == PIE_OK) { first_rc = rc; first_bad = i; }
    }
    if (first_rc) PIE_CCTX(c, first_bad, first_rc);
    m.write_rows();
    return PIE_OK;
}

} // namespace

extern "C" {

int pie_comm_token_lookup(pie_comm* c, const uint64_t* tok, size_t k, int64_t now, int32_t* row_out, uint8_t* live_out, int32_t* user_out,
                          int64_t* start_out, int64_t* end_out, int32_t* owner_rank_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    if (k > 0 && !tok) return cfail(c, PIE_E_INVAL, "tok is NULL");
    const ShardWait wait = pie_internal::shard_token_lookup_wait;
    rc = queue_all(c, k, [&](pie_ctx* x) { return pie_internal::shard_token_lookup_queue(x, tok, k, now); }, wait);
    if (rc || k == 0) return rc;
    KeyMerge m{row_out, live_out, user_out, start_out, end_out, owner_rank_out};
    if (!m.alloc(k)) {
        wait_out(c, c->n_local, k, wait);
        return cfail(c, PIE_E_NOMEM, "no memory for %zu answers", k);
    }
    m.preset(false);
    return wait_and_merge(c, m, wait);
}

int pie_comm_token_set_end(pie_comm* c, const uint64_t* tok, const int64_t* new_end, size_t k, int64_t now, int32_t* rows_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc || k == 0) return rc;
    if (!tok || !new_end) return cfail(c, PIE_E_INVAL, "NULL pointer");
    std::vector<int32_t> row, rows;
    std::vector<uint8_t> live;
    std::vector<int64_t> ends;
    try {
        row.resize(k);
        live.resize(k);
        rows.reserve(k);
        ends.reserve(k);
    } catch (...) {
        return cfail(c, PIE_E_NOMEM, "no memory for %zu touches", k);
    }
    rc = pie_comm_token_lookup(c, tok, k, now, row.data(), live.data(), nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    for (size_t i = 0; i < k; ++i) {
        const bool hit = live[i] != 0 && row[i] >= 0;
        if (rows_out) rows_out[i] = hit ? row[i] : -1;
        if (hit) {
            rows.push_back(row[i]);
            ends.push_back(new_end[i]);
        }
    }
    if (rows.empty()) return PIE_OK;
    return pie_comm_set_end(c, rows.data(), ends.data(), rows.size());
}

// the same turn on every local shard: all checked before any is changed, all queued before any is waited for, then
// pie_comm_token_lookup's merge per op (the shard with the largest global row answers)
int pie_comm_token_turn(pie_comm* c, const pie_turn_op* ops, size_t k, int32_t* row_out, uint8_t* live_out, int32_t* owner_rank_out,
                        int32_t* user_out, int64_t* start_out, int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_token_turn_check(c->ctx[i], ops, k));
    if (k == 0) return PIE_OK;
    KeyMerge m{row_out, live_out, user_out, start_out, end_out, owner_rank_out};
    if (!m.alloc(k)) return cfail(c, PIE_E_NOMEM, "no memory for %zu answers", k); // nothing queued yet
    const ShardWait wait = pie_internal::shard_token_turn_wait;
    rc = queue_all(c, k, [&](pie_ctx* x) { return pie_internal::shard_token_turn_queue(x, ops, k); }, wait);
    if (rc) return rc;
    // (a DELETE that met a tombstone answers -1 on its own shard too: it merges as a key nobody holds, which reads the same)
    m.preset(true);
    return wait_and_merge(c, m, wait);
}

// The turn that logs in, on every local shard (pie_shard_session_turn's phases): all checked before any is changed, room made on
// all before any is queued, all queued before any is waited for, then pie_comm_token_turn's merge per op.  A create is kept by
// one shard and answered -1 by the others, so the merge hands out the keeper's answer.
int pie_comm_session_turn(pie_comm* c, const pie_turn_op* ops, size_t k, const int32_t* user, const int32_t* disc, int32_t n_users,
                          int32_t* row_out, uint8_t* live_out, int32_t* owner_rank_out, int32_t* user_out, int64_t* start_out, int64_t* end_out)
{
    if (!c) return PIE_E_INVAL;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_session_turn_check(c->ctx[i], ops, k, user, disc, n_users));
    KeyMerge m{row_out, live_out, user_out, start_out, end_out, owner_rank_out};
    if (!m.alloc(k)) return cfail(c, PIE_E_NOMEM, "no memory for %zu answers", k); // nothing changed yet
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_session_turn_room(c->ctx[i], ops, k, user, n_users));
    const ShardWait wait = pie_internal::shard_session_turn_wait;
    rc = queue_all(c, k, [&](pie_ctx* x) { return pie_internal::shard_session_turn_queue(x, ops, k, user, disc, n_users); }, wait);
    if (rc || k == 0) return rc; // (an empty turn still ran its room and queue phases)
    m.preset(true);
    return wait_and_merge(c, m, wait);
}

} // extern "C"

// ---- the pipelined exchanges (pie_comm_step_* and pie_comm_wide_step_*): ONE union message per step and shard, written by the
// shard's own batch tail (layouts: pie_scan_batch_begin_union / pie_scan_wide_begin_union); the exchange of a step runs on a side
// stream while the shards scan the next ones (the C-ABI counterpart of shard.py's BatchedFeeds.run_steps).  One engine, two
// kinds; what differs between them is in StepKind and the four small functions below it.  For both kinds:
//   - a step's gathered buffers are handed out from its collect until `sets` more steps have begun (16 ordinary, 8 wide), and never
//     for a step that failed on this process;
//   - the geometry (u_pad, cap, words per row) is the kind's own: neither the other kind's reservation nor the synchronous path
//     (pie_comm_reserve / pie_comm_scan_batch_gather) moves it under the buffers;
//   - a shard that cannot begin after others began drains every step in flight (step_drain): nothing is left in the shards' FIFOs;
//   - every wait is bounded (wait_event, PIE_WAIT_DEADLINE_MS).
namespace {

struct StepKind {
    bool wide;
    int sets;              // rotating buffer sets: steps uncollected at most
    int ahead;             // steps begun and unfinished at most (what the shards' batch lanes hold, below the sets)
    int nq_max;
    const char* api;       // prefix of the kind's entry points, for messages
    const char* no_union;  // collect's text for Mu = -1
};

const StepKind kOrdinary{false, 16, 12, PIE_BATCH_MAX, "pie_comm_step",
                         "a shard's union could not be formed (Mu = -1: queries fell back and a user's merged union exceeds 32 rows, or more than 32 queries): use pie_comm_scan_batch_gather for this batch"};
const StepKind kWide{true, 8, 6, PIE_WIDE_MAX, "pie_comm_wide_step",
                     "a shard's wide batch kept no union (Mu = -1, pie_comm_wide_step_status): repeat the step; dense queries go through pie_comm_scan_batch_gather"};

pie_steps& steps_of(pie_comm* c, const StepKind& kd) { return kd.wide ? c->wide : c->ord; }

// words per union row for n_q queries (ordinary: row + one or two 32-bit mask planes; wide: 64-bit mask words) and the message length
int step_words(const StepKind& kd, int n_q) { return kd.wide ? (n_q + 63) / 64 : n_q > 32 ? 3 : 2; }
long long step_msg_words(const StepKind& kd, long long u_pad, long long cap, int words)
{
    return u_pad + 2 + cap * (kd.wide ? 1 + 2 * (long long)words : (long long)words);
}

int step_ctx_begin(const StepKind& kd, pie_ctx* ctx, const pie_query* queries, int n_q, int* msg, const pie_steps& st)
{
    return kd.wide ? pie_scan_wide_begin_union(ctx, queries, n_q, msg, (size_t)st.u_pad, (size_t)st.cap)
                   : pie_scan_batch_begin_union(ctx, queries, n_q, msg, (size_t)st.u_pad, (size_t)st.cap);
}

// the oldest batch in flight on a shard; m == nullptr: finished and dropped
int step_ctx_finish(const StepKind& kd, pie_ctx* ctx, size_t* m, int n_q, int* ready)
{
    int nq = 0;
    if (!m) return kd.wide ? pie_scan_wide_finish(ctx, nullptr, 0, nullptr) : pie_scan_batch_finish_packed(ctx, nullptr, nullptr);
    return kd.wide ? pie_scan_wide_finish_packed(ctx, m, (size_t)n_q, &nq, ready) : pie_scan_batch_finish_packed(ctx, m, ready);
}

void free_step_buffers(pie_comm* c, pie_steps& st)
{
    for (int s = 0; s < pie_steps::kMaxSets; ++s) {
        for (int k = 0; k < c->n_local; ++k) {
            (void)hipSetDevice(c->device[k]);
            if (k < (int)st.msg[s].size() && st.msg[s][k]) (void)hipFree(st.msg[s][k]);
            if (k < (int)st.gath[s].size() && st.gath[s][k]) (void)hipFree(st.gath[s][k]);
            if (k < (int)st.ready[s].size() && st.ready[s][k]) (void)hipEventDestroy(st.ready[s][k]);
            if (k < (int)st.done[s].size() && st.done[s][k]) (void)hipEventDestroy(st.done[s][k]);
        }
        for (auto* v : {&st.msg[s], &st.gath[s]}) v->assign((size_t)c->n_local, nullptr);
        for (auto* v : {&st.ready[s], &st.done[s]}) v->assign((size_t)c->n_local, nullptr);
        if (st.h_mu[s]) (void)hipHostFree(st.h_mu[s]);
        st.h_mu[s] = st.h_mu_dev[s] = nullptr;
    }
    st.cap = st.L = 0;
}

// the rotating buffer sets; the geometry changes only while no step of the kind is in flight
int step_reserve(pie_comm* c, const StepKind& kd, int32_t n_q, int32_t u_pad_in, size_t union_cap)
{
    if (!c) return PIE_E_INVAL;
    if (n_q < 1 || n_q > kd.nq_max) return cfail(c, PIE_E_INVAL, "%s_reserve: 1..%d queries (got %d)", kd.api, kd.nq_max, n_q);
    pie_steps& st = steps_of(c, kd);
    long long u_pad = 0;
    int rc = resolve_u_pad(c, u_pad_in, &u_pad);
    if (rc) return rc;
    const long long cap = (long long)(union_cap > 0 ? union_cap : 1024);
    int words = step_words(kd, n_q);
    if (st.L > 0 && st.u_pad == u_pad && cap <= st.cap && words <= st.words_max && st.msg[0].size() == (size_t)c->n_local && st.msg[0][0]) return PIE_OK;
    if (!kd.wide && st.words_max > words) words = st.words_max; // an ordinary reservation keeps the second mask plane once it had one
    if (step_msg_words(kd, u_pad, cap, words) > 0x7FFFFFF0LL) return cfail(c, PIE_E_INVAL, "a message of %lld words is too long", step_msg_words(kd, u_pad, cap, words));
    if (st.begun != st.collected) return cfail(c, PIE_E_STATE, "steps are in flight: %s_collect them before the message size changes", kd.api);
    free_step_buffers(c, st);
    st.u_pad = u_pad;
    st.cap = cap;
    st.words_max = words;
    const long long L = step_msg_words(kd, u_pad, cap, words); // st.L is set last: a reservation that failed midway reads as none
    if (c->xstream.size() != (size_t)c->n_local) c->xstream.assign((size_t)c->n_local, nullptr);
    for (int s = 0; s < kd.sets; ++s) {
        PIE_CHIP(c, hipHostMalloc(&st.h_mu[s], (size_t)c->n_local * (size_t)c->world * 4, hipHostMallocMapped));
        PIE_CHIP(c, hipHostGetDevicePointer((void**)&st.h_mu_dev[s], st.h_mu[s], 0));
    }
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        if (!c->xstream[k]) PIE_CHIP(c, hipStreamCreateWithFlags(&c->xstream[k], hipStreamNonBlocking));
        for (int s = 0; s < kd.sets; ++s) {
            PIE_CHIP(c, hipMalloc(&st.msg[s][k], (size_t)L * 4));
            PIE_CHIP(c, hipMalloc(&st.gath[s][k], (size_t)L * 4 * (size_t)c->world));
            PIE_CHIP(c, hipMemset(st.msg[s][k], 0, (size_t)L * 4));
            PIE_CHIP(c, hipEventCreateWithFlags(&st.ready[s][k], hipEventDisableTiming));
            PIE_CHIP(c, hipEventCreateWithFlags(&st.done[s][k], hipEventDisableTiming));
        }
    }
    st.L = L;
    return PIE_OK;
}

// a partial failure left batches begun on some shards: every step in flight on this process is finished in order and marked
// failed (its collect says so), then the batches of the step that failed to begin; nothing is left in the shards' FIFOs
void step_drain(pie_comm* c, const StepKind& kd, int begun_here, int why)
{
    pie_steps& st = steps_of(c, kd);
    for (; st.finished < st.begun; st.finished++) {
        for (int k = 0; k < c->n_local; ++k) (void)step_ctx_finish(kd, c->ctx[k], nullptr, 0, nullptr);
        st.rc[st.finished % kd.sets] = why;
    }
    for (int k = 0; k < begun_here; ++k) (void)step_ctx_finish(kd, c->ctx[k], nullptr, 0, nullptr);
}

int step_begin(pie_comm* c, const StepKind& kd, const pie_query* queries, int32_t n_q)
{
    if (!c) return PIE_E_INVAL;
    if (!queries || n_q < 1 || n_q > kd.nq_max) return cfail(c, PIE_E_INVAL, "%s_begin: a step holds 1..%d queries (got %d)", kd.api, kd.nq_max, n_q);
    pie_steps& st = steps_of(c, kd);
    const pie_steps& other = steps_of(c, kd.wide ? kOrdinary : kWide);
    if (st.L <= 0) return cfail(c, PIE_E_STATE, "%s_reserve first", kd.api);
    if (other.begun != other.collected) return cfail(c, PIE_E_STATE, "%s steps are in flight: collect them first", kd.wide ? "ordinary (pie_comm_step_*)" : "wide (pie_comm_wide_step_*)");
    if (step_words(kd, n_q) > st.words_max) return cfail(c, PIE_E_STATE, "reserved for fewer than %d queries: %s_reserve again", n_q, kd.api);
    // steps begun and unfinished: what the shards' batch lanes hold (three per lane, pie_set_batch_lanes; lane 0 only on the ordered run)
    if (st.begun - st.finished >= kd.ahead) return cfail(c, PIE_E_STATE, "%d steps are already begun: %s_finish first", kd.ahead, kd.api);
    for (int k = 0; k < c->n_local; ++k)
        if (pie_batch_room(c->ctx[k]) <= 0)
            return cfail(c, PIE_E_STATE, "rank %d: the steps begun fill its batch slots (three per batch lane): %s_finish first", c->rank_of[k], kd.api);
    if (st.begun - st.collected >= kd.sets) return cfail(c, PIE_E_STATE, "%d steps are uncollected: %s_collect first", kd.sets, kd.api);
    const int s = (int)(st.begun % kd.sets);
    int begun = 0, rc = PIE_OK;
    for (int k = 0; k < c->n_local && rc == PIE_OK; ++k) {
        rc = step_ctx_begin(kd, c->ctx[k], queries, n_q, st.msg[s][k], st);
        if (rc == PIE_OK) ++begun;
        else cfail(c, rc, "rank %d: %s", c->rank_of[k], pie_last_error(c->ctx[k]));
    }
    if (rc != PIE_OK) { // the step is not counted
        if (begun > 0) step_drain(c, kd, begun, rc);
        return rc;
    }
    st.nq[s] = n_q;
    st.rc[s] = PIE_OK;
    st.begun++;
    return PIE_OK;
}

int step_finish(pie_comm* c, const StepKind& kd, size_t* m_out, size_t m_cap)
{
    if (!c) return PIE_E_INVAL;
    pie_steps& st = steps_of(c, kd);
    if (st.finished >= st.begun) return cfail(c, PIE_E_STATE, "%s_finish without %s_begin", kd.api, kd.api);
    const int s = (int)(st.finished % kd.sets);
    const int n_q = st.nq[s];
    if (m_out && m_cap < (size_t)c->n_local * (size_t)n_q)
        return cfail(c, PIE_E_CAPACITY, "m_cap %zu < %d local ranks x %d queries", m_cap, c->n_local, n_q);
    std::vector<size_t> m((size_t)c->n_local * (size_t)n_q, 0);
    int first_rc = PIE_OK;
    for (int k = 0; k < c->n_local; ++k) {
        int ready = 0;
        const int rc = step_ctx_finish(kd, c->ctx[k], &m[(size_t)k * n_q], n_q, &ready);
        if (rc != PIE_OK && first_rc == PIE_OK) {
            first_rc = rc;
            cfail(c, rc, "rank %d: %s", c->rank_of[k], pie_last_error(c->ctx[k]));
        }
        // ready = 0: the message (or its Mu = -1 header) was written on the context's stream behind the batch: the exchange stream waits for exactly that
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        if (!ready) {
            PIE_CHIP(c, hipEventRecord(st.ready[s][k], c->stream[k]));
            PIE_CHIP(c, hipStreamWaitEvent(c->xstream[k], st.ready[s][k], 0));
        }
    }
    st.finished++;
    st.rc[s] = first_rc;
    if (first_rc != PIE_OK) return first_rc; // every local batch has been finished; no exchange is queued for this step (its collect says so)
    // the exchange of this step, on the side streams: nothing here waits for it.  An ordinary step sends the whole message, a wide
    // step only the prefix its n_q uses: every rank knows n_q, so every rank agrees on the length
    const size_t count = (size_t)(kd.wide ? step_msg_words(kd, st.u_pad, st.cap, step_words(kd, n_q)) : st.L);
    int rc = exchange(c, st.msg[s], st.gath[s], count, (size_t)st.L, c->xstream);
    if (rc) return st.rc[s] = rc;
    for (int k = 0; k < c->n_local; ++k) {
        PIE_CHIP(c, hipSetDevice(c->device[k]));
        hipLaunchKernelGGL(k_pick_words, dim3(1), dim3(64), 0, c->xstream[k], st.gath[s][k], st.L, st.u_pad + 1, c->world, st.h_mu_dev[s] + (size_t)k * (size_t)c->world);
        PIE_CHIP(c, hipEventRecord(st.done[s][k], c->xstream[k]));
    }
    if (m_out) memcpy(m_out, m.data(), m.size() * sizeof(size_t));
    return PIE_OK;
}

int step_collect(pie_comm* c, const StepKind& kd, int64_t* step_out)
{
    if (!c) return PIE_E_INVAL;
    pie_steps& st = steps_of(c, kd);
    if (st.collected >= st.finished) return cfail(c, PIE_E_STATE, "no exchange to collect: %s_finish first", kd.api);
    const long long step = st.collected++;
    const int s = (int)(step % kd.sets);
    if (step_out) *step_out = (int64_t)step;
    if (st.rc[s] != PIE_OK) return cfail(c, PIE_E_STATE, "step %lld failed before its exchange (status %d): nothing was exchanged", step, st.rc[s]);
    for (int k = 0; k < c->n_local; ++k) // the side stream only: the shards' scan streams run on
        if (int rc = wait_event(c, k, st.done[s][k], "step exchange")) return st.rc[s] = rc;
    long long need = 0;
    bool no_union = false;
    for (int p = 0; p < c->world; ++p) { // every rank holds the same world Mu words
        const int mu = st.h_mu[s][p];
        if (mu < 0) no_union = true;
        if (mu > need) need = mu;
    }
    c->need = need;
    if (no_union) return cfail(c, PIE_E_CAPACITY, "%s", kd.no_union);
    if (need > st.cap)
        return cfail(c, PIE_E_CAPACITY, "a union of %lld rows exceeds the reserved capacity %lld on some rank: collect what is in flight, %s_reserve(pie_comm_needed_cap), repeat the step", need, st.cap, kd.api);
    return PIE_OK;
}

// the gathered Mu words ([local index][world]) of a step that is collected, did not fail and whose buffers are not reused: nullptr otherwise
const int* step_mu(pie_comm* c, const StepKind& kd, int64_t step)
{
    const pie_steps& st = steps_of(c, kd);
    if (step < 0 || step >= st.collected || step + kd.sets <= st.begun) return nullptr;
    const int s = (int)(step % kd.sets);
    return st.rc[s] == PIE_OK ? st.h_mu[s] : nullptr;
}

int step_invalid(pie_comm* c, const StepKind& kd, int64_t step)
{
    return cfail(c, PIE_E_STATE, "%s: step %lld is not collected, failed before its exchange, or its buffers were reused", kd.api, (long long)step);
}

int step_gathered_ptr(pie_comm* c, const StepKind& kd, int32_t at_rank, int64_t step, void** base_out, size_t* rank_stride_words, size_t* u_pad_out, size_t* cap_out)
{
    if (!c) return PIE_E_INVAL;
    const pie_steps& st = steps_of(c, kd);
    const int k = local_index(c, at_rank);
    if (k < 0 || st.L <= 0) return cfail(c, PIE_E_STATE, "rank %d is not local to this communicator or nothing was reserved", at_rank);
    if (!step_mu(c, kd, step)) return step_invalid(c, kd, step);
    if (base_out) *base_out = st.gath[step % kd.sets][k];
    if (rank_stride_words) *rank_stride_words = (size_t)st.L;
    if (u_pad_out) *u_pad_out = (size_t)st.u_pad;
    if (cap_out) *cap_out = (size_t)st.cap;
    return PIE_OK;
}

// what both read_gathered forms share: the message of src_rank as at_rank holds it, its Mu from the words collect already has,
// the user offsets; *have_out = the union rows the message holds (PIE_E_CAPACITY if rows or masks are asked for and cap is below it)
int step_read_head(pie_comm* c, const StepKind& kd, int32_t at_rank, int32_t src_rank, int64_t step, int32_t* uoff_out, int32_t* rows_out, bool want_rows,
                   size_t cap, size_t* mu_out, const int** msg_out, size_t* have_out)
{
    void* base = nullptr;
    int rc = step_gathered_ptr(c, kd, at_rank, step, &base, nullptr, nullptr, nullptr);
    if (rc) return rc;
    if (src_rank < 0 || src_rank >= c->world) return cfail(c, PIE_E_INVAL, "source rank outside the communicator");
    const pie_steps& st = steps_of(c, kd);
    const int k = local_index(c, at_rank);
    PIE_CHIP(c, hipSetDevice(c->device[k]));
    const int* msg = static_cast<const int*>(base) + (size_t)src_rank * (size_t)st.L;
    const int mu32 = step_mu(c, kd, step)[(size_t)k * (size_t)c->world + (size_t)src_rank];
    const size_t mu = mu32 > 0 ? (size_t)mu32 : 0;
    if (mu_out) *mu_out = mu;
    if (uoff_out) PIE_CHIP(c, hipMemcpy(uoff_out, msg, ((size_t)st.u_pad + 1) * 4, hipMemcpyDeviceToHost));
    const size_t have = mu < (size_t)st.cap ? mu : (size_t)st.cap;
    if (want_rows && have > cap) return cfail(c, PIE_E_CAPACITY, "cap %zu < %zu union rows", cap, have);
    if (rows_out && have) PIE_CHIP(c, hipMemcpy(rows_out, msg + st.u_pad + 2, have * 4, hipMemcpyDeviceToHost));
    *msg_out = msg;
    *have_out = have;
    return PIE_OK;
}

} // namespace

extern "C" {

int pie_comm_step_reserve(pie_comm* c, int32_t n_q, int32_t u_pad, size_t union_cap) { return step_reserve(c, kOrdinary, n_q, u_pad, union_cap); }
int pie_comm_step_begin(pie_comm* c, const pie_query* queries, int32_t n_q) { return step_begin(c, kOrdinary, queries, n_q); }
int pie_comm_step_finish(pie_comm* c, size_t* m_out) { return step_finish(c, kOrdinary, m_out, (size_t)-1); }
int pie_comm_step_collect(pie_comm* c, int64_t* step_out) { return step_collect(c, kOrdinary, step_out); }
int pie_comm_step_gathered_ptr(pie_comm* c, int32_t at_rank, int64_t step, void** base_out, size_t* rank_stride_words, size_t* u_pad_out, size_t* cap_out)
{
    return step_gathered_ptr(c, kOrdinary, at_rank, step, base_out, rank_stride_words, u_pad_out, cap_out);
}

int pie_comm_wide_step_reserve(pie_comm* c, int32_t n_q_max, int32_t u_pad, size_t union_cap) { return step_reserve(c, kWide, n_q_max, u_pad, union_cap); }
int pie_comm_wide_step_begin(pie_comm* c, const pie_query* queries, int32_t n_q) { return step_begin(c, kWide, queries, n_q); }
int pie_comm_wide_step_finish(pie_comm* c, size_t* m_out, size_t m_cap) { return step_finish(c, kWide, m_out, m_cap); }
int pie_comm_wide_step_collect(pie_comm* c, int64_t* step_out) { return step_collect(c, kWide, step_out); }
int pie_comm_wide_step_gathered_ptr(pie_comm* c, int32_t at_rank, int64_t step, void** base_out, size_t* rank_stride_words, size_t* u_pad_out,
                                    size_t* cap_out, int* words_out)
{
    const int rc = step_gathered_ptr(c, kWide, at_rank, step, base_out, rank_stride_words, u_pad_out, cap_out);
    if (rc == PIE_OK && words_out) *words_out = step_words(kWide, c->wide.nq[step % kWide.sets]);
    return rc;
}

// masks: planar in an ordinary message (a plane of low 32-bit words, then a plane of high words when the step had more than 32 queries)
int pie_comm_step_read_gathered(pie_comm* c, int32_t at_rank, int32_t src_rank, int64_t step, int32_t* uoff_out, int32_t* rows_out, uint64_t* masks_out,
                                size_t cap, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    const int* msg = nullptr;
    size_t have = 0;
    int rc = step_read_head(c, kOrdinary, at_rank, src_rank, step, uoff_out, rows_out, rows_out || masks_out, cap, mu_out, &msg, &have);
    if (rc) return rc;
    const pie_steps& st = c->ord;
    if (masks_out && have) {
        std::vector<uint32_t> lo(have), hi;
        PIE_CHIP(c, hipMemcpy(lo.data(), msg + st.u_pad + 2 + st.cap, have * 4, hipMemcpyDeviceToHost));
        if (st.words_max == 3 && st.nq[step % kOrdinary.sets] > 32) {
            hi.resize(have);
            PIE_CHIP(c, hipMemcpy(hi.data(), msg + st.u_pad + 2 + 2 * st.cap, have * 4, hipMemcpyDeviceToHost));
        }
        for (size_t i = 0; i < have; ++i) masks_out[i] = (uint64_t)lo[i] | (hi.empty() ? 0ull : ((uint64_t)hi[i] << 32));
    }
    return PIE_OK;
}

// ... interleaved in a wide one: two int32 words per 64-bit mask word, low word first — the host's uint64 as it stands
int pie_comm_wide_step_read_gathered(pie_comm* c, int32_t at_rank, int32_t src_rank, int64_t step, int32_t* uoff_out, int32_t* rows_out,
                                     uint64_t* masks_out, size_t cap, int* words_out, size_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    if (mu_out) *mu_out = 0;
    if (words_out) *words_out = 0;
    const int* msg = nullptr;
    size_t have = 0;
    int rc = step_read_head(c, kWide, at_rank, src_rank, step, uoff_out, rows_out, rows_out || masks_out, cap, mu_out, &msg, &have);
    if (rc) return rc;
    const pie_steps& st = c->wide;
    const int words = step_words(kWide, st.nq[step % kWide.sets]);
    if (words_out) *words_out = words;
    if (masks_out && have) PIE_CHIP(c, hipMemcpy(masks_out, msg + st.u_pad + 2 + st.cap, have * (size_t)words * 8, hipMemcpyDeviceToHost));
    return PIE_OK;
}

int pie_comm_wide_step_status(pie_comm* c, int64_t step, int32_t* mu_out)
{
    if (!c) return PIE_E_INVAL;
    const int* mu = step_mu(c, kWide, step);
    if (!mu) return step_invalid(c, kWide, step);
    if (mu_out)
        for (int p = 0; p < c->world; ++p) mu_out[p] = mu[p];
    return PIE_OK;
}

int pie_comm_wide_step_read_feed(pie_comm* c, int32_t at_rank, int32_t src_rank, int64_t step, int32_t qi, int32_t local_user, int32_t* idx_out,
                                 size_t idx_cap, size_t* k_out)
{
    if (!c) return PIE_E_INVAL;
    if (k_out) *k_out = 0;
    void* base = nullptr;
    int words = 0;
    int rc = pie_comm_wide_step_gathered_ptr(c, at_rank, step, &base, nullptr, nullptr, nullptr, &words);
    if (rc) return rc;
    const pie_steps& st = c->wide;
    const int n_q = st.nq[step % kWide.sets];
    if (src_rank < 0 || src_rank >= c->world || qi < 0 || qi >= n_q || local_user < 0 || (long long)local_user >= st.u_pad)
        return cfail(c, PIE_E_INVAL, "source rank / query / user outside the step");
    const int k = local_index(c, at_rank);
    PIE_CHIP(c, hipSetDevice(c->device[k]));
    const int* msg = static_cast<const int*>(base) + (size_t)src_rank * (size_t)st.L;
    int ab[2] = {0, 0};
    PIE_CHIP(c, hipMemcpy(ab, msg + local_user, 8, hipMemcpyDeviceToHost));
    if (ab[0] < 0 || ab[1] < ab[0]) return cfail(c, PIE_E_STATE, "rank %d kept no union in wide step %lld (Mu = -1)", src_rank, (long long)step);
    if ((long long)ab[1] > st.cap) return cfail(c, PIE_E_CAPACITY, "the user's rows were cut: the union outgrew the reserved capacity %lld", st.cap);
    const size_t n = (size_t)(ab[1] - ab[0]);
    if (n == 0) return PIE_OK;
    std::vector<int32_t> rows(n);
    std::vector<uint64_t> masks(n * (size_t)words);
    PIE_CHIP(c, hipMemcpy(rows.data(), msg + st.u_pad + 2 + ab[0], n * 4, hipMemcpyDeviceToHost));
    PIE_CHIP(c, hipMemcpy(masks.data(), msg + st.u_pad + 2 + st.cap + (size_t)ab[0] * 2 * (size_t)words, n * (size_t)words * 8, hipMemcpyDeviceToHost));
    size_t kk = 0;
    for (size_t i = 0; i < n; ++i)
        if ((masks[i * (size_t)words + (size_t)(qi >> 6)] >> (qi & 63)) & 1ull) {
            if (idx_out && kk < idx_cap) idx_out[kk] = rows[i];
            ++kk;
        }
    if (k_out) *k_out = kk;
    if (idx_out && kk > idx_cap) return cfail(c, PIE_E_CAPACITY, "idx_cap %zu < %zu rows", idx_cap, kk);
    return PIE_OK;
}

} // extern "C"

// ---- token lookups and the expired queue WHILE STEPS ARE IN FLIGHT (pie_comm_token_lookup_begin / _finish / _room,
// pie_comm_expired_queue_begin / _finish / _room): pie_shard_token_lookup_* / pie_shard_expired_queue_* on every local shard.  No
// RCCL call, no exchange stream, no step buffer set, no wait on a context's stream or a lane: every shard's pass runs on its own
// side stream and every host wait is a bounded one (pie_wait.h).  The communicator counts what it has begun; a shard whose own
// room says otherwise was used directly (pie_shard_* on a context from pie_comm_ctx) and the begin is refused with nothing taken.
namespace {

bool xq_staged(const pie_comm* c, int k) { return c->xq_stage_all || c->device[k] != c->device[0]; }

// every local shard's ascending list as the shard holds it: global rows, the local rows beside them (all NULL: none ride along),
// the rows of it that are merged, and the event its pass is done at (NULL: already waited for)
struct ShardLists {
    const int32_t* rows[kMergeMaxLists] = {};
    const int32_t* local[kMergeMaxLists] = {};
    size_t kept[kMergeMaxLists] = {};
    void* done[kMergeMaxLists] = {};
};

// The merge of the local shards' lists on the first local rank's device, queued on `ms` (that device is current): lists that
// xq_staged names are copied into `stage` first (global rows, then local rows, back to back), each behind its shard's done event;
// the descriptor goes up from `pinned` asynchronously, or (NULL) from the stack with a copy that waits; the events of
// `before_launch` are recorded between the upload and k_merge_shard_queues<out_row != NULL>.  The buffers are the caller's.
hipError_t merge_shard_lists(pie_comm* c, const ShardLists& in, hipStream_t ms, MergeDesc* pinned, void* desc_dev, int* stage,
                             std::initializer_list<hipEvent_t> before_launch, long long out_cap, int* out_rows, int* out_rank, int* out_row)
{
    MergeDesc on_stack;
    MergeDesc* d = pinned ? pinned : &on_stack;
    memset(d, 0, sizeof(MergeDesc));
    hipError_t e = hipSuccess;
    long long acc = 0;
    for (int i = 0; i < c->n_local; ++i) {
        const size_t kept = in.kept[i];
        d->rows[i] = in.rows[i];
        d->local[i] = in.local[i];
        d->n[i] = (int)kept;
        d->rank[i] = c->rank_of[i];
        d->pre[i] = acc;
        acc += (long long)kept;
        if (kept == 0) continue;
        if (i > 0 && in.done[i] && (e = hipStreamWaitEvent(ms, (hipEvent_t)in.done[i], 0)) != hipSuccess) return e;
        if (!xq_staged(c, i)) continue;
        for (const int** list : {&d->rows[i], &d->local[i]}) {
            if (!*list) continue;
            e = c->device[i] != c->device[0] ? hipMemcpyPeerAsync(stage, c->device[0], *list, c->device[i], kept * 4, ms)
                                             : hipMemcpyAsync(stage, *list, kept * 4, hipMemcpyDeviceToDevice, ms);
            if (e != hipSuccess) return e;
            *list = stage;
            stage += kept;
        }
    }
    d->pre[c->n_local] = acc;
    d->count = c->n_local;
    e = pinned ? hipMemcpyAsync(desc_dev, d, sizeof(MergeDesc), hipMemcpyHostToDevice, ms) : hipMemcpy(desc_dev, d, sizeof(MergeDesc), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    for (hipEvent_t ev : before_launch)
        if ((e = hipEventRecord(ev, ms)) != hipSuccess) return e;
    const long long blocks = std::min<long long>((acc + 255) / 256, 2048);
    if (out_row)
        hipLaunchKernelGGL(k_merge_shard_queues<true>, dim3((unsigned)blocks), dim3(256), 0, ms, (const MergeDesc*)desc_dev, out_cap, out_rows, out_rank, out_row);
    else
        hipLaunchKernelGGL(k_merge_shard_queues<false>, dim3((unsigned)blocks), dim3(256), 0, ms, (const MergeDesc*)desc_dev, out_cap, out_rows, out_rank, out_row);
    return hipGetLastError();
}

// The merged list, the staging of lists held on other devices, the descriptor and the pinned block, sized by the begin.  A block
// a begin outgrew is set aside until pie_comm_destroy: hipFree and hipHostFree wait for the whole device, the steps included.
int xq_ensure(pie_comm* c, size_t cap_rows)
{
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    if (!c->xq_ev) PIE_CHIP(c, hipEventCreateWithFlags(&c->xq_ev, hipEventDisableTiming));
    if (!c->xq_desc) PIE_CHIP(c, hipMalloc(&c->xq_desc, sizeof(MergeDesc)));
    try {
        if (!c->xq_h || cap_rows > c->xq_room) {
            size_t rows = c->xq_room ? c->xq_room : 4096;
            while (rows < cap_rows) rows *= 2;
            int *nr = nullptr, *no = nullptr;
            char* nh = nullptr;
            c->xq_retired_dev.reserve(c->xq_retired_dev.size() + 2);
            c->xq_retired_host.reserve(c->xq_retired_host.size() + 1);
            PIE_CHIP(c, hipMalloc(&nr, rows * 4));
            if (hipMalloc(&no, rows * 4) != hipSuccess || hipHostMalloc(&nh, sizeof(MergeDesc) + rows * 8, hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                c->xq_retired_dev.push_back(nr);
                if (no) c->xq_retired_dev.push_back(no);
                return cfail(c, PIE_E_NOMEM, "no memory for a merged queue of %zu rows", cap_rows);
            }
            if (c->xq_rows) c->xq_retired_dev.push_back(c->xq_rows);
            if (c->xq_owner) c->xq_retired_dev.push_back(c->xq_owner);
            if (c->xq_h) c->xq_retired_host.push_back(c->xq_h);
            c->xq_rows = nr;
            c->xq_owner = no;
            c->xq_h = nh;
            c->xq_room = rows;
        }
        size_t staged = 0;
        for (int k = 0; k < c->n_local; ++k) staged += xq_staged(c, k) ? 1 : 0;
        if (staged * cap_rows > c->xq_stage_room) {
            size_t rows = c->xq_stage_room ? c->xq_stage_room : 4096;
            while (rows < staged * cap_rows) rows *= 2;
            int* ns = nullptr;
            c->xq_retired_dev.reserve(c->xq_retired_dev.size() + 1);
            PIE_CHIP(c, hipMalloc(&ns, rows * 4));
            if (c->xq_stage) c->xq_retired_dev.push_back(c->xq_stage);
            c->xq_stage = ns;
            c->xq_stage_room = rows;
        }
    } catch (const std::bad_alloc&) {
        return cfail(c, PIE_E_NOMEM, "out of host memory");
    }
    return PIE_OK;
}

// pie_comm_destroy: what was begun and not finished lands (every wait bounded), then the buffers go
void inflight_close(pie_comm* c)
{
    for (; c->lk_n > 0; c->lk_n--)
        for (int k = 0; k < c->n_local; ++k)
            if (c->ctx[k]) (void)pie_shard_token_lookup_finish(c->ctx[k], nullptr, nullptr, nullptr, nullptr, nullptr, (size_t)-1, nullptr);
    if (c->xq_begun)
        for (int k = 0; k < c->n_local; ++k)
            if (c->ctx[k]) (void)pie_shard_expired_queue_finish(c->ctx[k], nullptr, 0, nullptr);
    c->xq_begun = false;
    if (c->n_local > 0) (void)hipSetDevice(c->device[0]);
    for (void* p : c->xq_retired_dev) (void)hipFree(p);
    for (void* p : c->xq_retired_host) (void)hipHostFree(p);
    c->xq_retired_dev.clear();
    c->xq_retired_host.clear();
    for (void* p : {(void*)c->xq_rows, (void*)c->xq_owner, (void*)c->xq_stage, c->xq_desc})
        if (p) (void)hipFree(p);
    if (c->xq_h) (void)hipHostFree(c->xq_h);
    if (c->xq_ev) (void)hipEventDestroy(c->xq_ev);
    c->xq_rows = c->xq_owner = c->xq_stage = nullptr;
    c->xq_desc = nullptr;
    c->xq_h = nullptr;
    c->xq_ev = nullptr;
    c->xq_room = c->xq_stage_room = 0;
    c->xq_total = -1;
}

} // namespace

extern "C" {

int pie_comm_token_lookup_room(pie_comm* c)
{
    if (!c) return PIE_E_INVAL;
    int room = pie_comm::kLookups - c->lk_n;
    for (int k = 0; k < c->n_local; ++k) room = std::min(room, pie_token_lookup_room(c->ctx[k]));
    return room;
}

int pie_comm_token_lookup_begin(pie_comm* c, const uint64_t* tok, const int64_t* now, size_t k)
{
    if (!c) return PIE_E_INVAL;
    const char* what = "pie_comm_token_lookup_begin";
    // every local shard is asked before any begins
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_token_flight_check(c->ctx[i], what));
    for (int i = 0; i < c->n_local; ++i) {
        const int begun = pie_comm::kLookups - pie_token_lookup_room(c->ctx[i]);
        if (begun != c->lk_n)
            return cfail(c, PIE_E_STATE, "%s: rank %d has %d lookups begun, the communicator %d: pie_shard_token_lookup_* was used on its context directly",
                         what, c->rank_of[i], begun, c->lk_n);
    }
    if (c->lk_n >= pie_comm::kLookups) return cfail(c, PIE_E_STATE, "%s: %d lookups are begun and not finished", what, c->lk_n);
    if (k > 0 && (!tok || !now)) return cfail(c, PIE_E_INVAL, "%s: NULL pointer", what);
    if (k >= ((size_t)1 << 31)) return cfail(c, PIE_E_INVAL, "%s: %zu keys in one lookup", what, k);
    for (int i = 0; i < c->n_local; ++i) {
        const int rc = pie_shard_token_lookup_begin(c->ctx[i], tok, now, k);
        if (rc == PIE_OK) continue;
        cfail(c, rc, "rank %d: %s", c->rank_of[i], pie_last_error(c->ctx[i]));
        for (int j = 0; j < i; ++j) (void)pie_internal::shard_token_flight_drop_last(c->ctx[j], what); // finished and discarded
        return rc;
    }
    c->lk_k[(c->lk_head + c->lk_n) % pie_comm::kLookups] = k;
    c->lk_n++;
    return PIE_OK;
}

int pie_comm_token_lookup_finish(pie_comm* c, int32_t* row_out, uint8_t* live_out, int32_t* user_out, int64_t* start_out, int64_t* end_out,
                                 int32_t* owner_rank_out, size_t cap, size_t* k_out)
{
    if (!c) return PIE_E_INVAL;
    const char* what = "pie_comm_token_lookup_finish";
    if (c->lk_n == 0) return cfail(c, PIE_E_STATE, "%s: no lookup was begun", what);
    const size_t k = c->lk_k[c->lk_head];
    if (k_out) *k_out = k;
    if (cap < k) return cfail(c, PIE_E_CAPACITY, "%s: %zu keys, room for %zu", what, k, cap);
    KeyMerge m{row_out, live_out, user_out, start_out, end_out, owner_rank_out};
    if (!m.alloc(k)) return cfail(c, PIE_E_NOMEM, "%s: no memory for %zu answers", what, k); // nothing consumed
    m.preset(false);
    // the merge pie_comm_token_lookup does; a shard that fails does not keep the others' slots from being returned
    const int rc = wait_and_merge(c, m, shard_lookup_finish);
    c->lk_head = (c->lk_head + 1) % pie_comm::kLookups;
    c->lk_n--;
    return rc;
}

int pie_comm_expired_queue_room(pie_comm* c)
{
    if (!c) return PIE_E_INVAL;
    int room = c->xq_begun ? 0 : 1;
    for (int k = 0; k < c->n_local; ++k) room = std::min(room, pie_expired_queue_room(c->ctx[k]));
    return room;
}

int pie_comm_expired_queue_begin(pie_comm* c, int64_t prev_now, int64_t now, size_t cap_rows)
{
    if (!c) return PIE_E_INVAL;
    const char* what = "pie_comm_expired_queue_begin";
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_expq_check(c->ctx[i], what));
    for (int i = 0; i < c->n_local; ++i)
        if ((pie_expired_queue_room(c->ctx[i]) == 0) != c->xq_begun)
            return cfail(c, PIE_E_STATE, "%s: rank %d %s a queue begun, the communicator %s: pie_shard_expired_queue_* was used on its context directly",
                         what, c->rank_of[i], c->xq_begun ? "has not" : "has", c->xq_begun ? "has" : "has none");
    if (c->xq_begun) return cfail(c, PIE_E_STATE, "%s: an expired queue is begun and not finished", what);
    if (cap_rows >= ((size_t)1 << 31)) return cfail(c, PIE_E_INVAL, "%s: cap_rows %zu", what, cap_rows);
    if (cap_rows > 0) {
        const int rc = xq_ensure(c, cap_rows);
        if (rc) return rc;
    }
    for (int i = 0; i < c->n_local; ++i) {
        const int rc = pie_shard_expired_queue_begin(c->ctx[i], prev_now, now, cap_rows);
        if (rc == PIE_OK) continue;
        cfail(c, rc, "rank %d: %s", c->rank_of[i], pie_last_error(c->ctx[i]));
        for (int j = 0; j < i; ++j) (void)pie_shard_expired_queue_finish(c->ctx[j], nullptr, 0, nullptr); // finished and discarded
        return rc;
    }
    c->xq_cap_rows = cap_rows;
    c->xq_begun = true;
    c->xq_total = -1; // the merged list of the queue before is gone
    c->xq_have = 0;
    return PIE_OK;
}

int pie_comm_expired_queue_finish(pie_comm* c, int32_t* rows_out, int32_t* owner_rank_out, size_t cap, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    const char* what = "pie_comm_expired_queue_finish";
    if (!c->xq_begun) return cfail(c, PIE_E_STATE, "%s: no expired queue was begun", what);
    const size_t cap_rows = c->xq_cap_rows;
    if ((rows_out || owner_rank_out) && cap < cap_rows)
        return cfail(c, PIE_E_INVAL, "%s: room for %zu rows, the begin asked for %zu", what, cap, cap_rows);
    // 1. every shard's bounded wait; its list stays in its own queue buffer
    ShardLists in;
    void* s0 = nullptr;
    int first_rc = PIE_OK, first_bad = -1;
    for (int i = 0; i < c->n_local; ++i) {
        void* s = nullptr;
        const int rc = pie_internal::shard_expq_take(c->ctx[i], what, &in.rows[i], &in.kept[i], &s, &in.done[i]);
        if (rc && first_rc == PIE_OK) { first_rc = rc; first_bad = i; }
        if (i == 0) s0 = s;
    }
    c->xq_begun = false; // consumed on every shard, whatever the waits said
    if (first_rc) return cfail(c, first_rc, "rank %d: %s", c->rank_of[first_bad], pie_last_error(c->ctx[first_bad]));
    size_t total = 0, kept_sum = 0;
    for (int i = 0; i < c->n_local; ++i) {
        total += in.kept[i];
        in.kept[i] = std::min(in.kept[i], cap_rows); // (a shard's list is cut at what the begin asked for)
        kept_sum += in.kept[i];
    }
    if (q_out) *q_out = total;
    const size_t have = std::min(kept_sum, cap_rows);
    if (have > 0) {
        // 2. lists held on other devices come over behind their pass; 3. the merge, on the first shard's pass stream, its descriptor
        // going up from the pinned block
        hipStream_t ms = (hipStream_t)s0;
        PIE_CHIP(c, hipSetDevice(c->device[0]));
        int* h_rows = reinterpret_cast<int*>(c->xq_h + sizeof(MergeDesc));
        int* h_owner = h_rows + c->xq_room;
        hipError_t e = merge_shard_lists(c, in, ms, reinterpret_cast<MergeDesc*>(c->xq_h), c->xq_desc, c->xq_stage, {}, (long long)have, c->xq_rows,
                                         c->xq_owner, nullptr);
        if (e == hipSuccess && rows_out) e = hipMemcpyAsync(h_rows, c->xq_rows, have * 4, hipMemcpyDeviceToHost, ms);
        if (e == hipSuccess && owner_rank_out) e = hipMemcpyAsync(h_owner, c->xq_owner, have * 4, hipMemcpyDeviceToHost, ms);
        if (e == hipSuccess) e = hipEventRecord(c->xq_ev, ms);
        if (e != hipSuccess) {
            pie_internal::shard_expq_stale(c->ctx[0]); // what was queued may still read a shard's buffer: the next begin drains the stream
            return cfail(c, PIE_E_HIP, "%s: %s", what, hipGetErrorString(e));
        }
        const int rc = wait_event(c, 0, c->xq_ev, "in-flight queue merge");
        if (rc) {
            pie_internal::shard_expq_stale(c->ctx[0]);
            return rc;
        }
        if (rows_out) memcpy(rows_out, h_rows, have * 4);
        if (owner_rank_out) memcpy(owner_rank_out, h_owner, have * 4);
    }
    c->xq_total = (long long)total;
    c->xq_have = (long long)have;
    if (cap_rows > 0 && total > cap_rows) return cfail(c, PIE_E_CAPACITY, "%s: %zu rows, the begin asked for %zu", what, total, cap_rows);
    return PIE_OK;
}

int pie_comm_inflight_queue_device_ptrs(pie_comm* c, void** rows_dev, void** owner_rank_dev, size_t* n_out, size_t* q_out)
{
    if (!c) return PIE_E_INVAL;
    if (c->xq_total < 0) return cfail(c, PIE_E_STATE, "no merged in-flight queue: pie_comm_expired_queue_begin / _finish first");
    if (rows_dev) *rows_dev = c->xq_have ? c->xq_rows : nullptr;
    if (owner_rank_dev) *owner_rank_dev = c->xq_have ? c->xq_owner : nullptr;
    if (n_out) *n_out = (size_t)c->xq_have;
    if (q_out) *q_out = (size_t)c->xq_total;
    return PIE_OK;
}

} // extern "C"

// ---- a sharded table that ages: pruneCalendarEvents / purgeExpiredArchives / sessions.delete() (server/storage/sqlProvider.js:
// 956-968, 863-890, 991-1009) behind the communicator.  Every local shard runs its shard form with the list left on its device
// (global rows in the write pass's one store, local rows beside them); the lists are merged on the first local rank's device by
// k_merge_shard_queues<true>, lists held on other devices copied over first.  Nothing is exchanged.
namespace {

int maint_ensure(pie_comm* c, long long total, long long staged_words)
{
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    if (!c->mq_desc) PIE_CHIP(c, hipMalloc(&c->mq_desc, sizeof(MergeDesc)));
    if (total > c->mq_cap) {
        for (int** p : {&c->mq_rows, &c->mq_rank, &c->mq_row})
            if (*p) { PIE_CHIP(c, hipFree(*p)); *p = nullptr; }
        c->mq_cap = 0;
        const long long o = total + total / 16 + 64;
        for (int** p : {&c->mq_rows, &c->mq_rank, &c->mq_row}) PIE_CHIP(c, hipMalloc(p, (size_t)o * 4));
        c->mq_cap = o;
    }
    if (staged_words > c->mq_stage_cap) {
        if (c->mq_stage) { PIE_CHIP(c, hipFree(c->mq_stage)); c->mq_stage = nullptr; }
        c->mq_stage_cap = 0;
        const long long o = staged_words + staged_words / 16 + 64;
        PIE_CHIP(c, hipMalloc(&c->mq_stage, (size_t)o * 4));
        c->mq_stage_cap = o;
    }
    return PIE_OK;
}

// kind 2: prune (a = cutoff), 3: retention under a fixed offset (a = now), 4: under a zone table (a = now)
int comm_maint_list(pie_comm* c, int kind, int64_t a, int32_t months, int64_t tz_offset_ms, const int64_t* transitions, const int64_t* offsets,
                    int32_t n_transitions, int32_t* rows_out, size_t cap, size_t* n_out)
{
    if (!c) return PIE_E_INVAL;
    if (n_out) *n_out = 0;
    if (c->n_local > kMergeMaxLists) return cfail(c, PIE_E_INVAL, "the merge takes at most %d local ranks", kMergeMaxLists);
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i)
        PIE_CCTX(c, i, pie_internal::shard_check_row_list(c->ctx[i], kind, months, tz_offset_ms, transitions, offsets, n_transitions));
    rc = ensure_queue_heads(c); // (the timing events)
    if (rc) return rc;
    c->q_total = -1;
    c->q_kind = PIE_COMM_QUEUE_NONE;
    c->q_timed = false;
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    PIE_CHIP(c, hipEventRecord(c->q_tev[0], c->stream[0]));
    // 1. every shard's two passes; its lists stay in its own workspace
    ShardLists in;
    long long total = 0, staged = 0;
    for (int i = 0; i < c->n_local; ++i) {
        PIE_CCTX(c, i, pie_internal::shard_row_list_run(c->ctx[i], kind, a, months, tz_offset_ms, transitions, offsets, n_transitions, &in.kept[i],
                                                        &in.rows[i], &in.local[i]));
        total += (long long)in.kept[i];
        if (xq_staged(c, i)) staged += 2 * (long long)in.kept[i];
    }
    if (n_out) *n_out = (size_t)total;
    if (total >= 0x7FFFFFFFLL) return cfail(c, PIE_E_INVAL, "a merged list of %lld rows does not fit int32", total);
    PIE_CHIP(c, hipSetDevice(c->device[0]));
    hipStream_t ms = c->stream[0];
    PIE_CHIP(c, hipEventRecord(c->q_tev[1], ms));
    if (total > 0) {
        rc = maint_ensure(c, total, staged);
        if (rc) return rc;
        // 2. lists held on other devices come over (every shard's passes were waited for); 3. the merge.  The descriptor goes up
        // with a copy that waits: no merge of this communicator is running, every call waits for its own
        PIE_CHIP(c, merge_shard_lists(c, in, ms, nullptr, c->mq_desc, c->mq_stage, {c->q_tev[2], c->q_tev[3]}, c->mq_cap, c->mq_rows, c->mq_rank,
                                      c->mq_row));
    } else {
        PIE_CHIP(c, hipEventRecord(c->q_tev[2], ms));
        PIE_CHIP(c, hipEventRecord(c->q_tev[3], ms));
    }
    PIE_CHIP(c, hipEventRecord(c->q_tev[4], ms));
    PIE_CHIP(c, hipEventRecord(c->q_ev[0], ms));
    rc = wait_event(c, 0, c->q_ev[0], "maintenance list merge");
    if (rc) return rc;
    c->q_total = total;
    c->q_kind = PIE_COMM_QUEUE_MAINT;
    c->q_timed = true;
    if (rows_out && (size_t)total > cap) return cfail(c, PIE_E_CAPACITY, "list cap %zu < %lld", cap, total); // tombstoned all the same
    if (rows_out && total) PIE_CHIP(c, hipMemcpy(rows_out, c->mq_rows, (size_t)total * 4, hipMemcpyDeviceToHost));
    return PIE_OK;
}

} // namespace

extern "C" {

int pie_comm_prune_before(pie_comm* c, int64_t cutoff, int32_t* rows_out, size_t cap, size_t* n_out)
{
    return comm_maint_list(c, 2, cutoff, 0, 0, nullptr, nullptr, 0, rows_out, cap, n_out);
}

int pie_comm_retention_purge(pie_comm* c, int64_t now, int32_t months, int64_t tz_offset_ms, int32_t* rows_out, size_t cap, size_t* n_out)
{
    return comm_maint_list(c, 3, now, months, tz_offset_ms, nullptr, nullptr, 0, rows_out, cap, n_out);
}

int pie_comm_retention_purge_tz(pie_comm* c, int64_t now, int32_t months, const int64_t* transitions, const int64_t* offsets, int32_t n_transitions,
                                int32_t* rows_out, size_t cap, size_t* n_out)
{
    return comm_maint_list(c, 4, now, months, 0, transitions, offsets, n_transitions, rows_out, cap, n_out);
}

int pie_comm_compact_rows(pie_comm* c, int64_t dead_before, uint32_t flags, size_t* kept_total_out, size_t* kept_local_out)
{
    if (!c) return PIE_E_INVAL;
    if (kept_total_out) *kept_total_out = 0;
    int rc = mutate_ready(c, nullptr, nullptr);
    if (rc) return rc;
    for (int i = 0; i < c->n_local; ++i) PIE_CCTX(c, i, pie_internal::shard_check_compact(c->ctx[i], flags));
    c->q_total = -1; // a merged queue's source rows name the numbering that goes
    c->q_kind = PIE_COMM_QUEUE_NONE;
    c->q_timed = false;
    size_t total = 0;
    for (int i = 0; i < c->n_local; ++i) {
        size_t kept = 0;
        PIE_CCTX(c, i, pie_compact_rows(c->ctx[i], dead_before, flags, &kept)); // the shards before it stay compacted: global ids do not move
        if (kept_local_out) kept_local_out[i] = kept;
        total += kept;
        if (kept_total_out) *kept_total_out = total;
    }
    return PIE_OK;
}

} // extern "C"
