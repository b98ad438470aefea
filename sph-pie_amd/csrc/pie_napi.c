/*
 * pie_napi.c — raw N-API (no node-addon-api) shim over the C ABI of include/pie_scan.h.
 *
 * The addon holds no logic: it dlopen()s libpie_hip.so and forwards typed-array pointers (zero copy:
 * BigInt64Array for the int64 columns, Int32Array for ids) to the pie_* entry points.  A non-zero status
 * becomes a thrown JS Error carrying `.code` (the PIE_E_* value) and the library's error text — the same
 * shape the route's 500 handler reads (/root/reference/server/index.js:526-536).  All calls are made from
 * the JS main thread; scanAsync() runs the scan on the libuv pool (napi_create_async_work) so a long scan
 * does not block the event loop, one in-flight scan per context: the context handle is marked busy until the worker
 * is done and every other entry point refuses a busy (or destroyed) handle with code PIE_E_STATE.  Output arrays are
 * checked against the lengths the ABI will write (users, users + 1, rows) before any pointer is handed over.
 *
 * Build: gcc -shared -fPIC -I/usr/include/node -Iinclude pie_napi.c -ldl -o host/pie_napi.node
 */
#define NAPI_VERSION 6
#include <node_api.h>

#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pie_scan.h"
#include "pie_nq_ring.h"

/* ---- the C ABI, resolved at open() ------------------------------------------------------------------ */
#define PIE_SYMBOLS(X)                                                                                              \
    X(int, pie_abi_version, (void))                                                                                 \
    X(int, pie_device_count, (void))                                                                                \
    X(int, pie_ctx_create, (int, pie_ctx **))                                                                       \
    X(int, pie_ctx_destroy, (pie_ctx *))                                                                            \
    X(const char *, pie_last_error, (const pie_ctx *))                                                              \
    X(int, pie_load_columns, (pie_ctx *, const int64_t *, const int64_t *, const int32_t *, const int32_t *, size_t, int32_t)) \
    X(int, pie_append_rows, (pie_ctx *, const int64_t *, const int64_t *, const int32_t *, const int32_t *, size_t, int32_t)) \
    X(int, pie_gen_synthetic, (pie_ctx *, uint64_t, int64_t, int64_t, int64_t, int32_t, int32_t, uint32_t))         \
    X(int, pie_read_columns, (pie_ctx *, int64_t *, int64_t *, int32_t *, int32_t *, size_t))                       \
    X(int, pie_set_end, (pie_ctx *, const int32_t *, const int64_t *, size_t))                                      \
    X(int, pie_delete_user, (pie_ctx *, int32_t, int32_t *, size_t, size_t *))                                      \
    X(int, pie_delete_users, (pie_ctx *, const int32_t *, size_t, int32_t *, size_t, size_t *, int32_t *))          \
    X(int, pie_batch_fetch_requests, (pie_ctx *, const int32_t *, const int32_t *, size_t, size_t, int64_t *, int32_t *, int64_t *, int64_t *, int32_t *, size_t *)) \
    X(int, pie_retention_purge_tz, (pie_ctx *, int64_t, int32_t, const int64_t *, const int64_t *, int32_t, int32_t *, size_t, size_t *)) \
    X(int, pie_set_disciplines, (pie_ctx *, uint64_t, int32_t))                                                     \
    X(int, pie_scan, (pie_ctx *, int64_t, int64_t, int32_t *, int64_t *, int32_t *, size_t, size_t *))              \
    X(int, pie_fetch_rows, (pie_ctx *, const int32_t *, size_t, int64_t *, int64_t *, int32_t *, int32_t *))        \
    X(int, pie_save_columns, (pie_ctx *, const char *))                                                             \
    X(int, pie_load_columns_dir, (pie_ctx *, const char *))                                                         \
    X(int, pie_scan_device, (pie_ctx *, int64_t, int64_t, size_t *))                                                \
    X(int, pie_read_user_feed, (pie_ctx *, int32_t, int32_t *, size_t, size_t *))                                   \
    X(int, pie_expired_queue, (pie_ctx *, int64_t, int64_t, int32_t *, size_t, size_t *))                           \
    X(int, pie_archive_queue, (pie_ctx *, int64_t, int64_t, int32_t *, size_t, size_t *))                           \
    X(int, pie_set_profiling, (pie_ctx *, int))                                                                     \
    X(int, pie_set_ordered_run, (pie_ctx *, int))                                                                   \
    X(int, pie_set_wide_ordered, (pie_ctx *, int))                                                                  \
    X(int, pie_set_turn_ordered, (pie_ctx *, int))                                                                  \
    X(int, pie_table_info_get, (pie_ctx *, pie_table_info *))                                                       \
    X(int, pie_set_batch_lanes, (pie_ctx *, int))                                                                   \
    X(int, pie_batch_lanes, (pie_ctx *))                                                                            \
    X(int, pie_stats_get, (pie_ctx *, pie_stats *))                                                                 \
    X(int, pie_stats_reset, (pie_ctx *))                                                                            \
    X(int, pie_scan_batch, (pie_ctx *, const pie_query *, int, size_t *))                                           \
    X(int, pie_scan_wide_begin, (pie_ctx *, const pie_query *, int))                                                \
    X(int, pie_scan_wide_finish, (pie_ctx *, size_t *, size_t, int *))                                              \
    X(int, pie_batch_read_user_feed, (pie_ctx *, int, int32_t, int32_t *, size_t, size_t *))                        \
    X(int, pie_batch_union_wide_device_ptrs, (pie_ctx *, void **, void **, void **, int *, size_t *))               \
    X(int, pie_comm_create, (const int32_t *, int32_t, pie_comm **))                                                \
    X(int, pie_comm_destroy, (pie_comm *))                                                                          \
    X(const char *, pie_comm_last_error, (const pie_comm *))                                                        \
    X(int32_t, pie_comm_world, (const pie_comm *))                                                                  \
    X(pie_ctx *, pie_comm_ctx, (pie_comm *, int32_t))                                                               \
    X(int, pie_comm_gen_synthetic_sharded, (pie_comm *, uint64_t, int64_t, int32_t, int32_t, uint32_t))             \
    X(int, pie_comm_scan_batch_gather, (pie_comm *, const pie_query *, int32_t, int32_t, size_t *))                 \
    X(int, pie_comm_gathered_device_ptr, (pie_comm *, int32_t, void **, size_t *, size_t *, size_t *))              \
    X(int, pie_comm_read_gathered, (pie_comm *, int32_t, int32_t, int32_t, int32_t *, int32_t *, size_t, size_t *))            \
    X(size_t, pie_comm_needed_cap, (const pie_comm *))                                                              \
    X(int, pie_comm_step_reserve, (pie_comm *, int32_t, int32_t, size_t))                                           \
    X(int, pie_comm_step_begin, (pie_comm *, const pie_query *, int32_t))                                           \
    X(int, pie_comm_step_finish, (pie_comm *, size_t *))                                                            \
    X(int, pie_comm_step_collect, (pie_comm *, int64_t *))                                                          \
    X(int, pie_comm_step_gathered_ptr, (pie_comm *, int32_t, int64_t, void **, size_t *, size_t *, size_t *))       \
    X(int, pie_comm_step_read_gathered, (pie_comm *, int32_t, int32_t, int64_t, int32_t *, int32_t *, uint64_t *, size_t, size_t *)) \
    X(int, pie_comm_wide_step_reserve, (pie_comm *, int32_t, int32_t, size_t))                                      \
    X(int, pie_comm_wide_step_begin, (pie_comm *, const pie_query *, int32_t))                                      \
    X(int, pie_comm_wide_step_finish, (pie_comm *, size_t *, size_t))                                               \
    X(int, pie_comm_wide_step_collect, (pie_comm *, int64_t *))                                                     \
    X(int, pie_comm_wide_step_status, (pie_comm *, int64_t, int32_t *))                                             \
    X(int, pie_comm_wide_step_gathered_ptr, (pie_comm *, int32_t, int64_t, void **, size_t *, size_t *, size_t *, int *)) \
    X(int, pie_comm_wide_step_read_gathered, (pie_comm *, int32_t, int32_t, int64_t, int32_t *, int32_t *, uint64_t *, size_t, int *, size_t *)) \
    X(int, pie_comm_expired_queue, (pie_comm *, int64_t, int64_t, int32_t *, size_t, size_t *))                     \
    X(int, pie_comm_archive_queue, (pie_comm *, int64_t, int64_t, int32_t *, size_t, size_t *))                     \
    X(int, pie_comm_queue_read, (pie_comm *, int32_t, int32_t *, int32_t *, int32_t *, size_t, size_t *))            \
    X(int, pie_comm_append_rows, (pie_comm *, const int64_t *, const int64_t *, const int32_t *, const int32_t *, size_t, int32_t, int32_t *)) \
    X(int, pie_comm_set_end, (pie_comm *, const int32_t *, const int64_t *, size_t))                                 \
    X(int, pie_comm_delete_user, (pie_comm *, int32_t, int32_t *, size_t, size_t *, int32_t *))                      \
    X(int, pie_comm_delete_users, (pie_comm *, const int32_t *, size_t, int32_t *, size_t, size_t *, int32_t *, int32_t *)) \
    X(int, pie_comm_table_size, (pie_comm *, int64_t *, int32_t *))                                                  \
    X(int32_t, pie_comm_local_ranks, (const pie_comm *))                                                              \
    X(int, pie_comm_prune_before, (pie_comm *, int64_t, int32_t *, size_t, size_t *))                                \
    X(int, pie_comm_retention_purge_tz, (pie_comm *, int64_t, int32_t, const int64_t *, const int64_t *, int32_t, int32_t *, size_t, size_t *)) \
    X(int, pie_comm_compact_rows, (pie_comm *, int64_t, uint32_t, size_t *, size_t *))                               \
    X(int, pie_shard_maps, (pie_ctx *, int32_t *, int32_t *))                                                       \
    X(int, pie_compact_rows, (pie_ctx *, int64_t, uint32_t, size_t *))                                              \
    X(int, pie_compact_maps, (pie_ctx *, int32_t *, int32_t *, size_t *, size_t *))                                 \
    X(int, pie_compact_map_device_ptrs, (pie_ctx *, void **, void **, size_t *, size_t *))                          \
    X(int, pie_compact_translate, (pie_ctx *, int32_t *, size_t))                                                   \
    X(int, pie_token_set, (pie_ctx *, const uint64_t *, size_t))                                                    \
    X(int, pie_token_append, (pie_ctx *, const uint64_t *, size_t))                                                 \
    X(int, pie_token_lookup, (pie_ctx *, const uint64_t *, size_t, int64_t, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *)) \
    X(int, pie_token_turn, (pie_ctx *, const pie_turn_op *, size_t, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *)) \
    X(int, pie_session_turn, (pie_ctx *, const pie_turn_op *, size_t, const int32_t *, const int32_t *, int32_t, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *)) \
    X(int, pie_comm_token_turn, (pie_comm *, const pie_turn_op *, size_t, int32_t *, uint8_t *, int32_t *, int32_t *, int64_t *, int64_t *)) \
    X(int, pie_comm_session_turn, (pie_comm *, const pie_turn_op *, size_t, const int32_t *, const int32_t *, int32_t, int32_t *, uint8_t *, int32_t *, int32_t *, int64_t *, int64_t *)) \
    X(int, pie_token_set_end, (pie_ctx *, const uint64_t *, const int64_t *, size_t, int64_t, int32_t *))                \
    X(int, pie_token_lookup_begin, (pie_ctx *, const uint64_t *, const int64_t *, size_t))                           \
    X(int, pie_token_lookup_finish, (pie_ctx *, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *, size_t, size_t *)) \
    X(int, pie_token_lookup_room, (pie_ctx *))                                                                       \
    X(int, pie_token_turn_begin, (pie_ctx *, const pie_turn_op *, size_t))                                           \
    X(int, pie_token_turn_finish, (pie_ctx *, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *, size_t, size_t *)) \
    X(int, pie_token_turn_room, (pie_ctx *))                                                                         \
    X(int, pie_expired_queue_begin, (pie_ctx *, int64_t, int64_t, size_t))                                           \
    X(int, pie_expired_queue_finish, (pie_ctx *, int32_t *, size_t, size_t *))                                       \
    X(int, pie_expired_queue_room, (pie_ctx *))                                                                      \
    X(int, pie_scan_batch_begin, (pie_ctx *, const pie_query *, int))                                                \
    X(int, pie_scan_batch_finish, (pie_ctx *, size_t *))                                                             \
    X(int, pie_comm_token_set, (pie_comm *, const uint64_t *, size_t))                                               \
    X(int, pie_comm_token_append, (pie_comm *, const uint64_t *, size_t))                                            \
    X(int, pie_comm_token_lookup, (pie_comm *, const uint64_t *, size_t, int64_t, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *, int32_t *)) \
    X(int, pie_comm_token_set_end, (pie_comm *, const uint64_t *, const int64_t *, size_t, int64_t, int32_t *))                     \
    X(int, pie_comm_token_lookup_begin, (pie_comm *, const uint64_t *, const int64_t *, size_t))                     \
    X(int, pie_comm_token_lookup_finish, (pie_comm *, int32_t *, uint8_t *, int32_t *, int64_t *, int64_t *, int32_t *, size_t, size_t *)) \
    X(int, pie_comm_token_lookup_room, (pie_comm *))                                                                 \
    X(int, pie_comm_expired_queue_begin, (pie_comm *, int64_t, int64_t, size_t))                                     \
    X(int, pie_comm_expired_queue_finish, (pie_comm *, int32_t *, int32_t *, size_t, size_t *))                      \
    X(int, pie_comm_expired_queue_room, (pie_comm *))

#define X(ret, name, args) static ret(*p_##name) args;
PIE_SYMBOLS(X)
#undef X
static void *g_lib;

#define CHECK(env, call)                                                 \
    do {                                                                 \
        if ((call) != napi_ok) {                                         \
            napi_throw_error((env), NULL, "N-API call failed: " #call); \
            return NULL;                                                 \
        }                                                                \
    } while (0)

/* an Error with `text` and a numeric `code`: what every throw, rejection and callback error of this addon is */
static napi_value error_with_code(napi_env env, const char *text, int code)
{
    napi_value msg, err, num;
    napi_create_string_utf8(env, text, NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_create_int32(env, code, &num);
    napi_set_named_property(env, err, "code", num);
    return err;
}

static napi_value throw_pie(napi_env env, pie_ctx *ctx, int rc)
{
    char buf[640];
    snprintf(buf, sizeof buf, "pie_scan error %d: %s", rc, p_pie_last_error ? p_pie_last_error(ctx) : "library not open");
    napi_throw(env, error_with_code(env, buf, rc));
    return NULL;
}

static int need_lib(napi_env env)
{
    if (g_lib) return 1;
    napi_throw_error(env, NULL, "libpie_hip.so is not open: call open(path) first (there is no CPU fallback)");
    return 0;
}

/* Number (integer-valued double, exact to 2^53 — what Date.now() returns) or BigInt -> int64 */
static int get_i64(napi_env env, napi_value v, int64_t *out)
{
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return 0;
    if (t == napi_bigint) {
        bool lossless;
        return napi_get_value_bigint_int64(env, v, out, &lossless) == napi_ok;
    }
    if (t == napi_number) {
        double d;
        if (napi_get_value_double(env, v, &d) != napi_ok) return 0;
        if (!(d == d) || d > 9.2e18 || d < -9.2e18) return 0; /* NaN / out of range: Number.isFinite guard */
        *out = (int64_t)d;
        return 1;
    }
    return 0;
}

static void *typed(napi_env env, napi_value v, napi_typedarray_type want, size_t *len)
{
    bool is = false;
    napi_typedarray_type t;
    void *data = NULL;
    size_t n = 0;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) return NULL;
    if (napi_get_typedarray_info(env, v, &t, &n, &data, NULL, NULL) != napi_ok || t != want) return NULL;
    if (len) *len = n;
    return data ? data : (void *)(uintptr_t)16; /* zero-length arrays may report NULL */
}

/* What a JS context handle points at.  The header asks for one thread per context: while scanAsync() runs a scan on the
 * libuv pool the box is `busy` and every other entry point refuses it (PIE_E_STATE) instead of racing the worker on the
 * context's state; after ctxDestroy the box stays (the external keeps pointing at it) with ctx = NULL, so a stale handle
 * throws instead of touching freed memory.  `owned` = 0: the context belongs to a communicator (commCtx). */
struct comm_box_s;
typedef struct ctx_box_s {
    pie_ctx *ctx;
    int busy;
    int owned;
    /* a context handed out by commCtx: it lives inside its communicator.  The box holds a reference on the communicator's
     * JS handle (the communicator cannot be collected while a context handle is alive) and sits on the communicator's list,
     * so commDestroy can clear box->ctx: a stale handle then throws PIE_E_STATE like a destroyed context. */
    struct comm_box_s *parent;
    struct ctx_box_s *next;
    napi_ref comm_ref;
    /* what this handle has begun and not finished: the keys of every token lookup (tokenLookupBegin), oldest first, and the
     * queries of every batch (scanBatchBegin) — the sizes of the arrays their finish hands out */
    size_t lk_k[4];
    int lk_head, lk_n;
    int bt_q[16];
    int bt_head, bt_n;
    /* ... and the ops of every turn begun beside them (tokenTurnBegin), oldest first */
    size_t tn_k[4];
    int tn_head, tn_n;
    /* the expired queue begun beside them (expiredQueueBegin): the rows its finish has to make room for */
    size_t eq_cap;
    int eq_begun;
} ctx_box;

static void comm_unlink_ctx(ctx_box *b);

static void box_finalize(napi_env env, void *data, void *hint)
{
    (void)hint;
    ctx_box *b = (ctx_box *)data;
    if (b && b->ctx && b->owned && !b->busy && p_pie_ctx_destroy) p_pie_ctx_destroy(b->ctx);
    if (b) {
        comm_unlink_ctx(b);
        if (b->comm_ref) napi_delete_reference(env, b->comm_ref);
    }
    free(b);
}

static napi_value throw_state(napi_env env, const char *text)
{
    napi_throw(env, error_with_code(env, text, PIE_E_STATE));
    return NULL;
}

static ctx_box *get_box(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "expected a pie context");
        return NULL;
    }
    return (ctx_box *)p;
}

static pie_ctx *get_ctx(napi_env env, napi_value v)
{
    ctx_box *b = get_box(env, v);
    if (!b) return NULL;
    if (!b->ctx) {
        throw_state(env, "pie_scan error -6: this context was destroyed");
        return NULL;
    }
    if (b->busy) {
        throw_state(env, "pie_scan error -6: an asynchronous scan is in flight on this context (one thread per context)");
        return NULL;
    }
    return b->ctx;
}

/* rows / users of the resident table, for the length checks of caller-supplied output arrays */
static int table_shape(pie_ctx *ctx, size_t *rows, size_t *users)
{
    pie_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_pie_stats_get(ctx, &st);
    if (rc) return rc;
    *rows = (size_t)st.rows;
    *users = (size_t)st.users;
    return 0;
}

#define ARGS(n)                                                          \
    size_t argc = (n);                                                   \
    napi_value argv[(n)];                                                \
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));    \
    if (argc < (n)) {                                                    \
        napi_throw_type_error(env, NULL, "too few arguments");           \
        return NULL;                                                     \
    }

static napi_value js_int(napi_env env, int64_t v)
{
    napi_value out;
    napi_create_int64(env, v, &out);
    return out;
}

/* ---- open(path) -------------------------------------------------------------------------------------- */
static napi_value fn_open(napi_env env, napi_callback_info info)
{
    ARGS(1)
    char path[4096];
    size_t n = 0;
    CHECK(env, napi_get_value_string_utf8(env, argv[0], path, sizeof path, &n));
    if (!g_lib) {
        void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
        if (!lib) {
            char buf[4400];
            snprintf(buf, sizeof buf, "cannot load %s: %s (build it first; there is no CPU fallback)", path, dlerror());
            napi_throw_error(env, NULL, buf);
            return NULL;
        }
#define X(ret, name, args)                                                        \
    p_##name = (ret(*) args)dlsym(lib, #name);                                    \
    if (!p_##name) {                                                              \
        napi_throw_error(env, NULL, "libpie_hip.so lacks symbol " #name);         \
        dlclose(lib);                                                             \
        return NULL;                                                              \
    }
        PIE_SYMBOLS(X)
#undef X
        g_lib = lib;
    }
    return js_int(env, p_pie_abi_version());
}

static napi_value fn_device_count(napi_env env, napi_callback_info info)
{
    (void)info;
    if (!need_lib(env)) return NULL;
    return js_int(env, p_pie_device_count());
}

static napi_value fn_ctx_create(napi_env env, napi_callback_info info)
{
    ARGS(1)
    if (!need_lib(env)) return NULL;
    int32_t dev = 0;
    CHECK(env, napi_get_value_int32(env, argv[0], &dev));
    pie_ctx *ctx = NULL;
    int rc = p_pie_ctx_create(dev, &ctx);
    if (rc) return throw_pie(env, NULL, rc);
    ctx_box *b = (ctx_box *)calloc(1, sizeof *b);
    if (!b) {
        p_pie_ctx_destroy(ctx);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    b->ctx = ctx;
    b->owned = 1;
    napi_value ext;
    if (napi_create_external(env, b, box_finalize, NULL, &ext) != napi_ok) {
        p_pie_ctx_destroy(ctx);
        free(b);
        napi_throw_error(env, NULL, "N-API call failed: napi_create_external");
        return NULL;
    }
    return ext;
}

static napi_value fn_ctx_destroy(napi_env env, napi_callback_info info)
{
    ARGS(1)
    ctx_box *b = get_box(env, argv[0]);
    if (!b) return NULL;
    if (b->busy) return throw_state(env, "pie_scan error -6: an asynchronous scan is in flight on this context");
    if (b->ctx && b->owned) p_pie_ctx_destroy(b->ctx);
    b->ctx = NULL; /* the handle stays valid as an object and throws on any further use */
    return js_int(env, 0);
}

/* loadColumns(ctx, start, end, user, disc, nUsers) / appendRows(...) */
static napi_value load_or_append(napi_env env, napi_callback_info info, int append)
{
    ARGS(6)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t n0, n1, n2, n3;
    int64_t *s = typed(env, argv[1], napi_bigint64_array, &n0), *e = typed(env, argv[2], napi_bigint64_array, &n1);
    int32_t *u = typed(env, argv[3], napi_int32_array, &n2), *d = typed(env, argv[4], napi_int32_array, &n3);
    int32_t n_users = 0;
    if (!s || !e || !u || !d || n0 != n1 || n0 != n2 || n0 != n3) {
        napi_throw_type_error(env, NULL, "columns must be BigInt64Array, BigInt64Array, Int32Array, Int32Array of equal length");
        return NULL;
    }
    CHECK(env, napi_get_value_int32(env, argv[5], &n_users));
    int rc = append ? p_pie_append_rows(ctx, s, e, u, d, n0, n_users) : p_pie_load_columns(ctx, s, e, u, d, n0, n_users);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)n0);
}
static napi_value fn_load_columns(napi_env env, napi_callback_info info) { return load_or_append(env, info, 0); }
static napi_value fn_append_rows(napi_env env, napi_callback_info info) { return load_or_append(env, info, 1); }

/* genSynthetic(ctx, seed(BigInt|Number), nTotal, row0, n, nUsers, nDisc, flags) */
static napi_value fn_gen(napi_env env, napi_callback_info info)
{
    ARGS(8)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t seed, n_total, row0, n;
    int32_t n_users, n_disc, flags;
    if (!get_i64(env, argv[1], &seed) || !get_i64(env, argv[2], &n_total) || !get_i64(env, argv[3], &row0) ||
        !get_i64(env, argv[4], &n)) {
        napi_throw_type_error(env, NULL, "bad integer argument");
        return NULL;
    }
    CHECK(env, napi_get_value_int32(env, argv[5], &n_users));
    CHECK(env, napi_get_value_int32(env, argv[6], &n_disc));
    CHECK(env, napi_get_value_int32(env, argv[7], &flags));
    int rc = p_pie_gen_synthetic(ctx, (uint64_t)seed, n_total, row0, n, n_users, n_disc, (uint32_t)flags);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, n);
}

/* readColumns(ctx, start, end, user, disc) */
static napi_value fn_read_columns(napi_env env, napi_callback_info info)
{
    ARGS(5)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t n = 0, n1 = 0, n2 = 0, n3 = 0;
    int64_t *s = typed(env, argv[1], napi_bigint64_array, &n), *e = typed(env, argv[2], napi_bigint64_array, &n1);
    int32_t *u = typed(env, argv[3], napi_int32_array, &n2), *d = typed(env, argv[4], napi_int32_array, &n3);
    if (!s || !e || !u || !d || n1 < n || n2 < n || n3 < n) {
        napi_throw_type_error(env, NULL, "readColumns(ctx, BigInt64Array, BigInt64Array, Int32Array, Int32Array): every array at least as long as the first");
        return NULL;
    }
    int rc = p_pie_read_columns(ctx, s, e, u, d, n);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)n);
}

/* saveColumns(ctx, dir) / loadColumnsDir(ctx, dir) -> {rows, users}: the flat column files of pie_save_columns */
static napi_value dir_call(napi_env env, napi_callback_info info, int load)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    char dir[4096];
    size_t len = 0;
    if (napi_get_value_string_utf8(env, argv[1], dir, sizeof dir, &len) != napi_ok || len == 0 || len >= sizeof dir - 1) {
        napi_throw_type_error(env, NULL, "directory path expected");
        return NULL;
    }
    int rc = load ? p_pie_load_columns_dir(ctx, dir) : p_pie_save_columns(ctx, dir);
    if (rc) return throw_pie(env, ctx, rc);
    pie_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    rc = p_pie_stats_get(ctx, &st);
    if (rc) return throw_pie(env, ctx, rc);
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    napi_set_named_property(env, out, "rows", js_int(env, (int64_t)st.rows));
    napi_set_named_property(env, out, "users", js_int(env, (int64_t)st.users));
    return out;
}
static napi_value fn_save_columns(napi_env env, napi_callback_info info) { return dir_call(env, info, 0); }
static napi_value fn_load_columns_dir(napi_env env, napi_callback_info info) { return dir_call(env, info, 1); }

/* setEnd(ctx, rows Int32Array, newEnd BigInt64Array) */
static napi_value fn_set_end(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0, k2 = 0;
    int32_t *rows = typed(env, argv[1], napi_int32_array, &k);
    int64_t *ne = typed(env, argv[2], napi_bigint64_array, &k2);
    if (!rows || !ne || k != k2) {
        napi_throw_type_error(env, NULL, "setEnd(ctx, Int32Array rows, BigInt64Array newEnd)");
        return NULL;
    }
    int rc = p_pie_set_end(ctx, rows, ne, k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* compactRows(ctx, deadBefore BigInt|Number, shrink) -> rows kept: drop the rows with end <= deadBefore, order preserved
 * (pie_compact_rows; the device's counterpart of sessions.delete(), sessionStore.js:47-53,66-73) */
static napi_value fn_compact_rows(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t dead_before = 0;
    bool shrink = false;
    size_t kept = 0;
    if (!get_i64(env, argv[1], &dead_before)) {
        napi_throw_type_error(env, NULL, "compactRows(ctx, deadBefore BigInt|Number, shrink)");
        return NULL;
    }
    CHECK(env, napi_get_value_bool(env, argv[2], &shrink));
    int rc = p_pie_compact_rows(ctx, dead_before, shrink ? PIE_COMPACT_SHRINK : 0u, &kept);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)kept);
}

/* compactMaps(ctx, newOfOldOut Int32Array|null, oldOfNewOut Int32Array|null) -> {nOld, nKept}; an array given is filled and must
 * be long enough (call with nulls first to learn the sizes) */
static napi_value fn_compact_maps(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t n_old = 0, n_kept = 0, cap_new = 0, cap_old = 0;
    int rc = p_pie_compact_map_device_ptrs(ctx, NULL, NULL, &n_old, &n_kept);
    if (rc) return throw_pie(env, ctx, rc);
    napi_valuetype t0, t1;
    CHECK(env, napi_typeof(env, argv[1], &t0));
    CHECK(env, napi_typeof(env, argv[2], &t1));
    int32_t *m_new = (t0 == napi_null || t0 == napi_undefined) ? NULL : typed(env, argv[1], napi_int32_array, &cap_new);
    int32_t *m_old = (t1 == napi_null || t1 == napi_undefined) ? NULL : typed(env, argv[2], napi_int32_array, &cap_old);
    if ((t0 != napi_null && t0 != napi_undefined && (!m_new || cap_new < n_old)) ||
        (t1 != napi_null && t1 != napi_undefined && (!m_old || cap_old < n_kept))) {
        napi_throw_type_error(env, NULL, "compactMaps(ctx, Int32Array[nOld]|null, Int32Array[nKept]|null)");
        return NULL;
    }
    if (m_new || m_old) {
        rc = p_pie_compact_maps(ctx, m_new, m_old, NULL, NULL);
        if (rc) return throw_pie(env, ctx, rc);
    }
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    CHECK(env, napi_set_named_property(env, out, "nOld", js_int(env, (int64_t)n_old)));
    CHECK(env, napi_set_named_property(env, out, "nKept", js_int(env, (int64_t)n_kept)));
    return out;
}

/* compactTranslate(ctx, rows Int32Array) -> its length; old row indices rewritten in place to the new ones (-1: dropped) */
static napi_value fn_compact_translate(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0;
    int32_t *rows = typed(env, argv[1], napi_int32_array, &k);
    if (!rows && k) {
        napi_throw_type_error(env, NULL, "compactTranslate(ctx, Int32Array rows)");
        return NULL;
    }
    int rc = k ? p_pie_compact_translate(ctx, rows, k) : 0;
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* deleteUser(ctx, user, rowsOut Int32Array) -> number of rows tombstoned (rowsOut holds them, ascending) */
static napi_value fn_delete_user(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t user = -1;
    size_t cap = 0, k = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &user));
    int32_t *rows = typed(env, argv[2], napi_int32_array, &cap);
    if (!rows) {
        napi_throw_type_error(env, NULL, "deleteUser(ctx, user, Int32Array rowsOut)");
        return NULL;
    }
    int rc = p_pie_delete_user(ctx, user, rows, cap, &k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* deleteUsers(ctx, users Int32Array, rowsOut Int32Array[, perUser Int32Array]) -> number of rows tombstoned for the whole set in
 * one call (rowsOut holds them, ascending; perUser[i], as long as users, the rows of users[i]: a repeated id counts once) */
static napi_value fn_delete_users(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) {
        napi_throw_type_error(env, NULL, "too few arguments");
        return NULL;
    }
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t n = 0, cap = 0, np = 0, k = 0;
    int32_t *users = typed(env, argv[1], napi_int32_array, &n);
    int32_t *rows = typed(env, argv[2], napi_int32_array, &cap);
    int32_t *per = argc > 3 ? typed(env, argv[3], napi_int32_array, &np) : NULL;
    bool users_typed = false;
    if (napi_is_typedarray(env, argv[1], &users_typed) != napi_ok) users_typed = false;
    if (!users_typed || (!users && n) || !rows || (argc > 3 && n && (!per || np != n))) {
        napi_throw_type_error(env, NULL, "deleteUsers(ctx, Int32Array users, Int32Array rowsOut[, Int32Array perUser])");
        return NULL;
    }
    int rc = n ? p_pie_delete_users(ctx, users, n, rows, cap, &k, per) : 0;
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* retentionPurgeTz(ctx, now, months, transitions BigInt64Array[n], offsets BigInt64Array[n + 1], rowsOut Int32Array) -> rows
 * tombstoned (rowsOut holds them, ascending): now >= addMonths(start, months) with `setMonth` on a LOCAL Date under the zone the
 * table describes (host/tzTable.js builds it from this process's zone rules); sqlProvider.js:863-890,991-1009 */
static napi_value fn_retention_purge_tz(napi_env env, napi_callback_info info)
{
    ARGS(6)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t now = 0;
    int32_t months = 0;
    size_t nt = 0, no = 0, cap = 0, k = 0;
    CHECK(env, napi_get_value_int64(env, argv[1], &now));
    CHECK(env, napi_get_value_int32(env, argv[2], &months));
    int64_t *tr = typed(env, argv[3], napi_bigint64_array, &nt), *off = typed(env, argv[4], napi_bigint64_array, &no);
    int32_t *rows = typed(env, argv[5], napi_int32_array, &cap);
    if (!tr || !off || !rows || no != nt + 1) {
        napi_throw_type_error(env, NULL, "retentionPurgeTz(ctx, now, months, BigInt64Array transitions[n], BigInt64Array offsets[n + 1], Int32Array rowsOut)");
        return NULL;
    }
    int rc = p_pie_retention_purge_tz(ctx, now, months, tr, off, (int32_t)nt, rows, cap, &k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* batchFetchRequests(ctx, qi Int32Array[n], users Int32Array[n], off BigInt64Array[n + 1], idx Int32Array[cap], start BigInt64Array[cap],
 * end BigInt64Array[cap], disc Int32Array[cap]) -> total rows: the feeds of n (query, user) requests of the last batch in one call;
 * request i's rows are idx[off[i] .. off[i + 1]) with their columns.  Throws code -5 when cap is too small. */
static napi_value fn_batch_fetch_requests(napi_env env, napi_callback_info info)
{
    ARGS(8)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t nq = 0, nu = 0, no = 0, ci = 0, cs = 0, ce = 0, cd = 0, total = 0;
    int32_t *qi = typed(env, argv[1], napi_int32_array, &nq), *us = typed(env, argv[2], napi_int32_array, &nu);
    int64_t *off = typed(env, argv[3], napi_bigint64_array, &no);
    int32_t *idx = typed(env, argv[4], napi_int32_array, &ci);
    int64_t *st = typed(env, argv[5], napi_bigint64_array, &cs), *en = typed(env, argv[6], napi_bigint64_array, &ce);
    int32_t *di = typed(env, argv[7], napi_int32_array, &cd);
    if (!qi || !us || !off || !idx || !st || !en || !di || nq != nu || no < nq + 1 || cs < ci || ce < ci || cd < ci) {
        napi_throw_type_error(env, NULL, "batchFetchRequests(ctx, Int32Array qi[n], Int32Array users[n], BigInt64Array off[n + 1], Int32Array idx[cap], BigInt64Array start[cap], BigInt64Array end[cap], Int32Array disc[cap])");
        return NULL;
    }
    int rc = p_pie_batch_fetch_requests(ctx, qi, us, nq, ci, off, idx, st, en, di, &total);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)total);
}

/* setDisciplines(ctx, mask BigInt|Number, nDisc) */
static napi_value fn_set_disc(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    uint64_t mask = 0;
    napi_valuetype t;
    napi_typeof(env, argv[1], &t);
    if (t == napi_bigint) {
        bool lossless;
        CHECK(env, napi_get_value_bigint_uint64(env, argv[1], &mask, &lossless));
    } else {
        int64_t v;
        if (!get_i64(env, argv[1], &v)) {
            napi_throw_type_error(env, NULL, "mask must be a BigInt or an integer Number");
            return NULL;
        }
        mask = (uint64_t)v;
    }
    int32_t n_disc;
    CHECK(env, napi_get_value_int32(env, argv[2], &n_disc));
    int rc = p_pie_set_disciplines(ctx, mask, n_disc);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, 0);
}

/* scan(ctx, now, cutoff, counts Int32Array[U], offsets BigInt64Array[U+1], idx Int32Array[cap]) -> M */
static napi_value fn_scan(napi_env env, napi_callback_info info)
{
    ARGS(6)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t now, cutoff;
    if (!get_i64(env, argv[1], &now) || !get_i64(env, argv[2], &cutoff)) {
        napi_throw_type_error(env, NULL, "now / cutoff must be finite integers (Number or BigInt)");
        return NULL;
    }
    size_t cap = 0, nc = 0, no = 0, rows = 0, users = 0;
    int32_t *counts = typed(env, argv[3], napi_int32_array, &nc);
    int64_t *offsets = typed(env, argv[4], napi_bigint64_array, &no);
    int32_t *idx = typed(env, argv[5], napi_int32_array, &cap);
    int rc = table_shape(ctx, &rows, &users);
    if (rc) return throw_pie(env, ctx, rc);
    if (!counts || !offsets || !idx || nc < users || no < users + 1) { /* the ABI writes counts[U] and offsets[U + 1] */
        napi_throw_type_error(env, NULL, "scan(ctx, now, cutoff, Int32Array[>= users], BigInt64Array[>= users + 1], Int32Array)");
        return NULL;
    }
    size_t m = 0;
    rc = p_pie_scan(ctx, now, cutoff, counts, offsets, idx, cap, &m);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)m);
}

/* scanDevice(ctx, now, cutoff) -> M: the scan with its result left in HBM (read a user's slice with userFeed) */
static napi_value fn_scan_device(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t now, cutoff;
    if (!get_i64(env, argv[1], &now) || !get_i64(env, argv[2], &cutoff)) {
        napi_throw_type_error(env, NULL, "now / cutoff must be finite integers (Number or BigInt)");
        return NULL;
    }
    size_t m = 0;
    int rc = p_pie_scan_device(ctx, now, cutoff, &m);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)m);
}

/* userFeed(ctx, user, idx Int32Array) -> k: rows of that user's feed in the last scan, written to idx[0..k) */
static napi_value fn_user_feed(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t user = 0;
    size_t cap = 0;
    int32_t *idx = typed(env, argv[2], napi_int32_array, &cap);
    if (!get_i64(env, argv[1], &user) || !idx || user < INT32_MIN || user > INT32_MAX) {
        napi_throw_type_error(env, NULL, "userFeed(ctx, user, Int32Array)");
        return NULL;
    }
    size_t k = 0;
    int rc = p_pie_read_user_feed(ctx, (int32_t)user, idx, cap, &k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* A job on the libuv pool: the handle is busy from here until the job's `done` runs on the main thread.  0: nothing was queued
 * and an error is thrown (the caller frees its job). */
static int queue_promise_job(napi_env env, ctx_box *b, const char *name, napi_async_execute_callback exec,
                             napi_async_complete_callback done, void *job, napi_async_work *work)
{
    napi_value res;
    napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &res);
    b->busy = 1;
    if (napi_create_async_work(env, NULL, res, exec, done, job, work) == napi_ok && napi_queue_async_work(env, *work) == napi_ok) return 1;
    b->busy = 0;
    napi_throw_error(env, NULL, "cannot queue async work");
    return 0;
}

/* The rejection of such a job's promise: an Error with `text`, `code` (PIE_E_STATE for a job that was cancelled: rc 0) and, when
 * the result outgrew its room (PIE_E_CAPACITY, length >= 0), the true `length`. */
static void reject_with_code(napi_env env, napi_deferred deferred, int rc, const char *text, int64_t length)
{
    napi_value err = error_with_code(env, text, rc ? rc : PIE_E_STATE), len;
    if (rc == PIE_E_CAPACITY && length >= 0) {
        napi_create_int64(env, length, &len);
        napi_set_named_property(env, err, "length", len);
    }
    napi_reject_deferred(env, deferred, err);
}

/* scanAsync(ctx, now, cutoff, counts, offsets, idx, callback(err, m)) — same scan on the libuv pool */
typedef struct {
    napi_async_work work;
    napi_ref cb, keep[3];
    pie_ctx *ctx;
    ctx_box *box;
    int64_t now, cutoff;
    int32_t *counts, *idx;
    int64_t *offsets;
    size_t cap, m;
    int rc;
    char err[600];
} scan_job;

static void scan_exec(napi_env env, void *data)
{
    (void)env;
    scan_job *j = (scan_job *)data;
    j->rc = p_pie_scan(j->ctx, j->now, j->cutoff, j->counts, j->offsets, j->idx, j->cap, &j->m);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_scan error %d: %s", j->rc, p_pie_last_error(j->ctx));
}

static void scan_done(napi_env env, napi_status status, void *data)
{
    scan_job *j = (scan_job *)data;
    napi_value cb, global, args[2], res;
    j->box->busy = 0; /* the worker is done with the context: the main thread may use it again */
    napi_get_reference_value(env, j->cb, &cb);
    napi_get_global(env, &global);
    if (status != napi_ok || j->rc) {
        args[0] = error_with_code(env, j->rc ? j->err : "scan cancelled", j->rc);
        napi_get_undefined(env, &args[1]);
    } else {
        napi_get_null(env, &args[0]);
        napi_create_int64(env, (int64_t)j->m, &args[1]);
    }
    napi_call_function(env, global, cb, 2, args, &res);
    napi_delete_reference(env, j->cb);
    for (int i = 0; i < 3; ++i) napi_delete_reference(env, j->keep[i]);
    napi_delete_async_work(env, j->work);
    free(j);
}

static napi_value fn_scan_async(napi_env env, napi_callback_info info)
{
    ARGS(7)
    pie_ctx *ctx = get_ctx(env, argv[0]); /* refuses a context that is already busy */
    if (!ctx) return NULL;
    size_t nc = 0, no = 0, rows = 0, users = 0;
    int rc0 = table_shape(ctx, &rows, &users);
    if (rc0) return throw_pie(env, ctx, rc0);
    scan_job *j = (scan_job *)calloc(1, sizeof *j);
    if (!j) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    j->ctx = ctx;
    j->box = get_box(env, argv[0]);
    j->counts = typed(env, argv[3], napi_int32_array, &nc);
    j->offsets = typed(env, argv[4], napi_bigint64_array, &no);
    j->idx = typed(env, argv[5], napi_int32_array, &j->cap);
    if (!get_i64(env, argv[1], &j->now) || !get_i64(env, argv[2], &j->cutoff) || !j->counts || !j->offsets || !j->idx ||
        nc < users || no < users + 1) {
        free(j);
        napi_throw_type_error(env, NULL, "scanAsync(ctx, now, cutoff, Int32Array[>= users], BigInt64Array[>= users + 1], Int32Array, cb)");
        return NULL;
    }
    napi_create_reference(env, argv[6], 1, &j->cb);
    for (int i = 0; i < 3; ++i) napi_create_reference(env, argv[3 + i], 1, &j->keep[i]); /* keep buffers alive */
    if (!queue_promise_job(env, j->box, "pie_scan", scan_exec, scan_done, j, &j->work)) { /* its callback stands in for the promise */
        free(j);
        return NULL;
    }
    return js_int(env, 0);
}

/* fetchRows(ctx, idx Int32Array, m, start, end, user, disc) */
static napi_value fn_fetch_rows(napi_env env, napi_callback_info info)
{
    ARGS(7)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t cap = 0, c1 = 0;
    int32_t *idx = typed(env, argv[1], napi_int32_array, &cap);
    int64_t m = 0;
    if (!idx || !get_i64(env, argv[2], &m) || m < 0 || (size_t)m > cap) {
        napi_throw_type_error(env, NULL, "fetchRows(ctx, Int32Array idx, m <= idx.length, ...)");
        return NULL;
    }
    size_t c2 = 0, c3 = 0, c4 = 0;
    int64_t *s = typed(env, argv[3], napi_bigint64_array, &c1), *e = typed(env, argv[4], napi_bigint64_array, &c2);
    int32_t *u = typed(env, argv[5], napi_int32_array, &c3), *d = typed(env, argv[6], napi_int32_array, &c4);
    if (!s || !e || !u || !d || c1 < (size_t)m || c2 < (size_t)m || c3 < (size_t)m || c4 < (size_t)m) {
        napi_throw_type_error(env, NULL, "bad output arrays");
        return NULL;
    }
    int rc = p_pie_fetch_rows(ctx, idx, (size_t)m, s, e, u, d);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, m);
}

/* expiredQueue(ctx, prevNow, now, queue Int32Array) -> q */
static napi_value fn_expired_queue(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t prev, now;
    size_t cap = 0, q = 0;
    int32_t *queue = typed(env, argv[3], napi_int32_array, &cap);
    if (!get_i64(env, argv[1], &prev) || !get_i64(env, argv[2], &now) || !queue) {
        napi_throw_type_error(env, NULL, "expiredQueue(ctx, prevNow, now, Int32Array)");
        return NULL;
    }
    int rc = p_pie_expired_queue(ctx, prev, now, queue, cap, &q);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)q);
}

/* archiveQueue(ctx, now, windowMs, queue Int32Array) -> q */
static napi_value fn_archive_queue(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int64_t now, window;
    size_t cap = 0, q = 0;
    int32_t *queue = typed(env, argv[3], napi_int32_array, &cap);
    if (!get_i64(env, argv[1], &now) || !get_i64(env, argv[2], &window) || !queue) {
        napi_throw_type_error(env, NULL, "archiveQueue(ctx, now, windowMs, Int32Array)");
        return NULL;
    }
    int rc = p_pie_archive_queue(ctx, now, window, queue, cap, &q);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)q);
}

/* ---- native feed serialiser ---------------------------------------------------------------
 * serializeEvents(idx Int32Array, m, start BigInt64Array, end BigInt64Array, disc Int32Array, perDisc Array) -> Buffer
 * holding exactly the bytes of JSON.stringify({events: rows.map(eventFromRow)}) for the event shape of
 * /root/reference/server/calendarFeed.js:66-79 as host/calendarFeed.js builds it from session rows.  perDisc[d] =
 * [titlePrefixJson (no quotes, already escaped), eventNameJson, colorJson] — the per-discipline constants are computed
 * once in JS (parseCalendarMetadata), the per-row work (numbers, ISO dates, allDay) happens here.  Returns null when a
 * row needs something this fast path does not cover (year outside 0000..9999, discipline outside the table): the
 * caller then uses the JS path. */
typedef struct { char *p; size_t len, cap; } sbuf;
static int sb_need(sbuf *b, size_t extra)
{
    if (b->len + extra <= b->cap) return 1;
    size_t nc = b->cap ? b->cap * 2 : 4096;
    while (nc < b->len + extra) nc *= 2;
    char *np = (char *)realloc(b->p, nc);
    if (!np) return 0;
    b->p = np;
    b->cap = nc;
    return 1;
}
static int sb_put(sbuf *b, const char *s, size_t n)
{
    if (!sb_need(b, n)) return 0;
    memcpy(b->p + b->len, s, n);
    b->len += n;
    return 1;
}
#define SB_LIT(b, lit) sb_put((b), (lit), sizeof(lit) - 1)
static int sb_i64(sbuf *b, int64_t v)
{
    char tmp[24];
    int pos = 24;
    uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
    do { tmp[--pos] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) tmp[--pos] = '-';
    return sb_put(b, tmp + pos, (size_t)(24 - pos));
}
/* ms since epoch -> "YYYY-MM-DDTHH:mm:ss.sssZ"; returns 0 when the year is outside 0000..9999; *h / *mi = UTC hour, minute */
static int iso_utc(int64_t ms, char out[25], int *h, int *mi)
{
    int64_t days = ms / 86400000, rem = ms % 86400000;
    if (rem < 0) { rem += 86400000; days -= 1; }
    int64_t z = days + 719468;
    const int64_t era = (z >= 0 ? z : z - 146096) / 146097;
    const int64_t doe = z - era * 146097;
    const int64_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;
    const int64_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);
    const int64_t mp = (5 * doy + 2) / 153;
    const int64_t d = doy - (153 * mp + 2) / 5 + 1;
    const int64_t m = mp < 10 ? mp + 3 : mp - 9;
    const int64_t y = yoe + era * 400 + (m <= 2 ? 1 : 0);
    if (y < 0 || y > 9999) return 0;
    *h = (int)(rem / 3600000);
    *mi = (int)(rem / 60000 % 60);
    const int sec = (int)(rem / 1000 % 60), msec = (int)(rem % 1000), yy = (int)y;
#define D2(pos, v) (out[pos] = (char)('0' + (v) / 10), out[(pos) + 1] = (char)('0' + (v) % 10))
    D2(0, yy / 100); D2(2, yy % 100); out[4] = '-'; D2(5, (int)m); out[7] = '-'; D2(8, (int)d); out[10] = 'T';
    D2(11, *h); out[13] = ':'; D2(14, *mi); out[16] = ':'; D2(17, sec); out[19] = '.';
    out[20] = (char)('0' + msec / 100); D2(21, msec % 100); out[23] = 'Z'; out[24] = 0;
#undef D2
    return 1;
}

static napi_value fn_serialize_events(napi_env env, napi_callback_info info)
{
    ARGS(6)
    size_t cap = 0, n1 = 0, n2 = 0, n3 = 0;
    int32_t *idx = typed(env, argv[0], napi_int32_array, &cap);
    int64_t m = 0;
    int64_t *start = typed(env, argv[2], napi_bigint64_array, &n1), *end = typed(env, argv[3], napi_bigint64_array, &n2);
    int32_t *disc = typed(env, argv[4], napi_int32_array, &n3);
    uint32_t n_disc = 0;
    if (!idx || !get_i64(env, argv[1], &m) || m < 0 || (size_t)m > cap || !start || !end || !disc || n1 < (size_t)m ||
        n2 < (size_t)m || n3 < (size_t)m || napi_get_array_length(env, argv[5], &n_disc) != napi_ok || n_disc > 64) {
        napi_throw_type_error(env, NULL, "serializeEvents(Int32Array idx, m, BigInt64Array start, BigInt64Array end, Int32Array disc, Array perDisc)");
        return NULL;
    }
    /* per-discipline constants */
    char *parts[64][3];
    size_t plen[64][3];
    memset(parts, 0, sizeof parts);
    int ok = 1;
    for (uint32_t dix = 0; dix < n_disc && ok; ++dix) {
        napi_value row;
        if (napi_get_element(env, argv[5], dix, &row) != napi_ok) { ok = 0; break; }
        for (uint32_t k = 0; k < 3 && ok; ++k) {
            napi_value sv;
            size_t len = 0;
            if (napi_get_element(env, row, k, &sv) != napi_ok || napi_get_value_string_utf8(env, sv, NULL, 0, &len) != napi_ok) { ok = 0; break; }
            parts[dix][k] = (char *)malloc(len + 1);
            if (!parts[dix][k] || napi_get_value_string_utf8(env, sv, parts[dix][k], len + 1, &plen[dix][k]) != napi_ok) ok = 0;
        }
    }
    sbuf b = {NULL, 0, 0};
    int covered = ok;
    if (ok) ok = SB_LIT(&b, "{\"events\":[");
    for (int64_t i = 0; i < m && ok && covered; ++i) {
        const int32_t dv = disc[i];
        if (dv < 0 || (uint32_t)dv >= n_disc) { covered = 0; break; }
        const int has_end = end[i] != INT64_MIN;
        char iso_s[25], iso_e[25];
        int hs = 0, ms_ = 0, he = 0, me = 0;
        if (!iso_utc(start[i], iso_s, &hs, &ms_) || (has_end && !iso_utc(end[i], iso_e, &he, &me))) { covered = 0; break; }
        /* allDay heuristic of calendarFeed.js:64 on the UTC clock fields */
        const int all_day = hs == 0 && ms_ == 0 && (!has_end || he == 0);
        ok = (i == 0 || SB_LIT(&b, ",")) && SB_LIT(&b, "{\"id\":\"session-") && sb_i64(&b, idx[i]) && SB_LIT(&b, "\",\"title\":\"") &&
             sb_put(&b, parts[dv][0], plen[dv][0]) && SB_LIT(&b, " session #") && sb_i64(&b, idx[i]) &&
             SB_LIT(&b, "\",\"description\":\"\",\"location\":\"\",\"start\":\"") && sb_put(&b, iso_s, 24) && SB_LIT(&b, "\",\"end\":\"") &&
             (has_end ? sb_put(&b, iso_e, 24) : 1) && SB_LIT(&b, "\",\"startTs\":") && sb_i64(&b, start[i]) && SB_LIT(&b, ",\"endTs\":") &&
             (has_end ? sb_i64(&b, end[i]) : SB_LIT(&b, "null")) && SB_LIT(&b, ",\"allDay\":") &&
             (all_day ? SB_LIT(&b, "true") : SB_LIT(&b, "false")) && SB_LIT(&b, ",\"eventName\":") &&
             sb_put(&b, parts[dv][1], plen[dv][1]) && SB_LIT(&b, ",\"showNumber\":") && sb_i64(&b, idx[i]) && SB_LIT(&b, ",\"color\":") &&
             sb_put(&b, parts[dv][2], plen[dv][2]) && SB_LIT(&b, "}");
    }
    if (ok && covered) ok = SB_LIT(&b, "]}");
    for (uint32_t dix = 0; dix < 64; ++dix)
        for (int k = 0; k < 3; ++k) free(parts[dix][k]);
    napi_value out = NULL;
    if (!ok) {
        free(b.p);
        napi_throw_error(env, NULL, "serializeEvents: out of memory or bad perDisc table");
        return NULL;
    }
    if (!covered) {
        free(b.p);
        napi_get_null(env, &out);
        return out;
    }
    void *copy = NULL;
    if (napi_create_buffer_copy(env, b.len, b.p, &copy, &out) != napi_ok) {
        free(b.p);
        napi_throw_error(env, NULL, "cannot create Buffer");
        return NULL;
    }
    free(b.p);
    return out;
}

/* serializeICal(idx Int32Array, m, start BigInt64Array, end BigInt64Array, disc Int32Array, summaries Array<string>,
 *               dtstampMs) -> Buffer with exactly the bytes of host/calendarFeed.js toICalendar(rows.map(eventFromRow)):
 * the iCalendar (RFC 5545) form of the feed — new functionality, the reference only consumes .ics.  summaries[d] = the
 * escaped SUMMARY prefix of discipline d ("<name> session #" follows the row number).  Returns null when a row is
 * outside what this fast path covers (year outside 0000..9999, unknown discipline, a SUMMARY line that would need
 * folding): the caller then uses the JS path. */
static int ics_utc(int64_t ms, char out[17])
{
    char iso[25];
    int h, mi;
    int64_t sec_ms = ms - (((ms % 1000) + 1000) % 1000); /* floor to the second, also for negative ms */
    if (!iso_utc(sec_ms, iso, &h, &mi)) return 0;
    /* YYYY-MM-DDTHH:mm:ss.sssZ -> YYYYMMDDTHHMMSSZ */
    memcpy(out, iso, 4); memcpy(out + 4, iso + 5, 2); memcpy(out + 6, iso + 8, 2);
    out[8] = 'T';
    memcpy(out + 9, iso + 11, 2); memcpy(out + 11, iso + 14, 2); memcpy(out + 13, iso + 17, 2);
    out[15] = 'Z';
    out[16] = 0;
    return 1;
}

static napi_value fn_serialize_ical(napi_env env, napi_callback_info info)
{
    ARGS(7)
    size_t cap = 0, n1 = 0, n2 = 0, n3 = 0;
    int32_t *idx = typed(env, argv[0], napi_int32_array, &cap);
    int64_t m = 0, stamp_ms = 0;
    int64_t *start = typed(env, argv[2], napi_bigint64_array, &n1), *end = typed(env, argv[3], napi_bigint64_array, &n2);
    int32_t *disc = typed(env, argv[4], napi_int32_array, &n3);
    uint32_t n_disc = 0;
    if (!idx || !get_i64(env, argv[1], &m) || m < 0 || (size_t)m > cap || !start || !end || !disc || n1 < (size_t)m ||
        n2 < (size_t)m || n3 < (size_t)m || napi_get_array_length(env, argv[5], &n_disc) != napi_ok || n_disc > 64 ||
        !get_i64(env, argv[6], &stamp_ms)) {
        napi_throw_type_error(env, NULL, "serializeICal(Int32Array idx, m, BigInt64Array start, BigInt64Array end, Int32Array disc, Array summaries, dtstampMs)");
        return NULL;
    }
    char *sum[64];
    size_t sum_len[64];
    memset(sum, 0, sizeof sum);
    int ok = 1, covered = 1;
    for (uint32_t d = 0; d < n_disc && ok; ++d) {
        napi_value sv;
        size_t len = 0;
        if (napi_get_element(env, argv[5], d, &sv) != napi_ok || napi_get_value_string_utf8(env, sv, NULL, 0, &len) != napi_ok) { ok = 0; break; }
        sum[d] = (char *)malloc(len + 1);
        if (!sum[d] || napi_get_value_string_utf8(env, sv, sum[d], len + 1, &sum_len[d]) != napi_ok) ok = 0;
        /* "SUMMARY:" + prefix + up to 10 digits must stay within 75 octets, or the line would need folding */
        if (ok && 8 + sum_len[d] + 10 > 75) covered = 0;
    }
    char stamp[17];
    if (ok && !ics_utc(stamp_ms, stamp)) covered = 0;
    sbuf b = {NULL, 0, 0};
    if (ok && covered) ok = SB_LIT(&b, "BEGIN:VCALENDAR\r\nVERSION:2.0\r\nPRODID:-//sph-pie_amd//session feed//EN\r\nCALSCALE:GREGORIAN\r\n");
    for (int64_t i = 0; i < m && ok && covered; ++i) {
        const int32_t dv = disc[i];
        char ds[17], de[17];
        const int has_end = end[i] != INT64_MIN;
        if (dv < 0 || (uint32_t)dv >= n_disc || !ics_utc(start[i], ds) || (has_end && !ics_utc(end[i], de))) { covered = 0; break; }
        ok = SB_LIT(&b, "BEGIN:VEVENT\r\nUID:session-") && sb_i64(&b, idx[i]) && SB_LIT(&b, "\r\nDTSTAMP:") && sb_put(&b, stamp, 16) &&
             SB_LIT(&b, "\r\nDTSTART:") && sb_put(&b, ds, 16) && (has_end ? (SB_LIT(&b, "\r\nDTEND:") && sb_put(&b, de, 16)) : 1) &&
             SB_LIT(&b, "\r\nSUMMARY:") && sb_put(&b, sum[dv], sum_len[dv]) && sb_i64(&b, idx[i]) && SB_LIT(&b, "\r\nEND:VEVENT\r\n");
    }
    if (ok && covered) ok = SB_LIT(&b, "END:VCALENDAR\r\n");
    for (uint32_t d = 0; d < 64; ++d) free(sum[d]);
    napi_value out = NULL;
    if (!ok) {
        free(b.p);
        napi_throw_error(env, NULL, "serializeICal: out of memory or bad summaries table");
        return NULL;
    }
    if (!covered) {
        free(b.p);
        napi_get_null(env, &out);
        return out;
    }
    void *copy = NULL;
    if (napi_create_buffer_copy(env, b.len, b.p, &copy, &out) != napi_ok) {
        free(b.p);
        napi_throw_error(env, NULL, "cannot create Buffer");
        return NULL;
    }
    free(b.p);
    return out;
}

/* serializeCsv(idx Int32Array, m, start, end BigInt64Array, user, disc Int32Array, userIds Array<string>, discIds Array<string>,
 *              headerLine string) -> Buffer: header + one CSV line per row, '\n' between lines — exactly the bytes of
 * host/dispatchQueue.js [header].concat(rows.map(buildCsvRow)).join('\n') with the columns sessionRow, userId, discipline,
 * createdAt, expiredAt.  csvEscape is the reference's rule (/root/reference/server/webhookDispatcher.js:332-338): a field is
 * quoted iff it holds '"', ',', '\n' or '\r', inner quotes doubled.  Returns null for rows this fast path does not cover
 * (a year outside 0000..9999): the caller then uses the JS path. */
static int sb_csv_field(sbuf *b, const char *s, size_t n)
{
    int quote = 0;
    for (size_t i = 0; i < n; ++i)
        if (s[i] == '"' || s[i] == ',' || s[i] == '\n' || s[i] == '\r') { quote = 1; break; }
    if (!quote) return sb_put(b, s, n);
    if (!SB_LIT(b, "\"")) return 0;
    for (size_t i = 0; i < n; ++i) {
        if (s[i] == '"' && !SB_LIT(b, "\"")) return 0;
        if (!sb_put(b, s + i, 1)) return 0;
    }
    return SB_LIT(b, "\"");
}

static napi_value fn_serialize_csv(napi_env env, napi_callback_info info)
{
    ARGS(9)
    size_t cap = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0;
    int32_t *idx = typed(env, argv[0], napi_int32_array, &cap);
    int64_t m = 0;
    int64_t *start = typed(env, argv[2], napi_bigint64_array, &n1), *end = typed(env, argv[3], napi_bigint64_array, &n2);
    int32_t *user = typed(env, argv[4], napi_int32_array, &n3), *disc = typed(env, argv[5], napi_int32_array, &n4);
    uint32_t n_users = 0, n_disc = 0;
    size_t hlen = 0;
    if (!idx || !get_i64(env, argv[1], &m) || m < 0 || (size_t)m > cap || !start || !end || !user || !disc || n1 < (size_t)m ||
        n2 < (size_t)m || n3 < (size_t)m || n4 < (size_t)m || napi_get_array_length(env, argv[6], &n_users) != napi_ok ||
        napi_get_array_length(env, argv[7], &n_disc) != napi_ok || napi_get_value_string_utf8(env, argv[8], NULL, 0, &hlen) != napi_ok) {
        napi_throw_type_error(env, NULL, "serializeCsv(Int32Array idx, m, BigInt64Array start, BigInt64Array end, Int32Array user, Int32Array disc, Array userIds, Array discIds, header)");
        return NULL;
    }
    sbuf b = {NULL, 0, 0};
    int ok = sb_need(&b, hlen + 1), covered = 1;
    if (ok) {
        napi_get_value_string_utf8(env, argv[8], b.p, hlen + 1, &hlen);
        b.len = hlen;
    }
    char *tmp = NULL;
    size_t tmp_cap = 0;
    for (int64_t i = 0; i < m && ok && covered; ++i) {
        char iso_s[25], iso_e[25];
        int h, mi;
        const int has_end = end[i] != INT64_MIN;
        if (!iso_utc(start[i], iso_s, &h, &mi) || (has_end && !iso_utc(end[i], iso_e, &h, &mi))) { covered = 0; break; }
        ok = SB_LIT(&b, "\n") && sb_i64(&b, idx[i]) && SB_LIT(&b, ",");
        /* the two string columns: '' when the index is outside the table (userIds[u] === undefined / no discipline) */
        for (int col = 0; col < 2 && ok; ++col) {
            const int32_t k = col == 0 ? user[i] : disc[i];
            const uint32_t lim = col == 0 ? n_users : n_disc;
            if (k >= 0 && (uint32_t)k < lim) {
                napi_value sv;
                size_t len = 0;
                napi_valuetype t;
                if (napi_get_element(env, argv[6 + col], (uint32_t)k, &sv) != napi_ok || napi_typeof(env, sv, &t) != napi_ok) { ok = 0; break; }
                if (t == napi_string) {
                    if (napi_get_value_string_utf8(env, sv, NULL, 0, &len) != napi_ok) { ok = 0; break; }
                    if (len + 1 > tmp_cap) {
                        char *np = (char *)realloc(tmp, len + 1);
                        if (!np) { ok = 0; break; }
                        tmp = np;
                        tmp_cap = len + 1;
                    }
                    if (napi_get_value_string_utf8(env, sv, tmp, len + 1, &len) != napi_ok) { ok = 0; break; }
                    ok = sb_csv_field(&b, tmp, len);
                } else if (t != napi_undefined && t != napi_null) {
                    covered = 0; /* a non-string id: String(value) is the JS path's business */
                }
            }
            if (ok) ok = SB_LIT(&b, ",");
        }
        if (ok && covered) ok = sb_put(&b, iso_s, 24) && SB_LIT(&b, ",") && (has_end ? sb_put(&b, iso_e, 24) : 1);
    }
    free(tmp);
    napi_value out = NULL;
    if (!ok) {
        free(b.p);
        napi_throw_error(env, NULL, "serializeCsv: out of memory or bad id table");
        return NULL;
    }
    if (!covered) {
        free(b.p);
        napi_get_null(env, &out);
        return out;
    }
    void *copy = NULL;
    if (napi_create_buffer_copy(env, b.len, b.p, &copy, &out) != napi_ok) {
        free(b.p);
        napi_throw_error(env, NULL, "cannot create Buffer");
        return NULL;
    }
    free(b.p);
    return out;
}

/* ---- batched scan: the requests of one event-loop turn, one table pass ------------------------------------------------
 * queries travel as three typed arrays of equal length (<= PIE_BATCH_MAX): now, cutoff (BigInt64Array), mask (BigUint64Array) */
static int read_queries(napi_env env, napi_value nows, napi_value cutoffs, napi_value masks, pie_query *out, int *n_q)
{
    size_t a = 0, b = 0, c = 0;
    int64_t *pn = typed(env, nows, napi_bigint64_array, &a), *pc = typed(env, cutoffs, napi_bigint64_array, &b);
    uint64_t *pm = typed(env, masks, napi_biguint64_array, &c);
    if (!pn || !pc || !pm || a != b || a != c || a < 1 || a > PIE_BATCH_MAX) return 0;
    for (size_t k = 0; k < a; ++k) {
        out[k].now = pn[k];
        out[k].cutoff = pc[k];
        out[k].mask = pm[k];
    }
    *n_q = (int)a;
    return 1;
}

/* scanBatch(ctx, nows, cutoffs, masks) -> Array of M per query; results stay in HBM (batchUserFeed reads a slice) */
static napi_value fn_scan_batch(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    pie_query q[PIE_BATCH_MAX];
    int n_q = 0;
    if (!read_queries(env, argv[1], argv[2], argv[3], q, &n_q)) {
        napi_throw_type_error(env, NULL, "scanBatch(ctx, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks): 1..64 queries, equal lengths");
        return NULL;
    }
    size_t m[PIE_BATCH_MAX];
    int rc = p_pie_scan_batch(ctx, q, n_q, m);
    if (rc) return throw_pie(env, ctx, rc);
    napi_value out;
    CHECK(env, napi_create_array_with_length(env, (size_t)n_q, &out));
    for (int k = 0; k < n_q; ++k) napi_set_element(env, out, (uint32_t)k, js_int(env, (int64_t)m[k]));
    return out;
}

/* scanWide(ctx, nows, cutoffs, masks) -> Array of M per query: ONE wide batch of 1..PIE_WIDE_MAX queries (pie_scan_wide_*),
 * begun and finished; batchUserFeed / batchFetchRequests then read it for any query index.  The queries and counts live on the
 * heap, not on the stack. */
static napi_value fn_scan_wide(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t a = 0, b = 0, c = 0;
    int64_t *pn = typed(env, argv[1], napi_bigint64_array, &a), *pc = typed(env, argv[2], napi_bigint64_array, &b);
    uint64_t *pm = typed(env, argv[3], napi_biguint64_array, &c);
    if (!pn || !pc || !pm || a != b || a != c || a < 1 || a > PIE_WIDE_MAX) {
        napi_throw_type_error(env, NULL, "scanWide(ctx, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks): 1..512 queries, equal lengths");
        return NULL;
    }
    pie_query *q = (pie_query *)malloc(a * sizeof(pie_query));
    size_t *m = (size_t *)malloc(a * sizeof(size_t));
    if (!q || !m) {
        free(q);
        free(m);
        napi_throw_error(env, NULL, "scanWide: out of host memory");
        return NULL;
    }
    for (size_t k = 0; k < a; ++k) {
        q[k].now = pn[k];
        q[k].cutoff = pc[k];
        q[k].mask = pm[k];
    }
    int n_q = 0;
    int rc = p_pie_scan_wide_begin(ctx, q, (int)a);
    if (rc == 0) rc = p_pie_scan_wide_finish(ctx, m, a, &n_q);
    free(q);
    if (rc) {
        free(m);
        return throw_pie(env, ctx, rc);
    }
    napi_value out;
    if (napi_create_array_with_length(env, (size_t)n_q, &out) != napi_ok) {
        free(m);
        return NULL;
    }
    for (int k = 0; k < n_q; ++k) napi_set_element(env, out, (uint32_t)k, js_int(env, (int64_t)m[k]));
    free(m);
    return out;
}

/* batchUserFeed(ctx, qi, user, idx Int32Array) -> k */
static napi_value fn_batch_user_feed(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t qi = 0;
    int64_t user = 0;
    size_t cap = 0, k = 0;
    int32_t *idx = typed(env, argv[3], napi_int32_array, &cap);
    if (napi_get_value_int32(env, argv[1], &qi) != napi_ok || !get_i64(env, argv[2], &user) || !idx || user < INT32_MIN || user > INT32_MAX) {
        napi_throw_type_error(env, NULL, "batchUserFeed(ctx, qi, user, Int32Array)");
        return NULL;
    }
    int rc = p_pie_batch_read_user_feed(ctx, qi, (int32_t)user, idx, cap, &k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}

/* ---- communicator: the sharded table over several GPUs (pie_comm_*, RCCL behind the C ABI) -------------------------- */
static napi_value throw_comm(napi_env env, pie_comm *cm, int rc)
{
    char buf[640];
    snprintf(buf, sizeof buf, "pie_comm error %d: %s", rc, p_pie_comm_last_error ? p_pie_comm_last_error(cm) : "library not open");
    napi_throw(env, error_with_code(env, buf, rc));
    return NULL;
}

typedef struct comm_box_s {
    pie_comm *comm;
    ctx_box *boxes; /* context handles handed out by commCtx and still alive */
    pie_nq_ring step_nq, wide_nq; /* n_q of the ordinary / wide steps begun and not finished on THIS communicator */
    /* what THIS communicator has begun beside its steps and not finished: the keys of every lookup (commTokenLookupBegin), oldest
     * first, and the rows the queue's finish has to make room for (commExpiredQueueBegin) */
    size_t lk_k[4];
    int lk_head, lk_n;
    size_t eq_cap;
    int eq_begun;
    int busy; /* a finish of either is waiting on the libuv pool: one thread per communicator */
} comm_box;

enum { STEP_SETS = 16, WIDE_STEP_SETS = 8 }; /* the rings' capacities: the buffer sets of pie_comm_step_* / pie_comm_wide_step_* */

static void comm_unlink_ctx(ctx_box *b)
{
    if (!b->parent) return;
    for (ctx_box **pp = &b->parent->boxes; *pp; pp = &(*pp)->next)
        if (*pp == b) {
            *pp = b->next;
            break;
        }
    b->parent = NULL;
    b->next = NULL;
}

/* the communicator's contexts are about to die (or just died): every handle to them becomes a destroyed context */
static void comm_orphan_ctxs(comm_box *cb)
{
    for (ctx_box *b = cb->boxes; b;) {
        ctx_box *nx = b->next;
        b->ctx = NULL;
        b->parent = NULL;
        b->next = NULL;
        b = nx;
    }
    cb->boxes = NULL;
}

static int comm_any_busy(const comm_box *cb)
{
    if (cb->busy) return 1;
    for (const ctx_box *b = cb->boxes; b; b = b->next)
        if (b->busy) return 1;
    return 0;
}

static void comm_finalize(napi_env env, void *data, void *hint)
{
    (void)env;
    (void)hint;
    comm_box *b = (comm_box *)data;
    if (b) comm_orphan_ctxs(b);
    if (b && b->comm && p_pie_comm_destroy) p_pie_comm_destroy(b->comm);
    free(b);
}

static comm_box *get_comm_box(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((comm_box *)p)->comm) {
        napi_throw_type_error(env, NULL, "expected a live pie communicator");
        return NULL;
    }
    if (comm_any_busy((comm_box *)p)) {
        throw_state(env, "pie_comm error -6: an asynchronous scan is in flight on one of this communicator's contexts");
        return NULL;
    }
    return (comm_box *)p;
}

static pie_comm *get_comm(napi_env env, napi_value v)
{
    void *p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !((comm_box *)p)->comm) {
        napi_throw_type_error(env, NULL, "expected a live pie communicator");
        return NULL;
    }
    return ((comm_box *)p)->comm;
}

/* commCreate(Int32Array deviceIds) -> communicator: one shard per listed GPU, driven by this process */
static napi_value fn_comm_create(napi_env env, napi_callback_info info)
{
    ARGS(1)
    if (!need_lib(env)) return NULL;
    size_t n = 0;
    int32_t *ids = typed(env, argv[0], napi_int32_array, &n);
    if (!ids || n < 1) {
        napi_throw_type_error(env, NULL, "commCreate(Int32Array deviceIds)");
        return NULL;
    }
    pie_comm *cm = NULL;
    int rc = p_pie_comm_create(ids, (int32_t)n, &cm);
    if (rc) return throw_comm(env, NULL, rc);
    comm_box *b = (comm_box *)calloc(1, sizeof *b);
    napi_value ext;
    if (!b || napi_create_external(env, b, comm_finalize, NULL, &ext) != napi_ok) {
        p_pie_comm_destroy(cm);
        free(b);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    b->comm = cm;
    return ext;
}

static napi_value fn_comm_destroy(napi_env env, napi_callback_info info)
{
    ARGS(1)
    void *p = NULL;
    if (napi_get_value_external(env, argv[0], &p) != napi_ok || !p) {
        napi_throw_type_error(env, NULL, "expected a pie communicator");
        return NULL;
    }
    comm_box *b = (comm_box *)p;
    if (comm_any_busy(b)) return throw_state(env, "pie_comm error -6: an asynchronous scan is in flight on one of this communicator's contexts");
    comm_orphan_ctxs(b); /* handles handed out by commCtx now read as destroyed contexts */
    if (b->comm) p_pie_comm_destroy(b->comm);
    b->comm = NULL;
    nq_ring_clear(&b->step_nq);
    nq_ring_clear(&b->wide_nq);
    b->lk_head = b->lk_n = b->eq_begun = 0; /* pie_comm_destroy landed what was begun */
    return js_int(env, 0);
}

static napi_value fn_comm_world(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    return js_int(env, p_pie_comm_world(cm));
}

/* commCtx(comm, rank) -> context handle of that shard (owned by the communicator) */
static napi_value fn_comm_ctx(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t rank = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &rank));
    pie_ctx *ctx = p_pie_comm_ctx(cm, rank);
    if (!ctx) return throw_state(env, "pie_comm error -6: that rank is not local to this communicator");
    void *pcb = NULL;
    CHECK(env, napi_get_value_external(env, argv[0], &pcb));
    comm_box *cb = (comm_box *)pcb;
    if (cb->busy) return throw_state(env, "pie_comm error -6: a finish of this communicator is waiting on the pool");
    ctx_box *b = (ctx_box *)calloc(1, sizeof *b);
    napi_value ext;
    if (!b || napi_create_reference(env, argv[0], 1, &b->comm_ref) != napi_ok) {
        free(b);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    if (napi_create_external(env, b, box_finalize, NULL, &ext) != napi_ok) {
        napi_delete_reference(env, b->comm_ref);
        free(b);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    b->ctx = ctx;
    b->owned = 0;
    b->parent = cb;
    b->next = cb->boxes;
    cb->boxes = b;
    return ext;
}

/* commGenSyntheticSharded(comm, seed, nTotal, nUsers, nDisc, flags) */
static napi_value fn_comm_gen(napi_env env, napi_callback_info info)
{
    ARGS(6)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int64_t seed, n_total;
    int32_t n_users, n_disc, flags;
    if (!get_i64(env, argv[1], &seed) || !get_i64(env, argv[2], &n_total)) {
        napi_throw_type_error(env, NULL, "bad integer argument");
        return NULL;
    }
    CHECK(env, napi_get_value_int32(env, argv[3], &n_users));
    CHECK(env, napi_get_value_int32(env, argv[4], &n_disc));
    CHECK(env, napi_get_value_int32(env, argv[5], &flags));
    int rc = p_pie_comm_gen_synthetic_sharded(cm, (uint64_t)seed, n_total, n_users, n_disc, (uint32_t)flags);
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, n_total);
}

/* commScanBatchGather(comm, nows, cutoffs, masks) -> Array [rank][query] of M: every shard scans the batch, the messages
 * are exchanged over RCCL; commReadGathered then reads one (source rank, query) message as a given rank holds it */
static napi_value fn_comm_scan_gather(napi_env env, napi_callback_info info)
{
    ARGS(4)
    comm_box *cbx = get_comm_box(env, argv[0]); /* refuses while scanAsync runs on one of the shard contexts */
    if (!cbx) return NULL;
    pie_comm *cm = cbx->comm;
    pie_query q[PIE_BATCH_MAX];
    int n_q = 0;
    if (!read_queries(env, argv[1], argv[2], argv[3], q, &n_q)) {
        napi_throw_type_error(env, NULL, "commScanBatchGather(comm, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks)");
        return NULL;
    }
    const int world = p_pie_comm_world(cm);
    size_t *m = (size_t *)calloc((size_t)world * (size_t)n_q, sizeof *m);
    if (!m) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    int rc = p_pie_comm_scan_batch_gather(cm, q, n_q, 0, m);
    if (rc) {
        free(m);
        return throw_comm(env, cm, rc);
    }
    napi_value out;
    napi_create_array_with_length(env, (size_t)world, &out);
    for (int r = 0; r < world; ++r) {
        napi_value row;
        napi_create_array_with_length(env, (size_t)n_q, &row);
        for (int k = 0; k < n_q; ++k) napi_set_element(env, row, (uint32_t)k, js_int(env, (int64_t)m[(size_t)r * n_q + k]));
        napi_set_element(env, out, (uint32_t)r, row);
    }
    free(m);
    return out;
}

/* commReadGathered(comm, atRank, srcRank, qi, offsets Int32Array[>= uPad + 1], idx Int32Array) -> M */
static napi_value fn_comm_read(napi_env env, napi_callback_info info)
{
    ARGS(6)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t at = 0, src = 0, qi = 0;
    size_t no = 0, cap = 0, m = 0, u_pad = 0, rs = 0, qs = 0;
    void *base = NULL;
    CHECK(env, napi_get_value_int32(env, argv[1], &at));
    CHECK(env, napi_get_value_int32(env, argv[2], &src));
    CHECK(env, napi_get_value_int32(env, argv[3], &qi));
    int32_t *off = typed(env, argv[4], napi_int32_array, &no), *idx = typed(env, argv[5], napi_int32_array, &cap);
    int rc = p_pie_comm_gathered_device_ptr(cm, at, &base, &rs, &qs, &u_pad);
    if (rc) return throw_comm(env, cm, rc);
    if (!off || !idx || no < u_pad + 1) {
        napi_throw_type_error(env, NULL, "commReadGathered(comm, at, src, qi, Int32Array[>= uPad + 1], Int32Array)");
        return NULL;
    }
    rc = p_pie_comm_read_gathered(cm, at, src, qi, off, idx, cap, &m);
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, (int64_t)m);
}

/* commExpiredQueue(comm, prevNow, now, rows Int32Array[, srcRank Int32Array, srcRow Int32Array]) -> q
 * commArchiveQueue(comm, now, windowMs, rows Int32Array[, srcRank, srcRow]) -> q
 * The dispatch queue of the whole sharded table, merged on the devices: ascending global rows (expired), or the archive
 * queue's global rows; srcRank / srcRow (optional, both or neither) = the shard that holds each row and its local row there.
 * Throws with .code = PIE_E_CAPACITY (-5) when rows is shorter than the queue, like expiredQueue / archiveQueue. */
static napi_value comm_queue_call(napi_env env, napi_callback_info info, int archive)
{
    size_t argc = 6;
    napi_value argv[6];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = archive ? "commArchiveQueue(comm, now, windowMs, Int32Array rows[, Int32Array srcRank, Int32Array srcRow])"
                                : "commExpiredQueue(comm, prevNow, now, Int32Array rows[, Int32Array srcRank, Int32Array srcRow])";
    if (argc != 4 && argc != 6) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    comm_box *cbx = get_comm_box(env, argv[0]); /* refuses while scanAsync runs on one of the shard contexts */
    if (!cbx) return NULL;
    pie_comm *cm = cbx->comm;
    int64_t a = 0, b = 0;
    size_t cap = 0, c1 = 0, c2 = 0, q = 0;
    int32_t *rows = typed(env, argv[3], napi_int32_array, &cap);
    int32_t *src_rank = argc == 6 ? typed(env, argv[4], napi_int32_array, &c1) : NULL;
    int32_t *src_row = argc == 6 ? typed(env, argv[5], napi_int32_array, &c2) : NULL;
    if (!get_i64(env, argv[1], &a) || !get_i64(env, argv[2], &b) || !rows || (argc == 6 && (!src_rank || !src_row))) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    int rc = archive ? p_pie_comm_archive_queue(cm, a, b, rows, cap, &q) : p_pie_comm_expired_queue(cm, a, b, rows, cap, &q);
    if (rc) return throw_comm(env, cm, rc);
    if (src_rank) {
        int32_t at = 0; /* the first local rank: the copy rows came from */
        while (at < p_pie_comm_world(cm) && !p_pie_comm_ctx(cm, at)) ++at;
        rc = p_pie_comm_queue_read(cm, at, NULL, src_rank, src_row, c1 < c2 ? c1 : c2, &q);
        if (rc) return throw_comm(env, cm, rc);
    }
    return js_int(env, (int64_t)q);
}
static napi_value fn_comm_expired_queue(napi_env env, napi_callback_info info) { return comm_queue_call(env, info, 0); }
static napi_value fn_comm_archive_queue(napi_env env, napi_callback_info info) { return comm_queue_call(env, info, 1); }

/* ---- a live sharded table: createSession / touchSession / deleteSession / deleteSessionsForUser (server/sessionStore.js:12-19,
 * 37-64) on every shard of the communicator, by GLOBAL row and user id (pie_comm_append_rows ...).  Nothing is kept here: the
 * table's size lives in the library's contexts.
 * commAppendRows(comm, start BigInt64Array, end BigInt64Array, user Int32Array, disc Int32Array, nUsers) -> first new global row
 * commSetEnd(comm, rows Int32Array, newEnd BigInt64Array) -> elements
 * commDeleteUser(comm, user, rowsOut Int32Array) -> {deleted, owner}: rowsOut receives the tombstoned global rows, ascending;
 *   throws with .code = -5 when it is too short (the rows are tombstoned all the same); owner = -1 for an unknown id
 * commTableSize(comm) -> {rows, users} of the whole table */
static napi_value fn_comm_append_rows(napi_env env, napi_callback_info info)
{
    ARGS(6)
    comm_box *cbx = get_comm_box(env, argv[0]); /* refuses while scanAsync runs on one of the shard contexts */
    if (!cbx) return NULL;
    size_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    int64_t *s = typed(env, argv[1], napi_bigint64_array, &n0), *e = typed(env, argv[2], napi_bigint64_array, &n1);
    int32_t *u = typed(env, argv[3], napi_int32_array, &n2), *d = typed(env, argv[4], napi_int32_array, &n3);
    int32_t n_users = 0, first = 0;
    if (!s || !e || !u || !d || n0 != n1 || n0 != n2 || n0 != n3) {
        napi_throw_type_error(env, NULL, "commAppendRows(comm, BigInt64Array start, BigInt64Array end, Int32Array user, Int32Array disc, nUsers): equal lengths");
        return NULL;
    }
    CHECK(env, napi_get_value_int32(env, argv[5], &n_users));
    int rc = p_pie_comm_append_rows(cbx->comm, s, e, u, d, n0, n_users, &first);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, (int64_t)first);
}

static napi_value fn_comm_set_end(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0, k2 = 0;
    int32_t *rows = typed(env, argv[1], napi_int32_array, &k);
    int64_t *ne = typed(env, argv[2], napi_bigint64_array, &k2);
    if (!rows || !ne || k != k2) {
        napi_throw_type_error(env, NULL, "commSetEnd(comm, Int32Array rows, BigInt64Array newEnd)");
        return NULL;
    }
    int rc = p_pie_comm_set_end(cbx->comm, rows, ne, k);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, (int64_t)k);
}

static napi_value fn_comm_delete_user(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int32_t user = 0, owner = -1;
    size_t cap = 0, k = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &user));
    int32_t *rows = typed(env, argv[2], napi_int32_array, &cap);
    if (!rows) {
        napi_throw_type_error(env, NULL, "commDeleteUser(comm, user, Int32Array rowsOut)");
        return NULL;
    }
    int rc = p_pie_comm_delete_user(cbx->comm, user, rows, cap, &k, &owner);
    if (rc) return throw_comm(env, cbx->comm, rc);
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    napi_set_named_property(env, out, "deleted", js_int(env, (int64_t)k));
    napi_set_named_property(env, out, "owner", js_int(env, (int64_t)owner));
    return out;
}

/* commDeleteUsers(comm, users Int32Array, rowsOut Int32Array[, perUser Int32Array[, owners Int32Array]]) -> rows tombstoned over
 * the local shards (rowsOut: global rows, ascending) */
static napi_value fn_comm_delete_users(napi_env env, napi_callback_info info)
{
    size_t argc = 5;
    napi_value argv[5];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    if (argc < 3) {
        napi_throw_type_error(env, NULL, "too few arguments");
        return NULL;
    }
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t n = 0, cap = 0, np = 0, no = 0, k = 0;
    int32_t *users = typed(env, argv[1], napi_int32_array, &n);
    int32_t *rows = typed(env, argv[2], napi_int32_array, &cap);
    int32_t *per = argc > 3 ? typed(env, argv[3], napi_int32_array, &np) : NULL;
    int32_t *own = argc > 4 ? typed(env, argv[4], napi_int32_array, &no) : NULL;
    bool users_typed = false;
    if (napi_is_typedarray(env, argv[1], &users_typed) != napi_ok) users_typed = false;
    if (!users_typed || (!users && n) || !rows || (argc > 3 && n && (!per || np != n)) || (argc > 4 && n && (!own || no != n))) {
        napi_throw_type_error(env, NULL, "commDeleteUsers(comm, Int32Array users, Int32Array rowsOut[, Int32Array perUser[, Int32Array owners]])");
        return NULL;
    }
    int rc = n ? p_pie_comm_delete_users(cbx->comm, users, n, rows, cap, &k, per, own) : 0;
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, (int64_t)k);
}

/* A sharded table that ages (pie_comm_prune_before / pie_comm_retention_purge_tz / pie_comm_compact_rows; _pruneCalendarEvents,
 * sqlProvider.js:956-968; _purgeExpiredArchives, :863-890, 991-1009; sessions.delete(), sessionStore.js:47-53):
 * commPruneBefore(comm, cutoff, rows Int32Array[, srcRank Int32Array, srcRow Int32Array]) -> n
 * commRetentionPurge(comm, now, months, transitions BigInt64Array[n], offsets BigInt64Array[n + 1], rows[, srcRank, srcRow]) -> n
 *   rows receives the tombstoned GLOBAL rows, ascending, merged on the first local rank's device; srcRank / srcRow (both or
 *   neither) the shard that holds each and its local row there.  The zone table is host/tzTable.js's (no transitions: a fixed
 *   offset).  Throws with .code = -5 when rows is too short: the rows are tombstoned all the same.
 * commCompactRows(comm, deadBefore BigInt|Number, shrink[, keptLocal Int32Array[local ranks]]) -> rows kept over the local shards;
 *   global rows keep their numbers */
static napi_value comm_maint_call(napi_env env, napi_callback_info info, int retention)
{
    size_t argc = 8;
    napi_value argv[8];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = retention ? "commRetentionPurge(comm, now, months, BigInt64Array transitions[n], BigInt64Array offsets[n + 1], Int32Array rows[, Int32Array srcRank, Int32Array srcRow])"
                                  : "commPruneBefore(comm, cutoff, Int32Array rows[, Int32Array srcRank, Int32Array srcRow])";
    const size_t base = retention ? 6 : 3;
    if (argc != base && argc != base + 2) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    comm_box *cbx = get_comm_box(env, argv[0]); /* refuses while scanAsync runs on one of the shard contexts */
    if (!cbx) return NULL;
    pie_comm *cm = cbx->comm;
    int64_t a = 0;
    int32_t months = 0;
    size_t nt = 0, no = 0, cap = 0, c1 = 0, c2 = 0, n = 0;
    int64_t *tr = NULL, *off = NULL;
    bool ok = get_i64(env, argv[1], &a) != 0;
    if (ok && retention) {
        ok = napi_get_value_int32(env, argv[2], &months) == napi_ok;
        tr = typed(env, argv[3], napi_bigint64_array, &nt);
        off = typed(env, argv[4], napi_bigint64_array, &no);
        ok = ok && off && (tr || nt == 0) && no == nt + 1;
    }
    int32_t *rows = typed(env, argv[base - 1], napi_int32_array, &cap);
    int32_t *src_rank = argc == base + 2 ? typed(env, argv[base], napi_int32_array, &c1) : NULL;
    int32_t *src_row = argc == base + 2 ? typed(env, argv[base + 1], napi_int32_array, &c2) : NULL;
    if (!ok || !rows || (argc == base + 2 && (!src_rank || !src_row))) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    int rc = retention ? p_pie_comm_retention_purge_tz(cm, a, months, tr, off, (int32_t)nt, rows, cap, &n) : p_pie_comm_prune_before(cm, a, rows, cap, &n);
    if (rc) return throw_comm(env, cm, rc);
    if (src_rank) {
        int32_t at = 0; /* the first local rank holds the merged list */
        while (at < p_pie_comm_world(cm) && !p_pie_comm_ctx(cm, at)) ++at;
        rc = p_pie_comm_queue_read(cm, at, NULL, src_rank, src_row, c1 < c2 ? c1 : c2, &n);
        if (rc) return throw_comm(env, cm, rc);
    }
    return js_int(env, (int64_t)n);
}
static napi_value fn_comm_prune_before(napi_env env, napi_callback_info info) { return comm_maint_call(env, info, 0); }
static napi_value fn_comm_retention_purge(napi_env env, napi_callback_info info) { return comm_maint_call(env, info, 1); }

static napi_value fn_comm_compact_rows(napi_env env, napi_callback_info info)
{
    size_t argc = 4;
    napi_value argv[4];
    CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    const char *usage = "commCompactRows(comm, deadBefore BigInt|Number, shrink[, Int32Array keptLocal[local ranks]])";
    if (argc < 3) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    pie_comm *cm = cbx->comm;
    int64_t dead_before = 0;
    bool shrink = false;
    size_t nl = 0, total = 0, per[64] = {0};
    const int32_t n_local = p_pie_comm_local_ranks(cm);
    int32_t *kept_local = argc > 3 ? typed(env, argv[3], napi_int32_array, &nl) : NULL;
    if (!get_i64(env, argv[1], &dead_before) || napi_get_value_bool(env, argv[2], &shrink) != napi_ok || n_local < 0 || n_local > 64 ||
        (argc > 3 && (!kept_local || nl < (size_t)n_local))) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    int rc = p_pie_comm_compact_rows(cm, dead_before, shrink ? PIE_COMPACT_SHRINK : 0u, &total, per);
    for (int32_t i = 0; kept_local && i < n_local; ++i) kept_local[i] = (int32_t)per[i];
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, (int64_t)total);
}

static napi_value fn_comm_table_size(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int64_t rows = 0;
    int32_t users = 0;
    int rc = p_pie_comm_table_size(cm, &rows, &users);
    if (rc) return throw_comm(env, cm, rc);
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    napi_set_named_property(env, out, "rows", js_int(env, rows));
    napi_set_named_property(env, out, "users", js_int(env, (int64_t)users));
    return out;
}

/* shardMaps(ctx, rowsOut Int32Array[>= rows], usersOut Int32Array[>= users]) -> rows: a shard's local row -> global row and
 * local user -> global user (pie_shard_maps) */
static napi_value fn_shard_maps(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t rows = 0, users = 0, cr = 0, cu = 0;
    int rc = table_shape(ctx, &rows, &users);
    if (rc) return throw_pie(env, ctx, rc);
    int32_t *r = typed(env, argv[1], napi_int32_array, &cr), *u = typed(env, argv[2], napi_int32_array, &cu);
    if (!r || !u || cr < rows || cu < users) {
        napi_throw_type_error(env, NULL, "shardMaps(ctx, Int32Array rowsOut[>= rows], Int32Array usersOut[>= users])");
        return NULL;
    }
    rc = p_pie_shard_maps(ctx, r, u);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)rows);
}

/* commUPad(comm, atRank) -> users per message (the largest shard's user count) of the last exchange */
static napi_value fn_comm_upad(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t at = 0;
    size_t u_pad = 0, rs = 0, qs = 0;
    void *base = NULL;
    CHECK(env, napi_get_value_int32(env, argv[1], &at));
    int rc = p_pie_comm_gathered_device_ptr(cm, at, &base, &rs, &qs, &u_pad);
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, (int64_t)u_pad);
}

/* ---- the pipelined union exchange (pie_comm_step_*): commStepReserve(comm, nQ, unionCap); commStepBegin(comm, nows, cutoffs,
 * masks); commStepFinish(comm) -> [rank][query] M; commStepCollect(comm) -> step number (throws code -5 on every rank alike when a
 * union outgrew the reservation: commNeededCap says what to reserve); commStepReadGathered(comm, at, src, step, uoff, rows, masks) */
static napi_value fn_comm_needed_cap(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    return js_int(env, (int64_t)p_pie_comm_needed_cap(cm));
}

static napi_value fn_comm_step_reserve(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int32_t n_q = 0;
    int64_t cap = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &n_q));
    CHECK(env, napi_get_value_int64(env, argv[2], &cap));
    int rc = p_pie_comm_step_reserve(cbx->comm, n_q, 0, (size_t)(cap > 0 ? cap : 0));
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, 0);
}

/* the tail of both begins: the step's n_q is kept for its finish.  After a failure that is not a plain refusal (PIE_E_STATE /
 * PIE_E_INVAL) the ring is emptied: the library may have drained every step in flight (it does when a shard failed after others
 * began), and then nothing is left to finish here either.  The rule errs in two rare cases the status alone cannot tell apart —
 * the FIRST shard failing with another status (nothing was drained: the caller's next finish throws here although the library
 * holds the step) and a later shard's own PIE_E_STATE (drained, ring kept: the next finish returns the library's PIE_E_STATE).
 * Neither can write past a buffer: step_finish gives the library room for the largest step of the kind or tells it the room. */
static napi_value step_begun(napi_env env, comm_box *cbx, pie_nq_ring *ring, unsigned cap, int rc, int n_q)
{
    if (rc) {
        if (rc != PIE_E_STATE && rc != PIE_E_INVAL) nq_ring_clear(ring);
        return throw_comm(env, cbx->comm, rc);
    }
    nq_ring_push(ring, cap, n_q);
    return js_int(env, 0);
}

/* both finishes: -> [rank][query] M of the oldest begun step */
static napi_value step_finish(napi_env env, napi_value comm, int wide)
{
    comm_box *cbx = get_comm_box(env, comm);
    if (!cbx) return NULL;
    pie_nq_ring *ring = wide ? &cbx->wide_nq : &cbx->step_nq;
    const unsigned cap = wide ? WIDE_STEP_SETS : STEP_SETS;
    if (!nq_ring_count(ring))
        return throw_state(env, wide ? "pie_comm error -6: commWideStepFinish without commWideStepBegin" : "pie_comm error -6: commStepFinish without commStepBegin");
    const int n_q = nq_ring_front(ring, cap);
    const int world = p_pie_comm_world(cbx->comm);
    /* the library writes local_ranks x the step's OWN n_q: the wide call checks that against m_cap, the ordinary one has no such
     * argument and gets room for the largest ordinary step, whatever the ring says */
    const size_t m_cap = (size_t)world * (size_t)(wide ? n_q : PIE_BATCH_MAX);
    size_t *m = (size_t *)calloc(m_cap, sizeof *m);
    if (!m) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    int rc = wide ? p_pie_comm_wide_step_finish(cbx->comm, m, m_cap) : p_pie_comm_step_finish(cbx->comm, m);
    if (!wide || rc != PIE_E_CAPACITY) nq_ring_pop(ring); /* a wide finish's PIE_E_CAPACITY consumed nothing */
    if (rc) {
        free(m);
        return throw_comm(env, cbx->comm, rc);
    }
    napi_value out;
    napi_create_array_with_length(env, (size_t)world, &out);
    for (int r = 0; r < world; ++r) {
        napi_value row;
        napi_create_array_with_length(env, (size_t)n_q, &row);
        for (int k = 0; k < n_q; ++k) napi_set_element(env, row, (uint32_t)k, js_int(env, (int64_t)m[(size_t)r * n_q + k]));
        napi_set_element(env, out, (uint32_t)r, row);
    }
    free(m);
    return out;
}

static napi_value fn_comm_step_begin(napi_env env, napi_callback_info info)
{
    ARGS(4)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    pie_query q[PIE_BATCH_MAX];
    int n_q = 0;
    if (!read_queries(env, argv[1], argv[2], argv[3], q, &n_q)) {
        napi_throw_type_error(env, NULL, "commStepBegin(comm, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks)");
        return NULL;
    }
    if (nq_ring_count(&cbx->step_nq) >= STEP_SETS) return throw_state(env, "pie_comm error -6: sixteen steps are begun: commStepFinish first");
    return step_begun(env, cbx, &cbx->step_nq, STEP_SETS, p_pie_comm_step_begin(cbx->comm, q, n_q), n_q);
}

static napi_value fn_comm_step_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    return step_finish(env, argv[0], 0);
}

static napi_value fn_comm_step_collect(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int64_t step = -1;
    int rc = p_pie_comm_step_collect(cbx->comm, &step);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, step);
}

/* commStepReadGathered(comm, atRank, srcRank, step, uoff Int32Array[>= uPad + 1], rows Int32Array, masks BigUint64Array) -> Mu */
static napi_value fn_comm_step_read(napi_env env, napi_callback_info info)
{
    ARGS(7)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t at = 0, src = 0;
    int64_t step = 0;
    size_t no = 0, nr = 0, nm = 0, mu = 0, u_pad = 0, rs = 0, cap = 0;
    void *base = NULL;
    CHECK(env, napi_get_value_int32(env, argv[1], &at));
    CHECK(env, napi_get_value_int32(env, argv[2], &src));
    CHECK(env, napi_get_value_int64(env, argv[3], &step));
    int32_t *off = typed(env, argv[4], napi_int32_array, &no), *rows = typed(env, argv[5], napi_int32_array, &nr);
    uint64_t *masks = typed(env, argv[6], napi_biguint64_array, &nm);
    int rc = p_pie_comm_step_gathered_ptr(cm, at, step, &base, &rs, &u_pad, &cap);
    if (rc) return throw_comm(env, cm, rc);
    if (!off || !rows || !masks || no < u_pad + 1) {
        napi_throw_type_error(env, NULL, "commStepReadGathered(comm, at, src, step, Int32Array[>= uPad + 1], Int32Array rows, BigUint64Array masks)");
        return NULL;
    }
    rc = p_pie_comm_step_read_gathered(cm, at, src, step, off, rows, masks, nr < nm ? nr : nm, &mu);
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, (int64_t)mu);
}

/* commStepUPad(comm, atRank, step) -> users per union message */
static napi_value fn_comm_step_upad(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t at = 0;
    int64_t step = 0;
    size_t u_pad = 0, rs = 0, cap = 0;
    void *base = NULL;
    CHECK(env, napi_get_value_int32(env, argv[1], &at));
    CHECK(env, napi_get_value_int64(env, argv[2], &step));
    int rc = p_pie_comm_step_gathered_ptr(cm, at, step, &base, &rs, &u_pad, &cap);
    if (rc) return throw_comm(env, cm, rc);
    return js_int(env, (int64_t)u_pad);
}

/* ---- the pipelined WIDE exchange (pie_comm_wide_step_*): commWideStepReserve(comm, nQMax, unionCap); commWideStepBegin(comm, nows,
 * cutoffs, masks) with 1..512 queries; commWideStepFinish(comm) -> [rank][query] M; commWideStepCollect(comm) -> step number
 * (throws code -5 on every rank alike when a union outgrew the reservation or a rank kept no union); commWideStepStatus(comm, step)
 * -> Int32Array[world] of Mu words (-1: that rank kept no union: repeat the step); commWideStepReadGathered(comm, at, src, step,
 * uoff, rows, masks) -> {mu, words}, masks holding `words` 64-bit words per row. */
static napi_value fn_comm_wide_step_reserve(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int32_t n_q = 0;
    int64_t cap = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &n_q));
    CHECK(env, napi_get_value_int64(env, argv[2], &cap));
    int rc = p_pie_comm_wide_step_reserve(cbx->comm, n_q, 0, (size_t)(cap > 0 ? cap : 0));
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, 0);
}

static napi_value fn_comm_wide_step_begin(napi_env env, napi_callback_info info)
{
    ARGS(4)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t a = 0, b = 0, c = 0;
    int64_t *pn = typed(env, argv[1], napi_bigint64_array, &a), *pc = typed(env, argv[2], napi_bigint64_array, &b);
    uint64_t *pm = typed(env, argv[3], napi_biguint64_array, &c);
    if (!pn || !pc || !pm || a != b || a != c || a < 1 || a > PIE_WIDE_MAX) {
        napi_throw_type_error(env, NULL, "commWideStepBegin(comm, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks): 1..512 queries, equal lengths");
        return NULL;
    }
    if (nq_ring_count(&cbx->wide_nq) >= WIDE_STEP_SETS) return throw_state(env, "pie_comm error -6: eight wide steps are begun: commWideStepFinish first");
    pie_query *q = (pie_query *)malloc(a * sizeof(pie_query));
    if (!q) {
        napi_throw_error(env, NULL, "commWideStepBegin: out of host memory");
        return NULL;
    }
    for (size_t k = 0; k < a; ++k) {
        q[k].now = pn[k];
        q[k].cutoff = pc[k];
        q[k].mask = pm[k];
    }
    int rc = p_pie_comm_wide_step_begin(cbx->comm, q, (int32_t)a);
    free(q);
    return step_begun(env, cbx, &cbx->wide_nq, WIDE_STEP_SETS, rc, (int)a);
}

static napi_value fn_comm_wide_step_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    return step_finish(env, argv[0], 1);
}

static napi_value fn_comm_wide_step_collect(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int64_t step = -1;
    int rc = p_pie_comm_wide_step_collect(cbx->comm, &step);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, step);
}

/* commWideStepStatus(comm, step) -> Int32Array[world] */
static napi_value fn_comm_wide_step_status(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int64_t step = 0;
    CHECK(env, napi_get_value_int64(env, argv[1], &step));
    const int world = p_pie_comm_world(cm);
    napi_value buf, out;
    void *data = NULL;
    CHECK(env, napi_create_arraybuffer(env, (size_t)world * 4, &data, &buf));
    int rc = p_pie_comm_wide_step_status(cm, step, (int32_t *)data);
    if (rc) return throw_comm(env, cm, rc);
    CHECK(env, napi_create_typedarray(env, napi_int32_array, (size_t)world, buf, 0, &out));
    return out;
}

/* commWideStepReadGathered(comm, atRank, srcRank, step, uoff Int32Array[>= uPad + 1], rows Int32Array, masks BigUint64Array) ->
 * {mu, words, uPad}; masks must hold words x rows.length entries */
static napi_value fn_comm_wide_step_read(napi_env env, napi_callback_info info)
{
    ARGS(7)
    pie_comm *cm = get_comm(env, argv[0]);
    if (!cm) return NULL;
    int32_t at = 0, src = 0;
    int64_t step = 0;
    size_t no = 0, nr = 0, nm = 0, mu = 0, u_pad = 0, rs = 0, cap = 0;
    int words = 0;
    void *base = NULL;
    CHECK(env, napi_get_value_int32(env, argv[1], &at));
    CHECK(env, napi_get_value_int32(env, argv[2], &src));
    CHECK(env, napi_get_value_int64(env, argv[3], &step));
    int32_t *off = typed(env, argv[4], napi_int32_array, &no), *rows = typed(env, argv[5], napi_int32_array, &nr);
    uint64_t *masks = typed(env, argv[6], napi_biguint64_array, &nm);
    int rc = p_pie_comm_wide_step_gathered_ptr(cm, at, step, &base, &rs, &u_pad, &cap, &words);
    if (rc) return throw_comm(env, cm, rc);
    if (!off || !rows || !masks || no < u_pad + 1 || words < 1) {
        napi_throw_type_error(env, NULL, "commWideStepReadGathered(comm, at, src, step, Int32Array[>= uPad + 1], Int32Array rows, BigUint64Array masks)");
        return NULL;
    }
    const size_t room = nr < nm / (size_t)words ? nr : nm / (size_t)words;
    rc = p_pie_comm_wide_step_read_gathered(cm, at, src, step, off, rows, masks, room, &words, &mu);
    if (rc) return throw_comm(env, cm, rc);
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    napi_set_named_property(env, out, "mu", js_int(env, (int64_t)mu));
    napi_set_named_property(env, out, "words", js_int(env, words));
    napi_set_named_property(env, out, "uPad", js_int(env, (int64_t)u_pad));
    return out;
}

/* stats(ctx) -> {rows, users, selected, algBytes, k1MsSum, scanMsSum, nProfiled, maxBucket, k1Variant, nSmall, nOver, nHot, directShift} */
static napi_value fn_stats(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    pie_stats st;
    memset(&st, 0, sizeof st);
    st.struct_size = sizeof st;
    int rc = p_pie_stats_get(ctx, &st);
    if (rc) return throw_pie(env, ctx, rc);
    napi_value o, v;
    napi_create_object(env, &o);
#define PUT(name, val)                      \
    napi_create_double(env, (double)(val), &v); \
    napi_set_named_property(env, o, name, v);
    PUT("rows", st.rows) PUT("users", st.users) PUT("selected", st.selected) PUT("algBytes", st.alg_bytes)
    PUT("k1MsSum", st.k1_ms_sum) PUT("scanMsSum", st.scan_ms_sum) PUT("nProfiled", st.n_profiled)
    PUT("maxBucket", st.max_bucket) PUT("k1Variant", st.k1_variant)
    PUT("nSmall", st.n_small) PUT("nOver", st.n_over) PUT("nHot", st.n_hot) PUT("directShift", st.direct_shift)
#undef PUT
    return o;
}

/* tableInfo(ctx) -> {rows, users, orderedRows, orderedBuilds, orderedRespreads, tokenRows}: the ordered run as pie_table_info
 * reports it (orderedRows 0: there is none, or it was invalidated) */
static napi_value fn_table_info(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    pie_table_info ti;
    memset(&ti, 0, sizeof ti);
    ti.struct_size = sizeof ti;
    int rc = p_pie_table_info_get(ctx, &ti);
    if (rc) return throw_pie(env, ctx, rc);
    napi_value o, v;
    napi_create_object(env, &o);
#define PUT(name, val)                      \
    napi_create_double(env, (double)(val), &v); \
    napi_set_named_property(env, o, name, v);
    PUT("rows", ti.rows) PUT("users", ti.users) PUT("orderedRows", ti.ordered_rows) PUT("orderedBuilds", ti.ordered_builds)
    PUT("orderedRespreads", ti.ordered_respreads) PUT("tokenRows", ti.token_rows)
#undef PUT
    return o;
}

static napi_value fn_set_profiling(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    bool on = false;
    CHECK(env, napi_get_value_bool(env, argv[1], &on));
    p_pie_set_profiling(ctx, on ? 1 : 0);
    if (!on) p_pie_stats_reset(ctx);
    return js_int(env, 0);
}

/* setOrderedRun(ctx, mode): 0 never, 1 where the general path is weak (default), 2 always (pie_set_ordered_run) */
static napi_value fn_set_ordered_run(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t mode = 1;
    CHECK(env, napi_get_value_int32(env, argv[1], &mode));
    const int rc = p_pie_set_ordered_run(ctx, mode);
    if (rc != 0) return throw_pie(env, ctx, rc);
    return js_int(env, 0);
}

/* setWideOrdered(ctx, on): 1 = a wide batch on a table whose batches take the ordered run runs one pass there and keeps its
 * union; 0 (default) = it reruns its queries one by one (pie_set_wide_ordered) */
static napi_value fn_set_wide_ordered(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t on = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &on));
    const int rc = p_pie_set_wide_ordered(ctx, on);
    if (rc != 0) return throw_pie(env, ctx, rc);
    return js_int(env, 0);
}

/* setTurnOrdered(ctx, on): 1 = a turn that logs in keeps a valid ordered run where an append would (the created rows are inserted
 * in place); 0 (default) = such a turn drops the run (pie_set_turn_ordered) */
static napi_value fn_set_turn_ordered(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t on = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &on));
    const int rc = p_pie_set_turn_ordered(ctx, on);
    if (rc != 0) return throw_pie(env, ctx, rc);
    return js_int(env, 0);
}

/* wideUnionRows(ctx) -> union rows (Mu) of the last finished wide batch, -1 when it kept no union (its queries fell back) */
static napi_value fn_wide_union_rows(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t mu = 0;
    int words = 0;
    const int rc = p_pie_batch_union_wide_device_ptrs(ctx, NULL, NULL, NULL, &words, &mu);
    if (rc == PIE_E_STATE) return js_int(env, -1);
    if (rc != 0) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)mu);
}

/* setBatchLanes(ctx, n): lanes of the batched scan — independent streams whose batches run side by side — 1..4, 0 = by table
 * size (pie_set_batch_lanes) -> lanes in use now */
static napi_value fn_set_batch_lanes(napi_env env, napi_callback_info info)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    int32_t n = 0;
    CHECK(env, napi_get_value_int32(env, argv[1], &n));
    const int rc = p_pie_set_batch_lanes(ctx, n);
    if (rc != 0) return throw_pie(env, ctx, rc);
    return js_int(env, p_pie_batch_lanes(ctx));
}

/* ---- token index (pie_token_*): keys travel as a BigUint64Array of length 2 k (host/tokenKeys.js) ------------------------ */
static uint64_t *token_keys(napi_env env, napi_value v, size_t *k)
{
    size_t n = 0;
    uint64_t *keys = typed(env, v, napi_biguint64_array, &n);
    if (!keys || (n & 1)) {
        napi_throw_type_error(env, NULL, "token keys: a BigUint64Array of two words per key");
        return NULL;
    }
    *k = n / 2;
    return keys;
}

/* tokenSet(ctx, keys) / tokenAppend(ctx, keys) -> k */
static napi_value token_set_or_append(napi_env env, napi_callback_info info, int append)
{
    ARGS(2)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int rc = append ? p_pie_token_append(ctx, keys, k) : p_pie_token_set(ctx, keys, k);
    if (rc) return throw_pie(env, ctx, rc);
    return js_int(env, (int64_t)k);
}
static napi_value fn_token_set(napi_env env, napi_callback_info info) { return token_set_or_append(env, info, 0); }
static napi_value fn_token_append(napi_env env, napi_callback_info info) { return token_set_or_append(env, info, 1); }

/* a fresh typed array of n elements of `size` bytes as property `name` of obj; -> its storage */
static void *token_out(napi_env env, napi_value obj, const char *name, napi_typedarray_type type, size_t size, size_t n)
{
    napi_value buf, arr;
    void *data = NULL;
    if (napi_create_arraybuffer(env, n * size, &data, &buf) != napi_ok || napi_create_typedarray(env, type, n, buf, 0, &arr) != napi_ok ||
        napi_set_named_property(env, obj, name, arr) != napi_ok) {
        napi_throw_error(env, NULL, "N-API call failed: result array");
        return NULL;
    }
    return data ? data : (void *)(uintptr_t)16;
}

/* tokenLookup(ctx, keys, now) -> {row Int32Array, live Uint8Array, user Int32Array, start BigInt64Array, end BigInt64Array} */
static napi_value fn_token_lookup(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0;
    int64_t now = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    if (!get_i64(env, argv[2], &now)) {
        napi_throw_type_error(env, NULL, "tokenLookup(ctx, BigUint64Array keys, now)");
        return NULL;
    }
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    if (!row || !live || !user || !start || !end) return NULL;
    int rc = p_pie_token_lookup(ctx, keys, k, now, row, live, user, start, end);
    if (rc) return throw_pie(env, ctx, rc);
    return out;
}

/* tokenSetEnd(ctx, keys, newEnd BigInt64Array, now) -> Int32Array rows written (-1: not found, or not live at `now`) */
static napi_value fn_token_set_end(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0, k2 = 0;
    int64_t now = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int64_t *ne = typed(env, argv[2], napi_bigint64_array, &k2);
    if (!ne || k2 != k || !get_i64(env, argv[3], &now)) {
        napi_throw_type_error(env, NULL, "tokenSetEnd(ctx, BigUint64Array keys, BigInt64Array newEnd, now)");
        return NULL;
    }
    napi_value buf, out;
    void *data = NULL;
    CHECK(env, napi_create_arraybuffer(env, k * 4, &data, &buf));
    int rc = p_pie_token_set_end(ctx, keys, ne, k, now, (int32_t *)data);
    if (rc) return throw_pie(env, ctx, rc);
    CHECK(env, napi_create_typedarray(env, napi_int32_array, k, buf, 0, &out));
    return out;
}

/* ---- a whole turn in one launch (pie_token_turn): the ops travel as four parallel typed arrays and are packed into pie_turn_op
 * here.  turn_ops -> a malloc'ed array of *k ops (NULL with an exception pending; k = 0 gives a one-op block nobody reads). */
static pie_turn_op *turn_ops(napi_env env, napi_value *argv, const char *usage, size_t *k)
{
    size_t kn = 0, ke = 0, kk = 0;
    uint64_t *keys = token_keys(env, argv[0], k);
    if (!keys) return NULL;
    int64_t *nows = typed(env, argv[1], napi_bigint64_array, &kn);
    int64_t *ends = typed(env, argv[2], napi_bigint64_array, &ke);
    uint8_t *kinds = typed(env, argv[3], napi_uint8_array, &kk);
    if (!nows || !ends || !kinds || kn != *k || ke != *k || kk != *k) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    pie_turn_op *ops = calloc(*k ? *k : 1, sizeof(pie_turn_op));
    if (!ops) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    for (size_t i = 0; i < *k; ++i) {
        ops[i].tok[0] = keys[2 * i];
        ops[i].tok[1] = keys[2 * i + 1];
        ops[i].now = nows[i];
        ops[i].new_end = ends[i];
        ops[i].kind = kinds[i]; /* 0 get, 1 touch, 2 delete; anything else is the library's to refuse */
    }
    return ops;
}

/* tokenTurn(ctx, keys BigUint64Array[2k], nows BigInt64Array, newEnds BigInt64Array, kinds Uint8Array) -> tokenLookup's object,
 * one entry per op, the ops applied in order (include/pie_scan.h, pie_token_turn) */
static napi_value fn_token_turn(napi_env env, napi_callback_info info)
{
    ARGS(5)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0;
    pie_turn_op *ops = turn_ops(env, argv + 1, "tokenTurn(ctx, BigUint64Array keys, BigInt64Array nows, BigInt64Array newEnds, Uint8Array kinds)", &k);
    if (!ops) return NULL;
    napi_value out;
    if (napi_create_object(env, &out) != napi_ok) {
        free(ops);
        napi_throw_error(env, NULL, "N-API call failed: result object");
        return NULL;
    }
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    if (!row || !live || !user || !start || !end) {
        free(ops);
        return NULL;
    }
    int rc = p_pie_token_turn(ctx, ops, k, row, live, user, start, end);
    free(ops);
    if (rc) return throw_pie(env, ctx, rc);
    return out;
}

/* sessionTurn(ctx, keys, nows, newEnds, kinds, users Int32Array, discs Int32Array, nUsers) -> tokenTurn's object; kind 3 creates
 * a session of users[i] / discs[i] (read at creates only) with start = nows[i], end = newEnds[i] (pie_session_turn) */
static napi_value fn_session_turn(napi_env env, napi_callback_info info)
{
    static const char usage[] = "sessionTurn(ctx, BigUint64Array keys, BigInt64Array nows, BigInt64Array newEnds, Uint8Array kinds, Int32Array users, Int32Array discs, nUsers)";
    ARGS(8)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    size_t k = 0, ku = 0, kd = 0;
    int32_t n_users = 0;
    int32_t *users = typed(env, argv[5], napi_int32_array, &ku);
    int32_t *discs = typed(env, argv[6], napi_int32_array, &kd);
    if (!users || !discs || napi_get_value_int32(env, argv[7], &n_users) != napi_ok) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    pie_turn_op *ops = turn_ops(env, argv + 1, usage, &k);
    if (!ops) return NULL;
    napi_value out;
    if (ku != k || kd != k || napi_create_object(env, &out) != napi_ok) {
        free(ops);
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    if (!row || !live || !user || !start || !end) {
        free(ops);
        return NULL;
    }
    int rc = p_pie_session_turn(ctx, ops, k, users, discs, n_users, row, live, user, start, end);
    free(ops);
    if (rc) return throw_pie(env, ctx, rc);
    return out;
}

/* ---- a batch held in flight, and token lookups beside it (pie_scan_batch_begin / _finish, pie_token_lookup_begin / _finish) -----
 * scanBatchBegin queues a batch and returns; scanBatchFinish waits for the oldest.  Between the two the turn's cookies are
 * resolved: tokenLookupBegin queues the lookup on its own stream, tokenLookupFinish waits for it on the libuv pool (the handle is
 * busy meanwhile, like under scanAsync) and resolves a Promise, so the event loop is never blocked by the device. */

/* scanBatchBegin(ctx, nows, cutoffs, masks) -> queries begun */
static napi_value fn_scan_batch_begin(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    pie_query q[PIE_BATCH_MAX];
    int n_q = 0;
    if (!read_queries(env, argv[1], argv[2], argv[3], q, &n_q)) {
        napi_throw_type_error(env, NULL, "scanBatchBegin(ctx, BigInt64Array nows, BigInt64Array cutoffs, BigUint64Array masks): 1..64 queries, equal lengths");
        return NULL;
    }
    if (b->bt_n >= (int)(sizeof b->bt_q / sizeof b->bt_q[0])) return throw_state(env, "pie_scan error -6: too many batches begun and not finished");
    int rc = p_pie_scan_batch_begin(ctx, q, n_q);
    if (rc) return throw_pie(env, ctx, rc);
    b->bt_q[(b->bt_head + b->bt_n) % (int)(sizeof b->bt_q / sizeof b->bt_q[0])] = n_q;
    b->bt_n++;
    return js_int(env, n_q);
}

/* scanBatchFinish(ctx) -> Array of M per query of the oldest batch begun; its results stay in HBM as after scanBatch */
static napi_value fn_scan_batch_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    if (b->bt_n == 0) return throw_state(env, "pie_scan error -6: no batch was begun");
    size_t m[PIE_BATCH_MAX];
    int rc = p_pie_scan_batch_finish(ctx, m);
    const int n_q = b->bt_q[b->bt_head];
    b->bt_head = (b->bt_head + 1) % (int)(sizeof b->bt_q / sizeof b->bt_q[0]); /* the library dropped the batch, finished or failed */
    b->bt_n--;
    if (rc) return throw_pie(env, ctx, rc);
    napi_value out;
    CHECK(env, napi_create_array_with_length(env, (size_t)n_q, &out));
    for (int k = 0; k < n_q; ++k) napi_set_element(env, out, (uint32_t)k, js_int(env, (int64_t)m[k]));
    return out;
}

/* tokenLookupBegin(ctx, keys, nows BigInt64Array: one clock per key) -> k */
static napi_value fn_token_lookup_begin(napi_env env, napi_callback_info info)
{
    ARGS(3)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    size_t k = 0, kn = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int64_t *nows = typed(env, argv[2], napi_bigint64_array, &kn);
    if (!nows || kn != k) {
        napi_throw_type_error(env, NULL, "tokenLookupBegin(ctx, BigUint64Array keys, BigInt64Array nows): one clock per key");
        return NULL;
    }
    if (b->lk_n >= 4) return throw_state(env, "pie_scan error -6: four token lookups are begun and not finished");
    int rc = p_pie_token_lookup_begin(ctx, keys, nows, k);
    if (rc) return throw_pie(env, ctx, rc);
    b->lk_k[(b->lk_head + b->lk_n) % 4] = k;
    b->lk_n++;
    return js_int(env, (int64_t)k);
}

/* tokenLookupRoom(ctx) -> lookups tokenLookupBegin would take now */
static napi_value fn_token_lookup_room(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    return js_int(env, p_pie_token_lookup_room(ctx));
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref result;
    pie_ctx *ctx;
    ctx_box *box;
    size_t k;
    int32_t *row, *user;
    uint8_t *live;
    int64_t *start, *end;
    int rc;
    char err[600];
} lookup_job;

static void lookup_exec(napi_env env, void *data)
{
    (void)env;
    lookup_job *j = (lookup_job *)data;
    j->rc = p_pie_token_lookup_finish(j->ctx, j->row, j->live, j->user, j->start, j->end, j->k, NULL);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_scan error %d: %s", j->rc, p_pie_last_error(j->ctx));
}

static void lookup_done(napi_env env, napi_status status, void *data)
{
    lookup_job *j = (lookup_job *)data;
    j->box->busy = 0;
    napi_value out;
    if (status != napi_ok || j->rc) {
        reject_with_code(env, j->deferred, j->rc, j->rc ? j->err : "token lookup cancelled", -1);
    } else {
        napi_get_reference_value(env, j->result, &out);
        napi_resolve_deferred(env, j->deferred, out);
    }
    napi_delete_reference(env, j->result);
    napi_delete_async_work(env, j->work);
    free(j);
}

/* tokenLookupFinish(ctx) -> Promise of tokenLookup's object for the oldest lookup begun; the wait runs on the libuv pool */
static napi_value fn_token_lookup_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    if (b->lk_n == 0) return throw_state(env, "pie_scan error -6: no token lookup was begun");
    const size_t k = b->lk_k[b->lk_head];
    lookup_job *j = (lookup_job *)calloc(1, sizeof *j);
    if (!j) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    napi_value out, promise;
    if (napi_create_object(env, &out) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: result object");
        return NULL;
    }
    j->ctx = ctx;
    j->box = b;
    j->k = k;
    j->row = token_out(env, out, "row", napi_int32_array, 4, k);
    j->live = token_out(env, out, "live", napi_uint8_array, 1, k);
    j->user = token_out(env, out, "user", napi_int32_array, 4, k);
    j->start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    j->end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    if (!j->row || !j->live || !j->user || !j->start || !j->end) {
        free(j);
        return NULL;
    }
    if (napi_create_reference(env, out, 1, &j->result) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: promise");
        return NULL;
    }
    if (!queue_promise_job(env, b, "pie_token_lookup_finish", lookup_exec, lookup_done, j, &j->work)) {
        napi_delete_reference(env, j->result);
        free(j);
        return NULL;
    }
    b->lk_head = (b->lk_head + 1) % 4; /* the library returns the slot whatever the wait says (cap = k: never PIE_E_CAPACITY) */
    b->lk_n--;
    return promise;
}

/* ---- turns beside a batch held in flight (pie_token_turn_begin / _finish / _room): tokenTurnBegin queues the turn on the context's
 * stream, fenced against the batch lanes by the library, and returns; tokenTurnFinish waits for the turn's own event on the libuv
 * pool (the handle is busy meanwhile) and resolves a Promise of tokenTurn's object. */

/* tokenTurnBegin(ctx, keys, nows, newEnds, kinds) -> k */
static napi_value fn_token_turn_begin(napi_env env, napi_callback_info info)
{
    ARGS(5)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    size_t k = 0;
    pie_turn_op *ops = turn_ops(env, argv + 1, "tokenTurnBegin(ctx, BigUint64Array keys, BigInt64Array nows, BigInt64Array newEnds, Uint8Array kinds)", &k);
    if (!ops) return NULL;
    if (b->tn_n >= 4) {
        free(ops);
        return throw_state(env, "pie_scan error -6: four token turns are begun and not finished");
    }
    int rc = p_pie_token_turn_begin(ctx, ops, k);
    free(ops);
    if (rc) return throw_pie(env, ctx, rc);
    b->tn_k[(b->tn_head + b->tn_n) % 4] = k;
    b->tn_n++;
    return js_int(env, (int64_t)k);
}

/* tokenTurnRoom(ctx) -> turns tokenTurnBegin would take now */
static napi_value fn_token_turn_room(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    return js_int(env, p_pie_token_turn_room(ctx));
}

static void turn_exec(napi_env env, void *data)
{
    (void)env;
    lookup_job *j = (lookup_job *)data;
    j->rc = p_pie_token_turn_finish(j->ctx, j->row, j->live, j->user, j->start, j->end, j->k, NULL);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_scan error %d: %s", j->rc, p_pie_last_error(j->ctx));
}

/* tokenTurnFinish(ctx) -> Promise of tokenTurn's object for the oldest turn begun; the wait runs on the libuv pool */
static napi_value fn_token_turn_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    if (b->tn_n == 0) return throw_state(env, "pie_scan error -6: no token turn was begun");
    const size_t k = b->tn_k[b->tn_head];
    lookup_job *j = (lookup_job *)calloc(1, sizeof *j);
    if (!j) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    napi_value out, promise;
    if (napi_create_object(env, &out) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: result object");
        return NULL;
    }
    j->ctx = ctx;
    j->box = b;
    j->k = k;
    j->row = token_out(env, out, "row", napi_int32_array, 4, k);
    j->live = token_out(env, out, "live", napi_uint8_array, 1, k);
    j->user = token_out(env, out, "user", napi_int32_array, 4, k);
    j->start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    j->end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    if (!j->row || !j->live || !j->user || !j->start || !j->end) {
        free(j);
        return NULL;
    }
    if (napi_create_reference(env, out, 1, &j->result) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: promise");
        return NULL;
    }
    if (!queue_promise_job(env, b, "pie_token_turn_finish", turn_exec, lookup_done, j, &j->work)) {
        napi_delete_reference(env, j->result);
        free(j);
        return NULL;
    }
    b->tn_head = (b->tn_head + 1) % 4; /* the library returns the slot whatever the wait says (cap = k: never PIE_E_CAPACITY) */
    b->tn_n--;
    return promise;
}

/* ---- the expired queue beside scans and batches (pie_expired_queue_begin / _finish / _room) ---------------------------------
 * expiredQueueBegin queues the pass on its own stream and returns; expiredQueueFinish waits for it on the libuv pool (the handle
 * is busy meanwhile) and resolves a Promise of the queue, so a purge tick never blocks the event loop or drains the batches. */

/* expiredQueueBegin(ctx, prevNow, now, capRows) -> capRows */
static napi_value fn_expired_queue_begin(napi_env env, napi_callback_info info)
{
    ARGS(4)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    int64_t prev, now, cap;
    if (!get_i64(env, argv[1], &prev) || !get_i64(env, argv[2], &now) || !get_i64(env, argv[3], &cap) || cap < 0) {
        napi_throw_type_error(env, NULL, "expiredQueueBegin(ctx, prevNow, now, capRows)");
        return NULL;
    }
    int rc = p_pie_expired_queue_begin(ctx, prev, now, (size_t)cap);
    if (rc) return throw_pie(env, ctx, rc);
    b->eq_cap = (size_t)cap;
    b->eq_begun = 1;
    return js_int(env, cap);
}

/* expiredQueueRoom(ctx) -> 1 when expiredQueueBegin would be taken now, else 0 */
static napi_value fn_expired_queue_room(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    return js_int(env, p_pie_expired_queue_room(ctx));
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    pie_ctx *ctx;
    ctx_box *box;
    size_t cap, q;
    int32_t *rows;
    int rc;
    char err[600];
} expq_job;

static void expq_exec(napi_env env, void *data)
{
    (void)env;
    expq_job *j = (expq_job *)data;
    j->rc = p_pie_expired_queue_finish(j->ctx, j->cap ? j->rows : NULL, j->cap, &j->q);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_scan error %d: %s", j->rc, p_pie_last_error(j->ctx));
}

static void expq_done(napi_env env, napi_status status, void *data)
{
    expq_job *j = (expq_job *)data;
    j->box->busy = 0;
    napi_value out = NULL, buf;
    void *mem = NULL;
    const size_t rows = j->q < j->cap ? j->q : j->cap;
    int ok = status == napi_ok && !j->rc;
    if (ok) {
        ok = napi_create_arraybuffer(env, rows * 4, &mem, &buf) == napi_ok &&
             napi_create_typedarray(env, napi_int32_array, rows, buf, 0, &out) == napi_ok;
        if (ok && rows) memcpy(mem, j->rows, rows * 4);
        if (!ok) snprintf(j->err, sizeof j->err, "N-API call failed: result array");
    }
    if (ok) {
        napi_resolve_deferred(env, j->deferred, out);
    } else { /* with the true length when the queue outgrew its room: begin again with room for it */
        reject_with_code(env, j->deferred, j->rc, j->rc || status == napi_ok ? j->err : "expired queue cancelled", (int64_t)j->q);
    }
    napi_delete_async_work(env, j->work);
    free(j->rows);
    free(j);
}

/* expiredQueueFinish(ctx) -> Promise of an Int32Array: the queue begun (empty when the begin said capRows = 0; its `length`
 * rides on the rejection when it outgrew capRows, code -5); the wait runs on the libuv pool */
static napi_value fn_expired_queue_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    pie_ctx *ctx = get_ctx(env, argv[0]);
    if (!ctx) return NULL;
    ctx_box *b = get_box(env, argv[0]);
    if (!b->eq_begun) return throw_state(env, "pie_scan error -6: no expired queue was begun");
    expq_job *j = (expq_job *)calloc(1, sizeof *j);
    if (j) j->rows = (int32_t *)malloc((b->eq_cap ? b->eq_cap : 1) * 4);
    if (!j || !j->rows) {
        free(j);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    napi_value promise;
    j->ctx = ctx;
    j->box = b;
    j->cap = b->eq_cap;
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        free(j->rows);
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: promise");
        return NULL;
    }
    if (!queue_promise_job(env, b, "pie_expired_queue_finish", expq_exec, expq_done, j, &j->work)) {
        free(j->rows);
        free(j);
        return NULL;
    }
    b->eq_begun = 0; /* the library consumes the pass whatever the wait says (cap = capRows: never PIE_E_INVAL) */
    return promise;
}

/* ---- the token column behind the communicator (pie_comm_token_*): keys as tokenLookup takes them, GLOBAL ids out ----------- */
/* commTokenSet(comm, keys) / commTokenAppend(comm, keys) -> k */
static napi_value comm_token_set_or_append(napi_env env, napi_callback_info info, int append)
{
    ARGS(2)
    comm_box *cbx = get_comm_box(env, argv[0]); /* refuses while scanAsync runs on one of the shard contexts */
    if (!cbx) return NULL;
    size_t k = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int rc = append ? p_pie_comm_token_append(cbx->comm, keys, k) : p_pie_comm_token_set(cbx->comm, keys, k);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return js_int(env, (int64_t)k);
}
static napi_value fn_comm_token_set(napi_env env, napi_callback_info info) { return comm_token_set_or_append(env, info, 0); }
static napi_value fn_comm_token_append(napi_env env, napi_callback_info info) { return comm_token_set_or_append(env, info, 1); }

/* commTokenLookup(comm, keys, now) -> tokenLookup's object with global row and user, plus owner Int32Array (the rank that
 * answered, -1: no shard holds the key) */
static napi_value fn_comm_token_lookup(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0;
    int64_t now = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    if (!get_i64(env, argv[2], &now)) {
        napi_throw_type_error(env, NULL, "commTokenLookup(comm, BigUint64Array keys, now)");
        return NULL;
    }
    napi_value out;
    CHECK(env, napi_create_object(env, &out));
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    int32_t *owner = token_out(env, out, "owner", napi_int32_array, 4, k);
    if (!row || !live || !user || !start || !end || !owner) return NULL;
    int rc = p_pie_comm_token_lookup(cbx->comm, keys, k, now, row, live, user, start, end, owner);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return out;
}

/* commTokenTurn(comm, keys, nows, newEnds, kinds) -> tokenTurn's object with global row and user, plus owner Int32Array */
static napi_value fn_comm_token_turn(napi_env env, napi_callback_info info)
{
    ARGS(5)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0;
    pie_turn_op *ops = turn_ops(env, argv + 1, "commTokenTurn(comm, BigUint64Array keys, BigInt64Array nows, BigInt64Array newEnds, Uint8Array kinds)", &k);
    if (!ops) return NULL;
    napi_value out;
    if (napi_create_object(env, &out) != napi_ok) {
        free(ops);
        napi_throw_error(env, NULL, "N-API call failed: result object");
        return NULL;
    }
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    int32_t *owner = token_out(env, out, "owner", napi_int32_array, 4, k);
    if (!row || !live || !user || !start || !end || !owner) {
        free(ops);
        return NULL;
    }
    int rc = p_pie_comm_token_turn(cbx->comm, ops, k, row, live, owner, user, start, end);
    free(ops);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return out;
}

/* commSessionTurn(comm, keys, nows, newEnds, kinds, users Int32Array, discs Int32Array, nUsers) -> commTokenTurn's object; kind 3
 * creates a session of users[i] / discs[i] (GLOBAL ids, read at creates only) on the shard that owns the user (pie_comm_session_turn) */
static napi_value fn_comm_session_turn(napi_env env, napi_callback_info info)
{
    static const char usage[] = "commSessionTurn(comm, BigUint64Array keys, BigInt64Array nows, BigInt64Array newEnds, Uint8Array kinds, Int32Array users, Int32Array discs, nUsers)";
    ARGS(8)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0, ku = 0, kd = 0;
    int32_t n_users = 0;
    int32_t *users = typed(env, argv[5], napi_int32_array, &ku);
    int32_t *discs = typed(env, argv[6], napi_int32_array, &kd);
    if (!users || !discs || napi_get_value_int32(env, argv[7], &n_users) != napi_ok) {
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    pie_turn_op *ops = turn_ops(env, argv + 1, usage, &k);
    if (!ops) return NULL;
    napi_value out;
    if (ku != k || kd != k || napi_create_object(env, &out) != napi_ok) {
        free(ops);
        napi_throw_type_error(env, NULL, usage);
        return NULL;
    }
    int32_t *row = token_out(env, out, "row", napi_int32_array, 4, k);
    uint8_t *live = token_out(env, out, "live", napi_uint8_array, 1, k);
    int32_t *user = token_out(env, out, "user", napi_int32_array, 4, k);
    int64_t *start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    int64_t *end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    int32_t *owner = token_out(env, out, "owner", napi_int32_array, 4, k);
    if (!row || !live || !user || !start || !end || !owner) {
        free(ops);
        return NULL;
    }
    int rc = p_pie_comm_session_turn(cbx->comm, ops, k, users, discs, n_users, row, live, owner, user, start, end);
    free(ops);
    if (rc) return throw_comm(env, cbx->comm, rc);
    return out;
}

/* commTokenSetEnd(comm, keys, newEnd BigInt64Array, now) -> Int32Array global rows written (-1: not found, or not live at `now`) */
static napi_value fn_comm_token_set_end(napi_env env, napi_callback_info info)
{
    ARGS(4)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0, k2 = 0;
    int64_t now = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int64_t *ne = typed(env, argv[2], napi_bigint64_array, &k2);
    if (!ne || k2 != k || !get_i64(env, argv[3], &now)) {
        napi_throw_type_error(env, NULL, "commTokenSetEnd(comm, BigUint64Array keys, BigInt64Array newEnd, now)");
        return NULL;
    }
    napi_value buf, out;
    void *data = NULL;
    CHECK(env, napi_create_arraybuffer(env, k * 4, &data, &buf));
    int rc = p_pie_comm_token_set_end(cbx->comm, keys, ne, k, now, (int32_t *)data);
    if (rc) return throw_comm(env, cbx->comm, rc);
    CHECK(env, napi_create_typedarray(env, napi_int32_array, k, buf, 0, &out));
    return out;
}

/* ---- token lookups and the purge tick while steps are in flight (pie_comm_token_lookup_begin / _finish / _room,
 * pie_comm_expired_queue_begin / _finish / _room).  A begin queues the work on every local shard's side stream and returns; a finish
 * waits on the libuv pool and resolves a Promise, so neither the event loop nor the steps in flight wait for it.  The communicator
 * and the contexts handed out by commCtx are busy meanwhile (one thread per communicator). */
static void comm_set_busy(comm_box *cb, int v)
{
    cb->busy = v;
    for (ctx_box *b = cb->boxes; b; b = b->next) b->busy = v;
}

static int queue_comm_job(napi_env env, comm_box *cb, const char *name, napi_async_execute_callback exec, napi_async_complete_callback done,
                          void *job, napi_async_work *work)
{
    napi_value res;
    napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &res);
    comm_set_busy(cb, 1);
    if (napi_create_async_work(env, NULL, res, exec, done, job, work) == napi_ok && napi_queue_async_work(env, *work) == napi_ok) return 1;
    comm_set_busy(cb, 0);
    napi_throw_error(env, NULL, "cannot queue async work");
    return 0;
}

/* commTokenLookupBegin(comm, keys, nows BigInt64Array: one clock per key) -> k */
static napi_value fn_comm_token_lookup_begin(napi_env env, napi_callback_info info)
{
    ARGS(3)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    size_t k = 0, kn = 0;
    uint64_t *keys = token_keys(env, argv[1], &k);
    if (!keys) return NULL;
    int64_t *nows = typed(env, argv[2], napi_bigint64_array, &kn);
    if (!nows || kn != k) {
        napi_throw_type_error(env, NULL, "commTokenLookupBegin(comm, BigUint64Array keys, BigInt64Array nows): one clock per key");
        return NULL;
    }
    if (cbx->lk_n >= 4) return throw_state(env, "pie_comm error -6: four token lookups are begun and not finished");
    int rc = p_pie_comm_token_lookup_begin(cbx->comm, keys, nows, k);
    if (rc) return throw_comm(env, cbx->comm, rc);
    cbx->lk_k[(cbx->lk_head + cbx->lk_n) % 4] = k;
    cbx->lk_n++;
    return js_int(env, (int64_t)k);
}

/* commTokenLookupRoom(comm) -> lookups commTokenLookupBegin would take now */
static napi_value fn_comm_token_lookup_room(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    return js_int(env, p_pie_comm_token_lookup_room(cbx->comm));
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref result;
    comm_box *box;
    size_t k;
    int32_t *row, *user, *owner;
    uint8_t *live;
    int64_t *start, *end;
    int rc;
    char err[600];
} comm_lookup_job;

static void comm_lookup_exec(napi_env env, void *data)
{
    (void)env;
    comm_lookup_job *j = (comm_lookup_job *)data;
    j->rc = p_pie_comm_token_lookup_finish(j->box->comm, j->row, j->live, j->user, j->start, j->end, j->owner, j->k, NULL);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_comm error %d: %s", j->rc, p_pie_comm_last_error(j->box->comm));
}

static void comm_lookup_done(napi_env env, napi_status status, void *data)
{
    comm_lookup_job *j = (comm_lookup_job *)data;
    comm_set_busy(j->box, 0);
    napi_value out;
    if (status != napi_ok || j->rc) {
        reject_with_code(env, j->deferred, j->rc, j->rc ? j->err : "token lookup cancelled", -1);
    } else {
        napi_get_reference_value(env, j->result, &out);
        napi_resolve_deferred(env, j->deferred, out);
    }
    napi_delete_reference(env, j->result);
    napi_delete_async_work(env, j->work);
    free(j);
}

/* commTokenLookupFinish(comm) -> Promise of commTokenLookup's object for the oldest lookup begun; the wait runs on the libuv pool */
static napi_value fn_comm_token_lookup_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    if (cbx->lk_n == 0) return throw_state(env, "pie_comm error -6: no token lookup was begun");
    const size_t k = cbx->lk_k[cbx->lk_head];
    comm_lookup_job *j = (comm_lookup_job *)calloc(1, sizeof *j);
    if (!j) {
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    napi_value out, promise;
    if (napi_create_object(env, &out) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: result object");
        return NULL;
    }
    j->box = cbx;
    j->k = k;
    j->row = token_out(env, out, "row", napi_int32_array, 4, k);
    j->live = token_out(env, out, "live", napi_uint8_array, 1, k);
    j->user = token_out(env, out, "user", napi_int32_array, 4, k);
    j->start = token_out(env, out, "start", napi_bigint64_array, 8, k);
    j->end = token_out(env, out, "end", napi_bigint64_array, 8, k);
    j->owner = token_out(env, out, "owner", napi_int32_array, 4, k);
    if (!j->row || !j->live || !j->user || !j->start || !j->end || !j->owner) {
        free(j);
        return NULL;
    }
    if (napi_create_reference(env, out, 1, &j->result) != napi_ok || napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: promise");
        return NULL;
    }
    if (!queue_comm_job(env, cbx, "pie_comm_token_lookup_finish", comm_lookup_exec, comm_lookup_done, j, &j->work)) {
        napi_delete_reference(env, j->result);
        free(j);
        return NULL;
    }
    cbx->lk_head = (cbx->lk_head + 1) % 4; /* the library returns the slots whatever the waits say (cap = k: never PIE_E_CAPACITY) */
    cbx->lk_n--;
    return promise;
}

/* commExpiredQueueBegin(comm, prevNow, now, capRows) -> capRows */
static napi_value fn_comm_expired_queue_begin(napi_env env, napi_callback_info info)
{
    ARGS(4)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    int64_t prev, now, cap;
    if (!get_i64(env, argv[1], &prev) || !get_i64(env, argv[2], &now) || !get_i64(env, argv[3], &cap) || cap < 0) {
        napi_throw_type_error(env, NULL, "commExpiredQueueBegin(comm, prevNow, now, capRows)");
        return NULL;
    }
    int rc = p_pie_comm_expired_queue_begin(cbx->comm, prev, now, (size_t)cap);
    if (rc) return throw_comm(env, cbx->comm, rc);
    cbx->eq_cap = (size_t)cap;
    cbx->eq_begun = 1;
    return js_int(env, cap);
}

/* commExpiredQueueRoom(comm) -> 1 when commExpiredQueueBegin would be taken now, else 0 */
static napi_value fn_comm_expired_queue_room(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    return js_int(env, p_pie_comm_expired_queue_room(cbx->comm));
}

typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    comm_box *box;
    size_t cap, q;
    int32_t *rows, *owner; /* one block: rows[cap] then owner[cap] */
    int rc;
    char err[600];
} comm_expq_job;

static void comm_expq_exec(napi_env env, void *data)
{
    (void)env;
    comm_expq_job *j = (comm_expq_job *)data;
    j->rc = p_pie_comm_expired_queue_finish(j->box->comm, j->cap ? j->rows : NULL, j->cap ? j->owner : NULL, j->cap, &j->q);
    if (j->rc) snprintf(j->err, sizeof j->err, "pie_comm error %d: %s", j->rc, p_pie_comm_last_error(j->box->comm));
}

static int comm_expq_array(napi_env env, napi_value out, const char *name, const int32_t *src, size_t n)
{
    napi_value buf, arr;
    void *mem = NULL;
    if (napi_create_arraybuffer(env, n * 4, &mem, &buf) != napi_ok || napi_create_typedarray(env, napi_int32_array, n, buf, 0, &arr) != napi_ok) return 0;
    if (n) memcpy(mem, src, n * 4);
    return napi_set_named_property(env, out, name, arr) == napi_ok;
}

static void comm_expq_done(napi_env env, napi_status status, void *data)
{
    comm_expq_job *j = (comm_expq_job *)data;
    comm_set_busy(j->box, 0);
    napi_value out = NULL;
    const size_t rows = j->q < j->cap ? j->q : j->cap;
    int ok = status == napi_ok && !j->rc;
    if (ok) {
        ok = napi_create_object(env, &out) == napi_ok && comm_expq_array(env, out, "rows", j->rows, rows) &&
             comm_expq_array(env, out, "owner", j->owner, rows);
        if (!ok) snprintf(j->err, sizeof j->err, "N-API call failed: result arrays");
    }
    if (ok) {
        napi_resolve_deferred(env, j->deferred, out);
    } else { /* with the true length when the queue outgrew its room: begin again with room for it */
        reject_with_code(env, j->deferred, j->rc, j->rc || status == napi_ok ? j->err : "expired queue cancelled", (int64_t)j->q);
    }
    napi_delete_async_work(env, j->work);
    free(j->rows);
    free(j);
}

/* commExpiredQueueFinish(comm) -> Promise of {rows Int32Array, owner Int32Array}: the merged queue in global rows and the rank that
 * holds each (both empty when the begin said capRows = 0; the true `length` rides on the rejection when the queue outgrew
 * capRows, code -5); the wait runs on the libuv pool */
static napi_value fn_comm_expired_queue_finish(napi_env env, napi_callback_info info)
{
    ARGS(1)
    comm_box *cbx = get_comm_box(env, argv[0]);
    if (!cbx) return NULL;
    if (!cbx->eq_begun) return throw_state(env, "pie_comm error -6: no expired queue was begun");
    comm_expq_job *j = (comm_expq_job *)calloc(1, sizeof *j);
    if (j) j->rows = (int32_t *)malloc((cbx->eq_cap ? cbx->eq_cap : 1) * 8);
    if (!j || !j->rows) {
        free(j);
        napi_throw_error(env, NULL, "out of memory");
        return NULL;
    }
    napi_value promise;
    j->box = cbx;
    j->cap = cbx->eq_cap;
    j->owner = j->rows + (cbx->eq_cap ? cbx->eq_cap : 1);
    if (napi_create_promise(env, &j->deferred, &promise) != napi_ok) {
        free(j->rows);
        free(j);
        napi_throw_error(env, NULL, "N-API call failed: promise");
        return NULL;
    }
    if (!queue_comm_job(env, cbx, "pie_comm_expired_queue_finish", comm_expq_exec, comm_expq_done, j, &j->work)) {
        free(j->rows);
        free(j);
        return NULL;
    }
    cbx->eq_begun = 0; /* the library consumes the queue whatever the waits say (cap = capRows: never PIE_E_INVAL) */
    return promise;
}

static napi_value init(napi_env env, napi_value exports)
{
    static const struct {
        const char *name;
        napi_callback fn;
    } table[] = {
        {"open", fn_open}, {"deviceCount", fn_device_count}, {"ctxCreate", fn_ctx_create}, {"ctxDestroy", fn_ctx_destroy},
        {"loadColumns", fn_load_columns}, {"appendRows", fn_append_rows}, {"genSynthetic", fn_gen},
        {"readColumns", fn_read_columns}, {"saveColumns", fn_save_columns}, {"loadColumnsDir", fn_load_columns_dir}, {"setEnd", fn_set_end}, {"compactRows", fn_compact_rows}, {"compactMaps", fn_compact_maps}, {"compactTranslate", fn_compact_translate}, {"deleteUser", fn_delete_user}, {"deleteUsers", fn_delete_users}, {"retentionPurgeTz", fn_retention_purge_tz},
        {"setDisciplines", fn_set_disc}, {"scan", fn_scan}, {"scanDevice", fn_scan_device}, {"userFeed", fn_user_feed}, {"scanAsync", fn_scan_async}, {"fetchRows", fn_fetch_rows},
        {"expiredQueue", fn_expired_queue}, {"archiveQueue", fn_archive_queue}, {"serializeEvents", fn_serialize_events}, {"serializeICal", fn_serialize_ical}, {"stats", fn_stats}, {"setProfiling", fn_set_profiling},
        {"setOrderedRun", fn_set_ordered_run}, {"setWideOrdered", fn_set_wide_ordered}, {"setTurnOrdered", fn_set_turn_ordered}, {"tableInfo", fn_table_info}, {"wideUnionRows", fn_wide_union_rows}, {"setBatchLanes", fn_set_batch_lanes},
        {"serializeCsv", fn_serialize_csv}, {"scanBatch", fn_scan_batch}, {"scanWide", fn_scan_wide}, {"batchUserFeed", fn_batch_user_feed}, {"batchFetchRequests", fn_batch_fetch_requests},
        {"commCreate", fn_comm_create}, {"commDestroy", fn_comm_destroy}, {"commWorld", fn_comm_world}, {"commCtx", fn_comm_ctx},
        {"commGenSyntheticSharded", fn_comm_gen}, {"commScanBatchGather", fn_comm_scan_gather}, {"commReadGathered", fn_comm_read}, {"commUPad", fn_comm_upad},
        {"commNeededCap", fn_comm_needed_cap}, {"commStepReserve", fn_comm_step_reserve}, {"commStepBegin", fn_comm_step_begin},
        {"commStepFinish", fn_comm_step_finish}, {"commStepCollect", fn_comm_step_collect}, {"commStepReadGathered", fn_comm_step_read},
        {"commStepUPad", fn_comm_step_upad}, {"commWideStepReserve", fn_comm_wide_step_reserve}, {"commWideStepBegin", fn_comm_wide_step_begin},
        {"commWideStepFinish", fn_comm_wide_step_finish}, {"commWideStepCollect", fn_comm_wide_step_collect},
        {"commWideStepStatus", fn_comm_wide_step_status}, {"commWideStepReadGathered", fn_comm_wide_step_read}, {"commExpiredQueue", fn_comm_expired_queue}, {"commArchiveQueue", fn_comm_archive_queue},
        {"commAppendRows", fn_comm_append_rows}, {"commSetEnd", fn_comm_set_end}, {"commDeleteUser", fn_comm_delete_user}, {"commDeleteUsers", fn_comm_delete_users}, {"commPruneBefore", fn_comm_prune_before}, {"commRetentionPurge", fn_comm_retention_purge}, {"commCompactRows", fn_comm_compact_rows}, {"commTableSize", fn_comm_table_size},
        {"shardMaps", fn_shard_maps},
        {"tokenSet", fn_token_set}, {"tokenAppend", fn_token_append}, {"tokenLookup", fn_token_lookup}, {"tokenSetEnd", fn_token_set_end},
        {"tokenTurn", fn_token_turn}, {"sessionTurn", fn_session_turn}, {"commTokenTurn", fn_comm_token_turn},
        {"commSessionTurn", fn_comm_session_turn},
        {"commTokenSet", fn_comm_token_set}, {"commTokenAppend", fn_comm_token_append}, {"commTokenLookup", fn_comm_token_lookup},
        {"commTokenSetEnd", fn_comm_token_set_end},
        {"scanBatchBegin", fn_scan_batch_begin}, {"scanBatchFinish", fn_scan_batch_finish}, {"tokenLookupBegin", fn_token_lookup_begin},
        {"tokenLookupFinish", fn_token_lookup_finish}, {"tokenLookupRoom", fn_token_lookup_room},
        {"tokenTurnBegin", fn_token_turn_begin}, {"tokenTurnFinish", fn_token_turn_finish}, {"tokenTurnRoom", fn_token_turn_room},
        {"expiredQueueBegin", fn_expired_queue_begin}, {"expiredQueueFinish", fn_expired_queue_finish}, {"expiredQueueRoom", fn_expired_queue_room},
        {"commTokenLookupBegin", fn_comm_token_lookup_begin}, {"commTokenLookupFinish", fn_comm_token_lookup_finish},
        {"commTokenLookupRoom", fn_comm_token_lookup_room}, {"commExpiredQueueBegin", fn_comm_expired_queue_begin},
        {"commExpiredQueueFinish", fn_comm_expired_queue_finish}, {"commExpiredQueueRoom", fn_comm_expired_queue_room},
    };
    for (size_t i = 0; i < sizeof table / sizeof table[0]; ++i) {
        napi_value fn;
        if (napi_create_function(env, table[i].name, NAPI_AUTO_LENGTH, table[i].fn, NULL, &fn) != napi_ok) return NULL;
        napi_set_named_property(env, exports, table[i].name, fn);
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
