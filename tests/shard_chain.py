"""TEST INFRASTRUCTURE — the seeded chain over the GLOBAL-ID half of the C ABI: every pie_shard_* call (appends, touches and
deletes by global id, the sharded token column and its turns, prune / retention by global row, the in-flight shard forms) and
pie_compact_rows on single shards, each in the state the others leave behind.  tests/table_model.Chain covers the scan half and
tests/store_chain.StoreChain the session-store half, both on plain contexts; this one drives `world` sharded contexts of one GPU.

ShardStoreModel is ONE unsharded table — a tests/store_chain.StoreModel — with the owner of every user and, per rank, the global
rows that rank's own compactions dropped (the shape of tests/shard_token_model.ShardTokenModel, which it extends).  Everything
expected of rank r is derived from that table: its rows, its user map, its columns, covered_g / covered_l, its keys, its answers.
Two host-side sizes are mirrored per rank because they depend on the history: the slot count (pie_token_slots_for(local rows) at a
set and after a compaction that moved rows; the token append that follows the local row count passing half the slots rebuilds
into the next size) and the column capacity (a shard fits exactly, an append that outgrows it doubles it, PIE_COMPACT_SHRINK
re-sizes to the kept rows).  A row a shard dropped is gone from the table the shards make up together: the model tombstones it,
takes its key out of the unsharded index and lets no touch revive it, so that `tm` is "the unsharded table less the dropped rows".

ShardChain(pie or None, oracle, seed) drives the contexts and the model side by side, or — pie = None — the model alone with the
very same random draws (no draw depends on the device).  Every context is given the same call with the same arrays.  The model is
the only source of expected values; the first difference raises, tagged with seed, step and op.  Nothing here needs a GPU to
import."""
import ctypes as C

import numpy as np

from shard_token_model import ShardTokenModel, merge
from store_chain import MAX_ROWS, TILE_USERS, StoreChain, StoreModel, slots_for
from table_model import ALL, DAY, HOUR, INT64_MIN, PIE_E_STATE, add_months, ctx_with_env, same, shard_owner, shard_view
from token_model import END_NONE, check_layout
from turn_model import TurnModel, same_turn

PIE_E_INVAL, PIE_E_CAPACITY = -1, -5
ZONE = "Europe/Berlin"       # the zone table of tests/test_gpu_shard_maint.py
SMALL_ROWS = 5000            # tables up to this size run the readers after every step, larger ones every third step

# what a chain can arrive at; test_shard_chains_reached_every_state wants each of them seen on the device
STATES = (
    "touch_of_dropped_row",                              # pie_shard_set_end names a global row a compaction dropped
    "token_append_after_compact_with_uncovered_tail",    # covered_g < N_g across a compaction that dropped rows, then the keys land
    "lookup_key_on_dropped_row",
    "slots_doubled_on_one_rank_only",
    "capacity_outgrown_under_lookup_begun",              # a shard's columns and maps re-allocated with a lookup begun on it
    "user_without_rows_then_deleted",                    # pie_shard_append_rows(k = 0) made the user, pie_shard_delete_user names it
    "first_user_of_empty_rank",
    "compact_one_rank_then_delete_users",
    "compact_shrink_then_burst_append",
    "maint_list_over_cap",
    "turn_on_live_hot_index_then_batch",
    "plain_turn_kept_ordered_run",
    "refused_turn_begin_on_ordered_run",
    "inflight_turn_after_reshape",
    "inflight_lookup_after_reshape",
    "inflight_purge_after_reshape",
    "duplicate_key_resolved_by_merge",
    "refused_mutator_while_batch_in_flight",
    "refused_mutator_while_turn_begun",
)
# decided by the device alone (the hot index and the ordered run); the model-only run records a stand-in for the ordered run's
DEVICE_STATES = ("turn_on_live_hot_index_then_batch", "plain_turn_kept_ordered_run", "refused_turn_begin_on_ordered_run")
HOST_STATES = tuple(s for s in STATES if s not in DEVICE_STATES) + ("host:turn_begin_in_ordered_chain",)
# ... and what the chains that log in through pie_shard_session_turn (cfg["logins"]) add
LOGIN_STATES = (
    "shard_create_after_one_rank_compacted",             # the last compaction that dropped rows left some rank alone
    "shard_create_doubled_slots_on_one_rank",
    "shard_create_outgrew_capacity_on_one_rank",
    "shard_create_first_user_of_empty_rank",
    "shard_create_over_dropped_rows_key",                # a create under the key of a row a shard's compaction dropped
    "shard_create_kept_by_no_live_rank_row",             # a rank that keeps no create of the turn and answers -1 for all of them
    "shard_create_refused_short_column",                 # covered_g < N_g: PIE_E_STATE on every rank, nothing changed
    "shard_turn_kept_ordered_run_on_keeping_rank_only",  # pie_set_turn_ordered: the keeping rank's run took the rows, another's is untouched
    "shard_turn_create_with_lookup_begun",               # a lookup begun on one rank lands first (the header's rule), then the turn
    "shard_turn_refused_on_one_rank_with_batch",         # PIE_E_STATE on the rank with a batch in flight, nothing changed there
)
LOGIN_DEVICE_STATES = ("shard_turn_kept_ordered_run_on_keeping_rank_only",)
LOGIN_HOST_STATES = tuple(s for s in LOGIN_STATES if s not in LOGIN_DEVICE_STATES)
# the stand-ins StoreChain.do_logins records on its way (this chain inherits it)
LOGIN_STAND_INS = ("host:login_landed_uncovered_tail", "host:login_full_segment", "host:login_chain_of_one_user")

_TZ = {}


def zone_table(oracle):
    if "t" not in _TZ:
        _TZ["t"] = oracle.tz_table(ZONE, oracle.T0_MS - 3 * 365 * DAY, oracle.T0_MS + 3 * 365 * DAY)
    return _TZ["t"]


# ------------------------------------------------------------------------------------------------ the model
class ShardStoreModel(ShardTokenModel):
    """tm = the unsharded StoreModel; owner[user]; dropped[rank][global row]; slots[rank], cap[rank] (see the module's text)."""

    def __init__(self, oracle, start, end, user, disc, U, D, world):
        self.oracle, self.world = oracle, int(world)
        self.tm = StoreModel(oracle, start, end, user, disc, U, D)
        self.owner = shard_owner(oracle, np.zeros(0, np.int32), int(U), self.world)
        self.dropped = [np.zeros(self.N, bool) for _ in range(self.world)]
        self.cap = [max(int(self.held(r).size), 1) for r in range(self.world)]
        self.slots = [0] * self.world
        self._idx = None

    # ---- derived
    @property
    def U(self):
        return self.tm.U

    @property
    def gone(self):
        return np.logical_or.reduce(self.dropped)

    def users_of(self, rank):
        return np.nonzero(self.owner[:self.U] == rank)[0].astype(np.int32)

    def view(self, rank):
        """-> (the shard as a TableModel in local ids, its global rows ascending, its global users ascending)"""
        v, rows, users = shard_view(self.tm, rank, self.owner)
        keep = ~self.dropped[rank][rows]
        v.load(v.start[keep], v.end[keep], v.user[keep], v.disc[keep], v.U, v.D)
        return v, rows[keep], users

    def split(self, rows):
        """a list of global rows -> the part every rank holds"""
        own = self.owner[self.tm.user[rows]]
        return [rows[own == r] for r in range(self.world)]

    def indexes(self):
        """per rank {key: the largest global row under it that the rank holds and the column covers}: what
        ShardTokenModel.shard_lookup builds per call, kept until the column or the dropped rows change"""
        if self._idx is None:
            tm, cov = self.tm, self.tm.covered
            idx = [dict() for _ in range(self.world)]
            for g, (k, o, x) in enumerate(zip(tm.keys.tolist(), self.owner[tm.user[:cov]].tolist(), self.gone[:cov].tolist())):
                if not x:
                    idx[o][(k[0], k[1])] = g
            self._idx = idx
        return self._idx

    def rank_rows(self, rank, keys):
        idx = self.indexes()[rank]
        return np.array([idx.get((k[0], k[1]), -1) for k in np.asarray(keys, np.uint64).reshape(-1, 2).tolist()], np.int32)

    def shard_lookup(self, rank, keys, now):
        return self._answer(self.rank_rows(rank, keys), now)

    def lookup(self, keys, now):
        """the unsharded table's answer (less the dropped rows)"""
        return self.tm.lookup(keys, now)

    def _reindex(self):
        tm, gone = self.tm, self.gone
        tm.index = {}
        for row, k in enumerate(tm.keys.tolist()):
            if not gone[row]:
                tm.index[(k[0], k[1])] = row
        self._idx = None

    # ---- mutators: every one answers what each rank must answer, from the table as it stood before the call
    def append_rows(self, start, end, user, disc, U):
        """-> rows kept per rank"""
        user = np.asarray(user, np.int32)
        self.owner = shard_owner(self.oracle, self.owner, int(U), self.world)
        kept = [int(np.count_nonzero(self.owner[user] == r)) for r in range(self.world)]
        for r in range(self.world):
            n = int(self.held(r).size)
            if kept[r] and n + kept[r] > self.cap[r]:
                self.cap[r] = max(n + kept[r], 2 * self.cap[r])
        self.tm.append_rows(start, end, user, disc)
        self.tm.U = int(U)
        self.dropped = [np.concatenate([x, np.zeros(len(start), bool)]) for x in self.dropped]
        return kept

    def token_set(self, keys):
        self.slots = [slots_for(int(self.held(r).size)) for r in range(self.world)]
        self.tm.token_set(keys)
        self._reindex()

    def token_append(self, keys):
        if len(keys) == 0:
            return
        for r in range(self.world):
            n = int(self.held(r).size)
            if n > 0 and n > self.slots[r] // 2:
                self.slots[r] = slots_for(n)
        covered = self.tm.covered
        self.tm.token_append(keys)
        self._idx = None
        if self.gone[covered:self.tm.covered].any():      # keys of rows a shard dropped before they came: held by nobody
            self._reindex()

    def set_end(self, rows, new_end):
        rows, new_end = np.asarray(rows, np.int64), np.asarray(new_end, np.int64)
        ok = ~self.gone[rows]
        self.tm.set_end(rows[ok], new_end[ok])

    def token_set_end(self, keys, new_end, now):
        return self.shard_set_end(keys, new_end, now)

    def turn(self, ops):
        """pie_shard_token_turn on every rank -> the answers per rank; the ranks' rows are disjoint, so their chains never meet"""
        tm, merged, outs = self.tm, self.tm.index, []
        try:
            for r in range(self.world):
                tm.index = self.indexes()[r]
                outs.append(TurnModel.turn(tm, ops))
        finally:
            tm.index = merged
        return outs

    def session_turn_plan(self, ops, user_global, U):
        """pie_shard_session_turn_plan's four outputs restated from owner[] -> per rank (new_row_global[k], new_row_local[k],
        creates, creates the rank keeps): the j-th create gets global row N + j on every rank, and on the rank that owns its
        user the local row `rows the rank holds + creates it kept before this one`; -1 everywhere else"""
        from session_turn_model import CREATE
        owner = shard_owner(self.oracle, self.owner, int(U), self.world)
        is_create = ops["kind"] == CREATE
        row_g = np.where(is_create, self.N + np.cumsum(is_create) - 1, -1).astype(np.int32)
        own = np.where(is_create, owner[np.where(is_create, np.asarray(user_global, np.int64), 0)], -1)
        out = []
        for r in range(self.world):
            mine = own == r
            row_l = np.where(mine, int(self.held(r).size) + np.cumsum(mine) - 1, -1).astype(np.int32)
            out.append((row_g, row_l, int(is_create.sum()), int(mine.sum())))
        return out

    def session_turn(self, ops, user_global, disc, U=None):
        """pie_shard_session_turn on every rank -> the answers per rank.  The header's defining equivalence, op by op: a CREATE is
        pie_shard_append_rows of one row and pie_shard_token_append of its key (the rank that owns the user answers the GLOBAL
        row, every other rank -1 / live 0 / END_NONE / user -1), every other op a pie_shard_token_turn of one op on every rank.
        The unsharded StoreModel decides rows, liveness and ends.  The two mirrored sizes follow the turn's own room rule, made
        once for the whole call: local rows + kept creates against the capacity, and against half the slots."""
        from session_turn_model import CREATE
        U = self.U if U is None else int(U)
        k = ops.shape[0]
        plan = self.session_turn_plan(ops, user_global, U)
        cap, slots = list(self.cap), list(self.slots)
        for r in range(self.world):
            n, kept = int(self.held(r).size), plan[r][3]
            if kept and n + kept > cap[r]:
                cap[r] = max(n + kept, 2 * cap[r])
            if kept and n + kept > slots[r] // 2:
                slots[r] = slots_for(n + kept)
        outs = [{"row": np.full(k, -1, np.int32), "live": np.zeros(k, np.uint8), "user": np.full(k, -1, np.int32),
                 "start": np.zeros(k, np.int64), "end": np.full(k, END_NONE, np.int64), "found": np.zeros(k, bool)} for _ in range(self.world)]
        at = 0
        while at < k:
            if int(ops[at]["kind"]) == CREATE:
                now, new_end, u = int(ops[at]["now"]), int(ops[at]["new_end"]), int(user_global[at])
                self.append_rows([now], [new_end], [u], [disc[at]], max(U, self.U))
                self.token_append(np.asarray(ops[at]["tok"], np.uint64).reshape(1, 2))
                o = outs[int(self.owner[u])]
                o["row"][at], o["live"][at], o["user"][at], o["start"][at], o["end"][at], o["found"][at] = self.N - 1, new_end > now, u, now, new_end, True
                at += 1
                continue
            to = at
            while to < k and int(ops[to]["kind"]) != CREATE:
                to += 1
            for r, part in enumerate(self.turn(ops[at:to])):
                for col in outs[r]:
                    outs[r][col][at:to] = part[col]
            at = to
        if U > self.U:                                 # (a turn without a create still raises U_g)
            z = np.zeros(0, np.int64)
            self.append_rows(z, z, z.astype(np.int32), z.astype(np.int32), U)
        self.cap, self.slots = cap, slots
        return outs, plan

    def delete_user(self, u):
        rows = self.tm.delete_user(u) if 0 <= u < self.U else np.zeros(0, np.int32)
        return [rows if 0 <= u < self.U and self.owner[u] == r else np.zeros(0, np.int32) for r in range(self.world)]

    def delete_users(self, ids):
        """-> (rows per rank, counts per element per rank)"""
        ids = np.asarray(ids, np.int64)
        union, per = self.tm.delete_users(ids)
        valid = (ids >= 0) & (ids < self.U)
        own = np.where(valid, self.owner[np.where(valid, ids, 0)], -1)
        return self.split(union), [np.where(own == r, per, 0).astype(np.int32) for r in range(self.world)]

    def prune_before(self, cutoff):
        return self.split(self.tm.prune_before(cutoff))

    def retention_purge(self, now, months, tz_offset_ms=0):
        return self.split(self.tm.retention_purge(now, months, tz_offset_ms))

    def retention_purge_tz(self, now, months, table):
        rows = self.oracle.retention_queue_tz(self.tm.start, self.tm.end, now, months, *table)
        self.tm.end[rows] = END_NONE
        return self.split(rows)

    def expired_queue(self, prev_now, now):
        return self.split(self.tm.expired_queue(prev_now, now))

    def purge(self, now):
        return self.tm.purge(now)

    def compact(self, rank, dead_before=END_NONE, shrink=False):
        """pie_compact_rows on ONE shard -> (rows it holds now, rows it dropped)"""
        n_old = int(self.held(rank).size)
        before = self.dropped[rank].copy()
        kept = int(ShardTokenModel.compact(self, rank, dead_before).size)
        new = self.dropped[rank] & ~before
        if not (kept == n_old and not (shrink and self.cap[rank] > max(kept, 1))):
            self.slots[rank] = slots_for(kept)
            if shrink:
                self.cap[rank] = max(kept, 1)
        if new.any():
            self.tm.end[new] = END_NONE
            self._reindex()
        return kept, int(np.count_nonzero(new))


class ShardModelStore:
    """what tests/session_turn_model.replay_g5_sessions drives, on ShardStoreModel: every turn, logins included, goes through
    ShardStoreModel.session_turn on every rank and is merged by the largest global row"""

    def __init__(self, oracle, n_users, world):
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.sm = ShardStoreModel(oracle, z64, z64, z32, z32, n_users, 1, world)
        self.sm.token_set(np.zeros((0, 2), np.uint64))
        self.U = n_users

    def turn(self, ops, user, disc):
        outs, plan = self.sm.session_turn(ops, user, disc, self.U)
        assert sum(p[3] for p in plan) == plan[0][2], "the ranks keep the creates between them"
        return merge(outs)

    def delete_user(self, u):
        self.sm.delete_user(u)

    def purge(self, now):
        self.sm.purge(now)


# ------------------------------------------------------------------------------------------------ the driver
class CtxDriver:
    """`world` sharded contexts of GPU 0 in one process.  Every op is given to every context with the same arrays and answers
    one result per rank; the chain is written against these names only, so another driver can take their place."""

    def __init__(self, pie, cfg):
        self.pie, self.ctxs = pie, []
        n, U, D = cfg["n"], cfg["U"], cfg["D"]
        try:
            for r in range(cfg["world"]):
                c = ctx_with_env(pie, cfg["hot"], cfg["async"])
                self.ctxs.append(c)
                c.set_ordered_run(cfg["ordered"])
                c.set_turn_ordered(cfg.get("turn_ordered", 0))
                c.set_batch_lanes(cfg["lanes"])
                c.gen_synthetic(cfg["gen_seed"], n, 0, n, U, D, 0)
                c.shard_table(r, cfg["world"])
                c.set_disciplines(ALL, D)
        except Exception:
            self.close()
            raise

    def close(self):
        for c in self.ctxs:
            c.close()

    def each(self, fn):
        return [fn(c) for c in self.ctxs]

    def maint(self, rank, name, args, cap):
        """one of the three listing calls through the raw ABI with room for `cap` rows -> (return code, *n_out)"""
        c = self.ctxs[rank]
        rows, k = np.empty(max(cap, 1), np.int32), C.c_size_t(0)
        p = rows.ctypes.data_as(C.c_void_p)
        if name == "prune":
            rc = c._lib.pie_shard_prune_before(c._ctx, int(args[0]), p, cap, C.byref(k))
        elif name == "retention":
            rc = c._lib.pie_shard_retention_purge(c._ctx, int(args[0]), int(args[1]), int(args[2]), p, cap, C.byref(k))
        else:
            T, off = (np.ascontiguousarray(a, np.int64) for a in args[2])
            rc = c._lib.pie_shard_retention_purge_tz(c._ctx, int(args[0]), int(args[1]), T.ctypes.data_as(C.c_void_p),
                                                     off.ctypes.data_as(C.c_void_p), int(T.shape[0]), p, cap, C.byref(k))
        return rc, int(k.value)


# ------------------------------------------------------------------------------------------------ the chain
def shard_config(seed):
    rng = np.random.default_rng([seed, 0x5A4D])
    world = int(rng.choice([1, 2, 3, 5]))
    U = int(rng.choice([3, 64, 499]))
    n, steps = int(rng.choice([1, 65, 4099, 20000])), int(rng.integers(25, 41))
    if world * n >= 100000:                       # five contexts over the largest table: fewer steps, every check kept
        steps = 25
    return {
        "world": world, "n": n, "U": 7 if world == 5 else U, "D": int(rng.choice([1, 8, 32])),
        "hot": int(rng.integers(2)), "ordered": int(rng.integers(3)), "lanes": int(rng.integers(1, 5)), "async": int(rng.integers(2)),
        "steps": steps, "gen_seed": int(rng.integers(1, 2 ** 60)), "dup": seed % 3 == 0,
    }


def shard_logins_config(seed):
    """the draws of a chain that logs in, from a stream of their own (shard_config's stay what they were): the sizes of the designed
    shard chains, a mode that builds runs more often than not, the switch mostly on"""
    rng = np.random.default_rng([seed, 0x10616])
    return {"n": int(rng.choice([65, 4099])), "hot": 0, "ordered": int(rng.choice([0, 1, 2, 2])), "turn_ordered": int(rng.choice([0, 1, 1, 1]))}


class ShardChain(StoreChain):
    """One seeded chain: `world` shards of one generated table with a token column, a context configuration, 25 to 40 steps (or
    the fixed list `script`).  Every step is one mutator or in-flight form, the state checks on every rank, and the readers."""

    OPS = ("append", "append", "append", "token_append", "set_end", "set_end", "token_set_end", "token_turn", "token_turn",
           "delete_user", "delete_users", "prune", "retention", "retention_tz", "compact", "compact", "compact",
           "inflight_lookup", "inflight_turn", "inflight_purge", "refusals")
    OPS_LOGINS = OPS + ("session_turn", "session_turn", "session_turn", "logins", "logins", "logins_chain", "logins_undo")
    NEW_OPS = ("session_turn", "logins", "logins_chain", "logins_undo")

    def __init__(self, pie, oracle, seed, cfg=None, script=None, log=None):
        self.pie, self.oracle, self.seed = pie, oracle, seed
        self.cfg = dict(shard_config(seed), logins=0, turn_ordered=0)
        if (cfg or {}).get("logins"):
            self.cfg.update(shard_logins_config(seed))
            if self.cfg["U"] == 499:
                self.cfg["U"] = 64
        self.cfg.update(cfg or {})
        self.ops = self.OPS_LOGINS if self.cfg["logins"] else self.OPS
        self.since_compact, self.login_since_begin = None, False      # (StoreChain.do_logins' bookkeeping)
        self.script, self.log = script, log
        self.rng = np.random.default_rng([seed, 0x5A4E])
        self.t0 = oracle.T0_MS
        self.world = self.cfg["world"]
        self.drv, self.ctx = None, None
        self.states, self.executed, self.skipped, self.step = {}, {}, 0, -1
        self.issued = np.zeros((0, 2), np.uint64)
        self.pending, self.pending_due = None, 0
        self.reshaped = False                       # a shard compacted or grown earlier in the chain
        self.compacted_with_tail = False            # rows dropped while covered_g < N_g, the keys not landed yet
        self.part_compacted = False                 # the last compaction that dropped rows left some rank alone
        self.shrunk = False                         # the last change of capacity was a PIE_COMPACT_SHRINK that dropped rows
        self.rowless = []                           # users a k = 0 append made and no row names
        self.over_cap_done = False
        self.dup_key = None
        self.turn_on_hot = [None] * self.world      # per rank: hot_builds at a turn that found the index live
        self.seconds = 0.0

    # ---- set-up
    def run(self):
        import time
        c, o, rng = self.cfg, self.oracle, self.rng
        n, U, D = c["n"], c["U"], c["D"]
        s, e, u, d = [a.copy() for a in o.gen(c["gen_seed"], n, 0, n, U, D, 0)]
        sm = self.sm = ShardStoreModel(o, s, e, u, d, U, D, self.world)
        self.m = sm.tm                               # StoreChain's helpers (clocks, queries, keys) read the unsharded table
        self.mask = ALL
        self.absent = rng.integers(0, 2 ** 64, (64, 2), dtype=np.uint64)
        keys = rng.integers(0, 2 ** 64, (n, 2), dtype=np.uint64)
        t_start = time.perf_counter()
        if self.pie is not None:
            self.drv = CtxDriver(self.pie, c)
        try:
            if self.drv:
                self.drv.each(lambda x: x.shard_token_set(keys))
            sm.token_set(keys)
            self.issued = keys
            steps = len(self.script) if self.script else c["steps"]
            for step in range(-1, steps):
                self.step = step
                op = "load" if step < 0 else self.script[step] if self.script else str(rng.choice(self.ops))
                tag = "seed %s world %d step %d %s" % (self.seed, self.world, step, op)
                if self.log:
                    self.log("%s N %d U %d covered %d slots %s cap %s" % (tag, sm.N, sm.U, sm.covered_g, sm.slots, sm.cap))
                skipped = self.skipped
                try:
                    if step >= 0:
                        self.land_pending(tag)
                        getattr(self, "do_" + op)(tag)
                    else:
                        self.check_state(tag)
                    self.readers(tag)
                except AssertionError:
                    raise
                except Exception as exc:      # a refusal or an error of the library: tagged like a difference
                    raise AssertionError((tag, repr(exc))) from exc
                if step >= 0 and self.skipped == skipped:
                    kind = op.split(":")[0]
                    self.executed[kind] = self.executed.get(kind, 0) + 1
        finally:
            if self.drv:
                self.drv.close()
            self.seconds = time.perf_counter() - t_start
        return self

    def __getattr__(self, name):
        # a script names a variant as "op:variant" (do_append:burst): the op with its first choice fixed
        if name.startswith("do_") and ":" in name:
            op, variant = name.split(":", 1)
            return lambda tag: getattr(self, op)(tag, variant)
        raise AttributeError(name)

    # ---- bookkeeping
    def saw(self, state):
        assert state in STATES or state in HOST_STATES or state in LOGIN_STATES or state in LOGIN_STAND_INS, state
        self.states[state] = self.states.get(state, 0) + 1

    def skip(self, tag):
        self.skipped += 1

    def tombstoned_keys(self):
        return np.zeros((0, 2), np.uint64)

    def expect(self, tag, code, fn):
        """`fn(context)` is refused with `code` on every rank"""
        if not self.drv:
            return
        for r, c in enumerate(self.drv.ctxs):
            self.expect_one(tag, code, r, fn)

    def expect_one(self, tag, code, r, fn):
        c = self.drv.ctxs[r]
        n, nu = c.n, c.n_users
        try:
            fn(c)
        except self.pie.PieError as exc:
            assert exc.code == code, (tag, "rank", r, "refused with", exc.code, "not", code)
        else:
            raise AssertionError((tag, "rank", r, "a call the header refuses went through"))
        assert (c.n, c.n_users) == (n, nu)

    def mutators(self):
        """every pie_shard_* mutator, with arguments the idle context would take"""
        sm, t0 = self.sm, self.t0
        one64, one32 = np.full(1, t0, np.int64), np.zeros(1, np.int32)
        key = self.absent[:1]
        ops = np.zeros(1, self.turn_dtype())
        ops["tok"] = key
        return [
            lambda c: c.shard_append_rows(one64, one64 + HOUR, one32, one32, sm.U),
            lambda c: c.shard_set_end(one32, one64),
            lambda c: c.shard_token_append(np.zeros((0, 2), np.uint64)),
            lambda c: c.shard_token_set_end(key, one64, END_NONE),
            lambda c: c.shard_token_turn(ops),
            lambda c: c.shard_delete_user(0),
            lambda c: c.shard_delete_users(one32),
            lambda c: c.shard_prune_before(t0),
            lambda c: c.shard_retention_purge(t0, 2, 0),
            lambda c: c.shard_retention_purge(t0, 2, tz_table=zone_table(self.oracle)),
        ]

    @staticmethod
    def turn_dtype():
        from turn_model import TURN_OP
        return TURN_OP

    # ---- the state of every rank after every mutator
    def check_state(self, tag):
        sm = self.sm
        assert sm.covered_g + (0 if self.pending is None else len(self.pending)) == sm.N, (tag, "the chain lost count of its keys")
        if not self.drv:
            return
        N, U, gone = sm.N, sm.U, sm.gone
        for r, c in enumerate(self.drv.ctxs):
            t = (tag, "rank", r)
            v, rows, users = sm.view(r)
            info = c.shard_info()
            assert (info["rank"], info["world"], info["rows_global"], info["users_global"]) == (r, self.world, N, U), (t, "shard_info", info)
            assert c.n == rows.size and c.n_users == max(users.size, 1), (t, "shape", c.n, c.n_users, rows.size, users.size)
            st = c.stats()
            assert int(st["rows"]) == rows.size and int(st["users"]) == max(users.size, 1), (t, "stats")
            got_rows, got_users = c.shard_maps()
            assert np.array_equal(got_rows, rows), (t, "row map", np.nonzero(got_rows != rows)[0][:8] if got_rows.size == rows.size else (got_rows.size, rows.size))
            assert np.all(np.diff(got_rows) > 0), (t, "the row map ascends")
            assert np.array_equal(got_users[:users.size], users), (t, "user map")
            for name, got, want in zip(("start", "end", "user", "disc"), c.read_columns(), v.columns()):
                assert got.dtype == want.dtype and np.array_equal(got, want), (t, "column " + name, np.nonzero(got != want)[0][:8])
            cg, cl, slots, slot_row, back = c.shard_token_layout()
            assert (cg, cl, slots) == (sm.covered_g, sm.covered_l(r), sm.slots[r]), (t, "layout", cg, cl, slots, sm.covered_g, sm.covered_l(r), sm.slots[r])
            want_keys = sm.shard_keys(r)
            assert np.array_equal(back, want_keys), (t, "the token column", np.nonzero((back != want_keys).any(axis=1))[0][:8])
            if cl:
                check_layout(cl, slots, slot_row, back, self.pie.token_homes(back, int(slots).bit_length() - 1))
            else:
                assert np.all(slot_row < 0), (t, "a slot held by no row")
            ti = c.table_info()
            assert ti["token_rows"] == cl and ti["rows"] == rows.size, (t, "table_info", ti["token_rows"], ti["rows"])
            assert ti["table_bytes"] // 24 == sm.cap[r], (t, "capacity", ti["table_bytes"] // 24, sm.cap[r])
            # translation both ways: rows it holds, rows of other ranks, rows it dropped, rows outside [0, N_g)
            foreign = np.nonzero(sm.owner[sm.tm.user] != r)[0]
            probe = np.concatenate([rows[:16], rows[-4:], rows[rows.size // 2: rows.size // 2 + 4], foreign[:8], foreign[-2:],
                                    np.nonzero(sm.dropped[r])[0][:8], np.nonzero(gone)[0][-4:],
                                    [-1, N, N + 5, N - 1, 0, 2 ** 31 - 1, -(2 ** 31)]]).astype(np.int32)
            is_held = np.isin(probe, rows)
            local = c.shard_rows_to_local(probe)
            assert np.array_equal(local, np.where(is_held, np.searchsorted(rows, probe), -1)), (t, "rows_to_local", probe[local != np.where(is_held, np.searchsorted(rows, probe), -1)][:8])
            assert np.array_equal(c.shard_rows_to_global(local), np.where(is_held, probe, -1)), (t, "rows_to_global")
            edge = np.array([0, rows.size - 1, rows.size, -1, 2 ** 31 - 1], np.int32)
            want_edge = [int(rows[0]) if rows.size else -1, int(rows[-1]) if rows.size else -1, -1, -1, -1]
            assert c.shard_rows_to_global(edge).tolist() == want_edge, (t, "rows_to_global at the ends of the map")

    def lists(self, tag, got, want, total=None):
        """the per-rank lists of a listing call: each ascends and equals the model's, which are pairwise disjoint and whose union
        is the unsharded model's list"""
        allrows = np.concatenate([np.zeros(0, np.int32)] + list(want))
        assert np.unique(allrows).size == allrows.size, (tag, "the model's lists overlap")
        if total is not None:
            assert np.array_equal(np.sort(allrows), total), (tag, "the model's lists are not the unsharded list")
        if got is None:
            return
        for r in range(self.world):
            assert got[r].dtype == np.int32 and np.all(np.diff(got[r]) > 0), (tag, "rank", r, "the list does not ascend")
            assert np.array_equal(got[r], want[r]), (tag, "rank", r, "rows listed", got[r][:8], want[r][:8])

    # ---- readers
    def readers(self, tag):
        rng, sm, drv = self.rng, self.sm, self.drv
        keys = np.concatenate([self.issued, self.absent] + ([self.pending[:8]] if self.pending is not None else []))
        nows = [int(self.clocks(1)[0]), int(self.clocks(1)[0])]
        gone_keyed = sm.gone[:sm.covered_g]
        if gone_keyed.any():
            self.saw("lookup_key_on_dropped_row")
        if self.dup_key is not None and sm.tm.rows_of(self.dup_key)[0] >= 0:
            self.saw("duplicate_key_resolved_by_merge")
        rows = [sm.rank_rows(r, keys) for r in range(self.world)]
        for now in nows:
            per_rank = [sm._answer(rows[r], now) for r in range(self.world)]
            want = sm.lookup(keys, now)
            self.same_lookup(merge(per_rank), want, (tag, "the model's merged lookup is not the unsharded one", now))
            if drv:
                got = drv.each(lambda c: c.shard_token_lookup(keys, now))
                for r in range(self.world):
                    self.same_lookup(got[r], per_rank[r], (tag, "rank", r, "lookup of every key", now))
                    assert np.all(got[r]["row"][~per_rank[r]["found"]] == -1)
                self.same_lookup(merge(got), want, (tag, "merged lookup of every key", now))
        # one scan, one batch of sixteen, one wide batch, the expired queue in both forms: drawn once, asked of every rank
        small = sm.N <= SMALL_ROWS
        kind = str(rng.choice(["sparse", "sparse", "below_p90", "dense", "above"]))
        now, cutoff = self.pick_now(kind), int(rng.choice([INT64_MIN, self.t0 - 61 * DAY]))
        q16, q70 = self.query_set(16, dense=bool(self.step % 2)), self.query_set(70, dense=False)
        xnow = self.pick_now(str(rng.choice(["sparse", "below_p90", "above", "dense"])))
        xprev = xnow - int(rng.integers(0, 3 * DAY)) if xnow > INT64_MIN + 4 * DAY else INT64_MIN
        feeds = [(int(rng.integers(16)), float(rng.random())) for _ in range(3)]
        if not drv or not (small or self.step % 3 == 2 or self.step < 0):
            return
        xwant = sm.expired_queue(xprev, xnow)
        for r, c in enumerate(drv.ctxs):
            t = (tag, "rank", r)
            v, rows, users = sm.view(r)
            same(c.scan(now, cutoff), v.scan(now, cutoff, self.mask), (t, "scan", kind, now, cutoff))
            self.one_batch_on(r, (t, "batch"), q16, False, v, feeds)
            self.one_batch_on(r, (t, "wide"), q70, True, v, [])
            local = c.expired_queue(xprev, xnow)
            assert np.array_equal(local, v.expired_queue(xprev, xnow)), (t, "expired queue in local rows")
            c.shard_expired_queue_begin(xprev, xnow, max(c.n, 1))
            inflight = c.shard_expired_queue_finish()
            assert np.array_equal(c.shard_rows_to_global(local), inflight) and np.array_equal(inflight, xwant[r]), (t, "expired queue", xprev, xnow)

    def one_batch_on(self, r, tag, qs, wide, v, feeds):
        c = self.ctx = self.drv.ctxs[r]
        wants = v.scan_many(qs)
        (c.scan_wide_begin if wide else c.scan_batch_begin)(qs)
        at_begin = c.table_info()
        self.finish_one(tag, wide, qs, wants)
        for qi, f in feeds:
            u, w = int(f * v.U), wants[qi]
            assert np.array_equal(c.batch_read_user_feed(qi, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "feed", qi, u)
        if not wide and self.turn_on_hot[r] is not None:
            k1, info = c.stats()["k1_variant"], c.table_info()
            if k1 & 0x800 and not k1 & 0x2000 and at_begin["hot_rows"] > 0 and info["hot_rows"] > 0 and info["hot_builds"] == self.turn_on_hot[r]:
                self.saw("turn_on_live_hot_index_then_batch")
            self.turn_on_hot[r] = None

    # ---- appends by global id: the keys come at once, or one to three steps later
    def do_append(self, tag, mode=None, delay=None, land=True):
        rng, sm = self.rng, self.sm
        mode_draw = str(rng.choice(["users", "one", "wave", "wave", "257", "burst", "one_rank", "rank600"]))
        delay_draw, new_draw = int(rng.choice([0, 0, 1, 2, 3])), int(rng.choice([0, 0, 1, 5]))
        late, touch = bool(rng.random() < 0.25), bool(rng.random() < 0.5)
        mode = mode or mode_draw
        delay = delay_draw if delay is None else delay
        N, U = sm.N, sm.U
        k = {"users": 0, "one": 1, "wave": 64, "257": 257, "one_rank": 50, "rank600": 600, "burst": min(N + 1, MAX_ROWS - N)}[mode]
        if k < 1 or N + k > MAX_ROWS:                # no room for rows: the call still raises U_g
            mode, k = "users", 0
        new_users = new_draw + 2 if mode == "users" else new_draw
        U2 = U + new_users
        top = int(sm.tm.start.max()) if N else self.t0 - DAY
        s2 = (top - rng.integers(0, 2 * HOUR, k) if late else top + np.sort(rng.integers(0, 4000, k))).astype(np.int64)
        e2 = np.where(rng.random(k) < 0.5, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k), s2 + 12 * HOUR).astype(np.int64)
        u2, d2 = rng.integers(0, U2, k).astype(np.int32), rng.integers(0, sm.tm.D, k).astype(np.int32)
        owner2 = shard_owner(self.oracle, sm.owner, U2, self.world)
        if mode in ("one_rank", "rank600"):          # one rank keeps all of it: everybody's N_g still advances
            pool = np.nonzero(owner2[:U2] == owner2[int(rng.integers(U2))])[0]
            u2 = rng.choice(pool, k).astype(np.int32)
        elif k:
            u2[: min(new_users, k)] = np.arange(U, U + min(new_users, k))
        keys = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
        if self.cfg["dup"] and self.dup_key is None and k > 1:
            other = np.nonzero(owner2[u2] != owner2[u2[0]])[0]
            if other.size:                           # one key on sessions of users of two ranks: the larger global row answers
                keys[other[-1]] = keys[0]
                self.dup_key = keys[:1].copy()
        had_users = [sm.users_of(r).size for r in range(self.world)]
        cap = list(sm.cap)
        if self.drv:
            got = self.drv.each(lambda c: c.shard_append_rows(s2, e2, u2, d2, U2))
        kept = sm.append_rows(s2, e2, u2, d2, U2)
        assert sum(kept) == k, (tag, "the model's shards do not keep the rows between them")
        if self.drv:
            assert [g[0] for g in got] == [N] * self.world, (tag, "first global row", got)
            assert [g[1] for g in got] == kept, (tag, "rows kept", got, kept)
        if any(not a and sm.users_of(r).size for r, a in enumerate(had_users)):
            self.saw("first_user_of_empty_rank")
        if any(b > a for a, b in zip(cap, sm.cap)):
            self.reshaped = True
            if self.shrunk and mode == "burst":
                self.saw("compact_shrink_then_burst_append")
            self.shrunk = False
        named = set(u2.tolist())
        self.rowless = [g for g in self.rowless + (list(range(U, U2)) if mode == "users" else []) if g not in named]
        if k and touch:                              # a touch of rows the call before queued, with no wait in between
            rows = np.arange(max(N, N + k - 64), N + k).astype(np.int32)
            vals = (self.clocks(rows.size) + rng.integers(-HOUR, 12 * HOUR, rows.size)).astype(np.int64)
            if self.drv:
                self.drv.each(lambda c: c.shard_set_end(rows, vals))
            sm.set_end(rows, vals)
        if k:
            if self.pending is None:
                self.pending, self.pending_due = keys, self.step + delay
            else:
                self.pending = np.concatenate([self.pending, keys])
        self.check_state((tag, mode, k, "keys at step", self.pending_due))
        if land:
            self.land_pending(tag)

    def land_pending(self, tag, part=None):
        sm = self.sm
        if self.pending is None or (part is None and self.step < self.pending_due):
            return
        keys = self.pending if part is None else self.pending[:part]
        slots = list(sm.slots)
        if self.drv:
            self.drv.each(lambda c: c.shard_token_append(keys))
        sm.token_append(keys)
        grown = [r for r in range(self.world) if sm.slots[r] > slots[r]]
        if grown:
            self.reshaped = True
            if len(grown) < self.world:
                self.saw("slots_doubled_on_one_rank_only")
        if self.compacted_with_tail:
            self.saw("token_append_after_compact_with_uncovered_tail")
            self.compacted_with_tail = False
        self.issued = np.concatenate([self.issued, keys])
        self.pending = self.pending[len(keys):] if len(keys) < len(self.pending) else None
        self.check_state((tag, "token_append", len(keys)))

    def do_token_append(self, tag):
        """some of the pending keys, or all: the rest stays an uncovered tail (covered_g < N_g) across the next steps"""
        if self.pending is None:
            self.do_append(tag, "wave", delay=2, land=False)
            if self.pending is None:
                return
        part = int(self.rng.integers(1, len(self.pending) + 1))
        if part < len(self.pending):
            self.pending_due = max(self.pending_due, self.step + 2)
        self.land_pending(tag, part)

    # ---- touches
    def do_set_end(self, tag):
        """pie_shard_set_end by global row: into and out of the top of the range, tombstones, revivals, repeats, rows a compaction
        dropped, rows behind the covered prefix; and once in a while a row outside [0, N_g): PIE_E_INVAL, nothing changed"""
        rng, sm = self.rng, self.sm
        N = sm.N
        k = int(rng.choice([1, 7, 200]))
        rows = rng.integers(0, N, k).astype(np.int32)
        gone = np.nonzero(sm.gone)[0]
        if gone.size and rng.random() < 0.7:
            rows[: min(k, 3)] = rng.choice(gone, min(k, 3))
        if sm.gone[rows].any():
            self.saw("touch_of_dropped_row")
        r = rng.random(k)
        ne = np.where(r < 0.2, END_NONE, np.where(r < 0.7, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k), self.t0 - rng.integers(0, 100 * DAY, k))).astype(np.int64)
        twice = rng.integers(0, k, max(k // 10, 1))           # the same rows again with other values: the last element wins
        rows, ne = np.concatenate([rows, rows[twice]]), np.concatenate([ne, self.t0 + np.arange(twice.size)]).astype(np.int64)
        bad = int(rng.choice([-1, N, N + 7, 2 ** 31 - 1]))
        if rng.random() < 0.3:
            at = int(rng.integers(rows.size))
            wrong = rows.copy()
            wrong[at] = bad
            self.expect(tag, PIE_E_INVAL, lambda c: c.shard_set_end(wrong, ne))
            self.check_state((tag, "after a row outside [0, N_g)", bad))
        if self.drv:
            self.drv.each(lambda c: c.shard_set_end(rows, ne))
        sm.set_end(rows, ne)
        self.check_state((tag, k))

    def keys_for(self, k):
        """k keys: issued ones (repeats happen, keys of dropped rows and the duplicate among them), a tenth absent, and a few of
        rows behind the covered prefix"""
        keys = self.some_keys(k)
        if self.pending is not None:
            keys[: min(k, 2)] = self.pending[: min(k, 2)]
        if self.dup_key is not None and k > 2:
            keys[2] = self.dup_key[0]
        return keys

    def do_token_set_end(self, tag):
        rng, sm = self.rng, self.sm
        k = int(rng.choice([1, 7, 64, 257]))
        keys = self.keys_for(k)
        new_end = np.where(rng.random(k) < 0.2, END_NONE, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k)).astype(np.int64)
        now = END_NONE if rng.random() < 0.15 else int(self.clocks(1)[0])
        if self.drv:
            got = self.drv.each(lambda c: c.shard_token_set_end(keys, new_end, now))
        want = sm.token_set_end(keys, new_end, now)
        if self.drv:
            for r in range(self.world):
                assert np.array_equal(got[r], want[r]), (tag, "rank", r, "rows written", np.nonzero(got[r] != want[r])[0][:8])
        self.check_state((tag, k, now))

    def shard_turn_ops(self, k):
        ops, _, _ = self.turn_ops(k, 0.0)
        if self.pending is not None:                 # keys of rows behind the covered prefix: no shard answers them yet
            ops["tok"][: min(k, 2)] = self.pending[: min(k, 2)]
        if self.dup_key is not None and k > 2:
            ops["tok"][2] = self.dup_key[0]
        return ops

    def check_turn(self, tag, r, got, want):
        same_turn(got, want, (tag, "rank", r))
        f = want["found"]
        assert np.array_equal(got["user"][f], want["user"][f]) and np.array_equal(got["start"][f], want["start"][f]), (tag, "rank", r, "user / start")

    def turn_on(self, tag, r, ops, want):
        """the synchronous turn on one rank, with what the hot index and the ordered run made of it"""
        c = self.drv.ctxs[r]
        before = c.table_info()
        self.check_turn(tag, r, c.shard_token_turn(ops), want)
        after = c.table_info()
        if before["ordered_rows"] > 0 and after["ordered_rows"] > 0:
            self.saw("plain_turn_kept_ordered_run")
        self.turn_on_hot[r] = before["hot_builds"] if before["hot_rows"] > 0 else None

    def do_token_turn(self, tag):
        k = int(self.rng.choice([1, 7, 64, 257, 300]))
        ops = self.shard_turn_ops(k)
        want = self.sm.turn(ops)
        if self.drv:
            for r in range(self.world):
                self.turn_on((tag, k), r, ops, want[r])
        self.check_state((tag, k))

    # ---- turns that log in: pie_shard_session_turn on every rank, users as GLOBAL ids
    def do_session_turn(self, tag, variant=None):
        """StoreChain.turn_ops' mix (creates with clocks anywhere, known and tombstoned keys re-used), some creates naming users no
        rank has yet, one under the key of a row a compaction dropped"""
        rng, sm = self.rng, self.sm
        k, p = int(rng.choice([1, 7, 64, 257, 300])), float(rng.choice([0.0, 0.1, 0.2, 0.4]))
        new_users = int(rng.choice([0, 0, 1, 3]))
        if variant == "users":                       # (designed chains) 64 ops, 40 % creates, three of them for users nobody has yet
            k, p, new_users = 64, 0.4, 3
        ops, user, disc = self.turn_ops(k, p)
        is_create = np.nonzero(ops["kind"] == 3)[0]
        new_users = min(new_users, is_create.size)
        user[is_create[:new_users]] = sm.U + np.arange(new_users)
        gone_keyed = np.nonzero(sm.gone[:sm.covered_g])[0]
        if is_create.size and gone_keyed.size:
            ops["tok"][is_create[-1]] = sm.tm.keys[int(rng.choice(gone_keyed))]
        self.apply_turn((tag, k, p), ops, user, disc, True, sm.U + new_users)

    def apply_turn(self, tag, ops, user, disc, session=True, U2=None):
        """one turn that may log in, given to every context with the same arrays; the answers, the plan's four outputs and the
        ordered run's bookkeeping per rank, then everything check_state checks after a mutator"""
        rng, sm, drv, world = self.rng, self.sm, self.drv, self.world
        U2 = sm.U if U2 is None else U2
        is_create = ops["kind"] == 3
        if is_create.any() and sm.covered_g < sm.N:
            # a keyed turn is only defined with covered_g == N_g: every rank refuses, none changes
            self.expect(tag, PIE_E_STATE, lambda c: c.shard_session_turn(ops, user, disc, U2))
            self.saw("shard_create_refused_short_column")
            self.check_state((tag, "refused"))
        if is_create.any() and (sm.covered_g < sm.N or sm.N + int(is_create.sum()) > MAX_ROWS):
            ops, user, disc, U2 = ops[~is_create], user[~is_create], disc[~is_create], sm.U
            is_create = is_create[~is_create]
        if ops.shape[0] == 0:
            return self.skip(tag)
        creates, N0 = int(is_create.sum()), sm.N
        top = int(sm.tm.start.max()) if N0 else INT64_MIN
        in_order = bool(np.all(ops["now"][is_create] >= top))
        held0 = [int(sm.held(r).size) for r in range(world)]
        users0 = [int(sm.users_of(r).size) for r in range(world)]
        cap0, slots0 = list(sm.cap), list(sm.slots)
        dropped_keys = {tuple(k) for k in sm.tm.keys[np.nonzero(sm.gone[:sm.covered_g])[0]].tolist()} if creates else set()
        if creates and any(tuple(k) in dropped_keys for k in ops["tok"][is_create].tolist()):
            self.saw("shard_create_over_dropped_rows_key")
        if creates and self.part_compacted:
            self.saw("shard_create_after_one_rank_compacted")
        # one rank with something of its own in flight: a batch refuses the turn there (PIE_E_STATE, nothing changed on it); a lookup
        # begun does not: it lands first
        busy = int(rng.integers(world))
        how = str(rng.choice(["none", "batch", "lookup"])) if creates else "none"
        qs = self.query_set(16, dense=False)
        lkeys = np.concatenate([self.issued[:200], self.absent[:4]])
        lnow = self.clocks(lkeys.shape[0])
        lwant = sm.shard_lookup(busy, lkeys, lnow) if how == "lookup" else None
        if how == "batch" and held0[busy] > 0:
            self.saw("shard_turn_refused_on_one_rank_with_batch")
            if drv:
                c = self.ctx = drv.ctxs[busy]
                wants = sm.view(busy)[0].scan_many(qs)
                c.scan_batch_begin(qs)
                self.expect_one(tag, PIE_E_STATE, busy, lambda x: x.shard_session_turn(ops, user, disc, U2))
                self.finish_one((tag, "rank", busy, "the batch in flight"), False, qs, wants)
                self.check_state((tag, "refused on one rank"))
        if how == "lookup":
            self.saw("shard_turn_create_with_lookup_begun")
            if drv:
                drv.ctxs[busy].shard_token_lookup_begin(lkeys, lnow)
        before = drv.each(lambda c: c.table_info()) if drv else None
        want, plan = sm.session_turn(ops, user, disc, U2)
        kept = [p[3] for p in plan]
        assert sum(kept) == creates, (tag, "the model's shards do not keep the creates between them")
        merged, whole = merge(want), None
        if creates:
            assert np.array_equal(merged["row"][is_create], N0 + np.arange(creates)), (tag, "the merged answer of a create is its global row")
        if drv:
            for r, c in enumerate(drv.ctxs):
                _, _, row_g, row_l, n_create, n_kept = self.pie.shard_session_turn_plan(ops, user, N0, held0[r], r, world)
                assert np.array_equal(row_g, plan[r][0]) and np.array_equal(row_l, plan[r][1]), (tag, "rank", r, "the plan's rows")
                assert (n_create, n_kept) == plan[r][2:], (tag, "rank", r, "the plan's counts", n_create, n_kept, plan[r][2:])
            got = drv.each(lambda c: c.shard_session_turn(ops, user, disc, U2))
            if how == "lookup":
                self.same_lookup(drv.ctxs[busy].shard_token_lookup_finish(), lwant, (tag, "rank", busy, "the lookup begun before the turn"))
            for r in range(world):
                self.check_turn(tag, r, got[r], want[r])
                other = is_create & ~want[r]["found"]
                assert np.all(got[r]["row"][other] == -1) and np.all(got[r]["user"][other] == -1), (tag, "rank", r, "a create another rank keeps")
            self.same_lookup_rows(tag, merge(got), merged)
            self.check_runs_after_logins(tag, before, drv.each(lambda c: c.table_info()), kept, in_order, cap0, users0)
        if creates:
            grew = [r for r in range(world) if sm.cap[r] > cap0[r]]
            doubled = [r for r in range(world) if sm.slots[r] > slots0[r]]
            if grew and len(grew) < world:
                self.saw("shard_create_outgrew_capacity_on_one_rank")
            if doubled and len(doubled) < world:
                self.saw("shard_create_doubled_slots_on_one_rank")
            if grew or doubled:
                self.reshaped = True
            if any(not users0[r] and kept[r] for r in range(world)):
                self.saw("shard_create_first_user_of_empty_rank")
            if world > 1 and any(k == 0 for k in kept):
                self.saw("shard_create_kept_by_no_live_rank_row")
            self.issued = np.concatenate([self.issued, ops["tok"][is_create]])
            self.shrunk = False
            named = set(user[is_create].tolist())
            self.rowless = [g for g in self.rowless if g not in named]
        self.check_state(tag)

    def same_lookup_rows(self, tag, got, want):
        for col in ("row", "live"):
            assert np.array_equal(got[col], want[col]), (tag, "merged by the largest global row", col, np.nonzero(got[col] != want[col])[0][:8])

    def check_runs_after_logins(self, tag, before, after, kept, in_order, cap0, users0):
        """StoreChain.check_run_after_logins per rank, in the rank's local numbers: a rank that keeps no create is untouched; one
        that keeps some drops its run with the switch off or when its columns grew, and keeps it — every kept row in it, no build —
        when the run was valid, the creates came in order and the rank gained no user; everywhere else a valid run is kept whole
        or dropped (a valid run holding no row reports 0, like no run, and is left undecided).  The scans and batches behind the
        turn are compared with the model on every rank by the readers; that a query which took the run before a keeping turn still
        takes it (k1_variant & 0x2000) is checked by StoreChain alone, on plain contexts."""
        sm, on = self.sm, bool(self.cfg["turn_ordered"])
        took, untouched = False, False
        for r in range(self.world):
            b, a = int(before[r]["ordered_rows"]), int(after[r]["ordered_rows"])
            t = (tag, "rank", r, "ordered run", b, a, kept[r])
            if kept[r] == 0:
                assert a == b and after[r]["ordered_builds"] == before[r]["ordered_builds"], (t, "a rank that keeps no create")
                untouched = untouched or b > 0
            elif not on or sm.cap[r] > cap0[r]:
                assert a == 0, (t, "switch off, or columns that moved")
            elif b > 0 and in_order and kept[r] <= 4096 and int(sm.users_of(r).size) == users0[r]:
                assert a == b + kept[r] and after[r]["ordered_builds"] == before[r]["ordered_builds"], (t, "in-order logins on a valid run")
                assert int(after[r]["ordered_respreads"]) - int(before[r]["ordered_respreads"]) in (0, 1), t
                took = True
            elif b > 0:
                # a create before the top, or a rank that gained a user (the run has room for the users its columns had room for
                # when it was built, which the chain does not mirror): kept whole or dropped, nothing in between
                assert a == 0 or (a == b + kept[r] and after[r]["ordered_builds"] == before[r]["ordered_builds"]), (t, "neither kept nor dropped")
        if took and untouched:
            self.saw("shard_turn_kept_ordered_run_on_keeping_rank_only")

    # ---- deletes and maintenance by global id
    def do_delete_user(self, tag):
        rng, sm = self.rng, self.sm
        U = sm.U
        kind = str(rng.choice(["owned", "owned", "busy", "-5", "U_g", "rowless"]))
        u = int(rng.integers(U))
        if kind == "rowless" or self.rowless:        # an id a k = 0 append just created
            if not self.rowless:
                self.do_append(tag, "users", land=False)
            u = int(self.rowless.pop())
            assert not np.any(sm.tm.user == u)
            self.saw("user_without_rows_then_deleted")
        elif kind == "busy":
            u = int(np.bincount(sm.tm.user, minlength=U).argmax())
        elif kind in ("-5", "U_g"):
            u = -5 if kind == "-5" else U
        got = self.drv.each(lambda c: c.shard_delete_user(u)) if self.drv else None
        want = sm.delete_user(u)
        self.lists((tag, u), got, want)
        self.check_state((tag, u))

    def do_delete_users(self, tag):
        rng, sm = self.rng, self.sm
        U = sm.U
        kind = str(rng.choice(["1", "16", "300", "rank", "tile"]))
        if kind == "tile":
            tile = int(rng.integers((U + TILE_USERS - 1) // TILE_USERS))
            ids = np.arange(tile * TILE_USERS, min((tile + 1) * TILE_USERS, U))
        elif kind == "rank":                         # all users of one rank
            ids = sm.users_of(int(rng.integers(self.world)))
            ids = ids if ids.size else rng.integers(0, U, 1)
        else:
            ids = rng.integers(0, U, int(kind))
        ids = np.concatenate([ids, ids[:1], [-1, U]])[rng.permutation(ids.size + 3)].astype(np.int32)   # a repeat, two ids outside
        if self.part_compacted:
            self.saw("compact_one_rank_then_delete_users")
        got = self.drv.each(lambda c: c.shard_delete_users(ids)) if self.drv else None
        want_rows, want_per = sm.delete_users(ids)
        if got:
            for r in range(self.world):
                assert np.array_equal(got[r][1], want_per[r]), (tag, kind, "rank", r, "rows per element")
        self.lists((tag, kind), [g[0] for g in got] if got else None, want_rows)
        self.check_state((tag, kind))

    def maint(self, tag, name, args, want):
        """one listing call on every rank; once per chain with room for one row less than the list: PIE_E_CAPACITY with the true
        count, the rows tombstoned all the same (the state check that follows reads them)"""
        over = not self.over_cap_done and any(w.size for w in want)
        if over:
            self.over_cap_done = True
            self.saw("maint_list_over_cap")
        self.lists(tag, None, want)
        if self.drv:
            for r, c in enumerate(self.drv.ctxs):
                if over and want[r].size:
                    rc, n = self.drv.maint(r, name, args, want[r].size - 1)
                    assert (rc, n) == (PIE_E_CAPACITY, want[r].size), (tag, "rank", r, "a cap below the list", rc, n, want[r].size)
                    continue
                if name == "prune":
                    got = c.shard_prune_before(args[0])
                elif name == "retention":
                    got = c.shard_retention_purge(*args)
                else:
                    got = c.shard_retention_purge(args[0], args[1], tz_table=args[2])
                assert got.dtype == np.int32 and np.array_equal(got, want[r]), (tag, "rank", r, "rows listed", got[:8], want[r][:8])
        self.check_state(tag)

    def do_prune(self, tag):
        sm = self.sm
        live = sm.tm.start[~sm.gone]
        cutoff = int(np.quantile(live, float(self.rng.uniform(0, 0.05)))) + int(self.rng.integers(2)) if live.size else 0
        self.maint((tag, cutoff), "prune", (cutoff,), sm.prune_before(cutoff))

    def retention_now(self, months, tz):
        sm = self.sm
        live = sm.tm.start[sm.tm.end != END_NONE]
        first = int(live.min()) if live.size else self.t0
        return int(add_months(np.array([first], np.int64), months, tz)[0]) + int(self.rng.integers(-DAY, 4 * DAY))

    def do_retention(self, tag):
        months, tz = int(self.rng.choice([1, 2, 3])), int(self.rng.choice([0, 330 * 60000, -5 * HOUR]))
        now = self.retention_now(months, tz)
        self.maint((tag, now, months, tz), "retention", (now, months, tz), self.sm.retention_purge(now, months, tz))

    def do_retention_tz(self, tag):
        months = int(self.rng.choice([1, 2, 3]))
        now = self.retention_now(months, HOUR)
        table = zone_table(self.oracle)
        self.maint((tag, now, months, ZONE), "retention_tz", (now, months, table), self.sm.retention_purge_tz(now, months, table))

    # ---- compaction of one rank, some ranks, all ranks: global ids never move, the other ranks do not change
    def do_compact(self, tag, which=None):
        rng, sm, world = self.rng, self.sm, self.world
        which_draw = str(rng.choice(["one", "some", "all"]))
        expired, shrink_draw, q = rng.random() < 0.6, bool(rng.integers(2)), float(rng.choice([0.05, 0.1, 0.3]))
        order = rng.permutation(world)
        some = int(rng.integers(1, max(world, 2)))
        which = which or which_draw
        shrink = shrink_draw
        if which.startswith("shrink_") or which.startswith("inplace_"):
            shrink, which = which.startswith("shrink_"), which.split("_", 1)[1]
        ranks = sorted(int(r) for r in (order[:1] if which == "one" else order[:some] if which == "some" else order))
        live = sm.tm.end[sm.tm.end != END_NONE]
        dead_before = int(np.quantile(live, q)) if expired and live.size else END_NONE
        tag = (tag, which, ranks, dead_before, "shrink" if shrink else "in place")
        dropped = 0
        for r in ranks:
            kept, gone = sm.compact(r, dead_before, shrink)
            dropped += gone
            if self.drv:
                assert self.drv.ctxs[r].compact_rows(dead_before, shrink) == kept, (tag, "rank", r, "rows kept")
        if dropped:
            self.reshaped = True
            self.shrunk = shrink
            self.part_compacted = len(ranks) < world
            if self.pending is not None:
                self.compacted_with_tail = True
        self.check_state(tag)

    # ---- in-flight forms: begun beside one to three batches on one rank or on all, everything finished in begin order
    def begin_batches(self, tag):
        """-> per rank [(wide, queries, answers of the shard as it stands)]"""
        rng, sm = self.rng, self.sm
        plans = []
        for _ in range(int(rng.integers(1, 4))):
            wide = bool(rng.random() < 0.3)
            plans.append((wide, self.query_set(70 if wide else 16, dense=False)))
        only = int(rng.integers(self.world)) if rng.random() < 0.4 else None
        begun = [[] for _ in range(self.world)]
        if self.drv:
            for r, c in enumerate(self.drv.ctxs):
                if (only is not None and r != only) or c.n == 0:     # (a rank without rows has nothing to scan)
                    continue
                v = sm.view(r)[0]
                for wide, qs in plans:
                    if c.batch_room() <= 0:
                        break
                    (c.scan_wide_begin if wide else c.scan_batch_begin)(qs)
                    begun[r].append((wide, qs, v.scan_many(qs)))
        return begun

    def finish_batches(self, tag, r, begun, after=False):
        self.ctx = self.drv.ctxs[r]
        v = self.sm.view(r)[0] if after and begun else None
        for b, (wide, qs, wants) in enumerate(begun):
            self.finish_one((tag, "rank", r, "batch in flight", b), wide, qs, wants, v.scan_many(qs) if v else None)

    def do_inflight_lookup(self, tag, variant=None):
        """up to four lookups begun beside the batches, one clock per key, finished in begin order; or (variant "grow") begun with
        nothing else in flight and followed by an append that outgrows every shard's capacity: the columns and both maps are
        re-allocated under the lookups, which answer for the table they were begun on"""
        rng, sm = self.rng, self.sm
        keys = np.concatenate([self.issued, self.absent])
        n_lookups = int(rng.integers(1, 5))
        clocks = [self.clocks(keys.shape[0]) for _ in range(n_lookups)]
        grow_draw = bool(rng.random() < 0.3)
        grow = (variant == "grow" or (variant is None and grow_draw)) and 2 * sm.N + 1 <= MAX_ROWS
        begun = [[] for _ in range(self.world)] if grow else self.begin_batches(tag)
        if self.reshaped:
            self.saw("inflight_lookup_after_reshape")
        want = [[sm.shard_lookup(r, keys, now) for now in clocks] for r in range(self.world)]
        if self.drv:
            for c in self.drv.ctxs:
                for now in clocks:
                    c.shard_token_lookup_begin(keys, now)
        if grow:
            cap = list(sm.cap)
            self.do_append(tag, "burst", land=False)
            if any(b > a for a, b in zip(cap, sm.cap)):
                self.saw("capacity_outgrown_under_lookup_begun")
        if self.drv:
            for r, c in enumerate(self.drv.ctxs):
                self.finish_batches(tag, r, begun[r])
                for i in range(n_lookups):
                    self.same_lookup(c.shard_token_lookup_finish(), want[r][i], (tag, "rank", r, "lookup begun in flight", i))
        self.check_state(tag)

    def do_inflight_turn(self, tag):
        """pie_shard_token_turn_begin beside the batches: refused exactly where the rank's ordered run is valid (the turn then goes
        through the synchronous call); where it is taken every pie_shard_* mutator behind it is refused, a batch begun before it
        answers for the table before it, one begun after it sees it"""
        rng, sm, drv = self.rng, self.sm, self.drv
        k = int(rng.choice([1, 7, 64, 257, 300]))
        ops = self.shard_turn_ops(k)
        q_after = self.query_set(16, dense=False)
        begun = self.begin_batches(tag)
        if self.cfg["ordered"] == 2:
            self.saw("host:turn_begin_in_ordered_chain")
        elif not drv:                         # never a run: the begin is taken, and a mutator behind it refused
            self.saw("refused_mutator_while_turn_begun")
            if self.reshaped:
                self.saw("inflight_turn_after_reshape")
        taken = []
        if drv:
            for r, c in enumerate(drv.ctxs):
                before = c.table_info()
                if before["ordered_rows"] > 0:
                    self.expect_one(tag, PIE_E_STATE, r, lambda x: x.shard_token_turn_begin(ops))
                    self.saw("refused_turn_begin_on_ordered_run")
                    self.finish_batches(tag, r, begun[r])
                    continue
                # A valid run that holds no row (a rank without a live row, in a mode that builds runs) reports ordered_rows = 0
                # like no run at all: there, and only there, the begin may be refused or taken.
                undecided = self.cfg["ordered"] != 0 and not np.any(sm.view(r)[0].end != END_NONE)
                try:
                    c.shard_token_turn_begin(ops)
                except self.pie.PieError as exc:
                    assert undecided and exc.code == PIE_E_STATE, (tag, "rank", r, "begin refused with no ordered run reported", exc.code)
                    self.finish_batches(tag, r, begun[r])
                    continue
                taken.append((r, before))
                for call in self.mutators():
                    self.expect_one((tag, "behind a turn begun"), PIE_E_STATE, r, call)
                self.saw("refused_mutator_while_turn_begun")
        want = sm.turn(ops)
        if drv:
            for r, c in enumerate(drv.ctxs):
                if r not in [x[0] for x in taken]:
                    self.turn_on((tag, "synchronous"), r, ops, want[r])
            for r, before in taken:
                c = drv.ctxs[r]
                after = None
                if c.n and c.batch_room() > 0:     # a batch begun after the turn sees it
                    c.scan_batch_begin(q_after)
                    after = (False, q_after, sm.view(r)[0].scan_many(q_after))
                self.finish_batches(tag, r, begun[r], after=True)
                if after:
                    self.finish_batches((tag, "begun after the turn"), r, [after])
                self.check_turn((tag, "the turn begun in flight"), r, c.shard_token_turn_finish(), want[r])
                if self.reshaped:
                    self.saw("inflight_turn_after_reshape")
                self.turn_on_hot[r] = before["hot_builds"] if before["hot_rows"] > 0 else None
        self.check_state(tag)

    def do_inflight_purge(self, tag):
        """the purge tick: pie_shard_expired_queue_begin beside the batches, then the union of the ranks' global rows tombstoned
        by one pie_shard_set_end given to every rank"""
        rng, sm, drv = self.rng, self.sm, self.drv
        live = sm.tm.end[sm.tm.end != END_NONE]
        now = int(np.quantile(live, float(rng.uniform(0.0, 0.15)))) if live.size else self.t0
        begun = self.begin_batches(tag)
        if self.reshaped:
            self.saw("inflight_purge_after_reshape")
        want = sm.expired_queue(END_NONE, now)
        if drv:
            drv.each(lambda c: c.shard_expired_queue_begin(END_NONE, now, max(c.n, 1)))
            got = []
            for r, c in enumerate(drv.ctxs):
                self.finish_batches(tag, r, begun[r])
                got.append(c.shard_expired_queue_finish())
            self.lists((tag, "the queue begun in flight", now), got, want, sm.tm.expired_queue(END_NONE, now))
            rows = np.sort(np.concatenate(got)).astype(np.int32)
            if rows.size:
                drv.each(lambda c: c.shard_set_end(rows, np.full(rows.size, END_NONE)))
        sm.purge(now)
        self.check_state((tag, now))

    # ---- refusals: each expected exactly, each followed by the full state check on every rank
    def do_refusals(self, tag):
        rng, sm, drv = self.rng, self.sm, self.drv
        qs = self.query_set(16, dense=False)
        r = int(rng.integers(self.world))
        past = rng.integers(0, 2 ** 64, (sm.N - sm.covered_g + 1, 2), dtype=np.uint64)
        self.saw("refused_mutator_while_batch_in_flight")
        if not drv:
            return
        one64, one32 = np.full(1, self.t0, np.int64), np.zeros(1, np.int32)
        c = drv.ctxs[r]
        if c.n:                                       # every mutator while a batch is in flight on that rank
            wants = sm.view(r)[0].scan_many(qs)
            c.scan_batch_begin(qs)
            for call in self.mutators():
                self.expect_one((tag, "beside a batch"), PIE_E_STATE, r, call)
            self.ctx = c
            self.finish_one((tag, "rank", r, "the batch in flight"), False, qs, wants)
        else:
            r2 = max(range(self.world), key=lambda x: drv.ctxs[x].n)
            c2 = drv.ctxs[r2]
            if c2.n:
                wants = sm.view(r2)[0].scan_many(qs)
                c2.scan_batch_begin(qs)
                for call in self.mutators():
                    self.expect_one((tag, "beside a batch"), PIE_E_STATE, r2, call)
                self.ctx = c2
                self.finish_one((tag, "rank", r2, "the batch in flight"), False, qs, wants)
        self.check_state((tag, "after the mutators beside a batch"))
        self.expect((tag, "plain token_append"), PIE_E_STATE, lambda x: x.token_append(past[:1]))
        self.expect((tag, "keys past N_g"), PIE_E_INVAL, lambda x: x.shard_token_append(past))
        self.expect((tag, "fewer users"), PIE_E_INVAL, lambda x: x.shard_append_rows(one64, one64 + HOUR, one32, one32, sm.U - 1))
        self.check_state((tag, "after the refusals"))


# Fixed op lists through the same machinery, for the states the hot index and the ordered run decide and for the ones a seed
# reaches only by luck: a table large enough for the index with turns around batches; the ordered run held across synchronous
# turns and refusing the in-flight begin; a shrink that drops rows followed by the burst that outgrows it, a lookup begun under a
# growth, one rank compacted before a batched delete, keys landing behind a compaction.
DESIGNED = {
    "hot": ({"world": 1, "n": 20000, "U": 499, "D": 32, "hot": 1, "ordered": 0, "lanes": 3, "async": 1, "dup": False},
            ["token_turn", "token_turn", "inflight_turn", "set_end", "token_turn", "compact:inplace_all", "token_turn", "inflight_turn",
             "inflight_lookup", "inflight_purge", "token_append", "token_set_end", "token_turn"]),
    "ordered": ({"world": 2, "n": 4099, "U": 64, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 0, "dup": True},
                ["token_turn", "inflight_turn", "append:wave", "prune", "token_turn", "compact:shrink_one", "delete_users", "token_turn",
                 "inflight_turn", "refusals"]),
    "reshape": ({"world": 3, "n": 4099, "U": 64, "D": 8, "hot": 0, "ordered": 0, "lanes": 2, "async": 1, "dup": True},
                ["set_end", "prune", "append:wave", "token_append", "compact:shrink_all", "append:burst", "set_end", "token_append", "inflight_lookup:grow", "compact:inplace_one", "delete_users", "delete_user", "inflight_turn", "inflight_lookup",
                 "inflight_purge", "token_set_end", "retention_tz", "refusals"]),
    "empty_rank": ({"world": 5, "n": 65, "U": 7, "D": 8, "hot": 0, "ordered": 1, "lanes": 1, "async": 0, "dup": True},
                   ["append:users", "delete_user", "append:users", "append:wave", "append:rank600", "token_append", "compact:shrink_some", "append:one_rank", "token_turn", "token_set_end", "inflight_turn", "refusals"]),
}


# Chains that log in through the turn (a dict of their own: DESIGNED's names give its chains their seeds)
DESIGNED_LOGINS = {
    # world 5 over 7 users starts with a rank that owns nobody: new users until it gains one, by a create
    "empty_rank": ({"world": 5, "n": 65, "U": 7, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 0, "dup": False, "turn_ordered": 1, "logins": 1},
                   ["session_turn:users", "session_turn:users", "logins", "session_turn:users", "session_turn:users", "logins_chain"]),
    # about 500 rows and 1 024 slots a rank: a few logins carry one rank past half its slots before the other; one-user chains are
    # kept by one rank, whose run takes them while the other's stays as it was
    "slots": ({"world": 2, "n": 1000, "U": 64, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 1, "dup": False, "turn_ordered": 1, "logins": 1},
              ["logins", "logins_chain", "logins", "logins_chain", "logins_undo", "compact:one", "logins_chain", "logins", "logins_chain",
               "inflight_turn", "logins"]),
}


def run_designed_logins(pie, oracle, name):
    cfg, script = DESIGNED_LOGINS[name]
    return ShardChain(pie, oracle, 9300 + sorted(DESIGNED_LOGINS).index(name), cfg, script).run()


def run_shard_chain(pie, oracle, seed, cfg=None, script=None, log=None):
    return ShardChain(pie, oracle, seed, cfg, script, log).run()


def run_designed(pie, oracle, name):
    cfg, script = DESIGNED[name]
    return run_shard_chain(pie, oracle, 9100 + sorted(DESIGNED).index(name), cfg, script)
