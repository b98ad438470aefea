"""TEST INFRASTRUCTURE — the seeded chain over the SESSION-STORE half of the C ABI: the token column and its index, one-launch
turns (pie_token_turn, pie_session_turn), turns / lookups / the purge tick begun while batches are in flight, pie_delete_users,
and compaction that carries the keys over — each of them in the state the others leave behind.  tests/table_model.Chain covers
the scan half (set_end, append, delete_user, prune, retention, shard, flood against scan / batch / wide / pipeline / queues); this
one keeps a token column on the table the whole time and mixes what touches it.

StoreModel is ONE set of columns with the token column over them: tests/session_turn_model.SessionTurnModel for the token rules,
tests/compact_model.CompactModel (tests/table_model.TableModel) for the table rules, on the same arrays.  It also mirrors the two
host-side sizes the header documents — the slot count (pie_token_slots_for; it doubles when covered > slots / 2, a compaction
that moves rows rebuilds into the size of the kept covered rows) and the column capacity (a load fits exactly, an append or a
creating turn that outgrows it doubles it, PIE_COMPACT_SHRINK re-sizes to the kept rows) — so that the states below can be
decided without a device.

StoreChain(pie or None, oracle, seed) drives a context and the model side by side, or — pie = None — the model alone with the
very same random draws (no draw depends on the device).  The model is the only source of expected values; the first difference
raises, tagged with seed, step and op.  Nothing here needs a GPU to import.

cfg["logins"] (off unless asked for) makes a chain of another kind: OPS_LOGINS adds turns whose creates are stamped at or after the
table's top, pie_set_turn_ordered is part of the configuration (logins_config, a random stream of its own), and after every
creating turn check_run_after_logins decides on the host whether the ordered run had to survive.  A chain without the option
draws exactly what it drew before the option existed (tests/golden/store_chain_oplog.txt)."""
import numpy as np

from compact_model import CompactModel, compact_maps, translate
from delete_users_cases import expected as delete_users_expected
from session_turn_model import CREATE, SessionTurnModel
from table_model import ALL, DAY, HOUR, INT64_MIN, PIE_E_STATE, Chain, add_months, check_union, ctx_with_env, same
from token_model import END_NONE, check_layout, key_of
from turn_model import DELETE, GET, TOUCH, TURN_OP, same_turn

MAX_ROWS = 40000      # no chain grows its table past this
TILE_USERS = 256      # pie_delete_users: "all users of a tile"

# what a chain can arrive at; test_store_chains_reached_every_state wants each of them seen on the device
STATES = (
    "create_after_compact_shrink",            # a creating turn on a column whose last change was a compaction that dropped rows
    "create_after_compact_noshrink",          # ... without PIE_COMPACT_SHRINK: old keys lie behind the covered prefix
    "create_doubled_slots",                   # token_builds rose inside a creating turn
    "create_outgrew_capacity",                # table_bytes rose inside a creating turn
    "compact_across_prefix_then_create",      # token_rows < rows, rows dropped on both sides of the prefix end, append, create
    "create_over_foreign_tombstone",          # a create under a key whose older row delete_user(s) / prune / retention tombstoned
    "turn_on_live_hot_index_then_batch",      # hot_rows > 0 at the turn, the next batch answered by the index, hot_builds unchanged
    "hot_index_rebuilt_between_turns",
    "plain_turn_kept_ordered_run",
    "creating_turn_dropped_ordered_run",
    "inflight_turn_after_reshape",            # each in-flight form on a table compacted or grown earlier in the chain
    "inflight_lookup_after_reshape",
    "inflight_purge_after_reshape",
    "refused_begin_on_ordered_run",
    "refused_mutator_while_turn_begun",
    "refused_session_turn_with_batch",
    "refused_create_on_short_column",
)
# ... and what the chains that log in (cfg["logins"]) add: a creating turn under pie_set_turn_ordered, in the state the others leave
LOGIN_STATES = (
    "creating_turn_kept_ordered_run",         # the run valid before, every row of the turn in it afterwards, nothing rebuilt
    "kept_run_then_batch_on_run",             # the batch that took the run before a keeping turn takes it afterwards
    "kept_run_respread",                      # ordered_respreads rose inside a turn
    "kept_run_after_compact_shrink",          # the first turn that keeps the run since a compaction dropped rows (with
    "kept_run_after_compact_noshrink",        # PIE_COMPACT_SHRINK the turn right behind it has to grow the columns, and drops it)
    "kept_run_with_live_hot_index",
    "kept_run_create_then_delete_in_turn",    # a later op of the turn ended a row it created: the insert reads the table's `end`
    "kept_run_then_refused_inflight_begin",   # pie_token_turn_begin refused on the run a creating turn kept
    "back_fill_dropped_run",                  # a create before the table's top, the run gone
    "growth_dropped_run_switch_on",
)
# (A row the run does not hold was a tombstone, end = INT64_MIN, when the run was built.  turn_apply in sph-pie_amd/csrc/pie_token.h
# is the only place a get / touch / delete of k_token_turn and k_session_turn moves `end`: a TOUCH writes only when `e > op.now`,
# which INT64_MIN never is for an int64 clock; a DELETE writes INT64_MIN; a CREATE writes a row of its own at or behind the turn's
# first new row.  So no op of a turn brings such a row back to life, and "a creating turn revived a row and dropped the run" is
# not a state a chain can arrive at.  pie_set_end can revive one, outside a turn: do_set_end does, between the logins, and
# the first login the host expects to keep the run after it is recorded as host:login_since_set_end_revived_row.)
LOGIN_HOST_STATES = ("host:login_in_order_switch_on", "host:login_in_order_switch_off", "host:login_grew_switch_on", "host:login_before_top",
                     "host:login_create_then_delete", "host:login_since_compact_shrink", "host:login_since_compact_noshrink",
                     "host:login_full_segment", "host:login_chain_of_one_user", "host:login_landed_uncovered_tail",
                     "host:begin_after_login", "host:login_since_set_end_revived_row")
# decided by the device alone (the hot index and the ordered run); the model-only run records a stand-in for two of them
DEVICE_STATES = ("turn_on_live_hot_index_then_batch", "hot_index_rebuilt_between_turns", "plain_turn_kept_ordered_run",
                 "creating_turn_dropped_ordered_run", "refused_begin_on_ordered_run")
HOST_STATES = tuple(s for s in STATES if s not in DEVICE_STATES) + ("host:creating_turn_in_ordered_chain", "host:begin_in_ordered_chain")


def slots_for(covered):
    """pie_token_slots_for restated: the smallest power of two >= max(1024, 2 * covered)"""
    s = 1024
    while s // 2 < covered:
        s <<= 1
    return s


# ------------------------------------------------------------------------------------------------ the model
class StoreModel(SessionTurnModel, CompactModel):
    """start / end / user / disc once; the token rules (token_set, token_append, lookup, token_set_end, turn, delete_user, purge,
    compact) are SessionTurnModel's, the table rules (set_end, prune_before, retention_purge, scan_many, expired_queue) are
    TableModel's, and both read and write the same arrays."""

    def __init__(self, oracle, start, end, user, disc, U, D):
        CompactModel.__init__(self, oracle)
        SessionTurnModel.__init__(self, start, end, user, disc)
        self.U, self.D = int(U), int(D)
        self.cap = max(self.n, 1)           # rows of capacity: pie_table_info.table_bytes / 24
        self.slots, self.builds = 0, 0      # slots of the index; rebuilds since the column was set (pie_table_info.token_builds)
        self._in_turn = False

    # ---- the two host-side sizes
    def _room(self, rows, covered):
        if rows > self.cap:
            self.cap = max(rows, 2 * self.cap)
        if covered > self.slots // 2:
            self.slots = slots_for(covered)
            self.builds += 1

    def token_set(self, keys):
        super().token_set(keys)
        self.slots, self.builds = slots_for(self.covered), 0

    def token_append(self, keys):
        if not self._in_turn:
            self._room(self.n, self.covered + len(keys))
        super().token_append(keys)

    def append_rows(self, start, end, user, disc):
        if not self._in_turn:
            self._room(self.n + len(start), 0)
        super().append_rows(start, end, user, disc)

    def turn(self, ops, user=None, disc=None):
        creates = int(np.count_nonzero(ops["kind"] == CREATE))
        if creates:                          # room for all of them first, by one growth each (pie_session_turn)
            self._room(self.n + creates, self.n + creates)
        self._in_turn = True
        try:
            return super().turn(ops, user, disc)
        finally:
            self._in_turn = False

    def delete_users(self, ids):
        """K single deletes in array order -> (all rows tombstoned ascending, rows per element)"""
        _, union, per = delete_users_expected(self, ids)
        return union, per

    def compact(self, dead_before=END_NONE, shrink=False):
        """-> new_of_old.  A compaction that keeps every row leaves everything alone, unless PIE_COMPACT_SHRINK has capacity to
        give back: then the rows move like any others."""
        kept = int(np.count_nonzero(self.end > dead_before))
        same_table = kept == self.n and not (shrink and self.cap > max(kept, 1))
        new_of_old = super().compact(dead_before)
        if not same_table:
            self.slots = slots_for(self.covered)
            self.builds += 1
            if shrink:
                self.cap = max(kept, 1)
        return new_of_old


class StoreModelStore:
    """what tests/session_turn_model.replay_g5_sessions drives, built on StoreModel"""

    def __init__(self, oracle, n_users):
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.m = StoreModel(oracle, z64, z64, z32, z32, n_users, 1)
        self.m.token_set(np.zeros((0, 2), np.uint64))
        self.U = n_users

    def turn(self, ops, user, disc):
        return self.m.turn(ops, user, disc)

    def delete_user(self, u):
        self.m.delete_user(u)

    def purge(self, now):
        self.m.purge(now)


# ------------------------------------------------------------------------------------------------ the chain
def store_config(seed):
    rng = np.random.default_rng([seed, 0x5703E])
    return {
        "n": int(rng.choice([0, 1, 700, 3000, 20000])), "U": int(rng.choice([1, 64, 499])), "D": int(rng.choice([1, 8, 32])),
        "hot": int(rng.integers(2)), "ordered": int(rng.choice([0, 2])), "lanes": int(rng.integers(1, 5)),
        "async": int(rng.integers(2)), "wide_ordered": int(rng.integers(2)), "steps": int(rng.integers(30, 51)),
        "gen_seed": int(rng.integers(1, 2 ** 60)),
    }


def logins_config(seed):
    """the draws of a chain that logs in, from a stream of their own (store_config's draws stay what they were): the sizes of the
    existing `ordered` designed chain and below, a mode that builds runs, the switch mostly on"""
    rng = np.random.default_rng([seed, 0x10615])
    return {
        "n": int(rng.choice([1, 700, 3000, 4099])), "U": int(rng.choice([7, 64])), "D": int(rng.choice([1, 8])), "hot": 0,
        "ordered": int(rng.choice([1, 2, 2, 2])), "turn_ordered": int(rng.choice([0, 1, 1, 1])),
    }


class StoreChain(Chain):
    """One seeded chain: a table with a token column, a context configuration, 30 to 50 steps (or the fixed list `script`).
    Every step is one mutator or in-flight form, the state checks, and the readers.  run() raises at the first difference."""

    OPS = ("session_turn", "session_turn", "session_turn", "session_turn", "token_turn", "token_set_end", "set_end", "set_end",
           "append", "append", "delete_user", "delete_users", "prune", "retention", "compact", "compact", "compact",
           "inflight_turn", "inflight_lookup", "inflight_purge", "turn_vs_batch")
    # cfg["logins"]: the same mix with the in-order logins among it (a tuple of its own: OPS draws what it always drew)
    OPS_LOGINS = OPS + ("logins", "logins", "logins", "logins", "logins_chain", "logins_full", "logins_undo", "logins_late")

    def __init__(self, pie, oracle, seed, cfg=None, script=None, log=None):
        self.pie, self.oracle, self.seed = pie, oracle, seed
        self.cfg = dict(store_config(seed), logins=0, turn_ordered=0)
        if (cfg or {}).get("logins"):
            self.cfg.update(logins_config(seed))
        self.cfg.update(cfg or {})
        self.ops = self.OPS_LOGINS if self.cfg["logins"] else self.OPS
        self.script = script
        self.rng = np.random.default_rng([seed, 0x570E])
        self.log = log
        self.t0 = oracle.T0_MS
        self.ctx = None
        self.states = {}
        self.step = -1
        self.issued = np.zeros((0, 2), np.uint64)       # every key ever given to a row, rows dropped since included
        self.pending, self.pending_due = None, 0        # keys of the rows behind the covered prefix, and the step that lands them
        self.foreign = np.zeros(0, bool)                # rows tombstoned by delete_user(s) / prune / retention
        self.column_last = "set"                        # the last change of the token column
        self.reshaped = False                           # compacted or grown earlier in the chain
        self.straddle = None                            # None -> "pending" (the compaction) -> "appended" -> the creating turn
        self.scanned_since_drop = False                 # ordered mode 2: a scan since the run was last dropped
        self.turn_on_hot = None                         # hot_builds at a turn that found the index live
        self.builds_seen, self.dropped = 0, False       # Chain.watch_index's
        self.touched = True
        self.builds_at_turn, self.dropped_since_turn, self.rebuilt_since_turn = None, False, False
        self.builds0 = 0
        self.compactions = 0
        # chains that log in
        self.skipped = 0                                # steps that gave the library no call of their op: no room for the logins, a
                                                        # turn left without an op, a purge tick on a table without rows
        self.last_scan, self.last_batch = None, None    # the readers' last scan and batch, for the same queries around a turn
        self.since_compact = None                       # "shrink" / "noshrink": rows dropped, and no turn has kept the run since
        self.kept_builds = None                         # ordered_builds at the last turn that kept the run
        self.login_since_begin = False
        self.host_kept_seen, self.revived_since_kept = False, False   # pie_set_end revived a tombstone since the last keeping login

    # ---- set-up
    def make_table(self):
        c, o = self.cfg, self.oracle
        n, U, D = c["n"], c["U"], c["D"]
        s, e, u, d = [a.copy() for a in o.gen(c["gen_seed"], max(n, 1), 0, max(n, 1), U, D, 0)]
        self.m = StoreModel(o, s[:n], e[:n], u[:n], d[:n], U, D)
        self.mask = ALL
        self.absent = self.rng.integers(0, 2 ** 64, (64, 2), dtype=np.uint64)

    def run(self):
        self.make_table()
        c, m = self.cfg, self.m
        if self.pie is not None:
            ctx = self.ctx = ctx_with_env(self.pie, c["hot"], c["async"])
        try:
            keys = self.rng.integers(0, 2 ** 64, (m.n, 2), dtype=np.uint64)
            if self.ctx:
                ctx.set_ordered_run(c["ordered"])
                ctx.set_turn_ordered(c["turn_ordered"])
                ctx.set_batch_lanes(c["lanes"])
                ctx.set_wide_ordered(c["wide_ordered"])
                ctx.load_columns(*m.columns(), m.U)
                ctx.set_disciplines(self.mask, m.D)
                ctx.token_set(keys)
                self.builds0 = ctx.table_info()["token_builds"]
            m.token_set(keys)
            self.issued = keys
            self.foreign = np.zeros(m.n, bool)
            steps = len(self.script) if self.script else c["steps"]
            for step in range(-1, steps):
                self.step = step
                op = "load" if step < 0 else self.script[step] if self.script else str(self.rng.choice(self.ops))
                tag = "seed %d step %d %s" % (self.seed, step, op)
                if self.log:
                    self.log("%s n %d covered %d slots %d cap %d" % (tag, m.n, m.covered, m.slots, m.cap))
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
        finally:
            if self.ctx:
                self.ctx.close()
        return self

    # ---- bookkeeping
    def saw(self, state):
        assert state in STATES or state in HOST_STATES or state in LOGIN_STATES or state in LOGIN_HOST_STATES, state
        self.states[state] = self.states.get(state, 0) + 1

    def info(self):
        """table_info with Chain.watch_index's record of the hot index, plus: dropped / rebuilt since the last turn"""
        info = self.watch_index()
        if self.builds_at_turn is not None:
            if info["hot_builds"] and info["hot_rows"] == 0:
                self.dropped_since_turn = True
            if self.dropped_since_turn and info["hot_builds"] > self.builds_at_turn and info["hot_rows"] > 0:
                self.rebuilt_since_turn = True
        return info

    def snapshot(self):
        cov, slots, slot_row, back = self.ctx.token_layout()
        info = self.ctx.table_info()
        return [a.copy() for a in self.ctx.read_columns()] + [slot_row.copy(), back.copy(),
                                                              np.array([cov, slots, info["token_rows"], info["rows"], info["table_bytes"]])]

    def refused(self, tag, call, unchanged=True):
        """the header refuses `call` with PIE_E_STATE; unchanged: columns, layout and table_info are compared around it (only
        with nothing in flight: the readers of a snapshot are refused beside batches)"""
        if not self.ctx:
            return
        before = self.snapshot() if unchanged else None
        n = self.ctx.n
        try:
            call()
        except self.pie.PieError as exc:
            assert exc.code == PIE_E_STATE, (tag, "refused with", exc.code)
        else:
            raise AssertionError((tag, "a call the header refuses went through"))
        assert self.ctx.n == n
        if unchanged:
            for x, y in zip(before, self.snapshot()):
                assert np.array_equal(x, y), (tag, "a refused call changed something")

    def check_state(self, tag):
        """after every mutator: the columns bit for bit, the covered count, the two mirrored sizes, and the index's layout"""
        ctx, m = self.ctx, self.m
        if self.foreign.size < m.n:
            self.foreign = np.concatenate([self.foreign, np.zeros(m.n - self.foreign.size, bool)])
        assert m.covered + (0 if self.pending is None else len(self.pending)) == m.n, (tag, "the chain lost count of its keys")
        if not ctx:
            return
        assert ctx.n == m.n and ctx.n_users == m.U, (tag, "shape")
        for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), m.columns()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name, np.nonzero(got != want)[0][:8])
        info = self.info()
        assert info["rows"] == m.n and info["users"] == m.U and info["token_rows"] == m.covered, (tag, "table_info", info["rows"], info["token_rows"], m.n, m.covered)
        assert info["table_bytes"] // 24 == m.cap, (tag, "capacity", info["table_bytes"] // 24, m.cap)
        assert info["token_builds"] - self.builds0 == m.builds, (tag, "token_builds", info["token_builds"] - self.builds0, m.builds)
        cov, slots, slot_row, back = ctx.token_layout()
        assert cov == m.covered and slots == m.slots, (tag, "layout", cov, slots, m.covered, m.slots)
        assert np.array_equal(back, m.keys), (tag, "the token column", np.nonzero((back != m.keys).any(axis=1))[0][:8])
        if cov:
            check_layout(cov, slots, slot_row, back, self.pie.token_homes(back, int(slots).bit_length() - 1))
        else:
            assert np.all(slot_row < 0), (tag, "a slot held by no row")

    # ---- clocks and keys
    def clocks(self, k):
        """k clocks: most in the top tenth of the `end` range (where the hot index and the sparse queries live), some anywhere"""
        rng, e = self.rng, self.ends_in_range()
        lo, hi, bottom = int(np.quantile(e, 0.9)), int(e.max()), int(e.min())
        top = rng.integers(lo, hi + 1, k)
        anywhere = rng.integers(bottom, hi + 1, k)
        return np.where(rng.random(k) < 0.7, top, anywhere).astype(np.int64)

    def tombstoned_keys(self):
        m = self.m
        rows = np.nonzero(self.foreign[:m.covered] & (m.end[:m.covered] == END_NONE))[0]
        return m.keys[rows]

    def turn_ops(self, k, p_create):
        """tests/test_gpu_session_turn.twin_ops' mix: a tenth of the ops repeat a key of an earlier op of the same turn, creates
        mostly bring fresh keys and some re-use a known one (half of those a key whose row a maintenance call tombstoned), a
        few other ops name unknown keys"""
        rng, m = self.rng, self.m
        p = float(p_create)
        ops = np.zeros(k, TURN_OP)
        ops["kind"] = rng.choice([GET, TOUCH, DELETE, CREATE], k, p=[0.75 * (1 - p), 0.19 * (1 - p), 0.06 * (1 - p), p])
        ops["now"] = self.clocks(k)
        ops["new_end"] = np.where(np.isin(ops["kind"], (TOUCH, CREATE)), ops["now"] + rng.integers(-HOUR, 12 * HOUR, k), 0)
        fresh = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
        r = rng.random((3, k))
        pick = rng.integers(0, 2 ** 31, (2, k))
        known, tomb = self.issued, self.tombstoned_keys()
        for i in range(k):
            create = ops["kind"][i] == CREATE
            if i > 0 and r[0, i] < 0.1:
                ops["tok"][i] = ops["tok"][pick[0, i] % i]
            elif known.shape[0] == 0 or (create and r[1, i] < 0.85) or (not create and r[1, i] < 0.05):
                ops["tok"][i] = self.absent[pick[1, i] % 64] if not create and r[2, i] < 0.5 else fresh[i]
            elif create and tomb.shape[0] and r[2, i] < 0.5:
                ops["tok"][i] = tomb[pick[1, i] % tomb.shape[0]]
            else:
                ops["tok"][i] = known[pick[1, i] % known.shape[0]]
        return ops, rng.integers(0, m.U, k).astype(np.int32), rng.integers(0, m.D, k).astype(np.int32)

    # ---- readers
    def readers(self, tag):
        rng, m, ctx = self.rng, self.m, self.ctx
        # every key ever issued, and absent keys
        keys = np.concatenate([self.issued, self.absent])
        now = int(self.clocks(1)[0])
        if ctx:
            self.same_lookup(ctx.token_lookup(keys, now), m.lookup(keys, now), (tag, "lookup of every key", now))
        # one scan
        kind = str(rng.choice(["sparse", "sparse", "below_p90", "dense", "above"]))
        now, cutoff = self.pick_now(kind), int(rng.choice([INT64_MIN, self.t0 - 61 * DAY]))
        if ctx:
            same(ctx.scan(now, cutoff), m.scan(now, cutoff, self.mask), (tag, "scan", kind, now, cutoff))
        self.scanned_since_drop = True
        # one batch of sixteen: without a dense query on even steps (a batch that keeps its union), with one on odd steps
        qs = self.query_set(16, dense=bool(self.step % 2))
        self.last_scan, self.last_batch = (now, cutoff), qs
        self.one_batch((tag, "batch"), qs, False)
        if self.step % 4 == 3:
            self.one_batch((tag, "wide"), self.query_set(70, dense=False), True)
            now = self.pick_now(str(rng.choice(["sparse", "below_p90", "above", "dense"])))
            prev = now - int(rng.integers(0, 3 * DAY)) if now > INT64_MIN + 4 * DAY else INT64_MIN
            if ctx:
                assert np.array_equal(ctx.expired_queue(prev, now), m.expired_queue(prev, now)), (tag, "expired queue", prev, now)
        if ctx:
            self.info()

    @staticmethod
    def same_lookup(got, want, tag):
        """row and live of every key; end, user and start where the key was found (the header leaves them undefined elsewhere)"""
        for col in ("row", "live"):
            assert np.array_equal(got[col], want[col]), (tag, col, np.nonzero(got[col] != want[col])[0][:8])
        f = want["found"]
        for col in ("end", "user", "start"):
            assert np.array_equal(got[col][f], want[col][f]), (tag, col, np.nonzero(got[col][f] != want[col][f])[0][:8])

    def finish_one(self, tag, wide, qs, wants, after=None):
        """finish the oldest batch and compare it.  after: the model's answers once a turn begun behind the batch has landed —
        a batch that kept its union answers for the table before the turn, whole; of a batch without one (its queries were
        rerun on the general path at this finish) every query answers for the table before or after it (include/pie_scan.h)"""
        ctx = self.ctx
        ms = [int(x) for x in (ctx.scan_wide_finish() if wide else ctx.scan_batch_finish())]
        un = ctx.batch_read_union_wide() if wide else ctx.batch_read_union()
        if un is not None or after is None:
            assert ms == [int(w[2].size) for w in wants], (tag, "M per query")
            if un is not None:
                check_union(tag, un, wants, wide)
            for qi in range(len(qs)):
                same(ctx.batch_read_results(qi), wants[qi], (tag, "query", qi, qs[qi]))
        else:
            for qi in range(len(qs)):
                got = ctx.batch_read_results(qi)
                ok = [all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(got, w[qi])) and ms[qi] == w[qi][2].size for w in (wants, after)]
                assert any(ok), (tag, "a rerun query answers neither for the table before the turn nor for the one after", qi, qs[qi])
        return un is not None

    def one_batch(self, tag, qs, wide):
        rng, m, ctx = self.rng, self.m, self.ctx
        feeds = [(int(rng.integers(len(qs))), int(rng.integers(m.U))) for _ in range(3)]
        if not ctx:
            return
        wants = m.scan_many(qs)
        (ctx.scan_wide_begin if wide else ctx.scan_batch_begin)(qs)
        at_begin = self.info()
        self.finish_one(tag, wide, qs, wants)
        for qi, u in feeds:
            w = wants[qi]
            assert np.array_equal(ctx.batch_read_user_feed(qi, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "feed", qi, u)
        self.scanned_since_drop = True
        if not wide and self.turn_on_hot is not None:
            v = ctx.stats()["k1_variant"]
            info = self.info()
            if v & 0x800 and not v & 0x2000 and at_begin["hot_rows"] > 0 and info["hot_rows"] > 0 and info["hot_builds"] == self.turn_on_hot:
                self.saw("turn_on_live_hot_index_then_batch")
            self.turn_on_hot = None

    # ---- turns
    def apply_turn(self, tag, ops, user, disc, session):
        ctx, m = self.ctx, self.m
        is_create = ops["kind"] == CREATE
        if is_create.any() and m.covered < m.n:
            # rows the column does not cover: a create is refused and changes nothing; the turn without it answers for the prefix
            self.refused(tag, lambda: ctx.session_turn(ops, user, disc, m.U))
            self.saw("refused_create_on_short_column")
        if is_create.any() and (m.covered < m.n or m.n + int(is_create.sum()) > MAX_ROWS):
            ops, user, disc = ops[~is_create], user[~is_create], disc[~is_create]
            is_create = is_create[~is_create]
        if ops.shape[0] == 0:
            self.skipped += 1                    # a turn of creates alone, all of them refused: nothing was run
            return
        creates = int(is_create.sum())
        if creates:
            if self.column_last in ("compact_shrink", "compact_noshrink"):
                self.saw("create_after_" + self.column_last)
            if self.straddle == "appended":
                self.saw("compact_across_prefix_then_create")
            seen = set()
            for i in range(ops.shape[0]):        # a create whose key's row, as the turn finds it, is a maintenance call's tombstone
                key = key_of(ops["tok"][i])
                row = m.index.get(key, -1)
                if is_create[i] and key not in seen and row >= 0 and self.foreign[row] and m.end[row] == END_NONE:
                    self.saw("create_over_foreign_tombstone")
                    break
                seen.add(key)
            if self.cfg["ordered"] == 2 and self.scanned_since_drop:
                self.saw("host:creating_turn_in_ordered_chain")
        before = self.info() if ctx else None
        slots, cap = m.slots, m.cap
        logins = bool(creates and self.cfg["logins"])
        n_before = m.n
        in_order = bool(np.all(ops["now"][is_create] >= (int(m.start.max()) if m.n else INT64_MIN))) if creates else True
        probe = self.run_probe((tag, "before the turn")) if logins and ctx and before["ordered_rows"] > 0 else None
        want = m.turn(ops, user, disc)
        if logins:
            host_kept = self.login_host_states(creates, in_order, m.cap > cap, bool(np.any(m.end[n_before:] == END_NONE)))
        if ctx:
            got = ctx.session_turn(ops, user, disc, m.U) if session else ctx.token_turn(ops)
            same_turn(got, want, tag)
            f = want["found"]
            assert np.array_equal(got["user"][f], want["user"][f]) and np.array_equal(got["start"][f], want["start"][f]), (tag, "user / start")
            after = ctx.table_info()
            if logins:
                self.check_run_after_logins(tag, before, after, creates, in_order, m.cap > cap, n_before, probe)
            if creates and after["token_builds"] > before["token_builds"]:
                self.saw("create_doubled_slots")
            if creates and after["table_bytes"] > before["table_bytes"]:
                self.saw("create_outgrew_capacity")
            if before["ordered_rows"] > 0:
                if creates and after["ordered_rows"] == 0:
                    self.saw("creating_turn_dropped_ordered_run")
                if not creates and after["ordered_rows"] > 0:
                    self.saw("plain_turn_kept_ordered_run")
            if self.rebuilt_since_turn:
                self.saw("hot_index_rebuilt_between_turns")
            self.builds_at_turn, self.dropped_since_turn, self.rebuilt_since_turn = after["hot_builds"], False, False
            self.turn_on_hot = before["hot_builds"] if before["hot_rows"] > 0 else None
        else:                                    # the model alone: the two sizes it mirrors decide
            if creates and m.slots > slots:
                self.saw("create_doubled_slots")
            if creates and m.cap > cap:
                self.saw("create_outgrew_capacity")
        if logins and host_kept:
            self.since_compact = None
        if creates:
            self.issued = np.concatenate([self.issued, ops["tok"][is_create]])
            self.column_last, self.straddle = "turn", None
            self.scanned_since_drop = False
            if m.slots > slots or m.cap > cap:
                self.reshaped = True
        self.touched = True
        self.check_state(tag)

    # ---- turns that log in under pie_set_turn_ordered (cfg["logins"])
    def run_probe(self, tag):
        """the readers' last scan and last batch once more, against the model -> (the scan took the run, the batch took it).
        No draw: the model-only run makes none here either."""
        ctx, m = self.ctx, self.m
        now, cutoff = self.last_scan
        same(ctx.scan(now, cutoff), m.scan(now, cutoff, self.mask), (tag, "scan", now, cutoff))
        scan_on_run = bool(ctx.stats()["k1_variant"] & 0x2000)
        qs = self.last_batch
        wants = m.scan_many(qs)
        ctx.scan_batch_begin(qs)
        self.finish_one((tag, "batch"), False, qs, wants)
        return scan_on_run, bool(ctx.stats()["k1_variant"] & 0x2000)

    def login_host_states(self, creates, in_order, grew, ended_own):
        """what a host can say of a creating turn: the stand-ins the model-only run records"""
        on = bool(self.cfg["turn_ordered"])
        host_kept = on and in_order and not grew and creates <= 4096
        self.saw("host:login_grew_switch_on" if on and grew else "host:login_before_top" if not in_order else
                 "host:login_in_order_switch_on" if on else "host:login_in_order_switch_off")
        if host_kept and ended_own:
            self.saw("host:login_create_then_delete")
        if host_kept and self.since_compact:
            self.saw("host:login_since_compact_" + self.since_compact)
        if host_kept and self.revived_since_kept:
            self.saw("host:login_since_set_end_revived_row")
        if host_kept:
            self.host_kept_seen, self.revived_since_kept = True, False
        self.login_since_begin = True
        return host_kept

    def check_run_after_logins(self, tag, before, after, creates, in_order, grew, n_before, probe):
        """the run's bookkeeping behind a turn with creates, decided here wherever a host can decide it (include/pie_scan.h,
        pie_set_turn_ordered): switch off or a table that grew -> dropped; a valid run, the switch on, no growth, at most 4 096
        creates, no new user, every start at or after the table's top -> kept with every created row in it, nothing rebuilt, at
        most one re-spread; a create before the top -> kept or dropped (the 256 of the header are run positions), recorded.
        ordered_rows counts the rows the run HOLDS: rows that were tombstones (end = END_NONE) when it was built are not in it, so
        in a chain that deletes, a valid run reports fewer rows than the table has, and what a keeping turn owes is + creates; where
        the run held the whole table before, it holds the whole table afterwards.  Whether the run was valid before the turn is
        read from the device (a mode-1 run exists or not by the library's own choice): a run the library lost without cause before
        the turn goes unnoticed here, and is bounded only by the states the chains must reach."""
        ctx, m = self.ctx, self.m
        on = bool(self.cfg["turn_ordered"])
        rows = lambda i: int(i["ordered_rows"])
        valid = rows(before) > 0
        assert (after["table_bytes"] > before["table_bytes"]) == grew, (tag, "the model's capacity and the table's disagree on growth")
        if not on or grew:
            assert rows(after) == 0, (tag, "a run behind a creating turn with the switch off, or on columns that moved", rows(after))
            if valid and on:
                self.saw("growth_dropped_run_switch_on")
            return
        if not valid:
            return      # no run, or a valid one that holds no row (it reports 0 as well): nothing to decide
        kept = rows(after) > 0
        if in_order and creates <= 4096:
            assert kept, (tag, "in-order logins dropped a valid run", rows(before), n_before, creates)
        if not kept:
            self.saw("back_fill_dropped_run")
            return
        assert rows(after) == rows(before) + creates, (tag, "rows the kept run holds", rows(before), creates, rows(after))
        if rows(before) == n_before:
            assert rows(after) == m.n
        assert after["ordered_builds"] == before["ordered_builds"], (tag, "a kept run was rebuilt inside the turn")
        respread = int(after["ordered_respreads"]) - int(before["ordered_respreads"])
        assert respread in (0, 1), (tag, "re-spreads inside one turn", respread)
        self.saw("creating_turn_kept_ordered_run")
        if respread:
            self.saw("kept_run_respread")
        if self.since_compact:
            self.saw("kept_run_after_compact_" + self.since_compact)
        if before["hot_rows"] > 0 and after["hot_rows"] > 0:
            self.saw("kept_run_with_live_hot_index")
        if np.any(m.end[n_before:] == END_NONE):
            self.saw("kept_run_create_then_delete_in_turn")
        self.kept_builds = int(after["ordered_builds"])
        # the queries that took the run before the turn take it behind it, and answer for the table with the new rows
        scan_was, batch_was = probe
        scan_is, batch_is = self.run_probe((tag, "behind the keeping turn"))
        assert scan_is or not scan_was, (tag, "the scan that took the run before a keeping turn left it", self.last_scan)
        assert batch_is or not batch_was, (tag, "the batch that took the run before a keeping turn left it")
        if batch_was and batch_is:
            self.saw("kept_run_then_batch_on_run")
        info = ctx.table_info()
        assert rows(info) == rows(after) and info["ordered_builds"] == after["ordered_builds"], (tag, "the reads behind the turn ran on the run it kept")

    def do_logins(self, tag, variant="plain"):
        """a session turn whose creates carry clocks at or after every start of the table (tests/test_gpu_turn_ordered.logins),
        in any array order, among gets, touches and deletes of known keys and of keys the same turn creates.
        chain: 2 to 9 creates of one user, the starts descending; full: 25 creates of one user, more than a segment's spare slots
        (test_a_full_segment); undo: a create whose row a later op of the turn deletes; late: one create five minutes before the
        top; far: one create a day before the first row of the user with the most rows."""
        rng, m = self.rng, self.m
        if self.pending is not None:          # pie_token_append on the uncovered tail first: a create needs the whole column
            self.pending_due = self.step
            self.land_pending(tag)
            self.saw("host:login_landed_uncovered_tail")
        top = int(m.start.max()) if m.n else self.t0 - DAY
        kc = {"plain": int(rng.integers(1, 40)), "chain": int(rng.integers(2, 10)), "full": 25}.get(variant, int(rng.integers(2, 40)))
        ko = int(rng.integers(0, 60))
        if m.n + kc > MAX_ROWS:
            self.skipped += 1
            return
        new = rng.integers(0, 2 ** 64, (kc, 2), dtype=np.uint64)
        tomb = self.tombstoned_keys()
        if tomb.shape[0] and rng.random() < 0.5:
            new[kc - 1] = tomb[int(rng.integers(tomb.shape[0]))]      # a login under a key whose row a maintenance call ended
        at = top + np.sort(rng.integers(0, 1000, kc))
        user = rng.integers(0, m.U, kc)
        if variant in ("chain", "full"):
            user[:] = int(rng.integers(m.U))
            self.saw("host:login_full_segment" if variant == "full" else "host:login_chain_of_one_user")
        if variant == "chain":
            at = top + 10 * (kc - np.arange(kc))
        if variant == "late":
            at[-1] = top - 5 * 60 * 1000
        if variant == "far" and m.n:
            user[-1] = int(np.bincount(m.user, minlength=m.U).argmax())
            at[-1] = int(m.start[m.user == user[-1]].min()) - DAY
        creates = np.zeros(kc, TURN_OP)
        creates["tok"], creates["now"], creates["kind"] = new, at, CREATE
        creates["new_end"] = self.clocks(kc) + rng.integers(-HOUR, 12 * HOUR, kc)
        others = np.zeros(ko, TURN_OP)
        others["tok"] = self.some_keys(ko)
        others["kind"] = rng.choice([GET, TOUCH, DELETE], ko, p=[0.8, 0.15, 0.05])
        others["now"] = self.clocks(ko)
        others["new_end"] = np.where(others["kind"] == TOUCH, others["now"] + rng.integers(-HOUR, 12 * HOUR, ko), 0)
        if ko and kc > 1:
            others["tok"][0] = new[0]             # an op on a key the same turn creates, before or behind its create
            others["now"][0] = top
        order = rng.permutation(kc + ko) if variant != "chain" else np.arange(kc + ko)
        ops = np.concatenate([creates, others])[order]
        u = np.concatenate([user, rng.integers(0, m.U, ko)])[order].astype(np.int32)
        d = rng.integers(0, m.D, kc + ko).astype(np.int32)
        if variant == "undo" or rng.random() < 0.2:   # ... and a delete behind it: the row is in the table with `end` = END_NONE
            gone = np.zeros(1, TURN_OP)
            gone["tok"], gone["now"], gone["kind"] = new[int(rng.integers(kc))], top, DELETE
            ops, u, d = np.concatenate([ops, gone]), np.concatenate([u, u[:1]]), np.concatenate([d, d[:1]])
        self.apply_turn((tag, variant, kc, ko), ops, u, d, session=True)

    def do_logins_chain(self, tag):
        self.do_logins(tag, "chain")

    def do_logins_full(self, tag):
        self.do_logins(tag, "full")

    def do_logins_undo(self, tag):
        self.do_logins(tag, "undo")

    def do_logins_late(self, tag):
        self.do_logins(tag, "late")

    def do_logins_far(self, tag):
        self.do_logins(tag, "far")

    def do_dense_scans(self, tag):
        """(designed chains) three scans that select most of the table: what makes mode 1 build the ordered run"""
        now = self.pick_now("dense")
        self.last_scan = (now, INT64_MIN)
        for i in range(3):
            if self.ctx:
                same(self.ctx.scan(now, INT64_MIN), self.m.scan(now, INT64_MIN, self.mask), (tag, "dense scan", i, now))

    def do_session_turn(self, tag):
        k, p = int(self.rng.choice([1, 7, 64, 257, 300])), float(self.rng.choice([0.0, 0.1, 0.2, 0.4]))
        self.apply_turn((tag, k, p), *self.turn_ops(k, p), session=True)

    def do_creates(self, tag):
        """(designed chains) 300 ops, 40 % creates"""
        self.apply_turn((tag, 300, 0.4), *self.turn_ops(300, 0.4), session=True)

    def do_token_turn(self, tag):
        k = int(self.rng.choice([1, 7, 64, 257, 300]))
        self.apply_turn((tag, k), *self.turn_ops(k, 0.0), session=False)

    def some_keys(self, k):
        """k keys: issued ones (repeats happen), a tenth absent"""
        rng = self.rng
        pick, r = rng.integers(0, 2 ** 31, k), rng.random(k)
        keys = self.absent[pick % 64].copy()
        if self.issued.shape[0]:
            keys[r >= 0.1] = self.issued[pick[r >= 0.1] % self.issued.shape[0]]
        return keys

    def do_token_set_end(self, tag):
        rng, m = self.rng, self.m
        k = int(rng.choice([1, 7, 64, 257]))
        keys = self.some_keys(k)
        new_end = np.where(rng.random(k) < 0.2, END_NONE, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k)).astype(np.int64)
        now = END_NONE if rng.random() < 0.15 else int(self.clocks(1)[0])
        want = m.token_set_end(keys, new_end, now)
        if self.ctx:
            got = self.ctx.token_set_end(keys, new_end, now)
            assert np.array_equal(got, want), (tag, "rows written", np.nonzero(got != want)[0][:8])
        self.touched = True
        self.check_state((tag, k, now))

    def do_set_end(self, tag):
        """pie_set_end by row, on rows that carry keys: into and out of the top of the range, tombstones, revivals, repeats"""
        rng, m = self.rng, self.m
        if m.covered == 0:
            return self.do_token_set_end(tag)
        k = int(rng.choice([1, 7, 200]))
        rows = rng.integers(0, m.covered, k).astype(np.int32)
        r = rng.random(k)
        ne = np.where(r < 0.2, END_NONE, np.where(r < 0.7, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k), self.t0 - rng.integers(0, 100 * DAY, k))).astype(np.int64)
        twice = rng.integers(0, k, max(k // 10, 1))           # the same rows again with other values: the last element wins
        rows, ne = np.concatenate([rows, rows[twice]]), np.concatenate([ne, self.t0 + np.arange(twice.size)]).astype(np.int64)
        if self.ctx:
            self.ctx.set_end(rows, ne)
        was_dead = m.end[rows] == END_NONE
        m.set_end(rows, ne)
        if self.host_kept_seen and np.any(was_dead & (m.end[rows] != END_NONE)):
            self.revived_since_kept = True        # a tombstone came back to life between two logins that keep the run
        self.touched = True
        self.check_state((tag, k))

    # ---- appends: the keys come at once, or one to three steps later
    def do_append(self, tag):
        rng, m = self.rng, self.m
        k = int(rng.choice([1, 40, 300]))
        delay = int(rng.choice([0, 0, 1, 2, 3]))
        if m.n + k > MAX_ROWS:
            return self.do_token_turn(tag)
        top = int(m.start.max()) if m.n else self.t0 - DAY
        s2 = (top + np.sort(rng.integers(0, 4000, k))).astype(np.int64)
        e2 = np.where(rng.random(k) < 0.5, self.clocks(k) + rng.integers(-HOUR, 12 * HOUR, k), s2 + 12 * HOUR).astype(np.int64)
        u2, d2 = rng.integers(0, m.U, k).astype(np.int32), rng.integers(0, m.D, k).astype(np.int32)
        keys = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
        cap = m.cap
        if self.ctx:
            self.ctx.append_rows(s2, e2, u2, d2, m.U)
        m.append_rows(s2, e2, u2, d2)
        if m.cap > cap:
            self.reshaped = True
        if self.pending is None:
            self.pending, self.pending_due = keys, self.step + delay
        else:
            self.pending = np.concatenate([self.pending, keys])
        self.touched = True
        self.scanned_since_drop = False
        self.check_state((tag, k, "keys at step", self.pending_due))
        self.land_pending(tag)

    def land_pending(self, tag):
        m = self.m
        if self.pending is None or self.step < self.pending_due:
            return
        slots = m.slots
        if self.ctx:
            self.ctx.token_append(self.pending)
        m.token_append(self.pending)
        if m.slots > slots:
            self.reshaped = True
        self.issued = np.concatenate([self.issued, self.pending])
        self.pending = None
        self.column_last = "append"
        if self.straddle == "pending":
            self.straddle = "appended"
        self.check_state((tag, "token_append"))

    # ---- maintenance
    def listed(self, tag, got, want):
        if got is not None:
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "rows listed")
        self.foreign[want] = True
        self.check_state(tag)

    def do_delete_user(self, tag):
        m = self.m
        u = int(self.rng.integers(-1, m.U + 1))
        if m.n and self.rng.random() < 0.3:
            u = int(np.bincount(m.user, minlength=m.U).argmax())
        self.listed((tag, u), self.ctx.delete_user(u) if self.ctx else None, m.delete_user(u))

    def do_delete_users(self, tag):
        rng, m = self.rng, self.m
        kind = str(rng.choice(["1", "2", "17", "tile"]))
        if kind == "tile":
            tile = int(rng.integers((m.U + TILE_USERS - 1) // TILE_USERS))
            ids = np.arange(tile * TILE_USERS, min((tile + 1) * TILE_USERS, m.U))
        else:
            ids = rng.integers(0, m.U, int(kind))
        ids = np.concatenate([ids, ids[:1], [-1, m.U]])[rng.permutation(ids.size + 3)].astype(np.int32)   # a repeat, two unknown ids
        want_rows, want_per = m.delete_users(ids)
        if self.ctx:
            rows, per = self.ctx.delete_users(ids)
            assert np.array_equal(per, want_per), (tag, kind, "rows per element")
        self.listed((tag, kind), rows if self.ctx else None, want_rows)

    def do_prune(self, tag):
        m = self.m
        cutoff = int(np.quantile(m.start, float(self.rng.uniform(0, 0.05)))) + int(self.rng.integers(2)) if m.n else 0
        self.listed((tag, cutoff), self.ctx.prune_before(cutoff) if self.ctx else None, m.prune_before(cutoff))

    def do_retention(self, tag):
        m = self.m
        months, tz = int(self.rng.choice([1, 2, 3])), int(self.rng.choice([0, 0, 330 * 60000, -5 * HOUR]))
        first = int(m.start.min()) if m.n else self.t0
        now = int(add_months(np.array([first], np.int64), months, tz)[0]) + int(self.rng.integers(-DAY, 4 * DAY))
        self.listed((tag, now, months, tz), self.ctx.retention_purge(now, months, tz) if self.ctx else None, m.retention_purge(now, months, tz))

    def do_compact(self, tag, shrink=None, expired=None):
        rng, m = self.rng, self.m
        expired_draw, shrink_draw, q = rng.random() < 0.6, bool(rng.integers(2)), float(rng.choice([0.05, 0.1, 0.3]))
        shrink = shrink_draw if shrink is None else shrink
        expired = expired_draw if expired is None else expired
        live = m.end[m.end != END_NONE]
        dead_before = int(np.quantile(live, q)) if expired and live.size else END_NONE
        tag = (tag, dead_before, "shrink" if shrink else "in place")
        n_old, cov_old = m.n, m.covered
        want_maps = compact_maps(m.end, dead_before)[0]
        rows_before, keys_before = m.rows_of(self.issued), m.keys
        new_of_old = m.compact(dead_before, shrink)
        assert np.array_equal(new_of_old, want_maps), (tag, "the two models' maps")
        # the model's own consistency: every issued key answers its old row's new number; a key whose row was dropped answers
        # nothing, or an older row under the same key that was kept (the largest row under a key answers)
        rows_after, pushed = m.rows_of(self.issued), translate(new_of_old, rows_before)
        moved = pushed >= 0
        assert np.array_equal(rows_after[moved], pushed[moved]), (tag, "a kept row's key answers another row")
        older = ~moved & (rows_after >= 0)
        old_of_new = np.nonzero(new_of_old >= 0)[0]
        assert np.array_equal(keys_before[old_of_new[rows_after[older]]], self.issued[older]), (tag, "a dropped row's key answers a row of another key")
        assert np.all(old_of_new[rows_after[older]] < rows_before[older]), (tag, "a dropped row's key answers a later row")
        self.compactions += 1
        dropped = bool(np.any(new_of_old < 0))
        if self.ctx:
            assert self.ctx.compact_rows(dead_before, shrink) == m.n, (tag, "rows kept")
            got_maps = self.ctx.compact_maps()
            assert np.array_equal(got_maps[0], new_of_old) and np.array_equal(got_maps[1], old_of_new), (tag, "maps")
            probe = np.concatenate([rows_before[:64], [-1, n_old, n_old + 5]]).astype(np.int32)
            assert np.array_equal(self.ctx.compact_translate(probe), translate(new_of_old, probe)), (tag, "translate")
        if dropped:
            self.column_last = "compact_shrink" if shrink else "compact_noshrink"
            self.since_compact = "shrink" if shrink else "noshrink"
            self.reshaped = True
            self.scanned_since_drop = False
            if cov_old < n_old and np.any(new_of_old[:cov_old] < 0) and np.any(new_of_old[cov_old:] < 0):
                self.straddle = "pending"
            if self.pending is not None:
                self.pending = self.pending[new_of_old[cov_old:] >= 0]
            self.foreign = self.foreign[:n_old][new_of_old >= 0]
        self.touched = True
        self.check_state(tag)

    def do_compact_shrink(self, tag):
        self.do_compact(tag, True, True)

    def do_compact_in_place(self, tag):
        self.do_compact(tag, False, True)

    # ---- in-flight forms: begun with one to three batches in flight, everything finished in begin order
    def begin_batches(self, tag):
        rng, ctx = self.rng, self.ctx
        plans = []
        for _ in range(int(rng.integers(1, 4))):
            wide = bool(rng.random() < 0.3)
            plans.append((wide, self.query_set(70 if wide else 16, dense=False)))
        begun = []
        if ctx:
            for wide, qs in plans:
                if ctx.batch_room() <= 0:
                    break
                wants = self.m.scan_many(qs)
                (ctx.scan_wide_begin if wide else ctx.scan_batch_begin)(qs)
                begun.append((wide, qs, wants))
            self.scanned_since_drop = True
        return begun

    def finish_batches(self, tag, begun, after_turn=False):
        for b, (wide, qs, wants) in enumerate(begun):
            self.finish_one((tag, "batch in flight", b), wide, qs, wants, self.m.scan_many(qs) if after_turn else None)

    def do_inflight_turn(self, tag):
        ctx, m = self.ctx, self.m
        k = int(self.rng.choice([1, 7, 64, 257, 300]))
        ops, _, _ = self.turn_ops(k, 0.0)
        begun = self.begin_batches(tag)
        if self.cfg["logins"] and self.login_since_begin:
            self.saw("host:begin_after_login")
            self.login_since_begin = False
        if self.cfg["ordered"] == 2:
            self.saw("host:begin_in_ordered_chain")
        elif not ctx:                         # never a run: the begin is taken, and a synchronous mutator behind it refused
            self.saw("refused_mutator_while_turn_begun")
            if self.reshaped:
                self.saw("inflight_turn_after_reshape")
        if not ctx:
            m.turn(ops)
            return self.check_state(tag)
        if ctx.table_info()["ordered_rows"] > 0:
            # a valid ordered run: begin is refused; the batches land, and the turn goes through the synchronous call
            self.refused(tag, lambda: ctx.token_turn_begin(ops), unchanged=False)
            self.saw("refused_begin_on_ordered_run")
            if self.kept_builds == int(ctx.table_info()["ordered_builds"]):      # the very run a creating turn kept
                self.saw("kept_run_then_refused_inflight_begin")
            self.finish_batches(tag, begun)
            return self.apply_turn((tag, "synchronous"), ops, None, None, session=False)
        before = self.info()
        ctx.token_turn_begin(ops)
        self.refused(tag, lambda: ctx.token_turn(ops[:1]), unchanged=False)
        self.refused(tag, lambda: ctx.token_set_end(ops["tok"][:1], np.full(1, END_NONE), END_NONE), unchanged=False)
        if m.n:
            self.refused(tag, lambda: ctx.set_end(np.zeros(1, np.int32), np.full(1, self.t0, np.int64)), unchanged=False)
        self.saw("refused_mutator_while_turn_begun")
        want = m.turn(ops)
        self.finish_batches(tag, begun, after_turn=True)
        same_turn(ctx.token_turn_finish(), want, (tag, "the turn begun in flight"))
        if self.reshaped:
            self.saw("inflight_turn_after_reshape")
        if self.rebuilt_since_turn:
            self.saw("hot_index_rebuilt_between_turns")
        self.builds_at_turn, self.dropped_since_turn, self.rebuilt_since_turn = ctx.table_info()["hot_builds"], False, False
        self.turn_on_hot = before["hot_builds"] if before["hot_rows"] > 0 else None
        self.touched = True
        self.check_state(tag)

    def do_inflight_lookup(self, tag):
        ctx, m = self.ctx, self.m
        keys = np.concatenate([self.issued, self.absent])
        now = self.clocks(keys.shape[0])                  # one clock per key
        begun = self.begin_batches(tag)
        if self.reshaped:
            self.saw("inflight_lookup_after_reshape")
        if not ctx:
            return
        ctx.token_lookup_begin(keys, now)
        want = m.lookup(keys, now)
        self.finish_batches(tag, begun)
        self.same_lookup(ctx.token_lookup_finish(), want, (tag, "the lookup begun in flight"))
        self.check_state(tag)

    def do_inflight_purge(self, tag):
        """the purge tick: the expired queue begun beside the batches, then its rows tombstoned (purgeExpiredSessions)"""
        ctx, m = self.ctx, self.m
        live = m.end[m.end != END_NONE]                   # a tick that finds a few per cent of the sessions expired
        now = int(np.quantile(live, float(self.rng.uniform(0.0, 0.15)))) if live.size else self.t0
        begun = self.begin_batches(tag)
        if m.n == 0:                                      # (a begin for no rows only counts)
            self.skipped += 1
            if ctx:
                self.finish_batches(tag, begun)
            return
        if self.reshaped:
            self.saw("inflight_purge_after_reshape")
        if ctx:
            ctx.expired_queue_begin(END_NONE, now)
            self.finish_batches(tag, begun)
            rows = ctx.expired_queue_finish()
            assert np.array_equal(rows, m.expired_queue(END_NONE, now)), (tag, "the queue begun in flight", now)
            if rows.size:
                ctx.set_end(rows.astype(np.int32), np.full(rows.size, END_NONE))
        m.purge(now)
        self.touched = True
        self.check_state((tag, now))

    def do_turn_vs_batch(self, tag):
        """pie_session_turn with a batch in flight is refused; the batch answers, nothing has changed"""
        ctx, m = self.ctx, self.m
        ops, user, disc = self.turn_ops(7, 0.4)
        qs = self.query_set(16, dense=False)
        if ctx:
            wants = m.scan_many(qs)
            ctx.scan_batch_begin(qs)
            self.refused(tag, lambda: ctx.session_turn(ops, user, disc, m.U), unchanged=False)
            self.finish_one((tag, "the batch in flight"), False, qs, wants)
        self.saw("refused_session_turn_with_batch")
        self.check_state(tag)


# Fixed op lists through the same machinery, for the states the hot index and the ordered run decide: a table large enough for
# the index, turns around a compaction (the index is dropped with the table and rebuilt by the next batch), and the ordered run
# held across a create-free turn and dropped by a creating one.
DESIGNED = {
    "hot": ({"n": 20000, "U": 499, "D": 32, "hot": 1, "ordered": 0, "lanes": 3, "async": 1, "wide_ordered": 0},
            ["token_turn", "session_turn", "inflight_turn", "compact_in_place", "token_turn", "creates", "creates", "compact_shrink",
             "creates", "inflight_turn", "inflight_lookup", "inflight_purge", "token_turn"]),
    "ordered": ({"n": 3000, "U": 64, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 0, "wide_ordered": 1},
                ["token_turn", "creates", "token_turn", "inflight_turn", "compact_shrink", "token_turn", "creates", "inflight_turn"]),
}


def run_store_chain(pie, oracle, seed, cfg=None, script=None, log=None):
    return StoreChain(pie, oracle, seed, cfg, script, log).run()


def run_designed(pie, oracle, name):
    cfg, script = DESIGNED[name]
    return run_store_chain(pie, oracle, 9000 + sorted(DESIGNED).index(name), cfg, script)


# Chains that log in with pie_set_turn_ordered on (a dict of their own: DESIGNED's names give its chains their seeds).  A freshly
# loaded table fits its columns exactly: the first login grows them and drops the run, the readers' scan rebuilds it (mode 2), and
# the logins after that find room.  A compaction with PIE_COMPACT_SHRINK puts the table back into that state.
DESIGNED_LOGINS = {
    "kept": ({"n": 3000, "U": 64, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 0, "wide_ordered": 1, "turn_ordered": 1, "logins": 1},
             ["logins", "logins", "logins_full", "logins_full", "logins_chain", "logins_undo", "inflight_turn", "append", "logins",
              "compact_in_place", "logins", "delete_user", "prune", "logins", "compact_shrink", "logins", "logins", "retention",
              "logins_late", "logins", "session_turn", "logins"]),
    "far": ({"n": 3000, "U": 7, "D": 8, "hot": 0, "ordered": 2, "lanes": 1, "async": 1, "wide_ordered": 0, "turn_ordered": 1, "logins": 1},
            ["logins", "logins", "logins_far", "logins", "delete_users", "logins_far", "logins"]),
    # mode 1 on a table without skew: dense scans build the run and take it, the batches stay on the general pass and its hot index
    "hot": ({"n": 20000, "U": 499, "D": 32, "hot": 1, "ordered": 1, "lanes": 3, "async": 1, "wide_ordered": 0, "turn_ordered": 1, "logins": 1},
            ["logins", "dense_scans", "logins", "token_turn", "logins", "logins_undo", "logins_full", "inflight_turn"]),
    "off": ({"n": 700, "U": 64, "D": 8, "hot": 0, "ordered": 2, "lanes": 2, "async": 0, "wide_ordered": 0, "turn_ordered": 0, "logins": 1},
            ["logins", "logins", "logins_chain", "inflight_turn"]),
}


def run_designed_logins(pie, oracle, name):
    cfg, script = DESIGNED_LOGINS[name]
    return run_store_chain(pie, oracle, 9200 + sorted(DESIGNED_LOGINS).index(name), cfg, script)
