"""GPU: queued mutations and lane batches with NO host wait between them, against the numpy model (tests/table_model.py).

A production step is a burst of logins, a burst of touches and a batch, and nothing reads the table in between.  The rest of
the suite reads the columns back after every mutator, which drains the main stream before any reader begins: a missing event
edge between the main stream and a lane, a staging area reused or freed too early, or a launch moved behind the wrong upload
could not show there.  Here the model is advanced on the host alongside the calls and the device is compared with it only at
marked checkpoints.

THE RULE.  Between a mutator call and the `begin` of the next reader this file makes no call that waits for the device.  Every
waiting call below sits in set-up / tear-down code or in a function whose name starts with `checkpoint_`, and those are called
only after a reader has finished or at the end of a run.  (On every third step a touch is queued directly behind the last
`finish`, before that reader's results are read: the checkpoint that follows it is the reader's own.)

Which calls wait, read off binding.py and the entry points of pie_scan.hip:
  WAIT for the device
    read_columns, fetch_rows, shard_maps, synchronize, hot_layout, delete_user / prune_before / retention_purge / compact_rows
    and their shard forms (rows are read back), load_columns / gen_synthetic / shard_table (validation and key build);
    scan, scan_batch, scan_wide and every *_finish (the summary in pinned memory, or the wide batch's event);
    every reader of a finished result: read_results, read_user_feed, batch_read_results, batch_read_user_feed,
    batch_read_union, batch_read_union_wide, batch_fetch_requests (a copy and a stream wait each);
    stats (drains all streams when profiled scans are unresolved), table_info (waits for the timing event of the last
    hot-index build, once), and with it shard_append_rows called without local_size, which calls table_info;
    append_rows / shard_append_rows on the growth path (re-allocation), and every append_rows / set_end / shard_* mutator
    under PIE_ASYNC_MUTATIONS=0 or while the ordered run is valid (the waited form: the same calls, the same order).
  DO NOT WAIT (queued on the context's main stream, or host state only)
    append_rows in place, set_end, shard_set_end, shard_append_rows given local_size (the shard's size from the model),
    with PIE_ASYNC_MUTATIONS on and no valid ordered run; scan_begin, scan_batch_begin, scan_wide_begin; set_batch_lanes,
    batch_lanes, batch_room, set_disciplines.
  Inside the library a queued mutator still waits for the staging area it used two mutations ago and drains the main stream
  before it frees a grown area's device block, and a begin waits where it rebuilds keys, builds the hot index, allocates a
  lane or grows the union buckets.  Those waits are the code under test, not the test's.

A pass does NOT prove the ordering correct.  A race that is present need not fire on any one run, and this file does not loop
to provoke one: the fixed 30 steps per configuration are the whole run.  A pass proves only that the sequences the suite now
runs agree with the model.

No expected value comes from another GPU context: the model is the only source; the sharded pair is held against the
UNSHARDED model, shard by shard (table_model.shard_view), as test_gpu_shard_mutate.py does."""
import numpy as np
import pytest

import table_model as T
from table_model import ALL, DAY, HOUR, INT64_MIN, PIE_E_STATE, TableModel, check_union, ctx_with_env, same

pytestmark = pytest.mark.gpu

SEED, N0, U0, D = 20262, 1 << 18, 5000, 32
STEPS = 30
KS = (1, 64, 257, 1500)                                   # rows per append and elements per touch, in turn
READERS = ("scan", "batch16", "batch64", "three", "wide70")
THREE = (16, 40, 16)                                      # the three batches begun back to back (40: a second mask word)
HOT_DELTA_MIN = 1 << 16                                   # the hot index's delta holds at least this many moved rows

REPIN_AT = 13                                             # a step whose reader is "three": 14 begins before it, lanes 2, 3, 0 by the rule
REACHED = {}   # configuration id -> what its run recorded; filled by test_mixed_workload, read by the self-check after it


class Plain:
    """One unsharded context.  Its view is the model itself."""

    def __init__(self, pie, oracle, m, hot, async_mut, lanes, ordered):
        ctx = ctx_with_env(pie, hot, async_mut)
        self.ctxs = [ctx]
        self.m = m
        if ordered is not None:
            ctx.set_ordered_run(ordered)
        ctx.set_batch_lanes(lanes)
        ctx.load_columns(*m.columns(), m.U)
        ctx.set_disciplines(ALL, m.D)

    def views(self):
        return [self.m]

    def append(self, s, e, u, d, U):
        self.ctxs[0].append_rows(s, e, u, d, U)

    def touch(self, rows, vals):
        self.ctxs[0].set_end(rows, vals)

    def checkpoint_columns(self, tag):
        ctx, m = self.ctxs[0], self.m
        assert ctx.n == m.n and ctx.n_users == m.U, (tag, "shape")
        for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), m.columns()):
            assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "column " + name)


class Pair:
    """Two pie_shard_* contexts of world 2 on one GPU, driven by global id; the model stays unsharded."""

    WORLD = 2

    def __init__(self, pie, oracle, m, hot, async_mut, lanes, flags):
        self.m, self.oracle = m, oracle
        self.owner = T.shard_owner(oracle, np.zeros(0, np.int32), m.U, self.WORLD)
        self.ctxs = []
        for r in range(self.WORLD):
            ctx = ctx_with_env(pie, hot, async_mut)
            self.ctxs.append(ctx)
            ctx.set_batch_lanes(lanes)
            ctx.gen_synthetic(SEED, m.n, 0, m.n, m.U, m.D, flags)
            ctx.shard_table(r, self.WORLD)
            ctx.set_disciplines(ALL, m.D)

    def views(self):
        return [T.shard_view(self.m, r, self.owner)[0] for r in range(self.WORLD)]

    def append(self, s, e, u, d, U):
        """(the model has not taken the rows yet: the shards' sizes after the call are worked out here, on the host)"""
        self.owner = T.shard_owner(self.oracle, self.owner, U, self.WORLD)
        for r, ctx in enumerate(self.ctxs):
            kept = int(np.count_nonzero(self.owner[u] == r))
            users = max(int(np.count_nonzero(self.owner == r)), 1)
            got = ctx.shard_append_rows(s, e, u, d, U, local_size=(ctx.n + kept, users))
            assert got == (self.m.n, kept), ("first global row, rows kept", r, got)

    def touch(self, rows, vals):
        for ctx in self.ctxs:
            ctx.shard_set_end(rows, vals)

    def checkpoint_columns(self, tag):
        for r, ctx in enumerate(self.ctxs):
            v, rows, users = T.shard_view(self.m, r, self.owner)
            assert ctx.n == v.n and ctx.n_users == v.U, (tag, "rank", r, "shape")
            got_rows, got_users = ctx.shard_maps()
            assert np.array_equal(got_rows, rows) and np.array_equal(got_users[: users.size], users), (tag, "rank", r, "maps")
            for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), v.columns()):
                assert got.dtype == want.dtype and np.array_equal(got, want), (tag, "rank", r, "column " + name)


def new_users_for_every_rank(oracle, U, world):
    """the fewest new ids from U on that give every rank of `world` one: a growing append that brings them doubles every
    shard's user capacity, so that the later appends' new users fit in place"""
    k, seen = 0, set()
    while len(seen) < world:
        seen.add(oracle.shard_of(U + k, world))
        k += 1
    return k


def session_rows(oracle, rng, t_ms, k, U, first_new):
    """k sessions created from t_ms on, in creation order as a session store has them; users over all ids, the ids from
    first_new on (new in this call) on the first rows"""
    s = (t_ms + np.arange(k)).astype(np.int64)
    e = s + rng.integers(oracle.TTL_MS // 4, oracle.TTL_MS, k)
    u = rng.integers(0, U, k).astype(np.int32)
    fresh = min(U - first_new, k)
    u[:fresh] = np.arange(first_new, first_new + fresh)
    return s, e.astype(np.int64), u, rng.integers(0, D, k).astype(np.int32)


def make_target(pie, oracle, kind, n0, u0, hot=1, async_mut=1, lanes=3, ordered=None, flags=4):
    """The table loaded, then ONE growing append (64 rows, new users for every shard): from here on there is room in place."""
    m = TableModel(oracle)
    m.load(*oracle.gen(SEED, n0, 0, n0, u0, D, flags), u0, D)
    if kind == "pair":
        tg = Pair(pie, oracle, m, hot, async_mut, lanes, flags)
    else:
        tg = Plain(pie, oracle, m, hot, async_mut, lanes, ordered)
    rng = np.random.default_rng([SEED, n0])
    U = u0 + new_users_for_every_rank(oracle, u0, Pair.WORLD)
    s, e, u, d = session_rows(oracle, rng, oracle.T0_MS, 64, U, u0)
    u[U - u0:] = np.arange(64 - (U - u0)) % 16     # and rows for both shards
    tg.append(s, e, u, d, U)
    m.append_rows(s, e, u, d, U)
    tg.checkpoint_columns("after the growing append")
    return tg, m, rng


class LaneRule:
    """The lane a begin goes to, by the rule of include/pie_scan.h (round robin over the lanes in use; with three batches at
    most in flight no lane is ever full).  The C ABI does not report the lane: this is an INFERENCE, the rule applied to the
    begins the test made, with the lane count read back from pie_batch_lanes.  It places the re-pin and labels the records; what
    is observed of a batch is that its finish reports a real pass (checkpoint_batch)."""

    def __init__(self, lanes):
        self.lanes, self.rr = lanes, 0

    def next(self):
        if self.lanes <= 1:
            return 0
        lane = self.rr % self.lanes
        self.rr = (lane + 1) % self.lanes
        return lane


class Run:
    """One configuration: 30 mixed-workload steps."""

    def __init__(self, pie, oracle, kind="plain", hot=1, async_mut=1, lanes=3, ordered=None, repin_at=None):
        self.pie, self.oracle, self.kind, self.hot, self.ordered, self.repin_at = pie, oracle, kind, hot, ordered, repin_at
        self.tg, self.m, self.rng = make_target(pie, oracle, kind, N0, U0, hot, async_mut, lanes, ordered)
        self.rule = [LaneRule(lanes) for _ in self.tg.ctxs]
        self.rec = {"lane_above_0": 0, "hot_delta": 0, "hot_clean": 0, "wide_pass": 0, "queued_behind_finish": 0, "no_realloc": False, "repinned": False}
        self.builds_seen = [0 for _ in self.tg.ctxs]
        self.mutated_rows = 0

    # ---- one step's mutations and queries, all host work
    def plan(self, i):
        m, rng, o = self.m, self.rng, self.oracle
        k = KS[i % 4]
        new = 1 + i % 3 if i % 4 == 1 or i % 7 == 3 else 0
        U, n_old = m.U + new, m.n
        base = o.T0_MS + (i + 1) * 60000
        s, e, u, d = session_rows(o, rng, base, k, U, m.U)
        # the touch: rows the append just wrote first (row n_old is LIFTED two hours above its end: query 0 sits between the
        # two values), then rows that are live around `base`; repeats (the last value wins) and tombstones among them
        recent = max(k // 2, 1)
        live = np.nonzero(m.end > base - HOUR)[0]
        rows = np.concatenate([n_old + np.arange(recent), rng.choice(live, k - recent)]).astype(np.int32)
        vals = (base + rng.integers(-o.TTL_MS, o.TTL_MS, k)).astype(np.int64)
        vals[rng.random(k) < 0.2] = INT64_MIN
        vals[0] = e[0] + 2 * HOUR
        if k >= 8:
            rows[k // 2], rows[k - 1] = rows[2], rows[3]
        q0 = (int(e[0]) + HOUR, INT64_MIN, ALL)

        def query():
            cutoff = int(rng.choice([INT64_MIN, base - 2 * HOUR, o.T0_MS - 3 * DAY]))
            mask = ALL if rng.random() < 0.4 else int(rng.integers(1, 2 ** 32)) | (1 << int(rng.integers(0, D)))
            return int(base + rng.integers(-HOUR, 11 * HOUR)), cutoff, mask

        reader = READERS[i % 5]
        sizes = {"scan": (1,), "batch16": (16,), "batch64": (64,), "three": THREE, "wide70": (70,)}[reader]
        batches = [[q0] + [query() for _ in range(nq - 1)] for nq in sizes]
        return (s, e, u, d, U), (rows, vals), reader, batches

    def extra_touch(self, i):
        """the touch queued directly behind the last finish of every third step: rows the reader selected, killed or moved"""
        m, rng, o = self.m, self.rng, self.oracle
        base = o.T0_MS + (i + 1) * 60000
        live = np.nonzero(m.end > base)[0]
        rows = rng.choice(live, 64).astype(np.int32)
        vals = (base + rng.integers(-o.TTL_MS, o.TTL_MS, 64)).astype(np.int64)
        vals[:24] = INT64_MIN
        return rows, vals

    # ---- bookkeeping of the paths taken; called with no window open, or from a checkpoint
    def note_begins(self, ci, n_begun, wide):
        lanes = [self.rule[ci].next() for _ in range(n_begun)]
        info = self.tg.ctxs[ci].table_info()
        fresh = info["hot_builds"] > self.builds_seen[ci]
        self.builds_seen[ci] = info["hot_builds"]
        return {"hot_rows": info["hot_rows"], "fresh": fresh, "wide": wide, "lanes": lanes}

    def checkpoint_batch(self, tag, ci, bi, view, qs, wants, ms, note):
        ctx = self.tg.ctxs[ci]
        assert [int(x) for x in ms] == [int(w[2].size) for w in wants], (tag, "M per query")
        v = ctx.stats()["k1_variant"]
        un = ctx.batch_read_union_wide() if note["wide"] else ctx.batch_read_union()
        if un is not None:
            check_union(tag, un, wants, note["wide"])
            if note["wide"]:
                self.rec["wide_pass"] += 1
        # a batch whose finish reports a real pass on the general path and that kept its union (one that only fell back took a
        # lane and queued nothing on it); the lane itself is the rule's
        if (v & 0x1000) and not v & 0x2000 and un is not None and note["lanes"][bi] > 0 and self.ordered is None:
            self.rec["lane_above_0"] += 1
        # INFERRED, no stats field reports the delta: the pass read the 1-byte key with a hot index standing at its begin (the
        # library reads the index then: every `now` of this file lies above the fine key's base), and unless this very begin
        # built the index, every step since the build has moved rows into its delta
        if not note["wide"] and (v & 0x1800) == 0x1800 and not v & 0x2000 and note["hot_rows"] > 0:
            self.rec["hot_clean" if note["fresh"] else "hot_delta"] += 1
        which = range(len(qs)) if len(qs) <= 16 else sorted({0, len(qs) - 1} | {int(x) for x in self.rng.integers(0, len(qs), 6)})
        for qi in which:
            same(ctx.batch_read_results(qi), wants[qi], (tag, "query", qi, qs[qi]))
        u = int(self.rng.integers(view.U))
        w = wants[0]
        assert np.array_equal(ctx.batch_read_user_feed(0, u), w[2][w[1][u]:w[1][u + 1]]), (tag, "feed of user", u)

    def checkpoint_scan(self, tag, ci, q, want, m_got):
        ctx = self.tg.ctxs[ci]
        assert m_got == want[2].size, (tag, "M")
        same(ctx.read_results(), want, (tag, q))

    # ---- the steps
    def step(self, i):
        tg, m = self.tg, self.m
        ctxs = tg.ctxs
        tag = "step %d" % i
        (s, e, u, d, U), (rows, vals), reader, batches = self.plan(i)
        before = m.scan(*batches[0][0])
        if self.repin_at == i:
            # Nothing is in flight.  The very next calls are this step's mutators and then its three batches back to back; by
            # the round-robin rule the first goes to a lane above 0 and one of them to lane 3, which no batch has used yet.
            assert reader == "three"
            for ci, ctx in enumerate(ctxs):
                ctx.set_batch_lanes(1)
                ctx.set_batch_lanes(4)
                self.rule[ci].lanes = 4
                ahead = LaneRule(4)
                ahead.rr = self.rule[ci].rr
                lanes = [ahead.next() for _ in batches]
                assert lanes[0] > 0 and 3 in lanes, ("the re-pin step's batches go to lanes", lanes)
            self.rec["repinned"] = True
        # ---- WINDOW OPENS: mutators queued, the model advanced on the host beside them, no waiting call until the begin
        tg.append(s, e, u, d, U)
        m.append_rows(s, e, u, d, U)
        tg.touch(rows, vals)
        m.set_end(rows, vals)
        self.mutated_rows += 2 * rows.size
        views = tg.views()                                    # host only
        wants = [[v.scan_many(qs) for qs in batches] for v in views]
        # the step's own mutations decide query 0: a reader that ran ahead of either would answer as the table was before
        assert not np.array_equal(before[2], m.scan(*batches[0][0])[2]), (tag, "query 0 does not see the step's mutations")
        if reader == "scan":
            q = batches[0][0]
            for ctx in ctxs:
                ctx.scan_begin(q[0], q[1])
            # ---- WINDOW CLOSED
            got_m = [ctx.scan_finish() for ctx in ctxs]
            extra = self.queue_behind_finish(i)
            for ci in range(len(ctxs)):   # CHECKPOINT (the reader has finished)
                self.checkpoint_scan((tag, reader, "ctx", ci), ci, q, wants[ci][0][0], got_m[ci])
        else:
            wide = reader == "wide70"
            for qs in batches:   # ("three": back to back)
                for ctx in ctxs:
                    (ctx.scan_wide_begin if wide else ctx.scan_batch_begin)(qs)
            # ---- WINDOW CLOSED
            notes = [self.note_begins(ci, len(batches), wide) for ci in range(len(ctxs))]
            extra = None
            for bi, qs in enumerate(batches):
                ms = [ctx.scan_wide_finish() if wide else list(ctx.scan_batch_finish()) for ctx in ctxs]
                if bi == len(batches) - 1:
                    extra = self.queue_behind_finish(i)
                for ci in range(len(ctxs)):   # CHECKPOINT (the reader has finished)
                    self.checkpoint_batch((tag, reader, "batch", bi, "ctx", ci), ci, bi, views[ci], qs, wants[ci][bi], ms[ci], notes[ci])
        if extra is not None:
            m.set_end(*extra)
        if i % 10 == 9:   # CHECKPOINT (after a finished reader): the columns, bit for bit
            tg.checkpoint_columns(tag)

    def queue_behind_finish(self, i):
        """Every third step: a mutator directly behind the last finish, no result read in between, so that a main-stream
        mutation is queued while the lane's last launch may still run.  The results read afterwards are those of the table as
        the reader saw it (a touch leaves finished results alone, include/pie_scan.h); the model takes the touch after them."""
        if i % 3 != 2:
            return None
        rows, vals = self.extra_touch(i)
        self.tg.touch(rows, vals)
        self.mutated_rows += rows.size
        self.rec["queued_behind_finish"] += 1
        return rows, vals

    def run(self):
        tg = self.tg
        try:
            info0 = [ctx.table_info() for ctx in tg.ctxs]
            for i in range(STEPS):
                self.step(i)
            tg.checkpoint_columns("end")   # CHECKPOINT (the end)
            info1 = [ctx.table_info() for ctx in tg.ctxs]
            # no append re-allocated: the row capacity stands.  The user capacity is not reported: the users stayed inside what
            # the growing append left (it doubles what it outgrows), an indirect check; a re-allocation for users alone would
            # also drop the hot index, and hot_builds below would show the rebuild
            for a, b in zip(info0, info1):
                assert a["table_bytes"] == b["table_bytes"] and b["rows"] * 24 <= b["table_bytes"], ("an append re-allocated", a["table_bytes"], b["table_bytes"])
            assert self.m.U <= 2 * U0
            self.rec["no_realloc"] = True
            # the hot index: none when it is off or the batches run on the ordered run; otherwise ONE build, by the first batch
            # (all of this file's queries lie above the 90th percentile of `end`), never dropped: the rows moved since are
            # fewer than its delta holds
            assert self.mutated_rows < HOT_DELTA_MIN
            want_builds = 1 if self.hot and self.ordered is None else 0
            assert [b["hot_builds"] for b in info1] == [want_builds] * len(info1), ("hot_builds", [b["hot_builds"] for b in info1])
            assert [ctx.batch_lanes() for ctx in tg.ctxs] == [r.lanes for r in self.rule]
        finally:
            for ctx in tg.ctxs:
                ctx.close()
        return self.rec


CONFIGS = [("lanes%d-hot%d-async%d" % (lanes, hot, a), dict(lanes=lanes, hot=hot, async_mut=a, repin_at=REPIN_AT if (lanes, hot, a) == (3, 1, 1) else None))
           for lanes in (1, 3, 4) for hot in (1, 0) for a in (1, 0)]
CONFIGS.append(("ordered-run", dict(lanes=3, ordered=2)))
CONFIGS.append(("sharded-pair", dict(kind="pair", lanes=3)))


@pytest.mark.parametrize("name", [c[0] for c in CONFIGS])
def test_mixed_workload(pie, oracle, name):
    REACHED[name] = Run(pie, oracle, **dict(CONFIGS)[name]).run()


def test_mixed_workload_reached_every_path():
    missing = [c[0] for c in CONFIGS if c[0] not in REACHED]
    assert not missing, "runs %s failed or were deselected: their path records are missing, run the whole file" % missing
    print("paths reached:", REACHED)
    cfg = dict(CONFIGS)
    for name, rec in REACHED.items():
        c = cfg[name]
        general = c.get("ordered") is None
        assert rec["no_realloc"], (name, "an append re-allocated")
        assert rec["queued_behind_finish"] == STEPS // 3, (name, "touches queued directly behind a finish")
        if general and c["lanes"] > 1:
            assert rec["lane_above_0"] > 0, (name, "no batch with a real pass and a union on a lane above 0 (the lane is inferred from the "
                                             "header's round-robin rule: the C ABI reports none)")
        if general and c.get("hot", 1):
            assert rec["hot_delta"] > 0, (name, "no batch on the 1-byte key over a standing hot index after moved rows (the non-empty delta "
                                          "is inferred: no stats field reports it)")
        assert rec["repinned"] == (c.get("repin_at") is not None), (name, "the lanes were not re-pinned where the configuration says")
        if general:
            assert rec["wide_pass"] > 0, (name, "no wide pass")


# ------------------------------------------------------------------------------------------------ staging-area rotation
ROTATION = (1, 3000, 2, 6000, 1, 12000, 3, 3, 24000, 1, 48000, 5)   # append, touch, append, touch, ...


@pytest.mark.parametrize("kind,hot", [("plain", 1), ("pair", 1), ("plain", 0)])
def test_staging_rotation(pie, oracle, kind, hot):
    """Twelve queued mutations in a row.  An append stages k * 24 + 64 bytes (28 per row on a shard), a touch k * 12 + 64:
    the appends' area passes 64 KiB at 24000 rows and doubles again at 48000, the touches' at 6000 and 12000 elements, each
    while the other area's mutation is still queued behind it.  The batch behind them is the context's second: by the
    round-robin rule it runs on lane 1, behind the main stream only by the lane's event.  With the hot index on, the 48000-row
    append passes the delta's bound and drops the index, so that batch's begin rebuilds it and waits for the main stream
    while it does; with the index off nothing in the begin waits, and the large mutations are still queued when the lane's
    pass is launched."""
    n0, u0 = 1 << 17, 500
    tg, m, rng = make_target(pie, oracle, kind, n0, u0, hot=hot)
    o = oracle
    try:
        def queries(base):
            return [(int(base + rng.integers(-HOUR, 11 * HOUR)), int(rng.choice([INT64_MIN, base - 2 * HOUR])),
                     ALL if q % 3 == 0 else int(rng.integers(1, 2 ** 32))) for q in range(16)]

        # a batch first (lane 0): the hot index, where there is one, is built, and the mutations below are mirrored into it
        warm = queries(o.T0_MS)
        for ctx, v in zip(tg.ctxs, tg.views()):
            for got, want in zip(ctx.scan_batch(warm), v.scan_many(warm)):
                same(got, want, "warm-up batch")
        info0 = [ctx.table_info() for ctx in tg.ctxs]
        if kind == "plain":   # (a shard keeps its share of every append: checked below, by the capacity it ends with)
            assert m.n + sum(ROTATION[0::2]) <= info0[0]["table_bytes"] // 24
        # ---- WINDOW OPENS
        k_app = 0
        for j, k in enumerate(ROTATION):
            base = o.T0_MS + (j + 1) * 60000
            if j % 2 == 0:
                s, e, u, d = session_rows(o, rng, base, k, m.U, m.U)
                tg.append(s, e, u, d, m.U)
                m.append_rows(s, e, u, d, m.U)
                k_app = k
            else:   # rows of the append just before it first, then any rows; tombstones among the values
                named = min(k, k_app)
                rows = np.concatenate([m.n - k_app + np.arange(named), rng.integers(0, m.n, k - named)]).astype(np.int32)
                vals = (base + rng.integers(-o.TTL_MS, o.TTL_MS, k)).astype(np.int64)
                vals[rng.random(k) < 0.2] = INT64_MIN
                tg.touch(rows, vals)
                m.set_end(rows, vals)
        qs = queries(o.T0_MS + 13 * 60000)
        views = tg.views()
        wants = [v.scan_many(qs) for v in views]
        for ctx in tg.ctxs:
            ctx.scan_batch_begin(qs)
        # ---- WINDOW CLOSED
        for ctx, want in zip(tg.ctxs, wants):   # CHECKPOINT (the reader has finished)
            ms = list(ctx.scan_batch_finish())
            assert ms == [int(w[2].size) for w in want], "M per query after twelve queued mutations"
            un = ctx.batch_read_union()
            if un is not None:
                check_union("after twelve queued mutations", un, want, False)
            for qi in range(len(qs)):
                same(ctx.batch_read_results(qi), want[qi], ("after twelve queued mutations", "query", qi))
        tg.checkpoint_columns("after twelve queued mutations")   # CHECKPOINT (the end): bit for bit
        for a, ctx in zip(info0, tg.ctxs):
            assert ctx.table_info()["table_bytes"] == a["table_bytes"], "an append of the rotation re-allocated the table"
    finally:
        for ctx in tg.ctxs:
            ctx.close()


# ------------------------------------------------------------------------------------------------ finished results, later mutations
def refused(pie, tag, calls):
    for name, fn in calls:
        with pytest.raises(pie.PieError) as ei:
            fn()
        assert ei.value.code == PIE_E_STATE, (tag, name, "refused with", ei.value.code)


@pytest.mark.parametrize("async_mut", [1, 0])
def test_finished_results_under_later_mutations(pie, oracle, async_mut):
    """include/pie_scan.h: a touch leaves the results of a finished scan or batch as they were (only the `end` column of
    pie_batch_fetch_requests is the table's own, read when it is called); an append that adds rows or users ends them, and
    every reader returns PIE_E_STATE until the next finish."""
    tg, m, rng = make_target(pie, oracle, "plain", 60000, 300, async_mut=async_mut)
    ctx, o = tg.ctxs[0], oracle
    clock = [0]

    def queries(nq):
        base = o.T0_MS
        return [(int(base + rng.integers(-HOUR, 9 * HOUR)), int(rng.choice([INT64_MIN, base - 2 * HOUR])),
                 ALL if q % 3 == 0 else int(rng.integers(1, 2 ** 32))) for q in range(nq)]

    def touch_selected(want):
        """kill half of the rows the finished reader selected and move the rest: the table would now answer differently"""
        rows = want[2][:: max(want[2].size // 60, 1)][:60].astype(np.int32)
        assert rows.size >= 8
        vals = np.where(np.arange(rows.size) % 2 == 0, INT64_MIN, o.T0_MS + 20 * HOUR).astype(np.int64)
        ctx.set_end(rows, vals)
        m.set_end(rows, vals)

    def append_some(new_users=0):
        clock[0] += 1
        U = m.U + new_users
        s, e, u, d = session_rows(o, rng, o.T0_MS + clock[0] * 60000, 40, U, m.U)
        ctx.append_rows(s, e, u, d, U)
        m.append_rows(s, e, u, d, U)

    batch_readers = [("batch_read_results", lambda: ctx.batch_read_results(0)), ("batch_read_user_feed", lambda: ctx.batch_read_user_feed(0, 1)),
                     ("batch_read_union", lambda: ctx.batch_read_union()), ("batch_read_union_wide", lambda: ctx.batch_read_union_wide()),
                     ("batch_fetch_requests", lambda: ctx.batch_fetch_requests([0], [1])), ("batch_result_device_ptrs", lambda: ctx.batch_result_device_ptrs(0))]
    scan_readers = [("read_results", lambda: ctx.read_results()), ("read_user_feed", lambda: ctx.read_user_feed(1)),
                    ("result_device_ptrs", lambda: ctx.result_device_ptrs())]
    try:
        ctx.scan_batch(queries(3))   # lane 0; the batches below run on lanes 1 and 2
        # ---- a batch, then a queued touch, then a queued append
        qs = queries(16)
        wants = m.scan_many(qs)
        ctx.scan_batch_begin(qs)
        assert list(ctx.scan_batch_finish()) == [int(w[2].size) for w in wants]
        touch_selected(wants[0])
        assert not np.array_equal(m.scan(*qs[0])[2], wants[0][2]), "the touch does not change what query 0 selects"
        un = ctx.batch_read_union()
        if un is not None:
            check_union("after a queued touch", un, wants, False)
        for qi in range(16):
            same(ctx.batch_read_results(qi), wants[qi], ("after a queued touch", "query", qi))
        req_q = np.array([0, 0, 5, 15, 3], np.int32)
        req_u = np.array([1, 7, 7, m.U - 1, -1], np.int32)
        off, idx, st, en, di = ctx.batch_fetch_requests(req_q, req_u)
        for i, (q, u) in enumerate(zip(req_q.tolist(), req_u.tolist())):
            w = wants[q]
            feed = w[2][w[1][u]:w[1][u + 1]] if 0 <= u < m.U else np.zeros(0, np.int32)
            assert np.array_equal(idx[off[i]:off[i + 1]], feed), ("fetch_requests after a queued touch", i)
        assert np.array_equal(st, m.start[idx]) and np.array_equal(di, m.disc[idx])
        assert np.array_equal(en, m.end[idx]), "the `end` column of fetch_requests is the table's own, after the touch"
        append_some()
        refused(pie, "batch, touch, append", batch_readers)
        # ---- a batch, then directly a queued append (with new users)
        qs = queries(40)
        wants = m.scan_many(qs)
        ctx.scan_batch_begin(qs)
        assert list(ctx.scan_batch_finish()) == [int(w[2].size) for w in wants]
        append_some(new_users=2)
        refused(pie, "batch, append", batch_readers)
        # ---- a wide batch (run twice: the first one on a table grows the union slots and reruns its queries), touch, append
        qs = queries(70)
        wants = m.scan_many(qs)
        for _ in range(2):
            ctx.scan_wide_begin(qs)
            assert ctx.scan_wide_finish() == [int(w[2].size) for w in wants]
        touch_selected(wants[0])
        un = ctx.batch_read_union_wide()
        if un is not None:
            check_union("wide, after a queued touch", un, wants, True)
        for qi in (0, 33, 64, 69):
            same(ctx.batch_read_results(qi), wants[qi], ("wide, after a queued touch", "query", qi))
        append_some()
        refused(pie, "wide batch, touch, append", batch_readers)
        # ---- a single scan, touch, append; and a single scan, append
        q = queries(1)[0]
        want = m.scan(q[0], q[1], ALL)
        ctx.scan_begin(q[0], q[1])
        assert ctx.scan_finish() == want[2].size
        touch_selected(want)
        same(ctx.read_results(), want, "single scan, after a queued touch")
        for u in (0, 7, m.U - 1):
            assert np.array_equal(ctx.read_user_feed(u), want[2][want[1][u]:want[1][u + 1]]), ("feed after a queued touch", u)
        append_some()
        refused(pie, "scan, touch, append", scan_readers)
        want = m.scan(q[0], q[1], ALL)
        ctx.scan_begin(q[0], q[1])
        assert ctx.scan_finish() == want[2].size
        append_some(new_users=1)
        refused(pie, "scan, append", scan_readers)
        # the next finished reader is readable again, and sees everything that was queued
        qs = queries(16)
        wants = m.scan_many(qs)
        for got, w in zip(ctx.scan_batch(qs), wants):
            same(got, w, "the batch after all of it")
        tg.checkpoint_columns("end")
    finally:
        ctx.close()
