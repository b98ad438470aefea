"""pie_comm_prune_before / pie_comm_retention_purge / _tz / pie_comm_compact_rows in a fresh process on the one-GPU stand-in for
RCCL (the set-up is that of tests/comm_mutate_worker.py).  Every sharded table has a TWIN: an unsharded context that holds the
same columns and is given the plain call; the numpy model of tests/table_model.py keeps its tombstones throughout.
usage: comm_maint_worker.py CASE
  lists     worlds 1, 2, 3, 5 x tables of 1 row, 1 000 rows / 7 users, 50 000 rows / 300 users (some rows tombstoned beforehand):
            prune, retention under a fixed offset, retention under a zone of tests/golden/addmonths_zones.json
  edges     merged lists of exactly 0, 1, 255, 256, 257 and 65 537 rows (cutoffs from the sorted `start` column; 80 000 rows: with
            its tombstones the table still holds the longest list behind the five before it); a list that sits on one shard
  capacity  cap = total - 1: PIE_E_CAPACITY, everything tombstoned, the total reported, the full list readable
  refusal   a call while a pipelined step is uncollected: PIE_E_STATE, no shard changed
  compact   prune, compact (with and without PIE_COMPACT_SHRINK), then a chain of calls against the model"""
import json
import os
import sys

import numpy as np

from comm_mutate_worker import CASE, D, INT64_MIN, PIE_E_STATE, REPO, SEED, SPAN, T0, TOP, TTL, PieError, oracle_py, pie

sys.path.insert(0, os.path.join(REPO, "tests"))
from table_model import TableModel  # noqa: E402

PIE_E_CAPACITY = -5
MAINT, MINUTE = 3, 60000
ZONE = "America/New_York"
assert ZONE in json.load(open(os.path.join(REPO, "tests", "golden", "addmonths_zones.json")))["zones"]
TZ = oracle_py.tz_table(ZONE)


def table(n, U, dead_every=7):
    s, e, u, d = (a.copy() for a in oracle_py.gen(SEED, n, 0, n, U, D, 0))
    if n > 1:
        e[3::dead_every] = INT64_MIN  # tombstoned beforehand
    return s, e, u, d


class Pair:
    """A communicator over the shards of one table, the unsharded twin context, and the model."""

    def __init__(self, world, cols, U):
        self.world = world
        self.comm = pie.PieComm([0] * world)
        for r in range(world):
            c = self.comm.ctx(r)
            c.load_columns(*cols, U)
            c.shard_table(r, world)
        self.twin = pie.PieScan(0)
        self.twin.load_columns(*cols, U)
        self.m = TableModel(oracle_py)
        self.m.load(*cols, U, D)
        self.dropped = np.zeros(self.m.n, bool)  # global rows a compaction removed from the shards

    def close(self):
        self.comm.close()
        self.twin.close()

    def maps(self):
        out = []
        for r in range(self.world):
            c = self.comm.ctx(r)
            rows_g, users_g = c.shard_maps()
            out.append((rows_g.astype(np.int64), users_g[: c.n_users].astype(np.int64) if users_g[0] >= 0 else np.zeros(0, np.int64)))
        return out

    def owner(self):
        return np.array([pie.shard_of(g, self.world) for g in range(self.m.U)], np.int32)

    def check_sources(self, rows, src_rank, src_row):
        maps = self.maps()
        assert np.array_equal(src_rank, self.owner()[self.m.user[rows]])
        for r in range(self.world):
            sel = src_rank == r
            assert np.array_equal(maps[r][0][src_row[sel]], rows[sel]), r

    def listed(self, tag, got, twin_rows, *others):
        """got = (rows, src_rank, src_row) of the communicator; twin_rows the plain call's list on the twin"""
        rows, src_rank, src_row = got
        assert rows.dtype == np.int32 and np.array_equal(rows, twin_rows), (tag, self.world, rows.size, twin_rows.size)
        for o in others:
            assert np.array_equal(rows, o), (tag, self.world, rows.size, o.size)
        assert self.comm.last_n == rows.size and self.comm.queue_kind() == MAINT
        assert all(t >= 0 for t in self.comm.queue_timing())
        self.check_sources(rows, src_rank, src_row)
        return rows.size

    def prune(self, cutoff, tag="prune"):
        want = self.m.prune_before(cutoff)
        return self.listed(tag, self.comm.prune_before(cutoff, sources=True), self.twin.prune_before(cutoff), want)

    def retention(self, now, months, tz_offset_ms):
        oracle = oracle_py.retention_queue(self.m.start, self.m.end, now, months, tz_offset_ms)
        want = self.m.retention_purge(now, months, tz_offset_ms)
        return self.listed("retention", self.comm.retention_purge(now, months, tz_offset_ms, sources=True),
                           self.twin.retention_purge(now, months, tz_offset_ms), oracle, want)

    def retention_tz(self, now, months):
        oracle = oracle_py.retention_queue_tz(self.m.start, self.m.end, now, months, *TZ)
        self.m.end[oracle] = INT64_MIN
        return self.listed("retention_tz", self.comm.retention_purge(now, months, tz_table=TZ, sources=True),
                           self.twin.retention_purge(now, months, tz_table=TZ), oracle)

    def compare(self):
        """The sharded table against the twin (and the model) through the merged expired queue, read back column for column,
        and through a gathered batch."""
        ts, te, tu, td = self.twin.read_columns()
        held = ~self.dropped
        assert np.array_equal(te, self.m.end) and np.array_equal(ts, self.m.start) and np.all(te[self.dropped] == INT64_MIN)
        maps = self.maps()
        rows, src_rank, src_row = self.comm.expired_queue(INT64_MIN, 2 ** 62, sources=True)
        want = np.nonzero((te != INT64_MIN) & held)[0]
        assert np.array_equal(rows, want), (self.world, rows.size, want.size)
        cols = [self.comm.ctx(r).read_columns() for r in range(self.world)]
        for r in range(self.world):
            sel = src_rank == r
            s, e, u, d = (a[src_row[sel]] for a in cols[r])
            g = rows[sel]
            assert np.array_equal(s, ts[g]) and np.array_equal(e, te[g]) and np.array_equal(d, td[g]), r
            assert np.array_equal(maps[r][1][u], tu[g]), r
        # every shard's whole columns, tombstones included, are the twin's rows its map names
        for r in range(self.world):
            g = maps[r][0]
            assert np.array_equal(cols[r][1], te[g]) and np.array_equal(cols[r][0], ts[g]), r
        for r in range(self.world):
            self.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
        qs = [(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555), (T0 - TTL // 3, T0 - 3 * TTL, 0xAAAAAAAA), (T0 - SPAN // 2, T0 - SPAN, 0xFFFFFFFF)]
        ms = self.comm.scan_batch_gather(qs)
        for q, query in enumerate(qs):
            self.twin.set_disciplines(query[2], D)
            _, wo, wi = self.twin.scan(query[0], query[1])
            for a, b in zip((wo, wi), self.m.scan(*query)[1:]):
                assert np.array_equal(a, b), ("twin and model disagree", q)
            total = 0
            for r in range(self.world):
                off, idx = self.comm.read_gathered(0, r, q)
                assert ms[r][q] == idx.size
                total += idx.size
                rows_r, users_r = maps[r]
                for lu in range(users_r.size):
                    gu = int(users_r[lu])
                    assert np.array_equal(rows_r[idx[off[lu]:off[lu + 1]]], wi[wo[gu]:wo[gu + 1]]), (q, r, gu)
            assert total == wi.size
        return len(qs)


def case_lists():
    checks = 0
    for world in (1, 2, 3, 5):
        for n, U in ((1, 1), (1000, 7), (50000, 300)):
            p = Pair(world, table(n, U), U)
            s = np.sort(p.m.start)
            checks += p.prune(int(s[n // 10]) + 1)
            checks += p.retention(T0 - SPAN // 2 + 65 * 86400000, 2, -300 * MINUTE)
            checks += p.retention_tz(T0 - SPAN // 2 + 75 * 86400000, 2)
            checks += p.compare()
            checks += p.prune(int(s[n // 10]) + 1) == 0   # a second identical call finds nothing
            assert p.comm.queue_read(0).size == 0
            p.close()
    print("lists ok: %d checks" % checks)


def cutoff_for(p, length):
    """the cutoff below which exactly `length` non-tombstoned rows start"""
    live = np.sort(p.m.start[p.m.end != INT64_MIN])
    if length == 0:
        return int(live[0])
    assert live[length - 1] < live[length], "the generator tied two starts at the boundary"
    return int(live[length])


def case_edges():
    for world in (1, 2, 3, 5):
        n, U = 80000, 300
        if world == 3:  # every shard's lists are brought over as lists held on another device are
            os.environ["PIE_COMM_STAGE_ALL"] = "1"
        p = Pair(world, table(n, U), U)
        os.environ.pop("PIE_COMM_STAGE_ALL", None)
        for length in (0, 1, 255, 256, 257, 65537):
            assert p.prune(cutoff_for(p, length), "edge %d" % length) == length
        p.compare()
        p.close()
    # every listed row on one shard: the rows below the cutoff belong to users of one rank
    for world in (2, 5):
        n, U = 50000, 300
        s, e, u, d = table(n, U)
        owner = np.array([pie.shard_of(g, world) for g in range(U)], np.int32)
        target = int(owner[0])
        cutoff = int(np.sort(s)[n // 3])
        away = (owner[u] != target) & (s < cutoff)
        s[away] += cutoff - int(s.min()) + 1
        p = Pair(world, (s, e, u, d), U)
        rows, src_rank, _ = p.comm.prune_before(cutoff, sources=True)
        assert rows.size > 256 and np.all(src_rank == target)
        assert np.array_equal(rows, p.twin.prune_before(cutoff)) and np.array_equal(rows, p.m.prune_before(cutoff))
        p.compare()
        p.close()
    print("edges ok")


def case_capacity():
    for world in (1, 3):
        p = Pair(world, table(50000, 300), 300)
        cutoff = int(np.sort(p.m.start)[20000])
        want = p.m.prune_before(cutoff)
        try:
            p.comm.prune_before(cutoff, cap=want.size - 1)
            raise AssertionError("the short list went through")
        except PieError as err:
            assert err.code == PIE_E_CAPACITY, err
        assert p.comm.last_n == want.size
        rows, src_rank, src_row = p.comm.queue_read(0, sources=True)
        assert np.array_equal(rows, want)
        p.check_sources(rows, src_rank, src_row)
        assert np.array_equal(p.twin.prune_before(cutoff), want)
        p.compare()   # everything is tombstoned all the same
        p.close()
    print("capacity ok")


def case_refusal():
    p = Pair(3, table(50000, 300), 300)
    before = [p.comm.ctx(r).read_columns() for r in range(3)]
    for r in range(3):
        p.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
    calls = (lambda: p.comm.prune_before(TOP), lambda: p.comm.retention_purge(TOP + 100 * 86400000, 2),
             lambda: p.comm.retention_purge(TOP + 100 * 86400000, 2, tz_table=TZ), lambda: p.comm.compact_rows())

    def refused():
        for fn in calls:
            try:
                fn()
                raise AssertionError("the call went through")
            except PieError as err:
                assert err.code == PIE_E_STATE, err

    p.comm.step_reserve(1, 0, 1 << 16)
    p.comm.step_begin([(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555)])
    refused()
    p.comm.step_finish()
    refused()
    p.comm.step_collect()
    after = [p.comm.ctx(r).read_columns() for r in range(3)]
    for a, b in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert p.comm.table_size() == (50000, 300)
    # a bad argument is refused by every shard before any runs
    try:
        p.comm.retention_purge(TOP, 2, tz_offset_ms=1)
        raise AssertionError("a fractional-minute offset went through")
    except PieError as err:
        assert err.code == -1, err
    after = [p.comm.ctx(r).read_columns() for r in range(3)]
    for a, b in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    p.close()
    print("refusal ok")


def case_compact():
    checks = 0
    for world, shrink in ((2, False), (3, True), (5, False), (5, True)):
        n, U = 50000, 300
        p = Pair(world, table(n, U), U)
        m = p.m
        rng = np.random.default_rng(world)
        keys = rng.integers(1, 2 ** 63, (n, 2), dtype=np.uint64)
        p.comm.token_set(keys)
        p.prune(int(np.sort(m.start)[n // 4]))
        live = m.end != INT64_MIN
        kept_total, kept_local = p.comm.compact_rows(INT64_MIN, shrink=shrink)
        p.dropped = ~live
        assert kept_total == int(live.sum()) and sum(kept_local) == kept_total and len(kept_local) == world
        owner = p.owner()
        assert kept_local == [int((live & (owner[m.user] == r)).sum()) for r in range(world)]
        assert p.comm.table_size() == (n, U)
        assert p.comm.queue_kind() == 0
        checks += p.compare()
        # appends start at N_g
        k = 300
        s = (TOP + np.arange(k)).astype(np.int64)
        e = s + rng.integers(TTL // 4, TTL, k)
        u = rng.integers(0, U + 2, k).astype(np.int32)
        u[:2] = (U, U + 1)
        d = rng.integers(0, D, k).astype(np.int32)
        assert p.comm.append_rows(s, e, u, d, U + 2) == n
        m.append_rows(s, e, u, d, U + 2)
        p.twin.append_rows(s, e, u, d, U + 2)
        p.dropped = np.concatenate([p.dropped, np.zeros(k, bool)])
        keys2 = rng.integers(1, 2 ** 63, (k, 2), dtype=np.uint64)
        p.comm.token_append(keys2)
        keys = np.concatenate([keys, keys2])
        assert p.comm.table_size() == (n + k, U + 2)
        # touches that name kept and dropped rows: a dropped row is a row no shard holds
        rows = np.concatenate([np.nonzero(p.dropped)[0][:50], np.nonzero(~p.dropped)[0][::97], [n + 5, n + 5]]).astype(np.int32)
        vals = (TOP + rng.integers(-TTL, TTL, rows.size)).astype(np.int64)
        vals[::5] = INT64_MIN
        p.comm.set_end(rows, vals)
        held = ~p.dropped[rows]
        m.set_end(rows[held], vals[held])
        p.twin.set_end(rows[held], vals[held])
        # deleteSessionsForUser for a set
        ids = np.array([0, 5, U + 1, 299, 5, -1, U + 2], np.int32)
        want = np.sort(np.concatenate([m.delete_user(int(x)) for x in ids.tolist()]))
        got, per, _ = p.comm.delete_users(ids)
        assert np.array_equal(got, want), (world, got.size, want.size)
        p.twin.delete_users(ids)
        # getSession by token on the column set before the compaction
        now = TOP
        ask = np.concatenate([np.nonzero(p.dropped)[0][:40], np.nonzero(~p.dropped)[0][::53], [n, n + k - 1]])
        ans = p.comm.token_lookup(keys[ask], now)
        gone = p.dropped[ask]
        assert np.all(ans["row"][gone] == -1) and np.array_equal(ans["row"][~gone], ask[~gone])
        assert np.array_equal(ans["live"][~gone].astype(bool), m.end[ask[~gone]] > now)
        assert np.array_equal(ans["end"][~gone], m.end[ask[~gone]]) and np.array_equal(ans["user"][~gone], m.user[ask[~gone]])
        for prev, t in ((INT64_MIN, 2 ** 62), (TOP - TTL, TOP), (TOP, TOP + TTL)):
            assert np.array_equal(p.comm.expired_queue(prev, t), m.expired_queue(prev, t)), (world, prev, t)
            checks += 1
        checks += p.compare()
        # and it ages again: a second prune and compaction on the compacted shards
        p.prune(int(np.sort(m.start)[n // 2]))
        live = (m.end != INT64_MIN) & ~p.dropped
        kept_total, _ = p.comm.compact_rows(INT64_MIN, shrink=shrink)
        p.dropped = ~live
        assert kept_total == int(live.sum()) and p.comm.table_size() == (n + k, U + 2)
        checks += p.compare()
        p.close()
    print("compact ok: %d checks" % checks)


if __name__ == "__main__":
    {"lists": case_lists, "edges": case_edges, "capacity": case_capacity, "refusal": case_refusal, "compact": case_compact}[CASE]()
    sys.stdout.flush()
