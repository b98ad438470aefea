"""A whole turn on sharded tables (pie_shard_token_turn on every shard, pie_comm_token_turn behind the communicator), in a fresh
process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): several shards of one table on GPU 0.  The model is the UNSHARDED
TurnModel of tests/turn_model.py, in global ids: the same seeded turns must give its answers element for element.
usage: comm_token_turn_worker.py CASE
  worlds   worlds 1, 2, 3, 5: seeded turns (chains on a few keys, unknown keys, tombstoned and expired rows, clocks of their own),
           alternately through PieComm.token_turn and through shard_token_turn on every shard; columns, expired queues and
           gathered feeds equal the model's afterwards
  errors   refusal while a pipelined step is uncollected; a turn one shard refuses, or with a bad op, changes no shard"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
CASE = sys.argv[1]
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_turn.so")
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import PieError
from token_model import END_NONE
from turn_model import DELETE, GET, TOUCH, TURN_OP, TurnModel

T0, SPAN, TTL, SEED, D = oracle_py.T0_MS, oracle_py.SPAN_MS, oracle_py.TTL_MS, 0x5EED5EED, 32
TOP = T0 + SPAN
PIE_E_INVAL, PIE_E_STATE = -1, -6


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


class Live:
    """A communicator over one synthetic table with a key per row, and the unsharded TurnModel, kept in step."""

    def __init__(self, world, n, U):
        self.world, self.U = world, U
        self.comm = pie.PieComm([0] * world)
        self.comm.gen_synthetic_sharded(SEED, n, U, D, 0)
        self.tm = TurnModel(*oracle_py.gen(SEED, n, 0, n, U, D, 0))
        self.keys = random_keys(100 + world, n)
        self.comm.token_set(self.keys)
        self.tm.token_set(self.keys)
        self.rng = np.random.default_rng(world)
        self.owner = np.array([pie.shard_of(int(u), world) for u in range(U)], np.int32)

    def random_ops(self, k, now):
        """half of the ops on 8 keys (5 live rows, an expired one, a tombstone if there is one, an unknown key), the rest on keys
        of the table and unknown ones; clocks of their own on both sides of `now`"""
        rng, tm = self.rng, self.tm
        live = np.nonzero(tm.end > now + TTL // 8)[0]
        expired = np.nonzero((tm.end <= now - TTL // 8) & (tm.end != END_NONE))[0]
        tomb = np.nonzero(tm.end == END_NONE)[0]
        eight = np.concatenate([self.keys[rng.choice(live, 5, replace=False)], self.keys[expired[:1]],
                                self.keys[tomb[:1]] if tomb.size else random_keys(7, 1), random_keys(8, 1)])
        ops = np.zeros(k, TURN_OP)
        chain = rng.random(k) < 0.5
        others = np.concatenate([self.keys[rng.integers(0, self.keys.shape[0], k)], random_keys(int(rng.integers(1 << 30)), k)])[rng.permutation(2 * k)[:k]]
        ops["tok"] = np.where(chain[:, None], eight[rng.integers(0, 8, k)], others)
        ops["now"] = now + rng.integers(-TTL // 2, TTL // 2, k)
        ops["kind"] = rng.choice([GET, TOUCH, DELETE], k, p=[0.5, 0.35, 0.15])
        ops["new_end"] = np.where(ops["kind"] == TOUCH, ops["now"] + rng.integers(-TTL // 8, TTL, k), 0)
        return ops

    def through_comm(self, ops, tag):
        got, want = self.comm.token_turn(ops), self.tm.turn(ops)
        f = want["row"] >= 0          # (a delete that met a tombstone merges as a key nobody holds: user and start are undefined)
        for col in ("row", "live", "end"):
            assert np.array_equal(got[col], want[col]), (tag, col)
        for col in ("user", "start"):
            assert np.array_equal(got[col][f], want[col][f]), (tag, col)
        assert np.array_equal(got["owner"][f], self.owner[want["user"][f]]) and np.all(got["owner"][~want["found"]] == -1), (tag, "owner")
        return want

    def through_shards(self, ops, tag):
        """the same call on every shard: a shard answers the ops whose key it holds as the unsharded table does, the others -1 / 0"""
        want = self.tm.turn(ops)
        holder = np.where(want["found"], self.owner[np.where(want["found"], want["user"], 0)], -1)
        for r in range(self.world):
            got = self.comm.ctx(r).shard_token_turn(ops)
            mine = holder == r
            for col in ("row", "live", "end", "user", "start"):
                assert np.array_equal(got[col][mine], want[col][mine]), (tag, r, col)
            assert np.all(got["row"][~mine] == -1) and not got["live"][~mine].any() and np.all(got["end"][~mine] == END_NONE), (tag, r, "not held")
        return want

    def check_columns(self):
        total = 0
        for r in range(self.world):
            c = self.comm.ctx(r)
            rows_g, users_g = c.shard_maps()
            s, e, u, d = c.read_columns()
            total += rows_g.size
            assert np.array_equal(s, self.tm.start[rows_g]) and np.array_equal(e, self.tm.end[rows_g]), r
            assert np.array_equal(users_g[u] if rows_g.size else u, self.tm.user[rows_g]), r
        assert total == self.tm.start.shape[0]

    def check_queues_and_feeds(self, now):
        tm = self.tm
        for prev, at in ((END_NONE, 2 ** 62), (now - TTL, now), (now, now + TTL)):
            assert np.array_equal(self.comm.expired_queue(prev, at), oracle_py.expired_queue(tm.end, prev, at)), (prev, at)
        maps = []
        for r in range(self.world):
            c = self.comm.ctx(r)
            c.set_disciplines(0xFFFFFFFF, D)
            rows_g, users_g = c.shard_maps()
            maps.append((rows_g, users_g[: c.n_users] if users_g[0] >= 0 else np.zeros(0, np.int32)))
        qs = [(now - 977 * q, now - (2 + q % 2) * TTL, (0x55555555, 0xAAAAAAAA, 0xFFFFFFFF)[q % 3]) for q in range(3)]
        want = [oracle_py.scan(tm.start, tm.end, tm.user, tm.disc, self.U, *q) for q in qs]
        self.comm.scan_batch_gather(qs)
        for q in range(len(qs)):
            _, wo, wi = want[q]
            total = 0
            for r in range(self.world):
                off, idx = self.comm.read_gathered(0, r, q)
                total += idx.size
                rows_r, users_r = maps[r]
                for lu in range(users_r.size):
                    gu = int(users_r[lu])
                    assert np.array_equal(rows_r[idx[off[lu]:off[lu + 1]]], wi[wo[gu]:wo[gu + 1]]), (q, r, gu)
            assert total == wi.size


def case_worlds():
    turns = 0
    for world, n, U in [(1, 20000, 300), (2, 20000, 300), (3, 20000, 300), (5, 20000, 7)]:
        t = Live(world, n, U)
        now = int(np.percentile(t.tm.end, 60))
        seen = set()
        for k in (0, 1, 2, 255, 256, 257, 1025, 300):
            ops = t.random_ops(k, now) if k else np.zeros(0, TURN_OP)
            if k == 300:                                  # every op on one token: one lane of one shard walks them all
                ops["tok"] = t.keys[np.nonzero(t.tm.end > now + TTL // 2)[0][0]]
            for via in (t.through_comm, t.through_shards):   # two turns of each size, one each way
                want = via(ops, (world, k, via.__name__))
                seen |= {(int(kd), int(lv), bool(r >= 0)) for kd, lv, r in zip(ops["kind"], want["live"], want["row"])}
                turns += 1
                if k:
                    ops = t.random_ops(k, now)
            t.check_columns()
        assert {(GET, 1, True), (GET, 0, True), (GET, 0, False), (TOUCH, 1, True), (TOUCH, 0, True), (TOUCH, 0, False), (DELETE, 0, True),
                (DELETE, 0, False)} <= seen, sorted(seen)
        assert t.comm.token_turn(np.zeros(0, TURN_OP))["owner"].shape == (0,)
        t.check_queues_and_feeds(now)
        t.comm.close()
    print("worlds ok: %d turns" % turns)


def case_errors():
    t = Live(3, 20000, 300)
    now = int(np.percentile(t.tm.end, 60))
    ops = t.random_ops(64, now)

    def columns():
        return [t.comm.ctx(r).read_columns()[1].copy() for r in range(3)]

    before = columns()

    def refused(code, fn, text=None):
        try:
            fn()
            raise AssertionError("the call went through")
        except PieError as e:
            assert e.code == code and (text is None or text in str(e)), e

    def unchanged(ranks=(0, 1, 2)):
        after = columns()
        assert all(np.array_equal(after[r][: before[r].shape[0]], before[r]) for r in ranks)

    # a pipelined step begun and not collected, then finished and not collected
    for r in range(3):
        t.comm.ctx(r).set_disciplines(0xFFFFFFFF, D)
    t.comm.step_reserve(1, 0, 1 << 16)
    t.comm.step_begin([(TOP - TTL // 3, TOP - 3 * TTL, 0x55555555)])
    refused(PIE_E_STATE, lambda: t.comm.token_turn(ops))
    t.comm.step_finish()
    refused(PIE_E_STATE, lambda: t.comm.token_turn(ops))
    t.comm.step_collect()
    unchanged()
    # a bad op anywhere in the turn: no shard applies any of it
    bad = ops.copy()
    bad["kind"][63] = 7
    refused(PIE_E_INVAL, lambda: t.comm.token_turn(bad))
    bad = ops.copy()
    bad["reserved"][0] = 1
    refused(PIE_E_INVAL, lambda: t.comm.token_turn(bad))
    refused(PIE_E_INVAL, lambda: t.comm.ctx(2).shard_token_turn(bad))
    assert t.comm._lib.pie_comm_token_turn(t.comm._c, None, 3, None, None, None, None, None, None) == PIE_E_INVAL
    unchanged()
    # a context that is not sharded has no shard form
    with pie.PieScan(0) as plain:
        plain.load_columns(t.tm.start[:100], t.tm.end[:100], t.tm.user[:100], t.tm.disc[:100], t.U)
        plain.token_set(t.keys[:100])
        refused(PIE_E_STATE, lambda: plain.shard_token_turn(ops))
        assert plain.token_turn(ops[:0])["row"].shape == (0,)
    # one shard holds a row its map does not cover: the whole turn is refused and no shard changes
    c1 = t.comm.ctx(1)
    c1.append_rows([TOP], [TOP + TTL], [0], [1], c1.n_users)
    refused(PIE_E_STATE, lambda: t.comm.token_turn(ops), "rank 1")
    unchanged()
    # the other shards still answer for themselves
    want = t.tm.turn(ops)
    got = t.comm.ctx(0).shard_token_turn(ops)
    mine = want["found"] & (t.owner[np.where(want["found"], want["user"], 0)] == 0)
    assert mine.any() and np.array_equal(got["row"][mine], want["row"][mine]) and np.array_equal(got["end"][mine], want["end"][mine])
    t.comm.close()
    print("errors ok")


if __name__ == "__main__":
    {"worlds": case_worlds, "errors": case_errors}[CASE]()
