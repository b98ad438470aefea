"""GPU: turns that log in keep the ordered run (pie_set_turn_ordered; k_ord_stage_rows in sph-pie_amd/csrc/pie_ordered.h, the
create turn's host flow in pie_scan.hip).  A context with the switch on is driven against tests/session_turn_model.py and the
oracle, and beside a twin context that makes the same calls one by one (pie_append_rows of one row + pie_token_append, a
pie_token_turn of one op).  The shapes are the existing ordered-run test's: 20 000 rows, 499 users, 32 disciplines, mode 2, one
scan to build the run; `k1_variant & 0x2000` says a scan took the run."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from session_turn_model import CREATE, SessionTurnModel
from test_gpu_session_turn import one_by_one, random_keys, run_turn, state_matches
from token_model import END_NONE
from turn_model import DELETE, GET, TOUCH, make_ops

pytestmark = pytest.mark.gpu

N, USERS, DISCS = 20_000, 499, 32
HOUR, DAY = 3600 * 1000, 86400 * 1000
PIE_E_INVAL, PIE_E_STATE = -1, -6
ALL = (1 << DISCS) - 1
ROOM = 6000


class Bed:
    """a context on a keyed table with the model beside it; check() scans a sparse, a dense and a late query against the oracle"""

    def __init__(self, oracle, ctx, cols, users, seed):
        self.oracle, self.ctx, self.users, self.t0 = oracle, ctx, users, oracle.T0_MS
        ctx.load_columns(*cols, users)
        self.model = SessionTurnModel(*cols)
        self.keys = random_keys(seed, cols[0].shape[0])
        ctx.token_set(self.keys)
        self.model.token_set(self.keys)
        self.top = int(cols[0].max()) + 1          # a clock at or after every start of the table

    def queries(self):
        t0 = self.t0
        return [(t0 - 6 * HOUR, t0 - 61 * DAY, 0x55555555), (t0 - 100 * DAY, t0 - 130 * DAY, ALL), (self.top + HOUR, t0 - 10 * DAY, 0xAAAAAAAA)]

    def check(self, tag, queries=None, on_run=True):
        m = self.model
        for q, (now, cutoff, mask) in enumerate(queries or self.queries()):
            self.ctx.set_disciplines(mask, DISCS)
            got = self.ctx.scan(now, cutoff)
            for x, y in zip(got, self.oracle.scan(m.start, m.end, m.user, m.disc, self.users, now, cutoff, mask)):
                assert np.array_equal(x, y), (tag, q)
            if on_run:
                assert self.ctx.stats()["k1_variant"] & 0x2000, (tag, q, "the scan did not take the ordered run")

    def info(self):
        ti = self.ctx.table_info()
        return int(ti["ordered_rows"]), int(ti["ordered_builds"]), int(ti["ordered_respreads"])

    def turn(self, ops, user, disc, tag="", n_users=None):
        return run_turn(self.ctx, self.model, ops, user, disc, n_users or self.users, tag)


@contextlib.contextmanager
def bed(pie, oracle, seed, switch=1, cols=None, users=USERS, mode=2, build=True, room=ROOM):
    """room: rows of capacity beyond the table's own (a load fits the columns exactly, and a turn that has to grow them drops the run
    whatever the switch says): the context loads a larger table first and keeps its capacity"""
    cols = oracle.gen(0x5EED5EED + seed, N, 0, N, USERS, DISCS, 0) if cols is None else cols
    with pie.PieScan(0) as ctx:
        ctx.set_ordered_run(mode)
        ctx.set_turn_ordered(switch)
        if room:
            z = np.zeros(N + room, np.int64)
            ctx.load_columns(z, z, z.astype(np.int32), z.astype(np.int32), users)
        b = Bed(oracle, ctx, cols, users, seed + 1000)
        if build:
            b.check("built")
            assert b.info()[0] == cols[0].shape[0], "the run holds every row of the table"
        yield b


@contextlib.contextmanager
def twin_of(pie, b):
    """a second context on the same table, for the one-by-one sequence"""
    with pie.PieScan(0) as t:
        t.set_ordered_run(2)
        m = b.model
        t.load_columns(m.start.copy(), m.end.copy(), m.user.copy(), m.disc.copy(), b.users)
        t.token_set(b.keys)
        yield t


def same_as_twin(b, twin, got, want, ops, tag):
    found = want["row"] >= 0
    for col in ("row", "live", "end"):
        assert np.array_equal(got[col], want[col]), (tag, col)
    for col in ("user", "start"):
        assert np.array_equal(got[col][found | (ops["kind"] == CREATE)], want[col][found | (ops["kind"] == CREATE)]), (tag, col)
    for name, x, y in zip(("start", "end", "user", "disc"), b.ctx.read_columns(), twin.read_columns()):
        assert np.array_equal(x, y), (tag, name)
    for now, cutoff, mask in b.queries():
        for c in (b.ctx, twin):
            c.set_disciplines(mask, DISCS)
        for x, y in zip(b.ctx.scan(now, cutoff), twin.scan(now, cutoff)):
            assert np.array_equal(x, y), (tag, "scan of the twin")


def logins(b, rng, k, users=None):
    """k creates in time order, at or after every start of the table"""
    new = random_keys(int(rng.integers(1 << 30)), k)
    ops = make_ops(new, b.top + np.arange(k), CREATE, b.t0 + rng.integers(-HOUR, 12 * HOUR, k))
    user = rng.integers(0, b.users, k) if users is None else np.asarray(users)
    return new, ops, user.astype(np.int32), rng.integers(0, DISCS, k).astype(np.int32)


def in_order_turn(b, rng):
    new, ops, user, disc = logins(b, rng, 100)
    old = np.nonzero(b.model.end > b.t0 - 6 * HOUR)[0][:20]
    ops = np.concatenate([ops, make_ops(b.keys[old], b.t0, DELETE)])
    return new, ops, np.concatenate([user, np.zeros(20, np.int32)]), np.concatenate([disc, np.zeros(20, np.int32)])


def test_in_order_logins_keep_the_run(pie, oracle):
    """the test that fails without the feature: 100 creates behind every start of their users and 20 deletes of old keys"""
    with bed(pie, oracle, 10) as b, twin_of(pie, b) as twin:
        held, builds, respreads = b.info()
        new, ops, user, disc = in_order_turn(b, np.random.default_rng(1))
        got = b.turn(ops, user, disc, "in order")
        want = one_by_one(twin, ops, user, disc, USERS)
        assert b.ctx.n == N + 100 and b.info() == (N + 100, builds, respreads), "the run holds every row; nothing was rebuilt or moved"
        b.check("behind the turn")
        assert b.info() == (N + 100, builds, respreads), "the scans ran on the run the turn kept"
        same_as_twin(b, twin, got, want, ops, "in order")
        state_matches(b.ctx, b.model, np.concatenate([b.keys[:500], new]))
    with bed(pie, oracle, 10, switch=0) as b:
        new, ops, user, disc = in_order_turn(b, np.random.default_rng(1))
        b.turn(ops, user, disc, "switch off")
        assert b.info()[0] == 0, "with the switch off a turn with creates drops the run"
        b.check("switch off")
        state_matches(b.ctx, b.model, new)


def test_ops_on_rows_the_turn_created(pie, oracle):
    with bed(pie, oracle, 11) as b, twin_of(pie, b) as twin:
        held, builds, _ = b.info()
        T = b.top
        ka, kb, kc, kd = random_keys(77, 4)
        one = lambda key, now, kind, new_end=0: make_ops(np.asarray(key, np.uint64).reshape(1, 2), now, kind, new_end)
        ops = np.concatenate([
            one(ka, T, CREATE, T + HOUR), one(ka, T + 1, TOUCH, T + 10 * DAY),             # A lives on by its touched `end` alone
            one(kb, T + 2, CREATE, T + 30 * DAY), one(kb, T + 3, DELETE),                  # B is gone
            one(kc, T + 4, CREATE, T + 2 * HOUR), one(kc, T + 5, GET),
            one(kd, T + 6, CREATE, T + 3 * HOUR), one(kd, T + 7, TOUCH, T + 20 * DAY),     # the first row of the doubled key: touched
            one(kd, T + 8, CREATE, T + 5 * HOUR),                                          # ... and the second keeps its own `end`
            one(b.keys[5], T, GET)])
        user = np.asarray([3, 3, 4, 4, 5, 5, 6, 6, 6, 0], np.int32)
        disc = np.asarray([1, 0, 2, 0, 3, 0, 4, 0, 5, 0], np.int32)
        got = b.turn(ops, user, disc, "created rows")
        want = one_by_one(twin, ops, user, disc, USERS)
        assert got["row"][:9].tolist() == [N, N, N + 1, N + 1, N + 2, N + 2, N + 3, N + 3, N + 4]
        m = b.model
        assert m.end[N:].tolist() == [T + 10 * DAY, END_NONE, T + 2 * HOUR, T + 20 * DAY, T + 5 * HOUR]
        assert b.info()[:2] == (N + 5, builds)
        late = [(T + 2 * DAY, T - DAY, ALL), (T + 30 * 60 * 1000, T - DAY, ALL), (T + 4 * HOUR, T - DAY, ALL), (T + 2 * DAY, b.t0 - 130 * DAY, ALL)]
        b.check("created rows", late)
        ctx = b.ctx
        ctx.set_disciplines(ALL, DISCS)
        assert sorted(ctx.scan(T + 2 * DAY, T - DAY)[2].tolist()) == [N, N + 3], "A by its touched end, the doubled key's first row, not B"
        b.check("created rows, the usual queries")
        assert b.info()[:2] == (N + 5, builds)
        same_as_twin(b, twin, got, want, ops, "created rows")
        state_matches(ctx, m, np.stack([ka, kb, kc, kd]))


def test_several_creates_per_user_in_one_turn(pie, oracle):
    """chains of 2, 3 and 4 rows of one user (sorted in registers), of 5 and 9 (read off the batch), singles between them; the starts
    descend in array order, so every chain has to be sorted into place"""
    with bed(pie, oracle, 12) as b, twin_of(pie, b) as twin:
        _, builds, _ = b.info()
        rng = np.random.default_rng(3)
        users = np.concatenate([np.full(c, u) for u, c in ((11, 2), (12, 3), (13, 4), (14, 5), (15, 9))] + [np.arange(100, 112)])
        users = users[rng.permutation(users.shape[0])]
        k = users.shape[0]
        new = random_keys(78, k)
        ops = make_ops(new, b.top + 10 * (k - np.arange(k)), CREATE, b.t0 + rng.integers(-HOUR, 12 * HOUR, k))
        disc = rng.integers(0, DISCS, k).astype(np.int32)
        got = b.turn(ops, users.astype(np.int32), disc, "chains")
        want = one_by_one(twin, ops, users.astype(np.int32), disc, USERS)
        assert b.info()[:2] == (N + k, builds), "the run took every row, through a re-spread where a segment was full"
        b.check("chains")
        assert b.info()[:2] == (N + k, builds)
        same_as_twin(b, twin, got, want, ops, "chains")
        state_matches(b.ctx, b.model, new)


def test_a_full_segment(pie, oracle):
    """25 creates for one user of about 40 rows: more than its spare slots (rows / 16 + 16 or + 4) under either rule"""
    with bed(pie, oracle, 13) as b:
        _, builds, respreads = b.info()
        rng = np.random.default_rng(4)
        issued = []
        for turn in range(2):
            new, ops, user, disc = logins(b, rng, 25, np.full(25, 42))
            ops["now"] += 100 * turn
            extra = make_ops(b.keys[rng.integers(0, N, 10)], b.t0 - 200 * DAY, TOUCH, b.t0 + DAY)
            b.turn(np.concatenate([ops, extra]), np.concatenate([user, np.zeros(10, np.int32)]), np.concatenate([disc, np.zeros(10, np.int32)]),
                   "full segment %d" % turn)
            issued.append(new)
            rows = N + 25 * (turn + 1)
            assert b.info() == (rows, builds, respreads + turn + 1), "one re-spread, the run valid with every row"
            b.check("full segment %d" % turn)
            assert b.info() == (rows, builds, respreads + turn + 1)
        state_matches(b.ctx, b.model, np.concatenate(issued))


def test_a_far_back_fill_drops_the_run_and_nothing_else(pie, oracle):
    cols = [c.copy() for c in oracle.gen(0x5EED5EED + 14, N, 0, N, USERS, DISCS, 0)]
    rng = np.random.default_rng(5)
    cols[2][rng.choice(N, 600, replace=False)] = 7        # user 7 has at least 600 rows: far beyond the 256 a late row may shift
    with bed(pie, oracle, 14, cols=cols) as b:
        _, builds, _ = b.info()
        early = int(cols[0][cols[2] == 7].min()) - DAY
        new = random_keys(79, 3)
        ops = np.concatenate([make_ops(new[:2], b.top, CREATE, b.t0 + DAY), make_ops(new[2:], early, CREATE, b.t0 + DAY)])
        b.turn(ops, np.asarray([1, 2, 7], np.int32), np.asarray([0, 1, 2], np.int32), "back-fill")
        assert b.info()[0] == 0, "the run is dropped"
        state_matches(b.ctx, b.model, new)
        b.check("back-fill", b.queries() + [(b.t0 - 100 * DAY, early - DAY, ALL)])
        assert b.info()[:2] == (N + 3, builds + 1), "mode 2 rebuilt it with the new rows"


def test_fallbacks(pie, oracle):
    rng = np.random.default_rng(6)
    # more creates than an append may bring (the table has room: the context loaded a larger one first)
    with bed(pie, oracle, 16) as b:
        ctx = b.ctx
        new, ops, user, disc = logins(b, rng, 4097)
        b.turn(ops, user, disc, "4 097 creates")
        assert b.info()[0] == 0 and ctx.n == N + 4097
        b.check("4 097 creates")
        state_matches(ctx, b.model, new[::16])
        # ... and the rebuilt run takes the next turn
        new, ops, user, disc = logins(b, rng, 1)
        assert b.info()[0] == N + 4097
        b.turn(ops, user, disc, "one more")
        assert b.info()[0] == N + 4098
        b.check("one more")
    # a user beyond the ones the run has segments for; a table that has to grow; a run that is not valid
    with bed(pie, oracle, 17) as b:
        new, ops, user, disc = logins(b, rng, 5, [USERS, 1, 2, 3, USERS + 2])
        b.users = USERS + 3
        b.turn(ops, user, disc, "new users")
        # the run has a segment for every user the table has room for (ord.users is the user capacity at its build), so a user
        # beyond it also outgrows the user arrays: this case coincides with growth, and either way the run is gone before the launch
        assert b.info()[0] == 0, "the run went"
        b.check("new users")
        assert b.info()[0] == N + 5, "rebuilt with segments for the new users"
        state_matches(b.ctx, b.model, new)
    with bed(pie, oracle, 18, room=0) as b:
        cap = b.ctx.table_info()["table_bytes"] // 24
        new, ops, user, disc = logins(b, rng, int(cap - N) + 7)
        b.turn(ops, user, disc, "growth")
        assert b.ctx.table_info()["table_bytes"] // 24 > cap and b.info()[0] == 0, "columns that move drop the run, as an append's do"
        b.check("growth")
        state_matches(b.ctx, b.model, new)
    with bed(pie, oracle, 19, build=False) as b:
        assert b.info()[0] == 0
        new, ops, user, disc = logins(b, rng, 50)
        b.turn(ops, user, disc, "no run")
        assert b.info()[0] == 0
        b.check("no run")
        state_matches(b.ctx, b.model, new)


def test_the_switch(pie, oracle, gpu_ctx):
    ctx = gpu_ctx
    ctx.set_ordered_run(1)
    rng = np.random.default_rng(7)
    n = 600
    start = (oracle.T0_MS - rng.integers(1, 10 ** 9, n)).astype(np.int64)
    ctx.load_columns(start, start + 10 ** 10, rng.integers(0, 64, n).astype(np.int32), rng.integers(0, 8, n).astype(np.int32), 64)
    keys = random_keys(80, n)
    ctx.token_set(keys)
    for bad in (2, -1, 7):
        with pytest.raises(pie.PieError) as ei:
            ctx.set_turn_ordered(bad)
        assert ei.value.code == PIE_E_INVAL
    assert ctx._lib.pie_set_turn_ordered(None, 1) == PIE_E_INVAL
    ctx.set_disciplines(0xFF, 8)
    ctx.scan_batch_begin([(oracle.T0_MS, 0, 0xFF), (oracle.T0_MS - HOUR, 0, 1)])
    with pytest.raises(pie.PieError) as ei:
        ctx.set_turn_ordered(1)
    assert ei.value.code == PIE_E_STATE, "a batch in flight"
    ctx.scan_batch_finish()
    ctx.token_turn_begin(make_ops(keys[:3], oracle.T0_MS, GET))
    with pytest.raises(pie.PieError) as ei:
        ctx.set_turn_ordered(1)
    assert ei.value.code == PIE_E_STATE, "a turn begun and not finished"
    ctx.token_turn_finish()
    ctx.set_turn_ordered(1)
    ctx.set_turn_ordered(0)


ENV_CHILD = """
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import oracle_py, sph_pie_amd
from turn_model import make_ops
cols = oracle_py.gen(0x5EED5EED + 20, 20000, 0, 20000, 499, 32, 0)
with sph_pie_amd.PieScan(0) as ctx:
    ctx.set_ordered_run(2)
    z = np.zeros(26000, np.int64)
    ctx.load_columns(z, z, z.astype(np.int32), z.astype(np.int32), 499)   # room: a turn that grows the columns drops the run
    ctx.load_columns(*cols, 499)
    ctx.token_set(np.random.default_rng(1).integers(0, 2 ** 64, (20000, 2), dtype=np.uint64))
    ctx.set_disciplines(0x55555555, 32)
    ctx.scan(oracle_py.T0_MS, 0)
    new = np.random.default_rng(2).integers(0, 2 ** 64, (10, 2), dtype=np.uint64)
    ops = make_ops(new, int(cols[0].max()) + 1 + np.arange(10), 3, oracle_py.T0_MS + 10 ** 7)
    ctx.session_turn(ops, np.arange(10, dtype=np.int32), np.zeros(10, np.int32), 499)
    print("ordered_rows", ctx.table_info()["ordered_rows"])
"""


@pytest.mark.parametrize("env,rows", [("1", N + 10), ("0", 0), (None, 0)])
def test_the_env_default(pie, oracle, env, rows):
    child_env = {k: v for k, v in os.environ.items() if k != "PIE_TURN_ORDERED"}
    if env is not None:
        child_env["PIE_TURN_ORDERED"] = env
    code = ENV_CHILD % (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests"))
    res = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=child_env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ordered_rows %d\n" % rows in res.stdout, res.stdout


def chain_plan(seed, n_turns=30):
    """the seeded chain's script, drawn on the CPU: per turn the mix of ops and what runs between the turns.  Creates are stamped
    with the chain's clock, which only moves forward, so nearly all of them arrive in time order; one in twelve is a little late."""
    rng = np.random.default_rng(seed)
    plan = []
    for t in range(n_turns):
        plan.append({"creates": int(rng.integers(1, 40)), "others": int(rng.integers(0, 60)), "late": rng.random() < 1 / 12,
                     "between": str(rng.choice(["set_end", "delete_user", "append_rows", "scan", "none"])), "seed": int(rng.integers(1 << 30))})
    return plan


def test_a_seeded_chain(pie, oracle):
    with bed(pie, oracle, 21) as b:
        ctx, m = b.ctx, b.model
        known = b.keys
        clock = b.top
        kept_behind_a_create_turn = 0
        for t, step in enumerate(chain_plan(2024)):
            rng = np.random.default_rng(step["seed"])
            kc, ko = step["creates"], step["others"]
            new = random_keys(step["seed"], kc)
            at = clock + np.sort(rng.integers(0, 1000, kc))
            if step["late"]:
                at[-1] = clock - 5 * 60 * 1000                  # a front-end whose clock runs behind: a few places back, far from 256
            creates = make_ops(new, at, CREATE, at + rng.integers(-HOUR, 30 * DAY, kc))
            others = make_ops(known[rng.integers(0, known.shape[0], ko)], clock + rng.integers(-DAY, DAY, ko),
                              rng.choice([GET, TOUCH, DELETE], ko, p=[0.8, 0.15, 0.05]))
            others["new_end"] = np.where(others["kind"] == TOUCH, clock + rng.integers(0, 30 * DAY, ko), 0)
            if ko and kc > 1:
                others["tok"][0] = new[0]                      # an op on a key the same turn creates (before or behind its create)
            ops = np.concatenate([creates, others])[rng.permutation(kc + ko)]
            user = rng.integers(0, USERS, kc + ko).astype(np.int32)
            disc = rng.integers(0, DISCS, kc + ko).astype(np.int32)
            was_valid = b.info()[0] > 0
            b.turn(ops, user, disc, "turn %d" % t)
            kept_behind_a_create_turn += int(was_valid and b.info()[0] == ctx.n)
            known = np.concatenate([known, new])
            clock += 1000
            b.check("turn %d" % t, [(clock - rng.integers(0, 40 * DAY), b.t0 - 130 * DAY, ALL), (b.t0 - 6 * HOUR, b.t0 - 61 * DAY, 0x55555555)])
            state_matches(ctx, m, known[rng.integers(0, known.shape[0], 300)])
            how = step["between"]
            if how == "set_end":
                rows = rng.choice(ctx.n, 50, replace=False).astype(np.int32)
                rows = rows[m.end[rows] != END_NONE]
                ends = clock + rng.integers(-DAY, 30 * DAY, rows.shape[0])
                ctx.set_end(rows, ends)
                m.end[rows] = ends
            elif how == "delete_user":
                u = int(rng.integers(0, USERS))
                assert np.array_equal(np.sort(ctx.delete_user(u)), m.delete_user(u))
            elif how == "append_rows":
                k = int(rng.integers(1, 30))
                cols = (clock + np.arange(k), clock + rng.integers(0, 30 * DAY, k), rng.integers(0, USERS, k).astype(np.int32),
                        rng.integers(0, DISCS, k).astype(np.int32))
                more = random_keys(step["seed"] + 1, k)
                ctx.append_rows(*cols, USERS)
                ctx.token_append(more)
                m.append_rows(*cols)
                m.token_append(more)
                known = np.concatenate([known, more])
                clock += 1000
            elif how == "scan":
                b.check("between %d" % t)
        assert kept_behind_a_create_turn >= 1, "no create turn of the chain kept the run"
        b.check("the end of the chain")
        state_matches(ctx, m, known)
