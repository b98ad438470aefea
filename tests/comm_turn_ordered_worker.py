"""Turns that log in keep the ordered run on sharded tables (pie_set_turn_ordered on every shard's context, pie_comm_session_turn),
in a fresh process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): WORLD shards of one table of 20 000 rows, 499 users and 32
disciplines on GPU 0, every shard in mode 2 with its run built by one scan.  A twin communicator makes the same calls one by one
(pie_comm_append_rows of one row, pie_comm_token_append, pie_comm_token_turn of one op); the oracle runs on each shard's own rows.
usage: comm_turn_ordered_worker.py WORLD
  1. a first turn outgrows the shards' columns (a sharded table fits them exactly): the run goes, as behind an append that grows
  2. a turn with creates and deletes: every shard that keeps a create has ordered_rows == its local rows, no rebuild; scans and a
     batch per shard exact; the twin matches per rank
  3. a turn that brings a new user, which one shard owns
  4. a full segment on one shard only: that shard re-spreads, the others do not
  5. the switch off on every shard: a kept create drops the run (today's rule)"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
WORLD = int(sys.argv[1])
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_turn_ordered_%d.so" % os.getpid())
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub
os.environ.pop("PIE_TURN_ORDERED", None)

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from session_turn_model import CREATE
from turn_model import DELETE, make_ops

N, USERS, DISCS = 20_000, 499, 32
HOUR, DAY = 3600 * 1000, 86400 * 1000
T0 = oracle_py.T0_MS
ALL = (1 << DISCS) - 1
COLS = ("row", "live", "user", "start", "end")


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def owners(users):
    return np.array([pie.shard_of(int(u), WORLD) for u in range(users)], np.int32)


def sharded(cols, keys, switch, mode=2):
    comm = pie.PieComm([0] * WORLD)
    ctxs = [comm.ctx(r) for r in range(WORLD)]
    for r, c in enumerate(ctxs):
        c.set_ordered_run(mode)
        c.set_turn_ordered(switch)
        c.load_columns(*cols, USERS)
        c.shard_table(r, WORLD)
    comm.token_set(keys)
    return comm, ctxs


def local(c):
    ti = c.table_info()
    c.n, c.n_users = int(ti["rows"]), int(ti["users"])
    return c.read_columns()


def info(c):
    ti = c.table_info()
    return int(ti["ordered_rows"]), int(ti["ordered_builds"]), int(ti["ordered_respreads"])


def shard_exact(c, top, tag, on_run=True):
    """a sparse, a dense and a late scan and one batch of the three against the oracle on the shard's own rows"""
    s, e, u, d = local(c)
    qs = [(T0 - 6 * HOUR, T0 - 61 * DAY, 0x55555555), (T0 - 100 * DAY, T0 - 130 * DAY, ALL), (top + HOUR, T0 - 10 * DAY, 0xAAAAAAAA)]
    for q, (now, cutoff, mask) in enumerate(qs):
        c.set_disciplines(mask, DISCS)
        for x, y in zip(c.scan(now, cutoff), oracle_py.scan(s, e, u, d, c.n_users, now, cutoff, mask)):
            assert np.array_equal(x, y), (tag, "scan", q)
        assert not on_run or c.stats()["k1_variant"] & 0x2000, (tag, q, "the scan did not take the ordered run")
    c.set_disciplines(ALL, DISCS)
    for q, res in enumerate(c.scan_batch(qs)):
        for x, y in zip(res, oracle_py.scan(s, e, u, d, c.n_users, *qs[q])):
            assert np.array_equal(x, y), (tag, "batch", q)


def one_by_one(comm, ops, user, disc, users):
    k = ops.shape[0]
    out = {col: [] for col in COLS}
    for i in range(k):
        op = ops[i:i + 1]
        if int(op["kind"][0]) == CREATE:
            first = comm.append_rows(op["now"], op["new_end"], user[i:i + 1], disc[i:i + 1], users)
            comm.token_append(op["tok"])
            got = {"row": [first], "live": [op["new_end"][0] > op["now"][0]], "user": [user[i]], "start": op["now"], "end": op["new_end"]}
        else:
            got = comm.token_turn(op)
        for col in COLS:
            out[col].append(got[col][0])
    return {col: np.asarray(v) for col, v in out.items()}


def twin_turn(comm_a, a, comm_b, b, ops, user, disc, users, tag):
    got, want = comm_a.session_turn(ops, user, disc, users), one_by_one(comm_b, ops, user, disc, users)
    f = want["row"] >= 0
    for col in ("row", "live"):
        assert np.array_equal(got[col], want[col]), (tag, col)
    for col in ("end", "user", "start"):
        assert np.array_equal(got[col][f], want[col][f]), (tag, col)
    for r in range(WORLD):
        for name, x, y in zip(("start", "end", "user", "disc"), local(a[r]), local(b[r])):
            assert np.array_equal(x, y), (tag, r, name)
        for x, y in zip(a[r].shard_maps(), b[r].shard_maps()):
            assert np.array_equal(x, y), (tag, r, "maps")
    return got


def main():
    cols = oracle_py.gen(0x5EED5EED + 30, N, 0, N, USERS, DISCS, 0)
    keys = random_keys(131, N)
    owner = owners(USERS + 1)
    top = int(cols[0].max()) + 1
    rng = np.random.default_rng(132 + WORLD)
    comm_a, a = sharded(cols, keys, 1)
    comm_b, b = sharded(cols, keys, 0)
    for r in range(WORLD):
        shard_exact(a[r], top, ("built", r))
        assert info(a[r])[0] == a[r].n > 0

    def logins(k, users, at):
        new = random_keys(int(rng.integers(1 << 30)), k)
        return new, make_ops(new, at + np.arange(k), CREATE, T0 + rng.integers(-HOUR, 12 * HOUR, k)), np.asarray(users, np.int32), \
            rng.integers(0, DISCS, k).astype(np.int32)

    # 1. the columns of a sharded table have no spare row: the first logins grow them on every shard that keeps one, and columns
    #    that move take the run with them
    new, ops, user, disc = logins(WORLD * 8, np.arange(WORLD * 8) % USERS, top)
    twin_turn(comm_a, a, comm_b, b, ops, user, disc, USERS, "growth")
    for r in range(WORLD):
        shard_exact(a[r], top, ("growth", r))
        assert info(a[r])[0] == a[r].n
    top += 1000
    # 2. logins in time order and deletes of old keys, through the communicator
    before = [info(c) for c in a]
    rows_before = [c.n for c in a]
    new, ops, user, disc = logins(100, rng.integers(0, USERS, 100), top)
    old = np.nonzero(cols[1] > T0 - 6 * HOUR)[0][:20]
    ops = np.concatenate([ops, make_ops(keys[old], T0, DELETE)])
    user, disc = np.concatenate([user, np.zeros(20, np.int32)]), np.concatenate([disc, np.zeros(20, np.int32)])
    got = twin_turn(comm_a, a, comm_b, b, ops, user, disc, USERS, "in order")
    assert np.array_equal(got["owner"][:100], owner[user[:100]])
    for r in range(WORLD):
        kept = int(np.count_nonzero(owner[user[:100]] == r))
        assert kept > 0, "100 creates reach every shard of at most five"
        assert a[r].n == rows_before[r] + kept and info(a[r]) == (a[r].n, before[r][1], before[r][2]), ("in order", r, info(a[r]))
        shard_exact(a[r], top, ("in order", r))
        assert info(a[r]) == (a[r].n, before[r][1], before[r][2]), "the scans and the batch ran on the run the turn kept"
    top += 1000
    # 3. a new user, one shard's, logs in three times (that shard's run stays only if it has a segment for the user: exactness is
    #    what is asked of it); the other shards keep no create and gain no user, and are untouched
    before = [info(c) for c in a]
    new, ops, user, disc = logins(3, np.full(3, USERS), top)
    twin_turn(comm_a, a, comm_b, b, ops, user, disc, USERS + 1, "new users")
    for r in range(WORLD):
        shard_exact(a[r], top, ("new users", r))
        if r != owner[USERS]:
            assert info(a[r]) == before[r], ("new users", r, "a shard that keeps no create is untouched")
    top += 1000
    # 4. a full segment on one shard only
    before = [info(c) for c in a]
    new, ops, user, disc = logins(25, np.full(25, 42), top)
    twin_turn(comm_a, a, comm_b, b, ops, user, disc, USERS + 1, "full segment")
    for r in range(WORLD):
        moved = 1 if r == owner[42] else 0      # the rows the deletes of step 2 tombstoned are not held by a run built since
        assert info(a[r]) == (before[r][0] + 25 * moved, before[r][1], before[r][2] + moved), ("full segment", r, info(a[r]), before[r])
        shard_exact(a[r], top, ("full segment", r))
    comm_a.close()
    comm_b.close()
    # 5. the switch off: today's rule
    comm, c = sharded(cols, keys, 0)
    for r in range(WORLD):
        shard_exact(c[r], top, ("off, built", r))
    new, ops, user, disc = logins(WORLD * 8, np.arange(WORLD * 8) % USERS, top)
    comm.session_turn(ops, user, disc, USERS)
    for r in range(WORLD):
        shard_exact(c[r], top, ("off, grown", r))
        assert info(c[r])[0] == c[r].n
    new, ops, user, disc = logins(60, rng.integers(0, USERS, 60), top + 1000)
    comm.session_turn(ops, user, disc, USERS)
    for r in range(WORLD):
        assert np.any(owner[user] == r) and info(c[r])[0] == 0, "with the switch off a kept create drops the shard's run"
        shard_exact(c[r], top, ("off", r))
    comm.close()
    print("turn_ordered ok: world %d" % WORLD)


main()
