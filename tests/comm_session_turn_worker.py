"""A turn that logs in on sharded tables (pie_shard_session_turn on every shard, pie_comm_session_turn behind the communicator), in
a fresh process whose "RCCL" is tests/stub_rccl.c (PIE_RCCL_LIB): several shards of one table on GPU 0.  The model is
tests/shard_chain.py's ShardStoreModel / ShardModelStore: a login is pie_shard_append_rows of one row and pie_shard_token_append of
its key, every other op a pie_shard_token_turn of one op, merged by the largest global row.
usage: comm_session_turn_worker.py CASE [WORLD]
  g5      the recorded trace G5 through PieComm.session_turn on an empty table, in turns of 1, 7, 64 and whole runs: every recorded
          answer and census, and the model's answers op for op
  twin    seeded mixed turns (k = 1, 64, 257, 300, 640): one set of contexts driven by shard_session_turn, a second by the
          one-by-one sequence; after every turn, per rank: answers, columns, both maps, the token layout, lookups of every key, a
          scan and a batch against the oracle
  shapes  one create kept and not kept; 300 creates whose owners interleave; 257 ops whose one create is the last; the first row and
          the first user of an empty shard; new users arriving in the turn that logs them in; one designed two-shard key
  room    slots doubling on one rank only; column capacity outgrown; users outgrown; a turn after a compaction dropped rows on one
          rank
  wrap    probe runs that wrap the slot table, and slots claimed in the same launch, on one shard
  derived the hot index live, a turn with creates, then a batch exact against the oracle on every shard; the ordered run valid,
          kept by a create-free turn, dropped by a kept create
  errors  every refusal leaves every shard as it was: columns, maps, layout, N_g, covered_g"""
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
CASE = sys.argv[1]
WORLD = int(sys.argv[2]) if len(sys.argv) > 2 else 3
stub_dir = os.path.join(REPO, "tests", "_stub")
os.makedirs(stub_dir, exist_ok=True)
stub = os.path.join(stub_dir, "libstub_rccl_session_turn_%d.so" % os.getpid())
subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                "-L/opt/rocm/lib", "-lamdhip64"], check=True)
os.environ["PIE_RCCL_LIB"] = stub

import numpy as np
import torch  # noqa: F401  (before libpie_hip.so initialises HIP)
import oracle_py
import sph_pie_amd as pie
from sph_pie_amd.binding import PieError
from session_turn_model import CREATE, replay_g5_sessions
from shard_chain import ShardModelStore
from shard_token_model import merge
from token_model import END_NONE, check_layout
from trace_replay import load_trace
from turn_model import DELETE, GET, TOUCH, TURN_OP, g5_key, make_ops

NOW, HOUR, DAY, D = 1700000000000, 3600 * 1000, 86400 * 1000, 8
PIE_E_INVAL, PIE_E_STATE = -1, -6
GOLDEN = os.path.join(REPO, "tests", "golden")
COLS = ("row", "live", "user", "start", "end")


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def columns(seed, n, users):
    rng = np.random.default_rng(seed)
    start = NOW - rng.integers(1, 10 ** 9, n)
    end = NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, n)
    return start.astype(np.int64), end.astype(np.int64), rng.integers(0, users, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def owners(users, world):
    return np.array([pie.shard_of(int(u), world) for u in range(users)], np.int32)


def sharded(world, cols, users, keys=None, hot=False):
    """a communicator whose `world` local shards hold the table `cols` of `users` users, with a key per row -> (comm, contexts)"""
    os.environ["PIE_HOT_INDEX"] = "1" if hot else "0"        # read when the communicator creates its contexts
    comm = pie.PieComm([0] * world)
    ctxs = [comm.ctx(r) for r in range(world)]
    for r, c in enumerate(ctxs):
        c.load_columns(*cols, users)
        c.shard_table(r, world)
        c.set_disciplines((1 << D) - 1, D)
    comm.token_set(np.zeros((0, 2), np.uint64) if keys is None else keys)
    return comm, ctxs


def snapshot(c):
    """everything a refused call must leave alone, and everything the twin compares per rank"""
    ti = c.table_info()
    c.n, c.n_users = int(ti["rows"]), int(ti["users"])
    info = c.shard_info()
    rows_g, users_g = c.shard_maps()
    cg, cl, slots, slot_row, keys = c.shard_token_layout()
    return {"cols": [a.copy() for a in c.read_columns()], "rows_g": rows_g.copy(), "users_g": users_g.copy(), "N_g": info["rows_global"],
            "U_g": info["users_global"], "covered_g": cg, "covered_l": cl, "slots": slots, "slot_row": slot_row, "keys": keys}


def same_snapshot(a, b, tag, slots_exact=True):
    for x, y, name in zip(a["cols"], b["cols"], ("start", "end", "user", "disc")):
        assert np.array_equal(x, y), (tag, name)
    for name in ("rows_g", "users_g", "keys"):
        assert np.array_equal(a[name], b[name]), (tag, name)
    for name in ("N_g", "U_g", "covered_g", "covered_l", "slots"):
        assert a[name] == b[name], (tag, name, a[name], b[name])
    if slots_exact:
        assert np.array_equal(a["slot_row"], b["slot_row"]), (tag, "slot_row")
    else:   # the lanes of one launch claim in any order: the same rows in the same table, each reachable from its home
        assert np.array_equal(np.sort(a["slot_row"]), np.sort(b["slot_row"])), (tag, "slot_row")


def sound(c, snap):
    check_layout(snap["covered_l"], snap["slots"], snap["slot_row"], snap["keys"], pie.token_homes(snap["keys"], int(snap["slots"]).bit_length() - 1))


def one_by_one(c, ops, user, disc, users):
    """the sequence the header defines the turn by, on one shard"""
    k = ops.shape[0]
    out = {"row": np.full(k, -1, np.int32), "live": np.zeros(k, np.uint8), "user": np.full(k, -1, np.int32), "start": np.zeros(k, np.int64),
           "end": np.full(k, END_NONE, np.int64)}
    for i in range(k):
        op = ops[i:i + 1]
        if int(op["kind"][0]) == CREATE:
            first, kept = c.shard_append_rows(op["now"], op["new_end"], user[i:i + 1], disc[i:i + 1], users)
            c.shard_token_append(op["tok"])
            if kept:
                out["row"][i], out["live"][i], out["user"][i] = first, op["new_end"][0] > op["now"][0], user[i]
                out["start"][i], out["end"][i] = op["now"][0], op["new_end"][0]
        else:
            got = c.shard_token_turn(op)
            for col in COLS:
                out[col][i] = got[col][0]
    return out


def same_answers(got, want, ops, tag):
    """row and live of every op; end, user and start where the op answers for a row (a delete that wrote nothing answers -1, and
    tests/shard_token_model.merge leaves end = 0 where no shard holds the key: the ABI's answer there is PIE_END_NONE)"""
    f = want["row"] >= 0
    for col in ("row", "live"):
        assert np.array_equal(got[col], want[col]), (tag, col, np.nonzero(got[col] != want[col])[0][:8])
    for col in ("end", "user", "start"):
        assert np.array_equal(got[col][f], want[col][f]), (tag, col)
    assert np.all(got["end"][~f] == END_NONE), (tag, "an op that answers for no row answers end = PIE_END_NONE")


def scans_match(c, snap, tag):
    s, e, u, d = snap["cols"]
    qs = [(NOW - 977 * q * HOUR // 100 + (q % 5 - 2) * 10 ** 8, NOW - (11 + q % 4) * DAY, (0x55, 0xAA, 0xFF)[q % 3]) for q in range(5)]
    c.set_disciplines(qs[0][2], D)
    for x, y in zip(c.scan(qs[0][0], qs[0][1]), oracle_py.scan(s, e, u, d, c.n_users, *qs[0])):
        assert np.array_equal(x, y), (tag, "scan")
    c.set_disciplines(0xFF, D)
    for q, res in enumerate(c.scan_batch(qs)):
        for x, y in zip(res, oracle_py.scan(s, e, u, d, c.n_users, *qs[q])):
            assert np.array_equal(x, y), (tag, "batch", q)


# ------------------------------------------------------------------------------------------------ (a) the recorded trace
class DeviceShardStore:
    """what replay_g5_sessions drives: PieComm.session_turn with ShardModelStore beside it, every turn compared"""

    def __init__(self, world, n_users):
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        self.comm, self.ctxs = sharded(world, (z64, z64, z32, z32), n_users)
        self.model, self.U, self.world = ShardModelStore(oracle_py, n_users, world), n_users, world
        self.owner = owners(n_users, world)

    def turn(self, ops, user, disc):
        got, want = self.comm.session_turn(ops, user, disc, self.U), self.model.turn(ops, user, disc)
        same_answers(got, want, ops, "g5")
        f = want["row"] >= 0
        assert np.array_equal(got["owner"][f], self.owner[want["user"][f]]) and np.all(got["owner"][~f] == -1)
        return got

    def delete_user(self, u):
        rows, owner = self.comm.delete_user(u)
        tm = self.model.sm.tm
        assert np.array_equal(np.sort(rows), np.nonzero((tm.user == u) & (tm.end != END_NONE))[0])
        self.model.delete_user(u)

    def purge(self, now):
        tm = self.model.sm.tm
        rows = np.sort(self.comm.expired_queue(END_NONE, now)) if tm.start.shape[0] else np.zeros(0, np.int32)
        if rows.size:
            self.comm.set_end(rows.astype(np.int32), np.full(rows.size, END_NONE))
        assert np.array_equal(rows, np.sort(self.model.sm.purge(now)))


def case_g5():
    trace = load_trace(GOLDEN)
    for chunk in (None, 64, 7, 1):
        store = DeviceShardStore(WORLD, len(trace["users"]))
        checked, turns, largest, mixed = replay_g5_sessions(trace, store, chunk)
        assert checked == 1345 and largest <= (chunk or 10 ** 9) and (chunk == 1 or mixed > 300)
        tm = store.model.sm.tm
        assert store.comm.table_size() == (659, len(trace["users"])) and tm.start.shape[0] == 659
        keys = np.stack([g5_key(t) for t in range(659)])
        got, want = store.comm.token_lookup(keys, NOW), tm.lookup(keys, NOW)
        for col in ("row", "live", "end"):
            assert np.array_equal(got[col], want[col]), (chunk, col)
        total = 0
        for r, c in enumerate(store.ctxs):
            snap = snapshot(c)
            sound(c, snap)
            assert snap["N_g"] == snap["covered_g"] == 659
            assert np.array_equal(snap["cols"][1], tm.end[snap["rows_g"]]) and np.array_equal(snap["cols"][0], tm.start[snap["rows_g"]]), (chunk, r)
            assert np.array_equal(store.owner[tm.user[snap["rows_g"]]], np.full(snap["rows_g"].size, r)), (chunk, r)
            total += snap["rows_g"].size
        assert total == 659
        store.comm.close()
    print("g5 ok: world %d" % WORLD)


# ------------------------------------------------------------------------------------------------ (b) the twin
def twin_ops(rng, k, known, known_user, users, owner):
    """roughly 60 / 15 / 5 / 20 % get / touch / delete / create; a tenth of the ops repeat a key of an earlier op of the turn;
    creates mostly bring fresh keys; a create that re-uses a key draws its user from the owner the key's row has (no key is held
    by two shards here: `shapes` designs that one)"""
    ops = np.zeros(k, TURN_OP)
    ops["kind"] = rng.choice([GET, TOUCH, DELETE, CREATE], k, p=[0.6, 0.15, 0.05, 0.2])
    ops["now"] = NOW + rng.integers(-6 * 10 ** 8, 6 * 10 ** 8, k)
    ops["new_end"] = np.where(np.isin(ops["kind"], (TOUCH, CREATE)), ops["now"] + rng.integers(-10 ** 8, 6 * 10 ** 8, k), 0)
    fresh = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
    user = rng.integers(0, users, k).astype(np.int32)
    by_owner = [np.nonzero(owner == r)[0] for r in range(int(owner.max()) + 1)]
    holder = {}                                       # key -> the owner of the rows under it
    for key, u in zip(known.tolist(), known_user.tolist()):
        holder[tuple(key)] = int(owner[u])
    for i in range(k):
        if i > 0 and rng.random() < 0.1:
            ops["tok"][i] = ops["tok"][rng.integers(0, i)]
        elif (ops["kind"][i] == CREATE and rng.random() < 0.85) or rng.random() < 0.05:
            ops["tok"][i] = fresh[i]
        else:
            ops["tok"][i] = known[rng.integers(0, known.shape[0])]
        if ops["kind"][i] == CREATE:
            key = tuple(ops["tok"][i].tolist())
            if key in holder:
                user[i] = rng.choice(by_owner[holder[key]])
            holder[key] = int(owner[user[i]])
    return ops, user, rng.integers(0, D, k).astype(np.int32)


def case_twin():
    n, users = 1500, 64
    cols, keys = columns(71, n, users), random_keys(72, n)
    owner = owners(users, WORLD)
    comm_a, a = sharded(WORLD, cols, users, keys)
    comm_b, b = sharded(WORLD, cols, users, keys)
    rng = np.random.default_rng(73 + WORLD)
    known, known_user = keys, cols[2]
    for k in (1, 64, 257, 300, 640):
        ops, user, disc = twin_ops(rng, k, known, known_user, users, owner)
        create = ops["kind"] == CREATE
        n_g = comm_a.table_size()[0]
        answers = []
        for r in range(WORLD):
            got, want = a[r].shard_session_turn(ops, user, disc, users), one_by_one(b[r], ops, user, disc, users)
            same_answers(got, want, ops, (k, r))
            kept = create & (owner[user] == r)
            assert np.array_equal(got["row"][kept], n_g + np.cumsum(create)[kept] - 1), (k, r, "the j-th create is global row N_g + j")
            assert np.all(got["row"][create & ~kept] == -1) and np.all(got["end"][create & ~kept] == END_NONE), (k, r)
            answers.append(got)
        assert np.all(merge(answers)["row"][create] >= 0), "every create is kept by one shard"
        known, known_user = np.concatenate([known, ops["tok"][create]]), np.concatenate([known_user, user[create]])
        assert comm_a.table_size() == comm_b.table_size() == (known.shape[0], users)
        for r in range(WORLD):
            sa, sb = snapshot(a[r]), snapshot(b[r])
            same_snapshot(sa, sb, (k, r), slots_exact=False)
            sound(a[r], sa)
            la, lb = a[r].shard_token_lookup(known, NOW), b[r].shard_token_lookup(known, NOW)
            for col in COLS:
                assert np.array_equal(la[col], lb[col]), (k, r, "lookup", col)
            scans_match(a[r], sa, (k, r))
        got = comm_a.token_lookup(known, NOW)
        assert np.all(got["row"] >= 0)
    comm_a.close()
    comm_b.close()
    print("twin ok: world %d" % WORLD)


# ------------------------------------------------------------------------------------------------ (c), (f) shapes
def twin_turn(a, b, ops, user, disc, users, tag):
    """the turn on every shard of `a`, the one-by-one sequence on `b`; answers and state compared per rank -> the answers"""
    out = []
    for r in range(len(a)):
        got, want = a[r].shard_session_turn(ops, user, disc, users), one_by_one(b[r], ops, user, disc, users)
        same_answers(got, want, ops, (tag, r))
        sa = snapshot(a[r])
        same_snapshot(sa, snapshot(b[r]), (tag, r), slots_exact=False)
        sound(a[r], sa)
        out.append(got)
    return out


def case_shapes():
    world, n, users = 3, 700, 40
    owner = owners(users, world)
    cols, keys = columns(91, n, users), random_keys(92, n)
    comm_a, a = sharded(world, cols, users, keys)
    comm_b, b = sharded(world, cols, users, keys)
    u0 = int(np.nonzero(owner == 0)[0][0])
    # a turn of one create: kept by rank 0, not kept by the others
    new = random_keys(93, 1)
    got = twin_turn(a, b, make_ops(new, NOW, CREATE, NOW + HOUR), np.array([u0], np.int32), np.array([3], np.int32), users, "one create")
    assert got[0]["row"][0] == n and got[0]["user"][0] == u0 and got[1]["row"][0] == -1 and got[2]["row"][0] == -1
    # 300 creates whose owners interleave: the local ordinal differs from the global one on every rank
    new, rng = random_keys(94, 300), np.random.default_rng(95)
    user = rng.integers(0, users, 300).astype(np.int32)
    got = twin_turn(a, b, make_ops(new, NOW + np.arange(300), CREATE, NOW + rng.integers(-HOUR, DAY, 300)), user, rng.integers(0, D, 300).astype(np.int32),
                    users, "300 creates")
    for r in range(world):
        mine = owner[user] == r
        assert 50 < mine.sum() < 200 and np.array_equal(got[r]["row"][mine], n + 1 + np.nonzero(mine)[0])
        rows_g, _ = a[r].shard_maps()
        assert np.array_equal(rows_g[-int(mine.sum()):], n + 1 + np.nonzero(mine)[0]) and np.all(np.diff(rows_g) > 0)
    # 257 ops whose only create is the last op: the second block holds that op alone, the lane of op 3 walks to it
    ops = make_ops(np.concatenate([keys[:256], keys[3:4]]), NOW, GET)
    ops["kind"][100:200], ops["new_end"][100:200] = TOUCH, NOW + 5 * DAY
    ops["kind"][256], ops["new_end"][256] = CREATE, NOW + HOUR
    holder = int(owner[cols[2][3]])
    same_owner = int(np.nonzero(owner == holder)[0][-1])
    got = twin_turn(a, b, ops, np.full(257, same_owner, np.int32), np.full(257, 1, np.int32), users, "257 ops")
    assert got[holder]["row"][256] == n + 301 and got[holder]["row"][3] == 3
    # (f) one designed two-shard key: a create for a user of ANOTHER owner than the key's older row.  Each shard answers for
    # itself (the per-rank model is the one-by-one sequence); the communicator's merge hands out the newer row
    other = int(np.nonzero(owner != owner[cols[2][5]])[0][0])
    ops = np.concatenate([make_ops(keys[5:6], NOW, TOUCH, NOW + 9 * DAY), make_ops(keys[5:6], NOW, CREATE, NOW + HOUR), make_ops(keys[5:6], NOW + 1, GET),
                          make_ops(keys[5:6], NOW + 2, DELETE)])
    got = twin_turn(a, b, ops, np.full(4, other, np.int32), np.full(4, 2, np.int32), users, "two-shard key")
    old, new_r = int(owner[cols[2][5]]), int(owner[other])
    assert got[old]["row"].tolist() == [5, -1, 5, 5] and got[new_r]["row"].tolist() == [-1, n + 302, n + 302, n + 302]
    assert comm_a.token_lookup(keys[5:6], NOW)["row"][0] == n + 302
    comm_a.close()
    comm_b.close()
    # the first row and the first user of a shard that was empty; new users arriving in the turn that logs them in
    users0 = 2
    owner = owners(400, world)
    while len(set(owner[:users0].tolist())) == world:          # some rank must start without a user
        users0 -= 1
    empty = [r for r in range(world) if r not in owner[:users0]][0]
    first = int(np.nonzero(owner == empty)[0][0])
    cols = columns(96, 50, users0)
    keys = random_keys(97, 50)
    comm_a, a = sharded(world, cols, users0, keys)
    comm_b, b = sharded(world, cols, users0, keys)
    assert a[empty].n == 0
    new = random_keys(98, 2)
    ops = np.concatenate([make_ops(new[:1], NOW, GET), make_ops(new[:1], NOW, CREATE, NOW + HOUR), make_ops(new[:1], NOW + 1, TOUCH, NOW + DAY),
                          make_ops(new[1:], NOW, CREATE, NOW + 2 * HOUR)])
    got = twin_turn(a, b, ops, np.array([0, first, 0, 0], np.int32), np.zeros(4, np.int32), first + 1, "first row of an empty shard")
    assert got[empty]["row"].tolist() == [-1, 50, 50, -1] and got[empty]["user"][1] == first and a[empty].n == 1
    assert comm_a.table_size() == (52, first + 1)
    # a create-free turn that only brings users: pie_shard_append_rows(k = 0), then the turn
    ops = make_ops(np.concatenate([new, keys[:3]]), NOW + 5, GET)
    for r in range(world):
        got, _ = a[r].shard_session_turn(ops, None, None, 400), b[r].shard_append_rows([], [], [], [], 400)
        want = b[r].shard_token_turn(ops)
        same_answers(got, want, ops, ("users only", r))
        same_snapshot(snapshot(a[r]), snapshot(b[r]), ("users only", r))
    assert comm_a.table_size() == (52, 400)
    # 120 logins of users the table has never seen, half of them beyond the user count the call brings
    rng = np.random.default_rng(99)
    user = rng.integers(300, 900, 120).astype(np.int32)
    got = twin_turn(a, b, make_ops(random_keys(100, 120), NOW, CREATE, NOW + DAY), user, np.zeros(120, np.int32), 900, "new users")
    assert np.array_equal(merge(got)["user"], user) and comm_a.table_size() == (172, 900)
    for r in range(world):
        scans_match(a[r], snapshot(a[r]), ("new users", r))
    comm_a.close()
    comm_b.close()
    print("shapes ok")


# ------------------------------------------------------------------------------------------------ (e), (g) room and derived state
def case_room():
    world, users = 2, 30
    owner = owners(users, world)
    on0, on1 = np.nonzero(owner == 0)[0].astype(np.int32), np.nonzero(owner == 1)[0].astype(np.int32)
    rng = np.random.default_rng(111)
    # rank 0 holds 500 rows of 1 024 slots, rank 1 a handful; 40 logins for users of rank 0 pass half its slots and outgrow its
    # columns; rank 1 keeps neither a row nor its size
    n = 520
    cols = list(columns(112, n, users))
    cols[2] = np.concatenate([rng.choice(on0, 500), rng.choice(on1, 20)]).astype(np.int32)[rng.permutation(n)]
    keys = random_keys(113, n)
    comm_a, a = sharded(world, cols, users, keys)
    comm_b, b = sharded(world, cols, users, keys)
    before = [snapshot(c) for c in a]
    assert before[0]["slots"] == before[1]["slots"] == 1024 and a[0].n == 500
    got = twin_turn(a, b, make_ops(random_keys(114, 40), NOW, CREATE, NOW + DAY), rng.choice(on0, 40).astype(np.int32), np.zeros(40, np.int32), users, "slots")
    after = [snapshot(c) for c in a]
    assert after[0]["slots"] == 2048 and after[1]["slots"] == 1024 and a[0].n == 540 and a[1].n == 20, "slots doubled on one rank only"
    assert np.all(got[1]["row"] == -1)
    for r in range(world):
        scans_match(a[r], after[r], ("slots", r))
    # users outgrown: the table was sharded with 30 users; 300 arrive, 100 of them log in
    user = rng.integers(30, 330, 100).astype(np.int32)
    twin_turn(a, b, make_ops(random_keys(115, 100), NOW, CREATE, NOW + DAY), user, np.ones(100, np.int32), 330, "users outgrown")
    assert comm_a.table_size() == (660, 330)
    # a compaction drops rows on rank 1 only: global rows keep their numbers, the turn's probes and new rows follow the new map
    dead = comm_a.ctx(1).shard_maps()[0][:7].astype(np.int32)
    for comm, ctxs in ((comm_a, a), (comm_b, b)):
        comm.set_end(dead, np.full(7, END_NONE))
        n1 = ctxs[1].n
        assert ctxs[1].compact_rows() == n1 - 7
    owner = owners(330, world)
    u1 = int(np.nonzero(owner == 1)[0][0])
    ops = np.concatenate([make_ops(keys[dead[:2]], NOW, GET), make_ops(random_keys(116, 3), NOW, CREATE, NOW + DAY), make_ops(keys[:20], NOW, GET)])
    got = twin_turn(a, b, ops, np.full(25, u1, np.int32), np.zeros(25, np.int32), 330, "after a compaction")
    assert got[1]["row"][:5].tolist() == [-1, -1, 660, 661, 662] and comm_a.table_size()[0] == 663
    comm_a.close()
    comm_b.close()
    print("room ok")

# ------------------------------------------------------------------------------------------------ (d) wrapping probe runs
def case_wrap():
    """Rank 0 of two holds 400 rows in 1 024 slots.  Forty of its resident keys have their home in the last four slots, so their run
    crosses the end of the table and pushes the forty keys with home 0 along.  One turn then creates forty more of each kind for
    users of rank 0 — the creates' probe runs wrap — and, in the same launch, asks for every resident key of those runs and for
    absent keys with the same homes: those walks go through slots claimed in this launch.  (The construction of
    test_probe_runs_that_wrap_and_slots_claimed_in_the_launch, on one shard.)"""
    world, users, n, log2_slots = 2, 30, 420, 10
    owner = owners(users, world)
    on0, on1 = np.nonzero(owner == 0)[0].astype(np.int32), np.nonzero(owner == 1)[0].astype(np.int32)
    rng = np.random.default_rng(104)
    cols = list(columns(101, n, users))
    cols[2] = np.concatenate([rng.choice(on0, 400), rng.choice(on1, 20)]).astype(np.int32)[rng.permutation(n)]
    mine = np.nonzero(owner[cols[2]] == 0)[0]                     # the global rows rank 0 holds, ascending: its local rows
    pool = random_keys(102, 300_000)
    homes = pie.token_homes(pool, log2_slots)
    tail, head = pool[homes >= (1 << log2_slots) - 4], pool[homes == 0]
    assert tail.shape[0] >= 120 and head.shape[0] >= 120
    keys = random_keys(103, n)
    keys[mine[:40]], keys[mine[40:80]] = tail[:40], head[:40]
    comm_a, a = sharded(world, cols, users, keys)
    comm_b, b = sharded(world, cols, users, keys)
    assert a[0].n == 400 and snapshot(a[0])["slots"] == 1 << log2_slots
    created = np.concatenate([tail[40:80], head[40:80]])
    absent = np.concatenate([tail[80:120], head[80:120]])
    resident = keys[mine[:80]]
    ask = np.concatenate([created, resident, absent, resident])
    kinds = np.concatenate([np.full(80, CREATE), rng.choice([GET, TOUCH, DELETE], 240, p=[0.5, 0.3, 0.2])])
    order = rng.permutation(320)
    ops = make_ops(ask[order], NOW + rng.integers(-10 ** 8, 10 ** 8, 320), kinds[order])
    ops["new_end"] = NOW + rng.integers(1, 10 ** 9, 320)
    got = twin_turn(a, b, ops, rng.choice(on0, 320).astype(np.int32), rng.integers(0, D, 320).astype(np.int32), users, "wrap")
    assert np.all(got[0]["row"][np.isin(ops["tok"][:, 0], absent[:, 0])] == -1) and np.count_nonzero(got[0]["row"] >= n) == 80
    assert np.all(got[1]["row"][ops["kind"] == CREATE] == -1)
    snap = snapshot(a[0])
    assert (snap["covered_l"], snap["slots"]) == (480, 1 << log2_slots)
    slot_row, back = snap["slot_row"], snap["keys"]
    slot_of = np.empty(480, np.int64)
    slot_of[slot_row[slot_row >= 0]] = np.nonzero(slot_row >= 0)[0]
    new_tail = np.nonzero(np.isin(back[:, 0], tail[40:80, 0]))[0]
    # the last four slots were full before the turn: every one of these creates sits below its home, past the end of the table
    assert np.all(new_tail >= 400) and np.all(slot_of[new_tail] < pie.token_homes(back[new_tail], log2_slots)), "the creates' runs crossed the end"
    every = np.concatenate([keys, created, absent])
    la, lb = a[0].shard_token_lookup(every, NOW), b[0].shard_token_lookup(every, NOW)
    for col in COLS:
        assert np.array_equal(la[col], lb[col]), ("wrap", "lookup", col)
    assert np.all(la["row"][n + 80:] == -1) and np.all(comm_a.token_lookup(created, NOW)["row"] >= n)
    comm_a.close()
    comm_b.close()
    print("wrap ok")


# ------------------------------------------------------------------------------------------------ (g) derived state
def shard_batches_exact(c, queries, discs, tag):
    """a batch on one shard against the oracle on that shard's own columns"""
    ti = c.table_info()
    c.n, c.n_users = int(ti["rows"]), int(ti["users"])
    s, e, u, d = c.read_columns()
    for q, res in enumerate(c.scan_batch(queries)):
        for x, y in zip(res, oracle_py.scan(s, e, u, d, c.n_users, *queries[q])):
            assert np.array_equal(x, y), (tag, q)


def case_derived():
    world, n, users, discs = 2, 40_000, 499, 32
    t0 = oracle_py.T0_MS
    owner = owners(users, world)
    cols = oracle_py.gen(0x5EED5EED + 9, n, 0, n, users, discs, 0)
    keys = random_keys(121, n)
    lim = (1 << discs) - 1
    queries = [(t0 - 6 * HOUR - 977 * q - (q % 5) * HOUR, t0 - (61 + q % 4) * DAY, (0x55555555, 0xAAAAAAAA, lim)[q % 3]) for q in range(16)]
    # the hot index live (PIE_HOT_INDEX on its default: a batch builds it), then a turn whose creates end near the top of the `end`
    # range and which touches and deletes others, then the batch that follows at once, exact on every shard
    os.environ.pop("PIE_HOT_INDEX", None)
    comm = pie.PieComm([0] * world)
    c = [comm.ctx(r) for r in range(world)]
    for r in range(world):
        c[r].load_columns(*cols, users)
        c[r].shard_table(r, world)
        c[r].set_disciplines(lim, discs)
    comm.token_set(keys)
    for r in range(world):
        shard_batches_exact(c[r], queries, discs, ("hot built", r))
    before = [c[r].table_info() for r in range(world)]
    assert all(i["hot_builds"] >= 1 and i["hot_rows"] > 0 for i in before), "the hot index is live on every shard before the turns"
    rng = np.random.default_rng(122)
    # a sharded table fits its columns exactly: the first logins outgrow them on both shards, and the key build that follows the
    # growth drops the index (as it does behind pie_shard_append_rows); the batch builds it again, over columns with room
    first = comm.session_turn(make_ops(random_keys(125, 20), t0 - 9 * HOUR, CREATE, t0 + HOUR), (np.arange(20) % users).astype(np.int32),
                              np.zeros(20, np.int32), users)
    assert np.array_equal(first["row"], n + np.arange(20)) and len(set(first["owner"].tolist())) == world
    for r in range(world):
        shard_batches_exact(c[r], queries, discs, ("hot built again", r))
    before = [c[r].table_info() for r in range(world)]
    assert all(i["hot_rows"] > 0 for i in before), "the hot index is live on every shard before the turn that must keep it"
    n += 20
    end = cols[1]
    top = np.argsort(end, kind="stable")[-100:]
    new = random_keys(123, 200)
    ops = np.concatenate([
        make_ops(new, t0 - rng.integers(8 * HOUR, 70 * DAY, 200), CREATE, int(end.max()) - rng.integers(0, 3 * HOUR, 200)),
        make_ops(keys[top[:50]], end[top[:50]] - 1, TOUCH, t0 - 20 * DAY),
        make_ops(new[:50], t0 - 7 * HOUR, TOUCH, t0 + 12 * HOUR),                       # created, then moved up in the same turn
        make_ops(new[50:80], t0, DELETE)])
    user = rng.integers(0, users, 330).astype(np.int32)
    got = comm.session_turn(ops, user, rng.integers(0, discs, 330).astype(np.int32), users)
    assert got["live"][:200].all() and got["live"][250:300].all() and np.array_equal(got["row"][:200], n + np.arange(200))
    assert np.array_equal(got["owner"][:200], owner[user[:200]]) and 50 < np.count_nonzero(owner[user[:200]] == 0) < 150
    for r in range(world):
        i = c[r].table_info()
        assert i["hot_rows"] > 0 and i["hot_builds"] == before[r]["hot_builds"], "the index took the turn's rows through its mirror: live, not rebuilt"
        shard_batches_exact(c[r], queries, discs, ("hot behind the turn", r))
        assert c[r].table_info()["hot_rows"] > 0
    comm.close()
    # the ordered run: kept in step by a create-free turn, dropped by a kept create, kept by the shard that keeps none
    comm = pie.PieComm([0] * world)
    c = [comm.ctx(r) for r in range(world)]
    now, cutoff, mask = t0 - 6 * HOUR, t0 - 61 * DAY, 0x55555555
    for r in range(world):
        c[r].set_ordered_run(2)
        c[r].load_columns(*cols, users)
        c[r].shard_table(r, world)
        c[r].set_disciplines(mask, discs)
    comm.token_set(keys)

    def scans_exact(tag):
        for r in range(world):
            ti = c[r].table_info()
            c[r].n, c[r].n_users = int(ti["rows"]), int(ti["users"])
            s, e, u, d = c[r].read_columns()
            for x, y in zip(c[r].scan(now, cutoff), oracle_py.scan(s, e, u, d, c[r].n_users, now, cutoff, mask)):
                assert np.array_equal(x, y), (tag, r)

    scans_exact("built")
    for r in range(world):
        assert c[r].stats()["k1_variant"] & 0x2000 and c[r].table_info()["ordered_rows"] > 0, "the ordered run is valid and used on every shard"
    live = np.nonzero(end > now)[0][:40]
    comm.session_turn(make_ops(keys[live], now, TOUCH, t0 + HOUR), None, None, users)
    assert all(c[r].table_info()["ordered_rows"] > 0 for r in range(world)), "a create-free turn keeps the run"
    scans_exact("behind a create-free turn")
    on0 = np.nonzero(owner == 0)[0].astype(np.int32)
    ops = np.concatenate([make_ops(random_keys(124, 30), now, CREATE, t0 + 2 * HOUR), make_ops(keys[live[:20]], now, TOUCH, t0 + 3 * HOUR)])
    comm.session_turn(ops, np.concatenate([rng.choice(on0, 30), np.zeros(20)]).astype(np.int32), np.zeros(50, np.int32), users)
    assert c[0].table_info()["ordered_rows"] == 0, "a kept create drops the shard's run"
    assert c[1].table_info()["ordered_rows"] > 0, "the shard that keeps no create keeps its run"
    scans_exact("behind a turn with creates")
    comm.close()
    print("derived ok")


# ------------------------------------------------------------------------------------------------ (h) refusals
def case_errors():
    world, n, users = 3, 600, 40
    cols, keys = columns(131, n, users), random_keys(132, n)
    comm, c = sharded(world, cols, users, keys)
    for r in range(world):
        c[r].set_disciplines(0xFF, D)
    new = random_keys(133, 8)
    ops = np.concatenate([make_ops(keys[:8], NOW, TOUCH, NOW + DAY), make_ops(new, NOW, CREATE, NOW + DAY), make_ops(keys[8:16], NOW, DELETE)])
    user, disc = (np.arange(24) % users).astype(np.int32), np.zeros(24, np.int32)
    before = [snapshot(x) for x in c]

    def refused(code, fn, text=None):
        try:
            fn()
            raise AssertionError("the call went through")
        except PieError as e:
            assert e.code == code and (text is None or text in str(e)), e

    def unchanged(tag):
        for r in range(world):
            same_snapshot(snapshot(c[r]), before[r], (tag, r))

    both = lambda o=ops, u=user, d=disc, nu=users: (lambda: comm.session_turn(o, u, d, nu), lambda: c[1].shard_session_turn(o, u, d, nu))
    # PIE_E_INVAL: pie_session_turn's argument cases, in global ids
    for field, value in (("kind", 4), ("kind", -1), ("reserved", 1)):
        bad = ops.copy()
        bad[field][23] = value
        for fn in both(o=bad):
            refused(PIE_E_INVAL, fn)
    bad_user = user.copy()
    bad_user[15] = users                                    # the last create names a user outside [0, n_users)
    for fn in both(u=bad_user) + both(u=None) + both(d=None) + both(nu=users - 1):
        refused(PIE_E_INVAL, fn)
    lib = comm._lib
    assert lib.pie_comm_session_turn(comm._c, None, 3, None, None, users, None, None, None, None, None, None) == PIE_E_INVAL
    assert lib.pie_shard_session_turn(c[0]._ctx, None, 3, None, None, users, None, None, None, None, None) == PIE_E_INVAL
    unchanged("arguments")
    # ... and the entry points that keep refusing the kind
    refused(PIE_E_INVAL, lambda: comm.token_turn(ops))
    refused(PIE_E_INVAL, lambda: c[0].shard_token_turn(ops))
    refused(PIE_E_INVAL, lambda: c[0].shard_token_turn_begin(ops))
    refused(PIE_E_STATE, lambda: c[0].session_turn(ops, user, disc, users))
    unchanged("the kind elsewhere")
    # PIE_E_STATE: a pipelined step begun and not collected, then finished and not collected
    comm.step_reserve(1, 0, 1 << 16)
    comm.step_begin([(NOW, NOW - 30 * DAY, 0x55)])
    refused(PIE_E_STATE, lambda: comm.session_turn(ops, user, disc, users))
    comm.step_finish()
    refused(PIE_E_STATE, lambda: comm.session_turn(ops, user, disc, users))
    comm.step_collect()
    # ... a batch in flight, a turn begun
    c[1].scan_batch_begin([(NOW, NOW - 30 * DAY, 0x55)])
    for fn in both():
        refused(PIE_E_STATE, fn)
    c[1].scan_batch_finish()
    c[1].shard_token_turn_begin(ops[:8])
    for fn in both():
        refused(PIE_E_STATE, fn)
    begun = c[1].shard_token_turn_finish()
    assert begun["row"].shape == (8,)
    before = [snapshot(x) for x in c]                       # the begun turn's touches stand
    # ... not sharded, no column
    with pie.PieScan(0) as plain:
        plain.load_columns(*cols, users)
        plain.token_set(keys)
        refused(PIE_E_STATE, lambda: plain.shard_session_turn(ops, user, disc, users))
    # ... a create while covered_g < N_g: rows appended whose keys have not come
    extra = columns(134, 5, users)
    comm.append_rows(*extra, users)
    before = [snapshot(x) for x in c]
    for fn in both():
        refused(PIE_E_STATE, fn, "covers")
    unchanged("covered_g < N_g")
    assert comm.session_turn(ops[:8], None, None, users)["row"].shape == (8,), "a create-free turn runs on a column that lags"
    comm.token_append(random_keys(135, 5))
    # ... one shard holds a row its map does not cover: behind the communicator the whole turn is refused, no shard changes
    c[1].append_rows([NOW], [NOW + DAY], [0], [1], c[1].n_users)
    before_others = {r: snapshot(c[r]) for r in (0, 2)}
    refused(PIE_E_STATE, lambda: comm.session_turn(ops, user, disc, users), "rank 1")
    for r in (0, 2):
        same_snapshot(snapshot(c[r]), before_others[r], ("one shard refuses", r))
    # the other shards still take the turn for themselves
    got = c[0].shard_session_turn(ops, user, disc, users)
    owner = owners(users, world)
    assert np.array_equal(got["row"][8:16] >= 0, owner[user[8:16]] == 0)
    comm.close()
    print("errors ok")


if __name__ == "__main__":
    try:
        {"g5": case_g5, "twin": case_twin, "shapes": case_shapes, "room": case_room, "wrap": case_wrap, "derived": case_derived, "errors": case_errors}[CASE]()
    finally:
        os.unlink(stub)
