"""GPU: a turn that logs in (pie_session_turn, k_session_turn in sph-pie_amd/csrc/pie_token.h).  The defining equivalence is checked
two ways: against tests/session_turn_model.py, the executable form of the header's rules, and against a second context driven by
the one-by-one sequence of existing calls (a CREATE = pie_append_rows of one row + pie_token_append of its key, every other op a
pie_token_turn of one op).  Then the chains by hand, the shapes at which the kernel can go wrong, the three ways of making room,
the derived state (hot index, ordered run) behind a turn with creates, and the refusals, which change nothing."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN
from session_turn_model import CREATE, SessionTurnModel, replay_g5_sessions
from token_model import END_NONE, check_layout
from trace_replay import load_trace
from turn_model import DELETE, GET, TOUCH, TURN_OP, make_ops, same_turn

pytestmark = pytest.mark.gpu

N, U, D = 3000, 64, 8
NOW = 1700000000000
HOUR, DAY = 3600 * 1000, 86400 * 1000
PIE_E_INVAL, PIE_E_STATE = -1, -6


def columns(seed, n=N, users=U):
    """Seeded columns with `end` on both sides of NOW: live and expired rows"""
    rng = np.random.default_rng(seed)
    start = NOW - rng.integers(1, 10 ** 9, n)
    end = NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, n)
    return start.astype(np.int64), end.astype(np.int64), rng.integers(0, users, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def load(ctx, seed, n=N, users=U):
    """a table with a key per row -> (model, keys)"""
    cols = columns(seed, n, users)
    ctx.load_columns(*cols, users)
    model = SessionTurnModel(*cols)
    keys = random_keys(seed + 1000, n)
    ctx.token_set(keys)
    model.token_set(keys)
    return model, keys


def run_turn(ctx, model, ops, user=None, disc=None, n_users=None, tag=""):
    k = ops.shape[0]
    user = np.zeros(k, np.int32) if user is None else np.asarray(user, np.int32)
    disc = np.zeros(k, np.int32) if disc is None else np.asarray(disc, np.int32)
    got, want = ctx.session_turn(ops, user, disc, n_users), model.turn(ops, user, disc)
    same_turn(got, want, tag)
    return got


def state_matches(ctx, model, keys=None):
    """the four columns, the covered rows, and (keys given) a lookup of every key"""
    assert ctx.n == model.start.shape[0]
    for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), (model.start, model.end, model.user, model.disc)):
        assert np.array_equal(got, want), name
    assert ctx.table_info()["token_rows"] == model.covered
    if keys is not None and len(keys):
        got, want = ctx.token_lookup(keys, NOW), model.lookup(keys, NOW)
        for col in ("row", "live", "end"):
            assert np.array_equal(got[col], want[col]), col
        assert np.array_equal(got["user"][want["found"]], want["user"][want["found"]])


def index_is_sound(pie, ctx):
    cov, slots, slot_row, back = ctx.token_layout()
    check_layout(cov, slots, slot_row, back, pie.token_homes(back, int(slots).bit_length() - 1))
    return cov, slots


class DeviceSessionStore:
    """what replay_g5_sessions drives: the device with the model beside it, every turn compared"""

    def __init__(self, ctx, n_users):
        self.ctx, self.U = ctx, n_users
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        ctx.load_columns(z64, z64, z32, z32, n_users)
        ctx.token_set(np.zeros((0, 2), np.uint64))           # an empty table with an empty column: every session is a turn's
        self.m = SessionTurnModel(z64, z64, z32, z32)

    def turn(self, ops, user, disc):
        return run_turn(self.ctx, self.m, ops, user, disc, self.U)

    def delete_user(self, u):
        assert np.array_equal(np.sort(self.ctx.delete_user(u)), np.nonzero((self.m.user == u) & (self.m.end != END_NONE))[0])
        self.m.delete_user(u)

    def purge(self, now):
        rows = np.sort(self.ctx.expired_queue(END_NONE, now)) if self.m.start.shape[0] else np.zeros(0, np.int32)
        if rows.size:
            self.ctx.set_end(rows.astype(np.int32), np.full(rows.size, END_NONE))
        assert np.array_equal(rows, self.m.purge(now))


@pytest.mark.parametrize("chunk", [None, 64, 7, 1])
def test_g5_with_the_logins_in_the_turns(pie, gpu_ctx, chunk):
    """the reference's own answers, recorded call by call, from turns of every size that carry the create calls too"""
    from turn_model import g5_key
    trace = load_trace(GOLDEN)
    store = DeviceSessionStore(gpu_ctx, len(trace["users"]))
    checked, turns, largest, mixed = replay_g5_sessions(trace, store, chunk)
    assert checked == 1345 and largest <= (chunk or 10 ** 9) and (chunk == 1 or mixed > 300)
    assert store.m.start.shape[0] == trace["sessions"] == 659
    state_matches(gpu_ctx, store.m, np.stack([g5_key(t) for t in range(659)]))
    index_is_sound(pie, gpu_ctx)


def twin_ops(rng, k, known, n_users):
    """60 % get, 15 % touch, 5 % delete, 20 % create; a tenth of the ops repeat a key of an earlier op of the same turn (keys created
    earlier in the turn included); creates mostly bring fresh keys, some re-use a known key; a few gets name unknown keys"""
    ops = np.zeros(k, TURN_OP)
    ops["kind"] = rng.choice([GET, TOUCH, DELETE, CREATE], k, p=[0.6, 0.15, 0.05, 0.2])
    ops["now"] = NOW + rng.integers(-6 * 10 ** 8, 6 * 10 ** 8, k)
    ops["new_end"] = np.where(np.isin(ops["kind"], (TOUCH, CREATE)), ops["now"] + rng.integers(-10 ** 8, 6 * 10 ** 8, k), 0)
    fresh = rng.integers(0, 2 ** 64, (k, 2), dtype=np.uint64)
    for i in range(k):
        if i > 0 and rng.random() < 0.1:
            ops["tok"][i] = ops["tok"][rng.integers(0, i)]
        elif (ops["kind"][i] == CREATE and rng.random() < 0.85) or rng.random() < 0.05:
            ops["tok"][i] = fresh[i]
        else:
            ops["tok"][i] = known[rng.integers(0, known.shape[0])]
    return ops, rng.integers(0, n_users, k).astype(np.int32), rng.integers(0, D, k).astype(np.int32)


def one_by_one(ctx, ops, user, disc, n_users):
    """the sequence the header defines a turn by"""
    k = ops.shape[0]
    out = {"row": np.empty(k, np.int32), "live": np.empty(k, np.uint8), "user": np.empty(k, np.int32), "start": np.empty(k, np.int64),
           "end": np.empty(k, np.int64)}
    for i in range(k):
        op = ops[i:i + 1]
        if int(op["kind"][0]) == CREATE:
            row = ctx.n
            ctx.append_rows(op["now"], op["new_end"], user[i:i + 1], disc[i:i + 1], n_users)
            ctx.token_append(op["tok"])
            got = {"row": [row], "live": [op["new_end"][0] > op["now"][0]], "user": [user[i]], "start": op["now"], "end": op["new_end"]}
        else:
            got = ctx.token_turn(op)
        for col in out:
            out[col][i] = got[col][0]
    return out


def test_twin_of_the_one_by_one_sequence(pie, oracle, gpu_ctx):
    a = gpu_ctx
    cols, keys = columns(71), random_keys(72, N)
    with pie.PieScan(0) as b:
        for ctx in (a, b):
            ctx.load_columns(*cols, U)
            ctx.token_set(keys)
        rng = np.random.default_rng(73)
        known = keys
        mask = (1 << D) - 1
        queries = [(NOW - 977 * q * HOUR // 100 + (q % 5 - 2) * 10 ** 8, NOW - (11 + q % 4) * DAY, (0x55, 0xAA, mask)[q % 3]) for q in range(16)]
        for k in (1, 64, 257, 300, 640):
            ops, user, disc = twin_ops(rng, k, known, U)
            got, want = a.session_turn(ops, user, disc, U), one_by_one(b, ops, user, disc, U)
            found = want["row"] >= 0
            for col in ("row", "live", "end"):
                assert np.array_equal(got[col], want[col]), (k, col, np.nonzero(got[col] != want[col])[0][:8])
            for col in ("user", "start"):
                assert np.array_equal(got[col][found | (ops["kind"] == CREATE)], want[col][found | (ops["kind"] == CREATE)]), (k, col)
            known = np.concatenate([known, ops["tok"][ops["kind"] == CREATE]])
            assert a.n == b.n == known.shape[0]
            table = b.read_columns()
            for name, x, y in zip(("start", "end", "user", "disc"), a.read_columns(), table):
                assert np.array_equal(x, y), (k, name)
            la, lb = a.token_lookup(known, NOW), b.token_lookup(known, NOW)
            for col in ("row", "live", "user", "start", "end"):
                assert np.array_equal(la[col], lb[col]), (k, "lookup", col)
            assert np.all(la["row"] >= 0)
            a.set_disciplines(queries[0][2], D)
            for x, y in zip(a.scan(queries[0][0], queries[0][1]), oracle.scan(*table, U, *queries[0])):
                assert np.array_equal(x, y), (k, "scan")
            a.set_disciplines(mask, D)
            for q, res in enumerate(a.scan_batch(queries)):
                for x, y in zip(res, oracle.scan(*table, U, *queries[q])):
                    assert np.array_equal(x, y), (k, "batch", q)
        index_is_sound(pie, a)


def test_chains_by_hand(gpu_ctx):
    ctx = gpu_ctx
    model, keys = load(ctx, 81, 200)
    live = np.nonzero(model.end > NOW + 10 ** 8)[0]
    new = random_keys(82, 8)
    one = lambda key, now, kind, new_end=0: make_ops(np.asarray(key, np.uint64).reshape(1, 2), now, kind, new_end)
    ops = np.concatenate([
        # a fresh key: not found before its create; get, touch, delete behind it act on the new row
        one(new[0], NOW, GET), one(new[0], NOW, CREATE, NOW + HOUR), one(new[0], NOW + 1, GET), one(new[0], NOW + 2, TOUCH, NOW + DAY),
        one(new[0], NOW + 3, GET), one(new[0], NOW + 4, DELETE), one(new[0], NOW + 5, GET),
        # a key with an older live row: the touch before the create lands in the OLD row, everything after sees the new one
        one(keys[live[0]], NOW, TOUCH, NOW + 7 * DAY), one(keys[live[0]], NOW, CREATE, NOW + 2 * HOUR), one(keys[live[0]], NOW, GET),
        one(keys[live[0]], NOW, TOUCH, NOW + 3 * HOUR),
        # two creates of one key: both get rows, the later one answers
        one(new[1], NOW, CREATE, NOW + HOUR), one(new[1], NOW, CREATE, NOW + 2 * HOUR), one(new[1], NOW, GET),
        # new_end <= now: live 0, but findable
        one(new[2], NOW, CREATE, NOW), one(new[2], NOW - 1, GET), one(new[2], NOW, GET),
        # delete, then create, then get
        one(keys[live[1]], NOW, DELETE), one(keys[live[1]], NOW, CREATE, NOW + HOUR), one(keys[live[1]], NOW, GET)])
    user = np.arange(ops.shape[0], dtype=np.int32) % U
    got = run_turn(ctx, model, ops, user, user % D, U)
    r = 200
    assert got["row"][:7].tolist() == [-1, r, r, r, r, r, r] and got["live"][:7].tolist() == [0, 1, 1, 1, 1, 0, 0]
    assert got["end"][4] == NOW + DAY and model.end[r] == END_NONE
    assert got["row"][7:11].tolist() == [live[0], r + 1, r + 1, r + 1] and got["live"][7:11].all()
    assert model.end[live[0]] == NOW + 7 * DAY and model.end[r + 1] == NOW + 3 * HOUR
    assert got["row"][11:14].tolist() == [r + 2, r + 3, r + 3] and got["end"][13] == NOW + 2 * HOUR
    assert got["row"][14:17].tolist() == [r + 4] * 3 and got["live"][14:17].tolist() == [0, 1, 0]
    assert got["row"][17:].tolist() == [live[1], r + 5, r + 5] and got["live"][17:].tolist() == [0, 1, 1] and model.end[live[1]] == END_NONE
    assert got["user"][1] == 1 and got["start"][2] == NOW
    state_matches(ctx, model, np.concatenate([keys, new[:3]]))       # pie_read_columns shows the old row's touch and its tombstone
    # the next turn finds every new row through the index
    again = run_turn(ctx, model, make_ops(np.concatenate([new[:3], keys[live[:2]]]), NOW, GET))
    assert again["row"].tolist() == [r, r + 3, r + 4, r + 1, r + 5]


def test_shapes(pie, gpu_ctx):
    ctx = gpu_ctx
    model, keys = load(ctx, 91, 700)
    issued = [keys]
    # k = 1, a create
    new = random_keys(92, 1)
    run_turn(ctx, model, make_ops(new, NOW, CREATE, NOW + HOUR), [5], [3], U, "k = 1")
    issued.append(new)
    # 300 creates and nothing else: two blocks, the new rows span several waves
    new = random_keys(93, 300)
    rng = np.random.default_rng(94)
    got = run_turn(ctx, model, make_ops(new, NOW + np.arange(300), CREATE, NOW + rng.integers(-HOUR, DAY, 300)),
                   rng.integers(0, U, 300), rng.integers(0, D, 300), U, "300 creates")
    assert got["row"].tolist() == list(range(701, 1001))
    issued.append(new)
    # 257 ops, the one create is the last op: the second block holds that op alone, and the lane of op 3, in the first block,
    # walks to it
    ops = make_ops(np.concatenate([keys[:256], keys[3:4]]), NOW, GET)
    ops["kind"][100:200], ops["new_end"][100:200] = TOUCH, NOW + 5 * DAY
    ops["kind"][256], ops["new_end"][256] = CREATE, NOW + HOUR
    got = run_turn(ctx, model, ops, np.full(257, 9), np.full(257, 1), U, "257 ops")
    assert got["row"][256] == 1001 and got["row"][3] == 3
    state_matches(ctx, model, np.concatenate(issued))
    index_is_sound(pie, ctx)


def test_probe_runs_that_wrap_and_slots_claimed_in_the_launch(pie, gpu_ctx):
    """1 024 slots.  Forty resident keys have their home in the last four slots, so their run crosses the end of the table and
    pushes the forty keys with home 0 along.  One turn then creates forty more of each kind — the creates' probe runs wrap — and, in
    the same launch, asks for every resident key of those runs and for absent keys with the same homes: those walks go through
    slots claimed in this launch."""
    ctx = gpu_ctx
    n, log2_slots = 400, 10
    cols = columns(101, n)
    ctx.load_columns(*cols, U)
    model = SessionTurnModel(*cols)
    pool = random_keys(102, 300_000)
    homes = pie.token_homes(pool, log2_slots)
    tail, head = pool[homes >= (1 << log2_slots) - 4], pool[homes == 0]
    assert tail.shape[0] >= 120 and head.shape[0] >= 120
    keys = random_keys(103, n)
    keys[:40], keys[40:80] = tail[:40], head[:40]
    ctx.token_set(keys)
    model.token_set(keys)
    rng = np.random.default_rng(104)
    created = np.concatenate([tail[40:80], head[40:80]])
    absent = np.concatenate([tail[80:120], head[80:120]])
    ask = np.concatenate([created, keys[:80], absent, keys[:80]])
    kinds = np.concatenate([np.full(80, CREATE), rng.choice([GET, TOUCH, DELETE], 240, p=[0.5, 0.3, 0.2])])
    order = rng.permutation(320)
    ops = make_ops(ask[order], NOW + rng.integers(-10 ** 8, 10 ** 8, 320), kinds[order])
    ops["new_end"] = NOW + rng.integers(1, 10 ** 9, 320)
    got = run_turn(ctx, model, ops, rng.integers(0, U, 320), rng.integers(0, D, 320), U)
    assert np.all(got["row"][np.isin(ops["tok"][:, 0], absent[:, 0])] == -1) and np.count_nonzero(got["row"] >= n) == 80
    cov, slots = index_is_sound(pie, ctx)
    assert (cov, slots) == (480, 1 << log2_slots)
    _, _, slot_row, back = ctx.token_layout()
    slot_of = np.empty(cov, np.int64)
    slot_of[slot_row[slot_row >= 0]] = np.nonzero(slot_row >= 0)[0]
    new_tail = np.nonzero(np.isin(back[:, 0], tail[40:80, 0]))[0]
    # the last four slots were full before the turn: every one of these creates sits below its home, past the end of the table
    assert np.all(new_tail >= n) and np.all(slot_of[new_tail] < pie.token_homes(back[new_tail], log2_slots)), "the creates' runs crossed the end"
    state_matches(ctx, model, np.concatenate([keys, created, absent]))


def test_room(pie, oracle):
    """a context of its own: the capacities are the ones this table's load gave (the session's shared context keeps the capacity of
    the largest table any earlier test loaded, and nothing would have to grow)"""
    with pie.PieScan(0) as ctx:
        room_checks(pie, oracle, ctx)


def room_checks(pie, oracle, ctx):
    model, keys = load(ctx, 111, 500)
    issued = [keys]
    rng = np.random.default_rng(112)

    def creates(k, users, tag):
        new = random_keys(int(rng.integers(1 << 30)), k)
        ops = np.concatenate([make_ops(new, NOW, CREATE, NOW + rng.integers(-HOUR, DAY, k)), make_ops(new[: k // 2], NOW, GET)])
        user = np.concatenate([rng.integers(0, users, k), np.zeros(k // 2)])
        got = run_turn(ctx, model, ops, user, user % D, users, tag)
        issued.append(new)
        state_matches(ctx, model, np.concatenate(issued))
        index_is_sound(pie, ctx)
        return got

    # 500 keys in 1 024 slots; 20 creates cross 512 covered rows: the slots double, by one rebuild
    info = ctx.table_info()
    assert ctx.token_layout()[1] == 1024 and info["token_rows"] == 500
    builds = info["token_builds"]
    creates(20, U, "slots")
    info = ctx.table_info()
    assert ctx.token_layout()[1] == 2048 and info["token_builds"] == builds + 1
    # past the capacity of the columns
    cap = info["table_bytes"] // 24
    assert ctx.n <= cap <= 2 * ctx.n, "the turn below is a few hundred creates"
    creates(int(cap - ctx.n) + 5, U, "rows")
    info = ctx.table_info()
    assert info["table_bytes"] // 24 > cap and info["rows"] == cap + 5
    # past the capacity of the users: the new users' sessions come in the same turn
    got = creates(30, 4 * U + 3, "users")
    assert ctx.table_info()["users"] == 4 * U + 3 and got["user"][:30].max() >= U
    # a turn without a create brings users too, as an append of no rows does
    run_turn(ctx, model, make_ops(keys[:5], NOW, GET), n_users=4 * U + 9)
    assert ctx.table_info()["users"] == 4 * U + 9
    state_matches(ctx, model, np.concatenate(issued))
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)
    for x, y in zip(ctx.scan(NOW, 0), oracle.scan(model.start, model.end, model.user, model.disc, 4 * U + 9, NOW, 0, mask)):
        assert np.array_equal(x, y), "a scan behind the three growths"


def test_hot_index_behind_a_turn_with_creates(pie, oracle):
    """PIE_HOT_INDEX on its default: a batch builds the index, a turn creates sessions that end near the top of the `end` range
    (and touches and deletes others), and the batch that follows at once is exact"""
    n, users, discs = 20_000, 499, 32
    t0 = oracle.T0_MS
    cols = oracle.gen(0x5EED5EED + 9, n, 0, n, users, discs, 0)
    with pie.PieScan(0) as ctx:
        ctx.load_columns(*cols, users)
        model = SessionTurnModel(*cols)
        keys = random_keys(121, n)
        ctx.token_set(keys)
        model.token_set(keys)
        lim = (1 << discs) - 1
        ctx.set_disciplines(lim, discs)
        queries = [(t0 - 6 * HOUR - 977 * q - (q % 5) * HOUR, t0 - (61 + q % 4) * DAY, (0x55555555, 0xAAAAAAAA, lim)[q % 3]) for q in range(16)]

        def check(tag):
            for q, res in enumerate(ctx.scan_batch(queries)):
                for x, y in zip(res, oracle.scan(model.start, model.end, model.user, model.disc, users, *queries[q])):
                    assert np.array_equal(x, y), (tag, q)

        check("built")
        info = ctx.table_info()
        assert info["hot_builds"] >= 1 and info["hot_rows"] > 0
        rng = np.random.default_rng(122)
        top = np.argsort(model.end, kind="stable")[-100:]
        new = random_keys(123, 200)
        ops = np.concatenate([
            make_ops(new, t0 - rng.integers(8 * HOUR, 70 * DAY, 200), CREATE, int(model.end.max()) - rng.integers(0, 3 * HOUR, 200)),
            make_ops(keys[top[:50]], model.end[top[:50]] - 1, TOUCH, t0 - 20 * DAY),
            make_ops(new[:50], t0 - 7 * HOUR, TOUCH, t0 + 12 * HOUR),                       # created, then moved up in the same turn
            make_ops(new[50:80], t0, DELETE)])
        user = rng.integers(0, users, 330)
        got = run_turn(ctx, model, ops, user, rng.integers(0, discs, 330), users, "hot")
        assert got["live"][:200].all() and got["live"][250:300].all()
        assert np.count_nonzero(model.end[n:] > queries[0][0]) == 170, "the new sessions are among the rows the queries find live"
        check("behind the turn")
        state_matches(ctx, model)


def test_ordered_run_behind_a_turn_with_creates(pie, oracle):
    n, users, discs = 20_000, 499, 32
    t0 = oracle.T0_MS
    cols = oracle.gen(0x5EED5EED + 10, n, 0, n, users, discs, 0)
    with pie.PieScan(0) as ctx:
        ctx.set_ordered_run(2)
        ctx.load_columns(*cols, users)
        model = SessionTurnModel(*cols)
        keys = random_keys(131, n)
        ctx.token_set(keys)
        model.token_set(keys)
        now, cutoff, mask = t0 - 6 * HOUR, t0 - 61 * DAY, 0x55555555
        ctx.set_disciplines(mask, discs)

        def check(tag):
            for x, y in zip(ctx.scan(now, cutoff), oracle.scan(model.start, model.end, model.user, model.disc, users, now, cutoff, mask)):
                assert np.array_equal(x, y), tag

        check("built")
        assert ctx.stats()["k1_variant"] & 0x2000 and ctx.table_info()["ordered_rows"] > 0, "the ordered run was not used"
        # a turn without a create keeps the run, as pie_token_turn does
        live = np.nonzero(model.end > now)[0][:40]
        run_turn(ctx, model, make_ops(keys[live], now, TOUCH, t0 + HOUR), n_users=users)
        assert ctx.table_info()["ordered_rows"] > 0
        check("touched")
        rng = np.random.default_rng(132)
        new = random_keys(133, 100)
        ops = np.concatenate([make_ops(new, t0 - rng.integers(7 * HOUR, 30 * DAY, 100), CREATE, t0 + rng.integers(-HOUR, 12 * HOUR, 100)),
                              make_ops(keys[live[:20]], now, DELETE)])
        run_turn(ctx, model, ops, rng.integers(0, users, 120), rng.integers(0, discs, 120), users, "ordered")
        assert ctx.table_info()["ordered_rows"] == 0, "a turn with creates drops the run"
        check("behind the turn")
        held = ctx.table_info()["ordered_rows"]
        assert held == 0 or held >= np.count_nonzero(model.end[n:] > now), "dropped, or rebuilt with the new rows"
        state_matches(ctx, model)


def test_errors_change_nothing(pie, gpu_ctx):
    ctx = gpu_ctx
    model, keys = load(ctx, 141, 600)
    new = random_keys(142, 4)
    ops = np.concatenate([make_ops(keys[:3], NOW - 10 ** 9, TOUCH, NOW + 10 ** 9), make_ops(new, NOW, CREATE, NOW + HOUR)])
    user, disc = np.arange(7, dtype=np.int32), np.zeros(7, np.int32)
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)

    def snapshot():
        cov, slots, slot_row, back = ctx.token_layout()
        return [a.copy() for a in ctx.read_columns()] + [slot_row.copy(), back.copy(), np.array([cov, slots, ctx.table_info()["token_rows"], ctx.table_info()["rows"]])]

    def code(*a):
        before = snapshot()
        with pytest.raises(pie.PieError) as ei:
            ctx.session_turn(*a)
        for x, y in zip(before, snapshot()):
            assert np.array_equal(x, y)
        return ei.value.code

    bad_user = user.copy()
    bad_user[5] = U
    assert code(ops, bad_user, disc, U) == PIE_E_INVAL, "a user id out of range"
    bad_user[5] = -1
    assert code(ops, bad_user, disc, U) == PIE_E_INVAL
    assert code(ops, None, disc, U) == PIE_E_INVAL and code(ops, user, None, U) == PIE_E_INVAL, "NULL user / disc with a create"
    assert code(ops, user, disc, U - 1) == PIE_E_INVAL, "n_users below the context's"
    for field, value in (("kind", 4), ("kind", -1), ("reserved", 1)):
        bad = ops.copy()
        bad[field][1] = value
        assert code(bad, user, disc, U) == PIE_E_INVAL, (field, value)
    assert ctx._lib.pie_session_turn(ctx._ctx, None, 4, None, None, U, None, None, None, None, None) == PIE_E_INVAL
    before = snapshot()
    ctx.scan_batch_begin([(NOW, 0, mask), (NOW - HOUR, 0, 1)])
    with pytest.raises(pie.PieError) as ei:
        ctx.session_turn(ops, user, disc, U)
    assert ei.value.code == PIE_E_STATE, "a batch in flight"
    ctx.scan_batch_finish()
    ctx.token_turn_begin(make_ops(keys[:3], NOW, GET))
    with pytest.raises(pie.PieError) as ei:
        ctx.session_turn(ops, user, disc, U)
    assert ei.value.code == PIE_E_STATE, "a turn begun and not finished"
    ctx.token_turn_finish()
    for x, y in zip(before, snapshot()):
        assert np.array_equal(x, y)
    # pie_token_turn and its begin form keep refusing the kind
    for fn in (ctx.token_turn, ctx.token_turn_begin):
        with pytest.raises(pie.PieError) as ei:
            fn(ops)
        assert ei.value.code == PIE_E_INVAL
    # rows the column does not cover: a create is refused, a turn without one works
    ctx.append_rows([NOW], [NOW + HOUR], [1], [1], U)
    model.append_rows([NOW], [NOW + HOUR], [1], [1])
    assert code(ops, user, disc, U) == PIE_E_STATE, "token_rows < rows with a create"
    got = ctx.session_turn(ops[:3], None, None, U)
    same_turn(got, model.turn(ops[:3]), "no create, column short")
    assert ctx.table_info()["token_rows"] == 600 and ctx.n == 601
    # ... and with the column complete again the same turn goes through, outputs optional
    ctx.token_append(random_keys(143, 1))
    model.token_append(random_keys(143, 1))
    run_turn(ctx, model, ops, user, disc, U)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    more = make_ops(random_keys(144, 2), NOW, CREATE, NOW + HOUR)
    assert ctx._lib.pie_session_turn(ctx._ctx, p(more), 2, p(user), p(disc), U, None, None, None, None, None) == 0
    ctx.n += 2
    model.turn(more, user, disc)
    assert ctx._lib.pie_session_turn(ctx._ctx, None, 0, None, None, U, None, None, None, None, None) == 0
    state_matches(ctx, model, np.concatenate([keys, new, more["tok"]]))
    with pie.PieScan(0) as fresh:                    # no table at all; a table without a column
        with pytest.raises(pie.PieError) as ei:
            fresh.session_turn(ops, user, disc, U)
        assert ei.value.code == PIE_E_STATE
        fresh.load_columns(*columns(145, 10), U)
        with pytest.raises(pie.PieError) as ei:
            fresh.session_turn(ops, user, disc, U)
        assert ei.value.code == PIE_E_STATE
