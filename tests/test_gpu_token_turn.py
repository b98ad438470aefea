"""GPU: a whole turn in one launch (pie_token_turn, k_token_turn in sph-pie_amd/csrc/pie_token.h) against tests/turn_model.py, the
executable form of the header's rules: the recorded reference trace G5 replayed in turns, seeded random turns with clocks of
their own, probe runs that wrap, the derived state (hot index, ordered run) behind a turn, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN
from session_turn_model import CREATE, SessionTurnModel
from table_model import ctx_with_env
from token_model import END_NONE, check_layout
from trace_replay import load_trace
from turn_model import DELETE, GET, TOUCH, TURN_OP, TurnModel, make_ops, replay_g5, same_turn

pytestmark = pytest.mark.gpu

N, U, D = 3000, 50, 8
NOW = 1700000000000
ALL = 2 ** 64 - 1
HOUR, DAY = 3600 * 1000, 86400 * 1000
PIE_E_INVAL, PIE_E_STATE = -1, -6


def columns(seed, n=N):
    """Seeded columns with `end` on both sides of NOW: live and expired rows"""
    rng = np.random.default_rng(seed)
    start = NOW - rng.integers(1, 10 ** 9, n)
    end = NOW + rng.integers(-5 * 10 ** 8, 5 * 10 ** 8, n)
    return start.astype(np.int64), end.astype(np.int64), rng.integers(0, U, n).astype(np.int32), rng.integers(0, D, n).astype(np.int32)


def random_keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2 ** 64, (n, 2), dtype=np.uint64)


def load(ctx, seed, n=N, tombstones=30):
    """a table with a key per row, `tombstones` rows deleted -> (model, keys)"""
    cols = columns(seed, n)
    ctx.load_columns(*cols, U)
    model = TurnModel(*cols)
    keys = random_keys(seed + 1000, n)
    ctx.token_set(keys)
    model.token_set(keys)
    tomb = np.random.default_rng(seed + 2000).choice(n, tombstones, replace=False).astype(np.int32)
    ctx.set_end(tomb, np.full(tombstones, END_NONE))
    model.end[tomb] = END_NONE
    return model, keys


def run_turn(ctx, model, ops, tag=""):
    got, want = ctx.token_turn(ops), model.turn(ops)
    same_turn(got, want, tag)
    return got


def columns_match(ctx, model):
    for name, got, want in zip(("start", "end", "user", "disc"), ctx.read_columns(), (model.start, model.end, model.user, model.disc)):
        assert np.array_equal(got, want), name


class DeviceStore:
    """what replay_g5 drives: the device with the model beside it, every turn compared"""

    def __init__(self, ctx, n_users):
        self.ctx, self.U = ctx, n_users
        z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
        ctx.load_columns(z64, z64, z32, z32, n_users)
        self.m = TurnModel(z64, z64, z32, z32)

    def create(self, start, end, user, key):
        self.ctx.append_rows(np.array([start], np.int64), np.array([end], np.int64), np.array([user], np.int32), np.zeros(1, np.int32), self.U)
        if self.m.covered == 0:
            self.ctx.token_set(key.reshape(1, 2))      # the first session: the column comes with it
        else:
            self.ctx.token_append(key.reshape(1, 2))
        self.m.append_rows([start], [end], [user], [0])
        self.m.token_append(key.reshape(1, 2))

    def turn(self, ops):
        return run_turn(self.ctx, self.m, ops)

    def delete_user(self, u):
        assert np.array_equal(np.sort(self.ctx.delete_user(u)), np.nonzero((self.m.user == u) & (self.m.end != END_NONE))[0])
        self.m.delete_user(u)

    def purge(self, now):
        rows = np.sort(self.ctx.expired_queue(END_NONE, now)) if self.m.start.shape[0] else np.zeros(0, np.int32)
        if rows.size:
            self.ctx.set_end(rows.astype(np.int32), np.full(rows.size, END_NONE))
        assert np.array_equal(rows, self.m.purge(now))


@pytest.mark.parametrize("chunk", [None, 64, 7, 1])
def test_g5_in_turns_on_the_device(gpu_ctx, chunk):
    """the reference's own answers, recorded call by call, from turns of every size; the final columns are the model's"""
    trace = load_trace(GOLDEN)
    store = DeviceStore(gpu_ctx, len(trace["users"]))
    checked, turns, largest = replay_g5(trace, store, chunk)
    assert checked == 1345 and largest <= (chunk or 10 ** 9)
    assert store.m.start.shape[0] == trace["sessions"] == 659
    columns_match(gpu_ctx, store.m)


def random_ops(rng, k, keys, model, hot_keys):
    """k ops: half of them on the 8 `hot_keys` (chains form), the rest on keys of the table and on unknown keys; every op has a clock
    of its own, not monotone, on both sides of the rows' ends; touches set ends on both sides of the clocks"""
    ops = np.zeros(k, TURN_OP)
    pick_hot = rng.random(k) < 0.5
    others = np.concatenate([keys[rng.integers(0, keys.shape[0], k)], random_keys(int(rng.integers(1 << 30)), k)])[rng.permutation(2 * k)[:k]] if k else keys[:0]
    ops["tok"] = np.where(pick_hot[:, None], hot_keys[rng.integers(0, 8, k)], others)
    ops["now"] = NOW + rng.integers(-6 * 10 ** 8, 6 * 10 ** 8, k)
    ops["kind"] = rng.choice([GET, TOUCH, DELETE], k, p=[0.5, 0.35, 0.15])
    ops["new_end"] = np.where(ops["kind"] == TOUCH, ops["now"] + rng.integers(-10 ** 8, 6 * 10 ** 8, k), 0)
    return ops


def test_seeded_random_turns(oracle, gpu_ctx):
    ctx = gpu_ctx
    model, keys = load(ctx, 31)
    rng = np.random.default_rng(32)
    unknown = random_keys(33, 1)

    def rows_now(n_live):
        live = np.nonzero(model.end > NOW + 10 ** 8)[0]
        expired = np.nonzero((model.end <= NOW - 10 ** 8) & (model.end != END_NONE))[0]
        tomb = np.nonzero(model.end == END_NONE)[0]
        return live[:n_live], expired[:1], tomb[:1]

    kinds_seen = set()
    for k in (0, 1, 2, 255, 256, 257, 1025):
        for rep in range(2):
            live, expired, tomb = rows_now(5)
            hot_keys = np.concatenate([keys[live], keys[expired], keys[tomb], unknown])      # 8 keys: chains form on them
            ops = random_ops(rng, k, keys, model, hot_keys)
            got = run_turn(ctx, model, ops, (k, rep))
            assert got["row"].shape == (k,)
            kinds_seen |= {(int(kd), int(lv), bool(r >= 0)) for kd, lv, r in zip(ops["kind"], got["live"], got["row"])}
        columns_match(ctx, model)
    # every line of the header's table was met: gets live and not, touches applied and not, deletes applied and not, unknown keys
    assert {(GET, 1, True), (GET, 0, True), (GET, 0, False), (TOUCH, 1, True), (TOUCH, 0, True), (TOUCH, 0, False), (DELETE, 0, True),
            (DELETE, 0, False)} <= kinds_seen
    # 300 ops on a single key, none of them a delete: one lane walks them all, in order
    fresh = rows_now(3)[0]
    ops = random_ops(rng, 300, keys, model, hot_keys)
    ops["tok"] = keys[fresh[0]]
    ops["kind"] = np.where(ops["kind"] == DELETE, GET, ops["kind"])
    ops["kind"][:3] = (TOUCH, GET, GET)
    ops["now"][:3] = NOW - 1
    ops["new_end"][0] = NOW + 10 ** 9
    got = run_turn(ctx, model, ops, "one key")
    assert got["live"][:3].tolist() == [1, 1, 1] and got["end"][1] == NOW + 10 ** 9 and np.all(got["user"] == model.user[fresh[0]])
    assert np.all(got["row"] == fresh[0]) and 0 < got["live"].sum() < 300
    # ... and on another key with a delete in the middle: everything behind it is dead
    ops["tok"] = keys[fresh[1]]
    ops["kind"][150] = DELETE
    ops["now"][:150] = NOW - 1
    got = run_turn(ctx, model, ops, "one key, deleted")
    assert got["live"][0] == 1 and not got["live"][150:].any() and np.all(got["end"][150:] == END_NONE) and model.end[fresh[1]] == END_NONE
    columns_match(ctx, model)
    # outputs are optional, k = 0 needs no ops
    lib = ctx._lib
    ops = make_ops(keys[fresh[2]:fresh[2] + 1], NOW, TOUCH, NOW + 77)
    assert lib.pie_token_turn(ctx._ctx, ops.ctypes.data_as(C.c_void_p), 1, None, None, None, None, None) == 0
    assert model.turn(ops)["live"][0] == 1
    assert lib.pie_token_turn(ctx._ctx, None, 0, None, None, None, None, None) == 0
    columns_match(ctx, model)
    # the derived keys followed every store
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)
    for now in (NOW, NOW + 10 ** 8, NOW - 3 * 10 ** 8):
        for a, b in zip(ctx.scan(now, 0), oracle.scan(model.start, model.end, model.user, model.disc, U, now, 0, mask)):
            assert np.array_equal(a, b), "the derived keys fell out of step"


def test_staging_growth(pie):
    """The staging of the synchronous turns on a context of its own, whose first block (64 KiB) holds about 900 ops: a turn of 10
    ops, one of 4 096 that outgrows the block, then a turn of 2 048 ops that logs 100 sessions in, whose create arrays move the
    results inside the block."""
    with pie.PieScan(0) as ctx:
        cols = columns(61)
        ctx.load_columns(*cols, U)
        model = SessionTurnModel(*cols)
        keys = random_keys(1061, N)
        ctx.token_set(keys)
        model.token_set(keys)
        rng = np.random.default_rng(62)
        hot_keys = keys[rng.choice(N, 8, replace=False)]
        bytes_seen = []
        for k in (10, 4096):
            ops = random_ops(rng, k, keys, model, hot_keys)
            same_turn(ctx.token_turn(ops), model.turn(ops), k)
            columns_match(ctx, model)
            bytes_seen.append(ctx.table_info()["token_bytes"])
        assert bytes_seen[1] > bytes_seen[0], "the staging did not grow"
        ops = random_ops(rng, 2048, keys, model, hot_keys)
        at = rng.choice(2048, 100, replace=False)
        ops["kind"][at] = CREATE
        ops["tok"][at[10:]] = random_keys(63, 90)        # ten creates keep their key: some log in under a key of the table or a chain's
        ops["new_end"][at] = ops["now"][at] + rng.integers(1, 6 * 10 ** 8, 100)
        user, disc = rng.integers(0, U, 2048).astype(np.int32), rng.integers(0, D, 2048).astype(np.int32)
        want = model.turn(ops, user, disc)
        same_turn(ctx.session_turn(ops, user, disc, U), want, "2 048 ops, 100 creates")
        assert np.array_equal(want["row"][np.sort(at)], N + np.arange(100)) and ctx.n == N + 100
        columns_match(ctx, model)
        got, back = ctx.token_lookup(keys, NOW), model.lookup(keys, NOW)
        assert np.array_equal(got["row"], back["row"]) and np.array_equal(got["end"], back["end"])


def test_probe_runs_that_wrap(pie, gpu_ctx):
    """1 024 slots; forty keys whose home is one of the last four slots: their probe runs cross the end of the table"""
    ctx = gpu_ctx
    n, log2_slots = 400, 10
    cols = columns(41, n)
    ctx.load_columns(*cols, U)
    model = TurnModel(*cols)
    pool = random_keys(42, 200_000)
    homes = pie.token_homes(pool, log2_slots)
    tail, head = pool[homes >= (1 << log2_slots) - 4], pool[homes == 0]
    assert tail.shape[0] >= 80 and head.shape[0] >= 80
    keys = random_keys(43, n)
    keys[:40], keys[40:80] = tail[:40], head[:40]
    ctx.token_set(keys)
    model.token_set(keys)
    cov, slots, slot_row, back = ctx.token_layout()
    assert cov == n and slots == 1 << log2_slots
    slot_of = check_layout(cov, slots, slot_row, back, pie.token_homes(back, log2_slots))
    assert np.any(slot_of[:40] < pie.token_homes(keys[:40], log2_slots)), "the run crosses the end"
    rng = np.random.default_rng(44)
    absent = np.concatenate([tail[40:80], head[40:80]])                     # other keys, the same homes: the whole run is walked
    ask = np.concatenate([keys[:80], absent, keys[:80]])[rng.permutation(240)]
    ops = make_ops(ask, NOW + rng.integers(-10 ** 8, 10 ** 8, 240), rng.choice([GET, TOUCH, DELETE], 240, p=[0.4, 0.4, 0.2]))
    ops["new_end"] = NOW + rng.integers(1, 10 ** 9, 240)
    got = run_turn(ctx, model, ops)
    assert np.count_nonzero(got["row"] >= 0) >= 120 and np.all(got["row"][np.isin(ask[:, 0], absent[:, 0])] == -1)
    columns_match(ctx, model)


@pytest.mark.parametrize("mode", ["hot", "ordered"])
def test_derived_state_behind_a_turn(pie, oracle, mode):
    """a turn that moves rows into and out of the hot range and deletes others, followed at once by a single scan, a 16-query
    batch and a wide batch: each equals the oracle on the model's columns"""
    n, users, discs = 20_000, 499, 32
    t0 = oracle.T0_MS
    cols = oracle.gen(0x5EED5EED + 5, n, 0, n, users, discs, 0)
    ctx = ctx_with_env(pie, mode == "hot", 1)
    try:
        if mode == "ordered":
            ctx.set_ordered_run(2)
        ctx.load_columns(*cols, users)
        model = TurnModel(*cols)
        keys = random_keys(51, n)
        ctx.token_set(keys)
        model.token_set(keys)
        lim = (1 << discs) - 1
        queries = [(t0 - 6 * HOUR - 977 * q - (q % 5) * HOUR, t0 - (61 + q % 4) * DAY, (0x55555555, 0xAAAAAAAA, lim)[q % 3]) for q in range(100)]

        def check(tag):
            now, cutoff, mask = queries[0]
            ctx.set_disciplines(mask, discs)
            single = ctx.scan(now, cutoff)
            ctx.set_disciplines(lim, discs)
            batch = ctx.scan_batch(queries[:16])
            wide = ctx.scan_wide(queries)
            want = [oracle.scan(model.start, model.end, model.user, model.disc, users, qn, qc, qm) for qn, qc, qm in queries]
            for a, b in zip(single, want[0]):
                assert np.array_equal(a, b), (tag, "single scan")
            for q in range(16):
                for a, b in zip(batch[q], want[q]):
                    assert np.array_equal(a, b), (tag, "batch", q)
            for q in range(100):
                for a, b in zip(wide[q], want[q]):
                    assert np.array_equal(a, b), (tag, "wide batch", q)

        check("built")
        if mode == "hot":
            info = ctx.table_info()
            assert info["hot_builds"] == 1 and info["hot_rows"] > 0
        else:
            ctx.set_disciplines(queries[0][2], discs)
            ctx.scan(queries[0][0], queries[0][1])
            assert ctx.stats()["k1_variant"] & 0x2000, "the ordered run was not used"
        rng = np.random.default_rng(52)
        top = np.argsort(model.end, kind="stable")[-250:]                   # the rows the queries find live, and some more
        low = np.nonzero((model.end < t0 - 30 * DAY) & (model.end != END_NONE))[0]
        assert np.count_nonzero(model.end[top] > queries[0][0]) >= 100 and low.size >= 300
        top, low = rng.permutation(top), rng.permutation(low)[:300]
        parts = [
            make_ops(keys[low[:150]], model.end[low[:150]] - 1, TOUCH, t0 + rng.integers(1, 12 * HOUR, 150)),     # into the hot range
            make_ops(keys[top[:100]], model.end[top[:100]] - 1, TOUCH, t0 - rng.integers(1, 20, 100) * DAY),                  # out of it
            make_ops(keys[top[100:200]], t0, DELETE),                                                              # deleted
            make_ops(keys[top[200:250]], model.end[top[200:250]] - 1, TOUCH, t0 + rng.integers(0, 6 * HOUR, 50)),                # up inside it
            make_ops(keys[low[150:200]], t0, TOUCH, t0 + HOUR),                                                    # expired: no-ops
            make_ops(keys[low[:40]], t0, GET),                                                                     # behind their touches: live
            make_ops(keys[top[:40]], t0 - 25 * DAY, TOUCH, t0 + 2 * HOUR),                                         # and back in again
            make_ops(keys[low[200:230]], model.end[low[200:230]] - 1, TOUCH, t0 + 3 * HOUR),
            make_ops(keys[low[200:230]], t0, DELETE),                                                              # touched, then deleted in the same turn
        ]
        ops = np.concatenate(parts)
        got = run_turn(ctx, model, ops, mode)
        live = got["live"]
        assert live[:250].all() and not live[250:350].any() and live[350:400].all() and not live[400:450].any()
        assert live[450:560].all() and not live[560:].any()
        assert np.all(got["end"][560:] == END_NONE) and np.all(model.end[low[200:230]] == END_NONE)
        check("behind the turn")                      # at once: nothing between the turn and the scans
        columns_match(ctx, model)
        if mode == "hot":
            info = ctx.table_info()
            assert info["hot_builds"] == 1 and info["hot_rows"] > 0, "the turn was mirrored: the index was neither dropped nor rebuilt"
        # tombstones back to life are not a turn's to make (a touch of a dead row is a no-op): a second turn on the changed table
        ops2 = np.concatenate([make_ops(keys[top[100:200]], t0 - DAY, TOUCH, t0 + HOUR), make_ops(keys[low[:150]], t0, DELETE)])
        got = run_turn(ctx, model, ops2, mode)
        assert not got["live"].any() and np.all(got["row"][100:] == low[:150])
        check("behind the second turn")
    finally:
        ctx.close()


def test_refusals(pie, gpu_ctx):
    ctx = gpu_ctx
    cols = columns(61)
    ctx.load_columns(*cols, U)
    keys = random_keys(62, N)
    ops = make_ops(keys[:4], NOW - 10 ** 9, TOUCH, NOW + 10 ** 9)

    def code(fn, *a):
        with pytest.raises(pie.PieError) as ei:
            fn(*a)
        return ei.value.code

    assert code(ctx.token_turn, ops) == PIE_E_STATE, "no token column"
    assert code(ctx.token_turn, ops[:0]) == PIE_E_STATE, "... whatever the size"
    ctx.token_set(keys)
    model = TurnModel(*cols)
    model.token_set(keys)
    mask = (1 << D) - 1
    ctx.set_disciplines(mask, D)
    ctx.scan_begin(NOW, 0)
    assert code(ctx.token_turn, ops) == PIE_E_STATE, "a single scan in flight"
    ctx.scan_finish()
    ctx.scan_batch_begin([(NOW, 0, mask), (NOW - HOUR, 0, 1)])
    assert code(ctx.token_turn, ops) == PIE_E_STATE, "a batch in flight"
    ctx.scan_batch_finish()
    columns_match(ctx, model)
    # bad arguments change nothing, wherever they stand in the turn
    bad_kind, bad_reserved = ops.copy(), ops.copy()
    bad_kind["kind"][3] = 3
    bad_reserved["reserved"][3] = 1
    assert code(ctx.token_turn, bad_kind) == PIE_E_INVAL and code(ctx.token_turn, bad_reserved) == PIE_E_INVAL
    bad_kind["kind"][3] = -1
    assert code(ctx.token_turn, bad_kind) == PIE_E_INVAL
    assert ctx._lib.pie_token_turn(ctx._ctx, None, 4, None, None, None, None, None) == PIE_E_INVAL
    columns_match(ctx, model)
    with pie.PieScan(0) as fresh:                    # no table at all
        assert code(fresh.token_turn, ops) == PIE_E_STATE
    # and the same ops, well formed, go through
    got = run_turn(ctx, model, ops)
    assert got["live"].all() and np.all(got["end"] == NOW + 10 ** 9)
    columns_match(ctx, model)
