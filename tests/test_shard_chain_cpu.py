"""CPU: tests/shard_chain.py on the model alone.
  1. ShardStoreModel replays the recorded reference trace G5 in worlds 1, 2, 3 and 5, a login being an append by global id and a
     token append, every other run of ops a turn on every rank merged by the largest row: the 1 345 recorded answers.
  2. Every seed of tests/test_gpu_shard_chain.py's list runs with no device: ShardChain(None, ...) makes the very draws the GPU
     run makes.  After every step the union of the rank views is the unsharded table less the dropped rows, and the merged
     per-rank lookup of every key equals StoreModel.lookup (ShardChain.readers); the cached per-rank lookup is held against
     tests/shard_token_model.ShardTokenModel's own.
  3. The conditions that keep the GPU test from passing by never arriving anywhere: the seed list reaches every state a host can
     decide, every op kind is executed (not skipped) in every world, no chain skips more than a quarter of its steps.
  4. Every chain logs the op it drew at each step and the sizes it met; the lines equal tests/golden/shard_chain_oplog.txt,
     recorded before the session-store chains learned to log in: whatever is added beside these chains moves no draw of theirs."""
import os

import numpy as np
import pytest

import shard_chain as S
from conftest import GOLDEN
from session_turn_model import replay_g5_sessions
from shard_token_model import ShardTokenModel
from trace_replay import load_trace
from turn_model import g5_key

# Chosen here, on the model: together with the designed scripts they meet the three conditions of (3).
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 17, 18]

# ... and the chains that log in through pie_shard_session_turn (cfg["logins"])
LOGIN_SEEDS = [8, 5, 10, 12, 22, 14, 1]

RAN = {}
LOGINS_RAN = {}


class Checked(S.ShardChain):
    """the chain with the model's own consistency checked after every step"""

    def readers(self, tag):
        super().readers(tag)
        sm, tm = self.sm, self.sm.tm
        gone = sm.gone
        views = [sm.view(r) for r in range(self.world)]
        rows = np.concatenate([v[1] for v in views])
        order = np.argsort(rows, kind="stable")
        assert np.array_equal(rows[order], np.nonzero(~gone)[0]), (tag, "the rank views are not the table less the dropped rows")
        for name, whole in (("start", tm.start), ("end", tm.end), ("disc", tm.disc)):
            assert np.array_equal(np.concatenate([getattr(v[0], name) for v in views])[order], whole[~gone]), (tag, name)
        users = np.concatenate([v[2][v[0].user] if v[1].size else np.zeros(0, np.int32) for v in views])
        assert np.array_equal(users[order], tm.user[~gone]), (tag, "user")
        for r, (v, held, ids) in enumerate(views):
            assert np.array_equal(held, sm.held(r)) and np.all(np.diff(held) > 0) and v.U == max(ids.size, 1)
            assert np.array_equal(ids, sm.users_of(r)) and sm.covered_l(r) <= held.size <= sm.cap[r]
            assert sm.slots[r] >= S.slots_for(0) and (held.size <= sm.slots[r] // 2 or sm.covered_l(r) <= sm.slots[r] // 2)
        if self.step % 5 == 0:      # the cached per-rank index against ShardTokenModel's own lookup
            keys = np.concatenate([self.issued[-300:], self.issued[:50], self.absent[:5]])
            now = int(np.median(tm.end))            # (no draw here: the GPU run must see the same stream)
            for r in range(self.world):
                a, b = sm.shard_lookup(r, keys, now), ShardTokenModel.shard_lookup(sm, r, keys, now)
                assert all(np.array_equal(a[c], b[c]) for c in a), (tag, "rank", r, "the cached index")


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("chunk", [None, 7])
def test_shard_store_model_replays_g5(oracle, world, chunk):
    trace = load_trace(GOLDEN)
    store = S.ShardModelStore(oracle, len(trace["users"]), world)
    checked, turns, largest, mixed = replay_g5_sessions(trace, store, chunk)
    assert checked == 1345 and largest <= (chunk or 10 ** 9) and mixed > 300
    sm = store.sm
    assert sm.N == sm.covered_g == trace["sessions"] == 659
    assert sum(sm.held(r).size for r in range(world)) == 659 and sum(sm.covered_l(r) for r in range(world)) == 659
    keys = np.stack([g5_key(t) for t in range(659)])
    assert S.merge([sm.shard_lookup(r, keys, 0) for r in range(world)])["row"].tolist() == list(range(659))
    if world == 1:
        assert sm.slots == [2048] and 659 <= sm.cap[0] < 2 * 659, "the slots doubled once, by the append after the 513th row"


@pytest.mark.parametrize("seed", SEEDS)
def test_shard_chain_on_the_model_alone(oracle, seed):
    ch = Checked(None, oracle, seed).run()
    steps = ch.cfg["steps"]
    assert ch.sm.N <= S.MAX_ROWS
    assert ch.skipped * 4 <= steps, "the chain skipped %d of its %d steps" % (ch.skipped, steps)
    RAN[seed] = (ch.world, dict(ch.states), dict(ch.executed))


@pytest.mark.parametrize("name", sorted(S.DESIGNED))
def test_designed_chain_on_the_model_alone(oracle, name):
    cfg, script = S.DESIGNED[name]
    ch = Checked(None, oracle, 9100 + sorted(S.DESIGNED).index(name), cfg, script).run()
    assert ch.skipped == 0
    RAN[name] = (ch.world, dict(ch.states), dict(ch.executed))
    want = {"hot": ["inflight_turn_after_reshape"], "ordered": ["host:turn_begin_in_ordered_chain", "compact_one_rank_then_delete_users"],
            "reshape": ["compact_shrink_then_burst_append", "capacity_outgrown_under_lookup_begun", "token_append_after_compact_with_uncovered_tail",
                        "touch_of_dropped_row", "duplicate_key_resolved_by_merge", "maint_list_over_cap"],
            "empty_rank": ["first_user_of_empty_rank", "user_without_rows_then_deleted", "slots_doubled_on_one_rank_only"]}[name]
    assert not [s for s in want if s not in ch.states], (sorted(ch.states), want)


def test_the_lists_meet_the_conditions():
    missing = [s for s in SEEDS + sorted(S.DESIGNED) if s not in RAN]
    assert not missing, "chains %s failed or were deselected: run the whole file" % missing
    by_state = {s: sorted((c for c, r in RAN.items() if s in r[1]), key=str) for s in S.HOST_STATES}
    print("states reached on the model:", by_state)
    assert not [s for s in S.HOST_STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.HOST_STATES if not by_state[s]]
    assert set(S.DEVICE_STATES) | set(S.HOST_STATES) >= set(S.STATES)
    seeded = {c: r for c, r in RAN.items() if c in SEEDS}
    assert {r[0] for r in seeded.values()} == {1, 2, 3, 5}, "the seeds do not cover worlds 1, 2, 3 and 5"
    for world in (1, 2, 3, 5):
        done = set()
        for w, _, executed in RAN.values():
            if w == world:
                done |= set(executed)
        assert not set(S.ShardChain.OPS) - done, "world %d never executed %s" % (world, sorted(set(S.ShardChain.OPS) - done))


def test_old_seeds_replay_line_for_line(oracle):
    """(tag, N, U, covered, slots, cap) of every step of every chain from before the logins, model only, as recorded"""
    lines = []
    for seed in SEEDS:
        S.run_shard_chain(None, oracle, seed, log=lines.append)
    for name in sorted(S.DESIGNED):
        cfg, script = S.DESIGNED[name]
        S.run_shard_chain(None, oracle, 9100 + sorted(S.DESIGNED).index(name), cfg, script, log=lines.append)
    with open(os.path.join(GOLDEN, "shard_chain_oplog.txt")) as f:
        want = f.read().splitlines()
    assert len(lines) == len(want)
    assert lines == want, next((a, b) for a, b in zip(lines, want) if a != b)


@pytest.mark.parametrize("seed", LOGIN_SEEDS)
def test_login_chain_on_the_model_alone(oracle, seed):
    ch = Checked(None, oracle, seed, {"logins": 1}).run()
    steps = ch.cfg["steps"]
    assert ch.cfg["n"] <= 4099 and ch.cfg["U"] <= 64 and ch.sm.N <= S.MAX_ROWS
    assert ch.skipped * 10 <= steps, "the chain skipped %d of its %d steps" % (ch.skipped, steps)
    LOGINS_RAN[seed] = (ch.world, dict(ch.states), dict(ch.executed))


@pytest.mark.parametrize("name", sorted(S.DESIGNED_LOGINS))
def test_designed_login_chain_on_the_model_alone(oracle, name):
    cfg, script = S.DESIGNED_LOGINS[name]
    ch = Checked(None, oracle, 9300 + sorted(S.DESIGNED_LOGINS).index(name), cfg, script).run()
    assert ch.skipped == 0
    LOGINS_RAN[name] = (ch.world, dict(ch.states), dict(ch.executed))
    want = {"empty_rank": ["shard_create_first_user_of_empty_rank", "shard_create_kept_by_no_live_rank_row"],
            "slots": ["shard_create_doubled_slots_on_one_rank", "shard_create_after_one_rank_compacted"]}[name]
    assert not [s for s in want if s not in ch.states], (sorted(ch.states), want)


def test_the_login_lists_meet_the_conditions():
    missing = [s for s in LOGIN_SEEDS + sorted(S.DESIGNED_LOGINS) if s not in LOGINS_RAN]
    assert not missing, "chains %s failed or were deselected: run the whole file" % missing
    by_state = {s: sorted((c for c, r in LOGINS_RAN.items() if s in r[1]), key=str) for s in S.LOGIN_HOST_STATES}
    print("states the login chains reached on the model:", by_state)
    assert not [s for s in S.LOGIN_HOST_STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.LOGIN_HOST_STATES if not by_state[s]]
    seeded = {c: r for c, r in LOGINS_RAN.items() if c in LOGIN_SEEDS}
    assert {r[0] for r in seeded.values()} == {1, 2, 3, 5}, "the seeds do not cover worlds 1, 2, 3 and 5"
    for world in (1, 2, 3, 5):
        done = set()
        for w, _, executed in seeded.values():
            if w == world:
                done |= set(executed)
        assert not set(S.ShardChain.NEW_OPS) - done, "world %d never executed %s" % (world, sorted(set(S.ShardChain.NEW_OPS) - done))


def test_world_five_starts_with_an_empty_rank(oracle):
    cfg = S.shard_config(next(s for s in SEEDS if S.shard_config(s)["world"] == 5))
    assert cfg["U"] == 7 and [r for r in range(5) if all(oracle.shard_of(u, 5) != r for u in range(7))]


def test_mirrored_sizes_follow_the_library(pie):
    for rows in (0, 1, 511, 512, 513, 1024, 1025, 20000, 40000):
        assert S.slots_for(rows) == pie.token_slots_for(rows), rows
