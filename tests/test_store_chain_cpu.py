"""CPU: tests/store_chain.py on the model alone.
  1. StoreModel — SessionTurnModel and the table model on one set of columns — replays the recorded reference trace G5 with the
     logins inside the turns, in turns of every size: the 1 345 recorded answers.
  2. Every seed of tests/test_gpu_store_chain.py's list runs with no device: StoreChain(None, ...) makes the very draws the GPU
     run makes, so what the model alone arrives at the GPU run arrives at too.  After every compaction the chain checks that a
     lookup of every issued key equals the answer before it pushed through new_of_old (StoreChain.do_compact).
  3. The seed list reaches every state that can be decided without a device — the cap that keeps the GPU test from passing by
     never arriving anywhere — and the two sizes the model mirrors follow the library's own host-side rules.
  4. The chains that log in under pie_set_turn_ordered (cfg["logins"]) are chains of their own: the old seeds, replayed with a
     log, draw line for line what they drew before those chains existed (tests/golden/store_chain_oplog.txt); the new seed list
     reaches every stand-in state of S.LOGIN_HOST_STATES and skips at most a tenth of its steps."""
import os

import numpy as np
import pytest

import store_chain as S
from conftest import GOLDEN
from session_turn_model import CREATE, replay_g5_sessions
from trace_replay import load_trace
from turn_model import GET, g5_key, make_ops

# Chosen here, on the model: together they reach every state of S.HOST_STATES (test_seed_list_reaches_every_host_state).
SEEDS = [41, 26, 4, 11, 3, 8, 30, 42, 49, 6, 16, 60]

# ... and the chains that log in (cfg["logins"]): every S.LOGIN_HOST_STATES between them, at most a tenth of the steps skipped
LOGIN_SEEDS = [2, 3, 5, 9, 16, 17, 20, 0]

REACHED = {}
LOGINS_RAN = {}


@pytest.mark.parametrize("chunk", [None, 64, 7, 1])
def test_store_model_replays_g5(oracle, chunk):
    trace = load_trace(GOLDEN)
    store = S.StoreModelStore(oracle, len(trace["users"]))
    checked, turns, largest, mixed = replay_g5_sessions(trace, store, chunk)
    assert checked == 1345 and largest <= (chunk or 10 ** 9) and (chunk == 1 or mixed > 300)
    m = store.m
    assert m.n == m.covered == trace["sessions"] == 659
    assert m.rows_of(np.stack([g5_key(t) for t in range(659)])).tolist() == list(range(659))
    assert m.slots == S.slots_for(659) == 2048 and m.builds == 1, "the slots doubled once, when the 513th session logged in"
    assert 659 <= m.cap < 2 * 659


@pytest.mark.parametrize("seed", SEEDS)
def test_store_chain_on_the_model_alone(oracle, seed):
    ch = S.run_store_chain(None, oracle, seed)
    assert ch.m.n <= S.MAX_ROWS and ch.m.covered + (0 if ch.pending is None else len(ch.pending)) == ch.m.n
    REACHED[seed] = dict(ch.states)


@pytest.mark.parametrize("name", sorted(S.DESIGNED))
def test_designed_chain_on_the_model_alone(oracle, name):
    ch = S.run_designed(None, oracle, name)
    want = {"hot": "inflight_turn_after_reshape", "ordered": "host:creating_turn_in_ordered_chain"}[name]
    assert want in ch.states, sorted(ch.states)


def test_seed_list_reaches_every_host_state():
    missing = [s for s in SEEDS if s not in REACHED]
    assert not missing, "chains %s failed or were deselected: run the whole file" % missing
    seen = {}
    for r in REACHED.values():
        for state, k in r.items():
            seen[state] = seen.get(state, 0) + k
    print("states reached on the model:", {s: sorted(seed for seed, r in REACHED.items() if s in r) for s in S.HOST_STATES})
    assert not [s for s in S.HOST_STATES if not seen.get(s)], "no chain arrived at %s" % [s for s in S.HOST_STATES if not seen.get(s)]
    assert set(S.DEVICE_STATES) | set(S.HOST_STATES) >= set(S.STATES)


def test_mirrored_sizes_follow_the_library(pie, oracle):
    """pie_token_slots_for is the library's; the model's doubling points are the header's (covered > slots / 2)"""
    for covered in (0, 1, 511, 512, 513, 1024, 1025, 2048, 2049, 20000, 40000):
        assert S.slots_for(covered) == pie.token_slots_for(covered), covered
    z64, z32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    m = S.StoreModel(oracle, np.arange(500), np.arange(500) + 10, np.zeros(500, np.int32), np.zeros(500, np.int32), 1, 1)
    keys = np.random.default_rng(1).integers(0, 2 ** 64, (540, 2), dtype=np.uint64)
    m.token_set(keys[:500])
    assert (m.slots, m.builds, m.cap) == (1024, 0, 500)
    m.turn(make_ops(keys[500:512], 5, CREATE, 9), np.zeros(12, np.int32), np.zeros(12, np.int32))
    assert (m.slots, m.builds, m.cap) == (1024, 0, 1000), "512 covered rows still fit 1 024 slots; the columns doubled"
    m.turn(make_ops(keys[512:513], 5, CREATE, 9), np.zeros(1, np.int32), np.zeros(1, np.int32))
    assert (m.slots, m.builds, m.cap) == (2048, 1, 1000)
    m.end[:300] = S.END_NONE
    assert m.compact(S.END_NONE, shrink=True).tolist() == [-1] * 300 + list(range(213))
    assert (m.slots, m.builds, m.cap, m.covered) == (1024, 2, 213, 213)
    assert m.turn(make_ops(keys[300:301], 5, GET))["row"].tolist() == [0]
    assert np.array_equal(m.compact(S.END_NONE, shrink=True), np.arange(213)) and m.builds == 2, "nothing to drop, nothing to give back"


def test_old_seeds_replay_line_for_line(oracle):
    """every chain from before the logins, model only: the op drawn at each step and the sizes it met (tag, n, covered, slots,
    cap) are the recorded ones, so no new op name or config key has moved a draw of theirs"""
    lines = []
    for seed in SEEDS:
        S.run_store_chain(None, oracle, seed, log=lines.append)
    for name in sorted(S.DESIGNED):
        cfg, script = S.DESIGNED[name]
        S.run_store_chain(None, oracle, 9000 + sorted(S.DESIGNED).index(name), cfg, script, log=lines.append)
    with open(os.path.join(GOLDEN, "store_chain_oplog.txt")) as f:
        want = f.read().splitlines()
    assert len(lines) == len(want) == 525
    assert lines == want, next((a, b) for a, b in zip(lines, want) if a != b)


@pytest.mark.parametrize("seed", LOGIN_SEEDS)
def test_login_chain_on_the_model_alone(oracle, seed):
    ch = S.run_store_chain(None, oracle, seed, {"logins": 1})
    c = ch.cfg
    assert c["n"] <= 4099 and c["U"] <= 64 and c["D"] <= 8 and ch.m.n <= S.MAX_ROWS
    assert ch.skipped * 10 <= c["steps"], "the chain skipped %d of its %d steps" % (ch.skipped, c["steps"])
    LOGINS_RAN[seed] = dict(ch.states)


@pytest.mark.parametrize("name", sorted(S.DESIGNED_LOGINS))
def test_designed_login_chain_on_the_model_alone(oracle, name):
    ch = S.run_designed_logins(None, oracle, name)
    assert ch.skipped == 0
    want = {"kept": ["host:login_in_order_switch_on", "host:login_grew_switch_on", "host:login_full_segment", "host:login_chain_of_one_user",
                     "host:login_create_then_delete", "host:login_since_compact_shrink", "host:login_since_compact_noshrink",
                     "host:login_before_top", "host:begin_after_login", "create_over_foreign_tombstone"],
            "far": ["host:login_before_top", "host:login_in_order_switch_on"], "hot": ["host:login_in_order_switch_on", "host:begin_after_login"],
            "off": ["host:login_in_order_switch_off", "host:begin_after_login"]}[name]
    assert not [s for s in want if s not in ch.states], (sorted(ch.states), want)


def test_login_seed_list_reaches_every_host_state():
    missing = [s for s in LOGIN_SEEDS if s not in LOGINS_RAN]
    assert not missing, "chains %s failed or were deselected: run the whole file" % missing
    by_state = {s: sorted(seed for seed, r in LOGINS_RAN.items() if s in r) for s in S.LOGIN_HOST_STATES + ("create_over_foreign_tombstone",)}
    print("states the login chains reached on the model:", by_state)
    assert not [s for s, seeds in by_state.items() if not seeds], "no chain arrived at %s" % [s for s, seeds in by_state.items() if not seeds]
    assert {S.logins_config(seed)["turn_ordered"] for seed in LOGIN_SEEDS} == {0, 1}, "the switch on and off"
