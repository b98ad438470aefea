"""GPU: the global-id half of the C ABI against tests/shard_chain.ShardStoreModel, in long mixed chains on 1, 2, 3 and 5 sharded
contexts of one GPU — pie_shard_append_rows / _set_end / _delete_user(s), the sharded token column with its turns, lookups and
touches by token, pie_shard_prune_before / _retention_purge[_tz], the three in-flight shard forms and pie_compact_rows on single
shards, each in the state the others leave behind.  (tests/test_gpu_model.py and tests/test_gpu_store_chain.py are the chains over
the scan half and the session-store half, on plain contexts.)

test_shard_chains: seeded chains of 25 to 40 steps.  Every context is given the same call with the same arrays.  After every
mutator, on every rank: pie_shard_info, both maps, the columns bit for bit, the token layout (covered_g, covered_l, slots, keys,
the slot walk), the capacity, and the translation both ways on held, foreign, dropped and out-of-range rows; across ranks: the
lists ascend, are disjoint and unite to the unsharded list, n_kept sums to k, and the lookup of every key ever issued, merged by
the largest global row, equals the unsharded model's at two clocks.  Then a scan, a batch, a wide batch and the expired queue in
both forms on every rank against the oracle on that rank's view.  The model is the only source of expected values.
test_shard_chains_reached_every_state then requires every state of shard_chain.STATES; tests/test_shard_chain_cpu.py shows on the
model alone that the lists reach the ones a host can decide, execute every op in every world and skip few steps."""
import pytest

import shard_chain as S
from test_shard_chain_cpu import LOGIN_SEEDS, SEEDS

pytestmark = pytest.mark.gpu

REACHED = {}   # chain -> the states it recorded; filled by the chain tests, read by the test after them


@pytest.mark.parametrize("seed", SEEDS)
def test_shard_chains(pie, oracle, seed):
    ch = S.run_shard_chain(pie, oracle, seed)
    REACHED[seed] = dict(ch.states)
    print("seed %d world %d: %.1f s, reached %s" % (seed, ch.world, ch.seconds, sorted(ch.states)))


@pytest.mark.parametrize("name", sorted(S.DESIGNED))
def test_designed_shard_chains(pie, oracle, name):
    """fixed op lists through the same machinery, for the states the hot index and the ordered run decide"""
    ch = S.run_designed(pie, oracle, name)
    REACHED[name] = dict(ch.states)
    print("chain %s world %d: %.1f s, reached %s" % (name, ch.world, ch.seconds, sorted(ch.states)))


def test_shard_chains_reached_every_state():
    missing = [s for s in SEEDS + sorted(S.DESIGNED) if s not in REACHED]
    assert not missing, "chains %s failed or were deselected: their records are missing, run the whole file" % missing
    by_state = {state: sorted((c for c, r in REACHED.items() if state in r), key=str) for state in S.STATES}
    print("states reached:", by_state)
    assert not [s for s in S.STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.STATES if not by_state[s]]


LOGINS_REACHED = {}


@pytest.mark.parametrize("seed", LOGIN_SEEDS)
def test_shard_login_chains(pie, oracle, seed):
    """the same mix with pie_shard_session_turn among it (users as global ids, some of them new, in-order logins), the plan's four
    outputs per rank against the model's restatement, pie_set_turn_ordered drawn per chain"""
    ch = S.run_shard_chain(pie, oracle, seed, {"logins": 1})
    LOGINS_REACHED["login seed %d" % seed] = dict(ch.states)
    print("login seed %d world %d: %.1f s, reached %s" % (seed, ch.world, ch.seconds, sorted(s for s in ch.states if s in S.LOGIN_STATES)))


@pytest.mark.parametrize("name", sorted(S.DESIGNED_LOGINS))
def test_designed_shard_login_chains(pie, oracle, name):
    ch = S.run_designed_logins(pie, oracle, name)
    LOGINS_REACHED["login " + name] = dict(ch.states)
    print("chain %s world %d: %.1f s, reached %s" % (name, ch.world, ch.seconds, sorted(s for s in ch.states if s in S.LOGIN_STATES)))


def test_shard_login_chains_reached_every_state():
    want = ["login seed %d" % s for s in LOGIN_SEEDS] + ["login " + n for n in sorted(S.DESIGNED_LOGINS)]
    missing = [c for c in want if c not in LOGINS_REACHED]
    assert not missing, "chains %s failed or were deselected: their records are missing, run the whole file" % missing
    by_state = {state: sorted(c for c, r in LOGINS_REACHED.items() if state in r) for state in S.LOGIN_STATES}
    print("states reached:", by_state)
    assert not [s for s in S.LOGIN_STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.LOGIN_STATES if not by_state[s]]
