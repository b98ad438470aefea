"""GPU: the session-store half of the C ABI against tests/store_chain.StoreModel, in long mixed chains — the token column and its
index, pie_token_turn / pie_session_turn, turns, lookups and the purge tick begun while batches are in flight, pie_delete_users and
compaction that carries the keys over, each in the state the others leave behind.  (tests/test_gpu_model.py is the chain over the
scan half: set_end, appends, prune, retention and shards against scans, batches, wide batches and the queues, with no token column.)

test_store_chains: seeded chains of 30 to 50 steps on a context of their own (the capacities are the table's).  After every
mutator the columns are read back bit for bit, table_info's covered count, capacity and build count are compared with the model's,
and the index's layout is checked; then every key ever issued is looked up, and a scan and a batch are compared with the oracle on
the model's columns.  The model is the only source of expected values.  test_store_chains_reached_every_state then requires that
the chains arrived at every state of store_chain.STATES; tests/test_store_chain_cpu.py shows on the model alone that the seed list
reaches the ones a host can decide."""
import pytest

import store_chain as S
from test_store_chain_cpu import LOGIN_SEEDS, SEEDS

pytestmark = pytest.mark.gpu

REACHED = {}   # chain -> the states it recorded; filled by the chain tests, read by the test after them
LOGINS_REACHED = {}


@pytest.mark.parametrize("seed", SEEDS)
def test_store_chains(pie, oracle, seed):
    ch = S.run_store_chain(pie, oracle, seed)
    REACHED[seed] = dict(ch.states)
    print("seed %d reached %s" % (seed, sorted(ch.states)))


@pytest.mark.parametrize("name", sorted(S.DESIGNED))
def test_designed_store_chains(pie, oracle, name):
    """fixed op lists through the same machinery, for the states the hot index and the ordered run decide"""
    ch = S.run_designed(pie, oracle, name)
    REACHED[name] = dict(ch.states)
    print("chain %s reached %s" % (name, sorted(ch.states)))


def test_store_chains_reached_every_state():
    missing = [s for s in SEEDS + sorted(S.DESIGNED) if s not in REACHED]
    assert not missing, "chains %s failed or were deselected: their records are missing, run the whole file" % missing
    by_state = {state: sorted((c for c, r in REACHED.items() if state in r), key=str) for state in S.STATES}
    print("states reached:", by_state)
    assert not [s for s in S.STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.STATES if not by_state[s]]


@pytest.mark.parametrize("seed", LOGIN_SEEDS)
def test_login_chains(pie, oracle, seed):
    """the same mix with turns that log in in time order among it, pie_set_turn_ordered drawn per chain: the run's bookkeeping is
    decided on the host after every creating turn (StoreChain.check_run_after_logins)"""
    ch = S.run_store_chain(pie, oracle, seed, {"logins": 1})
    LOGINS_REACHED["login seed %d" % seed] = dict(ch.states)
    print("login seed %d reached %s" % (seed, sorted(ch.states)))


@pytest.mark.parametrize("name", sorted(S.DESIGNED_LOGINS))
def test_designed_login_chains(pie, oracle, name):
    ch = S.run_designed_logins(pie, oracle, name)
    LOGINS_REACHED["login " + name] = dict(ch.states)
    print("chain %s reached %s" % (name, sorted(ch.states)))


def test_login_chains_reached_every_state():
    want = ["login seed %d" % s for s in LOGIN_SEEDS] + ["login " + n for n in sorted(S.DESIGNED_LOGINS)]
    missing = [c for c in want if c not in LOGINS_REACHED]
    assert not missing, "chains %s failed or were deselected: their records are missing, run the whole file" % missing
    by_state = {state: sorted(c for c, r in LOGINS_REACHED.items() if state in r) for state in S.LOGIN_STATES}
    print("states reached:", by_state)
    assert not [s for s in S.LOGIN_STATES if not by_state[s]], "no chain arrived at %s" % [s for s in S.LOGIN_STATES if not by_state[s]]
