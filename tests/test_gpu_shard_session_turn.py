"""GPU: the turn that logs in on sharded tables and behind the communicator (pie_shard_session_turn, pie_comm_session_turn;
k_session_turn<true> in sph-pie_amd/csrc/pie_token.h).  Every case runs tests/comm_session_turn_worker.py in a fresh process whose
"RCCL" is the compiled tests/stub_rccl.c: worlds 1, 2, 3 and 5 on one GPU.  The model is tests/shard_chain.py's ShardModelStore and,
per rank, a second set of contexts driven by the one-by-one sequence of existing calls that the header defines the turn by."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "comm_session_turn_worker.py")


def run_worker(*args):
    res = subprocess.run([sys.executable, WORKER, *[str(a) for a in args]], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and args[0] + " ok" in res.stdout, res.stdout[-4000:]
    return res.stdout


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_g5_through_the_communicator(world):
    """(a) the reference's own answers, recorded call by call, from turns of 1, 7, 64 and whole runs that carry the logins"""
    run_worker("g5", world)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_twin_of_the_one_by_one_sequence(world):
    """(b) seeded mixed turns: shard_session_turn on one set of contexts, the one-by-one sequence on a second, compared per rank"""
    run_worker("twin", world)


def test_shapes_and_a_two_shard_key():
    """(c), (f)"""
    run_worker("shapes")


def test_room_on_one_rank_and_a_turn_after_a_compaction():
    """(e)"""
    run_worker("room")


def test_probe_runs_that_wrap_and_slots_claimed_in_the_launch_on_one_shard():
    """(d)"""
    run_worker("wrap")


def test_hot_index_and_ordered_run_behind_a_turn_with_creates():
    """(g) both asserted live and valid before the turns"""
    run_worker("derived")


def test_refusals_change_no_shard():
    """(h)"""
    run_worker("errors")
