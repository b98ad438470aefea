"""GPU: token lookups and the expired queue behind the C-ABI communicator while pipelined steps are in flight
(pie_comm_token_lookup_begin / _finish / _room, pie_comm_expired_queue_begin / _finish / _room).  Each case runs in a fresh process
(tests/comm_inflight_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c, so worlds above one run on one MI355X.  The
table has 40 000 rows; a shard's in-flight pass works in units of 16 384 rows, so worlds 1, 2, 3 and 5 give shards of three units
with a ragged last one, two units, and less than one unit.  The models are the unsharded TokenModel and the oracle."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_inflight_worker.py")
WORLDS = (1, 2, 3, 5)


def run_worker(args, timeout=120, env=None):
    res = subprocess.run([sys.executable, WORKER] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                         timeout=timeout, cwd=REPO, env=dict(os.environ, **(env or {})))
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


@pytest.mark.parametrize("world", WORLDS)
def test_lookups_with_ordinary_steps_in_flight(pie, oracle, world):
    """Three ordinary steps begun and uncollected; lookups of 0, 1, 64, 65 and 4096 keys with per-key clocks (present, absent,
    expired, tombstoned, duplicated, carried by rows of two shards); four begun before any finish, room 4 -> 0, a fifth refused,
    pie_comm_token_lookup refused meanwhile; finishes in begin order equal to TokenModel, owner included; the steps' gathered
    feeds equal the oracle afterwards."""
    assert "lookup ok" in run_worker(["lookup", world])


def test_lookups_with_wide_steps_in_flight(pie, oracle):
    """The same lookups with two wide steps in flight (world 3)."""
    assert "wide ok" in run_worker(["wide", 3])


@pytest.mark.parametrize("world", WORLDS)
def test_expired_queue_with_steps_in_flight(pie, oracle, world):
    """Windows: empty, hits on one shard only, the whole range of end, totals forced to 256 and 257 (the merge's block edge);
    cap_rows 0, the exact total and total - 1 (PIE_E_CAPACITY, the true prefix, *q_out the total); three ordinary steps in
    flight.  Rows equal pie_comm_expired_queue once drained and the oracle's queue; owner = pie_shard_of(user of the row)."""
    assert "expired ok" in run_worker(["expired", world])


def test_expired_queue_lists_brought_over(pie, oracle):
    """The same with every shard's list copied to the merging device first (PIE_COMM_STAGE_ALL=1): the path lists held on other
    devices take, on one GPU."""
    assert "expired ok" in run_worker(["expired", 3], env={"PIE_COMM_STAGE_ALL": "1"})


def test_refusals_and_destroy_with_work_begun(pie, oracle):
    """Finish with nothing begun; a second queue; a slot taken with pie_shard_token_lookup_begin on pie_comm_ctx(comm, 1): the
    communicator's begin returns PIE_E_STATE and every shard's room is unchanged; cap < k, then a successful finish; room below
    the begin's cap_rows; pie_comm_destroy with one lookup and one queue begun returns and the process exits 0."""
    assert "errors ok" in run_worker(["errors"])
