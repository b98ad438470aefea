"""GPU: a whole turn on sharded tables (pie_shard_token_turn, pie_comm_token_turn).  Each case runs in a fresh process
(tests/comm_token_turn_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c, so worlds above one run on one MI355X; the
model is the unsharded TurnModel of tests/turn_model.py, in global ids."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_token_turn_worker.py")


def run_worker(case, timeout):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_turns_across_shards_equal_the_unsharded_table(pie, oracle):
    """Worlds 1, 2, 3, 5: the same seeded turns through shard_token_turn on every shard and through PieComm.token_turn equal the
    unsharded TurnModel op for op (owner included); columns, merged expired queues and gathered feeds equal the model's."""
    assert "worlds ok" in run_worker("worlds", 300)


def test_refused_turns_change_no_shard(pie, oracle):
    """Refused while a pipelined step is uncollected; a bad op, or a turn one shard refuses, changes no shard."""
    assert "errors ok" in run_worker("errors", 120)
