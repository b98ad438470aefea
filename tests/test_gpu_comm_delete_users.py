"""GPU: pie_comm_delete_users, deleteSessionsForUser for a set of users on a live sharded table behind the C-ABI communicator.
Each case runs in a fresh process (tests/comm_delete_users_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c,
as tests/test_gpu_comm_mutate.py does; the model is the unsharded table deleted id by id in numpy."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_delete_users_worker.py")


def run_worker(case, timeout):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_merged_list_counts_owners_and_what_follows(pie, oracle):
    """Worlds 1, 2, 3: the merged ascending list, the per-user counts and the owners equal the unsharded model's; the shards'
    columns, the merged expired and archive queues and every gathered feed afterwards equal the oracle's."""
    assert "worlds ok" in run_worker("worlds", 300)


def test_refused_calls_change_no_shard(pie, oracle):
    """Refused while a pipelined step is uncollected, and when one shard refuses: no shard changes."""
    assert "errors ok" in run_worker("errors", 300)
