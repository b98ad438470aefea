"""GPU: a live sharded table behind the C-ABI communicator (pie_comm_append_rows / pie_comm_set_end / pie_comm_delete_user).
Each case runs in a fresh process (tests/comm_mutate_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c, so
worlds above one run on one MI355X; the model is the unsharded table mutated in numpy."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_mutate_worker.py")


def run_worker(case, timeout):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_queues_and_feeds_after_mutations_by_global_id(pie, oracle):
    """Worlds 1, 2, 3, 5: after appends (new users included), touches and deletes through the communicator the merged expired
    and archive queues equal the oracle's queues of the mutated unsharded table, sources included, and every gathered feed
    (u_pad = 0) equals the oracle's.  Before these calls existed every queue call after an append returned PIE_E_STATE."""
    assert "worlds ok" in run_worker("worlds", 600)


def test_refused_calls_change_no_shard(pie, oracle):
    """Refused while a pipelined step is uncollected; a call one shard refuses changes none of them."""
    assert "errors ok" in run_worker("errors", 600)
