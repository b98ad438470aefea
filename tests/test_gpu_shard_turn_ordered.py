"""GPU: turns that log in keep the ordered run on sharded tables and behind the communicator (pie_set_turn_ordered on every shard's
context, pie_comm_session_turn).  Every case runs tests/comm_turn_ordered_worker.py in a fresh process whose "RCCL" is the compiled
tests/stub_rccl.c: worlds 1, 2, 3 and 5 on one GPU, the oracle on every shard's own rows and a twin communicator driven by the
one-by-one pie_comm_* sequence."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "comm_turn_ordered_worker.py")


@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_shards_keep_their_runs_through_a_turn_with_creates(world):
    res = subprocess.run([sys.executable, WORKER, str(world)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "turn_ordered ok: world %d" % world in res.stdout, res.stdout[-4000:]
