"""GPU: the wide pipelined exchange of the C-ABI communicator (pie_comm_wide_step_*) with world > 1 — a fresh process whose
RCCL is the stand-in of tests/stub_rccl.c drives `world` shards on GPU 0 (tests/comm_wide_stub_worker.py): the warm-up step
without a union, the overflow every rank sees at collect, pipelined steps of 512 / 300 / 65 queries with rotating buffer sets,
every global feed against the oracle's scan of the unsharded table, wide_step_read_feed, and the mutual exclusion with the
ordinary steps."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world,n,U", [(3, 300_000, 3001), (2, 1 << 20, 10 ** 4), (3, 300_000, 101)])
def test_wide_steps_with_several_ranks(pie, oracle, world, n, U):
    """On the first two tables the oracle's answers show that no user's union of the 512 queries exceeds 16 rows, so every
    shard keeps its union from the first step on; the third table (about 3000 rows per user) is the one whose first wide steps
    outgrow the union slots and report Mu = -1 before the slot capacity has grown."""
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "comm_wide_stub_worker.py"), str(world), str(n), str(U)] + (["no-union"] if U == 101 else []),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900, cwd=REPO)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "comm wide stub ok" in res.stdout
