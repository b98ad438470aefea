"""GPU: the cross-shard archive queue at the boundaries of its merge (k_merge_archive: one wave per group, four groups per block,
a lane per rank).  One fresh process per world (tests/comm_archive_worker.py, RCCL replaced by the one-GPU stand-in
tests/stub_rccl.c) runs the designed shapes of archive_cases.py: 0, 1, 3, 4, 5 and 8 193 qualifying groups dealt to the ranks in
turn, a rank without rows, a rank with rows and no qualifying group, every group on one rank, groups of 63 / 64 / 65 rows, and one
group that holds most rows."""
import os
import subprocess
import sys

import pytest

import archive_cases as AC
from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_archive_worker.py")


@pytest.mark.parametrize("world", AC.COMM_WORLDS)
def test_merged_archive_queue_on_designed_shapes(pie, oracle, world):
    res = subprocess.run([sys.executable, WORKER, str(world)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "world %d ok: %d shapes" % (world, len(AC.comm_names(world))) in res.stdout
