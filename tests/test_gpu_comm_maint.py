"""GPU: a sharded table that ages behind the C-ABI communicator: pie_comm_prune_before, pie_comm_retention_purge / _tz and
pie_comm_compact_rows.  Each case runs in a fresh process (tests/comm_maint_worker.py) whose RCCL is the one-GPU stand-in
tests/stub_rccl.c, as tests/test_gpu_comm_delete_users.py does.  The reference of every list is the plain call on an unsharded
context that holds the same table; the retention lists are also the oracle's, and the numpy model keeps its tombstones."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_maint_worker.py")


def run_worker(case, timeout=300):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_lists_equal_the_unsharded_calls(pie, oracle):
    """Worlds 1, 2, 3, 5 on tables of 1, 1 000 and 50 000 rows with tombstones: the merged lists of the prune and of both
    retention purges equal the twin's and the oracle's, with source rank and source local row; the tables agree afterwards
    through the merged expired queue (read back column for column) and a gathered batch."""
    assert "lists ok" in run_worker("lists")


def test_merge_edges_and_a_list_on_one_shard(pie, oracle):
    """Merged lists of exactly 0, 1, 255, 256, 257 and 65 537 rows around the merge kernel's 256-thread block; every listed row
    on one shard."""
    assert "edges ok" in run_worker("edges")


def test_capacity_tombstones_and_keeps_the_list(pie, oracle):
    """cap = total - 1: PIE_E_CAPACITY, the total reported, everything tombstoned, the full list in pie_comm_queue_read."""
    assert "capacity ok" in run_worker("capacity")


def test_refused_calls_change_no_shard(pie, oracle):
    """While a pipelined step is uncollected every call returns PIE_E_STATE; a bad argument is refused by the checks: the
    shards' columns are the same before and after."""
    assert "refusal ok" in run_worker("refusal")


def test_compaction_keeps_global_rows(pie, oracle):
    """Prune, then pie_comm_compact_rows with and without PIE_COMPACT_SHRINK: kept_total is the model's live rows, N_g stays;
    then appends, touches of kept and dropped rows, pie_comm_delete_users, token lookups on a column set before the compaction,
    the merged expired queue and a gathered batch all answer as the model that keeps its tombstones."""
    assert "compact ok" in run_worker("compact")
