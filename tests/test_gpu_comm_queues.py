"""GPU: cross-shard dispatch queues behind the C ABI (pie_comm_expired_queue / pie_comm_archive_queue).  Each case runs in a
fresh process (tests/comm_queue_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c, so worlds above one run on
one MI355X; every merged queue is checked against the oracle's queue of the unsharded table."""
import os
import shutil
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_queue_worker.py")


def run_worker(case, timeout):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_merged_queues_equal_the_unsharded_queues(pie, oracle):
    """Worlds 1, 2, 3, 5 (a rank without rows): expired and archive windows, after touches and tombstones, sources, the copy
    every local rank holds, the capacity error and its repeat."""
    assert "worlds ok" in run_worker("worlds", 900)


def test_queue_errors_are_the_same_on_every_rank(pie, oracle):
    """Refused while a pipelined step is uncollected; a shard with rows outside its map fails every rank with PIE_E_STATE."""
    assert "errors ok" in run_worker("errors", 600)


def test_expired_queue_at_the_merge_block_edges(pie, oracle):
    """Worlds 3 and 5 (a rank without rows) over 20 000 rows: windows cut from the sorted end column so that the merged queue
    holds exactly 0, 1, 255, 256, 257 and 4 097 rows, and one whose rows all sit on one shard.  Each equals the oracle's queue
    of the unsharded table, its sources name the same global rows on their shards' maps, and the in-flight form on the same
    communicator (cap_rows = the total) returns the same rows and owners."""
    assert "edges ok: 14 windows" in run_worker("edges", 300)


def test_config5_sharded_queues(pie, oracle):
    """BASELINE config 5 shape: 8 shards of 10^8 sessions / 10^5 users on one GPU, one expired and one archive queue."""
    assert "cfg5 ok" in run_worker("cfg5", 1500)


def test_world_one_through_the_real_rccl(pie, oracle):
    out = run_worker("real", 600)
    if out.startswith("skip:"):
        pytest.skip(out.strip())
    assert "real ok" in out


@pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed on this machine")
def test_node_sharded_dispatch(pie):
    """host/shardedQueue.js over a world-3 communicator (stub RCCL, GPU 0): dispatchExpiredSessions / dispatchArchivedGroups
    give the summaries and payloads of a single-context source over the same unsharded table."""
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    stub_dir = os.path.join(REPO, "tests", "_stub")
    os.makedirs(stub_dir, exist_ok=True)
    stub = os.path.join(stub_dir, "libstub_rccl.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True)
    env = dict(os.environ, PIE_RCCL_LIB=stub)
    res = subprocess.run([shutil.which("node"), os.path.join(REPO, "sph-pie_amd", "host", "test", "comm_queue_test.js")], cwd=REPO, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "host comm_queue_test ok" in res.stdout
