"""GPU: commPruneBefore, commRetentionPurge and commCompactRows through host/shardedQueue.js (pruneBefore, purgeRetention,
compact) with world 2 at 1 000 rows — a fresh node child with its own timeout runs sph-pie_amd/host/test/comm_maint_test.js on
GPU 0 through PIE_RCCL_LIB (tests/stub_rccl.c).  The expected lists are written here, from the oracle's copy of the table."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

HOST = os.path.join(REPO, "sph-pie_amd", "host")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None, reason="node is not installed on this machine")
ZONE = "America/New_York"   # one of tests/golden/addmonths_zones.json
INT64_MIN = -(2 ** 63)


@needs_node
@pytest.mark.gpu
def test_sharded_table_ages_through_the_node_host(pie, oracle, tmp_path):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    n, U = 1000, 7
    s, e, u, _ = (a.copy() for a in oracle.gen(0x5EED5EED, n, 0, n, U, 32, 0))
    cutoff = int(np.sort(s)[n // 10]) + 1
    now, months = oracle.T0_MS - oracle.SPAN_MS // 2 + 70 * 86400000, 2
    prune = np.nonzero(s < cutoff)[0]
    e[prune] = INT64_MIN
    retention = oracle.retention_queue_tz(s, e, now, months, *oracle.tz_table(ZONE))
    assert prune.size > 50 and retention.size > 200
    e[retention] = INT64_MIN
    left = np.nonzero(e != INT64_MIN)[0]
    want = {"rows": n, "users": U, "cutoff": cutoff, "now": now, "months": months, "prune": prune.tolist(), "retention": retention.tolist(),
            "kept": int(left.size), "left": left.tolist(), "user": u.tolist(), "owner": [oracle.shard_of(int(x), 2) for x in u.tolist()]}
    expect = tmp_path / "expect.json"
    expect.write_text(json.dumps(want))
    stub_dir = os.path.join(REPO, "tests", "_stub")
    os.makedirs(stub_dir, exist_ok=True)
    stub = os.path.join(stub_dir, "libstub_rccl_node_comm_maint.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
    res = subprocess.run([node, os.path.join(HOST, "test", "comm_maint_test.js")], cwd=REPO,
                         env=dict(os.environ, TZ=ZONE, PIE_RCCL_LIB=stub, PIE_MAINT_EXPECT=str(expect)), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-3000:]
    assert "host comm_maint_test ok" in res.stdout
