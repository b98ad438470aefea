"""GPU: the token store's turnOrdered option through the Node addon (setTurnOrdered, tableInfo) — a fresh node child with its own
timeout runs sph-pie_amd/host/test/gpu_turn_ordered_test.js: 50 createSession calls and a mixed turn on a store whose table has a
valid ordered run keep that run with every row, and the feed of a scan on it equals the events the calls mean."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

HOST = os.path.join(REPO, "sph-pie_amd", "host")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None, reason="node is not installed on this machine")


@needs_node
@pytest.mark.gpu
def test_turn_ordered_through_the_node_host(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    env = {k: v for k, v in os.environ.items() if k != "PIE_TURN_ORDERED"}
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_turn_ordered_test.js")], cwd=REPO, env=dict(env, TZ="UTC"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "host gpu_turn_ordered_test ok" in res.stdout
