"""GPU: the in-flight expired queue through the Node addon (expiredQueueBegin / expiredQueueFinish / expiredQueueRoom with batches
held in flight by scanBatchBegin) and the feed service's {purgeInFlight: true} purge tick against the synchronous one on the same
trace — a fresh node child with its own timeout, as tests/test_node_token_inflight.py runs its host test."""
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
def test_inflight_expired_queue_through_the_node_addon(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    env = dict(os.environ, TZ="UTC")
    env.pop("PIE_PURGE_IN_FLIGHT", None)
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_expired_inflight_test.js")], cwd=REPO, env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "host gpu_expired_inflight_test ok" in res.stdout
