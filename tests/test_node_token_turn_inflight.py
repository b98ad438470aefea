"""GPU: turns beside a batch in flight through the Node addon (tokenTurnBegin / tokenTurnFinish / tokenTurnRoom): turnAsync of
host/tokenSessionStore.js on the recorded reference trace with a batch begun by scanBatchBegin open across every call, and the
feed service's {turns: true} turn against the default path — a fresh node child with its own timeout, as
tests/test_node_token_inflight.py runs its host test."""
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
def test_inflight_token_turn_through_the_node_addon(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_token_turn_inflight_test.js")], cwd=REPO, env=dict(os.environ, TZ="UTC"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "host gpu_token_turn_inflight_test ok" in res.stdout
