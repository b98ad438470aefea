"""GPU: turns that log in through the Node addon (sessionTurn) and host/tokenSessionStore.js: the recorded reference trace G5 with
the create calls inside the turns, in turns of 7, and createSession / getSession as a request handler calls them.  A fresh node
child with its own timeout, as tests/test_node_token_turn.py runs its host test."""
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
def test_session_turns_through_the_node_addon_and_the_token_store(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_session_turn_test.js")], cwd=REPO, env=dict(os.environ, TZ="UTC"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "host gpu_session_turn_test ok" in res.stdout
