"""GPU: a whole turn through the Node addon (tokenTurn) against a JS restatement of the rules, and host/tokenSessionStore.js — the
store that keeps no per-session state on the host — against the recorded reference trace G5, call by call and in turns.  A fresh
node child with its own timeout, as tests/test_node_token.py runs its host test."""
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
def test_turns_through_the_node_addon_and_the_token_store(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_token_turn_test.js")], cwd=REPO, env=dict(os.environ, TZ="UTC"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout
    assert "host gpu_token_turn_test ok" in res.stdout
