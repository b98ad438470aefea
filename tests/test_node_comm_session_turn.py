"""GPU: the turn that logs in behind the communicator through the Node addon (commSessionTurn) — a fresh node child with its own
timeout runs sph-pie_amd/host/test/gpu_comm_session_turn_test.js: world 2 on GPU 0 through PIE_RCCL_LIB (tests/stub_rccl.c), a short
hand-written turn (create, get, touch, delete, get) answered as the unsharded sessionTurn answers it."""
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
def test_comm_session_turn_through_the_node_addon(pie):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    stub_dir = os.path.join(REPO, "tests", "_stub")
    os.makedirs(stub_dir, exist_ok=True)
    stub = os.path.join(stub_dir, "libstub_rccl_node_session_turn.so")
    subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-I/opt/rocm/include", "-o", stub, os.path.join(REPO, "tests", "stub_rccl.c"),
                    "-L/opt/rocm/lib", "-lamdhip64"], check=True, timeout=300)
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_comm_session_turn_test.js")], cwd=REPO,
                         env=dict(os.environ, TZ="UTC", PIE_RCCL_LIB=stub), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stdout[-3000:]
    assert "host gpu_comm_session_turn_test ok" in res.stdout
