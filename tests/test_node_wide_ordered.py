"""GPU: the Node addon's setWideOrdered — a fresh node child with its own timeout runs
sph-pie_amd/host/test/gpu_wide_ordered_test.js: a 100-query wide batch on a mode-2 table keeps no union with the switch off and,
with it on, a union whose row count equals the one derived here from the CPU oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

HOST = os.path.join(REPO, "sph-pie_amd", "host")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None, reason="node is not installed on this machine")

T0, DAY, HOUR, SEED = 1700000000000, 86400 * 1000, 3600 * 1000, 0x5EED5EED


@needs_node
@pytest.mark.gpu
def test_wide_ordered_through_the_node_host(pie, oracle):
    assert pie.build_napi() is not None, "node headers (node_api.h) not found"
    n, U, D = 200000, 2000, 32
    cols = oracle.gen(SEED, n, 0, n, U, D, 0)
    masks = [0x55555555, 0xAAAAAAAA, 0xFFFFFFFF, 0xFFFF0000, 0x1, 0x80000001]
    lists = [oracle.scan(*cols, U, T0 - 6 * HOUR - 977 * q - (q % 3) * HOUR, T0 - (61 + q % 4) * DAY - 13 * q, masks[q % 6])[2] for q in range(100)]
    want_rows = int(np.unique(np.concatenate(lists)).size)
    assert 0 < want_rows <= n // 16 + 4096
    res = subprocess.run([node, os.path.join(HOST, "test", "gpu_wide_ordered_test.js"), str(want_rows)], cwd=REPO, env=dict(os.environ, TZ="UTC"),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:]
    assert "host gpu_wide_ordered_test ok" in res.stdout
