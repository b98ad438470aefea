"""CPU: the Node host's opt-in wide grouping (feedService({wide: true}) -> store.scanWideDevice, up to store.WIDE_MAX groups per
device pass; the default grouping unchanged) over a stub store.  No addon, no GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

node = shutil.which("node")


@pytest.mark.skipif(node is None, reason="node is not installed on this machine")
def test_feed_service_wide_grouping():
    res = subprocess.run([node, os.path.join(REPO, "sph-pie_amd", "host", "test", "wide_cpu_test.js")], cwd=REPO,
                         env=dict(os.environ, TZ="UTC"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert "wide_cpu_test ok" in res.stdout
