"""GPU: the wide pipelined exchange over shards of a skewed table with pie_set_wide_ordered on — a fresh process whose RCCL is
the stand-in of tests/stub_rccl.c drives two shards on GPU 0 (tests/comm_wide_ordered_worker.py): every rank keeps its union
from the first step on, and every global feed equals the oracle's scan of the unsharded table."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def test_wide_steps_on_a_skewed_table(pie, oracle):
    res = subprocess.run([sys.executable, os.path.join(REPO, "tests", "comm_wide_ordered_worker.py"), "2", "300000", "3001"],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=REPO)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "comm wide ordered ok" in res.stdout
