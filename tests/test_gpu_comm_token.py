"""GPU: the token column behind the C-ABI communicator (pie_comm_token_set / _append / _lookup / _set_end).  Each case runs in a
fresh process (tests/comm_token_worker.py) whose RCCL is the one-GPU stand-in tests/stub_rccl.c, so worlds above one run on one
MI355X; the model is the unsharded TokenModel of tests/token_model.py."""
import os
import subprocess
import sys

import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
WORKER = os.path.join(REPO, "tests", "comm_token_worker.py")


def run_worker(case, timeout):
    res = subprocess.run([sys.executable, WORKER, case], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout, cwd=REPO)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_getsession_across_shards_equals_the_unsharded_table(pie, oracle):
    """Worlds 1, 2, 3, 5: token_set, append_rows + token_append with no wait, token_lookup equal to the unsharded TokenModel
    element for element (owner included, cross-shard duplicates answering with the largest global row), token_set_end with
    repeats and expired tokens equal to TokenModel.token_set_end; merged expired queues and gathered feeds equal the oracle."""
    assert "worlds ok" in run_worker("worlds", 300)


def test_refused_calls_change_no_shard(pie, oracle):
    """Refused while a pipelined step is uncollected; a call one shard refuses changes covered_g and token_builds on none."""
    assert "errors ok" in run_worker("errors", 120)
