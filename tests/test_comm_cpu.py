"""The communicator's host-side bookkeeping, without a GPU: what pie_comm_create refuses before it opens anything, and the addon's
per-communicator n_q ring under ASan + UBSan (a stand-alone C program: nothing loaded into python or node is sanitized)."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

PIE_E_INVAL = -1


def test_comm_create_refuses_more_than_64_ranks(pie):
    """Pins a refusal both constructors have long made: one lane per rank picks the gathered Mu words (k_pick_words, a fixed
    64-thread launch) and merges the queues, so a world above 64 would silently drop ranks.  The check comes before RCCL or
    any device is opened, so it answers on a machine without a GPU."""
    with pytest.raises(pie.PieError) as ex:
        pie.PieComm([0] * 65)
    assert ex.value.code == PIE_E_INVAL, ex.value
    with pytest.raises(pie.PieError) as ex:
        pie.PieComm.for_rank(b"\0" * 128, 0, 65, 0)
    assert ex.value.code == PIE_E_INVAL, ex.value


def test_nq_ring_under_sanitizers(tmp_path):
    assert shutil.which("gcc") is not None, "gcc builds the addon and the RCCL stand-in too: it has to be there"
    exe = tmp_path / "nq_ring_test"
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(REPO, "tests", "nq_ring_test.c")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "nq ring ok" in res.stdout, res.stdout
