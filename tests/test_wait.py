"""CPU: the one bounded wait (csrc/pie_wait.h) behind every host wait on the device.  Its deadline branch cannot be reached on
a GPU without hanging a kernel, so a stand-alone program drives the loop with fake callables under ASan + UBSan."""
import os
import re
import shutil
import subprocess

from conftest import REPO

CSRC = os.path.join(REPO, "sph-pie_amd", "csrc")


def test_bounded_wait_under_sanitizers(tmp_path):
    assert shutil.which("g++") is not None, "g++ is needed for the stand-alone wait check"
    exe = tmp_path / "wait_test"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(REPO, "tests", "wait_test.cpp")])
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert res.returncode == 0 and "bounded wait ok" in res.stdout, res.stdout


def test_no_other_loop_polls_the_device():
    """one loop: outside pie_wait.h no source file pauses, yields or naps, so none can pace a polling loop of its own; and the
    library's source digest moves with the header"""
    for name in sorted(os.listdir(CSRC)):
        if name != "pie_wait.h":
            text = open(os.path.join(CSRC, name)).read()
            assert not re.search(r"\b(sched_yield|nanosleep|usleep|__builtin_ia32_pause)\b", text), name
    assert '"pie_wait.h"' in open(os.path.join(REPO, "sph-pie_amd", "build.py")).read()
