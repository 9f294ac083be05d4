"""The arithmetic between a finished mapping and its alignment (downpore_amd/csrc/host/align_plan.hpp: strand flip, circular wrap, the
out-of-range clauses, device items, run words to text) is plain C++ without a GPU call: a stand-alone program checks it, in a plain
build and under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downpore_amd", "csrc")


@pytest.mark.parametrize("name,flags", [
    ("plain", []),
    ("asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
])
def test_the_header_alone_in_every_build(tmp_path, name, flags):
    exe = str(tmp_path / ("align_plan_" + name))
    cmd = (["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(CSRC, "host"), "-I" + os.path.join(ROOT, "include")]
           + flags + [os.path.join(ROOT, "tests", "native", "align_plan_check.cpp"), "-o", exe])
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name == "asan" and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]
