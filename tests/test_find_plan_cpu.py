"""The find stage's plan (downpore_amd/csrc/dp_find_plan.h: the cursor block's layout and its decoding, the capacity rule, the grids
of the chaining launches, the d_pbase, query meta and upload blocks, the minCount table) is plain C++ without a GPU call: a
stand-alone program holds it to the same rules written out a second time, in a plain build and under ASan + UBSan."""
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
    exe = str(tmp_path / ("find_plan_" + name))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags + [
        os.path.join(ROOT, "tests", "native", "find_plan_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name == "asan" and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]
