"""The arithmetic that decides what `map` asks of the device (downpore_amd/csrc/host/map_plan.hpp: limits, join chunks, packed layout,
chunk schedule, window items, reverse-strand fix-up, shard window merge, dense estimate) is plain C++ without a GPU call: a stand-alone
program checks it against the oracle's Mapper, rules written out a second time, explicit lists and brute force, in a plain build and
under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downpore_amd", "csrc")
ORACLE_DIR = os.path.join(ROOT, "oracle", "_build")


@pytest.mark.parametrize("name,flags", [
    ("plain", []),
    ("asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
])
def test_the_header_alone_in_every_build(tmp_path, name, flags):
    assert os.path.exists(os.path.join(ORACLE_DIR, "liboracle.so")), "oracle/_build/liboracle.so is not built: run build() first"
    exe = str(tmp_path / ("map_plan_" + name))
    cmd = (["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(CSRC, "host"), "-I" + os.path.join(ROOT, "include"),
            "-I" + os.path.join(ROOT, "oracle")] + flags + [os.path.join(ROOT, "tests", "native", "map_plan_check.cpp"), "-o", exe,
           "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR, "-pthread"])
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name == "asan" and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]
