"""dp_scan_reads' host bookkeeping of the reads' ignore flags (downpore_amd/csrc/dp_scan_flags.h: the shadow of the flags, bases and
reads scanned) is plain C++ without a GPU call: a stand-alone program checks it against a brute-force recount, in a plain build and
under ASan + UBSan."""
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
    exe = str(tmp_path / ("scan_flags_" + name))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC] + flags + [os.path.join(ROOT, "tests", "native", "scan_flags_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name == "asan" and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]
