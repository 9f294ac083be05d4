"""A Mapper batch's arithmetic (downpore_amd/csrc/host/map_plan.hpp: mapBatchLayout, mapBatchReadId) without a GPU: a stand-alone
program holds it to brute force and to mapPackedLayout of head + batch, in a plain build and under ASan + UBSan; and the mapper's and
the tail replace's entry points are declared in the headers the libraries are held to (tests/test_abi_symbols.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downpore_amd", "csrc")


@pytest.mark.parametrize("name,flags", [
    ("plain", []),
    ("asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
])
def test_batch_layout_in_every_build(tmp_path, name, flags):
    exe = str(tmp_path / ("map_tail_" + name))
    cmd = (["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(CSRC, "host"), "-I" + os.path.join(ROOT, "include")]
           + flags + [os.path.join(ROOT, "tests", "native", "map_tail_check.cpp"), "-o", exe, "-pthread"])
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name == "asan" and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]


def _declared(header, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % prefix, txt))


def test_the_new_entry_points_are_declared_and_exported():
    import downpore_amd.hip as h
    from downpore_amd.overlap import load_host
    L, H = h.load_library(), load_host()
    for s in ("dp_reads_replace_tail_packed_rc", "dp_ctx_refresh_shared"):
        assert s in _declared("downpore_hip.h", "dp") and s in h.SYMBOLS and hasattr(L, s), s
    for s in ("dph_mapper_open", "dph_mapper_map", "dph_mapper_close"):
        assert s in _declared("downpore_host.h", "dph") and hasattr(H, s), s


def test_python_mapper_surface():
    import inspect

    from downpore_amd.mapping import Mapper, map_reads
    want = ["ref", "circular", "k", "query_size", "min_length", "chunk_size", "seed_rate", "device", "index", "all_sequences"]
    assert list(inspect.signature(Mapper.__init__).parameters)[1:] == want
    assert list(inspect.signature(map_reads).parameters) == ["ref", "reads"] + want[1:] + ["trim"]
    for name in ("map", "close", "__enter__", "__exit__"):
        assert callable(getattr(Mapper, name))
