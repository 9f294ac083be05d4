"""A Mapper's trimmed batch (Mapper.map(raw, trim=...), dph_mapper_map_trim) without a GPU: the trim dict is refused before any library
call with map_reads' own texts, the C entry point refuses bad arguments with a text, the new names are declared in the headers the
libraries are held to, and the arithmetic the batch step adds (map_plan.hpp: mapTailId, mapTailIds, mapTailSpans) is held to a second
statement of its rule by a stand-alone program, in a plain build and under ASan + UBSan."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import trim_cases as TC
from tests.test_map_trim_cpu import reference
from tests.test_overlap_trim_cpu import reads_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downpore_amd", "csrc")


def test_mapper_map_names_what_a_trim_dict_lacks_or_does_not_know():
    """on an instance whose handle was never opened: the dict is checked before the handle is looked at, let alone a library call made"""
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import Mapper, map_reads
    m = Mapper.__new__(Mapper)
    ads = object()  # (never touched)
    cases = [(dict(back=ads), "'front'"), (dict(front=ads, k=6), "'back'"), (dict(k=6), "'front' and 'back'"),
             (dict(front=ads, back=ads, midle=True), "unknown trim key 'midle'"), (True, "dict")]
    for trim, what in cases:
        with pytest.raises(DpError, match=what) as got:
            m.map(None, trim=trim)
        with pytest.raises(DpError) as want:
            map_reads(None, None, trim=trim)
        assert str(got.value) == str(want.value)  # the same texts map_reads gives
    assert list(inspect.signature(Mapper.map).parameters) == ["self", "reads", "trim"]
    assert inspect.signature(Mapper.map).parameters["trim"].default is None
    with pytest.raises(DpError, match="closed"):  # a good dict gets as far as the handle
        m.map(None, trim=dict(front=reads_of(TC.FRONT, 0), back=reads_of(TC.BACK, 0), k=6))
    with pytest.raises(DpError, match="closed"):
        m.map(None)


def test_dph_mapper_map_trim_refuses_bad_arguments_with_a_text():
    from downpore_amd.overlap import Reads, load_host
    H = load_host()
    vp = C.c_void_p
    H.dph_mapper_map_trim.restype = vp
    H.dph_mapper_map_trim.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
    H.dph_last_error.restype = C.c_char_p
    H.dph_last_error.argtypes = [vp]
    g, off = reference()
    raw = Reads(g[:5000], np.array([0, 2000, 5000], dtype=np.int64), min_len=50, himem=False)
    front, back = reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0)
    tp = np.array([6, 10000, 90, 5, 1, 0, 1, 1, 1, 5000, 85, 100, 0, 300_000_000], dtype=np.int64)
    # no mapper can be opened without a device: the slot holds NULL, or the address of a block that a call refused for another argument
    # never looks into
    block = (C.c_char * 256)()
    fake = C.cast(block, vp)

    def run(mapper=fake, handles=(raw.h, front.h, back.h), trim=tp.ctypes.data, n_trim=14, out=True):
        th = vp(0x1234)
        h = H.dph_mapper_map_trim(mapper, *handles, trim, n_trim, C.byref(th) if out else None)
        assert not h and (not out or not th.value)  # NULL, and no trim handle either
        return H.dph_last_error(None).decode()

    assert run(mapper=None).startswith("dph_mapper_map_trim: bad arguments")
    for i in range(3):
        hs = [raw.h, front.h, back.h]
        hs[i] = None
        assert run(handles=hs).startswith("dph_mapper_map_trim: bad arguments")
    assert run(trim=None).startswith("dph_mapper_map_trim: bad arguments")
    assert run(out=False).startswith("dph_mapper_map_trim: bad arguments")
    for n in (0, 7, 9, 13, 15):
        got = run(n_trim=n)
        assert got.startswith("dph_mapper_map_trim: bad arguments") and "8 trim parameters, or 14" in got


def _declared(header, prefix):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % prefix, txt))


def test_the_new_entry_points_are_declared_exported_and_wrapped():
    import downpore_amd.hip as h
    from downpore_amd.overlap import load_host
    L, H = h.load_library(), load_host()
    for s in ("dp_reads_replace_tail_packed", "dp_reads_respan_tail_rc"):
        assert s in _declared("downpore_hip.h", "dp") and s in h.SYMBOLS and hasattr(L, s), s
    assert "dph_mapper_map_trim" in _declared("downpore_host.h", "dph") and hasattr(H, "dph_mapper_map_trim")
    assert list(inspect.signature(h.Context.replace_tail_packed).parameters) == ["self", "keep", "packed", "lens", "pinned"]
    assert list(inspect.signature(h.Context.respan_tail_rc).parameters) == ["self", "keep", "spans"]
    go = open(os.path.join(ROOT, "integration", "gpuhost", "chost.go")).read()
    assert re.search(r"func \(m \*Mapper\) MapTrim\(", go) and "C.dph_mapper_map_trim(" in go


@pytest.mark.parametrize("name,flags", [
    ("plain", []),
    ("asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
])
def test_tail_ids_and_spans_in_every_build(tmp_path, name, flags):
    exe = str(tmp_path / ("map_trim_tail_" + name))
    cmd = (["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(CSRC, "host"), "-I" + os.path.join(ROOT, "include")]
           + flags + [os.path.join(ROOT, "tests", "native", "map_trim_tail_check.cpp"), "-o", exe, "-pthread"])
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]
