"""CPU-side checks of the drop-in boundary: the library loads and exports every symbol the header declares;
context creation fails loudly (no CPU fallback) when no GPU is present."""
import os
import re

import pytest


def _header_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "downpore_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dp_[a-z_0-9]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import downpore_amd.hip as h
    L = h.load_library()
    syms = _header_symbols()
    assert syms, "no symbols parsed from include/downpore_hip.h"
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(h.SYMBOLS) == syms
    assert b"gfx950" in L.dp_version()


def test_library_exports_nothing_else():
    """The dynamic symbol table holds the C ABI only (version script + -fvisibility=hidden): no kernel launch stubs, no
    C++ template instantiations, no internal helpers."""
    import subprocess
    import downpore_amd.hip as h
    out = subprocess.check_output(["nm", "-D", "--defined-only", h.lib_path()], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert exported == _header_symbols()


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_HEADER = os.path.join(ROOT, "include", "downpore_host.h")
TESTHOOKS_HEADER = os.path.join(ROOT, "downpore_amd", "csrc", "host", "dph_testhooks.h")


def _host_header_symbols(path=HOST_HEADER):
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dph_[a-z_0-9]+)\s*\(", txt)))


def test_host_library_exports_exactly_its_header():
    """libdownpore_host.so - the pipeline the bench measures - has a published boundary of its own (include/downpore_host.h):
    every declared entry point is exported under the version node DPH, the test hooks of csrc/host/dph_testhooks.h under DPH_TEST,
    and nothing else is exported (version script: the C++ mirror of the Go layers stays local)."""
    import subprocess
    from downpore_amd.overlap import host_lib_path, load_host
    H = load_host()
    public, hooks = _host_header_symbols(), _host_header_symbols(TESTHOOKS_HEADER)
    assert len(public) > 50
    for s in public + hooks:
        assert hasattr(H, s), s
    out = subprocess.check_output(["nm", "-D", "--defined-only", host_lib_path()], text=True)
    by_node, nodes = {}, []
    for ln in out.splitlines():
        if not ln.strip():
            continue
        kind, name = ln.split()[-2:]
        if kind == "A":  # the version nodes themselves
            nodes.append(name)
            continue
        sym, sep, node = name.partition("@@")
        assert sep, "%s is exported without a version node" % name
        by_node.setdefault(node, []).append(sym)
    assert sorted(nodes) == ["DPH", "DPH_TEST"]
    assert sorted(by_node) == ["DPH", "DPH_TEST"]
    assert sorted(by_node["DPH"]) == public
    assert sorted(by_node["DPH_TEST"]) == hooks


def test_host_headers_share_no_name():
    public, hooks = _host_header_symbols(), _host_header_symbols(TESTHOOKS_HEADER)
    assert len(hooks) == 16
    assert not set(public) & set(hooks)


def test_nothing_outside_the_tests_mentions_a_test_hook():
    """The Go side, the Python drivers, the benchmark and the command-line program stay on the boundary."""
    import glob
    hooks = _host_header_symbols(TESTHOOKS_HEADER)
    assert hooks
    files = glob.glob(os.path.join(ROOT, "integration", "**", "*"), recursive=True)
    files += glob.glob(os.path.join(ROOT, "downpore_amd", "*.py"))
    files += [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "downpore_amd", "csrc", "host", "host_cli.cpp")]
    files = [f for f in files if os.path.isfile(f)]
    assert len(files) > 10
    for f in files:
        txt = open(f, errors="replace").read()
        for s in hooks:
            assert not re.search(r"\b%s\b" % s, txt), "%s mentions the test hook %s" % (os.path.relpath(f, ROOT), s)


def test_stats_sizes_in_the_header_match_the_field_lists():
    """A C or Go caller sizes the buffers of the four stats calls from the header's defines (the C++ writers static_assert their
    arrays against the same defines); the Python drivers name the same number of fields."""
    from downpore_amd.mapping import MAP_STAT_FIELDS
    from downpore_amd.overlap import STAT_FIELDS
    from downpore_amd.trim import TRIM_MID_STAT_FIELDS, TRIM_STAT_FIELDS
    defines = dict((k, int(v)) for k, v in re.findall(r"^#define (DPH_[A-Z_]+_STATS) (\d+)\s*$", open(HOST_HEADER).read(), flags=re.M))
    assert defines == {"DPH_OVERLAP_STATS": len(STAT_FIELDS), "DPH_MAP_STATS": len(MAP_STAT_FIELDS),
                       "DPH_TRIM_STATS": len(TRIM_STAT_FIELDS), "DPH_TRIM_MID_STATS": len(TRIM_MID_STAT_FIELDS)}


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import downpore_amd
    with pytest.raises(downpore_amd.DpError):
        downpore_amd.Context(0)
