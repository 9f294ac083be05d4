"""Every run-time setting of the two libraries lives in one table (downpore_amd/csrc/dp_env.h), which is also the only place that calls
getenv.  The header's own behaviour is checked by a stand-alone program in three builds; the table, the sources and INTEGRATION.md
section 4 are held to each other by reading their text."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "downpore_amd", "csrc")
ENV_H = os.path.join(CSRC, "dp_env.h")
ACCESSORS = r"dp_env_str|dp_env_long|dp_env_tristate|dp_env_has_word|dp_tune|dp_debug|cache_cap"
HELPERS = {"dp_profile_on": "DPH_PROFILE", "dp_device_consensus_on": "DP_DEVICE_CONSENSUS", "dp_wait_mode_read": "DP_SPIN_SYNC"}


def _table():
    """{(kind, name): when} of dp_env.h's table"""
    rows = re.findall(r'^\s*\{(VAR|TUNE|DEBUG), "(\w+)", (CALL|CREATE|PROCESS), "[^"]+"\},$', open(ENV_H).read(), re.M)
    assert len(rows) > 60 and len(set((k, n) for k, n, _ in rows)) == len(rows)
    return {(k, n): w for k, n, w in rows}


def _sources():
    files = glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "host", "*.[ch]pp"))
    assert len(files) > 20
    return {f: open(f).read() for f in files}


def _kind(accessor):
    return {"dp_tune": "TUNE", "dp_debug": "DEBUG"}.get(accessor, "VAR")


@pytest.mark.parametrize("name,flags", [
    ("plain", []),
    ("asan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"]),
    ("tsan", ["-fsanitize=thread"]),
])
def test_the_header_alone_in_every_build(tmp_path, name, flags):
    exe = str(tmp_path / ("env_" + name))
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-I" + CSRC] + flags + [os.path.join(ROOT, "tests", "native", "env_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode != 0 and name in ("asan", "tsan") and "cannot find" in b.stderr:
        pytest.skip("no sanitizer runtime in this image")
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    if name == "tsan" and "unexpected memory mapping" in r.stderr:
        pytest.skip("this kernel's address-space layout is one the image's ThreadSanitizer runtime refuses to start under")
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout[-2000:] + r.stderr[-4000:]


def test_getenv_is_called_in_one_file_only():
    for f, text in _sources().items():
        if f != ENV_H:
            assert "getenv(" not in text, f


def test_every_name_the_code_asks_for_is_in_the_table_and_the_other_way_round():
    table = _table()
    used = set()
    for f, text in _sources().items():
        for acc, name in re.findall(r'\b(%s)\(\s*"(\w+)"' % ACCESSORS, text):
            assert (_kind(acc), name) in table, "%s asks for %s, which dp_env.h does not list" % (f, name)
            used.add((_kind(acc), name))
        for name in re.findall(r'Tokens t\("(\w+)"', text):
            used.add(("VAR", name))
    assert set(table) - used == set(), "listed in dp_env.h and read by nobody"


def _section4():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"^## 4\. [^\n]*\n(.*?)^## ", text, re.M | re.S)
    assert m
    return m.group(1)


def test_the_table_and_the_document_list_the_same_names():
    table, sec = _table(), _section4()
    for kind, name in table:
        assert re.search(r"`%s[`=]" % name, sec), "%s is in dp_env.h and not in INTEGRATION.md section 4" % name
    for name in set(re.findall(r"\bDPH?_[A-Z][A-Z0-9_]+\b", sec)):
        assert ("VAR", name) in table, "%s is in INTEGRATION.md section 4 and not in dp_env.h" % name
    for var, kind in (("DP_DEBUG", "DEBUG"), ("DP_TUNE", "TUNE")):
        bullet = re.search(r"^\* `%s=[^`]*`(.*?)(?=^\* |\Z)" % var, sec, re.M | re.S).group(1)
        keys = re.findall(r"`([a-z][a-z0-9_]*)`", bullet)
        assert len(keys) >= 14
        for key in keys:
            assert (kind, key) in table, "%s=%s is in INTEGRATION.md section 4 and not in dp_env.h" % (var, key)
    # ... and every key of the table is in its variable's bullet, not merely somewhere in the section
    for kind, name in table:
        if kind != "VAR":
            bullet = re.search(r"^\* `DP_%s=[^`]*`(.*?)(?=^\* |\Z)" % kind, sec, re.M | re.S).group(1)
            assert "`%s`" % name in bullet, name


def test_no_setting_is_frozen_in_a_static_unless_the_table_says_once_per_process():
    table = _table()
    # a variable with static storage - `static <type> <name> =` or `{`, not a function - whose initialiser reaches an accessor
    # before its first semicolon
    pat = re.compile(r"\bstatic\s+(?:const\s+|thread_local\s+)*[\w:<>\*&, ]+?[\s\*&]\w+\s*(?:=|\{)[^;]*?\b(%s|%s)\(\s*\"?(\w*)" % (ACCESSORS, "|".join(HELPERS)))
    seen = 0
    for f, text in _sources().items():
        for acc, name in pat.findall(text):
            name = HELPERS.get(acc, name)
            seen += 1
            assert table[(_kind(acc), name)] == "PROCESS", "%s keeps %s in a static, and dp_env.h does not list it as read once per process" % (f, name)
    assert seen >= 5  # (the pattern still finds the process-wide ones: the two cache caps, the upload ring, the text pool, the timing default)
