"""Loader of the model of the alignment rule (tests/native/align_model.cpp: full-matrix edit distance and the canonical CIGAR of
DESIGN.md 4.9): compiled on demand, then driven through ctypes.  Test infrastructure only; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "align_model.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "native", "_build")
PREFER_I_OVER_M, D_BEFORE_I = 1, 2  # the two mutations of the walk
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(OUT_DIR, "libalign_model.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(SRC):
        os.makedirs(OUT_DIR, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", SRC, "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    L.alm_align.restype = C.c_int64
    L.alm_align.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    _lib = L
    return L


def codes(s):
    """'ACGT...' (or an array of codes) -> uint8 codes, one per base: A 0, C 1, G 2, T 3 (any other letter: its byte value)"""
    if isinstance(s, str):
        a = np.frombuffer(s.encode(), dtype=np.uint8)
        out = a.copy()
        for ch, v in zip(b"ACGT", range(4)):
            out[a == ch] = v
        return out
    return np.ascontiguousarray(s, dtype=np.uint8)


def align(q, t, mutation=0):
    """(NM, CIGAR) of query q against target t by the rule, on the full matrix."""
    L = load()
    qa, ta = codes(q), codes(t)
    cap = 24 * (len(qa) + len(ta)) + 32
    buf = C.create_string_buffer(cap)
    n = C.c_int64(0)
    nm = L.alm_align(qa.ctypes.data, len(qa), ta.ctypes.data, len(ta), mutation, buf, cap, C.byref(n))
    assert n.value <= cap
    return int(nm), buf.raw[:n.value].decode()


def consumed(cigar):
    """(query bases, target bases) a CIGAR string consumes: its M + I and its M + D"""
    import re
    q = t = 0
    for ln, op in re.findall(r"(\d+)([MID])", cigar):
        q += int(ln) if op != "D" else 0
        t += int(ln) if op != "I" else 0
    return q, t
