"""Loader of the model of `map -all_sequences` (tests/native/map_multi_model.cpp): compiled on demand against the built oracle
library, then driven through ctypes.  Test infrastructure only; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "map_multi_model.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "native", "_build")
ORACLE_DIR = os.path.join(ROOT, "oracle", "_build")
ISCONSISTENT_IGNORES_REF, FIRST_LENGTH_FOR_EVERY_END = 1, 2  # the two mutations
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(OUT_DIR, "libmap_multi_model.so")
    oracle = os.path.join(ORACLE_DIR, "liboracle.so")
    if not os.path.exists(oracle):
        raise RuntimeError("oracle/_build/liboracle.so is not built: run build() first")
    deps = [SRC, os.path.join(ROOT, "oracle", "oracle.hpp"), oracle]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(OUT_DIR, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "oracle"), SRC, "-o", tmp,
                               "-L" + ORACLE_DIR, "-loracle", "-Wl,-rpath," + ORACLE_DIR])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.mmm_run.restype = vp
    L.mmm_run.argtypes = [vp, vp, C.c_int64, vp, vp, C.c_int64, vp]
    L.mmm_run_files.restype = vp
    L.mmm_run_files.argtypes = [C.c_char_p, C.c_char_p, vp]
    L.mmm_free.argtypes = [vp]
    L.mmm_text.restype = C.POINTER(C.c_char)
    L.mmm_text.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    _lib = L
    return L


def _params(circular, k, query_size, min_length, chunk_size, seed_rate, all_sequences, mutation):
    return np.array([1 if circular else 0, k, query_size, min_length, chunk_size, seed_rate, 1 if all_sequences else 0, mutation],
                    dtype=np.int64)


def _take(h):
    L = load()
    n = C.c_int64(0)
    paf, err, error = (C.string_at(L.mmm_text(h, w, C.byref(n)), n.value).decode() for w in range(3))
    L.mmm_free(h)
    if error:
        raise RuntimeError(error)
    return paf, err


def run(ref_bases, ref_off, bases, off, circular=True, k=11, query_size=1000, min_length=500, chunk_size=10000, seed_rate=40,
        all_sequences=True, mutation=0):
    """(paf, stderr text) of the model for reference sequences ref_bases[ref_off[c]:ref_off[c + 1]] (named r0000000, ...) and reads
    bases[off[i]:off[i + 1]] (the same names; shorter than min_length: left out)"""
    rb, ro = np.ascontiguousarray(ref_bases, dtype=np.uint8), np.ascontiguousarray(ref_off, dtype=np.int64)
    b, o = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
    p = _params(circular, k, query_size, min_length, chunk_size, seed_rate, all_sequences, mutation)
    return _take(load().mmm_run(rb.ctypes.data, ro.ctypes.data, len(ro) - 1, b.ctypes.data, o.ctypes.data, len(o) - 1, p.ctypes.data))


def run_files(ref_path, reads_path, circular=True, k=11, query_size=1000, min_length=500, chunk_size=10000, seed_rate=40,
              all_sequences=True, mutation=0):
    p = _params(circular, k, query_size, min_length, chunk_size, seed_rate, all_sequences, mutation)
    return _take(load().mmm_run_files(str(ref_path).encode(), str(reads_path).encode(), p.ctypes.data))
