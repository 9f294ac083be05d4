"""Loader of the `trim` edge-stage model (tests/native/trim_model.cpp): compiled on demand against the built oracle library,
then driven through ctypes.  Test infrastructure only; the product never loads it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "trim_model.cpp")
OUT_DIR = os.path.join(ROOT, "tests", "native", "_build")
ORACLE_DIR = os.path.join(ROOT, "oracle", "_build")
GOLDEN = os.path.join(ROOT, "tests", "golden", "trim")
FRONT = os.path.join(GOLDEN, "adapters_front.fasta")
BACK = os.path.join(GOLDEN, "adapters_back.fasta")

REC_FIELDS = ["earliest", "latest", "found", "best_match", "ambiguous", "best_ident"]
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(OUT_DIR, "libtrim_model.so")
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
    for f in (L.tm_run, L.tm_determine):
        f.restype = vp
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, vp]
    L.tm_run_with_records.restype = vp
    L.tm_run_with_records.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, vp, vp]
    L.tm_free.argtypes = [vp]
    L.tm_failed.argtypes = [vp]
    L.tm_text.restype = C.POINTER(C.c_char)
    L.tm_text.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.tm_ints.restype = C.POINTER(C.c_int32)
    L.tm_ints.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.tm_demultiplex.argtypes = [vp, C.c_char_p]
    _lib = L
    return L


def params(k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5, tag_adapters=True, require_pairs=False,
           determine_adapters=True, verbosity=1, mutation=0):
    return np.array([k, check_reads, adapter_threshold, extra_end_trim, int(tag_adapters), int(require_pairs), int(determine_adapters),
                     verbosity, mutation], dtype=np.int64)


class Result:
    def __init__(self, h):
        L = load()
        self._h = h
        n = C.c_int64(0)

        def text(which):
            return C.string_at(L.tm_text(h, which, C.byref(n)), n.value).decode()

        def ints(which):
            p = L.tm_ints(h, which, C.byref(n))
            return np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int32)

        self.failed = bool(L.tm_failed(h))
        self.output, self.stderr = text(0), text(1)
        self.adapters = [(ln.split("\t")[0], ln.split("\t")[1], int(ln.split("\t")[2])) for ln in text(2).splitlines()]
        self.table = ints(0).reshape(-1, 5)
        self.recs = ints(1).reshape(-1, 6)
        self.counts = ints(2).astype(np.uint64)
        self.enabled = ints(3).astype(np.uint8)
        self.eligible = ints(4)
        self.kmer_seed, self.segs, self.seg_off, self.pairs = ints(5), ints(6), ints(7), ints(8)

    def demultiplex(self, path):
        return load().tm_demultiplex(self._h, str(path).encode())

    def close(self):
        if self._h:
            load().tm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run(reads, front=FRONT, back=BACK, **kw):
    """The whole edge stage on the model: reads / front / back are file paths."""
    p = params(**kw)
    return Result(load().tm_run(str(reads).encode(), str(front).encode(), str(back).encode(), p.ctypes.data))


def determine(reads, front=FRONT, back=BACK, **kw):
    p = params(**kw)
    return Result(load().tm_determine(str(reads).encode(), str(front).encode(), str(back).encode(), p.ctypes.data))


def run_with_records(reads, front, back, recs, counts, enabled=None, **kw):
    p = params(determine_adapters=enabled is not None, **kw)
    r = np.ascontiguousarray(recs, dtype=np.int32)
    c = np.ascontiguousarray(counts, dtype=np.int64)
    en = None if enabled is None else np.ascontiguousarray(enabled, dtype=np.uint8)
    return Result(load().tm_run_with_records(str(reads).encode(), str(front).encode(), str(back).encode(), p.ctypes.data,
                                             None if en is None else en.ctypes.data, r.ctypes.data, c.ctypes.data))
