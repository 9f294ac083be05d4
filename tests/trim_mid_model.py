"""Loader of the model of `trim`'s middle-adapter stage (tests/native/trim_mid_model.cpp, which chains after the edge model):
compiled on demand against the built oracle library, then driven through ctypes.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import trim_model as TM

ROOT = TM.ROOT
SRC = os.path.join(ROOT, "tests", "native", "trim_mid_model.cpp")
FRONT, BACK = TM.FRONT, TM.BACK
PLAN_FIELDS = ["read", "start", "end", "remainder", "seeds", "indexed"]
REC_FIELDS = ["adapter", "chunk", "ordinal", "start_rel", "covered", "chain_len"]
SPLIT_FIELDS = ["read", "a_end", "b_start", "kept"]
_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.path.join(TM.OUT_DIR, "libtrim_mid_model.so")
    oracle = os.path.join(TM.ORACLE_DIR, "liboracle.so")
    if not os.path.exists(oracle):
        raise RuntimeError("oracle/_build/liboracle.so is not built: run build() first")
    deps = [SRC, TM.SRC, os.path.join(ROOT, "oracle", "oracle.hpp"), oracle]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(TM.OUT_DIR, exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-I" + os.path.join(ROOT, "oracle"), SRC, "-o", tmp,
                               "-L" + TM.ORACLE_DIR, "-loracle", "-Wl,-rpath," + TM.ORACLE_DIR])
        os.replace(tmp, so)
    L = C.CDLL(so)
    vp = C.c_void_p
    L.tmm_run.restype = vp
    L.tmm_run.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, vp, vp, vp, vp, vp, vp, C.c_int64]
    L.tmm_free.argtypes = [vp]
    L.tmm_failed.argtypes = [vp]
    L.tmm_error.restype = C.c_char_p
    L.tmm_error.argtypes = [vp]
    L.tmm_text.restype = C.POINTER(C.c_char)
    L.tmm_text.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.tmm_ints.restype = C.POINTER(C.c_int32)
    L.tmm_ints.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.tmm_chunk_plan.restype = C.c_int64
    L.tmm_chunk_plan.argtypes = [C.c_int64, C.c_int64, vp, C.c_int64]
    L.tmm_demultiplex.argtypes = [vp, C.c_char_p]
    _lib = L
    return L


def params(chunk_size=5000, middle_threshold=85, extra_middle_trim=100, discard_middle=False, flush_seeds=300_000_000, mid_mutation=0, **kw):
    return np.concatenate([TM.params(**kw), np.array([chunk_size, middle_threshold, extra_middle_trim, int(discard_middle), flush_seeds,
                                                      mid_mutation], dtype=np.int64)])


class Result:
    def __init__(self, h):
        L = load()
        self._h = h
        self.error = L.tmm_error(h).decode()
        if self.error:
            return
        n = C.c_int64(0)

        def text(which):
            return C.string_at(L.tmm_text(h, which, C.byref(n)), n.value).decode()

        def ints(which, width=1):
            p = L.tmm_ints(h, which, C.byref(n))
            a = np.ctypeslib.as_array(p, shape=(n.value,)).copy() if n.value else np.zeros(0, dtype=np.int32)
            return a.reshape(-1, width) if width > 1 else a

        self.failed = bool(L.tmm_failed(h))
        self.output, self.stderr = text(0), text(1)
        self.adapters = [(ln.split("\t")[0], ln.split("\t")[1], int(ln.split("\t")[2])) for ln in text(2).splitlines()]
        self.extras = text(3).splitlines()
        self.table = ints(0, 5)
        self.plan = ints(1, 6)
        self.recs = ints(2, 6)
        self.splits = ints(3, 4)
        c = ints(4)
        self.counters = dict(batches=int(c[0]), out_of_range=int(c[1]), candidate_pairs=int(c[2]), indexed_chunks=int(c[3]),
                             front_adapters=int(c[4]))
        self.segs, self.seg_off = ints(5), ints(6)
        self.edge_recs = ints(7, 6)
        self.edge_counts = ints(8).astype(np.uint64)
        self.enabled = ints(9).astype(np.uint8)
        self.candidates = ints(10, 2)

    def chunk_segments(self, c):
        return self.segs[self.seg_off[c]:self.seg_off[c + 1]]

    def demultiplex(self, path):
        return load().tmm_demultiplex(self._h, str(path).encode())

    def close(self):
        if self._h:
            load().tmm_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run(reads, front=FRONT, back=BACK, edge=None, seed_counts=None, mid_recs=None, **kw):
    """The whole command on the model.  edge = (recs, counts, enabled or None): the edge stage's matching results supplied;
    seed_counts (per planned chunk) with mid_recs ([n, 6], canonical order): the middle stage's supplied."""
    keep = []

    def ptr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a.ctypes.data

    if edge is not None:
        kw["determine_adapters"] = edge[2] is not None
    p = params(**kw)
    er, ec, en = (None, None, None) if edge is None else edge
    if mid_recs is not None:
        mid_recs = np.ascontiguousarray(mid_recs, dtype=np.int32).reshape(-1, 6)
    return Result(load().tmm_run(str(reads).encode(), str(front).encode(), str(back).encode(), p.ctypes.data, ptr(en, np.uint8),
                                 ptr(er, np.int32), ptr(ec, np.int64), ptr(seed_counts, np.int32), ptr(mid_recs, np.int32),
                                 0 if mid_recs is None else len(mid_recs)))


def chunk_plan(length, chunk_size):
    """[(start, end, remainder)] of trim.go:165-184 for one trimmed length"""
    L = load()
    n = L.tmm_chunk_plan(length, chunk_size, None, 0)
    out = np.zeros((max(n, 1), 3), dtype=np.int32)
    L.tmm_chunk_plan(length, chunk_size, out.ctypes.data, n)
    return out[:n]
