"""`downpore trim`, edge stage, on the GPU: Python front end of the C++ host mirror of trim.Trimmer (libdownpore_host.so) and a
thin binding of the device entry points behind it (dp_trim_setup / dp_trim_edges, libdownpore_hip.so)."""
import ctypes as C

import numpy as np

from .hip import DpError, load_library
from .overlap import load_host

TRIM_STAT_FIELDS = ["seen", "none", "reads", "front_adapters", "back_adapters", "t_determine_s", "t_extract_s", "upload_ms", "kernel_ms",
                    "download_ms", "t_apply_s", "t_write_s", "determine_kernel_ms", "bytes_up", "bytes_down"]
#: columns of the per-read table
TRIM_TABLE_FIELDS = ["front_trim", "back_trim", "ignore", "front_adapter", "back_adapter"]
#: fields of one edge record (dp_trim_rec)
TRIM_REC_FIELDS = ["earliest", "latest", "found", "best_match", "ambiguous", "best_ident"]
EDGE = 150
MODE_TRIM, MODE_DETERMINE = 0, 1


def _host():
    H = load_host()
    vp = C.c_void_p
    H.dph_trim_run.restype = vp
    H.dph_trim_run.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int]
    H.dph_trim_apply.restype = vp
    H.dph_trim_apply.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int64, vp]
    H.dph_trim_free.argtypes = [vp]
    for f in (H.dph_trim_output, H.dph_trim_errtext, H.dph_trim_adapters):
        f.restype = C.POINTER(C.c_char)
        f.argtypes = [vp, C.POINTER(C.c_int64)]
    H.dph_trim_table.restype = C.c_int64
    H.dph_trim_table.argtypes = [vp, vp, C.c_int64]
    H.dph_trim_stats.argtypes = [vp, vp]
    H.dph_trim_demultiplex.argtypes = [vp, C.c_char_p]
    H.dph_trim_index.restype = C.c_int64
    H.dph_trim_index.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int64, vp, vp, vp, vp]
    return H


def _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity):
    return np.array([k, check_reads, adapter_threshold, extra_end_trim, 1 if tag_adapters else 0, 1 if require_pairs else 0,
                     1 if determine_adapters else 0, verbosity], dtype=np.int64)


class TrimResult:
    """What a trim run leaves: output text, stderr text (the reference's log lines without timestamps), the per-read table
    (int32 [reads, 5], TRIM_TABLE_FIELDS), the adapters after determination as (side, name, matches) and the stats."""

    def __init__(self, H, h):
        n = C.c_int64(0)
        self.output = C.string_at(H.dph_trim_output(h, C.byref(n)), n.value).decode()
        self.stderr = C.string_at(H.dph_trim_errtext(h, C.byref(n)), n.value).decode()
        nr = H.dph_trim_table(h, None, 0)
        self.table = np.zeros((nr, 5), dtype=np.int32)
        H.dph_trim_table(h, self.table.ctypes.data, nr)
        ad = C.string_at(H.dph_trim_adapters(h, C.byref(n)), n.value).decode()
        self.adapters = [(ln.split("\t")[0], ln.split("\t")[1], int(ln.split("\t")[2])) for ln in ad.splitlines()]
        st = np.zeros(16, dtype=np.float64)
        H.dph_trim_stats(h, st.ctypes.data)
        self.stats = dict(zip(TRIM_STAT_FIELDS, st.tolist()))
        self._H, self._h = H, h

    def __iter__(self):
        """output, stderr, table, stats = trim_reads(...)"""
        return iter((self.output, self.stderr, self.table, self.stats))

    def demultiplex(self, path):
        """Demultiplex (sequence/seqio.go:460-523) into directory `path`; returns the number of files written."""
        rc = self._H.dph_trim_demultiplex(self._h, str(path).encode())
        if rc < 0:
            raise DpError("dph_trim_demultiplex: " + self._H.dph_last_error(None).decode())
        return rc

    def close(self):
        if self._h:
            self._H.dph_trim_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trim_reads(reads, front, back, k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5, tag_adapters=True,
               require_pairs=False, determine_adapters=True, device=0, verbosity=1):
    """reads: downpore_amd.overlap.Reads loaded with min_len=50 (commands/trim.go:35); front / back: the adapter files as Reads
    with min_len=0.  Runs adapter determination, end trimming and the writer on the GPU and returns a TrimResult (output text,
    stderr text, per-read table, stats); keep `reads` alive while the result is in use.  There is no CPU fallback."""
    H = _host()
    p = _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity)
    h = H.dph_trim_run(reads.h, front.h, back.h, p.ctypes.data, len(p), device)
    if not h:
        raise DpError("dph_trim_run: " + H.dph_last_error(None).decode())
    return TrimResult(H, h)


def trim_apply(reads, front, back, recs, counts, enabled=None, k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5,
               tag_adapters=True, require_pairs=False, verbosity=1):
    """The device-free half (dph_trim_apply): recs int32 [2 * eligible reads, 6] and counts as dp_trim_edges returns them for the
    adapter lists after determination; enabled: the determine flags over the adapters as loaded, or None."""
    H = _host()
    p = _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, enabled is not None, verbosity)
    r = np.ascontiguousarray(recs, dtype=np.int32).reshape(-1, 6)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    en = None if enabled is None else np.ascontiguousarray(enabled, dtype=np.uint8)
    h = H.dph_trim_apply(reads.h, front.h, back.h, p.ctypes.data, len(p), None if en is None else en.ctypes.data, r.ctypes.data,
                         len(r) // 2, c.ctypes.data)
    if not h:
        raise DpError("dph_trim_apply: " + H.dph_last_error(None).decode())
    return TrimResult(H, h)


def trim_index(front, back, k):
    """setupIndex (trim/trim.go:57-99) as dp_trim_setup takes it: dict of kmer_seed, n_seeds, segs, seg_off, lengths, is_barcode,
    pairs, n_front, n_back."""
    H = _host()
    n = len(front) + len(back)
    cap = 2 * (front.total_bases() + back.total_bases()) + n + 16
    ks = np.zeros(4 ** k if 0 < k < 12 else 1, dtype=np.uint16)
    segs = np.zeros(cap, dtype=np.int32)
    off = np.zeros(n + 1, dtype=np.uint64)
    ln = np.zeros(n, dtype=np.int32)
    bar = np.zeros(n, dtype=np.uint8)
    pairs = np.zeros(n, dtype=np.int32)
    ns = H.dph_trim_index(front.h, back.h, k, ks.ctypes.data, segs.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, bar.ctypes.data,
                          pairs.ctypes.data)
    if ns < 0:
        raise DpError("dph_trim_index: " + H.dph_last_error(None).decode())
    return dict(kmer_seed=ks, n_seeds=int(ns), segs=segs[:int(off[-1])].copy(), seg_off=off, lengths=ln, is_barcode=bar, pairs=pairs,
                n_front=len(front), n_back=len(back), k=k)


class TrimDevice:
    """One adapter index on the device (dp_trim_setup .. dp_trim_release)."""

    def __init__(self, index, device=0):
        L = load_library()
        vp = C.c_void_p
        L.dp_trim_setup.argtypes = [C.c_int, C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(vp)]
        L.dp_trim_edges.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.dp_trim_release.argtypes = [vp]
        L.dp_trim_release.restype = None
        L.dp_trim_error.restype = C.c_char_p
        L.dp_trim_error.argtypes = [vp]
        self.L = L
        self.n_adapters = index["n_front"] + index["n_back"]
        ix = {key: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for key, v in index.items()}
        h = vp()
        rc = L.dp_trim_setup(device, ix["k"], ix["kmer_seed"].ctypes.data, ix["n_seeds"], ix["n_front"], ix["n_back"], ix["segs"].ctypes.data,
                             ix["seg_off"].ctypes.data, ix["lengths"].ctypes.data, ix["is_barcode"].ctypes.data, ix["pairs"].ctypes.data,
                             C.byref(h))
        if rc != 0:
            raise DpError("dp_trim_setup failed (%d): %s" % (rc, L.dp_trim_error(None).decode()))
        self.h = h

    def edges(self, ends, mode=MODE_TRIM, min_match=3, threshold=90):
        """ends: uint8 [reads, 2, 150] ASCII.  Trim mode -> (recs int32 [2 * reads, 6], counts uint64, times_ms); determine mode ->
        (enabled uint8, times_ms).  Counts and flags accumulate over the calls on one set-up."""
        e = np.ascontiguousarray(ends, dtype=np.uint8).reshape(-1, 2 * EDGE)
        recs = np.zeros((2 * len(e), 6), dtype=np.int32)
        counts = np.zeros(self.n_adapters, dtype=np.uint64)
        enabled = np.zeros(self.n_adapters, dtype=np.uint8)
        times = np.zeros(3, dtype=np.float64)
        rc = self.L.dp_trim_edges(self.h, e.ctypes.data, len(e), mode, min_match, threshold, recs.ctypes.data, counts.ctypes.data,
                                  enabled.ctypes.data, times.ctypes.data)
        if rc != 0:
            raise DpError("dp_trim_edges failed (%d): %s" % (rc, self.L.dp_trim_error(self.h).decode()))
        return (recs, counts, times) if mode == MODE_TRIM else (enabled, times)

    def close(self):
        if getattr(self, "h", None):
            self.L.dp_trim_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
