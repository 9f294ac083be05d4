"""`downpore trim`, edge stage, on the GPU: Python front end of the C++ host mirror of trim.Trimmer (libdownpore_host.so) and a
thin binding of the device entry points behind it (dp_trim_setup / dp_trim_edges, libdownpore_hip.so)."""
import ctypes as C

import numpy as np

from .hip import DpError, load_library
from .overlap import load_host

TRIM_STAT_FIELDS = ["seen", "none", "reads", "front_adapters", "back_adapters", "t_determine_s", "t_extract_s", "upload_ms", "kernel_ms",
                    "download_ms", "t_apply_s", "t_write_s", "determine_kernel_ms", "bytes_up", "bytes_down",
                    "reserved"]  # (the writer's sixteenth double, always 0: the list is as long as DPH_TRIM_STATS says)
#: columns of the per-read table
TRIM_TABLE_FIELDS = ["front_trim", "back_trim", "ignore", "front_adapter", "back_adapter"]
#: fields of one edge record (dp_trim_rec)
TRIM_REC_FIELDS = ["earliest", "latest", "found", "best_match", "ambiguous", "best_ident"]
#: the middle stage's stats, columns of its plan / split / record tables
TRIM_MID_STAT_FIELDS = ["mid_chunks", "mid_seeds", "mid_batches", "mid_pairs", "mid_records", "mid_overflow_pairs", "mid_out_of_range",
                        "mid_upload_ms", "mid_scan_ms", "mid_index_ms", "mid_query_ms", "mid_kernel_ms"]
TRIM_PLAN_FIELDS = ["read", "start", "end", "remainder", "seeds", "indexed"]
TRIM_SPLIT_FIELDS = ["read", "a_end", "b_start", "kept"]
TRIM_MID_REC_FIELDS = ["adapter", "chunk", "ordinal", "start_rel", "covered", "chain_len"]
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
    H.dph_trim_apply_mid.restype = vp
    H.dph_trim_apply_mid.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, C.c_int64, vp, vp, C.c_int64, vp, C.c_int64]
    H.dph_trim_chunk_plan.restype = C.c_int64
    H.dph_trim_chunk_plan.argtypes = [C.c_int64, C.c_int64, vp, C.c_int64]
    H.dph_trim_mid_ints.restype = C.c_int64
    H.dph_trim_mid_ints.argtypes = [vp, C.c_int, vp, C.c_int64]
    H.dph_trim_extras.restype = C.POINTER(C.c_char)
    H.dph_trim_extras.argtypes = [vp, C.POINTER(C.c_int64)]
    H.dph_trim_mid_stats.argtypes = [vp, vp]
    H.dph_trim_reads.restype = vp
    H.dph_trim_reads.argtypes = [vp, C.c_int64, C.c_int]
    return H


def _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity):
    return np.array([k, check_reads, adapter_threshold, extra_end_trim, 1 if tag_adapters else 0, 1 if require_pairs else 0,
                     1 if determine_adapters else 0, verbosity], dtype=np.int64)


def _mid_params(edge, chunk_size, middle_threshold, extra_middle_trim, discard_middle, flush_seeds):
    return np.concatenate([edge, np.array([1, chunk_size, middle_threshold, extra_middle_trim, 1 if discard_middle else 0, flush_seeds],
                                          dtype=np.int64)])


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
        st = np.zeros(len(TRIM_STAT_FIELDS), dtype=np.float64)
        H.dph_trim_stats(h, st.ctypes.data)
        self.stats = dict(zip(TRIM_STAT_FIELDS, st.tolist()))
        # the middle stage (empty / zero when it did not run)
        def ints(which, width):
            m = H.dph_trim_mid_ints(h, which, None, 0)
            a = np.zeros(m, dtype=np.int32)
            H.dph_trim_mid_ints(h, which, a.ctypes.data, m)
            return a.reshape(-1, width)

        self.plan, self.splits, self.applied = ints(0, 6), ints(1, 4), ints(2, 6)
        self.extras = C.string_at(H.dph_trim_extras(h, C.byref(n)), n.value).decode().splitlines()
        ms = np.zeros(len(TRIM_MID_STAT_FIELDS), dtype=np.float64)
        H.dph_trim_mid_stats(h, ms.ctypes.data)
        self.stats.update(zip(TRIM_MID_STAT_FIELDS, ms.tolist()))
        self._H, self._h = H, h

    def __iter__(self):
        """output, stderr, table, stats = trim_reads(...)"""
        return iter((self.output, self.stderr, self.table, self.stats))

    def reads(self, min_len, himem=True):
        """The read set `output` gives when it is read back with Reads(fasta=..., min_len=min_len) - the non-ignored reads trimmed, then
        the halves of split reads - without the text (dph_trim_reads; no device needed).  This is how a consumer such as map_reads
        gets trimmed reads without a file.  Keep the reads the trim ran on alive while calling it."""
        from .overlap import Reads
        h = self._H.dph_trim_reads(self._h, min_len, 1 if himem else 0)
        if not h:
            raise DpError("dph_trim_reads: " + self._H.dph_last_error(None).decode())
        return Reads._wrap(h)

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


def trim_params(k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5, tag_adapters=True, require_pairs=False, determine_adapters=True,
                verbosity=1, middle=False, chunk_size=5000, middle_threshold=85, extra_middle_trim=100, discard_middle=False, flush_seeds=300_000_000):
    """trim_reads' keyword arguments as the int64 parameter block dph_trim_run / dph_overlap_open_trim take"""
    p = _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity)
    return _mid_params(p, chunk_size, middle_threshold, extra_middle_trim, discard_middle, flush_seeds) if middle else p


def trim_reads(reads, front, back, k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5, tag_adapters=True,
               require_pairs=False, determine_adapters=True, device=0, verbosity=1, middle=False, chunk_size=5000, middle_threshold=85,
               extra_middle_trim=100, discard_middle=False, flush_seeds=300_000_000):
    """reads: downpore_amd.overlap.Reads loaded with min_len=50 (commands/trim.go:35); front / back: the adapter files as Reads
    with min_len=0.  Runs adapter determination, end trimming and the writer on the GPU and returns a TrimResult (output text,
    stderr text, per-read table, stats); keep `reads` alive while the result is in use.  There is no CPU fallback.
    middle=True adds the search for front adapters in the middle of reads (trim/trim.go:151-256): reads are cropped or split, the
    halves of split reads follow the file's reads as <name>_(left) / <name>_(right) (TrimResult.splits / .extras; needs k >= 4).
    middle=False is the edge stage alone."""
    H = _host()
    p = trim_params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity, middle, chunk_size,
                    middle_threshold, extra_middle_trim, discard_middle, flush_seeds)
    h = H.dph_trim_run(reads.h, front.h, back.h, p.ctypes.data, len(p), device)
    if not h:
        raise DpError("dph_trim_run: " + H.dph_last_error(None).decode())
    return TrimResult(H, h)


def _apply(reads, front, back, recs, counts, enabled, p, middle=None):
    """dph_trim_apply, or dph_trim_apply_mid when middle = (seed_counts, mid_recs)"""
    H = _host()
    r = np.ascontiguousarray(recs, dtype=np.int32).reshape(-1, 6)
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    en = None if enabled is None else np.ascontiguousarray(enabled, dtype=np.uint8)
    f, more = H.dph_trim_apply, []
    if middle is not None:
        sc = np.ascontiguousarray(middle[0], dtype=np.int32)
        mr = np.ascontiguousarray(middle[1], dtype=np.int32).reshape(-1, 6)
        f, more = H.dph_trim_apply_mid, [sc.ctypes.data, len(sc), mr.ctypes.data, len(mr)]
    h = f(reads.h, front.h, back.h, p.ctypes.data, len(p), None if en is None else en.ctypes.data, r.ctypes.data, len(r) // 2, c.ctypes.data, *more)
    if not h:
        raise DpError(f.__name__ + ": " + H.dph_last_error(None).decode())
    return TrimResult(H, h)


def trim_apply(reads, front, back, recs, counts, enabled=None, k=6, check_reads=10000, adapter_threshold=90, extra_end_trim=5,
               tag_adapters=True, require_pairs=False, verbosity=1):
    """The device-free half (dph_trim_apply): recs int32 [2 * eligible reads, 6] and counts as dp_trim_edges returns them for the
    adapter lists after determination; enabled: the determine flags over the adapters as loaded, or None."""
    p = _params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, enabled is not None, verbosity)
    return _apply(reads, front, back, recs, counts, enabled, p)


def trim_apply_middle(reads, front, back, recs, counts, seed_counts, mid_recs, enabled=None, k=6, check_reads=10000, adapter_threshold=90,
                      extra_end_trim=5, tag_adapters=True, require_pairs=False, verbosity=1, chunk_size=5000, middle_threshold=85,
                      extra_middle_trim=100, discard_middle=False, flush_seeds=300_000_000):
    """trim_apply followed by the middle stage's sequential half (dph_trim_apply_mid), without a device: seed_counts = seeds of every
    planned chunk (trim_chunk_plan over the edge-trimmed reads, in file order), mid_recs int32 [n, 6] (TRIM_MID_REC_FIELDS) = the matches
    that passed the identity test, in any order."""
    p = _mid_params(_params(k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, enabled is not None, verbosity),
                    chunk_size, middle_threshold, extra_middle_trim, discard_middle, flush_seeds)
    return _apply(reads, front, back, recs, counts, enabled, p, (seed_counts, mid_recs))


def trim_chunk_plan(length, chunk_size):
    """The chunks the middle stage cuts from an edge-trimmed read of `length` bases (trim/trim.go:165-184): int32 [n, 3] =
    start, end, is-remainder.  chunk_size <= 100 is refused (the reference's loop would not end)."""
    H = _host()
    n = H.dph_trim_chunk_plan(length, chunk_size, None, 0)
    if n < 0:
        raise DpError("dph_trim_chunk_plan: " + H.dph_last_error(None).decode())
    out = np.zeros((max(n, 1), 3), dtype=np.int32)
    H.dph_trim_chunk_plan(length, chunk_size, out.ctypes.data, n)
    return out[:n]


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


class MidBatch(C.Structure):
    """dp_trim_mid_batch"""
    _fields_ = [("n_recs", C.c_uint32), ("recs", C.c_void_p), ("n_overflow", C.c_uint32), ("overflow", C.POINTER(C.c_uint32)),
                ("n_pairs", C.c_uint32), ("launches", C.c_uint32), ("index_ms", C.c_double), ("query_ms", C.c_double), ("kernel_ms", C.c_double)]


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
        L.dp_trim_scan_chunks.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
        L.dp_trim_chunk_segments.argtypes = [vp, C.c_uint32, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.dp_trim_search.argtypes = [vp, vp, C.c_uint32, C.c_int, C.POINTER(MidBatch)]
        L.dp_trim_edges_resident.argtypes = [vp, vp, vp, C.c_uint32, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
        L.dp_trim_scan_chunks_resident.argtypes = [vp, vp, vp, C.c_uint32, vp, vp]
        self.L = L
        self.n_adapters = index["n_front"] + index["n_back"]
        ix = {key: (np.ascontiguousarray(v) if isinstance(v, np.ndarray) else v) for key, v in index.items()}
        h = vp()
        rc = L.dp_trim_setup(device, ix["k"], ix["kmer_seed"].ctypes.data, ix["n_seeds"], ix["n_front"], ix["n_back"], ix["segs"].ctypes.data,
                             ix["seg_off"].ctypes.data, ix["lengths"].ctypes.data, ix["is_barcode"].ctypes.data, ix["pairs"].ctypes.data,
                             C.byref(h))
        self._check(rc, "dp_trim_setup")
        self.h = h

    def _check(self, rc, what):
        if rc != 0:
            raise DpError("%s failed (%d): %s" % (what, rc, self.L.dp_trim_error(getattr(self, "h", None)).decode()))  # (no handle: the set-up's text)

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
        self._check(rc, "dp_trim_edges")
        return (recs, counts, times) if mode == MODE_TRIM else (enabled, times)

    def edges_resident(self, ctx, read_ids, mode=MODE_TRIM, min_match=3, threshold=90):
        """edges() for reads the Context `ctx` holds resident (dp_trim_edges_resident): read_ids = the reads, each of 200 bases or more;
        their ends are spelled on the device and only the ids go up.  Returns what edges() returns."""
        ids = np.ascontiguousarray(read_ids, dtype=np.uint32)
        recs = np.zeros((2 * len(ids), 6), dtype=np.int32)
        counts = np.zeros(self.n_adapters, dtype=np.uint64)
        enabled = np.zeros(self.n_adapters, dtype=np.uint8)
        times = np.zeros(3, dtype=np.float64)
        rc = self.L.dp_trim_edges_resident(self.h, ctx.h, ids.ctypes.data, len(ids), mode, min_match, threshold, recs.ctypes.data, counts.ctypes.data,
                                           enabled.ctypes.data, times.ctypes.data)
        self._check(rc, "dp_trim_edges_resident")
        return (recs, counts, times) if mode == MODE_TRIM else (enabled, times)

    def scan_chunks_resident(self, ctx, spans):
        """scan_chunks() with chunk c = bases [start, start + len) of resident read `read` of the Context `ctx`: spans uint32 [n, 3] =
        (read, start, len).  Returns what scan_chunks() returns; chunk_segments / search follow as usual."""
        sp = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 3)
        counts = np.zeros(len(sp), dtype=np.uint32)
        times = np.zeros(2, dtype=np.float64)
        rc = self.L.dp_trim_scan_chunks_resident(self.h, ctx.h, sp.ctypes.data, len(sp), counts.ctypes.data, times.ctypes.data)
        self._check(rc, "dp_trim_scan_chunks_resident")
        return counts, times

    def scan_chunks(self, chunks):
        """dp_trim_scan_chunks: chunks = a list of ASCII base strings (or bytes) -> (seeds per chunk uint32, times_ms [upload, scan]).
        The segments stay on the device for chunk_segments / search until the next scan."""
        raw = [c.encode() if isinstance(c, str) else bytes(c) for c in chunks]
        off = np.zeros(len(raw) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c) for c in raw], dtype=np.uint64)
        bases = np.frombuffer(b"".join(raw) + b"\0", dtype=np.uint8)
        counts = np.zeros(len(raw), dtype=np.uint32)
        times = np.zeros(2, dtype=np.float64)
        rc = self.L.dp_trim_scan_chunks(self.h, bases.ctypes.data, off.ctypes.data, len(raw), counts.ctypes.data, times.ctypes.data)
        self._check(rc, "dp_trim_scan_chunks")
        return counts, times

    def chunk_segments(self, chunk):
        """The [gap, seed, ..., gap] segments of one chunk of the last scan (int32)."""
        n = C.c_uint64(0)
        rc = self.L.dp_trim_chunk_segments(self.h, chunk, None, 0, C.byref(n))
        out = np.zeros(max(int(n.value), 1), dtype=np.int32)
        if rc == 0:
            rc = self.L.dp_trim_chunk_segments(self.h, chunk, out.ctypes.data, len(out), C.byref(n))
        self._check(rc, "dp_trim_chunk_segments")
        return out[:int(n.value)]

    def search(self, sel, middle_threshold=85):
        """dp_trim_search over the chunks `sel` (ascending ids of the last scan) -> dict(recs int32 [n, 6] (TRIM_MID_REC_FIELDS, sorted
        by adapter, chunk, ordinal), overflow uint32 [m, 2] (chunk, adapter), pairs, launches, index_ms, query_ms, kernel_ms)."""
        s = np.ascontiguousarray(sel, dtype=np.uint32)
        b = MidBatch()
        rc = self.L.dp_trim_search(self.h, s.ctypes.data, len(s), middle_threshold, C.byref(b))
        self._check(rc, "dp_trim_search")
        recs = np.ctypeslib.as_array(C.cast(b.recs, C.POINTER(C.c_int32)), shape=(b.n_recs, 6)).copy() if b.n_recs else np.zeros((0, 6), dtype=np.int32)
        over = np.ctypeslib.as_array(b.overflow, shape=(b.n_overflow, 2)).copy() if b.n_overflow else np.zeros((0, 2), dtype=np.uint32)
        return dict(recs=recs, overflow=over, pairs=b.n_pairs, launches=b.launches, index_ms=b.index_ms, query_ms=b.query_ms, kernel_ms=b.kernel_ms)

    def close(self):
        if getattr(self, "h", None):
            self.L.dp_trim_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
