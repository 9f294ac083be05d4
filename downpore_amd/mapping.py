"""`downpore map` on the GPU: Python front end of the C++ host mirror of mapping.Mapper (libdownpore_host.so)."""
import ctypes as C

import numpy as np

from .hip import DpError
from .overlap import load_host

MAP_STAT_FIELDS = ["n_chunks", "n_seeds", "n_windows", "n_chains", "n_batches", "k_scan_ms", "k_map_ms", "t_setup_s", "t_scan_s",
                   "t_chain_s", "t_host_s", "map_bytes", "scan_bytes"]
#: dph_map_index_info's values, in order (the "index" entry of the stats)
MAP_INDEX_FIELDS = ["layout", "index_bytes", "dense_estimate", "device_total", "hits", "index_builds", "q_ladder8", "q_ladder16",
                    "q_exact", "q_big"]
#: dph_map_align_info's values, in order (the "align" entry of map_aligned's stats)
MAP_ALIGN_FIELDS = ["lines", "aligned", "over_max_edits", "out_of_range", "cells", "band_doublings", "kernel_us", "traceback_bytes"]
INDEX_LAYOUTS = {"auto": 0, "dense": 1, "sparse": 2}


def index_layout_code(index):
    """"auto" / "dense" / "sparse" (or 0 / 1 / 2) -> the layout code of dph_map_run_ex; anything else raises DpError."""
    if isinstance(index, str) and index in INDEX_LAYOUTS:
        return INDEX_LAYOUTS[index]
    if isinstance(index, (int, np.integer)) and not isinstance(index, bool) and 0 <= int(index) <= 2:
        return int(index)
    raise DpError("map_reads: index must be 'auto', 'dense' or 'sparse' (0, 1, 2), not %r" % (index,))


def _trim_block(trim):
    """map_reads' trim=dict(front=Reads, back=Reads, **keyword arguments of trim_params) -> (front, back, parameter block); a missing
    front / back or an unknown key raises DpError before any library call."""
    import inspect

    from . import trim as T
    if not isinstance(trim, dict):
        raise DpError("map_reads: trim must be a dict(front=Reads, back=Reads, ...), not %r" % (type(trim).__name__,))
    kw = dict(trim)
    missing = [key for key in ("front", "back") if kw.get(key) is None]
    if missing:
        raise DpError("map_reads: trim lacks %s (the adapter files as Reads loaded with min_len=0)" % " and ".join(repr(m) for m in missing))
    front, back = kw.pop("front"), kw.pop("back")
    known = list(inspect.signature(T.trim_params).parameters)
    unknown = sorted(key for key in kw if key not in known)
    if unknown:
        raise DpError("map_reads: unknown trim key %s (known: front, back, %s)" % (", ".join(repr(u) for u in unknown), ", ".join(known)))
    return front, back, T.trim_params(**kw)


def _result_types(H):
    """ctypes signatures of the calls that read a map handle (dph_map_run_ex's or dph_mapper_map's)."""
    H.dph_map_free.argtypes = [C.c_void_p]
    for f in (H.dph_map_paf, H.dph_map_errtext):
        f.restype = C.POINTER(C.c_char)
        f.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    H.dph_map_stats.argtypes = [C.c_void_p, C.c_void_p]
    H.dph_map_index_info.restype = C.c_int
    H.dph_map_index_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int]


def _take_result(H, h, align=False):
    """(paf, stderr_text, stats) of a map handle, which is freed; align: with stats["align"] (dph_map_align_info)."""
    n = C.c_int64(0)
    paf = C.string_at(H.dph_map_paf(h, C.byref(n)), n.value).decode()
    err = C.string_at(H.dph_map_errtext(h, C.byref(n)), n.value).decode()
    st = np.zeros(len(MAP_STAT_FIELDS), dtype=np.float64)
    H.dph_map_stats(h, st.ctypes.data)
    ix = np.zeros(len(MAP_INDEX_FIELDS), dtype=np.int64)
    got = H.dph_map_index_info(h, ix.ctypes.data, len(ix))
    al = np.zeros(len(MAP_ALIGN_FIELDS), dtype=np.int64)
    if align:
        H.dph_map_align_info.restype = C.c_int
        H.dph_map_align_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        H.dph_map_align_info(h, al.ctypes.data, len(al))
    H.dph_map_free(h)
    stats = dict(zip(MAP_STAT_FIELDS, st.tolist()))
    info = dict(zip(MAP_INDEX_FIELDS[:got], (int(v) for v in ix[:got])))
    info["layout"] = {1: "dense", 2: "sparse"}.get(info.get("layout", 0), "none")
    stats["index"] = info
    if align:
        stats["align"] = dict(zip(MAP_ALIGN_FIELDS, (int(v) for v in al)))
    return paf, err, stats


class Mapper:
    """A reference opened once, batches of reads mapped against it: `with Mapper(ref) as m: paf, err, stats = m.map(reads)`.
    The reference's sequences and join chunks, its value table, seeds, chunk scan and index are made by the constructor and stay on
    the device; map(reads) sends the batch alone and returns what map_reads(ref, reads, ...) returns, text for text.  Arguments as
    map_reads takes them, its trim among them, per batch: map(raw, trim=dict(front=..., back=..., ...)) trims the batch first on the
    device's copy, as map_reads(ref, raw, trim=...) does.  One map() at a time per mapper; DpError on use after close()."""

    def __init__(self, ref, circular=True, k=11, query_size=1000, min_length=500, chunk_size=10000, seed_rate=40, device=0,
                 index="auto", all_sequences=False):
        self.h = None
        layout = index_layout_code(index)
        H = self.H = load_host()
        H.dph_mapper_open.restype = C.c_void_p
        H.dph_mapper_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        H.dph_mapper_map.restype = C.c_void_p
        H.dph_mapper_map.argtypes = [C.c_void_p, C.c_void_p]
        H.dph_mapper_map_trim.restype = C.c_void_p
        H.dph_mapper_map_trim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        H.dph_mapper_close.argtypes = [C.c_void_p]
        _result_types(H)
        p = np.array([1 if circular else 0, k, query_size, min_length, chunk_size, seed_rate, layout, 1 if all_sequences else 0], dtype=np.int64)
        self.ref = ref  # (the library reads the reference through the mapper's lifetime)
        h = H.dph_mapper_open(ref.h, p.ctypes.data, len(p), device)
        if not h:
            raise DpError("dph_mapper_open: " + H.dph_last_error(None).decode())
        self.h = h

    def map(self, reads, trim=None):
        """-> (paf, stderr_text, stats) exactly as map_reads returns them for (ref, reads), or with trim - the dict map_reads takes,
        `reads` then being the raw set loaded with min_len=50 - for (ref, reads, trim=trim): the batch goes up once, 2-bit packed,
        both trim stages run on the device's copy behind the resident reference, and the reads that are mapped are cut from it on
        the device (dph_mapper_map_trim); stats["trim"] is the trim's TrimResult (keep `reads` alive while it is in use).  A trim
        refused for its parameters or its input raises DpError and leaves the mapper usable."""
        trim_block = None if trim is None else _trim_block(trim)  # (refused before any library call)
        if not getattr(self, "h", None):
            raise DpError("Mapper.map: the mapper is closed")
        if trim_block is None:
            h = self.H.dph_mapper_map(self.h, reads.h)
            if not h:
                raise DpError("dph_mapper_map: " + self.H.dph_last_error(None).decode())
            return _take_result(self.H, h)
        from . import trim as T
        front, back, tp = trim_block
        th = C.c_void_p()
        h = self.H.dph_mapper_map_trim(self.h, reads.h, front.h, back.h, tp.ctypes.data, len(tp), C.byref(th))
        if not h:
            raise DpError("dph_mapper_map_trim: " + self.H.dph_last_error(None).decode())
        trim_result = T.TrimResult(T._host(), th)
        paf, err, stats = _take_result(self.H, h)
        stats["trim"] = trim_result
        return paf, err, stats

    def map_aligned(self, reads, trim=None, max_edits=4096):
        """map(reads, trim) with the base-level alignment of every PAF line behind its column 12: "\\tNM:i:<edit distance>\\tcg:Z:<CIGAR>"
        (unit costs, M for matches and mismatches, gaps at the left end of a tie), computed on the device over the reads
        and the reference it holds anyway (dph_mapper_map_align).  Columns 1 - 12, the lines' order, the stderr text and every other
        stats key are map's.  A line whose edit distance exceeds max_edits (1 .. 32768) or whose coordinates lie outside its read or
        sequence gets no tags; stats["align"] counts them (MAP_ALIGN_FIELDS).  A refused max_edits raises DpError and leaves the mapper
        usable."""
        trim_block = None if trim is None else _trim_block(trim)
        if isinstance(max_edits, bool) or not isinstance(max_edits, (int, np.integer)) or not 1 <= int(max_edits) <= 32768:
            raise DpError("Mapper.map_aligned: max_edits must be an integer in 1 .. 32768, not %r" % (max_edits,))
        if not getattr(self, "h", None):
            raise DpError("Mapper.map_aligned: the mapper is closed")
        H = self.H
        H.dph_mapper_map_align.restype = C.c_void_p
        H.dph_mapper_map_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
        ap = np.array([int(max_edits)], dtype=np.int64)
        th = C.c_void_p()
        if trim_block is None:
            h = H.dph_mapper_map_align(self.h, reads.h, None, None, None, 0, C.byref(th), ap.ctypes.data, 1)
        else:
            front, back, tp = trim_block
            h = H.dph_mapper_map_align(self.h, reads.h, front.h, back.h, tp.ctypes.data, len(tp), C.byref(th), ap.ctypes.data, 1)
        if not h:
            raise DpError("dph_mapper_map_align: " + H.dph_last_error(None).decode())
        trim_result = None
        if trim_block is not None:
            from . import trim as T
            trim_result = T.TrimResult(T._host(), th)
        paf, err, stats = _take_result(H, h, align=True)
        if trim_result is not None:
            stats["trim"] = trim_result
        return paf, err, stats

    def close(self):
        if getattr(self, "h", None):
            self.H.dph_mapper_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def map_reads(ref, reads, circular=True, k=11, query_size=1000, min_length=500, chunk_size=10000, seed_rate=40, device=0,
              index="auto", all_sequences=False, trim=None):
    """ref / reads: downpore_amd.overlap.Reads (reference loaded with min_len=0, reads with min_len=min_length; both are
    treated as top-level sequences exactly like commands/map.go does).  index: the reference index's layout ("auto" takes the
    sparse one when the dense one would not fit the device; both give the same PAF).  all_sequences: map against every sequence of
    ref (one seed index and one chunk index over all of them; a PAF line names the sequence it lies on), not the first one only.
    trim: dict(front=Reads, back=Reads, **keyword arguments of trim_reads) = `downpore trim` first, on the reads the device holds
    anyway (dph_map_run_trim): `reads` (then loaded with min_len=50, as `trim` loads them) go up once, 2-bit packed, both trim stages
    run on the resident copy, and the reads that are mapped are cut from it on the device with their reverse strands - the PAF is
    that of map_reads(ref, trim_reads(reads, ...).reads(min_length), ...) without the bases crossing the link again.  The trim runs
    on `device`; stats["trim"] is its TrimResult (no output text; keep `reads` alive while it is in use).
    Returns (paf, stderr_text, stats);
    stats["index"] describes the index (MAP_INDEX_FIELDS, layout "dense" / "sparse")."""
    layout = index_layout_code(index)
    trim_block = None if trim is None else _trim_block(trim)
    H = load_host()
    H.dph_map_run_ex.restype = C.c_void_p
    H.dph_map_run_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    _result_types(H)
    p = np.array([1 if circular else 0, k, query_size, min_length, chunk_size, seed_rate, layout, 1 if all_sequences else 0], dtype=np.int64)
    trim_result = None
    if trim_block is None:
        h = H.dph_map_run_ex(ref.h, reads.h, p.ctypes.data, len(p), device)
        if not h:
            raise DpError("dph_map_run: " + H.dph_last_error(None).decode())
    else:
        from . import trim as T
        front, back, tp = trim_block
        H.dph_map_run_trim.restype = C.c_void_p
        H.dph_map_run_trim.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]
        th = C.c_void_p()
        h = H.dph_map_run_trim(ref.h, reads.h, front.h, back.h, tp.ctypes.data, len(tp), p.ctypes.data, len(p), device, C.byref(th))
        if not h:
            raise DpError("dph_map_run_trim: " + H.dph_last_error(None).decode())
        trim_result = T.TrimResult(T._host(), th)
    paf, err, stats = _take_result(H, h)
    if trim_result is not None:
        stats["trim"] = trim_result
    return paf, err, stats


def map_reads_aligned(ref, reads, circular=True, k=11, query_size=1000, min_length=500, chunk_size=10000, seed_rate=40, device=0,
                      index="auto", all_sequences=False, trim=None, max_edits=4096):
    """map_reads with NM and cg tags behind every PAF line (Mapper.map_aligned): opens a Mapper on `ref`, maps the one batch `reads`
    and closes it.  Because it goes through a Mapper, DP_MAP_SHARDS > 1 and the ASCII upload keys (DP_TUNE=map_ascii_upload /
    map_async_upload) are not available to it: they are refused by name, as Mapper refuses them.  Returns (paf, stderr_text, stats)
    with stats["align"]."""
    with Mapper(ref, circular=circular, k=k, query_size=query_size, min_length=min_length, chunk_size=chunk_size, seed_rate=seed_rate,
                device=device, index=index, all_sequences=all_sequences) as m:
        return m.map_aligned(reads, trim=trim, max_edits=max_edits)
