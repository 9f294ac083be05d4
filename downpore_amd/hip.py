"""ctypes binding of libdownpore_hip.so (C ABI: include/downpore_hip.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_dir():
    # DP_LIB_DIR: another build of both libraries (make LIB=../lib_prof PROF=1, make LIB=../lib_copylog COPYLOG=1: diagnosis builds)
    return os.environ.get("DP_LIB_DIR") or os.path.join(_HERE, "lib")


def lib_path():
    return os.path.join(lib_dir(), "libdownpore_hip.so")


class DpError(RuntimeError):
    pass


class SeedSeqBatch(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("n_seeds", C.POINTER(C.c_uint32)), ("seg_off", C.POINTER(C.c_uint64)),
                ("segs", C.POINTER(C.c_int32)), ("n_segs", C.c_uint64), ("kernel_ms", C.c_double),
                ("count_kernel_ms", C.c_double), ("write_kernel_ms", C.c_double), ("bases_scanned", C.c_uint64)]


class SurvivorBatch(C.Structure):
    _fields_ = [("n_survivors", C.c_uint32), ("read", C.POINTER(C.c_uint32)), ("n_seeds", C.POINTER(C.c_uint32)),
                ("seg_off", C.POINTER(C.c_uint64)), ("n_extra", C.c_uint32), ("extra_n_seeds", C.POINTER(C.c_uint32)),
                ("extra_seg_off", C.POINTER(C.c_uint64)), ("segs", C.POINTER(C.c_int32)), ("n_segs", C.c_uint64),
                ("kernel_ms", C.c_double), ("count_kernel_ms", C.c_double), ("write_kernel_ms", C.c_double),
                ("bases_scanned", C.c_uint64), ("reads_scanned", C.c_uint32), ("index_mode", C.c_uint32),
                ("index_hits", C.c_uint64)]


class MatchBatch(C.Structure):
    _fields_ = [("n_matches", C.c_uint32), ("query", C.POINTER(C.c_uint32)), ("target", C.POINTER(C.c_uint32)),
                ("off", C.POINTER(C.c_uint64)), ("match_a", C.POINTER(C.c_int32)), ("match_b", C.POINTER(C.c_int32)),
                ("target_anchor", C.POINTER(C.c_int32)), ("n_queries", C.c_uint32), ("cand_off", C.POINTER(C.c_uint64)), ("cand", C.POINTER(C.c_uint32)),
                ("query_kernel_ms", C.c_double), ("chain_kernel_ms", C.c_double), ("query_bytes", C.c_uint64),
                ("chain_bytes", C.c_uint64)]


class ChainBatch(C.Structure):
    _fields_ = [("n_chains", C.c_uint32), ("window", C.POINTER(C.c_uint32)), ("target", C.POINTER(C.c_uint32)),
                ("off", C.POINTER(C.c_uint64)), ("match_a", C.POINTER(C.c_int32)), ("match_b", C.POINTER(C.c_int32)),
                ("kernel_ms", C.c_double), ("alg_bytes", C.c_double)]


class SingleSeedBatch(C.Structure):  # dp_single_seed_batch
    _fields_ = [("n_windows", C.c_uint32), ("best", C.POINTER(C.c_uint32)), ("cand_off", C.POINTER(C.c_uint32)),
                ("cand", C.POINTER(C.c_uint32))]


class SingleSeedMultiBatch(C.Structure):  # dp_single_seed_multi_batch
    _fields_ = [("n_windows", C.c_uint32), ("n_reads", C.c_uint32), ("best", C.POINTER(C.c_uint32)),
                ("cand_off", C.POINTER(C.c_uint32)), ("cand", C.POINTER(C.c_uint32)), ("win_off", C.POINTER(C.c_uint32))]


class CandidateBatch(C.Structure):  # dp_candidate_batch
    _fields_ = [("n_queries", C.c_uint32), ("cand_off", C.POINTER(C.c_uint64)), ("cand", C.POINTER(C.c_uint32)),
                ("meta", C.POINTER(C.c_uint32))]


class ConsensusBatch(C.Structure):  # dp_consensus_batch
    _fields_ = [("n_groups", C.c_uint32), ("cons", C.POINTER(C.c_int32)), ("cons_off", C.POINTER(C.c_uint64)),
                ("cons_len", C.POINTER(C.c_uint32)), ("match_a", C.POINTER(C.c_int32)), ("match_b", C.POINTER(C.c_int32)),
                ("match_len", C.POINTER(C.c_uint32)), ("flags", C.POINTER(C.c_uint32)), ("kernel_ms", C.c_double)]


class PafBatch(C.Structure):  # dp_paf_batch
    _fields_ = [("n_groups", C.c_uint32), ("groups", C.c_void_p), ("paf", C.c_void_p), ("ignore_ids", C.POINTER(C.c_uint32)),
                ("kernel_ms", C.c_double), ("n_indexed", C.c_uint32), ("query_kernel_ms", C.c_double), ("chain_kernel_ms", C.c_double),
                ("query_bytes", C.c_uint64), ("chain_bytes", C.c_uint64), ("index_kernel_ms", C.c_double)]


SEQ_META = np.dtype([("read", np.uint32), ("length", np.int32), ("offset", np.int32), ("inset", np.int32)])  # dp_seq_meta
PAF_REC = np.dtype([("q_read", np.uint32), ("t_read", np.uint32), ("q_len", np.int32), ("q_start", np.int32), ("q_end", np.int32),
                    ("t_len", np.int32), ("t_start", np.int32), ("t_end", np.int32), ("ident", np.int32), ("minus", np.uint32)])  # dp_paf_rec
GROUP_META = np.dtype([("slot", np.uint32), ("n_lines", np.uint32), ("n_ignore", np.uint32), ("bad_back", np.uint32),
                       ("empty_match", np.uint32), ("flag", np.uint32), ("n_matches", np.uint32), ("reserved", np.uint32)])  # dp_group_meta


class IndexInfo(C.Structure):  # dp_index_info_t
    _fields_ = [("layout", C.c_uint32), ("borrowed", C.c_uint32), ("n_seeds", C.c_uint32), ("n_seqs", C.c_uint32),
                ("device_bytes", C.c_uint64), ("entries", C.c_uint64), ("queries", C.c_uint64 * 4)]


class AlignBatch(C.Structure):  # dp_align_batch
    _fields_ = [("n", C.c_uint32), ("recs", C.c_void_p), ("runs", C.POINTER(C.c_uint32)), ("n_runs", C.c_uint64), ("cells", C.c_uint64),
                ("tb_bytes", C.c_uint64), ("doublings", C.c_uint32), ("kernel_ms", C.c_double)]


ALIGN_ITEM = np.dtype([("q_read", np.uint32), ("q_off", np.uint32), ("q_len", np.uint32), ("t_read", np.uint32), ("t_off", np.uint32),
                       ("t_len", np.uint32)])  # dp_align_item
ALIGN_REC = np.dtype([("nm", np.int32), ("n_runs", np.uint32), ("run_off", np.uint64)])  # dp_align_rec


#: every entry point include/downpore_hip.h declares (checked by the CPU-side symbol test)
SYMBOLS = ["dp_version", "dp_ctx_create", "dp_ctx_create_shared", "dp_ctx_set_priority", "dp_ctx_destroy", "dp_last_error", "dp_reads_upload", "dp_reads_packed",
           "dp_reads_count", "dp_reads_total_bases", "dp_kmer_histogram", "dp_kmer_values", "dp_round_begin", "dp_scan", "dp_scan_prepare", "dp_scan_reads", "dp_index_build",
           "dp_find_overlaps", "dp_query_prestage", "dp_map_windows", "dp_index_posting_row", "dp_index_seedset_row", "dp_scan_device_buffers",
           "dp_scan_import_segments", "dp_values_upload", "dp_select_seeds", "dp_reads_upload_rc", "dp_consensus_align", "dp_scan_release", "dp_consensus_paf", "dp_fetch_overlaps", "dp_select_windows", "dp_values_download",
    "dp_values_download_codes", "dp_values_download_codes8", "dp_index_build_chunked", "dp_index_prechain", "dp_index_prechained", "dp_index_chunks", "dp_scan_fetch_mode", "dp_scan_fetch_segments", "dp_set_stream_wait", "dp_set_kernel_timing", "dp_index_meta", "dp_index_set_global", "dp_map_windows_shard", "dp_single_seed_candidates", "dp_single_seed_candidates_multi", "dp_comm_unique_id", "dp_comm_init", "dp_comm_init_local", "dp_quality_upload",
           "dp_comm_destroy", "dp_comm_abort", "dp_allgather_blobs", "dp_gather_blobs", "dp_kindex_set_comm", "dp_kindex_digest", "dp_kindex_dump", "dp_release_device_caches", "dp_reads_upload_rc_begin", "dp_reads_upload_wait", "dp_reads_upload_packed_rc", "dp_host_alloc", "dp_host_free", "dp_comm_rank", "dp_comm_size", "dp_allgather_survivors",
           "dp_index_build_sparse", "dp_index_borrow", "dp_index_info", "dp_device_memory", "dp_query_candidates",
           "dp_trim_setup", "dp_trim_edges", "dp_trim_release", "dp_trim_error", "dp_trim_scan_chunks",
           "dp_trim_chunk_segments", "dp_trim_search", "dp_trim_edges_resident", "dp_trim_scan_chunks_resident", "dp_reads_respan", "dp_reads_respan_rc", "dp_reads_replace_tail_packed_rc", "dp_ctx_refresh_shared",
           "dp_reads_replace_tail_packed", "dp_reads_respan_tail_rc",
           "dp_debug_chain_paths", "dp_align_spans"]

_lib = None


def load_library():
    """Loads the HIP library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise DpError("libdownpore_hip.so is not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C downpore_amd/csrc`. There is no CPU fallback." % p)
    L = C.CDLL(p)
    vp = C.c_void_p
    L.dp_version.restype = C.c_char_p
    L.dp_last_error.restype = C.c_char_p
    L.dp_last_error.argtypes = [vp]
    L.dp_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.dp_ctx_create_shared.argtypes = [vp, C.POINTER(vp)]
    L.dp_ctx_destroy.argtypes = [vp]
    L.dp_reads_upload.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint32]
    L.dp_reads_packed.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.dp_reads_count.restype = C.c_uint32
    L.dp_reads_count.argtypes = [vp]
    L.dp_reads_total_bases.restype = C.c_uint64
    L.dp_reads_total_bases.argtypes = [vp]
    L.dp_kmer_histogram.argtypes = [vp, C.c_int, C.c_void_p]
    L.dp_kmer_values.argtypes = [vp, C.c_int, C.c_void_p]
    L.dp_round_begin.argtypes = [vp, C.c_int, C.c_void_p, C.c_uint32]
    L.dp_scan.argtypes = [vp, C.c_void_p, C.c_uint32, C.POINTER(SeedSeqBatch)]
    L.dp_scan_reads.argtypes = [vp, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32,
                                C.POINTER(SurvivorBatch)]
    L.dp_index_build.argtypes = [vp, C.c_void_p, C.c_uint32]
    L.dp_find_overlaps.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_int, C.c_uint32, C.c_int,
                                   C.POINTER(MatchBatch)]
    L.dp_map_windows.argtypes = [vp, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(ChainBatch)]
    L.dp_index_posting_row.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.dp_index_seedset_row.argtypes = [vp, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.dp_scan_device_buffers.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64)]
    L.dp_scan_import_segments.argtypes = [vp, C.c_void_p, C.c_uint64]
    _lib = L
    return L


def _arr(p, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(p, shape=(int(n),)).astype(dtype, copy=True)


class Context:
    """One GPU context (`dp_ctx`): reads resident in HBM + per-round seed/index state."""

    def __init__(self, device=0, shared_from=None):
        """shared_from: another Context whose resident reads this one borrows (dp_ctx_create_shared); close it before that one."""
        self.L = load_library()
        h = C.c_void_p()
        if shared_from is not None:
            rc = self.L.dp_ctx_create_shared(shared_from.h, C.byref(h))
            if rc != 0:
                raise DpError("dp_ctx_create_shared failed (%d): %s" % (rc, self.L.dp_last_error(shared_from.h).decode()))
        else:
            rc = self.L.dp_ctx_create(device, C.byref(h))
            if rc != 0:
                raise DpError("dp_ctx_create failed (%d): %s" % (rc, self.L.dp_last_error(None).decode()))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.dp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise DpError("libdownpore_hip error %d: %s" % (rc, self.L.dp_last_error(self.h).decode()))

    # ---- A1
    def upload_reads(self, bases, off):
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        self._chk(self.L.dp_reads_upload(self.h, bases.ctypes.data, off.ctypes.data, len(off) - 1))
        self.read_len = np.diff(off).astype(np.int64)

    def upload_reads_rc(self, bases, off, first_paired):
        """Reads >= first_paired are stored as (forward, reverse complement) pairs; the device makes the second strand."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        self.L.dp_reads_upload_rc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        self._chk(self.L.dp_reads_upload_rc(self.h, bases.ctypes.data, off.ctypes.data, len(off) - 1, first_paired))
        ln = np.diff(off).astype(np.int64)
        self.read_len = np.concatenate([ln[:first_paired], np.repeat(ln[first_paired:], 2)])

    def upload_reads_packed_rc(self, packed, lens, first_paired, pinned=False):
        """The reads arrive 2-bit packed (read r at the sum of the 16-byte-rounded packed sizes before it); pinned: through a block of
        dp_host_alloc, as the mapper does."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        self.L.dp_reads_upload_packed_rc.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        self.L.dp_host_alloc.restype = C.c_void_p
        self.L.dp_host_alloc.argtypes = [C.c_size_t]
        self.L.dp_host_free.argtypes = [C.c_void_p]
        blk = None
        ptr = packed.ctypes.data
        if pinned:
            blk = self.L.dp_host_alloc(max(1, packed.size))
            assert blk
            C.memmove(blk, packed.ctypes.data, packed.size)
            ptr = blk
        try:
            self._chk(self.L.dp_reads_upload_packed_rc(self.h, ptr, lens.ctypes.data, len(lens), first_paired))
        finally:
            if blk:
                self.L.dp_host_free(blk)
        ln = lens.astype(np.int64)
        self.read_len = np.concatenate([ln[:first_paired], np.repeat(ln[first_paired:], 2)])

    def _replace_tail(self, call, keep, packed, lens, pinned):
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        call.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
        self.L.dp_host_alloc.restype = C.c_void_p
        self.L.dp_host_alloc.argtypes = [C.c_size_t]
        self.L.dp_host_free.argtypes = [C.c_void_p]
        blk = None
        ptr = packed.ctypes.data
        if pinned:
            blk = self.L.dp_host_alloc(max(1, packed.size))
            assert blk
            C.memmove(blk, packed.ctypes.data, packed.size)
            ptr = blk
        try:
            self._chk(call(self.h, keep, ptr, lens.ctypes.data, len(lens)))
        finally:
            if blk:
                self.L.dp_host_free(blk)
        return lens.astype(np.int64)

    def replace_tail_packed_rc(self, keep, packed, lens, pinned=True):
        """dp_reads_replace_tail_packed_rc: the device reads [0, keep) stay, everything behind them becomes the batch (packed, lens)
        as (forward, reverse complement) pairs.  Borrowing contexts need refresh_shared() afterwards."""
        ln = self._replace_tail(self.L.dp_reads_replace_tail_packed_rc, keep, packed, lens, pinned)
        self.read_len = np.concatenate([np.asarray(self.read_len[:keep], dtype=np.int64), np.repeat(ln, 2)])

    def replace_tail_packed(self, keep, packed, lens, pinned=True):
        """dp_reads_replace_tail_packed: replace_tail_packed_rc without the reverse strands - device read keep + r is batch read r."""
        ln = self._replace_tail(self.L.dp_reads_replace_tail_packed, keep, packed, lens, pinned)
        self.read_len = np.concatenate([np.asarray(self.read_len[:keep], dtype=np.int64), ln])

    def respan_tail_rc(self, keep, spans):
        """dp_reads_respan_tail_rc: the reads behind `keep` replaced by the (forward, reverse complement) pairs of spans of themselves -
        uint32 [n, 3] = (device read >= keep, start, len), any order, a read any number of times.  The head stays byte for byte;
        borrowing contexts need refresh_shared() afterwards."""
        sp = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 3)
        self.L.dp_reads_respan_tail_rc.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        self._chk(self.L.dp_reads_respan_tail_rc(self.h, keep, sp.ctypes.data if len(sp) else None, len(sp)))
        self.read_len = np.concatenate([np.asarray(self.read_len[:keep], dtype=np.int64), np.repeat(sp[:, 2].astype(np.int64), 2)])

    def refresh_shared(self, owner):
        """dp_ctx_refresh_shared: a borrowing context takes its owner's read set again after a tail replace."""
        self.L.dp_ctx_refresh_shared.argtypes = [C.c_void_p]
        self._chk(self.L.dp_ctx_refresh_shared(self.h))
        self.read_len = np.array(owner.read_len, dtype=np.int64)

    def packed_read(self, r):
        nb = (int(self.read_len[r]) + 3) // 4
        out = np.zeros(max(nb, 1), dtype=np.uint8)
        n = C.c_uint64(0)
        self._chk(self.L.dp_reads_packed(self.h, r, out.ctypes.data, nb, C.byref(n)))
        return out[:nb]

    def respan(self, spans):
        """dp_reads_respan: the resident read set replaced by spans of itself - uint32 [n, 3] = (read, start, len) per new read, any order,
        a read any number of times.  Only between the upload and the first round / index / value table (DpError otherwise)."""
        sp = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 3)
        self.L.dp_reads_respan.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._chk(self.L.dp_reads_respan(self.h, sp.ctypes.data if len(sp) else None, len(sp)))
        self.read_len = sp[:, 2].astype(np.int64)

    def respan_rc(self, spans, first_paired):
        """dp_reads_respan_rc: respan with the layout of upload_reads_rc - spans >= first_paired are stored as (forward, reverse
        complement) pairs, the second strand made on the device.  A value table on the context is no reason to refuse (DpError for a
        round, a k-mer position index, borrowed or lent reads, a pending upload, a span outside its read, first_paired > n)."""
        sp = np.ascontiguousarray(spans, dtype=np.uint32).reshape(-1, 3)
        self.L.dp_reads_respan_rc.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        self._chk(self.L.dp_reads_respan_rc(self.h, sp.ctypes.data if len(sp) else None, len(sp), first_paired))
        ln = sp[:, 2].astype(np.int64)
        self.read_len = np.concatenate([ln[:first_paired], np.repeat(ln[first_paired:], 2)])

    # ---- A22
    def kmer_histogram(self, k):
        out = np.zeros(4 ** k, dtype=np.uint64)
        self._chk(self.L.dp_kmer_histogram(self.h, k, out.ctypes.data))
        return out

    # ---- A22 + A23: value table computed (and left resident) on the device
    def kmer_values(self, k):
        out = np.zeros(4 ** k, dtype=np.float64)
        self._chk(self.L.dp_kmer_values(self.h, k, out.ctypes.data))
        self.n_values = len(out)
        return out

    def values_codes(self, width):
        """The resident table of kmer_values as one code per k-mer (dp_values_download_codes8 for width 1, dp_values_download_codes for
        width 2): its own count where it has a value, 0 where it has none, clamped to 255 / 65535.  -> (codes, total, overflow): total =
        the sum of all counts, overflow = 1 when a valued k-mer counts more than 254 / 65535.  DpError for a table that was uploaded."""
        if width not in (1, 2):
            raise ValueError("values_codes: width is 1 or 2")
        n = getattr(self, "n_values", 0)
        if not n:
            raise DpError("values_codes: no value table resident")
        call = self.L.dp_values_download_codes8 if width == 1 else self.L.dp_values_download_codes
        call.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_int)]
        codes = np.zeros(n, dtype=np.uint8 if width == 1 else np.uint16)
        total, overflow = C.c_uint64(0), C.c_int(0)
        self._chk(call(self.h, codes.ctypes.data, n, C.byref(total), C.byref(overflow)))
        return codes, int(total.value), int(overflow.value)

    # ---- A18: the parallel part of AddSingleSeeds
    def single_seed_candidates(self, read, k, seed_rate):
        """dp_single_seed_candidates for one resident read (its value table resident): dict best, cand_off, cand"""
        b = SingleSeedBatch()
        self.L.dp_single_seed_candidates.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int64, C.POINTER(SingleSeedBatch)]
        self._chk(self.L.dp_single_seed_candidates(self.h, read, k, seed_rate, C.byref(b)))
        n = b.n_windows
        off = _arr(b.cand_off, n + 1, np.uint32) if n else np.zeros(1, dtype=np.uint32)
        return dict(best=_arr(b.best, n, np.uint32), cand_off=off, cand=_arr(b.cand, off[-1], np.uint32))

    def single_seed_candidates_multi(self, first_read, n_reads, k, seed_rate):
        """dp_single_seed_candidates_multi for a run of resident reads on one seed index: dict best, cand_off, cand, win_off"""
        b = SingleSeedMultiBatch()
        self.L.dp_single_seed_candidates_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int64,
                                                           C.POINTER(SingleSeedMultiBatch)]
        self._chk(self.L.dp_single_seed_candidates_multi(self.h, first_read, n_reads, k, seed_rate, C.byref(b)))
        n = b.n_windows
        off = _arr(b.cand_off, n + 1, np.uint32) if n else np.zeros(1, dtype=np.uint32)
        return dict(best=_arr(b.best, n, np.uint32), cand_off=off, cand=_arr(b.cand, off[-1], np.uint32),
                    win_off=_arr(b.win_off, n_reads + 1, np.uint32))

    # ---- round
    def round_begin(self, k, seed_kmers):
        s = np.ascontiguousarray(seed_kmers, dtype=np.uint32)
        self.k = k
        self.n_seeds = len(s)
        self._chk(self.L.dp_round_begin(self.h, k, s.ctypes.data, len(s)))

    # ---- A2 + A10
    def scan(self, items):
        """items: array-like of (read, start, n_kmers, min_seeds).  Returns dict with n_seeds, seg_off, segs."""
        it = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 4)
        b = SeedSeqBatch()
        self._chk(self.L.dp_scan(self.h, it.ctypes.data, len(it), C.byref(b)))
        n = b.n_items
        return dict(n_seeds=_arr(b.n_seeds, n, np.uint32), seg_off=_arr(b.seg_off, n + 1, np.uint64),
                    segs=_arr(b.segs, b.n_segs, np.int32), kernel_ms=b.kernel_ms, count_kernel_ms=b.count_kernel_ms,
                    write_kernel_ms=b.write_kernel_ms, bases_scanned=b.bases_scanned)

    def scan_prepare(self, k):
        """One-off work of dp_scan_reads (the resident k-mer position index, when this read set gets one) done now."""
        self.L.dp_scan_prepare.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.L.dp_scan_prepare(self.h, k))

    def set_priority(self, high=True):
        self.L.dp_ctx_set_priority.argtypes = [C.c_void_p, C.c_int]
        self._chk(self.L.dp_ctx_set_priority(self.h, 1 if high else 0))

    def scan_reads(self, ignore, epoch, lo, hi, top_level, min_seeds, extra=None):
        ig = np.ascontiguousarray(ignore, dtype=np.uint8)
        ex = np.ascontiguousarray(extra if extra is not None else np.zeros((0, 4)), dtype=np.uint32).reshape(-1, 4)
        b = SurvivorBatch()
        self._chk(self.L.dp_scan_reads(self.h, ig.ctypes.data, epoch, lo, hi, 1 if top_level else 0, min_seeds, ex.ctypes.data,
                                       len(ex), C.byref(b)))
        ns, ne = b.n_survivors, b.n_extra
        return dict(read=_arr(b.read, ns, np.uint32), n_seeds=_arr(b.n_seeds, ns, np.uint32), seg_off=_arr(b.seg_off, ns, np.uint64),
                    extra_n_seeds=_arr(b.extra_n_seeds, ne, np.uint32), extra_seg_off=_arr(b.extra_seg_off, ne, np.uint64),
                    segs=_arr(b.segs, b.n_segs, np.int32), bases_scanned=b.bases_scanned, reads_scanned=b.reads_scanned,
                    kernel_ms=b.kernel_ms, index_mode=int(b.index_mode), index_hits=int(b.index_hits))

    # ---- A9 selection
    def values_upload(self, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self.L.dp_values_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        self._chk(self.L.dp_values_upload(self.h, v.ctypes.data, len(v)))
        self.n_values = len(v)

    def select_seeds(self, windows, k, num_seeds):
        """windows: (read, start, length in bases) rows -> uint32 [n, num_seeds] k-mers in insertion-list order."""
        w = np.zeros((len(windows), 4), dtype=np.uint32)
        if len(windows):
            w[:, :3] = np.asarray(windows, dtype=np.uint32).reshape(-1, 3)
        out = np.zeros((len(windows), num_seeds), dtype=np.uint32)
        self.L.dp_select_seeds.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
        self._chk(self.L.dp_select_seeds(self.h, w.ctypes.data, len(w), k, num_seeds, out.ctypes.data))
        return out

    def import_segments(self, segs):
        s = np.ascontiguousarray(segs, dtype=np.int32)
        self._chk(self.L.dp_scan_import_segments(self.h, s.ctypes.data, len(s)))

    def scan_device_buffer(self):
        p = C.c_void_p()
        n = C.c_uint64(0)
        self._chk(self.L.dp_scan_device_buffers(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    # ---- A13
    def index_build(self, seg_off, n_seeds):
        refs = np.zeros(len(seg_off), dtype=[("seg_off", np.uint64), ("n_seeds", np.uint32), ("reserved", np.uint32)])
        refs["seg_off"] = seg_off
        refs["n_seeds"] = n_seeds
        self._chk(self.L.dp_index_build(self.h, refs.ctypes.data, len(refs)))
        self.n_seqs = len(refs)

    def index_build_sparse(self, seg_off, n_seeds):
        """The same index as id lists (dp_index_build_sparse); the row and meta calls answer alike."""
        refs = np.zeros(len(seg_off), dtype=[("seg_off", np.uint64), ("n_seeds", np.uint32), ("reserved", np.uint32)])
        refs["seg_off"] = seg_off
        refs["n_seeds"] = n_seeds
        self.L.dp_index_build_sparse.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._chk(self.L.dp_index_build_sparse(self.h, refs.ctypes.data, len(refs)))
        self.n_seqs = len(refs)

    def index_borrow(self, src):
        """dp_index_borrow: after round_begin with src's seeds, read src's sparse index instead of building one."""
        self.L.dp_index_borrow.argtypes = [C.c_void_p, C.c_void_p]
        self._chk(self.L.dp_index_borrow(self.h, src.h))
        self.n_seqs = src.n_seqs

    def index_info(self):
        """dp_index_info: layout ("none" / "dense" / "sparse"), borrowed, n_seeds, n_seqs, device_bytes, entries, queries[4]."""
        info = IndexInfo()
        self.L.dp_index_info.argtypes = [C.c_void_p, C.POINTER(IndexInfo)]
        self._chk(self.L.dp_index_info(self.h, C.byref(info)))
        return dict(layout={0: "none", 1: "dense", 2: "sparse"}[info.layout], borrowed=bool(info.borrowed), n_seeds=info.n_seeds,
                    n_seqs=info.n_seqs, device_bytes=info.device_bytes, entries=info.entries, queries=list(info.queries))

    def index_meta(self):
        """dp_index_meta: the {count, first word, last word, last + 1} rows of every seed, uint32 [S, 4]."""
        out = np.zeros((self.n_seeds, 4), dtype=np.uint32)
        self.L.dp_index_meta.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._chk(self.L.dp_index_meta(self.h, out.ctypes.data, self.n_seeds))
        return out

    def index_set_global(self, meta_global, word_base, n_seqs_global):
        m = np.ascontiguousarray(meta_global, dtype=np.uint32)
        self.L.dp_index_set_global.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
        self._chk(self.L.dp_index_set_global(self.h, m.ctypes.data, self.n_seeds, word_base, n_seqs_global))

    def posting_row(self, seed):
        W = max(1, (self.n_seqs + 63) // 64)
        words = np.zeros(W, dtype=np.uint64)
        nw, cnt, st, en = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.L.dp_index_posting_row(self.h, seed, words.ctypes.data, W, C.byref(nw), C.byref(cnt), C.byref(st),
                                              C.byref(en)))
        return words, cnt.value, st.value, en.value

    def seedset_row(self, seq):
        SW = max(1, (self.n_seeds + 63) // 64)
        words = np.zeros(SW, dtype=np.uint64)
        nw = C.c_uint32()
        self._chk(self.L.dp_index_seedset_row(self.h, seq, words.ctypes.data, SW, C.byref(nw)))
        return words

    # ---- A14 .. A8
    def find_overlaps(self, q_segs, q_off, hit_fraction, k, max_query_len, want_candidates=False, on_device=False, pending=False):
        """on_device (bit 1 of want_candidates): the matches stay on the device for consensus_paf, only times and byte counts come
        back; pending (bit 2, with on_device): the stage is not even waited for - the next call must be consensus_paf."""
        qs = np.ascontiguousarray(q_segs, dtype=np.int32)
        qo = np.ascontiguousarray(q_off, dtype=np.uint64)
        b = MatchBatch()
        if pending and not on_device:
            raise ValueError("find_overlaps: pending needs on_device")
        bits = (1 if want_candidates else 0) | (2 if on_device else 0) | (4 if pending else 0)
        self._chk(self.L.dp_find_overlaps(self.h, qs.ctypes.data, qo.ctypes.data, len(qo) - 1, float(hit_fraction), k,
                                          max_query_len, bits, C.byref(b)))
        if on_device:
            return dict(query_kernel_ms=b.query_kernel_ms, chain_kernel_ms=b.chain_kernel_ms, query_bytes=b.query_bytes,
                        chain_bytes=b.chain_bytes)
        return self._match_lists(b, want_candidates)

    def fetch_overlaps(self):
        """dp_fetch_overlaps: the match lists of the last find_overlaps (what that call returns itself unless on_device)"""
        b = MatchBatch()
        self.L.dp_fetch_overlaps.argtypes = [C.c_void_p, C.POINTER(MatchBatch)]
        self._chk(self.L.dp_fetch_overlaps(self.h, C.byref(b)))
        return self._match_lists(b, False)

    @staticmethod
    def _match_lists(b, want_candidates):
        nm = b.n_matches
        off = _arr(b.off, nm + 1, np.uint64)
        tot = int(off[-1]) if nm else 0
        res = dict(query=_arr(b.query, nm, np.uint32), target=_arr(b.target, nm, np.uint32), off=off,
                   match_a=_arr(b.match_a, tot, np.int32), match_b=_arr(b.match_b, tot, np.int32),
                   target_anchor=_arr(b.target_anchor, 2 * nm, np.int32).reshape(-1, 2),
                   query_kernel_ms=b.query_kernel_ms, chain_kernel_ms=b.chain_kernel_ms, query_bytes=b.query_bytes,
                   chain_bytes=b.chain_bytes)
        if want_candidates:
            co = _arr(b.cand_off, b.n_queries + 1, np.uint64)
            res["cand_off"] = co
            res["cand"] = _arr(b.cand, int(co[-1]), np.uint32)
        return res

    def chain_paths(self):
        """dp_debug_chain_paths (test hook) for the last find_overlaps, which must have run under DP_DEBUG=chain_paths: dict of query,
        target, path (uint32 per pair, the header's bits), attempts, passes, error_bits, pair_cap."""
        self.L.dp_debug_chain_paths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]
        n = C.c_uint32(0)
        info = np.zeros(4, dtype=np.uint32)
        self._chk(self.L.dp_debug_chain_paths(self.h, None, 0, C.byref(n), info.ctypes.data))
        out = np.zeros((max(1, n.value), 3), dtype=np.uint32)
        self._chk(self.L.dp_debug_chain_paths(self.h, out.ctypes.data, n.value, C.byref(n), info.ctypes.data))
        out = out[:n.value]
        return dict(query=out[:, 0].copy(), target=out[:, 1].copy(), path=out[:, 2].copy(), attempts=int(info[0]), passes=int(info[1]),
                    error_bits=int(info[2]), pair_cap=int(info[3]))

    # ---- A15 - A17
    def consensus_paf(self, metas, rc_of, k, overlap_size):
        """dp_consensus_paf for the round whose find_overlaps(on_device=True) ran last.  metas: SEQ_META [n_seqs] (read, Len(),
        GetOffset(), GetInset() of every indexed sequence), rc_of: int32 [n_seeds].  Returns dict groups (GROUP_META [windows]), paf
        (PAF_REC, a window's lines at groups.slot ..), ignore_ids (uint32, likewise), n_indexed."""
        m = np.ascontiguousarray(metas, dtype=SEQ_META)
        rc = np.ascontiguousarray(rc_of, dtype=np.int32)
        b = PafBatch()
        self.L.dp_consensus_paf.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(PafBatch)]
        self._chk(self.L.dp_consensus_paf(self.h, m.ctypes.data, len(m), rc.ctypes.data, len(rc), k, overlap_size, C.byref(b)))
        ng = b.n_groups
        if ng == 0 or not b.groups:
            return dict(groups=np.zeros(0, dtype=GROUP_META), paf=np.zeros(0, dtype=PAF_REC), ignore_ids=np.zeros(0, dtype=np.uint32),
                        n_indexed=int(b.n_indexed))
        groups = np.frombuffer(C.string_at(b.groups, ng * GROUP_META.itemsize), dtype=GROUP_META).copy()
        # the slots of the arrays are the round's matched pairs; a window owns [slot, slot + its pairs): read up to the last one in use
        ok = groups["flag"] == 0
        n = int(max((groups["slot"][ok].astype(np.int64) + np.maximum(groups["n_lines"][ok], groups["n_ignore"][ok])).max(initial=0), 0))
        paf = np.frombuffer(C.string_at(b.paf, n * PAF_REC.itemsize), dtype=PAF_REC).copy() if n else np.zeros(0, dtype=PAF_REC)
        return dict(groups=groups, paf=paf, ignore_ids=_arr(b.ignore_ids, n, np.uint32), n_indexed=int(b.n_indexed))

    def consensus_align(self, segs, seq_off, group_off, k):
        """dp_consensus_align: group g = sequences group_off[g] .. group_off[g + 1], sequence s = segs[seq_off[s] .. seq_off[s + 1]) in its
        Reduced() form.  Returns dict flags [groups], cons (list of int32 arrays), match_a / match_b (lists, one pair of arrays per
        sequence; match_b indexes the reduced sequence)."""
        sg = np.ascontiguousarray(segs, dtype=np.int32)
        so = np.ascontiguousarray(seq_off, dtype=np.uint64)
        go = np.ascontiguousarray(group_off, dtype=np.uint32)
        b = ConsensusBatch()
        self.L.dp_consensus_align.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(ConsensusBatch)]
        self._chk(self.L.dp_consensus_align(self.h, sg.ctypes.data, so.ctypes.data, go.ctypes.data, len(go) - 1, k, C.byref(b)))
        ng, ns = len(go) - 1, int(go[-1])
        flags = _arr(b.flags, ng, np.uint32)
        coff, clen = _arr(b.cons_off, ng + 1, np.uint64), _arr(b.cons_len, ng, np.uint32)
        call = _arr(b.cons, int(coff[-1]), np.int32)
        mlen = _arr(b.match_len, ns, np.uint32)
        ma, mb = _arr(b.match_a, int(so[-1]), np.int32), _arr(b.match_b, int(so[-1]), np.int32)
        cons, la, lb = [], [], []
        for g in range(ng):
            cons.append(call[int(coff[g]):int(coff[g]) + int(clen[g])] if flags[g] == 0 else None)
            for s in range(int(go[g]), int(go[g + 1])):
                n = int(mlen[s]) if flags[g] == 0 else 0
                la.append(ma[int(so[s]):int(so[s]) + n])
                lb.append(mb[int(so[s]):int(so[s]) + n])
        return dict(flags=flags, cons=cons, match_a=la, match_b=lb)

    def query_candidates(self, q_segs, q_off, hit_fraction):
        """dp_query_candidates: Matches() alone on either layout -> cand_off, cand (ascending ids per query, shard-local), meta
        uint32 [n, 3] = {sets, minCount, status}."""
        qs = np.ascontiguousarray(q_segs, dtype=np.int32)
        qo = np.ascontiguousarray(q_off, dtype=np.uint64)
        b = CandidateBatch()
        self.L.dp_query_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.POINTER(CandidateBatch)]
        self._chk(self.L.dp_query_candidates(self.h, qs.ctypes.data, qo.ctypes.data, len(qo) - 1, float(hit_fraction), C.byref(b)))
        n = b.n_queries
        co = _arr(b.cand_off, n + 1, np.uint64)
        return dict(cand_off=co, cand=_arr(b.cand, int(co[-1]), np.uint32), meta=_arr(b.meta, 3 * n, np.uint32).reshape(-1, 3))

    # ---- A19 + A20
    def map_windows(self, w_segs, w_off, w_len, k):
        ws = np.ascontiguousarray(w_segs, dtype=np.int32)
        wo = np.ascontiguousarray(w_off, dtype=np.uint64)
        wl = np.ascontiguousarray(w_len, dtype=np.uint32)
        b = ChainBatch()
        self._chk(self.L.dp_map_windows(self.h, ws.ctypes.data, wo.ctypes.data, wl.ctypes.data, len(wo) - 1, k, C.byref(b)))
        return self._chains(b)

    @staticmethod
    def _chains(b):
        n = b.n_chains
        off = _arr(b.off, n + 1, np.uint64)
        tot = int(off[-1]) if n else 0
        return dict(window=_arr(b.window, n, np.uint32), target=_arr(b.target, n, np.uint32), off=off,
                    match_a=_arr(b.match_a, tot, np.int32), match_b=_arr(b.match_b, tot, np.int32), kernel_ms=b.kernel_ms)

    def map_windows_shard(self, w_segs, w_off, w_len, k, phase, thr):
        """dp_map_windows_shard: one strand (phase 0 forward, 1 reverse complement) of every window pair against this context's
        shard.  thr: int32 [n_windows] minMatches / minRCMatches per pair (-1: the window's own).  Returns (chains, updated thr)."""
        ws = np.ascontiguousarray(w_segs, dtype=np.int32)
        wo = np.ascontiguousarray(w_off, dtype=np.uint64)
        wl = np.ascontiguousarray(w_len, dtype=np.uint32)
        t = np.array(thr, dtype=np.int32)
        assert t.shape == (len(wo) - 1,)
        b = ChainBatch()
        self.L.dp_map_windows_shard.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                C.POINTER(ChainBatch)]
        self._chk(self.L.dp_map_windows_shard(self.h, ws.ctypes.data, wo.ctypes.data, wl.ctypes.data, len(wo) - 1, k, phase, t.ctypes.data,
                                              C.byref(b)))
        return self._chains(b), t

    # ---- base-level alignment of spans of the resident reads
    def align_spans(self, items, max_edits=4096, circular=False):
        """dp_align_spans: items = rows (q_read, q_off, q_len, t_read, t_off, t_len) over the resident reads.  Returns dict nm (int32
        [n], -1 = over max_edits), cigar (list of strings, "" where nm is -1), runs (list of uint32 arrays len << 2 | op), cells,
        tb_bytes, doublings, kernel_ms."""
        it = np.ascontiguousarray(np.asarray(items, dtype=np.uint32).reshape(-1, 6))
        b = AlignBatch()
        self.L.dp_align_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(AlignBatch)]
        self._chk(self.L.dp_align_spans(self.h, it.ctypes.data if len(it) else None, len(it), int(max_edits), 1 if circular else 0, C.byref(b)))
        n = b.n
        recs = np.frombuffer(C.string_at(b.recs, n * ALIGN_REC.itemsize), dtype=ALIGN_REC) if n else np.zeros(0, dtype=ALIGN_REC)
        runs = _arr(b.runs, b.n_runs, np.uint32)
        per = [runs[int(r["run_off"]):int(r["run_off"]) + int(r["n_runs"])] for r in recs]
        return dict(nm=recs["nm"].astype(np.int32), runs=per, cigar=["".join("%d%s" % (int(x) >> 2, "MID?"[int(x) & 3]) for x in pr) for pr in per],
                    cells=int(b.cells), tb_bytes=int(b.tb_bytes), doublings=int(b.doublings), kernel_ms=float(b.kernel_ms))
