"""A Mapper - the reference opened once, read sets mapped against it batch after batch - must print for every batch what the oracle's
whole `map` run prints for that batch alone, PAF and stderr, line for line: on both index layouts, circular and linear references, with
-all_sequences (against the model of tests/native/map_multi_model.cpp), for batches that grow, shrink, repeat, are empty, hold only
short reads or only reads below min_length; through the Python class and through the C ABI alone."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests.test_gpu_map import first_diff

pytestmark = pytest.mark.gpu

# the generator parameters of tests/test_gpu_map.py::test_map_paf_bit_exact, with batches of at most 120 reads
CASES = {True: (3, 200000, 8000, 0.0, False), False: (5, 300000, 9000, 0.10, True)}
ORDER = ["A", "B", "A", "empty", "C", "D", "short", "tiny"]


def _take(bases, off, i0, i1):
    return np.array(bases[off[i0]:off[i1]], dtype=np.uint8), (off[i0:i1 + 1] - off[i0]).astype(np.int64)


def _batches(seed, G, L, e, variable):
    """A, B: 100 reads each; C: 100 reads of twice the length (twice A's bases); D: a tenth of A; short: reads <= 2 * query_size, some with
    len % 4 == 0 (the top-level scan quirks on both strands); tiny: every read below min_length; empty: no read at all"""
    bases, off = O.gen_reads(seed, G, 210, L, e, variable)
    b2, o2 = O.gen_reads(seed, G, 100, 2 * L, e, variable)
    xb, xo = O.gen_reads(seed, G, 40, 1400, e, True)
    cut = [1200, 1600, 1996, 2000, 900, 1333]
    parts = [xb[xo[i]:xo[i] + min(int(xo[i + 1] - xo[i]), cut[i % len(cut)])] for i in range(40)]
    short = (np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64))
    assert any(len(p) % 4 == 0 and len(p) <= 2000 for p in parts)
    tiny = (np.concatenate([p[:300] for p in parts]), (300 * np.arange(41)).astype(np.int64))
    return {"A": _take(bases, off, 0, 100), "B": _take(bases, off, 100, 200), "C": (b2, o2), "D": _take(bases, off, 200, 210),
            "short": short, "tiny": tiny, "empty": (np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64))}


_cache = {}


def _oracle_case(circular):
    """the reference, the batches and the oracle's answer for each batch alone - computed once per reference"""
    if circular not in _cache:
        seed, G, L, e, variable = CASES[circular]
        genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
        goff = np.array([0, G], dtype=np.int64)
        batches = _batches(seed, G, L, e, variable)
        oref = O.ReadSet(genome, goff, min_len=0, himem=False)
        want = {}
        for name, (b, o) in batches.items():
            want[name] = O.map_run(oref, O.ReadSet(b, o, min_len=500, himem=False), circular=circular)
            n = len(o) - 1
            if name in ("A", "B", "C", "D", "short"):  # (on the oracle's text: an all-unmapped run cannot pass)
                assert want[name][0].count("\n") > n // 2, name
        assert want["empty"][0] == "" and want["tiny"][0] == ""
        _cache[circular] = dict(ref=(genome, goff), batches=batches, want=want)
    return _cache[circular]


def _same(got, want, what):
    d = first_diff(got[0], want[0])
    assert d is None, (what, d)
    assert got[1] == want[1], what


@pytest.mark.parametrize("index", ["dense", "sparse"])
@pytest.mark.parametrize("circular", [True, False])
def test_every_batch_is_the_oracles_run_on_that_batch(circular, index):
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    c = _oracle_case(circular)
    ref = Reads(*c["ref"], min_len=0, himem=False)
    stats = []
    with Mapper(ref, circular=circular, index=index) as m:
        for name in ORDER:
            reads = Reads(*c["batches"][name], min_len=500, himem=False)
            paf, err, st = m.map(reads)
            _same((paf, err), c["want"][name], (name, index))
            stats.append(st)
    assert all(st["index"]["layout"] == index for st in stats)
    assert len(set(st["index"]["index_builds"] for st in stats)) == 1 and stats[0]["index"]["index_builds"] >= 1
    assert len(set(st["index"]["index_bytes"] for st in stats)) == 1
    assert len(set(st["n_seeds"] for st in stats)) == 1 and stats[0]["n_seeds"] > 0
    assert len(set(st["n_chunks"] for st in stats)) == 1 and stats[0]["n_chunks"] > 0
    by = dict(zip(ORDER, stats))
    assert by["A"]["n_windows"] >= 100 and by["empty"]["n_windows"] == 0 and by["D"]["n_windows"] >= 10
    assert stats[2]["n_windows"] == stats[0]["n_windows"] and stats[2]["n_chains"] == stats[0]["n_chains"]  # A again
    assert stats[2]["index"]["q_ladder8"] + stats[2]["index"]["q_ladder16"] + stats[2]["index"]["q_exact"] == \
        stats[0]["index"]["q_ladder8"] + stats[0]["index"]["q_ladder16"] + stats[0]["index"]["q_exact"]


def test_several_threads_keep_their_contexts(monkeypatch):
    """with a thread plan of more than one thread the worker contexts are opened by the first batch that needs them, kept, and
    refreshed by every later batch: index_builds grows with the first such batch and never again"""
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    monkeypatch.setenv("DP_MAP_THREADS", "3")
    monkeypatch.setenv("DP_TUNE", "map_min_reads_per_thread=30")
    c = _oracle_case(True)
    ref = Reads(*c["ref"], min_len=0, himem=False)
    builds = []
    with Mapper(ref, circular=True, index="dense") as m:
        for name in ["D", "A", "B", "empty", "A"]:
            paf, err, st = m.map(Reads(*c["batches"][name], min_len=500, himem=False))
            _same((paf, err), c["want"][name], name)
            builds.append(st["index"]["index_builds"])
    assert builds == [1, 3, 3, 3, 3]


def test_all_sequences_against_the_model():
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    from tests import map_multi_cases as MC
    from tests import map_multi_model as MM
    ref_bases, ref_off, bases, off, _ = MC.multi_case()
    n = len(off) - 1
    cuts = [(0, 110), (110, 220), (n - 60, n), (0, 110)]  # (the third holds the 40 short reads)
    ref = Reads(ref_bases, ref_off, min_len=0, himem=False)
    with Mapper(ref, circular=True, all_sequences=True) as m:
        for i0, i1 in cuts:
            b, o = _take(bases, off, i0, i1)
            want = MM.run(ref_bases, ref_off, b, o, circular=True)
            assert want[0].count("\n") > (i1 - i0) // 2
            got = m.map(Reads(b, o, min_len=500, himem=False))
            _same(got[:2], want, (i0, i1))
            assert "is shorter than query_size" in got[1]


def test_reference_too_short_for_any_chunk():
    from downpore_amd.mapping import Mapper, map_reads
    from downpore_amd.overlap import Reads
    c = _oracle_case(True)
    genome = np.array(c["ref"][0][:3000])
    goff = np.array([0, 3000], dtype=np.int64)
    ref = Reads(genome, goff, min_len=0, himem=False)
    with Mapper(ref, circular=False) as m:  # (a circular reference of query_size bases or more always has its join chunk)
        for name in ("D", "empty", "D"):
            reads = Reads(*c["batches"][name], min_len=500, himem=False)
            paf, err, st = m.map(reads)
            wpaf, werr, _ = map_reads(ref, reads, circular=False)
            n = len(c["batches"][name][1]) - 1
            assert paf == wpaf == "" and err == werr and ("Unmapped: %d\n" % n) in err
            assert st["n_chunks"] == 0 and st["n_windows"] == 0


def test_use_after_close_and_refusals(monkeypatch):
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    c = _oracle_case(True)
    ref = Reads(*c["ref"], min_len=0, himem=False)
    reads = Reads(*c["batches"]["D"], min_len=500, himem=False)
    m = Mapper(ref)
    _same(m.map(reads)[:2], c["want"]["D"], "D")
    m.close()
    m.close()
    with pytest.raises(DpError, match="closed"):
        m.map(reads)
    with pytest.raises(DpError, match="index must be"):
        Mapper(ref, index="roomy")
    monkeypatch.setenv("DP_MAP_SHARDS", "2")
    with pytest.raises(DpError, match="DP_MAP_SHARDS"):
        Mapper(ref)
    monkeypatch.delenv("DP_MAP_SHARDS")
    for key in ("map_ascii_upload", "map_async_upload"):
        monkeypatch.setenv("DP_TUNE", key + "=1")
        with pytest.raises(DpError, match=key):
            Mapper(ref)
    monkeypatch.delenv("DP_TUNE")
    with Mapper(ref) as m2:  # (a refused open leaves nothing behind that disturbs the next one)
        _same(m2.map(reads)[:2], c["want"]["D"], "D")


def test_two_mappers_on_different_references():
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    c1, c2 = _oracle_case(True), _oracle_case(False)
    r1, r2 = Reads(*c1["ref"], min_len=0, himem=False), Reads(*c2["ref"], min_len=0, himem=False)
    with Mapper(r1, circular=True) as m1, Mapper(r2, circular=False) as m2:
        for name in ("A", "D", "B"):
            _same(m2.map(Reads(*c2["batches"][name], min_len=500, himem=False))[:2], c2["want"][name], ("linear", name))
            _same(m1.map(Reads(*c1["batches"][name], min_len=500, himem=False))[:2], c1["want"][name], ("circular", name))


def test_c_abi_by_ctypes_alone():
    """the header's names and nothing else: dph_reads_from_arrays, dph_mapper_open / _map / _close, and the map handle's readers"""
    from downpore_amd.overlap import host_lib_path
    H = C.CDLL(host_lib_path())
    vp, i64 = C.c_void_p, C.c_int64
    H.dph_reads_from_arrays.restype = vp
    H.dph_reads_from_arrays.argtypes = [vp, vp, i64, i64, C.c_int]
    H.dph_reads_free.argtypes = [vp]
    H.dph_last_error.restype = C.c_char_p
    H.dph_last_error.argtypes = [vp]
    H.dph_mapper_open.restype = vp
    H.dph_mapper_open.argtypes = [vp, vp, C.c_int, C.c_int]
    H.dph_mapper_map.restype = vp
    H.dph_mapper_map.argtypes = [vp, vp]
    H.dph_mapper_close.argtypes = [vp]
    H.dph_map_free.argtypes = [vp]
    for f in (H.dph_map_paf, H.dph_map_errtext):
        f.restype = C.POINTER(C.c_char)
        f.argtypes = [vp, C.POINTER(i64)]
    H.dph_map_stats.argtypes = [vp, vp]
    H.dph_map_index_info.restype = C.c_int
    H.dph_map_index_info.argtypes = [vp, vp, C.c_int]

    def reads_handle(b, o, min_len):
        b, o = np.ascontiguousarray(b, dtype=np.uint8), np.ascontiguousarray(o, dtype=np.int64)
        h = H.dph_reads_from_arrays(b.ctypes.data, o.ctypes.data, len(o) - 1, min_len, 0)
        assert h
        return h

    c = _oracle_case(True)
    ref = reads_handle(*c["ref"], 0)
    p = np.array([1, 11, 1000, 500, 10000, 40, 1], dtype=np.int64)  # circular, k, query_size, min_length, chunk_size, seed_rate, dense
    assert not H.dph_mapper_open(ref, p.ctypes.data, 5, 0) and b"dph_mapper_open" in H.dph_last_error(None)
    bad = p.copy()
    bad[6] = 7
    assert not H.dph_mapper_open(ref, bad.ctypes.data, 7, 0) and b"index layout 7" in H.dph_last_error(None)
    m = H.dph_mapper_open(ref, p.ctypes.data, len(p), 0)
    assert m, H.dph_last_error(None)
    assert not H.dph_mapper_map(m, None) and b"dph_mapper_map" in H.dph_last_error(None)  # (refused for its arguments: still usable)
    seeds = set()
    for name in ORDER:
        rh = reads_handle(*c["batches"][name], 500)
        h = H.dph_mapper_map(m, rh)
        assert h, H.dph_last_error(None)
        H.dph_reads_free(rh)  # (the handle holds nothing of the batch)
        n = i64(0)
        paf = C.string_at(H.dph_map_paf(h, C.byref(n)), n.value).decode()
        err = C.string_at(H.dph_map_errtext(h, C.byref(n)), n.value).decode()
        st = np.zeros(13, dtype=np.float64)
        H.dph_map_stats(h, st.ctypes.data)
        ix = np.zeros(10, dtype=np.int64)
        assert H.dph_map_index_info(h, ix.ctypes.data, 10) == 10
        H.dph_map_free(h)
        _same((paf, err), c["want"][name], name)
        assert ix[0] == 1 and ix[5] == 1 and st[0] > 0  # dense, one build, the mapper's chunks
        seeds.add(st[1])
    assert len(seeds) == 1
    H.dph_mapper_close(m)
    H.dph_mapper_close(None)
    H.dph_reads_free(ref)
