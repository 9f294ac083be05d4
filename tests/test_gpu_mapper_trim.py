"""A Mapper that trims each raw batch on the device before it maps it: m.map(raw, trim=...) must print, batch after batch on one open
mapper, what the one-shot call map_reads(ref, raw, trim=...) prints for that batch alone - PAF and stderr text, text for text - with
plain batches in between, on both index layouts, linear, with -all_sequences, with several mapper threads; the first batch is also held
to the oracle's map_run over the MODEL's trimmed output.  A trim that fails for its parameters or its input leaves the mapper usable.
Inputs are those of tests/test_map_trim_gpu.py.  Integers and text: equal means equal."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import trim_cases as TC
from tests import trim_mid_model as MM
from tests.test_map_trim_cpu import MAP, MIN_LENGTH, reference
from tests.test_map_trim_gpu import _ads, _product_ref
from tests.test_overlap_trim_cpu import GEN, dump, generate, reads_of, written
from tests.test_overlap_trim_gpu import WRITING

pytestmark = pytest.mark.gpu

MIDDLE = dict(k=6, middle=True)
EDGES = dict(k=6, middle=False)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("mapper_trim_gpu")
    out = {"dir": d}
    for fastq in (False, True):
        names, seqs, quals, kinds = generate(fastq=fastq, **GEN)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = path
        if not fastq:  # the first 20 reads: too few for a second mapper thread
            out["few"] = str(d / "few.fasta")
            TC.write_fasta(out["few"], names[:20], seqs[:20], None)
    return out


def _raw(sets, fmt="fasta"):
    return reads_of(sets[fmt], himem=False)


_oneshot_cache = {}


def _oneshot(sets, fmt, trim, ref=None, tag="", **kw):
    """map_reads(ref, raw, trim=...) for the batch alone: (paf, stderr, stats, raw) - computed once per setting"""
    from downpore_amd.mapping import map_reads
    key = (fmt, tuple(sorted(trim.items())), tag, tuple(sorted(kw.items())))
    if key not in _oneshot_cache:
        raw = _raw(sets, fmt)
        paf, err, st = map_reads(ref if ref is not None else _product_ref(), raw, trim=dict(**trim, **_ads()), **MAP, **kw)
        _oneshot_cache[key] = (paf, err, st, raw)
    return _oneshot_cache[key]


def _same_trim(t, w, raw):
    """stats["trim"] of a mapper's batch against the one-shot call's"""
    assert np.array_equal(t.table, w.table) and t.adapters == w.adapters
    assert np.array_equal(t.splits, w.splits) and t.extras == w.extras and t.stderr == w.stderr
    assert dump(t.reads(MIN_LENGTH, himem=False)) == dump(w.reads(MIN_LENGTH, himem=False))
    assert t.output == "" and WRITING not in t.stderr
    assert 0 < t.stats["bytes_up"] * 10 < raw.total_bases()  # one crossing: ids and spans went up, never bases


def _trimmed_batch(m, sets, fmt, trim, want):
    raw = _raw(sets, fmt)
    paf, err, st = m.map(raw, trim=dict(**trim, **_ads()))
    assert paf == want[0] and err == want[1], (fmt, trim)
    _same_trim(st["trim"], want[2]["trim"], raw)
    return st


def test_trimmed_and_plain_batches_on_one_mapper(sets):
    from downpore_amd.mapping import Mapper
    g, off = reference()
    oref = O.ReadSet(g, off, min_len=0, himem=False)
    # the independent pin: the oracle's map over the model's written output
    model = MM.run(sets["fasta"], k=6)
    assert WRITING in model.stderr
    pin, _ = O.map_run(oref, O.ReadSet(fasta=written(sets["dir"], model, False, "model"), min_len=MIN_LENGTH, himem=False), **MAP)
    assert pin.count("\n") > 100 and "_(left)" in pin and "_(right)" in pin
    plain_want = O.map_run(oref, O.ReadSet(fasta=sets["fasta"], min_len=MIN_LENGTH, himem=False), **MAP)
    w_mid, w_edge = _oneshot(sets, "fasta", MIDDLE), _oneshot(sets, "fastq", EDGES)
    assert w_mid[0] == pin
    assert w_mid[0].count("\n") > 100 and w_edge[0].count("\n") > 100
    assert "_(left)" not in w_edge[0]
    assert plain_want[0].count("\n") > 100 and plain_want[0] != w_mid[0] and plain_want[0] != w_edge[0]  # a run that skipped the trim cannot pass
    stats = []
    with Mapper(_product_ref(), **MAP) as m:
        stats.append(_trimmed_batch(m, sets, "fasta", MIDDLE, w_mid))
        assert np.array_equal(stats[0]["trim"].table, model.table) and stats[0]["trim"].stderr == model.stderr.replace(WRITING, "")
        stats.append(_trimmed_batch(m, sets, "fastq", EDGES, w_edge))
        stats.append(_trimmed_batch(m, sets, "fasta", MIDDLE, w_mid))
        paf, err, st = m.map(reads_of(sets["fasta"], MIN_LENGTH, himem=False))
        assert (paf, err) == plain_want and "trim" not in st
        stats.append(st)
        stats.append(_trimmed_batch(m, sets, "fasta", MIDDLE, w_mid))
    for key in ("n_seeds", "n_chunks"):
        assert len(set(st[key] for st in stats)) == 1 and stats[0][key] > 0, key
    for key in ("index_bytes", "index_builds"):
        assert len(set(st["index"][key] for st in stats)) == 1 and stats[0]["index"][key] > 0, key
    assert stats[0]["n_seeds"] == w_mid[2]["n_seeds"] and stats[0]["n_chunks"] == w_mid[2]["n_chunks"]
    assert stats[2]["n_windows"] == stats[0]["n_windows"] == stats[4]["n_windows"] > 100


@pytest.mark.parametrize("kw", [dict(index="sparse"), dict(circular=False)], ids=["sparse", "linear"])
def test_index_layout_and_linear_reference(sets, kw):
    from downpore_amd.mapping import Mapper
    want = _oneshot(sets, "fasta", MIDDLE, **kw)
    assert want[0].count("\n") > 100
    with Mapper(_product_ref(), **MAP, **kw) as m:
        for _ in range(2):
            st = _trimmed_batch(m, sets, "fasta", MIDDLE, want)
            if "index" in kw:
                assert st["index"]["layout"] == "sparse"


def test_all_sequences_with_a_sequence_too_short_for_a_join_chunk(sets):
    """the genome in three; the middle piece gets no join chunk, so the head is neither 2 nor T + T device reads"""
    from downpore_amd.mapping import Mapper
    G = GEN["genome"]
    cut = [0, 60_000, 60_600, G]
    want = _oneshot(sets, "fasta", MIDDLE, ref=_product_ref(cut=cut), tag="three", all_sequences=True)
    assert "is shorter than query_size" in want[1]
    assert len(set(ln.split("\t")[5] for ln in want[0].splitlines())) >= 2 and want[0].count("\n") > 100
    with Mapper(_product_ref(cut=cut), all_sequences=True, **MAP) as m:
        _trimmed_batch(m, sets, "fasta", MIDDLE, want)
        _trimmed_batch(m, sets, "fasta", MIDDLE, want)


def test_several_threads_keep_their_contexts_across_trimmed_batches(sets, monkeypatch):
    """the worker contexts are opened by the first batch whose thread plan asks for them - here a trimmed one - kept, and refreshed after
    every later tail: index_builds grows once and stays, and every batch is correct"""
    from downpore_amd.mapping import Mapper, map_reads
    w_mid, w_edge = _oneshot(sets, "fasta", MIDDLE), _oneshot(sets, "fastq", EDGES)
    few_want = map_reads(_product_ref(), reads_of(sets["few"], MIN_LENGTH, himem=False), **MAP)
    assert few_want[0].count("\n") >= 10
    monkeypatch.setenv("DP_MAP_THREADS", "3")
    monkeypatch.setenv("DP_TUNE", "map_min_reads_per_thread=30")
    builds = []
    with Mapper(_product_ref(), index="dense", **MAP) as m:
        for step in ("few", "middle", "edges", "few", "middle"):
            if step == "few":
                paf, err, st = m.map(reads_of(sets["few"], MIN_LENGTH, himem=False))
                assert (paf, err) == few_want[:2]
            elif step == "middle":
                st = _trimmed_batch(m, sets, "fasta", MIDDLE, w_mid)
            else:
                st = _trimmed_batch(m, sets, "fastq", EDGES, w_edge)
            builds.append(st["index"]["index_builds"])
    assert builds == [1, 3, 3, 3, 3]


def test_a_minimum_length_above_every_trimmed_read(sets):
    from downpore_amd.mapping import Mapper
    want = _oneshot(sets, "fasta", MIDDLE, min_length=6000)
    with Mapper(_product_ref(), min_length=6000, **MAP) as m:
        for _ in range(2):
            paf, err, st = m.map(_raw(sets), trim=dict(**MIDDLE, **_ads()))
            assert paf == want[0] == "" and err == want[1] and "Unmapped: 0\n" in err and "total: 0\n" in err
            assert len(st["trim"].table) == GEN["n_reads"] and np.array_equal(st["trim"].table, want[2]["trim"].table)


def test_a_trim_that_fails_leaves_the_mapper_usable(sets):
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    g, off = reference()
    plain_want = O.map_run(O.ReadSet(g, off, min_len=0, himem=False), O.ReadSet(fasta=sets["fasta"], min_len=MIN_LENGTH, himem=False), **MAP)
    w_mid = _oneshot(sets, "fasta", MIDDLE)
    empty = Reads(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), min_len=50, himem=False)
    failures = [(empty, MIDDLE, "no reads long enough to trim"),
                (None, dict(k=9), r"trim: k = 9 is outside 3\.\.8"),
                (None, dict(k=6, middle=True, chunk_size=100), "trim: -chunk_size must be larger than 100")]
    m = Mapper(_product_ref(), **MAP)
    try:
        _trimmed_batch(m, sets, "fasta", MIDDLE, w_mid)
        for raw, bad, reason in failures:
            with pytest.raises(DpError, match="dph_mapper_map_trim: .*" + reason):
                m.map(raw if raw is not None else _raw(sets), trim=dict(**bad, **_ads()))
            _trimmed_batch(m, sets, "fasta", MIDDLE, w_mid)
            paf, err, st = m.map(reads_of(sets["fasta"], MIN_LENGTH, himem=False))
            assert (paf, err) == plain_want
        m.close()
        with pytest.raises(DpError, match="closed"):
            m.map(_raw(sets), trim=dict(**MIDDLE, **_ads()))
    finally:
        m.close()


def test_c_abi_by_ctypes_alone(sets):
    """the header's names and nothing else"""
    from downpore_amd.overlap import host_lib_path
    H = C.CDLL(host_lib_path())
    vp, i64 = C.c_void_p, C.c_int64
    H.dph_reads_from_fasta.restype = vp
    H.dph_reads_from_fasta.argtypes = [C.c_char_p, i64, C.c_int]
    H.dph_reads_from_arrays.restype = vp
    H.dph_reads_from_arrays.argtypes = [vp, vp, i64, i64, C.c_int]
    H.dph_reads_free.argtypes = [vp]
    H.dph_last_error.restype = C.c_char_p
    H.dph_last_error.argtypes = [vp]
    H.dph_mapper_open.restype = vp
    H.dph_mapper_open.argtypes = [vp, vp, C.c_int, C.c_int]
    H.dph_mapper_map_trim.restype = vp
    H.dph_mapper_map_trim.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
    H.dph_mapper_close.argtypes = [vp]
    H.dph_map_free.argtypes = [vp]
    H.dph_trim_free.argtypes = [vp]
    for f in (H.dph_map_paf, H.dph_map_errtext, H.dph_trim_errtext):
        f.restype = C.POINTER(C.c_char)
        f.argtypes = [vp, C.POINTER(i64)]
    H.dph_trim_table.restype = i64
    H.dph_trim_table.argtypes = [vp, vp, i64]
    want = _oneshot(sets, "fasta", MIDDLE)
    g, off = reference()
    g, off = np.ascontiguousarray(g, dtype=np.uint8), np.ascontiguousarray(off, dtype=np.int64)
    ref = H.dph_reads_from_arrays(g.ctypes.data, off.ctypes.data, 1, 0, 0)
    front, back = H.dph_reads_from_fasta(str(TC.FRONT).encode(), 0, 0), H.dph_reads_from_fasta(str(TC.BACK).encode(), 0, 0)
    assert ref and front and back
    p = np.array([1, MAP["k"], 1000, MIN_LENGTH, 10000, 40, 0, 0], dtype=np.int64)
    tp = np.array([6, 10000, 90, 5, 1, 0, 1, 1, 1, 5000, 85, 100, 0, 300_000_000], dtype=np.int64)
    m = H.dph_mapper_open(ref, p.ctypes.data, len(p), 0)
    assert m, H.dph_last_error(None)
    th = vp(0x1234)
    raw = H.dph_reads_from_fasta(sets["fasta"].encode(), 50, 0)
    assert not H.dph_mapper_map_trim(m, raw, front, back, tp.ctypes.data, 9, C.byref(th)) and not th.value
    assert H.dph_last_error(None).startswith(b"dph_mapper_map_trim: bad arguments")  # (refused for its arguments: still usable)
    H.dph_reads_free(raw)
    for _ in range(2):
        raw = H.dph_reads_from_fasta(sets["fasta"].encode(), 50, 0)
        h = H.dph_mapper_map_trim(m, raw, front, back, tp.ctypes.data, len(tp), C.byref(th))
        assert h and th.value, H.dph_last_error(None)
        n = i64(0)
        paf = C.string_at(H.dph_map_paf(h, C.byref(n)), n.value).decode()
        err = C.string_at(H.dph_map_errtext(h, C.byref(n)), n.value).decode()
        log = C.string_at(H.dph_trim_errtext(th, C.byref(n)), n.value).decode()
        table = np.zeros((GEN["n_reads"], 5), dtype=np.int32)
        assert H.dph_trim_table(th, table.ctypes.data, GEN["n_reads"]) == GEN["n_reads"]
        H.dph_map_free(h)
        H.dph_trim_free(th)
        H.dph_reads_free(raw)
        assert paf == want[0] and err == want[1] and log == want[2]["trim"].stderr
        assert np.array_equal(table, want[2]["trim"].table)
    H.dph_mapper_close(m)
    for r in (ref, front, back):
        H.dph_reads_free(r)
