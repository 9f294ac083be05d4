"""`map` with the trim in front on the GPU.  The kernel behind it (repack_spans_rc_kernel through Context.respan_rc) against two
independent expectations - the host packer plus reverse strands computed from codes (tests/test_map_trim_cpu.py holds that computation
to the packer on ASCII reverse complements), and what dp_reads_upload_rc stores for the host-cut slices, the path `map` trusts without a
trim - then the whole run, FASTA and FASTQ, with the middle stage and without, against the oracle's map_run over the MODEL's trimmed
output and against the product's own two steps, and the variants of `map` against the two steps.  Integers and text: equal means equal."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import trim_cases as TC
from tests import trim_mid_model as MM
from tests import trim_model as M
from tests.test_map_trim_cpu import MAP, MIN_LENGTH, SRC_LENS, pack, reference, reverse_strand, sources
from tests.test_overlap_trim_cpu import GEN, dump, generate, reads_of, written
from tests.test_overlap_trim_gpu import WRITING, _span_list

pytestmark = pytest.mark.gpu

BIG = len(SRC_LENS) - 1  # the 70 001-base source


# ---- repack_spans_rc_kernel ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_case():
    """sources, spans and both strands of every span as the host computes them, made once"""
    seqs = sources()
    spans = [tuple(int(v) for v in sp) for sp in _span_list(seqs[:BIG])]  # every start % 16 x every length, shuffled; one source used twice
    n = len(seqs[BIG])
    big = [(BIG, 4096 * a + 16 * (a + ln) + a, ln) for a in range(16) for ln in (1, 15, 16, 17, 63, 64, 65)]  # every alignment, in many workgroups
    big.append((BIG, 5, n - 5))  # ... and to the end
    big = [big[i] for i in np.random.default_rng(8).permutation(len(big))]
    spans += big
    spans.append((BIG, 3, 69_990))    # one read that spans many workgroups
    spans.append((BIG, n - 17, 17))   # ends on the last base of the last read of the buffer
    spans = np.array(spans, dtype=np.uint32)
    assert len(spans) > 500 and set((spans[:, 1] % 16).tolist()) == set(range(16))
    assert all(st + ln <= len(seqs[r]) for r, st, ln in spans.tolist())
    cuts = [seqs[r][st:st + ln] for r, st, ln in spans.tolist()]
    fw = [pack(c) for c in cuts]
    rv = [reverse_strand(p, len(c)) for p, c in zip(fw, cuts)]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return dict(seqs=seqs, bases=np.frombuffer(b"".join(seqs), dtype=np.uint8), off=off, spans=spans, cuts=cuts, fw=fw, rv=rv)


def _upload(kc):
    from downpore_amd import hip
    ctx = hip.Context()
    ctx.upload_reads(kc["bases"], kc["off"])
    return ctx


def _expected(kc, first_paired):
    """the packed bytes of every device read, in device order"""
    out = []
    for i in range(len(kc["spans"])):
        out.append(kc["fw"][i])
        if i >= first_paired:
            out.append(kc["rv"][i])
    return out


@pytest.mark.parametrize("where", ["all-paired", "half-paired", "none-paired"])
def test_respan_rc_equals_the_host_expectation_and_upload_rc_of_the_cut_slices(kernel_case, where):
    from downpore_amd import hip
    kc = kernel_case
    n_out = len(kc["spans"])
    first_paired = {"all-paired": 0, "half-paired": n_out // 2, "none-paired": n_out}[where]
    ctx = _upload(kc)
    ctx.respan_rc(kc["spans"], first_paired)
    # the path `map` trusts today: the host-cut ASCII slices through dp_reads_upload_rc
    other = hip.Context()
    coff = np.concatenate([[0], np.cumsum([len(c) for c in kc["cuts"]])]).astype(np.int64)
    other.upload_reads_rc(np.frombuffer(b"".join(kc["cuts"]), dtype=np.uint8), coff, first_paired)
    want = _expected(kc, first_paired)
    n_dev = first_paired + 2 * (n_out - first_paired)
    assert len(want) == n_dev == ctx.L.dp_reads_count(ctx.h) == other.L.dp_reads_count(other.h)
    assert ctx.L.dp_reads_total_bases(ctx.h) == other.L.dp_reads_total_bases(other.h) == int(other.read_len.sum())
    assert np.array_equal(ctx.read_len, other.read_len)
    for d in range(n_dev):
        got = ctx.packed_read(d)
        assert np.array_equal(got, want[d]), (d, "host expectation")
        assert np.array_equal(got, other.packed_read(d)), (d, "dp_reads_upload_rc")
    ctx.close()
    other.close()


def test_respan_rc_identity_and_empty(kernel_case):
    kc = kernel_case
    seqs = kc["seqs"]
    ctx = _upload(kc)
    before = [ctx.packed_read(r).copy() for r in range(len(seqs))]
    ident = np.array([(r, 0, len(s)) for r, s in enumerate(seqs)], dtype=np.uint32)
    ctx.respan_rc(ident, len(seqs))
    assert ctx.L.dp_reads_count(ctx.h) == len(seqs)
    for r in range(len(seqs)):
        assert np.array_equal(ctx.packed_read(r), before[r]) and np.array_equal(before[r], pack(seqs[r]))
    ctx.respan_rc(np.zeros((0, 3), dtype=np.uint32), 0)
    assert ctx.L.dp_reads_count(ctx.h) == 0 and ctx.L.dp_reads_total_bases(ctx.h) == 0
    ctx.close()


def test_respan_rc_refusals_name_the_call_and_the_reason_and_change_nothing(kernel_case, monkeypatch):
    from downpore_amd import hip
    kc = kernel_case
    n_src = len(SRC_LENS)
    one = np.array([(0, 0, 1)], dtype=np.uint32)
    ctx = _upload(kc)
    before = [ctx.packed_read(r).copy() for r in range(n_src)]

    def unchanged(c=ctx):
        assert c.L.dp_reads_count(c.h) == n_src and c.L.dp_reads_total_bases(c.h) == sum(SRC_LENS)
        assert all(np.array_equal(c.packed_read(r), before[r]) for r in range(n_src))

    with pytest.raises(hip.DpError, match="dp_reads_respan_rc: span 1 lies outside its read"):
        ctx.respan_rc(np.array([(0, 0, 1), (10, 990, 11)], dtype=np.uint32), 0)
    unchanged()
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc: span 0 lies outside its read"):
        ctx.respan_rc(np.array([(n_src, 0, 1)], dtype=np.uint32), 1)
    unchanged()
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc: first_paired 2 is beyond the 1 spans"):
        ctx.respan_rc(one, 2)
    unchanged()
    borrower = hip.Context(shared_from=ctx)
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc while contexts borrowing these reads exist"):
        ctx.respan_rc(one, 0)
    unchanged()
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc on a context that borrows its reads"):
        borrower.respan_rc(one, 0)
    unchanged()
    borrower.close()
    # a read set of dp_reads_upload_rc_begin stays pending until the owner's final wait
    L = ctx.L
    L.dp_reads_upload_rc_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    L.dp_reads_upload_wait.argtypes = [C.c_void_p, C.c_uint32]
    travelling = hip.Context()
    travelling._chk(L.dp_reads_upload_rc_begin(travelling.h, kc["bases"].ctypes.data, kc["off"].ctypes.data, n_src, n_src, n_src))
    travelling.read_len = np.diff(kc["off"])
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc while an upload of dp_reads_upload_rc_begin is pending"):
        travelling.respan_rc(one, 0)
    travelling._chk(L.dp_reads_upload_wait(travelling.h, 0xffffffff))
    unchanged(travelling)
    travelling.respan_rc(one, 0)  # (the upload joined, the call goes through)
    assert L.dp_reads_count(travelling.h) == 2
    travelling.close()
    # a resident k-mer position index
    monkeypatch.setenv("DP_SCAN_INDEX", "1")
    indexed = _upload(kc)
    indexed.scan_prepare(10)
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc after a k-mer position index"):
        indexed.respan_rc(one, 0)
    unchanged(indexed)
    indexed.close()
    monkeypatch.delenv("DP_SCAN_INDEX")
    # an open round
    ctx.round_begin(10, np.arange(5, dtype=np.uint32))
    with pytest.raises(hip.DpError, match="dp_reads_respan_rc after dp_round_begin"):
        ctx.respan_rc(one, 0)
    unchanged()
    ctx.close()


def test_a_value_table_is_no_reason_to_refuse_respan_rc_and_still_one_for_respan(kernel_case):
    """`map` makes the reference's value table before its reads arrive"""
    from downpore_amd import hip
    kc = kernel_case
    ctx = _upload(kc)
    ctx.kmer_values(10)
    with pytest.raises(hip.DpError, match="dp_reads_respan after"):
        ctx.respan(kc["spans"][:3])
    sel = np.concatenate([kc["spans"][:40], kc["spans"][-2:]])
    ctx.respan_rc(sel, 1)
    idx = list(range(40)) + [len(kc["spans"]) - 2, len(kc["spans"]) - 1]
    want = [kc["fw"][idx[0]]]
    for i in idx[1:]:
        want += [kc["fw"][i], kc["rv"][i]]
    assert ctx.L.dp_reads_count(ctx.h) == len(want)
    for d, w in enumerate(want):
        assert np.array_equal(ctx.packed_read(d), w), d
    ctx.close()


# ---- the whole run ---------------------------------------------------------------------------------------------------------------
def _ads():
    return dict(front=reads_of(TC.FRONT, 0), back=reads_of(TC.BACK, 0))


def _product_ref(cut=None):
    from downpore_amd.overlap import Reads
    g, off = reference()
    if cut is not None:
        off = np.array(cut, dtype=np.int64)
    return Reads(g, off, min_len=0, himem=False)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("map_trim_gpu")
    out = {"dir": d}
    for fastq in (False, True):
        names, seqs, quals, kinds = generate(fastq=fastq, **GEN)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = dict(path=path)
    return out


@pytest.mark.parametrize("middle", [True, False], ids=["middle", "edges-only"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_the_fused_run_equals_the_oracle_on_the_models_output_and_the_two_steps(sets, fmt, middle):
    from downpore_amd import trim as T
    from downpore_amd.mapping import map_reads
    s = sets[fmt]
    m = MM.run(s["path"], k=6) if middle else M.run(s["path"], k=6)
    assert WRITING in m.stderr
    trimmed = written(sets["dir"], m, fmt == "fastq", "model_%d" % middle)
    g, off = reference()
    want, _ = O.map_run(O.ReadSet(g, off, min_len=0, himem=False), O.ReadSet(fasta=trimmed, min_len=MIN_LENGTH, himem=False), **MAP)
    assert want.count("\n") > 100
    if middle:
        assert "_(left)" in want and "_(right)" in want
    ref = _product_ref()
    raw = reads_of(s["path"], himem=False)
    got, gerr, st = map_reads(ref, raw, trim=dict(k=6, middle=middle, **_ads()), **MAP)
    assert got == want
    # the product's two steps
    raw2 = reads_of(s["path"], himem=False)
    res = T.trim_reads(raw2, k=6, middle=middle, **_ads())
    two, terr, _ = map_reads(ref, res.reads(MIN_LENGTH, himem=False), **MAP)
    assert got == two and gerr == terr
    t = st["trim"]
    assert dump(t.reads(MIN_LENGTH, himem=False)) == dump(reads_of(trimmed, MIN_LENGTH, himem=False))
    assert np.array_equal(t.table, m.table) and t.adapters == m.adapters
    if middle:
        assert np.array_equal(t.splits, m.splits) and t.extras == m.extras and len(m.extras) >= 6
    assert t.output == "" and t.stderr == m.stderr.replace(WRITING, "")
    # one crossing: ids and spans went up, never bases
    assert 0 < t.stats["bytes_up"] * 10 < raw.total_bases()


@pytest.fixture(scope="module")
def two_steps(sets):
    """the trim of the product's two steps, run once for the variants: its result hands out the trimmed reads at any minimum length"""
    from downpore_amd import trim as T
    raw = reads_of(sets["fasta"]["path"], himem=False)
    res = T.trim_reads(raw, k=6, middle=True, **_ads())
    return dict(raw=raw, res=res)


def _both(sets, two_steps, ref=None, min_length=MIN_LENGTH, **kw):
    """(fused PAF, stats) after holding PAF and stderr text to the two steps' with the same settings"""
    from downpore_amd.mapping import map_reads
    ref = ref if ref is not None else _product_ref()
    fused, ferr, st = map_reads(ref, reads_of(sets["fasta"]["path"], himem=False), trim=dict(k=6, middle=True, **_ads()), min_length=min_length,
                                **MAP, **kw)
    two, terr, _ = map_reads(ref, two_steps["res"].reads(min_length, himem=False), min_length=min_length, **MAP, **kw)
    assert fused == two and ferr == terr
    return fused, ferr, st


def test_linear_reference_and_sparse_index(sets, two_steps):
    plain, _, _ = _both(sets, two_steps)
    linear, _, _ = _both(sets, two_steps, circular=False)
    assert linear.count("\n") > 100  # (no read of this input maps across the join: the text may equal the circular run's)
    sparse, _, st = _both(sets, two_steps, index="sparse")
    assert st["index"]["layout"] == "sparse" and sparse == plain


def test_sharded_index(sets, two_steps, monkeypatch):
    """chunk_size = 1 500 makes more than 64 chunks of the 100 kb genome, so that two shards really hold two ranges (whole 64-chunk words)"""
    plain, _, _ = _both(sets, two_steps, chunk_size=1500)
    monkeypatch.setenv("DP_MAP_SHARDS", "2")
    sharded, _, st = _both(sets, two_steps, chunk_size=1500)
    monkeypatch.delenv("DP_MAP_SHARDS")
    assert st["n_chunks"] > 64 and sharded == plain and plain.count("\n") > 100


def test_all_sequences_with_a_sequence_too_short_for_a_join_chunk(sets, two_steps):
    """the genome in three; the middle piece is shorter than query_size and gets no join chunk, so that the first paired device read is
    neither 2 nor T + T"""
    G = GEN["genome"]
    ref = _product_ref(cut=[0, 60_000, 60_600, G])
    paf, err, _ = _both(sets, two_steps, ref=ref, all_sequences=True)
    assert "is shorter than query_size" in err
    assert len(set(ln.split("\t")[5] for ln in paf.splitlines())) >= 2 and paf.count("\n") > 100


def test_the_other_upload_paths_are_not_consulted(sets, two_steps, monkeypatch):
    plain, perr, _ = _both(sets, two_steps)
    for tune in ("map_async_upload=1", "map_ascii_upload=1"):
        monkeypatch.setenv("DP_TUNE", tune)
        got, gerr, _ = _both(sets, two_steps)
        assert got == plain and gerr == perr, tune
    monkeypatch.delenv("DP_TUNE")


def test_a_minimum_length_above_every_trimmed_read(sets, two_steps):
    paf, err, st = _both(sets, two_steps, min_length=6000)
    assert paf == "" and "Unmapped: 0\n" in err and "total: 0\n" in err
    assert len(st["trim"].table) == GEN["n_reads"]


def test_an_empty_raw_read_set_fails_as_the_two_steps_do():
    from downpore_amd import trim as T
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    ref = _product_ref()

    def empty():
        return Reads(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64), min_len=50, himem=False)

    with pytest.raises(DpError, match="no reads long enough to trim"):
        T.trim_reads(empty(), k=6, middle=True, **_ads())
    with pytest.raises(DpError, match="dph_map_run_trim: .*no reads long enough to trim"):
        map_reads(ref, empty(), trim=dict(k=6, middle=True, **_ads()), **MAP)


def test_a_trim_that_fails_before_or_during_its_device_work_fails_as_the_two_steps_do(sets):
    """k = 9 is refused when the adapters are indexed, before anything goes up; chunk_size = 100 by the middle stage's plan, after the
    upload and the edge stage, while the context exists.  Either way: DpError with the trim's own reason, nothing left behind, and the
    next run is as good as any"""
    from downpore_amd import trim as T
    from downpore_amd.hip import DpError
    from downpore_amd.mapping import map_reads
    ref = _product_ref()
    path = sets["fasta"]["path"]
    for bad, reason in ((dict(k=9), r"k = 9 is outside 3\.\.8"), (dict(k=6, middle=True, chunk_size=100), "-chunk_size must be larger than 100")):
        with pytest.raises(DpError, match="dph_trim_run: trim: " + reason):
            T.trim_reads(reads_of(path, himem=False), **bad, **_ads())
        with pytest.raises(DpError, match="dph_map_run_trim: trim: " + reason):
            map_reads(ref, reads_of(path, himem=False), trim=dict(**bad, **_ads()), **MAP)
    good, _, st = map_reads(ref, reads_of(path, himem=False), trim=dict(k=6, middle=True, **_ads()), **MAP)
    assert good.count("\n") > 100 and "_(left)" in good and len(st["trim"].table) == GEN["n_reads"]


def test_map_without_a_trim_is_unchanged(sets):
    from downpore_amd.mapping import map_reads
    g, off = reference()
    path = sets["fasta"]["path"]
    want, werr = O.map_run(O.ReadSet(g, off, min_len=0, himem=False), O.ReadSet(fasta=path, min_len=MIN_LENGTH, himem=False), **MAP)
    got, gerr, st = map_reads(_product_ref(), reads_of(path, MIN_LENGTH, himem=False), trim=None, **MAP)
    assert got == want and gerr == werr and want.count("\n") > 100 and "trim" not in st
