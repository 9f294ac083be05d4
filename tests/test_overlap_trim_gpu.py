"""`overlap -trim true` on the GPU: the two kernels behind it each against an independent host computation (repack_spans_kernel through
Context.respan, unpack_spans_kernel through the resident forms of the edge call and of the chunk scan), then the whole command - library
and CLI, FASTA and FASTQ, with the middle stage and without - against the oracle's OverlapRun over the MODEL's trimmed output, which
shares no code with the product, and against the product's own two commands through a file.  Integers and text: equal means equal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import trim_cases as TC
from tests import trim_mid_cases as MC
from tests import trim_mid_model as MM
from tests import trim_model as M
from tests.test_overlap_trim_cpu import GEN, OVERLAP, dump, generate, reads_of, written
from tests.test_trim_cpu import CLI

pytestmark = pytest.mark.gpu


# ---- repack_spans_kernel ---------------------------------------------------------------------------------------------------------
SRC_LENS = [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1000]  # 64 bases = 16 packed bytes: the boundary every read starts on


def _pack(seq):
    """dph_pack_bases of a host slice: ceil(n / 4) bytes, the last byte's unused bits zero"""
    from downpore_amd.overlap import load_host
    H = load_host()
    H.dph_pack_bases.restype = None
    H.dph_pack_bases.argtypes = [C.c_char_p, C.c_int64, C.c_void_p, C.c_int]
    out = np.zeros((len(seq) + 3) // 4, dtype=np.uint8)
    if len(seq):
        H.dph_pack_bases(bytes(seq), len(seq), out.ctypes.data, 0)
        if len(seq) % 4:
            assert out[-1] & ((1 << (2 * (4 - len(seq) % 4))) - 1) == 0
    return out


def _sources():
    rng = np.random.default_rng(91)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnUuRY", dtype=np.uint8)
    seqs = [alphabet[rng.integers(0, len(alphabet), n)].tobytes() for n in SRC_LENS]
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return seqs, np.frombuffer(b"".join(seqs), dtype=np.uint8), off


def _upload(seqs_bases_off):
    from downpore_amd import hip
    _, bases, off = seqs_bases_off
    ctx = hip.Context()
    ctx.upload_reads(bases, off)
    return ctx


def _span_list(seqs):
    """every start % 16 with every length of the list, as far as each read allows; the order is not monotone in the source"""
    spans = []
    for r, s in enumerate(seqs):
        n = len(s)
        for start in sorted(set(list(range(min(n, 16))) + [st for st in (16, 17, 47, 48, 63, 64, 65, 500, 990) if st < n])):
            for ln in sorted(set([1, 15, 16, 17, 63, 64, 65, n - start])):
                if 0 < ln <= n - start:
                    spans.append((r, start, ln))
    spans = [spans[i] for i in np.random.default_rng(4).permutation(len(spans))]
    last = len(seqs) - 1
    spans.append((last, len(seqs[last]) - 17, 17))  # ends on the last base of the last read of the buffer
    spans.append((4, 0, 63))                          # ... and one source used twice, whole
    spans.append((4, 0, 63))
    return np.array(spans, dtype=np.uint32)


def test_respan_equals_the_host_packer_on_every_alignment():
    src = _sources()
    seqs = src[0]
    spans = _span_list(seqs)
    assert len(spans) > 500 and set(spans[:, 1] % 16) == set(range(16))
    assert (np.diff(spans[:, 0].astype(np.int64)) < 0).any()
    ctx = _upload(src)
    ctx.respan(spans)
    assert ctx.L.dp_reads_count(ctx.h) == len(spans)
    assert ctx.L.dp_reads_total_bases(ctx.h) == int(spans[:, 2].sum())
    for i, (r, start, ln) in enumerate(spans.tolist()):
        got = ctx.packed_read(i)
        want = _pack(seqs[r][start:start + ln])
        assert np.array_equal(got, want), (i, r, start, ln)
    ctx.close()


def test_respan_identity_and_empty():
    src = _sources()
    seqs = src[0]
    ctx = _upload(src)
    before = [ctx.packed_read(r).copy() for r in range(len(seqs))]
    ctx.respan(np.array([(r, 0, len(s)) for r, s in enumerate(seqs)], dtype=np.uint32))
    assert ctx.L.dp_reads_count(ctx.h) == len(seqs)
    for r in range(len(seqs)):
        assert np.array_equal(ctx.packed_read(r), before[r]) and np.array_equal(before[r], _pack(seqs[r]))
    ctx.respan(np.zeros((0, 3), dtype=np.uint32))
    assert ctx.L.dp_reads_count(ctx.h) == 0 and ctx.L.dp_reads_total_bases(ctx.h) == 0
    ctx.close()


def test_respan_refusals_name_their_reason():
    from downpore_amd import hip
    src = _sources()
    ctx = _upload(src)
    with pytest.raises(hip.DpError, match="span 1 lies outside its read"):
        ctx.respan(np.array([(0, 0, 1), (10, 990, 11)], dtype=np.uint32))
    with pytest.raises(hip.DpError, match="outside its read"):
        ctx.respan(np.array([(len(SRC_LENS), 0, 1)], dtype=np.uint32))
    assert ctx.L.dp_reads_count(ctx.h) == len(SRC_LENS)  # a refused call changes nothing
    borrower = hip.Context(shared_from=ctx)
    with pytest.raises(hip.DpError, match="borrowing these reads"):
        ctx.respan(np.array([(0, 0, 1)], dtype=np.uint32))
    with pytest.raises(hip.DpError, match="borrows its reads"):
        borrower.respan(np.array([(0, 0, 1)], dtype=np.uint32))
    borrower.close()
    ctx.respan(np.array([(10, 1, 999)], dtype=np.uint32))  # (the borrower gone, the call goes through)
    ctx.round_begin(10, np.arange(5, dtype=np.uint32))
    with pytest.raises(hip.DpError, match="dp_round_begin"):
        ctx.respan(np.array([(0, 0, 1)], dtype=np.uint32))
    ctx.close()


# ---- unpack_spans_kernel, ends ---------------------------------------------------------------------------------------------------------
END_LENS = [200, 201, 202, 203, 299, 300, 301, 5000]


@pytest.fixture(scope="module")
def end_reads():
    """reads of the lengths above that keep both 150-base ends of reads of trim_cases' kernel-level set (adapters are found), with
    N, U and lower-case letters mixed in; a few reads below 200 bases sit between them and are not listed"""
    names, seqs, _, _ = TC.generate(seed=20260, n_reads=400)
    donors = [s for s in seqs if len(s) >= 320][:48]
    filler = TC.random_bases(5, 6000)
    rng = np.random.default_rng(17)
    out = []
    for i, s in enumerate(donors):
        L = END_LENS[i % len(END_LENS)]
        a, b = (L + 1) // 2, L // 2
        r = s[:a] + s[-b:] if L < 300 else s[:150] + filler[i:i + L - 300] + s[-150:]
        assert len(r) == L
        r = list(r)
        for p in rng.integers(0, L, max(2, L // 40)):
            r[p] = ("N", "U", r[p].lower())[int(rng.integers(3))]
        out.append("".join(r))
        if i % 5 == 0:
            out.append(filler[:150 + i])
    off = np.concatenate([[0], np.cumsum([len(r) for r in out])]).astype(np.int64)
    bases = np.frombuffer("".join(out).encode(), dtype=np.uint8)
    ends, ids = TC.ends_of(out)
    assert sorted(set(len(out[i]) for i in ids)) == END_LENS and len(ids) < len(out)
    order = np.random.default_rng(2).permutation(len(ids))  # the id list need not ascend
    return dict(bases=bases, off=off, ends=ends[order], ids=ids[order])


@pytest.mark.parametrize("k", [5, 8], ids=["k5-table-in-lds", "k8-table-through-l2"])
def test_edges_resident_equals_edges_on_host_extracted_ends(end_reads, k):
    from downpore_amd import hip
    from downpore_amd import trim as T
    ix = T.trim_index(reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0), k)
    ctx = hip.Context()
    ctx.upload_reads(end_reads["bases"], end_reads["off"])
    a, b = T.TrimDevice(ix), T.TrimDevice(ix)
    want, want_counts, _ = a.edges(end_reads["ends"])
    got, got_counts, _ = b.edges_resident(ctx, end_reads["ids"])
    assert want[:, 2].sum() > 10 and want_counts.sum() > 10  # adapters are found
    assert np.array_equal(got, want)
    assert np.array_equal(got_counts, want_counts)
    a.close()
    b.close()
    a, b = T.TrimDevice(ix), T.TrimDevice(ix)
    want_en, _ = a.edges(end_reads["ends"], mode=T.MODE_DETERMINE, threshold=90)
    got_en, _ = b.edges_resident(ctx, end_reads["ids"], mode=T.MODE_DETERMINE, threshold=90)
    assert 0 < want_en.sum() < len(want_en)
    assert np.array_equal(got_en, want_en)
    with pytest.raises(hip.DpError, match="200 bases"):
        short = int(np.nonzero(np.diff(end_reads["off"]) < 200)[0][0])
        b.edges_resident(ctx, np.array([short], dtype=np.uint32))
    a.close()
    b.close()
    ctx.close()


# ---- unpack_spans_kernel, chunks -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,chunk_size", [(6, 5000), (8, 1000)])
def test_scan_chunks_resident_equals_scan_chunks(tmp_path, k, chunk_size):
    from downpore_amd import hip
    from downpore_amd import trim as T
    from tests.test_trim_mid_gpu import _kernel_case
    m, dev, counts = _kernel_case(dict(dir=tmp_path), k, chunk_size, False)
    names, seqs, _, _ = MC.generate(seed=11, n_reads=60, chunk_size=chunk_size)  # (the input _kernel_case generated)
    e = M.run(str(tmp_path / ("kernel_%d_%d.fasta" % (k, chunk_size))), k=k, determine_adapters=False)
    spans = np.array([(r, e.table[r, 0] + s, en - s) for r, s, en, _, _, _ in m.plan.tolist()], dtype=np.uint32)
    assert (e.table[m.plan[:, 0], 0] > 0).any()  # chunks behind a non-zero front trim
    ctx = hip.Context()
    off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    ctx.upload_reads(np.frombuffer("".join(seqs).encode(), dtype=np.uint8), off)
    res = T.TrimDevice(T.trim_index(reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0), k))
    got, _ = res.scan_chunks_resident(ctx, spans)
    assert np.array_equal(got, counts) and counts.sum() > 0
    for c in range(len(spans)):
        assert np.array_equal(res.chunk_segments(c), dev.chunk_segments(c)), c
    sel = np.nonzero(m.plan[:, 5])[0]
    a, b = dev.search(sel), res.search(sel)
    assert len(a["recs"]) > 0
    assert np.array_equal(a["recs"], b["recs"]) and np.array_equal(a["overflow"], b["overflow"]) and a["pairs"] == b["pairs"]
    with pytest.raises(hip.DpError, match="outside its read"):
        res.scan_chunks_resident(ctx, np.array([(0, len(seqs[0]) - 5, 6)], dtype=np.uint32))
    dev.close()
    res.close()
    ctx.close()


# ---- the whole thing -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_trim_gpu")
    out = {"dir": d}
    for fastq in (False, True):
        names, seqs, quals, kinds = generate(fastq=fastq, **GEN)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = dict(path=path, seqs=seqs)
    return out


def _unstamp(text):
    """stderr lines without log.Println's `2006/01/02 15:04:05 ` prefix where they carry one"""
    out = []
    for ln in text.splitlines():
        if len(ln) > 20 and ln[4] == "/" and ln[7] == "/" and ln[10] == " " and ln[13] == ":" and ln[16] == ":" and ln[19] == " ":
            ln = ln[20:]
        out.append(ln)
    return out


WRITING = "Writing trimmed sequences...\n"


@pytest.mark.parametrize("middle", [True, False], ids=["middle", "edges-only"])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_the_fused_run_equals_the_oracle_on_the_models_output_and_the_two_commands(sets, fmt, middle):
    from downpore_amd.overlap import OverlapPipeline
    s = sets[fmt]
    m = MM.run(s["path"], k=6) if middle else M.run(s["path"], k=6)
    assert WRITING in m.stderr
    trimmed = written(sets["dir"], m, fmt == "fastq", "model_%d" % middle)
    oreads = O.ReadSet(fasta=trimmed, min_len=OVERLAP["overlap_size"])
    want = O.OverlapRun(oreads, **OVERLAP)
    assert want.paf.count("\n") > 0
    if middle:
        assert "_(left)" in want.paf or "_(right)" in want.paf
    # the library
    raw = reads_of(s["path"])
    pipe = OverlapPipeline(raw, trim=dict(front=reads_of(TC.FRONT, 0), back=reads_of(TC.BACK, 0), k=6, middle=middle), **OVERLAP)
    while pipe.step():
        pass
    assert pipe.all_paf() == want.paf
    assert np.array_equal(pipe.reads.ignore(), oreads.ignore())
    assert dump(pipe.reads) == dump(reads_of(trimmed, OVERLAP["overlap_size"]))
    t = pipe.trim
    assert np.array_equal(t.table, m.table) and t.adapters == m.adapters
    if middle:
        assert np.array_equal(t.splits, m.splits) and t.extras == m.extras and len(m.extras) >= 6
    assert t.output == "" and t.stderr == m.stderr.replace(WRITING, "")
    # one crossing: ids and spans went up (4 bytes per read and pass, 12 per chunk and scan), never bases - the host-extracted path
    # sends 300 bytes per read and every centre at a byte per base
    assert 0 < t.stats["bytes_up"] * 10 < raw.total_bases()
    pipe.close()
    # the command line, and the same build's two commands through a file
    env = {k: v for k, v in os.environ.items() if k != "DP_TRIM_MIDDLE"}
    if middle:
        env["DP_TRIM_MIDDLE"] = "1"
    ads = ["-front_adapters", TC.FRONT, "-back_adapters", TC.BACK]
    fused = subprocess.run([CLI, "overlap", "-input", s["path"], "-trim", "true", "-k", str(OVERLAP["k"])] + ads, capture_output=True, text=True,
                           timeout=300, env=env)
    assert fused.returncode == 0, fused.stderr[-2000:]
    assert fused.stdout == want.paf
    first = subprocess.run([CLI, "trim", "-input", s["path"]] + ads, capture_output=True, text=True, timeout=300, env=env)
    assert first.returncode == 0 and first.stdout == m.output
    through = str(sets["dir"] / ("two_commands_%d.%s" % (middle, fmt)))
    with open(through, "w") as f:
        f.write(first.stdout)
    second = subprocess.run([CLI, "overlap", "-input", through, "-k", str(OVERLAP["k"])], capture_output=True, text=True, timeout=300, env=env)
    assert second.returncode == 0 and second.stdout == fused.stdout
    # trim's notice and log first (minus the line about writing), then overlap's own lines
    assert _unstamp(fused.stderr) == [ln for ln in _unstamp(first.stderr) if ln + "\n" != WRITING] + _unstamp(second.stderr)
    assert ("not part of this build" in fused.stderr) == (not middle)


def test_overlap_without_the_switch_is_unchanged(sets):
    s = sets["fasta"]
    want = O.OverlapRun(O.ReadSet(fasta=s["path"], min_len=OVERLAP["overlap_size"]), **OVERLAP)
    r = subprocess.run([CLI, "overlap", "-input", s["path"], "-k", str(OVERLAP["k"]), "-trim", "false"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want.paf and want.paf.count("\n") > 0


def test_map_on_trimmed_reads_equals_map_on_the_written_file(sets):
    from downpore_amd import trim as T
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    s = sets["fastq"]
    genome = np.frombuffer(O.gen_genome(GEN["seed"], GEN["genome"]), dtype=np.uint8)  # the genome the reads were drawn from
    ref = Reads(genome, np.array([0, GEN["genome"]], dtype=np.int64), min_len=0, himem=False)
    raw = reads_of(s["path"], himem=False)
    res = T.trim_reads(raw, reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0), k=6, middle=True)
    path = str(sets["dir"] / "for_map.fastq")
    with open(path, "w") as f:
        f.write(res.output)
    want, _, _ = map_reads(ref, reads_of(path, 500, himem=False), k=11)
    got, _, _ = map_reads(ref, res.reads(500, himem=False), k=11)
    assert want.count("\n") > 100 and "_(left)" in want
    assert got == want
