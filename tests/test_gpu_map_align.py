"""Mapper.map_aligned: the tags behind every PAF line are the model's (tests/native/align_model.cpp) on the spans the rule takes from
the line's own columns and the bases (rules 1 - 3), and everything in front of them is Mapper.map's, byte for byte.
A 200 kb circular synthetic reference and 60 reads of 3 kb; then once each a trimmed raw batch, two sequences with a wrapping read, a
linear mapper and the sparse index."""
import ctypes as C
import re

import numpy as np
import pytest

from tests import align_model as A
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

G, N, L = 200000, 60, 3000
COUNT_KEYS = ["n_chunks", "n_seeds", "n_windows", "n_chains", "n_batches"]
TAGS = re.compile(r"\tNM:i:(\d+)\tcg:Z:((?:\d+[MID])+)$")


def codes_of(ascii_bases):
    b = np.asarray(ascii_bases, dtype=np.uint8)
    return (((b >> 1) ^ ((b & 4) >> 2)) & 3).astype(np.uint8)  # the packer's 2-bit code of a letter


def split_tags(paf):
    """-> (the text without tags, per line its (NM, CIGAR) or None)"""
    plain, tags = [], []
    for ln in paf.splitlines():
        m = TAGS.search(ln)
        tags.append((int(m.group(1)), m.group(2)) if m else None)
        plain.append(ln[:m.start()] if m else ln)
        assert plain[-1].count("\t") == 11 and plain[-1].endswith("\t255"), ln[:200]
    return "".join(p + "\n" for p in plain), tags


def model_tags(line, read_codes, ref_codes, circular):
    """rules 1 - 3 on the line's columns, then the model; None = out of range.  read_codes / ref_codes: name -> codes"""
    f = line.split("\t")
    Lq, qs, qe, Lr, start, end = int(f[1]), int(f[2]), int(f[3]), int(f[6]), int(f[7]), int(f[8])
    read, ref = read_codes[f[0]], ref_codes[f[5]]
    assert len(read) == Lq and len(ref) == Lr
    tl = end - start
    if circular and tl < 0:
        tl += Lr
    if qs < 0 or qe > Lq or qs >= qe or tl < 1 or tl > Lr or start < 0 or (start > Lr if circular else end > Lr) or qe - qs > 1 << 20 or tl > 1 << 20:
        return None
    q = read[qs:qe]
    if f[4] == "-":
        q = (3 - q[::-1]).astype(np.uint8)
    t = ref[(start + np.arange(tl)) % Lr] if circular else ref[start:start + tl]
    return A.align(q, t), qe - qs, tl


def check_against_model(paf_aligned, paf_plain, read_codes, ref_codes, circular, max_edits=4096):
    """-> (tags per line, model NM per line); asserts text, tags and the CIGARs' sums"""
    plain, tags = split_tags(paf_aligned)
    assert plain == paf_plain
    nms = []
    for ln, tg in zip(plain.splitlines(), tags):
        want = model_tags(ln, read_codes, ref_codes, circular)
        assert want is not None, ln  # (nothing here is out of range)
        (nm, cigar), qlen, tlen = want
        nms.append(nm)
        if nm > max_edits:
            assert tg is None, ln
            continue
        assert tg == (nm, cigar), (ln, tg and tg[0], nm)
        assert A.consumed(tg[1]) == (qlen, tlen)  # M + I = qe - qs, M + D = tl
    return tags, nms


def _names(off):
    return ["r%07d" % i for i in range(len(off) - 1)]  # (the names a read set made from arrays gives)


def _codes_by_name(bases, off):
    c = codes_of(bases)
    return {nm: c[off[i]:off[i + 1]] for i, nm in enumerate(_names(off))}


def _counts(st):
    return {k: st[k] for k in COUNT_KEYS}, st["index"]


@pytest.fixture(scope="module")
def world():
    """the circular mapper, the 10 % batch and the error-free batch: map and map_aligned of each, computed once"""
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    from tools.synth import gen_reads_truth
    genome = np.frombuffer(O.gen_genome(3, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    ref = Reads(genome, goff, min_len=0, himem=False)
    w = dict(ref_codes={"r0000000": codes_of(genome)}, genome=(genome, goff))
    m = Mapper(ref, circular=True)
    w["mapper"] = m
    for name, e in (("noisy", 0.10), ("clean", 0.0)):
        bases, off, starts, strands = gen_reads_truth(3, G, N, L, e, False)  # (seed 3: reads of the genome above)
        if name == "clean":
            assert 0 < int(strands.sum()) < N  # both strands
        reads = Reads(bases, off, min_len=500, himem=False)
        w[name] = dict(reads=reads, codes=_codes_by_name(bases, off), plain=m.map(reads), aligned=m.map_aligned(reads))
    yield w
    m.close()


def test_tags_are_the_models_and_the_rest_is_maps(world):
    d = world["noisy"]
    (paf, err, st), (paf0, err0, st0) = d["aligned"], d["plain"]
    assert paf0.count("\n") >= N // 2 and "NM:i:" not in paf0 and "cg:Z:" not in paf0
    assert err == err0 and _counts(st) == _counts(st0) and "align" not in st0
    tags, nms = check_against_model(paf, paf0, d["codes"], world["ref_codes"], True)
    # zero untagged lines, and zero is the condition: spans under 4 000 bases have NM <= max(m, n) < 4096
    assert all(t is not None for t in tags)
    a = st["align"]
    lines = paf0.count("\n")
    assert (a["lines"], a["aligned"], a["over_max_edits"], a["out_of_range"]) == (lines, lines, 0, 0)
    assert a["cells"] > 0 and a["traceback_bytes"] > 0 and a["kernel_us"] >= 0
    assert max(nms) > 100  # (10 % errors: the alignments are not trivial)


def test_error_free_reads_pin_strand_and_wrap_conventions(world):
    """NM <= 60 per line on error-free reads of both strands - twice the 30-base end-point tolerance tests/test_ground_truth.py holds
    map to - whatever the model says: a flipped strand or a shifted wrap would cost hundreds of edits"""
    d = world["clean"]
    tags, nms = check_against_model(d["aligned"][0], d["plain"][0], d["codes"], world["ref_codes"], True)
    assert len(tags) >= N // 2 and all(t is not None and t[0] <= 60 for t in tags)
    assert {ln.split("\t")[4] for ln in d["plain"][0].splitlines()} == {"+", "-"}


def test_max_edits_64_untags_exactly_the_lines_above_it(world):
    d = world["noisy"]
    paf, err, st = world["mapper"].map_aligned(d["reads"], max_edits=64)
    tags, nms = check_against_model(paf, d["plain"][0], d["codes"], world["ref_codes"], True, max_edits=64)
    over = [nm > 64 for nm in nms]
    assert [t is None for t in tags] == over and any(over)
    assert st["align"]["over_max_edits"] == sum(over) and st["align"]["aligned"] == len(over) - sum(over) and st["align"]["out_of_range"] == 0


def test_refused_max_edits_leaves_the_mapper_usable_and_batches_alternate(world):
    from downpore_amd.hip import DpError
    m, d = world["mapper"], world["noisy"]
    for bad in (0, 40000):
        with pytest.raises(DpError, match="max_edits"):
            m.map_aligned(d["reads"], max_edits=bad)
        # ... and at the C boundary, past the Python check
        ap = np.array([bad], dtype=np.int64)
        th = C.c_void_p()
        assert not m.H.dph_mapper_map_align(m.h, d["reads"].h, None, None, None, 0, C.byref(th), ap.ctypes.data, 1)
        assert m.H.dph_last_error(None).decode().startswith("dph_mapper_map_align: bad arguments")
    # three batches on the one mapper: aligned, plain, aligned
    a1 = m.map_aligned(d["reads"])
    p = m.map(d["reads"])
    a2 = m.map_aligned(d["reads"])
    assert a1[0] == d["aligned"][0] == a2[0] and a1[1] == a2[1]
    assert p[0] == d["plain"][0] and p[1] == d["plain"][1] and "align" not in p[2]
    counts = [{k: v for k, v in x[2]["align"].items() if k != "kernel_us"} for x in (a1, a2, d["aligned"])]
    assert counts[0] == counts[1] == counts[2]


@pytest.mark.parametrize("setting", ["linear", "sparse"])
def test_linear_mapper_and_sparse_index(world, setting):
    from downpore_amd.mapping import Mapper
    from downpore_amd.overlap import Reads
    d = world["noisy"]
    kw = dict(circular=False) if setting == "linear" else dict(circular=True, index="sparse")
    with Mapper(Reads(*world["genome"], min_len=0, himem=False), **kw) as m:
        paf0, err0, st0 = m.map(d["reads"])
        paf, err, st = m.map_aligned(d["reads"])
    assert st["index"]["layout"] == ("sparse" if setting == "sparse" else st0["index"]["layout"])
    assert err == err0 and paf0.count("\n") >= N // 2
    tags, _ = check_against_model(paf, paf0, d["codes"], world["ref_codes"], kw["circular"])
    assert all(t is not None for t in tags)


def test_all_sequences_with_a_read_that_wraps_one_of_them():
    from downpore_amd.mapping import map_reads_aligned, Mapper
    from downpore_amd.overlap import Reads
    s0 = np.frombuffer(O.gen_genome(11, 120000), dtype=np.uint8)
    s1 = np.frombuffer(O.gen_genome(12, 80000), dtype=np.uint8)
    ref_bases, ref_off = np.concatenate([s0, s1]), np.array([0, 120000, 200000], dtype=np.int64)
    b0, o0 = O.gen_reads(11, 120000, 15, L, 0.05, False)
    b1, o1 = O.gen_reads(12, 80000, 15, L, 0.05, False)
    wrap = np.concatenate([s1[-1500:], s1[:1500]])
    bases = np.concatenate([b0, b1, wrap])
    off = np.concatenate([o0, o0[-1] + o1[1:], [o0[-1] + o1[-1] + len(wrap)]]).astype(np.int64)
    ref = Reads(ref_bases, ref_off, min_len=0, himem=False)
    reads = Reads(bases, off, min_len=500, himem=False)
    with Mapper(ref, circular=True, all_sequences=True) as m:
        paf0, err0, _ = m.map(reads)
    paf, err, st = map_reads_aligned(ref, reads, circular=True, all_sequences=True)
    assert err == err0
    ref_codes = {"r0000000": codes_of(s0), "r0000001": codes_of(s1)}
    tags, nms = check_against_model(paf, paf0, _codes_by_name(bases, off), ref_codes, True)
    assert all(t is not None for t in tags) and {ln.split("\t")[5] for ln in paf0.splitlines()} == {"r0000000", "r0000001"}
    wrapped = [(ln, t) for ln, t in zip(paf0.splitlines(), tags) if ln.split("\t")[0] == "r0000030" and int(ln.split("\t")[8]) < int(ln.split("\t")[7])]
    assert wrapped and all(ln.split("\t")[5] == "r0000001" and t[0] <= 60 for ln, t in wrapped)  # the wrapping read, error free, across r1's end


def test_trimmed_raw_batch(tmp_path):
    """trim=... on a raw batch: the reads that are mapped (and aligned) are the trimmed ones, cut on the device"""
    from downpore_amd.mapping import Mapper
    from tests import trim_cases as TC
    from tests.test_map_trim_cpu import MIN_LENGTH, reference
    from tests.test_map_trim_gpu import _ads, _product_ref
    from tests.test_overlap_trim_cpu import GEN, dump, generate, reads_of
    names, seqs, quals, kinds = generate(fastq=False, **GEN)
    path = str(tmp_path / "reads.fasta")
    TC.write_fasta(path, names[:80], seqs[:80], None)
    trim = dict(k=6, middle=True, **_ads())
    with Mapper(_product_ref(), k=11) as m:
        raw = reads_of(path, himem=False)
        paf0, err0, st0 = m.map(raw, trim=trim)
        raw2 = reads_of(path, himem=False)
        paf, err, st = m.map_aligned(raw2, trim=trim)
        recs = dump(st["trim"].reads(MIN_LENGTH, himem=False))
    assert err == err0 and paf0.count("\n") > 30
    read_codes = {}
    for rec in recs:  # name, bases spelled from their codes, qualities
        f = rec.split("\t")
        read_codes[f[0]] = codes_of(np.frombuffer(f[1].encode(), dtype=np.uint8))
    g, _ = reference()
    ref_name = paf0.split("\t")[5]
    tags, _ = check_against_model(paf, paf0, read_codes, {ref_name: codes_of(g)}, True)
    assert all(t is not None for t in tags) and st["align"]["lines"] == len(tags)
