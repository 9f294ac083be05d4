"""`trim`, edge stage, on the GPU: dp_trim_edges against the model end by end, determine mode, the whole command through
trim_reads and the CLI across the flag matrix, capacity and error paths.  Everything is integers and text: product and model
agree exactly."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import trim_cases as TC
from tests import trim_model as M
from tests.test_trim_cpu import (CLI, E2E_SET, FLAG_MATRIX, HAND, KERNEL_SET, RECORDED, _dir_files, _reads, _write_adapters,
                                 hand_edge_files)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def adapters():
    return _reads(TC.FRONT, 0), _reads(TC.BACK, 0)


@pytest.fixture(scope="module")
def kernel_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_gpu_kernel_set")
    names, seqs, _, _ = TC.generate(**KERNEL_SET)
    path = str(d / "reads.fasta")
    TC.write_fasta(path, names, seqs)
    ends, ids = TC.ends_of(seqs)
    assert len(ends) * 2 >= 20000
    return dict(path=path, seqs=seqs, ends=ends, ids=ids, dir=d)


@pytest.fixture(scope="module")
def e2e_set(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_gpu_e2e_set")
    out = {}
    for fastq in (False, True):
        names, seqs, quals, _ = TC.generate(fastq=fastq, **E2E_SET)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = dict(path=path, seqs=seqs)
    return out


def _compare_records(got, counts, m):
    bad = np.nonzero((got != m.recs).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d ends differ; first: end %d kernel %s model %s" % (len(bad), len(got), bad[0], got[bad[0]], m.recs[bad[0]])
    assert np.array_equal(counts, m.counts)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_edges_equal_the_model_end_by_end_with_all_adapters(kernel_set, adapters, k):
    from downpore_amd import trim as T
    m = M.run(kernel_set["path"], determine_adapters=False, k=k)
    d = T.TrimDevice(T.trim_index(adapters[0], adapters[1], k))
    recs, counts, _ = d.edges(kernel_set["ends"])
    d.close()
    _compare_records(recs, counts, m)


@pytest.mark.parametrize("k", [5, 6, 7, 8])
def test_edges_equal_the_model_with_a_determined_subset(kernel_set, k):
    """The adapters DetermineAdapters leaves (in its swap-removed order) as the index."""
    from downpore_amd import trim as T
    det = M.determine(kernel_set["path"], k=k)
    n_front = sum(1 for s, _, _ in det.adapters if s == "F")
    fn, fs = TC.read_fasta(TC.FRONT)
    bn, bs = TC.read_fasta(TC.BACK)
    d = kernel_set["dir"]
    fp = _write_adapters(d / ("front_k%d.fasta" % k), [dict(name=n, seq=fs[fn.index(n)]) for s, n, _ in det.adapters if s == "F"])
    bp = _write_adapters(d / ("back_k%d.fasta" % k), [dict(name=n, seq=bs[bn.index(n)]) for s, n, _ in det.adapters if s == "B"])
    assert 0 < n_front < 116
    m = M.run(kernel_set["path"], fp, bp, determine_adapters=False, k=k)
    dev = T.TrimDevice(T.trim_index(_reads(fp, 0), _reads(bp, 0), k))
    recs, counts, _ = dev.edges(kernel_set["ends"])
    dev.close()
    _compare_records(recs, counts, m)


def test_two_batches_through_one_setup_equal_one_batch(kernel_set, adapters):
    from downpore_amd import trim as T
    ix = T.trim_index(adapters[0], adapters[1], 6)
    e = kernel_set["ends"][:3000]
    d = T.TrimDevice(ix)
    whole, counts_whole, _ = d.edges(e)
    d.close()
    d = T.TrimDevice(ix)
    a, counts_a, _ = d.edges(e[:1100])
    b, counts_ab, _ = d.edges(e[1100:])
    d.close()
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(counts_ab, counts_whole) and counts_a.sum() < counts_ab.sum()


@pytest.mark.parametrize("check_reads", [400, 1500, 5000])
def test_determine_flags_and_compacted_order_equal_the_model(e2e_set, adapters, check_reads):
    """check_reads below, at and above the read count."""
    from downpore_amd import trim as T
    s = e2e_set["fasta"]
    assert len(s["seqs"]) == 1500
    m = M.determine(s["path"], check_reads=check_reads)
    ends, _ = TC.ends_of(s["seqs"][:check_reads])
    d = T.TrimDevice(T.trim_index(adapters[0], adapters[1], 6))
    half = len(ends) // 2
    d.edges(ends[:half], mode=T.MODE_DETERMINE, threshold=90)
    enabled, _ = d.edges(ends[half:], mode=T.MODE_DETERMINE, threshold=90)
    d.close()
    assert np.array_equal(enabled, m.enabled) and 0 < enabled.sum() < len(enabled)
    res = T.trim_reads(_reads(s["path"]), adapters[0], adapters[1], check_reads=check_reads)
    assert [(a, n) for a, n, _ in res.adapters] == [(a, n) for a, n, _ in m.adapters]


def _cli_flags(flags):
    out = []
    for key, v in flags.items():
        out += ["-" + key, str(v).lower() if isinstance(v, bool) else str(v)]
    return out


def _strip_stamps(text):
    """The CLI's log lines without Go's `2006/01/02 15:04:05 ` prefix; its own one-off notice is dropped."""
    out = []
    for ln in text.splitlines():
        if ln.startswith("downpore trim:"):
            continue
        assert ln[4] == "/" and ln[7] == "/" and ln[10] == " " and ln[13] == ":" and ln[19] == " ", ln
        out.append(ln[20:])
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("flags", FLAG_MATRIX, ids=["-".join("%s=%s" % kv for kv in f.items()) or "defaults" for f in FLAG_MATRIX])
def test_trim_reads_and_the_cli_give_the_models_output(e2e_set, adapters, fmt, flags, tmp_path):
    from downpore_amd import trim as T
    s = e2e_set[fmt]
    m = M.run(s["path"], **flags)
    res = T.trim_reads(_reads(s["path"]), adapters[0], adapters[1], **flags)
    assert res.output == m.output
    assert res.stderr == m.stderr
    assert np.array_equal(res.table, m.table)
    assert res.adapters == m.adapters
    assert res.stats["kernel_ms"] > 0
    r = subprocess.run([CLI, "trim", "-input", s["path"], "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK, "-num_workers", "7",
                        "-himem", "true", "-discard_middle", "true", "-middle_threshold", "70", "-chunk_size", "3000",
                        "-extra_middle_trim", "50"] + _cli_flags(flags), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == m.output
    assert r.stderr.count("the search for adapters in the middle of reads is not part of this build") == 1
    assert _strip_stamps(r.stderr) == m.stderr
    if flags in (dict(), dict(require_pairs=True)):
        a, b, c = tmp_path / "product", tmp_path / "model", tmp_path / "cli"
        for p in (a, b, c):
            p.mkdir()
        assert res.demultiplex(a) == m.demultiplex(b) > 0
        assert _dir_files(a) == _dir_files(b)
        r = subprocess.run([CLI, "trim", "-input", s["path"], "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK, "-demultiplex", str(c)]
                           + _cli_flags(flags), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout == ""
        assert _dir_files(c) == _dir_files(b)


def test_recorded_model_result_without_the_live_model(adapters, tmp_path):
    from downpore_amd import trim as T
    rec = json.load(open(RECORDED))
    names, seqs, _, _ = TC.generate(rec["seed"], rec["n_reads"])
    path = str(tmp_path / "r.fasta")
    TC.write_fasta(path, names, seqs)
    res = T.trim_reads(_reads(path), adapters[0], adapters[1], **rec["flags"])
    assert res.table.tolist() == rec["table"]
    assert [list(a) for a in res.adapters] == rec["adapters"]
    assert hashlib.sha256(res.output.encode()).hexdigest() == rec["output_sha256"]
    assert hashlib.sha256(res.stderr.encode()).hexdigest() == rec["stderr_sha256"]


@pytest.mark.parametrize("path", [p for p in HAND if json.load(open(p))["kind"] == "edge"],
                         ids=[os.path.basename(p)[:-5] for p in HAND if json.load(open(p))["kind"] == "edge"])
def test_hand_edge_case_on_the_kernel(path, tmp_path):
    from downpore_amd import trim as T
    case = json.load(open(path))
    reads, front, back = hand_edge_files(case, tmp_path)
    _, seqs = TC.read_fasta(reads)
    ends, _ = TC.ends_of(seqs)
    d = T.TrimDevice(T.trim_index(_reads(front, 0), _reads(back, 0), case["k"]))
    recs, _, _ = d.edges(ends)
    d.close()
    assert dict(zip(M.REC_FIELDS, (int(v) for v in recs[0 if case["side"] == "front" else 1]))) == case["expect"]


# ---- capacity and error paths -----------------------------------------------------------------------------------------------
def _long_adapter_files(tmp_path, length):
    long_adapter = TC.random_bases(77, length)
    reads = []
    for i, off in enumerate((0, 20, 40)):
        filler = TC.random_bases(100 + i, 2000)
        reads.append(TC.plant(filler, off, long_adapter[-120:]) if i < 2 else TC.plant(filler, 2000 - 150 + 10, long_adapter[:130]))
    rp = str(tmp_path / "reads.fasta")
    TC.write_fasta(rp, ["r%d" % i for i in range(len(reads))], reads)
    fp = _write_adapters(tmp_path / "front.fasta", [dict(name="Long", seq=long_adapter), dict(name="Barcode-1", seq=TC.random_bases(5, 24))])
    bp = _write_adapters(tmp_path / "back.fasta", [dict(name="Long", seq=long_adapter)])
    return rp, fp, bp, reads


def test_a_256_base_adapter_matches_the_model(tmp_path):
    from downpore_amd import trim as T
    rp, fp, bp, reads = _long_adapter_files(tmp_path, 256)
    m = M.run(rp, fp, bp, determine_adapters=False)
    assert m.recs[:, 2].sum() >= 3  # the long adapter is found at both kinds of end
    res = T.trim_reads(_reads(rp), _reads(fp, 0), _reads(bp, 0), determine_adapters=False)
    assert res.output == m.output and res.stderr == m.stderr and np.array_equal(res.table, m.table)
    d = T.TrimDevice(T.trim_index(_reads(fp, 0), _reads(bp, 0), 6))
    recs, counts, _ = d.edges(TC.ends_of(reads)[0])
    d.close()
    _compare_records(recs, counts, m)


def test_an_adapter_beyond_the_documented_limit_is_a_clean_error(tmp_path):
    from downpore_amd import DpError
    from downpore_amd import trim as T
    rp, fp, bp, _ = _long_adapter_files(tmp_path, 600)
    with pytest.raises(DpError, match="the longest adapter this build matches has 512"):
        T.trim_reads(_reads(rp), _reads(fp, 0), _reads(bp, 0), determine_adapters=False)


def test_k_9_is_refused(e2e_set, adapters):
    from downpore_amd import DpError
    from downpore_amd import trim as T
    with pytest.raises(DpError, match="outside 3..8"):
        T.trim_reads(_reads(e2e_set["fasta"]["path"]), adapters[0], adapters[1], k=9)
    ix = T.trim_index(adapters[0], adapters[1], 8)
    ix["k"] = 9
    ix["kmer_seed"] = np.full(4 ** 9, 0xffff, dtype=np.uint16)
    with pytest.raises(DpError, match="outside 3..8"):
        T.TrimDevice(ix)


def test_no_read_of_200_bases_ends_with_the_documented_error(adapters, tmp_path):
    from downpore_amd import DpError
    from downpore_amd import trim as T
    path = str(tmp_path / "short.fasta")
    TC.write_fasta(path, ["a", "b", "c"], [TC.random_bases(1, 199), TC.random_bases(2, 60), TC.random_bases(3, 150)])
    with pytest.raises(DpError, match="no reads long enough to trim"):
        T.trim_reads(_reads(path), adapters[0], adapters[1])
    r = subprocess.run([CLI, "trim", "-input", path, "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "no reads long enough to trim" in r.stderr and r.stdout == ""
