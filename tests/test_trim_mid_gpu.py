"""`trim`'s middle stage on the GPU: the chunk scan and the (front adapter, chunk) search against the model record by record, the
whole command through trim_reads(middle=True) and the CLI under DP_TRIM_MIDDLE=1 across the flag matrix, flush batches, the forced
tiny record buffer and the pairs the kernel hands to the host's Match.  Everything is integers and text: product and model agree
exactly."""
import os
import subprocess

import numpy as np
import pytest

from tests import trim_cases as TC
from tests import trim_mid_cases as MC
from tests import trim_mid_model as MM
from tests import trim_model as M
from tests.test_trim_cpu import CLI, _dir_files, _reads
from tests.test_trim_mid_cpu import GEN, MATRIX

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_mid_gpu")
    out = {}
    for fastq in (False, True):
        names, seqs, quals, truth = MC.generate(fastq=fastq, **GEN)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = dict(path=path, seqs=seqs, truth=truth)
    out["dir"] = d
    return out


def _subset_files(path, k, d):
    """the adapters DetermineAdapters leaves, in its swap-removed order, as files"""
    det = M.determine(path, k=k)
    fn, fs = TC.read_fasta(TC.FRONT)
    bn, bs = TC.read_fasta(TC.BACK)
    F, B = dict(zip(fn, fs)), dict(zip(bn, bs))
    fp, bp = str(d / ("front_k%d.fasta" % k)), str(d / ("back_k%d.fasta" % k))
    TC.write_fasta(fp, [n for s, n, _ in det.adapters if s == "F"], [F[n] for s, n, _ in det.adapters if s == "F"])
    TC.write_fasta(bp, [n for s, n, _ in det.adapters if s == "B"], [B[n] for s, n, _ in det.adapters if s == "B"])
    return fp, bp


def _kernel_case(sets, k, chunk_size, subset):
    """-> model run, device handle with the model's chunks scanned, seed counts"""
    from downpore_amd import trim as T
    names, seqs, _, _ = MC.generate(seed=11, n_reads=60, chunk_size=chunk_size)
    path = str(sets["dir"] / ("kernel_%d_%d.fasta" % (k, chunk_size)))
    TC.write_fasta(path, names, seqs)
    fp, bp = _subset_files(path, k, sets["dir"]) if subset else (TC.FRONT, TC.BACK)
    m = MM.run(path, fp, bp, k=k, chunk_size=chunk_size, determine_adapters=False)
    e = M.run(path, fp, bp, k=k, determine_adapters=False)
    chunks = [seqs[r][e.table[r, 0]:len(seqs[r]) - e.table[r, 1]][s:en] for r, s, en, _, _, _ in m.plan]
    dev = T.TrimDevice(T.trim_index(_reads(fp, 0), _reads(bp, 0), k))
    counts, _ = dev.scan_chunks(chunks)
    return m, dev, counts


CONFIGS = [(5, 5000, False), (6, 5000, False), (7, 5000, False), (8, 5000, False), (6, 5000, True), (8, 5000, True), (6, 1000, True), (6, 20000, True)]


@pytest.mark.parametrize("k,chunk_size,subset", CONFIGS, ids=["k%d-cs%d-%s" % (k, c, "subset" if s else "all") for k, c, s in CONFIGS])
def test_scan_and_search_equal_the_model(sets, k, chunk_size, subset):
    m, dev, counts = _kernel_case(sets, k, chunk_size, subset)
    assert np.array_equal(counts.astype(np.int64), m.plan[:, 4].astype(np.int64))
    for c in range(len(m.plan)):
        assert np.array_equal(dev.chunk_segments(c), m.chunk_segments(c)), c
    s = dev.search(np.nonzero(m.plan[:, 5])[0])
    dev.close()
    assert s["pairs"] == m.counters["candidate_pairs"]
    # the pairs the kernel lists for the host's Match carry no device records; every other record equals the model's, in its order
    over = set(map(tuple, s["overflow"].tolist()))
    keep = np.array([(int(c), int(a)) not in over for a, c in zip(m.recs[:, 0], m.recs[:, 1])], dtype=bool)
    assert len(m.recs) > 0 and keep.any()
    assert np.array_equal(s["recs"], m.recs[keep])
    if subset and k in (6, 8):  # a configuration in which Matches really filters
        share = m.counters["candidate_pairs"] / (m.counters["indexed_chunks"] * m.counters["front_adapters"])
        assert 0 < share < 1, share


def _assert_equal(res, m):
    assert res.output == m.output
    assert res.stderr == m.stderr
    assert np.array_equal(res.table, m.table)
    assert np.array_equal(res.splits, m.splits)
    assert res.extras == m.extras
    assert np.array_equal(res.plan, m.plan)
    assert np.array_equal(res.applied, m.recs)
    assert res.adapters == m.adapters
    assert res.stats["mid_pairs"] == m.counters["candidate_pairs"]


def _strip_stamps(text):
    out = []
    for ln in text.splitlines():
        assert ln[4] == "/" and ln[7] == "/" and ln[10] == " " and ln[13] == ":" and ln[19] == " ", ln
        out.append(ln[20:])
    return "\n".join(out) + "\n"


def _cli_flags(flags):
    out = []
    for key, v in flags.items():
        out += ["-" + key, ("true" if v else "false") if isinstance(v, bool) else str(v)]
    return out


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
@pytest.mark.parametrize("flags", MATRIX, ids=["-".join("%s=%s" % kv for kv in f.items()) or "defaults" for f in MATRIX])
def test_trim_reads_and_the_cli_equal_the_model(sets, fmt, flags, tmp_path):
    from downpore_amd import trim as T
    s = sets[fmt]
    m = MM.run(s["path"], k=6, **flags)
    R, F, B = _reads(s["path"]), _reads(TC.FRONT, 0), _reads(TC.BACK, 0)
    res = T.trim_reads(R, F, B, k=6, middle=True, **flags)
    _assert_equal(res, m)
    assert res.stats["mid_kernel_ms"] > 0 and res.stats["mid_scan_ms"] > 0
    env = dict(os.environ, DP_TRIM_MIDDLE="1")
    r = subprocess.run([CLI, "trim", "-input", s["path"], "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK, "-num_workers", "7", "-himem", "true"]
                       + _cli_flags(flags), capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == m.output
    assert "not part of this build" not in r.stderr
    assert _strip_stamps(r.stderr) == m.stderr
    if flags in (dict(), dict(discard_middle=True), dict(tag_adapters=False)):
        a, b, c = tmp_path / "product", tmp_path / "model", tmp_path / "cli"
        for p in (a, b, c):
            p.mkdir()
        assert res.demultiplex(a) == m.demultiplex(b)
        assert _dir_files(a) == _dir_files(b)
        r = subprocess.run([CLI, "trim", "-input", s["path"], "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK, "-demultiplex", str(c)]
                           + _cli_flags(flags), capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout == ""
        assert _dir_files(c) == _dir_files(b)


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_three_and_more_flush_batches_equal_the_model(sets, fmt):
    from downpore_amd import trim as T
    s = sets[fmt]
    m = MM.run(s["path"], k=6, flush_seeds=2000)
    assert m.counters["batches"] >= 3
    res = T.trim_reads(_reads(s["path"]), _reads(TC.FRONT, 0), _reads(TC.BACK, 0), k=6, middle=True, flush_seeds=2000)
    _assert_equal(res, m)
    assert res.stats["mid_batches"] == m.counters["batches"]
    assert all(c == 0 for _, _, c in res.adapters)


def test_a_forced_tiny_record_buffer_gives_the_same_bytes_after_its_repeat(sets, monkeypatch):
    from downpore_amd import trim as T
    m, dev, _ = _kernel_case(sets, 6, 5000, True)
    sel = np.nonzero(m.plan[:, 5])[0]
    plain = dev.search(sel)
    monkeypatch.setenv("DP_TRIM_MID_REC_CAP", "2")
    tiny = dev.search(sel)
    dev.close()
    assert plain["launches"] == 1 and tiny["launches"] == 2 and len(plain["recs"]) > 2
    assert np.array_equal(plain["recs"], tiny["recs"]) and np.array_equal(plain["overflow"], tiny["overflow"])
    s = sets["fasta"]
    mm = MM.run(s["path"], k=6)
    res = T.trim_reads(_reads(s["path"]), _reads(TC.FRONT, 0), _reads(TC.BACK, 0), k=6, middle=True)
    _assert_equal(res, mm)


def test_the_pairs_beyond_the_kernels_working_set_are_counted_and_matched_on_the_host(sets):
    """at k = 5 the (GA)n centres keep thousands of reduced seeds against the adapter that holds GAGAGA"""
    from downpore_amd import trim as T
    s = sets["fasta"]
    m = MM.run(s["path"], k=5, determine_adapters=False)
    res = T.trim_reads(_reads(s["path"]), _reads(TC.FRONT, 0), _reads(TC.BACK, 0), k=5, middle=True, determine_adapters=False)
    assert res.stats["mid_overflow_pairs"] > 0
    _assert_equal(res, m)


def test_the_cli_without_the_switch_still_prints_its_notice_once(sets):
    env = {k: v for k, v in os.environ.items() if k != "DP_TRIM_MIDDLE"}
    s = sets["fasta"]
    r = subprocess.run([CLI, "trim", "-input", s["path"], "-front_adapters", TC.FRONT, "-back_adapters", TC.BACK], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0
    assert r.stderr.count("not part of this build") == 1
    assert "_(left)" not in r.stdout and r.stdout == M.run(s["path"]).output
