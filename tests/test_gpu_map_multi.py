"""GPU parity of `map -all_sequences`: the product must print what the model of tests/native/map_multi_model.cpp prints (which
tests/test_map_multi_cpu.py holds against the oracle and against the truth), line for line and with the same stderr text, on every
index layout, upload path and seed walk; and dp_single_seed_candidates_multi must be the single-sequence entry point run over a set
of sequences that share one index.  k = 11 and default flags unless a test says otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import map_multi_cases as MC
from tests import map_multi_model as MM
from tests import oracle_lib as O
from tests.test_gpu_map import first_diff

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROD = os.path.join(ROOT, "downpore_amd", "bin", "downpore")
ORAC = os.path.join(ROOT, "oracle", "_build", "dp_oracle")


def _product(ref, reads, **kw):
    from downpore_amd.mapping import map_reads
    from downpore_amd.overlap import Reads
    return map_reads(Reads(*ref, min_len=0, himem=False), Reads(*reads, min_len=500, himem=False), all_sequences=True, **kw)


@pytest.fixture(scope="module")
def multi():
    """the multi-sequence input and the model's answers, computed once"""
    ref_bases, ref_off, bases, off, _ = MC.multi_case()
    m = dict(ref=(ref_bases, ref_off), reads=(bases, off))
    for circular in (True, False):
        m[circular] = MM.run(ref_bases, ref_off, bases, off, circular=circular)
    return m


def test_one_sequence_with_the_switch_is_the_oracle():
    seed, G, N, L, e, variable, circular = 4, 150000, 300, 6000, 0.05, True, True
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    bases, off = O.gen_reads(seed, G, N, L, e, variable)
    want, werr = O.map_run(O.ReadSet(genome, goff, min_len=0, himem=False), O.ReadSet(bases, off, min_len=500, himem=False), circular=circular)
    got, gerr, _ = _product((genome, goff), (bases, off), circular=circular)
    assert first_diff(got, want) is None and gerr == werr and want.count("\n") > N // 2


@pytest.mark.parametrize("circular", [True, False])
def test_multi_sequence_run_is_the_model(multi, circular):
    want, werr = multi[circular]
    got, gerr, st = _product(multi["ref"], multi["reads"], circular=circular)
    d = first_diff(got, want)
    assert d is None, d
    assert gerr == werr
    rows = MC.parse(got)
    assert len(set(r[5] for r in rows)) >= 4
    by_read = {}
    for r in rows:
        by_read.setdefault(r[0], set()).add(r[5])
    assert any(len(v) > 1 for v in by_read.values())
    assert int(gerr.split("Multiple mappings: ")[1].split("\n")[0]) > 0
    if circular:
        assert "Sequence r0000003 (900 bases) is shorter than query_size" in gerr


def test_sparse_index_and_shards_print_the_dense_paf(multi, monkeypatch):
    """both layouts and the sharded index cut by chunk id and know nothing about sequences; chunk_size = 2 000 makes more than 64
    chunks, so that two shards really hold two ranges (a shard holds whole 64-chunk words)"""
    want, werr = multi[True]
    dense, derr, st = _product(multi["ref"], multi["reads"], index="dense")
    assert st["index"]["layout"] == "dense" and first_diff(dense, want) is None and derr == werr
    sparse, serr, st = _product(multi["ref"], multi["reads"], index="sparse")
    assert st["index"]["layout"] == "sparse" and first_diff(sparse, dense) is None and serr == derr
    monkeypatch.setenv("DP_MAP_SHARDS", "2")
    sharded, herr, _ = _product(multi["ref"], multi["reads"])
    assert first_diff(sharded, dense) is None and herr == derr
    small, smerr = MM.run(*multi["ref"], *multi["reads"], chunk_size=2000)
    sharded, herr, st = _product(multi["ref"], multi["reads"], chunk_size=2000)
    assert st["n_chunks"] > 64 and first_diff(sharded, small) is None and herr == smerr
    monkeypatch.delenv("DP_MAP_SHARDS")
    sparse, serr, st = _product(multi["ref"], multi["reads"], chunk_size=2000, index="sparse")
    assert first_diff(sparse, small) is None and serr == smerr


def test_host_seed_walk_and_the_other_upload_paths_agree(multi, monkeypatch):
    want, werr = multi[True]
    _, _, st = _product(multi["ref"], multi["reads"])
    for tune in ("map_seeds_host=1", "map_ascii_upload=1", "map_async_upload=1"):
        monkeypatch.setenv("DP_TUNE", tune)
        got, gerr, st2 = _product(multi["ref"], multi["reads"])
        assert first_diff(got, want) is None and gerr == werr, tune
        assert st2["n_seeds"] == st["n_seeds"] > 0 and st2["n_chunks"] == st["n_chunks"], tune
    monkeypatch.delenv("DP_TUNE")


def _codes(bases):
    b = np.asarray(bases, dtype=np.uint8)
    return ((b >> 1) ^ ((b & 4) >> 2)) & 3


def _count_region(i, length, seed_rate, k):
    """CountKmersBetween(i, i + seed_rate) of a top-level sequence (seeds.go:160-200, sequence.go:332-337): whole bytes only, the
    sequence's own skipBack = 4 - len % 4, the do-while group loop.  Returns (first base, number of k-mers)."""
    start_b, end_b = (i + 3) // 4, (i + seed_rate) // 4
    nk = 4 * (end_b - start_b - 1) - (4 - length % 4) - k + 1
    groups = max(1, (nk & ~3) // 4)
    return start_b * 4, 4 + 4 * groups + (nk & 3)


def test_the_kernel_directly():
    from downpore_amd.hip import Context
    k, seed_rate = 11, 40
    lens = [40, 41, 79, 80, 81, 163, 164, 4001, 10]
    rng = np.random.default_rng(9)
    seqs = []
    for ln in lens:  # every sequence begins with a run of T's (code 3): a base read past its neighbour's end would show, zero padding not
        s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, ln)].copy()
        s[:min(ln, 24)] = ord("T")
        seqs.append(s)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ctx = Context(0)
    ctx.upload_reads(np.concatenate(seqs), off)
    ctx.kmer_values(k)
    singles = [ctx.single_seed_candidates(r, k, seed_rate) for r in range(len(lens))]
    m = ctx.single_seed_candidates_multi(0, len(lens), k, seed_rate)
    n_win = [(ln - seed_rate + seed_rate - 1) // seed_rate if ln > seed_rate else 0 for ln in lens]
    assert n_win == [0, 1, 1, 1, 2, 4, 4, 100, 0]
    assert m["win_off"].tolist() == np.concatenate([[0], np.cumsum(n_win)]).tolist()
    assert [len(s["best"]) for s in singles] == n_win
    assert np.array_equal(m["best"], np.concatenate([s["best"] for s in singles]))
    # candidates: the k-mers of every window's count region that are the best of ANY window of ANY sequence, bases past the end zero
    any_best = set(int(v) for v in m["best"])
    want, want_off = [], [0]
    for c, ln in enumerate(lens):
        code = np.concatenate([_codes(seqs[c]), np.zeros(seed_rate + k + 8, dtype=np.uint8)])
        for w in range(n_win[c]):
            p0, P = _count_region(w * seed_rate, ln, seed_rate, k)
            for j in range(P):
                km = 0
                for b in code[p0 + j:p0 + j + k]:
                    km = (km << 2) | int(b)
                if km in any_best:
                    want.append(km)
            want_off.append(len(want))
    assert m["cand_off"].tolist() == want_off
    assert m["cand"].tolist() == want
    # one sequence: the old entry point's arrays
    for r in (1, 4, 7):
        one = ctx.single_seed_candidates_multi(r, 1, k, seed_rate)
        old = ctx.single_seed_candidates(r, k, seed_rate)
        assert one["win_off"].tolist() == [0, n_win[r]]
        for f in ("best", "cand_off", "cand"):
            assert np.array_equal(one[f], old[f]), (r, f)
    none = ctx.single_seed_candidates_multi(8, 1, k, seed_rate)
    assert none["win_off"].tolist() == [0, 0] and len(none["best"]) == 0
    ctx.close()


def _two_short_sequences(tmp_path):
    g = np.frombuffer(O.gen_genome(31, 6000), dtype=np.uint8)
    goff = np.array([0, 3000, 6000], dtype=np.int64)
    bases, off = O.gen_reads(31, 6000, 20, 1500, 0.0, False)
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    O.write_fasta(ref_fa, g, goff, prefix="chr")
    O.write_fasta(reads_fa, bases, off)
    return (g, goff), (bases, off), ref_fa, reads_fa


def test_a_reference_without_any_chunk_leaves_every_read_unmapped(tmp_path):
    """two sequences of 3 000 bases (<= chunk_size / 2), not circular: no chunk at all, no device call on an empty index"""
    ref, reads, ref_fa, reads_fa = _two_short_sequences(tmp_path)
    want, werr = MM.run(*ref, *reads, circular=False)
    assert want == "" and werr.endswith("Uniquely mapped: 0\nMultiple mappings: 0\ntotal: 0\nUnmapped: 20\n")
    got, gerr, st = _product(ref, reads, circular=False)
    assert got == "" and gerr == werr and st["n_chunks"] == 0
    a = subprocess.run([PROD, "map", "-input", reads_fa, "-reference", ref_fa, "-circular", "false", "-all_sequences", "true"], capture_output=True)
    assert a.returncode == 0 and a.stdout == b"" and a.stderr.decode() == werr


def test_cli(multi, tmp_path):
    ref_fa, reads_fa = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fa")
    O.write_fasta(ref_fa, *multi["ref"], prefix="chr")
    O.write_fasta(reads_fa, *multi["reads"])
    want, werr = MM.run_files(ref_fa, reads_fa)
    assert "\tchr0000002\t" in want and want.replace("\tchr", "\tr") == multi[True][0]
    a = subprocess.run([PROD, "map", "-input", reads_fa, "-reference", ref_fa, "-all_sequences", "true"], capture_output=True, check=True)
    assert first_diff(a.stdout.decode(), want) is None and a.stderr.decode() == werr
    b = subprocess.run([PROD, "map", "-i", reads_fa, "-r", ref_fa, "-a", "true"], capture_output=True, check=True)
    assert b.stdout == a.stdout
    # without the flag: the first sequence only, as the oracle's CLI
    c = subprocess.run([PROD, "map", "-input", reads_fa, "-reference", ref_fa], capture_output=True, check=True)
    d = subprocess.run([ORAC, "map", "-input", reads_fa, "-reference", ref_fa], capture_output=True, check=True)
    assert first_diff(c.stdout.decode(), d.stdout.decode()) is None and c.stdout.count(b"\n") > 100
    assert set(ln.split(b"\t")[5] for ln in c.stdout.splitlines()) == {b"chr0000000"}


HELP_MAP = """-input  -i  Fasta/fastq input file  (default:)
-reference  -r  A fasta file containing a reference sequence to align against  (default:)
-circular  -ci  Whether the reference genome is circular  (default:true)
-k  -k  Length of seeds in bases  (default:11)
-query_size  -q  The number of bases to query at a time  (default:1000)
-min_length  -m  The minimum sequence size to generate queries from  (default:500)
-chunk_size  -ch  The number of bases for reference index chunks  (default:10000)
-seed_rate  -s  The maximum number of bases between seeds in the reference  (default:40)
-num_workers  -n  The number of worker process to use for mapping  (default:4)
"""


def test_help_map_keeps_its_nine_lines():
    """the lines `help map` printed before the switch existed (names, generated aliases, descriptions, defaults), then the new one"""
    out = subprocess.run([PROD, "help", "map"], capture_output=True, check=True).stdout.decode()
    assert out.startswith(HELP_MAP)
    rest = out[len(HELP_MAP):].splitlines()
    assert len(rest) == 1 and rest[0].startswith("-all_sequences  -a  ") and rest[0].endswith("(default:false)")


def _host():
    from downpore_amd.overlap import load_host
    H = load_host()
    H.dph_map_run_ex.restype = C.c_void_p
    H.dph_map_run_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    H.dph_last_error.restype = C.c_char_p
    return H


@pytest.mark.parametrize("value", [2, -1, 1 << 33])
def test_host_abi_refuses_another_value_of_the_switch(value):
    from downpore_amd.overlap import Reads
    H = _host()
    bases, off = O.gen_reads(3, 20000, 4, 2000, 0.0, False)
    reads = Reads(bases, off, min_len=500)
    p = np.array([1, 11, 1000, 500, 10000, 40, 0, value], dtype=np.int64)
    assert not H.dph_map_run_ex(reads.h, reads.h, p.ctypes.data, 8, 0)
    msg = H.dph_last_error(None).decode()
    assert "all sequences" in msg and str(value) in msg, msg
    assert not H.dph_map_run_ex(reads.h, reads.h, p.ctypes.data, 9, 0)


def test_an_over_long_sequence_is_refused_with_its_name():
    from downpore_amd import DpError
    from downpore_amd.overlap import Reads
    n = (1 << 31) + 64
    bases = np.full(5000 + n, ord("A"), dtype=np.uint8)
    bases[1::7] = ord("C")
    ref = Reads(bases, np.array([0, 5000, 5000 + n], dtype=np.int64), min_len=0, himem=False)
    del bases
    rb, ro = O.gen_reads(3, 20000, 4, 2000, 0.0, False)
    from downpore_amd.mapping import map_reads
    with pytest.raises(DpError) as e:
        map_reads(ref, Reads(rb, ro, min_len=500), all_sequences=True)
    msg = str(e.value)
    assert "r0000001" in msg and str(n) in msg, msg
    assert "device" not in msg.lower() and "hip" not in msg.replace("dph_", "").lower(), msg
