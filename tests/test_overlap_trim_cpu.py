"""`overlap -trim true` without a GPU: the rule that turns a finished trim run into the read set `overlap` works on
(TrimResult.reads over dph_trim_reads) against the model's written output read back from a file, the generator of overlapping reads
with adapters the GPU tests share, and the command line.  Everything is integers and text: equal means equal."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import trim_cases as TC
from tests import trim_mid_model as MM
from tests.test_trim_cpu import CLI

# the overlap flags of the GPU test (tests/test_overlap_trim_gpu.py); everything else is the command's default
OVERLAP = dict(k=10, overlap_size=1000)
GEN = dict(seed=23, genome=100_000, n_reads=330)
KINDS = ["plain", "front", "back", "split", "both", "front_crop", "plain", "tail_crop", "split5", "short", "tiny_both", "ignored_crop"]


def generate(seed, genome, n_reads, fastq=False):
    """Reads of 3 000 - 5 000 bases drawn from ONE random genome (they overlap one another: ~13x coverage), a few below 1 000, with
    the fixture adapters planted at their ends and in their centres the way trim_mid_cases.generate plants them.
    -> names, seqs, quals (or None), kinds"""
    rng = np.random.default_rng(seed)
    bases, off = O.gen_reads(seed, genome, n_reads, 5000, 0.0, False)
    fn, fs = TC.read_fasta(TC.FRONT)
    bn, bs = TC.read_fasta(TC.BACK)
    F, B = dict(zip(fn, fs)), dict(zip(bn, bs))
    both = [n for n in fn if n in bn]
    plain = [n for n in both if not n.startswith("Barcode")][:2]
    bars = [n for n in both if n.startswith("Barcode")][:4]
    names, seqs, kinds = [], [], []
    for i in range(n_reads):
        kind = KINDS[i % len(KINDS)]
        full = bases[off[i]:off[i + 1]].tobytes().decode()
        length = int(rng.integers(3000, 5001))
        if kind == "short":
            length = int(rng.integers(400, 1000))
        if kind == "tiny_both":
            length = int(rng.integers(200, 261))
        if kind == "ignored_crop":  # a front crop by the middle stage that leaves less than 500 bases
            length = int(rng.integers(700, 900))
        read = full[:length]
        name = plain[i % 2] if i % 3 else bars[i % 4]
        mid = length // 2
        if kind in ("front", "both"):
            read = TC.plant(read, int(rng.integers(0, 60)), TC.mutate(rng, F[name], 0.05 if kind == "both" else 0.0))
        if kind in ("back", "both"):
            read = TC.plant(read, length - TC.EDGE + int(rng.integers(60, 110)), TC.mutate(rng, B[name], 0.05 if kind == "both" else 0.0))
        if kind == "split":
            read = TC.plant(read, mid, F[name])
            if i % 2:  # a split read that lost an end adapter first: the halves' spans start behind a front trim
                read = TC.plant(read, int(rng.integers(0, 40)), F[plain[0]])
        if kind == "split5":
            read = TC.plant(read, mid, TC.mutate(rng, F[name], 0.05))
        if kind == "front_crop":
            read = TC.plant(read, int(rng.integers(200, 420)), F[name])
        if kind == "tail_crop":
            read = TC.plant(read, length - int(rng.integers(330, 520)), F[name])
        if kind == "tiny_both":
            read = TC.plant(read, 95, F[plain[0]])
            read = TC.plant(read, length - TC.EDGE + 15, B[plain[0]])
        if kind == "ignored_crop":
            read = TC.plant(read, int(rng.integers(330, 420)), F[name])
        names.append("read%05d_%s" % (i, kind))
        seqs.append(read[:length])
        kinds.append(kind)
    quals = None
    if fastq:
        quals = ["".join(chr(33 + int(q)) for q in rng.integers(2, 41, size=len(s))) for s in seqs]
    return names, seqs, quals, kinds


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("overlap_trim")
    out = {"dir": d}
    for fastq in (False, True):
        names, seqs, quals, kinds = generate(fastq=fastq, **GEN)
        path = str(d / ("reads.fastq" if fastq else "reads.fasta"))
        TC.write_fasta(path, names, seqs, quals)
        out["fastq" if fastq else "fasta"] = dict(path=path, names=names, seqs=seqs, kinds=kinds)
    return out


def reads_of(path, min_len=50, himem=True):
    from downpore_amd.overlap import Reads
    return Reads(fasta=str(path), min_len=min_len, himem=himem)


def dump(reads):
    """dph_reads_dump: name, bases spelled from their codes and the stored quality bytes of every record"""
    from downpore_amd.overlap import load_host
    fn = load_host().dph_reads_dump
    fn.restype = C.POINTER(C.c_char)
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    n = C.c_int64(0)
    return C.string_at(fn(reads.h, C.byref(n)), n.value).decode().splitlines()


def written(d, m, fastq, tag):
    """the model's output as the file the two-command pipeline passes on"""
    path = str(d / ("trimmed_%s.%s" % (tag, "fastq" if fastq else "fasta")))
    with open(path, "w") as f:
        f.write(m.output)
    return path


FLAGS = [dict(), dict(tag_adapters=False), dict(discard_middle=True), dict(tag_adapters=False, discard_middle=True)]


@pytest.mark.parametrize("flags", FLAGS, ids=["-".join("%s=%s" % kv for kv in f.items()) or "defaults" for f in FLAGS])
@pytest.mark.parametrize("min_len", [50, 1000])
@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_the_trimmed_read_set_equals_the_models_output_read_back(sets, fmt, min_len, flags):
    from downpore_amd import trim as T
    s = sets[fmt]
    m = MM.run(s["path"], k=6, **flags)
    assert not m.error and not m.failed
    R, F, B = reads_of(s["path"]), reads_of(TC.FRONT, 0), reads_of(TC.BACK, 0)
    res = T.trim_apply_middle(R, F, B, m.edge_recs, m.edge_counts, m.plan[:, 4], m.recs, enabled=m.enabled, k=6, **flags)
    assert res.output == m.output
    got = dump(res.reads(min_len))
    want = dump(reads_of(written(sets["dir"], m, fmt == "fastq", "%d_%d" % (min_len, FLAGS.index(flags))), min_len))
    assert len(want) > 100
    assert got == want
    if fmt == "fastq":
        assert all(ln.count("\t") == 2 for ln in got)  # every record kept its quality bytes


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_the_input_is_not_vacuous(sets, fmt):
    s = sets[fmt]
    m = MM.run(s["path"], k=6)
    t = m.table
    assert len(t) == len(s["names"]) == GEN["n_reads"]
    assert ((t[:, 0] > 0) | (t[:, 1] > 0)).sum() * 3 >= len(t)
    assert (m.splits[:, 3] == 3).sum() >= 3  # both halves kept
    split = set(m.splits[:, 0].tolist())
    assert any(t[r, 2] == 1 and r not in split for r in range(len(t)))  # ignored, and not because it was split
    assert any(t[r, 0] > 0 for r in split)  # a split read behind a front trim
    assert sum(1 for q in s["seqs"] if len(q) < 1000) >= 3
    path = written(sets["dir"], m, fmt == "fastq", "oracle")
    want = O.OverlapRun(O.ReadSet(fasta=path, min_len=OVERLAP["overlap_size"]), **OVERLAP)
    lines = want.paf.splitlines()
    assert len(lines) > 0
    assert any("_(left)" in ln or "_(right)" in ln for ln in lines)


HELP_OVERLAP = """-overlap_size  -o  Size of overlap to search for in bases  (default:1000)
-k  -k  Number of bases in each seed  (default:10)
-num_seeds    Minimum number of seeds to generate for each overlap query  (default:15)
-seed_batch_size    Maximum total unique seeds to use in each query batch  (default:10000)
-chunk_size  -c  Size to chop long reads into for querying against, in bases  (default:10000)
-query_batch_size  -q  Maximum number of queries per batch (if max seeds not reached)  (default:20000)
-min_hits  -m  Minimum proportion of seeds that must match each query  (default:0.25)
-num_workers    Number of worker threads to spawn  (default:4)
-input  -i  Fasta/fastq input file  (default:)
-seed_values    File containing values to use during seed selection.  (default:)
-himem  -h  Whether to cache all reads in memory  (default:true)
"""


def test_help_overlap_keeps_its_eleven_lines_and_lists_the_three_new_flags():
    out = subprocess.run([CLI, "help", "overlap"], capture_output=True, check=True).stdout.decode()
    assert out.startswith(HELP_OVERLAP)
    rest = out[len(HELP_OVERLAP):].splitlines()
    assert len(rest) == 3
    assert rest[0].startswith("-trim  -t  ") and rest[0].endswith("(default:false)")
    assert rest[1].startswith("-front_adapters  -f  ") and rest[1].endswith("(default:)")
    assert rest[2].startswith("-back_adapters  -b  ") and rest[2].endswith("(default:)")


def test_help_map_and_help_trim_do_not_list_the_switch():
    for cmd in ("map", "trim"):
        out = subprocess.run([CLI, "help", cmd], capture_output=True, check=True).stdout.decode()
        assert "-trim " not in out


def test_trim_without_its_adapter_lists_is_an_error_that_names_the_flag(sets):
    r = subprocess.run([CLI, "overlap", "-input", sets["fasta"]["path"], "-trim", "true", "-back_adapters", TC.BACK], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    assert "-front_adapters" in r.stderr
    r = subprocess.run([CLI, "overlap", "-input", sets["fasta"]["path"], "-trim", "true", "-front_adapters", TC.FRONT], capture_output=True, text=True)
    assert r.returncode == 1 and "-back_adapters" in r.stderr
