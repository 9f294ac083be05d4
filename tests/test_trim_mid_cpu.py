"""`trim`'s middle stage without a GPU: the hand-worked cases on the model (tests/native/trim_mid_model.cpp) and on the product's
device-free entry (dph_trim_apply_mid), the deliberate mutations of the model, the generated classes, the flag matrix, the chunk plan,
the flush batches and the unchanged eight-parameter behaviour."""
import glob
import json
import os

import numpy as np
import pytest

from tests import trim_cases as TC
from tests import trim_mid_cases as MC
from tests import trim_mid_model as MM
from tests import trim_model as M

HAND = sorted(glob.glob(os.path.join(TC.GOLDEN, "hand_mid", "*.json")))
IDS = [os.path.basename(p)[:-5] for p in HAND]
EDGE_KEYS = ("k", "extra_end_trim", "tag_adapters", "require_pairs", "verbosity")
MID_KEYS = ("chunk_size", "middle_threshold", "extra_middle_trim", "discard_middle", "flush_seeds")


def _reads(path, min_len=50):
    from downpore_amd.overlap import Reads
    return Reads(fasta=str(path), min_len=min_len, himem=False)


def _hand_files(case, tmp):
    names = [r["name"] for r in case["reads"]]
    seqs = [("ACGGTCATTG" * (r["len"] // 10 + 1))[:r["len"]] for r in case["reads"]]
    reads = str(tmp / "reads.fasta")
    TC.write_fasta(reads, names, seqs)
    paths = []
    for side in ("front", "back"):
        p = str(tmp / (side + ".fasta"))
        TC.write_fasta(p, [a["name"] for a in case[side]], [a["seq"] for a in case[side]])
        paths.append(p)
    return reads, paths[0], paths[1]


def _run_hand_model(case, tmp, mid_mutation=0):
    reads, front, back = _hand_files(case, tmp)
    p = case["params"]
    return MM.run(reads, front, back, edge=(case["recs"], case["counts"], None), seed_counts=case["seed_counts"],
                  mid_recs=np.array(case["mid_recs"], dtype=np.int32).reshape(-1, 6), mid_mutation=mid_mutation, **p)


def _check_hand(case, res):
    exp = case["expect"]
    assert res.plan[:, :4].tolist() == exp["plan"]
    assert res.table.tolist() == exp["table"]
    assert res.splits.tolist() == exp["splits"]
    assert res.extras == exp["extras"]
    lines = res.output.splitlines()
    halves = {"left": [], "right": []}
    for i, ln in enumerate(lines):
        if ln.startswith(">") and ln.endswith("_(left)"):
            halves["left"].append(len(lines[i + 1]))
        if ln.startswith(">") and ln.endswith("_(right)"):
            halves["right"].append(len(lines[i + 1]))
    assert halves["left"] == exp.get("left_len", [])
    assert halves["right"] == exp.get("right_len", [])
    if "names" in exp:
        kept = [n for n, row in zip(exp["names"], exp["table"]) if not row[2]]
        assert [ln[1:] for ln in lines if ln.startswith(">")][:len(kept)] == kept
    for text in exp.get("stderr_contains", []):
        assert text in res.stderr, (text, res.stderr)


@pytest.mark.parametrize("path", HAND, ids=IDS)
def test_hand_case_on_the_model(path, tmp_path):
    case = json.load(open(path))
    assert len(case["derivation"]) > 80
    res = _run_hand_model(case, tmp_path)
    assert not res.error
    _check_hand(case, res)
    assert res.recs.tolist() == case["mid_recs"]


@pytest.mark.parametrize("path", HAND, ids=IDS)
def test_hand_case_on_the_product_host_entry(path, tmp_path):
    from downpore_amd import trim as T
    case = json.load(open(path))
    reads, front, back = _hand_files(case, tmp_path)
    R, F, B = _reads(reads), _reads(front, 0), _reads(back, 0)
    res = T.trim_apply_middle(R, F, B, case["recs"], case["counts"], case["seed_counts"], np.array(case["mid_recs"], dtype=np.int32).reshape(-1, 6),
                              **case["params"])
    _check_hand(case, res)
    model = _run_hand_model(case, tmp_path)
    assert res.output == model.output and res.stderr == model.stderr
    assert res.applied.tolist() == model.recs.tolist()


def test_there_are_at_least_eight_hand_cases():
    assert len(HAND) >= 8


@pytest.mark.parametrize("mutation,name", [(1, "04_split_at_exactly_500"), (2, "02_plain_split_with_front_trim")])
def test_a_mutated_model_fails_a_hand_case(mutation, name, tmp_path):
    """1: `<` of trim.go:543 as `<=`; 2: the `- frontTrim` of :579 dropped"""
    case = json.load(open(HAND[IDS.index(name)]))
    _check_hand(case, _run_hand_model(case, tmp_path))
    with pytest.raises(AssertionError):
        _check_hand(case, _run_hand_model(case, tmp_path, mid_mutation=mutation))


# ---- generated inputs ---------------------------------------------------------------------------------------------------------
GEN = dict(seed=3, n_reads=90)


@pytest.fixture(scope="module", params=[False, True], ids=["fasta", "fastq"])
def gen_set(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("trim_mid")
    names, seqs, quals, truth = MC.generate(fastq=request.param, **GEN)
    path = str(d / ("reads.fastq" if request.param else "reads.fasta"))
    TC.write_fasta(path, names, seqs, quals)
    return path, names, seqs, truth


def test_every_class_is_populated_on_the_model(gen_set):
    path, names, seqs, truth = gen_set
    m = MM.run(path, k=6)
    e = M.run(path, k=6)
    cls = MC.model_classes(m, e.table, truth)
    assert set(cls) == set(MC.CLASSES)
    empty = [c for c in MC.CLASSES if cls[c] == 0]
    assert not empty, cls
    assert len(m.table) == len(names)


def test_matches_filters_some_but_not_all_chunks_for_the_determined_subset(gen_set):
    """Matches(ad, 0.2) at k = 6 with the determined adapters: the candidate share lies strictly between 0 and 1"""
    path = gen_set[0]
    m = MM.run(path, k=6)
    share = m.counters["candidate_pairs"] / (m.counters["indexed_chunks"] * m.counters["front_adapters"])
    assert 0 < share < 1, share


def _product_from_model(path, m, **kw):
    from downpore_amd import trim as T
    R, F, B = _reads(path), _reads(TC.FRONT, 0), _reads(TC.BACK, 0)
    rng = np.random.default_rng(5)
    recs = m.recs[rng.permutation(len(m.recs))] if len(m.recs) else m.recs  # (the entry sorts them into canonical order itself)
    enabled = m.enabled if kw.pop("determine_adapters", True) else None
    return T.trim_apply_middle(R, F, B, m.edge_recs, m.edge_counts, m.plan[:, 4], recs, enabled=enabled, **kw), (R, F, B)


def _assert_equal(res, m):
    assert res.output == m.output
    assert res.stderr == m.stderr
    assert np.array_equal(res.table, m.table)
    assert np.array_equal(res.splits, m.splits)
    assert res.extras == m.extras
    assert np.array_equal(res.plan, m.plan)
    assert np.array_equal(res.applied, m.recs)
    assert [(s, n, c) for s, n, c in res.adapters] == m.adapters
    assert res.stats["mid_out_of_range"] == m.counters["out_of_range"]
    assert res.stats["mid_batches"] == m.counters["batches"]


MATRIX = [dict(), dict(discard_middle=True), dict(tag_adapters=False), dict(extra_middle_trim=0), dict(extra_middle_trim=50),
          dict(middle_threshold=70), dict(chunk_size=1000), dict(chunk_size=3000), dict(chunk_size=20000), dict(verbosity=0), dict(verbosity=2),
          dict(require_pairs=True), dict(determine_adapters=False), dict(chunk_size=1000, verbosity=2, extra_middle_trim=0, middle_threshold=70)]


@pytest.mark.parametrize("flags", MATRIX, ids=["-".join("%s=%s" % kv for kv in f.items()) or "defaults" for f in MATRIX])
def test_host_entry_fed_with_the_models_records_equals_the_model(gen_set, flags, tmp_path):
    path = gen_set[0]
    kw = dict(k=6, **flags)
    m = MM.run(path, **kw)
    assert not m.error and not m.failed
    res, _keep = _product_from_model(path, m, **kw)
    _assert_equal(res, m)
    da, db = tmp_path / "a", tmp_path / "b"
    da.mkdir()
    db.mkdir()
    assert res.demultiplex(da) == m.demultiplex(db)
    for f in sorted(os.listdir(db)):
        assert open(da / f).read() == open(db / f).read(), f
    assert sorted(os.listdir(da)) == sorted(os.listdir(db))


@pytest.mark.parametrize("chunk_size", [1000, 5000, 20000])
def test_chunk_plan_equals_the_model(chunk_size):
    from downpore_amd import trim as T
    for length in list(range(300, 16001, 1)):
        a, b = T.trim_chunk_plan(length, chunk_size), MM.chunk_plan(length, chunk_size)
        assert np.array_equal(a, b), (length, a.tolist(), b.tolist())


def test_chunk_size_100_is_refused_and_the_flag_is_named(gen_set):
    from downpore_amd import DpError
    from downpore_amd import trim as T
    with pytest.raises(DpError, match="chunk_size"):
        T.trim_chunk_plan(5000, 100)
    path = gen_set[0]
    m = MM.run(path, k=6)
    with pytest.raises(DpError, match="chunk_size"):
        _product_from_model(path, m, k=6, chunk_size=100)
    assert "chunk_size" in MM.run(path, k=6, chunk_size=100).error


def test_a_small_flush_threshold_gives_batches_and_zeroed_edge_counts(gen_set):
    path = gen_set[0]
    kw = dict(k=6, flush_seeds=500)
    m = MM.run(path, **kw)
    assert m.counters["batches"] >= 3
    assert m.stderr.count("Searching ") == m.counters["batches"]
    assert all(c == 0 for _, _, c in m.adapters)
    assert " \t 0 %" in m.stderr
    res, _keep = _product_from_model(path, m, **kw)
    _assert_equal(res, m)
    one = MM.run(path, k=6)
    assert one.counters["batches"] == 1 and any(c > 0 for _, _, c in one.adapters)


def test_eight_parameters_still_give_the_edge_stage_alone(gen_set):
    from downpore_amd import trim as T
    path = gen_set[0]
    m = M.run(path, k=6)
    R, F, B = _reads(path), _reads(TC.FRONT, 0), _reads(TC.BACK, 0)
    res = T.trim_apply(R, F, B, m.recs, m.counts, enabled=m.enabled, k=6)
    assert res.output == m.output and res.stderr == m.stderr and np.array_equal(res.table, m.table)
    assert len(res.plan) == 0 and len(res.splits) == 0 and res.extras == [] and res.stats["mid_chunks"] == 0
    assert "_(left)" not in res.output


@pytest.mark.parametrize("k", [5, 6])
def test_the_hosts_match_of_every_candidate_pair_equals_the_models_records(gen_set, k):
    """the exact host Match (the fallback for pairs beyond the matching kernel's working set, among them the (GA)n centres at
    k = 5) run on EVERY candidate pair of the model: its records are the model's, pair by pair and in Match's return order"""
    import ctypes as C
    from downpore_amd import trim as T
    path = gen_set[0]
    m = MM.run(path, k=k, determine_adapters=False)
    ix = T.trim_index(_reads(TC.FRONT, 0), _reads(TC.BACK, 0), k)
    H = T._host()
    H.dph_hand_trim_match.restype = C.c_int64
    H.dph_hand_trim_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    got = []
    out = np.zeros((4096, 6), dtype=np.int32)
    big = 0
    for a, c in m.candidates.tolist():
        cs = np.ascontiguousarray(m.chunk_segments(c), dtype=np.int32)
        asg = np.ascontiguousarray(ix["segs"][int(ix["seg_off"][a]):int(ix["seg_off"][a + 1])], dtype=np.int32)
        n = H.dph_hand_trim_match(cs.ctypes.data, len(cs), asg.ctypes.data, len(asg), int(ix["lengths"][a]), ix["n_seeds"], k, 85, a, c, out.ctypes.data,
                                  len(out))
        assert n <= len(out)
        got += out[:n].tolist()
        # seeds the chunk keeps when reduced to the adapter's (seeds/sequence.go:85-123): beyond 1024 the matching kernel hands the pair over
        mine = np.isin(cs[1::2], asg[1::2])
        kept = cs[1::2][mine]
        big += (1 + int((kept[1:] != kept[:-1]).sum()) if len(kept) else 0) > 1024
    assert len(m.candidates) > 100
    assert big > 0 if k == 5 else True, "no candidate pair reduces to more than 1024 seeds: the (GA)n class lost its purpose"
    assert got == m.recs.tolist()
