"""`map -all_sequences` without a GPU: the model (tests/native/map_multi_model.cpp) restates the rule of DESIGN 4.7 on the oracle's
types.  With one reference sequence it must be the oracle byte for byte; its two deliberate mutations must be caught by what is
known about the reads without any mapper; and a ground-truth witness checks the rule itself against where reads were drawn from."""
import glob
import json
import os

import numpy as np
import pytest

from tests import map_multi_cases as MC
from tests import map_multi_model as MM
from tests import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAP_FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "map_*_k11.json")))

# (seed, G, N, L, e, variable, circular): tests/test_gpu_map.py's test_map_paf_bit_exact, then the generators of the map_*_k11 fixtures
SINGLE = [(3, 200000, 300, 8000, 0.0, False, True), (4, 150000, 300, 6000, 0.05, True, True), (5, 300000, 200, 9000, 0.10, True, False)]
for _p in MAP_FIXTURES:
    _fx = json.load(open(_p))
    _g = _fx["generator"]
    assert _fx["k"] == 11
    SINGLE.append((_g["seed"], _g["genome"], _g["reads"], _g["read_len"], _g["error"], _g["variable"], _fx["circular"]))


def test_the_three_map_fixtures_are_there():
    assert len(MAP_FIXTURES) == 3 and len(SINGLE) == 6


@pytest.mark.parametrize("case", SINGLE, ids=lambda c: "-".join(str(v) for v in c))
def test_model_with_one_sequence_is_the_oracle(case):
    seed, G, N, L, e, variable, circular = case
    genome = np.frombuffer(O.gen_genome(seed, G), dtype=np.uint8)
    goff = np.array([0, G], dtype=np.int64)
    bases, off = O.gen_reads(seed, G, N, L, e, variable)
    want, werr = O.map_run(O.ReadSet(genome, goff, min_len=0, himem=False), O.ReadSet(bases, off, min_len=500, himem=False),
                           circular=circular, k=11)
    assert want.count("\n") > N // 2
    for all_sequences in (True, False):
        got, gerr = MM.run(genome, goff, bases, off, circular=circular, all_sequences=all_sequences)
        assert got == want and gerr == werr


def test_model_without_the_switch_uses_the_first_sequence_only():
    """all_sequences = 0 on a file of seven sequences: the oracle's run (k-mers counted over all of them, the first one mapped against)"""
    ref_bases, ref_off, bases, off, _ = MC.multi_case()
    want, werr = O.map_run(O.ReadSet(ref_bases, ref_off, min_len=0, himem=False), O.ReadSet(bases, off, min_len=500, himem=False))
    got, gerr = MM.run(ref_bases, ref_off, bases, off, all_sequences=False)
    assert got == want and gerr == werr and set(ln.split("\t")[5] for ln in got.splitlines()) == {"r0000000"}


@pytest.fixture(scope="module")
def multi():
    ref_bases, ref_off, bases, off, truth = MC.multi_case()
    return dict(ref=(ref_bases, ref_off), reads=(bases, off), truth=truth, read_len=np.diff(off))


@pytest.mark.parametrize("circular", [True, False])
def test_model_on_the_multi_sequence_case_agrees_with_where_the_reads_came_from(multi, circular):
    """The input of the GPU suite's model comparison, checked here against the truth - and for the three properties that suite
    asserts of it: at least 4 target names, a read with lines on two targets, "Multiple mappings" above 0."""
    paf, err = MM.run(*multi["ref"], *multi["reads"], circular=circular)
    assert MC.check_lines(paf, multi["ref"][1], multi["truth"], multi["read_len"]) >= 200
    rows = MC.parse(paf)
    assert len(set(r[5] for r in rows)) >= 4
    by_read = {}
    for r in rows:
        by_read.setdefault(r[0], set()).add(r[5])
    assert any(len(v) > 1 for v in by_read.values())
    assert int(err.split("Multiple mappings: ")[1].split("\n")[0]) > 0
    notes = [ln for ln in err.splitlines() if "no circular join chunk" in ln]
    # the sequences shorter than query_size: the one of 900 bases and the one of 30 (which has no seed window either)
    assert [ln.split()[1] for ln in notes] == (["r0000003", "r0000004"] if circular else [])
    assert err.splitlines()[0].startswith("K-mer counting complete") and err.splitlines()[-4].startswith("Uniquely mapped: ")


@pytest.mark.parametrize("mutation,what", [(MM.ISCONSISTENT_IGNORES_REF, "a read that spans two sequences is joined across them"),
                                           (MM.FIRST_LENGTH_FOR_EVERY_END, "a hit on another sequence than the first gets its End from L_0")])
def test_a_mutated_model_is_caught_by_the_truth(multi, mutation, what):
    paf, _ = MM.run(*multi["ref"], *multi["reads"], circular=True, mutation=mutation)
    with pytest.raises(AssertionError):
        MC.check_lines(paf, multi["ref"][1], multi["truth"], multi["read_len"])


def _witness(e, seed):
    """400 reads of 6 kb, each wholly inside one sequence and at least chunk_size from its ends.  Returns (reads left out because
    the oracle alone misplaces them on the one-sequence layout, N_single, N_multi, lines that name a foreign sequence)."""
    ref_bases, ref_off = MC.reference()
    bases, off, truth = MC.witness_reads(seed, ref_bases, ref_off, 400, 6000, e)
    n = len(truth)
    total = int(ref_off[-1])
    single, _ = O.map_run(O.ReadSet(ref_bases, np.array([0, total], dtype=np.int64), min_len=0, himem=False),
                          O.ReadSet(bases, off, min_len=500, himem=False))
    hit_single, misplaced = set(), set()
    for ln in single.splitlines():
        f = ln.split("\t")
        r, s, t = int(f[0][1:]), int(f[7]), int(f[8])
        c, start, _ = truth[r]
        a = int(ref_off[c]) + start
        if s < a + 6000 and t > a:
            hit_single.add(r)
        elif not (MC.touches_copy(c, start, start + 6000) and s < int(ref_off[-2]) + (start - MC.COPY[0]) + 6000 and t > int(ref_off[-2]) + (start - MC.COPY[0])):
            misplaced.add(r)  # a line that overlaps neither the read's origin nor, for a read from the copied stretch, its copy
    left_out = misplaced
    paf, _ = MM.run(ref_bases, ref_off, bases, off)
    hit_multi, foreign = set(), []
    for r, qlen, qs, qe, strand, t, tl, s, e2 in MC.parse(paf):
        if r in left_out:
            continue
        c, start, _ = truth[r]
        if t == c and s < start + 6000 and e2 > start:
            hit_multi.add(r)
        if t != c and not MC.touches_copy(c, start, start + 6000):
            foreign.append((r, MC.NAMES[c], MC.NAMES[t]))
    return n, len(left_out), len(hit_single - left_out), len(hit_multi), foreign


@pytest.mark.parametrize("e,seed", [(0.0, 101), (0.05, 102)], ids=["error-free", "5-percent"])
def test_ground_truth_witness(e, seed):
    """Independent of the model's text: reads drawn from inside one sequence (a) are never reported on a sequence they were not drawn
    from (reads from the copied stretch are exempt), and (b) are found on their own sequence, over their true interval, as often as
    the unchanged oracle finds them when the same bases are given as ONE sequence - less 1 % of the reads for seeds and chunk starts
    that differ between the two layouts.  A read the oracle alone misplaces is left out (at most 1 %).  Default flags, k = 11.
    Counts on record: profiles/map_multi.txt."""
    n, left_out, n_single, n_multi, foreign = _witness(e, seed)
    print("witness e=%.2f: reads %d, left out %d, N_single %d, N_multi %d, foreign lines %d" % (e, n, left_out, n_single, n_multi, len(foreign)))
    assert left_out <= n // 100
    assert not foreign, foreign[:5]
    assert n_multi >= n_single - n // 100
