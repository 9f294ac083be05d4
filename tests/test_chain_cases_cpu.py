"""The oracle side of the chaining stage tests (no GPU): the entry that runs Overlapper.FindOverlaps on crafted segments gives what a
traced generated round gives; the per-pair profile does not change the chains; and every crafted case of tests/chain_cases.py sits,
by the oracle's own numbers, on the side of its boundary that its name states - so that tests/test_gpu_chain_stage.py cannot pass on
cases that have drifted away from the capacities they are there for."""
import json
import os

import numpy as np
import pytest

from tests import chain_cases as CC
from tests import oracle_lib as O

HAND = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand")


def test_segments_entry_gives_a_traced_round():
    """one generated round (k = 10): the entry on the trace's indexed sequences and queries = the trace's candidates and matches"""
    bases, off = O.gen_reads(11, 30000, 120, 3000, 0.02, True)
    run = O.OverlapRun(O.ReadSet(bases, off, min_len=1000), k=10, max_rounds=1, traces=True)
    isegs, ioffs = run.trace(0, "indexedSegments")
    qsegs, qoffs = run.trace(0, "querySegments")
    index = [isegs[ioffs[i]:ioffs[i + 1]] for i in range(len(ioffs) - 1)]
    queries = [qsegs[qoffs[i]:qoffs[i + 1]] for i in range(len(qoffs) - 1)]
    got = O.find_overlaps_segments(index, queries, len(run.trace(0, "seedKmers")), 0.25, 10, 500)
    assert got["limit"] == 0
    cdata, coffs = run.trace(0, "candidates")
    assert np.array_equal(got["cand_off"], coffs) and np.array_equal(got["cand"], cdata)
    ma, mao = run.trace(0, "matchA")
    mb, _ = run.trace(0, "matchB")
    assert len(mao) > 50
    assert np.array_equal(got["query"], run.trace(0, "matchQueryIndex"))
    assert np.array_equal(got["target"], run.trace(0, "matchTarget"))
    assert np.array_equal(got["off"], mao) and np.array_equal(got["match_a"], ma) and np.array_equal(got["match_b"], mb)
    # the pair table: one row per candidate, and a kept chain for exactly the matches
    assert len(got["pairs"]) == len(cdata)
    kept = got["pairs"][got["pairs"][:, O.PAIR_COLS.index("kept")] > 0]
    assert np.array_equal(kept[:, 0], got["query"]) and np.array_equal(kept[:, 2], got["target"])
    assert np.array_equal(kept[:, O.PAIR_COLS.index("kept")], np.diff(mao))


@pytest.mark.parametrize("name", ["pairwise_two_chains.json", "pairwise_break_after_first_extension.json"])
def test_profile_leaves_the_chains_alone(name):
    h = json.load(open(os.path.join(HAND, name)))
    ms, prof = O.pairwise_profile(h["a_segments"], h["b_segments"], h["min_matches"], h["k"])
    assert [(a.tolist(), b.tolist()) for a, b in ms] == [(m["match_a"], m["match_b"]) for m in h["expect_pairwise"]]
    assert prof["limit"] == 0 and prof["resultsSize"] == len(ms) and prof["longestChain"] == max(len(m["match_a"]) for m in h["expect_pairwise"])


def test_caps_are_the_sources():
    """the capacity table against the text of dp_overlap.hip"""
    import re
    src = open(os.path.join(os.path.dirname(HAND), "..", "..", "downpore_amd", "csrc", "dp_overlap.hip")).read()
    for name in ("C_ACAP", "C_BCAP", "C_LNODES", "C_REV", "C_QSW", "C_OPEN", "C_RESULTS", "C_POOLSTATES"):
        val = int(re.search(r"#define %s (\d+)" % name, src).group(1))
        assert val == CC.CAPS[{"C_OPEN": "OPEN", "C_RESULTS": "RESULTS", "C_POOLSTATES": "POOL"}.get(name, name)], name
    assert "#define C_NODES (1u << 16)" in src and CC.CAPS["C_NODES"] == 1 << 16
    wave = re.search(r"struct CWave \{.*?enum \{([^}]*)\}", src, re.S).group(1)
    slim = re.search(r"struct CSlim \{.*?enum \{([^}]*)\}", src, re.S).group(1)
    assert "COLN = 64, EVN = C_REV, ACAP = C_ACAP, RSEEDS = 255, SLIM = 0, ROWS = 64, BCAP = C_BCAP" in wave
    assert "COLN = 64, EVN = 128, ACAP = 256, RSEEDS = 64, SLIM = 1, ROWS = 32, BCAP = C_BCAP" in slim
    assert (CC.CAPS["RSEEDS"], CC.CAPS["REG_ROWS"]) == (255, 64)
    assert [CC.CAPS[x] for x in ("SLIM_COLN", "SLIM_EVN", "SLIM_ACAP", "SLIM_RSEEDS", "SLIM_ROWS")] == [64, 128, 256, 64, 32]


@pytest.mark.parametrize("name", CC.CASE_NAMES + ("many_grow",))
def test_case_is_where_its_name_says(name):
    c, res = CC.case(name), CC.oracle(name)
    want = CC.ERROR_CASES.get(name, 0)
    assert res["limit"] == want == c.error, "the oracle's limit"
    assert all(len(q) <= 2 * 65535 + 1 for q in c.queries)
    for label, q, t, claim in c.claims:
        row = CC.pair_row(name, q, t)
        assert row is not None, (label, "the loop never reached the pair")
        if want:
            assert (res["limit_query"], row["rank"], row["limit"]) == (q, res["limit_rank"], want), label
        for key, val in claim.items():
            if isinstance(val, tuple):
                assert val[0] == "ge" and row[key] >= val[1], (label, key, row[key], val)
            else:
                assert row[key] == val, (label, key, row[key], val)
    if not want:
        assert len(res["pairs"]) == len(res["cand"])


def test_sizes_case_pairs_predict_the_paths_their_names_say():
    """the capacity table turns the oracle's profiles of the boundary pairs into the expected paths: (chained on the slim layout,
    tier of the full layout).  The parameters the builders use (sizes, gaps) are pinned by this table."""
    c = CC.case("sizes")
    want = {
        "qseeds_64": (True, 1), "qseeds_65": (True, 1), "qseeds_127": (True, 1), "qseeds_128": (False, 1), "qseeds_129": (False, 1),
        "qseeds_255": (False, 1), "qseeds_256": (False, 3), "qseeds_257": (False, 3),
        "alen_64_at": (True, 1), "alen_64_over": (False, 2), "tgt_1056_at": (True, 1), "tgt_1056_over": (False, 3),
        "bev_128": (True, 1), "bev_129": (False, 1), "bev_256": (False, 1), "bev_257": (False, 2),
        "open_32": (True, 1), "open_33": (False, 1), "open_64": (False, 1), "open_65": (False, 2),
        "chain_64": (False, 2), "chain_65": (False, 2),
    }
    seen = set()
    for label, q, t, _ in c.claims:
        mm = CC.pair_row("sizes", q, t)["mm"]
        assert (CC.fits_slim(c, q, t, mm), CC.full_tier(c, q, t, mm)) == want[label], label
        seen.add(label)
    assert seen == set(want)
    c = CC.case("links")
    label, q, t, _ = c.claims[0]
    assert not CC.fits_slim(c, q, t, 5) and CC.full_tier(c, q, t, 5) == 2
    c = CC.case("kept_wide")
    for (label, q, t, _), tier in zip(c.claims, (2, 2, 3, 3)):
        mm = CC.pair_row("kept_wide", q, t)["mm"]
        assert not CC.fits_slim(c, q, t, mm) and CC.full_tier(c, q, t, mm) == tier, label


def test_gap_cases_sit_on_the_window():
    """every gap pair: the chain breaks at seed 6 exactly when the query's gap is outside gapRange of the target's"""
    for name in ("perfect", "perfect_clamp"):
        c = CC.case(name)
        hits = 0
        for label, q, t, _ in c.claims:
            if label.startswith("gap_"):
                row = CC.pair_row(name, q, t)
                inside = label.endswith("_min") or label.endswith("_max")
                assert (row["longestChain"] == 12) == inside, (label, row)
                hits += 1
        assert hits == (8 if name == "perfect" else 4)


def test_ratchet_cases_move_as_stated():
    res = CC.oracle("ratchet_steps")
    assert res["pairs"][:, O.PAIR_COLS.index("mm")].tolist() == [3, 4, 6, 10, 16]
    assert res["pairs"][:, O.PAIR_COLS.index("kept")].tolist() == [6, 10, 16, 25, 40]
    # the late start: under the stale value (9) the pair's answer is another chain than under the one in force (11)
    c = CC.case("ratchet_stale")
    label, q, t, _ = c.claims[2]
    assert label == "late_start"
    stale = O.pairwise_profile(c.queries[q], c.index[t], 9, c.k)[0][-1]
    fresh = O.pairwise_profile(c.queries[q], c.index[t], 11, c.k)[0][-1]
    assert stale[0].tolist() == list(range(20, 30)) and fresh[0].tolist() == list(range(12))


def test_many_candidates_counts():
    res = CC.oracle("many")
    assert np.diff(res["cand_off"]).tolist() == [n for n, _ in CC.MANY]
    first = {}
    for row in res["pairs"]:
        if row[O.PAIR_COLS.index("kept")] > 0:
            first.setdefault(int(row[0]), int(row[1]))
    assert [first[q] for q in range(len(CC.MANY))] == [h for _, h in CC.MANY]
    # the grown form needs more scratch ints than the stage's first size (2^18): candidates x query seeds, over all queries
    c, res = CC.case("many_grow"), CC.oracle("many_grow")
    assert sum(int(n) * (len(q) // 2) for n, q in zip(np.diff(res["cand_off"]), c.queries)) > 1 << 18


def test_sweep_mostly_finishes():
    for hf in CC.SWEEP_HIT_FRACTIONS:
        name = "sweep_%g" % hf
        c = CC.case(name)
        done = 0
        for q in range(len(c.queries)):
            r = O.find_overlaps_segments(c.index, [c.queries[q]], c.n_seed_ids, c.hf, c.k, c.max_length)
            done += r["limit"] == 0
        assert done >= 250, (name, done)


def test_predicted_paths_cover_every_pair():
    for name in ("sizes", "ratchet_steps", "ratchet_stale", "many"):
        res = CC.oracle(name)
        paths = CC.predict_paths(name, 3)
        assert len(paths) == len(res["cand"])
        assert all(CC.kernel_of(p) in (CC.K_WALK0, 2, 3, 4, CC.K_FINAL) for p in paths.values())
    # the ratchet case: one hit per step - walk 0, the three resolve steps, the final walk
    paths = CC.predict_paths("ratchet_steps", 3)
    assert [CC.kernel_of(paths[(0, t)]) for t in range(5)] == [1, 2, 3, 4, 15]
