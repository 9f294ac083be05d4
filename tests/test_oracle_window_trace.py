"""The oracle's per-window trace of a round (OverlapRun.trace_windows: which window printed which PAF line and ignored which
read, and what BuildConsensus saw there) is held to the fields the trace had before, and the inputs of
tests/test_gpu_consensus_stage.py are shown to reach what that file relies on - all on the CPU."""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import oracle_lib as O

COL = {n: i for i, n in enumerate(O.OverlapRun.WINDOW_COLS)}


def _check_round(run, rnd):
    w = run.trace_windows(rnd)
    st, lines, ignores = w["stats"], w["lines"], w["ignores"]
    n = len(st)
    assert n == run.trace(rnd, "scalars")[1]  # numQuerySeqs
    # lines joined in window order are the round's PAF
    assert "".join(ln + "\n" for ls in lines for ln in ls) == run.trace_paf(rnd)
    pw = run.trace(rnd, "pafWindow")
    assert len(pw) == run.trace_paf(rnd).count("\n") and np.all(np.diff(pw) >= 0)
    # the SetIgnore calls, as a set, are the reads the round newly ignored; in call order their first occurrences are that list
    calls = run.trace(rnd, "ignoreCalls")
    assert len(calls) == len(run.trace(rnd, "ignoreWindow")) and np.all(np.diff(run.trace(rnd, "ignoreWindow")) >= 0)
    newly = run.trace(rnd, "newlyIgnored")
    assert set(calls.tolist()) == set(newly.tolist())
    assert list(dict.fromkeys(calls.tolist())) == newly.tolist()
    # counts against matchQueryIndex: a window's matches are those of its two queries
    mq = run.trace(rnd, "matchQueryIndex")
    assert np.array_equal(st[:, COL["matches"]], np.bincount(mq // 2, minlength=n))
    assert st[:, COL["matches"]].sum() == run.trace(rnd, "scalars")[2]  # hits
    for g in range(n):
        m, kept, trimmed, reduced, cons, parts, _, empty = st[g].tolist()
        assert 0 <= kept <= m and 0 <= parts <= kept
        if m < 2:
            assert (kept, trimmed, reduced, cons, parts) == (0, 0, 0, 0, 0)
        assert trimmed >= 3 * kept and trimmed % 2 == kept % 2  # a trimmed sequence: [gap, seed, gap] at least, an odd number of ints
        assert reduced <= trimmed                               # Reduced() only drops seeds
        if kept < 2:
            assert (reduced, cons, parts) == (0, 0, 0)          # no alignment with fewer than two sequences
        else:
            assert cons % 2 == 1 and cons <= reduced + 1
        assert len(lines[g]) == (parts - 1 if parts >= 2 else 0)  # one line per part after the first
        assert empty <= len(lines[g])
        if parts < 2:
            assert not ignores[g]
        assert len(ignores[g]) <= max(parts, 0)
    return st


def test_window_trace_two_rounds():
    """A job of more than one round: every round's window fields agree with its own older fields, and the diagnostics counted by
    window add up to the job's."""
    bases, off = O.gen_reads(31, 60000, 300, 4000, 0.02, True)
    rs = O.ReadSet(bases, off, min_len=1000)
    run = O.OverlapRun(rs, k=10, query_batch_size=150, max_rounds=-1, traces=True)
    assert run.rounds >= 2
    bad = empty = 0
    for rnd in range(run.rounds):
        st = _check_round(run, rnd)
        bad += int(st[:, COL["bad_back"]].sum())
        empty += int(st[:, COL["empty_match"]].sum())
    assert "bad_back_suppressed=%d empty_match_panics_avoided=%d" % (bad, empty) in run.err
    assert "".join(run.trace_paf(r) for r in range(run.rounds)) == run.paf


# windows and PAF lines of the rounds, and what each must reach for the device tests to mean something: (windows, lines, smallest
# number of windows whose smallest fitting layout is small / large / huge / none)
_REACH = {"ordinary": (336, 5674, dict(small=50, large=50, huge=1, host=0)),
          "deep": (320, 12203, dict(small=1, large=1, huge=50, host=50)),
          "long": (180, 7144, dict(small=0, large=1, huge=1, host=100))}


@pytest.mark.parametrize("name", list(_REACH))
def test_stage_cases_reach_the_layouts(name):
    c = CC.oracle_case(name)
    windows, n_lines, least = _REACH[name]
    assert c.n_windows == windows and sum(len(ls) for ls in c.lines) == n_lines
    st = _check_round(c.run, 0)
    assert int(st[:, COL["bad_back"]].sum()) == c.bad_back and int(st[:, COL["empty_match"]].sum()) == c.empty_match
    by = CC.split(c)
    for lay, n in least.items():
        assert len(by[lay]) >= n, (name, lay, {k: len(v) for k, v in by.items()})
    if name == "ordinary":
        assert not by["host"]  # with the huge layout on, nothing of the ordinary round is left to the host
        assert st[:, COL["matches"]].max() <= 29
    if name == "deep":
        why = {r for w in CC.beyond(c, "huge") for r in w}
        assert why == {"sequences", "trimmed ints", "reduced ints", "consensus ints"}
        assert (st[:, COL["kept"]] > 64).sum() == 16 and c.query_seeds.max() == 164
        # windows on either side of the sequence limit, and one the large layout holds but for its trimmed ints
        assert (st[:, COL["kept"]] == 64).any() or (st[:, COL["kept"]] == 63).any()
    if name == "long":
        assert c.query_seeds.max() == 325
        assert any("query seeds" in w for w in CC.beyond(c, "huge"))


@pytest.mark.parametrize("k", [10, 13])
def test_generated_groups_run_on_the_oracle(k):
    """The generated groups of the alignment kernel's test: Reduced() in Python is what the oracle's own Reduced() leaves alone (so the
    oracle, fed the reduced forms, aligns exactly what the device is given), and every group runs through multiAligner.Consensus."""
    sizes = {}
    for name, (red, flagged) in CC.align_groups(k).items():
        again, maps = CC.reduce_group([r if r else [0] for r in red], k)
        assert again == red and all(m == list(range(len(m))) for m in maps), name
        ints = sum(len(r) for r in red)
        sizes[name] = (len(red), ints)
        assert flagged == (len(red) > 64 or ints > 6144), name
        cons, pairs, order = O.hand_consensus([r if r else [0] for r in red], k)
        assert len(cons) % 2 == 1 and all(len(a) >= 3 for a, _ in pairs.values())
        if name in ("clean3", "clean64"):
            assert len(pairs) == len(red)  # identical sequences: all survive
    assert sizes["cap6144"] == (64, 6144) and sizes["cap6145"] == (63, 6145)
    assert sizes["seqs65"][0] == 65 and sizes["seqs64"][0] == 64 and sizes["seqs63"][0] == 63 and sizes["two"][0] == 2
