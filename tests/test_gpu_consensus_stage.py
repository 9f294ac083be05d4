"""Stage parity of the device consensus (run with `-m gpu` on an MI355X).

dp_consensus_paf - match_anchor_kernel + consensus_full_kernel<0|1|2> - is held to the oracle window by window: what the device
computed equals the oracle's lines, ignores and counts of that window, and what it left to the host is exactly what the documented
capacities of the last layout that ran, applied to the ORACLE's numbers (tests/consensus_cases.py: beyond()), say it cannot hold.
dp_consensus_align is held to multiAligner.Consensus on generated groups up to its limits.

Seed counts of the many-seeds pair (k = 10, seed_batch_size 40000): 794 reads -> 32796 seeds (small layout off, ids beyond 2^15),
797 reads -> 32711 seeds (small layout on with its largest ids).
"""
import numpy as np
import pytest

from tests import consensus_cases as CC
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

#: DP_CONS_LAYOUTS settings (None: unset)
SETTINGS = [None, "nosmall,nohuge", "nosmall,huge", "huge", "eager,nohuge"]
LAYOUT_ID = {"small": 0, "large": 1, "huge": 2}


def _new_ctx():
    import downpore_amd
    c = downpore_amd.Context(0)
    c.huge_on = False  # what the library keeps per context: the huge layout follows once a window was left to the host
    return c


@pytest.fixture(scope="module")
def ctx():
    c = _new_ctx()
    yield c
    c.close()


def _load(ctx, c):
    ctx.upload_reads(c.bases, c.off)
    ctx.round_begin(c.k, c.seed_kmers)
    ctx.import_segments(c.isegs)
    ctx.index_build(c.ioffs[:-1].astype(np.uint64), ((c.ioffs[1:] - c.ioffs[:-1]) // 2).astype(np.uint32))


def _round(ctx, c, monkeypatch, setting, pending=False):
    """One chaining stage + consensus stage under `setting`; returns (output, the layouts that ran in order)."""
    if setting is None:
        monkeypatch.delenv("DP_CONS_LAYOUTS", raising=False)
    else:
        monkeypatch.setenv("DP_CONS_LAYOUTS", setting)
    words = (setting or "").split(",")
    huge = False if "nohuge" in words else True if "huge" in words else ctx.huge_on
    small = "nosmall" not in words and len(c.seed_kmers) <= 32767
    ctx.find_overlaps(c.qsegs, c.qoffs.astype(np.uint64), 0.25, c.k, c.overlap_size // 2, on_device=True, pending=pending)
    out = ctx.consensus_paf(c.metas, c.rc_of, c.k, c.overlap_size)
    if (out["groups"]["flag"] == 1).any():
        ctx.huge_on = True
    return out, (["small"] if small else []) + ["large"] + (["huge"] if huge else [])


def _records(out, g):
    gm = out["groups"][g]
    s = int(gm["slot"])
    r = out["paf"][s:s + int(gm["n_lines"])]
    return np.stack([r[f].astype(np.int64) for f in CC.PAF_FIELDS], axis=1) if len(r) else np.zeros((0, 10), dtype=np.int64)


def _check(c, out, layouts, forced=()):
    """Every window of one call against the oracle; returns the windows left to the host (forced: windows a test hook sends there)."""
    gms = out["groups"]
    assert len(gms) == c.n_windows
    assert set(np.unique(gms["flag"]).tolist()) <= {0, 1}
    last = layouts[-1]
    beyond = CC.beyond(c, last)
    left = set(np.flatnonzero(gms["flag"] == 1).tolist())
    # host-left windows: justified by the oracle's numbers and the last layout's capacities - and every window inside them computed
    for g in sorted(left):
        # (the oracle ran this round to the end: none of its windows is a state the reference would panic in)
        assert int(gms["reserved"][g]) in CC.CAPACITY_REASONS, (c.name, last, g, int(gms["reserved"][g]), c.stats[g].tolist())
    want_left = {g for g, why in enumerate(beyond) if why} | set(forced)
    assert left == want_left, (c.name, last, "left without a capacity exceeded:", [(g, c.stats[g].tolist(), int(c.query_seeds[g])) for g in sorted(left - want_left)][:5],
                               "computed beyond a capacity:", [(g, beyond[g]) for g in sorted(want_left - left)][:5])
    assert np.array_equal(gms["n_matches"], c.stats[:, 0])
    smallest = {}
    for n, ws in CC.split(c).items():
        for g in ws:
            smallest[g] = n
    for g in range(c.n_windows):
        if g in left:
            continue
        gm = gms[g]
        matches, kept, _, _, _, parts, bad_back, empty = c.stats[g].tolist()
        want = c.recs[g]
        if matches < 2 or parts < 2:
            assert len(want) == 0
        assert int(gm["n_lines"]) == len(want), (c.name, g)
        got = _records(out, g)
        assert np.array_equal(got, want), (c.name, g, got.tolist(), want.tolist())
        s = int(gm["slot"])
        assert out["ignore_ids"][s:s + int(gm["n_ignore"])].tolist() == c.ignores[g], (c.name, g)
        assert (int(gm["bad_back"]), int(gm["empty_match"])) == (bad_back, empty), (c.name, g)
        if parts >= 2:
            # the layout that computed it: the first of the chain that holds the window by the oracle's counts.  (The small layout
            # also passes on a window with a value beyond 16 bits; every gap and offset of a trimmed target lies inside the
            # stretch a query window of at most 3000 bases aligns to, a few thousand bases: there is none here.)
            first = next(n for n in layouts if LAYOUT_ID[n] >= LAYOUT_ID[smallest[g]])
            assert int(gm["reserved"]) >> 30 == LAYOUT_ID[first], (c.name, g, layouts, smallest[g], int(gm["reserved"]) >> 30)
    if not left:
        assert (int(gms["bad_back"].sum()), int(gms["empty_match"].sum())) == (c.bad_back, c.empty_match)
    return left


def _require_split(c, least):
    by = CC.split(c)
    for lay, n in least.items():
        assert len(by[lay]) >= n, (c.name, lay, {k: len(v) for k, v in by.items()})
    return by


# what each case must reach (smallest fitting layout by the oracle's counts -> least number of windows), or the test says nothing
REACH = {"ordinary": dict(small=50, large=50, huge=1), "deep": dict(small=1, large=1, huge=50, host=50),
         "long": dict(large=1, huge=1, host=100), "seeds_over": dict(large=500, huge=100), "seeds_under": dict(small=100, large=500, huge=100)}


@pytest.mark.parametrize("name", list(CC.CASES))
def test_consensus_stage_matches_oracle_under_every_layout_setting(ctx, monkeypatch, name):
    c = CC.oracle_case(name)
    _require_split(c, REACH[name])
    if name in CC.SEED_COUNTS:
        assert len(c.seed_kmers) == CC.SEED_COUNTS[name]
        assert (len(c.seed_kmers) > 32767) == (name == "seeds_over")
        if name == "seeds_over":
            assert max(int(c.isegs[a + 1:b:2].max(initial=0)) for a, b in zip(c.ioffs[:-1], c.ioffs[1:])) >= 1 << 15  # indexed seed ids
    if name == "deep":  # windows of exactly 64 sequences that the huge layout holds, and of more
        inside = [g for g, why in enumerate(CC.beyond(c, "huge")) if not why]
        assert any(c.stats[g, 1] == 64 for g in inside) and (c.stats[:, 1] > 64).any()
    _load(ctx, c)
    outs = {}
    for setting in SETTINGS:
        out, layouts = _round(ctx, c, monkeypatch, setting)
        left = _check(c, out, layouts)
        if setting is not None and "nohuge" in setting:
            assert left == {g for g, why in enumerate(CC.beyond(c, "large")) if why}
        outs[setting] = (out, left)
    # computed windows agree record for record across the settings
    base, base_left = outs["nosmall,huge"]
    for setting, (out, left) in outs.items():
        for g in range(c.n_windows):
            if g in left or g in base_left:
                continue
            a, b = out["groups"][g], base["groups"][g]
            for f in ("slot", "n_lines", "n_ignore", "bad_back", "empty_match", "flag", "n_matches"):
                assert a[f] == b[f], (name, setting, g, f)
            assert int(a["reserved"]) & 0x3fffffff == int(b["reserved"]) & 0x3fffffff, (name, setting, g)
            assert np.array_equal(_records(out, g), _records(base, g)), (name, setting, g)


def test_ordinary_round_leaves_no_window_to_the_host(ctx, monkeypatch):
    """Cap: with the huge layout on, every window of the ordinary round is computed on the device."""
    c = CC.oracle_case("ordinary")
    _load(ctx, c)
    out, layouts = _round(ctx, c, monkeypatch, "huge")
    assert layouts[-1] == "huge" and not (out["groups"]["flag"] != 0).any()
    assert int(out["groups"]["n_lines"].sum()) == sum(len(ls) for ls in c.lines) == 5674


def test_cons_flag_every_is_read_by_every_call(ctx, monkeypatch):
    """DP_TUNE=cons_flag_every between three calls of one process, on the module's context, under one layout setting, on the case with
    the fewest reads.  Unset: the windows left to the host are the ones the oracle's numbers say the last layout cannot hold.  =2: every
    window with g % 2 == 0 that builds a consensus at all is left to the host as well (consensus_full_kernel: the hook sits behind the
    exit of the windows with fewer than two matches, which no path builds a consensus for), the odd windows are left exactly as before,
    and every window that is not left still equals the oracle.  Unset again: the first call's output."""
    c = CC.oracle_case("deep")
    assert c.n_windows >= 4
    _load(ctx, c)
    monkeypatch.delenv("DP_TUNE", raising=False)
    first, layouts = _round(ctx, c, monkeypatch, "huge")
    left = _check(c, first, layouts)
    assert left == {g for g, why in enumerate(CC.beyond(c, "huge")) if why}
    forced = {g for g in range(0, c.n_windows, 2) if c.stats[g, 0] >= 2}
    assert len(forced - left) >= 2 and any(g % 2 == 1 and g not in left and c.stats[g, 0] >= 2 for g in range(c.n_windows))
    monkeypatch.setenv("DP_TUNE", "cons_flag_every=2")
    second, layouts2 = _round(ctx, c, monkeypatch, "huge")
    assert layouts2 == layouts
    left2 = _check(c, second, layouts2, forced)
    assert left2 == left | forced and forced <= left2
    assert {g for g in left2 if g % 2} == {g for g in left if g % 2}
    monkeypatch.delenv("DP_TUNE")
    third, layouts3 = _round(ctx, c, monkeypatch, "huge")
    assert layouts3 == layouts and _check(c, third, layouts3) == left
    assert np.array_equal(third["groups"], first["groups"])
    for g in range(c.n_windows):
        assert np.array_equal(_records(third, g), _records(first, g)), g


def test_huge_layout_follows_the_first_window_left_to_the_host(monkeypatch):
    """DP_CONS_LAYOUTS unset on a fresh context: the first call ends with the large layout and leaves what that cannot hold; that
    switches the huge layout on for the context's next calls."""
    c = CC.oracle_case("ordinary")
    ctx = _new_ctx()
    try:
        _load(ctx, c)
        out, layouts = _round(ctx, c, monkeypatch, None)
        assert layouts == ["small", "large"]
        assert _check(c, out, layouts) == {g for g, why in enumerate(CC.beyond(c, "large")) if why} != set()
        out, layouts = _round(ctx, c, monkeypatch, None)
        assert layouts == ["small", "large", "huge"]
        assert _check(c, out, layouts) == set()
    finally:
        ctx.close()


def test_pending_chaining_stage_is_finished_by_the_consensus_call(monkeypatch):
    """The chaining stage left pending (bits 1 and 2) on a fresh context: the consensus call sizes its output for 4096 pairs, the
    ordinary round has more, so the call repeats itself - and returns what the call after a finished stage returns."""
    c = CC.oracle_case("ordinary")
    assert int(c.stats[:, 0].sum()) > 4096
    ctx = _new_ctx()
    try:
        _load(ctx, c)
        pend, layouts = _round(ctx, c, monkeypatch, "huge", pending=True)
        assert _check(c, pend, layouts) == set()
        plain, layouts = _round(ctx, c, monkeypatch, "huge")
        assert _check(c, plain, layouts) == set()
        assert np.array_equal(pend["groups"], plain["groups"])
        for g in range(c.n_windows):
            assert np.array_equal(_records(pend, g), _records(plain, g)), g
            s, ni = int(plain["groups"]["slot"][g]), int(plain["groups"]["n_ignore"][g])
            assert np.array_equal(pend["ignore_ids"][s:s + ni], plain["ignore_ids"][s:s + ni]), g
    finally:
        ctx.close()


# ---- dp_consensus_align on generated groups ---------------------------------------------------------------------------------------

_want = {}


def _oracle_group(k, name):
    if (k, name) not in _want:
        red = CC.align_groups(k)[name][0]
        _want[(k, name)] = O.hand_consensus([r if r else [0] for r in red], k)
    return _want[(k, name)]


def _align(ctx, k, names):
    groups = CC.align_groups(k)
    segs, seq_off, group_off = [], [0], [0]
    for n in names:
        for r in groups[n][0]:
            segs += r
            seq_off.append(len(segs))
        group_off.append(len(seq_off) - 1)
    out = ctx.consensus_align(segs, seq_off, group_off, k)
    assert len(out["flags"]) == len(names)
    s = 0
    for gi, n in enumerate(names):
        red, flagged = groups[n]
        # Cap: no group within 64 sequences and 6144 ints is flagged - and every one beyond is
        assert bool(out["flags"][gi]) == flagged, (k, n, len(red), sum(len(r) for r in red))
        if not flagged:
            cons, pairs, _ = _oracle_group(k, n)
            assert np.array_equal(out["cons"][gi], cons), (k, n)
            survive = {i for i in range(len(red)) if len(out["match_a"][s + i]) >= 3}
            assert survive == set(pairs), (k, n)
            for i in survive:
                assert np.array_equal(out["match_a"][s + i], pairs[i][0]) and np.array_equal(out["match_b"][s + i], pairs[i][1]), (k, n, i)
            for i, r in enumerate(red):
                if not r:
                    assert len(out["match_a"][s + i]) == 0, (k, n, i)
        s += len(red)


@pytest.mark.parametrize("k", [10, 13])
def test_consensus_align_single_groups(ctx, k):
    for name in CC.align_groups(k):
        _align(ctx, k, [name])


@pytest.mark.parametrize("k", [10, 13])
@pytest.mark.parametrize("n_groups", [4, 5, 9])
def test_consensus_align_several_groups_a_call(ctx, k, n_groups):
    """A block holds four waves, one group each: calls of one block exactly, one block and a wave, two blocks and a wave - groups of
    mixed sizes, flagged ones among them, in two orders."""
    names = list(CC.align_groups(k))
    order = ["cap6144", "clean3", "seqs65", "lossy64", "empty", "cap6145", "lossy40", "two", "seqs64", "apart", "clean64", "lossy20", "seqs63"]
    assert sorted(order) == sorted(names)
    _align(ctx, k, order[:n_groups])
    _align(ctx, k, order[::-1][:n_groups])
