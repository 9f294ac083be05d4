"""Stage parity of window mapping at the device boundary (run with `-m gpu` on an MI355X): dp_map_windows, dp_map_windows_shard,
dp_query_candidates, dp_index_borrow and both index layouts, held against
  a. the oracle's trace of performMapping (tests/oracle_lib.MapRun) on three seeded `map` runs - windows in, candidates and
     chains out, array for array, in every layout the mapper can put the index in;
  b. the oracle's GetSharedIDs on the sparse index query's count rule (the ladder tests of tests/test_gpu_kernels.py again through
     dp_query_candidates, both layouts; queries in which the 16-ladder's p7 term decides; ids on either side of the kernel's
     8 192-id tiles);
  c. the plain model of tests/map_model.py on crafted batches that make dp_map_windows launch again - the BIG variant, a record
     overflow, an int overflow - on the whole index and on two shards, each with a window pair whose first chain only survives
     when the relaunch starts from the caller's thresholds.
None of this goes through the host mapper, which sorts, de-overlaps and drops what the kernels return before any PAF is printed.

Wall time on one MI355X (profiles/map_windows_tests.txt): this file alone 8.2 s; the whole `pytest -m gpu` run 847 s on the parent
commit and 858 s with this file in it."""
import contextlib
import functools

import numpy as np
import pytest

from tests import map_crafted as MC
from tests import map_model as MM
from tests import oracle_lib as O
from tests.test_gpu_kernels import _all_seed_query, _index_from_sets
from tests.test_map_sparse_index_spec import _random_query, _rule_ids

pytestmark = pytest.mark.gpu

_TINY = (np.frombuffer(b"ACGT" * 30, dtype=np.uint8), np.array([0, 120], dtype=np.int64))
KEYS = ("window", "target", "off", "match_a", "match_b")


@contextlib.contextmanager
def _fresh():
    """A fresh context with a read set resident (contexts that borrow from it need one), closed whatever happens."""
    from downpore_amd import Context
    ctx = Context(0)
    try:
        ctx.upload_reads(*_TINY)
        yield ctx
    finally:
        ctx.close()


# ---- an index in any layout ---------------------------------------------------------------------------------------------------

def _flat(chunks):
    segs = np.concatenate([np.asarray(c, dtype=np.int32) for c in chunks])
    offs = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype(np.int64)
    return segs, offs


def shard_bounds(M, n):
    """n shards of whole 64-chunk words, as the mapper deals them"""
    per = (((M + n - 1) // n) + 63) // 64 * 64
    b = list(range(0, M, per)) + [M]
    assert len(b) == n + 1, (M, n, b)
    return b


class Built:
    """The index of `chunks` (flat segments + offsets) on the device: layout "dense" / "sparse" / "borrowed" (a sparse index read by
    a context made with dp_ctx_create_shared), whole (bounds = [0, M]) or in shards of whole 64-chunk words, every shard a context
    of its own that knows the sets' global windows (dp_index_meta combined into dp_index_set_global as the header prescribes)."""

    def __init__(self, k, seed_kmers, segs, offs, layout="dense", bounds=None):
        from downpore_amd import Context
        self.k, self.M = k, len(offs) - 1
        self.bounds = bounds or [0, self.M]
        self.all, self.shards = [], []
        seeds = np.ascontiguousarray(seed_kmers, dtype=np.uint32)
        nseeds = ((offs[1:] - offs[:-1]) // 2).astype(np.uint32)
        try:
            glob = np.tile(np.array([0, 1, 0, 1], dtype=np.uint32), (len(seeds), 1))  # NewIntSet(): count 0, start 1, end 0
            for lo, hi in zip(self.bounds[:-1], self.bounds[1:]):
                assert lo % 64 == 0
                ctx = Context(0)
                self.all.append(ctx)
                ctx.upload_reads(*_TINY)
                ctx.round_begin(k, seeds)
                s0 = int(offs[lo])
                ctx.import_segments(segs[s0:int(offs[hi])])
                build = ctx.index_build if layout == "dense" else ctx.index_build_sparse
                build((offs[lo:hi] - s0).astype(np.uint64), nseeds[lo:hi])
                if len(self.bounds) > 2:
                    m = ctx.index_meta().astype(np.int64)
                    nz = m[:, 0] > 0
                    st, en = m[:, 1] + lo // 64, m[:, 2] + lo // 64
                    new, more = nz & (glob[:, 0] == 0), nz & (glob[:, 0] > 0)
                    glob[new, 1], glob[new, 2] = st[new], en[new]
                    glob[more, 1] = np.minimum(glob[more, 1], st[more])
                    glob[more, 2] = np.maximum(glob[more, 2], en[more])
                    glob[nz, 0] += m[nz, 0].astype(np.uint32)
                    glob[nz, 3] = glob[nz, 2] + 1
                use = ctx
                if layout == "borrowed":
                    use = Context(0, shared_from=ctx)
                    self.all.append(use)
                    use.round_begin(k, seeds)
                    use.index_borrow(ctx)
                    info = use.index_info()
                    assert info["layout"] == "sparse" and info["borrowed"], info
                self.shards.append((use, lo, hi))
            if len(self.bounds) > 2:
                for ctx, lo, hi in self.shards:
                    ctx.index_set_global(glob, lo // 64, self.M)
        except Exception:
            self.close()
            raise

    def close(self):
        for ctx in reversed(self.all):  # (borrowers before the contexts they borrow from)
            ctx.close()
        self.all = []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def candidates(self, w_segs, w_off):
        """dp_query_candidates on every shard -> [(lo, hi, result)]"""
        return [(lo, hi, ctx.query_candidates(w_segs, w_off, 0.25)) for ctx, lo, hi in self.shards]

    def map(self, w_segs, w_off, w_len, sizes=None, calls=None):
        """dp_map_windows (whole index) or dp_map_windows_shard (phase 0 over the shards in order, then phase 1, thresholds from -1,
        targets shifted by the shard's first chunk, a window's chains concatenated in call order) over the window pairs, in calls of
        sizes[i] pairs (default: one call).  calls (a list): every device call's (shard, phase, n_chains, n_ints) is appended."""
        n_pairs = (len(w_off) - 1) // 2
        sizes = list(sizes or [n_pairs])
        assert sum(sizes) == n_pairs
        parts, p0 = [], 0
        for bi, np_ in enumerate(sizes):
            a, b = 2 * p0, 2 * (p0 + np_)
            ws = w_segs[int(w_off[a]):int(w_off[b])]
            wo = (w_off[a:b + 1] - w_off[a]).astype(np.uint64)
            wl = w_len[a:b]
            if len(self.shards) == 1:
                out = self.shards[0][0].map_windows(ws, wo, wl, self.k)
                if calls is not None:
                    calls.append((0, 2, len(out["window"]), len(out["match_a"])))
                outs = [out]
            else:
                thr = np.full(2 * np_, -1, dtype=np.int32)
                outs = []
                for phase in (0, 1):
                    if phase == 1 and bi % 2 == 1:  # (a foreign query stage between the passes: the reverse pass must not reuse the forward one's)
                        for ctx, lo, hi in self.shards:
                            ctx.query_candidates(ws[:int(wo[2])], wo[:3], 0.25)
                    for si, (ctx, lo, hi) in enumerate(self.shards):
                        out, thr = ctx.map_windows_shard(ws, wo, wl, self.k, phase, thr)
                        assert np.all(out["window"] % 2 == phase)
                        out["target"] = out["target"] + lo
                        if calls is not None:
                            calls.append((si, phase, len(out["window"]), len(out["match_a"])))
                        outs.append(out)
            parts.append(_concat(outs, 2 * p0, sort=len(outs) > 1))
            p0 += np_
        return _concat(parts, 0, sort=False)


def _concat(outs, window_base, sort):
    window = np.concatenate([o["window"].astype(np.int64) for o in outs]) + window_base
    target = np.concatenate([o["target"].astype(np.int64) for o in outs])
    lens = np.concatenate([np.diff(o["off"].astype(np.int64)) for o in outs])
    starts, at = [], 0
    for o in outs:
        starts.append(o["off"][:-1].astype(np.int64) + at)
        at += len(o["match_a"])
    starts = np.concatenate(starts)
    ma = np.concatenate([o["match_a"].astype(np.int64) for o in outs])
    mb = np.concatenate([o["match_b"].astype(np.int64) for o in outs])
    if sort and len(window):
        order = np.argsort(window, kind="stable")
        window, target, lens, starts = window[order], target[order], lens[order], starts[order]
        new_off = np.concatenate([[0], np.cumsum(lens)])
        idx = np.repeat(starts - new_off[:-1], lens) + np.arange(int(lens.sum()))
        ma, mb = ma[idx], mb[idx]
    return dict(window=window, target=target, off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), match_a=ma, match_b=mb)


def _assert_same(got, want, what):
    for key in KEYS:
        g, w = np.asarray(got[key], dtype=np.int64), np.asarray(want[key], dtype=np.int64)
        if not np.array_equal(g, w):
            n = min(len(g), len(w))
            d = np.nonzero(g[:n] != w[:n])[0]
            at = int(d[0]) if len(d) else n
            raise AssertionError("%s: %s differs at %d (got %d entries, want %d): got %s want %s" % (
                what, key, at, len(g), len(w), g[at:at + 6].tolist(), w[at:at + 6].tolist()))


def _check_candidates(built, w_segs, w_off, want_lists, what):
    """every shard's candidate lists = the matching slice of the global lists, shard-local; meta = {sets, minCount, 0} wherever
    Matches() asked GetSharedIDs at all"""
    for lo, hi, res in built.candidates(w_segs, w_off):
        co = res["cand_off"].astype(np.int64)
        assert len(co) == len(want_lists) + 1
        want = [np.asarray([x - lo for x in w if lo <= x < hi], dtype=np.int64) for w in want_lists]
        assert np.array_equal(co, np.concatenate([[0], np.cumsum([len(w) for w in want])])), (what, lo, hi)
        assert np.array_equal(res["cand"].astype(np.int64), np.concatenate(want + [np.zeros(0, dtype=np.int64)])), (what, lo, hi)
        assert not res["meta"][:, 2].any(), (what, "status")


# ---- a. trace replay ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _traced(name):
    """the traced run of input `name` as dp_map_windows takes and returns it"""
    run = MC.traced_run(name)
    isegs, ioffs = run.trace("indexedSegments")
    w_segs, w_off, w_len, cands = [], [0], [], []
    window, target, lens, ma, mb = [], [], [], [], []
    for c in range(run.n_calls):
        tc = run.call(c)
        for s, key in enumerate(("fwdSegments", "rcSegments")):
            w_segs.append(tc[key].astype(np.int32))
            w_off.append(w_off[-1] + len(tc[key]))
            w_len.append(int(tc["lengths"][s]))
        cands += [tc["candidates"].tolist(), tc["rcCandidates"].tolist()]
        a, ao = tc["matchA"]
        b, _ = tc["matchB"]
        window.append(2 * c + tc["chainStrand"])
        target.append(tc["chainTarget"])
        lens.append(np.diff(ao))
        ma.append(a)
        mb.append(b)
    want = dict(window=np.concatenate(window), target=np.concatenate(target),
                off=np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64), match_a=np.concatenate(ma),
                match_b=np.concatenate(mb))
    return dict(k=run.k, seeds=run.trace("seedKmers"), segs=isegs.astype(np.int32), offs=ioffs, w_segs=np.concatenate(w_segs),
                w_off=np.array(w_off, dtype=np.uint64), w_len=np.array(w_len, dtype=np.uint32), cands=cands, want=want)


def _uneven(n_pairs):
    sizes, left, i = [], n_pairs, 0
    pattern = [1, 7, 64, 3, 29, 2, 101]
    while left:
        s = min(left, pattern[i % len(pattern)])
        sizes.append(s)
        left -= s
        i += 1
    return sizes


LAYOUTS = [("dense", 1), ("sparse", 1), ("borrowed", 1), ("one_lane", 1), ("dense", 2), ("sparse", 2), ("dense", 3), ("sparse", 3)]


@pytest.mark.parametrize("layout,shards", LAYOUTS, ids=["%s-%d" % ls for ls in LAYOUTS])
@pytest.mark.parametrize("name", sorted(MC.TRACED))
def test_trace_replay(monkeypatch, name, layout, shards):
    """The oracle's traced windows through dp_map_windows(_shard) on an index over the traced chunks: the chains of the trace -
    window, target, off, match_a, match_b - from one call and from calls of uneven sizes, and dp_query_candidates = the traced
    matchingIndices / matchingRCIndices (per shard: their slice, shard-local)."""
    t = _traced(name)
    assert len(t["want"]["window"]) >= 300
    if layout == "one_lane":
        monkeypatch.setenv("DP_TUNE", "map_one_lane=1")
        layout = "dense"
    M = len(t["offs"]) - 1
    what = "%s %s x%d" % (name, layout, shards)
    with Built(t["k"], t["seeds"], t["segs"], t["offs"], layout, shard_bounds(M, shards)) as built:
        assert len(built.shards) == shards
        _check_candidates(built, t["w_segs"], t["w_off"], t["cands"], what)
        _assert_same(built.map(t["w_segs"], t["w_off"], t["w_len"]), t["want"], what + ", one call")
        _assert_same(built.map(t["w_segs"], t["w_off"], t["w_len"], _uneven(len(t["w_len"]) // 2)), t["want"], what + ", uneven calls")


# ---- b. the ladder tests on either layout through dp_query_candidates --------------------------------------------------------------

BUILDS = ["index_build", "index_build_sparse"]


@pytest.mark.parametrize("build", BUILDS)
def test_candidates_reference_test2sharedids_vectors(build):
    """util/bitset_test.go:38-161 (20 sets over 500 ids with multiplicities 16/8/4/2, minCount 16, 15, 8, 4, 2)"""
    counts = np.zeros(500, dtype=np.int64)
    for i in range(500):
        counts[i] = 16 if i % 7 == 0 else 8 if i % 5 == 0 else 4 if i % 3 == 0 else 2 if i % 2 == 0 else 0
    member = [[j < counts[i] for i in range(500)] for j in range(20)]
    qs, qo = _all_seed_query(20)
    with _fresh() as ctx:
        _index_from_sets(ctx, 10, member, build)
        assert ctx.index_info()["layout"] == ("sparse" if build == "index_build_sparse" else "dense")
        for hf, min_count, expect in ((0.8, 16, 16), (0.75, 15, 16), (0.4, 8, 8), (0.2, 4, 4), (0.1, 2, 2)):
            out = ctx.query_candidates(qs, qo, hf)
            assert out["cand"].tolist() == [i for i in range(500) if counts[i] >= expect], (min_count,)
            assert out["meta"].tolist() == [[20, min_count, 0]]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_candidates_all_ladder_regimes_vs_oracle(seed, build):
    """test_matches_all_ladder_regimes_vs_oracle's sets and hit fractions (every threshold regime, uneven set windows)"""
    rng = np.random.default_rng(seed)
    S, M = 48, 700
    dens = rng.choice([0.05, 0.2, 0.45, 0.7], size=M)
    member = [[bool(rng.random() < dens[i]) for i in range(M)] for _ in range(S)]
    for s in range(S):
        if s % 5 == 0:
            lo = int(rng.integers(0, M - 150))
            member[s] = [member[s][i] and lo <= i < lo + 150 for i in range(M)]
    qs, qo = _all_seed_query(S)
    with _fresh() as ctx:
        sets = _index_from_sets(ctx, 10, member, build)
        for hf in (0.01, 0.03, 0.1, 0.16, 0.2, 0.24, 0.27, 0.32, 0.36, 0.41, 0.5, 0.52, 0.62, 0.8):
            min_count = int(hf * S + 0.5)
            out = ctx.query_candidates(qs, qo, hf)
            assert out["cand"].tolist() == [int(x) for x in O.shared_ids(sets, min_count, True)], (seed, hf, min_count)
            assert out["meta"].tolist() == [[S, min_count, 0]]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("S", [300, 511, 513, 900])
def test_candidates_exact_count_regime_with_long_queries(S, build):
    """test_matches_exact_count_regime_with_long_queries' sets (sequences that hold more than 255 of the query's seeds; more than 512
    sets: the BIG tier of the query stage)"""
    rng = np.random.default_rng(S)
    M = 400
    dens = rng.choice([0.02, 0.3, 0.6, 0.85, 0.97, 1.0], size=M)
    member = [[bool(rng.random() < dens[i]) for i in range(M)] for _ in range(S)]
    assert max(sum(member[s][i] for s in range(S)) for i in range(M)) > 255
    qs, qo = _all_seed_query(S)
    with _fresh() as ctx:
        sets = _index_from_sets(ctx, 10, member, build)
        for hf in (0.005, 0.012, 0.016, 0.09, 0.4, 0.8, 0.86, 0.99):
            min_count = int(hf * S + 0.5)
            want = [int(x) for x in O.shared_ids(sets, min_count, True)]
            assert len(want) > 0
            out = ctx.query_candidates(qs, qo, hf)
            assert out["cand"].tolist() == want, (S, hf, min_count)
            assert out["meta"].tolist() == [[S, min_count, 0]]


def _index_of_queries(ctx, k, queries, M, build):
    """One index for many independent queries: query j's sets become seeds of their own (in set order), all over the same M
    sequences; one more seed held by every sequence keeps every row non-empty and is in no query (Matches() drops a set that holds
    every sequence).  -> per query (segments, offsets)"""
    rows = [[] for _ in range(M)]
    seed, out = 0, []
    for members in queries:
        q = [1]
        for m in members:
            for x in m:
                rows[int(x)].append(seed)
            q += [seed, 1]
            seed += 1
        out.append((np.array(q, dtype=np.int32), np.array([0, len(q)], dtype=np.uint64)))
    for r in rows:
        r.append(seed)
    ctx.round_begin(k, np.arange(seed + 1, dtype=np.uint32) * 3 + 1)
    segs, offs = _flat([MC.seg_of(r, gap=2) for r in rows])
    ctx.import_segments(segs)
    getattr(ctx, build)(offs[:-1].astype(np.uint64), ((offs[1:] - offs[:-1]) // 2).astype(np.uint32))
    return out


@pytest.mark.parametrize("build", BUILDS)
def test_candidates_where_the_p7_term_decides(build):
    """Queries of tests/test_map_sparse_index_spec.py's generator with aim_p7: 16-ladder queries with ids planted in exactly minCount
    sets that include gather position 7 and none of 0 - 6, where step 8 of the reference's ladder omits its ORQ.  The device's
    candidates = the oracle's GetSharedIDs = the Python statement of the count rule (_rule_ids); in at least 20 of the queries the
    p7 term decides an id."""
    rng = np.random.default_rng(20261017)
    queries = [_random_query(rng, aim_p7=True) for _ in range(60)]
    wants, decided = [], 0
    for members, mc in queries:
        sets = []
        for m in members:
            s = O.IntSet()
            for x in m:
                s.add(int(x))
            sets.append(s)
        want = [int(x) for x in O.shared_ids(sets, mc, True)]
        rule, d = _rule_ids(members, mc)
        assert rule == want
        decided += d > 0
        wants.append(want)
    assert decided >= 20, decided
    with _fresh() as ctx:
        qsegs = _index_of_queries(ctx, 10, [m for m, _ in queries], 3000, build)
        for (members, mc), (qs, qo), want in zip(queries, qsegs, wants):
            hf = mc / len(members)
            assert int(hf * len(members) + 0.5) == mc
            out = ctx.query_candidates(qs, qo, hf)
            assert out["meta"].tolist() == [[len(members), mc, 0]]
            assert out["cand"].tolist() == want, (len(members), mc)
    print("p7 decided in %d of %d queries" % (decided, len(queries)))


def _tiling_queries():
    """Sets over 20 000 ids whose members sit on both sides of the sparse query's 8 192-id tiles - counted from id 0 and from the
    first populated word of queries that start elsewhere (the tile start jumps to it) - with long empty stretches in between, empty
    sets and sets confined to one word; every ladder regime."""
    rng = np.random.default_rng(8192)
    M = 20000
    queries = []
    for first in (0, 130, 8191, 4100):
        w0 = first & ~63
        hot = sorted(set(x for x in (first, 8191, 8192, 8193, 16383, 16384, w0 + 8191, w0 + 8192, w0 + 8193, w0 + 16383, w0 + 16384,
                                     19999) if first <= x < M))
        for n, mc in ((8, 2), (24, 6), (40, 10), (40, 14), (80, 20), (120, 30)):
            share = {x: float(rng.choice([0.15, 0.3, 0.6, 0.9])) for x in hot}  # (ids on both sides of every threshold)
            members = []
            for j in range(n):
                if j % 11 == 3:
                    members.append(set())                                                  # an empty set
                elif j % 11 == 5:
                    members.append(set(int(x) for x in rng.integers(8192, 8256, size=9)))   # confined to one word
                else:
                    m = set(x for x in hot if rng.random() < share[x])
                    m |= set(int(x) for x in rng.integers(first, M, size=int(rng.integers(0, 6))))
                    members.append(m)
            members[0].add(first)
            queries.append(([np.array(sorted(m), dtype=np.int64) for m in members], mc))
    return M, queries


@pytest.mark.parametrize("build", BUILDS)
def test_candidates_across_sparse_tiles_and_in_shards(build):
    """20 000 chunks: the whole index, and shards whose word ranges start inside the sets' windows (word bases 127, 128, 256) -
    shard-local candidates = the slice of the oracle's global list."""
    M, queries = _tiling_queries()
    wants = []
    for members, mc in queries:
        sets = []
        for m in members:
            s = O.IntSet()
            for x in reversed(m):  # IndexSequences adds in descending sequence order
                s.add(int(x))
            sets.append(s)
        wants.append([int(x) for x in O.shared_ids(sets, mc, True)])
    assert sum(len(w) > 0 for w in wants) > len(wants) // 2
    crossing = sum(1 for w in wants if any(x >= 8192 for x in w) and any(x < 8192 for x in w))
    assert crossing >= 4, crossing
    # the same rows as chunks: one index, every query's sets seeds of their own
    rows = [[] for _ in range(M)]
    seed, qsegs = 0, []
    for members, mc in queries:
        q = [1]
        for m in members:
            for x in m:
                rows[int(x)].append(seed)
            q += [seed, 1]
            seed += 1
        qsegs.append((np.array(q, dtype=np.int32), np.array([0, len(q)], dtype=np.uint64), mc / len(members)))
    for r in rows:
        r.append(seed)  # (held by every chunk: in no query)
    segs, offs = _flat([MC.seg_of(r, gap=2) for r in rows])
    kmers = np.arange(seed + 1, dtype=np.uint32) * 3 + 1
    layout = "sparse" if build == "index_build_sparse" else "dense"
    for bounds in ([0, M], [0, 8128, M], [0, 8192, 16384, M]):
        with Built(10, kmers, segs, offs, layout, bounds) as built:
            for (qs, qo, hf), (members, mc), want in zip(qsegs, queries, wants):
                assert int(hf * len(members) + 0.5) == mc
                for ctx, lo, hi in built.shards:
                    out = ctx.query_candidates(qs, qo, hf)
                    assert out["meta"].tolist() == [[len(members), mc, 0]]
                    assert out["cand"].tolist() == [x - lo for x in want if lo <= x < hi], (bounds, lo, mc, len(members))


# ---- c. relaunch paths against the model ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _crafted(case):
    c = MC.build(case)
    want = MM.map_windows(MM.Index(c["chunks"], c["n_seeds"]), c["w_segs"], c["w_off"], c["w_len"], c["k"])
    assert want["distinct"] == c["distinct"]  # (the model ran once per distinct window pair)
    segs, offs = _flat(c["chunks"])
    return c, want, segs, offs


@pytest.mark.parametrize("layout", ["dense", "sparse"])
@pytest.mark.parametrize("shards", [1, 2], ids=["whole", "two_shards"])
@pytest.mark.parametrize("case", ["big", "records", "ints"])
def test_relaunch_paths_against_model(case, shards, layout):
    """dp_map_windows / dp_map_windows_shard on fresh contexts (65 536 records, 2 097 152 chain ints to start with) over the crafted
    batches of tests/map_crafted.py.  What came back proves that the call launched again: a chain longer than the 256 reduced
    seeds the ordinary kernel holds (the BIG variant ran), more chains than the first launch had records for, more chain ints than
    it had room for - in the sharded runs inside ONE call, the forward pass of the first shard.  A relaunch that starts from
    thresholds the launch before it has raised loses the chain of the ratchet-sensitive pair's first target (t0: count 10, below
    the 32 its neighbour t1 ratchets to)."""
    c, want, segs, offs = _crafted(case)
    bounds = [0, len(c["chunks"])] if shards == 1 else [0, c["split"], len(c["chunks"])]
    calls = []
    with Built(c["k"], np.arange(c["n_seeds"], dtype=np.uint32) * 3 + 1, segs, offs, layout, bounds) as built:
        got = built.map(c["w_segs"], c["w_off"], c["w_len"], calls=calls)
    shard, phase, n_chains, n_ints = calls[0]  # the whole index's only call / the first shard's forward pass
    longest = int(np.diff(got["off"]).max())
    print("%s %s x%d: first call %d chains, %d ints; longest chain %d; calls %s" % (case, layout, shards, n_chains, n_ints, longest, calls))
    if case == "big":
        assert longest > 256
    elif case == "records":
        assert n_chains > 65536 and n_ints <= 2097152
    else:
        assert n_ints > 2097152 and n_chains <= 65536
    w = 2 * c["sensitive_pair"]
    mine = got["target"][got["window"] == w].tolist()
    assert MC.T0 in mine, "the ratchet-sensitive pair lost t0's chain (its targets: %s, want %s): the relaunch started from raised thresholds" % (
        mine, want["target"][want["window"] == w].tolist())
    _assert_same(got, want, "%s %s x%d" % (case, layout, shards))
