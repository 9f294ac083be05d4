"""Crafted inputs of the chaining stage tests (tests/test_chain_cases_cpu.py on the CPU, tests/test_gpu_chain_stage.py on the device):
indexed sequences and queries as segment arrays [gap, seed id, gap, ..., gap], placed on either side of every capacity that picks a
path in dp_overlap.hip, the oracle's answer for each (oracle_lib.find_overlaps_segments) and the path the capacities predict for every
(query, candidate) pair.  Test infrastructure only.

A Case is one dp_find_overlaps call: an index, its queries, k, hitFraction, maxLength.  Its `claims` name single pairs and say what the
oracle's profile of that pair must show - the CPU test holds every case to them, so that a case cannot drift off the boundary its name
states without a test noticing.
"""
import types

import numpy as np

from tests import oracle_lib as O

#: Capacities of the chaining stage, from the structs and constants of downpore_amd/csrc/dp_overlap.hip.  Ints are segment ints
#: (a sequence of n seeds has 2 n + 1).
CAPS = dict(
    # struct CSlim: the layout of walk 0 and of the proposal passes (chain_spec_kernel)
    SLIM_ACAP=256,      # enum ACAP: query ints staged -> at most 127 query seeds
    SLIM_RSEEDS=64,     # enum RSEEDS: kept seeds of a
    SLIM_EVN=128,       # enum EVN: b events
    SLIM_ROWS=32,       # enum ROWS: open chains
    SLIM_COLN=64,       # enum COLN: links of a chain
    # struct CWave: the full layout (final walk; walk 0 when a tier is forced or there are no passes)
    C_ACAP=512,         # query ints staged -> at most 255 query seeds; beyond: one lane, operands in global memory (tier 3)
    C_BCAP=1056,        # target ints staged (both layouts) -> at most 527 target seeds; beyond: tier 3
    RSEEDS=255,         # enum RSEEDS: kept seeds the staged prepareInitial holds (a query of 255 seeds cannot keep more)
    REG_ALEN=64,        # chain_pair: aLen <= 64 tries the reg tier
    C_REV=256,          # enum EVN of CWave: b events of the reg tier
    REG_ROWS=64,        # enum ROWS of CWave: open chains of the reg tier
    C_LNODES=512,       # chain links of the lds tier kept in LDS; later ones live in the wave's slice of the global pool
    C_NODES=65536,      # links of one pair in that slice (one-lane path: links in use, dropped chains are recycled)
    C_QSW=256,          # query bitset words staged in LDS -> rounds of up to 16 384 seeds
    PREFILTER_SEEDS=64, # chain_walk_kernel / chain_spec_kernel: a staged query of <= 64 seeds probes the target's set seed by seed
    LDS_MAXLENGTH=510,  # chain_pool_stride: an aligner with maxLength above it keeps the one-lane path's reduced a in the spill area
    # the reference's own limits (seeds/alignment.go:298-302), which the device reports as DP_ERR_CAPACITY bits 1, 2, 4
    OPEN=500, RESULTS=500, POOL=10000,
)
ERR_BITS = {"reduced buffer": 1, "state pool": 2, "results": 4, "nodes": 8}

# path bits of dp_debug_chain_paths (include/downpore_hip.h)
P_TIER, P_SLIM, P_CHAINED, P_MARKED = 3, 4, 8, 16
K_WALK0, K_RESOLVE0, K_FINAL = 1, 2, 15


def kernel_of(path):
    return (int(path) >> 8) & 15


def seq(seeds, gaps=10, first=0, last=0):
    """[first, s0, g1, s1, ..., last]; gaps: one value or the list of the len(seeds) - 1 gaps between the seeds"""
    seeds = [int(s) for s in seeds]
    if np.isscalar(gaps):
        gaps = [gaps] * (len(seeds) - 1)
    assert len(gaps) == len(seeds) - 1
    out = [first]
    for i, s in enumerate(seeds):
        out += [s, gaps[i] if i + 1 < len(seeds) else last]
    return out


class _Builder:
    def __init__(self, name, k=10, hf=0.25, max_length=500, error=0):
        self.c = types.SimpleNamespace(name=name, k=k, hf=hf, max_length=max_length, error=error, index=[], queries=[], claims=[],
                                       n_seed_ids=0)
        self.next_id = 0

    def ids(self, n):
        """n fresh seed ids"""
        a = list(range(self.next_id, self.next_id + n))
        self.next_id += n
        return a

    def target(self, segs):
        self.c.index.append(list(segs))
        return len(self.c.index) - 1

    def query(self, segs):
        self.c.queries.append(list(segs))
        return len(self.c.queries) - 1

    def pair(self, label, a, b, **claim):
        """query a against its own target b; claim: what the oracle's row of the pair must show (PAIR_COLS names; a value, or
        ("ge", v))"""
        q, t = self.query(a), self.target(b)
        self.c.claims.append((label, q, t, claim))
        return q, t

    def done(self, n_seed_ids=None, decoys=3):
        for _ in range(decoys):  # (sequences no query shares a seed with: no seed of a query is in every sequence, seeds.go:343)
            self.target(seq(self.ids(8)))
        self.c.n_seed_ids = n_seed_ids or ((self.next_id + 63) // 64 * 64)
        assert self.next_id <= self.c.n_seed_ids
        return self.c


def _mm(hf, n_seeds):
    return int(hf * n_seeds + 0.5)


# --------------------------------------------------------------------------------------------------------------------- the cases
def _case_sizes():
    """query seeds, kept seeds, target ints, b events, open chains, chain links: one pair on either side of each capacity"""
    B = _Builder("sizes", hf=0.1)
    # query seeds: 64 | 65 the prefilter by seed, 127 | 128 CSlim::ACAP (256 ints hold 127 seeds; 129 as well), 255 | 256 C_ACAP (and 257)
    for n in (64, 65, 127, 128, 129, 255, 256, 257):
        s = B.ids(n)
        B.pair("qseeds_%d" % n, seq(s), seq(s[:40]), aLen=40, kept=40)
    # kept seeds of a: 64 | 65, reg -> lds tier and the end of the slim layout
    for n, tag in ((64, "at"), (65, "over")):
        s = B.ids(100)
        B.pair("alen_64_%s" % tag, seq(s), seq(s[:n]), aLen=n, kept=n)
    # target ints 1055 | 1057 around C_BCAP: 527 and 528 seeds, the query's 40 first
    for n, tag in ((527, "at"), (528, "over")):
        s = B.ids(40)
        B.pair("tgt_1056_%s" % tag, seq(s), seq(s + B.ids(n - 40)), aLen=40, kept=40)
    # b events: the query's 40 seeds in order (one chain), then - far behind - two seeds of the query's tail, which hold no initial
    # position (aPos > maxAIndex), over and over: events that neither start nor extend anything
    for n in (128, 129, 256, 257):
        s = B.ids(40)
        fill = [s[38 + (i & 1)] for i in range(n - 40)]
        B.pair("bev_%d" % n, seq(s), seq(s + fill, gaps=[10] * 39 + [3000] + [10] * (n - 41)), bEvents=n, aLen=40, peakOpen=1, kept=40)
    # open chains: n times the query's first seed X (a seed foreign to the query between two of them keeps the duplicate rule away) opens
    # n chains at the one initial position that holds X; the query's gaps are wide, so none of them runs off its end; then the rest of
    # the query in order
    for n in (32, 33, 64, 65):
        s = B.ids(40)
        z = B.ids(1)[0]
        xs = []
        for _ in range(n):
            xs += [s[0], z]
        B.pair("open_%d" % n, seq(s, gaps=100), seq(xs + s[1:], gaps=[0] * (2 * n - 1) + [100] * 39), peakOpen=n, aLen=40)
    # a chain of 64 and of 65 links with more than 64 kept seeds (lds tier): the query's last six seeds first, far in front
    for n in (64, 65):
        s = B.ids(n + 6)
        B.pair("chain_%d" % n, seq(s), seq(s[n:] + s[:n], gaps=[10] * 5 + [5000] + [10] * (n - 1)), aLen=n + 6, kept=n, longestChain=n)
    return B.done()


def _case_links():
    """more links than C_LNODES: X a1 X a2 .. X a9 against X z X z .. - every X of the target opens a chain at every X of the query -
    and, far behind, four of the a's (the prefilter wants minMatches = 5 distinct shared seeds)"""
    B = _Builder("links", hf=0.25)
    s = B.ids(9)
    x, z = B.ids(2)
    a, b = [], []
    for i in range(9):
        a += [x, s[i]]
    for i in range(60):
        b += [x, z]
    B.pair("links_over_lnodes", seq(a), seq(b + s[:4], gaps=[10] * 119 + [4000] + [10] * 3), popped=("ge", CAPS["C_LNODES"] + 1),
           peakOpen=("ge", CAPS["REG_ROWS"] + 1), mm=5)
    return B.done()


def _case_kept_wide():
    """maxLength 1500: 254 | 255 kept seeds are staged (lds tier); a query of 256 seeds is not (one lane); the reduced-buffer limit
    of this aligner (749 kept seeds fit) on its near side"""
    B = _Builder("kept_wide", hf=0.25, max_length=1500)
    for n, nq in ((254, 255), (255, 255), (256, 256)):
        s = B.ids(nq)
        B.pair("alen_%d" % n, seq(s), seq(s[:n]), aLen=n, kept=n)
    s = B.ids(760)
    B.pair("redbuf1500_at", seq(s), seq(s[:749]), aLen=749, kept=749)
    return B.done()


def _case_redbuf(name, max_length, n_query, n_kept, error):
    B = _Builder(name, hf=0.25, max_length=max_length, error=error)
    s = B.ids(n_query)
    B.pair(name, seq(s), seq(s[:n_kept]), **({} if error else dict(aLen=n_kept, kept=n_kept)))
    return B.done()


def _case_results(name, n, filler=0):
    """results overflow: a query of five seeds 50 bases long (minMatches 1) and a target that alternates its first two seeds, 1 000
    bases apart: every event drops the chain the previous one opened - it has run off the query's end - into results, and opens one.
    500 events fill results exactly, the 501st is the reference's panic.  Up to 527 target seeds the pair is staged (lds tier: more
    than 256 events); filler seeds behind them make it a one-lane pair."""
    B = _Builder(name, hf=0.25, error=ERR_BITS["results"] if n > CAPS["RESULTS"] else 0)
    s = B.ids(5)
    claim = dict(bEvents=n, peakOpen=1) if n > CAPS["RESULTS"] else dict(bEvents=n, resultsSize=CAPS["RESULTS"], kept=1)
    B.pair(name, seq(s, gaps=0), seq([s[i & 1] for i in range(n)] + B.ids(filler), gaps=1000), **claim)
    return B.done()


def _case_pool(name, n):
    """state pool: a query of 249 kept seeds (hitFraction 0.9: minMatches 224, 26 initial positions) against its own seeds over and
    over.  Every copy is one chain of 249 links that ends in results and stays live: 40 copies and 223 seeds more - too few to
    start another chain - finish with 9 986 live states; one seed more starts the chain that asks for the 10 001st."""
    B = _Builder(name, hf=0.9, error=ERR_BITS["state pool"] if n > 10183 else 0)
    s = B.ids(249)
    claim = {} if n > 10183 else dict(peakLive=("ge", CAPS["POOL"] - 20), resultsSize=40, kept=249)
    B.pair(name, seq(s), seq((s * (n // 249 + 1))[:n]), **claim)
    return B.done()


def _case_nodes(name, n_target):
    """The device's own limit (C_NODES links per pair) where the reference has none: four seeds over and over on both sides, the
    target's seeds 1 000 bases apart and the query 120 bases long - every event drops the chain opened last (it runs off the
    query's end) and opens one.  65 535 target seeds make 66 032 links, 65 000 make 65 497; the reference finishes both."""
    B = _Builder(name, hf=0.25)
    s = B.ids(4)
    B.pair(name, seq(s * 3, gaps=0), seq((s * (n_target // 4 + 1))[:n_target], gaps=1000), bEvents=n_target, peakOpen=500,
           popped=("ge", CAPS["C_NODES"] + 1) if n_target == 65535 else n_target + 497, kept=0)
    return B.done()


def _gap_pair(B, label, k, bgap, agap):
    """twelve seeds on both sides, gap 30 between them; in front of seed 6 the target has bgap and the query agap"""
    s = B.ids(12)
    ga, gb = [30] * 11, [30] * 11
    ga[5], gb[5] = agap, bgap
    return B.pair(label, seq(s, gaps=ga), seq(s, gaps=gb))


def gap_range(gap, k):
    """seeds/alignment.go:411-424 (Go's division truncates toward zero)"""
    def div(a, b):
        return int(a / b) if a * b < 0 else a // b
    mn, mx = div(gap * 2, 3) - k, div(gap * 3, 2) + k + 1
    if mn < 0:
        return -k, max(mx, 0)
    if mx < 20:
        return 0, 20
    return mn, mx


def _case_perfect(k=10, name="perfect"):
    """what decides whether wave_chain_reg may take the perfect-chain shortcut"""
    B = _Builder(name, k=k, hf=0.25)
    if k == 10:
        for n in (1, 2):  # nE = 1, 2: a query of five seeds (minMatches 1) and a target that holds one or two of them
            s = B.ids(5)
            B.pair("ne_%d" % n, seq(s), seq(s[:n] + B.ids(3)), bEvents=n, kept=n)
        for n in (64, 65):
            s = B.ids(n)
            B.pair("ne_%d" % n, seq(s), seq(s), bEvents=n, kept=n, aLen=n)
        s = B.ids(20)  # event 0 holds a seed of the query's tail: no initial position (minMatches 5: positions 0 .. 15 are initial)
        B.pair("ev0_none", seq(s), seq([s[18]] + s, gaps=[400] + [10] * 19), bEvents=21, kept=20)
        s = B.ids(19)  # event 0's seed at two initial positions
        a = [s[0], s[1], s[0]] + s[2:]
        B.pair("ev0_two", seq(a), seq(a), bEvents=20)
        s = B.ids(19)  # a later event's seed at a second initial position
        a = s[:2] + s[2:6] + [s[1]] + s[6:]
        B.pair("second_start", seq(a), seq(a), bEvents=20)
        # the first event exactly at maxBIndex (a first event BEYOND it cannot reach the chaining: the prefilter wants minMatches
        # distinct shared seeds, every one of them an event, and an event beyond maxBIndex has fewer than minMatches seeds behind it)
        s = B.ids(20)
        B.pair("first_at_maxb", seq(s), seq(B.ids(30) + s[:5]), bEvents=5, kept=5)
        gaps = {"neg": 6, "plain": 30}
    else:
        gaps = {"clamp": 8}
    for branch, bgap in gaps.items():
        mn, mx = gap_range(bgap, k)
        assert (branch == "neg") == (mn == -k) and (branch == "clamp") == ((mn, mx) == (0, 20) and bgap * 3 // 2 + k + 1 < 20)
        for tag, agap in (("below", mn - 1), ("min", mn), ("max", mx), ("above", mx + 1)):
            _gap_pair(B, "gap_%s_%s" % (branch, tag), k, bgap, agap)
    return B.done()


def _case_dups():
    """the duplicate-seed rule (a seed equal to the previous kept one is dropped when it is the last seed or the next raw seed is
    the same): runs of 2, 3, 4 at the very start, the very end and across the 64-lane block boundary (seed indices 62 .. 66) of the
    query, of the target, of both.  Every query meets every target: the ratchet runs over 36 candidates."""
    B = _Builder("dups", hf=0.25)
    s = B.ids(80)
    r = B.ids(1)[0]

    def with_run(length, at):
        out = list(s)
        start = {"start": 0, "end": 80 - length, "b62": 62, "b63": 63}[at]
        for i in range(length):
            out[start + i] = r
        return out

    plain = list(s)
    plain[40] = r
    for length in (2, 3, 4):
        for at in ("start", "end", "b62", "b63"):
            run = with_run(length, at)
            tag = "run%d_%s" % (length, at)
            B.pair("a_" + tag, seq(run), seq(plain))
            B.pair("b_" + tag, seq(plain), seq(run))
            B.pair("ab_" + tag, seq(run), seq(run))
    return B.done()


def _case_ratchet():
    """candidates, in ascending id order, whose chains have 6, 10, 16, 25, 40 links (hitFraction 0.08 of 40 seeds: minMatches 3, then
    4, 6, 10, 16, 26): every proposal pass works with a value the next hit outdates"""
    B = _Builder("ratchet_steps", hf=0.08)
    s = B.ids(40)
    q = B.query(seq(s))
    for n in (6, 10, 16, 25, 40):
        t = B.target(seq(s[:n] + B.ids(4)))
        B.c.claims.append(("len_%d" % n, q, t, dict(kept=n)))
    return B.done()


def _case_ratchet_stale():
    """hitFraction 0.25.  Query A (30 seeds, minMatches 8): candidate 0 chains 14 (-> 9), candidate 1 chains 17 (-> 11), candidate 2 holds
    the query's seeds 20 .. 29 first and 0 .. 11 behind them: with minMatches 9 position 20 is an initial one and the chain of ten
    is results[0]; with the value in force, 11, it is cut off by maxAIndex and the chain of twelve is the answer.  Query B (32 seeds,
    minMatches 8): a chain of 12 (12 * 2 == 8 * 3: no ratchet), then one of 13, then one of 17 (-> 11), then a chain of 10, which
    the value in force refuses."""
    B = _Builder("ratchet_stale", hf=0.25)
    s = B.ids(30)
    q = B.query(seq(s))
    for label, t, claim in (("first_14", seq(s[:14] + B.ids(3)), dict(kept=14, mm=8)), ("second_17", seq(s[:17] + B.ids(3)), dict(kept=17, mm=9)),
                            ("late_start", seq(s[20:30] + s[:12], gaps=[10] * 9 + [600] + [10] * 11), dict(kept=12, mm=11))):
        B.c.claims.append((label, q, B.target(t), claim))
    s = B.ids(32)
    q = B.query(seq(s))
    for label, t, claim in (("exact_12", seq(s[:12] + B.ids(3)), dict(kept=12, mm=8)), ("above_13", seq(s[:13] + B.ids(3)), dict(kept=13, mm=8)),
                            ("then_17", seq(s[:17] + B.ids(3)), dict(kept=17, mm=8)), ("refused_10", seq(s[:10] + B.ids(3)), dict(kept=0, mm=11, chained=0))):
        B.c.claims.append((label, q, B.target(t), claim))
    return B.done()


#: (candidates, rank of the first hit) of the queries of the many-candidates case
MANY = ((65, 0), (65, 63), (65, 64), (128, 63), (128, 127), (130, 0), (130, 64), (130, 127))


def _case_many(copies=1, name="many"):
    """more than 64 candidates for one query (chain_resolve_kernel replays 64 pairs a step).  A query of 40 seeds, minMatches 10.
    Candidates before the first hit hold twelve of its seeds in reverse order (chained, no chain of ten); the first hit holds all
    40 in order (minMatches -> 26); behind it candidates hold 30 in order (hits) - except ranks 63, 64, 127, 128, which hold twelve:
    they fail the prefilter on either side of a step boundary.  copies > 1: the same queries several times over (the scratch
    columns of the stage outgrow their first size)."""
    B = _Builder(name, hf=0.25)
    for n, first in MANY:
        s = B.ids(40)
        qs = [B.query(seq(s)) for _ in range(copies)]
        for rank in range(n):
            if rank < first:
                t = seq(s[11::-1] + B.ids(2))
                claim = dict(chained=1, kept=0, mm=10)
            elif rank == first:
                t = seq(s)
                claim = dict(chained=1, kept=40, mm=10)
            elif rank in (63, 64, 127, 128):
                t = seq(s[:12] + B.ids(2))
                claim = dict(chained=0, kept=0, mm=26)
            else:
                t = seq(s[:30] + B.ids(2))
                claim = dict(chained=1, kept=30, mm=26)
            ti = B.target(t)
            if rank in (0, first, 62, 63, 64, 65, 126, 127, 128, 129):
                B.c.claims.append(("c%d_h%d_r%d" % (n, first, rank), qs[0], ti, dict(rank=rank, **claim)))
    return B.done()


def _case_width(n_seed_ids):
    """a round of 16 384 seeds (query bitsets of 256 words: staged in LDS) and of 16 448 (257 words: read from global memory); the
    pairs of the perfect-chain case with their seed ids spread over the whole range, the last id included"""
    c = _case_perfect()
    used = c.n_seed_ids
    step = (n_seed_ids - 1) // (used - 1)
    remap = lambda sg: [v if i % 2 == 0 else (n_seed_ids - 1 - (used - 1 - v) * step) for i, v in enumerate(sg)]
    c.index = [remap(t) for t in c.index]
    c.queries = [remap(q) for q in c.queries]
    c.n_seed_ids = n_seed_ids
    c.name = "width_%d" % n_seed_ids
    return c


def _case_neg_gaps():
    """first and last gaps below zero (overlapping seeds at a chunk's edge) on both sides: target_anchor is a sum that starts with them"""
    B = _Builder("neg_gaps", hf=0.25)
    for first, last in ((-3, -5), (-9, 0), (0, -9), (-1, -1)):
        s = B.ids(20)
        B.pair("neg_%d_%d" % (-first, -last), seq(s, first=first, last=last), seq(B.ids(2) + s + B.ids(2), gaps=[-2, -4] + [10] * 19 + [-3, -6], first=first, last=last), kept=20)
    return B.done()


SWEEP_SEED = 20260
SWEEP_HIT_FRACTIONS = (0.03, 0.05, 0.12)  # minMatches 0 .. 2, 1 .. 4, 1 .. 10 over queries of 10 .. 80 seeds


def _case_sweep(hf):
    """300 random repetitive pairs: an alphabet of 3 to 6 seeds (every pair its own ids), 10 to 80 seeds a side"""
    B = _Builder("sweep_%g" % hf, hf=hf)
    rng = np.random.default_rng(SWEEP_SEED)
    for i in range(300):
        al = B.ids(int(rng.integers(3, 7)))
        a = rng.choice(al, int(rng.integers(10, 81)))
        b = rng.choice(al, int(rng.integers(10, 81)))
        ga = rng.integers(0, 40, len(a) - 1).tolist()
        gb = rng.integers(0, 40, len(b) - 1).tolist()
        B.query(seq(a, gaps=ga))
        B.target(seq(b, gaps=gb))
    return B.done()


_BUILDERS = {
    "sizes": _case_sizes,
    "links": _case_links,
    "kept_wide": _case_kept_wide,
    "redbuf500_at": lambda: _case_redbuf("redbuf500_at", 500, 255, 249, 0),
    "redbuf500_over": lambda: _case_redbuf("redbuf500_over", 500, 255, 250, 1),
    "redbuf500_lane_over": lambda: _case_redbuf("redbuf500_lane_over", 500, 300, 250, 1),
    "redbuf1500_over": lambda: _case_redbuf("redbuf1500_over", 1500, 760, 750, 1),
    "results_at": lambda: _case_results("results_at", 500),
    "results_over": lambda: _case_results("results_over", 501),
    "results_lane_over": lambda: _case_results("results_lane_over", 501, filler=100),
    "pool_at": lambda: _case_pool("pool_at", 10183),
    "pool_over": lambda: _case_pool("pool_over", 10184),
    "nodes_at": lambda: _case_nodes("nodes_at", 65000),
    "nodes_over": lambda: _case_nodes("nodes_over", 65535),
    "perfect": _case_perfect,
    "perfect_clamp": lambda: _case_perfect(k=4, name="perfect_clamp"),
    "dups": _case_dups,
    "ratchet_steps": _case_ratchet,
    "ratchet_stale": _case_ratchet_stale,
    "many": _case_many,
    "width_16384": lambda: _case_width(16384),
    "width_16448": lambda: _case_width(16448),
    "neg_gaps": _case_neg_gaps,
}
CASE_NAMES = tuple(_BUILDERS)
#: the cases whose call must fail with DP_ERR_CAPACITY, and the bit
ERROR_CASES = {"redbuf500_over": 1, "redbuf500_lane_over": 1, "redbuf1500_over": 1, "results_over": 4, "results_lane_over": 4, "pool_over": 2}

_cases, _oracle, _profiles = {}, {}, {}


def case(name):
    if name not in _cases:
        if name.startswith("sweep_"):
            _cases[name] = _case_sweep(float(name[6:]))
        elif name == "many_grow":
            _cases[name] = _case_many(copies=9, name="many_grow")
        else:
            _cases[name] = _BUILDERS[name]()
    return _cases[name]


def oracle(name):
    """the case on the oracle, once per process, never changed afterwards"""
    if name not in _oracle:
        c = case(name)
        r = O.find_overlaps_segments(c.index, c.queries, c.n_seed_ids, c.hf, c.k, c.max_length)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _oracle[name] = r
    return _oracle[name]


def pair_row(name, q, t):
    """the oracle's row (dict of PAIR_COLS) of pair (query q, target t), or None when the loop never reached it"""
    for row in oracle(name)["pairs"]:
        if row[0] == q and row[2] == t:
            return dict(zip(O.PAIR_COLS, (int(x) for x in row)))
    return None


def anchors(c, res):
    """GetSeedOffset(first matched target seed), GetSeedOffsetFromEnd(last one) of every match of an oracle result, from the segments"""
    out = []
    for i in range(len(res["target"])):
        sg = np.asarray(c.index[int(res["target"][i])], dtype=np.int64)
        first, last = int(res["match_b"][res["off"][i]]), int(res["match_b"][res["off"][i + 1] - 1])
        out.append((int(sg[0] + (sg[2:2 * first + 1:2] + c.k).sum()), int(sg[-1] + (sg[2 * last + 2:len(sg) - 1:2] + c.k).sum())))
    return out


# --------------------------------------------------------------------------------------------- the path the capacities predict
def _profile(c, q, t, mm):
    key = (c.name, q, t, mm)
    if key not in _profiles:
        _profiles[key] = O.pairwise_profile(c.queries[q], c.index[t], mm, c.k, c.max_length)
    return _profiles[key]


def fits_slim(c, q, t, mm):
    """does chain_pair<CSlim> chain this pair (else it answers -1 and the pair is left to the full layout)"""
    aN, bN = len(c.queries[q]), len(c.index[t])
    if aN > CAPS["SLIM_ACAP"] or bN > CAPS["C_BCAP"]:
        return False
    ms, p = _profile(c, q, t, mm)
    if p["aLen"] > CAPS["SLIM_RSEEDS"] or p["limit"]:
        return False
    if p["initialSize"] == 0:
        return True  # (no initial position: answered before the events are counted)
    return p["bEvents"] <= CAPS["SLIM_EVN"] and p["peakOpen"] <= CAPS["SLIM_ROWS"] and p["longestChain"] <= CAPS["SLIM_COLN"]


def full_tier(c, q, t, mm):
    """usedTier of chain_pair<CWave> with no tier forced"""
    aN, bN = len(c.queries[q]), len(c.index[t])
    if aN > CAPS["C_ACAP"] or bN > CAPS["C_BCAP"]:
        return 3
    ms, p = _profile(c, q, t, mm)
    if p["aLen"] > CAPS["REG_ALEN"]:
        return 2
    if p["initialSize"] == 0:
        return 1
    if p["bEvents"] > CAPS["C_REV"] or p["peakOpen"] > CAPS["REG_ROWS"]:
        return 2
    return 1


def _kept_len(c, q, t, mm):
    ms, p = _profile(c, q, t, mm)
    return len(ms[-1][0]) if ms else 0  # (matchWorker keeps the last match of the reversed list: results[0])


def predict_paths(name, passes):
    """The path word (dp_debug_chain_paths) of every pair of a case that finishes, under the default settings with `passes` proposal
    passes: the stage's protocol (walk 0 on the slim layout, `passes` times proposals + resolve, the final walk on the
    full layout) replayed with the oracle as the chainer and CAPS as the only knowledge of the layouts.  -> {(query, target): path}"""
    c, res = case(name), oracle(name)
    out = {}
    for q in range(len(c.queries)):
        cands = [int(x) for x in res["cand"][res["cand_off"][q]:res["cand_off"][q + 1]]]
        if not cands:
            continue
        qseeds = set(c.queries[q][1::2])
        cs = [len(qseeds & set(c.index[t][1::2])) for t in cands]
        mm = _mm(c.hf, len(c.queries[q]) // 2)
        spec = [None] * len(cands)  # proposal: (mm, len) or "marked"
        nxt = 0

        def ratchet(mm, ln):
            return (ln * 2) // 3 if ln > 0 and ln * 2 > mm * 3 else mm
        # walk 0 (slim): up to and including the first pair it chains; a pair that needs the full layout stops it
        while nxt < len(cands):
            t = cands[nxt]
            if cs[nxt] < mm:
                out[(q, t)] = K_WALK0 << 8
                nxt += 1
                continue
            if not fits_slim(c, q, t, mm):
                spec[nxt] = "marked"
                break
            out[(q, t)] = (K_WALK0 << 8) | P_CHAINED | P_SLIM | 1
            mm = ratchet(mm, _kept_len(c, q, t, mm))
            nxt += 1
            break
        for ps in range(passes):
            for i in range(nxt, len(cands)):  # chain_spec_kernel
                if spec[i] == "marked" or (spec[i] is not None and spec[i][0] == mm):
                    continue
                if cs[i] < mm:
                    spec[i] = (mm, 0)
                elif fits_slim(c, q, cands[i], mm):
                    spec[i] = (mm, _kept_len(c, q, cands[i], mm))
                else:
                    spec[i] = "marked"
            while nxt < len(cands):  # chain_resolve_query
                t = cands[nxt]
                if cs[nxt] < mm:
                    out[(q, t)] = (K_RESOLVE0 + ps) << 8
                elif spec[nxt] == "marked" or spec[nxt][0] != mm:
                    break
                else:
                    out[(q, t)] = ((K_RESOLVE0 + ps) << 8) | P_CHAINED | P_SLIM | 1
                    mm = ratchet(mm, spec[nxt][1])
                nxt += 1
        while nxt < len(cands):  # the final walk (full layout)
            t = cands[nxt]
            marked = P_MARKED if spec[nxt] == "marked" else 0
            if cs[nxt] < mm:
                out[(q, t)] = (K_FINAL << 8) | marked
            elif spec[nxt] not in (None, "marked") and spec[nxt][0] == mm:
                out[(q, t)] = (K_FINAL << 8) | P_CHAINED | P_SLIM | 1
                mm = ratchet(mm, spec[nxt][1])
            else:
                out[(q, t)] = (K_FINAL << 8) | P_CHAINED | marked | full_tier(c, q, t, mm)
                mm = ratchet(mm, _kept_len(c, q, t, mm))
            nxt += 1
    return out
