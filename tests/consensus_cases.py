"""Inputs and oracle-side expectations of the consensus stage tests (tests/test_oracle_window_trace.py on the CPU,
tests/test_gpu_consensus_stage.py on the device): the traced rounds, the capacities of the device layouts, and generated groups
for the alignment kernel.  Test infrastructure only.
"""
import re
import types

import numpy as np

from tests import oracle_lib as O

K = 10
MIN_LEN = 1000

#: one traced round each (k = 10, min_len = 1000): gen_reads arguments, OverlapRun parameters
CASES = {
    # at most 29 matches a window; most windows fit the small layout, a hundred and a half need the large one, one the huge one
    "ordinary": ((8, 40000, 300, 4000, 0.05, True), {}),
    # more than 64 sequences, trimmed ints beyond every layout, consensus beyond CONS, query seeds past the small layout's 128
    "deep": ((7, 12000, 160, 4000, 0.01, False), {}),
    # query windows of up to 325 seeds: past every layout's 256
    "long": ((5, 60000, 300, 8000, 0.0, False), dict(overlap_size=3000, num_seeds=45)),
    # 32796 seeds: the small layout (int16 seed ids) is switched off, seed ids run beyond 2^15.  794 reads is the fewest that
    # keeps the round above 32767 seeds (792: 32420, 790: 32560, 780: 32599; the count is not monotonic in the reads)
    "seeds_over": ((5, 300000, 794, 5000, 0.0, False), dict(seed_batch_size=40000)),
    # 32711 seeds: the small layout runs with its largest ids
    "seeds_under": ((5, 300000, 797, 5000, 0.0, False), dict(seed_batch_size=40000)),
}
SEED_COUNTS = {"seeds_over": 32796, "seeds_under": 32711}

#: capacities of the three LDS layouts of consensus_full_kernel (dp_consensus.hip, CFCfg): ints of the trimmed sequences (T), of
#: their Reduced() forms (R), of the consensus (CONS), seeds of the forward query (A), matches of the window (M); every layout
#: holds 64 sequences.  The small one also needs every seed id of the round below 2^15.
LAYOUTS = {
    "small": dict(T=2048, R=2048, CONS=256, A=128, M=128),
    "large": dict(T=4096, R=4096, CONS=1024, A=256, M=256),
    "huge": dict(T=12288, R=12288, CONS=1024, A=256, M=256),
}
MAX_SEQS = 64
#: group records' reason codes (dp_group_meta.reserved with flag == 1) that name a capacity
CAPACITY_REASONS = {1, 4, 6, 8, 9}

_cache = {}


def oracle_case(name):
    """The case's round on the oracle, once per process: reads (those of at least min_len, as the oracle numbers them), the trace
    fields the device calls need, and the round's output by window."""
    if name in _cache:
        return _cache[name]
    gen, kw = CASES[name]
    bases, off = O.gen_reads(*gen)
    ln = np.diff(off)
    keep = np.flatnonzero(ln + 1 >= MIN_LEN)  # (a line counts with its newline: sequence/seqio.go)
    kb = np.concatenate([bases[off[i]:off[i + 1]] for i in keep])
    koff = np.concatenate([[0], np.cumsum(ln[keep])]).astype(np.int64)
    rs = O.ReadSet(bases, off, min_len=MIN_LEN)
    assert len(rs) == len(keep)
    run = O.OverlapRun(rs, k=K, max_rounds=1, traces=True, **kw)
    assert run.rounds == 1
    c = types.SimpleNamespace(name=name, k=K, overlap_size=kw.get("overlap_size", 1000), run=run, bases=kb, off=koff)
    c.read_of_name = {"r%07d" % int(i): n for n, i in enumerate(keep)}
    c.seed_kmers = run.trace(0, "seedKmers")
    c.qsegs, c.qoffs = run.trace(0, "querySegments")
    c.isegs, c.ioffs = run.trace(0, "indexedSegments")
    c.metas = np.zeros(len(c.ioffs) - 1, dtype=[("read", np.uint32), ("length", np.int32), ("offset", np.int32), ("inset", np.int32)])
    c.metas["read"] = run.trace(0, "indexedIds")
    c.metas["length"] = run.trace(0, "indexedLength")
    c.metas["offset"] = run.trace(0, "indexedOffset")
    c.metas["inset"] = run.trace(0, "indexedInset")
    c.rc_of = rc_table(c.seed_kmers, K)
    w = run.trace_windows(0)
    c.stats, c.lines, c.ignores = w["stats"], w["lines"], w["ignores"]
    c.n_windows = len(c.stats)
    assert c.n_windows * 2 == len(c.qoffs) - 1
    c.query_seeds = (np.diff(c.qoffs)[0::2] // 2).astype(np.int64)  # seeds of every window's forward query
    c.recs = [parse_lines(c, ls) for ls in c.lines]
    m = re.search(r"bad_back_suppressed=(\d+) empty_match_panics_avoided=(\d+)", run.err)
    c.bad_back, c.empty_match = int(m.group(1)), int(m.group(2))
    _cache[name] = c
    return c


def rc_table(seed_kmers, k):
    """SeedIndex.seedOfRcKmer for every seed: the id of the seed's reverse-complement k-mer, or 0 where that is no seed."""
    km = np.asarray(seed_kmers, dtype=np.int64)
    rc = np.zeros_like(km)
    x = km.copy()
    for _ in range(k):
        rc = (rc << 2) | (3 - (x & 3))
        x >>= 2
    ids = {int(v): i for i, v in enumerate(km)}
    return np.array([ids.get(int(v), 0) for v in rc], dtype=np.int32)


PAF_FIELDS = ("q_read", "t_read", "q_len", "q_start", "q_end", "t_len", "t_start", "t_end", "ident", "minus")


def parse_lines(c, lines):
    """The ten numbers of dp_paf_rec from the oracle's PAF text of one window: int64 [lines, 10] in PAF_FIELDS order."""
    out = np.zeros((len(lines), len(PAF_FIELDS)), dtype=np.int64)
    for i, ln in enumerate(lines):
        f = ln.split("\t")
        assert len(f) == 12 and f[4] in "+-" and f[10:] == ["0", "255"], ln
        out[i] = [c.read_of_name[f[0]], c.read_of_name[f[5]], int(f[1]), int(f[2]), int(f[3]), int(f[6]), int(f[7]), int(f[8]),
                  int(f[9]), 1 if f[4] == "-" else 0]
    return out


def beyond(c, layout):
    """Per window: the capacities of `layout` the oracle's numbers exceed (empty tuple: the layout holds the window).  A window with
    fewer than two matches never reaches a layout."""
    L = LAYOUTS[layout]
    out = []
    for (matches, kept, trimmed, reduced, cons, parts, _, _), qs in zip(c.stats.tolist(), c.query_seeds.tolist()):
        why = []
        if matches >= 2:
            if matches > L["M"]:
                why.append("matches")
            if qs > L["A"]:
                why.append("query seeds")
            if kept > MAX_SEQS:
                why.append("sequences")
            if trimmed > L["T"]:
                why.append("trimmed ints")
            if reduced > L["R"]:
                why.append("reduced ints")
            if cons > L["CONS"]:
                why.append("consensus ints")
        out.append(tuple(why))
    return out


def split(c):
    """The smallest layout that holds each window that builds a consensus (two or more matches): dict layout / "host" -> windows.
    (The small layout also sends on windows with a value beyond 16 bits: those the oracle's counts do not show, so "small" here is an
    upper bound of what it computes and "large" a lower one.)"""
    small_ok = len(c.seed_kmers) <= 32767
    by = {"small": [], "large": [], "huge": [], "host": []}
    b = {n: beyond(c, n) for n in LAYOUTS}
    for g in range(c.n_windows):
        if c.stats[g, 0] < 2:
            continue
        for n in ("small", "large", "huge"):
            if not b[n][g] and (n != "small" or small_ok):
                by[n].append(g)
                break
        else:
            by["host"].append(g)
    return by


# ---- generated groups for dp_consensus_align -------------------------------------------------------------------------------------

def gen_group(rng, k, n_seqs, n, p=0.0, j=0, f=0.0, seed_base=0, stretch=None):
    """Sequences cut from a hidden consensus of n seeds (ids seed_base ..) with gaps 0..59, as [gap, seed, ..., gap] int lists: each
    takes a contiguous stretch of it (all of it when stretch is None, else stretch(i) -> (first, last + 1)), loses seeds with
    probability p (the gap becomes g1 + k + g2), has its gaps jittered by +-j (never below 0) and foreign seeds (ids from 2^20 on, each
    used once) inserted into its gaps with probability f."""
    gaps = rng.integers(0, 60, n + 1)
    foreign = (1 << 20) + int(rng.integers(0, 1 << 10)) * 65536
    out = []
    for i in range(n_seqs):
        a, b = (0, n) if stretch is None else stretch(i)
        seg = [int(gaps[a])]
        for x in range(a, b):
            nxt = int(gaps[x + 1])
            if rng.random() < p:
                seg[-1] += k + nxt
                continue
            if j:
                seg[-1] = max(0, seg[-1] + int(rng.integers(-j, j + 1)))
            if rng.random() < f:
                g1 = seg[-1] // 2
                seg[-1:] = [g1, foreign, seg[-1] - g1]
                foreign += 1
            seg += [seed_base + x, nxt]
        out.append(seg)
    return out


def reduce_group(seqs, k):
    """Reduced() of every sequence of a group as multiAligner.Consensus does it (seeds/alignment.go:45-57, sequence.go:85-123): seeds
    held by two or more of the sequences stay (a seed following itself among the kept ones is dropped), the gaps of dropped seeds
    merge (g1 + k + g2).  Returns (reduced sequences - [] where none of a sequence's seeds is shared - and their index maps)."""
    held = {}
    for s in seqs:
        for sd in set(s[1::2]):
            held[sd] = held.get(sd, 0) + 1
    red, maps = [], []
    for s in seqs:
        r, m, prev, offset = [], [], -1, s[0] if s else 0
        for i in range(1, len(s), 2):
            if s[i] != prev and held[s[i]] >= 2:
                r += [offset, s[i]]
                m.append(i // 2)
                offset = s[i + 1]
                prev = s[i]
            else:
                offset += s[i + 1] + k
        red.append(r + [offset] if r else [])
        maps.append(m)
    return red, maps


_groups = {}


def align_groups(k):
    """Named groups for dp_consensus_align at seed size k: name -> (Reduced() forms of the sequences, [] = no shared seed; whether the
    kernel must leave the group to the caller: more than 64 sequences or more than 6144 ints)."""
    if k in _groups:
        return _groups[k]
    rng = np.random.default_rng(1000 + k)
    raw = {}
    raw["clean3"] = gen_group(rng, k, 3, 8)
    raw["two"] = gen_group(rng, k, 2, 12, .1, 1, 0)
    raw["lossy20"] = gen_group(rng, k, 20, 40, .1, 2, .02, stretch=lambda i: _stretch(rng, 40, 12))
    raw["lossy64"] = gen_group(rng, k, 64, 30, .15, 3, .05, stretch=lambda i: _stretch(rng, 30, 10))
    raw["clean64"] = gen_group(rng, k, 64, 46)
    raw["lossy40"] = gen_group(rng, k, 40, 70, .3, 5, .1, stretch=lambda i: _stretch(rng, 70, 25))
    raw["seqs63"] = gen_group(rng, k, 63, 24, .1, 2, .02, stretch=lambda i: _stretch(rng, 24, 8))
    raw["seqs64"] = gen_group(rng, k, 64, 24, .1, 2, .02, stretch=lambda i: _stretch(rng, 24, 8))
    raw["seqs65"] = gen_group(rng, k, 65, 24, .1, 2, .02, stretch=lambda i: _stretch(rng, 24, 8))
    # exactly CA_CAP ints and one more: prefixes of one consensus, 2 * seeds + 1 ints each (every seed is held by two or more)
    raw["cap6144"] = gen_group(rng, k, 64, 60, stretch=lambda i: (0, 48 if i < 32 else 47))
    raw["cap6145"] = gen_group(rng, k, 63, 60, stretch=lambda i: (0, 49 if i < 17 else 48))
    # a sequence none of whose seeds another one holds: its reduced form is empty
    raw["empty"] = gen_group(rng, k, 5, 20, .1, 2, 0) + gen_group(rng, k, 1, 9, seed_base=5000)
    # two sequences on a stretch the other three never touch
    raw["apart"] = gen_group(rng, k, 5, 40, .05, 1, 0, stretch=lambda i: (0, 16) if i in (1, 3) else (24, 40))
    out = {}
    for name, seqs in raw.items():
        red, _ = reduce_group(seqs, k)
        out[name] = (red, len(red) > 64 or sum(len(r) for r in red) > 6144)
    assert out["empty"][0][5] == [] and all(out["empty"][0][:5])
    _groups[k] = out
    return out


def _stretch(rng, n, least):
    a = int(rng.integers(0, n - least + 1))
    return a, int(rng.integers(a + least, n + 1))
