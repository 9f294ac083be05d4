"""Crafted inputs for dp_map_windows' relaunch paths (tests/test_gpu_map_windows.py, tests/test_map_windows_model.py): an index
of hand-made chunks and a batch of window pairs for which no reads exist - the expected chains come from tests/map_model.py.

Every case holds the same skeleton, 130 chunks in two 64-chunk-aligned shards ([0, 64) and [64, 130)):
  chunks 0 - 15, 70, 71   "multi" chunks: the seeds of all D repeated windows one after another, so every repeated window chains
                          with each of them (16 chains from the first shard, 2 from the second, the ratchet carried across)
  chunks 20, 21, 22, 23   the ratchet-sensitive pair's targets (below)
  chunks 30, 31           (case "big" only) targets of the BIG window
  the rest                decoys of five private seeds each
and a batch of P window pairs dealt round robin from the D repeated windows (forward window real, its reverse complement without
seeds), with the ratchet-sensitive pair in the middle of the batch:
  forward window A, 40 seeds; t0 = chunk 20 holds every fourth of them at the same places: a candidate (10 of 40 sets, minCount
  10 -> the 8-ladder), prefilter count 10 >= minMatches 8, a chain of 10 (limit 8: no ratchet); t1 = chunk 21 holds all 40: a chain
  of 40 that raises minMatches AND minRCMatches to 32.  A launch that starts from thresholds an earlier launch of the same call
  has raised drops t0 (10 < 32).  t3 = chunk 23 holds A's first 32 seeds: its count EQUALS the raised threshold - kept, a chain
  of 32 (CountIntersectionTo(.., min) < min drops, == does not).  Its reverse window B, 40 other seeds; t2 = chunk 22 holds every fourth: count 10 reaches B's
  own threshold 8 but not the 32 the forward chain left: dropped by the reference too (the forward-raises-reverse rule).
Cases: "big" (a window of 300 seeds against a chunk that shares them all - a reduced window beyond the kernel's 256 - and a chunk
of 2 400 reduced seeds - beyond its 2 048: the BIG variant runs again over the batch), "records" (more than 65 536 chains, fewer
than 2 097 152 chain ints), "ints" (more than 2 097 152 chain ints, fewer than 65 536 chains)."""
import numpy as np

K = 11
GAP = 20          # bases between two seeds of a window
SPLIT = 64        # first chunk of the second shard
N_CHUNKS = 130
T0, T1, T2, T3 = 20, 21, 22, 23
BIG_Q, BIG_T = 30, 31
MULTI = list(range(16)) + [70, 71]


def seg_of(seeds, gap=GAP, first=3, last=4):
    s = [first]
    for x in seeds:
        s += [int(x), gap]
    s[-1] = last
    return s


def seg_len(seg, k=K):
    """bases a segment array spans: its gaps plus k per seed"""
    return int(sum(seg[0::2])) + (len(seg) // 2) * k


def build(case):
    """-> dict(k, n_seeds, chunks, w_segs, w_off, w_len, split, sensitive_pair, distinct)"""
    D, n, P = {"big": (4, 25, 9), "records": (24, 25, 4200), "ints": (12, 200, 700)}[case]
    nxt = [0]

    def fresh(m):
        nxt[0] += m
        return list(range(nxt[0] - m, nxt[0]))

    A, B = fresh(40), fresh(40)
    rep = [fresh(n) for _ in range(D)]
    chunks = [None] * N_CHUNKS
    multi = seg_of([s for w in rep for s in w])
    for c in MULTI:
        chunks[c] = multi
    sub_gap = 4 * (GAP + K) - K  # every fourth seed of a window at the places the window has them
    chunks[T0] = seg_of(A[::4], gap=sub_gap)
    chunks[T1] = seg_of(A)
    chunks[T2] = seg_of(B[::4], gap=sub_gap)
    chunks[T3] = seg_of(A[:32])
    pairs = [(seg_of(w), [seg_len(seg_of(w))]) for w in rep]
    big_pair = None
    if case == "big":
        Q = fresh(300)
        chunks[BIG_Q] = seg_of(Q)
        chunks[BIG_T] = seg_of(Q * 8)
        big_pair = (seg_of(Q), [seg_len(seg_of(Q))])
    for c in range(N_CHUNKS):
        if chunks[c] is None:
            chunks[c] = seg_of(fresh(5))
    batch = [pairs[i % D] for i in range(P)]
    sensitive = P // 2
    batch.insert(sensitive, (seg_of(A), seg_of(B)))
    if big_pair:
        batch.insert(2, big_pair)
        sensitive += 1
    w_segs, w_off, w_len = [], [0], []
    for f, r in batch:
        for s in (f, r):
            w_segs.append(np.asarray(s, dtype=np.int32))
            w_off.append(w_off[-1] + len(s))
            w_len.append(seg_len(s))
    return dict(k=K, n_seeds=nxt[0], chunks=chunks, w_segs=np.concatenate(w_segs), w_off=np.array(w_off, dtype=np.uint64),
                w_len=np.array(w_len, dtype=np.uint32), split=SPLIT, sensitive_pair=sensitive, distinct=D + 1 + (1 if big_pair else 0))


# ---- the traced inputs: `map` runs of the oracle whose performMapping calls both test files replay -------------------------------
# (the parameters of tests/test_gpu_map.py's sharded cases - k = 9 makes every seed frequent, k = 13 makes them rare - with 150
# reads: 300 traced calls each)
TRACED = {"k11": dict(seed=14, G=6000000, k=11, e=0.10), "k9": dict(seed=15, G=2600000, k=9, e=0.05),
          "k13": dict(seed=13, G=1500000, k=13, e=0.0)}
TRACED_READS = 150
_RUNS = {}


def traced_inputs(name):
    """-> (reference ReadSet, reads ReadSet, k)"""
    from tests import oracle_lib as O
    p = TRACED[name]
    genome = np.frombuffer(O.gen_genome(p["seed"], p["G"]), dtype=np.uint8)
    bases, off = O.gen_reads(p["seed"], p["G"], TRACED_READS, 7000, p["e"], True)
    return (O.ReadSet(genome, np.array([0, p["G"]], dtype=np.int64), min_len=0, himem=False),
            O.ReadSet(bases, off, min_len=500, himem=False), p["k"])


def traced_run(name):
    """The oracle's traced run of input `name` (every performMapping call), once per process."""
    from tests import oracle_lib as O
    if name not in _RUNS:
        ref, reads, k = traced_inputs(name)
        _RUNS[name] = O.MapRun(ref, reads, circular=True, k=k, max_calls=1 << 20)
    return _RUNS[name]


def traced_chains(call):
    """A traced call's chains as [(strand, target, match_a, match_b)]"""
    a, ao = call["matchA"]
    b, bo = call["matchB"]
    return [(int(call["chainStrand"][i]), int(call["chainTarget"][i]), a[ao[i]:ao[i + 1]].tolist(), b[bo[i]:bo[i + 1]].tolist())
            for i in range(len(call["chainStrand"]))]
