"""A plain model of the part of mapping.performMapping (mapping/mapping.go:489-589) that the product runs on the device: what
dp_map_windows must return for a (forward, reverse-complement) window pair given as seed segments.  No GPU, no product code: it is
composed from oracle primitives that the reference's own vectors or the hand cases pin - IntSet (Add, CountIntersectionTo),
GetSharedIDs, SeedSequence.Match - plus the few lines of arithmetic in between (Matches' filter, the thresholds, the 2/3 flank
test, the 4/5 ratchets).  tests/test_map_windows_model.py holds it against the oracle's own performMapping trace; the GPU tests
use it for crafted inputs for which no reads exist.  Test infrastructure only."""
import numpy as np

from tests import oracle_lib as O


def _seed_set(seg):
    """SeedIndex.AddSequence's / performMapping's seed set of a sequence (seeds.go:272-285, mapping.go:505-510)"""
    seeds = [int(x) for x in seg[1::2]]
    s = O.IntSet(max(seeds, default=0) + 1)
    for x in seeds:
        s.add(x)
    return s


def seed_offset(seg, index, k):
    """GetSeedOffset (seeds/sequence.go:1239-1246)"""
    return int(seg[0]) + sum(int(seg[i]) + k for i in range(2, 2 * index + 1, 2))


def seed_offset_from_end(seg, index, k):
    """GetSeedOffsetFromEnd (seeds/sequence.go:1269-1276)"""
    return int(seg[-1]) + sum(int(seg[i]) + k for i in range(len(seg) - 3, 2 * index + 1, -2))


class Index:
    """The mapper's SeedIndex over `chunks` (segment arrays, seeds as ids below n_seeds): AddSequence per chunk, IndexSequences."""

    def __init__(self, chunks, n_seeds):
        self.chunks = [np.asarray(c, dtype=np.int64) for c in chunks]
        self.M = len(self.chunks)
        self.seed_sets = [_seed_set(c) for c in self.chunks]
        self.posting = [O.IntSet() for _ in range(n_seeds)]
        for i in reversed(range(self.M)):  # IndexSequences adds in descending sequence order (seeds.go:373-381)
            for s in self.chunks[i][1::2]:
                self.posting[int(s)].add(i)
        self.posting_size = [p.size() for p in self.posting]

    def matches(self, seg, hit_fraction=0.25):
        """SeedIndex.Matches (seeds.go:335-353) -> (candidate ids, sets, minCount)"""
        sets, prev = [], -1
        for s in seg[1::2]:
            s = int(s)
            if s != prev and self.posting_size[s] < self.M:
                sets.append(self.posting[s])
                prev = s
        if len(sets) < 5:
            return [], len(sets), 0
        min_count = int(hit_fraction * len(sets) + 0.5)
        return [int(x) for x in O.shared_ids(sets, min_count, True)], len(sets), min_count

    def perform(self, fwd, rc, fwd_len, rc_len, k, detail=None):
        """One performMapping call up to its sort: -> (forward candidates, reverse candidates, chains), chains = [(strand, target,
        match_a, match_b)] in append order.  detail (a dict): 'ratchet_drops' = candidates the prefilter dropped only because an
        earlier chain had raised the threshold (their count reaches the window's own threshold), 'thr' = the final thresholds."""
        segs = [np.asarray(fwd, dtype=np.int64), np.asarray(rc, dtype=np.int64)]
        lens = [int(fwd_len), int(rc_len)]
        thr = [max(5, (len(s) // 2) // 5) for s in segs]  # minMatches, minRCMatches (:494-501)
        own = list(thr)
        cands = [self.matches(s)[0] for s in segs]
        chains, drops = [], []
        for strand in (0, 1):
            q = segs[strand]
            qset = _seed_set(q)
            for t in cands[strand]:  # ascending ids
                tset = self.seed_sets[t]
                if tset.count_intersection_to(qset, thr[strand]) < thr[strand]:
                    if thr[strand] > own[strand] and tset.count_intersection(qset) >= own[strand]:
                        drops.append((strand, t))
                    continue
                for a, b in O.match(self.chunks[t], q, thr[strand], k):
                    # (the forward strand's qOffset / qInset are the reverse strand's qInset / qOffset: the same sum, :536, :576)
                    if seed_offset(q, int(a[0]), k) + seed_offset_from_end(q, int(a[-1]), k) > (lens[strand] * 2) // 3:
                        continue
                    chains.append((strand, t, [int(x) for x in a], [int(x) for x in b]))
                    limit = (len(a) * 4) // 5
                    if limit > thr[strand]:
                        thr[strand] = limit
                    if strand == 0 and limit > thr[1]:  # a forward chain also raises minRCMatches (:547-549)
                        thr[1] = limit
        if detail is not None:
            detail["ratchet_drops"] = drops
            detail["thr"] = thr
        return cands[0], cands[1], chains


def map_windows(index, w_segs, w_off, w_len, k):
    """What dp_map_windows returns for windows given as it takes them (pairs 2 i, 2 i + 1): dict(window, target, off, match_a,
    match_b) as the ABI lays them out, plus cands = every window's candidate list.  Equal window pairs are evaluated once."""
    w_segs = np.asarray(w_segs, dtype=np.int64)
    memo, window, target, lens, ma, mb, cands = {}, [], [], [], [], [], []
    for p in range((len(w_off) - 1) // 2):
        f = w_segs[int(w_off[2 * p]):int(w_off[2 * p + 1])]
        r = w_segs[int(w_off[2 * p + 1]):int(w_off[2 * p + 2])]
        key = (f.tobytes(), r.tobytes(), int(w_len[2 * p]), int(w_len[2 * p + 1]))
        if key not in memo:
            cf, cr, chains = index.perform(f, r, w_len[2 * p], w_len[2 * p + 1], k)
            memo[key] = (cf, cr, np.array([s for s, _, _, _ in chains], dtype=np.int64), np.array([t for _, t, _, _ in chains], dtype=np.int64),
                         np.array([len(a) for _, _, a, _ in chains], dtype=np.int64),
                         np.array([x for _, _, a, _ in chains for x in a], dtype=np.int64),
                         np.array([x for _, _, _, b in chains for x in b], dtype=np.int64))
        cf, cr, st, tg, ln, a, b = memo[key]
        cands += [cf, cr]
        window.append(2 * p + st)
        target.append(tg)
        lens.append(ln)
        ma.append(a)
        mb.append(b)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.int64)
    return dict(window=cat(window), target=cat(target), off=np.concatenate([[0], np.cumsum(cat(lens))]).astype(np.int64),
                match_a=cat(ma), match_b=cat(mb), cands=cands, distinct=len(memo))
