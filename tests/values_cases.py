"""Crafted k-mer count tables for the value table's 1 % cut (tests/test_values_cases_cpu.py on the CPU, tests/test_gpu_values_table.py on the
device).  Test infrastructure only.

dp_kmer_values (dp_values.hip) has two complete implementations of the cut: the histogram path (value pass with an LDS histogram of VH_BINS
bins, threshold, tie count per tile of 16 384 k-mers, tie locate, cut) for a threshold T below VH_BINS, and the sort path (radix sort, bounds,
scan of tie flags, cut) for a T beyond it.  Random read sets land wherever they land; every table here is built so that the model
(tests/values_model.py) puts T, the k-mers above it, the ties and the id X of the lowest cut tie where the case's name says, and the builder
asserts it.  A table reaches the device as sum(counts) reads of k bases (values_model.reads_of).

Merged counts are even and come in reverse-complement pairs (i, rc(i)); only a palindrome (even k) stands alone.  A tie pair splits its
T / 2 reads over both members, each with 3 or more wherever T allows, so that every tie carries a value of its own and a cut in the wrong
place changes the table.

The smallest read set with a given T holds topN * T / 4 reads (the topN highest merged counts sum to four times their reads), so the tables
with T >= 2046 at k = 9, 10 and 11 are large: 1.5, 6 and 22 million reads of k bases.

`CASES` lists (name, k); `case(name)` -> Case(name, k, counts, table, info), built once.
"""
import collections
import functools

import numpy as np

from tests import values_model as M

VH_BINS = 2048   # dp_values.hip: a T below this is found by the histogram path, one at or above it by the sort path
TILE = 16384     # dp_values.hip: k-mers per tile of the tie count / tie locate kernels (1024 threads x VH_ITEMS)
ROW = 1024       # ... per row of a tile (one k-mer per thread)
WAVE = 64
SLICE_TILES = 4  # tiles per thread of values_tie_locate_kernel at k = 13 (4096 tiles over 1024 threads)

Case = collections.namedtuple("Case", "name k counts table info")


def _craft(k, seed, T, tie_pairs, above=None, X=None, tie_pals=0, above_base=None, split_max=None, below=300, keep_first=False):
    """A table with threshold T: `tie_pairs` reverse-complement pairs (and `tie_pals` palindromes) at merged == T, `above` k-mers with
    merged > T, `below` pairs under it.  With X the tie pairs are thinned until exactly topN - above ties lie at or behind X (X itself and
    its partner always tie), and `above` is what is left of topN; keep_first: the pair of k-mer 0 ties as well."""
    rng = np.random.default_rng(seed)
    n, topN = 4 ** k, 4 ** k // 100
    rc = M.rc_ids(k).astype(np.int64)
    ids = np.arange(n, dtype=np.int64)
    lo_all = ids[ids < rc]
    pals = rng.permutation(ids[ids == rc])
    half = T // 2
    assert T % 2 == 0 and half >= 1
    used = np.zeros(n, dtype=bool)

    def take_pairs(m):
        free = lo_all[~used[lo_all]]
        lo = rng.choice(free, size=m, replace=False) if m else np.zeros(0, dtype=np.int64)
        used[lo] = True
        used[rc[lo]] = True
        return lo

    forced = []
    if X is not None:
        forced.append(min(X, int(rc[X])))
    if keep_first:
        forced.append(0)
    forced = np.array(sorted(set(forced)), dtype=np.int64)
    assert not len(forced) or (forced != rc[forced]).all()
    used[forced] = True
    used[rc[forced]] = True
    tie_lo = np.concatenate([forced, take_pairs(tie_pairs - len(forced))])
    tie_pal = pals[:tie_pals]
    used[tie_pal] = True
    pals = pals[tie_pals:]
    if X is not None:
        # ties at or behind X: the forced pairs first, then as many of the others as the quota allows
        behind = (tie_lo >= X).astype(np.int64) + (rc[tie_lo] >= X)
        quota = topN - (above if above is not None else max(1, topN // 5))
        cum = np.cumsum(behind) + int((tie_pal >= X).sum())
        keep = (behind == 0) | (cum <= quota)
        keep[:len(forced)] = True
        dropped = tie_lo[~keep]
        used[dropped] = False
        used[rc[dropped]] = False
        tie_lo = tie_lo[keep]
        cut = int(((tie_lo >= X).sum() + (rc[tie_lo] >= X).sum() + (tie_pal >= X).sum()))
        above = topN - cut
    assert above is not None and 0 <= above <= topN
    assert above % 2 == 0 or len(pals), "an odd number of k-mers above T needs a palindrome (even k)"
    ab_lo = take_pairs(above // 2)
    ab_pal = pals[:above % 2]
    used[ab_pal] = True

    counts = np.zeros(n, dtype=np.int64)
    # ties: T / 2 reads per pair, 3 or more on either member where there are 6
    if half >= 6:
        hi_split = min(half - 3, split_max if split_max is not None else half - 3)
        s = rng.integers(3, hi_split + 1, size=len(tie_lo))
    else:
        s = np.zeros(len(tie_lo), dtype=np.int64)
    swap = rng.integers(0, 2, size=len(tie_lo)).astype(bool)
    a, b = np.where(swap, rc[tie_lo], tie_lo), np.where(swap, tie_lo, rc[tie_lo])
    counts[a] = half - s
    counts[b] = s
    counts[tie_pal] = half
    # above: everything on one member
    base = above_base if above_base is not None else half
    swap = rng.integers(0, 2, size=len(ab_lo)).astype(bool)
    counts[np.where(swap, rc[ab_lo], ab_lo)] = base + 1 + rng.integers(0, 40, size=len(ab_lo))
    counts[ab_pal] = base + 1 + rng.integers(0, 40, size=len(ab_pal))
    # below: valued k-mers the cut must leave alone
    if half > 3:
        be_lo = take_pairs(min(below, int((~used[lo_all]).sum())))
        swap = rng.integers(0, 2, size=len(be_lo)).astype(bool)
        counts[np.where(swap, rc[be_lo], be_lo)] = rng.integers(3, min(half, 40), size=len(be_lo))
    return counts


def _finish(name, k, counts, check):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    table, info = M.values(counts, k)
    assert check(info, table, counts), (name, info)
    counts.setflags(write=False)
    table.setflags(write=False)
    return Case(name, k, counts, table, info)


def _tiles(k):
    return max(1, 4 ** k // TILE)


# ------------------------------------------------------------------------------------------------------------------- builders
def _edge(k, T):
    # the same draws for both levels: only the tied level differs (splits stay below 1000, the k-mers above T start at 1025 reads)
    topN = 4 ** k // 100
    if topN < 8:   # k = 4: two k-mers are cut - one palindrome above T, one tie of a pair
        above, tie_pairs = 1, 2
    else:
        above = 2 * (topN // 16)
        tie_pairs = ((topN - above) * 9 // 8 + 1) // 2
    counts = _craft(k, 100 + k, T, tie_pairs, above=above, above_base=1024, split_max=1000, below=50)
    return counts, lambda i, t, c: i["T"] == T and i["above"] > 0 and 0 < i["cut_ties"] < i["ties"]


_TIE_T = 20  # histogram path; a pair's 10 reads split 3..7


def _tie_at_positions(k):
    """name -> X for the tie-at tables of this k"""
    n, tiles = 4 ** k, _tiles(k)
    mid = tiles // 2 + 1 if tiles > 4 else 2  # a tile that is neither the first nor the last
    return collections.OrderedDict([
        ("id1", 1),
        ("tile-first", mid * TILE),
        ("tile-last", (mid - 1) * TILE + TILE - 1),
        ("row-first", (mid - 1) * TILE + 5 * ROW),
        ("row-last", (mid - 1) * TILE + 9 * ROW + ROW - 1),
        ("wave-first", 1 * TILE + 3 * ROW + 7 * WAVE),
        ("wave-last", 1 * TILE + 12 * ROW + 10 * WAVE + WAVE - 1),
        ("last-tile", n - TILE + 6 * ROW + 333),
    ])


def _tie_at(k, where):
    X = _tie_at_positions(k)[where]
    topN = 4 ** k // 100
    counts = _craft(k, 200 + k, _TIE_T, topN, X=X, keep_first=(X == 1))

    def check(i, t, c):
        ok = i["T"] == _TIE_T and i["X"] == X and i["above"] > 0 and 0 < i["cut_ties"] < i["ties"] and t[X] == 0 and c[X] >= 3
        return ok and {"id1": X == 1, "tile-first": X % TILE == 0 and X >= TILE, "tile-last": X % TILE == TILE - 1,
                       "row-first": X % ROW == 0 and X % TILE, "row-last": X % ROW == ROW - 1 and X % TILE != TILE - 1,
                       "wave-first": X % WAVE == 0 and X % ROW, "wave-last": X % WAVE == WAVE - 1 and X % ROW != ROW - 1,
                       "last-tile": X // TILE == _tiles(k) - 1}[where]
    return counts, check


def _every_tie(k, T):
    topN = 4 ** k // 100
    tie_pairs = topN // 4
    counts = _craft(k, 300 + k + T, T, tie_pairs, above=topN - 2 * tie_pairs)
    return counts, lambda i, t, c: i["T"] == T and i["cut_ties"] == i["ties"] and i["above"] > 0


def _one_tie(k, T):
    topN = 4 ** k // 100
    counts = _craft(k, 400 + k + T, T, max(2, topN // 8), above=topN - 1)
    return counts, lambda i, t, c: i["T"] == T and i["cut_ties"] == 1 and i["ties"] > 1


def _flat(k):
    return np.full(4 ** k, 5), lambda i, t, c: i["T"] == 20 and i["ties"] > 4 ** k * 9 // 10 and 0 < i["cut_ties"] < i["ties"]


def _sparse(k, exact):
    """k-mers with a count: topN - 2 of them (T = 0), or exactly topN (T = the lowest merged count); both members of every pair counted"""
    rng = np.random.default_rng(500 + k)
    n, topN = 4 ** k, 4 ** k // 100
    rc = M.rc_ids(k).astype(np.int64)
    ids = np.arange(n, dtype=np.int64)
    want = topN if exact else topN - 2
    lo = rng.choice(ids[(ids < rc) & (ids > 0)], size=want // 2, replace=False)
    counts = np.zeros(n, dtype=np.int64)
    counts[lo] = rng.integers(3, 60, size=len(lo))
    counts[rc[lo]] = rng.integers(3, 60, size=len(lo))
    if want % 2:
        counts[rng.choice(ids[ids == rc])] = 7

    def check(i, t, c):
        counted = int((c > 0).sum())
        return counted == want and not t.any() and (i["T"] > 0 and i["above"] + i["ties"] == topN if exact else i["T"] == 0)
    return counts, check


def _sort_path(k, T, tie_pals=0):
    topN = 4 ** k // 100
    above = 2 * (topN // 10)
    tie_pairs = max(((topN - above) * 21 // 20 + 1) // 2, (topN - above) // 2 + 1)
    counts = _craft(k, 600 + k, T, tie_pairs, above=above, tie_pals=tie_pals)

    def check(i, t, c):
        pal_ties = tie_pals == 0 or int(((M.merged_counts(c, k) == T) & (M.rc_ids(k) == np.arange(4 ** k))).sum()) >= tie_pals
        return i["T"] == T and T >= VH_BINS and i["ties"] >= topN // 2 and 0 < i["cut_ties"] < i["ties"] and pal_ties
    return counts, check


def _each_k(k):
    rng = np.random.default_rng(700 + k)
    n = 4 ** k
    if n <= 400000:
        counts = rng.poisson(min(40.0, 400000.0 / n), size=n)
        heavy = rng.choice(n, size=min(n // 8, 3000), replace=False)
        counts[heavy] += rng.integers(3, 60, size=len(heavy))
    else:  # (a read per k-mer is out of reach: twice topN k-mers with a count of 3 or more, so that T leaves valued k-mers under it)
        counts = np.zeros(n, dtype=np.int64)
        some = rng.choice(n, size=2 * (n // 100), replace=False)
        counts[some] = 2 + rng.geometric(0.35, size=len(some))
    return counts, lambda i, t, c: 0 < i["T"] < VH_BINS and (t > 0).sum() > 0


def _slices():
    """k = 13: about 1.3 % of the k-mers carry a merged count.  With counts of 1 and 2 no tie would have a value (a count below 3 has
    none) and the place of the cut would not show in the table, so the tied level is a count of 3 on one member of a pair (T = 6) and the
    k-mers above it count 4 to 6."""
    k, n = 13, 4 ** 13
    topN = n // 100
    rng = np.random.default_rng(801)
    ids = rng.choice(n, size=430000, replace=False)
    counts = np.zeros(n, dtype=np.uint32)
    counts[ids] = 3
    counts[ids[:40000]] = rng.integers(4, 7, size=40000)

    def check(i, t, c):
        return i["T"] == 6 and i["cut_ties"] < i["ties"] and (i["X"] // TILE) % SLICE_TILES != 0 and i["total"] < 1500000 and \
            abs((i["above"] + i["ties"]) / n - 0.013) < 0.001 and t[i["X"]] == 0 and c[i["X"]] == 3 and topN > 0
    return counts, check


CODES_K = 5


def _codes(V):
    """the largest count on a k-mer that keeps its value is V; the ten cut k-mers count more, one of them three times as much or more"""
    k, n = CODES_K, 4 ** CODES_K
    rng = np.random.default_rng(900)
    rc = M.rc_ids(k).astype(np.int64)
    ids = np.arange(n, dtype=np.int64)
    lo = rng.permutation(ids[(ids < rc) & (ids > 0)])
    counts = np.zeros(n, dtype=np.int64)
    rest = lo[6:]
    counts[rest] = rng.integers(0, min(V, 200), size=len(rest))
    counts[rc[rest]] = rng.integers(0, 4, size=len(rest))
    counts[lo[0]] = max(100000, 3 * V)
    counts[lo[1:5]] = V + 500 + np.arange(4)
    counts[rc[lo[5]]] = V

    def check(i, t, c):
        valued = t != 0
        return i["above"] + i["cut_ties"] == 10 and int(c[valued].max()) == V and int(c[~valued].max()) >= 3 * V and \
            int(c[~valued].max()) >= 100000 and valued.sum() > 100 and i["total"] == int(c.sum())
    return counts, check


# ---------------------------------------------------------------------------------------------------------------------- the list
_BUILDERS = collections.OrderedDict()


def _add(name, k, fn, *args):
    assert name not in _BUILDERS
    _BUILDERS[name] = (k, fn, args)


for _k in (4, 7, 8, 10):
    for _T in (VH_BINS - 2, VH_BINS):
        _add("edge-of-histogram-k%d-T%d" % (_k, _T), _k, _edge, _k, _T)
for _k in (8, 10):
    for _w in _tie_at_positions(_k):
        _add("tie-at-%s-k%d" % (_w, _k), _k, _tie_at, _k, _w)
for _k in (6, 8):
    for _T in (_TIE_T, VH_BINS + 52):
        _add("every-tie-falls-k%d-T%d" % (_k, _T), _k, _every_tie, _k, _T)
        _add("one-tie-falls-k%d-T%d" % (_k, _T), _k, _one_tie, _k, _T)
_add("flat-k6", 6, _flat, 6)
for _k in (6, 8):
    _add("sparse-under-topN-k%d" % _k, _k, _sparse, _k, False)
    _add("sparse-exactly-topN-k%d" % _k, _k, _sparse, _k, True)
_add("sort-path-k5", 5, _sort_path, 5, 4000)
_add("sort-path-k8-palindrome", 8, _sort_path, 8, 2600, 3)
_add("sort-path-k9", 9, _sort_path, 9, VH_BINS)
_add("sort-path-k11", 11, _sort_path, 11, VH_BINS)
for _k in range(4, 12):
    _add("each-k-k%d" % _k, _k, _each_k, _k)
_add("slices-k13", 13, _slices)
for _V in (254, 255, 65535, 65536):
    _add("codes-%d" % _V, CODES_K, _codes, _V)

CASES = [(name, k) for name, (k, _f, _a) in _BUILDERS.items()]
NAMES = [name for name, _k in CASES]
CODES = {"codes-%d" % v: v for v in (254, 255, 65535, 65536)}
SLICES = "slices-k13"


@functools.lru_cache(maxsize=None)
def _case(name):
    k, fn, args = _BUILDERS[name]
    counts, check = fn(*args)
    return _finish(name, k, counts, check)


def case(name):
    """-> Case(name, k, counts uint32 [4^k], table float64 [4^k], info); built once, read-only.  The k = 13 table is not kept."""
    if name == SLICES:
        k, fn, args = _BUILDERS[name]
        counts, check = fn(*args)
        return _finish(name, k, counts, check)
    return _case(name)


def path_of(c):
    """the path dp_kmer_values takes by its own definition: the histogram holds every T below VH_BINS"""
    return "histogram" if c.info["T"] < VH_BINS else "sort"


def first_difference(c, got):
    """None where got equals the case's table bit for bit, else a message naming the first differing id"""
    a, b = np.asarray(got).view(np.uint64), c.table.view(np.uint64)
    if a.shape == b.shape and np.array_equal(a, b):
        return None
    if a.shape != b.shape:
        return "%s: shape %s, want %s" % (c.name, a.shape, b.shape)
    i = int(np.flatnonzero(a != b)[0])
    rc = int(M.rc_ids(c.k)[i])
    m = 2 * int(c.counts[i]) if rc == i else 2 * (int(c.counts[i]) + int(c.counts[rc]))
    return "%s: %d entries differ, the first at id %d (count %d, merged %d): got %r, want %r; %r" % (
        c.name, int((a != b).sum()), i, int(c.counts[i]), m, float(np.asarray(got)[i]), float(c.table[i]), c.info)
