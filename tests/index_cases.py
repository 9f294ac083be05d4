"""Crafted reads of the index-build stage tests (tests/test_index_cases_cpu.py on the CPU, tests/test_gpu_index_stage.py on the device):
a round's index build is chunk_kernel - overlap.chunkWorker, reference overlap/overlap.go:253-318 - and the kernels
that fill the two bit matrices.  dp_index_build_chunked works from the context's last dp_scan_reads, so a case is a set of READS: random
filler with the round's seed k-mers written where the case wants them.  Test infrastructure only.

The truth of a read's segments is a plain scanner on the CPU (scan_reads; expected_segments is the oracle's scanner, read by read, and
the CPU test holds the two to each other), so a chance hit of the filler only shifts a case - and the CPU test proves that every case
still takes the branch its name states.  The expected chunks of a read are dpo_hand_chunks of the oracle on its expected segments, the
expected matrices are built here from those chunks.  Everything is integer-exact.
"""
import ctypes as C
import types

import numpy as np

from tests import oracle_lib as O

K = 13
IFR_SW_MAX = 512        # dp_overlap.hip: seed-set words a row of index_fill_rows_kernel holds in LDS (32 768 seeds)
TILE = 1024             # survivors of one workgroup of chunk_kernel
CK_CACHE = 2            # chunks of a read the count pass of chunk_kernel keeps in LDS
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.zeros(256, dtype=np.int64)
_CODE[_LETTERS] = np.arange(4)


def walk_bounded(chunk_size, overlap, min_seeds):
    """dp_chunk_walk_bounded (downpore_amd/csrc/dp_chunk_bound.h): the parameters the device accepts"""
    return chunk_size >= 1 and 6 <= min_seeds <= 100 and int(overlap / 2) <= chunk_size


def chunk_cap_of(num_seeds, length, chunk_size, min_seeds):
    """chunk_cap_of (downpore_amd/csrc/dp_overlap.hip): the bound dp_index_build_chunked sizes the chunk buffers and matrices from"""
    if length // chunk_size + 1 == 1 or num_seeds < min_seeds * 3 or num_seeds <= 150:
        return 1
    return (num_seeds - 150) // max(1, min_seeds - 5) + 3


# ------------------------------------------------------------------------------------------------------------ the CPU scanners
def seed_tables(k, seed_kmers):
    table = np.zeros(4 ** k, dtype=np.uint8)
    table[seed_kmers] = 1
    return table, {int(km): i for i, km in enumerate(seed_kmers)}


def expected_segments(read_str, k, seed_kmers, start=None, end=None, tables=None):
    """[gap, seed id, gap, ..., gap] of a read (or of its window [start, end)) by the oracle's scanner; tables: seed_tables(k,
    seed_kmers), for a caller that scans many reads of one round"""
    table, kmap = tables if tables is not None else seed_tables(k, seed_kmers)
    s = O.Seq(read_str)
    v = s.sub(0 if start is None else start, len(read_str) if end is None else end)
    seg = v.write_segments(k, table)
    seg[1::2] = [kmap[int(x)] for x in seg[1::2]]
    return seg


def scan_reads(bases, off, k, seed_kmers):
    """every read's segments at once: every k-mer position inside a read is looked up, a hit closes the running gap (which is negative
    where two hits overlap) -> (segs int64, seg_off int64 [reads + 1])"""
    off = np.asarray(off, dtype=np.int64)
    n_reads, n = len(off) - 1, len(bases)
    code = _CODE[bases]
    v = np.zeros(max(0, n - k + 1), dtype=np.int64)
    for j in range(k):
        v = (v << 2) | code[j:n - k + 1 + j]
    order = np.argsort(seed_kmers, kind="stable")
    skm = np.asarray(seed_kmers, dtype=np.int64)[order]
    at = np.minimum(np.searchsorted(skm, v), len(skm) - 1)
    pos = np.flatnonzero(skm[at] == v)
    read = np.searchsorted(off, pos, side="right") - 1
    ok = pos + k <= off[read + 1]
    pos, read = pos[ok], read[ok]
    sid = order[at[pos]]
    cnt = np.bincount(read, minlength=n_reads)
    seg_off = np.concatenate([[0], np.cumsum(2 * cnt + 1)])
    segs = np.zeros(seg_off[-1], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(cnt)])[:-1]       # ordinal of a read's first hit among all hits
    ordinal = np.arange(len(pos)) - first[read]
    rel = pos - off[read]
    prev_end = np.zeros(len(pos), dtype=np.int64)
    prev_end[1:] = rel[:-1] + k
    prev_end[ordinal == 0] = 0
    segs[seg_off[read] + 2 * ordinal] = rel - prev_end
    segs[seg_off[read] + 2 * ordinal + 1] = sid
    length = np.diff(off)
    last_end = np.zeros(n_reads, dtype=np.int64)
    last_end[read] = rel + k                                    # (ascending positions: the last hit of a read stays)
    segs[seg_off[1:] - 1] = length - last_end
    return segs, seg_off


# ------------------------------------------------------------------------------------------- chunkWorker, restated, with its branches
def walk(seg, length, inset, chunk_size, overlap, min_seeds, k):
    """overlap.go:253-318 on one read's segments -> (pieces [first seed, seeds, Len, offset, inset], set of the branches taken):
      whole_short    numChunks == 1                           whole_few      fewer than 3 minSeeds seeds
      below_min      ... and fewer than minSeeds: no piece    whole_loop     the loop's first test with prevSeedIndex == 0
      tail           the piece up to the end                  tail8 / tail1  fromEnd's sum: a gap taken eight at a time / singly
                                                                             (chunk_kernel's split of GetSeedOffsetFromEnd)
      limit100       the count stopped by seedCount == 100    by_size        ... by chunkSize bases
      piece          a piece of >= minSeeds seeds             backup5        back-up stopped by five seeds
      backup_overlap ... by overlap / 2 bases                 sparse         too few seeds inside chunkSize bases (:302-313)
      sparse_backup  ... and its back-up moved (outside walk_bounded only)"""
    seg = [int(x) for x in seg]
    n_seeds = len(seg) // 2
    nso = lambda i: seg[i * 2 + 2] + k                          # GetNextSeedOffset
    pieces, br = [], set()
    if length // chunk_size + 1 == 1 or n_seeds < min_seeds * 3:
        br.add("whole_short" if length // chunk_size + 1 == 1 else "whole_few")
        if n_seeds >= min_seeds:
            pieces.append([0, n_seeds, length, 0, inset])
        else:
            br.add("below_min")
        return pieces, br
    half = int(overlap / 2)                                     # (Go's division truncates toward zero)
    prev, total, lib_ = 0, seg[0], 0
    turns = 0
    while True:
        turns += 1
        assert turns <= 4 * n_seeds + 8, "the walk does not end"
        if prev >= n_seeds - 150:
            if prev == 0:
                br.add("whole_loop")
                pieces.append([0, n_seeds, length, 0, inset])
            else:
                br.add("tail")
                n_gaps = n_seeds - prev - 1                     # gaps fromEnd sums: chunk_kernel takes them eight at a time
                if n_gaps >= 8:                                 # (x - 14 > stop with x = n - 3, stop = 2 prev + 1) and the
                    br.add("tail8")                             # rest singly
                if n_gaps % 8:
                    br.add("tail1")
                nfg = nso(prev - 1) - k
                from_end = seg[-1] + sum(seg[x] + k for x in range(2 * prev + 2, len(seg) - 1, 2))
                lib_ += from_end + k + nfg
                pieces.append([prev, n_seeds - prev, lib_, total - nfg, 0])
            break
        count = 0
        while lib_ < chunk_size and count < 100 and prev + count < n_seeds:
            lib_ += nso(prev + count)
            count += 1
        br.add("by_size" if lib_ >= chunk_size else "limit100" if count == 100 else "ran_out")
        if count >= min_seeds:
            br.add("piece")
            nfg = nso(prev - 1) - k
            lib_ += nfg
            pieces.append([prev, count, lib_, total - nfg, length - total - lib_ + nfg])
            total += lib_ - nfg
            lib_ = 0
            prev += count
            if prev >= n_seeds:
                break
            count = 0
            while count < 5 and lib_ < half and prev > 0:
                prev -= 1
                lib_ += nso(prev)
                total -= nso(prev)
                count += 1
            br.add("backup5" if count == 5 else "backup_overlap")
            lib_ = 0
        else:
            br.add("sparse")
            prev += count
            count = 0
            while lib_ < half and prev > 0:                     # (lengthInBases is NOT reset in front of this loop, totalOffset
                prev -= 1                                       # is not advanced by the seeds skipped: both as the reference)
                lib_ += nso(prev)
                total -= nso(prev)
                count += 1
            if count:
                br.add("sparse_backup")
            lib_ = 0
    return pieces, br


_hand = None


def oracle_chunks(seg, length, inset, chunk_size, overlap, min_seeds, k):
    """dpo_hand_chunks: the pieces chunkWorker hands to AddSequence, [first seed, seeds, Len, offset, inset] each"""
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    return _oracle_chunks_at(seg.ctypes.data, len(seg), length, inset, chunk_size, overlap, min_seeds, k)


def _oracle_chunks_at(seg_addr, n_ints, length, inset, chunk_size, overlap, min_seeds, k):
    """... on the n_ints int64 at address seg_addr (a caller that walks many reads of one array)"""
    global _hand
    if _hand is None:  # (a prototype of its own: the function object of the library belongs to whoever set its argtypes)
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int,
                            C.c_void_p, C.c_int64, C.c_void_p)
        _hand = proto(("dpo_hand_chunks", O.lib()))
    assert walk_bounded(chunk_size, overlap, min_seeds), "the oracle's walk may not end either"
    cap = chunk_cap_of(n_ints // 2, length, chunk_size, min_seeds) + 8
    out = np.empty(5 * cap, dtype=np.int64)
    n = C.c_int64(0)
    rc = _hand(seg_addr, n_ints, length, 0, inset, chunk_size, overlap, min_seeds, k, out.ctypes.data, cap, C.addressof(n))
    assert rc == 0 and n.value <= cap, (rc, n.value, cap)
    return out[:5 * n.value].reshape(-1, 5)


# ----------------------------------------------------------------------------------------------------------------- the generator
def gaps(*runs):
    """[(gap, count), ...] -> the list of gaps between consecutive seeds"""
    out = []
    for g, c in runs:
        out += [g] * c
    return out


class _Builder:
    """reads as flat arrays: per planted seed (read, position, seed id), per read its length"""

    def __init__(self, name, n_seeds, chunk_size=10000, overlap=1000, min_seeds=15, inset=0, scan_min=0, k=K, seed=None):
        self.c = types.SimpleNamespace(name=name, k=k, n_seeds=n_seeds, chunk_size=chunk_size, overlap=overlap, min_seeds=min_seeds,
                                       inset=inset, scan_min=scan_min, claims={}, n_chunks=None)
        self.rng = np.random.default_rng(seed if seed is not None else sum(name.encode()) * 7919 + n_seeds)
        self.p_read, self.p_pos, self.p_sid, self.lengths = [], [], [], []
        self.n_reads = 0

    def read(self, gap_list, seeds=None, first=7, last=20, claim=None, chunks=None):
        """one read: len(gap_list) + 1 seeds (ids `seeds`, default 0, 1, 2, ... modulo the round's seeds) with these gaps between them;
        claim: branches (names of walk()) the read must take, chunks: the pieces it must make"""
        k, m = self.c.k, len(gap_list) + 1
        ids = np.arange(m) % self.c.n_seeds if seeds is None else np.asarray(seeds)
        pos = first + np.concatenate([[0], np.cumsum(np.asarray(gap_list, dtype=np.int64) + k)])
        self.many(ids[None, :], pos[None, :], np.array([pos[-1] + k + last]))
        if claim is not None or chunks is not None:
            self.c.claims[self.n_reads - 1] = (set(claim or ()), chunks)
        return self.n_reads - 1

    def many(self, ids, pos, lengths):
        """reads of the same number of seeds: ids, pos [reads, seeds], lengths [reads]"""
        ids, pos = np.asarray(ids, dtype=np.int64), np.asarray(pos, dtype=np.int64)
        r = np.repeat(np.arange(self.n_reads, self.n_reads + len(ids)), ids.shape[1])
        self.p_read.append(r)
        self.p_pos.append(pos.ravel())
        self.p_sid.append(ids.ravel())
        self.lengths.append(np.asarray(lengths, dtype=np.int64))
        self.n_reads += len(ids)

    def short(self, n, m, special=False):
        """n reads of m seeds each and 100 to 150 bases (2 <= m <= 7): one whole chunk, or none where m < min_seeds.  special: the seeds
        on the edges of the matrices' words (first, last, 63 | 64 | 65, 255 | 256 | 257) are dealt out over the reads, and the last
        read holds the last seed"""
        k, S = self.c.k, self.c.n_seeds
        ids = self.rng.integers(0, S, (n, m))
        if special and m:
            sp = np.array([s for s in (0, S - 1, 63, 64, 65, 255, 256, 257, S // 2) if 0 <= s < S])
            ids[:, 0] = sp[np.arange(n) % len(sp)]
            ids[-1, m - 1] = S - 1
            ids[0, 1] = 0
        g = self.rng.integers(0, 7, (n, m))                     # gap in front of every seed
        pos = np.cumsum(g + k, axis=1) - k + 3
        self.many(ids, pos, np.maximum(pos[:, -1] + k + self.rng.integers(2, 9, n), 100))

    def done(self, n_chunks=None):
        c, k = self.c, self.c.k
        S = c.n_seeds
        while True:                                             # distinct random k-mers
            km = np.unique(self.rng.integers(0, 4 ** k, S + S // 4 + 16))
            if len(km) >= S:
                break
        c.seed_kmers = self.rng.permutation(km)[:S].astype(np.uint32)
        lengths = np.concatenate(self.lengths)
        c.off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        c.bases = _LETTERS[self.rng.integers(0, 4, c.off[-1])]
        if self.p_read:
            r, p, s = np.concatenate(self.p_read), np.concatenate(self.p_pos), np.concatenate(self.p_sid)
            shifts = 2 * (k - 1 - np.arange(k))
            letters = _LETTERS[(c.seed_kmers[s].astype(np.int64)[:, None] >> shifts[None, :]) & 3]
            c.bases[(c.off[r] + p)[:, None] + np.arange(k)[None, :]] = letters
        c.n_reads = len(lengths)
        c.n_chunks = n_chunks
        return c


D = dict(chunk_size=10000, overlap=1000, min_seeds=15)          # the command's own parameters


def _one(name, gap_list, claim, chunks=None, seeds=None, last=20, **params):
    B = _Builder(name, len(gap_list) + 1 if seeds is None else max(seeds) + 1, **{**D, **params})
    B.read(gap_list, seeds=seeds, last=last, claim=claim, chunks=chunks)
    return B.done()


def _dense(n):
    return gaps((12, n - 1))


# one read each: (gaps, branches claimed, pieces claimed, parameters)
_WALKS = {
    "whole_short": (gaps((100, 49)), {"whole_short"}, 1, {}),
    "whole_few": (gaps((300, 43)), {"whole_few"}, 1, {}),
    "below_min": (gaps((800, 13)), {"whole_few", "below_min"}, 0, {}),
    "n150": (gaps((60, 149)), {"whole_loop"}, 1, {}),
    "n151": (gaps((60, 150)), {"limit100", "piece", "backup5", "tail", "tail8", "tail1"}, 2, {}),
    "dense400": (_dense(400), {"limit100", "piece", "backup5", "tail", "tail8", "tail1"}, 4, {}),
    "by_size": (gaps((187, 400)), {"by_size", "piece", "backup_overlap", "tail"}, 7, {}),
    "sparse_stretch": (gaps((2, 170), (40, 30), (2, 170)), {"sparse", "by_size", "piece", "tail"}, 21,
                       dict(chunk_size=200, overlap=100, min_seeds=6)),
    "sparse_stretch_long": (gaps((20, 60), (1200, 40), (20, 300)), {"sparse", "by_size", "limit100", "piece", "tail"}, 5, {}),
    # every piece holds six seeds and is followed by a back-up of five: 251 pieces against chunk_cap_of's 253.  (overlap 160, not more:
    # overlap / 2 may not exceed chunk_size on the device; five seeds are 70 bases, so the back-up is the same five seeds)
    "at_the_bound": (gaps((1, 399)), {"by_size", "piece", "backup5", "tail"}, 251, dict(chunk_size=80, overlap=160, min_seeds=6)),
}


def _case_walk(name):
    g, claim, chunks, params = _WALKS[name]
    return _one(name, g, claim, chunks, **params)


def _case_dense_tails():
    """the tail's sum from the end, eight gaps at a time and the rest singly: 114 .. 131 gaps, every remainder modulo 8 and 16"""
    B = _Builder("dense_tails", 417, **D)
    for n in range(400, 418):
        want = {"tail", "tail8"} | ({"tail1"} if (n - 286) % 8 else set())
        B.read(_dense(n), claim=want, chunks=4)
    return B.done()


def _case_repeats():
    """a seed twice inside one chunk (ids 3 and 50 again at positions 20 and 60), and seeds in the overlap of two consecutive chunks
    (the back-up of five seeds: 95 .. 99 belong to both)"""
    ids = list(range(300))
    ids[20], ids[60], ids[150] = 3, 50, 120
    return _one("repeats", _dense(300), {"limit100", "backup5", "tail"}, 3, seeds=ids, last=6000)


def _together(B):
    for name in ("whole_short", "whole_few", "below_min", "n150", "n151", "dense400", "by_size", "sparse_stretch_long"):
        g, claim, chunks, params = _WALKS[name]
        assert not params
        B.read(g, claim=claim, chunks=chunks)
    return B


def _case_together(name="together", **kw):
    # (seed: one whose filler holds no seed k-mer by chance - test_index_cases_cpu.py says so if that ever changes)
    return _together(_Builder(name, 401, seed=5, **{**D, **kw})).done()


# reads that make exactly 1, 2, 3, 4 chunks: up to CK_CACHE the write pass copies the count pass's cache, beyond it walks again
_BY_COUNT = {1: 120, 2: 245, 3: 300, 4: 400}


def _case_cache():
    """1, 2, 3 and 4 chunks side by side in one wave, in changing order: cached writes and rewalks share one prefix sum"""
    B = _Builder("cache_side_by_side", 400, **D)
    order = B.rng.permuted(np.tile(np.array([1, 2, 3, 4]), (16, 1)), axis=1).ravel()
    for n in order:
        B.read(_dense(_BY_COUNT[int(n)]), last=6000, chunks=int(n))  # (the last gap makes every read longer than chunk_size)
    return B.done(n_chunks=160)


def _mixed(B, n_reads, special):
    """n_reads reads of 100 to 150 bases, in runs of 50 alternately of seven seeds (one chunk) and of three (none), except at the
    indices of `special`: "multi" = a read of 400 seeds and four chunks, "ballast" = one of 150 seeds and one chunk"""
    nxt = 0
    for a in sorted(special) + [n_reads]:
        for lo in range(nxt, a, 50):
            B.short(min(50, a - lo), 7 if (lo // 50) % 2 == 0 else 3)
        if a < n_reads:
            if special[a] == "multi":
                B.read(_dense(400), claim={"limit100", "tail"}, chunks=4)
            else:
                B.read(_dense(150), claim={"whole_short"}, chunks=1)
        nxt = a + 1
    assert B.n_reads == n_reads
    return B


TILES_MULTI = (0, 1023, 1024, 2047, 2048, 2499)


def _case_tiles():
    """2 500 survivors, three tiles of chunk_kernel: reads that make one chunk or none, and a read of four chunks on either side of
    every tile boundary - the look-back carries them over"""
    B = _Builder("tiles", 400, chunk_size=10000, overlap=1000, min_seeds=6)
    return _mixed(B, 2500, {a: "multi" for a in TILES_MULTI}).done()


# the read set of the chained launches (dp_index_prechain): the rounds of tests/test_gpu_index_stage.py pick ranges of it
CHAINED_READS = 5400
CHAINED_MULTI = (0, 1023, 1024, 2047, 2048) + tuple(4300 + 64 * j for j in range(7)) + tuple(range(4700, 4712))
CHAINED_BALLAST = tuple(range(4301, 4321))


#: label, reads [lo, hi), dp_index_prechain called, extra items, dp_index_prechained() wanted (None: either), the returned bound
#: ("guess": sized from the previous round, the chained launch is used; "exact": no chained launch, or launched again)
CHAINED_ROUNDS = (
    ("first", 4300, 4700, True, False, 0, "exact"),                 # no round to size from
    ("same_range", 4300, 4700, True, False, 1, "guess"),
    ("bound_outgrown", 4300, 4704, True, False, None, "exact"),     # chunk bound above 1.25 x the previous one + 64
    ("bound_outgrown_again", 4300, 4712, True, False, None, "exact"),
    ("survivors_outgrown", 0, 4200, True, False, None, "exact"),    # more than max(4 096, 1.5 x previous) survivors: too few tiles
    ("extra_items", 4300, 4700, True, True, 1, "guess"),
    ("plain_after_chained", 0, 1100, False, False, 0, "exact"),
)


def chain_guess(prev_cap):
    """dp_index_prechain_launch (dp_overlap.hip): the chunk bound a chained launch is sized for"""
    return ((prev_cap + prev_cap // 4 + 64) + 63) & ~63


def _case_chained():
    B = _Builder("chained", 400, chunk_size=10000, overlap=1000, min_seeds=6)
    special = {a: "multi" for a in CHAINED_MULTI}
    special.update({a: "ballast" for a in CHAINED_BALLAST})
    return _mixed(B, CHAINED_READS, special).done()


def _case_matrix(n, S):
    """n reads of seven seeds = n whole chunks, S seeds of which the reads hold the ones on the word edges"""
    B = _Builder("matrix_%dx%d" % (n, S), S, chunk_size=10000, overlap=1000, min_seeds=6)
    B.short(n, 7, special=True)
    return B.done(n_chunks=n)


MATRIX_N = (1, 63, 64, 65, 511, 512, 513)
MATRIX_S = (1, 63, 64, 65, 255, 256, 257, 32768, 32769)
MATRIX = sorted(set([(n, 257) for n in MATRIX_N] + [(65, S) for S in MATRIX_S] + [(1, 1), (513, 32768), (513, 32769)]))
# (chunks, seeds) beyond one pass of a grid: the meta kernel's lanes stride over 66 words; more than 16 384 transpose tasks and 8 192 rows
BIG = ((4200, 300), (66000, 32768))
# dp_index_build_chunked picks the fill by size: rows from 4 M seed-set words (8 192 chunks x 512 words) up
DEFAULT_MODE = ((8192, 32768), (4096, 32768))
STALE = ((513, 32768), (65, 257))

WALK_NAMES = tuple(_WALKS)
_BUILDERS = {
    **{name: (lambda name=name: _case_walk(name)) for name in _WALKS},
    "dense_tails": _case_dense_tails,
    "repeats": _case_repeats,
    "together": _case_together,
    "together_inset": lambda: _case_together("together_inset", inset=37),
    "together_scan_min1": lambda: _case_together("together_scan_min1", scan_min=1),
    "cache_side_by_side": _case_cache,
    "tiles": _case_tiles,
    "chained": _case_chained,
}
SMALL_NAMES = tuple(_BUILDERS)
MATRIX_NAMES = tuple("matrix_%dx%d" % ns for ns in MATRIX)
BIG_NAMES = tuple("matrix_%dx%d" % ns for ns in BIG)
DEFAULT_MODE_NAMES = tuple("matrix_%dx%d" % ns for ns in DEFAULT_MODE)
ALL_NAMES = SMALL_NAMES + MATRIX_NAMES + BIG_NAMES + DEFAULT_MODE_NAMES

_cases, _expected, _scans = {}, {}, {}


def case(name):
    if name not in _cases:
        if name.startswith("matrix_"):
            n, S = name[7:].split("x")
            _cases[name] = _case_matrix(int(n), int(S))
        else:
            _cases[name] = _BUILDERS[name]()
    return _cases[name]


class Expected:
    """the oracle's answer of a case (of its reads [lo, hi) as one round), computed once and never changed"""

    def __init__(self, c, lo=0, hi=None, segs=None):
        hi = c.n_reads if hi is None else hi
        self.lo, self.hi = lo, hi
        all_segs, all_off = segs if segs is not None else scan_reads(c.bases, c.off, c.k, c.seed_kmers)
        cnt = (np.diff(all_off) - 1) // 2
        keep = np.flatnonzero(cnt[lo:hi] >= c.scan_min) + lo    # the scan's survivors, file order
        self.read = keep
        self.n_seeds = cnt[keep]
        self.seg_len = 2 * cnt[keep] + 1
        self.seg_off = np.concatenate([[0], np.cumsum(self.seg_len)])[:-1]
        self.segs = all_segs[np.repeat(all_off[keep] - self.seg_off, self.seg_len) + np.arange(self.seg_len.sum())]
        length = np.diff(c.off)
        rows = []
        self.pieces_of = {}
        all_segs = np.ascontiguousarray(all_segs, dtype=np.int64)
        base, offs, lens, cnts = all_segs.ctypes.data, all_off.tolist(), length.tolist(), cnt.tolist()
        who = []
        self.cap = 0
        for i, r in enumerate(keep.tolist()):
            p = _oracle_chunks_at(base + 8 * offs[r], offs[r + 1] - offs[r], lens[r], c.inset, c.chunk_size, c.overlap, c.min_seeds, c.k)
            self.pieces_of[r] = p
            rows.append(p)
            who.append(i)
            self.cap += chunk_cap_of(cnts[r], lens[r], c.chunk_size, c.min_seeds)
        # per chunk: survivor, first seed, seeds, length, offset, inset
        self.chunks = np.zeros((0, 6), dtype=np.int64)
        if rows:
            self.chunks = np.column_stack([np.repeat(np.array(who), [len(p) for p in rows]), np.concatenate(rows)])
        self.n_chunks = len(self.chunks)
        # the index's entries: (chunk, seed) of every seed occurrence, distinct
        ns = self.chunks[:, 2]
        start = self.seg_off[self.chunks[:, 0]] + 2 * self.chunks[:, 1] + 1
        at = np.repeat(start - 2 * (np.concatenate([[0], np.cumsum(ns)])[:-1]), ns) + 2 * np.arange(ns.sum())
        ch = np.repeat(np.arange(self.n_chunks), ns)
        pair = np.unique(ch * np.int64(c.n_seeds) + self.segs[at])
        self.e_chunk, self.e_seed = pair // c.n_seeds, pair % c.n_seeds
        S = c.n_seeds
        self.meta = np.zeros((S, 4), dtype=np.uint32)
        self.meta[:, 1], self.meta[:, 3] = 1, 1                 # NewIntSet(): start 1, end 0
        pop = np.bincount(self.e_seed, minlength=S)
        has = pop > 0
        first = np.full(S, 1 << 40)
        np.minimum.at(first, self.e_seed, self.e_chunk // 64)
        last = np.full(S, -1)
        np.maximum.at(last, self.e_seed, self.e_chunk // 64)
        self.meta[:, 0] = pop
        self.meta[has, 1], self.meta[has, 2], self.meta[has, 3] = first[has], last[has], last[has] + 1
        self._by_seed = np.argsort(self.e_seed, kind="stable")
        self._seed_at = np.concatenate([[0], np.cumsum(pop)])
        self._chunk_at = np.concatenate([[0], np.cumsum(np.bincount(self.e_chunk, minlength=self.n_chunks))])
        for a in (self.read, self.n_seeds, self.seg_off, self.segs, self.chunks, self.meta, self.e_chunk, self.e_seed):
            a.setflags(write=False)

    @staticmethod
    def _words(ids, n_words):
        w = np.zeros(n_words, dtype=np.uint64)
        np.bitwise_or.at(w, ids // 64, np.uint64(1) << (ids % 64).astype(np.uint64))
        return w

    def posting_row(self, seed, n_words):
        """the set of chunk indices that hold `seed`, as n_words words"""
        return self._words(self.e_chunk[self._by_seed[self._seed_at[seed]:self._seed_at[seed + 1]]], n_words)

    def seedset_row(self, chunk, n_words):
        return self._words(self.e_seed[self._chunk_at[chunk]:self._chunk_at[chunk + 1]], n_words)


def expected(name, lo=0, hi=None):
    """the oracle's answer for the case's reads [lo, hi) as one round"""
    c = case(name)
    key = (name, lo, c.n_reads if hi is None else hi)
    if key not in _expected:
        if name not in _scans:
            _scans[name] = scan_reads(c.bases, c.off, c.k, c.seed_kmers)
        _expected[key] = Expected(c, lo, hi, segs=_scans[name])
    return _expected[key]
