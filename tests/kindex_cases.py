"""Crafted read sets of the k-mer position index build tests (tests/test_kindex_cases_cpu.py on the CPU, tests/test_gpu_kindex_build.py
on the device): the resident index of DESIGN.md 4.1 - dp_kbuild.hip's kb_count1, kb_part1, kb_count2, kb_part2, kb_final and the
atomic count / scatter build of dp_kindex.hip - held to a plain numpy reference bucket by bucket.  Test infrastructure only.

The reference needs no device and no oracle: with the 2-bit code A C G T = 0 1 2 3 (what tests/test_gpu_kernels.py's
test_pack_matches_reference_encoding pins), the k-mer at every start of every read of at least k bases gives a tuple
(k-mer, read, position); counts = bincount of the k-mers, off = its exclusive prefix sum, the entries are read << 32 | position sorted
by (k-mer, entry).  The order of the entries inside a bucket is free on the device, so `compare` sorts every bucket before it compares.

`geometry` restates the width rule of dp_kindex_build_sorted (position bits, read-id bits, the three digit widths, the entry format,
radix build or atomic scatter).  The CPU test places every case with it; the GPU test holds it to what dp_kindex_dump reports, so it
cannot drift unnoticed.  Everything is integer-exact.
"""
import concurrent.futures
import functools
import types

import numpy as np

KB_TILE = 16384     # dp_kbuild.hip: entries per tile of passes 1 and 2
KB_P3_CAP = 8192    # dp_kbuild.hip: entries kb_final sorts inside LDS
_LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
A, C_, G, T = 0, 1, 2, 3


def codes_of(ascii_bases):
    """the packer's 2-bit code of ASCII bases (ACGT only here)"""
    c = np.asarray(ascii_bases, dtype=np.uint8)
    return (((c >> 1) ^ ((c & 4) >> 2)) & 3).astype(np.uint8)


def unpack(packed, length):
    """codes of a read from its packed bytes (four bases a byte, the first base in the top two bits)"""
    p = np.asarray(packed, dtype=np.uint8)
    return ((p[:, None] >> np.array([6, 4, 2, 0], dtype=np.uint8)) & 3).reshape(-1)[:length].astype(np.uint8)


def to_upload(reads):
    """list of code arrays -> (ASCII bases, off) as Context.upload_reads takes them"""
    off = np.zeros(len(reads) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(r) for r in reads])
    codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]) if len(reads) else np.zeros(0, dtype=np.uint8)
    return _LETTERS[codes], off


# ------------------------------------------------------------------------------------------------------------ the reference
def reference(reads, k):
    """reads: list of code arrays (the reads as the device holds them) -> Reference"""
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    start = np.zeros(len(reads) + 1, dtype=np.int64)
    start[1:] = np.cumsum(lens)
    total = int(start[-1])
    if total >= k:
        codes = np.concatenate([np.asarray(r, dtype=np.uint8) for r in reads]).astype(np.uint32)
        km = np.zeros(total - k + 1, dtype=np.uint32)
        for j in range(k):
            km = (km << np.uint32(2)) | codes[j:total - k + 1 + j]
        read_of = np.repeat(np.arange(len(reads), dtype=np.int64), lens)[:total - k + 1]
        pos = np.arange(total - k + 1, dtype=np.int64) - start[read_of]
        ok = pos <= lens[read_of] - k  # (the k-mer lies inside its read; reads shorter than k have none)
        km, read_of, pos = km[ok], read_of[ok], pos[ok]
    else:
        km, read_of, pos = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    entries = (read_of.astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64)  # (ascending as generated)
    order = np.argsort(km, kind="stable")
    km, entries = km[order], entries[order]
    present, n_of = np.unique(km, return_counts=True)
    return Reference(k, km, entries, present.astype(np.int64), n_of.astype(np.int64))


STEP = 1 << 22  # k-mers per piece wherever a 4^k table is walked


class Reference:
    """n, kmer [n] (uint32, ascending: the bucket of every slot), entries [n] (uint64 read << 32 | position, ascending inside a
    bucket), and the two 4^k tables: counts = bincount(kmer) as uint32, off [4^k + 1] = its exclusive prefix sum as uint64.  The
    tables are kept as the k-mers that occur (present, n_of) and written out piece by piece (counts_at, off_at: off is constant
    between two k-mers that occur) - at k = 14 they are 3 GB that no comparison needs at once; .counts and .off are the whole arrays."""

    def __init__(self, k, kmer, entries, present, n_of):
        self.k, self.n, self.kmer, self.entries, self.present, self.n_of = k, len(kmer), kmer, entries, present, n_of
        self.before = np.concatenate([[0], np.cumsum(n_of)]).astype(np.uint64)  # entries in front of present[i]; [-1] = n

    def counts_at(self, lo, hi):
        """counts[lo:hi]"""
        i0, i1 = np.searchsorted(self.present, [lo, hi])
        out = np.zeros(hi - lo, dtype=np.uint32)
        out[self.present[i0:i1] - lo] = self.n_of[i0:i1]
        return out

    def off_at(self, lo, hi):
        """off[lo:hi] (hi <= 4^k + 1): off[j] = before[number of occurring k-mers below j]"""
        if hi <= lo:
            return np.zeros(0, dtype=np.uint64)
        i0, i1 = np.searchsorted(self.present, [lo, hi - 1])
        edges = np.concatenate([[lo], self.present[i0:i1] + 1, [hi]])
        return np.repeat(self.before[i0:i1 + 1], np.diff(edges))

    @functools.cached_property
    def counts(self):
        return self.counts_at(0, 4 ** self.k)

    @functools.cached_property
    def off(self):
        return self.off_at(0, 4 ** self.k + 1)

    def group_sizes(self, shift):
        """entries per value of k-mer >> shift (a first digit, a sub-partition)"""
        return np.bincount(self.present >> shift, weights=self.n_of, minlength=4 ** self.k >> shift).astype(np.int64)


def _show(a, lo, hi, limit=12):
    s = [hex(int(x)) for x in a[int(lo):int(min(hi, lo + limit))]]
    return "[" + ", ".join(s) + (", ..." if hi - lo > limit else "") + "]"


def compare(ref, n_pos, off, entries, counts=None):
    """device dump against the reference -> None when equal, else a message naming the first k-mer that differs"""
    nk = 4 ** ref.k
    if int(n_pos) != ref.n:
        return "n_pos: device %d, reference %d" % (int(n_pos), ref.n)
    off = np.asarray(off)
    if off.shape != (nk + 1,) or off.dtype != np.uint64:
        return "off: shape %s dtype %s" % (off.shape, off.dtype)
    for lo in range(0, nk + 1, STEP):
        hi = min(nk + 1, lo + STEP)
        want = ref.off_at(lo, hi)
        if not np.array_equal(off[lo:hi], want):
            km = lo + int(np.flatnonzero(off[lo:hi] != want)[0])
            a = max(km - 1, 0)
            return "off differs first at k-mer %#x: device off[%#x..] = %s, reference %s" % (km, a, off[a:km + 2].tolist(), ref.off_at(a, min(nk + 1, km + 2)).tolist())
    if counts is not None:
        counts = np.asarray(counts)
        if counts.shape != (nk,):
            return "counts: shape %s" % (counts.shape,)
        for lo in range(0, nk, STEP):
            hi = min(nk, lo + STEP)
            want = ref.counts_at(lo, hi)
            if not np.array_equal(counts[lo:hi], want):
                km = lo + int(np.flatnonzero(counts[lo:hi] != want)[0])
                return "counts differ first at k-mer %#x: device %d, reference %d" % (km, int(counts[km]), int(want[km - lo]))
    entries = np.asarray(entries)
    if entries.shape != (ref.n,) or entries.dtype != np.uint64:
        return "entries: shape %s dtype %s" % (entries.shape, entries.dtype)
    # (off is the reference's here, so the bucket of every slot - np.repeat(np.arange(nk), np.diff(off)) - is ref.kmer)
    got = entries[np.lexsort((entries, ref.kmer))]
    if not np.array_equal(got, ref.entries):
        i = int(np.flatnonzero(got != ref.entries)[0])
        km = int(ref.kmer[i])
        lo, hi = int(off[km]), int(off[km + 1])
        return ("entries differ first in the bucket of k-mer %#x = [%d, %d), at its sorted entry %d: device %s, reference %s"
                % (km, lo, hi, i - lo, _show(got, lo, hi), _show(ref.entries, lo, hi)))
    return None


# ------------------------------------------------------------------------------------------------------------ dp_kindex_digest in numpy
def _mix(x):
    """splitmix64's finaliser on a uint64 array (numpy's array arithmetic wraps)"""
    x = x ^ (x >> np.uint64(30))
    x *= np.uint64(0xbf58476d1ce4e5b9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94d049bb133111eb)
    x ^= x >> np.uint64(31)
    return x


def digest(k, off, entries, kmer_of_entry):
    """kidx_digest_kernel (dp_kindex.hip) in wrap-around uint64: [entries, sum of mix(k-mer * golden + off[k-mer]), sum over the entries
    of mix(mix(k-mer + 1) ^ entry)]; off: the array, or a Reference (read piece by piece)"""
    nk = 4 ** k
    step = 1 << 20
    off_at = off.off_at if isinstance(off, Reference) else (lambda lo, hi: off[lo:hi])

    def part(lo):
        km = np.arange(lo, min(nk, lo + step), dtype=np.uint64)
        km *= np.uint64(0x9e3779b97f4a7c15)
        km += off_at(lo, min(nk, lo + step))
        return np.add.reduce(_mix(km), dtype=np.uint64)
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        a = np.add.reduce(np.array(list(ex.map(part, range(0, nk, step))), dtype=np.uint64), dtype=np.uint64)
    b = np.add.reduce(_mix(_mix(kmer_of_entry.astype(np.uint64) + np.uint64(1)) ^ entries), dtype=np.uint64) if len(entries) else np.uint64(0)
    return [len(entries), int(a), int(b)]


# ------------------------------------------------------------------------------------------------------------ the width rule
def _tune(env, key, dflt):
    for tok in (env.get("DP_TUNE") or "").split(","):
        name, _, val = tok.partition("=")
        if name == key:
            return int(val) if val else 1
    return dflt


def geometry(k, lens, env):
    """dp_kindex_build_sorted's choice for device reads of these lengths under these settings -> namespace sorted (radix build, else the
    atomic scatter), pbits, rbits, pay, bits (= 2k + pay: an entry in flight), b1, b2, r, r_unwidened, fmt"""
    lens = np.asarray(lens, dtype=np.int64)
    fallback = types.SimpleNamespace(sorted=False, pbits=32, rbits=0, pay=0, bits=0, b1=0, b2=0, r=0, r_unwidened=0, fmt=8)
    if k < 9 or k > 14 or len(lens) == 0 or _tune(env, "kindex_atomic", 0):
        return fallback
    max_len = max(1, int(lens.max()))
    pbits = 1
    while (1 << pbits) <= max_len:
        pbits += 1
    rbits = 1
    while (1 << rbits) < len(lens):
        rbits += 1
    if env.get("DP_KB_MIN_PBITS") is not None:
        pbits = max(pbits, min(32, int(env["DP_KB_MIN_PBITS"])))
    pay = pbits + rbits
    fallback.pbits_wanted, fallback.rbits, fallback.pay, fallback.bits = pbits, rbits, pay, 2 * k + pay
    if 2 * k + pay > 64:
        return fallback
    b1 = max(6, min(10, _tune(env, "kb_b1", 8)))
    b1 = min(b1, 2 * k - 2)
    b2 = max(1, 14 - b1)
    while b2 < 10 and (int(lens.sum()) >> (b1 + b2)) > 7800:
        b2 += 1
    if b1 + b2 > 2 * k:
        b2 = 2 * k - b1
    r = r0 = 2 * k - b1 - b2
    if r > 12:
        b2 += r - 12
        r = 12
    if b2 > 10:
        return fallback
    fmt = 8 if (env.get("DP_KINDEX_WIDE") is not None or pay > 40) else 5 if pay > 32 else 4
    return types.SimpleNamespace(sorted=True, pbits=pbits, rbits=rbits, pay=pay, bits=2 * k + pay, b1=b1, b2=b2, r=r, r_unwidened=r0, fmt=fmt)


def share_digits(ref, b1, world):
    """the digit split of a build in shares (dp_kindex_build_sorted with a shard): rank q sorts the first digits
    [first[q], first[q + 1]) -> (first [world + 1], entries of every rank's share [world])"""
    per_digit = ref.group_sizes(2 * ref.k - b1)
    pre = np.concatenate([[0], np.cumsum(per_digit)])
    total, nb1 = int(pre[-1]), 1 << b1
    first = [0]
    for q in range(1, world):
        want = (total * q + world - 1) // world
        b = first[q - 1]
        while b < nb1 and pre[b] < want:
            b += 1
        first.append(b)
    first.append(nb1)
    return first, [int(pre[first[q + 1]] - pre[first[q]]) for q in range(world)]


def sub_partitions(ref, g):
    """entries of every pass-3 sub-partition (the k-mer's top b1 + b2 bits)"""
    return ref.group_sizes(g.r)


def pass1_buckets(ref, g):
    return ref.group_sizes(2 * ref.k - g.b1)


# ------------------------------------------------------------------------------------------------------------ the read sets
def _random_reads(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in rng.integers(lo, hi + 1, n)]


def _break_a_runs(read, run):
    """no `run` consecutive As: the last base of such a run becomes C (random filler that must stay out of poly-A's sub-partition)"""
    r, n = read.copy(), 0
    for i in range(len(r)):
        n = n + 1 if r[i] == A else 0
        if n == run:
            r[i], n = C_, 0
    return r


def _poly(n, unit=(A,)):
    return np.resize(np.array(unit, dtype=np.uint8), n)


def _mutated_poly_a(seed, n):
    """poly-A with a random other base every 8 to 12 bases"""
    rng = np.random.default_rng(seed)
    r = _poly(n)
    i = int(rng.integers(0, 8))
    while i < n:
        r[i] = rng.integers(1, 4)
        i += int(rng.integers(8, 13))
    return r


def _with_lengths(seed, lens):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4, int(ln)).astype(np.uint8) for ln in lens]


_EDGE_K = 10
_MANY_SHORT = [30] * 20  # twenty reads inside two 1024-base blocks of the packed layout (a read starts on a 64-base boundary)


@functools.lru_cache(maxsize=None)
def read_set(name):
    """the reads of a named set, as code arrays (never modified)"""
    k = _EDGE_K
    if name.startswith("plain"):        # plain9, plain10, plain11, plain13: random variable-length reads
        return _random_reads(100 + int(name[5:]), 120, 500, 4000)
    if name == "k14":
        return _random_reads(114, 100, 1000, 5000)
    if name == "edges_short_first":
        return _with_lengths(21, [k - 1, 0, k, k + 1, 63, 64, 65] + _MANY_SHORT + [1023, 1024, 1025, 200, 777])
    if name == "edges_short_last":
        return _with_lengths(22, [k, k + 1, 63, 64, 65, 1023, 1024] + _MANY_SHORT + [1025, 200, 777, 0, k - 1])
    if name == "edges_longest_last":
        return _with_lengths(23, [k - 1, 0, k, k + 1, 63, 64, 65] + _MANY_SHORT + [1023, 1024, 200, 777, 1025])
    if name == "maxlen_1023":           # pbits = 10: the longest read has 2^10 - 1 bases
        return _with_lengths(24, [500, 1023, 64, 1000, 1023])
    if name == "maxlen_1024":           # pbits = 11
        return _with_lengths(25, [500, 1023, 64, 1000, 1024])
    if name.startswith("count_"):       # count_1, count_2, count_3, count_256, count_257 reads: rbits 1, 1, 2, 8, 9
        return _random_reads(30 + int(name[6:]), int(name[6:]), 100, 600)
    if name == "polya_8192":            # kb_final's sub-partition 0 holds exactly KB_P3_CAP entries: the last one sorted in LDS
        return [_break_a_runs(r, 7) for r in _random_reads(41, 30, 500, 3000)] + [_poly(1033)] * 8
    if name == "polya_8193":            # ... and one more: the first one placed straight from HBM
        return read_set("polya_8192") + [_poly(10)]
    if name == "skew_many":             # ~25 000 entries of one sub-partition over many k-mers
        return _random_reads(42, 20, 500, 2000) + [_mutated_poly_a(50 + i, 3000) for i in range(30)]
    if name == "dinucleotide":
        return _random_reads(43, 20, 500, 2000) + [_poly(5000, (A, C_))] * 4 + [_poly(4001, (C_, A))]
    if name == "tile_16384":            # pass-1 bucket 0 holds exactly one tile; nearly every other bucket and sub-partition is empty
        return [_poly(1033)] * 16 + [codes_of(np.frombuffer(b"CGTACGTTGCA", dtype=np.uint8))]
    if name == "tile_16385":            # ... and one entry more: two tiles
        return [_poly(1033)] * 16 + [codes_of(np.frombuffer(b"CGTACGTTGCA", dtype=np.uint8)), _poly(10)]
    if name == "skew_share":            # four fifths of the entries under the first digit AAAA: a rank of three gets nothing
        return [_mutated_poly_a(70 + i, 3000) for i in range(20)] + [_poly(20000)] * 4 + _random_reads(44, 5, 500, 1500)
    if name == "stale_small":
        return _random_reads(45, 40, 200, 1500)
    if name == "rc":                    # forward reads; the device makes the reverse strands of reads 3 ..
        return _random_reads(46, 40, 5, 1500)
    raise KeyError(name)


_ref_cache = {}


def reference_of(name, k):
    """reference(read_set(name), k), kept for the next case of the same set and k (one at a time from k = 13 up: 0.8 GB each)"""
    key = (name, k)
    if key not in _ref_cache:
        for old in [o for o in _ref_cache if o[1] >= 13 or k >= 13]:
            del _ref_cache[old]
        _ref_cache[key] = reference(read_set(name), k)
    return _ref_cache[key]


def case(name, reads, k, env=None, **want):
    """want: what the case's name claims, proven on the CPU and asserted on the device - sorted (radix build ran), fmt, pay, bits ..."""
    return types.SimpleNamespace(name=name, reads=reads, k=k, env=dict(env or {}), want=want)


W257 = "count_257"
CASES = [
    # ---- plain
    case("plain_k9", "plain9", 9, sorted=True, fmt=4, r=4),
    case("plain_k10", "plain10", 10, sorted=True, fmt=4, r=6),
    case("plain_k11", "plain11", 11, sorted=True, fmt=4, r=8),
    case("plain_k13", "plain13", 13, sorted=True, fmt=4, r=12),
    case("k14_widened_pass2", "k14", 14, sorted=True, fmt=4, r=12, r_unwidened=14, b2=8),
    # ---- read lengths
    case("edges_short_first", "edges_short_first", 10, sorted=True, pbits=11),
    case("edges_short_last", "edges_short_last", 10, sorted=True, pbits=11),
    case("edges_longest_last", "edges_longest_last", 10, sorted=True, pbits=11),
    case("pbits_at_1023", "maxlen_1023", 10, sorted=True, pbits=10),
    case("pbits_at_1024", "maxlen_1024", 10, sorted=True, pbits=11),
    # ---- read counts
    case("reads_1", "count_1", 10, sorted=True, rbits=1),
    case("reads_2", "count_2", 10, sorted=True, rbits=1),
    case("reads_3", "count_3", 10, sorted=True, rbits=2),
    case("reads_256", "count_256", 10, sorted=True, rbits=8),
    case("reads_257", "count_257", 10, sorted=True, rbits=9),
    # ---- payload formats (257 reads: rbits = 9)
    case("pay32_fmt4_bit31", W257, 10, {"DP_KB_MIN_PBITS": "23"}, sorted=True, fmt=4, pay=32, top_bit=31),
    case("pay33_fmt5", W257, 10, {"DP_KB_MIN_PBITS": "24"}, sorted=True, fmt=5, pay=33),
    case("pay40_fmt5_bit39", W257, 10, {"DP_KB_MIN_PBITS": "31"}, sorted=True, fmt=5, pay=40, top_bit=39),
    case("pay41_fmt8", W257, 10, {"DP_KB_MIN_PBITS": "32"}, sorted=True, fmt=8, pay=41),
    case("wide_fmt8", W257, 10, {"DP_KINDEX_WIDE": "1"}, sorted=True, fmt=8),
    # ---- entry width (k = 13, 257 reads)
    case("entry_64_bits", W257, 13, {"DP_KB_MIN_PBITS": "29"}, sorted=True, bits=64, fmt=5),
    case("entry_65_bits_atomic", W257, 13, {"DP_KB_MIN_PBITS": "30"}, sorted=False, bits=65, fmt=8),
    case("atomic_by_setting", "plain10", 10, {"DP_TUNE": "kindex_atomic=1"}, sorted=False, fmt=8),
    # ---- pass-1 widths
    case("b1_6_k9", "plain9", 9, {"DP_TUNE": "kb_b1=6"}, sorted=True, b1=6, b2=8, r=4),
    case("b1_9_k9", "plain9", 9, {"DP_TUNE": "kb_b1=9"}, sorted=True, b1=9, b2=5, r=4),
    case("b1_10_k9", "plain9", 9, {"DP_TUNE": "kb_b1=10"}, sorted=True, b1=10, b2=4, r=4),
    case("b1_6_k13", "plain13", 13, {"DP_TUNE": "kb_b1=6"}, sorted=True, b1=6, b2=8, r=12),
    case("b1_9_k13", "plain13", 13, {"DP_TUNE": "kb_b1=9"}, sorted=True, b1=9, b2=5, r=12),
    case("b1_10_k13", "plain13", 13, {"DP_TUNE": "kb_b1=10"}, sorted=True, b1=10, b2=4, r=12),
    # ---- skew
    case("polya_hold_8192", "polya_8192", 10, sorted=True, largest_sub=8192),
    case("polya_nohold_8193", "polya_8193", 10, sorted=True, largest_sub=8193),
    case("skew_many_kmers", "skew_many", 10, sorted=True, largest_sub_about=25000),
    case("dinucleotide", "dinucleotide", 10, sorted=True, two_kmers=True),
    case("bucket_one_tile", "tile_16384", 10, sorted=True, bucket0=16384),
    case("bucket_two_tiles", "tile_16385", 10, sorted=True, bucket0=16385),
]
CASE = {c.name: c for c in CASES}
FMT5 = [c.name for c in CASES if c.want.get("fmt") == 5]

# settings a case must not inherit from the process
CLEAN_ENV = {"DP_SCAN_INDEX": "1", "DP_TUNE": None, "DP_KB_MIN_PBITS": None, "DP_KINDEX_WIDE": None, "DP_KINDEX_SHARD": None,
             "DP_KINDEX_MAX_K": None}


def env_of(c):
    e = dict(CLEAN_ENV)
    e.update(c.env if hasattr(c, "env") else c)
    return e
