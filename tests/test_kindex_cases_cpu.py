"""The crafted read sets of tests/kindex_cases.py are where their names say - proven without a GPU from the reference's counts and the
restated width rule of dp_kindex_build_sorted - and the comparison helper tells a wrong index from a right one."""
import time

import numpy as np
import pytest

from tests import kindex_cases as KC


def _place(c):
    reads = KC.read_set(c.reads)
    ref = KC.reference_of(c.reads, c.k)
    g = KC.geometry(c.k, [len(r) for r in reads], KC.env_of(c))
    return reads, ref, g


@pytest.mark.parametrize("name", [c.name for c in KC.CASES])
def test_case_sits_on_the_branch_it_is_named_after(name):
    c = KC.CASE[name]
    reads, ref, g = _place(c)
    w = c.want
    assert sum(len(r) for r in reads) <= 2000000
    assert ref.n == sum(max(0, len(r) - c.k + 1) for r in reads) and ref.n > 0
    assert g.sorted == w["sorted"], "radix build or atomic scatter"
    for key in ("fmt", "pay", "bits", "pbits", "rbits", "b1", "b2", "r", "r_unwidened"):
        if key in w:
            assert getattr(g, key) == w[key], (key, getattr(g, key), w[key])
    if g.sorted:
        assert g.b1 + g.b2 + g.r == 2 * c.k and g.bits <= 64
        # the largest read id in its top position reaches the entry's top payload bit where the case says so
        if "top_bit" in w:
            last = len(reads) - 1
            assert len(reads[last]) >= c.k and (last << g.pbits).bit_length() - 1 == w["top_bit"] == g.pay - 1
    subs = KC.sub_partitions(ref, g) if g.sorted else None
    if "largest_sub" in w:
        assert int(subs.max()) == w["largest_sub"] and int(subs.argmax()) == 0
        assert (w["largest_sub"] <= KC.KB_P3_CAP) == (name == "polya_hold_8192")
        assert int(np.sort(subs)[-2]) < 100, "the filler stays small beside it"
    if "largest_sub_about" in w:
        sp = int(subs.argmax())
        inside = ref.counts_at(sp << g.r, (sp + 1) << g.r)
        assert 20000 <= int(subs.max()) <= 30000 and int(subs.max()) > KC.KB_P3_CAP
        assert int((inside >= 100).sum()) >= 8, "many placement cursors run, not one"
        assert int(inside.max()) < int(subs.max()) * 3 // 4
    if "two_kmers" in w:
        ac = int("".join("01" * 5), 4)  # ACACACACAC, and CACACACACA
        ca = int("".join("10" * 5), 4)
        top = np.sort(np.argsort(ref.counts)[-2:]).tolist()
        assert top == sorted([ac, ca]) and int(ref.counts[ac]) > KC.KB_P3_CAP and int(ref.counts[ca]) > KC.KB_P3_CAP
    if "bucket0" in w:
        b = KC.pass1_buckets(ref, g)
        assert int(b[0]) == w["bucket0"]
        assert -(-w["bucket0"] // KC.KB_TILE) == (1 if name == "bucket_one_tile" else 2)
        assert int((b > 0).sum()) <= 3 and int((subs > 0).sum()) <= 4, "nearly every bucket and sub-partition is empty"
    if c.reads.startswith("edges"):
        lens = [len(r) for r in reads]
        k = c.k
        for ln in (0, k - 1, k, k + 1, 63, 64, 65, 1023, 1024, 1025):
            assert ln in lens
        assert lens.count(30) == 20
        assert (lens[0] < k) == (name == "edges_short_first" or name == "edges_longest_last")
        assert (lens[-1] < k) == (name == "edges_short_last")
        assert (lens[-1] == max(lens)) == (name == "edges_longest_last")
        if name == "edges_longest_last":
            assert int(ref.entries.max()) == ((len(lens) - 1) << 32) | (1025 - k)
    if name.startswith("pbits_at"):
        assert max(len(r) for r in reads) == (1023 if name == "pbits_at_1023" else 1024)
    if name.startswith("reads_"):
        assert len(reads) == int(name[6:])


def test_entry_width_cases_are_one_bit_apart():
    a, b = KC.CASE["entry_64_bits"], KC.CASE["entry_65_bits_atomic"]
    ga, gb = _place(a)[2], _place(b)[2]
    assert (ga.bits, ga.sorted, gb.bits, gb.sorted) == (64, True, 65, False)
    assert [_place(KC.CASE[n])[2].pay for n in ("pay32_fmt4_bit31", "pay33_fmt5", "pay40_fmt5_bit39", "pay41_fmt8")] == [32, 33, 40, 41]
    assert sorted(KC.FMT5) == ["entry_64_bits", "pay33_fmt5", "pay40_fmt5_bit39"]


def test_share_cases_have_the_shares_they_claim():
    """skew_share with three ranks: the first digit AAAA holds more than two thirds of the entries, so rank 1 gets no digit at all;
    plain10 with two ranks: both shares hold entries"""
    reads = KC.read_set("skew_share")
    g = KC.geometry(10, [len(r) for r in reads], KC.CLEAN_ENV)
    ref = KC.reference_of("skew_share", 10)
    first, sizes = KC.share_digits(ref, g.b1, 3)
    assert first == [0, 1, 1, 256] and sizes[1] == 0 and sizes[0] > 2 * ref.n // 3 and sizes[2] > 0
    assert int(KC.sub_partitions(ref, g).max()) > KC.KB_P3_CAP
    ref = KC.reference_of("plain10", 10)
    first, sizes = KC.share_digits(ref, 8, 2)
    assert min(sizes) > ref.n // 3 and sum(sizes) == ref.n


def test_every_reference_is_quick():
    sets = sorted({(c.reads, c.k) for c in KC.CASES} | {("skew_share", 10), ("stale_small", 13), ("rc", 10)})
    for name, k in sets:
        reads = KC.read_set(name)
        t0 = time.perf_counter()
        ref = KC.reference(reads, k)
        for lo in range(0, 4 ** k, KC.STEP):  # (and both tables written out once, as a comparison reads them)
            hi = min(4 ** k, lo + KC.STEP)
            assert len(ref.counts_at(lo, hi)) == hi - lo == len(ref.off_at(lo, hi))
        dt = time.perf_counter() - t0
        assert dt < 2.0, (name, k, dt)


def test_reference_is_the_plain_definition():
    """the reference's tables against bincount / cumsum, and the whole of it against a dictionary walked base by base"""
    reads = KC.read_set("edges_short_last") + [KC._poly(40)]
    k = 9
    ref = KC.reference(reads, k)
    buckets = {}
    for r, rd in enumerate(reads):
        for p in range(len(rd) - k + 1):
            km = 0
            for c in rd[p:p + k]:
                km = km * 4 + int(c)
            buckets.setdefault(km, []).append((r << 32) | p)
    assert ref.n == sum(len(v) for v in buckets.values())
    assert np.array_equal(ref.counts, np.bincount(ref.kmer, minlength=4 ** k))
    assert ref.off[0] == 0 and np.array_equal(ref.off[1:], np.cumsum(ref.counts, dtype=np.uint64))
    nk, cuts = 4 ** k, [0, 1, 7, 4 ** k // 3, 4 ** k - 1, 4 ** k]  # (the tables piece by piece, as compare reads them)
    assert np.array_equal(np.concatenate([ref.counts_at(a, b) for a, b in zip(cuts, cuts[1:])]), ref.counts)
    assert np.array_equal(np.concatenate([ref.off_at(a, b) for a, b in zip(cuts, cuts[1:] + [nk + 1])]), ref.off)
    assert int(ref.off[nk]) == ref.n and len(ref.off_at(5, 5)) == 0
    for km, v in buckets.items():
        assert ref.entries[int(ref.off[km]):int(ref.off[km + 1])].tolist() == sorted(v), km
    assert KC.codes_of(np.frombuffer(b"ACGT", dtype=np.uint8)).tolist() == [0, 1, 2, 3]
    assert KC.unpack(np.array([0x1b, 0xe4], dtype=np.uint8), 7).tolist() == [0, 1, 2, 3, 3, 2, 1]


# ---- the comparison helper against hand-made wrong inputs
@pytest.fixture(scope="module")
def small():
    ref = KC.reference(KC.read_set("stale_small"), 9)
    return ref, ref.off.copy(), ref.entries.copy(), ref.counts.copy()


def test_compare_accepts_any_order_inside_a_bucket(small):
    ref, off, ent, cnt = small
    assert KC.compare(ref, ref.n, off, ent, cnt) is None
    rng = np.random.default_rng(1)
    shuffled = ent.copy()
    for km in np.flatnonzero(ref.counts > 1)[:200]:
        lo, hi = int(off[km]), int(off[km + 1])
        shuffled[lo:hi] = rng.permutation(shuffled[lo:hi])
    assert not np.array_equal(shuffled, ent)
    assert KC.compare(ref, ref.n, off, shuffled, cnt) is None


def _two_neighbours(ref):
    kms = np.flatnonzero(ref.counts > 0)
    i = int(np.flatnonzero(np.diff(kms) == 1)[0])
    return int(kms[i]), int(kms[i + 1])


def test_compare_flags_entries_swapped_between_neighbouring_buckets(small):
    ref, off, ent, cnt = small
    a, b = _two_neighbours(ref)
    bad = ent.copy()
    i, j = int(off[a]), int(off[b])
    bad[i], bad[j] = ent[j], ent[i]
    msg = KC.compare(ref, ref.n, off, bad, cnt)
    assert msg and "k-mer %#x" % a in msg and "[%d, %d)" % (off[a], off[a + 1]) in msg


def test_compare_flags_an_offset_shifted_by_one(small):
    ref, off, ent, cnt = small
    a, _ = _two_neighbours(ref)
    bad = off.copy()
    bad[a + 1] += np.uint64(1)
    msg = KC.compare(ref, ref.n, bad, ent, cnt)
    assert msg and msg.startswith("off differs first at k-mer %#x" % (a + 1))


def test_compare_flags_a_duplicated_entry(small):
    ref, off, ent, cnt = small
    km = int(np.flatnonzero(ref.counts > 1)[0])
    bad = ent.copy()
    bad[int(off[km]) + 1] = bad[int(off[km])]
    msg = KC.compare(ref, ref.n, off, bad, cnt)
    assert msg and "k-mer %#x" % km in msg


def test_compare_flags_a_position_off_by_one(small):
    ref, off, ent, cnt = small
    bad = ent.copy()
    bad[ref.n // 2] += np.uint64(1)
    msg = KC.compare(ref, ref.n, off, bad, cnt)
    assert msg and "k-mer %#x" % int(ref.kmer[ref.n // 2]) in msg


def test_compare_flags_counts_and_sizes(small):
    ref, off, ent, cnt = small
    bad = cnt.copy()
    bad[int(ref.kmer[0])] += 1
    assert "counts differ" in KC.compare(ref, ref.n, off, ent, bad)
    assert "n_pos" in KC.compare(ref, ref.n + 1, off, ent, cnt)
    assert "entries: shape" in KC.compare(ref, ref.n, off, ent[:-1], cnt)


def test_digest_moves_with_every_word(small):
    ref, off, ent, _ = small
    d0 = KC.digest(9, off, ent, ref.kmer)
    bad = off.copy()
    bad[5] += np.uint64(1)
    assert KC.digest(9, bad, ent, ref.kmer)[1] != d0[1]
    e2 = ent.copy()
    e2[0] += np.uint64(1)
    assert KC.digest(9, off, e2, ref.kmer)[2] != d0[2]
    # the finaliser itself: splitmix64's first output for the seed 0 is mix(golden)
    assert int(KC._mix(np.array([0x9e3779b97f4a7c15], dtype=np.uint64))[0]) == 0xe220a8397b1dcdaf


def test_nothing_outside_the_tests_calls_the_dump_hook():
    """dp_kindex_dump is declared in the header, defined in dp_kindex.hip and named in hip.SYMBOLS - and used by the tests alone"""
    import glob
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = glob.glob(os.path.join(root, "integration", "**", "*"), recursive=True) + glob.glob(os.path.join(root, "downpore_amd", "**", "*"), recursive=True)
    files += [os.path.join(root, "bench.py"), os.path.join(root, "__graft_entry__.py")]
    files = [f for f in files if os.path.isfile(f) and f.endswith((".py", ".go", ".cpp", ".hpp", ".h", ".hip"))]
    assert len(files) > 30
    users = sorted(os.path.relpath(f, root) for f in files if "dp_kindex_dump" in open(f, errors="replace").read())
    assert users == [os.path.join("downpore_amd", "csrc", "dp_common.h"), os.path.join("downpore_amd", "csrc", "dp_kindex.hip"), os.path.join("downpore_amd", "hip.py")]
    import downpore_amd.hip as h
    assert open(h.__file__).read().count("dp_kindex_dump") == 1
