"""The oracle side of the index-build stage tests (no GPU): the case module's scanner gives what the oracle's scanner gives; its
restatement of chunkWorker's walk makes the oracle's pieces, and by the branches it reports every crafted case of tests/index_cases.py
takes the branch its name states; every case's parameters lie inside the set for which the device's walk is bounded
(dp_chunk_walk_bounded) and its chunk count inside chunk_cap_of's bound - so that tests/test_gpu_index_stage.py cannot pass on cases
that have drifted, and cannot hand the device a walk that does not end."""
import os
import re

import numpy as np
import pytest

from tests import index_cases as IC
from tests import oracle_lib as O

CSRC = os.path.join(O.ROOT, "downpore_amd", "csrc")


def _read_str(c, r):
    return c.bases[c.off[r]:c.off[r + 1]].tobytes().decode()


def _survivor_segments(e, i):
    return e.segs[e.seg_off[i]:e.seg_off[i] + 2 * e.n_seeds[i] + 1]


def test_the_mirrors_are_the_sources():
    """walk_bounded, chunk_cap_of and the constants of the case module against the text they restate"""
    hdr = open(os.path.join(CSRC, "dp_chunk_bound.h")).read()
    assert "return chunk_size >= 1 && min_seeds >= 6 && min_seeds <= 100 && overlap / 2 <= chunk_size;" in hdr
    src = open(os.path.join(CSRC, "dp_overlap.hip")).read()
    assert "if (length / chunkSize + 1 == 1 || (int)numSeeds < minSeeds * 3 || numSeeds <= 150) return 1;" in src
    assert "const int step = std::max(1, minSeeds - 5);" in src and "return (numSeeds - 150) / (uint32_t)step + 3;" in src
    assert int(re.search(r"#define IFR_SW_MAX (\d+)", src).group(1)) == IC.IFR_SW_MAX
    assert int(re.search(r"#define CK_CACHE (\d+)", src).group(1)) == IC.CK_CACHE
    assert "const uint32_t i = tile * 1024 + threadIdx.x;" in src and IC.TILE == 1024
    assert "((uint64_t)4 << 20)" in src  # the default fill: rows from 4 M seed-set words up
    for n, S in IC.DEFAULT_MODE:
        assert (n * ((S + 63) // 64) >= 4 << 20) == (n == 8192)
    # both entry points refuse before they launch or arm, the host asks the same predicate
    assert src.count("if (!dp_chunk_walk_bounded(chunk_size, overlap, min_seeds))") == 2
    host = open(os.path.join(CSRC, "host", "host_overlap.cpp")).read()
    assert host.count("dp_chunk_walk_bounded(chunkSize_, overlap_, minSeeds_)") == 2 and "minSeeds_ > 5" not in host
    assert [IC.walk_bounded(*p) for p in ((10000, 1000, 15), (80, 160, 6), (80, 161, 6), (80, 162, 6), (10000, 1000, 5), (10000, 1000, 100),
                                          (10000, 1000, 101), (0, 0, 15), (10000, 20001, 15), (10000, 20002, 15))] == \
        [True, True, True, False, False, True, False, False, True, False]


@pytest.mark.parametrize("name", IC.SMALL_NAMES + ("matrix_65x257", "matrix_513x32769", "matrix_66000x32768"))
def test_scanner_is_the_oracles(name):
    """scan_reads (every read at once) = expected_segments (the oracle's packed scanner, read by read): every read of a small case, 300
    seeded ones and the first and last of a large one"""
    c = IC.case(name)
    segs, so = IC.scan_reads(c.bases, c.off, c.k, c.seed_kmers)
    reads = np.arange(c.n_reads)
    if c.n_reads > 300:
        reads = np.unique(np.concatenate([[0, c.n_reads - 1], np.random.default_rng(3).choice(c.n_reads, 300, replace=False)]))
    tables = IC.seed_tables(c.k, c.seed_kmers)
    for r in reads:
        want = IC.expected_segments(_read_str(c, r), c.k, c.seed_kmers, tables=tables)
        assert np.array_equal(segs[so[r]:so[r + 1]], want), (name, "read", int(r))


@pytest.mark.parametrize("name", IC.SMALL_NAMES)
def test_case_is_where_its_name_says(name):
    c, e = IC.case(name), IC.expected(name)
    assert IC.walk_bounded(c.chunk_size, c.overlap, c.min_seeds) and c.scan_min in (0, 1)
    length = np.diff(c.off)
    taken = {}
    for i, r in enumerate(e.read):
        r = int(r)
        pieces, br = IC.walk(_survivor_segments(e, i), int(length[r]), c.inset, c.chunk_size, c.overlap, c.min_seeds, c.k)
        assert pieces == e.pieces_of[r].tolist(), (name, "read", r, "the restated walk and the oracle disagree")
        assert "sparse_backup" not in br and "ran_out" not in br
        assert len(pieces) <= IC.chunk_cap_of(int(e.n_seeds[i]), int(length[r]), c.chunk_size, c.min_seeds), (name, "read", r)
        taken[r] = (br, len(pieces))
    assert c.claims, name
    for r, (claim, chunks) in c.claims.items():
        br, n = taken[r]
        assert claim <= br, (name, "read", r, "claimed", sorted(claim), "took", sorted(br))
        assert chunks is None or chunks == n, (name, "read", r, "claimed", chunks, "pieces, made", n)
    assert e.n_chunks <= e.cap and (c.n_chunks is None or c.n_chunks == e.n_chunks)


def test_what_the_names_promise_beyond_branches():
    # the bound is nearly met, every piece advances one seed
    e = IC.expected("at_the_bound")
    assert (e.n_chunks, e.cap) == (251, 253) and np.all(np.diff(e.chunks[:250, 1]) == 1) and np.all(e.chunks[:250, 2] == 6)
    # the sparse stretches: pieces are skipped (first seeds jump by more than a piece holds)
    for name in ("sparse_stretch", "sparse_stretch_long"):
        ch = IC.expected(name).chunks
        assert np.any(ch[1:, 1] > ch[:-1, 1] + ch[:-1, 2]), name
    # every remainder of the tail's eight-at-a-time sum, and of sixteen
    t = IC.expected("dense_tails").chunks
    tails = t[3::4]
    assert sorted(set((tails[:, 2] - 1) % 16)) == list(range(16)) and len(tails) == 18
    # a seed twice inside one chunk; seeds shared by consecutive chunks of a read
    c, e = IC.case("repeats"), IC.expected("repeats")
    first = e.chunks[0]
    ids = e.segs[2 * first[1] + 1:2 * (first[1] + first[2]) + 1:2]
    assert len(set(ids.tolist())) < len(ids)
    assert e.chunks[1, 1] < e.chunks[0, 1] + e.chunks[0, 2]
    # non-zero inset reaches whole reads only; the scan's own min_seeds drops nothing here (every read holds a seed)
    e0, e1 = IC.expected("together"), IC.expected("together_inset")
    assert np.array_equal(e0.chunks[:, :5], e1.chunks[:, :5]) and set(np.unique(e1.chunks[:, 5] - e0.chunks[:, 5])) == {0, 37}
    assert len(IC.expected("together_scan_min1").read) == 8
    # survivors that make no chunk stay survivors: the cap (and W) is larger than the exact count
    assert len(e0.read) == 8 and len(e0.pieces_of[2]) == 0
    # 1, 2, 3, 4 chunks side by side in one wave
    e = IC.expected("cache_side_by_side")
    per = np.bincount(e.chunks[:, 0], minlength=64)
    assert len(e.read) == 64 and sorted(set(per.tolist())) == [1, 2, 3, 4]
    assert all(sorted(per[i:i + 4].tolist()) == [1, 2, 3, 4] for i in range(0, 64, 4))
    # tiles: a read of four chunks on both sides of every boundary of 1 024 survivors
    c, e = IC.case("tiles"), IC.expected("tiles")
    assert len(e.read) == 2500 == c.n_reads
    per = np.bincount(e.chunks[:, 0], minlength=2500)
    assert [int(per[i]) for i in (0, 1023, 1024, 2047, 2048, 2499)] == [4] * 6
    assert set(np.delete(per, (0, 1023, 1024, 2047, 2048, 2499)).tolist()) == {0, 1} and e.cap > e.n_chunks + 64


def test_chained_rounds_are_where_their_labels_say():
    """the rounds of the chained-launch test against the sizes dp_index_prechain_launch guesses from the previous round: 1.25 x its
    chunk bound + 64, max(4 096, 1.5 x its survivors) survivors; and the index step before it must itself hold (1.5 x the hits)"""
    src = open(os.path.join(CSRC, "dp_overlap.hip")).read()
    assert "(((u64)ctx->pc_prev_cap + ctx->pc_prev_cap / 4 + 64) + 63) & ~63ull" in src
    assert "std::max<uint32_t>(4096u, ctx->pc_prev_ns + ctx->pc_prev_ns / 2)" in src
    prev = None
    for label, lo, hi, announce, with_extra, chained, bound in IC.CHAINED_ROUNDS:
        e = IC.expected("chained", lo, hi)
        ns, hits = len(e.read), int(e.n_seeds.sum())
        if prev is None:
            assert bound == "exact" and chained == 0
        else:
            p_cap, p_ns, p_hits = prev
            fits = e.cap <= IC.chain_guess(p_cap) and ns <= max(4096, p_ns + p_ns // 2)
            assert (bound == "guess") == (fits and announce), label
            if label.startswith("bound_outgrown"):
                assert e.cap > IC.chain_guess(p_cap) and ns <= 4096 and hits < p_hits + p_hits // 2, label
            if label == "survivors_outgrown":
                assert e.cap <= IC.chain_guess(p_cap) and ns > max(4096, p_ns + p_ns // 2), label
        prev = (e.cap, ns, hits)
    assert sum(r[4] for r in IC.CHAINED_ROUNDS) == 1 and IC.CHAINED_ROUNDS[-1][3] is False and IC.CHAINED_ROUNDS[-2][6] == "guess"


@pytest.mark.parametrize("name", IC.MATRIX_NAMES + IC.BIG_NAMES + IC.DEFAULT_MODE_NAMES)
def test_matrix_case_has_its_size(name):
    c, e = IC.case(name), IC.expected(name)
    n, S = (int(x) for x in name[7:].split("x"))
    assert IC.walk_bounded(c.chunk_size, c.overlap, c.min_seeds)
    # whole-read chunks: exactly n, and the bound the matrices are sized from is n as well (W = ceil(n / 64))
    assert (c.n_reads, e.n_chunks, e.cap, c.n_seeds) == (n, n, n, S)
    assert np.array_equal(e.chunks[:, 0], np.arange(n)) and np.all(e.chunks[:, 1] == 0)
    # the first and the last seed are held, the last one by the last chunk
    assert e.meta[0, 0] > 0 and e.meta[S - 1, 0] > 0 and e.seedset_row(n - 1, (S + 63) // 64)[(S - 1) // 64] >> np.uint64((S - 1) % 64) & np.uint64(1)
    if S >= 4096 and n <= 8192:
        assert (e.meta[:, 0] == 0).sum() > S // 8, "most seeds of a large set occur in no read"
        assert np.array_equal(np.unique(e.meta[e.meta[:, 0] == 0], axis=0), [[0, 1, 0, 1]])
    assert ((S + 63) // 64 > IC.IFR_SW_MAX) == (S == 32769)
    assert int(e.meta[:, 0].sum()) == len(e.e_seed)


def test_random_walks_stay_inside_the_bound():
    """a few thousand random segment arrays with parameters inside the bounded set: the restated walk ends, makes the oracle's pieces,
    and their number is within chunk_cap_of"""
    rng = np.random.default_rng(20261)
    k = 13
    sparse = 0
    for it in range(3000):
        min_seeds = int(rng.choice([6, 7, 10, 15, 40, 100]))
        chunk_size = int(rng.choice([60, 200, 1000, 10000]))
        overlap = int(rng.integers(0, 2 * chunk_size + 2))
        assert IC.walk_bounded(chunk_size, overlap, min_seeds)
        n = int(rng.integers(1, 700))
        style = it % 4
        if style == 0:
            g = rng.integers(-5, 40, n + 1)
        elif style == 1:
            g = rng.integers(0, 3, n + 1)
        elif style == 2:
            g = np.where(rng.random(n + 1) < 0.1, rng.integers(0, 3 * chunk_size, n + 1), rng.integers(0, 20, n + 1))
        else:
            g = rng.integers(0, max(2, 2 * chunk_size // max(1, min_seeds)), n + 1)
        seg = np.zeros(2 * n + 1, dtype=np.int64)
        seg[0::2] = g
        seg[1::2] = rng.integers(0, 50, n)
        length = int(seg[0::2].sum() + n * k)
        if length < 1:
            continue
        pieces, br = IC.walk(seg, length, 0, chunk_size, overlap, min_seeds, k)
        want = IC.oracle_chunks(seg, length, 0, chunk_size, overlap, min_seeds, k)
        assert pieces == want.tolist(), (it, chunk_size, overlap, min_seeds)
        assert len(pieces) <= IC.chunk_cap_of(n, length, chunk_size, min_seeds), (it, chunk_size, overlap, min_seeds, n)
        assert "sparse_backup" not in br
        sparse += "sparse" in br
    assert sparse > 100


def test_outside_the_set_the_walk_need_not_end():
    """why the library refuses: five seeds a chunk and min_seeds = 5 - the back-up of five seeds undoes every piece"""
    seg = IC.gaps((90, 400))
    segs = [7]
    for i, g in enumerate(seg):
        segs += [i, g]
    segs += [400, 20]
    assert not IC.walk_bounded(500, 1000, 5)
    with pytest.raises(AssertionError, match="the walk does not end"):
        IC.walk(segs, sum(segs[0::2]) + 401 * 13, 0, 500, 1000, 5, 13)
