"""dp_reads_replace_tail_packed_rc held to a fresh upload: context A gets head + batch in one dp_reads_upload_packed_rc, context B the
head (with another first batch) and then the tail replace; every device read of B, the read count and the base count must be A's.
Then what the head is for - its chunk scan - before and after a replace, and the contract with borrowing contexts: stale until
dp_ctx_refresh_shared, then the owner's view of the new reads, seeds and index untouched."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGE_LENS = [1, 3, 4, 15, 16, 17, 63, 64, 65] + list(range(208, 224))  # ... and every len % 16


def _reads(rng, lens):
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(n))] for n in lens]


def _pack_block(reads):
    """The host layout of dp_reads_upload_packed_rc: 2 bits per base, first base in a byte's top bits, every read on a 16-byte boundary."""
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    poff = np.concatenate([[0], np.cumsum(((lens.astype(np.int64) + 3) // 4 + 15) & ~15)])
    blk = np.zeros(int(poff[-1]), dtype=np.uint8)
    for r, b in enumerate(reads):
        n = len(b)
        if not n:
            continue
        codes = (((b >> 1) ^ ((b & 4) >> 2)) & 3).astype(np.uint8)
        codes = np.concatenate([codes, np.zeros((-n) % 4, dtype=np.uint8)]).reshape(-1, 4)
        by = (codes[:, 0] << 6) | (codes[:, 1] << 4) | (codes[:, 2] << 2) | codes[:, 3]
        blk[poff[r]:poff[r] + len(by)] = by
    return blk, lens


def _counts(c):
    return int(c.L.dp_reads_count(c.h)), int(c.L.dp_reads_total_bases(c.h))


def _all_reads(c):
    return [bytes(c.packed_read(d)) for d in range(_counts(c)[0])]


@pytest.fixture(scope="module")
def fresh():
    """context A: re-uploaded whole for every comparison"""
    import downpore_amd
    c = downpore_amd.Context(0)
    yield c
    c.close()


def _want(fresh, head, batch):
    blk, lens = _pack_block(head + batch)
    fresh.upload_reads_packed_rc(blk, lens, len(head), pinned=True)
    return _all_reads(fresh), _counts(fresh)


def _check(b, fresh, head, batch, what):
    want, wc = _want(fresh, head, batch)
    got = _all_reads(b)
    assert _counts(b) == wc, what
    assert len(got) == len(want) == len(head) + 2 * len(batch), what
    bad = [d for d in range(len(want)) if got[d] != want[d]]
    assert not bad, (what, bad[:8])


@pytest.mark.parametrize("keep,head_lens", [(0, []), (1, [64]), (1, [65]), (2, [63, 0]), (2, [4000, 128]), (5, [61, 64, 67, 129, 1])])
def test_tail_replace_equals_a_fresh_upload(fresh, keep, head_lens):
    """every keep, head byte sizes on both sides of a 16-byte step (64 bases = 16 bytes, 65 = 17 -> 32), a batch larger than the one before
    (the growth copy), a smaller one, an equal one and an empty one"""
    import downpore_amd
    rng = np.random.default_rng(100 + keep + sum(head_lens))
    head = _reads(rng, head_lens)
    assert len(head) == keep
    b = downpore_amd.Context(0)
    try:
        first = _reads(rng, [40, 7, 300])
        blk, lens = _pack_block(head + first)
        b.upload_reads_packed_rc(blk, lens, keep, pinned=True)
        head_before = [bytes(b.packed_read(d)) for d in range(keep)]
        batches = [("edge lengths, larger", EDGE_LENS + list(rng.integers(1, 3000, 40))),
                   ("smaller", [17, 5, 64]),
                   ("equal", [17, 5, 64]),
                   ("empty", []),
                   ("larger again", list(rng.integers(1, 5000, 90))),
                   ("one base", [1])]
        for what, bl in batches:
            batch = _reads(rng, bl)
            pk, ln = _pack_block(batch)
            b.replace_tail_packed_rc(keep, pk, ln, pinned=(what != "equal"))  # (once from pageable memory: the staged copy)
            assert [bytes(b.packed_read(d)) for d in range(keep)] == head_before, what
            _check(b, fresh, head, batch, what)
    finally:
        b.close()


def test_ten_batches_in_a_row(fresh):
    import downpore_amd
    rng = np.random.default_rng(9)
    head = _reads(rng, [20001, 2000])
    b = downpore_amd.Context(0)
    try:
        blk, lens = _pack_block(head)
        b.upload_reads_packed_rc(blk, lens, 2, pinned=True)
        for i in range(10):
            n = 110 if i % 2 == 0 else 9
            batch = _reads(rng, rng.integers(1, 2500 if i % 2 == 0 else 90, n))
            pk, ln = _pack_block(batch)
            b.replace_tail_packed_rc(2, pk, ln)
            _check(b, fresh, head, batch, "batch %d" % i)
    finally:
        b.close()


def test_argument_errors_touch_nothing():
    import downpore_amd
    from downpore_amd.hip import DpError
    rng = np.random.default_rng(2)
    reads = _reads(rng, [100, 200, 300])
    b = downpore_amd.Context(0)
    try:
        blk, lens = _pack_block(reads)
        b.upload_reads_packed_rc(blk, lens, 1, pinned=True)
        before, cb = _all_reads(b), _counts(b)
        assert cb[0] == 5
        pk, ln = _pack_block(reads[:1])
        with pytest.raises(DpError, match="keep 6"):
            b.replace_tail_packed_rc(6, pk, ln)
        with pytest.raises(DpError, match="length out of range"):
            b.replace_tail_packed_rc(1, pk, np.array([0x80000000], dtype=np.uint32))
        assert _all_reads(b) == before and _counts(b) == cb
        b.replace_tail_packed_rc(5, pk, ln)  # keep == dp_reads_count: the batch is appended
        assert _counts(b)[0] == 7 and _all_reads(b)[:5] == before
    finally:
        b.close()


@pytest.fixture(scope="module")
def genome_case():
    """a 150 kb reference with its join chunk as the head, seeds, its chunk items, and two batches of reads"""
    from tests import oracle_lib as O
    G, k = 150000, 11
    genome = np.frombuffer(O.gen_genome(21, G), dtype=np.uint8)
    join = np.concatenate([genome[-1000:], genome[:1000]])
    rng = np.random.default_rng(21)
    seeds = np.unique(rng.integers(0, 4 ** k, 60000).astype(np.uint32))
    items = [(0, s, 10000 - k + 1, 0) for s in range(0, G - 10000, 9000)] + [(1, 0, 2000 - k + 1 - 4, 0)]
    batches = []
    for seed, n in ((31, 60), (32, 100)):
        bases, off = O.gen_reads(seed, G, n, 3000, 0.05, True)
        batches.append([np.array(bases[off[i]:off[i + 1]], dtype=np.uint8) for i in range(n)])
    return dict(k=k, head=[genome, join], seeds=seeds, items=np.array(items, dtype=np.uint32), batches=batches)


def _same_scan(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("n_seeds", "seg_off", "segs"))


def test_head_chunk_scan_survives_a_replace(genome_case):
    import downpore_amd
    g = genome_case
    b = downpore_amd.Context(0)
    try:
        blk, lens = _pack_block(g["head"] + g["batches"][0])
        b.upload_reads_packed_rc(blk, lens, 2, pinned=True)
        b.round_begin(g["k"], g["seeds"])
        before = b.scan(g["items"])
        assert before["n_seeds"].sum() > 1000
        for batch in (g["batches"][1], g["batches"][0][:5], []):
            pk, ln = _pack_block(batch)
            b.replace_tail_packed_rc(2, pk, ln)
            assert _same_scan(b.scan(g["items"]), before)
    finally:
        b.close()


def test_borrowers_are_stale_until_refreshed(genome_case):
    import downpore_amd
    from downpore_amd.hip import DpError
    g = genome_case
    k = g["k"]
    own = downpore_amd.Context(0)
    w = None
    try:
        blk, lens = _pack_block(g["head"] + g["batches"][0][:4])
        own.upload_reads_packed_rc(blk, lens, 2, pinned=True)
        own.round_begin(k, g["seeds"])
        chunks = own.scan(g["items"])
        w = downpore_amd.Context(0, shared_from=own)
        w.read_len = np.array(own.read_len)
        w.round_begin(k, g["seeds"])
        w.import_segments(chunks["segs"])
        w.index_build(chunks["seg_off"][:-1], chunks["n_seeds"])
        info = w.index_info()
        assert info["layout"] == "dense" and info["n_seqs"] == len(g["items"])
        # a batch many times the size of the first: the packed block moves
        batch = g["batches"][1]
        pk, ln = _pack_block(batch)
        own.replace_tail_packed_rc(2, pk, ln)
        new_read = 2 + 2 * 57  # forward strand of batch read 57: no such device read before the replace
        win = np.array([(new_read, 0, len(batch[57]) - k + 1, 0), (new_read + 1, 0, len(batch[57]) - k + 1, 0)], dtype=np.uint32)
        for call in (lambda: w.scan(win), lambda: w.scan(g["items"][:1]), lambda: w.packed_read(0)):
            with pytest.raises(DpError, match=r"error -3: .*dp_ctx_refresh_shared"):
                call()
        w.refresh_shared(own)
        assert _counts(w) == _counts(own)
        got, want = w.scan(win), own.scan(win)
        assert want["n_seeds"].sum() > 10 and _same_scan(got, want)
        assert bytes(w.packed_read(new_read + 1)) == bytes(own.packed_read(new_read + 1))
        after = w.index_info()
        assert after == info
        assert w.n_seeds == len(g["seeds"])
        assert _same_scan(w.scan(g["items"]), chunks)  # (the round's seeds and the head, through the borrower)
    finally:
        if w is not None:
            w.close()
        own.close()
